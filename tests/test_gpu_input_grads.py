"""Gradients with respect to the model's inputs e (edge features) and pe (positional encodings) through
GraphGatedGCNModel on the HIP path (-m gpu): against the reference's own fp64 values (tests/golden/input_grads/,
make_golden_input_grads.py), against the fp64 oracle in-test for the routes the fixtures do not take (wide layers, the
generic encoder, shuffled node / edge ids, a mini-batch sub-graph), and the guarantee that asking for them changes none
of the existing results.  Every test runs under all three matmul modes."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, _branch_exact, _check, _oracle

pytestmark = pytest.mark.gpu

INPUT_GRADS = os.path.join(GOLDEN, "input_grads")
CASES = sorted(f for f in os.listdir(INPUT_GRADS) if f.endswith(".npz"))


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    from gnnome_assembly_amd import _lib
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _model(sd, H, L, bn, dev, edge_features=2):
    import gnnome_assembly_amd as G
    m = G.GraphGatedGCNModel(1, edge_features, H, 16, L, 64, bn, 16)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(dev)


def _run(model, g, e_np, pe_np, y_np, pw, dev, inputs=True):
    """One fwd + BCE + bwd; returns (scores, {param: grad}, e.grad, pe.grad) on the host."""
    import gnnome_assembly_amd as G
    e = torch.from_numpy(e_np).to(dev).requires_grad_(inputs)
    pe = torch.from_numpy(pe_np).to(dev).requires_grad_(inputs)
    model.zero_grad(set_to_none=True)
    s = model(g, None, e, pe)
    G.BCEWithLogitsLoss(pw)(s.squeeze(-1), torch.from_numpy(y_np).to(dev)).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.cpu() for k, p in model.named_parameters() if p.grad is not None}
    return s.detach().cpu(), grads, (e.grad.cpu() if inputs else None), (pe.grad.cpu() if inputs else None)


@pytest.mark.parametrize("fname", CASES)
def test_input_grads_match_reference(fname):
    """d e_raw and d pe against the reference's fp64 autograd on every fixture (_check: GRAD_L2, or exact on the device's
    branches): the fused encoder (128, 256), the padded width (64 -> 128), LayerNorm at 32 with the generic encoder."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    dev = _dev()
    z = np.load(os.path.join(INPUT_GRADS, fname))
    H, L, seed, bn = int(z["H"]), int(z["L"]), int(z["seed"]), bool(z["batch_norm"])
    model = _model(synth.synth_state_dict(H, L, seed), H, L, bn, dev)
    g = G.AssemblyGraph(z["src"], z["dst"], int(z["n"])).to(dev)
    _, _, ge, gpe = _run(model, g, z["e_raw"], z["pe"], z["y"], float(z["pos_weight"]), dev)
    exact = lambda: _branch_exact(g, synth.synth_state_dict(H, L, seed), H, L, z["e_raw"], z["pe"], z["y"],  # noqa: E731
                                  float(z["pos_weight"]), dev, bn)
    _check(ge.numpy(), gpe.numpy(), z["grad_e_raw"], z["grad_pe"], fname, exact)


def _case(name):
    """(sd, H, L, bn, edge_features, src, dst, n, e, pe, y, pw) of an oracle-checked case."""
    from gnnome_assembly_amd import synth
    seed = 5
    H, L, bn, F = {"wide_h320": (320, 2, True, 2), "generic_encoder_f3": (128, 2, True, 3),
                   "shuffled_nodes": (128, 2, True, 2), "shuffled_edges": (256, 2, True, 2),
                   "shuffled_edges_generic": (128, 2, True, 3)}[name]
    src, dst, n = synth.make_graph(800, seed, permute_edge_ids=name.startswith("shuffled_edges"))
    inp = synth.make_inputs(src, dst, n, seed)
    sd = synth.synth_state_dict(H, L, seed, edge_features=F)
    e, pe = inp["e"], inp["pe"]
    if F != 2:
        e = np.random.default_rng(seed).normal(size=(src.size, F)).astype(np.float32)
    if name == "shuffled_nodes":
        p = np.random.default_rng(11).permutation(n).astype(np.int32)        # caller id of node v: p[v]
        src, dst = p[src], p[dst]
        pe_s = np.empty_like(pe)
        pe_s[p] = pe
        pe = pe_s
    return sd, H, L, bn, F, src, dst, n, e, pe, inp["y"], float(inp["pos_weight"])


@pytest.mark.parametrize("name", ["wide_h320", "generic_encoder_f3", "shuffled_nodes", "shuffled_edges", "shuffled_edges_generic"])
def test_input_grads_match_oracle(name):
    """Routes the fixtures do not take, against the fp64 oracle: a width above 256 (padded to 512, 256-column problems),
    the generic encoder (edge_features = 3: gemm + the gather back to edge-id order), node ids in scattered order (the
    internal renumbering: d pe must come back in the caller's numbering), edge ids out of destination order (d e_raw must
    land on the caller's edge ids) on the fused and on the generic encoder."""
    import gnnome_assembly_amd as G
    dev = _dev()
    sd, H, L, bn, F, src, dst, n, e, pe, y, pw = _case(name)
    # shuffled node ids: renumbered internally (a graph this small stays in the caller's numbering under 'auto')
    g = G.AssemblyGraph(src, dst, n, node_order="bfs" if name == "shuffled_nodes" else None).to(dev)
    if name == "shuffled_nodes":
        assert "nperm" in g.index(), "the shuffled numbering must be renumbered internally"
    if name.startswith("shuffled_edges"):
        assert not np.array_equal(g.index()["perm"].cpu().numpy(), np.arange(src.size)), "edge ids must be out of order"
    model = _model(sd, H, L, bn, dev, edge_features=F)
    _, _, ge, gpe = _run(model, g, e, pe, y, pw, dev)
    want_e, want_pe = _oracle(sd, src, dst, n, e, pe, y, pw, bn)
    _check(ge.numpy(), gpe.numpy(), want_e, want_pe, name, lambda: _branch_exact(g, sd, H, L, e, pe, y, pw, dev))


def test_frozen_model_differentiates_its_inputs_only():
    """model.requires_grad_(False) with e, pe (and x) requiring grad: the forward saves its activations all the same,
    e.grad / pe.grad match the oracle, x.grad stays None (x is dead, full_graph.py:23), no parameter gets a .grad."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    dev = _dev()
    seed, H, L = 2, 128, 2
    src, dst, n = synth.make_graph(800, seed)
    inp = synth.make_inputs(src, dst, n, seed)
    sd = synth.synth_state_dict(H, L, seed)
    model = _model(sd, H, L, True, dev).requires_grad_(False)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    x = torch.from_numpy(inp["x"]).to(dev).requires_grad_(True)
    e = torch.from_numpy(inp["e"]).to(dev).requires_grad_(True)
    pe = torch.from_numpy(inp["pe"]).to(dev).requires_grad_(True)
    s = model(g, x, e, pe)
    assert s.requires_grad
    G.BCEWithLogitsLoss(float(inp["pos_weight"]))(s.squeeze(-1), torch.from_numpy(inp["y"]).to(dev)).backward()
    assert x.grad is None
    assert all(p.grad is None for p in model.parameters())
    want_e, want_pe = _oracle(sd, src, dst, n, inp["e"], inp["pe"], inp["y"], float(inp["pos_weight"]), True)
    _check(e.grad.cpu().numpy(), pe.grad.cpu().numpy(), want_e, want_pe, "frozen",
           lambda: _branch_exact(g, sd, H, L, inp["e"], inp["pe"], inp["y"], float(inp["pos_weight"]), dev))
    # only one of the two asked for: the other stays None
    pe2 = torch.from_numpy(inp["pe"]).to(dev)
    e2 = torch.from_numpy(inp["e"]).to(dev).requires_grad_(True)
    G.BCEWithLogitsLoss(float(inp["pos_weight"]))(model(g, None, e2, pe2).squeeze(-1), torch.from_numpy(inp["y"]).to(dev)).backward()
    assert pe2.grad is None and torch.equal(e2.grad, e.grad)


def test_minibatch_subgraph_grad_lands_on_the_parents_rows():
    """A cluster.induced_subgraph of a parent whose edata['e'] / ndata['pe'] require grad: the gradient reaches the
    parent's kept rows (the sub-graph's oracle gradient there), zeros elsewhere."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import cluster, synth
    dev = _dev()
    seed, H, L = 6, 128, 2
    src, dst, n = synth.make_graph(1000, seed, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed)
    sd = synth.synth_state_dict(H, L, seed)
    model = _model(sd, H, L, True, dev)
    parent = G.AssemblyGraph(src, dst, n).to(dev)
    e_par = torch.from_numpy(inp["e"]).to(dev).requires_grad_(True)
    pe_par = torch.from_numpy(inp["pe"]).to(dev).requires_grad_(True)
    parent.edata["e"], parent.ndata["pe"] = e_par, pe_par
    parent.edata["y"] = torch.from_numpy(inp["y"]).to(dev)
    mask = torch.from_numpy(np.random.default_rng(seed).random(n) < 0.6)
    sub = cluster.induced_subgraph(parent, mask)
    eid, nid = sub.edata[cluster.EID].cpu().numpy(), sub.ndata[cluster.NID].cpu().numpy()
    assert 0 < eid.size < src.size
    s = model(sub, None, sub.edata["e"], sub.ndata["pe"])
    G.BCEWithLogitsLoss(float(inp["pos_weight"]))(s.squeeze(-1), sub.edata["y"]).backward()
    ss, sd_ = (t.cpu().numpy() for t in sub.edges())
    want_e, want_pe = _oracle(sd, ss, sd_, int(nid.size), inp["e"][eid], inp["pe"][nid], inp["y"][eid],
                              float(inp["pos_weight"]), True)
    ge, gpe = e_par.grad.cpu().numpy(), pe_par.grad.cpu().numpy()
    _check(ge[eid], gpe[nid], want_e, want_pe, "mini-batch",
           lambda: _branch_exact(sub, sd, H, L, inp["e"][eid], inp["pe"][nid], inp["y"][eid], float(inp["pos_weight"]), dev))
    dead_e = np.ones(src.size, bool)
    dead_e[eid] = False
    dead_n = np.ones(n, bool)
    dead_n[nid] = False
    assert dead_e.any() and dead_n.any()
    assert not ge[dead_e].any() and not gpe[dead_n].any()


def test_flat_gradient_fast_path_returns_input_grads():
    """The dp.FlatGradients fast path (kernels write the parameter gradients straight into the zeroed flat buffer) with
    e / pe requiring grad: the input gradients come back, bit-identical to the ordinary autograd route's, and so do the
    parameter gradients."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp, synth
    dev = _dev()
    seed, H, L = 3, 128, 3
    src, dst, n = synth.make_graph(1500, seed, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed)
    model = _model(synth.synth_state_dict(H, L, seed), H, L, True, dev)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    args = (inp["e"], inp["pe"], inp["y"], float(inp["pos_weight"]), dev)
    _, ref_g, ref_e, ref_pe = _run(model, g, *args)                       # ordinary autograd route
    model.flatten_parameters()
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    flat.zero_()
    e = torch.from_numpy(inp["e"]).to(dev).requires_grad_(True)
    pe = torch.from_numpy(inp["pe"]).to(dev).requires_grad_(True)
    G.BCEWithLogitsLoss(float(inp["pos_weight"]))(model(g, None, e, pe).squeeze(-1), torch.from_numpy(inp["y"]).to(dev)).backward()
    assert not flat.fresh, "the fast path was not taken"
    assert torch.equal(e.grad.cpu(), ref_e) and torch.equal(pe.grad.cpu(), ref_pe)
    assert all(torch.equal(p.grad.cpu(), ref_g[k]) for k, p in model.named_parameters())


@pytest.mark.parametrize("cfg", ["h128_fused", "h256_fused", "h32ln_generic", "h96_padded"])
def test_asking_for_input_grads_changes_no_existing_result(cfg):
    """Logits and every parameter gradient are bit-identical whether or not e / pe require grad, and two runs that ask
    for them are bit-identical in everything, the input gradients included."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    dev = _dev()
    H, L, bn = {"h128_fused": (128, 2, True), "h256_fused": (256, 2, True), "h32ln_generic": (32, 2, False),
                "h96_padded": (96, 2, True)}[cfg]
    seed = 9
    src, dst, n = synth.make_graph(1200, seed, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed)
    model = _model(synth.synth_state_dict(H, L, seed), H, L, bn, dev)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    args = (inp["e"], inp["pe"], inp["y"], float(inp["pos_weight"]), dev)
    s0, g0, _, _ = _run(model, g, *args, inputs=False)
    s1, g1, e1, pe1 = _run(model, g, *args, inputs=True)
    s2, g2, e2, pe2 = _run(model, g, *args, inputs=True)
    assert torch.equal(s0, s1) and torch.equal(s1, s2)
    assert g0.keys() == g1.keys() == g2.keys() and len(g0) == len(list(model.parameters()))
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
        assert torch.equal(g1[k], g2[k]), k
    assert torch.equal(e1, e2) and torch.equal(pe1, pe2)
    assert e1.abs().sum() > 0 and pe1.abs().sum() > 0
