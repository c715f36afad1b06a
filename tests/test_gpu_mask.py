"""Read-masking coverage augmentation (-m gpu): gnm_read_mask bit for bit against the numpy restatement (tests/mask_reference.py),
gnm_index_degrees against bincount, cluster.masked_subgraph against induced_subgraph of the restatement's mask, a training step
on the thinned graph (bit-identical to the same model on the explicitly built sub-graph, and within the project's logit bar --
helpers.assert_parity -- of the fp64 oracle on that sub-graph), the prefetching loader, the mini-batch composition, and the
feature switched off (launch for launch).  Integer data and same-code comparisons are exact: no tolerance but assert_parity's."""
import numpy as np
import pytest
import torch

import induce_cases as ic
import mask_reference as ref
from helpers import assert_parity

pytestmark = pytest.mark.gpu

KEY = ref.mask_key(0x5EEDC0DE12345678)
SIZES = (1, 2, 7, 8, 9, 2047, 2049, 8193, 65537)
FRACTIONS = (0.0, 0.5, 0.85, 1.0)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ---- 1. mask bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FRACTIONS)
def test_mask_bits(f):
    from gnnome_assembly_amd import engine
    dev = _dev()
    for n in SIZES:
        for epoch, gi in ((0, 0), (7, 0), (0, 3), (2 ** 32 - 1, 5)):
            got = engine.read_mask(n, f, KEY, epoch, gi, dev)
            assert got.dtype == torch.bool and tuple(got.shape) == (n,)
            raw = got.view(torch.uint8).cpu().numpy()
            assert set(np.unique(raw)) <= {0, 1}
            want = ref.read_mask(n, f, KEY, epoch, gi)
            assert np.array_equal(raw.astype(bool), want), (n, f, epoch, gi, int((raw.astype(bool) != want).sum()))


def test_mask_bits_under_another_occupancy_cap_and_in_an_unaligned_buffer():
    """One workgroup per CU (another grid), and a buffer that starts one byte past an aligned address (byte stores instead of the
    8-byte ones): the same bits, and nothing written outside the n entries."""
    from gnnome_assembly_amd import _lib, engine
    dev = _dev()
    lib = _lib.load()
    for n in SIZES:
        want = ref.read_mask(n, 0.85, KEY, 2, 1)
        try:
            _lib.check(lib.gnm_set_occupancy_cap(1), "gnm_set_occupancy_cap")
            capped = engine.read_mask(n, 0.85, KEY, 2, 1, dev).cpu().numpy()
        finally:
            _lib.check(lib.gnm_set_occupancy_cap(0), "gnm_set_occupancy_cap")
        assert np.array_equal(capped, want), n
        buf = torch.full((n + 17,), 9, dtype=torch.uint8, device=dev)
        out = buf[1:n + 1]
        assert out.data_ptr() % 8 == 1
        got = engine.read_mask(n, 0.85, KEY, 2, 1, dev, out=out)
        assert got.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert np.array_equal(host[1:n + 1].astype(bool), want) and set(np.unique(host[1:n + 1])) <= {0, 1}, n
        assert host[0] == 9 and np.all(host[n + 1:] == 9), n


# ---- 2. degrees -----------------------------------------------------------------------------------------------------------------
def _degree_parents(dev):
    for seed, n, e in ((5, 64, 256), (6, 2000, 12000)):
        src, dst, n, isolated = ic.random_graph(seed, n, e, True)
        loops = src == dst
        pairs = set(zip(src.tolist(), dst.tolist()))
        assert loops.any() and len(pairs) < len(src)                                # a self loop, a duplicate edge
        assert np.setdiff1d(np.arange(n), dst).size > len(isolated) and np.setdiff1d(np.arange(n), src).size > len(isolated)
        for node_order in ("bfs", "keep"):
            yield (seed, node_order), src, dst, n, ic.parent(src, dst, n, node_order, dev)


def test_index_degrees_equals_bincount_on_both_induce_routes():
    """A node with no in-edge, one with no out-edge, a duplicate edge and a self loop (induce_cases.random_graph), at 64 nodes /
    256 edges and at 2,000 nodes; parents with and without an internal numbering; the whole graph and a thinned one."""
    from gnnome_assembly_amd import cluster, engine
    dev = _dev()
    for what, src, dst, n, g in _degree_parents(dev):
        for f in (1.0, 0.85):
            mask = torch.from_numpy(ref.read_mask(n, f, KEY, 1, 0))
            for method in ("sort", "index"):
                sub = cluster.induced_subgraph(g, mask, method)
                s, d = (t.cpu().numpy() for t in sub.edges())
                if f == 1.0:
                    assert np.array_equal(s, src) and np.array_equal(d, dst)
                ns = sub.num_nodes()
                pe = torch.full((ns, 18), 7.0, device=dev)
                assert engine.index_degrees(sub.index(dev), pe) is pe
                torch.cuda.synchronize()
                ind, outd = ref.degrees(s, d, ns)
                got = pe.cpu().numpy()
                assert (ind == 0).any() and (outd == 0).any()
                assert np.array_equal(got[:, 0], ind) and np.array_equal(got[:, 1], outd), (what, f, method)
                assert np.all(got[:, 2:] == 7.0)
                wide = torch.full((ns, 40), 7.0, device=dev)                        # rows 20 floats apart: a column slice
                engine.index_degrees(sub.index(dev), wide[:, 20:])
                got = wide.cpu().numpy()
                assert np.array_equal(got[:, 20], ind) and np.array_equal(got[:, 21], outd) and np.all(got[:, :20] == 7.0)
                assert np.all(got[:, 22:] == 7.0)


# ---- 3. the thinned graph -------------------------------------------------------------------------------------------------------
def _same_graph(got, want, what):
    gs, gd = got.edges()
    ws, wd = want.edges()
    ic.assert_same((got.ndata[cluster_NID()], got.edata[cluster_NID()], gs, gd, got.index()),
                   (want.ndata[cluster_NID()], want.edata[cluster_NID()], ws, wd, want.index()), what)
    assert (got.num_nodes(), got.num_edges()) == (want.num_nodes(), want.num_edges()), what
    for k in want.edata:
        assert torch.equal(got.edata[k], want.edata[k]), f"{what}: edata '{k}'"
    for k in want.ndata:
        if k != "pe":
            assert torch.equal(got.ndata[k], want.ndata[k]), f"{what}: ndata '{k}'"


def cluster_NID():
    from gnnome_assembly_amd import cluster
    return cluster.NID


def _check_pe(sub, pe_parent, what):
    s, d = (t.cpu().numpy() for t in sub.edges())
    ind, outd = ref.degrees(s, d, sub.num_nodes())
    got = sub.ndata["pe"]
    nid = sub.ndata[cluster_NID()]
    assert torch.equal(got[:, 2:], pe_parent[nid][:, 2:]), f"{what}: pe columns 2.. are the parent's rows"
    assert np.array_equal(got[:, 0].cpu().numpy(), ind) and np.array_equal(got[:, 1].cpu().numpy(), outd), f"{what}: degrees"


@pytest.mark.parametrize("node_order", ["bfs", "keep"])
def test_masked_subgraph_equals_induced_subgraph_of_the_reference_mask(node_order):
    from gnnome_assembly_amd import cluster
    dev = _dev()
    src, dst, n, _ = ic.random_graph(6, 2001, 12000, True)              # an odd N: the last read has one strand
    g = ic.parent(src, dst, n, node_order, dev)
    pe = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 18)).astype(np.float32)).to(dev)
    g.ndata["pe"] = pe.clone()
    for f in (0.85, 0.5, 1.0, 0.0):
        for method in ("sort", "index"):
            want = cluster.induced_subgraph(g, torch.from_numpy(ref.read_mask(n, f, KEY, 3, 2)), method)
            got = cluster.masked_subgraph(g, f, KEY, 3, 2, method)
            torch.cuda.synchronize()
            what = f"{node_order} f = {f} {method}"
            _same_graph(got, want, what)
            _check_pe(got, pe, what)
            info = got.relabel_info
            assert info["mask_fraction"] == f and info["mask_kept_nodes"] == got.num_nodes() and info["mask"] == "device"
            assert info.get("induce") == ("index" if method == "index" else None)
    assert torch.equal(g.ndata["pe"], pe), "the parent's pe is read-only"
    assert cluster.masked_subgraph(g, 0.0, KEY, 3, 2).num_edges() == 0


# ---- 4. a training step on the thinned graph ------------------------------------------------------------------------------------
_CASE = {}


def _case(dev):
    """The 2,000-read synthetic graph under scattered caller ids (the parent renumbers: nperm), features on ndata / edata, the
    model at H = 128, L = 2 -- built once and left unchanged."""
    if not _CASE:
        import gnnome_assembly_amd as G
        from gnnome_assembly_amd import synth
        seed, H, L = 6, 128, 2
        src, dst, n = synth.make_graph(2000, seed=seed)
        inp = synth.make_inputs(src, dst, n, seed=seed)
        p = (2 * np.random.default_rng(5).permutation(n // 2)).astype(np.int32)
        perm = np.empty(n, np.int32)                                      # reads are permuted, the strands of a read stay adjacent
        perm[0:2 * p.size:2], perm[1:2 * p.size:2] = p, p + 1
        if n % 2:
            perm[n - 1] = n - 1
        src, dst = perm[src], perm[dst]
        pe = np.empty_like(inp["pe"])
        pe[perm] = inp["pe"]
        g = G.AssemblyGraph(src, dst, n, node_order="bfs").to(dev)
        g.ndata["pe"] = torch.from_numpy(pe).to(dev)
        g.edata["e"] = torch.from_numpy(inp["e"]).to(dev)
        g.edata["y"] = torch.from_numpy(inp["y"]).to(dev)
        sd = synth.synth_state_dict(H, L, seed)
        _CASE.update(g=g, sd=sd, H=H, L=L, pw=float(inp["pos_weight"]), n=n)
    return _CASE


def _model(c, dev):
    import gnnome_assembly_amd as G
    model = G.GraphGatedGCNModel(1, 2, c["H"], 16, c["L"], 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
    return model.to(dev), G.BCEWithLogitsLoss(c["pw"])


def _step(model, crit, sub):
    model.zero_grad(set_to_none=True)
    s = model(sub, None, sub.edata["e"], sub.ndata["pe"]).squeeze(-1)
    loss = crit(s, sub.edata["y"])
    loss.backward()
    torch.cuda.synchronize()
    return s.detach().clone(), loss.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters()}


@pytest.mark.parametrize("method", ["sort", "index"])
def test_training_step_on_the_thinned_graph(method):
    """Logits, loss and every parameter gradient of a step on masked_subgraph(f = 0.85) are bit-identical to the same model on the
    sub-graph built explicitly from the restatement's mask with bincount degrees (same code, same graph: a difference is a
    plumbing error); and the logits are within helpers.assert_parity of the fp64 oracle on that sub-graph's edge list and
    features."""
    from gnnome_assembly_amd import cluster
    from oracle import gatedgcn_oracle as orc
    dev = _dev()
    c = _case(dev)
    g, n = c["g"], c["n"]
    model, crit = _model(c, dev)
    got = cluster.masked_subgraph(g, 0.85, KEY, 1, 0, method)
    want = cluster.induced_subgraph(g, torch.from_numpy(ref.read_mask(n, 0.85, KEY, 1, 0)), method)
    s, d = (t.cpu().numpy() for t in want.edges())
    ind, outd = ref.degrees(s, d, want.num_nodes())
    pe = want.ndata["pe"].clone()
    pe[:, 0], pe[:, 1] = torch.from_numpy(ind).to(dev), torch.from_numpy(outd).to(dev)
    want.ndata["pe"] = pe
    assert 0.7 * g.num_edges() * 0.85 ** 2 < want.num_edges() < g.num_edges() and want.num_edges() > 1000
    assert torch.equal(got.ndata["pe"], pe)
    s1, l1, g1 = _step(model, crit, got)
    s0, l0, g0 = _step(model, crit, want)
    assert bool(torch.isfinite(s0).all())
    assert torch.equal(s0, s1) and torch.equal(l0, l1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"gradient of {k}"
    p64 = {k: torch.from_numpy(v).double() for k, v in c["sd"].items()}
    with torch.no_grad():
        s64 = orc.model_forward(p64, torch.from_numpy(s).long(), torch.from_numpy(d).long(), want.num_nodes(),
                                want.edata["e"].cpu().double(), pe.cpu().double())
    assert_parity(s1.cpu().numpy(), s64.squeeze(-1).numpy(), f"logits on the thinned graph ({method})")


# ---- 5. the prefetching loader --------------------------------------------------------------------------------------------------
def test_prefetching_loader_yields_the_same_graphs_and_the_same_losses():
    from gnnome_assembly_amd import cluster, engine
    dev = _dev()
    c = _case(dev)
    g = c["g"]
    steps = [(g, 0.85, 0), (g, 0.6, 1), (g, 1.0, 2)]

    def run(prefetch):
        loader = cluster.MaskedGraphLoader(steps, KEY, 4, prefetch=prefetch, induce="index")
        assert loader.prefetch == prefetch and len(loader) == 3
        model, crit = _model(c, dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        graphs, losses = [], []
        for sub in loader:                          # three optimizer steps, each on the graph the loader hands over
            _, loss, _ = _step(model, crit, sub)
            opt.step()
            graphs.append(sub)
            losses.append(loss)
        torch.cuda.synchronize()
        return graphs, losses
    inline, ahead = run(False), run(True)
    for k, (a, b) in enumerate(zip(inline[0], ahead[0])):
        _same_graph(b, a, f"prefetched step {k}")
        assert torch.equal(a.ndata["pe"], b.ndata["pe"])
        assert b.relabel_info["mask_fraction"] == steps[k][1]
        for wg in (1, engine.GATE2_WG):
            pa, pb = a.sweep_plan(dev, wg), b.sweep_plan(dev, wg)
            assert all(torch.equal(pa[key], pb[key]) for key in ("sinfo", "dinfo", "fix_nodes"))
        assert torch.equal(inline[1][k], ahead[1][k]), f"loss of step {k}"
    assert inline[0][2].num_edges() == g.num_edges()
    recompute = cluster.MaskedGraphLoader(steps, KEY, 4, prefetch=True, recompute_pe=True)
    assert recompute.prefetch is False                                   # the PageRank kernels share the step's scratch buffers


def test_recompute_pe_runs_the_positional_encoding_on_the_thinned_graph():
    from gnnome_assembly_amd import cluster, features
    dev = _dev()
    g = _case(dev)["g"]
    sub = cluster.masked_subgraph(g, 0.85, KEY, 1, 0, recompute_pe=True)
    carried = cluster.masked_subgraph(g, 0.85, KEY, 1, 0)
    want = features.positional_encoding(carried, 16)
    torch.cuda.synchronize()
    assert torch.equal(sub.ndata["pe"], want) and torch.equal(want[:, :2], carried.ndata["pe"][:, :2])
    assert not torch.equal(want[:, 2:], carried.ndata["pe"][:, 2:])


# ---- 6. mini-batch composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["sort", "index"])
def test_minibatch_is_cluster_selection_and_read_mask_in_one_induce(method):
    from gnnome_assembly_amd import cluster
    dev = _dev()
    c = _case(dev)
    g, n = c["g"], c["n"]
    part = cluster.partition_graph(g, 8)
    fr = [0.85, 0.5, 0.9, 1.0]
    loader = cluster.ClusterBatchLoader(g, part, 2, shuffle=False, prefetch=False, induce=method,
                                        read_mask=dict(key=KEY, epoch=2, graph_index=3, fractions=fr))
    ids = loader.batches()
    subs = list(loader)
    torch.cuda.synchronize()
    assert len(subs) == 4
    for k in (0, 1):
        sel = np.isin(part, ids[k].numpy())
        combined = torch.from_numpy(sel & ref.read_mask(n, fr[k], KEY, 2, 3))
        want = cluster.induced_subgraph(g, combined, "sort")
        _same_graph(subs[k], want, f"batch {k}")
        _check_pe(subs[k], g.ndata["pe"], f"batch {k}")
        assert 0 < subs[k].num_edges() < g.num_edges() // 2
    with pytest.raises(ValueError):
        cluster.ClusterBatchLoader(g, part, 2, read_mask=dict(key=KEY, epoch=2, graph_index=3, fractions=[0.5]))


# ---- 7. off is off --------------------------------------------------------------------------------------------------------------
def test_off_is_off(tmp_path):
    """mask_frac_low = mask_frac_high = 100 is the loop without the keys: the same launches (engine.profile_ops, the mechanism of
    test_gpu_dropout.test_off_is_off), the same History and weights; with 85 / 85 the two new kernels appear once per step."""
    from gnnome_assembly_amd import engine, train as T
    dev = _dev()
    c = _case(dev)
    g = c["g"]
    sample = T.GraphSample(g, g.edata["e"], g.ndata["pe"], g.edata["y"])
    hp = dict(num_epochs=1, dim_latent=128, num_gnn_layers=2, seed=0)
    runs = {}
    for name, extra in (("plain", {}), ("off", dict(mask_frac_low=100, mask_frac_high=100)),
                        ("on", dict(mask_frac_low=85, mask_frac_high=85))):
        wd = tmp_path / name
        wd.mkdir()
        engine.profile_ops(True)
        try:
            model, _, hist = T.train([sample, sample], [sample], out=name, hyperparameters=dict(hp, **extra), workdir=str(wd),
                                     verbose=False)
        finally:
            ops = engine.profile_ops(False)
        runs[name] = ({k: v[0] for k, v in ops.items()}, hist, torch.cat([p.detach().reshape(-1) for p in model.parameters()]))
    assert runs["off"][0] == runs["plain"][0]
    assert "gnm_read_mask" not in runs["plain"][0] and "gnm_index_degrees" not in runs["plain"][0]
    assert runs["off"][1] == runs["plain"][1] and torch.equal(runs["off"][2], runs["plain"][2])
    on = runs["on"]
    assert on[0]["gnm_read_mask"] == 2 and on[0]["gnm_index_degrees"] == 2
    assert on[1].mask_fraction == [0.85, 0.85] and len(on[1].masked_edges) == 2
    assert all(0 < e < g.num_edges() for e in on[1].masked_edges) and np.isfinite(on[1].loss_train[0])
    assert on[1].loss_valid != [] and np.isfinite(on[1].loss_valid[0])
