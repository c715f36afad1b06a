"""LayerNorm models and layers wider than 256 channels, end to end, with the opt-in on (layers.WIDE_LAYERNORM, monkeypatched): the
body of test_gpu_parity.test_other_widths_and_norms_vs_oracle at (H, L) = (320, 2), (512, 1), (600, 1) against the fp64 oracle with
the same bars; a stand-alone GatedGCN_1d(48, 300, False) (no residual) against the oracle's layer; lean activations and activation
checkpointing bit-identical to the saved mode; and the default (switch off) still refusing.

A gradient outside GRAD_L2 must be exact on the device's own relu branches.  helpers.branch_exact_rows reads a LayerNorm layer's
branches with the <= 256-wide kernels (helpers.ln_layer_branches), which do not take a wide layer's chunks; _wide_branch_exact_rows
below is that function with the branches read from the wide kernels instead (zero residual: gnm_ln_wide_edge_gate_fwd /
gnm_ln_wide_node_update_fwd return relu(u) / relu(w) exactly, from the saved statistics) -- same fp64 backward
(oracle.manual_forward_backward on those branches), same bar (helpers._branch_exact_or_fail)."""
import copy

import numpy as np
import pytest
import torch

from helpers import GRAD_ABS_FLOOR, _branch_exact_or_fail, _grad_ok, assert_parity, device_masks, rel_l2, sd_to_torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    from gnnome_assembly_amd import _lib
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


@pytest.fixture(autouse=True)
def wide_on(monkeypatch):
    from gnnome_assembly_amd import layers
    monkeypatch.setattr(layers, "WIDE_LAYERNORM", True)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_CASES = {}


def _case(H, L):
    """Graph, inputs, parameters and the fp64 oracle's logits / loss / gradients of one (H, L), computed once for the three matmul modes."""
    if (H, L) in _CASES:
        return _CASES[(H, L)]
    from gnnome_assembly_amd import synth
    from oracle import gatedgcn_oracle as orc
    src, dst, n = synth.make_graph(700, seed=H + L, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed=H)
    sd = synth.synth_state_dict(H, L, seed=L)
    p64 = sd_to_torch(sd, torch.float64, requires_grad=True)
    s64 = orc.model_forward(p64, torch.from_numpy(src), torch.from_numpy(dst), n, torch.from_numpy(inp["e"]).double(),
                            torch.from_numpy(inp["pe"]).double(), False)
    l64 = orc.bce_loss(s64, torch.from_numpy(inp["y"]).double(), float(inp["pos_weight"]))
    l64.backward()
    c = dict(src=src, dst=dst, n=n, inp=inp, sd=sd, s64=s64.detach().numpy(), l64=l64.item(), g64={k: v.grad.numpy() for k, v in p64.items()})
    _CASES[(H, L)] = c
    return c


def _run_model(c, H, L, dev, checkpoint=0):
    import gnnome_assembly_amd as G
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, False, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
    model.to(dev)
    model.activation_checkpoint = checkpoint
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    inp = c["inp"]
    s = model(g, None, torch.from_numpy(inp["e"]).to(dev), torch.from_numpy(inp["pe"]).to(dev))
    loss = G.BCEWithLogitsLoss(float(inp["pos_weight"]))(s.squeeze(-1), torch.from_numpy(inp["y"]).to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return s.detach().cpu(), loss.item(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


def _wide_branch_exact_rows(src, dst, n, e_raw, pe, y, pw, sd, L, dev):
    """helpers.branch_exact_rows(..., batch_norm=False) for a model whose layers are wider than 256 channels."""
    from gnnome_assembly_amd import AssemblyGraph, engine, layers, models
    from oracle import gatedgcn_oracle as orc
    g = AssemblyGraph(src, dst, n).to(dev)
    idx = g.index()
    P = {k: v.to(dev) for k, v in sd_to_torch(sd).items()}
    H = P["linear_pe.weight"].shape[0]
    Hp = layers.padded_width(H)
    if Hp != H:
        P = {k: models._pad_param(k, v, H, Hp).contiguous() for k, v in P.items()}
    with engine.options(ACTIVATIONS="saved"):
        scores, ms = engine.model_forward(g, torch.from_numpy(e_raw).to(dev), torch.from_numpy(pe).to(dev), P, L, True, False, ln_width=H,
                                          wide_ln=True)
        rest = copy.copy(ms)
        rest.layers = []
        masks = device_masks(rest, sd, e_raw, idx)          # predictor and encoder branches
        perm = idx["perm"].long().cpu()
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        nrank = idx["nrank"].long().cpu() if "nrank" in idx else None
        N, E, w, p = n, perm.numel(), engine.WIDE_CHUNK, engine._ptr
        f32 = dict(dtype=torch.float32, device=dev)
        zero_e, zero_n = torch.zeros(E, w, **f32), torch.zeros(N, w, **f32)        # no residual: relu(u), relu(w) themselves
        for i, s in enumerate(ms.layers):
            prm = engine.layer_params(P, i)
            um, wm = [], []
            for ci, c in enumerate(s.chunks):
                sl = slice(ci * w, (ci + 1) * w)
                ru, rw, hf, inv_f = torch.empty(E, w, **f32), torch.empty(N, w, **f32), torch.empty(N, w, **f32), torch.empty(N, w, **f32)
                engine._call("gnm_ln_wide_edge_gate_fwd", N, E, p(c.t), p(zero_e), p(prm.gamma_e[sl]), p(prm.beta_e[sl]),
                             p(s.stat_e), p(c.P), p(idx["isrc"]), p(idx["in_ptr"]), p(ru), p(hf), p(inv_f), ci * w, H, engine._stream())
                engine._call("gnm_ln_wide_node_update_fwd", N, p(c.z), p(s.stat_h), p(prm.gamma_h[sl]), p(prm.beta_h[sl]),
                             p(zero_n), p(rw), ci * w, H, engine._stream())
                torch.cuda.synchronize()
                um.append((ru > 0).cpu()), wm.append((rw > 0).cpu())
            um, wm = torch.cat(um, 1)[:, :H], torch.cat(wm, 1)[:, :H]
            masks["u"].append(um[inv])
            masks["w"].append(wm if nrank is None else wm[nrank])
        loss, gs = engine.bce_with_logits(scores, torch.from_numpy(y).to(dev), pw)
        Gd = engine.model_backward(g, P, L, ms, gs, False, ln_width=H)
        torch.cuda.synchronize()
    for k, v in sd.items():
        if k == "predictor.W1.weight":
            Gd[k] = Gd[k].reshape(v.shape[0], 3, Hp)[:, :, :H].reshape(v.shape[0], 3 * H)
        else:
            Gd[k] = Gd[k][tuple(slice(0, d) for d in v.shape)]
    with torch.no_grad():
        _, l64, g64 = orc.manual_forward_backward(sd_to_torch(sd, torch.float64), torch.from_numpy(src), torch.from_numpy(dst), n,
                                                  torch.from_numpy(e_raw).double(), torch.from_numpy(pe).double(),
                                                  torch.from_numpy(y).double(), pw, masks=masks, batch_norm=False)
    assert abs(loss.item() - l64.item()) < 1e-5
    rows = [(k, rel_l2(Gd[k].cpu().double().numpy(), g64[k].double().numpy()),
             float(np.abs(Gd[k].cpu().double().numpy() - g64[k].double().numpy()).max()), float(g64[k].norm())) for k in g64]
    return rows, max(float(v.norm()) for v in g64.values())


@pytest.mark.parametrize("H,L", [(320, 2), (512, 1), (600, 1)])
def test_wide_layernorm_model_vs_oracle(H, L):
    """320 runs zero-padded to 512 (a half-dead second chunk), 512 as two full chunks, 600 zero-padded to 768 (three chunks)."""
    dev = _dev()
    c = _case(H, L)
    s, loss, grads = _run_model(c, H, L, dev)
    assert_parity(s.numpy(), c["s64"], f"H={H} L={L} LayerNorm logits")
    assert abs(loss - c["l64"]) < 1e-5
    bad = []
    for k, got in grads.items():
        got, want = got.double().numpy(), c["g64"][k]
        r = rel_l2(got, want)
        print(f"H={H} L={L} {k:32s} rel_l2={r:.3e}")
        if not _grad_ok(r, float(np.abs(got - want).max()), GRAD_ABS_FLOOR):
            bad.append((k, r))
    if bad:
        inp = c["inp"]
        brows, bgmax = _wide_branch_exact_rows(c["src"], c["dst"], c["n"], inp["e"], inp["pe"], inp["y"], float(inp["pos_weight"]), c["sd"], L, dev)
        _branch_exact_or_fail(bad, {r[0]: r for r in brows}, bgmax, f"H={H} L={L} LayerNorm")


def test_wide_branch_exact_comparison_holds():
    """Keeps the fall-back of the test above exercised: on the device's own branches every gradient of the 320-wide model is exact."""
    from helpers import BRANCH_L2
    dev = _dev()
    c = _case(320, 2)
    inp = c["inp"]
    rows, gmax = _wide_branch_exact_rows(c["src"], c["dst"], c["n"], inp["e"], inp["pe"], inp["y"], float(inp["pos_weight"]), c["sd"], 2, dev)
    assert len(rows) == len(c["sd"])
    bad = [r for r in rows if r[1] > BRANCH_L2 and r[2] > max(GRAD_ABS_FLOOR, 1e-6 * gmax)]
    assert not bad, bad


def test_standalone_wide_layernorm_layer_vs_oracle():
    """GatedGCN_1d(48, 300, False): in_channels != out_channels, so no residual; forward, input gradients and parameter gradients
    against the oracle's layer in fp64 autograd."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    from oracle import gatedgcn_oracle as orc
    from helpers import GRAD_L2
    dev = _dev()
    cin, cout = 48, 300
    src, dst, n = synth.make_graph(700, seed=5, permute_edge_ids=True)
    E = src.size
    rng = np.random.default_rng(300)
    conv = G.layers.GatedGCN_1d(cin, cout, False)
    with torch.no_grad():
        for k, prm in conv.named_parameters():
            if k.startswith("bn_"):
                prm.copy_(torch.from_numpy(((1.0 if k.endswith("weight") else 0.0) + 0.1 * rng.standard_normal(prm.shape)).astype(np.float32)))
    sd = {k: v.detach().clone() for k, v in conv.state_dict().items()}
    h, e, gh, ge = (rng.standard_normal(s).astype(np.float32) for s in ((n, cin), (E, cin), (n, cout), (E, cout)))
    conv.to(dev)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    hd, ed = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (h, e))
    ho, eo = conv(g, hd, ed)
    ((ho * torch.from_numpy(gh).to(dev)).sum() + (eo * torch.from_numpy(ge).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    p64 = {"gnn.convs.0." + k: v.double().requires_grad_(True) for k, v in sd.items()}
    h64, e64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (h, e))
    ho64, eo64 = orc.layer_forward(p64, 0, torch.from_numpy(src).long(), torch.from_numpy(dst).long(), n, h64, e64, False, residual=False)
    ((ho64 * torch.from_numpy(gh).double()).sum() + (eo64 * torch.from_numpy(ge).double()).sum()).backward()
    assert_parity(ho.detach().cpu().numpy(), ho64.detach().numpy(), "h_out")
    assert_parity(eo.detach().cpu().numpy(), eo64.detach().numpy(), "e_out")
    rows = [("d h", hd.grad, h64.grad), ("d e", ed.grad, e64.grad)] + \
        [(k, prm.grad, p64["gnn.convs.0." + k].grad) for k, prm in conv.named_parameters()]
    bad = []
    for k, got, want in rows:
        r = rel_l2(got.cpu().double().numpy(), want.numpy())
        print(f"GatedGCN_1d(48, 300, False) {k:14s} rel_l2={r:.3e}")
        if r > GRAD_L2:
            bad.append((k, r))
    assert not bad, bad


def _equal(a, b, what):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), f"{what}: logits differ"
    assert a[1] == b[1], f"{what}: loss differs"
    for k in a[2]:
        assert torch.equal(a[2][k].view(torch.int32), b[2][k].view(torch.int32)), f"{what}: gradient of {k} differs"


def test_wide_layernorm_lean_activations_bit_identical():
    from gnnome_assembly_amd import engine
    dev = _dev()
    c = _case(512, 1)
    saved = _run_model(c, 512, 1, dev)
    with engine.options(ACTIVATIONS="lean"):
        lean = _run_model(c, 512, 1, dev)
    _equal(saved, lean, "lean activations")


def test_wide_layernorm_checkpointing_bit_identical():
    dev = _dev()
    c = _case(320, 2)
    _equal(_run_model(c, 320, 2, dev), _run_model(c, 320, 2, dev, checkpoint=1), "activation_checkpoint = 1")


def test_switch_off_still_refuses(monkeypatch):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine, layers
    monkeypatch.setattr(layers, "WIDE_LAYERNORM", False)
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        G.GraphGatedGCNModel(1, 2, 512, 16, 1, 64, False, 16)
    dev = _dev()
    src, dst, n = np.array([0, 1], np.int32), np.array([1, 2], np.int32), 3
    g = G.AssemblyGraph(src, dst, n).to(dev)
    H = 512
    prm = engine.LayerParams(W5=torch.zeros(5 * H, H, device=dev), b5=torch.zeros(5 * H, device=dev), W3=torch.zeros(H, H, device=dev),
                             b3=torch.zeros(H, device=dev), gamma_e=torch.ones(H, device=dev), beta_e=torch.zeros(H, device=dev),
                             gamma_h=torch.ones(H, device=dev), beta_h=torch.zeros(H, device=dev))
    with pytest.raises(NotImplementedError, match="LayerNorm"):
        engine.layer_forward(g.index(), n, 2, H, prm, torch.zeros(n, H, device=dev), torch.zeros(2, H, device=dev), False, batch_norm=False)
