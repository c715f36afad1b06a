"""The two ends of the model (-m gpu): the edge encoder, the score predictor, the loss and the small reductions around them,
each called through the C ABI on device tensors and compared with a float64 computation on the host, at the row-tile tails
(E = 1, 63, 64, 65, 4097, ~100k: the fused predictor's 64-row tiles, the encoder's 16-row tiles and its Elast clamp, partial
workgroups) and at the edges of the arithmetic (BCE logits past where expf overflows, empty segments, signed zeros).  Every
kernel here is atomic-free by design, so every case also runs twice and must be bit-identical.

The bounds follow the arithmetic of each kernel: a contraction of K fp32 terms is within (K + c) u sum|terms| of the fp64
value (u = 2^-24; plus a norm-relative bar that a missing or doubled tile cannot meet), a fp64 accumulation with one final
rounding within one fp32 ulp, an fp32 segmented sum of n rows within n u sum|x|; the elementwise kernels are exact.

The second half runs GraphGatedGCNModel at the constructor arguments no other test varies -- hidden_edge_features,
hidden_edge_scores, nb_pos_enc, edge_features -- against the fp64 oracle, with the gradient clauses of
test_gpu_parity.test_other_widths_and_norms_vs_oracle; a hidden_edge_scores the row kernels are not built for runs as
zero-padded pieces of at most 256 columns (engine.pred_pieces)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import (GRAD_ABS_FLOOR, _branch_exact, _branch_exact_or_fail, _check, _grad_ok, assert_parity,
                     branch_exact_rows, rel_l2, sd_to_torch)
from oracle import gatedgcn_oracle as orc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # fp32 unit round-off
E_TAILS = [1, 63, 64, 65, 4097, 100003]
NAN = float("nan")


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    """The fused predictor and encoder and the whole-model rows run under all three matmul modes (include/gnm.h); the tests
    marked `mode_independent` never reach a mode-dependent kernel and run once."""
    from gnnome_assembly_amd import _lib
    if request.param != _lib.DEFAULT_MATMUL_MODE and request.node.get_closest_marker("mode_independent"):
        pytest.skip("runs once (does not depend on the matmul mode)")
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _lib():
    from gnnome_assembly_amd import _lib as L
    return L.load()


def _call(name, *args):
    from gnnome_assembly_amd import _lib as L
    L.check(getattr(L.load(), name)(*args), name)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=_dev())


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().double().numpy()


def _same_bits(a, b, what):
    """Bit-identical (NaN sentinels included): the run-twice determinism check."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    elif a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    assert torch.equal(a, b), f"{what}: two runs differ"


def _within(got, want, scale, k, what, l2=None):
    """|got - want| <= k u scale elementwise (scale: the fp64 sum of |terms| of each output), finite, and -- given l2 --
    norm-relative distance <= l2."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.all(np.isfinite(got)), f"{what}: non-finite values ({int((~np.isfinite(got)).sum())} of {got.size})"
    err = np.abs(got - want)
    lim = k * U * np.asarray(scale, np.float64) + 1e-30
    bad = err > lim
    i = int(np.argmax(err / lim))
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {got.size} outside {k} u sum|terms|; worst at {np.unravel_index(i, got.shape)}: "
                           f"got {got.flat[i]!r} want {want.flat[i]!r} limit {lim.flat[i]:.3e}")
    if l2 is not None:
        r = rel_l2(got, want)
        assert r <= l2, f"{what}: rel_l2 {r:.3e} > {l2:g}"


def _ulp_ok(got, want, slop, what):
    """A fp64 accumulation with one final rounding: within one fp32 ulp of the fp64 value (+ `slop`, the fp64 accumulation's
    own round-off bound)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert np.all(np.isfinite(got)), f"{what}: non-finite values"
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    bad = np.abs(got - want) > ulp + slop
    i = int(np.argmax(np.abs(got - want) - ulp - slop))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} more than 1 ulp off; worst: got {got.flat[i]!r} want {want.flat[i]!r}"


_GRAPHS = {}


def _graph(E):
    """(n, device index, host index) of a graph with E edges in shuffled edge-id order: the first E edges of
    synth.tiny_edge_case_graph (isolated, zero in- / out-degree nodes, hubs, self loops) up to 256, of synth.make_graph above."""
    if E not in _GRAPHS:
        from gnnome_assembly_amd import AssemblyGraph, synth
        if E <= 256:
            src, dst, n = synth.tiny_edge_case_graph(0)
        else:
            src, dst, n = synth.make_graph(12000, seed=3, permute_edge_ids=True)
        assert src.size >= E
        idx = AssemblyGraph(src[:E].copy(), dst[:E].copy(), n).to(_dev()).index(_dev())
        _GRAPHS[E] = (n, idx, {k: v.cpu().long().numpy() for k, v in idx.items()})
    return _GRAPHS[E]


def _partials():
    return torch.empty((_lib().gnm_max_partial_blocks() + 1) * 2 * 256, dtype=torch.float64, device=_dev())


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=_dev())


# ---------------------------------------------------------------------------------------------------------------------
# score predictor, fused (H = 128 / 256, hidden_edge_scores = 64)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", E_TAILS)
@pytest.mark.parametrize("H", [128, 256])
def test_predictor_fused_vs_fp64(H, E):
    """gnm_predictor_fused_fwd / _bwd with W1e a column slice of the real [HS, 3H] W1 (ldw = 3H > H): scores in edge-id
    order, hid, the in-place ghid, ge, gW1e, the gW2 / gb1 / gb2 sums and the zero tail of gsums."""
    HS = 64
    n, idx, hx = _graph(E)
    rng = np.random.default_rng(1000 * H + E)
    f32 = np.float32
    b = 1.0 / math.sqrt(3 * H)
    e = rng.standard_normal((E, H)).astype(f32)
    W1 = rng.uniform(-b, b, (HS, 3 * H)).astype(f32)
    b1 = rng.uniform(-b, b, HS).astype(f32)
    W2 = rng.uniform(-0.125, 0.125, (1, HS)).astype(f32)
    b2 = rng.uniform(-0.125, 0.125, 1).astype(f32)
    Pn = (0.5 * rng.standard_normal((n, 2 * HS))).astype(f32)
    gs = (rng.standard_normal(E) / E).astype(f32)
    de, dW1, db1, dW2, db2, dPn, dgs = map(_d, (e, W1, b1, W2, b2, Pn, gs))
    W1e = dW1[:, 2 * H:]
    assert W1e.stride(0) == 3 * H
    ws = _ws(_lib().gnm_predictor_fused_workspace_bytes())
    parts = _partials()

    def fwd(save):
        hid = _nan(E, HS) if save else None
        scores = _nan(E, 1)
        _call("gnm_predictor_fused_fwd", E, H, HS, _p(de), _p(W1e), W1e.stride(0), _p(db1), _p(dPn), _p(idx["isrc"]),
              _p(idx["idst"]), _p(idx["perm"]), _p(dW2), _p(db2), _p(hid), _p(scores), _p(ws), ws.numel(), _st())
        torch.cuda.synchronize()
        return hid, scores

    hid, scores = fwd(True)
    hid2, scores2 = fwd(True)
    _, scores3 = fwd(False)
    _same_bits(hid, hid2, "hid")
    _same_bits(scores, scores2, "scores")
    _same_bits(scores, scores3, "scores without hid")

    isrc, idst, perm = hx["isrc"], hx["idst"], hx["perm"]
    e64, W1e64, Pn64 = e.astype(np.float64), W1[:, 2 * H:].astype(np.float64), Pn.astype(np.float64)
    hid64 = e64 @ W1e64.T + b1 + Pn64[isrc, :HS] + Pn64[idst, HS:]
    hid_abs = np.abs(e64) @ np.abs(W1e64).T + np.abs(b1) + np.abs(Pn64[isrc, :HS]) + np.abs(Pn64[idst, HS:])
    _within(_host(hid), hid64, hid_abs, H + 4, f"H={H} E={E} hid", l2=1e-5)
    s_int = np.maximum(hid64, 0) @ W2[0].astype(np.float64) + b2[0]
    s_abs = hid_abs @ np.abs(W2[0]).astype(np.float64) + abs(float(b2[0]))
    want, scale = np.empty(E), np.empty(E)
    want[perm], scale[perm] = s_int, s_abs
    _within(_host(scores)[:, 0], want, scale, H + HS + 8, f"H={H} E={E} scores (edge-id order)", l2=1e-5)

    # backward from the device's own hid (its relu branches are the ones the backward must take)
    h32 = hid.cpu().numpy()

    def bwd():
        buf = hid.clone()
        ge, gW1e, gsums = _nan(E, H), _nan(HS, H), _nan(3 * HS)
        _call("gnm_predictor_fused_bwd", E, H, HS, _p(buf), _p(dgs), _p(idx["perm"]), _p(dW2), _p(de), _p(W1e), W1e.stride(0),
              _p(ge), _p(gW1e), _p(gsums), _p(parts), _p(ws), ws.numel(), _st())
        torch.cuda.synchronize()
        return buf, ge, gW1e, gsums

    out1, out2 = bwd(), bwd()
    for name, a, b_ in zip(("ghid", "ge", "gW1e", "gsums"), out1, out2):
        _same_bits(a, b_, name)
    ghid, ge, gW1e, gsums = out1
    gsi = gs[perm].astype(np.float64)
    ghid32 = np.where(h32 > 0, (gsi[:, None] * W2[0]).astype(np.float32), np.float32(0))     # fp32 product, then the gate
    assert np.array_equal(ghid.cpu().numpy(), ghid32), f"H={H} E={E} ghid (in place over hid) is not gscore[perm] W2 [hid > 0]"
    g64 = ghid32.astype(np.float64)
    _within(_host(ge), g64 @ W1e64, np.abs(g64) @ np.abs(W1e64), HS + 4, f"H={H} E={E} ge", l2=1e-5)
    _within(_host(gW1e), g64.T @ e64, np.abs(g64).T @ np.abs(e64), E + 2 * _lib().gnm_max_partial_blocks() + 4,
            f"H={H} E={E} gW1e", l2=1e-5)
    gsums = _host(gsums)
    prod = (gsi[:, None] * np.maximum(h32, 0)).astype(np.float32).astype(np.float64)     # the kernel's fp32 products
    slop = lambda t: 2 * E * 2.0 ** -53 * np.abs(t).sum(0)  # noqa: E731
    _ulp_ok(gsums[0:HS], prod.sum(0), slop(prod), f"H={H} E={E} gW2")
    _ulp_ok(gsums[HS:2 * HS], g64.sum(0), slop(g64), f"H={H} E={E} gb1")
    _ulp_ok(gsums[2 * HS:2 * HS + 1], [gsi.sum()], slop(gsi), f"H={H} E={E} gb2")
    assert np.all(gsums[2 * HS + 1:] == 0), f"H={H} E={E} gsums[{2 * HS + 1}:{3 * HS}] must stay zero"


# ---------------------------------------------------------------------------------------------------------------------
# score predictor, generic (any built hidden_edge_scores) and the reductions the engine chains behind it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.mode_independent
@pytest.mark.parametrize("E", E_TAILS)
@pytest.mark.parametrize("HS", [32, 64, 128, 256])
def test_predictor_generic_chain_vs_fp64(HS, E):
    """gnm_predictor_score_fwd / _bwd, then gnm_reduce_partials on the returned nblk and gnm_seg_sum_rows into gPn with
    ldo = 2 HS, the way engine.predictor_backward chains them."""
    n, idx, hx = _graph(E)
    rng = np.random.default_rng(7 * HS + E)
    f32 = np.float32
    hid0 = rng.standard_normal((E, HS)).astype(f32)           # e W1e^T + b1, as the GEMM in front leaves it
    Pn = (0.5 * rng.standard_normal((n, 2 * HS))).astype(f32)
    W2 = rng.uniform(-0.2, 0.2, (1, HS)).astype(f32)
    b2 = rng.uniform(-0.2, 0.2, 1).astype(f32)
    gs = (rng.standard_normal(E) / E).astype(f32)
    dPn, dW2, db2, dgs = map(_d, (Pn, W2, b2, gs))
    parts = _partials()
    maxb = _lib().gnm_max_partial_blocks()

    def run():
        hid = _d(hid0)
        scores = _nan(E, 1)
        _call("gnm_predictor_score_fwd", E, HS, _p(hid), _p(dPn), _p(idx["isrc"]), _p(idx["idst"]), _p(dW2), _p(db2),
              _p(idx["perm"]), _p(scores), _st())
        hid_f = hid.clone()
        nblk = C.c_int(0)
        _call("gnm_predictor_score_bwd", E, HS, _p(hid), _p(dgs), _p(dW2), _p(idx["perm"]), _p(parts), C.byref(nblk), _st())
        assert 0 < nblk.value <= maxb
        red = _nan(2, HS)
        _call("gnm_reduce_partials", _p(parts), nblk.value, 2, HS, _p(red), _st())
        gPn = _nan(n, 2 * HS)
        _call("gnm_seg_sum_rows", n, HS, _p(hid), _p(idx["out_ptr"]), _p(idx["out_pos"]), _p(gPn), 2 * HS, _st())
        _call("gnm_seg_sum_rows", n, HS, _p(hid), _p(idx["in_ptr"]), C.c_void_p(0), _p(gPn[:, HS:]), 2 * HS, _st())
        torch.cuda.synchronize()
        return hid_f, scores, hid, red, gPn

    r1, r2 = run(), run()
    for name, a, b_ in zip(("hid", "scores", "ghid", "partials reduced", "gPn"), r1, r2):
        _same_bits(a, b_, name)
    hid_f, scores, ghid, red, gPn = r1
    isrc, idst, perm = hx["isrc"], hx["idst"], hx["perm"]
    # hid += Ps[src] + Pd[dst]: two fp32 adds in this order -> exact
    want_hid = (torch.from_numpy(hid0) + torch.from_numpy(Pn[isrc, :HS])) + torch.from_numpy(Pn[idst, HS:])
    assert torch.equal(hid_f.cpu(), want_hid), f"HS={HS} E={E} hid"
    h32 = want_hid.numpy()
    h64 = h32.astype(np.float64)
    s_int = np.maximum(h64, 0) @ W2[0].astype(np.float64) + b2[0]
    s_abs = np.maximum(h64, 0) @ np.abs(W2[0]).astype(np.float64) + abs(float(b2[0]))
    want, scale = np.empty(E), np.empty(E)
    want[perm], scale[perm] = s_int, s_abs
    _within(_host(scores)[:, 0], want, scale, HS + 4, f"HS={HS} E={E} scores (edge-id order)")
    gsi = gs[perm].astype(np.float64)
    ghid32 = np.where(h32 > 0, (gsi[:, None] * W2[0]).astype(np.float32), np.float32(0))
    assert np.array_equal(ghid.cpu().numpy(), ghid32), f"HS={HS} E={E} ghid"
    red = _host(red)
    prod = (gsi[:, None] * np.maximum(h32, 0)).astype(np.float32).astype(np.float64)
    _ulp_ok(red[0], prod.sum(0), 2 * E * 2.0 ** -53 * np.abs(prod).sum(0), f"HS={HS} E={E} gW2")
    _ulp_ok(red[1, :1], [gsi.sum()], 2 * E * 2.0 ** -53 * np.abs(gsi).sum(), f"HS={HS} E={E} gb2")
    assert np.all(red[1, 1:] == 0), f"HS={HS} E={E} partial row 1 beyond column 0 must be zero"
    _check_seg_sums(_host(gPn)[:, :HS], ghid32, isrc, n, f"HS={HS} E={E} gPs (by source, through out_pos)")
    _check_seg_sums(_host(gPn)[:, HS:], ghid32, idst, n, f"HS={HS} E={E} gPd (by destination)")


def _check_seg_sums(got, x32, seg, n, what):
    """got[v] = sum of the rows j of x with seg[j] == v, in fp32: within deg(v) u sum|x| of the fp64 sum; empty segments 0."""
    x = x32.astype(np.float64)
    want = np.zeros((n, x.shape[1]))
    absum = np.zeros((n, x.shape[1]))
    np.add.at(want, seg, x)
    np.add.at(absum, seg, np.abs(x))
    deg = np.bincount(seg, minlength=n).astype(np.float64)
    _within(got, want, absum * (deg[:, None] + 1), 1, what)
    assert np.all(got[deg == 0] == 0), f"{what}: empty segments must be written as zeros"


# ---------------------------------------------------------------------------------------------------------------------
# edge encoder, fused (H = 128 / 256, edge_features = 2, hidden_edge_features = 16)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", E_TAILS)
@pytest.mark.parametrize("H", [128, 256])
def test_edge_encoder_fused_vs_fp64(H, E):
    """gnm_edge_encoder_fwd, _bwd and _bwd_dx: e in internal order, gW1 / gb1 / gW2 / gb2 and d e_raw in edge-id order.  The
    relu branches are the device's (the sign of fmaf(w1a, x0, fmaf(w1b, x1, b)), as helpers.device_masks models it): where
    fp32 and fp64 disagree on a pre-activation's sign, the fp64 backward is evaluated on the device's branch."""
    F, Q = 2, 16
    n, idx, hx = _graph(E)
    rng = np.random.default_rng(31 * H + E)
    f32 = np.float32
    e_raw = rng.standard_normal((E, F)).astype(f32)
    W1 = rng.uniform(-0.7, 0.7, (Q, F)).astype(f32)
    b1 = rng.uniform(-0.7, 0.7, Q).astype(f32)
    W2 = rng.uniform(-0.25, 0.25, (H, Q)).astype(f32)
    b2 = rng.uniform(-0.25, 0.25, H).astype(f32)
    ge0 = (rng.standard_normal((E, H)) / E).astype(f32)
    de_raw, dW1, db1, dW2, db2, dge0 = map(_d, (e_raw, W1, b1, W2, b2, ge0))
    ws = _ws(_lib().gnm_edge_encoder_bwd_workspace_bytes())

    def run():
        e0 = _nan(E, H)
        _call("gnm_edge_encoder_fwd", E, H, F, Q, _p(de_raw), _p(idx["perm"]), _p(dW1), _p(db1), _p(dW2), _p(db2), _p(e0), _st())
        g = [_nan(Q, F), _nan(Q), _nan(H, Q), _nan(H)]
        _call("gnm_edge_encoder_bwd", E, H, F, Q, _p(dge0), _p(de_raw), _p(idx["perm"]), _p(dW1), _p(db1), _p(dW2),
              *map(_p, g), _p(ws), ws.numel(), _st())
        gx = [_nan(Q, F), _nan(Q), _nan(H, Q), _nan(H)]
        ge_raw = _nan(E, F)
        _call("gnm_edge_encoder_bwd_dx", E, H, F, Q, _p(dge0), _p(de_raw), _p(idx["perm"]), _p(dW1), _p(db1), _p(dW2),
              *map(_p, gx), _p(ge_raw), _p(ws), ws.numel(), _st())
        torch.cuda.synchronize()
        return [e0] + g + gx + [ge_raw]

    r1, r2 = run(), run()
    for k, (a, b_) in enumerate(zip(r1, r2)):
        _same_bits(a, b_, f"output {k}")
    perm = hx["perm"]
    x = e_raw[perm].astype(np.float64)                              # internal order
    W1d, b1d, W2d = W1.astype(np.float64), b1.astype(np.float64), W2.astype(np.float64)
    inner = (x[:, 1:2] * W1d[None, :, 1] + b1d[None, :]).astype(f32).astype(np.float64)
    mask = (x[:, 0:1] * W1d[None, :, 0] + inner) > 0                 # the device's branch (exact sign of the fmaf)
    pre = x @ W1d.T + b1d
    a1 = np.where(mask, pre, 0.0)
    a1_abs = np.abs(x) @ np.abs(W1d).T + np.abs(b1d)
    what = f"H={H} E={E}"
    _within(_host(r1[0]), a1 @ W2d.T + b2, a1_abs @ np.abs(W2d).T + np.abs(b2), Q + 8, f"{what} e (internal order)", l2=1e-5)
    g64 = ge0.astype(np.float64)
    ga1 = (g64 @ W2d) * mask
    ga1_abs = np.abs(g64) @ np.abs(W2d)
    k = E + H + 2 * _lib().gnm_max_partial_blocks() + 16       # fp32 chains per workgroup, fp64 across workgroups: worst case
    want = [(ga1.T @ x, ga1_abs.T @ np.abs(x)), (ga1.sum(0), ga1_abs.sum(0)), (g64.T @ a1, np.abs(g64).T @ a1_abs),
            (g64.sum(0), np.abs(g64).sum(0))]
    for j, name in enumerate(("gW1", "gb1", "gW2", "gb2")):
        for off, variant in ((1, "bwd"), (5, "bwd_dx")):
            _within(_host(r1[off + j]), want[j][0], want[j][1], k, f"{what} {name} ({variant})", l2=1e-5)
    ge_raw = np.empty((E, F))
    ge_raw[perm] = ga1 @ W1d
    ge_abs = np.empty((E, F))
    ge_abs[perm] = ga1_abs @ np.abs(W1d)
    _within(_host(r1[9]), ge_raw, ge_abs, H + Q + 8, f"{what} d e_raw (edge-id order)", l2=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------------------------------
BCE_SPECIAL = [0.0, 1e-8, -1e-8, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 1e4, -1e4]


def _bce64(x, y, pw):
    """The closed-form fp64 BCEWithLogitsLoss(pos_weight) mean and its gradient, without overflow."""
    x = x.astype(np.float64)
    y = y.astype(np.float64)
    sp = lambda t: np.logaddexp(0.0, t)  # noqa: E731
    with np.errstate(over="ignore"):
        sig = lambda t: np.where(t >= 0, 1.0 / (1.0 + np.exp(-np.abs(t))), np.exp(-np.abs(t)) / (1.0 + np.exp(-np.abs(t))))  # noqa: E731
        loss = np.mean(pw * y * sp(-x) + (1.0 - y) * sp(x))
        g = (-pw * y * sig(-x) + (1.0 - y) * sig(x)) / x.size
    return loss, g


@pytest.mark.mode_independent
@pytest.mark.parametrize("labels", ["zeros", "ones", "mixed"])
@pytest.mark.parametrize("E", [1, 255, 256, 257, 1 << 20])
def test_bce_vs_closed_form_fp64(E, labels):
    """gnm_bce_fwd_bwd against the closed-form fp64 loss and gradient, logits from {0, +-1e-8, +-20, +-87, +-89, +-1e4} among
    random ones, pos_weight in {0, 0.27, 1, 50}: loss and every gradient element within 1e-6 relative (gradient: absolute
    floor max(pos_weight, 1) x the smallest normal fp32 -- below it sigmoid(-x) pos_weight is subnormal).  E = 2^20 puts
    kMaxPartialBlocks workgroups on the partial sums."""
    lib = _lib()
    rng = np.random.default_rng(E + len(labels))
    nb = lib.gnm_max_partial_blocks()
    if E == 1 << 20:
        assert min(-(-E // 256), lib.gnm_num_cus() * 8) >= nb, "this size must fill every partial-sum slot"
    ws = torch.empty(nb, dtype=torch.float64, device=_dev())
    if E == 1:
        xs = [np.array([v], np.float32) for v in BCE_SPECIAL] + [rng.standard_normal(1).astype(np.float32)]
    else:
        x = (4 * rng.standard_normal(E)).astype(np.float32)
        k = min(E // 2, 40 * len(BCE_SPECIAL))
        x[rng.permutation(E)[:k]] = np.resize(np.array(BCE_SPECIAL, np.float32), k)
        xs = [x]
    for x in xs:
        y = {"zeros": np.zeros(E), "ones": np.ones(E), "mixed": (rng.random(E) < 0.5)}[labels].astype(np.float32)
        dx, dy = _d(x), _d(y)
        for pw in (0.0, 0.27, 1.0, 50.0):
            outs = []
            for _ in range(2):
                loss, gs = _nan(1), _nan(E, 1)
                _call("gnm_bce_fwd_bwd", E, _p(dx), _p(dy), float(pw), _p(loss), _p(gs), _p(ws), ws.numel() * 8, _st())
                torch.cuda.synchronize()
                outs.append((loss, gs))
            _same_bits(outs[0][0], outs[1][0], "loss")
            _same_bits(outs[0][1], outs[1][1], "gradient")
            what = f"E={E} labels={labels} pw={pw}" + (f" x={float(x[0])!r}" if E == 1 else "")
            want_l, want_g = _bce64(x, y, np.float32(pw).astype(np.float64))
            got_l, got_g = float(outs[0][0].item()), _host(outs[0][1])[:, 0]
            assert math.isfinite(got_l) and abs(got_l - want_l) <= 1e-6 * abs(want_l) + 1e-37, (what, got_l, want_l)
            assert np.all(np.isfinite(got_g)), f"{what}: non-finite gradient"
            err = np.abs(got_g - want_g)
            lim = 1e-6 * np.abs(want_g) + max(pw, 1.0) * float(np.finfo(np.float32).tiny)
            bad = err > lim
            i = int(np.argmax(err / lim))
            assert not bad.any(), (f"{what}: {int(bad.sum())} gradient elements off; worst at logit {float(x[i])!r} label "
                                   f"{float(y[i])}: got {got_g[i]!r} want {want_g[i]!r}")


# ---------------------------------------------------------------------------------------------------------------------
# the small helpers
# ---------------------------------------------------------------------------------------------------------------------
COLSUM = {"vec64": (64, 64, 0), "w18": (18, 18, 0), "ld72": (64, 72, 0), "offset1": (64, 64, 1), "vec640": (640, 640, 0)}


@pytest.mark.mode_independent
@pytest.mark.parametrize("variant", list(COLSUM))
@pytest.mark.parametrize("M", [1, 255, 256, 257, 100003])
def test_colsum_within_one_ulp(M, variant):
    """gnm_colsum_f32, both stage-1 kernels: float4 columns (W % 4 == 0, 16-B aligned rows) and one column per thread (W = 18;
    a base pointer one float off alignment); ld > W.  fp64 accumulation, one rounding: within 1 ulp of the fp64 sum."""
    W, ld, off = COLSUM[variant]
    if variant == "vec640" and M > 257:
        M = 20011          # keeps the host reference small
    rng = np.random.default_rng(M + W + ld + off)
    base = rng.standard_normal(M * ld + off + 8).astype(np.float32)
    dbase = _d(base)
    X = dbase[off:]
    ws = _ws(_lib().gnm_colsum_workspace_bytes(M, W))
    outs = []
    for _ in range(2):
        out = _nan(W + 4)
        _call("gnm_colsum_f32", M, W, _p(X), ld, _p(out), _p(ws), ws.numel(), _st())
        outs.append(out)
    _same_bits(outs[0], outs[1], "colsum")
    got = _host(outs[0])
    assert np.all(np.isnan(got[W:])), f"{variant} M={M}: wrote past column {W}"
    rows = base[off:off + M * ld].reshape(M, ld)[:, :W].astype(np.float64)
    _ulp_ok(got[:W], rows.sum(0), 2 * M * 2.0 ** -53 * np.abs(rows).sum(0), f"colsum {variant} M={M}")


@pytest.mark.mode_independent
@pytest.mark.parametrize("E", [256, 4097])
@pytest.mark.parametrize("W", [32, 64, 128, 256])
def test_seg_sum_rows_vs_fp64(W, E):
    """gnm_seg_sum_rows at every width, through `pos` (the by-source segments) and without (by destination), with the empty
    segments of the edge-case graph; fp32 accumulation: within deg(v) u sum|x|."""
    n, idx, hx = _graph(E)
    rng = np.random.default_rng(W + E)
    x = rng.standard_normal((E, W)).astype(np.float32)
    dx = _d(x)
    for ptr, pos, seg, name in ((idx["out_ptr"], idx["out_pos"], hx["isrc"], "with pos"), (idx["in_ptr"], None, hx["idst"], "no pos")):
        outs = []
        for _ in range(2):
            out = _nan(n, W)
            _call("gnm_seg_sum_rows", n, W, _p(dx), _p(ptr), _p(pos), _p(out), W, _st())
            outs.append(out)
        _same_bits(outs[0], outs[1], name)
        _check_seg_sums(_host(outs[0]), x, seg, n, f"seg_sum_rows W={W} E={E} {name}")


@pytest.mark.mode_independent
@pytest.mark.parametrize("W", [1, 2, 3, 16])
def test_gather_rows_exact(W):
    """gnm_gather_rows_f32 (edge features into internal order, d e_raw back out): out[j] = X[idx[j]], exactly."""
    rng = np.random.default_rng(W)
    for M in (1, 257, 100003):
        X = rng.standard_normal((301, W)).astype(np.float32)
        ids = rng.integers(0, 301, M).astype(np.int32)
        dX, dids = _d(X), _d(ids)
        outs = []
        for _ in range(2):
            out = _nan(M, W)
            _call("gnm_gather_rows_f32", M, W, _p(dX), _p(dids), _p(out), _st())
            outs.append(out)
        _same_bits(outs[0], outs[1], "gather")
        assert np.array_equal(outs[0].cpu().numpy(), X[ids]), f"gather_rows W={W} M={M}"


@pytest.mark.mode_independent
def test_relu_mask_exact_at_signed_zero():
    """gnm_relu_mask_f32: x = (ref > 0) ? x : 0 exactly; ref = +0.0 and -0.0 (and NaN) mask, the smallest normal does not."""
    rng = np.random.default_rng(5)
    tiny = np.finfo(np.float32).tiny
    for n in (1, 1000, 100003):
        ref = rng.standard_normal(n).astype(np.float32)
        special = np.array([0.0, -0.0, tiny, -tiny, 1.0, -1.0, NAN], np.float32)
        k = min(n, 7 * 50)
        ref[rng.permutation(n)[:k]] = np.resize(special, k)
        if n == 1:
            ref[0] = -0.0
        x = rng.standard_normal(n).astype(np.float32)
        dref = _d(ref)
        outs = []
        for _ in range(2):
            dx = _d(x)
            _call("gnm_relu_mask_f32", n, _p(dx), _p(dref), _st())
            outs.append(dx)
        _same_bits(outs[0], outs[1], "relu_mask")
        want = np.where(ref > 0, x, np.float32(0))
        assert np.array_equal(outs[0].cpu().numpy().view(np.int32), want.view(np.int32)), f"relu_mask n={n}"


@pytest.mark.mode_independent
@pytest.mark.parametrize("rows,W", [(1, 1), (3, 7), (2, 33), (3, 64)])
def test_reduce_partials_within_one_ulp(rows, W):
    """gnm_reduce_partials at nblk = 1, 15, 16, 17 and the maximum, rows * W not a multiple of 16: fp64 sums in a fixed order,
    one rounding -- within 1 ulp of the exact sum, nothing written past rows * W."""
    rng = np.random.default_rng(rows * 100 + W)
    total = rows * W
    for nblk in (1, 15, 16, 17, _lib().gnm_max_partial_blocks()):
        p = rng.standard_normal((nblk, total)) * np.exp2(rng.integers(-20, 20, (nblk, total)))
        dp_ = _d(p)
        outs = []
        for _ in range(2):
            out = _nan(total + 5)
            _call("gnm_reduce_partials", _p(dp_), nblk, rows, W, _p(out), _st())
            outs.append(out)
        _same_bits(outs[0], outs[1], "reduce_partials")
        got = _host(outs[0])
        assert np.all(np.isnan(got[total:])), f"reduce_partials nblk={nblk}: wrote past rows * W"
        want = np.array([math.fsum(p[:, c]) for c in range(total)])
        _ulp_ok(got[:total], want, 2 * nblk * 2.0 ** -53 * np.abs(p).sum(0), f"reduce_partials nblk={nblk} {rows}x{W}")


# ---------------------------------------------------------------------------------------------------------------------
# whole model at the constructor arguments of the two ends, against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
# (H, Q = hidden_edge_features, HS = hidden_edge_scores, nb_pos_enc, F = edge_features, batch_norm) -> the kernels the forward
# must reach: fused encoder, fused predictor, generic predictor
HEAD_ROWS = {
    (128, 16, 32, 16, 2, True): (True, False, True),       # fused encoder; generic predictor at HS = 32 at a fused width
    (128, 8, 128, 16, 2, True): (False, False, True),      # generic encoder with F = 2; HS = 128
    (256, 33, 256, 4, 2, True): (False, False, True),      # odd Q; HS = 256; small PE
    (32, 16, 48, 16, 2, False): (False, False, True),      # HS = 48 zero-padded to 64 (LayerNorm)
    (128, 16, 100, 0, 1, True): (False, False, True),      # nb_pos_enc = 0 (K = 2 GEMM); F = 1; HS = 100 padded to 128
    (96, 24, 300, 30, 3, True): (False, True, True),       # HS = 300: a 256 piece and a 44 -> 64 piece (fused); H padded
}
L_HEADS = 2
_ROWS = {}


def _row_id(row):
    H, Q, HS, PE, F, bn = row
    return f"h{H}_q{Q}_hs{HS}_pe{PE}_f{F}_{'bn' if bn else 'ln'}"


def _row_case(row):
    """Inputs, parameters and the fp64 oracle (logits, loss, parameter and input gradients) of a row -- computed once, shared by
    the matmul modes."""
    if row in _ROWS:
        return _ROWS[row]
    from gnnome_assembly_amd import synth
    H, Q, HS, PE, F, bn = row
    seed = H + HS
    src, dst, n = synth.make_graph(700, seed, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed, nb_pos_enc=PE)
    sd = synth.synth_state_dict(H, L_HEADS, seed, nb_pos_enc=PE, edge_features=F, hidden_edge_features=Q, hidden_edge_scores=HS)
    e = inp["e"] if F == 2 else np.random.default_rng(seed).normal(size=(src.size, F)).astype(np.float32)
    c = dict(src=src, dst=dst, n=n, e=e, pe=inp["pe"], y=inp["y"], pw=float(inp["pos_weight"]), sd=sd)
    p64 = sd_to_torch(sd, torch.float64, requires_grad=True)
    e64 = torch.from_numpy(e).double().requires_grad_(True)
    pe64 = torch.from_numpy(inp["pe"]).double().requires_grad_(True)
    s64 = orc.model_forward(p64, torch.from_numpy(src), torch.from_numpy(dst), n, e64, pe64, bn)
    l64 = orc.bce_loss(s64, torch.from_numpy(inp["y"]).double(), c["pw"])
    l64.backward()
    c.update(s64=s64.detach().numpy(), l64=l64.item(), g64={k: v.grad.numpy() for k, v in p64.items()},
             ge64=e64.grad.numpy(), gpe64=pe64.grad.numpy())
    _ROWS[row] = c
    return c


def _head_model(row, c, dev):
    import gnnome_assembly_amd as G
    H, Q, HS, PE, F, bn = row
    model = G.GraphGatedGCNModel(1, F, H, Q, L_HEADS, HS, bn, PE)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: v.shape for k, v in c["sd"].items()}
    return model.to(dev)


def _step(model, g, c, dev, inputs=False):
    import gnnome_assembly_amd as G
    e = torch.from_numpy(c["e"]).to(dev).requires_grad_(inputs)
    pe = torch.from_numpy(c["pe"]).to(dev).requires_grad_(inputs)
    s = model(g, None, e, pe)
    loss = G.BCEWithLogitsLoss(c["pw"])(s.squeeze(-1), torch.from_numpy(c["y"]).to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return s.detach().cpu(), loss.item(), (e.grad.cpu() if inputs else None), (pe.grad.cpu() if inputs else None)


def _param_grads_vs_oracle(row, c, model, dev, what):
    """The gradient clauses of test_gpu_parity.test_other_widths_and_norms_vs_oracle."""
    H, Q, HS, PE, F, bn = row
    bad = []
    for k, prm in model.named_parameters():
        got, want = prm.grad.detach().cpu().double().numpy(), c["g64"][k]
        r = rel_l2(got, want)
        if not _grad_ok(r, float(np.abs(got - want).max()), GRAD_ABS_FLOOR):
            bad.append((k, r))
    if bad:             # only relu-kink flips may explain a miss, under either norm; no noise clause
        brows, bgmax = branch_exact_rows(c["src"], c["dst"], c["n"], c["e"], c["pe"], c["y"], c["pw"], c["sd"], L_HEADS, dev, bn)
        _branch_exact_or_fail(bad, {r[0]: r for r in brows}, bgmax, what)


@pytest.mark.parametrize("row", list(HEAD_ROWS), ids=[_row_id(r) for r in HEAD_ROWS])
def test_head_hyperparameters_vs_oracle(row):
    """GraphGatedGCNModel at hidden_edge_features / hidden_edge_scores / nb_pos_enc / edge_features no other test uses:
    logits, loss and every parameter gradient against the fp64 oracle; the forward reaches the encoder and predictor
    kernels the row names."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine
    dev = _dev()
    c = _row_case(row)
    what = _row_id(row)
    model = _head_model(row, c, dev)
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    engine.profile_ops(True)
    try:
        with torch.no_grad():
            model(g, None, torch.from_numpy(c["e"]).to(dev), torch.from_numpy(c["pe"]).to(dev))
    finally:
        ops = engine.profile_ops(False)
    enc_fused, pred_fused, pred_generic = HEAD_ROWS[row]
    assert ("gnm_edge_encoder_fwd" in ops) == enc_fused and ("gnm_gather_rows_f32" in ops) != enc_fused, (what, sorted(ops))
    assert ("gnm_predictor_fused_fwd" in ops) == pred_fused, (what, sorted(ops))
    assert ("gnm_predictor_score_fwd" in ops) == pred_generic, (what, sorted(ops))
    s, loss, _, _ = _step(model, g, c, dev)
    assert_parity(s.numpy(), c["s64"], f"{what} logits")
    assert abs(loss - c["l64"]) < 1e-5, (what, loss, c["l64"])
    _param_grads_vs_oracle(row, c, model, dev, what)


def test_generic_encoder_row_input_grads_vs_oracle():
    """d e_raw and d pe on the generic encoder at F = 2 (Q = 8) with HS = 128: against the fp64 oracle, or exact on the
    device's relu branches (test_gpu_input_grads._check)."""
    import gnnome_assembly_amd as G
    dev = _dev()
    row = (128, 8, 128, 16, 2, True)
    c = _row_case(row)
    model = _head_model(row, c, dev)
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    s, loss, ge, gpe = _step(model, g, c, dev, inputs=True)
    assert_parity(s.numpy(), c["s64"], "logits")
    _param_grads_vs_oracle(row, c, model, dev, _row_id(row))
    _check(ge.numpy(), gpe.numpy(), c["ge64"], c["gpe64"], _row_id(row),
           lambda: _branch_exact(g, c["sd"], 128, L_HEADS, c["e"], c["pe"], c["y"], c["pw"], dev))


def test_padded_scores_flat_gradients_equal_autograd():
    """HS = 48 at H = 128 (a padded piece on the fused predictor) through models.flatten_parameters + dp.FlatGradients
    (direct_write): the kernels write the predictor gradients into the flat buffer's [48, 384] views, and every gradient is
    bit-identical to the ordinary autograd accumulation."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp
    dev = _dev()
    row = (128, 16, 48, 16, 2, True)
    c = _row_case(row)
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    plain = _head_model(row, c, dev)
    s0, l0, _, _ = _step(plain, g, c, dev)
    flat_model = _head_model(row, c, dev)
    flat_model.flatten_parameters()
    flat = dp.FlatGradients(flat_model.parameters(), direct_write=True)
    flat.zero_()
    s1, l1, _, _ = _step(flat_model, g, c, dev)
    assert not flat.fresh, "the direct-write gradient path was not taken"
    assert torch.equal(s0, s1) and l0 == l1
    for (k, a), (_, b_) in zip(plain.named_parameters(), flat_model.named_parameters()):
        assert torch.equal(a.grad.cpu(), b_.grad.cpu()), k
    assert_parity(s0.numpy(), c["s64"], "logits")
    _param_grads_vs_oracle(row, c, plain, dev, _row_id(row))


@pytest.mark.parametrize("H", [32, 128])
def test_score_predictor_any_hidden_size(H):
    """layers.ScorePredictor(H, 48) on its own -- the module users build a predictor from -- against
    oracle.predictor_forward in fp64: scores, d x, d e and the four parameter gradients."""
    from gnnome_assembly_amd import AssemblyGraph, layers, synth
    dev = _dev()
    HS = 48
    src, dst, n = synth.make_graph(400, seed=H, permute_edge_ids=True)
    rng = np.random.default_rng(H)
    x = rng.standard_normal((n, H)).astype(np.float32)
    e = rng.standard_normal((src.size, H)).astype(np.float32)
    gs = rng.standard_normal((src.size, 1)).astype(np.float32)
    torch.manual_seed(H)
    mod = layers.ScorePredictor(H, HS)
    sd64 = {"predictor." + k: v.detach().double().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
    mod = mod.to(dev)
    dx, de = _d(x).requires_grad_(True), _d(e).requires_grad_(True)
    s = mod(AssemblyGraph(src, dst, n).to(dev), dx, de)
    s.backward(_d(gs))
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    e64 = torch.from_numpy(e).double().requires_grad_(True)
    s64 = orc.predictor_forward(sd64, torch.from_numpy(src).long(), torch.from_numpy(dst).long(), x64, e64)
    s64.backward(torch.from_numpy(gs).double())
    assert_parity(s.detach().cpu().numpy(), s64.detach().numpy(), f"ScorePredictor({H}, {HS}) scores")
    pairs = [("x", dx.grad, x64.grad), ("e", de.grad, e64.grad)] + [
        (k, p.grad, sd64["predictor." + k].grad) for k, p in mod.named_parameters()]
    for name, got, want in pairs:
        got = got.detach().cpu().double().numpy()
        r = rel_l2(got, want.numpy())
        assert _grad_ok(r, float(np.abs(got - want.numpy()).max()), GRAD_ABS_FLOOR), (name, r)
