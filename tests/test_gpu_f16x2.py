"""The "f16x2" matmul mode (include/gnm.h: gnm_set_matmul_mode(2), the library default since round 5): fp32 operands as two
fp16 terms of a POWER-OF-TWO multiple, three MFMAs per product.  The whole of tests/test_gpu_parity.py runs under it (the
autouse `matmul_mode` fixture there); this file holds what is specific to it -- the scaling.  Every kernel that has the mode is
driven with operands that would leave the fp16 exponent range under a fixed scale (rows, elements, column groups and weight
columns spread over many decades, gradients of 1e-7, zero rows, a row 1e12 above all others, magnitudes that jump by 1e8 from
one tile to the next) and must stay as close to an fp64 evaluation as the fp32-MFMA mode does: rel-L2 <= 2e-6 and no worse
than 1.5x the fp32 mode's + 1e-7, componentwise |err| <= 4e-6 (|x| |W| + |other terms|) where the kernel scales per row, finite
everywhere.  (Sizes and tile edges of the node projection kernels, per element against fp64: tests/test_gpu_node_proj_kernels.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu
H = 128


@pytest.fixture(autouse=True)
def restore_mode():
    from gnnome_assembly_amd import _lib
    yield
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _weights(rng, rows, cols, axis):
    W = (rng.standard_normal((rows, cols)) / 11).astype(np.float32)
    for i, f in ((7, 0.0), (9, 1e-20), (11, 1e5)):            # a zero, a tiny and a huge output column
        sl = [slice(None)] * 2
        sl[axis] = i
        W[tuple(sl)] *= f
    return W


def _check(name, run, ref, scale, cw_bar=4e-6, base="f32"):
    """base: the mode f16x2 is held against -- fp32 MFMA where the kernel has that form, else bf16x3 (the exact split)."""
    from gnnome_assembly_amd import _lib
    res = {}
    for mode in (base, "f16x2"):
        _lib.set_matmul_mode(mode)
        o = run().astype(np.float64)
        assert np.isfinite(o).all(), f"{name} [{mode}]: non-finite output"
        res[mode] = (rel_l2(o, ref), float(np.max(np.abs(o - ref) / np.maximum(scale, 1e-300))))
    (r32, c32), (r16, c16) = res[base], res["f16x2"]
    print(f"{name}: rel_l2 f16x2={r16:.2e} {base}={r32:.2e}  cw f16x2={c16:.2e} {base}={c32:.2e}")
    assert r16 <= 2e-6 and r16 <= 1.5 * r32 + 1e-7, (name, r16, r32)
    if cw_bar is not None:
        assert c16 <= cw_bar, (name, c16, c32)


def test_mode_is_the_default_and_switchable():
    from gnnome_assembly_amd import _lib
    assert _lib.DEFAULT_MATMUL_MODE == "f16x2" and _lib.load().gnm_get_matmul_mode() == 2 and _lib.split_mode()
    _lib.set_matmul_mode("bf16x3")
    assert _lib.get_matmul_mode() == "bf16x3" and _lib.split_mode()
    _lib.set_matmul_mode("f32")
    assert not _lib.split_mode()


@pytest.mark.parametrize("case", ["normal", "rows", "elements", "zero_rows", "tiny"])
def test_node_projections_scale_per_row(case):
    """gnm_node_proj_fwd: P = h W5^T + b5; a row's factor comes from its own largest magnitude (gnm_fused.hip MmH2::stage)."""
    from gnnome_assembly_amd import _lib, engine
    dev, lib = _dev(), _lib.load()
    rng = np.random.default_rng(1)
    N = 20011                                            # ragged last tile
    hn = {"normal": lambda: rng.standard_normal((N, H)),
          "rows": lambda: rng.standard_normal((N, H)) * np.exp(rng.uniform(-30, 30, (N, 1))),
          "elements": lambda: rng.standard_normal((N, H)) * np.exp(rng.uniform(-12, 12, (N, H))),
          "zero_rows": lambda: rng.standard_normal((N, H)) * (rng.random((N, 1)) < 0.5),
          "tiny": lambda: rng.standard_normal((N, H)) * 1e-30}[case]().astype(np.float32)
    Wn, bn = _weights(rng, 5 * H, H, 0), (rng.standard_normal(5 * H) * (0.0 if case == "tiny" else 1.0)).astype(np.float32)
    h, W5, b5 = (torch.from_numpy(a).to(dev) for a in (hn, Wn, bn))
    ref = hn.astype(np.float64) @ Wn.astype(np.float64).T + bn
    scale = np.abs(hn).astype(np.float64) @ np.abs(Wn).astype(np.float64).T + np.abs(bn)

    def run():
        need = lib.gnm_rowtile_workspace_bytes(5 * H)
        ws = engine.scratch(dev).ws(need)
        out = torch.empty(N, 5 * H, device=dev)
        engine._call("gnm_node_proj_fwd", N, H, 5 * H, engine._ptr(h), engine._ptr(W5), engine._ptr(b5), engine._ptr(out), engine._ptr(ws), need,
                     engine._stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()
    _check(f"node_proj_fwd [{case}]", run, ref, scale, cw_bar=None if case == "tiny" else 4e-6)   # tiny: products below the fp32 range in every mode


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("case", ["normal", "rows", "elements"])
def test_edge_t_kernel_scales_per_row(case, H):
    """gnm_edge_t_fused_fwd: t = e W3^T + b3 + B1h[src] + B2h[dst]; the row factors are made one tile ahead, inside the matrix phase
    of the tile before (edge_t32_b3p_k<MmH2>; H = 256: edge_t32_h256p_k<MmH2>, a row = the 64 lanes of one wave, one factor for both
    contraction halves, the weight's column factors over its whole K = 256)."""
    from gnnome_assembly_amd import _lib, engine
    dev, lib = _dev(), _lib.load()
    rng = np.random.default_rng(2)
    E, Nn = 50021, 9973
    en = {"normal": lambda: rng.standard_normal((E, H)),
          "rows": lambda: rng.standard_normal((E, H)) * np.exp(rng.uniform(-30, 30, (E, 1))),
          "elements": lambda: rng.standard_normal((E, H)) * np.exp(rng.uniform(-12, 12, (E, H)))}[case]().astype(np.float32)
    Wn, bn = _weights(rng, H, H, 0), rng.standard_normal(H).astype(np.float32)
    Pn = rng.standard_normal((Nn, 5 * H)).astype(np.float32)
    src, dst = rng.integers(0, Nn, E).astype(np.int32), np.sort(rng.integers(0, Nn, E)).astype(np.int32)
    e, W3, b3, Pt, s_, d_ = (torch.from_numpy(a).to(dev) for a in (en, Wn, bn, Pn, src, dst))
    g1, g2 = Pn[src, 3 * H:4 * H].astype(np.float64), Pn[dst, 4 * H:5 * H].astype(np.float64)
    ref = en.astype(np.float64) @ Wn.astype(np.float64).T + bn + g1 + g2
    scale = np.abs(en).astype(np.float64) @ np.abs(Wn).astype(np.float64).T + np.abs(bn) + np.abs(g1) + np.abs(g2)

    def run():
        need = lib.gnm_rowtile_workspace_bytes(5 * H)
        ws = engine.scratch(dev).ws(need)
        out = torch.empty(E, H, device=dev)
        nb = C.c_int(0)
        engine._call("gnm_edge_t_fused_fwd", E, H, engine._ptr(e), engine._ptr(W3), engine._ptr(b3), engine._ptr(Pt), engine._ptr(s_), engine._ptr(d_),
                     engine._ptr(out), engine._ptr(engine.scratch(dev).partials), C.byref(nb), engine._ptr(ws), need, engine._stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()
    _check(f"edge_t_fused_fwd H={H} [{case}]", run, ref, scale, base="f32" if H == 128 else "bf16x3")


@pytest.mark.parametrize("case", ["normal", "tiny_grads", "rows", "groups_apart", "groups_rising", "zero_groups"])
@pytest.mark.parametrize("stats", [False, True])
def test_projection_backward_keeps_one_unit_across_the_column_groups(case, stats):
    """gnm_node_proj_bwd_nn(_stats): gh_in = gh_out + gP W5 -- the accumulator of a row runs over five 128-column groups of gP
    whose magnitudes differ; the row's reference exponent only grows and the accumulator follows it (h2_stage_nn)."""
    from gnnome_assembly_amd import _lib, engine
    dev, lib = _dev(), _lib.load()
    rng = np.random.default_rng(3)
    N = 20011
    rep = lambda a: np.repeat(a, H, axis=1)  # noqa: E731
    gPn = {"normal": lambda: rng.standard_normal((N, 5 * H)),
           "tiny_grads": lambda: rng.standard_normal((N, 5 * H)) * 1e-7,
           "rows": lambda: rng.standard_normal((N, 5 * H)) * np.exp(rng.uniform(-25, 5, (N, 1))),
           "groups_apart": lambda: rng.standard_normal((N, 5 * H)) * rep(10.0 ** rng.integers(-6, 1, (N, 5))),
           "groups_rising": lambda: rng.standard_normal((N, 5 * H)) * rep(np.tile(np.array([1e-12, 1e-6, 1.0, 1e6, 1e12]), (N, 1))),
           "zero_groups": lambda: rng.standard_normal((N, 5 * H)) * rep(rng.random((N, 5)) < 0.5)}[case]().astype(np.float32)
    Wn = _weights(rng, 5 * H, H, 1)
    ghn = (rng.standard_normal((N, H)) * np.abs(gPn).max(1, keepdims=True) * 0.1).astype(np.float32)
    zn = rng.standard_normal((N, H)).astype(np.float32)
    statn = np.stack([np.zeros(H), np.ones(H), np.ones(H), np.zeros(H)]).astype(np.float32)
    gP, W5, gh, z, stat = (torch.from_numpy(a).to(dev) for a in (gPn, Wn, ghn, zn, statn))
    ref = gPn.astype(np.float64) @ Wn.astype(np.float64) + ghn
    scale = np.abs(gPn).astype(np.float64) @ np.abs(Wn).astype(np.float64) + np.abs(ghn)

    def run():
        need = lib.gnm_rowtile_workspace_bytes(5 * H)
        ws = engine.scratch(dev).ws(need)
        out = torch.empty(N, H, device=dev)
        if stats and _lib.split_mode():
            nb = C.c_int(0)
            engine._call("gnm_node_proj_bwd_nn_stats", N, H, 5 * H, engine._ptr(gP), engine._ptr(W5), engine._ptr(gh), engine._ptr(out), engine._ptr(z),
                         engine._ptr(stat), engine._ptr(engine.scratch(dev).partials), C.byref(nb), engine._ptr(ws), need, engine._stream())
        else:
            engine._call("gnm_node_proj_bwd_nn", N, H, 5 * H, engine._ptr(gP), engine._ptr(W5), engine._ptr(gh), engine._ptr(out), engine._ptr(ws), need,
                         engine._stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()
    _check(f"node_proj_bwd_nn{'_stats' if stats else ''} [{case}]", run, ref, scale)


@pytest.mark.parametrize("case", ["normal", "rows", "rising", "falling", "jumps", "giant_row", "zero_rows", "elements"])
def test_weight_gradient_kernel_keeps_one_unit_across_rows(case):
    """gnm_tn128: gW[cg] = A[:, cg]^T h -- the contraction runs over the ROWS, whose magnitudes differ (tn_tr_k<., ., ., true>: a
    reference exponent per workgroup that only grows, a tile with a row far above it is staged again).  `jumps`: 1e8 between
    neighbouring 1000-row stretches (the staged-again path, over and over); `giant_row`: one row 1e12 above all others --
    the other rows' share of an entry stays resolved down to 2^-36 of the giant row's product, where the fp32 sum itself
    resolves 2^-24."""
    from gnnome_assembly_amd import _lib, engine
    dev, lib = _dev(), _lib.load()
    rng = np.random.default_rng(4)
    N = 100003
    col = lambda v: np.asarray(v)[:, None]  # noqa: E731
    An, hn = {"normal": lambda: (rng.standard_normal((N, 3 * H)) * 1e-5, rng.standard_normal((N, H))),
              "rows": lambda: (rng.standard_normal((N, 3 * H)) * np.exp(rng.uniform(-30, 0, (N, 1))),
                               rng.standard_normal((N, H)) * np.exp(rng.uniform(-3, 3, (N, 1)))),
              "rising": lambda: (rng.standard_normal((N, 3 * H)) * col(10.0 ** np.linspace(-20, 0, N)), rng.standard_normal((N, H))),
              "falling": lambda: (rng.standard_normal((N, 3 * H)) * col(10.0 ** np.linspace(0, -20, N)), rng.standard_normal((N, H))),
              "jumps": lambda: (rng.standard_normal((N, 3 * H)) * col(10.0 ** (8 * ((np.arange(N) // 1000) % 3))), rng.standard_normal((N, H))),
              "giant_row": lambda: (rng.standard_normal((N, 3 * H)) * col(np.where(np.arange(N) == N // 2, 1e12, 1.0)), rng.standard_normal((N, H))),
              "zero_rows": lambda: (rng.standard_normal((N, 3 * H)) * (rng.random((N, 1)) < 0.5), rng.standard_normal((N, H)) * (rng.random((N, 1)) < 0.7)),
              "elements": lambda: (rng.standard_normal((N, 3 * H)) * np.exp(rng.uniform(-12, 12, (N, 3 * H))),
                                   rng.standard_normal((N, H)) * np.exp(rng.uniform(-12, 12, (N, H))))}[case]()
    An, hn = An.astype(np.float32), hn.astype(np.float32)
    A, h = torch.from_numpy(An).to(dev), torch.from_numpy(hn).to(dev)
    ref = np.concatenate([An[:, c * H:(c + 1) * H].astype(np.float64).T @ hn.astype(np.float64) for c in range(3)])
    scale = np.concatenate([np.abs(An[:, c * H:(c + 1) * H]).astype(np.float64).T @ np.abs(hn).astype(np.float64) for c in range(3)])

    def run():
        sc = engine.scratch(dev)
        need = lib.gnm_tn128_workspace_bytes()
        gW, gb = torch.empty(3 * H, H, device=dev), torch.empty(3 * H, device=dev)
        engine.tn128(N, A, 3 * H, 3, h, gW, gb, sc.partials, sc.ws(need), need)
        torch.cuda.synchronize()
        return gW.cpu().numpy()
    _check(f"tn128 [{case}]", run, ref, scale, cw_bar=4e-6)


@pytest.mark.parametrize("kind", ["NT", "NN", "TN"])
@pytest.mark.parametrize("case", ["normal", "rows", "groups_apart"])
def test_general_gemm_route_of_the_wide_models(kind, case):
    """gnm_gemm_f32 in the shapes of a hidden-256 model (the reference's default width): NT [M,256] x [1280,256]^T and NN
    [M,1280] x [1280,256] through gemm_rows_b3_k<MmH2> (the row reference over 2 / 10 column groups, the weight's column
    factors over its whole K), TN [M,256]^T [M,256] through tn_tr_k<., ., ., true> with (A group, B group) classes."""
    from gnnome_assembly_amd import engine
    dev = _dev()
    rng = np.random.default_rng(6)
    M = 20011 if kind != "TN" else 40000
    K, N = {"NT": (256, 1280), "NN": (1280, 256), "TN": (M, 256)}[kind]
    rows = M
    cols = K if kind != "TN" else 256
    Xn = {"normal": lambda: rng.standard_normal((rows, cols)),
          "rows": lambda: rng.standard_normal((rows, cols)) * np.exp(rng.uniform(-25, 5, (rows, 1))),
          "groups_apart": lambda: rng.standard_normal((rows, cols)) * np.repeat(10.0 ** rng.integers(-6, 1, (rows, cols // H)), H, axis=1)}[case]()
    Xn = Xn.astype(np.float32)
    if kind == "NT":
        Wn = _weights(rng, N, K, 0)
        ref = Xn.astype(np.float64) @ Wn.astype(np.float64).T
        scale = np.abs(Xn).astype(np.float64) @ np.abs(Wn).astype(np.float64).T
        mode, shape = engine.NT, (M, N)
    elif kind == "NN":
        Wn = _weights(rng, K, N, 1)
        ref = Xn.astype(np.float64) @ Wn.astype(np.float64)
        scale = np.abs(Xn).astype(np.float64) @ np.abs(Wn).astype(np.float64)
        mode, shape = engine.NN, (M, N)
    else:
        Wn = (rng.standard_normal((M, 256)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float32)      # B[K, N]: the other row operand
        ref = Xn.astype(np.float64).T @ Wn.astype(np.float64)
        scale = np.abs(Xn).astype(np.float64).T @ np.abs(Wn).astype(np.float64)
        mode, shape = engine.TN, (256, 256)
    X, W = torch.from_numpy(Xn).to(dev), torch.from_numpy(Wn).to(dev)

    def run():
        out = engine.gemm(mode, X, W, torch.empty(*shape, device=dev))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    _check(f"gemm {kind} [{case}]", run, ref, scale)


@pytest.mark.parametrize("spread", [0, 12])
def test_chained_backward_with_edge_gradients_spread_over_decades(spread):
    """The chained edge backward (edge_bwd_chain_k<..., H2>: gt W3 per row, gW3 = gt^T e across rows through the workgroup's
    reference exponent) inside the model's backward, from ONE forward state (the forward always runs in bf16x3 here, so every mode
    differentiates the same relu branches) and an upstream gradient whose rows are spread over `spread` decades edge by edge --
    neighbouring 16-row tiles then differ by more than the 2^10 a tile may lie above the reference, over and over (the
    staged-again path).  Every parameter gradient of the f16x2 backward must agree with the bf16x3 backward (exact products) as
    closely as the fp32-MFMA backward does."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import _lib, engine, synth
    from helpers import sd_to_torch
    dev = _dev()
    Hm, L = 128, 3
    src, dst, n = synth.make_graph(20000, 3)
    inp = synth.make_inputs(src, dst, n, 3)
    sd = synth.synth_state_dict(Hm, L, 3)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    P = {k: v.to(dev) for k, v in sd_to_torch(sd).items()}
    e_raw, pe, y = (torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y"))
    rng = np.random.default_rng(8)
    wts = torch.from_numpy((10.0 ** rng.uniform(-spread, 0, src.size)).astype(np.float32)).to(dev)
    grads = {}
    for mode in ("bf16x3", "f16x2", "f32"):
        _lib.set_matmul_mode("bf16x3")
        scores, ms = engine.model_forward(g, e_raw, pe, P, L, True)
        _, gs = engine.bce_with_logits(scores, y, float(inp["pos_weight"]))
        gs = gs * wts.reshape(gs.shape)
        _lib.set_matmul_mode(mode)
        ms.matmul = None                # a backward in ANOTHER mode than its forward is refused (engine._same_matmul_mode, round 6);
        for s_ in ms.layers:            # this test wants exactly that: it clears the recorded mode
            s_.matmul = None
        Gd = engine.model_backward(g, P, L, ms, gs)
        torch.cuda.synchronize()
        grads[mode] = {k: v.detach().double().cpu() for k, v in Gd.items()}
    gmax = max(float(v.norm()) for v in grads["bf16x3"].values())
    worst16 = worst32 = 0.0
    for k, ref in grads["bf16x3"].items():
        assert bool(torch.isfinite(grads["f16x2"][k]).all()), k
        if float(ref.norm()) < 1e-6 * gmax:
            continue                                                       # analytically zero (a bias in front of a BatchNorm)
        r16 = float((grads["f16x2"][k] - ref).norm() / ref.norm())
        r32 = float((grads["f32"][k] - ref).norm() / ref.norm())
        worst16, worst32 = max(worst16, r16), max(worst32, r32)
        # (the bias gradients of A_2 / A_3 are sums over all nodes that cancel to ~1e-4 of their terms: the fp32-MFMA backward sits 2e-4 from the
        #  exact-product one there, and so does this one -- what is bounded is the distance RELATIVE to what fp32 arithmetic shows)
        assert r16 <= 1e-3 and r16 <= 2.0 * r32 + 2e-6, (k, r16, r32)
    print(f"chained backward, edge gradients over {spread} decades: worst rel_l2 vs bf16x3: f16x2 {worst16:.2e}, f32 {worst32:.2e}")


@pytest.mark.parametrize("case", ["normal", "tiny_grads", "rows"])
def test_wide_edge_backward_gt_nn_scales_per_row(case):
    """gnm_edge_bwd_gt_nn (H = 256): gt = gamma rstd (gu - m1 - that m2), gu = ge [t scale + shift > 0], and ge_out = ge + gt W3 in one pass
    (edge_gt_nn_h256_k<MmH2>): gt is formed in the kernel, its rows scaled by their own largest magnitude over all 256 columns."""
    from gnnome_assembly_amd import _lib, engine
    dev, lib = _dev(), _lib.load()
    rng = np.random.default_rng(9)
    E, Hw = 30011, 256
    gen = {"normal": lambda: rng.standard_normal((E, Hw)),
           "tiny_grads": lambda: rng.standard_normal((E, Hw)) * 1e-7,
           "rows": lambda: rng.standard_normal((E, Hw)) * np.exp(rng.uniform(-25, 5, (E, 1)))}[case]().astype(np.float32)
    tn = rng.standard_normal((E, Hw)).astype(np.float32)
    stat = np.stack([rng.standard_normal(Hw) * 0.1, 1.0 + rng.random(Hw), 1.0 + rng.random(Hw), rng.standard_normal(Hw) * 0.3]).astype(np.float32)
    bstat = (np.stack([rng.standard_normal(Hw), rng.standard_normal(Hw)]) * 1e-3 * float(np.abs(gen).mean())).astype(np.float32)
    gam = (0.5 + rng.random(Hw)).astype(np.float32)
    Wn = _weights(rng, Hw, Hw, 1)
    ge, t, st_, bs_, ga_, W3 = (torch.from_numpy(a).to(dev) for a in (gen, tn, stat, bstat, gam, Wn))
    g64, t64 = gen.astype(np.float64), tn.astype(np.float64)
    gu = g64 * ((tn * stat[2] + stat[3]) > 0)            # the branch as the kernel takes it: sign of the fp32 fma (no kink within 1 ulp here)
    gt_ref = (gam.astype(np.float64) * stat[1]) * (gu - bstat[0] - ((t64 - stat[0]) * stat[1]) * bstat[1])
    ref = g64 + gt_ref @ Wn.astype(np.float64)
    scale = np.abs(g64) + np.abs(gt_ref) @ np.abs(Wn).astype(np.float64)

    def run():
        need = lib.gnm_rowtile_workspace_bytes(5 * Hw)
        ws = engine.scratch(dev).ws(need)
        gt, out = torch.empty(E, Hw, device=dev), torch.empty(E, Hw, device=dev)
        engine._call("gnm_edge_bwd_gt_nn", E, Hw, engine._ptr(ge), engine._ptr(t), engine._ptr(st_), engine._ptr(bs_), engine._ptr(ga_), engine._ptr(W3),
                     engine._ptr(gt), engine._ptr(out), engine._ptr(ws), need, engine._stream())
        torch.cuda.synchronize()
        assert rel_l2(gt.cpu().numpy().astype(np.float64), gt_ref) <= 5e-7
        return out.cpu().numpy()
    from gnnome_assembly_amd import _lib as L_
    res = {}
    for mode in ("bf16x3", "f16x2"):                     # (no fp32-MFMA twin of this kernel: bf16x3, the exact split, is the yardstick)
        L_.set_matmul_mode(mode)
        o = run().astype(np.float64)
        assert np.isfinite(o).all()
        res[mode] = (rel_l2(o, ref), float(np.max(np.abs(o - ref) / np.maximum(scale, 1e-300))))
    print(f"edge_bwd_gt_nn [{case}]: rel_l2 f16x2={res['f16x2'][0]:.2e} bf16x3={res['bf16x3'][0]:.2e}  cw f16x2={res['f16x2'][1]:.2e} bf16x3={res['bf16x3'][1]:.2e}")
    assert res["f16x2"][0] <= 2e-6 and res["f16x2"][0] <= 1.5 * res["bf16x3"][0] + 1e-7 and res["f16x2"][1] <= 4e-6
