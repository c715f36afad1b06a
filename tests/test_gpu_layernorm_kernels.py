"""The LayerNorm kernels (gnm_layernorm.hip, the row statistics of gnm_ln.h) one by one against numpy / torch fp64 on the same fp32
inputs, through the C ABI, and the LayerNorm twin of test_gpu_parity.test_layer_kernels_vs_oracle.

Every row family of tests/ln_reference.py (well conditioned; |mean| >> std; var << eps; constant; all-zero; one dominant channel) is
in every case, at every kernel width and at a zero-padded width of each, for one row, a partly filled wave, a partly filled
workgroup and many workgroups with a tail.  The relu branches are the device's own (the zero-residual forward:
helpers.ln_layer_branches), so no element is left out of any comparison.

Bounds.  The well-conditioned family: the fixed bars (5e-7 rel-L2 forward, helpers.BRANCH_L2 backward).  Every family, componentwise:
|err| <= c u A + u Rnd with the bound parts A, Rnd of tests/ln_reference.py propagated through each kernel's formula and c per
family = 4 x the worst ratio torch's fp32 CPU layer_norm / autograd shows against the same fp64 (tools/measure_layernorm_bounds.py
-> profiles/layernorm_kernel_bounds.json; torch 2.10 CPU, 6000 rows per (H, width)):
              normal  offset  tiny  constant  zero  dominant
   fwd ratio    1.60    4.11  1.42      0       0      1.74      -> c = 6.4 16.44 5.68 exact exact 6.96
   bwd ratio    0.80    1.78  2.88    1.21    2.18     0.49      -> c = 3.2 7.12 11.52 4.84 8.72 1.96
torch's forward is EXACT for constant and all-zero rows (a running mean of equal values is that value), so those rows are compared
bit for bit.  What a sum over edges or rows inherits (hf, inv_f, the gP blocks, gamma / beta gradients) is bounded per node / per
column by the same per-row bounds summed, plus (terms) u per fp32 addition; the gate sigmoid's hardware forms (v_exp_f32, v_rcp_f32:
1 ulp each, gnm_common.h) are given (6 + |x|) u relative, its derivative (8 + |x|) u.  The H = 128 sweep forms (gnm_sweep.hip, gnm_tr.hip:
gnm_ln_edge_gate2_fwd, gnm_ln_edge_bwd_top + gnm_ln_edge_bwd_src_fix, gnm_ln_edge_bwd_chain) are held to the same reference and the same
bounds as the separate passes, on a graph whose plans serve most nodes and leave some to the fix-up pass, under all three matmul modes;
what the chained kernel contracts on the matrix cores (gW3_hi, the gt W3 share of the ge it leaves) to test_gpu_f16x2's 4e-6 sum |a||b|.
Each test prints the worst fraction of its bound every kernel output used ("bound used:"; recorded in the bounds file)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ln_reference as lr
from helpers import (BRANCH_L2, GRAD_L2, _branch_exact_or_fail, _grad_ok, ln_layer_branches, load_case, rel_l2, replica_base_graph,
                     sd_to_torch)
from ln_reference import U

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_L2 = 5e-7           # test_gpu_parity.test_layernorm_row_statistics_at_every_kernel_width
NORMAL = lr.FAMILIES.index("normal")
TINY64 = 2.0 ** -52


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    """As in test_gpu_parity: the tests marked `mode_independent` (no matrix-core kernel behind them) run once."""
    from gnnome_assembly_amd import _lib
    if request.param != _lib.DEFAULT_MATMUL_MODE and request.node.get_closest_marker("mode_independent"):
        pytest.skip("runs once (does not depend on the matmul mode)")
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _waves_per_block():
    src = open(os.path.join(REPO, "gnnome_assembly_amd", "csrc", "gnm_common.h")).read()
    return int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) // 64


def _constants():
    d = lr.load_constants()
    return d["fwd"], d["bwd"], d["fwd_exact"]


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


_USED = {}      # kernel output -> the worst fraction of its bound the device used (printed per test; profiles/layernorm_kernel_bounds.json)


def _use(key, frac):
    _USED[key] = max(_USED.get(key, 0.0), float(frac))


def _report(prefix):
    print("\n".join(f"bound used: {k:34s} {v:.3f}" for k, v in sorted(_USED.items()) if k.startswith(prefix)))


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs between two runs"


def _normal_l2(name, got, want, fam, bar):
    rows = fam == NORMAL
    if rows.any():
        r = rel_l2(got[rows], want[rows])
        assert r <= bar, f"{name}: rel-L2 {r:.3e} > {bar:g} on the well-conditioned rows"


def _dead_zero(name, a, H, width, blocks=1):
    a = np.asarray(a)
    for b in range(blocks):
        assert not a[..., b * H + width:(b + 1) * H].any(), f"{name}: dead channels of block {b} are not exactly 0"


# -----------------------------------------------------------------------------------------
# 3a: gnm_ln_node_update_fwd, gnm_ln_node_bwd
# -----------------------------------------------------------------------------------------

def _run_node(dev, N, H, width, z, ga, be, gh, hf, inv_f, hb, inv_b):
    from gnnome_assembly_amd import engine
    p, st = engine._ptr, engine._stream()
    f32 = dict(dtype=torch.float32, device=dev)
    relu_w = torch.full((N, H), float("nan"), **f32)
    engine._call("gnm_ln_node_update_fwd", N, H, p(z), p(ga), p(be), p(torch.zeros(N, H, **f32)), p(relu_w), width, st)
    gP = torch.full((N, 5 * H), float("nan"), **f32)
    Q = torch.full((N, 4 * H), float("nan"), **f32)
    partials = engine.scratch(dev).partials
    nblk = C.c_int(0)
    engine._call("gnm_ln_node_bwd", N, H, p(z), p(ga), p(be), p(gh), p(hf), p(inv_f), p(hb), p(inv_b), p(gP), p(Q), p(partials),
                 C.byref(nblk), width, st)
    red = torch.empty(2, H, **f32)
    engine._call("gnm_reduce_partials", p(partials), nblk.value, 2, H, p(red), st)
    _, gg, gb = engine.bn_bwd_finalize(partials, nblk.value, N, H, dev)
    torch.cuda.synchronize()
    return dict(relu_w=relu_w, gP=gP, Q=Q, red=red, gg=gg, gb=gb)


def _column_checks(name, got_gb, got_gg, gy, ref, fam, cf, dgy=None, key=None):
    """Column sums sum_rows gy (exact fp32 terms summed in fp64, or terms with the error bound dgy) and sum_rows gy * xhat against
    fp64, per column."""
    R = gy.shape[0]
    xh, ex = ref["xhat"], ref["ex"]
    dgy = np.zeros_like(gy) if dgy is None else dgy
    want_b, want_g = gy.sum(0), (gy * xh).sum(0)
    bound_b = dgy.sum(0) + U * np.abs(want_b) + R * TINY64 * np.abs(gy).sum(0)
    dxh = cf[fam][:, None] * U * ex + U * np.abs(xh)
    bound_g = (dgy * np.abs(xh) + (np.abs(gy) + dgy) * dxh).sum(0) + U * np.abs(want_g) + R * TINY64 * np.abs(gy * xh).sum(0)
    for what, got, want, bound in ((f"{name} sum gy", got_gb, want_b, bound_b), (f"{name} sum gy*xhat", got_gg, want_g, bound_g)):
        err = np.abs(_np(got) - want)
        assert (err <= bound).all(), (f"{what}: columns {np.nonzero(err > bound)[0][:8].tolist()} outside the bound, worst err/bound "
                                      f"{(err / np.maximum(bound, 1e-300)).max():.3g}")
        if key:
            _use(f"{key} column sums", np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())


@pytest.mark.mode_independent
@pytest.mark.parametrize("H,width", lr.HW)
def test_node_kernels_vs_fp64(H, width):
    """gnm_ln_node_update_fwd and gnm_ln_node_bwd: relu(w), gz = gP[:, 0:H], the four blocks of Q and the reduced column sums
    (gnm_reduce_partials, gnm_bn_bwd_finalize) against fp64; dead channels exactly 0; what the kernel does not write untouched."""
    dev = _dev()
    cf, cb, exact_f = _constants()
    rpw, waves = 256 // H, _waves_per_block()
    for N in (1, rpw + 1, waves * rpw + 1, 1003):
        rng = np.random.default_rng(100000 * H + 1000 * width + N)
        z, fam = lr.make_rows(rng, N, H, width, first=H + width)
        ga, be = lr.make_affine(rng, H, width)
        gh, hf, hb = (rng.standard_normal((N, H)).astype(np.float32) for _ in range(3))
        inv_f, inv_b = (np.exp(rng.uniform(-2, 2, (N, H))).astype(np.float32) for _ in range(2))
        args = [torch.from_numpy(a).to(dev) for a in (z, ga, be, gh, hf, inv_f, hb, inv_b)]
        out = _run_node(dev, N, H, width, *args)
        _same(out, _run_node(dev, N, H, width, *args), f"H={H} width={width} N={N}")
        what = f"H={H} width={width} N={N}"
        ref = lr.ln_ref(z, ga, be, width)
        A, Rnd = lr.fwd_bound(ref)
        relu_w = _np(out["relu_w"])
        want = np.maximum(ref["pre"], 0)
        _use("node_update_fwd relu(w)", lr.check(f"{what} relu(w)", relu_w, want, A, Rnd, cf[fam], exact_f[fam]))
        _normal_l2(f"{what} relu(w)", relu_w, want, fam, FWD_L2)
        gw = gh.astype(np.float64) * (relu_w > 0)            # the device's own branches
        gz, Ab, Rb = lr.ln_bwd_ref(ref, gw)
        gP, Q = _np(out["gP"]), _np(out["Q"])
        assert np.isnan(gP[:, H:]).all(), f"{what}: gnm_ln_node_bwd wrote outside gP[:, 0:H]"
        _use("node_bwd gz", lr.check(f"{what} gz", gP[:, :H], gz, Ab, Rb, cb[fam]))
        _normal_l2(f"{what} gz", gP[:, :H], gz, fam, BRANCH_L2)
        i_f, i_b, f64 = inv_f.astype(np.float64), inv_b.astype(np.float64), np.float64
        blocks = (("Qf", i_f, 2), ("Rf", i_f * np.abs(hf.astype(f64)), 3), ("Qb", i_b, 2), ("Rb", i_b * np.abs(hb.astype(f64)), 3))
        signs = (1.0, hf.astype(f64), 1.0, hb.astype(f64))
        for b, ((nm, scale, nr), sg) in enumerate(zip(blocks, signs)):
            wantq = gz * (i_f if b < 2 else i_b) * sg
            _use("node_bwd Q", lr.check(f"{what} {nm}", Q[:, b * H:(b + 1) * H], wantq, Ab * scale, nr * np.abs(wantq), cb[fam]))
            _normal_l2(f"{what} {nm}", Q[:, b * H:(b + 1) * H], wantq, fam, BRANCH_L2)
        _column_checks(f"{what} finalize", out["gb"], out["gg"], gw, ref, fam, cf, key="node_bwd")
        _column_checks(f"{what} reduce", out["red"][0], out["red"][1], gw, ref, fam, cf, key="node_bwd")
        _dead_zero(f"{what} relu(w)", relu_w, H, width)
        _dead_zero(f"{what} gz", gP[:, :H], H, width)
        _dead_zero(f"{what} Q", Q, H, width, 4)
        _dead_zero(f"{what} column sums", np.stack([_np(out["gb"]), _np(out["gg"]), *_np(out["red"])]), H, width)
    _report("node_")


# -----------------------------------------------------------------------------------------
# 3b: gnm_ln_edge_gate_fwd, gnm_ln_edge_bwd_dst, gnm_ln_edge_bwd_src
# -----------------------------------------------------------------------------------------

def _sigmoid(x):
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def _seg(index, val, n):
    out = np.zeros((n, val.shape[1]))
    np.add.at(out, index, val)
    return out


def _run_edge(dev, idx, N, E, H, width, t, e_in, ga, be, P, Q, ge0):
    from gnnome_assembly_amd import engine
    p, st = engine._ptr, engine._stream()
    f32 = dict(dtype=torch.float32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), **f32)  # noqa: E731
    relu_u, e_out, hf, inv_f, hf0, inv_f0 = nan(E, H), nan(E, H), nan(N, H), nan(N, H), nan(N, H), nan(N, H)
    engine._call("gnm_ln_edge_gate_fwd", N, E, H, p(t), p(torch.zeros(E, H, **f32)), p(ga), p(be), p(P), p(idx["isrc"]), p(idx["in_ptr"]),
                 p(relu_u), p(hf0), p(inv_f0), width, st)
    engine._call("gnm_ln_edge_gate_fwd", N, E, H, p(t), p(e_in), p(ga), p(be), p(P), p(idx["isrc"]), p(idx["in_ptr"]),
                 p(e_out), p(hf), p(inv_f), width, st)
    ge, gP, gt = ge0.clone(), nan(N, 5 * H), nan(E, H)
    partials = engine.scratch(dev).partials
    nblk = C.c_int(0)
    engine._call("gnm_ln_edge_bwd_dst", N, E, H, p(e_out), p(t), p(ga), p(be), p(ge), p(P), p(Q), p(idx["isrc"]), p(idx["in_ptr"]),
                 p(gP), p(gt), p(partials), C.byref(nblk), width, st)
    _, gg, gb = engine.bn_bwd_finalize(partials, nblk.value, E, H, dev)
    engine._call("gnm_ln_edge_bwd_src", N, E, H, p(e_out), p(gt), p(Q), p(idx["out_ptr"]), p(idx["out_pos"]), p(idx["out_dst"]), p(gP), st)
    torch.cuda.synchronize()
    return dict(relu_u=relu_u, e_out=e_out, hf=hf, inv_f=inv_f, ge=ge, gP=gP, gt=gt, gg=gg, gb=gb)


def _bounded(name, got, want, bound, key=None):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), f"{name}: shape / non-finite"
    err = np.abs(got - want)
    bad = err > bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} elements outside the bound, worst err/bound "
                           f"{(err[bad] / np.maximum(bound[bad], 1e-300)).max():.3g} at {np.argwhere(bad)[:4].tolist()}")
    if key:
        _use(key, np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())


def _run_sweep(dev, idx, plans, N, E, H, width, t, e_in, ga, be, P, Q, ge0, hf_n, hb_n, chain=None):
    """The H = 128 sweep forms on the same inputs: gnm_ln_edge_gate2_fwd, then gnm_ln_edge_bwd_top + gnm_ln_edge_bwd_src_fix or, with
    chain = (gt_hi, W3_hi) and ge0 = d loss / d e_out of the layer above, gnm_ln_edge_bwd_chain + gnm_ln_edge_bwd_src_fix."""
    from gnnome_assembly_amd import _lib, engine
    p, st = engine._ptr, engine._stream()
    f32 = dict(dtype=torch.float32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), **f32)  # noqa: E731
    plan2, plan = plans
    relu_u, hf0, inv_f0 = nan(E, H), nan(N, H), nan(N, H)
    engine._call("gnm_ln_edge_gate_fwd", N, E, H, p(t), p(torch.zeros(E, H, **f32)), p(ga), p(be), p(P), p(idx["isrc"]), p(idx["in_ptr"]),
                 p(relu_u), p(hf0), p(inv_f0), width, st)
    e_out, hf, inv_f, hb, inv_b, z = nan(E, H), nan(N, H), nan(N, H), nan(N, H), nan(N, H), nan(N, H)
    sc, sc2 = engine.scratch(dev), engine.scratch(dev, "chain")
    nblk = C.c_int(0)
    engine._call("gnm_ln_edge_gate2_fwd", N, E, H, p(t), p(e_in), p(ga), p(be), width, p(P), p(idx["isrc"]), p(idx["idst"]), p(idx["in_ptr"]),
                 p(plan2["sinfo"]), p(plan2["dinfo"]), plan2["nodes_per_block"], plan2["nfix"], p(plan2["fix_nodes"]), p(idx["out_ptr"]),
                 p(idx["out_pos"]), p(idx["out_dst"]), p(e_out), p(hf), p(inv_f), p(hb), p(inv_b), p(z), p(sc.partials), C.byref(nblk), st)
    ge, gP, gt = ge0.clone(), nan(N, 5 * H), nan(E, H)
    need = _lib.load().gnm_edge_bwd_fused_workspace_bytes()
    ws = sc.ws(need)
    out = dict(relu_u=relu_u, e_out=e_out, hf=hf, inv_f=inv_f, hb=hb, inv_b=inv_b, z=z, ge=ge, gP=gP, gt=gt)
    if chain is None:
        engine._call("gnm_ln_edge_bwd_top", N, E, H, p(ge), p(e_out), p(t), p(ga), p(be), width, p(P), p(Q), p(hf_n), p(hb_n), p(idx["isrc"]),
                     p(idx["idst"]), p(idx["in_ptr"]), p(gP), p(gt), p(sc.partials), p(plan["sinfo"]), plan["nodes_per_block"], C.byref(nblk),
                     p(ws), need, st)
    else:
        gt_hi, W3 = chain
        out["gW3"], out["gb3"] = nan(H, H), nan(H)
        engine._call("gnm_ln_edge_bwd_chain", N, E, H, p(ge), p(gt_hi), p(e_out), p(W3), p(out["gW3"]), p(out["gb3"]), p(sc2.partials), p(t),
                     p(ga), p(be), width, p(P), p(Q), p(hf_n), p(hb_n), p(idx["isrc"]), p(idx["idst"]), p(idx["in_ptr"]), p(gP), p(gt),
                     p(sc.partials), p(plan["sinfo"]), plan["nodes_per_block"], C.byref(nblk), p(ws), need, st)
    engine._call("gnm_ln_edge_bwd_src_fix", plan["nfix"], p(plan["fix_nodes"]), N, E, H, p(e_out), p(gt), p(Q), p(idx["out_ptr"]),
                 p(idx["out_pos"]), p(idx["out_dst"]), p(gP), st)
    _, out["gg"], out["gb"] = engine.bn_bwd_finalize(sc.partials, nblk.value, E, H, dev)
    torch.cuda.synchronize()
    return out


CONTRACTION = 4e-6      # test_gpu_f16x2._check: |err| <= 4e-6 sum |a| |b| for a product of any K under every matmul mode


def _edge_case(dev, graph, H, width, seed, plans=None, chain=False, tag="edge"):
    """One graph at one (H, width): run the kernels twice, compare everything with fp64.  plans = (forward plan, backward plan): the
    H = 128 sweep forms (_run_sweep; chain: the chained backward, whose ge on entry is the layer above's) instead of the separate
    passes (_run_edge).  The sweeps form Rf = Qf hf and Rb = Qb hb from the saved node rows, the separate passes read them from Q."""
    cf, cb, exact_f = _constants()
    idx = graph.index()
    N, E = graph.num_nodes(), graph.num_edges()
    isrc, idst = idx["isrc"].cpu().numpy().astype(np.int64), idx["idst"].cpu().numpy().astype(np.int64)
    rng = np.random.default_rng(seed)
    t, fam = lr.make_rows(rng, E, H, width, first=seed)
    ga, be = lr.make_affine(rng, H, width)
    live = np.arange(H) < width

    def rnd(rows, blocks):
        a = rng.standard_normal((rows, blocks, H)).astype(np.float32) * live
        return a.reshape(rows, blocks * H).astype(np.float32)
    e_in, P, Q, ge0 = rnd(E, 1), rnd(N, 5), rnd(N, 4), rnd(E, 1)
    args = [torch.from_numpy(a).to(dev) for a in (t, e_in, ga, be, P, Q, ge0)]
    f64 = np.float64
    blk = lambda a, b: a[:, b * H:(b + 1) * H]  # noqa: E731
    what = f"H={H} width={width} N={N} E={E}{' chain' if chain else ''}"
    if plans is None:
        assert "nperm" not in idx
        out = _run_edge(dev, idx, N, E, H, width, *args)
        _same(out, _run_edge(dev, idx, N, E, H, width, *args), what)
        rf, rb = blk(Q, 1).astype(f64), blk(Q, 3).astype(f64)
    else:
        hf_n, hb_n = rnd(N, 1), rnd(N, 1)
        extra = [torch.from_numpy(a).to(dev) for a in (hf_n, hb_n)]
        ch = None
        if chain:
            gt_hi = rnd(E, 1) * np.exp(rng.uniform(-3, 3, (E, 1))).astype(np.float32)
            W3 = (rng.standard_normal((H, H)) / 11).astype(np.float32) * live[:, None] * live[None, :]
            ch = (torch.from_numpy(gt_hi).to(dev), torch.from_numpy(W3.astype(np.float32)).to(dev))
        out = _run_sweep(dev, idx, plans, N, E, H, width, *args, *extra, chain=ch)
        _same(out, _run_sweep(dev, idx, plans, N, E, H, width, *args, *extra, chain=ch), what)
        rf, rb = blk(Q, 0).astype(f64) * hf_n, blk(Q, 2).astype(f64) * hb_n
    P, Q, e_in, ge0 = (a.astype(f64) for a in (P, Q, e_in, ge0))
    deg_in = np.bincount(idst, minlength=N)[:, None].astype(f64)
    deg_out = np.bincount(isrc, minlength=N)[:, None].astype(f64)
    # ---- forward
    ref = lr.ln_ref(t, ga, be, width)
    A, Rnd = lr.fwd_bound(ref)
    relu_u, want_relu = _np(out["relu_u"]), np.maximum(ref["pre"], 0)
    _use(f"{tag}_fwd relu(u)", lr.check(f"{what} relu(u)", relu_u, want_relu, A, Rnd, cf[fam], exact_f[fam]))
    e_out = want_relu + e_in
    d_e = cf[fam][:, None] * U * A + U * (Rnd + np.abs(e_out))
    _bounded(f"{what} e_out", _np(out["e_out"]), e_out, d_e, f"{tag}_fwd e_out")
    _normal_l2(f"{what} e_out", _np(out["e_out"]), e_out, fam, FWD_L2)
    sig = _sigmoid(e_out)
    d_sig = 0.25 * d_e + (6 + np.abs(e_out)) * U * sig
    a2_s, a3_d = blk(P, 1)[isrc], blk(P, 2)[idst]

    def gated_mean(name_h, name_inv, at, a_other, deg):
        """sum_at sigma a / (sum_at sigma + 1e-6) and its reciprocal denominator against fp64; returns (h, d_h)."""
        den, num = _seg(at, sig, N), _seg(at, sig * a_other, N)
        inv = 1.0 / (den + f64(np.float32(1e-6)))
        d_den = _seg(at, d_sig, N) + deg * U * den
        d_inv = inv * inv * d_den + 2 * U * inv
        d_num = _seg(at, d_sig * np.abs(a_other), N) + (deg + 1) * U * _seg(at, sig * np.abs(a_other), N)
        d_h = d_num * inv + np.abs(num) * d_inv + U * np.abs(num * inv)
        _bounded(f"{what} {name_inv}", _np(out[name_inv]), inv, d_inv, f"{tag}_fwd {name_inv}")
        _bounded(f"{what} {name_h}", _np(out[name_h]), num * inv, d_h, f"{tag}_fwd {name_h}")
        return num * inv, d_h
    hf, d_hf = gated_mean("hf", "inv_f", idst, a2_s, deg_in)
    if plans is not None:
        hb, d_hb = gated_mean("hb", "inv_b", isrc, a3_d, deg_out)
        zz = blk(P, 0) + hf + hb
        _bounded(f"{what} z", _np(out["z"]), zz, d_hf + d_hb + 2 * U * (np.abs(blk(P, 0)) + np.abs(hf) + np.abs(hb)), f"{tag}_fwd z")
    # ---- by-destination backward
    mask = relu_u > 0                               # the device's own branches
    dsg = sig * (1 - sig)
    d_dsg = 0.1 * d_e + (8 + np.abs(e_out)) * U * dsg
    qf_d, rf_d = blk(Q, 0)[idst], rf[idst]
    qb_s, rb_s = blk(Q, 2)[isrc], rb[isrc]
    gsig = qf_d * a2_s + qb_s * a3_d - rf_d - rb_s
    S = np.abs(qf_d * a2_s) + np.abs(qb_s * a3_d) + np.abs(rf_d) + np.abs(rb_s)
    d_ge0 = 0.0
    if chain:
        # the layer above's share of the chain: gW3_hi = gt_hi^T e_mid, gb3_hi = sum gt_hi, ge <- ge + gt_hi W3_hi (e_mid = this layer's e_out,
        # as the device holds it); the contraction bound of test_gpu_f16x2
        gth, w3, e_mid = gt_hi.astype(f64), W3.astype(f64), _np(out["e_out"])
        _bounded(f"{what} gW3_hi", _np(out["gW3"]), gth.T @ e_mid, CONTRACTION * (np.abs(gth).T @ np.abs(e_mid)), f"{tag}_bwd gW3_hi")
        _bounded(f"{what} gb3_hi", _np(out["gb3"]), gth.sum(0), (U + E * TINY64) * np.abs(gth).sum(0), f"{tag}_bwd gb3_hi")
        _dead_zero(f"{what} gW3_hi", _np(out["gW3"]), H, width)
        assert not _np(out["gW3"])[width:].any() and not _np(out["gb3"])[width:].any(), f"{what}: dead rows of gW3_hi / gb3_hi are not 0"
        d_ge0 = CONTRACTION * (np.abs(gth) @ np.abs(w3)) + U * np.abs(ge0)
        ge0 = ge0 + gth @ w3
    g = ge0 + gsig * dsg
    d_g = np.abs(gsig) * d_dsg + 4 * U * S * dsg + U * (np.abs(ge0) + np.abs(g)) + d_ge0
    _bounded(f"{what} ge (in place)", _np(out["ge"]), g, d_g, f"{tag}_bwd ge")
    gu = g * mask
    gt, Ab, Rb = lr.ln_bwd_ref(ref, gu)
    _, lin, _ = lr.ln_bwd_ref(dict(ref, X=np.zeros_like(ref["X"]), ex=np.zeros_like(ref["ex"])), d_g * mask)     # |LNbwd| applied to the error of gu
    d_gt = cb[fam][:, None] * U * Ab + U * Rb + lin
    _bounded(f"{what} gt", _np(out["gt"]), gt, d_gt, f"{tag}_bwd gt")
    _normal_l2(f"{what} gt", _np(out["gt"]), gt, fam, BRANCH_L2)
    gP = _np(out["gP"]) if not np.isnan(_np(out["gP"])[:, H:]).any() else None
    assert gP is not None, f"{what}: a gP block in H:5H was left unwritten"
    assert np.isnan(out["gP"].cpu().numpy()[:, :H]).all(), f"{what}: the edge kernels wrote gP[:, 0:H] (the node kernel's block)"
    _bounded(f"{what} gA3h", blk(gP, 2), _seg(idst, sig * qb_s, N),
             _seg(idst, d_sig * np.abs(qb_s), N) + (deg_in + 1) * U * _seg(idst, sig * np.abs(qb_s), N), f"{tag}_bwd gP")
    _bounded(f"{what} gB2h", blk(gP, 4), _seg(idst, gt, N), _seg(idst, d_gt, N) + deg_in * U * _seg(idst, np.abs(gt), N), f"{tag}_bwd gP")
    _column_checks(f"{what} partials", out["gb"], out["gg"], gu, ref, fam, cf, dgy=d_g * mask, key=f"{tag}_bwd")
    # ---- by-source backward
    qf_dd = blk(Q, 0)[idst]
    _bounded(f"{what} gA2h", blk(gP, 1), _seg(isrc, sig * qf_dd, N),
             _seg(isrc, d_sig * np.abs(qf_dd), N) + (deg_out + 1) * U * _seg(isrc, sig * np.abs(qf_dd), N), f"{tag}_bwd gP")
    _bounded(f"{what} gB1h", blk(gP, 3), _seg(isrc, gt, N), _seg(isrc, d_gt, N) + deg_out * U * _seg(isrc, np.abs(gt), N), f"{tag}_bwd gP")
    dead = [("relu(u)", relu_u, 1), ("e_out", _np(out["e_out"]), 1), ("hf", _np(out["hf"]), 1), ("ge", _np(out["ge"]), 1),
            ("gt", _np(out["gt"]), 1), ("gP[:, H:]", gP[:, H:], 4), ("column sums", np.stack([_np(out["gb"]), _np(out["gg"])]), 1)]
    if plans is not None:
        dead += [("hb", _np(out["hb"]), 1), ("z", _np(out["z"]), 1)]
    for nm, a, blocks in dead:
        _dead_zero(f"{what} {nm}", a, H, width, blocks)


@pytest.mark.mode_independent
@pytest.mark.parametrize("H,width", lr.HW)
def test_edge_kernels_vs_fp64(H, width):
    """gnm_ln_edge_gate_fwd, gnm_ln_edge_bwd_dst, gnm_ln_edge_bwd_src on a graph with a hub, a self loop, a duplicated edge, an
    isolated node and odd E and N, and on a 3-node / 2-edge graph: e_out, hf, inv_f, the in-place ge, gt, gP[:, H:5H] (gP[:, 0:H]
    poisoned and left alone) and the column sums against fp64."""
    from gnnome_assembly_amd import AssemblyGraph
    dev = _dev()
    src, dst, n = replica_base_graph(reads=300, hub_in=300)
    g = AssemblyGraph(src, dst, n, node_order="keep").to(dev)
    assert g.num_edges() % 2 == 1 and n % 2 == 1
    _edge_case(dev, g, H, width, seed=7 * H + width)
    g3 = AssemblyGraph(np.array([0, 2], np.int32), np.array([1, 1], np.int32), 3, node_order="keep").to(dev)
    _edge_case(dev, g3, H, width, seed=11 * H + width)
    _report("edge_")


# -----------------------------------------------------------------------------------------
# 3c: the H = 128 sweep forms -- gnm_ln_edge_gate2_fwd, gnm_ln_edge_bwd_top + gnm_ln_edge_bwd_src_fix, gnm_ln_edge_bwd_chain
# -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [128, 96])
def test_sweep_kernels_vs_fp64(width, matmul_mode):
    """The two-sided sweeps of a LayerNorm layer at H = 128 through the C ABI, on a graph whose host-built plans serve most nodes
    and leave some to the fix-up pass: the forward sweep (e_out, hf, inv_f and the by-source hb, inv_b, z), the backward sweep with
    its fix-up (the in-place ge, gt, gP[:, H:5H] with gP[:, 0:H] poisoned and left alone, the column sums) against fp64 on the same
    rows and with the same bounds as the separate passes; the chained backward (split matmul modes: it holds the layer above's
    gt^T e and gt W3 on the matrix cores) likewise, its gW3_hi, gb3_hi and the ge it leaves for the layer below within the
    contraction bound of test_gpu_f16x2.  Under fp32 matmuls the chained kernel is not built and must refuse."""
    from gnnome_assembly_amd import AssemblyGraph, _lib, engine, synth
    dev = _dev()
    H = 128
    src, dst, n = synth.make_graph(700, 7, permute_edge_ids=True)
    g = AssemblyGraph(src, dst, n).to(dev)
    plans = (g.sweep_plan(dev, engine.GATE2_WG), g.sweep_plan(dev))
    for plan in plans:
        assert plan is not None and 0 < plan["nfix"] < 0.2 * n, plan and plan["nfix"]
    _edge_case(dev, g, H, width, seed=13 * H + width, plans=plans, tag="sweep")
    if _lib.split_mode():
        _edge_case(dev, g, H, width, seed=17 * H + width, plans=plans, chain=True, tag="chain")
    else:
        with pytest.raises(_lib.GnmError):
            _edge_case(dev, g, H, width, seed=17 * H + width, plans=plans, chain=True, tag="chain")
    _report("sweep_")
    _report("chain_")


# -----------------------------------------------------------------------------------------
# 3d: one LayerNorm layer, kernel by kernel, against the oracle's hand-derived decomposition
# -----------------------------------------------------------------------------------------

_LAYER_CASES = {"small_h32l2ln_s1.npz": (None, None), "synth_h96": (96, None), "synth_h128_sweep": (128, True), "synth_h128_separate": (128, False),
                "synth_h256": (256, None)}
_LAYER_ORACLE = {}


def _layer_case(case):
    """Inputs and the fp64 oracle's per-layer intermediates of a case, computed once and shared by the matmul modes."""
    if case in _LAYER_ORACLE:
        return _LAYER_ORACLE[case]
    from gnnome_assembly_amd import synth
    from oracle import gatedgcn_oracle as orc
    if case.endswith(".npz"):
        z, sd, H, L, bn = load_case(case)
        assert not bn
        c = dict(src=z["src"], dst=z["dst"], n=int(z["n"]), e=z["e_raw"], pe=z["pe"], y=z["y"], pw=float(z["pos_weight"]))
    else:
        H, L = _LAYER_CASES[case][0], 2
        src, dst, n = synth.make_graph(700, seed=H, permute_edge_ids=True)
        inp = synth.make_inputs(src, dst, n, seed=H)
        sd = synth.synth_state_dict(H, L, seed=L)
        c = dict(src=src, dst=dst, n=n, e=inp["e"], pe=inp["pe"], y=inp["y"], pw=float(inp["pos_weight"]))
    c.update(sd=sd, H=H, L=L, p64=sd_to_torch(sd, torch.float64))
    c["args"] = (torch.from_numpy(c["src"]), torch.from_numpy(c["dst"]), c["n"], torch.from_numpy(c["e"]).double(),
                 torch.from_numpy(c["pe"]).double(), torch.from_numpy(c["y"]).double(), c["pw"])
    with torch.no_grad():
        _, _, c["g64"], c["dbg"] = orc.manual_forward_backward(c["p64"], *c["args"], keep=True, batch_norm=False)
    _LAYER_ORACLE[case] = c
    return c


@pytest.mark.parametrize("case", list(_LAYER_CASES))
def test_layernorm_layer_kernels_vs_oracle(case):
    """engine.layer_forward / layer_backward(batch_norm=False) on the top layer against every intermediate of
    oracle.manual_forward_backward(batch_norm=False): forward 2e-5 rel-L2, backward GRAD_L2 or exact (BRANCH_L2) on the branches
    the device took.  H = 96 runs zero-padded on the 128-wide kernels, H = 128 with the LayerNorm sweeps on and off."""
    import torch.nn.functional as F
    from gnnome_assembly_amd import AssemblyGraph, engine, layers, models
    from oracle import gatedgcn_oracle as orc
    dev = _dev()
    c = _layer_case(case)
    H, L, n, dbg, g64, sd = c["H"], c["L"], c["n"], c["dbg"], c["g64"], c["sd"]
    sweep = _LAYER_CASES[case][1]
    Hp = layers.padded_width(H)
    graph = AssemblyGraph(c["src"], c["dst"], n, node_order="keep").to(dev)
    idx = graph.index()
    perm = idx["perm"].long().cpu()
    E = c["src"].size
    li = L - 1
    d = dbg[li]
    P32 = {k: models._pad_param(k, v, H, Hp).contiguous().to(dev) for k, v in sd_to_torch(sd).items()}
    prm = engine.layer_params(P32, li)
    f = lambda t: F.pad(t.float(), (0, Hp - H)).contiguous().to(dev)  # noqa: E731
    cut = lambda t: t[..., :H]  # noqa: E731
    opts = {} if sweep is None else dict(LN_SWEEP=sweep, TWO_SIDED=True, TWO_SIDED_FWD=True)
    with engine.options(**opts):
        plan2 = graph.sweep_plan(dev, engine.GATE2_WG) if Hp == 128 and sweep is not False else None
        plan = graph.sweep_plan(dev) if Hp == 128 and sweep is not False else None
        if sweep:
            assert plan is not None and plan2 is not None and 0 < plan["nfix"] < 0.2 * n, plan and plan["nfix"]
        h_out, e_out, s = engine.layer_forward(idx, n, E, Hp, prm, f(d["h"]), f(d["e"][perm]), True, False, plan=plan2, ln_width=H)
        torch.cuda.synchronize()
        um, wm = ln_layer_branches(idx, n, E, prm, s, H)
        gh_in, ge_in, g = engine.layer_backward(idx, n, E, Hp, prm, s, f(d["gh_out"]), f(d["ge_out"][perm]), False, plan=plan, ln_width=H)
        torch.cuda.synchronize()
    rows = []

    def cmp(name, got, want, rows=rows):
        got, want = got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy()
        assert got.shape == want.shape, f"{name}: {got.shape} vs {want.shape}"
        rows.append((name, rel_l2(got, want), float(np.abs(got - want).max()), float(np.linalg.norm(want))))
    blocks5 = lambda t: t.reshape(t.shape[0], 5, Hp)[:, :, :H].reshape(t.shape[0], 5 * H)  # noqa: E731
    cmp("P", blocks5(s.P), d["P"])
    cmp("t", cut(s.t), d["t"][perm])
    cmp("e_out", cut(e_out), d["e_out"][perm])
    for k in ("hf", "inv_f", "hb", "inv_b", "z"):
        cmp(k, cut(getattr(s, k)), d[k])
    cmp("h_out", cut(h_out), d["h_out"])
    for k, t in (("e_out", e_out), ("hf", s.hf), ("hb", s.hb), ("z", s.z), ("h_out", h_out)):
        assert not t[:, H:].any(), f"{k}: dead channels are not exactly 0"
    nfwd = len(rows)
    pfx = f"gnn.convs.{li}."

    def backward_rows(dd, gg, out):
        W5 = lambda t: t.reshape(5, Hp, -1)[:, :H, :H].reshape(5 * H, H)  # noqa: E731
        cmp("gh_in", cut(gh_in), dd[li]["gh_in"], out)
        cmp("ge_in", cut(ge_in), dd[li]["ge_in"][perm], out)
        cmp("gW5", W5(g["W5"]), torch.cat([gg[pfx + k + ".weight"] for k in engine.LIN5], 0), out)
        cmp("gb5", g["b5"].reshape(5, Hp)[:, :H].reshape(-1), torch.cat([gg[pfx + k + ".bias"] for k in engine.LIN5], 0), out)
        cmp("gW3", g["W3"][:H, :H], gg[pfx + "B_3.weight"], out)
        cmp("gb3", g["b3"][:H], gg[pfx + "B_3.bias"], out)
        for a, b in (("gamma_e", "bn_e.weight"), ("beta_e", "bn_e.bias"), ("gamma_h", "bn_h.weight"), ("beta_h", "bn_h.bias")):
            cmp("g " + a, g[a][:H], gg[pfx + b], out)
    backward_rows(dbg, g64, rows)
    print("\n".join(f"{case} {name:12s} rel_l2={r:.3e} max_abs={m:.3e} ref_norm={nn:.3e}" for name, r, m, nn in rows))
    bad = [r for r in rows[:nfwd] if r[1] > 2e-5]
    assert not bad, f"forward mismatches: {bad}"
    miss = [r for r in rows[nfwd:] if not _grad_ok(r[1], r[2], 0.0)]
    if miss:
        # outside GRAD_L2: against the fp64 backward on the relu branches THIS layer took on the device (read from the kernels); the
        # other layers, the predictor and the encoder keep the oracle's own branches -- gh_out / ge_out do not depend on this layer's
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        a1_pre = c["args"][3] @ c["p64"]["linear1_edge.weight"].t() + c["p64"]["linear1_edge.bias"]
        masks = {"u": [dbg[i]["u"] > 0 for i in range(L)], "w": [dbg[i]["w"] > 0 for i in range(L)], "hid": dbg["hid"] > 0, "a1": a1_pre > 0}
        masks["u"][li], masks["w"][li] = um[inv][:, :H], wm[:, :H]
        with torch.no_grad():
            _, _, gx, dx = orc.manual_forward_backward(c["p64"], *c["args"], keep=True, masks=masks, batch_norm=False)
        assert torch.equal(dx[li]["gh_out"], d["gh_out"]) and torch.equal(dx[li]["ge_out"], d["ge_out"])
        xrows = []
        backward_rows(dx, gx, xrows)
        print("\n".join(f"{case} on the device's branches {name:12s} rel_l2={r:.3e} max_abs={m:.3e}" for name, r, m, nn in xrows))
        _branch_exact_or_fail(miss, {r[0]: r for r in xrows}, max(r[3] for r in xrows), f"{case} layer {li}")
    assert GRAD_L2 > BRANCH_L2


# -----------------------------------------------------------------------------------------
# the LayerNorm model's gradients on the device's own branches (the comparison a tensor outside GRAD_L2 falls back to)
# -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [32, 96, 128, 256])
def test_layernorm_gradients_exact_for_the_branch_taken(H):
    """The LayerNorm twin of test_gpu_parity.test_gradients_exact_for_the_branch_taken, which also keeps the fall-back of every
    LayerNorm gradient test exercised (no LayerNorm tensor of the suite currently misses GRAD_L2): helpers.branch_exact_rows /
    _branch_exact with batch_norm=False -- the relu branches read from the kernels (helpers.ln_layer_branches), the fp64 backward
    oracle.manual_forward_backward(batch_norm=False) on them -- must give every parameter gradient and d e_raw, d pe to fp32
    round-off (rel-L2 <= BRANCH_L2).  96 runs zero-padded on the 128-wide kernels."""
    from gnnome_assembly_amd import AssemblyGraph, synth
    from helpers import GRAD_ABS_FLOOR, _branch_exact, branch_exact_rows
    dev = _dev()
    L = 2
    src, dst, n = synth.make_graph(700, seed=H + L, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed=H)
    sd = synth.synth_state_dict(H, L, seed=L)
    pw = float(inp["pos_weight"])
    rows, gmax = branch_exact_rows(src, dst, n, inp["e"], inp["pe"], inp["y"], pw, sd, L, dev, False)
    print("\n".join(f"H={H} {name:28s} rel_l2={r:.3e} max_abs={m:.3e} ref_norm={nn:.3e}" for name, r, m, nn in rows))
    assert len(rows) == len(sd)
    bad = [r for r in rows if r[1] > BRANCH_L2 and r[2] > max(GRAD_ABS_FLOOR, 1e-6 * gmax)]
    assert not bad, bad
    g = AssemblyGraph(src, dst, n).to(dev)
    dev_e, dev_pe, want_e, want_pe = _branch_exact(g, sd, H, L, inp["e"], inp["pe"], inp["y"], pw, dev, False)
    assert rel_l2(dev_e.numpy(), want_e) <= BRANCH_L2 and rel_l2(dev_pe.numpy(), want_pe) <= BRANCH_L2
