"""The BatchNorm layer kernels (gnm_layer.hip, the finalisers, the H = 128 sweep forms of gnm_sweep.hip / gnm_fused.hip) one by one
against numpy fp64 on the same fp32 inputs, through the C ABI.

Every kernel of one layer runs on what the kernel before it left on the device, and is compared with tests/bn_reference.py's function
for that kernel evaluated on those same fp32 arrays (the stat / bstat rows included), so no kernel is charged with another's error.
Inputs: the column families of bn_reference (well conditioned; |mean| >> std; var << eps; constant; all-zero; one dominant row) mixed
across the H columns of every case, plus the saturated gate rows.  Sizes: a path with E = 1, RPW - 1, RPW, RPW + 1, 4 RPW - 1, 4 RPW,
4 RPW + 1, 15, 16, 17 edges (RPW = 256 / H rows per wave) and with as many NODES (N = E + 1), a one-node self loop (count = 1 on both
sides), a path long enough for several workgroups with a ragged last one, synth.tiny_edge_case_graph and the hub graph of
helpers.replica_base_graph -- with and without the residual pointers, at every built width.

Bounds (bn_reference): |err| <= c u A + u Rnd per element with c per column family = 4 x the worst ratio torch's fp32 CPU batch_norm /
autograd shows against the same reference functions (tools/measure_batchnorm_bounds.py -> profiles/batchnorm_kernel_bounds.json); sums
over edges / rows: the summed per-row bounds plus one u per fp32 addition; the `normal` columns also within the fixed bars (2e-5 rel-L2
forward, helpers.BRANCH_L2 backward).  torch's forward is exact for the all-zero column (x * alpha + beta with x = 0); ours is too
when there is no residual (relu(shift)), and is compared bit for bit there; with a residual the sum rounds once more, and the constant
column's t scale + shift rounds for every implementation: both get the `normal` constant.  The finalisers alone: their direct fp64 ->
fp32 outputs (mean, rstd, bstat, ggamma, gbeta) within 1 ulp of the fp64 value, scale bit-equal to float(gamma * rstd) of the rstd
written, shift within 1 ulp of beta - mean * scale of the mean / scale written plus the rounding of that product (u |mean scale|)
should the compiler not fuse it.  Every output buffer is NaN-filled with canary rows behind its end that must stay NaN; every chain
runs twice and must give the same bits.  Each test prints the worst fraction of its bound every output used ("bound used:")."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_reference as br
from bn_reference import FTZ, U, U64, f64
from helpers import BRANCH_L2, rel_l2, replica_base_graph

pytestmark = pytest.mark.gpu

FWD_L2 = 2e-5            # test_gpu_parity.test_layer_kernels_vs_oracle
CANARY = 3


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


_USED = {}


def _use(key, frac):
    _USED[key] = max(_USED.get(key, 0.0), float(np.max(frac)) if np.size(frac) else 0.0)


def _report():
    print("\n".join(f"bound used: {k:34s} {v:.3f}" for k, v in sorted(_USED.items())))


def _bounded(name, got, want, bound, key):
    got = f64(got)
    assert got.shape == want.shape and np.isfinite(got).all(), f"{name}: shape / non-finite"
    err = np.abs(got - want)
    bad = err > bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} elements outside the bound, worst err/bound "
                           f"{(err[bad] / np.maximum(bound[bad], 1e-300)).max():.3g} at {np.argwhere(bad)[:4].tolist()}")
    _use(key, err / np.maximum(bound, 1e-300))


def _frac_ok(name, frac, key):
    bad = frac > 1
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements outside the bound, worst {frac.max():.3g} at {np.argwhere(bad)[:4].tolist()}"
    _use(key, frac)


def _normal_l2(name, got, want, fam, bar):
    cols = fam == br.NORMAL
    if cols.any() and np.abs(want[:, cols]).sum() > 0:
        r = rel_l2(f64(got)[:, cols], want[:, cols])
        assert r <= bar, f"{name}: rel-L2 {r:.3e} > {bar:g} on the well-conditioned columns"


def _ulp32(x):
    return f64(np.spacing(np.abs(np.asarray(x, np.float32))))


class _Bufs:
    """NaN-filled device outputs with CANARY rows behind the end; take() returns the rows as numpy and checks the canary."""

    def __init__(self, dev):
        self.dev, self.t = dev, {}

    def new(self, name, rows, cols, init=None):
        b = torch.full((rows + CANARY, cols), float("nan"), dtype=torch.float32, device=self.dev)
        if init is not None:
            b[:rows] = torch.from_numpy(np.ascontiguousarray(init)).to(self.dev)
        self.t[name] = (b, rows)
        return b

    def take(self):
        out = {}
        for k, (b, rows) in self.t.items():
            a = b.cpu().numpy()
            assert np.isnan(a[rows:]).all(), f"{k}: rows behind the end were written"
            out[k] = a[:rows]
        return out


def _partial_rows(partials, nblk, H, lib):
    assert 1 <= nblk <= lib.gnm_max_partial_blocks(), f"nblk_out = {nblk}"
    return partials[:nblk * 2 * H].view(nblk, 2, H).cpu().numpy().copy()


def _graph(dev, src, dst, n):
    from gnnome_assembly_amd import AssemblyGraph
    g = AssemblyGraph(np.asarray(src, np.int32), np.asarray(dst, np.int32), int(n), node_order="keep").to(dev)
    idx = g.index()
    assert "nperm" not in idx
    return g, idx, {k: idx[k].cpu().numpy().astype(np.int64) for k in ("isrc", "idst", "in_ptr", "out_ptr", "out_pos", "out_dst")}


def _run_chain(dev, idx, d, N, E, H, resid, src_cap=0):
    """The separate passes of one layer, forward and backward, each on the previous kernel's device output."""
    from gnnome_assembly_amd import _lib, engine
    lib = _lib.load()
    p, st, call = engine._ptr, engine._stream(), engine._call
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    P, e_in, h_in, gh, ga_e, be_e, ga_h, be_h = (up(d[k]) for k in ("P", "e_in", "h_in", "gh_out", "gamma_e", "beta_e", "gamma_h", "beta_h"))
    null = C.c_void_p(0)
    b = _Bufs(dev)
    partials = engine.scratch(dev).partials
    nblk = C.c_int(0)
    rows = {}
    t = b.new("t", E, H, d["t_in"])
    call("gnm_edge_t_stats_fwd", E, H, p(t), p(P), p(idx["isrc"]), p(idx["idst"]), p(partials), C.byref(nblk), st)
    torch.cuda.synchronize()
    rows["t"] = _partial_rows(partials, nblk.value, H, lib)
    stat_e = b.new("stat_e", 4, H)
    call("gnm_bn_finalize", p(partials), nblk.value, E, H, p(ga_e), p(be_e), float(br.EPS), p(stat_e), st)
    e_out, hf, inv_f = b.new("e_out", E, H), b.new("hf", N, H), b.new("inv_f", N, H)
    call("gnm_edge_gate_fwd", N, E, H, p(t), p(e_in) if resid else null, p(stat_e), p(P), p(idx["isrc"]), p(idx["in_ptr"]), p(e_out), p(hf),
         p(inv_f), st)
    hb, inv_b, z = b.new("hb", N, H), b.new("inv_b", N, H), b.new("z", N, H)
    call("gnm_node_agg_src_fwd", N, E, H, p(e_out), p(P), p(idx["out_ptr"]), p(idx["out_pos"]), p(idx["out_dst"]), p(hf), p(hb), p(inv_b),
         p(z), p(partials), C.byref(nblk), st)
    torch.cuda.synchronize()
    rows["z"] = _partial_rows(partials, nblk.value, H, lib)
    stat_h = b.new("stat_h", 4, H)
    call("gnm_bn_finalize", p(partials), nblk.value, N, H, p(ga_h), p(be_h), float(br.EPS), p(stat_h), st)
    h_out = b.new("h_out", N, H)
    call("gnm_node_update_fwd", N, H, p(z), p(stat_h), p(h_in) if resid else null, p(h_out), st)
    # backward
    call("gnm_node_bwd_stats", N, H, p(z), p(stat_h), p(gh), p(partials), C.byref(nblk), st)
    torch.cuda.synchronize()
    rows["gw"] = _partial_rows(partials, nblk.value, H, lib)
    bstat_h, gg_h, gb_h = b.new("bstat_h", 2, H), b.new("gg_h", 1, H), b.new("gb_h", 1, H)
    call("gnm_bn_bwd_finalize", p(partials), nblk.value, N, H, p(bstat_h), p(gg_h), p(gb_h), st)
    gP, Q = b.new("gP", N, 5 * H), b.new("Q", N, 2 * H)
    call("gnm_node_bwd_apply", N, H, p(z), p(stat_h), p(bstat_h), p(ga_h), p(gh), p(inv_f), p(inv_b), p(gP), p(Q), st)
    ge, Ud, Td = b.new("ge", E, H, d["ge_out"]), b.new("Ud", N, H), b.new("Td", N, H)
    call("gnm_edge_bwd_dst", N, E, H, p(e_out), p(t), p(stat_e), p(ge), p(P), p(Q), p(hf), p(hb), p(idx["isrc"]), p(idx["in_ptr"]), p(gP),
         p(Ud), p(Td), p(partials), C.byref(nblk), st)
    torch.cuda.synchronize()
    rows["gu"] = _partial_rows(partials, nblk.value, H, lib)
    bstat_e, gg_e, gb_e = b.new("bstat_e", 2, H), b.new("gg_e", 1, H), b.new("gb_e", 1, H)
    call("gnm_bn_bwd_finalize", p(partials), nblk.value, E, H, p(bstat_e), p(gg_e), p(gb_e), st)
    call("gnm_edge_bwd_src", N, E, H, p(e_out), p(t), p(stat_e), p(bstat_e), p(ga_e), p(ge), p(Q), p(idx["in_ptr"]), p(idx["out_ptr"]),
         p(idx["out_pos"]), p(idx["out_dst"]), p(Ud), p(Td), p(gP), src_cap, st)
    gt = b.new("gt", E, H)
    call("gnm_edge_bwd_gt", E, H, p(ge), p(t), p(stat_e), p(bstat_e), p(ga_e), p(gt), st)
    torch.cuda.synchronize()
    out = b.take()
    out.update({"rows_" + k: v for k, v in rows.items()})
    return out, b


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.int64 if a[k].dtype == np.float64 else np.int32),
                              b[k].view(np.int64 if b[k].dtype == np.float64 else np.int32)), f"{what}: {k} differs between two runs"


def _check_rows(what, rows, sums, mags, und=None, key="partials"):
    """The partial rows summed in fp64 against the reference column sums: 2 nblk 2^-53 sum |x| (plus the undecided terms)."""
    got = f64(rows).sum(0)
    bound = 2 * rows.shape[0] * U64 * mags + (0.0 if und is None else und) + FTZ
    _bounded(f"{what} partial rows", got, sums, bound, key)
    return got


def _row_sums(rows):
    """The column sums of the partial rows (80-bit accumulation: exact to fp64) and what the finaliser's own fp64 summation may
    differ by: it adds the rows in 16 groups x 4 chains, then 3 + 16 more additions -- a depth of nblk / 64 + 24."""
    s = np.asarray(rows, np.longdouble).sum(0).astype(np.float64)
    return s, (rows.shape[0] / 64 + 24) * U64 * np.abs(f64(rows)).sum(0) + FTZ


def _check_finalize(what, out, name, rows, count, gamma, beta):
    """gnm_bn_finalize on the partial rows the device wrote."""
    s, slack = _row_sums(rows)
    mean, rstd = br.bn_finalize_ref(s, count)
    st = out[name]
    _bounded(f"{what} {name} mean", st[0], mean, _ulp32(st[0]) + slack[0] / count, "bn_finalize mean (ulp)")
    d_var = (slack[1] + 2 * np.abs(mean) * slack[0]) / count + 4 * U64 * (s[1] / count + mean * mean)
    _bounded(f"{what} {name} rstd", st[1], rstd, _ulp32(st[1]) + 0.5 * rstd ** 3 * d_var, "bn_finalize rstd (ulp)")
    assert np.array_equal(st[2], (gamma.astype(np.float32) * st[1]).astype(np.float32)), f"{what} {name}: scale is not float(gamma * rstd)"
    prod = f64(st[0]) * f64(st[2])
    _bounded(f"{what} {name} shift", st[3], f64(beta) - prod, _ulp32(st[3]) + U * np.abs(prod), "bn_finalize shift")


def _check_bwd_finalize(what, out, sfx, rows, count):
    s, slack = _row_sums(rows)
    bstat, gg, gb = br.bwd_finalize_ref(s, count)
    _bounded(f"{what} bstat{sfx}", out["bstat" + sfx], bstat, _ulp32(out["bstat" + sfx]) + slack / count, "bn_bwd_finalize (ulp)")
    _bounded(f"{what} ggamma{sfx}", out["gg" + sfx][0], gg, _ulp32(out["gg" + sfx][0]) + slack[1], "bn_bwd_finalize (ulp)")
    _bounded(f"{what} gbeta{sfx}", out["gb" + sfx][0], gb, _ulp32(out["gb" + sfx][0]) + slack[0], "bn_bwd_finalize (ulp)")


def _check_forward(what, o, d, ix, N, E, H, resid, cf, tag=""):
    """e_out (from t, stat_e), hf, inv_f, hb, inv_b, z of `o` against fp64 -- shared by the separate passes and the sweep."""
    fam = d["fam"]
    isrc, idst = ix["isrc"], ix["idst"]
    P = f64(d["P"])
    want, A, Rnd, und = br.bn_apply_ref(o["t"], o["stat_e"], d["e_in"] if resid else None)
    assert und.mean() <= br.UNDECIDED_CAP or und.sum() <= 1, f"{what}: {und.mean():.2%} undecided edge branches"
    d_e = br.apply_bound(A, Rnd, und, cf[fam])
    _bounded(f"{what} e_out", o["e_out"], want, d_e, tag + "edge_gate_fwd e_out")
    _normal_l2(f"{what} e_out", o["e_out"], want, fam, FWD_L2)
    zc = fam == br.FAMILIES.index("zero")
    if not resid and zc.any():      # the exact case: relu(shift)
        assert np.array_equal(o["e_out"][:, zc], np.broadcast_to(np.maximum(o["stat_e"][3][zc], 0), (E, int(zc.sum())))), f"{what}: zero columns"
    # the gate and the by-destination mean: sigma of the e_out the kernel holds (the stored one, bit for bit)
    zero = np.zeros_like(want)
    (hf, d_hf), (inv_f, d_inv) = br.gated_mean_ref(o["e_out"], zero, P[:, H:2 * H][isrc], idst, N)
    _bounded(f"{what} hf", o["hf"], hf, d_hf, tag + "edge_gate_fwd hf")
    _bounded(f"{what} inv_f", o["inv_f"], inv_f, d_inv, tag + "edge_gate_fwd inv_f")
    _normal_l2(f"{what} hf", o["hf"], hf, fam, FWD_L2)
    (hb, d_hb), (inv_b, d_invb) = br.gated_mean_ref(o["e_out"], zero, P[:, 2 * H:3 * H][idst], isrc, N)
    _bounded(f"{what} hb", o["hb"], hb, d_hb, tag + "node_agg_src_fwd hb")
    _bounded(f"{what} inv_b", o["inv_b"], inv_b, d_invb, tag + "node_agg_src_fwd inv_b")
    _normal_l2(f"{what} hb", o["hb"], hb, fam, FWD_L2)
    big = np.float32(1.0) / np.float32(1e-6)
    for nm, inv_nm, at in (("hf", "inv_f", idst), ("hb", "inv_b", isrc)):
        empty = np.bincount(at, minlength=N) == 0
        assert not o[nm][empty].any(), f"{what}: {nm} of an empty segment is not exactly 0"
        assert (o[inv_nm][empty] == big).all(), f"{what}: {inv_nm} of an empty segment is not 1 / 1e-6"
    # z from the hf the kernel read (separate passes: the stored one; the sweep holds the same value) and its own hb
    z, d_z = br.z_ref(P, o["hf"], 0.0, o["hb"], 0.0)
    _bounded(f"{what} z", o["z"], z, d_z + U * np.abs(z), tag + "node_agg_src_fwd z")
    return und


def _check_case(what, o, d, ix, N, E, H, resid, cf, cb):
    fam = d["fam"]
    isrc, idst = ix["isrc"], ix["idst"]
    P = f64(d["P"])
    # ---- gnm_edge_t_stats_fwd -> gnm_bn_finalize
    t, A, Rnd = br.t_stats_ref(d["t_in"], P, isrc, idst)
    _bounded(f"{what} t", o["t"], t, U * A + U * Rnd + FTZ, "edge_t_stats_fwd t")
    _normal_l2(f"{what} t", o["t"], t, fam, FWD_L2)
    sums, mags = br.col_sums(o["t"])
    _check_rows(f"{what} t", o["rows_t"], sums, mags)
    _check_finalize(what, o, "stat_e", o["rows_t"], E, d["gamma_e"], d["beta_e"])
    if E == 1:
        assert (o["stat_e"][1] == np.float32(1.0 / np.sqrt(np.float64(br.EPS)))).all(), f"{what}: count = 1, rstd is not 1 / sqrt(eps)"
    # ---- gnm_edge_gate_fwd, gnm_node_agg_src_fwd -> gnm_bn_finalize, gnm_node_update_fwd
    _check_forward(what, o, d, ix, N, E, H, resid, cf)
    sums, mags = br.col_sums(o["z"])
    _check_rows(f"{what} z", o["rows_z"], sums, mags)
    _check_finalize(what, o, "stat_h", o["rows_z"], N, d["gamma_h"], d["beta_h"])
    want, A, Rnd, und_h = br.bn_apply_ref(o["z"], o["stat_h"], d["h_in"] if resid else None)
    assert und_h.mean() <= br.UNDECIDED_CAP or und_h.sum() <= 1, f"{what}: {und_h.mean():.2%} undecided node branches"
    _bounded(f"{what} h_out", o["h_out"], want, br.apply_bound(A, Rnd, und_h, cf[fam]), "node_update_fwd h_out")
    _normal_l2(f"{what} h_out", o["h_out"], want, fam, FWD_L2)
    # ---- gnm_node_bwd_stats -> gnm_bn_bwd_finalize, gnm_node_bwd_apply
    pre, _, und = br.branch(o["z"], o["stat_h"])
    gw, zh = f64(d["gh_out"]) * (pre > 0), br.xhat32(o["z"], o["stat_h"])
    sums, mags = br.col_sums(gw, zh)
    gund = np.abs(f64(d["gh_out"])) * und
    _check_rows(f"{what} gw", o["rows_gw"], sums, mags, np.stack([gund.sum(0), (gund * np.abs(zh)).sum(0)]))
    _check_bwd_finalize(what, o, "_h", o["rows_gw"], N)
    frac, _ = br.either_branch(o["gP"][:, :H], o["z"], o["stat_h"], o["bstat_h"], d["gamma_h"], d["gh_out"], cb[fam])
    _frac_ok(f"{what} gz", frac, "node_bwd_apply gz")
    gz_ref = br.bn_bwd_apply_ref(o["z"], o["stat_h"], o["bstat_h"], d["gamma_h"], d["gh_out"], pre > 0)[0]
    if not und.any():
        _normal_l2(f"{what} gz", o["gP"][:, :H], gz_ref, fam, BRANCH_L2)
    for blk, inv in ((0, "inv_f"), (1, "inv_b")):
        frac, _ = br.either_branch(o["Q"][:, blk * H:(blk + 1) * H], o["z"], o["stat_h"], o["bstat_h"], d["gamma_h"], d["gh_out"], cb[fam],
                                   scale=f64(o[inv]))
        _frac_ok(f"{what} Q block {blk}", frac, "node_bwd_apply Q")
    _check_edge_backward(what, o, d, ix, N, E, H, cb)
    frac, und_e = br.either_branch(o["gt"], o["t"], o["stat_e"], o["bstat_e"], d["gamma_e"], o["ge"], cb[fam])
    _frac_ok(f"{what} gt", frac, "edge_bwd_gt gt")
    if not und_e.any():
        pre_e = br.branch(o["t"], o["stat_e"])[0]
        _normal_l2(f"{what} gt", o["gt"], br.bn_bwd_apply_ref(o["t"], o["stat_e"], o["bstat_e"], d["gamma_e"], o["ge"], pre_e > 0)[0], fam, BRANCH_L2)


def _check_edge_backward(what, o, d, ix, N, E, H, cb, tag="", UT=None):
    """The in-place ge, gP[:, H:5H], Ud, Td, the partial rows and gnm_bn_bwd_finalize's rows of `o` against fp64 -- shared by the
    separate passes (gnm_edge_bwd_dst, gnm_edge_bwd_src) and the sweep (gnm_edge_bwd_top + gnm_edge_bwd_src_fix + gnm_node_bgrad)."""
    fam = d["fam"]
    isrc, idst = ix["isrc"], ix["idst"]
    deg_in, deg_out = (np.bincount(a, minlength=N)[:, None].astype(np.float64) for a in (idst, isrc))
    (g, d_g), (a3, d_a3) = br.edge_bwd_dst_ref(o["e_out"], d["ge_out"], d["P"], o["Q"], o["hf"], o["hb"], isrc, idst)
    _bounded(f"{what} ge (in place)", o["ge"], g, d_g, tag + "edge_bwd_dst ge")
    _normal_l2(f"{what} ge", o["ge"], g, fam, BRANCH_L2)
    _bounded(f"{what} gA3h", o["gP"][:, 2 * H:3 * H], a3, d_a3, tag + "edge_bwd_dst gA3h")
    m = br.masked_sums_ref(o["ge"], o["t"], o["stat_e"], idst, N)
    _bounded(f"{what} Ud", o["Ud"], m["U"], m["d_U"], tag + "edge_bwd_dst Ud")
    _bounded(f"{what} Td", o["Td"], m["T"], m["d_T"], tag + "edge_bwd_dst Td")
    _check_rows(f"{what} gu", o["rows_gu"], m["sums"], m["mags"], m["sums_und"], key=tag + "partials")
    _check_bwd_finalize(what, o, "_e", o["rows_gu"], E)
    a2, d_a2 = br.gated_sum_ref(o["e_out"], f64(o["Q"])[:, :H][idst], isrc, N)
    _bounded(f"{what} gA2h", o["gP"][:, H:2 * H], a2, d_a2, tag + "edge_bwd_src gA2h")
    ms = br.masked_sums_ref(o["ge"], o["t"], o["stat_e"], isrc, N)
    if UT is not None:
        _bounded(f"{what} UT sum gu", UT[:, :H], ms["U"], ms["d_U"], tag + "UT")
        _bounded(f"{what} UT sum that", UT[:, H:], ms["T"], ms["d_T"], tag + "UT")
    st, bs, ga = o["stat_e"], o["bstat_e"], d["gamma_e"]
    c = np.abs(f64(ga) * f64(st[1]))[None, :]
    b1, d_b1 = br.bgrad_ref(ms["U"], ms["T"], deg_out, st, bs, ga)
    d_b1 = d_b1 + c * (ms["d_U"] + np.abs(f64(bs[1]))[None, :] * (ms["d_T"] + 2 * U * ms["absT"]))
    _bounded(f"{what} gB1h", o["gP"][:, 3 * H:4 * H], b1, d_b1, tag + "edge_bwd_src gB1h")
    b2, d_b2 = br.bgrad_ref(o["Ud"], o["Td"], deg_in, st, bs, ga)       # from the Ud / Td rows the kernel read
    _bounded(f"{what} gB2h", o["gP"][:, 4 * H:5 * H], b2, d_b2, tag + "edge_bwd_src gB2h")
    for k in (3, 4):
        _normal_l2(f"{what} gP block {k}", o["gP"][:, k * H:(k + 1) * H], (b1, b2)[k - 3], fam, BRANCH_L2) if not m["und"].any() else None


@pytest.mark.mode_independent
@pytest.mark.parametrize("H", br.WIDTHS)
def test_generic_kernels_vs_fp64(H):
    """gnm_edge_t_stats_fwd -> gnm_bn_finalize, gnm_edge_gate_fwd, gnm_node_agg_src_fwd -> gnm_bn_finalize, gnm_node_update_fwd,
    gnm_node_bwd_stats -> gnm_bn_bwd_finalize, gnm_node_bwd_apply, gnm_edge_bwd_dst -> gnm_bn_bwd_finalize, gnm_edge_bwd_src,
    gnm_edge_bwd_gt at every size of cases(H), with and without the residual pointers."""
    dev = _dev()
    c = br.load_constants()
    for i, (name, src, dst, n) in enumerate(br.cases(H)):
        g, idx, ix = _graph(dev, src, dst, n)
        N, E = n, len(src)
        d = br.make_layer_inputs(br.case_seed(H, i), ix, N, E, H)
        for resid in (True, False):
            what = f"H={H} {name} N={N} E={E}{'' if resid else ' no residual'}"
            o, _ = _run_chain(dev, idx, d, N, E, H, resid)
            o2, _ = _run_chain(dev, idx, d, N, E, H, resid, src_cap=1)      # max_blocks_per_cu = 1: the bits of the default
            _same(o, o2, what)
            _check_case(what, o, d, ix, N, E, H, resid, c["fwd"], c["bwd"])
    _report()


# -----------------------------------------------------------------------------------------
# (b) the finalisers alone
# -----------------------------------------------------------------------------------------

@pytest.mark.mode_independent
@pytest.mark.parametrize("H", [1, 18, 32, 100, 256])
def test_finalisers_on_hand_made_partials(H):
    """gnm_bn_finalize / gnm_bn_bwd_finalize at nblk = 1, 15, 16, 17, max and count = 1, 2, 7.5e6 against fp64; column 0 has exact
    variance 0 with a fp64 s2 / count - mean^2 slightly below 0: the clamp holds and rstd = 1 / sqrt(eps) to the ulp."""
    from gnnome_assembly_amd import _lib, engine
    dev = _dev()
    lib = _lib.load()
    p, st = engine._ptr, engine._stream()
    nmax = lib.gnm_max_partial_blocks()
    partials = engine.scratch(dev).partials
    rsq = 1.0 / np.sqrt(np.float64(br.EPS))
    for nblk in (1, 15, 16, 17, nmax):
        for count in (1, 2, 7500000):
            rng = np.random.default_rng(1000 * H + 10 * nblk + count % 7)
            ga, be = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
            # |mean| small enough that the fp64 cancellation of s2 / count - mean^2 stays below the fp32 ulp of rstd (the check is
            # then to the ulp); the last column, if any, with |mean| = 1e3 (the fp64 slack of _check_finalize decides there)
            m = rng.standard_normal(H) * np.exp(rng.uniform(-4, -1.5, H))
            m[-1] = 1e3 if H > 1 else m[-1]
            sd = np.exp(rng.uniform(-6, 2, H))
            s1, s2 = m * count, (m * m + (sd * sd if count > 1 else 0.0)) * count
            v = np.float64(np.float32(1234567.0))   # `count` equal rows of this value: variance 0, s1 = n v, s2 = n v^2
            s1[0], s2[0] = count * v, count * (v * v)
            rows = rng.dirichlet(np.ones(nblk), 2 * H).T.reshape(nblk, 2, H) * np.stack([s1, s2])[None]
            rows[:, :, 0] = np.stack([s1[0], s2[0]])[None] / nblk
            rows[-1, 1, 0] -= abs(s2[0]) * 2.0 ** -50       # the fp64 s2 / count - mean^2 of column 0 below 0 by more than eps
            partials[:nblk * 2 * H].copy_(torch.from_numpy(rows.reshape(-1)).to(dev))
            b = _Bufs(dev)
            stat, bstat, gg, gb = b.new("stat_e", 4, H), b.new("bstat_x", 2, H), b.new("gg_x", 1, H), b.new("gb_x", 1, H)
            ga_d, be_d = torch.from_numpy(ga).to(dev), torch.from_numpy(be).to(dev)
            engine._call("gnm_bn_finalize", p(partials), nblk, count, H, p(ga_d), p(be_d), float(br.EPS), p(stat), st)
            engine._call("gnm_bn_bwd_finalize", p(partials), nblk, count, H, p(bstat), p(gg), p(gb), st)
            torch.cuda.synchronize()
            o = b.take()
            what = f"H={H} nblk={nblk} count={count}"
            s, _ = _row_sums(rows)
            assert s[1, 0] / count - (s[0, 0] / count) ** 2 < -float(br.EPS), what
            assert o["stat_e"][1, 0] == np.float32(rsq), f"{what}: rstd of the variance-0 column is {o['stat_e'][1, 0]!r}, not 1 / sqrt(eps)"
            _check_finalize(what, o, "stat_e", rows, count, ga, be)
            _check_bwd_finalize(what, o, "_x", rows, count)
    _report()


# -----------------------------------------------------------------------------------------
# (c) the H = 128 sweep forms
# -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [128, 256])
def test_sweep_kernels_vs_fp64(H, matmul_mode):
    """gnm_edge_gate2_fwd and gnm_edge_bwd_top + gnm_edge_bwd_src_fix + gnm_node_bgrad (H = 256: two 128-column halves inside the
    library, as engine calls them) on the hub graph with both plans, on the inputs, against the reference and within the bounds of
    the separate passes; the no-grad form of the forward sweep gives the same bits; e_out equals gnm_edge_gate_fwd's bit for bit."""
    from gnnome_assembly_amd import _lib, engine
    dev = _dev()
    lib = _lib.load()
    c = br.load_constants()
    src, dst, n = replica_base_graph(reads=300, hub_in=300)
    g, idx, ix = _graph(dev, src, dst, n)
    N, E = n, len(src)
    plan2, plan = g.sweep_plan(dev, engine.GATE2_WG), g.sweep_plan(dev)
    for pl in (plan2, plan):
        assert pl is not None and 0 < pl["nfix"] < N, pl and pl["nfix"]
    d = br.make_layer_inputs(br.case_seed(H, br.SWEEP_CASE), ix, N, E, H)
    o, bufs = _run_chain(dev, idx, d, N, E, H, True)
    dv = {k: v[0] for k, v in bufs.t.items()}
    p, st, call = engine._ptr, engine._stream(), engine._call
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    P, e_in, ga_e = up(d["P"]), up(d["e_in"]), up(d["gamma_e"])
    partials = engine.scratch(dev).partials
    what = f"H={H} sweep N={N} E={E}"

    def forward(grad):
        b = _Bufs(dev)
        e_out, hf, hb, z = b.new("e_out", E, H), b.new("hf", N, H), b.new("hb", N, H), b.new("z", N, H)
        inv_f, inv_b = (b.new("inv_f", N, H), b.new("inv_b", N, H)) if grad else (None, None)
        nblk = C.c_int(0)
        call("gnm_edge_gate2_fwd", N, E, H, p(dv["t"]), p(e_in), p(dv["stat_e"]), p(P), p(idx["isrc"]), p(idx["idst"]), p(idx["in_ptr"]),
             p(plan2["sinfo"]), p(plan2["dinfo"]), plan2["nodes_per_block"], plan2["nfix"], p(plan2["fix_nodes"]), p(idx["out_ptr"]),
             p(idx["out_pos"]), p(idx["out_dst"]), p(e_out), p(hf), p(inv_f), p(hb), p(inv_b), p(z), p(partials), C.byref(nblk), st)
        torch.cuda.synchronize()
        r = b.take()
        r["rows_z"] = _partial_rows(partials, nblk.value, H, lib)
        return r

    f1, f2, f0 = forward(True), forward(True), forward(False)
    _same(f1, f2, what)
    for k in ("e_out", "hf", "hb", "z"):
        assert np.array_equal(f0[k].view(np.int32), f1[k].view(np.int32)), f"{what}: {k} of the no-grad form differs"
    assert np.array_equal(f1["e_out"].view(np.int32), o["e_out"].view(np.int32)), \
        f"{what}: e_out differs from gnm_edge_gate_fwd's (max {np.abs(f64(f1['e_out']) - f64(o['e_out'])).max():.3e})"
    _check_forward(what, dict(f1, t=o["t"], stat_e=o["stat_e"]), d, ix, N, E, H, True, c["fwd"], tag="sweep ")
    sums, mags = br.col_sums(f1["z"])
    _check_rows(f"{what} z", f1["rows_z"], sums, mags, key="sweep partials")

    def backward():
        b = _Bufs(dev)
        ge, gP = b.new("ge", E, H, d["ge_out"]), b.new("gP", N, 5 * H)
        UT, DT = b.new("UT", N, 2 * H), b.new("DT", N, 2 * H)
        Ud, Td = DT[:, :H], DT[:, H:]
        need = lib.gnm_edge_bwd_fused_workspace_bytes()
        ws = engine.scratch(dev).ws(need)
        nblk = C.c_int(0)
        call("gnm_edge_bwd_top", N, E, H, p(ge), p(dv["e_out"]), p(dv["t"]), p(dv["stat_e"]), p(P), p(dv["Q"]), p(dv["hf"]), p(dv["hb"]),
             p(idx["isrc"]), p(idx["idst"]), p(idx["in_ptr"]), p(gP), p(Ud), p(Td), p(partials), p(plan["sinfo"]), plan["nodes_per_block"],
             p(UT), C.byref(nblk), p(ws), need, st)
        call("gnm_edge_bwd_src_fix", plan["nfix"], p(plan["fix_nodes"]), N, E, H, p(dv["e_out"]), p(dv["t"]), p(dv["stat_e"]), p(ge), p(dv["Q"]),
             p(idx["out_ptr"]), p(idx["out_pos"]), p(idx["out_dst"]), p(gP), p(UT), st)
        torch.cuda.synchronize()
        rows = _partial_rows(partials, nblk.value, H, lib)
        bstat_e, gg_e, gb_e = b.new("bstat_e", 2, H), b.new("gg_e", 1, H), b.new("gb_e", 1, H)
        call("gnm_bn_bwd_finalize", p(partials), nblk.value, E, H, p(bstat_e), p(gg_e), p(gb_e), st)
        call("gnm_node_bgrad", N, H, p(dv["stat_e"]), p(bstat_e), p(ga_e), p(idx["in_ptr"]), p(idx["out_ptr"]), p(UT), p(Ud), p(Td),
             Ud.stride(0), p(gP), st)
        torch.cuda.synchronize()
        r = b.take()
        assert np.isnan(r["gP"][:, :H]).all(), f"{what}: the edge sweep wrote gP[:, 0:H] (the node kernel's block)"
        r.update(rows_gu=rows, Ud=r["DT"][:, :H], Td=r["DT"][:, H:])
        return r

    b1, b2 = backward(), backward()
    _same(b1, b2, what)
    ob = dict(o, **{k: b1[k] for k in ("ge", "gP", "Ud", "Td", "rows_gu", "bstat_e", "gg_e", "gb_e")})
    _check_edge_backward(what, ob, d, ix, N, E, H, c["bwd"], tag="sweep ", UT=b1["UT"])
    _report()
