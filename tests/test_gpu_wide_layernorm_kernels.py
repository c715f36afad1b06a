"""The kernels of the LayerNorm layers wider than 256 channels (gnm_ln_wide_* in gnm_layernorm.hip) through the C ABI against fp64 on
the same fp32 inputs, driven chunk by chunk exactly as engine._wide_ln_layer_forward / _wide_ln_layer_backward drive them (phase A
of every chunk in ascending order before phase B of any).

Shapes (padded width, width): (512, 512) two full chunks, (512, 320) a half-dead last chunk, (768, 600) three chunks, (512, 257) one
live channel in the last chunk.  Rows: the six families of tests/ln_reference.py, 6 x 40 of them (edge cases: one row per edge).
Reference, bound parts and checks are those of tests/test_gpu_layernorm_kernels.py -- its _edge_case runs unchanged on the full-width
arrays assembled from the chunks, so every output of the separate-pass kernels (relu(u), e_out, hf, inv_f, the in-place ge, gt,
gP[:, H:5H], the column sums; dead channels exactly 0; gP[:, 0:H] left alone) is held to the same componentwise bounds -- with the
family constants measured AT THESE SHAPES: tools/measure_layernorm_bounds.py --wide (torch's fp32 CPU layer_norm / autograd /
native_layer_norm statistics against fp64) -> profiles/layernorm_wide_kernel_bounds.json, the device gets DEVICE_FACTOR = 4 x those
ratios, and a family whose CPU result is exact must be exact on the device.  Row statistics: |err| <= c u A + u Rnd with
measure_layernorm_bounds.stat_bound (mean: A = max|x|, Rnd = |mean|; rstd: A = rstd X, Rnd = 3 rstd for the roundings of var + eps, the
square root and the division).  Every kernel runs twice: the second run is bit-identical."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import ln_reference as lr
import test_gpu_layernorm_kernels as base
from helpers import BRANCH_L2
from ln_reference import U

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_BOUNDS_FILE = os.path.join(REPO, "profiles", "layernorm_wide_kernel_bounds.json")
SHAPES = [(512, 512), (512, 320), (768, 600), (512, 257)]
ROWS = 6 * 40
W = 256         # engine.WIDE_CHUNK


def _tool():
    spec = importlib.util.spec_from_file_location("measure_layernorm_bounds", os.path.join(REPO, "tools", "measure_layernorm_bounds.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _wide_constants():
    """(fwd c, bwd c, fwd_exact, stat c) per family: DEVICE_FACTOR x the CPU ratios measured at the wide shapes."""
    d = json.load(open(WIDE_BOUNDS_FILE))
    assert [tuple(s) for s in d["shapes"]] == SHAPES and d["device_factor"] == lr.DEVICE_FACTOR
    c = {k: np.array([lr.DEVICE_FACTOR * d["cpu_fp32_ratio"][k][f] for f in lr.FAMILIES]) for k in ("fwd", "bwd", "stat")}
    exact = np.array([bool(d["cpu_fp32_exact"]["fwd"][f]) for f in lr.FAMILIES])
    return c["fwd"], c["bwd"], exact, c["stat"]


def _stack(x):
    """[R, 256 C] -> the contiguous [C, R, 256] stack of chunk copies."""
    R, Hp = x.shape
    return x.view(R, Hp // W, W).permute(1, 0, 2).contiguous()


def _unstack(chunks, blocks=1):
    """C chunk tensors [R, blocks*256] -> [R, blocks * 256 C] in the full-width block layout (engine._put_cols)."""
    R = chunks[0].shape[0]
    return torch.stack([c.view(R, blocks, W) for c in chunks], 2).reshape(R, blocks * W * len(chunks))


def _row_stats(stack, width):
    from gnnome_assembly_amd import engine
    stat = torch.full((stack.shape[1], 2), float("nan"), dtype=torch.float32, device=stack.device)
    engine._call("gnm_ln_wide_row_stats", stack.shape[1], stack.shape[0], engine._ptr(stack), stack.shape[1] * W, width, engine._ptr(stat),
                 engine._stream())
    return stat


def _check_stat(what, stat, x, ga, be, width, fam, key):
    want, A, Rnd = _tool().stat_bound(x, lr.ln_ref(x, ga, be, width))
    base._use(key, lr.check(f"{what} stat (mean, rstd)", base._np(stat), want, A, Rnd, _wide_constants()[3][fam]))


# -----------------------------------------------------------------------------------------
# node side: gnm_ln_wide_row_stats, gnm_ln_wide_node_update_fwd, gnm_ln_wide_node_bwd_sums / _apply
# -----------------------------------------------------------------------------------------

def _run_node(dev, N, Hp, width, z, ga, be, gh, h_in, hf, inv_f, hb, inv_b):
    from gnnome_assembly_amd import engine
    p, st = engine._ptr, engine._stream()
    f32 = dict(dtype=torch.float32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), **f32)  # noqa: E731
    nc = Hp // W
    zs = _stack(z)
    # every chunk copy is made once and held to the end: a temporary handed to p() is freed, and its memory reused, before the launch
    ghc, h_inc, hfc, inv_fc, hbc, inv_bc = ([a[:, ci * W:(ci + 1) * W].clone() for ci in range(nc)] for a in (gh, h_in, hf, inv_f, hb, inv_b))
    zero = torch.zeros(N, W, **f32)
    stat = _row_stats(zs, width)
    relu_w, h_out, gPs, Qs = [], [], [], []
    gg, gb, red = nan(Hp), nan(Hp), nan(2, Hp)
    rowsum = nan(N, 2)
    partials = engine.scratch(dev).partials
    nblk = C.c_int(0)
    for ci in range(nc):
        sl = slice(ci * W, (ci + 1) * W)
        for res, outs in ((zero, relu_w), (h_inc[ci], h_out)):
            outs.append(nan(N, W))
            engine._call("gnm_ln_wide_node_update_fwd", N, p(zs[ci]), p(stat), p(ga[sl]), p(be[sl]), p(res), p(outs[-1]), ci * W, width, st)
    for ci in range(nc):            # phase A of every chunk, ascending
        sl = slice(ci * W, (ci + 1) * W)
        engine._call("gnm_ln_wide_node_bwd_sums", N, p(zs[ci]), p(stat), p(ga[sl]), p(be[sl]), p(ghc[ci]), p(rowsum), p(partials),
                     C.byref(nblk), ci * W, width, st)
        r = torch.empty(2, W, **f32)
        engine._call("gnm_reduce_partials", p(partials), nblk.value, 2, W, p(r), st)
        red[:, sl] = r
        engine.bn_bwd_finalize(partials, nblk.value, N, W, dev, gg[sl], gb[sl])
    for ci in range(nc):            # phase B
        sl = slice(ci * W, (ci + 1) * W)
        gPs.append(nan(N, 5 * W)), Qs.append(nan(N, 4 * W))
        engine._call("gnm_ln_wide_node_bwd_apply", N, p(zs[ci]), p(stat), p(ga[sl]), p(be[sl]), p(ghc[ci]), p(rowsum), p(hfc[ci]),
                     p(inv_fc[ci]), p(hbc[ci]), p(inv_bc[ci]), p(gPs[-1]), p(Qs[-1]), ci * W, width, st)
    torch.cuda.synchronize()
    return dict(stat=stat, relu_w=_unstack(relu_w), h_out=_unstack(h_out), gP=_unstack(gPs, 5), Q=_unstack(Qs, 4), red=red, gg=gg, gb=gb,
                rowsum=rowsum)


@pytest.mark.parametrize("Hp,width", SHAPES)
def test_wide_node_kernels_vs_fp64(Hp, width):
    """stat_h, relu(w), h_out, gz = gP[:, 0:Hp], the four blocks of Q and the column sums against fp64; dead channels exactly 0; the
    rest of gP untouched.  One row (a lone wave), and 6 x 40 rows."""
    dev = base._dev()
    cf, cb, exact_f, _ = _wide_constants()
    for N in (1, ROWS):
        rng = np.random.default_rng(100000 * Hp + 1000 * width + N)
        z, fam = lr.make_rows(rng, N, Hp, width, first=Hp + width)
        ga, be = lr.make_affine(rng, Hp, width)
        live = np.arange(Hp) < width
        gh, h_in, hf, hb = ((rng.standard_normal((N, Hp)) * live).astype(np.float32) for _ in range(4))
        inv_f, inv_b = (np.exp(rng.uniform(-2, 2, (N, Hp))).astype(np.float32) for _ in range(2))
        args = [torch.from_numpy(a).to(dev) for a in (z, ga, be, gh, h_in, hf, inv_f, hb, inv_b)]
        out = _run_node(dev, N, Hp, width, *args)
        what = f"Hp={Hp} width={width} N={N}"
        base._same(out, _run_node(dev, N, Hp, width, *args), what)
        _check_stat(what, out["stat"], z, ga, be, width, fam, "wide_node stat_h")
        ref = lr.ln_ref(z, ga, be, width)
        A, Rnd = lr.fwd_bound(ref)
        relu_w, want = base._np(out["relu_w"]), np.maximum(ref["pre"], 0)
        base._use("wide_node relu(w)", lr.check(f"{what} relu(w)", relu_w, want, A, Rnd, cf[fam], exact_f[fam]))
        base._normal_l2(f"{what} relu(w)", relu_w, want, fam, base.FWD_L2)
        h_out = want + h_in.astype(np.float64)
        base._bounded(f"{what} h_out", base._np(out["h_out"]), h_out, cf[fam][:, None] * U * A + U * (Rnd + np.abs(h_out)), "wide_node h_out")
        gw = gh.astype(np.float64) * (relu_w > 0)            # the device's own branches
        gz, Ab, Rb = lr.ln_bwd_ref(ref, gw)
        gP, Q = base._np(out["gP"]), base._np(out["Q"])
        assert np.isnan(gP[:, Hp:]).all(), f"{what}: gnm_ln_wide_node_bwd_apply wrote outside gP[:, 0:256] of a chunk"
        base._use("wide_node gz", lr.check(f"{what} gz", gP[:, :Hp], gz, Ab, Rb, cb[fam]))
        base._normal_l2(f"{what} gz", gP[:, :Hp], gz, fam, BRANCH_L2)
        f64 = np.float64
        i_f, i_b = inv_f.astype(f64), inv_b.astype(f64)
        blocks = (("Qf", i_f, 2, 1.0), ("Rf", i_f * np.abs(hf.astype(f64)), 3, hf.astype(f64)), ("Qb", i_b, 2, 1.0),
                  ("Rb", i_b * np.abs(hb.astype(f64)), 3, hb.astype(f64)))
        for b, (nm, scale, nr, sg) in enumerate(blocks):
            wantq = gz * (i_f if b < 2 else i_b) * sg
            base._use("wide_node Q", lr.check(f"{what} {nm}", Q[:, b * Hp:(b + 1) * Hp], wantq, Ab * scale, nr * np.abs(wantq), cb[fam]))
            base._normal_l2(f"{what} {nm}", Q[:, b * Hp:(b + 1) * Hp], wantq, fam, BRANCH_L2)
        base._column_checks(f"{what} finalize", out["gb"], out["gg"], gw, ref, fam, cf, key="wide_node")
        base._column_checks(f"{what} reduce", out["red"][0], out["red"][1], gw, ref, fam, cf, key="wide_node")
        base._dead_zero(f"{what} relu(w)", relu_w, Hp, width)
        base._dead_zero(f"{what} h_out", base._np(out["h_out"]), Hp, width)
        base._dead_zero(f"{what} gz", gP[:, :Hp], Hp, width)
        base._dead_zero(f"{what} Q", Q, Hp, width, 4)
        base._dead_zero(f"{what} column sums", np.stack([base._np(out["gb"]), base._np(out["gg"]), *base._np(out["red"])]), Hp, width)
    base._report("wide_node")


# -----------------------------------------------------------------------------------------
# edge side: gnm_ln_wide_row_stats, gnm_ln_wide_edge_gate_fwd, gnm_ln_wide_edge_bwd_sums / _apply, then gnm_ln_edge_bwd_src per chunk
# -----------------------------------------------------------------------------------------

_STATS = []         # (stat_e, t, gamma, beta, width) of the runs of the current case, for the statistics check


def _run_edge(dev, idx, N, E, Hp, width, t, e_in, ga, be, P, Q, ge0):
    """The wide twin of test_gpu_layernorm_kernels._run_edge: same inputs (full width), same outputs (full width)."""
    from gnnome_assembly_amd import engine
    p, st = engine._ptr, engine._stream()
    f32 = dict(dtype=torch.float32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), **f32)  # noqa: E731
    nc = Hp // W
    cols = lambda a, ci, blocks=1: engine._cols(a, ci * W, W, blocks)  # noqa: E731
    ts = _stack(t)
    stat = _row_stats(ts, width)
    _STATS.append((stat, t, ga, be, width))
    # chunk copies and scratch outputs are held to the end: a temporary handed to p() is freed, and its memory reused, before the launch
    Pc, Qc = [cols(P, ci, 5) for ci in range(nc)], [cols(Q, ci, 4) for ci in range(nc)]
    e_inc = [cols(e_in, ci).clone() for ci in range(nc)]
    zero, junk = torch.zeros(E, W, **f32), [nan(N, W), nan(N, W)]
    relu_u, e_out, hf, inv_f, ge, gt, gPs = [], [], [], [], [], [], []
    gg, gb = nan(Hp), nan(Hp)
    rowsum = nan(E, 2)
    partials = engine.scratch(dev).partials
    nblk = C.c_int(0)
    for ci in range(nc):
        sl = slice(ci * W, (ci + 1) * W)
        relu_u.append(nan(E, W)), e_out.append(nan(E, W)), hf.append(nan(N, W)), inv_f.append(nan(N, W))
        engine._call("gnm_ln_wide_edge_gate_fwd", N, E, p(ts[ci]), p(zero), p(ga[sl]), p(be[sl]), p(stat), p(Pc[ci]),
                     p(idx["isrc"]), p(idx["in_ptr"]), p(relu_u[-1]), p(junk[0]), p(junk[1]), ci * W, width, st)
        engine._call("gnm_ln_wide_edge_gate_fwd", N, E, p(ts[ci]), p(e_inc[ci]), p(ga[sl]), p(be[sl]), p(stat), p(Pc[ci]),
                     p(idx["isrc"]), p(idx["in_ptr"]), p(e_out[-1]), p(hf[-1]), p(inv_f[-1]), ci * W, width, st)
    for ci in range(nc):            # phase A of every chunk, ascending
        sl = slice(ci * W, (ci + 1) * W)
        ge.append(cols(ge0, ci).clone()), gPs.append(nan(N, 5 * W))
        engine._call("gnm_ln_wide_edge_bwd_sums", N, E, p(e_out[ci]), p(ts[ci]), p(stat), p(ga[sl]), p(be[sl]), p(ge[ci]), p(Pc[ci]), p(Qc[ci]),
                     p(idx["isrc"]), p(idx["in_ptr"]), p(gPs[ci]), p(rowsum), p(partials), C.byref(nblk), ci * W, width, st)
        engine.bn_bwd_finalize(partials, nblk.value, E, W, dev, gg[sl], gb[sl])
    for ci in range(nc):            # phase B, then the by-source pass
        sl = slice(ci * W, (ci + 1) * W)
        gt.append(nan(E, W))
        engine._call("gnm_ln_wide_edge_bwd_apply", N, E, p(ts[ci]), p(stat), p(ga[sl]), p(be[sl]), p(ge[ci]), p(rowsum), p(idx["in_ptr"]),
                     p(gt[ci]), p(gPs[ci]), ci * W, width, st)
        engine._call("gnm_ln_edge_bwd_src", N, E, W, p(e_out[ci]), p(gt[ci]), p(Qc[ci]), p(idx["out_ptr"]), p(idx["out_pos"]),
                     p(idx["out_dst"]), p(gPs[ci]), st)
    torch.cuda.synchronize()
    u = _unstack
    return dict(relu_u=u(relu_u), e_out=u(e_out), hf=u(hf), inv_f=u(inv_f), ge=u(ge), gP=u(gPs, 5), gt=u(gt), gg=gg, gb=gb, stat=stat)


@pytest.mark.parametrize("Hp,width", SHAPES)
def test_wide_edge_kernels_vs_fp64(Hp, width, monkeypatch):
    """On synth.tiny_edge_case_graph (nodes without in- or out-edges, self loops, duplicates, hubs) and a synth.make_graph(300, ...):
    stat_e against fp64, and test_gpu_layernorm_kernels._edge_case -- every forward and backward output of the separate passes,
    no element left out, each kernel run twice -- on the wide runner with the constants measured at the wide shapes."""
    from gnnome_assembly_amd import AssemblyGraph, synth
    dev = base._dev()
    monkeypatch.setattr(base, "_run_edge", _run_edge)
    monkeypatch.setattr(base, "_constants", lambda: _wide_constants()[:3])
    for k, (src, dst, n) in enumerate((synth.tiny_edge_case_graph(), synth.make_graph(300, seed=Hp + width))):
        g = AssemblyGraph(src, dst, n, node_order="keep").to(dev)
        del _STATS[:]
        base._edge_case(dev, g, Hp, width, seed=7 * Hp + width + k, tag="wide_edge")
        assert len(_STATS) == 2 and torch.equal(_STATS[0][0].view(torch.int32), _STATS[1][0].view(torch.int32)), "stat_e differs between two runs"
        stat, t, ga, be, w_ = _STATS[0]
        t = t.cpu().numpy()
        # the rows' families, as _edge_case drew them
        _, fam = lr.make_rows(np.random.default_rng(7 * Hp + width + k), t.shape[0], Hp, width, first=7 * Hp + width + k)
        _check_stat(f"Hp={Hp} width={width} graph {k}", stat, t, ga.cpu().numpy(), be.cpu().numpy(), w_, fam, "wide_edge stat_e")
    base._report("wide_edge")


def test_wide_entry_points_validate_their_arguments():
    """c0 < 0, c0 % 4 != 0 and width < 1 are refused before anything is launched."""
    from gnnome_assembly_amd import _lib, engine
    dev = base._dev()
    z = torch.zeros(1, 4, W, device=dev)
    stat, v = torch.zeros(4, 2, device=dev), torch.zeros(W, device=dev)
    p = engine._ptr
    for c0, width in ((-4, 300), (2, 300), (0, 0)):
        with pytest.raises(_lib.GnmError):
            engine._call("gnm_ln_wide_node_update_fwd", 4, p(z), p(stat), p(v), p(v), None, p(torch.empty(4, W, device=dev)), c0, width,
                         engine._stream())
    with pytest.raises(_lib.GnmError):
        engine._call("gnm_ln_wide_row_stats", 4, 1, p(z), 4 * W, 257, p(stat), engine._stream())        # width beyond the C chunks
