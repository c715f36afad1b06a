"""The node projection entry points one by one against numpy fp64 on the same fp32 arrays, per element, at every tile edge, through
the C ABI: gnm_node_proj_fwd (rowtile_nt_k), gnm_node_proj_bwd_nn (rowtile_nn_group32_b3_k / rowtile_nn_acc_k),
gnm_node_proj_bwd_nn_stats (rowtile_nn2_k), gnm_node_proj_bwd_tn and gnm_tn128 (tn_tr_k / tn_colgroup_k + the slab and partial
reductions), gnm_tn128_bgrad (tn_tr_k<CONV>), gnm_node_proj_bwd (= its two halves).  tests/test_gpu_f16x2.py and test_gpu_bf16x3.py
hold the same kernels to the operand-scaling bars at the workload's size; sizes and edges live here.

Sizes (tests/node_proj_reference.py): N = 1, 2, 3, 31 .. 33, 63 .. 65, 127 .. 129, 255 .. 257, 511 .. 513 -- one short of, exactly and one past
one tile (32 rows; 64 in the f32 mode and the forward), a group of four tiles, and the 8 tiles from which on none of the 8 forced
slots ("empty slots write zero slabs") is empty; and per kernel an N, derived from the launch arithmetic and the CU count, at which
some workgroup walks two tiles (groups) and the last one is ragged.  For gnm_tn128_bgrad (two column groups: CUS * occupancy / 2
slots) that N lies past the contraction classes of profiles/gemm_bounds.json: integer families only there, everything by equality.
gnm_tn128 (5 ncg x 2 pitches per N) runs `ints` and `normal` at every N, `rows` and `cancel` at N = 1, 2, 3, 33, 129, 256, 513 (a third
of the file's time otherwise); every other entry runs every family at every N.

Checks, each on its own (the issue's numbering is kept in the function names' comments):
  ints       operands in [-8, 8]: every output bit-equal to fp64 in all three matmul modes (a dropped, doubled or misplaced tile, row
             or column group cannot pass); gnm_tn128_bgrad with rstd = gamma = 1, means 0 and with power-of-two gammas, integer means
  bound      normal / rows / cancel inside gemm_reference.bound per element: c(K) of profiles/gemm_bounds.json for K = 128 (NT),
             ncols (NN), N (TN), u_arith of the mode, one epilogue addition for the bias / the gh_out residual; gb / colsum (fp64 sums
             rounded once) within one fp32 ulp; the BatchNorm sums of _nn_stats from the fp32 gh_in the kernel wrote, in fp64, within
             (N + nblk) 2^-53 sum |terms| plus the undecided branches; the groups _bgrad forms within bn_reference.bgrad_ref's bound
  inside     every output NaN-filled with canary rows behind its end; `partials` NaN-filled: rows behind the launch's stay NaN;
             the workspace of the TN entries filled with 0xFF bytes (NaN) before every launch: a slab reduced but never written shows;
             NaN padding columns of a pitched A reach no output; gP[:, :3H] comes back from _bgrad bit-identical
  repeats    every call twice: the same bits; under gnm_set_occupancy_cap(1) / (2) (and max_blocks_per_cu 0 / 1 / 2 for _tn): the NT /
             NN outputs bit-equal (rows are independent), the TN outputs inside the bound and bit-equal on ints
  aliasing   engine.py never passes gh_in == gh_out (gh_in is a fresh buffer at every call site); what it does rely on: gnm_tn128 on
             gP with lda = 5H for the first three groups and on gP + 3H for the last two, and gnm_node_proj_bwd_nn reading the gP that
             gnm_tn128_bgrad just completed -- both forms are run here
  refusals   return -1, set gnm_last_error and leave the NaN-filled outputs untouched (host argument checks; nothing is launched)
The worst fraction of its bound every output used is printed ("bound used:") and written to node_proj_bound_used.txt in the
suite's run-report directory.

A contraction shorter than one 32-row tile (N < 32) runs the fp32-MFMA kernel in every matmul mode (tn_colgroups; gnm_tn128_bgrad
behind gnm_node_bgrad), so tn_tr_k never runs on a single short tile and N = 1 .. 31 tests the fp32 kernel in all three modes, held
to the fp32 bound (_tn_arith).  This file found why: at N = 1 (K = 1, c(1) = 1, a bound of 5 u / 2 u per product) tn_tr_k came out at 32 x
(gW, `rows`) and 38 x (_bgrad out) the bound in f16x2 and 1.2 x in bf16x3 -- f16x2 stages a row at a power-of-two multiple of its
LARGEST element, so an element 2^-k below it keeps 22 - k bits, bf16x3 keeps six of nine partial products (3 u dropped), and with
one product per element nothing larger hides either; the integer families were bit-equal.  N = 2, 3 (c(K) < 3) are run for that.

gnm_tn128_bgrad's `out` (and only it) is held to the `rows` family's constant for the `normal` inputs too: the contraction runs over
the nodes, and the hub's row (degree x m1) stands out of the formed groups -- the class's committed worst case, looser than `normal`'s.

Mutations tried on a scratch copy of the library, each caught by equality on integers or by a canary: rowtile_nn2_k skipping a ragged
tile, and its row guard as `<=` (test_node_proj_bwd_nn_stats); an empty slot of tn_tr_k leaving its slab unwritten
(test_node_proj_bwd_tn, N = 32); slabs reduced over the slot count of the uncapped occupancy (test_bwd_tn_several_tiles_per_slot); the
write-back of _bgrad one column group down (test_tn128_bgrad: gP[:, :3H]).

Not covered: an lda or a pointer that is no multiple of 4 floats (the kernels load float4; the entry points do not check it, the
engine never passes one)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import bn_reference as br
import gemm_reference as gr
import node_proj_reference as nr
from node_proj_reference import H, cdiv
from test_gpu_dp import _log

pytestmark = pytest.mark.gpu

CANARY = 3
NAN = float("nan")


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    from gnnome_assembly_amd import _lib
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


_USED = {}


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    txt = "\n".join(f"bound used: {k:44s} {v:.3f}" for k, v in sorted(_USED.items()))
    print("\n" + txt)
    _log("node_proj_bound_used.txt", txt + "\n")
    nr._CASES.clear()            # the operands and fp64 results of ~1000 cases: nothing for the rest of the session to carry
    gc.collect()                 # nor the launch closures (they hold device buffers) as cyclic garbage for a later test to trip over


class _Env:
    def __init__(self):
        from gnnome_assembly_amd import _lib, engine
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        self.lib, self.dev = _lib.load(), torch.device("cuda:0")
        self.p, self.st = engine._ptr, engine._stream()
        self.cus = self.lib.gnm_num_cus()
        assert self.cus == torch.cuda.get_device_properties(0).multi_processor_count
        self.nmax = self.lib.gnm_max_partial_blocks()
        assert self.nmax == nr.MAX_PARTIAL_BLOCKS
        self._ws = {}

    def up(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)          # (a copy: the cases are read-only)

    def ws(self, nbytes):
        if nbytes not in self._ws:
            self._ws = {nbytes: torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.dev)}
        return self._ws[nbytes]

    def partials(self):
        """The BatchNorm partials buffer (include/gnm.h: (gnm_max_partial_blocks() + 1) * 2 * 256 doubles), NaN-filled."""
        return torch.full(((self.nmax + 1) * 2 * 256,), NAN, dtype=torch.float64, device=self.dev)

    def err(self):
        return self.lib.gnm_last_error().decode(errors="replace")


class _Out:
    """[rows, cols] fp32 inside a NaN-filled buffer with CANARY rows behind its end."""

    def __init__(self, env, rows, cols, init=None):
        self.rows = rows
        self.t = torch.full((rows + CANARY, cols), NAN, dtype=torch.float32, device=env.dev)
        if init is not None:
            self.t[:rows] = env.up(init)

    def take(self, what):
        a = self.t.cpu().numpy()
        assert np.isnan(a[self.rows:]).all(), f"{what}: rows behind the end were written"
        return a[:self.rows].copy()

    def untouched(self):
        return bool(torch.isnan(self.t).all().item())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b, what):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def _use(key, frac):
    _USED[key] = max(_USED.get(key, 0.0), float(frac))


def _verify(what, fam, arith, K, got, want, absprod, epi, key):
    """gemm_reference.bound per element; the integer families by equality."""
    assert got.shape == want.shape, (got.shape, want.shape)
    if fam.startswith("ints"):
        bad = gr.f64(got) != want            # (a NaN -- padding read, or an element never written -- differs too)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the exact result, first at {np.argwhere(bad)[:4].tolist()}"
        return
    assert np.isfinite(got).all(), f"{what}: NaN / inf in the result (a read of padding, or an element not written)"
    b = gr.bound(arith, K, absprod, want, epi, family=fam)
    err = np.abs(gr.f64(got) - want)
    frac = float((err / np.maximum(b, 1e-300)).max())
    print(f"{what}: err/bound {frac:.3f}")
    _use(key, frac)
    assert (err <= b).all(), f"{what}: {int((err > b).sum())} of {err.size} elements outside the bound, worst err/bound {frac:.3g} at {np.argwhere(err > b)[:4].tolist()}"


def _verify_sums(what, fam, got, want, key):
    """gb / colsum: a fp64 sum rounded once -- equal on integers, else within one fp32 ulp of the fp64 column sum."""
    got = got.reshape(-1)
    assert got.shape == want.shape and np.isfinite(got).all(), f"{what}: shape / NaN"
    if fam.startswith("ints"):
        assert np.array_equal(gr.f64(got), want), f"{what}: column sums differ from the exact result at {np.argwhere(gr.f64(got) != want)[:4].tolist()}"
        return
    ulp = gr.f64(np.spacing(np.abs(got))) + br.FTZ
    frac = float((np.abs(gr.f64(got) - want) / ulp).max())
    _use(key, frac)
    assert frac <= 1, f"{what}: column sums off by {frac:.3g} ulp"


def _repeats_and_caps(env, what, launch, verify, rows_independent, variants=()):
    """check 4: twice the same bits; caps 1 and 2 (and the entry's own variants): bit-equal where rows are independent, verified
    always (the integer families: bit-equal to fp64 under every grid)."""
    g1, g2 = launch(), launch()
    _same(g1, g2, f"{what}: two runs")
    verify(g1, "")
    try:
        for cap in (1, 2):
            assert env.lib.gnm_set_occupancy_cap(cap) == 0
            gc = launch()
            if rows_independent:
                _same(g1, gc, f"{what}: occupancy cap {cap}")
            verify(gc, f" cap={cap}")
    finally:
        env.lib.gnm_set_occupancy_cap(0)
    for tag, kw in variants:
        verify(launch(**kw), f" {tag}")
    return g1


def _rows_written(partials, width):
    """How many leading `width`-double rows of the NaN-filled partials buffer a launch wrote (and that nothing behind them was)."""
    a = partials.cpu().numpy()
    a = a[:a.size // width * width].reshape(-1, width)
    written = ~np.isnan(a).any(1)
    n = int(written.sum())
    assert written[:n].all() and np.isnan(a[n:]).all(), "partials: rows written behind a NaN row / half-written rows"
    return n


# ---- launchers: each uploads once and returns launch(**kw) -> {name: numpy} --------------------------------------------------------

def _fwd(env, d, N, what, ncols=5 * H):
    h, W, b = env.up(d["h"]), env.up(d["W"]), env.up(d["b"])
    need = env.lib.gnm_rowtile_workspace_bytes(ncols)
    ws = env.ws(need)

    def launch():
        P = _Out(env, N, ncols)
        rc = env.lib.gnm_node_proj_fwd(N, H, ncols, env.p(h), env.p(W), env.p(b), env.p(P.t), env.p(ws), need, env.st)
        assert rc == 0, env.err()
        torch.cuda.synchronize()
        return dict(P=P.take(what))
    return launch


def _nn(env, d, N, ncols, what, stats=None, gP_dev=None):
    """stats = (z_lo, stat_h_lo): gnm_node_proj_bwd_nn_stats -> also partial rows [nblk, 2, H]."""
    gP = env.up(d["gP"]) if gP_dev is None else gP_dev
    W, gh = env.up(d["W"]), env.up(d["gh_out"])
    need = env.lib.gnm_rowtile_workspace_bytes(ncols)
    ws = env.ws(need)
    if stats is not None:
        z, st_h = env.up(stats[0]), env.up(stats[1])

    def launch():
        out = _Out(env, N, H)
        if stats is None:
            rc = env.lib.gnm_node_proj_bwd_nn(N, H, ncols, env.p(gP), env.p(W), env.p(gh), env.p(out.t), env.p(ws), need, env.st)
            assert rc == 0, env.err()
            torch.cuda.synchronize()
            return dict(gh_in=out.take(what))
        part, nblk = env.partials(), C.c_int(-1)
        rc = env.lib.gnm_node_proj_bwd_nn_stats(N, H, ncols, env.p(gP), env.p(W), env.p(gh), env.p(out.t), env.p(z), env.p(st_h),
                                                env.p(part), C.byref(nblk), env.p(ws), need, env.st)
        assert rc == 0, env.err()
        torch.cuda.synchronize()
        assert 1 <= nblk.value <= env.nmax, f"{what}: nblk_out = {nblk.value}"
        assert _rows_written(part, 2 * H) == nblk.value, f"{what}: partial rows written != nblk_out = {nblk.value}"
        return dict(gh_in=out.take(what), rows=part[:nblk.value * 2 * H].view(nblk.value, 2, H).cpu().numpy().copy())
    return launch


def _tn(env, d, N, ncols, what, slots=None):
    gP, h = env.up(d["gP"]), env.up(d["h_in"])
    need = env.lib.gnm_node_proj_bwd_workspace_bytes(ncols)
    ws = env.ws(need)

    def launch(mb=0):
        ws.fill_(0xFF)               # NaN in every float: a slab that is reduced but was never written shows
        gW, gb, part = _Out(env, ncols, H), _Out(env, 1, ncols), env.partials()
        rc = env.lib.gnm_node_proj_bwd_tn(N, H, ncols, env.p(gP), env.p(h), env.p(gW.t), env.p(gb.t), env.p(part), env.p(ws), need, mb, env.st)
        assert rc == 0, env.err()
        torch.cuda.synchronize()
        if slots is not None:
            slots[mb] = _rows_written(part, H) // (ncols // H)
        return dict(gW=gW.take(what), gb=gb.take(what))
    return launch


def _tn128(env, A_dev, a_off, lda, ncg, B, N, what, slots=None):
    """A_dev: the flat device buffer A lives in, a_off floats in."""
    Bd = env.up(B)
    need = env.lib.gnm_tn128_workspace_bytes()
    ws = env.ws(need)

    def launch():
        ws.fill_(0xFF)
        out, cs, part = _Out(env, ncg * H, H), _Out(env, 1, ncg * H), env.partials()
        rc = env.lib.gnm_tn128(N, C.c_void_p(A_dev.data_ptr() + 4 * a_off), lda, ncg, env.p(Bd), env.p(out.t), env.p(cs.t), env.p(part),
                               env.p(ws), need, env.st)
        assert rc == 0, env.err()
        torch.cuda.synchronize()
        if slots is not None:
            slots[0] = _rows_written(part, H) // ncg
        return dict(out=out.take(what), colsum=cs.take(what))
    return launch


def _check_nn(what, fam, mode, d, g, tag, key):
    _verify(f"{what}{tag} gh_in", fam, mode, d["K"], g["gh_in"], d["ref"], d["absprod"], d["epi"], key)


def _tn_arith(mode, N):
    """f32: tn_colgroup_k on fp32 MFMA -- which also runs a contraction shorter than one 32-row tile in the split modes; else tn_tr_k
    in the mode's own arithmetic."""
    return "f32" if N < 32 else mode


def _check_tn(what, fam, mode, d, g, tag, entry):
    arith = _tn_arith(mode, d["K"])
    _verify(f"{what}{tag} gW", fam, arith, d["K"], g["gW"], d["ref"], d["absprod"], None, f"{entry} gW/{mode}")
    _verify_sums(f"{what}{tag} gb", fam, g["gb"], d["cs"], f"{entry} gb (ulp)/{mode}")


def _check_stats(what, N, g, z, stat, key):
    """The partial rows of _nn_stats summed in fp64 against the sums formed from the fp32 gh_in the kernel wrote."""
    s = nr.stats_ref(g["gh_in"], z, stat)
    assert s["share"] <= br.UNDECIDED_CAP or s["n_und"] <= 1, f"{what}: {s['share']:.2%} undecided branches"
    got = gr.f64(g["rows"]).sum(0)
    assert np.isfinite(got).all(), f"{what}: NaN in the partial rows"
    bound = nr.stats_bound(s, N, g["rows"].shape[0])
    err = np.abs(got - s["sums"])
    frac = float((err / bound).max())
    _use(key, frac)
    assert (err <= bound).all(), f"{what}: BatchNorm sums outside the bound, worst {frac:.3g} at {np.argwhere(err > bound)[:4].tolist()}"


# ---- the edge sizes --------------------------------------------------------------------------------------------------------------
ALL_ROWS = nr.rows_for(64)                   # 8 x 32 = 256 is in ROWS already: one list for both tile heights


@pytest.mark.parametrize("N", ALL_ROWS)
def test_node_proj_fwd(matmul_mode, N):
    """P = h W^T + b, ncols = 640 (64-row tiles; split modes: one column group per workgroup, 8 forced slots per group)."""
    env = _Env()
    for fam in nr.families(H):
        d = nr.case("fwd", fam, N)
        what = f"fwd {matmul_mode} N={N} {fam}"
        _repeats_and_caps(env, what, _fwd(env, d, N, what),
                          lambda g, tag: _verify(f"{what}{tag} P", fam, matmul_mode, H, g["P"], d["ref"], d["absprod"], d["epi"],
                                                 f"node_proj_fwd P/{matmul_mode}"), rows_independent=True)


@pytest.mark.parametrize("ncols", [H, 3 * H, 5 * H])
@pytest.mark.parametrize("N", ALL_ROWS)
def test_node_proj_bwd_nn(matmul_mode, N, ncols):
    """gh_in = gh_out + gP W (groups of four 32-row tiles; f32: 64-row tiles)."""
    env = _Env()
    for fam in nr.families(ncols):
        d = nr.case("nn", fam, N, ncols)
        what = f"bwd_nn {matmul_mode} N={N} ncols={ncols} {fam}"
        _repeats_and_caps(env, what, _nn(env, d, N, ncols, what),
                          lambda g, tag: _check_nn(what, fam, matmul_mode, d, g, tag, f"node_proj_bwd_nn gh_in/{matmul_mode}"), rows_independent=True)


@pytest.mark.parametrize("ncols", [H, 5 * H])
@pytest.mark.parametrize("N", nr.rows_for(32))
def test_node_proj_bwd_nn_stats(matmul_mode, N, ncols):
    """gh_in as gnm_node_proj_bwd_nn and the BatchNorm_h backward sums of the layer below in `partials` / *nblk_out (split modes; the
    f32 mode refuses: test_refusals)."""
    if matmul_mode == "f32":
        return
    env = _Env()
    z, stat, _, _ = nr.lower_layer(N, seed=5)
    for fam in nr.families(ncols):
        d = nr.case("nn", fam, N, ncols)
        what = f"bwd_nn_stats {matmul_mode} N={N} ncols={ncols} {fam}"

        def verify(g, tag):
            _check_nn(what, fam, matmul_mode, d, g, tag, f"node_proj_bwd_nn_stats gh_in/{matmul_mode}")
            _check_stats(what + tag, N, g, z, stat, f"node_proj_bwd_nn_stats sums/{matmul_mode}")
            assert g["rows"].shape[0] % nr.XCDS == 0
        g = _repeats_and_caps(env, what, _nn(env, d, N, ncols, what, stats=(z, stat)), verify, rows_independent=False)
        # the rows are independent here too: gh_in keeps its bits under every grid (the partial rows need not)
        try:
            for cap in (1, 2):
                assert env.lib.gnm_set_occupancy_cap(cap) == 0
                gc = _nn(env, d, N, ncols, what, stats=(z, stat))()
                assert np.array_equal(_bits(gc["gh_in"]), _bits(g["gh_in"])), f"{what}: gh_in differs under occupancy cap {cap}"
                assert gc["rows"].shape[0] == nr.nn_grid(N, matmul_mode, env.cus, cap)[0], f"{what}: nblk_out under cap {cap}"
        finally:
            env.lib.gnm_set_occupancy_cap(0)


TN_VARIANTS = (("max_blocks_per_cu=1", dict(mb=1)), ("max_blocks_per_cu=2", dict(mb=2)))


@pytest.mark.parametrize("ncols", [H, 3 * H, 5 * H])
@pytest.mark.parametrize("N", ALL_ROWS)
def test_node_proj_bwd_tn(matmul_mode, N, ncols):
    """gW = gP^T h_in, gb = sum gP under max_blocks_per_cu 0, 1, 2 (8 forced slots per column group: at N < 8 tiles some are empty
    and must contribute zero slabs and zero partial rows)."""
    env = _Env()
    tile, slots = nr.tile_rows(matmul_mode), {}
    for fam in nr.families(N):
        d = nr.case("tn", fam, N, ncols)
        what = f"bwd_tn {matmul_mode} N={N} ncols={ncols} {fam}"
        _repeats_and_caps(env, what, _tn(env, d, N, ncols, what, slots),
                          lambda g, tag: _check_tn(what, fam, matmul_mode, d, g, tag, "node_proj_bwd_tn"), rows_independent=False,
                          variants=TN_VARIANTS)
    assert slots[1] == nr.tn_nslot(N, tile, ncols // H, env.cus, 1)[0], f"slots under max_blocks_per_cu = 1: {slots}"
    assert slots[0] >= slots[2] >= slots[1] >= nr.XCDS and slots[0] <= max(nr.XCDS, cdiv(N, tile))


@pytest.mark.parametrize("ncols", [3 * H, 5 * H])
@pytest.mark.parametrize("N", [1, 33, 129, 257, 513])
def test_node_proj_bwd_equals_its_halves(matmul_mode, N, ncols):
    """gnm_node_proj_bwd = gnm_node_proj_bwd_nn, then gnm_node_proj_bwd_tn with max_blocks_per_cu = 0: bit for bit."""
    env = _Env()
    for fam in ("ints", "normal"):
        dn, dt = nr.case("nn", fam, N, ncols), nr.case("tn", fam, N, ncols)
        what = f"bwd {matmul_mode} N={N} ncols={ncols} {fam}"
        gP, W, gh, h = env.up(dt["gP"]), env.up(dn["W"]), env.up(dn["gh_out"]), env.up(dt["h_in"])
        need = env.lib.gnm_node_proj_bwd_workspace_bytes(ncols)
        ws = env.ws(need)

        def launch():
            ws.fill_(0xFF)
            gh_in, gW, gb, part = _Out(env, N, H), _Out(env, ncols, H), _Out(env, 1, ncols), env.partials()
            rc = env.lib.gnm_node_proj_bwd(N, H, ncols, env.p(gP), env.p(h), env.p(W), env.p(gh), env.p(gh_in.t), env.p(gW.t), env.p(gb.t),
                                           env.p(part), env.p(ws), need, env.st)
            assert rc == 0, env.err()
            torch.cuda.synchronize()
            return dict(gh_in=gh_in.take(what), gW=gW.take(what), gb=gb.take(what))
        both, again = launch(), launch()
        _same(both, again, f"{what}: two runs")
        halves = dict(_nn(env, dict(dn, gP=dt["gP"]), N, ncols, what)(), **_tn(env, dt, N, ncols, what)())
        _same(both, halves, f"{what}: the two halves run separately")
        _check_tn(what, fam, matmul_mode, dt, both, "", "node_proj_bwd")
        ref = gr.ref(gr.NN, dt["gP"], dn["W"], None, dn["gh_out"])
        _verify(f"{what} gh_in", fam, matmul_mode, ncols, both["gh_in"], ref, gr.absprod(gr.NN, dt["gP"], dn["W"]),
                gr.epilogue(gr.NN, dt["gP"], dn["W"], None, dn["gh_out"]), f"node_proj_bwd gh_in/{matmul_mode}")


def _pitched(env, A, lda):
    """A [N, w] inside a NaN-filled flat buffer of row pitch lda (NaN padding columns, NaN behind the last row)."""
    N, w = A.shape
    flat = torch.full((N * lda + 64,), NAN, dtype=torch.float32, device=env.dev)
    torch.as_strided(flat, (N, w), (lda, 1), 0).copy_(env.up(A))
    return flat


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("ncg", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("N", ALL_ROWS)
def test_tn128(matmul_mode, N, ncg, pad):
    """out[cg] = A[:, cg]^T B, colsum = sum A per column group, lda = ncg 128 (+ 4: NaN padding columns), at every edge size."""
    env = _Env()
    tile = nr.tile_rows(matmul_mode)
    for fam in nr.families(N) if N in (1, 2, 3, 33, 129, 256, 513) else ("ints", "normal"):
        d = nr.case("tn", fam, N, ncg * H)
        what = f"tn128 {matmul_mode} N={N} ncg={ncg} lda={ncg * H + pad} {fam}"
        slots = {}
        flat = _pitched(env, d["gP"], ncg * H + pad)
        launch = _tn128(env, flat, 0, ncg * H + pad, ncg, d["h_in"], N, what, slots)
        _repeats_and_caps(env, what, lambda: {"gW": (g := launch())["out"], "gb": g["colsum"]},
                          lambda g, tag: _check_tn(what, fam, matmul_mode, d, g, tag, "tn128"), rows_independent=False)
        assert nr.XCDS <= slots[0] <= max(nr.XCDS, cdiv(N, tile)) and slots[0] * ncg <= env.nmax and slots[0] % nr.XCDS == 0, slots


@pytest.mark.parametrize("N", [33, 257, 513])
def test_tn128_on_the_engines_views_of_gP(matmul_mode, N):
    """check 5: gnm_tn128 as engine.py calls it -- the first three column groups of gP [N,5H] (lda = 5H, ncg = 3) and the last two
    (A = gP + 3H, lda = 5H, ncg = 2); the groups outside the call are NaN here and must not reach its outputs."""
    env = _Env()
    for fam in ("ints", "normal"):
        d = nr.case("tn", fam, N, 5 * H)
        for off, ncg in ((0, 3), (3 * H, 2)):
            gP = np.full((N, 5 * H), np.nan, np.float32)
            gP[:, off:off + ncg * H] = d["gP"][:, off:off + ncg * H]
            what = f"tn128 {matmul_mode} N={N} gP[:, {off}:{off + ncg * H}] {fam}"
            sub = dict(K=N, ref=d["ref"][off:off + ncg * H], absprod=d["absprod"][off:off + ncg * H], cs=d["cs"][off:off + ncg * H])
            launch = _tn128(env, env.up(gP).reshape(-1), off, 5 * H, ncg, d["h_in"], N, what)
            g1, g2 = launch(), launch()
            _same(g1, g2, f"{what}: two runs")
            _check_tn(what, fam, matmul_mode, sub, dict(gW=g1["out"], gb=g1["colsum"]), "", "tn128 (gP views)")


# ---- gnm_tn128_bgrad -----------------------------------------------------------------------------------------------------------------

def _graph_ptrs(env, N):
    from gnnome_assembly_amd import AssemblyGraph
    src, dst = nr.degrees_graph(N)
    g = AssemblyGraph(src.astype(np.int32), dst.astype(np.int32), int(N), node_order="keep").to(env.dev)
    idx = g.index()
    assert "nperm" not in idx
    ip, op = (idx[k].cpu().numpy().astype(np.int64) for k in ("in_ptr", "out_ptr"))
    assert np.array_equal(np.diff(ip), np.bincount(dst, minlength=N)) and np.array_equal(np.diff(op), np.bincount(src, minlength=N))
    if N >= 33:
        assert (np.diff(ip) == 0).any() and (np.diff(op) == 0).any() and np.diff(ip).max() >= N // 3 - 1      # degree 0 on either side, a hub
    return g, idx, ip, op


def _pattern(N):
    return (np.arange(N * 3 * H, dtype=np.float32).reshape(N, 3 * H) % 251) - 125


def _bgrad(env, d, N, idx, pitch, what, slots, keep):
    """gnm_tn128_bgrad on a gP whose first three groups hold _pattern(N) and whose last two are NaN."""
    UT, B = env.up(d["UT"]), env.up(d["h_in"])
    if pitch == H:
        Ud, Td = env.up(d["Ud"]), env.up(d["Td"])
    else:
        DT = env.up(np.concatenate([d["Ud"], d["Td"]], 1))
        Ud, Td = DT[:, :H], DT[:, H:]
    stat, bstat, ga = env.up(d["stat_e"]), env.up(d["bstat_e"]), env.up(d["gamma_e"])
    need = env.lib.gnm_tn128_workspace_bytes()
    ws = env.ws(need)
    init = np.concatenate([_pattern(N), np.full((N, 2 * H), np.nan, np.float32)], 1)

    def launch():
        ws.fill_(0xFF)
        gP = _Out(env, N, 5 * H, init)
        out, cs, part = _Out(env, 2 * H, H), _Out(env, 1, 2 * H), env.partials()
        rc = env.lib.gnm_tn128_bgrad(N, H, env.p(UT), env.p(Ud), env.p(Td), pitch, env.p(stat), env.p(bstat), env.p(ga),
                                     env.p(idx["in_ptr"]), env.p(idx["out_ptr"]), env.p(gP.t), env.p(B), env.p(out.t), env.p(cs.t),
                                     env.p(part), env.p(ws), need, env.st)
        assert rc == 0, env.err()
        torch.cuda.synchronize()
        slots[0] = _rows_written(part, H) // 2
        assert slots[0] % nr.XCDS == 0 and nr.XCDS <= slots[0] <= max(nr.XCDS, cdiv(N, 32)), slots
        keep["gP"] = gP
        return dict(gP=gP.take(what), out=out.take(what), colsum=cs.take(what))
    return launch


def _check_bgrad(what, fam, mode, N, d, r, val, dval):
    assert np.array_equal(_bits(r["gP"][:, :3 * H]), _bits(_pattern(N))), f"{what}: gP[:, :3H] was written"
    grp = r["gP"][:, 3 * H:]
    if fam.startswith("ints"):
        bad = gr.f64(grp) != val
        assert not bad.any(), f"{what}: {int(bad.sum())} group elements differ from the exact result, first at {np.argwhere(bad)[:4].tolist()}"
    else:
        assert np.isfinite(grp).all(), f"{what}: NaN in gP[:, 3H:5H] (a row or column group not written)"
        err = np.abs(gr.f64(grp) - val)
        _use(f"tn128_bgrad groups/{mode}", (err / dval).max())
        assert (err <= dval).all(), f"{what}: groups outside bgrad_ref's bound, worst {(err / dval).max():.3g} at {np.argwhere(err > dval)[:4].tolist()}"
    ref, ap, cs = nr.tn_from(grp, d["h_in"])            # from the fp32 groups the kernel wrote
    # the contraction runs over the rows and the hub's row (degree x m1) stands out of the formed groups: `normal` inputs too are
    # held to the heavy-tailed family's constant here (the class's committed worst case), not to the `normal` one
    fam_tn = fam if fam.startswith("ints") else "rows"
    _verify(f"{what} out", fam_tn, _tn_arith(mode, N), N, r["out"], ref, ap, None, f"tn128_bgrad out/{mode}")
    _verify_sums(f"{what} colsum", fam, r["colsum"], cs, f"tn128_bgrad colsum (ulp)/{mode}")


@pytest.mark.parametrize("N", nr.rows_for(32))
def test_tn128_bgrad(matmul_mode, N):
    """gB1h | gB2h formed from the raw sums in the operand load and written to gP[:, 3H:5H]; out / colsum = their weight and bias
    gradients, from the fp32 groups the kernel wrote; gP[:, :3H] untouched; ud_pitch = H (two arrays) and 2H (the halves of one);
    then gnm_node_proj_bwd_nn on the gP just completed, as the engine chains them (split modes; f32 refuses: test_refusals)."""
    if matmul_mode == "f32":
        return
    env = _Env()
    g, idx, ip, op = _graph_ptrs(env, N)
    for fam in ("ints", "ints2", "normal", "rows"):
        d = nr.bgrad_inputs(N, fam, seed=9)
        val, dval = nr.bgrad_groups_ref(d, ip, op)
        for pitch in (H, 2 * H):
            what = f"tn128_bgrad {matmul_mode} N={N} ud_pitch={pitch} {fam}"
            keep = {}
            r = _repeats_and_caps(env, what, _bgrad(env, d, N, idx, pitch, what, {}, keep),
                                  lambda r, tag: _check_bgrad(what + tag, fam, matmul_mode, N, d, r, val, dval), rows_independent=False)
            if pitch == H and fam in ("ints", "normal"):          # check 5: the projection backward reads the gP this call completed
                dn = nr.case("nn", fam, N, 5 * H)
                got = _nn(env, dn, N, 5 * H, what, gP_dev=keep["gP"].t[:N])()
                ref = gr.ref(gr.NN, r["gP"], dn["W"], None, dn["gh_out"])
                _verify(f"{what} -> bwd_nn gh_in", fam, matmul_mode, 5 * H, got["gh_in"], ref, gr.absprod(gr.NN, r["gP"], dn["W"]),
                        gr.epilogue(gr.NN, r["gP"], dn["W"], None, dn["gh_out"]), f"tn128_bgrad -> node_proj_bwd_nn gh_in/{matmul_mode}")


@pytest.mark.parametrize("pitch", [H, 2 * H])
def test_tn128_bgrad_several_tiles_per_slot(matmul_mode, pitch):
    """tn_tr_k<CONV> walking several tiles per slot (the prefetch clamped at the slot's last tile, the write-back of every tile, the
    f16x2 reference exponent carried from tile to tile), a ragged last one.  Two column groups: CUS * occupancy / 2 slots, so N lies
    past the contraction classes of profiles/gemm_bounds.json -- integer families only (small values, degrees <= 1: every sum stays
    below 2^24), everything by equality.  N from the occupancy's upper bound 8; the slot count really used is read back."""
    if matmul_mode == "f32":
        return
    env = _Env()
    N = nr.first_rows_with_two_items(32, lambda n: nr.tn_nslot(n, 32, 2, env.cus, 8)[1], 5)
    from gnnome_assembly_amd import AssemblyGraph
    src, dst = nr.degrees_graph(N, hub=False)
    idx = AssemblyGraph(src.astype(np.int32), dst.astype(np.int32), int(N), node_order="keep").to(env.dev).index()
    ip, op = (idx[k].cpu().numpy().astype(np.int64) for k in ("in_ptr", "out_ptr"))
    assert np.diff(ip).max() == 1 and np.diff(op).max() == 1 and (np.diff(ip) == 0).any()
    for fam in ("ints", "ints2"):
        d = nr.bgrad_inputs(N, fam, seed=10, small=True)
        val, dval = nr.bgrad_groups_ref(d, ip, op)
        assert (np.abs(val).T @ np.abs(gr.f64(d["h_in"]))).max() < 2 ** 24
        what = f"tn128_bgrad {matmul_mode} N={N} ud_pitch={pitch} {fam}"
        slots = {}
        launch = _bgrad(env, d, N, idx, pitch, what, slots, {})
        r1, r2 = launch(), launch()
        assert cdiv(cdiv(N, 32), slots[0]) >= 2, f"{what}: {slots[0]} slots for {cdiv(N, 32)} tiles -- no slot walks two tiles"
        _same(r1, r2, f"{what}: two runs")
        _check_bgrad(what, fam, matmul_mode, N, d, r1, val, dval)


# ---- several tiles (groups) per workgroup, a ragged last one ----------------------------------------------------------------------

MULTI_FAMILIES = ("ints", "normal")


def test_fwd_several_tiles_per_workgroup(matmul_mode):
    env = _Env()
    if matmul_mode == "f32":                 # persistent_grid(ntiles, 2, occ) under cap 1
        N = nr.first_rows_with_two_items(64, lambda n: nr.nn_grid(n, "f32", env.cus, 1)[1], 5)
        per = nr.nn_grid(N, "f32", env.cus, 1)[1]
    else:                                    # no cap reaches this launch: the slot count at the largest occupancy
        N = nr.fwd_nslot_max(env.cus) * 64 + 64 + 5
        per = cdiv(cdiv(N, 64), nr.fwd_nslot_max(env.cus))       # a LOWER bound of the launch's own value (it cannot be read back):
        #                                                          a smaller occupancy only takes slots away
    assert per >= 2 and N % 64 == 5, (N, per)
    try:
        assert env.lib.gnm_set_occupancy_cap(1) == 0
        for fam in MULTI_FAMILIES:
            d = nr.case("fwd", fam, N)
            what = f"fwd {matmul_mode} N={N} ({per} tiles per workgroup) {fam}"
            g = _fwd(env, d, N, what)()
            _verify(f"{what} P", fam, matmul_mode, H, g["P"], d["ref"], d["absprod"], d["epi"], f"node_proj_fwd P/{matmul_mode}")
    finally:
        env.lib.gnm_set_occupancy_cap(0)


@pytest.mark.parametrize("stats", [False, True])
def test_bwd_nn_several_groups_per_workgroup(matmul_mode, stats):
    if stats and matmul_mode == "f32":
        return
    env = _Env()
    rows = nr.nn_grid(1, matmul_mode, env.cus, 1)[2]
    N = nr.first_rows_with_two_items(rows, lambda n: nr.nn_grid(n, matmul_mode, env.cus, 1)[1], 37)     # the last group: one tile and 5 rows
    grid, per, _ = nr.nn_grid(N, matmul_mode, env.cus, 1)
    assert per >= 2 and N % 32 == 5, (N, grid, per)
    z, stat, _, _ = nr.lower_layer(N, seed=6)
    try:
        assert env.lib.gnm_set_occupancy_cap(1) == 0
        for fam in MULTI_FAMILIES:
            d = nr.case("nn", fam, N, 5 * H)
            what = f"bwd_nn{'_stats' if stats else ''} {matmul_mode} N={N} ({per} per workgroup, grid {grid}) {fam}"
            g = _nn(env, d, N, 5 * H, what, stats=(z, stat) if stats else None)()
            _check_nn(what, fam, matmul_mode, d, g, "", f"node_proj_bwd_nn{'_stats' if stats else ''} gh_in/{matmul_mode}")
            if stats:
                assert g["rows"].shape[0] == grid, f"{what}: nblk_out = {g['rows'].shape[0]}, the derived grid is {grid}"
                _check_stats(what, N, g, z, stat, f"node_proj_bwd_nn_stats sums/{matmul_mode}")
    finally:
        env.lib.gnm_set_occupancy_cap(0)


def test_bwd_tn_several_tiles_per_slot(matmul_mode):
    """ncols = 640 under max_blocks_per_cu = 1: CUS / 5 slots (rounded down to 8) per column group.  N gives every such slot two
    tiles and one slot a third, ragged one -- twice as many tiles as slots, so that any larger occupancy (max_blocks_per_cu = 2, 0)
    plans MORE slots than the capped launch: a reduction over another slot count than the launch's own then reads slabs that were
    never written (the workspace is NaN-filled) or leaves written ones out."""
    env = _Env()
    tile = nr.tile_rows(matmul_mode)
    nslot = nr.tn_nslot(10 ** 6, tile, 5, env.cus, 1)[0]
    N = 2 * nslot * tile + 5
    assert nr.tn_nslot(N, tile, 5, env.cus, 1) == (nslot, 3) and N <= 8192, (N, nslot)
    assert env.cus < 40 or nr.tn_nslot(N, tile, 5, env.cus, 2)[0] > nslot
    for fam in MULTI_FAMILIES + ("rows",):
        d = nr.case("tn", fam, N, 5 * H)
        what = f"bwd_tn {matmul_mode} N={N} (3 tiles per slot, {nslot} slots) {fam}"
        slots = {}
        launch = _tn(env, d, N, 5 * H, what, slots)
        for mb in (1, 2, 0):
            g = launch(mb=mb)
            _check_tn(what, fam, matmul_mode, d, g, f" max_blocks_per_cu={mb}", "node_proj_bwd_tn")
        assert slots[1] == nslot and cdiv(cdiv(N, tile), slots[1]) >= 2, f"{what}: the launch wrote {slots[1]} slots per group"
        assert slots[0] >= slots[2] >= slots[1], slots


def test_tn128_several_tiles_per_slot(matmul_mode):
    """ncg = 16: at most 2048 / 16 = 128 slots whatever the occupancy; the slot count really used is read back from the partial rows."""
    env = _Env()
    tile = nr.tile_rows(matmul_mode)
    # f32: tn_colgroup_k holds two 64 x 132 fp32 images (66 KB of the CU's 160 KB LDS): at most 2 workgroups per CU
    bpc = 2 if matmul_mode == "f32" else 8       # (f32: an estimate, not measured -- the read-back below is what asserts)
    N = nr.first_rows_with_two_items(tile, lambda n: nr.tn_nslot(n, tile, 16, env.cus, bpc)[1], 5)
    assert N <= 8192, N
    for fam in MULTI_FAMILIES:
        d = nr.case("tn", fam, N, 16 * H)
        what = f"tn128 {matmul_mode} N={N} ncg=16 {fam}"
        slots = {}
        g = _tn128(env, _pitched(env, d["gP"], 16 * H + 4), 0, 16 * H + 4, 16, d["h_in"], N, what, slots)()
        assert cdiv(cdiv(N, tile), slots[0]) >= 2, f"{what}: {slots[0]} slots for {cdiv(N, tile)} tiles -- no slot walks two tiles"
        _check_tn(what, fam, matmul_mode, d, dict(gW=g["out"], gb=g["colsum"]), "", "tn128")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(matmul_mode):
    """check 6.  Host argument checks only: every call below is refused before anything is launched."""
    env = _Env()
    lib, p, st, null = env.lib, env.p, env.st, C.c_void_p(0)
    N, nc = 33, 5 * H
    g, idx, _, _ = _graph_ptrs(env, N)
    t = lambda *s: torch.ones(*s, device=env.dev)  # noqa: E731
    h, W, b, gP, gh, z, stat = t(N, H), t(nc, H), t(nc), t(N, nc), t(N, H), t(N, H), t(4, H)
    UT, Ud, Td, bstat, ga = t(N, 2 * H), t(N, H), t(N, H), t(2, H), t(H)
    A16 = t(N, 16 * H)
    outs = dict(P=_Out(env, N, nc), gh_in=_Out(env, N, H), gW=_Out(env, nc, H), gb=_Out(env, 1, nc), gPo=_Out(env, N, nc),
                out16=_Out(env, 16 * H, H), cs16=_Out(env, 1, 16 * H))
    part = env.partials()
    nblk = C.c_int(-7)
    need_rt, need_bw, need_tn = lib.gnm_rowtile_workspace_bytes(nc), lib.gnm_node_proj_bwd_workspace_bytes(nc), lib.gnm_tn128_workspace_bytes()
    ws = torch.empty(max(need_rt, need_bw, need_tn) + 64, dtype=torch.uint8, device=env.dev)
    o = {k: p(v.t) for k, v in outs.items()}
    entries = {
        "gnm_node_proj_fwd": (dict(N=N, H=H, ncols=nc, h=p(h), W=p(W), b=p(b), P=o["P"], ws=p(ws), wsb=need_rt, st=st), need_rt),
        "gnm_node_proj_bwd_nn": (dict(N=N, H=H, ncols=nc, gP=p(gP), W=p(W), gh_out=p(gh), gh_in=o["gh_in"], ws=p(ws), wsb=need_rt, st=st), need_rt),
        "gnm_node_proj_bwd_nn_stats": (dict(N=N, H=H, ncols=nc, gP=p(gP), W=p(W), gh_out=p(gh), gh_in=o["gh_in"], z_lo=p(z), stat_h_lo=p(stat),
                                            partials=p(part), nblk_out=C.pointer(nblk), ws=p(ws), wsb=need_rt, st=st), need_rt),
        "gnm_node_proj_bwd_tn": (dict(N=N, H=H, ncols=nc, gP=p(gP), h_in=p(h), gW=o["gW"], gb=o["gb"], partials=p(part), ws=p(ws), wsb=need_bw,
                                      mb=0, st=st), need_bw),
        "gnm_node_proj_bwd": (dict(N=N, H=H, ncols=nc, gP=p(gP), h_in=p(h), W=p(W), gh_out=p(gh), gh_in=o["gh_in"], gW=o["gW"], gb=o["gb"],
                                   partials=p(part), ws=p(ws), wsb=need_bw, st=st), need_bw),
        "gnm_tn128": (dict(N=N, A=p(A16), lda=16 * H, ncg=16, B=p(h), out=o["out16"], colsum=o["cs16"], partials=p(part), ws=p(ws), wsb=need_tn,
                           st=st), need_tn),
        "gnm_tn128_bgrad": (dict(N=N, H=H, UT=p(UT), Ud=p(Ud), Td=p(Td), ud_pitch=H, stat_e=p(stat), bstat_e=p(bstat), gamma_e=p(ga),
                                 in_ptr=p(idx["in_ptr"]), out_ptr=p(idx["out_ptr"]), gP=o["gPo"], B=p(h), out=o["gW"], colsum=o["gb"],
                                 partials=p(part), ws=p(ws), wsb=need_tn, st=st), need_tn),
    }
    split_only = ("gnm_node_proj_bwd_nn_stats", "gnm_tn128_bgrad")
    count = [0]

    def refused(entry, why, **over):
        base = entries[entry][0]
        lib.gnm_set_occupancy_cap(9)                  # (refused itself: leaves a message no entry point below produces)
        marker = env.err()
        rc = getattr(lib, entry)(*dict(base, **over).values())
        msg = env.err()
        torch.cuda.synchronize()
        assert rc == -1, f"{entry} ({why}): rc = {rc}, {msg!r}"
        assert msg and msg != marker and entry[4:] in msg, f"{entry} ({why}): gnm_last_error = {msg!r}"
        for k, v in outs.items():
            assert v.untouched(), f"{entry} ({why}): {k} was written"
        assert torch.isnan(part).all().item() and nblk.value == -7, f"{entry} ({why}): partials / nblk_out were written"
        count[0] += 1

    f32 = matmul_mode == "f32"
    for entry, (base, need) in entries.items():
        if entry in split_only and f32:
            refused(entry, "f32 mode")                # every other argument in order
            continue
        if "H" in base:
            refused(entry, "H = 64", H=64)
        if "ncols" in base:
            refused(entry, "ncols = 130", ncols=130)
            refused(entry, "ncols = 0", ncols=0)
        refused(entry, "N = 0", N=0)
        refused(entry, "N < 0", N=-1)
        refused(entry, "workspace one byte short", wsb=need - 1)
        for k, v in base.items():
            if isinstance(v, C.c_void_p) and k != "st":
                refused(entry, f"{k} = NULL", **{k: null})
        if "nblk_out" in base:
            refused(entry, "nblk_out = NULL", nblk_out=None)
    refused("gnm_node_proj_fwd", "ncols = 512", ncols=4 * H)
    refused("gnm_node_proj_bwd_tn", "max_blocks_per_cu = -1", mb=-1)
    refused("gnm_tn128", "ncg = 17", ncg=17, lda=17 * H)
    refused("gnm_tn128", "ncg = 0", ncg=0)
    refused("gnm_tn128", "lda < ncg * 128", lda=16 * H - 4)
    if not f32:
        refused("gnm_tn128_bgrad", "ud_pitch = 3H", ud_pitch=3 * H)
        refused("gnm_tn128_bgrad", "ud_pitch = 0", ud_pitch=0)
    assert count[0] >= 60
    # and the same calls with everything in order run
    for entry, (base, _) in entries.items():
        if not (entry in split_only and f32):
            assert getattr(lib, entry)(*base.values()) == 0, f"{entry}: {env.err()}"
    torch.cuda.synchronize()
    assert np.array_equal(outs["P"].take("P"), np.full((N, nc), float(H + 1), np.float32))
    assert np.array_equal(outs["gh_in"].take("gh_in"), np.full((N, H), float(nc + 1), np.float32))
    assert np.array_equal(outs["out16"].take("out16"), np.full((16 * H, H), float(N), np.float32))
    assert np.array_equal(outs["cs16"].take("cs16"), np.full((1, 16 * H), float(N), np.float32))
