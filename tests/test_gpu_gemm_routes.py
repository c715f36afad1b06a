"""gnm_gemm_f32 / gnm_gemm_tn_colsum per element against numpy fp64 (tests/gemm_reference.py) on every route of the dispatcher, at
the edges of each route's predicates, through engine.gemm / engine.gemm_tn_colsum (refusals: through ctypes).

Routes (gnm_gemm.hip, gemm_b3_try in gnm_fused.hip; the predicates below restate what was read there):
    skinny   TN, no epilogue, M == 128, 1 <= N <= 32, K >= 4096, A 16-byte aligned with lda % 4 == 0   tn_skinny128_k<1|2> + finish
    b3       split matmul modes only.  TN: K >= 4096, M % 128 == N % 128 == 0, (M/128)(N/128) <= 64, no epilogue, A, B and C aligned
             (tn_tr_k + slab_reduce_ld_k);  NT / NN: M >= 2048, N % 128 == K % 128 == 0, (N/128)(K/128) <= 256, A, C, resid aligned,
             bias 16-byte aligned (gemm_rows_b3_k; B goes through the pack kernels' element loads)
    general  everything else: gemm_f32_k<AR,BR> (float4 loads of an aligned operand on interior tiles, element loads otherwise);
             TN in 2+ k-splits (plan_split: >= 16 k-tiles of 32 per split) + splitk_reduce_k
general and skinny run fp32 MFMA arithmetic in every matmul mode, b3 the mode's own: the bound takes u_arith accordingly.

Every case: operands inside NaN-filled device buffers with NaN padding columns (ld > width) in A, B and resid -- a read past K or
past a row would poison the result; C NaN-filled with canary rows behind and canary columns on both sides.  `ints` must be bit-equal
to the fp64 result, `normal`, `rows` and `cancel` inside gemm_reference.bound per element (c(K) from profiles/gemm_bounds.json).
Each call runs twice (same bits), then under gnm_set_occupancy_cap(1) and (2): `ints` still bit-equal, the others inside the bound.
The worst fraction of the bound per (route, arithmetic) is printed ("bound used:") and written to gemm_bound_used.txt in the
suite's run-report directory (test_gpu_dp._log).

Not covered: the class limits of the b3 route for NT / NN ((N/128)(K/128) = 257 needs a 2048 x 32896 operand)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

import gemm_reference as gr
from gemm_reference import NN, NT, TN
from test_gpu_dp import _log

pytestmark = pytest.mark.gpu

CANARY = 3
SKN_BYTES = 1024 * (128 * 32 + 128) * 8          # the skinny route's workspace: kSkinnyMaxBlocks partial rows of fp64
BK, MIN_KTILES = 32, 16                          # plan_split: k-tile, least k-tiles per split


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    from gnnome_assembly_amd import _lib
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _lib_():
    from gnnome_assembly_amd import _lib
    return _lib.load()


# ---- layouts -----------------------------------------------------------------------------------------------------------------
# *_off: floats between the 16-byte aligned buffer and the operand; *_pad: ld - width (None: up to the next multiple of 4, + 4);
# c_off / r_off = 1: one float in and an odd leading dimension (0: four floats in, ld % 4 == 0)
Lay = namedtuple("Lay", "a_off a_pad b_off b_pad c_off r_off", defaults=(0, None, 0, None, 0, 0))
ALIGNED = Lay()
LAYOUTS = {"a+1": Lay(a_off=1), "lda=K+1": Lay(a_pad=1), "lda=K+4": Lay(a_pad=4), "b+1": Lay(b_off=1), "ldb+1": Lay(b_pad=1),
           "ldb+4": Lay(b_pad=4), "c+1,odd ldc": Lay(c_off=1), "r+1,odd ldr": Lay(r_off=1), "all": Lay(1, 1, 1, 1, 1, 1)}


def _ld(width, pad):
    return (width + 3) // 4 * 4 + 4 if pad is None else width + pad


def _al(off, ld):
    return off % 4 == 0 and ld % 4 == 0


def _operand(dev, data, off, pad):
    """`data` [rows, width] inside a NaN buffer: (view, off, ld)."""
    rows, width = data.shape
    ld = _ld(width, pad)
    flat = torch.full((off + rows * ld + 64,), float("nan"), dtype=torch.float32, device=dev)       # NaN behind the last row as well
    v = torch.as_strided(flat, (rows, width), (ld, 1), off)
    v.copy_(torch.from_numpy(np.array(data, dtype=np.float32)))
    v.ptr = flat.data_ptr() + 4 * off          # (an empty view -- K = 0 -- has no data_ptr of its own)
    assert (v.ptr % 16 == 0) == (off % 4 == 0) and v.stride(0) == ld and (v.numel() == 0 or v.data_ptr() == v.ptr)
    return v


class _Out:
    """[M, N] inside a NaN buffer of M + CANARY rows: `left` canary columns before, at least 2 behind."""

    def __init__(self, dev, M, N, off):
        self.M, self.N = M, N
        self.left = 1 if off else 4
        self.ld = ((N + 3) | 1) if off else (N + 3) // 4 * 4 + 8
        self.flat = torch.full(((M + CANARY) * self.ld + 8,), float("nan"), dtype=torch.float32, device=dev)
        self.view = torch.as_strided(self.flat, (M, N), (self.ld, 1), self.left)
        assert (self.view.data_ptr() % 16 == 0) == (off == 0) and (self.ld % 2 == 1) == bool(off) and self.ld >= self.left + N + 2

    def take(self, what):
        a = self.flat.cpu().numpy()
        tail, a = a[(self.M + CANARY) * self.ld:], a[:(self.M + CANARY) * self.ld].reshape(self.M + CANARY, self.ld)
        inside = np.zeros(a.shape, bool)
        inside[:self.M, self.left:self.left + self.N] = True
        assert np.isnan(a[~inside]).all() and np.isnan(tail).all(), f"{what}: written outside C (canary rows / columns)"
        return a[:self.M, self.left:self.left + self.N].copy()


# ---- the dispatcher's predicates, restated ----------------------------------------------------------------------------------------

def plan_split(mode, M, N, K, cus):
    if mode != TN or K == 0:
        return 1
    tiles = -(-M // 128) * -(-N // 128)
    ktiles = -(-K // BK)
    want = max(1, min(-(-cus * 4 // tiles), -(-ktiles // MIN_KTILES), 1024))
    per = -(-ktiles // want)
    return -(-ktiles // per)


def skinny_shape(M, N, K):
    return M == 128 and 1 <= N <= 32 and K >= 4096


def b3_shape(mm, mode, M, N, K):
    if mm == "f32":
        return False
    if mode == TN:
        return K >= 4096 and M > 0 and N > 0 and M % 128 == 0 and N % 128 == 0 and (M // 128) * (N // 128) <= 64
    return M >= 2048 and N > 0 and K > 0 and N % 128 == 0 and K % 128 == 0 and (N // 128) * (K // 128) <= 256


def route_of(mm, mode, M, N, K, epi, lay, cus):
    """(route, arithmetic) the dispatcher takes for this call (engine.gemm always passes the workspace asked for)."""
    wa, wb = gr.shapes(mode, M, N, K)
    a_al, b_al = _al(lay.a_off, _ld(wa[1], lay.a_pad)), _al(lay.b_off, _ld(wb[1], lay.b_pad))
    c_al, r_al = lay.c_off == 0, lay.r_off == 0
    if mode == TN and not epi and skinny_shape(M, N, K) and a_al:
        return "skinny", "f32"
    if b3_shape(mm, mode, M, N, K) and a_al:
        if (mode == TN and not epi and b_al and c_al) or (mode != TN and c_al and (r_al or not epi)):
            return "b3", mm
    return ("splitk" if plan_split(mode, M, N, K, cus) > 1 else "general"), "f32"


# ---- running one case ------------------------------------------------------------------------------------------------------------

_HOST = {}


def _host(fam, mode, M, N, K, epi):
    """Operands and fp64 results of a case, computed once for all matmul modes and layouts and never changed."""
    key = (fam, mode, M, N, K, epi)
    if key not in _HOST:
        A, B, bias, resid = gr.operands(fam, mode, M, N, K, seed=1 + 7 * mode + M + 3 * N + 5 * K, epi=epi)
        d = dict(A=A, B=B, bias=bias, resid=resid, ref=gr.ref(mode, A, B, bias, resid, epi), absprod=gr.absprod(mode, A, B),
                 epi=gr.epilogue(mode, A, B, bias, resid) if epi else None)
        if mode == TN:
            d["cs"], d["csabs"] = gr.colsum_ref(A)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _HOST[key] = d
    return _HOST[key]


_USED = {}


def _families(K):
    """`ints` first: an element dropped, doubled or taken from the wrong place is reported as such, not as a bound missed."""
    return ["ints"] + [f for f in gr.FAMILIES if f != "ints" and K > 0 and (f != "cancel" or gr.uses_cancel(K))]


def _verify(what, fam, arith, K, got, want, absprod, epi, key):
    assert got.shape == want.shape
    if fam == "ints":
        bad = gr.f64(got) != want            # (a NaN -- padding read, or an element never written -- differs too)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the exact result, first at {np.argwhere(bad)[:4].tolist()}"
        return
    assert np.isfinite(got).all(), f"{what}: NaN / inf in the result (a read of padding, or an element not written)"
    b = gr.bound(arith, K, absprod, want, epi, family=fam)
    err = np.abs(gr.f64(got) - want)
    frac = float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0
    _USED[key] = max(_USED.get(key, 0.0), frac)
    assert (err <= b).all(), f"{what}: {int((err > b).sum())} of {err.size} elements outside the bound, worst err/bound {frac:.3g}"


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run_case(mm, mode, M, N, K, epi=False, lay=ALIGNED, colsum=False, expect=None, families=None):
    from gnnome_assembly_amd import engine
    dev, lib = _dev(), _lib_()
    route, arith = route_of(mm, mode, M, N, K, epi, lay, lib.gnm_num_cus())
    if expect is not None:
        assert route == expect, f"the case was built for the {expect} route, the predicates say {route}"
    key = f"{route}{'+colsum' if colsum else ''}/{arith}"
    for fam in families or _families(K):
        h = _host(fam, mode, M, N, K, epi)
        what = f"{gr.MODE_NAMES[mode]} {M}x{N}x{K} {fam} epi={int(epi)} {lay} [{key}]"
        dA, dB = _operand(dev, h["A"], lay.a_off, lay.a_pad), _operand(dev, h["B"], lay.b_off, lay.b_pad)
        dbias = torch.from_numpy(h["bias"].copy()).to(dev) if epi else None
        dR = _operand(dev, h["resid"], 1 if lay.r_off else 4, (((N + 3) | 1) - N) if lay.r_off else None) if epi else None
        if epi:
            assert (dR.data_ptr() % 16 == 0) == (lay.r_off == 0) and (dR.stride(0) % 2 == 1) == bool(lay.r_off)

        def launch():
            out = _Out(dev, M, N, lay.c_off)
            cs = None
            if colsum:
                cs = _Out(dev, 1, M, 0)
                engine.gemm_tn_colsum(dA, dB, out.view, cs.view[0])
            elif K == 0:        # the wrapper hands an empty operand over as a null pointer, which the entry point refuses: ctypes
                p = engine._ptr
                engine._call("gnm_gemm_f32", mode, M, N, K, C.c_void_p(dA.ptr), dA.stride(0), C.c_void_p(dB.ptr), dB.stride(0), p(out.view),
                             out.ld, p(dbias), p(dR), dR.stride(0) if epi else 0, int(epi), C.c_void_p(0), 0, engine._stream())
            else:
                engine.gemm(mode, dA, dB, out.view, bias=dbias, resid=dR, relu=epi)
            torch.cuda.synchronize()
            return out.take(what), (cs.take(what + " colsum")[0] if colsum else None)

        def verify(got, gcs, tag):
            _verify(f"{what} {tag}", fam, arith, K, got, h["ref"], h["absprod"], h["epi"], key)
            if colsum:      # a column sum is the product with a vector of ones: the same c(K), on sum |a|
                _verify(f"{what} {tag} colsum", fam, "f32", K, gcs, h["cs"], h["csabs"], None, key + " (sums)")

        g1, c1 = launch()
        g2, c2 = launch()
        assert np.array_equal(_bits(g1), _bits(g2)), f"{what}: two runs differ"
        assert not colsum or np.array_equal(_bits(c1), _bits(c2)), f"{what}: two runs differ (colsum)"
        verify(g1, c1, "")
        try:
            for cap in (1, 2):
                assert lib.gnm_set_occupancy_cap(cap) == 0
                gc, cc = launch()
                verify(gc, cc, f"cap={cap}")
        finally:
            lib.gnm_set_occupancy_cap(0)
    print(f"bound used: {key:28s} {_USED.get(key, 0.0):.3f}")


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    txt = "\n".join(f"bound used: {k:28s} {v:.3f}" for k, v in sorted(_USED.items()))
    print("\n" + txt)
    _log("gemm_bound_used.txt", txt + "\n")


# ---- general tile kernel ---------------------------------------------------------------------------------------------------------
# M, N in {1, 127, 128, 129} crossed sparsely with K in {0, 1, 31, 32, 33, 65}: every pair of edge conditions (one row / column, one
# short of, exactly, one past a 128 tile; no k-tile, one element, one short of, exactly, one past a k-tile, two tiles + 1) meets once.
# All of them general: no K >= 4096, no M >= 2048.  K = 0 gives the epilogue of a zero product.
GENERAL = [(1, 1, 0), (129, 127, 0), (1, 128, 1), (127, 1, 1), (129, 129, 1), (128, 127, 31), (1, 129, 31), (128, 128, 32), (127, 129, 32),
           (129, 1, 33), (127, 127, 33), (129, 128, 65), (1, 127, 65), (128, 129, 65)]


@pytest.mark.parametrize("epi", [False, True])
@pytest.mark.parametrize("mode", [NT, NN, TN])
@pytest.mark.parametrize("M,N,K", GENERAL)
def test_general_tile_kernel(matmul_mode, M, N, K, mode, epi):
    run_case(matmul_mode, mode, M, N, K, epi=epi, expect="general")


# ---- TN split-K ------------------------------------------------------------------------------------------------------------------

def _first_k_with(splits, M, N, cus):
    K = 1
    while plan_split(TN, M, N, K, cus) < splits:
        K += 1
    return K


@pytest.mark.parametrize("which", ["2 splits", "2 splits - 1", "2 splits + 1", "ragged", "3 splits"])
def test_tn_split_k(matmul_mode, which):
    """One 128 x 128 tile.  The K values come from plan_split's constants and the CU count; the split count the entry point plans is
    read back from its workspace size (splits * M * N floats; none for one split)."""
    lib = _lib_()
    cus, M, N = lib.gnm_num_cus(), 128, 128
    k2 = _first_k_with(2, M, N, cus)
    assert k2 == BK * MIN_KTILES + 1, "one tile on any GPU with >= 1 CU: 2 splits as soon as there are 17 k-tiles"
    if which == "ragged":         # 19 k-tiles: the splits take 10 + 9 tiles, and the last tile holds 7 rows
        K, splits = 18 * BK + 7, 2
    elif which == "3 splits":
        K, splits = _first_k_with(3, M, N, cus), 3
    else:
        K = k2 + {"2 splits": 0, "2 splits - 1": -1, "2 splits + 1": 1}[which]
        splits = 1 if K < k2 else 2
    assert plan_split(TN, M, N, K, cus) == splits
    ws = lib.gnm_gemm_f32_workspace_bytes(TN, M, N, K)
    assert ws == (splits * M * N * 4 if splits > 1 else 0), f"K = {K}: workspace {ws} bytes is not that of {splits} splits"
    run_case(matmul_mode, TN, M, N, K, expect="splitk" if splits > 1 else "general")
    if which == "3 splits":
        run_case(matmul_mode, TN, 129, 127, K, epi=True, expect="splitk")        # 4 tiles, edge tiles, the reduce kernel's epilogue


# ---- skinny TN ---------------------------------------------------------------------------------------------------------------------
SKINNY_N = [1, 7, 16, 17, 18, 32]                      # 16 | 17: tn_skinny128_k<1> | <2>
SKINNY_K = [4096, 4097, 4096 + 15, 4096 + 16]          # 16 rows per tile: a full last tile, 1, 15 rows in it, one more full tile


@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("K", SKINNY_K)
@pytest.mark.parametrize("N", SKINNY_N)
def test_skinny_tn(matmul_mode, N, K, colsum):
    assert _lib_().gnm_gemm_f32_workspace_bytes(TN, 128, N, K) >= SKN_BYTES
    run_case(matmul_mode, TN, 128, N, K, colsum=colsum, expect="skinny")


@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("M,N,K", [(128, 32, 4095), (128, 33, 4096), (127, 32, 4096), (129, 32, 4096)])
def test_just_outside_skinny(matmul_mode, M, N, K, colsum):
    """One step outside each condition of tn_skinny_shape_ok: the general kernel in k-splits, held to its bound."""
    run_case(matmul_mode, TN, M, N, K, colsum=colsum, expect="splitk")
    assert _lib_().gnm_gemm_f32_workspace_bytes(TN, M, N, K) < SKN_BYTES, "the skinny route's workspace is planned for this shape"


def test_skinny_with_an_epilogue_falls_back(matmul_mode):
    run_case(matmul_mode, TN, 128, 18, 4097, epi=True, expect="splitk")


# ---- split-mode route ---------------------------------------------------------------------------------------------------------------
# the smallest shape gemm_b3_shape_ok accepts per mode, then one step outside each condition (always the general kernel)
B3 = [
    (NT, 2048, 128, 128, "b3"), (NN, 2048, 128, 128, "b3"), (TN, 128, 128, 4096, "b3"),
    (NT, 2047, 128, 128, "general"), (NN, 2047, 128, 128, "general"),               # M < 2048
    (NT, 2048, 127, 128, "general"), (NN, 2048, 129, 128, "general"),               # N % 128
    (NT, 2048, 128, 127, "general"), (NN, 2048, 128, 129, "general"),               # K % 128
    (NT, 2048, 256, 256, "b3"), (NN, 2049, 128, 256, "b3"),                         # two classes, two column groups; a ragged last row
    (TN, 128, 128, 4095, "splitk"),                                                 # K < 4096
    (TN, 127, 128, 4096, "splitk"), (TN, 128, 129, 4096, "splitk"),                 # M % 128, N % 128
    (TN, 256, 128, 4097, "b3"),                                                     # two A groups, a ragged last 32-row tile
]


@pytest.mark.parametrize("mode,M,N,K,route", B3)
def test_split_mode_route(matmul_mode, mode, M, N, K, route):
    if matmul_mode == "f32":
        route = "splitk" if mode == TN else "general"          # no split-mode route in the fp32-MFMA mode
    run_case(matmul_mode, mode, M, N, K, expect=route)
    if mode != TN:
        run_case(matmul_mode, mode, M, N, K, epi=True, expect=route)


def test_split_mode_class_limit_tn(matmul_mode):
    """(M/128)(N/128) = 65 > 64: 5 x 13 blocks, one step outside the last condition of the TN form."""
    run_case(matmul_mode, TN, 640, 1664, 4096, expect="splitk", families=["ints", "normal"])


def test_split_mode_tn_with_an_epilogue_falls_back(matmul_mode):
    run_case(matmul_mode, TN, 128, 128, 4096, epi=True, expect="splitk")


@pytest.mark.parametrize("M,N,K", [(128, 128, 4096), (256, 128, 4097), (128, 128, 4095), (128, 129, 4096)])
def test_tn_colsum_split_route_and_fallback(matmul_mode, M, N, K):
    route = "b3" if matmul_mode != "f32" and K >= 4096 and N % 128 == 0 else "splitk"
    run_case(matmul_mode, TN, M, N, K, colsum=True, expect=route)


# ---- alignment and strides -------------------------------------------------------------------------------------------------------------
# One shape per route.  Read before the first run (gnm_gemm.hip, gnm_fused.hip, gnm_tr.hip, gnm_misc.hip): gemm_f32_k loads an operand
# as float4 only under a_aligned / b_aligned and stores C, reads resid and bias by element, as splitk_reduce_k and tn_skinny_finish_k
# do; the skinny kernel loads A as float4 (tn_skinny_try checks A and lda) and B by element; gemm_rows_b3_k loads A, resid and bias and
# stores C as float4 (gemm_b3_try checks all four), its B goes through pack_w3_gen_k / pack_w2_gen_k by element; tn_tr_k loads A and
# B as float4 (checked); slab_reduce_ld_k stores C as float4, which gemm_b3_try did NOT check for TN: fixed there (al(C, ldc)), so
# that a TN call with a C that is not 16-byte aligned or has ldc % 4 != 0 takes the general kernel.
ALIGN_SHAPES = [(NT, 129, 127, 65, True), (NN, 129, 128, 64, True), (TN, 129, 128, 64, True), (TN, 128, 128, 513, False),
                (TN, 128, 18, 4097, False), (NT, 2048, 128, 128, True), (NN, 2048, 128, 128, True), (TN, 128, 128, 4096, False)]


ALIGN_CASES = [s + (name,) for s in ALIGN_SHAPES for name in LAYOUTS if s[4] or name != "r+1,odd ldr"]      # resid: where there is one


@pytest.mark.parametrize("mode,M,N,K,epi,layout", ALIGN_CASES)
def test_alignment_and_strides(matmul_mode, mode, M, N, K, epi, layout):
    lay = LAYOUTS[layout]
    cus = _lib_().gnm_num_cus()
    aligned, here = route_of(matmul_mode, mode, M, N, K, epi, ALIGNED, cus)[0], route_of(matmul_mode, mode, M, N, K, epi, lay, cus)[0]
    fallback = "splitk" if plan_split(mode, M, N, K, cus) > 1 else "general"
    assert here in (aligned, fallback)
    if aligned == "skinny":
        assert (here == "skinny") == _al(lay.a_off, _ld(128, lay.a_pad))
    if aligned == "b3" and mode == TN:
        assert (here == "b3") == (layout in ("lda=K+4", "ldb+4")), "A, B and C must all allow float4 accesses"
    if aligned == "b3" and mode != TN:
        assert (here == "b3") == (layout in ("lda=K+4", "b+1", "ldb+1", "ldb+4")), "A, C, resid must allow float4 accesses; B any"
    run_case(matmul_mode, mode, M, N, K, epi=epi, lay=lay)
    if mode == TN and not epi:
        run_case(matmul_mode, mode, M, N, K, lay=lay, colsum=True, families=["ints", "normal"])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_output_untouched(matmul_mode):
    from gnnome_assembly_amd import engine
    dev, lib = _dev(), _lib_()
    p, st, null = engine._ptr, engine._stream(), C.c_void_p(0)
    M, N, K = 128, 128, BK * MIN_KTILES + 1                        # TN: 2 k-splits
    A = torch.ones((K, M), device=dev)
    B = torch.ones((K, N), device=dev)
    out, cs = _Out(dev, M, N, 0), _Out(dev, 1, M, 0)
    need = lib.gnm_gemm_f32_workspace_bytes(TN, M, N, K)
    assert need == 2 * M * N * 4
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)

    def gemm(mode=TN, m=M, n=N, k=K, a=p(A), b=p(B), c=p(out.view), wsb=need):
        return lib.gnm_gemm_f32(mode, m, n, k, a, M, b, N, c, out.ld, null, null, 0, 0, p(ws), wsb, st)

    def refused(rc, word):
        msg = lib.gnm_last_error().decode(errors="replace")
        torch.cuda.synchronize()
        assert rc == -1 and word in msg, (rc, msg)
        assert np.isnan(out.flat.cpu().numpy()).all() and np.isnan(cs.flat.cpu().numpy()).all(), f"{msg}: the output was written"

    refused(gemm(mode=-1), "mode")
    refused(gemm(mode=3), "mode")
    refused(gemm(a=null), "null")
    refused(gemm(b=null), "null")
    refused(gemm(c=null), "null")
    refused(gemm(m=-1), "neg")
    refused(gemm(k=-1), "neg")
    refused(gemm(wsb=need - 1), "workspace")
    need2 = lib.gnm_gemm_tn_colsum_workspace_bytes(M, N, K)
    assert need2 >= need
    tn = lambda wsb, a=p(A), m=M: lib.gnm_gemm_tn_colsum(m, N, K, a, M, p(B), N, p(out.view), out.ld, p(cs.view), p(ws), wsb, st)  # noqa: E731
    refused(tn(need2 - 1), "workspace")
    refused(tn(need2, a=null), "null")
    refused(tn(need2, m=0), "null/neg")
    need_sk = lib.gnm_gemm_tn_colsum_workspace_bytes(128, 18, 4096)          # a skinny shape with the workspace one byte short
    assert need_sk >= SKN_BYTES
    big = torch.empty(need_sk, dtype=torch.uint8, device=dev)
    A2, B2 = torch.ones((4096, 128), device=dev), torch.ones((4096, 18), device=dev)
    refused(lib.gnm_gemm_tn_colsum(128, 18, 4096, p(A2), 128, p(B2), 18, p(out.view), out.ld, p(cs.view), p(big), need_sk - 1, st), "workspace")
    # nothing to do: 0, and nothing written
    assert gemm(m=0) == 0 and gemm(n=0) == 0
    torch.cuda.synchronize()
    assert np.isnan(out.flat.cpu().numpy()).all()
    # and the same call with everything in order runs
    assert gemm() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.take("all ones"), np.full((M, N), float(K), np.float32))
