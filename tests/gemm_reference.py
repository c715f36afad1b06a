"""numpy fp64 reference of gnm_gemm_f32 / gnm_gemm_tn_colsum, the input families of their tests and the per-element bound.

    ref(mode, A, B, bias, resid, relu)   C = op(A) op(B) (+ bias + resid, relu) in fp64 from the fp32 operands
    absprod(mode, A, B)                  sum_k |a| |b| per output element: what every rounding of the product sum scales with
    colsum_ref(A)                        (sum_k A[k, m], sum_k |A[k, m]|) of gnm_gemm_tn_colsum's second output
    bound(arith, K, absprod, ref, epi)   |err| <= c(K) u_arith absprod + u |ref| + (epilogue additions) u epi   per element

u = 2^-24 (half an fp32 ulp, relative).  u_arith is the operand precision the project documents for the arithmetic a route runs
(INTEGRATION.md "Numerics"): fp32 MFMA and bf16x3 carry 24-bit operands (u), f16x2 two fp16 terms = 22 bits
(4 u).  c(K) is not chosen here: tools/measure_gemm_bounds.py measures |torch fp32 CPU matmul - ref| / (u absprod) per K class over
every GEMM mode and family and stores c = 4 x the worst ratio in profiles/gemm_bounds.json (the factor 4 of
tools/measure_batchnorm_bounds.py: another summation order); c(K) <= K always, the worst case of any fp32 summation order.
The class's worst is set by the heavy-tailed `rows` family (one early large term makes every later partial sum round at its size);
the tests hold each family to its own, smaller constant (c_family: `rows` its own, the others the `normal` one -- torch's order keeps
the partial sums of `cancel` near zero, which a tiled kernel's order need not, while for any blocked order they stay a few OFFSET^2,
below a well-conditioned sum's partial sums relative to absprod).
The term u |ref| is the rounding of the result to fp32 (split-K and the skinny finisher round once more at the end); an epilogue
addition rounds once to at most u (|product| + |bias| + |resid|), whichever order the kernel adds in.

K classes: 0, then the next power of two >= K.  Families, each a function of (shape, seed) returning fp32 (`axis`: the contraction
axis of the operand, which only `cancel` looks at):
    normal   N(0, 1)
    rows     N(0, 1) with row magnitudes exp(2 N(0, 1))
    cancel   (OFFSET + N(0, 1)) with a sign that alternates along the contraction: + - + - in the A operand, + + - - in the B
             operand, so the products run + - - + and |ref| << absprod (up to one unpaired OFFSET^2 when K % 4 is 1 or 3: the
             family is used where K % 4 == 0 or K >= 2048, uses_cancel)
    ints     integers in [-8, 8]: products and partial sums are exact in fp32 in any order while 8 * 8 * K < 2^24, and the values
             are exact in the first term of both split modes (bf16: 8 bits; fp16 after a power-of-two scale: 11 bits)"""
import json
import os

import numpy as np

NT, NN, TN = 0, 1, 2
MODE_NAMES = ("NT", "NN", "TN")
U = 2.0 ** -24
U_ARITH = {"f32": U, "bf16x3": U, "f16x2": 2.0 ** -22}
OFFSET = 1024.0
FAMILIES = ("normal", "rows", "cancel", "ints")
K_CLASSES = (0,) + tuple(1 << i for i in range(14))          # up to 8192: the largest operand of the tests is 128 x ~4.2 k
BOUNDS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gemm_bounds.json")


def f64(x):
    return np.asarray(x, dtype=np.float64)


def k_class(K):
    c = 0 if K == 0 else 1 << (int(K) - 1).bit_length()
    assert c in K_CLASSES, f"K = {K}: no class"
    return c


def uses_cancel(K):
    return K >= 128 and (K % 4 == 0 or K >= 2048)


def shapes(mode, M, N, K):
    """Shapes of A and B (include/gnm.h): NT A[M,K] B[N,K];  NN A[M,K] B[K,N];  TN A[K,M] B[K,N]."""
    return {NT: ((M, K), (N, K)), NN: ((M, K), (K, N)), TN: ((K, M), (K, N))}[mode]


def contraction_axes(mode):
    return {NT: (1, 1), NN: (1, 0), TN: (0, 0)}[mode]


def _mk(mode, A, B):
    """(A as [M,K], B as [K,N]) in fp64."""
    A, B = f64(A), f64(B)
    return (A.T if mode == TN else A), (B.T if mode == NT else B)


def product(mode, A, B):
    a, b = _mk(mode, A, B)
    return a @ b


def absprod(mode, A, B):
    a, b = _mk(mode, A, B)
    return np.abs(a) @ np.abs(b)


def ref(mode, A, B, bias=None, resid=None, relu=False):
    c = product(mode, A, B)
    if bias is not None:
        c = c + f64(bias)[None, :]
    if resid is not None:
        c = c + f64(resid)
    return np.maximum(c, 0.0) if relu else c


def epilogue(mode, A, B, bias=None, resid=None):
    """(number of epilogue additions, |product| + |bias| + |resid|): what bound() charges u per addition for."""
    n = (bias is not None) + (resid is not None)
    mag = np.abs(product(mode, A, B))
    if bias is not None:
        mag = mag + np.abs(f64(bias))[None, :]
    if resid is not None:
        mag = mag + np.abs(f64(resid))
    return n, mag


def colsum_ref(A):
    A = f64(A)
    return A.sum(0), np.abs(A).sum(0)


# ---- families --------------------------------------------------------------------------------------------------------------

def _rng(shape, seed):
    return np.random.default_rng([int(seed), int(shape[0]), int(shape[1])])


def normal(shape, seed, axis=1, second=False):
    return _rng(shape, seed).standard_normal(shape).astype(np.float32)


def rows(shape, seed, axis=1, second=False):
    r = _rng(shape, seed)
    return (r.standard_normal(shape) * np.exp(2.0 * r.standard_normal((shape[0], 1)))).astype(np.float32)


def cancel(shape, seed, axis=1, second=False):
    k = np.arange(shape[axis])
    sign = np.where((k // 2 if second else k) % 2 == 0, 1.0, -1.0)
    sign = sign[None, :] if axis == 1 else sign[:, None]
    return ((OFFSET + _rng(shape, seed).standard_normal(shape)) * sign).astype(np.float32)


def ints(shape, seed, axis=1, second=False):
    assert 8 * 8 * shape[axis] < 2 ** 24, "ints: sums of products are exact in fp32 only while 8 * 8 * K < 2^24"
    return _rng(shape, seed).integers(-8, 9, shape).astype(np.float32)


FAMILY_FN = {"normal": normal, "rows": rows, "cancel": cancel, "ints": ints}


def operands(family, mode, M, N, K, seed, epi=False):
    """A, B and, with epi, bias [N] and resid [M,N] (else None) of one case; the ints family has integer bias and resid."""
    sa, sb = shapes(mode, M, N, K)
    xa, xb = contraction_axes(mode)
    fn = FAMILY_FN[family]
    A, B = fn(sa, seed, xa, False), fn(sb, seed + 1, xb, True)
    if not epi:
        return A, B, None, None
    side = ints if family == "ints" else normal
    return A, B, side((1, N), seed + 2)[0].copy(), side((M, N), seed + 3)


# ---- bound -----------------------------------------------------------------------------------------------------------------

_C = None


def c_of(K, family=None):
    """c(K) of the K class from profiles/gemm_bounds.json (measured on torch's fp32 CPU matmul, never on the code under test): of the
    family where one is given (<= the class's), else the class's worst over all families."""
    global _C
    if _C is None:
        d = json.load(open(BOUNDS_FILE))
        _C = {int(k): dict(d["c_family"][k], all=float(v)) for k, v in d["c"].items()}
    c = _C[k_class(K)][family or "all"]
    assert c <= _C[k_class(K)]["all"] <= k_class(K), f"c({K}) = {c} above the worst case K of any summation order: the measurement is wrong"
    return min(c, float(K))       # the class's constant was taken at its largest K: the hard cap is this K's own


def bound(arith, K, absprod_, ref_, epilogue_=None, family=None):
    """Per element; arith in U_ARITH; epilogue_ = epilogue(...) or None; family: c_of."""
    c = c_of(K, family)
    assert c <= max(K, 0)
    b = c * U_ARITH[arith] * f64(absprod_) + U * np.abs(f64(ref_))
    if epilogue_ is not None and epilogue_[0]:
        b = b + epilogue_[0] * U * epilogue_[1]
    return b
