"""fp64 statements of the two input-feature entry points (gnm_pagerank_pe, gnm_edge_feats_zscore; csrc/gnm_features.hip), their
per-element bars and the case matrix their tests run.  numpy and math only; nothing here touches a device.

    pagerank_pe64(src, dst, n, pe_dim, alpha)      float64 [n, 2 + pe_dim] = in_deg | out_deg | x_1 .. x_pe_dim, never rounded
    pagerank_bound(want64, max_in_deg, pe_dim)     the bar of every element of it
    zscore64(a, b)                                 float64 [E, 2] z-score (unbiased std), two passes with math.fsum
    zscore_bound(want64, x, nb)                    the bar of one column of it
    zscore_margin(x, nb)                           fp32 half-ulp / fp64 term at |z| = 1: a case is usable from 100 up
    emulate_zscore_kernel(a, b, nb, acc_dtype)     the kernel's blocked one-pass arithmetic in numpy (fp32 [E, 2])
    zs_blocks(E, cus) / pr_grid(n, cus)            the launch arithmetic of the two entry points, restated
    pagerank_cases(cus) / zscore_cases(cus)        the matrices of tests/test_gpu_features.py and test_features_reference_cpu.py

Launch arithmetic (read in gnm_features.hip, gnm_common.h): ew_grid(n, 256) = min(cdiv(n, 256), CUS * 8), at least 1, workgroups of 256
threads in grid-stride loops; the z-score's statistics kernel runs nb = min(ew_grid(E, 256), 2048) workgroups and writes 4 doubles each."""
import functools
import math

import numpy as np

U32 = 2.0 ** -24          # fp32 unit round-off: half an ulp of 1.0
U64 = 2.0 ** -53          # fp64 unit round-off
BLOCK = 256
MAX_PARTIAL_BLOCKS = 2048
MI355X_CUS = 256


def cdiv(a, b):
    return -(-a // b)


def pr_grid(n, cus=MI355X_CUS):
    return max(1, min(cdiv(n, BLOCK), cus * 8))


def zs_blocks(E, cus=MI355X_CUS):
    return min(pr_grid(E, cus), MAX_PARTIAL_BLOCKS)


def half_ulp32(want64):
    """Half the spacing of the fp32 numbers around each fp64 value: what rounding it to nearest can move it by.  The binade is
    the value's own (not that of its rounded image, which at a power of two is twice as coarse); below the smallest normal fp32
    number the spacing stays 2^-149, so 0 keeps a bar of 2^-150."""
    a = np.abs(np.asarray(want64, np.float64))
    _, e = np.frexp(a)                                               # |x| = m 2^e, m in [0.5, 1): ulp = 2^(e - 24)
    return np.ldexp(1.0, np.where(a > 0, np.maximum(e - 25, -150), -150))


# ---- PageRank ------------------------------------------------------------------------------------------------------------------

def pagerank_pe64(src, dst, n, pe_dim=16, alpha=0.95):
    """utils.add_positional_encoding in float64 throughout: dinv = 1 / (outdeg + 1e-9), 0 where outdeg < 1e-9; x_0 = 1/n;
    x <- alpha * sum over in-edges (u -> v) of dinv[u] x[u] + (1 - alpha)/n.  The in-edge terms of a node are added in edge-id
    order (np.bincount), the arithmetic of synth.pagerank_pe without its rounding to fp32."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    out_deg = np.bincount(src, minlength=n).astype(np.float64)
    in_deg = np.bincount(dst, minlength=n).astype(np.float64)
    dinv = 1.0 / (out_deg + 1e-9)
    dinv[out_deg < 1e-9] = 0.0
    w = dinv[src]
    x = np.full(n, 1.0 / n)
    pe = np.empty((n, 2 + pe_dim), np.float64)
    pe[:, 0], pe[:, 1] = in_deg, out_deg
    for t in range(pe_dim):
        x = alpha * np.bincount(dst, weights=w * x[src], minlength=n) + (1.0 - alpha) / n
        pe[:, 2 + t] = x
    return pe


def pagerank_bound(want64, max_in_deg, pe_dim):
    """|kernel - want64| may reach, per element: half an fp32 ulp of want64 + pe_dim (max_in_deg + 4) 2^-53 |want64|.

    Derivation.  Every quantity of the iteration is non-negative (x >= 0, dinv >= 0, alpha in [0, 1]), so nothing cancels and a
    relative error of the terms is at most the same relative error of their sum.  Kernel and oracle perform the same fp64
    operations on a node -- 1/(d + 1e-9), its product with x[u], the sum over the in-edges, alpha * sum + teleport -- and differ
    in two places only: the ORDER in which the d_in terms of a node are added (the kernel walks the destination-sorted index over
    whatever node numbering the index uses, the oracle adds in edge-id order), and the last step, which a compiler may contract
    into one fused multiply-add (one rounding where the oracle has two).  A sum of d non-negative terms added one by one in any
    order is within (d - 1) u of the exact sum, relatively (u = 2^-53, first order); the bar charges that once per step, plus 4 u
    for the contraction (<= 1 u), the two roundings of the last step and the product feeding the next step.  With delta_t the
    relative distance of the two iterates after t steps, delta_0 = 0 (1/n is the same correctly rounded quotient on both sides)
    and delta_{t+1} <= delta_t + (max_in_deg + 4) u, because alpha * sum <= x_{t+1}; hence delta_t <= pe_dim (max_in_deg + 4) u
    for every column.  The two orders can each be (d - 1) u from the exact sum in OPPOSITE directions; that worst case needs every
    partial sum of one order to round up and of the other to round down, and even the doubled term stays below 1e-3 of the fp32
    half-ulp at the largest case of the matrix (16 steps, in-degree 6000: 2e-11 against 3e-8), so charging it once keeps the bar
    tight where it matters; test_features_reference_cpu.py runs a shuffled summation order against it for every case.  Last,
    the kernel rounds the fp64 iterate to fp32 once: half an ulp of the value, taken in want64's own binade.

    The degree columns hold small integers; the tests compare them exactly, and this bar (half an ulp of an integer) would admit
    nothing else either.  Nothing here is taken from the kernel's output."""
    want64 = np.asarray(want64, np.float64)
    return half_ulp32(want64) + pe_dim * (max_in_deg + 4) * U64 * np.abs(want64)


def max_in_degree(dst, n):
    return int(np.bincount(np.asarray(dst, np.int64), minlength=n).max()) if len(dst) else 0


# ---- z-score -------------------------------------------------------------------------------------------------------------------

def _fsum(x):
    return math.fsum(x.tolist())


def _zscore_col64(x):
    x = np.asarray(x, np.float64)
    n = x.size
    d = x - _fsum(x) / n               # the sum is exact (fsum), the quotient rounded once; the difference of an fp32-valued
    d = d - _fsum(d) / n               # number and a nearby fp64 one is exact or rounded once: the second pass removes what the
    var = _fsum(d * d) / (n - 1)       # rounded mean left, so no error here grows with mean / std
    with np.errstate(divide="ignore", invalid="ignore"):
        return d / math.sqrt(var)


def zscore64(a, b):
    """utils.preprocess_graph's z-score of the two fp32-valued columns, float64 [E, 2]: (x - mean) / std with torch's default
    unbiased std.  Two passes, every sum by math.fsum (correctly rounded), the mean refined once: no cancellation of its own, a
    few 2^-53 |z| from the exact value.  A constant column divides by a zero std, like the reference (nan)."""
    return np.stack([_zscore_col64(a), _zscore_col64(b)], 1)


def _zs_depth(E, nb):
    """Additions a term passes through on its way into a column sum: the per-thread run of ceil(E / (nb 256)) terms, the eight
    levels of the 256-wide tree, the nb-long serial tail of zs_apply_k."""
    return cdiv(E, nb * BLOCK) + 8 + nb


def _kappa(x):
    """1 + mean^2 / var of a column, as sum x^2 / sum (x - mean)^2 (exactly that for the biased variance).  Two passes with
    numpy's pairwise sums: a condition number needs three digits, not sixteen."""
    x = np.asarray(x, np.float64)
    d = x - x.mean()
    q = float((d * d).sum())
    return float((x * x).sum()) / q if q > 0 else math.inf


def _zs_fp64_term(absz, E, nb, kappa):
    h = _zs_depth(E, nb)
    return U64 * ((1.5 * h + 12.0) * kappa * absz + (h + 1.0) * math.sqrt(kappa))


def zscore_bound(want64, x, nb):
    """The bar of one column: half an fp32 ulp of want64 + 2^-53 ((1.5 h + 12) kappa |want64| + (h + 1) sqrt(kappa)), with
    h = ceil(E / (nb 256)) + 8 + nb and kappa = sum x^2 / sum (x - mean)^2 = 1 + mean^2 / var.

    Derivation (u = 2^-53, first order).  The kernel forms S1 = sum x and S2 = sum x^2 in fp64 in one pass; x is an fp32 value, so
    x^2 is exact in fp64.  Every term reaches its sum through at most h additions (_zs_depth), so the computed sums are within
    h u sum|x| and h u S2 of the exact ones.  mean' = S1'/n adds one rounding: |mean' - mean| <= (h + 1) u mean|x|.  The variance
    comes from Q = S2 - n mean^2 = (n - 1) var, where the cancellation is: the errors of S2 (h u S2), of n mean'^2
    (2 n |mean| |mean' - mean| <= 2 (h + 1) u S2, since |mean| mean|x| <= S2 / n) and of its own roundings (2 u n mean^2 + u Q)
    add up to (3 h + 5) u S2 = (3 h + 5) u kappa Q.  The square root halves that relative error; the division by n - 1, the root
    and the reciprocal round once each: rstd' = rstd (1 + eps), |eps| <= (1.5 h + 5.5) u kappa.  The output (x - mean') rstd' has
    two more roundings and carries the shift of the mean, (h + 1) u mean|x| rstd <= (h + 1) u sqrt(kappa) (mean|x| <= rms, and
    rms / std = sqrt(kappa) up to n / (n - 1), which the + 12 absorbs together with the oracle's own few u |z|):
        |z' - z| <= u ((1.5 h + 12) kappa |z| + (h + 1) sqrt(kappa)).
    Then one rounding to fp32.  x: the column as the kernel receives it; nb: its block count (zs_blocks)."""
    want64 = np.asarray(want64, np.float64)
    return half_ulp32(want64) + _zs_fp64_term(np.abs(want64), len(x), nb, _kappa(x))


def zscore_margin(x, nb):
    """How far the fp64 term stays under the fp32 one: half an fp32 ulp of 1.0 over the fp64 term at |z| = 1.  A z-scored column
    has unit variance, so |z| = 1 is the scale of its elements; elements nearer the mean have a finer fp32 spacing while the part
    of the fp64 term that comes from the shifted mean does not shrink with them, so the ratio is stated per column, not per
    element.  Below 100 the column is too ill-conditioned for its comparison to say anything about the fp32 result."""
    return U32 / _zs_fp64_term(1.0, len(x), nb, _kappa(x))


def emulate_zscore_kernel(a, b, nb, acc_dtype=np.float64, ddof=1):
    """zs_stats_k + zs_apply_k in numpy: thread t of block k adds the terms k 256 + t + j nb 256 (j = 0, 1, ..) one by one in
    `acc_dtype`, the 256 threads of a block combine in the halving tree, the nb block sums are added serially; mean, one-pass
    variance (S2 - n mean^2) / (n - ddof) and the output in fp64 from those sums, rounded to fp32 like the kernel's store.
    acc_dtype = float32 is the mutant that accumulates in fp32; ddof = 0 the one with the biased std."""
    cols = []
    for x in (a, b):
        x = np.asarray(x, np.float32)
        E = x.size
        L = cdiv(E, nb * BLOCK)
        xp = np.zeros(L * nb * BLOCK, acc_dtype)       # the padding adds exact zeros: the same sums as the kernel's guarded loop
        xp[:E] = x
        xp = xp.reshape(L, nb, BLOCK)
        s1 = np.zeros((nb, BLOCK), acc_dtype)
        s2 = np.zeros((nb, BLOCK), acc_dtype)
        for j in range(L):
            s1 = s1 + xp[j]
            s2 = s2 + xp[j] * xp[j]
        st = BLOCK // 2
        while st > 0:
            s1 = s1[:, :st] + s1[:, st:2 * st]
            s2 = s2[:, :st] + s2[:, st:2 * st]
            st //= 2
        t1, t2 = acc_dtype(0), acc_dtype(0)
        for k in range(nb):
            t1 = t1 + s1[k, 0]
            t2 = t2 + s2[k, 0]
        n = float(E)
        t1, t2 = float(t1), float(t2)
        mean = t1 / n
        var = (t2 - n * mean * mean) / (n - ddof)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.float64(1.0) / np.sqrt(np.float64(var))
            cols.append(((x.astype(np.float64) - mean) * r).astype(np.float32))
    return np.stack(cols, 1)


# ---- the case matrices ---------------------------------------------------------------------------------------------------------

def _path(n):
    p = np.arange(n - 1, dtype=np.int32)
    return p, p + 1, n


def _random_graph(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, 4 * n).astype(np.int32), rng.integers(0, n, 4 * n).astype(np.int32), n


def _thirds():
    """300 nodes: 0..99 have no out-edge, 100..199 no in-edge, 200..279 both kinds, 280..299 neither (isolated)."""
    rng = np.random.default_rng(21)
    src = rng.integers(100, 280, 900)
    dst = rng.integers(0, 180, 900)
    dst = np.where(dst >= 100, dst + 100, dst)           # 0..99 and 200..279
    return src.astype(np.int32), dst.astype(np.int32), 300


def _loops_and_duplicates():
    rng = np.random.default_rng(22)
    n = 70
    src, dst = rng.integers(0, n, 200), rng.integers(0, n, 200)
    loops = np.arange(0, n, 3)
    src = np.concatenate([src, loops, loops, src[:40], src[:40]])      # every third node loops twice; 40 edges three times
    dst = np.concatenate([dst, loops, loops, dst[:40], dst[:40]])
    return src.astype(np.int32), dst.astype(np.int32), n


def _hub():
    """One destination with 6000 in-edges (the hub graph of test_gpu_parity._adversarial_graphs)."""
    rng = np.random.default_rng(12)
    dst = np.concatenate([np.full(6000, 7), rng.integers(0, 2000, 3000)]).astype(np.int32)
    return rng.integers(0, 2000, 9000).astype(np.int32), dst, 2000


def small_graph():
    """64 nodes, 256 edges: isolated, source-only and sink-only nodes, self loops, duplicates, two hubs, random edge ids
    (synth.tiny_edge_case_graph, restated here so that this module needs numpy alone)."""
    rng = np.random.default_rng(31)
    n, e = 64, 256
    src = rng.integers(0, n - 8, size=e)
    dst = rng.integers(4, n - 4, size=e)
    src[:6] = dst[:6]
    src[6:12], dst[6:12] = src[12:18], dst[12:18]
    dst[20:60] = 17
    src[60:90] = 23
    return src.astype(np.int32), dst.astype(np.int32), n


def shuffled_band_graph():
    """20000 nodes of a banded overlap graph (every node to its next four) under a random renumbering: one edge in five joins
    ids within the 2048-node window, so node_order='auto' gives the index an internal numbering."""
    n = 20000
    i = np.repeat(np.arange(n - 4), 4)
    j = i + np.tile(np.arange(1, 5), n - 4)
    p = np.random.default_rng(23).permutation(n)
    return p[i].astype(np.int32), p[j].astype(np.int32), n


PE_DIMS = (0, 1, 5, 16, 20)
ALPHAS = (0.95, 0.5, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def pagerank_cases(cus=MI355X_CUS):
    """name -> (src, dst, n, pe_dim, alpha).  `cus`: the device's compute units (the grid cap of fgrid is cus * 8 workgroups)."""
    e = np.zeros(0, np.int32)
    c = {
        "N=1, one self loop": (np.zeros(1, np.int32), np.zeros(1, np.int32), 1, 16, 0.95),
        "N=2": (np.array([0, 1, 0], np.int32), np.array([1, 0, 0], np.int32), 2, 16, 0.95),
        "tiny (5 nodes)": (np.array([0, 1, 2, 2], np.int32), np.array([1, 2, 0, 2], np.int32), 5, 16, 0.95),
        "no out-edge | no in-edge | isolated": _thirds() + (16, 0.95),
        "self loops + duplicates": _loops_and_duplicates() + (16, 0.95),
        "hub destination (6000 in-edges)": _hub() + (16, 0.95),
        "E=0, N=300": (e, e, 300, 16, 0.95),
        "shuffled node ids": shuffled_band_graph() + (16, 0.95),
    }
    for n in (255, 256, 257):
        c[f"path N={n}"] = _path(n) + (16, 0.95)
        c[f"random N={n}"] = _random_graph(n, n) + (16, 0.95)
    ncap = cus * 8 * BLOCK + 257
    c["path past the grid cap"] = _path(ncap) + (16, 0.95)
    for d in PE_DIMS:
        c[f"small graph, pe_dim={d}"] = small_graph() + (d, 0.95)
    for a in ALPHAS[1:]:
        c[f"small graph, alpha={a}"] = small_graph() + (16, a)
    for v in c.values():
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def pagerank_want(name, cus=MI355X_CUS):
    """(want64, bound) of a case, computed once and read-only."""
    src, dst, n, pe_dim, alpha = pagerank_cases(cus)[name]
    want = pagerank_pe64(src, dst, n, pe_dim, alpha)
    bound = pagerank_bound(want, max_in_degree(dst, n), pe_dim)
    want.setflags(write=False)
    bound.setflags(write=False)
    return want, bound


# z-score columns: fp32 vectors with a `spread` knob.  spread = 1 is the column as the issue names it; a case doubles it until
# the column's margin reaches 100 (zscore_cases), and records the spread and the condition number it ended with.
def _lengths_uniform(rng, E, spread):
    return rng.integers(500, 30000, E).astype(np.float32)


def _lengths_tight(rng, E, spread):
    w = 3 * spread
    return (20000 + rng.integers(-w, w + 1, E)).astype(np.float32)


def _sim_uniform(rng, E, spread):
    return (1.0 - 0.02 * spread * rng.random(E)).astype(np.float32)          # (1 - 0.02 spread, 1]


def _sim_normal(rng, E, spread):
    return np.minimum(0.999 + 1e-4 * spread * rng.standard_normal(E), 1.0).astype(np.float32)


def _negative(rng, E, spread):
    return (-5.0 - 2.0 * spread * rng.random(E)).astype(np.float32)


def _outlier(rng, E, spread):
    x = rng.integers(500, 30000, E).astype(np.float32)
    x[E // 2] = 1e6
    return x


def _constant(rng, E, spread):
    return np.full(E, 0.75, np.float32)


ZS_E = (2, 3, 255, 256, 257, 2048 * 256 - 1, 2048 * 256 + 257)
ZS_PAIRS = (("lengths uniform [500, 30000)", _lengths_uniform, "similarity uniform under 1", _sim_uniform),
            ("lengths 20000 +- w", _lengths_tight, "similarity 0.999 + s N(0,1), clipped", _sim_normal),
            ("negative", _negative, "one outlier of 1e6", _outlier))
MARGIN = 100.0


def _column(gen, seed, E, nb):
    """The column at the smallest power-of-two spread whose margin reaches MARGIN.  A draw that no spread helps (E = 2 with both
    values clipped to 1, or tied) is drawn again from the next seed."""
    for s in range(seed, seed + 8):
        for spread in (1 << k for k in range(13)):
            x = gen(np.random.default_rng(s), E, spread)
            if zscore_margin(x, nb) >= MARGIN:
                return x, spread
    raise AssertionError(f"no usable spread for {gen.__name__} at E={E}")


def zscore_case_names():
    """The keys of zscore_cases, without building a column (they do not depend on the device)."""
    return [f"E={E}: {na} | {nb_}" for E in ZS_E for na, _, nb_, _ in ZS_PAIRS] + [ZS_CONSTANT]


ZS_CONSTANT = "E=1000: constant | similarity uniform under 1"


@functools.lru_cache(maxsize=None)
def zscore_cases(cus=MI355X_CUS):
    """name -> dict(a, b fp32 [E]; nb; spread, kappa, margin: one per column; accuracy: which columns are under the accuracy
    contract).  The last case has a constant first column: the reference divides by a zero std there."""
    out = {}
    for E in ZS_E:
        nb = zs_blocks(E, cus)
        for k, (na, ga, nb_, gb) in enumerate(ZS_PAIRS):
            a, sa = _column(ga, 1000 * k + E % 997, E, nb)
            b, sb = _column(gb, 1000 * k + 500 + E % 997, E, nb)
            out[f"E={E}: {na} | {nb_}"] = dict(a=a, b=b, nb=nb, spread=(sa, sb), kappa=(_kappa(a), _kappa(b)),
                                               margin=(zscore_margin(a, nb), zscore_margin(b, nb)), accuracy=(True, True))
    E = 1000
    nb = zs_blocks(E, cus)
    b, sb = _column(_sim_uniform, 77, E, nb)
    out[ZS_CONSTANT] = dict(a=_constant(None, E, 1), b=b, nb=nb, spread=(1, sb),
                                                                 kappa=(math.inf, _kappa(b)), margin=(0.0, zscore_margin(b, nb)),
                                                                 accuracy=(False, True))
    assert list(out) == zscore_case_names()
    for v in out.values():
        v["a"].setflags(write=False)
        v["b"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def zscore_want(name, cus=MI355X_CUS):
    """(want64 [E, 2], bound [E, 2]) of a case, computed once and read-only; a column outside the accuracy contract has an
    infinite bar."""
    c = zscore_cases(cus)[name]
    want = zscore64(c["a"], c["b"])
    bound = np.full(want.shape, np.inf)
    for j, x in enumerate((c["a"], c["b"])):
        if c["accuracy"][j]:
            bound[:, j] = zscore_bound(want[:, j], x, c["nb"])
    want.setflags(write=False)
    bound.setflags(write=False)
    return want, bound


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements with a finite bar, and its flat index."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(bound)
    r = np.where(fin, np.abs(got - want) / np.where(fin, bound, 1.0), 0.0)
    r = np.where(fin & ~np.isfinite(got), np.inf, r)
    i = int(np.argmax(r))
    return float(r.flat[i]), i
