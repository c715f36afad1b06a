"""fp64 reference, row families and componentwise error bounds of the LayerNorm kernels (gnm_layernorm.hip, gnm_ln.h), shared by
tests/test_gpu_layernorm_kernels.py (the device against fp64) and tools/measure_layernorm_bounds.py (the fp32 CPU reference,
torch.nn.functional.layer_norm and its autograd, against the same fp64: where the constants in LN_BOUNDS come from).

Row families (FAMILIES; every case mixes all of them, row i gets family i % 6 under a fixed shuffle):
  normal    N(0,1) scaled by e^U(-3,3)                       well conditioned -- also held to the fixed rel-L2 bars
  offset    the same plus a common offset of 1e3 x its std    |mean| >> std
  tiny      std 1e-4                                          var << eps: rstd ~ 1/sqrt(eps)
  constant  one value in every live channel (up to ~100)      var = 0 exactly: xhat = 0 in fp64, (mean's rounding) x rstd in fp32
  zero      all-zero rows                                     everything exact in fp32
  dominant  one channel 1e4 x the rest

Bounds.  u = 2^-24.  Per row: rstd, xhat from fp64; X = max|x| * rstd (how much a rounding error of the mean is magnified) and
per element ex = X + |xhat|.  fp32 LayerNorm cannot do better than |d xhat| ~ u * ex whatever the summation order, and the relative
error of rstd is of the order u * X (d var ~ 2 sqrt(var) |d mean|, times rstd^2 / 2).  Propagated to first order through the kernels' formulas:
  pre = xhat*gamma + beta          |err| <= c u ex |gamma|                                                  + u |pre|
  gx  = rstd (a - m1 - xhat m2)    |err| <= c u rstd [(1 + X)(|a| + mean|a| + |xhat| mean|a xhat|) + ex |m2| + |xhat| mean(|a| ex)] + u |gx|
with a = gamma * gy, m1 = mean(a), m2 = mean(a * xhat) over the live channels.  The first term scales with the one constant c of
the row's family, the second is the final rounding.  c is NOT tuned on the kernels: tools/measure_layernorm_bounds.py measures the
worst (|err| - rounding) / (u * [...]) of torch's fp32 CPU layer_norm per family over every (H, width) of the tests, and the device
is allowed 4 x that (butterfly against sequential sums, v_rcp / rsqrt forms).  A family whose fp32 CPU result is exact is compared exactly."""
import json
import os

import numpy as np

U = 2.0 ** -24
EPS = 1e-5
FAMILIES = ("normal", "offset", "tiny", "constant", "zero", "dominant")
HW = [(32, 32), (32, 20), (64, 64), (64, 48), (128, 128), (128, 96), (256, 256), (256, 200)]
BOUNDS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "layernorm_kernel_bounds.json")
DEVICE_FACTOR = 4.0


def load_constants():
    """{"fwd": c [family], "bwd": c [family], "fwd_exact": bool [family]} -- c = DEVICE_FACTOR x the measured fp32-CPU ratios of
    profiles/layernorm_kernel_bounds.json; fwd_exact: the CPU reference is bit-exact for that family, and so must the device be."""
    d = json.load(open(BOUNDS_FILE))
    out = {k: np.array([DEVICE_FACTOR * d["cpu_fp32_ratio"][k][f] for f in FAMILIES]) for k in ("fwd", "bwd")}
    out["fwd_exact"] = np.array([bool(d["cpu_fp32_exact"]["fwd"][f]) for f in FAMILIES])
    return out


def make_rows(rng, R, H, width, first=0):
    """x fp32 [R,H] (dead channels 0) and fam int [R]: the families above, interleaved and shuffled; row 0 of a one-row case is
    family `first` % 6."""
    fam = (np.arange(R) + first) % len(FAMILIES)
    if R > 1:
        fam = rng.permutation(fam)
    s = np.exp(rng.uniform(-3, 3, (R, 1)))
    x = rng.standard_normal((R, H)) * s
    f = lambda name: (fam == FAMILIES.index(name))[:, None]  # noqa: E731
    x = np.where(f("offset"), x + 1e3 * s, x)
    x = np.where(f("tiny"), 1e-4 * rng.standard_normal((R, H)), x)
    x = np.where(f("constant"), rng.standard_normal((R, 1)) * s * 5.0, x)
    x = np.where(f("zero"), 0.0, x)
    hot = np.zeros((R, H), bool)
    hot[np.arange(R), rng.integers(0, width, R)] = True
    x = np.where(f("dominant") & hot, 1e4 * x, x)
    x = x.astype(np.float32)
    x[:, width:] = 0
    return x, fam


def make_affine(rng, H, width):
    """gamma, beta fp32 [H]; the dead channels as models._pad_param leaves them (gamma 1, beta 0)."""
    ga = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    be = (0.1 * rng.standard_normal(H)).astype(np.float32)
    ga[width:], be[width:] = 1.0, 0.0
    return ga, be


def ln_ref(x, gamma, beta, width):
    """fp64 LayerNorm over the first `width` channels of the fp32 rows x [R,H]: dict of [R,H] arrays (dead channels 0) xhat, pre,
    ex and [R,1] rstd, X."""
    x = np.asarray(x, np.float64)
    R, H = x.shape
    xl = x[:, :width]
    mu = xl.mean(1, keepdims=True)
    var = ((xl - mu) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + EPS)
    xh = np.zeros((R, H))
    xh[:, :width] = (xl - mu) * rstd
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    X = np.abs(xl).max(1, keepdims=True) * rstd
    live = (np.arange(H) < width)[None, :]
    ex = (X + np.abs(xh)) * live
    pre = (xh * g + b) * live
    assert np.isfinite(pre).all() and np.isfinite(X).all()
    return dict(xhat=xh, pre=pre, rstd=rstd, X=X, ex=ex, live=live, width=width, gamma=g)


def fwd_bound(ref):
    """(A, Rnd): |pre_got - pre| <= c u A + u Rnd."""
    return ref["ex"] * np.abs(ref["gamma"]), np.abs(ref["pre"])


def ln_bwd_ref(ref, gy):
    """gx = LNbwd(gy) in fp64 (gy [R,H], taken as 0 in the dead channels) and its bound parts (A, Rnd)."""
    w, live, xh, r, X, ex = ref["width"], ref["live"], ref["xhat"], ref["rstd"], ref["X"], ref["ex"]
    a = ref["gamma"] * np.asarray(gy, np.float64) * live
    mean = lambda v: v[:, :w].mean(1, keepdims=True)  # noqa: E731
    m1, m2 = mean(a), mean(a * xh)
    gx = r * (a - m1 - xh * m2) * live
    A = r * ((1 + X) * (np.abs(a) + mean(np.abs(a)) + np.abs(xh) * mean(np.abs(a * xh))) + ex * np.abs(m2)
             + np.abs(xh) * mean(np.abs(a) * ex)) * live
    assert np.isfinite(gx).all() and np.isfinite(A).all()
    return gx, A, np.abs(gx)


def worst_ratio(err, A, Rnd, fam):
    """Per family: max over its rows' elements of (|err| - u Rnd)+ / (u A); an element with A = 0 must be within its rounding."""
    over = np.maximum(np.abs(err) - U * Rnd, 0.0)
    assert not (over[A == 0] > 0).any(), "error beyond rounding where the bound has no scalable part"
    q = np.divide(over, U * A, out=np.zeros_like(over), where=A > 0)
    return np.array([q[fam == f].max() if (fam == f).any() else 0.0 for f in range(len(FAMILIES))])


def check(name, got, want, A, Rnd, c_rows, exact_rows=None):
    """Every element: |got - want| <= c u A + u Rnd with the row's constant c_rows [R]; rows of `exact_rows` (bool [R]) bit-equal
    to float32(want).  No element is left out.  Returns the worst used fraction of the bound (for the report)."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), f"{name}: shape / non-finite"
    err = np.abs(got - want)
    bound = c_rows[:, None] * U * A + U * Rnd
    if exact_rows is not None and exact_rows.any():
        w32 = want[exact_rows].astype(np.float32).astype(np.float64)
        assert np.array_equal(got[exact_rows], w32), f"{name}: rows that are exact in fp32 differ (max {np.abs(got[exact_rows] - w32).max():.3e})"
    bad = err > bound
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.size} elements outside the bound, worst err/bound "
                           f"{(err[bad] / np.maximum(bound[bad], 1e-300)).max():.3g} at {np.argwhere(bad)[:4].tolist()}")
    return float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())
