"""fp64 reference, column families and componentwise error bounds of the BatchNorm layer kernels (gnm_layer.hip and their H = 128
sweep forms), shared by tests/test_gpu_batchnorm_kernels.py (the device against fp64), tests/test_bn_reference_cpu.py (the reference
against the oracle and autograd) and tools/measure_batchnorm_bounds.py (torch's fp32 CPU batch_norm and its autograd against the same
fp64: where the constants come from).  numpy only.

Column families (FAMILIES; BatchNorm statistics are per column, so every case mixes all of them across its H columns):
  normal    N(0,1) scaled by e^U(-1.5,1.5)                     well conditioned -- also held to the fixed rel-L2 bars
  offset    the same plus 1e3 x its std                         |mean| >> std
  tiny      std 1e-4                                            var << eps: rstd ~ 1/sqrt(eps)
  constant  one value in every row                              var = 0 exactly
  zero      all-zero column
  dominant  one row of the column 1e4 x the rest
and one ROW family, the saturated gates: a few edges with e_in = -100, -30, +30, +100 in every column (sigma exactly 0 or 1 in fp32;
the in-edges of one destination all at -100 / -30, so that its sum sigma is far below the 1e-6 of the denominator).
A one-row case (count = 1: var = 0 in EVERY column) keeps the magnitudes of `normal` in the offset and dominant columns and a beta
well away from 0 everywhere -- pre = beta + (rounding of t scale, ~316 |t| u) leaves no fp32 form a decidable branch otherwise.

One function per kernel, each on what the kernel takes (the fp32 stat / bstat rows the device produced included), evaluated in fp64.
Elementwise outputs come back as (value, A, Rnd): |err| <= c u A + u Rnd, A the sum of the |terms| of the formula, Rnd the final
roundings, c per column family = DEVICE_FACTOR x what torch's fp32 CPU batch_norm shows (profiles/batchnorm_kernel_bounds.json).
Sums over edges or rows come back as (value, bound): the summed per-row bounds plus one u per fp32 addition (times the sum of
|terms|).  The gate sigmoid's hardware forms are given (6 + |x|) u relative, its derivative (8 + |x|) u (see
tests/test_gpu_layernorm_kernels.py), plus FTZ = 2^-126 absolute: v_exp_f32 flushes a denormal sigma (e_out = -100) to 0.
Relu branches: the sign of t scale + shift in fp64 from the fp32 stat row; an element within 4 u (|t scale| + |shift|) of 0 is
UNDECIDED -- either branch is accepted there (elementwise: the nearer of the two; sums: its |term| joins the bound)."""
import json
import os

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
FTZ = 2.0 ** -126
EPS = np.float32(1e-5)              # what engine.bn_finalize hands the kernel (float eps)
EPS_DEN = float(np.float32(1e-6))   # gnm_common.h kEpsDen
FAMILIES = ("normal", "offset", "tiny", "constant", "zero", "dominant")
NORMAL = 0
WIDTHS = (32, 64, 128, 256)
UNDECIDED_CAP = 1e-3
BOUNDS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batchnorm_kernel_bounds.json")
DEVICE_FACTOR = 4.0


def load_constants():
    """{"fwd": c [family], "bwd": c [family]}: DEVICE_FACTOR x the measured fp32-CPU ratios.  A family whose fp32-CPU forward is
    exact (ratio 0) gets the `normal` constant: the kernels' relu(fma(t, scale, shift)) + e_in rounds twice for any t but 0 -- the
    all-zero column with no residual is the one exact case, and the GPU test compares it bit for bit."""
    d = json.load(open(BOUNDS_FILE))["cpu_fp32_ratio"]
    out = {}
    for k in ("fwd", "bwd"):
        c = np.array([DEVICE_FACTOR * d[k][f] for f in FAMILIES])
        out[k] = np.where(c == 0, c[NORMAL], c)
    return out


def f64(a):
    return np.asarray(a, np.float64)


def sigmoid(x):
    ea = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + ea), ea / (1.0 + ea))


def seg(index, val, n):
    out = np.zeros((n, val.shape[1]))
    np.add.at(out, index, val)
    return out


# -----------------------------------------------------------------------------------------
# inputs
# -----------------------------------------------------------------------------------------

def col_families(rng, H, first=0):
    return rng.permutation((np.arange(H) + first) % len(FAMILIES))


def make_cols(rng, R, fam, offset=True, plain=False):
    """fp32 [R,H]: column c drawn from family fam[c]; plain (always for one row): the offset and dominant columns as `normal`."""
    H = fam.size
    s = np.exp(rng.uniform(-1.5, 1.5, (1, H)))
    x = rng.standard_normal((R, H)) * s
    f = lambda name: (fam == FAMILIES.index(name))[None, :]  # noqa: E731
    if R > 1 and not plain:
        if offset:
            x = np.where(f("offset"), x + 1e3 * s, x)
        hot = np.zeros((R, H), bool)
        hot[rng.integers(0, R, H), np.arange(H)] = True
        x = np.where(f("dominant") & hot, 1e4 * x, x)
    x = np.where(f("tiny"), 1e-4 * rng.standard_normal((R, H)), x)
    x = np.where(f("constant"), rng.standard_normal((1, H)) * s * 2.0, x)
    x = np.where(f("zero"), 0.0, x)
    return x.astype(np.float32)


def make_affine(rng, fam, R):
    """gamma, beta fp32 [H]; beta of the constant and zero columns (every column of a one-row case) well away from 0."""
    H = fam.size
    ga = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    be = 0.1 * rng.standard_normal(H)
    far = rng.uniform(0.3, 0.8, H) * rng.choice([-1.0, 1.0], H)
    flat = np.isin(fam, [FAMILIES.index("constant"), FAMILIES.index("zero")]) | (R == 1)
    return ga, np.where(flat, far, be).astype(np.float32)


def make_layer_inputs(seed, idx, N, E, H):
    """The inputs of one layer on a graph (idx: numpy int64 isrc, idst, in_ptr, ... in internal order): dict of fp32 arrays P [N,5H],
    t_in (= B3e) [E,H], e_in [E,H] (with the saturated rows), h_in, gh_out [N,H], ge_out [E,H], gamma / beta _e / _h [H] and fam [H].
    Constant columns: A2h = A3h = 0, so that z stays exactly constant; offset columns: A2h, A3h without the offset."""
    rng = np.random.default_rng(seed)
    fam = col_families(rng, H, seed)
    const = (fam == FAMILIES.index("constant"))[None, :]
    blocks = [make_cols(rng, N, fam, offset=b not in (1, 2), plain=E == 1 and b >= 3) for b in range(5)]      # E = 1: t stays plain
    for b in (1, 2):
        blocks[b] = np.where(const, np.float32(0), blocks[b])
    d = dict(fam=fam, P=np.concatenate(blocks, 1), t_in=make_cols(rng, E, fam))
    d["e_in"] = rng.standard_normal((E, H)).astype(np.float32)
    deg = np.diff(idx["in_ptr"])
    if E >= 8:
        cand = np.nonzero((deg >= 1) & (deg <= 2))[0]
        v = int(cand[0]) if cand.size else int(np.nonzero(deg)[0][0])
        a, b = int(idx["in_ptr"][v]), int(idx["in_ptr"][v + 1])
        d["e_in"][a:b] = np.float32(-100.0)
        d["e_in"][b - 1] = np.float32(-30.0) if b - a > 1 else np.float32(-100.0)
        rest = np.setdiff1d(np.arange(E), np.arange(a, b))
        d["e_in"][rest[E // 3]], d["e_in"][rest[E // 2]], d["e_in"][rest[-1]] = 30.0, 100.0, -30.0
        d["empty_gate_node"] = v
    d["h_in"], d["gh_out"] = (rng.standard_normal((N, H)).astype(np.float32) for _ in range(2))
    d["ge_out"] = rng.standard_normal((E, H)).astype(np.float32)
    d["gamma_e"], d["beta_e"] = make_affine(rng, fam, E)
    d["gamma_h"], d["beta_h"] = make_affine(rng, fam, N)
    return d


# -----------------------------------------------------------------------------------------
# statistics
# -----------------------------------------------------------------------------------------

def col_sums(x, y=None):
    """(sum x, sum x y) per column in fp64 and the sums of the |terms| (y None: x itself, the forward's sum x^2)."""
    x = f64(x)
    y = x if y is None else f64(y)
    acc = lambda a: np.asarray(a, np.longdouble).sum(0).astype(np.float64)  # noqa: E731  (80-bit accumulation: numpy adds rows one by one)
    return np.stack([acc(x), acc(x * y)]), np.stack([np.abs(x).sum(0), np.abs(x * y).sum(0)])


def bn_finalize_ref(sums, count, eps=EPS):
    """(mean, rstd) in fp64 from the column sums [2,H] = (sum x, sum x^2): biased variance, clamped at 0."""
    mean = sums[0] / count
    var = np.maximum(sums[1] / count - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + float(eps))


def stat_rows32(mean32, rstd32, gamma, beta):
    """scale, shift in fp64 from the fp32 mean / rstd a finaliser wrote (what the next two fp32 operations start from)."""
    scale = f64(gamma) * f64(rstd32)
    scale32 = f64(scale.astype(np.float32))
    return scale, f64(beta) - f64(mean32) * scale32


def stat_from_data(x, gamma, beta, eps=EPS):
    """float32 [4,H] stat row of the fp32 data x, as gnm_bn_finalize forms it (fp64 sums, fp32 scale and shift)."""
    s, _ = col_sums(x)
    mean, rstd = bn_finalize_ref(s, x.shape[0], eps)
    mean32, rstd32 = mean.astype(np.float32), rstd.astype(np.float32)
    scale32 = (np.float32(1) * gamma.astype(np.float32) * rstd32).astype(np.float32)
    shift32 = (beta.astype(np.float32) - (mean32 * scale32).astype(np.float32)).astype(np.float32)
    return np.stack([mean32, rstd32, scale32, shift32])


def xhat32(x, stat):
    """(x - mean) rstd as every backward kernel forms it: two fp32 operations, reproduced exactly."""
    x = np.asarray(x, np.float32)
    return f64(((x - stat[0][None, :].astype(np.float32)).astype(np.float32) * stat[1][None, :].astype(np.float32)).astype(np.float32))


def bwd_finalize_ref(sums, count):
    """bstat [2,H] = (mean gy, mean gy xhat), ggamma = sum gy xhat, gbeta = sum gy."""
    return sums / count, sums[1], sums[0]


# -----------------------------------------------------------------------------------------
# forward
# -----------------------------------------------------------------------------------------

def t_stats_ref(t_in, P, isrc, idst):
    """t = B3e + B1h[src] + B2h[dst]: (t, A, Rnd), two fp32 additions (c = 1)."""
    H = t_in.shape[1]
    b1, b2 = f64(P)[:, 3 * H:4 * H][isrc], f64(P)[:, 4 * H:5 * H][idst]
    t = f64(t_in) + b1 + b2
    return t, np.abs(f64(t_in)) + np.abs(b1) + np.abs(b2), np.abs(t)


def branch(x, stat):
    """(pre, A, undecided) of pre = x scale + shift from the fp32 stat row."""
    sx = f64(x) * f64(stat[2])[None, :]
    pre = sx + f64(stat[3])[None, :]
    A = np.abs(sx) + np.abs(f64(stat[3]))[None, :]
    return pre, A, np.abs(pre) <= 4 * U * A


def bn_apply_ref(x, stat, resid=None):
    """relu(x scale + shift) + resid (gnm_edge_gate_fwd's e_out, gnm_node_update_fwd's h_out): (out, A, Rnd, undecided)."""
    pre, A, und = branch(x, stat)
    out = np.maximum(pre, 0.0)
    Rnd = np.abs(pre)
    if resid is not None:
        out = out + f64(resid)
        Rnd = Rnd + np.abs(out)
    return out, A, Rnd, und


def apply_bound(A, Rnd, und, c_cols):
    return c_cols[None, :] * U * A + U * Rnd + und * 4 * U * A + FTZ


def gated_mean_ref(e_out, d_e, a_other, at, n, eps_den=EPS_DEN):
    """h[v] = sum_at sigma a / (sum_at sigma + 1e-6) and inv = 1 / (sum_at sigma + 1e-6) with sigma = sigmoid(e_out) of the e_out
    the kernel holds (error d_e: 0 where it reads a stored e_out): ((h, d_h), (inv, d_inv))."""
    e_out, a_other = f64(e_out), f64(a_other)
    deg = np.bincount(at, minlength=n)[:, None].astype(np.float64)
    sig = sigmoid(e_out)
    d_sig = 0.25 * d_e + (6 + np.abs(e_out)) * U * sig + FTZ
    den, num = seg(at, sig, n), seg(at, sig * a_other, n)
    inv = 1.0 / (den + eps_den)
    d_inv = inv * inv * (seg(at, d_sig, n) + (deg + 1) * U * (den + eps_den)) + 2 * U * inv
    d_num = seg(at, d_sig * np.abs(a_other), n) + (deg + 1) * U * seg(at, sig * np.abs(a_other), n)
    d_h = d_num * inv + np.abs(num) * d_inv + U * np.abs(num * inv) + FTZ
    return (num * inv, d_h), (inv, d_inv)


def z_ref(P, hf, d_hf, hb, d_hb):
    H = hf.shape[1]
    a1 = f64(P)[:, :H]
    z = a1 + f64(hf) + f64(hb)
    return z, d_hf + d_hb + 2 * U * (np.abs(a1) + np.abs(f64(hf)) + np.abs(f64(hb))) + FTZ


# -----------------------------------------------------------------------------------------
# backward
# -----------------------------------------------------------------------------------------

def bn_bwd_apply_ref(x, stat, bstat, gamma, gy, mask):
    """gx = gamma rstd (gy [mask] - m1 - xhat m2) (gnm_node_bwd_apply's gz, gnm_edge_bwd_gt's gt): (gx, A, Rnd).  A carries the
    column means of |gy| and |gy xhat| beside |m1| and |m2|: what a fp32 summation of m1, m2 is uncertain by."""
    xh = xhat32(x, stat)
    g = f64(gy) * mask
    c = (f64(gamma) * f64(stat[1]))[None, :]
    m1, m2 = f64(bstat[0])[None, :], f64(bstat[1])[None, :]
    gx = c * (g - m1 - xh * m2)
    M1, M2 = np.abs(g).mean(0, keepdims=True), np.abs(g * xh).mean(0, keepdims=True)
    A = np.abs(c) * (np.abs(g) + np.abs(m1) + M1 + np.abs(xh) * (np.abs(m2) + M2))
    return gx, A, np.abs(gx)


def either_branch(got, x, stat, bstat, gamma, gy, c_cols, scale=None):
    """|got - gx| / bound per element, with the nearer branch at the undecided elements; scale: a further exact factor per element
    (Q = gz inv_f: the product adds one rounding)."""
    pre, _, und = branch(x, stat)
    worst = None
    for flip in (False, True):
        mask = (pre > 0) ^ (und & flip)
        gx, A, Rnd = bn_bwd_apply_ref(x, stat, bstat, gamma, gy, mask)
        if scale is not None:
            gx, A, Rnd = gx * scale, A * np.abs(scale), 2 * np.abs(gx * scale)
        frac = np.abs(f64(got) - gx) / (c_cols[None, :] * U * A + U * Rnd + FTZ)
        worst = frac if worst is None else np.minimum(worst, frac)
        if not und.any():
            break
    return worst, und


def edge_bwd_dst_ref(e_out, ge0, P, Q, hf, hb, isrc, idst):
    """ge <- ge + gsigma sigma'(e_out) in place and gP[:, 2H:3H] = sum_dst sigma Qb[src]: ((g, d_g), (gA3h, bound))."""
    H = e_out.shape[1]
    N = hf.shape[0]
    e_out, ge0, P, Q, hf, hb = (f64(a) for a in (e_out, ge0, P, Q, hf, hb))
    deg_in = np.bincount(idst, minlength=N)[:, None].astype(np.float64)
    sig = sigmoid(e_out)
    dsg = sig * (1 - sig)
    d_sig = (6 + np.abs(e_out)) * U * sig + FTZ
    d_dsg = (8 + np.abs(e_out)) * U * dsg + FTZ
    qf_d, qb_s = Q[:, :H][idst], Q[:, H:][isrc]
    a2_s, a3_d = P[:, H:2 * H][isrc], P[:, 2 * H:3 * H][idst]
    rf_d, rb_s = qf_d * hf[idst], qb_s * hb[isrc]
    gsig = qf_d * a2_s + qb_s * a3_d - rf_d - rb_s
    S = np.abs(qf_d * a2_s) + np.abs(qb_s * a3_d) + np.abs(rf_d) + np.abs(rb_s)
    g = ge0 + gsig * dsg
    d_g = np.abs(gsig) * d_dsg + 5 * U * S * dsg + U * (np.abs(ge0) + np.abs(g)) + FTZ
    a3 = seg(idst, sig * qb_s, N)
    d_a3 = seg(idst, d_sig * np.abs(qb_s), N) + (deg_in + 1) * U * seg(idst, sig * np.abs(qb_s), N) + FTZ
    return (g, d_g), (a3, d_a3)


def masked_sums_ref(ge, t, stat, at, n):
    """Of gu = ge [t scale + shift > 0] and that = xhat32(t): the per-node sums (sum_at gu, sum_at that) with their bounds (one u per
    fp32 addition, the undecided |ge| on top), the column sums (sum gu, sum gu that) with the sums of their |terms| and the undecided
    share of each column sum: dict."""
    pre, _, und = branch(t, stat)
    gu = f64(ge) * (pre > 0)
    th = xhat32(t, stat)
    deg = np.bincount(at, minlength=n)[:, None].astype(np.float64)
    gund = np.abs(f64(ge)) * und
    sums, mags = col_sums(gu, th)
    return dict(gu=gu, th=th, und=und, U=seg(at, gu, n), d_U=deg * U * seg(at, np.abs(gu), n) + seg(at, gund, n) + FTZ,
                T=seg(at, th, n), d_T=deg * U * seg(at, np.abs(th), n) + FTZ, sums=sums, mags=mags,
                sums_und=np.stack([gund.sum(0), (gund * np.abs(th)).sum(0)]), absU=seg(at, np.abs(gu) + gund, n), absT=seg(at, np.abs(th), n))


def bgrad_ref(Us, Ts, deg, stat, bstat, gamma):
    """c (Us - deg m1 - m2 Ts), c = gamma rstd, from the raw per-node sums (gnm_edge_bwd_src's gB1h / gB2h, gnm_node_bgrad):
    (value, bound): six fp32 operations on A = |c| (|Us| + deg |m1| + |m2 Ts|)."""
    c = (f64(gamma) * f64(stat[1]))[None, :]
    m1, m2 = f64(bstat[0])[None, :], f64(bstat[1])[None, :]
    val = c * (f64(Us) - deg * m1 - m2 * f64(Ts))
    A = np.abs(c) * (np.abs(f64(Us)) + deg * np.abs(m1) + np.abs(m2 * f64(Ts)))
    return val, 6 * U * A + FTZ


def gated_sum_ref(e_out, q_other, at, n):
    """sum_at sigma(e_out) q_other (gA2h by source with Qf[dst]): (value, bound)."""
    e_out, q_other = f64(e_out), f64(q_other)
    deg = np.bincount(at, minlength=n)[:, None].astype(np.float64)
    sig = sigmoid(e_out)
    d_sig = (6 + np.abs(e_out)) * U * sig + FTZ
    return seg(at, sig * q_other, n), seg(at, d_sig * np.abs(q_other), n) + (deg + 1) * U * seg(at, sig * np.abs(q_other), n) + FTZ


# -----------------------------------------------------------------------------------------
# the reference composed: one layer end to end in fp64 (statistics in fp64 too)
# -----------------------------------------------------------------------------------------

def layer_ref(d, idx, N, h_in=None, e_in=None, masks=None):
    """Forward and backward of one layer from make_layer_inputs' arrays with the functions above, every statistic kept in fp64 and
    the module's double constants (eps 1e-5, 1e-6; the kernels take their float values)
    (tests/test_bn_reference_cpu.py: equals oracle.manual_forward_backward's layer and fp64 autograd).  Edge rows in internal order."""
    isrc, idst = idx["isrc"], idx["idst"]
    H = d["t_in"].shape[1]
    P = f64(d["P"])
    e_in = f64(d["e_in"]) if e_in is None else e_in
    h_in = f64(d["h_in"]) if h_in is None else h_in
    o = {}
    o["t"], _, _ = t_stats_ref(d["t_in"], P, isrc, idst)

    def stat64(x, ga, be):
        mean, rstd = bn_finalize_ref(col_sums(x)[0], x.shape[0], 1e-5)
        scale = f64(ga) * rstd
        return np.stack([mean, rstd, scale, f64(be) - mean * scale])

    def xh64(x, st):
        return (x - st[0][None, :]) * st[1][None, :]
    se = o["stat_e"] = stat64(o["t"], d["gamma_e"], d["beta_e"])
    o["e_out"] = np.maximum(xh64(o["t"], se) * f64(d["gamma_e"]) + f64(d["beta_e"]), 0) + e_in
    zero = np.zeros_like(o["e_out"])
    (o["hf"], _), (o["inv_f"], _) = gated_mean_ref(o["e_out"], zero, P[:, H:2 * H][isrc], idst, N, 1e-6)
    (o["hb"], _), (o["inv_b"], _) = gated_mean_ref(o["e_out"], zero, P[:, 2 * H:3 * H][idst], isrc, N, 1e-6)
    o["z"], _ = z_ref(P, o["hf"], 0.0, o["hb"], 0.0)
    sh = o["stat_h"] = stat64(o["z"], d["gamma_h"], d["beta_h"])
    w = xh64(o["z"], sh) * f64(d["gamma_h"]) + f64(d["beta_h"])
    o["h_out"] = np.maximum(w, 0) + h_in
    # backward
    mw = (w > 0) if masks is None else masks[1]
    gw = f64(d["gh_out"]) * mw
    zh = xh64(o["z"], sh)
    bs = col_sums(gw, zh)[0]
    o["bstat_h"], o["ggamma_h"], o["gbeta_h"] = bwd_finalize_ref(bs, N)
    c = (f64(d["gamma_h"]) * sh[1])[None, :]
    o["gz"] = c * (gw - o["bstat_h"][0] - zh * o["bstat_h"][1])
    o["Q"] = np.concatenate([o["gz"] * o["inv_f"], o["gz"] * o["inv_b"]], 1)
    (o["ge"], _), (o["gA3h"], _) = edge_bwd_dst_ref(o["e_out"], d["ge_out"], P, o["Q"], o["hf"], o["hb"], isrc, idst)
    u = xh64(o["t"], se) * f64(d["gamma_e"]) + f64(d["beta_e"])
    mu = (u > 0) if masks is None else masks[0]
    gu, th = o["ge"] * mu, xh64(o["t"], se)
    be_ = col_sums(gu, th)[0]
    o["bstat_e"], o["ggamma_e"], o["gbeta_e"] = bwd_finalize_ref(be_, gu.shape[0])
    o["Ud"], o["Td"] = seg(idst, gu, N), seg(idst, th, N)
    o["gA2h"], _ = gated_sum_ref(o["e_out"], o["Q"][:, :H][idst], isrc, N)
    ce = (f64(d["gamma_e"]) * se[1])[None, :]
    o["gt"] = ce * (gu - o["bstat_e"][0] - th * o["bstat_e"][1])
    deg_in, deg_out = (np.bincount(a, minlength=N)[:, None].astype(np.float64) for a in (idst, isrc))
    st_e = np.stack([se[0], se[1]])
    o["gB1h"], _ = bgrad_ref(seg(isrc, gu, N), seg(isrc, th, N), deg_out, st_e, o["bstat_e"], d["gamma_e"])
    o["gB2h"], _ = bgrad_ref(o["Ud"], o["Td"], deg_in, st_e, o["bstat_e"], d["gamma_e"])
    o["gP"] = np.concatenate([o["gz"], o["gA2h"], o["gA3h"], o["gB1h"], o["gB2h"]], 1)
    return o


def undecided_share(d, idx, N):
    """The share of undecided relu elements (edge and node side together) of a case, from the fp64 reference alone with the stat rows
    rounded to fp32 as the finaliser leaves them."""
    o = layer_ref(d, idx, N)
    n = 0
    for x, ga, be in ((o["t"], d["gamma_e"], d["beta_e"]), (o["z"], d["gamma_h"], d["beta_h"])):
        x32 = x.astype(np.float32)
        n += int(branch(x32, stat_from_data(x32, ga, be))[2].sum())
    return n / (o["t"].size + o["z"].size)


# -----------------------------------------------------------------------------------------
# the cases of tests/test_gpu_batchnorm_kernels.py::test_generic_kernels_vs_fp64 (test_bn_reference_cpu.py caps their undecided share)
# -----------------------------------------------------------------------------------------

def _kblock():
    import re
    src = open(os.path.join(os.path.dirname(BOUNDS_FILE), "..", "gnnome_assembly_amd", "csrc", "gnm_common.h")).read()
    return int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))


def cases(H):
    """(name, src, dst, n): a one-node self loop, paths with E (and with N = E + 1) = 1, RPW - 1, RPW, RPW + 1, 4 RPW - 1, 4 RPW,
    4 RPW + 1, 15, 16, 17 (RPW = 256 / H rows per wave, 4 waves per workgroup, 16 rows per sweep tile), a path of 8 kBlock + 3 edges
    (several workgroups, a ragged last one), synth.tiny_edge_case_graph and the hub graph of helpers.replica_base_graph."""
    from gnnome_assembly_amd import synth
    from helpers import replica_base_graph
    rpw = 256 // H
    sizes = {1, rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw, 4 * rpw + 1, 15, 16, 17}
    es = sorted({s for s in sizes | {s - 1 for s in sizes} if s >= 1}) + [8 * _kblock() + 3]
    out = [("selfloop", np.array([0]), np.array([0]), 1)] + [(f"path{e}", np.arange(e), np.arange(e) + 1, e + 1) for e in es]
    out.append(("tiny_edge_case",) + tuple(synth.tiny_edge_case_graph()))
    out.append(("hub",) + tuple(replica_base_graph(reads=300, hub_in=300)))
    return out


def case_seed(H, i):
    return 1000 * H + i


SWEEP_CASE = 99     # case_seed(H, SWEEP_CASE): the hub graph's inputs in the sweep test
