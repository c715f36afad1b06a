"""fp64 reference of the node projection entry points (gnm_node_proj_fwd, gnm_node_proj_bwd_nn(_stats), gnm_node_proj_bwd_tn,
gnm_tn128, gnm_tn128_bgrad), the row counts of their tests and the launch arithmetic those row counts come from.  numpy only;
the products, families and bounds are tests/gemm_reference.py's, the BatchNorm pieces tests/bn_reference.py's.

    case(kind, family, N, ncols)          operands and fp64 results of one case, computed once and read-only
    stats_ref(gh_in, z, stat)             (sum gw, sum gw zhat), gw = gh_in [z scale + shift > 0], from the fp32 gh_in a kernel wrote
    bgrad_groups_ref(...)                 gB1h | gB2h from the raw sums (bn_reference.bgrad_ref), with their bound
    degrees_graph(N)                      a graph on N nodes with nodes of in- / out-degree 0 and one hub
    ROWS, rows_for(tile)                  the row counts every entry runs at
    nn_grid / tn_nslot / fwd_nslot_max    the launch arithmetic of gnm_fused.hip, restated

Launch arithmetic (read in gnm_fused.hip / gnm_common.h; CUS = the device's compute units, cap = gnm_set_occupancy_cap):
    persistent_grid(items, min, occ)   min(cdiv(items, min), CUS * min(occ, cap), 2048) rounded UP to a multiple of 8
    forward, f32                       persistent_grid(cdiv(N, 64), 2, occ) workgroups over 64-row tiles
    forward, split modes               nslot = CUS * occ / 5 rounded DOWN to 8, at most cdiv(N, 64) rounded up to 8, at least 8 (no cap)
    backward NN, f32                   persistent_grid(cdiv(N, 64), 2, occ) over 64-row tiles
    backward NN (+ stats), split       persistent_grid(cdiv(N, 128), 1, occ) over groups of four 32-row tiles; *nblk_out = the grid
    TN (tn_colgroups)                  nslot = min(CUS * min(occ, max_blocks_per_cu) / ncg, 2048 / ncg, ntiles) rounded DOWN to 8,
                                       at least 8; tiles of 32 rows (split modes, and _bgrad) or 64 (f32); cdiv(ntiles, nslot) per slot.
                                       N < 32 (less than one tile of the split kernel) runs the f32 kernel in every mode, _bgrad
                                       behind gnm_node_bgrad: K = 1, 2, 3 have c(K) < 3, below what the split terms drop per product
occ (hipOccupancyMaxActiveBlocksPerMultiprocessor, at most 8) is not visible from outside: under cap = 1 / max_blocks_per_cu = 1 it
is 1; elsewhere the tests take its upper bound 8 for the row count and read the slot count a TN launch really used back from the
partial rows it wrote."""
import numpy as np

import bn_reference as br
import gemm_reference as gr
from gemm_reference import NN, NT, TN

H = 128
XCDS = 8
MAX_PARTIAL_BLOCKS = 2048
ROWS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
FAMILIES = ("ints", "normal", "rows", "cancel")       # ints first: a misplaced tile reads as one, not as a bound missed


def cdiv(a, b):
    return -(-a // b)


def rows_for(tile):
    """ROWS and 8 tile - 1, 8 tile, 8 tile + 1: the first sizes at which none of the 8 forced slots is empty."""
    return tuple(sorted(set(ROWS) | {8 * tile - 1, 8 * tile, 8 * tile + 1}))


def tile_rows(mode, forward=False):
    return 64 if mode == "f32" or forward else 32


def families(K):
    return [f for f in FAMILIES if f != "cancel" or gr.uses_cancel(K)]


# ---- launch arithmetic ---------------------------------------------------------------------------------------------------------

def persistent_grid(items, min_items, blocks_per_cu, cus):
    want = min(cdiv(items, min_items), min(cus * blocks_per_cu, MAX_PARTIAL_BLOCKS))
    return cdiv(max(want, 1), XCDS) * XCDS


def nn_grid(N, mode, cus, blocks_per_cu):
    """(workgroups, items per workgroup, rows per item) of the backward NN launch."""
    if mode == "f32":
        nt = cdiv(N, 64)
        g = persistent_grid(nt, 2, blocks_per_cu, cus)
        return g, cdiv(nt, g), 64
    ng = cdiv(N, 128)
    g = persistent_grid(ng, 1, blocks_per_cu, cus)
    return g, cdiv(ng, g), 128


def tn_nslot(N, tile, ncg, cus, blocks_per_cu):
    """(slots, tiles per slot) of tn_colgroups."""
    nt = cdiv(N, tile)
    n = min(cus * blocks_per_cu // ncg, MAX_PARTIAL_BLOCKS // ncg, nt) // XCDS * XCDS
    n = max(n, XCDS)
    return n, cdiv(nt, n)


def fwd_nslot_max(cus, ncg=5):
    """The split-mode forward's slot count at the largest occupancy (8)."""
    return max(cus * 8 // ncg // XCDS * XCDS, XCDS)


def first_rows_with_two_items(rows_per_item, per_block, ragged):
    """The smallest N = (items - 1) rows_per_item + ragged whose launch gives some workgroup two items (per_block(N) >= 2)."""
    items = 2
    while per_block((items - 1) * rows_per_item + ragged) < 2:
        items += 1
    return (items - 1) * rows_per_item + ragged


# ---- cases -----------------------------------------------------------------------------------------------------------------------

_CASES = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def case(kind, family, N, ncols=5 * H):
    """kind "fwd": h [N,128], W [ncols,128], b -> P = h W^T + b.   "nn": gP [N,ncols], W [ncols,128], gh_out -> gh_in = gh_out + gP W.
    "tn": gP [N,ncols], h_in [N,128] -> gW = gP^T h_in [ncols,128], gb = sum gP.  Each with absprod and the epilogue term of
    gemm_reference.bound; K = 128, ncols, N."""
    key = (kind, family, N, ncols)
    if key in _CASES:
        return _CASES[key]
    seed = 11 + 3 * N + ncols
    if kind == "fwd":
        A, B, bias, _ = gr.operands(family, NT, N, ncols, H, seed, epi=True)
        d = dict(h=A, W=B, b=bias, K=H, ref=gr.ref(NT, A, B, bias), absprod=gr.absprod(NT, A, B), epi=gr.epilogue(NT, A, B, bias))
    elif kind == "nn":
        A, B, _, resid = gr.operands(family, NN, N, H, ncols, seed + 1, epi=True)
        d = dict(gP=A, W=B, gh_out=resid, K=ncols, ref=gr.ref(NN, A, B, None, resid), absprod=gr.absprod(NN, A, B),
                 epi=gr.epilogue(NN, A, B, None, resid))
    elif kind == "tn":
        A, B, _, _ = gr.operands(family, TN, ncols, H, N, seed + 2)
        cs, csabs = gr.colsum_ref(A)
        d = dict(gP=A, h_in=B, K=N, ref=gr.ref(TN, A, B), absprod=gr.absprod(TN, A, B), epi=None, cs=cs, csabs=csabs)
    else:
        raise ValueError(kind)
    _CASES[key] = _freeze(d)
    return d


def tn_from(A, B):
    """out, absprod, colsum of a TN launch from the fp32 operand rows it read (A [N, ncg 128], B [N, 128])."""
    return gr.ref(TN, A, B), gr.absprod(TN, A, B), gr.colsum_ref(A)[0]


def lower_layer(N, seed):
    """z_lo [N,128] and the stat row gnm_bn_finalize would leave for it (beta well away from 0: a one-row z has var = 0 and
    pre = beta everywhere)."""
    rng = np.random.default_rng([seed, N])
    z = rng.standard_normal((N, H)).astype(np.float32)
    ga = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    be = (rng.uniform(0.3, 0.8, H) * rng.choice([-1.0, 1.0], H)).astype(np.float32)
    return z, br.stat_from_data(z, ga, be), ga, be


def stats_ref(gh_in, z, stat):
    """gnm_node_bwd_stats of the layer below on the fp32 gh_in a kernel wrote: dict(sums [2,H] = (sum gw, sum gw zhat), mags: the
    sums of the |terms|, und: what the rows with an undecided relu branch may add or take away, share: their share)."""
    pre, _, und = br.branch(z, stat)
    g = gr.f64(gh_in)
    gw, zh = g * (pre > 0), br.xhat32(z, stat)
    sums, mags = br.col_sums(gw, zh)
    gund = np.abs(g) * und
    return dict(sums=sums, mags=mags, und=np.stack([gund.sum(0), (gund * np.abs(zh)).sum(0)]), share=float(und.mean()), n_und=int(und.sum()))


def stats_bound(s, N, nblk):
    """fp64 sums of N exact terms (a float, and the product of two floats, are exact in fp64) in any order: (N - 1) 2^-53 sum |x|;
    the test adds the nblk partial rows once more."""
    return (N + nblk) * br.U64 * s["mags"] + s["und"] + br.FTZ


# ---- gnm_tn128_bgrad ----------------------------------------------------------------------------------------------------------------

def degrees_graph(N, hub=True):
    """(src, dst): a path over the even nodes, every third node -> node 0 (the hub), the odd nodes that are no multiple of three with
    no edge at all; the last path node has no out-edge, node 2 (N > 3) no in-edge but the hub's own.  N = 1: one self loop."""
    if N == 1:
        return np.array([0]), np.array([0])
    ev = np.arange(2, N, 2) if N > 3 else np.arange(0, N, 2)
    src, dst = list(ev[:-1]), list(ev[1:])
    t = np.arange(3, N, 3) if hub else np.arange(0)
    src += list(t)
    dst += [0] * len(t)
    if not src:
        src, dst = [1], [0]
    return np.asarray(src), np.asarray(dst)


def bgrad_inputs(N, family, seed, small=False):
    """UT = [Us | Ts] [N,2H], Ud, Td [N,H], stat_e [4,H] (rows 0, 2, 3 are not read), bstat_e [2,H], gamma_e [H], h_in [N,H].
    ints: rstd = 1, gamma = 1, means 0 -> the groups are Us, Ud;  ints2: gamma a power of two, integer means."""
    rng = np.random.default_rng([seed, N, len(family)])
    f32 = np.float32
    if family in ("ints", "ints2"):
        Us, Ts, Ud, Td, h_in = (rng.integers(-8, 9, (N, H)).astype(f32) for _ in range(5))
        if small:       # |Us|, |Ts|, |Ud|, |Td| <= 2, means in [-1, 1]: with degrees <= 1 the groups stay below 2^6 for any N < 2^15
            Us, Ts, Ud, Td = (np.trunc(x / 4) for x in (Us, Ts, Ud, Td))
        rstd = np.ones(H, f32)
        if family == "ints":
            ga, m = np.ones(H, f32), np.zeros((2, H), f32)
        else:
            ga, m = rng.choice([0.5, 1.0, 2.0, -4.0], H).astype(f32), rng.integers(-1 if small else -2, 2 if small else 3, (2, H)).astype(f32)
            Us, Ud = 2 * Us, 2 * Ud       # every term of the group even, so that gamma = 0.5 leaves an integer
            m[0] *= 2
            Ts, Td = 2 * Ts, 2 * Td
    else:
        Us, Ts, Ud, Td, h_in = (rng.standard_normal((N, H)).astype(f32) for _ in range(5))
        if family == "rows":
            s = np.exp(2.0 * rng.standard_normal((N, 1))).astype(f32)
            Us, Ud = Us * s, Ud * s
        rstd = np.exp(rng.uniform(-2, 2, H)).astype(f32)
        ga = (1 + 0.1 * rng.standard_normal(H)).astype(f32)
        m = (0.1 * rng.standard_normal((2, H))).astype(f32)
    stat = np.stack([np.zeros(H, f32), rstd, ga * rstd, np.zeros(H, f32)]).astype(f32)
    return _freeze(dict(UT=np.concatenate([Us, Ts], 1), Ud=Ud, Td=Td, stat_e=stat, bstat_e=m, gamma_e=ga, h_in=h_in))


def bgrad_groups_ref(d, in_ptr, out_ptr):
    """(gB1h | gB2h [N,2H], bound) of bn_reference.bgrad_ref: by source from UT and the out-degrees, by destination from Ud, Td."""
    deg_in, deg_out = (np.diff(np.asarray(p, np.int64))[:, None].astype(np.float64) for p in (in_ptr, out_ptr))
    b1, d1 = br.bgrad_ref(d["UT"][:, :H], d["UT"][:, H:], deg_out, d["stat_e"], d["bstat_e"], d["gamma_e"])
    b2, d2 = br.bgrad_ref(d["Ud"], d["Td"], deg_in, d["stat_e"], d["bstat_e"], d["gamma_e"])
    return np.concatenate([b1, b2], 1), np.concatenate([d1, d2], 1)
