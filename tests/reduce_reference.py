"""The yardstick of the transitive-reduction tests: plain numpy and Python loops in the caller's node numbering and edge-id order.
It states the rules literally (include/gnm.h, "transitive support"):

  Candidate.  Edge k = (u -> w) with u != w, scores[k] not NaN and scores[k] >= min_logit: cover_reference.candidates.
  Support.    For every edge k = (a -> c) with a != c, candidate or not: support[k] = the number of out-edges j = (a -> b) of a
              with j a candidate, b != a, b != c, prefix_length[j] < prefix_length[k] STRICTLY, and at least one candidate
              m = (b -> c) -- with fuzz >= 0 one that also has |prefix_length[j] + prefix_length[m] - prefix_length[k]| <= fuzz,
              the sum taken in int64 (wrapping).  fuzz None or -1: no length test.  Parallel a -> b edges each count, several
              parallel b -> c edges make one witness, a self loop has support 0.
  Reduced.    k is a candidate and support[k] > 0.  masked_scores[k] = the quiet NaN 0x7FC00000 where k is reduced, else the bits
              of scores[k].
  Record.     edges, candidates, reduced, reduced_label1 (reduced and y == 1; 0 without y), witnesses (the sum of support),
              max_support, self_loops, calls -- calls = 1, except for a graph without a node or an edge, which launches nothing
              and leaves the record at 0.

cover() is the composition the decoders run with reduce_transitive=True: the reduction, then cover_reference.contigs (or
bog_reference.contigs) on the masked scores.  Everything returned is an integer or a bit pattern, so the tests compare for equality."""
import numpy as np

import bog_reference as B
import cover_reference as R

COUNTERS = ("edges", "candidates", "reduced", "reduced_label1", "witnesses", "max_support", "self_loops", "calls")
NAN, INF = float("nan"), float("inf")
QNAN = np.uint32(0x7FC00000)


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def reduce(src, dst, n, scores, prefix_length, y=None, min_logit=-np.inf, fuzz=None):
    """dict: support [E] int64, reduced [E] bool, masked_bits [E] uint32, record [8] int64, witnesses (list per edge of the edge
    ids j that count), candidate [E] bool."""
    src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    pl = [int(v) for v in np.asarray(prefix_length, dtype=np.int64).reshape(-1)]
    lab = None if y is None else np.asarray(y, dtype=np.float32).reshape(-1)
    E = src.size
    fz = -1 if fuzz is None else int(fuzz)
    assert fz >= -1 and len(pl) == E and sc.size == E
    cand = np.zeros(E, bool)
    cand[R.candidates(src, dst, n, sc, min_logit)] = True
    outs = [[] for _ in range(n)]
    closing = {}                                        # (b, c) -> the candidate edges b -> c
    for k in range(E):
        outs[int(src[k])].append(k)
        if cand[k]:
            closing.setdefault((int(src[k]), int(dst[k])), []).append(k)
    support, wit = np.zeros(E, np.int64), [[] for _ in range(E)]
    for k in range(E):
        a, c = int(src[k]), int(dst[k])
        if a == c:
            continue
        for j in outs[a]:
            b = int(dst[j])
            if not cand[j] or b == a or b == c or not pl[j] < pl[k]:
                continue
            ms = closing.get((b, c), [])
            if fz >= 0:
                ms = [m for m in ms if -fz <= _wrap64(pl[j] + pl[m] - pl[k]) <= fz]
            if ms:
                wit[k].append(j)
        support[k] = len(wit[k])
    reduced = cand & (support > 0)
    bits = sc.view(np.uint32).copy()
    bits[reduced] = QNAN
    loops = int((src == dst).sum())
    label1 = 0 if lab is None else int((reduced & (lab == 1)).sum())
    rec = [E, int(cand.sum()), int(reduced.sum()), label1, int(support.sum()), int(support.max(initial=0)), loops, 1]
    if n == 0 or E == 0:
        rec = [0] * 8
    return dict(support=support, reduced=reduced, masked_bits=bits, record=np.asarray(rec, np.int64), witnesses=wit, candidate=cand)


def masked(r) -> np.ndarray:
    """The masked scores of a reduce() result as fp32."""
    return r["masked_bits"].view(np.float32)


def cover(src, dst, n, scores, prefix_length, read_length, y=None, min_logit=-np.inf, fuzz=None, max_rounds=None, best_overlap=False):
    """The composed restatement: cover_reference.contigs (best_overlap: bog_reference.contigs) on the masked scores of reduce();
    the result dict additionally holds reduce_record."""
    r = reduce(src, dst, n, scores, prefix_length, y, min_logit, fuzz)
    if best_overlap:
        out = B.contigs(src, dst, n, masked(r), prefix_length, read_length, y, min_logit)
    else:
        out = R.contigs(src, dst, n, masked(r), prefix_length, read_length, y, min_logit, max_rounds)
    out["reduce_record"] = r["record"]
    return out


# ---- the properties the strict < gives ---------------------------------------------------------------------------------------------
def no_mutual_removal(r) -> bool:
    """No two edges count each other as a witness."""
    return not any(k in r["witnesses"][j] for k in range(len(r["witnesses"])) for j in r["witnesses"][k])


def shortest_out_edge_survives(src, prefix_length, r) -> bool:
    """Per node: when one candidate out-edge has a prefix strictly below every other candidate out-edge's, it is not reduced."""
    src = np.asarray(src).reshape(-1)
    pl = np.asarray(prefix_length, dtype=np.int64).reshape(-1)
    for a in np.unique(src):
        ks = [int(k) for k in np.flatnonzero((src == a) & r["candidate"])]
        if not ks:
            continue
        low = min(int(pl[k]) for k in ks)
        first = [k for k in ks if int(pl[k]) == low]
        if len(first) == 1 and r["reduced"][first[0]]:
            return False
    return True


# ---- the cases written out by hand: (name, src, dst, n, scores, prefix_length, min_logit, fuzz, support, reduced) ----------------------
_TRI = ([0, 1, 0], [1, 2, 2], 3)                        # e0 0 -> 1, e1 1 -> 2, e2 0 -> 2
_PAIR = ([0, 0, 1, 2], [1, 2, 2, 1], 3)                 # e0 0 -> 1, e1 0 -> 2, e2 1 -> 2, e3 2 -> 1
_PAR = ([0, 0, 1, 1, 0, 0], [1, 1, 2, 2, 2, 2], 3)      # two 0 -> 1, two 1 -> 2, two 0 -> 2
_LOOPS = ([0, 0, 1, 0, 1, 2], [0, 1, 2, 2, 1, 2], 3)    # e0 0 -> 0, the triangle e1 e2 e3, e4 1 -> 1, e5 2 -> 2
HAND = [
    ("triangle", *_TRI, [1, 1, 1], [10, 10, 20], -INF, None, [0, 0, 1], [0, 0, 1]),
    # 0 -> 2 falls through 0 -> 1 -> 2; 0 -> 1 would fall through 0 -> 2 -> 1, but its prefix is the shorter one
    ("mutual pair", *_PAIR, [1, 1, 1, 1], [10, 15, 5, 5], -INF, None, [0, 1, 0, 0], [0, 1, 0, 0]),
    ("mutual pair, the other way", *_PAIR, [1, 1, 1, 1], [15, 10, 5, 5], -INF, None, [1, 0, 0, 0], [1, 0, 0, 0]),
    ("equal prefixes", *_PAIR, [1, 1, 1, 1], [10, 10, 5, 5], -INF, None, [0, 0, 0, 0], [0, 0, 0, 0]),
    ("NaN first step", *_TRI, [NAN, 1, 1], [10, 10, 20], -INF, None, [0, 0, 0], [0, 0, 0]),
    ("NaN second step", *_TRI, [1, NAN, 1], [10, 10, 20], -INF, None, [0, 0, 0], [0, 0, 0]),
    # an edge that is no candidate still has its support, and is not reduced
    ("NaN long edge", *_TRI, [1, 1, NAN], [10, 10, 20], -INF, None, [0, 0, 1], [0, 0, 0]),
    ("first step below min_logit", *_TRI, [0.1, 1, 1], [10, 10, 20], 0.5, None, [0, 0, 0], [0, 0, 0]),
    ("second step below min_logit", *_TRI, [1, 0.1, 1], [10, 10, 20], 0.5, None, [0, 0, 0], [0, 0, 0]),
    ("long edge below min_logit", *_TRI, [1, 1, 0.1], [10, 10, 20], 0.5, None, [0, 0, 1], [0, 0, 0]),
    ("-inf is a candidate without a cut", *_TRI, [-INF, -INF, -INF], [10, 10, 20], -INF, None, [0, 0, 1], [0, 0, 1]),
    # 10 + 10 - 23 = -3
    ("inconsistent, fuzz 0", *_TRI, [1, 1, 1], [10, 10, 23], -INF, 0, [0, 0, 0], [0, 0, 0]),
    ("inconsistent, fuzz 2", *_TRI, [1, 1, 1], [10, 10, 23], -INF, 2, [0, 0, 0], [0, 0, 0]),
    ("inconsistent, fuzz 3", *_TRI, [1, 1, 1], [10, 10, 23], -INF, 3, [0, 0, 1], [0, 0, 1]),
    ("inconsistent, fuzz 5", *_TRI, [1, 1, 1], [10, 10, 23], -INF, 5, [0, 0, 1], [0, 0, 1]),
    ("inconsistent, no fuzz", *_TRI, [1, 1, 1], [10, 10, 23], -INF, None, [0, 0, 1], [0, 0, 1]),
    ("consistent, fuzz 0", *_TRI, [1, 1, 1], [10, 13, 23], -INF, 0, [0, 0, 1], [0, 0, 1]),
    # 10 + 13 - 20 = +3: the tolerance is two-sided
    ("too long, fuzz 2", *_TRI, [1, 1, 1], [10, 13, 20], -INF, 2, [0, 0, 0], [0, 0, 0]),
    # e0, e1: 0 -> 1 at 10, 12; e2, e3: 1 -> 2 at 10, 8; e4, e5: 0 -> 2 at 20, 11
    ("parallel edges", *_PAR, [1] * 6, [10, 12, 10, 8, 20, 11], -INF, None, [0, 0, 0, 0, 2, 1], [0, 0, 0, 0, 1, 1]),
    # e4: 10 + 10 and 12 + 8; e5: 10 + 10 and 10 + 8 both miss 11
    ("parallel edges, fuzz 0", *_PAR, [1] * 6, [10, 12, 10, 8, 20, 11], -INF, 0, [0, 0, 0, 0, 2, 0], [0, 0, 0, 0, 1, 0]),
    ("parallel edges, one second step NaN", *_PAR, [1, 1, 1, NAN, 1, 1], [10, 12, 10, 8, 20, 11], -INF, 0, [0, 0, 0, 0, 1, 0],
     [0, 0, 0, 0, 1, 0]),
    ("self loops", *_LOOPS, [9, 1, 1, 1, 9, 9], [1, 10, 10, 20, 1, 1], -INF, None, [0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0]),
    # 2^40 + 2^40 - 2^41 = 0, and a negative prefix is below a positive one
    ("prefixes at 2^40", *_TRI, [1, 1, 1], [2 ** 40, 2 ** 40, 2 ** 41], -INF, 0, [0, 0, 1], [0, 0, 1]),
    ("prefixes at 2^40, off by one", *_TRI, [1, 1, 1], [2 ** 40, 2 ** 40 + 1, 2 ** 41], -INF, 0, [0, 0, 0], [0, 0, 0]),
    # the low 32 bits of the first step's prefix are 3 < 7; the prefix is not
    ("a prefix whose low word is small", *_TRI, [1, 1, 1], [2 ** 40 + 3, 5, 7], -INF, None, [0, 0, 0], [0, 0, 0]),
    ("negative prefixes", *_TRI, [1, 1, 1], [-30, 10, -20], -INF, 0, [0, 0, 1], [0, 0, 1]),
    # -2^63 + -2^63 - 0 = -2^64 wraps to 0: the sum is int64 arithmetic on both sides
    ("the sum wraps", *_TRI, [1, 1, 1], [-2 ** 63, -2 ** 63, 0], -INF, 0, [0, 0, 1], [0, 0, 1]),
    ("negative prefixes, not below", *_TRI, [1, 1, 1], [-20, 10, -30], -INF, None, [0, 0, 0], [0, 0, 0]),
]


def hand_case(row):
    name, src, dst, n, sc, pl, ml, fuzz, support, reduced = row
    return (np.asarray(src, np.int32), np.asarray(dst, np.int32), n, np.asarray(sc, np.float32), np.asarray(pl, np.int64), ml, fuzz,
            np.asarray(support, np.int64), np.asarray(reduced, bool))


# ---- the graphs both test files use ------------------------------------------------------------------------------------------------
def chain(reads: int, seed: int = 0, reach: int = 3):
    """Reads with strictly increasing starts and ends, every read overlapping exactly its next `reach` (clipped at the end): edges
    2i -> 2j with prefix start[j] - start[i] and their strand mirrors 2j+1 -> 2i+1 with prefix end[j] - end[i]; no long-range
    edges; edge ids shuffled; random scores.  Every triangle is exact, so fuzz = 0 reduces all but the nearest-neighbour edges.
    Returns (src, dst, n, scores, prefix_length, read_length, nearest [E] bool)."""
    rng = np.random.default_rng(seed)
    start = np.cumsum(rng.integers(500, 3000, reads)).astype(np.int64)
    end = start + 20000 + np.cumsum(rng.integers(1, 50, reads))       # strictly increasing; every read reaches past the next `reach`
    src, dst, pl, near = [], [], [], []
    for i in range(reads):
        for j in range(i + 1, min(i + reach, reads - 1) + 1):
            src += [2 * i, 2 * j + 1]
            dst += [2 * j, 2 * i + 1]
            pl += [int(start[j] - start[i]), int(end[j] - end[i])]
            near += [j == i + 1] * 2
    p = rng.permutation(len(src))
    a = lambda v, dt: np.asarray(v, dt)[p]              # noqa: E731
    rl = np.repeat(end - start, 2).astype(np.int64)
    return (a(src, np.int32), a(dst, np.int32), 2 * reads, rng.standard_normal(len(src)).astype(np.float32), a(pl, np.int64), rl,
            a(near, bool))


def synth_prefixes(src, dst, n, seed: int = 0, jitter: int = 0):
    """Length-consistent prefixes for a synth.make_graph graph: read i starts at a random increasing position; a forward edge
    2i -> 2j has prefix |start[j] - start[i]|, its mirror the same, plus up to `jitter` bases of noise.  Returns (prefix_length [E],
    read_length [n]) int64."""
    rng = np.random.default_rng(seed + 77)
    start = np.cumsum(rng.integers(500, 3000, (n + 1) // 2)).astype(np.int64)
    src, dst = np.asarray(src).astype(np.int64), np.asarray(dst).astype(np.int64)
    pl = np.abs(start[dst >> 1] - start[src >> 1])
    if jitter:
        pl = pl + rng.integers(0, jitter + 1, pl.size)
    return pl.astype(np.int64), np.repeat(rng.integers(15000, 25000, (n + 1) // 2), 2)[:n].astype(np.int64)
