"""The yardstick of the greedy-path-cover tests: plain numpy and Python loops in the caller's node numbering and edge-id order.
It states the rules literally (include/gnm.h, "cover rounds"):

  Candidates.  Edge k = (u -> w) with 0 <= u, w < n, u != w, scores[k] not NaN and scores[k] >= min_logit.  Duplicate edges are
               separate candidates.  Order: the larger score first (-0.0 == +0.0), the lowest edge id among equal scores
               (decision_reference.better).
  State.       msucc[u] / mpred[w]: the edge id of the accepted out-edge / in-edge, or -1.
  Round r, synchronously on the state after round r - 1:
    propose    u with msucc[u] < 0 takes cs[u], its best candidate out-edge whose destination w has mpred[w] < 0, or -1;
               w with mpred[w] < 0 takes cp[w], its best candidate in-edge whose source u has msucc[u] < 0, or -1.
    link       u sets msucc[u] = k when k = cs[u] >= 0 and cp[dst k] == k; w sets mpred[w] = k when k = cp[w] >= 0 and
               cs[src k] == k.  round_links[r] = the links the round added.
  rounds() stops after the first round that added nothing (a fixed point: the next round would see the same state) or after
  max_rounds.  greedy() is the sequential form: the candidates by descending score, lowest edge id among equals; an edge is
  accepted when its source has no successor yet and its destination no predecessor yet.  No union-find: cycles can close, and
  bog_reference cuts them.  Everything returned is an integer, so the tests compare for equality."""
import numpy as np

import bog_reference as B
import decision_reference as D


def candidates(src, dst, n, scores, min_logit=-np.inf):
    """The candidate edge ids, ascending."""
    src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    ml = np.float32(min_logit)
    out = []
    for k in range(src.size):
        u, w = int(src[k]), int(dst[k])
        if not (0 <= u < n and 0 <= w < n) or u == w:
            continue
        if bool(np.isnan(sc[k])) or not bool(sc[k] >= ml):
            continue
        out.append(k)
    return out


def _best(ks, sc):
    best = -1
    for k in ks:
        if best < 0 or D.better(sc[k], k, sc[best], best):
            best = k
    return best


def rounds(src, dst, n, scores, min_logit=-np.inf, max_rounds=None):
    """(msucc [n], mpred [n], round_links): the state after the rounds run, and the links each of them added."""
    src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    out_c, in_c = [[] for _ in range(n)], [[] for _ in range(n)]
    for k in candidates(src, dst, n, sc, min_logit):
        out_c[int(src[k])].append(k)
        in_c[int(dst[k])].append(k)
    msucc, mpred, round_links = [-1] * n, [-1] * n, []
    while max_rounds is None or len(round_links) < max_rounds:
        for u in range(n):                              # a taken slot stays taken: its edges are candidates no more (speed only)
            out_c[u] = [k for k in out_c[u] if mpred[int(dst[k])] < 0] if msucc[u] < 0 else []
            in_c[u] = [k for k in in_c[u] if msucc[int(src[k])] < 0] if mpred[u] < 0 else []
        cs = {u: _best(out_c[u], sc) for u in range(n) if msucc[u] < 0}
        cp = {w: _best(in_c[w], sc) for w in range(n) if mpred[w] < 0}
        new_s, new_p, added = list(msucc), list(mpred), 0
        for u, k in cs.items():
            if k >= 0 and cp.get(int(dst[k]), -1) == k:
                new_s[u] = k
                added += 1
        for w, k in cp.items():
            if k >= 0 and cs.get(int(src[k]), -1) == k:
                new_p[w] = k
        msucc, mpred = new_s, new_p
        round_links.append(added)
        if added == 0:
            break
    return np.asarray(msucc, np.int64), np.asarray(mpred, np.int64), round_links


def greedy(src, dst, n, scores, min_logit=-np.inf):
    """(msucc [n], mpred [n]) of the sequential sorted pass."""
    src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    order = sorted(candidates(src, dst, n, sc, min_logit), key=lambda k: (-float(sc[k]), k))   # -0.0 == 0.0: the edge id decides
    msucc, mpred = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for k in order:
        u, w = int(src[k]), int(dst[k])
        if msucc[u] < 0 and mpred[w] < 0:
            msucc[u], mpred[w] = k, k
    return msucc, mpred


def is_maximal(src, dst, n, scores, msucc, mpred, min_logit=-np.inf) -> bool:
    """No candidate edge has a free source slot and a free destination slot."""
    return not any(msucc[int(src[k])] < 0 and mpred[int(dst[k])] < 0 for k in candidates(src, dst, n, scores, min_logit))


def next_prev(src, dst, msucc, mpred):
    """The tables as node ids: next[u] = dst[msucc[u]], prev[w] = src[mpred[w]], -1 where the slot is free."""
    src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
    return ([int(dst[k]) if k >= 0 else -1 for k in msucc], [int(src[k]) if k >= 0 else -1 for k in mpred])


def contigs(src, dst, n, scores, prefix_length, read_length, y=None, min_logit=-np.inf, max_rounds=None):
    """bog_reference's result dict on the cover's tables, plus rounds / round_links / converged."""
    msucc, mpred, rl = rounds(src, dst, n, scores, min_logit, max_rounds)
    r = B.contigs_from_tables(src, dst, n, msucc, mpred, scores, prefix_length, read_length, y, min_logit)
    r.update(link_succ=msucc, link_pred=mpred, rounds=len(rl), round_links=rl, converged=bool(rl) and rl[-1] == 0)
    return r


# ---- the graphs both test files use ------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")


def lengths(rng, E, n):
    return rng.integers(1, 12000, E).astype(np.int64), rng.integers(1000, 25000, n).astype(np.int64)


def mix(seed, path_lens, cycle_lens, distractors, special_every=25, dprobs=(.3, .1, .1, .1, .15, .2, .05)):
    """The recipe of test_gpu_bog._mix: paths and cycles over randomly permuted node ids (main edges at scores 1, 2, 4 with a few
    specials among them), plus `distractors` random edges -- self loops and duplicates of main edges among them -- scored -1, +-0,
    -inf, NaN, 1 (ties) and 5 (wins), `dprobs` in that order; one main edge in `special_every` is NaN, -inf, +-0 or 0.5.  Edge ids
    are shuffled; labels are 0, 1, 0.5 and NaN.  Returns (src, dst, n, scores, y, prefix_length, read_length)."""
    rng = np.random.default_rng(seed)
    n = int(sum(path_lens) + sum(cycle_lens))
    ids = rng.permutation(n).astype(np.int32)
    src, dst, at = [], [], 0
    for m in path_lens:
        src += ids[at:at + m - 1].tolist()
        dst += ids[at + 1:at + m].tolist()
        at += m
    for m in cycle_lens:
        src += ids[at:at + m].tolist()
        dst += np.roll(ids[at:at + m], -1).tolist()
        at += m
    main = len(src)
    sc = np.array([1.0, 2.0, 4.0], np.float32)[rng.integers(0, 3, main)]
    sp = rng.permutation(main)[:main // special_every]
    sc[sp] = np.array([NAN, -INF, 0.0, -0.0, 0.5], np.float32)[rng.integers(0, 5, sp.size)]
    ds, dd = rng.integers(0, n, distractors), rng.integers(0, n, distractors)
    dup = rng.permutation(distractors)[:distractors // 10]
    pick = rng.integers(0, main, dup.size)
    ds[dup], dd[dup] = np.array(src)[pick], np.array(dst)[pick]
    loops = rng.permutation(distractors)[:distractors // 20]
    dd[loops] = ds[loops]
    dsc = np.array([-1.0, 0.0, -0.0, -INF, NAN, 1.0, 5.0], np.float32)[rng.choice(7, distractors, p=list(dprobs))]
    src, dst, sc = np.concatenate([src, ds]).astype(np.int32), np.concatenate([dst, dd]).astype(np.int32), np.concatenate([sc, dsc])
    p = rng.permutation(src.size)
    src, dst, sc = src[p], dst[p], sc[p]
    y = np.array([0.0, 1.0, 0.5, NAN], np.float32)[rng.choice(4, src.size, p=[0.3, 0.5, 0.1, 0.1])]
    pl, rl = lengths(rng, src.size, n)
    return src, dst, n, sc, y, pl, rl


def adversarial_chain(m=50, seed=7):
    """u_i -> v_i scored 2 (m - i), u_i -> v_{i+1} scored 2 (m - i) - 1, i < m: v_{i+1} prefers u_i until u_i is taken, so round r
    links u_{r-1} -> v_{r-1} alone and round m + 1 is the first empty one.  u_i = node i, v_i = node m + i; edge ids shuffled."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([np.arange(m), np.arange(m)]).astype(np.int32)
    dst = np.concatenate([m + np.arange(m), m + 1 + np.arange(m)]).astype(np.int32)
    sc = np.concatenate([2.0 * (m - np.arange(m)), 2.0 * (m - np.arange(m)) - 1.0]).astype(np.float32)
    p = rng.permutation(2 * m)
    n = 2 * m + 1
    pl, rl = lengths(rng, 2 * m, n)
    return src[p], dst[p], n, sc[p], np.ones(2 * m, np.float32), pl, rl
