"""The oracle of the ranking-metric tests: numpy only, nothing imported from the library.

key_of / hist_of restate the record of gnm_rank_hist (include/gnm.h) element by element; metrics_of restates what
train.RankingMetrics.from_counts derives from a record, with plain loops over the occupied bins; auroc_exact / ap_exact are the
O(P * N) definitions on the raw logits."""
import math

import numpy as np

BINS = 16384


def key_of(x) -> np.ndarray:
    """The 14-bit key of fp32 values that are not NaN: x + 0.0f (so -0 becomes +0), the order-preserving map of the bits, >> 18."""
    x = np.asarray(x, dtype=np.float32) + np.float32(0.0)
    u = x.view(np.uint32).astype(np.uint64)
    u = np.where(u >> 31 != 0, u ^ 0xFFFFFFFF, u ^ 0x80000000)
    return (u >> 18).astype(np.int64)


def lower_edge(k: int) -> float:
    """The smallest fp32 value with key k, found from the definition: the value of the bin's extreme bit pattern."""
    u = int(k) << 18
    bits = (u ^ 0x80000000) if u >> 31 else ((~u) & 0xFFFFFFFF)
    v = float(np.array([bits], np.uint32).view(np.float32)[0])
    if math.isnan(v):
        return math.inf if u >> 31 else -math.inf
    return v


def _sigmoid(x: float) -> float:
    with np.errstate(over="ignore"):
        return float(1.0 / (1.0 + np.exp(np.float64(-x))))


def hist_of(scores, y):
    """(hist int64 [2, BINS], tail int64 [4] = nan_pos, nan_neg, other_label, calls = 1), one element at a time."""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    y = np.asarray(y, dtype=np.float32).reshape(-1)
    hist = np.zeros((2, BINS), np.int64)
    tail = np.zeros(4, np.int64)
    tail[3] = 1
    lab = np.where(y == 1, 1, np.where(y == 0, 0, -1))
    tail[2] = int((lab < 0).sum())
    nan = np.isnan(scores)
    tail[0] = int((nan & (lab == 1)).sum())
    tail[1] = int((nan & (lab == 0)).sum())
    ok = (lab >= 0) & ~nan
    np.add.at(hist, (lab[ok], key_of(scores[ok])), 1)
    return hist, tail


def record_of(scores, y) -> np.ndarray:
    """hist_of as the flat int64 [2 * BINS + 4] record."""
    h, t = hist_of(scores, y)
    return np.concatenate([h.reshape(-1), t])


def metrics_of(hist, tail=None) -> dict:
    """The fields of RankingMetrics from a record, by loops over the occupied bins in Python integers and fp64."""
    hist = np.asarray(hist, np.int64).reshape(2, BINS)
    tail = np.zeros(4, np.int64) if tail is None else np.asarray(tail, np.int64)
    P, N = int(hist[1].sum()), int(hist[0].sum())
    occ = [int(k) for k in np.flatnonzero(hist[0] + hist[1])]
    nan = float("nan")
    out = dict(n_pos=P, n_neg=N, n_nan=int(tail[0] + tail[1]), n_other=int(tail[2]), calls=int(tail[3]),
               auroc=nan, auroc_lo=nan, auroc_hi=nan, average_precision=nan, best_f1=None)
    if P and N:
        lo = tie = 0
        above = 0
        for k in reversed(occ):
            lo += int(hist[0][k]) * above
            tie += int(hist[0][k]) * int(hist[1][k])
            above += int(hist[1][k])
        out.update(auroc=(lo + 0.5 * tie) / (float(P) * N), auroc_lo=lo / (float(P) * N), auroc_hi=(lo + tie) / (float(P) * N))
        ap, tp, fp = 0.0, 0, 0
        terms = []
        for k in reversed(occ):
            tp += int(hist[1][k]); fp += int(hist[0][k])                     # noqa: E702
            terms.append(float(hist[1][k]) / P * (float(tp) / float(tp + fp)))
        out["average_precision"] = float(np.sum(np.array(terms)))
    if occ:
        best, tp, fp = None, 0, 0
        for k in reversed(occ):
            tp += int(hist[1][k]); fp += int(hist[0][k])                     # noqa: E702
            den = 2 * tp + fp + (P - tp)
            f1 = 2.0 * tp / den if den else 0.0
            if best is None or f1 > best["f1"]:
                edge = lower_edge(k)
                best = dict(f1=f1, logit=edge, prob=_sigmoid(edge), bin=k,
                            TP=tp, TN=N - fp, FP=fp, FN=P - tp)
        out["best_f1"] = best
    return out


def auroc_exact(scores, y) -> float:
    """Mann-Whitney over all (positive, negative) pairs of the raw logits, ties 1/2.  NaN logits and other labels left out."""
    s = np.asarray(scores, np.float64).reshape(-1)
    y = np.asarray(y).reshape(-1)
    ok = ~np.isnan(s)
    p, n = s[ok & (y == 1)], s[ok & (y == 0)]
    if p.size == 0 or n.size == 0:
        return float("nan")
    with np.errstate(invalid="ignore"):                  # inf against inf: a tie
        gt = (p[:, None] > n[None, :]).sum()
        eq = (p[:, None] == n[None, :]).sum()
    return (float(gt) + 0.5 * float(eq)) / (float(p.size) * float(n.size))


def ap_exact(scores, y) -> float:
    """Average precision by definition: for every distinct logit value v from the top, the recall gained at the threshold
    "score >= v" times the precision there, each found by counting over all edges."""
    s = np.asarray(scores, np.float64).reshape(-1)
    y = np.asarray(y).reshape(-1)
    ok = ~np.isnan(s) & ((y == 1) | (y == 0))
    s, y = s[ok], y[ok]
    P = int((y == 1).sum())
    if P == 0 or P == y.size:
        return float("nan")
    terms, prev = [], 0
    for v in sorted(set(s.tolist()), reverse=True):
        sel = s >= v
        tp = int((sel & (y == 1)).sum())
        terms.append(float(tp - prev) / P * (float(tp) / float(sel.sum())))
        prev = tp
    return float(np.sum(np.array(terms)))


def best_f1_exhaustive(scores, y):
    """(max F1, the largest OCCUPIED bin attaining it) over every one of the BINS thresholds "key >= t", counted on the edges."""
    s = np.asarray(scores, np.float32).reshape(-1)
    y = np.asarray(y).reshape(-1)
    ok = ~np.isnan(s) & ((y == 1) | (y == 0))
    k, y = key_of(s[ok]), y[ok]
    P = int((y == 1).sum())
    sel = k[None, :] >= np.arange(BINS)[:, None]
    tp = (sel & (y == 1)[None, :]).sum(axis=1)
    fp = sel.sum(axis=1) - tp
    den = 2 * tp + fp + (P - tp)
    f1 = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    best = float(f1.max())
    occupied = np.zeros(BINS, bool)
    occupied[k] = True
    hits = np.flatnonzero((f1 == best) & occupied)
    return best, (int(hits[-1]) if hits.size else None)
