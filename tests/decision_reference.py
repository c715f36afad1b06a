"""The yardstick of the walk-decision tests: plain numpy and Python loops over (src, dst, scores, y) in the caller's node
numbering and edge-id order.  It states the rules literally:

  * the successor candidates of node v are the edges with src == v, the predecessor candidates those with dst == v;
  * a self loop is no candidate; duplicate edges are separate candidates;
  * the choice is the candidate with the largest score; equal scores (-0.0 == +0.0) go to the lowest edge id;
  * a NaN orders below every number, -inf included; among NaNs the lowest edge id wins;
  * a label counts as correct only when it == 1 (0.5 and NaN do not).

Scores are compared as numpy float32 scalars (IEEE comparison: denormals are numbers of their own, nothing is flushed).
Everything it returns is an integer, so the tests compare for equality."""
import numpy as np

COUNTERS = ("dead", "forced", "forced_ok", "branch", "branch_solvable", "branch_ok", "branch_nan")
WORDS = 2 * len(COUNTERS) + 1            # succ counters, pred counters, calls


def better(sa, ea, sb, eb) -> bool:
    """True when candidate a = (score, edge id) beats candidate b."""
    na, nb = bool(np.isnan(sa)), bool(np.isnan(sb))
    if na != nb:
        return nb                        # a number beats a NaN
    if not na and sa != sb:
        return bool(sa > sb)
    return ea < eb                       # equal scores, or two NaNs: the lowest edge id


def decisions(src, dst, n, scores, y=None):
    """(best_succ [n], best_pred [n], record [WORDS]) as int64 arrays; record = succ counters, pred counters, calls = 1."""
    src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    lab = None if y is None else np.asarray(y, dtype=np.float32).reshape(-1)
    assert src.size == dst.size == sc.size and (lab is None or lab.size == sc.size)
    cand = [[[] for _ in range(n)], [[] for _ in range(n)]]
    for k in range(src.size):
        s, d = int(src[k]), int(dst[k])
        if s == d:
            continue
        cand[0][s].append(k)
        cand[1][d].append(k)
    tables = np.full((2, n), -1, np.int64)
    rec = np.zeros(WORDS, np.int64)
    for side in (0, 1):
        c = dict.fromkeys(COUNTERS, 0)
        for v in range(n):
            ks = cand[side][v]
            if not ks:
                c["dead"] += 1
                continue
            best = ks[0]
            for k in ks[1:]:
                if better(sc[k], k, sc[best], best):
                    best = k
            tables[side, v] = best
            ok = lab is not None and bool(lab[best] == 1)
            if len(ks) == 1:
                c["forced"] += 1
                c["forced_ok"] += int(ok)
            else:
                c["branch"] += 1
                c["branch_solvable"] += int(lab is not None and any(bool(lab[k] == 1) for k in ks))
                c["branch_ok"] += int(ok)
                c["branch_nan"] += int(bool(np.isnan(sc[best])))
        rec[side * len(COUNTERS):(side + 1) * len(COUNTERS)] = [c[k] for k in COUNTERS]
    rec[-1] = 1
    return tables[0], tables[1], rec


def ratio(num, den) -> float:
    return float(num) / float(den) if den else float("nan")


def summary(rec) -> tuple:
    """(pooled branch accuracy, pooled solvable accuracy, succ branch accuracy, pred branch accuracy) of a record."""
    k = len(COUNTERS)
    s, p = dict(zip(COUNTERS, (int(v) for v in rec[:k]))), dict(zip(COUNTERS, (int(v) for v in rec[k:2 * k])))
    return (ratio(s["branch_ok"] + p["branch_ok"], s["branch"] + p["branch"]),
            ratio(s["branch_ok"] + p["branch_ok"], s["branch_solvable"] + p["branch_solvable"]),
            ratio(s["branch_ok"], s["branch"]), ratio(p["branch_ok"], p["branch"]))
