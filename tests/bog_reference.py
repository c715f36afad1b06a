"""The yardstick of the best-overlap-contig tests: plain numpy and Python loops in the caller's node numbering and edge-id order.
It states the rules literally (include/gnm.h, "best-overlap contigs"):

  Links.    Edge k = (u -> v) is a link iff u != v, best_succ[u] == k, best_pred[v] == k, scores[k] is not NaN and
            scores[k] >= min_logit.  A table entry outside [-1, E) or a src / dst entry outside [0, n) drops that candidate.
            Then next[u] = v, prev[v] = u, pedge[v] = k; else -1.
  Cycles.   A component in which every node has a prev is a cycle.  It is cut at its smallest node id m: prev[m] = pedge[m] = -1
            and next[old prev of m] = -1.
  Ranking.  Every node now lies on exactly one path (a node with no link is a path of one).  head(v) is the path's first node,
            rank(v) the hops from it, off(v) the int64 sum of prefix_length[pedge[w]] over the path from the head (excluded) to v
            (included), wrong(v) the same sum over [y[pedge[w]] != 1] -- 0 everywhere without y.
  Contigs.  The heads in ascending node id are contigs 0 .. C-1: contig_ptr [C+1], walk_nodes[contig_ptr[c] + rank(v)] = v,
            walk_edges = pedge in the same layout, bases[c] = off(tail) + read_length[tail], wrong[c] = wrong(tail).
  Record.   contigs, links (kept, after the cuts), cycles_cut, dropped (mutual-best edges refused for NaN or min_logit),
            wrong_links, multi_nodes (nodes on paths of >= 2 nodes), multi_contigs, calls.

The tables come from tests/decision_reference.decisions.  Scores are compared as numpy float32 scalars.  Everything returned is
an integer, so the tests compare for equality."""
import numpy as np

import decision_reference as D

COUNTERS = ("contigs", "links", "cycles_cut", "dropped", "wrong_links", "multi_nodes", "multi_contigs", "calls")
WORDS = len(COUNTERS)


def links(src, dst, n, best_succ, best_pred, scores, min_logit=-np.inf):
    """(next, prev, pedge, dropped) before the cycles are cut."""
    src, dst = np.asarray(src).reshape(-1), np.asarray(dst).reshape(-1)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    ml = np.float32(min_logit)
    E = src.size
    nxt, prv, pedge = [-1] * n, [-1] * n, [-1] * n
    dropped = 0
    for k in range(E):
        u, v = int(src[k]), int(dst[k])
        if not (0 <= u < n and 0 <= v < n) or u == v:
            continue
        if int(best_succ[u]) != k or int(best_pred[v]) != k:
            continue
        if bool(np.isnan(sc[k])) or not bool(sc[k] >= ml):
            dropped += 1
            continue
        nxt[u], prv[v], pedge[v] = v, u, k
    return nxt, prv, pedge, dropped


def cut_cycles(nxt, prv, pedge):
    """Cuts every cycle at its smallest node, in place; returns the number of cycles."""
    n = len(nxt)
    seen = [False] * n
    cycles = 0
    for v in range(n):
        if seen[v]:
            continue
        comp, w = [], v
        while w != -1 and not seen[w]:          # backwards from v: to a head (a path), or round to v again (a cycle)
            seen[w] = True
            comp.append(w)
            w = prv[w]
        if w == v:                              # every node of the component has a prev
            m = min(comp)
            old = prv[m]
            prv[m] = pedge[m] = -1
            nxt[old] = -1
            cycles += 1
        else:                                   # a path: mark the nodes after v as well
            w = nxt[v]
            while w != -1 and not seen[w]:
                seen[w] = True
                w = nxt[w]
    return cycles


def contigs_from_tables(src, dst, n, best_succ, best_pred, scores, prefix_length, read_length, y=None, min_logit=-np.inf):
    """dict: contig_ptr [C+1], walk_nodes [n], walk_edges [n], bases [C], wrong [C], record [WORDS] (int64 arrays)."""
    pl = np.asarray(prefix_length, dtype=np.int64).reshape(-1)
    rl = np.asarray(read_length, dtype=np.int64).reshape(-1)
    lab = None if y is None else np.asarray(y, dtype=np.float32).reshape(-1)
    nxt, prv, pedge, dropped = links(src, dst, n, best_succ, best_pred, scores, min_logit)
    cycles = cut_cycles(nxt, prv, pedge)
    ptr, nodes, edges, bases, wrong = [0], [], [], [], []
    rec = dict.fromkeys(COUNTERS, 0)
    for h in range(n):                          # the heads in ascending node id
        if prv[h] != -1:
            continue
        v, off, bad, length = h, 0, 0, 0
        while True:
            nodes.append(v)
            edges.append(pedge[v])
            if v != h:
                off += int(pl[pedge[v]])
                bad += int(lab is not None and not bool(lab[pedge[v]] == 1))
            length += 1
            if nxt[v] == -1:
                break
            v = nxt[v]
        ptr.append(len(nodes))
        bases.append(off + int(rl[v]))
        wrong.append(bad)
        rec["contigs"] += 1
        rec["links"] += length - 1
        rec["wrong_links"] += bad
        if length >= 2:
            rec["multi_nodes"] += length
            rec["multi_contigs"] += 1
    assert len(nodes) == n and sorted(nodes) == list(range(n))
    rec["cycles_cut"], rec["dropped"], rec["calls"] = cycles, dropped, 1
    i64 = lambda a: np.asarray(a, dtype=np.int64)  # noqa: E731
    return dict(contig_ptr=i64(ptr), walk_nodes=i64(nodes), walk_edges=i64(edges), bases=i64(bases), wrong=i64(wrong),
                record=i64([rec[k] for k in COUNTERS]))


def contigs(src, dst, n, scores, prefix_length, read_length, y=None, min_logit=-np.inf):
    """The same from the scores alone: the tables are decision_reference.decisions'."""
    bs, bp, _ = D.decisions(src, dst, n, scores, y)
    return contigs_from_tables(src, dst, n, bs, bp, scores, prefix_length, read_length, y, min_logit)


def n50(lengths) -> int:
    """The largest L such that the lengths >= L sum to at least half of the total; 0 for no length."""
    a = sorted((int(x) for x in lengths), reverse=True)
    total, run = sum(a), 0
    for x in a:
        run += x
        if 2 * run >= total:
            return x
    return 0


def summary(results, min_nodes=20) -> tuple:
    """(contigs, n50_bases, longest_bases, wrong_link_fraction) of the validation graphs' results (History.assembly_valid): the
    first three over the pooled contigs of at least min_nodes nodes, the last from the summed records."""
    pooled = []
    rec = np.zeros(WORDS, np.int64)
    for r in results:
        pooled += [int(b) for b, m in zip(r["bases"], np.diff(r["contig_ptr"])) if m >= min_nodes]
        rec += r["record"]
    links_, wrong_ = int(rec[COUNTERS.index("links")]), int(rec[COUNTERS.index("wrong_links")])
    return (len(pooled), n50(pooled), max(pooled, default=0), wrong_ / links_ if links_ else float("nan"))
