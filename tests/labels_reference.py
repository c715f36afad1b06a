"""An independent restatement of the ground-truth labels (include/gnm.h, "ground-truth labels") in plain Python -- union-find over the
valid edges, a search from the root, a maximum for the top, a search back, dictionaries for the mirrors -- and the hand-made graphs
the CPU and GPU tests share.  It shares no code with the library."""
from collections import defaultdict, deque

import numpy as np

COUNTERS = ("edges", "valid", "wrong_strand", "self_loops", "gap", "backward", "components", "singletons", "backbone", "positives",
            "twin_missing")


def reference_labels(src, dst, n, start, end, strand, twin=None):
    """dict(y, valid, backbone, component, top, stats) for a graph in the caller's numbering."""
    src, dst = [int(v) for v in src], [int(v) for v in dst]
    start, end, strand = [int(v) for v in start], [int(v) for v in end], [int(v) for v in strand]
    E = len(src)
    st = dict.fromkeys(COUNTERS, 0)
    st["edges"] = E
    valid = np.zeros(E, bool)
    for k, (s, d) in enumerate(zip(src, dst)):
        if strand[s] != 1 or strand[d] != 1:
            st["wrong_strand"] += 1
        elif s == d:
            st["self_loops"] += 1
        elif start[d] >= end[s]:
            st["gap"] += 1
        elif start[d] < start[s]:
            st["backward"] += 1
        else:
            valid[k] = True
            st["valid"] += 1
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    succ, pred = defaultdict(list), defaultdict(list)
    for k in np.flatnonzero(valid):
        s, d = src[k], dst[k]
        succ[s].append(d)
        pred[d].append(s)
        parent[find(s)] = find(d)
    members = defaultdict(list)
    for v in range(n):
        if strand[v] == 1:
            members[find(v)].append(v)
    component, top = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    backbone = np.zeros(n, bool)

    def reach(first, nbrs):
        seen, todo = {first}, deque([first])
        while todo:
            v = todo.popleft()
            for w in nbrs[v]:
                if w not in seen:
                    seen.add(w)
                    todo.append(w)
        return seen
    for nodes in members.values():
        root = min(nodes, key=lambda v: (start[v], v))
        fwd = reach(root, succ)
        t = min(fwd, key=lambda v: (-end[v], v))
        bwd = reach(t, pred)
        for v in nodes:
            component[v], top[v] = root, t
        for v in fwd & bwd:
            backbone[v] = True
        st["components"] += 1
        st["singletons"] += len(nodes) == 1
    st["backbone"] = int(backbone.sum())
    ids = defaultdict(list)
    for k, (s, d) in enumerate(zip(src, dst)):
        ids[(s, d)].append(k)
    y = np.zeros(E, np.float32)
    for k in np.flatnonzero(valid):
        s, d = src[k], dst[k]
        if not (backbone[s] and backbone[d]):
            continue
        y[k] = 1.0
        # with twins an edge knows its mirror through its own entry alone, believed when it names the mirrored pair
        names = lambda j, a, b: 0 <= int(twin[j]) < E and (src[int(twin[j])], dst[int(twin[j])]) == (a, b)  # noqa: E731
        mirror = ids.get((d ^ 1, s ^ 1), [])
        if (not mirror) if twin is None else (not names(k, d ^ 1, s ^ 1)):
            st["twin_missing"] += 1
        for m in mirror:
            if twin is None or names(m, s, d):
                y[m] = 1.0
    st["positives"] = int(y.sum())
    return dict(y=y, valid=valid, backbone=backbone, component=component, top=top, stats=st)


# ---- hand-made graphs ------------------------------------------------------------------------------------------------------------
def build(reads, links, plus_odd=(), extra=(), mirrors=True):
    """A graph over the reads [(start, end)]: read r owns nodes 2r and 2r + 1, its + strand node is 2r (2r + 1 for r in plus_odd).
    links: (a, b) pairs of reads -> the + strand edge a -> b and, with `mirrors`, its mirror; extra: raw (src, dst) node pairs."""
    R = len(reads)
    P = lambda r: 2 * r + (1 if r in plus_odd else 0)  # noqa: E731
    start, end, strand = np.zeros(2 * R, np.int64), np.zeros(2 * R, np.int64), np.zeros(2 * R, np.int64)
    for r, (s, e) in enumerate(reads):
        start[2 * r:2 * r + 2], end[2 * r:2 * r + 2] = s, e
        strand[P(r)], strand[P(r) ^ 1] = 1, -1
    edges = []
    for a, b in links:
        edges.append((P(a), P(b)))
        if mirrors:
            edges.append((P(b) ^ 1, P(a) ^ 1))
    edges += list(extra)
    src = np.asarray([e[0] for e in edges], np.int32)
    dst = np.asarray([e[1] for e in edges], np.int32)
    return dict(src=src, dst=dst, n=2 * R, start=start, end=end, strand=strand)


def chain(m, step=10, length=25, reverse_ids=False):
    """m reads in a chain along the genome; reverse_ids: the ids run against the starts."""
    reads = [(i * step, i * step + length) for i in range(m)]
    if reverse_ids:
        reads = reads[::-1]
        return build(reads, [(i + 1, i) for i in range(m - 1)])
    return build(reads, [(i, i + 1) for i in range(m - 1)])


def permuted(case, seed):
    order = np.random.default_rng(seed).permutation(case["src"].size)
    return dict(case, src=case["src"][order].copy(), dst=case["dst"][order].copy())


def twins(case):
    """a twin array: for every edge the id of some copy of its mirror, -1 when there is none"""
    ids = {}
    for k, (s, d) in enumerate(zip(case["src"].tolist(), case["dst"].tolist())):
        ids.setdefault((s, d), k)
    return np.asarray([ids.get((d ^ 1, s ^ 1), -1) for s, d in zip(case["src"].tolist(), case["dst"].tolist())], np.int64)


A, B, C, D, T = 0, 1, 2, 3, 4
CASES = {
    "no_edges": lambda: build([(0, 10), (5, 15)], []),
    "one_read": lambda: build([(0, 10)], [], extra=[(0, 1), (1, 0)]),                     # n = 2: an edge between the two strands
    "one_link": lambda: build([(0, 10), (5, 15)], [(A, B)]),
    "two_cycle": lambda: build([(0, 10), (0, 12)], [(A, B), (B, A)]),
    "touching": lambda: build([(0, 10), (10, 20)], [(A, B)]),                             # start[d] == end[s]
    "invalid_kinds": lambda: build([(0, 10), (5, 15), (20, 30)], [(A, B), (A, C), (B, A)], extra=[(0, 3)]),
    "self_loop_and_duplicate": lambda: build([(0, 10), (5, 15)], [(A, B), (A, B), (A, A)]),
    "tip": lambda: build([(0, 10), (5, 15), (10, 20), (15, 25), (8, 14)], [(A, B), (B, C), (C, D), (B, T)]),
    "unreachable": lambda: build([(0, 10), (2, 12), (5, 15)], [(A, C), (B, C)]),
    "two_components": lambda: build([(0, 10), (5, 15), (100, 110), (105, 115)], [(A, B), (C, D), (B, C)]),
    "singleton": lambda: build([(0, 10), (5, 15), (50, 60)], [(A, B)]),
    "top_tie": lambda: build([(0, 10), (5, 20), (6, 20)], [(A, B), (A, C)]),
    "missing_mirror": lambda: build([(0, 10), (5, 15), (10, 20)], [(A, B)], extra=[(2, 4)]),
    "mixed_parity": lambda: build([(0, 12), (5, 15), (10, 20), (15, 25)], [(A, B), (B, C), (C, D), (A, C)], plus_odd=(B, D)),
    "permuted": lambda: permuted(build([(0, 10), (5, 15), (10, 20), (15, 25), (8, 14), (12, 19)],
                                       [(A, B), (B, C), (C, D), (B, T), (A, B), (T, 5), (5, D), (D, A)], plus_odd=(C,)), 7),
}


def genome_case(seed, drop_contained=True, reads_n=60, min_overlap=50):
    """The graph the positions of overlap_reference.genome_reads imply (true_overlaps), with its node arrays."""
    import overlap_reference as oref
    truth = oref.genome_reads(seed=seed, reads_n=reads_n)["truth"]
    _, edges = oref.true_overlaps(truth, min_overlap, drop_contained)
    n = 2 * len(truth)
    start, end, strand = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for r, (s, e, t) in enumerate(truth):
        start[2 * r:2 * r + 2], end[2 * r:2 * r + 2] = s, e
        strand[2 * r + t], strand[2 * r + (1 - t)] = 1, -1
    return dict(src=np.asarray([e[0] for e in edges], np.int32), dst=np.asarray([e[1] for e in edges], np.int32), n=n, start=start,
                end=end, strand=strand, truth=truth)


_CACHE = {}


def expected(name, case, twin=None):
    """reference_labels of a named case, computed once and shared"""
    key = (name, twin is not None)
    if key not in _CACHE:
        _CACHE[key] = reference_labels(case["src"], case["dst"], case["n"], case["start"], case["end"], case["strand"], twin)
    return _CACHE[key]
