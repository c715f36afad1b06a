#!/usr/bin/env python3
"""Golden vectors for the ground-truth labels, produced by the REFERENCE's own algorithms.get_gt_graph (graph_parser.py:307-309) on
graphs that simulated read positions imply (tests/overlap_reference.py: genome_reads, true_overlaps).  The reference module imports
dgl, which is absent here: tests/golden/dgl_standin stands in for the import; nothing of the reference's text is written out.
Neighbour and edge dictionaries are built as graph_parser.get_neighbors / get_edges do.  Run where the reference is checked out:
    python tests/golden/make_golden_labels.py <reference directory>
The generator asserts the preconditions under which the library's definition must CONTAIN the reference's labels and takes the
first seeds for which they hold: the reference's fallback through a non-overlapping successor never fires (every consecutive pair of
every walk has start[next] <= end[cur]), no such pair has start[next] == end[cur] (the library's test is strict), and the graph has
at least 50 positive edges.  It also prints the share of the library's positives the reference has as well."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(HERE, "dgl_standin")]
import labels_reference as lref  # noqa: E402


class Graph:      # the surface get_gt_graph and dfs read
    def __init__(self, case):
        self.n = case["n"]
        self.ndata = {"read_start": torch.from_numpy(case["start"]), "read_end": torch.from_numpy(case["end"]),
                      "read_strand": torch.from_numpy(case["strand"])}

    def num_nodes(self):
        return self.n


def reference_positives(alg, case):
    """(sorted positive edge ids, walks) of algorithms.get_gt_graph"""
    neighbors, edges = {}, {}
    for k, (s, d) in enumerate(zip(case["src"].tolist(), case["dst"].tolist())):
        neighbors.setdefault(s, []).append(d)
        edges[(s, d)] = k
    walks, dfs = [], alg.dfs

    def recording(*a, **kw):
        walk, visited = dfs(*a, **kw)
        walks.append(walk)
        return walk, visited
    alg.dfs = recording
    try:
        pos, neg = alg.get_gt_graph(Graph(case), neighbors, edges)
    finally:
        alg.dfs = dfs
    return np.asarray(sorted(pos | neg), np.int64), walks


def preconditions(case, positives, walks):
    start, end = case["start"], case["end"]
    for walk in walks:
        for cur, nxt in zip(walk[:-1], walk[1:]):
            if not start[nxt] < end[cur]:          # > : the fallback fired; == : kept by the reference, a gap for the library
                return False
    return positives.size >= 50


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import algorithms as alg
    out, seed, shares = {}, 21, []
    while len(shares) < 3:
        case = lref.genome_case(seed, drop_contained=len(shares) != 2)      # the third graph keeps its contained reads
        pos, walks = reference_positives(alg, case)
        if preconditions(case, pos, walks):
            i = len(shares)
            for k in ("src", "dst", "start", "end", "strand"):
                out[f"{k}_{i}"] = case[k]
            out[f"positive_{i}"], out[f"seed_{i}"] = pos, seed
            ours = lref.reference_labels(case["src"], case["dst"], case["n"], case["start"], case["end"], case["strand"])["y"]
            shares.append(float(ours[pos].sum()) / max(float(ours.sum()), 1.0))
            print(f"graph {i}: seed {seed}, E = {case['src'].size}, reference positives {pos.size}, ours {int(ours.sum())}, "
                  f"reference positives that are ours {int(ours[pos].sum())}, share of ours the reference has {shares[-1]:.4f}")
        else:
            print(f"seed {seed}: preconditions not met, skipped")
        seed += 1
    os.makedirs(os.path.join(HERE, "labels"), exist_ok=True)      # a sub-directory: the .npz files beside this script are forward cases
    path = os.path.join(HERE, "labels", "gt_labels.npz")
    np.savez_compressed(path, graphs=3, **out)
    print(path, os.path.getsize(path), "bytes; shares", shares)


if __name__ == "__main__":
    main()
