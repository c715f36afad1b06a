"""Graphs, masks and the comparison shared by tests/test_induce_cpu.py and tests/test_gpu_induce.py: an induced sub-graph built
by filtering the parent's index must equal the one cluster.induced_subgraph(method="sort") + graph.tensor_index build, element
for element (integer data: no tolerance anywhere)."""
import numpy as np
import torch

from gnnome_assembly_amd import AssemblyGraph, cluster

INDEX_KEYS = ("perm", "isrc", "idst", "in_ptr", "out_ptr", "out_pos", "out_dst")


def random_graph(seed, n, e, shuffle):
    """A banded random multigraph with every structure the index has to survive: duplicate edges, self loops, isolated nodes
    (the last tenth), nodes without in-edges (3, 17) and without out-edges (5, 23); `shuffle` scatters the caller's ids.
    Returns src, dst (int32), n and the ids of the isolated nodes."""
    rng = np.random.default_rng(seed)
    live = n - max(n // 10, 1)
    src = rng.integers(0, live, e)
    dst = np.clip(src + rng.integers(-6, 7, e), 0, live - 1)
    k = min(20, e // 4)
    src[k:2 * k], dst[k:2 * k] = src[:k], dst[:k]                   # duplicates
    dst[2 * k:2 * k + k // 2] = src[2 * k:2 * k + k // 2]           # self loops
    for v in (3, 17):
        dst[dst == v] = v + 1                                       # no in-edge
    for v in (5, 23):
        src[src == v] = v + 1                                       # no out-edge
    isolated = np.arange(live, n)
    if shuffle:
        relabel = rng.permutation(n)
        src, dst, isolated = relabel[src], relabel[dst], relabel[isolated]
    return src.astype(np.int32), dst.astype(np.int32), n, isolated


def masks(src, dst, n, isolated, block=None):
    """name -> bool mask [n]: the cases every route is checked on"""
    m = {}
    m["all"] = np.ones(n, bool)
    m["none"] = np.zeros(n, bool)
    one = np.zeros(n, bool)
    one[int(src[len(src) // 2])] = True
    m["one"] = one
    noedge = np.zeros(n, bool)                  # the isolated nodes and one node without a self loop: nodes, but no edge
    noedge[isolated] = True
    loops = set(src[src == dst].tolist())
    noedge[next(v for v in src.tolist() if v not in loops)] = True
    m["nodes_without_edges"] = noedge
    m["every_second"] = np.arange(n) % 2 == 0
    lo, hi = block if block is not None else (n // 4, n // 4 + n // 3)
    blk = np.zeros(n, bool)
    blk[lo:hi] = True
    m["block"] = blk
    return {k: torch.from_numpy(v) for k, v in m.items()}


def parent(src, dst, n, node_order, device=None, seed=0):
    """the parent graph with one ndata and one edata tensor to slice"""
    g = AssemblyGraph(src, dst, n, node_order=node_order)
    rng = np.random.default_rng(seed)
    g.ndata["x"] = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    g.edata["e"] = torch.from_numpy(rng.standard_normal((len(src), 2)).astype(np.float32))
    return g.to(device) if device is not None else g


def sort_route(g, mask):
    """the reference of every check: (nid, eid, s_sub, d_sub, index, sub-graph) of the 'sort' route"""
    sub = cluster.induced_subgraph(g, mask, method="sort")
    s, d = sub.edges()
    return sub.ndata[cluster.NID], sub.edata[cluster.EID], s, d, sub.index(), sub


def assert_same(got, want, what):
    """got / want: (nid, eid, s_sub, d_sub, index dict, ...)"""
    for name, a, b in zip(("nid", "eid", "s_sub", "d_sub"), got[:4], want[:4]):
        assert a.shape == b.shape, f"{what}: {name} has shape {tuple(a.shape)}, expected {tuple(b.shape)}"
        assert torch.equal(a.long().cpu(), b.long().cpu()), f"{what}: {name} differs"
    gi, wi = got[4], want[4]
    assert set(gi) == set(wi), f"{what}: index keys {sorted(gi)} != {sorted(wi)}"
    for k in wi:
        assert gi[k].dtype == wi[k].dtype == torch.int32, f"{what}: {k} is {gi[k].dtype}"
        assert gi[k].shape == wi[k].shape, f"{what}: {k} has shape {tuple(gi[k].shape)}, expected {tuple(wi[k].shape)}"
        assert torch.equal(gi[k].cpu(), wi[k].cpu()), f"{what}: index['{k}'] differs"
