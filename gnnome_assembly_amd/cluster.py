"""ClusterGCN-style mini-batch mode: counterpart of `dgl.dataloading.ClusterGCNSampler` +
`DataLoader(g, arange(num_clusters), sampler, batch_size, shuffle=True)` as train.py:288-293 and
:438-439 use them.  It is the reference's DEFAULT training mode
(hyperparameters.py:15-18: 500 clusters, 50 per batch) and the escape hatch when a graph's saved
activations exceed HBM.

What DGL does there, restated: METIS splits the nodes into `num_parts` balanced clusters with a
small edge cut; a mini-batch is the union of `batch_size` clusters; the sampler returns
`g.subgraph(nodes)` -- the INDUCED subgraph with relabelled nodes, edges kept in ascending original
edge id, all `ndata` / `edata` rows carried along (so `in_deg`, `out_deg`, `pe` are the FULL graph's
values, train.py:301-305).

METIS lives inside DGL and is not available here, so the PARTITIONER is this module's own (parity
with METIS's particular cut is unpinned and not attempted): overlap graphs of a chromosome are
nearly one-dimensional, so a breadth-first (Cuthill-McKee) ordering of the symmetrised graph -- the one
the graph index numbers its nodes by, gnm_graph_locality_order -- cut
into equal contiguous blocks gives balanced parts whose edge cut is the band width per boundary.
Repeat-induced long-range edges would fold that ordering; they are recognised by having no common
neighbour and left out of the ordering (not out of the graph).
The SUBGRAPH semantics (induced edges, relabelling, edge order, feature slicing) are exact and
tested against a brute-force restatement."""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import os

import numpy as np
import torch

from . import engine
from .graph import AssemblyGraph

__all__ = ["node_order", "partition_graph", "edge_cut", "induced_subgraph", "ClusterBatchLoader", "NID", "EID"]

NID = "_ID"     # dgl.NID / dgl.EID: original ids of a subgraph's nodes / edges
EID = "_ID"


def node_order(graph: AssemblyGraph, method: str = "locality") -> np.ndarray:
    """The 1-D node ordering the parts are cut from (cached on the graph: only the number of parts
    changes between epochs, train.py:291)."""
    cache = graph.__dict__.setdefault("_node_order", {})
    if method not in cache:
        n = graph.num_nodes()
        if method == "order":
            cache[method] = np.arange(n, dtype=np.int64)
        elif method == "locality":
            # the same order the graph index numbers its nodes by (gnm_graph_locality_order, host C++, linear in E:
            # breadth-first over the triangle-supported overlaps from a pseudo-peripheral node of every component)
            idx = graph.host_index() if graph._host_index is not None or graph._src_t is None else None
            if idx is not None and "nperm" in idx:
                cache[method] = idx["nperm"].astype(np.int64)           # the index has it already
            else:
                import ctypes as C
                from . import _lib
                lib = _lib.load()
                src, dst = np.ascontiguousarray(graph._src, np.int32), np.ascontiguousarray(graph._dst, np.int32)
                order, rank = np.empty(n, np.int32), np.empty(n, np.int32)
                ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
                _lib.check(lib.gnm_graph_locality_order(ptr(src), ptr(dst), n, src.size, ptr(order), ptr(rank), None),
                           "gnm_graph_locality_order")
                cache[method] = order.astype(np.int64)
        elif method == "rcm":
            import scipy.sparse as sp
            from scipy.sparse.csgraph import reverse_cuthill_mckee
            src, dst = graph._src.astype(np.int64), graph._dst.astype(np.int64)
            a = sp.csr_matrix((np.ones(2 * src.size, np.int32), (np.concatenate((src, dst)), np.concatenate((dst, src)))),
                              shape=(n, n))
            a.data[:] = 1                      # duplicates were summed
            a.setdiag(0)
            a.eliminate_zeros()
            # True overlaps are transitive (reads that overlap share neighbours); repeat-induced edges
            # join reads with disjoint neighbourhoods and act as shortcuts that fold a breadth-first
            # ordering.  Order on the triangle-supported edges only (common-neighbour count > 0).
            tri = (a @ a).multiply(a)
            tri.eliminate_zeros()
            core = tri if tri.nnz >= a.nnz // 2 else a
            core.data[:] = 1
            cache[method] = np.asarray(reverse_cuthill_mckee(sp.csr_matrix(core), symmetric_mode=True), dtype=np.int64)
        else:
            raise ValueError(f"unknown partition method {method!r}")
    return cache[method]


def partition_graph(graph: AssemblyGraph, num_parts: int, method: str = "locality") -> np.ndarray:
    """part[v] in [0, num_parts) for every node; parts are balanced to within one node.
    method 'locality': contiguous blocks of the index's own breadth-first order (default; host C++, linear in E);
           'rcm': contiguous blocks of scipy's reverse Cuthill-McKee ordering (the round-1 partitioner: E-sized sparse
                  products, kept for comparison);
           'order': contiguous blocks of the node ids themselves (reads already position-sorted)."""
    n = graph.num_nodes()
    if num_parts < 1:
        raise ValueError("num_parts must be >= 1")
    num_parts = min(num_parts, max(n, 1))
    order = node_order(graph, method)
    part = np.empty(n, np.int32)
    # block b gets positions [b*n/P, (b+1)*n/P): sizes differ by at most one
    part[order] = (np.arange(n, dtype=np.int64) * num_parts // max(n, 1)).astype(np.int32)
    return part


def edge_cut(graph: AssemblyGraph, part: np.ndarray) -> int:
    """number of edges whose end points lie in different parts"""
    return int(np.count_nonzero(part[graph._src] != part[graph._dst]))


# How a sub-graph and its index are built: 'sort' (tensor ops: compaction here, two stable sorts in graph.tensor_index) or
# 'index' (gnm_graph_induce_count / _fill: the parent's index filtered, no sort).  GNM_INDUCE sets the default; unset: 'sort'.
INDUCE = os.environ.get("GNM_INDUCE", "sort").strip().lower() or "sort"
INDUCE_METHODS = ("sort", "index")


def _induce_method(method: Optional[str]) -> str:
    method = INDUCE if method is None else method
    if method not in INDUCE_METHODS:
        raise ValueError(f"induce method {method!r}: expected one of {INDUCE_METHODS}")
    return method


def induced_subgraph(graph: AssemblyGraph, node_mask: torch.Tensor, method: Optional[str] = None) -> AssemblyGraph:
    """`g.subgraph(nodes)` of DGL: nodes relabelled in ascending original id, induced edges in
    ascending original edge id, ndata / edata rows sliced, original ids in ndata[NID] / edata[EID].
    Runs on the graph's device (mask, compaction and relabelling are E- and N-sized tensor ops).

    method 'sort' (default; None: GNM_INDUCE, else 'sort'): the sub-graph's index is built from its edge list when it is first
    asked for (graph.tensor_index).  'index': the sub-graph AND its index are derived from the parent's device index by
    gnm_graph_induce_count / gnm_graph_induce_fill (graph.induced_index_from_parent states what they compute): no sort, one
    host synchronisation; the result is the same graph with `index(dev)` already filled in.  A parent on the CPU has no device
    index to filter: 'index' then runs 'sort' and says so in `relabel_info` ('induce': 'sort', 'induce_fallback': why)."""
    method = _induce_method(method)
    dev = graph.device
    node_mask = node_mask.to(dev)
    if node_mask.dtype != torch.bool or node_mask.numel() != graph.num_nodes():
        raise ValueError("node_mask must be a bool tensor with one entry per node")
    if method == "index" and dev.type == "cuda":
        return _induced_subgraph_index(graph, node_mask)
    sub = _induced_subgraph_sort(graph, node_mask)
    if method == "index":
        sub.relabel_info.update(induce="sort", induce_fallback="the parent graph is on the CPU: no device index to filter")
    return sub


def _induced_subgraph_index(graph: AssemblyGraph, node_mask: torch.Tensor) -> AssemblyGraph:
    from .graph import induce_index_device
    dev = graph.device
    src, dst = graph.edges()
    nid, eid, s_sub, d_sub, idx = induce_index_device(src, dst, graph.num_nodes(), graph.index(dev), node_mask)
    sub = AssemblyGraph.from_tensors(s_sub, d_sub, int(nid.numel()), idx.get("nrank"))
    sub._dev_index[sub.device] = idx            # index(dev) finds it: no tensor_index, the sweep plans are built from this one
    sub.relabel_info["induce"] = "index"
    nid, eid = nid.long(), eid.long()           # as torch.nonzero gives them on the other route
    sub.ndata = {k: v[nid] for k, v in graph.ndata.items()}
    sub.edata = {k: v[eid] for k, v in graph.edata.items()}
    sub.ndata[NID] = nid
    sub.edata[EID] = eid
    return sub


def _induced_subgraph_sort(graph: AssemblyGraph, node_mask: torch.Tensor) -> AssemblyGraph:
    dev = graph.device
    src, dst = graph.edges()
    nid = torch.nonzero(node_mask, as_tuple=False).squeeze(1)
    new_id = torch.cumsum(node_mask.to(torch.int32), 0, dtype=torch.int32) - 1
    keep = node_mask[src.long()] & node_mask[dst.long()]
    eid = torch.nonzero(keep, as_tuple=False).squeeze(1)
    s_sub = new_id[src[eid].long()]
    d_sub = new_id[dst[eid].long()]
    # the parent's internal node order (graph.py "Node numbering"), restricted to the sub-graph: ranks of the kept nodes
    # compressed to 0 .. n_sub-1 -- so a mini-batch of a graph with scattered node ids is as local as the parent
    nrank = None
    pr = graph.index(dev).get("nrank")      # (builds the parent's index once; cached on the graph)
    if pr is not None:
        nrank = torch.empty(nid.numel(), dtype=torch.int64, device=dev)
        nrank[torch.argsort(pr[nid].long())] = torch.arange(nid.numel(), device=dev)
    sub = AssemblyGraph.from_tensors(s_sub, d_sub, int(nid.numel()), nrank)  # edges and index stay on the device
    sub.ndata = {k: v[nid] for k, v in graph.ndata.items()}
    sub.edata = {k: v[eid] for k, v in graph.edata.items()}
    sub.ndata[NID] = nid
    sub.edata[EID] = eid
    return sub


def _graph_tensors(sub: AssemblyGraph):
    """every device tensor a sub-graph owns: edges, index, sweep plans, features"""
    out = [t for t in (sub._src_t, sub._dst_t, sub._nrank_t) if torch.is_tensor(t)]
    for d in list(sub._dev_index.values()) + [p for p in sub._plans.values() if p] + [sub.ndata, sub.edata]:
        out += [t for t in d.values() if torch.is_tensor(t)]
    return out


PREFETCH = os.environ.get("GNM_BATCH_PREFETCH", "1") != "0"


class ClusterBatchLoader:
    """Iterates the mini-batches of one graph: `batch_size` clusters per batch, clusters shuffled when
    `shuffle` (DataLoader(..., shuffle=True, drop_last=False)); yields induced subgraphs.

    prefetch (default on a HIP device; GNM_BATCH_PREFETCH=0 turns it off): batch k+1 -- its induced sub-graph, its index and both
    sweep plans -- is built on a SIDE stream while the caller's kernels of batch k run (the reference gets the same overlap from
    DataLoader(num_workers=4), train.py:293).  Building a sub-graph ends in host synchronisations (torch.nonzero: the sub-graph's
    sizes are launch arguments); on the caller's stream each of them waits for the whole previous training step and the device
    then idles while the host issues the next one -- and the ~2 ms of index / plan kernels (one wave per sweep workgroup, latency
    bound) sit on the critical path of a 21 ms step.  On the side stream the synchronisations wait for the small build kernels
    only, which run in the gaps of the training kernels.  The caller's stream waits for the build's event before it touches the
    batch; every tensor of the batch is handed over with record_stream, so the caching allocator does not recycle it under the
    training kernels."""

    def __init__(self, graph: AssemblyGraph, part: np.ndarray, batch_size: int, shuffle: bool = True,
                 generator: Optional[torch.Generator] = None, prefetch: Optional[bool] = None, induce: Optional[str] = None):
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.induce = _induce_method(induce)        # how the batches are built (induced_subgraph's method); None: GNM_INDUCE
        self.graph = graph
        self.part = torch.from_numpy(np.ascontiguousarray(part, dtype=np.int32)).to(graph.device)
        self.num_parts = int(part.max()) + 1 if part.size else 0
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.generator = generator
        self.prefetch = (PREFETCH if prefetch is None else bool(prefetch)) and graph.device.type == "cuda"
        self._side = None

    def __len__(self) -> int:
        return (self.num_parts + self.batch_size - 1) // self.batch_size

    def batches(self) -> List[torch.Tensor]:
        ids = torch.randperm(self.num_parts, generator=self.generator) if self.shuffle else torch.arange(self.num_parts)
        return [ids[i:i + self.batch_size] for i in range(0, self.num_parts, self.batch_size)]

    def _build(self, ids: torch.Tensor) -> AssemblyGraph:
        dev = self.graph.device
        sel = torch.zeros(self.num_parts, dtype=torch.bool, device=dev)
        sel[ids.to(dev)] = True
        return induced_subgraph(self.graph, sel[self.part.long()], self.induce)

    def __iter__(self) -> Iterator[AssemblyGraph]:
        dev = self.graph.device
        batches = self.batches()
        if not self.prefetch:
            for ids in batches:
                yield self._build(ids)
            return
        self.graph.index(dev)                       # the parent's index (cached) before anything runs on the side stream
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev)
        side = self._side

        def build(ids):
            # device and stream contexts are entered HERE only -- never held across a yield (a generator that yields inside
            # `with torch.cuda.device(...)` leaks the context into its consumer until it is closed) -- and the consumer's stream is
            # looked up at every hand-over: whatever stream is current in the caller when it asks for a batch is the one that
            # waits for the build and that the batch's tensors are recorded on
            with torch.cuda.device(dev):
                with torch.cuda.stream(side):
                    sub = self._build(ids)
                    sub.index(dev)
                    if hasattr(sub, "sweep_plan"):
                        sub.sweep_plan(dev, 1)
                        sub.sweep_plan(dev, engine.GATE2_WG)
                    ev = torch.cuda.Event()
                    ev.record(side)
            return sub, ev

        def hand_over(sub, ev):
            with torch.cuda.device(dev):
                consumer = torch.cuda.current_stream(dev)
                consumer.wait_event(ev)
                for t in _graph_tensors(sub):
                    t.record_stream(consumer)
            return sub
        # The side stream waits for the caller's stream ONCE, here: the parent graph's tensors as they are when the iteration starts.
        # (Waiting before every build -- tried in round 6 on ADVICE r5 -- makes build k+1 wait for batch k's training kernels: the overlap
        # this loader exists for is gone, 43 -> 38 M edges/s on the mini-batch epoch.)  The contract instead: the parent's ndata / edata
        # are read-only while its batches are being iterated, as in the reference's loop (train.py:296-343 only reads them).
        with torch.cuda.device(dev):
            side.wait_stream(torch.cuda.current_stream(dev))
        nxt = build(batches[0]) if batches else None
        for k in range(len(batches)):
            sub = hand_over(*nxt)
            yield sub                               # the caller issues batch k's kernels, then asks for the next batch:
            nxt = build(batches[k + 1]) if k + 1 < len(batches) else None           # built while those kernels run
