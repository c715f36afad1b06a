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

__all__ = ["node_order", "partition_graph", "edge_cut", "induced_subgraph", "ClusterBatchLoader", "NID", "EID",
           "masked_subgraph", "MaskedGraphLoader", "read_mask_host", "index_degrees_torch"]

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


def _iterate_built(loader, items: Sequence, build_one, parents: Sequence[AssemblyGraph]) -> Iterator[AssemblyGraph]:
    """The one iteration of every loader here (ClusterBatchLoader, MaskedGraphLoader): yields build_one(item) for every item.
    With `loader.prefetch`, item k+1 -- its sub-graph, its index and both sweep plans -- is built on the loader's side stream
    (`loader._side`, created on first use) while the caller's kernels of item k run, and handed over with an event wait and
    record_stream.  `parents`: the graphs the items are cut from, whose index is built before anything runs on the side stream."""
    if not loader.prefetch:
        for item in items:
            yield build_one(item)
        return
    dev = parents[0].device
    for parent in parents:
        parent.index(dev)                           # the parent's index (cached) before anything runs on the side stream
    if loader._side is None:
        loader._side = torch.cuda.Stream(device=dev)
    side = loader._side

    def build(item):
        # device and stream contexts are entered HERE only -- never held across a yield (a generator that yields inside
        # `with torch.cuda.device(...)` leaks the context into its consumer until it is closed) -- and the consumer's stream is
        # looked up at every hand-over: whatever stream is current in the caller when it asks for a batch is the one that
        # waits for the build and that the batch's tensors are recorded on
        with torch.cuda.device(dev):
            with torch.cuda.stream(side):
                sub = build_one(item)
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
    nxt = build(items[0]) if len(items) else None
    for k in range(len(items)):
        sub = hand_over(*nxt)
        yield sub                                   # the caller issues item k's kernels, then asks for the next one:
        nxt = build(items[k + 1]) if k + 1 < len(items) else None               # built while those kernels run


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
    training kernels.

    read_mask (optional; the read-masking augmentation in mini-batch mode): dict(key, epoch, graph_index, fractions) with one
    kept fraction per batch.  Batch k is then the sub-graph of `cluster selection & read mask(fractions[k])` -- ONE induce, through
    masked_subgraph, so its `pe` carries the thinned batch's degrees; the partition stays the parent's."""

    def __init__(self, graph: AssemblyGraph, part: np.ndarray, batch_size: int, shuffle: bool = True,
                 generator: Optional[torch.Generator] = None, prefetch: Optional[bool] = None, induce: Optional[str] = None,
                 read_mask: Optional[Dict] = None):
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
        self.read_mask = read_mask
        if read_mask is not None:
            if len(read_mask["fractions"]) != len(self):
                raise ValueError(f"read_mask: {len(read_mask['fractions'])} fractions for {len(self)} batches")
            if read_mask.get("recompute_pe"):       # features.positional_encoding works in the device's shared scratch buffers
                self.prefetch = False

    def __len__(self) -> int:
        return (self.num_parts + self.batch_size - 1) // self.batch_size

    def batches(self) -> List[torch.Tensor]:
        ids = torch.randperm(self.num_parts, generator=self.generator) if self.shuffle else torch.arange(self.num_parts)
        return [ids[i:i + self.batch_size] for i in range(0, self.num_parts, self.batch_size)]

    def selection(self, ids: torch.Tensor) -> torch.Tensor:
        """bool [N]: the nodes of the clusters `ids`"""
        dev = self.graph.device
        sel = torch.zeros(self.num_parts, dtype=torch.bool, device=dev)
        sel[ids.to(dev)] = True
        return sel[self.part.long()]

    def _build(self, ids: torch.Tensor, k: Optional[int] = None) -> AssemblyGraph:
        rm = self.read_mask
        if rm is None or k is None:
            return induced_subgraph(self.graph, self.selection(ids), self.induce)
        return masked_subgraph(self.graph, rm["fractions"][k], rm["key"], rm["epoch"], rm["graph_index"], self.induce,
                               select=self.selection(ids), recompute_pe=bool(rm.get("recompute_pe")))

    def __iter__(self) -> Iterator[AssemblyGraph]:
        batches = self.batches()
        if self.read_mask is None:
            yield from _iterate_built(self, batches, self._build, [self.graph])
        else:
            yield from _iterate_built(self, list(enumerate(batches)), lambda kb: self._build(kb[1], kb[0]), [self.graph])


# ---------------------------------------------------------------------------------------------------------------------------------
# Read-masking coverage augmentation: a training step on the sub-graph induced by a random subset of the READS.  A read set thinned
# to the fraction f is, to first order, the same genome sequenced at f times the coverage, so a model trained on thinned graphs
# meets at inference the node degrees of the coverages it will be used at -- and the degrees are the first two columns of `pe`.
# The mask is a pure function of (f, key, epoch, graph_index, node) (include/gnm.h, gnm_read_mask): nothing is stored, and any
# rank, test or later run re-derives it from five numbers.
# ---------------------------------------------------------------------------------------------------------------------------------
_PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
_PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))


def read_mask_host(n: int, f: float, key: int, epoch: int, graph_index: int) -> np.ndarray:
    """gnm_read_mask on the host (numpy, bool [n]): the route of a parent graph on the CPU, as induced_subgraph has one.  Read
    r = v >> 1, Philox4x32-10 with key (key low, key high) on the counter (q low, q high, graph_index, epoch), q = r >> 2; word
    r & 3 is the draw x; kept iff (x >> 8) * 2^-24 < float32(f)."""
    f = engine.read_mask_fraction(f)
    n = int(n)
    key = int(key) & (2 ** 64 - 1)
    lo, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    q = np.arange((n + 7) // 8, dtype=np.uint64)
    c0, c1 = q & lo, q >> s32
    c2 = np.full_like(q, int(graph_index) & 0xFFFFFFFF)
    c3 = np.full_like(q, int(epoch) & 0xFFFFFFFF)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    for _ in range(10):
        p0, p1 = _PHILOX_M[0] * c0, _PHILOX_M[1] * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & lo, (p0 >> s32) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + _PHILOX_W[0]) & lo, (k1 + _PHILOX_W[1]) & lo
    x = np.stack((c0, c1, c2, c3), 1).reshape(-1)              # one word per read, in read order
    u = (x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.repeat(u < np.float32(f), 2)[:n]


def index_degrees_torch(idx, pe: torch.Tensor) -> torch.Tensor:
    """gnm_index_degrees in tensor ops (the host route, and the statement the kernel is tested against): columns 0 and 1 of the
    caller's row nperm[i] of pe [n, >= 2] = in_ptr[i+1] - in_ptr[i], out_ptr[i+1] - out_ptr[i]; in place."""
    ind = (idx["in_ptr"][1:] - idx["in_ptr"][:-1]).to(pe.dtype)
    outd = (idx["out_ptr"][1:] - idx["out_ptr"][:-1]).to(pe.dtype)
    nperm = idx.get("nperm")
    if nperm is None:
        pe[:, 0], pe[:, 1] = ind, outd
    else:
        pe[nperm.long(), 0], pe[nperm.long(), 1] = ind, outd
    return pe


def masked_subgraph(graph: AssemblyGraph, f: float, key: int, epoch: int, graph_index: int, method: Optional[str] = None,
                    select: Optional[torch.Tensor] = None, recompute_pe: bool = False) -> AssemblyGraph:
    """The graph thinned to the reads that engine.read_mask(n, f, key, epoch, graph_index) keeps: induced_subgraph of that mask
    (`method` / GNM_INDUCE choose the route; `select`, bool [N]: ANDed into it first -- a mini-batch's cluster selection, still one
    induce).  Every ndata / edata row is carried from the parent as induced_subgraph carries it, with one exception: `ndata["pe"]`
    ([N, 2 + k]: in-degree | out-degree | k PageRank columns, as train._cluster_batches attaches it) is a copy whose columns 0 and
    1 are the THINNED graph's degrees (engine.index_degrees on the sub-graph's own index); the PageRank columns stay the parent's
    unless `recompute_pe`, which runs features.positional_encoding on the sub-graph (HIP device only).  relabel_info records
    'mask_fraction', 'mask_kept_nodes' and 'mask' ('device', or 'host' for a parent on the CPU: read_mask_host)."""
    f = engine.read_mask_fraction(f)
    dev = graph.device
    n = graph.num_nodes()
    if dev.type == "cuda":
        mask = engine.read_mask(n, f, key, epoch, graph_index, dev)
    else:
        mask = torch.from_numpy(read_mask_host(n, f, key, epoch, graph_index))
    if select is not None:
        select = select.to(dev)
        if select.dtype != torch.bool or select.numel() != n:
            raise ValueError("select must be a bool tensor with one entry per node")
        mask = mask & select
    sub = induced_subgraph(graph, mask, method)
    pe = sub.ndata.get("pe")
    if pe is not None:
        if pe.dim() != 2 or pe.shape[1] < 2:
            raise ValueError("masked_subgraph: ndata['pe'] must be [N, 2 + k]: in-degree | out-degree | positional encoding")
        if recompute_pe:
            from . import features
            sub.ndata["pe"] = features.positional_encoding(sub, pe.shape[1] - 2)
        elif dev.type == "cuda":
            sub.ndata["pe"] = engine.index_degrees(sub.index(dev), pe.contiguous())     # pe: the slice's own memory already
        else:
            sub.ndata["pe"] = index_degrees_torch(sub.index(dev), pe.contiguous())
    sub.relabel_info.update(mask_fraction=f, mask_kept_nodes=sub.num_nodes(), mask="device" if dev.type == "cuda" else "host")
    return sub


class MaskedGraphLoader:
    """One thinned graph per training step of an epoch: `steps` is the epoch's list of (graph, f, graph_index) in step order, the
    graphs with their features on ndata / edata (train._attach_features); yields masked_subgraph(graph, f, key, epoch,
    graph_index) for each.  With prefetch (default on a HIP device; GNM_BATCH_PREFETCH=0 turns it off) step k+1's graph, its index
    and both sweep plans are built on a side stream while step k runs, with ClusterBatchLoader's hand-over (_iterate_built); the
    parents' ndata / edata are read-only while the iteration is in flight.  recompute_pe builds in line: the PageRank kernels
    work in the device's shared scratch buffers, which the training step on the caller's stream uses too."""

    def __init__(self, steps: Sequence[Tuple[AssemblyGraph, float, int]], key: int, epoch: int, prefetch: Optional[bool] = None,
                 induce: Optional[str] = None, recompute_pe: bool = False):
        self.steps = list(steps)
        self.key, self.epoch = int(key), int(epoch)
        self.induce = _induce_method(induce)
        self.recompute_pe = bool(recompute_pe)
        devs = {g.device for g, _, _ in self.steps}
        if len(devs) > 1:
            raise ValueError(f"MaskedGraphLoader: the graphs of an epoch live on {sorted(map(str, devs))}: expected one device")
        on_gpu = bool(devs) and next(iter(devs)).type == "cuda"
        self.prefetch = (PREFETCH if prefetch is None else bool(prefetch)) and on_gpu and not self.recompute_pe
        self._side = None

    def __len__(self) -> int:
        return len(self.steps)

    def _build(self, step) -> AssemblyGraph:
        g, f, graph_index = step
        return masked_subgraph(g, f, self.key, self.epoch, graph_index, self.induce, recompute_pe=self.recompute_pe)

    def __iter__(self) -> Iterator[AssemblyGraph]:
        parents = list({id(g): g for g, _, _ in self.steps}.values())
        yield from _iterate_built(self, self.steps, self._build, parents)

