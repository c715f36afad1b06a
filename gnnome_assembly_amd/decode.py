"""Greedy decode of contigs from edge scores: counterpart of `inference.get_contigs` with
`sample_edges`, `walk_forwards`, `walk_backwards`, `get_contig_length`, `get_subgraph`
(inference.py:20-77,182-277).

The step consumes `g.edata['score']` BY EDGE ID (inference.py:454) -- the reason the model returns
logits in the caller's edge-id order.  It is sequential, branchy CPU work (greedy walks over
adjacency lists); the reference runs it in Python over dict-of-lists, here the walks, the best-walk
choice and the visited-set update of one iteration are one C++ call on CSR arrays
(`gnm_decode_iteration`, libgnm.so, host side).  Python keeps the loop, the candidate edge list of the
not-yet-visited sub-graph and the sampling, which uses the reference's own torch call so that a
seeded run draws the same start edges.

Differences from the reference, both deliberate:
  * self loops are dropped from the CANDIDATES only, edge ids are never renumbered (the reference
    calls dgl.remove_self_loop and then indexes the renumbered scores with ids of the original
    graph, which is only consistent when there are no self loops);
  * a cycle of forced single-successor moves raises instead of looping forever.

`get_contigs_device` is the opt-in form whose O(E) work per iteration -- the candidate list of the not-yet-visited
sub-graph, the sigmoid, the normalisation and the draw -- runs on the device where the logits already are
(gnm_decode_candidate_sums / gnm_decode_pick, inverse-CDF sampling), and whose candidate walks run side by side on host
threads (gnm_decode_iteration_mt).  It draws from the same distribution as `sample_edges`, not the same random numbers.

`best_overlap_contigs` is a second, deterministic decoder that runs on the device as a whole (gnm_bog_contigs): the mutual-best
edges of the scores form disjoint paths, which list ranking turns into contigs; `resolve_strands` then keeps one strand per read.
A different algorithm from the greedy walk, not a faster form of it: the walk follows a forced single successor even when that
edge is not the successor's best predecessor, the cover does not.

`greedy_cover_contigs` iterates those mutual-best links on the device (gnm_cover_rounds) until no node with a free slot finds a
free partner: the greedy path cover of overlap-layout assemblers, of which `best_overlap_contigs` is round one.

`transitive_support` marks, on the device (gnm_transitive_support), the candidate edges a two-step path of shorter prefix explains
(the string-graph reduction); with reduce_transitive=True the two cover decoders run on the scores with those edges masked out, so
that a link cannot jump over reads and leave them to a parallel contig.

`resolve_strands_device` is `resolve_strands` on the device (gnm_resolve_prepare / _rounds / _layout): the same pieces in the same
order, as a `BogContigs` that `contig_sequences` and `junction_identity` take as it is.

`contig_sequences` turns the walks of any of the decoders into bases on the device over a packed `reads.ReadStore`
(gnm_seq_layout / gnm_seq_emit), `ContigSequences.write_fasta`, `ng50` and `quick_evaluation` are evaluate.py's FASTA and report."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

from . import _lib
from .engine import RecordStats

__all__ = ["DecodeGraph", "sample_edges", "get_contigs", "get_contigs_device", "infer_contigs", "decision_table",
           "best_overlap_contigs", "greedy_cover_contigs", "BogContigs", "BogStats", "transitive_support", "TransitiveSupport",
           "ReduceStats", "resolve_strands", "ResolvedContigs", "resolve_strands_device", "StrandContigs", "ResolveStats", "n50", "junction_identity", "JunctionIdentity",
           "contig_sequences", "ContigSequences", "SeqStats", "walk_edge_ids", "ng50", "quick_evaluation", "CHR_LENGTHS"]


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class DecodeGraph:
    """Adjacency of a graph in edge-id order (what the reference pickles as *_succ.pkl, *_pred.pkl,
    *_edges.pkl; graph_parser.py:13-73), as CSR arrays."""

    def __init__(self, src, dst, num_nodes: int):
        self.src = np.ascontiguousarray(np.asarray(src), dtype=np.int32)
        self.dst = np.ascontiguousarray(np.asarray(dst), dtype=np.int32)
        self.n = int(num_nodes)
        e = self.src.size
        mk = lambda m: np.empty(m, np.int32)  # noqa: E731
        self.succ = (mk(self.n + 1), mk(e), mk(e))
        self.pred = (mk(self.n + 1), mk(e), mk(e))
        lib = _lib.load()
        _lib.check(lib.gnm_decode_build_adjacency(_p(self.src), _p(self.dst), self.n, e, *[_p(a) for a in self.succ],
                                                  *[_p(a) for a in self.pred]), "gnm_decode_build_adjacency")
        self._dev = {}      # device -> (src, dst) int32 on that device (get_contigs_device uploads them once)

    def on_device(self, device):
        """(src, dst) as int32 tensors on `device`, uploaded once per DecodeGraph."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.src).to(device), torch.from_numpy(self.dst).to(device))
        return self._dev[device]

    def successors(self, v: int) -> List[int]:
        ptr, nbr, _ = self.succ
        return nbr[ptr[v]:ptr[v + 1]].tolist()

    def predecessors(self, v: int) -> List[int]:
        ptr, nbr, _ = self.pred
        return nbr[ptr[v]:ptr[v + 1]].tolist()


def sample_edges(edge_scores: torch.Tensor, nb_paths: int) -> torch.Tensor:
    """inference.py:270-277: nb_paths independent start edges with p ~ sigmoid(score).  Up to 5e7
    probabilities this is the reference's own call (same draws for the same torch seed); beyond that
    its nb_paths-fold copy of the probability vector is replaced by torch.multinomial with replacement
    -- the same distribution without the copy."""
    p = torch.sigmoid(edge_scores.detach().float().cpu()).reshape(-1)
    p = p.masked_fill(p < 1e-9, 1e-9)
    p = p / p.sum()
    if p.numel() * nb_paths <= 50_000_000:
        return torch.distributions.categorical.Categorical(p.repeat(nb_paths, 1)).sample()
    return torch.multinomial(p, nb_paths, replacement=True)


def _host_walk_args(graph: DecodeGraph, num_scores: int, prefix_length, read_length, visited):
    """What the host walks of get_contigs / get_contigs_device read besides the scores: (prefix_length, read_length) as int64
    arrays and `visited` (a fresh one for None), checked against the graph."""
    n, e = graph.n, graph.src.size
    pl = np.ascontiguousarray(torch.as_tensor(prefix_length).cpu().numpy().reshape(-1), dtype=np.int64)
    rl = np.ascontiguousarray(torch.as_tensor(read_length).cpu().numpy().reshape(-1), dtype=np.int64)
    if num_scores != e or pl.size != e or rl.size != n:
        raise ValueError("scores / prefix_length need one entry per edge, read_length one per node")
    vis = np.zeros(n, np.uint8) if visited is None else visited
    if vis.dtype != np.uint8 or vis.size != n or not vis.flags.c_contiguous:
        raise ValueError("visited must be a contiguous uint8 array with one entry per node")
    return pl, rl, vis


def get_contigs(graph: DecodeGraph, scores, prefix_length, read_length, nb_paths: int = 50, len_threshold: int = 20,
                sampler: Callable[[torch.Tensor, int], torch.Tensor] = sample_edges,
                visited: Optional[np.ndarray] = None) -> List[List[int]]:
    """Iteratively extract walks until the best candidate has fewer than `len_threshold` nodes
    (inference.py:182-253).  `scores` [E] in edge-id order (logits), `prefix_length` [E], `read_length` [N]
    (g.edata['prefix_length'], g.ndata['read_length']).  Returns the walks as lists of node ids."""
    lib = _lib.load()
    n = graph.n
    sc = np.ascontiguousarray(torch.as_tensor(scores).detach().float().cpu().numpy().reshape(-1))
    pl, rl, vis = _host_walk_args(graph, sc.size, prefix_length, read_length, visited)
    sct = torch.from_numpy(sc)
    no_loop = graph.src != graph.dst
    walk = np.empty(2 * n + 2, np.int32)
    best_len = C.c_int64(0)
    contigs: List[List[int]] = []
    while True:
        free = vis == 0
        eid = np.flatnonzero(free[graph.src] & free[graph.dst] & no_loop)      # get_subgraph (:256-267)
        if eid.size == 0:
            break
        picks = eid[sampler(sct[torch.from_numpy(eid)], nb_paths).numpy().reshape(-1)]
        s0 = np.ascontiguousarray(graph.src[picks])
        d0 = np.ascontiguousarray(graph.dst[picks])
        length = lib.gnm_decode_iteration(n, _p(sc), _p(pl), _p(rl), *[_p(a) for a in graph.succ],
                                          *[_p(a) for a in graph.pred], _p(vis), int(picks.size), _p(s0), _p(d0),
                                          int(len_threshold), _p(walk), walk.size, C.byref(best_len))
        if length < 0:
            _lib.check(int(length), "gnm_decode_iteration")
        if length < len_threshold:
            break
        contigs.append(walk[:length].tolist())
    return contigs


def decode_threads(nb_paths: int) -> int:
    """Host threads of one iteration's candidate walks: min(nb_paths, 16), or GNM_DECODE_THREADS.  Deliberately not the
    machine's core count: a job is usually entitled to a slice of a large host."""
    env = os.environ.get("GNM_DECODE_THREADS", "").strip()
    return max(1, int(env)) if env else max(1, min(int(nb_paths), 16))


def get_contigs_device(graph: DecodeGraph, scores, prefix_length, read_length, nb_paths: int = 50, len_threshold: int = 20,
                       generator: Optional[torch.Generator] = None,
                       uniforms: Optional[Callable[[int, int], np.ndarray]] = None, threads: Optional[int] = None,
                       visited: Optional[np.ndarray] = None, timings: Optional[list] = None) -> List[List[int]]:
    """`get_contigs` with the start edges sampled on the device and the candidate walks on `threads` host threads
    (default `decode_threads(nb_paths)`).

    `scores` [E] must be a tensor on a HIP device; it is copied to the host once, for the walks.  Per iteration the device
    forms the candidate weights w (0 for an edge with a visited end or a self loop, else max(sigmoid(score), 1e-9)) and
    their fp64 prefix sums over fixed blocks of edge ids, and turns nb_paths uniforms u into the edges
    min{k : C_k > u * total}; the host reads back nb_paths picks and the candidate count, nothing of size E.  After every
    accepted contig the N bytes of `visited` go to the device mirror.

    This draws from the SAME DISTRIBUTION as `sample_edges` (inference.py:270-277: p = w / sum(w) over the candidate
    edges), by inverse CDF from `torch.rand(nb_paths, dtype=float64, generator=generator)` -- not the same random numbers
    as torch's Categorical / multinomial: a seeded run does not reproduce the reference's draws, `get_contigs` does.
    `uniforms(iteration, nb_paths) -> float64[nb_paths]` in [0, 1) replaces the generator (tests).
    `timings`: a list that receives (sampling seconds, walks seconds) per iteration (tools/decode_timing.py)."""
    import time
    from .engine import _call, _ptr, _stream, scratch
    lib = _lib.load()
    if not torch.is_tensor(scores) or scores.device.type != "cuda":
        raise _lib.GnmError("get_contigs_device: scores must be a tensor on a HIP device (get_contigs decodes host scores)")
    dev = scores.device
    n, e = graph.n, graph.src.size
    sd = scores.detach().reshape(-1)
    sd = (sd if sd.dtype == torch.float32 else sd.float()).contiguous()
    pl, rl, vis = _host_walk_args(graph, sd.numel(), prefix_length, read_length, visited)
    nb = int(nb_paths)
    if e == 0 or nb <= 0:
        return []
    nthreads = decode_threads(nb) if threads is None else max(1, int(threads))
    contigs: List[List[int]] = []
    with torch.cuda.device(dev):
        sc = np.ascontiguousarray(sd.cpu().numpy())                   # the one copy of the scores, for the walks
        src_d, dst_d = graph.on_device(dev)
        vis_h = torch.from_numpy(vis)
        vis_d = vis_h.to(dev)
        need = lib.gnm_decode_sample_workspace_bytes(e)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)         # its own buffer: the prefix lives across two calls
        out_d = torch.zeros(32 + 4 * nb, dtype=torch.uint8, device=dev)   # stats (gnm.h) | picks
        picks_ptr = C.c_void_p(out_d.data_ptr() + 32)
        walk = np.empty(2 * n + 2, np.int32)
        best_len = C.c_int64(0)
        it = 0
        while True:
            t0 = time.perf_counter()
            u = uniforms(it, nb) if uniforms is not None else torch.rand(nb, dtype=torch.float64, generator=generator)
            u = torch.as_tensor(u, dtype=torch.float64).reshape(-1)
            if u.numel() != nb or bool(((u < 0) | (u >= 1)).any()):
                raise ValueError("uniforms must return nb_paths float64 values in [0, 1)")
            u_d = u.to(dev)
            _call("gnm_decode_candidate_sums", e, n, _ptr(sd), _ptr(src_d), _ptr(dst_d), _ptr(vis_d), _ptr(ws), need,
                  C.c_void_p(0), _ptr(out_d), _stream())
            _call("gnm_decode_pick", e, n, _ptr(sd), _ptr(src_d), _ptr(dst_d), _ptr(vis_d), _ptr(ws), _ptr(out_d), nb,
                  _ptr(u_d), picks_ptr, _stream())
            out = out_d.cpu().numpy()
            if int(out[8:16].view(np.int64)[0]) == 0:                  # no candidate edge left
                break
            picks = out[32:].view(np.int32)
            s0 = np.ascontiguousarray(graph.src[picks])
            d0 = np.ascontiguousarray(graph.dst[picks])
            t1 = time.perf_counter()
            length = lib.gnm_decode_iteration_mt(n, _p(sc), _p(pl), _p(rl), *[_p(a) for a in graph.succ],
                                                 *[_p(a) for a in graph.pred], _p(vis), nb, _p(s0), _p(d0),
                                                 int(len_threshold), _p(walk), walk.size, C.byref(best_len), nthreads)
            t2 = time.perf_counter()
            if length < 0:
                _lib.check(int(length), "gnm_decode_iteration_mt")
            if length >= len_threshold:
                vis_d.copy_(vis_h)                                     # N bytes: the device mirror of visited
            if timings is not None:                                    # the mirror's upload counts as sampling time
                timings.append((t1 - t0 + time.perf_counter() - t2, t2 - t1))
            if length < len_threshold:
                break
            contigs.append(walk[:length].tolist())
            it += 1
    return contigs


def decision_table(graph, scores, y=None):
    """The choices the greedy walks make on `scores`, for every node at once (gnm_decision_stats, one launch): returns
    (best_succ, best_pred, DecisionMetrics).  best_succ[v] / best_pred[v] (int32 [N] on the graph's device, the CALLER's node
    numbering) are the edge ids of the top-scored out-edge / in-edge of node v -- what walk_forwards / walk_backwards take at v
    while all its neighbours are free (inference.py:45-51) -- with self loops left out, ties to the lowest edge id, NaN below
    every number, and -1 where v has no candidate.  `graph`: an AssemblyGraph on a HIP device; `scores` [E] in edge-id order;
    `y` [E] (optional): the edge labels, for the accuracy counters; without it the metrics hold the node counts (dead, forced,
    branch, branch_nan) alone and every accuracy is NaN.  The walks themselves stay on the host and do not read the tables."""
    from .graph import as_assembly_graph
    from .metrics import DecisionStats
    g = as_assembly_graph(graph)
    dev = g.device
    if dev.type != "cuda":
        raise _lib.GnmError("decision_table: the graph must be on a HIP device (no CPU fallback)")
    n = g.num_nodes()
    best_succ = torch.empty(n, dtype=torch.int32, device=dev)
    best_pred = torch.empty(n, dtype=torch.int32, device=dev)
    st = DecisionStats(dev).add(g, scores, y, best_succ, best_pred)
    return best_succ, best_pred, st.read()


def n50(lengths) -> int:
    """The N50 of a set of lengths: the largest L such that the lengths >= L sum to at least half of the total; 0 for none."""
    a = np.sort(np.asarray(lengths, dtype=np.int64).reshape(-1))[::-1]
    if a.size == 0:
        return 0
    cum = np.cumsum(a)
    return int(a[int(np.searchsorted(cum, (int(cum[-1]) + 1) // 2))])


@dataclass
class BogStats(RecordStats):
    """A gnm_bog_record (include/gnm.h): contigs, links (kept, after the cycle cuts), cycles_cut, dropped (mutual-best edges
    refused for a NaN score or min_logit), wrong_links (links whose label is not 1), multi_nodes / multi_contigs (nodes on and
    number of paths of two or more nodes), calls."""
    contigs: int = 0
    links: int = 0
    cycles_cut: int = 0
    dropped: int = 0
    wrong_links: int = 0
    multi_nodes: int = 0
    multi_contigs: int = 0
    calls: int = 0

    @property
    def wrong_link_fraction(self) -> float:
        return float(self.wrong_links) / float(self.links) if self.links else float("nan")


class BogContigs:
    """The best-overlap contigs of one graph, on the graph's device: contig c holds the nodes
    walk_nodes[contig_ptr[c] : contig_ptr[c+1]] in walk order, joined by the edges walk_edges[...] (-1 at a contig's first node);
    bases[c] is its length in bases (get_contig_length), wrong[c] the number of its links whose label is not 1 (0 without labels).
    Contigs are numbered by ascending id of their first node.  `stats`: BogStats.  The host views are copied once, on first use."""

    def __init__(self, contig_ptr, walk_nodes, walk_edges, bases, wrong, stats: BogStats, prefix_length, read_length):
        self.contig_ptr, self.walk_nodes, self.walk_edges, self.bases, self.wrong = contig_ptr, walk_nodes, walk_edges, bases, wrong
        self.stats = stats
        self.prefix_length, self.read_length = prefix_length, read_length
        self._host = None

    def __len__(self):
        return int(self.bases.numel())

    def host(self):
        """dict of numpy arrays: contig_ptr, walk_nodes, walk_edges, bases, wrong, prefix_length, read_length."""
        if self._host is None:
            self._host = {k: getattr(self, k).cpu().numpy() for k in
                          ("contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong", "prefix_length", "read_length")}
        return self._host

    def num_nodes(self) -> torch.Tensor:
        """int32 [C] on the device: the number of nodes of every contig."""
        return self.contig_ptr[1:] - self.contig_ptr[:-1]

    def walks(self, min_nodes: int = 1) -> List[List[int]]:
        """The contigs of at least `min_nodes` nodes as lists of node ids, in the format get_contigs returns."""
        h = self.host()
        ptr, nodes = h["contig_ptr"], h["walk_nodes"]
        return [nodes[ptr[c]:ptr[c + 1]].tolist() for c in range(ptr.size - 1) if ptr[c + 1] - ptr[c] >= min_nodes]

    def _bases(self, min_nodes: int) -> np.ndarray:
        h = self.host()
        return h["bases"][np.diff(h["contig_ptr"]) >= min_nodes]

    def n50(self, min_nodes: int = 1) -> int:
        return n50(self._bases(min_nodes))

    def longest(self, min_nodes: int = 1) -> int:
        b = self._bases(min_nodes)
        return int(b.max()) if b.size else 0


@dataclass
class ReduceStats(RecordStats):
    """A gnm_reduce_record (include/gnm.h): edges (seen), candidates (no self loop, no NaN, >= min_logit), reduced (candidates with
    support > 0), reduced_label1 (of those, the edges whose label is 1; 0 without labels), witnesses (the sum of support),
    max_support, self_loops, calls."""
    edges: int = 0
    candidates: int = 0
    reduced: int = 0
    reduced_label1: int = 0
    witnesses: int = 0
    max_support: int = 0
    self_loops: int = 0
    calls: int = 0

    @property
    def reduced_fraction(self) -> float:
        """reduced / candidates; NaN without a candidate."""
        return float(self.reduced) / float(self.candidates) if self.candidates else float("nan")


class TransitiveSupport:
    """transitive_support's result, on the graph's device: support int32 [E] and masked_scores fp32 [E] in edge-id order (the
    scores, NaN on every reduced edge), stats: ReduceStats."""

    def __init__(self, support, masked_scores, stats: ReduceStats):
        self.support, self.masked_scores, self.stats = support, masked_scores, stats


def _reduce_args(who: str, reduce_transitive, fuzz):
    """Checks the two arguments the cover decoders share; returns fuzz as given."""
    from .engine import reduce_fuzz_word
    if not isinstance(reduce_transitive, (bool, np.bool_)):
        raise ValueError(f"{who}: reduce_transitive={reduce_transitive!r}: expected True or False")
    reduce_fuzz_word(fuzz, f"{who}: fuzz")
    return fuzz


def _reduce_launch(g, scores, pl, y, min_logit, fuzz):
    """The launch behind transitive_support and the decoders' reduce_transitive: (support, masked_scores, record), nothing read
    back.  pl: int64 [E] on the graph's device."""
    from . import engine
    dev = g.device
    E = g.num_edges()
    if scores.numel() != E or pl.numel() != E:
        raise ValueError("scores / prefix_length need one entry per edge")
    with torch.cuda.device(dev):
        support = torch.empty(E, dtype=torch.int32, device=dev)
        masked = torch.empty(E, dtype=torch.float32, device=dev)
        rec = torch.zeros(engine.REDUCE_RECORD_WORDS, dtype=torch.int64, device=dev)
        engine.transitive_support(g.index(dev), scores, pl, y, min_logit, fuzz, support, masked, rec)
    return support, masked, rec


def transitive_support(graph, scores, prefix_length, y=None, min_logit: float = float("-inf"), fuzz: Optional[int] = None
                       ) -> TransitiveSupport:
    """The string-graph reduction of the candidate edges of `scores`, computed on the device in one launch
    (gnm_transitive_support).  A candidate is the cover decoders': no self loop, a score that is no NaN and >= min_logit.  For
    every edge k = (a -> c), support[k] counts the candidate out-edges j = (a -> b) of a, b not a and not c, with
    prefix_length[j] < prefix_length[k] strictly, for which a candidate edge m = (b -> c) exists -- with an integer fuzz >= 0 one
    that also has |prefix_length[j] + prefix_length[m] - prefix_length[k]| <= fuzz (None: no length test).  An edge is reduced
    when it is a candidate and its support is above 0; masked_scores holds the scores with a NaN on every reduced edge, which
    every decoder of this module treats as no candidate.  The strict < keeps two edges from removing each other and never reduces
    a node's candidate out-edge of uniquely smallest prefix.
    `graph`: an AssemblyGraph on a HIP device; `scores`, `prefix_length`, `y` (optional, for stats.reduced_label1): [E] in edge-id
    order.  One host synchronisation: the read of the record."""
    from .graph import as_assembly_graph
    _reduce_args("transitive_support", True, fuzz)
    g = as_assembly_graph(graph)
    dev = g.device
    if dev.type != "cuda":
        raise _lib.GnmError("transitive_support: the graph must be on a HIP device (no CPU fallback)")
    pl = torch.as_tensor(prefix_length).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    support, masked, rec = _reduce_launch(g, scores, pl, y, min_logit, fuzz)
    return TransitiveSupport(support, masked, ReduceStats.from_record(rec))


def _cover_prologue(who: str, graph, scores, prefix_length, read_length, y, min_logit, reduce_transitive, fuzz):
    """What the two cover decoders do before they choose links: the argument and device checks, prefix_length / read_length as
    int64 on the graph's device, and the optional reduction.  Returns (g, scores, pl, rl, red): the AssemblyGraph, the scores the
    decoder runs on (transitive_support's masked_scores when reducing), and the reduction's record on the device or None."""
    from .graph import as_assembly_graph
    _reduce_args(who, reduce_transitive, fuzz)
    g = as_assembly_graph(graph)
    dev = g.device
    if dev.type != "cuda":
        raise _lib.GnmError(f"{who}: the graph must be on a HIP device (no CPU fallback)")
    n, E = g.num_nodes(), g.num_edges()
    pl = torch.as_tensor(prefix_length).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    rl = torch.as_tensor(read_length).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    if pl.numel() != E or rl.numel() != n or scores.numel() != E:
        raise ValueError("scores / prefix_length need one entry per edge, read_length one per node")
    red = None
    if reduce_transitive:
        _, scores, red = _reduce_launch(g, scores, pl, y, min_logit, fuzz)
    return g, scores, pl, rl, red


def _links_to_contigs(g, link_succ, link_pred, scores, y, pl, rl, min_logit, red) -> BogContigs:
    """The contigs of the links (link_succ, link_pred) -- int32 [n] edge ids on the graph's device, -1: none -- by
    gnm_bog_contigs; the read of its record is the one synchronisation.  red: _cover_prologue's."""
    from . import engine
    dev, n = g.device, g.num_nodes()
    with torch.cuda.device(dev):
        i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)  # noqa: E731
        src, dst = g.edges()
        rec = torch.zeros(engine.BOG_RECORD_WORDS, dtype=torch.int64, device=dev)
        contig_ptr, walk_nodes, walk_edges, wrong = i32(n + 1), i32(n), i32(n), i32(n)
        bases = torch.empty(n, dtype=torch.int64, device=dev)
        engine.bog_contigs(src, dst, link_succ, link_pred, scores, y, pl, rl, rec, contig_ptr, walk_nodes, walk_edges, bases, wrong,
                           min_logit)
        stats = BogStats.from_record(rec)
    C = stats.contigs
    out = BogContigs(contig_ptr[:C + 1], walk_nodes, walk_edges, bases[:C], wrong[:C], stats, pl, rl)
    if red is not None:
        out.reduce_stats = ReduceStats.from_record(red)
    return out


def best_overlap_contigs(graph, scores, prefix_length, read_length, y=None, min_logit: float = float("-inf"),
                         reduce_transitive: bool = False, fuzz: Optional[int] = None) -> BogContigs:
    """Contigs of the best-overlap graph of `scores`, computed on the device: an edge is kept only when it is the top-scored
    out-edge of its source AND the top-scored in-edge of its destination (the tables of gnm_decision_stats; self loops out, ties
    to the lowest edge id, NaN lowest), not NaN and >= min_logit.  Every node then has at most one successor and one predecessor;
    a cycle is cut at its smallest node id; the paths are the contigs (gnm_bog_contigs: list ranking by pointer jumping).
    Deterministic: no sampling, no host walk, the same bits on every run.  `graph`: an AssemblyGraph on a HIP device; `scores`
    [E] in edge-id order; prefix_length [E], read_length [N] (g.edata['prefix_length'], g.ndata['read_length']); `y` [E]
    (optional): the labels, for the wrong-link counts.  One host synchronisation: the read of the 8-word record, for the contig
    count.  The two strands of a read may both be covered: see resolve_strands.
    reduce_transitive=True: transitive_support(graph, scores, prefix_length, y, min_logit, fuzz) runs first and its masked_scores
    take the place of the scores in every later call; the result additionally carries `reduce_stats` (ReduceStats).  False (the
    default) launches nothing more and `fuzz` is not read."""
    from .metrics import DecisionStats
    g, scores, pl, rl, red = _cover_prologue("best_overlap_contigs", graph, scores, prefix_length, read_length, y, min_logit,
                                             reduce_transitive, fuzz)
    dev, n = g.device, g.num_nodes()
    with torch.cuda.device(dev):
        best_succ = torch.empty(n, dtype=torch.int32, device=dev)
        best_pred = torch.empty(n, dtype=torch.int32, device=dev)
        DecisionStats(dev).add(g, scores, y, best_succ, best_pred)
    return _links_to_contigs(g, best_succ, best_pred, scores, y, pl, rl, min_logit, red)


COVER_CHECK_EVERY = 4      # rounds per chunk of greedy_cover_contigs: one read-back of the chunk's round_links


def greedy_cover_contigs(graph, scores, prefix_length, read_length, y=None, min_logit: float = float("-inf"),
                         max_rounds: Optional[int] = None, check_every: int = COVER_CHECK_EVERY, reduce_transitive: bool = False,
                         fuzz: Optional[int] = None) -> BogContigs:
    """Contigs of the greedy path cover of `scores`, computed on the device: best_overlap_contigs' mutual-best links are round one
    of a sequence (gnm_cover_rounds) in which every node that still has a free out- or in-slot chooses again among its edges whose
    other end is free too, until a round adds nothing.  The fixed point is the path cover of overlap-layout assemblers -- the edges
    by descending score, lowest edge id among equals, an edge accepted when its source has no successor and its destination no
    predecessor yet; self loops, NaN scores and scores < min_logit are no candidates.  Cycles CAN close: unlike the sequential
    textbook greedy, which refuses the closing edge with a union-find, the rounds accept it, and the existing pass of
    gnm_bog_contigs cuts every cycle at its smallest node id afterwards and counts it in stats.cycles_cut.
    The rounds run in chunks of `check_every`; after a chunk its round_links are read back -- the loop's only synchronisation --
    and the loop stops at the first round that added 0 links (rounds past it inside the chunk change nothing) or at `max_rounds`
    (None: until the fixed point; at most n + 1 rounds exist).  max_rounds=1 gives the links of best_overlap_contigs.
    Arguments and result as for best_overlap_contigs (stats.dropped is always 0: a refused edge is never proposed); the result
    additionally carries `rounds` (the rounds run, up to and including the first empty one), `round_links` (list: the links every
    one of them added) and `converged` (bool: the last of them added nothing).  The two strands of a read may both be covered:
    see resolve_strands.
    reduce_transitive=True: transitive_support(graph, scores, prefix_length, y, min_logit, fuzz) runs first and the rounds and the
    contig pass see its masked_scores, so no link jumps over a read that a two-step path of shorter prefix reaches; the result
    additionally carries `reduce_stats` (ReduceStats).  False (the default) launches nothing more and `fuzz` is not read."""
    from . import engine
    if max_rounds is not None and (not isinstance(max_rounds, (int, np.integer)) or max_rounds < 1):
        raise ValueError(f"greedy_cover_contigs: max_rounds={max_rounds!r}: expected None or an integer >= 1")
    if not isinstance(check_every, (int, np.integer)) or check_every < 1:
        raise ValueError(f"greedy_cover_contigs: check_every={check_every!r}: expected an integer >= 1")
    g, scores, pl, rl, red = _cover_prologue("greedy_cover_contigs", graph, scores, prefix_length, read_length, y, min_logit,
                                             reduce_transitive, fuzz)
    dev, n = g.device, g.num_nodes()
    limit = n + 1 if max_rounds is None else int(max_rounds)
    with torch.cuda.device(dev):
        idx = g.index(dev)
        link_succ = torch.empty(n, dtype=torch.int32, device=dev)
        link_pred = torch.empty(n, dtype=torch.int32, device=dev)
        ws = torch.empty(engine.cover_workspace_bytes(n), dtype=torch.uint8, device=dev)
        round_links, converged = [], False
        while not converged and len(round_links) < limit:
            chunk = torch.empty(min(int(check_every), limit - len(round_links)), dtype=torch.int64, device=dev)
            engine.cover_rounds(idx, scores, chunk, link_succ, link_pred, ws, len(round_links), min_logit)
            for added in chunk.cpu().tolist():                         # the loop's one synchronisation per chunk
                round_links.append(int(added))
                if added == 0:
                    converged = True
                    break
    out = _links_to_contigs(g, link_succ, link_pred, scores, y, pl, rl, min_logit, red)
    out.rounds, out.round_links, out.converged = len(round_links), round_links, converged
    out.link_succ, out.link_pred = link_succ, link_pred
    return out


@dataclass
class ResolvedContigs:
    """resolve_strands' result: the kept pieces as lists of node ids and their lengths in bases, in the order they were kept."""
    walks: List[List[int]]
    bases: List[int]


def resolve_strands(contigs: BogContigs, len_threshold: int = 20) -> ResolvedContigs:
    """One strand per read.  Nodes 2i and 2i+1 are the two strands of read i, and the best-overlap cover may hold a read on two
    different paths (typically a contig and its reverse complement).  Host side, plain numpy and Python:
      * the contigs are taken by bases descending, among equals by ascending id of their first node;
      * a contig's nodes are walked in order; a node whose read is already taken ends the current piece and belongs to none;
      * a piece of at least `len_threshold` nodes is kept and its reads are marked taken; a shorter piece is dropped and its reads
        are NOT marked;
      * a read that is already in the current piece (both strands on one path) ends the piece too; when the piece is dropped the
        node starts the next one, when it is kept the node is skipped like any taken one.
    A piece's length in bases is the sum of prefix_length over its inner links plus the read_length of its last node."""
    h = contigs.host()
    ptr, nodes, edges, pl, rl = h["contig_ptr"], h["walk_nodes"], h["walk_edges"], h["prefix_length"], h["read_length"]
    thr = max(1, int(len_threshold))
    C = ptr.size - 1
    order = sorted(range(C), key=lambda c: (-int(h["bases"][c]), c))
    taken = np.zeros(int(rl.size // 2 + 1), np.bool_)
    walks, bases = [], []

    def close(lo, hi):                       # the piece of positions [lo, hi): kept or dropped; True when kept
        if hi - lo < thr:
            return False
        piece = nodes[lo:hi]
        taken[piece >> 1] = True
        walks.append(piece.tolist())
        bases.append(int(pl[edges[lo + 1:hi]].sum()) + int(rl[piece[-1]]))
        return True

    for c in order:
        if ptr[c + 1] - ptr[c] < thr:        # no piece of it can reach the threshold
            continue
        lo, inside = int(ptr[c]), set()
        for pos in range(int(ptr[c]), int(ptr[c + 1])):
            r = int(nodes[pos]) >> 1
            if taken[r]:
                close(lo, pos)
                lo, inside = pos + 1, set()
            elif r in inside:
                kept = close(lo, pos)
                lo, inside = (pos + 1, set()) if kept else (pos, {r})
            else:
                inside.add(r)
        close(lo, int(ptr[c + 1]))
    return ResolvedContigs(walks, bases)


# ---- one strand per read on the device (gnm_resolve.hip) ----------------------------------------------------------------------------
@dataclass
class ResolveStats(RecordStats):
    """A gnm_resolve_record (include/gnm.h): contigs (given), eligible (of at least len_threshold nodes), pieces (kept), dropped
    (non-empty pieces below the threshold), nodes (on the kept pieces), serial (eligible contigs that hold both strands of a read:
    cut by one lane), invalid (positions, contig_ptr rows and order entries that failed the input check), calls."""
    contigs: int = 0
    eligible: int = 0
    pieces: int = 0
    dropped: int = 0
    nodes: int = 0
    serial: int = 0
    invalid: int = 0
    calls: int = 0


class StrandContigs(BogContigs):
    """resolve_strands_device's result: the kept pieces as a BogContigs of their own, on the device, in the order resolve_strands
    keeps them (walk_edges is -1 at every piece's first node).  `stats`: ResolveStats; `rounds`: the rounds the rule took."""

    def __init__(self, contig_ptr, walk_nodes, walk_edges, bases, wrong, stats: ResolveStats, prefix_length, read_length, rounds: int):
        super().__init__(contig_ptr, walk_nodes, walk_edges, bases, wrong, stats, prefix_length, read_length)
        self.rounds = rounds

    def resolved(self) -> ResolvedContigs:
        """The pieces in resolve_strands' own format (lists on the host), for comparison with it."""
        return ResolvedContigs(self.walks(), [int(b) for b in self.host()["bases"].tolist()])


RESOLVE_CHECK_EVERY = 4    # rounds per chunk of resolve_strands_device: one read-back of the chunk's undecided counts


def resolve_strands_device(contigs: BogContigs, len_threshold: int = 20, y=None, check_every: int = RESOLVE_CHECK_EVERY
                           ) -> StrandContigs:
    """resolve_strands on the device: the same pieces, in the same order, with the same bases -- as a StrandContigs, so that
    contig_sequences, junction_identity, .walks(), .n50() and .longest() take the result where it is.
    The rule runs in rounds (gnm_resolve_rounds): the contigs are ordered by a stable descending sort of `bases` (ascending contig
    index among equals, resolve_strands' key); a contig is cut once every contig that holds the other strand of one of its reads
    and comes earlier in that order is finished, so a contig and its reverse complement take two rounds and all contigs that share no
    read are cut side by side.  A contig that holds both strands of some read is cut by one lane (stats.serial counts them).
    `contigs`: a BogContigs on a HIP device whose nodes occur once each (a path cover); `y` [E] (optional): the labels, for `wrong`.
    The rounds run in chunks of `check_every`; the synchronisations are one read of a chunk's counts per chunk and the read of the
    record.  A node or edge id out of range, or a node listed twice, raises GnmError with `.record` (ResolveStats) set; nothing is
    written then.  No contig, or none of len_threshold nodes, gives zero-length tensors.
    The result's tensors are leading slices of buffers laid out for all P input positions before the kept pieces are counted, so
    the result keeps 24 bytes per INPUT position alive (36 MB at 1.5 M positions) however few nodes it keeps; `.clone()` the five
    tensors to hold on to a small result for long."""
    from . import engine
    if not isinstance(check_every, (int, np.integer)) or isinstance(check_every, bool) or check_every < 1:
        raise ValueError(f"resolve_strands_device: check_every={check_every!r}: expected an integer >= 1")
    if not isinstance(contigs, BogContigs):
        raise TypeError("resolve_strands_device: contigs must be a BogContigs")
    dev = contigs.walk_nodes.device
    if dev.type != "cuda":
        raise _lib.GnmError("resolve_strands_device: the contigs must be on a HIP device (no CPU fallback; resolve_strands is the "
                            "host route)")
    thr = max(1, int(len_threshold))
    i32c = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
    C = len(contigs)
    contig_ptr, walk_nodes = i32c(contigs.contig_ptr[:C + 1]), i32c(contigs.walk_nodes)
    P = int(walk_nodes.numel())
    walk_edges = i32c(contigs.walk_edges[:P])
    pl = contigs.prefix_length.to(device=dev, dtype=torch.int64).contiguous()
    rl = contigs.read_length.to(device=dev, dtype=torch.int64).contiguous()
    n, E = int(rl.numel()), int(pl.numel())
    with torch.cuda.device(dev):
        order = i32c(torch.sort(contigs.bases[:C].to(dev), descending=True, stable=True).indices)
        cover = (contig_ptr, walk_nodes, walk_edges, order)
        rec = torch.zeros(engine.RESOLVE_RECORD_WORDS, dtype=torch.int64, device=dev)
        ws = torch.empty(engine.resolve_workspace_bytes(C, P, n), dtype=torch.uint8, device=dev)
        engine.resolve_prepare(cover, n, E, thr, rec, ws)
        rounds, left = 0, 1
        while left > 0:
            if rounds > C:                                             # every round finishes a contig: cannot happen
                raise _lib.GnmError(f"resolve_strands_device: {left} contigs still undecided after {rounds} rounds")
            chunk = torch.empty(int(check_every), dtype=torch.int64, device=dev)
            engine.resolve_rounds(cover, n, E, thr, chunk, rec, ws, rounds)
            for left in chunk.cpu().tolist():                          # the loop's one synchronisation per chunk
                rounds += 1
                if left <= 0:
                    break
        if left < 0:
            stats = ResolveStats.from_record(rec)
            err = _lib.GnmError(f"resolve_strands_device: {stats.invalid} walk positions or order entries name a node or edge that "
                                f"is out of range or listed twice (cover of {C} contigs and {P} positions, graph of {n} nodes and "
                                f"{E} edges)")
            err.record = stats
            raise err
        out_ptr = torch.empty(P + 1, dtype=torch.int32, device=dev)
        out_nodes, out_edges, out_wrong = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
        out_bases = torch.empty(P, dtype=torch.int64, device=dev)
        engine.resolve_layout(cover, n, E, thr, pl, rl, y if y is None else y.to(dev), rec, out_ptr, out_nodes, out_edges, out_bases,
                              out_wrong, ws)
        stats = ResolveStats.from_record(rec)
    K, N = stats.pieces, stats.nodes
    return StrandContigs(out_ptr[:K + 1], out_nodes[:N], out_edges[:N], out_bases[:K], out_wrong[:K], stats, pl, rl, rounds)


# ---- contig sequences: walks + a packed read store -> bases, FASTA, N50 / NG50 (evaluate.py) ------------------------------------------
# evaluate.py:9-33, retyped: the chromosome lengths quick_evaluation divides by
CHR_LENGTHS = {
    "chr1": 248387328, "chr2": 242696752, "chr3": 201105948, "chr4": 193574945, "chr5": 182045439, "chr6": 172126628,
    "chr7": 160567428, "chr8": 146259331, "chr9": 150617247, "chr10": 134758134, "chr11": 135127769, "chr12": 133324548,
    "chr13": 113566686, "chr14": 101161492, "chr15": 99753195, "chr16": 96330374, "chr17": 84276897, "chr18": 80542538,
    "chr19": 61707364, "chr20": 66210255, "chr21": 45090682, "chr22": 51324926, "chrX": 154259566,
}


def _ref_length(ref_length) -> int:
    return int(CHR_LENGTHS[ref_length]) if isinstance(ref_length, str) else int(ref_length)


def _nx(lengths, target) -> int:
    """The length at which the running sum of the lengths, longest first, reaches `target`; -1 when it never does."""
    run = 0
    for v in sorted((int(v) for v in np.asarray(lengths).reshape(-1)), reverse=True):
        run += v
        if run >= target:
            return v
    return -1


def ng50(lengths, ref_length) -> int:
    """calculate_NG50 (evaluate.py:76-92): the contig length at which the lengths, longest first, sum to half of `ref_length` (a
    number of bases or a key of CHR_LENGTHS); -1 when they never do or ref_length <= 0."""
    ref = _ref_length(ref_length)
    return _nx(lengths, ref / 2) if ref > 0 else -1


def quick_evaluation(lengths, ref_length):
    """quick_evaluation (evaluate.py:95-104) on contig lengths: (contigs, longest, reconstructed, N50, NG50); reconstructed is the
    fraction sum(lengths) / ref_length, N50 / NG50 are -1 where the reference's loops fall through (no contig; less than half of
    the reference covered).  Unlike the reference, no contig at all gives longest = 0 instead of raising."""
    a = [int(v) for v in np.asarray(lengths).reshape(-1)]
    ref = _ref_length(ref_length)
    return len(a), max(a, default=0), sum(a) / ref, _nx(a, sum(a) / 2), ng50(a, ref)


@dataclass
class SeqStats(RecordStats):
    """A gnm_seq_record (include/gnm.h): contigs, pieces (walk positions), bases, clamped (pieces whose prefix_length was below 0
    or above the read's length), empty (valid pieces of 0 bases), reverse (valid pieces of odd nodes), invalid (positions whose
    node, read or edge is out of range: 0 bases, nothing read), calls."""
    contigs: int = 0
    pieces: int = 0
    bases: int = 0
    clamped: int = 0
    empty: int = 0
    reverse: int = 0
    invalid: int = 0
    calls: int = 0


class ContigSequences:
    """The bases of a set of contigs, back to back: contig c is bases[contig_ptr[c] : contig_ptr[c+1]], ASCII letters of
    "=ACMGRSVTWYHKDBN" (uint8; on the device when contig_sequences made it), contig_ptr int64 [C+1].  `record`: SeqStats.
    `lengths` (numpy int64 [C]) and the host copy of the bases are made once, on first use."""

    def __init__(self, bases, contig_ptr, record: Optional[SeqStats] = None):
        as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dt)  # noqa: E731
        self.bases, self.contig_ptr = as_t(bases, torch.uint8), as_t(contig_ptr, torch.int64)
        self.record = record if record is not None else SeqStats()
        self._ptr = self._host = None

    def __len__(self):
        return int(self.contig_ptr.numel()) - 1

    def _hptr(self) -> np.ndarray:
        if self._ptr is None:
            self._ptr = self.contig_ptr.cpu().numpy()
        return self._ptr

    def _hbases(self) -> np.ndarray:
        if self._host is None:
            self._host = self.bases.cpu().numpy()
        return self._host

    @property
    def lengths(self) -> np.ndarray:
        return np.diff(self._hptr())

    def sequence(self, c: int) -> str:
        p = self._hptr()
        return self._hbases()[p[c]:p[c + 1]].tobytes().decode("ascii")

    def write_fasta(self, path, line_width: int = 60) -> None:
        """`>contig_{c+1} length={n}` and the bases in lines of `line_width`: the records walk_to_sequence builds (evaluate.py:43-45)
        as Biopython's SeqIO.write(..., 'fasta') lays them out.  A contig of no bases is its header line alone."""
        w = int(line_width)
        if w < 1:
            raise ValueError("write_fasta: line_width must be at least 1")
        p, b = self._hptr(), self._hbases()
        with open(path, "wb") as fh:
            for c in range(len(self)):
                seq = b[p[c]:p[c + 1]]
                fh.write(f">contig_{c + 1} length={seq.size}\n".encode())
                full = seq.size // w
                if full:
                    rows = np.empty((full, w + 1), np.uint8)
                    rows[:, :w] = seq[:full * w].reshape(full, w)
                    rows[:, w] = 10
                    fh.write(rows.tobytes())
                if seq.size > full * w:
                    fh.write(seq[full * w:].tobytes() + b"\n")


def walk_edge_ids(graph: DecodeGraph, walks):
    """(contig_ptr [C+1], walk_nodes [P], walk_edges [P]) int32 numpy arrays for walks given as lists of node ids
    (gnm_decode_walk_edges): walk_edges[p] is the id of the edge from position p-1 to p -- the lowest id among parallel edges --
    and -1 at a contig's first node.  A step that is not an edge of `graph` raises ValueError naming it."""
    lib = _lib.load()
    ptr = np.zeros(len(walks) + 1, np.int64)
    np.cumsum([len(w) for w in walks], out=ptr[1:])
    if ptr[-1] >= 2 ** 31 - 1:
        raise ValueError("walk_edge_ids: the walks hold 2^31 - 1 positions or more")
    contig_ptr = ptr.astype(np.int32)
    nodes = np.ascontiguousarray(np.concatenate([np.asarray(w, np.int64).reshape(-1) for w in walks] + [np.zeros(0, np.int64)]))
    if nodes.size and (nodes.min() < 0 or nodes.max() >= graph.n):
        bad = int(nodes[(nodes < 0) | (nodes >= graph.n)][0])
        raise ValueError(f"walk_edge_ids: node {bad} outside [0, {graph.n})")
    walk_nodes = nodes.astype(np.int32)
    edges = np.full(walk_nodes.size, -1, np.int32)
    bad = np.zeros(4, np.int64)
    rc = lib.gnm_decode_walk_edges(_p(graph.src), _p(graph.dst), graph.n, graph.src.size, _p(graph.succ[0]), len(walks),
                                   _p(contig_ptr), _p(walk_nodes), _p(edges), _p(bad))
    if rc == -2:
        raise ValueError(lib.gnm_last_error().decode(errors="replace"))
    _lib.check(rc, "gnm_decode_walk_edges")
    return contig_ptr, walk_nodes, edges


def _as_decode_graph(graph) -> DecodeGraph:
    if isinstance(graph, DecodeGraph):
        return graph
    src, dst = graph.edges()
    return DecodeGraph(src.cpu().numpy(), dst.cpu().numpy(), graph.num_nodes())


def _default_prefix_length(walks, graph, prefix_length):
    """prefix_length as given; else graph.edata['prefix_length']; else the one a BogContigs was built with; else None."""
    if prefix_length is None:
        prefix_length = getattr(graph, "edata", {}).get("prefix_length")
    if prefix_length is None and isinstance(walks, BogContigs):
        prefix_length = walks.prefix_length
    return prefix_length


def _walks_csr(walks, graph):
    """(contig_ptr [C+1], walk_nodes [P], walk_edges [P]) of `walks` as int32 tensors: the device CSR of a BogContigs as it is, or
    host tensors for lists of node ids, whose edge ids are looked up on the host (walk_edge_ids) over `graph`.  The caller moves
    what it uses to its device and integer width."""
    if isinstance(walks, BogContigs):
        return walks.contig_ptr, walks.walk_nodes, walks.walk_edges
    return tuple(torch.from_numpy(a) for a in walk_edge_ids(_as_decode_graph(graph), walks))


def contig_sequences(walks, graph, reads, prefix_length=None, read_length=None) -> ContigSequences:
    """The sequences of `walks` on the device: evaluate.walk_to_sequence (evaluate.py:36-47) over a packed ReadStore.

    walks: a BogContigs -- its device CSR is used as it is, no host round trip -- or a list of lists of node ids (get_contigs,
    get_contigs_device, ResolvedContigs.walks), whose edge ids are looked up on the host (walk_edge_ids) and uploaded once.
    graph: the AssemblyGraph (or, for lists, a DecodeGraph).  reads: a ReadStore on a HIP device; node v is read v >> 1, an odd
    v its reverse complement.  prefix_length [E]: default graph.edata['prefix_length'] (a BogContigs falls back on the one it
    was built with).  read_length [N] (optional): checked against the store, a disagreement raises (one more synchronisation).

    Position p of a contig contributes the first prefix_length[edge to p+1] bases of its node's strand, the last position the
    whole read.  DIFFERENT from the reference on purpose: a prefix below 0 or above the read's length is clamped (a Python slice
    would take a negative prefix from the read's END) and counted in record.clamped.  A node, read or edge id out of range raises
    GnmError (its .record holds the counts); nothing is emitted then.  One host synchronisation: the read of the record, which
    sizes the output."""
    from . import engine
    from .reads import ReadStore
    if not isinstance(reads, ReadStore):
        raise TypeError("contig_sequences: reads must be a ReadStore")
    dev = reads.device
    if dev.type != "cuda":
        raise _lib.GnmError("contig_sequences: the ReadStore must be on a HIP device (no CPU fallback; ReadStore.sequence is the "
                            "host route)")
    n = int(graph.n if isinstance(graph, DecodeGraph) else graph.num_nodes())
    prefix_length = _default_prefix_length(walks, graph, prefix_length)
    if prefix_length is None:
        raise ValueError("contig_sequences: no prefix_length given and the graph has no edata['prefix_length']")
    pl = torch.as_tensor(prefix_length).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    if not isinstance(walks, BogContigs):
        graph = _as_decode_graph(graph)
        if pl.numel() != graph.src.size:
            raise ValueError("contig_sequences: prefix_length needs one entry per edge")
    contig_ptr, walk_nodes, walk_edges = (t.to(device=dev, dtype=torch.int32).contiguous() for t in _walks_csr(walks, graph))
    with torch.cuda.device(dev):
        if read_length is not None:
            rl = torch.as_tensor(read_length).reshape(-1).to(device=dev, dtype=torch.int64)
            if rl.numel() != n or (n + 1) // 2 > len(reads):
                raise ValueError(f"contig_sequences: read_length holds {rl.numel()} entries and the store {len(reads)} reads for "
                                 f"{n} nodes")
            diff = rl != reads.length[torch.arange(n, device=dev) >> 1]
            if bool(diff.any()):
                v = int(diff.nonzero()[0])
                raise ValueError(f"contig_sequences: read_length[{v}] = {int(rl[v])}, the store holds {int(reads.length[v >> 1])} "
                                 f"bases for read {v >> 1}")
        C, P = int(contig_ptr.numel()) - 1, int(walk_nodes.numel())
        i64 = lambda m: torch.empty(m, dtype=torch.int64, device=dev)  # noqa: E731
        rec = torch.zeros(engine.SEQ_RECORD_WORDS, dtype=torch.int64, device=dev)
        piece_len, piece_off, base_ptr = i64(P), i64(P + 1), i64(C + 1)
        engine.seq_layout(contig_ptr, walk_nodes, walk_edges, pl, n, reads.base_off, reads.length, reads.packed, rec, piece_len,
                          piece_off, base_ptr)
        stats = SeqStats.from_record(rec)                              # the one synchronisation
        if stats.invalid:
            err = _lib.GnmError(f"contig_sequences: {stats.invalid} of {stats.pieces} walk positions name a node, read or edge "
                                f"that is out of range (graph of {n} nodes and {pl.numel()} edges, store of {len(reads)} reads)")
            err.record = stats
            raise err
        out = torch.empty((stats.bases + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        engine.seq_emit(walk_nodes, piece_off, n, reads.base_off, reads.length, reads.packed, stats.bases, out)
    seqs = ContigSequences(out[:stats.bases], base_ptr, stats)
    seqs.piece_len, seqs.piece_off = piece_len, piece_off
    return seqs


@dataclass
class JunctionIdentity:
    """junction_identity's result, on the graph's device, one entry per contig: junctions int64 [C] (the contig's nodes - 1),
    edit_distance int64 [C] (the sum of the junction edges' edit distances; an exceeded junction adds max_errors + 1, an invalid
    one nothing), exceeded int64 [C] (junctions whose distance exceeds max_errors).  `features`: the per-edge OverlapFeatures
    the sums were gathered from."""
    junctions: torch.Tensor
    edit_distance: torch.Tensor
    exceeded: torch.Tensor
    features: object


def junction_identity(contigs, graph, reads, max_errors: int = 255, prefix_length=None) -> JunctionIdentity:
    """How many of the junctions contig_sequences glues together agree: features.overlap_features(graph, reads) gathered over
    the walk edges of `contigs` -- a BogContigs, or lists of node ids whose edge ids are looked up on the host (walk_edge_ids).
    graph: the AssemblyGraph on a HIP device; reads: a ReadStore on that device.  Torch indexing only, no kernel of its own."""
    from . import features
    f = features.overlap_features(graph, reads, _default_prefix_length(contigs, graph, prefix_length), max_errors)
    dev = graph.device
    contig_ptr, _, walk_edges = _walks_csr(contigs, graph)
    contig_ptr, walk_edges = contig_ptr.to(dev).long(), walk_edges.to(dev).long()
    C, P = int(contig_ptr.numel()) - 1, int(walk_edges.numel())
    contig = torch.repeat_interleave(torch.arange(C, device=dev), contig_ptr[1:] - contig_ptr[:-1], output_size=P)
    first = torch.zeros(P, dtype=torch.bool, device=dev)
    first[contig_ptr[:-1][contig_ptr[:-1] < P]] = True
    junction = ~first & (walk_edges >= 0)
    e = walk_edges.clamp(min=0)
    zeros = lambda: torch.zeros(C, dtype=torch.int64, device=dev)  # noqa: E731
    dist = f.edit_distance.long()[e] if P else zeros()[:0]
    junctions = zeros().index_add_(0, contig, junction.long())
    edits = zeros().index_add_(0, contig, torch.where(junction, dist.clamp(min=0), torch.zeros_like(dist)))
    exceeded = zeros().index_add_(0, contig, (junction & (dist > int(max_errors))).long())
    return JunctionIdentity(junctions, edits, exceeded, f)


def infer_contigs(model, graph, e, pe, prefix_length, read_length, nb_paths: int = 50, len_threshold: int = 20,
                  device_sampling: bool = False, decision_report: bool = False, decoder: str = "greedy", reads=None,
                  reduce_transitive: bool = False, fuzz: Optional[int] = None, junction_report: bool = False,
                  device_resolve: bool = False):
    """The per-graph body of inference.inference (inference.py:444-490): logits of the whole graph under
    no_grad in eval mode, stored by edge id, then greedy decode.  Returns (scores [E], walks).
    device_sampling=True: the logits stay on the device for `get_contigs_device` (same distribution of start edges,
    other random numbers); False is `get_contigs` with the reference's seeded draws.
    decision_report=True: returns (scores, walks, report) with report = decision_table(graph, scores, graph.edata.get('y')) --
    the per-node best successor / predecessor edges and their counts, taken before the walks, which it does not change.
    decoder="best_overlap": the walks are resolve_strands(best_overlap_contigs(graph, scores, ...), len_threshold).walks --
    deterministic, computed on the device, no sampling (nb_paths and device_sampling are not used).
    decoder="greedy_cover": the same over greedy_cover_contigs, the mutual-best links iterated to the greedy path cover.
    reads: a ReadStore on the graph's device: contig_sequences(walks, graph, reads, prefix_length) -- the walks' bases, ready for
    ContigSequences.write_fasta (inference.py:497-501) -- is appended as the LAST element of the returned tuple.
    reduce_transitive, fuzz: handed to best_overlap_contigs / greedy_cover_contigs (the string-graph reduction ahead of the cover).
    The sampled decoder refuses reduce_transitive=True: its walks already absorb the nodes they jump over.
    junction_report=True (needs reads): junction_identity(walks, graph, reads, prefix_length=prefix_length) -- per contig the
    junctions, their summed edit distance and how many exceed the band -- is appended behind the sequences, as the LAST element.
    device_resolve=True (cover decoders only): the strand rule runs on the device (resolve_strands_device): the walks are its
    .walks() -- the same lists -- and, with reads, the sequences and the junction report are computed from its device CSR directly,
    without looking the edge ids up on the host again.  False (the default) is resolve_strands on the host."""
    if not isinstance(device_resolve, (bool, np.bool_)):
        raise ValueError(f"infer_contigs: device_resolve={device_resolve!r}: expected True or False")
    if device_resolve and decoder == "greedy":
        raise ValueError("infer_contigs: device_resolve=True with decoder='greedy': the sampled walks keep one strand per read "
                         "themselves; the strand rule belongs to decoder='best_overlap' and 'greedy_cover'")
    if junction_report and reads is None:
        raise ValueError("infer_contigs: junction_report=True needs reads (a ReadStore on the graph's device)")
    if decoder not in ("greedy", "best_overlap", "greedy_cover"):
        raise ValueError(f"decoder {decoder!r}: expected 'greedy', 'best_overlap' or 'greedy_cover'")
    _reduce_args("infer_contigs", reduce_transitive, fuzz)
    if reduce_transitive and decoder == "greedy":
        raise ValueError("infer_contigs: reduce_transitive=True with decoder='greedy': the sampled walks already absorb the nodes "
                         "they jump over; the reduction belongs to decoder='best_overlap' and 'greedy_cover'")
    model.eval()
    with torch.no_grad():
        scores = model(graph, None, e, pe).squeeze(-1)                 # inference.py:453-454
    report = decision_table(graph, scores, getattr(graph, "edata", {}).get("y")) if decision_report else None
    if decoder in ("best_overlap", "greedy_cover"):
        cover = best_overlap_contigs if decoder == "best_overlap" else greedy_cover_contigs
        extra = dict(reduce_transitive=True, fuzz=fuzz) if reduce_transitive else {}
        labels = getattr(graph, "edata", {}).get("y")
        covered = cover(graph, scores, prefix_length, read_length, labels, **extra)
        if device_resolve:
            on_device = resolve_strands_device(covered, len_threshold, labels)
            walks = on_device.walks()
        else:
            walks = resolve_strands(covered, len_threshold).walks
        walk_graph = graph
    else:
        walk_graph = _as_decode_graph(graph)                           # built once: the walks and contig_sequences share it
        sampled = get_contigs_device if device_sampling else get_contigs
        walks = sampled(walk_graph, scores, prefix_length, read_length, nb_paths, len_threshold)
    result = (scores, walks, report) if decision_report else (scores, walks)
    if reads is not None:
        laid_out = on_device if device_resolve else walks              # the device CSR as it is, or lists of node ids
        result += (contig_sequences(laid_out, walk_graph, reads, prefix_length),)
        if junction_report:
            result += (junction_identity(laid_out, graph, reads, prefix_length=prefix_length),)
    return result
