"""The overlap graph FROM THE READS (include/gnm.h, "overlap graph"): what the reference obtains from an external overlapper
(graph_dataset.py:120) and parses in graph_parser.py.  An all-versus-all overlapper for accurate long reads (errors of about 1 %)
by exact minimizer matches: sketch -> stable sort by hash -> seed hits -> sort by diagonal, stable sort by read pair -> chains ->
(optionally) the banded alignment of features.overlap_features -> an AssemblyGraph in the edge order of graph_parser.py:297.

Three HIP stages (csrc/gnm_overlap.hip) on the store's device; a CPU store runs the host entries over the same header.  The sorts
between them are stable torch.sort calls.  By default all hits of the data set are resident at once: `stats.hits` says how many
(DESIGN.md states the bytes per hit).  find_overlaps(max_hits=m) bounds them: a hit's key is lower read << 32 | ..., so the hits
whose lower read lies in a range of reads hold whole chain groups, and consecutive ranges (plan_chunks), sorted and chained one
after the other, give the unchunked arrays element for element; the sketch and the candidate edges stay resident, the hits do not."""
from __future__ import annotations

import bisect
from dataclasses import dataclass

import torch

from . import _lib, engine
from .engine import RecordStats
from .graph import AssemblyGraph
from .reads import ReadStore

__all__ = ["find_overlaps", "plan_chunks", "sketch", "OverlapGraph", "OverlapStats", "Sketch"]


@dataclass
class OverlapStats(RecordStats):
    """A gnm_overlap_record (include/gnm.h): reads; kmers_valid (k-mers that are neither palindromic nor hold a non-ACGT code);
    minimizers; runs of equal hash, of which skipped_runs (skipped_entries entries) exceed max_occ; hits and same_read pairs;
    groups = few_hits + short + contained_groups + links; calls."""
    reads: int = 0
    kmers_valid: int = 0
    minimizers: int = 0
    runs: int = 0
    skipped_runs: int = 0
    skipped_entries: int = 0
    hits: int = 0
    same_read: int = 0
    groups: int = 0
    few_hits: int = 0
    short: int = 0
    contained_groups: int = 0
    links: int = 0
    calls: int = 0


@dataclass
class Sketch:
    """The minimizers of a store, ordered by read and position: hash int64 (the 64-bit hash's bit pattern), read int32, pos int32
    (of the + strand), strand uint8 (1: the canonical k-mer is the reverse complement); record: the int64 record tensor."""
    hash: torch.Tensor
    read: torch.Tensor
    pos: torch.Tensor
    strand: torch.Tensor
    record: torch.Tensor

    def __len__(self):
        return int(self.hash.numel())


@dataclass
class OverlapGraph:
    """find_overlaps' result.  graph: an AssemblyGraph on the store's device over N = 2 R nodes (node 2r is read r, 2r + 1 its
    reverse complement) whose edata carries prefix_length, overlap_length (int64), twin (int64: the id of the mirror edge) and,
    with verify=True, overlap_similarity (fp32); read_length int64 [N]; contained bool [R]; stats: OverlapStats; sketch_size,
    hit_count: the minimizers and the seed hits of the data set; record: the int64 record tensor on the device; exceeded_pairs:
    the twin pairs the verification dropped; chunks: the read ranges whose hits were formed (1 without max_hits); peak_hits: the
    most hits resident at once (hit_count without max_hits); oversize_chunks: single reads with more hits than max_hits."""
    graph: AssemblyGraph
    read_length: torch.Tensor
    contained: torch.Tensor
    stats: OverlapStats
    sketch_size: int
    hit_count: int
    record: torch.Tensor
    exceeded_pairs: int = 0
    chunks: int = 1
    peak_hits: int = 0
    oversize_chunks: int = 0


def _store(reads, fn):
    if not isinstance(reads, ReadStore):
        raise TypeError(f"{fn}: reads must be a ReadStore")
    if len(reads) and int(reads.length.max()) >= 2 ** 31 - 1:
        raise ValueError(f"{fn}: a read of 2^31 - 1 bases or more")
    return reads


def _record(dev):
    return torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=dev)


def sketch(reads: ReadStore, k: int = 21, w: int = 25, threads: int = 1) -> Sketch:
    """The (w, k) minimizers of every read's + strand, canonical k-mers hashed by the murmur3 finaliser (include/gnm.h, stage 1),
    on the store's device.  k in [8, 31], w in [1, 64]."""
    _store(reads, "sketch")
    rec = _record(reads.device)
    return Sketch(*engine.sketch(reads.base_off, reads.length, reads.packed, k, w, rec, threads), rec)


def _align(src, dst, prefix, n, reads, max_errors, threads):
    """(similarity fp32 [E], exceeded bool [E]) of the candidate edges: features.overlap_features on the device.  That function has
    no CPU route, so a CPU store calls the host twin of its kernel (gnm_overlap_align_host: the same header, the same `exceeded`
    rule, edit distance > max_errors)."""
    dev, E = reads.device, int(src.numel())
    if dev.type != "cpu":
        from .features import overlap_features
        f = overlap_features(AssemblyGraph.from_tensors(src, dst, n), reads, prefix, max_errors)
        return f.overlap_similarity, f.exceeded
    dist = torch.empty(E, dtype=torch.int32, device=dev)
    olen = torch.empty(E, dtype=torch.int64, device=dev)
    sim = torch.empty(E, dtype=torch.float32, device=dev)
    rec = torch.zeros(engine.ALIGN_RECORD_WORDS, dtype=torch.int64, device=dev)
    engine.overlap_align_host(src, dst, prefix, n, reads.base_off, reads.length, reads.packed, max_errors, dist, olen, sim, rec, threads)
    return sim, dist > int(max_errors)


def plan_chunks(lower_hits: torch.Tensor, max_hits: int):
    """The read ranges of the chunked route: (bounds int64 [C + 1], chunk_hits int64 [C]), CPU tensors.  lower_hits int64 [R]:
    the hits per lower read id (engine.seed_pairs_lower_hits), on any device.  Chunk c is reads [bounds[c], bounds[c + 1]): taken
    greedily from read 0, the longest run of consecutive reads whose hits sum to at most max_hits; reads without hits join the
    chunk in progress; a read with more hits than max_hits is a chunk of its own (chunk_hits[c] > max_hits marks it: an oversize
    chunk, not an error).  bounds ascends strictly from 0 to R.  One prefix sum read back, then a bisection per chunk on the host."""
    max_hits = engine._int_in("plan_chunks", "max_hits", max_hits, 1, 2 ** 62)
    if not torch.is_tensor(lower_hits) or lower_hits.dtype != torch.int64 or lower_hits.dim() != 1:
        raise ValueError("plan_chunks: lower_hits must be an int64 [R] tensor")
    R = int(lower_hits.numel())
    pre = [0] + torch.cumsum(lower_hits.cpu(), 0).tolist()
    bounds, s = [0], 0
    while s < R:
        e = bisect.bisect_right(pre, pre[s] + max_hits, s) - 1                 # the last e with pre[e] - pre[s] <= max_hits
        s = max(e, s + 1)                                                      # e == s: read s alone is over the budget
        bounds.append(s)
    sums = [pre[e] - pre[s] for s, e in zip(bounds[:-1], bounds[1:])]
    return torch.tensor(bounds, dtype=torch.int64), torch.tensor(sums, dtype=torch.int64)


def _candidates(hits, reads, band, min_hits, min_overlap, max_errors, verify, rec, threads):
    """The candidate edges of a set of hits that holds whole chain groups: the two stable sorts, the chains, the valid slots and,
    with verify, their alignment.  (src, dst, prefix, ovl, sim or None, exceeded or None, contained uint8 [R]); twins stay
    adjacent: 2 j, 2 j + 1.  hits: the LIST [key, diag], which is emptied: this function owns the hit arrays, the largest of the
    call, and lets each go as soon as its sorted form exists; none of them outlives the chains."""
    diag, key = hits.pop(), hits.pop()
    diag, order = torch.sort(diag, stable=True)
    key = key[order]
    del order
    key, order2 = torch.sort(key, stable=True)                         # groups (a, b, rel), diagonals ascending inside
    diag = diag[order2].contiguous()
    del order2
    src, dst, prefix, ovl, valid, contained = engine.chain_pairs(key, diag, reads.length, band, min_hits, min_overlap, rec, threads)
    del key, diag
    keep = valid.bool()
    src, dst, prefix, ovl = src[keep], dst[keep], prefix[keep], ovl[keep]
    sim = exceeded = None
    if verify:
        sim, exceeded = _align(src.contiguous(), dst.contiguous(), prefix.contiguous(), 2 * len(reads), reads, max_errors, threads)
    return src, dst, prefix, ovl, sim, exceeded, contained


def find_overlaps(reads: ReadStore, k: int = 21, w: int = 25, max_occ: int = 64, min_hits: int = 4, band: int = 32,
                  min_overlap: int = 500, max_errors: int = 255, verify: bool = True, drop_contained: bool = True,
                  threads: int = 1, max_hits=None) -> OverlapGraph:
    """All-versus-all overlaps of the reads of a store as an assembly graph, on the store's device (include/gnm.h, "overlap
    graph").  k, w: the minimizer scheme; max_occ: a minimizer that occurs more often seeds nothing; a pair of strands needs
    min_hits seed hits whose diagonals lie within `band` of each other; an overlap shorter than min_overlap bases is no edge.
    verify: the candidate edges are aligned (features.overlap_features' rule, at most max_errors edits); a twin pair is dropped when
    EITHER twin exceeds max_errors, and edata['overlap_similarity'] is the alignment's identity.  Without verify the graph carries
    no overlap_similarity (prepare_graph(graph, reads=store) then fills it).  drop_contained: edges that touch a contained read
    are dropped.  Edge ids are src-major (graph_parser.py:297).  threads: host threads of the CPU route.
    max_hits: None, all seed hits resident at once; an integer >= 1, the hits are formed, sorted, chained and verified in chunks
    of consecutive lower read ids of at most max_hits hits each (plan_chunks; a single read with more is a chunk of its own), and
    only the sketch and the candidate edges stay resident between chunks.  The result is the same in every bit.  max_hits counts
    hits, not bytes (about 55 to 70 bytes per hit, measured at one size).
    The defaults are starting points; nobody has measured an optimum for any of them."""
    _store(reads, "find_overlaps")
    for name, v in (("verify", verify), ("drop_contained", drop_contained)):
        if not isinstance(v, bool):
            raise ValueError(f"find_overlaps: {name}={v!r}: expected True or False")
    if max_hits is not None:
        max_hits = engine._int_in("find_overlaps", "max_hits", max_hits, 1, 2 ** 62)
    dev, R = reads.device, len(reads)
    rec = _record(dev)
    h, rd, ps, st = engine.sketch(reads.base_off, reads.length, reads.packed, k, w, rec, threads)
    h, order = torch.sort(h, stable=True)                              # runs of equal hash; inside a run by (read, pos)
    rd, ps, st = rd[order].contiguous(), ps[order].contiguous(), st[order].contiguous()
    del order
    sketch_size = int(h.numel())
    chain = (reads, band, min_hits, min_overlap, max_errors, verify, rec, threads)
    if max_hits is None:
        hits = list(engine.seed_pairs(h, rd, ps, st, reads.length, k, max_occ, rec, threads))
        del h, rd, ps, st                                              # the sketch has done its work on this route
        hit_count = peak_hits = int(hits[0].numel())
        chunks, oversize = 1, 0
        src, dst, prefix, ovl, sim, exceeded, contained = _candidates(hits, *chain)
        contained = contained.bool()
    else:
        lower = engine.seed_pairs_lower_hits(h, rd, R, max_occ, torch.zeros(R, dtype=torch.int64, device=dev), rec, threads)
        bounds, chunk_hits = plan_chunks(lower, max_hits)
        hit_count, peak_hits, chunks = int(chunk_hits.sum()), 0, 0
        oversize = int((chunk_hits > max_hits).sum())
        parts = []
        contained = torch.zeros(R, dtype=torch.bool, device=dev)
        for a_lo, a_hi, n_hits in zip(bounds[:-1].tolist(), bounds[1:].tolist(), chunk_hits.tolist()):
            if n_hits == 0:
                continue
            hits = list(engine.seed_pairs_range(h, rd, ps, st, reads.length, k, max_occ, a_lo, a_hi, rec, threads))
            chunks, peak_hits = chunks + 1, max(peak_hits, int(hits[0].numel()))
            *cand, c = _candidates(hits, *chain)                       # the chunk's hits are gone when this returns
            parts.append(cand)
            contained |= c.bool()
        del h, rd, ps, st
        cat =lambda j, dt: torch.cat([p[j] for p in parts]) if parts else torch.empty(0, dtype=dt, device=dev)  # noqa: E731
        src, dst, prefix, ovl = cat(0, torch.int32), cat(1, torch.int32), cat(2, torch.int64), cat(3, torch.int64)
        sim, exceeded = (cat(4, torch.float32), cat(5, torch.bool)) if verify else (None, None)
    n = 2 * R
    exceeded_pairs = 0
    pair_ok = torch.ones(int(src.numel()) // 2, dtype=torch.bool, device=dev)
    if verify:
        bad = exceeded.view(-1, 2).any(dim=1)
        exceeded_pairs = int(bad.sum())
        pair_ok &= ~bad
    if drop_contained:
        touched = contained[(src >> 1).long()] | contained[(dst >> 1).long()]
        pair_ok &= ~touched.view(-1, 2).any(dim=1)
    keep = pair_ok.repeat_interleave(2)
    src, dst, prefix, ovl = src[keep], dst[keep], prefix[keep], ovl[keep]
    E = int(src.numel())
    order = torch.sort(src.long() * max(n, 1) + dst.long(), stable=True).indices      # src-major edge ids
    rank = torch.empty_like(order)
    rank[order] = torch.arange(E, device=dev)
    twin = rank[torch.arange(E, device=dev) ^ 1][order]
    g = AssemblyGraph.from_tensors(src[order].contiguous(), dst[order].contiguous(), n)
    g.edata["prefix_length"], g.edata["overlap_length"], g.edata["twin"] = prefix[order].contiguous(), ovl[order].contiguous(), twin
    if sim is not None:
        g.edata["overlap_similarity"] = sim[keep][order].contiguous()
    read_length = reads.length.repeat_interleave(2)
    return OverlapGraph(g, read_length, contained, OverlapStats.from_record(rec), sketch_size, hit_count, rec, exceeded_pairs,
                        chunks, peak_hits, oversize)
