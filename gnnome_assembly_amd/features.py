"""GPU counterparts of the reference's input preparation (utils.preprocess_graph utils.py:67-74,
utils.add_positional_encoding utils.py:97-138, and the per-step assembly train.py:245-251):
features are computed once on the device from the graph index and stay resident."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .engine import RecordStats, _call, _ptr, _stream, on_device_of, scratch

__all__ = ["positional_encoding", "edge_features", "prepare_graph", "overlap_features", "OverlapFeatures", "AlignStats"]


@on_device_of(lambda graph, *a, **k: graph.device)
def positional_encoding(graph, pe_dim: int = 16, alpha: float = 0.95) -> torch.Tensor:
    """[N, 2+pe_dim] fp32 = in_deg | out_deg | k-step PageRank (the `pe` argument of the model)."""
    lib = _lib.load()
    dev = graph.device
    if dev.type != "cuda":
        raise _lib.GnmError("positional_encoding: the graph must be on a HIP device")
    idx = graph.index(dev)
    N, E = graph.num_nodes(), graph.num_edges()
    pe = torch.empty(N, pe_dim + 2, dtype=torch.float32, device=dev)
    need = lib.gnm_pagerank_pe_workspace_bytes(N)
    ws = scratch(dev).ws(need)
    _call("gnm_pagerank_pe", N, E, _ptr(idx["isrc"]), _ptr(idx["in_ptr"]), _ptr(idx["out_ptr"]), pe_dim,
          C.c_double(alpha), _ptr(pe), _ptr(ws), need, _stream())
    from .engine import node_rows_out
    return node_rows_out(idx, pe)      # the index may use an internal node numbering (graph.py); features leave in the caller's


@on_device_of(lambda overlap_length, overlap_similarity: overlap_similarity)
def edge_features(overlap_length: torch.Tensor, overlap_similarity: torch.Tensor) -> torch.Tensor:
    """[E,2] fp32 z-scored edge features in the caller's edge-id order (the `e` argument)."""
    dev = overlap_similarity.device
    if dev.type != "cuda":
        raise _lib.GnmError("edge_features: tensors must be on a HIP device")
    a = overlap_length.to(torch.float32).contiguous()
    b = overlap_similarity.to(torch.float32).contiguous()
    E = a.numel()
    e = torch.empty(E, 2, dtype=torch.float32, device=dev)
    sc = scratch(dev)
    _call("gnm_edge_feats_zscore", E, _ptr(a), _ptr(b), _ptr(e), _ptr(sc.partials), sc.partials.numel() * 8, _stream())
    return e


@dataclass
class AlignStats(RecordStats):
    """A gnm_align_record (include/gnm.h): edges = aligned (distance <= max_errors, non-empty) + exceeded + empty (no overlap:
    prefix_length == the read's length) + invalid (a node that names no read of the store); clamped (prefix below 0 or above the
    read's length); cells: the sum of m * |T| over the aligned edges; calls."""
    edges: int = 0
    aligned: int = 0
    exceeded: int = 0
    empty: int = 0
    clamped: int = 0
    invalid: int = 0
    cells: int = 0
    calls: int = 0

    @property
    def exceeded_fraction(self) -> float:
        return float(self.exceeded) / float(self.edges) if self.edges else float("nan")


class OverlapFeatures:
    """overlap_features' result, on the graph's device and in the caller's edge-id order: overlap_length int64 [E],
    overlap_similarity fp32 [E], edit_distance int32 [E] (max_errors + 1 where exceeded, -1 where invalid), exceeded bool [E];
    `record`: the int64 [8] gnm_align_record on the device; `stats` reads it once (AlignStats: the one synchronisation)."""

    def __init__(self, overlap_length, overlap_similarity, edit_distance, max_errors, record):
        self.overlap_length, self.overlap_similarity, self.edit_distance = overlap_length, overlap_similarity, edit_distance
        self.max_errors, self.record = int(max_errors), record
        self._stats = None

    @property
    def exceeded(self) -> torch.Tensor:
        return self.edit_distance > self.max_errors

    @property
    def stats(self) -> AlignStats:
        if self._stats is None:
            self._stats = AlignStats.from_record(self.record)
        return self._stats


def overlap_features(graph, reads, prefix_length=None, max_errors: int = 255) -> OverlapFeatures:
    """overlap_length and overlap_similarity of every edge FROM THE READS, on the device (gnm_overlap_align, one launch): for edge
    a -> c with p = prefix_length, the edit distance between bases [p, la) of a's strand and the best-fitting start of c's strand
    (all of the suffix aligned, the end in c free, at most max_errors edits; codes match when equal, N only with N);
    overlap_length = la - p (graph_parser.py:281) and overlap_similarity = max(0, 1 - distance / overlap_length) in fp32.  An
    edit-distance identity: NOT the overlapper's own similarity figure (graph_parser.py:268-282 copies that from its CSV line),
    for which the reference holds no formula.  An edge whose distance exceeds max_errors (0 .. 255) gets max_errors + 1.
    reads: a ReadStore on the graph's device; prefix_length [E]: default graph.edata['prefix_length']."""
    from . import engine
    from .reads import ReadStore
    if not isinstance(reads, ReadStore):
        raise TypeError("overlap_features: reads must be a ReadStore")
    dev = graph.device
    if dev.type != "cuda":
        raise _lib.GnmError("overlap_features: the graph must be on a HIP device (no CPU fallback)")
    if reads.device != dev:
        raise _lib.GnmError(f"overlap_features: the ReadStore is on {reads.device}, the graph on {dev}")
    if prefix_length is None:
        prefix_length = graph.edata.get("prefix_length")
        if prefix_length is None:
            raise ValueError("overlap_features: no prefix_length given and the graph has no edata['prefix_length']")
    E = graph.num_edges()
    pl = torch.as_tensor(prefix_length).reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    if pl.numel() != E:
        raise ValueError(f"overlap_features: prefix_length holds {pl.numel()} entries for {E} edges")
    src, dst = graph.edges()
    with torch.cuda.device(dev):
        src, dst = src.to(torch.int32).contiguous(), dst.to(torch.int32).contiguous()
        dist = torch.empty(E, dtype=torch.int32, device=dev)
        olen = torch.empty(E, dtype=torch.int64, device=dev)
        sim = torch.empty(E, dtype=torch.float32, device=dev)
        rec = torch.zeros(engine.ALIGN_RECORD_WORDS, dtype=torch.int64, device=dev)
        engine.overlap_align(src, dst, pl, graph.num_nodes(), reads.base_off, reads.length, reads.packed, max_errors, dist, olen, sim,
                             rec)
    return OverlapFeatures(olen, sim, dist, max_errors, rec)


def prepare_graph(graph, nb_pos_enc: int = 16, reads=None, max_errors: int = 255):
    """preprocess_graph + add_positional_encoding on the device: fills graph.ndata['x','pe','in_deg',
    'out_deg'] and graph.edata['e'] (from edata 'overlap_length' / 'overlap_similarity') and returns
    (x, e, pe18) exactly as train.py:246-251 hands them to the model.
    reads: a ReadStore on the graph's device.  When the graph carries no edata['overlap_similarity'], overlap_length and
    overlap_similarity are first filled from overlap_features(graph, reads, max_errors=max_errors)."""
    if reads is not None and "overlap_similarity" not in graph.edata:
        f = overlap_features(graph, reads, max_errors=max_errors)
        graph.edata["overlap_length"], graph.edata["overlap_similarity"] = f.overlap_length, f.overlap_similarity
    pe18 = positional_encoding(graph, nb_pos_enc)
    graph.ndata["in_deg"], graph.ndata["out_deg"], graph.ndata["pe"] = pe18[:, 0], pe18[:, 1], pe18[:, 2:]
    graph.ndata["x"] = torch.ones(graph.num_nodes(), 1, device=graph.device)        # utils.py:69
    e = None
    if "overlap_length" in graph.edata and "overlap_similarity" in graph.edata:
        e = edge_features(graph.edata["overlap_length"], graph.edata["overlap_similarity"])
        graph.edata["e"] = e
    return graph.ndata["x"], e, pe18
