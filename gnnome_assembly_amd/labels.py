"""Ground-truth edge labels FROM THE READS' POSITIONS (include/gnm.h, "ground-truth labels"): what the reference computes offline with
algorithms.get_gt_graph (graph_parser.py:307-309), restated without a walk order so that it runs in parallel.
With it simulated reads of known position are enough to train: ReadStore -> overlap.find_overlaps -> label_overlap_graph ->
prepare_graph -> train.GraphSample.

A graph on a device runs the kernels of csrc/gnm_labels.hip; a CPU graph runs the host entry over the same header."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import engine
from .engine import RecordStats
from .graph import as_assembly_graph

__all__ = ["ground_truth_labels", "node_positions", "label_overlap_graph", "GroundTruth", "GroundTruthStats"]


@dataclass
class GroundTruthStats(RecordStats):
    """A gnm_gt_record (include/gnm.h): edges = valid + wrong_strand + self_loops + gap + backward; components of + strand nodes, of
    which singletons hold one node; backbone nodes; positives (edges with y = 1); twin_missing (positive + strand edges without a
    mirror); invalid; calls -- then, filled on the host, the rounds each device stage took (0 on the CPU route; they depend on the
    schedule, nothing else here does)."""
    edges: int = 0
    valid: int = 0
    wrong_strand: int = 0
    self_loops: int = 0
    gap: int = 0
    backward: int = 0
    components: int = 0
    singletons: int = 0
    backbone: int = 0
    positives: int = 0
    twin_missing: int = 0
    invalid: int = 0
    calls: int = 0
    component_rounds: int = 0
    fwd_rounds: int = 0
    bwd_rounds: int = 0


@dataclass
class GroundTruth:
    """ground_truth_labels' result, on the graph's device: y fp32 [E] and valid bool [E] in edge-id order; backbone bool [n];
    component int32 [n] (the root's node id, -1 on - strand nodes); top int32 [n] (the top of the node's component, -1 likewise);
    stats: GroundTruthStats; record: the int64 record tensor."""
    y: torch.Tensor
    valid: torch.Tensor
    backbone: torch.Tensor
    component: torch.Tensor
    top: torch.Tensor
    stats: GroundTruthStats
    record: torch.Tensor


def _node_tensor(name, t, n, dev):
    if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() != n:
        raise ValueError(f"ground_truth_labels: {name} must be an int64 [{n}] tensor")
    return t.to(dev).contiguous()


def ground_truth_labels(graph, read_start, read_end, read_strand, twin=None, rounds_per_batch=None) -> GroundTruth:
    """Labels of the edges of `graph` from per-node read_start, read_end (int64, start < end, below 2^32) and read_strand (int64, +1 /
    -1) -- the reference's ndata (graph_parser.py:258-260); nodes v and v^1 are the two strands of one read.  An edge s -> d is valid
    when both ends are + strand, s != d and start[s] <= start[d] < end[s]; over those, per weakly connected component, the backbone
    is what the leftmost read reaches and what reaches the farthest-ending read so reached; y = 1 on the valid edges between
    backbone nodes and on their mirrors d^1 -> s^1, 0 elsewhere.  twin: None, or int64 [E] mirror edge ids (OverlapGraph carries
    them), which replace the search for the mirror.  rounds_per_batch: device rounds per read-back (engine.GT_ROUNDS_PER_BATCH)."""
    g = as_assembly_graph(graph)
    dev, n, E = g.device, g.num_nodes(), g.num_edges()
    start, end, strand = (_node_tensor(k, t, n, dev) for k, t in
                          (("read_start", read_start), ("read_end", read_end), ("read_strand", read_strand)))
    if twin is not None:
        if not torch.is_tensor(twin) or twin.dtype != torch.int64 or twin.dim() != 1 or twin.numel() != E:
            raise ValueError(f"ground_truth_labels: twin must be None or an int64 [{E}] tensor")
        twin = twin.to(dev).contiguous()
    src, dst = (t.to(torch.int32).contiguous() for t in g.edges())
    new = lambda m, dt: torch.empty(m, dtype=dt, device=dev)  # noqa: E731
    y, valid, backbone = new(E, torch.float32), new(E, torch.uint8), new(n, torch.uint8)
    component, top = new(n, torch.int32), new(n, torch.int32)
    rec = torch.zeros(engine.GT_RECORD_WORDS, dtype=torch.int64, device=dev)
    if dev.type == "cpu":
        rounds = engine.gt_labels_host(src, dst, n, start, end, strand, twin, y, valid, backbone, component, top, rec)
    else:
        rounds = engine.gt_labels(g.index(dev), src, dst, start, end, strand, twin, y, valid, backbone, component, top, rec,
                                  rounds_per_batch)
    stats = GroundTruthStats(*[int(v) for v in rec.cpu().tolist()], rounds["components"], rounds["fwd"], rounds["bwd"])
    return GroundTruth(y, valid.bool(), backbone.bool(), component, top, stats, rec)


def node_positions(truth, n: int):
    """(read_start, read_end, read_strand) int64 [n] CPU tensors for n = 2 R nodes from per-read (start, end, strand) rows, strand
    0 / 1 as tests and simulators give it (1: the stored read is the reverse complement of the genome): node 2r is the stored read,
    2r + 1 its reverse complement, so the node that reads along the genome -- 2r + strand -- is the + strand one."""
    t = torch.as_tensor(truth, dtype=torch.int64).reshape(-1, 3)
    if 2 * t.shape[0] != int(n):
        raise ValueError(f"node_positions: {t.shape[0]} reads for {n} nodes: expected n = 2 R")
    if bool(((t[:, 2] != 0) & (t[:, 2] != 1)).any()):
        raise ValueError("node_positions: a read's strand must be 0 or 1")
    start, end = t[:, 0].repeat_interleave(2), t[:, 1].repeat_interleave(2)
    strand = torch.stack((1 - 2 * t[:, 2], 2 * t[:, 2] - 1), dim=1).reshape(-1)
    return start.contiguous(), end.contiguous(), strand.contiguous()


def label_overlap_graph(og, truth, rounds_per_batch=None) -> GroundTruth:
    """ground_truth_labels for an overlap.OverlapGraph and the per-read (start, end, strand) rows of its reads, with the graph's own
    `twin`."""
    g = og.graph
    start, end, strand = node_positions(truth, g.num_nodes())
    return ground_truth_labels(g, start, end, strand, twin=g.edata.get("twin"), rounds_per_batch=rounds_per_batch)
