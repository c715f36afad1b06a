"""Training-harness counterpart of the reference's full-graph branch (train.py:115-533 with
batch_size_train <= 1): per-graph Adam steps, validation under no_grad/eval, ReduceLROnPlateau,
best-model + checkpoint files with the reference's key schema.  SURVEY.md section 8f row 2.

Differences from the reference, all deliberate:
  * graphs, features and the index stay resident on the device (the reference re-uploads every
    step, train.py:245-251);
  * TP/TN/FP/FN are accumulated on the device and read back once per epoch (the reference's
    utils.calculate_tfpn forces four .item() syncs per graph, utils.py:217-223);
  * under torch.distributed (one process per GPU) the W graphs of a step contribute the MEAN of
    their gradients through one RCCL all-reduce (dp.FlatGradients); single-process runs reproduce the
    reference's one-step-per-graph sequence;
  * the ClusterGCN mini-batch branch (train.py:282-343,428-486; batch_size_* > 1) runs on this
    package's own partitioner (cluster.py: METIS is part of DGL and not available), otherwise with
    the reference's loop: a fresh partition per graph and epoch with a random number of clusters in
    [num_parts-100, num_parts+100), shuffled batches of clusters, one Adam step per batch;
  * with the hyper-parameter "fused_metrics" (default: GNM_FUSED_METRICS=1, else off) the loss kernel also counts TP..FN and adds
    the step to the epoch's sums (BCEWithLogitsLoss.with_counts + EpochStats): same History, no metric launches in the loop;
  * with the hyper-parameter "optimizer": "library" (default: GNM_OPTIM=library, else "torch") the step is dp.LibAdam's: two
    launches over the flat buffers that also leave the gradient zeroed for the next backward, clip the gradient's norm to
    "clip_grad_norm" (0: off) and skip a step whose gradient is not finite, counted in History.skipped_steps;
  * with the hyper-parameter "ranking_metrics" (default: GNM_RANKING_METRICS=1, else off) every validation forward also adds its
    logits to a per-label histogram on the device (RankingStats, one launch, no sort, nothing of size [E]); once per epoch the 256 KiB
    record is read and History gains the threshold-free figures the fixed sigmoid(x) = 0.5 counts cannot give: AUROC, average
    precision and the best-F1 threshold.  Loss, schedule, best-model choice and every other History field are the same either way;
  * with the hyper-parameter "decision_metrics" (default: GNM_DECISION_METRICS=1, else off) every validation forward also counts the
    choices the greedy decode would make on its logits (DecisionStats: per node the top-scored out-edge and in-edge, one launch);
    once per epoch the 15-word record is read and History.decision_valid gains (branch_accuracy, solvable_accuracy, successor-side and
    predecessor-side branch accuracy): how often, at a node where the walk has a choice, the chosen edge is a correct one.  With
    batch_size_eval > 1 the decisions are counted on each batch's sub-graph and summed: a node at a cut sees only the candidates
    inside its batch, so it may count as forced or dead where the whole graph would have made it a branch.  Under the symmetry loss
    the original scores are counted.  Loss, schedule, best-model choice and every other History field are the same either way;
  * with the hyper-parameter "assembly_metrics" (default: GNM_ASSEMBLY_METRICS=1, else off) every full-graph validation forward also
    decodes its logits into the contigs of the best-overlap graph on the device (decode.best_overlap_contigs: mutual-best edges, list
    ranking; the graph's edata["prefix_length"] / ndata["read_length"]) and keeps the bases and wrong-link counts of the contigs with at
    least 20 nodes; once per epoch History.assembly_valid gains (contigs, N50 in bases, longest contig in bases, wrong links / links)
    over the pooled contigs of the epoch's validation graphs.  Refused with batch_size_eval > 1 (a cover across cluster cuts means
    nothing).  Under the symmetry loss the original scores are decoded.  Loss, schedule, best-model choice and every other History
    field are the same either way;
  * with the hyper-parameters "mask_frac_low" / "mask_frac_high" (per cent; default 100 / 100: off) every training step runs on the graph
    thinned to a random fraction of its READS (cluster.masked_subgraph: a device mask that is a pure function of seed, epoch, graph and
    read; the thinned graph's own degrees in `pe`), the next step's graph built on a side stream meanwhile (cluster.MaskedGraphLoader);
    a thinned graph without an edge is a zero-contribution step; validation is never masked; History gains mask_fraction / masked_edges;
  * wandb and the data pipeline are out of scope.
`calculate_metrics` keeps the reference's naming, in which "precision" and "recall" are swapped
(utils.py:227-234)."""
from __future__ import annotations

import copy
import os
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import cluster, dp, engine, models

__all__ = ["get_hyperparameters", "check_symmetry_hyperparameters", "symmetry_step", "GraphSample", "tfpn_counts", "calculate_metrics", "train", "save_checkpoint", "EpochStats",
           "RankingStats", "RankingMetrics", "BestF1", "DecisionStats", "DecisionMetrics", "DecisionCounts", "AssemblyStats"]


def get_hyperparameters() -> Dict:
    """hyperparameters.py:3-34 with the full-graph branch selected (batch_size_* = 1)."""
    return {
        "seed": 0, "lr": 1e-3, "num_epochs": 100, "dim_latent": 256, "node_features": 1, "edge_features": 2,
        "hidden_edge_features": 16, "hidden_edge_scores": 64, "num_gnn_layers": 16, "nb_pos_enc": 16,
        "batch_size_train": 1, "batch_size_eval": 1, "patience": 2, "decay": 0.95, "batch_norm": True,
        # only read when batch_size_* > 1 (hyperparameters.py:15-18 has 500 / 500 / 50 / 50)
        "num_parts_metis_train": 500, "num_parts_metis_eval": 500, "partition_method": "locality",
        # loss, TP..FN and the epoch sums from one pass over the logits (criterion.with_counts); same History either way
        "fused_metrics": os.environ.get("GNM_FUSED_METRICS", "0").strip() == "1",
        # node-output dropout of the GatedGCN layers (GraphGatedGCNModel's dropout keyword); validation runs in eval mode: none there
        "dropout": 0.0,
        # "torch": dp.make_adam.  "library": dp.LibAdam (Adam, norm clip and non-finite guard in the library's own two launches)
        "optimizer": "library" if os.environ.get("GNM_OPTIM", "").strip().lower() == "library" else "torch",
        # the gradient's global norm is clipped to this before the step (torch's clip_grad_norm_); 0: off; "library" route only
        "clip_grad_norm": 0.0,
        # AUROC, average precision and the best-F1 threshold of every validation epoch from a histogram of the logits (RankingStats)
        "ranking_metrics": os.environ.get("GNM_RANKING_METRICS", "0").strip() == "1",
        # how often the greedy decode's choice at a node (top-scored out-edge / in-edge) is a correct edge, per validation epoch (DecisionStats)
        "decision_metrics": os.environ.get("GNM_DECISION_METRICS", "0").strip() == "1",
        # contig count, N50, longest contig and wrong-link share of the best-overlap contigs of every validation epoch (AssemblyStats)
        "assembly_metrics": os.environ.get("GNM_ASSEMBLY_METRICS", "0").strip() == "1",
        # read-masking coverage augmentation: every TRAINING step keeps a fraction f = randint(low, high) / 100 of the reads (per cent,
        # 1 <= low <= high <= 100; 100 / 100: off) and runs on the induced sub-graph with its own degrees in `pe`; the 16 PageRank
        # columns are carried from the parent unless mask_recompute_pe.  Validation is never masked.
        "mask_frac_low": 100, "mask_frac_high": 100, "mask_recompute_pe": False,
        # symmetry loss (models.SymmetryLoss): every step scores the graph and its edge-reversed twin (model(..., reverse=True)) and
        # is penalised for both BCE terms and alpha |org - rev| per edge.  "symmetry_schedule": "joint" (two forwards, one backward,
        # both activation sets alive) or "sequential" (three forwards, one activation set alive at a time; no dropout)
        "symmetry_loss": os.environ.get("GNM_SYMMETRY_LOSS", "0").strip() == "1", "alpha": 0.1, "symmetry_schedule": "joint",
    }


def check_symmetry_hyperparameters(hp: Dict) -> bool:
    """True when the symmetry loss is on; ValueError for a schedule, an alpha or a combination that is not supported."""
    if hp["symmetry_schedule"] not in ("joint", "sequential"):
        raise ValueError(f"hyper-parameter symmetry_schedule={hp['symmetry_schedule']!r}: expected 'joint' or 'sequential'")
    if not (isinstance(hp["alpha"], (int, float)) and 0.0 <= float(hp["alpha"]) < float("inf")):
        raise ValueError(f"hyper-parameter alpha={hp['alpha']!r}: expected a finite number >= 0")
    if not hp["symmetry_loss"]:
        return False
    if hp["symmetry_schedule"] == "sequential" and float(hp["dropout"]) > 0.0:
        raise ValueError("hyper-parameter symmetry_schedule='sequential' with dropout > 0: the schedule runs the original forward "
                         "twice and the second run would draw another dropout mask; use 'joint' or dropout 0")
    return True


def symmetry_step(model, criterion, graph, x, e, pe, y, schedule: str = "joint", epoch_acc=None, counts: bool = False):
    """One training step's forward and backward passes under the symmetry loss; returns (loss, org), both detached.
    "joint": the reversed forward, then the original one, one loss.backward() -- autograd runs the later-built graph first, so the
    original pass writes its gradient straight into a fresh dp.FlatGradients buffer and the reversed pass folds its own in behind it.
    "sequential": original forward under no_grad, reversed forward with grad, the loss kernel, the reversed backward, the original
    forward again with grad (the kernels are bit-reproducible: the scores the loss saw), the original backward: one activation set
    alive at a time for a third forward.  counts / epoch_acc: criterion.with_counts' (the fused-metrics route)."""
    if schedule == "joint":
        rev = model(graph, x, e, pe, reverse=True).squeeze(-1)
        org = model(graph, x, e, pe).squeeze(-1)
        loss = criterion.with_counts(org, rev, y, epoch_acc)[0] if (counts or epoch_acc is not None) else criterion(org, rev, y)
        loss.backward()
        return loss.detach(), org.detach()
    with torch.no_grad():
        org0 = model(graph, x, e, pe).squeeze(-1)
    rev = model(graph, x, e, pe, reverse=True).squeeze(-1)
    loss, _, g_org, g_rev = criterion.gradients(org0, rev, y, epoch_acc)
    torch.autograd.backward(rev, g_rev)
    del rev
    org = model(graph, x, e, pe).squeeze(-1)
    torch.autograd.backward(org, g_org)
    return loss, org0


@dataclass
class GraphSample:
    """One training graph resident on the device: what train.py:245-254 pulls out of a DGLGraph."""
    graph: object                 # AssemblyGraph on the device
    e: torch.Tensor               # [E,2] z-scored edge features (edge-id order)
    pe: torch.Tensor              # [N, nb_pos_enc+2] = in_deg | out_deg | pe
    y: torch.Tensor               # [E] float labels
    x: Optional[torch.Tensor] = None


def tfpn_counts(edge_predictions: torch.Tensor, edge_labels: torch.Tensor) -> torch.Tensor:
    """[TP, TN, FP, FN] as a device int64 tensor (utils.calculate_tfpn without the .item() syncs)."""
    p = torch.round(torch.sigmoid(edge_predictions))
    return torch.stack([((p == 1) & (edge_labels == 1)).sum(), ((p == 0) & (edge_labels == 0)).sum(),
                        ((p == 1) & (edge_labels == 0)).sum(), ((p == 0) & (edge_labels == 1)).sum()])


class EpochStats:
    """The running sums of an epoch (or of one graph's batches) on the device, in the 48-byte record that
    BCEWithLogitsLoss.with_counts(..., epoch_acc=self) adds every step to: {double loss_sum; int64 steps; int64 counts[4]}.
    loss_sum is the fp64 sum of the steps' fp32 losses in call order.  `loss_sum`, `steps` and `counts` are views of `buf`."""

    def __init__(self, device):
        self.buf = torch.zeros(6, dtype=torch.int64, device=device)
        self.loss_sum = self.buf[0:1].view(torch.float64)[0]
        self.steps = self.buf[1]
        self.counts = self.buf[2:6]

    def zero_(self):
        self.buf.zero_()
        return self

    def read(self):
        """(loss_sum, steps, (TP, TN, FP, FN)) with one device-to-host copy."""
        b = self.buf.cpu()
        return float(b[0:1].view(torch.float64)[0]), int(b[1]), tuple(int(c) for c in b[2:6].tolist())


RANK_BINS = 16384            # bins per label: the 14-bit key of an fp32 logit (include/gnm.h, gnm_rank_record)


def rank_bin_lower_edge(k) -> np.ndarray:
    """The smallest fp32 value whose key is k (fp64 array): the logit threshold "predict positive from bin k upwards".  Invert
    key = u >> 18 with u = bits ^ (sign ? 0xFFFFFFFF : 0x80000000): a bin of positive values starts at its smallest bit pattern, a
    bin of negative values at its largest.  Bin 31 holds -inf alone among the values that are not NaN: its edge is -inf."""
    u = np.asarray(k, dtype=np.uint64) << np.uint64(18)
    bits = np.where(u >> np.uint64(31) != 0, u ^ np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF))
    with np.errstate(invalid="ignore"):              # the edges of the bins that only NaN patterns fall into
        x = bits.astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(np.isnan(x), np.where(u >> np.uint64(31) != 0, np.inf, -np.inf), x)


@dataclass
class BestF1:
    """The threshold "positive iff logit >= logit" (the lower edge of bin `bin`) with the largest F1 = 2TP / (2TP + FP + FN) among
    the occupied bins; of equal F1 values the highest bin.  prob = sigmoid(logit)."""
    f1: float
    logit: float
    prob: float
    bin: int
    TP: int
    TN: int
    FP: int
    FN: int


@dataclass
class RankingMetrics:
    """What a gnm_rank_record says about how the logits order positives and negatives (host code, fp64 numpy on integers).
    auroc counts a (positive, negative) pair in one bin as 1/2, auroc_lo as 0 and auroc_hi as 1: the exact Mann-Whitney AUROC of the
    raw logits (ties 1/2) lies in [auroc_lo, auroc_hi], because two edges in different bins are ordered as their bins are."""
    auroc: float
    auroc_lo: float
    auroc_hi: float
    average_precision: float
    best_f1: Optional[BestF1]
    n_pos: int               # binned positives and negatives (NaN logits and other labels are in n_nan / n_other)
    n_neg: int
    n_nan: int
    n_other: int
    calls: int
    hist: np.ndarray = field(repr=False, compare=False, default=None)       # int64 [2, RANK_BINS]: negatives, positives

    @classmethod
    def from_counts(cls, hist, tail) -> "RankingMetrics":
        hist = np.asarray(hist, dtype=np.int64).reshape(2, RANK_BINS)
        tail = np.asarray(tail, dtype=np.int64).reshape(4)
        neg, pos = hist[0].astype(np.float64), hist[1].astype(np.float64)
        P, N = float(pos.sum()), float(neg.sum())
        nan = float("nan")
        if P > 0 and N > 0:
            above = P - np.cumsum(pos)                                        # positives in the bins above k
            lo = float((neg * above).sum())
            tie = float((neg * pos).sum())
            auroc, auroc_lo, auroc_hi = (lo + 0.5 * tie) / (P * N), lo / (P * N), (lo + tie) / (P * N)
        else:
            auroc = auroc_lo = auroc_hi = nan
        occ = np.flatnonzero(hist[0] + hist[1])[::-1]                         # occupied bins, from the top
        best, ap = None, nan
        if occ.size:
            tp, fp = np.cumsum(pos[occ]), np.cumsum(neg[occ])                 # predicted positive from bin occ[i] upwards
            if P > 0 and N > 0:
                ap = float((pos[occ] / P * (tp / (tp + fp))).sum())           # sum over bins of (R_k - R_{k-1}) Prec_k
            den = 2.0 * tp + fp + (P - tp)
            f1 = np.where(den > 0, 2.0 * tp / np.where(den > 0, den, 1.0), 0.0)
            i = int(np.argmax(f1))                                            # first maximum from the top: the highest bin
            edge = float(rank_bin_lower_edge(occ[i]))
            with np.errstate(over="ignore"):
                prob = float(1.0 / (1.0 + np.exp(-edge)))
            best = BestF1(float(f1[i]), edge, prob, int(occ[i]), int(tp[i]), int(N - fp[i]), int(fp[i]), int(P - tp[i]))
        return cls(auroc, auroc_lo, auroc_hi, ap, best, int(P), int(N), int(tail[0] + tail[1]), int(tail[2]), int(tail[3]), hist)

    def _curve(self):
        occ = np.flatnonzero(self.hist[0] + self.hist[1])[::-1]
        tp, fp = np.cumsum(self.hist[1][occ]).astype(np.float64), np.cumsum(self.hist[0][occ]).astype(np.float64)
        return occ, tp, fp

    def roc(self):
        """(fpr, tpr, logit thresholds) over the occupied bins from the top; NaN where a class is empty."""
        occ, tp, fp = self._curve()
        with np.errstate(invalid="ignore", divide="ignore"):
            return fp / float(self.n_neg), tp / float(self.n_pos), rank_bin_lower_edge(occ)

    def pr(self):
        """(precision, recall, logit thresholds) over the occupied bins from the top."""
        occ, tp, fp = self._curve()
        with np.errstate(invalid="ignore", divide="ignore"):
            return tp / (tp + fp), tp / float(self.n_pos), rank_bin_lower_edge(occ)


class RankingStats:
    """A gnm_rank_record as one int64 tensor `buf` of 2 * RANK_BINS + 4 words: hist[2][RANK_BINS] (negatives, positives) and
    tail[4] = nan_pos, nan_neg, other_label, calls (`hist` and `tail` are views).  add() is one launch on the current stream and
    needs a HIP device; the buffer itself may live on the CPU (all_reduce_ under gloo, RankingMetrics.from_counts).  Records add:
    across steps, graphs and -- all_reduce_ -- ranks."""

    def __init__(self, device):
        self.buf = torch.zeros(2 * RANK_BINS + 4, dtype=torch.int64, device=device)
        self.hist = self.buf[:2 * RANK_BINS].view(2, RANK_BINS)
        self.tail = self.buf[2 * RANK_BINS:]

    def zero_(self):
        self.buf.zero_()
        return self

    def add(self, scores, y):
        from . import engine
        engine.rank_hist(scores.detach(), y, self.buf)
        return self

    def all_reduce_(self):
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.buf)
        return self

    def read(self) -> RankingMetrics:
        b = self.buf.cpu().numpy()
        return RankingMetrics.from_counts(b[:2 * RANK_BINS], b[2 * RANK_BINS:])


DECISION_COUNTERS = engine.DECISION_COUNTERS                   # the seven counters of gnm_decision_record.dir[d], in order
DECISION_RECORD_WORDS = engine.DECISION_RECORD_WORDS           # dir[2][7] (successors, predecessors), then calls


def _ratio(num: int, den: int) -> float:
    return float(num) / float(den) if den else float("nan")


@dataclass
class DecisionCounts:
    """One direction's counters of a gnm_decision_record (or the two directions' sums) and their ratios; a ratio whose denominator
    is 0 is NaN.  branch_accuracy: of the nodes where the walk has a choice (two or more candidate edges), the fraction whose
    top-scored candidate is a correct edge (y == 1); solvable_accuracy: the same over the nodes where some candidate IS correct
    (the others cannot be got right); forced_accuracy: of the nodes with exactly one candidate, the fraction where it is correct."""
    dead: int = 0
    forced: int = 0
    forced_ok: int = 0
    branch: int = 0
    branch_solvable: int = 0
    branch_ok: int = 0
    branch_nan: int = 0

    @property
    def branch_accuracy(self) -> float:
        return _ratio(self.branch_ok, self.branch)

    @property
    def solvable_accuracy(self) -> float:
        return _ratio(self.branch_ok, self.branch_solvable)

    @property
    def forced_accuracy(self) -> float:
        return _ratio(self.forced_ok, self.forced)

    def __add__(self, other: "DecisionCounts") -> "DecisionCounts":
        return DecisionCounts(*[getattr(self, k) + getattr(other, k) for k in DECISION_COUNTERS])


@dataclass
class DecisionMetrics:
    """What a gnm_decision_record says about the choices the greedy decode would make on the scores: `succ` (walk_forwards: the
    top-scored out-edge of every node), `pred` (walk_backwards: the top-scored in-edge) and `pooled` (their sums), each a
    DecisionCounts; branch_accuracy / solvable_accuracy / forced_accuracy are the pooled ratios.  Host code on integers."""
    succ: DecisionCounts
    pred: DecisionCounts
    pooled: DecisionCounts
    calls: int = 0

    @classmethod
    def from_counts(cls, counts) -> "DecisionMetrics":
        """counts: the DECISION_RECORD_WORDS int64 words of a record (DecisionStats.buf), or the 14 counters without `calls`."""
        c = [int(v) for v in np.asarray(counts).reshape(-1).tolist()]
        k = len(DECISION_COUNTERS)
        if len(c) not in (2 * k, 2 * k + 1):
            raise ValueError(f"DecisionMetrics.from_counts: {len(c)} words, expected {2 * k} or {2 * k + 1}")
        if min(c) < 0:
            raise ValueError("DecisionMetrics.from_counts: negative count")
        succ, pred = DecisionCounts(*c[:k]), DecisionCounts(*c[k:2 * k])
        return cls(succ, pred, succ + pred, c[2 * k] if len(c) > 2 * k else 0)

    @property
    def branch_accuracy(self) -> float:
        return self.pooled.branch_accuracy

    @property
    def solvable_accuracy(self) -> float:
        return self.pooled.solvable_accuracy

    @property
    def forced_accuracy(self) -> float:
        return self.pooled.forced_accuracy

    def summary(self) -> tuple:
        """The History.decision_valid entry: (branch_accuracy, solvable_accuracy, succ branch_accuracy, pred branch_accuracy)."""
        return (self.branch_accuracy, self.solvable_accuracy, self.succ.branch_accuracy, self.pred.branch_accuracy)


class DecisionStats:
    """A gnm_decision_record as one int64 tensor `buf` of DECISION_RECORD_WORDS words: dir[2][7] (successors, predecessors; the
    counters of DECISION_COUNTERS) and calls.  add() is one launch on the current stream and needs a HIP device; the buffer itself
    may live on the CPU (all_reduce_ under gloo, DecisionMetrics.from_counts).  Records add: across graphs, the sub-graphs of a
    mini-batch pass and -- all_reduce_ -- ranks."""

    def __init__(self, device):
        self.buf = torch.zeros(DECISION_RECORD_WORDS, dtype=torch.int64, device=device)

    def zero_(self):
        self.buf.zero_()
        return self

    def add(self, graph, scores, y=None, best_succ=None, best_pred=None):
        """Count the decisions of `graph` (an AssemblyGraph on the buffer's device) under `scores` [E] (edge-id order) and the
        labels `y` [E] (None: only dead / forced / branch / branch_nan move)."""
        from .graph import as_assembly_graph
        idx = as_assembly_graph(graph, self.buf.device).index(self.buf.device)
        engine.decision_stats(idx, scores, y, self.buf, best_succ, best_pred)
        return self

    def all_reduce_(self):
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.buf)
        return self

    def read(self) -> DecisionMetrics:
        return DecisionMetrics.from_counts(self.buf.cpu().numpy())


ASSEMBLY_MIN_NODES = 20      # History.assembly_valid pools the contigs of at least this many nodes (the decode's len_threshold)


class AssemblyStats:
    """The best-overlap contigs of an epoch's validation graphs: `rec`, the sum of their gnm_bog_records (int64 [8], host), and the
    bases of the contigs of at least `min_nodes` nodes, pooled.  add() decodes one graph on the device (decode.best_overlap_contigs:
    one host synchronisation) and needs a HIP device.  Under torch.distributed all_reduce_() sums the records and gathers the pooled
    lengths (all_gather_object), once per epoch."""

    def __init__(self, device, min_nodes: int = ASSEMBLY_MIN_NODES):
        self.device = torch.device(device)
        self.min_nodes = int(min_nodes)
        self.zero_()

    def zero_(self):
        self.rec = np.zeros(engine.BOG_RECORD_WORDS, np.int64)
        self.bases: List[int] = []
        self.wrong: List[int] = []
        return self

    def add(self, graph, scores, y=None):
        from . import decode
        c = decode.best_overlap_contigs(graph, scores.detach(), graph.edata["prefix_length"], graph.ndata["read_length"], y)
        self.rec += np.asarray(c.stats.words(), np.int64)
        keep = c.num_nodes() >= self.min_nodes
        self.bases += c.bases[keep].cpu().tolist()
        self.wrong += c.wrong[keep].cpu().tolist()
        return self

    def all_reduce_(self):
        if dist.is_available() and dist.is_initialized():
            t = torch.from_numpy(self.rec).to(self.device)
            dist.all_reduce(t)
            self.rec = t.cpu().numpy()
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, (self.bases, self.wrong))
            self.bases = [b for p in parts for b in p[0]]
            self.wrong = [w for p in parts for w in p[1]]
        return self

    def summary(self) -> tuple:
        """The History.assembly_valid entry: (contigs, n50_bases, longest_bases, wrong_link_fraction) -- the first three over the
        pooled contigs, the last = wrong_links / links of the summed records (NaN without a link)."""
        from .decode import n50
        links, wrong = int(self.rec[1]), int(self.rec[4])
        return (len(self.bases), n50(self.bases), max(self.bases, default=0), _ratio(wrong, links))


def calculate_metrics(TP, TN, FP, FN):
    """utils.calculate_metrics (utils.py:226-240), including its swapped precision/recall names."""
    recall = TP / (TP + FP) if (TP + FP) else 0
    precision = TP / (TP + FN) if (TP + FN) else 0
    f1 = TP / (TP + 0.5 * (FP + FN)) if (TP + 0.5 * (FP + FN)) else 0
    accuracy = (TP + TN) / (TP + TN + FP + FN)
    return accuracy, precision, recall, f1


def save_checkpoint(epoch, model, optimizer, loss_train, loss_valid, out, directory="checkpoints"):
    """train.py:28-58: same dict keys, same file name."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, f"{out}.pt")
    torch.save({"epoch": epoch, "model_state_dict": model.state_dict(), "optim_state_dict": optimizer.state_dict(),
                "loss_train": loss_train, "loss_valid": loss_valid}, path)
    return path


def pos_to_neg_ratio(samples: Sequence[GraphSample]) -> float:
    """train.py:181: dataset mean of #(y==1)/#(y==0)."""
    r = [((s.y == 1).sum() / (s.y == 0).sum()) for s in samples]
    return float(torch.stack(r).mean().item())


def _attach_features(s: GraphSample):
    """The sample's features on its graph's ndata / edata, exactly as the reference keeps them on the DGLGraph (train.py:298-307):
    what a sub-graph slices."""
    g = s.graph
    g.ndata = dict(g.ndata, pe=s.pe)
    g.edata = dict(g.edata, e=s.e, y=s.y)
    return g


def _cluster_batches(s: GraphSample, num_parts: int, batch_size: int, method: str, read_mask=None):
    """The sub-graphs of one pass over a graph in mini-batch mode; features ride on ndata / edata (_attach_features).
    read_mask: None, or (key, epoch, graph_index, recompute_pe, draw) -- every batch is then thinned to the reads its own
    f = draw() keeps (cluster.ClusterBatchLoader(read_mask=...)); the partition is the parent's cached one either way."""
    g = _attach_features(s)
    part = cluster.partition_graph(g, num_parts, method)
    if read_mask is None:
        return cluster.ClusterBatchLoader(g, part, batch_size, shuffle=True)
    key, epoch, graph_index, recompute_pe, draw = read_mask
    nb = len(cluster.ClusterBatchLoader(g, part, batch_size, shuffle=False, prefetch=False))
    return cluster.ClusterBatchLoader(g, part, batch_size, shuffle=True,
                                      read_mask=dict(key=key, epoch=epoch, graph_index=graph_index, recompute_pe=recompute_pe,
                                                     fractions=[draw() for _ in range(nb)]))


@dataclass
class History:
    loss_train: List[float] = field(default_factory=list)
    loss_valid: List[float] = field(default_factory=list)
    lr: List[float] = field(default_factory=list)
    metrics_train: List[tuple] = field(default_factory=list)
    metrics_valid: List[tuple] = field(default_factory=list)
    step_losses: List[float] = field(default_factory=list)      # every optimizer step's loss, in order (this rank's)
    step_graph: List[int] = field(default_factory=list)         # ... and the index of the graph it was taken on
    tfpn_train: List[tuple] = field(default_factory=list)       # per epoch: (TP, TN, FP, FN) summed over the graphs
    tfpn_valid: List[tuple] = field(default_factory=list)
    best_epoch: int = -1
    final_lr: float = 0.0
    skipped_steps: int = 0                                      # "optimizer": "library": steps skipped so far for a non-finite gradient
    total_norm: List[float] = field(default_factory=list)       # ... and per epoch the gradient norm of its last step (before clipping)
    auroc_valid: List[float] = field(default_factory=list)      # "ranking_metrics": per epoch RankingMetrics.auroc of the validation logits,
    ap_valid: List[float] = field(default_factory=list)         # ... .average_precision,
    best_f1_valid: List[tuple] = field(default_factory=list)    # ... and (best_f1.f1, best_f1.logit); all three stay empty when it is off
    decision_valid: List[tuple] = field(default_factory=list)   # "decision_metrics": per epoch DecisionMetrics.summary() of the validation logits:
                                                                # (branch_accuracy, solvable_accuracy, succ and pred branch accuracy); empty when it is off
    assembly_valid: List[tuple] = field(default_factory=list)   # "assembly_metrics": per epoch AssemblyStats.summary() of the validation logits:
                                                                # (contigs, n50_bases, longest_bases, wrong_link_fraction); empty when it is off
    mask_fraction: List[float] = field(default_factory=list)    # "mask_frac_*": the kept read fraction f of every step of this rank on a graph or batch,
    sym_gap_train: List[float] = field(default_factory=list)    # "symmetry_loss": per epoch the mean over the steps of mean_k |org_k - rev_k| (the
    sym_gap_valid: List[float] = field(default_factory=list)    # loss's parts[2], unscaled by alpha), training / validation; empty when it is off
    masked_edges: List[int] = field(default_factory=list)       # ... and the edge count of the thinned graph it ran on (0: a zero-contribution step, which
                                                                # has no entry in step_losses / step_graph); added once per epoch; both empty when it is off


def train(train_samples: Sequence[GraphSample], valid_samples: Sequence[GraphSample], out: str = "model",
          hyperparameters: Optional[Dict] = None, workdir: str = ".", verbose: bool = True,
          hooks: Optional[Dict] = None):
    """Full-graph training loop (train.py:232-281,379-529).  Returns (model, best_state_dict, History).
    Under torch.distributed every rank passes ITS shard of the training AND of the validation graphs
    (dp.shard_graphs; a shard may be empty for validation): the W graphs of a step contribute the mean of their
    gradients, epoch / validation losses and TP..FN counts are summed over the ranks, rank 0 writes the files.
    `hooks` (observers for tests and logging, never needed for training): "after_exchange"(epoch, it, flat) right
    after the gradient exchange of a full-graph step, "after_epoch"(epoch, model) at the end of every epoch;
    "model_factory"(hp) -> nn.Module and "criterion_factory"(pos_weight) -> loss module replace the HIP model / loss (the
    CPU tier drives THIS loop under eight gloo ranks with a CPU stand-in model: tests/test_dp_gloo.py).
    Activation checkpointing is a property of the model (GraphGatedGCNModel.activation_checkpoint): the model built here takes
    the environment's GNM_CHECKPOINT, a "model_factory" sets its own; the loop is the same either way."""
    hooks = hooks or {}
    hp = dict(get_hyperparameters())
    hp.update(hyperparameters or {})
    if hp["optimizer"] not in ("torch", "library"):
        raise ValueError(f"hyper-parameter optimizer={hp['optimizer']!r}: expected 'torch' or 'library'")
    lib_opt = hp["optimizer"] == "library"
    if not float(hp["clip_grad_norm"]) >= 0.0:
        raise ValueError(f"hyper-parameter clip_grad_norm={hp['clip_grad_norm']!r}: expected a number >= 0 (0: off)")
    if hp["clip_grad_norm"] > 0 and not lib_opt:
        raise ValueError("hyper-parameter clip_grad_norm > 0 needs \"optimizer\": \"library\": the torch route does not clip, and "
                         "the value is not silently ignored")
    mlo, mhi = hp["mask_frac_low"], hp["mask_frac_high"]
    if not (isinstance(mlo, int) and isinstance(mhi, int) and 1 <= mlo <= mhi <= 100):
        raise ValueError(f"hyper-parameters mask_frac_low={mlo!r}, mask_frac_high={mhi!r}: expected integers (per cent) with "
                         "1 <= low <= high <= 100 (100 / 100: no masking)")
    masking = not (mlo == 100 and mhi == 100)
    if not isinstance(hp["decision_metrics"], (bool, np.bool_)):
        raise ValueError(f"hyper-parameter decision_metrics={hp['decision_metrics']!r}: expected True or False")
    if not isinstance(hp["assembly_metrics"], (bool, np.bool_)):
        raise ValueError(f"hyper-parameter assembly_metrics={hp['assembly_metrics']!r}: expected True or False")
    if hp["assembly_metrics"]:
        if hp["batch_size_eval"] > 1:
            raise ValueError("hyper-parameter assembly_metrics=True with batch_size_eval > 1: the contigs are decoded on the whole "
                             "validation graph; a cover across cluster cuts means nothing")
        for i, s in enumerate(valid_samples):
            for where, key in (("edata", "prefix_length"), ("ndata", "read_length")):
                if key not in getattr(s.graph, where, {}):
                    raise ValueError(f"hyper-parameter assembly_metrics=True: validation sample {i} has no graph.{where}[{key!r}]")
    sym = check_symmetry_hyperparameters(hp)
    if sym and "criterion_factory" in hooks:
        raise ValueError("hyper-parameter symmetry_loss with a \"criterion_factory\" hook: the symmetry loss is models.SymmetryLoss")
    seed = hp["seed"]
    random.seed(seed)
    torch.manual_seed(seed)                                                     # utils.set_seed
    dev = train_samples[0].pe.device
    if hp["decision_metrics"] and dev.type != "cuda":
        raise ValueError(f"hyper-parameter decision_metrics=True with the samples on {dev}: the decisions are counted by a kernel "
                         "(gnm_decision_stats) and need a HIP device; there is no CPU route")
    if hp["assembly_metrics"] and dev.type != "cuda":
        raise ValueError(f"hyper-parameter assembly_metrics=True with the samples on {dev}: the contigs are decoded by kernels "
                         "(gnm_decision_stats, gnm_bog_contigs) and need a HIP device; there is no CPU route")
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    ratio = pos_to_neg_ratio(train_samples)                                     # train.py:181
    if world > 1:
        t = torch.tensor([ratio * len(train_samples), float(len(train_samples))], device=dev, dtype=torch.float64)
        dist.all_reduce(t)
        ratio = float(t[0] / t[1])
    if "model_factory" in hooks:
        model = hooks["model_factory"](hp).to(dev)
    else:
        model = models.GraphGatedGCNModel(hp["node_features"], hp["edge_features"], hp["dim_latent"],
                                          hp["hidden_edge_features"], hp["num_gnn_layers"], hp["hidden_edge_scores"],
                                          hp["batch_norm"], hp["nb_pos_enc"], dropout=hp["dropout"]).to(dev)   # train.py:195-198
    if world > 1:
        for p in model.parameters():
            dist.broadcast(p.data, 0)
    best_state = copy.deepcopy(model.state_dict())                                              # train.py:203
    models.flatten_parameters(model)
    flat = dp.FlatGradients(model.parameters(), direct_write=True)       # the loop below zero_()s before every backward
    if lib_opt:
        optimizer = dp.LibAdam(model.parameters(), hp["lr"], max_norm=float(hp["clip_grad_norm"]), flat=flat)
    else:
        optimizer = dp.make_adam(model.parameters(), hp["lr"])                           # train.py:209
    criterion = (hooks["criterion_factory"](1.0 / ratio) if "criterion_factory" in hooks
                 else models.SymmetryLoss(1.0 / ratio, hp["alpha"]) if sym
                 else models.BCEWithLogitsLoss(pos_weight=1.0 / ratio))                         # train.py:210-211
    if sym:
        gap = torch.zeros(2, device=dev, dtype=torch.float64)          # the epoch's sum of parts[2] and its number of steps
        schedule = hp["symmetry_schedule"]

        def note_gap():
            gap[0] += criterion.last_parts[2].double()
            gap[1] += 1

        def sym_eval(graph, x, e, pe, y, acc):     # under no_grad: (loss, org) of one validation forward pair
            org = model(graph, x, e, pe).squeeze(-1)
            rev = model(graph, x, e, pe, reverse=True).squeeze(-1)
            loss = criterion.with_counts(org, rev, y, acc)[0] if acc is not None else criterion(org, rev, y)
            note_gap()
            return loss, org
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=hp["decay"],
                                                           patience=hp["patience"])             # train.py:212
    # one pass for loss + TP..FN + epoch sums; a criterion without with_counts (a criterion_factory stand-in) takes the torch route
    fused = bool(hp["fused_metrics"]) and hasattr(criterion, "with_counts")
    if fused:
        ep_stats, graph_stats = EpochStats(dev), EpochStats(dev)       # the epoch's sums; one graph's batches (mini-batch mode)
    ranking = bool(hp["ranking_metrics"])
    if ranking:
        rank_stats = RankingStats(dev)                                 # the validation epoch's logit histogram
    decision = bool(hp["decision_metrics"])
    if decision:
        dec_stats = DecisionStats(dev)                                 # the validation epoch's walk decisions
    assembly = bool(hp["assembly_metrics"])
    if assembly:
        asm_stats = AssemblyStats(dev)                                 # the validation epoch's best-overlap contigs
    if masking:
        # a generator of its own: the global `random` decides the shuffle order, which masking must not change
        mask_rng = random.Random(f"read-mask:{seed}")
        mask_key = engine.read_mask_key(seed)                          # the rank-mixed dropout key ^ a fixed constant
        recompute_pe = bool(hp["mask_recompute_pe"])
        draw_f = lambda: mask_rng.randint(mlo, mhi) / 100.0            # noqa: E731
    hist = History()
    order = list(range(len(train_samples)))
    model_path = os.path.join(workdir, "pretrained", f"model_{out}.pt")
    for epoch in range(hp["num_epochs"]):
        random.shuffle(order)                                                                   # train.py:238
        model.train()
        loss_sum = torch.zeros((), device=dev, dtype=torch.float64)
        counts = torch.zeros(4, device=dev, dtype=torch.int64)
        ep_losses = []                       # device scalars; read back once per epoch
        if fused:
            ep_stats.zero_()
        # every rank takes the same number of optimizer steps: shards may be uneven (dp.shard_graphs), the
        # shorter ranks pad with zero-contribution steps so that the gradient collectives stay matched
        nsteps = dp.steps_per_epoch(len(order), dev)
        # library route: every step leaves the gradient buffer zeroed (step(zero_grad=True)); only the epoch's first step zeroes it
        # explicitly -- validation and the hooks have run since the last one
        zero_first = True
        empty_steps = 0                      # masking: graphs whose thinned form had no edge (zero-contribution steps)
        ep_fracs, ep_edges = [], []
        if masking and hp["batch_size_train"] <= 1:
            # the epoch's thinned graphs, one per step, in step order; step k+1's is built on a side stream while step k runs
            ep_fracs = [draw_f() for _ in order]
            thinned = iter(cluster.MaskedGraphLoader([(_attach_features(train_samples[g]), f, g) for g, f in zip(order, ep_fracs)],
                                                     mask_key, epoch, recompute_pe=recompute_pe))
        for it in range(nsteps):
            s = train_samples[order[it]] if it < len(order) else None
            if masking and hp["batch_size_train"] <= 1 and s is not None:
                sub = next(thinned)
                ep_edges.append(sub.num_edges())
                if sub.num_edges() == 0:     # nothing to train on: a padding step, so that the collectives stay matched
                    s, empty_steps = None, empty_steps + 1
                else:
                    s = GraphSample(sub, sub.edata["e"], sub.ndata["pe"], sub.edata["y"])
            if hp["batch_size_train"] <= 1:                                                     # full graph
                if zero_first or not lib_opt:
                    flat.zero_()
                    zero_first = False
                if s is not None and sym:
                    loss, pred = symmetry_step(model, criterion, s.graph, s.x, s.e, s.pe, s.y, schedule, ep_stats if fused else None)
                    note_gap()
                elif s is not None:
                    pred = model(s.graph, s.x, s.e, s.pe).squeeze(-1)                           # train.py:252-253
                    loss = criterion.with_counts(pred, s.y, ep_stats)[0] if fused else criterion(pred, s.y)
                    loss.backward()
                flat.all_reduce_mean(contributed=s is not None)
                if "after_exchange" in hooks:
                    hooks["after_exchange"](epoch, it, flat)
                if lib_opt:
                    optimizer.step(zero_grad=True)
                else:
                    optimizer.step()                                                            # train.py:256-258
                if s is not None and fused:              # the loss kernel has added the step to ep_stats
                    ep_losses.append(loss.detach())
                    hist.step_graph.append(order[it])
                elif s is not None:
                    loss_sum += loss.detach().double()
                    ep_losses.append(loss.detach())
                    hist.step_graph.append(order[it])
                    counts += tfpn_counts(pred.detach(), s.y)
            else:                                                                               # train.py:282-343
                lo = max(1, hp["num_parts_metis_train"] - 100)
                nparts = int(torch.randint(lo, hp["num_parts_metis_train"] + 100, (1,)).item())  # train.py:291
                gl = torch.zeros((), device=dev, dtype=torch.float64)
                nb = 0
                rm = (mask_key, epoch, order[it], recompute_pe, draw_f) if masking and s is not None else None
                loader = _cluster_batches(s, nparts, hp["batch_size_train"], hp["partition_method"], rm) if s is not None else []
                nbatches = dp.steps_per_epoch(len(loader), dev)          # the ranks' cluster counts differ
                batches = iter(loader)
                if fused:
                    graph_stats.zero_()
                for _ in range(nbatches):
                    sub = next(batches, None)
                    if rm is not None and sub is not None:
                        ep_fracs.append(sub.relabel_info["mask_fraction"])
                        ep_edges.append(sub.num_edges())
                        if sub.num_edges() == 0:         # a thinned batch without an edge: a zero-contribution step
                            sub = None
                    if zero_first or not lib_opt:
                        flat.zero_()
                        zero_first = False
                    if sub is not None and sym:
                        loss, pred = symmetry_step(model, criterion, sub, None, sub.edata["e"], sub.ndata["pe"], sub.edata["y"],
                                                   schedule, graph_stats if fused else None)
                        note_gap()
                    elif sub is not None:
                        pred = model(sub, None, sub.edata["e"], sub.ndata["pe"]).squeeze(-1)    # train.py:306
                        loss = (criterion.with_counts(pred, sub.edata["y"], graph_stats)[0] if fused
                                else criterion(pred, sub.edata["y"]))
                        loss.backward()
                    flat.all_reduce_mean(contributed=sub is not None)
                    if lib_opt:
                        optimizer.step(zero_grad=True)
                    else:
                        optimizer.step()
                    if sub is not None and not fused:
                        gl += loss.detach().double()
                        nb += 1
                        counts += tfpn_counts(pred.detach(), sub.edata["y"])
                if s is not None and fused:              # once per graph, on the device: the mean of its batches, its counts
                    loss_sum += graph_stats.loss_sum / graph_stats.steps.clamp(min=1)
                    counts += graph_stats.counts
                elif s is not None:
                    loss_sum += gl / max(nb, 1)                                                 # train.py:330
        if fused and hp["batch_size_train"] <= 1:
            loss_sum, counts = ep_stats.loss_sum.clone(), ep_stats.counts.clone()
        n_train = torch.tensor(float(len(order) - empty_steps), device=dev, dtype=torch.float64)
        hist.mask_fraction += ep_fracs
        hist.masked_edges += ep_edges
        if world > 1:
            dist.all_reduce(loss_sum); dist.all_reduce(n_train); dist.all_reduce(counts)        # noqa: E702
        if sym:                              # one read per epoch
            if world > 1:
                dist.all_reduce(gap)
            hist.sym_gap_train.append(float(gap[0] / gap[1].clamp(min=1)))
            gap.zero_()
        train_loss = float(loss_sum / n_train.clamp(min=1)) if masking else float(loss_sum / n_train)
        hist.loss_train.append(train_loss)
        if lib_opt:                          # the step kernels' device record, read here with the losses and never per step
            st = optimizer.stats().cpu()
            hist.skipped_steps = int(st[2])
            hist.total_norm.append(float(st[0]))
        if ep_losses:
            hist.step_losses += torch.stack(ep_losses).double().cpu().tolist()
        hist.tfpn_train.append(tuple(int(c) for c in counts.tolist()))
        # (no counts at all: an epoch whose every thinned graph came out without an edge)
        hist.metrics_train.append(calculate_metrics(*hist.tfpn_train[-1]) if sum(hist.tfpn_train[-1]) or not masking else None)
        # ---- validation (train.py:385-511): eval mode, no_grad, no activations kept ----
        model.eval()
        vloss = torch.zeros((), device=dev, dtype=torch.float64)
        vcounts = torch.zeros(4, device=dev, dtype=torch.int64)
        if fused:
            ep_stats.zero_()
        if ranking:
            rank_stats.zero_()
        if decision:
            dec_stats.zero_()
        if assembly:
            asm_stats.zero_()
        with torch.no_grad():
            for s in valid_samples:
                if hp["batch_size_eval"] <= 1 and fused:
                    if sym:
                        pred = sym_eval(s.graph, s.x, s.e, s.pe, s.y, ep_stats)[1]
                    else:
                        pred = model(s.graph, s.x, s.e, s.pe).squeeze(-1)
                        criterion.with_counts(pred, s.y, ep_stats)
                    if ranking:
                        rank_stats.add(pred, s.y)
                    if decision:
                        dec_stats.add(s.graph, pred, s.y)
                    if assembly:
                        asm_stats.add(s.graph, pred, s.y)
                elif hp["batch_size_eval"] <= 1:
                    if sym:
                        vl, pred = sym_eval(s.graph, s.x, s.e, s.pe, s.y, None)
                        vloss += vl.double()
                    else:
                        pred = model(s.graph, s.x, s.e, s.pe).squeeze(-1)
                        vloss += criterion(pred, s.y).double()
                    vcounts += tfpn_counts(pred, s.y)
                    if ranking:
                        rank_stats.add(pred, s.y)
                    if decision:
                        dec_stats.add(s.graph, pred, s.y)
                    if assembly:
                        asm_stats.add(s.graph, pred, s.y)
                elif fused:
                    graph_stats.zero_()
                    for sub in _cluster_batches(s, hp["num_parts_metis_eval"], hp["batch_size_eval"],
                                                hp["partition_method"]):
                        if sym:
                            pred = sym_eval(sub, None, sub.edata["e"], sub.ndata["pe"], sub.edata["y"], graph_stats)[1]
                        else:
                            pred = model(sub, None, sub.edata["e"], sub.ndata["pe"]).squeeze(-1)
                            criterion.with_counts(pred, sub.edata["y"], graph_stats)
                        if ranking:
                            rank_stats.add(pred, sub.edata["y"])
                        if decision:
                            dec_stats.add(sub, pred, sub.edata["y"])
                    vloss += graph_stats.loss_sum / graph_stats.steps.clamp(min=1)
                    vcounts += graph_stats.counts
                else:                                                                           # train.py:428-486
                    gl = torch.zeros((), device=dev, dtype=torch.float64)
                    nb = 0
                    for sub in _cluster_batches(s, hp["num_parts_metis_eval"], hp["batch_size_eval"],
                                                hp["partition_method"]):
                        if sym:
                            bl, pred = sym_eval(sub, None, sub.edata["e"], sub.ndata["pe"], sub.edata["y"], None)
                            gl += bl.double()
                        else:
                            pred = model(sub, None, sub.edata["e"], sub.ndata["pe"]).squeeze(-1)
                            gl += criterion(pred, sub.edata["y"]).double()
                        nb += 1
                        vcounts += tfpn_counts(pred, sub.edata["y"])
                        if ranking:
                            rank_stats.add(pred, sub.edata["y"])
                        if decision:
                            dec_stats.add(sub, pred, sub.edata["y"])
                    vloss += gl / max(nb, 1)
        if fused and hp["batch_size_eval"] <= 1:
            vloss, vcounts = ep_stats.loss_sum.clone(), ep_stats.counts.clone()
        n_val = torch.tensor(float(len(valid_samples)), device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(vloss); dist.all_reduce(n_val); dist.all_reduce(vcounts)            # noqa: E702
        if sym:
            if world > 1:
                dist.all_reduce(gap)
            hist.sym_gap_valid.append(float(gap[0] / gap[1].clamp(min=1)))
            gap.zero_()
        if ranking:                              # the record adds across ranks like the counts; one read per epoch
            rm = rank_stats.all_reduce_().read()
            hist.auroc_valid.append(rm.auroc)
            hist.ap_valid.append(rm.average_precision)
            hist.best_f1_valid.append((rm.best_f1.f1, rm.best_f1.logit) if rm.best_f1 is not None else None)
        if decision:                             # 15 integers; they add across ranks like the counts; one read per epoch
            hist.decision_valid.append(dec_stats.all_reduce_().read().summary())
        if assembly:                             # eight integers summed, the pooled lengths gathered; once per epoch
            hist.assembly_valid.append(asm_stats.all_reduce_().summary())
        val_loss = float(vloss / n_val.clamp(min=1))
        hist.loss_valid.append(val_loss)
        hist.tfpn_valid.append(tuple(int(c) for c in vcounts.tolist()))
        hist.metrics_valid.append(calculate_metrics(*hist.tfpn_valid[-1]) if int(vcounts.sum()) else None)
        hist.lr.append(optimizer.param_groups[0]["lr"])
        if len(hist.loss_valid) > 1 and hist.loss_valid[-1] < min(hist.loss_valid[:-1]):        # train.py:525-527
            best_state = copy.deepcopy(model.state_dict())
            hist.best_epoch = epoch
            if rank == 0:
                os.makedirs(os.path.dirname(model_path), exist_ok=True)
                torch.save(best_state, model_path)
        if rank == 0:
            save_checkpoint(epoch, model, optimizer, train_loss, val_loss, out, os.path.join(workdir, "checkpoints"))
        scheduler.step(val_loss)                                                                # train.py:529
        hist.final_lr = optimizer.param_groups[0]["lr"]
        if "after_epoch" in hooks:
            hooks["after_epoch"](epoch, model)
        if verbose and rank == 0:
            print(f"epoch {epoch}: train loss {train_loss:.4f}  valid loss {val_loss:.4f}  lr {hist.lr[-1]:.2e}")
    return model, best_state, hist
