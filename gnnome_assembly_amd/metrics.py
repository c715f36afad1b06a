"""What the training loop (train.py) counts and reports, apart from the loop itself: the TP..FN counts and the reference's metrics
(tfpn_counts, calculate_metrics), the device record of an epoch's sums (EpochStats), and the three observers of the validation
logits with their host-side figures -- RankingStats / RankingMetrics / BestF1 (a histogram of the logits: AUROC, average precision,
best-F1 threshold), DecisionStats / DecisionMetrics / DecisionCounts (the greedy decode's choices) and AssemblyStats (the
best-overlap contigs).  Every name here is re-exported by train.py.
`calculate_metrics` keeps the reference's naming, in which "precision" and "recall" are swapped (utils.py:227-234)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import engine
from .engine import DECISION_COUNTERS, DECISION_RECORD_WORDS, RANK_BINS


def tfpn_counts(edge_predictions: torch.Tensor, edge_labels: torch.Tensor) -> torch.Tensor:
    """[TP, TN, FP, FN] as a device int64 tensor (utils.calculate_tfpn without the .item() syncs)."""
    p = torch.round(torch.sigmoid(edge_predictions))
    return torch.stack([((p == 1) & (edge_labels == 1)).sum(), ((p == 0) & (edge_labels == 0)).sum(),
                        ((p == 1) & (edge_labels == 0)).sum(), ((p == 0) & (edge_labels == 1)).sum()])


def calculate_metrics(TP, TN, FP, FN):
    """utils.calculate_metrics (utils.py:226-240), including its swapped precision/recall names."""
    recall = TP / (TP + FP) if (TP + FP) else 0
    precision = TP / (TP + FN) if (TP + FN) else 0
    f1 = TP / (TP + 0.5 * (FP + FN)) if (TP + 0.5 * (FP + FN)) else 0
    accuracy = (TP + TN) / (TP + TN + FP + FN)
    return accuracy, precision, recall, f1


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
        engine.rank_hist(scores.detach(), y, self.buf)
        return self

    def all_reduce_(self):
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.buf)
        return self

    def read(self) -> RankingMetrics:
        b = self.buf.cpu().numpy()
        return RankingMetrics.from_counts(b[:2 * RANK_BINS], b[2 * RANK_BINS:])


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
ASSEMBLY_DECODERS = ("best_overlap", "greedy_cover")    # the hyper-parameter "assembly_decoder": which cover AssemblyStats decodes


class AssemblyStats:
    """The best-overlap contigs of an epoch's validation graphs: `rec`, the sum of their gnm_bog_records (int64 [8], host), and the
    bases of the contigs of at least `min_nodes` nodes, pooled.  add() decodes one graph on the device (decode.best_overlap_contigs:
    one host synchronisation; with decoder="greedy_cover" decode.greedy_cover_contigs, the mutual-best links iterated to the greedy
    path cover: one more synchronisation per chunk of rounds; with reduce_transitive=True either decoder runs behind
    decode.transitive_support's string-graph reduction, `fuzz` its length tolerance, and `reduce_rec` sums the gnm_reduce_records of
    this process) and needs a HIP device.  Under torch.distributed all_reduce_() sums the records and gathers the pooled
    lengths (all_gather_object), once per epoch."""

    def __init__(self, device, min_nodes: int = ASSEMBLY_MIN_NODES, decoder: str = "best_overlap", reduce_transitive: bool = False,
                 fuzz=None):
        from .decode import _reduce_args
        if decoder not in ASSEMBLY_DECODERS:
            raise ValueError(f"AssemblyStats: decoder {decoder!r}: expected one of {ASSEMBLY_DECODERS}")
        _reduce_args("AssemblyStats", reduce_transitive, fuzz)
        self.device = torch.device(device)
        self.min_nodes = int(min_nodes)
        self.decoder = decoder
        self.reduce_transitive, self.fuzz = bool(reduce_transitive), fuzz
        self.zero_()

    def zero_(self):
        self.rec = np.zeros(engine.BOG_RECORD_WORDS, np.int64)
        self.reduce_rec = np.zeros(engine.REDUCE_RECORD_WORDS, np.int64)   # the sum of the gnm_reduce_records; moves only when reduce_transitive
        self.bases: List[int] = []
        self.wrong: List[int] = []
        return self

    def add(self, graph, scores, y=None):
        from . import decode
        cover = decode.greedy_cover_contigs if self.decoder == "greedy_cover" else decode.best_overlap_contigs
        extra = dict(reduce_transitive=True, fuzz=self.fuzz) if self.reduce_transitive else {}
        c = cover(graph, scores.detach(), graph.edata["prefix_length"], graph.ndata["read_length"], y, **extra)
        self.rec += np.asarray(c.stats.words(), np.int64)
        if self.reduce_transitive:
            w = np.asarray(c.reduce_stats.words(), np.int64)
            k = engine.REDUCE_COUNTERS.index("max_support")
            w[k] = max(int(w[k]), int(self.reduce_rec[k])) - int(self.reduce_rec[k])   # a maximum, not a sum
            self.reduce_rec += w
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
        links, wrong = (int(self.rec[engine.BOG_COUNTERS.index(k)]) for k in ("links", "wrong_links"))
        return (len(self.bases), n50(self.bases), max(self.bases, default=0), _ratio(wrong, links))
