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
  * with the hyper-parameters "ranking_metrics", "decision_metrics" and "assembly_metrics" (defaults: GNM_RANKING_METRICS=1,
    GNM_DECISION_METRICS=1, GNM_ASSEMBLY_METRICS=1, else off) every validation forward also feeds its logits to an observer on the
    device (metrics.py: RankingStats, DecisionStats, AssemblyStats), read once per epoch: History gains AUROC, average precision and
    the best-F1 threshold / the greedy decode's branch accuracies / contig count, N50, longest contig and wrong-link share of the
    best-overlap contigs ("assembly_decoder": "greedy_cover", default GNM_ASSEMBLY_DECODER, else "best_overlap": of the greedy path
    cover instead; "assembly_reduce_transitive", default GNM_ASSEMBLY_REDUCE=1, else off: behind the string-graph reduction of
    decode.transitive_support, "assembly_reduce_fuzz" its length tolerance).  With batch_size_eval > 1 the decisions are counted on each batch's sub-graph and summed (a node at a cut
    sees only the candidates inside its batch) and "assembly_metrics" is refused (a cover across cluster cuts means nothing).  Under
    the symmetry loss the observers see the original scores.  Loss, schedule, best-model choice and every other History field are
    the same either way;
  * with the hyper-parameters "mask_frac_low" / "mask_frac_high" (per cent; default 100 / 100: off) every training step runs on the graph
    thinned to a random fraction of its READS (cluster.masked_subgraph: a device mask that is a pure function of seed, epoch, graph and
    read; the thinned graph's own degrees in `pe`), the next step's graph built on a side stream meanwhile (cluster.MaskedGraphLoader);
    a thinned graph without an edge is a zero-contribution step; validation is never masked; History gains mask_fraction / masked_edges;
  * wandb and the data pipeline are out of scope.
The counts, records and metric classes the loop uses live in metrics.py and are re-exported here."""
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
from .metrics import (ASSEMBLY_DECODERS, ASSEMBLY_MIN_NODES, DECISION_COUNTERS, DECISION_RECORD_WORDS, RANK_BINS, AssemblyStats, BestF1,  # noqa: F401
                      DecisionCounts, DecisionMetrics, DecisionStats, EpochStats, RankingMetrics, RankingStats, _ratio,
                      calculate_metrics, rank_bin_lower_edge, tfpn_counts)

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
        # ... of which decoder: "best_overlap" (mutual-best links, decode.best_overlap_contigs) or "greedy_cover" (those links iterated
        # to the greedy path cover, decode.greedy_cover_contigs); only read when assembly_metrics is on
        "assembly_decoder": os.environ.get("GNM_ASSEMBLY_DECODER", "").strip().lower() or "best_overlap",
        # ... behind the string-graph reduction of the candidate edges (decode.transitive_support): no link jumps over a read that a
        # two-step path of shorter prefix reaches; "assembly_reduce_fuzz": None, or the bases by which the two steps' prefixes may
        # miss the edge's; both only read when assembly_metrics is on
        "assembly_reduce_transitive": os.environ.get("GNM_ASSEMBLY_REDUCE", "0").strip() == "1",
        "assembly_reduce_fuzz": None,
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


def _check_hyperparameters(hp: Dict, hooks: Dict, train_samples, valid_samples) -> None:
    """ValueError for what train() refuses, before it seeds or builds anything: the optimizer and its clipping, the mask fractions, the
    decision / assembly metrics and what the latter needs on the validation graphs, the symmetry loss (check_symmetry_hyperparameters),
    and last -- only these look at a sample -- the metrics that have no CPU route."""
    if hp["optimizer"] not in ("torch", "library"):
        raise ValueError(f"hyper-parameter optimizer={hp['optimizer']!r}: expected 'torch' or 'library'")
    if not float(hp["clip_grad_norm"]) >= 0.0:
        raise ValueError(f"hyper-parameter clip_grad_norm={hp['clip_grad_norm']!r}: expected a number >= 0 (0: off)")
    if hp["clip_grad_norm"] > 0 and hp["optimizer"] != "library":
        raise ValueError("hyper-parameter clip_grad_norm > 0 needs \"optimizer\": \"library\": the torch route does not clip, and "
                         "the value is not silently ignored")
    mlo, mhi = hp["mask_frac_low"], hp["mask_frac_high"]
    if not (isinstance(mlo, int) and isinstance(mhi, int) and 1 <= mlo <= mhi <= 100):
        raise ValueError(f"hyper-parameters mask_frac_low={mlo!r}, mask_frac_high={mhi!r}: expected integers (per cent) with "
                         "1 <= low <= high <= 100 (100 / 100: no masking)")
    if not isinstance(hp["decision_metrics"], (bool, np.bool_)):
        raise ValueError(f"hyper-parameter decision_metrics={hp['decision_metrics']!r}: expected True or False")
    if not isinstance(hp["assembly_metrics"], (bool, np.bool_)):
        raise ValueError(f"hyper-parameter assembly_metrics={hp['assembly_metrics']!r}: expected True or False")
    if hp["assembly_decoder"] not in ASSEMBLY_DECODERS:
        raise ValueError(f"hyper-parameter assembly_decoder={hp['assembly_decoder']!r}: expected one of {ASSEMBLY_DECODERS}")
    if not isinstance(hp["assembly_reduce_transitive"], (bool, np.bool_)):
        raise ValueError(f"hyper-parameter assembly_reduce_transitive={hp['assembly_reduce_transitive']!r}: expected True or False")
    engine.reduce_fuzz_word(hp["assembly_reduce_fuzz"], "hyper-parameter assembly_reduce_fuzz")
    if hp["assembly_metrics"]:
        if hp["batch_size_eval"] > 1:
            raise ValueError("hyper-parameter assembly_metrics=True with batch_size_eval > 1: the contigs are decoded on the whole "
                             "validation graph; a cover across cluster cuts means nothing")
        for i, s in enumerate(valid_samples):
            for where, key in (("edata", "prefix_length"), ("ndata", "read_length")):
                if key not in getattr(s.graph, where, {}):
                    raise ValueError(f"hyper-parameter assembly_metrics=True: validation sample {i} has no graph.{where}[{key!r}]")
    if check_symmetry_hyperparameters(hp) and "criterion_factory" in hooks:
        raise ValueError("hyper-parameter symmetry_loss with a \"criterion_factory\" hook: the symmetry loss is models.SymmetryLoss")
    if hp["decision_metrics"] and train_samples[0].pe.device.type != "cuda":
        raise ValueError(f"hyper-parameter decision_metrics=True with the samples on {train_samples[0].pe.device}: the decisions are "
                         "counted by a kernel (gnm_decision_stats) and need a HIP device; there is no CPU route")
    if hp["assembly_metrics"] and train_samples[0].pe.device.type != "cuda":
        raise ValueError(f"hyper-parameter assembly_metrics=True with the samples on {train_samples[0].pe.device}: the contigs are "
                         "decoded by kernels (gnm_decision_stats, gnm_bog_contigs) and need a HIP device; there is no CPU route")


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
    mask_fraction: List[float] = field(default_factory=list)    # "mask_frac_*": the kept read fraction f of every step of this rank on a graph or batch;
                                                                # added once per epoch; empty when it is off
    sym_gap_train: List[float] = field(default_factory=list)    # "symmetry_loss": per epoch the mean over the steps of mean_k |org_k - rev_k| (the
    sym_gap_valid: List[float] = field(default_factory=list)    # loss's parts[2], unscaled by alpha), training / validation; empty when it is off
    masked_edges: List[int] = field(default_factory=list)       # "mask_frac_*": beside every entry of mask_fraction, the edge count of the thinned graph the
                                                                # step ran on (0: a zero-contribution step, which has no entry in step_losses / step_graph)


def _whole(s: GraphSample):
    """What a forward pass on the sample's whole graph takes: (graph, x, e, pe, y)."""
    return s.graph, s.x, s.e, s.pe, s.y


def _batch(sub):
    """... and on a sub-graph that carries its features (a cluster batch, a thinned graph)."""
    return sub, None, sub.edata["e"], sub.ndata["pe"], sub.edata["y"]


def _add_graph_mean(ep: EpochStats, graph: EpochStats):
    """Mini-batch mode, once per graph and on the device: the mean loss of the graph's batches and their counts join the epoch's
    (train.py:330)."""
    ep.loss_sum += graph.loss_sum / graph.steps.clamp(min=1)
    ep.counts += graph.counts


def _ranking_entries(stats: RankingStats) -> Dict:
    rm = stats.read()
    return {"auroc_valid": rm.auroc, "ap_valid": rm.average_precision,
            "best_f1_valid": (rm.best_f1.f1, rm.best_f1.logit) if rm.best_f1 is not None else None}


# The validation observers: the hyper-parameter that switches one on, its record (zero_() before an epoch's validation, all_reduce_()
# after it: the records add across ranks like the counts), how the record takes the scores of a (sub-)graph, and the History entries
# of an epoch, read from the reduced record.  Assembly is full-graph only (_check_hyperparameters).
_OBSERVERS = (
    ("ranking_metrics", RankingStats, lambda st, graph, pred, y: st.add(pred, y), _ranking_entries),
    ("decision_metrics", DecisionStats, lambda st, graph, pred, y: st.add(graph, pred, y), lambda st: {"decision_valid": st.read().summary()}),
    ("assembly_metrics", AssemblyStats, lambda st, graph, pred, y: st.add(graph, pred, y), lambda st: {"assembly_valid": st.summary()}),
)


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
    _check_hyperparameters(hp, hooks, train_samples, valid_samples)
    lib_opt = hp["optimizer"] == "library"
    mlo, mhi = hp["mask_frac_low"], hp["mask_frac_high"]
    masking = not (mlo == 100 and mhi == 100)
    sym = bool(hp["symmetry_loss"])
    full_train, full_eval = hp["batch_size_train"] <= 1, hp["batch_size_eval"] <= 1
    seed = hp["seed"]
    random.seed(seed)
    torch.manual_seed(seed)                                                     # utils.set_seed
    dev = train_samples[0].pe.device
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
    flat = dp.FlatGradients(model.parameters(), direct_write=True)       # zeroed before every backward (step() below)
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

        def note_gap():                      # after every symmetry step or evaluation that really ran
            gap[0] += criterion.last_parts[2].double()
            gap[1] += 1

        def read_gap():                      # one read per pass (training, validation), then zeroed for the next
            if world > 1:
                dist.all_reduce(gap)
            mean = float(gap[0] / gap[1].clamp(min=1))
            gap.zero_()
            return mean
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=hp["decay"],
                                                           patience=hp["patience"])             # train.py:212
    # one pass for loss + TP..FN + epoch sums; a criterion without with_counts (a criterion_factory stand-in) takes the torch route
    fused = bool(hp["fused_metrics"]) and hasattr(criterion, "with_counts")
    # {fp64 loss sum, steps, TP..FN} of the pass under way (training, then validation) and of one graph's batches (mini-batch mode):
    # filled by the loss kernel (fused), or by record() below
    ep_stats, graph_stats = EpochStats(dev), EpochStats(dev)
    observers = [(cls(dev, decoder=hp["assembly_decoder"], reduce_transitive=bool(hp["assembly_reduce_transitive"]),
                      fuzz=hp["assembly_reduce_fuzz"]) if cls is AssemblyStats else cls(dev), add, entries)
                 for key, cls, add, entries in _OBSERVERS if hp[key]]
    if masking:
        # a generator of its own: the global `random` decides the shuffle order, which masking must not change
        mask_rng = random.Random(f"read-mask:{seed}")
        mask_key = engine.read_mask_key(seed)                          # the rank-mixed dropout key ^ a fixed constant
        recompute_pe = bool(hp["mask_recompute_pe"])
        draw_f = lambda: mask_rng.randint(mlo, mhi) / 100.0            # noqa: E731

    def record(rec, loss, pred, y):
        """The torch-metrics route: add to `rec` what the loss kernel adds on the fused route."""
        rec.loss_sum += loss.detach().double()
        rec.steps += 1
        rec.counts += tfpn_counts(pred.detach(), y)

    def step(sample, rec, epoch, it=None):
        """One optimizer step on sample = (graph, x, e, pe, y), or on None: a zero-contribution step, so that the collectives stay
        matched.  `rec` collects the step's loss and counts; it: the number of a full-graph step (the "after_exchange" hook is
        full-graph only).  Returns the detached loss, or None."""
        if not lib_opt:                      # the library's step leaves the gradient buffer zeroed itself
            flat.zero_()
        if sample is not None:
            graph, x, e, pe, y = sample
            if sym:
                loss, pred = symmetry_step(model, criterion, graph, x, e, pe, y, schedule, rec if fused else None)
                note_gap()
            else:
                pred = model(graph, x, e, pe).squeeze(-1)                                       # train.py:252-253
                loss = criterion.with_counts(pred, y, rec)[0] if fused else criterion(pred, y)
                loss.backward()
        flat.all_reduce_mean(contributed=sample is not None)
        if it is not None and "after_exchange" in hooks:
            hooks["after_exchange"](epoch, it, flat)
        if lib_opt:
            optimizer.step(zero_grad=True)
        else:
            optimizer.step()                                                                    # train.py:256-258
        if sample is None:
            return None
        if not fused:
            record(rec, loss, pred, y)
        return loss.detach()

    def evaluate(sample, rec):
        """Under no_grad: the forward and the loss of one (sub-)graph, added to `rec` -- under the symmetry loss the forward pair,
        and its gap is noted -- then the observers take the (original) scores."""
        graph, x, e, pe, y = sample
        pred = model(graph, x, e, pe).squeeze(-1)
        args = (pred, model(graph, x, e, pe, reverse=True).squeeze(-1), y) if sym else (pred, y)
        loss = criterion.with_counts(*args, rec)[0] if fused else criterion(*args)
        if sym:
            note_gap()
        if not fused:
            record(rec, loss, pred, y)
        for stats, add, _ in observers:
            add(stats, graph, pred, y)

    hist = History()
    order = list(range(len(train_samples)))
    model_path = os.path.join(workdir, "pretrained", f"model_{out}.pt")
    for epoch in range(hp["num_epochs"]):
        random.shuffle(order)                                                                   # train.py:238
        model.train()
        ep_stats.zero_()
        ep_losses = []                       # device scalars; read back once per epoch
        # every rank takes the same number of optimizer steps: shards may be uneven (dp.shard_graphs), the
        # shorter ranks pad with zero-contribution steps so that the gradient collectives stay matched
        nsteps = dp.steps_per_epoch(len(order), dev)
        if lib_opt:                          # validation and the hooks have run since the last step left the gradient buffer zeroed
            flat.zero_()
        empty_steps = 0                      # masking: graphs whose thinned form had no edge (zero-contribution steps)
        ep_fracs, ep_edges = [], []
        if masking and full_train:
            # the epoch's thinned graphs, one per step, in step order; step k+1's is built on a side stream while step k runs
            ep_fracs = [draw_f() for _ in order]
            thinned = iter(cluster.MaskedGraphLoader([(_attach_features(train_samples[g]), f, g) for g, f in zip(order, ep_fracs)],
                                                     mask_key, epoch, recompute_pe=recompute_pe))
        for it in range(nsteps):
            s = train_samples[order[it]] if it < len(order) else None
            if full_train:
                sample = _whole(s) if s is not None else None
                if masking and s is not None:
                    sub = next(thinned)
                    ep_edges.append(sub.num_edges())
                    sample = _batch(sub) if sub.num_edges() else None        # no edge, nothing to train on: a padding step
                    empty_steps += sample is None
                loss = step(sample, ep_stats, epoch, it)
                if sample is not None:
                    ep_losses.append(loss)
                    hist.step_graph.append(order[it])
            else:                                                                               # train.py:282-343
                lo = max(1, hp["num_parts_metis_train"] - 100)
                nparts = int(torch.randint(lo, hp["num_parts_metis_train"] + 100, (1,)).item())  # train.py:291; on padding steps too
                rm = (mask_key, epoch, order[it], recompute_pe, draw_f) if masking and s is not None else None
                loader = _cluster_batches(s, nparts, hp["batch_size_train"], hp["partition_method"], rm) if s is not None else []
                nbatches = dp.steps_per_epoch(len(loader), dev)          # the ranks' cluster counts differ
                batches = iter(loader)
                graph_stats.zero_()
                for _ in range(nbatches):
                    sub = next(batches, None)
                    if rm is not None and sub is not None:
                        ep_fracs.append(sub.relabel_info["mask_fraction"])
                        ep_edges.append(sub.num_edges())
                        if sub.num_edges() == 0:         # a thinned batch without an edge: a zero-contribution step
                            sub = None
                    step(_batch(sub) if sub is not None else None, graph_stats, epoch)
                if s is not None:
                    _add_graph_mean(ep_stats, graph_stats)
        loss_sum, counts = ep_stats.loss_sum.clone(), ep_stats.counts.clone()
        n_train = torch.tensor(float(len(order) - empty_steps), device=dev, dtype=torch.float64)
        hist.mask_fraction += ep_fracs
        hist.masked_edges += ep_edges
        if world > 1:
            dist.all_reduce(loss_sum); dist.all_reduce(n_train); dist.all_reduce(counts)        # noqa: E702
        if sym:
            hist.sym_gap_train.append(read_gap())
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
        ep_stats.zero_()
        for stats, _, _ in observers:
            stats.zero_()
        with torch.no_grad():
            for s in valid_samples:
                if full_eval:
                    evaluate(_whole(s), ep_stats)
                else:                                                                           # train.py:428-486
                    graph_stats.zero_()
                    for sub in _cluster_batches(s, hp["num_parts_metis_eval"], hp["batch_size_eval"], hp["partition_method"]):
                        evaluate(_batch(sub), graph_stats)
                    _add_graph_mean(ep_stats, graph_stats)
        vloss, vcounts = ep_stats.loss_sum.clone(), ep_stats.counts.clone()
        n_val = torch.tensor(float(len(valid_samples)), device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(vloss); dist.all_reduce(n_val); dist.all_reduce(vcounts)            # noqa: E702
        if sym:
            hist.sym_gap_valid.append(read_gap())
        for stats, _, entries in observers:      # one reduction and one read per observer and epoch
            for name, value in entries(stats.all_reduce_()).items():
                getattr(hist, name).append(value)
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
