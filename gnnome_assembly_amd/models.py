"""Host-side mirror of the reference's `models` package (models/full_graph.py)."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

import torch.nn.functional as F

from . import dp, engine, layers
from .graph import as_assembly_graph

__all__ = ["GraphGatedGCNModel", "BCEWithLogitsLoss", "SymmetryLoss", "flatten_parameters", "mirror_state", "mirror_index"]


def _engine_order(names):
    """Parameter names in the order the kernels like them in memory: per layer the five stacked projection weights
    (A_1 A_2 A_3 B_1 B_2: one [5H,H] operand), their five biases ([5H]), then the rest; encoders and predictor last."""
    rank = {}
    for k in names:
        parts = k.split(".")
        if parts[0] == "gnn":
            layer, mod, kind = int(parts[2]), parts[3], parts[4]
            if mod in engine.LIN5:
                rank[k] = (0, layer, 0 if kind == "weight" else 1, engine.LIN5.index(mod))
            else:
                rank[k] = (0, layer, 2, names.index(k))
        else:
            rank[k] = (1, 0, 0, names.index(k))
    return sorted(names, key=lambda k: rank[k])


def flatten_parameters(model: nn.Module) -> torch.Tensor:
    """Move every parameter of `model` into ONE contiguous fp32 buffer (values preserved; each parameter becomes a
    view of it) laid out in _engine_order, so that the engine takes [5H,H] / [5H] views of the stacked projection
    parameters instead of torch.cat-ing them on every pass, and dp.FlatGradients (which follows the same order)
    can hand the kernels gradient targets of the same shape.  Returns the buffer.  state_dict keys, optimizers
    and load_state_dict are unaffected; model.to(device) un-flattens (the next forward flattens again)."""
    named = dict(model.named_parameters())
    order = _engine_order(list(named))
    dev = next(iter(named.values())).device
    flat = torch.empty(sum(p.numel() for p in named.values()), dtype=torch.float32, device=dev)
    o = 0
    with torch.no_grad():
        for slot, k in enumerate(order):
            p = named[k]
            v = flat[o:o + p.numel()].view_as(p)
            v.copy_(p.data)
            p.data = v
            p._gnm_slot = slot
            o += p.numel()
    model._gnm_flat = flat
    return flat


def _is_flat(model: nn.Module) -> bool:
    flat = getattr(model, "_gnm_flat", None)
    if flat is None:
        return False
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    return all(p.device == flat.device and lo <= p.data_ptr() < hi for p in model.parameters())


_MIRROR_PAIRS = {"A_2": "A_3", "A_3": "A_2", "B_1": "B_2", "B_2": "B_1"}


def _mirror_key(name: str) -> str:
    parts = name.split(".")
    if len(parts) == 5 and parts[0] == "gnn" and parts[3] in _MIRROR_PAIRS:
        parts[3] = _MIRROR_PAIRS[parts[3]]
        return ".".join(parts)
    return name


def mirror_state(named):
    """The parameter mirror M: name -> tensor of a GraphGatedGCNModel (a state dict, dict(model.named_parameters()), a dict of
    gradients) to name -> mirrored tensor, with scores(reverse(g); theta) = scores(g; M theta) on a graph whose in- and out-degree
    columns of `pe` are left where they are.  Every edge (s -> d) of reverse(g) is (d -> s), so in every layer B_1 <-> B_2 (the
    edge update reads h[d] where it read h[s]) and A_2 <-> A_3 (the by-destination and the by-source sums trade places; h is
    symmetric in them), the predictor's first two H-wide column blocks of W1 trade places (cat(x[src], x[dst], e)), and columns
    0 and 1 of linear_pe.weight do (in-degree | out-degree).  Everything else is untouched.  Views and index ops: differentiable,
    and an involution: mirror_state(mirror_state(d)) == d.  The gradient follows as dL/d theta = M (dL/d theta' at theta' = M theta)."""
    out = {}
    for k, v in named.items():
        if k == "linear_pe.weight":
            idx = torch.arange(v.shape[1], device=v.device)
            idx[0], idx[1] = 1, 0
            out[k] = v.index_select(1, idx)
        elif k == "predictor.W1.weight":
            H = v.shape[1] // 3
            out[k] = torch.cat([v[:, H:2 * H], v[:, :H], v[:, 2 * H:]], 1)
        else:
            out[k] = named[_mirror_key(k)]
    return out


def _flat_offsets(model: nn.Module):
    """[(name, parameter, element offset in model._gnm_flat)] of a flattened model, in the buffer's order."""
    base = model._gnm_flat.data_ptr()
    rows = [(k, p, (p.data_ptr() - base) // 4) for k, p in model.named_parameters()]
    return sorted(rows, key=lambda r: r[2])


def _mirror_of(model: nn.Module):
    """(pi, flat buffer, {name: element offset}, scratch holder) of a flattened model: what a reversed pass needs, built once per
    flattening and kept on the model.  The holder keeps the backward's flat scratch buffer between steps."""
    if not _is_flat(model):
        raise RuntimeError("mirror_index: the model is not flattened (models.flatten_parameters)")
    flat = model._gnm_flat
    cached = getattr(model, "_gnm_mirror", None)
    if cached is not None and cached[1] is flat:
        return cached
    rows = _flat_offsets(model)
    ids = {k: torch.arange(o, o + p.numel(), dtype=torch.int64).view(p.shape) for k, p, o in rows}
    m = mirror_state(ids)
    pi = torch.cat([m[k].reshape(-1) for k, _, _ in rows]).to(torch.int32).to(flat.device)
    model._gnm_mirror = (pi, flat, {k: o for k, _, o in rows}, {})
    return model._gnm_mirror


def mirror_index(model: nn.Module) -> torch.Tensor:
    """The mirror as a permutation of the flat parameter buffer: int32 [n] on the buffer's device with
    model._gnm_flat[pi] == the flattened mirror_state(parameters) and pi[pi] == arange (in the layout of _engine_order the five
    stacked projections of a layer are the block order (0, 2, 1, 4, 3), weights and biases alike).  Built once per flattening and
    kept on the model."""
    return _mirror_of(model)[0]


class _ModelFn(torch.autograd.Function):
    """Whole-model forward/backward: the edge stream stays in internal order from the encoder
    to the predictor, activations are released layer by layer in backward."""

    @staticmethod
    def forward(ctx, graph, e, pe, num_layers, names, need, norm, *flat):
        # `need` (grad mode on and some parameter or input e / pe requires grad) is decided by the caller: inside
        # Function.forward grad mode is always off, and needs_input_grad stays set under no_grad.
        # norm = (batch_norm, real hidden width): LayerNorm statistics run over the model's real width when the kernels
        # run it zero-padded to the next width up (gated_gcn_full.py:58-59: nn.LayerNorm(out_channels)); its third entry is the
        # model's activation_checkpoint (it rides here so that the positional layout backward() counts on stays as it is)
        batch_norm, ln_width, checkpoint, *wl = norm       # a fourth entry: the layers' WIDE_LAYERNORM decision (GatedGCN_1d._wide_ln)
        P = {k: v.detach() for k, v in zip(names, flat)}            # a fifth: this forward's node-output dropout (p, key, step) or None
        mirror = wl[2] if len(wl) > 2 else None                     # a sixth: reverse=True on a flat model: _mirror_of(model)
        if mirror is not None:
            # the reversed pass: the same kernels on the mirrored copy of the flat buffer (one gather launch), cut into views of
            # the same layout -- the five stacked projections stay one [5H,H] operand
            pi, buf, offs, _ = mirror
            mflat = engine.mirror_gather(buf, pi)
            P = {k: mflat[offs[k]:offs[k] + v.numel()].view(v.shape) for k, v in zip(names, flat)}
        ctx.mirror = mirror
        scores, saved = engine.model_forward(graph, e.detach(), pe.detach(), P, num_layers, need, batch_norm, ln_width=ln_width,
                                             checkpoint=checkpoint, wide_ln=wl[0] if wl else None,
                                             dropout=wl[1] if len(wl) > 1 else None)
        ctx.graph, ctx.saved, ctx.P, ctx.names, ctx.L, ctx.bn, ctx.lnw = graph, saved, P, names, num_layers, batch_norm, ln_width
        ctx.params = flat if need else None
        return scores

    @staticmethod
    def backward(ctx, gscores):
        if ctx.saved is None:
            raise RuntimeError("GraphGatedGCNModel: backward called twice or forward ran without grad")
        # Fast path: every .grad is a view of a dp.FlatGradients buffer that has been zeroed since its last use
        # (the training loops call flat.zero_() before each backward) -> the kernels write the gradients straight
        # into those views and autograd is told "no gradient": accumulating x into zeros is x, and the ~140
        # accumulation kernels per step disappear.  Anything else takes the ordinary autograd route.
        # Input gradients (e at position 1, pe at 2): the encoders' backward also writes them when asked for.
        want_e, want_pe = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        inputs = want_e or want_pe
        if ctx.mirror is not None:
            return _ModelFn._backward_mirrored(ctx, gscores, want_e, want_pe)
        fg = dp.fresh_flat_gradients(ctx.params)
        if fg is not None and all(ctx.needs_input_grad[7:]):
            out = {k: p.grad for k, p in zip(ctx.names, ctx.params)}
            r = engine.model_backward(ctx.graph, ctx.P, ctx.L, ctx.saved, gscores, ctx.bn, out=out, ln_width=ctx.lnw, inputs=inputs)
            fg.fresh = False
            ctx.saved = None
            _, ge, gpe = r if inputs else (r, None, None)
            return (None, ge if want_e else None, gpe if want_pe else None) + (None,) * (4 + len(ctx.names))
        r = engine.model_backward(ctx.graph, ctx.P, ctx.L, ctx.saved, gscores, ctx.bn, ln_width=ctx.lnw, inputs=inputs)
        ctx.saved = None
        G, ge, gpe = r if inputs else (r, None, None)
        return (None, ge if want_e else None, gpe if want_pe else None, None, None, None, None) + tuple(G[k] for k in ctx.names)

    @staticmethod
    def _backward_mirrored(ctx, gscores, want_e, want_pe):
        """The backward of a pass that ran on M theta: dL/d theta = M (dL/d theta').  With a direct-write dp.FlatGradients in the
        model's layout the kernels write dL/d theta' into a scratch buffer of that layout and ONE launch folds it,
        grad[i] += scratch[pi[i]] -- an accumulation, right whether or not the buffer already holds the original pass's
        gradient; it leaves the buffer not fresh.  Otherwise autograd gets M of the gradients."""
        inputs = want_e or want_pe
        pi, buf, offs, hold = ctx.mirror
        fg = dp.flat_gradients_of(ctx.params) if all(ctx.needs_input_grad[7:]) else None
        if fg is not None and fg.grads.numel() == buf.numel() and all(
                (p.grad.data_ptr() - fg.flat.data_ptr()) // 4 == offs[k] for k, p in zip(ctx.names, ctx.params)):
            sg = hold.get("scratch")          # one backward at a time per device (engine.model_backward): the buffer is reused
            if sg is None:
                sg = hold["scratch"] = torch.empty_like(buf)
            sg.zero_()
            out = {k: sg[offs[k]:offs[k] + p.numel()].view(p.shape) for k, p in zip(ctx.names, ctx.params)}
            r = engine.model_backward(ctx.graph, ctx.P, ctx.L, ctx.saved, gscores, ctx.bn, out=out, ln_width=ctx.lnw, inputs=inputs)
            engine.mirror_add(fg.grads, sg, pi)
            fg.fresh = False
            ctx.saved = None
            _, ge, gpe = r if inputs else (r, None, None)
            return (None, ge if want_e else None, gpe if want_pe else None) + (None,) * (4 + len(ctx.names))
        r = engine.model_backward(ctx.graph, ctx.P, ctx.L, ctx.saved, gscores, ctx.bn, ln_width=ctx.lnw, inputs=inputs)
        ctx.saved = None
        G, ge, gpe = r if inputs else (r, None, None)
        G = mirror_state(G)
        return (None, ge if want_e else None, gpe if want_pe else None, None, None, None, None) + tuple(G[k] for k in ctx.names)


def _pad_param(name: str, v: torch.Tensor, H: int, Hp: int) -> torch.Tensor:
    """One parameter of a width-H model as the parameter of the width-Hp model whose extra channels are dead."""
    d = Hp - H
    leaf = name.split(".")[-2] if "." in name else name
    if name.startswith("predictor.W1.weight"):                     # [hs, 3H]: three H-wide blocks (x[src] | x[dst] | e)
        return F.pad(v.reshape(v.shape[0], 3, H), (0, d)).reshape(v.shape[0], 3 * Hp)
    if name.startswith(("predictor.", "linear1_edge.")):
        return v
    if name.startswith(("linear_pe.", "linear2_edge.")):           # [H, in] / [H]: new output rows
        return F.pad(v, (0, 0, 0, d)) if v.dim() == 2 else F.pad(v, (0, d))
    if leaf in ("bn_h", "bn_e"):
        return F.pad(v, (0, d), value=1.0 if name.endswith("weight") else 0.0)
    return F.pad(v, (0, d, 0, d)) if v.dim() == 2 else F.pad(v, (0, d))     # [H, H] layer weights, [H] biases


def _default_checkpoint():
    """GraphGatedGCNModel.activation_checkpoint of a new model: GNM_CHECKPOINT, unset = 0.  A value that is no integer is kept as it
    is and refused where it is used (engine.model_forward)."""
    v = os.environ.get("GNM_CHECKPOINT", "").strip()
    try:
        return int(v) if v else 0
    except ValueError:
        return v


class GraphGatedGCNModel(nn.Module):
    """models/full_graph.py:11-29.  forward(graph, x, e, pe) -> scores [E,1] (edge-id order).

    `graph` is an AssemblyGraph (or anything AssemblyGraph-compatible on a HIP device); `x` is
    ignored exactly as in the reference (full_graph.py:23 overwrites it).

    `activation_checkpoint` (a plain int attribute, default 0 or the environment's GNM_CHECKPOINT; set it after construction):
    k > 0 keeps, of the layer stack, only the inputs of every k-th layer for the backward, which recomputes one k-layer segment at
    a time (engine.model_forward, `checkpoint`).  Same logits; less memory for one more forward of the stack per step.  No effect
    under torch.no_grad().  A negative or non-integer value raises GnmError at the next forward.

    `dropout` (keyword, default 0.0; the reference's model passes none to its layers): node-output dropout of every GatedGCN layer
    (gated_gcn_full.py:154) in training mode with grad enabled -- masks from the device counter (engine.dropout_seed; one step per
    such forward), re-derived by the backward and by a checkpoint recomputation, never stored.  `last_dropout` holds the latest
    forward's (p, key, step) for engine.dropout_mask.  No effect under eval() or torch.no_grad(); 0.0 changes nothing at all.

    `reverse=True` (keyword of forward, default False: the path, launches and bits of a call without it): the scores of the
    edge-reversed graph, edge k read as (dst_k -> src_k), in the same edge-id order -- the same graph object, index and sweep plans,
    run on the mirrored parameters (mirror_state).  The in- / out-degree columns of `pe` are swapped by the mirror; its PageRank
    columns are carried as they are, not recomputed on the reversed adjacency.  Gradients flow to the model's own parameters; with
    a direct-write dp.FlatGradients the reversed pass adds its gradient to the buffer in one launch (_ModelFn._backward_mirrored)."""

    def __init__(self, node_features, edge_features, hidden_features, hidden_edge_features, num_layers,
                 hidden_edge_scores, batch_norm, nb_pos_enc, dropout=0.0):
        super().__init__()
        self.dropout = engine.dropout_p(dropout)
        self.last_dropout = None
        self.linear_pe = nn.Linear(nb_pos_enc + 2, hidden_features)
        self.linear1_edge = nn.Linear(edge_features, hidden_edge_features)
        self.linear2_edge = nn.Linear(hidden_edge_features, hidden_features)
        self.gnn = layers.GraphGatedGCN(num_layers, hidden_features, batch_norm, dropout=self.dropout)
        self.predictor = layers.ScorePredictor(hidden_features, hidden_edge_scores)
        self.num_layers = num_layers
        self.batch_norm = bool(batch_norm)
        self.activation_checkpoint = _default_checkpoint()

    def flatten_parameters(self) -> torch.Tensor:
        """See models.flatten_parameters.  Call it after .to(device) and BEFORE building dp.FlatGradients so that the
        gradient buffer follows the same layout (forward() does it on its own otherwise, but a FlatGradients made
        earlier then keeps state_dict order and the kernels' stacked gradients are copied instead of written in place)."""
        return flatten_parameters(self)

    def _wide_ln(self) -> bool:
        """What the layers recorded of layers.WIDE_LAYERNORM when they were built (LayerNorm above 256 channels)."""
        return all(getattr(c, "_wide_ln", False) for c in self.gnn.convs)

    def forward(self, graph, x, e, pe, reverse=False):
        graph = as_assembly_graph(graph, pe.device)       # a DGLGraph(-like) object is wrapped once and cached on itself
        H = self.linear_pe.out_features
        Hp = layers.padded_width(H)
        drop = None
        if self.dropout and self.training and torch.is_grad_enabled():
            drop = self.last_dropout = engine.dropout_draw(self.dropout, pe.device)
        if Hp != H:
            # a width the kernels are not built for (they are for 32 / 64 / 128 / 256): run the next one up with zero-padded
            # parameters -- the extra channels stay exactly zero through every layer (t = 0 -> bn -> relu -> 0; their gates
            # are 0.5 and gate zeros) and autograd slices the gradients back out of the padded tensors
            names, flat = zip(*self.named_parameters())
            src = mirror_state(dict(zip(names, flat))) if reverse else dict(zip(names, flat))      # mirror first, then pad
            padded = tuple(_pad_param(k, src[k], H, Hp) for k in names)
            need = torch.is_grad_enabled() and (any(p.requires_grad for p in flat) or e.requires_grad or pe.requires_grad)
            return _ModelFn.apply(graph, e, pe, self.num_layers, names, need, (self.batch_norm, H, self.activation_checkpoint, self._wide_ln(), drop), *padded)
        if pe.is_cuda and not _is_flat(self):
            flatten_parameters(self)          # once per device placement: stacked-parameter views instead of torch.cat
        names, flat = zip(*self.named_parameters())
        # e / pe requiring grad (input attribution, a frozen model, a learnable transform in front of the encoders) also
        # needs the activations: the backward returns their gradients; x stays dead (full_graph.py:23), its .grad None
        need = torch.is_grad_enabled() and (any(p.requires_grad for p in flat) or e.requires_grad or pe.requires_grad)
        if reverse:
            if not _is_flat(self):          # parameters off the device: ordinary autograd through the mirror
                m = mirror_state(dict(zip(names, flat)))
                return _ModelFn.apply(graph, e, pe, self.num_layers, names, need,
                                      (self.batch_norm, H, self.activation_checkpoint, self._wide_ln(), drop), *(m[k] for k in names))
            mirror = _mirror_of(self)
            return _ModelFn.apply(graph, e, pe, self.num_layers, names, need,
                                  (self.batch_norm, H, self.activation_checkpoint, self._wide_ln(), drop, mirror), *flat)
        return _ModelFn.apply(graph, e, pe, self.num_layers, names, need, (self.batch_norm, H, self.activation_checkpoint, self._wide_ln(), drop), *flat)


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, y, pos_weight):
        loss, gs = engine.bce_with_logits(scores.detach(), y, pos_weight)
        ctx.gs = gs.reshape(scores.shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        return ctx.gs * gl, None, None


class _BCECountsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, y, pos_weight, need_grad, epoch_acc):
        loss, gs, counts = engine.bce_with_logits_counts(scores.detach(), y, pos_weight, need_grad, epoch_acc)
        ctx.gs = gs.reshape(scores.shape) if need_grad else None
        ctx.mark_non_differentiable(counts)
        return loss.reshape(()), counts

    @staticmethod
    def backward(ctx, gl, _gc):
        return ctx.gs * gl, None, None, None, None


class BCEWithLogitsLoss(nn.Module):
    """torch.nn.BCEWithLogitsLoss(pos_weight=[pw]) with mean reduction as train.py:210-211 uses
    it, as one fused HIP pass that also produces d loss / d logits."""

    def __init__(self, pos_weight):
        super().__init__()
        self.pos_weight = float(pos_weight.reshape(-1)[0]) if torch.is_tensor(pos_weight) else float(pos_weight)

    def forward(self, scores, y):
        return _BCEFn.apply(scores, y, self.pos_weight)

    def with_counts(self, pred, y, epoch_acc=None):
        """(loss, counts): forward's loss (same bits, same gradient) and [TP, TN, FP, FN] of round(sigmoid(pred)) against y
        (train.tfpn_counts) as a device int64 [4] tensor, from the same pass over the logits.  Where no gradient can be asked for
        (torch.no_grad(), a detached pred) the pass stores no per-edge output.  epoch_acc: a train.EpochStats that the step's
        loss and counts are added to on the device."""
        need = torch.is_grad_enabled() and pred.requires_grad
        return _BCECountsFn.apply(pred, y, self.pos_weight, need, getattr(epoch_acc, "buf", epoch_acc))


class _SymLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, org, rev, y, pos_weight, alpha, need_grad, want_counts, epoch_acc):
        loss, parts, go, gr, counts = engine.sym_bce(org.detach(), rev.detach(), y, pos_weight, alpha, need_grad, want_counts, epoch_acc)
        ctx.go = go.reshape(org.shape) if need_grad else None
        ctx.gr = gr.reshape(rev.shape) if need_grad else None
        if counts is None:
            counts = torch.empty(0, dtype=torch.int64, device=loss.device)
        ctx.mark_non_differentiable(parts, counts)
        return loss.reshape(()), parts, counts

    @staticmethod
    def backward(ctx, gl, _gp, _gc):
        return (ctx.go * gl if ctx.needs_input_grad[0] else None, ctx.gr * gl if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None)


class SymmetryLoss(nn.Module):
    """The symmetry loss of the published GNNome training recipe as one fused HIP pass:
    mean_k(bce(org_k, y_k) + bce(rev_k, y_k) + alpha |org_k - rev_k|), bce = BCEWithLogits with pos_weight, org the scores of the
    graph and rev those of its edge-reversed twin (GraphGatedGCNModel.forward(..., reverse=True)), both in edge-id order.
    `last_parts` holds the device [3] tensor of the latest call: mean bce(org), mean bce(rev), mean |org - rev|.  Under
    torch.no_grad() or with inputs that need no gradient nothing is stored per edge."""

    def __init__(self, pos_weight, alpha=0.1):
        super().__init__()
        self.pos_weight = float(pos_weight.reshape(-1)[0]) if torch.is_tensor(pos_weight) else float(pos_weight)
        self.alpha = float(alpha)
        if not (0.0 <= self.alpha < float("inf")):
            raise ValueError(f"SymmetryLoss: alpha={alpha!r}: expected a finite number >= 0")
        self.last_parts = None

    def _run(self, org, rev, y, want_counts, epoch_acc):
        need = torch.is_grad_enabled() and (org.requires_grad or rev.requires_grad)
        loss, parts, counts = _SymLossFn.apply(org, rev, y, self.pos_weight, self.alpha, need, want_counts,
                                               getattr(epoch_acc, "buf", epoch_acc))
        self.last_parts = parts
        return loss, counts

    def forward(self, org, rev, y):
        return self._run(org, rev, y, False, None)[0]

    def with_counts(self, org, rev, y, epoch_acc=None):
        """(loss, counts): forward's loss (same bits, same gradients) and [TP, TN, FP, FN] of `org` -- metrics are reported on the
        original orientation -- as a device int64 [4] tensor from the same pass; epoch_acc: a train.EpochStats that receives the
        step's loss and counts."""
        return self._run(org, rev, y, True, epoch_acc)

    def gradients(self, org, rev, y, epoch_acc=None):
        """(loss, counts, g_org, g_rev) outside autograd: the loss (a detached scalar), the counts of `org` and d loss / d org,
        d loss / d rev as [E] tensors -- what the "sequential" schedule of train.train hands to two separate backward passes."""
        loss, parts, go, gr, counts = engine.sym_bce(org.detach(), rev.detach(), y, self.pos_weight, self.alpha, True, True,
                                                     getattr(epoch_acc, "buf", epoch_acc))
        self.last_parts = parts
        return loss.reshape(()), counts, go.reshape(org.shape), gr.reshape(rev.shape)
