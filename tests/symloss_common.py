"""The symmetry loss stated in fp64, for the CPU and the GPU tests:

    l_k = bce(o_k, y_k) + bce(r_k, y_k) + alpha |o_k - r_k|,   L = mean_k l_k,   bce(x, y) = pw y softplus(-x) + (1 - y) softplus(x)

sym_loss_fp64 is the differentiable torch statement (what the whole-model tests differentiate through the oracle);
sym_closed_form is the same loss with its gradients written out, no autograd:
    dL/do_k = (bce'(o_k) + alpha sgn(o_k - r_k)) / E,  dL/dr_k = (bce'(r_k) - alpha sgn(o_k - r_k)) / E,  sgn(0) = 0,
    bce'(x) = -pw y sigma(-x) + (1 - y) sigma(x).
The graphs, configurations and the reversed-graph oracle of the tests live here too."""
import os

import numpy as np
import torch

from gnnome_assembly_amd import synth
from oracle import gatedgcn_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (hidden width, layers, batch_norm): BatchNorm H=64/L=1, BatchNorm H=128/L=2, LayerNorm H=32/L=2
CONFIGS = [(64, 1, True), (128, 2, True), (32, 2, False)]
# the tiny edge-case graph (N=64/E=256: isolated, zero-in-degree, self-loop, duplicate-edge cases) and the small banded one
GRAPHS = {"tiny": "tiny_h64l1_s0.npz", "small": "small_h64l1_s0.npz"}


def sym_loss_fp64(org, rev, y, pos_weight, alpha):
    """(loss, parts[3]) as fp64 torch tensors, differentiable in org and rev."""
    sp = lambda x: x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))       # noqa: E731  (F.softplus is linear above 20: 2e-9 off there)
    o, r, y = org.reshape(-1).double(), rev.reshape(-1).double(), y.reshape(-1).double()
    bo = (pos_weight * y * sp(-o) + (1.0 - y) * sp(o)).mean()
    br = (pos_weight * y * sp(-r) + (1.0 - y) * sp(r)).mean()
    ab = (o - r).abs().mean()
    return bo + br + alpha * ab, torch.stack([bo, br, ab])


def _softplus64(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid64(x):
    return np.exp(-_softplus64(-x))          # exp(-log(1 + e^-x)): no cancellation on either side


def sym_closed_form(org, rev, y, pos_weight, alpha):
    """numpy fp64: (loss, parts[3], g_org[E], g_rev[E], bce'(org)[E] / E, bce'(rev)[E] / E) without autograd."""
    o, r, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (org, rev, y))
    E, pw = o.size, float(pos_weight)
    term = lambda x: pw * y * _softplus64(-x) + (1.0 - y) * _softplus64(x)         # noqa: E731
    grad = lambda x: (-pw * y * _sigmoid64(-x) + (1.0 - y) * _sigmoid64(x)) / E    # noqa: E731
    parts = np.array([term(o).mean(), term(r).mean(), np.abs(o - r).mean()])
    sgn = np.sign(o - r)
    bo, br = grad(o), grad(r)
    return parts[0] + parts[1] + alpha * parts[2], parts, bo + alpha * sgn / E, br - alpha * sgn / E, bo, br


def load_graph(which):
    """(src, dst, n, e_raw, pe, y, pos_weight) of a golden graph, numpy."""
    z = np.load(os.path.join(GOLDEN, GRAPHS[which]))
    return z["src"], z["dst"], int(z["n"]), z["e_raw"], z["pe"], z["y"], float(z["pos_weight"])


def state_dict64(H, L, seed=0, requires_grad=False):
    sd = synth.synth_state_dict(H, L, seed)
    return {k: torch.from_numpy(np.asarray(v)).double().clone().requires_grad_(requires_grad) for k, v in sd.items()}


def swap_degree_columns(pe):
    """pe' = cat(out_deg, in_deg, pagerank): what reverse(g) has where g has cat(in_deg, out_deg, pagerank) (PageRank carried)."""
    idx = list(range(pe.shape[1]))
    idx[0], idx[1] = 1, 0
    return pe[:, idx]


def oracle_scores(sd, src, dst, n, e_raw, pe, bn, reverse=False):
    """fp64 oracle scores [E] of the graph, or of its edge-reversed twin (swapped edge list, swapped degree columns)."""
    s, d = torch.as_tensor(src).long(), torch.as_tensor(dst).long()
    e, p = torch.as_tensor(e_raw).double(), torch.as_tensor(pe).double()
    if reverse:
        return orc.model_forward(sd, d, s, n, e, swap_degree_columns(p), bn).reshape(-1)
    return orc.model_forward(sd, s, d, n, e, p, bn).reshape(-1)


def oracle_sym_loss(sd, src, dst, n, e_raw, pe, y, pw, alpha, bn):
    """(loss, parts, org, rev) in fp64 through the oracle on the graph and on the really reversed graph."""
    org = oracle_scores(sd, src, dst, n, e_raw, pe, bn)
    rev = oracle_scores(sd, src, dst, n, e_raw, pe, bn, reverse=True)
    loss, parts = sym_loss_fp64(org, rev, torch.as_tensor(y).double(), pw, alpha)
    return loss, parts, org, rev


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 gradient on the branches the device took (the escape of the gradient parity test, for this loss)
# ---------------------------------------------------------------------------------------------------------------------

def masked_forward(sd, src, dst, n, e_raw, pe, bn, masks):
    """oracle.model_forward with every relu decision replaced by the given one (helpers.device_masks' layout: edge-id / node
    order): the network is linear in those branches, so fp64 autograd through this is the exact gradient of the branch taken."""
    src, dst = torch.as_tensor(src).long(), torch.as_tensor(dst).long()
    e_raw, pe = torch.as_tensor(e_raw).double(), torch.as_tensor(pe).double()
    h = pe @ sd["linear_pe.weight"].t() + sd["linear_pe.bias"]
    e = (e_raw @ sd["linear1_edge.weight"].t() + sd["linear1_edge.bias"]) * masks["a1"]
    e = e @ sd["linear2_edge.weight"].t() + sd["linear2_edge.bias"]
    for i in range(orc.num_layers_of(sd)):
        p = f"gnn.convs.{i}."
        lin = lambda k, x: x @ sd[p + k + ".weight"].t() + sd[p + k + ".bias"]       # noqa: E731
        A1h, A2h, A3h, B1h, B2h = (lin(k, h) for k in ("A_1", "A_2", "A_3", "B_1", "B_2"))
        t = B1h.index_select(0, src) + B2h.index_select(0, dst) + lin("B_3", e)
        e_out = orc._norm(t, sd[p + "bn_e.weight"], sd[p + "bn_e.bias"], bn) * masks["u"][i] + e
        sig = torch.sigmoid(e_out)
        z0 = torch.zeros((n, A2h.shape[1]), dtype=h.dtype)
        f = z0.index_add(0, dst, sig * A2h.index_select(0, src)) / (z0.index_add(0, dst, sig) + orc.EPS_DEN)
        b = z0.index_add(0, src, sig * A3h.index_select(0, dst)) / (z0.index_add(0, src, sig) + orc.EPS_DEN)
        h = orc._norm(A1h + f + b, sd[p + "bn_h.weight"], sd[p + "bn_h.bias"], bn) * masks["w"][i] + h
        e = e_out
    data = torch.cat((h.index_select(0, src), h.index_select(0, dst), e), dim=1)
    hid = (data @ sd["predictor.W1.weight"].t() + sd["predictor.W1.bias"]) * masks["hid"]
    return (hid @ sd["predictor.W2.weight"].t() + sd["predictor.W2.bias"]).reshape(-1)


def device_scores_and_masks(which, H, L, bn, seed, reverse, dev):
    """The device's scores [E] (fp32, edge-id order) of one pass and its relu decisions -- helpers.branch_exact_rows' recipe, with
    the mirrored parameters for the reversed pass (mirror first, then pad, as GraphGatedGCNModel.forward does)."""
    from gnnome_assembly_amd import AssemblyGraph, engine, layers, models
    from helpers import device_masks
    src, dst, n, e_raw, pe, y, pw = load_graph(which)
    sd = synth.synth_state_dict(H, L, seed)
    P = {k: torch.from_numpy(np.asarray(v)).float().to(dev) for k, v in sd.items()}
    if reverse:
        P = models.mirror_state(P)
    Hp = layers.padded_width(H)
    P = {k: (models._pad_param(k, v, H, Hp) if Hp != H else v).contiguous() for k, v in P.items()}
    lnw = None if bn else H
    g = AssemblyGraph(src, dst, n).to(dev)
    scores, ms = engine.model_forward(g, torch.from_numpy(e_raw).to(dev), torch.from_numpy(pe).to(dev), P, L, True, bn, ln_width=lnw)
    masks = device_masks(ms, sd, e_raw, g.index(), None if bn else (P, lnw))
    torch.cuda.synchronize()
    masks["u"] = [m[:, :H] for m in masks["u"]]
    masks["w"] = [m[:, :H] for m in masks["w"]]
    return scores.reshape(-1).cpu(), {k: ([m.double() for m in v] if isinstance(v, list) else v.double()) for k, v in masks.items()}


def branch_exact_sym_grads(which, H, L, bn, seed, alpha, dev):
    """{name: fp64 gradient} of the symmetry loss evaluated on the device's own branches: the relu decisions of its two passes and
    its sign of o_k - r_k (alpha s_k (o_k - r_k) with s_k fixed is what alpha |o_k - r_k| is on that branch)."""
    src, dst, n, e_raw, pe, y, pw = load_graph(which)
    o_dev, m_org = device_scores_and_masks(which, H, L, bn, seed, False, dev)
    r_dev, m_rev = device_scores_and_masks(which, H, L, bn, seed, True, dev)
    sd = state_dict64(H, L, seed, requires_grad=True)
    o = masked_forward(sd, src, dst, n, e_raw, pe, bn, m_org)
    r = masked_forward(sd, dst, src, n, e_raw, swap_degree_columns(torch.as_tensor(pe).double()), bn, m_rev)
    yy = torch.as_tensor(y).double()
    sp = lambda x: x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))       # noqa: E731
    bce = lambda x: (pw * yy * sp(-x) + (1.0 - yy) * sp(x)).mean()          # noqa: E731
    s = torch.sign(o_dev.double() - r_dev.double())
    (bce(o) + bce(r) + alpha * (s * (o - r)).mean()).backward()
    return {k: v.grad.numpy() for k, v in sd.items()}
