"""Shared helpers for the parity tests (oracle side)."""
import os

import numpy as np
import torch

from gnnome_assembly_amd import synth
from oracle import gatedgcn_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The parity bar (BASELINE.json north_star: "within 1e-4 rel fp32"; SURVEY.md section 7
# "parity metric definition"): allclose(rtol=1e-4, atol=1e-5) AND norm-relative <= 1e-4.
RTOL = 1e-4
ATOL = 1e-5


def load_case(fname):
    z = np.load(os.path.join(GOLDEN, fname))
    H, L, seed = int(z["H"]), int(z["L"]), int(z["seed"])
    sd = synth.synth_state_dict(H, L, seed)
    return z, sd, H, L, bool(z["batch_norm"])


def grad_stride_of(z, H):
    """Sampling stride of a fixture's grad/* and adam/* arrays (make_golden.py: every grad_stride-th element for the large models)."""
    sampled = H == 128 or ("grad_sampled" in z.files and bool(z["grad_sampled"]))
    return int(z["grad_stride"]) if sampled else 1


def sd_to_torch(sd, dtype=torch.float32, requires_grad=False):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(requires_grad)
            for k, v in sd.items()}


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def assert_parity(got, want, what, rtol=RTOL, atol=ATOL, l2=1e-4):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.all(np.isfinite(got)), f"{what}: non-finite values"
    r = rel_l2(got, want)
    bad = np.abs(got - want) > atol + rtol * np.abs(want)
    assert r <= l2 and not bad.any(), (
        f"{what}: rel_l2={r:.3e} max_abs={np.abs(got - want).max():.3e} "
        f"violations={int(bad.sum())}/{bad.size}")


# -----------------------------------------------------------------------------------------
# gradient checks: which clause let a tensor pass (the table under profiles/), branch-exact comparison
# -----------------------------------------------------------------------------------------
GRAD_CLAUSES = {}       # pytest node id -> {clause: count}


def tally_clause(clause, count=1, forgiven=False):
    """Count a gradient tensor under the clause that decided it, for the running test.  `forgiven`: a tensor first
    counted as "miss" that the branch-exact comparison accepted -- moved from "miss" to "branch_exact"."""
    test = os.environ.get("PYTEST_CURRENT_TEST", "unknown").split(" ")[0]
    d = GRAD_CLAUSES.setdefault(test, {})
    d[clause] = d.get(clause, 0) + count
    if forgiven:
        d["miss"] = d.get("miss", 0) - count


def ln_layer_branches(idx, N, E, prm, s, ln_width=None):
    """The relu decisions (u > 0 [E,H], w > 0 [N,H]; internal order, on the CPU) of one LayerNorm layer, read from the kernels:
    the decision is the sign of fmaf(xhat, gamma, beta) with fp32 row statistics, which fp64 cannot re-derive -- but every
    LayerNorm kernel forms xhat with the one row_normalize expression of gnm_ln.h, so gnm_ln_edge_gate_fwd on the saved t with
    e_in = 0 returns relu(u) exactly and gnm_ln_node_update_fwd on the saved z with h_in = 0 returns relu(w) exactly (x + 0 is
    x: no residual left to absorb a tiny u).  prm: the layer's engine.LayerParams on the device; s: its LayerSaved."""
    from gnnome_assembly_amd import engine
    H = s.z.shape[1]
    lnw = H if ln_width is None else int(ln_width)
    dev = s.z.device
    f32 = dict(dtype=torch.float32, device=dev)
    P = s.P if s.P is not None else torch.zeros(N, 5 * H, **f32)
    relu_u, relu_w = torch.empty(E, H, **f32), torch.empty(N, H, **f32)
    hf, inv_f = torch.empty(N, H, **f32), torch.empty(N, H, **f32)
    p = engine._ptr
    with torch.cuda.device(dev):
        engine._call("gnm_ln_edge_gate_fwd", N, E, H, p(s.t), p(torch.zeros(E, H, **f32)), p(prm.gamma_e), p(prm.beta_e), p(P),
                     p(idx["isrc"]), p(idx["in_ptr"]), p(relu_u), p(hf), p(inv_f), lnw, engine._stream())
        engine._call("gnm_ln_node_update_fwd", N, H, p(s.z), p(prm.gamma_h), p(prm.beta_h), p(torch.zeros(N, H, **f32)), p(relu_w),
                     lnw, engine._stream())
        torch.cuda.synchronize()
    return (relu_u > 0).cpu(), (relu_w > 0).cpu()


def device_masks(ms, sd, e_raw_np, idx, ln=None):
    """The relu branch decisions the device kernels took, reproduced exactly: every kernel tests the
    sign of a single fmaf (or of a stored pre-activation), and the sign of round(a*b+c) equals the
    sign of a*b+c evaluated in fp64 (a*b is exact there).  A LayerNorm model: ln = (P, ln_width) -- the parameter dict the
    engine ran on (device tensors, padded like the run) and the width its rows were normalised over; the layers' decisions then
    come from the kernels themselves (ln_layer_branches)."""
    perm = idx["perm"].long().cpu()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    nrank = idx["nrank"].long().cpu() if "nrank" in idx else None      # internal node numbering -> the caller's
    u, w = [], []
    if ln is not None:
        from gnnome_assembly_amd import engine

    def branches(s):
        if getattr(s, "chunks", None):        # a layer wider than 256: one saved state per 256-column problem (engine.WIDE_CHUNK)
            uw = [branches(c) for c in s.chunks]
            return torch.cat([a for a, _ in uw], 1), torch.cat([b for _, b in uw], 1)
        uu = s.t.double() * s.stat_e[2].double() + s.stat_e[3].double()
        ww = s.z.double() * s.stat_h[2].double() + s.stat_h[3].double()
        return (uu > 0).cpu(), (ww > 0).cpu()
    for i, s in enumerate(ms.layers):
        if ln is None:
            um, wm = branches(s)
        else:
            um, wm = ln_layer_branches(idx, s.z.shape[0], perm.numel(), engine.layer_params(ln[0], i), s, ln[1])
        u.append(um[inv])                             # internal order -> edge-id order
        w.append(wm if nrank is None else wm[nrank])
    pred = ms.pred          # hidden_edge_scores run as zero-padded pieces (engine.pred_pieces): the real columns of each
    hid = torch.cat([ps.hid[:, :cols] for (_, cols, _), ps in pred.pieces], 1) if pred.pieces else pred.hid
    hid = (hid > 0).cpu()[inv]
    if ms.a1 is not None:   # the generic encoder keeps relu(a1) (one fp32 GEMM output): its sign is the branch taken
        return {"u": u, "w": w, "hid": hid, "a1": (ms.a1 > 0).cpu()[inv]}
    # fused encoder: ap = fmaf(w1a, x0, fmaf(w1b, x1, b))  (gnm_encoder.hip) -- inner fma rounded to fp32
    W1, b1 = sd["linear1_edge.weight"].astype(np.float64), sd["linear1_edge.bias"].astype(np.float64)
    x = e_raw_np.astype(np.float64)
    inner = (x[:, 1:2] * W1[None, :, 1] + b1[None, :]).astype(np.float32).astype(np.float64)
    a1 = torch.from_numpy((x[:, 0:1] * W1[None, :, 0] + inner) > 0)
    return {"u": u, "w": w, "hid": hid, "a1": a1}


def branch_exact_rows(src, dst, n, e_raw, pe, y, pw, sd, L, dev, batch_norm=True):
    """rows (name, rel_l2, max_abs, ref_norm) of the HIP gradients against the fp64 oracle backward evaluated
    on the SAME relu branches the device took, and the largest reference gradient norm."""
    from gnnome_assembly_amd import AssemblyGraph, engine, layers, models
    from oracle import gatedgcn_oracle as orc
    g = AssemblyGraph(src, dst, n).to(dev)
    P = {k: v.to(dev) for k, v in sd_to_torch(sd).items()}
    H = P["linear_pe.weight"].shape[0]
    Hp = layers.padded_width(H)
    if Hp != H:         # a width between the kernel instantiations: dead channels, exactly as GraphGatedGCNModel.forward pads
        P = {k: models._pad_param(k, v, H, Hp).contiguous() for k, v in P.items()}
    lnw = None if batch_norm else H        # what GraphGatedGCNModel.forward passes
    scores, ms = engine.model_forward(g, torch.from_numpy(e_raw).to(dev), torch.from_numpy(pe).to(dev), P, L, True, batch_norm, ln_width=lnw)
    masks = device_masks(ms, sd, e_raw, g.index(), None if batch_norm else (P, lnw))
    loss, gs = engine.bce_with_logits(scores, torch.from_numpy(y).to(dev), pw)
    Gd = engine.model_backward(g, P, L, ms, gs, batch_norm, ln_width=lnw)
    torch.cuda.synchronize()
    if Hp != H:
        masks["u"] = [m[:, :H] for m in masks["u"]]
        masks["w"] = [m[:, :H] for m in masks["w"]]
        for k, v in sd.items():
            if k == "predictor.W1.weight":
                Gd[k] = Gd[k].reshape(v.shape[0], 3, Hp)[:, :, :H].reshape(v.shape[0], 3 * H)
            else:
                Gd[k] = Gd[k][tuple(slice(0, d) for d in v.shape)]
    with torch.no_grad():
        _, l64, g64 = orc.manual_forward_backward(sd_to_torch(sd, torch.float64), torch.from_numpy(src), torch.from_numpy(dst),
                                                  n, torch.from_numpy(e_raw).double(), torch.from_numpy(pe).double(),
                                                  torch.from_numpy(y).double(), pw, masks=masks, batch_norm=batch_norm)
    assert abs(loss.item() - l64.item()) < 1e-5
    rows = []
    gmax = max(float(v.norm()) for v in g64.values())
    for k in g64:
        got, want = Gd[k].detach().cpu().double().numpy(), g64[k].detach().cpu().double().numpy()
        assert got.shape == want.shape, f"{k}: {got.shape} vs {want.shape}"
        rows.append((k, rel_l2(got, want), float(np.abs(got - want).max()), float(np.linalg.norm(want))))
    return rows, gmax


# -----------------------------------------------------------------------------------------
# the gradient clauses of the parameter gradients (test_gpu_parity.py) and of the input gradients (test_gpu_input_grads.py),
# shared with test_gpu_schedule_matrix.py
# -----------------------------------------------------------------------------------------
GRAD_L2 = 2e-4          # norm-relative bar for one parameter-gradient tensor (fp32 vs fp64 oracle)
GRAD_ABS_FLOOR = 2e-7   # gradients that are analytically zero (biases in front of a BatchNorm)
# Gradients that pass through the edge normalisation's backward (B_1/B_2/B_3, bn_e) are differences of large sums and flip with
# single relu-boundary elements: the reference's OWN fp32 arithmetic (the oracle run in fp32) differs from fp64 by up to ~1e-3
# norm-relative on them.  Rounds 1-4 let such a tensor pass when it was no further from the fp64 oracle than three times the
# fp32 oracle is -- a bar that moves with the fixture and bounded nothing.  There is NO noise clause any more, for
# either norm: a tensor outside GRAD_L2 must be EXACT (rel-L2 <= BRANCH_L2 = 5e-5) against the fp64 backward evaluated on the
# relu branches the device took -- the network is piecewise linear in those branches, so that comparison has no kink
# ambiguity and no fixture-dependent slack.  BatchNorm models: the branches are re-derived in fp64 from the stored statistics
# (device_masks); LayerNorm models: they are read from the kernels (ln_layer_branches), and the fp64 backward is
# oracle.manual_forward_backward(batch_norm=False).
BRANCH_L2 = 5e-5


def _grad_ok(r_ours, max_abs, floor):
    """Which clause decides this tensor is tallied per test (helpers.GRAD_CLAUSES -> gpurun_out/grad_clauses.json, committed
    under profiles/): rel-L2 <= GRAD_L2 or "miss", BatchNorm and LayerNorm models alike -- the caller takes the misses to the
    branch-exact comparison (_branch_exact_or_fail), where the absolute floor is the last resort.
    tests/test_zz_grad_clause_budget.py fails the suite when a test takes more "floor" escapes than the committed baseline."""
    clause = "l2" if r_ours <= GRAD_L2 else "miss"
    tally_clause(clause)
    return clause != "miss"


def _branch_exact_or_fail(bad, exact, bgmax, what, floor=None):
    """bad: rows (name, ...) that missed the plain bar; exact: name -> (name, rel_l2, max_abs, ref_norm) against the fp64
    backward on the device's branches.  Each must be exact (rel-L2 <= BRANCH_L2: tallied "branch_exact") or, failing that, under
    the absolute floor (max_abs <= max(GRAD_ABS_FLOOR, 1e-6 x the largest gradient norm): "floor" -- the gradients that are
    analytically zero, e.g. of a bias in front of a BatchNorm)."""
    floor = max(GRAD_ABS_FLOOR, 1e-6 * bgmax) if floor is None else floor
    ex = [b for b in bad if exact[b[0]][1] <= BRANCH_L2]
    fl = [b for b in bad if exact[b[0]][1] > BRANCH_L2 and exact[b[0]][2] <= floor]
    still = [b for b in bad if exact[b[0]][1] > BRANCH_L2 and exact[b[0]][2] > floor]
    tally_clause("branch_exact", len(ex), forgiven=True)
    tally_clause("floor", len(fl), forgiven=True)
    assert not still, (f"{what}: gradient tensors outside rel-L2 {GRAD_L2:g} of the fp64 oracle AND not exact ({BRANCH_L2:g}) for the "
                       f"relu branches the device took: {[(b, exact[b[0]]) for b in still]}")


def _oracle(sd, src, dst, n, e_np, pe_np, y_np, pw, bn):
    """fp64 autograd of oracle.model_forward: (d loss / d e_raw, d loss / d pe)."""
    p = sd_to_torch(sd, torch.float64)
    e = torch.from_numpy(e_np).double().requires_grad_(True)
    pe = torch.from_numpy(pe_np).double().requires_grad_(True)
    s = orc.model_forward(p, torch.as_tensor(src).long(), torch.as_tensor(dst).long(), n, e, pe, bn)
    orc.bce_loss(s, torch.from_numpy(y_np).double(), pw).backward()
    return e.grad.numpy(), pe.grad.numpy()


def _branch_exact(g, sd, H, L, e_np, pe_np, y_np, pw, dev, batch_norm=True):
    """The device's input gradients and the fp64 ones evaluated on the relu branches the device took (
    helpers.branch_exact_rows for the input gradients): the network is piecewise linear in those branches, so where a
    pre-activation within round-off of a kink flips between fp32 and fp64 -- which moves the gradient of the rows behind
    it by far more than round-off -- this comparison is exact all the same.  Runs the engine on the model's graph `g`
    (same index, same launches as GraphGatedGCNModel.forward / backward)."""
    from gnnome_assembly_amd import engine, layers, models
    P = {k: v.to(dev) for k, v in sd_to_torch(sd).items()}
    Hp = layers.padded_width(H)
    if Hp != H:
        P = {k: models._pad_param(k, v, H, Hp).contiguous() for k, v in P.items()}
    lnw = None if batch_norm else H        # what GraphGatedGCNModel.forward passes
    scores, ms = engine.model_forward(g, torch.from_numpy(e_np).to(dev), torch.from_numpy(pe_np).to(dev), P, L, True, batch_norm, ln_width=lnw)
    masks = device_masks(ms, sd, e_np, g.index(dev), None if batch_norm else (P, lnw))
    if e_np.shape[1] != 2:          # the generic encoder: relu of one fp32 GEMM output (device_masks models the fused kernel's fmaf)
        masks["a1"] = (ms.a1.cpu()[engine.edge_rank(g.index(dev)).long().cpu()] > 0)
    _, gs = engine.bce_with_logits(scores, torch.from_numpy(y_np).to(dev), pw)
    _, dev_e, dev_pe = engine.model_backward(g, P, L, ms, gs, batch_norm, ln_width=lnw, inputs=True)
    torch.cuda.synchronize()
    if Hp != H:
        masks["u"] = [m[:, :H] for m in masks["u"]]
        masks["w"] = [m[:, :H] for m in masks["w"]]
    s64 = sd_to_torch(sd, torch.float64)
    src, dst = (t.cpu() for t in g.edges())
    with torch.no_grad():
        _, _, _, dbg = orc.manual_forward_backward(s64, src, dst, g.num_nodes(), torch.from_numpy(e_np).double(),
                                                   torch.from_numpy(pe_np).double(), torch.from_numpy(y_np).double(), pw,
                                                   keep=True, masks=masks, batch_norm=batch_norm)
    want_pe = dbg[0]["gh_in"] @ s64["linear_pe.weight"]
    want_e = ((dbg[0]["ge_in"] @ s64["linear2_edge.weight"]) * masks["a1"]) @ s64["linear1_edge.weight"]
    return dev_e.cpu(), dev_pe.cpu(), want_e.numpy(), want_pe.numpy()


def _check(got_e, got_pe, want_e, want_pe, what, exact=None):
    """Each input gradient within GRAD_L2 of the fp64 reference or -- `exact` given -- exact (BRANCH_L2)
    against the fp64 backward on the branches the device took (the parameter gradients' two clauses; no other escape)."""
    ex = None
    for k, (name, got, want) in enumerate((("d e_raw", got_e, want_e), ("d pe", got_pe, want_pe))):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape, f"{what} {name}: shape {got.shape} vs {want.shape}"
        assert np.all(np.isfinite(got)), f"{what} {name}: non-finite values"
        r = rel_l2(got, want)
        if r <= GRAD_L2:
            tally_clause("l2")
            continue
        assert exact is not None, f"{what} {name}: rel_l2 {r:.3e} (max abs {np.abs(got - want).max():.3e}), no branch-exact oracle"
        ex = ex or exact()
        dev_g, want_x = ex[k], ex[2 + k]
        assert torch.equal(dev_g, torch.from_numpy(np.asarray(got, dtype=np.float32))), f"{what} {name}: engine route differs"
        rx = rel_l2(dev_g.numpy(), want_x)
        print(f"{what} {name}: rel_l2 {r:.3e} against fp64, {rx:.3e} on the device's branches")
        assert rx <= BRANCH_L2, f"{what} {name}: rel_l2 {r:.3e} against fp64 and {rx:.3e} on the device's own branches"
        tally_clause("branch_exact")


# -----------------------------------------------------------------------------------------
# the schedule-switch matrix (test_schedule_matrix_cpu.py checks the table, test_gpu_schedule_matrix.py runs it)
# -----------------------------------------------------------------------------------------
# Two levels per factor, (default, other): the engine.Options switches except the two side-stream caps (those are exercised by
# test_gpu_parity.test_side_stream_schedule_and_per_call_caps_change_nothing_but_rounding), and two choices of the caller --
# "inputs": e / pe require grad (the encoder backward that also writes their gradients), "flat": models.flatten_parameters +
# dp.FlatGradients(direct_write=True) (the kernels write the parameter gradients straight into the flat buffer).
SCHEDULE_FACTORS = {
    "FUSED": (True, False), "ACTIVATIONS": ("saved", "lean"), "CHAIN": (True, False), "TWO_SIDED": (True, False),
    "TWO_SIDED_FWD": (True, False), "WIDE_FUSED": (True, False), "NODE_FUSED": (True, False), "LN_SWEEP": (True, False),
    "TN_SIDE": (True, False), "TN_AT": ("auto", "now"), "TN_SPLIT": (True, False), "inputs": (False, True), "flat": (False, True),
}
SCHEDULE_CALLER = ("inputs", "flat")            # the factors that are not engine.Options switches
SCHEDULE_FORWARD = ("FUSED", "TWO_SIDED_FWD", "WIDE_FUSED")     # the switches a forward pass reads (ACTIVATIONS: only what it keeps)
# The factors each row sets to their non-default level.  Every factor gets its own 3-subset of rows 1..7 that contains row 1, so
# every pair of levels of every two factors appears in some row (row 0: both defaults; row 1: both others; the rows of one
# subset that are not in the other: one of each).  TN_AT = "auto" resolves to "next" at the matrix's graph size.
_SCHEDULE_OFF = {
    "r0": (),
    "r1": tuple(SCHEDULE_FACTORS),
    "r2": ("FUSED", "ACTIVATIONS", "CHAIN", "TWO_SIDED", "flat"),
    "r3": ("TWO_SIDED_FWD", "WIDE_FUSED", "NODE_FUSED", "LN_SWEEP", "flat"),
    "r4": ("FUSED", "TWO_SIDED_FWD", "TN_SIDE", "TN_AT"),
    "r5": ("ACTIVATIONS", "WIDE_FUSED", "TN_SPLIT", "inputs"),
    "r6": ("CHAIN", "NODE_FUSED", "TN_SIDE", "TN_SPLIT"),
    "r7": ("TWO_SIDED", "LN_SWEEP", "TN_AT", "inputs"),
}
SCHEDULE_ROWS = {r: {f: lv[f in off] for f, lv in SCHEDULE_FACTORS.items()} for r, off in _SCHEDULE_OFF.items()}


def schedule_switches(row: dict) -> dict:
    """The engine.options(...) keywords of a SCHEDULE_ROWS row (every switch given, whatever the process defaults are)."""
    return {k: v for k, v in row.items() if k not in SCHEDULE_CALLER}


# -----------------------------------------------------------------------------------------
# stand-alone GatedGCN_1d variants (residual=False, in_channels != out_channels): inputs and parameters are drawn
# from seeded numpy streams here -- shared by tests/golden/make_golden_layer.py (which runs the REFERENCE layer on
# them) and by the tests -- so the fixture only stores the reference's outputs
# -----------------------------------------------------------------------------------------
LAYER_VARIANTS = {                # name: (in_channels, out_channels, batch_norm, residual argument)
    "in48_out32_bn": (48, 32, True, True),
    "in32_out32_bn_nores": (32, 32, True, False),
    "in128_out128_bn_nores": (128, 128, True, False),
    "in16_out32_ln": (16, 32, False, True),
    "in32_out32_ln_nores": (32, 32, False, False),
}


def layer_variant_case(name):
    """graph (src, dst, n), fp32 inputs h0 [N,in], e0 [E,in], functional weights wh [N,out], we [E,out] and the layer's
    state_dict (fp32 numpy, the reference's keys) for one variant."""
    cin, cout, bn, res = LAYER_VARIANTS[name]
    src, dst, n = synth.make_graph(60, seed=9, permute_edge_ids=True)
    rng = np.random.default_rng(sum(map(ord, name)))
    E = src.size
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    case = dict(src=src, dst=dst, n=n, cin=cin, cout=cout, bn=bn, res=res,
                h0=f32(rng.standard_normal((n, cin))), e0=f32(rng.standard_normal((E, cin))),
                wh=f32(rng.standard_normal((n, cout))), we=f32(rng.standard_normal((E, cout))))
    sd = {}
    b = 1.0 / np.sqrt(cin)
    for k in ("A_1", "A_2", "A_3", "B_1", "B_2", "B_3"):
        sd[k + ".weight"] = f32(rng.uniform(-b, b, size=(cout, cin)))
        sd[k + ".bias"] = f32(rng.uniform(-b, b, size=(cout,)))
    for k in ("bn_h", "bn_e"):
        sd[k + ".weight"] = f32(rng.uniform(0.5, 1.5, size=cout))
        sd[k + ".bias"] = f32(rng.uniform(-0.3, 0.3, size=cout))
    case["sd"] = sd
    return case


# -----------------------------------------------------------------------------------------
# replicated graphs (test_replica_cpu.py checks the identity, test_gpu_scale_replicas.py runs it past the 32-bit limits):
# G_K = K disjoint copies of a small graph G0, every copy with G0's features and labels.  Exactly, in real arithmetic: the
# BatchNorm statistics (mean, biased variance) over edges and nodes are G0's, so every copy's logits are G0's, the loss (a mean)
# and every parameter gradient are G0's, and d loss / d e, d pe of each copy are G0's divided by K.  One fp64 oracle run on G0
# then checks every row of a graph far too large for the oracle itself.
# -----------------------------------------------------------------------------------------
def replica_base_graph(reads=4000, seed=11, hub_in=300):
    """G0: a synth.make_graph assembly graph plus the edge cases a replica run should carry -- one destination with `hub_in`
    in-edges (its run spans many 16-row sweep tiles), one self loop, one duplicated edge, one isolated node (the last id, so
    N0 is odd) and an edge dropped if need be so that E0 is odd; edge ids shuffled.  Returns (src, dst, n) int32 / int."""
    src, dst, n = synth.make_graph(reads, seed=seed)
    rng = np.random.default_rng(seed + 101)
    hub = n // 3
    hs = rng.choice(np.setdiff1d(np.arange(n), [hub]), size=hub_in, replace=False)
    src, dst = np.concatenate([src, hs]), np.concatenate([dst, np.full(hub_in, hub)])
    if src.size % 2 == 0:                       # two more follow: make E0 odd
        src, dst = src[1:], dst[1:]
    src = np.concatenate([src, [7, src[0]]])    # a self loop, a duplicated edge
    dst = np.concatenate([dst, [7, dst[0]]])
    p = rng.permutation(src.size)
    n += 1                                                                              # the isolated node
    assert src.size % 2 == 1 and n % 2 == 1
    return src[p].astype(np.int32), dst[p].astype(np.int32), n


def replicate(src, dst, n, K, shuffle_seed=None):
    """G_K: K disjoint copies of (src, dst, n), copy-major (copy c holds edges c*E0 .. and nodes c*N0 ..), or -- with
    `shuffle_seed` -- under one random permutation of ALL node ids and one of ALL edge ids.  Returns dict(src, dst [K*E0] int32,
    n = K*N0, K, E0, N0, ecopy / epos [K*E0]: the (copy, position in G0) of each edge, ncopy / npos [K*N0]: same for each node).
    Tile a G0 edge array with a[epos], a node array with a[npos]."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    E0, N0 = src.size, int(n)
    assert K * N0 < 2 ** 31 and K * E0 < 2 ** 31
    base = (np.arange(K, dtype=np.int64) * N0)[:, None]
    s, d = (src[None, :] + base).reshape(-1), (dst[None, :] + base).reshape(-1)
    ecopy, epos = np.repeat(np.arange(K, dtype=np.int32), E0), np.tile(np.arange(E0, dtype=np.int32), K)
    ncopy, npos = np.repeat(np.arange(K, dtype=np.int32), N0), np.tile(np.arange(N0, dtype=np.int32), K)
    if shuffle_seed is not None:
        rng = np.random.default_rng(shuffle_seed)
        pn = rng.permutation(K * N0)                  # old node id -> new
        pe = rng.permutation(K * E0)                  # new edge id -> old
        s, d = pn[s[pe]], pn[d[pe]]
        ecopy, epos = ecopy[pe], epos[pe]
        nc, npp = np.empty_like(ncopy), np.empty_like(npos)
        nc[pn], npp[pn] = ncopy, npos
        ncopy, npos = nc, npp
    return dict(src=s.astype(np.int32), dst=d.astype(np.int32), n=K * N0, K=K, E0=E0, N0=N0,
                ecopy=ecopy, epos=epos, ncopy=ncopy, npos=npos)


def per_copy(a, copy, pos, K, size0):
    """Rows of a G_K array (edge or node order of the replicated graph) as [K, size0, ...] fp64: out[copy[i], pos[i]] = a[i]."""
    a = np.asarray(a)
    out = np.empty((K, size0) + a.shape[1:], dtype=np.float64)
    out[copy, pos] = a
    return out


def copy_rel_l2(got, want):
    """Per-copy rel-L2 of got [K, size0, ...] against one copy's reference want [size0, ...]: [K] fp64."""
    g = np.asarray(got, np.float64).reshape(got.shape[0], -1)
    w = np.asarray(want, np.float64).reshape(1, -1)
    return np.linalg.norm(g - w, axis=1) / max(float(np.linalg.norm(w)), 1e-30)


def assert_copies_parity(got, want, what, rtol=RTOL, atol=ATOL, l2=1e-4):
    """assert_parity of EVERY copy of got [K, size0, ...] against want [size0, ...] (a whole-tensor norm would dilute a
    corrupted tail).  Returns (worst rel-L2, its copy)."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape[1:] == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.all(np.isfinite(got)), f"{what}: non-finite values in copies {np.unique(np.nonzero(~np.isfinite(got))[0])[:8]}"
    r = copy_rel_l2(got, want)
    g, w = got.reshape(got.shape[0], -1), want.reshape(1, -1)
    bad = (np.abs(g - w) > atol + rtol * np.abs(w)).sum(1)
    fail = np.nonzero((r > l2) | (bad > 0))[0]
    worst = int(np.argmax(r))
    assert fail.size == 0, (f"{what}: {fail.size} of {got.shape[0]} copies differ from the reference, first {fail[:8].tolist()} "
                            f"(rel_l2 {r[fail[:8]].tolist()}, violations {bad[fail[:8]].tolist()}); worst copy {worst} rel_l2 "
                            f"{r[worst]:.3e}")
    return float(r[worst]), worst


def zscore(a):
    """utils.preprocess_graph's z-score (torch .std(): unbiased) in fp64."""
    a = np.asarray(a, np.float64)
    return (a - a.mean()) / a.std(ddof=1)
