"""Layer-segment activation checkpointing (GraphGatedGCNModel.activation_checkpoint, engine.model_forward(checkpoint=k)) on the
HIP path (-m gpu).  The recompute runs the forward's kernels on the forward's inputs, so: logits are bit-identical to
checkpoint = 0; where the backward SCHEDULE is unchanged (per-layer backward, or one segment) every gradient is bit-identical
too; where segment ends fall inside a chained stack (1 <= k < L under the default options) the gradients are checked against
the fixtures' fp64 reference with the bars of test_gpu_parity.test_model_matches_golden (helpers.GRAD_L2, else exact on the
device's relu branches).  No tolerance of its own."""
import os

import numpy as np
import pytest
import torch

from helpers import (BRANCH_L2, GOLDEN, GRAD_ABS_FLOOR, _branch_exact_or_fail, _check, _grad_ok, _oracle, assert_parity, device_masks,
                     grad_stride_of, load_case, rel_l2, sd_to_torch)

pytestmark = pytest.mark.gpu

INPUT_GRADS = os.path.join(GOLDEN, "input_grads")
CASES = [("small_h128l8_s0.npz", 1), ("small_h128l8_s0.npz", 3), ("small_h128l8_s0.npz", 8), ("tiny_h256l16_s0.npz", 4),
         ("small_h32l2ln_s0.npz", 1), ("small_h64l1_s0.npz", 1)]
WITH_INPUT_GRADS = ("small_h128l8_s0.npz", "small_h32l2ln_s0.npz")    # the CASES with a file under tests/golden/input_grads
MODES = ["f16x2", "bf16x3", "f32"]        # the matmul modes test_model_matches_golden runs


@pytest.fixture(params=MODES)
def matmul_mode(request):
    from gnnome_assembly_amd import _lib
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _fixture_model(fname, dev):
    import gnnome_assembly_amd as G
    z, sd, H, L, bn = load_case(fname)
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, bn, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.to(dev)
    g = G.AssemblyGraph(z["src"], z["dst"], int(z["n"])).to(dev)
    return z, sd, H, L, bn, model, g


def _synth_model(reads, H, L, seed, dev):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    src, dst, n = synth.make_graph(reads, seed)
    inp = synth.make_inputs(src, dst, n, seed)
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, seed).items()})
    model.to(dev)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    e, pe, y = (torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y"))
    return model, g, e, pe, y, float(inp["pos_weight"])


def _step(model, g, e, pe, y, pw, k, inputs=False):
    """One fwd + BCE + bwd with activation_checkpoint = k: (scores, loss, {param: grad}, e.grad, pe.grad), clones."""
    import gnnome_assembly_amd as G
    model.activation_checkpoint = k
    model.zero_grad(set_to_none=True)
    e = e.detach().clone().requires_grad_(inputs)
    pe = pe.detach().clone().requires_grad_(inputs)
    s = model(g, None, e, pe)
    loss = G.BCEWithLogitsLoss(pw)(s.squeeze(-1), y)
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    return s.detach().clone(), loss.item(), grads, e.grad, pe.grad


def _z_inputs(z, dev):
    return (torch.from_numpy(z["e_raw"]).to(dev), torch.from_numpy(z["pe"]).to(dev), torch.from_numpy(z["y"]).to(dev),
            float(z["pos_weight"]))


def _same(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


# -----------------------------------------------------------------------------------------
# logits, and the gradients where the backward schedule is the one of checkpoint = 0
# -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fname,k", CASES)
def test_logits_are_bit_identical(fname, k, matmul_mode):
    dev = _dev()
    z, sd, H, L, bn, model, g = _fixture_model(fname, dev)
    e, pe, y, pw = _z_inputs(z, dev)
    s0, l0, _, _, _ = _step(model, g, e, pe, y, pw, 0)
    sk, lk, _, _, _ = _step(model, g, e, pe, y, pw, k)
    assert torch.equal(s0, sk) and l0 == lk
    model.activation_checkpoint = k         # no effect without grad: nothing is kept, same logits
    with torch.no_grad():
        assert torch.equal(model(g, None, e, pe), s0)


@pytest.mark.parametrize("fname,k", CASES)
def test_per_layer_backward_is_bit_identical_for_any_k(fname, k, matmul_mode):
    """CHAIN=False: every layer's backward is its own set of launches, wherever the segment ends are."""
    from gnnome_assembly_amd import engine
    dev = _dev()
    z, sd, H, L, bn, model, g = _fixture_model(fname, dev)
    e, pe, y, pw = _z_inputs(z, dev)
    with engine.options(CHAIN=False):
        _, _, g0, ge0, gpe0 = _step(model, g, e, pe, y, pw, 0, inputs=True)
        _, _, gk, gek, gpek = _step(model, g, e, pe, y, pw, k, inputs=True)
    assert _same(g0, gk) and torch.equal(ge0, gek) and torch.equal(gpe0, gpek)


@pytest.mark.parametrize("fname", ["small_h128l8_s0.npz", "tiny_h256l16_s0.npz", "small_h32l2ln_s0.npz", "small_h64l1_s0.npz"])
def test_one_segment_is_bit_identical_under_the_default_options(fname, matmul_mode):
    """k >= num_layers: the whole stack is one segment and gets the schedule a model of that shape gets."""
    dev = _dev()
    z, sd, H, L, bn, model, g = _fixture_model(fname, dev)
    e, pe, y, pw = _z_inputs(z, dev)
    _, _, g0, ge0, gpe0 = _step(model, g, e, pe, y, pw, 0, inputs=True)
    for k in (L, L + 3):
        _, _, gk, gek, gpek = _step(model, g, e, pe, y, pw, k, inputs=True)
        assert _same(g0, gk) and torch.equal(ge0, gek) and torch.equal(gpe0, gpek), k


# -----------------------------------------------------------------------------------------
# segment ends inside the stack under the default options: against the fp64 reference
# -----------------------------------------------------------------------------------------

def _engine_on_device_branches(g, z, sd, H, L, k, dev, bn=True):
    """helpers.branch_exact_rows / _branch_exact for a checkpointed run: the engine's gradients with checkpoint = k, and the fp64
    backward evaluated on the relu branches the device took.  The branches are read from the saved activations of a
    checkpoint = 0 forward (a checkpointed one keeps none; its logits and therefore its branches are the same bits).
    Returns (G, d e_raw, d pe, rows (name, rel_l2, max_abs, ref_norm), largest reference norm, want d e_raw, want d pe)."""
    from gnnome_assembly_amd import engine, layers
    from oracle import gatedgcn_oracle as orc
    assert layers.padded_width(H) == H
    P = {n: v.to(dev) for n, v in sd_to_torch(sd).items()}
    e, pe, y, pw = _z_inputs(z, dev)
    lnw = None if bn else H
    s0, ms0 = engine.model_forward(g, e, pe, P, L, True, bn, ln_width=lnw)
    masks = device_masks(ms0, sd, z["e_raw"], g.index(dev), None if bn else (P, lnw))
    del ms0
    scores, ms = engine.model_forward(g, e, pe, P, L, True, bn, ln_width=lnw, checkpoint=k)
    assert torch.equal(scores, s0) and not ms.layers and len(ms.boundaries) == len(engine.checkpoint_segments(L, k))
    _, gs = engine.bce_with_logits(scores, y, pw)
    Gd, dev_e, dev_pe = engine.model_backward(g, P, L, ms, gs, bn, ln_width=lnw, inputs=True)
    torch.cuda.synchronize()
    assert all(b is None for b in ms.boundaries)
    s64 = sd_to_torch(sd, torch.float64)
    with torch.no_grad():
        _, _, g64, dbg = orc.manual_forward_backward(s64, torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), int(z["n"]),
                                                     torch.from_numpy(z["e_raw"]).double(), torch.from_numpy(z["pe"]).double(),
                                                     torch.from_numpy(z["y"]).double(), pw, keep=True, masks=masks,
                                                     batch_norm=bn)
    rows = []
    for n in g64:
        got, want = Gd[n].cpu().double().numpy(), g64[n].double().numpy()
        rows.append((n, rel_l2(got, want), float(np.abs(got - want).max()), float(np.linalg.norm(want))))
    want_pe = dbg[0]["gh_in"] @ s64["linear_pe.weight"]
    want_e = ((dbg[0]["ge_in"] @ s64["linear2_edge.weight"]) * masks["a1"]) @ s64["linear1_edge.weight"]
    return Gd, dev_e.cpu(), dev_pe.cpu(), rows, max(float(v.norm()) for v in g64.values()), want_e.numpy(), want_pe.numpy()


@pytest.mark.parametrize("fname,k", [(f, k) for f, k in CASES if k < load_case(f)[3]])
def test_gradients_match_the_fp64_reference_with_segment_ends_inside_the_stack(fname, k, matmul_mode):
    """The bars of test_model_matches_golden, clause by clause: every parameter gradient within GRAD_L2 of the reference's fp64
    run, else exact
    (BRANCH_L2) against the fp64 backward on the branches the device took; and d e_raw, d pe against
    tests/golden/input_grads with the bars of test_input_grads_match_reference."""
    dev = _dev()
    z, sd, H, L, bn, model, g = _fixture_model(fname, dev)
    e, pe, y, pw = _z_inputs(z, dev)
    scores, loss, grads, ge, gpe = _step(model, g, e, pe, y, pw, k, inputs=True)
    assert_parity(scores.cpu().numpy(), z["scores64"], f"{fname} k={k} logits vs reference fp64")
    assert abs(loss - float(z["loss64"])) <= 1e-5 * max(1.0, abs(float(z["loss64"])))
    stride = grad_stride_of(z, H)
    gmax = max(float(np.linalg.norm(z["grad/" + n])) for n in grads)
    bad = []
    for n, gr in grads.items():
        got, want = gr.cpu().double().numpy().reshape(-1)[::stride], z["grad/" + n]
        assert got.shape == want.shape, n
        r, m = rel_l2(got, want), float(np.abs(got - want).max())
        print(f"{fname} k={k} {matmul_mode} {n:28s} rel_l2={r:.3e} max_abs={m:.3e}")
        if not _grad_ok(r, m, max(GRAD_ABS_FLOOR, 1e-6 * gmax)):
            bad.append((n, r, m, float(np.linalg.norm(want))))
    exact = []

    def on_branches():
        if not exact:
            exact.append(_engine_on_device_branches(g, z, sd, H, L, k, dev, bn))
            Gd = exact[0][0]         # the engine route must be the model's route: same launches, same bits
            assert all(torch.equal(Gd[n], grads[n]) for n in grads), "engine route differs from the model's"
        return exact[0]
    if bad:
        _, _, _, rows, bgmax, _, _ = on_branches()
        _branch_exact_or_fail(bad, {r[0]: r for r in rows}, bgmax, f"{fname} k={k}")
    ex = lambda: (on_branches()[1], on_branches()[2], on_branches()[5], on_branches()[6])  # noqa: E731
    if fname in WITH_INPUT_GRADS:       # the reference's own fp64 input gradients; the fixture must be there and be this case
        zi = np.load(os.path.join(INPUT_GRADS, fname))
        assert (int(zi["H"]), int(zi["L"]), int(zi["seed"]), bool(zi["batch_norm"])) == (H, L, int(z["seed"]), bn)   # same weights
        assert all(np.array_equal(zi[a], z[a]) for a in ("src", "dst", "n", "e_raw", "pe", "y", "pos_weight")), "not the same inputs"
        want_e, want_pe = zi["grad_e_raw"], zi["grad_pe"]
    else:                               # no input-gradient fixture for this case: the fp64 oracle's autograd, here
        assert fname == "tiny_h256l16_s0.npz" and not os.path.exists(os.path.join(INPUT_GRADS, fname))
        want_e, want_pe = _oracle(sd, z["src"], z["dst"], int(z["n"]), z["e_raw"], z["pe"], z["y"], pw, bn)
    _check(ge.cpu().numpy(), gpe.cpu().numpy(), want_e, want_pe, f"{fname} k={k}", ex)


@pytest.mark.parametrize("k", [1, 2])
def test_chained_layernorm_stack_with_segment_ends_inside(k, matmul_mode):
    """A route the fixtures do not take: LayerNorm at H = 128, the chained LayerNorm schedule (engine.ln_chain_eligible) run per
    segment with a layer offset.  Against the fp64 oracle with the bars of test_other_widths_and_norms_vs_oracle (GRAD_L2, else
    exact -- BRANCH_L2 -- on the branches the device took, else the floor) and, for d e_raw / d pe, of test_input_grads_match_oracle."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import _lib, engine, synth
    from oracle import gatedgcn_oracle as orc
    dev = _dev()
    H, L, seed = 128, 4, 6
    src, dst, n = synth.make_graph(700, seed=seed, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed=seed)
    sd = synth.synth_state_dict(H, L, seed=seed)
    pw = float(inp["pos_weight"])
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, False, 16)
    model.load_state_dict({a: torch.from_numpy(v) for a, v in sd.items()})
    model.to(dev)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    if _lib.split_mode():           # the schedule under test is the one that runs (the fp32-MFMA mode has no chained schedule)
        assert engine.ln_chain_eligible(H, False) and hasattr(g, "sweep_plan")
    e, pe, y = (torch.from_numpy(inp[a]).to(dev) for a in ("e", "pe", "y"))
    s0, l0, _, _, _ = _step(model, g, e, pe, y, pw, 0)
    scores, loss, grads, ge, gpe = _step(model, g, e, pe, y, pw, k, inputs=True)
    assert torch.equal(scores, s0) and loss == l0
    p64 = sd_to_torch(sd, torch.float64, requires_grad=True)
    s64 = orc.model_forward(p64, torch.from_numpy(src), torch.from_numpy(dst), n, torch.from_numpy(inp["e"]).double(),
                            torch.from_numpy(inp["pe"]).double(), False)
    l64 = orc.bce_loss(s64, torch.from_numpy(inp["y"]).double(), pw)
    l64.backward()
    assert_parity(scores.cpu().numpy(), s64.detach().numpy(), f"LayerNorm H={H} L={L} k={k} logits")
    assert abs(loss - l64.item()) < 1e-5
    zz = dict(src=src, dst=dst, n=n, e_raw=inp["e"], pe=inp["pe"], y=inp["y"], pos_weight=inp["pos_weight"])
    bad = []
    for name, gr in grads.items():
        got, want = gr.cpu().double().numpy(), p64[name].grad.numpy()
        r = rel_l2(got, want)
        print(f"LayerNorm H={H} L={L} k={k} {matmul_mode} {name:28s} rel_l2={r:.3e}")
        if not _grad_ok(r, float(np.abs(got - want).max()), GRAD_ABS_FLOOR):
            bad.append((name, r))
    exact = []

    def on_branches():
        if not exact:
            exact.append(_engine_on_device_branches(g, zz, sd, H, L, k, dev, False))
            assert all(torch.equal(exact[0][0][a], grads[a]) for a in grads), "engine route differs from the model's"
        return exact[0]
    if bad:
        _, _, _, rows, bgmax, _, _ = on_branches()
        _branch_exact_or_fail(bad, {r[0]: r for r in rows}, bgmax, f"LayerNorm H={H} L={L} k={k}", floor=GRAD_ABS_FLOOR)
    # the comparison a LayerNorm tensor outside GRAD_L2 falls back to, run whether or not one missed: every gradient of the segmented
    # run is exact on the branches the kernels report
    rows = on_branches()[3]
    assert len(rows) == len(grads)
    worse = [r for r in rows if r[1] > BRANCH_L2 and r[2] > GRAD_ABS_FLOOR]
    assert not worse, f"LayerNorm H={H} L={L} k={k}: not exact on the device's branches: {worse}"
    want_e, want_pe = _oracle(sd, src, dst, n, inp["e"], inp["pe"], inp["y"], pw, False)
    _check(ge.cpu().numpy(), gpe.cpu().numpy(), want_e, want_pe, f"LayerNorm H={H} L={L} k={k}",
           lambda: (on_branches()[1], on_branches()[2], on_branches()[5], on_branches()[6]))


# -----------------------------------------------------------------------------------------
# the flat gradient buffer, lean activations, retain_graph
# -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 8])
def test_flat_gradient_buffer_is_written_directly(k, matmul_mode):
    """dp.FlatGradients zeroed: the segment backward writes every gradient into the buffer; bit-identical to the non-flat run."""
    from gnnome_assembly_amd import dp
    dev = _dev()
    z, sd, H, L, bn, model, g = _fixture_model("small_h128l8_s0.npz", dev)
    e, pe, y, pw = _z_inputs(z, dev)
    _, _, ref, _, _ = _step(model, g, e, pe, y, pw, k)
    model.zero_grad(set_to_none=True)
    model.flatten_parameters()
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    flat.zero_()
    assert flat.fresh
    import gnnome_assembly_amd as G
    G.BCEWithLogitsLoss(pw)(model(g, None, e, pe).squeeze(-1), y).backward()
    torch.cuda.synchronize()
    assert not flat.fresh                 # the direct-write path ran
    lo, hi = flat.flat.data_ptr(), flat.flat.data_ptr() + flat.flat.numel() * 4
    for n, p in model.named_parameters():
        assert lo <= p.grad.data_ptr() < hi and torch.equal(p.grad, ref[n]), n


def test_lean_activations_inside_a_segment_are_bit_identical(matmul_mode):
    from gnnome_assembly_amd import engine
    dev = _dev()
    z, sd, H, L, bn, model, g = _fixture_model("small_h128l8_s0.npz", dev)
    e, pe, y, pw = _z_inputs(z, dev)
    s0, l0, g0, ge0, gpe0 = _step(model, g, e, pe, y, pw, 3, inputs=True)
    with engine.options(ACTIVATIONS="lean"):
        s1, l1, g1, ge1, gpe1 = _step(model, g, e, pe, y, pw, 3, inputs=True)
    assert torch.equal(s0, s1) and l0 == l1 and _same(g0, g1) and torch.equal(ge0, ge1) and torch.equal(gpe0, gpe1)


def test_a_second_backward_raises():
    import gnnome_assembly_amd as G
    dev = _dev()
    model, g, e, pe, y, pw = _synth_model(500, 128, 4, 4, dev)
    model.activation_checkpoint = 2
    loss = G.BCEWithLogitsLoss(pw)(model(g, None, e, pe).squeeze(-1), y)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward called twice"):
        loss.backward()


def test_a_bad_attribute_raises_at_the_forward():
    from gnnome_assembly_amd import _lib
    dev = _dev()
    model, g, e, pe, y, pw = _synth_model(500, 128, 2, 4, dev)
    for bad in (-1, 1.5, "x"):
        model.activation_checkpoint = bad
        with pytest.raises(_lib.GnmError, match="checkpoint"):
            model(g, None, e, pe)


# -----------------------------------------------------------------------------------------
# the training loop
# -----------------------------------------------------------------------------------------

def test_two_epochs_of_training_are_bit_identical(tmp_path):
    """train.train honours the attribute of the model it is given (the model_factory hook); per-layer backward: the same
    launches on the same data, so every step's loss and the final parameters are the same bits as without checkpointing."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine, synth, train as T
    dev = _dev()
    samples = []
    for seed in range(3):
        src, dst, n = synth.make_graph(400, seed)
        inp = synth.make_inputs(src, dst, n, seed)
        samples.append(T.GraphSample(G.AssemblyGraph(src, dst, n).to(dev), torch.from_numpy(inp["e"]).to(dev),
                                     torch.from_numpy(inp["pe"]).to(dev), torch.from_numpy(inp["y"]).to(dev)))
    hp = dict(num_epochs=2, dim_latent=128, num_gnn_layers=4, lr=1e-2)
    seen = []

    def factory(k):
        def make(h):
            m = G.GraphGatedGCNModel(h["node_features"], h["edge_features"], h["dim_latent"], h["hidden_edge_features"],
                                     h["num_gnn_layers"], h["hidden_edge_scores"], h["batch_norm"], h["nb_pos_enc"])
            m.activation_checkpoint = k
            seen.append(m)
            return m
        return make
    runs = []
    for k in (0, 2):
        with engine.options(CHAIN=False):
            model, _, hist = T.train(samples[:2], samples[2:], out=f"k{k}", hyperparameters=hp, workdir=str(tmp_path / f"k{k}"),
                                     verbose=False, hooks={"model_factory": factory(k)})
        assert model is seen[-1] and model.activation_checkpoint == k
        runs.append((hist.step_losses, hist.loss_valid, {n: v.clone() for n, v in model.state_dict().items()}))
    assert len(runs[0][0]) == 4 and runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert _same(runs[0][2], runs[1][2])


# -----------------------------------------------------------------------------------------
# memory
# -----------------------------------------------------------------------------------------

def test_peak_memory_of_a_step_drops():
    """One synthetic graph (E = 0.2 M edges: an [E,H] tensor is 0.096 GiB at H = 128, the largest step here about 5 GiB), H = 128, L = 8,
    one step per configuration in this process, the peak counter reset in between.  Two structural conditions: with k = 2 the
    step holds 4 boundaries and at most 2 layers' activations where it held 8 layers', in either activation mode.  The third,
    saved + k = 2 under lean + k = 0, follows from the per-layer sizes of DESIGN.md section 2 (4 boundaries + 2 live layers of
    about 2 + 5N/E [E,H] units each against 8 layers of about 1 unit plus two rebuilt ones) and is what DESIGN.md section 2
    states as measured: asserted too.  The four peaks are printed first."""
    from gnnome_assembly_amd import engine
    dev = _dev()
    model, g, e, pe, y, pw = _synth_model(20000, 128, 8, 3, dev)
    g.index()
    E = e.shape[0]
    unit = 4.0 * E * 128

    def peak(mode, k):
        with engine.options(ACTIVATIONS=mode):
            model.activation_checkpoint = k
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _step(model, g, e, pe, y, pw, k)
            return torch.cuda.max_memory_allocated() - base
    peak("saved", 0)            # warm-up: scratch buffers, sweep plans, the flat parameter buffer
    p = {(m, k): peak(m, k) for m in ("saved", "lean") for k in (0, 2)}
    for (m, k), v in p.items():
        print(f"peak memory of one training step, E={E} H=128 L=8: {m:5s} k={k}: {v / 2 ** 30:.3f} GiB = {v / unit:.1f} [E,H] units")
    assert p[("saved", 2)] < p[("saved", 0)]
    assert p[("lean", 2)] < p[("lean", 0)]
    assert p[("saved", 2)] < p[("lean", 0)]
