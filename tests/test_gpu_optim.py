"""GPU: the library's optimizer step (gnm_optim_grad_stats + gnm_optim_adam_step, dp.LibAdam, the "optimizer": "library" route of
train.train) against the fp64 restatement in tests/optim_reference.py.

The accuracy bound is not a number chosen here: torch.optim.Adam(fused=True) runs in the same test on the same fp32 inputs, its
per-tensor max absolute error against the same fp64 reference is taken, and the library may be at most 2 x that plus one fp32
ulp of max|p| (two equally valid operation orders; tensors where torch happens to be exact).  The measured pairs are printed
and, when GNM_OPTIM_ACCURACY_OUT names a file, written there as JSON (profiles/optim_step.json keeps a copy under "accuracy")."""
import json
import os

import numpy as np
import pytest
import torch

import optim_reference as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 2047, 2048, 2049, 3 * 2048 + 5]
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
_PAIRS = {}


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    """As in test_gpu_parity: the loop tests run under all three matmul modes; the optimizer kernels are behind no matrix-core
    kernel, so their tests are marked `mode_independent` and run once."""
    from gnnome_assembly_amd import _lib
    if request.param != _lib.DEFAULT_MATMUL_MODE and request.node.get_closest_marker("mode_independent"):
        pytest.skip("runs once (does not depend on the matmul mode)")
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Raw:
    """The two entry points on caller-owned flat buffers (engine.optim_step); the workspace starts as 0xFF bytes."""

    def __init__(self, p0, max_norm=0.0, **hyper):
        from gnnome_assembly_amd import engine
        self.e, dev = engine, _dev()
        self.h = dict(HYPER, **hyper)
        self.max_norm = max_norm
        self.p = torch.from_numpy(np.asarray(p0, np.float32)).to(dev)
        self.n = self.p.numel()
        self.g = torch.zeros_like(self.p)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.step_t = torch.zeros((), dtype=torch.float32, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int64, device=dev)
        self.ws = engine.optim_workspace(self.n, dev).fill_(-1)

    def step(self, g, zero_grad=False, inv_count=None):
        self.g.copy_(torch.from_numpy(np.asarray(g, np.float32)))
        self.e.optim_step(self.p, self.g, self.m, self.v, self.step_t, self.stats, self.ws, self.h["lr"], *self.h["betas"],
                          self.h["eps"], self.max_norm, inv_count, zero_grad)
        return self

    def read_stats(self):
        s = self.stats.cpu()
        f = s.view(torch.float64)
        return dict(total_norm=float(f[0]), nonfinite=int(s[1]), skipped=int(s[2]), clip=float(f[3]))

    def bits(self):
        return [t.clone().view(torch.int32) for t in (self.p, self.m, self.v, self.step_t.reshape(1))] + [self.stats.clone()]


def _fused_adam(p0, **hyper):
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0, np.float32)).to(_dev()))
    p.grad = torch.zeros_like(p)
    return p, torch.optim.Adam([p], fused=True, **dict(HYPER, **hyper))


def _err(t, want):
    return float(np.abs(t.detach().cpu().double().numpy().reshape(-1) - want.reshape(-1)).max())


def _check(tag, ours, theirs, want_p, record=True):
    """ours / theirs: (p, m, v) tensors of the library and of torch's fused Adam; want_p etc.: the fp64 reference (p, m, v)."""
    floor = ref.ulp32(np.abs(want_p[0]).max())
    rows = []
    for name, a, b, w in zip("pmv", ours, theirs, want_p):
        rows.append((name, _err(a, w), _err(b, w)))
    print(tag, " ".join(f"{n}: lib {x:.3e} torch {y:.3e}" for n, x, y in rows), f"floor {floor:.3e}")
    if record:
        _PAIRS[tag] = {n: {"library": x, "torch_fused": y} for n, x, y in rows} | {"ulp_of_max_abs_p": floor}
    for n, x, y in rows:
        assert x <= 2.0 * y + floor, (tag, n, x, y, floor)


def _dump_pairs():
    path = os.environ.get("GNM_OPTIM_ACCURACY_OUT", "").strip()
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_PAIRS, f, indent=1, sort_keys=True)


@pytest.mark.mode_independent
@pytest.mark.parametrize("n", SIZES)
def test_five_steps_against_fp64_within_twice_fused_adams_error(lib, n):
    p0, grads = ref.make_case(n, seed=n)
    if n >= 3:
        assert (grads[0] == 0).any()
    assert 1e-12 <= np.abs(grads[0][grads[0] != 0]).min() and np.abs(grads[0]).max() <= 1e3
    r, ours = ref.AdamRef(p0, **HYPER), Raw(p0)
    tp, topt = _fused_adam(p0)
    for k, g in enumerate(grads):
        ours.step(g)
        tp.grad.copy_(torch.from_numpy(g))
        topt.step()
        r.step(g)
        st = topt.state[tp]
        _check(f"n={n} step={k + 1}", (ours.p, ours.m, ours.v), (tp, st["exp_avg"], st["exp_avg_sq"]), (r.p, r.m, r.v))
        assert float(ours.step_t) == k + 1 == float(st["step"])
        assert torch.equal(ours.g.cpu(), torch.from_numpy(g))                 # zero_grad off: the gradient is left alone
        zero = torch.from_numpy(g == 0)
        assert torch.equal(ours.m.cpu()[zero], torch.zeros(int(zero.sum())))     # 0 / (0 + eps) stays 0: exact zeros all the way
        assert torch.equal(ours.p.cpu()[zero], torch.from_numpy(p0)[zero])
    s = ours.read_stats()
    assert s["nonfinite"] == 0 and s["skipped"] == 0 and s["clip"] == 1.0
    assert abs(s["total_norm"] - r.total_norm) <= 1e-12 * r.total_norm
    _dump_pairs()


def _tiny_model(dev, seed=3, H=64):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp, models
    torch.manual_seed(seed)
    model = G.GraphGatedGCNModel(1, 2, H, 16, 1, 64, True, 16).to(dev)
    models.flatten_parameters(model)
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    return model, flat


@pytest.mark.mode_independent
def test_model_layout_through_libadam_against_fp64(lib):
    """The real layout: a flattened GraphGatedGCNModel (H = 64, L = 1; n = 39,985, a ragged tail) through dp.LibAdam, per
    parameter tensor against torch's fused Adam on copies of the same tensors."""
    from gnnome_assembly_amd import dp
    dev = _dev()
    model, flat = _tiny_model(dev)
    opt = dp.LibAdam(model.parameters(), flat=flat, **HYPER)
    assert opt.gnm_impl == "library"
    order = opt._order
    n = opt._p.numel()
    assert n == sum(p.numel() for p in model.parameters()) and n % 4 != 0
    _, grads = ref.make_case(n, seed=11)
    p0 = opt._p.cpu().numpy().copy()
    copies = [torch.nn.Parameter(p.detach().clone()) for p in order]
    for c in copies:
        c.grad = torch.zeros_like(c)
    topt = torch.optim.Adam(copies, fused=True, **HYPER)
    r = ref.AdamRef(p0, **HYPER)
    for k, g in enumerate(grads):
        flat.grads.copy_(torch.from_numpy(g))
        o = 0
        for c in copies:
            c.grad.copy_(torch.from_numpy(g[o:o + c.numel()]).view_as(c))
            o += c.numel()
        opt.step()
        topt.step()
        r.step(g)
        o = 0
        for i, (p, c) in enumerate(zip(order, copies)):
            sl = slice(o, o + p.numel())
            if k == len(grads) - 1 or i < 3:
                _check(f"model tensor {i} step={k + 1}", (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]),
                       (c, topt.state[c]["exp_avg"], topt.state[c]["exp_avg_sq"]), (r.p[sl], r.m[sl], r.v[sl]),
                       record=k == len(grads) - 1)
            o += p.numel()
    assert float(opt.state[order[0]]["step"]) == 5.0
    st = opt.stats()
    assert st.is_cuda and st.dtype == torch.float64 and st.tolist()[1:] == [0.0, 0.0, 1.0]
    assert abs(float(st[0]) - r.total_norm) <= 1e-12 * r.total_norm
    _dump_pairs()


@pytest.mark.mode_independent
def test_clip_above_and_below_the_norm(lib):
    n = 3 * 2048 + 5
    p0, grads = ref.make_case(n, seed=21, steps=2)
    norm = float(np.sqrt((grads[0].astype(np.float64) ** 2).sum()))
    # norm = 10 x max_norm
    mx = norm / 10
    r, ours = ref.AdamRef(p0, max_norm=mx, **HYPER), Raw(p0, max_norm=mx)
    tp, topt = _fused_adam(p0)
    for k, g in enumerate(grads):
        ours.step(g)
        r.step(g)
        s = ours.read_stats()
        assert abs(s["total_norm"] - r.total_norm) <= 1e-12 * r.total_norm and abs(s["clip"] - r.clip) <= 1e-12 * r.clip
        assert k > 0 or abs(r.clip - 0.1) < 1e-6
        # torch's route to the same step: clip_grad_norm_, then fused Adam
        tp.grad.copy_(torch.from_numpy(g))
        torch.nn.utils.clip_grad_norm_([tp], mx)
        topt.step()
        st = topt.state[tp]
        _check(f"clip n={n} step={k + 1}", (ours.p, ours.m, ours.v), (tp, st["exp_avg"], st["exp_avg_sq"]), (r.p, r.m, r.v))
    # a gradient below max_norm: the same bits as with clipping off
    a, b = Raw(p0, max_norm=0.0), Raw(p0, max_norm=2 * max(float(np.sqrt((g.astype(np.float64) ** 2).sum())) for g in grads))
    for g in grads:
        a.step(g)
        b.step(g)
        assert b.read_stats()["clip"] == 1.0
        assert all(torch.equal(x, y) for x, y in zip(a.bits(), b.bits()))
    # the contributor count of the C ABI: c = 1 / max(count, 1)
    cnt = torch.tensor(4.0, device=_dev())
    c, rc = Raw(p0, max_norm=mx), ref.AdamRef(p0, max_norm=mx, **HYPER)
    c.step(grads[0], inv_count=cnt)
    rc.step(grads[0], count=4.0)
    s = c.read_stats()
    assert abs(s["total_norm"] - rc.total_norm) <= 1e-12 * rc.total_norm and abs(s["clip"] - rc.clip) <= 1e-12 * rc.clip
    assert _err(c.p, rc.p) <= 2 * ref.ulp32(np.abs(rc.p).max()) and _err(c.m, rc.m) <= ref.ulp32(np.abs(rc.m).max())
    z = Raw(p0)
    z.step(grads[0], inv_count=torch.tensor(0.0, device=_dev()))             # a count of 0 divides by 1
    y = Raw(p0).step(grads[0])
    assert all(torch.equal(u, w) for u, w in zip(z.bits(), y.bits()))
    _dump_pairs()


@pytest.mark.mode_independent
@pytest.mark.parametrize("zero_grad", [False, True])
def test_non_finite_gradient_skips_the_step_on_the_device(lib, zero_grad):
    n = 3 * 2048 + 5
    p0, grads = ref.make_case(n, seed=31, steps=3)
    ours, r = Raw(p0), ref.AdamRef(p0, **HYPER)
    bad = grads[0].copy()
    bad[5], bad[2048 + 7] = np.nan, np.inf              # input data in two different blocks
    before = ours.bits()
    for k in (1, 2):
        ours.step(bad, zero_grad=zero_grad)
        r.step(bad)
        s = ours.read_stats()
        assert s["nonfinite"] == 2 and s["skipped"] == k == r.skipped
        assert abs(s["total_norm"] - r.total_norm) <= 1e-12 * r.total_norm          # over the finite entries
        assert all(torch.equal(x, y) for x, y in zip(before[:4], ours.bits()[:4]))   # p, m, v, step: bit-unchanged
        if zero_grad:
            assert not bool(ours.g.view(torch.int32).any())
        else:
            assert torch.equal(ours.g.view(torch.int32).cpu(), torch.from_numpy(bad).view(torch.int32))
    # a clean step after the skipped ones is the FIRST step: t = 1 bias correction
    ours.step(grads[1], zero_grad=zero_grad)
    r.step(grads[1])
    tp, topt = _fused_adam(p0)
    tp.grad.copy_(torch.from_numpy(grads[1]))
    topt.step()
    st = topt.state[tp]
    _check(f"after skip n={n} zero_grad={zero_grad}", (ours.p, ours.m, ours.v), (tp, st["exp_avg"], st["exp_avg_sq"]), (r.p, r.m, r.v),
           record=False)
    s = ours.read_stats()
    assert float(ours.step_t) == 1.0 == r.t and s["skipped"] == 2 and s["nonfinite"] == 0
    assert bool(ours.g.view(torch.int32).any()) != zero_grad


@pytest.mark.mode_independent
def test_same_bits_twice_and_under_another_occupancy_cap(lib):
    """n = 300 blocks + 5: more blocks than one workgroup per CU, so the cap changes the grid and which workgroup owns which block."""
    n = 300 * 2048 + 5
    p0, grads = ref.make_case(n, seed=41, steps=2)
    runs = []
    for cap in (0, 0, 1, 3):
        assert lib.gnm_set_occupancy_cap(cap) == 0
        try:
            a = Raw(p0, max_norm=1.0)
            for g in grads:
                a.step(g, zero_grad=True)
        finally:
            lib.gnm_set_occupancy_cap(0)
        runs.append(a.bits())
    for other in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], other))
    # an unaligned view of the same data (element by element instead of 16-byte accesses): the same bits again
    dev = _dev()
    b = Raw(p0, max_norm=1.0)
    for name in ("p", "g", "m", "v"):
        buf = torch.zeros(n + 1, dtype=torch.float32, device=dev)
        buf[1:].copy_(getattr(b, name))
        setattr(b, name, buf[1:])
    assert b.p.data_ptr() % 16 == 4
    for g in grads:
        b.step(g, zero_grad=True)
    assert all(torch.equal(x, y) for x, y in zip(runs[0], b.bits()))


def _graph_inputs(dev, reads=200, seed=5):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    src, dst, n = synth.make_graph(reads, seed=seed)
    inp = synth.make_inputs(src, dst, n, seed=seed)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    return g, tuple(torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y")), float(inp["pos_weight"])


def test_zero_grad_leaves_the_buffer_fresh_for_the_direct_write_backward(lib):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp
    dev = _dev()
    model, flat = _tiny_model(dev, H=32)         # a width the kernels run natively: the backward writes straight into `flat`
    g, (e, pe, y), pw = _graph_inputs(dev)
    crit = G.BCEWithLogitsLoss(pw)
    opt = dp.LibAdam(model.parameters(), flat=flat, **HYPER)
    flat.zero_()
    crit(model(g, None, e, pe).squeeze(-1), y).backward()
    assert not flat.fresh and bool(flat.grads.any())
    flat.flat[-1] = 7.0                                  # the trailing contributor slot is not the optimizer's
    opt.step(zero_grad=True)
    assert flat.fresh and not bool(flat.grads.view(torch.int32).any()) and float(flat.flat[-1]) == 7.0
    assert float(opt._step) == 1.0
    crit(model(g, None, e, pe).squeeze(-1), y).backward()          # direct write into the buffer the step left
    assert not flat.fresh
    first = flat.grads.clone()
    flat.zero_()
    crit(model(g, None, e, pe).squeeze(-1), y).backward()          # the same parameters after an explicit zero
    assert bool(first.any()) and torch.equal(first.view(torch.int32), flat.grads.view(torch.int32))
    opt.step()                                            # zero_grad off: the gradient stays, the buffer is not fresh
    assert not flat.fresh and torch.equal(first, flat.grads)
    opt.zero_grad()
    assert flat.fresh and not bool(flat.grads.any())


def test_checkpoint_interchange_with_torch_adam(lib):
    """2 steps of one, state_dict, load into the other, 2 steps: within the accuracy bound of 4 fp64 steps, both directions.  The
    bound's torch side is 4 uninterrupted steps of fused Adam."""
    from gnnome_assembly_amd import dp
    dev = _dev()
    for direction in ("torch->library", "library->torch"):
        model, flat = _tiny_model(dev)
        lib_opt = dp.LibAdam(model.parameters(), flat=flat, **HYPER)
        order = lib_opt._order
        n = lib_opt._p.numel()
        _, grads = ref.make_case(n, seed=51, steps=4)
        p0 = lib_opt._p.cpu().numpy().copy()
        tor = torch.optim.Adam(model.parameters(), fused=True, **HYPER)
        # the yardstick: torch fused alone for 4 steps on copies
        copies = [torch.nn.Parameter(p.detach().clone()) for p in order]
        for c in copies:
            c.grad = torch.zeros_like(c)
        yard = torch.optim.Adam(copies, fused=True, **HYPER)
        r = ref.AdamRef(p0, **HYPER)
        first, second = (tor, lib_opt) if direction == "torch->library" else (lib_opt, tor)
        for k, g in enumerate(grads):
            if k == 2:
                second.load_state_dict(first.state_dict())
                if second is lib_opt:
                    lo, hi = lib_opt._m.data_ptr(), lib_opt._m.data_ptr() + 4 * n
                    assert all(lo <= lib_opt.state[p]["exp_avg"].data_ptr() < hi for p in order)     # still views
                    assert lib_opt.state[order[0]]["exp_avg"].data_ptr() == lo and float(lib_opt._step) == 2.0
            flat.grads.copy_(torch.from_numpy(g))
            o = 0
            for c in copies:
                c.grad.copy_(torch.from_numpy(g[o:o + c.numel()]).view_as(c))
                o += c.numel()
            (first if k < 2 else second).step()
            yard.step()
            r.step(g)
        who = second
        o = 0
        for i, (p, c) in enumerate(zip(order, copies)):
            sl = slice(o, o + p.numel())
            _check(f"{direction} tensor {i}", (p, who.state[p]["exp_avg"], who.state[p]["exp_avg_sq"]),
                   (c, yard.state[c]["exp_avg"], yard.state[c]["exp_avg_sq"]), (r.p[sl], r.m[sl], r.v[sl]), record=False)
            o += p.numel()
        assert float(who.state[order[0]]["step"]) == 4.0
    # per-parameter step counts that disagree are refused
    sd = tor.state_dict()
    sd["state"][0] = dict(sd["state"][0], step=torch.tensor(9.0))
    with pytest.raises(ValueError, match="disagree"):
        lib_opt.load_state_dict(sd)


# ---- the training loop -----------------------------------------------------------------------------------------------------

def _golden_run(golden_dir, dev):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth, train as T
    z = np.load(os.path.join(golden_dir, "train_loop_h128l2.npz"))
    hp = {str(k): float(v) for k, v in zip(z["hp_keys"], z["hp_vals"])}
    for k in ("seed", "num_epochs", "dim_latent", "node_features", "edge_features", "hidden_edge_features", "hidden_edge_scores",
              "num_gnn_layers", "nb_pos_enc", "batch_size_train", "batch_size_eval", "patience"):
        hp[k] = int(hp[k])
    hp["batch_norm"] = bool(hp["batch_norm"])

    def sample(spec):
        reads, seed, permute = (int(v) for v in spec)
        src, dst, n = synth.make_graph(reads, seed, permute_edge_ids=bool(permute))
        inp = synth.make_inputs(src, dst, n, seed)
        g = G.AssemblyGraph(src, dst, n).to(dev)
        return T.GraphSample(g, torch.from_numpy(inp["e"]).to(dev), torch.from_numpy(inp["pe"]).to(dev), torch.from_numpy(inp["y"]).to(dev))
    return z, hp, [sample(z[f"train{i}"]) for i in range(2)], [sample(z["valid0"])]


def test_library_route_meets_the_reference_loop_pin(lib, tmp_path, golden_dir):
    """train.train with "optimizer": "library" on the fixture of test_gpu_parity.test_train_loop_matches_the_reference_loop, under
    that test's bounds: per-step losses, epoch losses, the ReduceLROnPlateau LR sequence, the best epoch, TP/TN/FP/FN."""
    from gnnome_assembly_amd import train as T
    z, hp, train, valid = _golden_run(golden_dir, _dev())
    hp["optimizer"] = "library"
    model, best, hist = T.train(train, valid, out="pin", hyperparameters=hp, workdir=str(tmp_path), verbose=False)
    assert hist.step_graph == z["step_graph64"].tolist()
    got, w64, w32 = np.array(hist.step_losses), z["step_losses64"], z["step_losses32"]
    noise = np.abs(w32 - w64) / w64
    rel = np.abs(got - w64) / w64
    print("per-step loss rel. error vs reference fp64:", np.array2string(rel, precision=2), "reference fp32:", np.array2string(noise, precision=2))
    assert np.all(rel <= np.maximum(1e-4, 5 * noise)), (got, w64)
    for name, g_, want in (("train", hist.loss_train, z["loss_train64"]), ("valid", hist.loss_valid, z["loss_valid64"])):
        assert np.allclose(g_, want, rtol=1e-4, atol=0), (name, g_, want)
    assert hist.lr == z["lr64"].tolist() and hist.final_lr == float(z["final_lr64"])
    assert hist.best_epoch == int(z["best_epoch64"])
    for name, g_, r64, r32 in (("train", hist.tfpn_train, z["tfpn_train64"], z["tfpn_train32"]),
                               ("valid", hist.tfpn_valid, z["tfpn_valid64"], z["tfpn_valid32"])):
        g_ = np.array(g_)
        assert g_.shape == r64.shape and np.array_equal(g_.sum(1), r64.sum(1))
        slack = np.full(g_.shape, 2.0)
        slack[1:] = np.maximum(2.0, np.ceil(1e-3 * r64.sum(1, keepdims=True)[1:]))
        assert np.all(np.abs(g_ - r64) <= 3 * np.abs(r32 - r64) + slack), (name, g_.tolist(), r64.tolist())
    assert hist.skipped_steps == 0
    assert len(hist.total_norm) == hp["num_epochs"] and all(np.isfinite(t) and t > 0 for t in hist.total_norm)
    # the checkpoint the loop wrote holds torch Adam's schema
    ck = torch.load(os.path.join(str(tmp_path), "checkpoints", "pin.pt"), map_location="cpu")
    st = ck["optim_state_dict"]["state"]
    assert len(st) == len(list(model.parameters())) and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in st.values())
    assert {float(s["step"]) for s in st.values()} == {float(len(hist.step_losses))}


def test_mini_batch_loop_library_against_torch_route(lib, tmp_path, golden_dir):
    """Mini-batch mode (batch_size_train = 2) on the same tiny graphs, library against torch route: every loss the loop computes, in
    call order, within the per-step bound of the pin (1e-4 relative), and the same ReduceLROnPlateau decisions."""
    from gnnome_assembly_amd import models, train as T
    dev = _dev()
    z, hp, _, _ = _golden_run(golden_dir, dev)
    hp.update(batch_size_train=2, batch_size_eval=2, num_parts_metis_train=8, num_parts_metis_eval=8, num_epochs=4, fused_metrics=False)
    runs = {}
    for route in ("torch", "library"):
        _, _, train, valid = _golden_run(golden_dir, dev)
        losses = []

        class Recording(models.BCEWithLogitsLoss):
            def forward(self, scores, y):
                out = super().forward(scores, y)
                losses.append(out.detach())
                return out
        _, _, hist = T.train(train, valid, out=route, hyperparameters=dict(hp, optimizer=route), workdir=str(tmp_path / route),
                             verbose=False, hooks={"criterion_factory": lambda pw: Recording(pos_weight=pw)})
        runs[route] = (np.array(torch.stack(losses).double().cpu().tolist()), hist)
    (lt, ht), (ll, hl) = runs["torch"], runs["library"]
    assert lt.shape == ll.shape and lt.size > 2 * hp["num_epochs"]
    rel = np.abs(ll - lt) / lt
    print("mini-batch per-call loss, library vs torch route: max rel", rel.max())
    assert np.all(rel <= 1e-4), rel.max()
    assert np.allclose(hl.loss_train, ht.loss_train, rtol=1e-4, atol=0) and np.allclose(hl.loss_valid, ht.loss_valid, rtol=1e-4, atol=0)
    assert hl.lr == ht.lr and hl.final_lr == ht.final_lr                  # ReduceLROnPlateau changed lr at the same epochs
    assert hl.skipped_steps == 0 and ht.skipped_steps == 0 and ht.total_norm == []
