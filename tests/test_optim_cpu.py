"""CPU: the host side of the library's optimizer step -- the C ABI (declared, bound, exported, version 7, arguments refused
before any launch), the workspace size, the hyper-parameters of the training loop, dp.LibAdam's preconditions and checkpoint
schema (no launch involved), and the fp64 oracle of the GPU tier (tests/optim_reference.py) pinned to torch.optim.Adam in
float64."""
import os
import re

import numpy as np
import pytest
import torch

import optim_reference as ref

NAMES = ("gnm_optim_workspace_bytes", "gnm_optim_grad_stats", "gnm_optim_adam_step")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def test_abi_declares_binds_and_exports_the_entry_points(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib
    hdr = open(os.path.join(ge.REPO, "include", "gnm.h")).read()
    for name in NAMES:
        assert re.search(rf"\b(int|size_t) {name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "gnm_optim_stats" in hdr
    assert lib.gnm_abi_version() == 7 and "gnm_optim.hip" in ge.SOURCES


def test_workspace_bytes_is_monotone_and_covers_the_partials(lib):
    sizes = [0, 1, 3, 2047, 2048, 2049, 3 * 2048 + 5, 826033, 6600000, 2 ** 31 + 7]
    got = [lib.gnm_optim_workspace_bytes(n) for n in sizes]
    assert got == sorted(got)
    for n, b in zip(sizes, got):
        assert b >= 16 * ((n + ref.BLOCK - 1) // ref.BLOCK), (n, b)       # {double, int64} per block of 2048 elements
    assert lib.gnm_optim_workspace_bytes(2049) > lib.gnm_optim_workspace_bytes(2048) == lib.gnm_optim_workspace_bytes(1)


def test_bad_arguments_are_refused_before_any_launch(lib):
    one = 1 << 12                 # a non-null, aligned address that is never dereferenced: the checks fail first
    big = 1 << 20

    def stats(n=8, g=one, step=one, ws=one, wsb=big):
        return lib.gnm_optim_grad_stats(n, g, step, ws, wsb, None)

    def adam(n=8, p=one, g=one, m=one, v=one, step=one, st=one, ws=one, wsb=big, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, mx=0.0):
        return lib.gnm_optim_adam_step(n, p, g, m, v, step, st, ws, wsb, lr, b1, b2, eps, mx, None, 0, None)

    for bad in (dict(n=-1), dict(g=None), dict(step=None), dict(ws=None), dict(wsb=0), dict(n=2049, wsb=lib.gnm_optim_workspace_bytes(2048)),
                dict(ws=one + 4)):
        assert stats(**bad) < 0, bad
        assert b"optim_grad_stats" in lib.gnm_last_error()
    for bad in (dict(n=-1), dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(step=None), dict(st=None), dict(ws=None),
                dict(wsb=15), dict(n=2049, wsb=lib.gnm_optim_workspace_bytes(2048)), dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0),
                dict(b2=float("nan")), dict(eps=-1e-8), dict(eps=float("inf")), dict(lr=-1.0), dict(lr=float("nan")), dict(mx=-1.0),
                dict(st=one + 4)):
        assert adam(**bad) < 0, bad
        assert b"optim_adam_step" in lib.gnm_last_error()
    # n == 0: nothing to launch, success
    assert stats(n=0) == 0 and adam(n=0) == 0


def test_hyperparameter_defaults(monkeypatch):
    from gnnome_assembly_amd import train
    monkeypatch.delenv("GNM_OPTIM", raising=False)
    hp = train.get_hyperparameters()
    assert hp["optimizer"] == "torch" and hp["clip_grad_norm"] == 0.0
    monkeypatch.setenv("GNM_OPTIM", "library")
    assert train.get_hyperparameters()["optimizer"] == "library"
    assert train.History().skipped_steps == 0 and train.History().total_norm == []


def test_clip_without_the_library_route_raises():
    from gnnome_assembly_amd import train
    with pytest.raises(ValueError, match="clip_grad_norm"):         # decided before the samples are looked at
        train.train([], [], hyperparameters={"optimizer": "torch", "clip_grad_norm": 1.0}, verbose=False)
    with pytest.raises(ValueError, match="optimizer"):
        train.train([], [], hyperparameters={"optimizer": "adamw"}, verbose=False)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        train.train([], [], hyperparameters={"optimizer": "library", "clip_grad_norm": -1.0}, verbose=False)


def _flat_model():
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import models
    torch.manual_seed(3)
    model = G.GraphGatedGCNModel(1, 2, 64, 16, 1, 64, True, 16)
    models.flatten_parameters(model)
    return model


def test_libadam_names_the_precondition_that_failed():
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp
    plain = G.GraphGatedGCNModel(1, 2, 64, 16, 1, 64, True, 16)
    with pytest.raises(ValueError, match="not flattened"):
        dp.LibAdam(plain.parameters(), 1e-3)
    model = _flat_model()
    with pytest.raises(ValueError, match="FlatGradients"):
        dp.LibAdam(model.parameters(), 1e-3)
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    with pytest.raises(ValueError, match="flat float32 buffer"):
        dp.LibAdam(list(model.parameters())[1:], 1e-3, flat=flat)            # a hole in the buffer
    for kw in (dict(lr=-1.0), dict(betas=(0.9, 1.0)), dict(eps=-1.0), dict(max_norm=-1.0), dict(max_norm=float("nan"))):
        with pytest.raises(ValueError):
            dp.LibAdam(model.parameters(), **{"lr": 1e-3, **kw})
    other = dp.FlatGradients(_flat_model().parameters())
    with pytest.raises(ValueError, match="views of `flat`"):
        dp.LibAdam(model.parameters(), 1e-3, flat=other)
    opt = dp.LibAdam(model.parameters(), 1e-3, max_norm=2.0)                 # finds the live FlatGradients on its own
    assert opt.flat is flat and opt.gnm_impl == "library" and len(opt.param_groups) == 1
    assert opt.param_groups[0]["lr"] == 1e-3 and opt.param_groups[0]["max_norm"] == 2.0
    assert opt._p.data_ptr() == model._gnm_flat.data_ptr() and opt._p.numel() == model._gnm_flat.numel()
    with pytest.raises(Exception, match="HIP device"):                       # no CPU route for the step itself
        opt.step()


def test_libadam_checkpoint_schema_and_interchange_on_the_host():
    from gnnome_assembly_amd import dp
    model = _flat_model()
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    opt = dp.LibAdam(model.parameters(), 1e-3, flat=flat)
    params = list(model.parameters())
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["state"]) == len(params)
    for st in sd["state"].values():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].dtype == torch.float32 and st["step"].dim() == 0
    assert sd["state"][0]["exp_avg"].data_ptr() != opt.state[params[0]]["exp_avg"].data_ptr()          # clones
    # torch -> library
    tor = torch.optim.Adam(model.parameters(), lr=3e-3)
    for _ in range(2):
        for p in params:
            p.grad.normal_()
        tor.step()
    opt.load_state_dict(tor.state_dict())
    assert float(opt._step) == 2.0 and opt.param_groups[0]["lr"] == 3e-3 and opt.param_groups[0]["max_norm"] == 0.0
    lo, hi = opt._m.data_ptr(), opt._m.data_ptr() + opt._m.numel() * 4
    for p in params:
        assert lo <= opt.state[p]["exp_avg"].data_ptr() < hi and opt.state[p]["step"] is opt._step
        assert torch.equal(opt.state[p]["exp_avg"], tor.state[p]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], tor.state[p]["exp_avg_sq"])
    # library -> torch: the loaded optimizer takes a step
    back = torch.optim.Adam(model.parameters(), lr=1e-3)
    back.load_state_dict(opt.state_dict())
    assert all(float(back.state[p]["step"]) == 2.0 and torch.equal(back.state[p]["exp_avg_sq"], tor.state[p]["exp_avg_sq"]) for p in params)
    back.step()
    assert float(back.state[params[0]]["step"]) == 3.0
    # disagreeing step counts are refused, and the refusal leaves the optimizer as it was
    bad = tor.state_dict()
    bad["state"][1] = dict(bad["state"][1], step=torch.tensor(7.0))
    with pytest.raises(ValueError, match="disagree"):
        opt.load_state_dict(bad)
    assert float(opt._step) == 2.0 and opt.param_groups[0]["lr"] == 3e-3
    wd = tor.state_dict()
    wd["param_groups"][0]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="weight_decay"):
        opt.load_state_dict(wd)
    # ReduceLROnPlateau drives the group's lr, which step() reads
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0)
    sch.step(1.0)
    sch.step(2.0)
    assert opt.param_groups[0]["lr"] == 1.5e-3


@pytest.mark.parametrize("n", [1, 3, 2049])
def test_reference_is_torch_adam_in_float64(n):
    """Clipping off: the oracle is torch.optim.Adam, to 1e-12 relative, over 5 steps."""
    p0, grads = ref.make_case(n, seed=100 + n)
    r = ref.AdamRef(p0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    p = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    for g in grads:
        p.grad = torch.from_numpy(g).double()
        opt.step()
        r.step(g)
        for got, want in ((r.p, p.detach()), (r.m, opt.state[p]["exp_avg"]), (r.v, opt.state[p]["exp_avg_sq"])):
            want = want.numpy()
            assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (n, np.abs(got - want).max())
    assert r.t == 5 and r.skipped == 0 and r.clip == 1.0


def test_reference_guard_clip_and_count():
    p0, grads = ref.make_case(64, seed=7, steps=2)
    r = ref.AdamRef(p0, max_norm=1.0)
    g = grads[0].copy()
    g[3], g[40] = np.nan, np.inf
    before = (r.p.copy(), r.m.copy(), r.v.copy(), r.t)
    r.step(g)
    assert r.nonfinite == 2 and r.skipped == 1 and r.t == before[3] == 0
    assert all(np.array_equal(a, b) for a, b in zip(before[:3], (r.p, r.m, r.v)))
    r.step(grads[0], count=2.0)
    norm = np.sqrt((grads[0].astype(np.float64) ** 2).sum()) / 2
    assert abs(r.total_norm - norm) <= 1e-12 * norm and abs(r.clip - 1.0 / (norm + 1e-6)) <= 1e-15 and r.t == 1
    # first step: m = (1 - b1) gh and the bias correction undoes it -> |dp| = lr |gh| / (|gh| + eps)
    gh = grads[0].astype(np.float64) / 2 * r.clip
    want = p0.astype(np.float64) - 1e-3 * gh / (np.abs(gh) + 1e-8)
    assert np.allclose(r.p, want, rtol=0, atol=1e-12)
    assert np.array_equal(r.p[grads[0] == 0], p0.astype(np.float64)[grads[0] == 0])          # 0 / (0 + eps) stays 0
