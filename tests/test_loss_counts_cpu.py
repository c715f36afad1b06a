"""CPU: the C ABI of the fused loss + metric-count pass (gnm_bce_stats_fwd_bwd), the derivation of the threshold its kernel
uses instead of round(sigmoid(x)), and train.train's fall-back for criteria without with_counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from loop_common import CountingBCE, mix_sample, oracle_model_factory
from loss_counts_common import (REPO, WINDOW, X_STAR, bits_to_f32, boundary_logits, f32_bits, rule_counts, source_constant,
                                steps_from_zero, torch_counts)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def test_symbols_declared_bound_exported(lib):
    from gnnome_assembly_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gnm.h")).read(), flags=re.S)
    for name in ("gnm_bce_stats_workspace_bytes", "gnm_bce_stats_fwd_bwd"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.gnm_abi_version() == _lib.ABI_VERSION == 7
    # loss partials (double) + four int32 counts for every block the loss kernels may launch
    assert lib.gnm_bce_stats_workspace_bytes() == lib.gnm_max_partial_blocks() * (8 + 4 * 4)


def _p1_scalar(bits: int) -> bool:
    """round(sigmoid(x)) == 1 on a ONE-element tensor (torch's scalar code path)."""
    return bool(torch.round(torch.sigmoid(bits_to_f32([bits])))[0] == 1)


def test_threshold_derivation():
    """X_STAR is the smallest fp32 x with torch.round(torch.sigmoid(x)) == 1: bisection over the bit patterns of the positive
    floats (ordered like the values), then the decision is checked to be monotone -- 0 below, 1 from X_STAR on -- within 4096
    steps of X_STAR and of 0, element by element (scalar path) and in one long contiguous tensor (vector path)."""
    lo, hi = f32_bits(0.0), f32_bits(1.0)
    assert not _p1_scalar(lo) and _p1_scalar(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _p1_scalar(mid):
            hi = mid
        else:
            lo = mid
    assert bits_to_f32([hi])[0].item() == X_STAR and hi == 0x33C00001
    assert source_constant() == X_STAR
    assert X_STAR > 0 and torch.sigmoid(torch.tensor([X_STAR / 2]))[0] == 0.5      # small positive logits: exactly 0.5 -> 0
    around_star = np.arange(hi - WINDOW, hi + WINDOW + 1)
    xs = torch.cat([bits_to_f32(around_star), steps_from_zero(np.arange(-WINDOW, WINDOW + 1))])
    want = torch.cat([torch.from_numpy(around_star >= hi), torch.zeros(2 * WINDOW + 1, dtype=torch.bool)])
    scalar = torch.tensor([bool(torch.round(torch.sigmoid(xs[i:i + 1]))[0] == 1) for i in range(xs.numel())])
    assert torch.equal(scalar, want)
    long = xs.repeat(16).contiguous()                          # 262 k elements: vectorised (and threaded) evaluation
    assert torch.equal(torch.round(torch.sigmoid(long)) == 1, want.repeat(16))
    assert torch.equal(xs >= X_STAR, want) and torch.equal(xs < X_STAR, ~want)
    # ... and p == 0 there exactly when not p == 1 (no third value for finite logits)
    assert torch.equal(torch.round(torch.sigmoid(long)) == 0, ~want.repeat(16))


@pytest.mark.parametrize("scale", [1e-7, 1.0, 30.0])
def test_rule_equals_torch_expression(scale):
    """x >= X_STAR / x < X_STAR against round(sigmoid(x)) == 1 / == 0, as counts against labels from {0, 1, 0.5, nan}: the two
    windows, +-inf and nan (boundary_logits), and randn logits at three scales."""
    g = torch.Generator().manual_seed(int(scale * 10) + 1)
    x = torch.cat([boundary_logits(), torch.randn(200000, generator=g) * scale])
    y = torch.tensor([0.0, 1.0, 0.5, float("nan")])[torch.randint(0, 4, (x.numel(),), generator=g)]
    p = torch.round(torch.sigmoid(x))
    assert torch.equal(p == 1, x >= X_STAR) and torch.equal(p == 0, x < X_STAR)
    want = torch_counts(x, y)
    assert rule_counts(x, y) == want
    assert min(want) > 0 and sum(want) < x.numel()            # every class occurs; nan / 0.5 entries are counted nowhere
    for v in (float("inf"), float("-inf"), float("nan")):
        xv = torch.full((4,), v)
        yv = torch.tensor([0.0, 1.0, 0.5, float("nan")])
        assert rule_counts(xv, yv) == torch_counts(xv, yv)
    assert rule_counts(torch.full((2,), float("nan")), torch.tensor([0.0, 1.0])) == (0, 0, 0, 0)


def test_invalid_arguments_return_error_without_a_device(lib):
    need = lib.gnm_bce_stats_workspace_bytes()
    x = np.zeros(8, np.float32)
    y = np.zeros(8, np.float32)
    loss = np.zeros(1, np.float32)
    counts = np.full(4, -7, np.int64)
    ws = np.zeros(need // 8, np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lib.gnm_bce_stats_fwd_bwd
    assert call(8, None, p(y), 1.0, p(loss), None, p(counts), None, p(ws), need, None) < 0
    assert b"bce_stats_fwd_bwd" in lib.gnm_last_error()
    assert call(8, p(x), None, 1.0, p(loss), None, p(counts), None, p(ws), need, None) < 0
    assert call(8, p(x), p(y), 1.0, None, None, p(counts), None, p(ws), need, None) < 0
    assert call(8, p(x), p(y), 1.0, p(loss), None, None, None, p(ws), need, None) < 0
    assert call(8, p(x), p(y), 1.0, p(loss), None, p(counts), None, None, need, None) < 0
    assert call(8, p(x), p(y), 1.0, p(loss), None, p(counts), None, p(ws), need - 1, None) < 0
    assert b"workspace" in lib.gnm_last_error()
    assert call(0, p(x), p(y), 1.0, p(loss), None, p(counts), None, p(ws), need, None) < 0      # as gnm_bce_fwd_bwd: E > 0
    assert (counts == -7).all() and loss[0] == 0


def test_train_falls_back_for_a_criterion_without_with_counts(lib, tmp_path, monkeypatch):
    """fused_metrics=True with a criterion_factory stand-in (torch's loss: no with_counts) takes the torch route and gives the
    History of the off run; GNM_FUSED_METRICS=1 sets the hyper-parameter's default."""
    from gnnome_assembly_amd import train as T
    monkeypatch.delenv("GNM_FUSED_METRICS", raising=False)
    assert T.get_hyperparameters()["fused_metrics"] is False
    monkeypatch.setenv("GNM_FUSED_METRICS", "1")
    assert T.get_hyperparameters()["fused_metrics"] is True
    monkeypatch.delenv("GNM_FUSED_METRICS")
    hooks = {"model_factory": oracle_model_factory,
             "criterion_factory": lambda pw: torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw]))}
    assert not hasattr(hooks["criterion_factory"](1.0), "with_counts")
    runs = []
    for fused in (False, True):
        tr, va = [mix_sample(60, 1), mix_sample(50, 2)], [mix_sample(40, 3)]
        hp = dict(num_epochs=2, dim_latent=32, num_gnn_layers=1, lr=1e-3, seed=0, fused_metrics=fused)
        model, best, hist = T.train(tr, va, out="fb", hyperparameters=hp, workdir=str(tmp_path / str(fused)), verbose=False,
                                    hooks=hooks)
        runs.append((hist, model.state_dict()))
    (h0, s0), (h1, s1) = runs
    assert len(h0.step_losses) == 4 and len(h0.tfpn_train) == 2 and sum(h0.tfpn_train[0]) > 0
    assert h0 == h1                                                         # dataclass equality: every field
    assert all(torch.equal(s0[k], s1[k]) for k in s0)


@pytest.mark.parametrize("masking", [False, True])
@pytest.mark.parametrize("batch_size_eval", [1, 3])
@pytest.mark.parametrize("batch_size_train", [1, 20])
def test_train_fused_route_with_a_counting_stand_in_equals_the_torch_route(lib, tmp_path, monkeypatch, batch_size_train, batch_size_eval,
                                                                           masking):
    """The loop's fused-metrics route on the CPU: a criterion_factory stand-in WITH with_counts (loop_common.CountingBCE, which
    fills the EpochStats it is handed as the loss kernel does) against torch's loss, which takes the torch route -- full graph
    and mini-batch, training and validation, with and without read masking: the same History (every field) and the same final
    parameters, bit for bit."""
    from gnnome_assembly_amd import train as T
    torch.set_num_threads(1)
    hp = dict(num_epochs=2, dim_latent=32, num_gnn_layers=1, lr=1e-3, seed=0, fused_metrics=True,
              batch_size_train=batch_size_train, num_parts_metis_train=101, batch_size_eval=batch_size_eval, num_parts_metis_eval=8)
    if masking:
        hp.update(mask_frac_low=80, mask_frac_high=100)
    runs, calls, orig = [], [], CountingBCE.with_counts
    monkeypatch.setattr(CountingBCE, "with_counts", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    for cls in (torch.nn.BCEWithLogitsLoss, CountingBCE):
        tr = [mix_sample(r, s) for r, s in ((120, 0), (90, 1), (100, 2))]
        va = [mix_sample(60, 100), mix_sample(40, 101)]
        hooks = {"model_factory": oracle_model_factory, "criterion_factory": lambda pw: cls(pos_weight=torch.tensor([pw]))}
        model, _, hist = T.train(tr, va, out="m", hyperparameters=hp, workdir=str(tmp_path / cls.__name__), verbose=False, hooks=hooks)
        runs.append((hist, torch.cat([p.detach().reshape(-1) for p in sorted(model.parameters(), key=lambda p: p._gnm_slot)])))
    (h0, f0), (h1, f1) = runs
    assert len(calls) >= 2 * (3 + 2)                                        # the stand-in run took the fused route: every step and evaluation
    assert len(h0.loss_train) == len(h0.loss_valid) == 2 and sum(h0.tfpn_train[0]) > 0 and sum(h0.tfpn_valid[0]) > 0
    assert (len(h0.step_losses) == 6) == (batch_size_train == 1) and (len(h0.mask_fraction) > 0) == masking
    assert h0 == h1                                                         # dataclass equality: every field
    assert torch.equal(f0, f1)
