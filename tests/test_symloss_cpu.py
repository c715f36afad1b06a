"""CPU: the premise of the symmetry loss -- the model on the edge-reversed graph IS the model on the same graph with mirrored
parameters (models.mirror_state), forward and gradients, in fp64 through the oracle -- the mirror as an involution and as a
permutation of the flat buffer, the fp64 statement of the loss against the torch expression, and the hyper-parameters."""
import numpy as np
import pytest
import torch

from symloss_common import (CONFIGS, GRAPHS, load_graph, oracle_scores, state_dict64, swap_degree_columns, sym_closed_form,
                            sym_loss_fp64)


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


@pytest.mark.parametrize("which", list(GRAPHS))
@pytest.mark.parametrize("H,L,bn", CONFIGS)
def test_premise_reversed_graph_equals_mirrored_parameters(which, H, L, bn):
    """oracle(M sd, src, dst, pe) == oracle(sd, dst, src, pe[:, [1, 0, 2, ...]]) to 1e-12 rel-L2 in fp64, and for a scalar of the
    scores grad_theta of the left side (autograd through mirror_state) == grad_theta of the right side (the really reversed graph)
    == M applied to the gradient with respect to theta' = M theta of the same-graph model (the fold the engine uses)."""
    from gnnome_assembly_amd.models import mirror_state
    src, dst, n, e_raw, pe, y, pw = load_graph(which)
    theta = state_dict64(H, L, seed=3, requires_grad=True)
    w = torch.from_numpy(np.random.default_rng(5).standard_normal(src.size))        # the scalar: a fixed random functional
    left = oracle_scores(mirror_state(theta), src, dst, n, e_raw, pe, bn)
    g_left = torch.autograd.grad((left * w).sum(), list(theta.values()), allow_unused=True)
    right = oracle_scores(theta, src, dst, n, e_raw, pe, bn, reverse=True)
    g_right = dict(zip(theta, torch.autograd.grad((right * w).sum(), list(theta.values()), allow_unused=True)))
    # the fold the engine uses: theta' = M theta as a leaf, the gradient with respect to theta', then M of it
    prime = {k: v.detach().clone().requires_grad_(True) for k, v in mirror_state(theta).items()}
    same = oracle_scores(prime, src, dst, n, e_raw, pe, bn)
    g_prime = dict(zip(prime, torch.autograd.grad((same * w).sum(), list(prime.values()), allow_unused=True)))
    r = _rel(left.detach(), right.detach())
    print(f"{which} H={H} L={L} bn={bn}: scores rel-L2 {r:.2e}")
    assert r <= 1e-12
    # differs from the unreversed scores: the check has teeth
    assert _rel(oracle_scores(theta, src, dst, n, e_raw, pe, bn).detach(), right.detach()) > 1e-3
    assert all(g is not None for g in g_left) and all(g is not None for g in g_right.values())
    assert all(g is not None for g in g_prime.values()) and torch.equal(same.detach(), left.detach())
    mg = mirror_state(g_prime)
    scale = max(float(g.norm()) for g in g_right.values())
    for (k, _), gl in zip(theta.items(), g_left):
        lim = 1e-12 * max(float(g_right[k].norm()), 1e-3 * scale)
        d_real, d_fold = float((gl - g_right[k]).norm()), float((gl - mg[k]).norm())
        assert d_real <= lim and d_fold <= lim, (k, d_real, d_fold, float(g_right[k].norm()))


def test_mirror_is_an_involution_and_a_permutation_of_the_flat_buffer():
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import models
    for H, L, bn in CONFIGS + [(48, 2, True)]:
        torch.manual_seed(H)
        model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, bn, 16)
        for p in model.parameters():            # biases and norms are constant at init: make every element distinct
            p.data.copy_(torch.randn_like(p))
        named = dict(model.named_parameters())
        m = models.mirror_state(named)
        mm = models.mirror_state(m)
        assert set(m) == set(named) and all(m[k].shape == named[k].shape for k in named)
        assert all(torch.equal(mm[k], named[k]) for k in named)
        moved = [k for k in named if not torch.equal(m[k], named[k])]
        assert len(moved) == 8 * L + 2, moved         # A_2 A_3 B_1 B_2 (weight, bias) per layer, linear_pe.weight, W1.weight
        p0 = "gnn.convs.0."
        assert torch.equal(m[p0 + "A_2.weight"], named[p0 + "A_3.weight"]) and torch.equal(m[p0 + "B_1.bias"], named[p0 + "B_2.bias"])
        assert torch.equal(m["linear_pe.weight"], swap_degree_columns(named["linear_pe.weight"]))
        W1 = named["predictor.W1.weight"]
        assert torch.equal(m["predictor.W1.weight"], torch.cat([W1[:, H:2 * H], W1[:, :H], W1[:, 2 * H:]], 1))
        with pytest.raises(RuntimeError):
            models.mirror_index(G.GraphGatedGCNModel(1, 2, H, 16, L, 64, bn, 16))
        flat = models.flatten_parameters(model)
        pi = models.mirror_index(model)
        assert pi.dtype == torch.int32 and pi.shape == flat.shape and models.mirror_index(model) is pi
        assert torch.equal(pi[pi.long()].long(), torch.arange(flat.numel()))
        order = models._engine_order(list(named))
        named = dict(model.named_parameters())
        want = torch.cat([models.mirror_state(named)[k].reshape(-1) for k in order])
        assert torch.equal(flat[pi.long()], want)
        # per layer the stacked projections A_1 A_2 A_3 B_1 B_2 move as whole blocks in the order (0, 2, 1, 4, 3)
        blk = pi[:5 * H * H].long().view(5, H * H)
        assert torch.equal(blk, torch.arange(5 * H * H).view(5, H * H)[[0, 2, 1, 4, 3]])
        models.flatten_parameters(model)              # a new flattening: a new permutation object
        assert models.mirror_index(model) is not pi and torch.equal(models.mirror_index(model), pi)


@pytest.mark.parametrize("alpha", [0.0, 0.1, 1.0])
def test_fp64_statement_equals_the_torch_expression(alpha):
    rng = np.random.default_rng(11)
    E, pw = 1000, 0.27
    o = torch.from_numpy(rng.uniform(-80, 80, E)).requires_grad_(True)
    r0 = rng.uniform(-80, 80, E)
    r0[::10] = o.detach().numpy()[::10]               # ties: the subgradient is 0 there
    r = torch.from_numpy(r0).requires_grad_(True)
    y = torch.from_numpy((rng.random(E) < 0.5).astype(np.float64))
    bce = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw], dtype=torch.float64), reduction="none")
    want = (bce(o, y) + bce(r, y) + alpha * (o - r).abs()).mean()
    wo, wr = torch.autograd.grad(want, [o, r])
    loss, parts = sym_loss_fp64(o, r, y, pw, alpha)
    go, gr = torch.autograd.grad(loss, [o, r])
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-13 * abs(float(want.detach()))
    # torch forms 1 - sigma(x) by subtraction: its own gradient is off by up to one fp64 ulp of 1.0 times pos_weight / E where the
    # statement here (sigma(-x)) is not -- the absolute term
    floor = 2.3e-16 * max(pw, 1.0) / E
    assert torch.allclose(go, wo, rtol=1e-12, atol=floor) and torch.allclose(gr, wr, rtol=1e-12, atol=floor)
    assert abs(float(parts[2].detach()) - float((o - r).abs().mean().detach())) <= 1e-15 * float(parts[2].detach())
    cl, cparts, cgo, cgr, bo, br = sym_closed_form(o.detach().numpy(), r0, y.numpy(), pw, alpha)
    assert abs(cl - float(want.detach())) <= 1e-13 * abs(float(want.detach())) and np.allclose(cparts, parts.detach().numpy(), rtol=1e-13, atol=0)
    lim = 1e-12 * (np.abs(bo) + alpha / E) + floor
    assert np.all(np.abs(cgo - wo.numpy()) <= lim) and np.all(np.abs(cgr - wr.numpy()) <= lim)
    if alpha:
        assert np.all(cgo[::10] == bo[::10]) and np.all(cgr[::10] == br[::10])       # sgn(0) = 0


def test_hyperparameter_defaults_and_the_sequential_dropout_refusal(monkeypatch):
    from gnnome_assembly_amd import train as T
    monkeypatch.delenv("GNM_SYMMETRY_LOSS", raising=False)
    hp = T.get_hyperparameters()
    assert hp["symmetry_loss"] is False and hp["alpha"] == 0.1 and hp["symmetry_schedule"] == "joint"
    assert T.check_symmetry_hyperparameters(hp) is False
    monkeypatch.setenv("GNM_SYMMETRY_LOSS", "1")
    assert T.get_hyperparameters()["symmetry_loss"] is True
    on = dict(hp, symmetry_loss=True)
    assert T.check_symmetry_hyperparameters(on) is True
    assert T.check_symmetry_hyperparameters(dict(on, symmetry_schedule="sequential")) is True
    assert T.check_symmetry_hyperparameters(dict(on, dropout=0.2)) is True
    with pytest.raises(ValueError, match="sequential.*dropout"):
        T.check_symmetry_hyperparameters(dict(on, symmetry_schedule="sequential", dropout=0.2))
    with pytest.raises(ValueError, match="symmetry_schedule"):
        T.check_symmetry_hyperparameters(dict(on, symmetry_schedule="both"))
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            T.check_symmetry_hyperparameters(dict(on, alpha=bad))
    h = T.History()
    assert h.sym_gap_train == [] and h.sym_gap_valid == []
