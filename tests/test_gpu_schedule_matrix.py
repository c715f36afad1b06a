"""The schedule switches of engine.Options in combination (-m gpu): every row of helpers.SCHEDULE_ROWS -- a pairwise cover of the
two levels of the 11 switches, of asking for the input gradients and of the flat direct-write gradients -- runs a training step
through GraphGatedGCNModel at every width route (32 native, 64 / 96 zero-padded to 128, 128 fused, 256 wide-fused, 320 / 512 as
256-column chunks) and both norms, under all three matmul modes, against the fp64 oracle.  The one-switch tests of
test_gpu_parity.py change a single switch against the default route; the switches are documented to compute the same thing
whatever the others are, and this file checks that claim:
  - every row that keeps its activations: logits, loss, parameter gradients (and input gradients) against the fp64 oracle with
    the clauses of test_gpu_parity.test_other_widths_and_norms_vs_oracle / test_gpu_input_grads._check;
  - every lean row: bit-identical to the same row with saved activations (that twin carries the oracle check);
  - every row whose forward switches are the defaults': logits and loss bit-identical to row r0, gradients within the bar of the
    one-switch tests.
No combination in the matrix is refused by design (LayerNorm wider than 256 is, with NotImplementedError, and is not in it)."""
import numpy as np
import pytest
import torch

from helpers import (GRAD_ABS_FLOOR, SCHEDULE_FORWARD, SCHEDULE_ROWS, _branch_exact, _branch_exact_or_fail, _check, _grad_ok,
                     assert_parity, branch_exact_rows, rel_l2, schedule_switches, sd_to_torch)
from oracle import gatedgcn_oracle as orc

pytestmark = pytest.mark.gpu

# (H, batch_norm, L)
CONFIGS = [(32, True, 2), (32, False, 2), (64, True, 2), (96, False, 2), (128, True, 3), (128, False, 3), (256, True, 2),
           (256, False, 2), (320, True, 2), (512, True, 1)]
SEED = 7
LEAN_ROWS = [r for r, row in SCHEDULE_ROWS.items() if row["ACTIVATIONS"] == "lean"]
SAME_FORWARD_ROWS = [r for r, row in SCHEDULE_ROWS.items() if r != "r0"
                     and all(row[k] == SCHEDULE_ROWS["r0"][k] for k in SCHEDULE_FORWARD)]


@pytest.fixture(autouse=True, params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request):
    """Every test of this file runs under ALL THREE matmul modes of the fused kernels (include/gnm.h):
    "f16x2" -- the library default, the mode bench.py's `value` is measured in: two fp16 terms of a power-of-two
    multiple, three MFMAs per product --, "bf16x3" (the exact three-term split, six MFMAs
    per product; the default of rounds 2-4) and the fp32-MFMA mode.  Tests that never reach a fused kernel are marked
    `mode_independent` and run once."""
    from gnnome_assembly_amd import _lib
    if request.param != _lib.DEFAULT_MATMUL_MODE and (request.node.get_closest_marker("mode_independent")
                                                      or request.node.get_closest_marker("default_mode_only")):
        pytest.skip("runs once (does not depend on the matmul mode, or too large to run twice)")
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_ORACLE = {}


def _case(cfg):
    """Inputs, parameters and the fp64 oracle (logits, loss, parameter and input gradients) of a configuration -- computed once,
    shared by its rows and matmul modes."""
    if cfg in _ORACLE:
        return _ORACLE[cfg]
    from gnnome_assembly_amd import synth
    H, bn, L = cfg
    src, dst, n = synth.make_graph(700, SEED, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed=H)
    sd = synth.synth_state_dict(H, L, seed=L)
    c = dict(src=src, dst=dst, n=n, e=inp["e"], pe=inp["pe"], y=inp["y"], pw=float(inp["pos_weight"]), sd=sd)
    p64 = sd_to_torch(sd, torch.float64, requires_grad=True)
    e64 = torch.from_numpy(inp["e"]).double().requires_grad_(True)
    pe64 = torch.from_numpy(inp["pe"]).double().requires_grad_(True)
    s64 = orc.model_forward(p64, torch.from_numpy(src), torch.from_numpy(dst), n, e64, pe64, bn)
    l64 = orc.bce_loss(s64, torch.from_numpy(inp["y"]).double(), c["pw"])
    l64.backward()
    c.update(s64=s64.detach().numpy(), l64=l64.item(), g64={k: v.grad.numpy() for k, v in p64.items()},
             ge64=e64.grad.numpy(), gpe64=pe64.grad.numpy())
    _ORACLE[cfg] = c
    return c


def _step(cfg, c, row, g, dev):
    """One training step of a fresh model under the row's switches: GraphGatedGCNModel -> BCEWithLogitsLoss -> backward."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp, engine, layers
    H, bn, L = cfg
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, bn, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()})
    model.to(dev)
    e = torch.from_numpy(c["e"]).to(dev).requires_grad_(row["inputs"])
    pe = torch.from_numpy(c["pe"]).to(dev).requires_grad_(row["inputs"])
    flat = None
    if row["flat"]:
        model.flatten_parameters()
        flat = dp.FlatGradients(model.parameters(), direct_write=True)
        flat.zero_()
    with engine.options(**schedule_switches(row)):
        s = model(g, None, e, pe)
        loss = G.BCEWithLogitsLoss(c["pw"])(s.squeeze(-1), torch.from_numpy(c["y"]).to(dev))
        loss.backward()
    torch.cuda.synchronize()
    if flat is not None and layers.padded_width(H) == H:
        assert not flat.fresh, "the direct-write gradient path was not taken"
    return dict(s=s.detach().cpu(), loss=loss.item(), grads={k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()},
                ge=e.grad.cpu() if row["inputs"] else None, gpe=pe.grad.cpu() if row["inputs"] else None)


def _vs_oracle(cfg, c, res, row, g, dev, what):
    """The clauses of test_other_widths_and_norms_vs_oracle (parameter gradients) and test_gpu_input_grads (e / pe); the
    branch-exact comparisons run the engine under the row's switches."""
    H, bn, L = cfg
    assert_parity(res["s"].numpy(), c["s64"], f"{what} logits")
    assert abs(res["loss"] - c["l64"]) < 1e-5, (what, res["loss"], c["l64"])
    bad = []
    for k, want in c["g64"].items():
        got = res["grads"][k].double().numpy()
        r = rel_l2(got, want)
        if not _grad_ok(r, float(np.abs(got - want).max()), GRAD_ABS_FLOOR):
            bad.append((k, r))
    from gnnome_assembly_amd import engine
    with engine.options(**schedule_switches(row)):
        if bad:             # only relu-kink flips may explain a miss, under either norm; no noise clause
            brows, bgmax = branch_exact_rows(c["src"], c["dst"], c["n"], c["e"], c["pe"], c["y"], c["pw"], c["sd"], L, dev, bn)
            _branch_exact_or_fail(bad, {r[0]: r for r in brows}, bgmax, what)
        if row["inputs"]:
            exact = lambda: _branch_exact(g, c["sd"], H, L, c["e"], c["pe"], c["y"], c["pw"], dev, bn)  # noqa: E731
            _check(res["ge"].numpy(), res["gpe"].numpy(), c["ge64"], c["gpe64"], what, exact)


def _identical(a, b, what):
    assert torch.equal(a["s"], b["s"]) and a["loss"] == b["loss"], f"{what}: logits / loss differ"
    for k in b["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), f"{what}: {k}"
    for k in ("ge", "gpe"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), f"{what}: {k}"


@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"h{H}_{'bn' if bn else 'ln'}_l{L}" for H, bn, L in CONFIGS])
def test_schedule_rows_match_the_oracle(cfg):
    """Every SCHEDULE_ROWS row of one configuration in the current matmul mode (see the module docstring)."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine, layers
    dev = _dev()
    H, bn, L = cfg
    c = _case(cfg)
    g = G.AssemblyGraph(c["src"], c["dst"], c["n"]).to(dev)
    Hp = layers.padded_width(H)
    if engine.sweep_width(Hp, bn):          # the two-sided switches change something only where a plan exists
        for plan in (g.sweep_plan(dev), g.sweep_plan(dev, engine.GATE2_WG)):
            assert plan is not None and 0 < plan["nfix"] < 0.2 * c["n"], plan and plan["nfix"]
            print(f"{cfg}: sweep plan leaves {plan['nfix']} of {c['n']} nodes to the fix-up pass")
    res = {}
    for r, row in SCHEDULE_ROWS.items():
        what = f"H={H} {'BN' if bn else 'LN'} L={L} {r}"
        res[r] = _step(cfg, c, row, g, dev)
        if r in LEAN_ROWS:
            twin = dict(row, ACTIVATIONS="saved")
            saved = _step(cfg, c, twin, g, dev)
            _identical(res[r], saved, f"{what} lean vs saved")
            _vs_oracle(cfg, c, saved, twin, g, dev, f"{what} (saved twin)")
        else:
            _vs_oracle(cfg, c, res[r], row, g, dev, what)
    base = res["r0"]
    gmax = max(float(v.abs().max()) for v in base["grads"].values())
    for r in SAME_FORWARD_ROWS:         # the forward reads only FUSED, TWO_SIDED_FWD, WIDE_FUSED
        assert torch.equal(res[r]["s"], base["s"]) and res[r]["loss"] == base["loss"], f"{r}: forward differs from r0"
        bad = []
        for k, b in base["grads"].items():
            a, b = res[r]["grads"][k].double(), b.double()
            rr = float((a - b).norm() / b.norm().clamp_min(1e-30))
            if rr > 2e-5 and float((a - b).abs().max()) > 1e-6 * gmax:
                bad.append((k, rr))
        assert not bad, (r, bad)
