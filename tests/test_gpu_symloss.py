"""GPU: the symmetry loss -- gnm_sym_bce_fwd_bwd against the fp64 closed form, the reversed pass (model(..., reverse=True)) against
the fp64 oracle on the really reversed graph, the gradients of the whole loss on every route, and train.train with it on.

Bounds.  Loss and parts: 1e-6 relative (+1e-37), what tests/test_gpu_heads.py::test_bce_vs_closed_form_fp64 allows the plain kernel;
|o - r| is one fp32 subtraction (2^-24 relative) summed in fp64 and needs no more.  A gradient element without a symmetry term
(alpha = 0 or o == r) has the plain kernel's bound, 1e-6 |bce'/E| + max(pw, 1) x the smallest normal fp32.  With the term the
kernel adds t = +-fl(alpha / E) to fl(bce'/E) in fp32: t is rounded once (2^-24 alpha/E) and the sum once (2^-24 |a + t|), so the
bound grows by 2^-23 (|bce'/E| + alpha/E) -- relative to the two addends, not to their sum, which can cancel to nothing.  This
term derived from the number format stands in place of the measured figure (4 x the fp32-vs-fp64 error of the torch expression on
the same data) that would otherwise set a wider bound: it is about two ulp of the addends, tighter than that rule would give.
Logits: helpers.assert_parity, the bar of tests/test_gpu_parity.py.  Parameter gradients: rel-L2 <= helpers.GRAD_L2 per tensor or
max-abs under max(GRAD_ABS_FLOOR, 1e-6 x the largest gradient norm), the plain bar and absolute floor of the gradient parity test;
a tensor outside the plain bar must be exact (rel-L2 <= helpers.BRANCH_L2) against the fp64 gradient on the relu and sign branches
the device took (symloss_common.branch_exact_sym_grads), as in that test."""
import numpy as np
import pytest
import torch

from helpers import BRANCH_L2, GRAD_ABS_FLOOR, GRAD_L2, assert_parity, rel_l2
from loss_counts_common import torch_counts
from symloss_common import (CONFIGS, GRAPHS, branch_exact_sym_grads, load_graph, oracle_scores, oracle_sym_loss, state_dict64, swap_degree_columns,
                            sym_closed_form)
from test_gpu_loss_counts import _Runner, _bits, _samples, _sizes

pytestmark = pytest.mark.gpu

PW = 0.25
DEV = "cuda:0"
# The weights are synth.synth_state_dict(H, L, SEED), the seed the golden files themselves carry (both graphs are the _s0 fixtures).
SEED = 0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


class _Sym:
    """gnm_sym_bce_fwd_bwd on caller-owned buffers; outputs start as sentinels, the workspace as 0xFF bytes."""

    def __init__(self, lib):
        from gnnome_assembly_amd import engine
        self.lib, self.e, self.dev = lib, engine, torch.device(DEV)
        self.ws = torch.empty(lib.gnm_sym_bce_workspace_bytes(), dtype=torch.uint8, device=self.dev)

    def raw(self, E, o, r, y, pw, alpha, loss, parts, go, gr, counts, acc, ws_bytes=None):
        p = self.e._ptr
        return self.lib.gnm_sym_bce_fwd_bwd(E, p(o), p(r), p(y), pw, alpha, p(loss), p(parts), p(go), p(gr), p(counts), p(acc),
                                            p(self.ws), self.ws.numel() if ws_bytes is None else ws_bytes, self.e._stream())

    def __call__(self, o, r, y, alpha, grad=True, acc=None, pw=PW):
        E = o.numel()
        loss, parts = torch.full((1,), -1.0, device=self.dev), torch.full((3,), -1.0, device=self.dev)
        go = torch.full((E,), -1.0, device=self.dev) if grad else None
        gr = torch.full((E,), -1.0, device=self.dev) if grad else None
        counts = torch.full((4,), -1, dtype=torch.int64, device=self.dev)
        self.ws.fill_(0xFF)
        rc = self.raw(E, o, r, y, pw, alpha, loss, parts, go, gr, counts, acc)
        assert rc == 0, self.lib.gnm_last_error()
        return loss, parts, go, gr, counts


@pytest.fixture(scope="module")
def sym(lib):
    return _Sym(lib)


def _case(E, seed):
    """Finite logits spanning +-80; every tenth pair bit-equal, the next differing in the last bit upwards, the next downwards."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-80, 80, E).astype(np.float32)
    r = np.where(rng.random(E) < 0.5, rng.uniform(-80, 80, E), o + rng.standard_normal(E)).astype(np.float32)
    r[0::10] = o[0::10]
    r[1::10] = np.nextafter(o[1::10], np.float32(np.inf))
    r[2::10] = np.nextafter(o[2::10], np.float32(-np.inf))
    y = (rng.random(E) < 0.5).astype(np.float32)
    return o, r, y


@pytest.mark.parametrize("which", range(7))
def test_kernel_against_the_fp64_closed_form(lib, sym, which):
    E = _sizes(lib)[which]
    o, r, y = _case(E, 40 + which)
    do, dr, dy = (torch.from_numpy(a).to(sym.dev) for a in (o, r, y))
    plain = _Runner(lib, sym.dev)
    tiny, eps = float(np.finfo(np.float32).tiny), 2.0 ** -24
    for alpha in (0.0, 0.1, 1.0):
        loss, parts, go, gr, counts = sym(do, dr, dy, alpha)
        wl, wparts, wgo, wgr, bo, br = sym_closed_form(o, r, y, np.float64(np.float32(PW)), np.float64(np.float32(alpha)))
        gl, gp = float(loss.item()), parts.cpu().double().numpy()
        print(f"E={E} alpha={alpha} loss={gl!r} want={wl!r} parts={gp.tolist()} want={wparts.tolist()} counts={counts.tolist()}")
        assert np.isfinite(gl) and abs(gl - wl) <= 1e-6 * abs(wl) + 1e-37
        assert np.all(np.abs(gp - wparts) <= 1e-6 * np.abs(wparts) + 1e-37)
        term = (np.sign(o.astype(np.float64) - r) != 0) & (alpha > 0)
        for name, got, want, b in (("g_org", go, wgo, bo), ("g_rev", gr, wgr, br)):
            got = got.cpu().double().numpy()
            lim = 1e-6 * np.abs(b) + max(PW, 1.0) * tiny + term * 2 * eps * (np.abs(b) + alpha / E)
            err = np.abs(got - want)
            i = int(np.argmax(err / lim))
            assert np.all(np.isfinite(got)) and not (err > lim).any(), (name, alpha, int((err > lim).sum()), o[i], r[i], y[i], got[i], want[i])
            if alpha:       # sgn(0) = 0: the tied pairs carry the plain gradient, bit for bit
                assert np.array_equal(got[0::10], (go0 if name == "g_org" else gr0)[0::10])
        assert tuple(counts.tolist()) == torch_counts(torch.from_numpy(o), torch.from_numpy(y))
        if alpha == 0.0:
            # the two BCE halves are the plain kernel's, bit for bit
            lo, g_o = plain.plain(do, dy, PW)
            lr, g_r = plain.plain(dr, dy, PW)
            assert torch.equal(_bits(go), _bits(g_o)) and torch.equal(_bits(gr), _bits(g_r))
            assert torch.equal(_bits(parts[0:1]), _bits(lo)) and torch.equal(_bits(parts[1:2]), _bits(lr))
            go0, gr0 = go.cpu().double().numpy(), gr.cpu().double().numpy()
        # bit-reproducible
        l2, p2, go2, gr2, c2 = sym(do, dr, dy, alpha)
        assert torch.equal(_bits(l2), _bits(loss)) and torch.equal(_bits(p2), _bits(parts)) and torch.equal(c2, counts)
        assert torch.equal(_bits(go2), _bits(go)) and torch.equal(_bits(gr2), _bits(gr))
        # inputs and outputs 4 bytes off a 16-byte boundary (element-by-element route): the same bits
        if E > 1:
            sh = [torch.empty(E + 1, device=sym.dev)[1:].copy_(t) for t in (do, dr, dy)]
            assert all(t.data_ptr() % 16 == 4 for t in sh)
            l3, p3, go3, gr3, c3 = sym(*sh, alpha)
            assert torch.equal(_bits(l3), _bits(loss)) and torch.equal(_bits(p3), _bits(parts)) and torch.equal(c3, counts)
            assert torch.equal(_bits(go3), _bits(go)) and torch.equal(_bits(gr3), _bits(gr))
        # no gradient asked for (both gradient pointers NULL): same loss, parts and counts.  That nothing is stored per edge is
        # checked as tests/test_gpu_loss_counts.py checks it: where the allocator hands the memory of a just-freed buffer of the
        # gradients' size out again, that memory still holds what it held
        freed = [torch.full((E,), -3.0, device=sym.dev) for _ in range(2)]
        where = [t.data_ptr() for t in freed]
        torch.cuda.synchronize()
        del freed
        l4, p4, go4, gr4, c4 = sym(do, dr, dy, alpha, grad=False)
        again = [torch.empty(E, device=sym.dev) for _ in range(2)]
        assert go4 is None and gr4 is None and torch.equal(_bits(l4), _bits(loss)) and torch.equal(_bits(p4), _bits(parts))
        assert torch.equal(c4, counts)
        for t in again:
            if t.data_ptr() in where:
                assert bool((t == -3.0).all())


@pytest.mark.parametrize("which", [0, 3, 6])
def test_epoch_accumulator_adds_three_calls_in_order(lib, sym, which):
    from gnnome_assembly_amd.train import EpochStats
    E = _sizes(lib)[which]
    acc = EpochStats(sym.dev)
    losses, sums = [], [0, 0, 0, 0]
    for k in range(3):
        o, r, y = _case(E + k * (E > 1), 7 * which + k)
        l, _, _, _, c = sym(*(torch.from_numpy(a).to(sym.dev) for a in (o, r, y)), 0.1, grad=(k != 1), acc=acc.buf)
        want = torch_counts(torch.from_numpy(o), torch.from_numpy(y))
        assert tuple(c.tolist()) == want
        losses.append(l.cpu())
        sums = [a + b for a, b in zip(sums, want)]
    want = torch.zeros((), dtype=torch.float64)
    for l in losses:                         # the fp64 sum of the fp32 losses, in call order
        want = want + l[0].double()
    loss_sum, steps, counts = acc.read()
    assert steps == 3 and counts == tuple(sums) and loss_sum == want.item()


def test_error_cases_return_before_any_launch(lib, sym):
    E = 300
    o, r, y = (torch.from_numpy(a).to(sym.dev) for a in _case(E, 1))
    fresh = lambda: (torch.full((1,), -1.0, device=sym.dev), torch.full((3,), -1.0, device=sym.dev),      # noqa: E731
                     torch.full((E,), -1.0, device=sym.dev), torch.full((E,), -1.0, device=sym.dev),
                     torch.full((4,), -1, dtype=torch.int64, device=sym.dev))
    loss, parts, go, gr, counts = fresh()
    sym.ws.fill_(0xFF)
    nan, inf = float("nan"), float("inf")
    cases = {
        "E = 0": (0, o, r, y, PW, 0.1, loss, parts, go, gr, counts, None),
        "E < 0": (-5, o, r, y, PW, 0.1, loss, parts, go, gr, counts, None),
        "org NULL": (E, None, r, y, PW, 0.1, loss, parts, go, gr, counts, None),
        "rev NULL": (E, o, None, y, PW, 0.1, loss, parts, go, gr, counts, None),
        "y NULL": (E, o, r, None, PW, 0.1, loss, parts, go, gr, counts, None),
        "loss NULL": (E, o, r, y, PW, 0.1, None, parts, go, gr, counts, None),
        "parts NULL": (E, o, r, y, PW, 0.1, loss, None, go, gr, counts, None),
        "g_rev alone NULL": (E, o, r, y, PW, 0.1, loss, parts, go, None, counts, None),
        "g_org alone NULL": (E, o, r, y, PW, 0.1, loss, parts, None, gr, counts, None),
        "alpha < 0": (E, o, r, y, PW, -0.1, loss, parts, go, gr, counts, None),
        "alpha nan": (E, o, r, y, PW, nan, loss, parts, go, gr, counts, None),
        "alpha inf": (E, o, r, y, PW, inf, loss, parts, go, gr, counts, None),
    }
    for what, args in cases.items():
        assert sym.raw(*args) != 0, what
        assert lib.gnm_last_error(), what
    assert sym.raw(E, o, r, y, PW, 0.1, loss, parts, go, gr, counts, None, ws_bytes=sym.ws.numel() - 1) != 0
    torch.cuda.synchronize()
    assert bool((loss == -1).all() and (parts == -1).all() and (go == -1).all() and (gr == -1).all() and (counts == -1).all())
    assert bool((sym.ws == 0xFF).all())
    assert sym.raw(E, o, r, y, PW, 0.1, loss, parts, go, gr, None, None) == 0          # counts_out may be NULL
    torch.cuda.synchronize()
    assert float(loss.item()) > 0


def test_module_surface(lib):
    """SymmetryLoss: forward and with_counts give the same bits and gradients, last_parts, nothing per edge without grad."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd.train import EpochStats
    o, r, y = (torch.from_numpy(a).to(DEV) for a in _case(1000, 3))
    crit = G.SymmetryLoss(PW, 0.1)
    assert crit.to(DEV) is crit and crit.float() is crit and torch.nn.ModuleDict({"crit": crit}).to(DEV)["crit"] is crit
    a, b = o.clone().requires_grad_(True), r.clone().requires_grad_(True)
    c, d = o.clone().requires_grad_(True), r.clone().requires_grad_(True)
    acc = EpochStats(torch.device(DEV))
    la = crit(a, b, y)
    parts = crit.last_parts.clone()
    lb, counts = crit.with_counts(c, d, y, acc)
    (la * 3).backward()
    (lb * 3).backward()
    assert la.shape == () and torch.equal(la, lb) and torch.equal(a.grad, c.grad) and torch.equal(b.grad, d.grad)
    assert torch.equal(crit.last_parts, parts) and parts.shape == (3,) and not parts.requires_grad
    wl, wparts, wgo, wgr, _, _ = sym_closed_form(o.cpu().numpy(), r.cpu().numpy(), y.cpu().numpy(), np.float32(PW), np.float32(0.1))
    assert abs(la.item() - wl) <= 1e-6 * wl and rel_l2(a.grad.cpu().numpy() / 3, wgo) <= 1e-6 and rel_l2(b.grad.cpu().numpy() / 3, wgr) <= 1e-6
    assert tuple(counts.tolist()) == torch_counts(o.cpu(), y.cpu()) and not counts.requires_grad
    with torch.no_grad():
        ln, cn = crit.with_counts(c, d, y, acc)
    assert not ln.requires_grad and torch.equal(ln, la.detach()) and torch.equal(cn, counts)
    assert acc.read()[1] == 2
    l5, c5, go, gr = crit.gradients(o, r, y)
    assert torch.equal(l5, la.detach()) and torch.equal(go * 3, a.grad) and torch.equal(gr * 3, b.grad)
    with pytest.raises(ValueError):
        G.SymmetryLoss(PW, -1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the reversed pass and the gradients of the whole loss
# ---------------------------------------------------------------------------------------------------------------------

def _model(H, L, bn, seed=SEED):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    sd = synth.synth_state_dict(H, L, seed)
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, bn, 16)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model.to(DEV)


_INPUTS = {}


def _inputs(which):
    if which not in _INPUTS:
        import gnnome_assembly_amd as G
        src, dst, n, e_raw, pe, y, pw = load_graph(which)
        _INPUTS[which] = (G.AssemblyGraph(src, dst, n).to(DEV), G.AssemblyGraph(dst, src, n).to(DEV), torch.from_numpy(e_raw).to(DEV),
                          torch.from_numpy(pe).to(DEV), torch.from_numpy(y).to(DEV))
    return _INPUTS[which]


@pytest.mark.parametrize("which", list(GRAPHS))
@pytest.mark.parametrize("H,L,bn", CONFIGS + [(48, 2, True)])
def test_reversed_pass_matches_the_oracle_on_the_reversed_graph(lib, which, H, L, bn):
    src, dst, n, e_raw, pe_np, y, pw = load_graph(which)
    g, g_rev, e, pe, _ = _inputs(which)
    model = _model(H, L, bn)
    want = oracle_scores(state_dict64(H, L, SEED), src, dst, n, e_raw, pe_np, bn, reverse=True).numpy()
    with torch.no_grad():
        plain = model(g, None, e, pe)
        assert torch.equal(model(g, None, e, pe, reverse=False), plain)
        got = model(g, None, e, pe, reverse=True)
        real = model(g_rev, None, e, swap_degree_columns(pe).contiguous())       # a really reversed AssemblyGraph: summation order only
    assert got.shape == plain.shape == (src.size, 1)
    print(f"{which} H={H} L={L} bn={bn}: reverse=True rel-L2 {rel_l2(got.cpu().numpy().reshape(-1), want):.2e}, "
          f"reversed graph {rel_l2(real.cpu().numpy().reshape(-1), want):.2e}, plain vs reversed "
          f"{rel_l2(plain.cpu().numpy().reshape(-1), want):.2e}")
    assert_parity(got.cpu().numpy().reshape(-1), want, "reverse=True vs the fp64 oracle on the reversed graph")
    assert_parity(real.cpu().numpy().reshape(-1), want, "engine on AssemblyGraph(dst, src) vs the fp64 oracle")
    assert rel_l2(plain.cpu().numpy().reshape(-1), want) > 1e-3       # the reversed scores are other scores


def _want_grads(which, H, L, bn, alpha):
    src, dst, n, e_raw, pe, y, pw = load_graph(which)
    sd = state_dict64(H, L, SEED, requires_grad=True)
    loss, parts, org, rev = oracle_sym_loss(sd, src, dst, n, e_raw, pe, y, pw, alpha, bn)
    loss.backward()
    return float(loss.detach()), parts.detach().numpy(), {k: v.grad.numpy() for k, v in sd.items()}


def _grad_rows(got, want, exact=None):
    """The tensors of `got` outside the bar, and every row (name, rel-L2, max-abs).  The bar of the gradient parity test: rel-L2 <=
    GRAD_L2 against the fp64 oracle; failing that (`exact`: a callable returning the fp64 gradients on the device's own relu / sign
    branches, evaluated only when needed) rel-L2 <= BRANCH_L2 against those -- a decision that fell the other way in fp32 moves a
    tensor by ~1e-3 in any fp32 evaluation, the unchanged plain-loss path included -- or, last, max-abs under the absolute floor."""
    gmax = max(float(np.linalg.norm(w)) for w in want.values())
    floor = max(GRAD_ABS_FLOOR, 1e-6 * gmax)
    rows = [(k, rel_l2(got[k], want[k]), float(np.abs(np.asarray(got[k], dtype=np.float64) - want[k]).max())) for k in want]
    bad = [r for r in rows if r[1] > GRAD_L2 and r[2] > floor]
    if bad and exact is not None:
        ex = exact()
        print("outside the plain bar:", [(k, f"{r:.2e}") for k, r, _ in bad], "-> on the device's branches:",
              [(k, f"{rel_l2(got[k], ex[k]):.2e}") for k, _, _ in bad])
        bad = [(k, rel_l2(got[k], ex[k]), float(np.abs(got[k] - ex[k]).max())) for k, _, _ in bad]
        bad = [r for r in bad if r[1] > BRANCH_L2 and r[2] > floor]
    return bad, rows


_EXACT = {}


def _exact(which, H, L, bn, alpha):
    """The branch-exact fp64 gradients of a case, computed at most once."""
    def get():
        key = (which, H, L, bn, alpha)
        if key not in _EXACT:
            _EXACT[key] = branch_exact_sym_grads(which, H, L, bn, SEED, alpha, torch.device(DEV))
        return _EXACT[key]
    return get


def _step(model, which, alpha, route, schedule="joint"):
    """One forward / backward of the symmetry loss; route: 'flat' (direct-write FlatGradients, reversed forward first), 'flat_org_first'
    (the other forward order), 'autograd' (no flat gradient buffer).  Returns (loss, parts, org, {name: gradient})."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import engine
    crit = G.SymmetryLoss(load_graph(which)[6], alpha)
    folds, fold = [], engine.mirror_add
    engine.mirror_add = lambda *a, **k: (folds.append(1), fold(*a, **k))[1]
    try:
        return _step_counted(model, which, alpha, route, schedule, crit, folds)
    finally:
        engine.mirror_add = fold


def _step_counted(model, which, alpha, route, schedule, crit, folds):
    from gnnome_assembly_amd import dp, layers, models, train as T
    g, _, e, pe, y = _inputs(which)
    fg = None
    if route != "autograd":
        models.flatten_parameters(model)
        fg = dp.FlatGradients(model.parameters(), direct_write=True)
        fg.zero_()
    else:
        for p in model.parameters():
            p.grad = None
    if route == "flat_org_first":
        org = model(g, None, e, pe).squeeze(-1)
        rev = model(g, None, e, pe, reverse=True).squeeze(-1)
        loss = crit(org, rev, y)
        loss.backward()
        loss, org = loss.detach(), org.detach()
    else:
        loss, org = T.symmetry_step(model, crit, g, None, e, pe, y, schedule)
    H = model.linear_pe.out_features
    if fg is not None and layers.padded_width(H) == H:
        # the reversed pass took the one-launch fold (its fallback through mirror_state would give the same gradients), and the
        # buffer is marked as holding a gradient
        assert len(folds) == 1 and not fg.fresh
    else:       # no flat gradient buffer, or a zero-padded width (mirror, then pad, through autograd; the flag is left alone)
        assert not folds
    torch.cuda.synchronize()
    return float(loss), crit.last_parts.cpu().double().numpy(), org, {k: p.grad.detach().cpu().double().numpy().copy() for k, p in model.named_parameters()}


@pytest.mark.parametrize("which,H,L,bn", [("small", 64, 1, True), ("small", 128, 2, True), ("small", 32, 2, False), ("tiny", 64, 1, True),
                                          ("small", 48, 2, True)])
def test_gradients_of_the_whole_loss_on_every_route(lib, which, H, L, bn):
    alpha = 0.1
    wl, wparts, want = _want_grads(which, H, L, bn, alpha)
    out = {}
    for route in ("flat", "flat_org_first", "flat_sequential", "autograd"):
        loss, parts, org, got = _step(_model(H, L, bn), which, alpha, route.replace("_sequential", ""),
                                      "sequential" if route == "flat_sequential" else "joint")
        bad, rows = _grad_rows(got, want, _exact(which, H, L, bn, alpha))
        print(f"{which} H={H} L={L} bn={bn} {route}: loss {loss!r} (fp64 {wl!r}) parts {parts.tolist()} (fp64 {wparts.tolist()}) "
              f"worst rel-L2 {max(r[1] for r in rows):.2e}")
        assert abs(loss - wl) <= 1e-5 * max(1.0, abs(wl))
        assert not bad, (route, bad)
        out[route] = got
    for route in ("flat_org_first", "flat_sequential", "autograd"):
        bad, _ = _grad_rows(out[route], out["flat"])
        assert not bad, ("flat vs " + route, bad)


@pytest.mark.parametrize("variant", ["plain", "checkpoint", "lean"])
def test_sequential_schedule_checkpointing_and_lean_activations(lib, variant):
    from gnnome_assembly_amd import engine
    which, H, L, bn, alpha = "small", 64, 2, True, 0.1
    wl, _, want = _want_grads(which, H, L, bn, alpha)
    g, _, e, pe, y = _inputs(which)
    opts = dict(ACTIVATIONS="lean") if variant == "lean" else {}
    runs = {}
    with engine.options(**opts):
        for schedule in ("joint", "sequential"):
            model = _model(H, L, bn)
            if variant == "checkpoint":
                model.activation_checkpoint = 1
            runs[schedule] = _step(model, which, alpha, "flat", schedule)
        # what the sequential schedule relies on: the forward with grad gives the bits of the forward under no_grad
        with torch.no_grad():
            a = model(g, None, e, pe)
        b = model(g, None, e, pe)
        assert torch.equal(a, b.detach()) and torch.equal(runs["sequential"][2], a.squeeze(-1))
    (lj, pj, oj, gj), (ls, ps, os_, gs) = runs["joint"], runs["sequential"]
    assert lj == ls and np.array_equal(pj, ps) and torch.equal(oj, os_)
    bad, rows = _grad_rows(gj, want, _exact(which, H, L, bn, alpha))
    assert abs(lj - wl) <= 1e-5 * max(1.0, abs(wl)) and not bad, (variant, bad)
    for k in gj:       # one reordered fp32 add per element
        assert np.abs(gs[k] - gj[k]).max() <= 1e-6 * np.abs(gj[k]).max(), (variant, k)


def test_dropout_draws_one_more_step_for_the_reversed_forward(lib):
    from gnnome_assembly_amd import engine
    import gnnome_assembly_amd as G
    g, _, e, pe, y = _inputs("small")
    model = G.GraphGatedGCNModel(1, 2, 64, 16, 2, 64, True, 16, dropout=0.2).to(DEV)
    model.train()
    engine.dropout_seed(5)
    a = model(g, None, e, pe, reverse=True)
    first = model.last_dropout
    b = model(g, None, e, pe, reverse=True)
    assert model.last_dropout[2] == first[2] + 1 and not torch.equal(a, b)
    (a.sum() + b.sum()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


# ---------------------------------------------------------------------------------------------------------------------
# train.train
# ---------------------------------------------------------------------------------------------------------------------

def _sample(which):
    from gnnome_assembly_amd.train import GraphSample
    g, _, e, pe, y = _inputs(which)
    return GraphSample(g, e, pe, y)


HP = dict(num_epochs=3, dim_latent=64, num_gnn_layers=1, lr=1e-3, seed=0, symmetry_loss=True, alpha=0.1, fused_metrics=False,
          ranking_metrics=False)          # pinned: the environment's GNM_FUSED_METRICS / GNM_RANKING_METRICS must not pick the route


def test_train_loss_sequence_matches_the_fp64_oracle(lib, tmp_path, monkeypatch):
    """Three full-graph Adam steps (three epochs of one graph) with the symmetry loss against the fp64 oracle under torch's fp64
    Adam -- whose first step is oracle.adam_step -- at the bound of test_three_adam_steps_match_reference (5e-5 x max(1, |ref|))."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import train as T
    from oracle import gatedgcn_oracle as orc
    src, dst, n, e_raw, pe, y, _ = load_graph("small")
    s = _sample("small")
    steps = []
    orig = G.SymmetryLoss.forward
    monkeypatch.setattr(G.SymmetryLoss, "forward", lambda self, *a: (orig(self, *a), steps.append(self.last_parts.clone()))[0])
    model, best, hist = T.train([s], [s], out="sym", hyperparameters=HP, workdir=str(tmp_path), verbose=False)
    pw = 1.0 / T.pos_to_neg_ratio([s])
    torch.manual_seed(HP["seed"])
    m0 = G.GraphGatedGCNModel(1, 2, 64, 16, 1, 64, True, 16)
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in m0.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=HP["lr"])
    ref, ref_valid = [], []
    for it in range(3):
        opt.zero_grad()
        loss = oracle_sym_loss(params, src, dst, n, e_raw, pe, y, pw, HP["alpha"], True)[0]
        loss.backward()
        if it == 0:
            first = orc.adam_step({k: v.detach() for k, v in params.items()}, {k: v.grad for k, v in params.items()}, lr=HP["lr"])
        opt.step()
        if it == 0:
            assert all(torch.allclose(first[k], params[k].detach(), rtol=0, atol=1e-12) for k in params)
        ref.append(float(loss.detach()))
        with torch.no_grad():
            ref_valid.append(float(oracle_sym_loss(params, src, dst, n, e_raw, pe, y, pw, HP["alpha"], True)[0]))
    print("step losses", hist.step_losses, "fp64", ref, "valid", hist.loss_valid, "fp64", ref_valid, "gap", hist.sym_gap_train)
    bound = 5e-5 * max(1.0, np.abs(ref).max())
    assert len(hist.step_losses) == 3 and np.abs(np.array(hist.step_losses) - ref).max() <= bound
    assert np.abs(np.array(hist.loss_valid) - ref_valid).max() <= bound
    # every epoch is one training step and one validation pass: forward ran twice per epoch, in that order
    assert len(steps) == 6 and len(hist.sym_gap_train) == len(hist.sym_gap_valid) == 3
    for ep in range(3):
        assert np.isfinite(hist.sym_gap_train[ep]) and hist.sym_gap_train[ep] == float(steps[2 * ep][2].double())
        assert hist.sym_gap_valid[ep] == float(steps[2 * ep + 1][2].double())
    assert hist.sym_gap_train[0] > 0 and sum(hist.tfpn_train[0]) == src.size


@pytest.mark.parametrize("mode", ["full_graph", "mini_batch"])
@pytest.mark.parametrize("schedule", ["joint", "sequential"])
def test_train_same_history_with_fused_metrics_on_and_off(lib, tmp_path, mode, schedule):
    from gnnome_assembly_amd import train as T
    hp = dict(HP, num_epochs=2, num_gnn_layers=2, symmetry_schedule=schedule)
    if mode == "mini_batch":
        hp.update(batch_size_train=2, batch_size_eval=2, num_parts_metis_train=8, num_parts_metis_eval=8)
    runs = []
    for fused in (False, True):
        s = _samples(torch.device(DEV))          # the two synthetic graphs of the plain loss's fused-metrics test
        model, best, hist = T.train(s, s[::-1], out=mode, hyperparameters=dict(hp, fused_metrics=fused),
                                    workdir=str(tmp_path / str(fused)), verbose=False)
        runs.append((hist, {k: v.detach().cpu() for k, v in model.state_dict().items()}))
    (h0, s0), (h1, s1) = runs
    print(mode, schedule, "loss_train", h0.loss_train, "loss_valid", h0.loss_valid, "gap", h0.sym_gap_train, h0.sym_gap_valid)
    assert len(h0.loss_train) == 2 and (mode == "mini_batch" or len(h0.step_losses) == 4)
    for f in ("step_losses", "loss_train", "loss_valid", "tfpn_train", "tfpn_valid", "lr", "best_epoch", "sym_gap_train", "sym_gap_valid"):
        assert getattr(h0, f) == getattr(h1, f), f
    assert len(h0.sym_gap_train) == 2 and all(np.isfinite(h0.sym_gap_train + h0.sym_gap_valid + h0.loss_valid))
    assert sum(h0.tfpn_train[0]) > 0 and sum(h0.tfpn_valid[0]) > 0
    assert set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)


def test_symmetry_loss_off_leaves_the_history_fields_empty(lib, tmp_path):
    from gnnome_assembly_amd import train as T
    s = [_sample("small")]
    hp = dict(HP, num_epochs=1, symmetry_loss=False)
    _, _, hist = T.train(s, s, out="off", hyperparameters=hp, workdir=str(tmp_path), verbose=False)
    assert hist.sym_gap_train == [] and hist.sym_gap_valid == [] and len(hist.loss_train) == 1
    with pytest.raises(ValueError, match="sequential"):
        T.train(s, s, out="bad", hyperparameters=dict(HP, symmetry_schedule="sequential", dropout=0.1), workdir=str(tmp_path), verbose=False)
