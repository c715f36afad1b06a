"""GPU: gnm_bce_stats_fwd_bwd -- loss and gradient bit-identical to gnm_bce_fwd_bwd, TP/TN/FP/FN equal to the torch expression
evaluated on the CPU, epoch sums added in call order -- and train.train with fused_metrics on against off.

Two notes on how the comparisons are made.  (1) The boundary logits hold +-inf and nan and the labels hold nan, so the loss of
a case is nan (inf) and its gradient has nan rows: "equal" is therefore checked on the BIT PATTERNS (stronger than torch.equal,
which calls two nans different), and every size is checked a second time on the same data with the non-finite logits and the nan
labels replaced, where the loss is finite.  The epoch sums use those finite cases: a sum with a nan in it cannot be compared
with ==.  (2) The smallest E at which the grid reaches its cap fills the cap's blocks once, and so does that E plus 3; the
second trip of the grid-stride loop with a ragged tail is the further size cap * block + 3.  The grid is read off the kernel:
the number of loss partials gnm_bce_fwd_bwd writes into a workspace of 0xFF bytes."""
import os
import re

import pytest
import torch

from loss_counts_common import REPO, make_case, torch_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _block():
    """The loss kernels' workgroup size, from the source they are compiled from."""
    src = open(os.path.join(REPO, "gnnome_assembly_amd", "csrc", "gnm_common.h")).read()
    return int(re.search(r"constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", src).group(1))


_SIZES = []


def _sizes(lib):
    """1; block - 1, block, block + 1; the smallest E at which the loss kernel's grid reaches its cap, that + 3; cap * block + 3.
    The grid of an E is measured (_Runner.grid), the smallest E found by bisection: grid(E) does not decrease with E."""
    if not _SIZES:
        r = _Runner(lib, torch.device("cuda:0"))
        block, nb = _block(), lib.gnm_max_partial_blocks()
        cap = r.grid(2 * nb * block)
        assert cap == nb, f"the grid stops at {cap} blocks, below gnm_max_partial_blocks() = {nb}, on this device"
        lo, hi = 1, nb * block                # grid(lo) < cap <= grid(hi)
        assert r.grid(lo) < cap == r.grid(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if r.grid(mid) >= cap:
                hi = mid
            else:
                lo = mid
        _SIZES.extend([1, block - 1, block, block + 1, hi, hi + 3, cap * block + 3])
    return _SIZES


def _bits(t):
    return t.view(torch.int32)


class _Runner:
    """Calls the two entry points on caller-owned buffers; the workspace is filled with 0xFF bytes (NaN doubles, -1 counts)
    before every call."""

    def __init__(self, lib, dev):
        from gnnome_assembly_amd import engine
        self.lib, self.dev, self.e = lib, dev, engine
        self.ws = torch.empty(lib.gnm_bce_stats_workspace_bytes(), dtype=torch.uint8, device=dev)

    def plain(self, x, y, pw):
        E = x.numel()
        loss = torch.full((1,), -1.0, device=self.dev)
        gs = torch.full((E,), -1.0, device=self.dev)
        self.ws.fill_(0xFF)
        p = self.e._ptr
        rc = self.lib.gnm_bce_fwd_bwd(E, p(x), p(y), pw, p(loss), p(gs), p(self.ws), self.ws.numel(), self.e._stream())
        assert rc == 0, self.lib.gnm_last_error()
        return loss, gs

    def grid(self, E):
        """Workgroups the loss kernel launches for E elements: the partials it wrote (one double per workgroup, from the front)."""
        self.plain(torch.zeros(E, device=self.dev), torch.zeros(E, device=self.dev), 1.0)
        written = self.ws[:self.lib.gnm_max_partial_blocks() * 8].view(torch.int64) != -1
        n = int(written.sum())
        assert bool(written[:n].all())
        return n

    def stats(self, x, y, pw, grad=True, acc=None):
        E = x.numel()
        loss = torch.full((1,), -1.0, device=self.dev)
        gs = torch.full((E,), -1.0, device=self.dev) if grad else None
        counts = torch.full((4,), -1, dtype=torch.int64, device=self.dev)
        self.ws.fill_(0xFF)
        p = self.e._ptr
        rc = self.lib.gnm_bce_stats_fwd_bwd(E, p(x), p(y), pw, p(loss), p(gs), p(counts), p(acc), p(self.ws), self.ws.numel(),
                                            self.e._stream())
        assert rc == 0, self.lib.gnm_last_error()
        return loss, gs, counts


@pytest.fixture(scope="module")
def runner(lib):
    return _Runner(lib, torch.device("cuda:0"))


PW = 0.25


@pytest.mark.parametrize("which", range(7))
@pytest.mark.parametrize("clean", [False, True])
def test_kernel_against_plain_loss_and_torch_counts(lib, runner, which, clean):
    E = _sizes(lib)[which]
    xc, yc = make_case(E, seed=100 + which, clean=clean)
    want = torch_counts(xc, yc)
    x, y = xc.to(runner.dev), yc.to(runner.dev)
    l0, g0 = runner.plain(x, y, PW)
    l1, g1, c1 = runner.stats(x, y, PW)
    print(f"E={E} clean={clean} loss={l1.item()!r} counts={c1.tolist()} want={want}")
    assert torch.equal(_bits(l1), _bits(l0)) and torch.equal(_bits(g1), _bits(g0))
    if clean:
        assert torch.isfinite(l1).all() and torch.equal(l1, l0) and torch.equal(g1, g0)
    assert tuple(c1.tolist()) == want
    # no gradient asked for: same loss, same counts, and no per-edge store -- neither into a live sentinel buffer nor into the
    # memory of a gradient buffer of this size that was freed just before the call (where the allocator hands it out again)
    sentinel = torch.full((E,), -3.0, device=runner.dev)
    freed = torch.full((E,), -3.0, device=runner.dev)
    where = freed.data_ptr()
    torch.cuda.synchronize()
    del freed
    l2, g2, c2 = runner.stats(x, y, PW, grad=False)
    again = torch.empty(E, device=runner.dev)
    assert g2 is None and torch.equal(_bits(l2), _bits(l0)) and torch.equal(c2, c1)
    assert bool((sentinel == -3.0).all())
    print(f"freed gradient buffer handed out again: {again.data_ptr() == where}")
    if again.data_ptr() == where:
        assert bool((again == -3.0).all())
    # bit-reproducible
    l3, g3, c3 = runner.stats(x, y, PW)
    assert torch.equal(_bits(l3), _bits(l1)) and torch.equal(_bits(g3), _bits(g1)) and torch.equal(c3, c1)


@pytest.mark.parametrize("which", [0, 3, 6])
def test_epoch_accumulator_adds_three_calls_in_order(lib, runner, which):
    from gnnome_assembly_amd.train import EpochStats
    E = _sizes(lib)[which]
    acc = EpochStats(runner.dev)
    acc.buf.fill_(123)                       # zero_() must clear whatever is there
    acc.zero_()
    assert acc.read() == (0.0, 0, (0, 0, 0, 0))
    losses, sums = [], [0, 0, 0, 0]
    for k in range(3):
        xc, yc = make_case(E + k * (E > 1), seed=7 * which + k, clean=True)
        l, _, c = runner.stats(xc.to(runner.dev), yc.to(runner.dev), PW, grad=(k != 1), acc=acc.buf)
        assert tuple(c.tolist()) == torch_counts(xc, yc)
        losses.append(l.cpu())
        sums = [a + b for a, b in zip(sums, torch_counts(xc, yc))]
    want = torch.zeros((), dtype=torch.float64)
    for l in losses:                         # the fp64 sum of the fp32 losses, in call order
        want = want + l[0].double()
    loss_sum, steps, counts = acc.read()
    print(f"E={E} loss_sum={loss_sum!r} want={want.item()!r} counts={counts}")
    assert steps == 3 and counts == tuple(sums)
    assert loss_sum == want.item()
    assert acc.loss_sum.item() == loss_sum and int(acc.steps) == 3 and tuple(acc.counts.tolist()) == counts


def test_with_counts_module_surface(lib, runner):
    """BCEWithLogitsLoss.with_counts: forward's loss and gradient bit for bit, counts as tfpn_counts', no gradient buffer under
    no_grad, the accumulator fed through the EpochStats object."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd.train import EpochStats, tfpn_counts
    xc, yc = make_case(1000, seed=3, clean=True)
    y = yc.to(runner.dev)
    crit = G.BCEWithLogitsLoss(PW)
    a = xc.to(runner.dev).requires_grad_(True)
    b = xc.to(runner.dev).requires_grad_(True)
    acc = EpochStats(runner.dev)
    la = crit(a, y)
    lb, counts = crit.with_counts(b, y, acc)
    (la * 3).backward()
    (lb * 3).backward()
    assert lb.shape == () and torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert counts.dtype == torch.int64 and counts.shape == (4,) and not counts.requires_grad
    assert tuple(counts.tolist()) == torch_counts(xc, yc) == tuple(tfpn_counts(xc, yc).tolist())
    with torch.no_grad():
        ln, cn = crit.with_counts(b, y, acc)
    assert not ln.requires_grad and torch.equal(ln, la.detach()) and torch.equal(cn, counts)
    assert acc.read() == (2 * float(la.detach().double()), 2, tuple(2 * c for c in counts.tolist()))


def _samples(dev):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    from gnnome_assembly_amd.train import GraphSample
    out = []
    for reads, seed in ((300, 11), (280, 12)):
        src, dst, n = synth.make_graph(reads, seed=seed)
        inp = synth.make_inputs(src, dst, n, seed=seed)
        out.append(GraphSample(G.AssemblyGraph(src, dst, n).to(dev), torch.from_numpy(inp["e"]).to(dev),
                               torch.from_numpy(inp["pe"]).to(dev), torch.from_numpy(inp["y"]).to(dev)))
    return out


@pytest.fixture(params=["f16x2", "bf16x3", "f32"])
def matmul_mode(request, lib):
    """The loss kernels have no matrix-core code (the tests above run once); the model of the train loop has."""
    from gnnome_assembly_amd import _lib
    _lib.set_matmul_mode(request.param)
    yield request.param
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)


@pytest.mark.parametrize("mode", ["full_graph", "mini_batch"])
def test_train_loop_same_history_fused_on_and_off(lib, tmp_path, mode, matmul_mode, monkeypatch):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import train as T
    dev = torch.device("cuda:0")
    hp = dict(num_epochs=2, dim_latent=128, num_gnn_layers=2, lr=1e-3, seed=0)
    if mode == "mini_batch":
        hp.update(batch_size_train=2, batch_size_eval=2, num_parts_metis_train=8, num_parts_metis_eval=8)
    runs = []
    for fused in (False, True):
        s = _samples(dev)
        calls = []
        if fused:          # the on run must take the fused route: the torch route's tfpn_counts raises, with_counts is counted
            def no_torch_route(*a, **k):
                raise AssertionError("tfpn_counts called with fused_metrics on")
            monkeypatch.setattr(T, "tfpn_counts", no_torch_route)
            orig = G.BCEWithLogitsLoss.with_counts
            monkeypatch.setattr(G.BCEWithLogitsLoss, "with_counts", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
        model, best, hist = T.train(s, s[::-1], out=mode, hyperparameters=dict(hp, fused_metrics=fused),
                                    workdir=str(tmp_path / str(fused)), verbose=False)
        runs.append((hist, {k: v.detach().cpu() for k, v in model.state_dict().items()}))
        assert fused == (len(calls) >= 8), len(calls)          # 2 epochs x (>= 2 training + >= 2 validation passes)
    (h0, s0), (h1, s1) = runs
    print(mode, "steps", len(h0.step_losses), "loss_train", h0.loss_train, h1.loss_train, "tfpn", h0.tfpn_train, h1.tfpn_train)
    assert len(h0.loss_train) == 2 and (mode == "mini_batch" or len(h0.step_losses) == 4)
    for f in ("step_losses", "loss_train", "loss_valid", "tfpn_train", "tfpn_valid", "lr", "best_epoch"):
        assert getattr(h0, f) == getattr(h1, f), f
    assert sum(h0.tfpn_train[0]) > 0 and sum(h0.tfpn_valid[0]) > 0
    assert set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)
