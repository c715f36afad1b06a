"""GPU: gnm_rank_hist against the numpy oracle (tests/ranking_reference.py).  The record is made of integers, so every case
asserts that the device record EQUALS hist_of's, bin for bin -- no tolerance anywhere in this file except the fp64 figures of
RankingStats.read(), which are compared for equality with the oracle's as well (same integers in, same expressions).

Sizes: 0 and 1; one below / at / above a wave (64); one below / at / above half a tile (2048: the float4 path's ragged end
falls inside a tile of 4096); 100 003: several workgroups, a ragged tail, and an odd base address for the second half of a
split.  The grid has at most one workgroup per CU, so the occupancy cap cannot change it on a full-size device; the
grid-independence test therefore also compares against sizes whose grids differ (1 tile .. 25 tiles)."""
import numpy as np
import pytest
import torch

import ranking_reference as R

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 100_003]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _case(E, seed=0, odd_labels=False):
    rng = np.random.default_rng(seed)
    x = (4.0 * rng.standard_normal(E)).astype(np.float32)
    y = (rng.random(E) < 0.2).astype(np.float32)
    if odd_labels and E >= 8:
        idx = rng.permutation(E)[:max(2, E // 50)]
        y[idx[0::2]] = 0.5
        y[idx[1::2]] = 2.0
    return x, y


def _specials():
    """+-0, +-inf, NaN, denormals, +-FLT_MAX, powers of two with both nextafter neighbours: 12 + 9 * 6 values."""
    fmax = np.finfo(np.float32).max
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, fmax, -fmax]
    v += list(np.array([1, 0x007FFFFF, 0x80000001, 0x807FFFFF], np.uint32).view(np.float32))
    for e in (-126, -20, -1, 0, 1, 2, 3, 64, 127):
        p = np.float32(2.0) ** np.float32(e)
        for s in (p, -p):
            with np.errstate(over="ignore"):
                v += [s, np.nextafter(s, np.float32(np.inf)), np.nextafter(s, np.float32(-np.inf))]
    return np.array(v, np.float32)


def _device_record(x, y, rec=None, dev="cuda:0"):
    """The record after one engine.rank_hist call on (x, y) (numpy or tensors), as a numpy int64 array."""
    from gnnome_assembly_amd import engine
    from gnnome_assembly_amd.train import RankingStats
    st = RankingStats(dev)
    if rec is not None:
        st.buf.copy_(torch.from_numpy(rec))
    xt = torch.from_numpy(x).to(dev) if isinstance(x, np.ndarray) else x
    yt = torch.from_numpy(y).to(dev) if isinstance(y, np.ndarray) else y
    engine.rank_hist(xt, yt, st.buf)
    torch.cuda.synchronize()
    return st.buf.cpu().numpy()


@pytest.mark.parametrize("E", SIZES)
def test_record_equals_the_oracle_at_every_size(lib, E):
    x, y = _case(E, seed=E, odd_labels=(E == SIZES[-1]))
    got, want = _device_record(x, y), R.record_of(x, y)
    assert int(want[:-1].sum()) == E and np.array_equal(got, want)
    if E == SIZES[-1]:
        assert want[2 * R.BINS + 2] == max(2, E // 50)                   # the 0.5 and 2.0 labels: other_label alone


def test_special_values_under_both_labels(lib):
    E = 2049
    x, y = _case(E, seed=7)
    sp = _specials()
    pos = np.random.default_rng(8).permutation(E)[:2 * sp.size]
    x[pos[:sp.size]], y[pos[:sp.size]] = sp, 1.0
    x[pos[sp.size:]], y[pos[sp.size:]] = sp, 0.0
    got, want = _device_record(x, y), R.record_of(x, y)
    assert want[2 * R.BINS] == 2 and want[2 * R.BINS + 1] == 2           # NaN and -NaN under each label
    assert np.array_equal(got, want)
    h = got[:2 * R.BINS].reshape(2, R.BINS)
    assert h[:, 31].tolist() == [1, 1] and h[:, 16352].tolist() == [1, 1] and (h[:, :31] == 0).all() and (h[:, 16353:] == 0).all()


@pytest.mark.parametrize("labels", ["all_one", "all_zero", "mixed"])
def test_one_hot_bin(lib, labels):
    E = 100_003
    x = np.full(E, 1.25, np.float32)
    y = {"all_one": np.ones(E, np.float32), "all_zero": np.zeros(E, np.float32), "mixed": _case(E, seed=3)[1]}[labels]
    got, want = _device_record(x, y), R.record_of(x, y)
    assert np.array_equal(got, want)
    k = int(R.key_of(np.float32(1.25)))
    assert got[k] + got[R.BINS + k] == E and np.count_nonzero(got[:2 * R.BINS]) == (2 if labels == "mixed" else 1)


def test_records_add(lib):
    E = 100_003
    x, y = _case(E, seed=11, odd_labels=True)
    whole = _device_record(x, y)
    h = 50_001                                                           # an odd split: the second half starts 4 bytes off 16-byte alignment
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    first = _device_record(xt[:h], yt[:h])
    both = _device_record(xt[h:], yt[h:], rec=first)
    assert both[-1] == 2 and whole[-1] == 1 and np.array_equal(both[:-1], whole[:-1])
    base = np.arange(2 * R.BINS + 4, dtype=np.int64) * 3 + 1              # a call into a non-zero record adds to it
    assert np.array_equal(_device_record(x, y, rec=base), base + R.record_of(x, y))


def test_record_does_not_depend_on_the_grid(lib):
    E = 100_003
    x, y = _case(E, seed=13)
    want = R.record_of(x, y)
    a = _device_record(x, y)
    assert lib.gnm_set_occupancy_cap(1) == 0
    try:
        b = _device_record(x, y)
    finally:
        assert lib.gnm_set_occupancy_cap(0) == 0
    assert np.array_equal(a, b) and np.array_equal(a, want)
    # grids of 8, 16 and 32 workgroups (1, 9 and 25 tiles of 4096) on prefixes: each equals the oracle, i.e. the same function
    for n in (4096, 9 * 4096, E):
        assert np.array_equal(_device_record(x[:n], y[:n]), R.record_of(x[:n], y[:n]))


def test_input_forms(lib):
    from gnnome_assembly_amd import engine
    from gnnome_assembly_amd._lib import GnmError
    from gnnome_assembly_amd.train import RankingStats
    E = 2049
    x, y = _case(E, seed=17)
    want = R.record_of(x, y)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    wide = torch.stack([xt, xt + 1.0], dim=1)
    assert not wide[:, 0].is_contiguous()
    assert np.array_equal(_device_record(wide[:, 0], yt), want)                      # non-contiguous
    assert np.array_equal(_device_record(xt.reshape(E, 1), yt), want)                # [E, 1]
    xh = xt.half()
    assert np.array_equal(_device_record(xh, yt), R.record_of(xh.float().cpu().numpy(), y))      # fp16: its fp32 copy
    st = RankingStats("cuda:0")
    with pytest.raises(GnmError):
        engine.rank_hist(torch.from_numpy(x), yt, st.buf)                            # CPU scores
    with pytest.raises(ValueError):
        engine.rank_hist(xt, yt, st.buf[:-1])
    with pytest.raises(ValueError):
        engine.rank_hist(xt, yt[:-1], st.buf)
    torch.cuda.synchronize()
    assert int(st.buf.abs().sum()) == 0


def test_ranking_stats_read(lib):
    from gnnome_assembly_amd.train import RankingStats
    from test_ranking_cpu import _check_fields
    E = 100_003
    x, y = _case(E, seed=19, odd_labels=True)
    x[:5] = np.nan
    st = RankingStats("cuda:0")
    m = st.add(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()).read()
    _check_fields(m, R.metrics_of(*R.hist_of(x, y)))
    assert m.n_pos + m.n_neg + m.n_nan + m.n_other == E and m.calls == 1
    assert 0.4 < m.auroc_lo <= m.auroc <= m.auroc_hi < 0.6 and m.auroc_hi - m.auroc_lo < 0.02      # random logits, 32 bins per octave
    xs, ys = x[:3000], y[:3000]                                           # brute force is O(P * N): a subsample through the same path
    ms = st.zero_().add(torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()).read()
    exact = R.auroc_exact(xs[(ys == 0) | (ys == 1)], ys[(ys == 0) | (ys == 1)])
    print("auroc", ms.auroc_lo, ms.auroc, ms.auroc_hi, "exact", exact)
    assert ms.auroc_lo <= exact <= ms.auroc_hi


def _samples(dev):
    """The two smallest synthetic graphs of the loss-counts train-loop test."""
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


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("mode", ["full_graph", "mini_batch"])
def test_train_loop_reports_the_oracle_figures_and_changes_nothing_else(lib, tmp_path, mode, fused):
    from dataclasses import fields
    from gnnome_assembly_amd import train as T
    dev = torch.device("cuda:0")
    hp = dict(num_epochs=2, dim_latent=128, num_gnn_layers=2, lr=1e-3, seed=0, fused_metrics=fused)
    if mode == "mini_batch":
        hp.update(batch_size_train=2, batch_size_eval=2, num_parts_metis_train=8, num_parts_metis_eval=8)
    new = ("auroc_valid", "ap_valid", "best_f1_valid")
    runs = []
    for on in (False, True):
        s = _samples(dev)
        valid = s[::-1]
        want = []

        def after_epoch(epoch, model, valid=valid, want=want):
            # full graph: recompute the epoch's validation logits (eval mode, same weights: the loop has not stepped since)
            if mode != "full_graph":
                return
            with torch.no_grad():
                px = [model(v.graph, v.x, v.e, v.pe).squeeze(-1).cpu().numpy() for v in valid]
            h, t = R.hist_of(np.concatenate(px), np.concatenate([v.y.cpu().numpy() for v in valid]))
            t[3] = len(valid)
            want.append(R.metrics_of(h, t))

        model, best, hist = T.train(s, valid, out=mode, hyperparameters=dict(hp, ranking_metrics=on),
                                    workdir=str(tmp_path / f"{on}"), verbose=False, hooks={"after_epoch": after_epoch})
        runs.append((hist, {k: v.detach().cpu() for k, v in model.state_dict().items()}))
        if not on:
            assert all(getattr(hist, f) == [] for f in new)
            continue
        assert all(len(getattr(hist, f)) == 2 for f in new)
        for ep in range(2):
            assert 0.0 <= hist.auroc_valid[ep] <= 1.0 and 0.0 < hist.ap_valid[ep] <= 1.0 and 0.0 < hist.best_f1_valid[ep][0] <= 1.0
            if mode == "full_graph":
                w = want[ep]
                print("epoch", ep, "auroc", hist.auroc_valid[ep], "ap", hist.ap_valid[ep], "best f1", hist.best_f1_valid[ep])
                assert hist.auroc_valid[ep] == w["auroc"] and hist.ap_valid[ep] == w["average_precision"]
                assert hist.best_f1_valid[ep] == (w["best_f1"]["f1"], w["best_f1"]["logit"])
    (h0, s0), (h1, s1) = runs
    for f in fields(T.History):
        if f.name not in new:
            assert getattr(h0, f.name) == getattr(h1, f.name), f.name
    assert set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)
