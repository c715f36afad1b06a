"""CPU: the key of the ranking histogram, train.RankingMetrics.from_counts against brute force on the raw logits, the record's
edge conditions, RankingStats.all_reduce_ under two gloo ranks, and the bindings of the two entry points.

Tolerances.  from_counts and the brute-force definitions sum integers of at most 300^2 and ratios of them in fp64: on logits
that sit on bin lower edges (where binning loses nothing) they agree to 1e-12.  On raw logits only the bracket
auroc_lo <= exact <= auroc_hi is claimed, and it is exact: both sides are ratios of integers over the same P * N."""
import ctypes as C
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ranking_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(bits):
    return np.asarray(bits, dtype=np.uint64).astype(np.uint32).view(np.float32)


# ---- key_of ---------------------------------------------------------------------------------------------------------------------
def test_key_is_monotone_on_random_bit_patterns():
    rng = np.random.default_rng(0)
    x = _f32(rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64))
    x = np.sort(x[~np.isnan(x)])
    k = R.key_of(x)
    assert x.size > 99_000 and (np.diff(k) >= 0).all()
    assert k.min() >= 0 and k.max() < R.BINS


def test_key_of_zeros_powers_of_two_infinities_and_denormals():
    assert R.key_of(np.float32(-0.0)) == R.key_of(np.float32(0.0)) == 8192
    p2 = np.float32(2.0) ** np.arange(-126, 128, dtype=np.float32)
    for s in (1.0, -1.0):
        v = (s * p2).astype(np.float32)
        inner = np.nextafter(v, np.float32(0.0))             # the neighbour nearer to zero
        kv, ki = R.key_of(v), R.key_of(inner)
        if s > 0:      # a power of two starts a bin: its lower neighbour lies in the bin below
            assert (ki == kv - 1).all() and (np.diff(kv) == 32).all()
            assert all(R.lower_edge(int(k)) == float(x) for k, x in zip(kv, v))
        else:          # mirrored: -2^e is the top of its bin (keys fall as the magnitude grows), its inner neighbour the bin above
            assert (ki == kv + 1).all() and (np.diff(kv) == -32).all()
    inf = np.float32(np.inf)
    fmax = np.finfo(np.float32).max
    assert R.key_of(-inf) == 31 and R.key_of(inf) == 16352
    assert R.key_of(-inf) < R.key_of(-fmax) and R.key_of(fmax) < R.key_of(inf)
    assert R.lower_edge(31) == -math.inf and R.lower_edge(16352) == math.inf
    den = _f32([1, 0x007FFFFF, 0x80000001, 0x807FFFFF])      # smallest / largest denormal of either sign
    assert R.key_of(den).tolist() == [8192, 8192 + 31, 8191, 8191 - 31]
    assert R.key_of(_f32([0x00800000])) == 8192 + 32         # the smallest normal starts the next exponent's bins


def test_library_lower_edge_matches_the_oracle():
    from gnnome_assembly_amd.train import rank_bin_lower_edge, RANK_BINS
    assert RANK_BINS == R.BINS
    ks = np.arange(31, 16353)
    got = rank_bin_lower_edge(ks)
    want = np.array([R.lower_edge(int(k)) for k in ks])
    assert np.array_equal(got, want)
    fin = np.isfinite(want)
    assert (R.key_of(want[fin].astype(np.float32)) == ks[fin]).all()           # an edge lies in its own bin ...
    with np.errstate(over="ignore"):                                            # -FLT_MAX steps down to -inf
        below = np.nextafter(want[fin].astype(np.float32), np.float32(-np.inf))
    assert (R.key_of(below) == ks[fin] - 1).all()                               # ... and the value below it in the bin below


# ---- from_counts against brute force --------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(5)
    x = (4.0 * rng.standard_normal(300)).astype(np.float32)
    y = (rng.random(300) < 0.2).astype(np.float32)
    ties = np.round(x).astype(np.float32)                                       # ~25 distinct values: many ties
    one_bin = np.full(300, 1.25, np.float32)
    return {"random": (x, y), "ties": (ties, y), "one_bin": (one_bin, y),
            "one_bin_spread": ((1.25 + 0.03 * rng.random(300)).astype(np.float32), y)}


def _check_fields(m, want):
    for f in ("n_pos", "n_neg", "n_nan", "n_other", "calls"):
        assert getattr(m, f) == want[f], f
    for f in ("auroc", "auroc_lo", "auroc_hi", "average_precision"):
        a, b = getattr(m, f), want[f]
        assert (math.isnan(a) and math.isnan(b)) or a == b, (f, a, b)
    if want["best_f1"] is None:
        assert m.best_f1 is None
    else:
        assert {k: getattr(m.best_f1, k) for k in want["best_f1"]} == want["best_f1"]


@pytest.mark.parametrize("name", ["random", "ties", "one_bin", "one_bin_spread"])
def test_from_counts_against_brute_force(name):
    from gnnome_assembly_amd.train import RankingMetrics
    x, y = _cases()[name]
    hist, tail = R.hist_of(x, y)
    m = RankingMetrics.from_counts(hist, tail)
    _check_fields(m, R.metrics_of(hist, tail))
    exact = R.auroc_exact(x, y)
    print(name, "auroc", m.auroc_lo, m.auroc, m.auroc_hi, "exact", exact, "ap", m.average_precision, "best", m.best_f1)
    assert m.auroc_lo <= exact <= m.auroc_hi and m.auroc_lo <= m.auroc <= m.auroc_hi
    if name == "one_bin":
        assert (m.auroc_lo, m.auroc, m.auroc_hi) == (0.0, 0.5, 1.0) and exact == 0.5
    # the same edges with every logit moved to the lower edge of its bin: binning loses nothing, so the figures are the exact ones
    q = np.array([R.lower_edge(int(k)) for k in R.key_of(x)], np.float32)
    assert np.array_equal(R.hist_of(q, y)[0], hist)
    assert abs(m.auroc - R.auroc_exact(q, y)) <= 1e-12
    assert abs(m.average_precision - R.ap_exact(q, y)) <= 1e-12
    f1, k = R.best_f1_exhaustive(x, y)
    assert m.best_f1.f1 == f1 and m.best_f1.bin == k
    b = m.best_f1
    assert (b.TP + b.FN, b.TN + b.FP) == (m.n_pos, m.n_neg) and b.logit == R.lower_edge(k)
    pred = x >= np.float32(b.logit)
    assert (int((pred & (y == 1)).sum()), int((~pred & (y == 0)).sum())) == (b.TP, b.TN)
    fpr, tpr, thr = m.roc()
    prec, rec, thr2 = m.pr()
    nocc = int(((hist[0] + hist[1]) > 0).sum())
    assert fpr.shape == tpr.shape == thr.shape == prec.shape == rec.shape == (nocc,) and np.array_equal(thr, thr2)
    assert fpr[-1] == tpr[-1] == rec[-1] == 1.0 and (np.diff(thr) < 0).all() and (np.diff(tpr) >= 0).all()
    assert abs(float(np.sum(np.diff(np.concatenate([[0.0], rec])) * prec)) - m.average_precision) <= 1e-12


def test_degenerate_records_and_tail_counters():
    from gnnome_assembly_amd.train import RankingMetrics
    x = np.array([0.5, -1.0, 2.0, np.nan, np.nan, 1.0, 3.0, np.nan], np.float32)
    y = np.array([1.0, 1.0, 1.0, 1.0, 0.0, 0.5, 2.0, np.nan], np.float32)
    hist, tail = R.hist_of(x, y)
    assert tail.tolist() == [1, 1, 3, 1]                                         # NaN logit under y = 1, under y = 0; three other labels
    assert int(hist.sum() + tail[0] + tail[1] + tail[2]) == x.size
    m = RankingMetrics.from_counts(hist, tail)                                   # three positives, no negative
    assert (m.n_pos, m.n_neg, m.n_nan, m.n_other, m.calls) == (3, 0, 2, 3, 1)
    assert math.isnan(m.auroc) and math.isnan(m.auroc_lo) and math.isnan(m.auroc_hi) and math.isnan(m.average_precision)
    _check_fields(m, R.metrics_of(hist, tail))
    hist0, tail0 = R.hist_of(x[:3], np.zeros(3, np.float32))                     # three negatives, no positive
    m0 = RankingMetrics.from_counts(hist0, tail0)
    assert (m0.n_pos, m0.n_neg) == (0, 3) and math.isnan(m0.auroc) and math.isnan(m0.average_precision)
    assert m0.best_f1.f1 == 0.0
    _check_fields(m0, R.metrics_of(hist0, tail0))
    e = RankingMetrics.from_counts(np.zeros((2, R.BINS), np.int64), np.zeros(4, np.int64))      # an empty record
    assert e.best_f1 is None and math.isnan(e.auroc) and e.roc()[0].size == 0 and e.pr()[0].size == 0
    rng = np.random.default_rng(1)
    xs = (4.0 * rng.standard_normal(5000)).astype(np.float32)
    ys = rng.choice(np.array([0.0, 1.0, 0.5, 2.0], np.float32), size=5000, p=[0.7, 0.2, 0.05, 0.05])
    xs[rng.integers(0, 5000, 40)] = np.nan
    h, t = R.hist_of(xs, ys)
    assert int(h.sum() + t[0] + t[1] + t[2]) == 5000 and t[2] == int(((ys != 0) & (ys != 1)).sum())


# ---- RankingStats on the CPU: views, zero_, read, all_reduce_ under gloo --------------------------------------------------------
def _rank_case(rank):
    rng = np.random.default_rng(100 + rank)
    x = (4.0 * rng.standard_normal(2000)).astype(np.float32)
    y = (rng.random(2000) < 0.2).astype(np.float32)
    x[:3] = np.nan
    y[5:8] = 0.5
    return x, y


def test_ranking_stats_on_the_cpu_without_a_process_group():
    from gnnome_assembly_amd.train import RankingStats
    from gnnome_assembly_amd._lib import GnmError
    st = RankingStats("cpu")
    assert st.buf.dtype == torch.int64 and st.buf.numel() == 2 * R.BINS + 4 and int(st.buf.abs().sum()) == 0
    st.buf += torch.from_numpy(R.record_of(*_rank_case(0)))
    assert st.hist.shape == (2, R.BINS) and st.hist.data_ptr() == st.buf.data_ptr() and st.tail.tolist()[3] == 1
    assert st.all_reduce_() is st                                   # no process group: a no-op
    h, t = R.hist_of(*_rank_case(0))
    _check_fields(st.read(), R.metrics_of(h, t))
    with pytest.raises(GnmError):                                   # add() is the kernel: no CPU fallback
        st.add(torch.zeros(4), torch.zeros(4))
    assert int(st.zero_().buf.abs().sum()) == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from gnnome_assembly_amd import dp
    from gnnome_assembly_amd.train import RankingStats
    r, w = dp.init_process_group("gloo")
    assert (r, w) == (rank, world)
    st = RankingStats("cpu")
    st.buf += torch.from_numpy(R.record_of(*_rank_case(rank)))
    m = st.all_reduce_().read()
    np.save(os.path.join(out_dir, f"record{rank}.npy"), st.buf.numpy())
    np.save(os.path.join(out_dir, f"auroc{rank}.npy"), np.array([m.auroc, m.average_precision]))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_sums_the_records_of_two_gloo_ranks(tmp_path):
    from gnnome_assembly_amd.train import RankingMetrics
    world = 2
    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    recs = [np.load(tmp_path / f"record{r}.npy") for r in range(world)]
    want = sum(R.record_of(*_rank_case(r)) for r in range(world))
    assert np.array_equal(recs[0], want) and np.array_equal(recs[1], want)
    # the summed record is the record of the concatenated edges (apart from `calls`, which counts both)
    xs, ys = zip(*(_rank_case(r) for r in range(world)))
    h, t = R.hist_of(np.concatenate(xs), np.concatenate(ys))
    assert np.array_equal(want[:-1], np.concatenate([h.reshape(-1), t[:3]])) and want[-1] == 2
    m = RankingMetrics.from_counts(want[:2 * R.BINS], want[2 * R.BINS:])
    assert np.array_equal(np.load(tmp_path / "auroc0.npy"), np.array([m.auroc, m.average_precision]))
    assert m.auroc_lo <= R.auroc_exact(np.concatenate(xs), np.concatenate(ys)) <= m.auroc_hi


# ---- bindings -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def test_the_library_binds_both_entry_points_at_abi_7(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib, engine
    assert "gnm_rank.hip" in ge.SOURCES
    for name in ("gnm_rank_hist_workspace_bytes", "gnm_rank_hist"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.gnm_abi_version() == 7 == _lib.ABI_VERSION
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    assert "gnm_rank_record" in hdr and "int gnm_rank_hist(" in hdr and "#define GNM_ABI_VERSION 7" in hdr
    assert engine.RANK_RECORD_WORDS == 2 * R.BINS + 4 and engine.RANK_BINS == R.BINS


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Host-side returns: no device is touched (the checks run before the grid is even sized)."""
    rec = (C.c_int64 * (2 * R.BINS + 4))()
    buf = (C.c_float * 8)()
    p = lambda a: C.c_void_p(C.addressof(a))                                     # noqa: E731
    assert lib.gnm_rank_hist_workspace_bytes(7_540_000) == lib.gnm_rank_hist_workspace_bytes(0)
    for args, word in (((-1, p(buf), p(buf), p(rec), None, 0, None), "negative"),
                       ((8, None, p(buf), p(rec), None, 0, None), "null"),
                       ((8, p(buf), None, p(rec), None, 0, None), "null"),
                       ((8, p(buf), p(buf), None, None, 0, None), "record"),
                       ((0, None, None, None, None, 0, None), "record"),
                       ((8, p(buf), p(buf), C.c_void_p(C.addressof(rec) + 4), None, 0, None), "aligned"),
                       ((1 << 50, p(buf), p(buf), p(rec), None, 0, None), "2^31")):     # a workgroup's 32-bit bins would overflow
        assert lib.gnm_rank_hist(*args) != 0
        assert word in lib.gnm_last_error().decode()
    assert all(v == 0 for v in rec)
