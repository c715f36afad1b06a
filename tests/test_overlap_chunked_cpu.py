"""CPU: the overlap graph in read-range chunks (include/gnm.h, "Stage 2 in read-range chunks") through the host entries and
find_overlaps(max_hits=...) on a CPU store: the hits per lower read and the hits of a read range against the plain restatement of
tests/overlap_chunk_reference.py, plan_chunks on hand-written counts, the chunked find_overlaps against the unchunked call on the
same store -- every tensor, every count, every record word but `calls` -- and the refusals.  Integers, and fp32 values formed
from the same two integers: every comparison is an equality."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import overlap_chunk_reference as CR
import overlap_reference as O
from test_overlap_cpu import GENOME, PAIRS, _np, _t, genome_case, run_pairs, same

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = dict(PAIRS, one=(tuple(a[:1] for a in PAIRS["runs"][0]),) + PAIRS["runs"][1:])      # M = 1 beside "empty" (M = 0)
NEW_SYMBOLS = ("gnm_seed_pairs_lower_hits", "gnm_seed_pairs_lower_hits_host", "gnm_seed_pairs_count_range",
               "gnm_seed_pairs_emit_range", "gnm_seed_pairs_range_host")
BUDGETS = ("1", "7", "total // 3", "total - 1", "total", "2 ** 40")
GRAPH_TENSORS = ("prefix_length", "overlap_length", "twin", "overlap_similarity")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def run_lower(arr, lengths, k, max_occ, dev="cpu", threads=1):
    """(lower_hits, record) of engine.seed_pairs_lower_hits."""
    from gnnome_assembly_amd import engine
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=dev)
    low = torch.zeros(len(lengths), dtype=torch.int64, device=dev)
    engine.seed_pairs_lower_hits(_t(arr[0], dev), _t(arr[1], dev), len(lengths), max_occ, low, rec, threads)
    return low.cpu().numpy(), rec.cpu().numpy()


def run_range(arr, lengths, k, max_occ, a_lo, a_hi, dev="cpu", threads=1):
    """(key, diag, record) of engine.seed_pairs_range."""
    from gnnome_assembly_amd import engine
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=dev)
    out = engine.seed_pairs_range(*[_t(a, dev) for a in arr], _t(lengths, dev), k, max_occ, a_lo, a_hi, rec, threads)
    return _np(out) + (rec.cpu().numpy(),)


def ref_lower(name):
    arr, lengths, k, occ = PAIRS[name]
    low, rec = O.cached(("lower", name), lambda: CR.lower_hits(arr, lengths, k, occ))
    return low, O.rec_array(rec)


def ref_hits(name):
    arr, lengths, k, occ = PAIRS[name]
    return O.cached(("pairs+", name), lambda: O.seed_pairs(arr, lengths, k, occ))[0]


def partitions(R):
    """Every partition of [0, R) into 1, 2 and 3 consecutive ranges, empty ranges included, and the one into R ranges."""
    out = [[0, R]] + [[0, c, R] for c in range(R + 1)] + [[0, c, d, R] for c in range(R + 1) for d in range(c, R + 1)]
    return out + [list(range(R + 1))]


def check_ranges(name, dev="cpu", threads=1):
    """Every range of every partition equals the reference filter; every partition's concatenation is the unchunked hits once
    both went through the stage's two stable sorts; [0, R) is engine.seed_pairs itself.  The record stays zero."""
    arr, lengths, k, occ = PAIRS[name]
    R, hits = len(lengths), ref_hits(name)
    zero = np.zeros(len(O.COUNTERS), np.int64)
    got = {}
    for lo, hi in itertools.combinations_with_replacement(range(R + 1), 2):
        got[lo, hi] = run_range(arr, lengths, k, occ, lo, hi, dev, threads)
        same(got[lo, hi], CR.range_hits(hits, lo, hi) + (zero,), (name, lo, hi))
    whole = run_pairs(arr, lengths, k, occ, dev)
    same(got[0, R][:2], whole[:2], name + ": [0, R) against seed_pairs")
    want = O.sort_hits(whole[:2])
    for b in partitions(R):
        parts = [got[lo, hi] for lo, hi in zip(b[:-1], b[1:])]
        cat = tuple(np.concatenate([p[j] for p in parts]) for j in range(2))
        same(O.sort_hits(cat), want, (name, b))
    return got


@pytest.mark.parametrize("name", list(PAIRS))
def test_lower_hits_equal_the_reference(lib, name):
    want = ref_lower(name)
    same(run_lower(*PAIRS[name]), want, name)
    same(run_lower(*PAIRS[name], threads=3), want, name + " (3 threads)")
    assert want[0].sum() == want[1][O.COUNTERS.index("hits")]


def test_lower_hits_cases_cover_what_they_claim(lib):
    low, rec = run_lower(*PAIRS["runs"])
    r = dict(zip(O.COUNTERS, rec.tolist()))
    assert r["skipped_runs"] == 1 and r["same_read"] == 4 and r["hits"] == 17 == low.sum()     # as test_pair_cases_cover_what_they_claim
    assert low[6] == 0 and low[7] == 0 and low[11] == 0 and low[0] == 4 and low[2] == 2 + 4    # read 2 twice in a run: 2 hits each
    assert [len(PAIRS[n][0][0]) for n in ("empty", "one")] == [0, 1]
    low1, rec1 = run_lower(*PAIRS["one"])
    assert not low1.any() and rec1[O.COUNTERS.index("runs")] == 1
    assert not run_lower(*PAIRS["occ1"])[0].any()
    # lower_hits ADDS: a second call doubles both
    from gnnome_assembly_amd import engine
    arr, lengths, k, occ = PAIRS["runs"]
    rec2, low2 = torch.from_numpy(rec.copy()), torch.from_numpy(low.copy())
    engine.seed_pairs_lower_hits(_t(arr[0], "cpu"), _t(arr[1], "cpu"), len(lengths), occ, low2, rec2)
    assert np.array_equal(low2.numpy(), 2 * low) and np.array_equal(rec2.numpy(), 2 * rec)


def test_lower_hits_need_no_order_inside_a_run(lib):
    """The count is made entry by entry, so a run whose reads do not ascend (no sketch gives one) is counted correctly too, and a
    read id outside [0, R) lands in no word."""
    arr, lengths, k, occ = PAIRS["runs"]
    rev = tuple(a[::-1].copy() for a in arr)
    rev = (np.sort(rev[0], kind="stable"),) + tuple(a[np.argsort(rev[0], kind="stable")] for a in rev[1:])
    assert (np.diff(rev[1][rev[0] == -50]) < 0).all()
    same(run_lower(rev, lengths, k, occ), CR.lower_hits(rev, lengths, k, occ)[:1] + (ref_lower("runs")[1],), "descending runs")
    low, rec = run_lower(arr, lengths[:9], k, occ)           # reads 9, 10, 11 are outside: never a lower read of a hit that counts
    assert np.array_equal(low, ref_lower("runs")[0][:9]) and np.array_equal(rec, ref_lower("runs")[1])


@pytest.mark.parametrize("name", list(PAIRS))
def test_seed_hits_of_every_read_range(lib, name):
    got = check_ranges(name)
    if name == "runs":
        R = len(PAIRS[name][1])
        assert got[0, 2][0].size > 0 and got[2, 5][0].size > 0 and got[0, 2][0].size + got[2, R][0].size == 17   # a run is split
        assert got[3, 3][0].size == 0 and got[R, R][0].size == 0


def test_seed_hits_of_a_read_range_on_several_threads(lib):
    arr, lengths, k, occ = PAIRS["runs"]
    for lo, hi in ((0, 12), (1, 4), (2, 3), (5, 5)):
        same(run_range(arr, lengths, k, occ, lo, hi, threads=3), run_range(arr, lengths, k, occ, lo, hi), (lo, hi))


PLANS = {   # name -> (counts, max_hits, bounds)
    "budget == one read": ([5, 5, 5], 5, [0, 1, 2, 3]),
    "budget one less": ([5, 5, 5], 4, [0, 1, 2, 3]),
    "budget one more": ([5, 5, 5], 6, [0, 1, 2, 3]),
    "two fit exactly": ([5, 5, 5], 10, [0, 2, 3]),
    "all fit": ([5, 5, 5], 15, [0, 3]),
    "leading zeros": ([0, 0, 3, 3], 3, [0, 3, 4]),
    "trailing zeros": ([3, 3, 0, 0], 3, [0, 1, 4]),
    "interior zeros": ([3, 0, 0, 3, 0, 1], 3, [0, 3, 5, 6]),
    "oversize first": ([9, 1, 1], 2, [0, 1, 3]),
    "oversize last": ([1, 1, 9], 2, [0, 2, 3]),
    "oversize between": ([1, 9, 1], 2, [0, 1, 2, 3]),
    "oversize after zeros": ([0, 0, 9, 0, 1], 2, [0, 2, 3, 5]),
    "all oversize": ([4, 3, 5], 2, [0, 1, 2, 3]),
    "all zeros": ([0, 0, 0, 0], 1, [0, 4]),
    "one read": ([7], 7, [0, 1]),
    "no reads": ([], 3, [0]),
    "large budget": ([2 ** 40, 2 ** 40, 1], 2 ** 62, [0, 3]),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_chunks_on_hand_written_counts(lib, name):
    from gnnome_assembly_amd import overlap
    counts, max_hits, want = PLANS[name]
    bounds, chunk_hits = overlap.plan_chunks(torch.tensor(counts, dtype=torch.int64), max_hits)
    assert bounds.dtype == chunk_hits.dtype == torch.int64 and bounds.tolist() == want, (name, bounds.tolist())
    b, sums, oversize = CR.plan(counts, max_hits)
    assert b == want and chunk_hits.tolist() == sums and int((chunk_hits > max_hits).sum()) == oversize
    assert bounds[0] == 0 and bounds[-1] == len(counts) and (bounds[1:] > bounds[:-1]).all()
    for lo, hi, s in zip(want[:-1], want[1:], sums):
        assert s == sum(counts[lo:hi]) and (s <= max_hits or hi - lo == 1), (name, lo, hi, s)
        assert hi == len(counts) or s + counts[hi] > max_hits, (name, lo, hi, "the chunk is maximal")


def test_plan_chunks_on_random_counts(lib):
    from gnnome_assembly_amd import overlap
    rng = np.random.default_rng(5)
    for _ in range(60):
        counts = (rng.integers(0, 12, int(rng.integers(0, 40))) * (rng.random(1) < 0.8)).tolist()
        m = int(rng.integers(1, 30))
        bounds, chunk_hits = overlap.plan_chunks(torch.tensor(counts, dtype=torch.int64), m)
        b, sums, _ = CR.plan(counts, m)
        assert bounds.tolist() == b and chunk_hits.tolist() == sums, (counts, m)


def store_of(seqs, dev="cpu"):
    from gnnome_assembly_amd.reads import ReadStore
    return ReadStore.from_sequences(seqs).to(dev)


def find(store, **kw):
    from gnnome_assembly_amd import overlap
    return overlap.find_overlaps(store, **kw)


def same_overlaps(got, want, what, calls=False):
    """Every tensor of the OverlapGraph, the counts and every record word (but `calls` unless asked) are equal."""
    for a, b, k in zip(got.graph.edges(), want.graph.edges(), ("src", "dst")):
        assert a.dtype == b.dtype and torch.equal(a, b), (what, k)
    assert sorted(got.graph.edata) == sorted(want.graph.edata), (what, sorted(got.graph.edata))
    for k in want.graph.edata:
        assert k in GRAPH_TENSORS and got.graph.edata[k].dtype == want.graph.edata[k].dtype, (what, k)
        assert torch.equal(got.graph.edata[k], want.graph.edata[k]), (what, k)
    assert torch.equal(got.read_length, want.read_length) and torch.equal(got.contained, want.contained), what
    assert got.contained.dtype == torch.bool and got.graph.num_nodes() == want.graph.num_nodes()
    assert (got.hit_count, got.exceeded_pairs, got.sketch_size) == (want.hit_count, want.exceeded_pairs, want.sketch_size), what
    skip = () if calls else ("calls",)
    gs, ws = (dict(zip(O.COUNTERS, o.stats.words())) for o in (got, want))
    assert {k: v for k, v in gs.items() if k not in skip} == {k: v for k, v in ws.items() if k not in skip}, what
    assert got.stats.words() == got.record.tolist()


def check_budgets(store, kw, budgets=BUDGETS):
    """find_overlaps(max_hits=m) for every budget against max_hits=None on the same store; returns {budget: OverlapGraph}."""
    want = find(store, **kw)
    total = want.hit_count
    assert want.chunks == 1 and want.peak_hits == total and want.oversize_chunks == 0 and total > 100
    out = {None: want}
    for b in budgets:
        m = eval(b, {"total": total})
        got = find(store, max_hits=m, **kw)
        same_overlaps(got, want, (b, m))
        out[b] = got
    return out


@pytest.fixture(scope="module")
def lower_of_genome(lib):
    """rate -> lower_hits of the genome case under GENOME's scheme (through the engine: the reference covers it on PAIRS)."""
    from gnnome_assembly_amd import engine

    def get(rate):
        st = store_of(genome_case(rate)["reads"])
        rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64)
        h, rd, _, _ = engine.sketch(st.base_off, st.length, st.packed, GENOME["k"], GENOME["w"], rec)
        h, o = torch.sort(h, stable=True)
        return engine.seed_pairs_lower_hits(h, rd[o].contiguous(), len(st), 64, torch.zeros(len(st), dtype=torch.int64), rec)
    return lambda rate: O.cached(("genome lower", rate), lambda: get(rate))


@pytest.mark.parametrize("drop_contained", [True, False])
@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("rate", [0.0, 0.01])
def test_chunked_find_overlaps_equals_unchunked(lib, lower_of_genome, rate, verify, drop_contained):
    from gnnome_assembly_amd import overlap
    kw = dict(GENOME, verify=verify, drop_contained=drop_contained, max_errors=8)
    out = check_budgets(store_of(genome_case(rate)["reads"]), kw)
    want, low = out[None], lower_of_genome(rate)
    total = want.hit_count
    assert int(low.sum()) == total and want.graph.num_edges() > 20 and bool(want.contained.any())
    assert (want.exceeded_pairs > 0) == (verify and rate > 0)
    for b in BUDGETS:
        m, got = eval(b, {"total": total}), out[b]
        assert got.peak_hits <= max(m, int(low.max())), (b, got.peak_hits)
        if b in BUDGETS[:4]:
            assert got.chunks >= 2, (b, got.chunks)
        else:
            assert got.chunks == 1 and got.oversize_chunks == 0 and got.peak_hits == total, (b, got.chunks)
        bounds, chunk_hits = overlap.plan_chunks(low, m)
        assert got.chunks == int((chunk_hits > 0).sum()) and got.oversize_chunks == int((chunk_hits > m).sum())
        assert got.peak_hits == int(chunk_hits.max())
    assert out["1"].chunks == int((low > 0).sum()) and out["1"].oversize_chunks == int((low > 1).sum()) > 0


def shared_run_reads():
    """The genome's reads, the first 30 of them behind the same 120 bases: every minimizer of that stretch is one run of 30
    entries, and read 0 is the lower read of 29 hits per run."""
    from align_reference import random_sequence
    head = random_sequence(np.random.default_rng(31), 120)
    reads = genome_case(0.0)["reads"]
    return [head + r for r in reads[:30]] + reads[30:]


def test_a_read_with_more_hits_than_the_budget(lib):
    from gnnome_assembly_amd import engine
    st = store_of(shared_run_reads())
    kw = dict(GENOME, verify=True, max_errors=31, drop_contained=False)
    want = find(st, **kw)
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64)
    h, rd, _, _ = engine.sketch(st.base_off, st.length, st.packed, GENOME["k"], GENOME["w"], rec)
    h, o = torch.sort(h, stable=True)
    low = engine.seed_pairs_lower_hits(h, rd[o].contiguous(), len(st), 64, torch.zeros(len(st), dtype=torch.int64), rec)
    top = int(low.max())
    assert int(low[0]) >= 29 * 10 and int(low[-1]) == 0 and want.graph.num_edges() > 20
    for m in (top - 1, top, int(low[5])):
        got = find(st, max_hits=m, **kw)
        same_overlaps(got, want, ("shared run", m))
        assert got.oversize_chunks == int((low > m).sum()) and got.peak_hits <= max(m, top)
        assert got.oversize_chunks >= 1 or m == top


def test_stores_without_hits(lib):
    """No reads, one read, reads that share nothing: no chunk is run, and the result is the unchunked one."""
    rng = np.random.default_rng(3)
    from align_reference import random_sequence
    for seqs in ([], [random_sequence(rng, 400)], [random_sequence(rng, 300) for _ in range(3)]):
        st = store_of(seqs)
        want, got = find(st, **GENOME), find(st, max_hits=5, **GENOME)
        same_overlaps(got, want, len(seqs), calls=True)
        assert got.chunks == 0 and got.peak_hits == 0 and got.hit_count == 0 and got.graph.num_edges() == 0


def test_symbols_fields_and_exports(lib):
    from gnnome_assembly_amd import _lib, engine, overlap
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr and name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert "#define GNM_ABI_VERSION 7" in hdr and lib.gnm_abi_version() == 7
    assert "plan_chunks" in overlap.__all__ and callable(engine.seed_pairs_lower_hits) and callable(engine.seed_pairs_range)
    fields = list(overlap.OverlapGraph.__dataclass_fields__)
    assert fields[-3:] == ["chunks", "peak_hits", "oversize_chunks"] and fields[:8][-1] == "exceeded_pairs"


def test_refusals(lib):
    from gnnome_assembly_amd import _lib, engine, overlap
    st = store_of(genome_case(0.0)["reads"][:12])
    for bad in (0, -1, True, False, 1.5, "auto", 2 ** 63):
        with pytest.raises(ValueError, match="max_hits"):
            overlap.find_overlaps(st, max_hits=bad, **GENOME)
        with pytest.raises(ValueError, match="max_hits"):
            overlap.plan_chunks(torch.zeros(3, dtype=torch.int64), bad)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), [1, 2]):
        with pytest.raises(ValueError, match="lower_hits"):
            overlap.plan_chunks(bad, 4)
    arr, lengths, k, occ = PAIRS["runs"]
    R = len(lengths)
    ts = [_t(a, "cpu") for a in arr] + [_t(lengths, "cpu")]
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64)
    for lo, hi in ((3, 2), (0, R + 1), (-1, 2), (R + 1, R + 1), (True, 2), (0, 2.0)):
        with pytest.raises(ValueError, match="a_lo|a_hi"):
            engine.seed_pairs_range(*ts, k, occ, lo, hi, rec)
    with pytest.raises(ValueError, match="rec"):
        engine.seed_pairs_range(*ts, k, occ, 0, R, rec[:5])
    low = torch.zeros(R, dtype=torch.int64)
    for bad in (low.int(), low[:-1], torch.zeros(R + 1, dtype=torch.int64), torch.zeros(2 * R, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError, match="lower_hits"):
            engine.seed_pairs_lower_hits(ts[0], ts[1], R, occ, bad, rec)
    with pytest.raises((ValueError, _lib.GnmError)):
        engine.seed_pairs_lower_hits(ts[0], ts[1], R, occ, low.to("meta"), rec)     # another device than the sketch's
    for kw in (dict(R=-1), dict(R=True), dict(max_occ=0), dict(max_occ=4097)):
        a = dict(R=R, max_occ=occ)
        a.update(kw)
        with pytest.raises(ValueError):
            engine.seed_pairs_lower_hits(ts[0], ts[1], a["R"], a["max_occ"], low, rec)
    assert not rec.any() and not low.any()
    # the C entries: refused before anything runs or is launched, the record and lower_hits as they were
    crec, a, tot = (C.c_int64 * 14)(), (C.c_int64 * 16)(), C.c_int64(0)
    odd, odd_a = C.c_void_p(C.addressof(crec) + 4), C.c_void_p(C.addressof(a) + 4)
    lh = dict(M=2, hash=a, read=a, occ=4, lower=a, R=3, rec=crec, threads=1)
    ok_rec = (C.c_int64 * 14)()
    assert lib.gnm_seed_pairs_lower_hits_host(*dict(lh, rec=ok_rec).values()) == 0
    assert not any(a) and list(ok_rec)[3:8] == [1, 0, 0, 0, 1]          # two entries of read 0 in one run: same_read, no hit
    for change in (dict(M=-1), dict(occ=0), dict(occ=4097), dict(hash=None), dict(read=None), dict(lower=None), dict(lower=odd_a),
                   dict(R=-1), dict(R=2 ** 31 - 1), dict(rec=None), dict(rec=odd), dict(threads=0)):
        assert lib.gnm_seed_pairs_lower_hits_host(*dict(lh, **change).values()) < 0, change
        assert lib.gnm_last_error()
    dv = dict(M=2, hash=a, read=a, occ=4, lower=a, R=3, rec=crec, ws=None, wsb=0, stream=None)
    for change in (dict(M=-1), dict(occ=0), dict(hash=None), dict(lower=None), dict(lower=odd_a), dict(R=-1), dict(rec=None), dict(rec=odd)):
        assert lib.gnm_seed_pairs_lower_hits(*dict(dv, **change).values()) < 0, change
    rg = dict(M=2, hash=a, read=a, pos=a, strand=a, length=a, R=3, k=15, occ=4, lo=0, hi=3, cap=-1, key=None, diag=None,
              total=C.byref(tot), rec=crec, threads=1)
    assert lib.gnm_seed_pairs_range_host(*rg.values()) == 0 and tot.value == 0
    for change in (dict(lo=2, hi=1), dict(hi=4), dict(lo=-1), dict(lo=4, hi=4), dict(occ=0), dict(M=-1), dict(hash=None), dict(pos=None),
                   dict(length=None), dict(k=3), dict(rec=odd), dict(rec=None), dict(total=None), dict(threads=2000)):
        assert lib.gnm_seed_pairs_range_host(*dict(rg, **change).values()) < 0, change
    cr = dict(M=2, hash=a, read=a, occ=4, lo=0, hi=3, R=3, off=a, rec=crec, ws=None, wsb=0, stream=None)
    for change in (dict(lo=2, hi=1), dict(hi=4), dict(lo=-1), dict(R=-1), dict(occ=0), dict(off=None), dict(rec=odd), dict(rec=None),
                   dict(hash=None), dict()):                 # the last: a null workspace for M = 2
        assert lib.gnm_seed_pairs_count_range(*dict(cr, **change).values()) < 0, change
    er = dict(M=2, hash=a, read=a, pos=a, strand=a, length=a, R=3, k=15, occ=4, lo=0, hi=3, off=a, N=1, key=a, diag=a, stream=None)
    for change in (dict(lo=2, hi=1), dict(hi=4), dict(lo=-1), dict(N=-1), dict(key=None), dict(off=None), dict(pos=None), dict(k=32),
                   dict(occ=4097)):
        assert lib.gnm_seed_pairs_emit_range(*dict(er, **change).values()) < 0, change
    assert list(crec) == [0] * 14
