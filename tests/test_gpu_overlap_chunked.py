"""GPU: the overlap graph in read-range chunks on the device (csrc/gnm_overlap.hip: pair_lower_k and the range forms of pair_k)
against tests/overlap_chunk_reference.py and the host entries -- the cases of test_overlap_chunked_cpu.py; entry counts at the
scan block's edges; a store of 257 reads, chunked on the device against unchunked and against the CPU store, under occupancy caps
and twice; an output one element short; a read with more hits than the budget.  Every comparison is an equality."""
import numpy as np
import pytest
import torch

import overlap_chunk_reference as CR
import overlap_reference as O
from test_overlap_chunked_cpu import (PAIRS, check_ranges, find, ref_lower, run_lower, run_range, same_overlaps, shared_run_reads,
                                      store_of)
from test_overlap_cpu import GENOME, _t, genome_case, run_pairs, same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KW = dict(GENOME, max_occ=256, verify=True, max_errors=12)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", list(PAIRS))
def test_lower_hits_and_read_ranges_on_the_device(lib, name):
    got = run_lower(*PAIRS[name], DEV)
    same(got, ref_lower(name), name)
    same(got, run_lower(*PAIRS[name]), name + " (host entry)")
    ranges = check_ranges(name, DEV)                         # every range against the reference, every partition's concatenation
    if name == "runs":
        assert ranges[0, 2][0].size > 0 and ranges[2, 5][0].size > 0        # the run of reads 0 .. 4 is split between two ranges


@pytest.mark.parametrize("M", [0, 1, 255, 256, 257, 256 * 256 + 1])   # the scan block B = 256: B - 1, B, B + 1; 257 scan blocks
def test_lower_hits_and_ranges_at_the_scan_block_edges(lib, M):
    """The entries of test_seed_hit_offsets_at_the_scan_block_edges: runs of two entries of reads a < b = a + 1, a = 2 (j % 500),
    hit j with diag j.  lower_hits[a] = the runs of a; a range keeps the hits of its even reads, in order.  Closed form, and the
    host entries on the same arrays."""
    i = np.arange(M)
    a = 2 * ((i // 2) % 500)
    arr = (i // 2, (a + i % 2).astype(np.int32), np.where(i % 2 == 0, i // 2, 0).astype(np.int32), np.zeros(M, np.uint8))
    lengths = np.full(1000, 5000, np.int64)
    N = M // 2
    aj = 2 * (np.arange(N, dtype=np.int64) % 500)
    rec = np.zeros(len(O.COUNTERS), np.int64)
    rec[O.COUNTERS.index("runs")], rec[O.COUNTERS.index("hits")] = (M + 1) // 2, N
    got = run_lower(arr, lengths, 15, 16, DEV)
    same(got, (np.bincount(aj, minlength=1000).astype(np.int64), rec), f"M = {M}")
    same(got, run_lower(arr, lengths, 15, 16), f"M = {M} (host entry)")
    hits = ((aj << 32) | ((aj + 1) << 1), np.arange(N, dtype=np.int32))
    parts = []
    for lo, hi in ((0, 1), (1, 333), (333, 334), (334, 1000)):          # 333 is odd: never a lower read; (0, 1): read 0 alone
        part = run_range(arr, lengths, 15, 16, lo, hi, DEV)
        same(part, CR.range_hits(hits, lo, hi) + (0 * rec,), f"M = {M}, [{lo}, {hi})")
        parts.append(part)
    same(run_range(arr, lengths, 15, 16, 0, 1000, DEV)[:2], run_pairs(arr, lengths, 15, 16, DEV)[:2], f"M = {M}, [0, R)")
    same(run_range(arr, lengths, 15, 16, 1, 334, DEV), run_range(arr, lengths, 15, 16, 1, 334), f"M = {M} (host entry)")
    assert sum(p[0].size for p in parts) == N


@pytest.fixture(scope="module")
def store257(lib):
    """257 reads: the genome's 60 with 2 % errors, replicated (as test_replicated_store_grids_and_repeats does) and cut; the
    unchunked result on the device and the hits per lower read."""
    seqs = (genome_case(0.02)["reads"] * 5)[:257]
    want = find(store_of(seqs, DEV), **KW)
    assert want.hit_count > 256 * 256 and want.stats.skipped_runs == 0 and want.exceeded_pairs > 0      # the case is not trivial:
    assert want.graph.num_edges() > 20 and bool(want.contained.any()) and want.stats.groups > 256      # copies contain each other
    return seqs, want


@pytest.mark.parametrize("budget", ["1", "total // 5", "total"])
def test_chunked_on_the_device_equals_unchunked_and_the_cpu_store(store257, budget):
    seqs, want = store257
    m = eval(budget, {"total": want.hit_count})
    got = find(store_of(seqs, DEV), max_hits=m, **KW)
    same_overlaps(got, want, budget)
    assert got.graph.device == DEV and got.contained.device == DEV
    host = O.cached(("chunked host", budget), lambda: find(store_of(seqs), max_hits=m, **KW))
    for a, b in zip(got.graph.edges(), host.graph.edges()):
        assert torch.equal(a.cpu(), b)
    for k in host.graph.edata:
        assert torch.equal(got.graph.edata[k].cpu(), host.graph.edata[k]), k
    assert torch.equal(got.contained.cpu(), host.contained) and got.stats == host.stats
    assert (got.chunks, got.peak_hits, got.oversize_chunks, got.hit_count) == (host.chunks, host.peak_hits, host.oversize_chunks, host.hit_count)
    if budget == "total":
        assert got.chunks == 1 and got.oversize_chunks == 0
    else:
        assert got.chunks >= 5 and got.peak_hits < want.hit_count


def test_chunked_is_independent_of_the_grid(lib, store257):
    seqs, want = store257
    st, m = store_of(seqs, DEV), want.hit_count // 5
    runs = []
    try:
        for cap in (1, 2):
            lib.gnm_set_occupancy_cap(cap)
            runs += [find(st, max_hits=m, **KW), find(st, max_hits=m, **KW)]
    finally:
        lib.gnm_set_occupancy_cap(0)
    runs += [find(st, max_hits=m, **KW), find(st, max_hits=m, **KW)]
    for i, got in enumerate(runs):
        same_overlaps(got, want, f"run {i}")
        assert (got.chunks, got.peak_hits, got.oversize_chunks) == (runs[0].chunks, runs[0].peak_hits, runs[0].oversize_chunks)


def test_emit_range_writes_nothing_past_the_size_it_is_given(lib):
    from gnnome_assembly_amd import engine
    arr, lengths, k, occ = PAIRS["runs"]
    ts = [_t(a, DEV) for a in arr] + [_t(lengths, DEV)]
    M, R, lo, hi = len(arr[0]), len(lengths), 0, 5
    key, diag, _ = run_range(arr, lengths, k, occ, lo, hi, DEV)
    N = key.size
    assert N >= 10
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=DEV)
    off = torch.empty(M + 1, dtype=torch.int64, device=DEV)
    need = lib.gnm_overlap_scan_workspace_bytes(M)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p = engine._ptr
    engine._call("gnm_seed_pairs_count_range", M, p(ts[0]), p(ts[1]), occ, lo, hi, R, p(off), p(rec), p(ws), need, engine._stream())
    assert int(off[-1]) == N and not bool(rec.any())
    for short in (1, 3, N):
        gk = torch.full((N,), -7, dtype=torch.int64, device=DEV)       # slots [N - short, N) are the guard
        gd = torch.full((N,), -7, dtype=torch.int32, device=DEV)
        engine._call("gnm_seed_pairs_emit_range", M, *[p(t) for t in ts], R, k, occ, lo, hi, p(off), N - short, p(gk), p(gd), engine._stream())
        assert np.array_equal(gk.cpu().numpy()[:N - short], key[:N - short]) and np.array_equal(gd.cpu().numpy()[:N - short], diag[:N - short])
        assert bool((gk[N - short:] == -7).all()) and bool((gd[N - short:] == -7).all()), short


def test_a_read_with_more_hits_than_the_budget_on_the_device(lib):
    from gnnome_assembly_amd import engine
    seqs = shared_run_reads()
    st = store_of(seqs, DEV)
    kw = dict(GENOME, verify=True, max_errors=31, drop_contained=False)
    want = find(st, **kw)
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=DEV)
    h, rd, _, _ = engine.sketch(st.base_off, st.length, st.packed, GENOME["k"], GENOME["w"], rec)
    h, o = torch.sort(h, stable=True)
    low = engine.seed_pairs_lower_hits(h, rd[o].contiguous(), len(st), 64, torch.zeros(len(st), dtype=torch.int64, device=DEV), rec)
    top = int(low.max())
    assert int(low[0]) >= 29 * 10 and int(low.sum()) == want.hit_count
    got = find(st, max_hits=top - 1, **kw)
    same_overlaps(got, want, "shared run")
    assert got.oversize_chunks >= 1 and got.peak_hits == top and got.chunks >= 2
    host = find(store_of(seqs), max_hits=top - 1, **kw)
    assert got.stats == host.stats and torch.equal(got.graph.edata["twin"].cpu(), host.graph.edata["twin"])
    assert (got.chunks, got.oversize_chunks) == (host.chunks, host.oversize_chunks)
