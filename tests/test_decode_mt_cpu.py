"""gnm_decode_iteration_mt (host threads, no GPU needed): whole decodes, iteration by iteration, against
gnm_decode_iteration on the same start edges -- the walk, *best_length_out and visited[] after every iteration are EQUAL for
every thread count -- plus the error codes, nb < threads, and get_contigs_device's refusal of host scores."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

THREADS = (1, 2, 5, 16)


def _iteration(fn, g, sc, pl, rl, vis, s0, d0, thr, *extra):
    from gnnome_assembly_amd import decode
    p = decode._p
    walk = np.full(2 * g.n + 2, -1, np.int32)
    blen = C.c_int64(-7)
    ln = fn(g.n, p(sc), p(pl), p(rl), *[p(a) for a in g.succ], *[p(a) for a in g.pred], p(vis), int(s0.size), p(s0), p(d0),
            int(thr), p(walk), walk.size, C.byref(blen), *extra)
    return int(ln), walk[:max(ln, 0)].copy(), blen.value


def _decode_both(src, dst, n, sc, pl, rl, thr, nb, threads, rng, vis0=None, max_iter=10 ** 6):
    """Drive the serial and the threaded iteration side by side with the same random picks among the candidate edges."""
    from gnnome_assembly_amd import _lib, decode
    lib = _lib.load()
    g = decode.DecodeGraph(src, dst, n)
    sc = np.ascontiguousarray(sc, dtype=np.float32)
    pl = np.ascontiguousarray(pl, dtype=np.int64)
    rl = np.ascontiguousarray(rl, dtype=np.int64)
    va = np.zeros(n, np.uint8) if vis0 is None else vis0.copy()
    vb = va.copy()
    accepted = 0
    for _ in range(max_iter):
        free = va == 0
        eid = np.flatnonzero(free[g.src] & free[g.dst] & (g.src != g.dst))
        if eid.size == 0:
            break
        picks = eid[rng.integers(0, eid.size, nb)]
        s0, d0 = np.ascontiguousarray(g.src[picks]), np.ascontiguousarray(g.dst[picks])
        la, wa, ba = _iteration(lib.gnm_decode_iteration, g, sc, pl, rl, va, s0, d0, thr)
        lb, wb, bb = _iteration(lib.gnm_decode_iteration_mt, g, sc, pl, rl, vb, s0, d0, thr, threads)
        assert la >= 0 and la == lb and np.array_equal(wa, wb) and ba == bb
        assert np.array_equal(va, vb)
        if la < thr:
            break
        accepted += 1
    return accepted


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("seed,thr", [(0, 20), (1, 5), (2, 60)])
def test_mt_whole_decode_equals_serial_on_synthetic_graphs(seed, thr, threads):
    from gnnome_assembly_amd import synth
    rng = np.random.default_rng(seed)
    src, dst, n = synth.make_graph(500, seed=seed, permute_edge_ids=True)
    e = src.size
    scores = (rng.standard_normal(e) * 2).astype(np.float32)
    pl = rng.integers(500, 12000, e)
    rl = rng.integers(8000, 25000, n)
    assert _decode_both(src, dst, n, scores, pl, rl, thr, 20, threads, np.random.default_rng(100 + seed)) > 0


@pytest.mark.parametrize("threads", THREADS)
def test_mt_equals_serial_on_reference_golden(threads):
    """The reference-generated graph of decode_walks.npz: its recorded start edges all at once from every recorded visited
    state, then whole decodes with equal prefix lengths (every walk of equal node count ties: the FIRST must win)."""
    from gnnome_assembly_amd import _lib, decode
    z = np.load(os.path.join(GOLDEN, "decode_walks.npz"))
    n = int(z["n"])
    old = np.unpackbits(z["visited_old"], axis=1)[:, :n].astype(np.uint8)
    lib = _lib.load()
    g = decode.DecodeGraph(z["src"], z["dst"], n)
    sc = np.ascontiguousarray(z["scores"], dtype=np.float32)
    pl, rl = np.ascontiguousarray(z["prefix_length"], dtype=np.int64), np.ascontiguousarray(z["read_length"], dtype=np.int64)
    s0, d0 = np.ascontiguousarray(g.src[z["starts"]]), np.ascontiguousarray(g.dst[z["starts"]])
    for i in range(old.shape[0]):
        for thr in (1, 10 ** 9):
            va, vb = old[i].copy(), old[i].copy()
            la, wa, ba = _iteration(lib.gnm_decode_iteration, g, sc, pl, rl, va, s0, d0, thr)
            lb, wb, bb = _iteration(lib.gnm_decode_iteration_mt, g, sc, pl, rl, vb, s0, d0, thr, threads)
            assert la > 0 and la == lb and np.array_equal(wa, wb) and ba == bb and np.array_equal(va, vb), (i, thr)
    for thr, plx, rlx in ((5, pl, rl), (3, np.ones_like(pl), np.ones_like(rl))):
        _decode_both(z["src"], z["dst"], n, sc, plx, rlx, thr, 12, threads, np.random.default_rng(7))


@pytest.mark.parametrize("threads", THREADS)
def test_mt_error_codes_are_those_of_the_lowest_failing_candidate(threads):
    from gnnome_assembly_amd import _lib, decode
    lib = _lib.load()
    # 0 -> 2 -> 4 -> 0: every node has exactly one successor: a forced-move cycle (-3)
    g = decode.DecodeGraph(np.array([0, 2, 4], np.int32), np.array([2, 4, 0], np.int32), 6)
    sc, pl, rl = np.zeros(3, np.float32), np.ones(3, np.int64), np.ones(6, np.int64)
    s0, d0 = np.array([0, 2], np.int32), np.array([2, 4], np.int32)
    for fn, extra in ((lib.gnm_decode_iteration, ()), (lib.gnm_decode_iteration_mt, (threads,))):
        vis = np.zeros(6, np.uint8)
        assert _iteration(fn, g, sc, pl, rl, vis, s0, d0, 1, *extra)[0] == -3
        assert b"forced" in lib.gnm_last_error() and not vis.any()
    # a chain 0 -> 2 -> 4 -> 6 and the start "edge" 0 -> 6, which is no edge (-4); with the cycle-free candidates around it
    # and an out-of-range one (-2) after it, the lowest failing index decides
    g = decode.DecodeGraph(np.array([0, 2, 4], np.int32), np.array([2, 4, 6], np.int32), 8)
    rl = np.ones(8, np.int64)
    for s0, d0, want in (([0, 0, 2], [2, 6, 4], -4), ([0, 0, 9], [2, 6, 4], -4), ([0, 9, 0], [2, 4, 6], -2),
                         ([0], [6], -4)):
        s0, d0 = np.array(s0, np.int32), np.array(d0, np.int32)
        for fn, extra in ((lib.gnm_decode_iteration, ()), (lib.gnm_decode_iteration_mt, (threads,))):
            vis = np.zeros(8, np.uint8)
            assert _iteration(fn, g, sc, pl, rl, vis, s0, d0, 1, *extra)[0] == want
            assert not vis.any()
    assert _iteration(lib.gnm_decode_iteration_mt, g, sc, pl, rl, np.zeros(8, np.uint8), np.zeros(0, np.int32),
                      np.zeros(0, np.int32), 1, threads)[0] == -1                      # nb == 0: bad argument, as the serial call


def test_mt_with_fewer_candidates_than_threads():
    from gnnome_assembly_amd import synth
    rng = np.random.default_rng(3)
    src, dst, n = synth.make_graph(500, seed=3, permute_edge_ids=True)
    e = src.size
    scores = (rng.standard_normal(e) * 2).astype(np.float32)
    for nb in (1, 3):
        assert _decode_both(src, dst, n, scores, rng.integers(500, 12000, e), rng.integers(8000, 25000, n), 5, nb, 16,
                            np.random.default_rng(nb)) > 0


def test_default_thread_count_never_follows_the_core_count(monkeypatch):
    from gnnome_assembly_amd import decode
    monkeypatch.delenv("GNM_DECODE_THREADS", raising=False)
    assert decode.decode_threads(50) == 16 and decode.decode_threads(3) == 3
    monkeypatch.setenv("GNM_DECODE_THREADS", "4")
    assert decode.decode_threads(50) == 4


def test_get_contigs_device_rejects_host_scores():
    from gnnome_assembly_amd import _lib, decode
    g = decode.DecodeGraph(np.array([0, 2], np.int32), np.array([2, 4], np.int32), 6)
    for scores in (torch.zeros(2), np.zeros(2, np.float32)):
        with pytest.raises(_lib.GnmError, match="HIP device"):
            decode.get_contigs_device(g, scores, np.ones(2, np.int64), np.ones(6, np.int64))
