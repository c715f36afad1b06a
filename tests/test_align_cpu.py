"""CPU: the overlap alignment's arithmetic (csrc/gnm_align.h) through gnm_overlap_align_host against the plain dynamic programme of
tests/align_reference.py: hand cases with known distances, the band's word boundaries, short and empty targets, both strands and
nibble phases, ambiguity codes, bad input, random pairs; the bindings and the refusals.  Integers, and fp32 values formed from the
same two integers: every comparison is an equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import align_reference as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = A.all_cases()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def host_align(store, n, src, dst, pl, K, threads=1):
    """gnm_overlap_align_host -> (dist, overlap_length, similarity, record) as numpy arrays."""
    from gnnome_assembly_amd import engine
    E = len(src)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt)))  # noqa: E731
    dist, olen = torch.full((E,), 77, dtype=torch.int32), torch.full((E,), 77, dtype=torch.int64)
    sim, rec = torch.full((E,), 77.0), torch.zeros(engine.ALIGN_RECORD_WORDS, dtype=torch.int64)
    engine.overlap_align_host(t(src, np.int32), t(dst, np.int32), t(pl, np.int64), n, store.base_off, store.length, store.packed, K,
                              dist, olen, sim, rec, threads)
    return dist.numpy(), olen.numpy(), sim.numpy(), rec.numpy()


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("dist", "overlap_length", "similarity", "record")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert np.array_equal(gb, wb), (what, name, np.flatnonzero(gb != wb)[:8], g[gb != wb][:8], w[gb != wb][:8])


@pytest.mark.parametrize("name", list(CASES))
def test_host_entry_equals_the_dynamic_programme(lib, name):
    case = CASES[name]
    store, want = A.reference(case)
    _, _, n, src, dst, pl, K = case
    assert_same(host_align(store, n, src, dst, pl, K), want, name)
    assert_same(host_align(store, n, src, dst, pl, K, threads=3), want, name + " (3 threads)")


@pytest.mark.parametrize("K", [1, 3, 40])
def test_hand_cases_have_the_distances_they_were_built_with(lib, K):
    case, expect = A.hand_cases(K)
    dist, olen, sim, rec = A.reference(case)[1]
    assert dist.tolist() == expect and rec[A.COUNTERS.index("exceeded")] == 1 and rec[A.COUNTERS.index("aligned")] == 5
    assert sim[0] == 1.0 and sim[1] == np.float32(1) - np.float32(1) / np.float32(olen[1])
    got = host_align(A.reference(case)[0], *case[2:])
    assert got[0].tolist() == expect


def test_codes_match_when_equal_only(lib):
    case, expect = A.code_case(2)
    store, want = A.reference(case)
    assert want[0].tolist() == expect and host_align(store, *case[2:])[0].tolist() == expect


def test_bad_input_is_counted_and_never_read_through(lib):
    case = A.bad_case(10)
    store, want = A.reference(case)
    dist, olen, sim, rec = host_align(store, *case[2:])
    r = dict(zip(A.COUNTERS, rec.tolist()))
    la = int(store.length[0])
    assert dist.tolist()[4:] == [-1] * 5 and olen.tolist()[4:] == [0] * 5 and sim.tolist()[4:] == [0.0] * 5
    assert r["invalid"] == 5 and r["clamped"] == 2 and r["empty"] == 2 and r["edges"] == 9 and r["calls"] == 1
    assert olen.tolist()[:4] == [la - 6, la, 0, 0] and dist.tolist()[2:4] == [0, 0]
    assert r["edges"] == r["aligned"] + r["exceeded"] + r["empty"] + r["invalid"]
    assert_same((dist, olen, sim, rec), want, "bad")


def test_boundary_cases_cover_what_they_claim():
    assert A.BOUNDARY_M == (0, 1, 2, 63, 64, 65, 127, 128, 129, 300) and A.BOUNDARY_K == (0, 1, 31, 32, 63, 64, 127, 128, 255)
    for K in A.BOUNDARY_K:
        olen = A.reference(CASES[f"boundary-K{K}"])[1][1]
        assert (olen < K).any() or K == 0
        assert (olen > K).any() and ((olen == K).any() or K not in A.BOUNDARY_M)
        assert 2 * K + 1 <= 512
    for K in (2, 40):                                      # short targets: forced deletions, certainly exceeded, empty target
        _, seqs, n, src, dst, pl, _ = CASES[f"target_length-K{K}"]
        dist = A.reference(CASES[f"target_length-K{K}"])[1][0]
        lc = [len(seqs[d >> 1]) for d in dst]
        assert lc[-1] == 0 and dist.tolist() == [1, K, K + 1, K + 1, K + 1]


@pytest.mark.parametrize("K", A.RANDOM_K)
def test_random_cases_reach_both_branches(K):
    _, want = A.reference(CASES[f"random-K{K}"])
    r = dict(zip(A.COUNTERS, want[3].tolist()))
    assert r["aligned"] >= 20 and r["exceeded"] >= 5 and r["edges"] == 200, r
    assert r["cells"] > 0 and (want[1] <= 300).all()


def test_calls_add_to_the_record_and_an_empty_call_leaves_it(lib):
    from gnnome_assembly_amd import engine
    case = CASES["codes-K2"]
    store, want = A.reference(case)
    _, _, n, src, dst, pl, K = case
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt)))  # noqa: E731
    E = len(src)
    out = (torch.zeros(E, dtype=torch.int32), torch.zeros(E, dtype=torch.int64), torch.zeros(E))
    rec = torch.zeros(8, dtype=torch.int64)
    for _ in range(2):
        engine.overlap_align_host(t(src, np.int32), t(dst, np.int32), t(pl, np.int64), n, store.base_off, store.length, store.packed,
                                  K, *out, rec)
    assert rec.tolist() == (2 * want[3]).tolist()
    none = lambda dt: torch.zeros(0, dtype=dt)  # noqa: E731
    engine.overlap_align_host(none(torch.int32), none(torch.int32), none(torch.int64), n, store.base_off, store.length, store.packed,
                              K, none(torch.int32), none(torch.int64), none(torch.float32), rec)
    assert rec.tolist() == (2 * want[3]).tolist()


def test_sources_symbols_and_abi(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib, engine, features, decode
    assert "gnm_align.hip" in ge.SOURCES
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    for name in ("gnm_overlap_align", "gnm_overlap_align_host"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct gnm_align_record" in hdr and "#define GNM_ABI_VERSION 7" in hdr and lib.gnm_abi_version() == 7
    assert engine.ALIGN_COUNTERS == A.COUNTERS and engine.ALIGN_RECORD_WORDS == 8 and engine.ALIGN_MAX_ERRORS == 255
    assert tuple(features.AlignStats.__dataclass_fields__) == engine.ALIGN_COUNTERS and features.AlignStats(*range(8)).words() == list(range(8))
    assert {"overlap_features", "OverlapFeatures", "AlignStats"} <= set(features.__all__)
    assert {"junction_identity", "JunctionIdentity"} <= set(decode.__all__)


def test_refusals(lib):
    from gnnome_assembly_amd import _lib, engine, features
    from gnnome_assembly_amd.reads import ReadStore
    rec = (C.c_int64 * 8)()
    one = (C.c_int64 * 4)()
    pk = (C.c_int64 * 4)()                                 # 32 bytes of store, 8-byte aligned
    ok = dict(E=1, src=one, dst=one, pl=one, packed=pk, packed_bytes=32, base_off=one, length=one, R=1, n=2, K=5, dist=one, olen=one,
              sim=one, rec=rec)
    for fn, tail in ((lib.gnm_overlap_align_host, (1,)), (lib.gnm_overlap_align, (None,))):
        for change in (dict(K=-1), dict(K=256), dict(E=-1), dict(src=None), dict(dist=None), dict(pl=None), dict(rec=None),
                       dict(packed_bytes=24), dict(packed=None)):
            assert fn(*dict(ok, **change).values(), *tail) < 0, change
            assert lib.gnm_last_error()
        assert fn(*dict(ok, E=0, src=None, dst=None, pl=None, dist=None, olen=None, sim=None).values(), *tail) == 0
    assert lib.gnm_overlap_align_host(*ok.values(), 0) < 0 and b"threads" in lib.gnm_last_error()
    assert lib.gnm_overlap_align_host(*ok.values(), 1) == 0 and rec[0] == 1        # one edge of two empty reads: counted, empty
    st = ReadStore.from_sequences(["ACGT", "GTAA"])
    z = lambda dt: torch.zeros(1, dtype=dt)  # noqa: E731
    for bad in (-1, 256, True, 2.0):
        with pytest.raises(ValueError, match="max_errors"):
            engine.overlap_align_host(z(torch.int32), z(torch.int32), z(torch.int64), 4, st.base_off, st.length, st.packed, bad,
                                      z(torch.int32), z(torch.int64), z(torch.float32), torch.zeros(8, dtype=torch.int64))
    from gnnome_assembly_amd import AssemblyGraph
    g = AssemblyGraph([0], [2], 4)
    with pytest.raises(_lib.GnmError, match="HIP device"):
        features.overlap_features(g, st, prefix_length=[2])
    with pytest.raises(TypeError):
        features.overlap_features(g, ["ACGT", "GTAA"], prefix_length=[2])
