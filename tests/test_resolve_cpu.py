"""CPU: the round formulation of the strand rule (tests/resolve_reference.py -- what gnm_resolve.hip runs) against the host's
decode.resolve_strands, the bindings of the resolve entry points and the refusals of the Python surface.  Integers, compared for
equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import resolve_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM = 320
THRESHOLDS = (1, 2, 3, 5)


def _same(cover, thr):
    from gnnome_assembly_amd import decode
    want = decode.resolve_strands(R.to_contigs(cover), thr)
    got = R.resolve_rounds(cover, thr)
    assert got["walks"] == want.walks and got["bases"] == want.bases, (thr, got["walks"], want.walks)
    assert got["record"][R.COUNTERS.index("pieces")] == len(want.walks)
    assert got["contig_ptr"].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want.walks])]).astype(int).tolist()
    assert all(got["walk_edges"][p] == -1 for p in got["contig_ptr"][:-1])
    return got


@pytest.mark.parametrize("thr", [1, 2, 3, 4, 5, 6])
def test_the_hand_cases(thr):
    for cover in R.hand_cases():
        _same(cover, thr)


def test_the_rounds_are_the_host_rule_on_random_covers():
    """Equality on every cover, and the set is not vacuous: deep dependency chains, cuts at taken reads, dropped pieces, serially
    cut contigs and ties in bases all occur."""
    seen = dict(rounds3=0, taken_cuts=0, dropped=0, serial=0, ties=0, odd_n=0, absent_twin=0)
    for seed in range(N_RANDOM):
        cover = R.random_cover(seed)
        assert 40 <= cover["n"] <= 600
        on_walk = np.zeros(cover["n"] + 1, np.bool_)
        on_walk[cover["walk_nodes"]] = True
        seen["odd_n"] += cover["n"] % 2
        seen["absent_twin"] += int((on_walk[cover["walk_nodes"]] & ~on_walk[cover["walk_nodes"] ^ 1]).any())
        for thr in THRESHOLDS:
            got = _same(cover, thr)
            rec = dict(zip(R.COUNTERS, got["record"]))
            seen["rounds3"] += got["rounds"] >= 3
            seen["taken_cuts"] += got["taken_cuts"]
            seen["dropped"] += rec["dropped"]
            seen["serial"] += rec["serial"]
            seen["ties"] += got["ties"]
    assert all(v > 0 for v in seen.values()), seen


def test_ties_go_to_the_lower_contig_index_not_the_first_node():
    """Two mirrored contigs of equal bases: the one listed FIRST wins, though its first node id is the larger one."""
    from gnnome_assembly_amd import decode
    cover = R.cover_from_paths([[9, 7, 5], [4, 6, 8]], 10, [1, 1, 1, 1], [3] * 10)
    assert cover["bases"].tolist() == [5, 5]
    assert decode.resolve_strands(R.to_contigs(cover), 1).walks == [[9, 7, 5]] == R.resolve_rounds(cover, 1)["walks"]


def test_the_surface():
    from gnnome_assembly_amd import decode, engine
    assert {"resolve_strands_device", "StrandContigs", "ResolveStats"} <= set(decode.__all__)
    assert issubclass(decode.StrandContigs, decode.BogContigs) and decode.RESOLVE_CHECK_EVERY >= 1
    assert tuple(decode.ResolveStats.__dataclass_fields__) == engine.RESOLVE_COUNTERS == R.COUNTERS
    assert engine.RESOLVE_RECORD_WORDS == 8 and decode.ResolveStats(*range(8)).words() == list(range(8))
    c = R.to_contigs(R.hand_cases()[0])
    with pytest.raises(decode._lib.GnmError, match="HIP device"):
        decode.resolve_strands_device(c, 2)
    with pytest.raises(ValueError, match="check_every"):
        decode.resolve_strands_device(c, 2, check_every=0)
    with pytest.raises(TypeError):
        decode.resolve_strands_device([[0, 1]], 2)
    with pytest.raises(ValueError, match="device_resolve"):
        decode.infer_contigs(None, None, None, None, None, None, decoder="greedy", device_resolve=True)
    with pytest.raises(ValueError, match="device_resolve"):
        decode.infer_contigs(None, None, None, None, None, None, decoder="greedy_cover", device_resolve=1)
    for doc, word in (("README.md", "resolve_strands_device"), ("DESIGN.md", "gnm_resolve"), ("INTEGRATION.md", "gnm_resolve.hip")):
        assert word in open(os.path.join(REPO, doc)).read(), doc


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


NAMES = ("gnm_resolve_workspace_bytes", "gnm_resolve_prepare", "gnm_resolve_rounds", "gnm_resolve_layout")


def test_the_library_binds_the_entry_points_at_abi_7(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib
    assert "gnm_resolve.hip" in ge.SOURCES and lib.gnm_abi_version() == 7 == _lib.ABI_VERSION
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert "gnm_resolve_record" in hdr and "#define GNM_ABI_VERSION 7" in hdr
    assert lib.gnm_resolve_workspace_bytes(-1, 0, 0) == 0 == lib.gnm_resolve_workspace_bytes(0, 2 ** 31 - 1, 0)
    assert 0 < lib.gnm_resolve_workspace_bytes(0, 0, 0) <= 16 * 20
    for c, p, n in ((1, 1, 2), (7, 100, 101), (1025, 70000, 140000)):
        need = 8 * n + 8 * (n // 2 + 1) + 28 * c + 8 * p
        assert need <= lib.gnm_resolve_workspace_bytes(c, p, n) <= need + 16 * 20 + 8 * (c // 1024 + 1), (c, p, n)


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Host-side returns: no device is touched."""
    rec = (C.c_int64 * 8)()
    buf = (C.c_int64 * 64)()
    ws = (C.c_int64 * 1024)()
    p = lambda a: C.c_void_p(C.addressof(a))                                     # noqa: E731
    b, r = p(buf), p(rec)
    w = C.c_void_p(C.addressof(ws) + (C.addressof(ws) % 16))
    need = lib.gnm_resolve_workspace_bytes(2, 6, 8)
    assert 0 < need <= 8 * 1023
    head = dict(C=2, P=6, n=8, E=4, contig_ptr=b, walk_nodes=b, walk_edges=b, order=b, thr=2)
    tail = dict(ws=w, ws_bytes=need, stream=None)
    calls = {
        "gnm_resolve_prepare": dict(head, record=r, **tail),
        "gnm_resolve_rounds": dict(head, first_round=0, rounds=2, undecided=b, record=r, **tail),
        "gnm_resolve_layout": dict(head, prefix_length=b, read_length=b, y=None, record=r, out_ptr=b, out_nodes=b, out_edges=b,
                                   out_bases=b, out_wrong=b, **tail),
    }
    common = ((dict(C=-1), "C = -1"), (dict(P=2 ** 31 - 1), "2^31"), (dict(n=-1), "n = -1"), (dict(E=-1), "E = -1"),
              (dict(thr=0), "len_threshold"), (dict(record=None), "record"), (dict(record=C.c_void_p(C.addressof(rec) + 4)), "aligned"),
              (dict(contig_ptr=None), "contig_ptr"), (dict(order=None), "order"), (dict(walk_nodes=None), "walk_nodes"),
              (dict(walk_edges=None), "walk_edges"), (dict(ws=None), "workspace"), (dict(ws_bytes=need - 1), "workspace"),
              (dict(ws=C.c_void_p(w.value + 4)), "workspace"))
    own = {"gnm_resolve_prepare": (),
           "gnm_resolve_rounds": ((dict(first_round=-1), "first_round"), (dict(rounds=-1), "rounds"), (dict(undecided=None), "undecided"),
                                  (dict(undecided=C.c_void_p(C.addressof(buf) + 4)), "aligned")),
           "gnm_resolve_layout": ((dict(out_ptr=None), "out_ptr"), (dict(out_nodes=None), "out_nodes"), (dict(out_bases=None), "out_bases"),
                                  (dict(prefix_length=None), "prefix_length"), (dict(read_length=None), "read_length"))}
    for name, ok in calls.items():
        for change, word in common + own[name]:
            assert getattr(lib, name)(*dict(ok, **change).values()) == -1, (name, change)
            assert word in lib.gnm_last_error().decode(), (name, change, lib.gnm_last_error())
    assert all(v == 0 for v in rec) and all(v == 0 for v in buf)
