"""CPU: the greedy-path-cover yardstick (tests/cover_reference.py) against itself -- the round-synchronous definition at its fixed
point equals the sequential sorted pass, its first round equals the best-overlap links, its fixed point is maximal -- and against
cases written out by hand; the bindings of the two entry points and their host-side argument checks; the refusals of
decode.greedy_cover_contigs, decode.infer_contigs and of the hyper-parameter "assembly_decoder".  Integers throughout, compared
for equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bog_reference as B
import cover_reference as R
import decision_reference as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---- 1. the yardstick ----------------------------------------------------------------------------------------------------------------
def test_the_second_round_links_what_the_first_left_free():
    """e0 0->1 at 3, e1 0->2 at 2, e2 3->1 at 1.  Round 1: 0 and 1 agree on e0; 3 proposes e2 to node 1, which prefers e0; node 2's
    best in-edge e1 comes from node 0, which prefers e0.  Round 2: nothing is left for 3 (node 1 is taken) nor for 2 (node 0 is)."""
    ms, mp, rl = R.rounds([0, 0, 3], [1, 2, 1], 4, [3, 2, 1])
    assert ms.tolist() == [0, -1, -1, -1] and mp.tolist() == [-1, 0, -1, -1] and rl == [1, 0]
    # with e3 3->2 at 0.5 the second round links it: both ends lost their first choice
    ms, mp, rl = R.rounds([0, 0, 3, 3], [1, 2, 1, 2], 4, [3, 2, 1, 0.5])
    assert ms.tolist() == [0, -1, -1, 3] and mp.tolist() == [-1, 0, 3, -1] and rl == [1, 1, 0]
    assert R.rounds([0, 0, 3, 3], [1, 2, 1, 2], 4, [3, 2, 1, 0.5], max_rounds=1)[2] == [1]
    # the cut refuses e3: the cover stops after e0
    ms, mp, rl = R.rounds([0, 0, 3, 3], [1, 2, 1, 2], 4, [3, 2, 1, 0.5], min_logit=1.0)
    assert ms.tolist() == [0, -1, -1, -1] and rl == [1, 0]


def test_self_loops_nan_and_ties():
    """e0 0->0 (a self loop, score 9) and e1 0->1 (NaN) are no candidates; e2 and e3 are copies of 0->1 at +0 and -0: they tie and
    the lower id wins; e4 1->0 at -inf is a candidate at min_logit = -inf and closes a two-cycle."""
    src, dst, sc = [0, 0, 0, 0, 1], [0, 1, 1, 1, 0], [9, NAN, 0.0, -0.0, -INF]
    assert R.candidates(src, dst, 2, sc) == [2, 3, 4] and R.candidates(src, dst, 2, sc, min_logit=0.0) == [2, 3]
    ms, mp, rl = R.rounds(src, dst, 2, sc)
    assert ms.tolist() == [2, 4] and mp.tolist() == [4, 2] and rl == [2, 0]
    assert [a.tolist() for a in R.greedy(src, dst, 2, sc)] == [[2, 4], [4, 2]]
    r = R.contigs(src, dst, 2, sc, [1, 2, 3, 4, 5], [10, 20])
    assert r["walk_nodes"].tolist() == [0, 1] and r["walk_edges"].tolist() == [-1, 2] and r["record"].tolist() == [1, 1, 1, 0, 0, 2, 1, 1]
    assert r["rounds"] == 2 and r["converged"] is True


def test_the_adversarial_chain_takes_one_round_per_link():
    src, dst, n, sc, y, pl, rl = R.adversarial_chain(50)
    ms, mp, links = R.rounds(src, dst, n, sc)
    assert links == [1] * 50 + [0] and n == 101
    assert [a.tolist() for a in R.greedy(src, dst, n, sc)] == [ms.tolist(), mp.tolist()]
    ms10, mp10, links10 = R.rounds(src, dst, n, sc, max_rounds=10)
    assert links10 == [1] * 10 and int((ms10 >= 0).sum()) == 10 and not R.is_maximal(src, dst, n, sc, ms10, mp10)


@pytest.fixture(scope="module", params=[(21, -INF), (21, 1.0), (22, 0.0), (23, -INF)])
def mixed(request):
    seed, ml = request.param
    rng = np.random.default_rng(seed)
    case = R.mix(seed, rng.integers(1, 30, 40).tolist(), rng.integers(2, 12, 8).tolist(), distractors=900)
    return case, ml, R.rounds(*case[:4], min_logit=ml)


def test_the_fixed_point_of_the_rounds_is_the_sequential_greedy_cover(mixed):
    (src, dst, n, sc, *_), ml, (ms, mp, rl) = mixed
    gs, gp = R.greedy(src, dst, n, sc, ml)
    print("rounds", len(rl), "links per round", rl)
    assert np.array_equal(ms, gs) and np.array_equal(mp, gp)
    assert rl[-1] == 0 and all(v > 0 for v in rl[:-1]) and len(rl) >= 3 and sum(rl) == int((ms >= 0).sum()) == int((mp >= 0).sum())
    # the tables are mutual: msucc[u] = k <=> mpred[dst k] = k
    for u in range(n):
        if ms[u] >= 0:
            assert src[ms[u]] == u and mp[dst[ms[u]]] == ms[u]
    # one more round on the fixed point changes nothing
    again = R.rounds(src, dst, n, sc, ml, max_rounds=len(rl) + 1)
    assert np.array_equal(again[0], ms) and again[2] == rl


def test_round_one_is_the_best_overlap_graph(mixed):
    (src, dst, n, sc, *_), ml, _ = mixed
    ms, mp, rl = R.rounds(src, dst, n, sc, ml, max_rounds=1)
    bs, bp, _ = D.decisions(src, dst, n, sc)
    nxt, prv, pedge, _ = B.links(src, dst, n, bs, bp, sc, ml)
    assert R.next_prev(src, dst, ms, mp) == (nxt, prv) and mp.tolist() == pedge and rl == [sum(v >= 0 for v in nxt)]


def test_the_fixed_point_is_maximal(mixed):
    (src, dst, n, sc, *_), ml, (ms, mp, rl) = mixed
    assert R.is_maximal(src, dst, n, sc, ms, mp, ml)
    first = R.rounds(src, dst, n, sc, ml, max_rounds=1)
    assert not R.is_maximal(src, dst, n, sc, first[0], first[1], ml)


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_greedy_cover_contigs_refuses_a_cpu_graph_and_bad_round_counts():
    from gnnome_assembly_amd import AssemblyGraph, decode
    from gnnome_assembly_amd._lib import GnmError
    g = AssemblyGraph(np.array([0, 1], np.int32), np.array([1, 2], np.int32), 3)
    args = (g, torch.zeros(2), torch.ones(2, dtype=torch.int64), torch.ones(3, dtype=torch.int64))
    with pytest.raises(GnmError, match="HIP device"):
        decode.greedy_cover_contigs(*args)
    assert "greedy_cover_contigs" in decode.__all__ and decode.COVER_CHECK_EVERY >= 1
    with pytest.raises(GnmError):
        from gnnome_assembly_amd import engine
        engine.cover_rounds(g.index(), torch.zeros(2), torch.zeros(1, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                            torch.zeros(3, dtype=torch.int32), torch.zeros(128, dtype=torch.uint8))


def test_infer_contigs_knows_the_decoder_and_refuses_others():
    from gnnome_assembly_amd import decode
    with pytest.raises(ValueError, match="greedy_cover"):
        decode.infer_contigs(None, None, None, None, None, None, decoder="cover")


def test_hyperparameter_default_environment_and_validation(monkeypatch, tmp_path):
    from gnnome_assembly_amd import train as T
    monkeypatch.delenv("GNM_ASSEMBLY_DECODER", raising=False)
    assert T.get_hyperparameters()["assembly_decoder"] == "best_overlap"
    monkeypatch.setenv("GNM_ASSEMBLY_DECODER", "greedy_cover")
    assert T.get_hyperparameters()["assembly_decoder"] == "greedy_cover"
    monkeypatch.delenv("GNM_ASSEMBLY_DECODER")
    assert T.ASSEMBLY_DECODERS == ("best_overlap", "greedy_cover")
    assert T.AssemblyStats("cpu", decoder="greedy_cover").decoder == "greedy_cover" and T.AssemblyStats("cpu").decoder == "best_overlap"
    with pytest.raises(ValueError, match="decoder"):
        T.AssemblyStats("cpu", decoder="greedy")
    from loop_common import mix_sample, oracle_model_factory
    torch.set_num_threads(1)
    hooks = {"model_factory": oracle_model_factory,
             "criterion_factory": lambda pw: torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw]))}
    for bad in ("greedy", 1, None):
        with pytest.raises(ValueError, match="assembly_decoder"):
            T.train([mix_sample(40, 0)], [mix_sample(30, 1)], out="bad", workdir=str(tmp_path), verbose=False, hooks=hooks,
                    hyperparameters=dict(num_epochs=1, dim_latent=32, num_gnn_layers=1, assembly_decoder=bad))
    assert not (tmp_path / "checkpoints").exists()


# ---- 3. the entry points -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def test_the_library_binds_the_entry_points_at_abi_7(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib, engine
    assert "gnm_cover.hip" in ge.SOURCES
    for name in ("gnm_cover_workspace_bytes", "gnm_cover_rounds"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.gnm_abi_version() == 7 == _lib.ABI_VERSION
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    assert "int gnm_cover_rounds(" in hdr and "size_t gnm_cover_workspace_bytes(" in hdr and "#define GNM_ABI_VERSION 7" in hdr
    assert "gnm_cover.hip" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    # the key is shared, not copied
    csrc = os.path.join(REPO, "gnnome_assembly_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if "unsigned dec_key_(float" in open(os.path.join(csrc, f)).read()]
    assert defs == ["gnm_key.h"]
    for f in ("gnm_decision.hip", "gnm_cover.hip"):
        assert '#include "gnm_key.h"' in open(os.path.join(csrc, f)).read()
    # 24 bytes per node: two int32 state words and two 8-byte proposals
    assert lib.gnm_cover_workspace_bytes(0) == 0 == lib.gnm_cover_workspace_bytes(-1) == lib.gnm_cover_workspace_bytes(2 ** 31 - 1)
    for n in (1, 5, 1024, 1025, 68000):
        assert 24 * n <= lib.gnm_cover_workspace_bytes(n) <= 24 * n + 16 * 4 and \
            engine.cover_workspace_bytes(n) == lib.gnm_cover_workspace_bytes(n), n


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Host-side returns: no device is touched (the checks run before the grid is even sized)."""
    n, E = 4, 8
    buf = (C.c_int64 * 16)()
    links = (C.c_int64 * 4)()
    ws = (C.c_int64 * 1024)()
    p = lambda a: C.c_void_p(C.addressof(a))                                     # noqa: E731
    b, w = p(buf), p(ws)
    need = lib.gnm_cover_workspace_bytes(n)
    assert 0 < need <= 8 * 1024 and C.addressof(ws) % 16 in (0, 8)
    if C.addressof(ws) % 16:
        w = C.c_void_p(C.addressof(ws) + 8)
    ok = dict(n=n, E=E, perm=b, isrc=b, in_ptr=b, out_ptr=b, out_pos=b, out_dst=b, nperm=None, scores=b, min_logit=0.0, first_round=0,
              rounds=4, round_links=p(links), link_succ=b, link_pred=b, ws=w, ws_bytes=need, stream=None)
    for change, word in ((dict(n=-1), "n = -1"), (dict(E=-1), "E = -1"), (dict(n=2 ** 31 - 1), "2^31"), (dict(E=2 ** 31 - 1), "2^31"),
                         (dict(rounds=-1), "rounds = -1"), (dict(first_round=-1), "first_round = -1"), (dict(rounds=2 ** 31), "rounds"),
                         (dict(round_links=None), "round_links"), (dict(round_links=C.c_void_p(C.addressof(links) + 4)), "aligned"),
                         (dict(in_ptr=None), "in_ptr"), (dict(out_ptr=None), "out_ptr"), (dict(link_succ=None), "link_succ"),
                         (dict(link_pred=None), "link_pred"), (dict(perm=None), "perm"), (dict(isrc=None), "isrc"),
                         (dict(out_pos=None), "out_pos"), (dict(out_dst=None), "out_dst"), (dict(scores=None), "scores"),
                         (dict(ws=None), "workspace"), (dict(ws_bytes=need - 1), "workspace"),
                         (dict(ws=C.c_void_p(w.value + 4)), "workspace"), (dict(n=0, E=0, rounds=1, round_links=None), "round_links")):
        assert lib.gnm_cover_rounds(*dict(ok, **change).values()) == -1, change
        assert word in lib.gnm_last_error().decode(), (change, lib.gnm_last_error())
    assert all(v == 0 for v in links) and all(v == 0 for v in buf) and all(v == 0 for v in ws)
    assert lib.gnm_cover_rounds(*dict(ok, n=0, E=0, rounds=0, round_links=None, ws=None, ws_bytes=0).values()) == 0   # nothing to do
