"""CPU: the walk-decision yardstick (tests/decision_reference.py) against cases written out by hand, train.DecisionMetrics, the
record's additivity, the hyper-parameter, the bindings of the entry point and its host-side argument checks.  Integers
throughout; the only floating-point figures are ratios of two integers, compared for equality with the same division."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import decision_reference as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _rec(succ, pred, calls=1):
    return np.array([succ[k] for k in D.COUNTERS] + [pred[k] for k in D.COUNTERS] + [calls], np.int64)


def _c(**kw):
    return dict(dict.fromkeys(D.COUNTERS, 0), **kw)


# ---- 1. the reference against hand-written cases ----------------------------------------------------------------------------------
def test_six_node_graph_written_out():
    """  eid  edge   score  y        node  successors (eid)      predecessors (eid)
          0   0->1    0.5   1         0    1:e0 2:e1 -> e1        3:e5            -> e5 (forced, y 1)
          1   0->2    2.0   0         1    3:e2      -> e2        0:e0 2:e6       -> e0
          2   1->3    1.0   1         2    3:e3 1:e6 -> e6        0:e1            -> e1 (forced, y 0)
          3   2->3   -1.0   1         3    4:e4 0:e5 -> e5        1:e2 2:e3       -> e2
          4   3->4    0.0   0         4    --  (4->4 is a self loop: dead)        3:e4 (e7 is a self loop) -> e4 (forced, y 0)
          5   3->0    3.0   1         5    --  isolated: dead                     -- dead
          6   2->1    0.25  0
          7   4->4    9.0   1"""
    src = [0, 0, 1, 2, 3, 3, 2, 4]
    dst = [1, 2, 3, 3, 4, 0, 1, 4]
    sc = [0.5, 2.0, 1.0, -1.0, 0.0, 3.0, 0.25, 9.0]
    y = [1, 0, 1, 1, 0, 1, 0, 1]
    bs, bp, rec = D.decisions(src, dst, 6, sc, y)
    assert bs.tolist() == [1, 2, 6, 5, -1, -1]
    assert bp.tolist() == [5, 0, 1, 2, 4, -1]
    # successors: node 1 forced (e2, y 1); branches at 0 (e0 is correct: solvable; chosen e1: wrong), 2 (e3 correct; chosen e6:
    # wrong), 3 (chosen e5: right).  predecessors: forced at 0 (ok), 2 (not), 4 (not); branches at 1 (e0: right), 3 (e2: right)
    want = _rec(_c(dead=2, forced=1, forced_ok=1, branch=3, branch_solvable=3, branch_ok=1),
                _c(dead=1, forced=3, forced_ok=1, branch=2, branch_solvable=2, branch_ok=2))
    assert rec.tolist() == want.tolist()
    assert D.summary(rec) == (3 / 5, 3 / 5, 1 / 3, 2 / 2)
    # without labels only dead / forced / branch / branch_nan move
    _, _, rec0 = D.decisions(src, dst, 6, sc, None)
    assert rec0.tolist() == _rec(_c(dead=2, forced=1, branch=3), _c(dead=1, forced=3, branch=2)).tolist()


def test_a_tie_goes_to_the_lowest_edge_id():
    # node 0 -> {1, 2, 3}: edges 2 and 0 share the top score (-0.0 == +0.0); node 3 <- {0, 1}: edges 2 and 3 tie at 1.5
    src, dst = [0, 1, 0, 1, 0], [1, 2, 3, 3, 2]
    sc = np.array([0.0, -1.0, -0.0, -0.0, -5.0], np.float32)
    bs, bp, _ = D.decisions(src, dst, 4, sc)
    assert bs.tolist() == [0, 3, -1, -1] and bp.tolist() == [-1, 0, 1, 2]
    sc[2], sc[3] = 1.5, 1.5
    bs, bp, _ = D.decisions(src, dst, 4, sc)
    assert bs[0] == 2 and bp[3] == 2


def test_nan_orders_below_every_number_and_a_nan_only_node_takes_the_lowest_id():
    # node 0: candidates e0 (NaN), e1 (-inf), e2 (NaN) -> -inf wins.  node 1: e3 (NaN), e4 (NaN) -> e3, counted in branch_nan
    src, dst = [0, 0, 0, 1, 1], [2, 3, 4, 2, 3]
    sc = np.array([NAN, -INF, NAN, NAN, NAN], np.float32)
    y = [1, 0, 1, 0, 1]
    bs, bp, rec = D.decisions(src, dst, 5, sc, y)
    assert bs.tolist() == [1, 3, -1, -1, -1]
    assert bp.tolist() == [-1, -1, 0, 1, 2]                      # node 2 <- e0 (NaN), e3 (NaN): e0; node 3 <- e1 (-inf), e4 (NaN): e1
    assert rec.tolist() == _rec(_c(dead=3, branch=2, branch_solvable=2, branch_nan=1),
                                _c(dead=2, forced=1, forced_ok=1, branch=2, branch_solvable=2, branch_ok=1, branch_nan=1)).tolist()


def test_a_self_loop_only_node_is_dead_and_duplicates_are_separate_candidates():
    # node 0: only 0->0 (twice).  node 1 -> 2 three times (e2, e3, e4): a branch of three; e3 and e4 tie at the top
    src, dst = [0, 0, 1, 1, 1], [0, 0, 2, 2, 2]
    sc, y = [5.0, 6.0, 1.0, 2.0, 2.0], [1, 1, 1, 0, 0]
    bs, bp, rec = D.decisions(src, dst, 3, sc, y)
    assert bs.tolist() == [-1, 3, -1] and bp.tolist() == [-1, -1, 3]
    assert rec.tolist() == _rec(_c(dead=2, branch=1, branch_solvable=1), _c(dead=2, branch=1, branch_solvable=1)).tolist()
    # labels other than 0 and 1 are not 1
    _, _, rec = D.decisions(src, dst, 3, sc, [1, 1, 0.5, NAN, 2.0])
    assert rec.tolist() == _rec(_c(dead=2, branch=1), _c(dead=2, branch=1)).tolist()


def test_empty_graphs():
    bs, bp, rec = D.decisions([], [], 3, [], [])
    assert bs.tolist() == [-1] * 3 and bp.tolist() == [-1] * 3 and rec.tolist() == _rec(_c(dead=3), _c(dead=3)).tolist()
    bs, bp, rec = D.decisions([], [], 0, [], None)
    assert bs.size == 0 and bp.size == 0 and rec.tolist() == [0] * 14 + [1]


# ---- 2. DecisionMetrics ----------------------------------------------------------------------------------------------------------------
def test_from_counts_ratios_and_nan_denominators():
    from gnnome_assembly_amd import train as T
    assert T.DECISION_COUNTERS == D.COUNTERS and T.DECISION_RECORD_WORDS == D.WORDS
    rec = _rec(_c(dead=2, forced=10, forced_ok=7, branch=8, branch_solvable=6, branch_ok=3, branch_nan=1),
               _c(dead=1, forced=5, forced_ok=5, branch=4, branch_solvable=4, branch_ok=4), calls=3)
    m = T.DecisionMetrics.from_counts(rec)
    assert (m.succ.branch_accuracy, m.succ.solvable_accuracy, m.succ.forced_accuracy) == (3 / 8, 3 / 6, 7 / 10)
    assert (m.pred.branch_accuracy, m.pred.solvable_accuracy, m.pred.forced_accuracy) == (1.0, 1.0, 1.0)
    assert (m.branch_accuracy, m.solvable_accuracy, m.forced_accuracy) == (7 / 12, 7 / 10, 12 / 15)
    assert m.calls == 3 and m.pooled.dead == 3 and m.pooled.branch_nan == 1 and m.succ.branch == 8 and m.pred.forced == 5
    assert m.summary() == (7 / 12, 7 / 10, 3 / 8, 1.0) == D.summary(rec)
    # denominators of 0: NaN, never an exception and never 0
    z = T.DecisionMetrics.from_counts(_rec(_c(dead=4), _c(forced=2, forced_ok=1), calls=1))
    assert all(math.isnan(v) for v in (z.succ.branch_accuracy, z.succ.solvable_accuracy, z.succ.forced_accuracy,
                                        z.pred.branch_accuracy, z.pred.solvable_accuracy, z.branch_accuracy, z.solvable_accuracy))
    assert z.pred.forced_accuracy == 0.5 == z.forced_accuracy and all(math.isnan(v) for v in z.summary())
    # branches with no correct candidate: accuracy 0 over the branches, NaN over the solvable ones
    u = T.DecisionMetrics.from_counts(_rec(_c(branch=3), _c()))
    assert u.branch_accuracy == 0.0 and math.isnan(u.solvable_accuracy)
    assert T.DecisionMetrics.from_counts(rec[:-1]).calls == 0                      # the 14 counters alone
    for bad in (rec[:5], -rec):
        with pytest.raises(ValueError):
            T.DecisionMetrics.from_counts(bad)
    assert {"DecisionStats", "DecisionMetrics"} <= set(T.__all__)


def test_records_add():
    """The record of two graphs is the sum of their records -- of the yardstick's, and of DecisionStats buffers on the CPU."""
    from gnnome_assembly_amd import train as T
    rng = np.random.default_rng(0)
    recs = []
    for n, e in ((12, 40), (9, 30)):
        src, dst = rng.integers(0, n, e), rng.integers(0, n, e)
        recs.append(D.decisions(src, dst, n, rng.integers(0, 4, e).astype(np.float32), rng.integers(0, 2, e))[2])
    # one graph made of both (node ids of the second shifted): the counters are per node, so they add
    a, b = T.DecisionStats("cpu"), T.DecisionStats("cpu")
    assert a.buf.dtype == torch.int64 and a.buf.numel() == D.WORDS and int(a.buf.abs().sum()) == 0
    a.buf += torch.from_numpy(recs[0])
    b.buf += torch.from_numpy(recs[1])
    a.buf += b.buf
    m = a.all_reduce_().read()                                                      # no process group: all_reduce_ is the identity
    tot = recs[0] + recs[1]
    assert m.calls == 2 and [getattr(m.succ, k) for k in D.COUNTERS] == tot[:7].tolist()
    assert [getattr(m.pred, k) for k in D.COUNTERS] == tot[7:14].tolist() and m.summary() == D.summary(tot)
    assert [getattr(m.pooled, k) for k in D.COUNTERS] == (tot[:7] + tot[7:14]).tolist()
    assert int(a.zero_().buf.abs().sum()) == 0


# ---- 3. the hyper-parameter -------------------------------------------------------------------------------------------------------------
def test_hyperparameter_default_and_environment(monkeypatch):
    from gnnome_assembly_amd import train as T
    monkeypatch.delenv("GNM_DECISION_METRICS", raising=False)
    assert T.get_hyperparameters()["decision_metrics"] is False
    monkeypatch.setenv("GNM_DECISION_METRICS", "1")
    assert T.get_hyperparameters()["decision_metrics"] is True
    monkeypatch.setenv("GNM_DECISION_METRICS", "0")
    assert T.get_hyperparameters()["decision_metrics"] is False
    assert T.History().decision_valid == []


@pytest.fixture(scope="module")
def samples():
    from loop_common import mix_sample
    torch.set_num_threads(1)
    return [mix_sample(60, 0), mix_sample(50, 1)], [mix_sample(40, 100)]


def _train(samples, tmp_path, name, **hp):
    from gnnome_assembly_amd import train as T
    from loop_common import oracle_model_factory
    hooks = {"model_factory": oracle_model_factory,
             "criterion_factory": lambda pw: torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw]))}
    wd = tmp_path / name
    wd.mkdir()
    return T.train(samples[0], samples[1], out=name, workdir=str(wd), verbose=False, hooks=hooks,
                   hyperparameters=dict(dict(num_epochs=2, dim_latent=32, num_gnn_layers=1, lr=1e-3, seed=0), **hp))


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_a_value_that_is_not_a_bool_is_refused(samples, tmp_path, bad):
    with pytest.raises(ValueError, match="decision_metrics"):
        _train(samples, tmp_path, "bad", decision_metrics=bad)


def test_on_is_refused_up_front_for_samples_on_the_cpu(samples, tmp_path):
    """The count is a kernel: with the CPU stand-in model the run is refused before the first step, not at the first validation."""
    with pytest.raises(ValueError, match="decision_metrics=True.*HIP device"):
        _train(samples, tmp_path, "cpu_on", decision_metrics=True)
    assert not (tmp_path / "cpu_on" / "checkpoints").exists()


def test_off_leaves_the_history_field_empty(samples, tmp_path, monkeypatch):
    monkeypatch.delenv("GNM_DECISION_METRICS", raising=False)
    _, _, h0 = _train(samples, tmp_path, "default")
    _, _, h1 = _train(samples, tmp_path, "off", decision_metrics=False)
    assert h0.decision_valid == [] and h1.decision_valid == [] and h0 == h1 and len(h0.loss_valid) == 2


# ---- 4. the entry point ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def test_the_library_binds_the_entry_point_at_abi_7(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib, decode, engine
    assert "gnm_decision.hip" in ge.SOURCES
    assert getattr(lib, "gnm_decision_stats").argtypes == _lib.SIGNATURES["gnm_decision_stats"][1]
    assert lib.gnm_abi_version() == 7 == _lib.ABI_VERSION
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    assert "gnm_decision_record" in hdr and "int gnm_decision_stats(" in hdr and "#define GNM_ABI_VERSION 7" in hdr
    assert engine.DECISION_RECORD_WORDS == D.WORDS and engine.DECISION_COUNTERS == D.COUNTERS
    assert "decision_table" in decode.__all__


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Host-side returns: no device is touched (the checks run before the grid is even sized)."""
    rec = (C.c_int64 * D.WORDS)()
    buf = (C.c_int32 * 16)()
    sc = (C.c_float * 8)()
    p = lambda a: C.c_void_p(C.addressof(a))                                     # noqa: E731
    b, s, r = p(buf), p(sc), p(rec)
    ok = dict(n=4, E=8, perm=b, isrc=b, idst=b, in_ptr=b, out_ptr=b, out_pos=b, out_dst=b, nperm=None, scores=s, y=s, record=r,
              best_succ=None, best_pred=None, stream=None)
    for change, word in ((dict(n=-1), "n = -1"), (dict(E=-1), "E = -1"), (dict(n=2 ** 31 - 1), "2^31"), (dict(E=2 ** 31 - 1), "2^31"),
                         (dict(record=None), "record"), (dict(record=C.c_void_p(C.addressof(rec) + 4)), "aligned"),
                         (dict(in_ptr=None), "in_ptr"), (dict(out_ptr=None), "out_ptr"), (dict(perm=None), "perm"),
                         (dict(isrc=None), "isrc"), (dict(out_pos=None), "out_pos"), (dict(out_dst=None), "out_dst"),
                         (dict(scores=None), "scores"), (dict(n=0, E=0, record=None), "record")):
        assert lib.gnm_decision_stats(*dict(ok, **change).values()) == -1, change
        assert word in lib.gnm_last_error().decode(), (change, lib.gnm_last_error())
    assert all(v == 0 for v in rec)
