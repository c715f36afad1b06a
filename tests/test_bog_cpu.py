"""CPU: the best-overlap-contig yardstick (tests/bog_reference.py) against cases written out by hand, decode.resolve_strands,
the refusals of decode.best_overlap_contigs and of the hyper-parameter "assembly_metrics", the bindings of the two entry points
and their host-side argument checks.  Integers throughout, compared for equality."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import bog_reference as B

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def _rec(**kw):
    return [dict(dict.fromkeys(B.COUNTERS, 0), calls=1, **kw)[k] for k in B.COUNTERS]


def _is(r, ptr, nodes, edges, bases, wrong, **rec):
    assert r["contig_ptr"].tolist() == ptr and r["walk_nodes"].tolist() == nodes and r["walk_edges"].tolist() == edges
    assert r["bases"].tolist() == bases and r["wrong"].tolist() == wrong
    assert r["record"].tolist() == _rec(**rec), (r["record"].tolist(), _rec(**rec))


# ---- 1. the reference against hand-written cases ----------------------------------------------------------------------------------
def test_a_path_with_a_distractor():
    """e0 0->1, e1 1->2, e2 2->3 at score 2; e3 0->2 at score 1 loses at both ends.  One contig 0-1-2-3:
    bases = 10 + 20 + 30 + read_length[3] = 460; e1 has y == 0: one wrong link."""
    src, dst = [0, 1, 2, 0], [1, 2, 3, 2]
    r = B.contigs(src, dst, 4, [2, 2, 2, 1], [10, 20, 30, 5], [100, 200, 300, 400], y=[1, 0, 1, 1])
    _is(r, [0, 4], [0, 1, 2, 3], [-1, 0, 1, 2], [460], [1], contigs=1, links=3, wrong_links=1, multi_nodes=4, multi_contigs=1)


def test_without_labels_nothing_is_wrong():
    r = B.contigs([0, 1, 2, 0], [1, 2, 3, 2], 4, [2, 2, 2, 1], [10, 20, 30, 5], [100, 200, 300, 400], y=None)
    _is(r, [0, 4], [0, 1, 2, 3], [-1, 0, 1, 2], [460], [0], contigs=1, links=3, multi_nodes=4, multi_contigs=1)


def test_a_two_cycle_is_cut_at_its_smaller_node():
    """e0 1->2 and e1 2->1 are both mutual-best; node 0 has no edge.  m = 1 loses its prev (e1) and node 2 its next: 1 -> 2 by e0."""
    r = B.contigs([1, 2], [2, 1], 3, [0.5, 0.25], [7, 9], [10, 20, 30], y=[0, 1])
    _is(r, [0, 1, 3], [0, 1, 2], [-1, -1, 0], [10, 7 + 30], [0, 1], contigs=2, links=1, cycles_cut=1, wrong_links=1, multi_nodes=2,
        multi_contigs=1)


def test_a_three_cycle_with_a_tail_feeding_into_it():
    """Cycle 1 -> 2 -> 3 -> 1 (e0, e1, e2 at score 3), tail e3 0 -> 1 at score 1: e3 is node 0's best successor but not node 1's
    best predecessor, so it is no link.  The cycle is cut at 1: e2 goes, 1 -> 2 -> 3 stays."""
    r = B.contigs([1, 2, 3, 0], [2, 3, 1, 1], 4, [3, 3, 3, 1], [5, 6, 7, 8], [100, 200, 300, 400], y=[1, 1, 1, 1])
    _is(r, [0, 1, 4], [0, 1, 2, 3], [-1, -1, 0, 1], [100, 5 + 6 + 400], [0, 0], contigs=2, links=2, cycles_cut=1, multi_nodes=3,
        multi_contigs=1)


def test_a_self_loop_is_no_link_and_no_candidate():
    """e0 0->0 at score 9 is no candidate, so e1 0->1 at score 1 is mutual-best."""
    r = B.contigs([0, 0], [0, 1], 2, [9, 1], [50, 60], [100, 200], y=[1, 1])
    _is(r, [0, 2], [0, 1], [-1, 1], [260], [0], contigs=1, links=1, multi_nodes=2, multi_contigs=1)


def test_duplicate_edges_give_one_link_by_the_lowest_id_among_the_top_scores():
    """Three copies of 0 -> 1: e0 at 0.5, e1 and e2 at 1.0 -> e1 on both sides."""
    r = B.contigs([0, 0, 0], [1, 1, 1], 2, [0.5, 1.0, 1.0], [11, 22, 33], [100, 200], y=[1, 0, 1])
    _is(r, [0, 2], [0, 1], [-1, 1], [222], [1], contigs=1, links=1, wrong_links=1, multi_nodes=2, multi_contigs=1)


def test_a_nan_scored_best_edge_is_dropped():
    """The only edge is every node's best, but NaN: counted in dropped, two contigs of one node."""
    r = B.contigs([0], [1], 2, [NAN], [11], [100, 200], y=[1])
    _is(r, [0, 1, 2], [0, 1], [-1, -1], [100, 200], [0, 0], contigs=2, dropped=1)


def test_the_min_logit_cut_keeps_an_equal_score():
    src, dst, sc, pl, rl = [0, 1], [1, 2], [3.0, 0.5], [10, 20], [100, 200, 300]
    r = B.contigs(src, dst, 3, sc, pl, rl, y=[1, 1], min_logit=1.0)
    _is(r, [0, 2, 3], [0, 1, 2], [-1, 0, -1], [210, 300], [0, 0], contigs=2, links=1, dropped=1, multi_nodes=2, multi_contigs=1)
    r = B.contigs(src, dst, 3, sc, pl, rl, y=[1, 1], min_logit=0.5)
    _is(r, [0, 3], [0, 1, 2], [-1, 0, 1], [330], [0], contigs=1, links=2, multi_nodes=3, multi_contigs=1)
    r = B.contigs(src, dst, 3, sc, pl, rl, y=[1, 1], min_logit=INF)
    _is(r, [0, 1, 2, 3], [0, 1, 2], [-1, -1, -1], [100, 200, 300], [0, 0, 0], contigs=3, dropped=2)


def test_table_entries_outside_the_range_drop_the_candidate():
    src, dst = [0, 1], [1, 2]
    r = B.contigs_from_tables(src, dst, 3, [0, 99, -1], [-1, 0, -5], [1, 1], [10, 20], [100, 200, 300])
    _is(r, [0, 2, 3], [0, 1, 2], [-1, 0, -1], [210, 300], [0, 0], contigs=2, links=1, multi_nodes=2, multi_contigs=1)
    r = B.contigs_from_tables([0, 7], [1, 2], 3, [0, 1, -1], [-1, 0, 1], [1, 1], [10, 20], [100, 200, 300])     # src[1] outside
    assert r["record"].tolist() == _rec(contigs=2, links=1, multi_nodes=2, multi_contigs=1)


def test_empty_inputs_and_n50():
    r = B.contigs([], [], 5, [], [], [3, 1, 4, 1, 5])
    _is(r, [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4], [-1] * 5, [3, 1, 4, 1, 5], [0] * 5, contigs=5)
    r = B.contigs([], [], 0, [], [], [])
    _is(r, [0], [], [], [], [])
    from gnnome_assembly_amd import decode
    for lens, want in (([], 0), ([7], 7), ([2, 2, 2, 3, 3, 4, 8, 8], 8), ([1, 2, 3, 4], 3), ([5, 5], 5), ([10, 1, 1], 10)):
        assert B.n50(lens) == want == decode.n50(lens), lens
    s = B.summary([dict(bases=[100, 50, 7], contig_ptr=np.array([0, 25, 45, 50]), record=np.array(_rec(links=47, wrong_links=4)))],
                  min_nodes=20)
    assert s == (2, 100, 100, 4 / 47)
    assert math.isnan(B.summary([])[3]) and B.summary([])[:3] == (0, 0, 0)


# ---- 2. resolve_strands ------------------------------------------------------------------------------------------------------------
def _bog(src, dst, n, pl, rl):
    """A decode.BogContigs on the CPU from the yardstick's result for all-equal scores (every edge given is mutual-best)."""
    from gnnome_assembly_amd import decode
    r = B.contigs(src, dst, n, np.ones(len(src), np.float32), pl, rl)
    t = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt)           # noqa: E731
    st = decode.BogStats(*r["record"].tolist())
    return decode.BogContigs(t(r["contig_ptr"], torch.int32), t(r["walk_nodes"], torch.int32), t(r["walk_edges"], torch.int32),
                             t(r["bases"], torch.int64), t(r["wrong"], torch.int32), st, t(pl, torch.int64), t(rl, torch.int64))


def test_resolve_strands_with_a_read_on_two_paths():
    """Nodes 2i / 2i+1 are the strands of read i.  Paths: A = 0-2-4-6 (reads 0..3, 436 bases), B = 7-5-3-9-11 (reads 3, 2, 1, 4, 5;
    197 bases), D = 8-10-12 (reads 4, 5, 6; 173 bases); nodes 1 and 13 are alone.  A comes first and takes reads 0..3, so of B only
    the piece 9-11 is left."""
    src = [0, 2, 4, 7, 5, 3, 9, 8, 10]
    dst = [2, 4, 6, 5, 3, 9, 11, 10, 12]
    pl = [100, 110, 120, 20, 21, 22, 23, 30, 31]
    rl = [100 + v for v in range(14)]
    c = _bog(src, dst, 14, pl, rl)
    assert c.walks() == [[0, 2, 4, 6], [1], [7, 5, 3, 9, 11], [8, 10, 12], [13]] and c.walks(min_nodes=4) == [[0, 2, 4, 6], [7, 5, 3, 9, 11]]
    assert c.host()["bases"].tolist() == [436, 101, 197, 173, 113] and c.longest() == 436 and c.longest(min_nodes=5) == 197
    assert c.n50() == 197 and c.n50(min_nodes=4) == 436 and c.n50(min_nodes=5) == 197 and c.n50(min_nodes=6) == 0
    assert len(c) == 5 and c.stats.contigs == 5 and c.stats.links == 9 and c.num_nodes().tolist() == [4, 1, 5, 3, 1]
    from gnnome_assembly_amd import decode
    # threshold 2: 9-11 is kept (23 + read_length[11]) and takes reads 4, 5; of D only node 12 is left: below the threshold
    r = decode.resolve_strands(c, len_threshold=2)
    assert r.walks == [[0, 2, 4, 6], [9, 11]] and r.bases == [436, 23 + 111]
    # threshold 3: 9-11 falls below it and is dropped WITHOUT marking reads 4, 5 -- so D is kept whole
    r = decode.resolve_strands(c, len_threshold=3)
    assert r.walks == [[0, 2, 4, 6], [8, 10, 12]] and r.bases == [436, 173]
    assert decode.resolve_strands(c, len_threshold=4).walks == [[0, 2, 4, 6]]
    assert decode.resolve_strands(c, len_threshold=5).walks == [[7, 5, 3, 9, 11]]     # A is too short now, so B keeps its reads
    assert decode.resolve_strands(c, len_threshold=6).walks == []


def test_resolve_strands_splits_a_path_at_a_taken_read_and_within_one_path():
    """X = 0-2-4 (longest), Y = 6-8-5-10-12: node 5 is read 2's other strand, so Y falls into 6-8 and 10-12; the link into and out
    of node 5 counts for neither piece."""
    from gnnome_assembly_amd import decode
    src, dst = [0, 2, 6, 8, 5, 10], [2, 4, 8, 5, 10, 12]
    pl = [1000, 1000, 1, 2, 3, 4]
    rl = [10 * (v + 1) for v in range(13)]
    c = _bog(src, dst, 13, pl, rl)
    r = decode.resolve_strands(c, len_threshold=2)
    assert r.walks == [[0, 2, 4], [6, 8], [10, 12]] and r.bases == [2050, 1 + 90, 4 + 130]
    assert decode.resolve_strands(c, len_threshold=3).walks == [[0, 2, 4]]
    # both strands of reads 0 and 1 on ONE path 0-2-1-3: the piece 0-2 ends at node 1; kept (threshold 2) it takes reads 0, 1 and
    # nodes 1, 3 are skipped; dropped (threshold 3) node 1 starts the next piece 1-3, which is too short as well
    c = _bog([0, 2, 1], [2, 1, 3], 4, [5, 6, 7], [10, 20, 30, 40])
    r = decode.resolve_strands(c, len_threshold=2)
    assert r.walks == [[0, 2]] and r.bases == [5 + 30]
    assert decode.resolve_strands(c, len_threshold=3).walks == []
    assert decode.resolve_strands(c, len_threshold=1).walks == [[0, 2]]


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_best_overlap_contigs_refuses_a_cpu_graph():
    from gnnome_assembly_amd import AssemblyGraph, decode
    from gnnome_assembly_amd._lib import GnmError
    g = AssemblyGraph(np.array([0, 1], np.int32), np.array([1, 2], np.int32), 3)
    with pytest.raises(GnmError, match="HIP device"):
        decode.best_overlap_contigs(g, torch.zeros(2), torch.ones(2, dtype=torch.int64), torch.ones(3, dtype=torch.int64))
    assert {"best_overlap_contigs", "BogContigs", "resolve_strands"} <= set(decode.__all__)


def test_infer_contigs_refuses_an_unknown_decoder():
    from gnnome_assembly_amd import decode
    with pytest.raises(ValueError, match="decoder"):
        decode.infer_contigs(None, None, None, None, None, None, decoder="best")


def test_hyperparameter_default_and_environment(monkeypatch):
    from gnnome_assembly_amd import train as T
    monkeypatch.delenv("GNM_ASSEMBLY_METRICS", raising=False)
    assert T.get_hyperparameters()["assembly_metrics"] is False
    monkeypatch.setenv("GNM_ASSEMBLY_METRICS", "1")
    assert T.get_hyperparameters()["assembly_metrics"] is True
    monkeypatch.setenv("GNM_ASSEMBLY_METRICS", "0")
    assert T.get_hyperparameters()["assembly_metrics"] is False
    assert T.History().assembly_valid == [] and "AssemblyStats" in T.__all__ and T.ASSEMBLY_MIN_NODES == 20


def _samples(lengths=True):
    from loop_common import mix_sample
    torch.set_num_threads(1)
    out = [mix_sample(60, 0), mix_sample(50, 1)], [mix_sample(40, 100)]
    if lengths:
        for s in out[1]:
            s.graph.edata["prefix_length"] = torch.ones(s.graph.num_edges(), dtype=torch.int64)
            s.graph.ndata["read_length"] = torch.ones(s.graph.num_nodes(), dtype=torch.int64)
    return out


def _train(samples, tmp_path, name, **hp):
    from gnnome_assembly_amd import train as T
    from loop_common import oracle_model_factory
    hooks = {"model_factory": oracle_model_factory,
             "criterion_factory": lambda pw: torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw]))}
    wd = tmp_path / name
    wd.mkdir()
    return T.train(samples[0], samples[1], out=name, workdir=str(wd), verbose=False, hooks=hooks,
                   hyperparameters=dict(dict(num_epochs=2, dim_latent=32, num_gnn_layers=1, lr=1e-3, seed=0), **hp))


@pytest.mark.parametrize("bad", [1, "yes", None])
def test_a_value_that_is_not_a_bool_is_refused(tmp_path, bad):
    with pytest.raises(ValueError, match="assembly_metrics"):
        _train(_samples(), tmp_path, "bad", assembly_metrics=bad)


def test_on_is_refused_up_front(tmp_path):
    """Before the first step: on the CPU (the decode is kernels), for a validation sample without either array, and with
    batch_size_eval > 1."""
    with pytest.raises(ValueError, match="assembly_metrics=True.*HIP device"):
        _train(_samples(), tmp_path, "cpu_on", assembly_metrics=True)
    with pytest.raises(ValueError, match="assembly_metrics=True.*prefix_length"):
        _train(_samples(lengths=False), tmp_path, "no_lengths", assembly_metrics=True)
    s = _samples()
    del s[1][0].graph.ndata["read_length"]
    with pytest.raises(ValueError, match="assembly_metrics=True.*read_length"):
        _train(s, tmp_path, "no_read_length", assembly_metrics=True)
    with pytest.raises(ValueError, match="assembly_metrics=True.*batch_size_eval"):
        _train(_samples(), tmp_path, "batches", assembly_metrics=True, batch_size_eval=2)
    for name in ("cpu_on", "no_lengths", "no_read_length", "batches"):
        assert not (tmp_path / name / "checkpoints").exists()


def test_off_leaves_the_history_field_empty(tmp_path, monkeypatch):
    monkeypatch.delenv("GNM_ASSEMBLY_METRICS", raising=False)
    _, _, h0 = _train(_samples(lengths=False), tmp_path, "default")
    _, _, h1 = _train(_samples(lengths=False), tmp_path, "off", assembly_metrics=False)
    assert h0.assembly_valid == [] and h1.assembly_valid == [] and h0 == h1 and len(h0.loss_valid) == 2


# ---- 4. the entry points -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def test_the_library_binds_the_entry_points_at_abi_7(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib, decode, engine
    assert "gnm_bog.hip" in ge.SOURCES
    for name in ("gnm_bog_workspace_bytes", "gnm_bog_contigs"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.gnm_abi_version() == 7 == _lib.ABI_VERSION
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    assert "gnm_bog_record" in hdr and "int gnm_bog_contigs(" in hdr and "size_t gnm_bog_workspace_bytes(" in hdr
    assert "#define GNM_ABI_VERSION 7" in hdr
    assert engine.BOG_COUNTERS == B.COUNTERS and engine.BOG_RECORD_WORDS == B.WORDS == 8
    assert tuple(decode.BogStats.__dataclass_fields__) == engine.BOG_COUNTERS and decode.BogStats(*range(8)).words() == list(range(8))
    assert "gnm_bog.hip" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    # 72 bytes per node (two generations of a 16-byte record and an 8-byte offset, six int32 arrays) and the block sums
    assert lib.gnm_bog_workspace_bytes(0) == 0 == lib.gnm_bog_workspace_bytes(-1) == lib.gnm_bog_workspace_bytes(2 ** 31 - 1)
    for n in (1, 5, 1024, 1025, 68000):
        assert 72 * n <= lib.gnm_bog_workspace_bytes(n) <= 72 * n + 16 * 10 + 8 * (n // 1024 + 1) + 32, n


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Host-side returns: no device is touched (the checks run before the grid is even sized)."""
    n, E = 4, 8
    rec = (C.c_int64 * B.WORDS)()
    buf = (C.c_int64 * 16)()
    ws = (C.c_int64 * 1024)()
    p = lambda a: C.c_void_p(C.addressof(a))                                     # noqa: E731
    b, r, w = p(buf), p(rec), p(ws)
    need = lib.gnm_bog_workspace_bytes(n)
    assert 0 < need <= 8 * 1024 and C.addressof(ws) % 16 in (0, 8)
    if C.addressof(ws) % 16:
        w = C.c_void_p(C.addressof(ws) + 8)
    ok = dict(n=n, E=E, src=b, dst=b, best_succ=b, best_pred=b, scores=b, y=None, prefix_length=b, read_length=b, min_logit=0.0,
              record=r, contig_ptr=b, walk_nodes=b, walk_edges=b, contig_bases=b, contig_wrong=b, ws=w, ws_bytes=need, stream=None)
    for change, word in ((dict(n=-1), "n = -1"), (dict(E=-1), "E = -1"), (dict(n=2 ** 31 - 1), "2^31"), (dict(E=2 ** 31 - 1), "2^31"),
                         (dict(record=None), "record"), (dict(record=C.c_void_p(C.addressof(rec) + 4)), "aligned"),
                         (dict(best_succ=None), "best_succ"), (dict(best_pred=None), "best_pred"), (dict(read_length=None), "read_length"),
                         (dict(contig_ptr=None), "contig_ptr"), (dict(walk_nodes=None), "walk_nodes"), (dict(walk_edges=None), "walk_edges"),
                         (dict(contig_bases=None), "contig_bases"), (dict(contig_wrong=None), "contig_wrong"),
                         (dict(src=None), "src"), (dict(dst=None), "dst"), (dict(scores=None), "scores"),
                         (dict(prefix_length=None), "prefix_length"), (dict(ws=None), "workspace"), (dict(ws_bytes=need - 1), "workspace"),
                         (dict(ws=C.c_void_p(w.value + 4)), "workspace"), (dict(n=0, E=0, record=None), "record")):
        assert lib.gnm_bog_contigs(*dict(ok, **change).values()) == -1, change
        assert word in lib.gnm_last_error().decode(), (change, lib.gnm_last_error())
    assert all(v == 0 for v in rec) and all(v == 0 for v in buf)
