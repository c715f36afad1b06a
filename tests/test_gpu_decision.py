"""GPU: gnm_decision_stats (engine.decision_stats, train.DecisionStats, decode.decision_table) against the plain-Python yardstick
of tests/decision_reference.py.  Tables and counters are integers: every case asserts EQUALITY, there is no tolerance in this
file.  The accuracies of History.decision_valid are ratios of two of those integers, formed by the same fp64 division on both
sides, and are compared for equality as well.

Shapes.  A node takes eight lanes, a wave eight nodes, a workgroup 32 per round: the degree ladder (0, 1, 2, 63, 64, 65, 129, 300
in both directions, one of them with a self loop inside its range) covers below / at / above a group, the loop, and ranges whose
length is not their candidate count; its 400 nodes and the banded graph's 2,000 span several workgroups with a ragged last one.
Those graphs fit one round of the persistent grid under every cap; the banded graph at 34,000 reads (68,000 nodes, 2,125
workgroup-rounds) does not: its case runs the grid-stride loop for two to nine rounds with a ragged last one."""
import numpy as np
import pytest
import torch

import decision_reference as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LADDER = (0, 1, 2, 63, 64, 65, 129, 300)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _graph(src, dst, n, node_order=None):
    from gnnome_assembly_amd import AssemblyGraph
    return AssemblyGraph(np.asarray(src, np.int32), np.asarray(dst, np.int32), n, node_order=node_order).to(DEV)


def _device(g, scores, y, rec=None, tables=True):
    """(best_succ, best_pred, record) of one call on graph g, as numpy arrays (tables None when not asked for)."""
    from gnnome_assembly_amd.train import DecisionStats
    st = DecisionStats(DEV)
    if rec is not None:
        st.buf.copy_(torch.from_numpy(rec))
    n = g.num_nodes()
    bs = torch.full((n,), -7, dtype=torch.int32, device=DEV) if tables else None
    bp = torch.full((n,), -7, dtype=torch.int32, device=DEV) if tables else None
    st.add(g, torch.from_numpy(np.asarray(scores, np.float32)).to(DEV),
           None if y is None else torch.from_numpy(np.asarray(y, np.float32)).to(DEV), bs, bp)
    torch.cuda.synchronize()
    return (bs.cpu().numpy() if tables else None), (bp.cpu().numpy() if tables else None), st.buf.cpu().numpy()


def _check(g, src, dst, n, scores, y, what=""):
    bs, bp, rec = _device(g, scores, y)
    ws, wp, wrec = D.decisions(src, dst, n, scores, y)
    print(what, "record", rec.tolist())
    assert np.array_equal(rec, wrec), (what, rec.tolist(), wrec.tolist())
    assert np.array_equal(bs, ws) and np.array_equal(bp, wp), what
    return rec


def _ladder_graph(seed=0):
    """400 nodes: out-hub k (node k) has LADDER[k] out-edges to distinct leaves, in-hub k (node 8 + k) LADDER[k] in-edges from
    distinct leaves; leaves 16 .. 315, the rest isolated but for node 399.  The degree-64 hubs also carry one self loop (a range
    of 65 entries with 64 candidates); node 399 has the same edge to leaf 16 twice (a duplicate: two candidates).  Edge ids are
    shuffled."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for k, d in enumerate(LADDER):
        leaves = 16 + rng.permutation(300)[:d]
        src += [k] * d
        dst += leaves.tolist()
        leaves = 16 + rng.permutation(300)[:d]
        src += leaves.tolist()
        dst += [8 + k] * d
    k64 = LADDER.index(64)
    src += [k64, 8 + k64, 399, 399]
    dst += [k64, 8 + k64, 16, 16]
    p = rng.permutation(len(src))
    return np.array(src, np.int32)[p], np.array(dst, np.int32)[p], 400


def _specials(E, seed):
    """scores: 8 distinct values with +-inf, -0.0 / +0.0, NaN (both signs) and denormals sprinkled over a third of the edges;
    labels: 0, 1, 0.5 and NaN."""
    rng = np.random.default_rng(seed)
    sc = rng.integers(-3, 5, E).astype(np.float32) * np.float32(0.5)
    sp = np.array([np.inf, -np.inf, 0.0, -0.0, np.nan, -np.nan, 1e-45, -1e-45, 1e-39, -1e-39], np.float32)
    at = rng.permutation(E)[:E // 3]
    sc[at] = sp[rng.integers(0, sp.size, at.size)]
    y = np.array([0.0, 1.0, 0.5, np.nan], np.float32)[rng.choice(4, E, p=[0.4, 0.4, 0.1, 0.1])]
    return sc, y


# ---- 1. the tiny golden graph ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node_order", ["keep", "bfs"])
def test_tiny_edge_case_graph(lib, node_order):
    from gnnome_assembly_amd import synth
    src, dst, n = synth.tiny_edge_case_graph(0)
    assert n == 64 and src.size == 256 and (src == dst).any()
    rng = np.random.default_rng(1)
    sc = rng.standard_normal(src.size).astype(np.float32)
    y = (rng.random(src.size) < 0.5).astype(np.float32)
    rec = _check(_graph(src, dst, n, node_order), src, dst, n, sc, y, f"tiny/{node_order}")
    assert rec[0] > 0 and rec[3] > 0 and rec[7] > 0 and rec[10] > 0                 # dead and branching nodes on both sides


# ---- 2. / 3. the degree ladder, with frequent ties and with special scores and labels -----------------------------------------------
@pytest.mark.parametrize("node_order", ["keep", "bfs"])
def test_degree_ladder_with_eight_distinct_scores(lib, node_order):
    src, dst, n = _ladder_graph()
    outd, ind = np.bincount(src[src != dst], minlength=n), np.bincount(dst[src != dst], minlength=n)
    assert outd[:8].tolist() == list(LADDER) and ind[8:16].tolist() == list(LADDER) and outd[399] == 2
    rng = np.random.default_rng(2)
    sc = rng.integers(0, 8, src.size).astype(np.float32) - np.float32(3.5)
    y = (rng.random(src.size) < 0.3).astype(np.float32)
    _check(_graph(src, dst, n, node_order), src, dst, n, sc, y, f"ladder/{node_order}")


@pytest.mark.parametrize("seed", [3, 8])        # draws in which, by the yardstick, some branch has NaN candidates only
def test_special_scores_and_labels(lib, seed):
    src, dst, n = _ladder_graph()
    sc, y = _specials(src.size, seed)
    rec = _check(_graph(src, dst, n, "bfs"), src, dst, n, sc, y, f"specials/{seed}")
    assert rec[6] + rec[13] > 0                                                     # some branch whose every candidate is NaN
    # all NaN, all equal, all -0.0 / +0.0: every choice is the lowest edge id
    for name, flat in (("nan", np.full(src.size, np.nan, np.float32)), ("equal", np.full(src.size, 1.25, np.float32)),
                       ("zeros", np.where(np.arange(src.size) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32))):
        _check(_graph(src, dst, n), src, dst, n, flat, y, f"specials/{name}")


# ---- 4. numbering: shuffled edge ids and node ids, internal renumbering active ------------------------------------------------------
def _banded(reads=1000, seed=5):
    from gnnome_assembly_amd import synth
    src, dst, n = synth.make_graph(reads, seed=seed, permute_edge_ids=True)
    rng = np.random.default_rng(seed)
    relabel = rng.permutation(n).astype(np.int32)
    p = rng.permutation(src.size)
    return relabel[src][p], relabel[dst][p], n


def test_tables_come_back_in_the_callers_numbering(lib):
    src, dst, n = _banded()
    g = _graph(src, dst, n, "bfs")
    idx = g.index()
    assert "nperm" in idx and not torch.equal(idx["nperm"].cpu(), torch.arange(n, dtype=torch.int32))
    assert not torch.equal(idx["perm"].cpu(), torch.arange(src.size, dtype=torch.int32))
    rng = np.random.default_rng(6)
    sc = rng.standard_normal(src.size).astype(np.float32)
    y = (rng.random(src.size) < 0.6).astype(np.float32)
    _check(g, src, dst, n, sc, y, "banded/bfs")


# ---- 5. a mini-batch sub-graph, by both induce methods ------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["sort", "index"])
def test_induced_subgraph(lib, method):
    from gnnome_assembly_amd import cluster
    src, dst, n = _banded(reads=600, seed=7)
    g = _graph(src, dst, n, "bfs")
    rng = np.random.default_rng(8)
    mask = torch.from_numpy(rng.random(n) < 0.6).to(DEV)
    sub = cluster.induced_subgraph(g, mask, method)
    s, d = (t.cpu().numpy() for t in sub.edges())
    assert 0 < s.size < src.size and "nperm" in sub.index()
    sc = rng.integers(0, 6, s.size).astype(np.float32)
    y = (rng.random(s.size) < 0.5).astype(np.float32)
    _check(sub, s, d, sub.num_nodes(), sc, y, f"sub/{method}")


# ---- 6. / 7. empty inputs, NULL arguments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 0])
def test_empty_inputs(lib, n):
    e = np.zeros(0, np.int32)
    g = _graph(e, e, n)
    for y in (np.zeros(0, np.float32), None):
        bs, bp, rec = _device(g, np.zeros(0, np.float32), y)
        ws, wp, wrec = D.decisions(e, e, n, e, y)
        assert np.array_equal(rec, wrec) and rec[-1] == 1 and rec[0] == n == rec[7] and int(rec.sum()) == 2 * n + 1
        assert np.array_equal(bs, ws) and np.array_equal(bp, wp)


def test_null_labels_and_null_tables(lib):
    src, dst, n = _ladder_graph()
    sc, y = _specials(src.size, 8)
    g = _graph(src, dst, n, "bfs")
    ws, wp, wrec = D.decisions(src, dst, n, sc, None)
    bs, bp, rec = _device(g, sc, None)
    assert np.array_equal(rec, wrec) and np.array_equal(bs, ws) and np.array_equal(bp, wp)
    assert rec[[2, 4, 5, 9, 11, 12]].tolist() == [0] * 6 and rec[6] + rec[13] > 0   # only dead / forced / branch / branch_nan moved
    full = D.decisions(src, dst, n, sc, y)[2]
    assert np.array_equal(_device(g, sc, y, tables=False)[2], full)                # no tables: the same record
    # one table only
    from gnnome_assembly_amd.train import DecisionStats
    st, only = DecisionStats(DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)
    st.add(g, torch.from_numpy(sc).to(DEV), torch.from_numpy(y).to(DEV), None, only)
    assert np.array_equal(only.cpu().numpy(), wp) and np.array_equal(st.buf.cpu().numpy(), full)


# ---- 8. bad arguments ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_their_error_and_launch_nothing(lib):
    from gnnome_assembly_amd import engine
    from gnnome_assembly_amd._lib import GnmError
    from gnnome_assembly_amd.train import DecisionStats
    src, dst, n = _ladder_graph()
    g = _graph(src, dst, n)
    idx, E = g.index(), src.size
    sc, y = torch.zeros(E, device=DEV), torch.ones(E, device=DEV)
    st = DecisionStats(DEV)
    bs, bp = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    p = engine._ptr
    ok = dict(n=n, E=E, perm=p(idx["perm"]), isrc=p(idx["isrc"]), idst=p(idx["idst"]), in_ptr=p(idx["in_ptr"]), out_ptr=p(idx["out_ptr"]),
              out_pos=p(idx["out_pos"]), out_dst=p(idx["out_dst"]), nperm=None, scores=p(sc), y=p(y), record=p(st.buf), best_succ=p(bs),
              best_pred=p(bp), stream=None)
    for change, word in ((dict(n=-1), "n = -1"), (dict(E=-2), "E = -2"), (dict(n=2 ** 31 - 1), "2^31"), (dict(E=2 ** 40), "2^31"),
                         (dict(record=None), "record"), (dict(record=engine.C.c_void_p(st.buf.data_ptr() + 4)), "aligned"),
                         (dict(in_ptr=None), "in_ptr"), (dict(out_ptr=None), "out_ptr"), (dict(perm=None), "perm"),
                         (dict(isrc=None), "isrc"), (dict(out_pos=None), "out_pos"), (dict(out_dst=None), "out_dst"),
                         (dict(scores=None), "scores")):
        assert lib.gnm_decision_stats(*dict(ok, **change).values()) == -1, change
        assert word in lib.gnm_last_error().decode(), change
    for call in (lambda: engine.decision_stats(idx, sc[:-1], None, st.buf),                     # scores of another length
                 lambda: engine.decision_stats(idx, sc, y[:-1], st.buf),
                 lambda: engine.decision_stats(idx, sc, y, st.buf[:-1]),
                 lambda: engine.decision_stats(idx, sc, y, st.buf.int()),
                 lambda: engine.decision_stats(idx, sc, y, st.buf, bs[:-1]),
                 lambda: engine.decision_stats(idx, sc, y, st.buf, bs, bp.long())):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(GnmError):
        engine.decision_stats(idx, sc.cpu(), y, st.buf)                                        # CPU scores: no fallback
    torch.cuda.synchronize()
    assert int(st.buf.abs().sum()) == 0 and bool((bs == -7).all()) and bool((bp == -7).all())


# ---- 9. reproducibility ----------------------------------------------------------------------------------------------------------------
def test_same_bits_between_runs_grids_and_a_record_added_to_twice(lib):
    src, dst, n = _banded(reads=1000, seed=10)
    g = _graph(src, dst, n, "bfs")
    rng = np.random.default_rng(11)
    sc = rng.integers(0, 8, src.size).astype(np.float32)
    y = (rng.random(src.size) < 0.5).astype(np.float32)
    want = D.decisions(src, dst, n, sc, y)
    a, b = _device(g, sc, y), _device(g, sc, y)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and all(np.array_equal(u, v) for u, v in zip(a, want))
    capped = []
    for cap in (1, 2):                     # persistent_grid: at most cap workgroups per CU -- another grid where n is large enough
        assert lib.gnm_set_occupancy_cap(cap) == 0
        try:
            capped.append(_device(g, sc, y))
        finally:
            assert lib.gnm_set_occupancy_cap(0) == 0
    for c in capped:
        assert all(np.array_equal(u, v) for u, v in zip(a, c))
    twice = _device(g, sc, y, rec=a[2])
    assert np.array_equal(twice[2], 2 * a[2]) and twice[2][-1] == 2
    base = np.arange(D.WORDS, dtype=np.int64) * 5 + 3                                   # a call into a non-zero record adds to it
    assert np.array_equal(_device(g, sc, y, rec=base)[2], base + want[2])


def _grid(lib, n, cap):
    """Workgroups that gnm_decision_stats launches for n nodes (persistent_grid(n, 32, 8) of gnm_common.h under the cap)."""
    per_cu = min(8, cap) if cap else 8
    want = max(1, min(-(-n // 32), lib.gnm_num_cus() * per_cu, lib.gnm_max_partial_blocks()))
    return -(-want // 8) * 8


@pytest.fixture(scope="module")
def big():
    """The banded graph at 34,000 reads with shuffled ids, eight distinct scores, and the yardstick on it -- computed once."""
    src, dst, n = _banded(reads=34000, seed=12)
    rng = np.random.default_rng(13)
    sc = rng.integers(0, 8, src.size).astype(np.float32)
    y = (rng.random(src.size) < 0.5).astype(np.float32)
    return src, dst, n, sc, y, D.decisions(src, dst, n, sc, y)


def test_many_rounds_of_the_persistent_grid_under_three_caps(lib, big):
    """n = 68,000 is more than the 2,048 workgroups of the largest grid serve in one round (65,536 nodes): under the default the
    stride is taken once and the second round is ragged; under caps 1 and 2 a 256-CU device runs 9 and 5 rounds on grids of 256
    and 512.  Every one must equal the yardstick: the stride, the counters carried across rounds and the tail of a later round."""
    src, dst, n, sc, y, want = big
    g = _graph(src, dst, n, "bfs")
    assert "nperm" in g.index()
    grids = {cap: _grid(lib, n, cap) for cap in (0, 1, 2)}
    rounds = {cap: -(-n // (32 * grids[cap])) for cap in grids}
    print("grids", grids, "rounds", rounds)
    assert all(r > 1 for r in rounds.values()) and n % (32 * grids[0]) != 0
    if lib.gnm_num_cus() * 2 <= lib.gnm_max_partial_blocks():
        assert len(set(grids.values())) == 3
    for cap in (0, 1, 2):
        assert lib.gnm_set_occupancy_cap(cap) == 0
        try:
            got = _device(g, sc, y)
        finally:
            assert lib.gnm_set_occupancy_cap(0) == 0
        assert np.array_equal(got[2], want[2]), (cap, got[2].tolist(), want[2].tolist())
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), cap


# ---- 10. the training loop ----------------------------------------------------------------------------------------------------------------
def _samples():
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    from gnnome_assembly_amd.train import GraphSample
    out = []
    for reads, seed in ((300, 11), (280, 12)):
        src, dst, n = synth.make_graph(reads, seed=seed)
        inp = synth.make_inputs(src, dst, n, seed=seed)
        out.append(GraphSample(G.AssemblyGraph(src, dst, n).to(DEV), torch.from_numpy(inp["e"]).to(DEV),
                               torch.from_numpy(inp["pe"]).to(DEV), torch.from_numpy(inp["y"]).to(DEV)))
    return out


@pytest.mark.parametrize("mode", ["full_graph", "combined", "mini_batch"])
def test_train_loop_reports_the_reference_figures_and_changes_nothing_else(lib, tmp_path, mode):
    """full_graph: the option alone.  combined: with fused_metrics, ranking_metrics and symmetry_loss (the ORIGINAL scores are
    counted).  Both: History.decision_valid[k] equals the yardstick on the epoch's validation logits, recomputed in the hook with
    the same model (the forward is bit-reproducible).  mini_batch: batch_size_eval > 1 counts per sub-graph (the partition is
    drawn inside the loop), so only the entries' form is checked.  All: a run with the option off gives the same History and
    parameters."""
    from dataclasses import fields
    from gnnome_assembly_amd import train as T
    hp = dict(num_epochs=2, dim_latent=128, num_gnn_layers=2, lr=1e-3, seed=0)
    if mode == "combined":
        hp.update(fused_metrics=True, ranking_metrics=True, symmetry_loss=True)
    if mode == "mini_batch":
        hp.update(batch_size_train=2, batch_size_eval=2, num_parts_metis_train=8, num_parts_metis_eval=8)
    runs = []
    for on in (False, True):
        s = _samples()
        valid = s[::-1]
        want = []

        def after_epoch(epoch, model, valid=valid, want=want):
            rec = np.zeros(D.WORDS, np.int64)
            with torch.no_grad():
                for v in valid:
                    px = model(v.graph, v.x, v.e, v.pe).squeeze(-1).cpu().numpy()
                    sv, dv = (t.cpu().numpy() for t in v.graph.edges())
                    rec += D.decisions(sv, dv, v.graph.num_nodes(), px, v.y.cpu().numpy())[2]
            want.append(rec)

        model, _, hist = T.train(s, valid, out=mode, hyperparameters=dict(hp, decision_metrics=on), workdir=str(tmp_path / f"{on}"),
                                 verbose=False, hooks={"after_epoch": after_epoch} if mode != "mini_batch" else None)
        runs.append((hist, {k: v.detach().cpu() for k, v in model.state_dict().items()}))
        if not on:
            assert hist.decision_valid == []
            continue
        assert len(hist.decision_valid) == 2
        for ep in range(2):
            got = hist.decision_valid[ep]
            print(mode, "epoch", ep, "decision_valid", got)
            assert len(got) == 4 and all(0.0 <= v <= 1.0 for v in got)
            if mode != "mini_batch":
                assert want[ep][-1] == len(valid) and want[ep][3] > 0 and want[ep][10] > 0
                assert got == D.summary(want[ep])
    (h0, s0), (h1, s1) = runs
    for f in fields(T.History):
        if f.name != "decision_valid":
            assert getattr(h0, f.name) == getattr(h1, f.name), f.name
    assert h0.loss_valid == h1.loss_valid and set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)


# ---- 11. the decode side ----------------------------------------------------------------------------------------------------------------
def test_decision_table_and_infer_contigs_report(lib):
    from gnnome_assembly_amd import AssemblyGraph, decode, models, synth
    from gnnome_assembly_amd.train import DecisionMetrics
    seed = 4
    src, dst, n = synth.make_graph(600, seed=seed)
    inp = synth.make_inputs(src, dst, n, seed=seed)
    H, L = 128, 2
    model = models.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, seed=seed).items()})
    model.to(DEV)
    g = AssemblyGraph(src, dst, n, node_order="bfs").to(DEV)
    e, pe = torch.from_numpy(inp["e"]).to(DEV), torch.from_numpy(inp["pe"]).to(DEV)
    rng = np.random.default_rng(seed)
    pl, rl = rng.integers(500, 12000, src.size), rng.integers(8000, 25000, n)
    torch.manual_seed(seed)
    plain = decode.infer_contigs(model, g, e, pe, pl, rl, nb_paths=20, len_threshold=5)
    assert len(plain) == 2 and len(plain[1]) > 0
    # without labels on the graph: tables and node counts
    torch.manual_seed(seed)
    scores, walks, report = decode.infer_contigs(model, g, e, pe, pl, rl, nb_paths=20, len_threshold=5, decision_report=True)
    assert torch.equal(scores, plain[0]) and walks == plain[1]
    sc = scores.cpu().numpy()
    ws, wp, wrec = D.decisions(src, dst, n, sc, None)
    bs, bp, m = report
    assert isinstance(m, DecisionMetrics) and bs.is_cuda and bs.dtype == torch.int32
    assert np.array_equal(bs.cpu().numpy(), ws) and np.array_equal(bp.cpu().numpy(), wp)
    assert [getattr(m.succ, k) for k in D.COUNTERS] == wrec[:7].tolist() and [getattr(m.pred, k) for k in D.COUNTERS] == wrec[7:14].tolist()
    assert np.isnan(m.branch_accuracy) or m.pooled.branch == 0 or m.pooled.branch_ok == 0
    # with labels: decision_table directly, and through the graph's edata with device sampling
    y = inp["y"]
    ws, wp, wrec = D.decisions(src, dst, n, sc, y)
    bs, bp, m = decode.decision_table(g, scores, torch.from_numpy(y).to(DEV))
    assert np.array_equal(bs.cpu().numpy(), ws) and np.array_equal(bp.cpu().numpy(), wp) and m.calls == 1
    assert m.summary() == D.summary(wrec) and 0.0 <= m.branch_accuracy <= m.solvable_accuracy <= 1.0
    g.edata["y"] = torch.from_numpy(y).to(DEV)
    torch.manual_seed(seed)
    dev_plain = decode.infer_contigs(model, g, e, pe, pl, rl, nb_paths=20, len_threshold=5, device_sampling=True)
    torch.manual_seed(seed)
    _, dev_walks, (_, _, m2) = decode.infer_contigs(model, g, e, pe, pl, rl, nb_paths=20, len_threshold=5, device_sampling=True,
                                                    decision_report=True)
    assert dev_walks == dev_plain[1] and m2.summary() == D.summary(wrec)
    with pytest.raises(Exception):
        decode.decision_table(AssemblyGraph(src, dst, n), scores.cpu())                       # a graph on the CPU: no fallback
