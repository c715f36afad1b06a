"""GPU: gnm_cover_rounds (engine.cover_rounds, decode.greedy_cover_contigs, infer_contigs(decoder="greedy_cover"),
train.AssemblyStats(decoder="greedy_cover")) against the plain-Python yardstick of tests/cover_reference.py.  The link tables,
round_links, every contig array and the record are integers: every case asserts EQUALITY, there is no tolerance in this file.

Shapes.  A workgroup of the propose kernel serves 32 nodes per pass and a node takes eight lanes: n = 31, 32, 33 sit around the
first, hubs of 8, 9 and 17 candidates around the lane stride.  The link kernel serves 256 nodes per workgroup; the 68,000-node
graph gives both kernels several workgroups and, under an occupancy cap, several grid passes."""
import numpy as np
import pytest
import torch

import bog_reference as B
import cover_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
ARRAYS = ("record", "contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong", "link_succ", "link_pred")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _graph(src, dst, n, node_order=None):
    from gnnome_assembly_amd import AssemblyGraph
    return AssemblyGraph(np.asarray(src, np.int32), np.asarray(dst, np.int32), n, node_order=node_order).to(DEV)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)


def _device(case, node_order=None, min_logit=-INF, labels=True, **kw):
    from gnnome_assembly_amd import decode
    src, dst, n, sc, y, pl, rl = case
    c = decode.greedy_cover_contigs(_graph(src, dst, n, node_order), _t(sc, np.float32), _t(pl, np.int64), _t(rl, np.int64),
                                    _t(y, np.float32) if labels else None, min_logit, **kw)
    torch.cuda.synchronize()
    return c


def _arrays(c):
    h = c.host()
    out = {k: h[k].astype(np.int64) for k in ("contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong")}
    out["record"] = np.asarray(c.stats.words(), np.int64)
    out["link_succ"], out["link_pred"] = c.link_succ.cpu().numpy().astype(np.int64), c.link_pred.cpu().numpy().astype(np.int64)
    out["rounds"], out["round_links"], out["converged"] = c.rounds, list(c.round_links), c.converged
    return out


def _same(got, want, what=""):
    for k in ARRAYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])
    assert (got["rounds"], got["round_links"], got["converged"]) == (want["rounds"], want["round_links"], want["converged"]), \
        (what, got["rounds"], got["round_links"], want["rounds"], want["round_links"])


def _check(case, what="", node_order=None, min_logit=-INF, labels=True, want=None, **kw):
    src, dst, n, sc, y, pl, rl = case
    c = _device(case, node_order, min_logit, labels, **kw)
    got = _arrays(c)
    if want is None:
        want = R.contigs(src, dst, n, sc, pl, rl, y if labels else None, min_logit, kw.get("max_rounds"))
    print(what, "rounds", got["rounds"], "links per round", got["round_links"], "record", dict(zip(B.COUNTERS, got["record"].tolist())))
    _same(got, want, what)
    assert got["record"][3] == 0                              # the cover never counts a refused edge: it never proposes one
    assert c.contig_ptr.is_cuda and c.link_succ.dtype == torch.int32 and len(c) == want["bases"].size
    return c, got


def _raw(case, chunks, node_order=None, min_logit=-INF):
    """engine.cover_rounds called chunk by chunk: (link_succ, link_pred, round_links of every round run)."""
    from gnnome_assembly_amd import engine
    src, dst, n, sc = case[:4]
    g = _graph(src, dst, n, node_order)
    idx = g.index()
    ls, lp = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    ws = torch.empty(engine.cover_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    scd, links = _t(sc, np.float32), []
    for m in chunks:
        rl = torch.full((m,), -5, dtype=torch.int64, device=DEV)
        engine.cover_rounds(idx, scd, rl, ls, lp, ws, len(links), min_logit)
        links += rl.cpu().tolist()
    return ls.cpu().numpy().astype(np.int64), lp.cpu().numpy().astype(np.int64), links


def _case(src, dst, n, sc, seed=0):
    rng = np.random.default_rng(seed)
    E = len(src)
    pl, rl = R.lengths(rng, E, n)
    return (np.asarray(src, np.int32), np.asarray(dst, np.int32), n, np.asarray(sc, np.float32),
            (rng.random(E) < 0.7).astype(np.float32), pl, rl)


def _random(n, E, seed):
    rng = np.random.default_rng(seed)
    return _case(rng.integers(0, n, E), rng.integers(0, n, E), n, rng.standard_normal(E), seed)


# ---- 1. the smallest inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 5, 1])
def test_no_edges(lib, n):
    e = np.zeros(0, np.int32)
    case = (e, e, n, np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.arange(n, dtype=np.int64) + 7)
    for labels in (True, False):
        c, got = _check(case, f"E=0/n={n}", labels=labels)
        assert got["record"].tolist() == [n, 0, 0, 0, 0, 0, 0, 1] and got["contig_ptr"].tolist() == list(range(n + 1))
        assert got["round_links"] == [0] and c.converged and c.walks() == [[v] for v in range(n)]


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33])
def test_around_one_workgroup_pass(lib, n):
    for seed in (0, 1):
        case = _random(n, 5 * n, 100 * n + seed)
        _check(case, f"n={n}/{seed}", node_order="bfs" if seed else None)


@pytest.mark.parametrize("d", [8, 9, 17])
def test_a_hub_whose_candidates_fill_the_lane_stride(lib, d):
    """Node 0 has d out-edges (to 1 .. d) and d in-edges (from d+1 .. 2d); the scores rise with the edge id, so the winner is the
    last candidate a lane reaches; a second hub 2d+1 competes for the same neighbours with lower scores and settles in round 2."""
    h2 = 2 * d + 1
    src = [0] * d + list(range(d + 1, 2 * d + 1)) + [h2] * d + list(range(d + 1, 2 * d + 1))
    dst = list(range(1, d + 1)) + [0] * d + list(range(1, d + 1)) + [h2] * d
    sc = [10.0 + i for i in range(2 * d)] + [1.0 + i for i in range(2 * d)]
    c, got = _check(_case(src, dst, 2 * d + 2, sc, d), f"hub/{d}")
    assert got["link_succ"][0] == d - 1 and got["link_pred"][0] == 2 * d - 1 and got["rounds"] == 3
    assert got["link_succ"][h2] == 3 * d - 2 and got["link_pred"][h2] == 4 * d - 2


def test_nodes_without_a_candidate(lib):
    """Node 0: self loops only.  Node 1: NaN edges only.  Node 4: edges below min_logit only.  7 -> 8 -> 9 is the one path."""
    src = [0, 0, 0, 1, 1, 4, 4, 7, 8]
    dst = [0, 0, 0, 2, 3, 5, 6, 8, 9]
    sc = [9, 9, 9, NAN, NAN, 0.1, 0.5, 2, 2]
    c, got = _check(_case(src, dst, 10, sc), "no candidate", min_logit=1.0)
    assert got["link_succ"].tolist() == [-1] * 7 + [7, 8, -1] and got["link_pred"].tolist() == [-1] * 8 + [7, 8]
    assert got["round_links"] == [2, 0] and c.walks(min_nodes=2) == [[7, 8, 9]]
    c, got = _check(_case(src, dst, 10, sc), "no cut")             # without the cut node 4 links its better edge
    assert got["link_succ"][4] == 6 and got["link_succ"][:2].tolist() == [-1, -1]


# ---- 2. round by round ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mix():
    """About 3,100 nodes, with enough winning and tying distractors that the cover needs five rounds; the yardstick after 1, 2, 3
    and 4 rounds and at its fixed point, computed once."""
    rng = np.random.default_rng(40)
    case = R.mix(41, rng.integers(1, 60, 100).tolist(), rng.integers(2, 40, 15).tolist(), distractors=6000,
                 dprobs=(.1, .05, .05, .05, .1, .45, .2))
    src, dst, n, sc, y, pl, rl = case
    want = {k: R.rounds(src, dst, n, sc, max_rounds=k) for k in (1, 2, 3, 4)}
    return case, want, R.contigs(src, dst, n, sc, pl, rl, y)


@pytest.mark.parametrize("node_order", ["bfs", "keep"])
def test_round_by_round(lib, mix, node_order):
    case, want, full = mix
    assert 2000 < case[2] < 6000 and full["rounds"] >= 5 and full["converged"]
    for k in (1, 2, 3):
        ls, lp, links = _raw(case, [k], node_order)
        assert np.array_equal(ls, want[k][0]) and np.array_equal(lp, want[k][1]) and links == want[k][2], (k, links, want[k][2])
    c, got = _check(case, f"mix/{node_order}", node_order=node_order, want=full)
    F = full["rounds"]
    ls, lp, links = _raw(case, [F, 8], node_order)                 # one more chunk on the fixed point changes nothing
    assert np.array_equal(ls, full["link_succ"]) and np.array_equal(lp, full["link_pred"]) and links == full["round_links"] + [0] * 8
    a, b = _raw(case, [2, 2], node_order), _raw(case, [4], node_order)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == want[4][2]
    assert np.array_equal(b[0], want[4][0]) and np.array_equal(b[1], want[4][1])


def test_the_adversarial_chain_takes_51_rounds_in_several_chunks(lib):
    case = R.adversarial_chain(50)
    c, got = _check(case, "chain", check_every=8)
    assert got["rounds"] == 51 and got["round_links"] == [1] * 50 + [0] and c.converged is True
    c, got = _check(case, "chain/10", check_every=8, max_rounds=10)
    assert got["rounds"] == 10 and c.converged is False and int((got["link_succ"] >= 0).sum()) == 10
    c, got = _check(case, "chain/bfs", node_order="bfs", check_every=3)
    assert got["rounds"] == 51


def test_scores_of_three_values_on_a_10000_node_graph(lib):
    from gnnome_assembly_amd import synth
    src, dst, n = synth.make_graph(5000, seed=9)
    rng = np.random.default_rng(9)
    sc = np.array([-1.0, 0.0, 2.5], np.float32)[rng.integers(0, 3, src.size)]
    c, got = _check(_case(src, dst, n, sc, 9), "ties", node_order="bfs")
    assert n == 10000 and got["rounds"] > 8 and c.converged            # more than one chunk of the default check_every


# ---- 3. round one is the existing decoder ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_logit", [-INF, 1.0])
def test_one_round_is_best_overlap_contigs(lib, mix, min_logit):
    from gnnome_assembly_amd import decode
    case = mix[0]
    src, dst, n, sc, y, pl, rl = case
    c = _device(case, "bfs", min_logit, max_rounds=1)
    b = decode.best_overlap_contigs(_graph(src, dst, n, "bfs"), _t(sc, np.float32), _t(pl, np.int64), _t(rl, np.int64),
                                    _t(y, np.float32), min_logit)
    hc, hb = c.host(), b.host()
    for k in ("contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong"):
        assert np.array_equal(hc[k], hb[k]), k
    wc, wb = c.stats.words(), b.stats.words()
    assert wc[:3] == wb[:3] and wc[4:] == wb[4:] and wc[3] == 0 and wb[3] > 0
    assert c.rounds == 1 and c.round_links == [wb[1] + wb[2]] and (c.converged is False)   # links before the cuts


# ---- 4. several workgroups and grid passes; reproducibility --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """The 68,000-node graph of test_gpu_bog.py, from its recipe: paths of 30,000, 7,700, 4,097 and 1,024 nodes, 2,000 short ones,
    cycles of 3,000 and 1,000 nodes and 50 short ones, 40,000 distractor edges -- and the yardstick on it, computed once."""
    rng = np.random.default_rng(30)
    case = R.mix(31, [30000, 7700, 4097, 1024] + rng.integers(1, 20, 2000).tolist(), [3000, 1000] + rng.integers(2, 30, 50).tolist(),
                 distractors=40000, special_every=3000, dprobs=(.45, .15, .1, .1, .199, .0005, .0005))
    src, dst, n, sc, y, pl, rl = case
    return case, R.contigs(src, dst, n, sc, pl, rl, y, 0.75)


def test_a_68000_node_graph_twice_with_a_capped_grid_in_between(lib, big):
    case, want = big
    assert 60000 < case[2] < 76000
    c, a = _check(case, "big", node_order="bfs", min_logit=0.75, want=want)
    assert int(np.diff(a["contig_ptr"]).max()) > 1024 and a["record"][2] > 0 and a["rounds"] >= 3
    capped = []
    for cap in (1, 2):                        # persistent_grid: at most cap workgroups per CU -- another grid, several passes
        assert lib.gnm_set_occupancy_cap(cap) == 0
        try:
            capped.append(_arrays(_device(case, "bfs", 0.75)))
        finally:
            assert lib.gnm_set_occupancy_cap(0) == 0
    b = _arrays(_device(case, "bfs", 0.75))
    k = _arrays(_device(case, "keep", 0.75, check_every=1))
    for other in capped + [b, k]:
        _same(other, a, "big/again")


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def test_walks_are_walks_of_the_graph(lib, mix):
    case = mix[0]
    src, dst = case[0], case[1]
    c = _device(case)
    h = c.host()
    walks, seen = c.walks(), set()
    assert len(walks) == c.stats.contigs
    for ci, w in enumerate(walks):
        lo = int(h["contig_ptr"][ci])
        assert h["walk_edges"][lo] == -1 and not (seen & set(w)) and len(set(w)) == len(w)
        seen |= set(w)
        for i in range(1, len(w)):
            k = int(h["walk_edges"][lo + i])
            assert src[k] == w[i - 1] and dst[k] == w[i]
    assert seen == set(range(case[2]))


def _cpu_bog(r, pl, rl):
    from gnnome_assembly_amd import decode
    t = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt)           # noqa: E731
    return decode.BogContigs(t(r["contig_ptr"], torch.int32), t(r["walk_nodes"], torch.int32), t(r["walk_edges"], torch.int32),
                             t(r["bases"], torch.int64), t(r["wrong"], torch.int32), decode.BogStats(*r["record"].tolist()),
                             t(pl, torch.int64), t(rl, torch.int64))


def test_infer_contigs_with_the_greedy_cover_decoder(lib):
    from gnnome_assembly_amd import AssemblyGraph, decode, models, synth
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
    scores, walks = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="greedy_cover")
    best = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap")
    assert torch.equal(scores, best[0])
    want = R.contigs(src, dst, n, scores.cpu().numpy(), pl, rl)
    ref = decode.resolve_strands(_cpu_bog(want, pl, rl), 3)
    print("greedy_cover walks", len(walks), "of", int(want["record"][0]), "contigs in", want["rounds"], "rounds; longest",
          max(map(len, walks), default=0), "; best_overlap:", len(best[1]), "walks, longest", max(map(len, best[1]), default=0))
    assert walks == ref.walks and len(walks) > 0 and all(len(w) >= 3 for w in walks)
    assert want["record"][1] > B.contigs(src, dst, n, scores.cpu().numpy(), pl, rl)["record"][1]      # more links than round one alone
    reads = [v >> 1 for w in walks for v in w]
    assert len(set(reads)) == len(reads)                                                       # one strand per read
    _, w2, report = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="greedy_cover", decision_report=True)
    assert w2 == walks and len(report) == 3


def test_contig_sequences_accepts_the_cover(lib):
    import seq_reference as S
    from gnnome_assembly_amd import AssemblyGraph, decode, synth
    from gnnome_assembly_amd.reads import ReadStore
    src, dst, n = synth.make_graph(500, seed=4)
    rng = np.random.default_rng(4)
    reads = S.random_reads(rng, rng.integers(200, 1500, (n + 1) // 2))
    rl = np.array([len(r) for r in reads], np.int64)[np.arange(n) >> 1]
    pl = (rng.random(src.size) * rl[src]).astype(np.int64)
    g = AssemblyGraph(src, dst, n).to(DEV)
    g.edata["prefix_length"] = _t(pl, np.int64)
    cover = decode.greedy_cover_contigs(g, _t(rng.standard_normal(src.size), np.float32), pl, rl)
    store = ReadStore.from_sequences(reads).to(DEV)
    a = decode.contig_sequences(cover, g, store)
    assert a.record.clamped == 0 and a.record.invalid == 0 and len(a) == len(cover) and a.lengths.tolist() == cover.host()["bases"].tolist()
    h, walks = cover.host(), cover.walks()
    wedges = [h["walk_edges"][h["contig_ptr"][c]:h["contig_ptr"][c + 1]].tolist() for c in range(len(walks))]
    want, rec = S.contig_strings(walks, wedges, pl, reads)
    assert a.bases.cpu().numpy().tobytes().decode() == "".join(want) and a.record.words() == [rec[k] for k in S.COUNTERS]


# ---- 6. the training loop --------------------------------------------------------------------------------------------------------------
def _samples():
    """The samples of test_gpu_bog._samples, from their recipe."""
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    from gnnome_assembly_amd.train import GraphSample
    out = []
    for reads, seed in ((300, 11), (280, 12)):
        src, dst, n = synth.make_graph(reads, seed=seed)
        inp = synth.make_inputs(src, dst, n, seed=seed)
        rng = np.random.default_rng(seed)
        g = G.AssemblyGraph(src, dst, n).to(DEV)
        g.edata["prefix_length"] = torch.from_numpy(rng.integers(500, 12000, src.size)).to(DEV)
        g.ndata["read_length"] = torch.from_numpy(rng.integers(8000, 25000, n)).to(DEV)
        out.append(GraphSample(g, torch.from_numpy(inp["e"]).to(DEV), torch.from_numpy(inp["pe"]).to(DEV),
                               torch.from_numpy(inp["y"]).to(DEV)))
    return out


def test_train_loop_with_either_decoder(lib, tmp_path):
    """History.assembly_valid[k] equals the yardstick of the chosen decoder on the epoch's validation logits, recomputed in the hook
    with the same model (the forward is bit-reproducible): cover_reference for "greedy_cover", bog_reference -- the behaviour before
    the option existed -- for the default.  Every other History field and every parameter is the same in both runs."""
    from dataclasses import fields
    from gnnome_assembly_amd import train as T
    hp = dict(num_epochs=2, dim_latent=128, num_gnn_layers=2, lr=1e-3, seed=0, assembly_metrics=True)
    runs = []
    for extra in ({}, dict(assembly_decoder="greedy_cover")):
        s = _samples()
        valid = s[::-1]
        want = []

        def after_epoch(epoch, model, valid=valid, want=want, cover=bool(extra)):
            res = []
            with torch.no_grad():
                for v in valid:
                    px = model(v.graph, v.x, v.e, v.pe).squeeze(-1)
                    sv, dv = (t.cpu().numpy() for t in v.graph.edges())
                    res.append((R.contigs if cover else B.contigs)(
                        sv, dv, v.graph.num_nodes(), px.cpu().numpy(), v.graph.edata["prefix_length"].cpu().numpy(),
                        v.graph.ndata["read_length"].cpu().numpy(), v.y.cpu().numpy()))
            if cover:
                st = T.AssemblyStats(DEV, min_nodes=2, decoder="greedy_cover")
                with torch.no_grad():
                    for v in valid:
                        st.add(v.graph, model(v.graph, v.x, v.e, v.pe).squeeze(-1), v.y)
                assert st.summary() == B.summary(res, min_nodes=2) and st.summary()[0] > 0
            want.append(B.summary(res, min_nodes=20))

        model, _, hist = T.train(s, valid, out="m", hyperparameters=dict(hp, **extra), workdir=str(tmp_path / f"{len(runs)}"),
                                 verbose=False, hooks={"after_epoch": after_epoch})
        runs.append((hist, {k: v.detach().cpu() for k, v in model.state_dict().items()}))
        assert len(hist.assembly_valid) == 2
        for ep in range(2):
            print(extra, "epoch", ep, "assembly_valid", hist.assembly_valid[ep])
            assert hist.assembly_valid[ep] == want[ep]
    (h0, s0), (h1, s1) = runs
    for f in fields(T.History):
        if f.name != "assembly_valid":
            assert getattr(h0, f.name) == getattr(h1, f.name), f.name
    assert set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)
