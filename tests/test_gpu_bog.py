"""GPU: gnm_bog_contigs (engine.bog_contigs, decode.best_overlap_contigs, train.AssemblyStats) against the plain-Python yardstick
of tests/bog_reference.py.  Every output array and the record are integers: every case asserts EQUALITY, there is no tolerance
in this file.  The floats of History.assembly_valid are one ratio of two of those integers, formed by the same fp64 division.

Shapes.  The round count K = ceil(log2(max(n, 2))) changes at a power of two: single paths of 1024, 1025 and 4097 nodes sit at
and one past it, with node ids permuted so that ranks do not follow ids.  Cycles of 3, 5 and 1000 nodes are no powers of two:
the minimum must still go round.  The scans work in blocks of 1024 nodes and a workgroup serves 256: the 68,000-node graph spans
67 scan blocks and, under an occupancy cap, several grid rounds."""
import numpy as np
import pytest
import torch

import bog_reference as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


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


def _device(case, node_order=None, min_logit=-INF, labels=True):
    from gnnome_assembly_amd import decode
    src, dst, n, sc, y, pl, rl = case
    c = decode.best_overlap_contigs(_graph(src, dst, n, node_order), _t(sc, np.float32), _t(pl, np.int64), _t(rl, np.int64),
                                    _t(y, np.float32) if labels else None, min_logit)
    torch.cuda.synchronize()
    return c


def _arrays(c):
    h = c.host()
    return {k: h[k].astype(np.int64) for k in ("contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong")} | \
        {"record": np.asarray(c.stats.words(), np.int64)}


def _same(got, want, what=""):
    for k in ("record", "contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])


def _check(case, what="", node_order=None, min_logit=-INF, labels=True):
    src, dst, n, sc, y, pl, rl = case
    c = _device(case, node_order, min_logit, labels)
    got = _arrays(c)
    want = B.contigs(src, dst, n, sc, pl, rl, y if labels else None, min_logit)
    print(what, "record", dict(zip(B.COUNTERS, got["record"].tolist())))
    _same(got, want, what)
    assert c.contig_ptr.is_cuda and c.contig_ptr.dtype == torch.int32 and c.bases.dtype == torch.int64 and len(c) == want["bases"].size
    return c, got


def _lengths(rng, E, n):
    return rng.integers(1, 12000, E).astype(np.int64), rng.integers(1000, 25000, n).astype(np.int64)


def _chain(n, seed, cycle=False):
    """One path (or one cycle) over n nodes whose ids are randomly permuted, edge ids shuffled."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n).astype(np.int32)
    m = n if cycle else n - 1
    src, dst = ids[np.arange(m)], ids[(np.arange(m) + 1) % n]
    p = rng.permutation(m)
    src, dst = src[p], dst[p]
    pl, rl = _lengths(rng, m, n)
    return src, dst, n, rng.standard_normal(m).astype(np.float32), (rng.random(m) < 0.7).astype(np.float32), pl, rl


def _mix(seed, path_lens, cycle_lens, distractors, special_every=25, dprobs=(.3, .1, .1, .1, .15, .2, .05)):
    """Paths and cycles over randomly permuted node ids (main edges at scores 1, 2, 4 with a few specials among them), plus
    `distractors` random edges -- self loops and duplicates of main edges among them -- whose scores mostly lose (-1, +-0, -inf,
    NaN), sometimes tie (1: the lowest edge id decides) and sometimes win (5: the path breaks there) -- `dprobs` in that order; one
    main edge in `special_every` is NaN, -inf, +-0 or 0.5.  Edge ids are shuffled; labels are 0, 1, 0.5 and NaN."""
    rng = np.random.default_rng(seed)
    n = int(sum(path_lens) + sum(cycle_lens))
    ids = rng.permutation(n).astype(np.int32)
    src, dst, at = [], [], 0
    for m in path_lens:
        src += ids[at:at + m - 1].tolist()
        dst += ids[at + 1:at + m].tolist()
        at += m
    for m in cycle_lens:
        src += ids[at:at + m].tolist()
        dst += np.roll(ids[at:at + m], -1).tolist()
        at += m
    main = len(src)
    sc = np.array([1.0, 2.0, 4.0], np.float32)[rng.integers(0, 3, main)]
    sp = rng.permutation(main)[:main // special_every]
    sc[sp] = np.array([NAN, -INF, 0.0, -0.0, 0.5], np.float32)[rng.integers(0, 5, sp.size)]
    ds, dd = rng.integers(0, n, distractors), rng.integers(0, n, distractors)
    dup = rng.permutation(distractors)[:distractors // 10]
    pick = rng.integers(0, main, dup.size)
    ds[dup], dd[dup] = np.array(src)[pick], np.array(dst)[pick]
    loops = rng.permutation(distractors)[:distractors // 20]
    dd[loops] = ds[loops]
    dsc = np.array([-1.0, 0.0, -0.0, -INF, NAN, 1.0, 5.0], np.float32)[rng.choice(7, distractors, p=list(dprobs))]
    src, dst, sc = np.concatenate([src, ds]).astype(np.int32), np.concatenate([dst, dd]).astype(np.int32), np.concatenate([sc, dsc])
    p = rng.permutation(src.size)
    src, dst, sc = src[p], dst[p], sc[p]
    y = np.array([0.0, 1.0, 0.5, NAN], np.float32)[rng.choice(4, src.size, p=[0.3, 0.5, 0.1, 0.1])]
    pl, rl = _lengths(rng, src.size, n)
    return src, dst, n, sc, y, pl, rl


# ---- 1. the smallest inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 5, 1])
def test_no_edges(lib, n):
    e = np.zeros(0, np.int32)
    case = (e, e, n, np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.arange(n, dtype=np.int64) + 7)
    for labels in (True, False):
        c, got = _check(case, f"E=0/n={n}", labels=labels)
        assert got["record"].tolist() == [n, 0, 0, 0, 0, 0, 0, 1] and got["contig_ptr"].tolist() == list(range(n + 1))
        assert c.walks() == [[v] for v in range(n)] and c.longest() == (n + 6 if n else 0)


# ---- 2. single paths and single cycles at the round count's edges -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 1024, 1025, 4097, 256 * 1024 + 5])     # the last: 257 scan blocks, two block sums per thread
def test_one_path_with_permuted_ids(lib, n):
    case = _chain(n, seed=n)
    c, got = _check(case, f"path/{n}")
    assert got["record"][:4].tolist() == [1, n - 1, 0, 0] and got["record"][5:].tolist() == [n, 1, 1]
    head = int(np.setdiff1d(case[0], case[1])[0])
    assert got["walk_nodes"][0] == head and got["walk_edges"][0] == -1 and got["contig_ptr"].tolist() == [0, n]
    assert got["bases"][0] == case[5].sum() + case[6][got["walk_nodes"][-1]]


@pytest.mark.parametrize("n", [2, 3, 5, 64, 1000])
def test_one_cycle_is_cut_at_its_smallest_node(lib, n):
    case = _chain(n, seed=100 + n, cycle=True)
    c, got = _check(case, f"cycle/{n}")
    assert got["record"].tolist()[:4] == [1, n - 1, 1, 0] and got["walk_nodes"][0] == 0 and got["contig_ptr"].tolist() == [0, n]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 256 * 1024 + 1])   # the scan block B = 1024: B - 1, B, B + 1; 257 scan blocks
def test_chains_of_three_nodes_at_the_scan_block_edges(lib, n):
    """Nodes 3j -> 3j + 1 -> 3j + 2 in id order (the last chain may be shorter): the scanned head flags are 1, 0, 0, .. and the
    scanned lengths 3, 0, 0, .., so every output has a closed form and a wrong block offset moves a contig.  gnm_bog_contigs on
    hand-made tables; every output is the head of a longer buffer whose tail must keep its fill."""
    from gnnome_assembly_amd import engine
    v = np.arange(n)
    linked = (v % 3 != 2) & (v + 1 < n)                      # v -> v + 1 by edge id[v]
    src = v[linked]
    E = src.size
    eid = np.full(n, -1, np.int64)
    eid[src] = np.arange(E)
    pred = np.full(n, -1, np.int64)
    pred[src + 1] = eid[src]
    pl, rl = np.arange(E, dtype=np.int64) * 7 + 1, v.astype(np.int64) + 1000
    C = (n + 2) // 3
    ptr = np.minimum(3 * np.arange(C + 1), n)
    lens = np.diff(ptr)
    bases = np.zeros(C, np.int64)
    np.add.at(bases, src // 3, pl)
    bases += rl[ptr[1:] - 1]
    want = {"contig_ptr": ptr, "walk_nodes": v, "walk_edges": pred, "contig_bases": bases, "contig_wrong": np.zeros(C, np.int64)}
    record = [C, E, 0, 0, 0, int(lens[lens > 1].sum()), int((lens > 1).sum()), 1]
    pad, fill = 64, -7
    buf = {k: torch.full((m + pad,), fill, dtype=dt, device=DEV) for k, m, dt in
           (("contig_ptr", n + 1, torch.int32), ("walk_nodes", n, torch.int32), ("walk_edges", n, torch.int32),
            ("contig_bases", n, torch.int64), ("contig_wrong", n, torch.int32))}
    rec = torch.zeros(B.WORDS, dtype=torch.int64, device=DEV)
    engine.bog_contigs(_t(src, np.int32), _t(src + 1, np.int32), _t(eid, np.int32), _t(pred, np.int32), torch.ones(E, device=DEV),
                       torch.ones(E, device=DEV), _t(pl, np.int64), _t(rl, np.int64), rec,
                       **{k: b[:b.numel() - pad] for k, b in buf.items()})
    torch.cuda.synchronize()
    assert rec.tolist() == record
    for k, b in buf.items():
        got = b.cpu().numpy().astype(np.int64)
        assert np.array_equal(got[:want[k].size], want[k]), (k, got[:12], want[k][:12])
        assert (got[-pad:] == fill).all(), k


# ---- 3. a mix of paths and cycles with distractors, ties and special scores ----------------------------------------------------------------
@pytest.fixture(scope="module")
def mix():
    rng = np.random.default_rng(20)
    return _mix(21, rng.integers(1, 60, 300).tolist(), rng.integers(2, 40, 40).tolist(), distractors=6000)


@pytest.mark.parametrize("min_logit", [-INF, 1.0])
def test_mix_of_paths_and_cycles(lib, mix, min_logit):
    c, got = _check(mix, f"mix/{min_logit}", node_order="bfs", min_logit=min_logit)
    rec = dict(zip(B.COUNTERS, got["record"].tolist()))
    assert rec["cycles_cut"] > 0 and rec["dropped"] > 0 and rec["multi_contigs"] > 10 and rec["wrong_links"] > 0
    assert rec["links"] == mix[2] - rec["contigs"] and rec["wrong_links"] == int(got["wrong"].sum())
    if min_logit == 1.0:                      # the cut refuses links that the uncut run keeps
        assert rec["dropped"] > B.contigs(*mix[:4], mix[5], mix[6], mix[4])["record"][3]
    _check(mix, f"mix/{min_logit}/no labels", min_logit=min_logit, labels=False)


def test_walks_are_walks_of_the_graph(lib, mix):
    src, dst = mix[0], mix[1]
    c = _device(mix)
    h = c.host()
    walks, seen = c.walks(), set()
    assert len(walks) == c.stats.contigs and c.walks(min_nodes=2) == [w for w in walks if len(w) >= 2]
    for ci, w in enumerate(walks):
        lo = int(h["contig_ptr"][ci])
        assert h["walk_edges"][lo] == -1 and not (seen & set(w)) and len(set(w)) == len(w)
        seen |= set(w)
        for i in range(1, len(w)):
            k = int(h["walk_edges"][lo + i])
            assert src[k] == w[i - 1] and dst[k] == w[i]
    assert seen == set(range(mix[2]))


# ---- 4. several scan blocks and grid rounds; reproducibility ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """About 68,000 nodes: paths of 30,000, 7,700, 4,097 and 1,024 nodes, 2,000 short ones, cycles of 3,000 and 1,000 nodes and 50
    short ones, 40,000 distractor edges of which only a few dozen win or tie, so that paths of thousands of nodes survive -- and the
    yardstick on it, computed once."""
    rng = np.random.default_rng(30)
    case = _mix(31, [30000, 7700, 4097, 1024] + rng.integers(1, 20, 2000).tolist(), [3000, 1000] + rng.integers(2, 30, 50).tolist(),
                distractors=40000, special_every=3000, dprobs=(.45, .15, .1, .1, .199, .0005, .0005))
    src, dst, n, sc, y, pl, rl = case
    return case, B.contigs(src, dst, n, sc, pl, rl, y, 0.75)


def test_a_68000_node_graph_twice_with_a_capped_grid_in_between(lib, big):
    case, want = big
    assert 60000 < case[2] < 76000
    a = _arrays(_device(case, "bfs", 0.75))
    print("big record", dict(zip(B.COUNTERS, a["record"].tolist())), "longest", int(a["bases"].max()))
    _same(a, want, "big")
    assert int(np.diff(a["contig_ptr"]).max()) > 1024 and a["record"][2] > 0
    capped = []
    for cap in (1, 2):                        # persistent_grid: at most cap workgroups per CU -- another grid, several rounds
        assert lib.gnm_set_occupancy_cap(cap) == 0
        try:
            capped.append(_arrays(_device(case, "bfs", 0.75)))
        finally:
            assert lib.gnm_set_occupancy_cap(0) == 0
    b = _arrays(_device(case, "keep", 0.75))
    for other in capped + [b]:
        _same(other, a, "big/again")


def test_an_internal_node_order_gives_the_callers_numbering(lib, mix):
    g = _graph(mix[0], mix[1], mix[2], "bfs")
    assert "nperm" in g.index()
    _same(_arrays(_device(mix, "bfs")), _arrays(_device(mix, "keep")), "bfs vs keep")


def test_bases_do_not_wrap_in_32_bits(lib):
    big_pl = 2 ** 31 - 5
    case = (np.array([2, 0], np.int32), np.array([0, 1], np.int32), 3, np.ones(2, np.float32), np.ones(2, np.float32),
            np.array([big_pl, big_pl - 1], np.int64), np.array([2 ** 31 + 3, 2 ** 33, 11], np.int64))
    c, got = _check(case, "wide")
    assert got["walk_nodes"].tolist() == [2, 0, 1] and got["bases"].tolist() == [2 * big_pl - 1 + 2 ** 33] and c.longest() > 2 ** 33


# ---- 5. the thin call: records add, arguments are checked --------------------------------------------------------------------------------------
def test_the_record_adds_and_bad_arguments_launch_nothing(lib, mix):
    from gnnome_assembly_amd import engine
    from gnnome_assembly_amd._lib import GnmError
    from gnnome_assembly_amd.train import DecisionStats
    src, dst, n, sc, y, pl, rl = mix
    g = _graph(src, dst, n)
    E = src.size
    i32 = lambda m: torch.full((m,), -7, dtype=torch.int32, device=DEV)  # noqa: E731
    bs, bp = i32(n), i32(n)
    scd, yd = _t(sc, np.float32), _t(y, np.float32)
    DecisionStats(DEV).add(g, scd, yd, bs, bp)
    s, d = g.edges()
    base = np.arange(B.WORDS, dtype=np.int64) * 3 + 1
    rec = torch.from_numpy(base.copy()).to(DEV)
    out = dict(contig_ptr=i32(n + 1), walk_nodes=i32(n), walk_edges=i32(n), contig_bases=torch.zeros(n, dtype=torch.int64, device=DEV),
               contig_wrong=i32(n))
    args = [s, d, bs, bp, scd, yd, _t(pl, np.int64), _t(rl, np.int64), rec]
    for _ in range(2):
        engine.bog_contigs(*args, **out)
    want = B.contigs(src, dst, n, sc, pl, rl, y)
    assert np.array_equal(rec.cpu().numpy(), base + 2 * want["record"])
    C = int(want["record"][0])
    assert np.array_equal(out["contig_ptr"][:C + 1].cpu().numpy(), want["contig_ptr"])
    assert np.array_equal(out["contig_bases"][:C].cpu().numpy(), want["bases"])
    before = rec.clone()
    for change in (dict(contig_ptr=i32(n)), dict(walk_nodes=i32(n).long()), dict(contig_bases=i32(n)), dict(contig_wrong=i32(n + 1))):
        with pytest.raises(ValueError):
            engine.bog_contigs(*args, **dict(out, **change))
    for k, bad in ((4, scd[:-1]), (5, yd[:-1]), (6, _t(pl, np.int64).int()), (7, _t(rl, np.int64)[:-1]), (8, rec[:-1]), (2, bs.long())):
        with pytest.raises(ValueError):
            engine.bog_contigs(*(args[:k] + [bad] + args[k + 1:]), **out)
    with pytest.raises(GnmError):
        engine.bog_contigs(*(args[:4] + [scd.cpu()] + args[5:]), **out)
    torch.cuda.synchronize()
    assert torch.equal(rec, before)


# ---- 6. the decode side and the training loop ------------------------------------------------------------------------------------------------
def _cpu_bog(r, pl, rl):
    from gnnome_assembly_amd import decode
    t = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt)           # noqa: E731
    return decode.BogContigs(t(r["contig_ptr"], torch.int32), t(r["walk_nodes"], torch.int32), t(r["walk_edges"], torch.int32),
                             t(r["bases"], torch.int64), t(r["wrong"], torch.int32), decode.BogStats(*r["record"].tolist()),
                             t(pl, torch.int64), t(rl, torch.int64))


def test_infer_contigs_with_the_best_overlap_decoder(lib):
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
    torch.manual_seed(seed)
    plain = decode.infer_contigs(model, g, e, pe, pl, rl, nb_paths=20, len_threshold=5)
    scores, walks = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap")
    assert torch.equal(scores, plain[0])
    want = B.contigs(src, dst, n, scores.cpu().numpy(), pl, rl)
    ref = decode.resolve_strands(_cpu_bog(want, pl, rl), 3)
    print("best_overlap walks", len(walks), "of", int(want["record"][0]), "contigs; longest", max(map(len, walks), default=0))
    assert walks == ref.walks and len(walks) > 0 and all(len(w) >= 3 for w in walks)
    reads = [v >> 1 for w in walks for v in w]
    assert len(set(reads)) == len(reads)                                                       # one strand per read
    again = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap")
    assert again[1] == walks and torch.equal(again[0], scores)
    _, w2, report = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap", decision_report=True)
    assert w2 == walks and len(report) == 3


def _samples():
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


@pytest.mark.parametrize("mode", ["full_graph", "combined"])
def test_train_loop_reports_the_reference_figures_and_changes_nothing_else(lib, tmp_path, mode):
    """History.assembly_valid[k] equals the yardstick on the epoch's validation logits, recomputed in the hook with the same model
    (the forward is bit-reproducible); combined: with fused_metrics, decision_metrics and symmetry_loss (the ORIGINAL scores are
    decoded).  The hook also compares AssemblyStats at min_nodes = 2, where short contigs count.  A run with the option off gives
    the same History and parameters."""
    from dataclasses import fields
    from gnnome_assembly_amd import train as T
    hp = dict(num_epochs=2, dim_latent=128, num_gnn_layers=2, lr=1e-3, seed=0)
    if mode == "combined":
        hp.update(fused_metrics=True, decision_metrics=True, symmetry_loss=True)
    runs = []
    for on in (False, True):
        s = _samples()
        valid = s[::-1]
        want = []

        def after_epoch(epoch, model, valid=valid, want=want):
            res, st = [], T.AssemblyStats(DEV, min_nodes=2)
            with torch.no_grad():
                for v in valid:
                    px = model(v.graph, v.x, v.e, v.pe).squeeze(-1)
                    st.add(v.graph, px, v.y)
                    sv, dv = (t.cpu().numpy() for t in v.graph.edges())
                    res.append(B.contigs(sv, dv, v.graph.num_nodes(), px.cpu().numpy(), v.graph.edata["prefix_length"].cpu().numpy(),
                                         v.graph.ndata["read_length"].cpu().numpy(), v.y.cpu().numpy()))
            assert st.summary() == B.summary(res, min_nodes=2) and st.summary()[0] > 0
            want.append(B.summary(res, min_nodes=20))

        model, _, hist = T.train(s, valid, out=mode, hyperparameters=dict(hp, assembly_metrics=on), workdir=str(tmp_path / f"{on}"),
                                 verbose=False, hooks={"after_epoch": after_epoch})
        runs.append((hist, {k: v.detach().cpu() for k, v in model.state_dict().items()}))
        if not on:
            assert hist.assembly_valid == []
            continue
        assert len(hist.assembly_valid) == 2
        for ep in range(2):
            got = hist.assembly_valid[ep]
            print(mode, "epoch", ep, "assembly_valid", got)
            assert len(got) == 4 and 0.0 <= got[3] <= 1.0 and got == want[ep]
    (h0, s0), (h1, s1) = runs
    for f in fields(T.History):
        if f.name != "assembly_valid":
            assert getattr(h0, f.name) == getattr(h1, f.name), f.name
    assert set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)
