"""GPU: gnm_transitive_support (engine.transitive_support, decode.transitive_support, the reduce_transitive switch of
decode.best_overlap_contigs / greedy_cover_contigs / infer_contigs and of train.AssemblyStats) against the plain-Python yardstick of
tests/reduce_reference.py.  support, the bits of masked_scores (NaN positions included) and the record are integers: every case
asserts EQUALITY, there is no tolerance in this file.

Shapes.  A workgroup serves 32 source nodes per pass and a node takes eight lanes: n = 31, 32, 33 sit around the first, out-degrees
8, 9 and 17 around the lane stride; the second step is found by a binary search in b's row, so rows of 1, 2 and 33 entries hold c
first, last, twice and not at all.  The 68,000-node graph gives the kernel several workgroups and, under an occupancy cap, several
grid passes."""
import numpy as np
import pytest
import torch

import bog_reference as B
import cover_reference as R
import reduce_reference as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
COVER_ARRAYS = ("record", "contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong", "link_succ", "link_pred")


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


def _device(src, dst, n, sc, pl, y=None, min_logit=-INF, fuzz=None, node_order=None):
    """decode.transitive_support -> (support int64, masked bits uint32, record int64) on the host."""
    from gnnome_assembly_amd import decode
    r = decode.transitive_support(_graph(src, dst, n, node_order), _t(sc, np.float32), _t(pl, np.int64),
                                  None if y is None else _t(y, np.float32), min_logit, fuzz)
    torch.cuda.synchronize()
    assert r.support.dtype == torch.int32 and r.masked_scores.dtype == torch.float32 and r.support.is_cuda
    got = (r.support.cpu().numpy().astype(np.int64), r.masked_scores.cpu().numpy().view(np.uint32),
           np.asarray(r.stats.words(), np.int64))
    return got


def _same(got, want, what=""):
    assert np.array_equal(got[0], want["support"]), (what, "support", got[0][:20], want["support"][:20])
    assert np.array_equal(got[1], want["masked_bits"]), (what, "masked", got[1][:20], want["masked_bits"][:20])
    assert np.array_equal(got[2], want["record"]), (what, "record", got[2], want["record"])


def _check(src, dst, n, sc, pl, y=None, min_logit=-INF, fuzz=None, what="", orders=(None,), want=None):
    if want is None:
        want = T.reduce(src, dst, n, sc, pl, y, min_logit, fuzz)
    for order in orders:
        got = _device(src, dst, n, sc, pl, y, min_logit, fuzz, order)
        print(what, order, dict(zip(T.COUNTERS, got[2].tolist())))
        _same(got, want, (what, order))
    return want


def _random(n, E, seed, nan=0.1):
    """Random endpoints (self loops and parallel edges among them), scores with NaN and -inf, prefixes from a small range so that
    equal prefixes and exact sums happen, labels 0 / 1 / NaN."""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, max(n, 1), E).astype(np.int32), rng.integers(0, max(n, 1), E).astype(np.int32)
    sc = rng.standard_normal(E).astype(np.float32)
    sc[rng.random(E) < nan] = NAN
    sc[rng.random(E) < 0.05] = -INF
    y = np.array([0.0, 1.0, NAN], np.float32)[rng.integers(0, 3, E)]
    return src, dst, n, sc, rng.integers(1, 12, E).astype(np.int64), y


# ---- 1. the smallest inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 31, 32, 33])
def test_around_one_workgroup_pass_with_and_without_edges(lib, n):
    e = np.zeros(0, np.int32)
    got = _device(e, e, n, np.zeros(0, np.float32), np.zeros(0, np.int64))
    assert got[0].size == 0 and got[1].size == 0 and got[2].tolist() == [0] * 8      # nothing launched, nothing counted
    if n == 0:
        return
    for seed, (fuzz, ml) in enumerate(((None, -INF), (0, -INF), (3, -0.25))):
        src, dst, n_, sc, pl, y = _random(n, 6 * n, 10 * n + seed)
        want = _check(src, dst, n, sc, pl, y, ml, fuzz, f"n={n}/{seed}", orders=("bfs", "keep"))
        assert n < 3 or want["record"][2] > 0 or fuzz == 0


@pytest.mark.parametrize("d", [8, 9, 17])
def test_out_degrees_around_the_lane_stride(lib, d):
    """Node 0 has d out-edges: to 1 .. m = d - 1 at prefixes 10, 20, .., and a second copy of 0 -> m at prefix 10 m + 5; node i has
    the edge i -> i+1 at prefix 10.  Edge 0 -> i+1 has the one witness 0 -> i, with or without the length test (only i -> i+1
    enters i+1); the second copy has the same witness without the test and none under fuzz 0."""
    m = d - 1
    src = [0] * m + list(range(1, m)) + [0]
    dst = list(range(1, m + 1)) + list(range(2, m + 1)) + [m]
    pl = [10 * i for i in range(1, m + 1)] + [10] * (m - 1) + [10 * m + 5]
    rng = np.random.default_rng(d)
    p = rng.permutation(len(src))
    src, dst, pl = np.asarray(src, np.int32)[p], np.asarray(dst, np.int32)[p], np.asarray(pl, np.int64)[p]
    sc = rng.standard_normal(src.size).astype(np.float32)
    for fuzz in (0, None):
        want = _check(src, dst, m + 1, sc, pl, None, -INF, fuzz, f"d={d}/fuzz={fuzz}", orders=("bfs", "keep"))
        hub = want["support"][src == 0]
        assert hub.size == d and sorted(hub.tolist()) == ([0, 0] + [1] * (m - 1) if fuzz == 0 else [0] + [1] * m)
        assert want["record"][5] == 1


@pytest.mark.parametrize("row", [1, 2, 33])
@pytest.mark.parametrize("where", ["first", "last", "absent", "twice"])
def test_the_binary_search_in_the_second_steps_row(lib, row, where):
    """a = 0, b = 1: b's row has `row` out-edges to distinct nodes of 2 .. ; c is the first, the last or none of them, or (twice)
    the last with a parallel copy whose score is NaN placed so that the equal-range scan must pass it to reach the live one (the
    row is then one entry longer).  Node order "keep" keeps the row in this order; "bfs" renumbers it."""
    targets = list(range(2, 2 + row))                       # b's destinations, ascending
    c = {"first": targets[0], "last": targets[-1], "absent": 2 + row, "twice": targets[-1]}[where]
    n = 4 + row
    src = [0, 0] + [1] * row
    dst = [1, c] + targets
    pl = [10, 20] + [10] * row
    sc = [1.0, 1.0] + [1.0] * row
    if where == "twice":                                    # the copy with the LOWER position in the row is dead
        src.insert(2, 1); dst.insert(2, c); pl.insert(2, 10); sc.insert(2, NAN)
        assert dst[2] == c and len(src) == row + 3
    for fuzz in (None, 0):
        want = _check(src, dst, n, sc, pl, None, -INF, fuzz, f"row={row}/{where}", orders=("keep", "bfs"))
        assert want["support"][1] == (0 if where == "absent" else 1) and want["support"].sum() == want["support"][1]


@pytest.mark.parametrize("row", T.HAND, ids=[r[0] for r in T.HAND])
def test_hand_cases(lib, row):
    src, dst, n, sc, pl, ml, fuzz, support, reduced = T.hand_case(row)
    got = _device(src, dst, n, sc, pl, None, ml, fuzz)
    assert got[0].tolist() == support.tolist()
    assert ((got[1] == 0x7FC00000) & ~np.isnan(sc)).tolist() == reduced.tolist()
    _same(got, T.reduce(src, dst, n, sc, pl, None, ml, fuzz), row[0])
    _same(_device(src, dst, n, sc, pl, None, ml, fuzz, "bfs"), T.reduce(src, dst, n, sc, pl, None, ml, fuzz), row[0])


def test_a_nan_keeps_its_own_bits_and_a_reduced_edge_gets_the_quiet_nan(lib):
    src, dst, n, sc, pl = [0, 1, 0, 0], [1, 2, 2, 2], 3, np.array([1, 1, 1, 0], np.float32), [10, 10, 20, 25]
    bits = sc.view(np.uint32)
    bits[3] = 0xFFC12345                                     # a NaN with a payload and a sign: no candidate, passed through
    got = _device(src, dst, n, sc, pl)
    assert got[0].tolist() == [0, 0, 1, 1] and [hex(v) for v in got[1].tolist()] == ["0x3f800000", "0x3f800000", "0x7fc00000", "0xffc12345"]
    assert got[2].tolist() == [4, 3, 1, 0, 2, 1, 0, 1]


@pytest.mark.parametrize("node_order", ["bfs", "keep"])
def test_the_tiny_edge_case_graph(lib, node_order):
    from gnnome_assembly_amd import synth
    src, dst, n = synth.tiny_edge_case_graph()
    rng = np.random.default_rng(8)
    sc = rng.standard_normal(src.size).astype(np.float32)
    sc[rng.random(src.size) < 0.1] = NAN
    y = (rng.random(src.size) < 0.5).astype(np.float32)
    for fuzz, ml, pl in ((None, -INF, rng.integers(1, 40, src.size)), (4, -0.5, rng.integers(1, 12, src.size)),
                         (0, -INF, 2 ** 40 + rng.integers(-6, 6, src.size)), (2, -INF, -rng.integers(1, 12, src.size))):
        want = _check(src, dst, n, sc, pl.astype(np.int64), y, ml, fuzz, f"tiny/{fuzz}", orders=(node_order,))
        assert want["record"][6] >= 6 and (fuzz == 0 or want["record"][2] > 0) and want["record"][5] >= (2 if fuzz is None else 0)


def test_prefixes_around_two_to_the_forty(lib):
    """The chain graph with its positions scaled by 2^28: the prefixes reach past 2^40 and the triangles stay exact.  One base more
    on every edge that is not a nearest-neighbour edge breaks the triangles of the i -> i+2 edges (two nearest-neighbour steps) and
    of no other: at 2^40, one base off is off."""
    src, dst, n, sc, pl, rl, near = T.chain(60, seed=5)
    want = _check(src, dst, n, sc, pl << 28, None, -INF, 0, "2^40", orders=("bfs",))
    assert int((pl << 28).max()) > 2 ** 40 and ((want["support"] == 0) == near).all()
    off = _check(src, dst, n, sc, (pl << 28) + (~near).astype(np.int64), None, -INF, 0, "2^40 + 1")
    assert 0 < off["record"][2] < want["record"][2] and off["record"][4] < want["record"][4]


# ---- 2. several workgroups and grid passes; reproducibility; the record adds ---------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """68,000 nodes: synth.make_graph at mean degree 3 with shuffled edge ids, length-consistent prefixes with a few bases of noise,
    NaN and -inf scores; and the yardstick on it, computed once."""
    from gnnome_assembly_amd import synth
    src, dst, n = synth.make_graph(34000, seed=6, mean_degree=3.0, permute_edge_ids=True)
    rng = np.random.default_rng(6)
    sc = rng.standard_normal(src.size).astype(np.float32)
    sc[rng.random(src.size) < 0.03] = NAN
    pl, rl = T.synth_prefixes(src, dst, n, 6, jitter=3)
    y = (rng.random(src.size) < 0.8).astype(np.float32)
    return (src, dst, n, sc, pl, y), T.reduce(src, dst, n, sc, pl, y, -1.0, 4)


def test_a_68000_node_graph_twice_with_a_capped_grid_in_between(lib, big):
    (src, dst, n, sc, pl, y), want = big
    assert n == 68000 and want["record"][2] > 1000 and want["record"][5] >= 2 and want["record"][3] > 0
    a = _device(src, dst, n, sc, pl, y, -1.0, 4, "bfs")
    _same(a, want, "big")
    others = []
    for cap in (1, 2):                        # persistent_grid: at most cap workgroups per CU -- another grid, several passes
        assert lib.gnm_set_occupancy_cap(cap) == 0
        try:
            others.append(_device(src, dst, n, sc, pl, y, -1.0, 4, "bfs"))
        finally:
            assert lib.gnm_set_occupancy_cap(0) == 0
    others.append(_device(src, dst, n, sc, pl, y, -1.0, 4, "bfs"))
    others.append(_device(src, dst, n, sc, pl, y, -1.0, 4, "keep"))
    for o in others:
        for x, z in zip(a, o):
            assert np.array_equal(x, z)


def test_the_record_adds_over_two_calls_and_max_support_is_a_maximum(lib):
    from gnnome_assembly_amd import engine
    cases = [_random(40, 400, 1, nan=0.0), _random(33, 120, 2)]
    rec = torch.zeros(engine.REDUCE_RECORD_WORDS, dtype=torch.int64, device=DEV)
    wants = []
    for src, dst, n, sc, pl, y in cases:
        g = _graph(src, dst, n)
        sup = torch.full((src.size,), -7, dtype=torch.int32, device=DEV)
        engine.transitive_support(g.index(), _t(sc, np.float32), _t(pl, np.int64), _t(y, np.float32), -INF, None, sup, None, rec)
        wants.append(T.reduce(src, dst, n, sc, pl, y))
        assert np.array_equal(sup.cpu().numpy(), wants[-1]["support"])           # masked_scores is optional
    a, b = (w["record"] for w in wants)
    assert a[5] > b[5] > 0                                                       # the second call's maximum is the smaller one
    total = a + b
    total[5] = max(a[5], b[5])
    assert rec.cpu().tolist() == total.tolist() and total[7] == 2
    with pytest.raises(ValueError, match="masked_scores must not be the scores"):
        s = _t(cases[0][3], np.float32)
        engine.transitive_support(_graph(*cases[0][:3]).index(), s, _t(cases[0][4], np.int64), None, -INF, None,
                                  torch.zeros(400, dtype=torch.int32, device=DEV), s, rec)


# ---- 3. composition with the decoders ------------------------------------------------------------------------------------------------
def _cover_arrays(c):
    h = c.host()
    out = {k: h[k].astype(np.int64) for k in ("contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong")}
    out["record"] = np.asarray(c.stats.words(), np.int64)
    if hasattr(c, "link_succ"):
        out["link_succ"], out["link_pred"] = c.link_succ.cpu().numpy().astype(np.int64), c.link_pred.cpu().numpy().astype(np.int64)
        out["rounds"], out["round_links"], out["converged"] = c.rounds, list(c.round_links), c.converged
    return out


def _same_cover(got, want, what=""):
    for k in COVER_ARRAYS:
        if k in got:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, got[k][:20], want[k][:20])
    if "rounds" in got:
        assert (got["rounds"], got["round_links"], got["converged"]) == (want["rounds"], want["round_links"], want["converged"]), what


@pytest.fixture(scope="module")
def overlap_graph():
    """synth.make_graph at 400 reads with consistent prefixes, scores with NaN, labels."""
    from gnnome_assembly_amd import synth
    src, dst, n = synth.make_graph(400, seed=12, permute_edge_ids=True)
    rng = np.random.default_rng(12)
    sc = rng.standard_normal(src.size).astype(np.float32)
    sc[rng.random(src.size) < 0.03] = NAN
    pl, rl = T.synth_prefixes(src, dst, n, 12)
    return src, dst, n, sc, pl, rl, (rng.random(src.size) < 0.8).astype(np.float32)


@pytest.mark.parametrize("fuzz,min_logit", [(None, -INF), (0, -INF), (0, -0.5)])
def test_the_cover_decoders_behind_the_reduction_equal_the_composed_yardstick(lib, overlap_graph, fuzz, min_logit):
    from gnnome_assembly_amd import decode
    src, dst, n, sc, pl, rl, y = overlap_graph
    args = (_graph(src, dst, n, "bfs"), _t(sc, np.float32), _t(pl, np.int64), _t(rl, np.int64), _t(y, np.float32), min_logit)
    c = decode.greedy_cover_contigs(*args, reduce_transitive=True, fuzz=fuzz)
    want = T.cover(src, dst, n, sc, pl, rl, y, min_logit, fuzz)
    _same_cover(_cover_arrays(c), want, "greedy_cover")
    assert c.reduce_stats.words() == want["reduce_record"].tolist() and 0 < c.reduce_stats.reduced_fraction < 1
    b = decode.best_overlap_contigs(*args, reduce_transitive=True, fuzz=fuzz)
    wb = T.cover(src, dst, n, sc, pl, rl, y, min_logit, fuzz, best_overlap=True)
    _same_cover(_cover_arrays(b), wb, "best_overlap")
    assert b.reduce_stats.words() == wb["reduce_record"].tolist()
    plain = R.contigs(src, dst, n, sc, pl, rl, y, min_logit)
    print("greedy cover: contigs", int(plain["record"][0]), "->", int(want["record"][0]), "longest (nodes)",
          int(np.diff(plain["contig_ptr"]).max()), "->", int(np.diff(want["contig_ptr"]).max()))
    assert np.diff(want["contig_ptr"]).max() > np.diff(plain["contig_ptr"]).max()


def test_the_switch_off_is_the_call_without_it(lib, overlap_graph):
    from gnnome_assembly_amd import decode
    src, dst, n, sc, pl, rl, y = overlap_graph
    args = (_graph(src, dst, n, "bfs"), _t(sc, np.float32), _t(pl, np.int64), _t(rl, np.int64), _t(y, np.float32))
    for fn in (decode.greedy_cover_contigs, decode.best_overlap_contigs):
        a, b = fn(*args), fn(*args, reduce_transitive=False, fuzz=3)
        ga, gb = _cover_arrays(a), _cover_arrays(b)
        assert set(ga) == set(gb) and not hasattr(a, "reduce_stats") and not hasattr(b, "reduce_stats")
        _same_cover(gb, ga, fn.__name__)
    _same_cover(_cover_arrays(decode.greedy_cover_contigs(*args)), R.contigs(src, dst, n, sc, pl, rl, y), "plain")


@pytest.mark.parametrize("seed", [0, 1])
def test_a_chain_of_overlaps_becomes_one_contig_per_strand_whatever_the_scores(lib, seed):
    from gnnome_assembly_amd import decode
    reads = 150
    src, dst, n, sc, pl, rl, near = T.chain(reads, seed=seed)
    got = _device(src, dst, n, sc, pl, None, -INF, 0, "bfs")
    assert ((got[0] == 0) == near).all() and ((got[1] == 0x7FC00000) == ~near).all()
    _same(got, T.reduce(src, dst, n, sc, pl, None, -INF, 0), "chain")
    c = decode.greedy_cover_contigs(_graph(src, dst, n, "bfs"), _t(sc, np.float32), _t(pl, np.int64), _t(rl, np.int64),
                                    reduce_transitive=True, fuzz=0)
    assert c.num_nodes().cpu().tolist() == [reads, reads] and c.stats.cycles_cut == 0
    walks = c.walks()
    assert walks[0] == list(range(0, 2 * reads, 2)) and walks[1] == list(range(2 * reads - 1, 0, -2))
    plain = decode.greedy_cover_contigs(_graph(src, dst, n, "bfs"), _t(sc, np.float32), _t(pl, np.int64), _t(rl, np.int64))
    assert len(plain) > 2                                    # the same scores without the reduction: parallel contigs


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------
def _cpu_bog(r, pl, rl):
    from gnnome_assembly_amd import decode
    t = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt)           # noqa: E731
    return decode.BogContigs(t(r["contig_ptr"], torch.int32), t(r["walk_nodes"], torch.int32), t(r["walk_edges"], torch.int32),
                             t(r["bases"], torch.int64), t(r["wrong"], torch.int32), decode.BogStats(*r["record"].tolist()),
                             t(pl, torch.int64), t(rl, torch.int64))


def test_infer_contigs_with_the_reduction_through_to_sequences(lib):
    import seq_reference as S
    from gnnome_assembly_amd import AssemblyGraph, decode, models, synth
    from gnnome_assembly_amd.reads import ReadStore
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
    reads = S.random_reads(rng, rng.integers(3200, 4000, n // 2))
    rl = np.array([len(r) for r in reads], np.int64)[np.arange(n) >> 1]
    start = np.cumsum(rng.integers(20, 200, n // 2)).astype(np.int64)      # a read overlaps its next 16 or more
    pl = np.abs(start[dst >> 1] - start[src >> 1])
    pl = np.minimum(pl, rl[src])                                           # the few long-range edges: a prefix inside the read
    store = ReadStore.from_sequences(reads).to(DEV)
    scores, walks, seqs = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="greedy_cover", reads=store,
                                               reduce_transitive=True, fuzz=0)
    plain = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="greedy_cover")
    assert torch.equal(scores, plain[0])                                   # the scores returned are the model's, not the masked ones
    want = T.cover(src, dst, n, scores.cpu().numpy(), pl, rl, None, -INF, 0)
    ref = decode.resolve_strands(_cpu_bog(want, pl, rl), 3)
    print("reduced greedy_cover walks", len(walks), "longest", max(map(len, walks), default=0), "; plain:", len(plain[1]), "longest",
          max(map(len, plain[1]), default=0))
    assert walks == ref.walks and len(walks) > 0
    assert len(seqs) == len(walks) and seqs.record.invalid == 0 and seqs.lengths.tolist() == ref.bases
    dg = decode.DecodeGraph(src, dst, n)
    _, _, wedges = decode.walk_edge_ids(dg, walks)
    ptr = np.concatenate([[0], np.cumsum([len(w) for w in walks])])
    strings, _ = S.contig_strings(walks, [wedges[ptr[i]:ptr[i + 1]].tolist() for i in range(len(walks))], pl, reads)
    assert seqs.bases.cpu().numpy().tobytes().decode() == "".join(strings)
    b = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap", reduce_transitive=True)
    wb = T.cover(src, dst, n, scores.cpu().numpy(), pl, rl, None, -INF, None, best_overlap=True)
    assert b[1] == decode.resolve_strands(_cpu_bog(wb, pl, rl), 3).walks


# ---- 5. the training loop --------------------------------------------------------------------------------------------------------------
def _samples():
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    from gnnome_assembly_amd.train import GraphSample
    out = []
    for reads, seed in ((300, 11), (280, 12)):
        src, dst, n = synth.make_graph(reads, seed=seed)
        inp = synth.make_inputs(src, dst, n, seed=seed)
        pl, rl = T.synth_prefixes(src, dst, n, seed, jitter=2)
        g = G.AssemblyGraph(src, dst, n).to(DEV)
        g.edata["prefix_length"] = torch.from_numpy(pl).to(DEV)
        g.ndata["read_length"] = torch.from_numpy(rl).to(DEV)
        out.append(GraphSample(g, torch.from_numpy(inp["e"]).to(DEV), torch.from_numpy(inp["pe"]).to(DEV),
                               torch.from_numpy(inp["y"]).to(DEV)))
    return out


def test_train_loop_with_the_hyperparameter_on(lib, tmp_path):
    """History.assembly_valid[k] equals the composed yardstick on the epoch's validation logits, recomputed in the hook with the same
    model (the forward is bit-reproducible); every other History field and every parameter equals the run with the switch off."""
    from dataclasses import fields
    from gnnome_assembly_amd import train as TR
    hp = dict(num_epochs=2, dim_latent=128, num_gnn_layers=2, lr=1e-3, seed=0, assembly_metrics=True, assembly_decoder="greedy_cover")
    runs = []
    for extra in ({}, dict(assembly_reduce_transitive=True, assembly_reduce_fuzz=2)):
        s = _samples()
        valid = s[::-1]
        want = []

        def after_epoch(epoch, model, valid=valid, want=want, on=bool(extra)):
            res = []
            with torch.no_grad():
                for v in valid:
                    px = model(v.graph, v.x, v.e, v.pe).squeeze(-1)
                    sv, dv = (t.cpu().numpy() for t in v.graph.edges())
                    a = (sv, dv, v.graph.num_nodes(), px.cpu().numpy(), v.graph.edata["prefix_length"].cpu().numpy(),
                         v.graph.ndata["read_length"].cpu().numpy(), v.y.cpu().numpy())
                    res.append(T.cover(*a, fuzz=2) if on else R.contigs(*a))
            want.append(B.summary(res, min_nodes=20))

        model, _, hist = TR.train(s, valid, out="m", hyperparameters=dict(hp, **extra), workdir=str(tmp_path / f"{len(runs)}"),
                                  verbose=False, hooks={"after_epoch": after_epoch})
        runs.append((hist, {k: v.detach().cpu() for k, v in model.state_dict().items()}))
        assert len(hist.assembly_valid) == 2
        for ep in range(2):
            print(extra, "epoch", ep, "assembly_valid", hist.assembly_valid[ep])
            assert hist.assembly_valid[ep] == want[ep]
    (h0, s0), (h1, s1) = runs
    assert h0.assembly_valid != h1.assembly_valid
    for f in fields(TR.History):
        if f.name != "assembly_valid":
            assert getattr(h0, f.name) == getattr(h1, f.name), f.name
    assert set(s0) == set(s1) and all(torch.equal(s0[k], s1[k]) for k in s0)
