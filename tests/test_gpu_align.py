"""GPU: gnm_overlap_align through features.overlap_features against the dynamic programme of tests/align_reference.py and against
the host entry point (the cases of test_align_cpu.py, outputs and record equal); one edge, an edge count that is no multiple of
the workgroup, two grid sizes; prepare_graph(reads=...), decode.junction_identity and infer_contigs(junction_report=True) on a
small graph cut from one genome, whose exact overlaps have distance 0 and similarity 1."""
import numpy as np
import pytest
import torch

import align_reference as A
from test_align_cpu import assert_same, host_align

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = A.all_cases()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)


def device_align(store, n, src, dst, pl, K):
    """features.overlap_features -> (dist, overlap_length, similarity, record) on the host."""
    from gnnome_assembly_amd import AssemblyGraph, features
    g = AssemblyGraph(src, dst, n).to(DEV)
    f = features.overlap_features(g, store.to(DEV), _t(pl, np.int64), K)
    assert f.overlap_similarity.device == DEV and torch.equal(f.exceeded, f.edit_distance > K)
    st = f.stats
    rec = f.record.cpu().numpy()
    assert [st.edges, st.aligned, st.exceeded, st.empty, st.clamped, st.invalid, st.cells, st.calls] == rec.tolist()
    return f.edit_distance.cpu().numpy(), f.overlap_length.cpu().numpy(), f.overlap_similarity.cpu().numpy(), rec


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_dynamic_programme_and_the_host_entry(lib, name):
    case = CASES[name]
    store, want = A.reference(case)
    _, _, n, src, dst, pl, K = case
    got = device_align(store, n, src, dst, pl, K)
    assert_same(got, want, name)
    assert_same(got, host_align(store, n, src, dst, pl, K), name + " (host entry)")


def test_one_edge(lib):
    _, _, n, src, dst, pl, K = CASES["random-K40"]
    store, want = A.reference(CASES["random-K40"])
    for k in (0, 9):                                        # an overlap, and a pair without one
        got = device_align(store, n, src[k:k + 1], dst[k:k + 1], pl[k:k + 1], K)
        assert got[0][0] == want[0][k] and got[1][0] == want[1][k] and got[2][0] == want[2][k] and got[3][0] == 1


@pytest.fixture(scope="module")
def genome(lib):
    from gnnome_assembly_amd import AssemblyGraph
    from gnnome_assembly_amd.reads import ReadStore
    gg = A.genome_graph()
    g = AssemblyGraph(gg["src"], gg["dst"], gg["n"]).to(DEV)
    g.edata["prefix_length"] = _t(gg["prefix_length"], np.int64)
    return gg, g, ReadStore.from_sequences(gg["reads"]).to(DEV)


def test_exact_overlaps_have_distance_zero_and_similarity_one(genome):
    from gnnome_assembly_amd import features
    gg, g, store = genome
    E = gg["src"].size
    assert 3.0 <= E / gg["n"] <= 4.0 and E % 256 != 0 and E > 256          # mean degree ~4; no multiple of the workgroup
    f = features.overlap_features(g, store, max_errors=31)
    assert int(f.edit_distance.abs().max()) == 0 and bool((f.overlap_similarity == 1.0).all()) and not bool(f.exceeded.any())
    rl = np.array([len(r) for r in gg["reads"]], np.int64)[gg["src"] >> 1]
    assert f.overlap_length.cpu().tolist() == (rl - gg["prefix_length"]).tolist()
    assert f.stats.aligned == E == f.stats.edges and f.stats.clamped == f.stats.invalid == f.stats.empty == 0


def test_reads_with_errors_against_the_host_entry_and_two_grid_sizes(lib):
    from gnnome_assembly_amd.reads import ReadStore
    gg = A.genome_graph(seed=5, rate=0.04)
    store = ReadStore.from_sequences(gg["reads"])
    K = 20
    want = host_align(store, gg["n"], gg["src"], gg["dst"], gg["prefix_length"], K, threads=4)
    r = dict(zip(A.COUNTERS, want[3].tolist()))
    assert r["aligned"] > 100 and r["exceeded"] > 100, r
    assert_same(device_align(store, gg["n"], gg["src"], gg["dst"], gg["prefix_length"], K), want, "genome, 4 % errors")
    rep = 48                                                # more blocks of edges than one workgroup per CU: the grids differ
    src, dst, pl = np.tile(gg["src"], rep), np.tile(gg["dst"], rep), np.tile(gg["prefix_length"], rep)
    assert src.size > 256 * 256
    try:
        lib.gnm_set_occupancy_cap(1)
        one = device_align(store, gg["n"], src, dst, pl, K)
    finally:
        lib.gnm_set_occupancy_cap(0)
    full = device_align(store, gg["n"], src, dst, pl, K)
    assert_same(one, full, "one workgroup per CU against the full grid")
    for g_, w in zip(full[:3], want[:3]):
        assert np.array_equal(g_.view(np.int32) if g_.dtype == np.float32 else g_, np.tile(w.view(np.int32) if w.dtype == np.float32 else w, rep))
    assert full[3].tolist() == [rep * v for v in want[3][:7]] + [1]


def test_prepare_graph_fills_the_edge_features_from_the_reads(lib):
    from gnnome_assembly_amd import AssemblyGraph, features
    from gnnome_assembly_amd.reads import ReadStore
    gg = A.genome_graph(seed=5, rate=0.04)                  # reads with errors: the similarity varies, its z-score exists
    g0 = AssemblyGraph(gg["src"], gg["dst"], gg["n"]).to(DEV)
    g0.edata["prefix_length"] = _t(gg["prefix_length"], np.int64)
    store = ReadStore.from_sequences(gg["reads"]).to(DEV)
    fresh = lambda: AssemblyGraph(gg["src"], gg["dst"], gg["n"]).to(DEV)  # noqa: E731
    g = fresh()
    g.edata["prefix_length"] = g0.edata["prefix_length"]
    x, e, pe = features.prepare_graph(g, reads=store, max_errors=31)
    f = features.overlap_features(g, store, max_errors=31)
    assert torch.equal(g.edata["overlap_length"], f.overlap_length) and torch.equal(g.edata["overlap_similarity"], f.overlap_similarity)
    assert torch.equal(e, features.edge_features(f.overlap_length, f.overlap_similarity)) and torch.equal(g.edata["e"], e)
    assert bool(torch.isfinite(e).all()) and f.stats.exceeded > 0 and f.stats.aligned > 0
    # the feature already present: left untouched, and the result is the one without reads
    g2 = fresh()
    g2.edata["prefix_length"] = g0.edata["prefix_length"]
    given_len, given_sim = f.overlap_length + 3, torch.full_like(f.overlap_similarity, 0.5) + f.overlap_similarity * 0.25
    g2.edata["overlap_length"], g2.edata["overlap_similarity"] = given_len.clone(), given_sim.clone()
    x2, e2, pe2 = features.prepare_graph(g2, reads=store)
    assert torch.equal(g2.edata["overlap_length"], given_len) and torch.equal(g2.edata["overlap_similarity"], given_sim)
    g3 = fresh()
    g3.edata["overlap_length"], g3.edata["overlap_similarity"] = given_len.clone(), given_sim.clone()
    x3, e3, pe3 = features.prepare_graph(g3)
    assert torch.equal(e2, e3) and torch.equal(pe2, pe3) and torch.equal(x2, x3) and torch.equal(pe, pe3)
    g4 = fresh()                                            # reads=None and no feature: no e, as before
    g4.edata["prefix_length"] = g0.edata["prefix_length"]
    x4, e4, pe4 = features.prepare_graph(g4, reads=None)
    assert e4 is None and "overlap_similarity" not in g4.edata and torch.equal(pe4, pe3)
    with pytest.raises(Exception, match="is on cpu"):
        features.overlap_features(g, store.to("cpu"))


def test_junction_identity_equals_a_loop_over_the_walk_edges(lib):
    from gnnome_assembly_amd import AssemblyGraph, decode
    from gnnome_assembly_amd.reads import ReadStore
    gg = A.genome_graph(seed=6, rate=0.03)
    K = 12
    g = AssemblyGraph(gg["src"], gg["dst"], gg["n"]).to(DEV)
    g.edata["prefix_length"] = _t(gg["prefix_length"], np.int64)
    store = ReadStore.from_sequences(gg["reads"]).to(DEV)
    rl = np.array([len(r) for r in gg["reads"]], np.int64)[np.arange(gg["n"]) >> 1]
    scores = _t(np.random.default_rng(6).standard_normal(gg["src"].size), np.float32)
    bog = decode.best_overlap_contigs(g, scores, gg["prefix_length"], rl)
    ji = decode.junction_identity(bog, g, store, max_errors=K)
    dist = ji.features.edit_distance.cpu().numpy()
    h = bog.host()
    want = []
    for c in range(len(bog)):
        edges = h["walk_edges"][h["contig_ptr"][c] + 1:h["contig_ptr"][c + 1]]
        want.append((len(edges), int(dist[edges].sum()), int((dist[edges] > K).sum())))
    got = list(zip(ji.junctions.tolist(), ji.edit_distance.tolist(), ji.exceeded.tolist()))
    assert got == want and sum(w[0] for w in want) > 20 and sum(w[2] for w in want) > 0 and any(0 < w[1] for w in want)
    walks = bog.walks(min_nodes=2)                          # the list route: edge ids looked up on the host
    jl = decode.junction_identity(walks, g, store, max_errors=K)
    multi = [w for w in want if w[0] > 0]
    assert list(zip(jl.junctions.tolist(), jl.edit_distance.tolist(), jl.exceeded.tolist())) == multi


def test_infer_contigs_attaches_the_junction_record_only_when_asked(lib):
    from gnnome_assembly_amd import AssemblyGraph, decode, features, models, synth
    from gnnome_assembly_amd.reads import ReadStore
    gg = A.genome_graph(seed=8, rate=0.02)
    g = AssemblyGraph(gg["src"], gg["dst"], gg["n"]).to(DEV)
    g.edata["prefix_length"] = _t(gg["prefix_length"], np.int64)
    store = ReadStore.from_sequences(gg["reads"]).to(DEV)
    rl = np.array([len(r) for r in gg["reads"]], np.int64)[np.arange(gg["n"]) >> 1]
    H, L = 128, 2
    model = models.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, seed=8).items()})
    model.to(DEV)
    _, e, pe = features.prepare_graph(g, reads=store, max_errors=40)
    kw = dict(len_threshold=2, decoder="best_overlap")
    three = decode.infer_contigs(model, g, e, pe, gg["prefix_length"], rl, reads=store, **kw)
    four = decode.infer_contigs(model, g, e, pe, gg["prefix_length"], rl, reads=store, junction_report=True, **kw)
    assert len(three) == 3 and len(four) == 4 and four[1] == three[1] and torch.equal(four[2].bases, three[2].bases)
    ji = four[3]
    assert isinstance(ji, decode.JunctionIdentity) and ji.junctions.tolist() == [len(w) - 1 for w in four[1]]
    with pytest.raises(ValueError, match="needs reads"):
        decode.infer_contigs(model, g, e, pe, gg["prefix_length"], rl, junction_report=True, **kw)
