"""CPU: the overlap graph's arithmetic (csrc/gnm_overlap.h) through the host entries and find_overlaps on a CPU store against the
plain restatement of tests/overlap_reference.py: the sketch at its boundaries, seed hits and chains on hand-made runs and groups,
the error-free genome against the truth of the read positions, reads with errors against the reference, the bindings and the
refusals.  Integers, and fp32 values formed from the same two integers: every comparison is an equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import overlap_reference as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKETCH, PAIRS, CHAINS = O.sketch_cases(), O.pair_cases(), O.chain_cases()
GENOME = dict(k=15, w=5, min_hits=3, min_overlap=40)       # floor((40 - 15 + 1) / 5) = 5 >= min_hits


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(ts):
    return tuple(t.cpu().numpy() for t in ts)


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape, w.shape)
        gb, wb = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        assert np.array_equal(gb, wb), (what, i, np.flatnonzero(gb != wb)[:8], g[gb != wb][:8], w[gb != wb][:8])


def run_sketch(seqs, k, w, dev="cpu", threads=1):
    from gnnome_assembly_amd import engine
    from gnnome_assembly_amd.reads import ReadStore
    st = ReadStore.from_sequences(seqs).to(dev)
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=dev)
    out = engine.sketch(st.base_off, st.length, st.packed, k, w, rec, threads)
    return _np(out) + (rec.cpu().numpy(),)


def run_pairs(arr, lengths, k, max_occ, dev="cpu", threads=1):
    from gnnome_assembly_amd import engine
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=dev)
    out = engine.seed_pairs(*[_t(a, dev) for a in arr], _t(lengths, dev), k, max_occ, rec, threads)
    return _np(out) + (rec.cpu().numpy(),)


def run_chains(hits, lengths, band, min_hits, min_overlap, dev="cpu", threads=1):
    from gnnome_assembly_amd import engine
    rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=dev)
    out = engine.chain_pairs(_t(hits[0], dev), _t(hits[1], dev), _t(lengths, dev), band, min_hits, min_overlap, rec, threads)
    return _np(out) + (rec.cpu().numpy(),)


def run_find(seqs, dev="cpu", **kw):
    """find_overlaps -> the reference's dict layout."""
    from gnnome_assembly_amd import overlap
    from gnnome_assembly_amd.reads import ReadStore
    og = overlap.find_overlaps(ReadStore.from_sequences(seqs).to(dev), **kw)
    g = og.graph
    src, dst = g.edges()
    out = dict(src=src, dst=dst, prefix_length=g.edata["prefix_length"], overlap_length=g.edata["overlap_length"], twin=g.edata["twin"],
               contained=og.contained, record=og.record)
    if "overlap_similarity" in g.edata:
        out["overlap_similarity"] = g.edata["overlap_similarity"]
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["sketch_size"], out["hit_count"] = og.sketch_size, og.hit_count
    assert og.stats.words() == out["record"].tolist() and og.read_length.tolist() == [len(s) for s in seqs for _ in range(2)]
    return out, og


def same_graph(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        if isinstance(want[k], int):
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            same((got[k],), (want[k],), (what, k))


def ref_sketch(name):
    seqs, k, w = SKETCH[name]
    sk, rec = O.cached(("sketch", name), lambda: O.sketch(seqs, k, w))
    return sk + (O.rec_array(rec),)


def ref_pairs(name):
    arr, lengths, k, occ = PAIRS[name]
    hits, rec = O.cached(("pairs", name), lambda: O.seed_pairs(arr, lengths, k, occ))
    return hits + (O.rec_array(rec),)


def ref_chains(name):
    hits, lengths, band, mh, mo = CHAINS[name]
    out, rec = O.cached(("chains", name), lambda: O.chain_pairs(hits, lengths, band, mh, mo))
    return out + (O.rec_array(rec),)


def genome_case(rate=0.0, seed=21):
    return O.cached(("genome", rate, seed), lambda: O.genome_reads(seed=seed, rate=rate))


def ref_find(rate, **kw):
    gr = genome_case(rate)
    return O.cached(("find", rate, tuple(sorted(kw.items()))), lambda: O.find_overlaps(gr["reads"], **dict(GENOME, **kw)))


@pytest.mark.parametrize("name", list(SKETCH))
def test_sketch_equals_the_reference(lib, name):
    seqs, k, w = SKETCH[name]
    want = ref_sketch(name)
    same(run_sketch(seqs, k, w), want, name)
    same(run_sketch(seqs, k, w, threads=3), want, name + " (3 threads)")


@pytest.mark.parametrize("source", ["reference", "host entry"])
def test_sketch_cases_cover_what_they_claim(lib, source):
    """The boundary cases hold what their names say, in the reference's output and in the host entry's."""
    out = (lambda name: ref_sketch(name)) if source == "reference" else (lambda name: run_sketch(*SKETCH[name]))  # noqa: E731
    r = lambda name: dict(zip(O.COUNTERS, out(name)[4].tolist()))  # noqa: E731
    assert r("all-n")["kmers_valid"] == 90 - 15 + 1 and r("empty")["minimizers"] == 0 and r("empty")["calls"] == 1
    assert [len(s) for s in SKETCH["short"][0]] == [14, 15, 23, 24, 25]
    pal = r("palindrome")
    assert pal["kmers_valid"] < sum(len(s) - 7 for s in SKETCH["palindrome"][0])
    h, rd, ps = out("homopolymer")[:3]
    a = ps[rd == 0]                                         # equal hashes: the position breaks the tie, every window's first wins
    assert a.tolist() == list(range(0, 120 - 15 + 1 - 9)) and len(set(h[rd == 0].tolist())) == 1
    nk = [len(s) - 14 for s in SKETCH["tile"][0]]
    assert nk == [O.TILE - 1, O.TILE, O.TILE + 1, 2 * O.TILE + 40]
    assert r("k8-w1")["minimizers"] == r("k8-w1")["kmers_valid"]


@pytest.mark.parametrize("name", list(PAIRS))
def test_seed_hits_equal_the_reference(lib, name):
    want = ref_pairs(name)
    same(run_pairs(*PAIRS[name]), want, name)
    same(run_pairs(*PAIRS[name], threads=3), want, name + " (3 threads)")


@pytest.mark.parametrize("source", ["reference", "host entry"])
def test_pair_cases_cover_what_they_claim(lib, source):
    out = (lambda name: ref_pairs(name)) if source == "reference" else (lambda name: run_pairs(*PAIRS[name]))  # noqa: E731
    r = dict(zip(O.COUNTERS, out("runs")[2].tolist()))
    assert r["runs"] == 7 and r["skipped_runs"] == 1 and r["skipped_entries"] == 6 and r["same_read"] == 3 + 1
    assert r["hits"] == 10 + 5 + 1 + 1
    one = dict(zip(O.COUNTERS, out("occ1")[2].tolist()))
    assert one["hits"] == 0 and one["skipped_runs"] == 6


@pytest.mark.parametrize("name", list(CHAINS))
def test_chains_equal_the_reference(lib, name):
    want = ref_chains(name)
    same(run_chains(*CHAINS[name]), want, name)
    same(run_chains(*CHAINS[name], threads=3), want, name + " (3 threads)")


@pytest.mark.parametrize("source", ["reference", "host entry"])
def test_chain_cases_reach_every_branch(lib, source):
    out = (lambda name: ref_chains(name)) if source == "reference" else (lambda name: run_chains(*CHAINS[name]))  # noqa: E731
    src, dst, pre, ovl, val, contained, rec = out("branches")
    r = dict(zip(O.COUNTERS, rec.tolist()))
    assert r["groups"] == 13 and r["few_hits"] == 1 and r["short"] == 1 and r["contained_groups"] == 6 and r["links"] == 5
    assert contained.tolist() == [1, 0, 1, 1, 0, 1, 0]
    got = {(int(s), int(d)): (int(p), int(o)) for s, d, p, o, v in zip(src, dst, pre, ovl, val) if v}
    assert got[(0, 2)] == (400, 600) and got[(3, 1)] == (400, 600)                  # forward and its twin
    assert got[(3, 0)] == (300, 700) and got[(1, 2)] == (300, 700)                  # backward with rel = 1: node 3 -> node 0
    assert got[(6, 8)] == (20, 980)                                                 # the first of two equal windows: D = d_1 = 20
    assert got[(6, 10)] == (500, 500) and (6, 12) not in got
    assert got[(12, 10)] == (470, 530)                                              # backward: the window's median
    b0 = dict(zip(O.COUNTERS, out("band0")[6].tolist()))
    assert b0["few_hits"] > r["few_hits"] and b0["links"] >= 3


@pytest.fixture(scope="module")
def exact(lib):
    gr = genome_case(0.0)
    return gr, run_find(gr["reads"], verify=False, **GENOME)[0]


def test_error_free_reads_give_exactly_the_true_overlaps(exact):
    gr, got = exact
    want = ref_find(0.0, verify=False)
    contained, edges = O.true_overlaps(gr["truth"], GENOME["min_overlap"])
    ref_edges = sorted(zip(want["src"].tolist(), want["dst"].tolist(), want["prefix_length"].tolist(), want["overlap_length"].tolist()))
    assert ref_edges == edges and want["contained"].tolist() == contained.tolist()    # the precondition, on the reference alone
    assert len(edges) > 100 and contained.sum() > 3 and len({t[2] for t in gr["truth"]}) == 2
    got_edges = sorted(zip(got["src"].tolist(), got["dst"].tolist(), got["prefix_length"].tolist(), got["overlap_length"].tolist()))
    assert got_edges == edges and got["contained"].tolist() == contained.tolist()
    same_graph(got, want, "error-free genome")


def test_contained_reads_keep_their_edges_when_asked(lib):
    gr = genome_case(0.0)
    got, _ = run_find(gr["reads"], verify=False, drop_contained=False, **GENOME)
    _, edges = O.true_overlaps(gr["truth"], GENOME["min_overlap"], drop_contained=False)
    assert sorted(zip(got["src"].tolist(), got["dst"].tolist(), got["prefix_length"].tolist(), got["overlap_length"].tolist())) == edges
    same_graph(got, ref_find(0.0, verify=False, drop_contained=False), "contained kept")


def test_verification_drops_nothing_on_exact_overlaps(exact):
    gr, plain = exact
    got, og = run_find(gr["reads"], verify=True, max_errors=31, **GENOME)
    assert og.exceeded_pairs == 0 and (got["overlap_similarity"] == 1.0).all()
    for k in ("src", "dst", "prefix_length", "overlap_length", "twin"):
        assert np.array_equal(got[k], plain[k]), k
    assert "overlap_similarity" not in plain


def test_reads_with_errors_equal_the_reference(lib):
    gr = genome_case(0.02)
    kw = dict(verify=True, max_errors=12)
    want = ref_find(0.02, **kw)
    got, og = run_find(gr["reads"], threads=3, **dict(GENOME, **kw))
    same_graph(got, want, "2 % errors")
    _, edges = O.true_overlaps(gr["truth"], 100)
    true_pairs = {(s, d) for s, d, _, _ in edges}
    found = set(zip(got["src"].tolist(), got["dst"].tolist()))
    print(f"2 % errors: {len(found)} edges, {og.exceeded_pairs} pairs dropped by the alignment; recall of the true overlaps of >= 100 "
          f"bases: {len(true_pairs & found) / max(1, len(true_pairs)):.3f}")
    assert og.exceeded_pairs > 0 and len(found) > 50


def test_twins_and_edge_order(exact):
    _, got = exact
    E = got["src"].size
    tw = got["twin"]
    assert np.array_equal(tw[tw], np.arange(E)) and (tw != np.arange(E)).all()
    assert np.array_equal(got["src"][tw], got["dst"] ^ 1) and np.array_equal(got["dst"][tw], got["src"] ^ 1)
    assert np.array_equal(got["overlap_length"][tw], got["overlap_length"])
    key = got["src"].astype(np.int64) * 1000 + got["dst"]
    assert (np.diff(key) > 0).all()


def test_result_feeds_prepare_graph_arguments(lib):
    """prepare_graph itself has no CPU route (positional_encoding and edge_features refuse a graph that is not on a HIP device), so
    the call prepare_graph(graph, reads=store) is made in tests/test_gpu_overlap.py.  Here: the refusal, and that the graph of a
    CPU store has every field in the layout that call takes."""
    from gnnome_assembly_amd import _lib, features
    from gnnome_assembly_amd.reads import ReadStore
    gr = genome_case(0.0)
    _, og = run_find(gr["reads"], verify=True, max_errors=31, **GENOME)
    g = og.graph
    E = g.num_edges()
    assert g.num_nodes() == 2 * len(gr["reads"]) and g.edata["prefix_length"].dtype == torch.int64
    assert g.edata["overlap_length"].dtype == torch.int64 and g.edata["overlap_similarity"].dtype == torch.float32
    assert all(g.edata[k].numel() == E for k in ("prefix_length", "overlap_length", "overlap_similarity", "twin"))
    assert og.read_length.numel() == g.num_nodes() and og.contained.dtype == torch.bool
    with pytest.raises(_lib.GnmError, match="HIP device"):
        features.prepare_graph(g, reads=ReadStore.from_sequences(gr["reads"]))


def test_sources_symbols_and_abi(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib, engine, overlap
    import gnnome_assembly_amd as pkg
    assert "gnm_overlap.hip" in ge.SOURCES and pkg.overlap is overlap
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    for name in ("gnm_sketch_count", "gnm_sketch_emit", "gnm_sketch_host", "gnm_seed_pairs_count", "gnm_seed_pairs_emit",
                 "gnm_seed_pairs_host", "gnm_chain_count", "gnm_chain_pairs", "gnm_chain_pairs_host", "gnm_sketch_tile_bound",
                 "gnm_overlap_scan_workspace_bytes"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct gnm_overlap_record" in hdr and "#define GNM_ABI_VERSION 7" in hdr and lib.gnm_abi_version() == 7
    assert f"#define GNM_SKETCH_TILE {O.TILE}" in hdr and engine.SKETCH_TILE == O.TILE
    assert engine.OVERLAP_COUNTERS == O.COUNTERS and engine.OVERLAP_RECORD_WORDS == 14
    assert tuple(overlap.OverlapStats.__dataclass_fields__) == engine.OVERLAP_COUNTERS
    assert {"find_overlaps", "sketch", "OverlapGraph"} <= set(overlap.__all__)
    sk = overlap.sketch(__import__("gnnome_assembly_amd.reads", fromlist=["ReadStore"]).ReadStore.from_sequences(SKETCH["tile"][0]), 15, 25)
    same((sk.hash.numpy(), sk.read.numpy(), sk.pos.numpy(), sk.strand.numpy(), sk.record.numpy()), ref_sketch("tile"), "overlap.sketch")


def test_refusals(lib):
    from gnnome_assembly_amd import engine, overlap
    from gnnome_assembly_amd.reads import ReadStore
    rec = (C.c_int64 * 14)()
    a = (C.c_int64 * 8)()
    tot = C.c_int64(0)
    sk = dict(packed=a, packed_bytes=32, base_off=a, length=a, R=1, k=15, w=5, cap=-1, hash=None, read=None, pos=None, strand=None,
              total=C.byref(tot), rec=rec, threads=1)
    assert lib.gnm_sketch_host(*sk.values()) == 0 and tot.value == 0
    odd = C.c_void_p(C.addressof(rec) + 4)
    for change in (dict(k=7), dict(k=32), dict(w=0), dict(w=65), dict(R=-1), dict(R=2 ** 31 - 1), dict(packed_bytes=24),
                   dict(packed=None), dict(base_off=None), dict(rec=None), dict(rec=odd), dict(total=None), dict(threads=0),
                   dict(cap=0, R=1, length=(C.c_int64 * 1)(2 ** 31 - 1))):
        assert lib.gnm_sketch_host(*dict(sk, **change).values()) < 0, change
        assert lib.gnm_last_error()
    dev = dict(packed=a, packed_bytes=32, base_off=a, length=a, R=1, k=15, w=5, tile_ptr=a, tile_off=a, tb=1, rec=rec, ws=None, wsb=0,
               stream=None)
    for change in (dict(k=7), dict(w=65), dict(rec=odd), dict(rec=None), dict(tile_ptr=None), dict(tb=5), dict(R=2 ** 31 - 1)):
        assert lib.gnm_sketch_count(*dict(dev, **change).values()) < 0, change      # refused before anything is launched
    pr = dict(M=2, hash=a, read=a, pos=a, strand=a, length=a, R=1, k=15, occ=4, cap=-1, key=None, diag=None, total=C.byref(tot), rec=rec,
              threads=1)
    assert lib.gnm_seed_pairs_host(*pr.values()) == 0
    for change in (dict(occ=0), dict(occ=4097), dict(M=-1), dict(hash=None), dict(pos=None), dict(length=None), dict(rec=odd),
                   dict(k=3), dict(threads=2000)):
        assert lib.gnm_seed_pairs_host(*dict(pr, **change).values()) < 0, change
    assert lib.gnm_seed_pairs_count(2, a, a, 0, a, rec, None, 0, None) < 0 and lib.gnm_seed_pairs_count(2, a, a, 4, a, odd, None, 0, None) < 0
    ch = dict(N=2, key=a, diag=a, length=a, R=1, band=32, mh=4, mo=500, cap=-1, src=None, dst=None, pre=None, ovl=None, valid=None,
              contained=None, total=C.byref(tot), rec=rec, threads=1)
    assert lib.gnm_chain_pairs_host(*ch.values()) == 0 and tot.value == 1
    for change in (dict(band=-1), dict(mh=0), dict(mo=-1), dict(N=-1), dict(key=None), dict(length=None), dict(rec=None), dict(rec=odd),
                   dict(cap=1), dict(threads=0)):
        assert lib.gnm_chain_pairs_host(*dict(ch, **change).values()) < 0, change
    assert lib.gnm_chain_pairs(2, a, a, a, 1, a, 1, -1, 4, 500, a, a, a, a, a, a, rec, None) < 0
    assert lib.gnm_chain_count(2, a, a, odd, None, 0, None) < 0
    assert list(rec) == [0] * 14                            # a refused or size-only call leaves the record as it is
    st = ReadStore.from_sequences(["ACGTACGTACGTACGTACGTACGT", "GTAAGTAAGTAAGTAAGTAAGTAACC"])
    for kw in (dict(k=7), dict(k=32), dict(k=True), dict(w=0), dict(w=65), dict(w=2.0), dict(max_occ=0), dict(max_occ=4097),
               dict(min_hits=0), dict(band=-1), dict(min_overlap=-1), dict(verify=1), dict(drop_contained=None)):
        with pytest.raises(ValueError):
            overlap.find_overlaps(st, **kw)
    with pytest.raises(ValueError, match="max_errors"):
        overlap.find_overlaps(ReadStore.from_sequences(genome_case(0.0)["reads"][:12]), max_errors=256, **GENOME)
    with pytest.raises(TypeError):
        overlap.find_overlaps(["ACGT"])
    with pytest.raises(ValueError, match="rec"):
        engine.sketch(st.base_off, st.length, st.packed, 15, 5, torch.zeros(8, dtype=torch.int64))
