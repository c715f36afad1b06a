"""GPU: decode.resolve_strands_device (gnm_resolve.hip) against the host's decode.resolve_strands on the same contigs -- the lists of
.resolved() -- and against the numpy round formulation (tests/resolve_reference.py) for the raw tensors, the record and the
rounds.  Integers, compared for equality."""
import numpy as np
import pytest
import torch

import resolve_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)


def _check(cover, thr, y=None, what="", **kw):
    """Device == host lists, device tensors / record / rounds == the round formulation; returns the device result."""
    from gnnome_assembly_amd import decode
    got = decode.resolve_strands_device(R.to_contigs(cover, DEV), thr, None if y is None else _t(y, np.float32), **kw)
    torch.cuda.synchronize()
    want = decode.resolve_strands(R.to_contigs(cover), thr)
    res = got.resolved()
    assert res.walks == want.walks and res.bases == want.bases, (what, thr, res.walks, want.walks)
    ref = R.resolve_rounds(cover, thr, y)
    h = got.host()
    for k, r in (("contig_ptr", "contig_ptr"), ("walk_nodes", "walk_nodes"), ("walk_edges", "walk_edges"), ("bases", "piece_bases"),
                 ("wrong", "wrong")):
        assert h[k].tolist() == ref[r].tolist(), (what, thr, k)
    assert got.stats.words() == ref["record"], (what, thr, got.stats, ref["record"])
    assert isinstance(got, decode.BogContigs) and len(got) == len(want.walks)
    starts = np.zeros(h["walk_nodes"].size, np.bool_)
    starts[h["contig_ptr"][:-1]] = True
    assert np.array_equal(h["walk_edges"] == -1, starts), (what, thr)
    if kw.get("check_every", decode.RESOLVE_CHECK_EVERY) == 1:
        assert got.rounds == ref["rounds"], (what, thr, got.rounds, ref["rounds"])
    else:
        assert got.rounds >= ref["rounds"], (what, thr, got.rounds, ref["rounds"])
    return got


@pytest.mark.parametrize("thr", [1, 2, 3, 4, 5, 6])
def test_the_hand_cases(lib, thr):
    for i, cover in enumerate(R.hand_cases()):
        _check(cover, thr, what=f"hand {i}", check_every=1)


def test_fifty_random_covers(lib):
    """Covers 0 .. 49 of the CPU test's set, with labels on every other one; rounds compared with check_every=1."""
    deep = serial = 0
    for seed in range(50):
        cover = R.random_cover(seed)
        y = (np.random.default_rng(seed).random(cover["prefix_length"].size) < 0.8).astype(np.float32) if seed % 2 else None
        for thr in (1, 2, 3, 5):
            got = _check(cover, thr, y, what=f"random {seed}", check_every=1 if thr != 3 else 4)
            deep += got.rounds >= 3
            serial += got.stats.serial
    assert deep > 0 and serial > 0


def _with_twin(L, taken_at, pad=70):
    """Contig A: nodes 2i for i < L.  Contig B, of higher priority: the other strand of A's reads at positions `taken_at`, then
    `pad` reads of its own, so that it is kept at every threshold used here and takes exactly those reads of A."""
    a = [2 * i for i in range(L)]
    b = [2 * i + 1 for i in sorted(taken_at)] + [2 * (L + j) for j in range(pad)]
    cover = R.cover_from_paths([a, b], 2 * (L + pad), seed=L)
    cover["bases"] = np.array([10, 20], np.int64)      # the priority key only: B first
    return cover


@pytest.mark.parametrize("thr", [1, 2, 64, 65])
@pytest.mark.parametrize("L", [63, 64, 65, 256, 257, 1025])
def test_runs_that_open_close_and_reach_the_threshold_at_a_chunk_boundary(lib, L, thr):
    at = lambda *ps: {p for p in ps if 0 <= p < L}     # noqa: E731
    for taken_at in (at(0, 62, 63, 64, 65, 255, 256, 257, L - 1), at(0, 65, 130, 195, L - 1), at(0, 66, 132), at(63), at(64), at(L - 1),
                     at(1, 66, 130, 193), set()):
        got = _check(_with_twin(L, taken_at), thr, what=f"L {L} taken {sorted(taken_at)}")
        assert got.stats.serial == 0 and got.stats.eligible == (2 if L >= thr else 1)


@pytest.mark.parametrize("check_every", [1, 3])
def test_a_dependency_chain_of_depth_five(lib, check_every):
    """Contig k holds the other strand of a read of contig k - 1, and bases fall strictly: contig k waits for k - 1."""
    paths = []
    for k in range(5):
        p = [2 * (10 * k + j) for j in range(8)]
        if k:
            p.insert(4, 2 * (10 * (k - 1) + 3) + 1)
        paths.append(p)
    cover = R.cover_from_paths(paths, 100, order=[3, 0, 4, 2, 1])
    cover["bases"] = np.array([50 - 10 * k for k in (3, 0, 4, 2, 1)], np.int64)
    for thr in (1, 4, 5):
        got = _check(cover, thr, what="chain", check_every=check_every)
        assert got.rounds >= 5


def test_a_contig_that_visits_a_read_twice_is_cut_serially(lib):
    """130 nodes: reads 0 .. 99, read 40 again on its other strand, reads 100 .. 128.  A contig of higher priority takes reads 10,
    12, 14, 120 and 122: kept and dropped pieces on either side of the second visit."""
    a = [2 * i for i in range(100)] + [81] + [2 * i for i in range(100, 129)]
    b = [21, 25, 29, 241, 245]
    assert len(a) == 130
    cover = R.cover_from_paths([a, b], 260, seed=3)
    cover["bases"] = np.array([10, 20], np.int64)
    for thr in (1, 2, 5, 21, 86, 90, 131):
        got = _check(cover, thr, what="serial")
        assert got.stats.serial == (1 if thr <= 130 else 0)
    got = _check(cover, 5)
    assert [len(w) for w in got.walks()] == [5, 10, 85, 20, 6] and got.stats.dropped == 3


def test_empty_and_short_covers(lib):
    empty = dict(contig_ptr=np.zeros(1, np.int32), walk_nodes=np.zeros(0, np.int32), walk_edges=np.zeros(0, np.int32),
                 bases=np.zeros(0, np.int64), prefix_length=np.zeros(0, np.int64), read_length=np.ones(4, np.int64), n=4)
    got = _check(empty, 1, what="empty")
    assert len(got) == 0 and got.contig_ptr.tolist() == [0] and got.walk_nodes.numel() == 0 == got.bases.numel()
    cover = R.hand_cases()[0]
    got = _check(cover, 6, what="threshold above the longest contig")
    assert len(got) == 0 and got.contig_ptr.tolist() == [0] and got.walk_nodes.numel() == 0 and got.stats.eligible == 0
    assert got.walks() == [] and got.n50() == 0 and got.longest() == 0
    short = R.cover_from_paths([[v] for v in range(9)] + [[10, 12], [11, 13]], 14)
    got = _check(short, 3, what="every contig short")
    assert len(got) == 0 and got.stats.contigs == 11


@pytest.mark.parametrize("C", [1, 1023, 1024, 1025, 256 * 1024 + 1])   # the scan block B = 1024: B - 1, B, B + 1; 257 scan blocks
def test_contig_counts_at_the_scan_block_edges(lib, C):
    """Contig c holds nodes 4c, 4c + 2 when c is even and node 4c alone when it is odd; bases rise with c, so the priority order is
    the reverse of the input order.  At threshold 2 the scanned sequences are 2, 0, 2, 0, .. nodes and 1, 0, 1, 0, .. pieces in that
    order: the even contigs come out whole, last first, and every output has a closed form."""
    from gnnome_assembly_amd import decode
    c = np.arange(C)
    lens = np.where(c % 2 == 0, 2, 1)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    nodes, edges = np.empty(ptr[-1], np.int64), np.full(ptr[-1], -1, np.int64)
    nodes[ptr[:-1]] = 4 * c
    even = c[c % 2 == 0]
    nodes[ptr[even] + 1], edges[ptr[even] + 1] = 4 * even + 2, even // 2
    pl, rl = np.arange(even.size, dtype=np.int64) * 5 + 1, np.arange(4 * C, dtype=np.int64) + 50
    cover = dict(contig_ptr=ptr.astype(np.int32), walk_nodes=nodes.astype(np.int32), walk_edges=edges.astype(np.int32),
                 bases=c.astype(np.int64) + 1, prefix_length=pl, read_length=rl, n=4 * C)
    got = decode.resolve_strands_device(R.to_contigs(cover, DEV), 2)
    torch.cuda.synchronize()
    kept = even[::-1]
    K = kept.size
    h = got.host()
    assert got.stats.words() == [C, K, K, 0, 2 * K, 0, 0, 1] and got.rounds == 1
    assert np.array_equal(h["contig_ptr"], 2 * np.arange(K + 1))
    assert np.array_equal(h["walk_nodes"], np.stack([4 * kept, 4 * kept + 2], 1).reshape(-1))
    assert np.array_equal(h["walk_edges"], np.stack([np.full(K, -1), kept // 2], 1).reshape(-1))
    assert np.array_equal(h["bases"], pl[kept // 2] + rl[4 * kept + 2]) and not h["wrong"].any()
    assert len(got) == K and got.walk_nodes.numel() == 2 * K


def test_invalid_input_raises_and_counts(lib):
    from gnnome_assembly_amd import decode
    from gnnome_assembly_amd._lib import GnmError
    cover = R.cover_from_paths([[0, 2, 4], [6, 2, 8]], 10)                       # node 2 listed twice
    with pytest.raises(GnmError, match="listed twice") as e:
        decode.resolve_strands_device(R.to_contigs(cover, DEV), 1)
    assert e.value.record.invalid == 1 and e.value.record.pieces == 0 and e.value.record.nodes == 0
    cover = R.cover_from_paths([[0, 2, 4], [6, 8]], 10)
    cover["walk_nodes"][3] = 10                                                  # node id == n
    with pytest.raises(GnmError, match="out of range") as e:
        decode.resolve_strands_device(R.to_contigs(cover, DEV), 1)
    assert e.value.record.invalid == 1
    cover = R.cover_from_paths([[0, 2, 4], [6, 8]], 10)
    cover["walk_edges"][1] = 3                                                   # inner edge id == E
    with pytest.raises(GnmError) as e:
        decode.resolve_strands_device(R.to_contigs(cover, DEV), 1)
    assert e.value.record.invalid == 1


def test_a_capped_grid_and_a_second_run_give_the_same_bits(lib):
    from gnnome_assembly_amd import decode
    covers = [(R.random_cover(7), 2), (_with_twin(1025, {0, 64, 511, 1024}), 64)]
    for cover, thr in covers:
        y = _t(np.random.default_rng(1).random(cover["prefix_length"].size) < 0.5, np.float32)
        runs = [decode.resolve_strands_device(R.to_contigs(cover, DEV), thr, y)]
        assert lib.gnm_set_occupancy_cap(1) == 0
        try:
            runs.append(decode.resolve_strands_device(R.to_contigs(cover, DEV), thr, y))
        finally:
            assert lib.gnm_set_occupancy_cap(0) == 0
        runs.append(decode.resolve_strands_device(R.to_contigs(cover, DEV), thr, y))
        for other in runs[1:]:
            for k in ("contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong"):
                assert torch.equal(getattr(runs[0], k), getattr(other, k)), k
            assert runs[0].stats.words() == other.stats.words() and runs[0].rounds == other.rounds
        assert len(runs[0]) > 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_case(lib):
    import seq_reference as S
    from gnnome_assembly_amd import AssemblyGraph, synth
    from gnnome_assembly_amd.reads import ReadStore
    src, dst, n = synth.make_graph(2000, seed=6)
    rng = np.random.default_rng(6)
    reads = S.random_reads(rng, rng.integers(100, 400, (n + 1) // 2))
    rl = np.array([len(r) for r in reads], np.int64)[np.arange(n) >> 1]
    pl = (rng.random(src.size) * rl[src]).astype(np.int64)
    g = AssemblyGraph(src, dst, n).to(DEV)
    g.edata["prefix_length"] = _t(pl, np.int64)
    scores = _t(rng.standard_normal(src.size), np.float32)
    y = _t(rng.random(src.size) < 0.7, np.float32)
    return g, scores, y, pl, rl, ReadStore.from_sequences(reads).to(DEV)


@pytest.mark.parametrize("reduce_transitive", [False, True])
@pytest.mark.parametrize("decoder", ["best_overlap_contigs", "greedy_cover_contigs"])
def test_the_cover_decoders_end_to_end(synth_case, decoder, reduce_transitive):
    from gnnome_assembly_amd import decode
    g, scores, y, pl, rl, store = synth_case
    cover = getattr(decode, decoder)(g, scores, pl, rl, y, reduce_transitive=reduce_transitive)
    for thr in (2, 3):
        want = decode.resolve_strands(cover, thr)
        got = decode.resolve_strands_device(cover, thr, y)
        res = got.resolved()
        assert res.walks == want.walks and res.bases == want.bases and len(want.walks) > 0
        assert got.stats.contigs == len(cover) and got.stats.pieces == len(want.walks) and got.stats.invalid == 0
        h = got.host()
        inner = h["walk_edges"] >= 0
        wrong = np.add.reduceat(np.where(inner, y.cpu().numpy()[h["walk_edges"].clip(0)] != 1, False).astype(np.int64), h["contig_ptr"][:-1])
        assert h["wrong"].tolist() == wrong.tolist()
    a = decode.contig_sequences(got, g, store)                        # the device CSR as it is
    b = decode.contig_sequences(want.walks, g, store)                 # lists: edge ids looked up on the host
    assert torch.equal(a.bases, b.bases) and torch.equal(a.contig_ptr, b.contig_ptr) and a.record.words() == b.record.words()
    assert a.record.bases > 0 and a.lengths.tolist() == want.bases


@pytest.mark.parametrize("reduce_transitive", [False, True])
@pytest.mark.parametrize("decoder", ["best_overlap", "greedy_cover"])
def test_infer_contigs_with_device_resolve(synth_case, decoder, reduce_transitive):
    """infer_contigs on the 2000-read graph with a stand-in model that returns the fixed-seed logits: device_resolve=True gives the
    walks, the sequence bytes and the junction report of device_resolve=False."""
    from gnnome_assembly_amd import decode
    g, scores, _, pl, rl, store = synth_case

    class FixedLogits(torch.nn.Module):
        def forward(self, graph, x, e, pe):
            return scores[:, None]

    kw = dict(len_threshold=3, decoder=decoder, reduce_transitive=reduce_transitive)
    host = decode.infer_contigs(FixedLogits(), g, None, None, pl, rl, reads=store, junction_report=True, **kw)
    dev = decode.infer_contigs(FixedLogits(), g, None, None, pl, rl, reads=store, junction_report=True, device_resolve=True, **kw)
    assert len(host) == len(dev) == 4 and torch.equal(host[0], dev[0]) and host[1] == dev[1] and len(host[1]) > 0
    assert torch.equal(host[2].bases, dev[2].bases) and torch.equal(host[2].contig_ptr, dev[2].contig_ptr)
    assert host[2].record.words() == dev[2].record.words() and dev[2].record.bases > 0
    for k in ("junctions", "edit_distance", "exceeded"):
        assert torch.equal(getattr(host[3], k), getattr(dev[3], k)), k
    plain = decode.infer_contigs(FixedLogits(), g, None, None, pl, rl, device_resolve=True, **kw)
    assert len(plain) == 2 and plain[1] == host[1]
