"""GPU: the overlap graph's kernels (csrc/gnm_overlap.hip) against tests/overlap_reference.py and against the host entries -- the
cases of test_overlap_cpu.py, arrays and record equal; a store of one read; a replicated store whose minimizer, hit and group counts
are no multiple of the workgroup and exceed one scan block; occupancy caps and repeated runs; and the error-free genome end to end:
find_overlaps -> prepare_graph -> model -> infer_contigs, and the greedy cover of the true overlaps against the genome."""
import numpy as np
import pytest
import torch

import overlap_reference as O
from seq_reference import revcomp
from test_overlap_cpu import (CHAINS, GENOME, PAIRS, SKETCH, genome_case, ref_chains, ref_find, ref_pairs, ref_sketch, run_chains,
                              run_find, run_pairs, run_sketch, same, same_graph)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", list(SKETCH))
def test_sketch_on_the_device(lib, name):
    seqs, k, w = SKETCH[name]
    got = run_sketch(seqs, k, w, DEV)
    same(got, ref_sketch(name), name)
    same(got, run_sketch(seqs, k, w), name + " (host entry)")


@pytest.mark.parametrize("name", list(PAIRS))
def test_seed_hits_on_the_device(lib, name):
    got = run_pairs(*PAIRS[name], DEV)
    same(got, ref_pairs(name), name)
    same(got, run_pairs(*PAIRS[name]), name + " (host entry)")


@pytest.mark.parametrize("name", list(CHAINS))
def test_chains_on_the_device(lib, name):
    got = run_chains(*CHAINS[name], DEV)
    same(got, ref_chains(name), name)
    same(got, run_chains(*CHAINS[name]), name + " (host entry)")


@pytest.mark.parametrize("M", [0, 1, 255, 256, 257, 256 * 256 + 1])   # the scan block B = 256: B - 1, B, B + 1; 257 scan blocks
def test_seed_hit_offsets_at_the_scan_block_edges(lib, M):
    """Runs of two entries (2j, 2j + 1) of reads a < b on one strand, pos = (j, 0): the scanned counts are 0, 1, 0, 1, .. and hit j
    has diag j, so a wrong offset moves a hit.  Closed form, and the host entry on the same arrays."""
    i = np.arange(M)
    a = 2 * ((i // 2) % 500)
    arr = (i // 2, (a + i % 2).astype(np.int32), np.where(i % 2 == 0, i // 2, 0).astype(np.int32), np.zeros(M, np.uint8))
    lengths = np.full(1000, 5000, np.int64)
    got = run_pairs(arr, lengths, 15, 16, DEV)
    N = M // 2
    aj = 2 * (np.arange(N, dtype=np.int64) % 500)
    rec = np.zeros(len(O.COUNTERS), np.int64)
    rec[O.COUNTERS.index("runs")], rec[O.COUNTERS.index("hits")] = (M + 1) // 2, N
    same(got, ((aj << 32) | ((aj + 1) << 1), np.arange(N, dtype=np.int32), rec), f"M = {M}")
    same(got, run_pairs(arr, lengths, 15, 16), f"M = {M} (host entry)")


def test_a_store_of_one_read(lib):
    seqs = [SKETCH["tile"][0][3]]
    got = run_sketch(seqs, 15, 25, DEV)
    same(got, run_sketch(seqs, 15, 25), "one read")
    assert got[4][O.COUNTERS.index("minimizers")] == got[0].size > 50
    res, og = run_find(seqs, DEV, **GENOME)
    assert og.graph.num_edges() == 0 and og.graph.num_nodes() == 2 and og.hit_count == 0 and not bool(og.contained.any())


@pytest.mark.parametrize("rate,kw", [(0.0, dict(verify=False)), (0.0, dict(verify=True, max_errors=31)),
                                     (0.02, dict(verify=True, max_errors=12))])
def test_find_overlaps_on_the_device(lib, rate, kw):
    gr = genome_case(rate)
    got, _ = run_find(gr["reads"], DEV, **dict(GENOME, **kw))
    same_graph(got, ref_find(rate, **kw), f"genome, rate {rate}")
    same_graph(got, run_find(gr["reads"], **dict(GENOME, **kw))[0], f"genome, rate {rate} (host entries)")


def test_replicated_store_grids_and_repeats(lib):
    """Every read six times: counts past one scan block and off the workgroup size, the same bits under every grid and twice."""
    from gnnome_assembly_amd.graph import induce_scan_block
    gr = genome_case(0.02)
    seqs = gr["reads"] * 6
    kw = dict(GENOME, max_occ=256, verify=True, max_errors=12)
    want, og = run_find(seqs, threads=8, **kw)              # the host entries
    blk = induce_scan_block()
    for count in (og.sketch_size, og.hit_count, og.stats.groups):
        assert count > blk and count % 256 != 0, (count, blk)
    assert og.stats.skipped_runs == 0 and og.stats.contained_groups > 0 and og.stats.links > 0 and og.exceeded_pairs > 0
    runs = []
    try:
        for cap in (1, 2):
            lib.gnm_set_occupancy_cap(cap)
            runs.append(run_find(seqs, DEV, **kw)[0])
    finally:
        lib.gnm_set_occupancy_cap(0)
    runs += [run_find(seqs, DEV, **kw)[0], run_find(seqs, DEV, **kw)[0]]
    for i, got in enumerate(runs):
        same_graph(got, want, f"replicated store, run {i}")


def test_end_to_end_on_the_error_free_genome(lib):
    from gnnome_assembly_amd import decode, features, models, overlap, synth
    from gnnome_assembly_amd.reads import ReadStore
    gr = genome_case(0.0)
    store = ReadStore.from_sequences(gr["reads"]).to(DEV)
    og = overlap.find_overlaps(store, verify=True, max_errors=31, **GENOME)
    g = og.graph
    assert g.device == DEV and g.num_edges() > 100
    pl = g.edata["prefix_length"]
    x, e, pe = features.prepare_graph(g, reads=store)
    # every similarity is 1 here, so the z-score of that column has no spread to divide by; the length column is finite
    assert e.shape == (g.num_edges(), 2) and bool(torch.isfinite(e[:, 0]).all()) and pe.shape[0] == g.num_nodes()
    H, L = 128, 2
    model = models.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, seed=8).items()})
    model.to(DEV)
    scores, walks, seqs = decode.infer_contigs(model, g, e, pe, pl, og.read_length, len_threshold=2, decoder="greedy_cover", reads=store)
    assert scores.numel() == g.num_edges() and isinstance(seqs, decode.ContigSequences) and len(seqs) == len(walks)
    # the same route on reads with errors, whose similarities vary: finite features, finite scores, walks with bases
    noisy = ReadStore.from_sequences(genome_case(0.02)["reads"]).to(DEV)
    og2 = overlap.find_overlaps(noisy, verify=True, max_errors=40, **GENOME)
    g2 = og2.graph
    _, e2, pe2 = features.prepare_graph(g2, reads=noisy)
    assert bool(torch.isfinite(e2).all()) and g2.num_edges() > 100
    s2, w2, q2 = decode.infer_contigs(model, g2, e2, pe2, g2.edata["prefix_length"], og2.read_length, len_threshold=2,
                                      decoder="greedy_cover", reads=noisy)
    assert bool(torch.isfinite(s2).all()) and len(w2) > 0 and len(q2) == len(w2) and all(len(q2.sequence(c)) > 0 for c in range(len(q2)))
    # scores from the TRUTH of the read positions: a true overlap scores its true length, any other edge -1e4
    _, edges = O.true_overlaps(gr["truth"], GENOME["min_overlap"])
    true_len = {(s, d): ov for s, d, _, ov in edges}
    src, dst = (t.cpu().tolist() for t in g.edges())
    truth = torch.tensor([float(true_len.get(sd, -1e4)) for sd in zip(src, dst)], dtype=torch.float32, device=DEV)
    assert int((truth > 0).sum()) == len(edges) == g.num_edges()
    cover = decode.greedy_cover_contigs(g, truth, pl, og.read_length)
    spelled = decode.contig_sequences(cover, g, store, pl)
    genome, rc = gr["genome"], revcomp(gr["genome"])
    longest = 0
    for c in range(len(spelled)):
        s = spelled.sequence(c)
        assert s in genome or s in rc, (c, len(s))
        longest = max(longest, len(s))
    assert longest > 900                                    # longer than any read: reads were joined
