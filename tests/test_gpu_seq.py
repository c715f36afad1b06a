"""GPU: gnm_seq_layout / gnm_seq_emit (engine.seq_layout, engine.seq_emit, decode.contig_sequences) against the string yardstick
of tests/seq_reference.py.  The outputs are bytes and integer counters: every case asserts EQUALITY, there is no tolerance in
this file.

Shapes.  A lane writes 16 bases and a workgroup owns B = engine.SEQ_CHUNK_BASES of them: single pieces of 1, 15, 16, 17, B-1, B,
B+1 and 3B+5 bases sit at and around both; a 1-base contig in front makes every later destination odd against its source; runs
of 0- and 1-base pieces put many pieces into one lane's 16 bases."""
import numpy as np
import pytest
import torch

import seq_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def B(lib):
    from gnnome_assembly_amd import engine
    return engine.SEQ_CHUNK_BASES


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)


class _N:
    """The graph as far as the CSR route needs it: a node count."""

    def __init__(self, n):
        self._n, self.edata = n, {}

    def num_nodes(self):
        return self._n


def _csr(walks, wedges, pl):
    """A BogContigs holding exactly these walks and edge ids on the device (the layout gnm_bog_contigs leaves)."""
    from gnnome_assembly_amd import decode
    ptr = np.cumsum([0] + [len(w) for w in walks])
    flat = lambda ll: [v for w in ll for v in w]                       # noqa: E731
    return decode.BogContigs(_t(ptr, np.int32), _t(flat(walks), np.int32), _t(flat(wedges), np.int32), None, None, None,
                             _t(pl, np.int64), None)


def _device(walks, wedges, pl, reads, n=None, store=None):
    from gnnome_assembly_amd import decode
    from gnnome_assembly_amd.reads import ReadStore
    st = store if store is not None else ReadStore.from_sequences(reads).validate().to(DEV)
    cs = decode.contig_sequences(_csr(walks, wedges, pl), _N(2 * len(reads) if n is None else n), st)
    torch.cuda.synchronize()
    return cs


def _check(walks, wedges, pl, reads, what="", **kw):
    cs = _device(walks, wedges, pl, reads, **kw)
    want, rec = S.contig_strings(walks, wedges, pl, reads)
    print(what, "record", dict(zip(S.COUNTERS, cs.record.words())))
    assert cs.record.words() == [rec[k] for k in S.COUNTERS], (what, cs.record.words(), rec)
    assert cs.lengths.tolist() == [len(s) for s in want], what
    got = cs.bases.cpu().numpy().tobytes().decode("ascii")
    assert len(got) == rec["bases"] and got == "".join(want), (what, [(i, a, b) for i, (a, b) in enumerate(zip(got, "".join(want))) if a != b][:5])
    assert cs.bases.is_cuda and cs.bases.dtype == torch.uint8 and cs.contig_ptr.is_cuda and cs.contig_ptr.dtype == torch.int64
    pad = cs.bases.untyped_storage()
    assert pad.nbytes() % 16 == 0 and pad.nbytes() - rec["bases"] < 16            # whole 16-byte groups ...
    whole = torch.empty(0, dtype=torch.uint8, device=DEV).set_(pad)
    assert int(whole[rec["bases"]:].sum()) == 0                                    # ... and the tail is zero
    for c in range(min(len(want), 3)):
        assert cs.sequence(c) == want[c]
    return cs


def _reads(seed, lengths, p_plain=0.8):
    return S.random_reads(np.random.default_rng(seed), lengths, p_plain=p_plain)


# ---- 1. one piece, at the lane and chunk sizes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["1", "15", "16", "17", "B-1", "B", "B+1", "3*B+5"])
def test_a_single_piece_contig(lib, B, size):
    n = eval(size, {"B": B})
    reads = _reads(n, [n])
    _check([[0]], [[-1]], [], reads, f"fwd {size}")
    _check([[1]], [[-1]], [], reads, f"rev {size}")


@pytest.mark.parametrize("odd_dst", [False, True])
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("odd_len", [False, True])
def test_destination_parity_strand_and_read_parity(lib, B, odd_dst, rev, odd_len):
    """A 1-base contig in front shifts every later base to an odd destination: the lane's window of the store then starts on a
    half byte (forward) or ends on one (reverse)."""
    n = B + 70 + int(odd_len)
    reads = _reads(17 + 2 * odd_len, [n, 1, 37 + int(odd_len)])
    walks = ([[2]] if odd_dst else []) + [[0 + rev], [4 + rev, 0 + rev]]
    wedges = ([[-1]] if odd_dst else []) + [[-1], [-1, 0]]
    _check(walks, wedges, [20 + int(odd_len)], reads, f"odd_dst={odd_dst} rev={rev} odd_len={odd_len}")


# ---- 2. empty pieces, tiny pieces, contig shapes ------------------------------------------------------------------------------------------
def test_empty_pieces_first_last_inner_and_in_runs(lib, B):
    reads = _reads(5, [300, 41, 77, 5, 1, 2, 64])
    pl = [0, 1, 30, 41, 2, 5]
    first = [0, 2, 4]                                      # its first position contributes nothing
    last_inner = [2, 4, 0, 6]                              # ... its last inner position
    rng = np.random.default_rng(9)
    run = [int(v) for v in rng.integers(0, 14, 44)]        # 40 consecutive 0- and 1-base pieces between two real ones
    run_e = [-1, 2] + [int(v) for v in rng.integers(0, 2, 40)] + [3, 2]
    only_empty = [3, 5, 7]
    cs = _check([first, last_inner, run, only_empty], [[-1, 0, 2], [-1, 2, 3, 0], run_e, [-1, 0, 0]], pl, reads, "empties")
    assert cs.record.empty >= 20


def test_more_scan_blocks_than_threads(lib):
    """P = 256 * 256 + 3 pieces of one to three bases in one contig: 257 block sums, so a thread of the scan workgroup owns two of
    them, the last threads own none and the last block holds three pieces."""
    rng = np.random.default_rng(14)
    reads = _reads(14, rng.integers(3, 7, 40))
    P = 256 * 256 + 3
    walk = rng.integers(0, 2 * len(reads), P).tolist()
    wedges = [-1] + rng.integers(0, 3, P - 1).tolist()
    cs = _check([walk], [wedges], [1, 2, 3], reads, "P = 256 * 256 + 3")
    assert cs.record.pieces == P and cs.record.clamped == 0 and cs.record.empty == 0


def test_a_contig_of_one_node_and_empty_contigs(lib):
    reads = _reads(6, [33, 0, 18])
    cs = _check([[4], [], [2], [3], [1, 5]], [[-1], [], [-1], [-1], [-1, 0]], [9], reads, "one node / empty")
    assert cs.lengths.tolist() == [18, 0, 0, 0, 9 + 18]


def test_no_contig_at_all(lib):
    from gnnome_assembly_amd import decode, engine
    reads = _reads(7, [10])
    cs = _check([], [], [], reads, "C = 0")
    assert len(cs) == 0 and cs.bases.numel() == 0 and cs.contig_ptr.tolist() == [0] and cs.record.calls == 1
    cs = _check([[], []], [[], []], [5], reads, "two empty contigs")
    assert cs.bases.numel() == 0 and cs.contig_ptr.tolist() == [0, 0, 0]
    # the emit pass on an empty extent launches nothing: it does not even look at its pointers
    none = torch.empty(0, dtype=torch.uint8, device=DEV)
    st = _device([], [], [], reads)
    engine.seq_emit(torch.empty(0, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 2,
                    torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), none, 0, none)
    assert isinstance(st, decode.ContigSequences)


def test_a_contig_boundary_inside_a_chunk_and_a_piece_over_three_chunks(lib, B):
    reads = _reads(8, [B // 2 + 3, 2 * B + 900, 700, B // 3])
    # contig 0 ends inside chunk 0; contig 1 starts there with a piece that covers the rest of chunk 0, chunk 1 and part of chunk 2
    walks, wedges, pl = [[0], [2, 4, 7], [3, 6]], [[-1], [-1, 0, 1], [-1, 2]], [2 * B + 850, 699, 2 * B + 900]
    cs = _check(walks, wedges, pl, reads, "boundaries")
    off = cs.piece_off.tolist()
    assert off[1] < B and off[2] > 2 * B and off[1] // B == 0 and (off[2] - 1) // B == 2


def test_prefixes_outside_the_read_are_clamped_and_counted(lib):
    reads = _reads(10, [50, 60, 70, 80])
    pl = [-1, 51, 50, 0, 10 ** 12, -(10 ** 12), 61]
    walks, wedges = [[0, 2, 4, 6, 1], [3, 5, 7, 0]], [[-1, 0, 1, 2, 4], [-1, 6, 5, 3]]
    cs = _check(walks, wedges, pl, reads, "clamp")
    # into positions: node 0 gets pl[0] = -1 (clamped), 2: pl[1] = 51 (fits 60), 4: pl[2] = 50, 6: pl[4] = 1e12 (clamped);
    # node 3: pl[6] = 61 > 60 (clamped), 5: pl[5] = -1e12 (clamped), 7: pl[3] = 0 (empty, not clamped)
    assert cs.record.clamped == 4 and cs.record.empty == 3


@pytest.mark.parametrize("what", ["node", "read", "edge"])
def test_an_id_out_of_range_raises_and_emits_nothing(lib, what):
    from gnnome_assembly_amd._lib import GnmError
    reads = _reads(11, [40, 50, 60])
    walks, wedges, pl, n = [[0, 2, 4], [1]], [[-1, 0, 1], [-1]], [7, 8], 6
    if what == "node":
        walks = [[0, 6, 4], [-1]]                          # 6 >= n and -1: two invalid positions
    elif what == "read":
        n = 8
        walks = [[0, 2, 7], [1]]                           # node 7 < n names read 3 of a store of 3
    else:
        wedges = [[-1, 0, 2], [-1]]                        # edge 2 of 2: the position BEFORE it is the invalid one
    with pytest.raises(GnmError, match="out of range") as ei:
        _device(walks, wedges, pl, reads, n=n)
    rec = ei.value.record
    assert rec.invalid == (2 if what == "node" else 1) and rec.contigs == 2 and rec.pieces == 4 and rec.calls == 1
    # the pieces that ARE valid were still laid out: the count of bases leaves the invalid ones out
    want = {"node": 7 + 60, "read": 7 + 8 + 40, "edge": 7 + 60 + 40}[what]
    assert rec.bases == want


# ---- 3. codes and strands ------------------------------------------------------------------------------------------------------------------
def test_all_fifteen_codes_on_the_reverse_strand(lib):
    reads = [S.LETTERS * 3 + "ACG", S.LETTERS[::-1] * 2, S.LETTERS]
    _check([[1], [3, 5], [0, 1], [5]], [[-1], [-1, 0], [-1, 1], [-1]], [29, 48], reads, "codes")


def test_the_same_read_on_two_contigs_once_per_strand(lib, B):
    reads = _reads(12, [B + 11, 300, 45])
    _check([[2, 0, 4], [5, 1, 3]], [[-1, 0, 1], [-1, 2, 3]], [120, B + 2, 44, B + 11], reads, "both strands")


def test_a_read_past_nibble_index_two_to_the_32(lib):
    """A zero-filled store of 2.2 GB with one read at its end: base_off > 2^32, so every offset into the store needs 64 bits."""
    from gnnome_assembly_amd.reads import ReadStore
    reads = _reads(13, [5001])
    small = ReadStore.from_sequences(reads)
    nbytes = (2_200_000_000 // 16) * 16
    at = nbytes - small.packed.numel()
    assert at % 16 == 0 and 2 * at > 2 ** 32
    packed = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    packed[at:] = small.packed.to(DEV)
    store = ReadStore(packed, torch.tensor([2 * at], device=DEV), torch.tensor([5001], device=DEV))
    _check([[0], [1], [1, 0]], [[-1], [-1], [-1, 0]], [4098], reads, "past 2^32", store=store)
    del packed, store
    torch.cuda.empty_cache()


# ---- 4. against a genome, and the two routes ---------------------------------------------------------------------------------------------------
def test_a_genome_on_both_strands_through_the_list_route(lib):
    from gnnome_assembly_amd import decode
    from gnnome_assembly_amd.reads import ReadStore
    g = S.genome_case(2)
    dg = decode.DecodeGraph(g["src"], g["dst"], g["n"])
    store = ReadStore.from_sequences(g["reads"]).to(DEV)
    cs = decode.contig_sequences([g["fwd"], g["rev"]], dg, store, g["prefix_length"])
    assert cs.sequence(0) == g["want_fwd"] and cs.sequence(1) == g["want_rev"]
    assert cs.record.clamped == 0 and cs.record.invalid == 0 and cs.record.reverse == len(g["reads"])
    rl = np.repeat([len(r) for r in g["reads"]], 2)
    assert decode.contig_sequences([g["fwd"]], dg, store, g["prefix_length"], read_length=rl).sequence(0) == g["want_fwd"]
    rl[5] += 1
    with pytest.raises(ValueError, match=r"read_length\[5\]"):
        decode.contig_sequences([g["fwd"]], dg, store, g["prefix_length"], read_length=rl)
    with pytest.raises(ValueError, match="is not an edge"):
        decode.contig_sequences([[0, 4]], dg, store, g["prefix_length"])


@pytest.fixture(scope="module")
def synth_case(lib):
    from gnnome_assembly_amd import AssemblyGraph, decode, synth
    from gnnome_assembly_amd.reads import ReadStore
    src, dst, n = synth.make_graph(500, seed=4)
    rng = np.random.default_rng(4)
    reads = S.random_reads(rng, rng.integers(200, 1500, (n + 1) // 2))
    rlen = np.array([len(r) for r in reads], np.int64)
    rl = rlen[np.arange(n) >> 1]
    pl = (rng.random(src.size) * rl[src]).astype(np.int64)            # drawn below the read lengths
    g = AssemblyGraph(src, dst, n).to(DEV)
    g.edata["prefix_length"] = _t(pl, np.int64)
    scores = _t(rng.standard_normal(src.size), np.float32)
    bog = decode.best_overlap_contigs(g, scores, pl, rl)
    store = ReadStore.from_sequences(reads).to(DEV)
    return g, bog, store, reads, pl


def test_best_overlap_contigs_both_routes(synth_case):
    from gnnome_assembly_amd import decode
    g, bog, store, reads, pl = synth_case
    a = decode.contig_sequences(bog, g, store)                        # the device CSR as it is; prefix_length from g.edata
    b = decode.contig_sequences(bog.walks(), g, store)                # node lists: edge ids looked up on the host
    torch.cuda.synchronize()
    assert a.record.words() == b.record.words() and torch.equal(a.bases, b.bases) and torch.equal(a.contig_ptr, b.contig_ptr)
    assert a.record.clamped == 0 and a.record.invalid == 0 and len(a) == len(bog) and a.record.reverse > 0
    assert a.lengths.tolist() == bog.host()["bases"].tolist()
    h = bog.host()
    walks = bog.walks()
    wedges = [h["walk_edges"][h["contig_ptr"][c]:h["contig_ptr"][c + 1]].tolist() for c in range(len(walks))]
    want, rec = S.contig_strings(walks, wedges, pl, reads)
    assert a.bases.cpu().numpy().tobytes().decode() == "".join(want) and a.record.words() == [rec[k] for k in S.COUNTERS]
    print("best-overlap contigs", len(a), "bases", a.record.bases, "longest", int(a.lengths.max()), "multi-node", bog.stats.multi_contigs)
    assert bog.stats.multi_contigs > 0


def test_two_runs_give_the_same_bytes_and_record(synth_case):
    from gnnome_assembly_amd import decode
    g, bog, store, _, _ = synth_case
    a, b = decode.contig_sequences(bog, g, store), decode.contig_sequences(bog, g, store)
    assert a.record.words() == b.record.words() and torch.equal(a.bases, b.bases) and torch.equal(a.contig_ptr, b.contig_ptr)
    assert torch.equal(a.piece_off, b.piece_off) and a.record.calls == 1


def test_write_fasta_from_the_device(synth_case, tmp_path):
    from gnnome_assembly_amd import decode
    g, bog, store, _, _ = synth_case
    cs = decode.contig_sequences(bog, g, store)
    cs.write_fasta(tmp_path / "asm.fasta")
    lines = (tmp_path / "asm.fasta").read_text().split("\n")
    assert lines[0] == f">contig_1 length={cs.lengths[0]}" and max(map(len, lines)) <= 60
    body = "".join(x for x in lines if not x.startswith(">"))
    assert body == cs.bases.cpu().numpy().tobytes().decode() and sum(x.startswith(">") for x in lines) == len(cs)


# ---- 5. the pipeline ----------------------------------------------------------------------------------------------------------------------------
def test_infer_contigs_appends_the_sequences_only_when_given_reads(lib):
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
    reads = S.random_reads(rng, rng.integers(100, 400, (n + 1) // 2))
    rl = np.array([len(r) for r in reads], np.int64)[np.arange(n) >> 1]
    pl = (rng.random(src.size) * rl[src]).astype(np.int64)
    store = ReadStore.from_sequences(reads).to(DEV)
    plain = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap")
    assert len(plain) == 2
    scores, walks, seqs = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap", reads=store)
    assert torch.equal(scores, plain[0]) and walks == plain[1] and isinstance(seqs, decode.ContigSequences) and len(walks) > 0
    dg = decode.DecodeGraph(src, dst, n)
    want, rec = S.contig_strings(walks, [w.tolist() for w in np.split(decode.walk_edge_ids(dg, walks)[2], np.cumsum([len(w) for w in walks])[:-1])],
                                 pl, reads)
    assert [seqs.sequence(c) for c in range(len(walks))] == want and seqs.record.words() == [rec[k] for k in S.COUNTERS]
    four = decode.infer_contigs(model, g, e, pe, pl, rl, len_threshold=3, decoder="best_overlap", decision_report=True, reads=store)
    assert len(four) == 4 and torch.equal(four[3].bases, seqs.bases)
    torch.manual_seed(seed)
    greedy = decode.infer_contigs(model, g, e, pe, pl, rl, nb_paths=10, len_threshold=5, reads=store)
    assert len(greedy) == 3 and len(greedy[2]) == len(greedy[1])
