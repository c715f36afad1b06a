"""CPU: the packed read store (gnnome_assembly_amd/reads.py), the string yardstick of the contig sequences (tests/seq_reference.py)
against a genome it was cut from, the host lookup of walk edges, the FASTA writer, N50 / NG50 and the bindings of the new entry
points.  Strings and integers throughout, compared for equality."""
import gzip
import os

import numpy as np
import pytest
import torch

import seq_reference as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _store(seqs):
    from gnnome_assembly_amd.reads import ReadStore
    return ReadStore.from_sequences(seqs)


# ---- 1. the store ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, 31, 32, 33, 64, 1001])
def test_pack_and_sequence_round_trip_on_both_strands(n):
    rng = np.random.default_rng(n)
    seqs = S.random_reads(rng, [n, 7, n, 0, 40], p_plain=0.6)
    st = _store(seqs).validate()
    for r, s in enumerate(seqs):
        assert st.sequence(2 * r) == s and st.sequence(2 * r + 1) == S.revcomp(s), r
    assert st.length.tolist() == [len(s) for s in seqs]


def test_every_iupac_letter_lower_case_and_u():
    st = _store([S.LETTERS, S.LETTERS.lower(), "ACGU", b"acgun"])
    assert st.sequence(0) == S.LETTERS and st.sequence(2) == S.LETTERS
    assert st.sequence(1) == S.revcomp(S.LETTERS)
    assert st.sequence(4) == "ACGT" and st.sequence(5) == "ACGT" and st.sequence(6) == "ACGTN"
    codes = st.codes(0).tolist()                                      # A=1 C=2 G=4 T=8, the rest the OR of their bases, N=15
    assert codes[:4] == [1, 2, 4, 8] and codes[-1] == 15
    assert codes[S.LETTERS.index("M")] == 1 | 2 and codes[S.LETTERS.index("B")] == 2 | 4 | 8 and codes[S.LETTERS.index("W")] == 1 | 8


@pytest.mark.parametrize("bad", ["-", "=", "7", "\n", "*", " "])
def test_a_character_that_is_no_base_is_refused_by_read_and_position(bad):
    with pytest.raises(ValueError, match=r"read 1.*position 3"):
        _store(["ACGT", "ACG" + bad + "T"])


def test_bit_reversal_is_the_complement_and_an_involution():
    from gnnome_assembly_amd.reads import LETTERS, complement_code
    assert LETTERS == "=ACMGRSVTWYHKDBN"
    for c in range(1, 16):
        assert LETTERS[int(complement_code(c))] == S.PAIRS[LETTERS[c]], c
        assert int(complement_code(complement_code(c))) == c
    assert complement_code(np.arange(16)).tolist() == [int(f"{c:04b}"[::-1], 2) for c in range(16)]


def test_alignment_padding_and_save_load(tmp_path):
    from gnnome_assembly_amd.reads import ReadStore
    rng = np.random.default_rng(3)
    seqs = S.random_reads(rng, [5, 0, 33, 64, 1, 100])
    st = _store(seqs).validate()
    off, n, packed = st.base_off.numpy(), st.length.numpy(), st.packed.numpy()
    assert (off % 32 == 0).all() and off.tolist() == [0, 32, 32, 96, 160, 192] and packed.size % 16 == 0 and packed.size == (192 + 128) // 2
    nib = np.empty(2 * packed.size, np.uint8)
    nib[0::2], nib[1::2] = packed & 15, packed >> 4
    used = np.zeros(nib.size, bool)
    for o, k in zip(off, n):
        used[o:o + k] = True
    assert (nib[~used] == 0).all() and (nib[used] != 0).all()
    assert nib[:5].tolist() == [" ACMGRSVTWYHKDBN".index(c) for c in seqs[0]]             # low nibble first
    st.save(tmp_path / "reads.npz")
    back = ReadStore.load(tmp_path / "reads.npz")
    for a, b in ((st.packed, back.packed), (st.base_off, back.base_off), (st.length, back.length)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert back.names is None
    with pytest.raises(ValueError, match="read 2"):
        ReadStore(st.packed, st.base_off, [5, 0, 10 ** 6, 64, 1, 100]).validate()


def test_fasta_and_fastq_plain_and_gz(tmp_path):
    from gnnome_assembly_amd.reads import ReadStore
    fa = ">r0 first\nACGT\nNNAC\n\n>r1\nacgu\n>r2 empty\n>r3\nT\n"
    fq = "@q0 x\nACGT\nGG\n+\nII@I\n>I\n@q1\nTTA\n+q1\n@@@\n"
    (tmp_path / "a.fa").write_text(fa)
    with gzip.open(tmp_path / "a.fa.gz", "wt") as fh:
        fh.write(fa)
    (tmp_path / "b.fq").write_text(fq)
    with gzip.open(tmp_path / "b.fastq.gz", "wt") as fh:
        fh.write(fq)
    for name in ("a.fa", "a.fa.gz"):
        st = ReadStore.from_fasta(tmp_path / name)
        assert [st.sequence(2 * r) for r in range(len(st))] == ["ACGTNNAC", "ACGT", "", "T"] and st.names == ["r0 first", "r1", "r2 empty", "r3"]
    for name in ("b.fq", "b.fastq.gz"):
        st = ReadStore.from_fasta(tmp_path / name)
        assert [st.sequence(2 * r) for r in range(len(st))] == ["ACGTGG", "TTA"] and st.names == ["q0 x", "q1"]
    (tmp_path / "bad.fa").write_text(">ok\nACGT\n>broken one\nAC-GT\n")
    with pytest.raises(ValueError, match=r"broken one.*position 2"):
        ReadStore.from_fasta(tmp_path / "bad.fa")


# ---- 2. the yardstick against a genome ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_the_restatement_spells_the_genome_on_both_strands(seed):
    g = S.genome_case(seed)
    assert 150 <= len(g["reads"]) <= 200 and 40_000 <= len(g["want_fwd"]) <= 50_000
    assert any(c not in "ACGT" for c in g["genome"])
    got, rec = S.contig_strings([g["fwd"], g["rev"]], [g["fwd_edges"], g["rev_edges"]], g["prefix_length"], g["reads"])
    assert got[0] == g["want_fwd"] and got[1] == g["want_rev"]
    assert rec["clamped"] == 0 and rec["reverse"] == len(g["reads"]) and rec["bases"] == 2 * len(g["want_fwd"])
    for k, (u, v) in enumerate(zip(g["src"], g["dst"])):             # the edge tables name the steps of the two walks
        assert (u & 1) == (v & 1) and (v == u + 2 if not u & 1 else v == u - 2), k


def test_the_restatement_clamps_and_counts():
    got, rec = S.contig_strings([[0, 2, 1]], [[-1, 0, 1]], [-3, 99], ["ACGT", "GGA"])
    assert got == ["" + "GGA" + "ACGT"] and rec["clamped"] == 2 and rec["empty"] == 1 and rec["reverse"] == 1


# ---- 3. walk edges ---------------------------------------------------------------------------------------------------------------------
def test_walk_edges_against_a_dict(lib):
    from gnnome_assembly_amd import decode
    rng = np.random.default_rng(5)
    n, E = 60, 400
    src, dst = rng.integers(0, n, E).astype(np.int32), rng.integers(0, n, E).astype(np.int32)
    first = {}
    for k in range(E - 1, -1, -1):
        first[(int(src[k]), int(dst[k]))] = k                         # the lowest id of a parallel pair wins
    assert len(first) < E                                            # there ARE parallel edges in this graph
    dg = decode.DecodeGraph(src, dst, n)
    walks = []
    for _ in range(20):
        w = [int(rng.integers(0, n))]
        for _ in range(int(rng.integers(0, 12))):
            nxt = dg.successors(w[-1])
            if not nxt:
                break
            w.append(int(rng.choice(nxt)))
        walks.append(w)
    walks.append([])
    ptr, nodes, edges = decode.walk_edge_ids(dg, walks)
    assert ptr.dtype == nodes.dtype == edges.dtype == np.int32 and ptr.tolist() == np.cumsum([0] + [len(w) for w in walks]).tolist()
    assert nodes.tolist() == [v for w in walks for v in w]
    want =[e for w in walks if w for e in [-1] + [first[(a, b)] for a, b in zip(w[:-1], w[1:])]]
    assert edges.tolist() == want


def test_walk_edges_parallel_edges_and_non_edges(lib):
    from gnnome_assembly_amd import decode
    dg = decode.DecodeGraph([0, 1, 0, 0], [1, 2, 1, 1], 4)
    assert decode.walk_edge_ids(dg, [[0, 1, 2], [3]])[2].tolist() == [-1, 0, 1, -1]
    with pytest.raises(ValueError, match=r"contig 1 step 2: 1 -> 3 is not an edge"):
        decode.walk_edge_ids(dg, [[0, 1], [0, 1, 3]])
    with pytest.raises(ValueError, match="node 4 outside"):
        decode.walk_edge_ids(dg, [[0, 4]])
    assert [a.size for a in decode.walk_edge_ids(dg, [])] == [1, 0, 0]


# ---- 4. FASTA, N50, NG50 ---------------------------------------------------------------------------------------------------------------
def test_write_fasta_from_host_arrays(tmp_path):
    from gnnome_assembly_amd import decode
    lens = [0, 59, 60, 61, 120]
    seqs = ["".join("ACGT"[(i + j) % 4] for j in range(n)) for i, n in enumerate(lens)]
    cs = decode.ContigSequences(np.frombuffer("".join(seqs).encode(), np.uint8).copy(), np.cumsum([0] + lens))
    assert cs.lengths.tolist() == lens and [cs.sequence(c) for c in range(5)] == seqs and len(cs) == 5
    cs.write_fasta(tmp_path / "asm.fasta")
    want = (">contig_1 length=0\n"
            ">contig_2 length=59\n" + seqs[1] + "\n"
            ">contig_3 length=60\n" + seqs[2] + "\n"
            ">contig_4 length=61\n" + seqs[3][:60] + "\n" + seqs[3][60:] + "\n"
            ">contig_5 length=120\n" + seqs[4][:60] + "\n" + seqs[4][60:] + "\n")
    assert (tmp_path / "asm.fasta").read_text() == want
    cs.write_fasta(tmp_path / "w7.fasta", line_width=7)
    assert (tmp_path / "w7.fasta").read_text().splitlines()[2:4] == [seqs[1][:7], seqs[1][7:14]]


def test_ng50_and_quick_evaluation_by_hand():
    from gnnome_assembly_amd import decode
    lens = [10, 50, 20, 30]                       # sorted 50 30 20 10, total 110
    assert decode.ng50(lens, 100) == 50           # 50 >= 50
    assert decode.ng50(lens, 101) == 30           # 50 < 50.5 <= 80
    assert decode.ng50(lens, 200) == 20           # 100 >= 100 at the third
    assert decode.ng50(lens, 221) == -1           # total 110 < 110.5: below half of the reference
    assert decode.ng50(lens, 0) == -1 and decode.ng50([], 10) == -1
    assert decode.quick_evaluation(lens, 200) == (4, 50, 110 / 200, 30, 20)      # N50: 50 < 55 <= 80
    assert decode.quick_evaluation(lens, 1000) == (4, 50, 0.11, 30, -1)
    assert decode.quick_evaluation([7], "chr21") == (1, 7, 7 / 45090682, 7, -1)
    assert decode.quick_evaluation([], 10) == (0, 0, 0.0, -1, -1)
    assert len(decode.CHR_LENGTHS) == 23 and decode.CHR_LENGTHS["chr1"] == 248387328 and decode.CHR_LENGTHS["chrX"] == 154259566
    assert decode.ng50([decode.CHR_LENGTHS["chr19"]], "chr19") == 61707364


# ---- 5. the bindings ---------------------------------------------------------------------------------------------------------------------
def test_sources_symbols_and_abi(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib, decode, engine
    assert "gnm_seq.hip" in ge.SOURCES
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    for name in ("gnm_seq_layout", "gnm_seq_emit", "gnm_seq_workspace_bytes", "gnm_decode_walk_edges"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.gnm_abi_version() == _lib.ABI_VERSION == 7
    assert f"#define GNM_SEQ_CHUNK_BASES {engine.SEQ_CHUNK_BASES}\n" in hdr and engine.SEQ_CHUNK_BASES % 16 == 0
    assert engine.SEQ_COUNTERS == S.COUNTERS and engine.SEQ_RECORD_WORDS == 8
    assert tuple(decode.SeqStats.__dataclass_fields__) == engine.SEQ_COUNTERS and decode.SeqStats(*range(8)).words() == list(range(8))
    assert lib.gnm_seq_workspace_bytes(0) == 0 and lib.gnm_seq_workspace_bytes(257) == 16 and lib.gnm_seq_workspace_bytes(-1) == 0


def test_host_side_refusals(lib):
    import ctypes as C
    rec = (C.c_int64 * 8)()
    one = (C.c_int64 * 4)()
    # a store that is not whole 16-byte groups, a missing record, an output too small for the bases: refused before any launch
    assert lib.gnm_seq_layout(0, 0, 0, 0, 0, one, None, None, None, None, None, 24, rec, None, one, one, None, 0, None) < 0
    assert b"16-byte" in lib.gnm_last_error()
    assert lib.gnm_seq_layout(0, 0, 0, 0, 0, one, None, None, None, None, None, 32, None, None, one, one, None, 0, None) < 0
    assert lib.gnm_seq_emit(1, 2, 1, one, one, one, one, one, 32, 40, one, 32, None) < 0
    assert lib.gnm_seq_emit(-1, 2, 1, one, one, one, one, one, 32, 0, one, 32, None) < 0
    assert lib.gnm_seq_emit(0, 0, 0, None, None, None, None, None, 0, 0, None, 0, None) == 0       # nothing to do, nothing launched


def test_contig_sequences_needs_a_device_store(lib):
    from gnnome_assembly_amd import _lib, decode
    dg = decode.DecodeGraph([0], [2], 4)
    with pytest.raises(_lib.GnmError, match="HIP device"):
        decode.contig_sequences([[0, 2]], dg, _store(["ACGT", "GTAA"]), prefix_length=[2])
    with pytest.raises(TypeError):
        decode.contig_sequences([[0, 2]], dg, ["ACGT", "GTAA"], prefix_length=[2])
