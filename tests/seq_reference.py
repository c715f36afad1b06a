"""The yardstick of the contig-sequence tests: evaluate.walk_to_sequence (evaluate.py:36-47) restated over plain Python strings --
`str` slices, a `str` reverse complement over the IUPAC pairs -- with the one documented difference: a prefix below 0 or above
the read's length is clamped (include/gnm.h, "contig sequences").  Nothing here touches the packed store or the library.

genome_case(seed) needs no restatement at all: reads cut from a random genome, edges between consecutive reads with
prefix_length = the difference of their starts; the walk along the + nodes must spell the genome between the first start and the
last end, the mirrored walk along the - nodes its reverse complement."""
import numpy as np

COUNTERS = ("contigs", "pieces", "bases", "clamped", "empty", "reverse", "invalid", "calls")
PAIRS = {"A": "T", "C": "G", "G": "C", "T": "A", "M": "K", "K": "M", "R": "Y", "Y": "R", "S": "S", "W": "W", "V": "B", "B": "V",
         "H": "D", "D": "H", "N": "N"}
LETTERS = "ACGTMRSVWYHKDBN"


def revcomp(s: str) -> str:
    return "".join(PAIRS[c] for c in reversed(s))


def node_sequence(reads, v: int) -> str:
    """reads[v] of the reference: node v is read v >> 1, reverse-complemented when v is odd."""
    s = reads[v >> 1].upper().replace("U", "T")
    return revcomp(s) if v & 1 else s


def contig_strings(walks, walk_edges, prefix_length, reads):
    """walks: lists of node ids; walk_edges: per walk, the edge id INTO every position (-1 or anything at the first one).
    Returns (list of str, record dict)."""
    rec = dict.fromkeys(COUNTERS, 0)
    rec["calls"] = 1
    out = []
    for walk, edges in zip(walks, walk_edges):
        parts = []
        for i, v in enumerate(walk):
            s = node_sequence(reads, int(v))
            if i + 1 < len(walk):
                k = int(prefix_length[int(edges[i + 1])])
                if k < 0 or k > len(s):
                    rec["clamped"] += 1
                    k = min(max(k, 0), len(s))
                s = s[:k]
            parts.append(s)
            rec["pieces"] += 1
            rec["empty"] += len(s) == 0
            rec["reverse"] += int(v) & 1
        out.append("".join(parts))
        rec["contigs"] += 1
        rec["bases"] += len(out[-1])
    return out, rec


def random_reads(rng, lengths, letters=LETTERS, p_plain=0.97):
    """Strings of the given lengths: mostly A C G T, a few ambiguity letters and N."""
    alpha = np.array(list(letters))
    p = np.full(alpha.size, (1 - p_plain) / max(1, alpha.size - 4))
    p[:4] = p_plain / 4
    return ["".join(rng.choice(alpha, int(n), p=p / p.sum())) for n in lengths]


def genome_case(seed: int, genome_len: int = 50_000, n_reads: int = 200, lo: int = 500, hi: int = 3000):
    """dict: genome (str), reads (list of str, read i = node 2i), starts, ends, src, dst, prefix_length (edge arrays: edge i joins
    nodes 2i -> 2i+2, edge R-1+i joins (2i+3) -> (2i+1)), n (nodes), fwd / rev (the two walks as node lists), fwd_edges /
    rev_edges (the edge id into every position, -1 first), want_fwd / want_rev (what the walks must spell)."""
    rng = np.random.default_rng(seed)
    genome = random_reads(rng, [genome_len])[0]
    lens = rng.integers(lo, hi + 1, n_reads)
    # ascending starts, consecutive reads overlap, every read ends after the one before it (so the mirrored prefixes are > 0)
    starts, ends = [0], [int(lens[0])]
    for i in range(1, n_reads):
        s = int(rng.integers(starts[-1] + 1, min(ends[-1], starts[-1] + 480)))     # ~240 bases on: ~200 reads over ~50 kb
        e = max(s + int(lens[i]), ends[-1] + 1)
        if e > genome_len:
            break
        starts.append(s)
        ends.append(e)
    R = len(starts)
    reads = [genome[s:e] for s, e in zip(starts, ends)]
    src = [2 * i for i in range(R - 1)] + [2 * i + 3 for i in range(R - 1)]
    dst = [2 * i + 2 for i in range(R - 1)] + [2 * i + 1 for i in range(R - 1)]
    pl = [starts[i + 1] - starts[i] for i in range(R - 1)] + [ends[i + 1] - ends[i] for i in range(R - 1)]
    fwd = [2 * i for i in range(R)]
    rev = [2 * i + 1 for i in range(R - 1, -1, -1)]
    fwd_edges = [-1] + list(range(R - 1))
    rev_edges = [-1] + [R - 1 + i for i in range(R - 2, -1, -1)]       # into node 2i+1 comes the edge (2i+3) -> (2i+1)
    want = genome[starts[0]:ends[-1]]
    return dict(genome=genome, reads=reads, starts=starts, ends=ends, src=np.array(src, np.int32), dst=np.array(dst, np.int32),
                prefix_length=np.array(pl, np.int64), n=2 * R, fwd=fwd, rev=rev, fwd_edges=fwd_edges, rev_edges=rev_edges,
                want_fwd=want, want_rev=revcomp(want))
