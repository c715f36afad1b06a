"""The yardstick of the overlap-graph tests (include/gnm.h, "overlap graph"): the three stages and the assembly restated in plain
Python / numpy over strings -- k-mers as Python integers, every window's minimum by brute force, runs and groups by explicit loops,
the verification by align_reference's dynamic programme -- and the case builders.  Nothing here touches the packed store or the
library; nothing was taken from csrc/gnm_overlap.h."""
import numpy as np

from align_reference import mutate, prefix_distance, random_sequence
from seq_reference import node_sequence, revcomp

COUNTERS = ("reads", "kmers_valid", "minimizers", "runs", "skipped_runs", "skipped_entries", "hits", "same_read", "groups",
            "few_hits", "short", "contained_groups", "links", "calls")
TILE = 512
M64 = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def fmix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def kmer_value(s):
    v = 0
    for ch in s:
        v = v * 4 + CODE[ch]
    return v


def kmers(seq, k):
    """Per position of the + strand: (valid, hash, strand)."""
    out = []
    for p in range(len(seq) - k + 1):
        s = seq[p:p + k].upper().replace("U", "T")
        if any(ch not in CODE for ch in s):
            out.append((False, 0, 0))
            continue
        f, r = kmer_value(s), kmer_value(revcomp(s))
        out.append((f != r, fmix64(min(f, r)), int(r < f)))
    return out


def new_record():
    return dict.fromkeys(COUNTERS, 0)


def rec_array(rec):
    return np.array([rec[c] for c in COUNTERS], np.int64)


def sketch(seqs, k, w, rec=None):
    """(hash int64, read int32, pos int32, strand uint8) ordered by read and position; every window's smallest (h, p)."""
    rec = new_record() if rec is None else rec
    hs, rs, ps, ss = [], [], [], []
    for r, seq in enumerate(seqs):
        km = kmers(seq, k)
        nk = len(km)
        rec["kmers_valid"] += sum(1 for v, _, _ in km if v)
        if nk <= 0:
            continue
        W = min(w, nk)
        chosen = set()
        for j in range(nk - W + 1):
            cand = [(km[p][1], p) for p in range(j, j + W) if km[p][0]]
            if cand:
                chosen.add(min(cand)[1])
        for p in sorted(chosen):
            hs.append(km[p][1])
            rs.append(r)
            ps.append(p)
            ss.append(km[p][2])
    rec["reads"] += len(seqs)
    rec["minimizers"] += len(hs)
    rec["calls"] += 1
    return (np.array(hs, np.uint64).view(np.int64), np.array(rs, np.int32), np.array(ps, np.int32), np.array(ss, np.uint8)), rec


def sort_by_hash(sk):
    o = np.argsort(sk[0], kind="stable")                   # as signed int64
    return tuple(a[o] for a in sk)


def seed_pairs(sk_sorted, lengths, k, max_occ, rec=None):
    """(key int64, diag int32) of the entries sorted by hash: by the later entry, then the earlier ascending."""
    rec = new_record() if rec is None else rec
    h, rd, ps, st = sk_sorted
    keys, diags = [], []
    M = len(h)
    i = 0
    while i < M:
        e = i
        while e < M and h[e] == h[i]:
            e += 1
        rec["runs"] += 1
        if e - i > max_occ:
            rec["skipped_runs"] += 1
            rec["skipped_entries"] += e - i
        else:
            for x in range(i, e):
                for y in range(i, x):
                    if rd[x] == rd[y]:
                        rec["same_read"] += 1
                        continue
                    ea, eb = (y, x) if rd[y] < rd[x] else (x, y)
                    a, b = int(rd[ea]), int(rd[eb])
                    rel = int(st[ea]) ^ int(st[eb])
                    q = int(ps[eb]) if rel == 0 else int(lengths[b]) - k - int(ps[eb])
                    keys.append((a << 32) | (b << 1) | rel)
                    diags.append(int(ps[ea]) - q)
        i = e
    rec["hits"] += len(keys)
    return (np.array(keys, np.int64), np.array(diags, np.int32)), rec


def sort_hits(hits):
    key, diag = hits
    o = np.argsort(diag, kind="stable")
    key, diag = key[o], diag[o]
    o = np.argsort(key, kind="stable")
    return key[o], diag[o]


def chain_pairs(hits_sorted, lengths, band, min_hits, min_overlap, rec=None):
    """(src, dst, prefix_length, overlap_length, valid) [2 G] and contained [R]."""
    rec = new_record() if rec is None else rec
    key, diag = hits_sorted
    R = len(lengths)
    src, dst, pre, ovl, val = [], [], [], [], []
    contained = np.zeros(R, np.uint8)
    i = 0
    while i < len(key):
        e = i
        while e < len(key) and key[e] == key[i]:
            e += 1
        d = [int(x) for x in diag[i:e]]
        kk = int(key[i])
        a, b, rel = kk >> 32, (kk & 0xffffffff) >> 1, kk & 1
        rec["groups"] += 1
        counts = [sum(1 for j in range(x, len(d)) if d[j] <= d[x] + band) for x in range(len(d))]
        best = max(counts)
        x = counts.index(best)
        D = d[x + (best - 1) // 2]
        la, lb = int(lengths[a]), int(lengths[b])
        edge = None
        if best < min_hits:
            rec["few_hits"] += 1
        elif D > 0 and D + lb > la:
            ov = la - D
            edge = ((2 * a, 2 * b + rel, D), ((2 * b + rel) ^ 1, 2 * a + 1, lb - ov), ov)
        elif D < 0 and D + lb < la:
            ov = lb + D
            edge = ((2 * b + rel, 2 * a, -D), (2 * a + 1, (2 * b + rel) ^ 1, la - ov), ov)
        else:
            contained[b if (D >= 0 and D + lb <= la) else a] = 1
            rec["contained_groups"] += 1
        if edge is not None and edge[2] < min_overlap:
            rec["short"] += 1
            edge = None
        if edge is not None:
            rec["links"] += 1
        for t in range(2):
            s_, d_, p_ = edge[t] if edge else (-1, -1, 0)
            src.append(s_), dst.append(d_), pre.append(p_), ovl.append(edge[2] if edge else 0), val.append(1 if edge else 0)
        i = e
    return (np.array(src, np.int32), np.array(dst, np.int32), np.array(pre, np.int64), np.array(ovl, np.int64),
            np.array(val, np.uint8), contained), rec


def find_overlaps(seqs, k=21, w=25, max_occ=64, min_hits=4, band=32, min_overlap=500, max_errors=255, verify=True,
                  drop_contained=True):
    """dict: src, dst, prefix_length, overlap_length, twin (and overlap_similarity with verify) in src-major order; contained;
    record; sketch_size; hit_count."""
    lengths = np.array([len(s) for s in seqs], np.int64)
    rec = new_record()
    sk, _ = sketch(seqs, k, w, rec)
    hits, _ = seed_pairs(sort_by_hash(sk), lengths, k, max_occ, rec)
    (src, dst, pre, ovl, val, contained), _ = chain_pairs(sort_hits(hits), lengths, band, min_hits, min_overlap, rec)
    pairs = [j for j in range(0, len(src), 2) if val[j]]
    sim = {}
    if verify:
        good = []
        for j in pairs:
            ok = True
            for e in (j, j + 1):
                q = node_sequence(seqs, int(src[e]))[int(pre[e]):]
                t = node_sequence(seqs, int(dst[e]))[:len(q) + max_errors]
                d = prefix_distance(q, t)
                ok &= d <= max_errors
                sim[e] = max(np.float32(0), np.float32(1) - np.float32(min(d, max_errors + 1)) / np.float32(len(q)))
            if ok:
                good.append(j)
        pairs = good
    if drop_contained:
        pairs = [j for j in pairs if not any(contained[int(v) >> 1] for v in (src[j], dst[j], src[j + 1], dst[j + 1]))]
    edges = [e for j in pairs for e in (j, j + 1)]
    order = sorted(range(len(edges)), key=lambda x: (int(src[edges[x]]), int(dst[edges[x]]), x))
    ids = [edges[x] for x in order]
    where = {e: i for i, e in enumerate(ids)}
    out = dict(src=src[ids], dst=dst[ids], prefix_length=pre[ids], overlap_length=ovl[ids],
               twin=np.array([where[e ^ 1] for e in ids], np.int64), contained=contained.astype(bool), record=rec_array(rec),
               sketch_size=len(sk[0]), hit_count=len(hits[0]))
    if verify:
        out["overlap_similarity"] = np.array([sim[e] for e in ids], np.float32)
    return out


# ---- case builders ---------------------------------------------------------------------------------------------------------------
def sketch_cases():
    """name -> (sequences, k, w)."""
    rng = np.random.default_rng(11)
    rs = lambda n: random_sequence(rng, n)  # noqa: E731
    k, w = 15, 10
    out = {
        "short": ([rs(k - 1), rs(k), rs(k + w - 2), rs(k + w - 1), rs(k + w)], k, w),
        "all-n": (["".join("N" if i % 7 == 3 else c for i, c in enumerate(rs(200))), rs(90)], k, w),
        "one-n": ([rs(60) + "N" + rs(80), "N" + rs(50), rs(50) + "N"], k, w),
        "palindrome": ([rs(40) + "ACGTACGT" + rs(40), "ACGTACGT" * 6], 8, 4),
        "homopolymer": (["A" * 120, "T" * 75, "AC" * 60], k, w),
        "tile": ([rs(TILE + k - 1 + d) for d in (-1, 0, 1)] + [rs(2 * TILE + k - 1 + 40)], k, 25),
        "tile-w64": ([rs(TILE + 30 + 63), rs(2 * TILE + 31 + 5)], 31, 64),
        "empty": ([], k, w),
        "empty-reads": (["", rs(100), ""], k, w),
        "k8-w1": ([rs(300), rs(33)], 8, 1),
        "k31-w64": ([rs(400), rs(31 + 62), rs(31)], 31, 64),
        "k8-w64": ([rs(700)], 8, 64),
        "codes": ([rs(50) + "R" + rs(30) + "acgu" + rs(40)], 12, 6),
    }
    return out


def pair_cases():
    """name -> (sorted sketch arrays, lengths, k, max_occ): hand-made entries, so that run sizes are exact."""
    rng = np.random.default_rng(12)
    R, k, occ = 12, 15, 5
    lengths = rng.integers(200, 400, R).astype(np.int64)

    def run(h, reads):
        reads = sorted(reads)
        return [(h, r, int(rng.integers(0, 150)), int(rng.integers(2))) for r in reads]

    rows = []
    rows += run(-50, [0, 1, 2, 3, 4])                      # exactly max_occ
    rows += run(-7, [0, 1, 2, 3, 4, 5])                    # max_occ + 1: skipped
    rows += run(3, [6, 6, 6])                              # a run of one read
    rows += run(9, [7])                                    # a run of one entry
    rows += run(12, [2, 2, 9, 11])                         # same-read pairs inside a mixed run
    rows += run(2 ** 62, [1, 8])
    rows += run(-2 ** 63, [3, 10])                         # the smallest signed hash comes first
    rows.sort(key=lambda t: t[0])
    for x in range(1, len(rows)):                          # positions ascend inside (hash, read), as a sketch's do
        if rows[x][:2] == rows[x - 1][:2] and rows[x][2] <= rows[x - 1][2]:
            rows[x] = (rows[x][0], rows[x][1], rows[x - 1][2] + 1, rows[x][3])
    arr = (np.array([t[0] for t in rows], np.int64), np.array([t[1] for t in rows], np.int32),
           np.array([t[2] for t in rows], np.int32), np.array([t[3] for t in rows], np.uint8))
    none = tuple(a[:0] for a in arr)
    return {"runs": (arr, lengths, k, occ), "occ1": (arr, lengths, k, 1), "empty": (none, lengths, k, occ)}


def chain_cases():
    """name -> (sorted hits, lengths, band, min_hits, min_overlap), every branch by hand."""
    lengths = np.array([1000, 1000, 600, 1000, 1400, 1000, 1000], np.int64)
    K = lambda a, b, rel: (a << 32) | (b << 1) | rel  # noqa: E731
    groups = [
        (K(0, 1, 0), [400] * 4),                            # forward, ov = 600
        (K(0, 1, 1), [-300, -300, -299, -280]),             # backward on the other strand of the same pair (an inverted repeat)
        (K(0, 2, 0), [100, 101, 102, 103]),                 # b contained
        (K(0, 4, 0), [-200] * 5),                           # a contained
        (K(0, 3, 0), [0, 0, 0, 0]),                         # D == 0, equal lengths: the higher id is contained
        (K(1, 5, 0), [0, 0, 0, 0, 900, 901]),               # identical reads
        (K(2, 3, 0), [-400, -400, -400, -400]),             # D + lb == la: 600 = -400 + 1000: a contained
        (K(2, 4, 1), [7]),                                  # a group of one hit
        (K(3, 4, 0), [10, 20, 30, 40, 200, 210, 220, 230]),  # two windows of equal count: the lowest wins (band 32)
        (K(3, 5, 0), [500, 500, 500, 500]),                 # ov == 500 == min_overlap
        (K(3, 6, 0), [501, 501, 501, 501]),                 # ov == min_overlap - 1: short
        (K(4, 5, 1), [100, 140, 180, 220, 221, 222, 223]),  # the window is not the first
        (K(5, 6, 0), [-500, -499, -470, -469, -468]),       # backward, the median of the window
    ]
    key = np.concatenate([np.full(len(d), k_, np.int64) for k_, d in groups])
    diag = np.concatenate([np.array(d, np.int32) for _, d in groups])
    o = np.argsort(key, kind="stable")
    hits = (key[o], diag[o])
    none = (key[:0], diag[:0])
    return {"branches": (hits, lengths, 32, 4, 500), "band0": (hits, lengths, 0, 2, 500), "min-hits-1": (hits, lengths, 32, 1, 0),
            "empty": (none, lengths, 32, 4, 500)}


def genome_reads(seed=21, genome_len=6000, reads_n=60, lo=300, hi=900, rate=0.0):
    """Reads cut from one random genome on both strands: dict reads, genome, truth = [(start, end, strand)] per read (strand 1: the
    stored read is the reverse complement of genome[start:end]).  rate: per-base errors applied after the cut."""
    rng = np.random.default_rng(seed)
    genome = random_sequence(rng, genome_len)
    start = rng.integers(0, genome_len - hi, reads_n)
    end = start + rng.integers(lo, hi + 1, reads_n)
    strand = rng.integers(0, 2, reads_n)
    reads = []
    for s, e, t in zip(start, end, strand):
        r = genome[s:e]
        if rate:
            r = mutate(rng, r, rate)
        reads.append(revcomp(r) if t else r)
    return dict(reads=reads, genome=genome, truth=[(int(s), int(e), int(t)) for s, e, t in zip(start, end, strand)])


def true_overlaps(truth, min_overlap, drop_contained=True):
    """The overlap graph the read positions imply: contained [R] and the sorted list of (src, dst, prefix_length, overlap_length)."""
    R = len(truth)
    contained = np.zeros(R, bool)
    for i in range(R):
        for j in range(R):
            if i == j:
                continue
            (si, ei, _), (sj, ej, _) = truth[i], truth[j]
            if si <= sj and ej <= ei and ((si, ei) != (sj, ej) or j > i):
                contained[j] = True
    fwd = lambda i: 2 * i + truth[i][2]  # noqa: E731        the node of read i that reads along the genome
    edges = []
    for i in range(R):
        for j in range(R):
            (si, ei, _), (sj, ej, _) = truth[i], truth[j]
            if i == j or not (si < sj and ei < ej and ei - sj >= min_overlap):
                continue
            if drop_contained and (contained[i] or contained[j]):
                continue
            ov = ei - sj
            edges.append((fwd(i), fwd(j), sj - si, ov))
            edges.append((fwd(j) ^ 1, fwd(i) ^ 1, ej - ei, ov))
    return contained, sorted(edges)


_CACHE = {}


def cached(name, fn):
    if name not in _CACHE:
        _CACHE[name] = fn()
    return _CACHE[name]
