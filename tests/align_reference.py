"""The yardstick of the overlap alignment (include/gnm.h, "overlap alignment"): the rule as the plain O(m |T|) dynamic programme
over the strings ReadStore.sequence returns, with the same cut of T, the same K + 1 saturation and the same counters; and a seeded
generator of read pairs.  Nothing here touches the packed store or the library."""
import numpy as np

COUNTERS = ("edges", "aligned", "exceeded", "empty", "clamped", "invalid", "cells", "calls")
BASES = "ACGT"


def prefix_distance(q: str, t: str) -> int:
    """min over 0 <= j <= len(t) of Levenshtein(q, t[:j]): all of q, both from their first letter, the end in t free.  Letters
    match when they are equal."""
    tq = np.frombuffer(t.encode(), np.uint8)
    steps = np.arange(tq.size + 1, dtype=np.int64)
    row = steps.copy()                                      # Levenshtein("", t[:j]) = j
    for i, ch in enumerate(q.encode(), 1):
        new = np.empty_like(row)
        new[0] = i
        new[1:] = np.minimum(row[:-1] + (tq != ch), row[1:] + 1)
        row = np.minimum.accumulate(new - steps) + steps    # new[j] = min over k <= j of new[k] + (j - k): the insertions
    return int(row.min())


def overlap_align(store, n, src, dst, prefix_length, max_errors):
    """(dist int32 [E], overlap_length int64 [E], similarity fp32 [E], record int64 [8]) of the rule, one call."""
    K = int(max_errors)
    E = len(src)
    dist, olen, sim = np.zeros(E, np.int32), np.zeros(E, np.int64), np.zeros(E, np.float32)
    rec = dict.fromkeys(COUNTERS, 0)
    rec["edges"], rec["calls"] = E, 1
    R = len(store)
    for k in range(E):
        a, c, p = int(src[k]), int(dst[k]), int(prefix_length[k])
        if not (0 <= a < n and 0 <= c < n and (a >> 1) < R and (c >> 1) < R):
            dist[k] = -1
            rec["invalid"] += 1
            continue
        qa, tc = store.sequence(a), store.sequence(c)
        if p < 0 or p > len(qa):
            p = 0 if p < 0 else len(qa)
            rec["clamped"] += 1
        q = qa[p:]
        m = len(q)
        olen[k] = m
        if m == 0:
            rec["empty"] += 1
            continue
        t = tc[:min(len(tc), m + K)]
        d = prefix_distance(q, t)
        if d > K:
            d = K + 1
            rec["exceeded"] += 1
        else:
            rec["aligned"] += 1
            rec["cells"] += m * len(t)
        dist[k] = d
        sim[k] = max(np.float32(0), np.float32(1) - np.float32(d) / np.float32(m))
    return dist, olen, sim, np.array([rec[c] for c in COUNTERS], np.int64)


def random_sequence(rng, length, alphabet=BASES):
    return "".join(rng.choice(list(alphabet), size=int(length)))


def mutate(rng, s, rate, alphabet=BASES):
    """s with seeded substitutions, insertions and deletions, each at about rate / 3 per letter."""
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3:
            out.append(rng.choice([b for b in alphabet if b != ch]))        # substitution
        elif u < 2 * rate / 3:
            out.append(ch)
            out.append(rng.choice(list(alphabet)))                          # insertion
        elif u < rate:
            continue                                                        # deletion
        else:
            out.append(ch)
    return "".join(out)


def read_pair(rng, m, rate, extra=40, head=0, alphabet=BASES):
    """(source read, destination read, prefix_length): the destination starts with a region of m letters, the source ends with a
    mutated copy of it behind `head` letters of its own; `extra` more letters follow the region in the destination."""
    region = random_sequence(rng, m, alphabet)
    src = random_sequence(rng, head, alphabet) + mutate(rng, region, rate, alphabet)
    dst = region + random_sequence(rng, extra, alphabet)
    return src, dst, head


# ---- the cases both test files run: (name, sequences, n, src, dst, prefix_length, K) -------------------------------------------------
BOUNDARY_M = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
BOUNDARY_K = (0, 1, 31, 32, 63, 64, 127, 128, 255)
RANDOM_K = (3, 40, 130)


def _build(pairs):
    """pairs of (source sequence, destination sequence, prefix_length, source odd?, destination odd?) -> (sequences, n, src, dst,
    pl): two reads per pair; an odd node's read is stored reverse-complemented, so that the NODE reads as given."""
    from seq_reference import revcomp
    seqs, src, dst, pl = [], [], [], []
    for a, c, p, oa, oc in pairs:
        r = len(seqs)
        seqs += [revcomp(a) if oa else a, revcomp(c) if oc else c]
        src.append(2 * r + int(oa))
        dst.append(2 * r + 2 + int(oc))
        pl.append(p)
    return seqs, 2 * len(seqs), np.array(src, np.int32), np.array(dst, np.int32), np.array(pl, np.int64)


def _with_n(s, where):
    s = list(s)
    for i in where:
        s[i] = "N"
    return "".join(s)


def hand_cases(K):
    """Known distances for one K >= 1: (case, expected dist)."""
    rng = np.random.default_rng(100 + K)
    m = 3 * K + 40
    r, extra, h = random_sequence(rng, m), random_sequence(rng, 2 * K + 8), K + 5
    spread = [int(x) for x in np.linspace(2, m - 3, K + 1).astype(int)]
    assert len(set(spread)) == K + 1
    pairs = [(r, r + extra, 0, 0, 0),                                              # identical
             ("GG" + _with_n(r, [h]), r + extra, 2, 0, 0),                         # one substitution
             (r[:h] + "N" * K + r[h:], r + extra, 0, 0, 0),                        # K insertions in a run: the extreme diagonal
             (r, r[:h] + "N" * K + r[h:] + extra, 0, 0, 0),                        # K deletions in a run
             (_with_n(r, spread[:K]), r + extra, 0, 0, 0),                         # exactly K
             (_with_n(r, spread), r + extra, 0, 0, 0)]                             # exactly K + 1: exceeded
    return ("hand", *_build(pairs), K), [0, 1, K, K, K, K + 1]


def boundary_case(K):
    rng = np.random.default_rng(200 + K)
    pairs = []
    for m in BOUNDARY_M:
        for rate in (0.0, 0.06):
            a, c, p = read_pair(rng, m, rate, extra=int(rng.integers(0, 2 * K + 20)), head=int(rng.integers(0, 9)))
            pairs.append((a, c, p, int(rng.integers(2)), int(rng.integers(2))))
    return ("boundary", *_build(pairs), K)


def target_length_case(K):
    rng = np.random.default_rng(300 + K)
    m = 2 * K + 70
    pairs = []
    for cut in (1, K, K + 1, K + 30, m):                                           # lc = m - cut: forced deletions ... lc == 0
        a, c, p = read_pair(rng, m, 0.0, extra=0, head=3)                          # an exact copy: the distance is the cut
        pairs.append((a, c[:max(0, m - cut)], p, int(rng.integers(2)), int(rng.integers(2))))
    return ("target_length", *_build(pairs), K)


def strand_case(K):
    rng = np.random.default_rng(400 + K)
    pairs = []
    for oa, oc in ((0, 0), (1, 1), (0, 1), (1, 0)):
        for head in (0, 1, 2, 7, 8, 15, 16, 17):                                   # the query starts on either nibble
            a, c, p = read_pair(rng, int(rng.integers(20, 150)), 0.04, extra=int(rng.integers(0, 50)), head=head)
            pairs.append((a, c, p, oa, oc))
    for oa, oc in ((0, 1), (1, 0)):                                                # whole 16-byte groups: the LAST read ends the store
        g = random_sequence(rng, 96)
        pairs.append((random_sequence(rng, 32) + mutate(rng, g, 0.03), g, 32, oa, oc))
    seqs, n, src, dst, pl = _build(pairs)
    seqs[-1] = seqs[-1][:64]                                                       # 64 bases: no pad nibbles behind the last read
    assert len(seqs[-1]) == 64
    src, dst, pl = np.append(src, dst[-1]), np.append(dst, src[-1]), np.append(pl, 5)   # and the last read as the QUERY
    return ("strands", seqs, n, src.astype(np.int32), dst.astype(np.int32), pl.astype(np.int64), K)


def code_case(K):
    body = "ACGTACGGTCA"
    pairs = [(body + "N" + body, body + "N" + body + "TT", 0, 0, 0),               # N against N matches
             (body + "N" + body, body + "A" + body + "TT", 0, 0, 0),               # N against A does not
             (body + "R" + body, body + "R" + body + "TT", 0, 1, 1),               # an ambiguity code matches itself only,
             (body + "R" + body, body + "A" + body + "TT", 0, 0, 1),               # not one of its bases
             (body + "Y" + body, body + "R" + body, 0, 1, 0)]
    return ("codes", *_build(pairs), K), [0, 1, 0, 1, 1]


def bad_case(K):
    rng = np.random.default_rng(500 + K)
    a, c, _ = read_pair(rng, 40, 0.0, extra=10, head=6)
    seqs = [a, c]
    src = np.array([0, 0, 0, 0, 6, 0, 4, -1, 1], np.int32)                         # n = 6, R = 2: node 4 is a read the store lacks
    dst = np.array([2, 2, 2, 2, 2, 7, 2, 2, 5], np.int32)
    pl = np.array([6, -1, len(a) + 1, len(a), 0, 0, 0, 0, 0], np.int64)
    return ("bad", seqs, 6, src, dst, pl, K)


def random_case(K, pairs_n=200):
    rng = np.random.default_rng(7)                                                 # the same pairs under every K
    pairs = []
    for i in range(pairs_n):
        m = int(rng.integers(1, 301)) if i % 10 != 9 else int(rng.integers(285, 301))
        a, c, p = read_pair(rng, m, float(rng.uniform(0, 0.10)), extra=int(rng.integers(0, 200)), head=int(rng.integers(0, 40)))
        a = a[:p + 300]                                                            # m <= 300 also after insertions
        if i % 10 == 9:
            c = random_sequence(rng, len(c))                                       # no overlap at all
        pairs.append((a, c, p, int(rng.integers(2)), int(rng.integers(2))))
    return ("random", *_build(pairs), K)


_CACHE = {}


def reference(case):
    """overlap_align of a case over a host store, computed once per (name, K)."""
    from gnnome_assembly_amd.reads import ReadStore
    name, seqs, n, src, dst, pl, K = case
    if (name, K) not in _CACHE:
        store = ReadStore.from_sequences(seqs)
        _CACHE[(name, K)] = (store, overlap_align(store, n, src, dst, pl, K))
    return _CACHE[(name, K)]


def all_cases():
    """Every case of the two test files, by a readable id."""
    out = {}
    for K in (1, 3, 40):
        out[f"hand-K{K}"] = hand_cases(K)[0]
    for K in BOUNDARY_K:
        out[f"boundary-K{K}"] = boundary_case(K)
    for K in (2, 40):
        out[f"target_length-K{K}"] = target_length_case(K)
    for K in (4, 100):
        out[f"strands-K{K}"] = strand_case(K)
    out["codes-K2"] = code_case(2)[0]
    for K in (0, 10):
        out[f"bad-K{K}"] = bad_case(K)
    for K in RANDOM_K:
        out[f"random-K{K}"] = random_case(K)
    return out


def genome_graph(seed=3, genome_len=20000, reads_n=240, lo=200, hi=600, max_out=4, rate=0.0):
    """A small overlap graph cut from one random genome: read i covers [s_i, e_i), starts ascending; node 2i is read i, node 2i + 1
    its reverse complement.  Edge 2i -> 2j (and its mirror 2j+1 -> 2i+1) for the up to max_out next reads j that start inside read
    i and end behind it, with prefix_length s_j - s_i (mirror: e_j - e_i).  `rate`: seeded per-base errors applied to the reads
    AFTER the cut (0: every overlap is exact).  dict: reads, n, src, dst, prefix_length."""
    rng = np.random.default_rng(seed)
    genome = random_sequence(rng, genome_len)
    start = np.sort(rng.integers(0, genome_len - hi, reads_n))
    end = start + rng.integers(lo, hi + 1, reads_n)
    reads = [genome[s:e] for s, e in zip(start, end)]
    if rate:
        reads = [mutate(rng, r, rate) for r in reads]
    src, dst, pl = [], [], []
    for i in range(reads_n):
        out = 0
        for j in range(i + 1, reads_n):
            if start[j] >= end[i] or out == max_out:
                break
            if end[j] <= end[i] or start[j] == start[i]:
                continue
            src += [2 * i, 2 * j + 1]
            dst += [2 * j, 2 * i + 1]
            pl += [int(start[j] - start[i]), int(end[j] - end[i])]
            out += 1
    return dict(reads=reads, n=2 * reads_n, src=np.array(src, np.int32), dst=np.array(dst, np.int32),
                prefix_length=np.array(pl, np.int64))
