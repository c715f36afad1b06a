"""The yardstick of the chunked overlap route (include/gnm.h, "Stage 2 in read-range chunks"), on top of overlap_reference's
seed_pairs: a hit's lower read id is key >> 32; lower_hits counts the hits per lower read, a range keeps the hits whose lower read
lies in it, in the order they have.  plan: the greedy chunks, read by read."""
import numpy as np

import overlap_reference as O


def lower_of(key):
    return np.asarray(key, np.int64) >> 32


def lower_hits(sk_sorted, lengths, k, max_occ):
    """(lower_hits int64 [R], record): how many hits name each read as their lower one."""
    (key, _), rec = O.seed_pairs(sk_sorted, lengths, k, max_occ)
    return np.bincount(lower_of(key), minlength=len(lengths)).astype(np.int64), rec


def range_hits(hits, a_lo, a_hi):
    """(key, diag) of the hits with a_lo <= lower read < a_hi."""
    key, diag = hits
    m = (lower_of(key) >= a_lo) & (lower_of(key) < a_hi)
    return key[m], diag[m]


def plan(counts, max_hits):
    """(bounds, chunk_hits, oversize): reads are added to the chunk in progress while its sum stays <= max_hits; a read that alone
    exceeds max_hits closes the chunk in progress and is a chunk of its own."""
    bounds, sums, cur = [0], [], 0
    for r, c in enumerate(counts):
        c = int(c)
        if c > max_hits:
            if bounds[-1] < r:
                bounds.append(r), sums.append(cur)
            bounds.append(r + 1), sums.append(c)
            cur = 0
        elif cur + c > max_hits:
            bounds.append(r), sums.append(cur)
            cur = c
        else:
            cur += c
    if bounds[-1] < len(counts):
        bounds.append(len(counts)), sums.append(cur)
    return bounds, sums, sum(1 for s in sums if s > max_hits)
