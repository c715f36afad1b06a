#!/usr/bin/env python
"""What overlap.find_overlaps costs, stage by stage, on synthetic HiFi-like reads.

  reads        cut on the host from one random genome (--genome bases): --coverage-fold reads of --min-len .. --max-len bases at
               uniform starts, each on a random strand, each with a seeded per-base SUBSTITUTION rate (--error-rate, default 1 %; no
               indels: the cut stays a vectorised array operation, and a read keeps its true length).  The size is stated in the
               output; it fits the device comfortably and is NOT chromosome scale, which nobody has measured.
  stages       device events around every stage and every sort between them (sketch, sort by hash, seed hits, the two sorts of the
               hits, chains, verification + assembly), one warm-up pass, then --runs passes; medians and the passes are reported.
  counts       minimizers, hits, groups and the rest of the record; bytes per hit held by the stages themselves.
  quality      recall and precision of the found read pairs against the pairs whose true overlap (from the read positions) is at
               least min_overlap and of which neither read contains the other.
  memory       torch.cuda.max_memory_allocated over a pass.
One process, one JSON file (--out, default profiles/overlap_find.json).  Nothing here asserts a time; kernel times by rocprofv3 and
the share of peak were NOT measured."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
COMP = np.zeros(256, np.uint8)
for a_, b_ in zip(b"ACGT", b"TGCA"):
    COMP[a_] = b_


def make_reads(genome_len, fold, lo, hi, rate, seed):
    rng = np.random.default_rng(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, genome_len)]
    n = int(genome_len * fold / ((lo + hi) / 2))
    start = rng.integers(0, genome_len - hi, n)
    end = start + rng.integers(lo, hi + 1, n)
    strand = rng.integers(0, 2, n)
    reads = []
    for s, e, t in zip(start, end, strand):
        r = genome[s:e].copy()
        hit = rng.random(r.size) < rate
        r[hit] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), r[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
        reads.append((COMP[r[::-1]] if t else r).tobytes())
    return reads, start, end


def true_pairs(start, end, min_overlap):
    ov = np.minimum(end[:, None], end[None, :]) - np.maximum(start[:, None], start[None, :])
    inside = (start[:, None] <= start[None, :]) & (end[None, :] <= end[:, None])           # column read inside row read
    contained = (inside & ~np.eye(start.size, dtype=bool)).any(axis=0)
    ok = (ov >= min_overlap) & ~inside & ~inside.T & ~contained[:, None] & ~contained[None, :]
    i, j = np.nonzero(np.triu(ok, 1))
    return set(zip(i.tolist(), j.tolist())), contained


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=2_000_000)
    ap.add_argument("--coverage-fold", type=float, default=20.0)
    ap.add_argument("--min-len", type=int, default=5000)
    ap.add_argument("--max-len", type=int, default=15000)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "overlap_find.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import engine, overlap
    from gnnome_assembly_amd.reads import ReadStore
    if not torch.cuda.is_available():
        raise SystemExit("overlap_ab: needs a HIP device; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    reads, start, end = make_reads(a.genome, a.coverage_fold, a.min_len, a.max_len, a.error_rate, a.seed)
    store = ReadStore.from_sequences(reads).to(dev)
    p = dict(k=21, w=25, max_occ=64, min_hits=4, band=32, min_overlap=500, max_errors=255)

    def one_pass():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        rec = torch.zeros(engine.OVERLAP_RECORD_WORDS, dtype=torch.int64, device=dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ev[0].record()
        h, rd, ps, st = engine.sketch(store.base_off, store.length, store.packed, p["k"], p["w"], rec)
        ev[1].record()
        h, o = torch.sort(h, stable=True)
        rd, ps, st = rd[o].contiguous(), ps[o].contiguous(), st[o].contiguous()
        ev[2].record()
        key, diag = engine.seed_pairs(h, rd, ps, st, store.length, p["k"], p["max_occ"], rec)
        ev[3].record()
        diag, o = torch.sort(diag, stable=True)
        key, o2 = torch.sort(key[o], stable=True)
        diag = diag[o2].contiguous()
        ev[4].record()
        engine.chain_pairs(key, diag, store.length, p["band"], p["min_hits"], p["min_overlap"], rec)
        ev[5].record()
        del h, rd, ps, st, key, diag, o, o2
        og = overlap.find_overlaps(store, **p)
        ev[6].record()
        torch.cuda.synchronize()
        names = ("sketch", "sort_by_hash", "seed_pairs", "sort_hits", "chain_pairs", "find_overlaps_whole")
        return {n_: ev[i].elapsed_time(ev[i + 1]) for i, n_ in enumerate(names)}, og, torch.cuda.max_memory_allocated(dev)

    one_pass()
    passes = [one_pass() for _ in range(a.runs)]
    og = passes[-1][1]
    src, dst = og.graph.edges()
    found = {(min(x, y), max(x, y)) for x, y in zip((src >> 1).tolist(), (dst >> 1).tolist())}
    truth, contained = true_pairs(start, end, p["min_overlap"])
    got_c = og.contained.cpu().numpy()
    out = dict(
        what="overlap.find_overlaps on synthetic reads; times in ms (device events; each stage includes its one size read-back), "
             "medians of the passes after one warm-up pass; find_overlaps_whole is a complete second run including verification",
        device=torch.cuda.get_device_name(0), parameters=p,
        data=dict(genome_bases=a.genome, reads=len(reads), bases=int(sum(len(r) for r in reads)), min_len=a.min_len, max_len=a.max_len,
                  substitution_rate=a.error_rate, indels="none", strands="both", packed_bytes=int(store.packed.numel())),
        median_ms={k: statistics.median(t[0][k] for t in passes) for k in passes[0][0]},
        passes_ms=[t[0] for t in passes],
        record=dict(zip(engine.OVERLAP_COUNTERS, og.stats.words())), edges=og.graph.num_edges(), exceeded_pairs=og.exceeded_pairs,
        bytes_per_hit=dict(key=8, diag=4, count_offset=8, sort_temporaries="two int64 index arrays and the sorted copies (torch.sort)"),
        peak_memory_bytes=max(t[2] for t in passes),
        quality=dict(true_pairs=len(truth), found_pairs=len(found), recall=len(truth & found) / max(1, len(truth)),
                     precision=len(truth & found) / max(1, len(found)), contained_true=int(contained.sum()),
                     contained_found=int(got_c.sum()), contained_agree=int((got_c == contained).sum())),
        not_measured=["kernel times by rocprofv3", "share of peak bandwidth or issue rate", "reads with indels", "chromosome-scale data",
                      "any parameter other than the defaults"])
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms", "record", "quality", "peak_memory_bytes")}))


if __name__ == "__main__":
    main()
