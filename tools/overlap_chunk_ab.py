#!/usr/bin/env python
"""What bounding the resident seed hits costs: overlap.find_overlaps(max_hits=...) on the reads tools/overlap_ab.py builds.

  settings     max_hits = None (all hits resident), total / 4 and total / 16, total = the hits of the data set.
  protocol     per setting one warm-up call, then --runs calls, each between two device events with the peak-memory counter reset
               before it; the median and the calls are reported, with torch.cuda.max_memory_allocated, chunks and peak_hits.
  check        every chunked result is compared with the unchunked one (edges, edge data, contained, record); a difference ends
               the run with an error.
One process, one JSON file (--out, default profiles/overlap_chunked.json).  Recorded only: nothing asserts a time or a byte count,
and the chunked route may well be slower at a size that fits.  The memory figure includes the store, the sketch and the
candidate edges, which stay resident in every setting."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=2_000_000)
    ap.add_argument("--coverage-fold", type=float, default=20.0)
    ap.add_argument("--min-len", type=int, default=5000)
    ap.add_argument("--max-len", type=int, default=15000)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "overlap_chunked.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from overlap_ab import make_reads
    from gnnome_assembly_amd import engine, overlap
    from gnnome_assembly_amd.reads import ReadStore
    if not torch.cuda.is_available():
        raise SystemExit("overlap_chunk_ab: needs a HIP device; a CPU run measures nothing")
    dev = torch.device("cuda:0")
    reads, _, _ = make_reads(a.genome, a.coverage_fold, a.min_len, a.max_len, a.error_rate, a.seed)
    store = ReadStore.from_sequences(reads).to(dev)
    p = dict(k=21, w=25, max_occ=64, min_hits=4, band=32, min_overlap=500, max_errors=255)

    def one_call(max_hits):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        e0.record()
        og = overlap.find_overlaps(store, max_hits=max_hits, **p)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), torch.cuda.max_memory_allocated(dev), og

    def equal(x, y):
        return (all(torch.equal(s, t) for s, t in zip(x.graph.edges(), y.graph.edges())) and sorted(x.graph.edata) == sorted(y.graph.edata)
                and all(torch.equal(x.graph.edata[k], y.graph.edata[k]) for k in y.graph.edata) and torch.equal(x.contained, y.contained)
                and x.stats == y.stats and x.exceeded_pairs == y.exceeded_pairs)

    base = one_call(None)[2]
    total = base.hit_count
    settings = []
    for name, m in (("None", None), ("total/4", total // 4), ("total/16", total // 16)):
        one_call(m)                                          # the warm-up call
        calls = [one_call(m) for _ in range(a.runs)]
        og = calls[-1][2]
        if not equal(og, base):
            raise SystemExit(f"overlap_chunk_ab: max_hits={m} differs from the unchunked result")
        settings.append(dict(setting=name, max_hits=m, median_ms=statistics.median(c[0] for c in calls), calls_ms=[c[0] for c in calls],
                             peak_memory_bytes=max(c[1] for c in calls), chunks=og.chunks, peak_hits=og.peak_hits,
                             oversize_chunks=og.oversize_chunks))
        del calls, og
    out = dict(
        what="overlap.find_overlaps(max_hits=...) on synthetic reads: whole-call time in ms (device events, one warm-up call, the "
             "median of the calls) and torch.cuda.max_memory_allocated over a call; every chunked result equals the unchunked one",
        device=torch.cuda.get_device_name(0), parameters=p,
        data=dict(genome_bases=a.genome, reads=len(reads), bases=int(sum(len(r) for r in reads)), min_len=a.min_len, max_len=a.max_len,
                  substitution_rate=a.error_rate, indels="none", strands="both", packed_bytes=int(store.packed.numel())),
        record=dict(zip(engine.OVERLAP_COUNTERS, base.stats.words())), edges=base.graph.num_edges(), hits=total, settings=settings,
        not_measured=["kernel times by rocprofv3", "chromosome-scale data", "any budget other than these three",
                      "memory held outside the torch allocator"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(dict(hits=total, settings=[{k: s[k] for k in ("setting", "median_ms", "peak_memory_bytes", "chunks", "peak_hits")}
                                                for s in settings])))


if __name__ == "__main__":
    main()
