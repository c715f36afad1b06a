#!/usr/bin/env python
"""What the overlap alignment (features.overlap_features: gnm_overlap_align, one launch) costs on the benchmark's synthetic graph.

  graph        synth.make_graph(--reads): 2 * reads nodes, ~5 edges per node (the benchmark's topology).
  reads        cut on the device from one random genome: read r covers [r * stride, r * stride + length_r), length uniform in
               [--min-len, --max-len]; then a seeded per-base SUBSTITUTION rate (--error-rate; no indels: the cut stays a fixed-size
               tensor operation) is applied to every read on its own.  prefix_length of an edge u -> v is the distance of the two
               reads' starts when both nodes are + strands (ends, when both are - strands) and half the source read otherwise --
               such an edge has no true overlap and ends as `exceeded`, which the share reported below shows.
  launch       device events around ONE gnm_overlap_align per window, after a warm-up launch, --runs windows per configuration
               (--max-errors K, on the first --sample share of the edges); the median is reported, with the windows.
  rates        band cell updates per second counting (2 K + 1) * (m + K) per valid, non-empty edge, and DP cells (the record's
               `cells`, aligned edges only) per second.
  host         gnm_overlap_align_host on 16 threads over 1 % of the edges, on the host clock, equal outputs checked.

One process, one JSON file (--out, default profiles/overlap_align.json).  No speed was promised in advance; nothing here asserts one."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def build(reads, lo, hi, stride, rate, seed, dev):
    import torch
    from gnnome_assembly_amd import synth
    from gnnome_assembly_amd.reads import ReadStore
    src, dst, n = synth.make_graph(reads, seed=seed)
    gen = torch.Generator(device=dev).manual_seed(seed)
    R = (n + 1) // 2
    length = torch.randint(lo, hi + 1, (R,), device=dev, generator=gen)
    start = torch.arange(R, device=dev) * stride
    span = (length + 31) // 32 * 32
    base_off = torch.cumsum(span, 0) - span
    total = int(span.sum())
    genome = (1 << torch.randint(0, 4, (int(start[-1]) + hi + 32,), device=dev, generator=gen)).to(torch.uint8)   # A C G T
    read_of = torch.repeat_interleave(torch.arange(R, device=dev), span, output_size=total)
    t = torch.arange(total, device=dev) - base_off[read_of]
    nib = genome[start[read_of] + torch.minimum(t, length[read_of] - 1)]
    hit = torch.rand(total, device=dev, generator=gen) < rate
    rot = torch.randint(1, 4, (total,), device=dev, generator=gen).to(torch.uint8)
    nib = torch.where(hit, ((nib << rot) | (nib >> (4 - rot))) & 15, nib)                    # another of the four bases
    nib = torch.where(t < length[read_of], nib, torch.zeros_like(nib))                       # pad nibbles are 0
    packed = (nib[0::2] | (nib[1::2] << 4)).contiguous()
    del genome, read_of, t, hit, rot, nib
    store = ReadStore(packed, base_off, length)
    s, d = torch.from_numpy(src).to(dev).long(), torch.from_numpy(dst).to(dev).long()
    rs, rd = s >> 1, d >> 1
    end = start + length
    both_even, both_odd = ((s | d) & 1) == 0, ((s & d) & 1) == 1
    pl = torch.where(both_even, start[rd] - start[rs], torch.where(both_odd, end[rs] - end[rd], length[rs] // 2))
    pl = torch.minimum(pl.clamp(min=0), length[rs])
    return src, dst, n, store, pl, length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--min-len", type=int, default=300)
    ap.add_argument("--max-len", type=int, default=900)
    ap.add_argument("--stride", type=int, default=100)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--max-errors", default="31,255", help="comma-separated K, one configuration each")
    ap.add_argument("--sample", default="1.0,0.1", help="share of the edges per configuration")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-share", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "overlap_align.json"))
    a = ap.parse_args()
    import torch
    from gnnome_assembly_amd import _lib, engine
    if not torch.cuda.is_available():
        sys.exit("align_ab: needs a HIP device (a measurement does not fall back)")
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    src, dst, n, store, pl, length = build(a.reads, a.min_len, a.max_len, a.stride, a.error_rate, a.seed, dev)
    torch.cuda.synchronize()
    E = src.size
    s_d, d_d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    m_all = length[s_d.long() >> 1] - pl
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha": _lib.csrc_sha(), "args": vars(a), "nodes": int(n), "edges": int(E),
           "store_bytes": int(store.packed.numel()), "mean_overlap_length": float(m_all.double().mean()),
           "build_seconds": time.perf_counter() - t0, "configurations": []}
    print(f"graph: {n} nodes, {E} edges, store {store.packed.numel() / 1e6:.1f} MB, mean m {res['mean_overlap_length']:.1f}", flush=True)
    Ks = [int(x) for x in a.max_errors.split(",")]
    shares = [float(x) for x in a.sample.split(",")]
    outs = {}
    for K, share in zip(Ks, shares):
        Es = max(1, int(E * share))
        sl = slice(0, Es)
        dist = torch.empty(Es, dtype=torch.int32, device=dev)
        olen = torch.empty(Es, dtype=torch.int64, device=dev)
        sim = torch.empty(Es, dtype=torch.float32, device=dev)
        rec = torch.zeros(engine.ALIGN_RECORD_WORDS, dtype=torch.int64, device=dev)
        ss, dd, pp = s_d[sl].contiguous(), d_d[sl].contiguous(), pl[sl].contiguous()
        ms = []
        for run in range(a.runs + 1):                       # window 0 is the warm-up
            rec.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            engine.overlap_align(ss, dd, pp, n, store.base_off, store.length, store.packed, K, dist, olen, sim, rec)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            print(f"K={K} edges={Es} window {run}: {ms[-1]:.2f} ms", flush=True)
        r = dict(zip(engine.ALIGN_COUNTERS, rec.cpu().tolist()))
        m = olen.double()
        work = m > 0
        band = float((((2 * K + 1) * (m + K)) * work).sum())
        med = float(np.median(ms[1:]))
        res["configurations"].append({
            "max_errors": K, "band_words": 1 if K <= 31 else 2 if K <= 63 else 4 if K <= 127 else 8, "edges": Es,
            "windows_ms": ms[1:], "warmup_ms": ms[0], "median_ms_per_launch": med, "record": r,
            "exceeded_share": r["exceeded"] / max(1, r["edges"]),
            "band_cell_updates": band, "band_cell_updates_per_second": band / (med * 1e-3),
            "dp_cells_aligned_per_second": r["cells"] / (med * 1e-3)})
        outs[K] = (dist, olen, sim)
        print(json.dumps(res["configurations"][-1]), flush=True)
    # the host entry point on 16 threads over a share of the edges
    K = Ks[0]
    Eh = max(1, int(E * a.host_share))
    cpu = lambda t: t.cpu().contiguous()  # noqa: E731
    hs, hd, hp = cpu(s_d[:Eh]), cpu(d_d[:Eh]), cpu(pl[:Eh])
    hb, hl, hk = cpu(store.base_off), cpu(store.length), cpu(store.packed)
    hdist, holen, hsim = torch.empty(Eh, dtype=torch.int32), torch.empty(Eh, dtype=torch.int64), torch.empty(Eh, dtype=torch.float32)
    hrec = torch.zeros(engine.ALIGN_RECORD_WORDS, dtype=torch.int64)
    t1 = time.perf_counter()
    engine.overlap_align_host(hs, hd, hp, n, hb, hl, hk, K, hdist, holen, hsim, hrec, threads=16)
    host_s = time.perf_counter() - t1
    same = bool(torch.equal(hdist, outs[K][0][:Eh].cpu()) and torch.equal(holen, outs[K][1][:Eh].cpu())
                and torch.equal(hsim, outs[K][2][:Eh].cpu()))
    res["host"] = {"max_errors": K, "edges": Eh, "threads": 16, "seconds": host_s, "edges_per_second": Eh / host_s,
                   "equal_to_device": same}
    print(json.dumps(res["host"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not same:
        sys.exit("align_ab: the host entry point and the device disagree")


if __name__ == "__main__":
    main()
