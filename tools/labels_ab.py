#!/usr/bin/env python3
"""Measure the ground-truth labels (labels.ground_truth_labels) at chromosome scale and write profiles/gt_labels.json.

Graph: synth.make_graph at R reads (default 750,000), with positions made up to fit its banded structure: read i is node 2i, starts at
i * step and is (max_degree + 1) * step - 1 long, so every listed neighbour i + 1 .. i + 16 overlaps it; the 0.5 % long-range edges
come out as gap or backward edges.  Recorded: per stage the wall time between synchronisations (the read-backs are part of the
stage), rounds and launches, median / min / max over --repeats runs after --warmup runs on an otherwise idle device; the host entry's
time beside it; the equality of the two routes' outputs; VGPRs / waves per SIMD / LDS / scratch per kernel from a gfx950 compile of
csrc/gnm_labels.hip (when hipcc is there); and, from tests/golden/labels/gt_labels.npz, the share of the library's positives the
reference's walk-based labels hold as well (a measurement without a bar: the reference labels one walk per component).
    python tools/labels_ab.py [--reads 750000] [--repeats 5] [--warmup 2] [--out profiles/gt_labels.json]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gnnome_assembly_amd import AssemblyGraph, _lib, engine, labels, synth  # noqa: E402


def positions(R, step=1000, max_degree=16):
    start = np.repeat(np.arange(R, dtype=np.int64) * step, 2)
    end = start + (max_degree + 1) * step - 1
    strand = np.tile(np.asarray([1, -1], np.int64), R)
    return tuple(torch.from_numpy(a) for a in (start, end, strand))


def staged(g, pos, dev):
    """one run of engine.gt_labels' sequence with a synchronisation and a clock after every stage"""
    idx = g.index(dev)
    n, E = g.num_nodes(), g.num_edges()
    start, end, strand = (t.to(dev) for t in pos)
    src, dst = (t.to(torch.int32).contiguous() for t in g.edges())
    new = lambda m, dt: torch.empty(m, dtype=dt, device=dev)  # noqa: E731
    out = (new(E, torch.float32), new(E, torch.uint8), new(n, torch.uint8), new(n, torch.int32), new(n, torch.int32))
    rec = torch.zeros(engine.GT_RECORD_WORDS, dtype=torch.int64, device=dev)
    lib = _lib.load()
    need = int(lib.gnm_gt_workspace_bytes(n, E))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    p = engine._ptr
    head = (n, E, *[p(idx[k]) for k in engine._GT_INDEX_KEYS], p(idx.get("nperm")), p(idx.get("nrank")))
    tail = (p(ws), need, engine._stream())
    batch = engine.GT_ROUNDS_PER_BATCH
    changed = torch.empty(batch, dtype=torch.int64, device=dev)
    ms, rounds, launches = {}, {}, {}

    def clock(name, t0):
        torch.cuda.synchronize()
        ms[name] = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    engine._call("gnm_gt_prepare", *head, p(start), p(end), p(strand), p(rec), *tail)
    clock("prepare", t0)
    launches["prepare"] = 2
    for stage, name in enumerate(engine._GT_STAGES):
        t0, done, calls = time.perf_counter(), 0, 0
        while True:
            engine._call("gnm_gt_rounds", *head, stage, done, batch, p(changed), *tail)
            calls += 1
            got = changed.tolist()
            if 0 in got:
                done += got.index(0) + 1
                break
            done += batch
        clock(name, t0)
        rounds[name] = done
        launches[name] = calls * (batch + 1) + (0, 1, 2)[stage]
    t0 = time.perf_counter()
    engine._call("gnm_gt_emit", *head, None, p(src), p(dst), *[p(t) for t in out], p(rec), *tail)
    clock("emit", t0)
    launches["emit"] = 2
    ms["total"] = sum(ms.values())
    return ms, rounds, launches, out, rec, need


def kernel_resources():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    csrc = os.path.join(REPO, "gnnome_assembly_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-I", os.path.join(REPO, "include"),
                            "-I", csrc, "-c", os.path.join(csrc, "gnm_labels.hip"), "-o", os.path.join(tmp, "l.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN3gnm\d+", "", m.group(1))
            name = re.sub(r"(_k)(ILi(\d)E)?.*$", lambda q: q.group(1) + (f"<{q.group(3)}>" if q.group(3) else ""), name)
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or None


def reference_share():
    path = os.path.join(REPO, "tests", "golden", "labels", "gt_labels.npz")
    if not os.path.exists(path):
        return None
    z, rows = np.load(path), []
    for i in range(int(z["graphs"])):
        g = AssemblyGraph(z[f"src_{i}"], z[f"dst_{i}"], int(z[f"start_{i}"].size))
        gt = labels.ground_truth_labels(g, *(torch.from_numpy(z[f"{k}_{i}"]) for k in ("start", "end", "strand")))
        pos = torch.from_numpy(z[f"positive_{i}"])
        rows.append({"seed": int(z[f"seed_{i}"]), "edges": int(gt.y.numel()), "positives": int(gt.y.sum()), "reference_positives": int(pos.numel()),
                     "reference_positives_labelled_here": int(gt.y[pos].sum()),
                     "share_of_positives_the_reference_has": float(gt.y[pos].sum() / max(float(gt.y.sum()), 1.0))})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gt_labels.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    src, dst, n = synth.make_graph(a.reads, seed=0)
    pos = positions(a.reads)
    g = AssemblyGraph(src, dst, n)
    t0 = time.perf_counter()
    host = labels.ground_truth_labels(g, *pos)
    host_ms = (time.perf_counter() - t0) * 1e3
    gd = g.to(dev)
    gd.index(dev)
    runs = []
    for i in range(a.warmup + a.repeats):
        ms, rounds, launches, out, rec, ws_bytes = staged(gd, pos, dev)
        if i >= a.warmup:
            runs.append((ms, rounds))
    equal = bool(torch.equal(out[0].cpu(), host.y) and torch.equal(out[1].cpu().bool(), host.valid) and
                 torch.equal(out[2].cpu().bool(), host.backbone) and torch.equal(out[3].cpu(), host.component) and
                 torch.equal(out[4].cpu(), host.top))
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    result = {
        "what": "labels.ground_truth_labels on synth.make_graph with made-up banded positions; wall ms between synchronisations",
        "device": torch.cuda.get_device_name(0), "reads": a.reads, "nodes": n, "edges": int(src.size),
        "repeats": a.repeats, "warmup": a.warmup, "rounds_per_batch": engine.GT_ROUNDS_PER_BATCH, "sweeps_per_round": engine.gt_sweeps(),
        "workspace_bytes": ws_bytes, "relabelled_index": "nperm" in gd.index(dev),
        "stage_ms": {k: stat([m[k] for m, _ in runs]) for k in runs[0][0]},
        "rounds": {k: stat([r[k] for _, r in runs]) for k in runs[0][1]}, "launches_last_run": launches,
        "host_entry_ms": host_ms, "device_equals_host": equal,
        "record": dict(zip(engine.GT_COUNTERS, rec.cpu().tolist())),
        "kernels_gfx950": kernel_resources(), "reference_containment": reference_share(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("stage_ms", "rounds", "host_entry_ms", "device_equals_host")}))


if __name__ == "__main__":
    main()
