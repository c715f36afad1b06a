#!/usr/bin/env python3
"""The tail of the optimizer step -- loss, TP/TN/FP/FN, epoch sums -- on train.train's torch route ('off': BCEWithLogitsLoss +
tfpn_counts + the three `+=`) and on the fused route ('on': BCEWithLogitsLoss.with_counts with an EpochStats), each step written
as train.train writes it.  One process per configuration; inside it the two routes alternate epoch by epoch after one warm-up
epoch each, every pair of epochs on the same batches (same generator seed), so that like positions of a pair can be compared.

  --mode minibatch   ClusterGCN epochs (tools/minibatch_epoch.py's setting: --parts clusters, --batch per step, prefetching
                     loader, Adam): seconds and steps per epoch, and -- in a last pass of its own under torch.profiler -- the
                     device activities (kernel launches and copies) per step of both routes
  --mode fullgraph   full-graph steps on one graph (forward + loss + backward + Adam + metrics): milliseconds per step
  --all              runs the three configurations of profiles/loss_counts.json, one child process each, and writes that file

Without --all: one JSON file (--out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CONFIGS = [     # (key, arguments): the two mini-batch settings of DESIGN section 6, the full-graph step at the metric's graph
    ("minibatch_h128_l8_r750k", ["--mode", "minibatch", "--reads", "750000", "--hidden", "128", "--layers", "8", "--count-launches"]),
    ("minibatch_h256_l16_r110k", ["--mode", "minibatch", "--reads", "110000", "--hidden", "256", "--layers", "16", "--count-launches"]),
    ("fullgraph_h128_l8_r750k", ["--mode", "fullgraph", "--reads", "750000", "--hidden", "128", "--layers", "8"]),
]


def run_all(a):
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    res = {"what": "optimizer-step tail (loss + TP/TN/FP/FN + epoch sums): train.train's torch route ('off') against the fused "
                   "loss/count kernel ('on'), routes alternating epoch by epoch in one process per configuration",
           "configurations": {}}
    for key, args in CONFIGS:
        part = os.path.join(out_dir, f"loss_counts_{key}.part.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--out", part, "--runs", str(a.runs), "--parts", str(a.parts),
               "--batch", str(a.batch)] + args
        print("[loss_counts_ab]", " ".join(cmd), flush=True)
        rc = subprocess.call(cmd, timeout=a.child_timeout)
        if rc != 0:                                     # nothing more is started on the device after a failed child
            raise SystemExit(f"{key}: child exited with {rc}")
        with open(part) as f:
            res["configurations"][key] = json.load(f)
        os.remove(part)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v["summary"] for k, v in res["configurations"].items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--mode", choices=("minibatch", "fullgraph"), default="minibatch")
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--parts", type=int, default=500)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=4, help="timed epochs per route (after one warm-up epoch each)")
    ap.add_argument("--steps", type=int, default=10, help="full-graph mode: steps per epoch")
    ap.add_argument("--count-launches", action="store_true", help="a last pass under torch.profiler that counts device activities per step")
    ap.add_argument("--child-timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.all:
        a.out = a.out or os.path.join(REPO, "profiles", "loss_counts.json")
        return run_all(a)

    import torch
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import cluster, dp, synth
    from gnnome_assembly_amd.train import EpochStats, tfpn_counts
    assert torch.cuda.is_available(), "needs a GPU: this tool measures, it has no CPU mode"
    dev = torch.device("cuda:0")
    H, L = a.hidden, a.layers
    src, dst, n = synth.make_graph(a.reads, seed=0)
    inp = synth.make_inputs(src, dst, n, seed=0)
    E = int(src.size)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    g.ndata["pe"] = torch.from_numpy(inp["pe"]).to(dev)
    g.edata["e"] = torch.from_numpy(inp["e"]).to(dev)
    g.edata["y"] = torch.from_numpy(inp["y"]).to(dev)
    g.index()
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, 0, randomize_norm=False).items()})
    model.to(dev)
    model.flatten_parameters()
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    opt = dp.make_adam(model.parameters(), 1e-3)
    crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))
    stats = EpochStats(dev)
    part = cluster.partition_graph(g, a.parts) if a.mode == "minibatch" else None

    def batches(seed):
        if a.mode == "fullgraph":
            return [g] * a.steps
        return cluster.ClusterBatchLoader(g, part, a.batch, shuffle=True, generator=torch.Generator().manual_seed(seed))

    def epoch(route, seed):
        """One epoch as train.train runs it; returns the record and (loss_sum, counts) for the equality check."""
        loader = batches(seed)
        gl = torch.zeros((), device=dev, dtype=torch.float64)
        counts = torch.zeros(4, device=dev, dtype=torch.int64)
        stats.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seen = 0
        for sub in loader:
            flat.zero_()
            pred = model(sub, None, sub.edata["e"], sub.ndata["pe"]).squeeze(-1)
            if route == "on":
                loss = crit.with_counts(pred, sub.edata["y"], stats)[0]
                loss.backward()
                opt.step()
            else:
                loss = crit(pred, sub.edata["y"])
                loss.backward()
                opt.step()
                gl += loss.detach().double()
                counts += tfpn_counts(pred.detach(), sub.edata["y"])
            seen += sub.num_edges()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tot = stats.read() if route == "on" else (float(gl), len(loader), tuple(int(c) for c in counts.tolist()))
        return ({"route": route, "seed": seed, "seconds": round(dt, 5), "steps": len(loader), "ms_per_step": dt * 1e3 / len(loader),
                 "edges_per_s": seen / dt}, tot)

    routes = ("off", "on")
    for r in routes:
        epoch(r, 100)                                    # warm-up: code objects, allocator growth, optimizer state
    epochs, pairs = [], []
    for k in range(a.runs):
        got = {}
        for r in (routes if k % 2 == 0 else routes[::-1]):
            rec, got[r] = epoch(r, k)
            epochs.append(rec)
            print(json.dumps(rec), flush=True)
        off, on = [e for e in epochs[-2:] if e["route"] == "off"][0], [e for e in epochs[-2:] if e["route"] == "on"][0]
        # the weights move between the two epochs of a pair (Adam steps), so their sums differ; both are recorded, not compared
        pairs.append({"seed": k, "first": epochs[-2]["route"], "off_seconds": off["seconds"], "on_seconds": on["seconds"],
                      "on_over_off": on["seconds"] / off["seconds"], "off_totals": got["off"], "on_totals": got["on"]})
    med = {r: float(np.median([e["seconds"] for e in epochs if e["route"] == r])) for r in routes}
    res = {"mode": a.mode, "reads": a.reads, "nodes": n, "edges": E, "hidden": H, "layers": L,
           "num_parts": a.parts if a.mode == "minibatch" else None, "clusters_per_batch": a.batch if a.mode == "minibatch" else None,
           "device": torch.cuda.get_device_name(0), "epochs": epochs, "pairs": pairs,
           "summary": {"median_seconds_per_epoch": med, "steps_per_epoch": epochs[0]["steps"],
                       "median_ms_per_step": {r: med[r] * 1e3 / epochs[0]["steps"] for r in routes},
                       "on_over_off_median": med["on"] / med["off"],
                       "on_over_off_by_pair": [p["on_over_off"] for p in pairs],
                       "device_activities_per_step": None},
           "note": "seconds: host clock around an epoch that ends in a device synchronise; device_activities_per_step: every device "
                   "activity torch.profiler records (kernels, copies, fills) in one epoch over its steps, batch building included"}
    out = a.out or f"loss_counts_ab_{a.mode}_h{H}l{L}.json"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    if a.count_launches:      # last, in a pass of its own: tracing slows the host, no time above was taken under the profiler
        try:
            from torch.profiler import ProfilerActivity, profile
            acts = {}
            for r in routes:
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    rec, _ = epoch(r, 0)
                evs = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
                acts[r] = len(evs) / rec["steps"] if evs else None
            res["summary"]["device_activities_per_step"] = acts
        except Exception as ex:      # the profiler is optional: the count is reported as missing, never guessed
            print(f"torch.profiler unavailable: {ex!r}", flush=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res["summary"]))


if __name__ == "__main__":
    main()
