#!/usr/bin/env python3
"""The optimizer step of train.train on its two routes: 'torch' (flat.zero_() + backward + dp.make_adam's fused Adam) against
'library' (backward + dp.LibAdam.step(zero_grad=True): gnm_optim_grad_stats + gnm_optim_adam_step, the explicit zero only before
an epoch's first step), each step written as train.train writes it.  One process per configuration; inside it the two routes
alternate epoch by epoch after one warm-up epoch each, every pair of epochs on the same batches (same generator seed).

  --mode minibatch   ClusterGCN epochs (--parts clusters, --batch per step): milliseconds per step, and -- in a last pass of its
                     own under torch.profiler -- the device activities (kernel launches, copies, fills) per step of both routes
  --mode fullgraph   full-graph steps on one graph: milliseconds per step, the same count
  --all              the three configurations of profiles/optim_step.json, one child process each; keeps the file's "accuracy"
                     entry (the pairs tests/test_gpu_optim.py measures) if there is one

Both routes also get the two kernels alone timed on the model's flat buffers (HIP events, --kernel-reps calls).
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

CONFIGS = [     # the full-graph step at the metric's shape; the two mini-batch settings of DESIGN section 6 (500 parts, 50 per batch)
    ("fullgraph_h128_l8_r750k", ["--mode", "fullgraph", "--reads", "750000", "--hidden", "128", "--layers", "8"]),
    ("minibatch_h128_l8_r750k", ["--mode", "minibatch", "--reads", "750000", "--hidden", "128", "--layers", "8"]),
    ("minibatch_h256_l16_r110k", ["--mode", "minibatch", "--reads", "110000", "--hidden", "256", "--layers", "16"]),
]


def run_all(a):
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    res = {"what": "optimizer step: train.train's torch route (flat.zero_ + fused torch Adam) against the library route "
                   "(dp.LibAdam: two launches, gradient left zeroed), routes alternating epoch by epoch in one process per configuration",
           "configurations": {}}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "accuracy" in old:
            res["accuracy"] = old["accuracy"]
    for key, args in CONFIGS:
        part = os.path.join(out_dir, f"optim_step_{key}.part.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--out", part, "--runs", str(a.runs), "--parts", str(a.parts),
               "--batch", str(a.batch), "--count-launches"] + args
        print("[optim_step_ab]", " ".join(cmd), flush=True)
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
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--count-launches", action="store_true", help="a last pass under torch.profiler that counts device activities per step")
    ap.add_argument("--child-timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.all:
        a.out = a.out or os.path.join(REPO, "profiles", "optim_step.json")
        return run_all(a)

    import torch
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import cluster, dp, synth
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
    opts = {"torch": dp.make_adam(model.parameters(), 1e-3), "library": dp.LibAdam(model.parameters(), 1e-3, flat=flat)}
    crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))
    part = cluster.partition_graph(g, a.parts) if a.mode == "minibatch" else None

    def batches(seed):
        if a.mode == "fullgraph":
            return [g] * a.steps
        return cluster.ClusterBatchLoader(g, part, a.batch, shuffle=True, generator=torch.Generator().manual_seed(seed))

    def epoch(route, seed):
        """One epoch as train.train runs it on `route`."""
        loader = batches(seed)
        opt = opts[route]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = True
        for sub in loader:
            if route == "torch" or first:
                flat.zero_()
                first = False
            pred = model(sub, None, sub.edata["e"], sub.ndata["pe"]).squeeze(-1)
            crit(pred, sub.edata["y"]).backward()
            flat.all_reduce_mean()
            if route == "library":
                opt.step(zero_grad=True)
            else:
                opt.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"route": route, "seed": seed, "seconds": round(dt, 5), "steps": len(loader), "ms_per_step": dt * 1e3 / len(loader)}

    routes = ("torch", "library")
    for r in routes:
        epoch(r, 100)                                    # warm-up: code objects, allocator growth, optimizer state
    epochs, pairs = [], []
    for k in range(a.runs):
        for r in (routes if k % 2 == 0 else routes[::-1]):
            epochs.append(epoch(r, k))
            print(json.dumps(epochs[-1]), flush=True)
        t, l_ = [e for e in epochs[-2:] if e["route"] == "torch"][0], [e for e in epochs[-2:] if e["route"] == "library"][0]
        pairs.append({"seed": k, "first": epochs[-2]["route"], "torch_ms_per_step": t["ms_per_step"], "library_ms_per_step": l_["ms_per_step"],
                      "library_over_torch": l_["seconds"] / t["seconds"]})
    med = {r: float(np.median([e["ms_per_step"] for e in epochs if e["route"] == r])) for r in routes}

    # the step alone, on the model's own flat buffers: zero + fused Adam against the two library kernels
    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.kernel_reps

    def torch_step():
        opts["torch"].step()
        flat.zero_()
    alone = {"torch_zero_plus_fused_adam_us": timed(torch_step), "library_two_kernels_us": timed(lambda: opts["library"].step(zero_grad=True))}
    res = {"mode": a.mode, "reads": a.reads, "nodes": n, "edges": E, "hidden": H, "layers": L, "parameters": int(flat.grads.numel()),
           "num_parts": a.parts if a.mode == "minibatch" else None, "clusters_per_batch": a.batch if a.mode == "minibatch" else None,
           "device": torch.cuda.get_device_name(0), "epochs": epochs, "pairs": pairs,
           "summary": {"median_ms_per_step": med, "steps_per_epoch": epochs[0]["steps"],
                       "library_over_torch_median": med["library"] / med["torch"],
                       "library_over_torch_by_pair": [p["library_over_torch"] for p in pairs],
                       "optimizer_step_alone_us": alone, "device_activities_per_step": None},
           "note": "ms_per_step: host clock around an epoch that ends in a device synchronise, over its steps; optimizer_step_alone_us: "
                   "HIP events around back-to-back calls (host launch cost included); device_activities_per_step: every device activity "
                   "torch.profiler records (kernels, copies, fills) in one epoch over its steps, batch building included"}
    out = a.out or f"optim_step_ab_{a.mode}_h{H}l{L}.json"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    if a.count_launches:      # last, in a pass of its own: tracing slows the host, no time above was taken under the profiler
        try:
            from torch.profiler import ProfilerActivity, profile
            acts = {}
            for r in routes:
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    rec = epoch(r, 0)
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
