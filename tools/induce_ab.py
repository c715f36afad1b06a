#!/usr/bin/env python3
"""Mini-batch epochs with the batches built by the 'sort' route (cluster.induced_subgraph + graph.tensor_index) and by the
'index' route (gnm_graph_induce_count / _fill), in ONE process on one graph, the routes alternating epoch by epoch (the setting
of tools/minibatch_epoch.py: 500 parts, 50 per batch, prefetching loader, Adam step).  Every pair of epochs draws the same batches
(same generator seed).  Also the build alone -- sub-graph + index + both sweep plans of every batch of one epoch, on a side stream
with the device otherwise idle: milliseconds per batch by device events, kernel launches per batch counted by torch.profiler
(--count-launches; `null` otherwise).  Writes one JSON file (--out; profiles/induce_index.json keeps both configurations of such runs)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--parts", type=int, default=500)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3, help="timed epochs per route (after one warm-up epoch each)")
    ap.add_argument("--count-launches", action="store_true", help="a last pass under torch.profiler that counts the build's launches")
    ap.add_argument("--out", default=None, help="result file (default: induce_ab_h{H}l{L}.json in the current directory)")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=8)
    a = ap.parse_args()
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import cluster, dp, engine, synth
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
    part = cluster.partition_graph(g, a.parts)
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, 0, randomize_norm=False).items()})
    model.to(dev)
    model.flatten_parameters()
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    opt = dp.make_adam(model.parameters(), 1e-3)
    crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))

    def epoch(route, seed):
        loader = cluster.ClusterBatchLoader(g, part, a.batch, shuffle=True, generator=torch.Generator().manual_seed(seed), induce=route)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seen = 0
        for sub in loader:
            flat.zero_()
            s = model(sub, None, sub.edata["e"], sub.ndata["pe"])
            crit(s.squeeze(-1), sub.edata["y"]).backward()
            opt.step()
            seen += sub.num_edges()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"route": route, "seed": seed, "seconds": round(dt, 4), "steps": len(loader), "edges_in_batches": seen,
                "edges_per_s": seen / dt}

    routes = ("sort", "index")
    for r in routes:
        epoch(r, 100)                                    # warm-up: code objects, allocator growth, optimizer state
    epochs = []
    for k in range(a.runs):
        for r in (routes if k % 2 == 0 else routes[::-1]):
            epochs.append(epoch(r, k))
            print(json.dumps(epochs[-1]), flush=True)

    side = torch.cuda.Stream(device=dev)

    def builds(route, seed):
        loader = cluster.ClusterBatchLoader(g, part, a.batch, shuffle=True, generator=torch.Generator().manual_seed(seed), prefetch=False,
                                            induce=route)
        out = []
        with torch.cuda.stream(side):
            for ids in loader.batches():
                sub = loader._build(ids)
                sub.index(dev)
                sub.sweep_plan(dev, 1)
                sub.sweep_plan(dev, engine.GATE2_WG)
                out.append(sub)
        side.synchronize()
        return len(out)

    build = {}
    for r in routes:
        builds(r, 0)
        ms = []
        for k in range(a.runs):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            t0 = time.perf_counter()
            nb = builds(r, k)
            e1.record(side)
            side.synchronize()
            ms.append({"device_ms_per_batch": e0.elapsed_time(e1) / nb, "host_ms_per_batch": (time.perf_counter() - t0) * 1e3 / nb})
        build[r] = {"runs": ms, "median_device_ms_per_batch": float(np.median([m["device_ms_per_batch"] for m in ms])),
                    "median_host_ms_per_batch": float(np.median([m["host_ms_per_batch"] for m in ms])),
                    "device_launches_per_batch": None}
        print(json.dumps({r: build[r]}), flush=True)

    med = {r: float(np.median([ep["edges_per_s"] for ep in epochs if ep["route"] == r])) for r in routes}
    res = {"what": "ClusterGCN mini-batch epochs, batches built by the 'sort' and by the 'index' route, alternating in one process",
           "reads": a.reads, "nodes": n, "edges": E, "hidden": H, "layers": L, "num_parts": a.parts, "clusters_per_batch": a.batch,
           "device": torch.cuda.get_device_name(0), "epochs": epochs, "median_edges_per_s": med,
           "index_over_sort": med["index"] / med["sort"],
           "build_alone": build,
           "note": "build_alone: sub-graph + index + both sweep plans of each batch, side stream, device otherwise idle, prefetch off; "
                   "device_launches_per_batch counts every device activity torch.profiler records (kernels and copies)"}
    print(json.dumps({k: res[k] for k in ("hidden", "layers", "median_edges_per_s", "index_over_sort")}))
    out = a.out or f"induce_ab_h{H}l{L}.json"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    # the launch counts last, in a pass of their own (tracing slows the host: no time above was taken under the profiler)
    if not a.count_launches:
        return
    try:
        from torch.profiler import ProfilerActivity, profile
        for r in routes:
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                nb = builds(r, 0)
            kernels = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
            build[r]["device_launches_per_batch"] = len(kernels) / nb if kernels else None
            print(json.dumps({r: build[r]["device_launches_per_batch"]}), flush=True)
    except Exception as ex:      # the profiler is optional: the count is reported as missing, never guessed
        print(f"torch.profiler unavailable: {ex!r}", flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
