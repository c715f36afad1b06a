"""Per-launch time of gnm_node_dropout_apply at the metric's graph (N = 1.5 M nodes, H = 128), beside an [N,H] elementwise kernel
of the step measured in the same process (gnm_node_update_fwd: two [N,H] reads, one write), and beside that kernel's time in
profiles/r06_kernel_stats_serial.csv.  Device events around `reps` back-to-back launches, the two kernels alternating block by
block, after a warm-up of each.  Bytes are the algorithm's: one [N,H] read and one write for the dropout.

    python tools/dropout_cost.py OUT.json [--nodes 1500000] [--hidden 128] [--reps 50] [--blocks 6]
Nothing gates on the result; it is a recorded cost (profiles/dropout.json)."""
import argparse
import csv
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gnnome_assembly_amd import _lib, engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--nodes", type=int, default=1500000)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device (no CPU timing)"
    dev = torch.device("cuda:0")
    N, H = a.nodes, a.hidden
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(N, H, device=dev, generator=g)
    y = torch.empty_like(x)
    z, h_in, h_out = torch.randn(N, H, device=dev, generator=g), torch.randn(N, H, device=dev, generator=g), torch.empty_like(x)
    stat = torch.ones(4, H, device=dev)
    drop = (0.5, 1234, 0)
    p, st = engine._ptr, engine._stream
    runs = {
        "dropout_out_of_place": lambda: engine.node_dropout(x, drop, 0, out=y),
        "dropout_in_place": lambda: engine.node_dropout(y, drop, 0),
        "node_update_fwd": lambda: engine._call("gnm_node_update_fwd", N, H, p(z), p(stat), p(h_in), p(h_out), st()),
    }
    bytes_of = {"dropout_out_of_place": 2 * N * H * 4, "dropout_in_place": 2 * N * H * 4, "node_update_fwd": 3 * N * H * 4}
    for f in runs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(a.blocks):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.reps)         # microseconds per launch
    res = {}
    for k, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        res[k] = {"us_per_launch_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                  "algorithmic_bytes": bytes_of[k], "tb_per_s_at_median": round(bytes_of[k] / med / 1e6, 3)}
    ref = None
    try:
        for row in csv.DictReader(open(os.path.join(REPO, "profiles", "r06_kernel_stats_serial.csv"))):
            if "node_update_fwd_k<128" in row["Name"]:
                ref = {"kernel": row["Name"].split("(")[0], "us_per_launch_average": round(float(row["AverageNs"]) / 1e3, 2),
                       "tb_per_s": round(3 * 1500000 * 128 * 4 / float(row["AverageNs"]) / 1e3, 3)}
    except OSError:
        pass
    out = {"what": "gnm_node_dropout_apply per launch (device events, back-to-back launches), beside an [N,H] elementwise kernel of the step",
           "nodes": N, "hidden": H, "p": drop[0], "reps_per_block": a.reps, "blocks": a.blocks, "matmul_mode": _lib.get_matmul_mode(),
           "device": torch.cuda.get_device_name(0), "results": res, "r06_kernel_stats_serial": ref,
           "dropout_over_node_update_rate": round(res["dropout_out_of_place"]["tb_per_s_at_median"]
                                                  / res["node_update_fwd"]["tb_per_s_at_median"], 3),
           "gates": "nothing"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
