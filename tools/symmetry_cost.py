"""What the symmetry loss costs, recorded and not gated (profiles/symmetry_loss.json).

  step      the full-graph training step (forward, loss, backward into a direct-write dp.FlatGradients; no optimizer) at the
            metric's graph (bench.py: R = 750,000 reads, H = 128, L = 8) -- or the largest of --reads that fits: the "joint" schedule
            keeps two activation sets -- with the symmetry loss off, "joint" and "sequential": wall time per step over `steps`
            steps after `warmup`, the three alternating round by round in one process, and the peak device memory of each.
  kernel    gnm_sym_bce_fwd_bwd alone against the torch expression (BCEWithLogits twice, |o - r|, mean, autograd backward) at
            the same E: device events around `reps` back-to-back runs.

    python tools/symmetry_cost.py OUT.json [--reads 750000 375000 100000] [--steps 5] [--warmup 2] [--rounds 3] [--reps 20]"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gnnome_assembly_amd as G  # noqa: E402
from gnnome_assembly_amd import _lib, dp, models, synth, train as T  # noqa: E402


def _stats(t):
    t = sorted(t)
    return {"median": round(t[len(t) // 2], 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def _setup(reads, H, L, dev):
    src, dst, n = synth.make_graph(reads, seed=0)
    inp = synth.make_inputs(src, dst, n, seed=0)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    e, pe, y = (torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y"))
    torch.manual_seed(0)
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16).to(dev)
    models.flatten_parameters(model)
    flat = dp.FlatGradients(model.parameters(), direct_write=True)
    return model, flat, g, e, pe, y, float(inp["pos_weight"])


def step_cost(a, reads):
    dev = torch.device("cuda:0")
    model, flat, g, e, pe, y, pw = _setup(reads, a.hidden, a.layers, dev)
    plain, sym = G.BCEWithLogitsLoss(pw), G.SymmetryLoss(pw, a.alpha)

    def off():
        plain(model(g, None, e, pe).squeeze(-1), y).backward()
    runs = {"off": off,
            "joint": lambda: T.symmetry_step(model, sym, g, None, e, pe, y, "joint"),
            "sequential": lambda: T.symmetry_step(model, sym, g, None, e, pe, y, "sequential")}
    times, peak = {k: [] for k in runs}, {}
    for rnd in range(a.rounds):
        for k, f in runs.items():
            for _ in range(a.warmup if rnd == 0 else 1):
                flat.zero_()
                f()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                flat.zero_()
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            peak[k] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)
    out = {"reads": reads, "edges": g.num_edges(), "hidden": a.hidden, "layers": a.layers, "steps": a.steps, "rounds": a.rounds,
           "ms_per_step": {k: _stats(v) for k, v in times.items()}, "peak_mem_gib": peak,
           "sym_gap": float(sym.last_parts[2])}
    off_ms = out["ms_per_step"]["off"]["median"]
    out["ratio_to_off"] = {k: round(out["ms_per_step"][k]["median"] / off_ms, 3) for k in ("joint", "sequential")}
    return out, (g.num_edges(), y, pw)


def kernel_cost(a, E, y, pw):
    dev = y.device
    o = torch.randn(E, device=dev) * 4
    r = o + torch.randn(E, device=dev) * 0.3
    sym = G.SymmetryLoss(pw, a.alpha)
    bce = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw], device=dev))

    def lib():
        a_, b_ = o.requires_grad_(True), r.requires_grad_(True)
        a_.grad = b_.grad = None
        sym(a_, b_, y).backward()

    def torch_expr():
        a_, b_ = o.requires_grad_(True), r.requires_grad_(True)
        a_.grad = b_.grad = None
        (bce(a_, y) + bce(b_, y) + a.alpha * (a_ - b_).abs().mean()).backward()
    times = {}
    for name, f in (("library", lib), ("torch", torch_expr)):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / a.reps)
        times[name] = _stats(ts)
    return {"edges": E, "reps": a.reps, "ms_per_loss_fwd_bwd": times, "note": "host launch overhead and the autograd wrappers included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reads", type=int, nargs="+", default=[750000, 375000, 100000])
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "csrc_sha": _lib.csrc_sha(), "matmul": _lib.get_matmul_mode(), "skipped": []}
    for reads in a.reads:
        try:
            res["step"], (E, y, pw) = step_cost(a, reads)
            break
        except torch.cuda.OutOfMemoryError as ex:          # two activation sets do not fit: the next size down
            res["skipped"].append({"reads": reads, "reason": str(ex).split("\n")[0]})
            torch.cuda.empty_cache()
    else:
        raise SystemExit("symmetry_cost: none of --reads fits on this device")
    res["kernel"] = kernel_cost(a, E, y, pw)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
