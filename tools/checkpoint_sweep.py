#!/usr/bin/env python3
"""Step time and peak memory of full-graph training at one (R, H, L, k): k = GraphGatedGCNModel.activation_checkpoint.

    python tools/checkpoint_sweep.py --reads 750000 --hidden 128 --layers 8 --checkpoint 2 [--activations lean]

Builds the synthetic graph of bench.py (synth.make_graph(R): N = 2R nodes, E ~ 10R edges), runs --warmup and then --steps
steps of forward + BCE + backward + Adam exactly as bench.py's step does, and prints ONE JSON line: ms_per_step (wall clock
between two device synchronisations), peak_bytes / peak_gib (torch.cuda.max_memory_allocated over the timed steps: the
graph, its index, the parameters and the optimizer state included) and what was run.  An allocator out-of-memory error is
reported as {"oom": true} with exit status 0; anything else propagates.

One invocation measures one configuration in one process: run it under its own `timeout`, chain invocations with `&&`, and
alternate the configurations you compare (A B A B), not all of one and then all of the other."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, default=750_000, help="R; N = 2R nodes, E ~ 10R edges")
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--checkpoint", type=int, default=0, help="k: layers per recomputed segment (0: keep every layer)")
    ap.add_argument("--activations", default="saved", choices=["saved", "lean"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import dp, engine, synth
    assert torch.cuda.is_available(), "needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    H, L, R = args.hidden, args.layers, args.reads
    src, dst, n = synth.make_graph(R, seed=args.seed)
    inp = synth.make_inputs(src, dst, n, seed=args.seed)
    out = {"reads": R, "hidden": H, "layers": L, "checkpoint": args.checkpoint, "activations": args.activations,
           "nodes": int(n), "edges": int(src.size), "steps": args.steps, "warmup": args.warmup,
           "matmul": G._lib.get_matmul_mode()}
    try:
        g = G.AssemblyGraph(src, dst, n).to(dev)
        g.index()
        e, pe, y = (torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y"))
        crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))
        model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, 0, randomize_norm=False).items()})
        model.to(dev)
        model.activation_checkpoint = args.checkpoint
        model.flatten_parameters()
        flat = dp.FlatGradients(model.parameters(), direct_write=True)
        opt = dp.make_adam(model.parameters(), 1e-3)

        def step():
            flat.zero_()
            loss = crit(model(g, None, e, pe).squeeze(-1), y)
            loss.backward()
            opt.step()
            return loss

        with engine.options(ACTIVATIONS=args.activations):
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        out.update(ms_per_step=round(dt / max(args.steps, 1) * 1e3, 3), peak_bytes=int(peak), peak_gib=round(peak / 2 ** 30, 3),
                   edges_per_s=round(src.size * args.steps / dt), loss=float(loss.detach()))
    except torch.cuda.OutOfMemoryError as err:
        out.update(oom=True, error=str(err).split("\n")[0][:200])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
