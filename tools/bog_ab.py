#!/usr/bin/env python3
"""What the best-overlap contigs (decode.best_overlap_contigs: gnm_decision_stats for the tables, then gnm_bog_contigs) cost.

  call         on the logits of the synthetic model on the graph of --reads reads (E = 7.54 M at 750 000): the decision launch
               alone (tables and record), the composite gnm_bog_contigs call alone (2 ceil(log2 n) + 6 launches: link, the two
               pointer-jumping passes, scans, layout), both from device events around --inner back-to-back calls, median over
               --runs windows; and decode.best_overlap_contigs as a whole on the host clock (allocations, both calls, the read of
               the record).  The split of the composite call into its passes needs a kernel trace and is not taken here.
  validation   the validation pass of train.train's full-graph loop (eval mode, no_grad, torch route of the loss and the counts)
               over --steps copies of the graph, with "assembly_metrics" off and on (on: one AssemblyStats.add per forward).
               Host clock around a pass that ends in a device synchronise, routes alternating pass by pass; the spread of the
               off passes is recorded beside the medians.
  decode       for orientation only, the `device_default` figure of profiles/decode_timing.json (the sampled greedy decode) when
               that file is there: another algorithm with another result, recorded, not compared as a speed-up.

One process, one JSON file (--out, default profiles/bog_contigs.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def orientation() -> dict:
    """The `device_default` entries of profiles/decode_timing.json (the sampled greedy decode), when that file is there."""
    ref = os.path.join(REPO, "profiles", "decode_timing.json")
    if not os.path.exists(ref):
        return {}
    found = []

    def walk(o):
        if isinstance(o, dict):
            if o.get("path") == "device_default":
                found.append({k: v for k, v in o.items() if not isinstance(v, (list, dict))})
            for v in o.values():
                walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)

    with open(ref) as f:
        walk(json.load(f))
    return {"sampled_decode_for_orientation": {"device_default": found,
                                               "note": "another algorithm with another result: recorded, not compared"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5, help="timed windows (call) or passes (validation) per route, after a warm-up of each")
    ap.add_argument("--inner", type=int, default=20, help="call part: calls per window")
    ap.add_argument("--steps", type=int, default=10, help="validation part: graphs per pass")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bog_contigs.json"))
    a = ap.parse_args()

    import torch
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import decode, engine, synth
    from gnnome_assembly_amd.train import AssemblyStats, DecisionStats, tfpn_counts
    assert torch.cuda.is_available(), "needs a GPU: this tool measures, it has no CPU mode"
    dev = torch.device("cuda:0")
    H, L = a.hidden, a.layers
    src, dst, n = synth.make_graph(a.reads, seed=0)
    inp = synth.make_inputs(src, dst, n, seed=0)
    rng = np.random.default_rng(0)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    e, pe, y = (torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y"))
    pl = torch.from_numpy(rng.integers(500, 12000, src.size)).to(dev)
    rl = torch.from_numpy(rng.integers(8000, 25000, n)).to(dev)
    g.edata["prefix_length"], g.ndata["read_length"] = pl, rl
    g.index()
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, 0, randomize_norm=False).items()})
    model.to(dev).eval()
    with torch.no_grad():
        x = model(g, None, e, pe).squeeze(-1).contiguous()
    E = int(x.numel())
    res = {"what": "best-overlap contigs: (a) the decision launch, the composite gnm_bog_contigs call and decode.best_overlap_contigs "
                   "as a whole, (b) the full-graph validation pass with assembly_metrics off and on; one process, routes alternating",
           "edges": E, "nodes": n, "reads": a.reads, "hidden": H, "layers": L, "device": torch.cuda.get_device_name(0),
           "rounds_per_pass": int(np.ceil(np.log2(max(n, 2)))), "launches": 2 * int(np.ceil(np.log2(max(n, 2)))) + 6}

    # ---- (a) one call ------------------------------------------------------------------------------------------------------------------
    st = DecisionStats(dev)
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)  # noqa: E731
    bs, bp = i32(n), i32(n)
    s_d, d_d = g.edges()
    rec = torch.zeros(engine.BOG_RECORD_WORDS, dtype=torch.int64, device=dev)
    out = (i32(n + 1), i32(n), i32(n), torch.empty(n, dtype=torch.int64, device=dev), i32(n))
    routes = {"decision_stats": lambda: st.add(g, x, y, bs, bp),
              "bog_contigs": lambda: engine.bog_contigs(s_d, d_d, bs, bp, x, y, pl, rl, rec, *out)}

    def window(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            routes[name]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.inner            # microseconds per call

    for r in routes:
        routes[r]()
        window(r)                                            # warm-up: code objects, the caching allocator
    rec.zero_()
    windows = {r: [] for r in routes}
    names = list(routes)
    for k in range(a.runs):
        for r in (names if k % 2 == 0 else names[::-1]):
            windows[r].append(window(r))
    calls = int(rec[-1])
    assert calls == a.runs * a.inner and int(rec[0]) % calls == 0, "the record is not a multiple of one call's"
    whole = []
    for _ in range(a.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = decode.best_overlap_contigs(g, x, pl, rl, y)
        whole.append((time.perf_counter() - t0) * 1e3)
    med = {r: float(np.median(v)) for r, v in windows.items()}
    res["call"] = {"windows_us_per_call": windows, "calls_per_window": a.inner, "best_overlap_contigs_ms_host_clock": whole[1:],
                   "record_of_one_call": dict(zip(engine.BOG_COUNTERS, c.stats.words())),
                   "contigs_of_20_nodes_or_more": int((c.num_nodes() >= 20).sum()), "n50_bases_20": c.n50(20), "longest_bases": c.longest(),
                   "summary": {"median_us_per_call": med, "spread_us": {r: float(np.max(v) - np.min(v)) for r, v in windows.items()},
                               "best_overlap_contigs_ms_median": float(np.median(whole[1:]))},
                   "note": "device events around back-to-back calls on one stream; the whole-call figure is the host clock around "
                           "decode.best_overlap_contigs (allocations, the decision launch, gnm_bog_contigs, the read of the record)"}

    # ---- (b) the validation pass ----------------------------------------------------------------------------------------------------
    crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))
    asm = AssemblyStats(dev)

    def one_pass(on):
        vloss = torch.zeros((), device=dev, dtype=torch.float64)
        vcounts = torch.zeros(4, device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if on:
            asm.zero_()
        with torch.no_grad():
            for _ in range(a.steps):
                pred = model(g, None, e, pe).squeeze(-1)
                vloss += crit(pred, y).double()
                vcounts += tfpn_counts(pred, y)
                if on:
                    asm.add(g, pred, y)
        entry = asm.summary() if on else None
        total = float(vloss), vcounts.tolist()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps, entry, total

    modes = ("off", "on")
    for r in modes:
        one_pass(r == "on")
    passes = {r: [] for r in modes}
    totals, entry = {}, None
    for k in range(a.runs):
        for r in (modes if k % 2 == 0 else modes[::-1]):
            ms, got, totals[r] = one_pass(r == "on")
            passes[r].append(ms)
            entry = got if got is not None else entry
    assert totals["off"] == totals["on"], "the switch changed the loss or the counts"
    vmed = {r: float(np.median(v)) for r, v in passes.items()}
    res["validation"] = {"steps_per_pass": a.steps, "ms_per_graph_by_pass": passes, "assembly_valid_entry": list(entry),
                         "summary": {"median_ms_per_graph": vmed, "on_minus_off_ms": vmed["on"] - vmed["off"],
                                     "on_over_off": vmed["on"] / vmed["off"],
                                     "spread_off_ms": float(np.max(passes["off"]) - np.min(passes["off"])),
                                     "spread_on_ms": float(np.max(passes["on"]) - np.min(passes["on"]))},
                         "note": "host clock around a pass of steps_per_pass forwards + loss + counts (+ add, which reads the record "
                                 "and the kept lengths once per graph) ending in a device synchronise; off is the loop without the switch"}
    res.update(orientation())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"call": res["call"]["summary"], "validation": res["validation"]["summary"]}))


if __name__ == "__main__":
    main()
