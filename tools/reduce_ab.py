#!/usr/bin/env python3
"""What the transitive reduction ahead of the cover decoders (decode.transitive_support: gnm_transitive_support, one launch) costs
and gives, on the graph of --reads reads (E = 7.54 M at 750 000).

  prefixes     taken from synthetic read positions (read i starts at a random increasing position; an edge's prefix is the distance
               between its two reads' starts, cut at the source read's length for the few long-range edges), so that the triangles
               of true overlaps are length-consistent and --fuzz 0 reduces them.
  scores       the logits of the synthetic model, and standard normal scores (seed 0).
  launch       device events around --inner back-to-back calls of engine.transitive_support and of engine.decision_stats (DecisionStats.add),
               routes alternating, median over --runs windows: the reduction launch beside the decision launch, in one process.
  reduction    the record (reduced share, max support, witnesses) per score set, and the out-degree histogram of the graph with the
               sum of d^2 the kernel's row walks amount to.
  cover        decode.greedy_cover_contigs without and with reduce_transitive: rounds, links, contigs of at least 20 nodes, their N50,
               the longest contig and the summed bases of those contigs; host clock of the whole decode, routes alternating.
  validation   the validation pass of train.train's full-graph loop over --steps copies of the graph (model logits) with
               "assembly_metrics" off, on with AssemblyStats(decoder="greedy_cover") called as before the switch existed, on with
               reduce_transitive=False given explicitly, and on with reduce_transitive=True; host clock, routes alternating.

One process, one JSON file (--out, default profiles/transitive_reduce.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5, help="timed runs per figure, after a warm-up of each")
    ap.add_argument("--inner", type=int, default=20, help="launch figures: calls per window")
    ap.add_argument("--steps", type=int, default=3, help="validation part: graphs per pass")
    ap.add_argument("--fuzz", type=int, default=0, help="the length tolerance of the reduction; -1: none")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "transitive_reduce.json"))
    a = ap.parse_args()
    fuzz = None if a.fuzz < 0 else a.fuzz

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
    start = np.cumsum(rng.integers(500, 3000, a.reads)).astype(np.int64)
    rl_h = np.repeat(rng.integers(20000, 30000, a.reads), 2).astype(np.int64)
    pl_h = np.minimum(np.abs(start[dst >> 1] - start[src >> 1]), rl_h[src])
    g = G.AssemblyGraph(src, dst, n).to(dev)
    e, pe, y = (torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y"))
    pl, rl = torch.from_numpy(pl_h).to(dev), torch.from_numpy(rl_h).to(dev)
    g.edata["prefix_length"], g.ndata["read_length"] = pl, rl
    idx = g.index()
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, 0, randomize_norm=False).items()})
    model.to(dev).eval()
    with torch.no_grad():
        x_model = model(g, None, e, pe).squeeze(-1).contiguous()
    E = int(x_model.numel())
    score_sets = {"model_logits": x_model, "random_normal": torch.from_numpy(rng.standard_normal(E).astype(np.float32)).to(dev)}
    deg = np.bincount(src, minlength=n)
    hist = np.bincount(deg)
    res = {"what": "transitive reduction of the candidate edges ahead of the greedy path cover: the launch beside the decision launch, "
                   "what it removes, the cover without and with it, the validation pass with the switch off and on; one process",
           "edges": E, "nodes": n, "reads": a.reads, "hidden": H, "layers": L, "fuzz": fuzz, "device": torch.cuda.get_device_name(0),
           "out_degree": {"histogram": {str(d): int(c) for d, c in enumerate(hist) if c}, "max": int(deg.max()), "mean": float(deg.mean()),
                          "sum_d_squared": int((deg.astype(np.int64) ** 2).sum()),
                          "share_of_d_squared_in_rows_longer_than_16": float((deg[deg > 16].astype(np.int64) ** 2).sum() / max(1, (deg.astype(np.int64) ** 2).sum()))}}

    def timed(fn, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps               # microseconds per call

    def describe(c):
        keep = c.num_nodes() >= 20
        out = {"record": dict(zip(engine.BOG_COUNTERS, c.stats.words())), "rounds": c.rounds, "links": c.stats.links,
               "contigs_of_20_nodes_or_more": int(keep.sum()), "n50_bases_20": c.n50(20), "longest_bases": c.longest(),
               "longest_nodes": int(c.num_nodes().max()), "summed_bases_20": int(c.bases[keep].sum()),
               "wrong_link_share": c.stats.wrong_link_fraction}
        if hasattr(c, "reduce_stats"):
            out["reduce_record"] = dict(zip(engine.REDUCE_COUNTERS, c.reduce_stats.words()))
        return out

    med = lambda v: float(np.median(v))                      # noqa: E731
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)  # noqa: E731
    bs, bp, support = i32(n), i32(n), i32(E)
    masked = torch.empty(E, dtype=torch.float32, device=dev)
    rec = torch.zeros(engine.REDUCE_RECORD_WORDS, dtype=torch.int64, device=dev)
    st = DecisionStats(dev)
    for name, x in score_sets.items():
        routes = {"transitive_support": lambda: engine.transitive_support(idx, x, pl, y, float("-inf"), fuzz, support, masked, rec),
                  "transitive_support_no_fuzz": lambda: engine.transitive_support(idx, x, pl, y, float("-inf"), None, support, masked, rec),
                  "decision_stats": lambda: st.add(g, x, y, bs, bp)}
        windows = {k: [] for k in routes}
        for run in range(a.runs + 1):                        # run 0 warms up
            for k in (list(routes) if run % 2 == 0 else list(routes)[::-1]):
                t = timed(routes[k], a.inner)
                if run:
                    windows[k].append(t)
        red = decode.transitive_support(g, x, pl, y, fuzz=fuzz)
        covers = {"plain": lambda: decode.greedy_cover_contigs(g, x, pl, rl, y),
                  "reduced": lambda: decode.greedy_cover_contigs(g, x, pl, rl, y, reduce_transitive=True, fuzz=fuzz)}
        host, last = {k: [] for k in covers}, {}
        for run in range(a.runs + 1):
            for k in (list(covers) if run % 2 == 0 else list(covers)[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[k] = covers[k]()
                if run:
                    host[k].append((time.perf_counter() - t0) * 1e3)
        dp, dr = describe(last["plain"]), describe(last["reduced"])
        tus, dus = med(windows["transitive_support"]), med(windows["decision_stats"])
        res[name] = {
            "windows_us_per_call": windows, "reduce_record": dict(zip(engine.REDUCE_COUNTERS, red.stats.words())),
            "reduced_share_of_candidates": red.stats.reduced_fraction,
            "support_histogram": {str(d): int(c) for d, c in enumerate(torch.bincount(red.support.long()).cpu().tolist()) if c},
            "greedy_cover_contigs_ms_host_clock": host, "greedy_cover": dp, "greedy_cover_reduced": dr,
            "summary": {"median_transitive_support_us": tus, "median_transitive_support_no_fuzz_us": med(windows["transitive_support_no_fuzz"]),
                        "median_decision_stats_us": dus, "reduction_over_decision_launch": tus / dus,
                        "greedy_cover_contigs_ms_median": {k: med(v) for k, v in host.items()},
                        "reduced_share_of_candidates": red.stats.reduced_fraction, "max_support": red.stats.max_support,
                        "contigs_20": [dp["contigs_of_20_nodes_or_more"], dr["contigs_of_20_nodes_or_more"]],
                        "n50_bases_20": [dp["n50_bases_20"], dr["n50_bases_20"]],
                        "summed_bases_20": [dp["summed_bases_20"], dr["summed_bases_20"]],
                        "longest_nodes": [dp["longest_nodes"], dr["longest_nodes"]]},
            "note": "device events around calls on one stream for the launches; the whole-decode figures are the host clock "
                    "(allocations, every chunk's read-back, gnm_bog_contigs); lists of two are [plain, reduced]"}

    # ---- the validation pass ---------------------------------------------------------------------------------------------------------
    crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))
    asm = {"greedy_cover_as_before": AssemblyStats(dev, decoder="greedy_cover"),
           "greedy_cover_switch_off": AssemblyStats(dev, decoder="greedy_cover", reduce_transitive=False, fuzz=None),
           "greedy_cover_reduced": AssemblyStats(dev, decoder="greedy_cover", reduce_transitive=True, fuzz=fuzz)}

    def one_pass(mode):
        vloss = torch.zeros((), device=dev, dtype=torch.float64)
        vcounts = torch.zeros(4, device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode != "off":
            asm[mode].zero_()
        with torch.no_grad():
            for _ in range(a.steps):
                pred = model(g, None, e, pe).squeeze(-1)
                vloss += crit(pred, y).double()
                vcounts += tfpn_counts(pred, y)
                if mode != "off":
                    asm[mode].add(g, pred, y)
        entry = asm[mode].summary() if mode != "off" else None
        total = float(vloss), vcounts.tolist()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps, entry, total

    modes = ("off",) + tuple(asm)
    for m in modes:
        one_pass(m)
    passes, totals, entries = {m: [] for m in modes}, {}, {}
    for k in range(a.runs):
        for m in (modes if k % 2 == 0 else modes[::-1]):
            ms, entries[m], totals[m] = one_pass(m)
            passes[m].append(ms)
    assert len({json.dumps(totals[m]) for m in modes}) == 1, "the switch changed the loss or the counts"
    assert entries["greedy_cover_as_before"] == entries["greedy_cover_switch_off"], "the switch, off, changed the contigs"
    vmed = {m: med(v) for m, v in passes.items()}
    res["validation"] = {"steps_per_pass": a.steps, "ms_per_graph_by_pass": passes,
                         "assembly_valid_entry": {m: list(entries[m]) for m in modes[1:]},
                         "summary": {"median_ms_per_graph": vmed,
                                     "switch_off_minus_as_before_ms": vmed["greedy_cover_switch_off"] - vmed["greedy_cover_as_before"],
                                     "reduced_minus_as_before_ms": vmed["greedy_cover_reduced"] - vmed["greedy_cover_as_before"],
                                     "spread_as_before_ms": float(np.max(passes["greedy_cover_as_before"]) - np.min(passes["greedy_cover_as_before"]))},
                         "note": "host clock around a pass of steps_per_pass forwards + loss + counts (+ add) ending in a device synchronise"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k]["summary"] for k in list(score_sets) + ["validation"]}))


if __name__ == "__main__":
    main()
