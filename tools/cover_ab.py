#!/usr/bin/env python3
"""What the greedy path cover (decode.greedy_cover_contigs: gnm_cover_rounds until a round adds nothing, then gnm_bog_contigs)
costs and gives, next to the best-overlap contigs it extends (decode.best_overlap_contigs).

  scores       two score sets on the graph of --reads reads (E = 7.54 M at 750 000): the logits of the synthetic model, and
               standard normal scores (seed 0).
  rounds       per score set: the rounds to the fixed point and the links every round added.
  round time   device events around ONE gnm_cover_rounds call of one round, for every round r of the sequence in turn (the state
               carries over; a run restarts at round 0), median over --runs runs.  Such a call is four launches: begin, propose,
               link, export; `empty_call` is the same call with zero rounds (begin, export), so round - empty_call is the propose +
               link pair.  `whole` is one call of all rounds; `decision_stats` and `bog_contigs` are timed the same way in the
               same process, --inner back-to-back calls per window.
  decode       decode.greedy_cover_contigs as a whole on the host clock for several check_every, and best_overlap_contigs.
  result       contigs, contigs of at least 20 nodes, their N50, the longest contig and the wrong-link share for both decoders.
  validation   the validation pass of train.train's full-graph loop over --steps copies of the graph (model logits) with
               "assembly_metrics" off, on with "best_overlap" and on with "greedy_cover"; host clock, routes alternating.

One process, one JSON file (--out, default profiles/greedy_cover.json)."""
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
    ap.add_argument("--inner", type=int, default=20, help="decision_stats / bog_contigs: calls per window")
    ap.add_argument("--steps", type=int, default=5, help="validation part: graphs per pass")
    ap.add_argument("--check-every", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "greedy_cover.json"))
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
    idx = g.index()
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, 0, randomize_norm=False).items()})
    model.to(dev).eval()
    with torch.no_grad():
        x_model = model(g, None, e, pe).squeeze(-1).contiguous()
    E = int(x_model.numel())
    score_sets = {"model_logits": x_model, "random_normal": torch.from_numpy(rng.standard_normal(E).astype(np.float32)).to(dev)}
    res = {"what": "greedy path cover by rounds of mutual-best links next to the best-overlap contigs: rounds, links per round, time "
                   "per round and per call, the decode as a whole, the validation pass with the switch off and on; one process",
           "edges": E, "nodes": n, "reads": a.reads, "hidden": H, "layers": L, "device": torch.cuda.get_device_name(0)}

    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)  # noqa: E731
    ls, lp, bs, bp = i32(n), i32(n), i32(n), i32(n)
    ws = torch.empty(engine.cover_workspace_bytes(n), dtype=torch.uint8, device=dev)
    s_d, d_d = g.edges()
    rec = torch.zeros(engine.BOG_RECORD_WORDS, dtype=torch.int64, device=dev)
    out = (i32(n + 1), i32(n), i32(n), torch.empty(n, dtype=torch.int64, device=dev), i32(n))
    st = DecisionStats(dev)

    def timed(fn, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps               # microseconds per call

    def describe(c):
        return {"record": dict(zip(engine.BOG_COUNTERS, c.stats.words())), "contigs_of_20_nodes_or_more": int((c.num_nodes() >= 20).sum()),
                "n50_bases_20": c.n50(20), "longest_bases": c.longest(), "wrong_link_share": c.stats.wrong_link_fraction}

    med = lambda v: float(np.median(v))                      # noqa: E731
    for name, x in score_sets.items():
        cover = decode.greedy_cover_contigs(g, x, pl, rl, y)
        best = decode.best_overlap_contigs(g, x, pl, rl, y)
        F = cover.rounds
        one = torch.zeros(1, dtype=torch.int64, device=dev)
        none = torch.zeros(0, dtype=torch.int64, device=dev)
        allr = torch.zeros(F, dtype=torch.int64, device=dev)
        per_round = [[] for _ in range(F)]
        empty, whole = [], []
        for run in range(a.runs + 1):                        # run 0 warms up
            for r in range(F):
                t = timed(lambda: engine.cover_rounds(idx, x, one, ls, lp, ws, r))
                if run:
                    per_round[r].append(t)
            t = timed(lambda: engine.cover_rounds(idx, x, none, ls, lp, ws, F))
            tw = timed(lambda: engine.cover_rounds(idx, x, allr, ls, lp, ws, 0))
            if run:
                empty.append(t)
                whole.append(tw)
        assert allr.cpu().tolist() == cover.round_links and torch.equal(ls, cover.link_succ) and torch.equal(lp, cover.link_pred)
        routes = {"decision_stats": lambda: st.add(g, x, y, bs, bp),
                  "bog_contigs": lambda: engine.bog_contigs(s_d, d_d, bs, bp, x, y, pl, rl, rec, *out)}
        windows = {k: [] for k in routes}
        for run in range(a.runs + 1):
            for k in (list(routes) if run % 2 == 0 else list(routes)[::-1]):
                t = timed(routes[k], a.inner)
                if run:
                    windows[k].append(t)
        host = {}
        for ce in a.check_every:
            ts = []
            for run in range(a.runs + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                decode.greedy_cover_contigs(g, x, pl, rl, y, check_every=ce)
                ts.append((time.perf_counter() - t0) * 1e3)
            host[str(ce)] = ts[1:]
        tb = []
        for run in range(a.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            decode.best_overlap_contigs(g, x, pl, rl, y)
            tb.append((time.perf_counter() - t0) * 1e3)
        dec_us = med(windows["decision_stats"])
        round_us = [med(v) for v in per_round]
        res[name] = {
            "rounds_to_fixed_point": F, "round_links": cover.round_links, "converged": cover.converged,
            "one_round_call_us_by_round": per_round, "empty_call_us": empty, "whole_call_us": whole, "windows_us_per_call": windows,
            "greedy_cover_contigs_ms_host_clock_by_check_every": host, "best_overlap_contigs_ms_host_clock": tb[1:],
            "greedy_cover": describe(cover), "best_overlap": describe(best),
            "summary": {"median_one_round_call_us": round_us, "median_empty_call_us": med(empty),
                        "median_round_pair_us": [t - med(empty) for t in round_us], "median_whole_call_us": med(whole),
                        "median_decision_stats_us": dec_us, "median_bog_contigs_us": med(windows["bog_contigs"]),
                        "first_round_pair_over_decision_launch": (round_us[0] - med(empty)) / dec_us,
                        "greedy_cover_contigs_ms_median_by_check_every": {k: med(v) for k, v in host.items()},
                        "best_overlap_contigs_ms_median": med(tb[1:])},
            "note": "device events around calls on one stream; a one-round call is begin + propose + link + export, the empty call "
                    "begin + export; the whole-decode figures are the host clock (allocations, every chunk's read-back, gnm_bog_contigs)"}

    # ---- the validation pass ---------------------------------------------------------------------------------------------------------
    crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))
    asm = {"best_overlap": AssemblyStats(dev), "greedy_cover": AssemblyStats(dev, decoder="greedy_cover")}

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

    modes = ("off", "best_overlap", "greedy_cover")
    for m in modes:
        one_pass(m)
    passes, totals, entries = {m: [] for m in modes}, {}, {}
    for k in range(a.runs):
        for m in (modes if k % 2 == 0 else modes[::-1]):
            ms, entries[m], totals[m] = one_pass(m)
            passes[m].append(ms)
    assert totals["off"] == totals["best_overlap"] == totals["greedy_cover"], "the switch changed the loss or the counts"
    vmed = {m: med(v) for m, v in passes.items()}
    res["validation"] = {"steps_per_pass": a.steps, "ms_per_graph_by_pass": passes,
                         "assembly_valid_entry": {m: list(entries[m]) for m in modes[1:]},
                         "summary": {"median_ms_per_graph": vmed, "best_overlap_minus_off_ms": vmed["best_overlap"] - vmed["off"],
                                     "greedy_cover_minus_off_ms": vmed["greedy_cover"] - vmed["off"],
                                     "spread_off_ms": float(np.max(passes["off"]) - np.min(passes["off"]))},
                         "note": "host clock around a pass of steps_per_pass forwards + loss + counts (+ add) ending in a device synchronise"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k]["summary"] for k in list(score_sets) + ["validation"]}))


if __name__ == "__main__":
    main()
