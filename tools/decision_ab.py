#!/usr/bin/env python3
"""What the walk-decision metrics (train.DecisionStats: gnm_decision_stats, per node the top-scored out-edge and in-edge) cost.

  kernel       gnm_decision_stats alone (both tables and the record) on the logits of the synthetic model on the graph of --reads
               reads (E = 7.54 M at 750 000), against a torch restatement on the same device: per direction scatter_reduce amax of
               the scores by node, the edges that attain it, scatter_reduce amin of their ids (the tie rule), a bincount for the
               candidate counts, a scatter_reduce amax of the labels, and the sums of the seven counters (self loops masked; NaN
               scores are not handled on that side -- the model's logits hold none).  The two routes must give the same tables and
               counters.  Device events around --inner back-to-back calls, routes alternating, median over --runs windows.
  validation   the validation pass of train.train's full-graph loop (eval mode, no_grad, torch route of the loss and the counts:
               the parent's code path) over --steps copies of the graph, with "decision_metrics" off and on (on: one
               DecisionStats.add per forward, one read per pass).  Host clock around a pass that ends in a device synchronise,
               routes alternating pass by pass.

One process, one JSON file (--out, default profiles/decision_metrics.json)."""
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
    ap.add_argument("--runs", type=int, default=5, help="timed windows (kernel) or passes (validation) per route, after a warm-up of each")
    ap.add_argument("--inner", type=int, default=50, help="kernel part: gnm_decision_stats calls per window (the torch route takes a tenth)")
    ap.add_argument("--steps", type=int, default=10, help="validation part: graphs per pass")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decision_metrics.json"))
    a = ap.parse_args()

    import torch
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    from gnnome_assembly_amd.train import DECISION_COUNTERS, DecisionStats, tfpn_counts
    assert torch.cuda.is_available(), "needs a GPU: this tool measures, it has no CPU mode"
    dev = torch.device("cuda:0")
    H, L = a.hidden, a.layers
    src, dst, n = synth.make_graph(a.reads, seed=0)
    inp = synth.make_inputs(src, dst, n, seed=0)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    e, pe, y = (torch.from_numpy(inp[k]).to(dev) for k in ("e", "pe", "y"))
    g.index()
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, 0, randomize_norm=False).items()})
    model.to(dev).eval()
    with torch.no_grad():
        x = model(g, None, e, pe).squeeze(-1).contiguous()
    E = int(x.numel())
    assert not bool(torch.isnan(x).any())
    st = DecisionStats(dev)
    best = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    res = {"what": "walk-decision metrics: (a) gnm_decision_stats against a torch restatement (scatter_reduce amax + tie handling) on "
                   "the same device, (b) the full-graph validation pass with decision_metrics off (the parent's code path) and on; one "
                   "process, routes alternating", "edges": E, "nodes": n, "reads": a.reads, "hidden": H, "layers": L,
           "device": torch.cuda.get_device_name(0), "relabelled": bool(g.relabel_info.get("relabelled"))}

    # ---- (a) the launch against torch ----------------------------------------------------------------------------------------------
    ends = [t.long() for t in g.edges()]                 # int64 once, outside the timed region (in torch's favour)
    eid = torch.arange(E, device=dev)
    keep = ends[0] != ends[1]
    pos = y == 1

    def kernel_route():
        st.add(g, x, y, best[0], best[1])

    def torch_route():
        s = torch.where(keep, x, torch.full_like(x, float("-inf")))
        tables, counters = [], []
        for v in ends:
            top = torch.full((n,), float("-inf"), device=dev).scatter_reduce(0, v, s, "amax")
            hit = keep & (s == top[v])
            b = torch.full((n,), E, dtype=torch.int64, device=dev).scatter_reduce(0, v[hit], eid[hit], "amin")
            cnt = torch.bincount(v[keep], minlength=n)
            anyp = torch.zeros(n, device=dev).scatter_reduce(0, v[keep], y[keep], "amax") == 1      # labels are 0 / 1 here
            ok = pos[b.clamp(max=E - 1)] & (cnt > 0)
            one, many = cnt == 1, cnt > 1
            counters.append(torch.stack([(cnt == 0).sum(), one.sum(), (one & ok).sum(), many.sum(), (many & anyp).sum(),
                                         (many & ok).sum(), torch.zeros((), dtype=torch.int64, device=dev)]))
            tables.append(torch.where(cnt > 0, b, torch.full_like(b, -1)))
        return tables, torch.cat(counters)

    routes = {"decision_stats": (kernel_route, a.inner), "torch_scatter": (torch_route, max(a.inner // 10, 1))}

    def window(name):
        fn, k = routes[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / k            # microseconds per call

    st.zero_()
    kernel_route()
    t_tables, t_counters = torch_route()
    one_call = st.buf.cpu().numpy()
    assert np.array_equal(one_call[:-1], t_counters.cpu().numpy()), "the two routes count differently"
    assert all(torch.equal(best[d].long(), t_tables[d]) for d in (0, 1)), "the two routes choose differently"
    for r in routes:
        window(r)                                       # warm-up: code objects, the caching allocator
    st.zero_()
    windows = {r: [] for r in routes}
    names = list(routes)
    for k in range(a.runs):
        for r in (names if k % 2 == 0 else names[::-1]):
            windows[r].append(window(r))
    m = st.read()
    assert m.calls == a.runs * a.inner and m.pooled.dead + m.pooled.forced + m.pooled.branch == 2 * n * m.calls, "the record lost nodes"
    med = {r: float(np.median(v)) for r, v in windows.items()}
    res["kernel"] = {"windows_us_per_call": windows, "calls_per_window": {r: k for r, (_, k) in routes.items()},
                     "record_of_one_call": dict(succ=dict(zip(DECISION_COUNTERS, one_call[:7].tolist())),
                                                pred=dict(zip(DECISION_COUNTERS, one_call[7:14].tolist()))),
                     "summary": {"median_us_per_call": med, "kernel_over_torch": med["decision_stats"] / med["torch_scatter"]},
                     "note": "device events around back-to-back calls on one stream; both routes produce both tables and the 14 counters"}

    # ---- (b) the validation pass ----------------------------------------------------------------------------------------------------
    crit = G.BCEWithLogitsLoss(float(inp["pos_weight"]))

    def one_pass(on):
        vloss = torch.zeros((), device=dev, dtype=torch.float64)
        vcounts = torch.zeros(4, device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if on:
            st.zero_()
        with torch.no_grad():
            for _ in range(a.steps):
                pred = model(g, None, e, pe).squeeze(-1)
                vloss += crit(pred, y).double()
                vcounts += tfpn_counts(pred, y)
                if on:
                    st.add(g, pred, y)
        out = st.read() if on else None
        total = float(vloss), vcounts.tolist()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps, out, total

    modes = ("off", "on")
    for r in modes:
        one_pass(r == "on")
    passes = {r: [] for r in modes}
    totals, dm = {}, None
    for k in range(a.runs):
        for r in (modes if k % 2 == 0 else modes[::-1]):
            ms, got, totals[r] = one_pass(r == "on")
            passes[r].append(ms)
            dm = got if got is not None else dm
    assert totals["off"] == totals["on"], "the switch changed the loss or the counts"
    vmed = {r: float(np.median(v)) for r, v in passes.items()}
    res["validation"] = {"steps_per_pass": a.steps, "ms_per_graph_by_pass": passes, "decision_valid_entry": list(dm.summary()),
                         "summary": {"median_ms_per_graph": vmed, "on_minus_off_ms": vmed["on"] - vmed["off"],
                                     "on_over_off": vmed["on"] / vmed["off"],
                                     "spread_off_ms": float(np.max(passes["off"]) - np.min(passes["off"])),
                                     "kernel_us_over_forward_ms_percent": med["decision_stats"] / 1e3 / vmed["off"] * 100.0},
                         "note": "host clock around a pass of steps_per_pass forwards + loss + counts (+ add; + one read per pass) ending "
                                 "in a device synchronise; off is the loop without the switch"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"kernel": res["kernel"]["summary"], "validation": res["validation"]["summary"]}))


if __name__ == "__main__":
    main()
