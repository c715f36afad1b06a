#!/usr/bin/env python3
"""What keeping one strand per read costs on the host (decode.resolve_strands, including the BogContigs.host() copy it starts
with) and on the device (decode.resolve_strands_device: gnm_resolve_prepare / _rounds / _layout), on the greedy cover of the
synthetic graph of --reads reads (1.5 M nodes / 7.54 M edges at 750 000) under fixed-seed standard normal logits.

  resolve      per --len-threshold: both routes on the host clock (a fresh BogContigs per host run, so that host() copies), the
               device route also between device events; the results are compared for equality first.  rounds, kept pieces,
               serially cut contigs from the device record.
  infer        decode.infer_contigs(decoder="greedy_cover", reads=store) with device_resolve False and True on the host clock; the
               "model" returns the fixed logits, so the figure is the decode, the strand rule and the sequences.
  serial       a small cover of --serial-contigs contigs of --serial-nodes nodes that each visit one read twice (cut by one lane),
               next to the same cover without the second visit (cut by the wave).

Timing: the routes of a part take turns, window by window, and the turn order flips from run to run; a window of a device route
is --inner (--infer-inner) back-to-back calls, so that it holds tens of milliseconds of work and more; medians over --runs windows
after one warm-up call of each route.

One process, one JSON file (--out, default profiles/resolve_strands.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--min-len", type=int, default=2000)
    ap.add_argument("--max-len", type=int, default=6000)
    ap.add_argument("--runs", type=int, default=7, help="timed windows per route, after a warm-up call of each; the routes alternate")
    ap.add_argument("--inner", type=int, default=50, help="resolve_strands_device: back-to-back calls per timed window")
    ap.add_argument("--infer-inner", type=int, default=5,
                    help="infer_contigs(device_resolve=True) and the host rule on the small covers: calls per timed window")
    ap.add_argument("--len-threshold", type=int, nargs="+", default=[20, 2])
    ap.add_argument("--serial-contigs", type=int, default=64)
    ap.add_argument("--serial-nodes", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resolve_strands.json"))
    a = ap.parse_args()

    import torch
    from gnnome_assembly_amd import decode, engine
    from seq_ab import build
    assert torch.cuda.is_available(), "needs a GPU: this tool measures, it has no CPU mode"
    dev = torch.device("cuda:0")
    g, _, store, pl = build(a.reads, a.min_len, a.max_len, 0, dev)
    rl = g.ndata["read_length"]
    n, E = g.num_nodes(), g.num_edges()
    scores = torch.randn(E, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    med = lambda v: float(np.median(v))                      # noqa: E731
    spread = lambda v: [float(np.min(v)), float(np.max(v))]  # noqa: E731

    def window(fn, reps):
        """`reps` back-to-back calls: (ms per call on the host clock, ms per call between device events, the last result)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps, e0.elapsed_time(e1) / reps, out

    def alternate(routes):
        """routes: name -> (fn, calls per window).  One warm-up call of each, then --runs windows of each: the routes take turns
        within a run and the turn order flips from run to run.  name -> (host-clock ms per call by window, device-event ms per call
        by window, the last result)."""
        for fn, _ in routes.values():
            window(fn, 1)
        host, events, last = ({k: [] for k in routes} for _ in range(3))
        for run in range(a.runs):
            for k in (list(routes) if run % 2 == 0 else list(routes)[::-1]):
                h, d, last[k] = window(*routes[k])
                host[k].append(h)
                events[k].append(d)
        return {k: (host[k], events[k], last[k]) for k in routes}

    def fresh(c):                                            # the same cover with no host copy yet
        return decode.BogContigs(c.contig_ptr, c.walk_nodes, c.walk_edges, c.bases, c.wrong, c.stats, c.prefix_length, c.read_length)

    cover = decode.greedy_cover_contigs(g, scores, pl, rl)
    res = {"what": "one strand per read on the greedy cover of fixed-seed standard normal logits: decode.resolve_strands (host, with "
                   "the host() copy) next to decode.resolve_strands_device; infer_contigs with reads= on both routes; the serial "
                   "fallback on a small cover; one process, the routes alternating window by window, a window of a device route "
                   "being `inner` (`infer_inner`) back-to-back calls; ms per call, medians over `runs` windows",
           "edges": E, "nodes": n, "reads": a.reads, "contigs": len(cover), "cover_rounds": cover.rounds,
           "device": torch.cuda.get_device_name(0), "runs": a.runs, "inner": a.inner, "infer_inner": a.infer_inner,
           "resolve": {}, "infer_contigs": {}}
    for thr in a.len_threshold:
        want = decode.resolve_strands(fresh(cover), thr)
        got = decode.resolve_strands_device(cover, thr)
        r = got.resolved()
        assert r.walks == want.walks and r.bases == want.bases, "the device route differs from the host route"
        t = alternate({"host": (lambda: decode.resolve_strands(fresh(cover), thr), 1),
                       "device": (lambda: decode.resolve_strands_device(cover, thr), a.inner)})
        th, td, te = t["host"][0], t["device"][0], t["device"][1]
        res["resolve"][str(thr)] = {
            "host_resolve_strands_ms": th, "resolve_strands_device_ms_host_clock": td, "resolve_strands_device_ms_device_events": te,
            "rounds": got.rounds, "record": dict(zip(engine.RESOLVE_COUNTERS, got.stats.words())),
            "summary": {"host_ms": med(th), "host_ms_min_max": spread(th), "device_ms": med(td), "device_ms_min_max": spread(td),
                        "host_over_device": med(th) / med(td), "rounds": got.rounds, "kept_pieces": got.stats.pieces,
                        "serially_cut_contigs": got.stats.serial}}

    class Fixed(torch.nn.Module):                            # infer_contigs' model: the fixed logits
        def forward(self, graph, x, e, pe):
            return scores[:, None]

    for thr in a.len_threshold:
        kw = dict(len_threshold=thr, decoder="greedy_cover", reads=store)
        t = alternate({"host": (lambda: decode.infer_contigs(Fixed(), g, None, None, pl, rl, **kw), 1),
                       "device": (lambda: decode.infer_contigs(Fixed(), g, None, None, pl, rl, device_resolve=True, **kw), a.infer_inner)})
        (th, _, h), (td, _, d) = t["host"], t["device"]
        assert h[1] == d[1] and torch.equal(h[2].bases, d[2].bases) and torch.equal(h[2].contig_ptr, d[2].contig_ptr)
        res["infer_contigs"][str(thr)] = {"host_resolve_ms": th, "device_resolve_ms": td, "walks": len(h[1]), "bases": int(h[2].bases.numel()),
                                          "summary": {"host_resolve_ms": med(th), "host_resolve_ms_min_max": spread(th),
                                                      "device_resolve_ms": med(td), "device_resolve_ms_min_max": spread(td)}}
        del t, h, d

    # ---- the serial fallback ------------------------------------------------------------------------------------------------------------
    K, L = a.serial_contigs, a.serial_nodes

    def small(twice):
        nodes = np.arange(K * L, dtype=np.int64).reshape(K, L) * 2           # contig k: reads k L .. k L + L - 1, + strand
        if twice:
            nodes[:, L // 2] = nodes[:, L // 4] ^ 1                          # ... and one of them again on its other strand
        t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(device=dev, dtype=dt)   # noqa: E731
        edges = np.arange(K * L, dtype=np.int64).reshape(K, L)
        edges[:, 0] = -1
        nn = 2 * K * L
        return decode.BogContigs(t(np.arange(K + 1) * L, torch.int32), t(nodes.reshape(-1), torch.int32), t(edges.reshape(-1), torch.int32),
                                 t(np.arange(K, 0, -1), torch.int64), torch.zeros(K, dtype=torch.int32, device=dev),
                                 decode.BogStats(contigs=K), torch.ones(K * L, dtype=torch.int64, device=dev),
                                 torch.ones(nn, dtype=torch.int64, device=dev))
    res["serial"] = {"contigs": K, "nodes_per_contig": L}
    covers = {"wave_cut": small(False), "serial_cut": small(True)}
    routes = {}
    for name, c in covers.items():
        want = decode.resolve_strands(fresh(c), 20)
        got = decode.resolve_strands_device(c, 20)
        assert got.resolved().walks == want.walks and got.stats.serial == (K if name == "serial_cut" else 0)
        res["serial"][name] = {"rounds": got.rounds}
        routes[name, "device"] = (lambda c=c: decode.resolve_strands_device(c, 20), a.inner)
        routes[name, "host"] = (lambda c=c: decode.resolve_strands(fresh(c), 20), a.infer_inner)
    t = alternate(routes)
    for name in covers:
        te, th = t[name, "device"][1], t[name, "host"][0]
        res["serial"][name].update({"resolve_strands_device_ms_device_events": te, "host_resolve_strands_ms": th,
                                    "summary": {"device_ms": med(te), "device_ms_min_max": spread(te), "host_ms": med(th)}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"resolve": {k: v["summary"] for k, v in res["resolve"].items()},
                      "infer_contigs": {k: v["summary"] for k, v in res["infer_contigs"].items()},
                      "serial": {k: res["serial"][k]["summary"] for k in ("wave_cut", "serial_cut")}}))


if __name__ == "__main__":
    main()
