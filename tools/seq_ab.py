#!/usr/bin/env python3
"""What turning walks into bases costs (decode.contig_sequences: gnm_seq_layout + gnm_seq_emit).

  device   the synthetic graph of --reads reads (1.5 M nodes at 750 000), random scores, the contigs of
           decode.best_overlap_contigs (every node lies on one, so every read is written once per covered strand); a read store
           built ON the device with torch.randint (codes 1 .. 15, reads of --min-len .. --max-len bases), prefix lengths drawn
           below the read lengths.  Device events around --inner back-to-back calls, median over --runs windows, for the layout
           call, the emit call and both; the achieved bytes/s of the emit pass counts 1 B written + 0.5 B read per base.
  copy     in the same run, a plain torch device copy of a buffer as large as the output: what moving that many bytes costs.
  host     at 1/10 of the reads: the reference's method (evaluate.py:36-47) -- one Python string per node
           (ReadStore.sequence), slices joined per contig -- on the host clock, split into making the strings and joining them;
           the device bytes of that smaller case are compared with the joined strings.

One process, one JSON file (--out, default profiles/seq_emit.json).  No speed was promised in advance; nothing here asserts one."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def build(reads, lo, hi, seed, dev):
    import torch
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import decode, synth
    from gnnome_assembly_amd.reads import ReadStore
    src, dst, n = synth.make_graph(reads, seed=seed)
    gen = torch.Generator(device=dev).manual_seed(seed)
    R = (n + 1) // 2
    length = torch.randint(lo, hi + 1, (R,), device=dev, generator=gen)
    span = (length + 31) // 32 * 32
    base_off = torch.cumsum(span, 0) - span
    nbytes = int(span.sum()) // 2
    packed = (torch.randint(1, 16, (nbytes,), device=dev, generator=gen, dtype=torch.uint8)
              | (torch.randint(1, 16, (nbytes,), device=dev, generator=gen, dtype=torch.uint8) << 4))
    store = ReadStore(packed, base_off, length)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    s_d, _ = g.edges()
    rl = length[torch.arange(n, device=dev) >> 1]
    pl = (torch.rand(src.size, device=dev, generator=gen, dtype=torch.float64) * rl[s_d.long()]).long()
    g.edata["prefix_length"], g.ndata["read_length"] = pl, rl
    scores = torch.randn(src.size, device=dev, generator=gen)
    bog = decode.best_overlap_contigs(g, scores, pl, rl)
    return g, bog, store, pl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=750000)
    ap.add_argument("--min-len", type=int, default=2000)
    ap.add_argument("--max-len", type=int, default=6000)
    ap.add_argument("--runs", type=int, default=5, help="timed windows per route, after a warm-up of each")
    ap.add_argument("--inner", type=int, default=10, help="calls per window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seq_emit.json"))
    a = ap.parse_args()

    import torch
    from gnnome_assembly_amd import decode, engine
    assert torch.cuda.is_available(), "needs a GPU: this tool measures, it has no CPU mode"
    dev = torch.device("cuda:0")
    g, bog, store, pl = build(a.reads, a.min_len, a.max_len, 0, dev)
    n = g.num_nodes()
    cs = decode.contig_sequences(bog, g, store)
    total, P, C = cs.record.bases, cs.record.pieces, cs.record.contigs
    res = {"what": "contig sequences: gnm_seq_layout + gnm_seq_emit on the best-overlap contigs of the synthetic graph, a device "
                   "copy of an output-sized buffer, and the reference's string method on the host at 1/10 size; one process",
           "device": torch.cuda.get_device_name(0), "reads": a.reads, "nodes": n, "read_bases": [a.min_len, a.max_len],
           "store_bytes": int(store.packed.numel()), "record": dict(zip(engine.SEQ_COUNTERS, cs.record.words())),
           "launches": {"layout": 4, "emit": 1}, "chunk_bases": engine.SEQ_CHUNK_BASES}

    rec = torch.zeros(engine.SEQ_RECORD_WORDS, dtype=torch.int64, device=dev)
    i64 = lambda m: torch.empty(m, dtype=torch.int64, device=dev)  # noqa: E731
    piece_len, piece_off, base_ptr = i64(P), i64(P + 1), i64(C + 1)
    out = torch.empty((total + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    other = torch.empty_like(out)
    lay = lambda: engine.seq_layout(bog.contig_ptr, bog.walk_nodes, bog.walk_edges, pl, n, store.base_off, store.length,  # noqa: E731
                                    store.packed, rec, piece_len, piece_off, base_ptr)
    emit = lambda: engine.seq_emit(bog.walk_nodes, piece_off, n, store.base_off, store.length, store.packed, total, out)  # noqa: E731
    routes = {"layout": lay, "emit": emit, "layout_and_emit": lambda: (lay(), emit()), "torch_copy": lambda: other.copy_(out)}

    def window(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            routes[name]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.inner             # microseconds per call

    for r in routes:
        routes[r]()
        window(r)                                              # warm-up: code objects, the caching allocator
    assert torch.equal(out[:total], cs.bases), "the timed calls do not write what contig_sequences wrote"
    windows = {r: [] for r in routes}
    names = list(routes)
    for k in range(a.runs):
        for r in (names if k % 2 == 0 else names[::-1]):
            windows[r].append(window(r))
    med = {r: float(np.median(v)) for r, v in windows.items()}
    res["device_run"] = {
        "windows_us_per_call": windows, "calls_per_window": a.inner,
        "summary": {"median_us_per_call": med, "spread_us": {r: float(np.max(v) - np.min(v)) for r, v in windows.items()},
                    "output_bases": total, "emit_bytes_counted": 1.5 * total,
                    "emit_GB_per_s": 1.5 * total / med["emit"] / 1e3,
                    "layout_and_emit_GB_per_s": 1.5 * total / med["layout_and_emit"] / 1e3,
                    "torch_copy_GB_per_s_read_plus_write": 2.0 * out.numel() / med["torch_copy"] / 1e3},
        "note": "device events around back-to-back calls on one stream; emit bytes = 1 B written + 0.5 B read per base (offsets, "
                "walk arrays and re-read edges of the store are not counted); the copy moves 1 B read + 1 B written per byte"}
    del out, other, cs

    # ---- the reference's method on the host, at 1/10 size ----------------------------------------------------------------------------
    g2, bog2, store2, pl2 = build(max(a.reads // 10, 100), a.min_len, a.max_len, 1, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cs2 = decode.contig_sequences(bog2, g2, store2)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    h = bog2.host()
    host_store = store2.to("cpu")
    t0 = time.perf_counter()
    strings = [host_store.sequence(v) for v in range(g2.num_nodes())]
    t_strings = time.perf_counter() - t0
    ptr, nodes, edges, plh = h["contig_ptr"], h["walk_nodes"], h["walk_edges"], pl2.cpu().numpy()
    t0 = time.perf_counter()
    joined = []
    for c in range(ptr.size - 1):
        lo, hi = int(ptr[c]), int(ptr[c + 1])
        joined.append("".join([strings[nodes[p]][:plh[edges[p + 1]]] for p in range(lo, hi - 1)]) + strings[nodes[hi - 1]])
    t_join = time.perf_counter() - t0
    assert cs2.bases.cpu().numpy().tobytes().decode() == "".join(joined), "device bytes differ from the joined strings"
    res["host_route_tenth"] = {"reads": max(a.reads // 10, 100), "output_bases": cs2.record.bases,
                               "strings_per_node_s": t_strings, "slices_joined_s": t_join,
                               "contig_sequences_whole_call_s_host_clock": t_dev,
                               "note": "strings_per_node_s is what the reference holds in memory before it starts (one str per node); "
                                       "slices_joined_s is its walk_to_sequence loop; the device figure is ONE untimed-warm-up-free "
                                       "call with its allocations and its synchronisation, and its bytes equal the joined strings"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"device": res["device_run"]["summary"], "host_tenth": {k: v for k, v in res["host_route_tenth"].items() if k != "note"}}))


if __name__ == "__main__":
    main()
