#!/usr/bin/env python3
"""Wall time of the contig decode on the synthetic graph of bench.py: the host path (decode.get_contigs, the baseline) against
decode.get_contigs_device with one walk thread and with the default thread count.

    python tools/decode_timing.py [--reads 75000 750000] [--out profiles/decode_timing.json]

One process per row (graph size x path), each under its own `timeout`, one after the other; the first row that fails ends the
run (nothing is retried) and what was measured so far is still written.  A row builds synth.make_graph(R) (N = 2R nodes,
E ~ 10R edges), takes the logits of the fixed-seed model of bench.py --inference (hidden 128, 8 layers) on it, and decodes with
nb_paths = 50, len_threshold = 20 and seeded prefix / read lengths.  Reported per row: the number of iterations, and per
iteration (median and mean, milliseconds)
  sampling  (a) the candidate list of the not-yet-visited sub-graph and the draw of the start edges -- on the host path the
            gathers, flatnonzero, sigmoid and torch's sampler, on the device path the two launches, the read-back of the picks and
            the upload of visited[] after an accepted contig;
  walks     (b) the 2 x nb_paths greedy walks, the choice of the best and the visited[] update (gnm_decode_iteration[_mt]);
and `decode_s`, the whole decode (scores already computed; it includes the one copy of the scores to the host).  The host and
device paths draw different random numbers from the same distribution, so their iteration counts may differ by a few.
`--row` (internal) measures one row in this process and prints its JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PATHS = ("host", "device_threads1", "device_default")


class _Stop(Exception):
    pass


def _stats(ms):
    import numpy as np
    a = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(a)), 3), "mean_ms": round(float(a.mean()), 3)} if a.size else None


def row(reads: int, path: str, max_iterations: int, seed: int = 0):
    import numpy as np
    import torch
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import _lib, decode, synth
    assert torch.cuda.is_available(), "needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    H, L, nb, thr = 128, 8, 50, 20
    src, dst, n = synth.make_graph(reads, seed=seed)
    inp = synth.make_inputs(src, dst, n, seed=seed)
    g = G.AssemblyGraph(src, dst, n).to(dev)
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, seed, randomize_norm=False).items()})
    model.to(dev).eval()
    e, pe = torch.from_numpy(inp["e"]).to(dev), torch.from_numpy(inp["pe"]).to(dev)
    with torch.no_grad():
        scores = model(g, None, e, pe).squeeze(-1)
    torch.cuda.synchronize()
    rng = np.random.default_rng(seed)
    pl, rl = rng.integers(500, 12000, src.size), rng.integers(8000, 25000, n)
    dg = decode.DecodeGraph(src, dst, n)
    torch.manual_seed(seed)
    out = {"reads": reads, "nodes": int(n), "edges": int(src.size), "path": path, "nb_paths": nb, "len_threshold": thr,
           "threads": 1 if path != "device_default" else decode.decode_threads(nb)}
    sampling, walks, finished = [], [], True
    t_start = time.perf_counter()
    if path == "host":
        # get_contigs itself is untouched: the walks are timed around the library call it makes, the rest of an iteration
        # (from the end of the previous walks to the start of these) is its candidate list + sampling
        lib = _lib.load()
        marks = {"t": None}

        def timed_iteration(*a):
            t0 = time.perf_counter()
            sampling.append((t0 - marks["t"]) * 1e3)
            r = lib.gnm_decode_iteration(*a)
            marks["t"] = time.perf_counter()
            walks.append((marks["t"] - t0) * 1e3)
            if len(walks) >= max_iterations:
                raise _Stop
            return r

        proxy = types.SimpleNamespace(gnm_decode_iteration=timed_iteration)
        real = decode._lib
        decode._lib = types.SimpleNamespace(load=lambda: proxy, check=real.check, GnmError=real.GnmError)
        try:
            sc = scores.detach().float().cpu()
            marks["t"] = time.perf_counter()
            contigs = decode.get_contigs(dg, sc, pl, rl, nb, thr)
        except _Stop:
            contigs, finished = None, False
        finally:
            decode._lib = real
    else:
        tm = []
        count = {"n": 0}

        def uniforms(it, k):
            count["n"] += 1
            if count["n"] > max_iterations:
                raise _Stop
            return torch.rand(k, dtype=torch.float64)

        try:
            contigs = decode.get_contigs_device(dg, scores, pl, rl, nb, thr, uniforms=uniforms,
                                                threads=1 if path == "device_threads1" else None, timings=tm)
        except _Stop:
            contigs, finished = None, False
        sampling, walks = [a * 1e3 for a, _ in tm], [b * 1e3 for _, b in tm]
    dt = time.perf_counter() - t_start
    out.update(iterations=len(walks), sampling=_stats(sampling), walks=_stats(walks), finished=finished,
               decode_s=round(dt, 3) if finished else None, contigs=len(contigs) if contigs is not None else None,
               contig_nodes=sum(len(c) for c in contigs) if contigs is not None else None)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reads", type=int, nargs="+", default=[75_000, 750_000], help="R per graph; N = 2R nodes, E ~ 10R edges")
    ap.add_argument("--paths", nargs="+", default=list(PATHS), choices=PATHS)
    ap.add_argument("--max-iterations", type=int, default=200, help="stop a row after this many iterations (finished: false)")
    ap.add_argument("--row-timeout", type=int, default=420, help="seconds per row")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_timing.json"))
    ap.add_argument("--row", nargs=2, metavar=("READS", "PATH"), default=None, help="(internal) measure one row here")
    args = ap.parse_args()
    if args.row:
        row(int(args.row[0]), args.row[1], args.max_iterations)
        return 0
    rows, failed = [], None
    for reads in args.reads:
        for path in args.paths:
            cmd = ["timeout", "-k", "10", str(args.row_timeout), sys.executable, os.path.abspath(__file__), "--row", str(reads),
                   path, "--max-iterations", str(args.max_iterations)]
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                failed = {"reads": reads, "path": path, "returncode": p.returncode}
                break
            r = json.loads(lines[-1])
            r["process_s"] = round(time.perf_counter() - t0, 1)
            rows.append(r)
            print(json.dumps(r), flush=True)
        if failed:
            break
    result = {"tool": "tools/decode_timing.py", "rows": rows}
    if failed:
        result["failed"] = failed          # a fault, an abort or a time limit: nothing after it was started
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
