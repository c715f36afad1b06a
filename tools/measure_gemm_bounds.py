#!/usr/bin/env python3
"""Where c(K) of tests/gemm_reference.py comes from: torch's fp32 CPU matmul against the fp64 reference of the same fp32 operands, for
every GEMM mode (NT, NN, TN), input family and K class of tests/test_gpu_gemm_routes.py.  No GPU needed.
    python tools/measure_gemm_bounds.py [--write]      prints the table; --write: profiles/gemm_bounds.json
ratio = worst |torch - ref| / (u absprod) over the elements of a 128 x 128 product at the K of the class (its largest), over SEEDS
seeds; per K class the worst over modes and families, rounded up to two decimals; c(K) = min(4 x ratio, K) -- the factor 4 of
tools/measure_batchnorm_bounds.py for the other summation order of a tiled matrix-core kernel, K the worst case of any order.
c_family: the same per family (the heavy-tailed `rows` family sets the class's worst by an order of magnitude; a well-conditioned
family held to that would hide an error of 2^-18 per product), which is what the tests use.
One thread, so that the numbers do not depend on how the machine splits the product."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import gemm_reference as gr  # noqa: E402

SEEDS = range(4)
M = N = 128
FACTOR = 4.0


def torch_product(mode, A, B):
    a, b = torch.from_numpy(A), torch.from_numpy(B)
    return ((a @ b.t()) if mode == gr.NT else (a @ b) if mode == gr.NN else (a.t() @ b)).numpy()


def ratio(mode, family, K, seed):
    A, B, _, _ = gr.operands(family, mode, M, N, K, 1000 * seed + 17)
    err = np.abs(gr.f64(torch_product(mode, A, B)) - gr.product(mode, A, B))
    ap = gr.absprod(mode, A, B)
    assert not (err[ap == 0] > 0).any()
    return float(np.divide(err, gr.U * ap, out=np.zeros_like(err), where=ap > 0).max())


def measure():
    torch.set_num_threads(1)
    table = {}
    for K in gr.K_CLASSES:
        row = {}
        for mode in (gr.NT, gr.NN, gr.TN):
            for family in gr.FAMILIES:
                if K == 0 or (family == "cancel" and not gr.uses_cancel(K)):
                    continue
                row[f"{gr.MODE_NAMES[mode]}/{family}"] = max(ratio(mode, family, K, s) for s in SEEDS)
        table[K] = row
    return table


def main():
    table = measure()
    up = lambda v: float(np.ceil(v * 100) / 100)  # noqa: E731
    worst = {K: up(max(row.values(), default=0.0)) for K, row in table.items()}
    assert all(v <= K for K, v in worst.items()), "a ratio above K, the worst case of any summation order: the measurement is wrong"
    # per family over the three modes; `cancel` and `ints` take the `normal` ratio (gemm_reference: torch's own order happens to keep
    # cancel's partial sums near zero, which no other order has to; its absprod-relative error stays below a well-conditioned sum's)
    fam = {K: {f: up(max((v for k, v in row.items() if k.endswith("/" + ("rows" if f == "rows" else "normal"))), default=0.0))
               for f in gr.FAMILIES} for K, row in table.items()}
    out = {
        "what": "worst |torch fp32 CPU matmul - fp64 reference| / (2^-24 * sum_k |a||b|) per K class (0, then the next power of two >= K) "
                "over NT / NN / TN and the families of tests/gemm_reference.py on 128 x 128 products; c = min(factor * ratio, K)",
        "torch": torch.__version__, "seeds": len(SEEDS), "factor": FACTOR,
        "cpu_fp32_ratio": {str(K): v for K, v in worst.items()},
        "c": {str(K): min(FACTOR * v, float(K)) for K, v in worst.items()},
        "c_family": {str(K): {f: min(FACTOR * v, float(K)) for f, v in row.items()} for K, row in fam.items()},
        "per_class": {str(K): {k: round(v, 4) for k, v in row.items()} for K, row in table.items()},
    }
    print(json.dumps(out, indent=1))
    if "--write" in sys.argv:
        json.dump(out, open(gr.BOUNDS_FILE, "w"), indent=1)
        open(gr.BOUNDS_FILE, "a").write("\n")


if __name__ == "__main__":
    main()
