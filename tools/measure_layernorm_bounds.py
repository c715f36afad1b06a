#!/usr/bin/env python3
"""Where the constants of tests/ln_reference.py come from: torch.nn.functional.layer_norm and its autograd in fp32 on the CPU
against the fp64 reference, on the row families and at every (H, width) of tests/test_gpu_layernorm_kernels.py.  No GPU needed.
    python tools/measure_layernorm_bounds.py [--write]      prints the table; --write: profiles/layernorm_kernel_bounds.json"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import ln_reference as lr  # noqa: E402

ROWS = 6000


def measure(rows=ROWS):
    ROWS = rows
    nf = len(lr.FAMILIES)
    ratio = {"fwd": np.zeros(nf), "bwd": np.zeros(nf)}
    raw = {"fwd": np.zeros(nf), "bwd": np.zeros(nf)}
    per_shape = {}
    for H, width in lr.HW:
        rng = np.random.default_rng(1000 * H + width)
        x, fam = lr.make_rows(rng, ROWS, H, width)
        ga, be = lr.make_affine(rng, H, width)
        gy = rng.standard_normal((ROWS, H)).astype(np.float32)
        gy[:, width:] = 0
        gy[rng.random((ROWS, H)) < 0.5] = 0           # a relu's gate
        ref = lr.ln_ref(x, ga, be, width)               # asserts that the fp64 reference is finite for every family
        gx64, Ab, Rb = lr.ln_bwd_ref(ref, gy)
        xt = torch.from_numpy(x[:, :width].copy()).requires_grad_(True)
        y = torch.nn.functional.layer_norm(xt, (width,), torch.from_numpy(ga[:width].copy()), torch.from_numpy(be[:width].copy()), lr.EPS)
        y.backward(torch.from_numpy(gy[:, :width].copy()))
        Af, Rf = lr.fwd_bound(ref)
        ef = y.detach().numpy().astype(np.float64) - ref["pre"][:, :width]
        eb = xt.grad.numpy().astype(np.float64) - gx64[:, :width]
        rf = lr.worst_ratio(ef, Af[:, :width], Rf[:, :width], fam)
        rb = lr.worst_ratio(eb, Ab[:, :width], Rb[:, :width], fam)
        per_shape[f"{H}x{width}"] = {"fwd": rf.round(4).tolist(), "bwd": rb.round(4).tolist()}
        ratio["fwd"], ratio["bwd"] = np.maximum(ratio["fwd"], rf), np.maximum(ratio["bwd"], rb)
        for k, e in (("fwd", ef), ("bwd", eb)):
            raw[k] = np.maximum(raw[k], [np.abs(e[fam == f]).max() for f in range(nf)])
    return ratio, raw, per_shape


def main():
    ratio, raw, per_shape = measure()
    out = {
        "what": "worst (|err| - u*rounding)+ / (u*A) of torch's fp32 CPU layer_norm (fwd: xhat*gamma+beta; bwd: autograd's input "
                "gradient) against fp64, per row family, over every (H, width) of the tests; bound parts A as in tests/ln_reference.py",
        "torch": torch.__version__, "rows_per_shape": ROWS, "families": list(lr.FAMILIES), "device_factor": lr.DEVICE_FACTOR,
        "cpu_fp32_ratio": {k: {f: float(np.ceil(v[i] * 100) / 100) for i, f in enumerate(lr.FAMILIES)} for k, v in ratio.items()},
        "cpu_fp32_exact": {k: {f: bool(v[i] == 0.0) for i, f in enumerate(lr.FAMILIES)} for k, v in raw.items()},
        "device_constant": {k: {f: float(lr.DEVICE_FACTOR * np.ceil(v[i] * 100) / 100) for i, f in enumerate(lr.FAMILIES)}
                            for k, v in ratio.items()},
        "per_shape": per_shape,
    }
    print(json.dumps(out, indent=1))
    if "--write" in sys.argv:
        d = {}
        if os.path.exists(lr.BOUNDS_FILE):
            d = json.load(open(lr.BOUNDS_FILE))
        d.update(out)
        json.dump(d, open(lr.BOUNDS_FILE, "w"), indent=1)
        open(lr.BOUNDS_FILE, "a").write("\n")


if __name__ == "__main__":
    main()
