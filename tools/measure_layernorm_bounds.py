#!/usr/bin/env python3
"""Where the constants of tests/ln_reference.py come from: torch.nn.functional.layer_norm and its autograd in fp32 on the CPU
against the fp64 reference, on the row families and at every (H, width) of tests/test_gpu_layernorm_kernels.py.  No GPU needed.
    python tools/measure_layernorm_bounds.py [--write]      prints the table; --write: profiles/layernorm_kernel_bounds.json
    python tools/measure_layernorm_bounds.py --wide [--write]       the same measurement at the (padded width, width) shapes of the wide
        LayerNorm layers (tests/test_gpu_wide_layernorm_kernels.py), plus the row statistics (mean, rstd) torch.native_layer_norm
        returns; --write: profiles/layernorm_wide_kernel_bounds.json"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import ln_reference as lr  # noqa: E402

ROWS = 6000
WIDE_HW = [(512, 512), (512, 320), (768, 600), (512, 257)]      # two full chunks, a half-dead last chunk, three chunks, one live channel
WIDE_BOUNDS_FILE = os.path.join(REPO, "profiles", "layernorm_wide_kernel_bounds.json")


def stat_bound(x, ref):
    """Bound parts of the row statistics, [R,2] each for (mean, rstd): |err| <= c u A + u Rnd with the row family's forward constant.
    mean: a sum of `width` terms of size up to max|x| (A = max|x|), one final rounding.  rstd: its relative error is of the order
    u X (tests/ln_reference.py), then var + eps, the square root and the division round once each (Rnd = 3 rstd)."""
    xl = np.asarray(x, np.float64)[:, :ref["width"]]
    mean, rstd = xl.mean(1, keepdims=True), ref["rstd"]
    want = np.concatenate([mean, rstd], 1)
    A = np.concatenate([np.abs(xl).max(1, keepdims=True), rstd * ref["X"]], 1)
    return want, A, np.concatenate([np.abs(mean), 3 * rstd], 1)


def measure(rows=ROWS, shapes=None, stat=False):
    """shapes: the (H, width) list, default the kernel widths' (lr.HW).  stat: also measure torch.native_layer_norm's (mean, rstd)
    against stat_bound (key "stat" in every returned dict)."""
    ROWS = rows
    nf = len(lr.FAMILIES)
    kinds = ("fwd", "bwd", "stat") if stat else ("fwd", "bwd")
    ratio = {k: np.zeros(nf) for k in kinds}
    raw = {k: np.zeros(nf) for k in kinds}
    per_shape = {}
    for H, width in (lr.HW if shapes is None else shapes):
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
        errs = [("fwd", ef), ("bwd", eb)]
        if stat:
            _, mean32, rstd32 = torch.native_layer_norm(xt.detach(), (width,), None, None, lr.EPS)
            want, As, Rs = stat_bound(x, ref)
            es = torch.cat([mean32.reshape(-1, 1), rstd32.reshape(-1, 1)], 1).numpy().astype(np.float64) - want
            rs = lr.worst_ratio(es, As, Rs, fam)
            per_shape[f"{H}x{width}"]["stat"] = rs.round(4).tolist()
            ratio["stat"] = np.maximum(ratio["stat"], rs)
            errs.append(("stat", np.maximum(np.abs(es) - lr.U * Rs, 0.0)))     # "exact" for the statistics: within their final roundings
        for k, e in errs:
            raw[k] = np.maximum(raw[k], [np.abs(e[fam == f]).max() for f in range(nf)])
    return ratio, raw, per_shape


def main():
    wide = "--wide" in sys.argv
    ratio, raw, per_shape = measure(shapes=WIDE_HW, stat=True) if wide else measure()
    bounds_file = WIDE_BOUNDS_FILE if wide else lr.BOUNDS_FILE
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
    if wide:
        out["what"] = ("the measurement of layernorm_kernel_bounds.json at the (padded width, width) shapes of the LayerNorm layers wider "
                       "than 256 channels; stat: (mean, rstd) of torch.native_layer_norm against tools/measure_layernorm_bounds.stat_bound")
        out["shapes"] = [list(hw) for hw in WIDE_HW]
    print(json.dumps(out, indent=1))
    if "--write" in sys.argv:
        d = {}
        if os.path.exists(bounds_file):
            d = json.load(open(bounds_file))
        d.update(out)
        json.dump(d, open(bounds_file, "w"), indent=1)
        open(bounds_file, "a").write("\n")


if __name__ == "__main__":
    main()
