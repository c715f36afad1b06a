#!/usr/bin/env python3
"""Where the constants of tests/bn_reference.py come from: torch's fp32 CPU batch_norm (training mode) and its autograd against the
fp64 reference functions of tests/bn_reference.py, on the column families and at every kernel width of
tests/test_gpu_batchnorm_kernels.py.  No GPU needed.
    python tools/measure_batchnorm_bounds.py [--write]      prints the table; --write: profiles/batchnorm_kernel_bounds.json
fwd: torch.native_batch_norm's output against bn_reference.bn_apply_ref on the stat row formed from the (mean, invstd) torch itself
saved, with the terms of torch's own shift (|beta| + |mean scale|) in A; bwd: autograd's input gradient against bn_reference.bn_bwd_apply_ref on that stat row and the fp64 column means of gy,
gy * xhat rounded to fp32 (what gnm_bn_bwd_finalize writes).  The ratio is the worst (|err| - u Rnd)+ / (u A) per column family."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import bn_reference as br  # noqa: E402

ROWS = 6000
SEEDS = range(6)        # column draws per width: a column's statistics err as a whole, so the worst ratio is a maximum over COLUMNS


def _ratio(err, A, Rnd, fam):
    over = np.maximum(np.abs(err) - br.U * Rnd, 0.0)
    assert not (over[A == 0] > 0).any(), "error beyond rounding where the bound has no scalable part"
    q = np.divide(over, br.U * A, out=np.zeros_like(over), where=A > 0).max(0)
    return np.array([q[fam == f].max() if (fam == f).any() else 0.0 for f in range(len(br.FAMILIES))])


def measure(rows=ROWS, seed=0):
    nf = len(br.FAMILIES)
    ratio = {k: np.zeros(nf) for k in ("fwd", "bwd")}
    per_shape = {}
    for H in br.WIDTHS:
        rng = np.random.default_rng(1000 * H + seed)
        fam = br.col_families(rng, H, seed)
        x = br.make_cols(rng, rows, fam)
        ga, be = br.make_affine(rng, fam, rows)
        gy = rng.standard_normal((rows, H)).astype(np.float32)
        gy[rng.random((rows, H)) < 0.5] = 0           # a relu's gate
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        w, b = torch.from_numpy(ga.copy()), torch.from_numpy(be.copy())
        with torch.no_grad():
            y, mean, invstd = torch.native_batch_norm(xt.detach(), w, b, None, None, True, 0.1, float(br.EPS))
        mean32, rstd32 = mean.numpy(), invstd.numpy()
        scale32 = (ga * rstd32).astype(np.float32)
        stat = np.stack([mean32, rstd32, scale32, (be - (mean32 * scale32).astype(np.float32)).astype(np.float32)])
        want, A, Rnd, und = br.bn_apply_ref(x, stat)
        pre = br.branch(x, stat)[0]
        # torch forms its own shift: where beta - mean * scale cancels, |shift| says nothing about that rounding, so the terms of
        # the shift stand in A here (A >= the kernels' |x scale| + |shift|: the constant the tests take is the stricter one)
        A = np.abs(br.f64(x) * br.f64(scale32)[None, :]) + (np.abs(br.f64(be)) + np.abs(br.f64(mean32) * br.f64(scale32)))[None, :]
        rf = _ratio(y.numpy().astype(np.float64) - pre, A, np.abs(pre), fam)
        torch.nn.functional.batch_norm(xt, None, None, w, b, True, 0.1, float(br.EPS)).backward(torch.from_numpy(gy.copy()))
        xh = br.xhat32(x, stat)
        bstat = (br.col_sums(gy, xh)[0] / rows).astype(np.float32)
        gx, Ab, Rb = br.bn_bwd_apply_ref(x, stat, bstat, ga, gy, 1.0)
        rb = _ratio(xt.grad.numpy().astype(np.float64) - gx, Ab, Rb, fam)
        per_shape[str(H)] = {"fwd": rf.round(4).tolist(), "bwd": rb.round(4).tolist()}
        ratio["fwd"], ratio["bwd"] = np.maximum(ratio["fwd"], rf), np.maximum(ratio["bwd"], rb)
    return ratio, per_shape


def main():
    ratio, per_shape = None, {}
    for seed in SEEDS:
        r, ps = measure(seed=seed)
        ratio = r if ratio is None else {k: np.maximum(ratio[k], r[k]) for k in r}
        per_shape[f"seed{seed}"] = ps
    out = {
        "what": "worst (|err| - u*rounding)+ / (u*A) of torch's fp32 CPU batch_norm (fwd: x*scale+shift on its own saved mean / invstd; bwd: "
                "autograd's input gradient) against the fp64 functions of tests/bn_reference.py, per column family, over every kernel width",
        "torch": torch.__version__, "rows_per_shape": ROWS, "column_draws_per_width": len(SEEDS), "families": list(br.FAMILIES), "device_factor": br.DEVICE_FACTOR,
        "cpu_fp32_ratio": {k: {f: float(np.ceil(v[i] * 100) / 100) for i, f in enumerate(br.FAMILIES)} for k, v in ratio.items()},
        "per_shape": per_shape,
    }
    print(json.dumps(out, indent=1))
    if "--write" in sys.argv:
        d = {}
        if os.path.exists(br.BOUNDS_FILE):
            d = json.load(open(br.BOUNDS_FILE))
        d.update(out)
        json.dump(d, open(br.BOUNDS_FILE, "w"), indent=1)
        open(br.BOUNDS_FILE, "a").write("\n")


if __name__ == "__main__":
    main()
