"""CPU: the fp64 LayerNorm reference and the bound parts of tests/ln_reference.py, which tests/test_gpu_layernorm_kernels.py holds
the kernels to -- finite for every row family at every (H, width), equal to torch's fp64 autograd; the committed constants (profiles/layernorm_kernel_bounds.json) are four times the recorded
ratios, and a reduced run of tools/measure_layernorm_bounds.py stays within those ratios."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import ln_reference as lr


@pytest.mark.parametrize("H,width", lr.HW)
def test_fp64_reference_is_finite_and_equals_autograd(H, width):
    rng = np.random.default_rng(H + width)
    R = 600
    x, fam = lr.make_rows(rng, R, H, width)
    assert sorted(set(fam.tolist())) == list(range(len(lr.FAMILIES)))
    assert not x[:, width:].any() and not x[fam == lr.FAMILIES.index("zero")].any()
    const = x[fam == lr.FAMILIES.index("constant")][:, :width]
    assert (const == const[:, :1]).all() and np.abs(const).max() > 10
    ga, be = lr.make_affine(rng, H, width)
    gy = rng.standard_normal((R, H)).astype(np.float32)
    ref = lr.ln_ref(x, ga, be, width)                 # asserts finiteness itself
    gx, A, Rnd = lr.ln_bwd_ref(ref, gy)
    assert np.isfinite(A).all() and (A >= 0).all() and not gx[:, width:].any() and not ref["pre"][:, width:].any()
    xt = torch.from_numpy(x[:, :width].astype(np.float64)).requires_grad_(True)
    y = torch.nn.functional.layer_norm(xt, (width,), torch.from_numpy(ga[:width]).double(), torch.from_numpy(be[:width]).double(), lr.EPS)
    y.backward(torch.from_numpy(gy[:, :width]).double())
    assert np.abs(y.detach().numpy() - ref["pre"][:, :width]).max() <= 1e-12 * max(1.0, np.abs(ref["pre"]).max())
    assert np.abs(xt.grad.numpy() - gx[:, :width]).max() <= 1e-11 * max(1.0, np.abs(gx).max())
    assert (ref["xhat"][fam == lr.FAMILIES.index("constant")] == 0).all()


def test_committed_constants_are_four_times_the_recorded_cpu_ratios():
    d = json.load(open(lr.BOUNDS_FILE))
    c = lr.load_constants()
    assert d["families"] == list(lr.FAMILIES) and d["device_factor"] == lr.DEVICE_FACTOR == 4.0
    for k in ("fwd", "bwd"):
        for i, f in enumerate(lr.FAMILIES):
            assert c[k][i] == 4.0 * d["cpu_fp32_ratio"][k][f] == d["device_constant"][k][f]
            if d["cpu_fp32_exact"][k][f]:           # exact implies ratio 0
                assert d["cpu_fp32_ratio"][k][f] == 0.0
    assert c["fwd_exact"].tolist() == [False, False, False, True, True, False]


def test_reduced_measurement_stays_within_the_recorded_cpu_ratios():
    """tools/measure_layernorm_bounds.measure on a tenth of the rows: torch's fp32 CPU layer_norm shows no ratio above the recorded
    one (the recorded figure is the worst over ten times as many rows), and is exact where the record says so."""
    spec = importlib.util.spec_from_file_location("measure_layernorm_bounds", os.path.join(os.path.dirname(lr.BOUNDS_FILE), "..", "tools",
                                                                                       "measure_layernorm_bounds.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    ratio, raw, _ = m.measure(rows=600)
    d = json.load(open(lr.BOUNDS_FILE))
    for k in ("fwd", "bwd"):
        for i, f in enumerate(lr.FAMILIES):
            assert ratio[k][i] <= d["cpu_fp32_ratio"][k][f], (k, f, ratio[k][i])
            if d["cpu_fp32_exact"][k][f]:
                assert raw[k][i] == 0.0, (k, f, raw[k][i])
