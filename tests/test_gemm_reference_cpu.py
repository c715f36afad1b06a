"""CPU: the preconditions of tests/test_gpu_gemm_routes.py on its reference alone (tests/gemm_reference.py, profiles/gemm_bounds.json).

torch's fp32 CPU matmul stays inside bound(...) for every GEMM mode, family and K class; the `ints` family comes out bit-equal to the
fp64 result; the `cancel` family really cancels; the JSON holds every K class the GPU file uses, with c(K) <= K."""
import json

import numpy as np
import pytest
import torch

import gemm_reference as gr

# the K of the GPU file's tables that do not depend on the CU count (its split-K values lie between 513 and ~1100: classes 1024, 2048)
GPU_KS = (0, 1, 31, 32, 33, 65, 127, 128, 129, 256, 513, 514, 1025, 4095, 4096, 4097, 4096 + 15, 4096 + 16)
MODES = (gr.NT, gr.NN, gr.TN)


def _torch(mode, A, B):
    a, b = torch.from_numpy(A), torch.from_numpy(B)
    return ((a @ b.t()) if mode == gr.NT else (a @ b) if mode == gr.NN else (a.t() @ b)).numpy()


@pytest.mark.parametrize("K", [k for k in gr.K_CLASSES if k <= 4096] + [33, 65, 129, 513, 4097, 4112])
def test_torch_cpu_fp32_stays_inside_the_bound(K):
    for mode in MODES:
        for fam in gr.FAMILIES:
            if fam == "cancel" and not gr.uses_cancel(K):
                continue
            A, B, bias, resid = gr.operands(fam, mode, 65, 33, K, seed=5, epi=True)
            got = gr.f64(_torch(mode, A, B))
            err = np.abs(got - gr.product(mode, A, B))
            b = gr.bound("f32", K, gr.absprod(mode, A, B), gr.product(mode, A, B), family=fam)
            assert (err <= b).all(), f"{gr.MODE_NAMES[mode]} {fam} K={K}: worst err/bound {(err / np.maximum(b, 1e-300)).max():.3g}"
            # with the epilogue, added in fp32 the way the kernels do
            got2 = np.maximum((_torch(mode, A, B) + bias[None, :]) + resid, np.float32(0))
            want2 = gr.ref(mode, A, B, bias, resid, True)
            b2 = gr.bound("f32", K, gr.absprod(mode, A, B), want2, gr.epilogue(mode, A, B, bias, resid), family=fam)
            assert (np.abs(gr.f64(got2) - want2) <= b2).all(), f"{gr.MODE_NAMES[mode]} {fam} K={K}: epilogue"
            assert (b2 >= b - gr.U * np.abs(gr.product(mode, A, B))).all()


@pytest.mark.parametrize("K", [1, 33, 128, 1025, 4112])
def test_ints_family_is_exact_in_fp32(K):
    for mode in MODES:
        A, B, bias, resid = gr.operands("ints", mode, 129, 32, K, seed=2, epi=True)
        for x in (A, B, bias, resid):
            assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8
        want = gr.ref(mode, A, B, bias, resid, True)
        assert np.abs(gr.product(mode, A, B)).max() + 16 < 2 ** 24
        got = np.maximum((_torch(mode, A, B) + bias[None, :]) + resid, np.float32(0))
        assert got.dtype == np.float32 and np.array_equal(gr.f64(got), want)
    with pytest.raises(AssertionError):
        gr.ints((2, 1 << 18), 0, axis=1)


@pytest.mark.parametrize("K", [k for k in GPU_KS if gr.uses_cancel(k)])
def test_cancel_family_cancels(K):
    assert K in (128, 256, 4095, 4096, 4097, 4111, 4112)
    for mode in MODES:
        A, B, _, _ = gr.operands("cancel", mode, 128, 32, K, seed=3)
        small = np.abs(gr.product(mode, A, B)) <= 1e-3 * gr.absprod(mode, A, B)
        assert small.mean() >= 0.9, f"{gr.MODE_NAMES[mode]} K={K}: only {small.mean():.2f} of the elements cancel"
        assert np.abs(np.abs(A).mean() - gr.OFFSET) < 1 and np.abs(np.abs(B).mean() - gr.OFFSET) < 1


def test_bounds_file_holds_every_k_class():
    d = json.load(open(gr.BOUNDS_FILE))
    assert {int(k) for k in d["c"]} == set(gr.K_CLASSES) == {int(k) for k in d["c_family"]}
    for K in GPU_KS + (1100,):
        cls = gr.k_class(K)
        c = gr.c_of(K)
        assert c == min(d["c"][str(cls)], K) and (K == 0) == (c == 0)
        assert d["c"][str(cls)] == min(d["factor"] * d["cpu_fp32_ratio"][str(cls)], cls) and d["factor"] == 4.0
        assert d["cpu_fp32_ratio"][str(cls)] <= cls
        for fam in gr.FAMILIES:
            assert 0 <= gr.c_of(K, fam) <= c
    assert gr.k_class(4096) == 4096 and gr.k_class(4097) == 8192 and gr.k_class(1) == 1 and gr.k_class(0) == 0
    assert gr.U_ARITH == {"f32": 2.0 ** -24, "bf16x3": 2.0 ** -24, "f16x2": 2.0 ** -22}


def test_reference_functions_on_a_hand_case():
    A = np.array([[1, -2], [3, 4]], np.float32)       # NT: A[M,K], B[N,K]
    B = np.array([[5, 6], [-7, 8], [1, 0]], np.float32)
    assert np.array_equal(gr.ref(gr.NT, A, B), [[-7, -23, 1], [39, 11, 3]])
    assert np.array_equal(gr.absprod(gr.NT, A, B), [[17, 23, 1], [39, 53, 3]])
    assert np.array_equal(gr.ref(gr.NN, A, B.T.copy()), gr.ref(gr.NT, A, B))
    assert np.array_equal(gr.ref(gr.TN, A.T.copy(), B.T.copy()), gr.ref(gr.NT, A, B))
    bias, R = np.array([1, 2, 3], np.float32), np.full((2, 3), -10, np.float32)
    assert np.array_equal(gr.ref(gr.NT, A, B, bias, R, True), [[0, 0, 0], [30, 3, 0]])
    n, mag = gr.epilogue(gr.NT, A, B, bias, R)
    assert n == 2 and np.array_equal(mag, np.abs(gr.ref(gr.NT, A, B)) + bias[None, :] + 10)
    s, a = gr.colsum_ref(A)
    assert np.array_equal(s, [4, 2]) and np.array_equal(a, [4, 6])
    z = gr.ref(gr.NT, np.zeros((2, 0), np.float32), np.zeros((3, 0), np.float32), bias, R, True)      # K = 0: the epilogue alone
    assert np.array_equal(z, np.zeros((2, 3)))
