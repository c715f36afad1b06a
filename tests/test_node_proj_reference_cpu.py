"""CPU: tests/node_proj_reference.py against torch fp64 autograd of nn.Linear(128, 640) and of BatchNorm + relu, and the launch
arithmetic it restates against the properties tests/test_gpu_node_proj_kernels.py relies on."""
import numpy as np
import pytest
import torch

import bn_reference as br
import gemm_reference as gr
import node_proj_reference as nr

H = nr.H


@pytest.mark.parametrize("family", ["normal", "rows", "ints"])
def test_linear_reference_equals_fp64_autograd(family):
    N, ncols = 77, 5 * H
    f, n, t = nr.case("fwd", family, N, ncols), nr.case("nn", family, N, ncols), nr.case("tn", family, N, ncols)
    lin = torch.nn.Linear(H, ncols).double()
    close = lambda got, want: np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)  # noqa: E731
    # forward on the forward case's operands
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(gr.f64(f["W"])))
        lin.bias.copy_(torch.from_numpy(gr.f64(f["b"])))
        assert close(lin(torch.from_numpy(gr.f64(f["h"]))).numpy(), f["ref"])
    # gh_in = gh_out + gP W on the NN case's operands (the residual path adds gh_out to the Linear's input gradient)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(gr.f64(n["W"])))
    h = torch.zeros(N, H, dtype=torch.float64, requires_grad=True)
    (lin(h) * torch.from_numpy(gr.f64(n["gP"]))).sum().backward()
    assert close(gr.f64(n["gh_out"]) + h.grad.numpy(), n["ref"])
    # gW = gP^T h_in, gb = sum gP on the TN case's operands
    lin.zero_grad()
    (lin(torch.from_numpy(gr.f64(t["h_in"]))) * torch.from_numpy(gr.f64(t["gP"]))).sum().backward()
    assert close(lin.weight.grad.numpy(), t["ref"]) and close(lin.bias.grad.numpy(), t["cs"])
    assert t["ref"].shape == (ncols, H) and t["cs"].shape == (ncols,) and n["ref"].shape == (N, H) and f["ref"].shape == (N, ncols)
    if family == "ints":
        for d in (f, n, t):
            assert np.array_equal(d["ref"], np.round(d["ref"])) and np.abs(d["ref"]).max() < 2 ** 24


def test_stats_reference_equals_batchnorm_backward_sums():
    """(sum gw, sum gw zhat) = (gbeta, ggamma) of relu(BatchNorm(z)) under fp64 autograd, and bn_reference's own column sums.  The
    fp32 stat row (mean, rstd rounded to fp32; zhat in two fp32 operations) moves zhat by a few u (1 + |zhat|)."""
    N = 200
    z, stat, ga, be = nr.lower_layer(N, seed=3)
    gh = np.random.default_rng(4).standard_normal((N, H)).astype(np.float32)
    s = nr.stats_ref(gh, z, stat)
    assert s["n_und"] == 0 and not s["und"].any()
    zt = torch.from_numpy(gr.f64(z))
    g, b = (torch.from_numpy(gr.f64(x)).requires_grad_(True) for x in (ga, be))
    out = torch.relu(torch.nn.functional.batch_norm(zt, None, None, g, b, True, 0.0, float(br.EPS)))
    (out * torch.from_numpy(gr.f64(gh))).sum().backward()
    assert np.abs(s["sums"][0] - b.grad.numpy()).max() <= 1e-12 * s["mags"][0].max()
    slack = 8 * br.U * (np.abs(gr.f64(gh)) * (1 + np.abs(br.xhat32(z, stat)))).sum(0)
    assert (np.abs(s["sums"][1] - g.grad.numpy()) <= slack).all()
    pre = br.branch(z, stat)[0]
    sums, mags = br.col_sums(gr.f64(gh) * (pre > 0), br.xhat32(z, stat))
    assert np.array_equal(sums, s["sums"]) and np.array_equal(mags, s["mags"])
    assert (nr.stats_bound(s, N, 8) >= N * br.U64 * s["mags"]).all()
    # a one-row z: var = 0, zhat = 0, the branch is beta's sign
    z1, st1, _, be1 = nr.lower_layer(1, seed=3)
    s1 = nr.stats_ref(gh[:1], z1, st1)
    assert s1["n_und"] == 0 and np.array_equal(s1["sums"][0], gr.f64(gh[0]) * (be1 > 0)) and not s1["sums"][1].any()


def test_bgrad_reference_and_integer_families():
    for N in (1, 2, 3, 33, 257):
        src, dst = nr.degrees_graph(N)
        assert src.size >= 1 and src.max() < N and dst.max() < N
        deg_in, deg_out = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
        if N >= 33:
            assert (deg_in == 0).any() and (deg_out == 0).any() and ((deg_in == 0) & (deg_out == 0)).any() and deg_in.max() >= N // 3 - 1
        in_ptr, out_ptr = np.concatenate([[0], np.cumsum(deg_in)]), np.concatenate([[0], np.cumsum(deg_out)])
        for fam in ("ints", "ints2", "normal"):
            d = nr.bgrad_inputs(N, fam, seed=7)
            val, bound = nr.bgrad_groups_ref(d, in_ptr, out_ptr)
            c = gr.f64(d["gamma_e"]) * gr.f64(d["stat_e"][1])
            want = c * (gr.f64(d["UT"][:, :H]) - deg_out[:, None] * gr.f64(d["bstat_e"][0]) - gr.f64(d["bstat_e"][1]) * gr.f64(d["UT"][:, H:]))
            assert np.array_equal(val[:, :H], want) and (bound > 0).all()
            if fam != "normal":
                assert np.array_equal(val, np.round(val)) and np.abs(val).max() < 2 ** 22
                assert (np.abs(val).T @ np.abs(gr.f64(d["h_in"]))).max() < 2 ** 24       # the TN product stays exact in fp32
            if fam == "ints":
                assert np.array_equal(val[:, :H], d["UT"][:, :H]) and np.array_equal(val[:, H:], d["Ud"])
            else:
                assert not np.array_equal(val[:, :H], d["UT"][:, :H]) or N == 1


@pytest.mark.parametrize("cus", [8, 64, 104, 256, 304])
def test_launch_arithmetic(cus):
    """The derived row counts give two items to some workgroup, stay inside the contraction classes of profiles/gemm_bounds.json
    where the bound is used, and the forced slots are all busy from 8 tiles on."""
    for mode in ("f32", "bf16x3"):
        n = nr.first_rows_with_two_items(nr.nn_grid(1, mode, cus, 1)[2], lambda N: nr.nn_grid(N, mode, cus, 1)[1], 37)
        g, per, rows = nr.nn_grid(n, mode, cus, 1)
        assert per == 2 and g % 8 == 0 and g <= max(cus, 8) + 7 and n % 32 == 5 and nr.nn_grid(n - rows, mode, cus, 1)[1] == 1
    for tile, ncg in ((32, 5), (64, 5), (32, 16)):
        bpc = 1 if ncg == 5 else 8
        n = nr.first_rows_with_two_items(tile, lambda N: nr.tn_nslot(N, tile, ncg, cus, bpc)[1], 5)
        nslot, per = nr.tn_nslot(n, tile, ncg, cus, bpc)
        assert per == 2 and nslot % 8 == 0 and nslot * ncg <= nr.MAX_PARTIAL_BLOCKS and n <= 8192
        gr.k_class(n)
        for fewer in range(1, bpc + 1):         # a smaller occupancy only takes slots away
            assert nr.tn_nslot(n, tile, ncg, cus, fewer)[1] >= 2
    assert nr.fwd_nslot_max(cus) % 8 == 0 and nr.fwd_nslot_max(cus) >= 8
    for tile in (32, 64):
        assert {8 * tile - 1, 8 * tile, 8 * tile + 1} <= set(nr.rows_for(tile)) and set(nr.ROWS) <= set(nr.rows_for(tile))
        assert nr.tn_nslot(8 * tile, tile, 1, cus, 2) == (8, 1) and nr.tn_nslot(8 * tile - 1, tile, 1, cus, 2) == (8, 1)
        assert nr.tn_nslot(1, tile, 5, cus, 2) == (8, 1)        # seven empty slots
    assert nr.persistent_grid(1, 1, 8, cus) == 8 and nr.persistent_grid(10 ** 6, 1, 8, 256) == 2048
