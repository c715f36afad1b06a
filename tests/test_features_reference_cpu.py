"""CPU: tests/features_reference.py -- the fp64 statements of gnm_pagerank_pe and gnm_edge_feats_zscore against the project's
existing fp32 twins and the golden file, the two per-element bars against what a correct kernel may do (another summation order,
the kernel's blocked one-pass sums in fp64), and their teeth: every listed way of getting the features subtly wrong misses the
bar on at least one case of the matrix tests/test_gpu_features.py runs on the device.

One listed mutant cannot miss any bar: PageRank with dinv left at 1 / 1e-9 for nodes without out-edges.  Such a node is the source
of no edge, so its dinv -- zeroed or not -- is never read, in the reference's sparse product as little as in the kernel's gather;
test_unzeroed_dinv_is_unobservable pins that down (bit-identical output) instead of asserting a failure that no implementation
could produce.  The neighbouring mistake that IS observable, handing the leaked mass of those nodes back to everybody (textbook
PageRank), is in the mutant list in its place."""
import os

import numpy as np
import pytest

import features_reference as fr
from helpers import zscore

PR_CASES = fr.pagerank_cases()
ZS_CASES = fr.zscore_cases()


# ---- the oracles ---------------------------------------------------------------------------------------------------------------

def test_pagerank_pe64_rounds_to_the_fp32_twin():
    from gnnome_assembly_amd import synth
    for name, (src, dst, n, pe_dim, alpha) in PR_CASES.items():
        if n > 100000:
            continue
        want = fr.pagerank_pe64(src, dst, n, pe_dim, alpha)
        assert want.dtype == np.float64 and want.shape == (n, 2 + pe_dim)
        twin = synth.pagerank_pe(src, dst, n, pe_dim, alpha)
        assert np.array_equal(want[:, 2:].astype(np.float32), twin), name
        assert np.array_equal(want[:, 0], np.bincount(dst, minlength=n)) and np.array_equal(want[:, 1], np.bincount(src, minlength=n))


def test_pagerank_pe64_against_the_golden_file(golden_dir):
    """The golden file holds the reference's own fp32 output (scipy's sparse product: another summation order)."""
    z = np.load(os.path.join(golden_dir, "pe_pagerank.npz"))
    n = int(z["n"])
    want = fr.pagerank_pe64(z["src"], z["dst"], n, 16, 0.95)
    assert np.array_equal(want[:, 0], z["in_deg"]) and np.array_equal(want[:, 1], z["out_deg"])
    bound = fr.pagerank_bound(want, fr.max_in_degree(z["dst"], n), 16)
    assert np.all(np.abs(z["pe"].astype(np.float64) - want[:, 2:]) <= bound[:, 2:])


def test_pagerank_closed_forms():
    want, _ = fr.pagerank_want("E=0, N=300")
    assert np.array_equal(want[:, :2], np.zeros((300, 2))) and np.array_equal(want[:, 2:], np.full((300, 16), (1.0 - 0.95) / 300))
    want, _ = fr.pagerank_want("small graph, alpha=0.0")
    assert np.array_equal(want[:, 2:], np.full((64, 16), 1.0 / 64))
    want, _ = fr.pagerank_want("N=1, one self loop")
    assert np.all(np.abs(want[:, 2:] - 1.0) < 1e-7) and np.array_equal(want[:, :2], [[1.0, 1.0]])


def test_zscore64_against_helpers():
    for name, c in ZS_CASES.items():
        want, _ = fr.zscore_want(name)
        for j, x in enumerate((c["a"], c["b"])):
            if not c["accuracy"][j]:
                assert not np.isfinite(want[:, j]).any(), name          # 0 / 0 like the reference
                continue
            ref = zscore(x)                                              # two-pass numpy: pairwise sums, mean rounded once
            tol = 64 * fr.U64 * len(x) ** 0.5 * c["kappa"][j] ** 0.5 * (1.0 + np.abs(want[:, j]))
            assert np.all(np.abs(ref - want[:, j]) <= tol), (name, j, float(np.abs(ref - want[:, j]).max()))
        fin = np.isfinite(want)
        assert abs(np.where(fin, want, 0.0).sum(0)).max() < 1e-6
        E = len(c["a"])
        for j in range(2):
            if c["accuracy"][j]:
                assert abs((want[:, j] ** 2).sum() - (E - 1)) < 1e-6 * E


def test_half_ulp32():
    x = np.array([1.0, 1.5, 2.0 - 1e-12, 2.0, 3e-5, 0.0, 1e-45])
    h = fr.half_ulp32(x)
    assert h[0] == 2.0 ** -24 and h[1] == 2.0 ** -24 and h[2] == 2.0 ** -24 and h[3] == 2.0 ** -23
    assert h[4] == np.spacing(np.float32(3e-5)) / 2 and h[5] == 2.0 ** -150 and h[6] == 2.0 ** -150
    r = np.random.default_rng(0).standard_normal(10000) * 10.0 ** np.random.default_rng(1).integers(-20, 20, 10000)
    assert np.all(np.abs(r.astype(np.float32).astype(np.float64) - r) <= fr.half_ulp32(r))


def test_launch_arithmetic():
    assert fr.pr_grid(1) == 1 and fr.pr_grid(256) == 1 and fr.pr_grid(257) == 2 and fr.pr_grid(10 ** 7) == 2048
    assert fr.zs_blocks(2048 * 256 - 1) == 2048 and fr.zs_blocks(2048 * 256 + 257) == 2048 and fr.zs_blocks(2048 * 256 + 257, 304) == 2048
    assert fr.zs_blocks(255, 80) == 1 and fr.zs_blocks(10 ** 6, 80) == 640
    big = [n for (_, _, n, _, _) in PR_CASES.values() if n > fr.MI355X_CUS * 8 * fr.BLOCK]
    assert big == [fr.MI355X_CUS * 8 * fr.BLOCK + 257]                 # one case in which every grid-stride loop takes a second trip


# ---- the bars admit a correct kernel -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PR_CASES))
def test_pagerank_bound_admits_another_summation_order(name):
    src, dst, n, pe_dim, alpha = PR_CASES[name]
    want, bound = fr.pagerank_want(name)
    for seed in (0, 1):
        p = np.random.default_rng(seed).permutation(len(src))
        got = fr.pagerank_pe64(src[p], dst[p], n, pe_dim, alpha).astype(np.float32)
        assert np.array_equal(got[:, :2], want[:, :2])
        r, i = fr.worst_ratio(got, want, bound)
        assert r <= 1.0, (name, r, np.unravel_index(i, want.shape))


@pytest.mark.parametrize("name", list(ZS_CASES))
def test_zscore_bound_admits_the_blocked_one_pass_sums(name):
    c = ZS_CASES[name]
    want, bound = fr.zscore_want(name)
    for nb in sorted({c["nb"], fr.zs_blocks(len(c["a"]), 80)}):         # fewer blocks: longer runs, shorter tail; never deeper
        got = fr.emulate_zscore_kernel(c["a"], c["b"], nb, np.float64)
        r, i = fr.worst_ratio(got, want, bound)
        assert r <= 1.0, (name, nb, r, np.unravel_index(i, want.shape))


@pytest.mark.parametrize("name", list(ZS_CASES))
def test_zscore_cases_are_well_conditioned(name):
    """The fp64 term stays 100 times under the fp32 half-ulp (at |z| = 1) in every column under the accuracy contract; the spread
    and the condition number each column ended with are part of the case (DESIGN.md lists them)."""
    c = ZS_CASES[name]
    for j in range(2):
        if c["accuracy"][j]:
            assert c["margin"][j] >= fr.MARGIN, (name, j, c["kappa"][j], c["margin"][j])
            assert np.isfinite(c["kappa"][j]) and c["kappa"][j] >= 1.0
    print(f"{name}: nb {c['nb']} spread {c['spread']} kappa ({c['kappa'][0]:.3g}, {c['kappa'][1]:.3g}) "
          f"margin ({c['margin'][0]:.3g}, {c['margin'][1]:.3g})")


def test_zscore_matrix_reaches_narrow_bands():
    """The matrix is not only easy columns: some column has mean / std above 100 (kappa > 1e4), and at the clamp-crossing size
    some column has kappa > 500."""
    assert max(max(k for k, a in zip(c["kappa"], c["accuracy"]) if a) for c in ZS_CASES.values()) > 1e4
    big = [c for c in ZS_CASES.values() if len(c["a"]) == fr.ZS_E[-1]]
    assert max(max(c["kappa"]) for c in big) > 500


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def _pagerank_mutant(src, dst, n, pe_dim, alpha, kind):
    """fp32 [n, 2 + pe_dim] of a kernel that is wrong in one way."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    out_deg = np.bincount(src, minlength=n).astype(np.float64)
    in_deg = np.bincount(dst, minlength=n).astype(np.float64)
    dinv = 1.0 / (out_deg + 1e-9)
    if kind != "dinv not zeroed":
        dinv[out_deg < 1e-9] = 0.0
    teleport = (1.0 - alpha) if kind == "teleport not over n" else (1.0 - alpha) / n
    x = np.full(n, 1.0 / n)
    cols = [x]
    for _ in range(pe_dim):
        lost = x[out_deg < 1e-9].sum() / n if kind == "dangling mass handed back" else 0.0
        x = alpha * (np.bincount(dst, weights=dinv[src] * x[src], minlength=n) + lost) + teleport
        cols.append(x)
    cols = cols[:-1] if kind == "columns shifted by one" else cols[1:]
    deg = [out_deg, in_deg] if kind == "degrees swapped" else [in_deg, out_deg]
    return np.stack(deg + cols, 1).astype(np.float32)


PR_MUTANTS = ("teleport not over n", "columns shifted by one", "degrees swapped", "dangling mass handed back")


def _pr_fails(name, kind):
    src, dst, n, pe_dim, alpha = PR_CASES[name]
    want, bound = fr.pagerank_want(name)
    got = _pagerank_mutant(src, dst, n, pe_dim, alpha, kind)
    return not np.array_equal(got[:, :2], want[:, :2]) or fr.worst_ratio(got, want, bound)[0] > 1.0


def test_the_mutant_helper_without_a_mutation_is_the_oracle():
    for name in ("tiny (5 nodes)", "small graph, pe_dim=16", "no out-edge | no in-edge | isolated"):
        assert not _pr_fails(name, None)


@pytest.mark.parametrize("kind", PR_MUTANTS)
def test_pagerank_mutants_miss_the_bar(kind):
    caught = [name for name in PR_CASES if _pr_fails(name, kind)]
    print(f"{kind}: caught by {len(caught)} of {len(PR_CASES)} cases: {caught}")
    assert caught, f"PageRank mutant '{kind}' passes every case: the matrix has a hole"


def test_unzeroed_dinv_is_unobservable():
    """dinv[u] is read once per OUT-edge of u: where there is none, its value (0, or 1 / 1e-9 when the `outdeg < 1e-9` branch is
    dropped) reaches no sum.  The mutant's output equals the oracle's bit for bit on every case, the one built for it included
    (a third of the nodes without out-edges): no per-element bar can tell the two apart, and none needs to."""
    for name, (src, dst, n, pe_dim, alpha) in PR_CASES.items():
        if n > 100000:
            continue
        want, _ = fr.pagerank_want(name)
        assert np.array_equal(_pagerank_mutant(src, dst, n, pe_dim, alpha, "dinv not zeroed"), want.astype(np.float32)), name
    src, dst, n, _, _ = PR_CASES["no out-edge | no in-edge | isolated"]
    assert (np.bincount(src, minlength=n) == 0).sum() >= n // 3


ZS_MUTANTS = {"fp32 accumulation": dict(acc_dtype=np.float32), "biased std (/ n)": dict(acc_dtype=np.float64, ddof=0)}


@pytest.mark.parametrize("kind", list(ZS_MUTANTS))
def test_zscore_mutants_miss_the_bar(kind):
    caught = []
    for name, c in ZS_CASES.items():
        want, bound = fr.zscore_want(name)
        got = fr.emulate_zscore_kernel(c["a"], c["b"], c["nb"], **ZS_MUTANTS[kind])
        if fr.worst_ratio(got, want, bound)[0] > 1.0:
            caught.append(name)
    print(f"{kind}: caught by {len(caught)} of {len(ZS_CASES)} cases: {caught}")
    assert caught, f"z-score mutant '{kind}' passes every case: the matrix has a hole"
    if kind == "biased std (/ n)":
        assert len(caught) == len(ZS_CASES)                # 1 / (2 n) relative at the least: 1e-6 at the largest E, 30 half-ulps
