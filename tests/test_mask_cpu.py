"""Read-masking coverage augmentation, the tier without a GPU: the numpy restatement of the mask (tests/mask_reference.py) and its
properties, the library's plumbing (symbols, header, argument checks -- all refused on the host before any launch), the package's
host route against the restatement, the degrees' tensor restatement against bincount on the cases of tests/induce_cases.py, and
the training loop (train.train) with the CPU stand-in model of tests/loop_common.py."""
import os
import random
import re

import numpy as np
import pytest
import torch

import induce_cases as ic
import mask_reference as ref
from loop_common import mix_sample, oracle_model_factory

KEY = ref.mask_key(0x5EEDC0DE12345678)


# ---- 1. the restatement's properties --------------------------------------------------------------------------------------------
def test_both_strands_of_a_read_agree_and_the_ends_of_the_range():
    for n in (1, 2, 7, 8, 9, 4097):
        for f in (0.0, 0.3, 0.85, 1.0):
            m = ref.read_mask(n, f, KEY, 3, 1)
            assert m.dtype == bool and m.shape == (n,)
            assert np.array_equal(m[0:n - n % 2:2], m[1:n:2]), (n, f)
        assert ref.read_mask(n, 1.0, KEY, 3, 1).all() and not ref.read_mask(n, 0.0, KEY, 3, 1).any()


def test_prefix_nesting_and_what_the_mask_depends_on():
    base = ref.read_mask(4096, 0.5, KEY, 2, 5)
    for k in (1, 2, 7, 8, 1001):
        assert np.array_equal(ref.read_mask(4096 + k, 0.5, KEY, 2, 5)[:4096], base)          # the mask for N is a prefix
    assert np.all(ref.read_mask(4096, 0.4, KEY, 2, 5) <= base)                                # masks are nested in f
    assert not np.array_equal(ref.read_mask(4096, 0.5, KEY, 3, 5), base)                      # epoch
    assert not np.array_equal(ref.read_mask(4096, 0.5, KEY, 2, 6), base)                      # graph index
    assert not np.array_equal(ref.read_mask(4096, 0.5, KEY ^ 1, 2, 5), base)                  # key, low word
    assert not np.array_equal(ref.read_mask(4096, 0.5, KEY ^ (1 << 40), 2, 5), base)          # key, high word
    assert not np.array_equal(ref.read_mask(4096, 0.5, KEY, 5, 2), base)                      # the two counter words are not exchangeable


def test_kept_share_at_4096_reads():
    """4,096 reads at f = 0.85: the kept share within five binomial standard deviations (sqrt(.85 x .15 / 4096) = 0.0056)."""
    m = ref.read_mask(2 * 4096, 0.85, KEY, 0, 0)
    share = float(m[::2].mean())
    print(f"kept share {share:.4f}")
    assert abs(share - 0.85) <= 0.03


def test_the_mask_key_never_equals_the_dropout_key():
    from gnnome_assembly_amd import engine
    assert engine.READ_MASK_KEY_XOR == ref.KEY_XOR and ref.KEY_XOR % 2 == 1 and ref.KEY_XOR < 2 ** 64
    for seed in (0, 1, 2 ** 63 + 5):
        for rank in (0, 1, 7):
            assert engine.read_mask_key(seed, rank) == ref.mask_key(seed, rank) == engine.dropout_key(seed, rank) ^ ref.KEY_XOR
            assert engine.read_mask_key(seed, rank) != engine.dropout_key(seed, rank)


# ---- 2. library plumbing --------------------------------------------------------------------------------------------------------
def test_library_exports_and_argument_checks():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ge.REPO, "include", "gnm.h")).read()
    for name in ("gnm_read_mask", "gnm_index_degrees"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define\s+GNM_READ_MASK_KEY_XOR\s+0x%XULL" % ref.KEY_XOR, hdr)
    assert lib.gnm_abi_version() == 7 and _lib.ABI_VERSION == 7 and re.search(r"#define\s+GNM_ABI_VERSION\s+7\b", hdr)
    assert "gnm_mask.hip" in ge.SOURCES
    one = 1 << 12                                    # a non-null address that is never dereferenced: the checks fail first
    for f in (-0.01, 1.01, float("nan"), float("inf")):
        assert lib.gnm_read_mask(8, f, 1, 0, 0, one, None) < 0, f
        assert b"read_mask" in lib.gnm_last_error()
    assert lib.gnm_read_mask(-1, 0.5, 1, 0, 0, one, None) < 0
    assert lib.gnm_read_mask(8, 0.5, 1, 0, 0, None, None) < 0
    assert lib.gnm_read_mask(0, 0.5, 1, 0, 0, None, None) == 0 and lib.gnm_read_mask(0, 1.0, 1, 0, 0, one, None) == 0
    assert lib.gnm_index_degrees(-1, one, one, None, one, 18, None) < 0
    assert b"index_degrees" in lib.gnm_last_error()
    assert lib.gnm_index_degrees(4, one, one, None, one, 1, None) < 0            # ld < 2
    assert lib.gnm_index_degrees(4, None, one, None, one, 18, None) < 0
    assert lib.gnm_index_degrees(4, one, None, None, one, 18, None) < 0
    assert lib.gnm_index_degrees(4, one, one, None, None, 18, None) < 0
    assert lib.gnm_index_degrees(2 ** 31, one, one, None, one, 18, None) < 0
    assert lib.gnm_index_degrees(0, None, None, None, None, 18, None) == 0


# ---- 3. the package's host route ------------------------------------------------------------------------------------------------
def test_host_route_equals_the_restatement():
    from gnnome_assembly_amd import cluster
    for n in (0, 1, 2, 7, 8, 9, 2049):
        for f in (0.0, 0.5, 0.85, 1.0):
            for epoch, gi in ((0, 0), (3, 1), (2 ** 32 - 1, 7)):
                got = cluster.read_mask_host(n, f, KEY, epoch, gi)
                assert got.dtype == bool and np.array_equal(got, ref.read_mask(n, f, KEY, epoch, gi)), (n, f, epoch, gi)
    with pytest.raises(ValueError):
        cluster.read_mask_host(8, 1.5, KEY, 0, 0)


@pytest.mark.parametrize("node_order", ["keep", "bfs"])
def test_masked_subgraph_of_a_parent_on_the_cpu(node_order):
    """The thinned graph is induced_subgraph of the restatement's mask; pe is a copy with the thinned graph's degrees in columns 0
    and 1 and the parent's rows in the others; `select` is ANDed in; the parent is left alone."""
    from gnnome_assembly_amd import cluster
    src, dst, n, isolated = ic.random_graph(3, 300, 2000, True)
    g = ic.parent(src, dst, n, node_order)
    pe = torch.from_numpy(np.random.default_rng(0).standard_normal((n, 6)).astype(np.float32))
    g.ndata["pe"] = pe.clone()
    sel = ic.masks(src, dst, n, isolated)["block"]
    for f, select in ((0.85, None), (0.5, sel), (1.0, None), (0.0, None)):
        m = torch.from_numpy(ref.read_mask(n, f, KEY, 4, 2))
        want = cluster.induced_subgraph(g, m if select is None else m & select, "sort")
        for method in ("sort", "index"):
            sub = cluster.masked_subgraph(g, f, KEY, 4, 2, method, select=select)
            ws, wd = want.edges()
            s, d = sub.edges()
            ic.assert_same((sub.ndata[cluster.NID], sub.edata[cluster.EID], s, d, sub.index()),
                           (want.ndata[cluster.NID], want.edata[cluster.EID], ws, wd, want.index()), f"f = {f} {method}")
            ind, outd = ref.degrees(s.numpy(), d.numpy(), sub.num_nodes())
            got = sub.ndata["pe"]
            assert got.shape == (sub.num_nodes(), 6)
            assert np.array_equal(got[:, 0].numpy(), ind) and np.array_equal(got[:, 1].numpy(), outd)
            assert torch.equal(got[:, 2:], pe[sub.ndata[cluster.NID]][:, 2:])
            assert torch.equal(sub.ndata["x"], g.ndata["x"][sub.ndata[cluster.NID]])
            info = sub.relabel_info
            assert info["mask_fraction"] == f and info["mask_kept_nodes"] == sub.num_nodes() and info["mask"] == "host"
        assert torch.equal(g.ndata["pe"], pe)
    full = cluster.masked_subgraph(g, 1.0, KEY, 4, 2)
    assert full.num_nodes() == n and full.num_edges() == len(src)
    empty = cluster.masked_subgraph(g, 0.0, KEY, 4, 2)
    assert empty.num_nodes() == 0 and empty.num_edges() == 0 and empty.ndata["pe"].shape == (0, 6)


# ---- 4. degrees -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node_order,shuffle", [("bfs", True), ("keep", True), ("keep", False)])
def test_index_degrees_restatement_equals_bincount(node_order, shuffle):
    from gnnome_assembly_amd import cluster
    for seed, n, e in [(1, 300, 2000), (2, 97, 400)]:
        src, dst, n, isolated = ic.random_graph(seed, n, e, shuffle)
        g = ic.parent(src, dst, n, node_order)
        for name, mask in ic.masks(src, dst, n, isolated).items():
            _, _, s, d, idx, sub = ic.sort_route(g, mask)
            pe = torch.full((sub.num_nodes(), 5), 7.0)
            assert cluster.index_degrees_torch(idx, pe) is pe
            ind, outd = ref.degrees(s.numpy(), d.numpy(), sub.num_nodes())
            assert np.array_equal(pe[:, 0].numpy(), ind) and np.array_equal(pe[:, 1].numpy(), outd), (seed, name)
            assert bool((pe[:, 2:] == 7.0).all())


# ---- 5. the training loop -------------------------------------------------------------------------------------------------------
_HOOKS = {"model_factory": oracle_model_factory,
          "criterion_factory": lambda pw: torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw]))}
_HP = dict(num_epochs=2, dim_latent=32, num_gnn_layers=1, lr=1e-3, seed=0)


@pytest.fixture(scope="module")
def samples():
    torch.set_num_threads(1)
    return [mix_sample(r, s) for r, s in ((120, 0), (90, 1), (100, 2))], [mix_sample(40, 100)]


def _run(samples, tmp_path, name, **hp):
    from gnnome_assembly_amd import train as T
    tr, va = samples
    wd = tmp_path / name
    wd.mkdir()
    model, _, hist = T.train(tr, va, out=name, hyperparameters=dict(_HP, **hp), workdir=str(wd), verbose=False, hooks=_HOOKS)
    flat = torch.cat([p.detach().reshape(-1) for p in sorted(model.parameters(), key=lambda p: p._gnm_slot)])
    return hist, flat, random.getstate()


@pytest.fixture(scope="module")
def plain(samples, tmp_path_factory):
    return _run(samples, tmp_path_factory.mktemp("plain"), "plain")


def test_100_100_is_the_loop_without_the_keys(samples, plain, tmp_path):
    hist, flat, state = _run(samples, tmp_path, "off", mask_frac_low=100, mask_frac_high=100)
    assert hist == plain[0] and torch.equal(flat, plain[1]) and state == plain[2]
    assert hist.mask_fraction == [] and hist.masked_edges == []


def test_80_100_draws_per_step_from_a_private_generator(samples, plain, tmp_path):
    a = _run(samples, tmp_path, "a", mask_frac_low=80, mask_frac_high=100)
    b = _run(samples, tmp_path, "b", mask_frac_low=80, mask_frac_high=100)
    c = _run(samples, tmp_path, "c", mask_frac_low=80, mask_frac_high=100, seed=1)
    ha = a[0]
    assert len(ha.mask_fraction) == len(ha.step_graph) == len(ha.masked_edges) == 6
    assert all(0.80 <= f <= 1.00 and round(f * 100) == pytest.approx(f * 100) for f in ha.mask_fraction)
    assert ha.step_graph == plain[0].step_graph and a[2] == plain[2]          # the shuffle order and the global generator: untouched
    full = [s.graph.num_edges() for s in samples[0]]
    assert all(0 < e <= full[g] for e, g in zip(ha.masked_edges, ha.step_graph))
    assert any(e < full[g] for e, g in zip(ha.masked_edges, ha.step_graph)) and ha.step_losses != plain[0].step_losses
    assert ha == b[0] and torch.equal(a[1], b[1])
    assert c[0].mask_fraction != ha.mask_fraction
    assert all(np.isfinite(ha.loss_train)) and all(np.isfinite(ha.loss_valid))


def test_minibatch_mode_masks_every_batch(samples, tmp_path):
    hp = dict(batch_size_train=20, num_parts_metis_train=101, mask_frac_low=80, mask_frac_high=100, num_epochs=1)
    hist, _, _ = _run(samples, tmp_path, "mb", **hp)
    assert len(hist.mask_fraction) == len(hist.masked_edges) >= 3 and all(0.80 <= f <= 1.00 for f in hist.mask_fraction)
    assert np.isfinite(hist.loss_train[0])
    again, _, _ = _run(samples, tmp_path, "mb2", **hp)
    assert again == hist


def test_a_thinned_graph_without_edges_is_a_zero_contribution_step(samples, tmp_path):
    """A two-read graph whose four edges all join read 0 and read 1: at f = 0.5 it keeps both reads one time in four, and loses
    every edge otherwise (in this run: in all four epochs).  Such a step is a padding step (no forward, the collectives stay matched); the other graphs train, and the
    epochs complete.  Then f = 0.01 on every graph: about one read of a hundred survives, no two of them overlap, no step
    contributes at all -- and the epochs still complete."""
    from gnnome_assembly_amd import AssemblyGraph
    from gnnome_assembly_amd.train import GraphSample
    rng = np.random.default_rng(8)
    tiny = GraphSample(AssemblyGraph(np.array([0, 2, 1, 3]), np.array([2, 0, 3, 1]), 4),
                       torch.from_numpy(rng.standard_normal((4, 2)).astype(np.float32)),
                       torch.from_numpy(rng.standard_normal((4, 18)).astype(np.float32)), torch.tensor([1.0, 0.0, 1.0, 0.0]))
    tr, va = samples
    hist, flat, _ = _run((tr + [tiny], va), tmp_path, "some", mask_frac_low=50, mask_frac_high=50, num_epochs=4)
    print("masked_edges", hist.masked_edges)
    assert hist.mask_fraction == [0.5] * 16 and len(hist.masked_edges) == 16
    empty = sum(e == 0 for e in hist.masked_edges)
    assert 0 < empty <= 4 and len(hist.step_losses) == len(hist.step_graph) == 16 - empty
    assert len(hist.loss_train) == len(hist.loss_valid) == 4 and all(np.isfinite(hist.loss_train + hist.loss_valid))
    assert bool(torch.isfinite(flat).all())
    hist, flat, _ = _run(samples, tmp_path, "none", mask_frac_low=1, mask_frac_high=1)
    assert hist.mask_fraction == [0.01] * 6 and hist.masked_edges == [0] * 6 and hist.step_losses == []
    assert len(hist.loss_train) == 2 and hist.metrics_train == [None, None] and bool(torch.isfinite(flat).all())


@pytest.mark.parametrize("low,high", [(0, 100), (90, 80), (50, 101), (80.0, 100)])
def test_bad_fractions_are_refused(samples, tmp_path, low, high):
    with pytest.raises(ValueError, match="mask_frac"):
        _run(samples, tmp_path, "bad", mask_frac_low=low, mask_frac_high=high)
