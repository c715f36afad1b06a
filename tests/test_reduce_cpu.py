"""CPU: the transitive-reduction yardstick (tests/reduce_reference.py) against cases written out by hand and against the two
properties the strict prefix comparison gives -- no two edges remove each other through one another, and a node's candidate
out-edge of uniquely smallest prefix is never reduced; the binding of gnm_transitive_support and its host-side argument checks; the
refusals of decode.transitive_support, the three decoders' new arguments, metrics.AssemblyStats and the two hyper-parameters.
Integers and bit patterns throughout, compared for equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import reduce_reference as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


# ---- 1. the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", T.HAND, ids=[r[0] for r in T.HAND])
def test_hand_cases(row):
    src, dst, n, sc, pl, ml, fuzz, support, reduced = T.hand_case(row)
    r = T.reduce(src, dst, n, sc, pl, None, ml, fuzz)
    assert r["support"].tolist() == support.tolist() and r["reduced"].tolist() == reduced.tolist()
    bits = sc.view(np.uint32).copy()
    bits[reduced] = 0x7FC00000
    assert r["masked_bits"].tolist() == bits.tolist()
    loops = int((src == dst).sum())
    assert r["record"].tolist() == [src.size, int(r["candidate"].sum()), int(reduced.sum()), 0, int(support.sum()), int(support.max()),
                                    loops, 1]
    assert T.no_mutual_removal(r) and T.shortest_out_edge_survives(src, pl, r)


def test_the_record_counts_labels_and_an_empty_graph_counts_nothing():
    src, dst, n, sc, pl, ml, fuzz, support, reduced = T.hand_case(T.HAND[0])
    assert T.reduce(src, dst, n, sc, pl, [0, 0, 1], ml, fuzz)["record"].tolist() == [3, 3, 1, 1, 1, 1, 0, 1]
    assert T.reduce(src, dst, n, sc, pl, [1, 1, NAN], ml, fuzz)["record"].tolist() == [3, 3, 1, 0, 1, 1, 0, 1]
    e = np.zeros(0, np.int32)
    for m in (0, 4):
        r = T.reduce(e, e, m, np.zeros(0, np.float32), np.zeros(0, np.int64))
        assert r["record"].tolist() == [0] * 8 and r["support"].size == 0


def test_the_fuzz_sum_wraps_like_int64():
    """The kernel's arithmetic, not Python's: -2^63 + -2^63 - 0 is -2^64, which wraps to 0 and passes fuzz = 0.  Stated so that the
    yardstick and the kernel agree on every input; real prefixes are nowhere near."""
    low = -2 ** 63
    r = T.reduce([0, 1, 0], [1, 2, 2], 3, [1, 1, 1], [low, low, 0], None, -INF, 0)
    assert r["support"].tolist() == [0, 0, 1]
    r = T.reduce([0, 1, 0], [1, 2, 2], 3, [1, 1, 1], [low, low + 1, 0], None, -INF, 0)
    assert r["support"].tolist() == [0, 0, 0]                     # wraps to +1


def _graphs():
    from gnnome_assembly_amd import synth
    src, dst, n = synth.tiny_edge_case_graph()
    rng = np.random.default_rng(5)
    yield "tiny", src, dst, n, rng.integers(1, 40, src.size).astype(np.int64), rng
    src, dst, n = synth.make_graph(300, seed=3)
    yield "synth", src, dst, n, T.synth_prefixes(src, dst, n, 3, jitter=4)[0], rng


@pytest.mark.parametrize("fuzz", [None, 0, 6])
def test_the_two_properties_of_the_strict_comparison(fuzz):
    for name, src, dst, n, pl, rng in _graphs():
        sc = rng.standard_normal(src.size).astype(np.float32)
        sc[rng.random(src.size) < 0.05] = NAN
        for ml in (-INF, -0.5):
            r = T.reduce(src, dst, n, sc, pl, None, ml, fuzz)
            # the property is not vacuous (the tiny graph's random prefixes close no triangle within a few bases)
            assert r["record"][2] > 0 or (name == "tiny" and fuzz is not None), (name, fuzz, ml)
            assert T.no_mutual_removal(r), (name, fuzz, ml)
            assert T.shortest_out_edge_survives(src, pl, r), (name, fuzz, ml)
            assert not r["reduced"][~r["candidate"]].any() and (r["support"][src == dst] == 0).all()


def test_the_chain_keeps_its_nearest_neighbour_edges_and_the_cover_is_one_path_per_strand():
    src, dst, n, sc, pl, rl, near = T.chain(40, seed=2)
    r = T.reduce(src, dst, n, sc, pl, None, -INF, 0)
    assert ((r["support"] == 0) == near).all() and (r["reduced"] == ~near).all()
    c = T.cover(src, dst, n, sc, pl, rl, fuzz=0)
    assert np.diff(c["contig_ptr"]).tolist() == [40, 40] and c["reduce_record"].tolist() == r["record"].tolist()
    plain = T.R.contigs(src, dst, n, sc, pl, rl)
    assert plain["record"][0] > 2                                  # without the reduction the links jump over reads


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def _cpu_args():
    from gnnome_assembly_amd import AssemblyGraph
    g = AssemblyGraph(np.array([0, 1], np.int32), np.array([1, 2], np.int32), 3)
    return g, torch.zeros(2), torch.ones(2, dtype=torch.int64), torch.ones(3, dtype=torch.int64)


def test_the_decode_functions_refuse_a_cpu_graph_and_bad_arguments():
    from gnnome_assembly_amd import decode, engine
    from gnnome_assembly_amd._lib import GnmError
    g, sc, pl, rl = _cpu_args()
    assert {"transitive_support", "TransitiveSupport", "ReduceStats"} <= set(decode.__all__) and engine.REDUCE_RECORD_WORDS == 8
    assert engine.REDUCE_COUNTERS == T.COUNTERS
    assert tuple(decode.ReduceStats.__dataclass_fields__) == engine.REDUCE_COUNTERS and decode.ReduceStats(*range(8)).words() == list(range(8))
    with pytest.raises(GnmError, match="HIP device"):
        decode.transitive_support(g, sc, pl)
    for fn in (decode.best_overlap_contigs, decode.greedy_cover_contigs):
        with pytest.raises(GnmError, match="HIP device"):
            fn(g, sc, pl, rl, reduce_transitive=True, fuzz=0)
        for bad in (-1, 1.5, "3", True):
            with pytest.raises(ValueError, match="fuzz"):
                fn(g, sc, pl, rl, reduce_transitive=True, fuzz=bad)
        for bad in (1, None, "yes"):
            with pytest.raises(ValueError, match="reduce_transitive"):
                fn(g, sc, pl, rl, reduce_transitive=bad)
    for bad in (-1, 2.0, False):
        with pytest.raises(ValueError, match="fuzz"):
            decode.transitive_support(g, sc, pl, fuzz=bad)
    with pytest.raises(GnmError):
        engine.transitive_support(g.index(), sc, pl, None, -INF, None, torch.zeros(2, dtype=torch.int32), None,
                                  torch.zeros(8, dtype=torch.int64))
    st = decode.ReduceStats(10, 8, 2, 1, 3, 2, 1, 1)
    assert st.reduced_fraction == 0.25 and st.words() == [10, 8, 2, 1, 3, 2, 1, 1] and np.isnan(decode.ReduceStats().reduced_fraction)
    assert engine.reduce_fuzz_word(None) == -1 and engine.reduce_fuzz_word(np.int64(7)) == 7 and engine.reduce_fuzz_word(0) == 0


def test_infer_contigs_hands_the_switch_to_the_cover_decoders_only():
    from gnnome_assembly_amd import decode
    for kw in (dict(), dict(device_sampling=True)):
        with pytest.raises(ValueError, match="reduce_transitive=True with decoder='greedy'"):
            decode.infer_contigs(None, None, None, None, None, None, reduce_transitive=True, **kw)
    with pytest.raises(ValueError, match="fuzz"):
        decode.infer_contigs(None, None, None, None, None, None, decoder="greedy_cover", reduce_transitive=True, fuzz=-2)
    with pytest.raises(ValueError, match="reduce_transitive"):
        decode.infer_contigs(None, None, None, None, None, None, decoder="best_overlap", reduce_transitive="on")


def test_assembly_stats_arguments():
    from gnnome_assembly_amd import metrics as M
    st = M.AssemblyStats("cpu")
    assert st.reduce_transitive is False and st.fuzz is None and st.reduce_rec.tolist() == [0] * 8
    st = M.AssemblyStats("cpu", decoder="greedy_cover", reduce_transitive=True, fuzz=5)
    assert st.reduce_transitive is True and st.fuzz == 5
    with pytest.raises(ValueError, match="reduce_transitive"):
        M.AssemblyStats("cpu", reduce_transitive=1)
    for bad in (-1, 0.5, "0"):
        with pytest.raises(ValueError, match="fuzz"):
            M.AssemblyStats("cpu", reduce_transitive=True, fuzz=bad)


def test_hyperparameter_defaults_environment_and_validation(monkeypatch, tmp_path):
    from gnnome_assembly_amd import train as TR
    monkeypatch.delenv("GNM_ASSEMBLY_REDUCE", raising=False)
    hp = TR.get_hyperparameters()
    assert hp["assembly_reduce_transitive"] is False and hp["assembly_reduce_fuzz"] is None
    monkeypatch.setenv("GNM_ASSEMBLY_REDUCE", "1")
    assert TR.get_hyperparameters()["assembly_reduce_transitive"] is True
    monkeypatch.setenv("GNM_ASSEMBLY_REDUCE", "0")
    assert TR.get_hyperparameters()["assembly_reduce_transitive"] is False
    monkeypatch.delenv("GNM_ASSEMBLY_REDUCE")
    from loop_common import mix_sample, oracle_model_factory
    torch.set_num_threads(1)
    hooks = {"model_factory": oracle_model_factory,
             "criterion_factory": lambda pw: torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pw]))}
    for bad, word in ((dict(assembly_reduce_transitive=1), "assembly_reduce_transitive"),
                      (dict(assembly_reduce_transitive="1"), "assembly_reduce_transitive"),
                      (dict(assembly_reduce_fuzz=-1), "assembly_reduce_fuzz"), (dict(assembly_reduce_fuzz=2.5), "assembly_reduce_fuzz"),
                      (dict(assembly_reduce_fuzz=True), "assembly_reduce_fuzz")):
        with pytest.raises(ValueError, match=word):
            TR.train([mix_sample(40, 0)], [mix_sample(30, 1)], out="bad", workdir=str(tmp_path), verbose=False, hooks=hooks,
                     hyperparameters=dict(num_epochs=1, dim_latent=32, num_gnn_layers=1, **bad))
    assert not (tmp_path / "checkpoints").exists()


# ---- 3. the entry point --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def test_the_library_binds_the_entry_point_at_abi_7(lib):
    import __graft_entry__ as ge
    from gnnome_assembly_amd import _lib
    assert "gnm_reduce.hip" in ge.SOURCES
    name = "gnm_transitive_support"
    assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1] and len(_lib.SIGNATURES[name][1]) == 18
    assert lib.gnm_abi_version() == 7 == _lib.ABI_VERSION
    hdr = open(os.path.join(REPO, "include", "gnm.h")).read()
    assert "int gnm_transitive_support(" in hdr and "typedef struct gnm_reduce_record" in hdr and "#define GNM_ABI_VERSION 7" in hdr
    assert "gnm_reduce.hip" in open(os.path.join(REPO, "INTEGRATION.md")).read()
    src = open(os.path.join(REPO, "gnnome_assembly_amd", "csrc", "gnm_reduce.hip")).read()
    assert '#include "gnm_key.h"' in src and "unsigned dec_key_(float" not in src      # the key is shared, not copied


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Host-side returns: no device is touched (the checks run before the grid is even sized)."""
    n, E = 4, 8
    buf = (C.c_int64 * 16)()
    rec = (C.c_int64 * 9)()
    p = lambda a: C.c_void_p(C.addressof(a))                                     # noqa: E731
    b = p(buf)
    ok = dict(n=n, E=E, perm=b, isrc=b, in_ptr=b, out_ptr=b, out_pos=b, out_dst=b, nperm=None, scores=b, prefix_length=b, y=None,
              min_logit=0.0, fuzz=-1, support=b, masked_scores=None, record=p(rec), stream=None)
    for change, word in ((dict(n=-1), "n = -1"), (dict(E=-1), "E = -1"), (dict(n=2 ** 31 - 1), "2^31"), (dict(E=2 ** 31 - 1), "2^31"),
                         (dict(fuzz=-2), "fuzz = -2"), (dict(record=None), "record"),
                         (dict(record=C.c_void_p(C.addressof(rec) + 4)), "aligned"), (dict(out_ptr=None), "out_ptr"),
                         (dict(perm=None), "perm"), (dict(out_pos=None), "out_pos"), (dict(out_dst=None), "out_dst"),
                         (dict(scores=None), "scores"), (dict(prefix_length=None), "prefix_length"), (dict(support=None), "support"),
                         (dict(n=0, E=0, record=None), "record")):
        assert lib.gnm_transitive_support(*dict(ok, **change).values()) == -1, change
        assert word in lib.gnm_last_error().decode(), (change, lib.gnm_last_error())
    # nothing to do: valid, nothing launched, the record untouched
    for change in (dict(n=0, E=0), dict(n=4, E=0), dict(n=0, E=0, perm=None, out_ptr=None, out_pos=None, out_dst=None, scores=None,
                                                        prefix_length=None, support=None)):
        assert lib.gnm_transitive_support(*dict(ok, **change).values()) == 0, change
    assert all(v == 0 for v in rec) and all(v == 0 for v in buf)
