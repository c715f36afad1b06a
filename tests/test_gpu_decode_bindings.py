"""GPU: what the Python bindings of the decode stages promise around their kernels, pinned on one 6-node, 8-edge graph over a
3-read store: the exception type and the FULL message of every argument rule of engine.py's wrappers from bce_with_logits_counts
to optim_step (nothing is launched: sentinel-filled records and outputs stay as they were), and the C-ABI calls each decode
entry point makes (engine.profile_ops), with results equal to the plain-Python yardsticks of tests/*_reference.py.  Integers and
bytes throughout: every case asserts EQUALITY, there is no tolerance in this file."""
import numpy as np
import pytest
import torch

import align_reference as A
import bog_reference as B
import cover_reference as R
import reduce_reference as T
import seq_reference as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, E = 6, 8
SRC, DST = [0, 2, 2, 4, 4, 1, 0, 5], [1, 1, 3, 3, 5, 2, 2, 0]
SCORES = np.array([5, 4, 3, 3.5, 4.5, .5, 2, 1], np.float32)     # the cover needs rounds of 3, 2 and 0 links: 4 -> 5 -> 0 -> 1 -> 2 -> 3
LABELS = np.array([1, 0, 1, 0, 1, 1, 0, 1], np.float32)
PREFIX = np.array([10, 12, 9, 11, 13, 10, 25, 8], np.int64)        # 0 -> 2 (25) is explained by 0 -> 1 -> 2 (10 + 10): reduced
READS = ["ACGTTGCAAGGCTTAACCGGATATCGCGTTAACCGGTTAA", "TTGACCATGGCATCGATTGCAAGCTTAGGCCATAT",
         "GGCATTACGGATCCATGCAAGTCGATCGGATTACAGGCATCGATCCGGAA"]
READ_LEN = np.array([len(READS[v >> 1]) for v in range(N)], np.int64)
K = 20                                                             # junction_identity's max_errors


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(DEV)


@pytest.fixture(scope="module")
def world(lib):
    """The graph, its tensors and the store on the device, made once and never written to."""
    from gnnome_assembly_amd import AssemblyGraph
    from gnnome_assembly_amd.reads import ReadStore
    g = AssemblyGraph(np.asarray(SRC, np.int32), np.asarray(DST, np.int32), N).to(DEV)
    host = ReadStore.from_sequences(READS).validate()
    return dict(g=g, idx=g.index(), sc=_t(SCORES, np.float32), y=_t(LABELS, np.float32), pl=_t(PREFIX, np.int64),
                rl=_t(READ_LEN, np.int64), src=_t(SRC, np.int32), dst=_t(DST, np.int32), host=host, store=host.to(DEV))


# ---- 1. the messages ---------------------------------------------------------------------------------------------------------------
def _full(m, dt, value=-7):
    return torch.full((m,), value, dtype=dt, device=DEV)


def _calls(w):
    """name -> (function, its arguments by name in call order): every argument valid, records filled with 77 and outputs with -7."""
    from gnnome_assembly_amd import engine
    i32, i64, f32, u8 = torch.int32, torch.int64, torch.float32, torch.uint8
    st = w["store"]
    store = dict(base_off=st.base_off, length=st.length, packed=st.packed)
    P = N                                                          # one contig of all six nodes
    align = dict(src=w["src"], dst=w["dst"], prefix_length=w["pl"], n=N, **store, max_errors=K, dist=_full(E, i32),
                 overlap_length=_full(E, i64), similarity=_full(E, f32), rec=_full(8, i64, 77))
    flat = lambda: _full(E, f32, 0.5)                              # noqa: E731
    return {
        "bce_with_logits_counts": (engine.bce_with_logits_counts, dict(scores=w["sc"], y=w["y"], pos_weight=1.0,
                                                                       need_grad=False, epoch_acc=_full(6, i64, 77))),
        "sym_bce": (engine.sym_bce, dict(org=w["sc"], rev=w["sc"].clone(), y=w["y"], pos_weight=1.0, alpha=0.1, need_grad=False,
                                         want_counts=False, epoch_acc=_full(6, i64, 77))),
        "mirror_add": (engine.mirror_add, dict(g=flat(), scratch_grad=flat(), pi=_t(np.arange(E), np.int32))),
        "mirror_gather": (engine.mirror_gather, dict(src=flat(), pi=_t(np.arange(E), np.int32), out=flat())),
        "rank_hist": (engine.rank_hist, dict(scores=w["sc"], y=w["y"], record=_full(engine.RANK_RECORD_WORDS, i64, 77))),
        "decision_stats": (engine.decision_stats, dict(idx=w["idx"], scores=w["sc"], y=w["y"], record=_full(15, i64, 77),
                                                       best_succ=_full(N, i32), best_pred=_full(N, i32))),
        "bog_contigs": (engine.bog_contigs, dict(
            src=w["src"], dst=w["dst"], best_succ=_full(N, i32, -1), best_pred=_full(N, i32, -1), scores=w["sc"], y=w["y"],
            prefix_length=w["pl"], read_length=w["rl"], record=_full(8, i64, 77), contig_ptr=_full(N + 1, i32),
            walk_nodes=_full(N, i32), walk_edges=_full(N, i32), contig_bases=_full(N, i64), contig_wrong=_full(N, i32))),
        "cover_rounds": (engine.cover_rounds, dict(idx=w["idx"], scores=w["sc"], round_links=_full(2, i64), link_succ=_full(N, i32),
                                                   link_pred=_full(N, i32),
                                                   ws=_full(engine.cover_workspace_bytes(N), u8, 7))),
        "transitive_support": (engine.transitive_support, dict(
            idx=w["idx"], scores=w["sc"], prefix_length=w["pl"], y=w["y"], min_logit=float("-inf"), fuzz=None,
            support=_full(E, i32), masked_scores=_full(E, f32), rec=_full(8, i64, 77))),
        "seq_layout": (engine.seq_layout, dict(
            contig_ptr=_t([0, P], np.int32), walk_nodes=_t([4, 5, 0, 1, 2, 3], np.int32), walk_edges=_t([-1, 4, 7, 0, 5, 2], np.int32),
            prefix_length=w["pl"], n=N, **store, record=_full(8, i64, 77), piece_len=_full(P, i64), piece_off=_full(P + 1, i64),
            contig_base_ptr=_full(2, i64))),
        "seq_emit": (engine.seq_emit, dict(walk_nodes=_t([4, 5, 0, 1, 2, 3], np.int32), piece_off=_t(np.arange(P + 1), np.int64),
                                           n=N, **store, total=P, out=_full(16, u8, 7))),
        "overlap_align": (engine.overlap_align, align),
        "overlap_align_host": (engine.overlap_align_host, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in align.items()}),
        "optim_step": (engine.optim_step, dict(p=flat(), g=flat(), m=flat(), v=flat(), step=_full(1, f32, 0), stats=_full(4, i64, 77),
                                               ws=engine.optim_workspace(E, DEV).fill_(7), lr=1e-3, beta1=0.9, beta2=0.999,
                                               eps=1e-8)),
    }


def _dtype(t):
    return t.to({torch.int32: torch.int64, torch.int64: torch.int32, torch.float32: torch.float64, torch.uint8: torch.int8}[t.dtype])


def _longer(t):
    return torch.cat([t, t[:1]])


def _shorter(t):
    return t[:-1].clone()


def _strided(t):
    return torch.repeat_interleave(t, 2)[::2]                      # the same elements at a stride of two


def _index(key, how):
    return lambda idx: dict(idx, **{key: how(idx[key]) if key in idx else how(torch.arange(N, dtype=torch.int32, device=DEV))})


RANK_WORDS = 2 * 16384 + 4
ARG = "{fn}: {name} must be a contiguous {dt} [{m}] tensor"
INDEX = "{fn}: the index arrays must be contiguous int32 tensors (graph.index())"
EPOCH = "epoch_acc: a contiguous int64 [6] tensor (train.EpochStats.buf)"
# (wrapper, argument, what is wrong with it, the message); every row raises ValueError
ROWS = [
    ("bce_with_logits_counts", "epoch_acc", _shorter, EPOCH),
    ("bce_with_logits_counts", "epoch_acc", _dtype, EPOCH),
    ("sym_bce", "epoch_acc", _strided, EPOCH),
    ("sym_bce", "rev", _shorter, "sym_bce: 8 original scores, 7 reversed scores, 8 labels"),
    ("mirror_add", "pi", _dtype, "mirror_add: contiguous float32 buffers and an int32 permutation of 8 elements each"),
    ("mirror_add", "scratch_grad", _strided, "mirror_add: contiguous float32 buffers and an int32 permutation of 8 elements each"),
    ("mirror_gather", "out", _longer,
     "mirror_gather: contiguous float32 buffers (out is not src) and an int32 permutation of 8 elements each"),
    ("rank_hist", "record", _shorter, f"rank_hist: record must be a contiguous int64 [{RANK_WORDS}] tensor (train.RankingStats.buf)"),
    ("rank_hist", "record", _dtype, f"rank_hist: record must be a contiguous int64 [{RANK_WORDS}] tensor (train.RankingStats.buf)"),
    ("rank_hist", "y", _shorter, "rank_hist: 8 scores, 7 labels"),
    ("decision_stats", "record", _shorter, "decision_stats: record must be a contiguous int64 [15] tensor (train.DecisionStats.buf)"),
    ("decision_stats", "record", _strided, "decision_stats: record must be a contiguous int64 [15] tensor (train.DecisionStats.buf)"),
    ("decision_stats", "best_succ", _dtype, ARG.format(fn="decision_stats", name="best_succ", dt="int32", m=6)),
    ("decision_stats", "best_pred", _strided, ARG.format(fn="decision_stats", name="best_pred", dt="int32", m=6)),
    ("decision_stats", "best_pred", _longer, ARG.format(fn="decision_stats", name="best_pred", dt="int32", m=6)),
    ("decision_stats", "y", _longer, "decision_stats: 8 scores, 9 labels"),
    ("decision_stats", "scores", _shorter, "decision_stats: 7 scores for an index of 8 edges"),
    ("decision_stats", "idx", _index("out_pos", _dtype), INDEX.format(fn="decision_stats")),
    ("decision_stats", "idx", _index("idst", _strided), INDEX.format(fn="decision_stats")),
    ("bog_contigs", "record", _shorter, "bog_contigs: record must be a contiguous int64 [8] tensor"),
    ("bog_contigs", "src", _dtype, ARG.format(fn="bog_contigs", name="src", dt="int32", m=8)),
    ("bog_contigs", "best_succ", _dtype, ARG.format(fn="bog_contigs", name="best_succ", dt="int32", m=6)),
    ("bog_contigs", "best_pred", _strided, ARG.format(fn="bog_contigs", name="best_pred", dt="int32", m=6)),
    ("bog_contigs", "prefix_length", _dtype, ARG.format(fn="bog_contigs", name="prefix_length", dt="int64", m=8)),
    ("bog_contigs", "read_length", _shorter, ARG.format(fn="bog_contigs", name="read_length", dt="int64", m=6)),
    ("bog_contigs", "contig_ptr", _shorter, ARG.format(fn="bog_contigs", name="contig_ptr", dt="int32", m=7)),
    ("bog_contigs", "walk_nodes", _dtype, ARG.format(fn="bog_contigs", name="walk_nodes", dt="int32", m=6)),
    ("bog_contigs", "walk_edges", _strided, ARG.format(fn="bog_contigs", name="walk_edges", dt="int32", m=6)),
    ("bog_contigs", "contig_bases", _strided, ARG.format(fn="bog_contigs", name="contig_bases", dt="int64", m=6)),
    ("bog_contigs", "contig_wrong", _longer, ARG.format(fn="bog_contigs", name="contig_wrong", dt="int32", m=6)),
    ("bog_contigs", "y", _shorter, "bog_contigs: 8 scores, 7 labels"),
    ("bog_contigs", "scores", _shorter, "bog_contigs: 8 src entries, 8 dst entries, 7 scores"),
    ("bog_contigs", "dst", _shorter, "bog_contigs: 8 src entries, 7 dst entries, 8 scores"),
    ("cover_rounds", "link_succ", _dtype, ARG.format(fn="cover_rounds", name="link_succ", dt="int32", m=6)),
    ("cover_rounds", "link_pred", _shorter, ARG.format(fn="cover_rounds", name="link_pred", dt="int32", m=6)),
    ("cover_rounds", "round_links", _dtype, "cover_rounds: round_links must be a contiguous int64 [rounds] tensor"),
    ("cover_rounds", "scores", _longer, "cover_rounds: 9 scores for an index of 8 edges"),
    ("cover_rounds", "idx", _index("isrc", _dtype), INDEX.format(fn="cover_rounds")),
    ("cover_rounds", "idx", _index("nperm", _dtype), INDEX.format(fn="cover_rounds")),
    ("cover_rounds", "idx", _index("nperm", _longer), INDEX.format(fn="cover_rounds")),
    ("transitive_support", "rec", _longer, "transitive_support: rec must be a contiguous int64 [8] tensor"),
    ("transitive_support", "prefix_length", _strided, ARG.format(fn="transitive_support", name="prefix_length", dt="int64", m=8)),
    ("transitive_support", "support", _dtype, ARG.format(fn="transitive_support", name="support", dt="int32", m=8)),
    ("transitive_support", "masked_scores", _dtype, ARG.format(fn="transitive_support", name="masked_scores", dt="float32", m=8)),
    ("transitive_support", "masked_scores", _shorter, ARG.format(fn="transitive_support", name="masked_scores", dt="float32", m=8)),
    ("transitive_support", "y", _shorter, "transitive_support: 8 scores, 7 labels"),
    ("transitive_support", "scores", _shorter, "transitive_support: 7 scores for an index of 8 edges"),
    ("transitive_support", "idx", _index("out_ptr", _dtype), INDEX.format(fn="transitive_support")),
    ("transitive_support", "idx", _index("nperm", _strided), INDEX.format(fn="transitive_support")),
    ("seq_layout", "record", _longer, "seq_layout: record must be a contiguous int64 [8] tensor"),
    ("seq_layout", "base_off", _dtype, ARG.format(fn="seq_layout", name="base_off", dt="int64", m=3)),
    ("seq_layout", "length", _shorter, ARG.format(fn="seq_layout", name="length", dt="int64", m=3)),
    ("seq_layout", "packed", _dtype, ARG.format(fn="seq_layout", name="packed", dt="uint8", m="{packed}")),
    ("seq_layout", "walk_nodes", _dtype, ARG.format(fn="seq_layout", name="walk_nodes", dt="int32", m=6)),
    ("seq_layout", "walk_edges", _shorter, ARG.format(fn="seq_layout", name="walk_edges", dt="int32", m=6)),
    ("seq_layout", "piece_len", _strided, ARG.format(fn="seq_layout", name="piece_len", dt="int64", m=6)),
    ("seq_layout", "piece_off", _shorter, ARG.format(fn="seq_layout", name="piece_off", dt="int64", m=7)),
    ("seq_layout", "contig_base_ptr", _dtype, ARG.format(fn="seq_layout", name="contig_base_ptr", dt="int64", m=2)),
    ("seq_emit", "walk_nodes", _dtype, ARG.format(fn="seq_emit", name="walk_nodes", dt="int32", m=6)),
    ("seq_emit", "piece_off", _shorter, ARG.format(fn="seq_emit", name="piece_off", dt="int64", m=7)),
    ("seq_emit", "out", _strided, ARG.format(fn="seq_emit", name="out", dt="uint8", m=16)),
    ("seq_emit", "length", _strided, ARG.format(fn="seq_emit", name="length", dt="int64", m=3)),
    ("overlap_align", "rec", _shorter, "overlap_align: rec must be a contiguous int64 [8] tensor"),
    ("overlap_align", "src", _strided, ARG.format(fn="overlap_align", name="src", dt="int32", m=8)),
    ("overlap_align", "dst", _dtype, ARG.format(fn="overlap_align", name="dst", dt="int32", m=8)),
    ("overlap_align", "prefix_length", _shorter, ARG.format(fn="overlap_align", name="prefix_length", dt="int64", m=8)),
    ("overlap_align", "dist", _dtype, ARG.format(fn="overlap_align", name="dist", dt="int32", m=8)),
    ("overlap_align", "overlap_length", _longer, ARG.format(fn="overlap_align", name="overlap_length", dt="int64", m=8)),
    ("overlap_align", "similarity", _dtype, ARG.format(fn="overlap_align", name="similarity", dt="float32", m=8)),
    ("overlap_align", "base_off", _dtype, ARG.format(fn="overlap_align", name="base_off", dt="int64", m=3)),
    ("overlap_align_host", "rec", _dtype, "overlap_align_host: rec must be a contiguous int64 [8] tensor"),
    ("overlap_align_host", "dist", _longer, ARG.format(fn="overlap_align_host", name="dist", dt="int32", m=8)),
    ("optim_step", "stats", _shorter, "optim_step: stats must be a contiguous int64 [4] tensor"),
    ("optim_step", "stats", _dtype, "optim_step: stats must be a contiguous int64 [4] tensor"),
    ("optim_step", "g", _shorter, "optim_step: g must be a contiguous float32 tensor of 8 elements"),
    ("optim_step", "v", _strided, "optim_step: v must be a contiguous float32 tensor of 8 elements"),
]
# NEW with the shared index rule: decision_stats used to take an index whose node permutation was no int32 [n] tensor as it came
NEW_ROWS = [("decision_stats", "idx", _index("nperm", _dtype), INDEX.format(fn="decision_stats")),
            ("decision_stats", "idx", _index("nperm", _longer), INDEX.format(fn="decision_stats"))]


def _tensors(args):
    out = []
    for v in args.values():
        out += [v] if torch.is_tensor(v) else list(v.values()) if isinstance(v, dict) else []
    return out


@pytest.mark.parametrize("row", range(len(ROWS) + len(NEW_ROWS)))
def test_a_wrong_argument_raises_its_message_and_launches_nothing(world, row):
    fn, name, how, message = (ROWS + NEW_ROWS)[row]
    call, args = _calls(world)[fn]
    before = [(t, t.clone()) for t in _tensors(args)]
    bad = dict(args, **{name: how(args[name])})
    assert bad[name] is not args[name]
    with pytest.raises(ValueError) as ei:
        call(*bad.values())
    torch.cuda.synchronize()
    assert str(ei.value) == message.format(packed=world["store"].packed.numel()), (fn, name, str(ei.value))
    assert type(ei.value) is ValueError and all(torch.equal(t, was) for t, was in before), (fn, name)


# ---- 2. the launches ---------------------------------------------------------------------------------------------------------------
def _ops(fn):
    """(fn(), {op: calls}) of the C-ABI calls fn makes."""
    from gnnome_assembly_amd import engine
    engine.profile_ops(True)
    try:
        out = fn()
    finally:
        ops = engine.profile_ops(False)
    return out, {k: v[0] for k, v in ops.items()}


def _contig_arrays(c):
    h = c.host()
    out = {k: h[k].astype(np.int64) for k in ("contig_ptr", "walk_nodes", "walk_edges", "bases", "wrong")}
    out["record"] = np.asarray(c.stats.words(), np.int64)
    return out


def _same_contigs(c, want, cover, reduce_record=None):
    got = _contig_arrays(c)
    for k in got:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, got[k], want[k])
    if cover:
        assert np.array_equal(c.link_succ.cpu().numpy(), want["link_succ"]) and np.array_equal(c.link_pred.cpu().numpy(), want["link_pred"])
        assert (c.rounds, list(c.round_links), c.converged) == (want["rounds"], want["round_links"], want["converged"])
    else:
        assert not hasattr(c, "rounds") and not hasattr(c, "link_succ")
    if reduce_record is None:
        assert not hasattr(c, "reduce_stats")
    else:
        assert c.reduce_stats.words() == reduce_record.tolist()


def test_the_cover_decoders_make_the_calls_they_made_and_equal_the_references(world):
    from gnnome_assembly_amd import decode
    w = world
    ref = (SRC, DST, N, SCORES, PREFIX, READ_LEN, LABELS)
    args = (w["g"], w["sc"], w["pl"], w["rl"], w["y"])
    c, ops = _ops(lambda: decode.best_overlap_contigs(*args))
    assert ops == {"gnm_decision_stats": 1, "gnm_bog_contigs": 1}
    _same_contigs(c, B.contigs(*ref), cover=False)
    c, ops = _ops(lambda: decode.best_overlap_contigs(*args, reduce_transitive=True))
    assert ops == {"gnm_transitive_support": 1, "gnm_decision_stats": 1, "gnm_bog_contigs": 1}
    want = T.cover(*ref, best_overlap=True)
    _same_contigs(c, want, cover=False, reduce_record=want["reduce_record"])
    c, ops = _ops(lambda: decode.greedy_cover_contigs(*args, check_every=2))
    want = R.contigs(*ref)
    assert want["round_links"] == [3, 2, 0] and ops == {"gnm_cover_rounds": 2, "gnm_bog_contigs": 1}     # chunks of rounds 0-1, 2-3
    _same_contigs(c, want, cover=True)
    c, ops = _ops(lambda: decode.greedy_cover_contigs(*args, check_every=1))
    assert ops == {"gnm_cover_rounds": 3, "gnm_bog_contigs": 1}
    _same_contigs(c, want, cover=True)
    c, ops = _ops(lambda: decode.greedy_cover_contigs(*args, reduce_transitive=True))
    want = T.cover(*ref)
    assert want["round_links"] == [4, 1, 0] and ops == {"gnm_transitive_support": 1, "gnm_cover_rounds": 1, "gnm_bog_contigs": 1}
    _same_contigs(c, want, cover=True, reduce_record=want["reduce_record"])
    r, ops = _ops(lambda: decode.transitive_support(w["g"], w["sc"], w["pl"], w["y"]))
    want = T.reduce(SRC, DST, N, SCORES, PREFIX, LABELS)
    assert ops == {"gnm_transitive_support": 1} and r.stats.words() == want["record"].tolist() == [8, 8, 1, 0, 1, 1, 0, 1]
    assert np.array_equal(r.support.cpu().numpy(), want["support"])
    assert np.array_equal(r.masked_scores.cpu().numpy().view(np.uint32), want["masked_bits"])


def test_sequences_and_junctions_make_the_calls_they_made_and_equal_the_references(world):
    from gnnome_assembly_amd import decode
    w = world
    cover = decode.greedy_cover_contigs(w["g"], w["sc"], w["pl"], w["rl"], w["y"])
    walks, wedges = [[4, 5, 0, 1, 2, 3]], [[-1, 4, 7, 0, 5, 2]]
    assert cover.walks() == walks
    want, rec = S.contig_strings(walks, wedges, PREFIX, READS)
    for what in (cover, walks):                                       # the device CSR as it is; lists, edge ids looked up on the host
        seqs, ops = _ops(lambda: decode.contig_sequences(what, w["g"], w["store"], w["pl"], w["rl"]))
        assert ops == {"gnm_seq_layout": 1, "gnm_seq_emit": 1}
        assert [seqs.sequence(c) for c in range(len(seqs))] == want and seqs.record.words() == [rec[k] for k in S.COUNTERS]
        assert seqs.contig_ptr.dtype == torch.int64 and seqs.piece_off.tolist() == np.cumsum([0] + seqs.piece_len.tolist()).tolist()
    dist, olen, sim, arec = A.overlap_align(w["host"], N, SRC, DST, PREFIX, K)
    edges = wedges[0][1:]
    for what in (cover, walks):
        ji, ops = _ops(lambda: decode.junction_identity(what, w["g"], w["store"], K, w["pl"]))
        assert ops == {"gnm_overlap_align": 1}
        assert (ji.junctions.tolist(), ji.edit_distance.tolist(), ji.exceeded.tolist()) == \
            ([5], [int(dist[edges].sum())], [int((dist[edges] > K).sum())])
        assert ji.junctions.dtype == torch.int64 and np.array_equal(ji.features.edit_distance.cpu().numpy(), dist)
        assert [getattr(ji.features.stats, k) for k in A.COUNTERS] == arec.tolist() and np.array_equal(ji.features.overlap_length.cpu().numpy(), olen)
