"""GPU: the ground-truth label kernels (csrc/gnm_labels.hip) against the restatement of tests/labels_reference.py, by equality -- the
hand-made graphs and the simulated-position graphs of test_labels_cpu.py, in the caller's node numbering and in a renumbered index;
repeated runs and a round batch of 1 against the default, bit for bit; shapes that cross the kernels' own edges (chains longer than
one batch of rounds and than two workgroups, ids against starts, rows longer than a group's eight lanes); canaries round every
output; bad arguments; and reads -> find_overlaps -> label_overlap_graph -> prepare_graph -> GraphSample -> two training steps."""
import numpy as np
import pytest
import torch

import labels_reference as lref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build(verbose=False)
    from gnnome_assembly_amd import _lib
    return _lib.load()


def run(case, twin=None, node_order=None, batch=None):
    from gnnome_assembly_amd import AssemblyGraph, labels
    g = AssemblyGraph(case["src"], case["dst"], case["n"], node_order=node_order).to(DEV)
    t = None if twin is None else torch.from_numpy(twin)
    return labels.ground_truth_labels(g, *(torch.from_numpy(case[k]) for k in ("start", "end", "strand")), twin=t, rounds_per_batch=batch)


def check(got, want, what=""):
    assert got.y.device == DEV and got.y.dtype == torch.float32
    for k in ("y", "valid", "backbone", "component", "top"):
        np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), want[k], err_msg=f"{what}: {k}")
    assert {k: getattr(got.stats, k) for k in lref.COUNTERS} == want["stats"], what
    assert got.stats.invalid == 0 and got.stats.calls == 1


def same_bits(a, b):
    for k in ("y", "valid", "backbone", "component", "top"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.record.tolist() == b.record.tolist()


def hub():
    """a target with twelve predecessors (an in-row longer than a group's eight lanes) and a source with twelve successors"""
    reads = [(i, 100 + i) for i in range(12)] + [(60, 300)] + [(250 + i, 400 + i) for i in range(12)] + [(390, 500)]
    links = [(i, i + 1) for i in range(11)] + [(i, 12) for i in range(12)] + [(12, 13 + i) for i in range(12)] + \
            [(13 + i, 25) for i in range(0, 12, 2)]
    return lref.build(reads, links)


def shapes():
    from gnnome_assembly_amd import engine
    m = 3 * engine.GT_ROUNDS_PER_BATCH * engine.gt_sweeps() + 1
    return {"chain_batches": lref.chain(m), "chain_batches_reversed": lref.chain(m, reverse_ids=True),
            "chain_workgroups": lref.chain(600), "chain_workgroups_reversed": lref.chain(600, reverse_ids=True), "hub": hub()}


@pytest.mark.parametrize("name", list(lref.CASES))
def test_hand_made_cases_on_the_device(lib, name):
    case = lref.CASES[name]()
    want = lref.expected(name, case)
    check(run(case), want, name)
    check(run(case, node_order="bfs"), want, name + ", renumbered")
    tw = lref.twins(case)
    check(run(case, tw), lref.expected(name + "+twin", case, tw), name + ", twin")


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_simulated_read_positions_on_the_device(lib, seed):
    for drop in (True, False):
        case = lref.genome_case(seed, drop)
        want = lref.expected(f"genome{seed}{drop}", case)
        first = run(case)
        check(first, want, f"seed {seed}")
        same_bits(first, run(case))                                     # the same call again
        same_bits(first, run(case, batch=1))                            # one round per read-back
        check(run(case, node_order="bfs"), want, f"seed {seed}, renumbered")
        tw = lref.twins(case)
        check(run(case, tw), lref.expected(f"genome{seed}{drop}+twin", case, tw), f"seed {seed}, twin")


@pytest.mark.parametrize("name", ["chain_batches", "chain_batches_reversed", "chain_workgroups", "chain_workgroups_reversed", "hub"])
def test_shapes_that_cross_the_kernels_edges(lib, name):
    case = shapes()[name]
    want = lref.expected("shape " + name, case)
    got = run(case)
    check(got, want, name)
    assert want["stats"]["positives"] == want["stats"]["edges"] if name != "hub" else want["stats"]["positives"] > 24
    one = run(case, batch=1)
    same_bits(got, one)
    s = one.stats
    assert min(s.component_rounds, s.fwd_rounds, s.bwd_rounds) >= 1
    check(run(case, node_order="bfs"), want, name + ", renumbered")


def _buffers(n, E):
    """outputs with a canary element either side: (whole buffers, the views handed to the library)"""
    whole = [torch.full((E + 2,), 7.0, device=DEV), torch.full((E + 2,), 9, dtype=torch.uint8, device=DEV),
             torch.full((n + 2,), 9, dtype=torch.uint8, device=DEV), torch.full((n + 2,), -7, dtype=torch.int32, device=DEV),
             torch.full((n + 2,), -7, dtype=torch.int32, device=DEV)]
    return whole, [w[1:-1] for w in whole]


def _device_call(case, views, rec=None, **change):
    from gnnome_assembly_amd import AssemblyGraph, engine
    g = AssemblyGraph(case["src"], case["dst"], case["n"]).to(DEV)
    a = {k: torch.from_numpy(case[k]).to(DEV) for k in ("start", "end", "strand")}
    a.update(change)
    src, dst = (t.to(torch.int32).contiguous() for t in g.edges())
    rec = torch.zeros(engine.GT_RECORD_WORDS, dtype=torch.int64, device=DEV) if rec is None else rec
    return engine.gt_labels(g.index(DEV), src, dst, a["start"], a["end"], a["strand"], None, *views, rec)


def test_canaries_round_every_output(lib):
    case = lref.genome_case(23, False)
    n, E = case["n"], case["src"].size
    whole, views = _buffers(n, E)
    _device_call(case, views)
    torch.cuda.synchronize()
    want = lref.expected("genome23False", case)
    np.testing.assert_array_equal(views[0].cpu().numpy(), want["y"])
    np.testing.assert_array_equal(views[3].cpu().numpy(), want["component"])
    for w, c in zip(whole, (7.0, 9, 9, -7, -7)):
        assert w[0].item() == c and w[-1].item() == c


def test_bad_arguments_raise_and_leave_y_untouched(lib):
    case = lref.CASES["tip"]()
    n, E = case["n"], case["src"].size
    T = lambda k: torch.from_numpy(case[k]).to(DEV)  # noqa: E731
    bad_end, bad_strand = T("end"), T("strand")
    bad_end[3] = int(case["start"][3])
    bad_strand[2] = 2
    for change in (dict(start=T("start").int()), dict(end=T("end")[:-1].contiguous()), dict(end=bad_end), dict(strand=bad_strand)):
        whole, views = _buffers(n, E)
        with pytest.raises(ValueError):
            _device_call(case, views, **change)
        torch.cuda.synchronize()
        assert bool((whole[0] == 7.0).all()) and bool((whole[3] == -7).all()), list(change)
    whole, views = _buffers(n, E)                                       # the same buffers work once the arguments do
    _device_call(case, views)
    np.testing.assert_array_equal(views[0].cpu().numpy(), lref.expected("tip", case)["y"])


def test_reads_to_two_training_steps(lib):
    import overlap_reference as O
    from test_overlap_cpu import GENOME
    from gnnome_assembly_amd import features, labels, models, overlap, train
    from gnnome_assembly_amd.reads import ReadStore
    gr = O.cached(("genome", 0.0, 23), lambda: O.genome_reads(seed=23, rate=0.0))
    store = ReadStore.from_sequences(gr["reads"]).to(DEV)
    og = overlap.find_overlaps(store, verify=True, max_errors=31, drop_contained=False, **GENOME)
    g = og.graph
    gt = labels.label_overlap_graph(og, gr["truth"])
    src, dst = (t.cpu().numpy() for t in g.edges())
    start, end, strand = (t.numpy() for t in labels.node_positions(gr["truth"], g.num_nodes()))
    want = lref.reference_labels(src, dst, g.num_nodes(), start, end, strand, g.edata["twin"].cpu().numpy())
    check(gt, want, "overlap graph")
    assert 0 < int(gt.y.sum()) < g.num_edges()                          # both classes
    x, e, pe = features.prepare_graph(g, reads=store)
    sample = train.GraphSample(g, e, pe, gt.y, x)
    H, L = 128, 2
    torch.manual_seed(3)
    model = models.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16).to(DEV)
    crit = models.BCEWithLogitsLoss(pos_weight=1.0 / train.pos_to_neg_ratio([sample]))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad()
        loss = crit(model(sample.graph, sample.x, sample.e, sample.pe).squeeze(-1), sample.y)
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss))
