"""cluster.induced_subgraph(method="index") -- gnm_graph_induce_count / gnm_graph_induce_fill (csrc/gnm_induce.hip): the sub-graph
and its index derived from the parent's index -- against the 'sort' route (induced_subgraph + graph.tensor_index).  Integer data
throughout: every comparison is exact equality.  A kernel fault surfaces as an error of the synchronisation that ends each step."""
import ctypes as C

import numpy as np
import pytest
import torch

from gnnome_assembly_amd import _lib, cluster, engine, graph

import induce_cases as ic

pytestmark = pytest.mark.gpu

MASKS = ("all", "one", "none", "nodes_without_edges", "every_second", "block")


def _dev():
    assert torch.cuda.is_available(), "needs cuda:0"
    return torch.device("cuda:0")


def _index_route(g, mask):
    sub = cluster.induced_subgraph(g, mask, method="index")
    torch.cuda.synchronize()
    assert sub.relabel_info["induce"] == "index"
    assert g.device in sub._dev_index, "the sub-graph must come with its device index filled in"
    s, d = sub.edges()
    return sub.ndata[cluster.NID], sub.edata[cluster.EID], s, d, sub.index(), sub


def _assert_same_graph(got, want, what):
    ic.assert_same(got, want, what)
    gs, ws = got[5], want[5]
    assert (gs.num_nodes(), gs.num_edges()) == (ws.num_nodes(), ws.num_edges()), what
    assert set(gs.ndata) == set(ws.ndata) and set(gs.edata) == set(ws.edata), what
    for a, b in ((gs.ndata, ws.ndata), (gs.edata, ws.edata)):
        for k in b:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{what}: feature '{k}' differs"
    assert gs.relabel_info["relabelled"] == ws.relabel_info["relabelled"], what


@pytest.mark.parametrize("node_order,shuffle", [("bfs", True), ("keep", True), ("keep", False)])
def test_index_route_equals_sort_route_on_small_graphs(node_order, shuffle):
    """(a) and (c): the CPU test's graphs and masks -- duplicates, self loops, isolated nodes, nodes without in- / out-edges; all,
    one, no node, nodes without an edge, every second node, a block -- through the kernels; n' = 0 and e' = 0 give well-formed empty
    arrays."""
    dev = _dev()
    for seed, n, e in [(1, 300, 2000), (2, 97, 400)]:
        src, dst, n, isolated = ic.random_graph(seed, n, e, shuffle)
        g = ic.parent(src, dst, n, node_order, dev)
        ms = ic.masks(src, dst, n, isolated)
        for name in MASKS:
            want = ic.sort_route(g, ms[name])
            got = _index_route(g, ms[name])
            _assert_same_graph(got, want, f"seed {seed} {node_order} shuffle={shuffle} mask {name}")
        none, noedge = _index_route(g, ms["none"]), _index_route(g, ms["nodes_without_edges"])
        assert none[5].num_nodes() == 0 and none[5].num_edges() == 0
        assert noedge[5].num_nodes() == int(ms["nodes_without_edges"].sum()) > 1 and noedge[5].num_edges() == 0
        for r in (none, noedge):
            idx = r[4]
            assert all(idx[k].numel() == 0 for k in ("perm", "isrc", "idst", "out_pos", "out_dst")) and r[1].numel() == 0
            for k in ("in_ptr", "out_ptr"):
                assert idx[k].numel() == r[5].num_nodes() + 1 and not bool(idx[k].any())


def _boundary_graph(seed, n, e, B):
    """random banded edges; the edges with ids 0 and e - 1 are self loops of nodes 0 and n - 1 (the first and the last entry of
    the destination order and of the by-source order), the ids next to every block boundary join nodes that the mask keeps"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, e)
    dst = np.clip(src + rng.integers(-4, 5, e), 0, n - 1)
    edges_at = [k for b in range(0, e + B, B) for k in (b - 1, b) if 0 <= k < e] + [e - 1]
    nodes_at = sorted({v for b in range(0, n + B, B) for v in (b - 1, b) if 0 <= v < n} | {0, n - 1})
    for j, k in enumerate(edges_at):
        src[k], dst[k] = nodes_at[j % len(nodes_at)], nodes_at[(j + 1) % len(nodes_at)]
    src[0] = dst[0] = 0
    src[e - 1] = dst[e - 1] = n - 1
    mask = rng.random(n) < 0.5
    mask[nodes_at] = True
    return src.astype(np.int32), dst.astype(np.int32), torch.from_numpy(mask)


@pytest.mark.parametrize("dn", ["B-1", "B", "B+1", "2B+3"])
def test_scan_block_boundaries(dn):
    """(b): N and E at the block constant of the prefix sums, one below, one above and past two blocks (a partial third); the mask
    keeps the first and the last element of every block of the node order and of the edge-id order, and the first and last entry of
    both sorted orders.  Parents with and without an internal numbering."""
    dev = _dev()
    B = graph.induce_scan_block()
    assert B == 1024
    sizes = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+3": 2 * B + 3}
    n = sizes[dn]
    for de, e in sizes.items():
        src, dst, mask = _boundary_graph(n + e, n, e, B)
        for node_order in ("keep", "bfs"):
            g = ic.parent(src, dst, n, node_order, dev)
            want = ic.sort_route(g, mask)
            got = _index_route(g, mask)
            assert bool(mask[0]) and bool(mask[-1]) and want[1][0] == 0 and want[1][-1] == e - 1
            _assert_same_graph(got, want, f"N = {dn}, E = {de}, {node_order}")
            _assert_same_graph(_index_route(g, torch.ones(n, dtype=torch.bool)), ic.sort_route(g, torch.ones(n, dtype=torch.bool)),
                               f"N = {dn}, E = {de}, {node_order}, all nodes")


def test_block_sums_span_more_than_one_wave_and_more_than_one_block_per_thread():
    """(b): 69 blocks of nodes (more than the 64 lanes of one wave of block sums) and 293 blocks of edges (more than the 256
    threads of the workgroup that scans them: two blocks per thread)."""
    dev = _dev()
    B = graph.induce_scan_block()
    n, e = 68 * B + 3, 292 * B + 5
    src, dst, mask = _boundary_graph(9, n, e, B)
    for node_order in ("bfs", "keep"):
        g = ic.parent(src, dst, n, node_order, dev)
        _assert_same_graph(_index_route(g, mask), ic.sort_route(g, mask), f"large, {node_order}")


def test_cpu_parent_falls_back_and_oversized_graphs_are_rejected():
    """(c): a parent on the CPU has no device index: 'sort' runs and relabel_info says so.  E >= 2^31 is refused by the size check of
    the entry points (nothing is allocated, no pointer is read)."""
    _dev()
    src, dst, n, isolated = ic.random_graph(4, 120, 600, True)
    g = ic.parent(src, dst, n, "bfs")
    mask = ic.masks(src, dst, n, isolated)["block"]
    sub = cluster.induced_subgraph(g, mask, method="index")
    assert sub.relabel_info["induce"] == "sort" and "CPU" in sub.relabel_info["induce_fallback"]
    s, d = sub.edges()
    ic.assert_same((sub.ndata[cluster.NID], sub.edata[cluster.EID], s, d, sub.index()), ic.sort_route(g, mask), "fall-back")
    lib = _lib.load()
    assert lib.gnm_graph_induce_workspace_bytes(10, 2 ** 31) == 0
    null = C.c_void_p(None)
    with pytest.raises(_lib.GnmError, match="2\\^31"):
        _lib.check(lib.gnm_graph_induce_count(10, 2 ** 31, null, null, null, null, null, null, null, 0, null, null), "induce_count")
    with pytest.raises(_lib.GnmError):
        _lib.check(lib.gnm_graph_induce_fill(10, 2 ** 31, 1, 1, *([null] * 11), 0, *([null] * 13), null), "induce_fill")


def _loader_case(dev):
    import gnnome_assembly_amd as G
    from gnnome_assembly_amd import synth
    seed, H, L = 6, 128, 2
    src, dst, n = synth.make_graph(2000, seed=seed)
    inp = synth.make_inputs(src, dst, n, seed=seed)
    p = np.random.default_rng(5).permutation(n).astype(np.int32)          # scattered caller ids: the parent renumbers (nrank)
    src, dst = p[src], p[dst]
    pe = np.empty_like(inp["pe"])
    pe[p] = inp["pe"]
    g = G.AssemblyGraph(src, dst, n, node_order="bfs").to(dev)
    g.ndata["pe"] = torch.from_numpy(pe).to(dev)
    g.edata["e"] = torch.from_numpy(inp["e"]).to(dev)
    g.edata["y"] = torch.from_numpy(inp["y"]).to(dev)
    part = cluster.partition_graph(g, 8)
    model = G.GraphGatedGCNModel(1, 2, H, 16, L, 64, True, 16)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(H, L, seed).items()})
    model.to(dev)
    return g, part, model, G.BCEWithLogitsLoss(float(inp["pos_weight"]))


def _batches(g, part, induce, prefetch):
    loader = cluster.ClusterBatchLoader(g, part, 2, shuffle=True, generator=torch.Generator().manual_seed(3), prefetch=prefetch,
                                        induce=induce)
    assert loader.prefetch == prefetch and len(loader) == 4
    out = list(loader)
    torch.cuda.synchronize()
    return out


def _as_tuple(sub):
    s, d = sub.edges()
    return sub.ndata[cluster.NID], sub.edata[cluster.EID], s, d, sub.index(), sub


def test_one_training_step_through_each_loader_route():
    """(d): the same shuffled pass of four two-cluster batches with induce='index' and 'sort': equal graphs, equal sweep plans, and
    -- same index, same launches -- bit-identical logits and parameter gradients of one forward + backward per batch."""
    dev = _dev()
    g, part, model, crit = _loader_case(dev)
    routes = {m: _batches(g, part, m, False) for m in ("sort", "index")}
    assert all(b.relabel_info["induce"] == "index" for b in routes["index"])
    assert all("induce" not in b.relabel_info for b in routes["sort"])

    def step(sub):
        model.zero_grad(set_to_none=True)
        s = model(sub, None, sub.edata["e"], sub.ndata["pe"])
        crit(s.squeeze(-1), sub.edata["y"]).backward()
        torch.cuda.synchronize()
        return s.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters()}
    for k, (a, b) in enumerate(zip(routes["sort"], routes["index"])):
        _assert_same_graph(_as_tuple(b), _as_tuple(a), f"batch {k}")
        assert a.num_edges() > 1000
        for wg in (1, engine.GATE2_WG):
            pa, pb = a.sweep_plan(dev, wg), b.sweep_plan(dev, wg)
            assert pa is not None and pb is not None and pa["nodes_per_block"] == pb["nodes_per_block"]
            for key in ("sinfo", "dinfo", "fix_nodes", "served", "peak_dev"):
                assert torch.equal(pa[key], pb[key]), f"batch {k}: sweep plan ({wg} per CU) '{key}' differs"
        s0, g0 = step(a)
        s1, g1 = step(b)
        assert bool(torch.isfinite(s0).all())
        assert torch.equal(s0, s1), f"batch {k}: logits differ between the routes"
        for name in g0:
            assert torch.equal(g0[name], g1[name]), f"batch {k}: gradient of {name} differs between the routes"


def test_prefetching_loader_yields_the_same_batches():
    """(e): batches built on the side stream and handed over equal the ones built in line."""
    dev = _dev()
    g, part, _, _ = _loader_case(dev)
    inline, ahead = _batches(g, part, "index", False), _batches(g, part, "index", True)
    ref = _batches(g, part, "sort", False)
    for k, (a, b, c) in enumerate(zip(inline, ahead, ref)):
        _assert_same_graph(_as_tuple(b), _as_tuple(a), f"prefetched batch {k}")
        _assert_same_graph(_as_tuple(b), _as_tuple(c), f"prefetched batch {k} vs sort")
        for wg in (1, engine.GATE2_WG):                  # the prefetching loader builds the plans on the side stream too
            pa, pb = a.sweep_plan(dev, wg), b.sweep_plan(dev, wg)
            assert all(torch.equal(pa[key], pb[key]) for key in ("sinfo", "dinfo", "fix_nodes"))
