"""graph.induced_index_from_parent -- the torch statement of what gnm_graph_induce_count / _fill compute -- against the 'sort'
route (cluster.induced_subgraph + graph.tensor_index, itself pinned to the host builder by
test_host_cpu.py::test_tensor_index_equals_host_index).  Exact equality of every array; runs without a GPU."""
import pytest
import torch

from gnnome_assembly_amd import cluster, graph

import induce_cases as ic

GRAPHS = [(1, 300, 2000), (2, 97, 400), (3, 64, 1500)]      # (seed, N, E): N <= 300, E <= 2 000
MASKS = ("all", "one", "none", "nodes_without_edges", "every_second", "block")


@pytest.mark.parametrize("node_order,shuffle", [("bfs", True), ("bfs", False), ("keep", True), ("keep", False)])
@pytest.mark.parametrize("seed,n,e", GRAPHS)
def test_index_filtered_from_parent_equals_sort_route(seed, n, e, node_order, shuffle):
    src, dst, n, isolated = ic.random_graph(seed, n, e, shuffle)
    g = ic.parent(src, dst, n, node_order)
    pidx = g.index()
    assert ("nrank" in pidx) == (node_order == "bfs")
    ms = ic.masks(src, dst, n, isolated)
    assert set(ms) == set(MASKS)
    for name in MASKS:
        want = ic.sort_route(g, ms[name])
        got = graph.induced_index_from_parent(pidx, n, ms[name])
        ic.assert_same(got, want, f"seed {seed} {node_order} shuffle={shuffle} mask {name}")
        for t in got[:2]:
            assert t.dtype == torch.int64
        n_sub, e_sub = int(ms[name].sum()), want[1].numel()
        assert got[4]["in_ptr"].numel() == n_sub + 1 and int(got[4]["in_ptr"][-1]) == e_sub == int(got[4]["out_ptr"][-1])
    assert ic.sort_route(g, ms["nodes_without_edges"])[1].numel() == 0 and int(ms["nodes_without_edges"].sum()) > 1
    assert ic.sort_route(g, ms["all"])[1].numel() == e


def test_cpu_parent_runs_the_sort_route_and_says_so():
    src, dst, n, isolated = ic.random_graph(4, 120, 600, True)
    g = ic.parent(src, dst, n, "bfs")
    mask = ic.masks(src, dst, n, isolated)["block"]
    want = ic.sort_route(g, mask)
    sub = cluster.induced_subgraph(g, mask, method="index")
    assert sub.relabel_info["induce"] == "sort" and "CPU" in sub.relabel_info["induce_fallback"]
    s, d = sub.edges()
    ic.assert_same((sub.ndata[cluster.NID], sub.edata[cluster.EID], s, d, sub.index()), want, "fall-back")
    assert "induce" not in want[5].relabel_info
    with pytest.raises(ValueError):
        cluster.induced_subgraph(g, mask, method="radix")
    with pytest.raises(ValueError):
        cluster.ClusterBatchLoader(g, cluster.partition_graph(g, 4), 2, induce="radix")
    assert cluster.ClusterBatchLoader(g, cluster.partition_graph(g, 4), 2).induce == cluster.INDUCE
