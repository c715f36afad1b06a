"""The two input-feature entry points (-m gpu): gnm_pagerank_pe and gnm_edge_feats_zscore (csrc/gnm_features.hip), through the C
ABI and through features.positional_encoding / features.edge_features, EVERY element against the fp64 statements of
tests/features_reference.py within the per-element bars derived there (half an fp32 ulp of the wanted value plus the reach of the
kernel's fp64 sums); the degree columns exactly.  The matrix is features_reference.pagerank_cases / zscore_cases:
test_features_reference_cpu.py shows, without a device, that a correct kernel stays inside these bars on every case and that each
listed mutant misses one.

Every C-ABI call gets its output and its workspace -- exactly as many bytes as the entry point asks for -- inside larger
sentinel-filled buffers: the sentinels around them are intact afterwards and none is left inside an output.  Every kernel is
atomic-free with a fixed summation order, so every case runs twice and must repeat bit for bit, on another stream and (PageRank)
under another occupancy cap as well.  The rejected calls are all stopped by the host-side argument check, before any launch."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import features_reference as fr

pytestmark = pytest.mark.gpu

PAD = 64                           # sentinel elements on either side of an output or workspace (keeps them 16-byte aligned)
SENT32 = -1.2345678e30
SENT64 = -1.2345678e300
PR_NAMES = list(fr.pagerank_cases())
ZS_NAMES = fr.zscore_case_names()


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _lib():
    from gnnome_assembly_amd import _lib as L
    return L.load()


def _cus():
    _dev()
    return int(_lib().gnm_num_cus())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _st(stream=None):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def _msg():
    return _lib().gnm_last_error().decode(errors="replace")


def _guarded(n, dtype):
    """(buffer, view): `view` = n elements in the middle of a sentinel-filled buffer."""
    buf = torch.full((PAD + n + PAD,), SENT32 if dtype == torch.float32 else SENT64, dtype=dtype, device=_dev())
    return buf, buf[PAD:PAD + n]


def _sentinel(t):
    return t == (SENT32 if t.dtype == torch.float32 else SENT64)


def _guards_intact(buf, n, what):
    torch.cuda.synchronize()
    assert bool(_sentinel(buf[:PAD]).all()), f"{what}: written BEFORE its first element"
    assert bool(_sentinel(buf[PAD + n:]).all()), f"{what}: written PAST its last element"


def _d(a):
    """A device copy of a (read-only) case array."""
    return torch.tensor(a, device=_dev())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"{what}: results differ"


def _within(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    r, i = fr.worst_ratio(got, want, bound)
    # (rounding to fp32 alone uses the whole half-ulp, so the worst ratio of a large case is near 1; the second figure says how
    # many elements are NOT the fp32 number nearest to the fp64 value, i.e. how often the fp64 sums decided the last bit)
    off = int((got.astype(np.float32) != want.astype(np.float32))[np.isfinite(bound)].sum())
    print(f"ratio {what}: worst |error| / bar = {r:.3f}; {off} of {int(np.isfinite(bound).sum())} elements not the nearest fp32")
    assert r <= 1.0, (f"{what}: worst element {np.unravel_index(i, want.shape)}: got {got.flat[i]!r} want {want.flat[i]!r} "
                      f"bar {bound.flat[i]:.3e} ({r:.2f} bars)")


# ---- PageRank ------------------------------------------------------------------------------------------------------------------

def _graph(src, dst, n, node_order=None):
    from gnnome_assembly_amd import AssemblyGraph
    g = AssemblyGraph(np.array(src), np.array(dst), n, node_order=node_order).to(_dev())
    return g, g.index(_dev())


def _pagerank_abi(idx, n, E, pe_dim, alpha, stream=None):
    """gnm_pagerank_pe on guarded buffers with exactly the workspace it asks for -> fp32 [n, 2 + pe_dim] in the CALLER's numbering."""
    lib = _lib()
    ld = pe_dim + 2
    need = lib.gnm_pagerank_pe_workspace_bytes(n)
    assert need == 3 * n * 8
    pbuf, pe = _guarded(n * ld, torch.float32)
    wbuf, ws = _guarded(3 * n, torch.float64)
    torch.cuda.synchronize()
    rc = lib.gnm_pagerank_pe(n, E, _p(idx["isrc"]), _p(idx["in_ptr"]), _p(idx["out_ptr"]), pe_dim, C.c_double(alpha), _p(pe), _p(ws),
                             need, _st(stream))
    assert rc == 0, f"gnm_pagerank_pe: rc = {rc} ({_msg()})"
    _guards_intact(pbuf, n * ld, "pe")
    _guards_intact(wbuf, 3 * n, "PageRank workspace")
    assert not bool(_sentinel(pe).any()), "pe: an element was never written"
    rows = pe.view(n, ld).cpu().numpy()
    return rows[idx["nrank"].cpu().numpy()] if "nrank" in idx else rows


def _check_pagerank(name, got, what):
    want, bound = fr.pagerank_want(name, _cus())
    assert np.array_equal(got[:, :2].astype(np.float64), want[:, :2]), f"{name} ({what}): the degree columns are not exact"
    _within(got, want, bound, f"pagerank | {name} | {what}")


@pytest.mark.parametrize("name", PR_NAMES)
def test_pagerank_per_element(name):
    from gnnome_assembly_amd import features
    src, dst, n, pe_dim, alpha = fr.pagerank_cases(_cus())[name]
    if name == "path past the grid cap":
        assert n == _cus() * 8 * 256 + 257 and fr.pr_grid(n, _cus()) * 256 < n
    g, idx = _graph(src, dst, n)
    got = _pagerank_abi(idx, n, len(src), pe_dim, alpha)
    _check_pagerank(name, got, "C ABI")
    _same_bits(_pagerank_abi(idx, n, len(src), pe_dim, alpha), got, f"{name}: two runs")
    mod = features.positional_encoding(g, pe_dim, alpha)
    assert mod.shape == (n, pe_dim + 2) and mod.dtype == torch.float32
    _same_bits(mod.cpu().numpy(), got, f"{name}: features.positional_encoding vs the C ABI")


def test_pagerank_empty_graph_closed_form():
    """E = 0 is a graph: degrees 0 and every step (1 - alpha) / n.  (An empty index tensor has a null pointer; the entry point
    accepts that for E = 0.)"""
    src, dst, n, pe_dim, alpha = fr.pagerank_cases(_cus())["E=0, N=300"]
    g, idx = _graph(src, dst, n)
    assert idx["isrc"].numel() == 0
    got = _pagerank_abi(idx, n, 0, pe_dim, alpha)
    assert np.array_equal(got[:, :2], np.zeros((n, 2), np.float32))
    assert np.array_equal(got[:, 2:], np.full((n, pe_dim), np.float32((1.0 - alpha) / n)))


@pytest.mark.parametrize("node_order", ["auto", "keep"])
def test_pagerank_rows_come_back_in_the_callers_numbering(node_order):
    from gnnome_assembly_amd import features
    name = "shuffled node ids"
    src, dst, n, pe_dim, alpha = fr.pagerank_cases(_cus())[name]
    g, idx = _graph(src, dst, n, node_order)
    assert ("nrank" in idx) == (node_order == "auto"), "the shuffled graph must get an internal numbering under 'auto' only"
    got = features.positional_encoding(g, pe_dim, alpha).cpu().numpy()
    _check_pagerank(name, got, f"node_order={node_order}")
    _same_bits(_pagerank_abi(idx, n, len(src), pe_dim, alpha), got, f"{name}: C ABI vs module, node_order={node_order}")


def test_pagerank_same_bits_under_an_occupancy_cap_and_on_another_stream():
    lib = _lib()
    name = "hub destination (6000 in-edges)"
    src, dst, n, pe_dim, alpha = fr.pagerank_cases(_cus())[name]
    g, idx = _graph(src, dst, n)
    base = _pagerank_abi(idx, n, len(src), pe_dim, alpha)
    try:
        assert lib.gnm_set_occupancy_cap(1) == 0
        capped = _pagerank_abi(idx, n, len(src), pe_dim, alpha)
    finally:
        assert lib.gnm_set_occupancy_cap(0) == 0
    _same_bits(capped, base, "occupancy cap 1 vs default")
    _same_bits(_pagerank_abi(idx, n, len(src), pe_dim, alpha), base, "default again")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    _same_bits(_pagerank_abi(idx, n, len(src), pe_dim, alpha, stream=s), base, "C ABI on another stream")
    from gnnome_assembly_amd import features
    with torch.cuda.stream(s):
        mod = features.positional_encoding(g, pe_dim, alpha)
    s.synchronize()
    _same_bits(mod.cpu().numpy(), base, "features.positional_encoding on another stream")


# ---- z-score -------------------------------------------------------------------------------------------------------------------

def _zscore_abi(a, b, nb, stream=None):
    """gnm_edge_feats_zscore on guarded buffers with exactly nb * 4 doubles of workspace -> fp32 [E, 2]."""
    lib = _lib()
    E = a.numel()
    ebuf, e = _guarded(2 * E, torch.float32)
    wbuf, ws = _guarded(4 * nb, torch.float64)
    torch.cuda.synchronize()
    rc = lib.gnm_edge_feats_zscore(E, _p(a), _p(b), _p(e), _p(ws), nb * 4 * 8, _st(stream))
    assert rc == 0, f"gnm_edge_feats_zscore: rc = {rc} ({_msg()})"
    _guards_intact(ebuf, 2 * E, "e")
    _guards_intact(wbuf, 4 * nb, "z-score workspace")
    assert not bool(_sentinel(e).any()), "e: an element was never written"
    assert not bool(_sentinel(ws).any()), "z-score workspace: fewer block sums than the entry point's block count"
    return e.view(E, 2).cpu().numpy()


@pytest.mark.parametrize("name", ZS_NAMES)
def test_zscore_per_element(name):
    from gnnome_assembly_amd import features
    c = fr.zscore_cases(_cus())[name]
    E, nb = len(c["a"]), c["nb"]
    if E == fr.ZS_E[-1]:
        assert nb == fr.MAX_PARTIAL_BLOCKS and nb * 256 < E              # the clamp, and a second trip of the grid-stride loop
    a, b = _d(c["a"]), _d(c["b"])
    got = _zscore_abi(a, b, nb)
    want, bound = fr.zscore_want(name, _cus())
    _within(got, want, bound, f"zscore | {name}")        # (a column outside the accuracy contract has an infinite bar)
    _same_bits(_zscore_abi(a, b, nb), got, f"{name}: two runs")
    _same_bits(features.edge_features(a, b).cpu().numpy(), got, f"{name}: features.edge_features vs the C ABI")


def test_zscore_int64_lengths_and_a_strided_view():
    """features.edge_features converts and packs its inputs: int64 lengths (what the graph parser stores) and a column view of a
    wider tensor give the bits of the plain fp32 vectors."""
    from gnnome_assembly_amd import features
    name = "E=257: lengths uniform [500, 30000) | similarity uniform under 1"
    c = fr.zscore_cases(_cus())[name]
    a, b = _d(c["a"]), _d(c["b"])
    got = _zscore_abi(a, b, c["nb"])
    a64 = _d(c["a"].astype(np.int64))
    assert np.array_equal(a64.cpu().numpy().astype(np.float32), c["a"])
    wide = torch.stack([b, -b, b * 0.5], 1)
    view = wide[:, 0]
    assert not view.is_contiguous() and a64.dtype == torch.int64
    e = features.edge_features(a64, view)
    assert e.shape == (len(c["a"]), 2) and e.dtype == torch.float32
    _same_bits(e.cpu().numpy(), got, "int64 lengths + strided similarity")
    want, bound = fr.zscore_want(name, _cus())
    _within(e.cpu().numpy(), want, bound, "zscore | int64 lengths + strided view")


def test_zscore_same_bits_on_another_stream():
    from gnnome_assembly_amd import features
    name = f"E={fr.ZS_E[-1]}: negative | one outlier of 1e6"
    c = fr.zscore_cases(_cus())[name]
    a, b = _d(c["a"]), _d(c["b"])
    base = _zscore_abi(a, b, c["nb"])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    _same_bits(_zscore_abi(a, b, c["nb"], stream=s), base, "C ABI on another stream")
    with torch.cuda.stream(s):
        e = features.edge_features(a, b)
    s.synchronize()
    _same_bits(e.cpu().numpy(), base, "features.edge_features on another stream")


# ---- argument checks: each call is stopped by the host-side check, before any launch ----------------------------------------------

@pytest.fixture(scope="module")
def bufs():
    src, dst, n = fr.small_graph()
    g, idx = _graph(src, dst, n)
    E, pe_dim = len(src), 16
    rng = np.random.default_rng(9)
    pbuf, pe = _guarded(n * (pe_dim + 2), torch.float32)
    wbuf, ws = _guarded(3 * n, torch.float64)
    ebuf, e = _guarded(2 * E, torch.float32)
    zbuf, zws = _guarded(4 * fr.zs_blocks(E, _cus()), torch.float64)
    return dict(idx=idx, n=n, E=E, pe_dim=pe_dim, pbuf=pbuf, pe=pe, wbuf=wbuf, ws=ws, ebuf=ebuf, e=e, zbuf=zbuf, zws=zws,
                a=torch.from_numpy(rng.integers(500, 30000, E).astype(np.float32)).to(_dev()),
                b=torch.from_numpy(rng.random(E).astype(np.float32)).to(_dev()))


def _untouched(b, what):
    torch.cuda.synchronize()
    for k in ("pbuf", "wbuf", "ebuf", "zbuf"):
        assert bool(_sentinel(b[k]).all()), f"{what}: {k} was written: something was launched before the check"


def _pagerank_rejected(b, word, **bad):
    lib = _lib()
    a = dict(n=b["n"], E=b["E"], pe_dim=b["pe_dim"], pe=_p(b["pe"]), ws_bytes=lib.gnm_pagerank_pe_workspace_bytes(b["n"]))
    a.update(bad)
    idx = b["idx"]
    rc = lib.gnm_pagerank_pe(a["n"], a["E"], _p(idx["isrc"]), _p(idx["in_ptr"]), _p(idx["out_ptr"]), a["pe_dim"], C.c_double(0.95),
                             a["pe"], _p(b["ws"]), a["ws_bytes"], _st())
    msg = _msg()
    assert rc == -1, f"gnm_pagerank_pe({bad}): rc = {rc}, expected the argument error -1 ({msg!r})"
    assert re.match(r"pagerank_pe: ", msg) and word in msg, f"gnm_pagerank_pe({bad}): message {msg!r}"
    _untouched(b, f"gnm_pagerank_pe({bad})")


def _zscore_rejected(b, word, **bad):
    lib = _lib()
    a = dict(E=b["E"], ws_bytes=b["zws"].numel() * 8)
    a.update(bad)
    rc = lib.gnm_edge_feats_zscore(a["E"], _p(b["a"]), _p(b["b"]), _p(b["e"]), _p(b["zws"]), a["ws_bytes"], _st())
    msg = _msg()
    assert rc == -1, f"gnm_edge_feats_zscore({bad}): rc = {rc}, expected the argument error -1 ({msg!r})"
    assert re.match(r"edge_feats_zscore: ", msg) and word in msg, f"gnm_edge_feats_zscore({bad}): message {msg!r}"
    _untouched(b, f"gnm_edge_feats_zscore({bad})")


def test_pagerank_rejects_no_nodes(bufs):
    _pagerank_rejected(bufs, "bad argument", n=0)


def test_pagerank_rejects_a_negative_pe_dim(bufs):
    _pagerank_rejected(bufs, "bad argument", pe_dim=-1)


def test_pagerank_rejects_a_null_output(bufs):
    _pagerank_rejected(bufs, "bad argument", pe=C.c_void_p(0))


def test_pagerank_rejects_a_workspace_one_byte_short(bufs):
    _pagerank_rejected(bufs, "workspace", ws_bytes=_lib().gnm_pagerank_pe_workspace_bytes(bufs["n"]) - 1)


@pytest.mark.parametrize("E", [0, 1])
def test_zscore_rejects_fewer_than_two_edges(bufs, E):
    _zscore_rejected(bufs, "bad argument", E=E)


def test_zscore_rejects_a_workspace_one_byte_short(bufs):
    _zscore_rejected(bufs, "workspace", ws_bytes=bufs["zws"].numel() * 8 - 1)


def test_entry_points_accept_what_the_rejections_vary(bufs):
    """The same buffers with nothing replaced are accepted: the rejections above are down to the one argument they change."""
    lib = _lib()
    b, idx = bufs, bufs["idx"]
    pe, ws = torch.empty_like(b["pe"]), torch.empty_like(b["ws"])
    assert lib.gnm_pagerank_pe(b["n"], b["E"], _p(idx["isrc"]), _p(idx["in_ptr"]), _p(idx["out_ptr"]), b["pe_dim"], C.c_double(0.95),
                               _p(pe), _p(ws), ws.numel() * 8, _st()) == 0, _msg()
    e, zws = torch.empty_like(b["e"]), torch.empty_like(b["zws"])
    assert lib.gnm_edge_feats_zscore(b["E"], _p(b["a"]), _p(b["b"]), _p(e), _p(zws), zws.numel() * 8, _st()) == 0, _msg()
    torch.cuda.synchronize()
    _untouched(b, "accepted calls on buffers of their own")
