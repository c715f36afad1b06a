"""The argument checks of the five chained-sweep entry points (gnm_edge_bwd_chain, gnm_edge_bwd_chain_src, gnm_edge_bwd_top,
gnm_ln_edge_bwd_top, gnm_ln_edge_bwd_chain), through the C ABI: a workspace one byte too small, a sweep plan built for another
partition, a width that is not built and aliased outputs are argument errors (-1) that name the entry point and come back BEFORE
anything is launched.  Every call gets real, correctly sized device tensors for everything but the one argument under test; every
float buffer holds a sentinel that any launch of the sweep (its first kernel zeroes gP / Ud / Td rows) would disturb.

gnm_edge_bwd_chain_src shares its body with gnm_edge_bwd_chain: the checks that do not concern the plan may report either name."""
import ctypes as C
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 128
SENTINEL = 3.0

NAME = {
    "gnm_edge_bwd_chain": r"edge_bwd_chain: ",
    "gnm_edge_bwd_chain_src": r"edge_bwd_chain(_src)?: ",
    "gnm_edge_bwd_top": r"edge_bwd_top: ",
    "gnm_ln_edge_bwd_top": r"ln_edge_bwd_top: ",
    "gnm_ln_edge_bwd_chain": r"ln_edge_bwd_chain: ",
}
PLAN_NAME = dict(NAME, gnm_edge_bwd_chain_src=r"edge_bwd_chain_src: ")
TAKES_PLAN = [e for e in NAME if e != "gnm_edge_bwd_chain"]


@pytest.fixture(scope="module")
def bufs():
    from gnnome_assembly_amd import AssemblyGraph, _lib, synth
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    src, dst, N = synth.make_graph(32, seed=11)
    g = AssemblyGraph(src, dst, N).to(dev)
    plan = g.sweep_plan(dev, 1)
    assert N == 64 and plan is not None
    E = g.num_edges()
    f = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
    d = lambda: torch.full((lib.gnm_max_partial_blocks() * 2 * H,), SENTINEL, dtype=torch.float64, device=dev)  # noqa: E731
    b = dict(N=N, E=E, idx=g.index(), sinfo=plan["sinfo"], npb=int(plan["nodes_per_block"]),
             need=lib.gnm_edge_bwd_fused_workspace_bytes(),
             ge=f(E, H), ge_out=f(E, H), t_hi=f(E, H), e_mid=f(E, H), t_lo=f(E, H), gt_lo=f(E, H),
             stat_hi=f(2, H), bstat_hi=f(2, H), stat_lo=f(2, H), gamma=f(H), beta=f(H), W3=f(H, H), gW3=f(H, H), gb3=f(H),
             P=f(N, 5 * H), Q=f(N, 4 * H), hf=f(N, H), hb=f(N, H), gP=f(N, 5 * H), DT=f(N, 2 * H), UT=f(N, 2 * H),
             partials_hi=d(), partials_lo=d())
    b["ws"] = torch.empty(b["need"], dtype=torch.uint8, device=dev)
    _lib.set_matmul_mode(_lib.DEFAULT_MATMUL_MODE)        # a split mode: the chained entries are built for those only
    return lib, b


def _call(lib, b, entry, h=H, ws_bytes=None, npb=None, partials_hi=None, gt_hi=None):
    """rc and message of `entry` on the buffers of `b` with the named arguments replaced."""
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    idx = b["idx"]
    graph = [p(idx["isrc"]), p(idx["idst"]), p(idx["in_ptr"])]
    ws_bytes = b["need"] if ws_bytes is None else ws_bytes
    npb = b["npb"] if npb is None else npb
    phi = p(b["partials_hi"] if partials_hi is None else partials_hi)
    Ud, Td = b["DT"][:, :H], b["DT"][:, H:]
    tail = [C.byref(C.c_int(0)), p(b["ws"]), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    bn_hi = [p(b["ge"]), p(b["ge_out"]), p(b["t_hi"]), p(b["e_mid"]), p(b["stat_hi"]), p(b["bstat_hi"]), p(b["gamma"]), p(b["W3"]),
             p(b["gW3"]), p(b["gb3"]), phi]
    bn_lo = [p(b["t_lo"]), p(b["stat_lo"]), p(b["P"]), p(b["Q"]), p(b["hf"]), p(b["hb"])] + graph + [p(b["gP"]), p(Ud), p(Td),
                                                                                               p(b["partials_lo"])]
    plan = [p(b["sinfo"]), npb]
    args = {
        "gnm_edge_bwd_chain": bn_hi + bn_lo + tail,
        "gnm_edge_bwd_chain_src": bn_hi + bn_lo + plan + [p(b["UT"])] + tail,
        "gnm_edge_bwd_top": [p(b["ge"]), p(b["e_mid"])] + bn_lo + plan + [p(b["UT"])] + tail,
        "gnm_ln_edge_bwd_top": [p(b["ge"]), p(b["e_mid"]), p(b["t_lo"]), p(b["gamma"]), p(b["beta"]), H, p(b["P"]), p(b["Q"]), p(b["hf"]),
                                p(b["hb"])] + graph + [p(b["gP"]), p(b["gt_lo"]), p(b["partials_lo"])] + plan + tail,
        "gnm_ln_edge_bwd_chain": [p(b["ge"]), p(b["t_hi"] if gt_hi is None else gt_hi), p(b["e_mid"]), p(b["W3"]), p(b["gW3"]), p(b["gb3"]),
                                  phi, p(b["t_lo"]), p(b["gamma"]), p(b["beta"]), H, p(b["P"]), p(b["Q"]), p(b["hf"]), p(b["hb"])] + graph
                                 + [p(b["gP"]), p(b["gt_lo"]), p(b["partials_lo"])] + plan + tail,
    }[entry]
    rc = getattr(lib, entry)(b["N"], b["E"], h, *args)
    return rc, lib.gnm_last_error().decode(errors="replace")


def _rejected(lib, b, entry, name, **bad):
    rc, msg = _call(lib, b, entry, **bad)
    assert rc == -1, f"{entry}({bad}): rc = {rc}, expected the argument error -1 ({msg!r})"
    assert re.match(name, msg), f"{entry}({bad}): the message does not begin with the entry's name: {msg!r}"
    torch.cuda.synchronize()
    for k, t in b.items():
        if torch.is_tensor(t) and t.is_floating_point():
            assert bool((t == SENTINEL).all()), f"{entry}({bad}): {k} was written: something was launched before the check"
    return msg


@pytest.mark.parametrize("entry", list(NAME))
def test_workspace_one_byte_short(bufs, entry):
    lib, b = bufs
    msg = _rejected(lib, b, entry, NAME[entry], ws_bytes=b["need"] - 1)
    assert "workspace" in msg, msg


@pytest.mark.parametrize("off", [-1, 1])
@pytest.mark.parametrize("entry", TAKES_PLAN)
def test_plan_for_another_partition(bufs, entry, off):
    lib, b = bufs
    msg = _rejected(lib, b, entry, PLAN_NAME[entry], npb=b["npb"] + off)
    assert "sweep plan" in msg, msg


@pytest.mark.parametrize("entry", list(NAME))
def test_width_that_is_not_built(bufs, entry):
    lib, b = bufs
    msg = _rejected(lib, b, entry, NAME[entry], h=64)
    assert "H=64" in msg, msg


@pytest.mark.parametrize("entry", ["gnm_edge_bwd_chain", "gnm_ln_edge_bwd_chain"])
def test_partials_of_the_two_layers_must_differ(bufs, entry):
    lib, b = bufs
    msg = _rejected(lib, b, entry, NAME[entry], partials_hi=b["partials_lo"])
    assert "aliased" in msg, msg


def test_ln_chain_gt_of_the_two_layers_must_differ(bufs):
    lib, b = bufs
    msg = _rejected(lib, b, "gnm_ln_edge_bwd_chain", NAME["gnm_ln_edge_bwd_chain"], gt_hi=b["gt_lo"])
    assert "aliased" in msg, msg

