"""tests/bn_reference.py checked on the CPU: the per-kernel fp64 functions composed end to end equal the oracle's hand-derived layer
and fp64 autograd of the plain module formula; the cases of the GPU test keep their undecided relu branches under the cap; the bound
parts bound torch's own fp32 CPU evaluation with the recorded constants."""
import os
import sys

import numpy as np
import pytest
import torch

import bn_reference as br
from helpers import sd_to_torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_index(src, dst, n):
    from gnnome_assembly_amd import AssemblyGraph
    h = AssemblyGraph(np.asarray(src, np.int32), np.asarray(dst, np.int32), int(n), node_order="keep").host_index()
    return {k: np.asarray(h[k]).astype(np.int64) for k in ("isrc", "idst", "in_ptr", "out_ptr", "out_pos", "out_dst", "perm")}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("graph", ["tiny_edge_case", "generated"])
def test_composed_reference_equals_oracle_and_autograd(graph):
    from gnnome_assembly_amd import synth
    from oracle import gatedgcn_oracle as orc
    H, L = 32, 1
    src, dst, n = synth.tiny_edge_case_graph() if graph == "tiny_edge_case" else synth.make_graph(60, seed=5, permute_edge_ids=True)
    inp = synth.make_inputs(src, dst, n, seed=3)
    sd = synth.synth_state_dict(H, L, seed=1)
    rng = np.random.default_rng(2)
    for k in ("bn_e", "bn_h"):
        sd[f"gnn.convs.0.{k}.weight"] = (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)
        sd[f"gnn.convs.0.{k}.bias"] = (0.2 * rng.standard_normal(H)).astype(np.float32)
    p64 = sd_to_torch(sd, torch.float64)
    ts, td = torch.from_numpy(np.asarray(src)).long(), torch.from_numpy(np.asarray(dst)).long()
    with torch.no_grad():
        _, _, g64, dbg = orc.manual_forward_backward(p64, ts, td, n, torch.from_numpy(inp["e"]).double(), torch.from_numpy(inp["pe"]).double(),
                                                     torch.from_numpy(inp["y"]).double(), float(inp["pos_weight"]), keep=True)
    o = dbg[0]
    ix = _host_index(src, dst, n)
    perm = ix["perm"]
    npy = lambda t: t.numpy()  # noqa: E731
    e_in, P = npy(o["e"])[perm], npy(o["P"])
    pre = "gnn.convs.0."
    t_in = e_in @ npy(p64[pre + "B_3.weight"]).T + npy(p64[pre + "B_3.bias"])
    d = dict(P=P, t_in=t_in, e_in=e_in, h_in=npy(o["h"]), gh_out=npy(o["gh_out"]), ge_out=npy(o["ge_out"])[perm],
             gamma_e=npy(p64[pre + "bn_e.weight"]), beta_e=npy(p64[pre + "bn_e.bias"]), gamma_h=npy(p64[pre + "bn_h.weight"]),
             beta_h=npy(p64[pre + "bn_h.bias"]))
    r = br.layer_ref(d, ix, n)
    Q = npy(o["Q"])
    want = dict(t=npy(o["t"])[perm], e_out=npy(o["e_out"])[perm], hf=npy(o["hf"]), inv_f=npy(o["inv_f"]), hb=npy(o["hb"]), inv_b=npy(o["inv_b"]),
                z=npy(o["z"]), h_out=npy(o["h_out"]), gz=npy(o["gz"]), Q=np.concatenate([Q[:, :H], Q[:, 2 * H:3 * H]], 1), ge=npy(o["ge_tot"])[perm],
                gt=npy(o["gt"])[perm], gP=npy(o["gP"]), ggamma_h=npy(g64[pre + "bn_h.weight"]), gbeta_h=npy(g64[pre + "bn_h.bias"]),
                ggamma_e=npy(g64[pre + "bn_e.weight"]), gbeta_e=npy(g64[pre + "bn_e.bias"]))
    for k, w in want.items():
        assert _rel(r[k], w) <= 1e-12, f"{k}: {_rel(r[k], w):.3e} from the oracle's hand-derived layer"
    stat = np.stack([npy(o["t"]).mean(0), npy(o["rstd_e"])])
    assert _rel(r["stat_e"][:2], stat) <= 1e-12
    # fp64 autograd of the plain module formula
    h = o["h"].clone().requires_grad_(True)
    e = o["e"].clone().requires_grad_(True)
    q = {k: v.clone().requires_grad_(True) for k, v in p64.items() if "bn_" in k}
    h_out, e_out = orc.layer_forward({**p64, **q}, 0, ts, td, n, h, e)
    ((h_out * o["gh_out"]).sum() + (e_out * o["ge_out"]).sum()).backward()
    assert _rel(r["h_out"], h_out.detach().numpy()) <= 1e-12 and _rel(r["e_out"], e_out.detach().numpy()[perm]) <= 1e-12
    W5 = np.concatenate([npy(p64[pre + k + ".weight"]) for k in ("A_1", "A_2", "A_3", "B_1", "B_2")], 0)
    assert _rel(d["gh_out"] + r["gP"] @ W5, h.grad.numpy()) <= 1e-12
    assert _rel(r["ge"] + r["gt"] @ npy(p64[pre + "B_3.weight"]), e.grad.numpy()[perm]) <= 1e-12
    for k, mine in (("bn_e.weight", "ggamma_e"), ("bn_e.bias", "gbeta_e"), ("bn_h.weight", "ggamma_h"), ("bn_h.bias", "gbeta_h")):
        assert _rel(r[mine], q[pre + k].grad.numpy()) <= 1e-12, k


@pytest.mark.parametrize("H", br.WIDTHS)
def test_undecided_share_of_every_gpu_case(H):
    """No (case, H) of the GPU test has more than 0.1 % undecided relu elements in the fp64 reference alone (a case so small that
    0.1 % is less than one element: none at all)."""
    cs = [(i, c) for i, c in enumerate(br.cases(H))]
    cs.append((br.SWEEP_CASE, cs[-1][1]))
    for i, (name, src, dst, n) in cs:
        ix = _host_index(src, dst, n)
        d = br.make_layer_inputs(br.case_seed(H, i), ix, n, len(src), H)
        share = br.undecided_share(d, ix, n)
        assert share <= br.UNDECIDED_CAP, f"H={H} {name} (seed {br.case_seed(H, i)}): {share:.3%} undecided"


def test_bound_parts_bound_torch_fp32():
    """torch's fp32 CPU batch_norm and its autograd, on fresh data, stay inside c u A + u Rnd with c = DEVICE_FACTOR x the recorded ratios."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import measure_batchnorm_bounds as mb
    ratio, _ = mb.measure(rows=1500, seed=7)
    c = br.load_constants()
    for k in ("fwd", "bwd"):
        assert (ratio[k] <= c[k]).all(), f"{k}: torch fp32 ratios {ratio[k].round(2).tolist()} outside the constants {c[k].tolist()}"
