#!/usr/bin/env python3
"""Generate tests/golden/input_grads/*.npz: the gradients of the BCE loss with respect to the model's INPUTS e (edge
features) and pe (positional encodings), computed by the REFERENCE's own code.

Run in the build container only (it reads /root/reference, which does not exist on the GPU box):
      python tests/golden/make_golden_input_grads.py

How: as make_golden.py -- tests/golden/dgl_standin first on sys.path, the reference second, its `models` package
imported UNMODIFIED and run on torch-CPU in fp64, here with e and pe requiring grad (and x too: its .grad stays None,
full_graph.py:23 overwrites it).  Only data is written; no reference source is copied.  The fixtures live in a
subdirectory so that conftest.golden_files() (every top-level tests/golden/*.npz) does not hand them to the parity tests.

Cases: {tiny, small} x {h128l8, h256l2, h64l1, h32l2ln}, seed 0; parameters are regenerated from the seed by
gnnome_assembly_amd.synth.synth_state_dict (not stored).
  stored: src dst n e_raw pe y pos_weight seed H L batch_norm | loss64 grad_e_raw [E,2] grad_pe [N,18] (fp64)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "input_grads")
sys.path.insert(0, os.path.join(HERE, "dgl_standin"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import dgl  # noqa: E402  (the stand-in)
import models  # noqa: E402  (reference)
from gnnome_assembly_amd import synth  # noqa: E402

torch.set_num_threads(4)

CFGS = {
    "h128l8": dict(H=128, L=8, bn=True),
    "h256l2": dict(H=256, L=2, bn=True),
    "h64l1": dict(H=64, L=1, bn=True),
    "h32l2ln": dict(H=32, L=2, bn=False),
}


def build_graph(kind, seed):
    if kind == "tiny":
        return synth.tiny_edge_case_graph(seed)
    return synth.make_graph(1000, seed, permute_edge_ids=(seed % 2 == 1))


def run_case(kind, cfg_name, seed=0):
    cfg = CFGS[cfg_name]
    src, dst, n = build_graph(kind, seed)
    inp = synth.make_inputs(src, dst, n, seed)
    sd_np = synth.synth_state_dict(cfg["H"], cfg["L"], seed)
    m = models.GraphGatedGCNModel(1, 2, cfg["H"], 16, cfg["L"], 64, cfg["bn"], 16)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    m = m.double().train()
    g = dgl.graph((src, dst), num_nodes=n)
    x = torch.from_numpy(inp["x"]).double().requires_grad_(True)
    e = torch.from_numpy(inp["e"]).double().requires_grad_(True)
    pe = torch.from_numpy(inp["pe"]).double().requires_grad_(True)
    y = torch.from_numpy(inp["y"]).double()
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([float(inp["pos_weight"])], dtype=torch.float64))
    loss = crit(m(g, x, e, pe).squeeze(-1), y)                  # train.py:252-255
    loss.backward()
    assert x.grad is None
    out = dict(src=src, dst=dst, n=np.int64(n), e_raw=inp["e"], pe=inp["pe"], y=inp["y"], pos_weight=inp["pos_weight"],
               seed=np.int64(seed), H=np.int64(cfg["H"]), L=np.int64(cfg["L"]), batch_norm=np.bool_(cfg["bn"]),
               loss64=np.float64(loss.item()), grad_e_raw=e.grad.numpy().copy(), grad_pe=pe.grad.numpy().copy())
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{kind}_{cfg_name}_s{seed}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.relpath(path, HERE)}: E={src.size} N={n} loss64={out['loss64']:.9f} "
          f"|grad_e_raw|={np.linalg.norm(out['grad_e_raw']):.3e} |grad_pe|={np.linalg.norm(out['grad_pe']):.3e} "
          f"size={os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    for kind in ("tiny", "small"):
        for cfg_name in CFGS:
            run_case(kind, cfg_name)
