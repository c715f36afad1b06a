"""CPU: pin the oracle's input gradients -- d loss / d e_raw and d loss / d pe of oracle.model_forward in fp64 autograd --
against the reference's own values (tests/golden/make_golden_input_grads.py -> tests/golden/input_grads/)."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, sd_to_torch, rel_l2
from gnnome_assembly_amd import synth
from oracle import gatedgcn_oracle as orc

INPUT_GRADS = os.path.join(GOLDEN, "input_grads")
CASES = sorted(f for f in os.listdir(INPUT_GRADS) if f.endswith(".npz"))


def test_every_case_is_there():
    assert CASES == sorted(f"{k}_{c}_s0.npz" for k in ("tiny", "small") for c in ("h128l8", "h256l2", "h64l1", "h32l2ln"))


@pytest.mark.parametrize("fname", CASES)
def test_oracle_input_grads_match_reference(fname):
    z = np.load(os.path.join(INPUT_GRADS, fname))
    H, L, seed, bn = int(z["H"]), int(z["L"]), int(z["seed"]), bool(z["batch_norm"])
    p = sd_to_torch(synth.synth_state_dict(H, L, seed), torch.float64)
    e = torch.from_numpy(z["e_raw"]).double().requires_grad_(True)
    pe = torch.from_numpy(z["pe"]).double().requires_grad_(True)
    s = orc.model_forward(p, torch.from_numpy(z["src"]), torch.from_numpy(z["dst"]), int(z["n"]), e, pe, bn)
    loss = orc.bce_loss(s, torch.from_numpy(z["y"]).double(), float(z["pos_weight"]))
    loss.backward()
    assert abs(loss.item() - float(z["loss64"])) < 1e-12
    assert e.grad.shape == z["grad_e_raw"].shape and pe.grad.shape == z["grad_pe"].shape
    assert np.linalg.norm(z["grad_e_raw"]) > 0 and np.linalg.norm(z["grad_pe"]) > 0
    assert rel_l2(e.grad.numpy(), z["grad_e_raw"]) <= 1e-10
    assert rel_l2(pe.grad.numpy(), z["grad_pe"]) <= 1e-10
