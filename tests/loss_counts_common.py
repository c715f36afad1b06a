"""Shared by test_loss_counts_cpu.py and test_gpu_loss_counts.py: the torch expression the fused loss kernel's TP/TN/FP/FN
counts must equal, the threshold rule the kernel uses in its place, and the boundary logits both files test on."""
import os
import re

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the smallest fp32 logit with round(sigmoid(x)) == 1; test_loss_counts_cpu.py derives it and checks the source against it
X_STAR = float.fromhex("0x1.800002p-24")
WINDOW = 4096               # fp32 steps checked on either side of X_STAR and of 0


def source_constant():
    """kSigmoidRoundsUp as the kernel's source spells it (a hex float)."""
    src = open(os.path.join(REPO, "gnnome_assembly_amd", "csrc", "gnm_bce.h")).read()
    m = re.search(r"constexpr\s+float\s+kSigmoidRoundsUp\s*=\s*(-?0x[0-9a-fA-F.]+p[-+]?\d+)f\s*;", src)
    assert m, "kSigmoidRoundsUp must be a hex float literal in gnm_bce.h"
    return float.fromhex(m.group(1))


def bits_to_f32(bits) -> torch.Tensor:
    return torch.from_numpy(np.asarray(bits, dtype=np.int64).astype(np.uint32).view(np.float32).copy())


def f32_bits(x: float) -> int:
    return int(np.array([x], np.float32).view(np.uint32)[0])


def steps_from_zero(k):
    """The fp32 value k steps from +0 (k < 0: k steps below -0): sign-magnitude bit patterns."""
    k = np.asarray(k, dtype=np.int64)
    return bits_to_f32(np.where(k >= 0, k, (-k) | 0x80000000))


def torch_counts(x: torch.Tensor, y: torch.Tensor):
    """utils.calculate_tfpn's expression (train.tfpn_counts) on CPU tensors, as four Python ints."""
    p = torch.round(torch.sigmoid(x))
    return (int(((p == 1) & (y == 1)).sum()), int(((p == 0) & (y == 0)).sum()),
            int(((p == 1) & (y == 0)).sum()), int(((p == 0) & (y == 1)).sum()))


def rule_counts(x: torch.Tensor, y: torch.Tensor, x_star: float = X_STAR):
    """The kernel's rule: p1 = x >= X_STAR, p0 = x < X_STAR (a NaN fails both)."""
    p1, p0 = x >= x_star, x < x_star
    return (int((p1 & (y == 1)).sum()), int((p0 & (y == 0)).sum()), int((p1 & (y == 0)).sum()), int((p0 & (y == 1)).sum()))


def boundary_logits() -> torch.Tensor:
    """+-inf, nan, +-0, the threshold and its neighbours first (so that a short slice of this still holds them), then every fp32
    value within WINDOW steps of X_STAR and of 0."""
    b = f32_bits(X_STAR)
    head = torch.cat([bits_to_f32([b, b - 1, b + 1]), torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")]),
                      bits_to_f32([1, 0x80000001, 0x007fffff, 0x00800000])])
    return torch.cat([head, bits_to_f32(np.arange(b - WINDOW, b + WINDOW + 1)), steps_from_zero(np.arange(-WINDOW, WINDOW + 1))])


def make_case(E: int, seed: int, clean: bool = False):
    """Logits randn x 3 with a leading slice of boundary_logits(); labels Bernoulli(0.8) with a few 0.5 and NaN entries.
    clean: no non-finite logit and no NaN label (the loss is finite), everything else as before."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(E, generator=g) * 3.0
    b = boundary_logits()
    k = min(b.numel(), max(E // 2, 1))
    x[:k] = b[:k]
    y = (torch.rand(E, generator=g) < 0.8).float()
    odd = torch.randperm(E, generator=g)[:max(2, E // 50) if E >= 8 else 0]      # E = 1: the one label stays 0 or 1
    y[odd[0::2]] = 0.5
    y[odd[1::2]] = float("nan")
    if clean:
        x = torch.where(torch.isfinite(x), x, torch.randn(E, generator=g) * 3.0)
        y = torch.where(torch.isnan(y), torch.full_like(y, 0.5), y)
    return x, y
