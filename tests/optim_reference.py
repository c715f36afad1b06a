"""fp64 numpy restatement of the library's optimizer step (include/gnm.h: gnm_optim_grad_stats + gnm_optim_adam_step): the
non-finite guard, the contributor division, torch's clip_grad_norm_ formula and torch.optim.Adam without weight decay or
amsgrad.  Used by the CPU tier (pinned there to torch.optim.Adam run in float64) and as the oracle of the GPU tier."""
import math

import numpy as np

BLOCK = 2048        # elements per partial of gnm_optim_grad_stats


class AdamRef:
    def __init__(self, p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=0.0):
        self.p = np.asarray(p, np.float64).copy()
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.t = 0
        self.lr, self.betas, self.eps, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        self.total_norm, self.nonfinite, self.skipped, self.clip = 0.0, 0, 0, 1.0

    def step(self, g, count=None):
        """One call: g is the fp32 gradient as stored; count the contributor count (None: no division)."""
        g = np.asarray(g, np.float32).astype(np.float64)
        finite = np.isfinite(g)
        self.nonfinite = int((~finite).sum())
        c = 1.0 if count is None else 1.0 / max(float(count), 1.0)
        self.total_norm = c * math.sqrt(math.fsum(g[finite] ** 2))
        self.clip = min(1.0, self.max_norm / (self.total_norm + 1e-6)) if self.max_norm > 0 else 1.0
        if self.nonfinite:
            self.skipped += 1
            return self
        self.t += 1
        b1, b2 = self.betas
        gh = g * c * self.clip
        self.m = b1 * self.m + (1 - b1) * gh
        self.v = b2 * self.v + (1 - b2) * gh * gh
        self.p = self.p - (self.lr / (1 - b1 ** self.t)) * self.m / (np.sqrt(self.v) / math.sqrt(1 - b2 ** self.t) + self.eps)
        return self


def make_case(n, seed, steps=5):
    """(p0 float32 [n], [g_1 .. g_steps] float32 [n]): parameters ~ N(0, 1); gradient magnitudes log-uniform over 1e-12 .. 1e3 with
    random signs and, from n = 3 on, a block of exact zeros (the analytically zero bias gradients in front of a BatchNorm)."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = []
    for _ in range(steps):
        g = (10.0 ** rng.uniform(-12.0, 3.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        if n >= 3:
            g[n // 3: n // 3 + max(1, n // 4)] = 0.0
        grads.append(g)
    return p0, grads


def ulp32(x):
    """One fp32 unit in the last place at magnitude |x|."""
    return float(np.spacing(np.float32(abs(float(x)))))
