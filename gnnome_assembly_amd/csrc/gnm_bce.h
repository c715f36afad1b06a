// Per-element BCEWithLogits arithmetic and the block sum of the loss kernels, shared by gnm_misc.hip (bce_fwd_bwd,
// bce_stats_fwd_bwd) and gnm_symloss.hip (sym_bce_fwd_bwd): every kernel that calls these gives the same bits per element.
#pragma once
#include "gnm_common.h"

namespace gnm {

#ifdef __HIPCC__

__device__ __forceinline__ float softplusf_(float x) {
  // log(1 + exp(x)) without overflow: max(x,0) + log1p(exp(-|x|))
  return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}

// round(sigmoid(x)) == 1 (utils.calculate_tfpn; round half to even) holds exactly from this logit on: the smallest fp32 x whose
// fp32 sigmoid is above 0.5 (smaller positive logits give exactly 0.5, which rounds to 0).  Found by bisection over fp32 bit
// patterns against torch.round(torch.sigmoid(x)): tests/test_loss_counts_cpu.py holds the derivation.  Bits 0x33c00001.
// (gnm_misc.hip spells the literal once more, where that test reads it, and asserts at compile time that the two agree.)
constexpr float kSigmoidRoundsUp = 0x1.800002p-24f;

// One logit / label pair: the loss term, and sigma(x) / 1 - sigma(x) for the gradient.  The two products and their sum are
// kept as three roundings (no fma contraction), here and in bce_grad_: which of them the compiler would fuse depends on the code
// around the call, and every kernel that calls these must give the same bits.
__device__ __forceinline__ float bce_term_(float xi, float yi, float pw, float& p, float& q) {
#pragma clang fp contract(off)
  p = sigmoid_ieee_(xi);
  // 1 - p: for x > 0 as e^-x / (1 + e^-x), where 1.f - p cancels (it is 0 from x ~ 17 on, where 1 - p is ~4e-8)
  const float em = expf(-fabsf(xi));
  q = xi > 0.f ? em / (1.f + em) : 1.f - p;
  return pw * yi * softplusf_(-xi) + (1.f - yi) * softplusf_(xi);
}
__device__ __forceinline__ float bce_grad_(float yi, float pw, float p, float q, float inv_e) {
#pragma clang fp contract(off)
  return (-pw * yi * q + (1.f - yi) * p) * inv_e;
}

// Sum of the block's `acc` in red[0] (tree over kBlock slots, fixed order)
__device__ __forceinline__ void bce_block_sum_(double acc, double* red) {
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
}

#endif  // __HIPCC__

// The record gnm_bce_stats_fwd_bwd and gnm_sym_bce_fwd_bwd add a step to (gnm.h)
struct BceEpochAcc {
  double loss_sum;
  int64_t steps;
  int64_t counts[4];
};

// Workgroups of the loss kernels for E elements: one per kBlock elements, at most 8 per CU and kMaxPartialBlocks
inline int bce_grid(int64_t E) {
  int64_t g = (E + kBlock - 1) / kBlock;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (g > cap) g = cap;
  if (g > kMaxPartialBlocks) g = kMaxPartialBlocks;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace gnm
