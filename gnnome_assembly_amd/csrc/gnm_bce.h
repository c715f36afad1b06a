// Everything the loss kernels of gnm_symloss.hip (bce_fwd_bwd, bce_stats_fwd_bwd, sym_bce_fwd_bwd) share: the per-element
// BCEWithLogits arithmetic, the confusion-count rule, the per-workgroup sums and the pieces of the finalize kernel.  Every kernel
// that calls these gives the same bits per element and per sum.
#pragma once
#include "gnm_common.h"

namespace gnm {

// The record gnm_bce_stats_fwd_bwd and gnm_sym_bce_fwd_bwd add a step to (gnm.h)
struct BceEpochAcc {
  double loss_sum;
  int64_t steps;
  int64_t counts[4];
};

// Workgroups of the loss kernels for E elements: one per kBlock elements, at most 8 per CU and kMaxPartialBlocks
inline int bce_grid(int64_t E) {
  const int g = ew_grid(E);
  return g < kMaxPartialBlocks ? g : kMaxPartialBlocks;
}

#ifdef __HIPCC__

__device__ __forceinline__ float softplusf_(float x) {
  // log(1 + exp(x)) without overflow: max(x,0) + log1p(exp(-|x|))
  return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}

// round(sigmoid(x)) == 1 (utils.calculate_tfpn; round half to even) holds exactly from this logit on: the smallest fp32 x whose
// fp32 sigmoid is above 0.5 (smaller positive logits give exactly 0.5, which rounds to 0).  Found by bisection over fp32 bit
// patterns against torch.round(torch.sigmoid(x)): tests/test_loss_counts_cpu.py holds the derivation and reads the literal from
// this line.  Bits 0x33c00001.
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

// TP TN FP FN of p = round(sigmoid(x)) against y: a NaN logit and a label that is neither 0 nor 1 fail every comparison and
// are counted nowhere
__device__ __forceinline__ void bce_count_(float x, float y, int& tp, int& tn, int& fp, int& fn) {
  const bool p1 = x >= kSigmoidRoundsUp, p0 = x < kSigmoidRoundsUp, y1 = y == 1.f, y0 = y == 0.f;
  tp += p1 && y1; tn += p0 && y0; fp += p1 && y0; fn += p0 && y1;
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

// The workgroup's four counts into block_counts[blockIdx.x][4]: wave butterfly, one LDS row per wave, threads 0-3 add the rows
__device__ __forceinline__ void bce_block_store_counts_(int tp, int tn, int fp, int fn, int (*cred)[4], int* block_counts) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    tp += __shfl_xor(tp, off, kWave); tn += __shfl_xor(tn, off, kWave);
    fp += __shfl_xor(fp, off, kWave); fn += __shfl_xor(fn, off, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    int* c = cred[threadIdx.x / kWave];
    c[0] = tp; c[1] = tn; c[2] = fp; c[3] = fn;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) s += cred[w][threadIdx.x];
    block_counts[blockIdx.x * 4 + threadIdx.x] = s;
  }
}

// ---- the finalize kernel's pieces (one workgroup of kBlock threads) ----

// Sum of part[0 .. nblk) in every thread: thread t takes part[t], part[t + kBlock], ...; then the tree.  `red` is free again
// on return.
__device__ __forceinline__ double loss_partial_sum_(const double* __restrict__ part, int nblk, double* red) {
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblk; b += kBlock) acc += part[b];
  bce_block_sum_(acc, red);
  const double s = red[0];
  __syncthreads();
  return s;
}

// counts_out = the sum of the block counts, and one step (loss, counts) added to `acc`; either may be NULL, and with both NULL
// block_counts is not read.  The first wave: lane l takes blocks l, l + 64, ...; integers, any order.
__device__ __forceinline__ void loss_counts_finalize_(const int4* __restrict__ block_counts, int nblk, float loss,
                                                      int64_t* __restrict__ counts_out, BceEpochAcc* __restrict__ acc) {
  if ((!counts_out && !acc) || threadIdx.x >= kWave) return;
  long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int b = threadIdx.x; b < nblk; b += kWave) {
    const int4 v = block_counts[b];
    c0 += v.x; c1 += v.y; c2 += v.z; c3 += v.w;
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    c0 += __shfl_xor(c0, off, kWave); c1 += __shfl_xor(c1, off, kWave);
    c2 += __shfl_xor(c2, off, kWave); c3 += __shfl_xor(c3, off, kWave);
  }
  if (threadIdx.x != 0) return;
  if (counts_out) {
    counts_out[0] = c0; counts_out[1] = c1; counts_out[2] = c2; counts_out[3] = c3;
  }
  if (acc) {
    acc->loss_sum += (double)loss;
    acc->steps += 1;
    acc->counts[0] += c0; acc->counts[1] += c1; acc->counts[2] += c2; acc->counts[3] += c3;
  }
}

#endif  // __HIPCC__

}  // namespace gnm
