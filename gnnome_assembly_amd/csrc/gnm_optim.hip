// The optimizer step over the flat parameter / gradient buffers (train.py:209,256-258: torch.optim.Adam, no weight decay, no
// amsgrad) with the gradient's global norm (clip_grad_norm_), the division by a contributor count and a non-finite guard, in two
// launches and without a host read-back:
//
//   gnm_optim_grad_stats   one streaming pass over g: per block of kOptBlock = 2048 elements the fp64 sum of squares of the finite
//                          entries and the count of the non-finite ones -> workspace[b]; it also copies the step count into the
//                          workspace header (see "the step count" below).
//   gnm_optim_adam_step    every workgroup combines the block partials itself (same order in every workgroup, so all of them
//                          derive the same scalars: no finalise launch), then streams g, p, m, v.
//
// Determinism.  A partial is a function of its 2048 elements alone: thread i of the block owns elements 4i .. 4i+3 and
// 1024 + 4i .. 1024 + 4i+3 (whether they are loaded as two float4 or, in the tail block or from an unaligned buffer, one by one),
// adds their squares in that order, and the 256 thread sums go through one xor-butterfly per wave and the four waves in wave
// order.  The combination of nblk partials is a function of nblk alone: thread i adds partials i, i + 256, ... in ascending
// order, then the same butterfly.  Which workgroup processes which block (the grid, the CU count, gnm_set_occupancy_cap) decides
// only WHERE a value is computed.  The element update is independent per element.  No atomics.
//
// Arithmetic.  The scalars (c, total_norm, clip, the bias corrections) are fp64, formed by thread 0 of each workgroup.  The
// element update is evaluated in fp64 from the fp32 g, p, m, v and rounded once per stored value: the kernel is bound by its
// seven 4-byte streams per element, the fp64 sqrt and divide hide behind them, and each stored value is then within half an ulp
// of the exact update of the stored inputs -- no operation order to argue about.
//
// The step count is a device fp32 scalar that the call advances.  A workgroup that starts late must still see the count of
// BEFORE the call, so no workgroup of the step kernel reads `step`: grad_stats copies it into the workspace header, the step
// kernel reads the copy, and exactly one thread (workgroup 0, thread 0) writes `step` = copy + 1 with an ordinary store.
#include "gnm_common.h"

namespace gnm {

constexpr int kOptBlock = 2048;                 // elements per partial: fixed, NOT a launch parameter
constexpr int kOptHeader = 16;                  // workspace: {float t; 12 bytes pad} then nblk x {double sumsq; int64_t nonfinite}

struct OptPartial { double sumsq; long long nonfinite; };
struct OptStats { double total_norm; long long nonfinite; long long skipped; double clip; };   // gnm.h: gnm_optim_stats

static inline int64_t opt_blocks(int64_t n) { return (n + kOptBlock - 1) / kOptBlock; }

__device__ __forceinline__ bool finite_(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the block's (sum, count) in every thread; `lds` holds 2 * kWavesPerBlock doubles
__device__ __forceinline__ void block_sum_(double& s, long long& c, double* lds) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    s += __shfl_xor(s, off, 64);
    c += __shfl_xor(c, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();                               // a previous use of lds has been read
  if ((threadIdx.x & 63) == 0) {
    lds[wave] = s;
    reinterpret_cast<long long*>(lds)[kWavesPerBlock + wave] = c;
  }
  __syncthreads();
  s = 0.0; c = 0;
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w) {
    s += lds[w];
    c += reinterpret_cast<const long long*>(lds)[kWavesPerBlock + w];
  }
}

__device__ __forceinline__ void stat_add_(float x, double& s, long long& c) {
  if (finite_(x)) s += (double)x * (double)x; else c += 1;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void optim_grad_stats_k(int64_t n, const float* __restrict__ g, const float* step,
                                                            unsigned char* ws) {
  __shared__ double lds[2 * kWavesPerBlock];
  OptPartial* part = reinterpret_cast<OptPartial*>(ws + kOptHeader);
  if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<float*>(ws) = *step;
  const int64_t nblk = (n + kOptBlock - 1) / kOptBlock;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    double s = 0.0;
    long long c = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t i = b * kOptBlock + h * (kOptBlock / 2) + 4 * (int64_t)threadIdx.x;
      if (VEC && i + 4 <= n) {
        const float4 v = ld4(g + i);
        stat_add_(v.x, s, c); stat_add_(v.y, s, c); stat_add_(v.z, s, c); stat_add_(v.w, s, c);
      } else {
        for (int k = 0; k < 4; ++k)
          if (i + k < n) stat_add_(g[i + k], s, c);
      }
    }
    block_sum_(s, c, lds);
    if (threadIdx.x == 0) { part[b].sumsq = s; part[b].nonfinite = c; }
  }
}

struct OptScalars {          // what thread 0 of a workgroup derives and the others read from LDS
  double scale;              // c * clip: g_hat = g * scale
  double b1, one_b1, b2, one_b2, step_size, inv_bc2_sqrt, eps;
  int skip;
};

struct OptArgs {
  int64_t n;
  float *p, *g, *m, *v, *step;
  OptStats* stats;
  const unsigned char* ws;
  const float* inv_count;
  double lr, beta1, beta2, eps, max_norm;
  int zero_grad;
};

__device__ __forceinline__ void adam1_(const OptScalars& q, float g, float& p, float& m, float& v) {
  const double gh = (double)g * q.scale;
  const double md = q.b1 * (double)m + q.one_b1 * gh;
  const double vd = q.b2 * (double)v + q.one_b2 * gh * gh;
  const double pd = (double)p - q.step_size * md / (sqrt(vd) * q.inv_bc2_sqrt + q.eps);
  p = (float)pd; m = (float)md; v = (float)vd;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void optim_adam_step_k(OptArgs a) {
  __shared__ double lds[2 * kWavesPerBlock];
  __shared__ OptScalars sc;
  const OptPartial* part = reinterpret_cast<const OptPartial*>(a.ws + kOptHeader);
  const int64_t nblk = (a.n + kOptBlock - 1) / kOptBlock;
  double ss = 0.0;
  long long nf = 0;
  for (int64_t b = threadIdx.x; b < nblk; b += kBlock) { ss += part[b].sumsq; nf += part[b].nonfinite; }
  block_sum_(ss, nf, lds);
  if (threadIdx.x == 0) {
    double c = 1.0;
    if (a.inv_count) c = 1.0 / fmax((double)*a.inv_count, 1.0);
    const double total_norm = c * sqrt(ss);
    const double clip = a.max_norm > 0.0 ? fmin(1.0, a.max_norm / (total_norm + 1e-6)) : 1.0;     // clip_grad_norm_
    const double t = (double)*reinterpret_cast<const float*>(a.ws) + 1.0;
    const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
    sc.scale = c * clip;
    sc.b1 = a.beta1; sc.one_b1 = 1.0 - a.beta1; sc.b2 = a.beta2; sc.one_b2 = 1.0 - a.beta2;
    sc.step_size = a.lr / bc1;
    sc.inv_bc2_sqrt = 1.0 / sqrt(bc2);
    sc.eps = a.eps;
    sc.skip = nf > 0;
    if (blockIdx.x == 0) {          // the one writer of the device scalars
      a.stats->total_norm = total_norm;
      a.stats->nonfinite = nf;
      a.stats->clip = clip;
      if (nf > 0) a.stats->skipped = a.stats->skipped + 1;
      else *a.step = (float)t;
    }
  }
  __syncthreads();
  const OptScalars q = sc;
  if (q.skip && !a.zero_grad) return;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t i = b * kOptBlock + h * (kOptBlock / 2) + 4 * (int64_t)threadIdx.x;
      if (VEC && i + 4 <= a.n) {
        if (!q.skip) {
          const float4 g4 = ld4(a.g + i);
          float4 p4 = ld4(a.p + i), m4 = ld4(a.m + i), v4 = ld4(a.v + i);
          adam1_(q, g4.x, p4.x, m4.x, v4.x); adam1_(q, g4.y, p4.y, m4.y, v4.y);
          adam1_(q, g4.z, p4.z, m4.z, v4.z); adam1_(q, g4.w, p4.w, m4.w, v4.w);
          st4(a.p + i, p4); st4(a.m + i, m4); st4(a.v + i, v4);
        }
        if (a.zero_grad) st4(a.g + i, f4(0.f));
      } else {
        for (int k = 0; k < 4; ++k) {
          const int64_t j = i + k;
          if (j >= a.n) break;
          if (!q.skip) {
            float pj = a.p[j], mj = a.m[j], vj = a.v[j];
            adam1_(q, a.g[j], pj, mj, vj);
            a.p[j] = pj; a.m[j] = mj; a.v[j] = vj;
          }
          if (a.zero_grad) a.g[j] = 0.f;
        }
      }
    }
  }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace gnm

using namespace gnm;

extern "C" size_t gnm_optim_workspace_bytes(int64_t n) {
  return n < 0 ? 0 : (size_t)kOptHeader + (size_t)opt_blocks(n) * sizeof(OptPartial);
}

extern "C" int gnm_optim_grad_stats(int64_t n, const float* g, const float* step, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  GNM_CHECK_ARG(n >= 0 && g && step && workspace && ((uintptr_t)workspace & 7) == 0,
                "optim_grad_stats: bad argument (n >= 0; g, step and workspace not null; workspace 8-byte aligned)");
  GNM_CHECK_ARG(workspace_bytes >= gnm_optim_workspace_bytes(n), "optim_grad_stats: workspace of %zu bytes, %zu needed",
                workspace_bytes, gnm_optim_workspace_bytes(n));
  if (n == 0) return 0;
  const int grid = persistent_grid(opt_blocks(n), 1, 8);
  if (aligned16(g))
    hipLaunchKernelGGL(optim_grad_stats_k<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, n, g, step,
                       (unsigned char*)workspace);
  else
    hipLaunchKernelGGL(optim_grad_stats_k<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, n, g, step,
                       (unsigned char*)workspace);
  GNM_LAUNCH_CHECK("optim_grad_stats");
  return 0;
}

extern "C" int gnm_optim_adam_step(int64_t n, float* p, float* g, float* m, float* v, float* step, void* stats,
                                   const void* workspace, size_t workspace_bytes, double lr, double beta1, double beta2, double eps,
                                   double max_norm, const float* inv_count, int zero_grad, void* stream) {
  GNM_CHECK_ARG(n >= 0 && p && g && m && v && step && stats && workspace && ((uintptr_t)workspace & 7) == 0 &&
                    ((uintptr_t)stats & 7) == 0,
                "optim_adam_step: bad argument (n >= 0; p, g, m, v, step, stats and workspace not null; stats and workspace "
                "8-byte aligned)");
  GNM_CHECK_ARG(workspace_bytes >= gnm_optim_workspace_bytes(n), "optim_adam_step: workspace of %zu bytes, %zu needed",
                workspace_bytes, gnm_optim_workspace_bytes(n));
  // (a NaN fails every comparison)
  GNM_CHECK_ARG(lr >= 0.0 && lr <= 3.0e38 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 &&
                    eps <= 3.0e38 && max_norm >= 0.0 && max_norm <= 1.0e300,
                "optim_adam_step: bad hyper-parameter (lr >= 0, 0 <= beta1 < 1, 0 <= beta2 < 1, eps >= 0, max_norm >= 0, all "
                "finite)");
  if (n == 0) return 0;
  OptArgs a;
  a.n = n; a.p = p; a.g = g; a.m = m; a.v = v; a.step = step;
  a.stats = (OptStats*)stats; a.ws = (const unsigned char*)workspace; a.inv_count = inv_count;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.max_norm = max_norm; a.zero_grad = zero_grad != 0;
  const int grid = persistent_grid(opt_blocks(n), 1, 8);
  if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v))
    hipLaunchKernelGGL(optim_adam_step_k<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(optim_adam_step_k<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
  GNM_LAUNCH_CHECK("optim_adam_step");
  return 0;
}
