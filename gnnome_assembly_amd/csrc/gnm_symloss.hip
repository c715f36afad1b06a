// The loss kernels (gfx950): plain BCE, BCE with confusion counts, and the symmetry loss of the published GNNome training recipe.
//
//   bce_fwd_bwd         train.py:210-211,253-255 BCEWithLogitsLoss(pos_weight), mean, + dloss/dlogit
//   bce_stats_fwd_bwd   the same, + TP/TN/FP/FN (utils.py:217-223) and the epoch sums, from the same pass
//   sym_bce_fwd_bwd     l_k = bce(o_k, y_k) + bce(r_k, y_k) + alpha |o_k - r_k|, L = mean_k l_k, with dL/do, dL/dr, the three
//                       part means, TP..FN of `o` and the epoch sums: the original and the edge-reversed scores in one pass
//   mirror_add / mirror_gather   g[i] += s[pi[i]] / out[i] = s[pi[i]]: the parameter mirror (models.mirror_index) applied to a
//                       flat gradient / parameter buffer.
//
// The three loss entries promise each other's bits: bce_stats_fwd_bwd gives bce_fwd_bwd's loss and gradient, and with alpha = 0
// the two BCE parts and both gradients of sym_bce_fwd_bwd are those of bce_fwd_bwd on `o` and on `r`.  They keep that by sharing
// code, not by copying it: the per-element arithmetic, the count rule and the block sums are gnm_bce.h's, the grid is bce_grid,
// tile k (kBlock consecutive elements) belongs to workgroup k % grid with element k * kBlock + t added to thread t's sum in
// increasing k, and one kernel (loss_finalize_k) adds the workgroups' partials.
// Workspace: double[Q][kMaxPartialBlocks] loss partials (Q = 1, or 3: bce(o), bce(r), |o - r|), then int32[kMaxPartialBlocks][4]
// block counts.  gnm_bce_fwd_bwd's has no counts and only its grid's partials.
#include "gnm_common.h"
#include "gnm_bce.h"

namespace gnm {

constexpr size_t loss_ws_bytes(int Q) { return (size_t)kMaxPartialBlocks * (Q * sizeof(double) + 4 * sizeof(int32_t)); }

// STATS: also the block's TP TN FP FN, and gscore may be NULL (no per-edge store).  Elements, their order per thread and the
// loss arithmetic are the same for both instantiations: the loss partials are bit-identical.
template <bool STATS>
__global__ __launch_bounds__(kBlock) void bce_fwd_bwd_k(int64_t E, const float* __restrict__ x,
                                                        const float* __restrict__ y, float pw,
                                                        float inv_e, float* __restrict__ gscore,
                                                        double* __restrict__ ws) {
  __shared__ double red[kBlock];
  __shared__ int cred[kWavesPerBlock][4];
  double acc = 0.0;
  int tp = 0, tn = 0, fp = 0, fn = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < E; i += (int64_t)gridDim.x * kBlock) {
    const float xi = x[i], yi = y[i];
    float p, q;
    acc += (double)bce_term_(xi, yi, pw, p, q);
    if (!STATS || gscore) gscore[i] = bce_grad_(yi, pw, p, q, inv_e);
    if (STATS) bce_count_(xi, yi, tp, tn, fp, fn);
  }
  bce_block_sum_(acc, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = red[0];
  if (STATS) bce_block_store_counts_(tp, tn, fp, fn, cred, reinterpret_cast<int*>(ws + kMaxPartialBlocks));
}

struct SymElem {
  float bo, br, ab, go, gr;
};

// One edge.  alpha_e = (float)(alpha / E).  d == 0 (and a NaN d) adds nothing to either gradient: torch.abs's subgradient.
__device__ __forceinline__ SymElem sym_elem_(float oi, float ri, float yi, float pw, float inv_e, float alpha_e) {
#pragma clang fp contract(off)
  SymElem s;
  float p, q;
  s.bo = bce_term_(oi, yi, pw, p, q);
  s.go = bce_grad_(yi, pw, p, q, inv_e);
  s.br = bce_term_(ri, yi, pw, p, q);
  s.gr = bce_grad_(yi, pw, p, q, inv_e);
  const float d = oi - ri;
  s.ab = fabsf(d);
  const float t = d > 0.f ? alpha_e : (d < 0.f ? -alpha_e : 0.f);
  if (t != 0.f) {          // alpha = 0 or o == r: the plain kernel's bits, a -0 gradient included
    s.go += t;
    s.gr -= t;
  }
  return s;
}

// Tile k (kBlock consecutive edges) belongs to workgroup k % gridDim.x, and edge k * kBlock + t is added to thread t's sums in
// increasing k: the order of bce_fwd_bwd_k.  VEC: four full tiles of the workgroup per trip, one per wave, each lane with one
// 16-byte load per input and one 16-byte store per gradient; the loss terms cross to their owning thread through LDS, which
// adds them in the same order.  The ragged end (and everything, without VEC) goes element by element: same bits.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void sym_bce_k(int64_t E, const float* __restrict__ o, const float* __restrict__ r,
                                                    const float* __restrict__ y, float pw, float inv_e, float alpha_e,
                                                    float* __restrict__ g_o, float* __restrict__ g_r,
                                                    double* __restrict__ ws) {
  __shared__ double red[kBlock];
  __shared__ __align__(16) float stage[3][kWavesPerBlock][kBlock];
  __shared__ int cred[kWavesPerBlock][4];
  double a_o = 0.0, a_r = 0.0, a_d = 0.0;
  int tp = 0, tn = 0, fp = 0, fn = 0;
  const int64_t G = gridDim.x;
  int64_t k = blockIdx.x;
  if (VEC) {
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
    for (; (k + (kWavesPerBlock - 1) * G + 1) * kBlock <= E; k += kWavesPerBlock * G) {
      const int64_t base = (k + w * G) * kBlock + 4 * l;
      const float4 vo = ld4(o + base), vr = ld4(r + base), vy = ld4(y + base);
      const SymElem e0 = sym_elem_(vo.x, vr.x, vy.x, pw, inv_e, alpha_e), e1 = sym_elem_(vo.y, vr.y, vy.y, pw, inv_e, alpha_e);
      const SymElem e2 = sym_elem_(vo.z, vr.z, vy.z, pw, inv_e, alpha_e), e3 = sym_elem_(vo.w, vr.w, vy.w, pw, inv_e, alpha_e);
      if (g_o) {
        st4(g_o + base, make_float4(e0.go, e1.go, e2.go, e3.go));
        st4(g_r + base, make_float4(e0.gr, e1.gr, e2.gr, e3.gr));
      }
      bce_count_(vo.x, vy.x, tp, tn, fp, fn); bce_count_(vo.y, vy.y, tp, tn, fp, fn);
      bce_count_(vo.z, vy.z, tp, tn, fp, fn); bce_count_(vo.w, vy.w, tp, tn, fp, fn);
      st4(&stage[0][w][4 * l], make_float4(e0.bo, e1.bo, e2.bo, e3.bo));
      st4(&stage[1][w][4 * l], make_float4(e0.br, e1.br, e2.br, e3.br));
      st4(&stage[2][w][4 * l], make_float4(e0.ab, e1.ab, e2.ab, e3.ab));
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kWavesPerBlock; ++j) {
        a_o += (double)stage[0][j][threadIdx.x];
        a_r += (double)stage[1][j][threadIdx.x];
        a_d += (double)stage[2][j][threadIdx.x];
      }
      __syncthreads();
    }
  }
  for (int64_t i = k * kBlock + threadIdx.x; i < E; i += G * kBlock) {
    const float oi = o[i], yi = y[i];
    const SymElem e = sym_elem_(oi, r[i], yi, pw, inv_e, alpha_e);
    if (g_o) {
      g_o[i] = e.go;
      g_r[i] = e.gr;
    }
    bce_count_(oi, yi, tp, tn, fp, fn);
    a_o += (double)e.bo;
    a_r += (double)e.br;
    a_d += (double)e.ab;
  }
  bce_block_sum_(a_o, red);
  if (threadIdx.x == 0) ws[blockIdx.x] = red[0];
  __syncthreads();
  bce_block_sum_(a_r, red);
  if (threadIdx.x == 0) ws[kMaxPartialBlocks + blockIdx.x] = red[0];
  __syncthreads();
  bce_block_sum_(a_d, red);
  if (threadIdx.x == 0) ws[2 * kMaxPartialBlocks + blockIdx.x] = red[0];
  bce_block_store_counts_(tp, tn, fp, fn, cred, reinterpret_cast<int*>(ws + 3 * kMaxPartialBlocks));
}

// One workgroup of kBlock: the Q sums of the workgroups' partials, the loss from them, then the counts
template <int Q>
__global__ __launch_bounds__(kBlock) void loss_finalize_k(const double* __restrict__ ws, int nblk, double inv_e, double alpha,
                                                          float* __restrict__ loss_out, float* __restrict__ parts_out,
                                                          int64_t* __restrict__ counts_out, BceEpochAcc* __restrict__ epoch_acc) {
  __shared__ double red[kBlock];
  double S[Q];
  for (int q = 0; q < Q; ++q) S[q] = loss_partial_sum_(ws + q * kMaxPartialBlocks, nblk, red);
  float loss;
  if constexpr (Q == 1) {
    loss = (float)(S[0] * inv_e);
  } else {
    loss = (float)((S[0] + S[1] + alpha * S[2]) * inv_e);
    if (threadIdx.x == 0) {
      parts_out[0] = (float)(S[0] * inv_e);
      parts_out[1] = (float)(S[1] * inv_e);
      parts_out[2] = (float)(S[2] * inv_e);
    }
  }
  if (threadIdx.x == 0) loss_out[0] = loss;
  loss_counts_finalize_(reinterpret_cast<const int4*>(ws + Q * kMaxPartialBlocks), nblk, loss, counts_out, epoch_acc);
}

// pi is a permutation of [0, n): an entry outside it is skipped, never followed
__global__ void mirror_add_k(int64_t n, float* __restrict__ g, const float* __restrict__ s, const int32_t* __restrict__ pi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = pi[i];
    if (j >= 0 && j < n) g[i] += s[j];
  }
}

__global__ void mirror_gather_k(int64_t n, float* __restrict__ out, const float* __restrict__ s, const int32_t* __restrict__ pi) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = pi[i];
    if (j >= 0 && j < n) out[i] = s[j];
  }
}

}  // namespace gnm

using namespace gnm;

extern "C" int gnm_bce_fwd_bwd(int64_t E, const float* scores, const float* y, float pos_weight,
                               float* loss_out, float* gscore, void* ws, size_t ws_bytes,
                               void* stream) {
  GNM_CHECK_ARG(E > 0 && scores && y && loss_out && gscore, "bce_fwd_bwd: bad argument");
  const int grid = bce_grid(E);
  GNM_CHECK_ARG(ws && ws_bytes >= (size_t)grid * sizeof(double), "bce_fwd_bwd: workspace too small");
  hipLaunchKernelGGL(bce_fwd_bwd_k<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, E, scores, y,
                     pos_weight, (float)(1.0 / (double)E), gscore, (double*)ws);
  GNM_LAUNCH_CHECK("bce_fwd_bwd");
  hipLaunchKernelGGL(loss_finalize_k<1>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)ws, grid,
                     1.0 / (double)E, 0.0, loss_out, (float*)nullptr, (int64_t*)nullptr, (BceEpochAcc*)nullptr);
  GNM_LAUNCH_CHECK("bce finalize");
  return 0;
}

extern "C" size_t gnm_bce_stats_workspace_bytes(void) { return loss_ws_bytes(1); }

extern "C" int gnm_bce_stats_fwd_bwd(int64_t E, const float* scores, const float* y, float pos_weight,
                                     float* loss_out, float* gscore, int64_t* counts_out, void* epoch_acc,
                                     void* ws, size_t ws_bytes, void* stream) {
  static_assert(sizeof(BceEpochAcc) == 48, "gnm.h: epoch_acc is 48 bytes");
  GNM_CHECK_ARG(E > 0 && scores && y && loss_out && counts_out, "bce_stats_fwd_bwd: bad argument");
  GNM_CHECK_ARG(ws && ws_bytes >= loss_ws_bytes(1), "bce_stats_fwd_bwd: workspace too small");
  GNM_CHECK_ARG((uintptr_t)ws % 16 == 0 && (!epoch_acc || (uintptr_t)epoch_acc % 8 == 0) && (uintptr_t)counts_out % 8 == 0,
                "bce_stats_fwd_bwd: ws must be 16-byte, counts_out and epoch_acc 8-byte aligned");
  const int grid = bce_grid(E);
  hipLaunchKernelGGL(bce_fwd_bwd_k<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, E, scores, y,
                     pos_weight, (float)(1.0 / (double)E), gscore, (double*)ws);
  GNM_LAUNCH_CHECK("bce_stats_fwd_bwd");
  hipLaunchKernelGGL(loss_finalize_k<1>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)ws, grid,
                     1.0 / (double)E, 0.0, loss_out, (float*)nullptr, counts_out, (BceEpochAcc*)epoch_acc);
  GNM_LAUNCH_CHECK("bce stats finalize");
  return 0;
}

extern "C" size_t gnm_sym_bce_workspace_bytes(void) { return loss_ws_bytes(3); }

extern "C" int gnm_sym_bce_fwd_bwd(int64_t E, const float* org, const float* rev, const float* y, float pos_weight, float alpha,
                                   float* loss_out, float* parts_out, float* g_org, float* g_rev, int64_t* counts_out,
                                   void* epoch_acc, void* ws, size_t ws_bytes, void* stream) {
  static_assert(sizeof(BceEpochAcc) == 48, "gnm.h: epoch_acc is 48 bytes");
  GNM_CHECK_ARG(E > 0 && org && rev && y && loss_out && parts_out, "sym_bce_fwd_bwd: bad argument");
  GNM_CHECK_ARG((g_org == nullptr) == (g_rev == nullptr), "sym_bce_fwd_bwd: g_org and g_rev must both be given or both be NULL");
  GNM_CHECK_ARG(alpha >= 0.f && alpha <= 3.402823466e38f, "sym_bce_fwd_bwd: alpha must be finite and >= 0");
  GNM_CHECK_ARG(ws && ws_bytes >= loss_ws_bytes(3), "sym_bce_fwd_bwd: workspace too small");
  GNM_CHECK_ARG((uintptr_t)ws % 16 == 0 && (uintptr_t)epoch_acc % 8 == 0 && (uintptr_t)counts_out % 8 == 0,
                "sym_bce_fwd_bwd: ws must be 16-byte, counts_out and epoch_acc 8-byte aligned");
  const int grid = bce_grid(E);
  const double inv_e = 1.0 / (double)E;
  const float alpha_e = (float)((double)alpha * inv_e);
  const bool vec = ((uintptr_t)org | (uintptr_t)rev | (uintptr_t)y | (uintptr_t)g_org | (uintptr_t)g_rev) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(sym_bce_k<true>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, E, org, rev, y, pos_weight,
                       (float)inv_e, alpha_e, g_org, g_rev, (double*)ws);
  else
    hipLaunchKernelGGL(sym_bce_k<false>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, E, org, rev, y, pos_weight,
                       (float)inv_e, alpha_e, g_org, g_rev, (double*)ws);
  GNM_LAUNCH_CHECK("sym_bce_fwd_bwd");
  hipLaunchKernelGGL(loss_finalize_k<3>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (const double*)ws, grid, inv_e, (double)alpha,
                     loss_out, parts_out, counts_out, (BceEpochAcc*)epoch_acc);
  GNM_LAUNCH_CHECK("sym_bce finalize");
  return 0;
}

extern "C" int gnm_mirror_add(int64_t n, float* g, const float* scratch, const int32_t* pi, void* stream) {
  GNM_CHECK_ARG(n >= 0 && n <= INT32_MAX && (n == 0 || (g && scratch && pi)), "mirror_add: bad argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(mirror_add_k, dim3(ew_grid(n)), dim3(kBlock), 0, (hipStream_t)stream, n, g, scratch, pi);
  GNM_LAUNCH_CHECK("mirror_add");
  return 0;
}

extern "C" int gnm_mirror_gather(int64_t n, float* out, const float* src, const int32_t* pi, void* stream) {
  GNM_CHECK_ARG(n >= 0 && n <= INT32_MAX && (n == 0 || (out && src && pi)), "mirror_gather: bad argument");
  GNM_CHECK_ARG(n == 0 || out != src, "mirror_gather: out must not be src");
  if (n == 0) return 0;
  hipLaunchKernelGGL(mirror_gather_k, dim3(ew_grid(n)), dim3(kBlock), 0, (hipStream_t)stream, n, out, src, pi);
  GNM_LAUNCH_CHECK("mirror_gather");
  return 0;
}
