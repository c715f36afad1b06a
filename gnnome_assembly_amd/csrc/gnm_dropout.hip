// Node-output dropout of the layer stack (gated_gcn_full.py:154) without stored masks: the keep decision of an element is a pure
// function of (seed, step, layer, caller's node id, channel), so the backward, a checkpoint recomputation and another rank's
// inspection all re-derive the same mask from five integers.
//
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), key = (seed_lo,
//   seed_hi), counter = (q_lo, q_hi, layer, step) with q = (v * H + c) >> 2 as a 64-bit value -- v the CALLER's node id of the row, H
//   the model's real width, c the channel.  Word c & 3 of the output is the element's draw x; u = (x >> 8) * 2^-24 (exact in fp32);
//   the element is kept iff u >= p (fp32 comparison).  Kept elements are multiplied by float(1 / (1 - p)), dropped ones become +0.
//
// With H a multiple of 4 (every width the modules run natively, and any sensible model width) the four channels 4g .. 4g+3 of a
// row share one Philox call and one float4: one thread per call.  Any other H takes the same definition element by element (one
// call per element; there the elements (v, c) and (v', c') with equal q and equal c & 3 share a draw -- a property of the
// definition, not of this kernel).  Plain loads and stores, no LDS, no atomics: the result does not depend on the grid.
#include "gnm_philox.h"        // philox4x32_10

namespace gnm {

struct DropArgs {
  int64_t N;
  int H;                    // the model's real width: the mask function's H
  const int32_t* node_ids;  // internal row -> caller's node id (null: identity)
  float p;
  uint32_t k0, k1, step, layer;
};

__device__ __forceinline__ bool keep_(uint32_t x, float p) { return (float)(x >> 8) * 0x1p-24f >= p; }

__device__ __forceinline__ uint64_t node_of(const DropArgs& a, int64_t row) {
  return a.node_ids ? (uint64_t)(uint32_t)a.node_ids[row] : (uint64_t)row;
}

// the four draws of channels 4g .. 4g+3 of node v (H % 4 == 0: they are the four words of one call)
__device__ __forceinline__ uint4 draws4(const DropArgs& a, uint64_t v, int g) {
  const uint64_t q = v * (uint64_t)(a.H >> 2) + (uint64_t)g;
  return philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), a.layer, a.step), a.k0, a.k1);
}

// the draw of channel c of node v, any H
__device__ __forceinline__ uint32_t draw1(const DropArgs& a, uint64_t v, int c) {
  const uint64_t q = (v * (uint64_t)a.H + (uint64_t)c) >> 2;
  const uint4 r = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), a.layer, a.step), a.k0, a.k1);
  const int w = c & 3;
  return w == 0 ? r.x : (w == 1 ? r.y : (w == 2 ? r.z : r.w));
}

// y = mask * x * scale, one float4 per thread and Philox call; y == x allowed (each thread reads its four elements before it
// writes them)
__global__ __launch_bounds__(kBlock) void node_dropout_apply4_k(DropArgs a, int64_t ld, const float* x, float* y, float scale) {
  const int G = a.H >> 2;
  const int64_t total = a.N * G;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t row = i / G;
    const int g = (int)(i - row * G);
    const uint4 r = draws4(a, node_of(a, row), g);
    const int64_t off = row * ld + 4 * g;
    const float4 v = ld4(x + off);
    st4(y + off, make_float4(keep_(r.x, a.p) ? v.x * scale : 0.f, keep_(r.y, a.p) ? v.y * scale : 0.f,
                             keep_(r.z, a.p) ? v.z * scale : 0.f, keep_(r.w, a.p) ? v.w * scale : 0.f));
  }
}

__global__ __launch_bounds__(kBlock) void node_dropout_apply1_k(DropArgs a, int64_t ld, const float* x, float* y, float scale) {
  const int64_t total = a.N * a.H;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t row = i / a.H;
    const int c = (int)(i - row * a.H);
    const int64_t off = row * ld + c;
    y[off] = keep_(draw1(a, node_of(a, row), c), a.p) ? x[off] * scale : 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void node_dropout_mask4_k(DropArgs a, uint8_t* mask) {
  const int G = a.H >> 2;
  const int64_t total = a.N * G;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t row = i / G;
    const uint4 r = draws4(a, node_of(a, row), (int)(i - row * G));
    // [N,H] contiguous with H % 4 == 0: element 4 i is 4-byte aligned when the tensor is
    *reinterpret_cast<uchar4*>(mask + 4 * i) = make_uchar4(keep_(r.x, a.p), keep_(r.y, a.p), keep_(r.z, a.p), keep_(r.w, a.p));
  }
}

__global__ __launch_bounds__(kBlock) void node_dropout_mask1_k(DropArgs a, uint8_t* mask) {
  const int64_t total = a.N * a.H;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t row = i / a.H;
    mask[i] = keep_(draw1(a, node_of(a, row), (int)(i - row * a.H)), a.p);
  }
}

static inline bool drop_args(DropArgs& a, int64_t N, int H, const int32_t* node_ids, double p, uint64_t seed, uint32_t step,
                             int layer) {
  if (!(N >= 0 && H > 0 && layer >= 0 && p >= 0.0 && p < 1.0)) return false;     // (a NaN p fails the comparisons)
  a.N = N; a.H = H; a.node_ids = node_ids; a.p = (float)p;       // the comparison u >= p is made in fp32
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.step = step; a.layer = (uint32_t)layer;
  return true;
}

}  // namespace gnm

using namespace gnm;

extern "C" int gnm_node_dropout_apply(int64_t N, int H, int64_t ld, const float* x, float* y, const int32_t* node_ids, double p,
                                      uint64_t seed, uint32_t step, int layer, void* stream) {
  DropArgs a;
  GNM_CHECK_ARG(drop_args(a, N, H, node_ids, p, seed, step, layer) && ld >= H && x && y,
                "node_dropout_apply: bad argument (N >= 0, 0 < H <= ld, 0 <= p < 1, layer >= 0, x and y not null)");
  if (N == 0) return 0;
  const float scale = (float)(1.0 / (1.0 - p));      // rounded once
  const bool vec = H % 4 == 0 && ld % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  const int64_t items = vec ? N * (H / 4) : N * H;
  const int grid = persistent_grid(items, kBlock, 8);
  if (vec)
    hipLaunchKernelGGL(node_dropout_apply4_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, ld, x, y, scale);
  else
    hipLaunchKernelGGL(node_dropout_apply1_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, ld, x, y, scale);
  GNM_LAUNCH_CHECK("node_dropout_apply");
  return 0;
}

extern "C" int gnm_node_dropout_mask(int64_t N, int H, uint8_t* mask, const int32_t* node_ids, double p, uint64_t seed,
                                     uint32_t step, int layer, void* stream) {
  DropArgs a;
  GNM_CHECK_ARG(drop_args(a, N, H, node_ids, p, seed, step, layer) && mask,
                "node_dropout_mask: bad argument (N >= 0, H > 0, 0 <= p < 1, layer >= 0, mask not null)");
  if (N == 0) return 0;
  const bool vec = H % 4 == 0 && ((uintptr_t)mask & 3) == 0;
  const int64_t items = vec ? N * (H / 4) : N * H;
  const int grid = persistent_grid(items, kBlock, 8);
  if (vec)
    hipLaunchKernelGGL(node_dropout_mask4_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, mask);
  else
    hipLaunchKernelGGL(node_dropout_mask1_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, mask);
  GNM_LAUNCH_CHECK("node_dropout_mask");
  return 0;
}
