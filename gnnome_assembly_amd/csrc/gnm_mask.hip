// Read-masking coverage augmentation (include/gnm.h, "read mask"): which reads of a graph a training step keeps, and the
// degrees of the thinned graph.
//
//   gnm_read_mask      nodes 2i and 2i+1 are the two strands of read i; a read is kept or dropped as a whole.  The decision is a
//                      pure function of (key, epoch, graph_index, read): Philox4x32-10 with key (key low, key high) and counter
//                      (q low, q high, graph_index, epoch), q = read >> 2; word read & 3 of the output is the draw x,
//                      u = (x >> 8) * 2^-24, kept iff u < (float)f, compared in fp32.  One call serves four reads = eight nodes:
//                      one thread, one 8-byte store (mask 8-byte aligned and all eight nodes below N), byte stores otherwise.
//   gnm_index_degrees  columns 0 and 1 of the caller's row nperm[i] of a row-major [n, ld] fp32 matrix = the in- and out-degree of
//                      internal node i, read off the index's row pointers.
// Plain loads and stores, no LDS, no atomics, nothing allocated: neither result depends on the grid.
#include "gnm_philox.h"

namespace gnm {

struct MaskArgs {
  int64_t N;
  float f;
  uint32_t k0, k1, graph_index, epoch;
};

__device__ __forceinline__ uint32_t kept_(uint32_t x, float f) { return (float)(x >> 8) * 0x1p-24f < f ? 1u : 0u; }

__global__ __launch_bounds__(kBlock) void read_mask_k(MaskArgs a, uint8_t* mask, int vec) {
  const int64_t groups = (a.N + 7) >> 3;          // eight nodes = four reads = one Philox call
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < groups; q += (int64_t)gridDim.x * kBlock) {
    const uint4 r = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)((uint64_t)q >> 32), a.graph_index, a.epoch), a.k0, a.k1);
    const uint32_t b0 = kept_(r.x, a.f), b1 = kept_(r.y, a.f), b2 = kept_(r.z, a.f), b3 = kept_(r.w, a.f);
    const int64_t base = q << 3;
    if (vec && base + 8 <= a.N) {
      // bytes in address order: node 8q .. 8q+7, both strands of a read alike
      *reinterpret_cast<uint2*>(mask + base) = make_uint2(b0 * 0x0101u | b1 * 0x01010000u, b2 * 0x0101u | b3 * 0x01010000u);
    } else {
      const uint32_t b[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (base + j < a.N) mask[base + j] = (uint8_t)b[j >> 1];
    }
  }
}

__global__ __launch_bounds__(kBlock) void index_degrees_k(int64_t n, const int32_t* __restrict__ in_ptr,
                                                           const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ nperm,
                                                           float* __restrict__ pe, int64_t ld) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t row = nperm ? (int64_t)nperm[i] : i;
    if (row < 0 || row >= n) continue;             // a row outside the matrix is never written
    pe[row * ld] = (float)(in_ptr[i + 1] - in_ptr[i]);
    pe[row * ld + 1] = (float)(out_ptr[i + 1] - out_ptr[i]);
  }
}

}  // namespace gnm

using namespace gnm;

extern "C" int gnm_read_mask(int64_t N, double f, uint64_t key, uint32_t epoch, uint32_t graph_index, uint8_t* mask,
                             void* stream) {
  GNM_CHECK_ARG(N >= 0 && f >= 0.0 && f <= 1.0 && (mask || N == 0),       // (a NaN f fails the comparisons)
                "read_mask: bad argument (N >= 0, 0 <= f <= 1, mask not null)");
  if (N == 0) return 0;
  MaskArgs a;
  a.N = N; a.f = (float)f;                         // rounded once; the comparison u < f is made in fp32
  a.k0 = (uint32_t)key; a.k1 = (uint32_t)(key >> 32); a.graph_index = graph_index; a.epoch = epoch;
  const int vec = ((uintptr_t)mask & 7) == 0;
  const int grid = persistent_grid((N + 7) >> 3, kBlock, 8);
  hipLaunchKernelGGL(read_mask_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, mask, vec);
  GNM_LAUNCH_CHECK("read_mask");
  return 0;
}

extern "C" int gnm_index_degrees(int64_t n, const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* nperm, float* pe,
                                 int64_t ld, void* stream) {
  GNM_CHECK_ARG(n >= 0 && n < INT32_MAX && ld >= 2 && ((in_ptr && out_ptr && pe) || n == 0),
                "index_degrees: bad argument (0 <= n < 2^31 - 1, ld >= 2, in_ptr, out_ptr and pe not null)");
  if (n == 0) return 0;
  const int grid = persistent_grid(n, kBlock, 8);
  hipLaunchKernelGGL(index_degrees_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, n, in_ptr, out_ptr, nperm, pe, ld);
  GNM_LAUNCH_CHECK("index_degrees");
  return 0;
}
