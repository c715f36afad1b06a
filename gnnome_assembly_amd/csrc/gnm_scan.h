// The exclusive prefix sum of the index kernels (gnm_overlap, gnm_seq, gnm_bog, gnm_resolve), in three phases over fixed blocks of
// PER * kBlock elements: scan_sums_k (every block's sum), scan_middle_k (workgroup s turns the block sums of sequence s into their
// exclusive prefix, in place: gnm_group.h's scan_block_sums), scan_apply_k (in-block scan + the block's offset); scan_launch launches
// them.  T: int32_t or int64_t; PER: 1 or 4 consecutive elements per thread; S: 1 or 2 sequences of one length scanned together.
// No workgroup waits for another, no atomics, no float arithmetic: every result is a function of the inputs alone, whatever the grid.
// A user is a struct U : ScanUser, passed to the kernels by value (every thread owns a copy it may write to), with
//   load(x, int64_t k0, bool first, T (&v)[S][PER])   the thread's values at elements k0 .. k0 + PER - 1 of every sequence, 0 at and
//                                past x.n.  `first`: the sums phase -- a producer fused into the scan (seq) stores and counts there.
//   total(x, int s, T total)     thread 0 of the middle phase's workgroup s: what becomes of sequence s's total.
//   skip()                       true (in every thread of all three launches alike): do nothing at all.  ScanUser: false.
//   sums_end(T* lds)             every thread after the sums phase's last block; lds [kWavesPerBlock] is free.  ScanUser: nothing.
// gnm_induce.hip keeps three kernels of its own: it walks five sequences of two lengths through combined launches (ind_locate) and
// writes flag bytes in its sums phase, which would take parameters and branches that no user here needs.
#pragma once
#include "gnm_group.h"

namespace gnm {

// x: the scanned length, per sequence the block sums [nb] and the output [n] (16-byte aligned when PER == 4), the scan blocks
template <class T, int S>
struct ScanArrays {
  int64_t n;
  T *bsum[S], *out[S];
  int64_t nb;                            // scan_launch fills it in
};

template <class T, int S>
struct ScanUser {
  using Arrays = ScanArrays<T, S>;
  __device__ __forceinline__ bool skip() const { return false; }
  __device__ __forceinline__ void sums_end(T*) {}
};

// the scan blocks of n elements, and the bytes of one sequence's block sums as a workspace array
template <int PER>
inline int64_t scan_blocks(int64_t n) { return (n + PER * kBlock - 1) / (PER * kBlock); }
template <class T, int PER>
inline size_t scan_bsum_bytes(int64_t n) { return ws_pad((size_t)scan_blocks<PER>(n) * sizeof(T)); }

template <class T, int PER>
__device__ __forceinline__ T scan_sum_(const T (&v)[PER]) {
  if constexpr (PER == 1) return v[0];
  else return v[0] + v[1] + v[2] + v[3];
}

template <class T, int PER, int S, class U>
__global__ __launch_bounds__(kBlock) void scan_sums_k(U u, ScanArrays<T, S> x) {
  static_assert(PER == 1 || (PER == 4 && sizeof(T) == 4), "scan: one element per thread, or four int32 (store4_excl)");
  __shared__ T lds[kWavesPerBlock];
  if (u.skip()) return;
  for (int64_t b = blockIdx.x; b < x.nb; b += gridDim.x) {
    T v[S][PER];
    u.load(x, b * (PER * kBlock) + PER * (int64_t)threadIdx.x, true, v);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const T t = block_sum(scan_sum_<T, PER>(v[s]), lds);
      if (threadIdx.x == 0) x.bsum[s][b] = t;
    }
  }
  u.sums_end(lds);
}

template <class T, int S, class U>
__global__ __launch_bounds__(kBlock) void scan_middle_k(U u, ScanArrays<T, S> x) {
  __shared__ T lds[kWavesPerBlock];
  if (u.skip()) return;
  const int s = S == 1 ? 0 : (int)blockIdx.x;
  T total;
  scan_block_sums(x.bsum[s], x.nb, lds, total);
  if (threadIdx.x == 0) u.total(x, s, total);
}

template <class T, int PER, int S, class U>
__global__ __launch_bounds__(kBlock) void scan_apply_k(U u, ScanArrays<T, S> x) {
  __shared__ T lds[kWavesPerBlock];
  if (u.skip()) return;
  for (int64_t b = blockIdx.x; b < x.nb; b += gridDim.x) {
    const int64_t k0 = b * (PER * kBlock) + PER * (int64_t)threadIdx.x;
    T v[S][PER], total;
    u.load(x, k0, false, v);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const T x0 = x.bsum[s][b] + block_scan_excl(scan_sum_<T, PER>(v[s]), lds, total);
      if constexpr (PER == 4) store4_excl(x.out[s], k0, x.n, x0, v[s]);
      else if (k0 < x.n) x.out[s][k0] = x0;
    }
  }
}

// sums and apply on persistent_grid(nb, 1, 8), the middle phase on S workgroups; n == 0: the middle phase alone, its totals 0
template <class T, int PER, int S, class U>
inline void scan_launch(const U& u, ScanArrays<T, S> x, hipStream_t st) {
  x.nb = scan_blocks<PER>(x.n);
  const dim3 blk(kBlock), grid(persistent_grid(x.nb, 1, 8));
  if (x.nb > 0) hipLaunchKernelGGL((scan_sums_k<T, PER, S, U>), grid, blk, 0, st, u, x);
  hipLaunchKernelGGL((scan_middle_k<T, S, U>), dim3(S), blk, 0, st, u, x);
  if (x.nb > 0) hipLaunchKernelGGL((scan_apply_k<T, PER, S, U>), grid, blk, 0, st, u, x);
}

}  // namespace gnm
