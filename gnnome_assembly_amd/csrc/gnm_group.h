// Device helpers shared by the integer index kernels (gnm_decision, gnm_cover, gnm_reduce, gnm_align, gnm_induce, and through
// gnm_scan.h -- the one three-phase prefix sum -- gnm_overlap, gnm_seq, gnm_bog, gnm_resolve): wave and workgroup sums, the workgroup
// exclusive scan and the scan of block sums built on it, and the walk of eight lanes per node over the graph index.  Integer only: sums and maxima commute, so every result is a function of the
// inputs alone, whatever the grid.  Workgroups are kBlock threads; "every thread calls it" means all kBlock of them.
#pragma once
#include "gnm_common.h"

namespace gnm {

// ---- wave and workgroup sums ---------------------------------------------------------------------------------------------
// A 64-bit value moves as its two 32-bit halves.
template <int WIDTH>
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
  const unsigned lo = __shfl_xor((unsigned)v, off, WIDTH), hi = __shfl_xor((unsigned)(v >> 32), off, WIDTH);
  return ((unsigned long long)hi << 32) | lo;
}

// The wave's sum (maximum) of v, in every lane.  T: a 32- or 64-bit integer.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "wave_sum: 32- or 64-bit integers");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    if constexpr (sizeof(T) == 8) v += (T)shfl_xor_u64<64>((unsigned long long)v, off);
    else v += __shfl_xor(v, off, 64);
  }
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// The workgroup's sum of v, valid in thread 0.  Every thread calls it; `lds` [kWavesPerBlock] may be reused right after.
template <class T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
  if (threadIdx.x == 0) t = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return t;
}
// ... added to *word by ONE atomic per workgroup, none when it is 0.
template <class T>
__device__ __forceinline__ void block_count_add(T v, T* lds, unsigned long long* word) {
  const T t = block_sum(v, lds);
  if (threadIdx.x == 0 && t) atomicAdd(word, (unsigned long long)t);
}

// ---- workgroup exclusive scan ----------------------------------------------------------------------------------------------
template <int CTRL, class T>
__device__ __forceinline__ T dpp_mov(T v) {                // lanes shifted in from outside a row read 0
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "dpp_mov: 32- or 64-bit integers");
  if constexpr (sizeof(T) == 8) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)v >> 32), CTRL, 0xf, 0xf, true);
    return (T)(((unsigned long long)hi << 32) | lo);
  } else {
    return (T)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
  }
}
// Inclusive scan over the 64 lanes in lane order: row_shr 1/2/4/8 inside the 16-lane rows, then the totals of the rows before
// this lane's row.  `total` = the wave's sum, in every lane.
template <class T>
__device__ __forceinline__ T wave_scan(T v, T& total) {
  v += dpp_mov<0x111>(v);
  v += dpp_mov<0x112>(v);
  v += dpp_mov<0x114>(v);
  v += dpp_mov<0x118>(v);
  const T r0 = __shfl(v, 15, 64), r1 = __shfl(v, 31, 64), r2 = __shfl(v, 47, 64), r3 = __shfl(v, 63, 64);
  const int row = (threadIdx.x & 63) >> 4;
  total = r0 + r1 + r2 + r3;
  return v + (row > 0 ? r0 : 0) + (row > 1 ? r1 : 0) + (row > 2 ? r2 : 0);
}
// Exclusive scan of one value per thread over the workgroup, in thread order; `total` = the workgroup's sum, in every thread.
// Every thread calls it; `lds` [kWavesPerBlock] may be reused right after.  T: int or int64_t.
template <class T>
__device__ __forceinline__ T block_scan_excl(T v, T* lds, T& total) {
  T wt;
  const T incl = wave_scan(v, wt);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = wt;
  __syncthreads();
  T before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWavesPerBlock; ++w) {
    const T x = lds[w];
    before += w < wave ? x : 0;
    total += x;
  }
  __syncthreads();
  return before + incl - v;
}

// The middle phase of a three-phase prefix sum, run by ONE workgroup: bs[0 .. nb) -- the sums of fixed blocks of elements --
// become their exclusive prefix, in place.  Thread t owns `chunk` consecutive block sums, the workgroup scans the kBlock chunk
// totals.  `total` = the sum of all of them, in every thread.
template <class T>
__device__ __forceinline__ void scan_block_sums(T* bs, int64_t nb, T* lds, T& total) {
  const int64_t chunk = (nb + kBlock - 1) / kBlock;
  const int64_t b0 = (int64_t)threadIdx.x * chunk < nb ? (int64_t)threadIdx.x * chunk : nb;
  const int64_t b1 = b0 + chunk < nb ? b0 + chunk : nb;
  T t = 0;
  for (int64_t b = b0; b < b1; ++b) t += bs[b];
  T run = block_scan_excl(t, lds, total);
  for (int64_t b = b0; b < b1; ++b) {
    const T v = bs[b];
    bs[b] = run;
    run += v;
  }
}

// The last phase for a thread that owns the four consecutive elements k0 .. k0 + 3 (k0 a multiple of 4, `out` 16-byte aligned):
// out[k0 + i] = x0 + f[0] + .. + f[i - 1] for the elements below len.
__device__ __forceinline__ void store4_excl(int32_t* out, int64_t k0, int64_t len, int x0, const int f[4]) {
  const int x[4] = {x0, x0 + f[0], x0 + f[0] + f[1], x0 + f[0] + f[1] + f[2]};
  if (k0 + 3 < len) {
    *reinterpret_cast<int4*>(out + k0) = make_int4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k0 + i < len) out[k0 + i] = x[i];
  }
}

// ---- eight lanes per node over the graph index -------------------------------------------------------------------------
constexpr int kGroupLanes = 8;                          // lanes per node: mean degree is about 5
constexpr int kGroupNodes = kBlock / kGroupLanes;       // nodes per workgroup and pass

struct IndexRows {                                      // the index an AssemblyGraph carries, in its internal numbering
  int64_t n, E;
  const int32_t *perm, *isrc, *in_ptr, *out_ptr, *out_pos, *out_dst, *nperm;
};

// the maximum over the group's lanes, in every one of them
__device__ __forceinline__ unsigned long long group_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = kGroupLanes / 2; off > 0; off >>= 1) {
    const unsigned long long o = shfl_xor_u64<kGroupLanes>(v, off);
    v = o > v ? o : v;
  }
  return v;
}

// the row [ptr[i], ptr[i + 1]) clamped to 0 <= lo <= hi <= E
__device__ __forceinline__ void row_clamped(const int32_t* ptr, int i, int E, int& lo, int& hi) {
  lo = ptr[i];
  hi = ptr[i + 1];
  lo = lo < 0 ? 0 : (lo > E ? E : lo);
  hi = hi < lo ? lo : (hi > E ? E : hi);
}

// One lane's share of the candidates of a node in direction D (0: its out-edges, the by-source row; 1: its in-edges): the
// positions first, first + kGroupLanes, .. below hi of the clamped row.  keep(other) is asked about the other end before
// anything is read through the position, so a candidate the caller drops costs no gather; body(p, j, other, eid) gets the
// internal position j and the edge id eid = perm[j], both checked against [0, E).
template <int D, class Keep, class Body>
__device__ __forceinline__ void walk_candidates(const IndexRows& x, int first, int hi, Keep keep, Body body) {
  const unsigned E = (unsigned)x.E;
  for (int p = first; p < hi; p += kGroupLanes) {
    const int j = D ? p : x.out_pos[p];
    const int other = D ? x.isrc[p] : x.out_dst[p];
    if (!keep(other) || (unsigned)j >= E) continue;
    const int eid = x.perm[j];
    if ((unsigned)eid >= E) continue;
    body(p, j, other, eid);
  }
}

// body(i, valid, sub) for the nodes of this workgroup: group g of a pass takes node base + g, lane sub of the group.  base is
// workgroup-uniform: every lane of a wave takes the same number of passes, so a shuffle in the body never meets an idle group
// (`valid` is false for a group past the last node; i is then 0).  decision_stats_k writes this loop out; it says why.
template <class Body>
__device__ __forceinline__ void for_group_nodes(int64_t n, Body body) {
  const int sub = threadIdx.x & (kGroupLanes - 1), grp = threadIdx.x / kGroupLanes;
  for (int64_t base = (int64_t)blockIdx.x * kGroupNodes; base < n; base += (int64_t)gridDim.x * kGroupNodes) {
    const bool valid = base + grp < n;
    body(valid ? (int)(base + grp) : 0, valid, sub);
  }
}

}  // namespace gnm
