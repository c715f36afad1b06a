// Walk-decision accuracy: for every node the out-edge and the in-edge the greedy decode would follow, and how often that choice
// is a correct edge -- one launch over the index the graph already carries (include/gnm.h, "walk decisions").
//
// Candidates of internal node i.  Successors: the by-source range p in [out_ptr[i], out_ptr[i+1]), internal position
// j = out_pos[p], edge id perm[j], other end out_dst[p].  Predecessors: j in [in_ptr[i], in_ptr[i+1]), edge id perm[j], other
// end isrc[j].  A self loop (other end == i) is no candidate: the decode drops self loops from its candidates.  Duplicate
// edges are separate candidates.
//
// Choice.  The candidate with the largest score, the lowest edge id among equals.  Scores are compared on the order-preserving
// map of IEEE bits onto unsigned integers that gnm_rank_hist documents, all 32 bits of it:
//
//   key(x) = 0 if x is NaN, else u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000),  u = bits(x == -0 ? +0 : x)
//
// -0 and +0 tie (they are equal as numbers), a denormal keeps its bits, -inf has the lowest key a number takes (0x007FFFFF),
// and 0 -- the image of no number -- is given to every NaN: a NaN orders below every number and NaNs tie.  A candidate is the
// 64-bit word  key << 32 | (0x7FFFFFFF - eid) << 1 | (y[eid] == 1),  so "largest score, then lowest edge id" is a plain
// unsigned maximum (edge ids are distinct: the label bit never decides) and the winner carries its label along.  Every
// candidate word is >= 4 (eid <= 2^31 - 3), so 0 stands for "no candidate".
//
// Kernel.  Mean degree is about 5, so a node takes kDecLanes = 8 lanes, not a wave: a wave serves eight consecutive nodes side
// by side, a group's lanes stride over its node's candidates (a node with more than eight loops), and three xor-shuffles inside
// the group give every lane the group's maximum, candidate count and "some candidate has y == 1".  The group's first lane
// writes the two table entries (through nperm: the caller's numbering) and counts the node.  A group handles both directions
// of its node; the two chains of dependent loads are independent and overlap.
// Counters: 14 per thread in registers, summed over the wave by shuffles, over the workgroup in LDS (uint32: a workgroup counts
// fewer than 2^31 nodes), then ONE 64-bit integer atomic per non-zero counter and workgroup.  Integer sums commute: the record
// is a function of the inputs alone, whatever the grid, gnm_set_occupancy_cap or the order in which the atomics land.  The
// tables are plain stores of values that depend on the node alone.  No float atomics, no workspace, nothing allocated.
//
// Bounds.  Every value read from an index array is checked before it addresses anything: row pointers are clamped to
// 0 <= lo <= hi <= E, a position or edge id outside [0, E) drops the candidate, a row nperm[i] outside [0, n) is never written.
#include "gnm_common.h"
#include "gnm_key.h"                                    // dec_key_: shared with gnm_cover.hip

namespace gnm {

constexpr int kDecLanes = 8;                            // lanes per node
constexpr int kDecNodes = kBlock / kDecLanes;           // nodes per workgroup and round
constexpr int kDecCounters = 7;                         // per direction; the record's order
enum { kDead = 0, kForced, kForcedOk, kBranch, kBranchSolvable, kBranchOk, kBranchNan };

struct DecArgs {
  int64_t n, E;
  const int32_t *perm, *isrc, *in_ptr, *out_ptr, *out_pos, *out_dst, *nperm;
  const float *scores, *y;
  int32_t* best[2];                                     // succ, pred; either may be NULL
};

__device__ __forceinline__ unsigned long long dec_shfl_xor_(unsigned long long v, int off) {
  const unsigned lo = __shfl_xor((unsigned)v, off, kDecLanes), hi = __shfl_xor((unsigned)(v >> 32), off, kDecLanes);
  return ((unsigned long long)hi << 32) | lo;
}

// One direction of one node (D = 0: successors, 1: predecessors).  Every lane of the group calls this together; `valid` is
// group-uniform.  cnt: the thread's 2 x kDecCounters counters.
template <int D>
__device__ __forceinline__ void dec_node_(const DecArgs& a, int i, bool valid, int sub, int row, unsigned* cnt) {
  const int E = (int)a.E;
  unsigned long long best = 0ull;
  unsigned num = 0u, anyp = 0u;
  if (valid) {
    const int32_t* ptr = D ? a.in_ptr : a.out_ptr;
    int lo = ptr[i], hi = ptr[i + 1];
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < lo ? lo : (hi > E ? E : hi);
    for (int p = lo + sub; p < hi; p += kDecLanes) {
      const int j = D ? p : a.out_pos[p];
      const int other = D ? a.isrc[p] : a.out_dst[p];
      if (other == i || (unsigned)j >= (unsigned)E) continue;          // a self loop; a position outside the index
      const int eid = a.perm[j];
      if ((unsigned)eid >= (unsigned)E) continue;
      const unsigned yp = (a.y && a.y[eid] == 1.0f) ? 1u : 0u;         // any other label, NaN included: not 1
      const unsigned long long w = ((unsigned long long)dec_key_(a.scores[eid]) << 32) | ((0x7fffffffu - (unsigned)eid) << 1) | yp;
      best = w > best ? w : best;
      num += 1u;
      anyp |= yp;
    }
  }
#pragma unroll
  for (int off = kDecLanes / 2; off > 0; off >>= 1) {
    const unsigned long long o = dec_shfl_xor_(best, off);
    best = o > best ? o : best;
    num += __shfl_xor(num, off, kDecLanes);
    anyp |= __shfl_xor(anyp, off, kDecLanes);
  }
  if (!valid || sub != 0) return;
  unsigned* c = cnt + D * kDecCounters;
  const unsigned ok = (unsigned)best & 1u;
  if (num == 0u) {
    c[kDead] += 1u;
  } else if (num == 1u) {
    c[kForced] += 1u;
    c[kForcedOk] += ok;
  } else {
    c[kBranch] += 1u;
    c[kBranchSolvable] += anyp;
    c[kBranchOk] += ok;
    c[kBranchNan] += (best >> 32) == 0ull ? 1u : 0u;
  }
  if (a.best[D] && row >= 0)
    a.best[D][row] = num ? (int32_t)(0x7fffffffu - (((unsigned)best) >> 1)) : -1;
}

__global__ __launch_bounds__(kBlock) void decision_stats_k(DecArgs a, unsigned long long* rec) {
  __shared__ unsigned tot[2 * kDecCounters];
  if (threadIdx.x < 2 * kDecCounters) tot[threadIdx.x] = 0u;
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(rec + 2 * kDecCounters, 1ull);          // calls
  unsigned cnt[2 * kDecCounters];
#pragma unroll
  for (int k = 0; k < 2 * kDecCounters; ++k) cnt[k] = 0u;
  const int sub = threadIdx.x & (kDecLanes - 1), grp = threadIdx.x / kDecLanes;
  // base is workgroup-uniform: every lane of a wave takes the same number of rounds, so the shuffles never meet an idle group
  for (int64_t base = (int64_t)blockIdx.x * kDecNodes; base < a.n; base += (int64_t)gridDim.x * kDecNodes) {
    const int64_t i64 = base + grp;
    const bool valid = i64 < a.n;
    const int i = valid ? (int)i64 : 0;
    int row = -1;                                       // the caller's id of node i; -1: outside [0, n), never written
    if (valid && sub == 0) {
      const int64_t v = a.nperm ? (int64_t)a.nperm[i] : i64;
      row = (v >= 0 && v < a.n) ? (int)v : -1;
    }
    dec_node_<0>(a, i, valid, sub, row, cnt);
    dec_node_<1>(a, i, valid, sub, row, cnt);
  }
#pragma unroll
  for (int k = 0; k < 2 * kDecCounters; ++k) {
    unsigned v = cnt[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], v);
  }
  __syncthreads();
  if (threadIdx.x < 2 * kDecCounters && tot[threadIdx.x]) atomicAdd(rec + threadIdx.x, (unsigned long long)tot[threadIdx.x]);
}

}  // namespace gnm

using namespace gnm;

extern "C" int gnm_decision_stats(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst,
                                  const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                                  const int32_t* nperm, const float* scores, const float* y, void* record, int32_t* best_succ,
                                  int32_t* best_pred, void* stream) {
  (void)idst;                                           // the index travels whole; the destination of in-edge j of node i is i
  GNM_CHECK_ARG(n >= 0 && E >= 0 && n < INT32_MAX && E < INT32_MAX,
                "decision_stats: n = %lld, E = %lld: expected 0 <= n, E < 2^31 - 1 (the index holds 32-bit positions)", (long long)n,
                (long long)E);
  GNM_CHECK_ARG(record && ((uintptr_t)record & 7) == 0, "decision_stats: record must be a non-null, 8-byte aligned gnm_decision_record");
  GNM_CHECK_ARG(n == 0 || (in_ptr && out_ptr), "decision_stats: in_ptr and out_ptr must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || (perm && isrc && out_pos && out_dst && scores),
                "decision_stats: perm, isrc, out_pos, out_dst and scores must not be null when E > 0");
  DecArgs a;
  a.n = n; a.E = E;
  a.perm = perm; a.isrc = isrc; a.in_ptr = in_ptr; a.out_ptr = out_ptr; a.out_pos = out_pos; a.out_dst = out_dst; a.nperm = nperm;
  a.scores = scores; a.y = y;
  a.best[0] = best_succ; a.best[1] = best_pred;
  const int grid = persistent_grid(n, kDecNodes, 8);
  hipLaunchKernelGGL(decision_stats_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, (unsigned long long*)record);
  GNM_LAUNCH_CHECK("decision_stats");
  return 0;
}
