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
// Kernel.  Mean degree is about 5, so a node takes kGroupLanes = 8 lanes, not a wave (gnm_group.h): a wave serves eight consecutive
// nodes side by side, a group's lanes stride over its node's candidates (a node with more than eight loops), and three xor-shuffles inside
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
#include "gnm_group.h"
#include "gnm_key.h"                                    // dec_key_: shared with gnm_cover.hip

namespace gnm {

constexpr int kDecCounters = 7;                         // per direction; the record's order
enum { kDead = 0, kForced, kForcedOk, kBranch, kBranchSolvable, kBranchOk, kBranchNan };

struct DecArgs {
  IndexRows ix;
  const float *scores, *y;
  int32_t* best[2];                                     // succ, pred; either may be NULL
};

// One direction of one node (D = 0: successors, 1: predecessors).  Every lane of the group calls this together; `valid` is
// group-uniform.  cnt: the thread's 2 x kDecCounters counters.
template <int D>
__device__ __forceinline__ void dec_node_(const DecArgs& a, int i, bool valid, int sub, int row, unsigned* cnt) {
  unsigned long long best = 0ull;
  unsigned num = 0u, anyp = 0u;
  if (valid) {
    int lo, hi;
    row_clamped(D ? a.ix.in_ptr : a.ix.out_ptr, i, (int)a.ix.E, lo, hi);
    walk_candidates<D>(
        a.ix, lo + sub, hi, [&](int other) { return other != i; },     // a self loop is no candidate
        [&](int, int, int, int eid) {
          const unsigned yp = (a.y && a.y[eid] == 1.0f) ? 1u : 0u;     // any other label, NaN included: not 1
          const unsigned long long w = ((unsigned long long)dec_key_(a.scores[eid]) << 32) | ((0x7fffffffu - (unsigned)eid) << 1) | yp;
          best = w > best ? w : best;
          num += 1u;
          anyp |= yp;
        });
  }
#pragma unroll
  for (int off = kGroupLanes / 2; off > 0; off >>= 1) {                // the maximum as group_max_u64 does it, its steps shared
    const unsigned long long o = shfl_xor_u64<kGroupLanes>(best, off);
    best = o > best ? o : best;
    num += __shfl_xor(num, off, kGroupLanes);
    anyp |= __shfl_xor(anyp, off, kGroupLanes);
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
  // for_group_nodes written out, and the three shuffles of a step kept together in dec_node_: through the shared forms the
  // compiler orders this loop differently, and the launch measured 151 us against 146 us (7.5 M edges, windows within 5 us).
  const int sub = threadIdx.x & (kGroupLanes - 1), grp = threadIdx.x / kGroupLanes;
  for (int64_t base = (int64_t)blockIdx.x * kGroupNodes; base < a.ix.n; base += (int64_t)gridDim.x * kGroupNodes) {
    const int64_t i64 = base + grp;
    const bool valid = i64 < a.ix.n;
    const int i = valid ? (int)i64 : 0;
    int row = -1;                                       // the caller's id of node i; -1: outside [0, n), never written
    if (valid && sub == 0) {
      const int64_t v = a.ix.nperm ? (int64_t)a.ix.nperm[i] : i64;
      row = (v >= 0 && v < a.ix.n) ? (int)v : -1;
    }
    dec_node_<0>(a, i, valid, sub, row, cnt);
    dec_node_<1>(a, i, valid, sub, row, cnt);
  }
#pragma unroll
  for (int k = 0; k < 2 * kDecCounters; ++k) {
    const unsigned v = wave_sum(cnt[k]);
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
  if (index_size_check("decision_stats", n, E, "the index holds 32-bit positions") ||
      record_check("decision_stats", record, "gnm_decision_record"))
    return -1;
  GNM_CHECK_ARG(n == 0 || (in_ptr && out_ptr), "decision_stats: in_ptr and out_ptr must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || (perm && isrc && out_pos && out_dst && scores),
                "decision_stats: perm, isrc, out_pos, out_dst and scores must not be null when E > 0");
  DecArgs a;
  a.ix = IndexRows{n, E, perm, isrc, in_ptr, out_ptr, out_pos, out_dst, nperm};
  a.scores = scores; a.y = y;
  a.best[0] = best_succ; a.best[1] = best_pred;
  const int grid = persistent_grid(n, kGroupNodes, 8);
  hipLaunchKernelGGL(decision_stats_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, (unsigned long long*)record);
  GNM_LAUNCH_CHECK("decision_stats");
  return 0;
}
