// Transitive reduction of the candidate edges ahead of the cover decoders (include/gnm.h, "transitive support"): Myers' string-graph
// step on the index the graph already carries.  One launch, no workspace.
//
// A candidate is the cover kernel's: an edge k = (u -> w) with u != w, scores[k] no NaN and scores[k] >= min_logit.  For every
// edge k = (a -> c) with a != c, candidate or not, support[k] counts the out-edges j = (a -> b) of a with
//   j a candidate, b != a, b != c, prefix_length[j] < prefix_length[k] (strictly), and some candidate m = (b -> c) -- with
//   fuzz >= 0 one for which |prefix_length[j] + prefix_length[m] - prefix_length[k]| <= fuzz in (wrapping) int64.
// Parallel a -> b edges each count; several parallel b -> c edges make one witness; a self loop has support 0.  k is reduced when it
// is a candidate and support[k] > 0: masked_scores[k] is then a quiet NaN, else scores[k].  The strict < is what keeps two edges
// from removing each other through one another (b -> c and c -> b may both exist) and what spares a node's out-edge of uniquely
// smallest prefix.
//
// Kernel.  Eight lanes per source node a (gnm_group.h); the lanes stride over the positions p of a's by-source row
// (edge k), and every lane walks the whole row again (position q, edge j).  All eight lanes meet the same j in the same order, so
// its loads are broadcasts and the branch on "j is a candidate" is group-uniform; the lanes differ in c alone.  The out-rows are
// stored by ascending internal position, i.e. by ascending internal destination inside a row: "a candidate b -> c exists" is a
// lower-bound binary search for c in out_dst[out_ptr[b] .. out_ptr[b+1]) and a scan of the equal range (the parallel b -> c edges).
// d^2 log d steps per node of out-degree d.  Every edge has exactly one writer -- the lane that owns its position in its source's
// row -- so support and masked_scores are plain vector stores through perm.
// Record: seven counters per thread in registers, summed over the wave by shuffles, over the workgroup in LDS, then ONE 64-bit
// integer atomic per non-zero word and workgroup (max_support: an integer maximum).  Integer sums and maxima commute: the record,
// like the two arrays, is a function of the inputs alone, whatever the grid or gnm_set_occupancy_cap.  No float arithmetic (a score
// enters through dec_key_ and the comparison with min_logit), no cooperative launch, no workgroup waits for another.
//
// Bounds.  Row pointers are clamped to 0 <= lo <= hi <= E; a position or edge id outside [0, E) and a destination outside [0, n)
// drop the edge (it is not counted and nothing is written for it) or the witness before they address anything.
#include "gnm_common.h"
#include "gnm_group.h"
#include "gnm_key.h"

namespace gnm {

enum { kRedEdges = 0, kRedCandidates, kRedReduced, kRedLabel1, kRedSelfLoops, kRedCounters };   // the 32-bit thread counters
// the record's words: edges, candidates, reduced, reduced_label1, witnesses, max_support, self_loops, calls
enum { kRecEdges = 0, kRecCandidates, kRecReduced, kRecLabel1, kRecWitnesses, kRecMaxSupport, kRecSelfLoops, kRecCalls };

struct RedArgs {
  IndexRows ix;                                         // the by-source half of it is all this reads
  const float *scores, *y;
  const int64_t* pl;
  float min_logit;
  int64_t fuzz;
  int32_t* support;
  float* masked;
};

__device__ __forceinline__ bool red_candidate_(const RedArgs& a, float s) { return dec_key_(s) != 0u && s >= a.min_logit; }

// Is there a candidate edge m = (b -> c) -- and, with fuzz >= 0, one with |pj + pl[m] - pk| <= fuzz?
__device__ __forceinline__ bool red_closes_(const RedArgs& a, int b, int c, int64_t pj, int64_t pk) {
  const unsigned E = (unsigned)a.ix.E;
  int lo, end;
  row_clamped(a.ix.out_ptr, b, (int)a.ix.E, lo, end);
  for (int hi = end; lo < hi;) {                        // lower bound of c in the ascending destinations of b's row
    const int mid = lo + ((hi - lo) >> 1);
    if (a.ix.out_dst[mid] < c) lo = mid + 1; else hi = mid;
  }
  for (int t = lo; t < end && a.ix.out_dst[t] == c; ++t) {
    const int jm = a.ix.out_pos[t];
    if ((unsigned)jm >= E) continue;
    const int em = a.ix.perm[jm];
    if ((unsigned)em >= E) continue;
    if (!red_candidate_(a, a.scores[em])) continue;
    if (a.fuzz < 0) return true;
    const int64_t d = (int64_t)((uint64_t)pj + (uint64_t)a.pl[em] - (uint64_t)pk);
    if (d <= a.fuzz && d >= -a.fuzz) return true;
  }
  return false;
}

__global__ __launch_bounds__(kBlock) void transitive_support_k(RedArgs a, unsigned long long* rec) {
  __shared__ unsigned tot[kRedCounters + 1];            // the counters, then max_support
  __shared__ unsigned long long wit;
  if (threadIdx.x <= kRedCounters) tot[threadIdx.x] = 0u;
  if (threadIdx.x == 0) wit = 0ull;
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(rec + kRecCalls, 1ull);
  unsigned cnt[kRedCounters];
#pragma unroll
  for (int k = 0; k < kRedCounters; ++k) cnt[k] = 0u;
  unsigned long long witnesses = 0ull;
  unsigned max_support = 0u;
  const unsigned E = (unsigned)a.ix.E, n = (unsigned)a.ix.n;
  const int sub = threadIdx.x & (kGroupLanes - 1), grp = threadIdx.x / kGroupLanes;
  for (int64_t base = (int64_t)blockIdx.x * kGroupNodes; base < a.ix.n; base += (int64_t)gridDim.x * kGroupNodes) {
    const int64_t i64 = base + grp;
    if (i64 >= a.ix.n) continue;                        // no shuffle inside the loop: an idle group may leave
    const int i = (int)i64;
    int lo, hi;
    row_clamped(a.ix.out_ptr, i, (int)E, lo, hi);
    walk_candidates<0>(
        a.ix, lo + sub, hi, [&](int c) { return (unsigned)c < n; },    // outside the index: the edge is dropped
        [&](int, int, int c, int ek) {
          const float sk = a.scores[ek];
          cnt[kRedEdges] += 1u;
          unsigned sup = 0u;
          bool cand = false;
          if (c == i) {
            cnt[kRedSelfLoops] += 1u;
          } else {
            cand = red_candidate_(a, sk);
            const int64_t pk = a.pl[ek];
            for (int q = lo; q < hi; ++q) {
              const int b = a.ix.out_dst[q], jj = a.ix.out_pos[q];
              if (b == i || b == c || (unsigned)b >= n || (unsigned)jj >= E) continue;
              const int ej = a.ix.perm[jj];
              if ((unsigned)ej >= E) continue;
              const int64_t pj = a.pl[ej];
              if (!(pj < pk) || !red_candidate_(a, a.scores[ej])) continue;
              if (red_closes_(a, b, c, pj, pk)) sup += 1u;
            }
          }
          const bool reduced = cand && sup > 0u;
          a.support[ek] = (int32_t)sup;
          if (a.masked) a.masked[ek] = reduced ? __uint_as_float(0x7fc00000u) : sk;
          cnt[kRedCandidates] += cand ? 1u : 0u;
          cnt[kRedReduced] += reduced ? 1u : 0u;
          cnt[kRedLabel1] += (reduced && a.y && a.y[ek] == 1.0f) ? 1u : 0u;
          witnesses += sup;
          max_support = sup > max_support ? sup : max_support;
        });
  }
#pragma unroll
  for (int k = 0; k < kRedCounters; ++k) {
    const unsigned v = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&tot[k], v);
  }
  {
    const unsigned long long s = wave_sum(witnesses);
    const unsigned m = wave_max(max_support);
    if ((threadIdx.x & 63) == 0) {
      if (s) atomicAdd(&wit, s);
      if (m) atomicMax(&tot[kRedCounters], m);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (tot[kRedEdges]) atomicAdd(rec + kRecEdges, (unsigned long long)tot[kRedEdges]);
    if (tot[kRedCandidates]) atomicAdd(rec + kRecCandidates, (unsigned long long)tot[kRedCandidates]);
    if (tot[kRedReduced]) atomicAdd(rec + kRecReduced, (unsigned long long)tot[kRedReduced]);
    if (tot[kRedLabel1]) atomicAdd(rec + kRecLabel1, (unsigned long long)tot[kRedLabel1]);
    if (tot[kRedSelfLoops]) atomicAdd(rec + kRecSelfLoops, (unsigned long long)tot[kRedSelfLoops]);
    if (wit) atomicAdd(rec + kRecWitnesses, wit);
    if (tot[kRedCounters]) atomicMax(rec + kRecMaxSupport, (unsigned long long)tot[kRedCounters]);
  }
}

}  // namespace gnm

using namespace gnm;

extern "C" int gnm_transitive_support(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* in_ptr,
                                      const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                                      const float* scores, const int64_t* prefix_length, const float* y, float min_logit, int64_t fuzz,
                                      int32_t* support, float* masked_scores, void* record, void* stream) {
  if (index_size_check("transitive_support", n, E, "the index holds 32-bit positions")) return -1;
  GNM_CHECK_ARG(fuzz >= -1, "transitive_support: fuzz = %lld: expected -1 (no length test) or a length >= 0", (long long)fuzz);
  if (record_check("transitive_support", record, "gnm_reduce_record")) return -1;
  GNM_CHECK_ARG(n == 0 || out_ptr, "transitive_support: out_ptr must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || (perm && out_pos && out_dst && scores && prefix_length && support),
                "transitive_support: perm, out_pos, out_dst, scores, prefix_length and support must not be null when E > 0");
  if (n == 0 || E == 0) return 0;                       // no edge: nothing to write, nothing launched, the record stays as it is
  RedArgs a;
  a.ix = IndexRows{n, E, perm, isrc, in_ptr, out_ptr, out_pos, out_dst, nperm};
  a.scores = scores; a.y = y; a.pl = prefix_length;
  a.min_logit = min_logit; a.fuzz = fuzz;
  a.support = support; a.masked = masked_scores;
  const int grid = persistent_grid(n, kGroupNodes, 8);
  hipLaunchKernelGGL(transitive_support_k, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, (unsigned long long*)record);
  GNM_LAUNCH_CHECK("transitive_support");
  return 0;
}
