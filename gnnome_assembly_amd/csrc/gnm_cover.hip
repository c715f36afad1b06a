// Greedy path cover by rounds of mutual-best links (include/gnm.h, "cover rounds"): the locally-dominant matching algorithm on
// the index the graph already carries.  Round one is the best-overlap graph of gnm_decision_stats + gnm_bog_contigs; every later
// round lets the nodes that still have a free slot choose again among the edges whose other end is free as well.  The fixed
// point is the greedy path cover of overlap-layout assemblers (edges by descending score, an edge accepted when its source has no
// successor and its destination no predecessor yet) -- before any cycle is cut, which stays gnm_bog_contigs' business.
//
// State per INTERNAL node i (the index's numbering): msucc[i], mpred[i] -- the edge id of the accepted out- / in-edge, or -1.
// A candidate is an edge k = (u -> w) with u != w, every position and id in range, a score that is no NaN and >= min_logit.
// Candidates are ordered by the 64-bit word  dec_key_(score) << 32 | (0x7FFFFFFF - k)  (gnm_key.h; the decision kernel's word
// without its label bit): a plain unsigned maximum is "largest score, then lowest edge id".  A candidate's key is >= 0x007FFFFF,
// so the word 0 stands for "no candidate".
//
// Round r, on the state after round r - 1, is two launches:
//   cov_propose_k   eight lanes per node, as in decision_stats_k.  A node u with msucc[u] < 0 writes cs[u] = (k, w): its best
//                   candidate out-edge among those whose destination has mpred[w] < 0, or (-1, -1).  A node w with mpred[w] < 0
//                   writes cp[w] = (k, u) likewise over its in-edges whose source has msucc[u] < 0.  Reads the state, writes the
//                   proposals.  A node whose two slots are taken loads its two state words and nothing else; a wave of eight such
//                   nodes skips the pass.
//   cov_link_k      one thread per node.  u with msucc[u] < 0, cs[u] = (k, w), k >= 0 and cp[w].k == k sets msucc[u] = k; w with
//                   mpred[w] < 0, cp[w] = (k, u), k >= 0 and cs[u].k == k sets mpred[w] = k.  Reads the proposals, writes its own
//                   two state words: nothing is scattered, and both ends decide by the same test.  The proposal of a node whose
//                   slot was already taken is stale and is never read: the link kernel looks at cs[u] only while msucc[u] < 0, and
//                   follows a proposal only to a node whose slot was free when the proposals were written, which therefore wrote
//                   its own in the same round.  The links a round adds are counted per thread, summed over the workgroup and
//                   added to round_links[r] by ONE 64-bit integer atomic per workgroup.
// cov_begin_k zeroes the call's round_links and, for first_round == 0, sets the state to -1; cov_export_k copies the state to
// link_succ / link_pred through nperm (the caller's numbering) at the end of every call.
// No launch reads what another thread of the same launch writes, no workgroup waits for another, there is no cooperative launch
// and no float arithmetic (a score enters through dec_key_ and the one comparison with min_logit).  Every output is a function of
// the inputs alone: of the grid, gnm_set_occupancy_cap and timing it is independent.  A round on a fixed-point state proposes
// nothing that is answered, so it adds nothing and changes nothing.
//
// Bounds.  Row pointers are clamped to 0 <= lo <= hi <= E; a position or edge id outside [0, E) and an other end outside [0, n)
// drop the candidate before they address anything; a proposal's other end is checked again before the link kernel follows it; a
// row nperm[i] outside [0, n) is never written.
#include "gnm_common.h"
#include "gnm_key.h"

namespace gnm {

constexpr int kCovLanes = 8;                            // lanes per node: the decision kernel's layout
constexpr int kCovNodes = kBlock / kCovLanes;           // nodes per workgroup and pass

struct CovArgs {
  int64_t n, E;
  const int32_t *perm, *isrc, *in_ptr, *out_ptr, *out_pos, *out_dst, *nperm;
  const float* scores;
  float min_logit;
  int32_t *msucc, *mpred;                               // the state
  int2 *cs, *cp;                                        // the round's proposals: (edge id, other end) or (-1, -1)
  int32_t *link_succ, *link_pred;
};

__device__ __forceinline__ unsigned long long cov_shfl_xor_(unsigned long long v, int off) {
  const unsigned lo = __shfl_xor((unsigned)v, off, kCovLanes), hi = __shfl_xor((unsigned)(v >> 32), off, kCovLanes);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(kBlock) void cov_begin_k(CovArgs a, unsigned long long* round_links, int rounds, int init) {
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
  for (int64_t r = t0; r < rounds; r += step) round_links[r] = 0ull;
  if (!init) return;
  for (int64_t i = t0; i < a.n; i += step) {
    a.msucc[i] = -1;
    a.mpred[i] = -1;
  }
}

// One direction of one node (D = 0: its out-edges, 1: its in-edges).  Every lane of the group calls this together; `need` is
// group-uniform: the node exists and its slot in this direction is free.
template <int D>
__device__ __forceinline__ void cov_propose_(const CovArgs& a, int i, bool need, int sub) {
  const int E = (int)a.E;
  const unsigned n = (unsigned)a.n;
  unsigned long long mine = 0ull;
  int mother = -1;
  if (need) {
    const int32_t* ptr = D ? a.in_ptr : a.out_ptr;
    const int32_t* taken = D ? a.msucc : a.mpred;                      // the slot of the other end that the edge would fill
    int lo = ptr[i], hi = ptr[i + 1];
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < lo ? lo : (hi > E ? E : hi);
    for (int p = lo + sub; p < hi; p += kCovLanes) {
      const int j = D ? p : a.out_pos[p];
      const int other = D ? a.isrc[p] : a.out_dst[p];
      if (other == i || (unsigned)other >= n || (unsigned)j >= (unsigned)E) continue;   // a self loop; outside the index
      if (taken[other] >= 0) continue;                                 // the other end is spoken for: most edges of a late round
      const int eid = a.perm[j];
      if ((unsigned)eid >= (unsigned)E) continue;
      const float s = a.scores[eid];
      const unsigned key = dec_key_(s);
      if (key == 0u || !(s >= a.min_logit)) continue;                  // a NaN; below the cut
      const unsigned long long w = ((unsigned long long)key << 32) | (0x7fffffffu - (unsigned)eid);
      if (w > mine) {
        mine = w;
        mother = other;
      }
    }
  }
  unsigned long long best = mine;
#pragma unroll
  for (int off = kCovLanes / 2; off > 0; off >>= 1) {
    const unsigned long long o = cov_shfl_xor_(best, off);
    best = o > best ? o : best;
  }
  if (!need) return;
  int2* out = D ? a.cp : a.cs;
  if (best == 0ull) {
    if (sub == 0) out[i] = make_int2(-1, -1);
  } else if (mine == best) {                                           // edge ids are distinct: exactly one lane holds the winner
    out[i] = make_int2((int)(0x7fffffffu - (unsigned)best), mother);
  }
}

__global__ __launch_bounds__(kBlock) void cov_propose_k(CovArgs a) {
  const int sub = threadIdx.x & (kCovLanes - 1), grp = threadIdx.x / kCovLanes;
  // base is workgroup-uniform: every lane of a wave takes the same number of passes, so the shuffles never meet an idle group
  for (int64_t base = (int64_t)blockIdx.x * kCovNodes; base < a.n; base += (int64_t)gridDim.x * kCovNodes) {
    const int64_t i64 = base + grp;
    const bool valid = i64 < a.n;
    const int i = valid ? (int)i64 : 0;
    const bool need_s = valid && a.msucc[i] < 0, need_p = valid && a.mpred[i] < 0;
    if (!__any(need_s || need_p)) continue;             // wave-uniform: its eight nodes are all matched on both sides
    cov_propose_<0>(a, i, need_s, sub);
    cov_propose_<1>(a, i, need_p, sub);
  }
}

__global__ __launch_bounds__(kBlock) void cov_link_k(CovArgs a, unsigned long long* word) {
  __shared__ unsigned lds[kWavesPerBlock];
  const unsigned n = (unsigned)a.n;
  unsigned added = 0u;
  for (int64_t u64 = (int64_t)blockIdx.x * kBlock + threadIdx.x; u64 < a.n; u64 += (int64_t)gridDim.x * kBlock) {
    const unsigned u = (unsigned)u64;
    if (a.msucc[u] < 0) {
      const int2 c = a.cs[u];
      if (c.x >= 0 && (unsigned)c.y < n && a.cp[c.y].x == c.x) {
        a.msucc[u] = c.x;
        added += 1u;                                    // every link is counted once, at its source
      }
    }
    if (a.mpred[u] < 0) {
      const int2 c = a.cp[u];
      if (c.x >= 0 && (unsigned)c.y < n && a.cs[c.y].x == c.x) a.mpred[u] = c.x;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) added += __shfl_xor(added, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = added;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = lds[0] + lds[1] + lds[2] + lds[3];
    if (t) atomicAdd(word, (unsigned long long)t);
  }
}

__global__ __launch_bounds__(kBlock) void cov_export_k(CovArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t v = a.nperm ? (int64_t)a.nperm[i] : i;
    if (v < 0 || v >= a.n) continue;                    // the caller's id of node i, checked before it addresses anything
    a.link_succ[v] = a.msucc[i];
    a.link_pred[v] = a.mpred[i];
  }
}

}  // namespace gnm

using namespace gnm;

static inline size_t cov_pad(size_t bytes) { return (bytes + 15) / 16 * 16; }

// ws: msucc, mpred (4 n each), cs, cp (8 n each)
struct CovLayout {
  size_t state[2], prop[2], bytes;
};
static CovLayout cov_layout(int64_t n) {
  CovLayout l;
  size_t off = 0;
  for (int d = 0; d < 2; ++d) { l.state[d] = off; off += cov_pad((size_t)n * 4); }
  for (int d = 0; d < 2; ++d) { l.prop[d] = off; off += cov_pad((size_t)n * 8); }
  l.bytes = off;
  return l;
}

extern "C" size_t gnm_cover_workspace_bytes(int64_t n) {
  if (n < 0 || n >= INT32_MAX) return 0;
  return cov_layout(n).bytes;
}

extern "C" int gnm_cover_rounds(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* in_ptr,
                                const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                                const float* scores, float min_logit, int64_t first_round, int64_t rounds, int64_t* round_links,
                                int32_t* link_succ, int32_t* link_pred, void* ws, size_t ws_bytes, void* stream) {
  GNM_CHECK_ARG(n >= 0 && E >= 0 && n < INT32_MAX && E < INT32_MAX,
                "cover_rounds: n = %lld, E = %lld: expected 0 <= n, E < 2^31 - 1 (the index holds 32-bit positions)", (long long)n,
                (long long)E);
  GNM_CHECK_ARG(first_round >= 0 && rounds >= 0 && first_round < INT32_MAX && rounds < INT32_MAX,
                "cover_rounds: first_round = %lld, rounds = %lld: expected 0 <= first_round, rounds < 2^31 - 1", (long long)first_round,
                (long long)rounds);
  GNM_CHECK_ARG(rounds == 0 || (round_links && ((uintptr_t)round_links & 7) == 0),
                "cover_rounds: round_links must be a non-null, 8-byte aligned int64 [rounds] array when rounds > 0");
  GNM_CHECK_ARG(n == 0 || (in_ptr && out_ptr), "cover_rounds: in_ptr and out_ptr must not be null when n > 0");
  GNM_CHECK_ARG(n == 0 || (link_succ && link_pred), "cover_rounds: link_succ and link_pred must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || (perm && isrc && out_pos && out_dst && scores),
                "cover_rounds: perm, isrc, out_pos, out_dst and scores must not be null when E > 0");
  const CovLayout l = cov_layout(n);
  GNM_CHECK_ARG(l.bytes == 0 || (ws && ws_bytes >= l.bytes && ((uintptr_t)ws & 15) == 0),
                "cover_rounds: workspace of %zu bytes too small (gnm_cover_workspace_bytes: %zu), null or not 16-byte aligned", ws_bytes,
                l.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  CovArgs a;
  a.n = n; a.E = E;
  a.perm = perm; a.isrc = isrc; a.in_ptr = in_ptr; a.out_ptr = out_ptr; a.out_pos = out_pos; a.out_dst = out_dst; a.nperm = nperm;
  a.scores = scores; a.min_logit = min_logit;
  a.msucc = (int32_t*)(w + l.state[0]); a.mpred = (int32_t*)(w + l.state[1]);
  a.cs = (int2*)(w + l.prop[0]); a.cp = (int2*)(w + l.prop[1]);
  a.link_succ = link_succ; a.link_pred = link_pred;
  unsigned long long* rl = (unsigned long long*)round_links;
  const int init = first_round == 0 ? 1 : 0;
  if (rounds == 0 && n == 0) return 0;
  const dim3 blk(kBlock), grid(persistent_grid(n, kBlock, 8)), pgrid(persistent_grid(n, kCovNodes, 8));
  const int64_t begin_items = init && n > rounds ? n : rounds;
  hipLaunchKernelGGL(cov_begin_k, dim3(persistent_grid(begin_items, kBlock, 8)), blk, 0, st, a, rl, (int)rounds, init);
  if (n > 0) {
    for (int64_t r = 0; r < rounds; ++r) {
      hipLaunchKernelGGL(cov_propose_k, pgrid, blk, 0, st, a);
      hipLaunchKernelGGL(cov_link_k, grid, blk, 0, st, a, rl + r);
    }
    hipLaunchKernelGGL(cov_export_k, grid, blk, 0, st, a);
  }
  GNM_LAUNCH_CHECK("cover_rounds");
  return 0;
}
