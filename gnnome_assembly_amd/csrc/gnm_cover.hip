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
//   cov_propose_k   eight lanes per node (gnm_group.h).  A node u with msucc[u] < 0 writes cs[u] = (k, w): its best
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
#include "gnm_group.h"
#include "gnm_key.h"

namespace gnm {

struct CovArgs {
  IndexRows ix;
  const float* scores;
  float min_logit;
  int32_t *msucc, *mpred;                               // the state
  int2 *cs, *cp;                                        // the round's proposals: (edge id, other end) or (-1, -1)
  int32_t *link_succ, *link_pred;
};

__global__ __launch_bounds__(kBlock) void cov_begin_k(CovArgs a, unsigned long long* round_links, int rounds, int init) {
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
  for (int64_t r = t0; r < rounds; r += step) round_links[r] = 0ull;
  if (!init) return;
  for (int64_t i = t0; i < a.ix.n; i += step) {
    a.msucc[i] = -1;
    a.mpred[i] = -1;
  }
}

// One direction of one node (D = 0: its out-edges, 1: its in-edges).  Every lane of the group calls this together; `need` is
// group-uniform: the node exists and its slot in this direction is free.
template <int D>
__device__ __forceinline__ void cov_propose_(const CovArgs& a, int i, bool need, int sub) {
  const unsigned n = (unsigned)a.ix.n;
  unsigned long long mine = 0ull;
  int mother = -1;
  if (need) {
    const int32_t* taken = D ? a.msucc : a.mpred;                      // the slot of the other end that the edge would fill
    int lo, hi;
    row_clamped(D ? a.ix.in_ptr : a.ix.out_ptr, i, (int)a.ix.E, lo, hi);
    walk_candidates<D>(
        a.ix, lo + sub, hi,
        // no self loop, no end outside the index, none that is spoken for (most edges of a late round)
        [&](int other) { return other != i && (unsigned)other < n && taken[other] < 0; },
        [&](int, int, int other, int eid) {
          const float s = a.scores[eid];
          const unsigned key = dec_key_(s);
          if (key == 0u || !(s >= a.min_logit)) return;                // a NaN; below the cut
          const unsigned long long w = ((unsigned long long)key << 32) | (0x7fffffffu - (unsigned)eid);
          if (w > mine) {
            mine = w;
            mother = other;
          }
        });
  }
  const unsigned long long best = group_max_u64(mine);
  if (!need) return;
  int2* out = D ? a.cp : a.cs;
  if (best == 0ull) {
    if (sub == 0) out[i] = make_int2(-1, -1);
  } else if (mine == best) {                                           // edge ids are distinct: exactly one lane holds the winner
    out[i] = make_int2((int)(0x7fffffffu - (unsigned)best), mother);
  }
}

__global__ __launch_bounds__(kBlock) void cov_propose_k(CovArgs a) {
  for_group_nodes(a.ix.n, [&](int i, bool valid, int sub) {
    const bool need_s = valid && a.msucc[i] < 0, need_p = valid && a.mpred[i] < 0;
    if (!__any(need_s || need_p)) return;               // wave-uniform: its eight nodes are all matched on both sides
    cov_propose_<0>(a, i, need_s, sub);
    cov_propose_<1>(a, i, need_p, sub);
  });
}

__global__ __launch_bounds__(kBlock) void cov_link_k(CovArgs a, unsigned long long* word) {
  __shared__ unsigned lds[kWavesPerBlock];
  const unsigned n = (unsigned)a.ix.n;
  unsigned added = 0u;
  for (int64_t u64 = (int64_t)blockIdx.x * kBlock + threadIdx.x; u64 < a.ix.n; u64 += (int64_t)gridDim.x * kBlock) {
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
  block_count_add(added, lds, word);
}

__global__ __launch_bounds__(kBlock) void cov_export_k(CovArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ix.n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t v = a.ix.nperm ? (int64_t)a.ix.nperm[i] : i;
    if (v < 0 || v >= a.ix.n) continue;                    // the caller's id of node i, checked before it addresses anything
    a.link_succ[v] = a.msucc[i];
    a.link_pred[v] = a.mpred[i];
  }
}

}  // namespace gnm

using namespace gnm;

// ws: msucc, mpred (4 n each), cs, cp (8 n each)
struct CovLayout {
  size_t state[2], prop[2], bytes;
};
static CovLayout cov_layout(int64_t n) {
  CovLayout l;
  size_t off = 0;
  for (int d = 0; d < 2; ++d) { l.state[d] = off; off += ws_pad((size_t)n * 4); }
  for (int d = 0; d < 2; ++d) { l.prop[d] = off; off += ws_pad((size_t)n * 8); }
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
  if (index_size_check("cover_rounds", n, E, "the index holds 32-bit positions")) return -1;
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
  if (ws_check("cover_rounds", "gnm_cover_workspace_bytes", ws, ws_bytes, l.bytes)) return -1;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  CovArgs a;
  a.ix = IndexRows{n, E, perm, isrc, in_ptr, out_ptr, out_pos, out_dst, nperm};
  a.scores = scores; a.min_logit = min_logit;
  a.msucc = (int32_t*)(w + l.state[0]); a.mpred = (int32_t*)(w + l.state[1]);
  a.cs = (int2*)(w + l.prop[0]); a.cp = (int2*)(w + l.prop[1]);
  a.link_succ = link_succ; a.link_pred = link_pred;
  unsigned long long* rl = (unsigned long long*)round_links;
  const int init = first_round == 0 ? 1 : 0;
  if (rounds == 0 && n == 0) return 0;
  const dim3 blk(kBlock), grid(persistent_grid(n, kBlock, 8)), pgrid(persistent_grid(n, kGroupNodes, 8));
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
