// The index of an induced sub-graph DERIVED from its parent's index (gnm_graph_induce_count / _fill): the ClusterGCN
// mini-batches (train.py:288-343 counterpart, cluster.py) without a sort.  The parent's index is sorted by destination over its
// internal node numbering and by source; a sub-graph keeps the parent's node order and its edges in ascending edge id, so the
// maps old node -> new node and old edge -> new edge are monotone and the sub-graph's destination-sorted (by-source) list IS the
// parent's with the dropped entries removed.  Everything is flag -> exclusive prefix sum -> gather / scatter over five sequences:
//   0  keepN[v]  = mask[v]                          caller node order      -> newC
//   1  kI[i]     = mask[nperm[i]]                   internal node order    -> newI   (only when the parent has nperm; else = 0)
//   2  keepE[k]  = mask[src[k]] & mask[dst[k]]      edge-id order          -> newE
//   3  kP[p]     = keepE[perm[p]]                   destination order      -> q
//   4  kS[j]     = keepE[perm[out_pos[j]]]          by-source order        -> r
// The prefix sum has three phases over FIXED blocks of kIndBlk elements (independent of the grid and the CU count):
//   ind_flags_k   flags (bytes) + one int32 sum per block      (launch A: sequences 0-2; launch B: 3-4, which read keepE)
//   ind_scan_k    one workgroup per sequence turns its block sums into their exclusive prefix; totals n', e' as int64
//   ind_apply_k   in-block scan (gnm_group.h's block_scan_excl) + the block's offset
// No kernel waits for another workgroup: no look-back, no flag, no atomic.  ind_fill_k then writes every array of the sub-graph.
// Every index that is read from memory is range-checked before it addresses anything: a malformed index or sizes that do not
// belong to the count before them can give wrong numbers, never an access outside the caller's arrays.
#include "gnm_common.h"
#include "gnm_group.h"

namespace gnm {

constexpr int kIndBlk = 4 * kBlock;      // elements per scan block: thread t owns the four consecutive elements 4t .. 4t+3
constexpr int kIndSeqs = 5;

struct IndArgs {
  int64_t N, E;
  int64_t nbN, nbE;                      // scan blocks of a node / an edge sequence
  int has_rank;                          // the parent has an internal numbering (sequence 1 exists)
  int vec;                               // every int32 input is 16-byte aligned
  const uint8_t* mask;
  const int32_t *src, *dst, *perm, *out_pos, *nperm;
  uint8_t* flag[kIndSeqs];
  int32_t* bsum[kIndSeqs];               // block sums, then (ind_scan_k) their exclusive prefix
  int32_t* pre[kIndSeqs];                // the exclusive prefix of every element
  int64_t* sizes;                        // n', e'
};

__device__ __forceinline__ int64_t ind_len(const IndArgs& a, int s) { return s < 2 ? a.N : a.E; }
__device__ __forceinline__ int64_t ind_nblk(const IndArgs& a, int s) {
  return s < 2 ? ((s == 1 && !a.has_rank) ? 0 : a.nbN) : a.nbE;
}
// combined block c of a launch over the sequences in `seqs` (bit s) -> sequence and block; workgroup-uniform
__device__ __forceinline__ bool ind_locate(const IndArgs& a, unsigned seqs, int64_t c, int& s, int64_t& b) {
  for (s = 0; s < kIndSeqs; ++s) {
    if (!((seqs >> s) & 1u)) continue;
    const int64_t n = ind_nblk(a, s);
    if (c < n) { b = c; return true; }
    c -= n;
  }
  return false;
}

__device__ __forceinline__ void ind_ld4(const int32_t* __restrict__ p, int64_t k0, int64_t len, bool vec, int v[4]) {
  if (vec && k0 + 3 < len) {
    const int4 x = *reinterpret_cast<const int4*>(p + k0);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = k0 + i < len ? p[k0 + i] : -1;
  }
}
// four flag bytes of one thread (the flag arrays are 16-byte aligned and k0 is a multiple of 4); 0 past the end
__device__ __forceinline__ uint32_t ind_ldflags(const uint8_t* __restrict__ f, int64_t k0, int64_t len) {
  if (k0 + 3 < len) return *reinterpret_cast<const uint32_t*>(f + k0);
  uint32_t w = 0;
  for (int i = 0; i < 4; ++i)
    if (k0 + i < len) w |= (uint32_t)(f[k0 + i] != 0) << (8 * i);
  return w;
}

// Phase 1: the flags of the sequences in `seqs` and the sum of every block of kIndBlk of them.
__global__ __launch_bounds__(kBlock) void ind_flags_k(IndArgs a, unsigned seqs, int64_t nblocks) {
  __shared__ int red[kWavesPerBlock];
  const bool vec = a.vec != 0;
  const uint32_t N = (uint32_t)a.N, E = (uint32_t)a.E;
  for (int64_t c = blockIdx.x; c < nblocks; c += gridDim.x) {
    int s;
    int64_t b;
    if (!ind_locate(a, seqs, c, s, b)) break;
    const int64_t len = ind_len(a, s), k0 = b * kIndBlk + 4 * (int64_t)threadIdx.x;
    int f[4] = {0, 0, 0, 0};
    if (s == 0) {
      const uint32_t w = ind_ldflags(a.mask, k0, len);      // (bytes other than 0 / 1 count as set, element by element)
      if (k0 + 3 < len) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = ((w >> (8 * i)) & 0xffu) != 0;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (w >> (8 * i)) & 1u;
      }
    } else if (s == 2) {
      int u[4], v[4];
      ind_ld4(a.src, k0, len, vec, u);
      ind_ld4(a.dst, k0, len, vec, v);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        f[i] = ((uint32_t)u[i] < N && (uint32_t)v[i] < N) ? ((a.mask[u[i]] != 0) & (a.mask[v[i]] != 0)) : 0;
    } else {
      int x[4];
      ind_ld4(s == 1 ? a.nperm : (s == 3 ? a.perm : a.out_pos), k0, len, vec, x);      // -1 past the end
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (s == 1) {
          f[i] = (uint32_t)x[i] < N ? a.mask[x[i]] != 0 : 0;
        } else {
          uint32_t e = (uint32_t)x[i];
          if (s == 4) e = e < E ? (uint32_t)a.perm[e] : 0xffffffffu;
          f[i] = e < E ? a.flag[2][e] != 0 : 0;
        }
      }
    }
    uint8_t* fl = a.flag[s];
    if (k0 + 3 < len) {
      *reinterpret_cast<uint32_t*>(fl + k0) = (uint32_t)f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k0 + i < len) fl[k0 + i] = (uint8_t)f[i];
    }
    const int cnt = block_sum(f[0] + f[1] + f[2] + f[3], red);
    if (threadIdx.x == 0) a.bsum[s][b] = cnt;
  }
}

// Phase 2: workgroup s turns the block sums of sequence s into their exclusive prefix, in place (scan_block_sums).  The totals
// leave as int64 (the sums themselves stay below 2^31: E does).
__global__ __launch_bounds__(kBlock) void ind_scan_k(IndArgs a) {
  __shared__ int lds[kWavesPerBlock];
  const int s = blockIdx.x;
  if (s == 1 && !a.has_rank) return;
  int total;
  scan_block_sums(a.bsum[s], ind_nblk(a, s), lds, total);
  if (threadIdx.x == 0) {
    if (s == 0) a.sizes[0] = (int64_t)total;
    if (s == 2) a.sizes[1] = (int64_t)total;
  }
}

// Phase 3: pre[k] = the number of set flags before element k.
__global__ __launch_bounds__(kBlock) void ind_apply_k(IndArgs a, unsigned seqs, int64_t nblocks) {
  __shared__ int lds[kWavesPerBlock];
  for (int64_t c = blockIdx.x; c < nblocks; c += gridDim.x) {
    int s;
    int64_t b;
    if (!ind_locate(a, seqs, c, s, b)) break;
    const int64_t len = ind_len(a, s), k0 = b * kIndBlk + 4 * (int64_t)threadIdx.x;
    const uint32_t w = ind_ldflags(a.flag[s], k0, len);
    const int f[4] = {(int)(w & 1u), (int)((w >> 8) & 1u), (int)((w >> 16) & 1u), (int)((w >> 24) & 1u)};
    int total;
    const int x0 = a.bsum[s][b] + block_scan_excl(f[0] + f[1] + f[2] + f[3], lds, total);
    store4_excl(a.pre[s], k0, len, x0, f);
  }
}

struct IndFill {
  int64_t N, E, n_sub, e_sub;
  int has_rank;
  const int32_t *src, *dst, *perm, *isrc, *idst, *in_ptr, *out_ptr, *out_pos, *out_dst, *nrank;
  const uint8_t* flag[kIndSeqs];
  const int32_t* pre[kIndSeqs];
  int32_t *nid, *eid, *s_sub, *d_sub, *perm_o, *isrc_o, *idst_o, *in_ptr_o, *out_ptr_o, *out_pos_o, *out_dst_o, *nrank_o, *nperm_o;
};

// Thread g looks at the elements 4g .. 4g+3 of every sequence: the flag words first (a mini-batch keeps a few contiguous runs of
// the parent's order, so most words are all clear and nothing else is loaded), then the kept entries' gathers and their scatter
// to the compacted position.  Both maps are monotone, so neighbouring kept entries write neighbouring words.
__global__ __launch_bounds__(kBlock) void ind_fill_k(IndFill a, int64_t groups) {
  const uint32_t N = (uint32_t)a.N, E = (uint32_t)a.E, n_sub = (uint32_t)a.n_sub, e_sub = (uint32_t)a.e_sub;
  const int32_t *newC = a.pre[0], *newI = a.pre[1], *newE = a.pre[2], *q = a.pre[3], *r = a.pre[4];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.in_ptr_o[n_sub] = (int32_t)e_sub;
    a.out_ptr_o[n_sub] = (int32_t)e_sub;
  }
  for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
    const int64_t k0 = 4 * g;
    if (k0 < a.N) {
      const uint32_t wC = ind_ldflags(a.flag[0], k0, a.N);
      const uint32_t wI = a.has_rank ? ind_ldflags(a.flag[1], k0, a.N) : wC;
      for (int i = 0; i < 4; ++i) {
        const int64_t v = k0 + i;
        if ((wC >> (8 * i)) & 1u) {                             // caller order: the node's own id and its place in the order
          const uint32_t c = (uint32_t)newC[v];
          if (c < n_sub) {
            a.nid[c] = (int32_t)v;
            if (a.has_rank) {
              const uint32_t in = (uint32_t)a.nrank[v];
              const uint32_t ni = in < N ? (uint32_t)newI[in] : 0xffffffffu;
              if (ni < n_sub) {
                a.nrank_o[c] = (int32_t)ni;
                a.nperm_o[ni] = (int32_t)c;
              }
            }
          }
        }
        if ((wI >> (8 * i)) & 1u) {                             // internal order: where the node's rows start
          const uint32_t ni = (uint32_t)newI[v];
          if (ni < n_sub) {
            const uint32_t pi = (uint32_t)a.in_ptr[v], po = (uint32_t)a.out_ptr[v];
            a.in_ptr_o[ni] = pi < E ? q[pi] : (int32_t)e_sub;
            a.out_ptr_o[ni] = po < E ? r[po] : (int32_t)e_sub;
          }
        }
      }
    }
    if (k0 < a.E) {
      const uint32_t wE = ind_ldflags(a.flag[2], k0, a.E), wP = ind_ldflags(a.flag[3], k0, a.E),
                     wS = ind_ldflags(a.flag[4], k0, a.E);
      for (int i = 0; i < 4; ++i) {
        const int64_t k = k0 + i;
        if ((wE >> (8 * i)) & 1u) {                             // edge-id order
          const uint32_t o = (uint32_t)newE[k];
          const uint32_t s = (uint32_t)a.src[k], d = (uint32_t)a.dst[k];
          if (o < e_sub && s < N && d < N) {
            a.eid[o] = (int32_t)k;
            a.s_sub[o] = newC[s];
            a.d_sub[o] = newC[d];
          }
        }
        if ((wP >> (8 * i)) & 1u) {                             // destination order
          const uint32_t o = (uint32_t)q[k];
          const uint32_t s = (uint32_t)a.isrc[k], d = (uint32_t)a.idst[k], ek = (uint32_t)a.perm[k];
          if (o < e_sub && s < N && d < N && ek < E) {
            a.perm_o[o] = newE[ek];
            a.isrc_o[o] = newI[s];
            a.idst_o[o] = newI[d];
          }
        }
        if ((wS >> (8 * i)) & 1u) {                             // by-source order
          const uint32_t o = (uint32_t)r[k];
          const uint32_t d = (uint32_t)a.out_dst[k], p = (uint32_t)a.out_pos[k];
          if (o < e_sub && d < N && p < E) {
            a.out_pos_o[o] = q[p];
            a.out_dst_o[o] = newI[d];
          }
        }
      }
    }
  }
}

}  // namespace gnm

using namespace gnm;

static inline int64_t ind_blocks(int64_t n) { return (n + kIndBlk - 1) / kIndBlk; }

// ws: the five prefix arrays (int32), the five flag arrays (bytes), the five block-sum arrays (int32); each 16-byte aligned
struct IndLayout {
  size_t pre[kIndSeqs], flag[kIndSeqs], bsum[kIndSeqs], bytes;
};
static IndLayout ind_layout(int64_t N, int64_t E) {
  IndLayout l;
  size_t off = 0;
  for (int s = 0; s < kIndSeqs; ++s) { l.pre[s] = off; off += ws_pad((size_t)(s < 2 ? N : E) * sizeof(int32_t)); }
  for (int s = 0; s < kIndSeqs; ++s) { l.flag[s] = off; off += ws_pad((size_t)(s < 2 ? N : E)); }
  for (int s = 0; s < kIndSeqs; ++s) { l.bsum[s] = off; off += ws_pad((size_t)ind_blocks(s < 2 ? N : E) * sizeof(int32_t)); }
  l.bytes = off;
  return l;
}

extern "C" int gnm_graph_induce_scan_block(void) { return kIndBlk; }

extern "C" size_t gnm_graph_induce_workspace_bytes(int64_t N, int64_t E) {
  if (N < 0 || E < 0 || N >= INT32_MAX || E >= INT32_MAX) return 0;
  return ind_layout(N, E).bytes;
}

extern "C" int gnm_graph_induce_count(int64_t N, int64_t E, const int32_t* src, const int32_t* dst, const uint8_t* node_mask,
                                      const int32_t* perm, const int32_t* out_pos, const int32_t* nperm, void* ws,
                                      size_t ws_bytes, int64_t* sizes, void* stream) {
  GNM_CHECK_ARG(N >= 0 && E >= 0, "graph_induce_count: negative size");
  GNM_CHECK_ARG(N < INT32_MAX && E < INT32_MAX, "graph_induce_count: N = %lld, E = %lld: 32-bit positions, both must be below 2^31 - 1",
                (long long)N, (long long)E);
  GNM_CHECK_ARG(sizes, "graph_induce_count: null sizes");
  GNM_CHECK_ARG(N == 0 || (node_mask && ((uintptr_t)node_mask & 3) == 0), "graph_induce_count: node mask null or not 4-byte aligned");
  GNM_CHECK_ARG(E == 0 || (src && dst && perm && out_pos), "graph_induce_count: null edge or index array");
  const IndLayout l = ind_layout(N, E);
  GNM_CHECK_ARG(l.bytes == 0 || (ws && ws_bytes >= l.bytes && ((uintptr_t)ws & 15) == 0),
                "graph_induce_count: workspace too small or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  IndArgs a;
  a.N = N; a.E = E; a.nbN = ind_blocks(N); a.nbE = ind_blocks(E);
  a.has_rank = nperm != nullptr;
  a.vec = (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)perm | (uintptr_t)out_pos | (uintptr_t)nperm) & 15) == 0;
  a.mask = node_mask; a.src = src; a.dst = dst; a.perm = perm; a.out_pos = out_pos; a.nperm = nperm;
  for (int s = 0; s < kIndSeqs; ++s) {
    a.flag[s] = (uint8_t*)ws + l.flag[s];
    a.bsum[s] = (int32_t*)((char*)ws + l.bsum[s]);
    a.pre[s] = (int32_t*)((char*)ws + l.pre[s]);
  }
  a.sizes = sizes;
  const int64_t nA = a.nbN * (a.has_rank ? 2 : 1) + a.nbE, nB = 2 * a.nbE;
  const unsigned seqA = a.has_rank ? 0x7u : 0x5u, seqB = 0x18u;
  if (nA > 0) hipLaunchKernelGGL(ind_flags_k, dim3(persistent_grid(nA, 1, 8)), dim3(kBlock), 0, st, a, seqA, nA);
  if (nB > 0) hipLaunchKernelGGL(ind_flags_k, dim3(persistent_grid(nB, 1, 8)), dim3(kBlock), 0, st, a, seqB, nB);
  hipLaunchKernelGGL(ind_scan_k, dim3(kIndSeqs), dim3(kBlock), 0, st, a);
  if (nA + nB > 0)
    hipLaunchKernelGGL(ind_apply_k, dim3(persistent_grid(nA + nB, 1, 8)), dim3(kBlock), 0, st, a, seqA | seqB, nA + nB);
  GNM_LAUNCH_CHECK("graph_induce_count");
  return 0;
}

extern "C" int gnm_graph_induce_fill(int64_t N, int64_t E, int64_t n_sub, int64_t e_sub, const int32_t* src, const int32_t* dst,
                                     const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                                     const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst,
                                     const int32_t* nrank, const void* ws, size_t ws_bytes, int32_t* nid, int32_t* eid,
                                     int32_t* s_sub, int32_t* d_sub, int32_t* perm_sub, int32_t* isrc_sub, int32_t* idst_sub,
                                     int32_t* in_ptr_sub, int32_t* out_ptr_sub, int32_t* out_pos_sub, int32_t* out_dst_sub,
                                     int32_t* nrank_sub, int32_t* nperm_sub, void* stream) {
  GNM_CHECK_ARG(N >= 0 && E >= 0 && N < INT32_MAX && E < INT32_MAX, "graph_induce_fill: N and E must be in [0, 2^31 - 1)");
  GNM_CHECK_ARG(n_sub >= 0 && n_sub <= N && e_sub >= 0 && e_sub <= E, "graph_induce_fill: n_sub / e_sub outside [0, N] / [0, E]");
  GNM_CHECK_ARG(in_ptr_sub && out_ptr_sub, "graph_induce_fill: null in_ptr / out_ptr output");
  GNM_CHECK_ARG(N == 0 || (in_ptr && out_ptr), "graph_induce_fill: null in_ptr / out_ptr");
  GNM_CHECK_ARG(E == 0 || (src && dst && perm && isrc && idst && out_pos && out_dst), "graph_induce_fill: null edge or index array");
  GNM_CHECK_ARG(n_sub == 0 || (nid && (!nrank || (nrank_sub && nperm_sub))), "graph_induce_fill: null node output");
  GNM_CHECK_ARG(e_sub == 0 || (eid && s_sub && d_sub && perm_sub && isrc_sub && idst_sub && out_pos_sub && out_dst_sub),
                "graph_induce_fill: null edge output");
  const IndLayout l = ind_layout(N, E);
  GNM_CHECK_ARG(l.bytes == 0 || (ws && ws_bytes >= l.bytes && ((uintptr_t)ws & 15) == 0),
                "graph_induce_fill: workspace too small or not 16-byte aligned");
  IndFill a;
  a.N = N; a.E = E; a.n_sub = n_sub; a.e_sub = e_sub;
  a.has_rank = nrank != nullptr;
  a.src = src; a.dst = dst; a.perm = perm; a.isrc = isrc; a.idst = idst; a.in_ptr = in_ptr; a.out_ptr = out_ptr;
  a.out_pos = out_pos; a.out_dst = out_dst; a.nrank = nrank;
  for (int s = 0; s < kIndSeqs; ++s) {
    a.flag[s] = (const uint8_t*)ws + l.flag[s];
    a.pre[s] = (const int32_t*)((const char*)ws + l.pre[s]);
  }
  if (!a.has_rank) { a.flag[1] = a.flag[0]; a.pre[1] = a.pre[0]; }      // internal order = caller order
  a.nid = nid; a.eid = eid; a.s_sub = s_sub; a.d_sub = d_sub; a.perm_o = perm_sub; a.isrc_o = isrc_sub; a.idst_o = idst_sub;
  a.in_ptr_o = in_ptr_sub; a.out_ptr_o = out_ptr_sub; a.out_pos_o = out_pos_sub; a.out_dst_o = out_dst_sub;
  a.nrank_o = nrank_sub; a.nperm_o = nperm_sub;
  const int64_t groups = ((N > E ? N : E) + 3) / 4;
  hipLaunchKernelGGL(ind_fill_k, dim3(persistent_grid((groups + kBlock - 1) / kBlock, 1, 8)), dim3(kBlock), 0,
                     (hipStream_t)stream, a, groups);
  GNM_LAUNCH_CHECK("graph_induce_fill");
  return 0;
}
