// Best-overlap-graph contigs on the device (include/gnm.h, "best-overlap contigs"): keep an edge only when it is the top-scored
// out-edge of its source AND the top-scored in-edge of its destination (the tables gnm_decision_stats writes), cut every cycle
// at its smallest node, rank the nodes of the resulting disjoint paths by pointer jumping and lay the paths out as contigs.
// Everything is in the caller's node numbering and edge-id order.
//
// Launches of one call, all on one stream (K = ceil(log2(max(n, 2)))):
//   bog_link_k        next / prev / pedge of every node, each written by the node's own thread: node u tests its best successor
//                     edge, node v its best predecessor edge, under the same conditions, so the two sides agree and nothing is
//                     scattered.  Generation 0 of the cycle pass: (ptr = prev, min = own id).
//   bog_min_k   x K   round r: min[v] = min(min[v], min[ptr[v]]), ptr[v] = ptr[ptr[v]] -- after it min[v] covers v and its
//                     2^r - 1 predecessors.  A path of at most n nodes has reached its head (ptr = -1) after K rounds; a node
//                     whose ptr is still live is on a cycle and its min has gone at least once round it.
//   bog_rank_init_k   the cut, again by the owner alone: the cycle node v with min == v loses prev / pedge, the cycle node whose
//                     next is its min loses next.  Generation 0 of the ranking pass: a head holds ptr = ~v (its own id,
//                     complemented: "finished, head = v"), any other node (ptr = prev, rank = 1, wrong = [y[pedge] != 1],
//                     off = prefix_length[pedge]).
//   bog_rank_k  x K   round: a node whose ptr is live adds the record of ptr[v] to its own and takes over its ptr (a further
//                     pointer, or the finished ~head).  The last round also stores the path's length at its head.
//   scan_launch       exclusive prefix sums in NODE order of the head flags (-> contig number) and of the lengths stored at the
//                     heads (-> contig_ptr): the three launches of gnm_scan.h over blocks of 4 kBlock nodes, a thread owning four
//                     consecutive nodes (BogScan).
//   bog_layout_k      walk_nodes / walk_edges at contig_ptr[c] + rank, contig_bases / contig_wrong from the tails, the counters.
// Every round reads one generation and writes the other (ping-pong): no kernel reads what the same launch writes, no workgroup
// waits for another, there is no flag, no cooperative launch and no read-back between the launches.  A node's state is one
// 16-byte record (ptr, rank, wrong) and one 8-byte offset per generation; the cycle pass packs (ptr, min) into 8 bytes.
// No float arithmetic: a score enters through `scores[k] >= min_logit` (false for a NaN) alone, a label through `y == 1`.
// Integer atomics only on the record: one per counter and workgroup.  Every output is a function of the inputs alone.
//
// Bounds.  A table entry outside [0, E) and a src / dst entry outside [0, n) drop the candidate before they address anything;
// pointers kept in the workspace are built from checked values and are checked again where they address a caller's array.
#include "gnm_common.h"
#include "gnm_scan.h"

namespace gnm {

enum { kBogContigs = 0, kBogLinks, kBogCyclesCut, kBogDropped, kBogWrongLinks, kBogMultiNodes, kBogMultiContigs, kBogCalls };

struct BogArgs {
  int64_t n, E;
  const int32_t *src, *dst, *best_succ, *best_pred;
  const float *scores, *y;
  const int64_t *prefix_length, *read_length;
  float min_logit;
  int32_t *next, *prev, *pedge, *plen, *pre_f, *pre_l;
  int2* mn[2];                           // cycle pass: (ptr, min); lives in ra[1], which the ranking pass writes only later
  int4* ra[2];                           // ranking pass: (ptr or ~head, rank, wrong, 0)
  int64_t* ro[2];                        // ... and off
  int32_t *contig_ptr, *walk_nodes, *walk_edges, *contig_wrong;
  int64_t* contig_bases;
  unsigned long long* rec;
};

__global__ __launch_bounds__(kBlock) void bog_link_k(BogArgs a) {
  __shared__ unsigned lds[kWavesPerBlock];
  const unsigned n = (unsigned)a.n, E = (unsigned)a.E;
  unsigned dropped = 0u;
  for (int64_t v64 = (int64_t)blockIdx.x * kBlock + threadIdx.x; v64 < a.n; v64 += (int64_t)gridDim.x * kBlock) {
    const unsigned v = (unsigned)v64;
    int nx = -1, pv = -1, pe = -1;
    unsigned k = (unsigned)a.best_succ[v];
    if (k < E) {                                        // v -> d by edge k: mutual-best when it is also d's best predecessor
      const unsigned s = (unsigned)a.src[k], d = (unsigned)a.dst[k];
      if (s == v && d < n && d != v && (unsigned)a.best_pred[d] == k) {
        if (a.scores[k] >= a.min_logit) nx = (int)d;    // false for a NaN score
        else dropped += 1u;
      }
    }
    k = (unsigned)a.best_pred[v];
    if (k < E) {                                        // s -> v by edge k: the same conditions from the other end
      const unsigned s = (unsigned)a.src[k], d = (unsigned)a.dst[k];
      if (d == v && s < n && s != v && (unsigned)a.best_succ[s] == k && a.scores[k] >= a.min_logit) {
        pv = (int)s;
        pe = (int)k;
      }
    }
    a.next[v] = nx;
    a.prev[v] = pv;
    a.pedge[v] = pe;
    a.mn[0][v] = make_int2(pv, (int)v);
  }
  block_count_add(dropped, lds, a.rec + kBogDropped);
}

__global__ __launch_bounds__(kBlock) void bog_min_k(BogArgs a, int g) {
  const int2* __restrict__ in = a.mn[g];
  int2* __restrict__ out = a.mn[g ^ 1];
  const unsigned n = (unsigned)a.n;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kBlock) {
    int2 s = in[v];
    if ((unsigned)s.x < n) {
      const int2 q = in[s.x];
      s.y = q.y < s.y ? q.y : s.y;
      s.x = q.x;
    }
    out[v] = s;
  }
}

__global__ __launch_bounds__(kBlock) void bog_rank_init_k(BogArgs a, int gmin) {
  __shared__ unsigned lds[kWavesPerBlock];
  const int2* __restrict__ mn = a.mn[gmin];
  const unsigned n = (unsigned)a.n, E = (unsigned)a.E;
  unsigned cut = 0u;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kBlock) {
    const int2 m = mn[v];
    int pv = a.prev[v], pe = a.pedge[v];
    const bool cyc = (unsigned)m.x < n;                 // still live after K rounds: on a cycle, m.y = the cycle's smallest node
    if (cyc && m.y == (int)v) {
      pv = pe = -1;
      a.prev[v] = -1;
      a.pedge[v] = -1;
      cut += 1u;
    }
    if (cyc && m.y == a.next[v]) a.next[v] = -1;
    int4 r = make_int4(~(int)v, 0, 0, 0);
    int64_t off = 0;
    if ((unsigned)pv < n && (unsigned)pe < E) {
      r = make_int4(pv, 1, (a.y && !(a.y[pe] == 1.0f)) ? 1 : 0, 0);
      off = a.prefix_length[pe];
    }
    a.ra[0][v] = r;
    a.ro[0][v] = off;
    a.plen[v] = 0;
  }
  block_count_add(cut, lds, a.rec + kBogCyclesCut);
}

__global__ __launch_bounds__(kBlock) void bog_rank_k(BogArgs a, int g, int last) {
  const int4* __restrict__ ia = a.ra[g];
  const int64_t* __restrict__ io = a.ro[g];
  int4* __restrict__ oa = a.ra[g ^ 1];
  int64_t* __restrict__ oo = a.ro[g ^ 1];
  const unsigned n = (unsigned)a.n;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kBlock) {
    int4 r = ia[v];
    int64_t o = io[v];
    if ((unsigned)r.x < n) {
      const int4 q = ia[r.x];
      o += io[r.x];
      r.y += q.y;
      r.z += q.z;
      r.x = q.x;
    }
    oa[v] = r;
    oo[v] = o;
    if (last && a.next[v] < 0) {                        // the tail: its rank + 1 is the path's length, kept at the head
      const unsigned h = (unsigned)~r.x;
      if (h < n) a.plen[h] = r.y + 1;
    }
  }
}

// The two scanned sequences, in node order: head flags (-> contig number, pre_f) and the lengths kept at the heads (-> pre_l).
struct BogScan : ScanUser<int32_t, 2> {
  BogArgs a;
  __device__ __forceinline__ void load(const Arrays& x, int64_t k0, bool, int32_t (&v)[2][4]) const {
    int32_t f[4], l[4];                                  // (written straight into v, the rows end up in scratch memory)
    if (k0 + 3 < x.n) {
      const int4 p = *reinterpret_cast<const int4*>(a.prev + k0), q = *reinterpret_cast<const int4*>(a.plen + k0);
      f[0] = p.x < 0; f[1] = p.y < 0; f[2] = p.z < 0; f[3] = p.w < 0;
      l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f[i] = k0 + i < x.n ? a.prev[k0 + i] < 0 : 0;
        l[i] = k0 + i < x.n ? a.plen[k0 + i] : 0;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[0][i] = f[i];
      v[1][i] = l[i];
    }
  }
  // The flag sequence's total is the contig count C: contig_ptr[C] = n (every node lies on one path), record.contigs += C, calls += 1.
  __device__ __forceinline__ void total(const Arrays&, int s, int32_t total) const {
    if (s != 0) return;
    if (a.contig_ptr && total >= 0 && (int64_t)total <= a.n) a.contig_ptr[total] = (int32_t)a.n;
    if (total > 0) atomicAdd(a.rec + kBogContigs, (unsigned long long)total);
    atomicAdd(a.rec + kBogCalls, 1ull);
  }
};

__global__ __launch_bounds__(kBlock) void bog_layout_k(BogArgs a, int g) {
  __shared__ unsigned lds[kWavesPerBlock];
  const int4* __restrict__ ra = a.ra[g];
  const int64_t* __restrict__ ro = a.ro[g];
  const unsigned n = (unsigned)a.n;
  unsigned links = 0u, wrong = 0u, mnodes = 0u, mcontigs = 0u;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < a.n; v += (int64_t)gridDim.x * kBlock) {
    const int4 r = ra[v];
    const unsigned h = (unsigned)~r.x;
    if (h >= n || r.y < 0) continue;                    // (a finished record names its head; anything else is never used)
    const unsigned start = (unsigned)a.pre_l[h];
    const uint64_t pos = (uint64_t)start + (unsigned)r.y;
    if (pos < n) {
      a.walk_nodes[pos] = (int32_t)v;
      a.walk_edges[pos] = a.pedge[v];
    }
    if (h == (unsigned)v) {
      const unsigned c = (unsigned)a.pre_f[v];
      if (c < n) a.contig_ptr[c] = (int32_t)start;
    }
    if (a.next[v] < 0) {                                // the tail speaks for its contig
      const unsigned c = (unsigned)a.pre_f[h];
      if (c < n) {
        a.contig_bases[c] = ro[v] + a.read_length[v];
        a.contig_wrong[c] = r.z;
      }
      links += (unsigned)r.y;
      wrong += (unsigned)r.z;
      if (r.y >= 1) {
        mnodes += (unsigned)r.y + 1u;
        mcontigs += 1u;
      }
    }
  }
  block_count_add(links, lds, a.rec + kBogLinks);
  block_count_add(wrong, lds, a.rec + kBogWrongLinks);
  block_count_add(mnodes, lds, a.rec + kBogMultiNodes);
  block_count_add(mcontigs, lds, a.rec + kBogMultiContigs);
}

}  // namespace gnm

using namespace gnm;

// ws: ra[0], ra[1] (16 n each), ro[0], ro[1] (8 n), next, prev, pedge, plen, pre_f, pre_l (4 n), two block-sum arrays
struct BogLayout {
  size_t ra[2], ro[2], i32[6], bsum[2], bytes;
};
static BogLayout bog_layout(int64_t n) {
  BogLayout l;
  size_t off = 0;
  for (int g = 0; g < 2; ++g) { l.ra[g] = off; off += ws_pad((size_t)n * 16); }
  for (int g = 0; g < 2; ++g) { l.ro[g] = off; off += ws_pad((size_t)n * 8); }
  for (int i = 0; i < 6; ++i) { l.i32[i] = off; off += ws_pad((size_t)n * 4); }
  for (int s = 0; s < 2; ++s) { l.bsum[s] = off; off += scan_bsum_bytes<int32_t, 4>(n); }
  l.bytes = off;
  return l;
}

extern "C" size_t gnm_bog_workspace_bytes(int64_t n) {
  if (n < 0 || n >= INT32_MAX) return 0;
  return bog_layout(n).bytes;
}

extern "C" int gnm_bog_contigs(int64_t n, int64_t E, const int32_t* src, const int32_t* dst, const int32_t* best_succ,
                               const int32_t* best_pred, const float* scores, const float* y, const int64_t* prefix_length,
                               const int64_t* read_length, float min_logit, void* record, int32_t* contig_ptr, int32_t* walk_nodes,
                               int32_t* walk_edges, int64_t* contig_bases, int32_t* contig_wrong, void* ws, size_t ws_bytes,
                               void* stream) {
  if (index_size_check("bog_contigs", n, E, "32-bit node and edge ids") || record_check("bog_contigs", record, "gnm_bog_record"))
    return -1;
  GNM_CHECK_ARG(n == 0 || (best_succ && best_pred && read_length),
                "bog_contigs: best_succ, best_pred and read_length must not be null when n > 0");
  GNM_CHECK_ARG(n == 0 || (contig_ptr && walk_nodes && walk_edges && contig_bases && contig_wrong),
                "bog_contigs: contig_ptr, walk_nodes, walk_edges, contig_bases and contig_wrong must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || (src && dst && scores && prefix_length),
                "bog_contigs: src, dst, scores and prefix_length must not be null when E > 0");
  const BogLayout l = bog_layout(n);
  if (ws_check("bog_contigs", "gnm_bog_workspace_bytes", ws, ws_bytes, l.bytes)) return -1;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  BogArgs a;
  a.n = n; a.E = E;
  a.src = src; a.dst = dst; a.best_succ = best_succ; a.best_pred = best_pred; a.scores = scores; a.y = y;
  a.prefix_length = prefix_length; a.read_length = read_length; a.min_logit = min_logit;
  for (int g = 0; g < 2; ++g) {
    a.ra[g] = (int4*)(w + l.ra[g]);
    a.ro[g] = (int64_t*)(w + l.ro[g]);
    a.mn[g] = (int2*)(w + l.ra[1] + (size_t)g * (size_t)n * 8);               // both inside ra[1]: 2 x 8 n = 16 n bytes
  }
  a.next = (int32_t*)(w + l.i32[0]); a.prev = (int32_t*)(w + l.i32[1]); a.pedge = (int32_t*)(w + l.i32[2]);
  a.plen = (int32_t*)(w + l.i32[3]); a.pre_f = (int32_t*)(w + l.i32[4]); a.pre_l = (int32_t*)(w + l.i32[5]);
  a.contig_ptr = contig_ptr; a.walk_nodes = walk_nodes; a.walk_edges = walk_edges; a.contig_wrong = contig_wrong;
  a.contig_bases = contig_bases;
  a.rec = (unsigned long long*)record;
  int K = 1;
  while (((int64_t)1 << K) < n) ++K;                    // ceil(log2(max(n, 2)))
  const dim3 grid(persistent_grid(n, kBlock, 8)), blk(kBlock);
  if (n > 0) {
    hipLaunchKernelGGL(bog_link_k, grid, blk, 0, st, a);
    for (int r = 0; r < K; ++r) hipLaunchKernelGGL(bog_min_k, grid, blk, 0, st, a, r & 1);
    hipLaunchKernelGGL(bog_rank_init_k, grid, blk, 0, st, a, K & 1);
    for (int r = 0; r < K; ++r) hipLaunchKernelGGL(bog_rank_k, grid, blk, 0, st, a, r & 1, r == K - 1 ? 1 : 0);
  }
  // n == 0: the middle phase alone -- contig_ptr[0] = 0, calls += 1
  scan_launch<int32_t, 4, 2>(BogScan{{}, a}, {n, {(int32_t*)(w + l.bsum[0]), (int32_t*)(w + l.bsum[1])}, {a.pre_f, a.pre_l}}, st);
  if (n > 0) hipLaunchKernelGGL(bog_layout_k, grid, blk, 0, st, a, K & 1);
  GNM_LAUNCH_CHECK("bog_contigs");
  return 0;
}
