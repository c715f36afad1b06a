// Ground-truth edge labels on the device (include/gnm.h, "ground-truth labels"): y per edge from the reads' positions, over the index
// the graph already carries.  csrc/gnm_labels.h holds the arithmetic; gnm_gt_labels_host runs the same header on host pointers.
//
// Everything node-shaped lives in the workspace in the index's INTERNAL numbering (the caller's arrays are gathered through nperm
// once, by gt_init_k); a key carries the CALLER's node id, so "the node a key names" goes through nrank.  Launches:
//   gt_init_k        per node: the check (gt_node_ok_), ns / ne / plus, L = its own root key, the flags and the top slot cleared.
//   gt_flags_k       per edge, internal order: its class (gt_edge_class_) -> vflag, the five class counters, touched[] at both ends
//                    of a valid edge (a plain store of the same value by every writer).
//   gt_begin_k       the call's `changed` words: 0, or -1 when the input is invalid (every later launch then returns at once).
//   gt_cc_round_k    components, one round: for a valid edge u - v, m = min(L[L[u]], L[L[v]]) is offered to the parents of u and v
//                    (hooking), to u and v themselves (aggressive hooking; it also is their shortcut, m <= L[L[u]]).  L[x] only
//                    falls and always is the key of a node of x's component, so the rounds end -- no offer lowered anything -- with
//                    L constant on every component and equal to its smallest key, whatever the order: the label IS the root.  A
//                    64-bit atomicMin per offer that may lower; the value it leaves does not depend on the order.
//   gt_fwd_begin_k   fwd = the roots.
//   gt_reach_round_k<D>   one round of fwd (D = 1: an unreached node pulls along its in-row) or bwd (D = 0: along its out-row, among
//                    the nodes of fwd): eight lanes per node (gnm_group.h) look for a reached neighbour over a valid edge.  A
//                    workgroup owns a contiguous range of nodes and sweeps it kGtSweeps times per launch, fwd ascending, bwd
//                    descending, a window of kGroupNodes nodes at a time and each window until it reaches nothing more; a flag another group set in the same launch may be seen early or late: flags only rise, so every
//                    schedule ends in the same least fixpoint, and only the NUMBER of rounds depends on it.  No atomics but the
//                    workgroup's count.
//   gt_top_k         the top of every component: a 64-bit atomicMax of (end, ~id) over fwd into the root's slot.
//   gt_bwd_begin_k   bwd = the tops.
//   gt_nodes_k       component, top, backbone per node in the caller's numbering; components, singletons, backbone nodes.
//   gt_emit_k        per edge: y and valid through perm, plain stores, ONE writer per edge -- a valid edge reads its two ends, a
//                    - strand edge a -> b the + strand edge b^1 -> a^1 it mirrors, which exists when a lower-bound search of the
//                    out-row finds it (or `twin` names it).  positives, twin_missing.
// Bounds.  Rows are clamped (row_clamped); a node taken from isrc / idst / out_dst / nperm / nrank is checked against n and an edge
// id against E before it addresses anything; keys hold ids this file wrote.
#include "gnm_common.h"
#include "gnm_group.h"
#include "gnm_labels.h"

namespace gnm {

constexpr int kGtSweeps = 2;            // sweeps of a workgroup over its node range per reachability launch
enum { kGtTotInvalid = 0, kGtTotWords = 2 };

struct GtArgs {
  IndexRows ix;
  const int32_t *idst, *nrank;
  const int64_t *start, *end, *strand;   // the caller's numbering
  int64_t *ns, *ne;                      // internal numbering from here on
  unsigned long long *L, *topkey, *tot;
  int32_t *plus, *touched, *fwd, *bwd;
  uint8_t* vflag;
  const int64_t* twin;
  const int32_t *src, *dst;              // the caller's edge list: read only to check a twin entry
  float* y;
  uint8_t *valid, *backbone;
  int32_t *component, *top;
  unsigned long long* rec;
};

__device__ __forceinline__ unsigned long long gt_ld(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int gt_ldf(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gt_stf(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the caller's id of internal node i, and back; n (outside the index) for an entry that does not name a node
__device__ __forceinline__ unsigned gt_cid(const GtArgs& a, unsigned i) {
  const unsigned c = a.ix.nperm ? (unsigned)a.ix.nperm[i] : i;
  return c < (unsigned)a.ix.n ? c : (unsigned)a.ix.n;
}
__device__ __forceinline__ unsigned gt_iid(const GtArgs& a, unsigned c) {
  if (c >= (unsigned)a.ix.n) return (unsigned)a.ix.n;
  const unsigned i = a.nrank ? (unsigned)a.nrank[c] : c;
  return i < (unsigned)a.ix.n ? i : (unsigned)a.ix.n;
}
__device__ __forceinline__ bool gt_bad(const GtArgs& a) { return a.tot[kGtTotInvalid] != 0ull; }   // the same for a whole launch

__global__ __launch_bounds__(kBlock) void gt_init_k(GtArgs a) {
  __shared__ unsigned lds[kWavesPerBlock];
  const unsigned n = (unsigned)a.ix.n;
  unsigned invalid = 0u;
  for (int64_t i64 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i64 < a.ix.n; i64 += (int64_t)gridDim.x * kBlock) {
    const unsigned i = (unsigned)i64, c = gt_cid(a, i);
    bool ok = c < n && gt_iid(a, c) == i;
    int64_t s = 0, e = 1, t = 1;
    if (ok) {
      s = a.start[c];
      e = a.end[c];
      t = a.strand[c];
      ok = gt_node_ok_(s, e, t);
    }
    invalid += ok ? 0u : 1u;
    a.ns[i] = ok ? s : 0;
    a.ne[i] = ok ? e : 1;
    a.plus[i] = ok && t == 1 ? 1 : 0;
    a.L[i] = ok ? gt_root_key_(s, c) : ~0ull;
    a.topkey[i] = 0ull;
    a.touched[i] = 0;
    a.fwd[i] = 0;
    a.bwd[i] = 0;
  }
  const unsigned bad = block_sum(invalid, lds);
  if (threadIdx.x == 0 && bad) {
    atomicAdd(a.tot + kGtTotInvalid, (unsigned long long)bad);
    atomicAdd(a.rec + kGtInvalid, (unsigned long long)bad);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.rec + kGtCalls, 1ull);
}

__global__ __launch_bounds__(kBlock) void gt_flags_k(GtArgs a) {
  __shared__ unsigned lds[kWavesPerBlock];
  if (gt_bad(a)) return;
  const unsigned n = (unsigned)a.ix.n;
  unsigned cnt[kGtBackward + 1] = {};
  unsigned invalid = 0u;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.ix.E; j += (int64_t)gridDim.x * kBlock) {
    const unsigned s = (unsigned)a.ix.isrc[j], d = (unsigned)a.idst[j];
    int c = -1;
    if (s < n && d < n) c = gt_edge_class_(a.plus[s] != 0, a.plus[d] != 0, s == d, a.ns[s], a.ne[s], a.ns[d]);
    else invalid += 1u;
    a.vflag[j] = c == kGtValid ? 1 : 0;
    cnt[kGtEdges] += 1u;
#pragma unroll
    for (int k = kGtValid; k <= kGtBackward; ++k) cnt[k] += c == k ? 1u : 0u;
    if (c == kGtValid) {
      a.touched[s] = 1;
      a.touched[d] = 1;
    }
  }
#pragma unroll
  for (int k = 0; k <= kGtBackward; ++k) block_count_add(cnt[k], lds, a.rec + k);
  const unsigned bad = block_sum(invalid, lds);
  if (threadIdx.x == 0 && bad) {
    atomicAdd(a.tot + kGtTotInvalid, (unsigned long long)bad);
    atomicAdd(a.rec + kGtInvalid, (unsigned long long)bad);
  }
}

__global__ __launch_bounds__(kBlock) void gt_begin_k(GtArgs a, long long* changed, int rounds) {
  const long long v = gt_bad(a) ? -1ll : 0ll;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rounds; r += (int64_t)gridDim.x * kBlock) changed[r] = v;
}

// offer m to L[x]: 1 when it lowered it
__device__ __forceinline__ unsigned gt_lower(unsigned long long* p, unsigned long long m) {
  if (gt_ld(p) <= m) return 0u;
  return atomicMin(p, m) > m ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void gt_cc_round_k(GtArgs a, unsigned long long* word) {
  __shared__ unsigned lds[kWavesPerBlock];
  if (gt_bad(a)) return;
  const unsigned n = (unsigned)a.ix.n;
  unsigned lowered = 0u;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.ix.E; j += (int64_t)gridDim.x * kBlock) {
    if (!a.vflag[j]) continue;
    const unsigned u = (unsigned)a.ix.isrc[j], v = (unsigned)a.idst[j];      // checked by gt_flags_k: a valid edge's ends are nodes
    const unsigned pu = gt_iid(a, gt_root_id_(gt_ld(a.L + u))), pv = gt_iid(a, gt_root_id_(gt_ld(a.L + v)));
    if (pu >= n || pv >= n) continue;
    const unsigned long long gu = gt_ld(a.L + pu), gv = gt_ld(a.L + pv), m = gu < gv ? gu : gv;
    lowered += gt_lower(a.L + pu, m) + gt_lower(a.L + pv, m) + gt_lower(a.L + u, m) + gt_lower(a.L + v, m);
  }
  block_count_add(lowered, lds, word);
}

// Is internal node i the one its own label names?  (After the component rounds: the roots.)
__device__ __forceinline__ bool gt_is_root(const GtArgs& a, unsigned i) { return a.plus[i] && gt_iid(a, gt_root_id_(a.L[i])) == i; }

__global__ __launch_bounds__(kBlock) void gt_fwd_begin_k(GtArgs a) {
  if (gt_bad(a)) return;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.ix.n; i += (int64_t)gridDim.x * kBlock)
    if (gt_is_root(a, (unsigned)i)) a.fwd[i] = 1;
}

template <int D>
__global__ __launch_bounds__(kBlock) void gt_reach_round_k(GtArgs a, unsigned long long* word) {
  __shared__ unsigned lds[kWavesPerBlock];
  if (gt_bad(a)) return;
  int32_t* flag = D ? a.fwd : a.bwd;
  const unsigned n = (unsigned)a.ix.n;
  const int sub = threadIdx.x & (kGroupLanes - 1), grp = threadIdx.x / kGroupLanes;
  // this workgroup's nodes [lo, hi): a whole number of passes, so that every lane of a wave takes the same number of them
  const int64_t per = ((a.ix.n + gridDim.x - 1) / gridDim.x + kGroupNodes - 1) / kGroupNodes * kGroupNodes;
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < a.ix.n ? lo + per : a.ix.n;
  const int64_t span = lo < hi ? (hi - lo + kGroupNodes - 1) / kGroupNodes * kGroupNodes : 0;
  unsigned reached = 0u;
  for (int sweep = 0; sweep < kGtSweeps; ++sweep) {
    for (int64_t k = 0; k < span; k += kGroupNodes) {
      const int64_t base = D ? lo + k : lo + (span - kGroupNodes - k);         // fwd ascending, bwd descending
      const int64_t i64 = base + grp;
      const bool live = i64 < hi;
      const int i = live ? (int)i64 : 0;
      bool open = live && a.plus[i] && (D || a.fwd[i]) && !gt_ldf(flag + i);   // the same in the eight lanes of a group
      // Speed only: the pass is repeated until it reaches nothing more (at most kGroupNodes times, every repeat reaches a node),
      // so the window does not run ahead of a front that moves a few nodes per hop, and a front that enters the range crosses
      // it in one sweep.  The barrier's answer is the same in every thread of the workgroup.
      for (;;) {
        unsigned found = 0u;
        if (open) {
          int r0, r1;
          row_clamped(D ? a.ix.in_ptr : a.ix.out_ptr, i, (int)a.ix.E, r0, r1);
          walk_candidates<D>(
              a.ix, r0 + sub, r1, [&](int o) { return (unsigned)o < n && gt_ldf(flag + o) != 0; },
              [&](int, int j, int, int) { found |= a.vflag[j] ? 1u : 0u; });
        }
#pragma unroll
        for (int off = kGroupLanes / 2; off > 0; off >>= 1) found |= __shfl_xor(found, off, kGroupLanes);
        if (found) {
          open = false;
          if (sub == 0) {
            gt_stf(flag + i, 1);
            reached += 1u;
          }
        }
        if (!__syncthreads_or((int)found)) break;
      }
    }
  }
  block_count_add(reached, lds, word);
}

__global__ __launch_bounds__(kBlock) void gt_top_k(GtArgs a) {
  if (gt_bad(a)) return;
  const unsigned n = (unsigned)a.ix.n;
  for (int64_t i64 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i64 < a.ix.n; i64 += (int64_t)gridDim.x * kBlock) {
    const unsigned i = (unsigned)i64;
    if (!a.fwd[i]) continue;
    const unsigned r = gt_iid(a, gt_root_id_(a.L[i]));
    if (r < n) atomicMax(a.topkey + r, (unsigned long long)gt_top_key_(a.ne[i], gt_cid(a, i)));
  }
}

__global__ __launch_bounds__(kBlock) void gt_bwd_begin_k(GtArgs a) {
  if (gt_bad(a)) return;
  const unsigned n = (unsigned)a.ix.n;
  for (int64_t i64 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i64 < a.ix.n; i64 += (int64_t)gridDim.x * kBlock) {
    const unsigned i = (unsigned)i64;
    if (!a.fwd[i]) continue;
    const unsigned r = gt_iid(a, gt_root_id_(a.L[i]));
    if (r < n && a.topkey[r] == gt_top_key_(a.ne[i], gt_cid(a, i))) a.bwd[i] = 1;
  }
}

__global__ __launch_bounds__(kBlock) void gt_nodes_k(GtArgs a) {
  __shared__ unsigned lds[kWavesPerBlock];
  if (gt_bad(a)) return;
  const unsigned n = (unsigned)a.ix.n;
  unsigned comps = 0u, single = 0u, bbn = 0u;
  for (int64_t i64 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i64 < a.ix.n; i64 += (int64_t)gridDim.x * kBlock) {
    const unsigned i = (unsigned)i64, c = gt_cid(a, i);
    if (c >= n) continue;
    int comp = -1, top = -1;
    bool bb = false;
    if (a.plus[i]) {
      const unsigned rc = gt_root_id_(a.L[i]), r = gt_iid(a, rc);
      comp = (int)rc;
      if (r < n) top = (int)gt_top_id_(a.topkey[r]);
      bb = a.fwd[i] && a.bwd[i];
      if (r == i) {
        comps += 1u;
        single += a.touched[i] ? 0u : 1u;
      }
    }
    a.component[c] = comp;
    a.top[c] = top;
    a.backbone[c] = bb ? 1 : 0;
    bbn += bb ? 1u : 0u;
  }
  block_count_add(comps, lds, a.rec + kGtComponents);
  block_count_add(single, lds, a.rec + kGtSingletons);
  block_count_add(bbn, lds, a.rec + kGtBackbone);
}

// Does the caller's edge list hold ca -> cb?  `e`: the asking edge, whose twin entry is believed only when it names that pair;
// without twins a lower-bound search for cb's internal id in the ascending destinations of ca's out-row.
__device__ __forceinline__ bool gt_has_edge(const GtArgs& a, int e, unsigned ca, unsigned cb) {
  const unsigned n = (unsigned)a.ix.n;
  if (ca >= n || cb >= n) return false;
  if (a.twin) return gt_twin_is_(a.src, a.dst, a.ix.E, a.twin[e], ca, cb);
  const unsigned ia = gt_iid(a, ca), ib = gt_iid(a, cb);
  if (ia >= n || ib >= n) return false;
  int lo, end;
  row_clamped(a.ix.out_ptr, (int)ia, (int)a.ix.E, lo, end);
  for (int hi = end; lo < hi;) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a.ix.out_dst[mid] < (int)ib) lo = mid + 1; else hi = mid;
  }
  return lo < end && a.ix.out_dst[lo] == (int)ib;
}

__global__ __launch_bounds__(kBlock) void gt_emit_k(GtArgs a) {
  __shared__ unsigned lds[kWavesPerBlock];
  if (gt_bad(a)) return;
  const unsigned n = (unsigned)a.ix.n, E = (unsigned)a.ix.E;
  unsigned pos = 0u, missing = 0u;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.ix.E; j += (int64_t)gridDim.x * kBlock) {
    const unsigned e = (unsigned)a.ix.perm[j], s = (unsigned)a.ix.isrc[j], d = (unsigned)a.idst[j];
    if (e >= E || s >= n || d >= n) continue;
    const bool vf = a.vflag[j] != 0;
    bool one = false;
    if (vf) {
      one = a.fwd[s] && a.bwd[s] && a.fwd[d] && a.bwd[d];
      if (one && !gt_has_edge(a, (int)e, gt_cid(a, d) ^ 1u, gt_cid(a, s) ^ 1u)) missing += 1u;
    } else if (!a.plus[s] && !a.plus[d] && s != d) {
      const unsigned ca = gt_cid(a, d) ^ 1u, cb = gt_cid(a, s) ^ 1u, ia = gt_iid(a, ca), ib = gt_iid(a, cb);   // e mirrors ca -> cb
      if (ia < n && ib < n && a.fwd[ia] && a.bwd[ia] && a.fwd[ib] && a.bwd[ib] &&
          gt_edge_class_(a.plus[ia] != 0, a.plus[ib] != 0, ia == ib, a.ns[ia], a.ne[ia], a.ns[ib]) == kGtValid)
        one = gt_has_edge(a, (int)e, ca, cb);
    }
    a.y[e] = one ? 1.0f : 0.0f;
    a.valid[e] = vf ? 1 : 0;
    pos += one ? 1u : 0u;
  }
  block_count_add(pos, lds, a.rec + kGtPositives);
  block_count_add(missing, lds, a.rec + kGtTwinMissing);
}

}  // namespace gnm

using namespace gnm;

// ws: ns, ne, L, topkey (8 n each), plus, touched, fwd, bwd (4 n each), vflag (E), the totals
struct GtLayout {
  size_t node8[4], node4[4], edge, tot, bytes;
};
static GtLayout gt_layout(int64_t n, int64_t E) {
  GtLayout l;
  size_t off = 0;
  for (int i = 0; i < 4; ++i) { l.node8[i] = off; off += ws_pad((size_t)n * 8); }
  for (int i = 0; i < 4; ++i) { l.node4[i] = off; off += ws_pad((size_t)n * 4); }
  l.edge = off; off += ws_pad((size_t)E);
  l.tot = off; off += ws_pad(kGtTotWords * 8);
  l.bytes = off;
  return l;
}

extern "C" size_t gnm_gt_workspace_bytes(int64_t n, int64_t E) {
  if (n < 0 || E < 0 || n >= INT32_MAX || E >= INT32_MAX) return 0;
  return gt_layout(n, E).bytes;
}

extern "C" int gnm_gt_sweeps(void) { return kGtSweeps; }

// the checks the device entry points share, and the argument block over the workspace
static int gt_args(const char* what, int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst,
                   const int32_t* in_ptr, const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                   const int32_t* nrank, void* ws, size_t ws_bytes, GtArgs& a) {
  if (index_size_check(what, n, E, "the index holds 32-bit positions")) return -1;
  GNM_CHECK_ARG(n == 0 || (in_ptr && out_ptr), "%s: in_ptr and out_ptr must not be null when n > 0", what);
  GNM_CHECK_ARG(E == 0 || (perm && isrc && idst && out_pos && out_dst),
                "%s: perm, isrc, idst, out_pos and out_dst must not be null when E > 0", what);
  GNM_CHECK_ARG((nperm == nullptr) == (nrank == nullptr), "%s: nperm and nrank come together or not at all", what);
  const GtLayout l = gt_layout(n, E);
  if (ws_check(what, "gnm_gt_workspace_bytes", ws, ws_bytes, l.bytes)) return -1;
  char* w = (char*)ws;
  a = GtArgs{};
  a.ix = IndexRows{n, E, perm, isrc, in_ptr, out_ptr, out_pos, out_dst, nperm};
  a.idst = idst; a.nrank = nrank;
  a.ns = (int64_t*)(w + l.node8[0]); a.ne = (int64_t*)(w + l.node8[1]);
  a.L = (unsigned long long*)(w + l.node8[2]); a.topkey = (unsigned long long*)(w + l.node8[3]);
  a.plus = (int32_t*)(w + l.node4[0]); a.touched = (int32_t*)(w + l.node4[1]);
  a.fwd = (int32_t*)(w + l.node4[2]); a.bwd = (int32_t*)(w + l.node4[3]);
  a.vflag = (uint8_t*)(w + l.edge);
  a.tot = (unsigned long long*)(w + l.tot);
  return 0;
}

static dim3 gt_grid(int64_t items) { return dim3(persistent_grid(items > 0 ? items : 1, kBlock, 8)); }

extern "C" int gnm_gt_prepare(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                              const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                              const int32_t* nrank, const int64_t* start, const int64_t* end, const int64_t* strand, void* record,
                              void* ws, size_t ws_bytes, void* stream) {
  GtArgs a;
  if (gt_args("gt_prepare", n, E, perm, isrc, idst, in_ptr, out_ptr, out_pos, out_dst, nperm, nrank, ws, ws_bytes, a)) return -1;
  if (record_check("gt_prepare", record, "gnm_gt_record")) return -1;
  GNM_CHECK_ARG(n == 0 || (start && end && strand), "gt_prepare: start, end and strand must not be null when n > 0");
  a.start = start; a.end = end; a.strand = strand; a.rec = (unsigned long long*)record;
  hipStream_t st = (hipStream_t)stream;
  hipError_t err = hipMemsetAsync(a.tot, 0, kGtTotWords * 8, st);
  if (err != hipSuccess) return hip_fail(err, "gt_prepare");
  hipLaunchKernelGGL(gt_init_k, gt_grid(n), dim3(kBlock), 0, st, a);
  if (E > 0) hipLaunchKernelGGL(gt_flags_k, gt_grid(E), dim3(kBlock), 0, st, a);
  GNM_LAUNCH_CHECK("gt_prepare");
  return 0;
}

extern "C" int gnm_gt_rounds(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                             const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                             const int32_t* nrank, int stage, int64_t first_round, int64_t rounds, int64_t* changed, void* ws,
                             size_t ws_bytes, void* stream) {
  GtArgs a;
  if (gt_args("gt_rounds", n, E, perm, isrc, idst, in_ptr, out_ptr, out_pos, out_dst, nperm, nrank, ws, ws_bytes, a)) return -1;
  GNM_CHECK_ARG(stage >= 0 && stage <= 2, "gt_rounds: stage = %d: expected 0 (components), 1 (fwd) or 2 (bwd)", stage);
  GNM_CHECK_ARG(first_round >= 0 && rounds >= 0 && rounds < (1 << 20), "gt_rounds: first_round = %lld, rounds = %lld: expected "
                "first_round >= 0 and 0 <= rounds < 2^20", (long long)first_round, (long long)rounds);
  GNM_CHECK_ARG(rounds == 0 || (changed && ((uintptr_t)changed & 7) == 0),
                "gt_rounds: changed must be a non-null, 8-byte aligned int64 [rounds] array when rounds > 0");
  if (rounds == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kBlock);
  if (first_round == 0 && stage == 1) hipLaunchKernelGGL(gt_fwd_begin_k, gt_grid(n), blk, 0, st, a);
  if (first_round == 0 && stage == 2) {
    hipLaunchKernelGGL(gt_top_k, gt_grid(n), blk, 0, st, a);
    hipLaunchKernelGGL(gt_bwd_begin_k, gt_grid(n), blk, 0, st, a);
  }
  hipLaunchKernelGGL(gt_begin_k, gt_grid(rounds), blk, 0, st, a, (long long*)changed, (int)rounds);
  if (E > 0 && n > 0) {
    const dim3 ngrid(persistent_grid(n, kGroupNodes, 8));
    for (int64_t r = 0; r < rounds; ++r) {
      unsigned long long* word = (unsigned long long*)changed + r;
      if (stage == 0) hipLaunchKernelGGL(gt_cc_round_k, gt_grid(E), blk, 0, st, a, word);
      else if (stage == 1) hipLaunchKernelGGL(gt_reach_round_k<1>, ngrid, blk, 0, st, a, word);
      else hipLaunchKernelGGL(gt_reach_round_k<0>, ngrid, blk, 0, st, a, word);
    }
  }
  GNM_LAUNCH_CHECK("gt_rounds");
  return 0;
}

extern "C" int gnm_gt_emit(int64_t n, int64_t E, const int32_t* perm, const int32_t* isrc, const int32_t* idst, const int32_t* in_ptr,
                           const int32_t* out_ptr, const int32_t* out_pos, const int32_t* out_dst, const int32_t* nperm,
                           const int32_t* nrank, const int64_t* twin, const int32_t* src, const int32_t* dst, float* y, uint8_t* valid,
                           uint8_t* backbone, int32_t* component, int32_t* top, void* record, void* ws, size_t ws_bytes, void* stream) {
  GtArgs a;
  if (gt_args("gt_emit", n, E, perm, isrc, idst, in_ptr, out_ptr, out_pos, out_dst, nperm, nrank, ws, ws_bytes, a)) return -1;
  if (record_check("gt_emit", record, "gnm_gt_record")) return -1;
  GNM_CHECK_ARG(n == 0 || (backbone && component && top), "gt_emit: backbone, component and top must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || (y && valid), "gt_emit: y and valid must not be null when E > 0");
  GNM_CHECK_ARG(twin == nullptr || E == 0 || (src && dst), "gt_emit: src and dst must not be null when twin is given");
  a.twin = E > 0 ? twin : nullptr; a.src = src; a.dst = dst;
  a.y = y; a.valid = valid; a.backbone = backbone; a.component = component; a.top = top; a.rec = (unsigned long long*)record;
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) hipLaunchKernelGGL(gt_nodes_k, gt_grid(n), dim3(kBlock), 0, st, a);
  if (E > 0) hipLaunchKernelGGL(gt_emit_k, gt_grid(E), dim3(kBlock), 0, st, a);
  GNM_LAUNCH_CHECK("gt_emit");
  return 0;
}

extern "C" int gnm_gt_labels_host(int64_t n, int64_t E, const int32_t* src, const int32_t* dst, const int64_t* start, const int64_t* end,
                                  const int64_t* strand, const int64_t* twin, float* y, uint8_t* valid, uint8_t* backbone,
                                  int32_t* component, int32_t* top, void* record) {
  if (index_size_check("gt_labels_host", n, E, "node and edge ids are 32-bit")) return -1;
  if (record_check("gt_labels_host", record, "gnm_gt_record")) return -1;
  GNM_CHECK_ARG(n == 0 || (start && end && strand && backbone && component && top),
                "gt_labels_host: start, end, strand, backbone, component and top must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || (src && dst && y && valid), "gt_labels_host: src, dst, y and valid must not be null when E > 0");
  const int64_t bad = gt_host_invalid_(n, E, src, dst, start, end, strand);
  if (bad) {
    ((int64_t*)record)[kGtInvalid] += bad;
    GNM_CHECK_ARG(false, "gt_labels_host: %lld nodes or edges are unusable: expected 0 <= start < end < 2^32, strand +1 or -1, and "
                  "src, dst in [0, n)", (long long)bad);
  }
  gt_labels_host_(n, E, src, dst, start, end, strand, E > 0 ? twin : nullptr, GtHostOut{y, valid, backbone, component, top, (int64_t*)record});
  return 0;
}
