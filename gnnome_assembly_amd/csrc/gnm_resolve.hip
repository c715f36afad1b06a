// One strand per read on the device (include/gnm.h, "resolve strands"): decode.resolve_strands -- the contigs by descending bases,
// a node whose read is taken ends the piece, a piece of at least thr nodes is kept and takes its reads -- restated as rounds of
// independent contigs.  In a path cover a node lies on at most one contig, so taken[r] for a read r of contig c is written by c
// or by the one contig that holds r's other strand.  c is READY when every such contig is c itself, comes later in the priority
// order, or is done; two ready contigs share no read, and the first undecided contig of the order is always ready.
//
// One wave per contig throughout (the contigs of a trained model hold 10^4 - 10^5 nodes; the wave strides its contig in chunks
// of 64 positions).  Launches:
//   res_init_k      contig_of = -1, taken = stamp = 0, rank = -1, kn = kp = 0, the totals.
//   res_scatter_k   contig_of[v] = c and pos_of[v] = p for every walk position, rank[order[k]] = k.
//   res_flags_k     the checks -- a node outside [0, n), an inner edge id outside [0, E), a contig_ptr entry that does not ascend
//                   inside [0, P], an order entry outside [0, C), and a node or order entry listed twice, found by re-reading
//                   pos_of[walk_nodes[p]] != p (rank[order[k]] != k), which does not depend on which store won -- then per
//                   contig: done = 0 when it holds fewer than thr nodes (never walked), "undecided" otherwise, and serial = 1 when
//                   some read has both strands on it.
//   res_begin_k     the call's `undecided` words: 0, or -1 when the input is invalid (every later launch then returns at once).
//   res_round_k  r  the ready test against the done words of the rounds BEFORE r (a contig finished in round r stores r, which
//                   reads as "not done" to every other wave of the launch, exactly like "undecided"), then the cut:
//                   ordinary contig  pass 1: ballot of the free positions of a chunk -> run[p] = the start of p's run (the open run
//                                    is carried across chunks), rlen[start] = its length, stored where it ends; pass 2: a position
//                                    whose run has rlen >= thr is kept and marks its read.  No read occurs twice on such a contig,
//                                    so pass 1 sees no mark of pass 2.
//                   serial contig    lane 0 runs the host's loop as written; stamp[r] == lo + 1 stands for "r in inside" (lo only
//                                    grows and positions are unique, so a token is never used twice).
//                   Both leave run[p] = 0 (not kept), 1 (kept) or 2 (kept, first node of its piece), kn[c] / kp[c] = kept nodes /
//                   pieces, done[c] = r.  The contigs still undecided are counted into undecided[j]: one atomic per workgroup.
//   scan_launch     exclusive prefix sums of kn and kp in PRIORITY order (through `order`): the three launches of gnm_scan.h over
//                   blocks of 4 kBlock contigs, a thread owning four consecutive ranks (ResScan): where every contig's pieces and
//                   nodes start.
//   res_gather_k    the kept positions to out_nodes / out_edges (-1 at a piece's first node), out_ptr at the piece starts: wave
//                   scans of the two flags, carried across chunks.
//   res_piece_k     one wave per piece: bases = the sum of prefix_length over its inner links + read_length of its last node,
//                   wrong = its inner links whose label is not 1.
// Integers only.  Atomics: one integer add per workgroup and counter.  No workgroup waits for another; the ready test reads only
// what earlier launches wrote or a word whose two possible values mean the same, so every output is a function of the inputs alone,
// whatever the grid.
//
// Bounds.  contig_ptr rows are clamped to 0 <= lo <= hi <= P (a row that needed it is counted invalid and emptied); a node is
// checked against n and an edge id against E before they address anything; contig_of / rank hold values this file wrote.
#include "gnm_common.h"
#include "gnm_scan.h"

namespace gnm {

constexpr int kResUndecided = INT32_MAX;
enum { kResContigs = 0, kResEligible, kResPieces, kResDropped, kResNodes, kResSerial, kResInvalid, kResCalls };
enum { kTotInvalid = 0, kTotNodes, kTotPieces, kTotWords = 4 };

struct ResArgs {
  int64_t C, P, n, E, R;                 // R = n / 2 + 1 reads
  int thr;
  const int32_t *contig_ptr, *walk_nodes, *walk_edges, *order;
  const int64_t *prefix_length, *read_length;
  const float* y;
  int32_t *contig_of, *pos_of, *taken, *stamp, *rank, *done, *serial, *kn, *kp, *noff, *poff, *run, *rlen, *bsum[2];
  unsigned long long* tot;
  int32_t *out_ptr, *out_nodes, *out_edges, *out_wrong;
  int64_t* out_bases;
  unsigned long long* rec;
};

__device__ __forceinline__ int res_ld(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void res_st(int32_t* p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// body(c, lane) for the contigs of this wave; c is wave-uniform
template <class Body>
__device__ __forceinline__ void for_wave_contigs(int64_t C, Body body) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t c = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); c < C; c += step) body((int)c, lane);
}

// the positions [lo, hi) of contig c; false (and an empty range) when contig_ptr does not ascend inside [0, P]
__device__ __forceinline__ bool res_range(const ResArgs& a, int c, int& lo, int& hi) {
  lo = a.contig_ptr[c];
  hi = a.contig_ptr[c + 1];
  const bool ok = lo >= 0 && lo <= hi && (int64_t)hi <= a.P;
  if (!ok) lo = hi = 0;
  return ok;
}

__global__ __launch_bounds__(kBlock) void res_init_k(ResArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
  for (int64_t v = t0; v < a.n; v += step) a.contig_of[v] = -1;
  for (int64_t r = t0; r < a.R; r += step) {
    a.taken[r] = 0;
    a.stamp[r] = 0;
  }
  for (int64_t c = t0; c < a.C; c += step) {
    a.rank[c] = -1;
    a.kn[c] = 0;
    a.kp[c] = 0;
  }
  if (t0 < kTotWords) a.tot[t0] = 0ull;
}

__global__ __launch_bounds__(kBlock) void res_scatter_k(ResArgs a) {
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
  for (int64_t k = t0; k < a.C; k += step) {
    const unsigned o = (unsigned)a.order[k];
    if (o < (unsigned)a.C) a.rank[o] = (int32_t)k;
  }
  const unsigned n = (unsigned)a.n;
  for_wave_contigs(a.C, [&](int c, int lane) {
    int lo, hi;
    res_range(a, c, lo, hi);
    for (int p = lo + lane; p < hi; p += 64) {
      const unsigned v = (unsigned)a.walk_nodes[p];
      if (v < n) {
        a.contig_of[v] = c;
        a.pos_of[v] = p;
      }
    }
  });
}

__global__ __launch_bounds__(kBlock) void res_flags_k(ResArgs a) {
  __shared__ unsigned lds[kWavesPerBlock];
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock;
  const unsigned n = (unsigned)a.n, E = (unsigned)a.E;
  unsigned invalid = 0u, eligible = 0u, serial = 0u;
  for (int64_t k = t0; k < a.C; k += step) {
    const unsigned o = (unsigned)a.order[k];
    if (o >= (unsigned)a.C || a.rank[o] != (int32_t)k) invalid += 1u;
  }
  for_wave_contigs(a.C, [&](int c, int lane) {
    int lo, hi;
    if (!res_range(a, c, lo, hi) && lane == 0) invalid += 1u;
    bool both = false;
    for (int p = lo + lane; p < hi; p += 64) {
      const unsigned v = (unsigned)a.walk_nodes[p];
      if (v >= n || a.pos_of[v] != p || (p > lo && (unsigned)a.walk_edges[p] >= E)) {
        invalid += 1u;
        continue;
      }
      const unsigned w = v ^ 1u;
      if (w < n && a.contig_of[w] == c) both = true;
    }
    const bool ser = __any(both) != 0, elig = hi - lo >= a.thr;
    if (lane == 0) {
      a.serial[c] = ser ? 1 : 0;
      a.done[c] = elig ? kResUndecided : 0;
      eligible += elig ? 1u : 0u;
      serial += elig && ser ? 1u : 0u;
    }
  });
  const unsigned bad = block_sum(invalid, lds);
  if (threadIdx.x == 0 && bad) {
    atomicAdd(a.tot + kTotInvalid, (unsigned long long)bad);
    atomicAdd(a.rec + kResInvalid, (unsigned long long)bad);
  }
  block_count_add(eligible, lds, a.rec + kResEligible);
  block_count_add(serial, lds, a.rec + kResSerial);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (a.C > 0) atomicAdd(a.rec + kResContigs, (unsigned long long)a.C);
    atomicAdd(a.rec + kResCalls, 1ull);
  }
}

__global__ __launch_bounds__(kBlock) void res_begin_k(ResArgs a, long long* undecided, int rounds) {
  const long long v = a.tot[kTotInvalid] != 0ull ? -1ll : 0ll;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rounds; r += (int64_t)gridDim.x * kBlock) undecided[r] = v;
}

// The serial cut's close(): the piece of positions [x0, x1) is kept -- marked in run and its reads taken -- when it holds at least
// thr nodes; true when kept.
__device__ __forceinline__ bool res_close_(const ResArgs& a, int x0, int x1) {
  if (x1 - x0 < a.thr) return false;
  for (int q = x0; q < x1; ++q) {
    a.run[q] = q == x0 ? 2 : 1;
    const unsigned v = (unsigned)a.walk_nodes[q];
    if (v < (unsigned)a.n) a.taken[v >> 1] = 1;
  }
  return true;
}

__global__ __launch_bounds__(kBlock) void res_round_k(ResArgs a, int r, unsigned long long* word) {
  __shared__ unsigned lds[kWavesPerBlock];
  if (a.tot[kTotInvalid] != 0ull) return;               // the same for every thread of the launch
  const unsigned n = (unsigned)a.n;
  const int thr = a.thr;
  unsigned left = 0u, dropped = 0u;
  for_wave_contigs(a.C, [&](int c, int lane) {
    if (res_ld(a.done + c) != kResUndecided) return;
    int lo, hi;
    res_range(a, c, lo, hi);
    // ready: every contig that holds the other strand of one of c's reads is c, comes later, or was done before this round
    const int rk = a.rank[c];
    bool wait = false;
    for (int base = lo; base < hi; base += 64) {
      const int p = base + lane;
      if (p < hi) {
        const unsigned w = (unsigned)a.walk_nodes[p] ^ 1u;
        if (w < n) {
          const int d = a.contig_of[w];
          if (d >= 0 && d != c && a.rank[d] < rk && res_ld(a.done + d) >= r) wait = true;
        }
      }
      if (__any(wait)) break;
    }
    if (__any(wait)) {
      if (lane == 0) left += 1u;
      return;
    }
    unsigned kn = 0u, kp = 0u;
    if (!a.serial[c]) {
      // pass 1: the maximal runs of free positions; `carry` = the start of the run that is open at the chunk's first position
      int carry = -1;
      for (int base = lo; base < hi; base += 64) {
        const int p = base + lane;
        const bool in = p < hi;
        const unsigned v = in ? (unsigned)a.walk_nodes[p] : 0u;
        const bool fr = in && v < n && a.taken[v >> 1] == 0;
        const unsigned long long m = __ballot(fr);
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);
        const int start = below ? base + 64 - __clzll((long long)below) : (carry >= 0 ? carry : base);
        bool ends = fr;
        if (lane == 63) ends = ends && base + 64 >= hi;
        else ends = ends && !((m >> (lane + 1)) & 1ull);
        if (in) a.run[p] = fr ? start : -1;
        if (ends) a.rlen[start] = p + 1 - start;
        if (lane == 0 && carry >= 0 && !fr) a.rlen[carry] = base - carry;      // the open run ended with the chunk before
        const int s63 = __shfl(start, 63, 64);
        carry = ((m >> 63) & 1ull) && base + 64 < hi ? s63 : -1;
      }
      __threadfence();                                  // rlen[start] was stored by the lane at the run's end
      // pass 2: keep the runs of at least thr positions
      for (int p = lo + lane; p < hi; p += 64) {
        const int s = a.run[p];
        int mark = 0;
        if (s >= lo && s <= p) {
          const bool keep = a.rlen[s] >= thr;
          if (keep) {
            mark = p == s ? 2 : 1;
            a.taken[(unsigned)a.walk_nodes[p] >> 1] = 1;
            kn += 1u;
          }
          if (p == s) {
            if (keep) kp += 1u;
            else dropped += 1u;
          }
        }
        a.run[p] = mark;
      }
    } else if (lane == 0) {
      // both strands of a read on one contig: decode.resolve_strands' loop as written; stamp[r] == l + 1: r is in the open piece
      int l = lo;
      for (int pos = lo; pos <= hi; ++pos) {
        // what position pos does to the open piece [l, pos): 0 nothing, 1 close it and skip pos, 2 close it, pos starts the next
        // one when it was dropped and is skipped when it was kept
        int act = 1;
        unsigned rd = 0u;
        if (pos < hi) {
          a.run[pos] = 0;
          const unsigned v = (unsigned)a.walk_nodes[pos];
          if (v >= n) continue;
          rd = v >> 1;
          act = a.taken[rd] ? 1 : (a.stamp[rd] == l + 1 ? 2 : 0);
        }
        if (act == 0) {
          a.stamp[rd] = l + 1;
          continue;
        }
        const bool kept = res_close_(a, l, pos);
        kn += kept ? (unsigned)(pos - l) : 0u;
        kp += kept ? 1u : 0u;
        dropped += !kept && pos > l ? 1u : 0u;
        if (act == 2 && !kept) {
          l = pos;
          a.stamp[rd] = l + 1;
        } else {
          l = pos + 1;
        }
      }
    }
    kn = wave_sum(kn);
    kp = wave_sum(kp);
    if (lane == 0) {
      a.kn[c] = (int32_t)kn;
      a.kp[c] = (int32_t)kp;
      res_st(a.done + c, r);
    }
  });
  block_count_add(left, lds, word);
  block_count_add(dropped, lds, a.rec + kResDropped);
}

// The two scanned sequences, in priority order: kept nodes (-> noff) and kept pieces (-> poff) per contig; one look-up of `order`
// feeds both.  Nothing runs on invalid input.
struct ResScan : ScanUser<int32_t, 2> {
  ResArgs a;
  __device__ __forceinline__ bool skip() const { return a.tot[kTotInvalid] != 0ull; }
  __device__ __forceinline__ void load(const Arrays& x, int64_t k0, bool, int32_t (&v)[2][4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[0][i] = v[1][i] = 0;
      if (k0 + i < x.n) {
        const unsigned c = (unsigned)a.order[k0 + i];
        if (c < (unsigned)a.C) {
          v[0][i] = a.kn[c];
          v[1][i] = a.kp[c];
        }
      }
    }
  }
  __device__ __forceinline__ void total(const Arrays&, int s, int32_t total) const {   // the kept nodes / pieces
    a.tot[s == 0 ? kTotNodes : kTotPieces] = (unsigned long long)total;
    if (total > 0) atomicAdd(a.rec + (s == 0 ? kResNodes : kResPieces), (unsigned long long)total);
  }
};

__global__ __launch_bounds__(kBlock) void res_gather_k(ResArgs a) {
  if (a.tot[kTotInvalid] != 0ull) return;
  const unsigned P = (unsigned)a.P;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long K = a.tot[kTotPieces];
    if (K <= (unsigned long long)a.P) a.out_ptr[K] = (int32_t)a.tot[kTotNodes];
  }
  for_wave_contigs(a.C, [&](int c, int lane) {
    if (a.kn[c] <= 0) return;
    const unsigned k = (unsigned)a.rank[c];
    if (k >= (unsigned)a.C) return;
    int lo, hi;
    res_range(a, c, lo, hi);
    int nbase = a.noff[k], pbase = a.poff[k];
    for (int base = lo; base < hi; base += 64) {
      const int p = base + lane;
      const int mark = p < hi ? a.run[p] : 0;
      const int kf = mark > 0 ? 1 : 0, sf = mark == 2 ? 1 : 0;
      int tk, ts;
      const int ik = wave_scan(kf, tk), is = wave_scan(sf, ts);
      if (kf) {
        const unsigned q = (unsigned)(nbase + ik - 1);
        if (q < P) {
          a.out_nodes[q] = a.walk_nodes[p];
          a.out_edges[q] = sf ? -1 : a.walk_edges[p];
          const unsigned j = (unsigned)(pbase + is - 1);
          if (sf && j < P) a.out_ptr[j] = (int32_t)q;
        }
      }
      nbase += tk;
      pbase += ts;
    }
  });
}

__global__ __launch_bounds__(kBlock) void res_piece_k(ResArgs a) {
  if (a.tot[kTotInvalid] != 0ull) return;
  const unsigned long long K64 = a.tot[kTotPieces];
  const int64_t K = K64 <= (unsigned long long)a.P ? (int64_t)K64 : 0;
  const unsigned n = (unsigned)a.n, E = (unsigned)a.E;
  for_wave_contigs(K, [&](int j, int lane) {
    int lo = a.out_ptr[j], hi = a.out_ptr[j + 1];
    if (lo < 0 || hi < lo || (int64_t)hi > a.P) lo = hi = 0;
    long long bases = 0;
    int wrong = 0;
    for (int q = lo + 1 + lane; q < hi; q += 64) {
      const unsigned e = (unsigned)a.out_edges[q];
      if (e < E) {
        bases += a.prefix_length[e];
        if (a.y && !(a.y[e] == 1.0f)) wrong += 1;
      }
    }
    bases = wave_sum(bases);
    wrong = wave_sum(wrong);
    if (lane == 0) {
      if (hi > lo) {
        const unsigned v = (unsigned)a.out_nodes[hi - 1];
        if (v < n) bases += a.read_length[v];
      }
      a.out_bases[j] = bases;
      a.out_wrong[j] = wrong;
    }
  });
}

}  // namespace gnm

using namespace gnm;

// ws: contig_of, pos_of (4 n each), taken, stamp (4 (n / 2 + 1)), rank, done, serial, kn, kp, noff, poff (4 C), run, rlen (4 P),
// two block-sum arrays, four 64-bit totals
struct ResLayout {
  size_t node[2], read[2], contig[7], pos[2], bsum[2], tot, bytes;
};
static ResLayout res_layout(int64_t C, int64_t P, int64_t n) {
  ResLayout l;
  size_t off = 0;
  for (int i = 0; i < 2; ++i) { l.node[i] = off; off += ws_pad((size_t)n * 4); }
  for (int i = 0; i < 2; ++i) { l.read[i] = off; off += ws_pad((size_t)(n / 2 + 1) * 4); }
  for (int i = 0; i < 7; ++i) { l.contig[i] = off; off += ws_pad((size_t)C * 4); }
  for (int i = 0; i < 2; ++i) { l.pos[i] = off; off += ws_pad((size_t)P * 4); }
  for (int i = 0; i < 2; ++i) { l.bsum[i] = off; off += scan_bsum_bytes<int32_t, 4>(C); }
  l.tot = off; off += ws_pad(kTotWords * 8);
  l.bytes = off;
  return l;
}

static bool res_sizes_ok(int64_t C, int64_t P, int64_t n) {
  return C >= 0 && P >= 0 && n >= 0 && C < INT32_MAX && P < INT32_MAX && n < INT32_MAX;
}

extern "C" size_t gnm_resolve_workspace_bytes(int64_t C, int64_t P, int64_t n) {
  if (!res_sizes_ok(C, P, n)) return 0;
  return res_layout(C, P, n).bytes;
}

// the checks the three entry points share, and the argument block over the workspace
static int res_args(const char* what, int64_t C, int64_t P, int64_t n, int64_t E, const int32_t* contig_ptr, const int32_t* walk_nodes,
                    const int32_t* walk_edges, const int32_t* order, int64_t len_threshold, void* record, void* ws, size_t ws_bytes,
                    ResArgs& a) {
  GNM_CHECK_ARG(res_sizes_ok(C, P, n) && E >= 0 && E < INT32_MAX,
                "%s: C = %lld, P = %lld, n = %lld, E = %lld: expected 0 <= C, P, n, E < 2^31 - 1 (32-bit positions and ids)", what,
                (long long)C, (long long)P, (long long)n, (long long)E);
  GNM_CHECK_ARG(len_threshold >= 1 && len_threshold < INT32_MAX, "%s: len_threshold = %lld: expected 1 <= len_threshold < 2^31 - 1",
                what, (long long)len_threshold);
  if (record_check(what, record, "gnm_resolve_record")) return -1;
  GNM_CHECK_ARG(contig_ptr, "%s: contig_ptr must not be null", what);
  GNM_CHECK_ARG(C == 0 || order, "%s: order must not be null when C > 0", what);
  GNM_CHECK_ARG(P == 0 || (walk_nodes && walk_edges), "%s: walk_nodes and walk_edges must not be null when P > 0", what);
  const ResLayout l = res_layout(C, P, n);
  if (ws_check(what, "gnm_resolve_workspace_bytes", ws, ws_bytes, l.bytes)) return -1;
  char* w = (char*)ws;
  a = ResArgs{};
  a.C = C; a.P = P; a.n = n; a.E = E; a.R = n / 2 + 1;
  a.thr = (int)len_threshold;
  a.contig_ptr = contig_ptr; a.walk_nodes = walk_nodes; a.walk_edges = walk_edges; a.order = order;
  a.contig_of = (int32_t*)(w + l.node[0]); a.pos_of = (int32_t*)(w + l.node[1]);
  a.taken = (int32_t*)(w + l.read[0]); a.stamp = (int32_t*)(w + l.read[1]);
  a.rank = (int32_t*)(w + l.contig[0]); a.done = (int32_t*)(w + l.contig[1]); a.serial = (int32_t*)(w + l.contig[2]);
  a.kn = (int32_t*)(w + l.contig[3]); a.kp = (int32_t*)(w + l.contig[4]); a.noff = (int32_t*)(w + l.contig[5]);
  a.poff = (int32_t*)(w + l.contig[6]);
  a.run = (int32_t*)(w + l.pos[0]); a.rlen = (int32_t*)(w + l.pos[1]);
  a.bsum[0] = (int32_t*)(w + l.bsum[0]); a.bsum[1] = (int32_t*)(w + l.bsum[1]);
  a.tot = (unsigned long long*)(w + l.tot);
  a.rec = (unsigned long long*)record;
  return 0;
}

static int res_wave_grid(int64_t items) { return persistent_grid(items, kWavesPerBlock, 8); }

extern "C" int gnm_resolve_prepare(int64_t C, int64_t P, int64_t n, int64_t E, const int32_t* contig_ptr, const int32_t* walk_nodes,
                                   const int32_t* walk_edges, const int32_t* order, int64_t len_threshold, void* record, void* ws,
                                   size_t ws_bytes, void* stream) {
  ResArgs a;
  if (res_args("resolve_prepare", C, P, n, E, contig_ptr, walk_nodes, walk_edges, order, len_threshold, record, ws, ws_bytes, a))
    return -1;
  hipStream_t st = (hipStream_t)stream;
  const int64_t items = (n > C ? n : C) > kTotWords ? (n > C ? n : C) : kTotWords;
  const dim3 blk(kBlock), wgrid(res_wave_grid(C > 0 ? C : 1));
  hipLaunchKernelGGL(res_init_k, dim3(persistent_grid(items, kBlock, 8)), blk, 0, st, a);
  if (C > 0) hipLaunchKernelGGL(res_scatter_k, wgrid, blk, 0, st, a);
  hipLaunchKernelGGL(res_flags_k, wgrid, blk, 0, st, a);
  GNM_LAUNCH_CHECK("resolve_prepare");
  return 0;
}

extern "C" int gnm_resolve_rounds(int64_t C, int64_t P, int64_t n, int64_t E, const int32_t* contig_ptr, const int32_t* walk_nodes,
                                  const int32_t* walk_edges, const int32_t* order, int64_t len_threshold, int64_t first_round,
                                  int64_t rounds, int64_t* undecided, void* record, void* ws, size_t ws_bytes, void* stream) {
  ResArgs a;
  if (res_args("resolve_rounds", C, P, n, E, contig_ptr, walk_nodes, walk_edges, order, len_threshold, record, ws, ws_bytes, a))
    return -1;
  GNM_CHECK_ARG(first_round >= 0 && rounds >= 0 && first_round < INT32_MAX - 1 && rounds < INT32_MAX - 1 &&
                    first_round + rounds < INT32_MAX - 1,
                "resolve_rounds: first_round = %lld, rounds = %lld: expected 0 <= first_round, rounds and their sum < 2^31 - 2",
                (long long)first_round, (long long)rounds);
  GNM_CHECK_ARG(rounds == 0 || (undecided && ((uintptr_t)undecided & 7) == 0),
                "resolve_rounds: undecided must be a non-null, 8-byte aligned int64 [rounds] array when rounds > 0");
  if (rounds == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kBlock), wgrid(res_wave_grid(C > 0 ? C : 1));
  hipLaunchKernelGGL(res_begin_k, dim3(persistent_grid(rounds, kBlock, 8)), blk, 0, st, a, (long long*)undecided, (int)rounds);
  if (C > 0)
    for (int64_t j = 0; j < rounds; ++j)                // round numbers start at 1: done == 0 is "done from the start"
      hipLaunchKernelGGL(res_round_k, wgrid, blk, 0, st, a, (int)(first_round + j + 1), (unsigned long long*)undecided + j);
  GNM_LAUNCH_CHECK("resolve_rounds");
  return 0;
}

extern "C" int gnm_resolve_layout(int64_t C, int64_t P, int64_t n, int64_t E, const int32_t* contig_ptr, const int32_t* walk_nodes,
                                  const int32_t* walk_edges, const int32_t* order, int64_t len_threshold, const int64_t* prefix_length,
                                  const int64_t* read_length, const float* y, void* record, int32_t* out_ptr, int32_t* out_nodes,
                                  int32_t* out_edges, int64_t* out_bases, int32_t* out_wrong, void* ws, size_t ws_bytes, void* stream) {
  ResArgs a;
  if (res_args("resolve_layout", C, P, n, E, contig_ptr, walk_nodes, walk_edges, order, len_threshold, record, ws, ws_bytes, a))
    return -1;
  GNM_CHECK_ARG(out_ptr, "resolve_layout: out_ptr must not be null");
  GNM_CHECK_ARG(P == 0 || (out_nodes && out_edges && out_bases && out_wrong),
                "resolve_layout: out_nodes, out_edges, out_bases and out_wrong must not be null when P > 0");
  GNM_CHECK_ARG(n == 0 || read_length, "resolve_layout: read_length must not be null when n > 0");
  GNM_CHECK_ARG(E == 0 || prefix_length, "resolve_layout: prefix_length must not be null when E > 0");
  a.prefix_length = prefix_length; a.read_length = read_length; a.y = y;
  a.out_ptr = out_ptr; a.out_nodes = out_nodes; a.out_edges = out_edges; a.out_bases = out_bases; a.out_wrong = out_wrong;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(kBlock), wgrid(res_wave_grid(C > 0 ? C : 1));
  if (C > 0) {
    scan_launch<int32_t, 4, 2>(ResScan{{}, a}, {C, {a.bsum[0], a.bsum[1]}, {a.noff, a.poff}}, st);
  }
  hipLaunchKernelGGL(res_gather_k, wgrid, blk, 0, st, a);                   // C == 0: out_ptr[0] = 0
  if (P > 0) hipLaunchKernelGGL(res_piece_k, dim3(res_wave_grid(P / a.thr + 1)), blk, 0, st, a);
  GNM_LAUNCH_CHECK("resolve_layout");
  return 0;
}
