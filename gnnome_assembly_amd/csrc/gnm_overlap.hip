// Overlap graph from the reads on the device (include/gnm.h, "overlap graph"): minimizer sketch -> seed hits -> chains.  The
// arithmetic is csrc/gnm_overlap.h; this file is the launches, the counters and the host twins.  Every stage is count / scan / emit:
// the count pass leaves one int64 per item in `off`, the three-phase scan of gnm_scan.h turns it into offsets IN PLACE (ovl_scan:
// its three launches with OvlScan as their user) and adds the total to one record word; the caller reads that word, sizes the
// outputs and calls the emit pass, which writes nothing at or past the size it was given.
//
// gnm_sketch_count / _emit: sk_ntiles_k (tiles of kSketchTile k-mer positions per read) + scan = the tile table; sk_tile_k, ONE
//   WORKGROUP PER TILE, grid-stride: thread 0 finds the tile's read by binary search in the table; kSketchWords threads unpack 32
//   bases each into LDS as three words (2-bit codes first-base-high, complemented codes first-base-low, invalid bits); every
//   thread forms hashes for the tile and its halo of w - 1 positions per side from two 64-bit LDS words and a shift each; then
//   every thread tests its own two consecutive positions (at most w - 1 comparisons per side, LDS only).  Count: the tile's sum.
//   Emit: the workgroup's exclusive scan of the per-thread counts places the entries, ordered by read and position.
//   LDS per workgroup: 3 word arrays + 638 hashes + 638 flags, about 6.3 KB.
// gnm_seed_pairs_count / _emit: one lane per sorted entry; it walks back over the earlier entries of its run (at most max_occ).
// gnm_seed_pairs_lower_hits, gnm_seed_pairs_count_range / _emit_range: the same lane per entry.  lower_hits: the entries of its run
//   with a larger read id, one 64-bit atomic per entry into lower_hits[its read].  _range: pair_k with two more compares per pair.
// gnm_chain_count / gnm_chain_pairs: head flags + scan = the group numbers; one lane per group head walks its group twice (its
//   end, then the sliding window): the longest group bounds the launch's time.
// Integer atomics on the record words, one per counter and workgroup, and on lower_hits (integer sums); no workgroup waits for another: outputs and record
// depend on the inputs alone, not on the grid.
#include <thread>
#include <vector>

#include "gnm_common.h"
#include "gnm_scan.h"
#include "gnm_overlap.h"

namespace gnm {

static_assert(kSketchTile == 2 * kBlock, "sk_tile_k: every thread owns two consecutive positions of the tile");
static_assert(kSketchWords <= kBlock, "sk_tile_k: one thread per word of bases");

// ---- the scan every stage shares: off[0 .. n) counts -> exclusive offsets in place, off[n] = the total ---------------------------
struct OvlScan : ScanUser<int64_t, 1> {
  unsigned long long* rec_word;          // the record word the total is added to, or null
  __device__ __forceinline__ void load(const Arrays& x, int64_t p, bool, int64_t (&v)[1][1]) const { v[0][0] = p < x.n ? x.out[0][p] : 0; }
  __device__ __forceinline__ void total(const Arrays& x, int, int64_t total) const {
    x.out[0][x.n] = total;
    if (rec_word && total > 0) atomicAdd(rec_word, (unsigned long long)total);
  }
};
__global__ void ovl_rec_add_k(unsigned long long* rec, int w0, unsigned long long v0, int w1, unsigned long long v1) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (v0) atomicAdd(rec + w0, v0);
    if (v1) atomicAdd(rec + w1, v1);
  }
}

static void ovl_scan(int64_t* off, int64_t n, int64_t* bsum, unsigned long long* rec_word, hipStream_t st) {
  scan_launch<int64_t, 1, 1>(OvlScan{{}, rec_word}, {n, {bsum}, {off}}, st);
}

// ---- stage 1 -------------------------------------------------------------------------------------------------------------------
struct SketchArgs {
  SeqStore s;
  int k, w;
  int64_t TB, M;                         // the bound on tiles the tables were sized for; emit: the entries the outputs hold
  int64_t *tile_ptr, *tile_off;          // [R + 1], [TB + 1]
  int64_t* hash;
  int32_t *read, *pos;
  uint8_t* strand;
  unsigned long long* rec;
};

__global__ __launch_bounds__(kBlock) void sk_ntiles_k(SketchArgs a) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.s.R; r += (int64_t)gridDim.x * kBlock)
    a.tile_ptr[r] = sk_read_tiles_(a.s, r, a.k);
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void sk_tile_k(SketchArgs a) {
  __shared__ uint64_t FW[kSketchWords], RC[kSketchWords], H[kSketchHashes];
  __shared__ uint32_t INV[kSketchWords];
  __shared__ uint8_t F[kSketchHashes];
  __shared__ int64_t which[2];
  __shared__ int64_t lds64[kWavesPerBlock];
  const int64_t tiles_all = a.tile_ptr[a.s.R];
  const int64_t tiles = tiles_all < a.TB ? tiles_all : a.TB;
  unsigned long long valid = 0ull;
  for (int64_t t = blockIdx.x; t < a.TB; t += gridDim.x) {    // t, tiles: the same in every thread
    if (t >= tiles) {
      if (!EMIT && threadIdx.x == 0) a.tile_off[t] = 0;
      continue;
    }
    if (threadIdx.x == 0) {
      const int64_t r = seq_find_(a.tile_ptr, 0, a.s.R - 1, t);   // the LAST read whose tiles start at or before t: it has one
      which[0] = r;
      which[1] = t - a.tile_ptr[r];
    }
    __syncthreads();
    const int64_t r = which[0];
    const SketchGeom g = sk_geom_(a.s, r, which[1], a.k, a.w);
    const int n = (int)(g.h1 - g.h0);                          // <= kSketchHashes
    const int nw = n > 0 ? (n + a.k - 1 + 31) / 32 + 1 : 0;    // <= kSketchWords
    if ((int)threadIdx.x < nw) {
      uint64_t fw, rc;
      uint32_t inv;
      sk_word_(a.s, g.first, g.len, g.h0 + 32 * (int64_t)threadIdx.x, fw, rc, inv);
      FW[threadIdx.x] = fw;
      RC[threadIdx.x] = rc;
      INV[threadIdx.x] = inv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kBlock) {
      uint64_t h;
      unsigned f;
      sk_hash_(FW, RC, INV, i, a.k, h, f);
      H[i] = h;
      F[i] = (uint8_t)f;
    }
    __syncthreads();
    const int own0 = (int)(g.p0 - g.h0), own1 = (int)(g.p1 - g.h0);
    const int i0 = own0 + 2 * (int)threadIdx.x;
    bool sel[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sel[u] = i0 + u < own1 && sk_selected_(H, F, i0 + u, n, g.W);
      if (!EMIT && i0 + u < own1) valid += F[i0 + u] & 1u;
    }
    const int64_t mine = (sel[0] ? 1 : 0) + (sel[1] ? 1 : 0);
    if (!EMIT) {
      const int64_t total = block_sum(mine, lds64);
      if (threadIdx.x == 0) a.tile_off[t] = total;
    } else {
      int64_t total;
      int64_t at = a.tile_off[t] + block_scan_excl(mine, lds64, total);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (sel[u] && at >= 0 && at < a.M) {
          a.hash[at] = (int64_t)H[i0 + u];
          a.read[at] = (int32_t)r;
          a.pos[at] = (int32_t)(g.h0 + i0 + u);
          a.strand[at] = (uint8_t)((F[i0 + u] >> 1) & 1u);
        }
        at += sel[u] ? 1 : 0;
      }
    }
    __syncthreads();                                           // the tile's LDS is rewritten by the next one
  }
  if (!EMIT) {
    __shared__ unsigned long long ldsu[kWavesPerBlock];
    block_count_add(valid, ldsu, a.rec + kOvlKmersValid);
  }
}

// One tile on the host: the selected entries appended to `out` (count only when null).
struct SketchEntry { int64_t hash; int32_t read, pos; uint8_t strand; };
static int64_t sketch_tile_host_(const SeqStore& s, int64_t r, int64_t ti, int k, int w, int64_t& valid, SketchEntry* out) {
  uint64_t FW[kSketchWords], RC[kSketchWords], H[kSketchHashes];
  uint32_t INV[kSketchWords];
  uint8_t F[kSketchHashes];
  const SketchGeom g = sk_geom_(s, r, ti, k, w);
  const int n = (int)(g.h1 - g.h0);
  const int nw = n > 0 ? (n + k - 1 + 31) / 32 + 1 : 0;
  for (int j = 0; j < nw; ++j) sk_word_(s, g.first, g.len, g.h0 + 32 * (int64_t)j, FW[j], RC[j], INV[j]);
  for (int i = 0; i < n; ++i) {
    unsigned f;
    sk_hash_(FW, RC, INV, i, k, H[i], f);
    F[i] = (uint8_t)f;
  }
  int64_t m = 0;
  for (int i = (int)(g.p0 - g.h0); i < (int)(g.p1 - g.h0); ++i) {
    valid += F[i] & 1;
    if (!sk_selected_(H, F, i, n, g.W)) continue;
    if (out) out[m] = {(int64_t)H[i], (int32_t)r, (int32_t)(g.h0 + i), (uint8_t)((F[i] >> 1) & 1)};
    ++m;
  }
  return m;
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------------------
struct PairArgs {
  int64_t M, R, N;                       // entries, reads, emit: the hits the outputs hold
  const int64_t* hash;
  const int32_t *read, *pos;
  const uint8_t* strand;
  const int64_t* length;
  int k, max_occ;
  int64_t* off;                          // [M + 1]
  int64_t* key;
  int32_t* diag;
  int64_t a_lo, a_hi;                    // RANGE: only the hits whose lower read id lies in [a_lo, a_hi)
  int64_t* lower;                        // [R]: pair_lower_k's output
};

struct PairCounts { unsigned long long runs, skipped_runs, skipped_entries, same_read, hits; };

// entry i: its hits counted (key == null) or written from slot `at` on; the counters of the count pass in c
template <bool RANGE = false>
GNM_SEQ_FN int64_t pair_entry_(const PairArgs& a, int64_t i, int64_t at, bool emit, PairCounts& c) {
  int back;
  bool skipped;
  ovl_run_(a.hash, a.M, i, a.max_occ, back, skipped);
  c.runs += back == 0 ? 1 : 0;
  c.skipped_runs += back == 0 && skipped ? 1 : 0;
  c.skipped_entries += skipped ? 1 : 0;
  if (skipped) return 0;
  int64_t m = 0;
  for (int64_t j = i - back; j < i; ++j) {
    if (a.read[j] == a.read[i]) {
      c.same_read += 1;
      continue;
    }
    if (RANGE && !ovl_in_range_(a.read[j], a.read[i], a.a_lo, a.a_hi)) continue;
    if (emit && at + m >= 0 && at + m < a.N) ovl_hit_(a.read, a.pos, a.strand, a.length, a.R, a.k, j, i, a.key[at + m], a.diag[at + m]);
    ++m;
  }
  return m;
}

// RANGE: the hits of a read range only (gnm_seed_pairs_count_range / _emit_range); its count pass adds nothing to the record.
template <bool EMIT, bool RANGE = false>
__global__ __launch_bounds__(kBlock) void pair_k(PairArgs a, unsigned long long* rec) {
  __shared__ unsigned long long lds[kWavesPerBlock];
  PairCounts c = {};
  const int64_t nb = (a.M + kBlock - 1) / kBlock;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * kBlock + threadIdx.x;
    if (i >= a.M) continue;                                // no shuffle or barrier inside the loop
    if (EMIT) pair_entry_<RANGE>(a, i, a.off[i], true, c);
    else a.off[i] = pair_entry_<RANGE>(a, i, 0, false, c);
  }
  if (!EMIT && !RANGE) {
    block_count_add(c.runs, lds, rec + kOvlRuns);
    block_count_add(c.skipped_runs, lds, rec + kOvlSkippedRuns);
    block_count_add(c.skipped_entries, lds, rec + kOvlSkippedEntries);
    block_count_add(c.same_read, lds, rec + kOvlSameRead);
  }
}

// entry i: its hits as the lower read (ovl_lower_) and what the count pass of the hits adds to the record for it
GNM_SEQ_FN int64_t lower_entry_(const PairArgs& a, int64_t i, PairCounts& c) {
  int back;
  bool skipped;
  int64_t same;
  const int64_t m = ovl_lower_(a.hash, a.read, a.M, i, a.max_occ, back, skipped, same);
  c.runs += back == 0 ? 1 : 0;
  c.skipped_runs += back == 0 && skipped ? 1 : 0;
  c.skipped_entries += skipped ? 1 : 0;
  c.same_read += (unsigned long long)same;
  c.hits += (unsigned long long)m;
  return m;
}

// gnm_seed_pairs_lower_hits: one lane per sorted entry, one 64-bit integer atomic per entry that is some hit's lower read (sums of
// integers: their order does not show).  An entry whose read id lies outside [0, R) adds to the record only.
__global__ __launch_bounds__(kBlock) void pair_lower_k(PairArgs a, unsigned long long* rec) {
  __shared__ unsigned long long lds[kWavesPerBlock];
  PairCounts c = {};
  const int64_t nb = (a.M + kBlock - 1) / kBlock;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * kBlock + threadIdx.x;
    if (i >= a.M) continue;
    const int64_t m = lower_entry_(a, i, c);
    const int64_t r = a.read[i];
    if (m > 0 && r >= 0 && r < a.R) atomicAdd((unsigned long long*)(a.lower + r), (unsigned long long)m);
  }
  block_count_add(c.runs, lds, rec + kOvlRuns);
  block_count_add(c.skipped_runs, lds, rec + kOvlSkippedRuns);
  block_count_add(c.skipped_entries, lds, rec + kOvlSkippedEntries);
  block_count_add(c.same_read, lds, rec + kOvlSameRead);
  block_count_add(c.hits, lds, rec + kOvlHits);
}

// ---- stage 3 -------------------------------------------------------------------------------------------------------------------
struct ChainArgs {
  int64_t N, R, G;                       // hits, reads, emit: the groups the outputs hold
  const int64_t* key;
  const int32_t* diag;
  const int64_t* length;
  int64_t band, min_hits, min_overlap;
  int64_t* off;                          // [N + 1]: the group number of every head
  int32_t *src, *dst;                    // [2 G]
  int64_t *prefix, *ovl;                 // [2 G]
  uint8_t *valid, *contained;            // [2 G], [R]
};

struct ChainCounts { unsigned long long few_hits, short_, contained, links; };

// the group headed by hit i (key[i - 1] != key[i]), number g: its two slots, the contained flag, the counters
GNM_SEQ_FN void chain_group_(const ChainArgs& a, int64_t i, int64_t g, ChainCounts& c) {
  const int64_t key = a.key[i];
  int64_t n = 1;
  while (i + n < a.N && a.key[i + n] == key) ++n;
  const int64_t ra = (int64_t)((uint64_t)key >> 32), rb = (int64_t)(((uint64_t)key & 0xffffffffull) >> 1);
  const bool known = ra < a.R && rb < a.R && ra < INT32_MAX / 2 && rb < INT32_MAX / 2;   // a key of gnm_seed_pairs always is
  ChainOut o = {};
  if (known) o = ovl_chain_(a.diag, i, n, a.band, a.min_hits, a.min_overlap, ra, rb, (int)(key & 1), a.length[ra], a.length[rb]);
  const bool link = o.kind == kChainForward || o.kind == kChainBackward;
  c.few_hits += o.kind == kChainFewHits ? 1 : 0;
  c.short_ += o.kind == kChainShort ? 1 : 0;
  c.contained += o.kind == kChainContained ? 1 : 0;
  c.links += link ? 1 : 0;
  if (o.kind == kChainContained) a.contained[o.contained] = 1;   // the same value from every writer
  if (g < 0 || g >= a.G) return;
  a.src[2 * g] = link ? o.src0 : -1;
  a.dst[2 * g] = link ? o.dst0 : -1;
  a.src[2 * g + 1] = link ? o.src1 : -1;
  a.dst[2 * g + 1] = link ? o.dst1 : -1;
  a.prefix[2 * g] = link ? o.prefix0 : 0;
  a.prefix[2 * g + 1] = link ? o.prefix1 : 0;
  a.ovl[2 * g] = a.ovl[2 * g + 1] = link ? o.ov : 0;
  a.valid[2 * g] = a.valid[2 * g + 1] = link ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void chain_head_k(ChainArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.N; i += (int64_t)gridDim.x * kBlock)
    a.off[i] = i == 0 || a.key[i - 1] != a.key[i] ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void chain_emit_k(ChainArgs a, unsigned long long* rec) {
  __shared__ unsigned long long lds[kWavesPerBlock];
  ChainCounts c = {};
  const int64_t nb = (a.N + kBlock - 1) / kBlock;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t i = b * kBlock + threadIdx.x;
    if (i >= a.N || !(i == 0 || a.key[i - 1] != a.key[i])) continue;
    chain_group_(a, i, a.off[i], c);
  }
  block_count_add(c.few_hits, lds, rec + kOvlFewHits);
  block_count_add(c.short_, lds, rec + kOvlShort);
  block_count_add(c.contained, lds, rec + kOvlContainedGroups);
  block_count_add(c.links, lds, rec + kOvlLinks);
}

// fn(t, i0, i1) over contiguous ranges of [0, n) on up to `threads` host threads
template <class Fn>
static void host_ranges_(int64_t n, int threads, Fn fn) {
  const int nt = n < 1 ? 1 : ((int64_t)threads < n ? threads : (int)n);
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(fn, t, n * t / nt, n * (t + 1) / nt);
  fn(0, (int64_t)0, n / nt);
  for (auto& th : pool) th.join();
}

}  // namespace gnm

using namespace gnm;

static_assert(kSketchTile == GNM_SKETCH_TILE, "include/gnm.h states the tile size");
static_assert(kOvlWords * 8 == sizeof(gnm_overlap_record), "include/gnm.h lists the record's words");

static int threads_check(const char* what, int threads) {
  GNM_CHECK_ARG(threads >= 1 && threads <= 1024, "%s: threads = %d: expected 1 <= threads <= 1024", what, threads);
  return 0;
}

extern "C" size_t gnm_overlap_scan_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return ws_pad((size_t)(scan_blocks<1>(n) + 1) * 8);
}

extern "C" int64_t gnm_sketch_tile_bound(int64_t R, int64_t packed_bytes) {
  if (R < 0 || packed_bytes < 0 || packed_bytes > (INT64_MAX >> 2)) return -1;
  return packed_bytes * 2 / kSketchTile + R;               // a read of L bases has at most L / tile + 1 tiles
}

static int sketch_check(const char* what, const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length,
                        int64_t R, int k, int w) {
  GNM_CHECK_ARG(k >= kSketchMinK && k <= kSketchMaxK, "%s: k = %d: expected %d <= k <= %d", what, k, kSketchMinK, kSketchMaxK);
  GNM_CHECK_ARG(w >= 1 && w <= kSketchMaxW, "%s: w = %d: expected 1 <= w <= %d", what, w, kSketchMaxW);
  GNM_CHECK_ARG(R < INT32_MAX / 2, "%s: R = %lld: expected 2 R node ids below 2^31 - 1", what, (long long)R);
  if (seq_store_check(what, 2 * R, R, base_off, length, packed_bytes)) return -1;
  GNM_CHECK_ARG(packed_bytes == 0 || (packed && ((uintptr_t)packed & 3) == 0), "%s: packed must be non-null and 4-byte aligned", what);
  return 0;
}

static SeqStore store_of(const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R) {
  SeqStore s = {};
  s.packed = packed; s.base_off = base_off; s.length = length; s.nibbles = packed_bytes * 2; s.R = R; s.n = 2 * R;
  return s;
}

extern "C" int gnm_sketch_count(const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R,
                                int k, int w, int64_t* tile_ptr, int64_t* tile_off, int64_t tile_bound, void* record, void* ws,
                                size_t ws_bytes, void* stream) {
  if (sketch_check("sketch_count", packed, packed_bytes, base_off, length, R, k, w)) return -1;
  if (record_check("sketch_count", record, "gnm_overlap_record")) return -1;
  GNM_CHECK_ARG(tile_bound == gnm_sketch_tile_bound(R, packed_bytes), "sketch_count: tile_bound = %lld: expected gnm_sketch_tile_bound",
                (long long)tile_bound);
  GNM_CHECK_ARG(tile_ptr && tile_off, "sketch_count: tile_ptr and tile_off must not be null");
  const size_t need = gnm_overlap_scan_workspace_bytes(R > tile_bound ? R : tile_bound);
  if (ws_check("sketch_count", "gnm_overlap_scan_workspace_bytes", ws, ws_bytes, need)) return -1;
  hipStream_t st = (hipStream_t)stream;
  SketchArgs a = {};
  a.s = store_of(packed, packed_bytes, base_off, length, R);
  a.k = k; a.w = w; a.TB = tile_bound; a.tile_ptr = tile_ptr; a.tile_off = tile_off; a.rec = (unsigned long long*)record;
  const dim3 blk(kBlock);
  if (R > 0) hipLaunchKernelGGL(sk_ntiles_k, dim3(persistent_grid(R, kBlock, 8)), blk, 0, st, a);
  ovl_scan(tile_ptr, R, (int64_t*)ws, nullptr, st);
  if (tile_bound > 0) hipLaunchKernelGGL(sk_tile_k<false>, dim3(persistent_grid(tile_bound, 1, 8)), blk, 0, st, a);
  ovl_scan(tile_off, tile_bound, (int64_t*)ws, a.rec + kOvlMinimizers, st);
  hipLaunchKernelGGL(ovl_rec_add_k, dim3(1), dim3(64), 0, st, a.rec, (int)kOvlReads, (unsigned long long)R, (int)kOvlCalls, 1ull);
  GNM_LAUNCH_CHECK("sketch_count");
  return 0;
}

extern "C" int gnm_sketch_emit(const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R,
                               int k, int w, const int64_t* tile_ptr, const int64_t* tile_off, int64_t tile_bound, int64_t M,
                               int64_t* hash, int32_t* read, int32_t* pos, uint8_t* strand, void* stream) {
  if (sketch_check("sketch_emit", packed, packed_bytes, base_off, length, R, k, w)) return -1;
  GNM_CHECK_ARG(tile_bound == gnm_sketch_tile_bound(R, packed_bytes) && M >= 0,
                "sketch_emit: tile_bound = %lld, M = %lld: expected gnm_sketch_tile_bound and M >= 0", (long long)tile_bound, (long long)M);
  if (M == 0 || tile_bound == 0) return 0;
  GNM_CHECK_ARG(tile_ptr && tile_off && hash && read && pos && strand, "sketch_emit: the tables and outputs must not be null when M > 0");
  SketchArgs a = {};
  a.s = store_of(packed, packed_bytes, base_off, length, R);
  a.k = k; a.w = w; a.TB = tile_bound; a.M = M;
  a.tile_ptr = const_cast<int64_t*>(tile_ptr); a.tile_off = const_cast<int64_t*>(tile_off);
  a.hash = hash; a.read = read; a.pos = pos; a.strand = strand;
  hipLaunchKernelGGL(sk_tile_k<true>, dim3(persistent_grid(tile_bound, 1, 8)), dim3(kBlock), 0, (hipStream_t)stream, a);
  GNM_LAUNCH_CHECK("sketch_emit");
  return 0;
}

extern "C" int gnm_sketch_host(const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R,
                               int k, int w, int64_t capacity, int64_t* hash, int32_t* read, int32_t* pos, uint8_t* strand,
                               int64_t* total, void* record, int threads) {
  if (sketch_check("sketch_host", packed, packed_bytes, base_off, length, R, k, w)) return -1;
  if (record_check("sketch_host", record, "gnm_overlap_record") || threads_check("sketch_host", threads)) return -1;
  GNM_CHECK_ARG(total, "sketch_host: total must not be null");
  for (int64_t r = 0; r < R; ++r)
    GNM_CHECK_ARG(length[r] < INT32_MAX, "sketch_host: read %lld has %lld bases: expected fewer than 2^31 - 1", (long long)r,
                  (long long)length[r]);
  const SeqStore s = store_of(packed, packed_bytes, base_off, length, R);
  std::vector<int64_t> tr, tt;                               // the tile table: read and tile-in-read of every tile
  for (int64_t r = 0; r < R; ++r)
    for (int64_t ti = 0, n = sk_read_tiles_(s, r, k); ti < n; ++ti) {
      tr.push_back(r);
      tt.push_back(ti);
    }
  const int64_t T = (int64_t)tr.size();
  std::vector<int64_t> off((size_t)T + 1, 0), valid((size_t)threads, 0);
  host_ranges_(T, threads, [&](int t, int64_t t0, int64_t t1) {
    for (int64_t x = t0; x < t1; ++x) off[(size_t)x] = sketch_tile_host_(s, tr[(size_t)x], tt[(size_t)x], k, w, valid[(size_t)t], nullptr);
  });
  int64_t run = 0;
  for (int64_t x = 0; x <= T; ++x) {
    const int64_t v = off[(size_t)x];
    off[(size_t)x] = run;
    run += x < T ? v : 0;
  }
  *total = run;
  if (capacity < 0) return 0;                              // the size only: the record stays as it is
  GNM_CHECK_ARG(capacity >= run && (run == 0 || (hash && read && pos && strand)),
                "sketch_host: %lld entries need room, capacity = %lld (or an output is null)", (long long)run, (long long)capacity);
  host_ranges_(T, threads, [&](int, int64_t t0, int64_t t1) {
    std::vector<SketchEntry> buf(kSketchTile);
    for (int64_t x = t0; x < t1; ++x) {
      int64_t dummy = 0;
      const int64_t m = sketch_tile_host_(s, tr[(size_t)x], tt[(size_t)x], k, w, dummy, buf.data());
      for (int64_t e = 0; e < m; ++e) {
        const int64_t at = off[(size_t)x] + e;
        hash[at] = buf[(size_t)e].hash; read[at] = buf[(size_t)e].read; pos[at] = buf[(size_t)e].pos; strand[at] = buf[(size_t)e].strand;
      }
    }
  });
  int64_t* rec = (int64_t*)record;
  for (int64_t v : valid) rec[kOvlKmersValid] += v;
  rec[kOvlReads] += R;
  rec[kOvlMinimizers] += run;
  rec[kOvlCalls] += 1;
  return 0;
}

static int pairs_check(const char* what, int64_t M, const int64_t* hash, const int32_t* read, int max_occ) {
  GNM_CHECK_ARG(M >= 0 && M < INT32_MAX, "%s: M = %lld: expected 0 <= M < 2^31 - 1", what, (long long)M);
  GNM_CHECK_ARG(max_occ >= 1 && max_occ <= kOverlapMaxOcc, "%s: max_occ = %d: expected 1 <= max_occ <= %d", what, max_occ, kOverlapMaxOcc);
  GNM_CHECK_ARG(M == 0 || (hash && read), "%s: hash and read must not be null when M > 0", what);
  return 0;
}

static int pairs_emit_check(const char* what, int64_t M, const int32_t* pos, const uint8_t* strand, const int64_t* length, int64_t R, int k) {
  GNM_CHECK_ARG(R >= 0 && R < INT32_MAX && k >= kSketchMinK && k <= kSketchMaxK, "%s: R = %lld, k = %d: expected 0 <= R < 2^31 - 1, %d <= k <= %d",
                what, (long long)R, k, kSketchMinK, kSketchMaxK);
  GNM_CHECK_ARG(M == 0 || (pos && strand), "%s: pos and strand must not be null when M > 0", what);
  GNM_CHECK_ARG(R == 0 || length, "%s: length must not be null when R > 0", what);
  return 0;
}

extern "C" int gnm_seed_pairs_count(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t* off, void* record,
                                    void* ws, size_t ws_bytes, void* stream) {
  if (pairs_check("seed_pairs_count", M, hash, read, max_occ) || record_check("seed_pairs_count", record, "gnm_overlap_record")) return -1;
  GNM_CHECK_ARG(off, "seed_pairs_count: off must not be null");
  if (ws_check("seed_pairs_count", "gnm_overlap_scan_workspace_bytes", ws, ws_bytes, gnm_overlap_scan_workspace_bytes(M))) return -1;
  hipStream_t st = (hipStream_t)stream;
  PairArgs a = {};
  a.M = M; a.hash = hash; a.read = read; a.max_occ = max_occ; a.off = off;
  unsigned long long* rec = (unsigned long long*)record;
  if (M > 0) hipLaunchKernelGGL(pair_k<false>, dim3(persistent_grid((M + kBlock - 1) / kBlock, 1, 8)), dim3(kBlock), 0, st, a, rec);
  ovl_scan(off, M, (int64_t*)ws, rec + kOvlHits, st);
  GNM_LAUNCH_CHECK("seed_pairs_count");
  return 0;
}

extern "C" int gnm_seed_pairs_emit(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                                   const int64_t* length, int64_t R, int k, int max_occ, const int64_t* off, int64_t N, int64_t* key,
                                   int32_t* diag, void* stream) {
  if (pairs_check("seed_pairs_emit", M, hash, read, max_occ) || pairs_emit_check("seed_pairs_emit", M, pos, strand, length, R, k)) return -1;
  GNM_CHECK_ARG(N >= 0, "seed_pairs_emit: N = %lld: expected >= 0", (long long)N);
  if (M == 0 || N == 0) return 0;
  GNM_CHECK_ARG(off && key && diag, "seed_pairs_emit: off, key and diag must not be null when there are hits");
  PairArgs a = {};
  a.M = M; a.R = R; a.N = N; a.hash = hash; a.read = read; a.pos = pos; a.strand = strand; a.length = length; a.k = k;
  a.max_occ = max_occ; a.off = const_cast<int64_t*>(off); a.key = key; a.diag = diag;
  hipLaunchKernelGGL(pair_k<true>, dim3(persistent_grid((M + kBlock - 1) / kBlock, 1, 8)), dim3(kBlock), 0, (hipStream_t)stream, a,
                     (unsigned long long*)nullptr);
  GNM_LAUNCH_CHECK("seed_pairs_emit");
  return 0;
}

extern "C" int gnm_seed_pairs_host(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                                   const int64_t* length, int64_t R, int k, int max_occ, int64_t capacity, int64_t* key, int32_t* diag,
                                   int64_t* total, void* record, int threads) {
  if (pairs_check("seed_pairs_host", M, hash, read, max_occ) || pairs_emit_check("seed_pairs_host", M, pos, strand, length, R, k)) return -1;
  if (record_check("seed_pairs_host", record, "gnm_overlap_record") || threads_check("seed_pairs_host", threads)) return -1;
  GNM_CHECK_ARG(total, "seed_pairs_host: total must not be null");
  PairArgs a = {};
  a.M = M; a.R = R; a.hash = hash; a.read = read; a.pos = pos; a.strand = strand; a.length = length; a.k = k; a.max_occ = max_occ;
  std::vector<int64_t> off((size_t)M + 1, 0);
  std::vector<PairCounts> cs((size_t)threads, PairCounts{});
  host_ranges_(M, threads, [&](int t, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) off[(size_t)i] = pair_entry_(a, i, 0, false, cs[(size_t)t]);
  });
  int64_t run = 0;
  for (int64_t i = 0; i <= M; ++i) {
    const int64_t v = off[(size_t)i];
    off[(size_t)i] = run;
    run += i < M ? v : 0;
  }
  *total = run;
  if (capacity < 0) return 0;
  GNM_CHECK_ARG(capacity >= run && (run == 0 || (key && diag)), "seed_pairs_host: %lld hits need room, capacity = %lld (or an output is null)",
                (long long)run, (long long)capacity);
  a.N = run; a.key = key; a.diag = diag;
  host_ranges_(M, threads, [&](int, int64_t i0, int64_t i1) {
    PairCounts unused = {};
    for (int64_t i = i0; i < i1; ++i) pair_entry_(a, i, off[(size_t)i], true, unused);
  });
  int64_t* rec = (int64_t*)record;
  for (const PairCounts& c : cs) {
    rec[kOvlRuns] += (int64_t)c.runs; rec[kOvlSkippedRuns] += (int64_t)c.skipped_runs;
    rec[kOvlSkippedEntries] += (int64_t)c.skipped_entries; rec[kOvlSameRead] += (int64_t)c.same_read;
  }
  rec[kOvlHits] += run;
  return 0;
}

// ---- stage 2 in read-range chunks: the plan (hits per lower read) and the hits of one range of lower reads ----------------------
static int lower_check(const char* what, const int64_t* lower_hits, int64_t R) {
  GNM_CHECK_ARG(R >= 0 && R < INT32_MAX, "%s: R = %lld: expected 0 <= R < 2^31 - 1", what, (long long)R);
  GNM_CHECK_ARG(R == 0 || (lower_hits && ((uintptr_t)lower_hits & 7) == 0), "%s: lower_hits must be non-null and 8-byte aligned when R > 0",
                what);
  return 0;
}

static int range_check(const char* what, int64_t a_lo, int64_t a_hi, int64_t R) {
  GNM_CHECK_ARG(0 <= a_lo && a_lo <= a_hi && a_hi <= R, "%s: a_lo = %lld, a_hi = %lld: expected 0 <= a_lo <= a_hi <= R = %lld", what,
                (long long)a_lo, (long long)a_hi, (long long)R);
  return 0;
}

extern "C" int gnm_seed_pairs_lower_hits(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t* lower_hits, int64_t R,
                                         void* record, void* ws, size_t ws_bytes, void* stream) {
  if (pairs_check("seed_pairs_lower_hits", M, hash, read, max_occ) || lower_check("seed_pairs_lower_hits", lower_hits, R)) return -1;
  if (record_check("seed_pairs_lower_hits", record, "gnm_overlap_record")) return -1;
  (void)ws;                                                // no scan: the counts are summed where they belong
  (void)ws_bytes;
  if (M == 0) return 0;
  PairArgs a = {};
  a.M = M; a.R = R; a.hash = hash; a.read = read; a.max_occ = max_occ; a.lower = lower_hits;
  hipLaunchKernelGGL(pair_lower_k, dim3(persistent_grid((M + kBlock - 1) / kBlock, 1, 8)), dim3(kBlock), 0, (hipStream_t)stream, a,
                     (unsigned long long*)record);
  GNM_LAUNCH_CHECK("seed_pairs_lower_hits");
  return 0;
}

extern "C" int gnm_seed_pairs_lower_hits_host(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t* lower_hits,
                                              int64_t R, void* record, int threads) {
  if (pairs_check("seed_pairs_lower_hits_host", M, hash, read, max_occ) || lower_check("seed_pairs_lower_hits_host", lower_hits, R)) return -1;
  if (record_check("seed_pairs_lower_hits_host", record, "gnm_overlap_record") || threads_check("seed_pairs_lower_hits_host", threads)) return -1;
  PairArgs a = {};
  a.M = M; a.R = R; a.hash = hash; a.read = read; a.max_occ = max_occ;
  std::vector<int64_t> mine((size_t)M, 0);
  std::vector<PairCounts> cs((size_t)threads, PairCounts{});
  host_ranges_(M, threads, [&](int t, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) mine[(size_t)i] = lower_entry_(a, i, cs[(size_t)t]);
  });
  for (int64_t i = 0; i < M; ++i)
    if (read[i] >= 0 && read[i] < R) lower_hits[read[i]] += mine[(size_t)i];
  int64_t* rec = (int64_t*)record;
  for (const PairCounts& c : cs) {
    rec[kOvlRuns] += (int64_t)c.runs; rec[kOvlSkippedRuns] += (int64_t)c.skipped_runs;
    rec[kOvlSkippedEntries] += (int64_t)c.skipped_entries; rec[kOvlSameRead] += (int64_t)c.same_read;
    rec[kOvlHits] += (int64_t)c.hits;
  }
  return 0;
}

extern "C" int gnm_seed_pairs_count_range(int64_t M, const int64_t* hash, const int32_t* read, int max_occ, int64_t a_lo, int64_t a_hi,
                                          int64_t R, int64_t* off, void* record, void* ws, size_t ws_bytes, void* stream) {
  if (pairs_check("seed_pairs_count_range", M, hash, read, max_occ)) return -1;
  GNM_CHECK_ARG(R >= 0 && R < INT32_MAX, "seed_pairs_count_range: R = %lld: expected 0 <= R < 2^31 - 1", (long long)R);
  if (range_check("seed_pairs_count_range", a_lo, a_hi, R) || record_check("seed_pairs_count_range", record, "gnm_overlap_record")) return -1;
  GNM_CHECK_ARG(off, "seed_pairs_count_range: off must not be null");
  if (ws_check("seed_pairs_count_range", "gnm_overlap_scan_workspace_bytes", ws, ws_bytes, gnm_overlap_scan_workspace_bytes(M))) return -1;
  hipStream_t st = (hipStream_t)stream;
  PairArgs a = {};
  a.M = M; a.R = R; a.hash = hash; a.read = read; a.max_occ = max_occ; a.off = off; a.a_lo = a_lo; a.a_hi = a_hi;
  if (M > 0)
    hipLaunchKernelGGL((pair_k<false, true>), dim3(persistent_grid((M + kBlock - 1) / kBlock, 1, 8)), dim3(kBlock), 0, st, a,
                       (unsigned long long*)nullptr);
  ovl_scan(off, M, (int64_t*)ws, nullptr, st);             // the record stays as it is: the planning call added the totals
  GNM_LAUNCH_CHECK("seed_pairs_count_range");
  return 0;
}

extern "C" int gnm_seed_pairs_emit_range(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                                         const int64_t* length, int64_t R, int k, int max_occ, int64_t a_lo, int64_t a_hi,
                                         const int64_t* off, int64_t N, int64_t* key, int32_t* diag, void* stream) {
  if (pairs_check("seed_pairs_emit_range", M, hash, read, max_occ) || pairs_emit_check("seed_pairs_emit_range", M, pos, strand, length, R, k))
    return -1;
  if (range_check("seed_pairs_emit_range", a_lo, a_hi, R)) return -1;
  GNM_CHECK_ARG(N >= 0, "seed_pairs_emit_range: N = %lld: expected >= 0", (long long)N);
  if (M == 0 || N == 0) return 0;
  GNM_CHECK_ARG(off && key && diag, "seed_pairs_emit_range: off, key and diag must not be null when there are hits");
  PairArgs a = {};
  a.M = M; a.R = R; a.N = N; a.hash = hash; a.read = read; a.pos = pos; a.strand = strand; a.length = length; a.k = k;
  a.max_occ = max_occ; a.off = const_cast<int64_t*>(off); a.key = key; a.diag = diag; a.a_lo = a_lo; a.a_hi = a_hi;
  hipLaunchKernelGGL((pair_k<true, true>), dim3(persistent_grid((M + kBlock - 1) / kBlock, 1, 8)), dim3(kBlock), 0, (hipStream_t)stream, a,
                     (unsigned long long*)nullptr);
  GNM_LAUNCH_CHECK("seed_pairs_emit_range");
  return 0;
}

extern "C" int gnm_seed_pairs_range_host(int64_t M, const int64_t* hash, const int32_t* read, const int32_t* pos, const uint8_t* strand,
                                         const int64_t* length, int64_t R, int k, int max_occ, int64_t a_lo, int64_t a_hi,
                                         int64_t capacity, int64_t* key, int32_t* diag, int64_t* total, void* record, int threads) {
  if (pairs_check("seed_pairs_range_host", M, hash, read, max_occ) || pairs_emit_check("seed_pairs_range_host", M, pos, strand, length, R, k))
    return -1;
  if (range_check("seed_pairs_range_host", a_lo, a_hi, R)) return -1;
  if (record_check("seed_pairs_range_host", record, "gnm_overlap_record") || threads_check("seed_pairs_range_host", threads)) return -1;
  GNM_CHECK_ARG(total, "seed_pairs_range_host: total must not be null");
  PairArgs a = {};
  a.M = M; a.R = R; a.hash = hash; a.read = read; a.pos = pos; a.strand = strand; a.length = length; a.k = k; a.max_occ = max_occ;
  a.a_lo = a_lo; a.a_hi = a_hi;
  std::vector<int64_t> off((size_t)M + 1, 0);
  host_ranges_(M, threads, [&](int, int64_t i0, int64_t i1) {
    PairCounts unused = {};
    for (int64_t i = i0; i < i1; ++i) off[(size_t)i] = pair_entry_<true>(a, i, 0, false, unused);
  });
  int64_t run = 0;
  for (int64_t i = 0; i <= M; ++i) {
    const int64_t v = off[(size_t)i];
    off[(size_t)i] = run;
    run += i < M ? v : 0;
  }
  *total = run;
  if (capacity < 0) return 0;
  GNM_CHECK_ARG(capacity >= run && (run == 0 || (key && diag)), "seed_pairs_range_host: %lld hits need room, capacity = %lld (or an output is null)",
                (long long)run, (long long)capacity);
  a.N = run; a.key = key; a.diag = diag;
  host_ranges_(M, threads, [&](int, int64_t i0, int64_t i1) {
    PairCounts unused = {};
    for (int64_t i = i0; i < i1; ++i) pair_entry_<true>(a, i, off[(size_t)i], true, unused);
  });
  return 0;                                                // the record stays as it is, as after the device calls
}

static int chain_check(const char* what, int64_t N, const int64_t* key, const int32_t* diag, const int64_t* length, int64_t R, int64_t band,
                       int64_t min_hits, int64_t min_overlap) {
  GNM_CHECK_ARG(N >= 0 && N < INT32_MAX && R >= 0 && R < INT32_MAX / 2, "%s: N = %lld, R = %lld: expected 0 <= N < 2^31 - 1, 0 <= R < 2^30 - 1",
                what, (long long)N, (long long)R);
  GNM_CHECK_ARG(band >= 0 && band < INT32_MAX && min_hits >= 1 && min_hits < INT32_MAX && min_overlap >= 0,
                "%s: band = %lld, min_hits = %lld, min_overlap = %lld: expected 0 <= band < 2^31 - 1, 1 <= min_hits < 2^31 - 1, min_overlap >= 0",
                what, (long long)band, (long long)min_hits, (long long)min_overlap);
  GNM_CHECK_ARG(N == 0 || (key && diag), "%s: key and diag must not be null when N > 0", what);
  GNM_CHECK_ARG(R == 0 || length, "%s: length must not be null when R > 0", what);
  return 0;
}

extern "C" int gnm_chain_count(int64_t N, const int64_t* key, int64_t* off, void* record, void* ws, size_t ws_bytes, void* stream) {
  GNM_CHECK_ARG(N >= 0 && N < INT32_MAX, "chain_count: N = %lld: expected 0 <= N < 2^31 - 1", (long long)N);
  if (record_check("chain_count", record, "gnm_overlap_record")) return -1;
  GNM_CHECK_ARG(off && (N == 0 || key), "chain_count: off, and key when N > 0, must not be null");
  if (ws_check("chain_count", "gnm_overlap_scan_workspace_bytes", ws, ws_bytes, gnm_overlap_scan_workspace_bytes(N))) return -1;
  hipStream_t st = (hipStream_t)stream;
  ChainArgs a = {};
  a.N = N; a.key = key; a.off = off;
  if (N > 0) hipLaunchKernelGGL(chain_head_k, dim3(persistent_grid(N, kBlock, 8)), dim3(kBlock), 0, st, a);
  ovl_scan(off, N, (int64_t*)ws, (unsigned long long*)record + kOvlGroups, st);
  GNM_LAUNCH_CHECK("chain_count");
  return 0;
}

extern "C" int gnm_chain_pairs(int64_t N, const int64_t* key, const int32_t* diag, const int64_t* off, int64_t G, const int64_t* length,
                               int64_t R, int64_t band, int64_t min_hits, int64_t min_overlap, int32_t* src, int32_t* dst,
                               int64_t* prefix_length, int64_t* overlap_length, uint8_t* valid, uint8_t* contained, void* record,
                               void* stream) {
  if (chain_check("chain_pairs", N, key, diag, length, R, band, min_hits, min_overlap)) return -1;
  if (record_check("chain_pairs", record, "gnm_overlap_record")) return -1;
  GNM_CHECK_ARG(G >= 0 && G <= N, "chain_pairs: G = %lld: expected 0 <= G <= N", (long long)G);
  if (N == 0) return 0;
  GNM_CHECK_ARG(off && contained && (G == 0 || (src && dst && prefix_length && overlap_length && valid)),
                "chain_pairs: off, contained and the outputs of G groups must not be null");
  ChainArgs a = {};
  a.N = N; a.R = R; a.G = G; a.key = key; a.diag = diag; a.length = length; a.band = band; a.min_hits = min_hits;
  a.min_overlap = min_overlap; a.off = const_cast<int64_t*>(off); a.src = src; a.dst = dst; a.prefix = prefix_length;
  a.ovl = overlap_length; a.valid = valid; a.contained = contained;
  hipLaunchKernelGGL(chain_emit_k, dim3(persistent_grid((N + kBlock - 1) / kBlock, 1, 8)), dim3(kBlock), 0, (hipStream_t)stream, a,
                     (unsigned long long*)record);
  GNM_LAUNCH_CHECK("chain_pairs");
  return 0;
}

extern "C" int gnm_chain_pairs_host(int64_t N, const int64_t* key, const int32_t* diag, const int64_t* length, int64_t R, int64_t band,
                                    int64_t min_hits, int64_t min_overlap, int64_t capacity, int32_t* src, int32_t* dst,
                                    int64_t* prefix_length, int64_t* overlap_length, uint8_t* valid, uint8_t* contained, int64_t* total,
                                    void* record, int threads) {
  if (chain_check("chain_pairs_host", N, key, diag, length, R, band, min_hits, min_overlap)) return -1;
  if (record_check("chain_pairs_host", record, "gnm_overlap_record") || threads_check("chain_pairs_host", threads)) return -1;
  GNM_CHECK_ARG(total, "chain_pairs_host: total must not be null");
  std::vector<int64_t> off((size_t)N + 1, 0);
  int64_t G = 0;
  for (int64_t i = 0; i < N; ++i) {
    off[(size_t)i] = G;
    G += i == 0 || key[i - 1] != key[i] ? 1 : 0;
  }
  *total = G;
  if (capacity < 0) return 0;
  GNM_CHECK_ARG(capacity >= G && (G == 0 || (src && dst && prefix_length && overlap_length && valid)) && (N == 0 || R == 0 || contained),
                "chain_pairs_host: %lld groups need room, capacity = %lld (or an output is null)", (long long)G, (long long)capacity);
  ChainArgs a = {};
  a.N = N; a.R = R; a.G = G; a.key = key; a.diag = diag; a.length = length; a.band = band; a.min_hits = min_hits;
  a.min_overlap = min_overlap; a.src = src; a.dst = dst; a.prefix = prefix_length; a.ovl = overlap_length; a.valid = valid;
  a.contained = contained;
  std::vector<ChainCounts> cs((size_t)threads, ChainCounts{});
  host_ranges_(N, threads, [&](int t, int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i)
      if (i == 0 || key[i - 1] != key[i]) chain_group_(a, i, off[(size_t)i], cs[(size_t)t]);
  });
  int64_t* rec = (int64_t*)record;
  for (const ChainCounts& c : cs) {
    rec[kOvlFewHits] += (int64_t)c.few_hits; rec[kOvlShort] += (int64_t)c.short_;
    rec[kOvlContainedGroups] += (int64_t)c.contained; rec[kOvlLinks] += (int64_t)c.links;
  }
  rec[kOvlGroups] += G;
  return 0;
}
