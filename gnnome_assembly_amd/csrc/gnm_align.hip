// Overlap identity on the device (include/gnm.h, "overlap alignment"): for every edge the banded edit distance between the suffix
// of the source read and the start of the destination read, from the packed read store.  The per-edge arithmetic is
// csrc/gnm_align.h; this file is the launch, the counters and the host twin.
//
// gnm_overlap_align, one launch: ONE LANE PER EDGE, no LDS in the alignment, no traffic between lanes.  A workgroup takes blocks
// of kBlock consecutive edge ids, grid-stride.  The kernel is instantiated per word count of the band (1, 2, 4, 8 words of 64
// diagonals: K <= 31, 63, 127, 255); the band's vectors and the window over the target are register arrays indexed by unrolled
// loops only.  The column loop of an edge runs m = la - p times, m known (and checked against the store) before it starts; a lane
// whose edge is shorter than its wave's longest idles until the wave is done.
// Every edge has one writer: plain vector stores of dist, overlap_length and similarity at the edge's id.  Record: counters in
// registers, then gnm_group.h's block_count_add (one 64-bit integer atomic per non-zero word and workgroup): outputs and record
// depend on the inputs alone, not on the grid.
// gnm_overlap_align_host: the same header routine over host arrays, on `threads` host threads (contiguous ranges of edges, their
// counters added at the end).
#include <thread>
#include <vector>

#include "gnm_common.h"
#include "gnm_group.h"
#include "gnm_align.h"

namespace gnm {

struct AlignArgs {
  SeqStore s;
  int64_t E;
  const int32_t *src, *dst;
  const int64_t* pl;
  int K;
  int32_t* dist;
  int64_t* olen;
  float* sim;
};

template <int NW>
GNM_SEQ_FN AlignEdge align_one_(const AlignArgs& a, int64_t k) {
  const AlignEdge r = align_edge_<NW>(a.s, a.src[k], a.dst[k], a.pl[k], a.K);
  a.dist[k] = r.dist;
  a.olen[k] = r.m;
  a.sim[k] = r.similarity;
  return r;
}

template <int NW>
__global__ __launch_bounds__(kBlock) void overlap_align_k(AlignArgs a, unsigned long long* rec) {
  __shared__ unsigned long long lds[kWavesPerBlock];
  unsigned aligned = 0u, exceeded = 0u, empty = 0u, clamped = 0u, invalid = 0u;
  unsigned long long cells = 0ull;
  const int64_t nb = (a.E + kBlock - 1) / kBlock;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t k = b * kBlock + threadIdx.x;
    if (k >= a.E) continue;                              // no shuffle or barrier inside the loop
    const AlignEdge r = align_one_<NW>(a, k);
    clamped += r.flags & kAlnFlagClamped ? 1u : 0u;
    invalid += r.flags & kAlnFlagInvalid ? 1u : 0u;
    empty += r.flags & kAlnFlagEmpty ? 1u : 0u;
    exceeded += r.flags & kAlnFlagExceeded ? 1u : 0u;
    aligned += r.flags & (kAlnFlagInvalid | kAlnFlagEmpty | kAlnFlagExceeded) ? 0u : 1u;
    cells += (unsigned long long)r.cells;
  }
  block_count_add((unsigned long long)aligned, lds, rec + kAlnAligned);
  block_count_add((unsigned long long)exceeded, lds, rec + kAlnExceeded);
  block_count_add((unsigned long long)empty, lds, rec + kAlnEmpty);
  block_count_add((unsigned long long)clamped, lds, rec + kAlnClamped);
  block_count_add((unsigned long long)invalid, lds, rec + kAlnInvalid);
  block_count_add(cells, lds, rec + kAlnCells);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    atomicAdd(rec + kAlnEdges, (unsigned long long)a.E);
    atomicAdd(rec + kAlnCalls, 1ull);
  }
}

template <int NW>
static void align_host_range_(const AlignArgs& a, int64_t k0, int64_t k1, int64_t* rec) {
  for (int64_t k = k0; k < k1; ++k) {
    const AlignEdge r = align_one_<NW>(a, k);
    rec[kAlnClamped] += r.flags & kAlnFlagClamped ? 1 : 0;
    rec[kAlnInvalid] += r.flags & kAlnFlagInvalid ? 1 : 0;
    rec[kAlnEmpty] += r.flags & kAlnFlagEmpty ? 1 : 0;
    rec[kAlnExceeded] += r.flags & kAlnFlagExceeded ? 1 : 0;
    rec[kAlnAligned] += r.flags & (kAlnFlagInvalid | kAlnFlagEmpty | kAlnFlagExceeded) ? 0 : 1;
    rec[kAlnCells] += r.cells;
  }
}

}  // namespace gnm

using namespace gnm;

static int align_check(const char* what, int64_t E, const int32_t* src, const int32_t* dst, const int64_t* pl, const uint8_t* packed,
                       int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int64_t n, int max_errors,
                       const int32_t* dist, const int64_t* olen, const float* sim, const void* record) {
  GNM_CHECK_ARG(E >= 0 && E < INT32_MAX, "%s: E = %lld: expected 0 <= E < 2^31 - 1", what, (long long)E);
  GNM_CHECK_ARG(max_errors >= 0 && max_errors <= kAlignMaxErrors, "%s: max_errors = %d: expected 0 <= max_errors <= %d", what,
                max_errors, kAlignMaxErrors);
  if (seq_store_check(what, n, R, base_off, length, packed_bytes)) return -1;
  GNM_CHECK_ARG(packed_bytes == 0 || (packed && ((uintptr_t)packed & 3) == 0), "%s: packed must be non-null and 4-byte aligned", what);
  if (record_check(what, record, "gnm_align_record")) return -1;
  GNM_CHECK_ARG(E == 0 || (src && dst && pl && dist && olen && sim),
                "%s: src, dst, prefix_length, dist, overlap_length and similarity must not be null when E > 0", what);
  return 0;
}

static AlignArgs align_args(int64_t E, const int32_t* src, const int32_t* dst, const int64_t* pl, const uint8_t* packed,
                            int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int64_t n, int max_errors,
                            int32_t* dist, int64_t* olen, float* sim) {
  AlignArgs a = {};
  a.s.packed = packed; a.s.base_off = base_off; a.s.length = length; a.s.nibbles = packed_bytes * 2; a.s.R = R; a.s.n = n;
  a.E = E; a.src = src; a.dst = dst; a.pl = pl; a.K = max_errors;
  a.dist = dist; a.olen = olen; a.sim = sim;
  return a;
}

extern "C" int gnm_overlap_align(int64_t E, const int32_t* src, const int32_t* dst, const int64_t* prefix_length, const uint8_t* packed,
                                 int64_t packed_bytes, const int64_t* base_off, const int64_t* length, int64_t R, int64_t n,
                                 int max_errors, int32_t* dist, int64_t* overlap_length, float* similarity, void* record, void* stream) {
  if (align_check("overlap_align", E, src, dst, prefix_length, packed, packed_bytes, base_off, length, R, n, max_errors, dist,
                  overlap_length, similarity, record))
    return -1;
  if (E == 0) return 0;                                  // nothing to write: nothing is launched, the record stays as it is
  const AlignArgs a = align_args(E, src, dst, prefix_length, packed, packed_bytes, base_off, length, R, n, max_errors, dist,
                                 overlap_length, similarity);
  const dim3 grid(persistent_grid((E + kBlock - 1) / kBlock, 1, 8)), blk(kBlock);
  unsigned long long* rec = (unsigned long long*)record;
  hipStream_t st = (hipStream_t)stream;
  switch (align_words_(max_errors)) {
    case 1: hipLaunchKernelGGL(overlap_align_k<1>, grid, blk, 0, st, a, rec); break;
    case 2: hipLaunchKernelGGL(overlap_align_k<2>, grid, blk, 0, st, a, rec); break;
    case 4: hipLaunchKernelGGL(overlap_align_k<4>, grid, blk, 0, st, a, rec); break;
    default: hipLaunchKernelGGL(overlap_align_k<8>, grid, blk, 0, st, a, rec); break;
  }
  GNM_LAUNCH_CHECK("overlap_align");
  return 0;
}

extern "C" int gnm_overlap_align_host(int64_t E, const int32_t* src, const int32_t* dst, const int64_t* prefix_length,
                                      const uint8_t* packed, int64_t packed_bytes, const int64_t* base_off, const int64_t* length,
                                      int64_t R, int64_t n, int max_errors, int32_t* dist, int64_t* overlap_length, float* similarity,
                                      void* record, int threads) {
  if (align_check("overlap_align_host", E, src, dst, prefix_length, packed, packed_bytes, base_off, length, R, n, max_errors, dist,
                  overlap_length, similarity, record))
    return -1;
  GNM_CHECK_ARG(threads >= 1 && threads <= 1024, "overlap_align_host: threads = %d: expected 1 <= threads <= 1024", threads);
  if (E == 0) return 0;
  const AlignArgs a = align_args(E, src, dst, prefix_length, packed, packed_bytes, base_off, length, R, n, max_errors, dist,
                                 overlap_length, similarity);
  const int nt = (int64_t)threads < E ? threads : (int)E;
  std::vector<int64_t> recs((size_t)nt * 8, 0);
  auto run = [&](int t) {
    const int64_t k0 = E * t / nt, k1 = E * (t + 1) / nt;
    int64_t* r = recs.data() + (size_t)t * 8;
    switch (align_words_(max_errors)) {
      case 1: align_host_range_<1>(a, k0, k1, r); break;
      case 2: align_host_range_<2>(a, k0, k1, r); break;
      case 4: align_host_range_<4>(a, k0, k1, r); break;
      default: align_host_range_<8>(a, k0, k1, r); break;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < nt; ++t) pool.emplace_back(run, t);
  run(0);
  for (auto& th : pool) th.join();
  int64_t* rec = (int64_t*)record;
  for (int t = 0; t < nt; ++t)
    for (int w = 0; w < 8; ++w) rec[w] += recs[(size_t)t * 8 + w];
  rec[kAlnEdges] += E;
  rec[kAlnCalls] += 1;
  return 0;
}
