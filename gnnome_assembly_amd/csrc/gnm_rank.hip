// Threshold-free validation metrics: one streaming pass over (logit, label) builds a per-label histogram over a monotone
// 14-bit key of the fp32 logit.  AUROC (with exact bounds), average precision, the ROC / PR curves and the best-F1 threshold
// all follow from the 2 x 16384 counts on the host (train.RankingMetrics.from_counts); nothing is sorted and no [E] scratch
// exists.
//
//   key(x) = u >> 18,  u = bits(x == -0 ? +0 : x),  u ^= (u >> 31) ? 0xFFFFFFFF : 0x80000000
//
// (the usual order-preserving map of IEEE bits onto unsigned integers; sign + 8 exponent bits + 5 mantissa bits survive the
// shift).  key is monotone non-decreasing in x, -inf has the lowest key a value can take and +inf the highest.  -0 is mapped to
// +0 on the BIT PATTERN, which equals x + 0.0f and, unlike it, does not depend on the denormal mode: a denormal keeps its bits.
//
// The record (gnm.h: gnm_rank_record) is int64 hist[2][16384] (label 0 first) and int64 tail[4] = {nan_pos, nan_neg,
// other_label, calls}; a call ADDS to it.
//
// Kernel.  A persistent grid of at most one workgroup per CU (the grid of persistent_grid(): gnm_set_occupancy_cap can only
// lower a count, and one is the least), 1024 threads, the whole 2 x 16384 histogram privatised as uint32 in 128 KiB of LDS.
// A workgroup walks tiles of 4096 consecutive elements (one float4 of logits and one of labels per thread, two tiles in
// flight), adds to its LDS bins, and at the end adds its NON-ZERO bins to the record with 64-bit integer atomics.  Real logits
// occupy a few hundred bins, so a workgroup sends a few hundred atomics where a partials-and-reduce flush would write and read
// back 128 KiB per workgroup (32 MiB on 256 CUs: more than the 60 MB the pass itself reads at E = 7.5 M).
//
// Hot bins.  The LDS adds of a wave that fall into one bin serialise.  Before adding, a wave peels the bin of its first
// active lane, twice: the lanes that share it are counted with a ballot and ONE lane adds the count.  With all logits equal
// (one bin per label) a wave then issues two LDS adds for 64 elements; with spread logits it issues two single-lane adds more
// than it otherwise would.
//
// Result.  Every count in the record is an integer sum of per-element contributions, and integer addition is commutative and
// associative: whichever workgroup, wave or lane counts an element, and in whatever order the LDS and the global atomics land,
// the record is the same function of (scores, y, previous record).  No ordering argument is needed and none is made; two runs,
// two grids and two occupancy caps give identical bits.
//
// Overflow.  A workgroup's uint32 bins cannot overflow while its share of one call is below 2^31 elements; the host checks that
// and returns an error otherwise.
#include "gnm_common.h"

namespace gnm {

constexpr int kRankBins = 16384;                        // per label
constexpr int kRankThreads = 1024;                      // 16 waves: one workgroup per CU has to hide the load latency alone
constexpr int kRankTile = 4 * kRankThreads;             // elements per tile
constexpr int kRankPeel = 2;                            // hot bins combined per wave and element slot

// 0 .. 2 * kRankBins - 1: label * kRankBins + key.  -1: a NaN logit.  -2: a label that is neither 0 nor 1 (checked first).
__device__ __forceinline__ int rank_slot_(float x, float y) {
  int lab;
  if (y == 1.0f) lab = 1;
  else if (y == 0.0f) lab = 0;
  else return -2;
  unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return -1;
  if (u == 0x80000000u) u = 0u;                         // -0 -> +0
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return lab * kRankBins + (int)(u >> 18);
}

// Every lane of the wave calls this together; slot < 0: nothing to add.
__device__ __forceinline__ void rank_wave_add_(unsigned* hist, int slot) {
  bool active = slot >= 0;
#pragma unroll
  for (int r = 0; r < kRankPeel; ++r) {
    const unsigned long long m = __ballot(active);
    if (m == 0ull) return;                              // wave-uniform
    const int lead = __ffsll((long long)m) - 1;
    const int s0 = __builtin_amdgcn_readlane(slot, lead);
    const bool same = active && slot == s0;
    const unsigned long long sm = __ballot(same);
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(&hist[s0], (unsigned)__popcll(sm));
    active = active && !same;
  }
  if (active) atomicAdd(&hist[slot], 1u);
}

struct RankTile { float x[4]; float y[4]; int n; };     // n valid elements (0 .. 4)

template <bool VEC>
__device__ __forceinline__ RankTile rank_load_(int64_t E, const float* __restrict__ scores, const float* __restrict__ y,
                                               int64_t tile, int64_t ntiles) {
  RankTile t;
  const int64_t i = tile * kRankTile + 4 * (int64_t)threadIdx.x;
  const int64_t left = tile < ntiles ? E - i : 0;
  t.n = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  if (VEC && t.n == 4) {
    const float4 a = ld4_nt(scores + i), b = ld4_nt(y + i);
    t.x[0] = a.x; t.x[1] = a.y; t.x[2] = a.z; t.x[3] = a.w;
    t.y[0] = b.x; t.y[1] = b.y; t.y[2] = b.z; t.y[3] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      t.x[k] = k < t.n ? scores[i + k] : 0.f;
      t.y[k] = k < t.n ? y[i + k] : 0.f;
    }
  }
  return t;
}

__device__ __forceinline__ void rank_count_(const RankTile& t, unsigned* hist, unsigned& nan_pos, unsigned& nan_neg,
                                            unsigned& other) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int slot = -3;                                      // past the end: counted nowhere
    if (k < t.n) {
      slot = rank_slot_(t.x[k], t.y[k]);
      other += slot == -2 ? 1u : 0u;
      nan_pos += (slot == -1 && t.y[k] == 1.0f) ? 1u : 0u;
      nan_neg += (slot == -1 && t.y[k] != 1.0f) ? 1u : 0u;
    }
    rank_wave_add_(hist, slot);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kRankThreads) void rank_hist_k(int64_t E, const float* __restrict__ scores,
                                                           const float* __restrict__ y, unsigned long long* rec) {
  __shared__ unsigned hist[2 * kRankBins];
  __shared__ unsigned tails[3];
  const int64_t ntiles = (E + kRankTile - 1) / kRankTile;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(rec + 2 * kRankBins + 3, 1ull);         // calls
  if ((int64_t)blockIdx.x >= ntiles) return;            // workgroup-uniform: nothing to count (E == 0, or a rounded-up grid)
  for (int i = threadIdx.x; i < 2 * kRankBins / 4; i += kRankThreads)
    reinterpret_cast<uint4*>(hist)[i] = make_uint4(0u, 0u, 0u, 0u);
  if (threadIdx.x < 3) tails[threadIdx.x] = 0u;
  __syncthreads();
  unsigned nan_pos = 0u, nan_neg = 0u, other = 0u;
  for (int64_t t0 = blockIdx.x; t0 < ntiles; t0 += 2 * (int64_t)gridDim.x) {
    const RankTile a = rank_load_<VEC>(E, scores, y, t0, ntiles);
    const RankTile b = rank_load_<VEC>(E, scores, y, t0 + gridDim.x, ntiles);
    rank_count_(a, hist, nan_pos, nan_neg, other);
    rank_count_(b, hist, nan_pos, nan_neg, other);
  }
  if (nan_pos) atomicAdd(&tails[0], nan_pos);
  if (nan_neg) atomicAdd(&tails[1], nan_neg);
  if (other) atomicAdd(&tails[2], other);
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * kRankBins; i += kRankThreads) {
    const unsigned v = hist[i];
    if (v) atomicAdd(rec + i, (unsigned long long)v);
  }
  if (threadIdx.x < 3 && tails[threadIdx.x]) atomicAdd(rec + 2 * kRankBins + threadIdx.x, (unsigned long long)tails[threadIdx.x]);
}

}  // namespace gnm

using namespace gnm;

// The non-zero bins go straight to the record: no per-workgroup partials, so no workspace.  The argument stays in the entry
// point so that a flush through partials could be put behind the same signature.
extern "C" size_t gnm_rank_hist_workspace_bytes(int64_t E) {
  (void)E;
  return 0;
}

extern "C" int gnm_rank_hist(int64_t E, const float* scores, const float* y, void* record, void* ws, size_t ws_bytes,
                             void* stream) {
  GNM_CHECK_ARG(E >= 0, "rank_hist: E = %lld is negative", (long long)E);
  GNM_CHECK_ARG(record && ((uintptr_t)record & 7) == 0, "rank_hist: record must be a non-null, 8-byte aligned gnm_rank_record");
  GNM_CHECK_ARG(E == 0 || (scores && y), "rank_hist: scores and y must not be null when E > 0");
  const size_t need = gnm_rank_hist_workspace_bytes(E);
  GNM_CHECK_ARG(ws_bytes >= need && (need == 0 || ws), "rank_hist: workspace of %zu bytes, %zu needed", ws_bytes, need);
  const int64_t ntiles = (E + kRankTile - 1) / kRankTile;
  const int grid = persistent_grid(ntiles, 1, 1);
  const int64_t share = (ntiles + grid - 1) / grid * kRankTile;        // the most elements one workgroup counts
  GNM_CHECK_ARG(share < ((int64_t)1 << 31), "rank_hist: E = %lld gives one of %d workgroups %lld elements, its 32-bit bins hold "
                "fewer than 2^31: split the call", (long long)E, grid, (long long)share);
  if ((((uintptr_t)scores | (uintptr_t)y) & 15) == 0)
    hipLaunchKernelGGL(rank_hist_k<true>, dim3(grid), dim3(kRankThreads), 0, (hipStream_t)stream, E, scores, y,
                       (unsigned long long*)record);
  else
    hipLaunchKernelGGL(rank_hist_k<false>, dim3(grid), dim3(kRankThreads), 0, (hipStream_t)stream, E, scores, y,
                       (unsigned long long*)record);
  GNM_LAUNCH_CHECK("rank_hist");
  return 0;
}
