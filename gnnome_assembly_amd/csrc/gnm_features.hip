// Input feature preparation on the GPU ("next" row f-1 of SURVEY.md section 8): what the reference
// does on the CPU with scipy before every run and re-uploads every step (train.py:245-251).
//   pagerank_pe      utils.add_positional_encoding (utils.py:97-138): float in/out degrees and the
//                    16-step PageRank features x <- alpha * P x + (1-alpha)/n, P = (D^-1 A)^T,
//                    iterated in fp64 like the reference, emitted as the [N, 2+pe_dim] fp32 tensor
//                    that train.py:251 / inference.py:452 concatenate (in_deg | out_deg | pe)
//   edge_feats_zscore utils.preprocess_graph (utils.py:70-74): z-score of overlap length and
//                    similarity with the unbiased std (torch.std default), -> e[E,2]
// and, on the other side of the model, the O(E) part of every decode iteration (inference.py:256-277):
//   decode_candidate_sums / decode_pick   start edges drawn by inverse CDF from the logits, where they already are
// Pull-style SpMV over the destination-sorted index: one thread per node, fixed summation order,
// no atomics.  Negligible next to the layer stack (E*4 B of indices + 8-byte gathers per step).
#include "gnm_common.h"
#include "gnm_ln.h"

namespace gnm {

// w[u] = x[u] / (outdeg[u] + 1e-9), 0 for nodes without out-edges (utils.py:126-127)
__global__ void pr_scale_k(int64_t N, const double* __restrict__ x, const int32_t* __restrict__ out_ptr,
                           double* __restrict__ w) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += (int64_t)gridDim.x * blockDim.x) {
    const double d = (double)(out_ptr[v + 1] - out_ptr[v]);
    w[v] = d < 1e-9 ? 0.0 : x[v] * (1.0 / (d + 1e-9));
  }
}

// x_new[v] = alpha * sum_{j in in(v)} w[isrc j] + (1-alpha)/n ; pe[v][2+step] = (float)x_new[v]
__global__ void pr_step_k(int64_t N, const double* __restrict__ w, const int32_t* __restrict__ isrc,
                          const int32_t* __restrict__ in_ptr, double alpha, double teleport,
                          double* __restrict__ x_new, float* __restrict__ pe, int ldpe, int col) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += (int64_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int j = in_ptr[v]; j < in_ptr[v + 1]; ++j) acc += w[isrc[j]];
    const double xn = alpha * acc + teleport;
    x_new[v] = xn;
    pe[v * ldpe + col] = (float)xn;
  }
}

__global__ void pr_init_k(int64_t N, const int32_t* __restrict__ in_ptr, const int32_t* __restrict__ out_ptr,
                          double* __restrict__ x, float* __restrict__ pe, int ldpe) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += (int64_t)gridDim.x * blockDim.x) {
    x[v] = 1.0 / (double)N;
    pe[v * ldpe + 0] = (float)(in_ptr[v + 1] - in_ptr[v]);     // in_deg  (utils.py:102)
    pe[v * ldpe + 1] = (float)(out_ptr[v + 1] - out_ptr[v]);   // out_deg (utils.py:103)
  }
}

// per-block (sum a, sum a^2, sum b, sum b^2) in fp64
__global__ __launch_bounds__(kBlock) void zs_stats_k(int64_t E, const float* __restrict__ a,
                                                     const float* __restrict__ b, double* __restrict__ part) {
  __shared__ double red[4][kBlock];
  double s[4] = {0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < E; i += (int64_t)gridDim.x * kBlock) {
    const double x = a[i], y = b[i];
    s[0] += x; s[1] += x * x; s[2] += y; s[3] += y * y;
  }
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int st = kBlock / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x < 4) part[(size_t)blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// e[perm? no: edge-id order][0] = (a - mean_a)/std_a, [1] likewise (unbiased std)
__global__ void zs_apply_k(int64_t E, const float* __restrict__ a, const float* __restrict__ b,
                           const double* __restrict__ part, int nblk, float* __restrict__ e) {
  __shared__ double st[4];
  if (threadIdx.x < 4) {
    double acc = 0.0;
    for (int k = 0; k < nblk; ++k) acc += part[(size_t)k * 4 + threadIdx.x];
    st[threadIdx.x] = acc;
  }
  __syncthreads();
  const double n = (double)E;
  const double ma = st[0] / n, mb = st[2] / n;
  const double va = (st[1] - n * ma * ma) / (n - 1.0), vb = (st[3] - n * mb * mb) / (n - 1.0);
  const double ra = 1.0 / sqrt(va), rb = 1.0 / sqrt(vb);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (int64_t)gridDim.x * blockDim.x) {
    e[2 * i] = (float)(((double)a[i] - ma) * ra);
    e[2 * i + 1] = (float)(((double)b[i] - mb) * rb);
  }
}

// ------------------------------------------------------------------------------------------
// Decode: candidate weights and inverse-CDF sampling of start edges (inference.py:256-277) on the device.
//   w_k = 0 when either end of edge k is visited or the edge is a self loop (get_subgraph), else max(sigmoid(x_k), 1e-9f)
//   C_k = w_0 + ... + w_k in fp64, pick(u) = the smallest k with C_k > u * C_{E-1}
// The edge ids are cut into blocks of kDecBlk -- a compile-time constant, NOT a function of the grid: the tree that sums a
// block, the scan over the block sums and therefore every pick are the same on any number of CUs and under any occupancy cap.
// No atomics, every loop bound is known at launch.
// ------------------------------------------------------------------------------------------
constexpr int kDecBlk = 2048;                    // edge ids per block sum: 8 per thread of a 256-thread workgroup
constexpr int kDecRounds = kDecBlk / kWave;      // 64-edge rounds of the in-block scan of one wave

struct DecStats {          // the 32 bytes `stats` of gnm.h
  double total;
  int64_t count;
  int64_t last_block;      // the last block with a candidate (-1: none)
  int64_t nblk;
};

// The once-per-edge sigmoid is evaluated in fp64 and rounded once: the weight is the fp32 number nearest to the fp64
// value (the hardware exp / rcp forms of the gate lose |x| * 6e-8 relative where sigma is small, which is exactly where the
// 1e-9 floor decides).  exp overflow gives 1 / inf = 0 -> the floor; NaN logits sit on the floor as well (fmaxf).
__device__ __forceinline__ float dec_weight(float x, int32_t s, int32_t d, int64_t N, const uint8_t* __restrict__ visited) {
  if ((uint32_t)s >= (uint64_t)N || (uint32_t)d >= (uint64_t)N || s == d) return 0.f;     // out-of-range ends are never gathered
  if (visited[s] | visited[d]) return 0.f;
  return fmaxf((float)(1.0 / (1.0 + exp(-(double)x))), 1e-9f);
}

// gnm_ln.h's butterfly on the two halves of a double: after the six steps every lane holds the wave's sum, bit-identical in all
// of them (each step adds the same two partial sums in both partners; fp64 addition is commutative).
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_mov_f64<0xB1>(v);                   // quad_perm [1,0,3,2]
  v += dpp_mov_f64<0x4E>(v);                   // quad_perm [2,3,0,1]
  v += dpp_mov_f64<0x141>(v);                  // row_half_mirror
  v += dpp_mov_f64<0x140>(v);                  // row_mirror
  typedef unsigned u32x2_dec_ __attribute__((ext_vector_type(2)));
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const u32x2_dec_ sl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const u32x2_dec_ sh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const unsigned l0 = sl.x, l1 = sl.y, h0 = sh.x, h1 = sh.y;      // through scalars first (gnm_ln.h)
  v = __hiloint2double((int)h0, (int)l0) + __hiloint2double((int)h1, (int)l1);
  v += __shfl_xor(v, 32, 64);
  return v;
}
// Inclusive scan over the 64 lanes in lane order: row_shr 1/2/4/8 inside the 16-lane rows (lanes shifted in from outside
// a row read 0), then the totals of the rows before this lane's row, added in row order.  `total` = the wave's sum.
__device__ __forceinline__ double wave_scan_f64(double v, double& total) {
  v += dpp_mov_f64<0x111>(v);
  v += dpp_mov_f64<0x112>(v);
  v += dpp_mov_f64<0x114>(v);
  v += dpp_mov_f64<0x118>(v);
  const double r0 = __shfl(v, 15, 64), r1 = __shfl(v, 31, 64), r2 = __shfl(v, 47, 64), r3 = __shfl(v, 63, 64);
  const int row = (threadIdx.x & 63) >> 4;
  const double r01 = r0 + r1, r012 = r01 + r2;
  total = r012 + r3;
  return row == 0 ? v : (row == 1 ? r0 + v : (row == 2 ? r01 + v : r012 + v));
}

// Pass 1: a plain stream.  Workgroup-sized blocks of edge ids; thread t of a block owns the ids 4t..4t+3 and 1024+4t..+3 and adds
// them in that order, the lanes combine by the butterfly, the four waves through LDS in wave order.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void dec_sums_k(int64_t E, int64_t N, int64_t nblk, const float* __restrict__ x,
                                                     const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                     const uint8_t* __restrict__ visited, double* __restrict__ bsum,
                                                     int32_t* __restrict__ bcnt, float* __restrict__ w_out) {
  __shared__ double red[kWavesPerBlock];
  __shared__ int redc[kWavesPerBlock];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
    double acc = 0.0;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t k0 = b * kDecBlk + j * (kDecBlk / 2) + 4 * (int64_t)threadIdx.x;
      float w[4] = {0.f, 0.f, 0.f, 0.f};
      if (VEC && k0 + 3 < E) {
        const float4 xv = ld4(x + k0);
        const int4 sv = *reinterpret_cast<const int4*>(src + k0), dv = *reinterpret_cast<const int4*>(dst + k0);
        w[0] = dec_weight(xv.x, sv.x, dv.x, N, visited);
        w[1] = dec_weight(xv.y, sv.y, dv.y, N, visited);
        w[2] = dec_weight(xv.z, sv.z, dv.z, N, visited);
        w[3] = dec_weight(xv.w, sv.w, dv.w, N, visited);
        if (w_out) st4(w_out + k0, make_float4(w[0], w[1], w[2], w[3]));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (k0 + i < E) {
            w[i] = dec_weight(x[k0 + i], src[k0 + i], dst[k0 + i], N, visited);
            if (w_out) w_out[k0 + i] = w[i];
          }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc += (double)w[i];
        cnt += w[i] > 0.f ? 1 : 0;
      }
    }
    acc = wave_sum_f64(acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) { red[wave] = acc; redc[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
      bsum[b] = ((red[0] + red[1]) + red[2]) + red[3];
      bcnt[b] = redc[0] + redc[1] + redc[2] + redc[3];
    }
    __syncthreads();
  }
}

// One workgroup turns the block sums into their inclusive prefix, in place: thread t owns `chunk` consecutive blocks,
// thread 0 scans the 256 chunk totals in order.  Also the candidate count, the total and the last block that has a candidate.
__global__ __launch_bounds__(kBlock) void dec_scan_k(int64_t nblk, int64_t chunk, double* __restrict__ bsum,
                                                     const int32_t* __restrict__ bcnt, DecStats* __restrict__ stats) {
  __shared__ double tsum[kBlock];
  __shared__ long long tcnt[kBlock];
  __shared__ long long tlast[kBlock];
  const int64_t b0 = (int64_t)threadIdx.x * chunk, b1 = b0 + chunk < nblk ? b0 + chunk : nblk;
  double s = 0.0;
  long long c = 0, last = -1;
  for (int64_t b = b0; b < b1; ++b) {
    s += bsum[b];
    c += bcnt[b];
    if (bcnt[b] > 0) last = b;
  }
  tsum[threadIdx.x] = s; tcnt[threadIdx.x] = c; tlast[threadIdx.x] = last;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    long long cc = 0, ll = -1;
    for (int t = 0; t < kBlock; ++t) {
      const double v = tsum[t];
      tsum[t] = run;                 // exclusive: what precedes thread t's chunk
      run += v;
      cc += tcnt[t];
      if (tlast[t] > ll) ll = tlast[t];
    }
    stats->count = cc;               // (total: below, by the owner of the last block)
    stats->last_block = ll;
    stats->nblk = nblk;
  }
  __syncthreads();
  double run = tsum[threadIdx.x];
  for (int64_t b = b0; b < b1; ++b) {
    run += bsum[b];
    bsum[b] = run;
    if (b == nblk - 1) stats->total = run;
  }
}

// Pass 2: one wave per draw.  Binary search over the block prefix (`steps` = its bound, from the host), then the block's 2048
// weights again: lane l holds edge 64 j + l of round j, the rounds are scanned in order with a running carry, so the in-block
// prefix is in edge-id order.  The pick is the first edge with w > 0 whose prefix exceeds the target; when rounding leaves none
// (u * total == total, or the in-block sum a last bit below the block's tree sum) it is the last edge with w > 0 -- a pick never
// names a zero-weight edge.
__global__ __launch_bounds__(kBlock) void dec_pick_k(int64_t E, int64_t N, const float* __restrict__ x,
                                                     const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                     const uint8_t* __restrict__ visited, const double* __restrict__ bpre,
                                                     const DecStats* __restrict__ stats, int nb, int steps,
                                                     const double* __restrict__ u, int32_t* __restrict__ picks) {
  const int lane = threadIdx.x & 63;
  const int draw = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (draw >= nb || stats->count == 0) return;           // wave-uniform
  const int64_t nblk = stats->nblk;
  const double target = u[draw] * stats->total;
  int64_t lo = 0, hi = nblk;                            // the smallest b with bpre[b] > target; nblk if none
  for (int it = 0; it < steps; ++it)
    if (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (bpre[mid] > target) hi = mid; else lo = mid + 1;
    }
  const bool none = lo >= nblk;
  const int64_t b = none ? stats->last_block : lo;
  const double r = target - (b > 0 ? bpre[b - 1] : 0.0);
  float w[kDecRounds];
#pragma unroll
  for (int j = 0; j < kDecRounds; ++j) {
    const int64_t k = b * kDecBlk + j * kWave + lane;
    w[j] = k < E ? dec_weight(x[k], src[k], dst[k], N, visited) : 0.f;
  }
  double carry = 0.0;
  int first = -1, last = -1;                             // in-block offsets
#pragma unroll
  for (int j = 0; j < kDecRounds; ++j) {
    double tot;
    const double incl = carry + wave_scan_f64((double)w[j], tot);
    const unsigned long long live = __ballot(w[j] > 0.f);
    const unsigned long long hit = __ballot(w[j] > 0.f && !none && incl > r);
    if (first < 0 && hit) first = j * kWave + (__ffsll((long long)hit) - 1);
    if (live) last = j * kWave + (63 - __clzll((long long)live));
    carry += tot;
  }
  const int off = first >= 0 ? first : last;
  if (lane == 0 && off >= 0) picks[draw] = (int32_t)(b * kDecBlk + off);
}

}  // namespace gnm

using namespace gnm;

// ws: 3*N doubles
extern "C" size_t gnm_pagerank_pe_workspace_bytes(int64_t N) { return (size_t)3 * (size_t)N * sizeof(double); }

extern "C" int gnm_pagerank_pe(int64_t N, int64_t E, const int32_t* isrc, const int32_t* in_ptr,
                               const int32_t* out_ptr, int pe_dim, double alpha, float* pe, void* ws,
                               size_t ws_bytes, void* stream) {
  // isrc may be null when E == 0 (an empty tensor has no storage): in_ptr is all zeros then and no kernel reads isrc
  GNM_CHECK_ARG(N > 0 && E >= 0 && (E == 0 || isrc) && in_ptr && out_ptr && pe_dim >= 0 && pe, "pagerank_pe: bad argument");
  GNM_CHECK_ARG(ws && ws_bytes >= gnm_pagerank_pe_workspace_bytes(N), "pagerank_pe: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* x = (double*)ws;
  double* xn = x + N;
  double* w = x + 2 * N;
  const int ld = pe_dim + 2, g = ew_grid(N, 256);
  hipLaunchKernelGGL(pr_init_k, dim3(g), dim3(256), 0, st, N, in_ptr, out_ptr, x, pe, ld);
  for (int s = 0; s < pe_dim; ++s) {
    hipLaunchKernelGGL(pr_scale_k, dim3(g), dim3(256), 0, st, N, (const double*)x, out_ptr, w);
    hipLaunchKernelGGL(pr_step_k, dim3(g), dim3(256), 0, st, N, (const double*)w, isrc, in_ptr, alpha,
                       (1.0 - alpha) / (double)N, xn, pe, ld, 2 + s);
    double* tmp = x; x = xn; xn = tmp;
  }
  GNM_LAUNCH_CHECK("pagerank_pe");
  return 0;
}

// ws: 4 * gnm_max_partial_blocks() doubles
extern "C" int gnm_edge_feats_zscore(int64_t E, const float* overlap_length, const float* overlap_similarity,
                                     float* e, void* ws, size_t ws_bytes, void* stream) {
  GNM_CHECK_ARG(E > 1 && overlap_length && overlap_similarity && e, "edge_feats_zscore: bad argument");
  int nb = ew_grid(E, 256);
  if (nb > kMaxPartialBlocks) nb = kMaxPartialBlocks;
  GNM_CHECK_ARG(ws && ws_bytes >= (size_t)nb * 4 * sizeof(double), "edge_feats_zscore: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(zs_stats_k, dim3(nb), dim3(kBlock), 0, st, E, overlap_length, overlap_similarity, (double*)ws);
  hipLaunchKernelGGL(zs_apply_k, dim3(ew_grid(E, 256)), dim3(256), 0, st, E, overlap_length, overlap_similarity,
                     (const double*)ws, nb, e);
  GNM_LAUNCH_CHECK("edge_feats_zscore");
  return 0;
}

// ws: the block sums / prefix (fp64) and the block counts (int32) of ceil(E / 2048) blocks
static inline int64_t dec_blocks(int64_t E) { return (E + kDecBlk - 1) / kDecBlk; }
static inline size_t dec_cnt_offset(int64_t nblk) { return ((size_t)nblk * sizeof(double) + 15) / 16 * 16; }
extern "C" size_t gnm_decode_sample_workspace_bytes(int64_t E) {
  const int64_t nblk = dec_blocks(E < 0 ? 0 : E);
  return dec_cnt_offset(nblk) + (size_t)nblk * sizeof(int32_t) + 16;
}

extern "C" int gnm_decode_candidate_sums(int64_t E, int64_t N, const float* scores, const int32_t* src, const int32_t* dst,
                                         const uint8_t* visited, void* ws, size_t ws_bytes, float* w_out, void* stats,
                                         void* stream) {
  GNM_CHECK_ARG(E >= 0 && E < INT32_MAX && N >= 0 && N < INT32_MAX && stats, "decode_candidate_sums: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (E == 0) {                                    // no candidate, nothing to launch
    hipError_t e = hipMemsetAsync(stats, 0, sizeof(DecStats), st);
    if (e != hipSuccess) return hip_fail(e, "decode_candidate_sums");
    return 0;
  }
  GNM_CHECK_ARG(scores && src && dst && visited && N > 0, "decode_candidate_sums: null argument");
  GNM_CHECK_ARG(ws && ws_bytes >= gnm_decode_sample_workspace_bytes(E) && ((uintptr_t)ws & 15) == 0,
                "decode_candidate_sums: workspace too small or not 16-byte aligned");
  const int64_t nblk = dec_blocks(E);
  double* bsum = (double*)ws;
  int32_t* bcnt = (int32_t*)((char*)ws + dec_cnt_offset(nblk));
  const int grid = persistent_grid(nblk, 1, 8);    // any grid gives the same sums: the blocks are fixed
  const bool vec = (((uintptr_t)scores | (uintptr_t)src | (uintptr_t)dst | (uintptr_t)w_out) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(dec_sums_k<true>, dim3(grid), dim3(kBlock), 0, st, E, N, nblk, scores, src, dst, visited, bsum, bcnt, w_out);
  else
    hipLaunchKernelGGL(dec_sums_k<false>, dim3(grid), dim3(kBlock), 0, st, E, N, nblk, scores, src, dst, visited, bsum, bcnt, w_out);
  hipLaunchKernelGGL(dec_scan_k, dim3(1), dim3(kBlock), 0, st, nblk, (nblk + kBlock - 1) / kBlock, bsum, (const int32_t*)bcnt,
                     (DecStats*)stats);
  GNM_LAUNCH_CHECK("decode_candidate_sums");
  return 0;
}

extern "C" int gnm_decode_pick(int64_t E, int64_t N, const float* scores, const int32_t* src, const int32_t* dst,
                               const uint8_t* visited, const void* ws, const void* stats, int nb, const double* u,
                               int32_t* picks, void* stream) {
  GNM_CHECK_ARG(E >= 0 && E < INT32_MAX && N >= 0 && N < INT32_MAX && nb >= 0, "decode_pick: bad argument");
  if (E == 0 || nb == 0) return 0;
  GNM_CHECK_ARG(scores && src && dst && visited && ws && stats && u && picks && N > 0, "decode_pick: null argument");
  const int64_t nblk = dec_blocks(E);
  int steps = 1;
  while (((int64_t)1 << steps) < nblk + 1) ++steps;       // the search interval [0, nblk] halves every step
  ++steps;
  hipLaunchKernelGGL(dec_pick_k, dim3((nb + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, (hipStream_t)stream, E, N,
                     scores, src, dst, visited, (const double*)ws, (const DecStats*)stats, nb, steps, u, picks);
  GNM_LAUNCH_CHECK("decode_pick");
  return 0;
}
