// Contig sequences on the device (include/gnm.h, "contig sequences"): walks in CSR form + a packed read store -> the contigs'
// bases as ASCII, back to back in one buffer.  The per-position and per-lane arithmetic is csrc/gnm_seq.h.
//
// gnm_seq_layout, four launches on one stream:
//   scan_launch   the three launches of gnm_scan.h (int64, one position per thread) with SeqScan as their user: the sums phase also
//                 forms and stores piece_len[p] of every walk position and counts; the middle phase leaves piece_off[P] = the total
//                 and the record's contigs, pieces, bases, calls; the apply phase piece_off[p].
//   seq_cptr_k    contig_base_ptr[c] = piece_off[contig_ptr[c]].
// gnm_seq_emit, one launch: a workgroup owns a run of consecutive chunks of kSeqChunkBases output bases.  Per chunk its first
// thread finds the pieces of the chunk's first and last base in piece_off (binary search for the run's first chunk, a few steps
// forward from the previous chunk's last piece after that) and leaves the range in LDS; every lane then finds the piece of its
// first base inside that range and writes its 16 bases with one aligned 16-byte store.
// No workgroup waits for another, nothing is read back between the launches, no float arithmetic; integer atomics on the record
// words only (one per counter and workgroup): bytes and record depend on the inputs alone, not on the grid or on timing.
#include "gnm_common.h"
#include "gnm_scan.h"
#include "gnm_seq.h"

namespace gnm {

enum { kSeqContigs = 0, kSeqPieces, kSeqBases, kSeqClamped, kSeqEmpty, kSeqReverse, kSeqInvalid, kSeqCalls };

struct SeqArgs {
  SeqStore s;
  int64_t C, P, E;
  const int32_t *contig_ptr, *walk_nodes, *walk_edges;
  const int64_t* prefix_length;
  int64_t *piece_len, *piece_off, *contig_base_ptr;
  unsigned long long* rec;
  int64_t total;                         // emit: the bases the caller read from the record
  uint8_t* out;
};

// The scanned sequence: piece_len (-> piece_off).  The sums phase is its producer as well: it forms piece_len[p] (the position's contig
// by binary search in contig_ptr; node, read and edge checked before they address anything), stores it and counts; apply reads it back.
struct SeqScan : ScanUser<int64_t, 1> {
  SeqArgs a;
  unsigned clamped = 0u, empty = 0u, reverse = 0u, invalid = 0u;
  __device__ __forceinline__ void load(const Arrays& x, int64_t p, bool first, int64_t (&v)[1][1]) {
    int64_t k = 0;
    if (p < x.n && !first) k = a.piece_len[p];
    if (p < x.n && first) {
      unsigned f;
      k = seq_piece_len_(a.s, a.C, a.P, a.E, a.contig_ptr, a.walk_nodes, a.walk_edges, a.prefix_length, p, f);
      a.piece_len[p] = k;
      clamped += f & 1u;
      reverse += (f >> 1) & 1u;
      invalid += (f >> 2) & 1u;
      empty += (k == 0 && !(f & 4u)) ? 1u : 0u;
    }
    v[0][0] = k;
  }
  __device__ __forceinline__ void sums_end(int64_t* lds64) {
    unsigned* lds = reinterpret_cast<unsigned*>(lds64);
    block_count_add(clamped, lds, a.rec + kSeqClamped);
    block_count_add(empty, lds, a.rec + kSeqEmpty);
    block_count_add(reverse, lds, a.rec + kSeqReverse);
    block_count_add(invalid, lds, a.rec + kSeqInvalid);
  }
  // piece_off[P] = the total; record: contigs, pieces, bases, calls
  __device__ __forceinline__ void total(const Arrays& x, int, int64_t total) const {
    x.out[0][x.n] = total;
    if (a.C > 0) atomicAdd(a.rec + kSeqContigs, (unsigned long long)a.C);
    if (a.P > 0) atomicAdd(a.rec + kSeqPieces, (unsigned long long)a.P);
    if (total > 0) atomicAdd(a.rec + kSeqBases, (unsigned long long)total);
    atomicAdd(a.rec + kSeqCalls, 1ull);
  }
};

__global__ __launch_bounds__(kBlock) void seq_cptr_k(SeqArgs a) {
  for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c <= a.C; c += (int64_t)gridDim.x * kBlock) {
    int64_t i = a.contig_ptr[c];
    i = i < 0 ? 0 : (i > a.P ? a.P : i);
    a.contig_base_ptr[c] = a.piece_off[i];
  }
}

__global__ __launch_bounds__(kBlock) void seq_emit_k(SeqArgs a) {
  __shared__ int64_t range[2];
  const int64_t all = a.piece_off[a.P];
  const int64_t total = a.total < all ? a.total : all;   // never past what the layout pass laid out
  const int64_t nchunks = (total + kSeqChunkBases - 1) / kSeqChunkBases;
  // A workgroup takes a run of consecutive chunks: the piece that ends one chunk is where the search for the next one starts,
  // so only the first chunk of a workgroup pays a binary search over all P offsets.
  const int64_t per = (nchunks + gridDim.x - 1) / gridDim.x;
  const int64_t ch0 = (int64_t)blockIdx.x * per, ch1 = ch0 + per < nchunks ? ch0 + per : nchunks;
  int64_t prev = -1;                                     // thread 0: the piece of the previous chunk's last base
  for (int64_t ch = ch0; ch < ch1; ++ch) {
    const int64_t c0 = ch * kSeqChunkBases;
    if (threadIdx.x == 0) {
      const int64_t end = c0 + kSeqChunkBases < total ? c0 + kSeqChunkBases : total;
      const int64_t lo = prev < 0 ? seq_find_(a.piece_off, 0, a.P - 1, c0) : seq_gallop_(a.piece_off, prev, a.P - 1, c0);
      prev = seq_gallop_(a.piece_off, lo, a.P - 1, end - 1);
      range[0] = lo;
      range[1] = prev;
    }
    __syncthreads();
    const int64_t lo = range[0], hi = range[1];
    const int64_t g0 = c0 + (int64_t)threadIdx.x * kSeqLaneBases;
    if (g0 < total) {
      uint64_t o[2];
      seq_lane_(a.s, a.walk_nodes, a.piece_off, lo, hi, g0, total, o);
      *reinterpret_cast<uint4*>(a.out + g0) =
          make_uint4((uint32_t)o[0], (uint32_t)(o[0] >> 32), (uint32_t)o[1], (uint32_t)(o[1] >> 32));
    }
    __syncthreads();
  }
}

}  // namespace gnm

using namespace gnm;

static_assert(kSeqChunkBases == GNM_SEQ_CHUNK_BASES, "include/gnm.h states the chunk size");

extern "C" size_t gnm_seq_workspace_bytes(int64_t P) {
  if (P < 0 || P >= INT32_MAX) return 0;
  return scan_bsum_bytes<int64_t, 1>(P);
}

extern "C" int gnm_seq_layout(int64_t C, int64_t P, int64_t E, int64_t n, int64_t R, const int32_t* contig_ptr,
                              const int32_t* walk_nodes, const int32_t* walk_edges, const int64_t* prefix_length,
                              const int64_t* base_off, const int64_t* length, int64_t packed_bytes, void* record, int64_t* piece_len,
                              int64_t* piece_off, int64_t* contig_base_ptr, void* ws, size_t ws_bytes, void* stream) {
  GNM_CHECK_ARG(C >= 0 && P >= 0 && E >= 0 && C < INT32_MAX && P < INT32_MAX && E < INT32_MAX,
                "seq_layout: C = %lld, P = %lld, E = %lld: expected 0 <= C, P, E < 2^31 - 1", (long long)C, (long long)P, (long long)E);
  if (seq_store_check("seq_layout", n, R, base_off, length, packed_bytes)) return -1;
  if (record_check("seq_layout", record, "gnm_seq_record")) return -1;
  GNM_CHECK_ARG(contig_ptr && piece_off && contig_base_ptr, "seq_layout: contig_ptr, piece_off and contig_base_ptr must not be null");
  GNM_CHECK_ARG(P == 0 || (walk_nodes && walk_edges && piece_len), "seq_layout: walk_nodes, walk_edges and piece_len must not be null when P > 0");
  GNM_CHECK_ARG(E == 0 || prefix_length, "seq_layout: prefix_length must not be null when E > 0");
  const size_t need = gnm_seq_workspace_bytes(P);
  if (ws_check("seq_layout", "gnm_seq_workspace_bytes", ws, ws_bytes, need)) return -1;
  hipStream_t st = (hipStream_t)stream;
  SeqArgs a = {};
  a.s.packed = nullptr; a.s.base_off = base_off; a.s.length = length; a.s.nibbles = packed_bytes * 2; a.s.R = R; a.s.n = n;
  a.C = C; a.P = P; a.E = E;
  a.contig_ptr = contig_ptr; a.walk_nodes = walk_nodes; a.walk_edges = walk_edges; a.prefix_length = prefix_length;
  a.piece_len = piece_len; a.piece_off = piece_off; a.contig_base_ptr = contig_base_ptr;
  a.rec = (unsigned long long*)record;
  scan_launch<int64_t, 1, 1>(SeqScan{{}, a}, {P, {(int64_t*)ws}, {piece_off}}, st);       // P == 0: piece_off[0] = 0, calls += 1
  hipLaunchKernelGGL(seq_cptr_k, dim3(persistent_grid(C + 1, kBlock, 8)), dim3(kBlock), 0, st, a);
  GNM_LAUNCH_CHECK("seq_layout");
  return 0;
}

extern "C" int gnm_seq_emit(int64_t P, int64_t n, int64_t R, const int32_t* walk_nodes, const int64_t* piece_off,
                            const int64_t* base_off, const int64_t* length, const uint8_t* packed, int64_t packed_bytes,
                            int64_t total, uint8_t* out, int64_t out_bytes, void* stream) {
  GNM_CHECK_ARG(P >= 0 && P < INT32_MAX && total >= 0, "seq_emit: P = %lld, total = %lld: expected 0 <= P < 2^31 - 1, 0 <= total",
                (long long)P, (long long)total);
  if (seq_store_check("seq_emit", n, R, base_off, length, packed_bytes)) return -1;
  GNM_CHECK_ARG(out_bytes >= 0 && out_bytes % 16 == 0 && total <= out_bytes,
                "seq_emit: out_bytes = %lld for %lld bases: expected a multiple of 16 that holds them", (long long)out_bytes,
                (long long)total);
  if (total == 0 || P == 0) return 0;                                          // nothing to write: nothing is launched
  GNM_CHECK_ARG(walk_nodes && piece_off && out && ((uintptr_t)out & 15) == 0,
                "seq_emit: walk_nodes, piece_off and a 16-byte aligned out must not be null when there are bases to write");
  GNM_CHECK_ARG(packed_bytes == 0 || (packed && ((uintptr_t)packed & 3) == 0), "seq_emit: packed must be non-null and 4-byte aligned");
  SeqArgs a = {};
  a.s.packed = packed; a.s.base_off = base_off; a.s.length = length; a.s.nibbles = packed_bytes * 2; a.s.R = R; a.s.n = n;
  a.P = P; a.walk_nodes = walk_nodes; a.piece_off = const_cast<int64_t*>(piece_off); a.total = total; a.out = out;
  const int64_t nchunks = (total + kSeqChunkBases - 1) / kSeqChunkBases;
  hipLaunchKernelGGL(seq_emit_k, dim3(persistent_grid(nchunks, 1, 8)), dim3(kBlock), 0, (hipStream_t)stream, a);
  GNM_LAUNCH_CHECK("seq_emit");
  return 0;
}
