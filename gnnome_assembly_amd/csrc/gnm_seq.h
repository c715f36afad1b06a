// Contig sequences (include/gnm.h, "contig sequences"): what one lane of gnm_seq_emit does for its 16 output bases, and the piece
// length of one walk position, as plain C++ that compiles for the host as well as for the device (csrc/gnm_seq.hip is the only
// user in the library; a host program can include this file alone to run the same arithmetic without a GPU).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GNM_SEQ_FN __host__ __device__ __forceinline__
#else
#define GNM_SEQ_FN inline
#endif

namespace gnm {

constexpr int kSeqLaneBases = 16;                  // bases per lane and per 16-byte store
constexpr int kSeqChunkBases = 256 * kSeqLaneBases;  // output bases one workgroup (256 lanes) owns at a time

struct SeqStore {            // the packed + strands: 4 bits per base, BAM code, low nibble first
  const uint8_t* packed;     // [nibbles / 2] bytes; nibbles is a multiple of 32, so the array is whole 16-byte groups
  const int64_t* base_off;   // [R] nibble index of read r's first base
  const int64_t* length;     // [R] bases of read r
  int64_t nibbles, R, n;     // n: nodes of the graph; node v is read v >> 1, reversed and complemented when v is odd
};

#ifdef GNM_CHECK_ARG         // inside the library (gnm_common.h came first): the store's part of an entry point's argument check
inline int seq_store_check(const char* what, int64_t n, int64_t R, const int64_t* base_off, const int64_t* length, int64_t packed_bytes) {
  GNM_CHECK_ARG(n >= 0 && R >= 0 && n < INT32_MAX && R < INT32_MAX, "%s: n = %lld, R = %lld: expected 0 <= n, R < 2^31 - 1", what,
                (long long)n, (long long)R);
  GNM_CHECK_ARG(packed_bytes >= 0 && packed_bytes % 16 == 0 && packed_bytes <= (INT64_MAX >> 2),
                "%s: packed_bytes = %lld: the store is whole 16-byte groups", what, (long long)packed_bytes);
  GNM_CHECK_ARG(R == 0 || (base_off && length), "%s: base_off and length must not be null when R > 0", what);
  return 0;
}
#endif

struct SeqSrc {              // where the bases of one piece come from
  int64_t first, len;        // nibble index of the read's first base, the read's length
  int rev, ok;               // ok == 0: the node does not name a read that lies inside the store; nothing is read through it
};

GNM_SEQ_FN SeqSrc seq_src_(const SeqStore& s, int32_t v) {
  SeqSrc r = {0, 0, v & 1, 0};
  if (v < 0 || (int64_t)v >= s.n || (int64_t)(v >> 1) >= s.R) return r;
  r.first = s.base_off[v >> 1];
  r.len = s.length[v >> 1];
  r.ok = r.first >= 0 && r.len >= 0 && r.first <= s.nibbles && r.len <= s.nibbles - r.first;
  return r;
}

// All 64 bits in reverse order.  On 16 packed bases this is the reverse complement: the nibbles change ends, and the four
// bits of a code (A=1 C=2 G=4 T=8, an ambiguity code the OR of its bases) reversed are the code of the complement.
GNM_SEQ_FN uint64_t seq_brev64_(uint64_t x) {
  x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
  x = ((x >> 8) & 0x00ff00ff00ff00ffull) | ((x & 0x00ff00ff00ff00ffull) << 8);
  x = ((x >> 16) & 0x0000ffff0000ffffull) | ((x & 0x0000ffff0000ffffull) << 16);
  return (x >> 32) | (x << 32);
}
GNM_SEQ_FN unsigned seq_brev4_(unsigned c) { return ((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3); }

// Nibbles [w, w + 16) of the store, nibble w + i in bits 4 i .. 4 i + 3: three aligned 32-bit words funnel-shifted by the byte
// offset and, for an odd w, one more nibble.  The caller has checked 0 <= w and w + 16 <= nibbles; the third word is only needed
// for a non-zero shift and is clamped to the last word of the store.
GNM_SEQ_FN uint64_t seq_window_(const SeqStore& s, int64_t w) {
  const uint32_t* words = reinterpret_cast<const uint32_t*>(s.packed);
  const int64_t b0 = w >> 1, wi = b0 >> 2, last = (s.nibbles >> 3) - 1;
  const uint32_t w0 = words[wi], w1 = words[wi + 1 <= last ? wi + 1 : last], w2 = words[wi + 2 <= last ? wi + 2 : last];
  const unsigned sh = (unsigned)(b0 & 3) * 8u + (unsigned)(w & 1) * 4u;
  const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32);
  return sh ? (lo >> sh) | ((uint64_t)w2 << (64u - sh)) : lo;
}

// Eight codes (bits 0 .. 31 of x) as eight ASCII letters of "=ACMGRSVTWYHKDBN", first base in the low byte.
GNM_SEQ_FN uint64_t seq_ascii8_(uint32_t x) {
  constexpr uint64_t kLo = 0x565352474d43413dull;   // "=ACMGRSV", '=' in the low byte
  constexpr uint64_t kHi = 0x4e42444b48595754ull;   // "TWYHKDBN"
  uint64_t out = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) {
    const unsigned c = (x >> (4 * i)) & 15u;
    out |= (((c & 8u ? kHi : kLo) >> ((c & 7u) * 8u)) & 0xffull) << (8 * i);
  }
  return out;
}

// The largest p in [lo, hi] with off[p] <= g, given off[lo] <= g: the piece that holds output base g is the LAST one that
// starts at or before it -- the empty pieces in front of it start at the same offset and end there.
GNM_SEQ_FN int64_t seq_find_(const int64_t* off, int64_t lo, int64_t hi, int64_t g) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The same answer from a starting piece that is expected to be close: doubling steps forward, then the search in between.
GNM_SEQ_FN int64_t seq_gallop_(const int64_t* off, int64_t lo, int64_t last, int64_t g) {
  int64_t step = 1;
  while (lo + step <= last && off[lo + step] <= g) {
    lo += step;
    step <<= 1;
  }
  return seq_find_(off, lo, lo + step - 1 < last ? lo + step - 1 : last, g);
}

// The 16 output bytes of bases [g0, g0 + 16), g0 < total a multiple of 16.  [lo, hi]: the pieces of the workgroup's chunk
// (off[lo] <= g0, the last base of the chunk lies in piece hi).  Bytes of bases at and past `total` are 0.
GNM_SEQ_FN void seq_lane_(const SeqStore& s, const int32_t* walk_nodes, const int64_t* off, int64_t lo, int64_t hi, int64_t g0,
                          int64_t total, uint64_t out[2]) {
  int64_t p = seq_find_(off, lo, hi, g0);
  int64_t ps = off[p], pe = off[p + 1];
  SeqSrc src = seq_src_(s, walk_nodes[p]);
  uint64_t x = 0;
  int valid = kSeqLaneBases;
  if (g0 + kSeqLaneBases <= pe) {                        // fast path: one piece, one window of the store
    const int64_t t = g0 - ps;
    const int64_t w = src.rev ? src.first + src.len - kSeqLaneBases - t : src.first + t;
    if (src.ok && t >= 0 && w >= src.first && w + kSeqLaneBases <= src.first + src.len) x = seq_window_(s, w);
    if (src.rev) x = seq_brev64_(x);
  } else {                                               // a piece ends inside these 16 bases: base by base
    valid = 0;
    for (int i = 0; i < kSeqLaneBases; ++i) {
      const int64_t g = g0 + i;
      if (g >= total) break;
      while (g >= pe && p < hi) {                        // any number of pieces may end here, empty ones included
        ++p;
        ps = pe;
        pe = off[p + 1];
        src = seq_src_(s, walk_nodes[p]);
      }
      if (g >= pe) break;
      const int64_t t = g - ps;
      unsigned c = 0;
      if (src.ok && t >= 0 && t < src.len) {
        const int64_t k = src.rev ? src.first + src.len - 1 - t : src.first + t;
        c = (s.packed[k >> 1] >> ((unsigned)(k & 1) * 4u)) & 15u;
        if (src.rev) c = seq_brev4_(c);
      }
      x |= (uint64_t)c << (4 * i);
      valid = i + 1;
    }
  }
  out[0] = seq_ascii8_((uint32_t)x);
  out[1] = seq_ascii8_((uint32_t)(x >> 32));
  if (valid < 8) {
    out[0] = valid ? out[0] & (~0ull >> (64 - 8 * valid)) : 0;
    out[1] = 0;
  } else if (valid < 16) {
    out[1] = valid > 8 ? out[1] & (~0ull >> (64 - 8 * (valid - 8))) : 0;
  }
}

// What one walk position contributes.  flags: 1 clamped, 2 reverse, 4 invalid.
// contig_ptr [C+1], walk_nodes / walk_edges [P], prefix_length [E]; p < P.
GNM_SEQ_FN int64_t seq_piece_len_(const SeqStore& s, int64_t C, int64_t P, int64_t E, const int32_t* contig_ptr,
                                  const int32_t* walk_nodes, const int32_t* walk_edges, const int64_t* prefix_length, int64_t p,
                                  unsigned& flags) {
  flags = 4u;
  if (C <= 0) return 0;
  int64_t lo = 0, hi = C - 1;                            // the contig of p: the last one that starts at or before it
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if ((int64_t)contig_ptr[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  const int64_t end = contig_ptr[lo + 1];
  if ((int64_t)contig_ptr[lo] > p || end <= p || end > P) return 0;
  const SeqSrc src = seq_src_(s, walk_nodes[p]);
  if (!src.ok) return 0;
  int64_t k = src.len;
  unsigned f = src.rev ? 2u : 0u;
  if (p + 1 < end) {                                     // an inner position: the prefix of the edge to the next node
    const int32_t e = walk_edges[p + 1];
    if (e < 0 || (int64_t)e >= E) return 0;
    k = prefix_length[e];
    if (k < 0 || k > src.len) {
      k = k < 0 ? 0 : src.len;
      f |= 1u;
    }
  }
  flags = f;
  return k;
}

}  // namespace gnm
