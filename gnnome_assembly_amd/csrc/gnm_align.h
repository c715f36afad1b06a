// Overlap identity (include/gnm.h, "overlap alignment"): the banded edit distance of ONE edge as plain C++ that compiles for the
// host as well as for the device (csrc/gnm_align.hip is the only user in the library; a host program can include this file
// alone to run the same arithmetic without a GPU).  Integers only, except for the one fp32 division of the similarity.
//
// Edge k = (a -> c), p = prefix_length[k] clamped to [0, la]:  Q = bases [p, la) of a's strand (m of them),
// T = bases [0, n) of c's strand, n = min(lc, m + K);  dist = min over 0 <= i <= n of Levenshtein(Q, T[0:i]), K + 1 when that
// exceeds K.  D[i][j] = Levenshtein(T[0:i], Q[0:j]); the answer is the smallest entry of COLUMN m.
//
// The routine is Hyyro's diagonal-band form of Myers' bit-vector recurrence.  The columns are the bases of Q; bit k of the
// band in column j is row (prefix of T) i = j - K + k, k < 64 NW: K diagonals above the main one and 64 NW - 1 - K >= K below
// it, so the band holds every |i - j| <= K and the NW words are used whole -- no mask at the band's end.  The band moves down one
// row per column, which cancels the << 1 of the horizontal deltas; the diagonal vector is shifted >> 1 instead:
//   D0 = (((Eq & Pv) + Pv) ^ Pv) | Eq | Mv        Ph = Mv | ~(D0 | Pv)        Mh = Pv & D0
//   Pv' = Mh | ~((D0 >> 1) | Ph)                   Mv' = Ph & (D0 >> 1)
// Pv, Mv are stored aligned to the NEXT column's rows.  No carry enters bit 0 and 0 is shifted into the top of D0 >> 1: the cell
// above the band's first row and the cell left of its last row count as +infinity, which is Ukkonen's cut -- exact for every
// distance <= K, and never below the true distance.  Rows i <= 0 continue the matrix upward with D[i][j] = j - i (Eq = 0, Mv = 1
// in column 0), which makes D[0][j] = j come out of the recurrence; rows i > n never match and lie below everything that is read.
// The value of the band's LAST cell is carried along its diagonal (+1 where its D0 bit is 0); after column m the vertical deltas
// lead from it up to the rows max(0, m - K) .. n, and dist is the smallest value met there.
// Eq comes from a sliding window over T kept as four bit planes of the 4-bit codes and one plane of "no base here": the window
// is filled 16 packed bases at a time (the planes of 16 nibbles by four mask-and-shift steps), moves one bit per column, and
// Eq = ~((P0 ^ q0) | (P1 ^ q1) | (P2 ^ q2) | (P3 ^ q3) | none): two codes match when all four bits agree, N only with N.
// Every array below has NW entries and is indexed by unrolled loops only: all of it lives in registers.
#pragma once
#include "gnm_seq.h"

namespace gnm {

constexpr int kAlignMaxErrors = 255;             // 2 K + 1 <= 512 bits = 8 words
enum { kAlnEdges = 0, kAlnAligned, kAlnExceeded, kAlnEmpty, kAlnClamped, kAlnInvalid, kAlnCells, kAlnCalls };
enum : unsigned { kAlnFlagClamped = 1u, kAlnFlagInvalid = 2u, kAlnFlagEmpty = 4u, kAlnFlagExceeded = 8u };

GNM_SEQ_FN int align_words_(int K) { return K <= 31 ? 1 : K <= 63 ? 2 : K <= 127 ? 4 : 8; }

// Bases [t0, t0 + 16) of src's strand, base t0 + i in bits 4 i .. 4 i + 3; bit i of `valid`: 0 <= t0 + i < limit (limit <= src.len).
// A base outside [0, src.len) reads as 0 and nothing is loaded for it.
GNM_SEQ_FN uint64_t align_fetch16_(const SeqStore& s, const SeqSrc& src, int64_t t0, int64_t limit, unsigned& valid) {
  valid = 0u;
  if (t0 >= src.len || t0 <= -16) return 0;
  const int64_t left = limit - t0;
  if (t0 >= 0 && t0 + 16 <= src.len) {                   // one window of the store
    valid = left >= 16 ? 0xffffu : left > 0 ? (1u << (unsigned)left) - 1u : 0u;
    const uint64_t x = seq_window_(s, src.rev ? src.first + src.len - 16 - t0 : src.first + t0);
    return src.rev ? seq_brev64_(x) : x;
  }
  uint64_t x = 0;
  for (int i = 0; i < 16; ++i) {
    const int64_t t = t0 + i;
    if (t < 0 || t >= src.len) continue;
    const int64_t k = src.rev ? src.first + src.len - 1 - t : src.first + t;
    unsigned c = (s.packed[k >> 1] >> ((unsigned)(k & 1) * 4u)) & 15u;
    if (src.rev) c = seq_brev4_(c);
    x |= (uint64_t)c << (4 * i);
    if (t < limit) valid |= 1u << i;
  }
  return x;
}

// Bit b of each of the 16 codes in x, code i's in bit i.
GNM_SEQ_FN uint64_t align_plane16_(uint64_t x, int b) {
  uint64_t y = (x >> b) & 0x1111111111111111ull;
  y = (y | (y >> 3)) & 0x0303030303030303ull;
  y = (y | (y >> 6)) & 0x000f000f000f000full;
  y = (y | (y >> 12)) & 0x000000ff000000ffull;
  return (y | (y >> 24)) & 0xffffull;
}

#if defined(__HIPCC__)
#define GNM_ALIGN_UNROLL _Pragma("unroll")
#else
#define GNM_ALIGN_UNROLL
#endif

// The smallest D[i][m] over the rows max(0, m - K) <= i <= n of the band, or INT64_MAX when the band holds none of them.
// q: the source of Q (bases [p, p + m) of its strand, p + m == q.len), t: the source of T, n <= t.len, n <= m + K, m > 0.
template <int NW>
GNM_SEQ_FN int64_t align_band_(const SeqStore& s, const SeqSrc& q, int64_t p, int64_t m, const SeqSrc& t, int64_t n, int K) {
  constexpr int kBits = 64 * NW;
  uint64_t Pv[NW], Mv[NW], D0[NW], P0[NW], P1[NW], P2[NW], P3[NW], none[NW];
  GNM_ALIGN_UNROLL
  for (int w = 0; w < NW; ++w) {                         // column 0, aligned to column 1: bit k is row 1 - K + k
    const int below = K - 64 * w;                        // bits of this word whose row is <= 0
    Mv[w] = below >= 64 ? ~0ull : below > 0 ? (1ull << below) - 1ull : 0ull;
    Pv[w] = ~Mv[w];
    P0[w] = P1[w] = P2[w] = P3[w] = none[w] = 0;
    GNM_ALIGN_UNROLL
    for (int g = 0; g < 4; ++g) {
      unsigned valid;
      const uint64_t x = align_fetch16_(s, t, (int64_t)(64 * w + 16 * g) - K, n, valid);
      P0[w] |= align_plane16_(x, 0) << (16 * g);
      P1[w] |= align_plane16_(x, 1) << (16 * g);
      P2[w] |= align_plane16_(x, 2) << (16 * g);
      P3[w] |= align_plane16_(x, 3) << (16 * g);
      none[w] |= (uint64_t)(~valid & 0xffffu) << (16 * g);
    }
  }
  int64_t score = kBits - 1 - K;                         // D of the band's last cell: row 64 NW - 1 - K of column 0
  uint64_t qwin = 0, twin = 0;
  unsigned tvalid = 0u;
  for (int64_t j = 0; j < m; ++j) {                      // column j + 1
    const unsigned jj = (unsigned)j & 15u;
    if (jj == 0u) {
      unsigned qvalid;
      qwin = align_fetch16_(s, q, p + j, q.len, qvalid);
      twin = align_fetch16_(s, t, j + (kBits - K), n, tvalid);   // the rows that enter the band after columns j + 1 .. j + 16
    }
    const unsigned qc = (unsigned)(qwin >> (4u * jj)) & 15u;
    const uint64_t q0 = 0ull - (uint64_t)(qc & 1u), q1 = 0ull - (uint64_t)((qc >> 1) & 1u);
    const uint64_t q2 = 0ull - (uint64_t)((qc >> 2) & 1u), q3 = 0ull - (uint64_t)((qc >> 3) & 1u);
    uint64_t carry = 0;
    GNM_ALIGN_UNROLL
    for (int w = 0; w < NW; ++w) {
      const uint64_t eq = ~((P0[w] ^ q0) | (P1[w] ^ q1) | (P2[w] ^ q2) | (P3[w] ^ q3) | none[w]);
      const uint64_t x = eq & Pv[w];
      const uint64_t s1 = x + Pv[w];
      const uint64_t s2 = s1 + carry;
      carry = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
      D0[w] = (s2 ^ Pv[w]) | eq | Mv[w];
    }
    score += 1 - (int64_t)(D0[NW - 1] >> 63);
    const unsigned tc = (unsigned)(twin >> (4u * jj)) & 15u;
    const uint64_t in_none = (uint64_t)(~(tvalid >> jj) & 1u);
    GNM_ALIGN_UNROLL
    for (int w = 0; w < NW; ++w) {
      const uint64_t ph = Mv[w] | ~(D0[w] | Pv[w]);
      const uint64_t mh = Pv[w] & D0[w];
      const uint64_t d0s = (D0[w] >> 1) | (w + 1 < NW ? D0[w + 1 < NW ? w + 1 : w] << 63 : 0ull);
      Pv[w] = mh | ~(d0s | ph);
      Mv[w] = ph & d0s;
      const bool top = w + 1 == NW;                      // the window over T moves down one row
      const int u = top ? w : w + 1;
      P0[w] = (P0[w] >> 1) | ((top ? (uint64_t)(tc & 1u) : P0[u]) << 63);
      P1[w] = (P1[w] >> 1) | ((top ? (uint64_t)((tc >> 1) & 1u) : P1[u]) << 63);
      P2[w] = (P2[w] >> 1) | ((top ? (uint64_t)((tc >> 2) & 1u) : P2[u]) << 63);
      P3[w] = (P3[w] >> 1) | ((top ? (uint64_t)((tc >> 3) & 1u) : P3[u]) << 63);
      none[w] = (none[w] >> 1) | ((top ? in_none : none[u]) << 63);
    }
  }
  // Column m.  Band cell k is row m - K + k; bit k of Pv / Mv is the step from cell k to cell k + 1; `score` is cell 64 NW - 1.
  const int64_t klo = m < K ? K - m : 0, khi = n - m + K;   // rows 0 <= i <= n; khi <= 2 K < 64 NW
  int64_t best = INT64_MAX, val = score;
  GNM_ALIGN_UNROLL
  for (int w = NW - 1; w >= 0; --w) {
    const uint64_t pv = Pv[w], mv = Mv[w];
    for (int b = 63; b >= 0; --b) {
      const int k = 64 * w + b;
      if (k != kBits - 1) val -= (int64_t)((pv >> b) & 1ull) - (int64_t)((mv >> b) & 1ull);
      if (k >= klo && k <= khi && val < best) best = val;
    }
  }
  return best;
}

struct AlignEdge {
  int32_t dist;              // -1: invalid
  int64_t m, cells;          // cells: m * |T| of an aligned edge, else 0
  float similarity;
  unsigned flags;
};

// One edge.  K in [0, kAlignMaxErrors], NW >= align_words_(K).
template <int NW>
GNM_SEQ_FN AlignEdge align_edge_(const SeqStore& s, int32_t a, int32_t c, int64_t p, int K) {
  AlignEdge r = {-1, 0, 0, 0.f, kAlnFlagInvalid};
  const SeqSrc q = seq_src_(s, a), t = seq_src_(s, c);
  if (!q.ok || !t.ok) return r;
  r.flags = 0u;
  if (p < 0 || p > q.len) {
    p = p < 0 ? 0 : q.len;
    r.flags |= kAlnFlagClamped;
  }
  const int64_t m = q.len - p;
  r.m = m;
  r.dist = 0;
  if (m == 0) {
    r.flags |= kAlnFlagEmpty;
    return r;
  }
  const int64_t n = t.len < m + K ? t.len : m + K;
  const int64_t best = align_band_<NW>(s, q, p, m, t, n, K);
  if (best > K) {
    r.dist = K + 1;
    r.flags |= kAlnFlagExceeded;
  } else {
    r.dist = (int32_t)best;
    r.cells = m * n;
  }
  const float sim = 1.0f - (float)r.dist / (float)m;
  r.similarity = sim > 0.f ? sim : 0.f;
  return r;
}

}  // namespace gnm
