// Overlap graph from the reads (include/gnm.h, "overlap graph"): the arithmetic of the three stages -- minimizer sketch, seed hits,
// chains -- as plain C++ that compiles for the host as well as for the device, like gnm_align.h.  csrc/gnm_overlap.hip holds the
// kernels and the host entries; both call these routines, so the host entries compute what the kernels compute.  Integers only.
#pragma once
#include <stdint.h>

#include "gnm_seq.h"

namespace gnm {

constexpr int kSketchTile = 512;                                  // k-mer positions one workgroup owns at a time
constexpr int kSketchMinK = 8, kSketchMaxK = 31, kSketchMaxW = 64;
constexpr int kSketchHashes = kSketchTile + 2 * (kSketchMaxW - 1);  // the tile and w - 1 positions on each side
constexpr int kSketchBases = kSketchHashes + kSketchMaxK - 1;     // ... and the k - 1 bases behind the last of them
constexpr int kSketchWords = (kSketchBases + 31) / 32 + 1;        // words of 32 bases; one more, so word j + 1 always exists
constexpr int kOverlapMaxOcc = 4096;

enum { kOvlReads = 0, kOvlKmersValid, kOvlMinimizers, kOvlRuns, kOvlSkippedRuns, kOvlSkippedEntries, kOvlHits, kOvlSameRead,
       kOvlGroups, kOvlFewHits, kOvlShort, kOvlContainedGroups, kOvlLinks, kOvlCalls, kOvlWords };

// The murmur3 64-bit finaliser: a bijection of the 64-bit words.
GNM_SEQ_FN uint64_t ovl_fmix64_(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// ---- stage 1: sketch ---------------------------------------------------------------------------------------------------------
// The read a sketch tile belongs to and the tile's ranges, all in bases / k-mer positions of the read's + strand.
struct SketchGeom {
  int64_t first, len, nk;    // nibble index of the first base, bases, k-mers (0: the read gives nothing)
  int W;                     // min(w, nk)
  int64_t p0, p1, h0, h1;    // positions [p0, p1) are the tile's own; hashes are formed for [h0, h1), from bases [h0, h1 + k - 1)
};

// k-mers of read r; 0 for a read outside the store or of 2^31 - 1 bases or more (nothing is read through it).
GNM_SEQ_FN int64_t sk_read_kmers_(const SeqStore& s, int64_t r, int k, int64_t& first, int64_t& len) {
  first = len = 0;
  if (r < 0 || r >= s.R) return 0;
  const int64_t f = s.base_off[r], l = s.length[r];
  if (f < 0 || l < 0 || l >= INT32_MAX || f > s.nibbles || l > s.nibbles - f) return 0;
  first = f;
  len = l;
  return l - k + 1 > 0 ? l - k + 1 : 0;
}
GNM_SEQ_FN int64_t sk_read_tiles_(const SeqStore& s, int64_t r, int k) {
  int64_t f, l;
  return (sk_read_kmers_(s, r, k, f, l) + kSketchTile - 1) / kSketchTile;
}
GNM_SEQ_FN SketchGeom sk_geom_(const SeqStore& s, int64_t r, int64_t ti, int k, int w) {
  SketchGeom g = {};
  g.nk = sk_read_kmers_(s, r, k, g.first, g.len);
  g.W = (int)((int64_t)w < g.nk ? w : g.nk);
  g.p0 = ti * kSketchTile < g.nk ? ti * kSketchTile : g.nk;
  g.p1 = g.p0 + kSketchTile < g.nk ? g.p0 + kSketchTile : g.nk;
  g.h0 = g.p0 - (g.W - 1) > 0 ? g.p0 - (g.W - 1) : 0;
  g.h1 = g.p1 + (g.W - 1) < g.nk ? g.p1 + (g.W - 1) : g.nk;
  if (g.p0 >= g.p1) g.h0 = g.h1 = g.p0;
  return g;
}

// Nibbles [w, w + 16) of the store, 0 for those past its end; w >= 0.
GNM_SEQ_FN uint64_t sk_load16_(const SeqStore& s, int64_t w) {
  if (w + 16 <= s.nibbles) return seq_window_(s, w);
  uint64_t x = 0;
  for (int i = 0; i < 16 && w + i < s.nibbles; ++i)
    x |= (uint64_t)((s.packed[(w + i) >> 1] >> ((unsigned)((w + i) & 1) * 4u)) & 15u) << (4 * i);
  return x;
}

// Bases [g0, g0 + 32) of the read as three words.  A, C, G, T (codes 1, 2, 4, 8) are 0 .. 3; base i of the word lies
//   in fw at bits 62 - 2 i (first base most significant: a k-mer read from it is f),
//   in rc as 3 - code at bits 2 i (first base least significant: a k-mer read from it is the reverse complement r),
//   in inv as bit i, set for every other code and for bases at and past the read's end.
GNM_SEQ_FN void sk_word_(const SeqStore& s, int64_t first, int64_t len, int64_t g0, uint64_t& fw, uint64_t& rc, uint32_t& inv) {
  fw = rc = 0;
  inv = 0xffffffffu;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int half = 0; half < 2; ++half) {
    const int64_t g = g0 + 16 * half;
    if (g >= len) continue;
    const uint64_t x = sk_load16_(s, first + g);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 16; ++i) {
      const unsigned c = (unsigned)(x >> (4 * i)) & 15u;
      const bool ok = g + i < len && c != 0u && (c & (c - 1u)) == 0u;
      const uint64_t c2 = ((((c >> 2) | (c >> 3)) & 1u) << 1) | (((c >> 1) | (c >> 3)) & 1u);
      const int b = 16 * half + i;
      if (ok) {
        fw |= c2 << (62 - 2 * b);
        rc |= (3ull - c2) << (2 * b);
        inv &= ~(1u << b);
      }
    }
  }
}

// The k-mer at base offset o of the word arrays: two words and a shift each.  flag: bit 0 valid (no other code inside, f != r),
// bit 1 the strand bit s = (r < f); h = fmix64(min(f, r)).  Word o / 32 + 1 exists (kSketchWords).
template <class W64, class W32>
GNM_SEQ_FN void sk_hash_(const W64* FW, const W64* RC, const W32* INV, int o, int k, uint64_t& h, unsigned& flag) {
  const int j = o >> 5, sh = (o & 31) * 2;
  const uint64_t f0 = FW[j], f1 = FW[j + 1], r0 = RC[j], r1 = RC[j + 1];
  const uint64_t f = (sh ? (f0 << sh) | (f1 >> (64 - sh)) : f0) >> (64 - 2 * k);
  const uint64_t r = (sh ? (r0 >> sh) | (r1 << (64 - sh)) : r0) & ((1ull << (2 * k)) - 1ull);
  const uint64_t iv = ((((uint64_t)INV[j + 1] << 32) | (uint64_t)INV[j]) >> (o & 31)) & ((1ull << k) - 1ull);
  flag = (iv == 0ull && f != r ? 1u : 0u) | (r < f ? 2u : 0u);
  h = ovl_fmix64_(r < f ? r : f);
}

// Is entry i of the tile's n hashes a minimizer?  Some window of W positions holds it and no smaller valid key (h, position):
// with L (R) the entries right before (behind) it that do not beat it, counted up to W - 1 and the end of the read, that is
// L + R >= W - 1.  An earlier position beats with h <=, a later one with h <.  The array ends W - 1 entries from the tile's own
// positions or at the read's end, so its ends are the right caps.
template <class W64, class W8>
GNM_SEQ_FN bool sk_selected_(const W64* H, const W8* F, int i, int n, int W) {
  if (!(F[i] & 1)) return false;
  const uint64_t h = H[i];
  int free_ = 0;
  for (int q = i - 1; q >= 0 && free_ < W - 1; --q) {
    if ((F[q] & 1) && H[q] <= h) break;
    ++free_;
  }
  for (int q = i + 1; q < n && free_ < W - 1; ++q) {
    if ((F[q] & 1) && H[q] < h) break;
    ++free_;
  }
  return free_ >= W - 1;
}

// ---- stage 2: seed hits --------------------------------------------------------------------------------------------------------
// Entry i of the M entries sorted by hash: the earlier entries of its run (`back`), whether it heads the run, whether the run is
// longer than max_occ (then the entry has no partners).  At most max_occ + 1 entries are looked at.
GNM_SEQ_FN void ovl_run_(const int64_t* hash, int64_t M, int64_t i, int max_occ, int& back, bool& skipped) {
  const int64_t h = hash[i];
  back = 0;
  while (back < max_occ && i - back - 1 >= 0 && hash[i - back - 1] == h) ++back;
  skipped = back >= max_occ;
  if (!skipped) {
    int fwd = 0;
    while (back + 1 + fwd <= max_occ && i + fwd + 1 < M && hash[i + fwd + 1] == h) ++fwd;
    skipped = back + 1 + fwd > max_occ;
  }
}

// The hit of entries j < i of one run, reads different: key = a << 32 | b << 1 | rel and diag (include/gnm.h).
GNM_SEQ_FN void ovl_hit_(const int32_t* read, const int32_t* pos, const uint8_t* strand, const int64_t* length, int64_t R, int k,
                         int64_t j, int64_t i, int64_t& key, int32_t& diag) {
  const bool swap = read[j] > read[i];
  const int64_t ea = swap ? i : j, eb = swap ? j : i;
  const int64_t a = read[ea], b = read[eb];
  const int rel = (strand[ea] ^ strand[eb]) & 1;
  const int64_t lb = b >= 0 && b < R ? length[b] : 0;
  const int64_t q = rel ? lb - k - (int64_t)pos[eb] : (int64_t)pos[eb];
  key = (int64_t)(((uint64_t)a << 32) | ((uint64_t)(uint32_t)b << 1) | (uint64_t)rel);
  diag = (int32_t)((int64_t)pos[ea] - q);
}

// Entry i's hits as the LOWER read: a hit's `a` is the smaller of its two read ids whichever entry comes later, so these are the
// entries of i's run, before or behind it, whose read id is larger.  In a sketch sorted stably by hash a run is ordered by read and
// the count is the run's end minus the end of i's read in it; it is counted entry by entry here (the run has at most max_occ entries
// and ovl_run_ has walked it already), which needs no order inside the run.  back, skipped: as ovl_run_; same: the earlier entries
// of i's own read (what the hit pass counts as same_read).
GNM_SEQ_FN int64_t ovl_lower_(const int64_t* hash, const int32_t* read, int64_t M, int64_t i, int max_occ, int& back, bool& skipped,
                              int64_t& same) {
  ovl_run_(hash, M, i, max_occ, back, skipped);
  same = 0;
  if (skipped) return 0;
  const int64_t h = hash[i];
  const int32_t r = read[i];
  int64_t m = 0;
  for (int64_t j = i - back; j < i; ++j) {
    m += read[j] > r ? 1 : 0;
    same += read[j] == r ? 1 : 0;
  }
  for (int64_t j = i + 1; j < M && hash[j] == h; ++j) m += read[j] > r ? 1 : 0;   // not skipped: the run ends within max_occ entries
  return m;
}

// Does the hit of two entries of reads rj, ri belong to the read range [a_lo, a_hi)?  Its `a` is the smaller id.
GNM_SEQ_FN bool ovl_in_range_(int32_t rj, int32_t ri, int64_t a_lo, int64_t a_hi) {
  const int64_t a = rj < ri ? rj : ri;
  return a >= a_lo && a < a_hi;
}

// ---- stage 3: chains -----------------------------------------------------------------------------------------------------------
enum { kChainFewHits = 0, kChainForward, kChainBackward, kChainContained, kChainShort };

struct ChainOut {
  int kind, hits;
  int32_t src0, dst0, src1, dst1;      // the edge and its twin (forward, backward)
  int64_t D, ov, prefix0, prefix1;
  int64_t contained;                   // the contained read (kChainContained)
};

// The group of g hits at diag[i0 .. i0 + g), ascending, of reads a < b (lengths la, lb) and relative strand rel.
GNM_SEQ_FN ChainOut ovl_chain_(const int32_t* diag, int64_t i0, int64_t g, int64_t band, int64_t min_hits, int64_t min_overlap,
                               int64_t a, int64_t b, int rel, int64_t la, int64_t lb) {
  ChainOut c = {};
  int64_t j = i0, best = 0, besti = i0;
  for (int64_t i = i0; i < i0 + g; ++i) {                // c_i = #{j >= i : d_j <= d_i + band}: j only moves forward
    if (j < i) j = i;
    const int64_t top = (int64_t)diag[i] + band;
    while (j < i0 + g && (int64_t)diag[j] <= top) ++j;
    if (j - i > best) {
      best = j - i;
      besti = i;
    }
  }
  c.hits = (int)(best < INT32_MAX ? best : INT32_MAX);
  c.kind = kChainFewHits;
  if (best < min_hits || best < 1) return c;
  const int64_t D = diag[besti + (best - 1) / 2];
  const int32_t na = (int32_t)(2 * a), nb = (int32_t)(2 * b + rel);
  c.D = D;
  if (D > 0 && D + lb > la) {
    c.kind = kChainForward;
    c.ov = la - D;
    c.src0 = na; c.dst0 = nb; c.prefix0 = D;
    c.src1 = nb ^ 1; c.dst1 = na + 1; c.prefix1 = lb - c.ov;
  } else if (D < 0 && D + lb < la) {
    c.kind = kChainBackward;
    c.ov = lb + D;
    c.src0 = nb; c.dst0 = na; c.prefix0 = -D;
    c.src1 = na + 1; c.dst1 = nb ^ 1; c.prefix1 = la - c.ov;
  } else {
    c.kind = kChainContained;
    c.contained = D >= 0 && D + lb <= la ? b : a;
    return c;
  }
  if (c.ov < min_overlap) c.kind = kChainShort;
  return c;
}

}  // namespace gnm
