// Stand-alone host check of csrc/gnm_overlap.h (no GPU, no Python): random reads -- with N's, of every length around k, w and the
// tile size, the last one ending the store exactly -- through the tile routines against a brute-force sketch, and random runs and
// groups through the seed-hit (with the hits per lower read and the read-range test of the chunked route) and chain routines, meant to be built with a host sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gnnome_assembly_amd/csrc \
//       tools/overlap_host_check.cpp -o overlap_host_check && ./overlap_host_check
// Exit status 0 and "ok" when every case agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gnm_overlap.h"

using namespace gnm;

static const char kLetters[] = "=ACMGRSVTWYHKDBN";
static const char kBases[] = "ACGT";

struct Store {
  std::vector<uint8_t> packed;           // exactly the store's bytes: a read past its end is a heap overflow the sanitizer sees
  std::vector<int64_t> off, len;
  SeqStore view() const { return SeqStore{packed.data(), off.data(), len.data(), (int64_t)packed.size() * 2, (int64_t)off.size(), 2 * (int64_t)off.size()}; }
};

static Store pack(const std::vector<std::string>& reads) {
  Store s;
  std::vector<uint8_t> nib;
  for (const std::string& r : reads) {
    s.off.push_back((int64_t)nib.size());
    s.len.push_back((int64_t)r.size());
    for (char ch : r) nib.push_back((uint8_t)(strchr(kLetters, ch) - kLetters));
    while (nib.size() % 32) nib.push_back(0);
  }
  s.packed.resize(nib.size() / 2);
  for (size_t i = 0; i < s.packed.size(); ++i) s.packed[i] = (uint8_t)(nib[2 * i] | (nib[2 * i + 1] << 4));
  return s;
}

struct Entry { uint64_t h; int64_t p; int s; bool operator==(const Entry& o) const { return h == o.h && p == o.p && s == o.s; } };

static bool kmer(const std::string& r, int64_t p, int k, uint64_t& h, int& s) {
  uint64_t f = 0, c = 0;
  for (int i = 0; i < k; ++i) {
    const char* at = strchr(kBases, r[p + i]);
    if (!at || !r[p + i]) return false;
    f = f * 4 + (uint64_t)(at - kBases);
    c |= (uint64_t)(3 - (at - kBases)) << (2 * i);
  }
  if (f == c) return false;
  s = c < f;
  h = ovl_fmix64_(c < f ? c : f);
  return true;
}

static std::vector<Entry> brute(const std::string& r, int k, int w) {
  const int64_t nk = (int64_t)r.size() - k + 1;
  std::vector<Entry> out;
  if (nk <= 0) return out;
  const int64_t W = std::min<int64_t>(w, nk);
  std::vector<char> chosen((size_t)nk, 0);
  for (int64_t j = 0; j + W <= nk; ++j) {
    int64_t best = -1;
    uint64_t bh = 0;
    for (int64_t p = j; p < j + W; ++p) {
      uint64_t h;
      int s;
      if (kmer(r, p, k, h, s) && (best < 0 || h < bh)) best = p, bh = h;
    }
    if (best >= 0) chosen[(size_t)best] = 1;
  }
  for (int64_t p = 0; p < nk; ++p)
    if (chosen[(size_t)p]) {
      Entry e{0, p, 0};
      kmer(r, p, k, e.h, e.s);
      out.push_back(e);
    }
  return out;
}

static std::vector<Entry> tiles(const SeqStore& s, int64_t r, int k, int w) {
  std::vector<Entry> out;
  for (int64_t ti = 0, n = sk_read_tiles_(s, r, k); ti < n; ++ti) {
    uint64_t FW[kSketchWords], RC[kSketchWords], H[kSketchHashes];
    uint32_t INV[kSketchWords];
    uint8_t F[kSketchHashes];
    const SketchGeom g = sk_geom_(s, r, ti, k, w);
    const int nh = (int)(g.h1 - g.h0), nw = nh > 0 ? (nh + k - 1 + 31) / 32 + 1 : 0;
    if (nh > kSketchHashes || nw > kSketchWords) abort();
    for (int j = 0; j < nw; ++j) sk_word_(s, g.first, g.len, g.h0 + 32 * (int64_t)j, FW[j], RC[j], INV[j]);
    for (int i = 0; i < nh; ++i) {
      unsigned f;
      sk_hash_(FW, RC, INV, i, k, H[i], f);
      F[i] = (uint8_t)f;
    }
    for (int i = (int)(g.p0 - g.h0); i < (int)(g.p1 - g.h0); ++i)
      if (sk_selected_(H, F, i, nh, g.W)) out.push_back(Entry{H[i], g.h0 + i, (F[i] >> 1) & 1});
  }
  return out;
}

int main() {
  std::mt19937_64 rng(7);
  int bad = 0;
  const int ks[] = {8, 15, 21, 31}, ws[] = {1, 5, 25, 64};
  for (int k : ks)
    for (int w : ws) {
      std::vector<std::string> reads;
      const int lens[] = {0, 1, k - 1, k, k + w - 2, k + w, 100, kSketchTile + k - 2, kSketchTile + k - 1, kSketchTile + k, 2 * kSketchTile + k + 40, 64};
      for (int len : lens) {
        std::string r((size_t)std::max(len, 0), 'A');
        for (char& ch : r) ch = rng() % 97 == 0 ? 'N' : "ACGT"[rng() % 4];
        reads.push_back(r);
      }
      reads.push_back(std::string(90, 'A'));                 // equal hashes: the position decides
      reads.push_back(std::string(64, 'C'));                 // the last read ends the store: no pad nibbles behind it
      const Store st = pack(reads);
      const SeqStore s = st.view();
      for (size_t r = 0; r < reads.size(); ++r)
        if (!(tiles(s, (int64_t)r, k, w) == brute(reads[r], k, w))) {
          printf("sketch differs: k %d w %d read %zu (%zu bases)\n", k, w, r, reads[r].size());
          ++bad;
        }
    }
  // seed hits and chains: random runs and groups; the routines must stay inside the arrays they are given
  for (int round = 0; round < 200; ++round) {
    const int64_t M = (int64_t)(rng() % 60), R = 6;
    std::vector<int64_t> hash((size_t)M), length((size_t)R);
    std::vector<int32_t> read((size_t)M), pos((size_t)M);
    std::vector<uint8_t> strand((size_t)M);
    for (auto& l : length) l = 100 + (int64_t)(rng() % 400);
    for (int64_t i = 0; i < M; ++i) {
      hash[(size_t)i] = (int64_t)(rng() % 5) - 2;
      read[(size_t)i] = (int32_t)(rng() % R);
      pos[(size_t)i] = (int32_t)(rng() % 80);
      strand[(size_t)i] = (uint8_t)(rng() % 2);
    }
    std::sort(hash.begin(), hash.end());
    const int occ = 1 + (int)(rng() % 12);
    std::vector<int64_t> key;
    std::vector<int32_t> diag;
    for (int64_t i = 0; i < M; ++i) {
      int back;
      bool skipped;
      ovl_run_(hash.data(), M, i, occ, back, skipped);
      int64_t lo = i, hi = i;
      while (lo > 0 && hash[(size_t)lo - 1] == hash[(size_t)i]) --lo;
      while (hi + 1 < M && hash[(size_t)hi + 1] == hash[(size_t)i]) ++hi;
      if (skipped != (hi - lo + 1 > occ) || (!skipped && back != i - lo)) {
        printf("run differs: round %d entry %lld\n", round, (long long)i);
        ++bad;
      }
      for (int64_t j = i - back; !skipped && j < i; ++j)
        if (read[(size_t)j] != read[(size_t)i]) {
          key.push_back(0);
          diag.push_back(0);
          ovl_hit_(read.data(), pos.data(), strand.data(), length.data(), R, 15, j, i, key.back(), diag.back());
        }
    }
    // the chunked route: every entry's hits as the lower read (the reads of a run are in no order here) and the range test
    int64_t lower_sum = 0, in_ranges = 0;
    const int64_t cut = (int64_t)(rng() % (R + 1));
    for (int64_t i = 0; i < M; ++i) {
      int back;
      bool skipped;
      int64_t same_read, want = 0, lo = i, hi = i;
      const int64_t got = ovl_lower_(hash.data(), read.data(), M, i, occ, back, skipped, same_read);
      while (lo > 0 && hash[(size_t)lo - 1] == hash[(size_t)i]) --lo;
      while (hi + 1 < M && hash[(size_t)hi + 1] == hash[(size_t)i]) ++hi;
      for (int64_t j = lo; j <= hi && hi - lo + 1 <= occ; ++j) want += read[(size_t)j] > read[(size_t)i];
      if (got != want) {
        printf("lower hits differ: round %d entry %lld\n", round, (long long)i);
        ++bad;
      }
      lower_sum += got;
      for (int64_t j = i - back; !skipped && j < i; ++j)
        if (read[(size_t)j] != read[(size_t)i])
          in_ranges += (ovl_in_range_(read[(size_t)j], read[(size_t)i], 0, cut) ? 1 : 0) + (ovl_in_range_(read[(size_t)j], read[(size_t)i], cut, R) ? 1 : 0);
    }
    if (lower_sum != (int64_t)key.size() || in_ranges != (int64_t)key.size()) {
      printf("lower hits or ranges do not add up: round %d\n", round);
      ++bad;
    }
    std::vector<size_t> o(key.size());
    for (size_t i = 0; i < o.size(); ++i) o[i] = i;
    std::sort(o.begin(), o.end(), [&](size_t x, size_t y) { return key[x] != key[y] ? key[x] < key[y] : diag[x] < diag[y]; });
    std::vector<int32_t> d;
    std::vector<int64_t> ks2;
    for (size_t i : o) d.push_back(diag[i]), ks2.push_back(key[i]);
    for (size_t i = 0; i < d.size();) {
      size_t e = i;
      while (e < d.size() && ks2[e] == ks2[i]) ++e;
      const int64_t a = (int64_t)((uint64_t)ks2[i] >> 32), b = (int64_t)(((uint64_t)ks2[i] & 0xffffffffull) >> 1);
      const int64_t band = (int64_t)(rng() % 40);
      const ChainOut c = ovl_chain_(d.data(), (int64_t)i, (int64_t)(e - i), band, 1, 0, a, b, (int)(ks2[i] & 1), length[(size_t)a], length[(size_t)b]);
      int64_t best = 0;
      for (size_t x = i; x < e; ++x) {
        int64_t n = 0;
        for (size_t y = x; y < e; ++y) n += d[y] <= d[x] + band;
        best = std::max(best, n);
      }
      if (c.hits != best || a >= b) {
        printf("chain differs: round %d group at %zu\n", round, i);
        ++bad;
      }
      i = e;
    }
  }
  printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
