// Stand-alone host check of csrc/gnm_align.h (no GPU, no Python): the hand cases and the band's word boundaries against the plain
// dynamic programme, meant to be built with a host sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gnnome_assembly_amd/csrc \
//       tools/align_host_check.cpp -o align_host_check && ./align_host_check
// Exit status 0 and "ok" when every case agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gnm_align.h"

using namespace gnm;

static const char kLetters[] = "=ACMGRSVTWYHKDBN";

struct Store {
  std::vector<uint8_t> packed;           // exactly the store's bytes: a read past its end is a heap overflow the sanitizer sees
  std::vector<int64_t> off, len;
  SeqStore view(int64_t n) const { return SeqStore{packed.data(), off.data(), len.data(), (int64_t)packed.size() * 2, (int64_t)off.size(), n}; }
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

static std::string revcomp(const std::string& r) {
  std::string o(r.rbegin(), r.rend());
  for (char& ch : o) ch = kLetters[seq_brev4_((unsigned)(strchr(kLetters, ch) - kLetters))];
  return o;
}

static int64_t dp(const std::string& q, const std::string& t) {
  std::vector<int64_t> row(t.size() + 1), nw(t.size() + 1);
  for (size_t j = 0; j <= t.size(); ++j) row[j] = (int64_t)j;
  for (size_t i = 1; i <= q.size(); ++i) {
    nw[0] = (int64_t)i;
    for (size_t j = 1; j <= t.size(); ++j) nw[j] = std::min({row[j - 1] + (q[i - 1] != t[j - 1]), row[j] + 1, nw[j - 1] + 1});
    row.swap(nw);
  }
  return *std::min_element(row.begin(), row.end());
}

static AlignEdge run(const SeqStore& s, int32_t a, int32_t c, int64_t p, int K) {
  switch (align_words_(K)) {
    case 1: return align_edge_<1>(s, a, c, p, K);
    case 2: return align_edge_<2>(s, a, c, p, K);
    case 4: return align_edge_<4>(s, a, c, p, K);
    default: return align_edge_<8>(s, a, c, p, K);
  }
}

static int failures = 0, checked = 0;

// the pair on all four strand combinations: an odd node's read is stored reverse-complemented
static void check(const std::string& a, const std::string& c, int64_t p, int K, int expect = -2) {
  for (int oa = 0; oa < 2; ++oa)
    for (int oc = 0; oc < 2; ++oc) {
      const Store st = pack({oa ? revcomp(a) : a, oc ? revcomp(c) : c});
      const AlignEdge r = run(st.view(4), oa, 2 + oc, p, K);
      const int64_t pc = std::max<int64_t>(0, std::min<int64_t>(p, (int64_t)a.size())), m = (int64_t)a.size() - pc;
      const std::string q = a.substr((size_t)pc), t = c.substr(0, (size_t)std::min<int64_t>((int64_t)c.size(), m + K));
      int64_t want = m ? dp(q, t) : 0;
      if (want > K) want = K + 1;
      ++checked;
      if (r.dist != want || r.m != m || (expect != -2 && r.dist != expect)) {
        ++failures;
        fprintf(stderr, "MISMATCH K=%d m=%lld strands %d%d: got %d, dynamic programme %lld, expected %d\n", K, (long long)m, oa, oc, r.dist,
                (long long)want, expect);
      }
    }
}

int main() {
  std::mt19937 rng(1);
  auto rnd = [&](size_t n) { std::string s(n, 'A'); for (char& ch : s) ch = "ACGT"[rng() & 3]; return s; };
  auto mutate = [&](std::string s, double rate) {
    std::string o;
    for (char ch : s) {
      const double u = (rng() & 0xffffff) / double(0x1000000);
      if (u < rate / 3) o += "ACGT"[rng() & 3];
      else if (u < 2 * rate / 3) { o += ch; o += "ACGT"[rng() & 3]; }
      else if (u >= rate) o += ch;
    }
    return o;
  };
  for (int K : {1, 3, 40}) {                               // hand cases: N matches nothing but N
    const size_t m = 3 * K + 40, h = K + 5;
    const std::string r = rnd(m), extra = rnd(2 * K + 8);
    std::string one = r, kn = r, kn1 = r;
    one[h] = 'N';
    for (int i = 0; i <= K; ++i) { if (i < K) kn[2 + 3 * i] = 'N'; kn1[2 + 3 * i] = 'N'; }
    check(r, r + extra, 0, K, 0);
    check("GG" + one, r + extra, 2, K, 1);
    check(r.substr(0, h) + std::string(K, 'N') + r.substr(h), r + extra, 0, K, K);
    check(r, r.substr(0, h) + std::string(K, 'N') + r.substr(h) + extra, 0, K, K);
    check(kn, r + extra, 0, K, K);
    check(kn1, r + extra, 0, K, K + 1);
  }
  for (int K : {0, 1, 31, 32, 63, 64, 127, 128, 255})       // word boundaries
    for (size_t m : {0, 1, 2, 63, 64, 65, 127, 128, 129, 300})
      for (double rate : {0.0, 0.06}) {
        const std::string region = rnd(m), head = rnd(rng() % 9);
        check(head + mutate(region, rate), region + rnd(rng() % (2 * K + 20)), (int64_t)head.size(), K);
      }
  for (int K : {2, 40}) {                                  // short and empty targets, clamped prefixes
    const std::string r = rnd(2 * K + 70);
    for (size_t cut : {(size_t)1, (size_t)K, (size_t)K + 1, (size_t)K + 30, r.size()}) check("ACG" + r, r.substr(0, r.size() - cut), 3, K);
    check(r, r, -1, K);
    check(r, r, (int64_t)r.size() + 1, K);
    check(r, r, (int64_t)r.size(), K);
  }
  const Store st = pack({"ACGT", "ACGT"});                 // nodes and reads out of range: nothing is read
  for (int32_t bad : {-1, 4, 5, 6, 1 << 30})
    if (run(st.view(6), bad, 0, 0, 5).dist != -1 || run(st.view(6), 0, bad, 0, 5).dist != -1) ++failures;
  printf("%s: %d alignments checked, %d failures\n", failures ? "FAILED" : "ok", checked, failures);
  return failures ? 1 : 0;
}
