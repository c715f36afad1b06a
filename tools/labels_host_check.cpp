// Stand-alone host check of csrc/gnm_labels.h (no GPU, no Python): random position graphs -- duplicate edges, self loops, edges
// between strands, missing mirrors, + strands on odd and even ids, empty graphs -- through gt_host_invalid_ / gt_labels_host_, the
// body of gnm_gt_labels_host, against a brute-force fixpoint restatement, with and without twins.  Every array has exactly its size,
// so an access past an end is a heap overflow the sanitizer sees.  Meant to be built with a host sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gnnome_assembly_amd/csrc \
//       tools/labels_host_check.cpp -o labels_host_check && ./labels_host_check
// Exit status 0 and "ok" when every case agrees.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "gnm_labels.h"

using namespace gnm;

struct Case {
  int64_t n = 0;
  std::vector<int32_t> src, dst;
  std::vector<int64_t> start, end, strand, twin;
};

static Case make(std::mt19937_64& rng, int R, int span, double density) {
  Case c;
  c.n = 2 * R;
  c.start.resize((size_t)c.n); c.end.resize((size_t)c.n); c.strand.resize((size_t)c.n);
  std::vector<int> plus((size_t)R);
  for (int r = 0; r < R; ++r) {
    const int64_t s = (int64_t)(rng() % (uint64_t)span), l = 1 + (int64_t)(rng() % 40);
    plus[(size_t)r] = 2 * r + (int)(rng() & 1);
    for (int k = 0; k < 2; ++k) { c.start[(size_t)(2 * r + k)] = s; c.end[(size_t)(2 * r + k)] = s + l; }
    c.strand[(size_t)plus[(size_t)r]] = 1;
    c.strand[(size_t)(plus[(size_t)r] ^ 1)] = -1;
  }
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int a = 0; a < R; ++a)
    for (int b = 0; b < R; ++b) {
      if (u(rng) >= density) continue;
      const int s = plus[(size_t)a], d = plus[(size_t)b];
      const int copies = u(rng) < 0.1 ? 2 : 1;
      for (int k = 0; k < copies; ++k) { c.src.push_back(s); c.dst.push_back(d); }
      if (u(rng) < 0.9) { c.src.push_back(d ^ 1); c.dst.push_back(s ^ 1); }           // one mirror in ten is missing
      if (u(rng) < 0.05) { c.src.push_back(s); c.dst.push_back(d ^ 1); }              // an edge between the strands
    }
  std::map<std::pair<int, int>, int64_t> ids;
  for (size_t e = 0; e < c.src.size(); ++e) ids.emplace(std::make_pair(c.src[e], c.dst[e]), (int64_t)e);
  for (size_t e = 0; e < c.src.size(); ++e) {
    const auto it = ids.find(std::make_pair(c.dst[e] ^ 1, c.src[e] ^ 1));
    c.twin.push_back(it == ids.end() ? -1 : it->second);
  }
  return c;
}

// y by brute force: labels and flags by repeated passes over the edge list until nothing changes
static std::vector<float> brute(const Case& c, std::vector<uint8_t>& backbone) {
  const size_t N = (size_t)c.n, M = c.src.size();
  auto valid = [&](size_t s, size_t d) {
    return c.strand[s] == 1 && c.strand[d] == 1 && s != d && c.start[s] <= c.start[d] && c.start[d] < c.end[s];
  };
  std::vector<uint64_t> lab(N);
  for (size_t v = 0; v < N; ++v) lab[v] = ((uint64_t)c.start[v] << 31) | v;
  for (bool again = true; again;) {
    again = false;
    for (size_t e = 0; e < M; ++e) {
      const size_t s = (size_t)c.src[e], d = (size_t)c.dst[e];
      if (!valid(s, d) || lab[s] == lab[d]) continue;
      lab[s] = lab[d] = lab[s] < lab[d] ? lab[s] : lab[d];
      again = true;
    }
  }
  std::vector<uint8_t> fwd(N, 0), bwd(N, 0);
  for (size_t v = 0; v < N; ++v) fwd[v] = c.strand[v] == 1 && (lab[v] & kGtIdMask) == v;
  auto spread = [&](std::vector<uint8_t>& f, bool forward) {
    for (bool again = true; again;) {
      again = false;
      for (size_t e = 0; e < M; ++e) {
        const size_t s = (size_t)c.src[e], d = (size_t)c.dst[e];
        if (!valid(s, d)) continue;
        const size_t from = forward ? s : d, to = forward ? d : s;
        if (f[from] && !f[to]) { f[to] = 1; again = true; }
      }
    }
  };
  spread(fwd, true);
  for (size_t r = 0; r < N; ++r) {
    if (c.strand[r] != 1 || (lab[r] & kGtIdMask) != r) continue;
    size_t top = r;
    for (size_t v = 0; v < N; ++v)
      if (fwd[v] && lab[v] == lab[r] && (c.end[v] > c.end[top] || (c.end[v] == c.end[top] && v < top))) top = v;
    bwd[top] = 1;
  }
  spread(bwd, false);
  backbone.assign(N, 0);
  for (size_t v = 0; v < N; ++v) backbone[v] = fwd[v] && bwd[v];
  std::vector<float> y(M, 0.0f);
  for (size_t e = 0; e < M; ++e) {
    const size_t s = (size_t)c.src[e], d = (size_t)c.dst[e];
    if (!valid(s, d) || !backbone[s] || !backbone[d]) continue;
    y[e] = 1.0f;
    for (size_t m = 0; m < M; ++m)
      if ((size_t)c.src[m] == (d ^ 1) && (size_t)c.dst[m] == (s ^ 1)) y[m] = 1.0f;
  }
  return y;
}

static int fail(const char* what, int id) {
  std::printf("FAILED: %s (case %d)\n", what, id);
  return 1;
}

int main() {
  std::mt19937_64 rng(20261021);
  int cases = 0;
  for (int id = 0; id < 400; ++id) {
    const int R = id < 4 ? id : 1 + (int)(rng() % 40);
    const Case c = make(rng, R, 20 + (int)(rng() % 200), id % 5 == 0 ? 0.5 : 0.08);
    const size_t N = (size_t)c.n, M = c.src.size();
    if (gt_host_invalid_(c.n, (int64_t)M, c.src.data(), c.dst.data(), c.start.data(), c.end.data(), c.strand.data()) != 0)
      return fail("a usable case is called invalid", id);
    std::vector<uint8_t> want_bb;
    const std::vector<float> want = brute(c, want_bb);
    for (int with_twin = 0; with_twin < 2; ++with_twin) {
      std::vector<float> y(M, -1.0f);
      std::vector<uint8_t> valid(M, 9), bb(N, 9);
      std::vector<int32_t> comp(N, -9), top(N, -9);
      std::vector<int64_t> rec((size_t)kGtWords, 0);
      gt_labels_host_(c.n, (int64_t)M, c.src.data(), c.dst.data(), c.start.data(), c.end.data(), c.strand.data(),
                      with_twin && M ? c.twin.data() : nullptr, GtHostOut{y.data(), valid.data(), bb.data(), comp.data(), top.data(), rec.data()});
      if (y != want) return fail("y differs from the brute force", id);
      if (bb != want_bb) return fail("backbone differs from the brute force", id);
      int64_t pos = 0;
      for (float v : y) pos += v == 1.0f;
      if (rec[kGtPositives] != pos || rec[kGtEdges] != (int64_t)M || rec[kGtCalls] != 1) return fail("record", id);
      if (rec[kGtValid] + rec[kGtWrongStrand] + rec[kGtSelfLoops] + rec[kGtGap] + rec[kGtBackward] != (int64_t)M) return fail("classes", id);
    }
    ++cases;
  }
  // unusable nodes are counted, one by one
  Case c = make(rng, 6, 50, 0.3);
  c.end[3] = c.start[3];
  c.strand[5] = 0;
  c.start[7] = -1;
  if (gt_host_invalid_(c.n, (int64_t)c.src.size(), c.src.data(), c.dst.data(), c.start.data(), c.end.data(), c.strand.data()) != 3)
    return fail("three unusable nodes", -1);
  if (gt_top_id_(gt_top_key_(kGtMaxPos, kGtIdMask - 1)) != kGtIdMask - 1 || gt_root_id_(gt_root_key_(kGtMaxPos - 1, 5)) != 5)
    return fail("key packing", -1);
  std::printf("ok: %d random graphs, with and without twins\n", cases);
  return 0;
}
