// Ground-truth edge labels from read positions (include/gnm.h, "ground-truth labels"): the arithmetic the kernels of
// csrc/gnm_labels.hip and the host entry gnm_gt_labels_host share, as plain C++ that compiles for the host as well as for the device,
// like gnm_overlap.h -- the node check, the valid-edge predicate, the two packed keys and the record layout -- and, for the host
// alone, the whole labelling over union-find and queues (gt_labels_host_).  A host program can include this file alone
// (tools/labels_host_check.cpp).  Integers only.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gnm_seq.h"

namespace gnm {

constexpr int64_t kGtMaxPos = (1ll << 32) - 1;           // 0 <= start < end <= kGtMaxPos: a position and a node id share 64 bits
constexpr uint32_t kGtIdMask = 0x7fffffffu;              // node ids are below 2^31 - 1

// the record's words, in order (gnm_gt_record)
enum { kGtEdges = 0, kGtValid, kGtWrongStrand, kGtSelfLoops, kGtGap, kGtBackward, kGtComponents, kGtSingletons, kGtBackbone,
       kGtPositives, kGtTwinMissing, kGtInvalid, kGtCalls, kGtWords };

// A node's three values are usable: 0 <= start < end <= kGtMaxPos and strand +1 or -1.
GNM_SEQ_FN bool gt_node_ok_(int64_t start, int64_t end, int64_t strand) {
  return start >= 0 && start < end && end <= kGtMaxPos && (strand == 1 || strand == -1);
}

// The class of edge s -> d, as the record word it is counted under: kGtValid when both ends are + strand nodes, s != d and
// start[s] <= start[d] < end[s]; otherwise the first of wrong strand, self loop, gap (start[d] >= end[s]), backward
// (start[d] < start[s]) that applies.
GNM_SEQ_FN int gt_edge_class_(bool plus_s, bool plus_d, bool same, int64_t start_s, int64_t end_s, int64_t start_d) {
  if (!plus_s || !plus_d) return kGtWrongStrand;
  if (same) return kGtSelfLoops;
  if (start_d >= end_s) return kGtGap;
  if (start_d < start_s) return kGtBackward;
  return kGtValid;
}

// (start, node id), smallest first: a component's label is the smallest key among its nodes, its root the node that key names.
GNM_SEQ_FN uint64_t gt_root_key_(int64_t start, uint32_t id) { return ((uint64_t)start << 31) | (uint64_t)(id & kGtIdMask); }
GNM_SEQ_FN uint32_t gt_root_id_(uint64_t key) { return (uint32_t)key & kGtIdMask; }
// (end, ~node id), largest first: the top is the reached node of largest end, the smallest id among equals.  Never 0 (end >= 1).
GNM_SEQ_FN uint64_t gt_top_key_(int64_t end, uint32_t id) { return ((uint64_t)end << 31) | (uint64_t)(~id & kGtIdMask); }
GNM_SEQ_FN uint32_t gt_top_id_(uint64_t key) { return ~(uint32_t)key & kGtIdMask; }

// Does edge t of the caller's list join a -> b?  (The check of a `twin` entry before it is believed.)
GNM_SEQ_FN bool gt_twin_is_(const int32_t* src, const int32_t* dst, int64_t E, int64_t t, uint32_t a, uint32_t b) {
  return t >= 0 && t < E && (uint32_t)src[t] == a && (uint32_t)dst[t] == b;
}

// ---- the host's labelling -------------------------------------------------------------------------------------------------------
struct GtHostOut {
  float* y;                  // [E]
  uint8_t *valid, *backbone; // [E], [n]
  int32_t *component, *top;  // [n]
  int64_t* rec;              // [kGtWords], added to
};

// The number of unusable nodes, or of edges that name a node outside [0, n): with either, nothing may be labelled.
inline int64_t gt_host_invalid_(int64_t n, int64_t E, const int32_t* src, const int32_t* dst, const int64_t* start, const int64_t* end,
                                const int64_t* strand) {
  int64_t bad = 0;
  for (int64_t v = 0; v < n; ++v) bad += gt_node_ok_(start[v], end[v], strand[v]) ? 0 : 1;
  for (int64_t e = 0; e < E; ++e) bad += (uint32_t)src[e] < (uint32_t)n && (uint32_t)dst[e] < (uint32_t)n ? 0 : 1;
  return bad;
}

// Labels of a graph in the caller's numbering: union-find (the smaller key stays the representative) over the valid edges, one
// forward search from all roots, the tops, one backward search from all tops, then every edge looks up its own answer -- a + strand
// edge its two ends, a - strand edge the + strand edge it mirrors.  twin: NULL (the mirror is searched in a sorted copy of the edge
// list), or the caller's mirror edge ids, each believed only when it names the mirrored pair.  The input is valid (gt_host_invalid_).
inline void gt_labels_host_(int64_t n, int64_t E, const int32_t* src, const int32_t* dst, const int64_t* start, const int64_t* end,
                            const int64_t* strand, const int64_t* twin, const GtHostOut& o) {
  const size_t N = (size_t)n, M = (size_t)E;
  int64_t cnt[kGtWords] = {};
  std::vector<uint32_t> parent(N);
  for (size_t v = 0; v < N; ++v) parent[v] = (uint32_t)v;
  auto key = [&](uint32_t v) { return gt_root_key_(start[v], v); };
  auto find = [&](uint32_t v) {
    uint32_t r = v;
    while (parent[r] != r) r = parent[r];
    while (parent[v] != r) {
      const uint32_t nx = parent[v];
      parent[v] = r;
      v = nx;
    }
    return r;
  };
  std::vector<uint8_t> touched(N, 0);
  std::vector<int32_t> optr(N + 1, 0), iptr(N + 1, 0);
  for (size_t e = 0; e < M; ++e) {
    const uint32_t s = (uint32_t)src[e], d = (uint32_t)dst[e];
    const int c = gt_edge_class_(strand[s] == 1, strand[d] == 1, s == d, start[s], end[s], start[d]);
    cnt[c] += 1;
    o.valid[e] = c == kGtValid;
    if (c != kGtValid) continue;
    touched[s] = touched[d] = 1;
    optr[s + 1] += 1;
    iptr[d + 1] += 1;
    const uint32_t a = find(s), b = find(d);
    if (a != b) {
      if (key(a) < key(b)) parent[b] = a; else parent[a] = b;
    }
  }
  cnt[kGtEdges] = E;
  for (size_t v = 0; v < N; ++v) {
    optr[v + 1] += optr[v];
    iptr[v + 1] += iptr[v];
  }
  std::vector<int32_t> onbr((size_t)cnt[kGtValid]), inbr((size_t)cnt[kGtValid]), ofill(optr.begin(), optr.end() - 1),
      ifill(iptr.begin(), iptr.end() - 1);
  for (size_t e = 0; e < M; ++e)
    if (o.valid[e]) {
      onbr[(size_t)ofill[(size_t)src[e]]++] = dst[e];
      inbr[(size_t)ifill[(size_t)dst[e]]++] = src[e];
    }
  // forward from every root at once (the components are disjoint), the top of every component at its root, backward from the tops
  std::vector<uint8_t> fwd(N, 0), bwd(N, 0);
  std::vector<uint64_t> topkey(N, 0);
  std::vector<uint32_t> queue;
  queue.reserve(N);
  for (size_t v = 0; v < N; ++v)
    if (strand[v] == 1 && find((uint32_t)v) == (uint32_t)v) {
      fwd[v] = 1;
      queue.push_back((uint32_t)v);
      cnt[kGtComponents] += 1;
      cnt[kGtSingletons] += touched[v] ? 0 : 1;
    }
  for (size_t h = 0; h < queue.size(); ++h) {
    const uint32_t v = queue[h];
    uint64_t& t = topkey[find(v)];
    t = std::max(t, gt_top_key_(end[v], v));
    for (int32_t p = optr[v]; p < optr[v + 1]; ++p) {
      const uint32_t w = (uint32_t)onbr[(size_t)p];
      if (!fwd[w]) {
        fwd[w] = 1;
        queue.push_back(w);
      }
    }
  }
  queue.clear();
  for (size_t v = 0; v < N; ++v)
    if (strand[v] == 1 && find((uint32_t)v) == (uint32_t)v) {
      const uint32_t t = gt_top_id_(topkey[v]);
      bwd[t] = 1;
      queue.push_back(t);
    }
  for (size_t h = 0; h < queue.size(); ++h) {
    const uint32_t v = queue[h];
    for (int32_t p = iptr[v]; p < iptr[v + 1]; ++p) {
      const uint32_t w = (uint32_t)inbr[(size_t)p];
      if (!bwd[w]) {
        bwd[w] = 1;
        queue.push_back(w);
      }
    }
  }
  for (size_t v = 0; v < N; ++v) {
    const bool plus = strand[v] == 1;
    const uint32_t r = plus ? find((uint32_t)v) : 0u;
    o.component[v] = plus ? (int32_t)r : -1;
    o.top[v] = plus ? (int32_t)gt_top_id_(topkey[r]) : -1;
    o.backbone[v] = plus && fwd[v] && bwd[v];
    cnt[kGtBackbone] += o.backbone[v];
  }
  // the mirror of a -> b is b^1 -> a^1
  std::vector<uint64_t> pairs;
  if (!twin) {
    pairs.resize(M);
    for (size_t e = 0; e < M; ++e) pairs[e] = ((uint64_t)(uint32_t)src[e] << 32) | (uint32_t)dst[e];
    std::sort(pairs.begin(), pairs.end());
  }
  auto has_edge = [&](size_t e, uint32_t a, uint32_t b) {
    if (a >= (uint32_t)n || b >= (uint32_t)n) return false;
    if (twin) return gt_twin_is_(src, dst, E, twin[e], a, b);
    return std::binary_search(pairs.begin(), pairs.end(), ((uint64_t)a << 32) | b);
  };
  for (size_t e = 0; e < M; ++e) {
    const uint32_t s = (uint32_t)src[e], d = (uint32_t)dst[e];
    bool one = false;
    if (o.valid[e]) {
      one = o.backbone[s] && o.backbone[d];
      if (one && !has_edge(e, d ^ 1u, s ^ 1u)) cnt[kGtTwinMissing] += 1;
    } else if (strand[s] == -1 && strand[d] == -1 && s != d) {
      const uint32_t a = d ^ 1u, b = s ^ 1u;          // e mirrors a -> b
      if (a < (uint32_t)n && b < (uint32_t)n && o.backbone[a] && o.backbone[b] &&
          gt_edge_class_(strand[a] == 1, strand[b] == 1, a == b, start[a], end[a], start[b]) == kGtValid)
        one = has_edge(e, a, b);
    }
    o.y[e] = one ? 1.0f : 0.0f;
    cnt[kGtPositives] += one;
  }
  cnt[kGtCalls] = 1;
  for (int k = 0; k < kGtWords; ++k) o.rec[k] += cnt[k];
}

}  // namespace gnm
