// regions.hpp -- the one description of a context's annotated regions (calitas_set_regions), for the host and for the kernels that
// class a hit: regions_kernel (hits.hip), bin_regions_kernel (binned.hip) and the host stage (post.cpp, hits_regions).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/calitas_hip.h"
#include "common.hpp"

namespace calitas {

// The resident form.  Every contig is cut into segments that cover it from base 0 to its end without a hole: segment i of the table
// holds the bases [seg[i].start, seg[i + 1].start) of its contig -- the last one of a contig up to the contig's end -- and `cls` is the
// smallest class of the intervals that cover those bases, 0 where none does; neighbours have different classes.  A contig without
// intervals is one segment of class 0.  contig[2 c] is the first segment of contig c, contig[2 c + 1] the first entry of its coarse
// index: one entry per REGION_COARSE bases, the segment (a table index) that holds base j * REGION_COARSE.  contig[2 n_contigs] is the
// number of segments.
constexpr int REGION_COARSE_SHIFT = 13;
constexpr uint32_t REGION_COARSE = 1u << REGION_COARSE_SHIFT;
constexpr int REGION_WALK_MAX = CALITAS_MAX_OPS;     // a hit covers at most this many bases (hits_dev.hpp, HIT_MAX_LEN), a segment at least one

struct RegionSeg { uint32_t start, cls; };
struct RegionsView {
  const RegionSeg* seg;
  const uint32_t* coarse;
  const uint32_t* contig;     // 2 * n_contigs + 1 words
  uint32_t n_classes;         // 0: no regions set
};

// The class of the extent [start, end) of contig c (calitas_hip.h, calitas_search_regions): one coarse load, a binary search between
// two coarse entries for the segment that holds `start`, then the segments below `end`; the smallest class that is not 0 wins, and
// nothing beats class 1.  len: the contig's length (an extent is held against the contig's own bases: no interval lies outside them).
CAL_HD inline uint32_t region_class(const RegionsView& rv, uint32_t c, int64_t start, int64_t end, uint64_t len) {
  if (start < 0) start = 0;
  if (end > (int64_t)len) end = (int64_t)len;
  if (start >= end) return 0u;
  const uint32_t s1 = rv.contig[2 * c + 2], cb = rv.contig[2 * c + 1];
  const uint32_t b = (uint32_t)((uint64_t)start >> REGION_COARSE_SHIFT), nb = (uint32_t)((len + REGION_COARSE - 1) >> REGION_COARSE_SHIFT);
  uint32_t lo = rv.coarse[cb + b], hi = b + 1 < nb ? rv.coarse[cb + b + 1] : s1 - 1;   // the segment of `start` is one of lo .. hi
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (rv.seg[mid].start <= (uint32_t)start) lo = mid; else hi = mid - 1;
  }
  uint32_t best = 0;
  for (int k = 0; k < REGION_WALK_MAX && lo < s1; k++, lo++) {
    const RegionSeg s = rv.seg[lo];
    if (k && s.start >= (uint32_t)end) break;
    if (s.cls && (best == 0 || s.cls < best)) best = s.cls;
    if (best == 1) break;
  }
  return best;
}

// The set as the context keeps it on the host: the caller's intervals as they came (calitas_hits_regions and the tests' yardsticks
// need nothing of them; they are what a later question about the set is answered from) and the flattened tables.
// Every flattened set has a number of its own (never 0), so that what is derived from a context's set -- the site listing's presence
// table -- knows when the set is another one.
inline uint64_t regions_next_serial() { static std::atomic<uint64_t> n{0}; return ++n; }

struct RegionsHost {
  uint32_t n_classes = 0;
  uint64_t serial = 0;
  std::vector<calitas_region_t> raw;
  std::vector<RegionSeg> seg;
  std::vector<uint32_t> coarse, contig;
  bool empty() const { return n_classes == 0; }
  void clear() { n_classes = 0; serial = 0; raw.clear(); seg.clear(); coarse.clear(); contig.clear(); }
  RegionsView view() const { return RegionsView{seg.data(), coarse.data(), contig.data(), n_classes}; }
};

// Validates the intervals against the contigs (lens[c], absent(c)) and flattens them.  Returns an error text or "".
template <typename Absent>
inline std::string regions_flatten(const std::vector<uint64_t>& lens, Absent absent, const calitas_region_t* iv, uint64_t n, uint32_t n_classes,
                                   RegionsHost& out) {
  out.clear();
  if (n == 0) return "";
  if (!iv) return "NULL intervals";
  if (n_classes < 2 || n_classes > CALITAS_REGION_CLASSES_MAX) return "n_classes of a region set must be 2 .. CALITAS_REGION_CLASSES_MAX (8)";
  if (n > 0x7FFFFFF0ull) return "too many intervals";
  std::vector<std::vector<const calitas_region_t*>> by_contig(lens.size());
  for (uint64_t i = 0; i < n; i++) {
    const calitas_region_t& r = iv[i];
    const std::string at = "interval " + std::to_string(i) + ": ";
    if (r.contig_index < 0 || (size_t)r.contig_index >= lens.size()) return at + "contig index out of range";
    if (absent((size_t)r.contig_index)) return at + "its contig is absent from this context's reference";
    if (r.start < 0 || r.start >= r.end) return at + "start >= end (or negative)";
    if ((uint64_t)r.end > lens[(size_t)r.contig_index]) return at + "it ends beyond its contig";
    if (r.cls < 1 || r.cls >= n_classes) return at + "class out of range (1 .. n_classes - 1)";
    by_contig[(size_t)r.contig_index].push_back(&r);
  }
  out.contig.assign(2 * lens.size() + 1, 0u);
  for (size_t c = 0; c < lens.size(); c++) {
    out.contig[2 * c] = (uint32_t)out.seg.size();
    out.contig[2 * c + 1] = (uint32_t)out.coarse.size();
    const size_t first = out.seg.size();
    // a sweep over the interval ends in coordinate order, with the number of open intervals per class
    std::vector<std::pair<uint32_t, int>> ev;           // (position, +cls opens / -cls closes)
    ev.reserve(2 * by_contig[c].size());
    for (const calitas_region_t* r : by_contig[c]) { ev.emplace_back((uint32_t)r->start, (int)r->cls); ev.emplace_back((uint32_t)r->end, -(int)r->cls); }
    std::sort(ev.begin(), ev.end(), [](const std::pair<uint32_t, int>& a, const std::pair<uint32_t, int>& b) { return a.first < b.first; });
    uint64_t open[CALITAS_REGION_CLASSES_MAX] = {};
    out.seg.push_back(RegionSeg{0u, 0u});
    for (size_t e = 0; e < ev.size();) {
      const uint32_t pos = ev[e].first;
      for (; e < ev.size() && ev[e].first == pos; e++) { if (ev[e].second > 0) open[ev[e].second]++; else open[-ev[e].second]--; }
      if ((uint64_t)pos >= lens[c]) break;              // (ends at the contig's end: nothing follows)
      uint32_t cls = 0;
      for (uint32_t k = 1; k < n_classes && !cls; k++) if (open[k]) cls = k;
      if (out.seg.back().start == pos && out.seg.size() > first) {          // (the segment at base 0)
        out.seg.back().cls = cls;
        if (out.seg.size() > first + 1 && out.seg[out.seg.size() - 2].cls == cls) out.seg.pop_back();
      } else if (out.seg.back().cls != cls) out.seg.push_back(RegionSeg{pos, cls});
    }
    const uint64_t nb = std::max<uint64_t>((lens[c] + REGION_COARSE - 1) >> REGION_COARSE_SHIFT, 1);
    size_t s = first;
    for (uint64_t b = 0; b < nb; b++) {
      while (s + 1 < out.seg.size() && (uint64_t)out.seg[s + 1].start <= (b << REGION_COARSE_SHIFT)) s++;
      out.coarse.push_back((uint32_t)s);
    }
  }
  out.contig[2 * lens.size()] = (uint32_t)out.seg.size();
  out.n_classes = n_classes;
  out.serial = regions_next_serial();
  out.raw.assign(iv, iv + n);
  return "";
}

// What a regions call's kept hits add up to per class, besides ScoreWords' totals: per class sum_q32, perfect, max_q32 and rows
// (REGION_WORDS words), and its own counts table.  Pieces of a job add like ScoreWords do.
constexpr uint32_t REGION_WORDS = 4;
struct RegionWords {
  uint32_t n_classes = 0;
  std::vector<uint64_t> words;      // n_classes x REGION_WORDS
  std::vector<uint64_t> tables;     // n_classes x cells
  void init(uint32_t nc, size_t cells) { n_classes = nc; words.assign((size_t)nc * REGION_WORDS, 0); tables.assign((size_t)nc * cells, 0); }
  void add(const RegionWords& o) {
    if (o.n_classes == 0) return;
    if (n_classes == 0) { *this = o; return; }
    for (size_t i = 0; i < words.size() && i < o.words.size(); i++) {
      if (i % REGION_WORDS == 2) words[i] = std::max(words[i], o.words[i]); else words[i] += o.words[i];
    }
    if (tables.size() < o.tables.size()) tables.resize(o.tables.size(), 0);
    for (size_t i = 0; i < o.tables.size(); i++) tables[i] += o.tables[i];
  }
  // one kept hit of class c in cell `cell` of `cells` (the host stages); perfect hits have no score
  void count(uint32_t c, size_t cells, size_t cell, bool perfect, uint64_t score) {
    tables[(size_t)c * cells + cell]++;
    uint64_t* w = words.data() + (size_t)c * REGION_WORDS;
    w[3]++;
    if (perfect) w[1]++; else { w[0] += score; if (score > w[2]) w[2] = score; }
  }
};

}  // namespace calitas
