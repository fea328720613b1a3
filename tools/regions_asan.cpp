// regions_asan.cpp -- the host side of a regions call: the flattening of an interval set (regions_flatten), the lookup (region_class)
// against a plain scan of the raw intervals, the host stage (hits_regions) and the merges of its pieces (ScoreWords::add: RegionWords,
// TopList with its class bytes), as a stand-alone program for a run under AddressSanitizer and UBSan: host objects only, no device,
// nothing loaded into another process.
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer tools/regions_asan.cpp \
//         calitas_amd/csrc/post.cpp calitas_amd/csrc/refpack.cpp -pthread -o regions_asan && ./regions_asan
// The alignments are made up (a planted site every 40 bases, a few 'X' columns each, both strands): the run is about memory, about
// the lookup against the scan, and about the merge of pieces against the result of the whole.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../calitas_amd/csrc/hits.hpp"
#include "../calitas_amd/csrc/post.hpp"
#include "../calitas_amd/csrc/regions.hpp"

using namespace calitas;

static uint32_t scan_class(const std::vector<calitas_region_t>& iv, int32_t contig, int64_t a, int64_t b) {
  uint32_t best = 0;
  if (a >= b) return 0;
  for (const calitas_region_t& r : iv)
    if (r.contig_index == contig && r.start < b && r.end > a && (best == 0 || r.cls < best)) best = r.cls;
  return best;
}

int main() {
  std::mt19937 rng(13);
  const int n_contigs = 4;
  const int lens[n_contigs] = {3 * 8192 + 77, 6000, 8192, 500};
  std::vector<std::string> seqs, names;
  for (int c = 0; c < n_contigs; c++) {
    std::string s((size_t)lens[c], 'A');
    for (char& ch : s) ch = "ACGT"[rng() & 3];
    seqs.push_back(s); names.push_back("c" + std::to_string(c));
  }
  std::vector<const char*> nm; std::vector<uint64_t> ln; std::vector<const uint8_t*> bs;
  for (int c = 0; c < n_contigs; c++) { nm.push_back(names[(size_t)c].c_str()); ln.push_back((uint64_t)lens[c]); bs.push_back((const uint8_t*)seqs[(size_t)c].data()); }
  PackedRef ref;
  pack_reference(ref, n_contigs, nm.data(), ln.data(), bs.data(), "asan", 2);

  // 1. flattening and lookup against the scan, over random sets; contig 3 has no interval in every second set
  RegionsHost flat;
  std::vector<calitas_region_t> iv;
  for (int trial = 0; trial < 40; trial++) {
    const uint32_t n_classes = 2 + rng() % 7;
    iv.clear();
    for (int c = 0; c < n_contigs; c++) {
      if (c == 3 && (trial & 1)) continue;
      const int n = 1 + (int)(rng() % 80);
      for (int i = 0; i < n; i++) {
        const int a = (int)(rng() % (uint32_t)lens[c]);
        const int w[7] = {1, 1, 2, 7, 40, 300, 9000};
        iv.push_back(calitas_region_t{c, a, std::min(lens[c], a + w[rng() % 7]), (uint32_t)(1 + rng() % (n_classes - 1))});
      }
      iv.push_back(calitas_region_t{c, 0, 1, 1});
      iv.push_back(calitas_region_t{c, lens[c] - 1, lens[c], n_classes - 1});
      for (int m = 8192; m < lens[c]; m += 8192) iv.push_back(calitas_region_t{c, m - (int)(rng() % 3), std::min(lens[c], m + 1 + (int)(rng() % 2)), (uint32_t)(1 + rng() % (n_classes - 1))});
    }
    const std::string e = regions_flatten(ln, [](size_t) { return false; }, iv.data(), iv.size(), n_classes, flat);
    if (!e.empty()) { std::fprintf(stderr, "flatten: %s\n", e.c_str()); return 1; }
    for (size_t s = 1; s < flat.seg.size(); s++)       // neighbours of one contig differ
      for (int c = 0; c < n_contigs; c++)
        if (s > flat.contig[2 * c] && s < flat.contig[2 * c + 2] && flat.seg[s].cls == flat.seg[s - 1].cls) { std::fprintf(stderr, "unmerged segments\n"); return 1; }
    for (int q = 0; q < 20000; q++) {
      const int c = (int)(rng() % n_contigs);
      int64_t a;
      if (rng() & 1) { const calitas_region_t& r = iv[rng() % iv.size()]; a = (r.contig_index == c ? ((rng() & 1) ? r.start : r.end) : 0) + (int)(rng() % 27) - 24; }
      else a = (int64_t)(rng() % (uint32_t)(lens[c] + 35)) - 30;
      const int wq[6] = {0, 1, 20, 23, 25, 100};
      const int64_t b = a + wq[rng() % 6];
      const uint32_t got = region_class(flat.view(), (uint32_t)c, a, b, (uint64_t)lens[c]), want = scan_class(iv, c, a, b);
      if (got != want) { std::fprintf(stderr, "trial %d: class of c%d [%lld, %lld) is %u, the scan says %u\n", trial, c, (long long)a, (long long)b, got, want); return 1; }
    }
  }
  std::printf("lookup == scan over 40 sets x 20000 extents\n");
  // the refusals
  {
    RegionsHost bad;
    const calitas_region_t cases[] = {{4, 0, 5, 1}, {-1, 0, 5, 1}, {0, 5, 5, 1}, {0, -1, 5, 1}, {1, 0, 6001, 1}, {0, 0, 5, 0}, {0, 0, 5, 2}};
    for (const calitas_region_t& r : cases)
      if (regions_flatten(ln, [](size_t) { return false; }, &r, 1, 2, bad).empty() || !bad.empty()) { std::fprintf(stderr, "a bad interval was accepted\n"); return 1; }
    const calitas_region_t ok{1, 0, 5, 1};
    if (regions_flatten(ln, [](size_t c) { return c == 1; }, &ok, 1, 2, bad).empty()) { std::fprintf(stderr, "an interval on an absent contig was accepted\n"); return 1; }
    if (regions_flatten(ln, [](size_t) { return false; }, &ok, 1, 9, bad).empty()) { std::fprintf(stderr, "9 classes were accepted\n"); return 1; }
  }

  // 2. the host stage and the merges
  const char* proto = "CTTGCCCCACAGGGCAGTAA";
  const char* pam = "nrg";
  const char* pams[1] = {pam};
  calitas_guide_t g{};
  g.protospacer = proto; g.n_pams = 1; g.pams = pams; g.pam_is_5prime = 0; g.cli_length = 23;
  GuideHost gh;
  std::string e = make_guide_host(g, gh);
  if (!e.empty()) { std::fprintf(stderr, "guide: %s\n", e.c_str()); return 1; }
  calitas_params_t p{};
  p.window_size = 1000; p.max_guide_diffs = 5; p.max_pam_mismatches = 1; p.max_gaps_between_guide_and_pam = 0; p.max_total_diffs = 6; p.max_overlap = 10;
  p.chrom_index = -1;
  std::vector<uint32_t> mm(20 * 25);
  for (auto& v : mm) v = 1 + rng() % 65535;
  for (int uniform = 0; uniform < 2; uniform++) {
    if (uniform) for (auto& v : mm) v = 32768;
    const calitas_score_model_t cm{20, 16384, 49152, mm.data()};
    ScoreModelHost mh;
    e = make_score_model(&cm, 20, mh);
    if (!e.empty()) { std::fprintf(stderr, "model: %s\n", e.c_str()); return 1; }
    mh.regions = &flat;                                   // (the last set of part 1)
    std::vector<calitas_aln_t> alns;
    for (int c = 0; c < n_contigs; c++)
      for (int pos = 30; pos + 60 < lens[c]; pos += 40) {
        calitas_aln_t a{};
        a.contig_index = c; a.window_start = pos / 1000 * 1000; a.start_offset = pos; a.end_offset = pos + 23;
        const bool minus = (pos / 40) & 1;
        a.strand = minus ? '-' : '+';
        a.guide_start_offset = minus ? pos + 3 : pos; a.guide_end_offset = a.guide_start_offset + 20;
        a.score = 2000 - (int)(rng() % 500); a.pam_index = 0; a.n_ops = 23;
        const int edits = (int)(rng() % 4);                         // 0: a perfect hit
        std::memset(a.ops, '=', 23);
        for (int k = 0; k < edits; k++) a.ops[rng() % 20] = 'X';
        alns.push_back(a);
      }
    const uint32_t n_mm = 6, n_gaps = 2, n_pam = 2;
    const size_t cells = 2 * n_mm * n_gaps * n_pam;
    for (uint32_t k : {0u, 1u, 7u, 256u})
      for (uint32_t mask : {0xFFu, 0x1u, 0x6u}) {
        mh.top_k = k; mh.list_mask = mask;
        std::vector<uint64_t> table(cells, 0);
        uint64_t rows = 0;
        ScoreWords whole; whole.top.k = k;
        e = hits_regions(ref, gh, p, mh, alns.data(), alns.size(), n_mm, n_gaps, n_pam, table.data(), &rows, &whole.perfect, &whole.sum_q32, &whole.max_q32,
                         &whole.top, &whole.reg);
        if (!e.empty()) { std::fprintf(stderr, "hits_regions: %s\n", e.c_str()); return 1; }
        // every record's class byte is its extent's class and in the mask; the classes' words sum to the totals
        for (size_t i = 0; i < whole.top.hits.size(); i++) {
          const calitas_top_hit_t& h = whole.top.hits[i];
          if (whole.top.cls[i] != scan_class(iv, h.contig_index, h.coordinate_start, h.coordinate_end) || !((mask >> whole.top.cls[i]) & 1u)) { std::fprintf(stderr, "a record's class\n"); return 1; }
        }
        uint64_t r_sum = 0, s_sum = 0, p_sum = 0, t_sum = 0;
        for (uint32_t c = 0; c < whole.reg.n_classes; c++) { s_sum += whole.reg.words[c * 4]; p_sum += whole.reg.words[c * 4 + 1]; r_sum += whole.reg.words[c * 4 + 3]; }
        for (uint64_t v : whole.reg.tables) t_sum += v;
        if (r_sum != rows || t_sum != rows || s_sum != whole.sum_q32 || p_sum != whole.perfect) { std::fprintf(stderr, "the classes do not sum to the totals\n"); return 1; }
        // the contigs one by one (removeOverlaps never crosses a contig), merged in order, are the whole
        ScoreWords merged; merged.top.k = k;
        for (int c = 0; c < n_contigs; c++) {
          std::vector<calitas_aln_t> part;
          for (const auto& a : alns) if (a.contig_index == c) part.push_back(a);
          std::vector<uint64_t> t2(cells, 0);
          uint64_t r2 = 0;
          ScoreWords piece; piece.top.k = k;
          e = hits_regions(ref, gh, p, mh, part.data(), part.size(), n_mm, n_gaps, n_pam, t2.data(), &r2, &piece.perfect, &piece.sum_q32, &piece.max_q32, &piece.top,
                           &piece.reg);
          if (!e.empty()) { std::fprintf(stderr, "hits_regions (piece): %s\n", e.c_str()); return 1; }
          merged.add(piece);
        }
        const bool same = merged.top.hits.size() == whole.top.hits.size() && merged.top.cls == whole.top.cls && merged.reg.words == whole.reg.words &&
                          merged.reg.tables == whole.reg.tables && merged.sum_q32 == whole.sum_q32 && merged.perfect == whole.perfect && merged.max_q32 == whole.max_q32 &&
                          (whole.top.hits.empty() || std::memcmp(merged.top.hits.data(), whole.top.hits.data(), whole.top.hits.size() * sizeof(calitas_top_hit_t)) == 0);
        std::printf("%s model, k %u, mask %#x: rows %llu perfect %llu listed %zu, merge of the contigs %s\n", uniform ? "uniform" : "distinct", k, mask,
                    (unsigned long long)rows, (unsigned long long)whole.perfect, whole.top.hits.size(), same ? "equal" : "DIFFERENT");
        if (!same) return 1;
      }
  }
  return 0;
}
