// top_asan.cpp -- the host stage of a top call (hits_top) and the merges of its lists (TopList::push / merge), as a stand-alone program
// for a run under AddressSanitizer: host objects only, no device, nothing loaded into another process.
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address -fno-omit-frame-pointer tools/top_asan.cpp calitas_amd/csrc/post.cpp \
//         calitas_amd/csrc/refpack.cpp -pthread -o top_asan && ./top_asan
// The alignments are made up (a planted site every 40 bases, a few 'X' columns each, both strands): the run is about memory, and about
// the merge of pieces against the list of the whole.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../calitas_amd/csrc/post.hpp"

using namespace calitas;

int main() {
  std::mt19937 rng(7);
  const int n_contigs = 3, len = 6000;
  std::vector<std::string> seqs, names;
  for (int c = 0; c < n_contigs; c++) {
    std::string s((size_t)len, 'A');
    for (char& ch : s) ch = "ACGT"[rng() & 3];
    seqs.push_back(s); names.push_back("c" + std::to_string(c));
  }
  std::vector<const char*> nm; std::vector<uint64_t> ln; std::vector<const uint8_t*> bs;
  for (int c = 0; c < n_contigs; c++) { nm.push_back(names[(size_t)c].c_str()); ln.push_back((uint64_t)len); bs.push_back((const uint8_t*)seqs[(size_t)c].data()); }
  PackedRef ref;
  pack_reference(ref, n_contigs, nm.data(), ln.data(), bs.data(), "asan", 2);

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
    std::vector<calitas_aln_t> alns;
    for (int c = 0; c < n_contigs; c++)
      for (int pos = 30; pos + 60 < len; pos += 40) {
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
    for (uint32_t k : {1u, 7u, 256u}) {
      std::vector<uint64_t> table(2 * n_mm * n_gaps * n_pam, 0);
      uint64_t rows = 0, perfect = 0, sum = 0, mx = 0;
      TopList whole; whole.k = k;
      e = hits_top(ref, gh, p, mh, alns.data(), alns.size(), n_mm, n_gaps, n_pam, table.data(), &rows, &perfect, &sum, &mx, &whole);
      if (!e.empty()) { std::fprintf(stderr, "hits_top: %s\n", e.c_str()); return 1; }
      // the contigs one by one (removeOverlaps never crosses a contig), merged in order, are the whole
      TopList merged; merged.k = k;
      for (int c = 0; c < n_contigs; c++) {
        std::vector<calitas_aln_t> part;
        for (const auto& a : alns) if (a.contig_index == c) part.push_back(a);
        std::vector<uint64_t> t2(table.size(), 0);
        uint64_t r2 = 0, p2 = 0, s2 = 0, m2 = 0;
        TopList piece; piece.k = k;
        e = hits_top(ref, gh, p, mh, part.data(), part.size(), n_mm, n_gaps, n_pam, t2.data(), &r2, &p2, &s2, &m2, &piece);
        if (!e.empty()) { std::fprintf(stderr, "hits_top (piece): %s\n", e.c_str()); return 1; }
        merged.merge(piece);
      }
      const bool same = merged.hits.size() == whole.hits.size() &&
                        (whole.hits.empty() || std::memcmp(merged.hits.data(), whole.hits.data(), whole.hits.size() * sizeof(calitas_top_hit_t)) == 0);
      std::printf("%s model, k %u: rows %llu perfect %llu listed %zu, merge of the contigs %s\n", uniform ? "uniform" : "distinct", k,
                  (unsigned long long)rows, (unsigned long long)perfect, whole.hits.size(), same ? "equal" : "DIFFERENT");
      if (!same || whole.hits.size() != std::min<uint64_t>(k, rows - perfect)) return 1;
    }
  }
  return 0;
}
