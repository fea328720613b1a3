// post.hpp -- host-side stages above the kernels: raw alignment -> GuideAlignment record, the per-window filter,
// removeOverlaps / sort / hits.txt rows.
#pragma once
#include <algorithm>
#include <cstddef>
#include <memory>
#include <string>
#include <vector>

#include "../../include/calitas_hip.h"
#include "common.hpp"
#include "parallel.hpp"
#include "refpack.hpp"
#include "regions.hpp"

namespace calitas {

struct GuideHost {
  std::string protospacer;            // upper case
  std::vector<std::string> pams;      // lower case, as given
  bool pam5 = false;
  int cli_length = 0;
  std::string q;                      // aligner-space query: protospacer, or its reverse complement for a 5' PAM
  std::vector<std::string> pams_q;    // aligner-space PAMs
  // query string of an alignment in guide orientation (GuideAlignment.guide): protospacer+pam or pam+protospacer
  std::string query_for(int pam_index) const;
};

char complement_base(char c);
std::string revcomp_str(const std::string& s);
// Validates and converts; returns an empty string on success, else the error text.
std::string make_guide_host(const calitas_guide_t& g, GuideHost& out);

// Converts one raw kernel record into a GuideAlignment record (SequentialGuideAligner.scala:260-313, GuideAlignment.scala:10-50).
void raw_to_aln(const RawAln& r, const GuideHost& g, int64_t win_a, int64_t win_b, calitas_aln_t& out);

// SequentialGuideAligner.scala:315-320 on one window's alignments (forward list then reverse list, enumeration order).
void window_filter(const calitas_aln_t* alns, int n, int max_total_diffs, int max_overlap, std::vector<int>& kept);

// Padded strings in guide orientation.
void padded_strings(const PackedRef& ref, const GuideHost& g, const calitas_aln_t& a, std::string& pg, std::string& pa, std::string& pt);

// The pieces of a hits.txt row that are the same for every hit of one guide (RH:205-254), and the header line.
struct RowStrings {
  std::string header;                   // the 34 column names + newline
  std::string head;                     // guide_id \t protospacer \t genome_build \t
  std::string tail;                     // aligner \t version \t search_pam \t parameters \t time_stamp \n
  std::string proto_len;
  std::vector<std::string> query;       // per PAM index + 1: the query in guide orientation (GuideAlignment.guide)
  std::vector<std::string> pam_used;    // per PAM index + 1: its lower-case part (RH:229)
};
RowStrings make_row_strings(const PackedRef& ref, const GuideHost& g, const std::string& guide_id, const calitas_params_t& p,
                            const std::string& version, const std::string& time_stamp);

// Compact rows.  270 of a row's ~520 bytes are the same in every row of a call: head (guide_id, protospacer, genome_build) and tail
// (aligner ... time_stamp, ReferenceHit.scala:99-132).  Given row constants with an empty head and "\n" for a tail, the device's row
// kernels write `chromosome \t middle \n` per row -- the same kernels, half the bytes over PCIe -- and the library puts head and tail
// back on the host's worker pool while the next text is on the bus.
void stream_copy(char* dst, const char* src, size_t n);   // memcpy with non-temporal stores (large blocks nobody reads back soon)
RowStrings compact_row_strings(const RowStrings& full);
// The same with genome_build left in the rows: the variant branch's rows have one of their own ("<build>+variants" for a hit that
// touches a variant, ReferenceHit.scala:208), so only guide_id and protospacer are cut; *cut = what was cut from the head.
RowStrings compact_row_strings_keep_build(const RowStrings& full, std::string* cut);
// n bytes of compact rows (`rows` of them) -> full rows at out, which has room for n + rows * (head.size() + tail.size() - 1) bytes.
// Returns the bytes written, or (size_t)-1 when the text does not hold exactly `rows` newline-terminated rows.
size_t expand_rows(const char* compact, size_t n, uint64_t rows, const std::string& head, const std::string& tail, char* out, WorkerPool* pool);
// The same over a text that is still arriving (the pieces of a copy from the device): begin() wakes the workers, which expand what
// arrived() has announced -- the first `bytes` bytes of compact[] are there -- and end() has the caller join in and wait for the
// pieces in hand (complete = false: the copy failed, nothing more will arrive; the result is then (size_t)-1).  head, tail, compact
// and out stay valid until end() has returned.
struct RowExpansion;
std::shared_ptr<RowExpansion> expand_rows_begin(const char* compact, size_t n, uint64_t rows, const std::string& head, const std::string& tail,
                                                char* out, WorkerPool* pool);
void expand_rows_arrived(RowExpansion& job, size_t bytes);
size_t expand_rows_end(RowExpansion& job, bool complete);

// Text of the row of ext[e] (without the newline), for hits whose calitas_ext_hit_t::row is NULL: called from the worker pool, only for
// the hits removeOverlaps kept -- a caller with millions of hits of its own (the variant branch) builds no text for the ones that go.
typedef void (*ExtRowFn)(void* user, uint64_t e, std::string& row);

// hits.txt text for one guide's alignments: malloc'd, NUL-terminated (nullptr when out of memory).
char* hits_tsv(const PackedRef& ref, const GuideHost& g, const std::string& guide_id, const calitas_params_t& p,
               const calitas_aln_t* alns, uint64_t n, const std::string& version, const std::string& time_stamp,
               uint64_t* n_rows, WorkerPool* pool = nullptr, void* (*alloc)(size_t) = nullptr, const calitas_ext_hit_t* ext = nullptr,
               uint64_t n_ext = 0, ExtRowFn ext_row = nullptr, void* ext_user = nullptr);

// The twin of hits_tsv for calitas_hits_counts: removeOverlaps on one guide's alignments, then the kept hits counted by (strand,
// guide_mm, guide_gaps, pam_mm) -- the values hits_tsv writes into the columns of those names -- into table[2 * n_mm * n_gaps * n_pam],
// which the caller has cleared.  *n_rows: the kept hits.  An error text when a hit lies outside the extents, else "".
std::string hits_counts(const PackedRef& ref, const GuideHost& g, const calitas_params_t& p, const calitas_aln_t* alns, uint64_t n, uint32_t n_mm,
                        uint32_t n_gaps, uint32_t n_pam, uint64_t* table, uint64_t* n_rows, WorkerPool* pool = nullptr);

// ---- the specificity score (calitas_search_scores; include/calitas_hip.h has the contract) -----------------------------------------
// A validated calitas_score_model_t.  words: the model as the device holds it -- mismatch[32][5][5] zero-padded behind position L,
// then gap and pam_mismatch (hits.hpp: SCORE_MODEL_WORDS) --, so equal models have equal bytes.
struct ScoreModelHost {
  int L = 0;
  std::vector<uint32_t> words;
  uint32_t top_k = 0;                 // calitas_search_top: the k of the list the call keeps besides the sums (0: a scores call)
  // calitas_search_regions: the context's set (it outlives the call) -- the call classes every kept hit, keeps the sums per class
  // besides, and lists only hits whose class has its bit in list_mask (top_k may be 0 here: no list)
  const RegionsHost* regions = nullptr;
  uint32_t list_mask = ~0u;
  RegionsView regions_dev{};          // ... and the owner's device copy of its tables (null on a host-only context)
  uint32_t mismatch(int i, int g, int t) const { return words[(size_t)i * 25 + (size_t)g * 5 + (size_t)t]; }
  uint32_t gap() const { return words[32 * 25]; }
  uint32_t pam_mismatch() const { return words[32 * 25 + 1]; }
};
// "" or why the model is refused for a guide with a protospacer of guide_len bases.
std::string make_score_model(const calitas_score_model_t* m, int guide_len, ScoreModelHost& out);
// Letter index of the contract: A 0, C 1, G 2, T 3, anything else 4.
inline uint32_t score_letter_index(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
// The score of one hit from its padded columns in guide orientation (the hits.txt columns padded_guide, padded_alignment, padded_target
// and guide_gaps, pam_mm): the contract's loop, 64-bit with a truncation at every step.  false: the row has more upper-case guide
// letters than the model has positions.
bool score_columns(const ScoreModelHost& m, const char* pg, const char* pa, const char* pt, int len, int guide_gaps, int pam_mm, uint64_t* score);

// The k highest-scoring imperfect hits of a piece of a job (calitas_hip.h, calitas_top_t: score descending, the text's order among
// equal scores), best first.  merge: the piece that follows this one in the text -- a stable merge by score, this piece's records
// first among equals, cut at k; that is the top of the two pieces' concatenated text.
// cls: one byte per record, the record's class in a regions call (calitas_regions_t::hit_class; 0 elsewhere) -- it travels with it.
struct TopList {
  uint32_t k = 0;
  std::vector<calitas_top_hit_t> hits;
  std::vector<uint8_t> cls;
  void merge(const TopList& later) {
    if (later.k > k) k = later.k;
    if (later.hits.empty() && hits.size() <= k) return;      // (nothing to merge in: the text fallback adds plain score words per row)
    std::vector<calitas_top_hit_t> out;
    std::vector<uint8_t> out_cls;
    out.reserve(std::min<size_t>(k, hits.size() + later.hits.size()));
    size_t i = 0, j = 0;
    while (out.size() < k && (i < hits.size() || j < later.hits.size())) {
      if (j == later.hits.size() || (i < hits.size() && hits[i].score_q32 >= later.hits[j].score_q32)) { out.push_back(hits[i]); out_cls.push_back(cls[i++]); }
      else { out.push_back(later.hits[j]); out_cls.push_back(later.cls[j++]); }
    }
    hits.swap(out); cls.swap(out_cls);
  }
  // one more hit behind those seen so far (the host stages walk the kept hits in the text's order)
  void push(const calitas_top_hit_t& h, uint8_t c = 0) {
    if (hits.size() == k && (k == 0 || hits.back().score_q32 >= h.score_q32)) return;
    size_t at = hits.size();
    while (at > 0 && hits[at - 1].score_q32 < h.score_q32) at--;
    hits.insert(hits.begin() + (std::ptrdiff_t)at, h);
    cls.insert(cls.begin() + (std::ptrdiff_t)at, c);
    if (hits.size() > k) { hits.pop_back(); cls.pop_back(); }
  }
};

// hits_counts plus the score: the kept hits counted into table[] as there, and those with an edit scored from their ops (guide
// orientation) and the packed reference's bases; a kept hit without one is counted in *perfect.
std::string hits_scores(const PackedRef& ref, const GuideHost& g, const calitas_params_t& p, const ScoreModelHost& model, const calitas_aln_t* alns,
                        uint64_t n, uint32_t n_mm, uint32_t n_gaps, uint32_t n_pam, uint64_t* table, uint64_t* n_rows, uint64_t* perfect,
                        uint64_t* sum_q32, uint64_t* max_q32, WorkerPool* pool = nullptr);
// hits_scores plus the list: top->k is what the caller asks for, top->hits receives the records.
std::string hits_top(const PackedRef& ref, const GuideHost& g, const calitas_params_t& p, const ScoreModelHost& model, const calitas_aln_t* alns,
                     uint64_t n, uint32_t n_mm, uint32_t n_gaps, uint32_t n_pam, uint64_t* table, uint64_t* n_rows, uint64_t* perfect,
                     uint64_t* sum_q32, uint64_t* max_q32, TopList* top, WorkerPool* pool = nullptr);
// hits_top of a regions call (model.regions set): every kept hit classed from its record's coordinates, the sums and tables per class
// into *reg besides the totals, and only hits whose class is in model.list_mask offered to the list.
std::string hits_regions(const PackedRef& ref, const GuideHost& g, const calitas_params_t& p, const ScoreModelHost& model, const calitas_aln_t* alns,
                         uint64_t n, uint32_t n_mm, uint32_t n_gaps, uint32_t n_pam, uint64_t* table, uint64_t* n_rows, uint64_t* perfect,
                         uint64_t* sum_q32, uint64_t* max_q32, TopList* top, RegionWords* reg, WorkerPool* pool = nullptr);

}  // namespace calitas
