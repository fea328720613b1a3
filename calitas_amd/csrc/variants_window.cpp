// variants_window.cpp -- the windows of the variant branch: what each is made of (the walk over the VCF's records) and how it is built.
//
// RESTATEMENT, NOT DESIGN: four host functions below follow the reference statement by statement, because what they compute IS the
// contract -- the order in which allele combinations are enumerated decides the order of the variant windows (and so SR:622's arrival
// order of their hits), and the shape of a window's CIGAR decides every lifted coordinate:
//   ref_offset_at          = VariantWindow.refOffsetAtBaseOffset   SearchReference.scala:133-156
//   is_valid               = VariantSet.isValid                     SearchReference.scala:182-193
//   build_window           = buildVariantWindow                     SearchReference.scala:263-323  (windowStart / windowEnd, the right-to-left
//                            patch, refPos / baseOffset / precedingMatch, the M / I / D case split, the same `require`)
//   allele_combos_counts   = alleleCombos(Seq[Int])                 SearchReference.scala:377-399  (denominators, group size, (allele + 1) % n)
// The reference pins them by its own vectors V1-V9 (SearchReferenceTest.scala:150-295); here they are pinned end to end, by
// tests/test_gpu_variants.py against the oracle and against the Python twin (tests/variants_twin.py, which tests/test_variants_host.py
// holds against those vectors).  The walk around them (nextChunk / reChunk SR:326-347, alleleCombos SR:351-369) keeps the reference's
// order of windows; the lists, arenas and batches it works with have no counterpart there.
#include <algorithm>

#include "variants_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

// alleleCombos(counts) SR:377-399: every combination of allele indices, the first variant varying slowest
std::vector<std::vector<int>> allele_combos_counts(const std::vector<int>& counts) {
  size_t total = 1;
  for (int c : counts) total *= (size_t)c;
  std::vector<std::vector<int>> results(total, std::vector<int>(counts.size(), 0));
  size_t denom = 1;
  for (size_t i = 0; i < counts.size(); i++) {
    denom *= (size_t)counts[i];
    const size_t group = total / denom;
    size_t j = 0;
    int allele = 0;
    while (j < total) {
      for (size_t k = 0; k < group; k++) results[j++][i] = allele;
      allele = (allele + 1) % counts[i];
    }
  }
  return results;
}

bool is_valid(const std::vector<const Var*>& vs) {   // VariantSet.isValid SR:182-193
  for (size_t i = 0; i + 1 < vs.size(); i++) {
    const Var &a = *vs[i], &b = *vs[i + 1];
    const int s1 = a.pos, e1 = a.pos + (int)a.ref.size() - 1, s2 = b.pos, e2 = b.pos + (int)b.ref.size() - 1;
    if (a.chrom == b.chrom && s1 <= e2 && e1 >= s2) return false;
  }
  return true;
}

// Upper-cased bases [s, e) of a contig (what the reference reads after toUpperCase): 2-bit decode, exceptions through base_upper.
static void upper_span(const PackedRef& ref, int contig, long s, long e, std::string& out) {
  const ContigInfo& c = ref.contigs[contig];
  out.resize((size_t)std::max(0L, e - s));
  for (long q = s; q < e; q++) {
    const uint64_t gpos = c.gbase + (uint64_t)q;
    out[(size_t)(q - s)] = ((ref.mask[gpos >> 5] >> (gpos & 31)) & 1u) ? ref.base_upper(gpos) : "ACGT"[(ref.codes[gpos >> 4] >> ((gpos & 15) * 2)) & 3u];
  }
}

// buildVariantWindow SR:263-323.  The window's pieces are appended to A (w gets the counts, `mark` where they start); tmp / ctmp are scratch.
std::string build_window(const Var* const* variants, const int* alleles, size_t nv, int contig, const PackedRef& ref, int padding, Arena& A,
                         std::string& tmp, std::vector<CigarEl>& ctmp, Window& w, ArenaMark& mark) {
  const int window_start = std::max(1, variants[0]->pos - padding);
  const int window_end = std::min((int)ref.contigs[contig].len, variants[nv - 1]->end + padding);
  w.contig = contig; w.start = window_start;
  mark = ArenaMark{A.bases.size(), A.alleles.size(), A.cigars.size()};
  upper_span(ref, contig, window_start - 1, std::max(window_start - 1, window_end), tmp);
  for (size_t i = 0; i < nv; i++) {
    const Var* v = variants[i];
    const int a = alleles[i] - 1;
    A.alleles.push_back(Allele{v, a, (size_t)a < v->afs.size() ? v->afs[a] : 0.0f});
  }
  const Allele* const wv = A.alleles.data() + mark.alleles;
  w.nv = (int)nv;
  for (size_t k = nv; k-- > 0;) {                     // right to left, so earlier offsets stay valid
    const Allele& al = wv[k];
    const int i = al.v->pos - window_start;
    if (i < 0 || (size_t)i > tmp.size()) return "variant outside its window";
    tmp.replace((size_t)i, std::min(al.v->ref.size(), tmp.size() - (size_t)i), al.v->alts[al.alt]);
  }
  ctmp.clear();
  int ref_pos = window_start, base_off = 0;
  for (size_t k = 0; k < nv; k++) {
    const Allele& al = wv[k];
    const int pm = al.v->pos - ref_pos;
    if (pm > 0) { ctmp.push_back({'M', pm}); ref_pos += pm; base_off += pm; }
    const int rl = (int)al.v->ref.size(), alen = (int)al.v->alts[al.alt].size();
    if (rl == alen) ctmp.push_back({'M', rl});
    else if (rl == 1 && alen > 1) { ctmp.push_back({'M', 1}); ctmp.push_back({'I', alen - 1}); }
    else if (rl > 1 && alen == 1) { ctmp.push_back({'M', 1}); ctmp.push_back({'D', rl - 1}); }
    else { ctmp.push_back({'D', rl}); ctmp.push_back({'I', alen}); }
    ref_pos += rl; base_off += alen;
  }
  ctmp.push_back({'M', (int)tmp.size() - base_off});
  for (const CigarEl& e : ctmp) {                      // Cigar.coalesce
    if (A.cigars.size() > mark.cigars && A.cigars.back().op == e.op) A.cigars.back().n += e.n; else A.cigars.push_back(e);
  }
  w.nc = (int)(A.cigars.size() - mark.cigars);
  long on_query = 0;
  for (size_t k = mark.cigars; k < A.cigars.size(); k++) if (A.cigars[k].op == 'M' || A.cigars[k].op == 'I') on_query += A.cigars[k].n;
  if (on_query != (long)tmp.size()) return "requirement failed: cigar length on query != bases";
  A.bases.insert(A.bases.end(), tmp.begin(), tmp.end());
  w.len = (int)tmp.size();
  return "";
}

// refOffsetAtBaseOffset SR:133-156
bool ref_offset_at(const Window& w, int offset, bool preceding, int& out) {
  auto on_q = [](const CigarEl& e) { return (e.op == 'M' || e.op == 'I') ? e.n : 0; };
  auto on_t = [](const CigarEl& e) { return (e.op == 'M' || e.op == 'D') ? e.n : 0; };
  if (offset == w.len) {
    int t = 0;
    for (int k = 0; k < w.nc; k++) t += on_t(w.cigar[k]);
    out = w.start - 1 + t;
    return true;
  }
  int ref_off = w.start - 1, base_off = 0;
  int k = 0;
  while (k < w.nc && offset >= base_off + on_q(w.cigar[k])) { ref_off += on_t(w.cigar[k]); base_off += on_q(w.cigar[k]); k++; }
  if (k >= w.nc) return false;
  const char op = w.cigar[k].op;
  if (op == 'I') { out = preceding ? ref_off - 1 : ref_off; return true; }
  if (op == 'M') { out = ref_off + (offset - base_off); return true; }
  return false;                                       // "Query bases can't be present at operator D."
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------------
// variantWindowIterator SR:217-256 with nextChunk / reChunk SR:326-347.  The iterator itself only lists what each window is made
// of (variants and alleles: a Spec); a full batch of windows is then built on the worker pool and handed to the GPU by the builder
// stage (round 5: this thread used to wait for every batch's build, 0.15-0.3 s per call at BASELINE config 5's size, with the list
// of the next batch standing still meanwhile).

// The windows of a list (builder thread): build_window on the pool, the batch to one of the aligners.
int VariantSearch::build_spec(const Spec& sp, std::string& e_out) {
  const size_t n = sp.contig.size();
  if (n == 0) return CALITAS_OK;
  const auto t_build = Clock::now();
  Batch b;
  b.wins.resize(n + 1);
  b.arenas.resize((size_t)ctx->pool->size());
  std::vector<std::string> errs((size_t)ctx->pool->size());
  ctx->pool->for_blocks(n, [&](size_t lo, size_t hi, int tid) {
    Arena& A = b.arenas[(size_t)tid];
    std::string tmp;
    std::vector<CigarEl> ctmp;
    std::vector<ArenaMark> marks(hi - lo);
    A.bases.reserve((hi - lo) * (size_t)(2 * padding + 8));
    for (size_t k = lo; k < hi && errs[(size_t)tid].empty(); k++)
      errs[(size_t)tid] = build_window(sp.v.data() + sp.off[k], sp.a.data() + sp.off[k], sp.off[k + 1] - sp.off[k], sp.contig[k], ref,
                                       padding, A, tmp, ctmp, b.wins[k], marks[k - lo]);
    for (size_t k = lo; k < hi; k++) {                         // the arena is complete: the views get their pointers
      Window& w = b.wins[k];
      w.chunk = sp.chunk[k];
      w.bases = A.bases.data() + marks[k - lo].bases; w.variants = A.alleles.data() + marks[k - lo].alleles; w.cigar = A.cigars.data() + marks[k - lo].cigars;
    }
  });
  for (auto& e : errs) if (!e.empty() && e_out.empty()) e_out = e;
  tm.build += ms_since(t_build);
  if (trace_stages) std::fprintf(stderr, "[calitas] search_variants: a batch of %zu windows (contig %d ..) built %.1f .. %.1f ms\n", n, sp.contig[0], ms_since(t_call) - ms_since(t_build), ms_since(t_call));
  if (!e_out.empty()) return CALITAS_EINVAL;
  return hand_over(std::move(b), n);
}

// the windows listed so far go to the builder stage
int VariantSearch::flush_spec() {
  if (walked.spec.contig.empty()) return CALITAS_OK;
  auto held = std::make_shared<Spec>(std::move(walked.spec));
  walked.spec = Spec();
  return builder.enqueue([this, held](std::string& e) { return build_spec(*held, e); }, 2, &tm.wait_builder);
}

int VariantSearch::emit(const Var* const* vs, const int* al, size_t nv, int contig) {
  Spec& spec = walked.spec;
  spec.v.insert(spec.v.end(), vs, vs + nv);
  spec.a.insert(spec.a.end(), al, al + nv);
  spec.off.push_back((uint32_t)spec.v.size());
  spec.contig.push_back(contig);
  spec.chunk.push_back(walked.chunk_serial);
  walked.windows_total++;
  return spec.contig.size() >= kBatch ? flush_spec() : CALITAS_OK;
}

// The contigs before `upto` have all their windows emitted: what is listed goes to the builder, and the contigs' "finish" behind it.
int VariantSearch::finish_contigs(size_t upto) {
  if (upto <= walked.contigs_asked) return CALITAS_OK;
  const int r = flush_spec();
  if (r) return r;
  walked.contigs_asked = upto;
  // The contig's entries are made on the lifter thread, behind the lift of the contig's last batch, while this thread goes on with
  // the next contig -- no waiting for the stages to run dry at each of the 25 contig ends.  (Measured three times: on the one aligner
  // thread there was at first, that thread carried 1.26 s of host work one after the other, variant half 1.54 against 1.38 s; on the
  // lifter with two aligners but a pool that let one caller in at a time, the same 1.35-1.41 s; with the pool's shares, 0.95-1.04
  // against 1.25-1.32 s, step 1.36-1.38 against 1.60-1.62 s on one box, alternating.)
  // (through the builder stage, behind the contig's last batch: the batches are numbered where they are handed on)
  return builder.enqueue([this, upto](std::string&) -> int { return hand_over_finish(upto); }, 2, &tm.wait_builder);
}

// The calling thread from the first variant to the last window handed over; the reader thread is joined on the way out.
int VariantSearch::walk() {
  const ScopedMs timed{tm.walk};
  int rc = CALITAS_OK;
  uint32_t& chunk_serial = walked.chunk_serial;
  const int max_variants = p.max_variants;
  size_t ci = 0, i = 0;
  // (three million chunks per call at full size: the vectors are reused, and a chunk's contig is looked up when the contig changes --
  // a search through the 25 names per chunk was a third of this thread's 0.38 s in the loop)
  std::vector<const Var*> chunk, sub;
  size_t ci_of_contig = (size_t)-1;
  int contig = -1;
  while (vcf.have(i) && err.empty() && rc == CALITAS_OK) {
    chunk.assign(1, &vcf[i]);
    const Var* last = &vcf[i];
    i++;
    while (vcf.have(i) && vcf[i].chrom == last->chrom && vcf[i].pos <= last->end + padding) { last = &vcf[i]; chunk.push_back(last); i++; }
    while (ci < order.size() && order[ci] != chunk[0]->chrom) ci++;
    if (ci >= order.size()) { err = "next on empty iterator (VCF contig " + chunk[0]->chrom + " not in reference order)"; break; }
    if (ci != ci_of_contig) {
      contig = -1;
      for (size_t k = 0; k < ref.names.size(); k++) if (ref.names[k] == order[ci]) { contig = (int)k; break; }
      ci_of_contig = ci;
    }
    chunk_serial++;
    if ((size_t)contig > walked.contigs_asked) { rc = finish_contigs((size_t)contig); if (rc || !err.empty()) break; }   // the contigs before this one are complete: their entries are made behind their last batch
    for (size_t s = 0; s < chunk.size() && err.empty() && rc == CALITAS_OK; s++) {
      sub.clear();
      for (size_t k = s; k < chunk.size(); k++) { if (chunk[k]->pos - chunk[s]->end > padding) break; sub.push_back(chunk[k]); }
      // alleleCombos SR:351-369
      if ((int)sub.size() > max_variants || sub.size() == 1) {       // (a single variant: the same windows, without the tables)
        const Var* v = sub[0];
        for (size_t a = 0; a < v->alts.size() && err.empty() && rc == CALITAS_OK; a++) { const int al = (int)a + 1; rc = emit(&v, &al, 1, contig); }
      } else {
        std::vector<int> counts;
        for (const Var* v : sub) counts.push_back(1 + (int)v->alts.size());
        for (const std::vector<int>& alleles : allele_combos_counts(counts)) {
          std::vector<const Var*> sv; std::vector<int> sa;
          for (size_t k = 0; k < sub.size(); k++) if (alleles[k] != 0) { sv.push_back(sub[k]); sa.push_back(alleles[k]); }
          if (sv.empty() || !is_valid(sv)) continue;
          rc = emit(sv.data(), sa.data(), sv.size(), contig);
          if (rc || !err.empty()) break;
        }
      }
    }
  }
  vcf_reader.t.join();
  if (!vcf_err.empty() && err.empty()) { err = vcf_err; if (rc == CALITAS_OK) rc = CALITAS_EIO; }
  if (rc == CALITAS_OK && err.empty()) rc = finish_contigs(nc);
  return rc;
}

}  // namespace calitas
