// sites_host.cpp -- calitas_find_sites / calitas_count_sites / calitas_find_sites_host and their _filtered forms: the pattern and the
// filter both implementations share, the host twin (a base-by-base walk over the packed reference) and the driver of sites.hip's two
// passes.  calitas_count_copies / calitas_count_copies_host: the query keys and their table, the host twin and the driver of the copies
// kernel.  calitas_count_near / calitas_count_near_host: the pieces' bucket tables, the host twin (plain Hamming distances, no buckets) and
// the driver of the near kernel.  calitas_score_near / calitas_score_near_host: the same driver with the model's packed table behind the
// offsets and rows of M + 3 counters, the host twin (the score letter by letter from the caller's table) and the correction of sums and
// maxima around a U.  calitas_list_near / calitas_list_near_host: the near driver for the counts, the layout of a stretch of records per
// distinct query, the pass's second run and the order kernel (near_list.hip), the patch of the stretches beside a U, and the host twin
// (every pair a record, every stretch through std::sort).  calitas_find_sites_scored / calitas_find_sites_scored_host: the model's checks
// and its folded table, the per-site score base by base, the host twin, and the driver of activity.hip's kernels behind the site
// kernel's two passes with the correction of records and scores beside a U.  calitas_find_sites_regions / calitas_count_sites_regions and
// their host twins: the checks, the presence table, the host twin (every record classed through the host's flattened set) and the driver
// of site_regions.hip's kernels around the site kernel's two passes, with the records beside a U classed on the host.  calitas_find_site_pairs /
// calitas_count_site_pairs and their host twins: the checks, the one walk over a sorted listing (pair_walk) that the twins and the
// listings beside a U share, and the driver of site_pairs.hip's kernels behind the site kernel's two passes.  calitas_find_allele_sites / calitas_count_allele_sites and
// their host twins: the checks, the twin (a base-by-base walk with one base replaced) that also decides the SNVs beside a U, and the
// driver of allele_sites.hip's two kernels.  calitas_find_edit_sites / calitas_count_edit_sites and their host twins: the editor's
// checks, the twin (a base-by-base walk of the background allele on the SNV's strand) that also decides the SNVs beside a U, and the
// driver of edit_sites.hip's two kernels.  calitas_find_sites_microhomology / calitas_find_sites_microhomology_host: the model's checks, the
// score of one site as a diagonal walk over letters, the host twin, and the driver of microhomology.hip's kernels behind the site
// kernel's two passes with the correction of records and scores beside a U.  No reference counterpart.
#include "sites.hpp"
#include "site_regions.hpp"
#include "tuning.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <unordered_map>

namespace calitas {

std::string make_site_patterns(const GuideHost& gh, SitePatterns& out) {
  std::memset(&out, 0, sizeof(out));
  const int L = (int)gh.protospacer.size();
  out.pamless = gh.pams.empty() ? 1 : 0;
  out.n_pams = gh.pams.empty() ? 1 : (int)gh.pams.size();
  out.proto_len = L;
  for (int k = 0; k < out.n_pams; k++) {
    const std::string pam = gh.pams.empty() ? std::string() : gh.pams[(size_t)k];
    const int pl = (int)pam.size();
    const std::string strand_space = gh.pam5 ? pam + gh.protospacer : gh.protospacer + pam;
    for (int st = 0; st < 2; st++) {
      // what the forward text shows: the pattern itself on '+', its reverse complement on '-' (the PAM changes sides)
      const std::string q = st ? revcomp_str(strand_space) : strand_space;
      const bool pam_left = (gh.pam5 != 0) != (st != 0);
      SitePattern& sp = out.p[k][st];
      sp.lo = pam_left ? -pl : 0;
      sp.hi = sp.lo + L + pl;
      sp.pam_len = pl;
      sp.pam_off = pam_left ? -pl : L;
      for (uint32_t& w : sp.sets) w = 0xFFFFFFFFu;
      for (int i = 0; i < (int)q.size(); i++) {
        const uint32_t set = (uint32_t)iupac_mask((unsigned char)q[(size_t)i]);
        if (set == 0) return std::string("the pattern has a non-IUPAC character: ") + q[(size_t)i];
        const int at = 16 + sp.lo + i;            // 0 .. 63
        sp.sets[at >> 3] &= ~((15u ^ set) << (4 * (at & 7)));
      }
    }
  }
  return "";
}

namespace {

// 2-bit code of a plain base (A C G T in either case, U), -1 for everything else; *u: it is a U (kept as an exception run)
inline int plain_code(const PackedRef& ref, uint64_t g, bool* u) {
  if ((ref.mask[g >> 5] >> (g & 31)) & 1u) {
    const Run* r = ref.run_at(g);
    if (r && (r->ch == 'U' || r->ch == 'u')) { *u = true; return 3; }
    return -1;
  }
  return (int)((ref.codes[g >> 4] >> ((g & 15) * 2)) & 3u);
}

}  // namespace

std::string make_site_filter(const calitas_site_filter_t& f, int L, SiteFilterDev& out) {
  std::memset(&out, 0, sizeof(out));
  const int gc_max = std::min<int>(f.gc_max, L);
  if ((int)f.gc_min > gc_max) return "site filter: gc_min exceeds gc_max (or the protospacer's length)";
  if (f.reserved != 0) return "site filter: reserved must be 0";
  if (f.n_motifs > 8) return "site filter: n_motifs exceeds 8";
  out.gc_min = f.gc_min; out.gc_max = gc_max;
  for (int b = 0; b < 4; b++) {
    const int r = f.max_run[b] < L ? f.max_run[b] : 0;         // a run of L or more does not fit: no limit
    out.max_run[0][b] = r;                                     // '+': the forward base is the guide's
    out.max_run[1][3 - b] = r;                                 // '-': its complement's
  }
  out.n_motifs = 0;
  for (int m = 0; m < (int)f.n_motifs; m++) {
    const std::string at = "site filter: motifs[" + std::to_string(m) + "]";
    std::string text;
    for (int i = 0; i < 16 && f.motifs[m][i]; i++) text += f.motifs[m][i];
    if (text.empty()) return at + " is empty";
    if ((int)text.size() > L) return at + " is longer than the protospacer";
    bool all_n = true;
    for (char ch : text) {
      const int set = iupac_mask((unsigned char)ch);
      if (set == 0) return at + " has a non-IUPAC character: " + ch;
      all_n = all_n && set == 15;
    }
    if (all_n) return at + " is made of N only";
    const std::string shown[2] = {text, revcomp_str(text)};   // what the forward text shows of an occurrence, left to right
    for (int st = 0; st < 2; st++) {
      uint32_t sets[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
      for (int i = 0; i < (int)text.size(); i++) {
        const uint32_t set = (uint32_t)iupac_mask((unsigned char)shown[st][(size_t)i]);
        sets[i >> 3] &= ~((15u ^ set) << (4 * (i & 7)));
      }
      int e = 0;                                               // the same string from another motif or strand: one entry
      while (e < out.n_motifs && !(out.motif[e].len == (int32_t)text.size() && out.motif[e].sets[0] == sets[0] && out.motif[e].sets[1] == sets[1])) e++;
      if (e == out.n_motifs) {
        out.n_motifs++;
        out.motif[e].len = (int32_t)text.size(); out.motif[e].strands = 0; out.motif[e].sets[0] = sets[0]; out.motif[e].sets[1] = sets[1];
      }
      out.motif[e].strands |= 1u << st;
    }
  }
  return "";
}

bool site_passes(const PackedRef& ref, int contig, int64_t protospacer_start, int L, int strand, const calitas_site_filter_t& f) {
  const uint64_t g0 = ref.contigs[(size_t)contig].gbase + (uint64_t)protospacer_start;
  int code[MAX_L];                                             // the guide's bases, 5' to 3'
  for (int i = 0; i < L; i++) {
    bool u = false;
    const int c = plain_code(ref, g0 + (uint64_t)(strand ? L - 1 - i : i), &u);
    code[i] = strand ? 3 - c : c;
  }
  int gc = 0;
  for (int i = 0; i < L; i++) gc += code[i] == 1 || code[i] == 2;
  if (gc < (int)f.gc_min || gc > std::min<int>(f.gc_max, L)) return false;
  for (int i = 0, run = 0; i < L; i++) {
    run = (i > 0 && code[i] == code[i - 1]) ? run + 1 : 1;
    const int limit = f.max_run[code[i]];
    if (limit > 0 && run > limit) return false;
  }
  for (int m = 0; m < (int)f.n_motifs; m++) {
    int len = 0;
    while (len < 16 && f.motifs[m][len]) len++;
    for (int at = 0; at + len <= L; at++) {
      bool hit = true;
      for (int i = 0; i < len && hit; i++) hit = ((iupac_mask((unsigned char)f.motifs[m][i]) >> code[at + i]) & 1) != 0;
      if (hit) return false;
    }
  }
  return true;
}

namespace {

// The first PAM whose pattern matches at protospacer start p on strand st with its footprint inside [r_start, r_end), or -1.
// u_plain: a U is a T, as the contract has it; otherwise it is the exception base the kernel sees.  *with_u: the match's footprint holds a U.
int first_pam(const PackedRef& ref, const SitePatterns& pat, uint64_t gbase, int64_t p, int st, int64_t r_start, int64_t r_end, bool u_plain,
              bool* with_u) {
  for (int k = 0; k < pat.n_pams; k++) {
    const SitePattern& sp = pat.p[k][st];
    if (p + sp.lo < r_start || p + sp.hi > r_end) continue;
    bool ok = true, u = false;
    for (int d = sp.lo; d < sp.hi && ok; d++) ok = plain_code(ref, gbase + (uint64_t)(p + d), &u) >= 0 && (u_plain || !u);
    for (int d = sp.lo; d < sp.hi && ok; d++) {
      const uint32_t set = (sp.sets[(d + 16) >> 3] >> (4 * ((d + 16) & 7))) & 15u;
      ok = ((set >> plain_code(ref, gbase + (uint64_t)(p + d), &u)) & 1u) != 0;
    }
    if (ok) { *with_u = u; return k; }
  }
  return -1;
}

calitas_site_t site_record(const SitePatterns& pat, int contig, int64_t p, int st, int k) {
  const SitePattern& sp = pat.p[k][st];
  calitas_site_t s;
  s.contig_index = contig; s.protospacer_start = (int32_t)p; s.pam_start = pat.pamless ? -1 : (int32_t)(p + sp.pam_off);
  s.strand = st ? '-' : '+'; s.pam_index = pat.pamless ? (int8_t)-1 : (int8_t)k; s.pam_length = (uint8_t)sp.pam_len;
  s.protospacer_length = (uint8_t)pat.proto_len;
  return s;
}

}  // namespace

void host_sites(const PackedRef& ref, const SitePatterns& pat, const calitas_site_filter_t* filter, int contig, int64_t p_lo, int64_t p_hi,
                int64_t r_start, int64_t r_end, std::vector<calitas_site_t>& out, std::vector<calitas_site_t>* kernel_has) {
  const uint64_t gbase = ref.contigs[(size_t)contig].gbase;
  for (int64_t p = std::max(p_lo, r_start); p < std::min(p_hi, r_end); p++) {
    for (int st = 0; st < 2; st++) {
      bool u = false, unused = false;
      const int k = first_pam(ref, pat, gbase, p, st, r_start, r_end, true, &u);
      if (k < 0) continue;
      // the protospacer decides, whichever PAM matched: what holds for this record holds for the kernel's at the same place
      if (filter && !site_passes(ref, contig, p, pat.proto_len, st, *filter)) continue;
      if (!kernel_has) { out.push_back(site_record(pat, contig, p, st, k)); continue; }
      // A match without a U: no earlier PAM matches even with U as T, so the kernel has this very record.  With one: the kernel has
      // either nothing here or a LATER PAM whose own footprint is clean (PAMs differ in length) -- that record has to go.
      if (!u) continue;
      out.push_back(site_record(pat, contig, p, st, k));
      const int seen = first_pam(ref, pat, gbase, p, st, r_start, r_end, false, &unused);
      if (seen >= 0) kernel_has->push_back(site_record(pat, contig, p, st, seen));
    }
  }
}

struct SitesWork {
  SiteTables* d_pat = nullptr;       // the patterns and, behind them, the filter of the call in flight
  uint32_t* d_count = nullptr;
  uint64_t* d_off = nullptr;
  size_t blocks_cap = 0;
  unsigned long long* d_totals = nullptr;
  size_t totals_cap = 0;
  SiteRecord* d_out = nullptr;
  size_t out_cap = 0;
  // calitas_count_copies: the table of query keys (slots) and the distinct keys' counters (+ 1: the error flag)
  uint64_t* d_keys = nullptr;
  uint32_t* d_key_index = nullptr;
  size_t slots_cap = 0;
  unsigned long long* d_key_counts = nullptr;
  size_t key_counts_cap = 0;
  // calitas_count_near: the pieces' bucket tables and member lists (its counters are d_key_counts)
  uint32_t* d_near_offsets = nullptr;
  size_t near_offsets_cap = 0;
  uint4* d_near_members = nullptr;
  size_t near_members_cap = 0;
  // calitas_list_near: the stretches' first records, {cursor, length} per distinct key (+ 1: the error flag), the keys whose stretches
  // are put in order, and the records as the pass stored them (list_in) and in position order (list_out)
  uint64_t* d_list_base = nullptr;
  uint32_t* d_list_cursors = nullptr;
  uint32_t* d_list_order = nullptr;
  size_t list_keys_cap = 0;
  NearHit* d_list_in = nullptr;
  NearHit* d_list_out = nullptr;
  size_t list_cap = 0;
  // calitas_find_sites_scored: the model's folded table, a score per record of d_out, the workgroups' kept counts and their scan, and
  // the kept records and scores in order
  int32_t* d_act_table = nullptr;
  int32_t* d_act_scores = nullptr;
  size_t act_scores_cap = 0;
  uint32_t* d_act_count = nullptr;
  uint64_t* d_act_off = nullptr;
  size_t act_blocks_cap = 0;
  SiteRecord* d_act_out = nullptr;
  int32_t* d_act_out_scores = nullptr;
  size_t act_out_cap = 0;
  // calitas_find_sites_regions: the device copy of the context's presence table (one byte per segment of the packed space), a class byte per record of d_out, the workgroups' kept counts and their scan, the 16
  // (class, strand) counters, and the kept records and classes in order
  uint8_t* d_presence = nullptr;
  size_t presence_cap = 0;
  uint64_t presence_regions = 0, presence_ref = ~0ull;   // the set and the reference d_presence was made from
  uint8_t* d_reg_cls = nullptr;
  size_t reg_cls_cap = 0;
  uint32_t* d_reg_count = nullptr;
  uint64_t* d_reg_off = nullptr;
  size_t reg_blocks_cap = 0;
  unsigned long long* d_reg_cells = nullptr;
  SiteRecord* d_reg_out = nullptr;
  uint8_t* d_reg_out_cls = nullptr;
  size_t reg_out_cap = 0;
  // calitas_find_site_pairs: a count per record of d_out, the workgroups' sums and their scan, the four per-orientation counters, and
  // the pairs in order
  uint32_t* d_pair_lanes = nullptr;
  size_t pair_lanes_cap = 0;
  uint32_t* d_pair_count = nullptr;
  uint64_t* d_pair_off = nullptr;
  size_t pair_blocks_cap = 0;
  unsigned long long* d_pair_by = nullptr;
  SitePair* d_pair_out = nullptr;
  size_t pair_out_cap = 0;
  // calitas_find_allele_sites: the SNVs, a count and a status byte per SNV, the workgroups' sums and their scan, the per-kind counters,
  // and the records in order
  Snv* d_snvs = nullptr;
  uint32_t* d_al_lanes = nullptr;
  uint8_t* d_al_status = nullptr;
  size_t al_snvs_cap = 0;
  uint32_t* d_al_count = nullptr;
  uint64_t* d_al_off = nullptr;
  size_t al_blocks_cap = 0;
  unsigned long long* d_al_by = nullptr;
  AlleleSite* d_al_out = nullptr;
  size_t al_out_cap = 0;
  // calitas_find_sites_microhomology: a score per record of d_out, the workgroups' kept counts and their scan, and the kept records and
  // scores in order
  MhScore* d_mh_scores = nullptr;
  size_t mh_scores_cap = 0;
  uint32_t* d_mh_count = nullptr;
  uint64_t* d_mh_off = nullptr;
  size_t mh_blocks_cap = 0;
  SiteRecord* d_mh_out = nullptr;
  MhScore* d_mh_out_scores = nullptr;
  size_t mh_out_cap = 0;
  // calitas_find_edit_sites: the SNVs, a count and a status byte per SNV, the workgroups' sums and their scan, the four bystander
  // counters, and the records in order
  Snv* d_ed_snvs = nullptr;
  uint32_t* d_ed_lanes = nullptr;
  uint8_t* d_ed_status = nullptr;
  size_t ed_snvs_cap = 0;
  uint32_t* d_ed_count = nullptr;
  uint64_t* d_ed_off = nullptr;
  size_t ed_blocks_cap = 0;
  unsigned long long* d_ed_by = nullptr;
  EditSite* d_ed_out = nullptr;
  size_t ed_out_cap = 0;
  // the U / u runs of the resident reference (a U is a plain base to a site and an exception base to the kernels)
  uint64_t u_serial = ~0ull;
  std::vector<Run> u_runs;
};

void sites_destroy(SitesWork* w) {
  if (!w) return;
  (void)hipFree(w->d_pat); (void)hipFree(w->d_count); (void)hipFree(w->d_off); (void)hipFree(w->d_totals); (void)hipFree(w->d_out);
  (void)hipFree(w->d_keys); (void)hipFree(w->d_key_index); (void)hipFree(w->d_key_counts);
  (void)hipFree(w->d_near_offsets); (void)hipFree(w->d_near_members);
  (void)hipFree(w->d_list_base); (void)hipFree(w->d_list_cursors); (void)hipFree(w->d_list_order); (void)hipFree(w->d_list_in); (void)hipFree(w->d_list_out);
  (void)hipFree(w->d_presence); (void)hipFree(w->d_reg_cls); (void)hipFree(w->d_reg_count); (void)hipFree(w->d_reg_off); (void)hipFree(w->d_reg_cells); (void)hipFree(w->d_reg_out); (void)hipFree(w->d_reg_out_cls);
  (void)hipFree(w->d_act_table); (void)hipFree(w->d_act_scores); (void)hipFree(w->d_act_count); (void)hipFree(w->d_act_off); (void)hipFree(w->d_act_out); (void)hipFree(w->d_act_out_scores);
  (void)hipFree(w->d_pair_lanes); (void)hipFree(w->d_pair_count); (void)hipFree(w->d_pair_off); (void)hipFree(w->d_pair_by); (void)hipFree(w->d_pair_out);
  (void)hipFree(w->d_snvs); (void)hipFree(w->d_al_lanes); (void)hipFree(w->d_al_status); (void)hipFree(w->d_al_count); (void)hipFree(w->d_al_off); (void)hipFree(w->d_al_by); (void)hipFree(w->d_al_out);
  (void)hipFree(w->d_mh_scores); (void)hipFree(w->d_mh_count); (void)hipFree(w->d_mh_off); (void)hipFree(w->d_mh_out); (void)hipFree(w->d_mh_out_scores);
  (void)hipFree(w->d_ed_snvs); (void)hipFree(w->d_ed_lanes); (void)hipFree(w->d_ed_status); (void)hipFree(w->d_ed_count); (void)hipFree(w->d_ed_off); (void)hipFree(w->d_ed_by); (void)hipFree(w->d_ed_out);
  delete w;
}

}  // namespace calitas

namespace {

struct SiteCall {
  SiteTables tab;                    // the patterns; the filter as the kernel reads it
  const calitas_site_filter_t* filter = nullptr;
  int c_first = 0, c_last = 0;       // contigs [c_first, c_last]
  bool pam5 = false;                 // the pattern has PAMs and they stand in front of the protospacer
};

// the first half of plan_sites: the pattern and the filter
int plan_site_pattern(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, SiteCall& call) {
  if (!c->has_ref) return calitas_fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  GuideHost gh;
  std::string e = make_guide_host(*pattern, gh);
  if (e.empty()) e = make_site_patterns(gh, call.tab.pat);
  call.filter = filter;
  call.pam5 = gh.pam5 && !gh.pams.empty();
  if (e.empty() && filter) e = make_site_filter(*filter, call.tab.pat.proto_len, call.tab.filter);
  if (!e.empty()) return calitas_fail(c, CALITAS_EINVAL, e);
  return CALITAS_OK;
}

// arguments every entry point shares: the pattern, the filter, the contigs, the region
int plan_sites(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index, uint64_t start, uint64_t end,
               SiteCall& call) {
  if (int rc = plan_site_pattern(c, pattern, filter, call)) return rc;
  const PackedRef& ref = c->ref;
  const int nc = (int)ref.contigs.size();
  if (chrom_index >= nc) return calitas_fail(c, CALITAS_EINVAL, "chrom_index out of range");
  call.c_first = chrom_index < 0 ? 0 : chrom_index;
  call.c_last = chrom_index < 0 ? nc - 1 : chrom_index;
  if (chrom_index >= 0) {
    const uint64_t len = ref.contigs[(size_t)chrom_index].len;
    if (start > len || end > len || (end != 0 && end < start)) return calitas_fail(c, CALITAS_EINVAL, "the region does not lie on the contig");
  } else if (end != 0 && end < start) return calitas_fail(c, CALITAS_EINVAL, "the region ends before it starts");
  for (int i = call.c_first; i <= call.c_last; i++)
    if (ref.is_absent((size_t)i) && std::min<uint64_t>(start, ref.contigs[(size_t)i].len) < region_end(ref.contigs[(size_t)i].len, end))
      return calitas_fail(c, CALITAS_EINVAL, "contig " + ref.names[(size_t)i] + " is absent from this context (calitas_set_reference with bases == NULL)");
  return CALITAS_OK;
}

bool site_less(const calitas_site_t& a, const calitas_site_t& b) {
  if (a.contig_index != b.contig_index) return a.contig_index < b.contig_index;
  if (a.protospacer_start != b.protospacer_start) return a.protospacer_start < b.protospacer_start;
  return a.strand == '+' && b.strand == '-';
}

// The sites whose footprint holds a U: the kernel sees an exception base there.  Found on the host around every U run of the region
// (with_u), together with the records the kernel has at those positions in their place (kernel_has).
void sites_with_u(calitas_ctx* c, const SiteCall& call, uint64_t start, uint64_t end, std::vector<calitas_site_t>& with_u,
                  std::vector<calitas_site_t>& kernel_has) {
  if (!c->sites) c->sites = new SitesWork();
  SitesWork* w = c->sites;
  const PackedRef& ref = c->ref;
  if (w->u_serial != c->ref_serial) {
    w->u_runs.clear();
    for (const Run& r : ref.runs) if (r.ch == 'U' || r.ch == 'u') w->u_runs.push_back(r);
    w->u_serial = c->ref_serial;
  }
  int64_t done_contig = -1, done_to = 0;            // the runs are in position order: start positions already looked at
  for (const Run& r : w->u_runs) {
    const int contig = (int)ref.tiles[r.start / ref.tile].contig;
    if (contig < call.c_first || contig > call.c_last) continue;
    const ContigInfo& ci = ref.contigs[(size_t)contig];
    const int64_t x0 = (int64_t)(r.start - ci.gbase);
    int64_t p_lo = x0 - SITE_MAX_FOOT, p_hi = x0 + (int64_t)r.len + MAX_PAM_LEN;
    if (done_contig == contig && p_lo < done_to) p_lo = done_to;
    host_sites(ref, call.tab.pat, call.filter, contig, p_lo, p_hi, (int64_t)std::min<uint64_t>(start, ci.len), (int64_t)region_end(ci.len, end), with_u,
               &kernel_has);
    done_contig = contig; done_to = std::max(p_hi, p_lo);
  }
}

// The launch of a region: the words it touches, from a workgroup boundary on (contigs start on tile boundaries, tiles are whole
// workgroups), and the arguments every kernel of sites.hip shares.
int site_launch(calitas_ctx* ctx, const SiteCall& call, int32_t chrom_index, uint64_t start, uint64_t end, SitesWork* w, SitesArgs& a) {
  const PackedRef& ref = ctx->ref;
  const ContigInfo& cf = ref.contigs[(size_t)call.c_first];
  const ContigInfo& cl = ref.contigs[(size_t)call.c_last];
  uint64_t w0 = (cf.gbase + (chrom_index < 0 ? 0 : std::min(start, cf.len))) / 32, w1 = (cl.gbase + (chrom_index < 0 ? cl.len : region_end(cl.len, end)) + 31) / 32;
  w0 -= w0 % SITES_BLOCK_WORDS;
  const uint64_t blocks64 = w1 > w0 ? (w1 - w0 + SITES_BLOCK_WORDS - 1) / SITES_BLOCK_WORDS : 0;
  if (blocks64 > 0x7FFFFFFFull) return calitas_fail(ctx, CALITAS_EINVAL, "the region is too large for one launch");
  const uint32_t n_blocks = (uint32_t)blocks64;
  // enough workgroups to fill the chip for a small region, few enough for a genome that their launch rate does not bind
  uint32_t segs_per_wg = std::min<uint32_t>(16u, std::max<uint32_t>(1u, n_blocks / 2048u));
  if (const char* e = TUNE_GET("CALITAS_SITES_SEGS")) { const int v = std::atoi(e); if (v >= 1 && v <= 16) segs_per_wg = (uint32_t)v; }
  if (!w->d_pat) HIP_TRY(ctx, hipMalloc((void**)&w->d_pat, sizeof(SiteTables)));
  a = SitesArgs{};
  a.planes = ctx->d_planes; a.mask = ctx->d_mask; a.tiles = ctx->d_tiles; a.contigs = ctx->d_contigs; a.pat = &w->d_pat->pat;
  a.n_words = ref.total_packed / 32; a.w0 = w0; a.n_segs = n_blocks; a.segs_per_wg = segs_per_wg; a.tile_words = (uint32_t)(ref.tile / 32); a.chrom_index = chrom_index;
  a.start = start; a.end = end;
  return CALITAS_OK;
}

}  // namespace

int calitas_find_sites_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index,
                                 uint64_t start, uint64_t end, calitas_site_t** sites, uint64_t* n_sites) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  SiteCall call;
  if (int rc = plan_sites(c, pattern, filter, chrom_index, start, end, call)) return rc;
  std::vector<calitas_site_t> found;
  for (int i = call.c_first; i <= call.c_last; i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    host_sites(ctx->ref, call.tab.pat, filter, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
  }
  *n_sites = found.size();
  if (!sites) return CALITAS_OK;
  *sites = (calitas_site_t*)calitas_out_alloc(std::max<size_t>(1, found.size()) * sizeof(calitas_site_t));
  if (!*sites) return calitas_fail(c, CALITAS_EINVAL, "out of memory");
  if (!found.empty()) std::memcpy(*sites, found.data(), found.size() * sizeof(calitas_site_t));
  return CALITAS_OK;
}

int calitas_find_sites_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index, uint64_t start,
                            uint64_t end, bool listing, calitas_site_t** sites, uint64_t* per_contig_strand, uint64_t* n_sites) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_sites needs a GPU (there is no CPU fallback; calitas_find_sites_host is the host twin)");
  SiteCall call;
  if (int rc = plan_sites(ctx, pattern, filter, chrom_index, start, end, call)) return rc;
  static_assert(offsetof(SiteTables, pat) == 0, "SitesArgs::pat heads the block");
  static_assert(sizeof(SiteRecord) == sizeof(calitas_site_t) && offsetof(SiteRecord, contig) == offsetof(calitas_site_t, contig_index) &&
                offsetof(SiteRecord, proto_start) == offsetof(calitas_site_t, protospacer_start) &&
                offsetof(SiteRecord, pam_start) == offsetof(calitas_site_t, pam_start) && offsetof(SiteRecord, strand) == offsetof(calitas_site_t, strand) &&
                offsetof(SiteRecord, pam_index) == offsetof(calitas_site_t, pam_index) && offsetof(SiteRecord, pam_len) == offsetof(calitas_site_t, pam_length) &&
                offsetof(SiteRecord, proto_len) == offsetof(calitas_site_t, protospacer_length), "the kernel writes calitas_site_t");
  const PackedRef& ref = ctx->ref;
  const size_t nc = ref.contigs.size();
  if (nc == 0) {                                  // nothing to scan
    if (listing && !(*sites = (calitas_site_t*)calitas_out_alloc(sizeof(calitas_site_t)))) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
    return CALITAS_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;

  SitesArgs a{};
  if (int rc = site_launch(ctx, call, chrom_index, start, end, w, a)) return rc;
  const uint32_t n_blocks = a.n_segs;

  if (w->blocks_cap < (size_t)n_blocks + 1) {
    (void)hipFree(w->d_count); (void)hipFree(w->d_off); w->d_count = nullptr; w->d_off = nullptr; w->blocks_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_count, ((size_t)n_blocks + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_off, ((size_t)n_blocks + 1) * sizeof(uint64_t)));
    w->blocks_cap = (size_t)n_blocks + 1;
  }
  if (w->totals_cap < 2 * nc) {
    (void)hipFree(w->d_totals); w->d_totals = nullptr; w->totals_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_totals, 2 * nc * sizeof(unsigned long long)));
    w->totals_cap = 2 * nc;
  }
  a.wg_count = w->d_count; a.totals = w->d_totals; a.wg_offset = w->d_off; a.out = nullptr; a.out_capacity = 0;

  std::vector<uint64_t> totals(2 * nc + 1, 0);
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.tab, filter ? sizeof(SiteTables) : sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));   // (no filter: the patterns alone, as ever)
  HIP_TRY(ctx, hipMemsetAsync(w->d_totals, 0, 2 * nc * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_sites_count(a, filter != nullptr, ctx->stream));
  if (listing) {
    HIP_TRY(ctx, launch_sites_offsets(w->d_count, w->d_off, n_blocks, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&totals[2 * nc], w->d_off + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipMemcpyAsync(totals.data(), w->d_totals, 2 * nc * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t n_dev = 0;
  for (size_t i = 0; i < 2 * nc; i++) n_dev += totals[i];
  if (listing && n_dev != totals[2 * nc]) return calitas_fail(ctx, CALITAS_EHIP, "the workgroups' counts do not add up to the contigs' (internal error)");

  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call, start, end, with_u, kernel_has);
  for (const calitas_site_t& s : with_u) totals[2 * (size_t)s.contig_index + (s.strand == '-' ? 1 : 0)]++;
  for (const calitas_site_t& s : kernel_has) totals[2 * (size_t)s.contig_index + (s.strand == '-' ? 1 : 0)]--;
  *n_sites = n_dev + with_u.size() - kernel_has.size();
  if (per_contig_strand) std::memcpy(per_contig_strand, totals.data(), 2 * nc * sizeof(uint64_t));
  if (!listing) return CALITAS_OK;

  calitas_site_t* block = (calitas_site_t*)calitas_out_alloc(std::max<uint64_t>(1, n_dev + with_u.size()) * sizeof(calitas_site_t));
  if (!block) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  if (n_dev) {
    int rc = CALITAS_OK;
    do {   // (one exit that releases the block)
      hipError_t e = hipSuccess;
      if (w->out_cap < n_dev) {
        (void)hipFree(w->d_out); w->d_out = nullptr; w->out_cap = 0;
        if ((e = hipMalloc((void**)&w->d_out, n_dev * sizeof(SiteRecord))) != hipSuccess) { (void)hipGetLastError(); rc = calitas_fail(ctx, CALITAS_ENOMEM, "the site records do not fit the device: list the region in pieces"); break; }
        w->out_cap = n_dev;
      }
      a.out = w->d_out; a.out_capacity = n_dev;
      if ((e = launch_sites_write(a, filter != nullptr, ctx->stream)) != hipSuccess ||
          (e = hipMemcpyAsync(block, w->d_out, n_dev * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
          (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
        rc = calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_sites: ") + hipGetErrorString(e));
    } while (0);
    if (rc) { calitas_free(block); return rc; }
  }
  if (!with_u.empty()) {
    // the kernel's records at those positions out (both lists are in output order), the right ones in
    calitas_site_t* end_dev = block + n_dev;
    for (const calitas_site_t& s : kernel_has) {
      calitas_site_t* at = std::lower_bound(block, end_dev, s, site_less);
      if (at == end_dev || std::memcmp(at, &s, sizeof(s)) != 0) { calitas_free(block); return calitas_fail(ctx, CALITAS_EHIP, "a record the kernel should have written beside a U is not there (internal error)"); }
      at->contig_index = -1;
    }
    end_dev = std::remove_if(block, end_dev, [](const calitas_site_t& s) { return s.contig_index < 0; });
    std::memcpy(end_dev, with_u.data(), with_u.size() * sizeof(calitas_site_t));
    std::sort(block, block + *n_sites, site_less);
  }
  *sites = block;
  return CALITAS_OK;
}

// ---- calitas_count_copies: how often a guide's protospacer, or its PAM-proximal seed, stands next to a PAM ----

namespace {

constexpr uint64_t COPIES_MAX_QUERIES = 1ull << 24;

struct CopiesCall {
  SiteCall site;
  int L = 0, K = 0;
  std::vector<uint64_t> keys;                        // the distinct query keys, in the order of their first query
  std::vector<uint32_t> of_query;                    // per query: its key's index in `keys`
  std::unordered_map<uint64_t, uint32_t> index;      // key -> index in `keys`
};

// The arguments both implementations share, checked in this order: the pattern and the region (plan_sites), key_length, the number of
// queries, their letters.
int plan_copies(calitas_ctx* c, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start, uint64_t end, const char* queries,
                uint64_t n_queries, CopiesCall& call) {
  if (int rc = plan_sites(c, pattern, nullptr, chrom_index, start, end, call.site)) return rc;
  call.L = call.site.tab.pat.proto_len;
  if (key_length < 0 || key_length > call.L)
    return calitas_fail(c, CALITAS_EINVAL, "key_length is " + std::to_string(key_length) + ": it is 1 .. the protospacer's length (" + std::to_string(call.L) + "), or 0 for that length");
  call.K = key_length == 0 ? call.L : key_length;
  if (n_queries > COPIES_MAX_QUERIES) return calitas_fail(c, CALITAS_EINVAL, "n_queries exceeds 16777216 (2^24): count the queries in pieces");
  const size_t K = (size_t)call.K;
  call.of_query.resize((size_t)n_queries);
  call.index.reserve((size_t)n_queries);
  for (uint64_t q = 0; q < n_queries; q++) {
    uint32_t lo = 0, hi = 0;
    for (size_t i = 0; i < K; i++) {
      const unsigned char ch = (unsigned char)queries[q * K + i];
      const int set = iupac_mask(ch);
      if (set != 1 && set != 2 && set != 4 && set != 8)
        return calitas_fail(c, CALITAS_EINVAL, "queries[" + std::to_string(q) + "] holds a letter outside ACGTUacgtu at position " + std::to_string(i));
      const uint32_t code = set == 1 ? 0u : set == 2 ? 1u : set == 4 ? 2u : 3u;
      lo |= (code & 1u) << i; hi |= (code >> 1) << i;
    }
    const uint64_t key = copies_key(lo, hi, call.K, call.K, false, false);     // a guide of K bases on '+', all of it
    const auto at = call.index.emplace(key, (uint32_t)call.keys.size());
    if (at.second) call.keys.push_back(key);
    call.of_query[(size_t)q] = at.first->second;
  }
  return CALITAS_OK;
}

// the key of the site whose protospacer starts at p of the contig at gbase, base by base (a U is a T)
uint64_t key_at(const PackedRef& ref, uint64_t gbase, int64_t p, const CopiesCall& call, bool minus) {
  uint32_t lo = 0, hi = 0;
  for (int i = 0; i < call.L; i++) {
    bool u = false;
    const uint32_t code = (uint32_t)plain_code(ref, gbase + (uint64_t)(p + i), &u);
    lo |= (code & 1u) << i; hi |= (code >> 1) << i;
  }
  return copies_key(lo, hi, call.L, call.K, minus, call.site.pam5);
}

// counts[key's index] += by for every record whose key is a query's
void add_sites(const PackedRef& ref, const CopiesCall& call, const std::vector<calitas_site_t>& sites, uint64_t by, std::vector<uint64_t>& counts) {
  for (const calitas_site_t& s : sites) {
    const auto at = call.index.find(key_at(ref, ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, call, s.strand == '-'));
    if (at != call.index.end()) counts[at->second] += by;
  }
}

}  // namespace

int calitas_count_copies_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start,
                                   uint64_t end, const char* queries, uint64_t n_queries, uint64_t* copies) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  CopiesCall call;
  if (int rc = plan_copies(c, pattern, key_length, chrom_index, start, end, queries, n_queries, call)) return rc;
  std::vector<uint64_t> counts(call.keys.size(), 0);
  std::vector<calitas_site_t> found;
  for (int i = call.site.c_first; i <= call.site.c_last && !call.keys.empty(); i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, call.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    add_sites(ctx->ref, call, found, 1, counts);
  }
  for (uint64_t q = 0; q < n_queries; q++) copies[q] = counts[call.of_query[(size_t)q]];
  return CALITAS_OK;
}

int calitas_count_copies_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start, uint64_t end,
                              const char* queries, uint64_t n_queries, uint64_t* copies) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_count_copies needs a GPU (there is no CPU fallback; calitas_count_copies_host is the host twin)");
  CopiesCall call;
  if (int rc = plan_copies(ctx, pattern, key_length, chrom_index, start, end, queries, n_queries, call)) return rc;
  const PackedRef& ref = ctx->ref;
  const size_t n_keys = call.keys.size();
  if (n_keys == 0 || ref.contigs.empty()) {         // nothing to look up, or nothing to scan
    for (uint64_t q = 0; q < n_queries; q++) copies[q] = 0;
    return CALITAS_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.site, chrom_index, start, end, w, a)) return rc;

  // the table: a power of two of slots, at most half of them taken; linear probing from the multiplicative hash's slot.  The key that
  // looks like a free slot (COPIES_EMPTY: T x 32, possible at K = 32 only) stays outside, the kernel knows its index.
  uint32_t log2_slots = 4;
  static_assert(COPIES_MIN_SLOTS == 16, "log2_slots starts at the minimum");
  while (((size_t)1 << log2_slots) < 2 * n_keys) log2_slots++;
  const size_t slots = (size_t)1 << log2_slots;
  std::vector<uint64_t> table(slots, COPIES_EMPTY);
  std::vector<uint32_t> table_index(slots, COPIES_NONE);
  a.ones_index = COPIES_NONE;
  for (size_t k = 0; k < n_keys; k++) {
    const uint64_t key = call.keys[k];
    if (key == COPIES_EMPTY) { a.ones_index = (uint32_t)k; continue; }
    size_t slot = (size_t)((key * COPIES_HASH) >> (64 - log2_slots));
    while (table[slot] != COPIES_EMPTY) slot = (slot + 1) & (slots - 1);
    table[slot] = key; table_index[slot] = (uint32_t)k;
  }
  if (w->slots_cap < slots) {
    (void)hipFree(w->d_keys); (void)hipFree(w->d_key_index); w->d_keys = nullptr; w->d_key_index = nullptr; w->slots_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_keys, slots * sizeof(uint64_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_key_index, slots * sizeof(uint32_t)));
    w->slots_cap = slots;
  }
  if (w->key_counts_cap < n_keys + 1) {
    (void)hipFree(w->d_key_counts); w->d_key_counts = nullptr; w->key_counts_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_key_counts, (n_keys + 1) * sizeof(unsigned long long)));
    w->key_counts_cap = n_keys + 1;
  }
  a.keys = w->d_keys; a.key_index = w->d_key_index; a.key_counts = w->d_key_counts;
  a.table_mask = (uint32_t)(slots - 1); a.table_shift = 64 - log2_slots; a.n_keys = (uint32_t)n_keys;
  a.key_len = call.K; a.key_first = call.site.pam5 ? 1 : 0;

  std::vector<uint64_t> counts(n_keys + 1, 0);
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.site.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_keys, table.data(), slots * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_key_index, table_index.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_key_counts, 0, (n_keys + 1) * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_sites_copies(a, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts.data(), w->d_key_counts, (n_keys + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (counts[n_keys] != 0) return calitas_fail(ctx, CALITAS_EHIP, "calitas_count_copies: a probe of the key table found neither its key nor a free slot (internal error)");

  // a U is a T to a site and an exception base to the kernel: the sites it did not see in, the records it saw in their place out
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.site, start, end, with_u, kernel_has);
  add_sites(ref, call, with_u, 1, counts);
  add_sites(ref, call, kernel_has, ~0ull, counts);          // (- 1)
  for (uint64_t q = 0; q < n_queries; q++) copies[q] = counts[call.of_query[(size_t)q]];
  return CALITAS_OK;
}

// ---- calitas_count_near: how often a guide's protospacer, or its seed, stands next to a PAM with up to M substitutions ----

namespace {

struct NearCall {
  CopiesCall copies;                                 // the pattern, the region, K and the distinct query keys (plan_copies)
  int M = 0;
};

// checked in this order: max_mismatches, what calitas_count_copies checks, K >= M + 1
int plan_near(calitas_ctx* c, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index, uint64_t start, uint64_t end,
              const char* queries, uint64_t n_queries, NearCall& call) {
  static_assert(NEAR_MAX_M == CALITAS_NEAR_MAX_MISMATCHES, "the kernel unrolls what the contract allows");
  if (max_mismatches < 0 || max_mismatches > NEAR_MAX_M)
    return calitas_fail(c, CALITAS_EINVAL, "max_mismatches is " + std::to_string(max_mismatches) + ": it is 0 .. " + std::to_string(NEAR_MAX_M));
  call.M = max_mismatches;
  if (int rc = plan_copies(c, pattern, key_length, chrom_index, start, end, queries, n_queries, call.copies)) return rc;
  if (call.copies.K < call.M + 1)
    return calitas_fail(c, CALITAS_EINVAL, "key_length: a key of " + std::to_string(call.copies.K) + " bases is shorter than max_mismatches + 1 (" + std::to_string(call.M + 1) + ")");
  return CALITAS_OK;
}

// the number of positions at which two keys differ: a position differs where either plane does
inline int key_distance(uint64_t a, uint64_t b) {
  const uint64_t x = a ^ b;
  return __builtin_popcount((uint32_t)x | (uint32_t)(x >> 32));
}

// counts[index (M + 1) + d] += by for every record and every distinct query at distance d <= M of the record's key, query by query
void add_near_sites(const PackedRef& ref, const NearCall& call, const std::vector<calitas_site_t>& sites, uint64_t by, std::vector<uint64_t>& counts) {
  const size_t row = (size_t)call.M + 1;
  for (const calitas_site_t& s : sites) {
    const uint64_t key = key_at(ref, ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, call.copies, s.strand == '-');
    for (size_t k = 0; k < call.copies.keys.size(); k++) {
      const int d = key_distance(key, call.copies.keys[k]);
      if (d <= call.M) counts[k * row + (size_t)d] += by;
    }
  }
}

void near_rows(const NearCall& call, const std::vector<uint64_t>& counts, uint64_t n_queries, uint64_t* near) {
  const size_t row = (size_t)call.M + 1;
  for (uint64_t q = 0; q < n_queries; q++)
    for (size_t d = 0; d < row; d++) near[q * row + d] = counts[(size_t)call.copies.of_query[(size_t)q] * row + d];
}

}  // namespace

int calitas_count_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index,
                                 uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  NearCall call;
  if (int rc = plan_near(c, pattern, key_length, max_mismatches, chrom_index, start, end, queries, n_queries, call)) return rc;
  std::vector<uint64_t> counts(call.copies.keys.size() * ((size_t)call.M + 1), 0);
  std::vector<calitas_site_t> found;
  for (int i = call.copies.site.c_first; i <= call.copies.site.c_last && !call.copies.keys.empty(); i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, call.copies.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    add_near_sites(ctx->ref, call, found, 1, counts);
  }
  near_rows(call, counts, n_queries, near);
  return CALITAS_OK;
}

namespace {

// The near kernel's launch for a planned call: the pieces' bucket tables, the members, the counters zeroed, one pass, one copy-back.
// model == nullptr: calitas_count_near, counts of n_keys rows of M + 1 words.  Otherwise NEAR_MODEL_WORDS words, the packed table of
// calitas_score_near: it rides behind the offsets, and the rows have M + 3 words (the counts, the sum, the maximum).
// again != nullptr (calitas_list_near, with a model): the table rides along, the counts alone are taken (rows of M + 1 words), and
// *again receives the launch's arguments -- tables, members and patterns stay on the device for the pass's second run.
int run_near(calitas_ctx* ctx, const NearCall& call, int32_t chrom_index, uint64_t start, uint64_t end, const uint32_t* model, std::vector<uint64_t>& counts,
             SitesArgs* again = nullptr) {
  const std::vector<uint64_t>& keys = call.copies.keys;
  const size_t n_keys = keys.size(), row = (size_t)call.M + 1, n_counters = n_keys * (row + (model && !again ? 2 : 0));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.copies.site, chrom_index, start, end, w, a)) return rc;

  // per piece a bucket table in CSR form -- the offsets of piece p count from p n_keys on, so they address the one member array --
  // and every key as a member of its bucket: a counting sort by bucket
  const int pw = near_piece_width(call.copies.K, call.M);
  const size_t per_table = ((size_t)1 << (2 * pw)) + 1, n_offsets = row * per_table, n_members = row * n_keys;
  std::vector<uint32_t> offsets(n_offsets + (model ? NEAR_MODEL_WORDS : 0), 0);
  std::vector<uint4> members(n_members);
  for (size_t p = 0; p < row; p++) {
    uint32_t* o = offsets.data() + p * per_table;
    for (size_t k = 0; k < n_keys; k++) o[near_bucket((uint32_t)keys[k], (uint32_t)(keys[k] >> 32), (int)p, pw) + 1]++;
    o[0] = (uint32_t)(p * n_keys);
    for (size_t b = 1; b < per_table; b++) o[b] += o[b - 1];
    std::vector<uint32_t> at(o, o + per_table - 1);
    for (size_t k = 0; k < n_keys; k++)
      members[at[near_bucket((uint32_t)keys[k], (uint32_t)(keys[k] >> 32), (int)p, pw)]++] = make_uint4((uint32_t)keys[k], (uint32_t)(keys[k] >> 32), (uint32_t)k, 0u);
  }
  if (model) {
    if (near_model_offset(call.M, pw) != n_offsets) return calitas_fail(ctx, CALITAS_EHIP, "the score table does not stand where the kernel reads it (internal error)");
    std::memcpy(offsets.data() + n_offsets, model, NEAR_MODEL_WORDS * sizeof(uint32_t));
  }
  if (w->near_offsets_cap < offsets.size()) {
    (void)hipFree(w->d_near_offsets); w->d_near_offsets = nullptr; w->near_offsets_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_near_offsets, offsets.size() * sizeof(uint32_t)));
    w->near_offsets_cap = offsets.size();
  }
  if (w->near_members_cap < n_members) {
    (void)hipFree(w->d_near_members); w->d_near_members = nullptr; w->near_members_cap = 0;
    if (hipMalloc((void**)&w->d_near_members, n_members * sizeof(uint4)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, "the query keys do not fit the device: count the queries in pieces"); }
    w->near_members_cap = n_members;
  }
  if (w->key_counts_cap < n_counters) {
    (void)hipFree(w->d_key_counts); w->d_key_counts = nullptr; w->key_counts_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_key_counts, n_counters * sizeof(unsigned long long)));
    w->key_counts_cap = n_counters;
  }
  a.near_offsets = w->d_near_offsets; a.near_members = w->d_near_members; a.key_counts = w->d_key_counts;
  a.near_m = call.M; a.near_w = pw; a.n_keys = (uint32_t)n_keys;
  a.key_len = call.copies.K; a.key_first = call.copies.site.pam5 ? 1 : 0;

  counts.assign(n_counters, 0);
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.copies.site.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_near_offsets, offsets.data(), offsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_near_members, members.data(), n_members * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_key_counts, 0, n_counters * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, model && !again ? launch_sites_near_score(a, ctx->stream) : launch_sites_near(a, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts.data(), w->d_key_counts, n_counters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (again) *again = a;
  return CALITAS_OK;
}

}  // namespace

int calitas_count_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index, uint64_t start,
                            uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_count_near needs a GPU (there is no CPU fallback; calitas_count_near_host is the host twin)");
  NearCall call;
  if (int rc = plan_near(ctx, pattern, key_length, max_mismatches, chrom_index, start, end, queries, n_queries, call)) return rc;
  const PackedRef& ref = ctx->ref;
  const size_t row = (size_t)call.M + 1;
  if (call.copies.keys.empty() || ref.contigs.empty()) {         // nothing to look up, or nothing to scan
    for (uint64_t i = 0; i < n_queries * row; i++) near[i] = 0;
    return CALITAS_OK;
  }
  std::vector<uint64_t> counts;
  if (int rc = run_near(ctx, call, chrom_index, start, end, nullptr, counts)) return rc;

  // a U is a T to a site and an exception base to the kernel: the sites it did not see in, the records it saw in their place out
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.copies.site, start, end, with_u, kernel_has);
  add_near_sites(ref, call, with_u, 1, counts);
  add_near_sites(ref, call, kernel_has, ~0ull, counts);     // (- 1)
  near_rows(call, counts, n_queries, near);
  return CALITAS_OK;
}

// ---- calitas_score_near: the near copies of the whole protospacer, and what they add up to under a score model ----

namespace {

struct NearScoreCall {
  NearCall near;                                     // K = L
  const uint32_t* mismatch = nullptr;                // the caller's [L][5][5]
};

// the model as calitas_search_scores checks it -- of which the near calls read the mismatch table alone
int check_near_model(calitas_ctx* c, const calitas_score_model_t* model, NearScoreCall& call) {
  const int L = call.near.copies.L;
  if (!model || !model->mismatch) return calitas_fail(c, CALITAS_EINVAL, "the score model has no mismatch table");
  if (model->protospacer_length != L)
    return calitas_fail(c, CALITAS_EINVAL, "the score model is for protospacers of " + std::to_string(model->protospacer_length) + " bases, the guide has " + std::to_string(L));
  for (int i = 0; i < L * 25; i++)
    if (model->mismatch[i] > 65536u) return calitas_fail(c, CALITAS_EINVAL, "a factor of the score model is above 65536 (1.0)");
  call.mismatch = model->mismatch;
  return CALITAS_OK;
}

// checked in this order: what calitas_count_near checks (the key is the whole protospacer), then the model
int plan_near_score(calitas_ctx* c, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                    uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, NearScoreCall& call) {
  if (int rc = plan_near(c, pattern, 0, max_mismatches, chrom_index, start, end, queries, n_queries, call.near)) return rc;
  return check_near_model(c, model, call);
}

// The contract's loop on two keys of L positions, letter by letter from the planes: the factors of the differing positions in
// ascending order, each read from the caller's table as it stands (never from the kernel's packed one).
uint64_t near_pair_score(const uint32_t* mismatch, int L, uint64_t query, uint64_t site) {
  uint64_t s = 1ull << 32;
  for (int i = 0; i < L; i++) {
    const uint32_t g = (uint32_t)((query >> i) & 1u) | ((uint32_t)((query >> (32 + i)) & 1u) << 1);
    const uint32_t t = (uint32_t)((site >> i) & 1u) | ((uint32_t)((site >> (32 + i)) & 1u) << 1);
    if (g != t) s = (s * mismatch[(size_t)i * 25 + g * 5 + t]) >> 16;
  }
  return s;
}

// rows[k]: M + 1 counts, the sum, the maximum.  Every record against every distinct query: the count by `by` (1 or - 1), and at
// d >= 1 the pair's score into the sum by the same sign; into the maximum only when the record comes in.
void add_near_scores(const PackedRef& ref, const NearScoreCall& call, const std::vector<calitas_site_t>& sites, bool in, std::vector<uint64_t>& rows) {
  const NearCall& nc = call.near;
  const size_t M = (size_t)nc.M, row = M + 3;
  for (const calitas_site_t& s : sites) {
    const uint64_t key = key_at(ref, ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, nc.copies, s.strand == '-');
    for (size_t k = 0; k < nc.copies.keys.size(); k++) {
      const int d = key_distance(key, nc.copies.keys[k]);
      if (d > nc.M) continue;
      uint64_t* r = &rows[k * row];
      r[d] += in ? 1 : ~0ull;
      if (d == 0) continue;
      const uint64_t sc = near_pair_score(call.mismatch, nc.copies.L, nc.copies.keys[k], key);
      if (in) { r[M + 1] += sc; r[M + 2] = std::max(r[M + 2], sc); }
      else r[M + 1] -= sc;
    }
  }
}

void near_score_rows(const NearScoreCall& call, const std::vector<uint64_t>& rows, uint64_t n_queries, uint64_t* near, calitas_near_score_t* scores) {
  const size_t M = (size_t)call.near.M, row = M + 3;
  for (uint64_t q = 0; q < n_queries; q++) {
    const uint64_t* r = rows.empty() ? nullptr : &rows[(size_t)call.near.copies.of_query[(size_t)q] * row];
    for (size_t d = 0; d <= M; d++) near[q * (M + 1) + d] = r ? r[d] : 0;
    scores[q].sum_q32 = r ? r[M + 1] : 0;
    scores[q].max_q32 = r ? r[M + 2] : 0;
  }
}

}  // namespace

int calitas_score_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                                 int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near,
                                 calitas_near_score_t* scores) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  NearScoreCall call;
  if (int rc = plan_near_score(c, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, call)) return rc;
  const CopiesCall& cc = call.near.copies;
  std::vector<uint64_t> rows(cc.keys.size() * ((size_t)call.near.M + 3), 0);
  std::vector<calitas_site_t> found;
  for (int i = cc.site.c_first; i <= cc.site.c_last && !cc.keys.empty(); i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, cc.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    add_near_scores(ctx->ref, call, found, true, rows);
  }
  near_score_rows(call, rows, n_queries, near, scores);
  return CALITAS_OK;
}

int calitas_score_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                            uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near, calitas_near_score_t* scores) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_score_near needs a GPU (there is no CPU fallback; calitas_score_near_host is the host twin)");
  NearScoreCall call;
  if (int rc = plan_near_score(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, call)) return rc;
  const PackedRef& ref = ctx->ref;
  std::vector<uint64_t> rows;
  if (call.near.copies.keys.empty() || ref.contigs.empty()) {    // nothing to look up, or nothing to scan
    near_score_rows(call, rows, n_queries, near, scores);
    return CALITAS_OK;
  }
  // the 4 x 4 block of plain bases of every position, as the kernel indexes it
  std::vector<uint32_t> packed(NEAR_MODEL_WORDS, 0u);
  for (uint32_t i = 0; i < (uint32_t)call.near.copies.L; i++)
    for (uint32_t g = 0; g < 4; g++)
      for (uint32_t t = 0; t < 4; t++) packed[near_model_index(i, g, t)] = call.mismatch[(size_t)i * 25 + g * 5 + t];
  if (int rc = run_near(ctx, call.near, chrom_index, start, end, packed.data(), rows)) return rc;

  // a U is a T to a site and an exception base to the kernel: the sites it did not see in, the records it saw in their place out.
  // Counts and sums are corrected both ways.  A maximum cannot be taken back, and need not be: host_sites pushes a kernel_has record
  // only at the (contig, strand, protospacer start) of the with_u record it has just pushed, so the two have one key and the same
  // scores -- what the kernel's record put into a maximum, the true site puts there as well.  That pairing is checked here.
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.near.copies.site, start, end, with_u, kernel_has);
  size_t at = 0;
  for (const calitas_site_t& s : kernel_has) {                   // (both lists are in output order)
    while (at < with_u.size() && site_less(with_u[at], s)) at++;
    if (at == with_u.size() || site_less(s, with_u[at]))
      return calitas_fail(ctx, CALITAS_EHIP, "calitas_score_near: a record the kernel has beside a U stands where no site with a U does (internal error)");
  }
  add_near_scores(ref, call, with_u, true, rows);
  add_near_scores(ref, call, kernel_has, false, rows);
  near_score_rows(call, rows, n_queries, near, scores);
  return CALITAS_OK;
}

// ---- calitas_list_near: where every query's copies within M substitutions stand ----

namespace {

struct NearListCall {
  NearScoreCall score;                               // K = L; mismatch == nullptr: no weights, every score is 2^32
  uint32_t limit = 0;
};

// checked in this order: what calitas_score_near checks, a NULL model being legal; then the limit
int plan_near_list(calitas_ctx* c, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                   uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, NearListCall& call) {
  if (int rc = plan_near(c, pattern, 0, max_mismatches, chrom_index, start, end, queries, n_queries, call.score.near)) return rc;
  if (model)
    if (int rc = check_near_model(c, model, call.score)) return rc;
  if (limit < 1 || limit > CALITAS_NEAR_LIST_MAX)
    return calitas_fail(c, CALITAS_EINVAL, "limit is " + std::to_string(limit) + ": it is 1 .. " + std::to_string(CALITAS_NEAR_LIST_MAX));
  call.limit = limit;
  return CALITAS_OK;
}

bool hit_less(const calitas_near_hit_t& a, const calitas_near_hit_t& b) {
  if (a.contig_index != b.contig_index) return a.contig_index < b.contig_index;
  if (a.protospacer_start != b.protospacer_start) return a.protospacer_start < b.protospacer_start;
  return a.strand == '+' && b.strand == '-';
}

// the record of a site whose key is within M of a query's, from the host's side: the twin's, and the ones a U keeps from the kernel
calitas_near_hit_t near_hit(const NearListCall& call, const calitas_site_t& s, uint64_t site_key, uint64_t query_key) {
  const uint64_t x = site_key ^ query_key;
  calitas_near_hit_t h;
  std::memset(&h, 0, sizeof(h));
  h.score_q32 = call.score.mismatch ? near_pair_score(call.score.mismatch, call.score.near.copies.L, query_key, site_key) : 1ull << 32;
  h.contig_index = s.contig_index; h.protospacer_start = s.protospacer_start;
  h.target_lo = (uint32_t)site_key; h.target_hi = (uint32_t)(site_key >> 32);
  h.diff_mask = (uint32_t)x | (uint32_t)(x >> 32);
  h.strand = s.strand; h.pam_index = s.pam_index; h.mismatches = (uint8_t)__builtin_popcount(h.diff_mask);
  return h;
}

typedef std::pair<const calitas_near_hit_t*, size_t> HitSpan;

// What the call hands over, from the distinct keys' counts and ordered stretches: near, the stretches laid out in query order -- a
// key over the limit lists nothing, a duplicate gets its key's stretch again -- and the one block of records.
int near_list_block(calitas_ctx* c, const NearListCall& call, const std::vector<uint64_t>& counts, const std::vector<HitSpan>& spans, uint64_t n_queries,
                    uint64_t* near, uint64_t* offsets, calitas_near_hit_t** hits, uint64_t* n_hits) {
  const NearCall& nc = call.score.near;
  const size_t row = (size_t)nc.M + 1;
  if (n_queries) near_rows(nc, counts, n_queries, near);
  uint64_t run = 0;
  for (uint64_t q = 0; q < n_queries; q++) {
    const size_t k = nc.copies.of_query[(size_t)q];
    uint64_t sum = 0;
    for (size_t d = 0; d < row; d++) sum += counts[k * row + d];
    offsets[q] = run;
    if (sum > call.limit) continue;
    if (spans[k].second != sum) return calitas_fail(c, CALITAS_EHIP, "calitas_list_near: a query's records are not as many as its counts (internal error)");
    run += sum;
  }
  offsets[n_queries] = run;
  calitas_near_hit_t* block = (calitas_near_hit_t*)calitas_out_alloc(std::max<uint64_t>(1, run) * sizeof(calitas_near_hit_t));
  if (!block) return calitas_fail(c, CALITAS_ENOMEM, "the records do not fit the host's memory: list the queries in pieces");
  for (uint64_t q = 0; q < n_queries; q++) {
    const uint64_t n = offsets[q + 1] - offsets[q];
    if (n) std::memcpy(block + offsets[q], spans[nc.copies.of_query[(size_t)q]].first, n * sizeof(calitas_near_hit_t));
  }
  *hits = block; *n_hits = run;
  return CALITAS_OK;
}

}  // namespace

int calitas_list_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                                int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near,
                                uint64_t* offsets, calitas_near_hit_t** hits, uint64_t* n_hits) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  NearListCall call;
  if (int rc = plan_near_list(c, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, limit, call)) return rc;
  const NearCall& nc = call.score.near;
  const CopiesCall& cc = nc.copies;
  const size_t n_keys = cc.keys.size(), row = (size_t)nc.M + 1;
  std::vector<uint64_t> counts(n_keys * row, 0);
  std::vector<std::vector<calitas_near_hit_t>> lists(n_keys);
  std::vector<calitas_site_t> found;
  for (int i = cc.site.c_first; i <= cc.site.c_last && n_keys; i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, cc.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    for (const calitas_site_t& s : found) {
      const uint64_t key = key_at(ctx->ref, ctx->ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, cc, s.strand == '-');
      for (size_t k = 0; k < n_keys; k++) {
        const int d = key_distance(key, cc.keys[k]);
        if (d > nc.M) continue;
        counts[k * row + (size_t)d]++;
        if (lists[k].size() <= call.limit) lists[k].push_back(near_hit(call, s, key, cc.keys[k]));   // (one beyond the limit: such a key lists nothing)
      }
    }
  }
  std::vector<HitSpan> spans(n_keys);
  for (size_t k = 0; k < n_keys; k++) {
    std::sort(lists[k].begin(), lists[k].end(), hit_less);
    spans[k] = HitSpan(lists[k].data(), lists[k].size());
  }
  return near_list_block(c, call, counts, spans, n_queries, near, offsets, hits, n_hits);
}

int calitas_list_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                           uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near, uint64_t* offsets,
                           calitas_near_hit_t** hits, uint64_t* n_hits) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_list_near needs a GPU (there is no CPU fallback; calitas_list_near_host is the host twin)");
  static_assert(sizeof(NearHit) == sizeof(calitas_near_hit_t) && offsetof(NearHit, score_q32) == offsetof(calitas_near_hit_t, score_q32) &&
                offsetof(NearHit, contig) == offsetof(calitas_near_hit_t, contig_index) && offsetof(NearHit, proto_start) == offsetof(calitas_near_hit_t, protospacer_start) &&
                offsetof(NearHit, target_lo) == offsetof(calitas_near_hit_t, target_lo) && offsetof(NearHit, target_hi) == offsetof(calitas_near_hit_t, target_hi) &&
                offsetof(NearHit, diff_mask) == offsetof(calitas_near_hit_t, diff_mask) && offsetof(NearHit, strand) == offsetof(calitas_near_hit_t, strand) &&
                offsetof(NearHit, pam_index) == offsetof(calitas_near_hit_t, pam_index) && offsetof(NearHit, mismatches) == offsetof(calitas_near_hit_t, mismatches),
                "the kernel writes calitas_near_hit_t");
  NearListCall call;
  if (int rc = plan_near_list(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, limit, call)) return rc;
  const NearCall& nc = call.score.near;
  const std::vector<uint64_t>& keys = nc.copies.keys;
  const PackedRef& ref = ctx->ref;
  const size_t n_keys = keys.size(), row = (size_t)nc.M + 1;
  std::vector<uint64_t> counts(n_keys * row, 0);
  std::vector<HitSpan> spans(n_keys, HitSpan(nullptr, 0));
  if (n_keys == 0 || ref.contigs.empty())            // nothing to look up, or nothing to scan
    return near_list_block(ctx, call, counts, spans, n_queries, near, offsets, hits, n_hits);

  // pass 1: the counts.  The model's 4 x 4 blocks as the kernel indexes them ride along for pass 2; without a model every factor is 1.0
  std::vector<uint32_t> packed(NEAR_MODEL_WORDS, call.score.mismatch ? 0u : 65536u);
  for (uint32_t i = 0; call.score.mismatch && i < (uint32_t)nc.copies.L; i++)
    for (uint32_t g = 0; g < 4; g++)
      for (uint32_t t = 0; t < 4; t++) packed[near_model_index(i, g, t)] = call.score.mismatch[(size_t)i * 25 + g * 5 + t];
  SitesArgs a{};
  if (int rc = run_near(ctx, nc, chrom_index, start, end, packed.data(), counts, &a)) return rc;

  // The layout.  A U is a T to a site and an exception base to the kernel, so the counts are corrected as calitas_count_near's are,
  // and the corrected counts decide whether a key lists.  A key that does gets room for what the KERNEL will store, its own count;
  // where the two differ the host patches the stretch below.
  std::vector<uint64_t> kernel_sum(n_keys, 0);
  for (size_t k = 0; k < n_keys; k++)
    for (size_t d = 0; d < row; d++) kernel_sum[k] += counts[k * row + d];
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, nc.copies.site, start, end, with_u, kernel_has);
  add_near_sites(ref, nc, with_u, 1, counts);
  add_near_sites(ref, nc, kernel_has, ~0ull, counts);       // (- 1)
  std::vector<uint64_t> base(n_keys, 0);
  std::vector<uint32_t> cursors(2 * n_keys + 1, 0), order, longer;
  uint64_t total = 0;
  for (size_t k = 0; k < n_keys; k++) {
    uint64_t sum = 0;
    for (size_t d = 0; d < row; d++) sum += counts[k * row + d];
    base[k] = total;
    cursors[2 * k + 1] = NEAR_LIST_SKIP;
    if (sum > call.limit) continue;
    if (kernel_sum[k] >= NEAR_LIST_SKIP) return calitas_fail(ctx, CALITAS_ENOMEM, "the records do not fit the device: list the queries in pieces");
    cursors[2 * k + 1] = (uint32_t)kernel_sum[k];
    total += kernel_sum[k];
    if (kernel_sum[k] > NEAR_ORDER_SHORT) longer.push_back((uint32_t)k);
    else if (kernel_sum[k]) order.push_back((uint32_t)k);
  }
  const uint32_t n_short = (uint32_t)order.size(), n_long = (uint32_t)longer.size();
  order.insert(order.end(), longer.begin(), longer.end());

  // pass 2, the order, one copy-back
  std::vector<calitas_near_hit_t> dev;
  if (total) {
    SitesWork* w = ctx->sites;
    try { dev.resize((size_t)total); } catch (const std::bad_alloc&) { return calitas_fail(ctx, CALITAS_ENOMEM, "the records do not fit the host's memory: list the queries in pieces"); }
    if (w->list_keys_cap < n_keys) {
      (void)hipFree(w->d_list_base); (void)hipFree(w->d_list_cursors); (void)hipFree(w->d_list_order);
      w->d_list_base = nullptr; w->d_list_cursors = nullptr; w->d_list_order = nullptr; w->list_keys_cap = 0;
      HIP_TRY(ctx, hipMalloc((void**)&w->d_list_base, n_keys * sizeof(uint64_t)));
      HIP_TRY(ctx, hipMalloc((void**)&w->d_list_cursors, (2 * n_keys + 1) * sizeof(uint32_t)));
      HIP_TRY(ctx, hipMalloc((void**)&w->d_list_order, n_keys * sizeof(uint32_t)));
      w->list_keys_cap = n_keys;
    }
    if (w->list_cap < total) {
      (void)hipFree(w->d_list_in); (void)hipFree(w->d_list_out); w->d_list_in = nullptr; w->d_list_out = nullptr; w->list_cap = 0;
      if (hipMalloc((void**)&w->d_list_in, total * sizeof(NearHit)) != hipSuccess || hipMalloc((void**)&w->d_list_out, total * sizeof(NearHit)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(w->d_list_in); w->d_list_in = nullptr;
        return calitas_fail(ctx, CALITAS_ENOMEM, "the records do not fit the device: list the queries in pieces");
      }
      w->list_cap = total;
    }
    a.wg_offset = w->d_list_base; a.wg_count = w->d_list_cursors; a.out = reinterpret_cast<SiteRecord*>(w->d_list_in); a.out_capacity = total;
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(w->d_list_base, base.data(), n_keys * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w->d_list_cursors, cursors.data(), (2 * n_keys + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w->d_list_order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_sites_near_list(a, ctx->stream));
    HIP_TRY(ctx, launch_near_order(w->d_list_in, w->d_list_out, w->d_list_base, w->d_list_cursors, w->d_list_order, n_short, n_long, (uint32_t)(2 * n_keys), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&flag, w->d_list_cursors + 2 * n_keys, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dev.data(), w->d_list_out, total * sizeof(NearHit), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag != 0) return calitas_fail(ctx, CALITAS_EHIP, "calitas_list_near: the second pass found other pairs than the first counted (internal error)");
  }
  for (size_t k = 0; k < n_keys; k++)
    if (cursors[2 * k + 1] != NEAR_LIST_SKIP) spans[k] = HitSpan(dev.data() + base[k], cursors[2 * k + 1]);

  // Beside a U: the stretches of the keys within M of such a site lose the records the kernel has in its place, gain the site's own
  // and are put in order again -- also the few a U made longer than the order kernel takes.
  std::vector<std::vector<calitas_near_hit_t>> fixed;
  if (!with_u.empty() || !kernel_has.empty()) {
    std::vector<uint64_t> key_in(with_u.size()), key_out(kernel_has.size());
    for (size_t i = 0; i < with_u.size(); i++) key_in[i] = key_at(ref, ref.contigs[(size_t)with_u[i].contig_index].gbase, with_u[i].protospacer_start, nc.copies, with_u[i].strand == '-');
    for (size_t i = 0; i < kernel_has.size(); i++) key_out[i] = key_at(ref, ref.contigs[(size_t)kernel_has[i].contig_index].gbase, kernel_has[i].protospacer_start, nc.copies, kernel_has[i].strand == '-');
    fixed.reserve(n_keys);                                  // (the spans point into its elements)
    for (size_t k = 0; k < n_keys; k++) {
      if (cursors[2 * k + 1] == NEAR_LIST_SKIP) continue;
      bool touched = false;
      for (size_t i = 0; i < key_in.size() && !touched; i++) touched = key_distance(key_in[i], keys[k]) <= nc.M;
      for (size_t i = 0; i < key_out.size() && !touched; i++) touched = key_distance(key_out[i], keys[k]) <= nc.M;
      if (!touched) continue;
      fixed.emplace_back(spans[k].first, spans[k].first + spans[k].second);
      std::vector<calitas_near_hit_t>& v = fixed.back();
      for (size_t i = 0; i < key_out.size(); i++) {
        if (key_distance(key_out[i], keys[k]) > nc.M) continue;
        const calitas_site_t& s = kernel_has[i];
        const auto at = std::find_if(v.begin(), v.end(), [&](const calitas_near_hit_t& h) {
          return h.contig_index == s.contig_index && h.protospacer_start == s.protospacer_start && h.strand == s.strand; });
        if (at == v.end()) return calitas_fail(ctx, CALITAS_EHIP, "calitas_list_near: a record the kernel should have written beside a U is not there (internal error)");
        v.erase(at);
      }
      for (size_t i = 0; i < key_in.size(); i++)
        if (key_distance(key_in[i], keys[k]) <= nc.M) v.push_back(near_hit(call, with_u[i], key_in[i], keys[k]));
      std::sort(v.begin(), v.end(), hit_less);
      spans[k] = HitSpan(v.data(), v.size());
    }
  }
  return near_list_block(ctx, call, counts, spans, n_queries, near, offsets, hits, n_hits);
}

// ---- calitas_find_sites_scored: every site's on-target activity under a linear model of its sequence context ----

namespace {

struct ActivityCall {
  SiteCall site;
  const calitas_activity_model_t* model = nullptr;
  int L = 0, W = 0;
  int32_t min_score = CALITAS_ACTIVITY_NONE;
  bool threshold = false;            // min_score != CALITAS_ACTIVITY_NONE: sites below it, the unscored ones among them, are dropped
};

// checked in this order: what calitas_find_sites_filtered checks (plan_sites), then the model, field by field
int plan_activity(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_activity_model_t* model,
                  int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end, ActivityCall& call) {
  static_assert(CALITAS_ACTIVITY_MAX_FLANK + MAX_L + CALITAS_ACTIVITY_MAX_FLANK == ACTIVITY_MAX_W, "the kernel's three words hold the widest window");
  static_assert(ACTIVITY_NONE == CALITAS_ACTIVITY_NONE, "the kernel stores the contract's value");
  if (int rc = plan_sites(c, pattern, filter, chrom_index, start, end, call.site)) return rc;
  const int L = call.site.tab.pat.proto_len;
  if (!model) return calitas_fail(c, CALITAS_EINVAL, "activity model: model is NULL");
  if (!model->single) return calitas_fail(c, CALITAS_EINVAL, "activity model: single is NULL");
  if (!model->pair) return calitas_fail(c, CALITAS_EINVAL, "activity model: pair is NULL");
  if (!model->gc) return calitas_fail(c, CALITAS_EINVAL, "activity model: gc is NULL");
  if (model->protospacer_length != L)
    return calitas_fail(c, CALITAS_EINVAL, "activity model: protospacer_length is " + std::to_string(model->protospacer_length) + ", the pattern's protospacer has " + std::to_string(L) + " bases");
  if (model->up < 0 || model->up > CALITAS_ACTIVITY_MAX_FLANK) return calitas_fail(c, CALITAS_EINVAL, "activity model: up is " + std::to_string(model->up) + ": it is 0 .. 16");
  if (model->down < 0 || model->down > CALITAS_ACTIVITY_MAX_FLANK) return calitas_fail(c, CALITAS_EINVAL, "activity model: down is " + std::to_string(model->down) + ": it is 0 .. 16");
  if (model->link < 0 || model->link > 1) return calitas_fail(c, CALITAS_EINVAL, "activity model: link is " + std::to_string(model->link) + ": it is 0 (identity) or 1 (logistic)");
  const int W = model->up + L + model->down;
  const auto outside = [](int32_t v) { return v < -CALITAS_ACTIVITY_MAX_WEIGHT || v > CALITAS_ACTIVITY_MAX_WEIGHT; };
  if (outside(model->intercept)) return calitas_fail(c, CALITAS_EINVAL, "activity model: intercept lies outside +-1048576 (16.0)");
  const struct { const char* name; const int32_t* at; int n; } tables[3] = {{"single", model->single, 4 * W}, {"pair", model->pair, 16 * (W - 1)}, {"gc", model->gc, L + 1}};
  for (const auto& t : tables)
    for (int i = 0; i < t.n; i++)
      if (outside(t.at[i])) return calitas_fail(c, CALITAS_EINVAL, std::string("activity model: ") + t.name + "[" + std::to_string(i) + "] lies outside +-1048576 (16.0)");
  call.model = model; call.L = L; call.W = W; call.min_score = min_score; call.threshold = min_score != CALITAS_ACTIVITY_NONE;
  return CALITAS_OK;
}

// The contract on one site, base by base: the window's letters from PackedRef::base_upper, turned as the guide reads, the three sums
// from the caller's tables as they stand.  *flagged: the window lies in the contig and holds an exception base -- a U among them --
// which is when the kernel leaves the site to the host.
int32_t activity_at(const PackedRef& ref, const calitas_activity_model_t& m, const calitas_site_t& s, bool* flagged) {
  const int L = m.protospacer_length, W = m.up + L + m.down;
  const bool minus = s.strand == '-';
  const ContigInfo& ci = ref.contigs[(size_t)s.contig_index];
  const int64_t left = (int64_t)s.protospacer_start - (minus ? m.down : m.up);
  *flagged = false;
  if (left < 0 || (uint64_t)(left + W) > ci.len) return CALITAS_ACTIVITY_NONE;
  int code[ACTIVITY_MAX_W];                                    // the context, 5' to 3' as the guide reads
  bool plain = true;
  for (int j = 0; j < W; j++) {
    const uint64_t g = ci.gbase + (uint64_t)(left + j);
    if ((ref.mask[g >> 5] >> (g & 31)) & 1u) *flagged = true;
    const char ch = ref.base_upper(g);
    const int c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : (ch == 'T' || ch == 'U') ? 3 : -1;
    if (c < 0) plain = false;
    code[minus ? W - 1 - j : j] = minus ? 3 - c : c;
  }
  if (!plain) return CALITAS_ACTIVITY_NONE;
  int32_t sum = m.intercept;
  int gc = 0;
  for (int i = 0; i < W; i++) sum += m.single[4 * i + code[i]];
  for (int i = 0; i + 1 < W; i++) sum += m.pair[16 * i + 4 * code[i] + code[i + 1]];
  for (int i = m.up; i < m.up + L; i++) gc += code[i] == 1 || code[i] == 2;
  return sum + m.gc[gc];
}

inline bool activity_passes(const ActivityCall& call, int32_t score) { return score >= call.min_score; }   // (NONE passes NONE alone)

// the two blocks of the call: room for n records and n scores (at least one each)
int activity_blocks_alloc(calitas_ctx* c, uint64_t n, calitas_site_t** sites, int32_t** scores) {
  *sites = (calitas_site_t*)calitas_out_alloc(std::max<uint64_t>(1, n) * sizeof(calitas_site_t));
  *scores = (int32_t*)calitas_out_alloc(std::max<uint64_t>(1, n) * sizeof(int32_t));
  if (*sites && *scores) return CALITAS_OK;
  calitas_free(*sites); calitas_free(*scores);
  *sites = nullptr; *scores = nullptr;
  return calitas_fail(c, CALITAS_EINVAL, "out of memory");
}

// what the caller gets: the blocks, or the number alone
void activity_hand_over(calitas_site_t* block, int32_t* block_scores, uint64_t n, calitas_site_t** sites, int32_t** scores, uint64_t* n_sites) {
  *n_sites = n;
  if (sites) { *sites = block; *scores = block_scores; }
  else { calitas_free(block); calitas_free(block_scores); }
}

}  // namespace

int calitas_find_sites_scored_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                        const calitas_activity_model_t* model, int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end,
                                        calitas_site_t** sites, int32_t** scores, uint64_t* n_sites) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  ActivityCall call;
  if (int rc = plan_activity(c, pattern, filter, model, min_score, chrom_index, start, end, call)) return rc;
  std::vector<calitas_site_t> found;
  for (int i = call.site.c_first; i <= call.site.c_last; i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    host_sites(ctx->ref, call.site.tab.pat, filter, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
  }
  calitas_site_t* block = nullptr;
  int32_t* block_scores = nullptr;
  if (int rc = activity_blocks_alloc(c, found.size(), &block, &block_scores)) return rc;
  uint64_t n = 0;
  for (const calitas_site_t& s : found) {
    bool flagged = false;
    const int32_t score = activity_at(ctx->ref, *model, s, &flagged);
    if (!activity_passes(call, score)) continue;
    block[n] = s; block_scores[n] = score; n++;
  }
  activity_hand_over(block, block_scores, n, sites, scores, n_sites);
  return CALITAS_OK;
}

int calitas_find_sites_scored_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_activity_model_t* model,
                                   int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, int32_t** scores,
                                   uint64_t* n_sites) {
  ActivityCall call;
  if (int rc = plan_activity(ctx, pattern, filter, model, min_score, chrom_index, start, end, call)) return rc;
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_sites_scored needs a GPU (there is no CPU fallback; calitas_find_sites_scored_host is the host twin)");
  const PackedRef& ref = ctx->ref;
  const size_t nc = ref.contigs.size();
  calitas_site_t* block = nullptr;
  int32_t* block_scores = nullptr;
  if (nc == 0) {                                  // nothing to scan
    if (int rc = activity_blocks_alloc(ctx, 0, &block, &block_scores)) return rc;
    activity_hand_over(block, block_scores, 0, sites, scores, n_sites);
    return CALITAS_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;

  // calitas_find_sites' two passes as they are; the records stay in d_out
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.site, chrom_index, start, end, w, a)) return rc;
  const uint32_t n_blocks = a.n_segs;
  if (w->blocks_cap < (size_t)n_blocks + 1) {
    (void)hipFree(w->d_count); (void)hipFree(w->d_off); w->d_count = nullptr; w->d_off = nullptr; w->blocks_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_count, ((size_t)n_blocks + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_off, ((size_t)n_blocks + 1) * sizeof(uint64_t)));
    w->blocks_cap = (size_t)n_blocks + 1;
  }
  if (w->totals_cap < 2 * nc) {
    (void)hipFree(w->d_totals); w->d_totals = nullptr; w->totals_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_totals, 2 * nc * sizeof(unsigned long long)));
    w->totals_cap = 2 * nc;
  }
  a.wg_count = w->d_count; a.totals = w->d_totals; a.wg_offset = w->d_off; a.out = nullptr; a.out_capacity = 0;
  uint64_t n_dev = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.site.tab, filter ? sizeof(SiteTables) : sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_totals, 0, 2 * nc * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_sites_count(a, filter != nullptr, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_count, w->d_off, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&n_dev, w->d_off + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const char* const no_room = "the site records and their scores do not fit the device: list the region in pieces";
  if (n_dev / ACTIVITY_THREADS >= 0x7FFFFFFFull) return calitas_fail(ctx, CALITAS_ENOMEM, no_room);
  uint64_t n_kept = n_dev;
  const SiteRecord* d_recs = nullptr;
  const int32_t* d_scores = nullptr;
  std::vector<int32_t> table;                     // (uploaded from here: it lives until the call's last wait)
  if (n_dev) {
    if (w->out_cap < n_dev) {
      (void)hipFree(w->d_out); w->d_out = nullptr; w->out_cap = 0;
      if (hipMalloc((void**)&w->d_out, n_dev * sizeof(SiteRecord)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->out_cap = n_dev;
    }
    if (w->act_scores_cap < n_dev) {
      (void)hipFree(w->d_act_scores); w->d_act_scores = nullptr; w->act_scores_cap = 0;
      if (hipMalloc((void**)&w->d_act_scores, n_dev * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->act_scores_cap = n_dev;
    }
    const uint32_t act_blocks = activity_blocks(n_dev);
    if (call.threshold && w->act_blocks_cap < (size_t)act_blocks + 1) {
      (void)hipFree(w->d_act_count); (void)hipFree(w->d_act_off); w->d_act_count = nullptr; w->d_act_off = nullptr; w->act_blocks_cap = 0;
      HIP_TRY(ctx, hipMalloc((void**)&w->d_act_count, ((size_t)act_blocks + 1) * sizeof(uint32_t)));
      HIP_TRY(ctx, hipMalloc((void**)&w->d_act_off, ((size_t)act_blocks + 1) * sizeof(uint64_t)));
      w->act_blocks_cap = (size_t)act_blocks + 1;
    }
    if (!w->d_act_table) HIP_TRY(ctx, hipMalloc((void**)&w->d_act_table, ACTIVITY_TABLE_MAX_WORDS * sizeof(int32_t)));
    a.out = w->d_out; a.out_capacity = n_dev;

    // the model as the kernel reads it: single folded into pair (integer sums: exact), the last position's single, gc, the intercept
    const int W = call.W, L = call.L;
    table.resize(activity_table_words(L, W));
    for (int i = 0; i + 1 < W; i++)
      for (int ab = 0; ab < 16; ab++) table[(size_t)(16 * i + ab)] = model->pair[16 * i + ab] + model->single[4 * i + (ab >> 2)];
    int32_t* tail = table.data() + 16 * (W - 1);
    for (int b = 0; b < 4; b++) tail[b] = model->single[4 * (W - 1) + b];
    for (int g = 0; g <= L; g++) tail[4 + g] = model->gc[g];
    tail[4 + L + 1] = model->intercept;

    ActivityArgs s{};
    s.planes = ctx->d_planes; s.mask = ctx->d_mask; s.contigs = ctx->d_contigs; s.table = w->d_act_table; s.recs = w->d_out; s.scores = w->d_act_scores;
    s.wg_kept = call.threshold ? w->d_act_count : nullptr;
    s.n = n_dev; s.n_words = ref.total_packed / 32; s.n_contigs = (int32_t)nc; s.L = L; s.up = model->up; s.down = model->down; s.min_score = min_score;
    HIP_TRY(ctx, launch_sites_write(a, filter != nullptr, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w->d_act_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_activity_score(s, ctx->stream));
    d_recs = w->d_out; d_scores = w->d_act_scores;
    if (call.threshold) {
      HIP_TRY(ctx, launch_sites_offsets(w->d_act_count, w->d_act_off, act_blocks, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(&n_kept, w->d_act_off + act_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));             // (the table's host copy is done with as well)
      if (n_kept > n_dev) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_scored: more records kept than written (internal error)");
      if (n_kept && w->act_out_cap < n_kept) {
        (void)hipFree(w->d_act_out); (void)hipFree(w->d_act_out_scores); w->d_act_out = nullptr; w->d_act_out_scores = nullptr; w->act_out_cap = 0;
        if (hipMalloc((void**)&w->d_act_out, n_kept * sizeof(SiteRecord)) != hipSuccess || hipMalloc((void**)&w->d_act_out_scores, n_kept * sizeof(int32_t)) != hipSuccess) {
          (void)hipGetLastError();
          (void)hipFree(w->d_act_out); w->d_act_out = nullptr;
          return calitas_fail(ctx, CALITAS_ENOMEM, no_room);
        }
        w->act_out_cap = n_kept;
      }
      if (n_kept) HIP_TRY(ctx, launch_activity_compact(w->d_out, w->d_act_scores, n_dev, min_score, w->d_act_off, w->d_act_out, w->d_act_out_scores, n_kept, ctx->stream));
      d_recs = w->d_act_out; d_scores = w->d_act_out_scores;
    }
  }

  // a U is a T to a site and an exception base to the kernels: the sites the site kernel did not see, and what it has in their place
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.site, start, end, with_u, kernel_has);
  if (int rc = activity_blocks_alloc(ctx, n_kept + with_u.size(), &block, &block_scores)) return rc;
  int rc = CALITAS_OK;
  do {   // (one exit that releases the blocks)
    hipError_t e = hipSuccess;
    if ((n_kept && ((e = hipMemcpyAsync(block, d_recs, n_kept * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
                    (e = hipMemcpyAsync(block_scores, d_scores, n_kept * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)) ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
      rc = calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_sites_scored: ") + hipGetErrorString(e));
      break;
    }
    // A record the site kernel has beside a U is in the block exactly when its own score passes or its window was left to the host
    // (both lists are in output order); it goes.
    bool gaps = false;
    calitas_site_t* const end_dev = block + n_kept;
    for (const calitas_site_t& s : kernel_has) {
      bool flagged = false;
      const int32_t score = activity_at(ref, *model, s, &flagged);
      const bool expected = flagged || activity_passes(call, score);
      calitas_site_t* at = std::lower_bound(block, end_dev, s, site_less);
      const bool there = at != end_dev && std::memcmp(at, &s, sizeof(s)) == 0;
      if (there != expected) { rc = calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_scored: the records beside a U are not the ones the host expects (internal error)"); break; }
      if (there) { at->contig_index = -1; gaps = true; }
    }
    if (rc) break;
    // the windows the kernel left to the host: scored base by base, dropped when below the threshold
    for (uint64_t i = 0; i < n_kept; i++) {
      if (block_scores[i] != ACTIVITY_HOST_DECIDES || block[i].contig_index < 0) continue;
      bool flagged = false;
      const int32_t score = activity_at(ref, *model, block[i], &flagged);
      if (activity_passes(call, score)) block_scores[i] = score;
      else { block[i].contig_index = -1; gaps = true; }
    }
    uint64_t n = n_kept;
    if (gaps) {
      n = 0;
      for (uint64_t i = 0; i < n_kept; i++)
        if (block[i].contig_index >= 0) { block[n] = block[i]; block_scores[n] = block_scores[i]; n++; }
    }
    // the sites with a U in their footprint come in with the host's scores, each at its place: a merge from the back that ends
    // with the last of them
    std::vector<int32_t> u_scores;
    size_t n_in = 0;
    for (const calitas_site_t& s : with_u) {
      bool flagged = false;
      const int32_t score = activity_at(ref, *model, s, &flagged);
      if (!activity_passes(call, score)) continue;
      with_u[n_in++] = s; u_scores.push_back(score);
    }
    for (uint64_t i = n, j = n_in, k = n + n_in; j > 0; k--) {
      if (i > 0 && site_less(with_u[j - 1], block[i - 1])) { block[k - 1] = block[i - 1]; block_scores[k - 1] = block_scores[i - 1]; i--; }
      else { block[k - 1] = with_u[j - 1]; block_scores[k - 1] = u_scores[j - 1]; j--; }
    }
    activity_hand_over(block, block_scores, n + n_in, sites, scores, n_sites);
  } while (0);
  if (rc) { calitas_free(block); calitas_free(block_scores); }
  return rc;
}

// ---- calitas_find_sites_regions: the sites of a pattern classed by the context's annotated regions ----

namespace calitas {

// The presence table of the context's region set: one byte per segment of the site pass over the whole packed space.  Bit c of a
// segment's byte: some base of its contig within [segment start - SITE_MAX_FOOT, segment end + SITE_MAX_FOOT) has class c in the
// flattened set, bit 0 standing for the bases of no interval.  An extent of a site that starts in the segment lies inside its
// protospacer, so inside that stretch, and its class is the class of one of its bases (or 0 when all of them have 0): the site's class
// has its bit set whatever the extent and the strand.  One walk over the segments, each begun at its coarse entry.
std::string site_presence(calitas_ctx* c, const std::vector<uint8_t>** out) {
  *out = &c->site_presence;
  if (c->site_presence_regions == c->regions.serial && c->site_presence_ref == c->ref_serial) return "";
  const PackedRef& ref = c->ref;
  const RegionsHost& rh = c->regions;
  constexpr uint64_t SEG = 32ull * SITES_BLOCK_WORDS;
  if (ref.tile == 0 || ref.tile % SEG != 0) return "the scan tiles are not whole segments of the site pass (internal error)";
  std::vector<uint8_t>& t = c->site_presence;
  t.assign((size_t)(ref.total_packed / SEG), 0);
  c->site_presence_regions = 0;
  for (size_t ci = 0; ci < ref.contigs.size(); ci++) {
    const ContigInfo& k = ref.contigs[ci];
    if (k.len == 0 || ref.is_absent(ci)) continue;
    if (k.gbase % ref.tile != 0) return "a contig does not start on a tile boundary (internal error)";
    const uint32_t s1 = rh.contig[2 * ci + 2], cb = rh.contig[2 * ci + 1];
    const uint64_t nb = (k.len + SEG - 1) / SEG, first = k.gbase / SEG;
    if (first + nb > t.size()) return "a contig leaves the packed space (internal error)";
    for (uint64_t b = 0; b < nb; b++) {
      const uint64_t lo = b * SEG > (uint64_t)SITE_MAX_FOOT ? b * SEG - SITE_MAX_FOOT : 0, hi = std::min<uint64_t>(k.len, (b + 1) * SEG + SITE_MAX_FOOT);
      uint32_t i = rh.coarse[cb + (lo >> REGION_COARSE_SHIFT)];
      while (i + 1 < s1 && (uint64_t)rh.seg[i + 1].start <= lo) i++;
      uint32_t bits = 0;
      for (; i < s1 && (uint64_t)rh.seg[i].start < hi; i++) bits |= 1u << rh.seg[i].cls;
      t[(size_t)(first + b)] = (uint8_t)bits;
    }
  }
  c->site_presence_regions = rh.serial;
  c->site_presence_ref = c->ref_serial;
  return "";
}

}  // namespace calitas

namespace {

struct RegionsCall {
  SiteCall site;
  uint32_t mask = 0;                 // class_mask's bits below n_classes
  int L = 0, from = 0, to = 0;       // the extent, {0, 0} resolved
};

// checked in this order: what calitas_find_sites_filtered checks (plan_sites), then opt, the context's set, the mask, the extent, reserved
int plan_site_regions(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_regions_t* opt,
                      int32_t chrom_index, uint64_t start, uint64_t end, RegionsCall& call) {
  if (int rc = plan_sites(c, pattern, filter, chrom_index, start, end, call.site)) return rc;
  call.L = call.site.tab.pat.proto_len;
  if (!opt) return calitas_fail(c, CALITAS_EINVAL, "site regions: opt is NULL");
  if (c->regions.empty()) return calitas_fail(c, CALITAS_EINVAL, "site regions: the context has no regions (calitas_set_regions)");
  call.mask = opt->class_mask & ((1u << c->regions.n_classes) - 1u);
  if (call.mask == 0) return calitas_fail(c, CALITAS_EINVAL, "site regions: class_mask has no bit below n_classes (" + std::to_string(c->regions.n_classes) + ")");
  call.from = opt->ext_from; call.to = opt->ext_to;
  if (call.from == 0 && call.to == 0) call.to = call.L;
  else if (call.from >= call.to || call.to > call.L)
    return calitas_fail(c, CALITAS_EINVAL, "site regions: ext_from " + std::to_string(call.from) + ", ext_to " + std::to_string(call.to) + ": 0 <= ext_from < ext_to <= " + std::to_string(call.L) + ", the protospacer's length, or both 0");
  if (opt->reserved != 0) return calitas_fail(c, CALITAS_EINVAL, "site regions: reserved must be 0");
  return CALITAS_OK;
}

inline uint32_t class_of_site(const calitas_ctx* c, const RegionsCall& call, const calitas_site_t& s) {
  return site_region_class(c->regions.view(), (uint32_t)s.contig_index, s.protospacer_start, call.L, s.strand == '-', call.from, call.to,
                           c->ref.contigs[(size_t)s.contig_index].len);
}
inline bool class_kept(const RegionsCall& call, uint32_t cls) { return ((call.mask >> cls) & 1u) != 0; }

// the two blocks of a listing: room for n records and n class bytes (at least one each)
int regions_blocks_alloc(calitas_ctx* c, uint64_t n, calitas_site_t** sites, uint8_t** classes) {
  *sites = (calitas_site_t*)calitas_out_alloc(std::max<uint64_t>(1, n) * sizeof(calitas_site_t));
  *classes = (uint8_t*)calitas_out_alloc(std::max<uint64_t>(1, n));
  if (*sites && *classes) return CALITAS_OK;
  calitas_free(*sites); calitas_free(*classes);
  *sites = nullptr; *classes = nullptr;
  return calitas_fail(c, CALITAS_EINVAL, "out of memory");
}

void regions_cells_out(const calitas_ctx* c, const uint64_t (&cells)[SITE_CLASS_CELLS], uint64_t* per_class_strand) {
  if (per_class_strand) std::memcpy(per_class_strand, cells, 2 * (size_t)c->regions.n_classes * sizeof(uint64_t));
}

}  // namespace

int calitas_find_sites_regions_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                         const calitas_site_regions_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, bool listing,
                                         calitas_site_t** sites, uint8_t** classes, uint64_t* per_class_strand, uint64_t* n_sites) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  RegionsCall call;
  if (int rc = plan_site_regions(c, pattern, filter, opt, chrom_index, start, end, call)) return rc;
  std::vector<calitas_site_t> found;
  for (int i = call.site.c_first; i <= call.site.c_last; i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    host_sites(ctx->ref, call.site.tab.pat, filter, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
  }
  std::vector<uint8_t> cls_of;
  uint64_t cells[SITE_CLASS_CELLS] = {};
  size_t n = 0;
  for (const calitas_site_t& s : found) {
    const uint32_t cls = class_of_site(ctx, call, s);
    if (!class_kept(call, cls)) continue;
    found[n++] = s; cls_of.push_back((uint8_t)cls);
    cells[2 * cls + (s.strand == '-' ? 1 : 0)]++;
  }
  *n_sites = n;
  regions_cells_out(ctx, cells, per_class_strand);
  if (!listing) return CALITAS_OK;
  if (int rc = regions_blocks_alloc(c, n, sites, classes)) return rc;
  if (n) { std::memcpy(*sites, found.data(), n * sizeof(calitas_site_t)); std::memcpy(*classes, cls_of.data(), n); }
  return CALITAS_OK;
}

int calitas_find_sites_regions_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_regions_t* opt,
                                    int32_t chrom_index, uint64_t start, uint64_t end, bool listing, calitas_site_t** sites, uint8_t** classes,
                                    uint64_t* per_class_strand, uint64_t* n_sites) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_sites_regions needs a GPU (there is no CPU fallback; calitas_find_sites_regions_host is the host twin)");
  RegionsCall call;
  if (int rc = plan_site_regions(ctx, pattern, filter, opt, chrom_index, start, end, call)) return rc;
  const PackedRef& ref = ctx->ref;
  const size_t nc = ref.contigs.size();
  uint64_t cells[SITE_CLASS_CELLS] = {};
  if (nc == 0) {                                  // nothing to scan
    regions_cells_out(ctx, cells, per_class_strand);
    return listing ? regions_blocks_alloc(ctx, 0, sites, classes) : CALITAS_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;

  // calitas_find_sites' two passes; with the skip (the default) a segment no wanted class comes near is dead in both
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.site, chrom_index, start, end, w, a)) return rc;
  const uint32_t n_blocks = a.n_segs;
  bool skip = true;
  if (const char* e = TUNE_GET("CALITAS_SITES_SKIP")) skip = std::atoi(e) != 0;
  if (skip) {
    const std::vector<uint8_t>* table = nullptr;
    const std::string e = site_presence(ctx, &table);
    if (!e.empty()) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_regions: " + e);
    if (a.w0 / SITES_BLOCK_WORDS + n_blocks > table->size()) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_regions: the launch leaves the presence table (internal error)");
    if (w->presence_regions != ctx->regions.serial || w->presence_ref != ctx->ref_serial) {
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));            // (nothing queued still reads the old copy)
      if (w->presence_cap < table->size()) {
        (void)hipFree(w->d_presence); w->d_presence = nullptr; w->presence_cap = 0;
        HIP_TRY(ctx, hipMalloc((void**)&w->d_presence, std::max<size_t>(1, table->size())));
        w->presence_cap = std::max<size_t>(1, table->size());
      }
      w->presence_regions = 0;
      if (!table->empty()) HIP_TRY(ctx, hipMemcpy(w->d_presence, table->data(), table->size(), hipMemcpyHostToDevice));
      w->presence_regions = ctx->regions.serial; w->presence_ref = ctx->ref_serial;
    }
    a.presence = w->d_presence; a.class_mask = call.mask;
  }
  if (w->blocks_cap < (size_t)n_blocks + 1) {
    (void)hipFree(w->d_count); (void)hipFree(w->d_off); w->d_count = nullptr; w->d_off = nullptr; w->blocks_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_count, ((size_t)n_blocks + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_off, ((size_t)n_blocks + 1) * sizeof(uint64_t)));
    w->blocks_cap = (size_t)n_blocks + 1;
  }
  if (w->totals_cap < 2 * nc) {
    (void)hipFree(w->d_totals); w->d_totals = nullptr; w->totals_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_totals, 2 * nc * sizeof(unsigned long long)));
    w->totals_cap = 2 * nc;
  }
  a.wg_count = w->d_count; a.totals = w->d_totals; a.wg_offset = w->d_off; a.out = nullptr; a.out_capacity = 0;
  uint64_t n_dev = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.site.tab, filter ? sizeof(SiteTables) : sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_totals, 0, 2 * nc * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, skip ? launch_sites_regions_count(a, filter != nullptr, ctx->stream) : launch_sites_count(a, filter != nullptr, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_count, w->d_off, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&n_dev, w->d_off + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const char* const no_room = "the site records and their classes do not fit the device: list the region in pieces";
  if (n_dev / SITE_CLASS_THREADS >= 0x7FFFFFFFull) return calitas_fail(ctx, CALITAS_ENOMEM, no_room);

  // the records stay in d_out: a lane per record classes its extent, the workgroups' kept counts are scanned
  uint64_t n_kept = 0;
  const uint32_t cls_blocks = site_class_blocks(n_dev);
  if (n_dev) {
    if (w->out_cap < n_dev) {
      (void)hipFree(w->d_out); w->d_out = nullptr; w->out_cap = 0;
      if (hipMalloc((void**)&w->d_out, n_dev * sizeof(SiteRecord)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->out_cap = n_dev;
    }
    if (w->reg_cls_cap < n_dev) {
      (void)hipFree(w->d_reg_cls); w->d_reg_cls = nullptr; w->reg_cls_cap = 0;
      if (hipMalloc((void**)&w->d_reg_cls, n_dev) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->reg_cls_cap = n_dev;
    }
    if (w->reg_blocks_cap < (size_t)cls_blocks + 1) {
      (void)hipFree(w->d_reg_count); (void)hipFree(w->d_reg_off); w->d_reg_count = nullptr; w->d_reg_off = nullptr; w->reg_blocks_cap = 0;
      HIP_TRY(ctx, hipMalloc((void**)&w->d_reg_count, ((size_t)cls_blocks + 1) * sizeof(uint32_t)));
      HIP_TRY(ctx, hipMalloc((void**)&w->d_reg_off, ((size_t)cls_blocks + 1) * sizeof(uint64_t)));
      w->reg_blocks_cap = (size_t)cls_blocks + 1;
    }
    if (!w->d_reg_cells) HIP_TRY(ctx, hipMalloc((void**)&w->d_reg_cells, SITE_CLASS_CELLS * sizeof(unsigned long long)));
    a.out = w->d_out; a.out_capacity = n_dev;
    SiteClassArgs s{};
    s.recs = w->d_out; s.contigs = ctx->d_contigs;
    s.rv = RegionsView{ctx->d_region_seg, ctx->d_region_coarse, ctx->d_region_contig, ctx->regions.n_classes};
    s.cls = w->d_reg_cls; s.wg_kept = w->d_reg_count; s.cells = w->d_reg_cells;
    s.n = n_dev; s.n_contigs = (int32_t)nc; s.ext_from = call.from; s.ext_to = call.to; s.class_mask = call.mask;
    HIP_TRY(ctx, skip ? launch_sites_regions_write(a, filter != nullptr, ctx->stream) : launch_sites_write(a, filter != nullptr, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w->d_reg_cells, 0, SITE_CLASS_CELLS * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, launch_site_class(s, ctx->stream));
    HIP_TRY(ctx, launch_sites_offsets(w->d_reg_count, w->d_reg_off, cls_blocks, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&n_kept, w->d_reg_off + cls_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(cells, w->d_reg_cells, sizeof(cells), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t in_cells = 0;
    for (uint64_t v : cells) in_cells += v;
    if (n_kept > n_dev || in_cells != n_kept) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_regions: the kept counts do not add up (internal error)");
  }

  // A U is a T to a site and an exception base to the kernels: the sites the site kernel did not see, and what it has in their place.
  // Both are classed here, by the same function on the host's copy of the set.  A record the kernel has in their place is on the
  // device's list exactly when its class is kept: a kept class has its bit in the presence byte of the record's segment, so the
  // segment was not skipped; a record of another class is dropped by the class kernel, or was never written.
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.site, start, end, with_u, kernel_has);
  std::vector<uint8_t> u_cls;
  size_t n_in = 0;
  for (const calitas_site_t& s : with_u) {
    const uint32_t cls = class_of_site(ctx, call, s);
    if (!class_kept(call, cls)) continue;
    with_u[n_in++] = s; u_cls.push_back((uint8_t)cls);
    cells[2 * cls + (s.strand == '-' ? 1 : 0)]++;
  }
  if (!listing) {
    uint64_t n_out = 0;
    for (const calitas_site_t& s : kernel_has) {
      const uint32_t cls = class_of_site(ctx, call, s);
      if (!class_kept(call, cls)) continue;
      if (cells[2 * cls + (s.strand == '-' ? 1 : 0)] == 0) return calitas_fail(ctx, CALITAS_EHIP, "calitas_count_sites_regions: the records beside a U are not the ones the host expects (internal error)");
      cells[2 * cls + (s.strand == '-' ? 1 : 0)]--; n_out++;
    }
    *n_sites = n_kept + n_in - n_out;
    regions_cells_out(ctx, cells, per_class_strand);
    return CALITAS_OK;
  }

  if (n_kept && w->reg_out_cap < n_kept) {
    (void)hipFree(w->d_reg_out); (void)hipFree(w->d_reg_out_cls); w->d_reg_out = nullptr; w->d_reg_out_cls = nullptr; w->reg_out_cap = 0;
    if (hipMalloc((void**)&w->d_reg_out, n_kept * sizeof(SiteRecord)) != hipSuccess || hipMalloc((void**)&w->d_reg_out_cls, n_kept) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(w->d_reg_out); w->d_reg_out = nullptr;
      return calitas_fail(ctx, CALITAS_ENOMEM, no_room);
    }
    w->reg_out_cap = n_kept;
  }
  if (n_kept) HIP_TRY(ctx, launch_site_class_compact(w->d_out, w->d_reg_cls, n_dev, w->d_reg_off, w->d_reg_out, w->d_reg_out_cls, n_kept, ctx->stream));
  calitas_site_t* block = nullptr;
  uint8_t* block_cls = nullptr;
  if (int rc = regions_blocks_alloc(ctx, n_kept + n_in, &block, &block_cls)) return rc;
  int rc = CALITAS_OK;
  do {   // (one exit that releases the blocks)
    hipError_t e = hipSuccess;
    if ((n_kept && ((e = hipMemcpyAsync(block, w->d_reg_out, n_kept * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
                    (e = hipMemcpyAsync(block_cls, w->d_reg_out_cls, n_kept, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)) ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
      rc = calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_sites_regions: ") + hipGetErrorString(e));
      break;
    }
    bool gaps = false;
    calitas_site_t* const end_dev = block + n_kept;
    for (const calitas_site_t& s : kernel_has) {                 // (both lists are in output order)
      const uint32_t cls = class_of_site(ctx, call, s);
      const bool expected = class_kept(call, cls);
      calitas_site_t* at = std::lower_bound(block, end_dev, s, site_less);
      const bool there = at != end_dev && std::memcmp(at, &s, sizeof(s)) == 0;
      if (there != expected || (there && block_cls[at - block] != cls)) { rc = calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_regions: the records beside a U are not the ones the host expects (internal error)"); break; }
      if (there) { at->contig_index = -1; gaps = true; cells[2 * cls + (s.strand == '-' ? 1 : 0)]--; }
    }
    if (rc) break;
    uint64_t n = n_kept;
    if (gaps) {
      n = 0;
      for (uint64_t i = 0; i < n_kept; i++)
        if (block[i].contig_index >= 0) { block[n] = block[i]; block_cls[n] = block_cls[i]; n++; }
    }
    // the sites with a U in their footprint come in with the host's classes, each at its place: a merge from the back
    for (uint64_t i = n, j = n_in, k = n + n_in; j > 0; k--) {
      if (i > 0 && site_less(with_u[j - 1], block[i - 1])) { block[k - 1] = block[i - 1]; block_cls[k - 1] = block_cls[i - 1]; i--; }
      else { block[k - 1] = with_u[j - 1]; block_cls[k - 1] = u_cls[j - 1]; j--; }
    }
    *n_sites = n + n_in;
    regions_cells_out(ctx, cells, per_class_strand);
    *sites = block; *classes = block_cls;
  } while (0);
  if (rc) { calitas_free(block); calitas_free(block_cls); }
  return rc;
}

// ---- calitas_find_site_pairs: the sites of a pattern paired by cut distance and orientation ----

namespace {

struct PairsCall {
  SiteCall site;
  SitePairRule rule{};
};

// checked in this order: what calitas_find_sites_filtered checks (plan_sites), then opt, field by field
int plan_site_pairs(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_pairs_t* opt, int32_t chrom_index,
                    uint64_t start, uint64_t end, PairsCall& call) {
  if (int rc = plan_sites(c, pattern, filter, chrom_index, start, end, call.site)) return rc;
  const int L = call.site.tab.pat.proto_len;
  if (!opt) return calitas_fail(c, CALITAS_EINVAL, "site pairs: opt is NULL");
  if (opt->orientations == 0 || opt->orientations > 15) return calitas_fail(c, CALITAS_EINVAL, "site pairs: orientations " + std::to_string(opt->orientations) + ": a mask of the orientations ++ -+ +- --, 1 .. 15");
  if (opt->reserved[0] != 0 || opt->reserved[1] != 0) return calitas_fail(c, CALITAS_EINVAL, "site pairs: reserved must be 0");
  if (opt->min_distance < 0) return calitas_fail(c, CALITAS_EINVAL, "site pairs: min_distance " + std::to_string(opt->min_distance) + " is negative");
  if (opt->min_distance > opt->max_distance) return calitas_fail(c, CALITAS_EINVAL, "site pairs: min_distance " + std::to_string(opt->min_distance) + " is above max_distance " + std::to_string(opt->max_distance));
  if (opt->max_distance > CALITAS_PAIR_MAX_DISTANCE) return calitas_fail(c, CALITAS_EINVAL, "site pairs: max_distance " + std::to_string(opt->max_distance) + " is above CALITAS_PAIR_MAX_DISTANCE (" + std::to_string(CALITAS_PAIR_MAX_DISTANCE) + ")");
  if (opt->cut_offset > L) return calitas_fail(c, CALITAS_EINVAL, "site pairs: cut_offset " + std::to_string(opt->cut_offset) + " is beyond the protospacer's length, " + std::to_string(L));
  static_assert(SITE_PAIR_MAX_DISTANCE == CALITAS_PAIR_MAX_DISTANCE, "one bound");
  call.rule.min_distance = opt->min_distance; call.rule.max_distance = opt->max_distance;
  call.rule.L = L; call.rule.cut = opt->cut_offset; call.rule.slack = std::abs(L - 2 * (int)opt->cut_offset);
  call.rule.orientations = opt->orientations;
  return CALITAS_OK;
}

int pairs_too_many_sites(calitas_ctx* c, uint64_t n) {
  if (n < (1ull << 32)) return CALITAS_OK;
  return calitas_fail(c, CALITAS_EINVAL, "site pairs: the listing has " + std::to_string(n) + " sites, 2^32 or more: pair the region in pieces");
}

// The pairs of a listing in (i, j) order, the contract as the kernel walks it: per site i the sites j > i of its contig from the first
// whose start min_distance does not rule out to the last whose start max_distance does not.  out == nullptr: the numbers alone.
uint64_t pair_walk(const calitas_site_t* s, uint64_t n, const SitePairRule& rule, std::vector<calitas_site_pair_t>* out, uint64_t (&by)[4]) {
  uint64_t n_pairs = 0;
  const int64_t reach = (int64_t)rule.max_distance + rule.slack;
  for (uint64_t i = 0; i < n; i++) {
    const bool minus = s[i].strand == '-';
    const int32_t cut = site_cut(rule, s[i].protospacer_start, minus);
    uint64_t j = i + 1;
    if (rule.min_distance > rule.slack) {
      calitas_site_t from = s[i];
      from.protospacer_start += rule.min_distance - rule.slack; from.strand = '+';
      j = (uint64_t)(std::lower_bound(s + i + 1, s + n, from, site_less) - s);
    }
    for (; j < n && s[j].contig_index == s[i].contig_index && (int64_t)s[j].protospacer_start - s[i].protospacer_start <= reach; j++) {
      const bool other_minus = s[j].strand == '-';
      const int32_t other_cut = site_cut(rule, s[j].protospacer_start, other_minus);
      const int o = site_pair_orientation(rule, cut, minus, other_cut, other_minus);
      if (o < 0) continue;
      n_pairs++; by[o]++;
      if (!out) continue;
      const int32_t d = other_cut - cut;
      calitas_site_pair_t p{};
      p.left = (uint32_t)(d < 0 ? j : i); p.right = (uint32_t)(d < 0 ? i : j); p.distance = d < 0 ? -d : d; p.orientation = (uint8_t)o;
      out->push_back(p);
    }
  }
  return n_pairs;
}

// what both implementations return from a finished listing: its pairs by pair_walk, as a block
int pairs_from_listing(calitas_ctx* c, const PairsCall& call, const calitas_site_t* s, uint64_t n, bool listing, calitas_site_pair_t** pairs,
                       uint64_t* n_pairs, uint64_t* per_orientation) {
  if (int rc = pairs_too_many_sites(c, n)) return rc;
  std::vector<calitas_site_pair_t> found;
  uint64_t by[4] = {};
  *n_pairs = pair_walk(s, n, call.rule, listing ? &found : nullptr, by);
  if (per_orientation) std::memcpy(per_orientation, by, sizeof(by));
  if (!listing) return CALITAS_OK;
  *pairs = (calitas_site_pair_t*)calitas_out_alloc(std::max<size_t>(1, found.size()) * sizeof(calitas_site_pair_t));
  if (!*pairs) return calitas_fail(c, CALITAS_EINVAL, "out of memory");
  if (!found.empty()) std::memcpy(*pairs, found.data(), found.size() * sizeof(calitas_site_pair_t));
  return CALITAS_OK;
}

}  // namespace

int calitas_find_site_pairs_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                      const calitas_site_pairs_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, bool listing,
                                      calitas_site_t** sites, uint64_t* n_sites, calitas_site_pair_t** pairs, uint64_t* n_pairs,
                                      uint64_t* per_orientation) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  PairsCall call;
  if (int rc = plan_site_pairs(c, pattern, filter, opt, chrom_index, start, end, call)) return rc;
  std::vector<calitas_site_t> found;
  for (int i = call.site.c_first; i <= call.site.c_last; i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    host_sites(ctx->ref, call.site.tab.pat, filter, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
  }
  *n_sites = found.size();
  if (int rc = pairs_from_listing(c, call, found.data(), found.size(), listing, pairs, n_pairs, per_orientation)) return rc;
  if (!listing) return CALITAS_OK;
  *sites = (calitas_site_t*)calitas_out_alloc(std::max<size_t>(1, found.size()) * sizeof(calitas_site_t));
  if (!*sites) { calitas_free(*pairs); *pairs = nullptr; return calitas_fail(c, CALITAS_EINVAL, "out of memory"); }
  if (!found.empty()) std::memcpy(*sites, found.data(), found.size() * sizeof(calitas_site_t));
  return CALITAS_OK;
}

int calitas_find_site_pairs_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_pairs_t* opt,
                                 int32_t chrom_index, uint64_t start, uint64_t end, bool listing, calitas_site_t** sites, uint64_t* n_sites,
                                 calitas_site_pair_t** pairs, uint64_t* n_pairs, uint64_t* per_orientation) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_site_pairs needs a GPU (there is no CPU fallback; calitas_find_site_pairs_host is the host twin)");
  PairsCall call;
  if (int rc = plan_site_pairs(ctx, pattern, filter, opt, chrom_index, start, end, call)) return rc;
  static_assert(sizeof(SitePair) == sizeof(calitas_site_pair_t) && offsetof(SitePair, left) == offsetof(calitas_site_pair_t, left) &&
                offsetof(SitePair, right) == offsetof(calitas_site_pair_t, right) && offsetof(SitePair, distance) == offsetof(calitas_site_pair_t, distance) &&
                offsetof(SitePair, orientation) == offsetof(calitas_site_pair_t, orientation), "the kernel writes calitas_site_pair_t");
  const PackedRef& ref = ctx->ref;
  const size_t nc = ref.contigs.size();
  uint64_t by[4] = {};
  if (per_orientation) std::memcpy(per_orientation, by, sizeof(by));
  if (nc == 0) {                                  // nothing to scan
    if (!listing) return CALITAS_OK;
    *sites = (calitas_site_t*)calitas_out_alloc(sizeof(calitas_site_t));
    *pairs = (calitas_site_pair_t*)calitas_out_alloc(sizeof(calitas_site_pair_t));
    if (*sites && *pairs) return CALITAS_OK;
    calitas_free(*sites); calitas_free(*pairs); *sites = nullptr; *pairs = nullptr;
    return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  }

  // A U is a T to a site and an exception base to the kernels.  Where the region has a site beside one, the listing is the one
  // calitas_find_sites corrects on the host, and its pairs are made here by the host twin's walk: pairs are not patched one by one.
  {
    std::vector<calitas_site_t> with_u, kernel_has;
    sites_with_u(ctx, call.site, start, end, with_u, kernel_has);
    if (!with_u.empty() || !kernel_has.empty()) {
      calitas_site_t* block = nullptr;
      if (int rc = calitas_find_sites_impl(ctx, pattern, filter, chrom_index, start, end, true, &block, nullptr, n_sites)) return rc;
      const int rc = pairs_from_listing(ctx, call, block, *n_sites, listing, pairs, n_pairs, per_orientation);
      if (rc || !listing) calitas_free(block); else *sites = block;
      return rc;
    }
  }

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.site, chrom_index, start, end, w, a)) return rc;
  const uint32_t n_blocks = a.n_segs;
  if (w->blocks_cap < (size_t)n_blocks + 1) {
    (void)hipFree(w->d_count); (void)hipFree(w->d_off); w->d_count = nullptr; w->d_off = nullptr; w->blocks_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_count, ((size_t)n_blocks + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_off, ((size_t)n_blocks + 1) * sizeof(uint64_t)));
    w->blocks_cap = (size_t)n_blocks + 1;
  }
  if (w->totals_cap < 2 * nc) {
    (void)hipFree(w->d_totals); w->d_totals = nullptr; w->totals_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_totals, 2 * nc * sizeof(unsigned long long)));
    w->totals_cap = 2 * nc;
  }
  a.wg_count = w->d_count; a.totals = w->d_totals; a.wg_offset = w->d_off; a.out = nullptr; a.out_capacity = 0;
  uint64_t n_dev = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.site.tab, filter ? sizeof(SiteTables) : sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_totals, 0, 2 * nc * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_sites_count(a, filter != nullptr, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_count, w->d_off, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&n_dev, w->d_off + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_sites = n_dev;
  if (int rc = pairs_too_many_sites(ctx, n_dev)) return rc;
  const char* const no_room = "the site records and their pairs do not fit the device: pair the region in pieces";

  // the records stay in d_out, in listing order: a lane per record counts its partners, the workgroups' sums are scanned
  uint64_t total = 0;
  const uint32_t pair_blocks = site_pair_blocks(n_dev);
  SitePairArgs p{};
  if (n_dev) {
    if (w->out_cap < n_dev) {
      (void)hipFree(w->d_out); w->d_out = nullptr; w->out_cap = 0;
      if (hipMalloc((void**)&w->d_out, n_dev * sizeof(SiteRecord)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->out_cap = n_dev;
    }
    if (w->pair_lanes_cap < n_dev) {
      (void)hipFree(w->d_pair_lanes); w->d_pair_lanes = nullptr; w->pair_lanes_cap = 0;
      if (hipMalloc((void**)&w->d_pair_lanes, n_dev * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->pair_lanes_cap = n_dev;
    }
    if (w->pair_blocks_cap < (size_t)pair_blocks + 1) {
      (void)hipFree(w->d_pair_count); (void)hipFree(w->d_pair_off); w->d_pair_count = nullptr; w->d_pair_off = nullptr; w->pair_blocks_cap = 0;
      HIP_TRY(ctx, hipMalloc((void**)&w->d_pair_count, ((size_t)pair_blocks + 1) * sizeof(uint32_t)));
      HIP_TRY(ctx, hipMalloc((void**)&w->d_pair_off, ((size_t)pair_blocks + 1) * sizeof(uint64_t)));
      w->pair_blocks_cap = (size_t)pair_blocks + 1;
    }
    if (!w->d_pair_by) HIP_TRY(ctx, hipMalloc((void**)&w->d_pair_by, 4 * sizeof(unsigned long long)));
    a.out = w->d_out; a.out_capacity = n_dev;
    p.recs = w->d_out; p.n = n_dev; p.lane_count = w->d_pair_lanes; p.wg_count = w->d_pair_count; p.per_orientation = w->d_pair_by;
    p.wg_offset = w->d_pair_off; p.out = nullptr; p.out_capacity = 0; p.rule = call.rule;
    HIP_TRY(ctx, launch_sites_write(a, filter != nullptr, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w->d_pair_by, 0, 4 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, launch_site_pairs_count(p, ctx->stream));
    HIP_TRY(ctx, launch_sites_offsets(w->d_pair_count, w->d_pair_off, pair_blocks, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&total, w->d_pair_off + pair_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(by, w->d_pair_by, sizeof(by), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (by[0] + by[1] + by[2] + by[3] != total) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_site_pairs: the workgroups' sums do not add up to the orientations' (internal error)");
  }
  *n_pairs = total;
  if (per_orientation) std::memcpy(per_orientation, by, sizeof(by));
  if (!listing) return CALITAS_OK;

  if (total && w->pair_out_cap < total) {
    (void)hipFree(w->d_pair_out); w->d_pair_out = nullptr; w->pair_out_cap = 0;
    if (hipMalloc((void**)&w->d_pair_out, total * sizeof(SitePair)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
    w->pair_out_cap = total;
  }
  calitas_site_t* block = (calitas_site_t*)calitas_out_alloc(std::max<uint64_t>(1, n_dev) * sizeof(calitas_site_t));
  calitas_site_pair_t* block_pairs = (calitas_site_pair_t*)calitas_out_alloc(std::max<uint64_t>(1, total) * sizeof(calitas_site_pair_t));
  int rc = CALITAS_OK;
  do {   // (one exit that releases the blocks)
    if (!block || !block_pairs) { rc = calitas_fail(ctx, CALITAS_EINVAL, "out of memory"); break; }
    hipError_t e = hipSuccess;
    p.out = w->d_pair_out; p.out_capacity = total;
    if ((total && ((e = launch_site_pairs_write(p, ctx->stream)) != hipSuccess ||
                   (e = hipMemcpyAsync(block_pairs, w->d_pair_out, total * sizeof(SitePair), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)) ||
        (n_dev && (e = hipMemcpyAsync(block, w->d_out, n_dev * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
      rc = calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_site_pairs: ") + hipGetErrorString(e));
  } while (0);
  if (rc) { calitas_free(block); calitas_free(block_pairs); return rc; }
  *sites = block; *pairs = block_pairs;
  return CALITAS_OK;
}

// ---- calitas_find_allele_sites: the sites a single-nucleotide variant creates, destroys or changes ----

namespace {

inline bool allele_letter(char ch) { const int c = ch & 0xDF; return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'U'; }

// checked in this order: the pattern as calitas_find_sites checks it (plan_site_pattern), n_snvs, then the SNVs field by field -- of
// the first field that some SNV has wrong, the first SNV that has it wrong
int plan_allele_sites(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, SiteCall& call) {
  if (int rc = plan_site_pattern(c, pattern, nullptr, call)) return rc;
  if (n_snvs >= (1ull << 32)) return calitas_fail(c, CALITAS_EINVAL, "allele sites: n_snvs " + std::to_string(n_snvs) + " is 2^32 or more: pass the SNVs in pieces");
  if (n_snvs && !snvs) return calitas_fail(c, CALITAS_EINVAL, "allele sites: snvs is NULL");
  const PackedRef& ref = c->ref;
  const int64_t nc = (int64_t)ref.contigs.size();
  constexpr uint64_t none = ~0ull;
  uint64_t bad[5] = {none, none, none, none, none};     // contig_index, position, alt, ref, reserved
  for (uint64_t i = 0; i < n_snvs; i++) {
    const calitas_snv_t& v = snvs[i];
    const bool contig_ok = v.contig_index >= 0 && v.contig_index < nc && !ref.is_absent((size_t)v.contig_index);
    if (!contig_ok) { if (bad[0] == none) bad[0] = i; continue; }
    if (bad[1] == none && (v.position < 0 || (uint64_t)v.position >= ref.contigs[(size_t)v.contig_index].len)) bad[1] = i;
    if (bad[2] == none && !allele_letter(v.alt)) bad[2] = i;
    if (bad[3] == none && v.ref != 0 && !allele_letter(v.ref)) bad[3] = i;
    if (bad[4] == none && v.reserved != 0) bad[4] = i;
  }
  if (bad[0] != none) {
    const int32_t ci = snvs[bad[0]].contig_index;
    const bool absent = ci >= 0 && ci < nc;
    return calitas_fail(c, CALITAS_EINVAL, "allele sites: snvs[" + std::to_string(bad[0]) + "].contig_index " + std::to_string(ci) +
                                               (absent ? " is absent from this context (calitas_set_reference with bases == NULL)" : " is out of range"));
  }
  if (bad[1] != none)
    return calitas_fail(c, CALITAS_EINVAL, "allele sites: snvs[" + std::to_string(bad[1]) + "].position " + std::to_string(snvs[bad[1]].position) +
                                               " does not lie on the contig (length " + std::to_string(ref.contigs[(size_t)snvs[bad[1]].contig_index].len) + ")");
  if (bad[2] != none) return calitas_fail(c, CALITAS_EINVAL, "allele sites: snvs[" + std::to_string(bad[2]) + "].alt is not one of A C G T U");
  if (bad[3] != none) return calitas_fail(c, CALITAS_EINVAL, "allele sites: snvs[" + std::to_string(bad[3]) + "].ref is not 0 or one of A C G T U");
  if (bad[4] != none) return calitas_fail(c, CALITAS_EINVAL, "allele sites: snvs[" + std::to_string(bad[4]) + "].reserved must be 0");
  return CALITAS_OK;
}

// A contig's text with one base replaced, letter by letter: the 2-bit code of position x, -1 for a base that is not A C G T U and
// outside the contig.  with < 0: the reference as it is.
struct AlleleText {
  const PackedRef& ref;
  uint64_t gbase;
  int64_t len, at;
  int with;
  int code(int64_t x) const {
    if (x < 0 || x >= len) return -1;
    if (x == at && with >= 0) return with;
    switch (ref.base_upper(gbase + (uint64_t)x)) {
      case 'A': return 0;  case 'C': return 1;  case 'G': return 2;  case 'T': case 'U': return 3;
      default: return -1;
    }
  }
};

// the first PAM whose pattern the text shows at protospacer start p on strand st, or -1
int allele_first_pam(const AlleleText& text, const SitePatterns& pat, int64_t p, int st) {
  for (int k = 0; k < pat.n_pams; k++) {
    const SitePattern& sp = pat.p[k][st];
    bool ok = true;
    for (int d = sp.lo; d < sp.hi && ok; d++) {
      const int code = text.code(p + d);
      const uint32_t set = (sp.sets[(d + 16) >> 3] >> (4 * ((d + 16) & 7))) & 15u;
      ok = code >= 0 && ((set >> code) & 1u) != 0;
    }
    if (ok) return k;
  }
  return -1;
}

// The contract on one SNV, base by base: its status; its records appended to *out (may be null) and counted by kind.
uint8_t allele_sites_of_snv(const PackedRef& ref, const SitePatterns& pat, const calitas_snv_t& v, uint32_t index, std::vector<calitas_allele_site_t>* out,
                            uint64_t (&by)[4]) {
  const ContigInfo& ci = ref.contigs[(size_t)v.contig_index];
  const int64_t pos = v.position;
  const AlleleText on_ref{ref, ci.gbase, (int64_t)ci.len, pos, -1};
  const int ref_code = on_ref.code(pos);
  if (ref_code < 0) return 2;
  if (v.ref != 0 && (int)allele_code(v.ref) != ref_code) return 1;
  if ((int)allele_code(v.alt) == ref_code) return 3;
  const AlleleText on_alt{ref, ci.gbase, (int64_t)ci.len, pos, (int)allele_code(v.alt)};
  const int L = pat.proto_len;
  for (int64_t p = pos - (SITE_MAX_FOOT - 1); p <= pos + MAX_PAM_LEN; p++) {
    for (int st = 0; st < 2; st++) {
      const int k_ref = allele_first_pam(on_ref, pat, p, st), k_alt = allele_first_pam(on_alt, pat, p, st);
      bool covers = false;
      if (k_ref >= 0) covers = pos >= p + pat.p[k_ref][st].lo && pos < p + pat.p[k_ref][st].hi;
      if (k_alt >= 0 && !covers) covers = pos >= p + pat.p[k_alt][st].lo && pos < p + pat.p[k_alt][st].hi;
      if (!covers) continue;
      const int kind = (k_alt >= 0 ? 1 : 0) + (k_ref >= 0 ? 2 : 0);
      by[kind]++;
      if (!out) continue;
      const AlleleText& text = k_alt >= 0 ? on_alt : on_ref;
      calitas_allele_site_t r;
      std::memset(&r, 0, sizeof(r));
      r.site = site_record(pat, v.contig_index, p, st, k_alt >= 0 ? k_alt : k_ref);
      r.snv_index = index;
      r.kind = (uint8_t)kind;
      r.other_pam_index = (kind == 3 && !pat.pamless) ? (int8_t)k_ref : (int8_t)-1;
      r.guide_offset = (int8_t)(st ? p + L - 1 - pos : pos - p);
      for (int i = 0; i < L; i++) {                               // the guide's bases, 5' to 3'
        const int c = st ? 3 - text.code(p + L - 1 - i) : text.code(p + i);
        r.guide_lo |= (uint32_t)(c & 1) << i;
        r.guide_hi |= (uint32_t)(c >> 1) << i;
      }
      out->push_back(r);
    }
  }
  return 0;
}

int allele_block_out(calitas_ctx* c, const std::vector<calitas_allele_site_t>& found, calitas_allele_site_t** sites) {
  *sites = (calitas_allele_site_t*)calitas_out_alloc(std::max<size_t>(1, found.size()) * sizeof(calitas_allele_site_t));
  if (!*sites) return calitas_fail(c, CALITAS_EINVAL, "out of memory");
  if (!found.empty()) std::memcpy(*sites, found.data(), found.size() * sizeof(calitas_allele_site_t));
  return CALITAS_OK;
}

}  // namespace

int calitas_find_allele_sites_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, bool listing,
                                        calitas_allele_site_t** sites, uint64_t* per_kind, uint64_t* n_sites, uint8_t* status) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  SiteCall call;
  if (int rc = plan_allele_sites(c, pattern, snvs, n_snvs, call)) return rc;
  std::vector<calitas_allele_site_t> found;
  uint64_t by[4] = {};
  for (uint64_t i = 0; i < n_snvs; i++) {
    const uint8_t s = allele_sites_of_snv(ctx->ref, call.tab.pat, snvs[i], (uint32_t)i, listing ? &found : nullptr, by);
    if (status) status[i] = s;
  }
  *n_sites = by[1] + by[2] + by[3];
  if (per_kind) std::memcpy(per_kind, by, sizeof(by));
  return listing ? allele_block_out(c, found, sites) : CALITAS_OK;
}

int calitas_find_allele_sites_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, bool listing,
                                   calitas_allele_site_t** sites, uint64_t* per_kind, uint64_t* n_sites, uint8_t* status) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_allele_sites needs a GPU (there is no CPU fallback; calitas_find_allele_sites_host is the host twin)");
  SiteCall call;
  if (int rc = plan_allele_sites(ctx, pattern, snvs, n_snvs, call)) return rc;
  static_assert(sizeof(Snv) == sizeof(calitas_snv_t) && offsetof(Snv, contig) == offsetof(calitas_snv_t, contig_index) &&
                offsetof(Snv, position) == offsetof(calitas_snv_t, position) && offsetof(Snv, ref) == offsetof(calitas_snv_t, ref) &&
                offsetof(Snv, alt) == offsetof(calitas_snv_t, alt) && offsetof(Snv, reserved) == offsetof(calitas_snv_t, reserved), "the kernel reads calitas_snv_t");
  static_assert(sizeof(AlleleSite) == sizeof(calitas_allele_site_t) && offsetof(AlleleSite, snv_index) == offsetof(calitas_allele_site_t, snv_index) &&
                offsetof(AlleleSite, kind) == offsetof(calitas_allele_site_t, kind) && offsetof(AlleleSite, other_pam_index) == offsetof(calitas_allele_site_t, other_pam_index) &&
                offsetof(AlleleSite, guide_offset) == offsetof(calitas_allele_site_t, guide_offset) && offsetof(AlleleSite, guide_lo) == offsetof(calitas_allele_site_t, guide_lo) &&
                offsetof(AlleleSite, guide_hi) == offsetof(calitas_allele_site_t, guide_hi), "the kernel writes calitas_allele_site_t");
  static_assert(ALLELE_MAX_RECORDS == 96 && SITE_MAX_FOOT - 1 + 1 + MAX_PAM_LEN == 64, "the window of starts is one 64-bit vector");
  uint64_t by[4] = {};
  if (per_kind) std::memcpy(per_kind, by, sizeof(by));
  std::vector<calitas_allele_site_t> on_host;
  if (n_snvs == 0) return listing ? allele_block_out(ctx, on_host, sites) : CALITAS_OK;
  const PackedRef& ref = ctx->ref;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;

  // A U is a T to a site and an exception base to the kernel.  The SNVs with one within the 63 bases either side that a footprint over
  // the SNV can reach are decided here, by the twin's walk; the device's copy of such a SNV says so and the kernel leaves it alone.
  if (w->u_serial != ctx->ref_serial) {
    w->u_runs.clear();
    for (const Run& r : ref.runs) if (r.ch == 'U' || r.ch == 'u') w->u_runs.push_back(r);
    w->u_serial = ctx->ref_serial;
  }
  std::vector<Snv> marked;
  std::vector<uint64_t> host_snvs;
  if (!w->u_runs.empty()) {
    for (uint64_t i = 0; i < n_snvs; i++) {
      const uint64_t g = ref.contigs[(size_t)snvs[i].contig_index].gbase + (uint64_t)snvs[i].position;
      const uint64_t from = g >= 63 ? g - 63 : 0;
      const auto at = std::partition_point(w->u_runs.begin(), w->u_runs.end(), [&](const Run& r) { return r.start + r.len <= from; });
      if (at != w->u_runs.end() && at->start <= g + 63) host_snvs.push_back(i);
    }
    if (!host_snvs.empty()) {
      marked.resize(n_snvs);
      std::memcpy(marked.data(), snvs, n_snvs * sizeof(Snv));
      for (uint64_t i : host_snvs) marked[i].reserved = ALLELE_HOST_DECIDES;
    }
  }

  const char* const no_room = "the SNVs and their records do not fit the device: pass the SNVs in pieces";
  const uint32_t n_blocks = allele_blocks(n_snvs);
  if (!w->d_pat) HIP_TRY(ctx, hipMalloc((void**)&w->d_pat, sizeof(SiteTables)));
  if (w->al_snvs_cap < n_snvs) {
    (void)hipFree(w->d_snvs); (void)hipFree(w->d_al_lanes); (void)hipFree(w->d_al_status);
    w->d_snvs = nullptr; w->d_al_lanes = nullptr; w->d_al_status = nullptr; w->al_snvs_cap = 0;
    if (hipMalloc((void**)&w->d_snvs, n_snvs * sizeof(Snv)) != hipSuccess || hipMalloc((void**)&w->d_al_lanes, n_snvs * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void**)&w->d_al_status, n_snvs) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(w->d_snvs); (void)hipFree(w->d_al_lanes); (void)hipFree(w->d_al_status);
      w->d_snvs = nullptr; w->d_al_lanes = nullptr; w->d_al_status = nullptr;
      return calitas_fail(ctx, CALITAS_ENOMEM, no_room);
    }
    w->al_snvs_cap = n_snvs;
  }
  if (w->al_blocks_cap < (size_t)n_blocks + 1) {
    (void)hipFree(w->d_al_count); (void)hipFree(w->d_al_off); w->d_al_count = nullptr; w->d_al_off = nullptr; w->al_blocks_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_al_count, ((size_t)n_blocks + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_al_off, ((size_t)n_blocks + 1) * sizeof(uint64_t)));
    w->al_blocks_cap = (size_t)n_blocks + 1;
  }
  if (!w->d_al_by) HIP_TRY(ctx, hipMalloc((void**)&w->d_al_by, 4 * sizeof(unsigned long long)));

  AlleleArgs a{};
  a.planes = ctx->d_planes; a.mask = ctx->d_mask; a.contigs = ctx->d_contigs; a.pat = &w->d_pat->pat; a.snvs = w->d_snvs; a.n = n_snvs;
  a.n_words = ref.total_packed / 32; a.n_contigs = (int32_t)ref.contigs.size();
  a.lane_count = w->d_al_lanes; a.status = w->d_al_status; a.wg_count = w->d_al_count; a.per_kind = w->d_al_by; a.wg_offset = w->d_al_off;
  a.out = nullptr; a.out_capacity = 0;
  uint64_t total = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_snvs, marked.empty() ? (const void*)snvs : (const void*)marked.data(), n_snvs * sizeof(Snv), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_al_by, 0, 4 * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_allele_count(a, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_al_count, w->d_al_off, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&total, w->d_al_off + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(by, w->d_al_by, sizeof(by), hipMemcpyDeviceToHost, ctx->stream));
  if (status) HIP_TRY(ctx, hipMemcpyAsync(status, w->d_al_status, n_snvs, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (by[1] + by[2] + by[3] != total) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_allele_sites: the workgroups' sums do not add up to the kinds' (internal error)");

  for (uint64_t i : host_snvs) {
    const uint8_t s = allele_sites_of_snv(ref, call.tab.pat, snvs[i], (uint32_t)i, listing ? &on_host : nullptr, by);
    if (status) status[i] = s;
  }
  *n_sites = by[1] + by[2] + by[3];
  if (per_kind) std::memcpy(per_kind, by, sizeof(by));
  if (!listing) return CALITAS_OK;

  if (total && w->al_out_cap < total) {
    (void)hipFree(w->d_al_out); w->d_al_out = nullptr; w->al_out_cap = 0;
    if (hipMalloc((void**)&w->d_al_out, total * sizeof(AlleleSite)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
    w->al_out_cap = total;
  }
  calitas_allele_site_t* block = (calitas_allele_site_t*)calitas_out_alloc(std::max<uint64_t>(1, *n_sites) * sizeof(calitas_allele_site_t));
  if (!block) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  if (total) {
    hipError_t e = hipSuccess;
    a.out = w->d_al_out; a.out_capacity = total;
    if ((e = launch_allele_write(a, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(block, w->d_al_out, total * sizeof(AlleleSite), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
      calitas_free(block);
      return calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_allele_sites: ") + hipGetErrorString(e));
    }
  }
  if (!on_host.empty()) {                          // both stretches are in SNV order and share no SNV
    std::memcpy(block + total, on_host.data(), on_host.size() * sizeof(calitas_allele_site_t));
    std::inplace_merge(block, block + total, block + *n_sites,
                       [](const calitas_allele_site_t& x, const calitas_allele_site_t& y) { return x.snv_index < y.snv_index; });
  }
  *sites = block;
  return CALITAS_OK;
}

// ---- calitas_find_edit_sites: the base-editor guides of a single-nucleotide variant and their bystanders ----

namespace {

// checked in this order: the pattern as calitas_find_sites checks it, the editor field by field, the SNVs as calitas_find_allele_sites
// checks them (plan_allele_sites: its messages name the SNV's field and index)
int plan_edit_sites(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs, uint64_t n_snvs, SiteCall& call,
                    EditRule& rule) {
  if (int rc = plan_site_pattern(c, pattern, nullptr, call)) return rc;
  const int L = call.tab.pat.proto_len;
  if (!allele_letter(edit->from_base)) return calitas_fail(c, CALITAS_EINVAL, "edit sites: from_base is not one of A C G T U");
  if (!allele_letter(edit->to_base)) return calitas_fail(c, CALITAS_EINVAL, "edit sites: to_base is not one of A C G T U");
  if (allele_code(edit->from_base) == allele_code(edit->to_base)) return calitas_fail(c, CALITAS_EINVAL, "edit sites: from_base and to_base are the same base");
  if (edit->window_from >= edit->window_to)
    return calitas_fail(c, CALITAS_EINVAL, "edit sites: window_from " + std::to_string(edit->window_from) + " .. window_to " + std::to_string(edit->window_to) + " is an empty window");
  if (edit->window_to > L)
    return calitas_fail(c, CALITAS_EINVAL, "edit sites: window_to " + std::to_string(edit->window_to) + " lies past the protospacer's " + std::to_string(L) + " bases");
  const int context = edit->context == 0 ? 15 : iupac_mask((unsigned char)edit->context);
  if (context == 0) return calitas_fail(c, CALITAS_EINVAL, "edit sites: context is no IUPAC letter");
  if (edit->correct > 1) return calitas_fail(c, CALITAS_EINVAL, "edit sites: correct is 0 (install) or 1 (correct), not " + std::to_string(edit->correct));
  if (edit->max_bystanders >= 32 && edit->max_bystanders != EDIT_NO_BOUND)
    return calitas_fail(c, CALITAS_EINVAL, "edit sites: max_bystanders is 0 .. 31 or 255 (no bound), not " + std::to_string(edit->max_bystanders));
  if (edit->reserved != 0) return calitas_fail(c, CALITAS_EINVAL, "edit sites: reserved must be 0");
  rule.from = allele_code(edit->from_base); rule.to = allele_code(edit->to_base);
  rule.window_from = edit->window_from; rule.window_to = edit->window_to;
  rule.context = (uint32_t)context; rule.correct = edit->correct; rule.max_bystanders = edit->max_bystanders;
  return plan_allele_sites(c, pattern, snvs, n_snvs, call);
}

// The contract on one SNV, base by base: its status; its records appended to *out (may be null) and counted by bystanders.
uint8_t edit_sites_of_snv(const PackedRef& ref, const SitePatterns& pat, const EditRule& e, const calitas_snv_t& v, uint32_t index,
                          std::vector<calitas_edit_site_t>* out, uint64_t (&by)[4]) {
  const ContigInfo& ci = ref.contigs[(size_t)v.contig_index];
  const int64_t pos = v.position;
  const AlleleText on_ref{ref, ci.gbase, (int64_t)ci.len, pos, -1};
  const int ref_code = on_ref.code(pos);
  if (ref_code < 0) return 2;
  if (v.ref != 0 && (int)allele_code(v.ref) != ref_code) return 1;
  const int alt_code = (int)allele_code(v.alt);
  if (alt_code == ref_code) return 3;
  const int background = e.correct ? alt_code : ref_code, product = e.correct ? ref_code : alt_code;
  const int st = edit_strand(e, (uint32_t)background, (uint32_t)product);
  if (st < 0) return 4;
  const AlleleText text{ref, ci.gbase, (int64_t)ci.len, pos, background};
  const int L = pat.proto_len;
  // base i of the guide at start p, -1 .. L - 1: its code, -1 where there is none
  const auto guide_base = [&](int64_t p, int i) {
    const int c = st ? text.code(p + L - 1 - i) : text.code(p + i);
    return c < 0 ? -1 : st ? 3 - c : c;
  };
  const auto editable = [&](int64_t p, int i) {
    if (i < (int)e.window_from || i >= (int)e.window_to || guide_base(p, i) != (int)e.from) return false;
    if (e.context == 15u) return true;
    const int before = guide_base(p, i - 1);
    return before >= 0 && ((e.context >> before) & 1u) != 0;
  };
  {   // the target's own 5' neighbour: the same bases whatever the start
    const int64_t p = st ? pos - L + 1 + (int64_t)e.window_from : pos - (int64_t)e.window_from;
    if (!editable(p, (int)e.window_from)) return 5;
  }
  const int64_t p0 = st ? pos - L + 1 + (int64_t)e.window_from : pos - (int64_t)e.window_to + 1;   // the first start that holds the SNV in the window
  for (int64_t p = p0; p < p0 + (int64_t)(e.window_to - e.window_from); p++) {
    const int k = allele_first_pam(text, pat, p, st);
    if (k < 0) continue;
    calitas_edit_site_t r;
    std::memset(&r, 0, sizeof(r));
    for (int i = 0; i < L; i++) {
      const int c = guide_base(p, i);
      r.editable |= (uint32_t)(editable(p, i) ? 1 : 0) << i;
      r.guide_lo |= (uint32_t)(c & 1) << i;
      r.guide_hi |= (uint32_t)(c >> 1) << i;
    }
    const int64_t o = st ? p + L - 1 - pos : pos - p;
    if (!((r.editable >> o) & 1u)) continue;                        // (cannot happen: status 5 otherwise)
    const uint32_t bystanders = (uint32_t)__builtin_popcount(r.editable) - 1u;
    if (e.max_bystanders != EDIT_NO_BOUND && bystanders > e.max_bystanders) continue;
    by[bystanders < 3u ? bystanders : 3u]++;
    if (!out) continue;
    r.site = site_record(pat, v.contig_index, p, st, k);
    r.snv_index = index;
    out->push_back(r);
  }
  return 0;
}

int edit_block_out(calitas_ctx* c, const std::vector<calitas_edit_site_t>& found, calitas_edit_site_t** sites) {
  *sites = (calitas_edit_site_t*)calitas_out_alloc(std::max<size_t>(1, found.size()) * sizeof(calitas_edit_site_t));
  if (!*sites) return calitas_fail(c, CALITAS_EINVAL, "out of memory");
  if (!found.empty()) std::memcpy(*sites, found.data(), found.size() * sizeof(calitas_edit_site_t));
  return CALITAS_OK;
}

}  // namespace

int calitas_find_edit_sites_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs,
                                      uint64_t n_snvs, bool listing, calitas_edit_site_t** sites, uint64_t* per_bystanders, uint64_t* n_sites, uint8_t* status) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  SiteCall call;
  EditRule rule{};
  if (int rc = plan_edit_sites(c, pattern, edit, snvs, n_snvs, call, rule)) return rc;
  std::vector<calitas_edit_site_t> found;
  uint64_t by[4] = {};
  for (uint64_t i = 0; i < n_snvs; i++) {
    const uint8_t s = edit_sites_of_snv(ctx->ref, call.tab.pat, rule, snvs[i], (uint32_t)i, listing ? &found : nullptr, by);
    if (status) status[i] = s;
  }
  *n_sites = by[0] + by[1] + by[2] + by[3];
  if (per_bystanders) std::memcpy(per_bystanders, by, sizeof(by));
  return listing ? edit_block_out(c, found, sites) : CALITAS_OK;
}

int calitas_find_edit_sites_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs, uint64_t n_snvs,
                                 bool listing, calitas_edit_site_t** sites, uint64_t* per_bystanders, uint64_t* n_sites, uint8_t* status) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_edit_sites needs a GPU (there is no CPU fallback; calitas_find_edit_sites_host is the host twin)");
  SiteCall call;
  EditRule rule{};
  if (int rc = plan_edit_sites(ctx, pattern, edit, snvs, n_snvs, call, rule)) return rc;
  static_assert(sizeof(EditSite) == sizeof(calitas_edit_site_t) && offsetof(EditSite, snv_index) == offsetof(calitas_edit_site_t, snv_index) &&
                offsetof(EditSite, editable) == offsetof(calitas_edit_site_t, editable) && offsetof(EditSite, guide_lo) == offsetof(calitas_edit_site_t, guide_lo) &&
                offsetof(EditSite, guide_hi) == offsetof(calitas_edit_site_t, guide_hi), "the kernel writes calitas_edit_site_t");
  static_assert(sizeof(calitas_base_edit_t) == 8 && EDIT_MAX_RECORDS == 32 && MAX_L - 1 + MAX_PAM_LEN + SITE_MAX_FOOT <= 96, "the window of starts is one 32-bit vector, its text 96 bases");
  uint64_t by[4] = {};
  if (per_bystanders) std::memcpy(per_bystanders, by, sizeof(by));
  std::vector<calitas_edit_site_t> on_host;
  if (n_snvs == 0) return listing ? edit_block_out(ctx, on_host, sites) : CALITAS_OK;
  const PackedRef& ref = ctx->ref;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;

  // A U is a T to a site and an exception base to the kernel.  Every base a lane's records depend on lies within 63 of its SNV (a
  // footprint over a start that holds the SNV in the window, the base 5' of a protospacer): the SNVs with a U that near are decided
  // here, by the twin's walk; the device's copy of such a SNV says so and the kernel leaves it alone.
  if (w->u_serial != ctx->ref_serial) {
    w->u_runs.clear();
    for (const Run& r : ref.runs) if (r.ch == 'U' || r.ch == 'u') w->u_runs.push_back(r);
    w->u_serial = ctx->ref_serial;
  }
  std::vector<Snv> marked;
  std::vector<uint64_t> host_snvs;
  if (!w->u_runs.empty()) {
    for (uint64_t i = 0; i < n_snvs; i++) {
      const uint64_t g = ref.contigs[(size_t)snvs[i].contig_index].gbase + (uint64_t)snvs[i].position;
      const uint64_t from = g >= 63 ? g - 63 : 0;
      const auto at = std::partition_point(w->u_runs.begin(), w->u_runs.end(), [&](const Run& r) { return r.start + r.len <= from; });
      if (at != w->u_runs.end() && at->start <= g + 63) host_snvs.push_back(i);
    }
    if (!host_snvs.empty()) {
      marked.resize(n_snvs);
      std::memcpy(marked.data(), snvs, n_snvs * sizeof(Snv));
      for (uint64_t i : host_snvs) marked[i].reserved = ALLELE_HOST_DECIDES;
    }
  }

  const char* const no_room = "the SNVs and their records do not fit the device: pass the SNVs in pieces";
  const uint32_t n_blocks = edit_blocks(n_snvs);
  if (!w->d_pat) HIP_TRY(ctx, hipMalloc((void**)&w->d_pat, sizeof(SiteTables)));
  if (w->ed_snvs_cap < n_snvs) {
    (void)hipFree(w->d_ed_snvs); (void)hipFree(w->d_ed_lanes); (void)hipFree(w->d_ed_status);
    w->d_ed_snvs = nullptr; w->d_ed_lanes = nullptr; w->d_ed_status = nullptr; w->ed_snvs_cap = 0;
    if (hipMalloc((void**)&w->d_ed_snvs, n_snvs * sizeof(Snv)) != hipSuccess || hipMalloc((void**)&w->d_ed_lanes, n_snvs * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void**)&w->d_ed_status, n_snvs) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(w->d_ed_snvs); (void)hipFree(w->d_ed_lanes); (void)hipFree(w->d_ed_status);
      w->d_ed_snvs = nullptr; w->d_ed_lanes = nullptr; w->d_ed_status = nullptr;
      return calitas_fail(ctx, CALITAS_ENOMEM, no_room);
    }
    w->ed_snvs_cap = n_snvs;
  }
  if (w->ed_blocks_cap < (size_t)n_blocks + 1) {
    (void)hipFree(w->d_ed_count); (void)hipFree(w->d_ed_off); w->d_ed_count = nullptr; w->d_ed_off = nullptr; w->ed_blocks_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_ed_count, ((size_t)n_blocks + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_ed_off, ((size_t)n_blocks + 1) * sizeof(uint64_t)));
    w->ed_blocks_cap = (size_t)n_blocks + 1;
  }
  if (!w->d_ed_by) HIP_TRY(ctx, hipMalloc((void**)&w->d_ed_by, 4 * sizeof(unsigned long long)));

  EditArgs a{};
  a.planes = ctx->d_planes; a.mask = ctx->d_mask; a.contigs = ctx->d_contigs; a.pat = &w->d_pat->pat; a.snvs = w->d_ed_snvs; a.n = n_snvs;
  a.n_words = ref.total_packed / 32; a.n_contigs = (int32_t)ref.contigs.size();
  a.lane_count = w->d_ed_lanes; a.status = w->d_ed_status; a.wg_count = w->d_ed_count; a.per_bystanders = w->d_ed_by; a.wg_offset = w->d_ed_off;
  a.out = nullptr; a.out_capacity = 0;
  a.rule = rule;
  uint64_t total = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_ed_snvs, marked.empty() ? (const void*)snvs : (const void*)marked.data(), n_snvs * sizeof(Snv), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_ed_by, 0, 4 * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_edit_count(a, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_ed_count, w->d_ed_off, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&total, w->d_ed_off + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(by, w->d_ed_by, sizeof(by), hipMemcpyDeviceToHost, ctx->stream));
  if (status) HIP_TRY(ctx, hipMemcpyAsync(status, w->d_ed_status, n_snvs, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (by[0] + by[1] + by[2] + by[3] != total) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_edit_sites: the workgroups' sums do not add up to the bystander bins' (internal error)");

  for (uint64_t i : host_snvs) {
    const uint8_t s = edit_sites_of_snv(ref, call.tab.pat, rule, snvs[i], (uint32_t)i, listing ? &on_host : nullptr, by);
    if (status) status[i] = s;
  }
  *n_sites = by[0] + by[1] + by[2] + by[3];
  if (per_bystanders) std::memcpy(per_bystanders, by, sizeof(by));
  if (!listing) return CALITAS_OK;

  if (total && w->ed_out_cap < total) {
    (void)hipFree(w->d_ed_out); w->d_ed_out = nullptr; w->ed_out_cap = 0;
    if (hipMalloc((void**)&w->d_ed_out, total * sizeof(EditSite)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
    w->ed_out_cap = total;
  }
  calitas_edit_site_t* block = (calitas_edit_site_t*)calitas_out_alloc(std::max<uint64_t>(1, *n_sites) * sizeof(calitas_edit_site_t));
  if (!block) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  if (total) {
    hipError_t e = hipSuccess;
    a.out = w->d_ed_out; a.out_capacity = total;
    if ((e = launch_edit_write(a, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(block, w->d_ed_out, total * sizeof(EditSite), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
      calitas_free(block);
      return calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_edit_sites: ") + hipGetErrorString(e));
    }
  }
  if (!on_host.empty()) {                          // both stretches are in SNV order and share no SNV
    std::memcpy(block + total, on_host.data(), on_host.size() * sizeof(calitas_edit_site_t));
    std::inplace_merge(block, block + total, block + *n_sites,
                       [](const calitas_edit_site_t& x, const calitas_edit_site_t& y) { return x.snv_index < y.snv_index; });
  }
  *sites = block;
  return CALITAS_OK;
}

// ---- calitas_find_sites_microhomology: every site's microhomology score and the out-of-frame share of it ----

namespace {

struct MhCall {
  SiteCall site;
  const calitas_mh_model_t* model = nullptr;
  int L = 0, W = 0;
  uint32_t permille = 0;             // 0: every site is kept; else mh_kept decides
};

// checked in this order: what calitas_find_sites_filtered checks (plan_sites), then the model, field by field, then the threshold
int plan_microhomology(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_mh_model_t* model,
                       int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end, MhCall& call) {
  static_assert(2 * CALITAS_MH_MAX_SIDE == MH_MAX_W, "the kernel's three words hold the widest window");
  static_assert(MH_NONE == CALITAS_MH_NONE && sizeof(MhScore) == sizeof(calitas_mh_score_t), "the kernel stores the contract's values");
  if (int rc = plan_sites(c, pattern, filter, chrom_index, start, end, call.site)) return rc;
  const int L = call.site.tab.pat.proto_len;
  if (!model) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: model is NULL");
  if (!model->weight) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: weight is NULL");
  if (model->left < 1 || model->left > CALITAS_MH_MAX_SIDE) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: left is " + std::to_string(model->left) + ": it is 1 .. 32");
  if (model->right < 1 || model->right > CALITAS_MH_MAX_SIDE) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: right is " + std::to_string(model->right) + ": it is 1 .. 32");
  if (model->cut_offset < 0 || model->cut_offset > L)
    return calitas_fail(c, CALITAS_EINVAL, "microhomology model: cut_offset is " + std::to_string(model->cut_offset) + ": it is 0 .. " + std::to_string(L) + ", the protospacer's length");
  if (model->min_length < 2 || model->min_length > 8) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: min_length is " + std::to_string(model->min_length) + ": it is 2 .. 8");
  const int W = model->left + model->right;
  for (int d = 1; d < W; d++)
    if (model->weight[d - 1] > CALITAS_MH_MAX_WEIGHT) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: weight[" + std::to_string(d - 1) + "] lies above 65536 (1.0)");
  if (permille < 0 || permille > 1000) return calitas_fail(c, CALITAS_EINVAL, "min_out_of_frame_permille is " + std::to_string(permille) + ": it is 0 .. 1000");
  call.model = model; call.L = L; call.W = W; call.permille = (uint32_t)permille;
  return CALITAS_OK;
}

const calitas_mh_score_t MH_UNSCORED = {CALITAS_MH_NONE, CALITAS_MH_NONE};

// The contract on one site, letter by letter: the window's letters from PackedRef::base_upper, turned as the guide reads, then every
// diagonal d walked from lo(d) to hi(d) with the current run's length and its G + C count.  *flagged: the window lies in the contig
// and holds an exception base -- a U among them -- which is when the kernel leaves the site to the host.
calitas_mh_score_t mh_at(const PackedRef& ref, const calitas_mh_model_t& m, int L, const calitas_site_t& s, bool* flagged) {
  const int left = m.left, right = m.right, W = left + right;
  const bool minus = s.strand == '-';
  const ContigInfo& ci = ref.contigs[(size_t)s.contig_index];
  const int64_t cut = (int64_t)s.protospacer_start + (minus ? L - m.cut_offset : m.cut_offset);
  const int64_t first = cut - (minus ? right : left);
  *flagged = false;
  if (first < 0 || (uint64_t)(first + W) > ci.len) return MH_UNSCORED;
  char x[MH_MAX_W];                                            // the window, 5' to 3' as the guide reads
  bool plain = true;
  for (int j = 0; j < W; j++) {
    const uint64_t g = ci.gbase + (uint64_t)(first + j);
    if ((ref.mask[g >> 5] >> (g & 31)) & 1u) *flagged = true;
    char ch = ref.base_upper(g);
    if (ch == 'U') ch = 'T';
    if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') plain = false;
    if (minus) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
    x[minus ? W - 1 - j : j] = ch;
  }
  if (!plain) return MH_UNSCORED;
  calitas_mh_score_t out = {0, 0};
  for (int d = 1; d < W; d++) {
    const int from = std::max(0, left - d), to = std::min(left, W - d);
    uint32_t units = 0;                                        // the sum of k + g over the diagonal's runs
    int k = 0, g = 0;
    for (int i = from; i <= to; i++) {
      if (i < to && x[i] == x[i + d]) { k++; g += x[i] == 'G' || x[i] == 'C'; continue; }
      if (k >= m.min_length) units += (uint32_t)(k + g);
      k = 0; g = 0;
    }
    const uint32_t term = m.weight[d - 1] * units;
    out.total_q16 += term;
    if (d % 3 != 0) out.out_of_frame_q16 += term;
  }
  return out;
}

inline bool mh_passes(const MhCall& call, const calitas_mh_score_t& v) {
  if (call.permille == 0) return true;
  return v.total_q16 != CALITAS_MH_NONE && v.total_q16 > 0 && (uint64_t)v.out_of_frame_q16 * 1000u >= (uint64_t)call.permille * v.total_q16;
}

// the two blocks of the call: room for n records and n scores (at least one each)
int mh_blocks_alloc(calitas_ctx* c, uint64_t n, calitas_site_t** sites, calitas_mh_score_t** scores) {
  *sites = (calitas_site_t*)calitas_out_alloc(std::max<uint64_t>(1, n) * sizeof(calitas_site_t));
  *scores = (calitas_mh_score_t*)calitas_out_alloc(std::max<uint64_t>(1, n) * sizeof(calitas_mh_score_t));
  if (*sites && *scores) return CALITAS_OK;
  calitas_free(*sites); calitas_free(*scores);
  *sites = nullptr; *scores = nullptr;
  return calitas_fail(c, CALITAS_EINVAL, "out of memory");
}

// what the caller gets: the blocks, or the number alone
void mh_hand_over(calitas_site_t* block, calitas_mh_score_t* block_scores, uint64_t n, calitas_site_t** sites, calitas_mh_score_t** scores, uint64_t* n_sites) {
  *n_sites = n;
  if (sites) { *sites = block; *scores = block_scores; }
  else { calitas_free(block); calitas_free(block_scores); }
}

}  // namespace

int calitas_find_sites_microhomology_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                               const calitas_mh_model_t* model, int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end,
                                               calitas_site_t** sites, calitas_mh_score_t** scores, uint64_t* n_sites) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  MhCall call;
  if (int rc = plan_microhomology(c, pattern, filter, model, permille, chrom_index, start, end, call)) return rc;
  std::vector<calitas_site_t> found;
  for (int i = call.site.c_first; i <= call.site.c_last; i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    host_sites(ctx->ref, call.site.tab.pat, filter, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
  }
  calitas_site_t* block = nullptr;
  calitas_mh_score_t* block_scores = nullptr;
  if (int rc = mh_blocks_alloc(c, found.size(), &block, &block_scores)) return rc;
  uint64_t n = 0;
  for (const calitas_site_t& s : found) {
    bool flagged = false;
    const calitas_mh_score_t score = mh_at(ctx->ref, *model, call.L, s, &flagged);
    if (!mh_passes(call, score)) continue;
    block[n] = s; block_scores[n] = score; n++;
  }
  mh_hand_over(block, block_scores, n, sites, scores, n_sites);
  return CALITAS_OK;
}

int calitas_find_sites_microhomology_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_mh_model_t* model,
                                          int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                          calitas_mh_score_t** scores, uint64_t* n_sites) {
  MhCall call;
  if (int rc = plan_microhomology(ctx, pattern, filter, model, permille, chrom_index, start, end, call)) return rc;
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_sites_microhomology needs a GPU (there is no CPU fallback; calitas_find_sites_microhomology_host is the host twin)");
  const PackedRef& ref = ctx->ref;
  const size_t nc = ref.contigs.size();
  calitas_site_t* block = nullptr;
  calitas_mh_score_t* block_scores = nullptr;
  if (nc == 0) {                                  // nothing to scan
    if (int rc = mh_blocks_alloc(ctx, 0, &block, &block_scores)) return rc;
    mh_hand_over(block, block_scores, 0, sites, scores, n_sites);
    return CALITAS_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;

  // calitas_find_sites' two passes as they are; the records stay in d_out
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.site, chrom_index, start, end, w, a)) return rc;
  const uint32_t n_blocks = a.n_segs;
  if (w->blocks_cap < (size_t)n_blocks + 1) {
    (void)hipFree(w->d_count); (void)hipFree(w->d_off); w->d_count = nullptr; w->d_off = nullptr; w->blocks_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_count, ((size_t)n_blocks + 1) * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&w->d_off, ((size_t)n_blocks + 1) * sizeof(uint64_t)));
    w->blocks_cap = (size_t)n_blocks + 1;
  }
  if (w->totals_cap < 2 * nc) {
    (void)hipFree(w->d_totals); w->d_totals = nullptr; w->totals_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&w->d_totals, 2 * nc * sizeof(unsigned long long)));
    w->totals_cap = 2 * nc;
  }
  a.wg_count = w->d_count; a.totals = w->d_totals; a.wg_offset = w->d_off; a.out = nullptr; a.out_capacity = 0;
  uint64_t n_dev = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat, &call.site.tab, filter ? sizeof(SiteTables) : sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_totals, 0, 2 * nc * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_sites_count(a, filter != nullptr, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_count, w->d_off, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&n_dev, w->d_off + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const char* const no_room = "the site records and their microhomology scores do not fit the device: list the region in pieces";
  if (n_dev / MH_THREADS >= 0x7FFFFFFFull) return calitas_fail(ctx, CALITAS_ENOMEM, no_room);
  const bool threshold = call.permille != 0;
  uint64_t n_kept = n_dev;
  const SiteRecord* d_recs = nullptr;
  const MhScore* d_scores = nullptr;
  if (n_dev) {
    if (w->out_cap < n_dev) {
      (void)hipFree(w->d_out); w->d_out = nullptr; w->out_cap = 0;
      if (hipMalloc((void**)&w->d_out, n_dev * sizeof(SiteRecord)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->out_cap = n_dev;
    }
    if (w->mh_scores_cap < n_dev) {
      (void)hipFree(w->d_mh_scores); w->d_mh_scores = nullptr; w->mh_scores_cap = 0;
      if (hipMalloc((void**)&w->d_mh_scores, n_dev * sizeof(MhScore)) != hipSuccess) { (void)hipGetLastError(); return calitas_fail(ctx, CALITAS_ENOMEM, no_room); }
      w->mh_scores_cap = n_dev;
    }
    const uint32_t mh_wgs = mh_blocks(n_dev);
    if (threshold && w->mh_blocks_cap < (size_t)mh_wgs + 1) {
      (void)hipFree(w->d_mh_count); (void)hipFree(w->d_mh_off); w->d_mh_count = nullptr; w->d_mh_off = nullptr; w->mh_blocks_cap = 0;
      HIP_TRY(ctx, hipMalloc((void**)&w->d_mh_count, ((size_t)mh_wgs + 1) * sizeof(uint32_t)));
      HIP_TRY(ctx, hipMalloc((void**)&w->d_mh_off, ((size_t)mh_wgs + 1) * sizeof(uint64_t)));
      w->mh_blocks_cap = (size_t)mh_wgs + 1;
    }
    a.out = w->d_out; a.out_capacity = n_dev;

    MhArgs s{};                                    // (the weights travel in the argument block)
    s.planes = ctx->d_planes; s.mask = ctx->d_mask; s.contigs = ctx->d_contigs; s.recs = w->d_out; s.scores = w->d_mh_scores;
    s.wg_kept = threshold ? w->d_mh_count : nullptr;
    s.n = n_dev; s.n_words = ref.total_packed / 32; s.n_contigs = (int32_t)nc; s.L = call.L; s.left = model->left; s.right = model->right;
    s.cut = model->cut_offset; s.min_length = model->min_length; s.permille = call.permille;
    for (int d = 1; d < call.W; d++) s.weight[d - 1] = model->weight[d - 1];
    HIP_TRY(ctx, launch_sites_write(a, filter != nullptr, ctx->stream));
    HIP_TRY(ctx, launch_mh_score(s, ctx->stream));
    d_recs = w->d_out; d_scores = w->d_mh_scores;
    if (threshold) {
      HIP_TRY(ctx, launch_sites_offsets(w->d_mh_count, w->d_mh_off, mh_wgs, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(&n_kept, w->d_mh_off + mh_wgs, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      if (n_kept > n_dev) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_microhomology: more records kept than written (internal error)");
      if (n_kept && w->mh_out_cap < n_kept) {
        (void)hipFree(w->d_mh_out); (void)hipFree(w->d_mh_out_scores); w->d_mh_out = nullptr; w->d_mh_out_scores = nullptr; w->mh_out_cap = 0;
        if (hipMalloc((void**)&w->d_mh_out, n_kept * sizeof(SiteRecord)) != hipSuccess || hipMalloc((void**)&w->d_mh_out_scores, n_kept * sizeof(MhScore)) != hipSuccess) {
          (void)hipGetLastError();
          (void)hipFree(w->d_mh_out); w->d_mh_out = nullptr;
          return calitas_fail(ctx, CALITAS_ENOMEM, no_room);
        }
        w->mh_out_cap = n_kept;
      }
      if (n_kept) HIP_TRY(ctx, launch_mh_compact(w->d_out, w->d_mh_scores, n_dev, call.permille, w->d_mh_off, w->d_mh_out, w->d_mh_out_scores, n_kept, ctx->stream));
      d_recs = w->d_mh_out; d_scores = w->d_mh_out_scores;
    }
  }

  // a U is a T to a site and an exception base to the kernels: the sites the site kernel did not see, and what it has in their place
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.site, start, end, with_u, kernel_has);
  if (int rc = mh_blocks_alloc(ctx, n_kept + with_u.size(), &block, &block_scores)) return rc;
  int rc = CALITAS_OK;
  do {   // (one exit that releases the blocks)
    hipError_t e = hipSuccess;
    if ((n_kept && ((e = hipMemcpyAsync(block, d_recs, n_kept * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
                    (e = hipMemcpyAsync(block_scores, d_scores, n_kept * sizeof(MhScore), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)) ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
      rc = calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_sites_microhomology: ") + hipGetErrorString(e));
      break;
    }
    // A record the site kernel has beside a U is in the block exactly when its own score passes or its window was left to the host
    // (both lists are in output order); it goes.
    bool gaps = false;
    calitas_site_t* const end_dev = block + n_kept;
    for (const calitas_site_t& s : kernel_has) {
      bool flagged = false;
      const calitas_mh_score_t score = mh_at(ref, *model, call.L, s, &flagged);
      const bool expected = flagged || mh_passes(call, score);
      calitas_site_t* at = std::lower_bound(block, end_dev, s, site_less);
      const bool there = at != end_dev && std::memcmp(at, &s, sizeof(s)) == 0;
      if (there != expected) { rc = calitas_fail(ctx, CALITAS_EHIP, "calitas_find_sites_microhomology: the records beside a U are not the ones the host expects (internal error)"); break; }
      if (there) { at->contig_index = -1; gaps = true; }
    }
    if (rc) break;
    // the windows the kernel left to the host: walked letter by letter, dropped when below the threshold
    for (uint64_t i = 0; i < n_kept; i++) {
      if (block_scores[i].total_q16 != MH_NONE || block_scores[i].out_of_frame_q16 != MH_HOST_DECIDES || block[i].contig_index < 0) continue;
      bool flagged = false;
      const calitas_mh_score_t score = mh_at(ref, *model, call.L, block[i], &flagged);
      if (mh_passes(call, score)) block_scores[i] = score;
      else { block[i].contig_index = -1; gaps = true; }
    }
    uint64_t n = n_kept;
    if (gaps) {
      n = 0;
      for (uint64_t i = 0; i < n_kept; i++)
        if (block[i].contig_index >= 0) { block[n] = block[i]; block_scores[n] = block_scores[i]; n++; }
    }
    // the sites with a U in their footprint come in with the host's scores, each at its place: a merge from the back that ends
    // with the last of them
    std::vector<calitas_mh_score_t> u_scores;
    size_t n_in = 0;
    for (const calitas_site_t& s : with_u) {
      bool flagged = false;
      const calitas_mh_score_t score = mh_at(ref, *model, call.L, s, &flagged);
      if (!mh_passes(call, score)) continue;
      with_u[n_in++] = s; u_scores.push_back(score);
    }
    for (uint64_t i = n, j = n_in, k = n + n_in; j > 0; k--) {
      if (i > 0 && site_less(with_u[j - 1], block[i - 1])) { block[k - 1] = block[i - 1]; block_scores[k - 1] = block_scores[i - 1]; i--; }
      else { block[k - 1] = with_u[j - 1]; block_scores[k - 1] = u_scores[j - 1]; j--; }
    }
    mh_hand_over(block, block_scores, n + n_in, sites, scores, n_sites);
  } while (0);
  if (rc) { calitas_free(block); calitas_free(block_scores); }
  return rc;
}
