// sites_host.cpp -- calitas_find_sites / calitas_count_sites / calitas_find_sites_host and their _filtered forms: the pattern and the
// filter both implementations share, the host twin (a base-by-base walk over the packed reference) and the driver of sites.hip's two
// passes.  What every later guide-site unit builds on is here as well (sites_work.hpp): the plan of a call, the sites beside a U, the
// launch of a region, the first pass and the room for the second.  No reference counterpart.
#include "sites_work.hpp"
#include "tuning.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

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

void sites_destroy(SitesWork* w) { delete w; }   // (every DevBuf frees its own)

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

const std::vector<Run>& u_runs_of(calitas_ctx* c) {
  if (!c->sites) c->sites = new SitesWork();
  SitesWork* w = c->sites;
  if (w->u_serial != c->ref_serial) {
    w->u_runs.clear();
    for (const Run& r : c->ref.runs) if (r.ch == 'U' || r.ch == 'u') w->u_runs.push_back(r);
    w->u_serial = c->ref_serial;
  }
  return w->u_runs;
}

void sites_with_u(calitas_ctx* c, const SiteCall& call, uint64_t start, uint64_t end, std::vector<calitas_site_t>& with_u,
                  std::vector<calitas_site_t>& kernel_has) {
  const PackedRef& ref = c->ref;
  int64_t done_contig = -1, done_to = 0;            // the runs are in position order: start positions already looked at
  for (const Run& r : u_runs_of(c)) {
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
  HIP_TRY(ctx, w->d_pat.grow(1));
  a = SitesArgs{};
  a.planes = ctx->d_planes; a.mask = ctx->d_mask; a.tiles = ctx->d_tiles; a.contigs = ctx->d_contigs; a.pat = &w->d_pat.p->pat;
  a.n_words = ref.total_packed / 32; a.w0 = w0; a.n_segs = n_blocks; a.segs_per_wg = segs_per_wg; a.tile_words = (uint32_t)(ref.tile / 32); a.chrom_index = chrom_index;
  a.start = start; a.end = end;
  return CALITAS_OK;
}

int sites_first_pass(calitas_ctx* ctx, const SiteCall& call, SitesWork* w, SitesArgs& a, SitesCountLaunch count, uint64_t* n_dev, uint64_t* totals) {
  static_assert(offsetof(SiteTables, pat) == 0, "SitesArgs::pat heads the block");
  const uint32_t n_blocks = a.n_segs;
  const size_t nc = ctx->ref.contigs.size();
  HIP_TRY(ctx, w->d_count.grow((size_t)n_blocks + 1));
  HIP_TRY(ctx, w->d_off.grow((size_t)n_blocks + 1));
  HIP_TRY(ctx, w->d_totals.grow(2 * nc));
  a.wg_count = w->d_count.p; a.totals = w->d_totals.p; a.wg_offset = w->d_off.p; a.out = nullptr; a.out_capacity = 0;
  const bool filtered = call.filter != nullptr;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat.p, &call.tab, filtered ? sizeof(SiteTables) : sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));   // (no filter: the patterns alone, as ever)
  HIP_TRY(ctx, hipMemsetAsync(w->d_totals.p, 0, 2 * nc * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, count(a, filtered, ctx->stream));
  if (n_dev) {
    HIP_TRY(ctx, launch_sites_offsets(w->d_count.p, w->d_off.p, n_blocks, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(n_dev, w->d_off.p + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (totals) HIP_TRY(ctx, hipMemcpyAsync(totals, w->d_totals.p, 2 * nc * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CALITAS_OK;
}

int sites_out_room(calitas_ctx* ctx, SitesWork* w, SitesArgs& a, uint64_t n_dev, const char* no_room) {
  if (int rc = no_room_unless(ctx, w->d_out.grow(n_dev), no_room)) return rc;
  a.out = w->d_out.p; a.out_capacity = n_dev;
  return CALITAS_OK;
}

}  // namespace calitas

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
  // the first pass; a count needs neither the scan nor its total, and both read the contigs' totals in the same wait
  std::vector<uint64_t> totals(2 * nc + 1, 0);
  if (int rc = sites_first_pass(ctx, call, w, a, launch_sites_count, listing ? &totals[2 * nc] : nullptr, totals.data())) return rc;
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
      if ((rc = sites_out_room(ctx, w, a, n_dev, "the site records do not fit the device: list the region in pieces"))) break;
      if ((e = launch_sites_write(a, filter != nullptr, ctx->stream)) != hipSuccess ||
          (e = hipMemcpyAsync(block, w->d_out.p, n_dev * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
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
