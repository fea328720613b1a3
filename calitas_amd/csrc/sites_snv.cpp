// sites_snv.cpp -- calitas_find_allele_sites / calitas_count_allele_sites and their host twins: the checks, the twin (a base-by-base
// walk with one base replaced) that also decides the SNVs beside a U, and the driver of allele_sites.hip's two kernels.
// calitas_find_edit_sites / calitas_count_edit_sites and their host twins: the editor's checks, the twin (a base-by-base walk of the
// background allele on the SNV's strand) that also decides the SNVs beside a U, and the driver of edit_sites.hip's two kernels.
// No reference counterpart.
#include "sites_work.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>

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

// A U is a T to a site and an exception base to the kernels.  The SNVs with one within 63 bases either side -- every base a lane's
// records depend on lies that near its SNV -- are decided on the host, by the twin's walk: their indices (host_snvs) and, when there
// are any, the copy of the SNVs for the device in which each of them says so (marked; otherwise empty) and the kernel leaves it alone.
void snvs_beside_u(calitas_ctx* ctx, const calitas_snv_t* snvs, uint64_t n_snvs, std::vector<Snv>& marked, std::vector<uint64_t>& host_snvs) {
  const PackedRef& ref = ctx->ref;
  const std::vector<Run>& u_runs = u_runs_of(ctx);
  if (u_runs.empty()) return;
  for (uint64_t i = 0; i < n_snvs; i++) {
    const uint64_t g = ref.contigs[(size_t)snvs[i].contig_index].gbase + (uint64_t)snvs[i].position;
    const uint64_t from = g >= 63 ? g - 63 : 0;
    const auto at = std::partition_point(u_runs.begin(), u_runs.end(), [&](const Run& r) { return r.start + r.len <= from; });
    if (at != u_runs.end() && at->start <= g + 63) host_snvs.push_back(i);
  }
  if (host_snvs.empty()) return;
  marked.resize(n_snvs);
  std::memcpy(marked.data(), snvs, n_snvs * sizeof(Snv));
  for (uint64_t i : host_snvs) marked[i].reserved = ALLELE_HOST_DECIDES;
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
  std::vector<Snv> marked;
  std::vector<uint64_t> host_snvs;
  snvs_beside_u(ctx, snvs, n_snvs, marked, host_snvs);

  const char* const no_room = "the SNVs and their records do not fit the device: pass the SNVs in pieces";
  const uint32_t n_blocks = allele_blocks(n_snvs);
  HIP_TRY(ctx, w->d_pat.grow(1));
  if (int rc = no_room_unless(ctx, w->d_snvs.grow(n_snvs), no_room)) return rc;
  if (int rc = no_room_unless(ctx, w->d_al_lanes.grow(n_snvs), no_room)) return rc;
  if (int rc = no_room_unless(ctx, w->d_al_status.grow(n_snvs), no_room)) return rc;
  HIP_TRY(ctx, w->d_al_count.grow((size_t)n_blocks + 1));
  HIP_TRY(ctx, w->d_al_off.grow((size_t)n_blocks + 1));
  HIP_TRY(ctx, w->d_al_by.grow(4));

  AlleleArgs a{};
  a.planes = ctx->d_planes; a.mask = ctx->d_mask; a.contigs = ctx->d_contigs; a.pat = &w->d_pat.p->pat; a.snvs = w->d_snvs.p; a.n = n_snvs;
  a.n_words = ref.total_packed / 32; a.n_contigs = (int32_t)ref.contigs.size();
  a.lane_count = w->d_al_lanes.p; a.status = w->d_al_status.p; a.wg_count = w->d_al_count.p; a.per_kind = w->d_al_by.p; a.wg_offset = w->d_al_off.p;
  a.out = nullptr; a.out_capacity = 0;
  uint64_t total = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat.p, &call.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_snvs.p, marked.empty() ? (const void*)snvs : (const void*)marked.data(), n_snvs * sizeof(Snv), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_al_by.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_allele_count(a, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_al_count.p, w->d_al_off.p, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&total, w->d_al_off.p + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(by, w->d_al_by.p, sizeof(by), hipMemcpyDeviceToHost, ctx->stream));
  if (status) HIP_TRY(ctx, hipMemcpyAsync(status, w->d_al_status.p, n_snvs, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (by[1] + by[2] + by[3] != total) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_allele_sites: the workgroups' sums do not add up to the kinds' (internal error)");

  for (uint64_t i : host_snvs) {
    const uint8_t s = allele_sites_of_snv(ref, call.tab.pat, snvs[i], (uint32_t)i, listing ? &on_host : nullptr, by);
    if (status) status[i] = s;
  }
  *n_sites = by[1] + by[2] + by[3];
  if (per_kind) std::memcpy(per_kind, by, sizeof(by));
  if (!listing) return CALITAS_OK;

  if (int rc = no_room_unless(ctx, w->d_al_out.grow(total), no_room)) return rc;
  calitas_allele_site_t* block = (calitas_allele_site_t*)calitas_out_alloc(std::max<uint64_t>(1, *n_sites) * sizeof(calitas_allele_site_t));
  if (!block) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  if (total) {
    hipError_t e = hipSuccess;
    a.out = w->d_al_out.p; a.out_capacity = total;
    if ((e = launch_allele_write(a, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(block, w->d_al_out.p, total * sizeof(AlleleSite), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
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
  std::vector<Snv> marked;
  std::vector<uint64_t> host_snvs;
  snvs_beside_u(ctx, snvs, n_snvs, marked, host_snvs);

  const char* const no_room = "the SNVs and their records do not fit the device: pass the SNVs in pieces";
  const uint32_t n_blocks = edit_blocks(n_snvs);
  HIP_TRY(ctx, w->d_pat.grow(1));
  if (int rc = no_room_unless(ctx, w->d_ed_snvs.grow(n_snvs), no_room)) return rc;
  if (int rc = no_room_unless(ctx, w->d_ed_lanes.grow(n_snvs), no_room)) return rc;
  if (int rc = no_room_unless(ctx, w->d_ed_status.grow(n_snvs), no_room)) return rc;
  HIP_TRY(ctx, w->d_ed_count.grow((size_t)n_blocks + 1));
  HIP_TRY(ctx, w->d_ed_off.grow((size_t)n_blocks + 1));
  HIP_TRY(ctx, w->d_ed_by.grow(4));

  EditArgs a{};
  a.planes = ctx->d_planes; a.mask = ctx->d_mask; a.contigs = ctx->d_contigs; a.pat = &w->d_pat.p->pat; a.snvs = w->d_ed_snvs.p; a.n = n_snvs;
  a.n_words = ref.total_packed / 32; a.n_contigs = (int32_t)ref.contigs.size();
  a.lane_count = w->d_ed_lanes.p; a.status = w->d_ed_status.p; a.wg_count = w->d_ed_count.p; a.per_bystanders = w->d_ed_by.p; a.wg_offset = w->d_ed_off.p;
  a.out = nullptr; a.out_capacity = 0;
  a.rule = rule;
  uint64_t total = 0;
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat.p, &call.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_ed_snvs.p, marked.empty() ? (const void*)snvs : (const void*)marked.data(), n_snvs * sizeof(Snv), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_ed_by.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_edit_count(a, ctx->stream));
  HIP_TRY(ctx, launch_sites_offsets(w->d_ed_count.p, w->d_ed_off.p, n_blocks, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&total, w->d_ed_off.p + n_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(by, w->d_ed_by.p, sizeof(by), hipMemcpyDeviceToHost, ctx->stream));
  if (status) HIP_TRY(ctx, hipMemcpyAsync(status, w->d_ed_status.p, n_snvs, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (by[0] + by[1] + by[2] + by[3] != total) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_edit_sites: the workgroups' sums do not add up to the bystander bins' (internal error)");

  for (uint64_t i : host_snvs) {
    const uint8_t s = edit_sites_of_snv(ref, call.tab.pat, rule, snvs[i], (uint32_t)i, listing ? &on_host : nullptr, by);
    if (status) status[i] = s;
  }
  *n_sites = by[0] + by[1] + by[2] + by[3];
  if (per_bystanders) std::memcpy(per_bystanders, by, sizeof(by));
  if (!listing) return CALITAS_OK;

  if (int rc = no_room_unless(ctx, w->d_ed_out.grow(total), no_room)) return rc;
  calitas_edit_site_t* block = (calitas_edit_site_t*)calitas_out_alloc(std::max<uint64_t>(1, *n_sites) * sizeof(calitas_edit_site_t));
  if (!block) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  if (total) {
    hipError_t e = hipSuccess;
    a.out = w->d_ed_out.p; a.out_capacity = total;
    if ((e = launch_edit_write(a, ctx->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(block, w->d_ed_out.p, total * sizeof(EditSite), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
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
