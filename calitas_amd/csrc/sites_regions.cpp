// sites_regions.cpp -- calitas_find_sites_regions / calitas_count_sites_regions and their host twins: the checks, the presence table,
// the host twin (every record classed through the host's flattened set) and the driver of site_regions.hip's kernels around the site
// kernel's two passes, with the records beside a U classed on the host.  No reference counterpart.
#include "sites_work.hpp"
#include "site_regions.hpp"
#include "tuning.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

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
      HIP_TRY(ctx, w->d_presence.grow(table->size()));            // (an empty table: nothing to hold, nothing to copy)
      w->presence_regions = 0;
      if (!table->empty()) HIP_TRY(ctx, hipMemcpy(w->d_presence.p, table->data(), table->size(), hipMemcpyHostToDevice));
      w->presence_regions = ctx->regions.serial; w->presence_ref = ctx->ref_serial;
    }
    a.presence = w->d_presence.p; a.class_mask = call.mask;
  }
  uint64_t n_dev = 0;
  if (int rc = sites_first_pass(ctx, call.site, w, a, skip ? launch_sites_regions_count : launch_sites_count, &n_dev)) return rc;
  const char* const no_room = "the site records and their classes do not fit the device: list the region in pieces";
  if (n_dev / SITE_CLASS_THREADS >= 0x7FFFFFFFull) return calitas_fail(ctx, CALITAS_ENOMEM, no_room);

  // the records stay in d_out: a lane per record classes its extent, the workgroups' kept counts are scanned
  uint64_t n_kept = 0;
  const uint32_t cls_blocks = site_class_blocks(n_dev);
  if (n_dev) {
    if (int rc = sites_out_room(ctx, w, a, n_dev, no_room)) return rc;
    if (int rc = no_room_unless(ctx, w->d_reg_cls.grow(n_dev), no_room)) return rc;
    HIP_TRY(ctx, w->d_reg_count.grow((size_t)cls_blocks + 1));
    HIP_TRY(ctx, w->d_reg_off.grow((size_t)cls_blocks + 1));
    HIP_TRY(ctx, w->d_reg_cells.grow(SITE_CLASS_CELLS));
    SiteClassArgs s{};
    s.recs = w->d_out.p; s.contigs = ctx->d_contigs;
    s.rv = RegionsView{ctx->d_region_seg, ctx->d_region_coarse, ctx->d_region_contig, ctx->regions.n_classes};
    s.cls = w->d_reg_cls.p; s.wg_kept = w->d_reg_count.p; s.cells = w->d_reg_cells.p;
    s.n = n_dev; s.n_contigs = (int32_t)nc; s.ext_from = call.from; s.ext_to = call.to; s.class_mask = call.mask;
    HIP_TRY(ctx, skip ? launch_sites_regions_write(a, filter != nullptr, ctx->stream) : launch_sites_write(a, filter != nullptr, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w->d_reg_cells.p, 0, SITE_CLASS_CELLS * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, launch_site_class(s, ctx->stream));
    HIP_TRY(ctx, launch_sites_offsets(w->d_reg_count.p, w->d_reg_off.p, cls_blocks, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&n_kept, w->d_reg_off.p + cls_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(cells, w->d_reg_cells.p, sizeof(cells), hipMemcpyDeviceToHost, ctx->stream));
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

  if (int rc = no_room_unless(ctx, w->d_reg_out.grow(n_kept), no_room)) return rc;
  if (int rc = no_room_unless(ctx, w->d_reg_out_cls.grow(n_kept), no_room)) return rc;
  if (n_kept) HIP_TRY(ctx, launch_site_class_compact(w->d_out.p, w->d_reg_cls.p, n_dev, w->d_reg_off.p, w->d_reg_out.p, w->d_reg_out_cls.p, n_kept, ctx->stream));
  calitas_site_t* block = nullptr;
  uint8_t* block_cls = nullptr;
  if (int rc = regions_blocks_alloc(ctx, n_kept + n_in, &block, &block_cls)) return rc;
  int rc = CALITAS_OK;
  do {   // (one exit that releases the blocks)
    hipError_t e = hipSuccess;
    if ((n_kept && ((e = hipMemcpyAsync(block, w->d_reg_out.p, n_kept * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
                    (e = hipMemcpyAsync(block_cls, w->d_reg_out_cls.p, n_kept, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)) ||
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
