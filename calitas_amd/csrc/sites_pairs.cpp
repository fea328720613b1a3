// sites_pairs.cpp -- calitas_find_site_pairs / calitas_count_site_pairs and their host twins: the checks, the one walk over a sorted
// listing (pair_walk) that the twins and the listings beside a U share, and the driver of site_pairs.hip's kernels behind the site
// kernel's two passes.  No reference counterpart.
#include "sites_work.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

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
  uint64_t n_dev = 0;
  if (int rc = sites_first_pass(ctx, call.site, w, a, launch_sites_count, &n_dev)) return rc;
  *n_sites = n_dev;
  if (int rc = pairs_too_many_sites(ctx, n_dev)) return rc;
  const char* const no_room = "the site records and their pairs do not fit the device: pair the region in pieces";

  // the records stay in d_out, in listing order: a lane per record counts its partners, the workgroups' sums are scanned
  uint64_t total = 0;
  const uint32_t pair_blocks = site_pair_blocks(n_dev);
  SitePairArgs p{};
  if (n_dev) {
    if (int rc = sites_out_room(ctx, w, a, n_dev, no_room)) return rc;
    if (int rc = no_room_unless(ctx, w->d_pair_lanes.grow(n_dev), no_room)) return rc;
    HIP_TRY(ctx, w->d_pair_count.grow((size_t)pair_blocks + 1));
    HIP_TRY(ctx, w->d_pair_off.grow((size_t)pair_blocks + 1));
    HIP_TRY(ctx, w->d_pair_by.grow(4));
    p.recs = w->d_out.p; p.n = n_dev; p.lane_count = w->d_pair_lanes.p; p.wg_count = w->d_pair_count.p; p.per_orientation = w->d_pair_by.p;
    p.wg_offset = w->d_pair_off.p; p.out = nullptr; p.out_capacity = 0; p.rule = call.rule;
    HIP_TRY(ctx, launch_sites_write(a, filter != nullptr, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w->d_pair_by.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, launch_site_pairs_count(p, ctx->stream));
    HIP_TRY(ctx, launch_sites_offsets(w->d_pair_count.p, w->d_pair_off.p, pair_blocks, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&total, w->d_pair_off.p + pair_blocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(by, w->d_pair_by.p, sizeof(by), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (by[0] + by[1] + by[2] + by[3] != total) return calitas_fail(ctx, CALITAS_EHIP, "calitas_find_site_pairs: the workgroups' sums do not add up to the orientations' (internal error)");
  }
  *n_pairs = total;
  if (per_orientation) std::memcpy(per_orientation, by, sizeof(by));
  if (!listing) return CALITAS_OK;

  if (int rc = no_room_unless(ctx, w->d_pair_out.grow(total), no_room)) return rc;
  calitas_site_t* block = (calitas_site_t*)calitas_out_alloc(std::max<uint64_t>(1, n_dev) * sizeof(calitas_site_t));
  calitas_site_pair_t* block_pairs = (calitas_site_pair_t*)calitas_out_alloc(std::max<uint64_t>(1, total) * sizeof(calitas_site_pair_t));
  int rc = CALITAS_OK;
  do {   // (one exit that releases the blocks)
    if (!block || !block_pairs) { rc = calitas_fail(ctx, CALITAS_EINVAL, "out of memory"); break; }
    hipError_t e = hipSuccess;
    p.out = w->d_pair_out.p; p.out_capacity = total;
    if ((total && ((e = launch_site_pairs_write(p, ctx->stream)) != hipSuccess ||
                   (e = hipMemcpyAsync(block_pairs, w->d_pair_out.p, total * sizeof(SitePair), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)) ||
        (n_dev && (e = hipMemcpyAsync(block, w->d_out.p, n_dev * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
      rc = calitas_fail(ctx, CALITAS_EHIP, std::string("calitas_find_site_pairs: ") + hipGetErrorString(e));
  } while (0);
  if (rc) { calitas_free(block); calitas_free(block_pairs); return rc; }
  *sites = block; *pairs = block_pairs;
  return CALITAS_OK;
}
