// site_regions.hpp -- launch interface of site_regions.hip (calitas_find_sites_regions / calitas_count_sites_regions; device pointers
// only) and the one rule both implementations class a site by.
#pragma once
#include "kernels.hpp"
#include "regions.hpp"

namespace calitas {

// What the skip test of the regions passes rests on: a segment of sites_kernel is exactly one bucket of the regions' coarse index,
// provided contigs start on segment boundaries (they start on tile boundaries, and the host checks that tiles are whole segments).
static_assert(REGION_COARSE == 32u * SITES_BLOCK_WORDS, "a segment of the site pass is one coarse bucket of its contig");
static_assert(SITE_MAX_FOOT >= MAX_L, "the presence table's halo covers a protospacer that starts on a segment's last base");

// The class of a site (calitas_hip.h, calitas_site_regions_t): guide positions [from, to) of the protospacer of L bases at forward
// position p are the forward bases [p + from, p + to) on '+' and [p + L - to, p + L - from) on '-'; their class is region_class's.
CAL_HD inline uint32_t site_region_class(const RegionsView& rv, uint32_t contig, int64_t p, int L, bool minus, int from, int to, uint64_t len) {
  const int64_t s = minus ? p + L - to : p + from, e = minus ? p + L - from : p + to;
  return region_class(rv, contig, s, e, len);
}

constexpr int SITE_CLASS_THREADS = 256;
constexpr uint32_t SITE_CLASS_KEEP = 0x80u;                 // the keep flag beside the class in site_class_kernel's byte
constexpr uint32_t SITE_CLASS_CELLS = 2 * CALITAS_REGION_CLASSES_MAX;
struct SiteClassArgs {
  const SiteRecord* recs;            // n records, as launch_sites_write left them
  const ContigInfo* contigs;
  RegionsView rv;                    // the context's device copy of the flattened set
  uint8_t* cls;                      // n: the record's class, | SITE_CLASS_KEEP when its bit is in class_mask
  uint32_t* wg_kept;                 // per workgroup: records kept
  unsigned long long* cells;         // SITE_CLASS_CELLS, 0 at launch: kept records per (class, strand), '+' first
  uint64_t n;
  int32_t n_contigs;
  int32_t ext_from, ext_to;
  uint32_t class_mask;
};
inline uint32_t site_class_blocks(uint64_t n) { return (uint32_t)((n + SITE_CLASS_THREADS - 1) / SITE_CLASS_THREADS); }
// the find passes with the presence test (SitesArgs::presence, class_mask set)
hipError_t launch_sites_regions_count(const SitesArgs& a, bool filtered, hipStream_t stream);
hipError_t launch_sites_regions_write(const SitesArgs& a, bool filtered, hipStream_t stream);
hipError_t launch_site_class(const SiteClassArgs& a, hipStream_t stream);
// The kept records and their classes, in order: record i of workgroup g goes to wg_offset[g] + its rank among g's kept records.
hipError_t launch_site_class_compact(const SiteRecord* recs, const uint8_t* cls, uint64_t n, const uint64_t* wg_offset, SiteRecord* out_recs,
                                     uint8_t* out_cls, uint64_t out_capacity, hipStream_t stream);

}  // namespace calitas
