// sites_work.hpp -- private: what the guide-site units (sites_host.cpp, sites_copies.cpp, sites_scored.cpp, sites_regions.cpp,
// sites_pairs.cpp, sites_snv.cpp) share: the device scratch of a context and its buffer type, a call's plan, the sites beside a U, the
// launch of a region and the site kernel's first pass.  sites.hpp is what api.cpp sees.
#pragma once
#include "sites.hpp"

namespace calitas {

// A device buffer of the scratch, grown on demand and freed with the SitesWork it is a member of (sites_destroy deletes that).  It
// holds exactly what its largest call asked for, no slack: a context's footprint is the sum of those.  p and cap are both set or both
// clear, also after a failed grow.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;                    // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t grow(size_t need) {
    if (need <= cap) return hipSuccess;
    release();
    const hipError_t e = hipMalloc((void**)&p, need * sizeof(T));
    if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
    cap = need;
    return hipSuccess;
  }
  void release() { (void)hipFree(p); p = nullptr; cap = 0; }
};

// the buffers of a scored listing (sites_scored.cpp): a score per record of d_out, the workgroups' kept counts and their scan, and the
// kept records and scores in order
template <typename S>
struct ScoredBufs {
  DevBuf<S> scores;
  DevBuf<uint32_t> count;
  DevBuf<uint64_t> off;
  DevBuf<SiteRecord> out;
  DevBuf<S> out_scores;
};

struct SitesWork {
  DevBuf<SiteTables> d_pat;          // the patterns and, behind them, the filter of the call in flight
  DevBuf<uint32_t> d_count;
  DevBuf<uint64_t> d_off;
  DevBuf<unsigned long long> d_totals;
  DevBuf<SiteRecord> d_out;
  // calitas_count_copies: the table of query keys (slots) and the distinct keys' counters (+ 1: the error flag)
  DevBuf<uint64_t> d_keys;
  DevBuf<uint32_t> d_key_index;
  DevBuf<unsigned long long> d_key_counts;
  // calitas_count_near: the pieces' bucket tables and member lists (its counters are d_key_counts)
  DevBuf<uint32_t> d_near_offsets;
  DevBuf<uint4> d_near_members;
  // calitas_list_near: the stretches' first records, {cursor, length} per distinct key (+ 1: the error flag), the keys whose stretches
  // are put in order, and the records as the pass stored them (list_in) and in position order (list_out)
  DevBuf<uint64_t> d_list_base;
  DevBuf<uint32_t> d_list_cursors;
  DevBuf<uint32_t> d_list_order;
  DevBuf<NearHit> d_list_in;
  DevBuf<NearHit> d_list_out;
  // calitas_find_sites_scored: the model's folded table and the listing's buffers
  DevBuf<int32_t> d_act_table;
  ScoredBufs<int32_t> act;
  // calitas_find_sites_regions: the device copy of the context's presence table (one byte per segment of the packed space), a class byte
  // per record of d_out, the workgroups' kept counts and their scan, the 16 (class, strand) counters, and the kept records and classes
  // in order
  DevBuf<uint8_t> d_presence;
  uint64_t presence_regions = 0, presence_ref = ~0ull;   // the set and the reference d_presence was made from
  DevBuf<uint8_t> d_reg_cls;
  DevBuf<uint32_t> d_reg_count;
  DevBuf<uint64_t> d_reg_off;
  DevBuf<unsigned long long> d_reg_cells;
  DevBuf<SiteRecord> d_reg_out;
  DevBuf<uint8_t> d_reg_out_cls;
  // calitas_find_site_pairs: a count per record of d_out, the workgroups' sums and their scan, the four per-orientation counters, and
  // the pairs in order
  DevBuf<uint32_t> d_pair_lanes;
  DevBuf<uint32_t> d_pair_count;
  DevBuf<uint64_t> d_pair_off;
  DevBuf<unsigned long long> d_pair_by;
  DevBuf<SitePair> d_pair_out;
  // calitas_find_allele_sites: the SNVs, a count and a status byte per SNV, the workgroups' sums and their scan, the per-kind counters,
  // and the records in order
  DevBuf<Snv> d_snvs;
  DevBuf<uint32_t> d_al_lanes;
  DevBuf<uint8_t> d_al_status;
  DevBuf<uint32_t> d_al_count;
  DevBuf<uint64_t> d_al_off;
  DevBuf<unsigned long long> d_al_by;
  DevBuf<AlleleSite> d_al_out;
  // calitas_find_sites_microhomology: the listing's buffers
  ScoredBufs<MhScore> mh;
  // calitas_find_edit_sites: the SNVs, a count and a status byte per SNV, the workgroups' sums and their scan, the four bystander
  // counters, and the records in order
  DevBuf<Snv> d_ed_snvs;
  DevBuf<uint32_t> d_ed_lanes;
  DevBuf<uint8_t> d_ed_status;
  DevBuf<uint32_t> d_ed_count;
  DevBuf<uint64_t> d_ed_off;
  DevBuf<unsigned long long> d_ed_by;
  DevBuf<EditSite> d_ed_out;
  // the U / u runs of the resident reference (a U is a plain base to a site and an exception base to the kernels): u_runs_of
  uint64_t u_serial = ~0ull;
  std::vector<Run> u_runs;
};

// a per-record or per-SNV buffer that does not grow: the driver's own "... do not fit the device: ... in pieces"
inline int no_room_unless(calitas_ctx* c, hipError_t grown, const char* no_room) {
  return grown == hipSuccess ? CALITAS_OK : calitas_fail(c, CALITAS_ENOMEM, no_room);
}

// 2-bit code of a plain base (A C G T in either case, U), -1 for everything else; *u: it is a U (kept as an exception run)
inline int plain_code(const PackedRef& ref, uint64_t g, bool* u) {
  if ((ref.mask[g >> 5] >> (g & 31)) & 1u) {
    const Run* r = ref.run_at(g);
    if (r && (r->ch == 'U' || r->ch == 'u')) { *u = true; return 3; }
    return -1;
  }
  return (int)((ref.codes[g >> 4] >> ((g & 15) * 2)) & 3u);
}

// the record of the site at protospacer start p on strand st that PAM k matched
inline calitas_site_t site_record(const SitePatterns& pat, int contig, int64_t p, int st, int k) {
  const SitePattern& sp = pat.p[k][st];
  calitas_site_t s;
  s.contig_index = contig; s.protospacer_start = (int32_t)p; s.pam_start = pat.pamless ? -1 : (int32_t)(p + sp.pam_off);
  s.strand = st ? '-' : '+'; s.pam_index = pat.pamless ? (int8_t)-1 : (int8_t)k; s.pam_length = (uint8_t)sp.pam_len;
  s.protospacer_length = (uint8_t)pat.proto_len;
  return s;
}

struct SiteCall {
  SiteTables tab;                    // the patterns; the filter as the kernel reads it
  const calitas_site_filter_t* filter = nullptr;
  int c_first = 0, c_last = 0;       // contigs [c_first, c_last]
  bool pam5 = false;                 // the pattern has PAMs and they stand in front of the protospacer
};

// the first half of plan_sites: the pattern and the filter
int plan_site_pattern(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, SiteCall& call);
// arguments every entry point shares: the pattern, the filter, the contigs, the region
int plan_sites(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index, uint64_t start, uint64_t end,
               SiteCall& call);

inline bool site_less(const calitas_site_t& a, const calitas_site_t& b) {
  if (a.contig_index != b.contig_index) return a.contig_index < b.contig_index;
  if (a.protospacer_start != b.protospacer_start) return a.protospacer_start < b.protospacer_start;
  return a.strand == '+' && b.strand == '-';
}

// the U / u runs of the resident reference in position order, listed again when the reference is another one (makes the scratch)
const std::vector<Run>& u_runs_of(calitas_ctx* c);
// The sites whose footprint holds a U: the kernel sees an exception base there.  Found on the host around every U run of the region
// (with_u), together with the records the kernel has at those positions in their place (kernel_has).
void sites_with_u(calitas_ctx* c, const SiteCall& call, uint64_t start, uint64_t end, std::vector<calitas_site_t>& with_u,
                  std::vector<calitas_site_t>& kernel_has);
// The launch of a region: the words it touches, from a workgroup boundary on (contigs start on tile boundaries, tiles are whole
// workgroups), and the arguments every kernel of sites.hip shares.
int site_launch(calitas_ctx* ctx, const SiteCall& call, int32_t chrom_index, uint64_t start, uint64_t end, SitesWork* w, SitesArgs& a);

// The site kernel's first pass, queued on the context's stream in this order: the patterns up (the filter behind them only when the
// call has one), the contigs' totals cleared, `count` (launch_sites_count, or the regions driver's launch_sites_regions_count with
// a.presence and a.class_mask set), with n_dev the scan of the workgroups' counts and the copy of its total, with totals the copy of
// the 2 n_contigs totals, one wait.  d_count / d_off (n_segs + 1) and d_totals grow first; a.out stays null.
typedef hipError_t (*SitesCountLaunch)(const SitesArgs& a, bool filtered, hipStream_t stream);
int sites_first_pass(calitas_ctx* ctx, const SiteCall& call, SitesWork* w, SitesArgs& a, SitesCountLaunch count, uint64_t* n_dev, uint64_t* totals = nullptr);
// room for the second pass's n_dev records in d_out, or the driver's no_room; a.out and a.out_capacity set
int sites_out_room(calitas_ctx* ctx, SitesWork* w, SitesArgs& a, uint64_t n_dev, const char* no_room);

}  // namespace calitas
