// sites.hpp -- private: guide-site enumeration as api.cpp sees it (sites_host.cpp, sites_copies.cpp, sites_scored.cpp, sites_regions.cpp,
// sites_pairs.cpp, sites_snv.cpp; what those share: sites_work.hpp; kernels in sites.hip and the feature units, launch interface in kernels.hpp).
#pragma once
#include <string>
#include <vector>

#include "ctx.hpp"

namespace calitas {

// The per-(PAM, strand) patterns of a guide read as a pattern; returns an error text or "".
std::string make_site_patterns(const GuideHost& gh, SitePatterns& out);
// A site filter checked against a protospacer of L bases and turned into what the kernel reads; returns an error text that names the
// field, or "".
std::string make_site_filter(const calitas_site_filter_t& f, int L, SiteFilterDev& out);
// Base by base: does the protospacer of L bases at [protospacer_start, protospacer_start + L) of the contig, read on the strand
// (0 '+', 1 '-': the reverse complement), upper case and a U as T, pass the filter?  The protospacer alone: the verdict is the same for
// every PAM that matches there.  Every base must be a plain one (any site's is).
bool site_passes(const PackedRef& ref, int contig, int64_t protospacer_start, int L, int strand, const calitas_site_filter_t& filter);
inline uint64_t region_end(uint64_t len, uint64_t end) { return (end == 0 || end > len) ? len : end; }
// Base by base: the sites of one contig whose protospacer starts in [p_lo, p_hi), region [r_start, r_end), in output order, appended.
// kernel_has != nullptr: none but those whose footprint holds a U, and appended to *kernel_has the record sites_kernel -- to which a U
// is an exception base -- has at such a position instead (a later, shorter PAM's whose own footprint is clean), if it has one.
// filter != nullptr: none but the sites that pass it, in `out` and in *kernel_has alike (the kernel filters what it writes).
void host_sites(const PackedRef& ref, const SitePatterns& pat, const calitas_site_filter_t* filter, int contig, int64_t p_lo, int64_t p_hi,
                int64_t r_start, int64_t r_end, std::vector<calitas_site_t>& out, std::vector<calitas_site_t>* kernel_has);
// The presence table of the context's region set (calitas_find_sites_regions), made when the set or the reference is another one than
// the table's; returns an error text or "".  Needs no device.
std::string site_presence(calitas_ctx* c, const std::vector<uint8_t>** out);
struct SitesWork;                 // device scratch of a context, kept between calls (sites_work.hpp)
void sites_destroy(SitesWork* w);

}  // namespace calitas

// filter == nullptr: every site
int calitas_find_sites_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index,
                                 uint64_t start, uint64_t end, calitas_site_t** sites, uint64_t* n_sites);
// listing: both passes and the records; otherwise the first pass alone
int calitas_find_sites_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index, uint64_t start,
                            uint64_t end, bool listing, calitas_site_t** sites, uint64_t* per_contig_strand, uint64_t* n_sites);
// copies[i]: the sites of the unfiltered count whose key -- the PAM-proximal key_length bases of the protospacer (0: all of it) -- is query i
int calitas_count_copies_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start,
                                   uint64_t end, const char* queries, uint64_t n_queries, uint64_t* copies);
int calitas_count_copies_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start, uint64_t end,
                              const char* queries, uint64_t n_queries, uint64_t* copies);
// near[i (M + 1) + d]: the sites of the unfiltered count whose key differs from query i at exactly d of its positions, d = 0 .. M = max_mismatches
int calitas_count_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index,
                                 uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near);
int calitas_count_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index, uint64_t start,
                            uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near);
// near: as calitas_count_near with the whole protospacer as the key; scores[i]: sum and maximum of the model's scores of query i's sites at d = 1 .. M
int calitas_score_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                                 int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near,
                                 calitas_near_score_t* scores);
int calitas_score_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                            uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near, calitas_near_score_t* scores);
// near: as above; hits[offsets[i] .. offsets[i + 1]): a record per site of query i at d = 0 .. M in position order, none where the row of near sums
// to more than limit; model may be null (every score 2^32)
int calitas_list_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                                int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near,
                                uint64_t* offsets, calitas_near_hit_t** hits, uint64_t* n_hits);
int calitas_list_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                           uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near, uint64_t* offsets,
                           calitas_near_hit_t** hits, uint64_t* n_hits);
// the records of calitas_find_sites_filtered whose activity score under the model is >= min_score, and the scores; CALITAS_ACTIVITY_NONE keeps all
int calitas_find_sites_scored_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                        const calitas_activity_model_t* model, int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end,
                                        calitas_site_t** sites, int32_t** scores, uint64_t* n_sites);
int calitas_find_sites_scored_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_activity_model_t* model,
                                   int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, int32_t** scores,
                                   uint64_t* n_sites);
// the records of calitas_find_sites_filtered whose class under opt has its bit in opt->class_mask, and the classes; listing false: the
// numbers alone (per_class_strand may be null)
int calitas_find_sites_regions_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                         const calitas_site_regions_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, bool listing,
                                         calitas_site_t** sites, uint8_t** classes, uint64_t* per_class_strand, uint64_t* n_sites);
int calitas_find_sites_regions_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_regions_t* opt,
                                    int32_t chrom_index, uint64_t start, uint64_t end, bool listing, calitas_site_t** sites, uint8_t** classes,
                                    uint64_t* per_class_strand, uint64_t* n_sites);
// the listing of calitas_find_sites_filtered and its pairs under opt; listing false: the numbers alone (per_orientation may be null)
int calitas_find_site_pairs_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                      const calitas_site_pairs_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, bool listing,
                                      calitas_site_t** sites, uint64_t* n_sites, calitas_site_pair_t** pairs, uint64_t* n_pairs,
                                      uint64_t* per_orientation);
int calitas_find_site_pairs_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_pairs_t* opt,
                                 int32_t chrom_index, uint64_t start, uint64_t end, bool listing, calitas_site_t** sites, uint64_t* n_sites,
                                 calitas_site_pair_t** pairs, uint64_t* n_pairs, uint64_t* per_orientation);
// the records of the SNVs in input order; listing false: the numbers alone (per_kind and status may be null)
int calitas_find_allele_sites_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, bool listing,
                                        calitas_allele_site_t** sites, uint64_t* per_kind, uint64_t* n_sites, uint8_t* status);
int calitas_find_allele_sites_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, bool listing,
                                   calitas_allele_site_t** sites, uint64_t* per_kind, uint64_t* n_sites, uint8_t* status);
// the records of the SNVs in input order; listing false: the numbers alone (per_bystanders and status may be null)
int calitas_find_edit_sites_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs,
                                      uint64_t n_snvs, bool listing, calitas_edit_site_t** sites, uint64_t* per_bystanders, uint64_t* n_sites, uint8_t* status);
int calitas_find_edit_sites_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs, uint64_t n_snvs,
                                 bool listing, calitas_edit_site_t** sites, uint64_t* per_bystanders, uint64_t* n_sites, uint8_t* status);
// the records of calitas_find_sites_filtered kept under permille (0: all of them) and their microhomology scores under the model
int calitas_find_sites_microhomology_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                               const calitas_mh_model_t* model, int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end,
                                               calitas_site_t** sites, calitas_mh_score_t** scores, uint64_t* n_sites);
int calitas_find_sites_microhomology_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_mh_model_t* model,
                                          int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                          calitas_mh_score_t** scores, uint64_t* n_sites);
