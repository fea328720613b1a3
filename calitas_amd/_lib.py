"""ctypes binding of libcalitas_hip.so (C ABI: include/calitas_hip.h).

The library is built in-tree by `make -C calitas_amd/csrc` (see __graft_entry__.build).  There is no Python or CPU
fallback: if the shared library is missing, importing this module raises; if no GPU is present, creating a device
context raises CalitasError(ENODEV).
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# CALITAS_LIB_PATH: another build of the same library -- tools/sanitize.sh points it at the host-side sanitizer builds
# (make SAN=address|thread).  Still a native library: there is no Python or CPU implementation to fall back to.
LIB_PATH = os.environ.get("CALITAS_LIB_PATH") or os.path.join(HERE, "libcalitas_hip.so")

MAX_OPS = 128
OK, EINVAL, ENODEV, EHIP, EIO, ESTATE, ENOMEM = 0, 1, 2, 3, 4, 5, 6


class CalitasError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("calitas error %d: %s" % (code, message))
        self.code = code


class GuideT(ctypes.Structure):
    _fields_ = [("protospacer", ctypes.c_char_p), ("n_pams", ctypes.c_int32), ("pams", ctypes.POINTER(ctypes.c_char_p)),
                ("pam_is_5prime", ctypes.c_int32), ("cli_length", ctypes.c_int32)]


class ParamsT(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "window_size", "max_guide_diffs", "max_pam_mismatches", "max_gaps_between_guide_and_pam", "max_total_diffs", "max_overlap",
        "guide_mismatch_net_cost", "pam_mismatch_net_cost", "genome_gap_net_cost", "guide_gap_net_cost", "chrom_index",
        "eqx_by_score", "max_variants", "first_window", "n_windows")]


class AlnT(ctypes.Structure):
    _fields_ = [("guide_index", ctypes.c_int32), ("contig_index", ctypes.c_int32), ("window_start", ctypes.c_int32),
                ("start_offset", ctypes.c_int32), ("end_offset", ctypes.c_int32), ("guide_start_offset", ctypes.c_int32),
                ("guide_end_offset", ctypes.c_int32), ("score", ctypes.c_int32), ("strand", ctypes.c_int8),
                ("pam_index", ctypes.c_int8), ("n_ops", ctypes.c_int16), ("ops", ctypes.c_uint8 * MAX_OPS)]


class ExtHitT(ctypes.Structure):
    _fields_ = [("contig_index", ctypes.c_int32), ("coordinate_start", ctypes.c_int32), ("end", ctypes.c_int32), ("score", ctypes.c_int32),
                ("strand", ctypes.c_int8), ("variant_description", ctypes.c_char_p), ("row", ctypes.c_char_p)]


class TimingT(ctypes.Structure):
    _fields_ = [("scan_kernel_ms", ctypes.c_double), ("align_kernel_ms", ctypes.c_double), ("gpu_total_ms", ctypes.c_double),
                ("host_post_ms", ctypes.c_double), ("bases_scanned", ctypes.c_uint64), ("packed_bytes", ctypes.c_uint64),
                ("scan_records", ctypes.c_uint64), ("candidate_columns", ctypes.c_uint64), ("raw_alignments", ctypes.c_uint64),
                ("accepted_alignments", ctypes.c_uint64), ("retries", ctypes.c_uint32), ("lanes", ctypes.c_uint32),
                ("hits_kernel_ms", ctypes.c_double), ("hits_copy_ms", ctypes.c_double), ("hit_rows", ctypes.c_uint64),
                ("hits_bytes", ctypes.c_uint64), ("contig_passes", ctypes.c_uint32), ("binned_lanes", ctypes.c_uint32),
                ("owned_general_lanes", ctypes.c_uint32), ("scan_variant", ctypes.c_uint32)]


class SiteT(ctypes.Structure):
    _fields_ = [("contig_index", ctypes.c_int32), ("protospacer_start", ctypes.c_int32), ("pam_start", ctypes.c_int32),
                ("strand", ctypes.c_int8), ("pam_index", ctypes.c_int8), ("pam_length", ctypes.c_uint8), ("protospacer_length", ctypes.c_uint8)]


class CountsT(ctypes.Structure):
    _fields_ = [("n_mm", ctypes.c_uint32), ("n_gaps", ctypes.c_uint32), ("n_pam", ctypes.c_uint32), ("rows", ctypes.c_uint64),
                ("counts", ctypes.POINTER(ctypes.c_uint64))]


class ScoreModelT(ctypes.Structure):
    _fields_ = [("protospacer_length", ctypes.c_int32), ("gap", ctypes.c_uint32), ("pam_mismatch", ctypes.c_uint32),
                ("mismatch", ctypes.POINTER(ctypes.c_uint32))]


class ScoresT(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_uint64), ("perfect", ctypes.c_uint64), ("sum_q32", ctypes.c_uint64), ("max_q32", ctypes.c_uint64),
                ("table", CountsT)]


class TopHitT(ctypes.Structure):
    _fields_ = [("score_q32", ctypes.c_uint64), ("contig_index", ctypes.c_int32), ("coordinate_start", ctypes.c_int32),
                ("coordinate_end", ctypes.c_int32), ("strand", ctypes.c_int8), ("guide_mm", ctypes.c_uint8), ("guide_gaps", ctypes.c_uint8),
                ("pam_mm", ctypes.c_uint8)]


class TopT(ctypes.Structure):
    _fields_ = [("scores", ScoresT), ("k", ctypes.c_uint32), ("n", ctypes.c_uint32), ("hits", ctypes.POINTER(TopHitT))]


class SiteFilterT(ctypes.Structure):
    _fields_ = [("gc_min", ctypes.c_uint8), ("gc_max", ctypes.c_uint8), ("max_run", ctypes.c_uint8 * 4), ("n_motifs", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8), ("motifs", (ctypes.c_char * 16) * 8)]


class RegionT(ctypes.Structure):
    _fields_ = [("contig_index", ctypes.c_int32), ("start", ctypes.c_int32), ("end", ctypes.c_int32), ("cls", ctypes.c_uint32)]


class RegionsT(ctypes.Structure):
    _fields_ = [("top", TopT), ("hit_class", ctypes.POINTER(ctypes.c_uint8)), ("n_classes", ctypes.c_uint32), ("list_mask", ctypes.c_uint32),
                ("by_class", ctypes.POINTER(ScoresT))]


class NearHitT(ctypes.Structure):
    _fields_ = [("score_q32", ctypes.c_uint64), ("contig_index", ctypes.c_int32), ("protospacer_start", ctypes.c_int32), ("target_lo", ctypes.c_uint32),
                ("target_hi", ctypes.c_uint32), ("diff_mask", ctypes.c_uint32), ("strand", ctypes.c_int8), ("pam_index", ctypes.c_int8),
                ("mismatches", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class ActivityModelT(ctypes.Structure):
    _fields_ = [("protospacer_length", ctypes.c_int32), ("up", ctypes.c_int32), ("down", ctypes.c_int32), ("link", ctypes.c_int32),
                ("intercept", ctypes.c_int32), ("single", ctypes.POINTER(ctypes.c_int32)), ("pair", ctypes.POINTER(ctypes.c_int32)),
                ("gc", ctypes.POINTER(ctypes.c_int32))]


class SiteRegionsT(ctypes.Structure):
    _fields_ = [("class_mask", ctypes.c_uint32), ("ext_from", ctypes.c_uint8), ("ext_to", ctypes.c_uint8), ("reserved", ctypes.c_uint16)]


class SitePairsT(ctypes.Structure):
    _fields_ = [("min_distance", ctypes.c_int32), ("max_distance", ctypes.c_int32), ("cut_offset", ctypes.c_uint8), ("orientations", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 2)]


class SitePairT(ctypes.Structure):
    _fields_ = [("left", ctypes.c_uint32), ("right", ctypes.c_uint32), ("distance", ctypes.c_int32), ("orientation", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 3)]


class SnvT(ctypes.Structure):
    _fields_ = [("contig_index", ctypes.c_int32), ("position", ctypes.c_int32), ("ref", ctypes.c_char), ("alt", ctypes.c_char), ("reserved", ctypes.c_uint16)]


class AlleleSiteT(ctypes.Structure):
    _fields_ = [("site", SiteT), ("snv_index", ctypes.c_uint32), ("kind", ctypes.c_uint8), ("other_pam_index", ctypes.c_int8), ("guide_offset", ctypes.c_int8),
                ("reserved", ctypes.c_uint8), ("guide_lo", ctypes.c_uint32), ("guide_hi", ctypes.c_uint32)]


class BaseEditT(ctypes.Structure):
    _fields_ = [("from_base", ctypes.c_char), ("to_base", ctypes.c_char), ("window_from", ctypes.c_uint8), ("window_to", ctypes.c_uint8), ("context", ctypes.c_char),
                ("correct", ctypes.c_uint8), ("max_bystanders", ctypes.c_uint8), ("reserved", ctypes.c_uint8)]


class EditSiteT(ctypes.Structure):
    _fields_ = [("site", SiteT), ("snv_index", ctypes.c_uint32), ("editable", ctypes.c_uint32), ("guide_lo", ctypes.c_uint32), ("guide_hi", ctypes.c_uint32)]


class MhModelT(ctypes.Structure):
    _fields_ = [("left", ctypes.c_int32), ("right", ctypes.c_int32), ("cut_offset", ctypes.c_int32), ("min_length", ctypes.c_int32),
                ("weight", ctypes.POINTER(ctypes.c_uint32))]


class MhScoreT(ctypes.Structure):
    _fields_ = [("total_q16", ctypes.c_uint32), ("out_of_frame_q16", ctypes.c_uint32)]


assert ctypes.sizeof(SnvT) == 12 and ctypes.sizeof(AlleleSiteT) == 32 and ctypes.sizeof(MhScoreT) == 8
assert ctypes.sizeof(BaseEditT) == 8 and ctypes.sizeof(EditSiteT) == 32
EDIT_NO_BOUND = 255
MH_NONE = 0xFFFFFFFF
MH_MAX_SIDE = 32
MH_MAX_WEIGHT = 1 << 16
PAIR_MAX_DISTANCE = 65535
assert ctypes.sizeof(SitePairsT) == 12 and ctypes.sizeof(SitePairT) == 16
TOP_MAX = 256
NEAR_LIST_MAX = 4096
ACTIVITY_NONE = -(1 << 31)
ACTIVITY_MAX_FLANK = 16
ACTIVITY_MAX_WEIGHT = 1 << 20
assert ctypes.sizeof(NearHitT) == 32
REGION_CLASSES_MAX = 8
assert ctypes.sizeof(TopHitT) == 24

# every symbol include/calitas_hip.h declares
SYMBOLS = ["calitas_create", "calitas_destroy", "calitas_last_error", "calitas_free", "calitas_set_reference",
           "calitas_set_reference_fasta", "calitas_save_index", "calitas_load_index", "calitas_reference_info", "calitas_contig_name", "calitas_genome_build", "calitas_fetch_bases", "calitas_expand_rows",
           "calitas_window_table", "calitas_search", "calitas_search_hits", "calitas_search_hits_stream", "calitas_search_hits_into", "calitas_pin_host", "calitas_unpin_host", "calitas_alloc_host", "calitas_release_parked", "calitas_search_hits_batch", "calitas_get_timing", "calitas_scan_candidates", "calitas_scan_candidates_columnwise", "calitas_contig_packed_base", "calitas_reference_tiles", "calitas_window_filter", "calitas_hits_tsv", "calitas_hits_tsv_ext", "calitas_search_variants", "calitas_search_variants_into", "calitas_vcf_identifier", "calitas_vcf_records",
           "calitas_padded_strings", "calitas_align_windows", "calitas_padded_strings_target", "calitas_version", "calitas_switches", "calitas_reap_wait",
           "calitas_search_counts", "calitas_search_counts_batch", "calitas_hits_counts",
           "calitas_search_scores", "calitas_search_scores_batch", "calitas_hits_scores",
           "calitas_search_top", "calitas_search_top_batch", "calitas_hits_top",
           "calitas_set_regions", "calitas_search_regions", "calitas_search_regions_batch", "calitas_hits_regions", "calitas_region_class",
           "calitas_find_sites", "calitas_count_sites", "calitas_find_sites_host",
           "calitas_find_sites_filtered", "calitas_count_sites_filtered", "calitas_find_sites_filtered_host",
           "calitas_count_copies", "calitas_count_copies_host", "calitas_count_near", "calitas_count_near_host",
           "calitas_score_near", "calitas_score_near_host", "calitas_list_near", "calitas_list_near_host",
           "calitas_find_sites_scored", "calitas_find_sites_scored_host",
           "calitas_find_sites_regions", "calitas_count_sites_regions", "calitas_find_sites_regions_host", "calitas_count_sites_regions_host",
           "calitas_site_presence",
           "calitas_find_site_pairs", "calitas_count_site_pairs", "calitas_find_site_pairs_host", "calitas_count_site_pairs_host",
           "calitas_find_allele_sites", "calitas_count_allele_sites", "calitas_find_allele_sites_host", "calitas_count_allele_sites_host",
           "calitas_find_edit_sites", "calitas_count_edit_sites", "calitas_find_edit_sites_host", "calitas_count_edit_sites_host",
           "calitas_find_sites_microhomology", "calitas_find_sites_microhomology_host"]

if not os.path.exists(LIB_PATH):
    raise ImportError("%s is missing: build it with `make -C calitas_amd/csrc` (hipcc, gfx950). "
                      "calitas_amd has no fallback implementation." % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)
lib.calitas_last_error.restype = ctypes.c_char_p
lib.calitas_last_error.argtypes = [ctypes.c_void_p]
lib.calitas_version.restype = ctypes.c_char_p
lib.calitas_switches.restype = ctypes.c_char_p
if hasattr(lib, "calitas_reap_wait"):
    lib.calitas_reap_wait.restype = None
    lib.calitas_reap_wait.argtypes = []
lib.calitas_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
lib.calitas_destroy.argtypes = [ctypes.c_void_p]
lib.calitas_destroy.restype = None
lib.calitas_free.argtypes = [ctypes.c_void_p]
lib.calitas_free.restype = None
lib.calitas_set_reference.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p]
lib.calitas_set_reference_fasta.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
lib.calitas_save_index.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
lib.calitas_load_index.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
lib.calitas_reference_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64),
                                       ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_contig_name.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_fetch_bases.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p]
if hasattr(lib, "calitas_expand_rows"):   # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_expand_rows.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p,
                                        ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_window_table.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_search.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT),
                               ctypes.POINTER(ctypes.POINTER(AlnT)), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_scan_candidates.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT),
                                        ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_scan_candidates_columnwise.argtypes = lib.calitas_scan_candidates.argtypes
lib.calitas_reference_tiles.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint64)] * 4
lib.calitas_contig_packed_base.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_get_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(TimingT)]
lib.calitas_window_filter.argtypes = [ctypes.POINTER(AlnT), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
lib.calitas_hits_tsv.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_char_p, ctypes.POINTER(ParamsT),
                                 ctypes.POINTER(AlnT), ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p,
                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_search_hits.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_char_p, ctypes.POINTER(ParamsT), ctypes.c_char_p,
                                    ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                    ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_search_hits_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ctypes.c_char_p),
                                          ctypes.POINTER(ParamsT), ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_search_hits_into.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_char_p, ctypes.POINTER(ParamsT), ctypes.c_char_p,
                                         ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_search_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(ctypes.POINTER(CountsT))]
lib.calitas_search_counts_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT),
                                            ctypes.POINTER(ctypes.POINTER(CountsT))]
lib.calitas_hits_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(AlnT), ctypes.c_uint64,
                                    ctypes.POINTER(ctypes.POINTER(CountsT))]
lib.calitas_find_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                   ctypes.POINTER(ctypes.POINTER(SiteT)), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_find_sites_host.argtypes = lib.calitas_find_sites.argtypes
lib.calitas_count_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                    ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_find_sites_filtered.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.c_int32, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(SiteT)), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_find_sites_filtered_host.argtypes = lib.calitas_find_sites_filtered.argtypes
lib.calitas_count_sites_filtered.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.c_int32, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_count_copies.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_count_copies_host.argtypes = lib.calitas_count_copies.argtypes
lib.calitas_count_near.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64,
                                   ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_count_near_host.argtypes = lib.calitas_count_near.argtypes
# (scores: calitas_near_score_t[n], two uint64 each -- passed as the words of a (n, 2) array)
lib.calitas_score_near.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_int32, ctypes.POINTER(ScoreModelT), ctypes.c_int32, ctypes.c_uint64,
                                   ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_score_near_host.argtypes = lib.calitas_score_near.argtypes
if hasattr(lib, "calitas_list_near"):      # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_list_near.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_int32, ctypes.POINTER(ScoreModelT), ctypes.c_int32, ctypes.c_uint64,
                                      ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.POINTER(NearHitT)), ctypes.POINTER(ctypes.c_uint64)]
    lib.calitas_list_near_host.argtypes = lib.calitas_list_near.argtypes
if hasattr(lib, "calitas_find_sites_scored"):      # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_find_sites_scored.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.POINTER(ActivityModelT), ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(SiteT)),
                                              ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), ctypes.POINTER(ctypes.c_uint64)]
    lib.calitas_find_sites_scored_host.argtypes = lib.calitas_find_sites_scored.argtypes
if hasattr(lib, "calitas_find_sites_regions"):     # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_find_sites_regions.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.POINTER(SiteRegionsT), ctypes.c_int32,
                                               ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(SiteT)),
                                               ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(ctypes.c_uint64)]
    lib.calitas_find_sites_regions_host.argtypes = lib.calitas_find_sites_regions.argtypes
    lib.calitas_count_sites_regions.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.POINTER(SiteRegionsT), ctypes.c_int32,
                                                ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.calitas_count_sites_regions_host.argtypes = lib.calitas_count_sites_regions.argtypes
    lib.calitas_site_presence.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint64)]
if hasattr(lib, "calitas_find_site_pairs"):        # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_find_site_pairs.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.POINTER(SitePairsT), ctypes.c_int32,
                                            ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(SiteT)), ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.POINTER(SitePairT)), ctypes.POINTER(ctypes.c_uint64)]
    lib.calitas_find_site_pairs_host.argtypes = lib.calitas_find_site_pairs.argtypes
    lib.calitas_count_site_pairs.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.POINTER(SitePairsT), ctypes.c_int32,
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.POINTER(ctypes.c_uint64)]
    lib.calitas_count_site_pairs_host.argtypes = lib.calitas_count_site_pairs.argtypes
if hasattr(lib, "calitas_find_allele_sites"):      # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_find_allele_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(AlleleSiteT)),
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.calitas_find_allele_sites_host.argtypes = lib.calitas_find_allele_sites.argtypes
    lib.calitas_count_allele_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.calitas_count_allele_sites_host.argtypes = lib.calitas_count_allele_sites.argtypes
if hasattr(lib, "calitas_find_edit_sites"):        # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_find_edit_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(BaseEditT), ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.POINTER(ctypes.POINTER(EditSiteT)), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.calitas_find_edit_sites_host.argtypes = lib.calitas_find_edit_sites.argtypes
    lib.calitas_count_edit_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(BaseEditT), ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.calitas_count_edit_sites_host.argtypes = lib.calitas_count_edit_sites.argtypes
if hasattr(lib, "calitas_find_sites_microhomology"):   # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_find_sites_microhomology.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(SiteFilterT), ctypes.POINTER(MhModelT), ctypes.c_int32,
                                                     ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(SiteT)),
                                                     ctypes.POINTER(ctypes.POINTER(MhScoreT)), ctypes.POINTER(ctypes.c_uint64)]
    lib.calitas_find_sites_microhomology_host.argtypes = lib.calitas_find_sites_microhomology.argtypes
lib.calitas_search_scores.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(ScoreModelT),
                                      ctypes.POINTER(ctypes.POINTER(ScoresT))]
lib.calitas_search_scores_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT),
                                            ctypes.POINTER(ScoreModelT), ctypes.POINTER(ctypes.POINTER(ScoresT))]
lib.calitas_hits_scores.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(ScoreModelT),
                                    ctypes.POINTER(AlnT), ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(ScoresT))]
lib.calitas_search_top.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(ScoreModelT), ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.POINTER(TopT))]
lib.calitas_search_top_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT),
                                         ctypes.POINTER(ScoreModelT), ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(TopT))]
lib.calitas_hits_top.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(ScoreModelT), ctypes.c_uint32,
                                 ctypes.POINTER(AlnT), ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(TopT))]
lib.calitas_set_regions.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(RegionT), ctypes.c_uint32]
lib.calitas_search_regions.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(ScoreModelT), ctypes.c_uint32,
                                       ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(RegionsT))]
lib.calitas_search_regions_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT),
                                             ctypes.POINTER(ScoreModelT), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(RegionsT))]
lib.calitas_hits_regions.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(ParamsT), ctypes.POINTER(ScoreModelT), ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.POINTER(AlnT), ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(RegionsT))]
lib.calitas_region_class.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]
lib.calitas_pin_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
lib.calitas_unpin_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.calitas_genome_build.restype = ctypes.c_char_p
lib.calitas_genome_build.argtypes = [ctypes.c_void_p]
TextSink = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p)
lib.calitas_search_hits_stream.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_char_p, ctypes.POINTER(ParamsT), ctypes.c_char_p,
                                           ctypes.c_char_p, TextSink, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_search_variants.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_char_p, ctypes.POINTER(ParamsT), ctypes.c_char_p,
                                        ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p),
                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
if hasattr(lib, "calitas_search_variants_into"):   # (an older build behind CALITAS_LIB_PATH, for A/B runs, does not have it)
    lib.calitas_search_variants_into.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_char_p, ctypes.POINTER(ParamsT), ctypes.c_char_p,
                                                 ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
if hasattr(lib, "calitas_alloc_host"):
    lib.calitas_alloc_host.argtypes = [ctypes.c_uint64]
    lib.calitas_alloc_host.restype = ctypes.c_void_p
if hasattr(lib, "calitas_vcf_records"):
    lib.calitas_vcf_identifier.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.calitas_vcf_records.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_hits_tsv_ext.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.c_char_p, ctypes.POINTER(ParamsT), ctypes.POINTER(AlnT),
                                     ctypes.c_uint64, ctypes.POINTER(ExtHitT), ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p,
                                     ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
lib.calitas_padded_strings.argtypes = [ctypes.c_void_p, ctypes.POINTER(GuideT), ctypes.POINTER(AlnT), ctypes.c_char_p,
                                       ctypes.c_char_p, ctypes.c_char_p]


lib.calitas_align_windows.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(GuideT), ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ParamsT),
                                      ctypes.POINTER(ctypes.POINTER(AlnT)), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))]
lib.calitas_padded_strings_target.argtypes = [ctypes.POINTER(GuideT), ctypes.POINTER(AlnT), ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int32,
                                              ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]


def check(ctx, rc):
    if rc != OK:
        msg = lib.calitas_last_error(ctx)
        raise CalitasError(rc, msg.decode() if msg else "?")
