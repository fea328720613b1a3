"""calitas_amd -- MI355X-native CALITAS SearchReference hot path (HIP kernels behind a C ABI)."""
from .aligner import (ACTIVITY_NONE, ALLELE_KINDS, ALLELE_SITE_DTYPE, MH_NONE, MH_SCORE_DTYPE, SNV_DTYPE, ActivityModel, MicrohomologyModel, AlleleSites, Alignment, CalitasError, Context, Defaults, Guide, NearList, NearScores, Regions, RegionScores, ScoreModel, Scores, SearchReference, SiteFilter, SitePairs, Top, TopHit,  # noqa: F401
                      activity_of, activity_value, allele_sites_of, snvs_of, counts_of_rows, counts_tsv, make_params, microhomology_of, near_hits_of, near_score, read_counts_tsv, read_hits, score_of_row, scores_of_rows, scores_tsv,
                      class_of_row, iupac_revcomp, site_class_of, site_cut_of, site_pairs_of, regions_of_rows, regions_tsv, top_of_rows, top_tsv, window_filter)
from .tools import (ALLELE_COLUMNS, GuideAlignment, GuideSite, SequentialGuideAligner, align_to_reference, allele_sites_tsv, find_guides, find_guides_tool,  # noqa: F401,E402
                    guide_copies, guide_counts, guide_near, guide_near_list, guide_near_scores, guide_pairs, guide_scores, guides_tsv, pairs_tsv, near_list_tsv, pairwise_align_sequences, read_fasta, site_filter_of_flags, snvs_of_vcf)
from .variants import prepare_vcf, read_vcf  # noqa: F401,E402
