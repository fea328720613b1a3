"""`python -m calitas_amd <Tool> [flags]` -- FindGuides (this project's own: tools.find_guides_tool) and the reference's four tools (Main.scala; flags as in SearchReference.scala:452-470,
AlignToReference.scala:34-51, PairwiseAlignSequences.scala:25-33, PrepareVcf.scala:32-36) on the MI355X path.
`-t/--threads` is accepted and ignored: the GPU replaces the thread pool."""
import argparse
import sys

from .aligner import Defaults, ScoreModel, SearchReference
from .tools import align_to_reference, find_guides_tool, pairwise_align_sequences
from .variants import prepare_vcf


def _costs(ap):
    ap.add_argument("-m", "--guide-mismatch-net-cost", type=int, default=Defaults.MismatchNetCost)
    ap.add_argument("-M", "--pam-mismatch-net-cost", type=int, default=Defaults.PamMismatchNetCost)
    ap.add_argument("-b", "--genome-gap-net-cost", type=int, default=Defaults.GenomeGapNetCost)
    ap.add_argument("-B", "--guide-gap-net-cost", type=int, default=Defaults.GuideGapNetCost)
    ap.add_argument("-t", "--threads", type=int, default=8)
    ap.add_argument("--device", type=int, default=0, help="HIP device index")


def main(argv=None):
    top = argparse.ArgumentParser(prog="calitas_amd")
    sub = top.add_subparsers(dest="tool", required=True)

    sr = sub.add_parser("SearchReference")
    sr.add_argument("-i", "--guide", required=True)
    sr.add_argument("-I", "--guide-id", required=True)
    sr.add_argument("-x", "--auxiliary-pams", nargs="*", default=[])
    sr.add_argument("-r", "--ref", required=True)
    sr.add_argument("-v", "--variants")
    sr.add_argument("-V", "--max-variants", type=int, default=Defaults.MaxVariantsInCluster)
    sr.add_argument("-o", "--output")
    sr.add_argument("-w", "--window-size", type=int, default=1000)
    sr.add_argument("-d", "--max-guide-diffs", type=int, default=Defaults.MaxGuideDiffs)
    sr.add_argument("-p", "--max-pam-mismatches", type=int, default=Defaults.MaxPamMismatches)
    sr.add_argument("-g", "--max-gaps-between-guide-and-pam", type=int, default=Defaults.MaxGapsBetweenGuideAndPam)
    sr.add_argument("-D", "--max-total-diffs", type=int)
    sr.add_argument("-O", "--max-overlap", type=int, default=Defaults.MaxOverlap)
    sr.add_argument("-c", "--chrom")
    sr.add_argument("--counts", action="store_true",
                    help="write the off-target table (guide_id strand guide_mm guide_gaps pam_mm hits; non-zero cells) instead of hits.txt")
    sr.add_argument("--scores", metavar="MODEL",
                    help="write the specificity score under the model file (guide_id rows perfect offtarget_sum_q32 max_q32 specificity) "
                         "instead of hits.txt; with --counts the table's TSV follows it behind an empty line")
    sr.add_argument("--top", metavar="K", type=int,
                    help="with --scores: the K (1 .. 256) highest-scoring imperfect hits of the same pass behind the scores and an empty line "
                         "(guide_id rank chromosome coordinate_start coordinate_end strand guide_mm guide_gaps pam_mm score_q32 score)")
    sr.add_argument("--regions", metavar="FILE.bed",
                    help="with --scores: the scores split by the classes of a four-column BED file (chromosome start end class; the classes take "
                         "priority in order of first appearance, at most 7) behind the scores and an empty line "
                         "(guide_id class rows perfect offtarget_sum_q32 max_q32 specificity); the --top lines gain a last column class")
    sr.add_argument("--top-classes", metavar="NAME,...",
                    help="with --regions and --top: list only hits of these classes (elsewhere: outside every interval)")
    _costs(sr)

    a2r = sub.add_parser("AlignToReference")
    a2r.add_argument("-i", "--input", required=True)
    a2r.add_argument("-r", "--ref", required=True)
    a2r.add_argument("-o", "--output")
    a2r.add_argument("-w", "--window-size", type=int)
    a2r.add_argument("-d", "--max-guide-diffs", type=int)
    a2r.add_argument("-p", "--max-pam-mismatches", type=int)
    a2r.add_argument("-g", "--max-gaps-between-guide-and-pam", type=int, default=Defaults.MaxGapsBetweenGuideAndPam)
    a2r.add_argument("-D", "--max-total-diffs", type=int)
    a2r.add_argument("-O", "--max-overlap", type=int)
    _costs(a2r)

    pas = sub.add_parser("PairwiseAlignSequences")
    pas.add_argument("-i", "--input", required=True)
    pas.add_argument("-o", "--output", default="/dev/stdout")
    pas.add_argument("-g", "--max-gaps-between-guide-and-pam", type=int, default=Defaults.MaxGapsBetweenGuideAndPam)
    pas.add_argument("-O", "--max-overlap", type=int, default=Defaults.MaxOverlap)   # declared and unused by the reference as well
    _costs(pas)

    fg = sub.add_parser("FindGuides", help="the guides a region offers: exact sites of an IUPAC pattern such as NNNNNNNNNNNNNNNNNNNNnrg")
    fg.add_argument("-i", "--guide", required=True, help="the pattern: IUPAC protospacer in upper case, PAM in lower case at either end")
    fg.add_argument("-x", "--auxiliary-pams", nargs="*", default=[])
    fg.add_argument("-r", "--ref", required=True)
    fg.add_argument("-c", "--chrom")
    fg.add_argument("-s", "--start", type=int, default=0, help="0-based first base of the region")
    fg.add_argument("-e", "--end", type=int, help="0-based end of the region, exclusive (default: the contig's end)")
    fg.add_argument("-o", "--output")
    fg.add_argument("--counts", action="store_true",
                    help="search every distinct guide of the table (the flags below) and add hits, hits_mm0 .. hits_mmE per row")
    fg.add_argument("--scores", metavar="MODEL",
                    help="like --counts, and score every guide's hits under the model file: the columns perfect and specificity follow")
    fg.add_argument("--gc-min", metavar="PCT", type=int, help="keep guides whose protospacer has at least PCT percent G + C (0 .. 100)")
    fg.add_argument("--gc-max", metavar="PCT", type=int, help="... and at most PCT percent")
    fg.add_argument("--max-run", metavar="SPEC", help="the longest run of one base a protospacer may hold: N, or T=3,G=4 (unnamed bases unlimited)")
    fg.add_argument("--avoid", metavar="MOTIF", action="append", default=[],
                    help="drop guides whose protospacer holds this IUPAC motif or its reverse complement (repeatable; 8 motifs in all)")
    fg.add_argument("--copies", action="store_true",
                    help="add copies: the sites of the pattern in the whole reference with this row's protospacer, the row's own among them")
    fg.add_argument("--seed-copies", metavar="K", type=int,
                    help="add seed_copies: the same for the PAM-proximal K bases of the protospacer (1 .. its length)")
    fg.add_argument("--max-copies", metavar="N", type=int, help="drop guides with more than N copies (N >= 1; implies --copies)")
    fg.add_argument("--max-seed-copies", metavar="N", type=int, help="drop guides with more than N seed copies (needs --seed-copies)")
    fg.add_argument("--near-copies", metavar="M", type=int,
                    help="add copies_mm0 .. copies_mmM: the sites of the pattern in the whole reference whose protospacer differs from this row's at exactly that many positions (M is 0 .. 3)")
    fg.add_argument("--max-near-copies", metavar="N", type=int, help="drop guides whose copies_mm columns sum to more than N (N >= 1; needs --near-copies)")
    fg.add_argument("--near-scores", metavar="MODEL",
                    help="with --near-copies M: score every row's near copies under the model file in the same pass and add near_sum_q32, near_max_q32, near_specificity")
    fg.add_argument("--near-list", metavar="FILE",
                    help="with --near-copies M: write every kept guide's copies within M substitutions to FILE, one per line (scored under --near-scores' model when given)")
    fg.add_argument("--near-list-limit", metavar="N", type=int, help="with --near-list: a guide with more than N copies writes no line (1 .. 4096, default 1000)")
    fg.add_argument("--activity", metavar="MODEL",
                    help="add activity_q16 and activity: every site's on-target score under the activity model file (models/example_activity30.tsv shows the format), NA where a site has none")
    fg.add_argument("--min-activity", metavar="X",
                    help="with --activity: drop guides whose LINEAR score is below the decimal X, and those without a score; under `link logistic` a probability p is X = ln(p / (1 - p))")
    fg.add_argument("--regions", metavar="FILE.bed",
                    help="keep only the sites that lie in the file's intervals (chromosome, start, end, class name; the rules of SearchReference --regions) and add the column class")
    fg.add_argument("--classes", metavar="NAME,...", help="with --regions: the classes to keep (default: every named class; elsewhere: outside every interval)")
    fg.add_argument("--class-extent", metavar="FROM:TO",
                    help="with --regions: class positions FROM .. TO - 1 of the protospacer as the guide reads (0-based, half-open; 16:18 of a 20-mer with a 3' PAM is the Cas9 cut) instead of all of it")
    fg.add_argument("--pairs", metavar="FILE",
                    help="write the pairs of the kept guides whose cuts are --pair-distance apart to FILE, one per line (paired nickases, excisions); the table itself does not change")
    fg.add_argument("--pair-distance", metavar="MIN:MAX", help="with --pairs (required): the bounds on the distance of the two cuts, 0 <= MIN <= MAX <= 65535")
    fg.add_argument("--pair-cut", metavar="N",
                    help="with --pairs: where a site is cut, a position 0 .. L of the protospacer as the guide reads (default L - 3, the Cas9 cut, with a 3' PAM; required otherwise)")
    fg.add_argument("--pair-orientation", metavar="out|in|same|any|CODE,...",
                    help="with --pairs: the orientations to keep -- out (PAMs facing outwards, the default), in, same, any, or codes among ++ -+ +- -- (left strand, right strand)")
    fg.add_argument("--alleles", metavar="FILE.vcf[.gz]",
                    help="with --allele-sites or --edit-sites: the SNVs (single-letter REF and ALT of A C G T) whose position lies in the region; the table itself does not change")
    fg.add_argument("--allele-sites", metavar="OUT.tsv",
                    help="with --alleles: write the sites each SNV creates (allele alt), destroys (ref) or changes (both) to OUT.tsv, one per line")
    fg.add_argument("--allele-kinds", metavar="alt,ref,both", help="with --alleles: the kinds of lines to write (default all three)")
    fg.add_argument("--edit-sites", metavar="OUT.tsv",
                    help="with --alleles, --editor and --edit-window: write the guides that put each SNV into the base editor's window on the strand it can change it on, and their bystanders, to OUT.tsv, one per line")
    fg.add_argument("--editor", metavar="FROM:TO", help="with --edit-sites: the editor's change, two different letters of A C G T (C:T a CBE, A:G an ABE, C:G a CGBE)")
    fg.add_argument("--edit-window", metavar="FROM:TO", help="with --edit-sites: the positions of the protospacer as the guide reads that the editor reaches, 0-based and half-open")
    fg.add_argument("--edit-context", metavar="LETTER", help="with --edit-sites: the IUPAC letter the base 5' of an edited base must lie in (default N: any)")
    fg.add_argument("--edit-mode", metavar="install|correct", help="with --edit-sites: install (default): the cell carries REF and the edit makes ALT; correct: the cell carries ALT and the edit makes REF")
    fg.add_argument("--max-bystanders", metavar="N", help="with --edit-sites: only the guides with at most N other editable bases in the window (0 .. 31)")
    fg.add_argument("--microhomology", metavar="MODEL",
                    help="add mh_total_q16, mh_oof_q16, mh_score and out_of_frame: the microhomology score around every site's cut and the share of it that shifts the frame, under the model file (models/example_microhomology60.tsv shows the format), NA where a site has none")
    fg.add_argument("--mh-cut", metavar="N", help="with --microhomology: the cut's position in the protospacer as the guide reads, 0 .. L (default L - 3 with a 3' PAM, required otherwise)")
    fg.add_argument("--min-out-of-frame", metavar="PCT",
                    help="with --microhomology: drop guides whose out_of_frame is below the integer PCT (0 .. 100), those whose mh_total_q16 is 0 and those without a score")
    fg.add_argument("-d", "--max-guide-diffs", type=int, default=Defaults.MaxGuideDiffs)
    fg.add_argument("-p", "--max-pam-mismatches", type=int, default=Defaults.MaxPamMismatches)
    fg.add_argument("-g", "--max-gaps-between-guide-and-pam", type=int, default=Defaults.MaxGapsBetweenGuideAndPam)
    fg.add_argument("-D", "--max-total-diffs", type=int)
    fg.add_argument("-O", "--max-overlap", type=int, default=Defaults.MaxOverlap)
    _costs(fg)

    pv = sub.add_parser("PrepareVcf")
    pv.add_argument("-i", "--input", nargs="+", required=True)
    pv.add_argument("-o", "--output", required=True)
    pv.add_argument("-f", "--min-af", type=float, default=0.01)
    pv.add_argument("-d", "--dict", help="sequence dictionary (.dict, .fai, or a FASTA with its .dict) that overrides the contig lines")
    pv.add_argument("-c", "--add-chr-prefix", type=lambda s: s.lower() in ("1", "true", "yes"), default=True)

    a = top.parse_args(argv)
    if a.tool == "SearchReference":
        if a.scores is not None and a.variants is not None:
            top.error("--scores covers the reference-genome branch only (no --variants)")
        if a.top is not None and a.scores is None:
            top.error("--top K requires --scores MODEL")
        if a.top is not None and not 1 <= a.top <= 256:
            top.error("--top K: K is 1 .. 256")
        if a.regions is not None and a.scores is None:
            top.error("--regions FILE.bed requires --scores MODEL")
        if a.regions is not None and a.variants is not None:
            top.error("--regions covers the reference-genome branch only (no --variants)")
        if a.top_classes is not None and (a.regions is None or a.top is None):
            top.error("--top-classes requires --regions and --top")
        SearchReference(guide=a.guide, guide_id=a.guide_id, ref=a.ref, output=a.output, auxiliary_pams=a.auxiliary_pams,
                        window_size=a.window_size, max_guide_diffs=a.max_guide_diffs, max_pam_mismatches=a.max_pam_mismatches,
                        max_gaps_between_guide_and_pam=a.max_gaps_between_guide_and_pam, max_total_diffs=a.max_total_diffs,
                        max_overlap=a.max_overlap, guide_mismatch_net_cost=a.guide_mismatch_net_cost,
                        pam_mismatch_net_cost=a.pam_mismatch_net_cost, genome_gap_net_cost=a.genome_gap_net_cost,
                        guide_gap_net_cost=a.guide_gap_net_cost, chrom=a.chrom, variants=a.variants, max_variants=a.max_variants,
                        device=a.device).execute(counts=a.counts, scores=ScoreModel.read(a.scores) if a.scores is not None else None, top=a.top,
                                                   regions=a.regions, top_classes=a.top_classes)
    elif a.tool == "AlignToReference":
        text = align_to_reference(a.input, a.ref, a.output, window_size=a.window_size, max_guide_diffs=a.max_guide_diffs,
                                  max_pam_mismatches=a.max_pam_mismatches, max_gaps_between_guide_and_pam=a.max_gaps_between_guide_and_pam,
                                  max_total_diffs=a.max_total_diffs, max_overlap=a.max_overlap,
                                  guide_mismatch_net_cost=a.guide_mismatch_net_cost, pam_mismatch_net_cost=a.pam_mismatch_net_cost,
                                  genome_gap_net_cost=a.genome_gap_net_cost, guide_gap_net_cost=a.guide_gap_net_cost, device=a.device)
        if a.output is None:
            sys.stdout.write(text)
    elif a.tool == "FindGuides":
        text = find_guides_tool(a.ref, a.guide, a.auxiliary_pams, chrom=a.chrom, start=a.start, end=a.end, output=a.output, counts=a.counts, scores=a.scores,
                                device=a.device, gc_min=a.gc_min, gc_max=a.gc_max, max_run=a.max_run, avoid=a.avoid, copies=a.copies,
                                seed_copies=a.seed_copies, max_copies=a.max_copies, max_seed_copies=a.max_seed_copies, near_copies=a.near_copies, max_near_copies=a.max_near_copies, near_scores=a.near_scores, near_list=a.near_list, near_list_limit=a.near_list_limit, activity=a.activity, min_activity=a.min_activity, regions=a.regions, classes=a.classes, class_extent=a.class_extent, pairs=a.pairs, pair_distance=a.pair_distance, pair_cut=a.pair_cut, pair_orientation=a.pair_orientation, alleles=a.alleles, allele_sites=a.allele_sites, allele_kinds=a.allele_kinds, microhomology=a.microhomology, mh_cut=a.mh_cut, min_out_of_frame=a.min_out_of_frame, edit_sites=a.edit_sites, editor=a.editor, edit_window=a.edit_window, edit_context=a.edit_context, edit_mode=a.edit_mode, max_bystanders=a.max_bystanders,
                                max_guide_diffs=a.max_guide_diffs, max_pam_mismatches=a.max_pam_mismatches,
                                max_gaps_between_guide_and_pam=a.max_gaps_between_guide_and_pam, max_total_diffs=a.max_total_diffs,
                                max_overlap=a.max_overlap, guide_mismatch_net_cost=a.guide_mismatch_net_cost,
                                pam_mismatch_net_cost=a.pam_mismatch_net_cost, genome_gap_net_cost=a.genome_gap_net_cost,
                                guide_gap_net_cost=a.guide_gap_net_cost)
        if a.output is None:
            sys.stdout.write(text)
    elif a.tool == "PairwiseAlignSequences":
        pairwise_align_sequences(a.input, a.output, max_gaps_between_guide_and_pam=a.max_gaps_between_guide_and_pam,
                                 mismatch_net_cost=a.guide_mismatch_net_cost, pam_mismatch_net_cost=a.pam_mismatch_net_cost,
                                 genome_gap_net_cost=a.genome_gap_net_cost, guide_gap_net_cost=a.guide_gap_net_cost, device=a.device)
    else:
        prepare_vcf(a.input, a.output, min_af=a.min_af, add_chr_prefix=a.add_chr_prefix, dict_path=a.dict)
    return 0


if __name__ == "__main__":
    sys.exit(main())
