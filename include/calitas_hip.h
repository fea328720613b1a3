/* calitas_hip.h -- C ABI of the MI355X-native CALITAS SearchReference hot path (libcalitas_hip.so).
 *
 * The reference (editasmedicine/calitas, Scala/JVM) has no FFI.  The narrowest seam with stable meaning is
 *   SequentialGuideAligner.align(guide, target, targetName, targetOffset, maxGuideDiffs, maxGapsBetweenGuideAndPam,
 *                                maxPamDiffs, maxTotalDiffs, maxOverlap): Seq[GuideAlignment]
 *   (calitas/src/main/scala/com/editasmedicine/aligner/SequentialGuideAligner.scala:228-236), called once per
 *   reference window from SearchReference.execute (SearchReference.scala:537-561).
 * One call per 1000-bp window is too fine for a GPU, so this ABI lifts the same contract to
 * "all windows of a resident reference x a batch of guides": calitas_search returns, window by window and in the
 * reference's order, exactly the GuideAlignments those align() calls return.  Everything below that seam
 * (the fgbio glocal DP, PAM extension, per-window overlap filter) runs in hand-written HIP kernels for gfx950;
 * everything above it (removeOverlaps, ReferenceHit rows, hits.txt) is host code with the reference's semantics.
 *
 * Conventions: plain C types only; inputs are borrowed for the duration of the call; outputs are allocated by the
 * library and released with calitas_free; every function returning int returns 0 on success and a non-zero
 * CALITAS_E* code on failure, with a message available from calitas_last_error.  Results are never truncated:
 * a device buffer overflow is detected and the search is re-run with larger buffers.
 * Threading: calls on one context are serialised by the caller; one context drives one GPU.
 */
#ifndef CALITAS_HIP_H
#define CALITAS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CALITAS_OK 0
#define CALITAS_EINVAL 1   /* bad argument / unsupported configuration */
#define CALITAS_ENODEV 2   /* no usable HIP device, or context created host-only */
#define CALITAS_EHIP 3     /* HIP runtime error */
#define CALITAS_EIO 4      /* file could not be read / written */
#define CALITAS_ESTATE 5   /* call made in the wrong state (e.g. search before set_reference) */
#define CALITAS_ENOMEM 6   /* a device allocation failed (calitas_search_hits answers it with one pass per contig before giving up) */

#define CALITAS_MAX_PROTOSPACER 32   /* rows of the bit-vector scan kernel */
#define CALITAS_MAX_PAMS 8
#define CALITAS_MAX_PAM_LEN 16
#define CALITAS_MAX_OPS 128          /* padded alignment columns per record */
#define CALITAS_MAX_GUIDES 64        /* guides per calitas_search batch */

typedef struct calitas_ctx calitas_ctx;

/* Guide = SequentialGuideAligner.Guide (SequentialGuideAligner.scala:32-52): protospacer in upper case, zero or more
 * PAMs in lower case, all on the same side. */
typedef struct {
  const char* protospacer;
  int32_t n_pams;
  const char* const* pams;
  int32_t pam_is_5prime;
  int32_t cli_length;        /* length of the `-i` string (protospacer + primary PAM), SearchReference.scala:528,536 */
} calitas_guide_t;

/* Flags of SearchReference (SearchReference.scala:452-470) that reach the aligner. */
typedef struct {
  int32_t window_size;                     /* -w  default 1000 */
  int32_t max_guide_diffs;                 /* -d  default 5 */
  int32_t max_pam_mismatches;              /* -p  default 1 */
  int32_t max_gaps_between_guide_and_pam;  /* -g  default 3 */
  int32_t max_total_diffs;                 /* -D  <0 => d+g+p (SearchReference.scala:493) */
  int32_t max_overlap;                     /* -O  default 10 */
  int32_t guide_mismatch_net_cost;         /* -m  default -120 */
  int32_t pam_mismatch_net_cost;           /* -M  default -260 */
  int32_t genome_gap_net_cost;             /* -b  default -122 */
  int32_t guide_gap_net_cost;              /* -B  default -121 */
  int32_t chrom_index;                     /* -c  contig index, <0 => all */
  int32_t eqx_by_score;                    /* bit flags for the two readings of fgbio 2.0.0 that the reference's own tests do not
                                            * pin; 0 = the defaults.
                                            * bit 0 (1): '=' / 'X' by pairing score > 0 instead of IUPAC compatibility (U2; differs for a target N)
                                            * bit 1 (2): one alignment per bottom-row matrix cell (Diag, Left, Up) that reaches minScore
                                            *            instead of one per end column from the best of the three (U1) */
  int32_t max_variants;                    /* -V  only echoed into aligner_other_parameters */
  /* A window range [first_window, first_window + n_windows) of windowIterator's sequence for this (window size, step) over the whole
   * reference, contigs in order (the index calitas_window_table lists them in when min_length is 0); n_windows = 0 means all of
   * them.  The piece of a job one process of a multi-GPU partition runs (calitas_amd/shard.py window_partition):
   *  - calitas_search aligns exactly those windows: the alignments of consecutive ranges, concatenated, are those of the whole call;
   *  - calitas_search_hits / calitas_search_hits_into return the rows the range OWNS: the hits whose coordinate_start lies at or
   *    behind the start of window first_window and before the start of window first_window + n_windows.  coordinate_start is the
   *    first sort key of hits.txt, so the texts of consecutive ranges (minus their header lines) concatenate to the text of the
   *    whole call, wherever the cuts fall; removeOverlaps is exact across a cut because every process also aligns the windows
   *    around its stretch that can decide its hits.
   *  - calitas_search_hits_batch does the same for every guide of the batch (round 4: BASELINE config 4 on several GPUs is every
   *    process running all guides on its stretch), guides pipelined through the device stages as in the whole-genome batch.
   * The stream call refuses a range. */
  int32_t first_window;
  int32_t n_windows;
} calitas_params_t;

/* One GuideAlignment (GuideAlignment.scala:72-88).  Coordinates are 0-based half-open on the contig.  ops holds
 * one byte per padded column in the orientation of the guide as given on the command line:
 * '=' match, 'X' mismatch, 'I' base only in the guide (gap in genome), 'D' base only in the genome.
 * The padded strings are a pure function of (query, ops, strand, start_offset) and the reference bases. */
typedef struct {
  int32_t guide_index;
  int32_t contig_index;
  int32_t window_start;        /* 0-based offset of the (N-trimmed) window the alignment was found in */
  int32_t start_offset, end_offset;
  int32_t guide_start_offset, guide_end_offset;
  int32_t score;
  int8_t strand;               /* '+' or '-' */
  int8_t pam_index;            /* index into the guide's pams, -1 for a PAM-less guide */
  int16_t n_ops;
  uint8_t ops[CALITAS_MAX_OPS];
} calitas_aln_t;

/* Timing and volume of the last calitas_search on this context; kernel times are HIP-event measurements on the
 * stream the kernels were launched on.  Exception, for ranges whose tail ran on the per-bin kernels (binned_lanes): no event sits
 * between those kernels (each would hold the next kernel back by ~5 us), so align_kernel_ms is the difference of two stamps of the
 * device's wall clock taken by the kernels themselves, gpu_total_ms = the scan + the stamps' span up to the start of the row kernel,
 * and hits_kernel_ms = (end of the scan .. end of the row kernel, by events) - align_kernel_ms, which includes the kernel boundaries
 * of the chain.  scan_kernel_ms is always a pair of events riding on the scan's dispatch. */
typedef struct {
  double scan_kernel_ms;       /* bit-vector scan over the packed reference (both strands, all guides of the batch) */
  double align_kernel_ms;      /* banded glocal DP + traceback + PAM extension on the scan's candidates */
  double gpu_total_ms;         /* first launch to last copy-back */
  double host_post_ms;         /* per-window filter on the host */
  uint64_t bases_scanned;      /* reference bases covered by the scan (one count per base, not per strand) */
  uint64_t packed_bytes;       /* 2-bit bytes the scan reads from HBM per pass */
  uint64_t scan_records;       /* 16-base groups with at least one candidate end column */
  uint64_t candidate_columns;  /* candidate end columns (guide x strand x position) handed to the aligner kernel */
  uint64_t raw_alignments;     /* alignments surviving PAM extension, before the per-window filter */
  uint64_t accepted_alignments;
  uint32_t retries;            /* re-runs caused by device buffer overflow */
  uint32_t lanes;              /* contig ranges the last calitas_search_hits call pipelined (1 = one pass; 0 after calitas_search) */
  /* calitas_search_hits only */
  double hits_kernel_ms;       /* removeOverlaps + sorts + row text on the device */
  double hits_copy_ms;         /* the text's copy-back */
  uint64_t hit_rows;
  uint64_t hits_bytes;
  uint32_t contig_passes;        /* calitas_search_hits in one-pass-per-contig mode: passes run (0 otherwise) */
  uint32_t binned_lanes;         /* calitas_search_hits*: contig ranges / passes / guides whose tail (per-window filter ... rows) ran on the
                                  * per-bin kernels (binned.hpp); the others ran on the general kernels (same text) */
  uint32_t owned_general_lanes;  /* a window range (first_window / n_windows): pieces whose bins were crowded and whose owned rows the general
                                  * kernels decided from the same alignments (round 4; before, such a range searched its contigs whole) */
  uint32_t scan_variant;          /* calitas_scan_candidates: the scan_rows_kernel instantiation it launched, lane chunk << 8 | warm-up words
                                  * (0 for the column-wise kernel and after every other call) */
} calitas_timing_t;

/* Context ------------------------------------------------------------------------------------------------------- */

/* device_id >= 0: bind to that HIP device (fails with CALITAS_ENODEV when there is none -- there is no CPU fallback).
 * device_id == -1: host-only context for reference packing, window tables and hits formatting; calitas_search fails. */
int calitas_create(int device_id, calitas_ctx** out);
void calitas_destroy(calitas_ctx* ctx);
const char* calitas_last_error(const calitas_ctx* ctx);   /* ctx may be NULL: last error of calitas_create */
void calitas_free(void* p);

/* Reference ----------------------------------------------------------------------------------------------------- */

/* Replaces ReferenceSequenceIterator + windowIterator's byte[] contigs (SearchReference.scala:39-49): ASCII bases of
 * every contig, in sequence-dictionary order.  Packs to 2 bit/base + an exception-run table (N runs, IUPAC codes) and
 * uploads to HBM.  genome_build = first AS tag of the .dict or "unknown" (ReferenceHit.scala:208).
 * bases[i] == NULL with lengths[i] > 0: contig i is ABSENT -- its name and length count (windowIterator's sequence, the coordinates
 * and the sort order are those of the whole dictionary) but its bases are not held here: what a process of a multi-GPU job does
 * with the contigs its window range (calitas_params_t.first_window / n_windows) does not touch.  A search that would need an absent
 * contig fails with CALITAS_EINVAL. */
int calitas_set_reference(calitas_ctx* ctx, int32_t n_contigs, const char* const* names, const uint64_t* lengths,
                          const uint8_t* const* bases, const char* genome_build);
/* Convenience: read FASTA (+ .dict next to it when present) and call calitas_set_reference. */
int calitas_set_reference_fasta(calitas_ctx* ctx, const char* fasta_path);
/* Persistent packed index: the 2-bit codes, exception mask, run table and tile table of the resident reference, so a later
 * run can skip FASTA parsing and packing (replaces the per-run ReferenceSequenceFile scan of SearchReference.scala:34-49). */
int calitas_save_index(const calitas_ctx* ctx, const char* path);
int calitas_load_index(calitas_ctx* ctx, const char* path);
int calitas_reference_info(const calitas_ctx* ctx, int32_t* n_contigs, uint64_t* total_bases, uint64_t* packed_bytes);
int calitas_contig_name(const calitas_ctx* ctx, int32_t contig_index, const char** name, uint64_t* length);
/* genome_build column: first AS tag of the sequence dictionary, or "unknown" (ReferenceHit.scala:208). */
const char* calitas_genome_build(const calitas_ctx* ctx);
/* Upper-cased bases [start, start+len) of a contig re-derived from the packed form (what fetchBases sees after
 * toUpperCase, ReferenceHit.scala:261-266); out must hold len bytes. */
int calitas_fetch_bases(const calitas_ctx* ctx, int32_t contig_index, uint64_t start, uint32_t len, char* out);

/* Every environment switch the library reads (calitas_amd/csrc/tuning.hpp): "NAME <values> what it does" per line; the product has one
 * behaviour, the switches are for measurements, for tests that force a fallback path and for a caller that shares the card.  The string
 * lives as long as the library. */
const char* calitas_switches(void);

/* calitas_free of a text of gigabytes, and the tables calitas_search_variants builds on the way (millions of small heap blocks), are
 * handed back on a thread of the library's own: the calls return at once (CALITAS_FREE_NOW=1: before they return).  This waits until
 * that thread has nothing left to do -- for a caller who measures, or who wants the memory back before going on.  No reference
 * counterpart (the JVM's collector plays this part there). */
void calitas_reap_wait(void);

/* Test hook without a reference counterpart: the host half of the compact rows calitas_search_hits_batch moves over PCIe (round 4).  A
 * row of hits.txt is head | chromosome \t middle | tail with head (guide_id, unpadded_guide_sequence, genome_build) and tail (aligner ..
 * time_stamp, ReferenceHit.scala:99-132) the same for every row of a call; the device writes `chromosome \t middle \n` per row and
 * the library puts head and tail back on its worker pool.  compact[0..n): `rows` such rows; out: room for n + rows * (strlen(head) +
 * strlen(tail) - 1) bytes (out_capacity is checked).  *written receives the bytes written.  CALITAS_EINVAL when the text does not hold
 * exactly `rows` newline-terminated rows or out is too small.  ctx may be a host-only context (its worker pool is used). */
int calitas_expand_rows(calitas_ctx* ctx, const char* compact, uint64_t n, uint64_t rows, const char* head, const char* tail, char* out,
                        uint64_t out_capacity, uint64_t* written);

/* Window table of windowIterator (SearchReference.scala:39-71) after the length filter (SearchReference.scala:536):
 * rows of (contig_index, start0, end0) with N-trimmed 0-based half-open bounds.  Caller frees *out. */
int calitas_window_table(const calitas_ctx* ctx, int32_t window_size, int32_t step, int32_t min_length, int32_t chrom_index,
                         int32_t** out, uint64_t* n_windows);

/* Search -------------------------------------------------------------------------------------------------------- */

/* SearchReference.execute's alignment phase (SearchReference.scala:527-561) for n_guides guides in one pass over the
 * resident reference.  *out receives, guide by guide and window by window in windowIterator order, the alignments
 * SequentialGuideAligner.align returns for each window (after its per-window overlap filter). */
int calitas_search(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                   calitas_aln_t** out, uint64_t* n_out);
int calitas_get_timing(const calitas_ctx* ctx, calitas_timing_t* out);

/* The candidate filter of calitas_search on its own (the stage that decides which end columns the aligner kernel looks at):
 * every (16-base word of the packed reference, strand, guide) that holds at least one end column whose glocal bottom-row score
 * reaches minGuideScore for a seamless scan of the contig, i.e. fgbio's enumeration rule (SequentialGuideAligner.scala:261-299)
 * before windowing.  Out: n records of two uint32 each, sorted: [0] packed position / 16, [1] bits 0-15 column mask,
 * bit 16 strand pass (0 = target as is, 1 = reverse-complemented), bits 17-23 guide.  Exposed so that the two scan kernels can
 * be held against each other and against a plain dynamic-programming count in the tests; calitas_free releases *records. */
int calitas_scan_candidates(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                            uint32_t** records, uint64_t* n_records);
/* Test hook only: the same record set from round 1's column-wise scan kernel (one DP column per 32-bit word, the text walked base by
 * base).  No search entry point uses that kernel; it is kept as an independent second implementation of the filter for the tests. */
int calitas_scan_candidates_columnwise(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                       uint32_t** records, uint64_t* n_records);
/* Scan tiles of the resident reference: how many there are (contig tiles, padding excluded), how many of them the scan skips because
 * they hold nothing but upper-case N (no window can contain any of their bases, SearchReference.scala:58-59), how many carry
 * exception bases (N-run edges, IUPAC codes, contig ends), and the bases per tile. */
int calitas_reference_tiles(const calitas_ctx* ctx, uint64_t* n_tiles, uint64_t* n_dead, uint64_t* n_masked, uint64_t* tile_bases);
/* Packed position (the unit of calitas_scan_candidates) of base 0 of contig i. */
int calitas_contig_packed_base(const calitas_ctx* ctx, int32_t i, uint64_t* gbase);

/* SearchReference.execute for one guide on the reference genome, end to end (SearchReference.scala:527-564 and 641-648):
 * calitas_search followed by removeOverlaps, ReferenceHit.sort and the 34-column rows, with the alignments never leaving
 * the device -- the per-window filter, removeOverlaps, both sorts and the row text are produced by kernels and only the
 * finished hits.txt text (header + rows, NUL-terminated, *tsv_bytes without the NUL) is copied back.  Byte-identical to
 * calitas_search + calitas_hits_tsv; when a device stage cannot represent a search the host
 * implementation of that stage finishes the call, and when the buffers of a pass over the whole reference do not fit the
 * device (very permissive searches) the call runs one pass per contig instead (CALITAS_ENOMEM only if a single contig does
 * not fit).  aligner_version / time_stamp as in calitas_hits_tsv. */
int calitas_search_hits(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                        const char* aligner_version, const char* time_stamp, char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows);

/* calitas_search_hits for a batch of guides (BASELINE config 4: 96 guides against one reference) -- the loop a caller would
 * write around SearchReference, with the guides flowing through the stages as a pipeline: while guide g's alignments are
 * filtered, de-duplicated, turned into rows and copied back, guide g+1 is already being scanned.  tsv[i] / tsv_bytes[i] /
 * n_rows[i] receive what calitas_search_hits returns for guides[i] (byte-identical); each text is freed with calitas_free.
 * All guides must have the same length (one window tiling).  guide_ids may be NULL. */
int calitas_search_hits_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const char* const* guide_ids,
                              const calitas_params_t* params, const char* aligner_version, const char* time_stamp, char** tsv,
                              uint64_t* tsv_bytes, uint64_t* n_rows);

/* The off-target table of one guide: how many rows the hits.txt of calitas_search_hits (same guide, same params: after the per-window
 * filter and removeOverlaps; with first_window / n_windows, the rows the range owns) has per strand, guide_mm, guide_gaps and pam_mm
 * -- the hits.txt columns of those names (GuideAlignment.scala:103, 104, 106; the gap between guide and PAM counts as guide gaps).
 * Cell [s][m][g][p] of counts (strand '+' = 0, '-' = 1) is at ((s * n_mm + m) * n_gaps + g) * n_pam + p.  The extents depend on the
 * guide and the params only, never on the reference: n_mm = E + 1 with E the most edits the protospacer can have at this
 * max_guide_diffs and these net costs (max_guide_diffs itself for the default costs, more when an edit is cheaper than the dearest),
 * n_gaps = E + max_gaps_between_guide_and_pam + 1, n_pam = max_pam_mismatches + 1 (1 for a PAM-less guide) -- so the tables of window
 * ranges, contigs and ranks of one job add up element by element.  A hit outside the extents fails the call (it is never dropped or
 * clamped).  The struct and its counts are one block: one calitas_free. */
typedef struct {
  uint32_t n_mm, n_gaps, n_pam;
  uint64_t rows;               /* == n_rows of calitas_search_hits == the sum of counts */
  uint64_t* counts;            /* [2][n_mm][n_gaps][n_pam] */
} calitas_counts_t;

/* calitas_search_hits without the text: the table alone.  The alignments never leave the device and no row is built -- behind
 * removeOverlaps one kernel counts the kept hits into a histogram per workgroup and the few KB of the table reach the host with the
 * counters the call waits for anyway.  Accepts whatever calitas_search_hits accepts (the whole reference, chrom_index, a window range);
 * where a device stage declines, the host stages of calitas_hits_counts finish the call. */
int calitas_search_counts(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, calitas_counts_t** out);
/* ... for a batch of guides, pipelined through the lanes as in calitas_search_hits_batch (same same-length rule, same meaning of a
 * window range): out[i] receives the table of guides[i], each freed with calitas_free. */
int calitas_search_counts_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                calitas_counts_t** out);

/* Guide sites ---------------------------------------------------------------------------------------------------- */

/* One place of the resident reference where a guide can be cut out: an exact match of an IUPAC pattern.  The pattern is a
 * calitas_guide_t read as a pattern: protospacer of any IUPAC letters (NNNNNNNNNNNNNNNNNNNN is the usual case), 0..8 PAMs of any
 * lengths, pam_is_5prime as in a guide, cli_length ignored.  In strand space PAM k's pattern is protospacer + pam_k (3' PAM),
 * pam_k + protospacer (5' PAM) or the protospacer alone; a site is a (contig, strand, protospacer position) where some PAM's pattern
 * matches the text read on that strand ('-': the reverse complement of the footprint), every base of the footprint being a plain
 * A C G T (either case) or U and lying in the IUPAC set of its pattern letter.  pam_index is the first PAM that matches; there is
 * one record per (contig, strand, protospacer start), never one per PAM.
 * Not a `-d 0` search: a search lets an ambiguity code of the REFERENCE (an R in the FASTA) pair with a compatible guide base; a site
 * never contains one (nor an N, nor padding), because a guide cut from it would not be an ACGT guide. */
typedef struct {
  int32_t contig_index;
  int32_t protospacer_start;   /* leftmost base of the protospacer, forward coordinates, 0-based */
  int32_t pam_start;           /* leftmost base of the matched PAM, forward coordinates; -1 for a PAM-less pattern */
  int8_t strand;               /* '+' or '-' */
  int8_t pam_index;            /* -1 for a PAM-less pattern */
  uint8_t pam_length;
  uint8_t protospacer_length;
} calitas_site_t;

/* All sites of `pattern` in a region, sorted by contig_index, protospacer_start, '+' before '-'; the same bytes from call to call.
 * Region: chrom_index (< 0: every contig) and [start, end) in 0-based contig coordinates, end == 0 meaning the contig's end (with
 * chrom_index < 0 the bounds apply to every contig, cut to its length); a site counts when its whole footprint -- protospacer plus
 * the matching PAM -- lies inside, and a PAM whose footprint would leave the region does not match there.  A region that needs an
 * absent contig fails with CALITAS_EINVAL, as a search does.  Runs on the device: one kernel matches 32 start positions per lane on the
 * bit-planes the scan streams, in two passes (count, then write at scanned offsets: no sort).  sites == NULL: *n_sites only, after the
 * first pass.  *sites is one block for calitas_free.  No reference counterpart. */
int calitas_find_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t chrom_index, uint64_t start, uint64_t end,
                       calitas_site_t** sites, uint64_t* n_sites);
/* The first pass alone: *n_sites and, when per_contig_strand is not NULL, the sites per contig and strand ([n_contigs][2], '+'
 * first; contigs outside the region get 0).  No reference counterpart. */
int calitas_count_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t chrom_index, uint64_t start, uint64_t end,
                        uint64_t* per_contig_strand, uint64_t* n_sites);
/* The host twin of calitas_find_sites: the same records from a base-by-base walk over the packed reference of the context, which may
 * be host-only (calitas_create(-1)) -- the second implementation the tests hold the kernel against.  No reference counterpart. */
int calitas_find_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t chrom_index, uint64_t start, uint64_t end,
                            calitas_site_t** sites, uint64_t* n_sites);

/* A site filter: which of a pattern's sites are guides worth ordering.  It applies to the PROTOSPACER of a site as it reads on the site's
 * strand (upper case, U as T, L = its length) and to nothing else -- not the PAM, not the flanks -- so the verdict does not depend on
 * which PAM matched.  A site is kept when all of these hold:
 *   GC      gc_min <= (number of G and C among the L bases) <= gc_max; a gc_max above L means L.
 *   runs    for each base b of A C G T with max_run[b] > 0 the protospacer holds no run of b longer than max_run[b].  Only bases inside
 *           the protospacer count: a run that goes on into the PAM or the flank is cut at the protospacer's edge.  A limit >= L is legal
 *           and rejects nothing.
 *   motifs  none of the n_motifs IUPAC motifs matches anywhere entirely inside the protospacer: each is 1 .. 16 letters, at most L, read in
 *           the guide's orientation; a guide base matches a letter when it lies in the letter's IUPAC set.  No reverse complement is
 *           added: pass both orientations to avoid both.
 * CALITAS_EINVAL, with a message that names the field: gc_min > min(gc_max, L); n_motifs > 8; a motif that is empty, longer than L, made
 * of N only or holds a non-IUPAC letter; reserved != 0.  A filter that rejects every site returns none. */
typedef struct {
  uint8_t gc_min, gc_max;     /* counts of G + C among the protospacer's bases, inclusive; {0, 255}: no bound */
  uint8_t max_run[4];         /* A C G T as the guide reads; 0: no limit */
  uint8_t n_motifs;           /* 0..8 */
  uint8_t reserved;           /* 0 */
  char motifs[8][16];         /* IUPAC letters, either case, NUL-padded */
} calitas_site_filter_t;

/* calitas_find_sites, calitas_count_sites and calitas_find_sites_host with a filter: the records of the unfiltered listing that pass, in
 * its order and with its pam_index, and the counts of those alone; every other argument as there.  filter == NULL is the unfiltered
 * call.  On the device the filter is part of the kernel's match (bit-parallel over the planes it holds already): nothing is listed and
 * dropped.  No reference counterpart. */
int calitas_find_sites_filtered(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index,
                                uint64_t start, uint64_t end, calitas_site_t** sites, uint64_t* n_sites);
int calitas_count_sites_filtered(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index,
                                 uint64_t start, uint64_t end, uint64_t* per_contig_strand, uint64_t* n_sites);
int calitas_find_sites_filtered_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                     int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, uint64_t* n_sites);

/* Copies: how often a guide's protospacer -- or its PAM-proximal seed -- stands next to a PAM of the pattern, exactly.  The KEY of a site
 * is its protospacer as the guide reads it on the site's strand (upper case, U as T, L bases: what a guide cut from the site is made
 * of), cut to its PAM-proximal K bases: the last K for a 3' PAM and for a PAM-less pattern, the first K for a 5' PAM; K = L is the
 * whole protospacer.  The PAM is no part of the key: copies next to different PAMs of the pattern count alike.
 * copies[i] is the number of sites the unfiltered calitas_count_sites(pattern, chrom_index, start, end) counts whose key equals query i
 * -- the region rules, absent contigs, one site per (contig, strand, protospacer start) and a U in the footprint as there -- so a guide
 * cut from the resident reference has at least 1, itself.  queries: n_queries * K letters A C G T in either case (U as T), one query
 * after the other without terminators; key_length: K, 0 meaning L.  Duplicated queries each get the full count; a query no site carries
 * gets 0, one the pattern's own protospacer letters exclude among them; n_queries == 0 is legal.  Counts are 64-bit integers added in
 * any order: every path gives the same numbers, and the counts of disjoint contig sets add up element by element.
 * CALITAS_EINVAL, with a message that names the field or the query's index: key_length < 0 or > L; n_queries above 16777216 (2^24; the
 * queries are independent: count them in pieces); a query letter outside ACGTUacgtu; and what calitas_count_sites refuses.
 * Runs on the device: one pass of calitas_count_sites' match, every site's key looked up in a hash table of the distinct queries, one
 * copy-back of their counters.  CALITAS_ENODEV on a host-only context.  No reference counterpart. */
int calitas_count_copies(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start, uint64_t end,
                         const char* queries, uint64_t n_queries, uint64_t* copies);
/* The host twin of calitas_count_copies: the same numbers from a base-by-base walk over the packed reference of the context, which may
 * be host-only -- the second implementation the tests hold the kernel against.  No reference counterpart. */
int calitas_count_copies_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start,
                              uint64_t end, const char* queries, uint64_t n_queries, uint64_t* copies);

/* Near copies: how often a guide's protospacer -- or its seed -- stands next to a PAM of the pattern with up to M = max_mismatches
 * substitutions, 0 <= M <= CALITAS_NEAR_MAX_MISMATCHES.  Key, K, key_length (0 = L), the queries' letters, the region rules, absent contigs,
 * one site per (contig, strand, protospacer start) and a U in the footprint are exactly those of calitas_count_copies, and the sites
 * are those the unfiltered calitas_count_sites(pattern, chrom_index, start, end) counts.  K >= M + 1.
 * near has n_queries * (M + 1) entries: near[i * (M + 1) + d] is the number of sites whose key differs from query i at exactly d of
 * its K positions, d = 0 .. M -- a Hamming count over the key.  The PAM is no part of the key: any PAM of the pattern qualifies a site,
 * and it has to match the pattern as it does for calitas_find_sites (no PAM mismatches).  There are no gaps, and overlapping sites
 * are not merged (no removeOverlaps): this is not calitas_search's gapped alignment, which remains the tool for that question.
 * What holds: column 0 (d = 0) equals calitas_count_copies of the same arguments; duplicated queries each get the full row; a site
 * counts for every query it is near, so two queries one substitution apart see each other's sites in column 1; the counts of disjoint
 * contig sets add up element by element; counts are 64-bit integers added in any order, so every path returns the same numbers.
 * CALITAS_EINVAL, with a message that names the field or the query's index: max_mismatches outside 0 .. 3; key_length (K) below
 * max_mismatches + 1; and what calitas_count_copies refuses, its limit of 16777216 (2^24) queries among them.
 * Runs on the device: one pass of calitas_count_sites' match; the key is cut into M + 1 pieces, of which M substitutions leave one
 * untouched, and every site's key is held against the distinct queries that share a piece with it (a directly addressed bucket table
 * per piece, no hash table); one copy-back of the counters.  CALITAS_ENOMEM when the tables do not fit the device.  CALITAS_ENODEV on a
 * host-only context.  No reference counterpart. */
#define CALITAS_NEAR_MAX_MISMATCHES 3
int calitas_count_near(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index,
                       uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near);
/* The host twin of calitas_count_near: the same numbers from a base-by-base walk over the packed reference of the context, which may be
 * host-only, every site's key compared with every distinct query by plain Hamming distance (no buckets) -- the second implementation
 * the tests hold the kernel against; its cost is sites x distinct queries.  No reference counterpart. */
int calitas_count_near_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index,
                            uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near);

/* The specificity score of a guide: one number per off-target hit, summed per guide.  No reference counterpart.
 * A model for protospacers of L bases holds Q16 factors (65536 = 1.0, none above it): mismatch[L][5][5] indexed by guide position,
 * guide letter and target letter, one gap factor and one pam_mismatch factor.  Guide positions are 0-based and count the upper-case
 * letters of the guide as written on the command line, left to right; the letter index is A 0, C 1, G 2, T 3, anything else 4 (U, N
 * and the IUPAC codes alike), for both letters.  The score of one hit is defined on its hits.txt row:
 *     s = 1 << 32
 *     for each column, left to right, whose padded_guide letter is upper case (i = its index among them):
 *         if padded_alignment is '.':  s = (s * mismatch[i][idx(padded_guide)][idx(padded_target)]) >> 16
 *     repeat guide_gaps times:  s = (s * gap) >> 16
 *     repeat pam_mm times:      s = (s * pam_mismatch) >> 16
 * in 64-bit unsigned arithmetic, truncating at every step: the order is part of the contract, and every implementation (the device
 * kernels, the host stage, a reader of the text) gives the same integers.  A hit with total_mm_plus_gaps == 0 is perfect (the guide's
 * own site and its exact copies): counted, not scored.  The library ships no published weight table, only the mechanism. */
typedef struct {
  int32_t protospacer_length;  /* L: must be the guide's */
  uint32_t gap;
  uint32_t pam_mismatch;
  const uint32_t* mismatch;    /* [L][5][5] */
} calitas_score_model_t;

/* What a guide's hits add up to.  Across window ranges, contigs and ranks of one job rows, perfect, sum_q32 and the table add and
 * max_q32 takes the maximum; specificity = 2^32 / (2^32 + sum_q32), in double on the host.  The struct, table.counts included, is one
 * block: one calitas_free. */
typedef struct {
  uint64_t rows;               /* all hits == n_rows of calitas_search_hits */
  uint64_t perfect;            /* hits with total_mm_plus_gaps == 0 */
  uint64_t sum_q32;            /* the sum of s over the other hits */
  uint64_t max_q32;            /* the largest such s, 0 when there is none */
  calitas_counts_t table;      /* the table of calitas_search_counts, from the same pass */
} calitas_scores_t;

/* calitas_search_counts plus the score.  No reference counterpart.  Behind removeOverlaps one lane per kept hit reads the hit's
 * mismatch columns, fetches the reference base under each, looks the pair up in the model and the sums are reduced per workgroup; a
 * few words cross PCIe.  Accepts whatever calitas_search_counts accepts (the whole reference, chrom_index, a window range).
 * CALITAS_EINVAL for a model of another length than the guide's protospacer, a factor above 65536 or a NULL table.  Where a device
 * stage declines, the host stage of calitas_hits_scores finishes the call. */
int calitas_search_scores(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                          calitas_scores_t** out);
/* ... for a batch of guides.  No reference counterpart.  It follows the rules of calitas_search_counts_batch: all guides have one length, so
 * one model serves them; out[i] receives the block of guides[i], each freed with calitas_free. */
int calitas_search_scores_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                const calitas_score_model_t* model, calitas_scores_t** out);

/* Near copies with the score: calitas_count_near over the whole protospacer, and per query what its near copies add up to under a
 * model -- for all guides of a table in the one genome pass.  No reference counterpart.
 * Sites, region rules, absent contigs, one site per (contig, strand, protospacer start), a U in the footprint, the queries' letters and
 * the limit of 2^24 queries are those of calitas_count_near.  The key is always the whole protospacer (K = L; there is no key_length:
 * a score over a seed has no meaning in the model), so queries holds n_queries * L letters.  near receives exactly what
 * calitas_count_near(pattern, 0, M, ...) returns, n_queries * (M + 1) counts from the same pass.
 * The score of one (site, query) pair at d >= 1:
 *     s = 1 << 32
 *     for each position i at which the two differ, in ascending guide position:
 *         s = (s * mismatch[i][idx(query letter)][idx(site letter)]) >> 16
 * in 64-bit unsigned arithmetic, truncating at every step; i is 0-based in the guide as written on the command line.  That is the
 * contract of calitas_score_model_t on a substitution-only row without a PAM mismatch: model->gap and model->pam_mismatch are not used.
 * Both letters are plain bases, indices 0 .. 3, and a U in a query is a T (index 3) as in every copies call -- the ONE difference from
 * the search's contract, which reads a U guide letter as index 4.
 * scores[i].sum_q32 is the sum of s over query i's sites at d = 1 .. M, scores[i].max_q32 the largest such s, 0 when there is none.
 * Sites at d = 0 are counted in near[i * (M + 1)] and not scored (the perfect hits of calitas_scores_t).  A factor of 0 gives s = 0:
 * the pair is counted, adds nothing to the sum and leaves the maximum as it is.  Duplicated queries each get the full result; over
 * disjoint contig sets counts and sums add and the maxima take the maximum; every path returns the same integers.  A sum wraps only
 * past 2^32 scored sites of one query (each s is at most 2^32).
 * CALITAS_EINVAL, with a message that names the field: what calitas_count_near refuses, in its order (the protospacer has at least
 * M + 1 bases); then a NULL model or table, model->protospacer_length != L and a mismatch factor above 65536, with the messages of
 * calitas_search_scores.  n_queries == 0 is legal.
 * Runs on the device: the near kernel's pass; a member that counts at d >= 1 walks its at most three differing positions, looks each
 * factor up in the model's 4 x 4 plain-base blocks (2 KB, in LDS) and adds s into the query's sum and maximum beside its count.
 * CALITAS_ENOMEM when the tables do not fit the device, CALITAS_ENODEV on a host-only context. */
typedef struct { uint64_t sum_q32, max_q32; } calitas_near_score_t;
int calitas_score_near(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                       int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near,
                       calitas_near_score_t* scores);
/* The host twin of calitas_score_near: a base-by-base walk over the packed reference of the context, which may be host-only; plain
 * Hamming distances against every distinct query, the score letter by letter from the caller's table.  No reference counterpart. */
int calitas_score_near_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                            int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near,
                            calitas_near_score_t* scores);

/* Near copies listed: WHERE every query's copies within M substitutions stand.  No reference counterpart.
 * Sites, region rules, absent contigs, one site per (contig, strand, protospacer start), the queries' letters (U as T), the key (the
 * whole protospacer: queries holds n_queries * L letters) and the limit of 2^24 queries are those of calitas_score_near; near receives
 * exactly what calitas_count_near(pattern, 0, M, ...) returns.
 * Query q's records are (*hits)[offsets[q] .. offsets[q + 1]); offsets has n_queries + 1 entries and is non-decreasing, *n_hits is its
 * last one.  A stretch holds one record for every (site, query) pair at d = 0 .. M -- d = 0 included: the guide's own site and its exact
 * copies -- ordered by contig_index, then protospacer_start, then '+' before '-'.  That order is total within a stretch, so the device,
 * the host twin and repeated calls return the same bytes.  A query whose row of near sums to more than `limit` (1 ..
 * CALITAS_NEAR_LIST_MAX) lists nothing: its stretch is empty, and its row of near says why.  Duplicated queries each get the full stretch.
 * score_q32 is the pair's score as calitas_score_near defines it, 1 << 32 at d = 0; model == NULL means no weights: every score is
 * 1 << 32.  Over disjoint contig sets a query's lists concatenate in contig order (and a query over the limit in the sum lists nothing).
 * *hits is one block for calitas_free, also when it holds no record; n_queries == 0 is legal.
 * CALITAS_EINVAL, with a message that names the field: what calitas_score_near refuses, in its order, except that a NULL model is
 * legal; then a limit outside 1 .. CALITAS_NEAR_LIST_MAX.
 * Runs on the device: the near kernel's pass once for the counts; the host lays a stretch per distinct query out of them; the pass
 * again, every pair that counts storing its record at a slot it takes from its query's cursor; a small kernel that puts every stretch
 * in position order by ranking; one copy-back.  Stretches next to a U in the reference are corrected on the host.
 * CALITAS_ENOMEM when the records or the tables do not fit, CALITAS_ENODEV on a host-only context. */
#define CALITAS_NEAR_LIST_MAX 4096
typedef struct {                 /* 32 bytes */
  uint64_t score_q32;
  int32_t  contig_index;
  int32_t  protospacer_start;    /* leftmost base, forward coordinates, 0-based: calitas_site_t's */
  uint32_t target_lo, target_hi; /* the site's protospacer as the guide reads it, as bit-planes: bit i of target_lo / target_hi = low / high
                                    bit of the code of guide position i (A 0, C 1, G 2, T 3) */
  uint32_t diff_mask;            /* bit i: guide position i differs from the query */
  int8_t   strand;               /* '+' or '-' */
  int8_t   pam_index;            /* the first PAM that matches; -1 for a PAM-less pattern */
  uint8_t  mismatches;           /* popcount(diff_mask), 0 .. M */
  uint8_t  reserved;             /* 0 */
} calitas_near_hit_t;
int calitas_list_near(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model /* may be NULL */,
                      int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit,
                      uint64_t* near /* n_queries * (M + 1) */, uint64_t* offsets /* n_queries + 1 */, calitas_near_hit_t** hits, uint64_t* n_hits);
/* The host twin of calitas_list_near: the base-by-base walk of calitas_score_near_host, every pair a record, every stretch through
 * std::sort; also on a host-only context.  No reference counterpart. */
int calitas_list_near_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                           int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit,
                           uint64_t* near, uint64_t* offsets, calitas_near_hit_t** hits, uint64_t* n_hits);

/* On-target activity: how well a guide cut from a site is expected to cut, from the site's sequence context under a linear model.
 * The CONTEXT of a site is W = up + L + down letters as the guide reads: `up` bases 5' of the protospacer, its L bases, `down` bases
 * 3' of it.  With p the record's protospacer_start it is the forward bases [p - up, p + L + down) on '+' and the reverse complement of
 * the forward bases [p - down, p + L + up) on '-'.  The model knows nothing of PAMs: for an ...nrg pattern and down = 6 the context holds
 * the PAM and three bases behind it, for a 5' PAM the PAM lies in `up`; a site matched by an auxiliary PAM of another length is scored
 * over the same window.
 * A site is scored when the window lies inside its contig -- the contig bounds it, not the region, which bounds footprints as in
 * calitas_find_sites -- and every base of it is a plain A C G T, in either case, or a U (read as T).  Otherwise its score is
 * CALITAS_ACTIVITY_NONE.  With c_i the code of context letter i (A 0, C 1, G 2, T 3) the score is
 *   intercept + sum_i single[i][c_i] + sum_{i < W - 1} pair[i][4 c_i + c_{i+1}] + gc[number of G and C among the L protospacer bases]
 * in 32-bit signed integers, all Q16 (65536 = 1.0).  Every weight lies within +-CALITAS_ACTIVITY_MAX_WEIGHT and there are at most
 * 2 * 64 + 1 terms, so the sum stays below 2^28 in magnitude: it never overflows and never equals CALITAS_ACTIVITY_NONE.  Integer
 * addition has no order, so the kernel, the host twin and a plain loop give the same numbers.  `link` says how a tool prints the score
 * (0: score / 65536, 1: 1 / (1 + exp(-score / 65536))) and changes nothing else.  The library ships the mechanism and a file format
 * (models/example_activity30.tsv), no published weight table. */
#define CALITAS_ACTIVITY_NONE INT32_MIN       /* this site has no score */
#define CALITAS_ACTIVITY_MAX_FLANK 16
#define CALITAS_ACTIVITY_MAX_WEIGHT 1048576   /* |weight| <= 16.0 in Q16 */
typedef struct {
  int32_t protospacer_length;   /* L: must be the pattern's */
  int32_t up, down;             /* bases 5' and 3' of the protospacer AS THE GUIDE READS, 0 .. 16 each; W = up + L + down <= 64 */
  int32_t link;                 /* 0 identity, 1 logistic: how a tool prints the score, nothing else */
  int32_t intercept;            /* Q16, signed */
  const int32_t* single;        /* [W][4]      position in the context, base A C G T */
  const int32_t* pair;          /* [W - 1][16] position i, 4 * base(i) + base(i + 1) */
  const int32_t* gc;            /* [L + 1]     by the protospacer's G + C count */
} calitas_activity_model_t;
/* The records of calitas_find_sites_filtered(pattern, filter, ...) whose score is >= min_score_q16, in that call's order and with its
 * bytes; scores[i] belongs to sites[i].  min_score_q16 == CALITAS_ACTIVITY_NONE keeps every site, the unscored ones carrying
 * CALITAS_ACTIVITY_NONE; any other threshold drops the unscored ones as well (one signed comparison says all of this).
 * sites == NULL && scores == NULL: *n_sites only.  Each block takes one calitas_free.
 * On the device the records of the site kernel's two passes stay where they are: one lane per record scores its window from the
 * bit-planes (the model's tables in LDS), and with a threshold a second kernel compacts records and scores in order (ranks from
 * ballots: no sort, no returning atomic) before the one copy-back.  Windows with an exception base -- a U among them, which the
 * device cannot tell from an N -- are decided on the host.
 * Errors, in this order: what calitas_find_sites_filtered refuses; CALITAS_EINVAL, with a message that names the field, for a NULL
 * model or table, a protospacer_length other than the pattern's, up or down outside 0 .. 16, link outside 0 .. 1, intercept or a weight
 * outside +-CALITAS_ACTIVITY_MAX_WEIGHT; CALITAS_ENODEV on a host-only context; CALITAS_ENOMEM when records and scores do not fit the
 * device.  No reference counterpart. */
int calitas_find_sites_scored(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter /* may be NULL */,
                              const calitas_activity_model_t* model, int32_t min_score_q16, int32_t chrom_index, uint64_t start, uint64_t end,
                              calitas_site_t** sites, int32_t** scores, uint64_t* n_sites);
/* The host twin of calitas_find_sites_scored: calitas_find_sites_filtered_host's records, each scored base by base; also on a host-only
 * context.  No reference counterpart. */
int calitas_find_sites_scored_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                   const calitas_activity_model_t* model, int32_t min_score_q16, int32_t chrom_index, uint64_t start,
                                   uint64_t end, calitas_site_t** sites, int32_t** scores, uint64_t* n_sites);

/* The K highest-scoring imperfect hits of a guide, from the pass that scores them.  No reference counterpart.
 * The candidates are the kept hits that are not perfect (total_mm_plus_gaps != 0); they are ordered by score_q32 descending, and among
 * equal scores the hit whose row comes earlier in the hits.txt of the same call comes first.  That is a total order: the n records are
 * the same bytes from call to call and on every path (per-bin kernels, general kernels, host stage).  For consecutive pieces of one
 * job (window ranges, contigs, ranks in order) the top of the whole is the first k of a stable merge of the pieces' lists by score,
 * pieces in their order -- the texts of the pieces concatenate. */
#define CALITAS_TOP_MAX 256
typedef struct {
  uint64_t score_q32;          /* the row's score under the model (calitas_score_model_t contract): 1 .. 2^32, or 0 where a factor is 0 */
  int32_t contig_index;
  int32_t coordinate_start;    /* the integers of the row's coordinate_start / coordinate_end columns */
  int32_t coordinate_end;
  int8_t strand;               /* '+' or '-' */
  uint8_t guide_mm, guide_gaps, pam_mm;   /* the row's columns of these names */
} calitas_top_hit_t;
#ifdef __cplusplus
static_assert(sizeof(calitas_top_hit_t) == 24, "calitas_top_hit_t is 24 bytes");
#else
_Static_assert(sizeof(calitas_top_hit_t) == 24, "calitas_top_hit_t is 24 bytes");
#endif
typedef struct {
  calitas_scores_t scores;     /* exactly what calitas_search_scores returns for the same arguments */
  uint32_t k;                  /* as asked */
  uint32_t n;                  /* records returned = min(k, scores.rows - scores.perfect) */
  calitas_top_hit_t* hits;     /* n records, best first */
} calitas_top_t;               /* one block: one calitas_free */

/* calitas_search_scores plus the list.  CALITAS_EINVAL for k == 0, k > CALITAS_TOP_MAX and everything calitas_search_scores refuses;
 * accepts whatever it accepts (the whole reference, chrom_index, a window range, ownership applied as there).  The selection runs in
 * the lanes that score the hits (top_kernel / bin_top_kernel); at most k records of 24 bytes cross PCIe besides the scores.  Where a
 * device stage declines, the host stage of calitas_hits_top finishes the call. */
int calitas_search_top(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                       uint32_t k, calitas_top_t** out);
/* ... for a batch of guides, with the rules of calitas_search_scores_batch.  No reference counterpart. */
int calitas_search_top_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                             const calitas_score_model_t* model, uint32_t k, calitas_top_t** out);

/* A guide's scores and top list split by annotated regions.  No reference counterpart.
 * calitas_set_regions gives the context a set of intervals, each with a class 1 .. n_classes - 1 (2 <= n_classes <=
 * CALITAS_REGION_CLASSES_MAX); [start, end) is 0-based and half-open in the contig's coordinates, like BED.  Intervals come in any
 * order and may overlap or nest.  n == 0 clears the set; calitas_set_reference* and calitas_load_index clear it too.  Works on a
 * host-only context.  CALITAS_EINVAL for a bad contig index, start >= end, an end beyond the contig, an interval on an absent contig
 * and a class out of range.  The set is flattened once here and brought to the device once, not per call.
 *
 * The class of a hit is defined on its hits.txt row: the hit occupies [coordinate_start, coordinate_end) of its chromosome (the
 * protospacer, as those two columns give it; half-open), and its class is the smallest cls among the intervals of that contig with
 * start < coordinate_end && end > coordinate_start -- 0 ("elsewhere") when there is none or the extent is empty.  Every hit has
 * exactly one class. */
#define CALITAS_REGION_CLASSES_MAX 8
typedef struct {
  int32_t contig_index;
  int32_t start, end;
  uint32_t cls;
} calitas_region_t;
int calitas_set_regions(calitas_ctx* ctx, uint64_t n, const calitas_region_t* iv, uint32_t n_classes);

typedef struct {
  calitas_top_t top;           /* top.scores: exactly what calitas_search_scores returns for the same arguments; top.hits: the
                                  n = min(k, candidates) best imperfect hits whose class has its bit set in list_mask, in the order
                                  of the calitas_top_t contract (score descending, then the earlier row) */
  uint8_t* hit_class;          /* top.n bytes: the class of every record */
  uint32_t n_classes;
  uint32_t list_mask;          /* as asked */
  calitas_scores_t* by_class;  /* n_classes entries: rows, perfect, sum_q32, max_q32 and an own counts table, of the hits of that class */
} calitas_regions_t;           /* one block: one calitas_free */

/* calitas_search_top split by the context's regions, with the rules of calitas_search_top (the whole reference, chrom_index, a
 * window range with ownership).  k is 0 .. CALITAS_TOP_MAX; k == 0 means no list.  With k > 0 a list_mask without a bit below
 * n_classes is CALITAS_EINVAL; higher bits are ignored.  CALITAS_EINVAL when the context has no regions and for everything
 * calitas_search_top refuses.  Invariants: the by_class entries sum, field by field and cell by cell, to top.scores (max_q32 is their
 * maximum); with every bit set in list_mask, top equals calitas_search_top's result.  Across consecutive pieces of a job by_class
 * adds (max_q32 takes the maximum) and the lists merge stably as calitas_top_t's do; hit_class travels with its records.  The class
 * lookup and the selection run in the lanes that score the hits (regions_kernel / bin_regions_kernel). */
int calitas_search_regions(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                           uint32_t k, uint32_t list_mask, calitas_regions_t** out);
int calitas_search_regions_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                 const calitas_score_model_t* model, uint32_t k, uint32_t list_mask, calitas_regions_t** out);

/* Guide sites by annotated regions: which of a pattern's sites lie where the caller wants to cut.  No reference counterpart.
 * THE CLASS OF A SITE.  Positions ext_from .. ext_to - 1 of the protospacer are counted as the guide reads it, 0 its 5' base,
 * 0 <= ext_from < ext_to <= L; {0, 0} means {0, L}, the whole protospacer.  With p the record's protospacer_start they are the forward
 * bases [p + ext_from, p + ext_to) on '+' and [p + L - ext_to, p + L - ext_from) on '-'.  The site's class is the smallest cls among
 * the intervals of its contig that overlap that extent, 0 when there is none: the rule calitas_search_regions classes a hit by.
 * {16, 18} on a 20-mer with a 3' PAM is the two bases beside the Cas9 cut, {k, k + 1} one base; the PAM is never part of the extent. */
typedef struct {
  uint32_t class_mask;         /* bit c: keep the sites of class c (0 = elsewhere).  Bits >= n_classes are ignored. */
  uint8_t ext_from, ext_to;    /* the part of the protospacer that is classed; {0, 0} means {0, L} */
  uint16_t reserved;           /* 0 */
} calitas_site_regions_t;
/* The records of calitas_find_sites_filtered(pattern, filter, chrom_index, start, end) whose class has its bit in opt->class_mask, in
 * that call's order and with its bytes; classes[i] is the class of sites[i].  sites == NULL && classes == NULL: *n_sites only.  Each
 * block takes one calitas_free.  With every bit below n_classes set, sites is the filtered listing byte for byte; masks that partition
 * the classes partition the records.
 * On the device the site kernel's two passes skip every segment of 8192 bases that no wanted class comes near -- a table of one byte
 * per segment, made from the flattened set at the first such call and kept on the context, decides before a word is loaded -- then one
 * lane per record classes its extent, and a second kernel compacts records and classes in order (ranks from ballots: no sort, no
 * returning atomic) before the one copy-back.  Sites beside a U are classed on the host, as calitas_find_sites finds them there.
 * Errors, in this order: CALITAS_ENODEV on a host-only context (the device calls); what calitas_find_sites_filtered refuses;
 * CALITAS_EINVAL, with a message that names the field, for a NULL opt, a context without regions, a class_mask without a bit below
 * n_classes, ext_from >= ext_to or ext_to > L other than {0, 0}, reserved != 0. */
int calitas_find_sites_regions(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter /* may be NULL */,
                               const calitas_site_regions_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                               uint8_t** classes, uint64_t* n_sites);
/* The same chain without the records: *n_sites and, when per_class_strand is not NULL, the kept sites per class and strand
 * ([n_classes][2], '+' first; the cells of classes outside the mask are 0, and the cells sum to *n_sites). */
int calitas_count_sites_regions(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_regions_t* opt,
                                int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* per_class_strand, uint64_t* n_sites);
/* The host twins: calitas_find_sites_filtered_host's records, each classed through the host's flattened set; also on a host-only
 * context. */
int calitas_find_sites_regions_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                    const calitas_site_regions_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                    uint8_t** classes, uint64_t* n_sites);
int calitas_count_sites_regions_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                     const calitas_site_regions_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* per_class_strand,
                                     uint64_t* n_sites);
/* (test hook) A copy of the presence table the regions listing skips by, made if need be; needs no device.  bytes[i] belongs to the
 * 256 words of the packed space from word *first_word + 256 i on (calitas_contig_packed_base gives a contig's first base there): bit c
 * is set when a base of class c of the segment's contig -- bit 0: a base of no interval -- lies within 48 bases (the longest footprint)
 * of the segment.  *bytes is one block for calitas_free.  CALITAS_EINVAL when the context has no regions. */
int calitas_site_presence(const calitas_ctx* ctx, uint8_t** bytes, uint64_t* n, uint64_t* first_word);

/* Guide sites in pairs: which two sites of a pattern can be used together -- paired nickases (opposite strands, PAMs facing outwards,
 * cuts a few tens of bases apart) or an excision (two cuts a chosen distance apart).  No reference counterpart.
 * THE LISTING.  The records of calitas_find_sites_filtered(pattern, filter, chrom_index, start, end) in its order; site i is the record
 * at index i.  L is the protospacer's length.
 * THE CUT OF A SITE.  cut_offset = c, 0 .. L, is a position in the protospacer as the guide reads it (as ext_from / ext_to above):
 * cut = protospacer_start + c on '+' and protospacer_start + L - c on '-'.  c = L - 3 with a 3' PAM is the Cas9 cut.
 * A PAIR.  Two different sites i < j of one contig with min_distance <= |cut_j - cut_i| <= max_distance whose orientation has its bit in
 * `orientations`.  The left member is the one with the smaller cut, at equal cuts the one with the smaller index;
 * distance = cut_right - cut_left >= 0; orientation = (left is '-') + 2 (right is '-'): 0 "++", 1 "-+" (PAM-out for a 3' PAM), 2 "+-"
 * (PAM-in for a 3' PAM, PAM-out for a 5' PAM), 3 "--".  Sites of different contigs never pair, a site never pairs with itself; two
 * records at one protospacer_start on opposite strands are two sites and may pair.
 * THE ORDER.  Pairs come ordered by (i, j), that is by (min(left, right), max(left, right)): a total order, so the device, the host
 * twin and repeated calls return the same bytes. */
#define CALITAS_PAIR_MAX_DISTANCE 65535
typedef struct {
  int32_t min_distance, max_distance;   /* 0 <= min_distance <= max_distance <= CALITAS_PAIR_MAX_DISTANCE */
  uint8_t cut_offset;                   /* 0 .. L */
  uint8_t orientations;                 /* bit o: pairs of orientation o; 1 .. 15 */
  uint8_t reserved[2];                  /* 0 */
} calitas_site_pairs_t;
typedef struct {
  uint32_t left, right;                 /* indices into the listing */
  int32_t distance;
  uint8_t orientation;
  uint8_t reserved[3];                  /* 0 */
} calitas_site_pair_t;
/* *sites: the listing, exactly the bytes of calitas_find_sites_filtered; *pairs: its pairs under opt.  Each is one block for
 * calitas_free.  On the device the site kernel's two passes leave the records in device memory; one lane per record walks the records
 * behind it -- up to the first whose start is more than max_distance + |L - 2c| beyond its own, from the first, found by bisection,
 * that min_distance does not rule out -- and counts its partners; after a scan of the workgroups' sums the same walk stores every pair
 * at its place (no sort, no returning atomic), and the records and the pairs are copied back once each.  When the reference has a U
 * beside a site of the region the listing is corrected on the host as calitas_find_sites corrects it and the pairs are made there, by
 * the host twin's walk over the final listing.
 * Errors, in this order: CALITAS_ENODEV on a host-only context (the device calls); what calitas_find_sites_filtered refuses;
 * CALITAS_EINVAL, with a message that names the field, for a NULL opt, orientations of 0 or above 15, reserved != 0, min_distance < 0,
 * min_distance > max_distance, max_distance > CALITAS_PAIR_MAX_DISTANCE, cut_offset > L, and for a listing of 2^32 sites or more (pair
 * the region in pieces); CALITAS_ENOMEM when the records do not fit the device. */
int calitas_find_site_pairs(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter /* may be NULL */,
                            const calitas_site_pairs_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                            uint64_t* n_sites, calitas_site_pair_t** pairs, uint64_t* n_pairs);
/* The same chain without the blocks: *n_sites, *n_pairs and, when per_orientation is not NULL, the pairs per orientation ([4]; they
 * sum to *n_pairs).  Neither records nor pairs are copied back. */
int calitas_count_site_pairs(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_pairs_t* opt,
                             int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* n_sites, uint64_t* n_pairs,
                             uint64_t* per_orientation /* [4], may be NULL */);
/* The host twins: calitas_find_sites_filtered_host's records and one walk over them; also on a host-only context. */
int calitas_find_site_pairs_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                 const calitas_site_pairs_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                 uint64_t* n_sites, calitas_site_pair_t** pairs, uint64_t* n_pairs);
int calitas_count_site_pairs_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                  const calitas_site_pairs_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* n_sites,
                                  uint64_t* n_pairs, uint64_t* per_orientation);

/* Allele-specific guide sites: the sites a single-nucleotide variant creates, destroys or changes -- a PAM that exists on one allele
 * only, a protospacer that differs by the variant's base.  No reference counterpart.
 * A SNV.  One base of a contig replaced by `alt`; `ref`, when not 0, is held against the reference's base.  Letters are A C G T U in
 * either case; a U reads as T.
 * A RECORD.  For SNV i and an allele X of {ref, alt} let site_X(p, s) be the record calitas_find_sites(pattern, the whole contig) would
 * list at protospacer start p on strand s if the contig carried X's base at `position` (the first matching PAM wins, a base that is not
 * A C G T U is in no footprint, a footprint that leaves the contig is no site), or none.  A record is written for (i, p, s) when
 * `position` lies in the footprint -- the protospacer plus the matched PAM -- of site_ref(p, s) or of site_alt(p, s); then
 * kind = (site_alt exists) + 2 (site_ref exists), `site` is site_alt where it exists and site_ref otherwise, guide_lo / guide_hi hold
 * the protospacer of that allele as the guide reads it, and guide_offset is position - p on '+' and p + L - 1 - position on '-'
 * (L: the protospacer's length).  Each SNV is taken alone on the reference background: two SNVs in one footprint do not combine.
 * THE ORDER.  By snv_index (the input's order: SNVs need not be sorted and may repeat), then protospacer_start, then '+' before '-': a
 * total order, so the device, the host twin and repeated calls return the same bytes.  A SNV has at most 2 x 48 records.
 * STATUS.  status[i], one byte per SNV (caller-allocated, may be NULL), checked in this order: 2: the reference's base at `position` is
 * not A C G T U; 1: `ref` is given and differs from the reference's base (upper case, U as T); 3: `alt` equals the reference's base;
 * 0: examined.  A SNV whose status is not 0 has no records. */
typedef struct {                /* 12 bytes */
  int32_t contig_index;
  int32_t position;             /* 0-based, forward */
  char ref;                     /* 0: not checked; else A C G T U, either case */
  char alt;                     /* A C G T U, either case */
  uint16_t reserved;            /* 0 */
} calitas_snv_t;
typedef struct {                /* 32 bytes */
  calitas_site_t site;          /* the alt allele's site where one stands (kind & 1), else the reference's */
  uint32_t snv_index;
  uint8_t kind;                 /* 1: on alt only, 2: on the reference only, 3: on both */
  int8_t other_pam_index;       /* kind 3: the reference site's pam_index; else -1 */
  int8_t guide_offset;          /* where the SNV is, counted as the guide reads from the protospacer's first base:
                                   0 .. L-1 inside it, L .. L+15 in a 3' PAM, -1 .. -16 in a 5' PAM */
  uint8_t reserved;             /* 0 */
  uint32_t guide_lo, guide_hi;  /* protospacer of `site`'s allele as the guide reads, bit-planes as calitas_near_hit_t's target_lo/hi */
} calitas_allele_site_t;
/* *sites: the records, one block for calitas_free, also when there are none.  n_snvs == 0 is legal.  On the device one lane takes one
 * SNV: it holds the SNV against the contig's bounds, loads the words of the bit-planes and of the exception mask around it, matches
 * the 64 protospacer starts whose footprint can hold the SNV bit-parallel on both alleles, and stores its count; after a scan of the
 * workgroups' sums the same match stores every record at its place (no sort, no returning atomic); records and status bytes are
 * copied back once each.  A SNV with a U of the reference within 63 bases is decided on the host by the twin's walk and its records
 * are merged into place.
 * Errors, in this order: CALITAS_ENODEV on a host-only context (the device calls); what calitas_find_sites refuses about the pattern;
 * CALITAS_EINVAL, with a message that names the field and the first offending index, for n_snvs >= 2^32, a contig_index out of range
 * or absent, a position at or beyond the contig's length, an alt or a non-zero ref that is not one of the letters, reserved != 0;
 * CALITAS_ENOMEM when the SNVs and their records do not fit the device. */
int calitas_find_allele_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs,
                              calitas_allele_site_t** sites, uint64_t* n_sites, uint8_t* status /* [n_snvs], may be NULL */);
/* The first pass alone: *n_sites and, when per_kind is not NULL, the records per kind ([4]; [0] stays 0, they sum to *n_sites).  No
 * records are copied back. */
int calitas_count_allele_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs,
                               uint64_t* per_kind /* [4], may be NULL */, uint64_t* n_sites, uint8_t* status);
/* The host twins: a base-by-base walk with one base replaced; also on a host-only context. */
int calitas_find_allele_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs,
                                   calitas_allele_site_t** sites, uint64_t* n_sites, uint8_t* status);
int calitas_count_allele_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs,
                                    uint64_t* per_kind, uint64_t* n_sites, uint8_t* status);

/* Base-editor guides of a SNV and their bystanders: the guides that put a single-nucleotide variant into a base editor's activity
 * window on the strand the editor can change it on, and the other editable bases that share the window.  No reference counterpart.
 * Letters are upper-cased and a U reads as T throughout; L is the pattern's protospacer length (at most 32).  Targets are
 * calitas_snv_t.  For SNV i:
 * ALLELES.  R is the reference's base at `position`.  The background allele B is R when installing (correct == 0: the cell carries
 * REF, the edit makes ALT) and `alt` when correcting (correct == 1: the cell carries ALT, the edit makes REF); the product P is the
 * other one.  The background contig is the contig with B at `position`.  Each SNV is taken alone.
 * STRAND.  '+' when (B, P) == (from_base, to_base), '-' when (complement of B, complement of P) == (from_base, to_base); at most one
 * holds.
 * SITE.  site_B(p, s) is the record calitas_find_sites(pattern, the whole contig) would list at protospacer start p on strand s of the
 * background contig (the first matching PAM wins, a base that is not A C G T U is in no footprint, a footprint that leaves the contig
 * is no site), or none.
 * GUIDE BASES.  g_0 .. g_{L-1} are the site's protospacer as the guide reads; g_{-1} is the base 5' of it -- on '+' the contig's base
 * p - 1, on '-' the complement of base p + L -- and is absent outside the contig and where that base is not A C G T U.
 * EDITABLE.  Position i is editable when window_from <= i < window_to, g_i == from_base, and the context is any or g_{i-1} is present
 * and in the context's set.
 * A RECORD is written for (i, p) on the SNV's strand when site_B(p, s) exists, the target's offset o (position - p on '+',
 * p + L - 1 - position on '-') lies in the window, position o is editable, and popcount(editable) - 1 <= max_bystanders.  `site` is
 * site_B(p, s), bit i of `editable` says that position i is editable (the target's bit is set), guide_lo / guide_hi hold the
 * background allele's protospacer as the guide reads (calitas_allele_site_t's planes).
 * THE ORDER.  By snv_index (the input's order: SNVs need not be sorted and may repeat), then protospacer_start: a total order, so the
 * device, the host twin and repeated calls return the same bytes.  A SNV has at most window_to - window_from records.
 * STATUS.  status[i], one byte per SNV (caller-allocated, may be NULL), checked in this order: 2: the reference's base at `position` is
 * not A C G T U; 1: `ref` is given and differs from the reference's base; 3: `alt` equals the reference's base; 4: the change is not
 * this editor's on either strand; 5: it is, but the target's own 5' neighbour fails `context` (this depends on the contig alone, not
 * on the guide); 0: examined.  A SNV whose status is not 0 has no records. */
typedef struct {                /* 8 bytes */
  char from_base, to_base;      /* A C G T U, either case; distinct.  C->T: a CBE, A->G: an ABE, C->G: a CGBE */
  uint8_t window_from, window_to; /* positions of the protospacer as the guide reads, 0-based half-open: 0 <= from < to <= L */
  char context;                 /* IUPAC letter the base 5' of an edited base (as the guide reads) must lie in; 0 or N: any */
  uint8_t correct;              /* 0 install: the cell carries REF, the edit makes ALT.  1 correct: the cell carries ALT, the edit makes REF */
  uint8_t max_bystanders;       /* 0 .. 31: keep records with at most this many; 255: no bound */
  uint8_t reserved;             /* 0 */
} calitas_base_edit_t;
typedef struct {                /* 32 bytes: two 16-byte stores */
  calitas_site_t site;          /* the site on the background allele */
  uint32_t snv_index;
  uint32_t editable;            /* bit i: protospacer position i (as the guide reads) is editable; the target's bit is set */
  uint32_t guide_lo, guide_hi;  /* the background allele's protospacer as the guide reads: calitas_allele_site_t's planes */
} calitas_edit_site_t;
/* *sites: the records, one block for calitas_free, also when there are none.  n_snvs == 0 is legal.  On the device one lane takes one
 * SNV: it holds the SNV against the contig's bounds, loads in one round the words of the bit-planes and of the exception mask that
 * cover the 95 bases from position - 47 (every footprint of the 32 protospacer starts position - 31 .. position, on either strand),
 * takes the reference's base from that window (it decides the strand, which from there on is a select), matches the 32 starts
 * bit-parallel on the background allele, keeps those that hold the SNV in the editor's window, and stores its count; after a scan
 * of the workgroups' sums the same match stores every record at its place (no sort, no returning atomic); records and status bytes
 * are copied back once each.  A SNV with a U of the reference within 63 bases is decided on the host by the twin's walk and its
 * records are merged into place.
 * Errors, in this order: CALITAS_ENODEV on a host-only context (the device calls); what calitas_find_sites refuses about the pattern;
 * CALITAS_EINVAL, with a message that names the field, for a from_base or to_base that is not one of the letters or the two equal, a
 * window that is empty or ends past L, a context that is no IUPAC letter, correct > 1, max_bystanders of 32 .. 254, reserved != 0;
 * what calitas_find_allele_sites refuses about the SNVs; CALITAS_ENOMEM when the SNVs and their records do not fit the device. */
int calitas_find_edit_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs,
                            uint64_t n_snvs, calitas_edit_site_t** sites, uint64_t* n_sites, uint8_t* status /* [n_snvs], may be NULL */);
/* The first pass alone: *n_sites and, when per_bystanders is not NULL, the records with 0, 1, 2 and 3 or more bystanders ([4], they
 * sum to *n_sites).  No records are copied back. */
int calitas_count_edit_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs,
                             uint64_t n_snvs, uint64_t* per_bystanders /* [4], may be NULL */, uint64_t* n_sites, uint8_t* status);
/* The host twins: a base-by-base walk of the background contig; also on a host-only context. */
int calitas_find_edit_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit,
                                 const calitas_snv_t* snvs, uint64_t n_snvs, calitas_edit_site_t** sites, uint64_t* n_sites, uint8_t* status);
int calitas_count_edit_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit,
                                  const calitas_snv_t* snvs, uint64_t n_snvs, uint64_t* per_bystanders, uint64_t* n_sites, uint8_t* status);

/* Microhomology and frameshift odds: what the cut of a site is likely to become.  A double-strand break with microhomologies either
 * side of it is repaired by MMEJ into a few predictable deletions; a guide whose likely deletions are multiples of three leaves the
 * protein in frame.  No reference counterpart.
 * THE WINDOW.  `left` bases 5' and `right` bases 3' of the cut as the guide reads, 1 .. 32 each, W = left + right <= 64.  The cut is
 * cut_offset bases into the protospacer as the guide reads, 0 .. L (calitas_site_pairs_t's cut_offset: L - 3 is the Cas9 cut with a
 * 3' PAM).  With p the record's protospacer_start the forward cut is c = p + cut_offset on '+' and c = p + L - cut_offset on '-'; the
 * window is the forward bases [c - left, c + right) on '+' and the reverse complement of the forward bases [c - right, c + left) on
 * '-'.  Call its letters x[0 .. W): the cut lies between x[left - 1] and x[left].
 * A site is scored when the window lies inside its contig -- the contig bounds it, not the region -- and every base of it is a plain
 * A C G T, in either case, or a U (read as T).  Otherwise both numbers are CALITAS_MH_NONE.
 * THE SCORE.  For every deletion length d = 1 .. W - 1 let lo(d) = max(0, left - d) and hi(d) = min(left, W - d).  Position i in
 * [lo(d), hi(d)) is a match when x[i] == x[i + d]: the left copy lies left of the cut, the right copy right of it.  A microhomology
 * is a maximal run of matches, maximal within [lo(d), hi(d)), of length k >= min_length (2 .. 8); its term is weight[d - 1] * (k + g)
 * with g the number of G and C among its k bases.  `weight` is W - 1 unsigned Q16 values, each <= CALITAS_MH_MAX_WEIGHT; a weight
 * exp(-d / 20) gives the published shape.  total_q16 is the sum of all terms, out_of_frame_q16 the sum of those with d % 3 != 0.
 * The sum of 2 (hi(d) - lo(d)) * 65536 over d is at most 2^27 (64 G's at left = right = 32 under unit weights reach 133 955 584), so
 * neither sum overflows nor equals CALITAS_MH_NONE.  Integer addition has no order, so the kernel, the host twin and a plain loop
 * give the same numbers.  The library ships the mechanism and a file format (models/example_microhomology60.tsv), no published
 * weight table. */
#define CALITAS_MH_NONE 0xFFFFFFFFu           /* this site has no score */
#define CALITAS_MH_MAX_SIDE 32
#define CALITAS_MH_MAX_WEIGHT 65536u          /* 1.0 in Q16 */
typedef struct {
  int32_t left, right;          /* bases 5' and 3' of the cut AS THE GUIDE READS, 1 .. 32 each */
  int32_t cut_offset;           /* 0 .. L */
  int32_t min_length;           /* 2 .. 8: the shortest run that counts */
  const uint32_t* weight;       /* [left + right - 1] by deletion length d - 1, Q16, each <= CALITAS_MH_MAX_WEIGHT */
} calitas_mh_model_t;
typedef struct { uint32_t total_q16, out_of_frame_q16; } calitas_mh_score_t;   /* 8 bytes */
/* The records of calitas_find_sites_filtered(pattern, filter, ...), in that call's order and with its bytes; scores[i] belongs to
 * sites[i].  min_out_of_frame_permille == 0 keeps every site, the unscored ones carrying CALITAS_MH_NONE twice; 1 .. 1000 keeps the
 * scored sites with total_q16 > 0 and (uint64_t)out_of_frame_q16 * 1000 >= (uint64_t)permille * total_q16.
 * sites == NULL && scores == NULL: *n_sites only.  Each block takes one calitas_free.
 * On the device the records of the site kernel's two passes stay where they are: one lane per record brings its window down to bit 0
 * of a pair of 64-bit planes and takes each diagonal d with two shifts, two XORs and a popcount; with a threshold a second kernel
 * compacts records and scores in order (ranks from ballots: no sort, no returning atomic) before the one copy-back.  Windows with an
 * exception base -- a U among them, which the device cannot tell from an N -- are decided on the host.
 * Errors, in this order: what calitas_find_sites_filtered refuses; CALITAS_EINVAL, with a message that names the field, for a NULL
 * model or weight, left or right outside 1 .. 32, cut_offset outside 0 .. L, min_length outside 2 .. 8, a weight above
 * CALITAS_MH_MAX_WEIGHT, a permille outside 0 .. 1000; CALITAS_ENODEV on a host-only context; CALITAS_ENOMEM when records and scores
 * do not fit the device. */
int calitas_find_sites_microhomology(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter /* may be NULL */,
                                     const calitas_mh_model_t* model, int32_t min_out_of_frame_permille, int32_t chrom_index, uint64_t start,
                                     uint64_t end, calitas_site_t** sites, calitas_mh_score_t** scores, uint64_t* n_sites);
/* The host twin: calitas_find_sites_filtered_host's records, each window walked diagonal by diagonal, letter by letter; also on a
 * host-only context. */
int calitas_find_sites_microhomology_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                          const calitas_mh_model_t* model, int32_t min_out_of_frame_permille, int32_t chrom_index, uint64_t start,
                                          uint64_t end, calitas_site_t** sites, calitas_mh_score_t** scores, uint64_t* n_sites);

/* SequentialGuideAligner.align on explicit (guide, target) pairs -- the per-task call of PairwiseAlignSequences
 * (PairwiseAlignSequences.scala:64 -> alignBest, SequentialGuideAligner.scala:333-345) and AlignToReference
 * (AlignToReference.scala:114-135 -> alignToRef / alignToRefBest, SequentialGuideAligner.scala:359-418).  Task t aligns
 * guides[t] to targets[t] (target_lengths[t] bytes, used as given: no N trimming, case-insensitive scoring) with
 * targetOffset = target_offsets[t] (NULL = 0).  params->max_guide_diffs < 0 selects alignBest's limits per task
 * (d = protospacer length, p = longest PAM, D = d + g + p, maxOverlap = 0); otherwise the limits in params apply to every
 * task.  *out receives, task by task, what align() returns (forward-strand list then reverse-strand list after the
 * overlap filter); contig_index / guide_index of each record hold the task index; counts[t] = alignments of task t. */
int calitas_align_windows(calitas_ctx* ctx, int32_t n_tasks, const calitas_guide_t* guides, const uint8_t* const* targets,
                          const uint32_t* target_lengths, const int32_t* target_offsets, const calitas_params_t* params,
                          calitas_aln_t** out, uint64_t* n_out, uint32_t** counts);
/* Padded strings of a record returned by calitas_align_windows, from the caller's own target bytes (case preserved). */
int calitas_padded_strings_target(const calitas_guide_t* guide, const calitas_aln_t* aln, const uint8_t* target, uint32_t target_length,
                                  int32_t target_offset, char* padded_guide, char* padded_alignment, char* padded_target);

/* Host-side stages, usable on a host-only context ------------------------------------------------------------------ */

/* The per-window greedy filter of SequentialGuideAligner.align (SequentialGuideAligner.scala:315-320) on the
 * alignments of ONE window given in enumeration order (forward-strand list then reverse-strand list): stable sort by
 * (score desc, gap bases asc), keep if edits <= max_total_diffs and no kept same-strand alignment overlaps by more
 * than max_overlap.  keep[i] is set to 1 for survivors; order[] receives the indices of survivors in output order. */
int calitas_window_filter(const calitas_aln_t* alns, int32_t n, int32_t max_total_diffs, int32_t max_overlap,
                          int32_t* order, int32_t* n_kept);

/* removeOverlaps + ReferenceHit.sort + the 34-column rows (SearchReference.scala:641-648, ReferenceHit.scala:99-287)
 * for the alignments of one guide.  Returns the full hits.txt text (header + rows) in *tsv. */
int calitas_hits_tsv(const calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                     const calitas_aln_t* alns, uint64_t n_alns, const char* aligner_version, const char* time_stamp,
                     char** tsv, uint64_t* n_rows);

/* The twin of calitas_hits_tsv for the table: removeOverlaps on the alignments of one guide, then the kept hits counted (the host stage
 * calitas_search_counts falls back to; works on a host-only context). */
int calitas_hits_counts(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_aln_t* alns,
                        uint64_t n_alns, calitas_counts_t** out);

/* The twin of calitas_hits_counts for the score.  No reference counterpart.  It runs removeOverlaps on the alignments of one guide, then the kept
 * hits counted and scored from their ops (guide orientation) and the bases of the packed reference -- the host stage
 * calitas_search_scores falls back to; works on a host-only context. */
int calitas_hits_scores(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                        const calitas_aln_t* alns, uint64_t n_alns, calitas_scores_t** out);

/* The twin of calitas_hits_scores for the list.  No reference counterpart.  It is calitas_hits_scores plus the k highest-scoring imperfect
 * kept hits in the order of the calitas_top_t contract -- the host stage calitas_search_top falls back to; works on a host-only context. */
int calitas_hits_top(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                     uint32_t k, const calitas_aln_t* alns, uint64_t n_alns, calitas_top_t** out);

/* The twin of calitas_hits_top for calitas_search_regions -- the host stage it falls back to (CALITAS_HOST_HITS=1, -O 0, a declined
 * device stage); works on a host-only context.  No reference counterpart. */
int calitas_hits_regions(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                         uint32_t k, uint32_t list_mask, const calitas_aln_t* alns, uint64_t n_alns, calitas_regions_t** out);
/* (test hook) The class the context's flattened regions give the extent [start, end) of a contig, or -1 without regions / for a bad contig. */
int calitas_region_class(const calitas_ctx* ctx, int32_t contig_index, int64_t start, int64_t end);

/* A hit row built by the caller -- the variant branch of SearchReference.execute (SearchReference.scala:570-630) builds its
 * ReferenceHits from variant windows on the host.  calitas_hits_tsv_ext lets such hits take part in removeOverlaps (grouped by
 * chromosome, strand and variant_description, SearchReference.scala:656) and in the final sort next to the reference hits;
 * `row` (34 tab-separated columns, no newline) is emitted verbatim. */
typedef struct {
  int32_t contig_index;
  int32_t coordinate_start;     /* ReferenceHit.coordinate_start */
  int32_t end;                  /* ReferenceHit.end = coordinate_start + cigar.lengthOnTarget - 1 (ReferenceHit.scala:135-138) */
  int32_t score;
  int8_t strand;
  const char* variant_description;   /* NULL or "" = none */
  const char* row;
} calitas_ext_hit_t;
int calitas_hits_tsv_ext(const calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                         const calitas_aln_t* alns, uint64_t n_alns, const calitas_ext_hit_t* ext, uint64_t n_ext,
                         const char* aligner_version, const char* time_stamp, char** tsv, uint64_t* n_rows);

/* calitas_search_hits with the text delivered into a buffer of the caller (dst_capacity bytes, NUL included) instead of a block of
 * the library: what a multi-process job uses to have every process's piece of hits.txt land in one shared mapping without a second
 * copy (bench.py --gpus N).  The buffer should be page-locked -- calitas_pin_host does that -- or the copy from the device falls back
 * to the runtime's staged path; a block from calitas_alloc_host is what the copy engines like best.  A search that does not fit the
 * device in one pass runs one pass per contig, as calitas_search_hits does, with every contig's rows crossing the bus straight to
 * their place in the buffer.  CALITAS_EINVAL when the buffer is too small. */
int calitas_search_hits_into(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                             const char* aligner_version, const char* time_stamp, char* dst, uint64_t dst_capacity, uint64_t* tsv_bytes,
                             uint64_t* n_rows);
/* Page-locks / releases host memory the caller owns (hipHostRegister): destinations of calitas_search_hits_into. */
int calitas_pin_host(calitas_ctx* ctx, void* p, uint64_t bytes);
int calitas_unpin_host(calitas_ctx* ctx, void* p);
/* calitas_free parks the blocks it is given -- up to 24 GB of texts and arrays, and one pageable block of a gigabyte or more (the text
 * of a whole-genome search with variants: writing 22 GB into pages nobody has touched, and handing them back, is most of what such a
 * call costs on the host) -- for the next call of the kind to take as they are.  calitas_release_parked() returns all of it to the
 * system; CALITAS_FREE_NOW=1 parks nothing big. */
void calitas_release_parked(void);

/* A page-locked block of the runtime's own (hipHostMalloc), handed back with calitas_free: the destination the *_into calls like best --
 * the GPU's copy engines write into such a block directly (a range that calitas_pin_host merely locked is served by the runtime's
 * copy kernels instead).  NULL when the block cannot be had.  Meant to be reused from call to call: page-locking is not cheap. */
void* calitas_alloc_host(uint64_t bytes);

/* calitas_search_hits with the text handed to a callback instead of returned in one block (Metric.writer's output stream,
 * SearchReference.scala:646-648): `sink` receives consecutive pieces of hits.txt -- the whole text in one piece when the search fits
 * one call, the header and then every contig's rows (in portions of at most 1 GB) when it runs one pass per contig; a piece is
 * valid only during the call.  A non-zero return of the sink aborts the search with CALITAS_EIO.  For searches whose hits.txt has
 * tens of gigabytes this avoids holding it in memory. */
typedef int (*calitas_text_sink_t)(const char* piece, uint64_t bytes, void* user);
int calitas_search_hits_stream(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                               const char* aligner_version, const char* time_stamp, calitas_text_sink_t sink, void* user,
                               uint64_t* tsv_bytes, uint64_t* n_rows);

/* SearchReference.execute with --variants (SearchReference.scala:570-648), end to end: the reference hits of calitas_search plus
 * the hits of every variant window -- variantWindowIterator / nextChunk / reChunk / alleleCombos / buildVariantWindow
 * (SearchReference.scala:217-399) on the host, the windows aligned on the GPU in batches (the calitas_align_windows path), coordinates
 * lifted back with refOffsetAtBaseOffset (SearchReference.scala:133-156), window-local flanks (SearchReference.scala:598-613), the
 * variant columns of ReferenceHit.Builder.build (ReferenceHit.scala:211-233) -- merged by removeOverlaps / ReferenceHit.sort.
 * vcf_path: plain or gzip VCF, records in reference order (CHROM POS ID REF ALT FILTER INFO with AF / END); chrom: NULL or the
 * --chrom filter (params->chrom_index must name the same contig); vcf_id: the "name:md5" string of ReferenceHit.scala:175-183,
 * or NULL to have it computed from the file; params->max_variants = --max-variants.  *n_windows (optional) receives the number of variant windows. */
int calitas_search_variants(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                            const char* vcf_path, const char* chrom, const char* vcf_id, const char* aligner_version,
                            const char* time_stamp, char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows, uint64_t* n_windows);
/* calitas_search_variants with the text delivered into a buffer of the caller (dst_capacity bytes, NUL included), as
 * calitas_search_hits_into does for a search without variants.  A hits.txt with variants at whole-genome size is tens of gigabytes
 * (21.8 GB for BASELINE config 5's shape): into a block of the library's it crosses the bus into a bounce buffer and is copied from there
 * into pages nobody has touched yet; into a page-locked buffer (calitas_pin_host, once, reused from call to call) every contig's rows
 * cross the bus straight to their place.  CALITAS_EINVAL when the buffer is too small (the message says how far the text got). */
int calitas_search_variants_into(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                                 const char* vcf_path, const char* chrom, const char* vcf_id, const char* aligner_version,
                                 const char* time_stamp, char* dst, uint64_t dst_capacity, uint64_t* tsv_bytes, uint64_t* n_rows,
                                 uint64_t* n_windows);

/* What calitas_search_variants knows about a VCF, on its own.
 * calitas_vcf_identifier: the "name:md5" string of ReferenceHit.scala:175-183 (*id: a block for calitas_free) -- a caller that
 * searches many guides against one VCF computes it once and passes it as vcf_id (0.14 s per 127 MB otherwise, per call).
 * calitas_vcf_records: the records as the search reads them -- plain or gzip, parsed in waves on the context's worker pool, the --chrom
 * filter applied -- one line each: CHROM, POS, end (INFO END, else POS + len(REF) - 1: fgbio Variant.end), ID ("" for "."), REF, the ALT
 * alleles and the AF values (as %.9g of the float the search keeps) separated by commas, tab-separated.  Works on a host-only context
 * (calitas_create(-1)); there so that the reader can be held against an independent one (tests/test_variants_host.py). */
int calitas_vcf_identifier(calitas_ctx* ctx, const char* vcf_path, char** id);
int calitas_vcf_records(calitas_ctx* ctx, const char* vcf_path, const char* chrom, char** text, uint64_t* n_records);

/* Padded strings of one alignment (Alignment.paddedString as used at SequentialGuideAligner.scala:511, plus the
 * reverse-complement handling of 5' PAM guides): each buffer must hold CALITAS_MAX_OPS+1 bytes. */
int calitas_padded_strings(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_aln_t* aln, char* padded_guide,
                           char* padded_alignment, char* padded_target);

const char* calitas_version(void);

#ifdef __cplusplus
}
#endif
#endif
