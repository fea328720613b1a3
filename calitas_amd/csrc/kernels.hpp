// kernels.hpp -- launch interface of scan_columns.hip, scan_rows.hip, align.hip, trace.hip, setup.hip, sites.hip, activity.hip, site_pairs.hip, allele_sites.hip, microhomology.hip and edit_sites.hip (device pointers only).
#pragma once
#include "mailbox.hpp"
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include "common.hpp"

namespace calitas {

struct ScanArgs {
  const uint32_t* codes;
  const uint2* planes;     // the same 2-bit codes as two bit-planes per 32 bases (.x = low bits, .y = high bits): what scan_rows_kernel streams
  const uint32_t* mask;
  const TileInfo* tiles;
  const GuideDev* guides;
  ScanRecord* recs;
  uint32_t* rec_count;
  uint32_t rec_capacity;
  int32_t n_guides;
  int32_t chrom_index;
  uint32_t tile_offset;    // first tile of this launch (a chunked search scans one contig range per launch)
  uint32_t tile_stride;    // 1; > 1 = every tile_stride-th tile only (the record-count estimate of a search that may not fit the device)
};

struct AlignArgs {
  const uint32_t* codes;
  const uint32_t* mask;
  const Run* runs;
  int64_t n_runs;
  const ContigInfo* contigs;
  const TileInfo* tiles;
  const uint64_t* win_base;  // per contig: index of its window 0 in win[] (n_contigs + 1 entries)
  const int2* win;           // N-trimmed window bounds for the current (window size, step)
  const GuideDev* guides;
  const ScanRecord* recs;
  const uint32_t* rec_count;
  RawAln* out;
  uint32_t* out_count;
  uint32_t* anomalies;
  uint32_t* trace_done;     // trace_kernel: workgroups finished (zero at launch); the last one posts the counters to the mailbox
  uint8_t* slab;            // one slab per aligner job (slab.hpp): rec_capacity x slots_per_rec of them
  uint32_t* job_count;      // jobs numbered by expand_kernel (zero at launch)
  uint32_t* cand_count;     // statistics only
  uint64_t* items;          // passing candidates, (slab index << 4 | candidate slot): align_kernel appends, trace_kernel consumes
  uint32_t* item_count;
  uint32_t item_capacity;
  uint32_t slab_bytes;      // size of one slab
  uint32_t slots_per_rec;   // windows a 16-base record can fall into
  uint32_t rec_capacity;
  uint32_t out_capacity;
  uint64_t gw_lo, gw_hi;   // global window indices [gw_lo, gw_hi) this call covers (calitas_params_t::first_window / n_windows)
  uint32_t tile_words;     // code words per scan tile
  // Reference bins (binned.hip): trace_kernel also drops every alignment into the bin its window starts in, so that the stages behind
  // it can work bin by bin without a global grouping step.  bin_idx == nullptr: off.
  uint32_t* bin_idx;       // (n_bins of this lane's range) x bin_cap indices into out[]
  uint32_t* bin_count;     // alignments per bin, zero at launch; may exceed bin_cap (the surplus is not stored: the bin is "crowded")
  const uint32_t* bin_base;  // per contig: index of its first bin
  uint32_t bin_first;      // first bin of this lane's range (bins / bin_count are indexed relative to it)
  uint32_t bin_n;          // bins of the range (an alignment whose window starts outside is not listed: cannot happen, checked)
  uint32_t bin_shift;      // log2 of the bases per bin
  uint32_t bin_cap;
  int32_t pack16;                   // 1: every guide has the same protospacer length (<= 20) and the cells fit sixteen bits: align_pk_kernel
  int32_t max_guide_len;            // longest protospacer among the guides (0 = unknown): align_kernel packs three jobs per wave up to 20
  unsigned long long* stamps;       // (binned tail) stamps[0] = the device's wall clock when align_kernel starts; may be null
  SearchDev sp;
};

// The small inputs of one lane's search in ONE launch: the guide's constants, the lane's eight counters cleared, the row stage's three
// counts cleared, the constant row strings, the bins' scratch cleared.  As separate stream commands (two uploads, three or four fills)
// they took ~4.5 us each on the device and as long again on the host: 28 of the 140 us of an E. coli-sized call.  Everything travels
// in the kernel's argument block (one guide, row strings up to LANE_SETUP_BLOB bytes); callers fall back to the commands otherwise.
constexpr uint32_t LANE_SETUP_BLOB = 1536;
struct LaneSetupArgs {
  alignas(16) GuideDev guide;      // (16-byte aligned: the kernel reads its argument block in 16-byte pieces -- it lives in host memory)
  GuideDev* d_guides;              // (both null: the row stage's part only)
  uint32_t* d_counters;            // 8 words
  uint64_t* d_row_counts;          // 3 x 64 bit, or null
  char* d_blob;                    // or null
  uint4* clear;                    // or null; clear_bytes is a multiple of 16
  uint32_t clear_bytes;
  uint32_t blob_bytes;             // d_blob has room for this rounded up to 16
  alignas(16) uint8_t blob[LANE_SETUP_BLOB];
};
hipError_t launch_lane_setup(const LaneSetupArgs& a, hipStream_t stream);

hipError_t launch_scan(const ScanArgs& a, int chunk, uint32_t n_tiles, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// scan_rows.hip: the row-wise scan (default) and the one-off conversion codes[] -> planes[] at upload time
hipError_t launch_scan_rows(const ScanArgs& a, int chunk, int warm_words, uint32_t n_tiles, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
hipError_t launch_planes(const uint32_t* codes, uint2* planes, uint64_t n32, hipStream_t stream);
// expand_kernel (scan records -> aligner jobs, their slabs' heads written) + align_kernel
hipError_t launch_align(const AlignArgs& a, uint32_t n_blocks, hipStream_t stream);
// post: the kernel's last workgroup publishes the eight counters at a.rec_count to that mailbox (mailbox.hpp) -- wait for it with mailbox_wait
hipError_t launch_trace(const AlignArgs& a, uint32_t n_blocks, hipStream_t stream, hipEvent_t stop = nullptr, Mailbox* post = nullptr);
hipError_t launch_window_table(const Run* runs, int64_t n_runs, const ContigInfo* contigs, const uint64_t* win_base, int n_contigs,
                               uint64_t n_windows, int W, int step, int2* out, hipStream_t stream);
hipError_t launch_dpp_selftest(int* out, hipStream_t stream);

// sites.hip: exact IUPAC pattern scan (calitas_find_sites / calitas_count_sites).  One SitePattern per (PAM, strand): the letters the
// FORWARD text must show around a protospacer that starts at base p -- for '-' the reverse complement of the strand-space pattern, so
// both strands are matched on the same planes.  Offsets are relative to p: the footprint is [p + lo, p + hi), -16 <= lo <= 0 < hi <= 48.
constexpr int SITE_MAX_FOOT = MAX_L + MAX_PAM_LEN;
constexpr int SITES_BLOCK_WORDS = 256;   // 32-base words of a segment = lanes of a workgroup
struct SitePattern {
  int32_t lo, hi;
  int32_t pam_off;                 // the PAM starts at p + pam_off (lo for a PAM on the left, the protospacer's length on the right)
  int32_t pam_len;
  uint32_t sets[8];                // four bits per offset -16 .. 47 (bit 4 (d + 16) on): the IUPAC set the forward base at p + d must be in,
                                   // 15 for N and outside the footprint
};
struct SitePatterns {
  int32_t n_pams;                  // >= 1: a PAM-less pattern has one entry with pam_len 0
  int32_t pamless;
  int32_t proto_len;
  int32_t pad;
  SitePattern p[MAX_PAMS][2];      // [PAM][strand: 0 '+', 1 '-']
};
// A site filter as the kernel reads it (calitas_site_filter_t after validation): everything about the protospacer as the
// FORWARD text shows it, so that '-' needs no second set of planes -- a run limit sits at the complement's code, a motif is reverse
// complemented.  It lives behind the patterns in one device block (SiteTables), which keeps SitesArgs what it is without a filter.
struct SiteFilterDev {
  int32_t gc_min, gc_max;          // bounds on the G + C count that can bind; 0 and >= proto_len otherwise
  int32_t max_run[2][4];           // [strand][forward base code A C G T]: longest run allowed, 0: no limit (or one no protospacer can exceed)
  int32_t n_motifs;                // distinct strings the forward text must not show: a motif on '+', its reverse complement on '-' --
  int32_t pad;                     // one entry where the two coincide (a palindrome; a motif passed in both orientations), 16 at most
  struct Motif {
    int32_t len;                   // 1 .. 16, <= proto_len
    uint32_t strands;              // bit 0: rejects on '+', bit 1: on '-'
    uint32_t sets[2];              // four bits per offset 0 .. 15 from the occurrence's leftmost forward base, 15 for N and beyond len
  } motif[16];
};
struct SiteTables {
  SitePatterns pat;
  SiteFilterDev filter;            // read by the FILTER instantiations only
};
struct SiteRecord {                // = calitas_site_t
  int32_t contig, proto_start, pam_start;
  int8_t strand, pam_index;
  uint8_t pam_len, proto_len;
};
// The one argument block of every sites_kernel launch.  The fields up to `end` mean the same in every mode; the rest are reused, so
// that the block stays the size it was however many modes there are.  What each mode reads there ("-": nothing):
//   field                     | find pass 1        | find pass 2       | copies          | near / near score       | near list (pass 2)
//   wg_count                  | sites per segment  | -                 | -               | -                       | cursors (a)
//   totals, 0 at launch       | per (contig, strand)| -                | -               | -                       | -
//   wg_offset                 | -                  | scan of wg_count  | -               | -                       | [k]: first record of key k's stretch
//   out, out_capacity         | -                  | SiteRecords       | -               | -                       | NearHits, all stretches (b)
//   keys / near_offsets       | -                  | -                 | slot table (c)  | bucket tables (d)       | as near score
//   key_index / near_members  | -                  | -                 | index per slot  | members (e)             | as near
//   key_counts, 0 at launch   | -                  | -                 | [k]: key k's sites, [n_keys]: the error flag | n_keys rows (f) | -
//   table_mask, table_shift   | -                  | -                 | a key's first slot is (key * COPIES_HASH) >> table_shift
//    / near_m, near_w         | -                  | -                 | -               | M, 0 .. NEAR_MAX_M; bases per piece, 1 .. NEAR_MAX_W: piece p is positions [p w, (p + 1) w)
//   n_keys, key_len, key_first| -                  | -                 | the distinct keys; K, 1 .. proto_len; 1: the guide's first K bases (a 5' PAM), 0: its last K
//   ones_index                | -                  | -                 | the index of the key COPIES_EMPTY itself (all T at K = 32), COPIES_NONE: no query | - | -
// The regions passes (calitas_find_sites_regions: sites_kernel<., ., KEYS_REGIONS>, site_regions.hip) read what find pass 1 and 2 read and
// two fields more, which the find passes leave alone:
//   keys / presence           | the presence table (g), whole packed space: byte w0 / SITES_BLOCK_WORDS + seg is the launch's segment seg
//   table_mask / class_mask   | the classes the call keeps, bit c = class c; a segment whose byte shares no bit with it is dead
// (a) [2 k]: key k's cursor, 0 at launch; [2 k + 1]: its stretch's length or NEAR_LIST_SKIP; [2 n_keys]: the error flag.  (b) the field's
//     type is the site listing's.  (c) open addressing, table_mask + 1 slots (a power of two, at most half taken), COPIES_EMPTY: free.
// (d) near_m + 1 tables of 4^near_w + 1 offsets, one behind the other: the members of piece p's bucket b are near_members[o[b] .. o[b + 1]),
//     o = near_offsets + p (4^near_w + 1); near score and near list: the model's packed table behind them (near_model_offset).
// (e) {the key's low plane, its high plane, its index among the distinct keys, 0}: every key once per piece.  (f) near: near_m + 1
//     counters; near score: near_m + 3, the counters, the sum, the maximum.  Copies and near never run in one launch: they share fields.
// (g) one byte per SITES_BLOCK_WORDS words: bit c is set when a base of class c (0: of no interval) of the segment's contig lies within
//     SITE_MAX_FOOT of the segment -- so every site that starts in the segment has a class whose bit is set.
struct SitesArgs {
  const uint2* planes;
  const uint32_t* mask;
  const TileInfo* tiles;
  const ContigInfo* contigs;
  const SitePatterns* pat;         // device memory: the head of a SiteTables
  uint64_t n_words;                // 32-base words of the packed space
  uint64_t w0;                     // first word of the launch, a multiple of SITES_BLOCK_WORDS
  uint32_t n_segs;                 // segments of SITES_BLOCK_WORDS words from w0 on
  uint32_t segs_per_wg;            // consecutive segments a workgroup takes
  uint32_t tile_words;             // 32-base words per scan tile, a multiple of SITES_BLOCK_WORDS: a segment never spans two tiles
  int32_t chrom_index;
  uint64_t start, end;             // the region, in contig coordinates; end == 0: the contig's end
  uint32_t* wg_count;              // (from here on: the table above)
  unsigned long long* totals;
  const uint64_t* wg_offset;
  SiteRecord* out;
  uint64_t out_capacity;
  union {
    const uint64_t* keys;
    const uint32_t* near_offsets;
    const uint8_t* presence;
  };
  union {
    const uint32_t* key_index;
    const uint4* near_members;
  };
  unsigned long long* key_counts;
  union {
    struct { uint32_t table_mask, table_shift; };
    struct { uint32_t class_mask, class_pad; };
    struct {
      int32_t near_m;
      int32_t near_w;
    };
  };
  uint32_t n_keys;
  uint32_t ones_index;
  int32_t key_len;
  int32_t key_first;
};
// filtered: a.pat's SiteTables holds a filter, and the match vectors are ANDed with it in both passes
hipError_t launch_sites_count(const SitesArgs& a, bool filtered, hipStream_t stream);
// wg_count[0 .. n) -> wg_offset[0 .. n], wg_offset[n] = the total
hipError_t launch_sites_offsets(const uint32_t* wg_count, uint64_t* wg_offset, uint32_t n, hipStream_t stream);
hipError_t launch_sites_write(const SitesArgs& a, bool filtered, hipStream_t stream);

// The KEY of a site (calitas_count_copies): the PAM-proximal K bases of its protospacer as the guide reads them, bit i of the low word
// = low bit of base i's code (A 0, C 1, G 2, T 3), bit i of the high word = its high bit, base 0 the 5' one.  w_lo, w_hi: the planes of
// the protospacer's L FORWARD bases from its leftmost one (bits above L - 1: anything); minus: the guide is their reverse complement --
// the planes' bits in reverse order and complemented; first: the guide's first K bases (5' PAM) instead of its last K.  The host encodes
// a query with L = K on '+': one function for both sides.  At K = 32 a key takes every value of 64 bits.
CAL_HD inline uint64_t copies_key(uint32_t w_lo, uint32_t w_hi, int L, int K, bool minus, bool first) {
  if (minus) { w_lo = __builtin_bitreverse32(~w_lo) >> (32 - L); w_hi = __builtin_bitreverse32(~w_hi) >> (32 - L); }
  const uint32_t by = first ? 0u : (uint32_t)(L - K), m = 0xFFFFFFFFu >> (32 - K);
  return (uint64_t)((w_lo >> by) & m) | ((uint64_t)((w_hi >> by) & m) << 32);
}
constexpr uint64_t COPIES_EMPTY = ~0ull;                    // a free slot; as a key (T x 32) it is kept outside the table (ones_index)
constexpr uint64_t COPIES_HASH = 0x9E3779B97F4A7C15ull;     // multiplicative hash: the product's top bits
constexpr uint32_t COPIES_NONE = 0xFFFFFFFFu;
constexpr uint32_t COPIES_MIN_SLOTS = 16;
// one pass of the unfiltered match; every site's key looked up, a hit adds 1 to its key's counter
hipError_t launch_sites_copies(const SitesArgs& a, hipStream_t stream);

// calitas_count_near: the query keys within M substitutions of a site's key.  The key's K positions are cut into M + 1 disjoint PIECES of
// w = min(K / (M + 1), NEAR_MAX_W) bases from position 0 on (what is left over belongs to no piece): M substitutions leave one piece
// as it was, so every query within M of a site stands in the bucket one of the site's pieces names -- a bucket per value of a piece's
// 2 w bits, addressed directly.
constexpr int NEAR_MAX_M = 3;
constexpr int NEAR_MAX_W = 8;                               // 4^8 + 1 = 65 537 offsets per piece
CAL_HD inline int near_piece_width(int K, int M) { const int w = K / (M + 1); return w < NEAR_MAX_W ? w : NEAR_MAX_W; }
// the bucket of a key's piece: the piece's w bits of the low plane, above them those of the high plane
CAL_HD inline uint32_t near_bucket(uint32_t k_lo, uint32_t k_hi, int p, int w) {
  const uint32_t m = (1u << w) - 1u;
  return ((k_lo >> (p * w)) & m) | (((k_hi >> (p * w)) & m) << w);
}
// one pass of the unfiltered match; every site's key held against the members of its M + 1 buckets, a query at distance d <= M adds 1
// to its counter d
hipError_t launch_sites_near(const SitesArgs& a, hipStream_t stream);

// calitas_score_near: the near kernel with K = L and the score of every pair that counts at d >= 1.  Both letters of a scored position
// are plain bases, so only the 4 x 4 block of the model's mismatch[i] can be read: the host packs it as [MAX_L][4][4] words
// (near_model_index; positions beyond L hold 0) and lays it behind the offsets in the near_offsets allocation (near_model_offset),
// which needs no field of SitesArgs.  key_counts: n_keys rows of near_m + 3 words -- near_m + 1 counts, the sum, the maximum -- zero
// at launch.
constexpr uint32_t NEAR_MODEL_WORDS = 32 * 16;              // 2 KB
static_assert(MAX_L == 32, "a row of the packed model per guide position");
CAL_HD inline uint32_t near_model_index(uint32_t position, uint32_t query_letter, uint32_t site_letter) { return position * 16u + query_letter * 4u + site_letter; }
CAL_HD inline size_t near_model_offset(int M, int w) { return (size_t)(M + 1) * (((size_t)1 << (2 * w)) + 1); }
hipError_t launch_sites_near_score(const SitesArgs& a, hipStream_t stream);

// calitas_list_near: the near kernel's pass run a second time (K = L, the model's table in LDS as above), every (site, query) pair
// that counts written as a record.  The fields no other KEYS_* mode reads carry the layout the host made from the first pass's counts
// (the table at SitesArgs): a pair takes its slot with a returning 32-bit atomicAdd on its key's cursor, the stretch's length is the
// key's count of the first pass, and a slot at or beyond the length is not stored, it raises the call's flag.
// near_order_kernel then writes every stretch in position order into a second buffer of the same layout.  Both kernels are
// near_list.hip's: it instantiates sites.hip's template for this one ending.
struct NearHit {                   // = calitas_near_hit_t
  uint64_t score_q32;
  int32_t contig, proto_start;
  uint32_t target_lo, target_hi, diff_mask;
  int8_t strand, pam_index;
  uint8_t mismatches, reserved;
};
static_assert(sizeof(NearHit) == 32, "two 16-byte stores per record");
constexpr uint32_t NEAR_LIST_SKIP = 0xFFFFFFFFu;
constexpr uint32_t NEAR_ORDER_SHORT = 64;                   // stretches up to here: one wave, a record per lane
constexpr uint32_t NEAR_ORDER_LONG = 4096;                  // up to here: a workgroup, the position keys in 32 KB of LDS; beyond: copied as they are
hipError_t launch_sites_near_list(const SitesArgs& a, hipStream_t stream);
// keys[0 .. n_short): the distinct keys with stretches of 1 .. NEAR_ORDER_SHORT records, keys[n_short .. n_short + n_long): the longer ones
hipError_t launch_near_order(const NearHit* in, NearHit* out, const uint64_t* base, uint32_t* cursors, const uint32_t* keys, uint32_t n_short, uint32_t n_long,
                             uint32_t flag_index, hipStream_t stream);
static_assert(sizeof(SitesArgs) == 176, "a longer argument block costs every sites_kernel launch (DESIGN 4.15)");

// activity.hip: calitas_find_sites_scored.  The records launch_sites_write left on the device, one lane per record: the window of
// W = up + L + down bases around the protospacer, from the planes, under the model's tables.  The host folds `single` into the pair
// table -- integer sums, so exactly -- and lays everything out as one block of words that a workgroup copies to LDS:
//   [0, 16 (W - 1))   pair'[i][4 a + b] = pair[i][4 a + b] + single[i][a]
//   then 4            single[W - 1][.], the last position's
//   then L + 1        gc[.]
//   then 1            intercept
constexpr int ACTIVITY_THREADS = 256;
constexpr int ACTIVITY_MAX_W = 64;
constexpr int ACTIVITY_TABLE_MAX_WORDS = 16 * (ACTIVITY_MAX_W - 1) + 4 + (MAX_L + 1) + 1;
constexpr int32_t ACTIVITY_NONE = INT32_MIN;             // = CALITAS_ACTIVITY_NONE
constexpr int32_t ACTIVITY_HOST_DECIDES = INT32_MIN + 1; // the window holds an exception base (N, IUPAC code, U): scored on the host, always kept
CAL_HD inline uint32_t activity_table_words(int L, int W) { return (uint32_t)(16 * (W - 1) + 4 + (L + 1) + 1); }
struct ActivityArgs {
  const uint2* planes;
  const uint32_t* mask;
  const ContigInfo* contigs;
  const int32_t* table;            // device memory: activity_table_words(L, W) words
  const SiteRecord* recs;          // n records, 16-byte aligned
  int32_t* scores;                 // n
  uint32_t* wg_kept;               // per workgroup: records kept (score >= min_score, or the host decides); nullptr: no threshold
  uint64_t n;
  uint64_t n_words;                // 32-base words of the packed space
  int32_t n_contigs;
  int32_t L, up, down;
  int32_t min_score;
};
hipError_t launch_activity_score(const ActivityArgs& a, hipStream_t stream);
// The kept records and their scores, in order: record i of workgroup g goes to wg_offset[g] + its rank among g's kept records.
hipError_t launch_activity_compact(const SiteRecord* recs, const int32_t* scores, uint64_t n, int32_t min_score, const uint64_t* wg_offset,
                                   SiteRecord* out_recs, int32_t* out_scores, uint64_t out_capacity, hipStream_t stream);
inline uint32_t activity_blocks(uint64_t n) { return (uint32_t)((n + ACTIVITY_THREADS - 1) / ACTIVITY_THREADS); }

// site_pairs.hip: calitas_find_site_pairs.  The records launch_sites_write left on the device, in listing order, one lane per record.
// The rule of a pair (calitas_hip.h, calitas_site_pairs_t) in the two functions the kernels and the host twin share:
// a site's cut, and whether two cuts and strands make a pair -- integers only.
constexpr int SITE_PAIR_THREADS = 256;
constexpr int32_t SITE_PAIR_MAX_DISTANCE = 65535;         // = CALITAS_PAIR_MAX_DISTANCE
struct SitePairRule {
  int32_t min_distance, max_distance;
  int32_t L, cut;                  // the protospacer's length; the cut's position in it as the guide reads, 0 .. L
  int32_t slack;                   // |L - 2 cut|: how far the difference of two cuts can be from that of the two starts
  uint32_t orientations;           // bit o: pairs of orientation o count
};
struct SitePair {                  // = calitas_site_pair_t
  uint32_t left, right;
  int32_t distance;
  uint8_t orientation, reserved[3];
};
static_assert(sizeof(SitePair) == 16, "one 16-byte store per record");
CAL_HD inline int32_t site_cut(const SitePairRule& r, int32_t proto_start, bool minus) { return minus ? proto_start + r.L - r.cut : proto_start + r.cut; }
// Sites i < j of one contig with these cuts and strands: the pair's orientation (left is '-') + 2 (right is '-'), the left member the
// one with the smaller cut and at equal cuts i; -1: no pair.
CAL_HD inline int site_pair_orientation(const SitePairRule& r, int32_t cut_i, bool minus_i, int32_t cut_j, bool minus_j) {
  const int32_t d = cut_j - cut_i, distance = d < 0 ? -d : d;
  if (distance < r.min_distance || distance > r.max_distance) return -1;
  const int o = ((d < 0 ? minus_j : minus_i) ? 1 : 0) + ((d < 0 ? minus_i : minus_j) ? 2 : 0);
  return ((r.orientations >> o) & 1u) ? o : -1;
}
struct SitePairArgs {
  const SiteRecord* recs;          // n records in listing order (contig, protospacer start, '+' first), 16-byte aligned
  uint64_t n;                      // < 2^32
  uint32_t* lane_count;            // n: the pairs (i, j > i) of record i
  uint32_t* wg_count;              // per workgroup: the sum of its lanes' counts
  unsigned long long* per_orientation;   // 4, 0 at launch (the count kernel)
  const uint64_t* wg_offset;       // the scan of wg_count (the write kernel)
  SitePair* out;
  uint64_t out_capacity;
  SitePairRule rule;
};
inline uint32_t site_pair_blocks(uint64_t n) { return (uint32_t)((n + SITE_PAIR_THREADS - 1) / SITE_PAIR_THREADS); }
hipError_t launch_site_pairs_count(const SitePairArgs& a, hipStream_t stream);
// The pairs in (i, j) order: pair k of record i of workgroup g goes to wg_offset[g] + the counts of g's lanes before i + k.
hipError_t launch_site_pairs_write(const SitePairArgs& a, hipStream_t stream);

// allele_sites.hip: calitas_find_allele_sites.  One lane per SNV; the 64 protospacer starts p of (position - 48, position + 16] are the
// ones whose footprint [p + lo, p + hi) can hold the SNV, one 64-bit match vector per (allele, PAM, strand).
constexpr int ALLELE_THREADS = 256;
constexpr uint32_t ALLELE_MAX_RECORDS = 2 * SITE_MAX_FOOT;   // per SNV
constexpr uint16_t ALLELE_HOST_DECIDES = 1;                  // Snv::reserved of the device's copy: a U within reach, the host twin decides
struct Snv {                       // = calitas_snv_t
  int32_t contig, position;
  char ref, alt;
  uint16_t reserved;
};
struct AlleleSite {                // = calitas_allele_site_t
  SiteRecord site;
  uint32_t snv_index;
  uint8_t kind;
  int8_t other_pam_index, guide_offset;
  uint8_t reserved;
  uint32_t guide_lo, guide_hi;
};
static_assert(sizeof(Snv) == 12 && sizeof(AlleleSite) == 32, "two 16-byte stores per record");
// 2-bit code of A C G T U in either case (the host has checked the letter)
CAL_HD inline uint32_t allele_code(char ch) { const int c = ch & 0xDF; return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }
struct AlleleArgs {
  const uint2* planes;
  const uint32_t* mask;
  const ContigInfo* contigs;
  const SitePatterns* pat;         // device memory: the head of a SiteTables
  const Snv* snvs;
  uint64_t n;                      // < 2^32
  uint64_t n_words;                // 32-base words of the packed space
  int32_t n_contigs;
  uint32_t* lane_count;            // n: the records of SNV i
  uint8_t* status;                 // n
  uint32_t* wg_count;              // per workgroup: the sum of its lanes' counts
  unsigned long long* per_kind;    // 4, 0 at launch (the count kernel)
  const uint64_t* wg_offset;       // the scan of wg_count (the write kernel)
  AlleleSite* out;
  uint64_t out_capacity;
};
inline uint32_t allele_blocks(uint64_t n) { return (uint32_t)((n + ALLELE_THREADS - 1) / ALLELE_THREADS); }
hipError_t launch_allele_count(const AlleleArgs& a, hipStream_t stream);
// The records in (SNV, start, strand) order: record k of SNV i of workgroup g goes to wg_offset[g] + the counts of g's lanes before i + k.
hipError_t launch_allele_write(const AlleleArgs& a, hipStream_t stream);

// microhomology.hip: calitas_find_sites_microhomology.  The records launch_sites_write left on the device, one lane per record: the
// window of W = left + right bases around the cut, from the planes, brought to bit 0 of two 64-bit planes; every deletion length d is
// one diagonal -- two shifts, two XORs, the runs of min_length and more, a popcount.  The weights travel in the argument
// block: d is a loop counter, so weight[d - 1] is a scalar load.
constexpr int MH_THREADS = 256;
constexpr int MH_MAX_W = 64;
constexpr uint32_t MH_NONE = 0xFFFFFFFFu;                // = CALITAS_MH_NONE
constexpr uint32_t MH_HOST_DECIDES = 0xFFFFFFFEu;        // out_of_frame beside total == MH_NONE: the window holds an exception base (N, IUPAC
                                                         // code, U): scored on the host, always kept
struct MhScore { uint32_t total, out_of_frame; };        // = calitas_mh_score_t
static_assert(sizeof(MhScore) == 8, "one 8-byte store per record");
struct MhArgs {
  const uint2* planes;
  const uint32_t* mask;
  const ContigInfo* contigs;
  const SiteRecord* recs;          // n records, 16-byte aligned
  MhScore* scores;                 // n
  uint32_t* wg_kept;               // per workgroup: records kept under permille (or the host decides); nullptr: no threshold
  uint64_t n;
  uint64_t n_words;                // 32-base words of the packed space
  int32_t n_contigs;
  int32_t L, left, right, cut, min_length;
  uint32_t permille;               // 1 .. 1000 with wg_kept
  uint32_t weight[MH_MAX_W - 1];   // [d - 1], Q16; W - 1 of them are read
};
// kept under a threshold of `permille` >= 1: a scored site with total > 0 whose out-of-frame share reaches it, or one the host decides
CAL_HD inline bool mh_kept(MhScore s, uint32_t permille) {
  if (s.total == MH_NONE) return s.out_of_frame == MH_HOST_DECIDES;
  return s.total > 0 && (uint64_t)s.out_of_frame * 1000u >= (uint64_t)permille * s.total;
}
hipError_t launch_mh_score(const MhArgs& a, hipStream_t stream);
// The kept records and their scores, in order: record i of workgroup g goes to wg_offset[g] + its rank among g's kept records.
hipError_t launch_mh_compact(const SiteRecord* recs, const MhScore* scores, uint64_t n, uint32_t permille, const uint64_t* wg_offset,
                             SiteRecord* out_recs, MhScore* out_scores, uint64_t out_capacity, hipStream_t stream);
inline uint32_t mh_blocks(uint64_t n) { return (uint32_t)((n + MH_THREADS - 1) / MH_THREADS); }

// edit_sites.hip: calitas_find_edit_sites.  One lane per SNV (Snv, as the allele call reads it); the at most 32 protospacer starts
// whose protospacer can hold the SNV, p = position - 31 + j, are one 32-bit match vector per PAM, matched on the background allele
// alone and on the SNV's strand alone.
constexpr int EDIT_THREADS = 256;
constexpr uint32_t EDIT_MAX_RECORDS = MAX_L;                // per SNV: window_to - window_from
constexpr uint32_t EDIT_NO_BOUND = 255;                     // EditRule::max_bystanders
struct EditRule {                  // calitas_base_edit_t after validation
  uint32_t from, to;               // 2-bit codes
  uint32_t window_from, window_to; // 0 <= from < to <= L
  uint32_t context;                // the set the base 5' of an edited base must be in, bit c = code c; 15: any
  uint32_t correct;                // 0: the background allele is the reference's base, 1: it is alt
  uint32_t max_bystanders;         // 0 .. 31, EDIT_NO_BOUND
};
struct EditSite {                  // = calitas_edit_site_t
  SiteRecord site;
  uint32_t snv_index;
  uint32_t editable;
  uint32_t guide_lo, guide_hi;
};
static_assert(sizeof(EditSite) == 32, "two 16-byte stores per record");
// the set of the complements of a set's bases
CAL_HD inline uint32_t edit_complement_set(uint32_t set) { return ((set & 1u) << 3) | ((set & 2u) << 1) | ((set & 4u) >> 1) | ((set & 8u) >> 3); }
// The strand on which background base b becoming p is the editor's change: 0 '+', 1 '-', -1 neither.
CAL_HD inline int edit_strand(const EditRule& e, uint32_t b, uint32_t p) {
  return (b == e.from && p == e.to) ? 0 : (3u - b == e.from && 3u - p == e.to) ? 1 : -1;
}
struct EditArgs {
  const uint2* planes;
  const uint32_t* mask;
  const ContigInfo* contigs;
  const SitePatterns* pat;         // device memory: the head of a SiteTables
  const Snv* snvs;                 // reserved == ALLELE_HOST_DECIDES: a U within reach, the host twin decides
  uint64_t n;                      // < 2^32
  uint64_t n_words;                // 32-base words of the packed space
  int32_t n_contigs;
  uint32_t* lane_count;            // n: the records of SNV i
  uint8_t* status;                 // n
  uint32_t* wg_count;              // per workgroup: the sum of its lanes' counts
  unsigned long long* per_bystanders;   // 4 (0, 1, 2, 3 or more), 0 at launch (the count kernel)
  const uint64_t* wg_offset;       // the scan of wg_count (the write kernel)
  EditSite* out;
  uint64_t out_capacity;
  EditRule rule;
};
inline uint32_t edit_blocks(uint64_t n) { return (uint32_t)((n + EDIT_THREADS - 1) / EDIT_THREADS); }
hipError_t launch_edit_count(const EditArgs& a, hipStream_t stream);
// The records in (SNV, start) order: record k of SNV i of workgroup g goes to wg_offset[g] + the counts of g's lanes before i + k.
hipError_t launch_edit_write(const EditArgs& a, hipStream_t stream);

}  // namespace calitas
