// sites.hip -- exact IUPAC pattern scan of the packed reference: where can a guide be cut out (calitas_find_sites, gfx950).
// No reference counterpart: the reference starts from a guide somebody already has.
//
// The match runs along the text, as scan_rows.hip does.  A lane owns one 32-base word of the two bit-planes (lo, hi: bit j = low / high
// bit of base j's 2-bit code) and of the exception mask, and builds a MATCH VECTOR per (PAM, strand): bit j = a protospacer can start
// at base 32 w + j.  A footprint reaches at most 16 bases to the left of its protospacer's first base and 48 to the right, so the lane
// sees a chain of four words, w - 1 .. w + 2, staged once per segment of 256 words in LDS.
//   * "the base at offset d from the start lies in the letter's IUPAC set" is a two-input boolean function of the planes moved down
//     by d: two v_alignbit_b32 across the word boundary, then a selection among four all-ones / all-zeros masks, one per base of the
//     letter's set, ANDed into the accumulator.  The pattern is 64 four-bit sets in scalar registers, one per offset; the offsets are
//     unrolled, so every shift is an immediate.  N costs a scalar branch.
//   * "no exception base in the footprint" is a run-length test on ~exc by doubling (runs of 1, 2, 4, .. ANDed with themselves moved
//     down), six steps at most, once per footprint length.
//   * '-' is the reverse-complemented pattern on the same forward planes (the host builds both, SitePattern): one pass over memory.
//   * the region is a mask of start positions per lane; contig ends need nothing (padding is exception bases).
// Output in order, without a sort and without a returning atomic: pass 1 stores one count per segment, a one-workgroup scan turns
// the counts into offsets, pass 2 recomputes the vectors and every lane writes its records at offset + prefix (a DPP prefix sum per
// wave, the waves' sums through LDS); the '+' and '-' record of one position are neighbours.
// COPIES (calitas_count_copies): the copies kernel, sites_kernel<false, false, KEYS_EXACT>, is the first pass's match with another ending -- instead of being counted, every site of the
// lane's word gives its KEY (copies_key: the PAM-proximal K bases as the guide reads, from the chain registers), which is looked up in the
// caller's table of query keys; a hit adds 1 to that key's counter (count_keys).
// NEAR (calitas_count_near): the near kernel, sites_kernel<false, false, KEYS_NEAR>, is the same match with a third ending -- the key is
// held against the query keys that share one of its M + 1 pieces, and a query at Hamming distance d <= M gets 1 in its counter d (near_keys).
// NEAR SCORE (calitas_score_near): sites_kernel<false, false, KEYS_NEAR_SCORE>, the near kernel's ending with the pair's score besides --
// a product of Q16 factors of a model table kept in LDS -- added into a sum and a maximum per query behind its counts.
// NEAR LIST (calitas_list_near): sites_kernel<false, false, KEYS_NEAR_LIST>, the pass run again after the host has laid out a stretch per
// query key from the counts -- every pair that counts stores a 32-byte record at a slot taken from its key's cursor.  It is
// instantiated in near_list.hip, beside near_order_kernel, which puts each stretch in position order by ranking.
// FILTER (calitas_find_sites_filtered): a keep vector per strand from the same registers -- G + C count, base runs and motifs of the
// protospacer, chain positions 32 + j .. 32 + j + L - 1 -- ANDed into the match vectors in both passes (site_keep).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"

namespace calitas {

namespace {

typedef const __attribute__((address_space(4))) SitePatterns PatConst;   // scalar loads
typedef const __attribute__((address_space(4))) SitePattern PatOne;

// acc & "the base at chain position X lies in the set" for the 32 starts of the lane's word: the planes moved down by X across the word
// boundary (X is a compile-time constant: the shift is an immediate, the word pair fixed), then a selection among four all-ones /
// all-zeros masks, one per base of the set (A=1 C=2 G=4 T=8), as in scan_rows.hip's IUPAC part 1.  The set is wave-uniform.
template <int X>
CAL_DEV uint32_t and_letter(uint32_t acc, uint32_t set, const uint32_t (&c_lo)[4], const uint32_t (&c_hi)[4]) {
  constexpr int Q = X >> 5, SH = X & 31;
  const uint32_t lo = SH ? __builtin_amdgcn_alignbit(c_lo[Q + 1], c_lo[Q], SH) : c_lo[Q];
  const uint32_t hi = SH ? __builtin_amdgcn_alignbit(c_hi[Q + 1], c_hi[Q], SH) : c_hi[Q];
  const uint32_t ka = 0u - (set & 1u), kc = 0u - ((set >> 1) & 1u), kg = 0u - ((set >> 2) & 1u), kt = 0u - ((set >> 3) & 1u);
  const uint32_t hi0 = (lo & kc) | (~lo & ka), hi1 = (lo & kt) | (~lo & kg);
  return acc & ((hi & hi1) | (~hi & hi0));
}

// The eight letters of one word of SitePattern::sets (chain positions 16 + 8 I ..): N -- and everything outside the footprint -- is
// skipped by a scalar branch, a whole word of them by one.
template <int I>
CAL_DEV uint32_t and_letters(uint32_t acc, uint32_t sets, const uint32_t (&c_lo)[4], const uint32_t (&c_hi)[4]) {
  if (sets == 0xFFFFFFFFu) return acc;
#define CALITAS_SITE_LETTER(J) \
  if (((sets >> (4 * J)) & 15u) != 15u) acc = and_letter<16 + 8 * I + J>(acc, (sets >> (4 * J)) & 15u, c_lo, c_hi);
  CALITAS_SITE_LETTER(0) CALITAS_SITE_LETTER(1) CALITAS_SITE_LETTER(2) CALITAS_SITE_LETTER(3)
  CALITAS_SITE_LETTER(4) CALITAS_SITE_LETTER(5) CALITAS_SITE_LETTER(6) CALITAS_SITE_LETTER(7)
#undef CALITAS_SITE_LETTER
  return acc;
}

// bits j of a word whose first base is contig position base0 with pmin <= base0 + j <= pmax
CAL_DEV uint32_t range_bits(int64_t base0, int64_t pmin, int64_t pmax) {
  const int64_t a = pmin - base0, b = pmax - base0;
  if (b < 0 || a > 31 || a > b) return 0u;
  const uint32_t from = a > 0 ? (uint32_t)a : 0u, to = b < 31 ? (uint32_t)b : 31u;
  return (0xFFFFFFFFu << from) & (0xFFFFFFFFu >> (31u - to));
}

// inclusive prefix sum over the wave: row_shr 1, 2, 4, 8 inside the rows of 16 lanes, then row 0's and rows 0-1's totals handed on
CAL_DEV uint32_t wave_inclusive_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
  return v;
}

typedef const __attribute__((address_space(4))) SiteFilterDev FilterConst;
typedef const __attribute__((address_space(4))) SiteTables TablesConst;

// ---- the site filter: keep vectors for the 32 starts of the lane's word from chain words 1 - 3 ----
// A vector over chain positions 32 .. 95 is a pair (word 1, word 2).  Zeros come in at position 96: what a window reads from there is
// wrong, and no protospacer that starts in word 1 reaches it (32 + 31 + L - 1 <= 94).

// bit j: some / every bit of [j, j + n) is set (1 <= n <= 32, wave-uniform), by doubling; the last step's windows overlap
template <bool ALL>
CAL_DEV void window(uint32_t (&v)[2], int n) {
  int len = 1;
  while (len < n) {
    const uint32_t by = (uint32_t)(2 * len <= n ? len : n - len);
    const uint32_t m0 = __builtin_amdgcn_alignbit(v[1], v[0], by), m1 = v[1] >> by;
    if (ALL) { v[0] &= m0; v[1] &= m1; } else { v[0] |= m0; v[1] |= m1; }
    len += (int)by;
  }
}

CAL_DEV uint32_t maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (c & (a ^ b)); }

// Starts whose L bases hold between gc_min and gc_max G or C (the same on both strands).  The count is a bit-sliced number per start,
// plane i = bit i: the counts over windows of 1, 2, 4, .. bases by adding a number to itself moved down, and the pieces that make L
// added up as they come by.  Planes that cannot be set yet are constants the compiler drops.
CAL_DEV uint32_t keep_gc(const uint32_t (&c_lo)[4], const uint32_t (&c_hi)[4], int L, int gc_min, int gc_max) {
  uint32_t pw[6][2] = {{c_lo[1] ^ c_hi[1], c_lo[2] ^ c_hi[2]}, {0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}};   // C = 01, G = 10
  uint32_t sum[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  uint32_t done = 0;                                           // bases in sum
#pragma unroll
  for (int k = 0; k < 6; k++) {
    if (L & (1 << k)) {                                        // sum += the windows of 2^k that start `done` further on
      uint32_t c = 0u;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const uint32_t b = __builtin_amdgcn_alignbit(pw[i][1], pw[i][0], done), a = sum[i];
        sum[i] = a ^ b ^ c;
        c = maj(a, b, c);
      }
      done += 1u << k;
    }
    if ((L >> (k + 1)) == 0) break;
    uint32_t c0 = 0u, c1 = 0u;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const uint32_t a0 = pw[i][0], a1 = pw[i][1];
      const uint32_t b0 = __builtin_amdgcn_alignbit(a1, a0, 1u << k), b1 = a1 >> (1u << k);
      pw[i][0] = a0 ^ b0 ^ c0;  c0 = maj(a0, b0, c0);
      pw[i][1] = a1 ^ b1 ^ c1;  c1 = maj(a1, b1, c1);
    }
  }
  // sum >= gc_min and sum <= gc_max, from the low plane up: a plane decides unless it equals the bound's bit
  uint32_t keep = 0xFFFFFFFFu;
  if (gc_min > 0) {
    uint32_t ge = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 6; i++) ge = ((gc_min >> i) & 1) ? (sum[i] & ge) : (sum[i] | ge);
    keep &= ge;
  }
  if (gc_max < L) {
    uint32_t le = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < 6; i++) le = ((gc_max >> i) & 1) ? (~sum[i] | le) : (~sum[i] & le);
    keep &= le;
  }
  return keep;
}

// Chain positions 32 .. 95 at which a run of R + 1 of the forward base `code` starts
CAL_DEV void run_starts(int code, const uint32_t (&c_lo)[4], const uint32_t (&c_hi)[4], int R, uint32_t (&v)[2]) {
#pragma unroll
  for (int i = 0; i < 2; i++) v[i] = ((code & 1) ? c_lo[1 + i] : ~c_lo[1 + i]) & ((code & 2) ? c_hi[1 + i] : ~c_hi[1 + i]);
  window<true>(v, R + 1);
}

// Starts whose L bases hold a run longer than its base's limit (lim: by forward base code, 0 for none): a run of R + 1 starts somewhere
// in [j, j + L - R).  Bases with the same limit share that window.
CAL_DEV uint32_t long_runs(FilterConst* f, int st, const uint32_t (&c_lo)[4], const uint32_t (&c_hi)[4], int L) {
  const int lim[4] = {f->max_run[st][0], f->max_run[st][1], f->max_run[st][2], f->max_run[st][3]};
  uint32_t bad = 0u, done = 0u;
#pragma unroll
  for (int code = 0; code < 4; code++) {
    const int R = lim[code];
    if (R <= 0 || ((done >> code) & 1u)) continue;
    uint32_t v[2];
    run_starts(code, c_lo, c_hi, R, v);
#pragma unroll
    for (int other = code + 1; other < 4; other++) {
      if (lim[other] != R) continue;
      uint32_t w[2];
      run_starts(other, c_lo, c_hi, R, w);
      v[0] |= w[0]; v[1] |= w[1];
      done |= 1u << other;
    }
    window<false>(v, L - R);
    bad |= v[0];
  }
  return bad;
}

// Starts whose L bases hold the motif: an occurrence starts somewhere in [j, j + L - len].  The occurrence vector is and_letter over the
// letters, for the starts in chain words 1 and 2.
CAL_DEV uint32_t has_motif(const uint32_t (&sets)[2], int len, uint32_t (&c_lo)[4], uint32_t (&c_hi)[4], int L) {
#pragma unroll
  for (int i = 0; i < 4; i++) asm volatile("" : "+v"(c_lo[i]), "+v"(c_hi[i]));     // (as in match_word: no moved plane kept across motifs)
  uint32_t v[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#define CALITAS_MOTIF_LETTER(J) \
  if (((sets[J >> 3] >> (4 * (J & 7))) & 15u) != 15u) { \
    v[0] = and_letter<32 + J>(v[0], (sets[J >> 3] >> (4 * (J & 7))) & 15u, c_lo, c_hi); \
    v[1] = and_letter<64 + J>(v[1], (sets[J >> 3] >> (4 * (J & 7))) & 15u, c_lo, c_hi); \
  }
  CALITAS_MOTIF_LETTER(0) CALITAS_MOTIF_LETTER(1) CALITAS_MOTIF_LETTER(2) CALITAS_MOTIF_LETTER(3)
  CALITAS_MOTIF_LETTER(4) CALITAS_MOTIF_LETTER(5) CALITAS_MOTIF_LETTER(6) CALITAS_MOTIF_LETTER(7)
  if (sets[1] != 0xFFFFFFFFu) {
    CALITAS_MOTIF_LETTER(8) CALITAS_MOTIF_LETTER(9) CALITAS_MOTIF_LETTER(10) CALITAS_MOTIF_LETTER(11)
    CALITAS_MOTIF_LETTER(12) CALITAS_MOTIF_LETTER(13) CALITAS_MOTIF_LETTER(14) CALITAS_MOTIF_LETTER(15)
  }
#undef CALITAS_MOTIF_LETTER
  window<false>(v, L - len + 1);
  return v[0];
}

// The filter's verdict on the protospacers that start in the lane's word, per strand.  Every parameter is wave-uniform and comes
// through the scalar path; a test that is not set costs a scalar branch.  Where the footprint holds an exception base the match vector is
// clear already, so the planes' content there does not matter.
CAL_DEV void site_keep(FilterConst* f, int L, uint32_t (&c_lo)[4], uint32_t (&c_hi)[4], uint32_t& plus, uint32_t& minus) {
  const int gc_min = f->gc_min, gc_max = f->gc_max;
  if (gc_min > 0 || gc_max < L) {
    const uint32_t keep = keep_gc(c_lo, c_hi, L, gc_min, gc_max);
    plus &= keep; minus &= keep;
  }
  bool limited = false, same = true;                           // (the same limits by forward base on both strands: A = T and C = G)
#pragma unroll
  for (int code = 0; code < 4; code++) {
    limited = limited || f->max_run[0][code] > 0 || f->max_run[1][code] > 0;
    same = same && f->max_run[0][code] == f->max_run[1][code];
  }
  if (limited) {
    const uint32_t bad = long_runs(f, 0, c_lo, c_hi, L);
    plus &= ~bad;
    minus &= ~(same ? bad : long_runs(f, 1, c_lo, c_hi, L));
  }
  const int n_motifs = f->n_motifs;
  for (int m = 0; m < n_motifs; m++) {
    const uint32_t sets[2] = {f->motif[m].sets[0], f->motif[m].sets[1]}, strands = f->motif[m].strands;
    const uint32_t bad = has_motif(sets, f->motif[m].len, c_lo, c_hi, L);
    if (strands & 1u) plus &= ~bad;
    if (strands & 2u) minus &= ~bad;
  }
}

struct LaneSites {
  uint32_t plus, minus;        // match vectors: a site of that strand starts at base j
  uint32_t kp[3], km[3];       // bit-planes of the matching PAM's index
};

// The match vectors of the lane's word.  c_*: the chain w - 1 .. w + 2; base0: contig position of the word's first base.
template <bool FILTER>
CAL_DEV LaneSites match_word(PatConst* pat, uint32_t (&c_lo)[4], uint32_t (&c_hi)[4], const uint32_t (&c_ex)[4], int64_t base0,
                             int64_t r_start, int64_t r_end) {
  LaneSites s{0u, 0u, {0u, 0u, 0u}, {0u, 0u, 0u}};
  const int n_pams = pat->n_pams;
  int run_len = 0;
  uint32_t run[4] = {0u, 0u, 0u, 0u};       // bit = a run of run_len clean bases starts here (chain positions; beyond the chain: none)
  for (int k = 0; k < n_pams; k++) {
    const int foot = pat->p[k][0].hi - pat->p[k][0].lo;
    if (foot != run_len) {
      run_len = foot;
#pragma unroll
      for (int i = 0; i < 4; i++) run[i] = ~c_ex[i];
      int len = 1;
      while (len < foot) {
        const uint32_t by = (uint32_t)(2 * len <= foot ? len : foot - len);   // < 32; the last step's windows overlap
        run[0] &= __builtin_amdgcn_alignbit(run[1], run[0], by);
        run[1] &= __builtin_amdgcn_alignbit(run[2], run[1], by);
        run[2] &= __builtin_amdgcn_alignbit(run[3], run[2], by);
        run[3] &= run[3] >> by;
        len += (int)by;
      }
    }
#pragma unroll
    for (int st = 0; st < 2; st++) {
      PatOne* sp = &pat->p[k][st];
      const int lo = sp->lo, hi = sp->hi;
      // the moved planes are the same for every PAM and strand: left alone the compiler computes all 128 of them ahead of the loop
      // and keeps them (300 VGPRs)
#pragma unroll
      for (int i = 0; i < 4; i++) asm volatile("" : "+v"(c_lo[i]), "+v"(c_hi[i]));
      // starts whose footprint [p + lo, p + hi) lies in the region and is clean
      uint32_t acc = range_bits(base0, r_start - lo, r_end - hi);
      const uint32_t at = (uint32_t)(32 + lo);                                // 16 .. 32
      acc &= at >= 32u ? run[1] : __builtin_amdgcn_alignbit(run[1], run[0], at);
      acc = and_letters<0>(acc, sp->sets[0], c_lo, c_hi);  acc = and_letters<1>(acc, sp->sets[1], c_lo, c_hi);
      acc = and_letters<2>(acc, sp->sets[2], c_lo, c_hi);  acc = and_letters<3>(acc, sp->sets[3], c_lo, c_hi);
      acc = and_letters<4>(acc, sp->sets[4], c_lo, c_hi);  acc = and_letters<5>(acc, sp->sets[5], c_lo, c_hi);
      acc = and_letters<6>(acc, sp->sets[6], c_lo, c_hi);  acc = and_letters<7>(acc, sp->sets[7], c_lo, c_hi);
      uint32_t& found = st ? s.minus : s.plus;
      uint32_t (&kb)[3] = st ? s.km : s.kp;
      acc &= ~found;                                                          // the first PAM that matches wins
      found |= acc;
      if (k & 1) kb[0] |= acc;
      if (k & 2) kb[1] |= acc;
      if (k & 4) kb[2] |= acc;
    }
  }
  // (the filter sees the protospacer alone, so it commutes with the PAMs' priority; kp / km are read at surviving bits only)
  if constexpr (FILTER) site_keep(&((TablesConst*)pat)->filter, pat->proto_len, c_lo, c_hi, s.plus, s.minus);
  return s;
}

// What a lane brings from memory for one segment: its own word, and for lanes 0-2 one of the three words around the segment.
struct Fetched {
  uint2 pl, halo_pl;
  uint32_t ex, halo_ex;
};

// The keys of the sites that start in the lane's word (chain word 1), looked up one after the other: a site per turn of the loop, '+'
// before '-'.  The protospacer's L <= 32 forward bases from bit j of word 1 on are one v_alignbit_b32 per plane.  The table is open
// addressing with linear probing from the multiplicative hash's slot; at most half of its slots are taken, so a probe ends at the key
// or at a free slot -- and at table_mask + 1 steps whatever the table holds: a probe that runs off that bound sets the call's error flag
// and gives up (the host reports an internal error), it never spins.  A hit adds 1 to the key's counter with a non-returning atomic;
// adds of a wave to one counter are not combined first (what was tried and what it gave).
CAL_DEV void count_keys(const SitesArgs& a, const LaneSites& s, const uint32_t (&c_lo)[4], const uint32_t (&c_hi)[4], int L) {
  const int K = a.key_len;
  const bool first = a.key_first != 0;
  const uint32_t mask = a.table_mask, shift = a.table_shift;
  uint32_t left_p = s.plus, left_m = s.minus;
  while (left_p | left_m) {
    const bool minus = left_p == 0u;
    const uint32_t j = (uint32_t)__builtin_ctz(minus ? left_m : left_p);
    if (minus) left_m &= left_m - 1u; else left_p &= left_p - 1u;
    const uint64_t key = copies_key(__builtin_amdgcn_alignbit(c_lo[2], c_lo[1], j), __builtin_amdgcn_alignbit(c_hi[2], c_hi[1], j), L, K, minus, first);
    uint32_t idx = COPIES_NONE;
    if (key == COPIES_EMPTY) {
      idx = a.ones_index;
    } else {
      uint32_t slot = (uint32_t)((key * COPIES_HASH) >> shift), step = 0;
      for (; step <= mask; step++) {
        const uint64_t k = a.keys[slot];
        if (k == key) { idx = a.key_index[slot]; break; }
        if (k == COPIES_EMPTY) break;
        slot = (slot + 1u) & mask;
      }
      if (step > mask) a.key_counts[a.n_keys] = 1ull;       // no free slot in the whole table: the error flag
    }
    if (idx != COPIES_NONE) (void)atomicAdd(&a.key_counts[idx], 1ull);
  }
}

// The keys of the sites that start in the lane's word, held against the queries within M substitutions: a site per turn of the loop as
// in count_keys.  A query within M of the key equals it in one of the M + 1 pieces at least (kernels.hpp), so it is a member of one of
// the M + 1 buckets the key's pieces name: their offsets are loaded together, then each bucket is walked, a 16-byte member per turn.
// m = the positions at which key and member differ (either plane), d their number.  A member at d <= M counts in the FIRST piece in
// which it equals the key -- in piece p only if every piece before p holds a difference -- so a (site, query) pair counts once however
// many pieces agree.  M, w and the pieces' masks are wave-uniform; both loops end at offsets the host wrote, nothing can spin.
// SCORE (calitas_score_near; K = L, so bit j of the key is guide position j): a member that counts at d >= 1 also gets the pair's score
// under the model -- the set bits of m in ascending order, three at most, each one factor of `model` (near_model_index: position, the
// query's letter, the site's letter; both letters from the four planes) multiplied into s = 2^32 with a truncation by 16 bits -- and
// the key's row of M + 3 counters takes the count, s into the sum and s into the maximum.
// LIST (calitas_list_near; the second run of the pass, K = L): a member that counts, and whose key lists, takes the next slot of its
// key's stretch with a returning atomicAdd on the key's cursor and stores the pair's record there -- the score (2^32 at d = 0), the
// site's contig, start, strand and PAM index (contig, base0 + j, kp / km), both planes of its key, m and d -- as two 16-byte stores.
// The slots' order is whatever the waves' order was; near_order_kernel puts the stretch in position order.  A slot the host's layout
// has no room for is not stored: it raises the call's flag.  Nothing is counted.
constexpr int NEAR_COUNT = 0, NEAR_SCORE = 1, NEAR_LIST = 2;
template <int MODE>
CAL_DEV void near_keys(const SitesArgs& a, const LaneSites& s, const uint32_t (&c_lo)[4], const uint32_t (&c_hi)[4], int L, const uint32_t* model,
                       uint32_t contig = 0u, int64_t base0 = 0, bool pamless = false) {
  constexpr bool SCORE = MODE == NEAR_SCORE;
  const int K = a.key_len, M = a.near_m, w = a.near_w;
  const bool first = a.key_first != 0;
  const uint32_t per_table = (1u << (2 * w)) + 1u, piece = (1u << w) - 1u, row = (uint32_t)M + (SCORE ? 3u : 1u);
  uint32_t left_p = s.plus, left_m = s.minus;
  while (left_p | left_m) {
    const bool minus = left_p == 0u;
    const uint32_t j = (uint32_t)__builtin_ctz(minus ? left_m : left_p);
    if (minus) left_m &= left_m - 1u; else left_p &= left_p - 1u;
    const uint64_t key = copies_key(__builtin_amdgcn_alignbit(c_lo[2], c_lo[1], j), __builtin_amdgcn_alignbit(c_hi[2], c_hi[1], j), L, K, minus, first);
    const uint32_t k_lo = (uint32_t)key, k_hi = (uint32_t)(key >> 32);
    uint32_t from[NEAR_MAX_M + 1], to[NEAR_MAX_M + 1];
#pragma unroll
    for (int p = 0; p <= NEAR_MAX_M; p++) {
      from[p] = to[p] = 0u;
      if (p > M) continue;
      const uint32_t b = __builtin_amdgcn_ubfe(k_lo, (uint32_t)(p * w), (uint32_t)w) | (__builtin_amdgcn_ubfe(k_hi, (uint32_t)(p * w), (uint32_t)w) << w);
      const uint32_t* o = a.near_offsets + (uint32_t)p * per_table + b;
      from[p] = o[0]; to[p] = o[1];
    }
#pragma unroll
    for (int p = 0; p <= NEAR_MAX_M; p++) {
      if (p > M) break;
      for (uint32_t i = from[p]; i < to[p]; i++) {
        uint4 q = a.near_members[i];
        // (one 16-byte load: left alone the compiler fetches the planes first and the index in a second, dependent load once the member counts)
        asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
        const uint32_t m = (k_lo ^ q.x) | (k_hi ^ q.y);
        const uint32_t d = (uint32_t)__builtin_popcount(m);
        bool counts = d <= (uint32_t)M;
#pragma unroll
        for (int e = 0; e < NEAR_MAX_M; e++)
          if (e < p) counts = counts && (m & (piece << (e * w))) != 0u;
        if constexpr (MODE == NEAR_LIST) {
          if (!counts) continue;
          const uint32_t len = a.wg_count[2u * q.z + 1u];
          if (len == NEAR_LIST_SKIP) continue;
          uint64_t sc = 1ull << 32;
          uint32_t left = m;
#pragma unroll
          for (int e = 0; e < NEAR_MAX_M; e++) {
            if (left == 0u) break;
            const uint32_t pos = (uint32_t)__builtin_ctz(left);
            left &= left - 1u;
            const uint32_t g = ((q.x >> pos) & 1u) | (((q.y >> pos) & 1u) << 1), t = ((k_lo >> pos) & 1u) | (((k_hi >> pos) & 1u) << 1);
            sc = (sc * model[near_model_index(pos, g, t)]) >> 16;
          }
          const uint32_t (&kb)[3] = minus ? s.km : s.kp;
          const uint32_t pam = ((kb[0] >> j) & 1u) | (((kb[1] >> j) & 1u) << 1) | (((kb[2] >> j) & 1u) << 2);
          const uint32_t tail = (minus ? (uint32_t)'-' : (uint32_t)'+') | ((pamless ? 0xFFu : pam) << 8) | (d << 16);
          const uint32_t slot = atomicAdd(&a.wg_count[2u * q.z], 1u);
          const uint64_t at = a.wg_offset[q.z] + slot;
          if (slot < len && at < a.out_capacity) {
            uint4* rec = reinterpret_cast<uint4*>(reinterpret_cast<NearHit*>(a.out) + at);
            rec[0] = make_uint4((uint32_t)sc, (uint32_t)(sc >> 32), contig, (uint32_t)(int32_t)(base0 + j));
            rec[1] = make_uint4(k_lo, k_hi, m, tail);
          } else {
            a.wg_count[2u * a.n_keys] = 1u;                 // the layout has no room for this pair: the error flag
          }
        } else if constexpr (!SCORE) {
          if (counts) (void)atomicAdd(&a.key_counts[q.z * row + d], 1ull);
        } else if (counts) {
          unsigned long long* out = a.key_counts + (uint64_t)q.z * row;
          (void)atomicAdd(&out[d], 1ull);
          if (d != 0u) {
            uint64_t sc = 1ull << 32;
            uint32_t left = m;
#pragma unroll
            for (int e = 0; e < NEAR_MAX_M; e++) {
              if (left == 0u) break;
              const uint32_t j = (uint32_t)__builtin_ctz(left);
              left &= left - 1u;
              const uint32_t g = ((q.x >> j) & 1u) | (((q.y >> j) & 1u) << 1), t = ((k_lo >> j) & 1u) | (((k_hi >> j) & 1u) << 1);
              sc = (sc * model[near_model_index(j, g, t)]) >> 16;           // (s <= 2^32, a factor <= 2^16: the product has 48 bits)
            }
            (void)atomicAdd(&out[M + 1], (unsigned long long)sc);
            (void)atomicMax(&out[M + 2], (unsigned long long)sc);
          }
        }
      }
    }
  }
}

// WRITE = false: pass 1 (counts); true: pass 2 (records).  KEYS (with neither): the match of pass 1 with the sites' keys looked up, KEYS_EXACT in the copies table (count_keys), KEYS_NEAR in the near buckets (near_keys).  FILTER: a.pat heads a SiteTables whose filter applies.  A SEGMENT is SITES_BLOCK_WORDS consecutive words, all of one tile, one lane
// per word; it is the unit of the counts and offsets.  A workgroup takes segs_per_wg consecutive segments, the next one's words on
// their way from memory while it matches the current one's (a workgroup per segment is bound by the rate at which workgroups start).
// KEYS_NEAR_SCORE: near_keys with the score; the model's packed table stands behind the near kernel's offsets in device memory and is
// copied to LDS once per workgroup, ahead of the first segment.
// KEYS_NEAR_LIST: near_keys with the records (calitas_list_near's second run of the pass); the model's table as in KEYS_NEAR_SCORE.
// KEYS_REGIONS (calitas_find_sites_regions; instantiated in site_regions.hip): the two find passes as they are, with one more reason
// for a segment to be dead -- a.presence, one byte per segment of the packed space, shares no bit with a.class_mask: no site that starts
// in the segment can have a wanted class.  Such a segment counts 0 and, its turn as the next segment included, loads no plane or mask word.
constexpr int KEYS_NONE = 0, KEYS_EXACT = 1, KEYS_NEAR = 2, KEYS_NEAR_SCORE = 3, KEYS_NEAR_LIST = 4, KEYS_REGIONS = 5;
// (a function's own LDS: it belongs to the one instantiation that calls this)
CAL_DEV uint32_t* near_model_lds() {
  __shared__ uint32_t s_model[NEAR_MODEL_WORDS];
  return s_model;
}
template <bool WRITE, bool FILTER, int KEYS = KEYS_NONE>
__global__ __launch_bounds__(SITES_BLOCK_WORDS) void sites_kernel(SitesArgs a) {
  __shared__ uint32_t s_lo[SITES_BLOCK_WORDS + 3], s_hi[SITES_BLOCK_WORDS + 3], s_ex[SITES_BLOCK_WORDS + 3];
  __shared__ uint32_t s_wave[SITES_BLOCK_WORDS / 64];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, wl = tid & 63u;
  const uint32_t seg0 = blockIdx.x * a.segs_per_wg, seg1 = min(seg0 + a.segs_per_wg, a.n_segs);
  constexpr bool LIST = KEYS == KEYS_NONE || KEYS == KEYS_REGIONS;     // the find passes: counts, offsets, records
  PatConst* pat = (PatConst*)a.pat;
  uint32_t* s_model = nullptr;
  if constexpr (KEYS == KEYS_NEAR_SCORE || KEYS == KEYS_NEAR_LIST) {
    static_assert(NEAR_MODEL_WORDS == 2 * SITES_BLOCK_WORDS, "two words per lane fill the table");
    s_model = near_model_lds();
    const uint32_t* g_model = a.near_offsets + near_model_offset(a.near_m, a.near_w);
    s_model[tid] = g_model[tid];
    s_model[tid + SITES_BLOCK_WORDS] = g_model[tid + SITES_BLOCK_WORDS];
    __syncthreads();
  }

  // dead tile, padding, another contig: nothing to do (wave-uniform)
  auto tile_of = [&](uint32_t seg) { return a.tiles[(a.w0 + (uint64_t)seg * SITES_BLOCK_WORDS) / a.tile_words]; };
  auto live = [&](const TileInfo ti) {
    return !(ti.flag == 2u || ti.contig == 0xFFFFFFFFu || (a.chrom_index >= 0 && ti.contig != (uint32_t)a.chrom_index));
  };
  // KEYS_REGIONS: some wanted class comes near the segment (seg < n_segs: the table covers the packed space)
  [[maybe_unused]] auto wanted = [&](uint32_t seg) { return (a.presence[a.w0 / SITES_BLOCK_WORDS + seg] & a.class_mask) != 0u; };
  // the words wb - 1 .. wb + 257 of a segment (wb >= one tile: the packed space starts with a tile of padding)
  auto fetch = [&](uint32_t seg) {
    Fetched f{make_uint2(0u, 0u), make_uint2(0u, 0u), 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (seg >= seg1 || !live(tile_of(seg))) return f;
    if constexpr (KEYS == KEYS_REGIONS) {
      if (!wanted(seg)) return f;
    }
    const uint64_t wb = a.w0 + (uint64_t)seg * SITES_BLOCK_WORDS;
    const uint64_t w = wb + tid, h = tid == 0 ? wb - 1 : wb + SITES_BLOCK_WORDS - 1 + tid;
    if (w < a.n_words) { f.pl = a.planes[w]; f.ex = a.mask[w]; }
    if (tid < 3u && h < a.n_words) { f.halo_pl = a.planes[h]; f.halo_ex = a.mask[h]; }
    return f;
  };

  uint32_t t_contig = 0xFFFFFFFFu, t_plus = 0u, t_minus = 0u;     // lane 0: sites of the segments so far, per strand, of one contig
  auto flush_totals = [&]() {
    if (t_plus) (void)atomicAdd(&a.totals[2 * t_contig], (unsigned long long)t_plus);
    if (t_minus) (void)atomicAdd(&a.totals[2 * t_contig + 1], (unsigned long long)t_minus);
    t_plus = t_minus = 0u;
  };

  Fetched f = fetch(seg0);
  for (uint32_t seg = seg0; seg < seg1; seg++) {
    const TileInfo ti = tile_of(seg);
    if (!live(ti)) {
      if (!WRITE && LIST && tid == 0) a.wg_count[seg] = 0u;
      f = fetch(seg + 1);
      continue;
    }
    if constexpr (KEYS == KEYS_REGIONS) {
      if (!wanted(seg)) {
        if (!WRITE && tid == 0) a.wg_count[seg] = 0u;
        f = fetch(seg + 1);
        continue;
      }
    }
    s_lo[tid + 1] = f.pl.x; s_hi[tid + 1] = f.pl.y; s_ex[tid + 1] = f.ex;
    if (tid < 3u) {
      const uint32_t i = tid == 0 ? 0u : SITES_BLOCK_WORDS + tid;
      s_lo[i] = f.halo_pl.x; s_hi[i] = f.halo_pl.y; s_ex[i] = f.halo_ex;
    }
    __syncthreads();
    uint32_t c_lo[4], c_hi[4], c_ex[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { c_lo[i] = s_lo[tid + i]; c_hi[i] = s_hi[tid + i]; c_ex[i] = s_ex[tid + i]; }
    f = fetch(seg + 1);

    const uint64_t wb = a.w0 + (uint64_t)seg * SITES_BLOCK_WORDS;
    const ContigInfo ci = a.contigs[ti.contig];
    const int64_t r_start = (int64_t)(a.start < ci.len ? a.start : ci.len);
    const int64_t r_end = (int64_t)((a.end == 0 || a.end > ci.len) ? ci.len : a.end);
    const int64_t base0 = (int64_t)((wb + tid) * 32u) - (int64_t)ci.gbase;
    const LaneSites s = match_word<FILTER>(pat, c_lo, c_hi, c_ex, base0, r_start, r_end);
    if constexpr (!LIST) {
      if constexpr (KEYS == KEYS_NEAR_LIST) near_keys<NEAR_LIST>(a, s, c_lo, c_hi, pat->proto_len, s_model, ti.contig, base0, pat->pamless != 0);
      else if constexpr (KEYS == KEYS_NEAR_SCORE) near_keys<NEAR_SCORE>(a, s, c_lo, c_hi, pat->proto_len, s_model);
      else if constexpr (KEYS == KEYS_NEAR) near_keys<NEAR_COUNT>(a, s, c_lo, c_hi, pat->proto_len, nullptr);
      else count_keys(a, s, c_lo, c_hi, pat->proto_len);
      __syncthreads();                                      // (every lane has its chain out of LDS before the next segment goes in)
      continue;
    }

    const uint32_t n_plus = (uint32_t)__builtin_popcount(s.plus), n_minus = (uint32_t)__builtin_popcount(s.minus);
    if (!WRITE) {
      // '+' in the low half, '-' in the high half: a segment has at most 8192 of each
      const uint32_t incl = wave_inclusive_sum(n_plus | (n_minus << 16));
      if (wl == 63u) s_wave[wave] = incl;
      __syncthreads();                                    // (also: every lane has its chain out of LDS before the next segment goes in)
      if (tid == 0) {
        const uint32_t t = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        a.wg_count[seg] = (t & 0xFFFFu) + (t >> 16);
        if (ti.contig != t_contig) { flush_totals(); t_contig = ti.contig; }
        t_plus += t & 0xFFFFu; t_minus += t >> 16;
      }
      continue;
    }
    const uint32_t mine = n_plus + n_minus;
    const uint32_t incl = wave_inclusive_sum(mine);
    if (wl == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint64_t at = a.wg_offset[seg] + (incl - mine);
    for (uint32_t v = 0; v < wave; v++) at += s_wave[v];
    const int pamless = pat->pamless, proto_len = pat->proto_len;
    uint32_t any = s.plus | s.minus;
    while (any) {
      const uint32_t j = (uint32_t)__builtin_ctz(any);
      any &= any - 1u;
      const int32_t p = (int32_t)(base0 + j);
#pragma unroll
      for (int st = 0; st < 2; st++) {
        if (!(((st ? s.minus : s.plus) >> j) & 1u)) continue;
        const uint32_t (&kb)[3] = st ? s.km : s.kp;
        const uint32_t k = ((kb[0] >> j) & 1u) | (((kb[1] >> j) & 1u) << 1) | (((kb[2] >> j) & 1u) << 2);
        const SitePattern* sp = &a.pat->p[k][st];                              // (per lane: an ordinary load)
        const int pam_len = sp->pam_len;
        SiteRecord r;
        r.contig = (int32_t)ti.contig; r.proto_start = p; r.pam_start = pamless ? -1 : p + sp->pam_off;
        r.strand = st ? '-' : '+'; r.pam_index = pamless ? (int8_t)-1 : (int8_t)k; r.pam_len = (uint8_t)pam_len; r.proto_len = (uint8_t)proto_len;
        static_assert(sizeof(SiteRecord) == 16, "one 16-byte store per record");
        if (at < a.out_capacity) *reinterpret_cast<uint4*>(&a.out[at]) = *reinterpret_cast<const uint4*>(&r);
        at++;
      }
    }
  }
  if (!WRITE && LIST && tid == 0) flush_totals();
}

// near_list.hip takes everything above -- for its one instantiation, KEYS_NEAR_LIST -- by including this file with
// CALITAS_SITES_KERNEL_ONLY defined: its kernels get a code object of their own, and this file's stays what it was without them.
#ifndef CALITAS_SITES_KERNEL_ONLY
// Exclusive scan of the workgroups' counts by one workgroup: a stretch per thread, the stretches' sums scanned in LDS.
constexpr int OFFSETS_THREADS = 1024;
__global__ __launch_bounds__(OFFSETS_THREADS) void sites_offsets_kernel(const uint32_t* wg_count, uint64_t* wg_offset, uint32_t n) {
  __shared__ uint64_t s_sum[OFFSETS_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + OFFSETS_THREADS - 1) / OFFSETS_THREADS;
  const uint64_t b = (uint64_t)tid * per, e = b + per < n ? b + per : n;
  uint64_t sum = 0;
  for (uint64_t i = b; i < e; i++) sum += wg_count[i];
  s_sum[tid] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < OFFSETS_THREADS; d <<= 1) {      // inclusive scan, Hillis-Steele
    const uint64_t add = tid >= d ? s_sum[tid - d] : 0;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  uint64_t run = s_sum[tid] - sum;
  for (uint64_t i = b; i < e; i++) { wg_offset[i] = run; run += wg_count[i]; }
  if (tid == OFFSETS_THREADS - 1) wg_offset[n] = s_sum[tid];
}

#endif
}  // namespace

#ifndef CALITAS_SITES_KERNEL_ONLY
hipError_t launch_sites_count(const SitesArgs& a, bool filtered, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  if (filtered) hipLaunchKernelGGL((sites_kernel<false, true>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  else hipLaunchKernelGGL((sites_kernel<false, false>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sites_offsets(const uint32_t* wg_count, uint64_t* wg_offset, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(sites_offsets_kernel, dim3(1), dim3(OFFSETS_THREADS), 0, stream, wg_count, wg_offset, n);
  return hipGetLastError();
}

hipError_t launch_sites_write(const SitesArgs& a, bool filtered, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  if (filtered) hipLaunchKernelGGL((sites_kernel<true, true>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  else hipLaunchKernelGGL((sites_kernel<true, false>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sites_copies(const SitesArgs& a, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  hipLaunchKernelGGL((sites_kernel<false, false, KEYS_EXACT>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sites_near(const SitesArgs& a, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  hipLaunchKernelGGL((sites_kernel<false, false, KEYS_NEAR>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sites_near_score(const SitesArgs& a, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  hipLaunchKernelGGL((sites_kernel<false, false, KEYS_NEAR_SCORE>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

#endif
}  // namespace calitas
