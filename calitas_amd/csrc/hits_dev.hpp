// hits_dev.hpp -- device code and scratch shared by hits.hip (the general removeOverlaps / sort / rows kernels) and binned.hip (the
// same stages fused per reference bin): the hit record, its coordinates, the ownership key and ReferenceHit.sort's comparison, a row's
// length, the wave-per-row builder of a hits.txt row's middle part and the copy-out of the finished row.
// Private to those two translation units (everything sits in an anonymous namespace there).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/calitas_hip.h"
#include "common.hpp"
#include "hits.hpp"
#include "mailbox.hpp"
#include "refpack.hpp"

namespace calitas {

namespace {

constexpr int SCORE_BITS = 14;
constexpr uint32_t CLUSTER_MAX = 1u << 20;

struct HitRec {
  int32_t contig, start, end, gstart, gend, score, rh_end;
  uint32_t minus;
};

struct RowConstDev {
  uint32_t head_off, head_len, tail_off, tail_len, plen_off, plen_len;
  uint32_t q_off[MAX_PAMS + 1], q_len[MAX_PAMS + 1], pu_off[MAX_PAMS + 1], pu_len[MAX_PAMS + 1];
};

// GuideAlignment coordinates (GA:21-31 with the '+' rule in aligner space, mapped per SGA:260-313) and ReferenceHit.end (RH:135-138)
// of one accepted alignment.
__device__ __forceinline__ HitRec hit_record(const RawAln* rp, const GuideDev* guides, const uint64_t* win_base, const int2* win) {
  struct { uint32_t contig, window_k; int32_t score; int t_start, t_end_guide, dir, guide, pam, offset, n_ops; } r;
  r.contig = rp->contig; r.window_k = rp->window_k; r.score = rp->score; r.t_start = rp->t_start; r.t_end_guide = rp->t_end_guide;
  r.dir = rp->dir; r.guide = rp->guide; r.pam = rp->pam; r.offset = rp->offset; r.n_ops = rp->n_ops;
  const GuideDev& g = guides[r.guide];
  const int ng = r.n_ops;
  int pam_len = 0, gap = 0;
  if (r.pam >= 0) { pam_len = g.pam_len[r.pam]; gap = r.offset; }
  // aligner-order op k is traceback op ng - 1 - k.  Everything left of the first / right of the last protospacer column is 'D'
  // (GA:21-31 with the '+' rule in aligner space, SGA:264,281,297,302).
  const OpCounts oc = count_ops(load_ops_words(rp->ops), ng);
  int lead = oc.lead_d, trail = oc.trail_d;
  const int t_guide = oc.not_ins;
  if (lead == ng) { lead = 0; trail = ng; }            // no protospacer column at all: cannot happen, kept total
  const int left_delta = lead, right_delta = trail + gap + pam_len;
  const int tlen = t_guide + gap + pam_len;
  const int start_s = (int)r.t_start - 1, end_s = (int)r.t_end_guide + r.offset + pam_len;   // SGA:515-516
  const int gstart_s = start_s + left_delta, gend_s = end_s - right_delta;
  const int2 w = win[win_base[r.contig] + r.window_k];
  HitRec h;
  h.contig = (int32_t)r.contig; h.score = r.score;
  if (r.dir == 0) { h.start = w.x + start_s; h.end = w.x + end_s; h.gstart = w.x + gstart_s; h.gend = w.x + gend_s; }   // SGA:297, 281
  else            { h.start = w.y - end_s; h.end = w.y - start_s; h.gstart = w.y - gend_s; h.gend = w.y - gstart_s; }   // SGA:303-309, 271-274
  const bool plus = g.pam5 ? (r.dir == 1) : (r.dir == 0);
  h.minus = plus ? 0u : 1u;
  h.rh_end = h.gstart + tlen - 1;                      // RH:135-138
  return h;
}

// (The four stages below exist as functions of one index: each has a kernel of its own, and hits_small_kernel runs them one after
// the other in a single workgroup when the call has at most HITS_SMALL alignments -- four launches less on the path of a small call.)
__device__ __forceinline__ void hit_body(const uint32_t i, const RawAln* fin, const GuideDev* guides, const uint64_t* win_base, const int2* win,
                                         int score_hi, HitRec* hits, uint64_t* keys, uint32_t* vals, uint32_t* wks, uint32_t* flags) {
  const HitRec h = hit_record(fin + i, guides, win_base, win);
  hits[i] = h;
  int sb = score_hi - h.score;
  if (sb < 0 || sb >= (1 << SCORE_BITS) || h.gstart < 0) { atomicOr(flags, HITS_FLAG_SCORE_RANGE); sb = 0; }
  keys[i] = ((uint64_t)(uint32_t)h.contig << 46) | ((uint64_t)(uint32_t)h.gstart << 15) | ((uint64_t)h.minus << 14) | (uint64_t)sb;
  vals[i] = i;
  wks[i] = fin[i].window_k;
}

constexpr int HIT_MAX_LEN = CALITAS_MAX_OPS;   // a hit covers at most this many reference bases (ReferenceHit.end - start + 1)

// What HitsOwn / BinnedParams hold a hit against: (contig << 32 | coordinate_start), owned when it lies in [own_lo, own_hi).
__device__ __forceinline__ unsigned long long own_key(uint32_t contig, int32_t gstart) { return ((unsigned long long)contig << 32) | (uint32_t)gstart; }

// ReferenceHit.sort (RH:284) between two hits of one contig: does (gs, mi, sc) = (start, strand, score) come before hit h -- start and
// strand ascending, score descending --, or is it the same key?  (The counting sorts of binned.hip; arrival order breaks the tie there.)
struct SortCmp { bool less, same; };
__device__ __forceinline__ SortCmp sort_cmp(int gs, uint32_t mi, int sc, int h_gs, uint32_t h_mi, int h_sc) {
  return SortCmp{gs < h_gs || (gs == h_gs && (mi < h_mi || (mi == h_mi && sc > h_sc))), gs == h_gs && mi == h_mi && sc == h_sc};
}

// ---- rows ------------------------------------------------------------------------------------------------------------
// A row is  head | chromosome \t | middle | tail  where head and tail are the same for every row of the call.  One *wave* per row:
// build_middle lays the middle part out in the wave's LDS line (lane i owns padded column i of the alignment, lane f field f's length and
// digits), write_row copies the four pieces to the row's final place with coalesced byte stores; middle_length is build_middle's
// arithmetic for one lane, for the kernels that place the rows before they are built (DESIGN.md 4.4 has the history).

__device__ __forceinline__ char comp_base(char c) {   // fgbio Sequences.complement on an upper-case base
  switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'U': return 'A';
    case 'M': return 'K'; case 'K': return 'M'; case 'R': return 'Y'; case 'Y': return 'R';
    case 'V': return 'B'; case 'B': return 'V'; case 'H': return 'D'; case 'D': return 'H';
    default: return c;
  }
}

// "ACGT"[code] and "=XID"[op] from a constant in a register (indexing the string literals is a load from constant memory per character)
__device__ __forceinline__ char base_letter(uint32_t code) { return (char)((0x54474341u >> (8u * code)) & 0xFFu); }   // A C G T
__device__ __forceinline__ char op_letter(int op) { return (char)((0x4449583Du >> (8 * op)) & 0xFFu); }               // = X I D

__device__ char base_upper_dev(const HitsRef& ref, uint64_t gpos) {
  if ((ref.mask[gpos >> 5] >> (gpos & 31)) & 1u) {
    const int64_t r = run_floor(ref.runs, ref.n_runs, gpos);
    uint8_t ch = 0;
    if (r >= 0 && gpos < ref.runs[r].start + ref.runs[r].len) ch = ref.runs[r].ch;
    if (ch == 0) return 'N';
    return (char)((ch >= 'a' && ch <= 'z') ? ch - 32 : ch);
  }
  return base_letter((ref.codes[gpos >> 4] >> ((gpos & 15) * 2)) & 3u);
}

constexpr int HITS_BOX_LATE = 8;      // word of the work's mailbox for flags raised while rows are written (the post uses words 0..6)
constexpr int MID_COLS = 64;          // padded columns a row may have on this path: one per lane
constexpr int MID_LINE = 6 * MID_COLS + 128;   // bytes of a wave's line buffer = the largest mid_bound
constexpr int MID_FWD = 128;          // reference bases staged per row: the alignment and its flanks
constexpr int MID_FIELDS = 25;

struct MidArgs {
  HitsRef ref;
  RowConstDev rc;
  const char* blob;
  const uint32_t* name_off;
  const RawAln* fin;
  const HitRec* hits;
  const GuideDev* guides;
  const uint8_t* keep;       // per sorted position: survives removeOverlaps
  const uint32_t* order;     // sorted values: index into fin / hits
  uint32_t n;
  uint32_t mid_bound;        // bytes reserved for the middle part = staging stride (<= MID_LINE)
  uint32_t n_max;            // most padded columns a row of this search can have (<= MID_COLS)
  uint32_t blob_bytes;       // constant strings, copied to LDS by each block
  uint32_t* n_rows;          // out: number of live rows
  uint32_t n_dev;            // order[k] >= n_dev: a hit the caller built (HitsExt) -- no row to build, its length comes from ext_off
  const uint64_t* ext_off;
  uint32_t* ext_kept;        // out: how many of those were kept
  unsigned long long own_lo, own_hi;   // HitsOwn: rows only for hits with own_lo <= (contig << 32 | coordinate_start) < own_hi (0 / ~0: all)
};

static_assert(offsetof(RawAln, ops) % 4 == 0 && sizeof(RawAln) % 4 == 0, "RawAln::ops must be word aligned");

struct RowIn {             // the fields of one RawAln a row needs, ops as five words (2 bits per op, traceback order)
  uint32_t w0, w1, w2, w3, w4;
  int n_ops, pam, offset;
  uint32_t pam_x;
};
static_assert(RAW_MAX_OPS / 16 == 5, "RowIn holds five ops words");
struct RowGuide { int L, pam5, pam_len; };   // what a row needs of its GuideDev (pam_len: of the row's PAM, 0 without one)

// op i of the row: the word is chosen by comparison (the five words are wave-uniform and live in scalar registers; indexing them
// as an array made the compiler spill them to scratch and load per lane)
__device__ __forceinline__ int row_op(const uint32_t w0, const uint32_t w1, const uint32_t w2, const uint32_t w3, const uint32_t w4, int i) {
  const int k = i >> 4;
  uint32_t w = w0;
  w = (k == 1) ? w1 : w; w = (k == 2) ? w2 : w; w = (k == 3) ? w3 : w; w = (k == 4) ? w4 : w;
  return (int)((w >> ((i & 15) * 2)) & 3u);
}

// Read-only inputs of a row are the same for all lanes of its wave: through the constant address space they are scalar loads into
// scalar registers (everything they point to was written by earlier kernels).
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* uniform_ptr(const T* p) {
  return (const __attribute__((address_space(4))) T*)p;
}

__device__ __forceinline__ void wave_lds_sync() {       // LDS writes of this wave visible to all its lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long bits_below(int i) { return i >= 64 ? ~0ull : (1ull << i) - 1ull; }
// number of set bits of a wave-uniform mask below this lane: two instructions (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ int bits_before_lane(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// `v` (wave-uniform) in lane L, `old` elsewhere: one v_writelane_b32
template <int L>
__device__ __forceinline__ int set_lane(int v, int old) {
  asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(v), "n"(L));
  return old;
}

// The middle part of one hits.txt row (RH:210-254, columns coordinate_start .. unpadded_target_sequence_length) in `line`, built by
// the 64 lanes of a wave; every argument but `lane` is the same in all of them.  `fwd` holds MID_FWD bytes, `blob` is the LDS copy
// of the constant strings.  Returns the length, or -1 when the row has more columns (or a longer span) than this path lays out.
// EMIT = false: only the length (the same arithmetic, nothing fetched or written; line / fwd may be null) -- what the binned path needs
// to place a row before it is built.
template <bool EMIT = true>
__device__ __forceinline__ int build_middle(uint8_t* line, uint8_t* fwd, const MidArgs& a, const uint8_t* blob, const RowIn r, const HitRec h,
                                            const RowGuide g, const int lane) {
  const int pam_len = g.pam_len, gap = r.pam >= 0 ? r.offset : 0;
  const int ng = r.n_ops, n = ng + gap + pam_len;
  const bool minus = h.minus != 0;
  // one fetch covers the alignment and all four flanks (RH:213-216); a minus-strand hit keeps the complemented bases: every
  // reader below wants them in guide orientation
  const int lo = min(h.start - 8, h.gstart - 10), hi = max(h.end + 8, h.gend + 10);
  if (n > (int)a.n_max || n > MID_COLS || hi - lo > MID_FWD) return -1;
  if (EMIT) {
    const uint64_t c_gbase = uniform_ptr(a.ref.contigs)[h.contig].gbase, c_len = uniform_ptr(a.ref.contigs)[h.contig].len;
    for (int x = lane; x < hi - lo; x += 64) {
      const int64_t p = (int64_t)lo + x;
      char b = 'N';                                                                          // RH:262-264
      if (p >= 0 && p < (int64_t)c_len) b = base_upper_dev(a.ref, c_gbase + (uint64_t)p);
      if (minus) b = comp_base(b);
      fwd[x] = (uint8_t)b;
    }
  }
  // ---- column `lane` of the alignment in guide orientation: guide part (stored in traceback order), gap to the PAM, PAM
  //      (SGA:472-476); reversed for a 5' PAM (SGA:267-269)
  const bool valid = lane < n;
  int op = 0;                                             // 0 '=', 1 'X', 2 'I', 3 'D'
  {
    const int k = g.pam5 ? n - 1 - lane : lane;
    const int guide_op = row_op(r.w0, r.w1, r.w2, r.w3, r.w4, ng - 1 - k), pam_op = (int)((r.pam_x >> ((k - ng - gap) & 15)) & 1u);
    op = k < ng ? guide_op : k < ng + gap ? 3 : pam_op;
    if (!valid) op = 0;
  }
  const unsigned long long MX = __ballot(valid && op == 1), MI = __ballot(valid && op == 2), MD = __ballot(valid && op == 3);
  const unsigned long long V = bits_below(n), nonD = V & ~MD, nonI = V & ~MI;
  const int qi = bits_before_lane(nonD), ti = bits_before_lane(nonI);
  // Alignment.paddedString (SGA:511): query, alignment and target character of this column
  const uint8_t* q = blob + a.rc.q_off[r.pam + 1];
  char qc = '-';
  if (valid && op != 3) qc = (char)q[qi];
  const bool q_low = valid && qc >= 'a', q_up = valid && qc >= 'A' && qc <= 'Z';   // (the query holds letters only: lower = the PAM)
  const unsigned long long ML = __ballot(q_low), MU = __ballot(q_up);
  const char ac = op == 0 ? '|' : op == 1 ? '.' : '~';
  wave_lds_sync();                                        // fwd[] is complete
  // j-th target base of the alignment in guide orientation
  const int t_first = minus ? h.end - 1 - lo : h.start - lo, t_step = minus ? -1 : 1;
  char tc = '-';
  if (EMIT && valid && op != 2) tc = (char)fwd[t_first + t_step * ti];
  // unpaddedTargetWithoutPam (GA:111-115): the target bases under the first .. last upper-case query column
  const int ps = MU ? __ffsll((long long)MU) - 1 : 0, pe = MU ? 63 - __clzll((long long)MU) : -1;
  const unsigned long long span_cols = bits_below(pe + 1) & ~bits_below(ps);
  const int utn = __popcll(nonI & span_cols), ut0 = __popcll(nonI & bits_below(ps));
  // GuideAlignment.count (GA:139-163) as ballots.  Mismatches: '.' columns by the case of the query base.  Gaps ('~' columns): an
  // inserted query base counts by its own case; a deleted one ('-' in the padded guide) by its nearest non-dash neighbours
  // (previousNonDash / nextNonDash, GA:168-182: the scan stops at the first / last column, which is then a dash itself).
  const int gmm = __popcll(MX & ~ML), pam_mm = __popcll(MX & ML), edits = __popcll(MX | MI | MD);
  bool guide_gap = valid && op == 2 && !q_low;            // is_lower(pg[i]) == false
  if (valid && op == 3) {                                 // (no lane gets here in a row without deletions)
    const unsigned long long below = bits_below(lane), left = nonD & below, right = nonD & ~below;   // (this column is not in nonD)
    const bool prev_up = left != 0 && ((MU >> (63 - __clzll((long long)left))) & 1ull);
    const bool next_up = right != 0 && ((MU >> (__ffsll((long long)right) - 1)) & 1ull);
    guide_gap = prev_up || next_up;                       // both_sides = false, lower = false: an upper-case letter on either side
  }
  const int ggp = __popcll(__ballot(guide_gap));
  // Cigar.coalesce + toString: a run starts where the op changes; its text is the length and the op letter
  const int op_prev = __builtin_amdgcn_update_dpp(op, op, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  const bool run_start = valid && (lane == 0 || op != op_prev);
  const unsigned long long RS = __ballot(run_start);
  int run_len = 0;
  {
    // next run start above this lane: clear bits 0..lane of RS (lane-dependent shift of a uniform mask)
    const unsigned long long nx = lane >= 63 ? 0ull : (RS >> (lane + 1));
    run_len = nx ? __ffsll((long long)nx) : n - lane;
  }
  const unsigned long long RL = __ballot(run_start && run_len >= 10);       // (a run has at most 64 columns: one or two digits)
  const int cigar_len = 2 * __popcll(RS) + __popcll(RL);
  // ---- the 25 fields: lane f holds the length of field f (every field is followed by a tab) and, for a number, its value
  const int pu_len = (int)a.rc.pu_len[r.pam + 1];
  int flen = 0, val = 0;
  flen = set_lane<2>(1, flen);                            // strand
  flen = set_lane<3>(utn, flen);                          // unpadded target without PAM
  flen = set_lane<4>(10, flen); flen = set_lane<5>(10, flen);    // 10-base flanks of the hit (RH:227-228)
  flen = set_lane<6>(pu_len, flen);                       // pam_used; 7-10: variant_id, variant_description, variant_vcf, allele_frequency: None
  flen = set_lane<17>(n, flen); flen = set_lane<18>(n, flen); flen = set_lane<19>(n, flen);   // padded guide, alignment string, padded target
  flen = set_lane<20>(8, flen); flen = set_lane<21>(8, flen);    // 8-base flanks of the alignment (RH:243-244)
  flen = set_lane<22>(cigar_len, flen);
  val = set_lane<0>(h.gstart, val); val = set_lane<1>(h.gend, val); val = set_lane<11>(h.score, val);
  val = set_lane<12>(gmm, val);                           // guide_mm GA:103
  val = set_lane<13>(ggp, val);                           // guide_gaps GA:104
  val = set_lane<14>(gmm + ggp, val);                     // guide_mm_plus_gaps GA:105
  val = set_lane<15>(pam_mm, val);                        // pam_mm GA:106
  val = set_lane<16>(edits, val);                         // total_mm_plus_gaps = edits GA:101
  val = set_lane<23>(g.L, val);                           // unpadded_guide_sequence_length
  val = set_lane<24>(utn, val);
  const bool numeric = (0x0181F803u >> (lane & 31)) & (lane < 32 ? 1u : 0u);   // fields 0 1 11-16 23 24
  unsigned uval = (unsigned)(val < 0 ? -val : val);
  const int nd = 1 + (uval >= 10u) + (uval >= 100u) + (uval >= 1000u) + (uval >= 10000u) + (uval >= 100000u) + (uval >= 1000000u) +
                 (uval >= 10000000u) + (uval >= 100000000u) + (uval >= 1000000000u);
  if (numeric) flen = nd + (val < 0 ? 1 : 0);
  int incl = lane < MID_FIELDS ? flen + 1 : 0;            // inclusive prefix sum over the field lanes
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  const int foff = incl - (flen + 1);
  const int total = __builtin_amdgcn_readlane(incl, MID_FIELDS - 1);
  if (total > (int)a.mid_bound) return -1;
  if (!EMIT) return total;
  if (lane < MID_FIELDS) line[foff + flen] = '\t';
  if (numeric) {
    uint8_t* w = line + foff;
    if (val < 0) *w++ = '-';
    for (int i = nd - 1; i >= 0; i--) { const unsigned t = uval / 10u; w[i] = (uint8_t)('0' + (uval - 10u * t)); uval = t; }
  }
  auto off_of = [&](int f) { return __builtin_amdgcn_readlane(foff, f); };
  // bases [from, to) of the forward strand in guide orientation (flanks): a minus-strand hit reads them backwards
  auto put_bases = [&](int off, int from, int to) {
    if (lane < to - from) line[off + lane] = fwd[minus ? to - 1 - lane - lo : from + lane - lo];
  };
  const int o2 = off_of(2), o3 = off_of(3), o4 = off_of(4), o5 = off_of(5), o6 = off_of(6), o17 = off_of(17), o18 = off_of(18), o19 = off_of(19),
            o20 = off_of(20), o21 = off_of(21), o22 = off_of(22);
  if (lane == 0) line[o2] = minus ? '-' : '+';
  if (lane < utn) line[o3 + lane] = fwd[t_first + t_step * (ut0 + lane)];
  const int gs = h.gstart, ge = h.gend, as = h.start, ae = h.end;
  if (!minus) { put_bases(o4, gs - 10, gs); put_bases(o5, ge, ge + 10); put_bases(o20, as - 8, as); put_bases(o21, ae, ae + 8); }
  else        { put_bases(o4, ge, ge + 10); put_bases(o5, gs - 10, gs); put_bases(o20, ae, ae + 8); put_bases(o21, as - 8, as); }
  if (lane < pu_len) line[o6 + lane] = blob[a.rc.pu_off[r.pam + 1] + lane];
  if (valid) { line[o17 + lane] = (uint8_t)qc; line[o18 + lane] = (uint8_t)ac; line[o19 + lane] = (uint8_t)tc; }
  if (run_start) {
    uint8_t* w = line + o22 + 2 * bits_before_lane(RS) + bits_before_lane(RL);
    if (run_len >= 10) *w++ = (uint8_t)('0' + run_len / 10);
    *w++ = (uint8_t)('0' + run_len % 10);
    *w = (uint8_t)op_letter(op);
  }
  return total;
}

// The RowIn of an alignment and the RowGuide of its guide: scalar loads.
__device__ __forceinline__ RowIn load_row_in(const RawAln* p) {
  const auto* rp = uniform_ptr(p);
  RowIn r;
  const auto* ow = (const __attribute__((address_space(4))) uint32_t*)rp->ops;   // RawAln::ops sits at a 4-byte aligned offset
  r.w0 = ow[0]; r.w1 = ow[1]; r.w2 = ow[2]; r.w3 = ow[3]; r.w4 = ow[4];
  r.n_ops = rp->n_ops; r.pam = rp->pam; r.offset = rp->offset; r.pam_x = rp->pam_x;
  return r;
}
__device__ __forceinline__ RowGuide row_guide(const GuideDev* p, int pam) {
  const auto* gp = uniform_ptr(p);
  return RowGuide{gp->L, gp->pam5, pam >= 0 ? gp->pam_len[pam] : 0};
}

// A row's middle part in the wave's line buffer, held against the length `want` its sizing kernel computed for it.  The two cannot
// differ (both run the same arithmetic); if they do, `flag` is raised in the mailbox word `late` and the row must not be written: -1.
__device__ __forceinline__ int checked_middle(uint8_t* line, uint8_t* fwd, const MidArgs& a, const uint8_t* blob, const RowIn& r, const HitRec& h,
                                              const RowGuide& g, const int lane, uint32_t want, uint32_t* late, uint32_t flag) {
  wave_lds_sync();                                        // the copy-out of the previous row is done with line[]
  const int len = build_middle<true>(line, fwd, a, blob, r, h, g, lane);
  if (len < 0 || (uint32_t)len != want) {
    if (lane == 0) __hip_atomic_fetch_or(late, flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return -1;
  }
  wave_lds_sync();
  return len;
}

// head | chromosome \t | middle | tail at dst, by the 64 lanes of a wave: line[0..len) is the middle part, head and tail lie in `blob`.
// Returns the row's length (row_length of the same row).
__device__ __forceinline__ uint32_t write_row(char* dst, const uint8_t* line, uint32_t len, int32_t contig, const RowConstDev& rc, const uint8_t* blob,
                                              const char* names, const uint32_t* name_off, const int lane) {
  const uint8_t* head = blob + rc.head_off;
  const uint8_t* tail = blob + rc.tail_off;
  const uint32_t nb = uniform_ptr(name_off)[contig], nl = uniform_ptr(name_off)[contig + 1] - nb;
  const uint32_t s0 = rc.head_len, s1 = s0 + nl + 1, s2 = s1 + len, total = s2 + rc.tail_len;
  for (uint32_t x = (uint32_t)lane; x < total; x += 64) {
    uint8_t ch;
    if (x < s0) ch = head[x];
    else if (x < s1) ch = (x - s0 < nl) ? (uint8_t)names[nb + x - s0] : (uint8_t)'\t';
    else if (x < s2) ch = line[x - s1];
    else ch = tail[x - s2];
    dst[x] = (char)ch;
  }
  return total;
}

// Device scratch of at least `need` elements: a quarter more than asked for, or exactly that (slack = false: sized by the reference, not the call).
template <typename T>
hipError_t grow(T** p, size_t& cap, size_t need, bool slack = true) {
  if (need <= cap) return hipSuccess;
  (void)hipFree(*p); *p = nullptr; cap = 0;
  if (slack) need += need / 4;
  hipError_t e = hipMalloc((void**)p, need * sizeof(T));
  if (e == hipSuccess) cap = need;
  return e;
}
// The same in page-locked host memory.
template <typename T>
hipError_t grow_pinned(T** p, size_t& cap, size_t need) {
  if (need <= cap) return hipSuccess;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr; cap = 0; need += need / 4 + 4096;
  hipError_t e = hipHostMalloc((void**)p, need * sizeof(T), hipHostMallocDefault);
  if (e == hipSuccess) cap = need;
  return e;
}

// MidArgs::n_max and MidArgs::mid_bound of a search whose alignments have at most max_ops padded columns.
struct MidSize { uint32_t n_max, mid_bound; };
inline MidSize mid_size(int max_ops) {
  const uint32_t n_max = (uint32_t)std::min<int>(MID_COLS, std::max(1, max_ops));
  return MidSize{n_max, (6 * n_max + 128 + 3) & ~3u};
}


}  // namespace

// guide_mm, guide_gaps and pam_mm of a hit (the hits.txt columns, GA:103, 104, 106) from the alignment's op counts -- the one place this
// arithmetic lives: middle_length formats the three into a row's length, the counts kernels (counts_kernel, bin_counts_kernel) make a
// table cell of them.
struct HitKey { int guide_mm, guide_gaps, pam_mm; };
__device__ __forceinline__ HitKey hit_key(const OpCounts& oc, int pam, int offset, uint32_t pam_x) {
  const int gap = pam >= 0 ? offset : 0;
  HitKey k;
  k.guide_mm = oc.non_eq - oc.gaps;                      // 'X' columns by the case of the query base (GA:103)
  k.pam_mm = pam >= 0 ? __popc(pam_x) : 0;               // GA:106
  k.guide_gaps = oc.gaps + gap;                          // every gap column has a protospacer base on one side (GA:104, 168-182)
  return k;
}

// Length of the middle part of a row = what build_middle computes with ballots, for one lane: the field lengths of RH:210-254 from
// the alignment's op counts (GA:99-115, 139-183) and the run-length encoding of its cigar.  -1: the row builder does not lay it out.
__device__ __forceinline__ int middle_length(const MidArgs& a, const RawAln* rp, const HitRec& h) {
  const GuideDev* gp = a.guides + rp->guide;
  const int ng = rp->n_ops, pam = rp->pam;
  const int L = gp->L, pam_len = pam >= 0 ? gp->pam_len[pam] : 0, pu_len = (int)a.rc.pu_len[pam + 1], n_max = (int)a.n_max, mid_bound = (int)a.mid_bound;
  const int gap = pam >= 0 ? rp->offset : 0;
  const uint32_t pam_x = rp->pam_x;
  const int n = ng + gap + pam_len;
  const int lo = min(h.start - 8, h.gstart - 10), hi = max(h.end + 8, h.gend + 10);
  if (n > n_max || n > MID_COLS || hi - lo > MID_FWD) return -1;
  const OpsWords ow = load_ops_words(rp->ops);
  const OpCounts oc = count_ops(ow, ng);
  const int utn = oc.not_ins - oc.lead_d - oc.trail_d;                 // target bases under the first .. last protospacer column (GA:111-115)
  const HitKey hk = hit_key(oc, pam, rp->offset, pam_x);
  const int gmm = hk.guide_mm, pam_mm = hk.pam_mm, ggp = hk.guide_gaps;
  const int edits = oc.non_eq + gap + pam_mm;                          // GA:101
  // Cigar.coalesce + toString over the columns: guide part (aligner order = traceback order reversed), the gap, the PAM; the number of
  // runs and of two-digit run lengths does not depend on the direction the columns are read in (5' PAM)
  int runs = 0, long_runs = 0, prev = -1, len = 0;
  for (int k = 0; k < n; k++) {
    const int op = k < ng ? ow.op(ng - 1 - k) : k < ng + gap ? 3 : (int)((pam_x >> ((k - ng - gap) & 15)) & 1u);
    if (op != prev) { if (len >= 10) long_runs++; runs++; len = 0; prev = op; }
    len++;
  }
  if (len >= 10) long_runs++;
  const int cigar_len = 2 * runs + long_runs;
  auto digits = [](int v) {
    const unsigned u = (unsigned)(v < 0 ? -v : v);
    return (v < 0 ? 1 : 0) + 1 + (u >= 10u) + (u >= 100u) + (u >= 1000u) + (u >= 10000u) + (u >= 100000u) + (u >= 1000000u) + (u >= 10000000u) +
           (u >= 100000000u) + (u >= 1000000000u);
  };
  const int total = MID_FIELDS + digits(h.gstart) + digits(h.gend) + 1 + utn + 10 + 10 + pu_len + digits(h.score) + digits(gmm) + digits(ggp) +
                    digits(gmm + ggp) + digits(pam_mm) + digits(edits) + 3 * n + 8 + 8 + cigar_len + digits(L) + digits(utn);
  return total > mid_bound ? -1 : total;
}

// The length of the whole row around a middle part of middle_len bytes -- what write_row returns for it.
__device__ __forceinline__ uint32_t row_length(const RowConstDev& rc, const uint32_t* name_off, int32_t contig, uint32_t middle_len) {
  return rc.head_len + (name_off[contig + 1] - name_off[contig]) + 1 + middle_len + rc.tail_len;
}

// ---- the off-target table (calitas_search_counts) ---------------------------------------------------------------------------------
// Both counts kernels work the same way: a histogram per workgroup in LDS (non-returning ds_add_u32), its non-zero cells flushed once
// into the call's table in device memory (non-returning 64-bit adds), and the workgroup that finishes last -- a ticket per workgroup,
// never an atomic whose value a hit waits for -- writes the table into page-locked host memory, clears table and ticket for the next
// call and posts the lane's mailbox: the host reads the table behind the wait it makes anyway.  A table with more cells than
// COUNTS_LDS_CELLS (extents of a search with very many differences) adds every hit to the device table directly: slower, same table.
constexpr uint32_t COUNTS_LDS_CELLS = 4096;    // 16 KB of a workgroup's LDS
constexpr uint32_t COUNTS_BLOCK = 256;

struct CountsOut {
  CountsShape shape;
  uint32_t cells;
  unsigned long long* table;   // device memory, `cells` words: zero at launch, zero again when the kernel ends
  uint32_t* tickets;           // one word, likewise
  unsigned long long* host;    // page-locked host memory, `cells` words
};

// The cell of a hit, or -1 when it lies outside the extents.
__device__ __forceinline__ int counts_cell(const RawAln* rp, uint32_t minus, const CountsShape& s) {
  const OpCounts oc = count_ops(load_ops_words(rp->ops), rp->n_ops);
  const HitKey k = hit_key(oc, rp->pam, rp->offset, rp->pam_x);
  if (k.guide_mm < 0 || k.guide_gaps < 0 || (uint32_t)k.guide_mm >= s.n_mm || (uint32_t)k.guide_gaps >= s.n_gaps || (uint32_t)k.pam_mm >= s.n_pam) return -1;
  return (int)((((minus & 1u) * s.n_mm + (uint32_t)k.guide_mm) * s.n_gaps + (uint32_t)k.guide_gaps) * s.n_pam + (uint32_t)k.pam_mm);
}

__device__ __forceinline__ void counts_begin(uint32_t* hist, const CountsOut& o) {
  if (o.cells <= COUNTS_LDS_CELLS) for (uint32_t i = threadIdx.x; i < o.cells; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
}

__device__ __forceinline__ void counts_add(uint32_t* hist, const CountsOut& o, int cell) {
  if (o.cells <= COUNTS_LDS_CELLS) (void)__hip_atomic_fetch_add(hist + cell, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else (void)__hip_atomic_fetch_add(o.table + cell, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The workgroup's histogram into the call's table; true in every thread of the workgroup that finished last, which then sees every
// workgroup's adds (and whatever else they wrote with device-scope atomics).
__device__ __forceinline__ bool counts_flush(uint32_t* hist, const CountsOut& o) {
  __shared__ uint32_t s_ticket;
  __syncthreads();
  if (o.cells <= COUNTS_LDS_CELLS)
    for (uint32_t i = threadIdx.x; i < o.cells; i += blockDim.x) {
      const uint32_t v = hist[i];
      if (v) (void)__hip_atomic_fetch_add(o.table + i, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's adds have been performed ...
  __syncthreads();                                        // ... and every wave's of the workgroup
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_ticket = __hip_atomic_fetch_add(o.tickets, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_ticket != gridDim.x - 1) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return true;
}

// The last workgroup: the table to the host, table and ticket cleared.  The caller posts the mailbox behind this (thread 0).
__device__ __forceinline__ void counts_publish(const CountsOut& o) {
  for (uint32_t i = threadIdx.x; i < o.cells; i += blockDim.x) {
    o.host[i] = __hip_atomic_load(o.table + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(o.table + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) __hip_atomic_store(o.tickets, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence_system();                                 // every thread's words are on the host before thread 0 posts
  __syncthreads();
}

// ---- the specificity score (calitas_search_scores) --------------------------------------------------------------------------------
// Score mode is counts mode plus, per kept hit and in the same lane, the product of the model's factors (calitas_hip.h has the
// contract): scores_kernel and bin_scores_kernel are the counts kernels' bodies with SCORE set.  Each workgroup copies the model to LDS
// once; a lane keeps a 64-bit sum, a count of perfect hits and a maximum; score_reduce brings them wave -> LDS -> one set of
// non-returning device atomics per workgroup into the SCORE_WORDS words behind the table's cells, ahead of counts_flush, whose ticket
// then covers them; the workgroup that finishes last publishes them with the table (score_publish, counts_publish).
struct ScoreArgs {
  const uint32_t* model;       // device memory, SCORE_MODEL_WORDS words (null in a counts kernel)
  unsigned long long letters_lo, letters_hi;   // ScoreCall::letters
};
struct ScoreAcc { unsigned long long sum = 0, max = 0; uint32_t perfect = 0, hits = 0; };
struct ScoreLds { uint32_t model[SCORE_MODEL_WORDS]; unsigned long long sum, max, perfect, hits; };

__device__ __forceinline__ void score_begin(ScoreLds& s, const ScoreArgs& sa) {     // (counts_begin's barrier follows)
  for (uint32_t i = threadIdx.x; i < SCORE_MODEL_WORDS; i += blockDim.x) s.model[i] = sa.model[i];
  if (threadIdx.x == 0) { s.sum = 0; s.max = 0; s.perfect = 0; s.hits = 0; }
}

__device__ __forceinline__ uint32_t score_letter(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

// One kept hit.  The columns are walked in the order the row shows them -- ascending command-line position: aligner order for a 3' PAM,
// traceback order (= aligner order reversed, what the row of a 5' PAM guide is) for a 5' PAM, where the PAM and the gap to it come first
// among the target's bases.  An 'X' column at position i: the target letter is the one base_upper_dev gives for the forward strand,
// complemented on the minus strand (as the row builder does) -- the packed code and the exception bit are loaded together, the runs are
// looked at for an exception base only --, the guide letter is position i of the command line.  Returns the score (top mode keeps it).
constexpr unsigned long long SCORE_PERFECT = ~0ull;   // what score_hit returns for a perfect hit (a score is at most 2^32)
__device__ __forceinline__ unsigned long long score_hit(const ScoreLds& s, const ScoreArgs& sa, const HitsRef& ref, const RawAln* rp, const HitRec& h,
                                                        const GuideDev* gp, ScoreAcc& acc) {
  const int ng = rp->n_ops, pam = rp->pam;
  const OpsWords ow = load_ops_words(rp->ops);
  const OpCounts oc = count_ops(ow, ng);
  const HitKey k = hit_key(oc, pam, rp->offset, rp->pam_x);
  const int gap = pam >= 0 ? rp->offset : 0;
  acc.hits++;
  if (oc.non_eq + gap + k.pam_mm == 0) { acc.perfect++; return SCORE_PERFECT; }   // total_mm_plus_gaps == 0 (GA:101): counted, not scored
  const bool minus = h.minus != 0, pam5 = gp->pam5 != 0;
  const ContigInfo ci = ref.contigs[h.contig];
  unsigned long long v = 1ull << 32;
  int i = 0, tj = pam5 ? gap + (pam >= 0 ? (int)gp->pam_len[pam] : 0) : 0;
  for (int c = 0; c < ng; c++) {
    const int op = ow.op(pam5 ? c : ng - 1 - c);
    if (op == 1) {
      const int64_t p = minus ? (int64_t)h.end - 1 - tj : (int64_t)h.start + tj;
      uint32_t t = 4u;                                                 // beyond the contig: 'N' (RH:262-264)
      if (p >= 0 && p < (int64_t)ci.len) {
        const uint64_t g = ci.gbase + (uint64_t)p;
        const uint32_t cw = ref.codes[g >> 4], mw = ref.mask[g >> 5];
        const uint32_t code = (cw >> ((g & 15) * 2)) & 3u;
        t = minus ? 3u - code : code;
        if ((mw >> (g & 31)) & 1u) { const char b = base_upper_dev(ref, g); t = score_letter(minus ? comp_base(b) : b); }
      }
      const unsigned long long lw = i < 16 ? sa.letters_lo : sa.letters_hi;
      const uint32_t gl = (uint32_t)(lw >> ((i & 15) * 4)) & 7u;
      v = (v * s.model[(uint32_t)(i & (MAX_L - 1)) * 25u + min(gl, 4u) * 5u + t]) >> 16;
    }
    i += op != 3; tj += op != 2;
  }
  for (int r = 0; r < k.guide_gaps; r++) v = (v * s.model[MAX_L * 25]) >> 16;
  for (int r = 0; r < k.pam_mm; r++) v = (v * s.model[MAX_L * 25 + 1]) >> 16;
  acc.sum += v; acc.max = max(acc.max, v);
  return v;
}

// The lanes' sums into the workgroup's, the workgroup's into the words behind the table's cells.  Every thread of the workgroup calls it.
__device__ __forceinline__ void score_reduce(ScoreLds& s, const CountsOut& o, ScoreAcc acc) {
  unsigned long long pk = ((unsigned long long)acc.perfect << 32) | acc.hits;      // (a lane sees fewer than 2^32 hits)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc.sum += __shfl_xor(acc.sum, off); pk += __shfl_xor(pk, off);
    acc.max = max(acc.max, (unsigned long long)__shfl_xor(acc.max, off));
  }
  if ((threadIdx.x & 63u) == 0 && (uint32_t)pk != 0u) {                             // (a wave sees fewer than 2^32 hits, too)
    (void)__hip_atomic_fetch_add(&s.sum, acc.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(&s.perfect, pk >> 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(&s.hits, pk & 0xFFFFFFFFull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_max(&s.max, acc.max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s.hits) {
    unsigned long long* w = o.table + o.cells;
    (void)__hip_atomic_fetch_add(w + 0, s.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(w + 1, s.perfect, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(w + 2, s.max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(w + 3, s.hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The last workgroup, ahead of counts_publish (whose fence and barrier then cover these stores): the words to the host, and cleared.
__device__ __forceinline__ void score_publish(const CountsOut& o) {
  if (threadIdx.x < SCORE_WORDS) {
    o.host[o.cells + threadIdx.x] = __hip_atomic_load(o.table + o.cells + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(o.table + o.cells + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- the top list (calitas_search_top) --------------------------------------------------------------------------------------------
// Top mode is score mode plus an exact selection of the k best imperfect hits: top_kernel and bin_top_kernel are the
// counts kernels' bodies in a third mode.  A hit is one comparable word, key = score << 31 | (0x7FFFFFFF - rank), where rank is the
// hit's place in the text order of the call (below TOP_RANK_MAX, so no key is 0 and no two are equal; larger is better): the k largest
// keys ARE the list, whatever order they are met in.  A workgroup keeps TOP_CAP keys and a threshold in LDS; a lane appends a key above
// the threshold through an LDS counter; before a trip that could overflow the buffer the workgroup sorts it (bitonic), keeps the best
// k and raises the threshold to the k-th.  At its end a workgroup stores its at most k keys and their number into its slot of the
// work's lists, ahead of counts_flush, whose ticket then covers them; the workgroup that finishes last runs all slots through the same
// buffer and writes the winners' records behind the score words in the work's page-locked block.  Every workgroup stores its number
// in every call and the last one reads the slots of this grid only, so the slots need no clearing between calls.
constexpr uint32_t TOP_CAP = 2 * CALITAS_TOP_MAX;
constexpr uint32_t TOP_LISTS = 128;                      // the most workgroups counts_grid gives
constexpr uint32_t TOP_RANK_MAX = 0x7FFFFFFEu;           // ranks are 0 .. TOP_RANK_MAX: a call with more declines
static_assert(TOP_CAP == 2 * COUNTS_BLOCK && CALITAS_TOP_MAX <= COUNTS_BLOCK, "a thread per pair of the sort; a trip appends at most COUNTS_BLOCK keys");

// The four modes of the counts kernels' bodies (counts_body in hits.hip, bin_counts_body in binned.hip).
constexpr int MODE_COUNTS = 0, MODE_SCORES = 1, MODE_TOP = 2, MODE_REGIONS = 3;

struct TopArgs {
  uint32_t k;
  unsigned long long* lists;   // device memory, TOP_LISTS x CALITAS_TOP_MAX keys
  uint32_t* list_n;            // TOP_LISTS numbers of keys
};
struct TopLds { unsigned long long key[TOP_CAP]; unsigned long long thr, floor; uint32_t n, most; uint32_t list_n[TOP_LISTS]; };   // most: bin_top_kernel, the most rows of a bin of a trip

__device__ __forceinline__ unsigned long long top_key(unsigned long long score, uint32_t rank) { return (score << 31) | (0x7FFFFFFFu - rank); }

__device__ __forceinline__ void top_begin(TopLds& t) {            // (counts_begin's barrier follows)
  if (threadIdx.x == 0) { t.n = 0; t.thr = 0; }
}

// The buffer sorted, best first, and cut at k: returns what is left (t.n).  Every thread of the workgroup calls it, behind a barrier
// that follows the last append.
__device__ __forceinline__ uint32_t top_compact(TopLds& t, uint32_t k) {
  const uint32_t n = t.n, tid = threadIdx.x;
  for (uint32_t i = tid; i < TOP_CAP; i += COUNTS_BLOCK) if (i >= n) t.key[i] = 0;
  __syncthreads();
  for (uint32_t size = 2; size <= TOP_CAP; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      const uint32_t lo = ((tid & ~(stride - 1)) << 1) | (tid & (stride - 1)), hi = lo | stride;
      const unsigned long long x = t.key[lo], y = t.key[hi];
      if ((lo & size) == 0 ? x < y : x > y) { t.key[lo] = y; t.key[hi] = x; }
      __syncthreads();
    }
  const uint32_t m = min(n, k);
  if (tid == 0) { t.n = m; if (n > k) t.thr = t.key[k - 1]; }
  __syncthreads();
  return m;
}

// One trip of every thread of the workgroup (key 0: this lane has none): room for a trip's appends is made first -- the decision is
// taken on a value read between two barriers, so it is the same in every thread --, then the keys above the threshold are appended.
__device__ __forceinline__ void top_offer(TopLds& t, uint32_t k, unsigned long long key) {
  __syncthreads();                                        // the appends of the trip before are in
  const uint32_t n = t.n;
  __syncthreads();                                        // ... and everybody has read their number
  if (n > TOP_CAP - COUNTS_BLOCK) (void)top_compact(t, k);
  if (key > t.thr) t.key[__hip_atomic_fetch_add(&t.n, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)] = key;
}

// The end of a workgroup's hits: its best k keys into its slot.  Every thread calls it.
__device__ __forceinline__ void top_store(TopLds& t, const TopArgs& ta) {
  __syncthreads();
  const uint32_t m = top_compact(t, ta.k);
  if (threadIdx.x < m) __hip_atomic_store(ta.lists + (size_t)blockIdx.x * CALITAS_TOP_MAX + threadIdx.x, t.key[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0) __hip_atomic_store(ta.list_n + blockIdx.x, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The last workgroup (counts_flush said so): the slots of the grid's workgroups through the buffer, COUNTS_BLOCK / k slots to a trip;
// returns the number of winners, which are t.key[0 .. ), best first.  Every thread calls it.
__device__ __forceinline__ uint32_t top_fold(TopLds& t, const TopArgs& ta) {
  const uint32_t tid = threadIdx.x, lists = min(gridDim.x, TOP_LISTS);
  __syncthreads();                                        // (top_store's readers of key[] are done)
  if (tid == 0) { t.n = 0; t.thr = 0; t.floor = ~0ull; }
  if (tid < lists) t.list_n[tid] = min(__hip_atomic_load(ta.list_n + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), ta.k);
  __syncthreads();
  // A floor under the k-th key before any slot is read whole: with c = ceil(k / slots), the c-th key of every slot -- where every slot
  // has one -- makes slots * c >= k keys at or above the smallest of them, so nothing below that can be among the k best: the fold of
  // 128 slots of 256 keys then appends a few hundred keys instead of compacting on most of its 128 trips.
  const uint32_t c = (ta.k + lists - 1) / lists;
  if (tid < lists) {
    const unsigned long long f = t.list_n[tid] >= c ? __hip_atomic_load(ta.lists + (size_t)tid * CALITAS_TOP_MAX + (c - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    (void)__hip_atomic_fetch_min(&t.floor, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (tid == 0 && t.floor != 0) t.thr = t.floor - 1;      // (a key equal to the floor passes top_offer's `>`)
  const uint32_t per = COUNTS_BLOCK / ta.k, sub = tid / ta.k, e = tid - sub * ta.k;
  auto load = [&](uint32_t l0) -> unsigned long long {
    const uint32_t l = l0 + sub;
    if (sub >= per || l >= lists || e >= t.list_n[l]) return 0ull;
    return __hip_atomic_load(ta.lists + (size_t)l * CALITAS_TOP_MAX + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  unsigned long long key = load(0);
  for (uint32_t l0 = 0; l0 < lists; l0 += per) {
    const unsigned long long next = l0 + per < lists ? load(l0 + per) : 0ull;   // (in flight across this trip's barriers)
    top_offer(t, ta.k, key);
    key = next;
  }
  __syncthreads();
  return top_compact(t, ta.k);
}

// A winner's record into the work's page-locked block, behind the score words: three words in the layout of calitas_top_hit_t.
__device__ __forceinline__ void top_record(const CountsOut& o, uint32_t i, unsigned long long key, const RawAln* rp, const HitRec& h) {
  const HitKey hk = hit_key(count_ops(load_ops_words(rp->ops), rp->n_ops), rp->pam, rp->offset, rp->pam_x);
  unsigned long long* w = o.host + o.cells + SCORE_WORDS + 1 + 3 * (size_t)i;
  w[0] = key >> 31;
  w[1] = (unsigned long long)(uint32_t)h.contig | ((unsigned long long)(uint32_t)h.gstart << 32);
  w[2] = (unsigned long long)(uint32_t)h.gend | ((unsigned long long)(h.minus ? '-' : '+') << 32) | ((unsigned long long)(hk.guide_mm & 255) << 40) |
         ((unsigned long long)(hk.guide_gaps & 255) << 48) | ((unsigned long long)(hk.pam_mm & 255) << 56);
}
__device__ __forceinline__ uint32_t top_rank(unsigned long long key) { return 0x7FFFFFFFu - (uint32_t)(key & 0x7FFFFFFFull); }

// ---- the regions (calitas_search_regions) ------------------------------------------------------------------------------------------
// Regions mode is top mode with a class per kept hit (regions.hpp: region_class on the record's coordinate_start / coordinate_end):
// regions_kernel and bin_regions_kernel are the counts kernels' bodies in a fourth mode.  The table gets a leading class dimension --
// CountsOut::cells is n_classes x the shape's cells, so counts_begin / counts_add / counts_flush / counts_publish do for it what they
// do for any table: in LDS up to COUNTS_LDS_CELLS, by direct adds beyond.  The totals take the path they take in score mode (a lane's
// registers, score_reduce); per class, every hit adds to REGION_WORDS 64-bit words in LDS -- no array indexed by the class in a
// lane's registers --, which region_reduce flushes behind the SCORE_WORDS of the device table ahead of counts_flush and the last
// workgroup publishes and clears (region_publish).  A hit offers its key to the selection only when its class is in list_mask; k = 0
// (uniform) skips the selection.  The last workgroup writes a class byte per record behind the classes' words.
struct RegionArgs {
  RegionsView rv;
  uint32_t base_cells;         // the shape's cells: a hit's cell is cls * base_cells + counts_cell
  uint32_t list_mask;
};
struct RegionLds { unsigned long long w[CALITAS_REGION_CLASSES_MAX * REGION_WORDS]; };

__device__ __forceinline__ void region_begin(RegionLds& r) {      // (counts_begin's barrier follows)
  if (threadIdx.x < CALITAS_REGION_CLASSES_MAX * REGION_WORDS) r.w[threadIdx.x] = 0;
}
__device__ __forceinline__ uint32_t region_of_hit(const RegionArgs& ra, const HitsRef& ref, const HitRec& h) {
  return min(region_class(ra.rv, (uint32_t)h.contig, h.gstart, h.gend, ref.contigs[h.contig].len), ra.rv.n_classes - 1u);
}
// One kept hit of class cls with score s (SCORE_PERFECT: a perfect one).
__device__ __forceinline__ void region_hit(RegionLds& r, uint32_t cls, unsigned long long s) {
  unsigned long long* w = r.w + cls * REGION_WORDS;
  (void)__hip_atomic_fetch_add(w + 3, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (s == SCORE_PERFECT) (void)__hip_atomic_fetch_add(w + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else {
    (void)__hip_atomic_fetch_add(w + 0, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_max(w + 2, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}
// The workgroup's words into the device table's, behind the totals' SCORE_WORDS.  Every thread calls it, ahead of counts_flush.
__device__ __forceinline__ void region_reduce(RegionLds& r, const CountsOut& o, uint32_t n_classes) {
  __syncthreads();
  if (threadIdx.x < n_classes * REGION_WORDS) {
    const unsigned long long v = r.w[threadIdx.x];
    unsigned long long* w = o.table + o.cells + SCORE_WORDS + threadIdx.x;
    if (v) {
      if ((threadIdx.x & 3u) == 2u) (void)__hip_atomic_fetch_max(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else (void)__hip_atomic_fetch_add(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
// The last workgroup, ahead of counts_publish: the classes' words to the host (behind the top list's words), and cleared.
__device__ __forceinline__ void region_publish(const CountsOut& o, uint32_t n_classes) {
  if (threadIdx.x < CALITAS_REGION_CLASSES_MAX * REGION_WORDS) {
    unsigned long long v = 0;
    if (threadIdx.x < n_classes * REGION_WORDS) {
      v = __hip_atomic_load(o.table + o.cells + SCORE_WORDS + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(o.table + o.cells + SCORE_WORDS + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    o.host[o.cells + SCORE_WORDS + TOP_WORDS + threadIdx.x] = v;
  }
}
__device__ __forceinline__ void region_record(const CountsOut& o, uint32_t i, uint32_t cls) {
  reinterpret_cast<uint8_t*>(o.host + o.cells + SCORE_WORDS + TOP_WORDS + REGION_CLASS_WORDS)[i] = (uint8_t)cls;
}

// Workgroups of a counts kernel over `items` items (each strides over them).
static inline unsigned counts_grid(size_t items) { return (unsigned)std::min<size_t>(std::max<size_t>((items + COUNTS_BLOCK - 1) / COUNTS_BLOCK, 1), 128); }

struct HitsWork {
  HitRec* hits = nullptr; size_t hits_cap = 0;
  uint64_t *keys = nullptr, *keys2 = nullptr, *lens = nullptr, *offs = nullptr;
  size_t keys_cap = 0, keys2_cap = 0, lens_cap = 0, offs_cap = 0;
  uint32_t *vals = nullptr, *vals2 = nullptr, *s_cs = nullptr, *wks = nullptr; size_t vals_cap = 0, vals2_cap = 0, cs_cap = 0, wks_cap = 0;
  int32_t *s_start = nullptr, *s_end = nullptr, *s_score = nullptr; size_t ss_cap = 0, se_cap = 0, sc_cap = 0;
  uint8_t *keep = nullptr, *head = nullptr; size_t keep_cap = 0, head_cap = 0;
  void* temp = nullptr; size_t temp_cap = 0;
  char* text = nullptr; size_t text_cap = 0;
  uint32_t* midlen = nullptr; size_t midlen_cap = 0;
  char* blob = nullptr; size_t blob_cap = 0;
  char* names = nullptr; size_t names_cap = 0;
  uint32_t* name_off = nullptr; size_t name_off_cap = 0;
  HitsExtKey* ext_keys = nullptr; size_t ext_keys_cap = 0;   // the caller's own hits of this call (HitsExt)
  uint64_t* ext_off = nullptr; size_t ext_off_cap = 0;
  char* ext_rows = nullptr; size_t ext_rows_cap = 0;
  uint8_t* ext_keep = nullptr; size_t ext_keep_cap = 0;      // HitsExt::rows_for: the walks' verdict per entry, and its page-locked copy
  uint8_t* h_ext_keep = nullptr; size_t h_ext_keep_cap = 0;
  uint64_t* ext_place = nullptr; size_t ext_place_cap = 0;   // HitsExtRows::fill_on_host: where every kept entry's row belongs in the text
  uint64_t* h_ext_place = nullptr; size_t h_ext_place_cap = 0;
  uint64_t* d_counts = nullptr;   // [0] text bytes, [1] low word: kept rows, high word: kept hits of the caller's own, [2] low word: flags
  uint64_t* h_counts = nullptr;   // pinned
  // counts mode (CountsOut): the call's table on the device with its ticket word behind it, and the table's page-locked copy
  unsigned long long* cnt_table = nullptr; size_t cnt_cap = 0;
  unsigned long long* cnt_host = nullptr; size_t cnt_host_cap = 0;
  // score mode: this context's device copy of the model, brought up again only when its bytes change (score_model)
  uint32_t* score_dev = nullptr; std::vector<uint32_t> score_host;
  // top mode (TopArgs): the workgroups' slots and their numbers of keys
  unsigned long long* top_lists = nullptr; uint32_t* top_n = nullptr;
  Mailbox mbox;                   // carries d_counts to the host (mailbox.hpp)
  RowConstDev rc{};               // set by hits_prepare
  size_t blob_bytes = 0;
  std::string blob_host;
  bool prepared = false;
};

// The buffers of a call's table in the work (zero on the device: the kernels leave them so), with room for a score call's SCORE_WORDS
// behind the cells -- and in the page-locked copy for a top call's TOP_WORDS behind those.  n_classes != 0: a regions call, whose
// table has that many times the cells, and REGION_WORDS per class behind the SCORE_WORDS (in the page-locked copy: REGION_HOST_WORDS
// behind the TOP_WORDS).
inline hipError_t counts_buffers(HitsWork& w, const CountsShape& shape, CountsOut* out, uint32_t n_classes = 0) {
  const size_t table_cells = (size_t)shape.cells() * std::max(n_classes, 1u);
  const size_t cells = table_cells + SCORE_WORDS + (size_t)n_classes * REGION_WORDS;
  if (table_cells == 0 || table_cells > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (cells + 2 > w.cnt_cap) {
    (void)hipFree(w.cnt_table); w.cnt_table = nullptr; w.cnt_cap = 0;
    const size_t cap = ((cells + 2) + 1) & ~(size_t)1;     // (a multiple of 16 bytes)
    hipError_t e = hipMalloc((void**)&w.cnt_table, cap * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    e = hipMemset(w.cnt_table, 0, cap * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (the kernels run on streams nothing orders against the null stream)
    if (e != hipSuccess) return e;
    w.cnt_cap = cap;
  }
  if (cells > w.cnt_host_cap) {
    if (w.cnt_host) (void)hipHostFree(w.cnt_host);
    w.cnt_host = nullptr; w.cnt_host_cap = 0;
    hipError_t e = hipHostMalloc((void**)&w.cnt_host, (cells + TOP_WORDS + REGION_HOST_WORDS) * sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) return e;
    w.cnt_host_cap = cells;
  }
  out->shape = shape; out->cells = (uint32_t)table_cells; out->table = w.cnt_table; out->tickets = reinterpret_cast<uint32_t*>(w.cnt_table + w.cnt_cap - 1);
  out->host = w.cnt_host;
  return hipSuccess;
}

// The slots of a top call in the work.
inline hipError_t top_buffers(HitsWork& w, uint32_t k, TopArgs* out) {
  hipError_t e;
  if (!w.top_lists && (e = hipMalloc((void**)&w.top_lists, (size_t)TOP_LISTS * CALITAS_TOP_MAX * sizeof(unsigned long long))) != hipSuccess) return e;
  if (!w.top_n && (e = hipMalloc((void**)&w.top_n, TOP_LISTS * sizeof(uint32_t))) != hipSuccess) return e;
  out->k = k; out->lists = w.top_lists; out->list_n = w.top_n;
  return hipSuccess;
}

// The model of a score call on the device: the work's copy, uploaded on `stream` when its bytes differ from the last call's.
inline hipError_t score_model(HitsWork& w, const ScoreCall& sc, hipStream_t stream, ScoreArgs* out) {
  hipError_t e;
  if (!w.score_dev && (e = hipMalloc((void**)&w.score_dev, SCORE_MODEL_WORDS * sizeof(uint32_t))) != hipSuccess) return e;
  if (w.score_host.size() != SCORE_MODEL_WORDS || std::memcmp(w.score_host.data(), sc.model, SCORE_MODEL_WORDS * sizeof(uint32_t)) != 0) {
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;      // (a copy of the old bytes may still be reading them)
    w.score_host.assign(sc.model, sc.model + SCORE_MODEL_WORDS);
    if ((e = hipMemcpyAsync(w.score_dev, w.score_host.data(), SCORE_MODEL_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, stream)) != hipSuccess) {
      w.score_host.clear();
      return e;
    }
  }
  out->model = w.score_dev; out->letters_lo = sc.letters[0]; out->letters_hi = sc.letters[1];
  return hipSuccess;
}

}  // namespace calitas
