// edit_sites.hip -- the base-editor guides of a single-nucleotide variant and their bystanders (calitas_find_edit_sites, gfx950).
// No reference counterpart.
//
// One lane per SNV.  A protospacer of at most 32 bases that holds the SNV starts at one of the 32 positions p = position - 31 + j,
// j = 0 .. 31, whatever the strand and the window, and everything about start j is bit j of a 32-bit vector.  A footprint is
// [p + lo, p + hi) with -16 <= lo <= 0 < hi <= 48, so the text those starts read is the 95 bases from position - 47: base t of the
// window is position - 47 + t, what start j shows at offset d of its pattern is base j + 16 + d, and the SNV is base 47.
//   * The lane holds the SNV against the contig's bounds BEFORE it loads anything, then loads the four consecutive 32-base words of
//     both planes and of the exception mask that cover the window, each held against the packed space's end (a word beyond it reads
//     as exception bases), and funnels (v_alignbit_b32) them into three words per plane: one round of loads, the same for every
//     lane.  The reference's base is bit 47; with the editor's change it decides the strand, and from there on the strand is DATA, a
//     select, never a branch.  Only the background allele is matched: the SNV's two plane bits are replaced by the background base
//     (the reference's when installing, alt when correcting).  The starts that hold the SNV inside the editor's window on the
//     lane's strand are a contiguous range of j.
//   * edit_walk matches the 32 starts bit-parallel, as sites_kernel does: per pattern offset at which either strand's pattern has a
//     letter that is not N (a uniform test: the patterns sit in LDS and PAM and offset are loop counters) one funnel shift per plane
//     at a scalar offset and a selection among the four base masks by the lane's strand's set.  A start whose footprint holds an
//     exception base or leaves the contig is cleared by a run test (log2 steps) on the bases that are plain and inside.  The first
//     PAM that matches wins.
//   * The editable bases are ONE vector for the whole window: plain & is(from) & (any context | the 5' neighbour is plain and in the
//     set), `from` and the set complemented and the neighbour taken at +1 instead of -1 on '-'.  The SNV's own bit decides status 5.
//     A start's `editable` word is a funnel shift of that vector, cut to the protospacer, bit-reversed into guide order on '-' (as
//     copies_key does with the planes), masked by the window; its bystanders are a popcount.
//   * edit_count_kernel stores the lane's count and status, the workgroup's sum and adds the workgroup's four bystander bins (wave
//     reductions, the waves' sums added in LDS) to the call's counters: at most four non-returning atomics.
//   * edit_write_kernel, after launch_sites_offsets over the workgroups' sums: the exclusive prefix of the workgroup's lane counts
//     (a wave scan, the earlier waves' sums from LDS), the same walk again, every record as two 16-byte stores at its place.
// Both kernels run the one edit_walk, so count and write cannot disagree.  No sort, no returning atomic.
#include "kernels.hpp"

#include <hip/hip_runtime.h>

namespace calitas {

namespace {

constexpr int EDIT_WAVES = EDIT_THREADS / 64;
constexpr uint32_t EDIT_PAT_WORDS = sizeof(SitePatterns) / 4;
static_assert(sizeof(SitePatterns) % 4 == 0 && EDIT_PAT_WORDS <= EDIT_THREADS, "a word of the patterns per lane");
static_assert(SITE_MAX_FOOT <= 64 && MAX_L <= 32 && MAX_PAM_LEN <= 16, "the window is 96 bases and a step of the run test is below 32");

struct W96 { uint32_t a, b, c; };   // bits 0 .. 31, 32 .. 63, 64 .. 95

CAL_DEV uint32_t ones32(int n) { return n <= 0 ? 0u : n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }   // bits [0, n)
CAL_DEV W96 ones96(int n) { return W96{ones32(n), ones32(n - 32), ones32(n - 64)}; }
// bits [o, o + 32) of x (zeros beyond bit 95), o = 0 .. 63 the same in every lane
CAL_DEV uint32_t take32(const W96& x, uint32_t o) { return o < 32u ? __builtin_amdgcn_alignbit(x.b, x.a, o) : __builtin_amdgcn_alignbit(x.c, x.b, o - 32u); }
// the same at a lane's own o = 0 .. 63: the words by a select (of values: x is passed by value, so that no select of addresses
// turns the window into an indexed array)
CAL_DEV uint32_t take32_lane(W96 x, uint32_t o) {
  const bool up = o >= 32u;
  return __builtin_amdgcn_alignbit(up ? x.c : x.b, up ? x.b : x.a, o & 31u);
}
CAL_DEV W96 shr96(const W96& x, uint32_t s) {   // s = 1 .. 31
  return W96{__builtin_amdgcn_alignbit(x.b, x.a, s), __builtin_amdgcn_alignbit(x.c, x.b, s), x.c >> s};
}
CAL_DEV W96 and96(const W96& x, const W96& y) { return W96{x.a & y.a, x.b & y.b, x.c & y.c}; }
// the window of 96 bases from bit sh of four consecutive words
CAL_DEV W96 align96(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t sh) {
  return W96{__builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh), __builtin_amdgcn_alignbit(w3, w2, sh)};
}
// the bases of a word that are in `set` (bit c = code c), a lane's own
CAL_DEV uint32_t in_set(uint32_t lo, uint32_t hi, uint32_t set) {
  const uint32_t sa = 0u - (set & 1u), sc = 0u - ((set >> 1) & 1u), sg = 0u - ((set >> 2) & 1u), st = 0u - ((set >> 3) & 1u);
  return (sa & ~lo & ~hi) | (sc & lo & ~hi) | (sg & ~lo & hi) | (st & lo & hi);
}
CAL_DEV W96 in_set96(const W96& lo, const W96& hi, uint32_t set) { return W96{in_set(lo.a, hi.a, set), in_set(lo.b, hi.b, set), in_set(lo.c, hi.c, set)}; }

constexpr int EDIT_SNV_AT = 47;    // the SNV's place in the window: protospacer start position - 31 + j shows offset d of its pattern at j + 16 + d

struct EditWindow {
  W96 lo, hi;                      // the planes of the 95 bases from position - 47 on the background allele
  W96 editable;                    // base t can be edited on the lane's strand
  uint32_t minus;
};

// The records of SNV v in output order: emit(k, j, the PAM, the editable word, the bystanders, the window) for the k-th of them, start
// j of the window; returns their number and leaves the SNV's status in *status.
// UNROLL: how far the loop over a word's eight offsets is unrolled.  Measured on 10^7 targets: the count kernel is
// fastest with the loop flat (8: the funnel shifts of a word issue together), the write kernel, most of whose lanes have left before
// the walk, with the loop rolled (1: 60 VGPRs instead of 93).
template <int UNROLL, class Emit>
CAL_DEV uint32_t edit_walk(const EditArgs& a, const SitePatterns& pat, const Snv& v, uint32_t* status, Emit emit) {
  *status = 0;
  if (v.reserved == ALLELE_HOST_DECIDES) return 0;
  if (v.contig < 0 || v.contig >= a.n_contigs || v.position < 0) { *status = 2; return 0; }   // (cannot happen: the host has checked)
  const ContigInfo ci = a.contigs[v.contig];
  if ((uint64_t)v.position >= ci.len) { *status = 2; return 0; }                              // (nor this)
  const EditRule& e = a.rule;
  const int64_t pos = v.position;
  const int L = pat.proto_len;

  EditWindow win;
  const int64_t origin = pos - (EDIT_SNV_AT);                        // base 0 of the window, in the contig's coordinates
  const int64_t first = (int64_t)ci.gbase + origin;
  const int64_t wf = first >> 5;
  const uint32_t sh = (uint32_t)(first & 31);
  uint32_t l[4], h[4], x[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int64_t w = wf + i;
    const bool in = w >= 0 && (uint64_t)w < a.n_words;
    const uint2 p = in ? a.planes[w] : make_uint2(0u, 0u);
    l[i] = p.x; h[i] = p.y; x[i] = in ? a.mask[w] : 0xFFFFFFFFu;
  }
  win.lo = align96(l[0], l[1], l[2], l[3], sh);
  win.hi = align96(h[0], h[1], h[2], h[3], sh);
  W96 plain = align96(~x[0], ~x[1], ~x[2], ~x[3], sh);               // base t is a plain one inside the contig
  {
    const int from = origin < 0 ? (int)-origin : 0;                  // base 0 of the contig
    const int64_t left = (int64_t)ci.len - origin;                   // >= 48
    const int to = left >= 96 ? 96 : (int)left;                      // the contig's end
    const W96 upto = ones96(to), below = ones96(from);
    plain = W96{plain.a & upto.a & ~below.a, plain.b & upto.b & ~below.b, plain.c & upto.c & ~below.c};
  }

  // the reference's base, the statuses that need nothing else, and the strand
  constexpr uint32_t snv_bit = 1u << (EDIT_SNV_AT - 32);             // of the windows' second words
  if (!(plain.b & snv_bit)) { *status = 2; return 0; }
  const uint32_t ref_code = ((win.lo.b & snv_bit) ? 1u : 0u) | ((win.hi.b & snv_bit) ? 2u : 0u);
  if (v.ref != 0 && allele_code(v.ref) != ref_code) { *status = 1; return 0; }
  const uint32_t alt_code = allele_code(v.alt);
  if (alt_code == ref_code) { *status = 3; return 0; }
  const uint32_t background = e.correct ? alt_code : ref_code, product = e.correct ? ref_code : alt_code;
  const int strand = edit_strand(e, background, product);
  if (strand < 0) { *status = 4; return 0; }
  const uint32_t minus = (uint32_t)strand;
  win.minus = minus;
  win.lo.b = (win.lo.b & ~snv_bit) | ((background & 1u) ? snv_bit : 0u);   // the background allele's base at the SNV
  win.hi.b = (win.hi.b & ~snv_bit) | ((background & 2u) ? snv_bit : 0u);

  // the editable bases of the whole window, in forward terms: `from` and the context's set complemented on '-', the 5' neighbour the
  // base at t - 1 on '+' and at t + 1 on '-'
  {
    const uint32_t from_code = minus ? 3u - e.from : e.from;
    const uint32_t f_lo = (from_code & 1u) ? 0u : 0xFFFFFFFFu, f_hi = (from_code & 2u) ? 0u : 0xFFFFFFFFu;   // base == code: both planes agree
    win.editable = W96{plain.a & (win.lo.a ^ f_lo) & (win.hi.a ^ f_hi), plain.b & (win.lo.b ^ f_lo) & (win.hi.b ^ f_hi),
                       plain.c & (win.lo.c ^ f_lo) & (win.hi.c ^ f_hi)};
    if (e.context != 15u) {                                          // (uniform)
      const W96 nb = and96(plain, in_set96(win.lo, win.hi, minus ? edit_complement_set(e.context) : e.context));   // a neighbour that satisfies the context
      const W96 before = W96{nb.a << 1, (nb.b << 1) | (nb.a >> 31), (nb.c << 1) | (nb.b >> 31)};
      const W96 after = W96{(nb.a >> 1) | (nb.b << 31), (nb.b >> 1) | (nb.c << 31), nb.c >> 1};
      win.editable = and96(win.editable, W96{minus ? after.a : before.a, minus ? after.b : before.b, minus ? after.c : before.c});
    }
  }
  if (!(win.editable.b & snv_bit)) { *status = 5; return 0; }        // (plain and `from` it is: the 5' neighbour fails the context)

  // the starts with a site, the winning PAM's index bit by bit
  uint32_t has = 0, k0 = 0, k1 = 0, k2 = 0;
#pragma unroll 1
  for (int k = 0; k < pat.n_pams; k++) {
    // run.bit t: the n = L + pam_len bases from t on are plain and inside (both strands' footprints have this length)
    const int n = L + pat.p[k][0].pam_len;
    W96 run = plain;
    for (int len = 1; len < n;) {
      const int step = len < n - len ? len : n - len;
      run = and96(run, shr96(run, (uint32_t)step));
      len += step;
    }
    const SitePattern& plus = pat.p[k][0];
    const SitePattern& rev = pat.p[k][1];
    const uint32_t run_plus = take32(run, (uint32_t)(16 + plus.lo)), run_rev = take32(run, (uint32_t)(16 + rev.lo));
    uint32_t m = minus ? run_rev : run_plus;
    // eight offsets a word of the sets: a word in which neither strand has a letter is skipped as one (N20 + nrg: two words of eight)
#pragma unroll 1
    for (int w = 0; w < 8; w++) {
      const uint32_t both = plus.sets[w] & rev.sets[w];
      if (both == 0xFFFFFFFFu) continue;                             // (uniform: a scalar branch, as the one below)
      const uint32_t sets_plus = plus.sets[w], sets_rev = rev.sets[w];
#pragma unroll UNROLL
      for (int i = 0; i < 8; i++) {
        if (((both >> (4 * i)) & 15u) == 15u) continue;
        const uint32_t o = (uint32_t)(8 * w + i);
        m &= in_set(take32(win.lo, o), take32(win.hi, o), ((minus ? sets_rev : sets_plus) >> (4 * i)) & 15u);
      }
    }
    const uint32_t fresh = m & ~has;
    has |= fresh;
    if (k & 1) k0 |= fresh;
    if (k & 2) k1 |= fresh;
    if (k & 4) k2 |= fresh;
  }
  {   // the starts that hold the SNV in the window: p = position - o on '+', position - (L - 1) + o on '-', o = window_from .. window_to - 1
    const int j_from = minus ? 32 - L + (int)e.window_from : 32 - (int)e.window_to, j_to = minus ? 32 - L + (int)e.window_to : 32 - (int)e.window_from;
    has &= ones32(j_to) & ~ones32(j_from);
  }

  const uint32_t in_window = ones32((int)e.window_to) & ~ones32((int)e.window_from);
  uint32_t count = 0;
  for (uint32_t rest = has; rest; rest &= rest - 1u) {
    const int j = __builtin_ctz(rest);
    uint32_t ed = take32_lane(win.editable, (uint32_t)(16 + j)) & ones32(L);
    if (minus) ed = __builtin_bitreverse32(ed) >> (32 - L);
    ed &= in_window;
    const uint32_t bystanders = (uint32_t)__builtin_popcount(ed) - 1u;   // (the SNV's own bit is set: status 5 otherwise)
    if (e.max_bystanders != EDIT_NO_BOUND && bystanders > e.max_bystanders) continue;
    emit(count, j, (int)(((k0 >> j) & 1u) | (((k1 >> j) & 1u) << 1) | (((k2 >> j) & 1u) << 2)), ed, bystanders, win);
    count++;
  }
  return count;
}

CAL_DEV uint32_t edit_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

CAL_DEV void edit_stage_patterns(SitePatterns& s_pat, const SitePatterns* pat, uint32_t tid) {
  if (tid < EDIT_PAT_WORDS) reinterpret_cast<uint32_t*>(&s_pat)[tid] = reinterpret_cast<const uint32_t*>(pat)[tid];
  __syncthreads();
}

__global__ __launch_bounds__(EDIT_THREADS) void edit_count_kernel(EditArgs a) {
  __shared__ SitePatterns s_pat;
  __shared__ uint32_t s_by[EDIT_WAVES][4];
  const uint32_t tid = threadIdx.x;
  edit_stage_patterns(s_pat, a.pat, tid);
  const uint64_t r = (uint64_t)blockIdx.x * EDIT_THREADS + tid;
  uint32_t by0 = 0, by1 = 0, by2 = 0, by3 = 0;
  if (r < a.n) {
    uint32_t status = 0;
    a.lane_count[r] = edit_walk<8>(a, s_pat, a.snvs[r], &status, [&](uint32_t, int, int, uint32_t, uint32_t bystanders, const EditWindow&) {
      by0 += bystanders == 0u ? 1u : 0u; by1 += bystanders == 1u ? 1u : 0u; by2 += bystanders == 2u ? 1u : 0u; by3 += bystanders >= 3u ? 1u : 0u;
    });
    a.status[r] = (uint8_t)status;
  }
  by0 = edit_wave_sum(by0); by1 = edit_wave_sum(by1); by2 = edit_wave_sum(by2); by3 = edit_wave_sum(by3);
  if ((tid & 63u) == 0) { uint32_t* s = s_by[tid >> 6]; s[0] = by0; s[1] = by1; s[2] = by2; s[3] = by3; }
  __syncthreads();
  if (tid < 4) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < EDIT_WAVES; k++) sum += s_by[k][tid];
    if (sum) (void)atomicAdd(&a.per_bystanders[tid], (unsigned long long)sum);
  }
  if (tid == 0) {
    uint32_t sum = 0;                                                // (at most 256 x 32: no overflow)
#pragma unroll
    for (int k = 0; k < EDIT_WAVES; k++) sum += s_by[k][0] + s_by[k][1] + s_by[k][2] + s_by[k][3];
    a.wg_count[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(EDIT_THREADS) void edit_write_kernel(EditArgs a) {
  __shared__ SitePatterns s_pat;
  __shared__ uint32_t s_wave[EDIT_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  edit_stage_patterns(s_pat, a.pat, tid);
  const uint64_t r = (uint64_t)blockIdx.x * EDIT_THREADS + tid;
  const uint32_t mine = r < a.n ? a.lane_count[r] : 0u;
  uint32_t upto = mine;                                              // the counts of the wave's lanes up to and with this one
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)upto, d);
    if (lane >= (uint32_t)d) upto += t;
  }
  if (lane == 63u) s_wave[tid >> 6] = upto;
  __syncthreads();
  if (mine == 0) return;
  uint32_t before = upto - mine;
#pragma unroll
  for (uint32_t k = 0; k < EDIT_WAVES; k++) before += k < (tid >> 6) ? s_wave[k] : 0u;
  const uint64_t base = a.wg_offset[blockIdx.x] + before;
  const Snv v = a.snvs[r];
  const int L = s_pat.proto_len;
  const bool pamless = s_pat.pamless != 0;
  uint32_t status = 0;
  (void)edit_walk<1>(a, s_pat, v, &status, [&](uint32_t k, int j, int pam, uint32_t editable, uint32_t, const EditWindow& win) {
    const uint64_t at = base + k;
    if (k >= mine || at >= a.out_capacity) return;                   // (cannot happen: count and offsets come from this very walk)
    const bool minus = win.minus != 0;
    const SitePattern& sp = s_pat.p[pam][win.minus];
    const int32_t p = v.position - 31 + j;
    const int32_t pam_start = pamless ? -1 : p + sp.pam_off;
    const uint32_t pam_index = pamless ? 0xFFu : (uint32_t)pam;
    const uint64_t guide = copies_key(take32_lane(win.lo, (uint32_t)(16 + j)), take32_lane(win.hi, (uint32_t)(16 + j)), L, L, minus, false);
    uint4* out = reinterpret_cast<uint4*>(a.out + at);
    out[0] = make_uint4((uint32_t)v.contig, (uint32_t)p, (uint32_t)pam_start,
                        (uint32_t)(minus ? '-' : '+') | (pam_index << 8) | ((uint32_t)sp.pam_len << 16) | ((uint32_t)L << 24));
    out[1] = make_uint4((uint32_t)r, editable, (uint32_t)guide, (uint32_t)(guide >> 32));
  });
}

}  // namespace

hipError_t launch_edit_count(const EditArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(edit_count_kernel, dim3(edit_blocks(a.n)), dim3(EDIT_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_edit_write(const EditArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(edit_write_kernel, dim3(edit_blocks(a.n)), dim3(EDIT_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace calitas
