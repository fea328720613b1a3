// allele_sites.hip -- the sites a single-nucleotide variant creates, destroys or changes (calitas_find_allele_sites, gfx950).
// No reference counterpart.
//
// One lane per SNV.  A footprint is [p + lo, p + hi) with -16 <= lo <= 0 < hi <= 48, so the protospacer starts whose footprint can
// hold the SNV are the 64 of (position - 48, position + 16]: start j of the window is p = position - 47 + j, and everything about it
// is bit j of a 64-bit vector.  The text those starts read is the 127 bases [position - 63, position + 64): base t of the window is
// position - 63 + t, the SNV is base 63, and what start j shows at offset d of its pattern is base j + 16 + d.
//   * The lane holds the SNV against the contig's bounds BEFORE it loads anything, then loads the five consecutive 32-base words of
//     both planes and of the exception mask that cover the window (each held against the packed space's end) and brings the window
//     down to bit 0 with v_alignbit_b32.  The alt window is the reference's with the two plane bits of base 63 replaced.
//   * allele_walk matches the 64 starts bit-parallel, as sites_kernel matches its 32: per pattern letter that is not N (a uniform
//     test: the patterns sit in LDS and PAM, strand and offset are loop counters) one funnel shift per plane and a selection among the
//     four base masks by the letter's set.  A start whose footprint holds an exception base or leaves the contig is cleared by a run
//     test (log2 steps) on the vector of bases that are plain and inside.  The first PAM that matches wins, per allele; the starts
//     whose footprint under a (PAM, strand) holds the SNV are a contiguous range.
//   * allele_count_kernel stores the lane's count and status, the workgroup's sum (wave reductions, the waves' sums added in LDS) and
//     adds the workgroup's three per-kind sums to the call's counters: at most three non-returning atomics.
//   * allele_write_kernel, after launch_sites_offsets over the workgroups' sums: the exclusive prefix of the workgroup's lane counts
//     (a wave scan, the earlier waves' sums from LDS), the same walk again, every record as two 16-byte stores at its place.
// Both kernels run the one allele_walk, so count and write cannot disagree.  No sort, no returning atomic.
#include "kernels.hpp"

#include <hip/hip_runtime.h>

namespace calitas {

namespace {

constexpr int ALLELE_WAVES = ALLELE_THREADS / 64;
constexpr uint32_t PAT_WORDS = sizeof(SitePatterns) / 4;
static_assert(sizeof(SitePatterns) % 4 == 0 && PAT_WORDS <= ALLELE_THREADS, "a word of the patterns per lane");

struct W128 { uint64_t a, b; };    // bits 0 .. 63, 64 .. 127

// bits [o, o + 64) of x, o = 0 .. 127 (zeros beyond bit 127)
CAL_DEV uint64_t take64(const W128& x, uint32_t o) {
  if (o >= 64u) return x.b >> (o - 64u);
  return o == 0u ? x.a : (x.a >> o) | (x.b << (64u - o));
}
CAL_DEV uint64_t ones64(int n) { return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull; }   // bits [0, n)
CAL_DEV W128 shr128(const W128& x, int s) { return W128{(x.a >> s) | (x.b << (64 - s)), x.b >> s}; }   // s = 1 .. 63

struct AlleleWindow {
  W128 lo_ref, hi_ref, lo_alt, hi_alt;   // the planes of the 127 bases around the SNV on either allele
};

// The records of SNV v in output order: emit(k, j, minus, kind, pam of the alt site, pam of the reference site, the window) for the
// k-th of them, start j of the window; returns their number and leaves the SNV's status in *status.
template <class Emit>
CAL_DEV uint32_t allele_walk(const AlleleArgs& a, const SitePatterns& pat, const Snv& v, uint32_t* status, Emit emit) {
  *status = 0;
  if (v.reserved == ALLELE_HOST_DECIDES) return 0;
  if (v.contig < 0 || v.contig >= a.n_contigs || v.position < 0) { *status = 2; return 0; }   // (cannot happen: the host has checked)
  const ContigInfo ci = a.contigs[v.contig];
  if ((uint64_t)v.position >= ci.len) { *status = 2; return 0; }                              // (nor this)
  const int64_t pos = v.position;
  const int64_t first = (int64_t)(ci.gbase + (uint64_t)pos) - 63;
  const int64_t wf = first >> 5;
  const uint32_t sh = (uint32_t)(first & 31);
  uint32_t l[5], h[5], e[5];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int64_t w = wf + i;
    const bool in = w >= 0 && (uint64_t)w < a.n_words;
    const uint2 p = in ? a.planes[w] : make_uint2(0u, 0u);
    l[i] = p.x; h[i] = p.y; e[i] = in ? a.mask[w] : 0xFFFFFFFFu;
  }
  AlleleWindow win;
  win.lo_ref.a = (uint64_t)__builtin_amdgcn_alignbit(l[1], l[0], sh) | ((uint64_t)__builtin_amdgcn_alignbit(l[2], l[1], sh) << 32);
  win.lo_ref.b = (uint64_t)__builtin_amdgcn_alignbit(l[3], l[2], sh) | ((uint64_t)__builtin_amdgcn_alignbit(l[4], l[3], sh) << 32);
  win.hi_ref.a = (uint64_t)__builtin_amdgcn_alignbit(h[1], h[0], sh) | ((uint64_t)__builtin_amdgcn_alignbit(h[2], h[1], sh) << 32);
  win.hi_ref.b = (uint64_t)__builtin_amdgcn_alignbit(h[3], h[2], sh) | ((uint64_t)__builtin_amdgcn_alignbit(h[4], h[3], sh) << 32);
  W128 plain;                                                        // base t is a plain one inside the contig
  plain.a = ~((uint64_t)__builtin_amdgcn_alignbit(e[1], e[0], sh) | ((uint64_t)__builtin_amdgcn_alignbit(e[2], e[1], sh) << 32));
  plain.b = ~((uint64_t)__builtin_amdgcn_alignbit(e[3], e[2], sh) | ((uint64_t)__builtin_amdgcn_alignbit(e[4], e[3], sh) << 32));
  {
    const int from = pos < 63 ? (int)(63 - pos) : 0;                 // base 0 of the contig
    const uint64_t left = ci.len - (uint64_t)pos;                    // >= 1
    const int to = left >= 65u ? 128 : 63 + (int)left;               // the contig's end
    plain.a &= ones64(to) & ~ones64(from);
    plain.b &= ones64(to - 64) & ~ones64(from - 64);
  }
  if (!((plain.a >> 63) & 1ull)) { *status = 2; return 0; }
  const uint32_t ref_code = (uint32_t)((win.lo_ref.a >> 63) & 1ull) | ((uint32_t)((win.hi_ref.a >> 63) & 1ull) << 1);
  if (v.ref != 0 && allele_code(v.ref) != ref_code) { *status = 1; return 0; }
  const uint32_t alt_code = allele_code(v.alt);
  if (alt_code == ref_code) { *status = 3; return 0; }
  const uint64_t snv_bit = 1ull << 63;
  win.lo_alt = win.lo_ref; win.hi_alt = win.hi_ref;
  win.lo_alt.a = (win.lo_alt.a & ~snv_bit) | ((alt_code & 1u) ? snv_bit : 0ull);
  win.hi_alt.a = (win.hi_alt.a & ~snv_bit) | ((alt_code & 2u) ? snv_bit : 0ull);

  // per strand: the starts with a site on either allele, the winning PAM's index bit by bit, the starts of a record
  uint64_t has_ref[2] = {0, 0}, has_alt[2] = {0, 0}, rec[2] = {0, 0};
  uint64_t kr0[2] = {0, 0}, kr1[2] = {0, 0}, kr2[2] = {0, 0}, ka0[2] = {0, 0}, ka1[2] = {0, 0}, ka2[2] = {0, 0};
  const int L = pat.proto_len;
  for (int k = 0; k < pat.n_pams; k++) {
    // run.bit t: the n = L + pam_len bases from t on are plain and inside (both strands' footprints have this length)
    const int n = L + pat.p[k][0].pam_len;
    W128 run = plain;
    for (int len = 1; len < n;) {
      const int step = len < n - len ? len : n - len;
      const W128 s = shr128(run, step);
      run.a &= s.a; run.b &= s.b;
      len += step;
    }
#pragma unroll
    for (int st = 0; st < 2; st++) {
      const SitePattern& sp = pat.p[k][st];
      const int lo = sp.lo, hi = sp.hi;
      uint64_t m_ref = take64(run, (uint32_t)(16 + lo)), m_alt = m_ref;
      for (int o = 16 + lo; o < 16 + hi; o++) {
        const uint32_t set = (sp.sets[o >> 3] >> (4 * (o & 7))) & 15u;
        if (set == 15u) continue;                                    // (uniform: a scalar branch)
        const uint64_t lr = take64(win.lo_ref, (uint32_t)o), hr = take64(win.hi_ref, (uint32_t)o);
        const uint64_t la = take64(win.lo_alt, (uint32_t)o), ha = take64(win.hi_alt, (uint32_t)o);
        const uint64_t sa = (set & 1u) ? ~0ull : 0ull, sc = (set & 2u) ? ~0ull : 0ull, sg = (set & 4u) ? ~0ull : 0ull, stt = (set & 8u) ? ~0ull : 0ull;
        m_ref &= (sa & ~lr & ~hr) | (sc & lr & ~hr) | (sg & ~lr & hr) | (stt & lr & hr);
        m_alt &= (sa & ~la & ~ha) | (sc & la & ~ha) | (sg & ~la & ha) | (stt & la & ha);
      }
      // the footprint [j + 16 + lo, j + 16 + hi) holds base 63: j = 48 - hi .. 47 - lo
      const uint64_t cover = ones64(48 - lo) & ~ones64(48 - hi);
      const uint64_t new_ref = m_ref & ~has_ref[st], new_alt = m_alt & ~has_alt[st];
      has_ref[st] |= new_ref; has_alt[st] |= new_alt;
      rec[st] |= (new_ref | new_alt) & cover;
      if (k & 1) { kr0[st] |= new_ref; ka0[st] |= new_alt; }
      if (k & 2) { kr1[st] |= new_ref; ka1[st] |= new_alt; }
      if (k & 4) { kr2[st] |= new_ref; ka2[st] |= new_alt; }
    }
  }
  uint32_t count = 0;
  for (uint64_t any = rec[0] | rec[1]; any; any &= any - 1ull) {
    const int j = __builtin_ctzll(any);
#pragma unroll
    for (int st = 0; st < 2; st++) {
      if (!((rec[st] >> j) & 1ull)) continue;
      const uint32_t kind = (uint32_t)((has_alt[st] >> j) & 1ull) + 2u * (uint32_t)((has_ref[st] >> j) & 1ull);
      const int k_alt = (int)(((ka0[st] >> j) & 1ull) | (((ka1[st] >> j) & 1ull) << 1) | (((ka2[st] >> j) & 1ull) << 2));
      const int k_ref = (int)(((kr0[st] >> j) & 1ull) | (((kr1[st] >> j) & 1ull) << 1) | (((kr2[st] >> j) & 1ull) << 2));
      emit(count, j, st != 0, kind, k_alt, k_ref, win);
      count++;
    }
  }
  return count;
}

CAL_DEV uint32_t allele_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

CAL_DEV void stage_patterns(SitePatterns& s_pat, const SitePatterns* pat, uint32_t tid) {
  if (tid < PAT_WORDS) reinterpret_cast<uint32_t*>(&s_pat)[tid] = reinterpret_cast<const uint32_t*>(pat)[tid];
  __syncthreads();
}

__global__ __launch_bounds__(ALLELE_THREADS) void allele_count_kernel(AlleleArgs a) {
  __shared__ SitePatterns s_pat;
  __shared__ uint32_t s_by[ALLELE_WAVES][4];
  const uint32_t tid = threadIdx.x;
  stage_patterns(s_pat, a.pat, tid);
  const uint64_t r = (uint64_t)blockIdx.x * ALLELE_THREADS + tid;
  uint32_t by1 = 0, by2 = 0, by3 = 0;
  if (r < a.n) {
    uint32_t status = 0;
    a.lane_count[r] = allele_walk(a, s_pat, a.snvs[r], &status, [&](uint32_t, int, bool, uint32_t kind, int, int, const AlleleWindow&) {
      by1 += kind == 1u ? 1u : 0u; by2 += kind == 2u ? 1u : 0u; by3 += kind == 3u ? 1u : 0u;
    });
    a.status[r] = (uint8_t)status;
  }
  by1 = allele_wave_sum(by1); by2 = allele_wave_sum(by2); by3 = allele_wave_sum(by3);
  if ((tid & 63u) == 0) { uint32_t* s = s_by[tid >> 6]; s[0] = 0; s[1] = by1; s[2] = by2; s[3] = by3; }
  __syncthreads();
  if (tid >= 1 && tid < 4) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < ALLELE_WAVES; k++) sum += s_by[k][tid];
    if (sum) (void)atomicAdd(&a.per_kind[tid], (unsigned long long)sum);
  }
  if (tid == 0) {
    uint32_t sum = 0;                                                // (at most 256 x 96: no overflow)
#pragma unroll
    for (int k = 0; k < ALLELE_WAVES; k++) sum += s_by[k][1] + s_by[k][2] + s_by[k][3];
    a.wg_count[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(ALLELE_THREADS) void allele_write_kernel(AlleleArgs a) {
  __shared__ SitePatterns s_pat;
  __shared__ uint32_t s_wave[ALLELE_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  stage_patterns(s_pat, a.pat, tid);
  const uint64_t r = (uint64_t)blockIdx.x * ALLELE_THREADS + tid;
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
  for (uint32_t k = 0; k < ALLELE_WAVES; k++) before += k < (tid >> 6) ? s_wave[k] : 0u;
  const uint64_t base = a.wg_offset[blockIdx.x] + before;
  const Snv v = a.snvs[r];
  const int L = s_pat.proto_len;
  const bool pamless = s_pat.pamless != 0;
  uint32_t status = 0;
  (void)allele_walk(a, s_pat, v, &status, [&](uint32_t k, int j, bool minus, uint32_t kind, int k_alt, int k_ref, const AlleleWindow& win) {
    const uint64_t at = base + k;
    if (k >= mine || at >= a.out_capacity) return;                   // (cannot happen: count and offsets come from this very walk)
    const bool alt = (kind & 1u) != 0;
    const int pam = alt ? k_alt : k_ref;
    const SitePattern& sp = s_pat.p[pam][minus ? 1 : 0];
    const int32_t p = v.position - 47 + j;
    const int32_t pam_start = pamless ? -1 : p + sp.pam_off;
    const uint32_t pam_index = pamless ? 0xFFu : (uint32_t)pam;
    const uint32_t other = (kind == 3u && !pamless) ? (uint32_t)k_ref : 0xFFu;
    const int32_t offset = minus ? p + L - 1 - v.position : v.position - p;
    const uint32_t w_lo = (uint32_t)take64(alt ? win.lo_alt : win.lo_ref, (uint32_t)(j + 16));
    const uint32_t w_hi = (uint32_t)take64(alt ? win.hi_alt : win.hi_ref, (uint32_t)(j + 16));
    const uint64_t guide = copies_key(w_lo, w_hi, L, L, minus, false);
    uint4* out = reinterpret_cast<uint4*>(a.out + at);
    out[0] = make_uint4((uint32_t)v.contig, (uint32_t)p, (uint32_t)pam_start,
                        (uint32_t)(minus ? '-' : '+') | (pam_index << 8) | ((uint32_t)sp.pam_len << 16) | ((uint32_t)L << 24));
    out[1] = make_uint4((uint32_t)r, kind | (other << 8) | (((uint32_t)offset & 0xFFu) << 16), (uint32_t)guide, (uint32_t)(guide >> 32));
  });
}

}  // namespace

hipError_t launch_allele_count(const AlleleArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(allele_count_kernel, dim3(allele_blocks(a.n)), dim3(ALLELE_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_allele_write(const AlleleArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(allele_write_kernel, dim3(allele_blocks(a.n)), dim3(ALLELE_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace calitas
