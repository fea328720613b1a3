// microhomology.hip -- microhomology and out-of-frame scores of guide sites (calitas_find_sites_microhomology, gfx950).  No reference
// counterpart.
//
// The site kernel's second pass leaves its records on the device; here one lane takes one record.
//   * mh_score_kernel: the lane reads its 16-byte record, finds the forward cut and the leftmost forward base of the window of
//     W = left + right bases, and holds the window against the contig BEFORE it loads anything: a window that leaves the contig has no
//     score and reads nothing.  Otherwise three consecutive 32-base words of the planes and of the exception mask cover any window of up
//     to 64 bases; two v_alignbit_b32 per plane bring the window down to bit 0.  '-' reads the reverse complement: the planes' bits in
//     reverse order and complemented, as activity_score_kernel does.  Letter x[i] is then bit i of the two planes.  A deletion of d
//     bases pairs x[i] with x[i + d]: the planes shifted down by d, XORed with themselves, are 0 in both exactly where the letters are
//     equal.  Only i < left <= 32 can lie left of the cut, so everything behind the two 64-bit shifts is 32-bit: e, the matches within
//     [lo(d), hi(d)); r, where a run of min_length starts; run, the bases of the runs of min_length and more.  The sum over the
//     diagonal's maximal runs of k + g is popc(run) + popc(run & (lo ^ hi)) (C = 01, G = 10).  d, the bounds of the diagonal, d % 3 and
//     weight[d - 1] are the same in every lane: loop counters and loads from the argument block, no LDS.  The loop runs for every lane
//     of the wave, on zeros where a lane has no window, so nothing in it depends on the lane but the planes.  A window with an exception
//     bit -- an N, an IUPAC code, a U: the device cannot tell them apart -- stores MH_HOST_DECIDES and is always kept.  With a
//     threshold the workgroup stores how many of its records are kept: a ballot and a popcount per wave, the waves' counts added in
//     LDS, no global atomic.
//   * mh_compact_kernel: after launch_sites_offsets over those counts, every kept lane writes record and score at its workgroup's
//     offset + its rank -- mbcnt of the wave's ballot plus the counts of the waves before it.  The order stays: no sort, no returning
//     atomic.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"

namespace calitas {

namespace {

constexpr int WAVES = MH_THREADS / 64;

// the lanes of the wave before this one whose bit is set
CAL_DEV uint32_t rank_in_wave(uint64_t ballot) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

__global__ __launch_bounds__(MH_THREADS) void mh_score_kernel(MhArgs a) {
  __shared__ uint32_t s_kept[WAVES];
  const uint32_t tid = threadIdx.x;
  const int L = a.L, left = a.left, right = a.right, W = left + right, m = a.min_length;

  const uint64_t r = (uint64_t)blockIdx.x * MH_THREADS + tid;
  const bool live = r < a.n;
  bool scored = false, host = false;
  uint64_t lo = 0, hi = 0;
  if (live) {
    const uint4 rec = reinterpret_cast<const uint4*>(a.recs)[r];     // contig, proto_start, pam_start, {strand, pam_index, pam_len, proto_len}
    const int32_t contig = (int32_t)rec.x;
    const bool minus = (rec.w & 0xFFu) == (uint32_t)'-';
    const int64_t cut = (int64_t)(int32_t)rec.y + (minus ? L - a.cut : a.cut);
    const int64_t first = cut - (minus ? right : left);
    bool inside = contig >= 0 && contig < a.n_contigs && first >= 0;
    uint64_t g = 0;
    if (inside) {
      const ContigInfo ci = a.contigs[contig];
      inside = (uint64_t)first + (uint64_t)W <= ci.len;
      g = ci.gbase + (uint64_t)first;
      inside = inside && (g >> 5) + 2 < a.n_words;                   // (contigs end a padding tile before the planes do)
    }
    if (inside) {
      const uint64_t w = g >> 5;
      const uint32_t sh = (uint32_t)(g & 31u);
      const uint2 p0 = a.planes[w], p1 = a.planes[w + 1], p2 = a.planes[w + 2];
      const uint32_t e0 = a.mask[w], e1 = a.mask[w + 1], e2 = a.mask[w + 2];
      const uint64_t wm = W == 64 ? ~0ull : (1ull << W) - 1ull;
      lo = (uint64_t)__builtin_amdgcn_alignbit(p1.x, p0.x, sh) | ((uint64_t)__builtin_amdgcn_alignbit(p2.x, p1.x, sh) << 32);
      hi = (uint64_t)__builtin_amdgcn_alignbit(p1.y, p0.y, sh) | ((uint64_t)__builtin_amdgcn_alignbit(p2.y, p1.y, sh) << 32);
      const uint64_t ex = (uint64_t)__builtin_amdgcn_alignbit(e1, e0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(e2, e1, sh) << 32);
      host = (ex & wm) != 0;
      scored = !host;
      if (minus) {                                                   // the guide reads the reverse complement
        lo = __builtin_bitreverse64(~lo) >> (64 - W);
        hi = __builtin_bitreverse64(~hi) >> (64 - W);
      } else {
        lo &= wm; hi &= wm;
      }
    }
  }

  // every diagonal: nothing below depends on the lane but lo and hi
  const uint32_t x_lo = (uint32_t)lo, x_hi = (uint32_t)hi, gc = x_lo ^ x_hi;
  uint32_t total = 0, out_of_frame = 0;
  int d3 = 1;                                                        // d % 3
  for (int d = 1; d < W; d++) {
    const int from = left - d > 0 ? left - d : 0, to = W - d < left ? W - d : left;   // lo(d), hi(d); to <= 32
    const uint32_t valid = (uint32_t)(((1ull << to) - 1ull) & ~((1ull << from) - 1ull));
    const uint32_t e = ~((x_lo ^ (uint32_t)(lo >> d)) | (x_hi ^ (uint32_t)(hi >> d))) & valid;
    uint32_t s = e;                                                  // bit i: a run of m matches starts at i
    for (int k = 1; k < m; k++) s &= e >> k;
    uint32_t run = s;                                                // the bases of the runs of m and more (they end below `to`)
    for (int k = 1; k < m; k++) run |= s << k;
    const uint32_t term = a.weight[d - 1] * (uint32_t)(__builtin_popcount(run) + __builtin_popcount(run & gc));
    total += term;
    if (d3 != 0) out_of_frame += term;
    d3 = d3 == 2 ? 0 : d3 + 1;
  }

  MhScore score;
  score.total = scored ? total : MH_NONE;
  score.out_of_frame = scored ? out_of_frame : host ? MH_HOST_DECIDES : MH_NONE;
  if (live) reinterpret_cast<uint2*>(a.scores)[r] = make_uint2(score.total, score.out_of_frame);
  if (a.wg_kept) {                                                   // (the same for every lane)
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(live && mh_kept(score, a.permille));
    if ((tid & 63u) == 0) s_kept[tid >> 6] = (uint32_t)__builtin_popcountll(ballot);
    __syncthreads();
    if (tid == 0) {
      uint32_t kept = 0;
#pragma unroll
      for (int k = 0; k < WAVES; k++) kept += s_kept[k];
      a.wg_kept[blockIdx.x] = kept;
    }
  }
}

__global__ __launch_bounds__(MH_THREADS) void mh_compact_kernel(const SiteRecord* recs, const MhScore* scores, uint64_t n, uint32_t permille,
                                                                const uint64_t* wg_offset, SiteRecord* out_recs, MhScore* out_scores,
                                                                uint64_t out_capacity) {
  __shared__ uint32_t s_kept[WAVES];
  const uint32_t tid = threadIdx.x;
  const uint64_t r = (uint64_t)blockIdx.x * MH_THREADS + tid;
  const bool live = r < n;
  uint2 word = make_uint2(MH_NONE, MH_NONE);
  if (live) word = reinterpret_cast<const uint2*>(scores)[r];
  MhScore score;
  score.total = word.x; score.out_of_frame = word.y;
  const bool keep = live && mh_kept(score, permille);
  const uint64_t ballot = __builtin_amdgcn_ballot_w64(keep);
  if ((tid & 63u) == 0) s_kept[tid >> 6] = (uint32_t)__builtin_popcountll(ballot);
  __syncthreads();
  if (!keep) return;
  uint32_t before = rank_in_wave(ballot);
#pragma unroll
  for (uint32_t k = 0; k < WAVES; k++) before += k < (tid >> 6) ? s_kept[k] : 0u;
  const uint64_t at = wg_offset[blockIdx.x] + before;
  if (at >= out_capacity) return;                                    // (cannot happen: the offsets are the scan of these very counts)
  reinterpret_cast<uint4*>(out_recs)[at] = reinterpret_cast<const uint4*>(recs)[r];
  reinterpret_cast<uint2*>(out_scores)[at] = word;
}

}  // namespace

hipError_t launch_mh_score(const MhArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(mh_score_kernel, dim3(mh_blocks(a.n)), dim3(MH_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_mh_compact(const SiteRecord* recs, const MhScore* scores, uint64_t n, uint32_t permille, const uint64_t* wg_offset,
                             SiteRecord* out_recs, MhScore* out_scores, uint64_t out_capacity, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mh_compact_kernel, dim3(mh_blocks(n)), dim3(MH_THREADS), 0, stream, recs, scores, n, permille, wg_offset, out_recs, out_scores,
                     out_capacity);
  return hipGetLastError();
}

}  // namespace calitas
