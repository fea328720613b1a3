// activity.hip -- on-target activity of guide sites (calitas_find_sites_scored, gfx950).  No reference counterpart.
//
// The site kernel's second pass leaves its records on the device; here one lane takes one record.
//   * activity_score_kernel: the lane reads its 16-byte record, finds the leftmost forward base of the record's window of W = up + L +
//     down bases and holds the window against the contig BEFORE it loads anything: a window that leaves the contig has no score and
//     reads nothing.  Otherwise three consecutive 32-base words of the planes and of the exception mask cover any window of up to 64
//     bases; two v_alignbit_b32 per plane bring the window down to bit 0.  '-' reads the reverse complement: the planes' bits in
//     reverse order and complemented, as copies_key does.  G + C of the protospacer is a popcount of lo ^ hi over its bits.  The model
//     is one block of words in LDS (kernels.hpp has the layout), `single` folded into the pair table by the host, so a position costs
//     one LDS read.  A window with an exception bit -- an N, an IUPAC code, a U: the device cannot tell them apart -- stores
//     ACTIVITY_HOST_DECIDES and is always kept.  With a threshold the workgroup stores how many of its records are kept: a ballot and
//     a popcount per wave, the waves' counts added in LDS, no global atomic.
//   * activity_compact_kernel: after launch_sites_offsets over those counts, every kept lane writes record and score at its
//     workgroup's offset + its rank -- mbcnt of the wave's ballot plus the counts of the waves before it.  The order stays: no sort, no
//     returning atomic.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"

namespace calitas {

namespace {

constexpr int WAVES = ACTIVITY_THREADS / 64;

CAL_DEV bool activity_kept(int32_t score, int32_t min_score) { return score >= min_score || score == ACTIVITY_HOST_DECIDES; }

// the lanes of the wave before this one whose bit is set
CAL_DEV uint32_t rank_in_wave(uint64_t ballot) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

__global__ __launch_bounds__(ACTIVITY_THREADS) void activity_score_kernel(ActivityArgs a) {
  __shared__ int32_t s_table[ACTIVITY_TABLE_MAX_WORDS];
  __shared__ uint32_t s_kept[WAVES];
  const uint32_t tid = threadIdx.x;
  const int L = a.L, up = a.up, down = a.down, W = up + L + down;
  const uint32_t n_table = activity_table_words(L, W);
  for (uint32_t i = tid; i < n_table; i += ACTIVITY_THREADS) s_table[i] = a.table[i];
  __syncthreads();

  const uint64_t r = (uint64_t)blockIdx.x * ACTIVITY_THREADS + tid;
  const bool live = r < a.n;
  int32_t score = ACTIVITY_NONE;
  if (live) {
    const uint4 rec = reinterpret_cast<const uint4*>(a.recs)[r];     // contig, proto_start, pam_start, {strand, pam_index, pam_len, proto_len}
    const int32_t contig = (int32_t)rec.x;
    const bool minus = (rec.w & 0xFFu) == (uint32_t)'-';
    const int64_t left = (int64_t)(int32_t)rec.y - (minus ? down : up);
    bool inside = contig >= 0 && contig < a.n_contigs && left >= 0;
    uint64_t g = 0;
    if (inside) {
      const ContigInfo ci = a.contigs[contig];
      inside = (uint64_t)left + (uint64_t)W <= ci.len;
      g = ci.gbase + (uint64_t)left;
      inside = inside && (g >> 5) + 2 < a.n_words;                   // (contigs end a padding tile before the planes do)
    }
    if (inside) {
      const uint64_t w = g >> 5;
      const uint32_t sh = (uint32_t)(g & 31u);
      const uint2 p0 = a.planes[w], p1 = a.planes[w + 1], p2 = a.planes[w + 2];
      const uint32_t e0 = a.mask[w], e1 = a.mask[w + 1], e2 = a.mask[w + 2];
      const uint64_t wm = W == 64 ? ~0ull : (1ull << W) - 1ull;
      uint64_t lo = (uint64_t)__builtin_amdgcn_alignbit(p1.x, p0.x, sh) | ((uint64_t)__builtin_amdgcn_alignbit(p2.x, p1.x, sh) << 32);
      uint64_t hi = (uint64_t)__builtin_amdgcn_alignbit(p1.y, p0.y, sh) | ((uint64_t)__builtin_amdgcn_alignbit(p2.y, p1.y, sh) << 32);
      const uint64_t ex = (uint64_t)__builtin_amdgcn_alignbit(e1, e0, sh) | ((uint64_t)__builtin_amdgcn_alignbit(e2, e1, sh) << 32);
      if (ex & wm) score = ACTIVITY_HOST_DECIDES;
      else {
        if (minus) {                                                 // the guide reads the reverse complement
          lo = __builtin_bitreverse64(~lo) >> (64 - W);
          hi = __builtin_bitreverse64(~hi) >> (64 - W);
        }
        const uint32_t proto = 0xFFFFFFFFu >> (32 - L);
        const int gc = __builtin_popcount((uint32_t)((lo ^ hi) >> up) & proto);   // C = 01, G = 10
        const int32_t* tail = s_table + 16 * (W - 1);
        int32_t sum = tail[4 + (L + 1)] + tail[4 + gc];              // the intercept, gc[.]
        uint32_t c = ((uint32_t)lo & 1u) | (((uint32_t)hi & 1u) << 1);
        for (int i = 0; i + 1 < W; i++) {
          lo >>= 1; hi >>= 1;
          const uint32_t next = ((uint32_t)lo & 1u) | (((uint32_t)hi & 1u) << 1);
          sum += s_table[16 * i + (int)(4u * c + next)];
          c = next;
        }
        score = sum + tail[c];
      }
    }
    a.scores[r] = score;
  }
  if (a.wg_kept) {                                                   // (the same for every lane)
    const uint64_t ballot = __builtin_amdgcn_ballot_w64(live && activity_kept(score, a.min_score));
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

__global__ __launch_bounds__(ACTIVITY_THREADS) void activity_compact_kernel(const SiteRecord* recs, const int32_t* scores, uint64_t n, int32_t min_score,
                                                                            const uint64_t* wg_offset, SiteRecord* out_recs, int32_t* out_scores,
                                                                            uint64_t out_capacity) {
  __shared__ uint32_t s_kept[WAVES];
  const uint32_t tid = threadIdx.x;
  const uint64_t r = (uint64_t)blockIdx.x * ACTIVITY_THREADS + tid;
  const bool live = r < n;
  const int32_t score = live ? scores[r] : ACTIVITY_NONE;
  const bool keep = live && activity_kept(score, min_score);
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
  out_scores[at] = score;
}

}  // namespace

hipError_t launch_activity_score(const ActivityArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(activity_score_kernel, dim3(activity_blocks(a.n)), dim3(ACTIVITY_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_activity_compact(const SiteRecord* recs, const int32_t* scores, uint64_t n, int32_t min_score, const uint64_t* wg_offset,
                                   SiteRecord* out_recs, int32_t* out_scores, uint64_t out_capacity, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(activity_compact_kernel, dim3(activity_blocks(n)), dim3(ACTIVITY_THREADS), 0, stream, recs, scores, n, min_score, wg_offset, out_recs,
                     out_scores, out_capacity);
  return hipGetLastError();
}

}  // namespace calitas
