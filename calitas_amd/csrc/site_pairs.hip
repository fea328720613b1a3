// site_pairs.hip -- the sites of a pattern paired by cut distance and orientation (calitas_find_site_pairs, gfx950).
// No reference counterpart.
//
// The records the site kernel's write pass left on the device are in listing order: contig, protospacer start, '+' before '-'.  One
// lane per record i walks the records behind it (pair_walk) and takes every j > i that makes a pair with it.
//   * pair_count_kernel: the lane stores its count; the workgroup stores the sum of its lanes' counts (a wave reduction, the four
//     waves' sums added in LDS) and adds its four per-orientation sums to the call's counters, at most four non-returning atomics.
//   * pair_write_kernel: after launch_sites_offsets over the workgroups' sums.  The lane takes the exclusive prefix of its
//     workgroup's lane counts (a wave scan, the earlier waves' sums from LDS), repeats the walk and stores pair k at its workgroup's
//     offset + that prefix + k: the pairs leave in (i, j) order, no sort, no returning atomic.
// Both kernels run the one pair_walk, so count and write cannot disagree about which pairs there are or how many.
#include "kernels.hpp"

#include <hip/hip_runtime.h>

namespace calitas {

namespace {

constexpr int PAIR_WAVES = SITE_PAIR_THREADS / 64;

// The partners j > i of record i, in ascending j: emit(k, j, cut_j - cut_i, orientation) for the k-th of them; returns their number.
// A record's cut is its start + rule.cut or + L - rule.cut, so cut_j - cut_i differs from start_j - start_i by at most
// rule.slack = |L - 2 cut|:
//   * start_j - start_i > max_distance + slack: the cuts are more than max_distance apart, for this j and every later one of the
//     contig (the starts ascend) -- the walk ends;
//   * start_j - start_i < min_distance - slack: -slack <= cut_j - cut_i < min_distance, and with min_distance > slack that is no pair
//     -- the walk begins at the first j that is not so, found by bisection over the sorted records.
template <class Emit>
CAL_DEV uint32_t pair_walk(const SitePairArgs& a, uint64_t i, Emit emit) {
  const uint4* recs = reinterpret_cast<const uint4*>(a.recs);        // contig, proto_start, pam_start, {strand, pam_index, pam_len, proto_len}
  const SitePairRule& rule = a.rule;
  const uint4 me = recs[i];
  const int32_t contig = (int32_t)me.x;
  const int64_t start = (int64_t)(int32_t)me.y;
  const bool minus = (me.w & 0xFFu) == (uint32_t)'-';
  const int32_t cut = site_cut(rule, (int32_t)me.y, minus);
  uint64_t j = i + 1;
  if (rule.min_distance > rule.slack) {
    const int64_t from = start + rule.min_distance - rule.slack;
    uint64_t lo = i + 1, hi = a.n;                                   // the first record of [lo, hi) of another contig or at `from` or beyond
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      const uint4 m = recs[mid];
      if ((int32_t)m.x == contig && (int64_t)(int32_t)m.y < from) lo = mid + 1; else hi = mid;
    }
    j = lo;
  }
  const int64_t reach = (int64_t)rule.max_distance + rule.slack;
  uint32_t k = 0;
  for (; j < a.n; j++) {
    const uint4 other = recs[j];
    if ((int32_t)other.x != contig || (int64_t)(int32_t)other.y - start > reach) break;
    const bool other_minus = (other.w & 0xFFu) == (uint32_t)'-';
    const int32_t other_cut = site_cut(rule, (int32_t)other.y, other_minus);
    const int o = site_pair_orientation(rule, cut, minus, other_cut, other_minus);
    if (o < 0) continue;
    emit(k, j, other_cut - cut, o);
    k++;
  }
  return k;
}

CAL_DEV uint32_t pair_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

__global__ __launch_bounds__(SITE_PAIR_THREADS) void pair_count_kernel(SitePairArgs a) {
  __shared__ uint32_t s_by[PAIR_WAVES][4];
  const uint32_t tid = threadIdx.x;
  const uint64_t r = (uint64_t)blockIdx.x * SITE_PAIR_THREADS + tid;
  uint32_t by0 = 0, by1 = 0, by2 = 0, by3 = 0;
  if (r < a.n) {
    a.lane_count[r] = pair_walk(a, r, [&](uint32_t, uint64_t, int32_t, int o) {
      by0 += o == 0 ? 1u : 0u; by1 += o == 1 ? 1u : 0u; by2 += o == 2 ? 1u : 0u; by3 += o == 3 ? 1u : 0u;
    });
  }
  by0 = pair_wave_sum(by0); by1 = pair_wave_sum(by1); by2 = pair_wave_sum(by2); by3 = pair_wave_sum(by3);
  if ((tid & 63u) == 0) { uint32_t* s = s_by[tid >> 6]; s[0] = by0; s[1] = by1; s[2] = by2; s[3] = by3; }
  __syncthreads();
  if (tid < 4) {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < PAIR_WAVES; k++) sum += s_by[k][tid];
    if (sum) (void)atomicAdd(&a.per_orientation[tid], (unsigned long long)sum);
  }
  if (tid == 0) {
    uint32_t sum = 0;                                                // (a lane has fewer than 2^18 partners: no overflow)
#pragma unroll
    for (int k = 0; k < PAIR_WAVES; k++) sum += s_by[k][0] + s_by[k][1] + s_by[k][2] + s_by[k][3];
    a.wg_count[blockIdx.x] = sum;
  }
}

__global__ __launch_bounds__(SITE_PAIR_THREADS) void pair_write_kernel(SitePairArgs a) {
  __shared__ uint32_t s_wave[PAIR_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * SITE_PAIR_THREADS + tid;
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
  for (uint32_t k = 0; k < PAIR_WAVES; k++) before += k < (tid >> 6) ? s_wave[k] : 0u;
  const uint64_t base = a.wg_offset[blockIdx.x] + before;
  const uint32_t i = (uint32_t)r;
  (void)pair_walk(a, r, [&](uint32_t k, uint64_t j, int32_t d, int o) {
    const uint64_t at = base + k;
    if (k >= mine || at >= a.out_capacity) return;                   // (cannot happen: count and offsets come from this very walk)
    const uint32_t left = d < 0 ? (uint32_t)j : i, right = d < 0 ? i : (uint32_t)j;
    reinterpret_cast<uint4*>(a.out)[at] = make_uint4(left, right, (uint32_t)(d < 0 ? -d : d), (uint32_t)o);
  });
}

}  // namespace

hipError_t launch_site_pairs_count(const SitePairArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(pair_count_kernel, dim3(site_pair_blocks(a.n)), dim3(SITE_PAIR_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_site_pairs_write(const SitePairArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(pair_write_kernel, dim3(site_pair_blocks(a.n)), dim3(SITE_PAIR_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace calitas
