// near_list.hip -- the two kernels of calitas_list_near (gfx950): the near kernel's pass with the records as its ending,
// sites_kernel<false, false, KEYS_NEAR_LIST>, and near_order_kernel, which puts every query's stretch of records in position order.
// No reference counterpart.
// sites_kernel and everything it is made of live in sites.hip, which is included here with its own kernels' launchers left out: this
// translation unit instantiates the one new ending and nothing else, and sites.hip's code object -- the kernels of calitas_find_sites,
// calitas_count_copies, calitas_count_near and calitas_score_near -- is the same bytes with and without the listing.
#define CALITAS_SITES_KERNEL_ONLY
#include "sites.hip"

namespace calitas {

namespace {

// calitas_list_near: a stretch of the near kernel's records in position order.  The records' position keys -- contig, protospacer
// start, strand: unique in a stretch -- go to LDS, every record counts the keys below its own, and that rank is its place in `out`,
// which has the layout of `in`.  keys[blockIdx.x]: the distinct key whose stretch this is; cursors: SitesArgs::wg_count of the pass.
// A cursor that did not end at the stretch's length raises the call's flag (the ranks stay inside the stretch whatever `in` holds).
// A stretch longer than CAP is copied as it is: the host orders the few that a U made longer than any limit.
template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void near_order_kernel(const NearHit* in, NearHit* out, const uint64_t* base, uint32_t* cursors, const uint32_t* keys,
                                                             uint32_t flag_index) {
  __shared__ uint64_t s_pos[CAP];
  const uint32_t tid = threadIdx.x, k = keys[blockIdx.x], len = cursors[2u * k + 1u];
  const uint4* from = reinterpret_cast<const uint4*>(in + base[k]);
  uint4* to = reinterpret_cast<uint4*>(out + base[k]);
  if (tid == 0 && cursors[2u * k] != len) cursors[flag_index] = 1u;
  if (len > (uint32_t)CAP) {                                   // (uniform)
    for (uint32_t i = tid; i < 2u * len; i += THREADS) to[i] = from[i];
    return;
  }
  for (uint32_t i = tid; i < len; i += THREADS) {
    const uint4 head = from[2u * i];
    s_pos[i] = ((uint64_t)head.z << 33) | ((uint64_t)head.w << 1) | (uint64_t)((from[2u * i + 1u].w & 0xFFu) == (uint32_t)'-');
  }
  __syncthreads();
  for (uint32_t i = tid; i < len; i += THREADS) {
    const uint64_t mine = s_pos[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < len; j++) rank += s_pos[j] < mine ? 1u : 0u;
    to[2u * rank] = from[2u * i];
    to[2u * rank + 1u] = from[2u * i + 1u];
  }
}

}  // namespace

hipError_t launch_sites_near_list(const SitesArgs& a, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  hipLaunchKernelGGL((sites_kernel<false, false, KEYS_NEAR_LIST>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_near_order(const NearHit* in, NearHit* out, const uint64_t* base, uint32_t* cursors, const uint32_t* keys, uint32_t n_short, uint32_t n_long,
                             uint32_t flag_index, hipStream_t stream) {
  if (n_short) hipLaunchKernelGGL((near_order_kernel<(int)NEAR_ORDER_SHORT, 64>), dim3(n_short), dim3(64), 0, stream, in, out, base, cursors, keys, flag_index);
  if (n_long) hipLaunchKernelGGL((near_order_kernel<(int)NEAR_ORDER_LONG, 256>), dim3(n_long), dim3(256), 0, stream, in, out, base, cursors, keys + n_short, flag_index);
  return hipGetLastError();
}

}  // namespace calitas
