// site_regions.hip -- the sites of a pattern classed by the context's annotated regions (calitas_find_sites_regions, gfx950).
// No reference counterpart.
//
//   * sites_kernel<., ., KEYS_REGIONS>: the two find passes of sites.hip with the presence test -- a segment none of whose sites can
//     have a wanted class is dead before a word of it is loaded.  sites_kernel and everything it is made of live in sites.hip, which is
//     included here with its own kernels' launchers left out, as near_list.hip does: sites.hip's code object stays the bytes it was.
//   * site_class_kernel: the records the write pass left on the device, one lane per record.  The lane reads its 16-byte record, turns
//     strand, protospacer start and the call's {from, to} into a forward extent of at most 32 bases and classes it with regions.hpp's
//     region_class, the function calitas_search_regions classes a hit with.  It stores one byte, the class and a keep flag.  The kept
//     records of the workgroup are a ballot and a popcount per wave; the (class, strand) cells are counted in LDS and leave the
//     workgroup as at most 16 non-returning atomics.
//   * site_class_compact_kernel: after launch_sites_offsets over the workgroups' kept counts every kept lane writes its record and
//     class at its workgroup's offset + its rank (mbcnt of the wave's ballot plus the waves before it), as activity_compact_kernel
//     does: the order stays, no sort, no returning atomic.
#define CALITAS_SITES_KERNEL_ONLY
#include "sites.hip"

#include "site_regions.hpp"

namespace calitas {

namespace {

constexpr int CLASS_WAVES = SITE_CLASS_THREADS / 64;

// the lanes of the wave before this one whose bit is set
CAL_DEV uint32_t class_rank_in_wave(uint64_t ballot) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

__global__ __launch_bounds__(SITE_CLASS_THREADS) void site_class_kernel(SiteClassArgs a) {
  __shared__ uint32_t s_kept[CLASS_WAVES];
  __shared__ uint32_t s_cells[SITE_CLASS_CELLS];
  const uint32_t tid = threadIdx.x;
  if (tid < SITE_CLASS_CELLS) s_cells[tid] = 0u;
  __syncthreads();
  const uint64_t r = (uint64_t)blockIdx.x * SITE_CLASS_THREADS + tid;
  bool keep = false;
  if (r < a.n) {
    const uint4 rec = reinterpret_cast<const uint4*>(a.recs)[r];     // contig, proto_start, pam_start, {strand, pam_index, pam_len, proto_len}
    const int32_t contig = (int32_t)rec.x;
    const bool minus = (rec.w & 0xFFu) == (uint32_t)'-';
    uint32_t cls = 0u;
    if (contig >= 0 && contig < a.n_contigs)                         // (every record of the write pass)
      cls = site_region_class(a.rv, (uint32_t)contig, (int64_t)(int32_t)rec.y, (int)(rec.w >> 24), minus, a.ext_from, a.ext_to, a.contigs[contig].len);
    cls &= SITE_CLASS_CELLS / 2 - 1u;
    keep = ((a.class_mask >> cls) & 1u) != 0u;
    a.cls[r] = (uint8_t)(cls | (keep ? SITE_CLASS_KEEP : 0u));
    if (keep) (void)atomicAdd(&s_cells[2u * cls + (minus ? 1u : 0u)], 1u);
  }
  const uint64_t ballot = __builtin_amdgcn_ballot_w64(keep);
  if ((tid & 63u) == 0) s_kept[tid >> 6] = (uint32_t)__builtin_popcountll(ballot);
  __syncthreads();
  if (tid == 0) {
    uint32_t kept = 0;
#pragma unroll
    for (int k = 0; k < CLASS_WAVES; k++) kept += s_kept[k];
    a.wg_kept[blockIdx.x] = kept;
  }
  if (tid < SITE_CLASS_CELLS && s_cells[tid]) (void)atomicAdd(&a.cells[tid], (unsigned long long)s_cells[tid]);
}

__global__ __launch_bounds__(SITE_CLASS_THREADS) void site_class_compact_kernel(const SiteRecord* recs, const uint8_t* cls, uint64_t n, const uint64_t* wg_offset,
                                                                                SiteRecord* out_recs, uint8_t* out_cls, uint64_t out_capacity) {
  __shared__ uint32_t s_kept[CLASS_WAVES];
  const uint32_t tid = threadIdx.x;
  const uint64_t r = (uint64_t)blockIdx.x * SITE_CLASS_THREADS + tid;
  const uint32_t mine = r < n ? (uint32_t)cls[r] : 0u;
  const bool keep = (mine & SITE_CLASS_KEEP) != 0u;
  const uint64_t ballot = __builtin_amdgcn_ballot_w64(keep);
  if ((tid & 63u) == 0) s_kept[tid >> 6] = (uint32_t)__builtin_popcountll(ballot);
  __syncthreads();
  if (!keep) return;
  uint32_t before = class_rank_in_wave(ballot);
#pragma unroll
  for (uint32_t k = 0; k < CLASS_WAVES; k++) before += k < (tid >> 6) ? s_kept[k] : 0u;
  const uint64_t at = wg_offset[blockIdx.x] + before;
  if (at >= out_capacity) return;                                    // (cannot happen: the offsets are the scan of these very counts)
  reinterpret_cast<uint4*>(out_recs)[at] = reinterpret_cast<const uint4*>(recs)[r];
  out_cls[at] = (uint8_t)(mine & ~SITE_CLASS_KEEP);
}

}  // namespace

hipError_t launch_sites_regions_count(const SitesArgs& a, bool filtered, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  if (filtered) hipLaunchKernelGGL((sites_kernel<false, true, KEYS_REGIONS>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  else hipLaunchKernelGGL((sites_kernel<false, false, KEYS_REGIONS>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sites_regions_write(const SitesArgs& a, bool filtered, hipStream_t stream) {
  if (a.n_segs == 0) return hipSuccess;
  const uint32_t n_blocks = (a.n_segs + a.segs_per_wg - 1) / a.segs_per_wg;
  if (filtered) hipLaunchKernelGGL((sites_kernel<true, true, KEYS_REGIONS>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  else hipLaunchKernelGGL((sites_kernel<true, false, KEYS_REGIONS>), dim3(n_blocks), dim3(SITES_BLOCK_WORDS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_site_class(const SiteClassArgs& a, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(site_class_kernel, dim3(site_class_blocks(a.n)), dim3(SITE_CLASS_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_site_class_compact(const SiteRecord* recs, const uint8_t* cls, uint64_t n, const uint64_t* wg_offset, SiteRecord* out_recs,
                                     uint8_t* out_cls, uint64_t out_capacity, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(site_class_compact_kernel, dim3(site_class_blocks(n)), dim3(SITE_CLASS_THREADS), 0, stream, recs, cls, n, wg_offset, out_recs, out_cls,
                     out_capacity);
  return hipGetLastError();
}

}  // namespace calitas
