// setup.hip -- the two small kernels ahead of a search: the window table of a (window size, step), and a lane's small inputs in
// one launch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>

#include "common.hpp"
#include "refpack.hpp"
#include "kernels.hpp"

namespace calitas {

// Window table of windowIterator (SearchReference.scala:39-71) for one (window size, step): out[win_base[c] + k] = N-trimmed
// 0-based half-open bounds of window k of contig c.  Rebuilt only when the tiling changes.
__global__ void window_table_kernel(const Run* runs, int64_t n_runs, const ContigInfo* contigs, const uint64_t* win_base,
                                    int n_contigs, int W, int step, int2* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= win_base[n_contigs]) return;
  int lo = 0, hi = n_contigs;              // last contig with win_base[c] <= i
  while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (win_base[mid] <= i) lo = mid; else hi = mid; }
  int64_t a = 0, b = 0;
  window_bounds(runs, n_runs, contigs[lo].gbase, contigs[lo].len, W, step, i - win_base[lo], a, b);
  out[i] = make_int2((int)a, (int)b);
}

hipError_t launch_window_table(const Run* runs, int64_t n_runs, const ContigInfo* contigs, const uint64_t* win_base, int n_contigs,
                               uint64_t n_windows, int W, int step, int2* out, hipStream_t stream) {
  if (n_windows == 0) return hipSuccess;
  hipLaunchKernelGGL(window_table_kernel, dim3((unsigned)((n_windows + 255) / 256)), dim3(256), 0, stream, runs, n_runs, contigs,
                     win_base, n_contigs, W, step, out);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void lane_setup_kernel(LaneSetupArgs a) {
  if (blockIdx.x == 0) {
    // The argument block is host memory: a load from it crosses the bus.  16 bytes per lane, all of them in flight at once -- byte by
    // byte the 700 bytes of a typical call took 15 us.
    const uint8_t* args = (const uint8_t*)__builtin_amdgcn_kernarg_segment_ptr();   // (a C-style cast: out of the constant address space)
    if (a.d_guides) {                                          // (null: the row stage's inputs only, the scan's went ahead)
      const uint32_t* g = reinterpret_cast<const uint32_t*>(args + offsetof(LaneSetupArgs, guide));
      uint32_t* dg = reinterpret_cast<uint32_t*>(a.d_guides);
      constexpr uint32_t n4 = sizeof(GuideDev) / 16, rest = (sizeof(GuideDev) % 16) / 4;
      if (threadIdx.x < n4) reinterpret_cast<uint4*>(dg)[threadIdx.x] = reinterpret_cast<const uint4*>(g)[threadIdx.x];
      else if (threadIdx.x < n4 + rest) dg[n4 * 4 + (threadIdx.x - n4)] = g[n4 * 4 + (threadIdx.x - n4)];
      if (threadIdx.x >= 64 && threadIdx.x < 72) a.d_counters[threadIdx.x - 64] = 0u;
    }
    if (a.d_row_counts && threadIdx.x >= 72 && threadIdx.x < 78) reinterpret_cast<uint32_t*>(a.d_row_counts)[threadIdx.x - 72] = 0u;
    if (a.d_blob && threadIdx.x >= 128) {
      const uint4* b = reinterpret_cast<const uint4*>(args + offsetof(LaneSetupArgs, blob));
      for (uint32_t i = threadIdx.x - 128; i < (a.blob_bytes + 15) / 16; i += 128) reinterpret_cast<uint4*>(a.d_blob)[i] = b[i];
    }
  }
  if (a.clear)
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < a.clear_bytes / 16; i += gridDim.x * 256) a.clear[i] = make_uint4(0u, 0u, 0u, 0u);
}

hipError_t launch_lane_setup(const LaneSetupArgs& a, hipStream_t stream) {
  static_assert(sizeof(GuideDev) % 4 == 0 && sizeof(GuideDev) / 16 + 4 <= 64 && sizeof(LaneSetupArgs) <= 4096 && offsetof(LaneSetupArgs, guide) % 16 == 0 &&
                offsetof(LaneSetupArgs, blob) % 16 == 0, "the lane's small inputs travel as kernel arguments, read in 16-byte pieces");
  if ((a.d_guides != nullptr) != (a.d_counters != nullptr) || a.blob_bytes > LANE_SETUP_BLOB || (a.clear_bytes & 15u)) return hipErrorInvalidValue;
  const unsigned grid = a.clear ? std::min<unsigned>(256u, std::max<unsigned>(1u, a.clear_bytes / (16u * 256u))) : 1u;
  hipLaunchKernelGGL(lane_setup_kernel, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace calitas
