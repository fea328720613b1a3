// api.cpp -- C ABI of libcalitas_hip.so (include/calitas_hip.h): context, reference upload, the search pipeline.
#include <hip/hip_runtime_api.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <ctime>
#include <numeric>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/calitas_hip.h"
#include "tuning.hpp"
#include "common.hpp"
#include "fasta.hpp"
#include "kernels.hpp"
#include "parallel.hpp"
#include "post.hpp"
#include "refpack.hpp"
#include "ctx.hpp"
#include "sites.hpp"

static std::string g_create_error;

// Output buffers (alignment arrays, hits.txt text) are tens of MB per pass; handing each one back to the OS and faulting
// a fresh one in costs milliseconds, so calitas_free parks the most recent blocks and out_alloc reuses them.
namespace {
struct BlockHeader { uint64_t magic; uint64_t capacity; uint64_t pinned; uint64_t pad; };
constexpr uint64_t kMagic = 0xCA117A5B10C0FFEEull;
std::mutex g_pool_mutex;
std::vector<BlockHeader*> g_pool;   // parked blocks
constexpr size_t kPoolBlocks = 128;    // a batch call hands out one text buffer per guide (BASELINE config 4: 96 guides)
constexpr uint64_t kPoolBytes = 24ull << 30;   // ... of ~180 MB each at hg38 size; page-locking a fresh one costs tens of milliseconds

struct Reaper {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::function<void()>> jobs;
  bool quit = false, busy = false;
  std::thread t;
  void wait_idle() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return jobs.empty() && !busy; });
  }
  void give(std::function<void()> job) {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!t.joinable()) t = std::thread([this] {
        for (;;) {
          std::function<void()> j;
          {
            std::unique_lock<std::mutex> lk2(mu);
            cv.wait(lk2, [&] { return !jobs.empty() || quit; });
            if (jobs.empty()) return;
            j = std::move(jobs.front());
            jobs.pop_front();
            busy = true;
          }
          j();
          j = nullptr;
          { std::lock_guard<std::mutex> lk2(mu); busy = false; }
          cv.notify_all();
        }
      });
      jobs.push_back(std::move(job));
    }
    cv.notify_all();
  }
  ~Reaper() {
    if (!t.joinable()) return;
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv.notify_all();
    t.join();
  }
};
Reaper g_reaper;
// Bytes of pageable blocks whose pages are still on their way back (release_block): a caller that frees a text of tens of gigabytes
// and asks for the next one at once would hold both for a moment -- on a box with a memory limit that is the OOM killer's cue --,
// so a fresh block of a gigabyte or more waits for them first (out_alloc_impl).
std::atomic<uint64_t> g_deferred_bytes{0};

void release_block_now(BlockHeader* h);
void release_block(BlockHeader* h) {
  h->magic = 0;
  if (h->pinned) { (void)hipHostFree(h); return; }
  // (a text of gigabytes: the caller's free() returns at once, the pages go back on the library's own thread -- 0.13 s per 22 GB even
  // with sixteen threads handing them back)
  if (h->capacity >= (1ull << 30) && !TUNE_GET("CALITAS_FREE_NOW")) {
    const uint64_t cap = h->capacity;
    g_deferred_bytes += cap;
    g_reaper.give([h, cap] { release_block_now(h); g_deferred_bytes -= cap; });
    return;
  }
  release_block_now(h);
}
void release_block_now(BlockHeader* h) {
  // A text of tens of gigabytes: the kernel clears pages as it takes them back (16 GB: 0.77 s inside free() on the GPU boxes, huge
  // pages or not).  MADV_DONTNEED takes the address-space lock shared, so the workers hand the pages back side by side first
  // (0.135 s, tools/thp_bench.cpp) and free() then unmaps an empty range.
  const uint64_t cap = h->capacity;
  if (cap >= (1ull << 30)) {
    const uintptr_t lo = ((uintptr_t)h + 2 * 4096) & ~(uintptr_t)4095, hi = ((uintptr_t)h + sizeof(BlockHeader) + cap) & ~(uintptr_t)4095;
    const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t per = (((hi - lo) / (size_t)T) + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
      th.emplace_back([=] { const uintptr_t a = lo + per * (size_t)t, b = std::min<uintptr_t>(hi, a + per); if (a < b) (void)madvise((void*)a, b - a, MADV_DONTNEED); });
    for (auto& x : th) x.join();
  }
  std::free(h);
}

// pinned: page-locked memory (hipHostMalloc) -- the destination of the text copy-back, so that the copy is one DMA at
// PCIe rate from the first use on instead of the runtime pinning pageable memory piecemeal.
void* out_alloc_impl(size_t size, bool pinned = false) {
  if (size < 1) size = 1;
  {
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    int best = -1;
    for (size_t i = 0; i < g_pool.size(); i++)
      if ((g_pool[i]->pinned != 0) == pinned && g_pool[i]->capacity >= size && g_pool[i]->capacity <= 2 * size + (1u << 20) &&
          (best < 0 || g_pool[i]->capacity < g_pool[best]->capacity)) best = (int)i;
    if (best >= 0) { BlockHeader* h = g_pool[best]; g_pool.erase(g_pool.begin() + best); return h + 1; }
  }
  size_t cap = size + size / 8;
  if (!pinned && size >= (1ull << 30) && g_deferred_bytes.load() != 0) g_reaper.wait_idle();   // (see g_deferred_bytes)
  if (size >= (1u << 20) && TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] out_alloc: fresh %s block of %zu bytes\n", pinned ? "pinned" : "pageable", cap);
  BlockHeader* h = nullptr;
  if (pinned) {
    if (hipHostMalloc((void**)&h, sizeof(BlockHeader) + cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h = nullptr; pinned = false; }
  }
  if (!h) h = (BlockHeader*)std::malloc(sizeof(BlockHeader) + cap);
  if (!h) return nullptr;
  h->magic = kMagic; h->capacity = cap; h->pinned = pinned ? 1 : 0; h->pad = 0;
  return h + 1;
}

// One pageable block of a gigabyte or more stays parked as well (round 5): the text of a per-contig search -- 21.8 GB for BASELINE
// config 5's shape -- is copied into its block from a bounce buffer, and into pages nobody has touched that copy is the slowest thing the
// call does (0.6 s; 0.13 s more to hand the pages back).  The next such search takes the block as it is (calitas_out_take_big): its pages
// are there.  At most one, at most kBigPark bytes; calitas_release_parked() lets go of it and of everything else that is parked.
constexpr uint64_t kBigPark = 48ull << 30;
BlockHeader* g_big = nullptr;          // (under g_pool_mutex)

void out_free(void* p) {
  if (!p) return;
  BlockHeader* h = (BlockHeader*)p - 1;
  if (h->magic != kMagic) return;     // not ours: refuse rather than corrupt the heap
  if (!h->pinned && h->capacity >= (1ull << 30) && h->capacity <= kBigPark && !TUNE_GET("CALITAS_FREE_NOW")) {
    BlockHeader* old = nullptr;
    {
      std::lock_guard<std::mutex> lk(g_pool_mutex);
      if (!g_big || g_big->capacity < h->capacity) { old = g_big; g_big = h; h = nullptr; }
    }
    if (old) release_block(old);
    if (!h) return;
  }
  // (a block of many gigabytes would only crowd the others out; small page-locked blocks are parked too: hipHostFree + hipHostMalloc
  // of the 11 KB text of an E. coli-sized call cost 0.2 ms per call, more than the search's kernels)
  if ((h->capacity >= (1u << 20) || h->pinned) && h->capacity <= kPoolBytes / 4) {
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    g_pool.push_back(h);
    uint64_t parked = 0;
    for (auto* b : g_pool) parked += b->capacity;
    if (g_pool.size() <= kPoolBlocks && parked <= kPoolBytes) return;
    size_t small = 0;                   // full: let the smallest parked block go, the big ones are the expensive ones
    for (size_t i = 1; i < g_pool.size(); i++) if (g_pool[i]->capacity < g_pool[small]->capacity) small = i;
    h = g_pool[small];
    g_pool.erase(g_pool.begin() + small);
  }
  release_block(h);
}
}  // namespace
// A pageable block of at least `size` bytes with the first `keep` bytes of p (a pageable block of this allocator, or NULL): realloc,
// so growing a multi-gigabyte text moves pages instead of copying them.
void* calitas_out_grow(void* p, size_t keep, size_t size) {
  if (!p) return out_alloc_impl(size);
  BlockHeader* h = (BlockHeader*)p - 1;
  if (h->magic != kMagic || h->pinned) return nullptr;
  if (h->capacity >= size) return p;
  (void)keep;
  const size_t cap = size + size / 4;
  BlockHeader* n = (BlockHeader*)std::realloc(h, sizeof(BlockHeader) + cap);
  if (!n) return nullptr;
  n->capacity = cap;
  if (cap >= (1ull << 30)) {   // tens of gigabytes are about to be touched for the first time: ask for huge pages (512x fewer faults)
    const uintptr_t lo = ((uintptr_t)n + 4095) & ~(uintptr_t)4095, hi = ((uintptr_t)n + sizeof(BlockHeader) + cap) & ~(uintptr_t)4095;
    if (hi > lo) (void)madvise((void*)lo, hi - lo, MADV_HUGEPAGE);
  }
  return n + 1;
}
// A block that turned out far larger than what it holds (a parked block of 22 GB taken for a text of 2) gives the rest back: p or its
// new address; the first `size` bytes stay.
void* calitas_out_shrink(void* p, size_t size) {
  if (!p) return p;
  BlockHeader* h = (BlockHeader*)p - 1;
  if (h->magic != kMagic || h->pinned || h->capacity < (1ull << 30) || h->capacity <= 2 * (uint64_t)size + (256ull << 20)) return p;
  const size_t cap = size + size / 16 + 4096;
  BlockHeader* n = (BlockHeader*)std::realloc(h, sizeof(BlockHeader) + cap);
  if (!n) return p;
  n->capacity = cap;
  return n + 1;
}
// The parked big block (above) if it has at least min_bytes of room, else NULL.  The caller owns it from here on (calitas_out_grow, calitas_free).
void* calitas_out_take_big(size_t min_bytes) {
  std::lock_guard<std::mutex> lk(g_pool_mutex);
  if (!g_big || g_big->capacity < min_bytes) return nullptr;
  BlockHeader* h = g_big;
  g_big = nullptr;
  return h + 1;
}
extern "C" void calitas_release_parked(void) {
  std::vector<BlockHeader*> all;
  {
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    all.swap(g_pool);
    if (g_big) { all.push_back(g_big); g_big = nullptr; }
  }
  for (BlockHeader* h : all) release_block(h);
}
void calitas_reap_later(std::function<void()> job) { g_reaper.give(std::move(job)); }
extern "C" void calitas_reap_wait(void) { g_reaper.wait_idle(); }
void* calitas_out_alloc(size_t size) { return out_alloc_impl(size); }
void* calitas_out_alloc_pinned(size_t size) { return out_alloc_impl(size, true); }
static void* out_alloc(size_t size) { return out_alloc_impl(size); }

int calitas_fail(calitas_ctx* ctx, int code, const std::string& msg) {
  // (a helper thread of a call may report on the same context as the caller's thread: the per-contig passes, the lanes' retries)
  static std::mutex err_mu;
  std::lock_guard<std::mutex> lk(err_mu);
  if (ctx) ctx->err = msg; else g_create_error = msg;
  return code;
}
static int fail(calitas_ctx* ctx, int code, const std::string& msg) { return calitas_fail(ctx, code, msg); }

// The device copy of the regions' tables (calitas_set_regions); the caller has made sure nothing on the device still reads them.
static void free_regions_device(calitas_ctx* c) {
  if (c->device < 0) return;
  (void)hipFree(c->d_region_seg); (void)hipFree(c->d_region_coarse); (void)hipFree(c->d_region_contig);
  c->d_region_seg = nullptr; c->d_region_coarse = nullptr; c->d_region_contig = nullptr;
}

static void free_reference_device(calitas_ctx* c) {
  if (c->device < 0) return;
  free_regions_device(c);
  (void)hipFree(c->d_codes); (void)hipFree(c->d_planes); (void)hipFree(c->d_mask); (void)hipFree(c->d_runs); (void)hipFree(c->d_contigs); (void)hipFree(c->d_tiles); (void)hipFree(c->d_tile_list); (void)hipFree(c->d_win_base); (void)hipFree(c->d_win);
  c->d_win_base = nullptr; c->d_win = nullptr; c->win_cap = 0; c->win_W = c->win_step = 0;
  (void)hipFree(c->d_bin_base); c->d_bin_base = nullptr; (void)hipFree(c->d_bin_contig); c->d_bin_contig = nullptr; c->bin_shift = 0; c->bin_base.clear(); c->bin_decl_pams = -1;
  c->d_codes = c->d_mask = nullptr; c->d_planes = nullptr; c->d_runs = nullptr; c->d_contigs = nullptr; c->d_tiles = nullptr; c->d_tile_list = nullptr;
}

extern "C" {

const char* calitas_version(void) { return "calitas-hip 0.1 (gfx950)"; }

const char* calitas_switches(void) {
  static const std::string text = [] {
    std::string t;
    for (const tune::Switch& s : tune::kSwitches) { t += s.name; t += " <"; t += s.values; t += "> "; t += s.what; t += "\n"; }
    return t;
  }();
  return text.c_str();
}

const char* calitas_last_error(const calitas_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

void calitas_free(void* p) { out_free(p); }

void* calitas_alloc_host(uint64_t bytes) { return out_alloc_impl((size_t)bytes, true); }

int calitas_create(int device_id, calitas_ctx** out) {
  if (!out) return fail(nullptr, CALITAS_EINVAL, "out is NULL");
  *out = nullptr;
  calitas_ctx* c = new calitas_ctx();
  c->device = device_id;
  c->pool = new WorkerPool(WorkerPool::default_threads());
  if (device_id >= 0) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
      delete c;
      return fail(nullptr, CALITAS_ENODEV, "no HIP device available (the product path has no CPU fallback)");
    }
    if (device_id >= n) { delete c; return fail(nullptr, CALITAS_ENODEV, "device index out of range"); }
    // non-blocking, like the lanes' streams: nothing here relies on the null stream, and an application's own default-stream work
    // (PyTorch) neither waits for a search nor holds one up
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
      std::string m = hipGetErrorString(e);
      delete c;
      return fail(nullptr, CALITAS_EHIP, "device init failed: " + m);
    }
    // [0..5] sit between kernels of one device: a device-scope release is enough (the default, release to system, made whatever
    // waited for the end of a scan wait ~90 us longer); [6..7] bracket the text copy the host waits for
    for (int i = 0; i < 8; i++) (void)hipEventCreateWithFlags(&c->ev[i], i < 6 ? hipEventReleaseToDevice : hipEventDefault);
    (void)hipMalloc((void**)&c->d_counters, 8 * sizeof(uint32_t));
    (void)hipHostMalloc((void**)&c->h_counters, 8 * sizeof(uint32_t), hipHostMallocDefault);
    (void)hipMalloc((void**)&c->d_guides, sizeof(GuideDev) * MAX_GUIDES);
    (void)hipHostMalloc((void**)&c->h_guides, sizeof(GuideDev) * MAX_GUIDES, hipHostMallocDefault);
    // The aligner kernel's wavefront relies on the DPP wave shift; verify it on this device once.
    int* d = nullptr;
    int* h = nullptr;                       // page-locked: no copy of this library lands in pageable memory
    bool ok = hipMalloc((void**)&d, 64 * sizeof(int)) == hipSuccess && hipHostMalloc((void**)&h, 64 * sizeof(int), hipHostMallocDefault) == hipSuccess &&
              launch_dpp_selftest(d, c->stream) == hipSuccess &&
              hipMemcpyAsync(h, d, 64 * sizeof(int), hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
              hipStreamSynchronize(c->stream) == hipSuccess;
    (void)hipFree(d);
    for (int i = 1; ok && i < 64; i++) ok = h[i] == (i - 1) * 7 + 3;
    if (h) (void)hipHostFree(h);
    if (!ok || !c->d_counters || !c->h_counters || !c->d_guides || !c->h_guides) {
      calitas_destroy(c);
      return fail(nullptr, CALITAS_EHIP, "device self-test failed (DPP wave_shr / allocation)");
    }
  } else if (device_id != -1) {
    delete c;
    return fail(nullptr, CALITAS_EINVAL, "device_id must be >= 0 or -1");
  }
  *out = c;
  return CALITAS_OK;
}

void calitas_destroy(calitas_ctx* c) {
  if (!c) return;
  if (c->device >= 0) {
    (void)hipSetDevice(c->device);
    free_reference_device(c);
    (void)hipFree(c->d_guides); (void)hipFree(c->d_recs); (void)hipFree(c->d_raw); (void)hipFree(c->d_counters);
    (void)hipFree(c->d_slab); (void)hipFree(c->d_items);
    calitas_destroy_lanes(c);
    if (c->side) { calitas_destroy(c->side); c->side = nullptr; }
    if (c->side2) { calitas_destroy(c->side2); c->side2 = nullptr; }
    for (void* q : c->aw.p) (void)hipFree(q);
    select_destroy(c->select);
    hits_destroy(c->hits);
    hits_destroy(c->hits_alt);
    binned_destroy(c->binned);
    sites_destroy(c->sites);
    if (c->scan_done) (void)hipEventDestroy(c->scan_done);
    if (c->rows_ready) (void)hipEventDestroy(c->rows_ready);
    if (c->inputs_ready) (void)hipEventDestroy(c->inputs_ready);
    if (c->h_counters) (void)hipHostFree(c->h_counters);
    mailbox_close(c->mbox);
    if (c->h_guides) (void)hipHostFree(c->h_guides);
    if (c->h_raw) (void)hipHostFree(c->h_raw);
    for (auto& ev : c->ev) if (ev) (void)hipEventDestroy(ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
  }
  delete c;
}

static int upload_reference_device(calitas_ctx* ctx) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // searches of the old reference may still be queued on the lanes' streams: nothing of it may be freed under them
  HIP_TRY(ctx, hipDeviceSynchronize());
  free_reference_device(ctx);
  const PackedRef& r = ctx->ref;
  size_t nruns = std::max<size_t>(1, r.runs.size());
  if (const char* e = TUNE_GET("CALITAS_DEVICE_BUDGET_MB")) {   // the budget a caller sharing the card sets covers the reference too
    const uint64_t want = (uint64_t)r.codes.size() * 8 + (uint64_t)r.mask.size() * 4 + nruns * sizeof(Run) + r.tiles.size() * sizeof(TileInfo);
    if (want > (uint64_t)std::atoll(e) << 20)
      return fail(ctx, CALITAS_ENOMEM, "the packed reference (" + std::to_string(want >> 20) + " MB on the device) exceeds CALITAS_DEVICE_BUDGET_MB");
  }
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_codes, r.codes.size() * 4));
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_planes, r.codes.size() * 4));
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_mask, r.mask.size() * 4));
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_runs, nruns * sizeof(Run)));
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_contigs, r.contigs.size() * sizeof(ContigInfo)));
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_tiles, r.tiles.size() * sizeof(TileInfo)));
  HIP_TRY(ctx, hipMemcpy(ctx->d_codes, r.codes.data(), r.codes.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->d_mask, r.mask.data(), r.mask.size() * 4, hipMemcpyHostToDevice));
  if (!r.runs.empty()) HIP_TRY(ctx, hipMemcpy(ctx->d_runs, r.runs.data(), r.runs.size() * sizeof(Run), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->d_contigs, r.contigs.data(), r.contigs.size() * sizeof(ContigInfo), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->d_tiles, r.tiles.data(), r.tiles.size() * sizeof(TileInfo), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMalloc((void**)&ctx->d_tile_list, std::max<size_t>(1, r.masked_tiles.size()) * sizeof(uint32_t)));
  if (!r.masked_tiles.empty())
    HIP_TRY(ctx, hipMemcpy(ctx->d_tile_list, r.masked_tiles.data(), r.masked_tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  // the scan streams the codes as two bit-planes per 32 bases (scan_rows.hip); derived on the device, once per reference
  HIP_TRY(ctx, launch_planes(ctx->d_codes, ctx->d_planes, r.total_packed / 32, ctx->stream));
  HIP_TRY(ctx, hipDeviceSynchronize());   // the searches run on non-blocking streams, which nothing orders against these copies
  return CALITAS_OK;
}

// ctx->ref holds a freshly packed reference.  has_ref becomes true only when the device copy is complete: a failed upload
// (CALITAS_ENOMEM for a genome that does not fit) leaves a context that answers CALITAS_ESTATE, not one whose next search
// launches kernels on freed pointers.
static int upload_reference(calitas_ctx* ctx) {
  ctx->ref_serial++;
  ctx->seq_pams = -1; ctx->fit_pams = -1;   // what did (not) fit the old reference may (not) fit this one
  ctx->has_ref = false;
  ctx->regions.clear();                     // (the intervals were given in the old reference's coordinates; free_reference_device drops their device copy)
  if (ctx->device >= 0) {
    const int rc = upload_reference_device(ctx);
    if (rc) {
      (void)hipDeviceSynchronize();
      free_reference_device(ctx);
      ctx->ref = PackedRef();
      return rc;
    }
  }
  ctx->has_ref = true;
  return CALITAS_OK;
}

int calitas_set_regions(calitas_ctx* ctx, uint64_t n, const calitas_region_t* iv, uint32_t n_classes) {
  if (!ctx) return CALITAS_EINVAL;
  if (!ctx->has_ref) return fail(ctx, CALITAS_ESTATE, "calitas_set_reference has not been called");
  std::vector<uint64_t> lens(ctx->ref.contigs.size());
  for (size_t c = 0; c < lens.size(); c++) lens[c] = ctx->ref.contigs[c].len;
  RegionsHost flat;
  const std::string e = regions_flatten(lens, [&](size_t c) { return ctx->ref.is_absent(c); }, iv, n, n_classes, flat);
  if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e);
  if (ctx->device >= 0) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());   // (nothing of the old set may be freed under a kernel that reads it)
    free_regions_device(ctx);
  }
  ctx->regions.clear();
  if (flat.empty()) return CALITAS_OK;
  if (ctx->device >= 0) {
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_region_seg, flat.seg.size() * sizeof(RegionSeg)));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_region_coarse, flat.coarse.size() * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_region_contig, flat.contig.size() * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_region_seg, flat.seg.data(), flat.seg.size() * sizeof(RegionSeg), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_region_coarse, flat.coarse.data(), flat.coarse.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_region_contig, flat.contig.data(), flat.contig.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipDeviceSynchronize());   // the searches run on non-blocking streams, which nothing orders against these copies
  }
  ctx->regions = std::move(flat);
  return CALITAS_OK;
}

int calitas_region_class(const calitas_ctx* ctx, int32_t contig_index, int64_t start, int64_t end) {
  if (!ctx || !ctx->has_ref || ctx->regions.empty() || contig_index < 0 || (size_t)contig_index >= ctx->ref.contigs.size()) return -1;
  return (int)region_class(ctx->regions.view(), (uint32_t)contig_index, start, end, ctx->ref.contigs[(size_t)contig_index].len);
}

int calitas_set_reference(calitas_ctx* ctx, int32_t n_contigs, const char* const* names, const uint64_t* lengths,
                          const uint8_t* const* bases, const char* genome_build) {
  if (!ctx) return CALITAS_EINVAL;
  if (n_contigs <= 0 || !names || !lengths || !bases) return fail(ctx, CALITAS_EINVAL, "bad contig arguments");
  for (int i = 0; i < n_contigs; i++)
    if (lengths[i] > 0x7FFFFFFFull) return fail(ctx, CALITAS_EINVAL, "contigs longer than 2^31-1 bases are not supported (the reference uses Int coordinates)");
  try {
    pack_reference(ctx->ref, n_contigs, names, lengths, bases, genome_build, 0);
  } catch (std::exception& e) {
    ctx->has_ref = false;
    return fail(ctx, CALITAS_EINVAL, e.what());
  }
  return upload_reference(ctx);
}

int calitas_set_reference_fasta(calitas_ctx* ctx, const char* fasta_path) {
  if (!ctx || !fasta_path) return CALITAS_EINVAL;
  FastaData fd;
  std::string e = read_fasta(fasta_path, fd);
  if (!e.empty()) return fail(ctx, CALITAS_EIO, e);
  std::vector<const char*> names;
  std::vector<uint64_t> lens;
  std::vector<const uint8_t*> bases;
  for (size_t i = 0; i < fd.names.size(); i++) {
    names.push_back(fd.names[i].c_str());
    lens.push_back(fd.seqs[i].size());
    bases.push_back(reinterpret_cast<const uint8_t*>(fd.seqs[i].data()));
  }
  return calitas_set_reference(ctx, (int32_t)names.size(), names.data(), lens.data(), bases.data(), fd.genome_build.c_str());
}


// ---- persistent packed index: skips re-packing 3 GB of ASCII on repeated runs ----
}  // extern "C"
namespace {
struct IndexHeader {
  char magic[8];            // "CALIDX02"
  uint32_t chunk, n_contigs;
  uint64_t tile, total_packed, total_bases, n_runs, n_tiles, n_masked, build_len, names_len;
  uint64_t layout;          // kIndexLayout: a file written by a build with another packed layout is refused, not misread
  uint64_t checksum;        // index_checksum() over contigs, codes, mask, runs, tiles, masked_tiles
};
constexpr uint64_t kIndexLayout = 2 | ((uint64_t)LANES_PER_TILE << 8) | ((uint64_t)sizeof(Run) << 24) | ((uint64_t)sizeof(TileInfo) << 32) | ((uint64_t)sizeof(ContigInfo) << 40);

// 64-bit multiply-xor hash over 8-byte words in four independent lanes (memory-bound; the arrays are 4-byte aligned and a multiple of 4 bytes long)
uint64_t hash_bytes(const void* p, size_t n, uint64_t seed) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h[4] = {seed ^ 0x9E3779B97F4A7C15ull, seed ^ 0xC2B2AE3D27D4EB4Full, seed ^ 0x165667B19E3779F9ull, seed ^ 0x27D4EB2F165667C5ull};
  size_t i = 0;
  for (; i + 32 <= n; i += 32) {
    uint64_t w[4];
    std::memcpy(w, b + i, 32);
    for (int k = 0; k < 4; k++) { h[k] = (h[k] ^ w[k]) * 0x9FB21C651E98DF25ull; h[k] ^= h[k] >> 29; }
  }
  uint64_t tail = 0x1234567ull + n;
  for (; i < n; i++) tail = (tail ^ b[i]) * 0x100000001B3ull;
  uint64_t r = tail;
  for (int k = 0; k < 4; k++) { r = (r ^ h[k]) * 0xFF51AFD7ED558CCDull; r ^= r >> 32; }
  return r;
}
uint64_t index_checksum(const PackedRef& r) {
  uint64_t c = hash_bytes(r.contigs.data(), r.contigs.size() * sizeof(ContigInfo), 1);
  c = hash_bytes(r.codes.data(), r.codes.size() * 4, c);
  c = hash_bytes(r.mask.data(), r.mask.size() * 4, c);
  c = hash_bytes(r.runs.data(), r.runs.size() * sizeof(Run), c);
  c = hash_bytes(r.tiles.data(), r.tiles.size() * sizeof(TileInfo), c);
  return hash_bytes(r.masked_tiles.data(), r.masked_tiles.size() * 4, c);
}

// Everything the kernels index with goes to the device unchecked, so a loaded index is checked here: "" or what is wrong.
std::string validate_index(const PackedRef& r) {
  if (!(r.chunk == 64 || r.chunk == 128 || r.chunk == 256 || r.chunk == 512) || r.tile != (uint64_t)r.chunk * LANES_PER_TILE) return "tile geometry";
  const uint64_t T = r.tile, n_tiles = r.total_packed / T;
  if (r.contigs.empty() || r.total_packed / 16 > 0xFFFFFFFFull || n_tiles < 3) return "size";
  if (r.codes.size() != r.total_packed / 16 || r.mask.size() != r.total_packed / 32 || r.tiles.size() != n_tiles) return "array sizes";
  uint64_t next = T, sum = 0;            // tile 0 is padding
  std::vector<uint32_t> owner(n_tiles, 0xFFFFFFFFu);
  for (size_t c = 0; c < r.contigs.size(); c++) {
    const ContigInfo& ci = r.contigs[c];
    if (ci.gbase % T != 0 || ci.gbase < next || ci.len > 0x7FFFFFFFull) return "contig placement";
    uint64_t nt = (ci.len + (uint64_t)r.chunk + T - 1) / T;   // the contig and >= one chunk of padding
    if (nt == 0) nt = 1;
    if (ci.gbase / T + nt + 1 > n_tiles) return "contig beyond the packed space";
    for (uint64_t t = 0; t < nt; t++) owner[ci.gbase / T + t] = (uint32_t)c;
    next = ci.gbase + nt * T;
    sum += ci.len;
  }
  if (sum != r.total_bases) return "total_bases";
  for (uint64_t t = 0; t < n_tiles; t++)
    if (r.tiles[t].contig != owner[t] || r.tiles[t].flag > 2u) return "tile table";
  uint64_t prev_end = 0;
  for (const Run& u : r.runs) {
    if (u.len == 0 || u.start < prev_end || u.start + u.len > r.total_packed) return "run table";
    prev_end = u.start + u.len;
  }
  uint64_t prev_tile = 0;
  for (size_t i = 0; i < r.masked_tiles.size(); i++) {
    const uint32_t t = r.masked_tiles[i];
    if (t >= n_tiles || (i && t <= prev_tile) || r.tiles[t].flag != 1u) return "masked tile list";
    prev_tile = t;
  }
  return "";
}
template <typename T> bool wr(FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }
template <typename T> bool rd(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
}  // namespace
extern "C" {

int calitas_save_index(const calitas_ctx* ctx, const char* path) {
  if (!ctx || !path) return CALITAS_EINVAL;
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  if (!ctx->has_ref) return fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  const PackedRef& r = ctx->ref;
  if (!r.absent.empty()) return fail(c, CALITAS_EINVAL, "a reference with absent contigs (one process's share of a multi-GPU job) is not saved as an index");
  std::string names;
  for (auto& n : r.names) { names += n; names += '\n'; }
  IndexHeader h{};
  std::memcpy(h.magic, "CALIDX02", 8);
  h.layout = kIndexLayout; h.checksum = index_checksum(r);
  h.chunk = (uint32_t)r.chunk; h.n_contigs = (uint32_t)r.contigs.size(); h.tile = r.tile; h.total_packed = r.total_packed;
  h.total_bases = r.total_bases; h.n_runs = r.runs.size(); h.n_tiles = r.tiles.size(); h.n_masked = r.masked_tiles.size();
  h.build_len = r.genome_build.size(); h.names_len = names.size();
  FILE* f = std::fopen(path, "wb");
  if (!f) return fail(c, CALITAS_EIO, std::string("cannot write ") + path);
  bool ok = wr(f, &h, 1) && wr(f, r.genome_build.data(), r.genome_build.size()) && wr(f, names.data(), names.size()) &&
            wr(f, r.contigs.data(), r.contigs.size()) && wr(f, r.codes.data(), r.codes.size()) && wr(f, r.mask.data(), r.mask.size()) &&
            wr(f, r.runs.data(), r.runs.size()) && wr(f, r.tiles.data(), r.tiles.size()) && wr(f, r.masked_tiles.data(), r.masked_tiles.size());
  ok = (std::fclose(f) == 0) && ok;
  return ok ? CALITAS_OK : fail(c, CALITAS_EIO, std::string("short write to ") + path);
}

int calitas_load_index(calitas_ctx* ctx, const char* path) {
  if (!ctx || !path) return CALITAS_EINVAL;
  FILE* f = std::fopen(path, "rb");
  if (!f) return fail(ctx, CALITAS_EIO, std::string("cannot read ") + path);
  IndexHeader h{};
  PackedRef r;
  std::string names;
  bool ok = rd(f, &h, 1) && std::memcmp(h.magic, "CALIDX02", 8) == 0 && h.layout == kIndexLayout && h.tile == (uint64_t)h.chunk * LANES_PER_TILE &&
            h.total_packed % std::max<uint64_t>(1, h.tile) == 0 && h.n_tiles == h.total_packed / std::max<uint64_t>(1, h.tile) &&
            h.build_len < (1u << 16) && h.names_len < (1ull << 32);
  if (ok) {   // the counts size the allocations below: they must add up to the file's own length
    const uint64_t want = sizeof(IndexHeader) + h.build_len + h.names_len + (uint64_t)h.n_contigs * sizeof(ContigInfo) + h.total_packed / 16 * 4 +
                          h.total_packed / 32 * 4 + h.n_runs * sizeof(Run) + h.n_tiles * sizeof(TileInfo) + h.n_masked * 4;
    ok = h.n_runs < (1ull << 40) && h.n_masked <= h.n_tiles && std::fseek(f, 0, SEEK_END) == 0 && (uint64_t)std::ftell(f) == want &&
         std::fseek(f, (long)sizeof(IndexHeader), SEEK_SET) == 0;
  }
  if (ok) {
    r.chunk = (int)h.chunk; r.tile = h.tile; r.total_packed = h.total_packed; r.total_bases = h.total_bases;
    r.genome_build.resize(h.build_len); names.resize(h.names_len);
    r.contigs.resize(h.n_contigs); r.codes.resize(h.total_packed / 16); r.mask.resize(h.total_packed / 32);
    r.runs.resize(h.n_runs); r.tiles.resize(h.n_tiles); r.masked_tiles.resize(h.n_masked);
    ok = rd(f, &r.genome_build[0], h.build_len) && rd(f, &names[0], h.names_len) && rd(f, r.contigs.data(), r.contigs.size()) &&
         rd(f, r.codes.data(), r.codes.size()) && rd(f, r.mask.data(), r.mask.size()) && rd(f, r.runs.data(), r.runs.size()) &&
         rd(f, r.tiles.data(), r.tiles.size()) && rd(f, r.masked_tiles.data(), r.masked_tiles.size());
  }
  std::fclose(f);
  if (ok) {
    size_t a = 0;
    while (a < names.size()) { size_t b = names.find('\n', a); if (b == std::string::npos) break; r.names.push_back(names.substr(a, b - a)); a = b + 1; }
    ok = r.names.size() == r.contigs.size();
  }
  if (ok && index_checksum(r) != h.checksum) return fail(ctx, CALITAS_EIO, std::string("calitas index fails its checksum: ") + path);
  if (!ok) return fail(ctx, CALITAS_EIO, std::string("not a calitas index (or truncated): ") + path);
  const std::string bad = validate_index(r);
  if (!bad.empty()) return fail(ctx, CALITAS_EIO, std::string("corrupt calitas index (") + bad + "): " + path);
  ctx->ref = std::move(r);
  return upload_reference(ctx);
}

int calitas_reference_info(const calitas_ctx* ctx, int32_t* n_contigs, uint64_t* total_bases, uint64_t* packed_bytes) {
  if (!ctx || !ctx->has_ref) return CALITAS_ESTATE;
  if (n_contigs) *n_contigs = (int32_t)ctx->ref.contigs.size();
  if (total_bases) *total_bases = ctx->ref.total_bases;
  if (packed_bytes) {                                          // 2 bits per base of the contigs that are resident here (all of them, usually)
    uint64_t bases = 0;
    for (size_t i = 0; i < ctx->ref.contigs.size(); i++) if (!ctx->ref.is_absent(i)) bases += ctx->ref.contigs[i].len;
    *packed_bytes = (bases + 3) / 4;
  }
  return CALITAS_OK;
}

const char* calitas_genome_build(const calitas_ctx* ctx) { return (ctx && ctx->has_ref) ? ctx->ref.genome_build.c_str() : ""; }

int calitas_contig_name(const calitas_ctx* ctx, int32_t i, const char** name, uint64_t* length) {
  if (!ctx || !ctx->has_ref || i < 0 || i >= (int32_t)ctx->ref.contigs.size()) return CALITAS_EINVAL;
  if (name) *name = ctx->ref.names[i].c_str();
  if (length) *length = ctx->ref.contigs[i].len;
  return CALITAS_OK;
}

int calitas_expand_rows(calitas_ctx* ctx, const char* compact, uint64_t n, uint64_t rows, const char* head, const char* tail, char* out,
                        uint64_t out_capacity, uint64_t* written) {
  if (!ctx) return CALITAS_EINVAL;
  if ((!compact && n) || !head || !tail || !out || !written) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  const std::string h(head), t(tail);
  if (t.empty() || t.back() != '\n') return fail(ctx, CALITAS_EINVAL, "the tail of a row ends with a newline");
  if (out_capacity < n + rows * (uint64_t)(h.size() + t.size() - 1)) return fail(ctx, CALITAS_EINVAL, "out is too small");
  const size_t w = expand_rows(compact, (size_t)n, rows, h, t, out, ctx->pool);
  if (w == (size_t)-1) return fail(ctx, CALITAS_EINVAL, "the compact text does not hold exactly the given number of newline-terminated rows");
  *written = w;
  return CALITAS_OK;
}

int calitas_fetch_bases(const calitas_ctx* ctx, int32_t i, uint64_t start, uint32_t len, char* out) {
  if (!ctx || !ctx->has_ref || i < 0 || i >= (int32_t)ctx->ref.contigs.size() || !out) return CALITAS_EINVAL;
  const ContigInfo& c = ctx->ref.contigs[i];
  if (start + len > c.len) return CALITAS_EINVAL;
  for (uint32_t k = 0; k < len; k++) out[k] = ctx->ref.base_upper(c.gbase + start + k);
  return CALITAS_OK;
}

int calitas_window_table(const calitas_ctx* ctx, int32_t window_size, int32_t step, int32_t min_length, int32_t chrom_index,
                         int32_t** out, uint64_t* n_windows) {
  if (!ctx || !ctx->has_ref || !out || !n_windows || step <= 0 || window_size <= 0) return CALITAS_EINVAL;
  const PackedRef& r = ctx->ref;
  std::vector<int32_t> rows;
  for (size_t c = 0; c < r.contigs.size(); c++) {
    if (chrom_index >= 0 && (int)c != chrom_index) continue;
    uint64_t nw = window_count(r.contigs[c].len, step);
    for (uint64_t k = 0; k < nw; k++) {
      int64_t a, b;
      if (!window_bounds(r.runs.data(), (int64_t)r.runs.size(), r.contigs[c].gbase, r.contigs[c].len, window_size, step, k, a, b)) continue;
      if (b - a < min_length) continue;
      rows.push_back((int32_t)c); rows.push_back((int32_t)a); rows.push_back((int32_t)b);
    }
  }
  *n_windows = rows.size() / 3;
  *out = (int32_t*)out_alloc(std::max<size_t>(1, rows.size()) * sizeof(int32_t));
  if (!rows.empty()) std::memcpy(*out, rows.data(), rows.size() * sizeof(int32_t));
  return CALITAS_OK;
}

}  // extern "C"

extern "C" {

int calitas_search(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                   calitas_aln_t** out, uint64_t* n_out) {
  return calitas_search_impl(ctx, n_guides, guides, params, out, n_out);
}

int calitas_search_hits(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                        const char* aligner_version, const char* time_stamp, char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !tsv) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  return calitas_search_hits_impl(ctx, guide, guide_id ? guide_id : "", params, aligner_version, time_stamp, tsv, tsv_bytes, n_rows);
}

int calitas_search_hits_into(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                             const char* aligner_version, const char* time_stamp, char* dst, uint64_t dst_capacity, uint64_t* tsv_bytes,
                             uint64_t* n_rows) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !dst) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  if (tsv_bytes) *tsv_bytes = 0;
  if (n_rows) *n_rows = 0;
  return calitas_search_hits_into_impl(ctx, guide, guide_id ? guide_id : "", params, aligner_version, time_stamp, dst, dst_capacity, tsv_bytes, n_rows);
}

int calitas_pin_host(calitas_ctx* ctx, void* p, uint64_t bytes) {
  if (!ctx || !p || !bytes) return CALITAS_EINVAL;
  if (ctx->device < 0) return fail(ctx, CALITAS_ENODEV, "host-only context");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault));
  return CALITAS_OK;
}

int calitas_unpin_host(calitas_ctx* ctx, void* p) {
  if (!ctx || !p) return CALITAS_EINVAL;
  HIP_TRY(ctx, hipHostUnregister(p));
  return CALITAS_OK;
}

int calitas_search_hits_stream(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                               const char* aligner_version, const char* time_stamp, calitas_text_sink_t sink, void* user,
                               uint64_t* tsv_bytes, uint64_t* n_rows) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !sink) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  if (tsv_bytes) *tsv_bytes = 0;
  if (n_rows) *n_rows = 0;
  if (params->first_window != 0 || params->n_windows != 0)
    return fail(ctx, CALITAS_EINVAL, "a window range (first_window / n_windows) is for calitas_search, calitas_search_hits(_into) and calitas_search_hits_batch");
  return calitas_search_hits_stream_impl(ctx, guide, guide_id ? guide_id : "", params, aligner_version, time_stamp, sink, user, tsv_bytes, n_rows);
}

int calitas_search_hits_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const char* const* guide_ids,
                              const calitas_params_t* params, const char* aligner_version, const char* time_stamp, char** tsv,
                              uint64_t* tsv_bytes, uint64_t* n_rows) {
  if (!ctx) return CALITAS_EINVAL;
  if (n_guides <= 0 || !guides || !params || !tsv) return fail(ctx, CALITAS_EINVAL, "bad argument");
  return calitas_search_hits_batch_impl(ctx, n_guides, guides, guide_ids, params, aligner_version, time_stamp, tsv, tsv_bytes, n_rows);
}

// A table as the ABI hands it over: struct and cells in one block of the library's.
static calitas_counts_t* counts_block(const CountsShape& shape, const uint64_t* table, uint64_t rows) {
  const size_t cells = shape.cells();
  calitas_counts_t* c = (calitas_counts_t*)out_alloc(sizeof(calitas_counts_t) + cells * sizeof(uint64_t));
  if (!c) return nullptr;
  c->n_mm = shape.n_mm; c->n_gaps = shape.n_gaps; c->n_pam = shape.n_pam; c->rows = rows;
  c->counts = reinterpret_cast<uint64_t*>(c + 1);
  std::memcpy(c->counts, table, cells * sizeof(uint64_t));
  return c;
}

int calitas_search_counts(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, calitas_counts_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !out) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *out = nullptr;
  CountsShape shape;
  std::vector<uint64_t> table;
  uint64_t rows = 0;
  const int rc = calitas_search_counts_impl(ctx, guide, params, &shape, &table, &rows);
  if (rc) return rc;
  *out = counts_block(shape, table.data(), rows);
  return *out ? CALITAS_OK : fail(ctx, CALITAS_EINVAL, "out of memory");
}

int calitas_search_counts_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                calitas_counts_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (n_guides <= 0 || !guides || !params || !out) return fail(ctx, CALITAS_EINVAL, "bad argument");
  for (int i = 0; i < n_guides; i++) out[i] = nullptr;
  std::vector<std::vector<uint64_t>> tables((size_t)n_guides);
  std::vector<uint64_t> rows((size_t)n_guides, 0);
  int rc = calitas_search_hits_batch_impl(ctx, n_guides, guides, nullptr, params, nullptr, nullptr, nullptr, nullptr, rows.data(), &tables);
  for (int i = 0; i < n_guides && !rc; i++) {
    GuideHost gh;
    CountsShape shape;
    std::string e = make_guide_host(guides[i], gh);
    if (e.empty()) e = counts_shape(gh, *params, shape);
    if (!e.empty() || tables[(size_t)i].size() != shape.cells()) rc = fail(ctx, CALITAS_EINVAL, e.empty() ? "a guide's table has another shape than its plan (internal error)" : e);
    else if (!(out[i] = counts_block(shape, tables[(size_t)i].data(), rows[(size_t)i]))) rc = fail(ctx, CALITAS_EINVAL, "out of memory");
  }
  if (rc) for (int i = 0; i < n_guides; i++) { calitas_free(out[i]); out[i] = nullptr; }
  return rc;
}

// Guide sites (sites_host.cpp; the copies and near calls below: sites_copies.cpp): no reference counterpart.  The unfiltered calls are the filtered ones without a filter.
int calitas_find_sites_filtered(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index,
                                uint64_t start, uint64_t end, calitas_site_t** sites, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) *sites = nullptr;
  return calitas_find_sites_impl(ctx, pattern, filter, chrom_index, start, end, sites != nullptr, sites, nullptr, n_sites);
}

int calitas_count_sites_filtered(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, int32_t chrom_index,
                                 uint64_t start, uint64_t end, uint64_t* per_contig_strand, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  return calitas_find_sites_impl(ctx, pattern, filter, chrom_index, start, end, false, nullptr, per_contig_strand, n_sites);
}

int calitas_find_sites_filtered_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                     int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) *sites = nullptr;
  return calitas_find_sites_host_impl(ctx, pattern, filter, chrom_index, start, end, sites, n_sites);
}

int calitas_find_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t chrom_index, uint64_t start, uint64_t end,
                       calitas_site_t** sites, uint64_t* n_sites) {
  return calitas_find_sites_filtered(ctx, pattern, nullptr, chrom_index, start, end, sites, n_sites);
}

int calitas_count_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t chrom_index, uint64_t start, uint64_t end,
                        uint64_t* per_contig_strand, uint64_t* n_sites) {
  return calitas_count_sites_filtered(ctx, pattern, nullptr, chrom_index, start, end, per_contig_strand, n_sites);
}

int calitas_find_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t chrom_index, uint64_t start, uint64_t end,
                            calitas_site_t** sites, uint64_t* n_sites) {
  return calitas_find_sites_filtered_host(ctx, pattern, nullptr, chrom_index, start, end, sites, n_sites);
}

int calitas_count_copies(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start, uint64_t end,
                         const char* queries, uint64_t n_queries, uint64_t* copies) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || (n_queries && (!queries || !copies))) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  return calitas_count_copies_impl(ctx, pattern, key_length, chrom_index, start, end, queries, n_queries, copies);
}

int calitas_count_copies_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start,
                              uint64_t end, const char* queries, uint64_t n_queries, uint64_t* copies) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || (n_queries && (!queries || !copies))) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  return calitas_count_copies_host_impl(ctx, pattern, key_length, chrom_index, start, end, queries, n_queries, copies);
}

int calitas_count_near(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index, uint64_t start,
                       uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || (n_queries && (!queries || !near))) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  return calitas_count_near_impl(ctx, pattern, key_length, max_mismatches, chrom_index, start, end, queries, n_queries, near);
}

int calitas_count_near_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index,
                            uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || (n_queries && (!queries || !near))) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  return calitas_count_near_host_impl(ctx, pattern, key_length, max_mismatches, chrom_index, start, end, queries, n_queries, near);
}

// (the model is the implementation's to check: it comes after everything calitas_count_near refuses)
int calitas_score_near(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                       uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near, calitas_near_score_t* scores) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || (n_queries && (!queries || !near || !scores))) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  return calitas_score_near_impl(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, near, scores);
}

int calitas_score_near_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                            int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near,
                            calitas_near_score_t* scores) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || (n_queries && (!queries || !near || !scores))) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  return calitas_score_near_host_impl(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, near, scores);
}

int calitas_list_near(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                      uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near, uint64_t* offsets,
                      calitas_near_hit_t** hits, uint64_t* n_hits) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !offsets || !hits || !n_hits || (n_queries && (!queries || !near))) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *hits = nullptr; *n_hits = 0;
  return calitas_list_near_impl(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, limit, near, offsets, hits, n_hits);
}

int calitas_list_near_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                           int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near,
                           uint64_t* offsets, calitas_near_hit_t** hits, uint64_t* n_hits) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !offsets || !hits || !n_hits || (n_queries && (!queries || !near))) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *hits = nullptr; *n_hits = 0;
  return calitas_list_near_host_impl(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, limit, near, offsets, hits, n_hits);
}

// A guide's scores as the ABI hands them over: struct, table and cells in one block of the library's.
static calitas_scores_t* scores_block(const CountsShape& shape, const uint64_t* table, uint64_t rows, const ScoreWords& w) {
  const size_t cells = shape.cells();
  calitas_scores_t* c = (calitas_scores_t*)out_alloc(sizeof(calitas_scores_t) + cells * sizeof(uint64_t));
  if (!c) return nullptr;
  c->rows = rows; c->perfect = w.perfect; c->sum_q32 = w.sum_q32; c->max_q32 = w.max_q32;
  c->table.n_mm = shape.n_mm; c->table.n_gaps = shape.n_gaps; c->table.n_pam = shape.n_pam; c->table.rows = rows;
  c->table.counts = reinterpret_cast<uint64_t*>(c + 1);
  std::memcpy(c->table.counts, table, cells * sizeof(uint64_t));
  return c;
}

// The guide and the model of a score call, validated against each other; "" or the reason for CALITAS_EINVAL.
static std::string score_inputs(const calitas_guide_t& guide, const calitas_score_model_t* model, GuideHost& gh, ScoreModelHost& mh) {
  std::string e = make_guide_host(guide, gh);
  if (e.empty()) e = make_score_model(model, (int)gh.protospacer.size(), mh);
  return e;
}

int calitas_search_scores(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                          calitas_scores_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !model || !out) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *out = nullptr;
  GuideHost gh;
  ScoreModelHost mh;
  const std::string e = score_inputs(*guide, model, gh, mh);
  if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e);
  CountsShape shape;
  std::vector<uint64_t> table;
  uint64_t rows = 0;
  ScoreWords w;
  const int rc = calitas_search_counts_impl(ctx, guide, params, &shape, &table, &rows, &mh, &w);
  if (rc) return rc;
  *out = scores_block(shape, table.data(), rows, w);
  return *out ? CALITAS_OK : fail(ctx, CALITAS_EINVAL, "out of memory");
}

int calitas_search_scores_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                const calitas_score_model_t* model, calitas_scores_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (n_guides <= 0 || !guides || !params || !model || !out) return fail(ctx, CALITAS_EINVAL, "bad argument");
  for (int i = 0; i < n_guides; i++) out[i] = nullptr;
  ScoreModelHost mh;
  for (int i = 0; i < n_guides; i++) {                        // (all guides of a batch have one length: one model serves them)
    GuideHost gh;
    const std::string e = score_inputs(guides[i], model, gh, mh);
    if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e);
  }
  std::vector<std::vector<uint64_t>> tables((size_t)n_guides);
  std::vector<uint64_t> rows((size_t)n_guides, 0);
  std::vector<ScoreWords> words((size_t)n_guides);
  int rc = calitas_search_hits_batch_impl(ctx, n_guides, guides, nullptr, params, nullptr, nullptr, nullptr, nullptr, rows.data(), &tables, &mh, &words);
  for (int i = 0; i < n_guides && !rc; i++) {
    GuideHost gh;
    CountsShape shape;
    std::string e = make_guide_host(guides[i], gh);
    if (e.empty()) e = counts_shape(gh, *params, shape);
    if (!e.empty() || tables[(size_t)i].size() != shape.cells()) rc = fail(ctx, CALITAS_EINVAL, e.empty() ? "a guide's table has another shape than its plan (internal error)" : e);
    else if (!(out[i] = scores_block(shape, tables[(size_t)i].data(), rows[(size_t)i], words[(size_t)i]))) rc = fail(ctx, CALITAS_EINVAL, "out of memory");
  }
  if (rc) for (int i = 0; i < n_guides; i++) { calitas_free(out[i]); out[i] = nullptr; }
  return rc;
}

// A guide's top list as the ABI hands it over: struct, table cells and records in one block of the library's.
static calitas_top_t* top_block(const CountsShape& shape, const uint64_t* table, uint64_t rows, const ScoreWords& w, uint32_t k) {
  const size_t cells = shape.cells(), n = std::min<size_t>(w.top.hits.size(), k);
  calitas_top_t* t = (calitas_top_t*)out_alloc(sizeof(calitas_top_t) + cells * sizeof(uint64_t) + n * sizeof(calitas_top_hit_t));
  if (!t) return nullptr;
  calitas_scores_t* c = &t->scores;
  c->rows = rows; c->perfect = w.perfect; c->sum_q32 = w.sum_q32; c->max_q32 = w.max_q32;
  c->table.n_mm = shape.n_mm; c->table.n_gaps = shape.n_gaps; c->table.n_pam = shape.n_pam; c->table.rows = rows;
  c->table.counts = reinterpret_cast<uint64_t*>(t + 1);
  std::memcpy(c->table.counts, table, cells * sizeof(uint64_t));
  t->k = k; t->n = (uint32_t)n;
  t->hits = reinterpret_cast<calitas_top_hit_t*>(c->table.counts + cells);
  if (n) std::memcpy(t->hits, w.top.hits.data(), n * sizeof(calitas_top_hit_t));
  return t;
}
static const char* const kBadTopK = "k of a top call must be 1 .. CALITAS_TOP_MAX (256)";

int calitas_search_top(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                       uint32_t k, calitas_top_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !model || !out) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *out = nullptr;
  if (k == 0 || k > CALITAS_TOP_MAX) return fail(ctx, CALITAS_EINVAL, kBadTopK);
  GuideHost gh;
  ScoreModelHost mh;
  const std::string e = score_inputs(*guide, model, gh, mh);
  if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e);
  mh.top_k = k;
  CountsShape shape;
  std::vector<uint64_t> table;
  uint64_t rows = 0;
  ScoreWords w;
  const int rc = calitas_search_counts_impl(ctx, guide, params, &shape, &table, &rows, &mh, &w);
  if (rc) return rc;
  if (w.top.hits.size() != std::min<uint64_t>(k, rows - w.perfect)) return fail(ctx, CALITAS_EHIP, "the list of a top call does not have min(k, imperfect rows) records (internal error)");
  *out = top_block(shape, table.data(), rows, w, k);
  return *out ? CALITAS_OK : fail(ctx, CALITAS_EINVAL, "out of memory");
}

int calitas_search_top_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                             const calitas_score_model_t* model, uint32_t k, calitas_top_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (n_guides <= 0 || !guides || !params || !model || !out) return fail(ctx, CALITAS_EINVAL, "bad argument");
  for (int i = 0; i < n_guides; i++) out[i] = nullptr;
  if (k == 0 || k > CALITAS_TOP_MAX) return fail(ctx, CALITAS_EINVAL, kBadTopK);
  ScoreModelHost mh;
  for (int i = 0; i < n_guides; i++) {                        // (all guides of a batch have one length: one model serves them)
    GuideHost gh;
    const std::string e = score_inputs(guides[i], model, gh, mh);
    if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e);
  }
  mh.top_k = k;
  std::vector<std::vector<uint64_t>> tables((size_t)n_guides);
  std::vector<uint64_t> rows((size_t)n_guides, 0);
  std::vector<ScoreWords> words((size_t)n_guides);
  int rc = calitas_search_hits_batch_impl(ctx, n_guides, guides, nullptr, params, nullptr, nullptr, nullptr, nullptr, rows.data(), &tables, &mh, &words);
  for (int i = 0; i < n_guides && !rc; i++) {
    GuideHost gh;
    CountsShape shape;
    const ScoreWords& w = words[(size_t)i];
    std::string e = make_guide_host(guides[i], gh);
    if (e.empty()) e = counts_shape(gh, *params, shape);
    if (!e.empty() || tables[(size_t)i].size() != shape.cells()) rc = fail(ctx, CALITAS_EINVAL, e.empty() ? "a guide's table has another shape than its plan (internal error)" : e);
    else if (w.top.hits.size() != std::min<uint64_t>(k, rows[(size_t)i] - w.perfect)) rc = fail(ctx, CALITAS_EHIP, "the list of a top call does not have min(k, imperfect rows) records (internal error)");
    else if (!(out[i] = top_block(shape, tables[(size_t)i].data(), rows[(size_t)i], w, k))) rc = fail(ctx, CALITAS_EINVAL, "out of memory");
  }
  if (rc) for (int i = 0; i < n_guides; i++) { calitas_free(out[i]); out[i] = nullptr; }
  return rc;
}

// A guide's regions result as the ABI hands it over: struct, by_class entries, the cells of the totals and of every class, the records
// and their class bytes in one block of the library's.
static calitas_regions_t* regions_block(const CountsShape& shape, const uint64_t* table, uint64_t rows, const ScoreWords& w, uint32_t k, uint32_t list_mask,
                                        uint32_t n_classes) {
  const size_t cells = shape.cells(), n = std::min<size_t>(w.top.hits.size(), k);
  const size_t bytes = sizeof(calitas_regions_t) + n_classes * sizeof(calitas_scores_t) + (1 + (size_t)n_classes) * cells * sizeof(uint64_t) +
                       n * sizeof(calitas_top_hit_t) + n;
  calitas_regions_t* r = (calitas_regions_t*)out_alloc(bytes);
  if (!r) return nullptr;
  r->by_class = reinterpret_cast<calitas_scores_t*>(r + 1);
  uint64_t* cell_mem = reinterpret_cast<uint64_t*>(r->by_class + n_classes);
  auto fill = [&](calitas_scores_t* c, uint64_t c_rows, uint64_t perfect, uint64_t sum, uint64_t max, const uint64_t* src) {
    c->rows = c_rows; c->perfect = perfect; c->sum_q32 = sum; c->max_q32 = max;
    c->table.n_mm = shape.n_mm; c->table.n_gaps = shape.n_gaps; c->table.n_pam = shape.n_pam; c->table.rows = c_rows;
    c->table.counts = cell_mem;
    if (src) std::memcpy(cell_mem, src, cells * sizeof(uint64_t)); else std::memset(cell_mem, 0, cells * sizeof(uint64_t));
    cell_mem += cells;
  };
  fill(&r->top.scores, rows, w.perfect, w.sum_q32, w.max_q32, table);
  const bool have = w.reg.n_classes == n_classes;             // (a call without any hit leaves no words: every class is empty)
  for (uint32_t c = 0; c < n_classes; c++) {
    const uint64_t* cw = have ? w.reg.words.data() + (size_t)c * REGION_WORDS : nullptr;
    fill(&r->by_class[c], cw ? cw[3] : 0, cw ? cw[1] : 0, cw ? cw[0] : 0, cw ? cw[2] : 0, have ? w.reg.tables.data() + (size_t)c * cells : nullptr);
  }
  r->top.k = k; r->top.n = (uint32_t)n;
  r->top.hits = reinterpret_cast<calitas_top_hit_t*>(cell_mem);
  if (n) std::memcpy(r->top.hits, w.top.hits.data(), n * sizeof(calitas_top_hit_t));
  r->hit_class = reinterpret_cast<uint8_t*>(r->top.hits + n);
  if (n) std::memcpy(r->hit_class, w.top.cls.data(), n);
  r->n_classes = n_classes; r->list_mask = list_mask;
  return r;
}
// What every regions entry point checks first, and what it gives the model.  Returns an error text or "".
static std::string regions_inputs(const calitas_ctx* ctx, uint32_t k, uint32_t list_mask, ScoreModelHost& mh) {
  if (ctx->regions.empty()) return "the context has no regions (calitas_set_regions)";
  if (k > CALITAS_TOP_MAX) return "k of a regions call must be 0 .. CALITAS_TOP_MAX (256)";
  if (k > 0 && (list_mask & ((1u << ctx->regions.n_classes) - 1u)) == 0) return "list_mask of a regions call has no bit below n_classes";
  mh.top_k = k;
  mh.regions = &ctx->regions;
  mh.list_mask = list_mask & ((1u << ctx->regions.n_classes) - 1u);
  mh.regions_dev = RegionsView{ctx->d_region_seg, ctx->d_region_coarse, ctx->d_region_contig, ctx->regions.n_classes};
  return "";
}
// What a regions call's words must satisfy before they are handed over (internal errors otherwise): the list as long as it can be at
// most, a class byte per record, and the classes' rows adding up to the call's.
static bool regions_words_ok(const ScoreWords& w, uint64_t rows, uint32_t k) {
  if (w.top.hits.size() > std::min<uint64_t>(k, rows - w.perfect) || w.top.cls.size() != w.top.hits.size()) return false;
  if (w.reg.n_classes == 0) return rows == 0;
  uint64_t sum = 0;
  for (uint32_t c = 0; c < w.reg.n_classes; c++) sum += w.reg.words[(size_t)c * REGION_WORDS + 3];
  return sum == rows;
}

int calitas_search_regions(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                           uint32_t k, uint32_t list_mask, calitas_regions_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !model || !out) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *out = nullptr;
  GuideHost gh;
  ScoreModelHost mh;
  std::string e = score_inputs(*guide, model, gh, mh);
  if (e.empty()) e = regions_inputs(ctx, k, list_mask, mh);
  if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e);
  CountsShape shape;
  std::vector<uint64_t> table;
  uint64_t rows = 0;
  ScoreWords w;
  const int rc = calitas_search_counts_impl(ctx, guide, params, &shape, &table, &rows, &mh, &w);
  if (rc) return rc;
  if (!regions_words_ok(w, rows, k)) return fail(ctx, CALITAS_EHIP, "the words of a regions call do not add up to its rows (internal error)");
  *out = regions_block(shape, table.data(), rows, w, k, list_mask, ctx->regions.n_classes);
  return *out ? CALITAS_OK : fail(ctx, CALITAS_EINVAL, "out of memory");
}

int calitas_search_regions_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                 const calitas_score_model_t* model, uint32_t k, uint32_t list_mask, calitas_regions_t** out) {
  if (!ctx) return CALITAS_EINVAL;
  if (n_guides <= 0 || !guides || !params || !model || !out) return fail(ctx, CALITAS_EINVAL, "bad argument");
  for (int i = 0; i < n_guides; i++) out[i] = nullptr;
  ScoreModelHost mh;
  for (int i = 0; i < n_guides; i++) {                        // (all guides of a batch have one length: one model serves them)
    GuideHost gh;
    const std::string e = score_inputs(guides[i], model, gh, mh);
    if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e);
  }
  { const std::string e = regions_inputs(ctx, k, list_mask, mh); if (!e.empty()) return fail(ctx, CALITAS_EINVAL, e); }
  std::vector<std::vector<uint64_t>> tables((size_t)n_guides);
  std::vector<uint64_t> rows((size_t)n_guides, 0);
  std::vector<ScoreWords> words((size_t)n_guides);
  int rc = calitas_search_hits_batch_impl(ctx, n_guides, guides, nullptr, params, nullptr, nullptr, nullptr, nullptr, rows.data(), &tables, &mh, &words);
  for (int i = 0; i < n_guides && !rc; i++) {
    GuideHost gh;
    CountsShape shape;
    const ScoreWords& w = words[(size_t)i];
    std::string e = make_guide_host(guides[i], gh);
    if (e.empty()) e = counts_shape(gh, *params, shape);
    if (!e.empty() || tables[(size_t)i].size() != shape.cells()) rc = fail(ctx, CALITAS_EINVAL, e.empty() ? "a guide's table has another shape than its plan (internal error)" : e);
    else if (!regions_words_ok(w, rows[(size_t)i], k)) rc = fail(ctx, CALITAS_EHIP, "the words of a regions call do not add up to its rows (internal error)");
    else if (!(out[i] = regions_block(shape, tables[(size_t)i].data(), rows[(size_t)i], w, k, list_mask, ctx->regions.n_classes))) rc = fail(ctx, CALITAS_EINVAL, "out of memory");
  }
  if (rc) for (int i = 0; i < n_guides; i++) { calitas_free(out[i]); out[i] = nullptr; }
  return rc;
}

int calitas_scan_candidates(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                            uint32_t** records, uint64_t* n_records) {
  return calitas_scan_candidates_impl(ctx, n_guides, guides, params, records, n_records);
}

int calitas_scan_candidates_columnwise(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                       uint32_t** records, uint64_t* n_records) {
  return calitas_scan_candidates_impl(ctx, n_guides, guides, params, records, n_records, true);
}

int calitas_reference_tiles(const calitas_ctx* ctx, uint64_t* n_tiles, uint64_t* n_dead, uint64_t* n_masked, uint64_t* tile_bases) {
  if (!ctx || !ctx->has_ref) return CALITAS_ESTATE;
  uint64_t n = 0, dead = 0, masked = 0;
  for (const TileInfo& t : ctx->ref.tiles) {
    if (t.contig == 0xFFFFFFFFu) continue;
    n++;
    if (t.flag == 2u) dead++; else if (t.flag == 1u) masked++;
  }
  if (n_tiles) *n_tiles = n;
  if (n_dead) *n_dead = dead;
  if (n_masked) *n_masked = masked;
  if (tile_bases) *tile_bases = ctx->ref.tile;
  return CALITAS_OK;
}

int calitas_contig_packed_base(const calitas_ctx* ctx, int32_t i, uint64_t* gbase) {
  if (!ctx || !ctx->has_ref || i < 0 || i >= (int32_t)ctx->ref.contigs.size() || !gbase) return CALITAS_EINVAL;
  *gbase = ctx->ref.contigs[i].gbase;
  return CALITAS_OK;
}

int calitas_get_timing(const calitas_ctx* ctx, calitas_timing_t* out) {
  if (!ctx || !out) return CALITAS_EINVAL;
  *out = ctx->timing;
  return CALITAS_OK;
}

// -------------------------------------------------------------------------------------------------------------------
// host-side stages
// -------------------------------------------------------------------------------------------------------------------

int calitas_window_filter(const calitas_aln_t* alns, int32_t n, int32_t max_total_diffs, int32_t max_overlap, int32_t* order,
                          int32_t* n_kept) {
  if (!alns || n < 0 || !order || !n_kept) return CALITAS_EINVAL;
  // forward-strand list first, then reverse-strand list, each in the order given
  std::vector<calitas_aln_t> v;
  std::vector<int> src;
  for (int s = 0; s < 2; s++)
    for (int i = 0; i < n; i++) if ((alns[i].strand == '-') == (s == 1)) { v.push_back(alns[i]); src.push_back(i); }
  std::vector<int> kept;
  window_filter(v.data(), (int)v.size(), max_total_diffs, max_overlap, kept);
  for (size_t i = 0; i < kept.size(); i++) order[i] = src[kept[i]];
  *n_kept = (int32_t)kept.size();
  return CALITAS_OK;
}

int calitas_hits_tsv(const calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                     const calitas_aln_t* alns, uint64_t n_alns, const char* aligner_version, const char* time_stamp, char** tsv,
                     uint64_t* n_rows) {
  return calitas_hits_tsv_ext(ctx, guide, guide_id, params, alns, n_alns, nullptr, 0, aligner_version, time_stamp, tsv, n_rows);
}

int calitas_hits_tsv_ext(const calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                         const calitas_aln_t* alns, uint64_t n_alns, const calitas_ext_hit_t* ext, uint64_t n_ext,
                         const char* aligner_version, const char* time_stamp, char** tsv, uint64_t* n_rows) {
  if (n_ext && !ext) return CALITAS_EINVAL;
  if (!ctx || !guide || !params || !tsv || (n_alns && !alns)) return CALITAS_EINVAL;
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  if (!ctx->has_ref) return fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  GuideHost gh;
  std::string e = make_guide_host(*guide, gh);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  std::string version, stamp;
  calitas_default_version_and_stamp(aligner_version, time_stamp, version, stamp);
  *tsv = hits_tsv(ctx->ref, gh, guide_id ? guide_id : "", *params, alns, n_alns, version, stamp, n_rows, ctx->pool, out_alloc, ext, n_ext);
  if (!*tsv) return fail(c, CALITAS_EINVAL, "out of memory");
  return CALITAS_OK;
}

int calitas_hits_counts(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_aln_t* alns,
                        uint64_t n_alns, calitas_counts_t** out) {
  if (!ctx || !guide || !params || !out || (n_alns && !alns)) return CALITAS_EINVAL;
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  *out = nullptr;
  if (!ctx->has_ref) return fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  GuideHost gh;
  CountsShape shape;
  std::string e = make_guide_host(*guide, gh);
  if (e.empty()) e = counts_shape(gh, *params, shape);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  std::vector<uint64_t> table(shape.cells(), 0);
  uint64_t rows = 0;
  e = hits_counts(ctx->ref, gh, *params, alns, n_alns, shape.n_mm, shape.n_gaps, shape.n_pam, table.data(), &rows, ctx->pool);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  *out = counts_block(shape, table.data(), rows);
  return *out ? CALITAS_OK : fail(c, CALITAS_EINVAL, "out of memory");
}

int calitas_hits_scores(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                        const calitas_aln_t* alns, uint64_t n_alns, calitas_scores_t** out) {
  if (!ctx || !guide || !params || !model || !out || (n_alns && !alns)) return CALITAS_EINVAL;
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  *out = nullptr;
  if (!ctx->has_ref) return fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  GuideHost gh;
  ScoreModelHost mh;
  CountsShape shape;
  std::string e = score_inputs(*guide, model, gh, mh);
  if (e.empty()) e = counts_shape(gh, *params, shape);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  std::vector<uint64_t> table(shape.cells(), 0);
  uint64_t rows = 0;
  ScoreWords w;
  e = hits_scores(ctx->ref, gh, *params, mh, alns, n_alns, shape.n_mm, shape.n_gaps, shape.n_pam, table.data(), &rows, &w.perfect, &w.sum_q32, &w.max_q32,
                  ctx->pool);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  *out = scores_block(shape, table.data(), rows, w);
  return *out ? CALITAS_OK : fail(c, CALITAS_EINVAL, "out of memory");
}

int calitas_hits_top(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                     uint32_t k, const calitas_aln_t* alns, uint64_t n_alns, calitas_top_t** out) {
  if (!ctx || !guide || !params || !model || !out || (n_alns && !alns)) return CALITAS_EINVAL;
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  *out = nullptr;
  if (!ctx->has_ref) return fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  if (k == 0 || k > CALITAS_TOP_MAX) return fail(c, CALITAS_EINVAL, kBadTopK);
  GuideHost gh;
  ScoreModelHost mh;
  CountsShape shape;
  std::string e = score_inputs(*guide, model, gh, mh);
  if (e.empty()) e = counts_shape(gh, *params, shape);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  std::vector<uint64_t> table(shape.cells(), 0);
  uint64_t rows = 0;
  ScoreWords w;
  w.top.k = k;
  e = hits_top(ctx->ref, gh, *params, mh, alns, n_alns, shape.n_mm, shape.n_gaps, shape.n_pam, table.data(), &rows, &w.perfect, &w.sum_q32, &w.max_q32,
               &w.top, ctx->pool);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  *out = top_block(shape, table.data(), rows, w, k);
  return *out ? CALITAS_OK : fail(c, CALITAS_EINVAL, "out of memory");
}

int calitas_hits_regions(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, const calitas_score_model_t* model,
                         uint32_t k, uint32_t list_mask, const calitas_aln_t* alns, uint64_t n_alns, calitas_regions_t** out) {
  if (!ctx || !guide || !params || !model || !out || (n_alns && !alns)) return CALITAS_EINVAL;
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  *out = nullptr;
  if (!ctx->has_ref) return fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  GuideHost gh;
  ScoreModelHost mh;
  CountsShape shape;
  std::string e = score_inputs(*guide, model, gh, mh);
  if (e.empty()) e = regions_inputs(ctx, k, list_mask, mh);
  if (e.empty()) e = counts_shape(gh, *params, shape);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  std::vector<uint64_t> table(shape.cells(), 0);
  uint64_t rows = 0;
  ScoreWords w;
  w.top.k = k;
  e = hits_regions(ctx->ref, gh, *params, mh, alns, n_alns, shape.n_mm, shape.n_gaps, shape.n_pam, table.data(), &rows, &w.perfect, &w.sum_q32, &w.max_q32,
                   &w.top, &w.reg, ctx->pool);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  *out = regions_block(shape, table.data(), rows, w, k, list_mask, ctx->regions.n_classes);
  return *out ? CALITAS_OK : fail(c, CALITAS_EINVAL, "out of memory");
}

int calitas_padded_strings(const calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_aln_t* aln, char* padded_guide,
                           char* padded_alignment, char* padded_target) {
  if (!ctx || !ctx->has_ref || !guide || !aln || !padded_guide || !padded_alignment || !padded_target) return CALITAS_EINVAL;
  GuideHost gh;
  std::string e = make_guide_host(*guide, gh);
  if (!e.empty()) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, e);
  std::string pg, pa, pt;
  padded_strings(ctx->ref, gh, *aln, pg, pa, pt);
  std::strcpy(padded_guide, pg.c_str()); std::strcpy(padded_alignment, pa.c_str()); std::strcpy(padded_target, pt.c_str());
  return CALITAS_OK;
}

// Activity scores (sites_scored.cpp, activity.hip): no reference counterpart.  The newest entry points stand last, so that everything
// above keeps its place in the object file.
// (the model is the implementation's to check: it comes after everything calitas_find_sites_filtered refuses)
int calitas_find_sites_scored(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_activity_model_t* model,
                              int32_t min_score_q16, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, int32_t** scores,
                              uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || (sites == nullptr) != (scores == nullptr)) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) { *sites = nullptr; *scores = nullptr; }
  return calitas_find_sites_scored_impl(ctx, pattern, filter, model, min_score_q16, chrom_index, start, end, sites, scores, n_sites);
}

int calitas_find_sites_scored_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                   const calitas_activity_model_t* model, int32_t min_score_q16, int32_t chrom_index, uint64_t start, uint64_t end,
                                   calitas_site_t** sites, int32_t** scores, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || (sites == nullptr) != (scores == nullptr)) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) { *sites = nullptr; *scores = nullptr; }
  return calitas_find_sites_scored_host_impl(ctx, pattern, filter, model, min_score_q16, chrom_index, start, end, sites, scores, n_sites);
}

// Sites by annotated regions (sites_regions.cpp, site_regions.hip): no reference counterpart.
int calitas_find_sites_regions(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_regions_t* opt,
                               int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, uint8_t** classes, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || (sites == nullptr) != (classes == nullptr)) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) { *sites = nullptr; *classes = nullptr; }
  return calitas_find_sites_regions_impl(ctx, pattern, filter, opt, chrom_index, start, end, sites != nullptr, sites, classes, nullptr, n_sites);
}

int calitas_count_sites_regions(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_regions_t* opt,
                                int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* per_class_strand, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  return calitas_find_sites_regions_impl(ctx, pattern, filter, opt, chrom_index, start, end, false, nullptr, nullptr, per_class_strand, n_sites);
}

int calitas_find_sites_regions_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                    const calitas_site_regions_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                    uint8_t** classes, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || (sites == nullptr) != (classes == nullptr)) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) { *sites = nullptr; *classes = nullptr; }
  return calitas_find_sites_regions_host_impl(ctx, pattern, filter, opt, chrom_index, start, end, sites != nullptr, sites, classes, nullptr, n_sites);
}

int calitas_count_sites_regions_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                     const calitas_site_regions_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* per_class_strand,
                                     uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  return calitas_find_sites_regions_host_impl(ctx, pattern, filter, opt, chrom_index, start, end, false, nullptr, nullptr, per_class_strand, n_sites);
}

int calitas_site_presence(const calitas_ctx* ctx, uint8_t** bytes, uint64_t* n, uint64_t* first_word) {
  if (!ctx) return CALITAS_EINVAL;
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  if (!bytes || !n || !first_word) return fail(c, CALITAS_EINVAL, "NULL argument");
  *bytes = nullptr; *n = 0; *first_word = 0;
  if (!ctx->has_ref) return fail(c, CALITAS_ESTATE, "calitas_set_reference has not been called");
  if (ctx->regions.empty()) return fail(c, CALITAS_EINVAL, "site regions: the context has no regions (calitas_set_regions)");
  const std::vector<uint8_t>* table = nullptr;
  const std::string e = site_presence(c, &table);
  if (!e.empty()) return fail(c, CALITAS_EINVAL, e);
  *bytes = (uint8_t*)calitas_out_alloc(std::max<size_t>(1, table->size()));
  if (!*bytes) return fail(c, CALITAS_EINVAL, "out of memory");
  if (!table->empty()) std::memcpy(*bytes, table->data(), table->size());
  *n = table->size();
  return CALITAS_OK;
}

// Sites in pairs (sites_pairs.cpp, site_pairs.hip): no reference counterpart.
int calitas_find_site_pairs(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_pairs_t* opt,
                            int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, uint64_t* n_sites, calitas_site_pair_t** pairs,
                            uint64_t* n_pairs) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !sites || !n_sites || !pairs || !n_pairs) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *sites = nullptr; *n_sites = 0; *pairs = nullptr; *n_pairs = 0;
  return calitas_find_site_pairs_impl(ctx, pattern, filter, opt, chrom_index, start, end, true, sites, n_sites, pairs, n_pairs, nullptr);
}

int calitas_count_site_pairs(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_site_pairs_t* opt,
                             int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* n_sites, uint64_t* n_pairs, uint64_t* per_orientation) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || !n_pairs) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0; *n_pairs = 0;
  return calitas_find_site_pairs_impl(ctx, pattern, filter, opt, chrom_index, start, end, false, nullptr, n_sites, nullptr, n_pairs, per_orientation);
}

int calitas_find_site_pairs_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                 const calitas_site_pairs_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                 uint64_t* n_sites, calitas_site_pair_t** pairs, uint64_t* n_pairs) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !sites || !n_sites || !pairs || !n_pairs) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *sites = nullptr; *n_sites = 0; *pairs = nullptr; *n_pairs = 0;
  return calitas_find_site_pairs_host_impl(ctx, pattern, filter, opt, chrom_index, start, end, true, sites, n_sites, pairs, n_pairs, nullptr);
}

int calitas_count_site_pairs_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                  const calitas_site_pairs_t* opt, int32_t chrom_index, uint64_t start, uint64_t end, uint64_t* n_sites,
                                  uint64_t* n_pairs, uint64_t* per_orientation) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || !n_pairs) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0; *n_pairs = 0;
  return calitas_find_site_pairs_host_impl(ctx, pattern, filter, opt, chrom_index, start, end, false, nullptr, n_sites, nullptr, n_pairs, per_orientation);
}

// Allele-specific sites (sites_snv.cpp, allele_sites.hip): no reference counterpart.
int calitas_find_allele_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, calitas_allele_site_t** sites,
                              uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !sites || !n_sites) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *sites = nullptr; *n_sites = 0;
  return calitas_find_allele_sites_impl(ctx, pattern, snvs, n_snvs, true, sites, nullptr, n_sites, status);
}

int calitas_count_allele_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, uint64_t* per_kind,
                               uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  return calitas_find_allele_sites_impl(ctx, pattern, snvs, n_snvs, false, nullptr, per_kind, n_sites, status);
}

int calitas_find_allele_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs,
                                   calitas_allele_site_t** sites, uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !sites || !n_sites) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *sites = nullptr; *n_sites = 0;
  return calitas_find_allele_sites_host_impl(ctx, pattern, snvs, n_snvs, true, sites, nullptr, n_sites, status);
}

int calitas_count_allele_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_snv_t* snvs, uint64_t n_snvs, uint64_t* per_kind,
                                    uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  return calitas_find_allele_sites_host_impl(ctx, pattern, snvs, n_snvs, false, nullptr, per_kind, n_sites, status);
}

// Base-editor guides of a SNV (sites_snv.cpp, edit_sites.hip): no reference counterpart.
int calitas_find_edit_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs, uint64_t n_snvs,
                            calitas_edit_site_t** sites, uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !edit || !sites || !n_sites) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *sites = nullptr; *n_sites = 0;
  return calitas_find_edit_sites_impl(ctx, pattern, edit, snvs, n_snvs, true, sites, nullptr, n_sites, status);
}

int calitas_count_edit_sites(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs, uint64_t n_snvs,
                             uint64_t* per_bystanders, uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !edit || !n_sites) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  return calitas_find_edit_sites_impl(ctx, pattern, edit, snvs, n_snvs, false, nullptr, per_bystanders, n_sites, status);
}

int calitas_find_edit_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs,
                                 uint64_t n_snvs, calitas_edit_site_t** sites, uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !edit || !sites || !n_sites) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *sites = nullptr; *n_sites = 0;
  return calitas_find_edit_sites_host_impl(ctx, pattern, edit, snvs, n_snvs, true, sites, nullptr, n_sites, status);
}

int calitas_count_edit_sites_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_base_edit_t* edit, const calitas_snv_t* snvs,
                                  uint64_t n_snvs, uint64_t* per_bystanders, uint64_t* n_sites, uint8_t* status) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !edit || !n_sites) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  return calitas_find_edit_sites_host_impl(ctx, pattern, edit, snvs, n_snvs, false, nullptr, per_bystanders, n_sites, status);
}

// Microhomology scores (sites_scored.cpp, microhomology.hip): no reference counterpart.
// (the model is the implementation's to check: it comes after everything calitas_find_sites_filtered refuses)
int calitas_find_sites_microhomology(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_mh_model_t* model,
                                     int32_t min_out_of_frame_permille, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                     calitas_mh_score_t** scores, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || (sites == nullptr) != (scores == nullptr)) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) { *sites = nullptr; *scores = nullptr; }
  return calitas_find_sites_microhomology_impl(ctx, pattern, filter, model, min_out_of_frame_permille, chrom_index, start, end, sites, scores, n_sites);
}

int calitas_find_sites_microhomology_host(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                          const calitas_mh_model_t* model, int32_t min_out_of_frame_permille, int32_t chrom_index, uint64_t start,
                                          uint64_t end, calitas_site_t** sites, calitas_mh_score_t** scores, uint64_t* n_sites) {
  if (!ctx) return CALITAS_EINVAL;
  if (!pattern || !n_sites || (sites == nullptr) != (scores == nullptr)) return fail(const_cast<calitas_ctx*>(ctx), CALITAS_EINVAL, "NULL argument");
  *n_sites = 0;
  if (sites) { *sites = nullptr; *scores = nullptr; }
  return calitas_find_sites_microhomology_host_impl(ctx, pattern, filter, model, min_out_of_frame_permille, chrom_index, start, end, sites, scores, n_sites);
}

}  // extern "C"
