// search_run.cpp -- the calitas_search chain on one context or lane: scan -> align -> trace -> per-window filter (device or host) ->
// alignment records, with its retry after an overflow; calitas_search and calitas_scan_candidates themselves.  The row stage and
// everything about lanes is in search_lane.cpp.
#include <algorithm>
#include <cstring>

#include "search_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

// Guides, cleared counters and the scan kernel of this lane, queued on `stream` (the lane's own, or the shared scan stream of a
// chunked search).  t_scan0 / t_scan1 bracket the kernel: ev[0], and the lane's scan_done (the event its stream waits for) or ev[1].
// Both ride on the dispatch itself (hipExtLaunchKernel): as marker packets of their own on the lowest-priority stream they delayed
// whatever waited for the end of the scan by 60-90 us.
// (Queuing the inputs of all ranges first and their scans back to back was tried as well: no gain, the pause between two scans is
// where the previous range's tail gets onto the CUs.)
// The inputs of a lane's scan: guide constants and cleared counters, queued on `stream`.
int queue_scan_inputs(calitas_ctx* ctx, const SearchPlan& pl, hipStream_t stream) {
  // from the context's pinned copy (an async copy from pageable memory may wait for the stream to drain)
  std::memcpy(ctx->h_guides, pl.gd.data(), sizeof(GuideDev) * pl.n_guides);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_guides, ctx->h_guides, sizeof(GuideDev) * pl.n_guides, hipMemcpyHostToDevice, stream));
  g_marks.mark("guides");
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8 * sizeof(uint32_t), stream));
  g_marks.mark("counters");
  return CALITAS_OK;
}

// columnwise: round 1's column-wise scan_kernel (scan_columns.hip) instead of scan_rows_kernel.  Only calitas_scan_candidates_columnwise
// asks for it -- a test hook that holds the two kernels' record sets against each other; no search path does.
int launch_scan_stage(calitas_ctx* ctx, const SearchPlan& pl, hipStream_t stream, bool inputs_queued, bool columnwise) {
  { int rc = check_resident(ctx, pl); if (rc) return rc; }
  if (!inputs_queued) { int rc = queue_scan_inputs(ctx, pl, stream); if (rc) return rc; }
  ScanArgs sa; AlignArgs aa;
  fill_kernel_args(ctx, pl, sa, aa);
  ctx->t_scan0 = ctx->ev[0];
  ctx->t_scan1 = ctx->scan_done ? ctx->scan_done : ctx->ev[1];
  // the events ride on the dispatch
  if (columnwise) HIP_TRY(ctx, launch_scan(sa, ref_owner(ctx)->ref.chunk, pl.n_tiles, stream, ctx->t_scan0, ctx->t_scan1));
  else HIP_TRY(ctx, launch_scan_rows(sa, ref_owner(ctx)->ref.chunk, pl.warm_words, pl.n_tiles, stream, ctx->t_scan0, ctx->t_scan1));
  return CALITAS_OK;
}

// Kernel durations of the last search on this context, from its events (all of them complete).
void kernel_times(calitas_ctx* ctx, calitas_timing_t& tm) {
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->t_scan0, ctx->t_scan1); tm.scan_kernel_ms = ms;
  if (ctx->align_ms_by_stamps >= 0) tm.align_kernel_ms = ctx->align_ms_by_stamps;   // (a search the binned tail started and declined: no ev[2])
  else { (void)hipEventElapsedTime(&ms, ctx->t_scan1, ctx->ev[2]); tm.align_kernel_ms = ms; }
  (void)hipEventElapsedTime(&ms, ctx->t_scan0, ctx->ev[3]); tm.gpu_total_ms = ms;
}

// Grids of align_kernel (units of four one-wave workgroups) and trace_kernel.  align_kernel: 2048 workgroups = 8 per CU, each looping
// over its share of the records.  4096 (all the CUs can hold next to nothing else: 16 x ~11 KB of LDS) was round 2's choice; swept again
// with three jobs per wave (tools/sweep_align.sh, profiles/r03_sweep_align.txt): 384-683 units beat 1024 at every size -- 2.33-2.35
// against 2.42 ms for the hg38-sized call, 0.77 against 0.87 ms for a quarter, 0.51 against 0.53 ms for an eighth -- because the
// scan of the next range keeps more of each CU while the tail runs beside it, and below 256 units the aligner itself runs out of waves.
// trace_kernel's grid makes no difference between 512 and 2048 (256 costs 0.3 ms at full size).
// CALITAS_ALIGN_BLOCKS / CALITAS_TRACE_BLOCKS (and ..._NARROW for the ranges whose tail runs beside the next range's scan) override.
constexpr int kAlignBlocks = 512, kTraceBlocks = 2048;
// ... with two jobs per lane group (align_pk_kernel, round 5) a wave does the work of two: 256 units beside a scan (an eighth of the
// genome as a rank's window range: 0.446 against 0.494 ms at 512, tools/owned_sweep.py), 384 for a tail that runs alone.
constexpr int kAlignBlocksPackedNarrow = 256, kAlignBlocksPacked = 384;
static int narrow_blocks(const char* e, int fallback) {   // e = the switch's value (TUNE_GET), or null
  if (e) { const int v = std::atoi(e); if (v >= 1 && v <= 8192) return v; }
  return fallback;
}
// align_kernel and trace_kernel of a plan on `stream` with the grids above; `trace_done` (may be null) is recorded behind trace_kernel.
hipError_t launch_align_trace(const SearchPlan& pl, const AlignArgs& aa, hipStream_t stream, hipEvent_t trace_done) {
  hipError_t e = launch_align(aa, narrow_blocks(pl.narrow_tail ? TUNE_GET("CALITAS_ALIGN_BLOCKS_NARROW") : TUNE_GET("CALITAS_ALIGN_BLOCKS"), aa.pack16 && !aa.sp.per_matrix ? (pl.narrow_tail ? kAlignBlocksPackedNarrow : kAlignBlocksPacked) : kAlignBlocks), stream);
  if (e != hipSuccess) return e;
  return launch_trace(aa, narrow_blocks(pl.narrow_tail ? TUNE_GET("CALITAS_TRACE_BLOCKS_NARROW") : TUNE_GET("CALITAS_TRACE_BLOCKS"), kTraceBlocks), stream, trace_done);
}

// Pinned staging for the copy-back of n alignments: regrown to the lane's whole raw capacity when it is too small.
static int ensure_h_raw(calitas_ctx* ctx, uint32_t n) {
  if (n <= ctx->h_raw_cap) return CALITAS_OK;
  if (ctx->h_raw) (void)hipHostFree(ctx->h_raw);
  ctx->h_raw = nullptr; ctx->h_raw_cap = 0;
  HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_raw, (size_t)ctx->raw_cap * sizeof(RawAln), hipHostMallocDefault));
  ctx->h_raw_cap = ctx->raw_cap;
  return CALITAS_OK;
}

// Copies the device-selected alignments back and converts them to GuideAlignment records (GA:21-31, SGA:260-313).
int convert_selected(calitas_ctx* ctx, const RawAln* d_final, uint32_t n_sel, const std::vector<GuideHost>& gh,
                     const calitas_params_t& p, int step, calitas_aln_t** out) {
  const PackedRef& ref = ref_owner(ctx)->ref;
  { int rc = ensure_h_raw(ctx, n_sel); if (rc) return rc; }
  if (n_sel) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_raw, d_final, (size_t)n_sel * sizeof(RawAln), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, calitas_spin_sync(ctx->stream));
  const RawAln* raw = ctx->h_raw;
  calitas_aln_t* result = (calitas_aln_t*)out_alloc(std::max<size_t>(1, n_sel) * sizeof(calitas_aln_t));
  if (!result) return fail(ctx, CALITAS_EINVAL, "out of memory");
  ref_owner(ctx)->pool->for_blocks(n_sel, [&](size_t b, size_t e, int) {
    for (size_t i = b; i < e; i++) {
      const RawAln& r = raw[i];
      int64_t wa = 0, wb = 0;
      window_bounds(ref.runs.data(), (int64_t)ref.runs.size(), ref.contigs[r.contig].gbase, ref.contigs[r.contig].len, p.window_size, step,
                    r.window_k, wa, wb);
      raw_to_aln(r, gh[r.guide], wa, wb, result[i]);
    }
  });
  *out = result;
  return CALITAS_OK;
}

// A round of the search overflowed a buffer: all of them resized from what the kernels counted, for the next round.
static int grow_after_overflow(calitas_ctx* ctx, const SearchPlan& pl, uint32_t n_rec, uint32_t n_raw, uint32_t n_items) {
  uint64_t nr = n_rec > ctx->rec_cap ? (uint64_t)n_rec + n_rec / 4 : ctx->rec_cap;
  uint64_t nw = n_raw > ctx->raw_cap ? (uint64_t)n_raw * 2 : ctx->raw_cap;
  if (n_rec > ctx->rec_cap)   // the raw count was cut short as well: scale it with the record count
    nw = std::max<uint64_t>(nw, (uint64_t)((double)n_raw * nr / std::max<uint32_t>(1, ctx->rec_cap)) + 1024);
  if (nr > 0xFFFFFFF0ull || nw > 0xFFFFFFF0ull) return fail(ctx, CALITAS_EINVAL, "result volume exceeds 2^32 records");
  // passing candidates: as counted, or scaled with the record count when that was cut short
  uint64_t ni = n_items > ctx->item_cap ? (uint64_t)n_items + n_items / 4 : ctx->item_cap;
  if (n_rec > ctx->rec_cap) ni = std::max<uint64_t>(ni, (uint64_t)((double)std::max<uint32_t>(n_items, 1024) * nr / std::max<uint32_t>(1, ctx->rec_cap)) * 2);
  if (ni > 0xFFFFFFF0ull) return fail(ctx, CALITAS_EINVAL, "result volume exceeds 2^32 records");
  return ensure_buffers(ctx, (uint32_t)nr, (uint32_t)nw, pl.slab_per_rec, (uint32_t)ni);
}

// The per-window filter on the host, from the n_raw alignments copied to ctx->h_raw; completes tm and leaves it in ctx->timing.
static int host_window_filter(calitas_ctx* ctx, const SearchPlan& pl, uint32_t n_rec, uint32_t n_raw, calitas_timing_t& tm,
                              std::chrono::steady_clock::time_point t_call, calitas_aln_t** out, uint64_t* n_out) {
  // ---- host: restore the reference's enumeration order, then the per-window filter (SGA:315-320) ----
  const calitas_params_t& p = pl.p;
  const PackedRef& ref = ref_owner(ctx)->ref;
  const int n_guides = pl.n_guides, step = pl.step, max_total = pl.max_total;
  const std::vector<GuideHost>& gh = pl.gh;
  const RawAln* raw = ctx->h_raw;
  WorkerPool* pool = ref_owner(ctx)->pool;                                  // lanes share the owner's pool, one at a time
  std::lock_guard<std::mutex> host_lock(ref_owner(ctx)->host_mu);
  // Raw records arrive in atomic-append order.  They are bucketed by (guide, contig, 4096-window chunk), each bucket is
  // sorted by (window, strand list, end column, PAM) = fgbio's enumeration order (ascending end column) followed
  // by the PAM order of extendAndFilterRight (SGA:455), filtered window by window, and the buckets are concatenated.
  auto t0 = std::chrono::steady_clock::now();
  constexpr int WCHUNK_SHIFT = 12;
  const size_t n_contigs = ref.contigs.size();
  std::vector<uint64_t> chunk_base(n_contigs + 1, 0);   // bucket index base per contig (within one guide)
  for (size_t c = 0; c < n_contigs; c++)
    chunk_base[c + 1] = chunk_base[c] + ((window_count(ref.contigs[c].len, step) >> WCHUNK_SHIFT) + 1);
  const uint64_t buckets_per_guide = chunk_base[n_contigs];
  const size_t n_buckets = (size_t)(buckets_per_guide * (uint64_t)n_guides);
  auto bucket_of = [&](const RawAln& r) { return (size_t)(r.guide * buckets_per_guide + chunk_base[r.contig] + (r.window_k >> WCHUNK_SHIFT)); };
  std::vector<uint32_t> bucket_off(n_buckets + 1, 0);
  for (uint32_t i = 0; i < n_raw; i++) bucket_off[bucket_of(raw[i]) + 1]++;
  for (size_t b = 0; b < n_buckets; b++) bucket_off[b + 1] += bucket_off[b];
  std::vector<uint32_t> perm(n_raw);
  {
    std::vector<uint32_t> cur(bucket_off.begin(), bucket_off.end() - 1);
    for (uint32_t i = 0; i < n_raw; i++) perm[cur[bucket_of(raw[i])]++] = i;
  }
  const auto t_bucketed = std::chrono::steady_clock::now();
  std::vector<std::vector<calitas_aln_t>> bucket_out(n_buckets);
  {
    std::atomic<size_t> next(0);
    pool->run([&](int) {
      std::vector<std::pair<uint64_t, uint32_t>> keyed;
      std::vector<calitas_aln_t> win;
      std::vector<int> kept;
      for (;;) {
        size_t b = next.fetch_add(1);
        if (b >= n_buckets) break;
        const uint32_t lo = bucket_off[b], hi = bucket_off[b + 1];
        if (lo == hi) continue;
        keyed.clear();
        for (uint32_t i = lo; i < hi; i++) {
          const RawAln& r = raw[perm[i]];
          const uint64_t list = gh[r.guide].pam5 ? (r.dir == 1 ? 0 : 1) : (r.dir == 0 ? 0 : 1);   // 0 = forward-strand list (SGA:316)
          const uint64_t key = ((uint64_t)r.window_k << 24) | (list << 23) | ((uint64_t)r.t_end_guide << 7) | ((uint64_t)r.pad << 5) | (uint64_t)(r.pam + 1);
          keyed.emplace_back(key, perm[i]);
        }
        std::sort(keyed.begin(), keyed.end());
        auto& outv = bucket_out[b];
        size_t i = 0;
        while (i < keyed.size()) {
          const RawAln& f = raw[keyed[i].second];
          size_t j = i;
          while (j < keyed.size() && raw[keyed[j].second].window_k == f.window_k) j++;
          int64_t wa = 0, wb = 0;
          window_bounds(ref.runs.data(), (int64_t)ref.runs.size(), ref.contigs[f.contig].gbase, ref.contigs[f.contig].len, p.window_size,
                        step, f.window_k, wa, wb);
          if (win.size() < j - i) win.resize(j - i);
          for (size_t k = i; k < j; k++) raw_to_aln(raw[keyed[k].second], gh[f.guide], wa, wb, win[k - i]);
          window_filter(win.data(), (int)(j - i), max_total, p.max_overlap, kept);
          for (int k : kept) outv.push_back(win[k]);
          i = j;
        }
      }
    });
  }
  const auto t_filtered = std::chrono::steady_clock::now();
  std::vector<size_t> out_off(n_buckets + 1, 0);
  for (size_t b = 0; b < n_buckets; b++) out_off[b + 1] = out_off[b] + bucket_out[b].size();
  const size_t n_result = out_off[n_buckets];
  calitas_aln_t* result = (calitas_aln_t*)out_alloc(std::max<size_t>(1, n_result) * sizeof(calitas_aln_t));
  if (!result) return fail(ctx, CALITAS_EINVAL, "out of memory");
  {
    std::atomic<size_t> next(0);
    pool->run([&](int) {
      for (;;) {
        size_t b = next.fetch_add(1);
        if (b >= n_buckets) break;
        if (!bucket_out[b].empty()) std::memcpy(result + out_off[b], bucket_out[b].data(), bucket_out[b].size() * sizeof(calitas_aln_t));
      }
    });
  }
  tm.host_post_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (TUNE_GET("CALITAS_TRACE")) {
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "[calitas] host filter: bucket %.2f ms, sort+convert+filter %.2f ms, concat %.2f ms (%zu buckets)\n",
                 ms(t0, t_bucketed), ms(t_bucketed, t_filtered), ms(t_filtered, std::chrono::steady_clock::now()), n_buckets);
  }
  if (TUNE_GET("CALITAS_TRACE"))
    std::fprintf(stderr, "[calitas] search: scan %.3f ms, align %.3f ms, gpu total %.3f ms, host filter %.3f ms, call %.3f ms (%u records, %u raw, %zu accepted)\n",
                 tm.scan_kernel_ms, tm.align_kernel_ms, tm.gpu_total_ms, tm.host_post_ms,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(), n_rec, n_raw, n_result);
  tm.accepted_alignments = n_result;
  tm.candidate_columns = ctx->h_counters[4];   // end columns whose best bottom-row score reached minGuideScore inside a window
  ctx->timing = tm;

  *n_out = n_result;
  *out = result;
  return CALITAS_OK;
}

// calitas_search; with dev != nullptr the accepted alignments stay on the device when the device filter handled them
// (dev->valid), and *out stays NULL.  prelaunched: the scan stage of this lane was queued by the caller on another stream
// and ctx->stream already waits for it; an overflow then fails the call instead of retrying.
// resume: the stages through trace_kernel have run and the lane's counters are in ctx->h_counters (the binned tail declined, see
// lane_rows_binned): the first round starts at the per-window filter.
int search_run(calitas_ctx* ctx, const SearchPlan& pl, calitas_aln_t** out, uint64_t* n_out, DeviceSel* dev, bool prelaunched,
               bool resume) {
  const auto t_call = std::chrono::steady_clock::now();
  *out = nullptr; *n_out = 0;
  if (!resume) ctx->align_ms_by_stamps = -1;
  const calitas_params_t& p = pl.p;
  const int n_guides = pl.n_guides, step = pl.step, max_total = pl.max_total;
  const std::vector<GuideHost>& gh = pl.gh;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!prelaunched) {
    int rc = lane_prepare(ctx, pl);
    if (rc) return rc;
    rc = ensure_window_table(ctx, pl, ctx->stream);
    if (rc) return rc;
  }
  calitas_timing_t tm{};
  tm.bases_scanned = pl.bases;
  tm.packed_bytes = (tm.bases_scanned + 3) / 4;
  uint32_t n_rec = 0, n_raw = 0;
  const calitas_ctx* own = ref_owner(ctx);
  const bool device_filter = !TUNE_GET("CALITAS_HOST_FILTER") && select_supported(pl.win_n, p.window_size, n_guides);
  // A small reference usually yields few alignments: the one-workgroup filter is queued right behind trace_kernel and reads the counts
  // on the device, so the host hears about the counters and the filter's result in one round trip (select_run_speculative).
  const bool speculate = !prelaunched && !resume && device_filter && pl.bases <= (64ull << 20);
  const RawAln* d_spec = nullptr;
  uint32_t spec_counts[3] = {0, 0, 0};
  bool spec_done = false;
  for (bool first_round = true;; first_round = false) {
    if (!(resume && first_round)) {
    ctx->align_ms_by_stamps = -1;                     // (this round's trace_kernel carries ev[2])
    if (!prelaunched) {
      int rc = launch_scan_stage(ctx, pl, ctx->stream);
      if (rc) return rc;
    }
    ScanArgs sa; AlignArgs aa;
    fill_kernel_args(ctx, pl, sa, aa);
    // (trace_kernel can post the counters itself from its last workgroup -- launch_trace's `post` -- but finding the last of 2048
    // workgroups is 2048 atomics on one word, ~8 ns each: 20-30 us against the ~10 us of this launch)
    HIP_TRY(ctx, launch_align_trace(pl, aa, ctx->stream, ctx->ev[2]));
    if (speculate) {
      HIP_TRY(ctx, select_run_speculative(&ctx->select, ctx->d_raw, ctx->d_counters, ctx->rec_cap, ctx->raw_cap, ctx->item_cap, ctx->d_guides,
                                          own->d_win_base, own->d_win, pl.win_lo, pl.win_n, max_total, p.max_overlap, ctx->stream, &d_spec, &ctx->mbox));
      HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    } else {
      HIP_TRY(ctx, mailbox_post(ctx->mbox, ctx->d_counters, 8, ctx->stream));
    }
    g_marks.mark("queued-scan-align-trace");
    HIP_TRY(ctx, mailbox_wait(ctx->mbox, ctx->stream));
    g_marks.mark("counts1");
    for (int k = 0; k < 8; k++) ctx->h_counters[k] = ctx->mbox.host[1 + k];
    if (speculate) { for (int k = 0; k < 3; k++) spec_counts[k] = ctx->mbox.host[9 + k]; spec_done = !(spec_counts[1] & SELECT_FLAG_RETRY); }
    }
    n_rec = ctx->h_counters[0]; n_raw = ctx->h_counters[1];
    const uint32_t n_items = ctx->h_counters[3];
    if (ctx->h_counters[2] != 0) return fail(ctx, CALITAS_EHIP, "aligner kernel reported an inconsistent traceback (internal error)");
    if (n_rec > ctx->rec_cap || n_raw > ctx->raw_cap || n_items > ctx->item_cap) {
      if (prelaunched) return fail(ctx, CALITAS_ESTATE, "lane buffers overflowed");   // the caller reruns unchunked
      tm.retries++;
      int rc = grow_after_overflow(ctx, pl, n_rec, n_raw, n_items);
      if (rc) return rc;
      continue;
    }
    break;
  }
  // ---- per-window filter (SGA:315-320): on the GPU (select.hip) unless the tiling does not fit its sort key, a window
  //      exceeds its group limit, or CALITAS_HOST_FILTER asks for the host implementation of the same stage ----
  bool gpu_select = n_raw > 0 && device_filter;
  uint32_t n_sel = 0;
  const RawAln* d_sel = nullptr;
  if (gpu_select && spec_done) {                    // the filter ran with the aligner kernels: its counts came with theirs
    ctx->h_counters[5] = spec_counts[0]; ctx->h_counters[6] = spec_counts[1]; ctx->h_counters[7] = spec_counts[2];
    n_sel = spec_counts[0];
    d_sel = d_spec;
  } else if (gpu_select) {
    const RawAln* d_final = nullptr;
    const uint32_t* d_cnt = nullptr;
    // (second round: the one-workgroup version met a window it leaves to the general kernels -- here, or already behind trace_kernel)
    for (bool general = speculate && n_raw <= 1024;; general = true) {
      HIP_TRY(ctx, select_run(&ctx->select, ctx->d_raw, n_raw, ctx->d_guides, own->d_win_base, own->d_win, pl.win_lo, pl.win_n, n_guides, max_total,
                              p.max_overlap, ctx->stream, &d_final, &d_cnt, &ctx->mbox, general));   // its last kernel posts the three counts
      HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
      g_marks.mark("queued-filter");
      HIP_TRY(ctx, mailbox_wait(ctx->mbox, ctx->stream));
      g_marks.mark("counts2");
      if (general || !(ctx->mbox.host[2] & SELECT_FLAG_RETRY)) break;
    }
    ctx->h_counters[5] = ctx->mbox.host[1]; ctx->h_counters[6] = ctx->mbox.host[2]; ctx->h_counters[7] = ctx->mbox.host[3];
    select_done(ctx->select);
    if (ctx->h_counters[6] & SELECT_FLAG_INTERNAL)
      return fail(ctx, CALITAS_EHIP, "per-window filter: window counters were not clear at the start of the stage (internal error)");
    if (ctx->h_counters[6] != 0) gpu_select = false;   // a window beyond what the device filter handles
    else {
      n_sel = ctx->h_counters[5];
      d_sel = d_final;
    }
  }
  if (!gpu_select && n_raw) {
    int rc = ensure_h_raw(ctx, n_raw);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_raw, ctx->d_raw, (size_t)n_raw * sizeof(RawAln), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (!gpu_select) {              // (the device filter recorded ev[3] and waited above)
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    HIP_TRY(ctx, calitas_spin_sync(ctx->stream));
  }
  if (!(gpu_select && dev)) kernel_times(ctx, tm);   // calitas_search_hits asks later, while its row kernels run
  tm.scan_records = n_rec;
  tm.raw_alignments = n_raw;

  if (gpu_select) {
    tm.accepted_alignments = n_sel;
    tm.candidate_columns = ctx->h_counters[4];
    if (dev) {   // calitas_search_hits goes on from the device copy
      dev->valid = true; dev->d_final = d_sel; dev->n_sel = n_sel; dev->crowded = ctx->h_counters[7] != 0;
      ctx->timing = tm;
      return CALITAS_OK;
    }
    // accepted alignments arrive in final order; only the coordinate conversion (GA:21-31, SGA:260-313) is left
    auto t0 = std::chrono::steady_clock::now();
    calitas_aln_t* result = nullptr;
    int rc = convert_selected(ctx, d_sel, n_sel, gh, p, step, &result);
    if (rc) return rc;
    tm.host_post_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ctx->timing = tm;
    if (TUNE_GET("CALITAS_TRACE"))
      std::fprintf(stderr, "[calitas] search: scan %.3f ms, align %.3f ms, gpu total %.3f ms (incl. sort+filter on the GPU), copy+convert %.3f ms, call %.3f ms (%u records, %u raw, %u accepted)\n",
                   tm.scan_kernel_ms, tm.align_kernel_ms, tm.gpu_total_ms, tm.host_post_ms,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(), n_rec, n_raw, n_sel);
    *n_out = n_sel;
    *out = result;
    return CALITAS_OK;
  }
  return host_window_filter(ctx, pl, n_rec, n_raw, tm, t_call, out, n_out);
}

}  // namespace calitas

int calitas_search_impl(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                        calitas_aln_t** out, uint64_t* n_out) {
  if (!ctx) return CALITAS_EINVAL;
  if (!out || !n_out) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *out = nullptr; *n_out = 0;
  SearchPlan pl;
  int rc = plan_search(ctx, n_guides, guides, params, pl);
  if (rc) return rc;
  return search_run(ctx, pl, out, n_out, nullptr, false);
}

// calitas_scan_candidates: plan, scan stage, records back (sorted).  Test and profiling entry; no lanes.
int calitas_scan_candidates_impl(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params,
                                 uint32_t** records, uint64_t* n_records, bool columnwise) {
  if (!ctx) return CALITAS_EINVAL;
  if (!records || !n_records) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  *records = nullptr; *n_records = 0;
  SearchPlan pl;
  int rc = plan_search(ctx, n_guides, guides, params, pl);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = lane_prepare(ctx, pl);
  if (rc) return rc;
  uint32_t n_rec = 0;
  for (;;) {
    rc = launch_scan_stage(ctx, pl, ctx->stream, false, columnwise);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    n_rec = ctx->h_counters[0];
    if (n_rec <= ctx->rec_cap) break;
    const uint64_t grown = (uint64_t)n_rec + n_rec / 4;        // 64-bit: a dense PAM-less scan can pass 3.4e9 records
    if (grown > 0xFFFFFFF0ull) return fail(ctx, CALITAS_EINVAL, "result volume exceeds 2^32 records");
    rc = ensure_buffers(ctx, (uint32_t)grown, ctx->raw_cap, pl.slab_per_rec, ctx->item_cap);
    if (rc) return rc;
  }
  static_assert(sizeof(ScanRecord) == 8, "two words per record");
  uint64_t* recs = (uint64_t*)out_alloc(std::max<size_t>(1, n_rec) * sizeof(ScanRecord));
  if (!recs) return fail(ctx, CALITAS_EINVAL, "out of memory");
  if (n_rec) HIP_TRY(ctx, hipMemcpy(recs, ctx->d_recs, (size_t)n_rec * sizeof(ScanRecord), hipMemcpyDeviceToHost));
  // {gword, info} little-endian as one 64-bit key: sort by info then gword would interleave; sort by (gword, info) instead
  std::sort(recs, recs + n_rec, [](uint64_t a, uint64_t b) {
    const uint64_t ka = (a << 32) | (a >> 32), kb = (b << 32) | (b >> 32);
    return ka < kb;
  });
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->t_scan0, ctx->t_scan1);
  ctx->timing = calitas_timing_t{};
  ctx->timing.scan_kernel_ms = ms; ctx->timing.scan_records = n_rec; ctx->timing.bases_scanned = pl.bases; ctx->timing.packed_bytes = (pl.bases + 3) / 4;
  if (!columnwise) ctx->timing.scan_variant = (uint32_t)ref_owner(ctx)->ref.chunk << 8 | (uint32_t)pl.warm_words;
  *records = (uint32_t*)recs;
  *n_records = n_rec;
  return CALITAS_OK;
}
