// search_batch.cpp -- calitas_search_hits_batch: guides flowing through the lanes as a pipeline.  The lanes themselves are in
// search_lane.cpp; a guide the pipeline cannot finish goes through calitas_search_hits (search_hits.cpp).
#include <algorithm>
#include <cstring>

#include "search_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

// The plans of a batch, the lanes and their buffers, the window table.
static int plan_batch(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params, int n_lanes,
                      std::vector<SearchPlan>& plans, std::vector<char>& owned_ok) {
  // plans first: every guide is validated before anything is queued, and all must share one window tiling
  // A window range (a process's stretch of a multi-GPU job): every guide's plan is the stretch's -- the rows it owns, decided by the
  // per-bin kernels (plan_owned_range); a guide whose bins decline goes through calitas_search_hits on the range afterwards.
  const bool ranged = params && (params->first_window != 0 || params->n_windows != 0);
  calitas_params_t whole = *params;
  whole.first_window = 0; whole.n_windows = 0;
  if (ranged && whole.chrom_index >= 0) return fail(ctx, CALITAS_EINVAL, "a window range and chrom_index exclude each other");
  for (int i = 0; i < n_guides; i++) {
    int rc = plan_search(ctx, 1, &guides[i], &whole, plans[i]);
    if (rc) return rc;
    if (plans[i].step != plans[0].step)
      return fail(ctx, CALITAS_EINVAL, "all guides of one batch must have the same length (same window tiling, SearchReference.scala:529)");
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (int i = 0; i < n_guides; i++) { int rc = ensure_bin_base(ctx, plans[i], ctx->stream); if (rc) return rc; }
  // Which tail: every guide's tail runs beside the scans of the guides behind it, where the per-bin kernels cost the scans more than
  // they save the tail (binned_possible: the three-range call's finding) -- the general kernels, then, unless the batch
  // runs on a stretch, which only the bins can own.  (Round 3 got there by accident: the first guide that crowded a bin switched the
  // bins off for every guide behind it; with the decline remembered per guide the batch took 328 instead of 295 ms per 96 guides.)
  // (A reference below 2 Gb keeps the bins, as a single call on it does: fewer launches, and its scans are short.)
  if (!ranged && ctx->ref.total_bases >= (2048ull << 20)) for (auto& q : plans) q.three_ranges = true;
  if (ranged) {
    if (params->first_window < 0 || params->n_windows <= 0 || (uint64_t)params->first_window + (uint64_t)params->n_windows > plans[0].win_n)
      return fail(ctx, CALITAS_EINVAL, "first_window / n_windows outside the window table (" + std::to_string(plans[0].win_n) + " windows)");
    for (int i = 0; i < n_guides; i++)
      owned_ok[(size_t)i] = plan_owned_range(ctx, plans[i], (uint64_t)params->first_window, (uint64_t)params->n_windows) && binned_possible(ctx, plans[i]);
  }
  int rc = ensure_lanes(ctx, (size_t)n_lanes);
  if (rc) return rc;
  for (int l = 0; l < n_lanes && !rc; l++) { rc = lane_prepare(ctx->lanes[l], plans[0]); if (rc) ctx->err = ctx->lanes[l]->err; }
  if (rc) return rc;
  return ensure_window_table(ctx, plans[0], ctx->scan_stream);
}

// The guides' timings summed.  (Not add_lane_timing: this sum leaves out host_post_ms, hits_kernel_ms and hits_copy_ms -- a batch reports
// them as zero, which is on record.)
static calitas_timing_t batch_timing(const std::vector<calitas_timing_t>& tms) {
  calitas_timing_t tm{};
  for (auto& t : tms) {
    tm.scan_kernel_ms += t.scan_kernel_ms; tm.align_kernel_ms += t.align_kernel_ms; tm.gpu_total_ms += t.gpu_total_ms;
    tm.bases_scanned += t.bases_scanned; tm.packed_bytes += t.packed_bytes; tm.scan_records += t.scan_records;
    tm.candidate_columns += t.candidate_columns; tm.raw_alignments += t.raw_alignments; tm.accepted_alignments += t.accepted_alignments;
    tm.retries += t.retries; tm.hit_rows += t.hit_rows; tm.hits_bytes += t.hits_bytes; tm.binned_lanes += t.binned_lanes; tm.owned_general_lanes += t.owned_general_lanes;
  }
  return tm;
}

}  // namespace calitas

// ---- calitas_search_hits_batch ----------------------------------------------------------------------------------------
// Guides flow through the lanes as a pipeline: every lane thread queues the scan of its next guide on the shared low-priority
// scan stream and then runs that guide's tail (align ... rows, copy) on its own stream, so guide g+1 is being scanned while
// guide g's tail runs.  Each guide's text goes to its own pinned buffer.
int calitas_search_hits_batch_impl(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const char* const* guide_ids,
                                  const calitas_params_t* params, const char* aligner_version, const char* time_stamp, char** tsv,
                                  uint64_t* tsv_bytes, uint64_t* n_rows, std::vector<std::vector<uint64_t>>* tables, const ScoreModelHost* model,
                                  std::vector<ScoreWords>* scores) {
  // model, scores (calitas_search_scores_batch): with tables, the tails run in score mode and (*scores)[i] receives guides[i]'s words
  // tables (calitas_search_counts_batch): every guide's tail runs in counts mode and `finish` takes its table -- no text is built, copied
  // or expanded, tsv is not touched; (*tables)[i] and n_rows[i] receive what calitas_search_counts returns for guides[i]
  const bool counting = tables != nullptr;
  const auto t_call = std::chrono::steady_clock::now();
  for (int i = 0; i < n_guides; i++) { if (tsv) tsv[i] = nullptr; if (tsv_bytes) tsv_bytes[i] = 0; if (n_rows) n_rows[i] = 0; }
  // one guide through the single-guide call: when there is nothing to pipeline, and for a guide the pipeline could not finish
  auto single = [&](int i, const std::string& version, const std::string& stamp) -> int {
    if (counting) {
      CountsShape shape;
      uint64_t rows = 0;
      const int rc = calitas_search_counts_impl(ctx, &guides[i], params, &shape, &(*tables)[(size_t)i], &rows, model, scores ? &(*scores)[(size_t)i] : nullptr);
      if (!rc && n_rows) n_rows[i] = rows;
      return rc;
    }
    return calitas_search_hits_impl(ctx, &guides[i], guide_ids && guide_ids[i] ? guide_ids[i] : "", params, version.c_str(), stamp.c_str(), &tsv[i],
                                    tsv_bytes ? &tsv_bytes[i] : nullptr, n_rows ? &n_rows[i] : nullptr);
  };
  std::string version, stamp;
  calitas_default_version_and_stamp(aligner_version, time_stamp, version, stamp);
  auto release = [&]() { if (tsv) for (int i = 0; i < n_guides; i++) { calitas_free(tsv[i]); tsv[i] = nullptr; } };
  // Five guides in flight: with three the bus idled a sixth of the time between the texts of a 96-guide batch on an hg38-sized genome
  // (15.3 GB per batch: 328.6 ms; four lanes 298.0, five 292.1 = 52 GB/s, six 300.6, eight 295.5).
  int n_lanes = 5;
  if (const char* e = TUNE_GET("CALITAS_BATCH_LANES")) n_lanes = std::max(1, std::min(8, std::atoi(e)));
  n_lanes = std::min(n_lanes, (int)n_guides);
  if (n_lanes < 2) {   // nothing to pipeline
    for (int i = 0; i < n_guides; i++) {
      int rc = single(i, version, stamp);
      if (rc) { release(); return rc; }
    }
    return CALITAS_OK;
  }
  std::vector<SearchPlan> plans((size_t)n_guides);
  std::vector<char> owned_ok((size_t)n_guides, 1);
  int rc = plan_batch(ctx, n_guides, guides, params, n_lanes, plans, owned_ok);
  if (rc) return rc;
  if (counting) for (auto& q : plans) { q.counts = true; q.model = model; }
  const PackedRef& ref = ctx->ref;
  std::mutex scan_mu, copy_mu;
  const bool device_rows = !TUNE_GET("CALITAS_HOST_HITS");
  std::atomic<uint64_t> expand_us{0};                           // lane threads' time in expand_rows (their turn on the pool included)
  bool compact_rows = device_rows;
  if (const char* e = TUNE_GET("CALITAS_COMPACT_ROWS")) compact_rows = compact_rows && std::atoi(e) != 0;
  std::vector<int> rcs((size_t)n_guides, CALITAS_OK);
  std::vector<std::string> errs((size_t)n_guides);   // a failed guide's message, kept apart from its lane (a retry below destroys the lanes)
  std::vector<calitas_timing_t> tms((size_t)n_guides);
  // A guide on a lane, in three parts: its scan queued on the scan stream; its tail (aligner, filter, rows) on the lane's stream with
  // the host answering the tail's counters; its text brought to the host (copy + expansion) and handed over.
  struct InFlight {
    int g = -1;
    LaneText lt;
    RowStrings rs_full, rs;
  };
  auto queue_scan = [&](calitas_ctx* lane, int g, InFlight& f) -> int {
    const SearchPlan& pl = plans[g];
    const std::string gid = guide_ids && guide_ids[g] ? guide_ids[g] : "";
    f.g = g;
    f.lt = LaneText();
    f.rs_full = make_row_strings(ref, pl.gh[0], gid, pl.p, version, stamp);
    // the device writes compact rows (post.hpp): a batch is bound by its texts on the bus (15.3 GB per 96 guides on an hg38-sized
    // genome), and 270 of a row's ~520 bytes are the call's constants
    f.rs = compact_rows ? compact_row_strings(f.rs_full) : f.rs_full;
    // the previous guide of this lane is done on the device (its tail ended before this is queued), so the lane's buffers are free
    // for this scan
    if (device_rows) HIP_TRY(lane, queue_row_constants(lane, pl, f.rs));   // before the wait for the scan is queued
    std::lock_guard<std::mutex> lk(scan_mu);
    return launch_scan_stage(lane, pl, ctx->scan_stream);       // records lane->scan_done
  };
  auto run_tail = [&](calitas_ctx* lane, InFlight& f, hipEvent_t scans_done) -> int {
    HIP_TRY(lane, hipStreamWaitEvent(lane->stream, scans_done, 0));
    const std::string gid = guide_ids && guide_ids[f.g] ? guide_ids[f.g] : "";
    return lane_rows(lane, plans[f.g], true, f.rs, gid, version, stamp, f.lt, device_rows);
  };
  auto finish = [&](calitas_ctx* lane, InFlight& f) -> int {
    const int g = f.g;
    LaneText& lt = f.lt;
    if (counting) {                                            // the table is on the host already: nothing to bring in
      if (lt.counts.size() != plans[g].cshape.cells()) return fail(lane, CALITAS_EHIP, "a guide's tail returned no counts table (internal error)");
      (*tables)[(size_t)g] = std::move(lt.counts);
      if (scores) (*scores)[(size_t)g] = lt.score;
      if (n_rows) n_rows[g] = lt.rows;
      tms[g] = lt.tm; tms[g].hit_rows = lt.rows; tms[g].hits_bytes = 0;
      return CALITAS_OK;
    }
    const RowStrings& rs = f.rs;
    const RowStrings& rs_full = f.rs_full;
    const bool expand = compact_rows && !lt.on_host;           // (rows the host stages built are whole already)
    const size_t add = rs_full.head.size() + rs_full.tail.size() - 1;
    const size_t hlen = rs.header.size(), total = hlen + (size_t)lt.bytes + (expand ? (size_t)lt.rows * add : 0);
    char* text = (char*)(expand ? calitas_out_alloc(total + 1) : calitas_out_alloc_pinned(total + 1));
    if (!text) return fail(lane, CALITAS_EINVAL, "out of memory");
    std::memcpy(text, rs.header.data(), hlen);
    if (lt.bytes) {
      char* staging = expand ? (char*)calitas_out_alloc_pinned((size_t)lt.bytes) : nullptr;
      if (expand && !staging) { calitas_free(text); return fail(lane, CALITAS_EINVAL, "out of memory"); }
      const auto t_exp = std::chrono::steady_clock::now();
      const int cr = deliver_lane_text(ctx, lane, lt, expand ? (size_t)lt.bytes : 0, total - hlen, staging, rs_full.head, rs_full.tail, text + hlen, &copy_mu,
                                       "the compact rows of a guide");
      if (expand) expand_us.fetch_add((uint64_t)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_exp).count());
      calitas_free(staging);
      if (cr) { calitas_free(text); return cr; }
    }
    text[total] = 0;
    tsv[g] = text;
    if (tsv_bytes) tsv_bytes[g] = total;
    if (n_rows) n_rows[g] = lt.rows;
    tms[g] = lt.tm; tms[g].hit_rows = lt.rows; tms[g].hits_bytes = total;
    return CALITAS_OK;
  };
  auto failed = [&](calitas_ctx* lane, int g, int r) {
    rcs[g] = r;
    errs[g] = lane->err;
    (void)hipStreamSynchronize(lane->stream);                   // leave the lane quiet before its next guide
  };
  // (Phases -- the guides in groups of one per lane, the group's scans back to back with nothing beside them, then the group's tails side
  // by side with no scan beside them, the texts of the group before brought in meanwhile -- were tried in round 4: the scans then take
  // 1.27 instead of 2.05 ms per guide, and the 96 guides take as long as before, 249 ms.  A guide's tail is 1.3 ms of the whole chip
  // whatever runs beside it (five tails side by side: 6.6 ms); it is the tail's own kernels that have to get cheaper, not their place.
  // tools/batch_probe.py)
  // one host thread per lane: the caller drives lane 0, the context's lane threads (they live as long as the lanes: starting a thread
  // per lane and call cost ~100 us) the others
  auto lane_job = [&](size_t l_) {
    const int l = (int)l_;
    (void)hipSetDevice(ctx->device);
    calitas_ctx* lane = ctx->lanes[l];
    InFlight f;
    for (int g = l; g < n_guides; g += n_lanes) {
      if (!owned_ok[(size_t)g]) { rcs[g] = kOwnedDeclined; continue; }   // (the stretch is not one for the bins: below, one guide at a time)
      int r = queue_scan(lane, g, f);
      if (!r) r = run_tail(lane, f, lane->scan_done);
      if (!r) r = finish(lane, f);
      if (r) failed(lane, g, r);
    }
  };
  ctx->lane_threads->start((size_t)n_lanes, lane_job);
  ctx->lane_threads->guarded([&] { lane_job(0); });
  ctx->lane_threads->wait();
  if (ctx->lane_threads->threw.load()) {
    (void)hipDeviceSynchronize();
    release();
    return fail(ctx, CALITAS_EHIP, ctx->lane_threads->failure());
  }
  for (int g = 0; g < n_guides; g++) {
    if (rcs[g] == CALITAS_OK) continue;
    if (rcs[g] == CALITAS_ESTATE || rcs[g] == CALITAS_ENOMEM || rcs[g] == kOwnedDeclined) {   // a lane's buffers overflowed / did not fit / the bins declined a stretch: this guide again through calitas_search_hits (retry logic, per-contig passes, the whole-contig path of a stretch)
      int r = single(g, version, stamp);
      if (r) { release(); return r; }
      tms[g] = ctx->timing;
      continue;
    }
    ctx->err = errs[g];
    release();
    return rcs[g];
  }
  calitas_timing_t tm = batch_timing(tms);
  tm.lanes = (uint32_t)n_lanes;
  ctx->timing = tm;
  if (TUNE_GET("CALITAS_TRACE"))
    std::fprintf(stderr, "[calitas] search_hits_batch: %d guides on %d lanes, scan %.3f ms, align %.3f ms, rows expanded on the host %.3f ms (sums), call %.3f ms (%llu rows, %llu bytes)\n",
                 n_guides, n_lanes, tm.scan_kernel_ms, tm.align_kernel_ms, (double)expand_us.load() * 1e-3,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(),
                 (unsigned long long)tm.hit_rows, (unsigned long long)tm.hits_bytes);
  return CALITAS_OK;
}
