// search_lane.cpp -- the lane machinery of calitas_search_hits: one lane from its scan to finished rows (lane_rows, the binned tail),
// the small inputs queued ahead of it, the ways a lane's text reaches the host, and the child contexts and host threads that are the
// lanes.  Who cuts a call into lanes and places their texts is in search_hits.cpp / search_sequential.cpp / search_batch.cpp.
#include <algorithm>
#include <cstring>

#include "search_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

std::atomic<double> g_pass_ms[2]; // (trace only; written by the one thread that runs a sequential call's passes -- atomics: two contexts may run such calls at once, and the figures are then both calls')

// The finished text of a lane, device -> page-locked host.  Preferred: an SDMA engine through the HSA runtime (dma.hpp), after
// waiting for the lane's row kernels -- the CUs stay with the search kernels.  Otherwise the runtime's copy (a blit kernel) on the
// owner's low-priority copy stream (chunked / batch calls: one stream for all lanes) or on the lane's own stream.
void dma_open_once(calitas_ctx* owner) {
  if (owner->dma_tried) return;
  std::lock_guard<std::mutex> lk(owner->host_mu);
  if (!owner->dma_tried) {
    const char* e = TUNE_GET("CALITAS_SDMA");
    if (!(e && std::atoi(e) == 0)) owner->dma.open(owner->device);
    owner->dma_tried = true;
  }
}

// Waits for a lane's row kernels: for rows_done if the caller recorded it (other work may be queued behind it on the stream), else
// for the lane's stream.
static hipError_t rows_sync(calitas_ctx* lane, hipEvent_t rows_done) {
  return rows_done ? calitas_spin_sync(rows_done) : calitas_spin_sync(lane->stream);
}

// Once the binned rows kernel's text is complete: did it find a row whose length differs from the one its first kernel counted?
int binned_late_failed(calitas_ctx* lane) {
  if (lane->binned_late_check && lane->mbox.host && lane->mbox.host[BIN_BOX_LATE] != 0)
    return fail(lane, CALITAS_EHIP, "binned rows kernel: a row's length differs between the two kernels (internal error)");
  return CALITAS_OK;
}

int text_to_host(calitas_ctx* owner, calitas_ctx* lane, char* dst, const char* src, size_t n, std::mutex* copy_mu, double* ms_out,
                 hipEvent_t rows_done) {
  dma_open_once(owner);
  if (lane->binned_late_check && src && src == binned_host_text(lane->binned)) {   // the rows kernel wrote the text into host memory itself
    HIP_TRY(lane, rows_sync(lane, rows_done));
    g_marks.mark("rows-done");
    if (int r = binned_late_failed(lane)) return r;
    std::memcpy(dst, src, n);
    if (ms_out) *ms_out = 0;
    return CALITAS_OK;
  }
  if (owner->dma.usable()) {
    HIP_TRY(lane, rows_sync(lane, rows_done));
    g_marks.mark("rows-done");
    const auto t0 = std::chrono::steady_clock::now();
    if (int r = binned_late_failed(lane)) return r;
    if (owner->dma.copy_to_host(dst, src, n)) {
      g_marks.mark("copied");
      if (ms_out) *ms_out = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      return CALITAS_OK;
    }
    if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] SDMA copy declined (%s), using hipMemcpyAsync\n", DmaCopier::last_reason());
  }
  // a stream of its own for the copy whenever other work may be queued behind the rows on the lane's stream: the lanes of a chunked /
  // batch call, and the per-contig passes (rows_done given: the helper thread queues the next contig's kernels on ctx->stream)
  hipStream_t cs = (owner->copy_stream && (lane->parent || rows_done)) ? owner->copy_stream : lane->stream;
  if (cs != lane->stream) {
    hipEvent_t ready = rows_done;
    if (!ready) { HIP_TRY(lane, hipEventRecord(lane->rows_ready, lane->stream)); ready = lane->rows_ready; }
    std::lock_guard<std::mutex> lk(*copy_mu);
    HIP_TRY(lane, hipStreamWaitEvent(cs, ready, 0));
    HIP_TRY(lane, hipEventRecord(lane->ev[6], cs));
    HIP_TRY(lane, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, cs));
    HIP_TRY(lane, hipEventRecord(lane->ev[7], cs));
  } else {
    HIP_TRY(lane, hipEventRecord(lane->ev[6], cs));
    HIP_TRY(lane, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, cs));
    HIP_TRY(lane, hipEventRecord(lane->ev[7], cs));
  }
  HIP_TRY(lane, calitas_spin_sync(lane->ev[7]));
  if (int r = binned_late_failed(lane)) return r;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, lane->ev[6], lane->ev[7]);
  if (ms_out) *ms_out = ms;
  return CALITAS_OK;
}

// A lane's kernel times and counts added to the call's.
void add_lane_timing(calitas_timing_t& tm, const calitas_timing_t& l) {
  tm.scan_kernel_ms += l.scan_kernel_ms; tm.align_kernel_ms += l.align_kernel_ms; tm.gpu_total_ms += l.gpu_total_ms;
  tm.host_post_ms += l.host_post_ms; tm.bases_scanned += l.bases_scanned; tm.packed_bytes += l.packed_bytes;
  tm.scan_records += l.scan_records; tm.candidate_columns += l.candidate_columns; tm.raw_alignments += l.raw_alignments;
  tm.accepted_alignments += l.accepted_alignments; tm.retries += l.retries;
  tm.hits_kernel_ms += l.hits_kernel_ms; tm.hits_copy_ms += l.hits_copy_ms; tm.binned_lanes += l.binned_lanes; tm.owned_general_lanes += l.owned_general_lanes;
}

// After the text of a lane has been copied (so its rows kernel is done): did the rows kernel of the general stage object to anything?
int rows_late_check(calitas_ctx* lane, const LaneText& lt) {
  if (lt.rows_by && hits_late(lt.rows_by) != 0)
    return calitas_fail(lane, CALITAS_EHIP, "rows kernel: a row's length differs between the two kernels (internal error)");
  return CALITAS_OK;
}

// The compact rows of a lane (nbytes of `chromosome \t middle \n` in lt.d_text) become full rows at dst: the text crosses PCIe in
// pieces queued back to back on the DMA engine, and the worker pool expands what has landed while the rest is on the bus
// (post.cpp RowExpansion) -- the call's last expansion ends ~one piece after its copy instead of a whole expansion after it.
// *wrote: bytes written at dst, (size_t)-1 when the text does not hold lt.rows rows.
static int compact_rows_to_host(calitas_ctx* owner, calitas_ctx* lane, LaneText& lt, size_t nbytes, char* staging, const std::string& head,
                                const std::string& tail, char* dst, std::mutex* copy_mu, size_t* wrote, hipEvent_t rows_done) {
  *wrote = 0;
  dma_open_once(owner);
  // (pieces of a sixth of the text, 256 KB to 2 MB -- less left to do behind the last piece of a short text: 2.028 against 2.001 ms)
  size_t piece = 2u << 20;
  if (const char* e = TUNE_GET("CALITAS_COMPACT_PIECE_KB")) piece = (size_t)std::max(64, std::atoi(e)) << 10;
  const bool in_host_text = lane->binned_late_check && lt.d_text == binned_host_text(lane->binned);
  auto whole = [&]() -> int {
    int r = text_to_host(owner, lane, staging, lt.d_text, nbytes, copy_mu, &lt.tm.hits_copy_ms, rows_done);
    if (r) return r;
    *wrote = expand_rows(staging, nbytes, lt.rows, head, tail, dst, owner->pool);
    g_marks.mark("expanded");
    return CALITAS_OK;
  };
  if (!owner->dma.usable() || in_host_text || nbytes < std::min<size_t>(1u << 20, 2 * piece)) return whole();   // (a short text: one copy, then the rows)
  HIP_TRY(lane, rows_sync(lane, rows_done));
  g_marks.mark("rows-done");
  if (int r = binned_late_failed(lane)) return r;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<unsigned long long> tickets;
  if (!owner->dma.start_pieces(staging, lt.d_text, nbytes, piece, tickets)) {
    if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] SDMA copy declined (%s), using hipMemcpyAsync\n", DmaCopier::last_reason());
    return whole();
  }
  auto job = expand_rows_begin(staging, nbytes, lt.rows, head, tail, dst, owner->pool);   // the workers wake while the first piece is on the bus
  bool ok = true;
  for (size_t i = 0; i < tickets.size(); i++) {
    if (!owner->dma.finish(tickets[i])) ok = false;           // (every ticket is waited for: nothing may land in a freed block)
    if (ok) expand_rows_arrived(*job, std::min(nbytes, (i + 1) * piece));
  }
  g_marks.mark("copied");
  lt.tm.hits_copy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *wrote = expand_rows_end(*job, ok);
  g_marks.mark("expanded");
  if (!ok) return fail(lane, CALITAS_EHIP, "SDMA copy failed");
  return CALITAS_OK;
}

// A lane's finished rows brought to dst on the host, one of three ways: rows the host stages built are copied; compact rows
// (compact_bytes != 0) cross the bus into `staging` -- page-locked, that long -- and must expand to full_bytes at dst; any other text is
// copied as it is.  rows_done: as for text_to_host.  what: whose compact rows, for the message.  The time of the row stage
// (rows_stage_ms) is the caller's to ask for.
int deliver_lane_text(calitas_ctx* owner, calitas_ctx* lane, LaneText& lt, size_t compact_bytes, size_t full_bytes, char* staging, const std::string& head,
                      const std::string& tail, char* dst, std::mutex* copy_mu, const char* what, hipEvent_t rows_done) {
  if (lt.on_host) { std::memcpy(dst, lt.host_rows.data(), (size_t)lt.bytes); return CALITAS_OK; }
  if (compact_bytes) {
    size_t wrote = 0;
    int r = compact_rows_to_host(owner, lane, lt, compact_bytes, staging, head, tail, dst, copy_mu, &wrote, rows_done);
    if (r) return r;
    if ((r = rows_late_check(lane, lt)) != CALITAS_OK) return r;
    if (wrote != full_bytes) return fail(lane, CALITAS_EHIP, std::string(what) + " do not expand to the row count the device reported (internal error)");
    return CALITAS_OK;
  }
  int r = text_to_host(owner, lane, dst, lt.d_text, (size_t)lt.bytes, copy_mu, &lt.tm.hits_copy_ms, rows_done);
  if (r) return r;
  return rows_late_check(lane, lt);
}

// Kernel time of a lane's row stage once its last kernel is done.  General kernels: ev[4] .. ev[5] around hits_run.  Binned tail: no event
// sits between its kernels, so: end of the scan .. end of the rows kernel, less align_kernel + trace_kernel (by the stamps) -- the two bin
// kernels, the rows kernel and the kernel boundaries of the chain.
double rows_stage_ms(calitas_ctx* lane, const calitas_timing_t& tm) {
  float ms = 0;
  if (lane->rows_ev0 >= 0) { (void)hipEventElapsedTime(&ms, lane->ev[lane->rows_ev0], lane->ev[5]); return ms; }
  (void)hipEventElapsedTime(&ms, lane->t_scan1, lane->ev[5]);
  return std::max(0.0, (double)ms - tm.align_kernel_ms);
}

// Whether this lane's search takes the binned tail (binned.hpp): one guide on the device path, a window size the bins handle, not
// a search planned as dense (rec_hint: per-contig passes of a permissive PAM-less search would crowd every bin), and not one at least
// as permissive as the last the bins declined on this reference.
static uint64_t guide_hash(const GuideDev& g) {
  uint64_t h = 1469598103934665603ull;                       // FNV-1a over what the kernels see of the guide
  auto mix = [&](uint64_t v) { for (int k = 0; k < 8; k++) { h ^= (v >> (8 * k)) & 0xFF; h *= 1099511628211ull; } };
  mix((uint64_t)g.L); mix((uint64_t)g.n_pams); mix((uint64_t)g.pam5);
  for (int i = 0; i < g.L; i++) mix(g.qmask[i]);
  for (int p = 0; p < g.n_pams; p++) { mix(g.pam_len[p]); for (int k = 0; k < g.pam_len[p]; k++) mix(g.pam_mask[p][k]); }
  return h;
}

// binned_possible: the search is one the per-bin kernels take at all.  binned_remembered: ... but this very guide met a crowded bin on this
// context before (a property of guide x reference: it would again).  binned_wanted: both considered -- what decides a lane's tail.
static bool binned_remembered(calitas_ctx* lane, const SearchPlan& pl) {
  const calitas_ctx* own = ref_owner(lane);
  const GuideDev& g = pl.gd[0];
  return own->bin_decl_pams == g.n_pams && own->bin_decl_L == g.L && g.min_guide_score <= own->bin_decl_min_score && own->bin_decl_guide == guide_hash(g);
}

bool binned_possible(calitas_ctx* lane, const SearchPlan& pl) {
  const calitas_ctx* own = ref_owner(lane);
  if (!pl.bin_shift || pl.n_bins == 0 || pl.n_guides != 1 || pl.rec_hint != 0 || pl.general_tail) return false;
  if (!pl.owned && (pl.gw_lo != 0 || pl.gw_hi != ~0ull)) return false;   // (a window range of calitas_search: alignment records, no rows)
  if (TUNE_GET("CALITAS_HOST_FILTER") || TUNE_GET("CALITAS_HOST_HITS")) return false;
  // Which tail by default: the per-bin kernels wherever a call is one pass or two ranges (references up to 2 Gb: a rank's share of a
  // genome on 2-8 GPUs, a bacterial genome) -- 0.58 against 0.62 ms for an eighth of the hg38-sized genome, 0.164 against 0.190 ms for
  // an E. coli-sized one.  A call cut into three ranges (the whole hg38-sized genome on one GPU) is bound by its scans, and those
  // lose more to the per-bin kernels running beside them (many short waves) than the last range's tail gains: 2.39 ms per pass on
  // the general kernels against 2.45-2.53 (tools/sweep_lanes.py, profiles/r03_*).  The last range's tail has the chip to itself, and
  // since the leading ranges' rows cross PCIe compact (round 4) it ends the call: per-bin there, 2.15 / 2.23 / 2.17 against
  // 2.18 / 2.26 / 2.29 ms (three boxes, tools/sweep_env.py CALITAS_BINNED - last).  CALITAS_BINNED=1 / 0 / last force a choice.
  bool want = !pl.three_ranges || pl.owned || pl.last_range;   // (a stretch that cuts a contig: only the bins can own it)
  if (const char* e = TUNE_GET("CALITAS_BINNED")) {
    if (std::strcmp(e, "last") == 0) want = !pl.narrow_tail;
    else want = std::atoi(e) != 0;
  }
  if (!want) return false;
  if (pl.p.max_overlap < 1 || own->ref.contigs.size() >= (1u << 18) - 1) return false;
  if (pl.model && (pl.model->top_k || pl.model->regions) && (uint64_t)pl.n_bins * BIN_ROWS > 0x7FFFFFFEull) return false;   // (a top call: more ranks than a key holds)
  return true;
}

static bool binned_wanted(calitas_ctx* lane, const SearchPlan& pl) { return binned_possible(lane, pl) && !binned_remembered(lane, pl); }

// The per-call constants of a lane's row stage -- and the cleared scratch of the bins when the lane takes the binned tail --, queued on
// its stream ahead of its kernels (callers that queue a wait for a scan on that stream do this first).
hipError_t queue_row_constants(calitas_ctx* lane, const SearchPlan& pl, const RowStrings& rs) {
  hipError_t e = hits_prepare(&lane->hits, rs, lane->stream);
  if (e == hipSuccess && binned_wanted(lane, pl)) e = binned_prepare(&lane->binned, pl.n_bins, lane->stream);
  return e;
}

// Everything small a lane's search needs on the device in one launch (kernels.hpp, LaneSetupArgs): guide constants, cleared counters,
// and -- rs given -- what queue_row_constants would queue (constant row strings, the row stage's counts, the bins' scratch).  Returns
// false when the search does not fit that form (several guides, very long parameter strings, CALITAS_LANE_SETUP=0): the caller queues
// the separate commands then (*done = false).
int queue_lane_setup(calitas_ctx* lane, const SearchPlan& pl, const RowStrings* rs, hipStream_t stream, bool* done, bool with_scan_inputs) {
  *done = false;
  if (pl.n_guides != 1) return CALITAS_OK;
  if (const char* e = TUNE_GET("CALITAS_LANE_SETUP")) if (std::atoi(e) == 0) return CALITAS_OK;
  LaneSetupArgs a{};
  if (rs) {
    HitsSetup hs{};
    HIP_TRY(lane, hits_prepare_host(&lane->hits, *rs, &hs));
    if (hs.blob_bytes > LANE_SETUP_BLOB) {                      // (the strings are assembled: bring them over the usual way)
      HIP_TRY(lane, hits_prepare(&lane->hits, *rs, stream));
    } else {
      std::memcpy(a.blob, hs.blob, hs.blob_bytes);
      a.blob_bytes = hs.blob_bytes; a.d_blob = hs.d_blob; a.d_row_counts = hs.d_counts;
    }
    if (binned_wanted(lane, pl)) {
      void* clear = nullptr;
      size_t bytes = 0;
      HIP_TRY(lane, binned_prepare_host(&lane->binned, pl.n_bins, &clear, &bytes));
      if (bytes > 0xFFFFFFF0u) HIP_TRY(lane, hipMemsetAsync(clear, 0, bytes, stream));
      else { a.clear = static_cast<uint4*>(clear); a.clear_bytes = (uint32_t)bytes; }
    }
  }
  if (with_scan_inputs) { a.guide = pl.gd[0]; a.d_guides = lane->d_guides; a.d_counters = lane->d_counters; }
  HIP_TRY(lane, launch_lane_setup(a, stream));
  g_marks.mark("lane-setup");
  *done = true;
  return CALITAS_OK;
}

// What the row stage of either tail needs besides the plan: the longest PAM, the widest hit in reference bases, the reference as the row
// kernels address it, and the contig names on the device (sent again when the reference has changed).
static int longest_pam(const GuideHost& gh) {
  int max_pam = 0;
  for (auto& q : gh.pams) max_pam = std::max<int>(max_pam, (int)q.size());
  return max_pam;
}
static int widest_hit(const SearchPlan& pl, int max_pam) { return pl.gd[0].span + 1 + pl.p.max_gaps_between_guide_and_pam + max_pam; }
static HitsRef hits_ref(const calitas_ctx* own) {
  return HitsRef{own->d_codes, own->d_mask, own->d_runs, (int64_t)own->ref.runs.size(), own->d_contigs, (int)own->ref.contigs.size()};
}
static int ensure_hit_names(calitas_ctx* lane) {
  const calitas_ctx* own = ref_owner(lane);
  if (lane->hits_names_serial == own->ref_serial) return CALITAS_OK;
  HIP_TRY(lane, hits_set_names(&lane->hits, own->ref.names, lane->stream));
  lane->hits_names_serial = own->ref_serial;
  return CALITAS_OK;
}

// The binned tail of one lane: scan (unless queued by the caller) -> align_kernel -> trace_kernel (alignments into the bins as well)
// -> bin_hits_kernel -> bin_rows_kernel, ONE host round trip (the rows kernel posts counters, rows, bytes and flags as it starts).
// prepared: the caller queued hits_prepare and binned_prepare on the lane's stream already, ahead of its wait for the scan.
// *declined: a bin was crowded / a repeat outran the halo / a lane buffer overflowed: nothing is lost, the general kernels take over.
static int lane_rows_binned(calitas_ctx* lane, const SearchPlan& pl, bool prelaunched, const RowStrings& rs, LaneText& lt, bool prepared,
                            bool* declined, const LaneDest* dest, uint32_t* decline_flags) {
  if (decline_flags) *decline_flags = 0;
  calitas_ctx* own = ref_owner(lane);
  const PackedRef& ref = own->ref;
  const calitas_params_t& p = pl.p;
  const GuideHost& gh = pl.gh[0];
  *declined = false;
  HIP_TRY(lane, hipSetDevice(lane->device));
  if (!prelaunched) {
    int rc = lane_prepare(lane, pl);
    if (rc) return rc;
    rc = ensure_window_table(lane, pl, lane->stream);
    if (rc) return rc;
  }
  if (!prelaunched) {
    // one launch for everything small the lane needs (guide constants, cleared counters, row constants, the bins' scratch), then the scan
    bool one = false;
    int rc = prepared ? CALITAS_OK : queue_lane_setup(lane, pl, &rs, lane->stream, &one);
    if (rc) return rc;
    if (one) prepared = true;
    rc = launch_scan_stage(lane, pl, lane->stream, one);
    if (rc) return rc;
  }
  if (!prepared) HIP_TRY(lane, queue_row_constants(lane, pl, rs));
  { int rc = ensure_hit_names(lane); if (rc) return rc; }
  const BinnedGeometry geo{own->d_bin_base, own->d_bin_contig, (int)ref.contigs.size(), pl.bin_first, pl.n_bins, (uint32_t)pl.bin_shift};
  const BinnedParams bp{p.window_size, pl.step, pl.max_total, p.max_overlap, widest_hit(pl, longest_pam(gh)), pl.own_lo, pl.own_hi};
  const HitsRef hr = hits_ref(own);
  ScanArgs sa; AlignArgs aa;
  fill_kernel_args(lane, pl, sa, aa);
  binned_fill_align_args(lane->binned, geo, aa);
  // (no events on these dispatches: each would hold back the kernel behind it by ~5 us; the kernels stamp the device's wall clock instead)
  HIP_TRY(lane, launch_align_trace(pl, aa, lane->stream, nullptr));
  const BinnedCall bc{lane->binned, &lane->hits, geo, hr, lane->d_raw, lane->d_guides, own->d_win_base, own->d_win, bp, lane->d_counters, lane->stream, &lane->mbox};
  HIP_TRY(lane, binned_run(bc, nullptr, nullptr, lane->ev[5], dest == nullptr && !pl.counts));
  char* host_dst = nullptr;
  uint64_t host_dst_cap = 0;
  if (pl.counts) {
    // the table instead of rows: bin_counts_kernel where the rows kernel would go, with the same post behind it
    const ScoreCall sc = pl.model ? score_call(*pl.model, pl.gh[0]) : ScoreCall{};
    HIP_TRY(lane, binned_counts(bc, lane->ev[5], pl.cshape, pl.model ? &sc : nullptr));
  } else if (dest) {
    // the rows kernel goes out once the text's final place is known (the byte counts of the ranges before this one: their row kernels
    // have started by then) and writes there itself -- no copy behind it
    if (!dest->get(&host_dst, &host_dst_cap)) { host_dst = nullptr; host_dst_cap = 0; }
    HIP_TRY(lane, binned_rows(bc, lane->ev[5], host_dst, host_dst_cap));
  }
  lane->rows_ev0 = -1;                                       // (the row stage's time: binned_rows_ms)
  g_marks.mark("queued-binned");
  HIP_TRY(lane, mailbox_wait(lane->mbox, lane->stream));
  g_marks.mark("binned-counts");
  for (int k = 0; k < 8; k++) lane->h_counters[k] = lane->mbox.host[BIN_BOX_COUNTERS + k];
  lane->align_ms_by_stamps = binned_stamp_ms(lane->binned, lane->mbox, 0, 1);                    // align_kernel + trace_kernel
  const uint32_t n_rec = lane->h_counters[0], n_raw = lane->h_counters[1], n_items = lane->h_counters[3];
  if (lane->h_counters[2] != 0) return fail(lane, CALITAS_EHIP, "aligner kernel reported an inconsistent traceback (internal error)");
  uint32_t flags = lane->mbox.host[BIN_BOX_FLAGS];
  const bool overflow = n_rec > lane->rec_cap || n_raw > lane->raw_cap || n_items > lane->item_cap;
  if (overflow || (flags & ~BIN_FLAG_TEXT)) {
    if (!overflow) {   // a property of this search on this reference: remember it
      own->bin_decl_L = pl.gd[0].L; own->bin_decl_pams = pl.gd[0].n_pams; own->bin_decl_min_score = pl.gd[0].min_guide_score;
      own->bin_decl_guide = guide_hash(pl.gd[0]);
      if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] binned tail declined (flags %u): finishing on the general kernels\n", flags);
    }
    HIP_TRY(lane, calitas_spin_sync(lane->stream));          // the rows kernel returns at once; nothing of it may linger over the retry
    *declined = true;
    if (decline_flags) *decline_flags = overflow ? ~0u : (flags & ~BIN_FLAG_TEXT);
    return CALITAS_OK;
  }
  uint64_t bytes = (uint64_t)lane->mbox.host[BIN_BOX_BYTES] | ((uint64_t)lane->mbox.host[BIN_BOX_BYTES + 1] << 32);
  if (pl.counts) {                                           // the table arrived ahead of the post
    const uint64_t* table = binned_counts_table(lane->hits);
    const bool regions = pl.model && pl.model->regions;
    const uint32_t n_classes = regions ? pl.model->regions->n_classes : 1u;
    ScoreWords rw;                                           // a regions call: the classes' tables, folded into the one every call returns
    if (!regions) lt.counts.assign(table, table + pl.cshape.cells());
    else if (!regions_from_words(table, pl.cshape.cells(), n_classes, pl.model->top_k, lt.counts, rw))
      return fail(lane, CALITAS_EHIP, "binned regions kernel: a class's table does not add up to its hits (internal error)");
    uint64_t sum = 0;
    for (uint64_t v : lt.counts) sum += v;
    if (sum != lane->mbox.host[BIN_BOX_ROWS]) return fail(lane, CALITAS_EHIP, "binned counts kernel: the table does not add up to the bins' kept hits (internal error)");
    if (regions) {
      lt.score = rw;
      if (table[(size_t)pl.cshape.cells() * n_classes + 3] != sum) return fail(lane, CALITAS_EHIP, "binned regions kernel: the hits it scored are not the hits it counted (internal error)");
    } else if (pl.model) {                                   // ... and so did the four words behind its cells
      const uint64_t* w = table + pl.cshape.cells();
      lt.score = ScoreWords{w[0], w[1], w[2], TopList(), RegionWords()};
      if (pl.model->top_k) lt.score.top = top_from_words(w + SCORE_WORDS, pl.model->top_k);
      if (w[3] != sum) return fail(lane, CALITAS_EHIP, "binned scores kernel: the hits it scored are not the hits it counted (internal error)");
    }
  }
  if (flags & BIN_FLAG_TEXT) {                               // the text buffer was a guess: grow it, the rows kernel once more
    HIP_TRY(lane, binned_rerun_rows(bc, bytes, lane->ev[5]));
    HIP_TRY(lane, mailbox_wait(lane->mbox, lane->stream));
    flags = lane->mbox.host[BIN_BOX_FLAGS];
    if (flags) return fail(lane, CALITAS_EHIP, "binned rows kernel: flags " + std::to_string(flags) + " after the text buffer was grown (internal error)");
  }
  calitas_timing_t tm{};
  tm.bases_scanned = pl.bases; tm.packed_bytes = (pl.bases + 3) / 4;
  tm.scan_records = n_rec; tm.raw_alignments = n_raw; tm.candidate_columns = lane->h_counters[4];
  tm.accepted_alignments = lane->mbox.host[BIN_BOX_ACCEPTED];
  if (TUNE_GET("CALITAS_TRACE"))
    std::fprintf(stderr, "[calitas] binned tail: %u bins, %u of them by a whole wave, %u rows, %llu bytes\n", pl.n_bins, (unsigned)lane->mbox.host[BIN_BOX_COMPLEX],
                 (unsigned)lane->mbox.host[BIN_BOX_ROWS], (unsigned long long)bytes);
  {                                                          // scan: its events; the kernels behind it: their stamps
    float ms = 0;
    (void)hipEventElapsedTime(&ms, lane->t_scan0, lane->t_scan1); tm.scan_kernel_ms = ms;
    tm.align_kernel_ms = lane->align_ms_by_stamps;
    tm.gpu_total_ms = tm.scan_kernel_ms + binned_stamp_ms(lane->binned, lane->mbox, 0, 2);       // ... + the bin kernels, up to the start of the rows kernel
  }
  tm.binned_lanes = 1;
  lane->timing = tm;
  lt.tm = tm;
  // (a short text is already on its way into the lane's page-locked buffer: text_to_host only waits for the kernel)
  if (pl.counts) lt.d_text = nullptr;
  else if (host_dst) { lt.in_place = bytes <= host_dst_cap; lt.d_text = lt.in_place ? host_dst : binned_text(lane->hits); }
  else lt.d_text = bytes <= binned_host_cap(lane->binned) ? binned_host_text(lane->binned) : binned_text(lane->hits);
  lt.bytes = bytes; lt.rows = lane->mbox.host[BIN_BOX_ROWS];
  lane->binned_late_check = !pl.counts;
  return CALITAS_OK;
}

// One lane from the scan stage (queued here, or already queued by the caller) to its finished rows.
// hits_prepared: the caller queued hits_prepare on the lane's stream already -- *before* the stream's wait for the scan, so that
// the constants are in place while the scan runs instead of sitting between the end of the scan and align_kernel.
int lane_rows(calitas_ctx* lane, const SearchPlan& pl, bool prelaunched, const RowStrings& rs, const std::string& guide_id,
              const std::string& version, const std::string& stamp, LaneText& lt, bool hits_prepared, const LaneDest* dest, const HitsExtSource* ext_source,
              int ext_contig) {
  calitas_ctx* own = ref_owner(lane);
  const PackedRef& ref = own->ref;
  const calitas_params_t& p = pl.p;
  const GuideHost& gh = pl.gh[0];
  DeviceSel dev;
  calitas_aln_t* alns = nullptr;
  uint64_t n_alns = 0;
  bool resume = false;
  lane->binned_late_check = false;
  // A stretch (SearchPlan::owned) is the bins' to decide.  Where one of its bins is crowded -- the guide meets a repeat: more alignments
  // than a wave holds -- the general kernels finish it from the same alignments and keep the rows the stretch owns (HitsOwn): exact
  // unless a chain of overlapping hits reaches from the edge of the aligned context into the stretch, which they detect (HITS_FLAG_HALO)
  // and which the bins' own halo flag says as well; then, and for anything else, the caller searches the touched contigs whole.
  bool own_general = false;
  if (pl.owned && !binned_possible(lane, pl)) return kOwnedDeclined;   // (no bins for this window size / forced off: the caller's whole-contig path)
  if (pl.owned && binned_remembered(lane, pl)) {                        // this guide crowded a bin here before: the general kernels at once
    if (TUNE_GET("CALITAS_OWN_GENERAL_OFF")) return kOwnedDeclined;
    own_general = true;
  } else if (binned_wanted(lane, pl)) {
    bool declined = false;
    uint32_t why = 0;
    int rc = lane_rows_binned(lane, pl, prelaunched, rs, lt, hits_prepared, &declined, dest, &why);
    if (rc || !declined) return rc;
    if (pl.owned) {
      if (why != BIN_FLAG_CROWDED || TUNE_GET("CALITAS_OWN_GENERAL_OFF")) return kOwnedDeclined;
      own_general = true;
    }
    // the bins declined: the raw alignments are where the general kernels expect them, the lane's counters in h_counters
    resume = true;
    hits_prepared = false;                                   // binned_run consumed the row constants
  }
  if (!hits_prepared && !TUNE_GET("CALITAS_HOST_HITS")) HIP_TRY(lane, hits_prepare(&lane->hits, rs, lane->stream));   // ahead of the lane's kernels
  const auto t_pass0 = std::chrono::steady_clock::now();
  int rc = search_run(lane, pl, &alns, &n_alns, &dev, prelaunched, resume);
  if (rc) return rc;
  lt.tm = lane->timing;
  if (own_general && !dev.valid) { calitas_free(alns); return kOwnedDeclined; }
  const HitsExt* ext = nullptr;             // the caller's own hits of this contig: asked for now, the search kernels of the pass are behind us
  const auto t_pass1 = std::chrono::steady_clock::now();
  if (ext_source && ext_source->get(ext_contig, &ext) != 0) { calitas_free(alns); return kExtDeclined; }
  if (ext_source) {                         // (CALITAS_TRACE of the per-contig passes: the search kernels' part of a pass, and its wait for the caller's hits)
    const auto t_pass2 = std::chrono::steady_clock::now();
    g_pass_ms[0].store(g_pass_ms[0].load(std::memory_order_relaxed) + std::chrono::duration<double, std::milli>(t_pass1 - t_pass0).count(), std::memory_order_relaxed);
    g_pass_ms[1].store(g_pass_ms[1].load(std::memory_order_relaxed) + std::chrono::duration<double, std::milli>(t_pass2 - t_pass1).count(), std::memory_order_relaxed);
  }
  if (ext && !dev.valid && n_alns == 0) {   // nothing of the reference's own on this contig: the row stage still places the caller's hits
    dev.valid = true; dev.d_final = nullptr; dev.n_sel = 0; dev.crowded = true;
  }
  if (ext && (!dev.valid || TUNE_GET("CALITAS_HOST_HITS"))) { calitas_free(alns); return kExtDeclined; }
  if (dev.valid && !TUNE_GET("CALITAS_HOST_HITS")) {
    // removeOverlaps, ReferenceHit.sort and the rows on the device (hits.hip); only text crosses PCIe
    const int max_pam = longest_pam(gh);
    const int score_hi = pl.sc.match * (int)gh.protospacer.size() + pl.sc.pam_match * max_pam;
    const int worst_gap = std::max(iabs(pl.sc.query_gap), std::max(iabs(pl.sc.target_gap), iabs(pl.sc.mismatch)));
    const int score_lo = pl.gd[0].min_guide_score - iabs(pl.sc.pam_mismatch) * max_pam - worst_gap * (p.max_gaps_between_guide_and_pam + 1);
    if (hits_supported(ref.contigs.size(), p.max_overlap, score_lo, score_hi)) {
      if ((rc = ensure_hit_names(lane)) != CALITAS_OK) return rc;
      const HitsRef hr = hits_ref(own);
      HitsResult res{};
      HitsOwn ho;
      if (own_general) {
        // from where on every hit that could overlap is known: the first aligned window's start + a window (hits of the windows left of it
        // end before that) + the longest hit; a context that starts with its contig knows everything
        ho.lo = pl.own_lo; ho.hi = pl.own_hi;
        const std::vector<uint64_t> wb = window_prefix(ref, pl.step);
        const uint64_t c = (uint64_t)window_contig(wb, pl.gw_lo), pos = (pl.gw_lo - wb[c]) * (uint64_t)pl.step;
        ho.safe = pos == 0 ? (c << 32) : ((c << 32) | (pos + (uint64_t)p.window_size + CALITAS_MAX_OPS));
      }
      HIP_TRY(lane, hipEventRecord(lane->ev[4], lane->stream));
      lane->rows_ev0 = 4;
      HitsRunCall hc{};
      hc.ref = hr; hc.d_final = dev.d_final; hc.n = dev.n_sel; hc.d_guides = lane->d_guides; hc.d_win_base = own->d_win_base; hc.d_win = own->d_win;
      hc.strings = &rs; hc.max_overlap = p.max_overlap; hc.score_hi = score_hi; hc.max_ops = widest_hit(pl, max_pam);
      hc.window_reach = dev.crowded ? 0u : (uint32_t)((p.window_size + pl.step - 1) / pl.step); hc.stream = lane->stream;
      hc.ext = ext; hc.own = own_general ? &ho : nullptr; hc.counts = pl.counts ? &pl.cshape : nullptr;
      const ScoreCall sc = pl.model ? score_call(*pl.model, pl.gh[0]) : ScoreCall{};
      hc.score = pl.counts && pl.model ? &sc : nullptr;
      HIP_TRY(lane, hits_run(&lane->hits, hc, &res));
      HIP_TRY(lane, hipEventRecord(lane->ev[5], lane->stream));
      g_marks.mark("rows-queued");
      kernel_times(lane, lt.tm);          // while out_kernel runs
      if (pl.counts && (res.flags & HITS_FLAG_EXTENT)) return fail(lane, CALITAS_EHIP, "a hit lies outside the extents of the counts table (internal error)");
      if (res.flags == 0 && pl.counts) {
        const bool regions = pl.model && pl.model->regions;
        const uint32_t n_classes = regions ? pl.model->regions->n_classes : 1u;
        ScoreWords rw;
        if (!regions) lt.counts.assign(res.counts, res.counts + pl.cshape.cells());
        else if (!regions_from_words(res.counts, pl.cshape.cells(), n_classes, pl.model->top_k, lt.counts, rw))
          return fail(lane, CALITAS_EHIP, "regions kernel: a class's table does not add up to its hits (internal error)");
        uint64_t sum = 0;
        for (uint64_t v : lt.counts) sum += v;
        if (sum != res.n_rows) return fail(lane, CALITAS_EHIP, "counts kernel: the table does not add up to the kept hits (internal error)");
        if (regions) {
          lt.score = rw;
          if (res.counts[(size_t)pl.cshape.cells() * n_classes + 3] != sum) return fail(lane, CALITAS_EHIP, "regions kernel: the hits it scored are not the hits it counted (internal error)");
        } else if (pl.model) {
          const uint64_t* w = res.counts + pl.cshape.cells();
          lt.score = ScoreWords{w[0], w[1], w[2], TopList(), RegionWords()};
          if (pl.model->top_k) lt.score.top = top_from_words(w + SCORE_WORDS, pl.model->top_k);
          if (w[3] != sum) return fail(lane, CALITAS_EHIP, "scores kernel: the hits it scored are not the hits it counted (internal error)");
        }
        lt.rows = res.n_rows;
        if (own_general) lt.tm.owned_general_lanes = 1;
        return CALITAS_OK;
      }
      if (res.flags == 0) {
        lt.d_text = res.d_text; lt.bytes = res.text_bytes; lt.rows = res.n_rows; lt.rows_by = lane->hits;
        if (res.ext_place) { lt.ext = ext; lt.ext_place = res.ext_place; }
        if (own_general) lt.tm.owned_general_lanes = 1;
        return CALITAS_OK;
      }
      if (own_general) return kOwnedDeclined;
      if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] search_hits: device rows declined (flags %u), finishing on the host\n", res.flags);
    }
    if (ext) return kExtDeclined;       // (a contig without hits of the caller's needs no merge: any tail writes its text)
  }
  // host tail: the same stages as calitas_hits_tsv (one lane at a time: they share the owner's worker pool)
  std::lock_guard<std::mutex> host_lock(own->host_mu);
  if (dev.valid) {
    kernel_times(lane, lt.tm);
    rc = convert_selected(lane, dev.d_final, dev.n_sel, pl.gh, p, pl.step, &alns);
    if (rc) return rc;
    n_alns = dev.n_sel;
  }
  uint64_t rows = 0;
  if (pl.counts) {                                           // the host stage of calitas_hits_counts
    lt.counts.assign(pl.cshape.cells(), 0);
    lt.score.top.k = pl.model ? pl.model->top_k : 0;
    const std::string e = pl.model && pl.model->regions
                              ? hits_regions(ref, gh, p, *pl.model, alns, n_alns, pl.cshape.n_mm, pl.cshape.n_gaps, pl.cshape.n_pam, lt.counts.data(), &rows,
                                             &lt.score.perfect, &lt.score.sum_q32, &lt.score.max_q32, &lt.score.top, &lt.score.reg, own->pool)
                          : pl.model ? hits_top(ref, gh, p, *pl.model, alns, n_alns, pl.cshape.n_mm, pl.cshape.n_gaps, pl.cshape.n_pam, lt.counts.data(), &rows,
                                              &lt.score.perfect, &lt.score.sum_q32, &lt.score.max_q32, &lt.score.top, own->pool)
                                   : hits_counts(ref, gh, p, alns, n_alns, pl.cshape.n_mm, pl.cshape.n_gaps, pl.cshape.n_pam, lt.counts.data(), &rows, own->pool);
    calitas_free(alns);
    if (!e.empty()) return fail(lane, CALITAS_EHIP, e);
    lt.on_host = true;
    lt.rows = rows;
    return CALITAS_OK;
  }
  char* text = hits_tsv(ref, gh, guide_id, p, alns, n_alns, version, stamp, &rows, own->pool, out_alloc, nullptr, 0);
  calitas_free(alns);
  if (!text) return fail(lane, CALITAS_EINVAL, "out of memory");
  lt.on_host = true;
  lt.host_rows.assign(text + rs.header.size());
  calitas_free(text);
  lt.bytes = lt.host_rows.size(); lt.rows = rows;
  return CALITAS_OK;
}

// Child contexts of a chunked search: own stream (high priority), buffers and scratch; the parent's reference.
int ensure_lanes(calitas_ctx* ctx, size_t k) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  // (Reserving CUs for the lanes with hipExtStreamCreateWithCUMask on the scan stream was tried: 8 of 256 CUs masked out cost the
  // scan 9 %, 32 cost 80 %, and the lanes' small kernels did not get faster.)
  if (!ctx->scan_stream) HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->scan_stream, hipStreamNonBlocking, least));   // (two levels on this device: 0 and -1)
  // The runtime performs these device-to-host copies with a blit kernel (rocprofv3: __amd_rocclr_copyBuffer) that shares the CUs
  // with everything else.  On a high-priority stream it held up the other lane's small kernels for the whole copy (rocprofv3
  // timeline: a 5 us merge pass took 370 us); on the lowest priority the lanes' kernels get their slots first.  A copy kernel of
  // our own with a small grid reached the same 55 GB/s but slowed the other lane more, so the runtime's copy stays.
  if (!ctx->copy_stream) HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->copy_stream, hipStreamNonBlocking, least));
  if (!ctx->lane_threads) ctx->lane_threads = new LaneThreads();
  ctx->lane_threads->ensure(k);
  while (ctx->lanes.size() < k) {
    calitas_ctx* c = new calitas_ctx();
    c->device = ctx->device; c->parent = ctx;
    bool ok = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, greatest) == hipSuccess;
    for (int i = 0; i < 8; i++) ok = ok && hipEventCreateWithFlags(&c->ev[i], i < 6 ? hipEventReleaseToDevice : hipEventDefault) == hipSuccess;   // as in calitas_create
    ok = ok && hipEventCreateWithFlags(&c->scan_done, hipEventReleaseToDevice) == hipSuccess;   // timed: it also brackets the scan
    ok = ok && hipEventCreateWithFlags(&c->rows_ready, hipEventDisableTiming | hipEventReleaseToDevice) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->inputs_ready, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_counters, 8 * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&c->h_counters, 8 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_guides, sizeof(GuideDev) * MAX_GUIDES) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&c->h_guides, sizeof(GuideDev) * MAX_GUIDES, hipHostMallocDefault) == hipSuccess;
    ctx->lanes.push_back(c);
    if (!ok) { calitas_destroy_lanes(ctx); return fail(ctx, CALITAS_EHIP, "could not create a search lane"); }
  }
  return CALITAS_OK;
}

// Frees every scratch buffer of the context and its lanes (not the reference): the state a memory-bounded retry starts from.
void release_scratch(calitas_ctx* ctx) {
  (void)hipDeviceSynchronize();
  calitas_destroy_lanes(ctx);
  (void)hipFree(ctx->d_recs); (void)hipFree(ctx->d_raw); (void)hipFree(ctx->d_slab); (void)hipFree(ctx->d_items);
  ctx->d_recs = nullptr; ctx->d_raw = nullptr; ctx->d_slab = nullptr; ctx->d_items = nullptr;
  ctx->rec_cap = ctx->raw_cap = ctx->item_cap = 0; ctx->slab_cap = 0;
  if (ctx->h_raw) { (void)hipHostFree(ctx->h_raw); ctx->h_raw = nullptr; ctx->h_raw_cap = 0; }
  select_destroy(ctx->select); ctx->select = nullptr;
  hits_destroy(ctx->hits); ctx->hits = nullptr; ctx->hits_names_serial = ~0ull;
  hits_destroy(ctx->hits_alt); ctx->hits_alt = nullptr; ctx->hits_alt_names_serial = ~0ull;
  binned_destroy(ctx->binned); ctx->binned = nullptr;
}

}  // namespace calitas

// ctx->side: a child context with a stream and buffers of its own, the parent's reference and worker pool (see ctx.hpp).
int calitas_side_context(calitas_ctx* ctx, calitas_ctx** side, int which) {
  *side = nullptr;
  if (ctx->device < 0) return fail(ctx, CALITAS_ENODEV, "host-only context");
  calitas_ctx*& slot = which ? ctx->side2 : ctx->side;
  if (!slot) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    calitas_ctx* c = new calitas_ctx();
    c->device = ctx->device; c->parent = ctx;
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 8; i++) ok = ok && hipEventCreateWithFlags(&c->ev[i], i < 6 ? hipEventReleaseToDevice : hipEventDefault) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_counters, 8 * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&c->h_counters, 8 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_guides, sizeof(GuideDev) * MAX_GUIDES) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&c->h_guides, sizeof(GuideDev) * MAX_GUIDES, hipHostMallocDefault) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); calitas_destroy(c); return fail(ctx, CALITAS_EHIP, "could not create the side context"); }
    slot = c;
  }
  *side = slot;
  return CALITAS_OK;
}

void calitas_destroy_lanes(calitas_ctx* ctx) {
  delete ctx->lane_threads; ctx->lane_threads = nullptr;
  for (calitas_ctx* c : ctx->lanes) calitas_destroy(c);
  ctx->lanes.clear();
  if (ctx->scan_stream) { (void)hipStreamDestroy(ctx->scan_stream); ctx->scan_stream = nullptr; }
  if (ctx->copy_stream) { (void)hipStreamDestroy(ctx->copy_stream); ctx->copy_stream = nullptr; }
}
