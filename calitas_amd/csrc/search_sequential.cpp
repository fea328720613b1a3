// search_sequential.cpp -- calitas_search_hits as one pass per contig, for a search that does not fit the device in one pass (and for
// the variant branch, which brings hits of its own into every contig's row stage).  The decision to come here is in search_hits.cpp.
#include <algorithm>
#include <cstring>

#include "search_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

namespace {
// A pass whose device stages are queued, until its text is on the host.
struct Slot { LaneText lt; int rc = CALITAS_OK; double ms = 0; hipEvent_t rows_done = nullptr; int state = 0; };   // 0 free, 1 rows queued
// What the caller's thread and the helper thread that runs the passes share.
struct Passes {
  std::vector<SearchPlan> plans;
  std::vector<int> contig;
  Slot slots[2];
  std::mutex mu;
  std::condition_variable cv;
  bool abort = false;
  void release(Slot& sl) {
    { std::lock_guard<std::mutex> lk(mu); sl.state = 0; }
    cv.notify_all();
  }
};
// The text of the call as it grows (null with a sink), and the page-locked bounce buffer its pieces come through.
struct SeqText {
  char* text = nullptr;
  size_t hlen = 0, total = 0;
  char* bounce = nullptr;
  size_t bounce_cap = 0;
  std::mutex copy_mu;
  double ms_grow = 0, ms_land = 0; // this thread: the text block grown, the texts copied from the bounce buffer to their place
  bool bounce_holds(size_t n) {
    if (n > bounce_cap) { calitas_free(bounce); bounce = (char*)calitas_out_alloc_pinned(n); bounce_cap = bounce ? n : 0; }
    return bounce != nullptr;
  }
};
}  // namespace

// The passes: one plan per selected contig.
static void plan_passes(calitas_ctx* ctx, const SearchPlan& pl, Passes& ps) {
  const PackedRef& ref = ctx->ref;
  const std::vector<uint64_t> wb = window_prefix(ref, pl.step);
  for (int c = 0; c < (int)ref.contigs.size(); c++) {
    if (pl.p.chrom_index >= 0 && pl.p.chrom_index != c) continue;
    SearchPlan q = pl;
    plan_contig_range(ctx, q, wb, c, c + 1);
    // buffers sized from the estimate that sent this search here: no retry round per contig
    if (ctx->seq_recs_per_tile > 0 && ctx->seq_pams == pl.gd[0].n_pams && ctx->seq_L == pl.gd[0].L && pl.gd[0].min_guide_score == ctx->seq_min_score)
      q.rec_hint = (uint64_t)(ctx->seq_recs_per_tile * (double)q.n_tiles) + 1;
    ps.plans.push_back(q); ps.contig.push_back(c);
  }
}

// The helper thread: the device stages of every pass, each into the slot of its turn.  ctx->hits / hits_alt take turns as the row stage's
// scratch; they are put back, as the passes left them, on every way out of the loop.
static void run_passes(calitas_ctx* ctx, Passes& ps, const HitsCall& call, const RowStrings& rs_dev, const std::string& version, const std::string& stamp) {
  (void)hipSetDevice(ctx->device);
  HitsWork* work[2] = {ctx->hits, ctx->hits_alt};
  uint64_t serial[2] = {ctx->hits_names_serial, ctx->hits_alt_names_serial};
  for (size_t i = 0; i < ps.plans.size(); i++) {
    Slot& sl = ps.slots[i & 1];
    {
      std::unique_lock<std::mutex> lk(ps.mu);
      ps.cv.wait(lk, [&] { return sl.state == 0 || ps.abort; });
      if (ps.abort) break;
    }
    ctx->hits = work[i & 1]; ctx->hits_names_serial = serial[i & 1];
    sl.lt = LaneText();
    const auto t_rows = std::chrono::steady_clock::now();
    ps.plans[i].general_tail = call.ext_source != nullptr;
    try {
      sl.rc = lane_rows(ctx, ps.plans[i], false, rs_dev, call.guide_id, version, stamp, sl.lt, false, nullptr, call.ext_source, ps.contig[i]);
    } catch (const std::exception& e) {                      // (this thread has no caller to unwind to)
      sl.rc = fail(ctx, CALITAS_EHIP, std::string("a contig pass ended with an exception: ") + e.what());
    }
    if (sl.rc == CALITAS_OK && hipEventRecord(sl.rows_done, ctx->stream) != hipSuccess) sl.rc = fail(ctx, CALITAS_EHIP, "hipEventRecord failed");
    sl.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_rows).count();
    work[i & 1] = ctx->hits; serial[i & 1] = ctx->hits_names_serial;
    {
      std::lock_guard<std::mutex> lk(ps.mu);
      sl.state = 1;
    }
    ps.cv.notify_all();
    if (sl.rc) break;
  }
  ctx->hits = work[0]; ctx->hits_names_serial = serial[0];
  ctx->hits_alt = work[1]; ctx->hits_alt_names_serial = serial[1];
}

// A contig's full rows from the device through the bounce buffer (at most 1 GB page-locked) to dst, or to the sink.
static int rows_through_bounce(calitas_ctx* ctx, const HitsCall& call, LaneText& lt, hipEvent_t rows_done, char* dst_all, SeqText& tx) {
  int rc = CALITAS_OK;
  const size_t kPiece = 1ull << 30;
  for (size_t off = 0; off < (size_t)lt.bytes && !rc; off += kPiece) {
    const size_t n = std::min(kPiece, (size_t)lt.bytes - off);
    if (!tx.bounce_holds(n)) { rc = fail(ctx, CALITAS_EINVAL, "out of memory"); break; }
    char* const bounce = tx.bounce;
    double ms = 0;
    dma_open_once(ctx);
    if (!call.sink && ctx->dma.usable() && n >= (64u << 20)) {
      // The portion crosses the bus in 32 MB pieces queued back to back on the DMA engine, and every piece goes from the bounce
      // buffer to its place while the ones behind it are still on their way (round 5: one copy, then one memcpy of the whole
      // portion, was 0.4 s on the bus + 0.4-0.5 s of memcpy into fresh pages, one after the other, per 22 GB of rows -- the
      // longest chain of a search with variants at BASELINE config 5's size).
      if (hipError_t e = calitas_spin_sync(rows_done); e != hipSuccess) { rc = fail(ctx, CALITAS_EHIP, std::string("waiting for a contig's rows: ") + hipGetErrorString(e)); break; }
      const size_t piece = 32u << 20;
      std::vector<unsigned long long> tickets;
      if (ctx->dma.start_pieces(bounce, lt.d_text + off, n, piece, tickets)) {
        char* dst = dst_all + off;
        bool ok = true;
        double ms_wait_dma = 0;
        for (size_t k = 0; k < tickets.size(); k++) {
          const auto t_w = std::chrono::steady_clock::now();
          if (!ctx->dma.finish(tickets[k])) ok = false;     // (every ticket is waited for: nothing may land in a freed block)
          ms_wait_dma += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_w).count();
          if (!ok) continue;
          const size_t b0 = k * piece, nb = std::min(piece, n - b0);
          const auto t_land = std::chrono::steady_clock::now();
          std::lock_guard<std::mutex> host_lock(ctx->host_mu);   // the helper thread's host stages (if any) use the same pool
          ctx->pool->for_blocks(nb, [&](size_t b, size_t e, int) { stream_copy(dst + b0 + b, bounce + b0 + b, e - b); });
          tx.ms_land += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_land).count();
        }
        if (!ok) { rc = fail(ctx, CALITAS_EHIP, "SDMA copy failed"); break; }
        lt.tm.hits_copy_ms += ms_wait_dma;                  // (what this thread waited for the bus; the rest of the copy hid behind the memcpy)
        continue;
      }
      if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] SDMA copy declined (%s), using one copy per portion\n", DmaCopier::last_reason());
    }
    rc = text_to_host(ctx, ctx, bounce, lt.d_text + off, n, &tx.copy_mu, &ms, rows_done);
    if (rc) break;
    lt.tm.hits_copy_ms += ms;
    if (call.sink) {
      if (call.sink(bounce, n, call.sink_user) != 0) rc = fail(ctx, CALITAS_EIO, "the text sink reported an error");
      continue;
    }
    char* dst = dst_all + off;
    const char* src = bounce;
    const auto t_land = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> host_lock(ctx->host_mu);      // the helper thread's host stages (if any) use the same pool
    ctx->pool->for_blocks(n, [&](size_t b, size_t e, int) { std::memcpy(dst + b, src + b, e - b); });
    tx.ms_land += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_land).count();
  }
  return rc;
}

// One contig's rows (lt.bytes != 0) to their place behind the text so far -- or to the sink --, whichever way they come: compact over the
// bus and expanded, built by the host stages, straight into the caller's page-locked buffer, or through the bounce buffer.
// pass / n_passes and bases_done (this contig included): for the caller's buffer's message and the growth of the library's block.
static int land_contig(calitas_ctx* ctx, const HitsCall& call, const SearchPlan& pl, const RowStrings& rs, bool compact, const std::string& cut_head,
                       Slot& sl, size_t pass, size_t n_passes, uint64_t bases_done, SeqText& tx) {
  const PackedRef& ref = ctx->ref;
  LaneText& lt = sl.lt;
  int rc = CALITAS_OK;
  // room for this contig, and -- extrapolating from the bases done so far -- for the rest
  const bool expand = compact && !lt.on_host;             // (rows the host stages built are whole already)
  const size_t full_bytes = expand ? (size_t)lt.bytes + (size_t)lt.rows * (cut_head.size() + rs.tail.size() - 1) : (size_t)lt.bytes;
  const double per_base = (double)(tx.total - tx.hlen + full_bytes) / (double)std::max<uint64_t>(1, bases_done);
  const size_t guess = pl.p.chrom_index >= 0 ? 0 : (size_t)(per_base * 1.05 * (double)(ref.total_bases - bases_done));
  if (call.user_dst) {
    if ((uint64_t)tx.total + full_bytes + 1 > call.user_cap)
      return fail(ctx, CALITAS_EINVAL, "the destination buffer is too small for the text (" + std::to_string(call.user_cap) + " bytes; " +
                                       std::to_string(tx.total + full_bytes + 1) + " needed after " + std::to_string(pass + 1) + " of " + std::to_string(n_passes) + " contigs)");
  } else if (!call.sink) {
    const auto t_grow = std::chrono::steady_clock::now();
    char* grown = (char*)calitas_out_grow(tx.text, tx.total, tx.total + full_bytes + 1 + guess);
    if (!grown) return fail(ctx, CALITAS_EINVAL, "out of memory");
    tx.text = grown;
    tx.ms_grow += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_grow).count();
  }
  char* const dst = tx.text + tx.total;
  if (expand) {
    // the contig's compact text over the bus in pieces into the page-locked block, the worker pool puts guide_id, protospacer and
    // the tail back while the rest is still on its way (compact_rows_to_host); the next contig's kernels run meanwhile
    if (!tx.bounce_holds((size_t)lt.bytes)) return fail(ctx, CALITAS_EINVAL, "out of memory");
    rc = deliver_lane_text(ctx, ctx, lt, (size_t)lt.bytes, full_bytes, tx.bounce, cut_head, rs.tail, dst, &tx.copy_mu, "a contig's compact rows", sl.rows_done);
    if (rc) return rc;
  } else {
    if (lt.on_host) {
      if (!call.sink) std::memcpy(dst, lt.host_rows.data(), (size_t)lt.bytes);
      else if (call.sink(lt.host_rows.data(), lt.bytes, call.sink_user) != 0) return fail(ctx, CALITAS_EIO, "the text sink reported an error");
    } else if (call.user_dst) {                       // straight to its place in the caller's page-locked buffer
      // (in portions: one copy of a whole contig's rows -- 1.7 GB for chr1 of BASELINE config 5's shape -- held up everybody else's
      // copies for 20-65 ms at a time: the variant half's aligner batches took 15 instead of 3 ms)
      const size_t kPortion = 128u << 20;
      for (size_t off = 0; off < (size_t)lt.bytes && !rc; off += kPortion) {
        double ms = 0;
        rc = text_to_host(ctx, ctx, dst + off, lt.d_text + off, std::min(kPortion, (size_t)lt.bytes - off), &tx.copy_mu, &ms, sl.rows_done);
        lt.tm.hits_copy_ms += ms;
      }
      if (rc) return rc;
      if ((rc = rows_late_check(ctx, lt)) != CALITAS_OK) return rc;
    } else {
      rc = rows_through_bounce(ctx, call, lt, sl.rows_done, dst, tx);
      if (rc) return rc;
      if ((rc = rows_late_check(ctx, lt)) != CALITAS_OK) return rc;
    }
    if (lt.ext_place) {                                 // the caller's own rows into the holes the rows kernel left for them
      if (call.sink || !lt.ext || !lt.ext->fill) return fail(ctx, CALITAS_EINVAL, "rows left to the caller, but nowhere to write them (internal error)");
      if (lt.ext->fill(lt.ext_place, dst, call.user_dst != nullptr) != 0) return fail(ctx, CALITAS_EINVAL, "the caller's rows could not be written into the text");
    }
  }
  tx.total += full_bytes;
  return CALITAS_OK;
}

// calitas_search_hits when one pass does not fit the device (a PAM-less search at max-guide-diffs 8 on a whole genome keeps 2.4 KB of
// strip per scan record and yields ~27 rows per kilobase): one pass per contig, one after the other on this context's own stream,
// every contig's text copied to the host before the next one starts; the texts are concatenated at the end (removeOverlaps groups
// and the final sort never cross a contig).
// With a sink the pieces (header, then every contig's rows in at most 1 GB portions) are handed over as they arrive instead of being
// collected: no text block at all, out.tsv stays NULL.
// call.user_dst (round 5): the text goes to user_cap bytes of the caller's -- page-locked (calitas_pin_host), so that every contig's rows
// cross the bus straight to their place: no bounce buffer, no memcpy into fresh pages (0.4-0.6 s per 22 GB of rows), out.tsv = user_dst.
int search_hits_sequential(calitas_ctx* ctx, const HitsCall& call, HitsOut& out) {
  const auto t_call = std::chrono::steady_clock::now();
  char* const user_dst = call.user_dst;
  const calitas_text_sink_t sink = call.sink;
  SearchPlan pl;
  int rc = plan_search(ctx, 1, call.guide, call.params, pl);
  if (rc) return rc;
  if (user_dst && sink) return fail(ctx, CALITAS_EINVAL, "a text sink and a destination buffer at once");
  const PackedRef& ref = ctx->ref;
  std::string version, stamp;
  calitas_default_version_and_stamp(call.aligner_version, call.time_stamp, version, stamp);
  const RowStrings rs = make_row_strings(ref, pl.gh[0], call.guide_id, pl.p, version, stamp);
  // Round 5: the per-contig texts cross PCIe compact (post.hpp) when the call builds one block and a caller's entries, if any, are
  // compact as well -- 21.8 GB of rows at BASELINE config 5's size were 0.42-0.47 s of the reference passes on the bus.  genome_build
  // stays in the rows (the variant branch's rows have one of their own); a text sink still gets whole rows as they come.
  std::string cut_head;
  bool compact = !sink && (!call.ext_source || call.ext_source->compact_rows);
  if (const char* e = TUNE_GET("CALITAS_COMPACT_ROWS")) compact = compact && std::atoi(e) != 0;
  const RowStrings rs_dev = compact ? compact_row_strings_keep_build(rs, &cut_head) : rs;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_bin_base(ctx, pl, ctx->stream);
  if (rc) return rc;
  if (!ctx->copy_stream) {   // the fallback of the SDMA copy must not share ctx->stream with the helper thread's next pass (text_to_host)
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->copy_stream, hipStreamNonBlocking, least));
  }
  // The text grows in one pageable block (realloc: pages move, bytes are not copied); every contig's rows come over PCIe into a
  // reused page-locked bounce buffer and from there into the block on the worker pool (page-locking 40+ GB of pieces and
  // concatenating them afterwards took longer than the search).
  SeqText tx;
  const size_t hlen = tx.hlen = rs.header.size();
  if (user_dst && call.user_cap < hlen + 1) return fail(ctx, CALITAS_EINVAL, "the destination buffer does not hold the header line");
  // (a block of the library's: the one the last such search's caller handed back, if it is still parked -- its pages are there)
  tx.text = sink ? nullptr : user_dst ? user_dst : (char*)calitas_out_take_big(hlen + (64u << 20));
  if (!sink && !tx.text) tx.text = (char*)calitas_out_grow(nullptr, 0, hlen + (64u << 20));
  if (!sink && !tx.text) return fail(ctx, CALITAS_EINVAL, "out of memory");
  if (tx.text) std::memcpy(tx.text, rs.header.data(), hlen);
  else if (sink(rs.header.data(), hlen, call.sink_user) != 0) return fail(ctx, CALITAS_EIO, "the text sink reported an error");
  tx.total = hlen;
  auto drop = [&] { if (!user_dst) calitas_free(tx.text); calitas_free(tx.bounce); };
  calitas_timing_t tm{};
  uint64_t rows = 0;
  const int n_contigs = (int)ref.contigs.size();
  uint64_t bases_done = 0;
  double ms_rows = 0;              // inside lane_rows: kernels, their host round trips and every (re)allocation of scratch
  Passes ps;
  plan_passes(ctx, pl, ps);
  const uint32_t n_passes = (uint32_t)ps.plans.size();
  g_pass_ms[0].store(0, std::memory_order_relaxed); g_pass_ms[1].store(0, std::memory_order_relaxed);
  // Two row-stage scratch sets (ctx->hits / hits_alt) take turns: a helper thread runs the device stages of pass i+1 while this thread
  // copies the text of pass i over PCIe and hands it on -- the copy is 1.5 of the 2.7 s of a PAM-less d = 8 search on an hg38-sized
  // genome, the device stages 1.0.  The sink is only ever called from this (the caller's) thread.
  for (auto& sl : ps.slots)
    if (hipEventCreateWithFlags(&sl.rows_done, hipEventDisableTiming) != hipSuccess) {
      for (auto& s2 : ps.slots) if (s2.rows_done) (void)hipEventDestroy(s2.rows_done);
      drop();
      return fail(ctx, CALITAS_EHIP, "hipEventCreateWithFlags failed");
    }
  std::thread producer([&] { run_passes(ctx, ps, call, rs_dev, version, stamp); });
  auto stop_producer = [&] {
    { std::lock_guard<std::mutex> lk(ps.mu); ps.abort = true; }
    ps.cv.notify_all();
    producer.join();
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& sl : ps.slots) (void)hipEventDestroy(sl.rows_done);
  };
  rc = CALITAS_OK;
  for (size_t i = 0; i < ps.plans.size() && !rc; i++) {
    Slot& sl = ps.slots[i & 1];
    {
      std::unique_lock<std::mutex> lk(ps.mu);
      ps.cv.wait(lk, [&] { return sl.state == 1; });
    }
    if (sl.rc) { rc = sl.rc; break; }
    LaneText& lt = sl.lt;
    const int c = ps.contig[i];
    const bool trace_contigs = TUNE_GET("CALITAS_TRACE") && std::atoi(TUNE_GET("CALITAS_TRACE")) >= 3;
    const double ms_rows_at = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    struct Said { bool on; int c; double at; uint64_t bytes; std::chrono::steady_clock::time_point t0;
                  ~Said() { if (on) std::fprintf(stderr, "[calitas] search_hits: contig %d: rows queued at %.1f ms, %llu bytes on the host at %.1f ms\n", c, at, (unsigned long long)bytes,
                                                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); } } said{trace_contigs, c, ms_rows_at, lt.bytes, t_call};
    ms_rows += sl.ms;
    bases_done += ref.contigs[c].len;
    if (lt.bytes && (rc = land_contig(ctx, call, pl, rs, compact, cut_head, sl, i, ps.plans.size(), bases_done, tx)) != CALITAS_OK) break;
    rows += lt.rows;
    add_lane_timing(tm, lt.tm);
    ps.release(sl);
  }
  stop_producer();
  if (rc) { drop(); return rc; }
  calitas_free(tx.bounce);
  char* text = tx.text;
  const size_t total = tx.total;
  if (user_dst) {
    if ((uint64_t)total + 1 > call.user_cap) return fail(ctx, CALITAS_EINVAL, "the destination buffer is too small for the text");
    text[total] = 0;
  } else if (!sink) {
    char* grown = (char*)calitas_out_grow(text, total, total + 1);
    if (!grown) { calitas_free(text); return fail(ctx, CALITAS_EINVAL, "out of memory"); }
    text = (char*)calitas_out_shrink(grown, total + 1);           // (a parked block taken for a much smaller text)
    text[total] = 0;
  }
  tm.hit_rows = rows; tm.hits_bytes = total; tm.lanes = 1; tm.contig_passes = n_passes;
  ctx->timing = tm;
  ctx->last_text_bytes = total;
  if (TUNE_GET("CALITAS_TRACE"))
    std::fprintf(stderr, "[calitas] search_hits: one pass per contig (%d), scan %.3f ms, align %.3f ms, all device stages incl. allocation %.3f ms (with a caller's hits: %.3f ms up to the row stage, %.3f ms waiting for the hits), text copy %.3f ms + %.3f ms from the bounce buffer to its place + %.3f ms growing the block (sums), call %.3f ms (%llu rows, %zu bytes)\n",
                 n_contigs, tm.scan_kernel_ms, tm.align_kernel_ms, ms_rows, g_pass_ms[0].load(std::memory_order_relaxed), g_pass_ms[1].load(std::memory_order_relaxed), tm.hits_copy_ms, tx.ms_land, tx.ms_grow,
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(), (unsigned long long)rows, total);
  out.tsv = text; out.bytes = total; out.rows = rows;
  return CALITAS_OK;
}

// calitas_search_counts as one pass per contig: every contig's table is a few KB on the host when its pass returns, so the passes simply
// follow each other on this context's stream -- no second scratch set, no helper thread, nothing to copy -- and the tables are summed
// (removeOverlaps never crosses a contig).
int search_counts_sequential(calitas_ctx* ctx, const HitsCall& call, HitsOut& out) {
  SearchPlan pl;
  int rc = plan_search(ctx, 1, call.guide, call.params, pl);
  if (rc) return rc;
  pl.counts = true;
  pl.model = call.model;
  std::string version, stamp;
  calitas_default_version_and_stamp(call.aligner_version, call.time_stamp, version, stamp);
  const RowStrings rs = make_row_strings(ctx->ref, pl.gh[0], call.guide_id, pl.p, version, stamp);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_bin_base(ctx, pl, ctx->stream);
  if (rc) return rc;
  Passes ps;
  plan_passes(ctx, pl, ps);
  out = HitsOut();
  out.shape = pl.cshape;
  out.counts.assign(pl.cshape.cells(), 0);
  calitas_timing_t tm{};
  for (size_t i = 0; i < ps.plans.size(); i++) {
    LaneText lt;
    rc = lane_rows(ctx, ps.plans[i], false, rs, call.guide_id, version, stamp, lt);
    if (rc) return rc;
    if (lt.counts.size() != out.counts.size()) return fail(ctx, CALITAS_EHIP, "a contig pass returned no counts table (internal error)");
    add_counts(out.counts, lt.counts);
    out.score.add(lt.score);
    out.rows += lt.rows;
    add_lane_timing(tm, lt.tm);
  }
  tm.hit_rows = out.rows; tm.hits_bytes = 0; tm.lanes = 1; tm.contig_passes = (uint32_t)ps.plans.size();
  ctx->timing = tm;
  return CALITAS_OK;
}

}  // namespace calitas
