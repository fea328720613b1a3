// search_hits.cpp -- calitas_search_hits and its siblings (_into, _stream, _ext): whether a search fits one pass, the one-pass call cut
// into lanes (search_hits_attempt), and a window range of a multi-GPU job (search_hits_owned).  The per-contig passes are in
// search_sequential.cpp, the guide batch in search_batch.cpp.
#include <algorithm>
#include <cstring>
#include <ctime>

#include "search_internal.hpp"

void calitas_default_version_and_stamp(const char* aligner_version, const char* time_stamp, std::string& version, std::string& stamp) {
  version = aligner_version ? aligner_version : "";
  stamp = time_stamp ? time_stamp : "";
  if (version.empty()) {  // EditasMetric.Version without a jar manifest: unknown-YYYY-MM-DD
    char b[32]; std::time_t t = std::time(nullptr); std::tm tmv; gmtime_r(&t, &tmv);
    std::strftime(b, sizeof b, "unknown-%Y-%m-%d", &tmv); version = b;
  }
  if (stamp.empty()) {    // RH:169-173 "EEE MMM dd HH:mm:ss z yyyy" in UTC
    char b[64]; std::time_t t = std::time(nullptr); std::tm tmv; gmtime_r(&t, &tmv);
    std::strftime(b, sizeof b, "%a %b %d %H:%M:%S UTC %Y", &tmv); stamp = b;
  }
}

namespace calitas __attribute__((visibility("hidden"))) {

// Whether this search is known not to fit one pass: forced (CALITAS_SEQUENTIAL, tests), or at least as permissive as the last one on
// this context that did not.  remember = true records the search as such.
static bool known_not_to_fit(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, bool remember) {
  if (!remember && TUNE_GET("CALITAS_SEQUENTIAL")) return true;
  SearchPlan pl;
  if (!guide || !params || plan_search(ctx, 1, guide, params, pl) != CALITAS_OK) return false;
  const GuideDev& g = pl.gd[0];
  if (remember) { ctx->seq_L = g.L; ctx->seq_pams = g.n_pams; ctx->seq_min_score = g.min_guide_score; ctx->seq_recs_per_tile = 0; return true; }
  return params->chrom_index < 0 && ctx->seq_pams == g.n_pams && ctx->seq_L == g.L && g.min_guide_score <= ctx->seq_min_score;
}

// Scan records per live tile this search produces, from a scan of every k-th tile with a record capacity of 0 (counted, not kept):
// a few hundred tiles, tens of microseconds.
static int estimate_scan_records(calitas_ctx* ctx, const SearchPlan& pl, double* recs_per_tile, uint64_t* live_tiles) {
  const PackedRef& ref = ctx->ref;
  const uint32_t stride = std::max<uint32_t>(1, pl.n_tiles / 512);
  const uint32_t n_sample = (pl.n_tiles + stride - 1) / stride;
  auto live = [&](uint32_t t) {
    const TileInfo& ti = ref.tiles[t];
    return ti.flag != 2u && ti.contig != 0xFFFFFFFFu && (pl.p.chrom_index < 0 || ti.contig == (uint32_t)pl.p.chrom_index);
  };
  uint64_t live_all = 0, live_sample = 0;
  for (uint32_t t = 0; t < pl.n_tiles; t++) if (live(pl.tile_lo + t)) { live_all++; if (t % stride == 0) live_sample++; }
  *live_tiles = live_all; *recs_per_tile = 0;
  if (live_sample == 0) return CALITAS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::memcpy(ctx->h_guides, pl.gd.data(), sizeof(GuideDev) * pl.n_guides);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_guides, ctx->h_guides, sizeof(GuideDev) * pl.n_guides, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, 8 * sizeof(uint32_t), ctx->stream));
  ScanArgs sa; AlignArgs aa;
  fill_kernel_args(ctx, pl, sa, aa);
  sa.rec_capacity = 0; sa.tile_stride = stride;
  HIP_TRY(ctx, launch_scan_rows(sa, ref.chunk, pl.warm_words, n_sample, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *recs_per_tile = (double)ctx->h_counters[0] / (double)live_sample;
  return CALITAS_OK;
}

// Whether one pass of this search over the whole reference would overrun the device (or CALITAS_DEVICE_BUDGET_MB): decided from the
// worst case when that is harmless, from the memory of the last search that fit, and otherwise from a sampled record count -- not
// from a failed allocation of hundreds of gigabytes.  true: the search is remembered as one for per-contig passes.
static bool predicted_not_to_fit(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params) {
  SearchPlan pl;
  if (!guide || !params || plan_search(ctx, 1, guide, params, pl) != CALITAS_OK) return false;   // the attempt reports the error
  const GuideDev& g = pl.gd[0];
  if (ctx->fit_pams == g.n_pams && ctx->fit_L == g.L && g.min_guide_score >= ctx->fit_min_score) return false;
  uint64_t limit = 0;
  if (const char* e = TUNE_GET("CALITAS_DEVICE_BUDGET_MB")) limit = (uint64_t)std::atoll(e) << 20;
  else {
    size_t mem_free = 0, mem_total = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) return false;
    limit = (uint64_t)mem_total * 7 / 10;
  }
  // per scan record: its strips and itself, with the growth margin of the buffers; per raw alignment (about 1.5 per record): the
  // record, the filter's and the row stage's scratch and its share of the text (~110 + ~1100 bytes)
  const uint64_t per_rec = (pl.slab_per_rec + sizeof(ScanRecord)) * 5 / 4 + (sizeof(RawAln) + 110 + 1100) * 3 / 2;
  const uint64_t worst = (pl.bases / 16 + 1) * 2;
  if (worst <= limit / per_rec) return false;
  double per_tile = 0;
  uint64_t live = 0;
  if (estimate_scan_records(ctx, pl, &per_tile, &live) != CALITAS_OK) return false;
  const double n_rec = per_tile * (double)live;
  if (TUNE_GET("CALITAS_TRACE"))
    std::fprintf(stderr, "[calitas] search_hits: about %.3g scan records expected (%.1f per tile), %.1f GB of scratch for one pass, limit %.1f GB\n",
                 n_rec, per_tile, n_rec * (double)per_rec / 1e9, (double)limit / 1e9);
  if (n_rec * (double)per_rec <= (double)limit) return false;
  ctx->seq_L = g.L; ctx->seq_pams = g.n_pams; ctx->seq_min_score = g.min_guide_score; ctx->seq_recs_per_tile = per_tile;
  return true;
}

// ---- calitas_search_hits on a window range ------------------------------------------------------------------------------
// A process of a multi-GPU job owns a stretch of the genome: the rows whose coordinate_start lies at or behind the start of window
// first_window and before the start of window first_window + n_windows (windowIterator's sequence over the whole reference,
// SearchReference.scala:39-71).  coordinate_start is the first key of ReferenceHit.sort, so the stretches of consecutive ranges are
// consecutive pieces of hits.txt, wherever the cuts fall -- inside a contig, inside a repeat.  The per-bin kernels decide a bin's
// hits from the bin and the edges of its neighbours (binned.hip), so the call aligns the windows the stretch's bins (plus one on
// either side) reach and keeps the rows of the stretch; nothing is exchanged between the processes.  When a bin declines (crowded,
// a chain of hits longer than the halo) the contigs the stretch touches are searched whole on the general kernels and their rows
// filtered by position on the host: slower, same rows.
static int search_hits_owned(calitas_ctx* ctx, const HitsCall& call, HitsOut& out) {
  const calitas_params_t* params = call.params;
  out = HitsOut();
  calitas_params_t whole = *params;
  whole.first_window = 0; whole.n_windows = 0;
  if (whole.chrom_index >= 0) return fail(ctx, CALITAS_EINVAL, "a window range and chrom_index exclude each other");
  SearchPlan pl;
  int rc = plan_search(ctx, 1, call.guide, &whole, pl);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_bin_base(ctx, pl, ctx->stream);
  if (rc) return rc;
  const PackedRef& ref = ctx->ref;
  if (params->first_window < 0 || params->n_windows <= 0 || (uint64_t)params->first_window + (uint64_t)params->n_windows > pl.win_n)
    return fail(ctx, CALITAS_EINVAL, "first_window / n_windows outside the window table (" + std::to_string(pl.win_n) + " windows)");
  std::string version, stamp;
  calitas_default_version_and_stamp(call.aligner_version, call.time_stamp, version, stamp);
  const RowStrings rs = make_row_strings(ref, pl.gh[0], call.guide_id, pl.p, version, stamp);
  const size_t hlen = rs.header.size();
  {
    // the stretch on the per-bin kernels, cut into lanes like any other call (search_hits_attempt): everything it returns is final
    const uint64_t range[2] = {(uint64_t)params->first_window, (uint64_t)params->n_windows};
    bool declined = false;
    const HitsCall all{call.guide, call.guide_id, &whole, call.aligner_version, call.time_stamp, call.user_dst, call.user_cap, nullptr, nullptr, nullptr, call.counts, call.model};
    rc = search_hits_attempt(ctx, all, out, range, &declined);
    if (rc || !declined) return rc;
    HIP_TRY(ctx, calitas_spin_sync(ctx->stream));
  }
  // ---- the contigs the stretch touches, whole, on the general kernels; their rows filtered by position ----
  if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] search_hits on a window range: the bins declined, searching the touched contigs whole\n");
  const std::vector<uint64_t> wb = window_prefix(ref, pl.step);
  const uint64_t first = (uint64_t)params->first_window, last = first + (uint64_t)params->n_windows;
  auto key_of = [&](uint64_t w) {
    int c = 0;
    uint64_t pos = 0;
    window_start(wb, pl.step, w, c, pos);
    return ((uint64_t)c << 32) | pos;
  };
  const uint64_t own_lo = key_of(first), own_hi = key_of(last);
  std::string body;
  uint64_t rows = 0;
  calitas_timing_t tm{};
  // counts mode on this (rare, slow) path: the kept rows are counted by their columns strand (6), guide_mm (16), guide_gaps (17) and
  // pam_mm (19) of RH:99-132 -- the text calls of the touched contigs decide the rows either way
  // score mode: the row's score besides, from its columns total_mm_plus_gaps (20), padded_guide (21), padded_alignment (22) and
  // padded_target (23) -- the contract as written (calitas_hip.h)
  std::vector<uint64_t> table(call.counts ? pl.cshape.cells() : 0, 0);
  // top mode: the row's record besides, from coordinate_start (4), coordinate_end (5) and the columns above; the rows pass in the text's order
  ScoreWords score;
  score.top.k = call.model ? call.model->top_k : 0;
  // regions mode: the row's class besides, from the same two columns (regions.hpp: region_class)
  const RegionsHost* regions = call.model ? call.model->regions : nullptr;
  if (regions) score.reg.init(regions->n_classes, pl.cshape.cells());
  auto count_row = [&](const char* q, const char* row_end, int32_t contig) -> bool {
    const char* f = q;
    uint32_t minus = 0;
    long v[4] = {0, 0, 0, 0}, coord[2] = {0, 0};
    const char* col[3] = {nullptr, nullptr, nullptr};
    size_t col_len[3] = {0, 0, 0};
    for (int k = 0; k < 24 && f < row_end; k++) {
      const char* tab = (const char*)std::memchr(f, '\t', (size_t)(row_end - f));
      if (k == 4 || k == 5) coord[k - 4] = std::strtol(f, nullptr, 10);
      if (k == 6) minus = *f == '-' ? 1u : 0u;
      if (k == 16) v[0] = std::strtol(f, nullptr, 10);
      if (k == 17) v[1] = std::strtol(f, nullptr, 10);
      if (k == 19) v[2] = std::strtol(f, nullptr, 10);
      if (k == 20) v[3] = std::strtol(f, nullptr, 10);
      if (k >= 21) { col[k - 21] = f; col_len[k - 21] = (size_t)((tab ? tab : row_end) - f); }
      f = tab ? tab + 1 : row_end;
    }
    const CountsShape& cs = pl.cshape;
    if (v[0] < 0 || v[1] < 0 || v[2] < 0 || (uint32_t)v[0] >= cs.n_mm || (uint32_t)v[1] >= cs.n_gaps || (uint32_t)v[2] >= cs.n_pam) return false;
    const size_t cell = ((minus * cs.n_mm + (uint32_t)v[0]) * cs.n_gaps + (uint32_t)v[1]) * cs.n_pam + (uint32_t)v[2];
    table[cell]++;
    if (!call.model) return true;
    const uint32_t cls = regions ? region_class(regions->view(), (uint32_t)contig, coord[0], coord[1], ref.contigs[(size_t)contig].len) : 0u;
    if (v[3] == 0) { score.perfect++; if (regions) score.reg.count(cls, cs.cells(), cell, true, 0); return true; }
    uint64_t one = 0;
    if (!col[2] || col_len[0] != col_len[1] || col_len[0] != col_len[2] ||
        !score_columns(*call.model, col[0], col[1], col[2], (int)col_len[0], (int)v[1], (int)v[2], &one)) return false;
    ScoreWords w; w.sum_q32 = one; w.max_q32 = one;
    score.add(w);
    if (regions) score.reg.count(cls, cs.cells(), cell, false, one);
    if (score.top.k && (!regions || ((call.model->list_mask >> cls) & 1u)))
      score.top.push(calitas_top_hit_t{one, contig, (int32_t)coord[0], (int32_t)coord[1], (int8_t)(minus ? '-' : '+'), (uint8_t)v[0], (uint8_t)v[1], (uint8_t)v[2]}, (uint8_t)cls);
    return true;
  };
  for (size_t c = 0; c < ref.contigs.size(); c++) {
    if (wb[c + 1] <= first || wb[c] >= last || wb[c + 1] == wb[c]) continue;
    calitas_params_t pc = whole;
    pc.chrom_index = (int32_t)c;
    const HitsCall one{call.guide, call.guide_id, &pc, version.c_str(), stamp.c_str()};
    HitsOut got;
    rc = search_hits_attempt(ctx, one, got);
    if (rc) return rc;
    char* t = got.tsv;
    // rows: chromosome is column 4, coordinate_start column 5 (RH:99-132); the contig is c, so only the position decides
    const char* q = t + hlen;
    const char* end = t + got.bytes;
    while (q < end) {
      const char* nl = (const char*)std::memchr(q, '\n', (size_t)(end - q));
      const char* row_end = nl ? nl + 1 : end;
      const char* f = q;
      for (int k = 0; k < 4 && f < row_end; k++) { const char* tab = (const char*)std::memchr(f, '\t', (size_t)(row_end - f)); f = tab ? tab + 1 : row_end; }
      const uint64_t pos = std::strtoull(f, nullptr, 10);
      const uint64_t key = ((uint64_t)c << 32) | pos;
      if (key >= own_lo && key < own_hi) {
        if (!call.counts) body.append(q, (size_t)(row_end - q));
        else if (!count_row(q, row_end, (int32_t)c)) { calitas_free(t); return fail(ctx, CALITAS_EHIP, "a hit lies outside the extents of the counts table, or its row cannot be scored (internal error)"); }
        rows++;
      }
      q = row_end;
    }
    calitas_free(t);
    add_lane_timing(tm, ctx->timing);                          // (a whole call's timing each)
  }
  if (call.counts) {
    tm.hit_rows = rows; tm.hits_bytes = 0; tm.lanes = 1;
    ctx->timing = tm;
    out.counts = std::move(table); out.shape = pl.cshape; out.rows = rows; out.score = score;
    return CALITAS_OK;
  }
  const size_t total = hlen + body.size();
  if (call.user_dst && call.user_cap < total + 1) return fail(ctx, CALITAS_EINVAL, "the caller's buffer is too small for the text");
  char* text = call.user_dst ? call.user_dst : (char*)calitas_out_alloc_pinned(total + 1);
  if (!text) return fail(ctx, CALITAS_EINVAL, "out of memory");
  std::memcpy(text, rs.header.data(), hlen);
  std::memcpy(text + hlen, body.data(), body.size());
  text[total] = 0;
  tm.hit_rows = rows; tm.hits_bytes = total; tm.lanes = 1;
  ctx->timing = tm;
  out.tsv = text; out.bytes = total; out.rows = rows;
  return CALITAS_OK;
}

// ---- one pass, cut into lanes ----------------------------------------------------------------------------------------------

// How a one-pass call over `bases` bases is cut into ranges, as relative sizes (empty / one entry: not at all).
static std::vector<double> range_weights(uint64_t bases) {
  std::vector<double> weights;
  if (const char* e = TUNE_GET("CALITAS_CHUNKS")) {
    // "3" = three equal chunks, "5:3:2" = relative sizes
    for (const char* q = e; *q;) {
      char* end = nullptr;
      double v = std::strtod(q, &end);
      if (end == q) break;
      weights.push_back(v);
      q = *end == ':' ? end + 1 : end;
    }
    if (weights.size() == 1) { int k = std::max(1, std::min(16, (int)weights[0])); weights.assign((size_t)k, 1.0); }
    for (double w : weights) if (!(w > 0)) { weights.clear(); break; }
  } else if (bases >= (2048ull << 20)) {
    // measured on hg38-sized input: the last range small, its tail is what nothing hides.  5:3:2 while all of the text
    // crossed the bus behind the first range's rows; with compact rows for the first two ranges (round 4) the copies are half as long
    // and the first range can be larger, the last smaller: 5.5:3:1.5 2.196 ms against 2.268 (tools/sweep_env.py, interleaved;
    // 6:3:1 2.253, 5:3.5:1.5 2.207, four ranges 2.28).  With the last range on the per-bin kernels, its rows compact too and every
    // expansion fed by its copy, the last range shrinks again: 5.8:2.9:1.3 2.016 / 2.025 ms against 2.073 for 5.5:3:1.5 (6:2.8:1.2
    // 2.021, 6.2:2.8:1 2.013, 6.4:2.6:1 2.022, 5.6:3.2:1.2 2.083, 5:3:2 2.104; the cuts fall on contig boundaries)
    weights = {5.8, 2.9, 1.3};
  } else if (bases >= (256ull << 20)) {
    // a half, a quarter or an eighth of it (a rank's share on 2, 4 or 8 GPUs).  Round 3, with the per-bin tail: 1.41 / 0.86 / 0.58 ms
    // for two equal ranges against 1.46 / 0.89 / 0.62 for 3:2 and 1.53 / 0.96 / 0.72 for three; one pass: - / 0.90 / 0.60.
    // Round 4, with the last range's text written in place by its rows kernel (nothing of it is left to copy when its tail ends) the
    // second range shrinks: interleaved on one box (tools/owned_cut_sweep.py) a half 1.315 -> 1.23 ms at 5:3 (3:2 1.25, 2:1 1.31), a
    // quarter 0.75 -> 0.72 at 5:3 (3:2 0.73), an eighth 0.48 -> 0.46 at 3:2 (5:3 0.46-0.49, 2:1 0.53)
    if (bases >= (600ull << 20)) weights = {5, 3};
    else weights = {3, 2};
  }
  return weights;
}

// A window range of a multi-GPU job is cut into consecutive window ranges the same way (a rank of two searches half the genome: one
// pass took 1.68 ms, scan, tail and copy one after the other): each piece owns its stretch, the texts concatenate (coordinate_start
// is the first sort key), and a piece whose bins decline declines the call.
// false: a piece is not one for the bins.  Fewer than two pieces: none (the range stays whole).
static bool cut_owned_range(calitas_ctx* ctx, const SearchPlan& whole, const uint64_t* owned, const std::vector<double>& weights, std::vector<SearchPlan>& owned_plans) {
  double wsum = 0, acc = 0;
  for (double w : weights) wsum += w;
  uint64_t first = owned[0];
  for (size_t c = 0; c < weights.size(); c++) {
    acc += weights[c];
    const uint64_t end = c + 1 == weights.size() ? owned[0] + owned[1] : owned[0] + (uint64_t)((double)owned[1] * acc / wsum);
    if (end <= first) continue;
    SearchPlan q = whole;
    if (!plan_owned_range(ctx, q, first, end - first) || !binned_possible(ctx, q)) return false;
    owned_plans.push_back(q);
    first = end;
  }
  if (owned_plans.size() < 2) owned_plans.clear();
  return true;
}

namespace {
// The block the text of a call is assembled in: the caller's buffer (as much room as it has) or page-locked memory of the library's.
struct TextBlock {
  char* user_dst = nullptr;
  uint64_t user_cap = 0;
  char* text = nullptr;
  char* dev = nullptr;                                         // the same memory as the device addresses it (null: it cannot)
  size_t capacity = 0;                                         // room for rows behind the header
  bool alloc(const std::string& header, size_t body) {
    const size_t hlen = header.size();
    dev = nullptr;
    if (user_dst) {                                   // the caller's buffer: as much room as it has
      if (user_cap < hlen + body + 1 && user_cap < hlen + 1) return false;
      capacity = (size_t)user_cap - hlen - 1;
      text = user_dst;
    } else {
      capacity = body;
      text = (char*)calitas_out_alloc_pinned(hlen + body + 1);
    }
    if (text) std::memcpy(text, header.data(), hlen);
    if (text && !TUNE_GET("CALITAS_TEXT_IN_PLACE_OFF")) {
      void* dp = nullptr;
      if (hipHostGetDevicePointer(&dp, text, 0) == hipSuccess) dev = static_cast<char*>(dp); else (void)hipGetLastError();
    }
    return text != nullptr;
  }
  void release() { if (!user_dst && text) calitas_free(text); text = nullptr; }
};

// A one-pass call under way: what its stages, and the threads of its lanes, share.
struct Attempt {
  calitas_ctx* ctx;
  const HitsCall& call;
  const std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
  SearchPlan pl;                                               // the whole call's; plans: one per lane of a chunked call
  std::vector<SearchPlan> plans;
  std::vector<LaneText> parts;
  std::vector<calitas_ctx*> lanes;
  // The constant pieces of a row.  A chunked search builds them after its scans are queued: nothing on the device needs them before
  // the first range's rows, and the first scan should not wait for string formatting on the host.
  std::string version, stamp;
  RowStrings rs, rs_compact;
  size_t hlen = 0;
  // Compact rows (post.hpp) for the ranges of a chunked call whose text is copied while later ranges are still at work: half the bytes
  // on the bus, head and tail put back by the worker pool.  Not the last range: nothing hides its expansion, and where the per-bin
  // kernels run its rows kernel writes the text straight to its final place.
  std::vector<char> lane_compact;
  bool device_rows = true;
  TextBlock tb;
  std::mutex copy_mu;
  std::mutex mu;                                               // done / placed of the lanes, and parts[] as far as the lanes behind read it
  std::condition_variable cv;
  std::vector<char> done, placed;
  Attempt(calitas_ctx* c, const HitsCall& k) : ctx(c), call(k) { tb.user_dst = k.user_dst; tb.user_cap = k.user_cap; }
  void make_rows() {
    calitas_default_version_and_stamp(call.aligner_version, call.time_stamp, version, stamp);
    rs = make_row_strings(ctx->ref, pl.gh[0], call.guide_id, pl.p, version, stamp);
    rs_compact = compact_row_strings(rs);
    hlen = rs.header.size();
  }
  const RowStrings& rs_lane(size_t c) const { return c < lane_compact.size() && lane_compact[c] ? rs_compact : rs; }
};
enum class Chunked { Done, Declined, OnePass };                // how the lanes of a chunked call ended: with the text / the bins declined a window range / a lane overflowed
}  // namespace

static size_t text_guess(size_t last) { return last + last / 4 + (1u << 20); }   // the next call's text is about as long as the last one's
static const char* const kNoRoom = "the caller's buffer is too small for the text";

// copies lane c's rows to their place (offset = header + rows of the lanes before it)
static int place(Attempt& a, size_t c, size_t offset) {
  LaneText& lt = a.parts[c];
  if (!lt.bytes) return CALITAS_OK;
  calitas_ctx* lane = a.lanes[c];
  if (lt.in_place) {                                         // written by the rows kernel where it belongs: wait for the kernel
    if (lt.d_text != a.tb.dev + a.hlen + offset) return fail(lane, CALITAS_EHIP, "a lane's text was written to another place than the one it belongs to (internal error)");
    HIP_TRY(lane, calitas_spin_sync(lane->stream));
    g_marks.mark("rows-done");
    if (int r = binned_late_failed(lane)) return r;
    lt.tm.hits_copy_ms = 0;
    lt.tm.hits_kernel_ms = rows_stage_ms(lane, lt.tm);
    return CALITAS_OK;
  }
  char* staging = nullptr;
  if (lt.compact_bytes && !lt.on_host) {                     // compact rows: over the bus into a staging block, head and tail put back on the pool
    staging = (char*)calitas_out_alloc_pinned((size_t)lt.compact_bytes);
    if (!staging) return fail(lane, CALITAS_EINVAL, "out of memory");
    g_marks.mark("staging");
  }
  // (Copy and expansion in pieces were no faster while every piece cost two passes of the whole pool -- ~100 us of fixed latency, 2.164
  // against 2.170 ms per hg38-sized call with 4 MB pieces, 3.4 ms with 1 MB; as one job fed by the copy's pieces: see DESIGN.md 4.5.)
  const int r = deliver_lane_text(a.ctx, lane, lt, (size_t)lt.compact_bytes, (size_t)lt.bytes, staging, a.rs.head, a.rs.tail, a.tb.text + a.hlen + offset, &a.copy_mu,
                                  "a lane's compact rows");
  calitas_free(staging);
  if (r) return r;
  if (!lt.on_host) lt.tm.hits_kernel_ms = rows_stage_ms(lane, lt.tm);   // (general kernels: recorded around hits_run by lane_rows)
  return CALITAS_OK;
}

// The lanes of a chunked call, planned and their buffers in place; then everything their kernels need queued, the scans on the scan stream.
static int queue_ranges(Attempt& a, const std::vector<std::pair<int, int>>& ranges, const std::vector<SearchPlan>& owned_plans) {
  calitas_ctx* ctx = a.ctx;
  const size_t K = a.parts.size();
  std::vector<calitas_ctx*>& lanes = a.lanes;
  int rc = ensure_lanes(ctx, K);
  if (rc) return rc;
  a.plans.assign(K, a.pl);
  std::vector<SearchPlan>& plans = a.plans;
  std::vector<uint64_t> wb;
  if (owned_plans.empty()) wb = window_prefix(ctx->ref, a.pl.step);
  for (size_t c = 0; c < K && !rc; c++) {
    lanes[c] = ctx->lanes[c];
    SearchPlan& q = plans[c];
    if (!owned_plans.empty()) q = owned_plans[c];            // (a piece of a window range: planned by cut_owned_range)
    else plan_contig_range(ctx, q, wb, ranges[c].first, ranges[c].second);
    q.narrow_tail = c + 1 < K; q.three_ranges = K >= 3; q.last_range = K >= 3 && c + 1 == K;
    rc = lane_prepare(lanes[c], q);
    if (rc) ctx->err = lanes[c]->err;
  }
  if (rc) return rc;
  // all scans go to one low-priority stream in chunk order; each lane's own (high-priority) stream picks its chunk up
  // when its scan is done, so the tail of chunk c runs while chunk c+1 is still being scanned
  rc = ensure_window_table(ctx, a.pl, ctx->scan_stream);
  if (rc) return rc;
  const bool device_rows = a.device_rows = !TUNE_GET("CALITAS_HOST_HITS");
  {
    bool compact_on = device_rows;
    if (const char* e = TUNE_GET("CALITAS_COMPACT_ROWS")) compact_on = compact_on && std::atoi(e) != 0;
    a.lane_compact.assign(K, 0);
    // Which ranges move compact rows: the leading ones always (their expansion hides behind the later ranges' scans); the last one
    // where the text is long -- a call cut into three: its rows kernel then writes 3 MB into device memory and the text's pieces are
    // expanded as they land, instead of 9 MB written across PCIe by the kernel itself, 2.072 against 2.098 ms per hg38-sized call;
    // the last of two ranges keeps its rows kernel writing in place (a rank of eight: 0.48 against 0.50 ms).
    size_t n_compact = K >= 3 ? K : K - 1;
    if (const char* e = TUNE_GET("CALITAS_COMPACT_LANES")) n_compact = std::min<size_t>(K, (size_t)std::max(0, std::atoi(e)));
    for (size_t c = 0; c < n_compact; c++) a.lane_compact[c] = compact_on ? 1 : 0;
  }
  // (no early return inside this loop: the scans of the earlier lanes are already in flight and every exit waits for them)
  auto hip_rc = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) return (int)CALITAS_OK;
    if (e == hipErrorOutOfMemory) (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? CALITAS_ENOMEM : CALITAS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  // (The inputs of all ranges queued ahead of the first scan, so that the scans run back to back: tried again with the row-wise
  // scan, 2.71 vs 2.68-2.72 ms per pass -- the scans then take 6 % longer beside the tails and nothing is won.)
  g_marks.mark("lanes-ready");
  // (Holding the scan of a range back until the aligner kernels of the range before it are done -- they take half as long again
  // beside a scan, the scan twice as long beside them -- was tried: 2.77 against 2.55 ms per pass.)
  // The inputs of all ranges (guide constants, cleared counters: a 272-byte upload and a fill per lane, 60-140 us of the scan stream
  // each when they sit between two scans) are queued ahead of the scans (round 3: 2.320 against 2.335 ms per hg38-sized call, 0.510
  // against 0.517 for an eighth, interleaved, than all of them ahead of the first scan on the scan stream as in round 2): the first
  // range's inputs ahead of its scan on the scan stream, the later ranges' on their own streams (which have nothing else to do yet);
  // the scan stream waits for each with an event that has long fired when its turn comes.  A range's small inputs are ONE launch
  // (queue_lane_setup) where they used to be two stream commands for the scan and three or four for the row stage.
  std::vector<char> rows_queued(K, 0);                      // the lane's row constants went out with its scan inputs (one launch for both)
  // the first range: its scan inputs (one launch: queue_lane_setup) and its scan, before anything else is prepared
  bool one = false;
  rc = queue_lane_setup(lanes[0], plans[0], nullptr, ctx->scan_stream, &one);
  if (!rc && !one) rc = queue_scan_inputs(lanes[0], plans[0], ctx->scan_stream);
  if (!rc) rc = launch_scan_stage(lanes[0], plans[0], ctx->scan_stream, true);
  if (rc) ctx->err = lanes[0]->err;
  g_marks.mark("scan-queued");
  if (!rc) a.make_rows();
  g_marks.mark("row-strings");
  // the later ranges: scan inputs and row constants in one launch on the range's own stream, then its scan behind the event
  for (size_t c = 1; c < K && !rc; c++) {
    one = false;
    if (device_rows) rc = queue_lane_setup(lanes[c], plans[c], &a.rs_lane(c), lanes[c]->stream, &one);
    if (!rc && one) rows_queued[c] = 1;
    if (!rc && !one) rc = queue_scan_inputs(lanes[c], plans[c], lanes[c]->stream);
    if (!rc) rc = hip_rc(hipEventRecord(lanes[c]->inputs_ready, lanes[c]->stream), "hipEventRecord");
    if (!rc) rc = hip_rc(hipStreamWaitEvent(ctx->scan_stream, lanes[c]->inputs_ready, 0), "hipStreamWaitEvent");
    if (!rc) rc = launch_scan_stage(lanes[c], plans[c], ctx->scan_stream, true);           // records lanes[c]->scan_done
    if (rc && ctx->err.empty()) ctx->err = lanes[c]->err;
    g_marks.mark("scan-queued");
  }
  // ... and the first range's row constants (its tail starts when its scan ends)
  if (!rc && device_rows) {
    one = false;
    rc = queue_lane_setup(lanes[0], plans[0], &a.rs_lane(0), lanes[0]->stream, &one, false);
    if (!rc && one) rows_queued[0] = 1;
    if (rc) ctx->err = lanes[0]->err;
  }
  for (size_t c = 0; c < K && !rc; c++) {
    // the row constants of a range go onto its stream before the wait for its scan: in place while the scan runs
    if (device_rows && !rows_queued[c]) rc = hip_rc(queue_row_constants(lanes[c], plans[c], a.rs_lane(c)), "hits_prepare");
    if (!rc) rc = hip_rc(hipStreamWaitEvent(lanes[c]->stream, lanes[c]->scan_done, 0), "hipStreamWaitEvent");
  }
  g_marks.mark("rows-prepared");
  if (rc) (void)hipDeviceSynchronize();
  return rc;
}

// What lane c of a chunked call does on its thread: its tail (lane_rows), and -- once the lanes before it have said how long their texts
// are -- its text to its place.
static void run_lane(Attempt& a, size_t c) {
  const size_t K = a.parts.size();
  (void)hipSetDevice(a.ctx->device);
  if (c) g_marks.start_at(a.t_call);
  LaneText& lt = a.parts[c];
  // (whatever happens to this lane -- an exception included --, the lanes behind it must not wait for it forever)
  struct DoneGuard {
    std::mutex& mu; std::condition_variable& cv; std::vector<char>& done; size_t c;
    ~DoneGuard() { std::lock_guard<std::mutex> lk(mu); done[c] = 1; cv.notify_all(); }
  } done_guard{a.mu, a.cv, a.done, c};
  // the last range's text is what nothing hides: its rows kernel writes it to its final place -- 0.475 against 0.512 ms for an eighth
  // of the genome, 1.285 against 1.346 for a half.  (For the earlier ranges too: 0.531 / 1.50 ms -- their row kernels then sit on
  // the CUs waiting for the bus while the next range is being scanned; their copies run beside the later ranges' kernels anyway.)
  LaneDest dest;
  dest.get = [&a, c](char** dst, uint64_t* cap) {
    if (!a.tb.dev) return false;
    size_t before = 0;
    std::unique_lock<std::mutex> lk(a.mu);
    a.cv.wait(lk, [&] { for (size_t i = 0; i < c; i++) if (!a.done[i]) return false; return true; });
    for (size_t i = 0; i < c; i++) { if (a.parts[i].rc != CALITAS_OK) return false; before += a.parts[i].bytes; }
    if (before >= a.tb.capacity) return false;
    *dst = a.tb.dev + a.hlen + before; *cap = a.tb.capacity - before;
    return true;
  };
  lt.rc = lane_rows(a.lanes[c], a.plans[c], true, a.rs_lane(c), a.call.guide_id, a.version, a.stamp, lt, a.device_rows,
                    c + 1 == K && a.device_rows && !a.lane_compact[c] && !a.call.counts ? &dest : nullptr);
  if (lt.rc == CALITAS_OK && a.lane_compact[c] && !lt.on_host && !lt.in_place && lt.bytes) {   // what the lanes behind it place their text by: the expanded size
    lt.compact_bytes = lt.bytes;
    lt.bytes += lt.rows * (uint64_t)(a.rs.head.size() + a.rs.tail.size() - 1);
  }
  size_t offset = 0;
  bool ok = lt.rc == CALITAS_OK;
  {
    std::unique_lock<std::mutex> lk(a.mu);
    a.done[c] = 1;
    a.cv.notify_all();
    a.cv.wait(lk, [&] { for (size_t i = 0; i < c; i++) if (!a.done[i]) return false; return true; });
    for (size_t i = 0; i < c; i++) { offset += a.parts[i].bytes; ok = ok && a.parts[i].rc == CALITAS_OK; }
  }
  if (ok && offset + lt.bytes <= a.tb.capacity) {
    int r = place(a, c, offset);
    if (r) lt.rc = r; else a.placed[c] = 1;
  }
  if (c) g_marks.dump((int)c);
}

// The scan stream's idle time between the scans of consecutive ranges: fn(range, whether the events could be read, milliseconds).
template <typename F>
static void for_scan_gaps(const std::vector<calitas_ctx*>& lanes, F fn) {
  for (size_t c = 0; c + 1 < lanes.size(); c++) {
    float ms = 0;
    const bool ok = hipEventElapsedTime(&ms, lanes[c]->t_scan1, lanes[c + 1]->t_scan0) == hipSuccess;
    fn(c, ok, ms);
  }
}

// What became of the lanes of a chunked call: an error, a window range the bins declined, a lane that overflowed (the caller reruns in
// one pass), or the text -- placed again in a block of the right size where the guess was too small.
static int collect_ranges(Attempt& a, bool owned, bool trace, Chunked* outcome) {
  calitas_ctx* ctx = a.ctx;
  const size_t K = a.parts.size();
  std::vector<LaneText>& parts = a.parts;
  int rc = CALITAS_OK;
  bool overflow = false;
  for (size_t c = 0; c < K; c++) {
    if (parts[c].rc == CALITAS_ESTATE) overflow = true;
    else if (parts[c].rc && !rc) { rc = parts[c].rc; ctx->err = a.lanes[c]->err; }
  }
  if (rc == kOwnedDeclined || (owned && overflow)) {          // a piece of the window range could not be decided bin by bin: the caller's slow path
    (void)hipDeviceSynchronize();
    a.tb.release();
    *outcome = Chunked::Declined;
    return CALITAS_OK;
  }
  if (rc || overflow) {
    (void)hipDeviceSynchronize();
    a.tb.release();
    if (rc) return rc;
    {
      // the lanes counted their scan records and alignments even where they could not keep them: would one pass over everything fit?
      uint64_t n_rec = 0, n_raw = 0;
      for (size_t c = 0; c < K; c++) { n_rec += a.lanes[c]->h_counters[0]; n_raw += std::max(a.lanes[c]->h_counters[1], a.lanes[c]->h_counters[3]); }
      // strips + records + alignments with the filter's and the row stage's scratch (~110 + ~1100 bytes each, text included)
      const uint64_t need = n_rec * (a.pl.slab_per_rec + sizeof(ScanRecord)) * 5 / 4 + n_raw * (sizeof(RawAln) + 110 + 1100);
      size_t mem_free = 0, mem_total = 0;
      if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && need > (uint64_t)mem_total * 7 / 10)
        return fail(ctx, CALITAS_ENOMEM, "one pass would need about " + std::to_string(need >> 30) + " GB of scratch on the device");
    }
    if (trace) std::fprintf(stderr, "[calitas] search_hits: a lane's buffers overflowed, rerunning in one pass\n");
    *outcome = Chunked::OnePass;
    return CALITAS_OK;
  }
  size_t total = 0;
  for (auto& lt : parts) total += lt.bytes;
  bool all = true;
  for (size_t c = 0; c < K; c++) all = all && (a.placed[c] || parts[c].bytes == 0);
  if (!all) {   // the guess was too small: place everything again in a buffer of the right size
    if (a.call.user_dst) return fail(ctx, CALITAS_EINVAL, kNoRoom);
    a.tb.release();
    if (!a.tb.alloc(a.rs.header, text_guess(total))) return fail(ctx, CALITAS_EINVAL, "out of memory");   // big enough for the next call's guess as well
    size_t off = 0;
    for (size_t c = 0; c < K; c++) { rc = place(a, c, off); if (rc) { ctx->err = a.lanes[c]->err; a.tb.release(); return rc; } off += parts[c].bytes; }
  }
  *outcome = Chunked::Done;
  return CALITAS_OK;
}

// A call cut into ranges: the lanes planned and queued, one host thread per lane through tail and text, the outcome.
static int attempt_chunked(Attempt& a, const std::vector<std::pair<int, int>>& ranges, const std::vector<SearchPlan>& owned_plans, bool owned, bool trace,
                           Chunked* outcome) {
  calitas_ctx* ctx = a.ctx;
  const size_t K = a.parts.size();
  int rc = queue_ranges(a, ranges, owned_plans);
  if (rc) return rc;
  // (counts mode: no text block -- the lanes' tables are summed when they are all in)
  if (!a.call.counts && !a.tb.alloc(a.rs.header, text_guess(ctx->last_text_bytes))) {
    (void)hipDeviceSynchronize();
    return fail(ctx, CALITAS_EINVAL, "out of memory");
  }
  a.done.assign(K, 0);
  a.placed.assign(K, 0);
  g_marks.mark("text-allocated");
  ctx->lane_threads->start(K, [&a](size_t c) { run_lane(a, c); });
  g_marks.mark("threads-started");
  ctx->lane_threads->guarded([&] { run_lane(a, 0); });         // the calling thread drives the first lane itself
  ctx->lane_threads->wait();
  g_marks.mark("joined");
  if (g_marks.on && !ctx->lane_threads->threw.load()) {       // the scan stream's idle time between the ranges' scans
    std::string gaps;
    for_scan_gaps(a.lanes, [&](size_t c, bool ok, float gap_ms) {
      float ms = 0;
      if (ok) gaps += " " + std::to_string((int)(gap_ms * 1e3f));
      if (hipEventElapsedTime(&ms, a.lanes[c]->t_scan0, a.lanes[c]->t_scan1) == hipSuccess) gaps += " (scan " + std::to_string((int)(ms * 1e3f)) + ")";
    });
    std::fprintf(stderr, "[calitas] scan stream idle between ranges (us):%s\n", gaps.c_str());
  }
  if (ctx->lane_threads->threw.load()) {
    (void)hipDeviceSynchronize();
    a.tb.release();
    return fail(ctx, CALITAS_EHIP, ctx->lane_threads->failure());
  }
  return collect_ranges(a, owned, trace, outcome);
}

// CALITAS_TRACE: the lanes' times, what the scan stream lost between two scans, and the call's line.
static void trace_attempt(const Attempt& a, const calitas_timing_t& tm, bool chunked, uint64_t rows, size_t total) {
  if (a.parts.size() > 1) {
    std::string per;
    for (auto& lt : a.parts) { char b[96]; std::snprintf(b, sizeof b, " [scan %.3f align+trace %.3f rows %.3f copy %.3f]", lt.tm.scan_kernel_ms, lt.tm.align_kernel_ms, lt.tm.hits_kernel_ms, lt.tm.hits_copy_ms); per += b; }
    std::fprintf(stderr, "[calitas] search_hits lanes (ms):%s\n", per.c_str());
    if (chunked) {                                             // what the scan stream lost between two scans: end of one .. start of the next
      std::string gaps;
      for_scan_gaps(a.lanes, [&](size_t, bool ok, float ms) {
        if (!ok) { (void)hipGetLastError(); return; }
        char b[32]; std::snprintf(b, sizeof b, " %.1f", ms * 1e3); gaps += b;
      });
      std::fprintf(stderr, "[calitas] search_hits: scan stream idle between the scans (us):%s\n", gaps.c_str());
    }
  }
  std::fprintf(stderr, "[calitas] search_hits: %zu lane(s), scan %.3f ms, align %.3f ms, hits kernels %.3f ms, text copy %.3f ms (sums over lanes), call %.3f ms (%llu accepted, %llu rows, %zu bytes)\n",
               a.parts.size(), tm.scan_kernel_ms, tm.align_kernel_ms, tm.hits_kernel_ms, tm.hits_copy_ms,
               std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a.t_call).count(),
               (unsigned long long)tm.accepted_alignments, (unsigned long long)rows, total);
}

// One pass over everything the call covers, in one lane or cut into ranges that are pipelined against each other.
int search_hits_attempt(calitas_ctx* ctx, const HitsCall& call, HitsOut& out, const uint64_t* owned, bool* owned_declined) {
  if (!owned && call.params && (call.params->first_window != 0 || call.params->n_windows != 0)) return search_hits_owned(ctx, call, out);
  if (owned_declined) *owned_declined = false;
  Attempt a(ctx, call);
  SearchPlan& pl = a.pl;
  out = HitsOut();
  int rc = plan_search(ctx, 1, call.guide, call.params, pl);
  if (rc) return rc;
  pl.counts = call.counts;
  pl.model = call.counts ? call.model : nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_bin_base(ctx, pl, ctx->stream);                // (built once per reference and window size)
  if (rc) return rc;
  const PackedRef& ref = ctx->ref;
  const SearchPlan whole = pl;
  if (owned && (!plan_owned_range(ctx, pl, owned[0], owned[1]) || !binned_possible(ctx, pl))) { if (owned_declined) *owned_declined = true; return CALITAS_OK; }
  const bool trace = TUNE_GET("CALITAS_TRACE") != nullptr;

  // ---- how many lanes: one pass over the whole reference, or contig ranges pipelined against each other ----
  const std::vector<double> weights = range_weights(owned ? owned[1] * (uint64_t)pl.step : ref.total_bases);
  std::vector<std::pair<int, int>> ranges;
  if (!owned && weights.size() > 1 && pl.p.chrom_index < 0 && ref.contigs.size() > 1) ranges = chunk_ranges(ref, weights);
  std::vector<SearchPlan> owned_plans;
  if (owned && weights.size() > 1 && !cut_owned_range(ctx, whole, owned, weights, owned_plans)) { if (owned_declined) *owned_declined = true; return CALITAS_OK; }
  const size_t K = !owned_plans.empty() ? owned_plans.size() : ranges.size() > 1 ? ranges.size() : 1;
  a.parts.assign(K, LaneText());
  a.lanes.assign(K, ctx);

  bool chunked = K > 1;
  g_marks.mark("planned");
  if (chunked) {
    Chunked outcome = Chunked::Done;
    rc = attempt_chunked(a, ranges, owned_plans, owned != nullptr, trace, &outcome);
    if (rc) return rc;
    if (outcome == Chunked::Declined) { if (owned_declined) *owned_declined = true; return CALITAS_OK; }
    if (outcome == Chunked::OnePass) {
      chunked = false;
      a.parts.assign(1, LaneText()); a.lanes.assign(1, ctx);
    }
  }
  if (!chunked) {
    if (a.rs.header.empty()) a.make_rows();
    rc = lane_rows(ctx, pl, false, a.rs, call.guide_id, a.version, a.stamp, a.parts[0]);
    if (rc == kOwnedDeclined) { if (owned_declined) *owned_declined = true; return CALITAS_OK; }
    if (rc) return rc;
    g_marks.mark("lane-done");
    if (!call.counts) {                                      // (counts mode: no text to place)
      if (!a.tb.alloc(a.rs.header, (size_t)a.parts[0].bytes) || a.parts[0].bytes > a.tb.capacity) return fail(ctx, CALITAS_EINVAL, call.user_dst ? kNoRoom : "out of memory");
      rc = place(a, 0, 0);
      if (rc) { a.tb.release(); return rc; }
      g_marks.mark("text-copied");
    }
  }
  if (call.counts) {                                         // the ranges' tables summed: no text, no copy
    calitas_timing_t tm{};
    out.counts.assign(pl.cshape.cells(), 0);
    out.shape = pl.cshape;
    for (auto& lt : a.parts) {
      if (lt.counts.size() != out.counts.size()) return fail(ctx, CALITAS_EHIP, "a lane returned no counts table (internal error)");
      add_counts(out.counts, lt.counts);
      out.score.add(lt.score);
      out.rows += lt.rows;
      add_lane_timing(tm, lt.tm);
    }
    tm.hit_rows = out.rows; tm.hits_bytes = 0; tm.lanes = (uint32_t)a.parts.size();
    ctx->timing = tm;
    if (trace) trace_attempt(a, tm, chunked, out.rows, 0);
    return CALITAS_OK;
  }
  size_t total = a.hlen;
  calitas_timing_t tm{};
  uint64_t rows = 0;
  for (auto& lt : a.parts) {
    total += lt.bytes; rows += lt.rows;
    add_lane_timing(tm, lt.tm);
  }
  a.tb.text[total] = 0;
  tm.hit_rows = rows; tm.hits_bytes = total; tm.lanes = (uint32_t)a.parts.size();
  ctx->timing = tm;
  ctx->last_text_bytes = total;
  if (trace) trace_attempt(a, tm, chunked, rows, total);
  if (pl.p.chrom_index < 0 && (ctx->fit_pams != pl.gd[0].n_pams || ctx->fit_L != pl.gd[0].L || pl.gd[0].min_guide_score < ctx->fit_min_score)) {
    ctx->fit_L = pl.gd[0].L; ctx->fit_pams = pl.gd[0].n_pams; ctx->fit_min_score = pl.gd[0].min_guide_score;   // the most permissive search seen to fit
  }
  out.tsv = a.tb.text; out.bytes = total; out.rows = rows;
  return CALITAS_OK;
}

// The way of every whole-reference call: one pass unless the search is known or predicted not to fit the device -- or turns out not to
// (CALITAS_ENOMEM: scratch released, the search remembered) -- and then one pass per contig.  label: the entry point, for the trace line.
// *one_pass: the result is the attempt's (the text in one block, whatever call.sink says).
static int search_hits_fitted(calitas_ctx* ctx, const HitsCall& call, HitsOut& out, const char* label, bool* one_pass) {
  *one_pass = false;
  if (!known_not_to_fit(ctx, call.guide, call.params, false) && !predicted_not_to_fit(ctx, call.guide, call.params)) {
    const int rc = search_hits_attempt(ctx, call, out);
    if (rc != CALITAS_ENOMEM) { *one_pass = true; return rc; }
    if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] %s: %s -- retrying with one pass per contig\n", label, ctx->err.c_str());
    release_scratch(ctx);
    (void)known_not_to_fit(ctx, call.guide, call.params, true);
  }
  out = HitsOut();
  const int rc = call.counts ? search_counts_sequential(ctx, call, out) : search_hits_sequential(ctx, call, out);
  if (rc == CALITAS_ENOMEM) release_scratch(ctx);   // leave the context usable for smaller searches
  return rc;
}

}  // namespace calitas

int calitas_search_hits_impl(calitas_ctx* ctx, const calitas_guide_t* guide, const std::string& guide_id, const calitas_params_t* params,
                            const char* aligner_version, const char* time_stamp, char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows) {
  g_marks.start();
  struct Dump { ~Dump() { g_marks.mark("return"); g_marks.dump(); } } dump_at_exit;
  const HitsCall call{guide, guide_id, params, aligner_version, time_stamp};
  HitsOut out;
  bool one_pass = false;
  const int rc = params && (params->first_window != 0 || params->n_windows != 0)     // a process's stretch of a multi-GPU job: one pass, no per-contig mode
                     ? search_hits_attempt(ctx, call, out) : search_hits_fitted(ctx, call, out, "search_hits", &one_pass);
  out.store(tsv, tsv_bytes, n_rows);
  return rc;
}

// calitas_search_counts: the ways of calitas_search_hits (one pass in lanes, a window range, one pass per contig) with HitsCall::counts set.
int calitas_search_counts_impl(calitas_ctx* ctx, const calitas_guide_t* guide, const calitas_params_t* params, CountsShape* shape,
                               std::vector<uint64_t>* table, uint64_t* rows, const ScoreModelHost* model, ScoreWords* score) {
  // (model: calitas_search_scores -- the same ways in score mode, *score receives what the rows' scores add up to)
  g_marks.start();
  struct Dump { ~Dump() { g_marks.mark("return"); g_marks.dump(); } } dump_at_exit;
  static const std::string no_id;
  HitsCall call{guide, no_id, params, "-", "-"};             // (no row carries them: nothing to format)
  call.counts = true;
  call.model = model;
  HitsOut out;
  bool one_pass = false;
  const int rc = params && (params->first_window != 0 || params->n_windows != 0)
                     ? search_hits_attempt(ctx, call, out) : search_hits_fitted(ctx, call, out, "search_counts", &one_pass);
  if (rc) return rc;
  if (out.counts.size() != out.shape.cells() || out.counts.empty()) return fail(ctx, CALITAS_EHIP, "the search returned no counts table (internal error)");
  *shape = out.shape; *table = std::move(out.counts); *rows = out.rows;
  if (score) *score = out.score;
  return CALITAS_OK;
}

// calitas_search_hits with hits of the caller's own brought into every contig's row stage (the variant branch, variants.cpp: VariantSearch::start_threads): one pass per
// contig on the general kernels.  kExtDeclined is returned as CALITAS_ESTATE + *declined: a stage left the device path, the caller
// merges on the host instead.
int calitas_search_hits_ext_impl(calitas_ctx* ctx, const calitas_guide_t* guide, const std::string& guide_id, const calitas_params_t* params,
                                 const char* aligner_version, const char* time_stamp, const HitsExtSource& source, char** tsv,
                                 uint64_t* tsv_bytes, uint64_t* n_rows, bool* declined, char* user_dst, uint64_t user_cap) {
  *declined = false;
  *tsv = nullptr;
  if (!known_not_to_fit(ctx, guide, params, false)) (void)predicted_not_to_fit(ctx, guide, params);   // (sizes the passes' buffers when the search is a dense one)
  const HitsCall call{guide, guide_id, params, aligner_version, time_stamp, user_dst, user_cap, nullptr, nullptr, &source};
  HitsOut out;
  int rc = search_hits_sequential(ctx, call, out);
  if (rc == kExtDeclined) { *declined = true; *tsv = nullptr; return CALITAS_ESTATE; }
  if (rc == CALITAS_ENOMEM) release_scratch(ctx);
  if (rc == CALITAS_OK) out.store(tsv, tsv_bytes, n_rows);
  return rc;
}

// calitas_search_hits_into: one pass (with lanes), text straight into the caller's buffer -- or, since round 5, one pass per contig when
// the search does not fit the device (a PAM-less search at eight differences on a whole genome: tens of gigabytes of text): every
// contig's rows then cross the bus straight to their place in the buffer (search_hits_sequential's user_dst).  A window range
// (first_window / n_windows) stays one pass.
int calitas_search_hits_into_impl(calitas_ctx* ctx, const calitas_guide_t* guide, const std::string& guide_id, const calitas_params_t* params,
                                  const char* aligner_version, const char* time_stamp, char* dst, uint64_t dst_capacity, uint64_t* tsv_bytes,
                                  uint64_t* n_rows) {
  if (!dst || dst_capacity < 2) return fail(ctx, CALITAS_EINVAL, "no destination buffer");
  const HitsCall call{guide, guide_id, params, aligner_version, time_stamp, dst, dst_capacity};
  HitsOut out;
  bool one_pass = false;
  const int rc = params && (params->first_window != 0 || params->n_windows != 0) ? search_hits_attempt(ctx, call, out)
                                                                                  : search_hits_fitted(ctx, call, out, "search_hits_into", &one_pass);
  out.store(nullptr, tsv_bytes, n_rows);
  return rc;
}

// calitas_search_hits_stream: the text goes to `sink` -- in one piece when the search fits one call, header and per-contig pieces
// otherwise (no block of the size of the whole text is ever allocated then).
int calitas_search_hits_stream_impl(calitas_ctx* ctx, const calitas_guide_t* guide, const std::string& guide_id, const calitas_params_t* params,
                                    const char* aligner_version, const char* time_stamp, calitas_text_sink_t sink, void* user,
                                    uint64_t* tsv_bytes, uint64_t* n_rows) {
  const HitsCall call{guide, guide_id, params, aligner_version, time_stamp, nullptr, 0, sink, user};
  HitsOut out;
  bool one_pass = false;
  const int rc = search_hits_fitted(ctx, call, out, "search_hits", &one_pass);
  if (rc) return rc;
  if (one_pass) {                                   // the text in one block: handed over whole
    const int s = sink(out.tsv, out.bytes, user);
    calitas_free(out.tsv);
    if (s != 0) return fail(ctx, CALITAS_EIO, "the text sink reported an error");
  }
  out.store(nullptr, tsv_bytes, n_rows);
  return CALITAS_OK;
}
