// search_plan.cpp -- planning: validation and the host-side constants of a search (SearchPlan), the buffers and device tables a plan
// needs (window table, bin bases), the kernel arguments, and the cuts of a reference into contig ranges / of a window range into
// pieces.  Nothing here launches a search kernel (search_run.cpp) or drives a lane (search_lane.cpp).
#include <algorithm>
#include <cstring>

#include "search_internal.hpp"
#include "slab.hpp"

std::string build_guide_dev(const GuideHost& gh, const calitas_params_t& p, const Scores& sc, int max_guide_diffs, int max_pam_mismatches,
                            GuideDev& gd) {
  std::memset(&gd, 0, sizeof(gd));
  const int L = (int)gh.q.size();
  gd.L = L;
  gd.n_pams = (int)gh.pams_q.size();
  gd.cli_length = gh.cli_length;
  gd.min_guide_score = sc.match * L + sc.worst_guide_diff * max_guide_diffs;         // SGA:239-243
  gd.max_guide_diffs = max_guide_diffs;
  gd.max_pam_mismatches = max_pam_mismatches;
  gd.max_diffs_filtering = max_guide_diffs + p.max_gaps_between_guide_and_pam + max_pam_mismatches;   // SGA:249
  gd.pam5 = gh.pam5 ? 1 : 0;
  const int budget = sc.match * L - gd.min_guide_score;                              // = |worst| * d
  // score(all matches) - score(path) = sum of per-edit costs: mismatch |m|, guide-only base |b|, genome-only base |B|
  const int c_mm = iabs(p.guide_mismatch_net_cost), c_ins = iabs(p.genome_gap_net_cost), c_del = iabs(p.guide_gap_net_cost);
  const int c_min = std::min(c_mm, std::min(c_ins, c_del));
  if (c_min <= 0 || c_del <= 0) return "net costs of 0 are not supported (the candidate filter needs every edit to cost something)";
  gd.scan_max_edits = budget / c_min;
  const int max_del = budget / c_del;
  gd.span = L + max_del;
  if (gd.span + 1 + 16 > STRIP_MAX_COLS || gd.span + 1 > RAW_MAX_OPS)
    return "max-guide-diffs too large for this protospacer (strip wider than the aligner kernel supports)";
  if (L + gd.scan_max_edits > 64) return "max-guide-diffs too large for the scan warm-up";
  for (int code = 0; code < 4; code++) {
    uint32_t v = 0;
    for (int i = 0; i < L; i++) if (iupac_mask((unsigned char)gh.q[i]) & (1 << code)) v |= 1u << (32 - L + i);
    gd.peq_a[code] = v;
  }
  uint32_t all = 0;
  for (int i = 0; i < L; i++) all |= 1u << (32 - L + i);
  gd.peq_a[4] = 0; gd.peq_a[5] = all; gd.peq_a[6] = 0; gd.peq_a[7] = 0;
  for (int code = 0; code < 4; code++) gd.peq_b[code] = gd.peq_a[3 - code];
  for (int k = 4; k < 8; k++) gd.peq_b[k] = gd.peq_a[k];
  for (int i = 0; i < L; i++) gd.qmask[i] = (uint8_t)iupac_mask((unsigned char)gh.q[i]);
  for (int i = 0; i < L; i++) gd.row_sets[i >> 4] |= (uint64_t)gd.qmask[i] << ((i & 15) * 4);
  for (int pi = 0; pi < gd.n_pams; pi++) {
    gd.pam_len[pi] = (uint8_t)gh.pams_q[pi].size();
    for (size_t k = 0; k < gh.pams_q[pi].size(); k++) gd.pam_mask[pi][k] = (uint8_t)iupac_mask((unsigned char)gh.pams_q[pi][k]);
  }
  return "";
}

static CountsShape shape_of(const GuideDev& gd, const calitas_params_t& p) {
  CountsShape s;
  s.n_mm = (uint32_t)gd.scan_max_edits + 1u;
  s.n_gaps = (uint32_t)gd.scan_max_edits + (uint32_t)p.max_gaps_between_guide_and_pam + 1u;
  s.n_pam = (gd.n_pams > 0 ? (uint32_t)p.max_pam_mismatches : 0u) + 1u;
  return s;
}

std::string counts_shape(const GuideHost& gh, const calitas_params_t& p, CountsShape& shape) {
  if (p.max_guide_diffs < 0 || p.max_pam_mismatches < 0 || p.max_gaps_between_guide_and_pam < 0 || p.max_gaps_between_guide_and_pam > 16)
    return "limits out of range (max-gaps-between-guide-and-pam must be 0..16)";
  const Scores sc = derive_scores(p.guide_mismatch_net_cost, p.pam_mismatch_net_cost, p.genome_gap_net_cost, p.guide_gap_net_cost);
  GuideDev gd;
  const std::string e = build_guide_dev(gh, p, sc, p.max_guide_diffs, p.max_pam_mismatches, gd);
  if (e.empty()) shape = shape_of(gd, p);
  return e;
}

int ensure_buffers(calitas_ctx* ctx, uint32_t rec_cap, uint32_t raw_cap, uint64_t slab_per_rec, uint32_t item_cap) {
  rec_cap = std::max(rec_cap, ctx->rec_cap);
  if (const char* e = TUNE_GET("CALITAS_DEVICE_BUDGET_MB")) {   // refuse instead of trying: what a caller sharing the card can set
    const uint64_t want = (uint64_t)rec_cap * slab_per_rec + (uint64_t)rec_cap * sizeof(ScanRecord) +
                          (uint64_t)std::max(raw_cap, ctx->raw_cap) * sizeof(RawAln) + (uint64_t)std::max(item_cap, ctx->item_cap) * sizeof(uint64_t);
    if (want > (uint64_t)std::atoll(e) << 20)
      return calitas_fail(ctx, CALITAS_ENOMEM, "search buffers of " + std::to_string(want >> 20) + " MB exceed CALITAS_DEVICE_BUDGET_MB");
  }
  if (item_cap > ctx->item_cap) {
    (void)hipFree(ctx->d_items); ctx->d_items = nullptr; ctx->item_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_items, (size_t)item_cap * sizeof(uint64_t)));
    ctx->item_cap = item_cap;
  }
  if ((uint64_t)rec_cap * slab_per_rec > ctx->slab_cap) {
    (void)hipFree(ctx->d_slab); ctx->d_slab = nullptr; ctx->slab_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_slab, (size_t)rec_cap * slab_per_rec));
    ctx->slab_cap = (uint64_t)rec_cap * slab_per_rec;
  }
  if (rec_cap > ctx->rec_cap) {
    (void)hipFree(ctx->d_recs); ctx->d_recs = nullptr; ctx->rec_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_recs, (size_t)rec_cap * sizeof(ScanRecord)));
    ctx->rec_cap = rec_cap;
  }
  if (raw_cap > ctx->raw_cap) {
    (void)hipFree(ctx->d_raw); ctx->d_raw = nullptr; ctx->raw_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_raw, (size_t)raw_cap * sizeof(RawAln)));
    ctx->raw_cap = raw_cap;
  }
  return CALITAS_OK;
}

namespace calitas __attribute__((visibility("hidden"))) {

// The bins of contigs [c0, c1) of the plan's geometry (the owner's bin_base must be built: ensure_bin_base).
static void plan_bins(const calitas_ctx* owner, SearchPlan& q, int c0, int c1) {
  if (!q.bin_shift || owner->bin_base.empty()) { q.bin_first = 0; q.n_bins = 0; return; }
  q.bin_first = owner->bin_base[c0];
  q.n_bins = owner->bin_base[c1] - q.bin_first;
}

// Per contig the index of its first window in windowIterator's sequence over the whole reference; [n_contigs] = all windows.
std::vector<uint64_t> window_prefix(const PackedRef& ref, int step) {
  std::vector<uint64_t> wb(ref.contigs.size() + 1, 0);
  for (size_t c = 0; c < ref.contigs.size(); c++) wb[c + 1] = wb[c] + window_count(ref.contigs[c].len, step);
  return wb;
}

// The contig global window w lies in (the last contig for a w at or behind the end of the table).
int window_contig(const std::vector<uint64_t>& wb, uint64_t w) {
  return std::min((int)(std::upper_bound(wb.begin(), wb.end(), w) - wb.begin()) - 1, (int)wb.size() - 2);
}

// Start of global window w as (contig, position); a w at or behind the end of the table: (number of contigs, 0), the end of the reference.
void window_start(const std::vector<uint64_t>& wb, int step, uint64_t w, int& c, uint64_t& pos) {
  if (w >= wb.back()) { c = (int)wb.size() - 1; pos = 0; return; }
  c = window_contig(wb, w);
  pos = (w - wb[c]) * (uint64_t)step;
}

// Narrows a plan of the whole reference to contigs [c0, c1): their tiles, bases, windows (wb = window_prefix of the plan's step) and bins.
void plan_contig_range(const calitas_ctx* ctx, SearchPlan& q, const std::vector<uint64_t>& wb, int c0, int c1) {
  const PackedRef& ref = ctx->ref;
  q.tile_lo = (uint32_t)(ref.contigs[c0].gbase / ref.tile);
  const uint32_t tile_hi = c1 < (int)ref.contigs.size() ? (uint32_t)(ref.contigs[c1].gbase / ref.tile) : (uint32_t)ref.tiles.size();
  q.n_tiles = tile_hi - q.tile_lo;
  q.bases = 0;
  for (int k = c0; k < c1; k++) q.bases += ref.contigs[k].len;
  q.win_lo = wb[c0]; q.win_n = wb[c1] - wb[c0];
  plan_bins(ctx, q, c0, c1);
}

// Validation and the host-side constants of a search.  Covers the whole reference (or the one contig of chrom_index);
// a chunked search narrows tile_lo / n_tiles / bases per lane afterwards.
int plan_search(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params, SearchPlan& pl) {
  if (!guides || !params) return fail(ctx, CALITAS_EINVAL, "NULL argument");
  if (ctx->device < 0) return fail(ctx, CALITAS_ENODEV, "host-only context: calitas_search needs a GPU (there is no CPU fallback)");
  if (!ref_owner(ctx)->has_ref) return fail(ctx, CALITAS_ESTATE, "calitas_set_reference has not been called");
  if (n_guides <= 0 || n_guides > MAX_GUIDES) return fail(ctx, CALITAS_EINVAL, "n_guides must be 1..64");
  const calitas_params_t& p = *params;
  if (p.window_size <= 0 || p.window_size > 60000) return fail(ctx, CALITAS_EINVAL, "window-size must be 1..60000");
  if (p.max_guide_diffs < 0 || p.max_pam_mismatches < 0 || p.max_gaps_between_guide_and_pam < 0 || p.max_gaps_between_guide_and_pam > 16)
    return fail(ctx, CALITAS_EINVAL, "limits out of range (max-gaps-between-guide-and-pam must be 0..16)");
  const PackedRef& ref = ref_owner(ctx)->ref;
  if (p.chrom_index >= (int)ref.contigs.size()) return fail(ctx, CALITAS_EINVAL, "chrom_index out of range");
  pl.p = p; pl.n_guides = n_guides;
  pl.sc = derive_scores(p.guide_mismatch_net_cost, p.pam_mismatch_net_cost, p.genome_gap_net_cost, p.guide_gap_net_cost);
  pl.max_total = p.max_total_diffs >= 0 ? p.max_total_diffs : p.max_guide_diffs + p.max_gaps_between_guide_and_pam + p.max_pam_mismatches;
  pl.gh.assign(n_guides, GuideHost());
  pl.gd.assign(n_guides, GuideDev());
  for (int i = 0; i < n_guides; i++) {
    std::string e = make_guide_host(guides[i], pl.gh[i]);
    if (e.empty()) e = build_guide_dev(pl.gh[i], p, pl.sc, p.max_guide_diffs, p.max_pam_mismatches, pl.gd[i]);
    if (!e.empty()) return fail(ctx, CALITAS_EINVAL, "guide " + std::to_string(i) + ": " + e);
    // SR:529-530: the window step depends on the CLI guide length; one pass shares one tiling
    int overlap = pl.gh[i].cli_length + p.max_guide_diffs + p.max_gaps_between_guide_and_pam - 1;
    int s = p.window_size - overlap;
    if (s <= 0) return fail(ctx, CALITAS_EINVAL, "window-size is not larger than guide length + max-guide-diffs + max-gaps - 1");
    if (i == 0) pl.step = s;
    else if (s != pl.step) return fail(ctx, CALITAS_EINVAL, "all guides of one batch must have the same length (same window tiling, SearchReference.scala:529)");
    if ((pl.gd[i].L + pl.gd[i].scan_max_edits + 15) / 16 > ref.chunk / 16) return fail(ctx, CALITAS_EINVAL, "scan warm-up exceeds the lane chunk");
    pl.warm_words = std::max(pl.warm_words, (pl.gd[i].L + pl.gd[i].scan_max_edits - 1 + 31) / 32);
  }
  pl.cshape = shape_of(pl.gd[0], p);
  // Strip slabs (align_kernel -> trace_kernel): fixed size and fixed address per (record, window slot).
  pl.slots_per_rec = (uint32_t)((p.window_size + 14) / pl.step + 1);   // windows a 16-base word can fall into
  if (pl.slots_per_rec > 8) return fail(ctx, CALITAS_EINVAL, "window step is too small relative to the window size (more than 8 windows per position)");
  pl.slab_bytes = 0;
  for (int i = 0; i < n_guides; i++) pl.slab_bytes = std::max(pl.slab_bytes, slab_bytes_for(pl.gd[i].L, pl.gd[i].span, p.max_gaps_between_guide_and_pam));
  pl.slab_per_rec = (uint64_t)pl.slab_bytes * pl.slots_per_rec;
  pl.tile_lo = 0; pl.n_tiles = (uint32_t)ref.tiles.size();
  pl.bin_shift = binned_shift(p.window_size);
  pl.bases = p.chrom_index >= 0 ? ref.contigs[p.chrom_index].len : ref.total_bases;
  pl.win_lo = 0; pl.win_n = 0;
  for (auto& c : ref.contigs) pl.win_n += window_count(c.len, pl.step);
  if (p.n_windows != 0 || p.first_window != 0) {
    // a window range of the job: scan the tiles its windows touch, align only inside those windows
    if (p.first_window < 0 || p.n_windows <= 0 || (uint64_t)p.first_window + (uint64_t)p.n_windows > pl.win_n)
      return fail(ctx, CALITAS_EINVAL, "first_window / n_windows outside the window table (" + std::to_string(pl.win_n) + " windows)");
    if (p.chrom_index >= 0) return fail(ctx, CALITAS_EINVAL, "a window range and chrom_index exclude each other");
    pl.gw_lo = (uint64_t)p.first_window; pl.gw_hi = pl.gw_lo + (uint64_t)p.n_windows;
    uint64_t base = 0, g_lo = 0, g_hi = 0, bases = 0;
    bool first = true;
    for (auto& c : ref.contigs) {
      const uint64_t nw = window_count(c.len, pl.step);
      const uint64_t a = std::max(pl.gw_lo, base), b = std::min(pl.gw_hi, base + nw);     // this contig's share of the range
      if (a < b) {
        const uint64_t lo = (a - base) * (uint64_t)pl.step, hi = std::min<uint64_t>(c.len, (b - 1 - base) * (uint64_t)pl.step + (uint64_t)p.window_size);
        if (first) { g_lo = c.gbase + lo; first = false; }
        g_hi = c.gbase + hi;
        bases += hi - lo;
      }
      base += nw;
    }
    pl.tile_lo = (uint32_t)(g_lo / ref.tile);
    pl.n_tiles = (uint32_t)((g_hi + ref.tile - 1) / ref.tile) - pl.tile_lo;
    pl.bases = bases;
    pl.win_lo = pl.gw_lo; pl.win_n = pl.gw_hi - pl.gw_lo;
  }
  return CALITAS_OK;
}

// The device window table for (window size, step) lives with the reference; (re)built on `stream` when the tiling changes.
int ensure_window_table(calitas_ctx* ctx, const SearchPlan& pl, hipStream_t stream) {
  calitas_ctx* o = ref_owner(ctx);
  if (o->win_W == pl.p.window_size && o->win_step == pl.step) return CALITAS_OK;
  const PackedRef& ref = o->ref;
  const std::vector<uint64_t> wb = window_prefix(ref, pl.step);
  const uint64_t nw = wb.back();
  if (!o->d_win_base) HIP_TRY(ctx, hipMalloc((void**)&o->d_win_base, wb.size() * sizeof(uint64_t)));
  if (nw > o->win_cap) {
    (void)hipFree(o->d_win); o->d_win = nullptr; o->win_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&o->d_win, std::max<uint64_t>(1, nw) * sizeof(int2)));
    o->win_cap = nw;
  }
  HIP_TRY(ctx, hipMemcpyAsync(o->d_win_base, wb.data(), wb.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream));   // ordered before the kernel below
  HIP_TRY(ctx, hipStreamSynchronize(stream));                                                                              // wb is a local
  HIP_TRY(ctx, launch_window_table(o->d_runs, (int64_t)ref.runs.size(), o->d_contigs, o->d_win_base, (int)ref.contigs.size(), nw,
                                   pl.p.window_size, pl.step, o->d_win, stream));
  o->win_W = pl.p.window_size; o->win_step = pl.step;
  return CALITAS_OK;
}

// Per contig the index of its first bin (binned.hpp), for the plan's bin size; lives with the reference like the window table.
int ensure_bin_base(calitas_ctx* ctx, SearchPlan& pl, hipStream_t stream) {
  calitas_ctx* o = ref_owner(ctx);
  if (!pl.bin_shift) return CALITAS_OK;
  const PackedRef& ref = o->ref;
  if (o->bin_shift != pl.bin_shift || o->bin_base.size() != ref.contigs.size() + 1) {
    std::vector<uint32_t> bb(ref.contigs.size() + 1, 0);
    uint64_t acc = 0;
    for (size_t c = 0; c < ref.contigs.size(); c++) { bb[c] = (uint32_t)acc; acc += (ref.contigs[c].len >> pl.bin_shift) + 1; }
    bb[ref.contigs.size()] = (uint32_t)acc;
    if (acc >= 0x7FFFFFFFull) { pl.bin_shift = 0; return CALITAS_OK; }
    (void)hipFree(o->d_bin_base); o->d_bin_base = nullptr; o->bin_shift = 0;
    (void)hipFree(o->d_bin_contig); o->d_bin_contig = nullptr;
    std::vector<uint32_t> bc((size_t)acc + 1, 0);
    for (size_t c = 0; c < ref.contigs.size(); c++) std::fill(bc.begin() + bb[c], bc.begin() + bb[c + 1], (uint32_t)c);
    HIP_TRY(ctx, hipMalloc((void**)&o->d_bin_base, bb.size() * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMalloc((void**)&o->d_bin_contig, bc.size() * sizeof(uint32_t)));
    HIP_TRY(ctx, hipMemcpyAsync(o->d_bin_base, bb.data(), bb.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipMemcpyAsync(o->d_bin_contig, bc.data(), bc.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));                                                                              // bb / bc are locals
    o->bin_base.swap(bb); o->bin_shift = pl.bin_shift;
  }
  if (pl.n_bins == 0) plan_bins(o, pl, pl.p.chrom_index >= 0 ? pl.p.chrom_index : 0, pl.p.chrom_index >= 0 ? pl.p.chrom_index + 1 : (int)ref.contigs.size());
  return CALITAS_OK;
}

void fill_kernel_args(calitas_ctx* ctx, const SearchPlan& pl, ScanArgs& sa, AlignArgs& aa) {
  const calitas_ctx* o = ref_owner(ctx);
  const PackedRef& ref = o->ref;
  const calitas_params_t& p = pl.p;
  sa = ScanArgs{};
  sa.codes = o->d_codes; sa.planes = o->d_planes; sa.mask = o->d_mask; sa.tiles = o->d_tiles; sa.guides = ctx->d_guides;
  sa.recs = ctx->d_recs; sa.rec_count = ctx->d_counters; sa.rec_capacity = ctx->rec_cap;
  sa.n_guides = pl.n_guides; sa.chrom_index = p.chrom_index; sa.tile_offset = pl.tile_lo; sa.tile_stride = 1;
  aa = AlignArgs{};
  aa.codes = o->d_codes; aa.mask = o->d_mask; aa.runs = o->d_runs; aa.n_runs = (int64_t)ref.runs.size();
  aa.contigs = o->d_contigs; aa.tiles = o->d_tiles; aa.win_base = o->d_win_base; aa.win = o->d_win; aa.guides = ctx->d_guides; aa.recs = ctx->d_recs;
  aa.rec_count = ctx->d_counters; aa.out = ctx->d_raw; aa.out_count = ctx->d_counters + 1; aa.anomalies = ctx->d_counters + 2;
  aa.trace_done = ctx->d_counters + 5; aa.job_count = ctx->d_counters + 6;
  for (int g = 0; g < pl.n_guides; g++) aa.max_guide_len = std::max<int32_t>(aa.max_guide_len, pl.gd[g].L);
  {
    // two jobs per lane group (align_pk_kernel): one protospacer length for all guides of the launch, and every cell a passing
    // alignment can go through -- within +-max|cost| x L of zero -- times four, with a step's cost on top, inside sixteen bits
    bool same_L = true;
    for (int g = 1; g < pl.n_guides; g++) same_L = same_L && pl.gd[g].L == pl.gd[0].L;
    const int64_t big = std::max<int64_t>(std::max<int64_t>(std::abs(pl.sc.match), std::abs(pl.sc.mismatch)), std::max<int64_t>(std::abs(pl.sc.target_gap), std::abs(pl.sc.query_gap)));
    aa.pack16 = (same_L && aa.max_guide_len <= 20 && 4 * big * ((int64_t)aa.max_guide_len + 2) < 30000) ? 1 : 0;
  }
  aa.rec_capacity = ctx->rec_cap; aa.out_capacity = ctx->raw_cap;
  aa.slab = ctx->d_slab; aa.cand_count = ctx->d_counters + 4; aa.items = ctx->d_items; aa.item_count = ctx->d_counters + 3; aa.item_capacity = ctx->item_cap;
  aa.slab_bytes = pl.slab_bytes; aa.slots_per_rec = pl.slots_per_rec; aa.tile_words = (uint32_t)(ref.tile / 16);
  aa.gw_lo = pl.gw_lo; aa.gw_hi = pl.gw_hi;
  aa.sp.window_size = p.window_size; aa.sp.step = pl.step; aa.sp.n_guides = pl.n_guides;
  aa.sp.max_guide_diffs = p.max_guide_diffs; aa.sp.max_pam_mismatches = p.max_pam_mismatches;
  aa.sp.max_gaps = p.max_gaps_between_guide_and_pam;
  aa.sp.max_diffs_filtering = p.max_guide_diffs + p.max_gaps_between_guide_and_pam + p.max_pam_mismatches;   // SGA:249
  aa.sp.match = pl.sc.match; aa.sp.mismatch = pl.sc.mismatch; aa.sp.pam_match = pl.sc.pam_match; aa.sp.pam_mismatch = pl.sc.pam_mismatch;
  aa.sp.query_gap = pl.sc.query_gap; aa.sp.target_gap = pl.sc.target_gap; aa.sp.eqx_by_score = p.eqx_by_score & 1; aa.sp.per_matrix = (p.eqx_by_score >> 1) & 1; aa.sp.chrom_index = p.chrom_index;
}

// Device buffers of one lane for this plan (allocation only).
int lane_prepare(calitas_ctx* ctx, const SearchPlan& pl) {
  uint64_t want = std::max<uint64_t>(1u << 16, std::min<uint64_t>(1u << 20, pl.bases / 8 + 1024));
  uint64_t want_raw = want, want_items = 2 * want;
  if (pl.rec_hint) {   // a dense search (estimate_scan_records): no retry round per contig -- such searches yield ~3 alignments and passing candidates per record
    want = std::max<uint64_t>(want, std::min<uint64_t>(0xFFFFFFF0ull, pl.rec_hint + pl.rec_hint / 4 + 4096));
    want_raw = std::min<uint64_t>(0xFFFFFFF0ull, want * 7 / 2);
    want_items = std::min<uint64_t>(0xFFFFFFF0ull, want * 4);
  }
  return ensure_buffers(ctx, std::max<uint32_t>(ctx->rec_cap, (uint32_t)want), std::max<uint32_t>(ctx->raw_cap, (uint32_t)want_raw), pl.slab_per_rec,
                        std::max<uint32_t>(ctx->item_cap, (uint32_t)want_items));
}

// Contigs that are absent here (refpack.hpp: a process of a multi-GPU job holds what its window range touches): a search must not need
// one.  Checked where a plan is about to run -- the callers of a ranged search plan the whole job first and narrow it afterwards.
int check_resident(calitas_ctx* ctx, const SearchPlan& pl) {
  const PackedRef& ref = ref_owner(ctx)->ref;
  if (ref.absent.empty()) return CALITAS_OK;
  int bad = -1;
  if (pl.p.chrom_index >= 0) {
    if (ref.is_absent((size_t)pl.p.chrom_index)) bad = pl.p.chrom_index;
  } else {
    const std::vector<uint64_t> wb = window_prefix(ref, pl.step);
    for (size_t c = 0; c < ref.contigs.size() && bad < 0; c++) {
      const uint64_t t0 = ref.contigs[c].gbase / ref.tile;          // (a chunked call's lanes: contig ranges by tiles)
      if (ref.is_absent(c) && std::max(pl.gw_lo, wb[c]) < std::min(pl.gw_hi, wb[c + 1]) && t0 >= pl.tile_lo && t0 < (uint64_t)pl.tile_lo + pl.n_tiles) bad = (int)c;
    }
  }
  if (bad < 0) return CALITAS_OK;
  return calitas_fail(ctx, CALITAS_EINVAL, "contig " + ref.names[(size_t)bad] + " is not resident in this context (it was given without bases): "
                                           "search a window range that leaves it out");
}

// Contig ranges [first, last) of a chunked search: cut at contig boundaries (removeOverlaps groups and the final sort never
// cross a contig), sized by `weights`.
std::vector<std::pair<int, int>> chunk_ranges(const PackedRef& ref, const std::vector<double>& weights) {
  const int n = (int)ref.contigs.size();
  std::vector<std::pair<int, int>> out;
  double wsum = 0;
  for (double w : weights) wsum += w;
  uint64_t total = ref.total_bases, acc = 0;
  double target = 0;
  int first = 0;
  size_t k = 0;
  for (int c = 0; c < n && k + 1 < weights.size(); c++) {
    acc += ref.contigs[c].len;
    const double goal = (target + weights[k]) / wsum * (double)total;
    const uint64_t next = c + 1 < n ? ref.contigs[c + 1].len : 0;
    // close the chunk after contig c when that lands nearer to the goal than taking one more contig would
    if ((double)acc >= goal || (double)acc + (double)next / 2 > goal) {
      if (c + 1 < n) { out.emplace_back(first, c + 1); first = c + 1; target += weights[k]; k++; }
    }
  }
  out.emplace_back(first, n);
  return out;
}

// The plan of a stretch: bins, the windows their contexts reach, the tiles those windows lie in.
bool plan_owned_range(const calitas_ctx* ctx, SearchPlan& pl, uint64_t first, uint64_t count) {
  const PackedRef& ref = ctx->ref;
  const int nc = (int)ref.contigs.size();
  if (!pl.bin_shift || ctx->bin_base.size() != (size_t)nc + 1) return false;
  const std::vector<uint64_t> wb = window_prefix(ref, pl.step);
  if (count == 0 || first + count > wb[nc]) return false;
  int c_lo = 0, c_hi = 0;
  uint64_t p_lo = 0, p_hi = 0;
  window_start(wb, pl.step, first, c_lo, p_lo);
  window_start(wb, pl.step, first + count, c_hi, p_hi);
  // a stretch that starts with the first window of a contig owns the contig from base 0, one that ends at a contig's first window
  // owns the contig before it to its end -- (c, 0) keys say exactly that
  pl.owned = true;
  pl.own_lo = ((uint64_t)c_lo << 32) | p_lo;
  pl.own_hi = ((uint64_t)c_hi << 32) | p_hi;
  // last owned position
  int c_last = c_hi;
  uint64_t p_last = p_hi;
  if (p_hi == 0) { c_last = c_hi - 1; while (c_last > c_lo && ref.contigs[c_last].len == 0) c_last--; p_last = ref.contigs[c_last].len; }
  if (p_last > 0) p_last--;
  uint32_t b_lo = ctx->bin_base[c_lo] + (uint32_t)(p_lo >> pl.bin_shift), b_hi = ctx->bin_base[c_last] + (uint32_t)(p_last >> pl.bin_shift);
  if (b_lo > ctx->bin_base[c_lo]) b_lo--;                      // one bin of context on either side, inside the contig
  if (b_hi + 1 < ctx->bin_base[c_last + 1]) b_hi++;
  pl.bin_first = b_lo; pl.n_bins = b_hi - b_lo + 1;
  // the windows that start in those bins: the context of the first owned bin (two windows to the left) lies in the bin before it, that
  // of the last one (the longest hit to the right) in the bin behind it (binned.hip) -- and trace_kernel lists an alignment in the
  // bin its window starts in, which must be one of the lane's
  const int64_t ctx_lo = (int64_t)((uint64_t)(b_lo - ctx->bin_base[c_lo]) << pl.bin_shift);
  const uint64_t ctx_hi = std::min<uint64_t>(ref.contigs[c_last].len, ((uint64_t)(b_hi - ctx->bin_base[c_last]) + 1) << pl.bin_shift);
  const uint64_t k_lo = ((uint64_t)ctx_lo + (uint64_t)pl.step - 1) / (uint64_t)pl.step;
  const uint64_t nw_last = wb[c_last + 1] - wb[c_last];
  const uint64_t k_hi = ctx_hi == 0 ? 0 : std::min<uint64_t>(nw_last, (ctx_hi - 1) / (uint64_t)pl.step + 1);
  pl.gw_lo = std::min(wb[c_lo] + k_lo, wb[c_lo + 1]);
  pl.gw_hi = wb[c_last] + k_hi;
  if (pl.gw_hi < pl.gw_lo) pl.gw_hi = pl.gw_lo;
  // tiles those windows lie in
  const uint64_t g_lo = ref.contigs[c_lo].gbase + (uint64_t)ctx_lo;
  const uint64_t g_hi = ref.contigs[c_last].gbase + std::min<uint64_t>(ref.contigs[c_last].len, ctx_hi + (uint64_t)pl.p.window_size);
  pl.tile_lo = (uint32_t)(g_lo / ref.tile);
  pl.n_tiles = (uint32_t)((g_hi + ref.tile - 1) / ref.tile) - pl.tile_lo;
  uint64_t bases = 0;
  for (int c = c_lo; c <= c_last; c++) bases += ref.contigs[c].len;
  if (c_lo == c_last) bases = std::min<uint64_t>(ref.contigs[c_lo].len, ctx_hi + (uint64_t)pl.p.window_size) - (uint64_t)ctx_lo;
  pl.bases = bases;
  pl.win_lo = pl.gw_lo; pl.win_n = pl.gw_hi - pl.gw_lo;
  return true;
}

}  // namespace calitas
