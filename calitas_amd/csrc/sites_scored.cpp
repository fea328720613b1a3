// sites_scored.cpp -- the listings that carry a score per site.  calitas_find_sites_scored / calitas_find_sites_scored_host: the
// activity model's checks and its folded table, the per-site score base by base, and the driver of activity.hip's kernels.
// calitas_find_sites_microhomology / calitas_find_sites_microhomology_host: the model's checks, the score of one site as a diagonal
// walk over letters, and the driver of microhomology.hip's kernels.  Both run behind the site kernel's two passes with the correction
// of records and scores beside a U, and both twins and both drivers are one template each over a scoring.  No reference counterpart.
#include "sites_work.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>

// ---- what the two share.  A scoring S (ActivityScoring, MhScoring below) is a call's plan seen through one interface: ----
//   Score, DevScore      what the caller gets per site and what the kernels store, the same bytes
//   NAME, NO_ROOM        the entry point's name for internal errors, and its text for records that do not fit the device
//   THREADS, blocks(n)   the score kernel's workgroup size and the workgroups for n records
//   site(), threshold()  the plan of the site listing; whether records are dropped, so that the kept ones are compacted
//   at, passes           the host's score of one site (*flagged: the kernel leaves it to the host) and whether a score is kept
//   host_decides(v)      the kernel's mark in a downloaded score: the host scores this window
//   bufs(w)              the listing's buffers in the context's scratch
//   prepare, score       what the score kernel needs beside the records, made before the second pass is queued; the kernel's launch
//   compact              the launch that moves the kept records and scores together

namespace {

// the two blocks of the call: room for n records and n scores (at least one each)
template <typename Score>
int scored_blocks_alloc(calitas_ctx* c, uint64_t n, calitas_site_t** sites, Score** scores) {
  *sites = (calitas_site_t*)calitas_out_alloc(std::max<uint64_t>(1, n) * sizeof(calitas_site_t));
  *scores = (Score*)calitas_out_alloc(std::max<uint64_t>(1, n) * sizeof(Score));
  if (*sites && *scores) return CALITAS_OK;
  calitas_free(*sites); calitas_free(*scores);
  *sites = nullptr; *scores = nullptr;
  return calitas_fail(c, CALITAS_EINVAL, "out of memory");
}

// what the caller gets: the blocks, or the number alone
template <typename Score>
void scored_hand_over(calitas_site_t* block, Score* block_scores, uint64_t n, calitas_site_t** sites, Score** scores, uint64_t* n_sites) {
  *n_sites = n;
  if (sites) { *sites = block; *scores = block_scores; }
  else { calitas_free(block); calitas_free(block_scores); }
}

// the host twin of a planned call: every site of the region base by base, scored and kept by the scoring
template <typename S>
int scored_host_twin(calitas_ctx* c, const S& sc, uint64_t start, uint64_t end, calitas_site_t** sites, typename S::Score** scores, uint64_t* n_sites) {
  const SiteCall& site = sc.site();
  std::vector<calitas_site_t> found;
  for (int i = site.c_first; i <= site.c_last; i++) {
    const uint64_t len = c->ref.contigs[(size_t)i].len;
    host_sites(c->ref, site.tab.pat, site.filter, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
  }
  calitas_site_t* block = nullptr;
  typename S::Score* block_scores = nullptr;
  if (int rc = scored_blocks_alloc(c, found.size(), &block, &block_scores)) return rc;
  uint64_t n = 0;
  for (const calitas_site_t& s : found) {
    bool flagged = false;
    const typename S::Score score = sc.at(c->ref, s, &flagged);
    if (!sc.passes(score)) continue;
    block[n] = s; block_scores[n] = score; n++;
  }
  scored_hand_over(block, block_scores, n, sites, scores, n_sites);
  return CALITAS_OK;
}

// The device's side of a planned call on a context with a device: calitas_find_sites' two passes as they are, a score per record of
// d_out, with a threshold the kept ones moved together, one copy-back, and the correction of records and scores beside a U.
template <typename S>
int scored_listing(calitas_ctx* ctx, S& sc, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, typename S::Score** scores,
                   uint64_t* n_sites) {
  typedef typename S::Score Score;
  typedef typename S::DevScore DevScore;
  static_assert(sizeof(Score) == sizeof(DevScore), "the kernel stores the contract's values");
  const SiteCall& site = sc.site();
  const bool filtered = site.filter != nullptr;
  const PackedRef& ref = ctx->ref;
  calitas_site_t* block = nullptr;
  Score* block_scores = nullptr;
  if (ref.contigs.empty()) {                      // nothing to scan
    if (int rc = scored_blocks_alloc(ctx, 0, &block, &block_scores)) return rc;
    scored_hand_over(block, block_scores, 0, sites, scores, n_sites);
    return CALITAS_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;
  ScoredBufs<DevScore>& b = S::bufs(w);

  // calitas_find_sites' two passes as they are; the records stay in d_out
  SitesArgs a{};
  if (int rc = site_launch(ctx, site, chrom_index, start, end, w, a)) return rc;
  uint64_t n_dev = 0;
  if (int rc = sites_first_pass(ctx, site, w, a, launch_sites_count, &n_dev)) return rc;
  if (n_dev / S::THREADS >= 0x7FFFFFFFull) return calitas_fail(ctx, CALITAS_ENOMEM, S::NO_ROOM);
  const bool threshold = sc.threshold();
  uint64_t n_kept = n_dev;
  const SiteRecord* d_recs = nullptr;
  const DevScore* d_scores = nullptr;
  if (n_dev) {
    if (int rc = sites_out_room(ctx, w, a, n_dev, S::NO_ROOM)) return rc;
    if (int rc = no_room_unless(ctx, b.scores.grow(n_dev), S::NO_ROOM)) return rc;
    const uint32_t wgs = S::blocks(n_dev);
    if (threshold) {
      HIP_TRY(ctx, b.count.grow((size_t)wgs + 1));
      HIP_TRY(ctx, b.off.grow((size_t)wgs + 1));
    }
    if (int rc = sc.prepare(ctx, w)) return rc;
    HIP_TRY(ctx, launch_sites_write(a, filtered, ctx->stream));
    if (int rc = sc.score(ctx, w, n_dev, threshold ? b.count.p : nullptr)) return rc;
    d_recs = w->d_out.p; d_scores = b.scores.p;
    if (threshold) {
      HIP_TRY(ctx, launch_sites_offsets(b.count.p, b.off.p, wgs, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(&n_kept, b.off.p + wgs, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));             // (what prepare made on the host is done with as well)
      if (n_kept > n_dev) return calitas_fail(ctx, CALITAS_EHIP, std::string(S::NAME) + ": more records kept than written (internal error)");
      if (int rc = no_room_unless(ctx, b.out.grow(n_kept), S::NO_ROOM)) return rc;
      if (int rc = no_room_unless(ctx, b.out_scores.grow(n_kept), S::NO_ROOM)) return rc;
      if (n_kept) HIP_TRY(ctx, sc.compact(b, w->d_out.p, n_dev, n_kept, ctx->stream));
      d_recs = b.out.p; d_scores = b.out_scores.p;
    }
  }

  // a U is a T to a site and an exception base to the kernels: the sites the site kernel did not see, and what it has in their place
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, site, start, end, with_u, kernel_has);
  if (int rc = scored_blocks_alloc(ctx, n_kept + with_u.size(), &block, &block_scores)) return rc;
  int rc = CALITAS_OK;
  do {   // (one exit that releases the blocks)
    hipError_t e = hipSuccess;
    if ((n_kept && ((e = hipMemcpyAsync(block, d_recs, n_kept * sizeof(SiteRecord), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess ||
                    (e = hipMemcpyAsync(block_scores, d_scores, n_kept * sizeof(DevScore), hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess)) ||
        (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) {
      rc = calitas_fail(ctx, CALITAS_EHIP, std::string(S::NAME) + ": " + hipGetErrorString(e));
      break;
    }
    // A record the site kernel has beside a U is in the block exactly when its own score passes or its window was left to the host
    // (both lists are in output order); it goes.
    bool gaps = false;
    calitas_site_t* const end_dev = block + n_kept;
    for (const calitas_site_t& s : kernel_has) {
      bool flagged = false;
      const Score score = sc.at(ref, s, &flagged);
      const bool expected = flagged || sc.passes(score);
      calitas_site_t* at = std::lower_bound(block, end_dev, s, site_less);
      const bool there = at != end_dev && std::memcmp(at, &s, sizeof(s)) == 0;
      if (there != expected) { rc = calitas_fail(ctx, CALITAS_EHIP, std::string(S::NAME) + ": the records beside a U are not the ones the host expects (internal error)"); break; }
      if (there) { at->contig_index = -1; gaps = true; }
    }
    if (rc) break;
    // the windows the kernel left to the host: scored base by base, dropped when below the threshold
    for (uint64_t i = 0; i < n_kept; i++) {
      if (!S::host_decides(block_scores[i]) || block[i].contig_index < 0) continue;
      bool flagged = false;
      const Score score = sc.at(ref, block[i], &flagged);
      if (sc.passes(score)) block_scores[i] = score;
      else { block[i].contig_index = -1; gaps = true; }
    }
    uint64_t n = n_kept;
    if (gaps) {
      n = 0;
      for (uint64_t i = 0; i < n_kept; i++)
        if (block[i].contig_index >= 0) { block[n] = block[i]; block_scores[n] = block_scores[i]; n++; }
    }
    // the sites with a U in their footprint come in with the host's scores, each at its place: a merge from the back that ends
    // with the last of them
    std::vector<Score> u_scores;
    size_t n_in = 0;
    for (const calitas_site_t& s : with_u) {
      bool flagged = false;
      const Score score = sc.at(ref, s, &flagged);
      if (!sc.passes(score)) continue;
      with_u[n_in++] = s; u_scores.push_back(score);
    }
    for (uint64_t i = n, j = n_in, k = n + n_in; j > 0; k--) {
      if (i > 0 && site_less(with_u[j - 1], block[i - 1])) { block[k - 1] = block[i - 1]; block_scores[k - 1] = block_scores[i - 1]; i--; }
      else { block[k - 1] = with_u[j - 1]; block_scores[k - 1] = u_scores[j - 1]; j--; }
    }
    scored_hand_over(block, block_scores, n + n_in, sites, scores, n_sites);
  } while (0);
  if (rc) { calitas_free(block); calitas_free(block_scores); }
  return rc;
}

}  // namespace

// ---- calitas_find_sites_scored: every site's on-target activity under a linear model of its sequence context ----

namespace {

struct ActivityCall {
  SiteCall site;
  const calitas_activity_model_t* model = nullptr;
  int L = 0, W = 0;
  int32_t min_score = CALITAS_ACTIVITY_NONE;
  bool threshold = false;            // min_score != CALITAS_ACTIVITY_NONE: sites below it, the unscored ones among them, are dropped
};

// checked in this order: what calitas_find_sites_filtered checks (plan_sites), then the model, field by field
int plan_activity(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_activity_model_t* model,
                  int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end, ActivityCall& call) {
  static_assert(CALITAS_ACTIVITY_MAX_FLANK + MAX_L + CALITAS_ACTIVITY_MAX_FLANK == ACTIVITY_MAX_W, "the kernel's three words hold the widest window");
  static_assert(ACTIVITY_NONE == CALITAS_ACTIVITY_NONE, "the kernel stores the contract's value");
  if (int rc = plan_sites(c, pattern, filter, chrom_index, start, end, call.site)) return rc;
  const int L = call.site.tab.pat.proto_len;
  if (!model) return calitas_fail(c, CALITAS_EINVAL, "activity model: model is NULL");
  if (!model->single) return calitas_fail(c, CALITAS_EINVAL, "activity model: single is NULL");
  if (!model->pair) return calitas_fail(c, CALITAS_EINVAL, "activity model: pair is NULL");
  if (!model->gc) return calitas_fail(c, CALITAS_EINVAL, "activity model: gc is NULL");
  if (model->protospacer_length != L)
    return calitas_fail(c, CALITAS_EINVAL, "activity model: protospacer_length is " + std::to_string(model->protospacer_length) + ", the pattern's protospacer has " + std::to_string(L) + " bases");
  if (model->up < 0 || model->up > CALITAS_ACTIVITY_MAX_FLANK) return calitas_fail(c, CALITAS_EINVAL, "activity model: up is " + std::to_string(model->up) + ": it is 0 .. 16");
  if (model->down < 0 || model->down > CALITAS_ACTIVITY_MAX_FLANK) return calitas_fail(c, CALITAS_EINVAL, "activity model: down is " + std::to_string(model->down) + ": it is 0 .. 16");
  if (model->link < 0 || model->link > 1) return calitas_fail(c, CALITAS_EINVAL, "activity model: link is " + std::to_string(model->link) + ": it is 0 (identity) or 1 (logistic)");
  const int W = model->up + L + model->down;
  const auto outside = [](int32_t v) { return v < -CALITAS_ACTIVITY_MAX_WEIGHT || v > CALITAS_ACTIVITY_MAX_WEIGHT; };
  if (outside(model->intercept)) return calitas_fail(c, CALITAS_EINVAL, "activity model: intercept lies outside +-1048576 (16.0)");
  const struct { const char* name; const int32_t* at; int n; } tables[3] = {{"single", model->single, 4 * W}, {"pair", model->pair, 16 * (W - 1)}, {"gc", model->gc, L + 1}};
  for (const auto& t : tables)
    for (int i = 0; i < t.n; i++)
      if (outside(t.at[i])) return calitas_fail(c, CALITAS_EINVAL, std::string("activity model: ") + t.name + "[" + std::to_string(i) + "] lies outside +-1048576 (16.0)");
  call.model = model; call.L = L; call.W = W; call.min_score = min_score; call.threshold = min_score != CALITAS_ACTIVITY_NONE;
  return CALITAS_OK;
}

// The contract on one site, base by base: the window's letters from PackedRef::base_upper, turned as the guide reads, the three sums
// from the caller's tables as they stand.  *flagged: the window lies in the contig and holds an exception base -- a U among them --
// which is when the kernel leaves the site to the host.
int32_t activity_at(const PackedRef& ref, const calitas_activity_model_t& m, const calitas_site_t& s, bool* flagged) {
  const int L = m.protospacer_length, W = m.up + L + m.down;
  const bool minus = s.strand == '-';
  const ContigInfo& ci = ref.contigs[(size_t)s.contig_index];
  const int64_t left = (int64_t)s.protospacer_start - (minus ? m.down : m.up);
  *flagged = false;
  if (left < 0 || (uint64_t)(left + W) > ci.len) return CALITAS_ACTIVITY_NONE;
  int code[ACTIVITY_MAX_W];                                    // the context, 5' to 3' as the guide reads
  bool plain = true;
  for (int j = 0; j < W; j++) {
    const uint64_t g = ci.gbase + (uint64_t)(left + j);
    if ((ref.mask[g >> 5] >> (g & 31)) & 1u) *flagged = true;
    const char ch = ref.base_upper(g);
    const int c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : (ch == 'T' || ch == 'U') ? 3 : -1;
    if (c < 0) plain = false;
    code[minus ? W - 1 - j : j] = minus ? 3 - c : c;
  }
  if (!plain) return CALITAS_ACTIVITY_NONE;
  int32_t sum = m.intercept;
  int gc = 0;
  for (int i = 0; i < W; i++) sum += m.single[4 * i + code[i]];
  for (int i = 0; i + 1 < W; i++) sum += m.pair[16 * i + 4 * code[i] + code[i + 1]];
  for (int i = m.up; i < m.up + L; i++) gc += code[i] == 1 || code[i] == 2;
  return sum + m.gc[gc];
}

inline bool activity_passes(const ActivityCall& call, int32_t score) { return score >= call.min_score; }   // (NONE passes NONE alone)

struct ActivityScoring {
  typedef int32_t Score;
  typedef int32_t DevScore;
  static constexpr const char* NAME = "calitas_find_sites_scored";
  static constexpr const char* NO_ROOM = "the site records and their scores do not fit the device: list the region in pieces";
  static constexpr int THREADS = ACTIVITY_THREADS;
  const ActivityCall& call;
  std::vector<int32_t> table;                     // the model as the kernel reads it (uploaded from here: it lives until the call's last wait)

  const SiteCall& site() const { return call.site; }
  bool threshold() const { return call.threshold; }
  int32_t at(const PackedRef& ref, const calitas_site_t& s, bool* flagged) const { return activity_at(ref, *call.model, s, flagged); }
  bool passes(int32_t score) const { return activity_passes(call, score); }
  static bool host_decides(int32_t score) { return score == ACTIVITY_HOST_DECIDES; }
  static ScoredBufs<int32_t>& bufs(SitesWork* w) { return w->act; }
  static uint32_t blocks(uint64_t n) { return activity_blocks(n); }

  // the table: single folded into pair (integer sums: exact), the last position's single, gc, the intercept
  int prepare(calitas_ctx* ctx, SitesWork* w) {
    HIP_TRY(ctx, w->d_act_table.grow(ACTIVITY_TABLE_MAX_WORDS));
    const calitas_activity_model_t* model = call.model;
    const int W = call.W, L = call.L;
    table.resize(activity_table_words(L, W));
    for (int i = 0; i + 1 < W; i++)
      for (int ab = 0; ab < 16; ab++) table[(size_t)(16 * i + ab)] = model->pair[16 * i + ab] + model->single[4 * i + (ab >> 2)];
    int32_t* tail = table.data() + 16 * (W - 1);
    for (int b = 0; b < 4; b++) tail[b] = model->single[4 * (W - 1) + b];
    for (int g = 0; g <= L; g++) tail[4 + g] = model->gc[g];
    tail[4 + L + 1] = model->intercept;
    return CALITAS_OK;
  }
  int score(calitas_ctx* ctx, SitesWork* w, uint64_t n_dev, uint32_t* wg_kept) {
    ActivityArgs s{};
    s.planes = ctx->d_planes; s.mask = ctx->d_mask; s.contigs = ctx->d_contigs; s.table = w->d_act_table.p; s.recs = w->d_out.p; s.scores = w->act.scores.p;
    s.wg_kept = wg_kept;
    s.n = n_dev; s.n_words = ctx->ref.total_packed / 32; s.n_contigs = (int32_t)ctx->ref.contigs.size(); s.L = call.L; s.up = call.model->up; s.down = call.model->down;
    s.min_score = call.min_score;
    HIP_TRY(ctx, hipMemcpyAsync(w->d_act_table.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_activity_score(s, ctx->stream));
    return CALITAS_OK;
  }
  hipError_t compact(ScoredBufs<int32_t>& b, const SiteRecord* recs, uint64_t n_dev, uint64_t n_kept, hipStream_t stream) const {
    return launch_activity_compact(recs, b.scores.p, n_dev, call.min_score, b.off.p, b.out.p, b.out_scores.p, n_kept, stream);
  }
};

}  // namespace

int calitas_find_sites_scored_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                        const calitas_activity_model_t* model, int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end,
                                        calitas_site_t** sites, int32_t** scores, uint64_t* n_sites) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  ActivityCall call;
  if (int rc = plan_activity(c, pattern, filter, model, min_score, chrom_index, start, end, call)) return rc;
  return scored_host_twin(c, ActivityScoring{call, {}}, start, end, sites, scores, n_sites);
}

int calitas_find_sites_scored_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_activity_model_t* model,
                                   int32_t min_score, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites, int32_t** scores,
                                   uint64_t* n_sites) {
  ActivityCall call;
  if (int rc = plan_activity(ctx, pattern, filter, model, min_score, chrom_index, start, end, call)) return rc;
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_sites_scored needs a GPU (there is no CPU fallback; calitas_find_sites_scored_host is the host twin)");
  ActivityScoring sc{call, {}};
  return scored_listing(ctx, sc, chrom_index, start, end, sites, scores, n_sites);
}

// ---- calitas_find_sites_microhomology: every site's microhomology score and the out-of-frame share of it ----

namespace {

struct MhCall {
  SiteCall site;
  const calitas_mh_model_t* model = nullptr;
  int L = 0, W = 0;
  uint32_t permille = 0;             // 0: every site is kept; else mh_kept decides
};

// checked in this order: what calitas_find_sites_filtered checks (plan_sites), then the model, field by field, then the threshold
int plan_microhomology(calitas_ctx* c, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_mh_model_t* model,
                       int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end, MhCall& call) {
  static_assert(2 * CALITAS_MH_MAX_SIDE == MH_MAX_W, "the kernel's three words hold the widest window");
  static_assert(MH_NONE == CALITAS_MH_NONE && sizeof(MhScore) == sizeof(calitas_mh_score_t), "the kernel stores the contract's values");
  if (int rc = plan_sites(c, pattern, filter, chrom_index, start, end, call.site)) return rc;
  const int L = call.site.tab.pat.proto_len;
  if (!model) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: model is NULL");
  if (!model->weight) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: weight is NULL");
  if (model->left < 1 || model->left > CALITAS_MH_MAX_SIDE) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: left is " + std::to_string(model->left) + ": it is 1 .. 32");
  if (model->right < 1 || model->right > CALITAS_MH_MAX_SIDE) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: right is " + std::to_string(model->right) + ": it is 1 .. 32");
  if (model->cut_offset < 0 || model->cut_offset > L)
    return calitas_fail(c, CALITAS_EINVAL, "microhomology model: cut_offset is " + std::to_string(model->cut_offset) + ": it is 0 .. " + std::to_string(L) + ", the protospacer's length");
  if (model->min_length < 2 || model->min_length > 8) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: min_length is " + std::to_string(model->min_length) + ": it is 2 .. 8");
  const int W = model->left + model->right;
  for (int d = 1; d < W; d++)
    if (model->weight[d - 1] > CALITAS_MH_MAX_WEIGHT) return calitas_fail(c, CALITAS_EINVAL, "microhomology model: weight[" + std::to_string(d - 1) + "] lies above 65536 (1.0)");
  if (permille < 0 || permille > 1000) return calitas_fail(c, CALITAS_EINVAL, "min_out_of_frame_permille is " + std::to_string(permille) + ": it is 0 .. 1000");
  call.model = model; call.L = L; call.W = W; call.permille = (uint32_t)permille;
  return CALITAS_OK;
}

const calitas_mh_score_t MH_UNSCORED = {CALITAS_MH_NONE, CALITAS_MH_NONE};

// The contract on one site, letter by letter: the window's letters from PackedRef::base_upper, turned as the guide reads, then every
// diagonal d walked from lo(d) to hi(d) with the current run's length and its G + C count.  *flagged: the window lies in the contig
// and holds an exception base -- a U among them -- which is when the kernel leaves the site to the host.
calitas_mh_score_t mh_at(const PackedRef& ref, const calitas_mh_model_t& m, int L, const calitas_site_t& s, bool* flagged) {
  const int left = m.left, right = m.right, W = left + right;
  const bool minus = s.strand == '-';
  const ContigInfo& ci = ref.contigs[(size_t)s.contig_index];
  const int64_t cut = (int64_t)s.protospacer_start + (minus ? L - m.cut_offset : m.cut_offset);
  const int64_t first = cut - (minus ? right : left);
  *flagged = false;
  if (first < 0 || (uint64_t)(first + W) > ci.len) return MH_UNSCORED;
  char x[MH_MAX_W];                                            // the window, 5' to 3' as the guide reads
  bool plain = true;
  for (int j = 0; j < W; j++) {
    const uint64_t g = ci.gbase + (uint64_t)(first + j);
    if ((ref.mask[g >> 5] >> (g & 31)) & 1u) *flagged = true;
    char ch = ref.base_upper(g);
    if (ch == 'U') ch = 'T';
    if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') plain = false;
    if (minus) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
    x[minus ? W - 1 - j : j] = ch;
  }
  if (!plain) return MH_UNSCORED;
  calitas_mh_score_t out = {0, 0};
  for (int d = 1; d < W; d++) {
    const int from = std::max(0, left - d), to = std::min(left, W - d);
    uint32_t units = 0;                                        // the sum of k + g over the diagonal's runs
    int k = 0, g = 0;
    for (int i = from; i <= to; i++) {
      if (i < to && x[i] == x[i + d]) { k++; g += x[i] == 'G' || x[i] == 'C'; continue; }
      if (k >= m.min_length) units += (uint32_t)(k + g);
      k = 0; g = 0;
    }
    const uint32_t term = m.weight[d - 1] * units;
    out.total_q16 += term;
    if (d % 3 != 0) out.out_of_frame_q16 += term;
  }
  return out;
}

inline bool mh_passes(const MhCall& call, const calitas_mh_score_t& v) {
  if (call.permille == 0) return true;
  return v.total_q16 != CALITAS_MH_NONE && v.total_q16 > 0 && (uint64_t)v.out_of_frame_q16 * 1000u >= (uint64_t)call.permille * v.total_q16;
}


struct MhScoring {
  typedef calitas_mh_score_t Score;
  typedef MhScore DevScore;
  static constexpr const char* NAME = "calitas_find_sites_microhomology";
  static constexpr const char* NO_ROOM = "the site records and their microhomology scores do not fit the device: list the region in pieces";
  static constexpr int THREADS = MH_THREADS;
  const MhCall& call;

  const SiteCall& site() const { return call.site; }
  bool threshold() const { return call.permille != 0; }
  calitas_mh_score_t at(const PackedRef& ref, const calitas_site_t& s, bool* flagged) const { return mh_at(ref, *call.model, call.L, s, flagged); }
  bool passes(const calitas_mh_score_t& score) const { return mh_passes(call, score); }
  static bool host_decides(const calitas_mh_score_t& score) { return score.total_q16 == MH_NONE && score.out_of_frame_q16 == MH_HOST_DECIDES; }
  static ScoredBufs<MhScore>& bufs(SitesWork* w) { return w->mh; }
  static uint32_t blocks(uint64_t n) { return mh_blocks(n); }

  int prepare(calitas_ctx*, SitesWork*) { return CALITAS_OK; }   // (the weights travel in the argument block)
  int score(calitas_ctx* ctx, SitesWork* w, uint64_t n_dev, uint32_t* wg_kept) {
    const calitas_mh_model_t* model = call.model;
    MhArgs s{};
    s.planes = ctx->d_planes; s.mask = ctx->d_mask; s.contigs = ctx->d_contigs; s.recs = w->d_out.p; s.scores = w->mh.scores.p;
    s.wg_kept = wg_kept;
    s.n = n_dev; s.n_words = ctx->ref.total_packed / 32; s.n_contigs = (int32_t)ctx->ref.contigs.size(); s.L = call.L; s.left = model->left; s.right = model->right;
    s.cut = model->cut_offset; s.min_length = model->min_length; s.permille = call.permille;
    for (int d = 1; d < call.W; d++) s.weight[d - 1] = model->weight[d - 1];
    HIP_TRY(ctx, launch_mh_score(s, ctx->stream));
    return CALITAS_OK;
  }
  hipError_t compact(ScoredBufs<MhScore>& b, const SiteRecord* recs, uint64_t n_dev, uint64_t n_kept, hipStream_t stream) const {
    return launch_mh_compact(recs, b.scores.p, n_dev, call.permille, b.off.p, b.out.p, b.out_scores.p, n_kept, stream);
  }
};

}  // namespace

int calitas_find_sites_microhomology_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter,
                                               const calitas_mh_model_t* model, int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end,
                                               calitas_site_t** sites, calitas_mh_score_t** scores, uint64_t* n_sites) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  MhCall call;
  if (int rc = plan_microhomology(c, pattern, filter, model, permille, chrom_index, start, end, call)) return rc;
  return scored_host_twin(c, MhScoring{call}, start, end, sites, scores, n_sites);
}

int calitas_find_sites_microhomology_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, const calitas_site_filter_t* filter, const calitas_mh_model_t* model,
                                          int32_t permille, int32_t chrom_index, uint64_t start, uint64_t end, calitas_site_t** sites,
                                          calitas_mh_score_t** scores, uint64_t* n_sites) {
  MhCall call;
  if (int rc = plan_microhomology(ctx, pattern, filter, model, permille, chrom_index, start, end, call)) return rc;
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_find_sites_microhomology needs a GPU (there is no CPU fallback; calitas_find_sites_microhomology_host is the host twin)");
  MhScoring sc{call};
  return scored_listing(ctx, sc, chrom_index, start, end, sites, scores, n_sites);
}
