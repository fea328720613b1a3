// sites_copies.cpp -- calitas_count_copies / calitas_count_copies_host: the query keys and their table, the host twin and the driver of
// the copies kernel.  calitas_count_near / calitas_count_near_host: the pieces' bucket tables, the host twin (plain Hamming distances, no
// buckets) and the driver of the near kernel.  calitas_score_near / calitas_score_near_host: the same driver with the model's packed
// table behind the offsets and rows of M + 3 counters, the host twin (the score letter by letter from the caller's table) and the
// correction of sums and maxima around a U.  calitas_list_near / calitas_list_near_host: the near driver for the counts, the layout of
// a stretch of records per distinct query, the pass's second run and the order kernel (near_list.hip), the patch of the stretches
// beside a U, and the host twin (every pair a record, every stretch through std::sort).  No reference counterpart.
#include "sites_work.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <unordered_map>

// ---- calitas_count_copies: how often a guide's protospacer, or its PAM-proximal seed, stands next to a PAM ----

namespace {

constexpr uint64_t COPIES_MAX_QUERIES = 1ull << 24;

struct CopiesCall {
  SiteCall site;
  int L = 0, K = 0;
  std::vector<uint64_t> keys;                        // the distinct query keys, in the order of their first query
  std::vector<uint32_t> of_query;                    // per query: its key's index in `keys`
  std::unordered_map<uint64_t, uint32_t> index;      // key -> index in `keys`
};

// The arguments both implementations share, checked in this order: the pattern and the region (plan_sites), key_length, the number of
// queries, their letters.
int plan_copies(calitas_ctx* c, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start, uint64_t end, const char* queries,
                uint64_t n_queries, CopiesCall& call) {
  if (int rc = plan_sites(c, pattern, nullptr, chrom_index, start, end, call.site)) return rc;
  call.L = call.site.tab.pat.proto_len;
  if (key_length < 0 || key_length > call.L)
    return calitas_fail(c, CALITAS_EINVAL, "key_length is " + std::to_string(key_length) + ": it is 1 .. the protospacer's length (" + std::to_string(call.L) + "), or 0 for that length");
  call.K = key_length == 0 ? call.L : key_length;
  if (n_queries > COPIES_MAX_QUERIES) return calitas_fail(c, CALITAS_EINVAL, "n_queries exceeds 16777216 (2^24): count the queries in pieces");
  const size_t K = (size_t)call.K;
  call.of_query.resize((size_t)n_queries);
  call.index.reserve((size_t)n_queries);
  for (uint64_t q = 0; q < n_queries; q++) {
    uint32_t lo = 0, hi = 0;
    for (size_t i = 0; i < K; i++) {
      const unsigned char ch = (unsigned char)queries[q * K + i];
      const int set = iupac_mask(ch);
      if (set != 1 && set != 2 && set != 4 && set != 8)
        return calitas_fail(c, CALITAS_EINVAL, "queries[" + std::to_string(q) + "] holds a letter outside ACGTUacgtu at position " + std::to_string(i));
      const uint32_t code = set == 1 ? 0u : set == 2 ? 1u : set == 4 ? 2u : 3u;
      lo |= (code & 1u) << i; hi |= (code >> 1) << i;
    }
    const uint64_t key = copies_key(lo, hi, call.K, call.K, false, false);     // a guide of K bases on '+', all of it
    const auto at = call.index.emplace(key, (uint32_t)call.keys.size());
    if (at.second) call.keys.push_back(key);
    call.of_query[(size_t)q] = at.first->second;
  }
  return CALITAS_OK;
}

// the key of the site whose protospacer starts at p of the contig at gbase, base by base (a U is a T)
uint64_t key_at(const PackedRef& ref, uint64_t gbase, int64_t p, const CopiesCall& call, bool minus) {
  uint32_t lo = 0, hi = 0;
  for (int i = 0; i < call.L; i++) {
    bool u = false;
    const uint32_t code = (uint32_t)plain_code(ref, gbase + (uint64_t)(p + i), &u);
    lo |= (code & 1u) << i; hi |= (code >> 1) << i;
  }
  return copies_key(lo, hi, call.L, call.K, minus, call.site.pam5);
}

// counts[key's index] += by for every record whose key is a query's
void add_sites(const PackedRef& ref, const CopiesCall& call, const std::vector<calitas_site_t>& sites, uint64_t by, std::vector<uint64_t>& counts) {
  for (const calitas_site_t& s : sites) {
    const auto at = call.index.find(key_at(ref, ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, call, s.strand == '-'));
    if (at != call.index.end()) counts[at->second] += by;
  }
}

}  // namespace

int calitas_count_copies_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start,
                                   uint64_t end, const char* queries, uint64_t n_queries, uint64_t* copies) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  CopiesCall call;
  if (int rc = plan_copies(c, pattern, key_length, chrom_index, start, end, queries, n_queries, call)) return rc;
  std::vector<uint64_t> counts(call.keys.size(), 0);
  std::vector<calitas_site_t> found;
  for (int i = call.site.c_first; i <= call.site.c_last && !call.keys.empty(); i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, call.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    add_sites(ctx->ref, call, found, 1, counts);
  }
  for (uint64_t q = 0; q < n_queries; q++) copies[q] = counts[call.of_query[(size_t)q]];
  return CALITAS_OK;
}

int calitas_count_copies_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t chrom_index, uint64_t start, uint64_t end,
                              const char* queries, uint64_t n_queries, uint64_t* copies) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_count_copies needs a GPU (there is no CPU fallback; calitas_count_copies_host is the host twin)");
  CopiesCall call;
  if (int rc = plan_copies(ctx, pattern, key_length, chrom_index, start, end, queries, n_queries, call)) return rc;
  const PackedRef& ref = ctx->ref;
  const size_t n_keys = call.keys.size();
  if (n_keys == 0 || ref.contigs.empty()) {         // nothing to look up, or nothing to scan
    for (uint64_t q = 0; q < n_queries; q++) copies[q] = 0;
    return CALITAS_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.site, chrom_index, start, end, w, a)) return rc;

  // the table: a power of two of slots, at most half of them taken; linear probing from the multiplicative hash's slot.  The key that
  // looks like a free slot (COPIES_EMPTY: T x 32, possible at K = 32 only) stays outside, the kernel knows its index.
  uint32_t log2_slots = 4;
  static_assert(COPIES_MIN_SLOTS == 16, "log2_slots starts at the minimum");
  while (((size_t)1 << log2_slots) < 2 * n_keys) log2_slots++;
  const size_t slots = (size_t)1 << log2_slots;
  std::vector<uint64_t> table(slots, COPIES_EMPTY);
  std::vector<uint32_t> table_index(slots, COPIES_NONE);
  a.ones_index = COPIES_NONE;
  for (size_t k = 0; k < n_keys; k++) {
    const uint64_t key = call.keys[k];
    if (key == COPIES_EMPTY) { a.ones_index = (uint32_t)k; continue; }
    size_t slot = (size_t)((key * COPIES_HASH) >> (64 - log2_slots));
    while (table[slot] != COPIES_EMPTY) slot = (slot + 1) & (slots - 1);
    table[slot] = key; table_index[slot] = (uint32_t)k;
  }
  HIP_TRY(ctx, w->d_keys.grow(slots));
  HIP_TRY(ctx, w->d_key_index.grow(slots));
  HIP_TRY(ctx, w->d_key_counts.grow(n_keys + 1));
  a.keys = w->d_keys.p; a.key_index = w->d_key_index.p; a.key_counts = w->d_key_counts.p;
  a.table_mask = (uint32_t)(slots - 1); a.table_shift = 64 - log2_slots; a.n_keys = (uint32_t)n_keys;
  a.key_len = call.K; a.key_first = call.site.pam5 ? 1 : 0;

  std::vector<uint64_t> counts(n_keys + 1, 0);
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat.p, &call.site.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_keys.p, table.data(), slots * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_key_index.p, table_index.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_key_counts.p, 0, (n_keys + 1) * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, launch_sites_copies(a, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts.data(), w->d_key_counts.p, (n_keys + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (counts[n_keys] != 0) return calitas_fail(ctx, CALITAS_EHIP, "calitas_count_copies: a probe of the key table found neither its key nor a free slot (internal error)");

  // a U is a T to a site and an exception base to the kernel: the sites it did not see in, the records it saw in their place out
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.site, start, end, with_u, kernel_has);
  add_sites(ref, call, with_u, 1, counts);
  add_sites(ref, call, kernel_has, ~0ull, counts);          // (- 1)
  for (uint64_t q = 0; q < n_queries; q++) copies[q] = counts[call.of_query[(size_t)q]];
  return CALITAS_OK;
}

// ---- calitas_count_near: how often a guide's protospacer, or its seed, stands next to a PAM with up to M substitutions ----

namespace {

struct NearCall {
  CopiesCall copies;                                 // the pattern, the region, K and the distinct query keys (plan_copies)
  int M = 0;
};

// checked in this order: max_mismatches, what calitas_count_copies checks, K >= M + 1
int plan_near(calitas_ctx* c, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index, uint64_t start, uint64_t end,
              const char* queries, uint64_t n_queries, NearCall& call) {
  static_assert(NEAR_MAX_M == CALITAS_NEAR_MAX_MISMATCHES, "the kernel unrolls what the contract allows");
  if (max_mismatches < 0 || max_mismatches > NEAR_MAX_M)
    return calitas_fail(c, CALITAS_EINVAL, "max_mismatches is " + std::to_string(max_mismatches) + ": it is 0 .. " + std::to_string(NEAR_MAX_M));
  call.M = max_mismatches;
  if (int rc = plan_copies(c, pattern, key_length, chrom_index, start, end, queries, n_queries, call.copies)) return rc;
  if (call.copies.K < call.M + 1)
    return calitas_fail(c, CALITAS_EINVAL, "key_length: a key of " + std::to_string(call.copies.K) + " bases is shorter than max_mismatches + 1 (" + std::to_string(call.M + 1) + ")");
  return CALITAS_OK;
}

// the number of positions at which two keys differ: a position differs where either plane does
inline int key_distance(uint64_t a, uint64_t b) {
  const uint64_t x = a ^ b;
  return __builtin_popcount((uint32_t)x | (uint32_t)(x >> 32));
}

// counts[index (M + 1) + d] += by for every record and every distinct query at distance d <= M of the record's key, query by query
void add_near_sites(const PackedRef& ref, const NearCall& call, const std::vector<calitas_site_t>& sites, uint64_t by, std::vector<uint64_t>& counts) {
  const size_t row = (size_t)call.M + 1;
  for (const calitas_site_t& s : sites) {
    const uint64_t key = key_at(ref, ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, call.copies, s.strand == '-');
    for (size_t k = 0; k < call.copies.keys.size(); k++) {
      const int d = key_distance(key, call.copies.keys[k]);
      if (d <= call.M) counts[k * row + (size_t)d] += by;
    }
  }
}

void near_rows(const NearCall& call, const std::vector<uint64_t>& counts, uint64_t n_queries, uint64_t* near) {
  const size_t row = (size_t)call.M + 1;
  for (uint64_t q = 0; q < n_queries; q++)
    for (size_t d = 0; d < row; d++) near[q * row + d] = counts[(size_t)call.copies.of_query[(size_t)q] * row + d];
}

}  // namespace

int calitas_count_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index,
                                 uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  NearCall call;
  if (int rc = plan_near(c, pattern, key_length, max_mismatches, chrom_index, start, end, queries, n_queries, call)) return rc;
  std::vector<uint64_t> counts(call.copies.keys.size() * ((size_t)call.M + 1), 0);
  std::vector<calitas_site_t> found;
  for (int i = call.copies.site.c_first; i <= call.copies.site.c_last && !call.copies.keys.empty(); i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, call.copies.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    add_near_sites(ctx->ref, call, found, 1, counts);
  }
  near_rows(call, counts, n_queries, near);
  return CALITAS_OK;
}

namespace {

// The near kernel's launch for a planned call: the pieces' bucket tables, the members, the counters zeroed, one pass, one copy-back.
// model == nullptr: calitas_count_near, counts of n_keys rows of M + 1 words.  Otherwise NEAR_MODEL_WORDS words, the packed table of
// calitas_score_near: it rides behind the offsets, and the rows have M + 3 words (the counts, the sum, the maximum).
// again != nullptr (calitas_list_near, with a model): the table rides along, the counts alone are taken (rows of M + 1 words), and
// *again receives the launch's arguments -- tables, members and patterns stay on the device for the pass's second run.
int run_near(calitas_ctx* ctx, const NearCall& call, int32_t chrom_index, uint64_t start, uint64_t end, const uint32_t* model, std::vector<uint64_t>& counts,
             SitesArgs* again = nullptr) {
  const std::vector<uint64_t>& keys = call.copies.keys;
  const size_t n_keys = keys.size(), row = (size_t)call.M + 1, n_counters = n_keys * (row + (model && !again ? 2 : 0));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->sites) ctx->sites = new SitesWork();
  SitesWork* w = ctx->sites;
  SitesArgs a{};
  if (int rc = site_launch(ctx, call.copies.site, chrom_index, start, end, w, a)) return rc;

  // per piece a bucket table in CSR form -- the offsets of piece p count from p n_keys on, so they address the one member array --
  // and every key as a member of its bucket: a counting sort by bucket
  const int pw = near_piece_width(call.copies.K, call.M);
  const size_t per_table = ((size_t)1 << (2 * pw)) + 1, n_offsets = row * per_table, n_members = row * n_keys;
  std::vector<uint32_t> offsets(n_offsets + (model ? NEAR_MODEL_WORDS : 0), 0);
  std::vector<uint4> members(n_members);
  for (size_t p = 0; p < row; p++) {
    uint32_t* o = offsets.data() + p * per_table;
    for (size_t k = 0; k < n_keys; k++) o[near_bucket((uint32_t)keys[k], (uint32_t)(keys[k] >> 32), (int)p, pw) + 1]++;
    o[0] = (uint32_t)(p * n_keys);
    for (size_t b = 1; b < per_table; b++) o[b] += o[b - 1];
    std::vector<uint32_t> at(o, o + per_table - 1);
    for (size_t k = 0; k < n_keys; k++)
      members[at[near_bucket((uint32_t)keys[k], (uint32_t)(keys[k] >> 32), (int)p, pw)]++] = make_uint4((uint32_t)keys[k], (uint32_t)(keys[k] >> 32), (uint32_t)k, 0u);
  }
  if (model) {
    if (near_model_offset(call.M, pw) != n_offsets) return calitas_fail(ctx, CALITAS_EHIP, "the score table does not stand where the kernel reads it (internal error)");
    std::memcpy(offsets.data() + n_offsets, model, NEAR_MODEL_WORDS * sizeof(uint32_t));
  }
  HIP_TRY(ctx, w->d_near_offsets.grow(offsets.size()));
  if (int rc = no_room_unless(ctx, w->d_near_members.grow(n_members), "the query keys do not fit the device: count the queries in pieces")) return rc;
  HIP_TRY(ctx, w->d_key_counts.grow(n_counters));
  a.near_offsets = w->d_near_offsets.p; a.near_members = w->d_near_members.p; a.key_counts = w->d_key_counts.p;
  a.near_m = call.M; a.near_w = pw; a.n_keys = (uint32_t)n_keys;
  a.key_len = call.copies.K; a.key_first = call.copies.site.pam5 ? 1 : 0;

  counts.assign(n_counters, 0);
  HIP_TRY(ctx, hipMemcpyAsync(w->d_pat.p, &call.copies.site.tab, sizeof(SitePatterns), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_near_offsets.p, offsets.data(), offsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(w->d_near_members.p, members.data(), n_members * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(w->d_key_counts.p, 0, n_counters * sizeof(unsigned long long), ctx->stream));
  HIP_TRY(ctx, model && !again ? launch_sites_near_score(a, ctx->stream) : launch_sites_near(a, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts.data(), w->d_key_counts.p, n_counters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (again) *again = a;
  return CALITAS_OK;
}

}  // namespace

int calitas_count_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t key_length, int32_t max_mismatches, int32_t chrom_index, uint64_t start,
                            uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_count_near needs a GPU (there is no CPU fallback; calitas_count_near_host is the host twin)");
  NearCall call;
  if (int rc = plan_near(ctx, pattern, key_length, max_mismatches, chrom_index, start, end, queries, n_queries, call)) return rc;
  const PackedRef& ref = ctx->ref;
  const size_t row = (size_t)call.M + 1;
  if (call.copies.keys.empty() || ref.contigs.empty()) {         // nothing to look up, or nothing to scan
    for (uint64_t i = 0; i < n_queries * row; i++) near[i] = 0;
    return CALITAS_OK;
  }
  std::vector<uint64_t> counts;
  if (int rc = run_near(ctx, call, chrom_index, start, end, nullptr, counts)) return rc;

  // a U is a T to a site and an exception base to the kernel: the sites it did not see in, the records it saw in their place out
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.copies.site, start, end, with_u, kernel_has);
  add_near_sites(ref, call, with_u, 1, counts);
  add_near_sites(ref, call, kernel_has, ~0ull, counts);     // (- 1)
  near_rows(call, counts, n_queries, near);
  return CALITAS_OK;
}

// ---- calitas_score_near: the near copies of the whole protospacer, and what they add up to under a score model ----

namespace {

struct NearScoreCall {
  NearCall near;                                     // K = L
  const uint32_t* mismatch = nullptr;                // the caller's [L][5][5]
};

// the model as calitas_search_scores checks it -- of which the near calls read the mismatch table alone
int check_near_model(calitas_ctx* c, const calitas_score_model_t* model, NearScoreCall& call) {
  const int L = call.near.copies.L;
  if (!model || !model->mismatch) return calitas_fail(c, CALITAS_EINVAL, "the score model has no mismatch table");
  if (model->protospacer_length != L)
    return calitas_fail(c, CALITAS_EINVAL, "the score model is for protospacers of " + std::to_string(model->protospacer_length) + " bases, the guide has " + std::to_string(L));
  for (int i = 0; i < L * 25; i++)
    if (model->mismatch[i] > 65536u) return calitas_fail(c, CALITAS_EINVAL, "a factor of the score model is above 65536 (1.0)");
  call.mismatch = model->mismatch;
  return CALITAS_OK;
}

// checked in this order: what calitas_count_near checks (the key is the whole protospacer), then the model
int plan_near_score(calitas_ctx* c, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                    uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, NearScoreCall& call) {
  if (int rc = plan_near(c, pattern, 0, max_mismatches, chrom_index, start, end, queries, n_queries, call.near)) return rc;
  return check_near_model(c, model, call);
}

// The contract's loop on two keys of L positions, letter by letter from the planes: the factors of the differing positions in
// ascending order, each read from the caller's table as it stands (never from the kernel's packed one).
uint64_t near_pair_score(const uint32_t* mismatch, int L, uint64_t query, uint64_t site) {
  uint64_t s = 1ull << 32;
  for (int i = 0; i < L; i++) {
    const uint32_t g = (uint32_t)((query >> i) & 1u) | ((uint32_t)((query >> (32 + i)) & 1u) << 1);
    const uint32_t t = (uint32_t)((site >> i) & 1u) | ((uint32_t)((site >> (32 + i)) & 1u) << 1);
    if (g != t) s = (s * mismatch[(size_t)i * 25 + g * 5 + t]) >> 16;
  }
  return s;
}

// rows[k]: M + 1 counts, the sum, the maximum.  Every record against every distinct query: the count by `by` (1 or - 1), and at
// d >= 1 the pair's score into the sum by the same sign; into the maximum only when the record comes in.
void add_near_scores(const PackedRef& ref, const NearScoreCall& call, const std::vector<calitas_site_t>& sites, bool in, std::vector<uint64_t>& rows) {
  const NearCall& nc = call.near;
  const size_t M = (size_t)nc.M, row = M + 3;
  for (const calitas_site_t& s : sites) {
    const uint64_t key = key_at(ref, ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, nc.copies, s.strand == '-');
    for (size_t k = 0; k < nc.copies.keys.size(); k++) {
      const int d = key_distance(key, nc.copies.keys[k]);
      if (d > nc.M) continue;
      uint64_t* r = &rows[k * row];
      r[d] += in ? 1 : ~0ull;
      if (d == 0) continue;
      const uint64_t sc = near_pair_score(call.mismatch, nc.copies.L, nc.copies.keys[k], key);
      if (in) { r[M + 1] += sc; r[M + 2] = std::max(r[M + 2], sc); }
      else r[M + 1] -= sc;
    }
  }
}

void near_score_rows(const NearScoreCall& call, const std::vector<uint64_t>& rows, uint64_t n_queries, uint64_t* near, calitas_near_score_t* scores) {
  const size_t M = (size_t)call.near.M, row = M + 3;
  for (uint64_t q = 0; q < n_queries; q++) {
    const uint64_t* r = rows.empty() ? nullptr : &rows[(size_t)call.near.copies.of_query[(size_t)q] * row];
    for (size_t d = 0; d <= M; d++) near[q * (M + 1) + d] = r ? r[d] : 0;
    scores[q].sum_q32 = r ? r[M + 1] : 0;
    scores[q].max_q32 = r ? r[M + 2] : 0;
  }
}

}  // namespace

int calitas_score_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                                 int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near,
                                 calitas_near_score_t* scores) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  NearScoreCall call;
  if (int rc = plan_near_score(c, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, call)) return rc;
  const CopiesCall& cc = call.near.copies;
  std::vector<uint64_t> rows(cc.keys.size() * ((size_t)call.near.M + 3), 0);
  std::vector<calitas_site_t> found;
  for (int i = cc.site.c_first; i <= cc.site.c_last && !cc.keys.empty(); i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, cc.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    add_near_scores(ctx->ref, call, found, true, rows);
  }
  near_score_rows(call, rows, n_queries, near, scores);
  return CALITAS_OK;
}

int calitas_score_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                            uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint64_t* near, calitas_near_score_t* scores) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_score_near needs a GPU (there is no CPU fallback; calitas_score_near_host is the host twin)");
  NearScoreCall call;
  if (int rc = plan_near_score(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, call)) return rc;
  const PackedRef& ref = ctx->ref;
  std::vector<uint64_t> rows;
  if (call.near.copies.keys.empty() || ref.contigs.empty()) {    // nothing to look up, or nothing to scan
    near_score_rows(call, rows, n_queries, near, scores);
    return CALITAS_OK;
  }
  // the 4 x 4 block of plain bases of every position, as the kernel indexes it
  std::vector<uint32_t> packed(NEAR_MODEL_WORDS, 0u);
  for (uint32_t i = 0; i < (uint32_t)call.near.copies.L; i++)
    for (uint32_t g = 0; g < 4; g++)
      for (uint32_t t = 0; t < 4; t++) packed[near_model_index(i, g, t)] = call.mismatch[(size_t)i * 25 + g * 5 + t];
  if (int rc = run_near(ctx, call.near, chrom_index, start, end, packed.data(), rows)) return rc;

  // a U is a T to a site and an exception base to the kernel: the sites it did not see in, the records it saw in their place out.
  // Counts and sums are corrected both ways.  A maximum cannot be taken back, and need not be: host_sites pushes a kernel_has record
  // only at the (contig, strand, protospacer start) of the with_u record it has just pushed, so the two have one key and the same
  // scores -- what the kernel's record put into a maximum, the true site puts there as well.  That pairing is checked here.
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, call.near.copies.site, start, end, with_u, kernel_has);
  size_t at = 0;
  for (const calitas_site_t& s : kernel_has) {                   // (both lists are in output order)
    while (at < with_u.size() && site_less(with_u[at], s)) at++;
    if (at == with_u.size() || site_less(s, with_u[at]))
      return calitas_fail(ctx, CALITAS_EHIP, "calitas_score_near: a record the kernel has beside a U stands where no site with a U does (internal error)");
  }
  add_near_scores(ref, call, with_u, true, rows);
  add_near_scores(ref, call, kernel_has, false, rows);
  near_score_rows(call, rows, n_queries, near, scores);
  return CALITAS_OK;
}

// ---- calitas_list_near: where every query's copies within M substitutions stand ----

namespace {

struct NearListCall {
  NearScoreCall score;                               // K = L; mismatch == nullptr: no weights, every score is 2^32
  uint32_t limit = 0;
};

// checked in this order: what calitas_score_near checks, a NULL model being legal; then the limit
int plan_near_list(calitas_ctx* c, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                   uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, NearListCall& call) {
  if (int rc = plan_near(c, pattern, 0, max_mismatches, chrom_index, start, end, queries, n_queries, call.score.near)) return rc;
  if (model)
    if (int rc = check_near_model(c, model, call.score)) return rc;
  if (limit < 1 || limit > CALITAS_NEAR_LIST_MAX)
    return calitas_fail(c, CALITAS_EINVAL, "limit is " + std::to_string(limit) + ": it is 1 .. " + std::to_string(CALITAS_NEAR_LIST_MAX));
  call.limit = limit;
  return CALITAS_OK;
}

bool hit_less(const calitas_near_hit_t& a, const calitas_near_hit_t& b) {
  if (a.contig_index != b.contig_index) return a.contig_index < b.contig_index;
  if (a.protospacer_start != b.protospacer_start) return a.protospacer_start < b.protospacer_start;
  return a.strand == '+' && b.strand == '-';
}

// the record of a site whose key is within M of a query's, from the host's side: the twin's, and the ones a U keeps from the kernel
calitas_near_hit_t near_hit(const NearListCall& call, const calitas_site_t& s, uint64_t site_key, uint64_t query_key) {
  const uint64_t x = site_key ^ query_key;
  calitas_near_hit_t h;
  std::memset(&h, 0, sizeof(h));
  h.score_q32 = call.score.mismatch ? near_pair_score(call.score.mismatch, call.score.near.copies.L, query_key, site_key) : 1ull << 32;
  h.contig_index = s.contig_index; h.protospacer_start = s.protospacer_start;
  h.target_lo = (uint32_t)site_key; h.target_hi = (uint32_t)(site_key >> 32);
  h.diff_mask = (uint32_t)x | (uint32_t)(x >> 32);
  h.strand = s.strand; h.pam_index = s.pam_index; h.mismatches = (uint8_t)__builtin_popcount(h.diff_mask);
  return h;
}

typedef std::pair<const calitas_near_hit_t*, size_t> HitSpan;

// What the call hands over, from the distinct keys' counts and ordered stretches: near, the stretches laid out in query order -- a
// key over the limit lists nothing, a duplicate gets its key's stretch again -- and the one block of records.
int near_list_block(calitas_ctx* c, const NearListCall& call, const std::vector<uint64_t>& counts, const std::vector<HitSpan>& spans, uint64_t n_queries,
                    uint64_t* near, uint64_t* offsets, calitas_near_hit_t** hits, uint64_t* n_hits) {
  const NearCall& nc = call.score.near;
  const size_t row = (size_t)nc.M + 1;
  if (n_queries) near_rows(nc, counts, n_queries, near);
  uint64_t run = 0;
  for (uint64_t q = 0; q < n_queries; q++) {
    const size_t k = nc.copies.of_query[(size_t)q];
    uint64_t sum = 0;
    for (size_t d = 0; d < row; d++) sum += counts[k * row + d];
    offsets[q] = run;
    if (sum > call.limit) continue;
    if (spans[k].second != sum) return calitas_fail(c, CALITAS_EHIP, "calitas_list_near: a query's records are not as many as its counts (internal error)");
    run += sum;
  }
  offsets[n_queries] = run;
  calitas_near_hit_t* block = (calitas_near_hit_t*)calitas_out_alloc(std::max<uint64_t>(1, run) * sizeof(calitas_near_hit_t));
  if (!block) return calitas_fail(c, CALITAS_ENOMEM, "the records do not fit the host's memory: list the queries in pieces");
  for (uint64_t q = 0; q < n_queries; q++) {
    const uint64_t n = offsets[q + 1] - offsets[q];
    if (n) std::memcpy(block + offsets[q], spans[nc.copies.of_query[(size_t)q]].first, n * sizeof(calitas_near_hit_t));
  }
  *hits = block; *n_hits = run;
  return CALITAS_OK;
}

}  // namespace

int calitas_list_near_host_impl(const calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model,
                                int32_t chrom_index, uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near,
                                uint64_t* offsets, calitas_near_hit_t** hits, uint64_t* n_hits) {
  calitas_ctx* c = const_cast<calitas_ctx*>(ctx);
  NearListCall call;
  if (int rc = plan_near_list(c, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, limit, call)) return rc;
  const NearCall& nc = call.score.near;
  const CopiesCall& cc = nc.copies;
  const size_t n_keys = cc.keys.size(), row = (size_t)nc.M + 1;
  std::vector<uint64_t> counts(n_keys * row, 0);
  std::vector<std::vector<calitas_near_hit_t>> lists(n_keys);
  std::vector<calitas_site_t> found;
  for (int i = cc.site.c_first; i <= cc.site.c_last && n_keys; i++) {
    const uint64_t len = ctx->ref.contigs[(size_t)i].len;
    found.clear();
    host_sites(ctx->ref, cc.site.tab.pat, nullptr, i, 0, (int64_t)len, (int64_t)std::min(start, len), (int64_t)region_end(len, end), found, nullptr);
    for (const calitas_site_t& s : found) {
      const uint64_t key = key_at(ctx->ref, ctx->ref.contigs[(size_t)s.contig_index].gbase, s.protospacer_start, cc, s.strand == '-');
      for (size_t k = 0; k < n_keys; k++) {
        const int d = key_distance(key, cc.keys[k]);
        if (d > nc.M) continue;
        counts[k * row + (size_t)d]++;
        if (lists[k].size() <= call.limit) lists[k].push_back(near_hit(call, s, key, cc.keys[k]));   // (one beyond the limit: such a key lists nothing)
      }
    }
  }
  std::vector<HitSpan> spans(n_keys);
  for (size_t k = 0; k < n_keys; k++) {
    std::sort(lists[k].begin(), lists[k].end(), hit_less);
    spans[k] = HitSpan(lists[k].data(), lists[k].size());
  }
  return near_list_block(c, call, counts, spans, n_queries, near, offsets, hits, n_hits);
}

int calitas_list_near_impl(calitas_ctx* ctx, const calitas_guide_t* pattern, int32_t max_mismatches, const calitas_score_model_t* model, int32_t chrom_index,
                           uint64_t start, uint64_t end, const char* queries, uint64_t n_queries, uint32_t limit, uint64_t* near, uint64_t* offsets,
                           calitas_near_hit_t** hits, uint64_t* n_hits) {
  if (ctx->device < 0) return calitas_fail(ctx, CALITAS_ENODEV, "host-only context: calitas_list_near needs a GPU (there is no CPU fallback; calitas_list_near_host is the host twin)");
  static_assert(sizeof(NearHit) == sizeof(calitas_near_hit_t) && offsetof(NearHit, score_q32) == offsetof(calitas_near_hit_t, score_q32) &&
                offsetof(NearHit, contig) == offsetof(calitas_near_hit_t, contig_index) && offsetof(NearHit, proto_start) == offsetof(calitas_near_hit_t, protospacer_start) &&
                offsetof(NearHit, target_lo) == offsetof(calitas_near_hit_t, target_lo) && offsetof(NearHit, target_hi) == offsetof(calitas_near_hit_t, target_hi) &&
                offsetof(NearHit, diff_mask) == offsetof(calitas_near_hit_t, diff_mask) && offsetof(NearHit, strand) == offsetof(calitas_near_hit_t, strand) &&
                offsetof(NearHit, pam_index) == offsetof(calitas_near_hit_t, pam_index) && offsetof(NearHit, mismatches) == offsetof(calitas_near_hit_t, mismatches),
                "the kernel writes calitas_near_hit_t");
  NearListCall call;
  if (int rc = plan_near_list(ctx, pattern, max_mismatches, model, chrom_index, start, end, queries, n_queries, limit, call)) return rc;
  const NearCall& nc = call.score.near;
  const std::vector<uint64_t>& keys = nc.copies.keys;
  const PackedRef& ref = ctx->ref;
  const size_t n_keys = keys.size(), row = (size_t)nc.M + 1;
  std::vector<uint64_t> counts(n_keys * row, 0);
  std::vector<HitSpan> spans(n_keys, HitSpan(nullptr, 0));
  if (n_keys == 0 || ref.contigs.empty())            // nothing to look up, or nothing to scan
    return near_list_block(ctx, call, counts, spans, n_queries, near, offsets, hits, n_hits);

  // pass 1: the counts.  The model's 4 x 4 blocks as the kernel indexes them ride along for pass 2; without a model every factor is 1.0
  std::vector<uint32_t> packed(NEAR_MODEL_WORDS, call.score.mismatch ? 0u : 65536u);
  for (uint32_t i = 0; call.score.mismatch && i < (uint32_t)nc.copies.L; i++)
    for (uint32_t g = 0; g < 4; g++)
      for (uint32_t t = 0; t < 4; t++) packed[near_model_index(i, g, t)] = call.score.mismatch[(size_t)i * 25 + g * 5 + t];
  SitesArgs a{};
  if (int rc = run_near(ctx, nc, chrom_index, start, end, packed.data(), counts, &a)) return rc;

  // The layout.  A U is a T to a site and an exception base to the kernel, so the counts are corrected as calitas_count_near's are,
  // and the corrected counts decide whether a key lists.  A key that does gets room for what the KERNEL will store, its own count;
  // where the two differ the host patches the stretch below.
  std::vector<uint64_t> kernel_sum(n_keys, 0);
  for (size_t k = 0; k < n_keys; k++)
    for (size_t d = 0; d < row; d++) kernel_sum[k] += counts[k * row + d];
  std::vector<calitas_site_t> with_u, kernel_has;
  sites_with_u(ctx, nc.copies.site, start, end, with_u, kernel_has);
  add_near_sites(ref, nc, with_u, 1, counts);
  add_near_sites(ref, nc, kernel_has, ~0ull, counts);       // (- 1)
  std::vector<uint64_t> base(n_keys, 0);
  std::vector<uint32_t> cursors(2 * n_keys + 1, 0), order, longer;
  uint64_t total = 0;
  for (size_t k = 0; k < n_keys; k++) {
    uint64_t sum = 0;
    for (size_t d = 0; d < row; d++) sum += counts[k * row + d];
    base[k] = total;
    cursors[2 * k + 1] = NEAR_LIST_SKIP;
    if (sum > call.limit) continue;
    if (kernel_sum[k] >= NEAR_LIST_SKIP) return calitas_fail(ctx, CALITAS_ENOMEM, "the records do not fit the device: list the queries in pieces");
    cursors[2 * k + 1] = (uint32_t)kernel_sum[k];
    total += kernel_sum[k];
    if (kernel_sum[k] > NEAR_ORDER_SHORT) longer.push_back((uint32_t)k);
    else if (kernel_sum[k]) order.push_back((uint32_t)k);
  }
  const uint32_t n_short = (uint32_t)order.size(), n_long = (uint32_t)longer.size();
  order.insert(order.end(), longer.begin(), longer.end());

  // pass 2, the order, one copy-back
  std::vector<calitas_near_hit_t> dev;
  if (total) {
    SitesWork* w = ctx->sites;
    try { dev.resize((size_t)total); } catch (const std::bad_alloc&) { return calitas_fail(ctx, CALITAS_ENOMEM, "the records do not fit the host's memory: list the queries in pieces"); }
    HIP_TRY(ctx, w->d_list_base.grow(n_keys));
    HIP_TRY(ctx, w->d_list_cursors.grow(2 * n_keys + 1));
    HIP_TRY(ctx, w->d_list_order.grow(n_keys));
    const char* const no_room = "the records do not fit the device: list the queries in pieces";
    if (int rc = no_room_unless(ctx, w->d_list_in.grow(total), no_room)) return rc;
    if (int rc = no_room_unless(ctx, w->d_list_out.grow(total), no_room)) return rc;
    a.wg_offset = w->d_list_base.p; a.wg_count = w->d_list_cursors.p; a.out = reinterpret_cast<SiteRecord*>(w->d_list_in.p); a.out_capacity = total;
    uint32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(w->d_list_base.p, base.data(), n_keys * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w->d_list_cursors.p, cursors.data(), (2 * n_keys + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(w->d_list_order.p, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_sites_near_list(a, ctx->stream));
    HIP_TRY(ctx, launch_near_order(w->d_list_in.p, w->d_list_out.p, w->d_list_base.p, w->d_list_cursors.p, w->d_list_order.p, n_short, n_long, (uint32_t)(2 * n_keys), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&flag, w->d_list_cursors.p + 2 * n_keys, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dev.data(), w->d_list_out.p, total * sizeof(NearHit), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag != 0) return calitas_fail(ctx, CALITAS_EHIP, "calitas_list_near: the second pass found other pairs than the first counted (internal error)");
  }
  for (size_t k = 0; k < n_keys; k++)
    if (cursors[2 * k + 1] != NEAR_LIST_SKIP) spans[k] = HitSpan(dev.data() + base[k], cursors[2 * k + 1]);

  // Beside a U: the stretches of the keys within M of such a site lose the records the kernel has in its place, gain the site's own
  // and are put in order again -- also the few a U made longer than the order kernel takes.
  std::vector<std::vector<calitas_near_hit_t>> fixed;
  if (!with_u.empty() || !kernel_has.empty()) {
    std::vector<uint64_t> key_in(with_u.size()), key_out(kernel_has.size());
    for (size_t i = 0; i < with_u.size(); i++) key_in[i] = key_at(ref, ref.contigs[(size_t)with_u[i].contig_index].gbase, with_u[i].protospacer_start, nc.copies, with_u[i].strand == '-');
    for (size_t i = 0; i < kernel_has.size(); i++) key_out[i] = key_at(ref, ref.contigs[(size_t)kernel_has[i].contig_index].gbase, kernel_has[i].protospacer_start, nc.copies, kernel_has[i].strand == '-');
    fixed.reserve(n_keys);                                  // (the spans point into its elements)
    for (size_t k = 0; k < n_keys; k++) {
      if (cursors[2 * k + 1] == NEAR_LIST_SKIP) continue;
      bool touched = false;
      for (size_t i = 0; i < key_in.size() && !touched; i++) touched = key_distance(key_in[i], keys[k]) <= nc.M;
      for (size_t i = 0; i < key_out.size() && !touched; i++) touched = key_distance(key_out[i], keys[k]) <= nc.M;
      if (!touched) continue;
      fixed.emplace_back(spans[k].first, spans[k].first + spans[k].second);
      std::vector<calitas_near_hit_t>& v = fixed.back();
      for (size_t i = 0; i < key_out.size(); i++) {
        if (key_distance(key_out[i], keys[k]) > nc.M) continue;
        const calitas_site_t& s = kernel_has[i];
        const auto at = std::find_if(v.begin(), v.end(), [&](const calitas_near_hit_t& h) {
          return h.contig_index == s.contig_index && h.protospacer_start == s.protospacer_start && h.strand == s.strand; });
        if (at == v.end()) return calitas_fail(ctx, CALITAS_EHIP, "calitas_list_near: a record the kernel should have written beside a U is not there (internal error)");
        v.erase(at);
      }
      for (size_t i = 0; i < key_in.size(); i++)
        if (key_distance(key_in[i], keys[k]) <= nc.M) v.push_back(near_hit(call, with_u[i], key_in[i], keys[k]));
      std::sort(v.begin(), v.end(), hit_less);
      spans[k] = HitSpan(v.data(), v.size());
    }
  }
  return near_list_block(ctx, call, counts, spans, n_queries, near, offsets, hits, n_hits);
}
