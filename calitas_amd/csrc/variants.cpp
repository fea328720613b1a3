// variants.cpp -- the variant branch of SearchReference.execute (SearchReference.scala:101-400, 570-630) behind one C entry point.
//
// calitas_search_variants = the reference hits of calitas_search + the hits of every variant window, merged by removeOverlaps /
// ReferenceHit.sort (calitas_hits_tsv_ext).  Variant windows are produced on the host exactly as variantWindowIterator does
// (nextChunk / reChunk SR:326-347, alleleCombos SR:351-399, buildVariantWindow SR:263-323: variants_window.cpp), aligned on the GPU
// through the calitas_align_windows path in batches, lifted back with refOffsetAtBaseOffset (SR:133-156) and turned into rows with
// window-local flanks (SR:598-613) and the variant columns (RH:211-233: variants_rows.cpp).  tests/variants_twin.py holds the same
// logic in Python (the parity tests run both); this code exists because BASELINE config 5 has three million variants.
// This unit holds the call itself -- search_variants_impl, which takes the steps of a VariantSearch (variants_internal.hpp) in order --
// and the stages between the walk and the text; none of it has a counterpart in the reference.
//
// THE THREADS OF ONE CALL (round 5), and what each of them owns.  A stage is a thread that runs jobs in the order they are handed
// over (StageThread: two jobs waiting at most, a failed stage drops what is behind it but still pays its turns); all of them share the
// context's worker pool for the parallel part of a job.
//   caller       walks the VCF's records as they are published (VarTable::have), lists what every window is made of (Spec), hands a
//                full list to the builder and, at a contig's end, the contig's "finish" behind its last batch
//   vcf reader   maps the file, parses it in waves of 16 MB on the pool, publishes the records wave by wave
//   md5          the VCF's identifier "name:md5" (RH:175-183); whoever needs it first joins it (Identifier::need)
//   builder      build_window for a list (pool), the batch to one of the aligners
//   aligner x2   calitas_align_windows of a batch on a side context each (device); the batches reach the lifter in the order they were built
//   lifter       lifts a batch's alignments back, lists them as hits (HitList: pieces that never move); at a contig's end the groups' own
//                walks, the entries' tie order and keys (finish_contig)
//   finisher     the rows of the contig's placed entries (with a placeholder where the identifier goes), then publishes the contig
//   helper       the reference's per-contig passes (search_hits.cpp, calitas_search_hits_ext_impl): asks for a contig's entries when its row stage
//                is due (HitsExtSource::get, blocks until published), makes the rows of the plain entries the device's walk kept
//                (HitsExt::rows_for), and its copying thread hands every contig's text to ...
//   filler       ... which waits for the identifier once and writes the kept entries' rows into the holes the rows kernel left
//                (HitsExt::fill; on the copying thread itself when the text is in a block of the library's, which may still move)
// cx[c] (ContigExt) is the lifter's until finish_contig(c) returns, the finisher's until it publishes c, then the helper's and the
// filler's; hits[] grows on the lifter only, everybody else reads published contigs through the pointers in cx[c].entry.
#include <sys/resource.h>

#include <algorithm>
#include <array>
#include <unordered_map>

#include "variants_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

static double cpu_seconds() {                                      // (CALITAS_TRACE: how busy the call kept the process's threads)
  rusage u{};
  (void)getrusage(RUSAGE_SELF, &u);
  return (double)u.ru_utime.tv_sec + (double)u.ru_stime.tv_sec + 1e-6 * ((double)u.ru_utime.tv_usec + (double)u.ru_stime.tv_usec);
}

VariantSearch::Identifier::Identifier(const char* vcf_path, const char* vcf_id)
    : vid(vcf_id ? vcf_id : ""), placeholder(vcf_id ? std::string(vcf_id) : vcf_identifier(vcf_path, std::string(32, '0'))) {
  if (!vcf_id)                                                     // ReferenceHit.scala:175-183: file name and md5, needed when the first row is written
    md5_thread = std::thread([this, vcf_path] {
      std::string hex;
      md5_err = md5_file(vcf_path, hex);
      vid = vcf_identifier(vcf_path, hex);
    });
}

VariantSearch::VariantSearch(calitas_ctx* ctx_, const calitas_guide_t* guide_, const char* guide_id, const calitas_params_t* params_, GuideHost&& gh_,
                             const char* vcf_path_, const char* chrom_, const char* vcf_id, std::string version_, std::string stamp_,
                             char* user_dst_, uint64_t user_cap_)
    : ctx(ctx_), guide(guide_), params(params_), vcf_path(vcf_path_), chrom(chrom_), user_dst(user_dst_), user_cap(user_cap_), ref(ctx_->ref),
      p(*params_), ap(*params_), gh(std::move(gh_)), gid(guide_id ? guide_id : ""), version(std::move(version_)), stamp(std::move(stamp_)),
      rs(make_row_strings(ref, gh, gid, p, version, stamp)), row_in{ref, gh, gid, rs, ref.genome_build + "+variants"},
      padding([this] {
        size_t max_pam = 0;
        for (auto& q : gh.pams) max_pam = std::max(max_pam, q.size());
        return (int)gh.protospacer.size() + (int)max_pam - 1 + p.max_guide_diffs + p.max_gaps_between_guide_and_pam;
      }()),
      nc(ref.contigs.size()),
      device_merge([this] { const char* force_host = TUNE_GET("CALITAS_VARIANTS_HOST"); return !(force_host && std::atoi(force_host) != 0) && p.max_overlap >= 1; }()),
      actx(ctx_), trace_stages(TUNE_GET("CALITAS_TRACE") && std::atoi(TUNE_GET("CALITAS_TRACE")) >= 3), cpu0(cpu_seconds()),
      id(vcf_path_, vcf_id), cx(nc) {
  ap.chrom_index = -1;
  for (auto& n : ref.names) if (!chrom || n == chrom) order.push_back(n);
}

// ---- the reference windows (SR:527-561) and the merge (SR:641-648) on the device, beside the variant windows --------------------
// The reference's own hits never leave the device.  A hit of a variant window that touches no variant joins the removeOverlaps
// group of the reference hits of its chromosome and strand (SR:656) -- most of them repeat a reference hit and lose against it there,
// the ones an edge of their window cut short do not -- so every one of them goes into the device's walk of that group (hits.hpp,
// HitsExt), behind the reference hits with the same sort key as SR:622 has them arrive.  The groups of the hits that do touch variants
// hold nothing else: they are walked here, and what they keep is handed to the device for its place in ReferenceHit.sort's order only.
// The device then writes every surviving row, its own and these, into one text per contig.  Ties between rows of different groups
// follow calitas_hits_tsv_ext (the reference leaves them to a hash map): the reference group first, then the variant groups in order
// of first appearance.
// The two halves run side by side: the calling thread and the stages produce, align (on side contexts: a stream and buffers of their
// own) and key the variant windows contig by contig -- host work, mostly -- while the helper thread drives the reference's per-contig
// passes (device work and the text over PCIe); the row stage of contig c waits until the contig's entries are published.
int VariantSearch::set_up() {
  if (device_merge) {
    int rc = calitas_side_context(ctx, &actx);
    if (rc) return rc;
    rc = calitas_side_context(ctx, &actx2, 1);
    if (rc) return rc;
  }
  two_aligners = actx2 != nullptr;
  // Compact rows on the per-contig stream of this call: OFF unless asked for.  Measured at BASELINE config 5's size (round 5): the texts'
  // time on the bus halves (0.40 -> 0.21 s) and the call does not get shorter (1.10-1.14 against 1.12-1.17 s) -- this branch is bound by
  // its host threads (a 16-core quota), and putting guide_id, protospacer and the tail back into 41 million rows is more work for them
  // (window building 0.31-0.39 -> 0.42-0.51 s, the entries' rows 0.37-0.42 -> 0.41-0.51 s).
  source.compact_rows = device_merge && TUNE_ON("CALITAS_VARIANTS_COMPACT");
  fill_on_host = device_merge && !source.compact_rows;             // (variants_rows.cpp: which rows go where)
  source.get = [this](int c, const HitsExt** e) -> int { return get_contig(c, e); };
  return CALITAS_OK;
}

void VariantSearch::publish(size_t upto, bool quit) {
  { std::lock_guard<std::mutex> lk(pub.mu); pub.published = std::max(pub.published, upto); pub.give_up = pub.give_up || quit; }
  pub.cv.notify_all();
  if (trace_stages) std::fprintf(stderr, "[calitas] search_variants: contigs before %zu published at %.1f ms\n", upto, ms_since(t_call));
}

int VariantSearch::get_contig(int c, const HitsExt** e) {
  std::unique_lock<std::mutex> lk(pub.mu);
  pub.cv.wait(lk, [&] { return pub.published > (size_t)c || pub.give_up; });
  if (pub.published <= (size_t)c) return 1;
  *e = cx[(size_t)c].ext.n ? &cx[(size_t)c].ext : nullptr;
  return 0;
}

// Two stage threads at least: batch k is on the device (aligner), the alignments of batch k - 1 are lifted back and listed as hits
// (lifter), while the calling thread walks the VCF and the builder builds batch k + 1 -- 48 batches of 65 536 windows at full size: 8-10
// ms each in the aligner, 3 to lift, 5 to walk and build.  Jobs run in the order they were handed over; two wait per stage at most.
// (Two aligners when the call has side contexts: a batch is 8-10 ms in calitas_align_windows and 5 ms to walk and build, so one
// aligner was the pipeline's slowest stage; the batches alternate between them and reach the lifter in their own order.)
void VariantSearch::start_threads() {
  if (fill_on_host) filler.start(-1);
  if (device_merge)
    helper.t = std::thread([this] {
      const auto t0 = Clock::now();
      (void)hipSetDevice(ctx->device);
      try {
        hr.rc = calitas_search_hits_ext_impl(ctx, guide, gid, params, version.c_str(), stamp.c_str(), source, &hr.tsv, &hr.bytes, &hr.rows, &hr.declined, user_dst, user_cap);
      } catch (const std::exception& e) {                                                           // (a thread of its own has no caller to unwind to)
        hr.rc = calitas_fail(ctx, CALITAS_EHIP, std::string("the reference passes ended with an exception: ") + e.what());
      }
      hr.ms = ms_since(t0);
    });
  aligner.start(ctx->device);
  if (two_aligners) aligner2.start(ctx->device);
  lifter.start(-1);
  finisher.start(-1);
  builder.start(-1);
  // The VCF, beside the first of the reference passes (they need nothing of it before their first row stage: 0.15 s at BASELINE config
  // 5's size that the helper thread used to sit out) -- and beside the walk: a thread of its own parses the file wave by wave,
  // the walk follows it record by record (VarTable::have).
  vcf_reader.t = std::thread([this] {
    const auto t0 = Clock::now();
    try { vcf_err = read_vcf(vcf_path, chrom, ctx->pool, vcf); }
    catch (const std::exception& x) { vcf_err = std::string("reading the VCF ended with an exception: ") + x.what(); }
    tm.parse = ms_since(t0);
    vcf.publish(vcf.size(), true);                                  // (whatever happened: the walk must not wait for more)
  });
}

// ---- builder -> aligner -> lifter -----------------------------------------------------------------------------------------------------

// Batch k's turn at the lifter: every batch takes it exactly once, in the order the batches were built -- whether its job ran, failed,
// threw or was dropped because the stage had failed before (StageThread's `skipped` handler) -- so a job of the other aligner that
// waits for "batches_lifting == k" is never left waiting for a job that will not run.  at_turn (may be empty) runs inside the turn.
int VariantSearch::pass_turn(uint64_t k, const std::function<int()>& at_turn) {
  std::unique_lock<std::mutex> lk(turns.mu);
  turns.cv.wait(lk, [&] { return turns.batches_lifting == k; });
  int r = CALITAS_OK;
  try { if (at_turn) r = at_turn(); }
  catch (...) { turns.batches_lifting = k + 1; lk.unlock(); turns.cv.notify_all(); throw; }
  turns.batches_lifting = k + 1;
  lk.unlock();
  turns.cv.notify_all();
  return r;
}

// A built batch of windows (builder thread) to one of the aligners, and from there to the lifter.
int VariantSearch::hand_over(Batch&& b, size_t n) {
  auto held = std::make_shared<Batch>(std::move(b));
  const uint64_t k = turns.batches_handed++;
  const bool second = two_aligners && (k & 1);
  calitas_ctx* const where = second ? actx2 : actx;
  return (second ? aligner2 : aligner).enqueue([this, held, n, k, where](std::string& e) -> int {
    auto res = std::make_shared<Aligned>();
    int r = CALITAS_OK;
    try { if (n) r = align_part(where, *held, n, *res); }
    catch (const std::exception& x) { r = CALITAS_EHIP; e = std::string("the aligner stage of the variant branch ended with an exception: ") + x.what(); }
    // the lifter takes the batches in the order they were built, whichever aligner is done first
    return pass_turn(k, [&]() -> int {
      if (r || !n) return r;
      return lifter.enqueue([this, held, n, res](std::string& le) { return lift_part(*held, n, *res, le); }, 2, nullptr);
    });
  }, 2, &tm.wait, [this, k] { (void)pass_turn(k, nullptr); });
}

// A contig's entries for the device are made on the lifter thread, behind the lift of the contig's last batch, while the calling thread is
// already walking the next contig (waiting for the stages to run dry at every one of 25 contig ends was 0.22 s of the variant half):
// the "finish" takes a batch's number and its turn, so it reaches the lifter behind every batch handed over before it.
int VariantSearch::hand_over_finish(size_t upto) {
  const uint64_t k = turns.batches_handed++;
  const bool second = two_aligners && (k & 1);
  return (second ? aligner2 : aligner).enqueue([this, k, upto](std::string&) -> int {
    return pass_turn(k, [&]() -> int { return lifter.enqueue([this, upto](std::string&) { return finish_upto(upto); }, 2, nullptr); });
  }, 2, &tm.wait, [this, k] { (void)pass_turn(k, nullptr); });
}

// A built batch of windows through the aligner (device), on an aligner thread.
int VariantSearch::align_part(calitas_ctx* where, Batch& batch, const size_t n, Aligned& res) {
  std::vector<calitas_guide_t> guides(n, *guide);
  std::vector<const uint8_t*> targets(n);
  std::vector<uint32_t> lens(n);
  std::vector<int32_t> offs(n, 0);
  for (size_t i = 0; i < n; i++) { targets[i] = reinterpret_cast<const uint8_t*>(batch.wins[i].bases); lens[i] = (uint32_t)batch.wins[i].len; }
  const auto t0 = Clock::now();
  if (const char* inj = TUNE_GET("CALITAS_FAIL_ALIGN_BATCH"))        // tests: the error path of the stages (a failed batch must fail the call, not hang it)
    if (std::atoi(inj) == batch_serial++) return calitas_fail(ctx, CALITAS_EHIP, "injected failure of an aligner batch (CALITAS_FAIL_ALIGN_BATCH)");
  int r = calitas_align_windows(where, (int32_t)n, guides.data(), targets.data(), lens.data(), offs.data(), &ap, &res.out, &res.n_out, &res.counts);
  if (r) { if (where != ctx) calitas_fail(ctx, r, calitas_last_error(where)); return r; }
  tm.ns_align += (long long)(ms_since(t0) * 1e6);
  if (trace_stages) std::fprintf(stderr, "[calitas] search_variants: a batch (contig %d ..) aligned %.1f .. %.1f ms\n", batch.wins[0].contig, ms_since(t_call) - ms_since(t0), ms_since(t_call));
  return CALITAS_OK;
}

// ... and its alignments lifted back and listed as hits (lifter thread, worker pool); `err_out` is that thread's own.
int VariantSearch::lift_part(Batch& batch, const size_t n, const Aligned& res, std::string& err_out) {
  calitas_aln_t* const out = res.out;
  const auto t1 = Clock::now();
  // the batch's windows and records stay until the rows are written
  lifted.kept_windows.emplace_back(std::move(batch));            // (vectors move: the views keep pointing into the arenas)
  const std::vector<Window>& wins = lifted.kept_windows.back().wins;
  lifted.kept_out.push_back(out);
  std::vector<uint64_t> first(n + 1, 0);
  for (size_t t = 0; t < n; t++) first[t + 1] = first[t] + res.counts[t];
  HitList& hits = lifted.hits;
  const size_t base = hits.size();
  hits.resize(base + (size_t)res.n_out);
  std::vector<std::string> errs((size_t)ctx->pool->size());
  ctx->pool->for_blocks(n, [&](size_t tb, size_t te, int tid) {
    for (size_t t = tb; t < te && errs[(size_t)tid].empty(); t++) {
      const Window& w = wins[t];
      for (uint64_t k = first[t]; k < first[t + 1]; k++) {
        const calitas_aln_t& a = out[k];
        ExtHit& h = hits[base + (size_t)k];
        h.w = &w; h.a = &a;
        int start = 0, end = 0, gend = 0;
        if (!lift(w, a, start, end, h.gstart, gend)) { errs[(size_t)tid] = "Query bases can't be present at operator D."; break; }
        h.tlen = target_length(a);
        // variants under the hit (RH:211): their display strings are the hit's removeOverlaps group (SR:656)
        for_variants_under(w, start, end, [&h](const Allele& al) { if (!h.desc.empty()) h.desc += ';'; h.desc += display_string(al); });
      }
    }
  });
  for (auto& e : errs) if (!e.empty() && err_out.empty()) err_out = e;
  calitas_free(res.counts);
  tm.rows += ms_since(t1);
  if (trace_stages) std::fprintf(stderr, "[calitas] search_variants: a batch (contig %d ..) lifted %.1f .. %.1f ms\n", wins[0].contig, ms_since(t_call) - ms_since(t1), ms_since(t_call));
  return CALITAS_OK;
}

// ---- a contig's end (lifter), and the finisher behind it ------------------------------------------------------------------------------

// The contigs before `upto` have all their batches lifted: finish them, and their rows and publication to the finisher.
int VariantSearch::finish_upto(size_t upto) {
  if (upto <= lifted.contigs_done) return CALITAS_OK;
  const ScopedMs timed{tm.finish};
  const HitList& hits = lifted.hits;
  if (device_merge) {
    // hits[hits_done, ...) lie on contigs [contigs_done, upto), in contig order
    size_t h = lifted.hits_done;
    for (size_t c = lifted.contigs_done; c < upto; c++) {
      size_t e = h;
      while (e < hits.size() && (size_t)hits[e].w->contig == c) e++;
      int r = finish_contig(c, h, e);
      if (r) return r;
      h = e;
      r = finisher.enqueue([this, c](std::string&) -> int { const int rr = finish_rows(c); if (!rr) publish(c + 1, false); return rr; }, 4, nullptr);
      if (r) return r;
    }
  }
  lifted.hits_done = hits.size();
  lifted.contigs_done = upto;
  return CALITAS_OK;
}

// The entries of contig c -- hits[h0, h1), in arrival order -- for the device: the groups' walks and every entry's key (the rows:
// finish_rows, on the finisher, or on demand).
int VariantSearch::finish_contig(size_t c, size_t h0, size_t h1) {
  if (h1 == h0) return CALITAS_OK;
  if (h1 - h0 >= 0xFFFFFFF0ull) return calitas_fail(ctx, CALITAS_EINVAL, "more than 2^32 hits of variant windows on one contig");
  const auto t0 = Clock::now();
  const HitList& hits = lifted.hits;
  const size_t T = (size_t)ctx->pool->size();
  // blocks of hits cut where the chunk changes: hits of two chunks share no variant, hence no group
  std::vector<size_t> cut(T + 1, h1);
  cut[0] = h0;
  for (size_t t = 1; t < T; t++) {
    size_t k = std::max(cut[t - 1], h0 + (h1 - h0) * t / T);
    while (k < h1 && k > h0 && hits[k].w->chunk == hits[k - 1].w->chunk) k++;
    cut[t] = k;
  }
  struct Lite { int start, end, score; uint32_t idx; };
  const int max_overlap = p.max_overlap;
  std::vector<std::vector<uint32_t>> plain(T), kept(T);
  ctx->pool->run([&](int tid) {
    const size_t b = cut[(size_t)tid], e = cut[(size_t)tid + 1];
    if (b >= e) return;
    std::unordered_map<std::string, uint32_t> group_of;
    std::vector<std::vector<Lite>> groups;
    std::string key;
    for (size_t k = b; k < e; k++) {
      const ExtHit& h = hits[k];
      if (h.desc.empty()) { plain[(size_t)tid].push_back((uint32_t)(k - h0)); continue; }
      key.assign(1, (char)h.a->strand);
      key += h.desc;
      auto it = group_of.find(key);
      if (it == group_of.end()) { it = group_of.emplace(key, (uint32_t)groups.size()).first; groups.emplace_back(); }
      groups[it->second].push_back(Lite{h.gstart, h.gstart + h.tlen - 1, h.a->score, (uint32_t)(k - h0)});
    }
    for (auto& hs : groups) {                                                                    // removeOverlaps SR:653-675 on one group
      std::stable_sort(hs.begin(), hs.end(), [](const Lite& x, const Lite& y) { return x.start != y.start ? x.start < y.start : -x.score < -y.score; });
      auto overlap = [](const Lite& x, const Lite& y) { return std::max(0, std::min(x.end, y.end) - std::max(x.start, y.start)); };   // RH:141-144
      size_t i = 0;
      while (i < hs.size()) {
        const Lite hit = hs[i++];
        while (i < hs.size() && overlap(hs[i], hit) >= max_overlap && hs[i].score <= hit.score) i++;
        if (i >= hs.size() || overlap(hs[i], hit) < max_overlap) kept[(size_t)tid].push_back(hit.idx);
      }
    }
  });
  std::vector<uint32_t> order;                                                                    // the entries in tie order (as offsets from h0)
  for (auto& v : plain) order.insert(order.end(), v.begin(), v.end());
  const size_t n_plain = order.size();
  for (auto& v : kept) order.insert(order.end(), v.begin(), v.end());
  const size_t n = order.size();
  ContigExt& x = cx[c];
  x.entry.resize(n);
  x.keys.resize(n);
  for (size_t i = 0; i < n; i++) {
    const ExtHit& h = hits[h0 + order[i]];
    x.entry[i] = &h;
    x.keys[i] = HitsExtKey{h.gstart, h.gstart + h.tlen - 1, h.a->score, (h.a->strand == '-' ? HITS_EXT_MINUS : 0u) | (i >= n_plain ? HITS_EXT_PLACED : 0u)};
  }
  x.ext.contig = (int32_t)c; x.ext.n = (uint32_t)n; x.ext.keys = x.keys.data();
  x.n_plain = n_plain;
  x.row_len.assign(n, 0);
  if (fill_on_host) { x.vid_off.assign(n, 0); x.row_ptr.assign(n, nullptr); }
  tm.groups += ms_since(t0);
  if (trace_stages) std::fprintf(stderr, "[calitas] search_variants: contig %zu: groups and keys %.1f .. %.1f ms\n", c, ms_since(t_call) - ms_since(t0), ms_since(t_call));
  return CALITAS_OK;
}

// ---- the calling thread, once the walk is over ----------------------------------------------------------------------------------------

int VariantSearch::drain() {
  const ScopedMs timed{tm.drain};
  const int r0 = builder.drain(&tm.wait_builder, &err);
  const int ra = aligner.drain(&tm.wait, &err);
  const int rb = two_aligners ? aligner2.drain(&tm.wait, &err) : CALITAS_OK;
  const int rl = lifter.drain(&tm.wait, &err);
  const int rf = finisher.drain(&tm.wait, &err);
  return r0 ? r0 : ra ? ra : rb ? rb : rl ? rl : rf;
}

int VariantSearch::give_up(int rc) {
  publish(nc, true);
  if (helper.t.joinable()) helper.t.join();
  if (hr.tsv != user_dst) calitas_free(hr.tsv);                   // (never the caller's own block)
  if (!err.empty()) return calitas_fail(ctx, rc != CALITAS_OK ? rc : CALITAS_EINVAL, err);   // (a stage's own text, or this thread's)
  return rc;                                                      // (the context's error text was set where the call failed)
}

// What the variant half built is millions of small heap blocks (descriptions, VCF records, arenas): handed back by all workers, not
// by the one thread that happens to leave the function.
void VariantSearch::teardown() {
  const auto t0 = Clock::now();
  HitList& hits = lifted.hits;
  std::deque<Batch>& kept_windows = lifted.kept_windows;
  std::vector<calitas_aln_t*>& kept_out = lifted.kept_out;
  ctx->pool->for_blocks(hits.size(), [&](size_t b, size_t e, int) { for (size_t k = b; k < e; k++) std::string().swap(hits[k].desc); });
  ctx->pool->for_blocks(vcf.parts.size(), [&](size_t b, size_t e, int) { for (size_t k = b; k < e; k++) std::vector<Var>().swap(vcf.parts[k]); });
  ctx->pool->for_blocks(kept_windows.size(), [&](size_t b, size_t e, int) { for (size_t k = b; k < e; k++) kept_windows[k] = Batch(); });
  ctx->pool->for_blocks(kept_out.size(), [&](size_t b, size_t e, int) { for (size_t k = b; k < e; k++) { calitas_free(kept_out[k]); kept_out[k] = nullptr; } });
  // the contigs' row blobs (1.1 GB at full size) and entry tables, and the big tables themselves: the kernel clears pages as they are
  // handed back, on the thread that hands them back -- one thread per block instead of this one for all of them on the way out
  ctx->pool->for_blocks(cx.size() + 2, [&](size_t b, size_t e, int) {
    for (size_t k = b; k < e; k++) {
      if (k < cx.size()) {
        std::vector<std::string>().swap(cx[k].segs);
        std::vector<std::string>().swap(cx[k].segs_placed);
        std::vector<uint32_t>().swap(cx[k].row_len);
        std::vector<uint32_t>().swap(cx[k].vid_off);
        std::vector<const char*>().swap(cx[k].row_ptr);
        std::vector<HitsExtKey>().swap(cx[k].keys);
        std::vector<uint64_t>().swap(cx[k].row_off);
        std::vector<const ExtHit*>().swap(cx[k].entry);
      } else if (k == cx.size()) {
        hits.release();
      } else {
        std::vector<Var*>().swap(vcf.at);
      }
    }
  });
  if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] search_variants: teardown %.1f ms\n", ms_since(t0));
}

// The device merge's end: the helper's text is the call's.  *fall_back: a stage of the device path declined -- nothing is returned here,
// the caller merges on the host.
int VariantSearch::deliver(char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows, uint64_t* n_windows, bool* fall_back) {
  helper.t.join();
  if (fill_on_host) {                                             // the rows the filler stage still owes the text
    std::string fe;
    const int fr = filler.drain(nullptr, &fe);
    if (hr.rc == CALITAS_OK && (fr || !fe.empty())) { hr.rc = fr ? fr : CALITAS_EINVAL; if (!fe.empty()) calitas_fail(ctx, hr.rc, fe); if (hr.tsv != user_dst) calitas_free(hr.tsv); hr.tsv = nullptr; }
  }
  if (hr.rc != CALITAS_OK) {
    if (hr.tsv != user_dst) calitas_free(hr.tsv);
    if (!hr.declined) { teardown(); return hr.rc; }
    if (TUNE_GET("CALITAS_TRACE")) std::fprintf(stderr, "[calitas] search_variants: the device row stage declined, merging on the host\n");
    *fall_back = true;
    return CALITAS_OK;
  }
  const size_t n_hits = lifted.hits.size(), n_vcf = vcf.size();
  if (TUNE_GET("CALITAS_FREE_NOW")) teardown();
  else {
    // millions of small heap blocks and a few gigabytes of tables: nobody waits for them (0.17 s per call at full size even with
    // every worker handing them back) -- they go to the library's own thread as they are.  (cx goes with its callbacks in it: they
    // point at this call and are dropped there, never called -- the helper is joined and the filler drained.)
    struct Garbage { HitList h; VarTable v; std::deque<Batch> kw; std::vector<calitas_aln_t*> ko; std::vector<ContigExt> c; };
    auto g = std::make_shared<Garbage>();
    g->h = std::move(lifted.hits); g->v = std::move(vcf); g->kw = std::move(lifted.kept_windows); g->ko = std::move(lifted.kept_out); g->c = std::move(cx);
    calitas_reap_later([g]() mutable { for (auto* o : g->ko) calitas_free(o); g.reset(); });
  }
  *tsv = hr.tsv;
  if (tsv_bytes) *tsv_bytes = hr.bytes;
  if (n_rows) *n_rows = hr.rows;
  if (n_windows) *n_windows = walked.windows_total;
  if (TUNE_GET("CALITAS_TRACE"))
    std::fprintf(stderr, "[calitas] search_variants: VCF %.1f ms (%zu records), %llu windows: walked and handed over in %.1f ms (waiting for the builder stage %.1f ms; there: built in %.1f ms, waiting for the aligner threads %.1f ms), stages drained in %.1f ms (align %.1f ms, keys %.1f ms there), "
                         "contigs finished in %.1f ms (groups %.1f + rows %.1f ms) of %zu hits (%llu rows made, %.1f ms of them on demand; %llu written into the text on the host in %.1f ms), "
                         "variant half done at %.1f ms; beside it the reference search with those hits on the device %.1f ms; call %.1f ms, %.2f s of CPU time\n",
                 tm.parse, n_vcf, (unsigned long long)walked.windows_total, tm.walk, tm.wait_builder, tm.build, tm.wait, tm.drain, (double)tm.ns_align.load() / 1e6, tm.rows, tm.finish, tm.groups, tm.make, n_hits, (unsigned long long)tm.rows_made.load(), (double)tm.ns_demand.load() / 1e6, (unsigned long long)tm.rows_filled.load(), (double)tm.ns_fill.load() / 1e6, tm.variant_half, hr.ms, ms_since(t_call), cpu_seconds() - cpu0);
  return CALITAS_OK;
}

// CALITAS_TWIN_STATS: how many hits of variant windows that touch no variant repeat a reference hit exactly
void VariantSearch::twin_stats(const calitas_aln_t* ref_alns, uint64_t n_ref) const {
  const HitList& hits = lifted.hits;
  std::vector<std::array<int64_t, 3>> keys(n_ref);
  for (uint64_t i = 0; i < n_ref; i++) {
    const calitas_aln_t& a = ref_alns[i];
    keys[i] = {((int64_t)a.contig_index << 32) | (uint32_t)a.guide_start_offset, ((int64_t)(a.guide_start_offset + target_length(a) - 1) << 8) | (uint8_t)a.strand, a.score};
  }
  std::sort(keys.begin(), keys.end());
  uint64_t plain = 0, twins = 0, with_desc = 0, shown = 0;
  for (size_t hk = 0; hk < hits.size(); hk++) {
    const ExtHit& h = hits[hk];
    if (!h.desc.empty()) { with_desc++; continue; }
    plain++;
    const std::array<int64_t, 3> k{((int64_t)h.w->contig << 32) | (uint32_t)h.gstart, ((int64_t)(h.gstart + h.tlen - 1) << 8) | (uint8_t)h.a->strand, h.a->score};
    if (std::binary_search(keys.begin(), keys.end(), k)) twins++;
    else if (shown++ < 8)
      std::fprintf(stderr, "[calitas] no twin: contig %d start %d len %d strand %c score %d, window start %d len %zu, aln offsets %d..%d\n", h.w->contig, h.gstart, h.tlen,
                   (char)h.a->strand, h.a->score, h.w->start, (size_t)h.w->len, h.a->start_offset, h.a->end_offset);
  }
  std::fprintf(stderr, "[calitas] variant-window hits: %zu, %llu with a description, %llu without, of those %llu repeat a reference hit\n", hits.size(),
               (unsigned long long)with_desc, (unsigned long long)plain, (unsigned long long)twins);
}

// On the host (a stage the device declines: -O 0, a window beyond the device filter, an overlap cluster beyond one lane's walk):
// reference windows on the GPU, their alignment records back, removeOverlaps + sort over everything.
int VariantSearch::merge_on_host(char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows, uint64_t* n_windows) {
  calitas_aln_t* ref_alns = nullptr;
  uint64_t n_ref = 0;
  {
    const auto t0 = Clock::now();
    const int rc = calitas_search_impl(ctx, 1, guide, params, &ref_alns, &n_ref);
    if (rc) { teardown(); return rc; }
    tm.ref = ms_since(t0);
  }
  // the rows of the kept variant-window hits are made on the way out
  const HitList& hits = lifted.hits;
  std::vector<calitas_ext_hit_t> ext(hits.size());
  for (size_t k = 0; k < hits.size(); k++) {
    const ExtHit& h = hits[k];
    ext[k].contig_index = h.w->contig; ext[k].coordinate_start = h.gstart; ext[k].end = h.gstart + h.tlen - 1; ext[k].score = h.a->score;
    ext[k].strand = (int8_t)h.a->strand; ext[k].variant_description = h.desc.empty() ? nullptr : h.desc.c_str(); ext[k].row = nullptr;
  }
  if (TUNE_GET("CALITAS_TWIN_STATS")) twin_stats(ref_alns, n_ref);
  if (!id.need()) { calitas_free(ref_alns); teardown(); return calitas_fail(ctx, CALITAS_EIO, id.md5_err); }   // (the rows below name the VCF)
  uint64_t nr = 0;
  const auto t_merge = Clock::now();
  *tsv = hits_tsv(ref, gh, gid, p, ref_alns, n_ref, version, stamp, &nr, ctx->pool, calitas_out_alloc, ext.data(), (uint64_t)ext.size(),
                  [](void* user, uint64_t e, std::string& row) {
                    auto* s = static_cast<const VariantSearch*>(user);
                    row.clear();
                    make_row(s->row_in, s->lifted.hits[(size_t)e], s->id.vid, row, false, nullptr);
                  }, this);
  calitas_free(ref_alns);
  const size_t n_vcf_records = vcf.size();
  teardown();
  if (!*tsv) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  if (user_dst) {                                                 // (the merge on the host built a block of the library's: into the caller's buffer)
    const size_t len = std::strlen(*tsv);
    if ((uint64_t)len + 1 > user_cap) {
      calitas_free(*tsv); *tsv = nullptr;
      return calitas_fail(ctx, CALITAS_EINVAL, "the destination buffer is too small for the text (" + std::to_string(user_cap) + " bytes; " + std::to_string(len + 1) + " needed)");
    }
    std::memcpy(user_dst, *tsv, len + 1);
    calitas_free(*tsv);
    *tsv = user_dst;
  }
  if (tsv_bytes) *tsv_bytes = std::strlen(*tsv);
  if (n_rows) *n_rows = nr;
  if (n_windows) *n_windows = walked.windows_total;
  tm.merge = ms_since(t_merge);
  if (TUNE_GET("CALITAS_TRACE"))
    std::fprintf(stderr, "[calitas] search_variants: reference search %.1f ms, VCF %.1f ms (%zu records), %llu windows: align %.1f ms, rows %.1f ms, merge %.1f ms, call %.1f ms\n",
                 tm.ref, tm.parse, n_vcf_records, (unsigned long long)walked.windows_total, (double)tm.ns_align.load() / 1e6, tm.rows, tm.merge, ms_since(t_call));
  return CALITAS_OK;
}

}  // namespace calitas

// user_dst / user_cap: calitas_search_variants_into -- the text goes to the caller's (page-locked) buffer, *tsv = user_dst on success.
static int search_variants_impl(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                                const char* vcf_path, const char* chrom, const char* vcf_id, const char* aligner_version,
                                const char* time_stamp, char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows, uint64_t* n_windows,
                                char* user_dst, uint64_t user_cap) {
  if (!ctx) return CALITAS_EINVAL;
  if (!guide || !params || !vcf_path || !tsv) return calitas_fail(ctx, CALITAS_EINVAL, "NULL argument");
  *tsv = nullptr;
  if (tsv_bytes) *tsv_bytes = 0;
  if (n_rows) *n_rows = 0;
  if (n_windows) *n_windows = 0;
  if (!ctx->has_ref) return calitas_fail(ctx, CALITAS_ESTATE, "calitas_set_reference has not been called");
  if (params->first_window != 0 || params->n_windows != 0)
    return calitas_fail(ctx, CALITAS_EINVAL, "a window range (first_window / n_windows) is for calitas_search only: removeOverlaps needs every alignment of a contig");
  GuideHost gh;
  {
    std::string e = make_guide_host(*guide, gh);
    if (!e.empty()) return calitas_fail(ctx, CALITAS_EINVAL, e);
  }
  std::string version, stamp;
  calitas_default_version_and_stamp(aligner_version, time_stamp, version, stamp);

  VariantSearch s(ctx, guide, guide_id, params, std::move(gh), vcf_path, chrom, vcf_id, std::move(version), std::move(stamp), user_dst, user_cap);
  int rc = s.set_up();                                            // (the md5 thread runs from here on)
  if (rc) return rc;
  s.start_threads();                                              // filler and helper (the device merge's), the stages, the VCF reader
  rc = s.walk();                                                  // every window listed and handed over, contig by contig
  { const int dr = s.drain(); if (rc == CALITAS_OK) rc = dr; }    // ... and aligned, lifted and -- the device merge's -- finished
  if (rc != CALITAS_OK || !s.err.empty()) return s.give_up(rc);
  s.tm.variant_half = ms_since(s.t_call);
  if (s.device_merge) {
    bool fall_back = false;
    rc = s.deliver(tsv, tsv_bytes, n_rows, n_windows, &fall_back);
    if (!fall_back) return rc;
  }
  return s.merge_on_host(tsv, tsv_bytes, n_rows, n_windows);
}

extern "C" int calitas_search_variants(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                                       const char* vcf_path, const char* chrom, const char* vcf_id, const char* aligner_version,
                                       const char* time_stamp, char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows, uint64_t* n_windows) {
  return search_variants_impl(ctx, guide, guide_id, params, vcf_path, chrom, vcf_id, aligner_version, time_stamp, tsv, tsv_bytes, n_rows, n_windows, nullptr, 0);
}

extern "C" int calitas_search_variants_into(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params,
                                            const char* vcf_path, const char* chrom, const char* vcf_id, const char* aligner_version,
                                            const char* time_stamp, char* dst, uint64_t dst_capacity, uint64_t* tsv_bytes, uint64_t* n_rows,
                                            uint64_t* n_windows) {
  if (!ctx) return CALITAS_EINVAL;
  if (!dst || dst_capacity < 2) return calitas_fail(ctx, CALITAS_EINVAL, "no destination buffer");
  char* text = nullptr;
  return search_variants_impl(ctx, guide, guide_id, params, vcf_path, chrom, vcf_id, aligner_version, time_stamp, &text, tsv_bytes, n_rows, n_windows, dst, dst_capacity);
}
