// search_internal.hpp -- private to the search_*.cpp units: the types one search hands from stage to stage (SearchPlan, DeviceSel,
// LaneText, HitsCall), the lane threads, the CALITAS_TRACE=2 time line, and the prototypes the units share.  What api.cpp,
// align_windows.cpp and the variants*.cpp units call is in ctx.hpp.  Everything here stays out of the library's dynamic symbol table.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ctx.hpp"
#include "tuning.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

// CALITAS_TRACE=2: host-side time line of a call (microseconds since the first mark), one line at the end of calitas_search_hits
struct HostMarks {
  bool on = false;
  std::chrono::steady_clock::time_point t0;
  std::string line;
  void start() { start_at(std::chrono::steady_clock::now()); }
  void start_at(std::chrono::steady_clock::time_point t) { const char* e = TUNE_GET("CALITAS_TRACE"); on = e && std::atoi(e) >= 2; line.clear(); t0 = t; }
  void mark(const char* what) {
    if (!on) return;
    char b[64];
    std::snprintf(b, sizeof b, " %s %.0f", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    line += b;
  }
  void dump(int lane = -1) { if (on) std::fprintf(stderr, "[calitas] host marks (us)%s%s:%s\n", lane >= 0 ? " lane " : "", lane >= 0 ? std::to_string(lane).c_str() : "", line.c_str()); }
};
inline thread_local HostMarks g_marks;   // one per thread for all units (the lane threads dump theirs, the caller's thread its own)

static inline int fail(calitas_ctx* ctx, int code, const std::string& msg) { return calitas_fail(ctx, code, msg); }
static inline void* out_alloc(size_t size) { return calitas_out_alloc(size); }

// A lane of a chunked search (see calitas_search_hits) is a child context: its own stream, buffers and scratch, the
// parent's resident reference and window table.
static inline calitas_ctx* ref_owner(calitas_ctx* ctx) { return ctx->parent ? ctx->parent : ctx; }

// Everything about one search that does not depend on the lane running it.
struct SearchPlan {
  calitas_params_t p{};
  int n_guides = 0, step = 0, max_total = 0;
  Scores sc{};
  std::vector<GuideHost> gh;
  std::vector<GuideDev> gd;
  uint32_t slots_per_rec = 0, slab_bytes = 0;
  uint64_t slab_per_rec = 0;
  int warm_words = 1;                 // 32-base warm-up words of a scan lane: L + E - 1 <= 32 * warm_words
  uint64_t rec_hint = 0;              // expected scan records of this job (from estimate_scan_records), 0 = unknown
  uint64_t gw_lo = 0, gw_hi = ~0ull;  // global window range of the call (calitas_params_t::first_window / n_windows); all by default
  // the part of the packed reference this job covers
  uint32_t tile_lo = 0, n_tiles = 0;
  uint64_t bases = 0;
  uint64_t win_lo = 0, win_n = 0;     // its entries of the device window table
  // its reference bins (binned.hpp); bin_shift = 0: the binned tail does not take this window size
  int bin_shift = 0;
  uint32_t bin_first = 0, n_bins = 0;
  // calitas_search_hits on a window range (a process of a multi-GPU job): the rows it owns, as keys (contig << 32 | coordinate_start)
  bool owned = false;
  uint64_t own_lo = 0, own_hi = ~0ull;
  bool narrow_tail = false;           // a range of a chunked call that is not the last: its tail shares the chip with the next scan
  bool three_ranges = false;          // a range of a call cut into three or more
  bool last_range = false;            // ... and the last of them: no scan runs beside its tail
  // calitas_search_counts: the lanes count the kept hits into a table of these extents instead of building rows.  The extents are
  // always planned (counts_shape: from the guide and the params alone); `counts` is set by the entry point
  bool counts = false;
  CountsShape cshape;
  // calitas_search_scores: counts mode with the score of every kept hit besides (set with `counts`; the model outlives the call)
  const ScoreModelHost* model = nullptr;
  bool general_tail = false;          // the caller brings hits of its own into the row stage (HitsExt): the general kernels take them, the bins do not
};

// Accepted alignments left on the device by search_impl for calitas_search_hits.
struct DeviceSel {
  bool valid = false;
  const RawAln* d_final = nullptr;
  uint32_t n_sel = 0;
  bool crowded = false;    // some window held more records than a wave filters in registers (select.hip GROUP_MAX)
};

// ---- calitas_search_hits ------------------------------------------------------------------------------------------------

// What one lane contributes to a hits.txt: rows on the device, or rows built by the host stages when a device stage declined.
struct LaneText {
  int rc = CALITAS_OK;
  const char* d_text = nullptr;
  uint64_t bytes = 0, rows = 0;
  uint64_t compact_bytes = 0;          // != 0: the device holds compact rows (post.hpp) of that many bytes; `bytes` is what they expand to
  bool on_host = false;
  bool in_place = false;               // the rows kernel wrote the text to its final place in the caller's page-locked buffer (LaneDest)
  std::string host_rows;
  const HitsWork* rows_by = nullptr;   // the general row stage that wrote d_text (its late flags are looked at once the text has been copied)
  const HitsExt* ext = nullptr;        // the caller's hits whose rows the caller writes into the text itself (HitsExtRows::fill_on_host) ...
  const uint64_t* ext_place = nullptr; // ... and where (HitsResult::ext_place)
  std::vector<uint64_t> counts;        // counts mode (SearchPlan::counts): the lane's table, SearchPlan::cshape.cells() words; no text, bytes = 0
  ScoreWords score;                    // score mode (SearchPlan::model): what the lane's kept hits add up to
  calitas_timing_t tm{};
};

// Where a lane's text finally goes, asked for when its row kernel is about to be launched: page-locked memory the device can address
// and the room there.  false: not known / not addressable -- the text takes the device buffer and the copy.
struct LaneDest { std::function<bool(char** dst, uint64_t* cap)> get; };

constexpr int kOwnedDeclined = -1000;   // (internal) a lane of an owned range (SearchPlan::owned) met bins it leaves to the general kernels
constexpr int kExtDeclined = -1001;     // (internal) a pass that brings hits of the caller's (HitsExt) met a stage the device declines: the caller merges on the host

// What a calitas_search_hits* entry point was asked for, as its arguments came in; the paths behind it (search_hits_attempt,
// search_hits_owned, search_hits_sequential) pass it on whole.
struct HitsCall {
  const calitas_guide_t* guide;
  const std::string& guide_id;
  const calitas_params_t* params;
  const char *aligner_version, *time_stamp;
  char* user_dst = nullptr;                 // the text goes into this caller-owned buffer of user_cap bytes (calitas_search_hits_into) instead
  uint64_t user_cap = 0;                    // of a block of the library; CALITAS_EINVAL when it is too small
  calitas_text_sink_t sink = nullptr;       // per-contig passes: the pieces of the text are handed over as they arrive ...
  void* sink_user = nullptr;
  const HitsExtSource* ext_source = nullptr;   // ... and hits of the caller's own are brought into every contig's row stage
  bool counts = false;                      // calitas_search_counts: no text at all, HitsOut::counts receives the table of the rows
  const ScoreModelHost* model = nullptr;    // calitas_search_scores: with counts, HitsOut::score receives the rows' scores
};
// ... and what it gets back (tsv stays NULL where the text went to a sink).
struct HitsOut {
  char* tsv = nullptr;
  uint64_t bytes = 0, rows = 0;
  std::vector<uint64_t> counts;             // HitsCall::counts: the table, shape.cells() words
  CountsShape shape;
  ScoreWords score;                         // HitsCall::model
  void store(char** t, uint64_t* b, uint64_t* r) const { if (t) *t = tsv; if (b) *b = bytes; if (r) *r = rows; }
};

// search_plan.cpp
int plan_search(calitas_ctx* ctx, int32_t n_guides, const calitas_guide_t* guides, const calitas_params_t* params, SearchPlan& pl);
int ensure_window_table(calitas_ctx* ctx, const SearchPlan& pl, hipStream_t stream);
int ensure_bin_base(calitas_ctx* ctx, SearchPlan& pl, hipStream_t stream);
void fill_kernel_args(calitas_ctx* ctx, const SearchPlan& pl, ScanArgs& sa, AlignArgs& aa);
int lane_prepare(calitas_ctx* ctx, const SearchPlan& pl);
int check_resident(calitas_ctx* ctx, const SearchPlan& pl);
std::vector<std::pair<int, int>> chunk_ranges(const PackedRef& ref, const std::vector<double>& weights);
bool plan_owned_range(const calitas_ctx* ctx, SearchPlan& pl, uint64_t first, uint64_t count);
std::vector<uint64_t> window_prefix(const PackedRef& ref, int step);
int window_contig(const std::vector<uint64_t>& wb, uint64_t w);
void window_start(const std::vector<uint64_t>& wb, int step, uint64_t w, int& c, uint64_t& pos);
void plan_contig_range(const calitas_ctx* ctx, SearchPlan& q, const std::vector<uint64_t>& wb, int c0, int c1);

// search_run.cpp
int queue_scan_inputs(calitas_ctx* ctx, const SearchPlan& pl, hipStream_t stream);
int launch_scan_stage(calitas_ctx* ctx, const SearchPlan& pl, hipStream_t stream, bool inputs_queued = false, bool columnwise = false);
void kernel_times(calitas_ctx* ctx, calitas_timing_t& tm);
hipError_t launch_align_trace(const SearchPlan& pl, const AlignArgs& aa, hipStream_t stream, hipEvent_t trace_done);
int convert_selected(calitas_ctx* ctx, const RawAln* d_final, uint32_t n_sel, const std::vector<GuideHost>& gh, const calitas_params_t& p, int step, calitas_aln_t** out);
int search_run(calitas_ctx* ctx, const SearchPlan& pl, calitas_aln_t** out, uint64_t* n_out, DeviceSel* dev, bool prelaunched, bool resume = false);

// search_lane.cpp
extern std::atomic<double> g_pass_ms[2];   // (trace only) the per-contig passes' search kernels / their wait for the caller's hits, summed by lane_rows
void dma_open_once(calitas_ctx* owner);
int binned_late_failed(calitas_ctx* lane);
int text_to_host(calitas_ctx* owner, calitas_ctx* lane, char* dst, const char* src, size_t n, std::mutex* copy_mu, double* ms_out, hipEvent_t rows_done = nullptr);
void add_lane_timing(calitas_timing_t& tm, const calitas_timing_t& l);
int rows_late_check(calitas_ctx* lane, const LaneText& lt);
int deliver_lane_text(calitas_ctx* owner, calitas_ctx* lane, LaneText& lt, size_t compact_bytes, size_t full_bytes, char* staging, const std::string& head,
                      const std::string& tail, char* dst, std::mutex* copy_mu, const char* whose, hipEvent_t rows_done = nullptr);
double rows_stage_ms(calitas_ctx* lane, const calitas_timing_t& tm);
bool binned_possible(calitas_ctx* lane, const SearchPlan& pl);
hipError_t queue_row_constants(calitas_ctx* lane, const SearchPlan& pl, const RowStrings& rs);
int queue_lane_setup(calitas_ctx* lane, const SearchPlan& pl, const RowStrings* rs, hipStream_t stream, bool* done, bool with_scan_inputs = true);
int lane_rows(calitas_ctx* lane, const SearchPlan& pl, bool prelaunched, const RowStrings& rs, const std::string& guide_id, const std::string& version,
              const std::string& stamp, LaneText& lt, bool hits_prepared = false, const LaneDest* dest = nullptr,
              const HitsExtSource* ext_source = nullptr, int ext_contig = 0);
int ensure_lanes(calitas_ctx* ctx, size_t k);
void release_scratch(calitas_ctx* ctx);

// search_hits.cpp / search_sequential.cpp
// owned: {first window, windows} of a window range (calitas_params_t::first_window / n_windows) whose rows the call returns, all of it
// on the per-bin kernels; *owned_declined: they could not decide it (the caller then takes the slow path), nothing is returned.
int search_hits_attempt(calitas_ctx* ctx, const HitsCall& call, HitsOut& out, const uint64_t* owned = nullptr, bool* owned_declined = nullptr);
int search_hits_sequential(calitas_ctx* ctx, const HitsCall& call, HitsOut& out);
int search_counts_sequential(calitas_ctx* ctx, const HitsCall& call, HitsOut& out);
// What the tails take of a plan's model (hits.hpp: ScoreCall): its words and the letter indices of the guide's positions.
inline ScoreCall score_call(const ScoreModelHost& m, const GuideHost& gh) {
  ScoreCall sc{m.words.data(), {0, 0}, m.top_k, m.regions ? m.regions_dev : RegionsView{}, m.list_mask};
  for (size_t i = 0; i < gh.protospacer.size() && i < 32; i++) sc.letters[i >> 4] |= (uint64_t)score_letter_index(gh.protospacer[i]) << ((i & 15) * 4);
  return sc;
}
// b += a, element by element (tables of one shape: of ranges, contigs, lanes)
inline void add_counts(std::vector<uint64_t>& b, const std::vector<uint64_t>& a) {
  if (b.size() < a.size()) b.resize(a.size(), 0);
  for (size_t i = 0; i < a.size(); i++) b[i] += a[i];
}

}  // namespace calitas

#pragma GCC visibility push(hidden)
// The host threads behind lanes 1..K-1 of a chunked search (the caller's thread drives lane 0).  They live as long as the lanes:
// starting two threads took ~110 us of every call and joining them ~40 us after the last copy had finished -- on the caller's clock.
struct LaneThreads {
  std::vector<std::thread> threads;
  std::mutex m;
  std::condition_variable cv;
  unsigned long gen = 0;
  bool stop = false;
  size_t k = 0;                                    // lanes of the current job (worker i runs job(i) when i < k)
  std::function<void(size_t)> job;
  std::atomic<size_t> remaining{0};
  std::atomic<bool> threw{false};                  // a job ended with an exception (std::bad_alloc, ...): the call fails with CALITAS_EHIP
  std::string what;                                // ... and says which (the first one's text; under m)
  void note(const char* text) {
    std::lock_guard<std::mutex> lk(m);
    if (!threw.load(std::memory_order_relaxed)) what = text ? text : "";
    threw.store(true, std::memory_order_relaxed);
  }
  // Runs fn: an exception must not take the process down (a lane thread has no caller to unwind to), and must not be lost either.
  template <typename F>
  void guarded(F&& fn) {
    try { fn(); }
    catch (const std::exception& e) { note(e.what()); }
    catch (...) { note("an exception that is not a std::exception"); }
  }
  std::string failure() { std::lock_guard<std::mutex> lk(m); return "a lane of the search ended with an exception: " + (what.empty() ? std::string("(no text)") : what); }
  ~LaneThreads() {
    { std::lock_guard<std::mutex> lk(m); stop = true; gen++; }
    cv.notify_all();
    for (auto& t : threads) t.join();
  }
  void ensure(size_t lanes) {                      // workers for lanes 1 .. lanes-1
    while (threads.size() + 1 < lanes) {
      const size_t i = threads.size() + 1;
      threads.emplace_back([this, i] {
        unsigned long seen = 0;
        for (;;) {
          {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return gen != seen; });
            seen = gen;
            if (stop) return;
            if (i >= k) continue;
          }
          guarded([&] { job(i); });
          if (remaining.fetch_sub(1, std::memory_order_acq_rel) == 1) {   // the last lane: wake a caller that has stopped spinning
            { std::lock_guard<std::mutex> lk(m); }
            done_cv.notify_all();
          }
        }
      });
    }
  }
  void start(size_t lanes, std::function<void(size_t)> fn) {
    { std::lock_guard<std::mutex> lk(m); job = std::move(fn); k = lanes; remaining.store(lanes - 1, std::memory_order_relaxed); threw.store(false, std::memory_order_relaxed); gen++; }
    cv.notify_all();
  }
  std::condition_variable done_cv;
  void wait() {                                    // the last lane to finish is the end of the call: watch for it (spinning, then yielding) for 2 ms, then sleep until it says so
    Backoff spin;
    while (remaining.load(std::memory_order_acquire) != 0) {
      // (the caller's own lane of an hg38-sized call ends 0.3 ms before the last one: woken from a condition variable it returned
      // 35 us after that lane had finished)
      if (spin.spins < 256 || spin.waited_us() < 2000) { spin.pause(); continue; }
      std::unique_lock<std::mutex> lk(m);
      done_cv.wait(lk, [&] { return remaining.load(std::memory_order_acquire) == 0; });
    }
  }
};
#pragma GCC visibility pop
