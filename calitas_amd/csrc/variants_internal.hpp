// variants_internal.hpp -- private to the variants*.cpp units: the types of the variant branch (VCF records, windows, arenas, hits), the
// stage thread, the state of one call (VariantSearch) and the prototypes the units share.  Everything here stays out of the library's
// dynamic symbol table.
//
//   variants_vcf.cpp      the VCF reader (parse_record, read_vcf), the MD5 and the identifier "name:md5", calitas_vcf_identifier / _records
//   variants_window.cpp   the four functions restated from the reference, and the walk that lists what every window is made of
//   variants_rows.cpp     the row of a hit of a variant window (make_row) and the rows of a contig's entries for the device
//   variants.cpp          the stages of a call, delivery, the merge on the host, the two C entry points
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "tuning.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

// One element in place, more on the heap: a VCF record has one ALT and one AF value nearly always, and three million records with two
// small heap blocks each were six million allocations per call to make -- and to hand back.
template <typename T>
struct Few {
  T first{};
  std::vector<T> rest;
  uint32_t n = 0;
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  const T& operator[](size_t i) const { return i == 0 ? first : rest[i - 1]; }
  template <class... A>
  void emplace_back(A&&... a) { if (n == 0) first = T(std::forward<A>(a)...); else rest.emplace_back(std::forward<A>(a)...); n++; }
  void push_back(const T& v) { emplace_back(v); }
  void clear() { n = 0; rest.clear(); }
};

struct Var {
  std::string chrom, id, ref;
  int pos = 0, end = 0;                    // 1-based; fgbio Variant.end
  Few<std::string> alts;
  Few<float> afs;
};

struct Allele {                            // VariantAllele SR:105-110
  const Var* v;
  int alt;                                 // index into v->alts
  float af;
};

struct CigarEl { char op; int n; };

// VariantWindow SR:118-157.  A view: alleles, cigar and bases live in the arena of the worker that built the window (three million
// windows with three small heap blocks each cost more to allocate and free than to align).
struct Window {
  int contig = 0, start = 0;               // start: 1-based reference position of the first base
  uint32_t chunk = 0;                      // serial number of the nextChunk() cluster it came from: windows of two chunks share no variant
  const Allele* variants = nullptr; int nv = 0;
  const CigarEl* cigar = nullptr; int nc = 0;
  const char* bases = nullptr; int len = 0;
};
struct Arena { std::vector<char> bases; std::vector<Allele> alleles; std::vector<CigarEl> cigars; };
struct ArenaMark { size_t bases, alleles, cigars; };   // where a window's pieces start in its arena (pointers are set once the arena is complete)

// The records of a VCF in file order.  They stay in the blocks the workers parsed them into (one contiguous table of three million
// records is 460 MB touched for the first time by ONE thread: 0.18 of the file's 0.3 s); at[i] finds record i.
struct VarTable {
  std::vector<std::vector<Var>> parts;
  std::vector<Var*> at;                    // room for every line of the file; at[0, ready) are there
  // The file is parsed in waves (read_vcf) while the caller already walks the records of the waves before: have(i) waits until record i
  // is there or the file is done.  (Behind a pointer: the table itself moves -- into the call's garbage, at the end.)
  struct Sync { std::mutex mu; std::condition_variable cv; std::atomic<size_t> ready{0}; std::atomic<bool> done{false}; };
  std::unique_ptr<Sync> sync{new Sync()};
  size_t seen = 0;                         // (the consumer's copy of ready: no atomic load per record)
  size_t size() const { return sync->ready.load(std::memory_order_acquire); }
  Var& operator[](size_t i) { return *at[i]; }
  const Var& operator[](size_t i) const { return *at[i]; }
  bool have(size_t i) {
    if (i < seen) return true;
    seen = sync->ready.load(std::memory_order_acquire);
    if (i < seen) return true;
    std::unique_lock<std::mutex> lk(sync->mu);
    sync->cv.wait(lk, [&] { return i < sync->ready.load(std::memory_order_acquire) || sync->done.load(std::memory_order_acquire); });
    seen = sync->ready.load(std::memory_order_acquire);
    return i < seen;
  }
  void publish(size_t ready, bool done) {
    { std::lock_guard<std::mutex> lk(sync->mu); sync->ready.store(ready, std::memory_order_release); if (done) sync->done.store(true, std::memory_order_release); }
    sync->cv.notify_all();
  }
};

// A thread that runs jobs in the order they are handed over (a stage of the variant branch's pipeline).  After a job has failed the
// ones behind it are dropped -- but a dropped job's `skipped` handler still runs, in the job's place: whatever a job owes OTHER threads
// (its turn in the order in which batches reach the lifter) is paid there, so nobody waits for a job that will never run.  drain()
// reports the failure.  A stage that is destroyed with jobs still queued (the calling thread left through an exception) drops them
// the same way before it joins its thread.
struct StageThread {
  struct Job { std::function<int(std::string&)> run; std::function<void()> skipped; };
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> jobs;
  bool busy = false, quit = false;
  int rc = CALITAS_OK;
  std::string err;
  std::thread t;
  void start(int device) {
    t = std::thread([this, device] {
      if (device >= 0) (void)hipSetDevice(device);
      for (;;) {
        Job job;
        bool skip = false;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return !jobs.empty() || quit; });
          if (jobs.empty()) return;
          job = std::move(jobs.front());
          jobs.pop_front();
          busy = true;
          skip = quit || rc != CALITAS_OK || !err.empty();
        }
        cv.notify_all();
        int r = CALITAS_OK;
        std::string e;
        try {
          if (!skip) r = job.run(e);
          else if (job.skipped) job.skipped();
        } catch (const std::exception& x) { r = CALITAS_EHIP; e = std::string("a stage of the variant branch ended with an exception: ") + x.what(); }
        catch (...) { r = CALITAS_EHIP; e = "a stage of the variant branch ended with an exception"; }
        job = Job();
        {
          std::lock_guard<std::mutex> lk(mu);
          busy = false;
          if (r && rc == CALITAS_OK) rc = r;
          if (!e.empty() && err.empty()) err = e;
        }
        cv.notify_all();
      }
    });
  }
  // hands a job over; waits while max_waiting jobs are waiting (ms_wait: that time is added to it)
  // (a job refused here -- the stage has failed -- has NOT been queued: its `skipped` handler runs on the calling thread, now)
  int enqueue(std::function<int(std::string&)> job, size_t max_waiting, double* ms_wait, std::function<void()> skipped = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return jobs.size() < max_waiting; });
    if (ms_wait) *ms_wait += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != CALITAS_OK || !err.empty()) {                      // (the caller learns the reason from drain())
      const int r = rc != CALITAS_OK ? rc : CALITAS_EINVAL;
      lk.unlock();
      if (skipped) skipped();
      return r;
    }
    jobs.push_back(Job{std::move(job), std::move(skipped)});
    lk.unlock();
    cv.notify_all();
    return CALITAS_OK;
  }
  // every job handed over has run
  int drain(double* ms_wait, std::string* err_out) {
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return jobs.empty() && !busy; });
    if (ms_wait) *ms_wait += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (err_out && !err.empty() && err_out->empty()) *err_out = err;
    return rc;
  }
  ~StageThread() {
    if (!t.joinable()) return;
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    cv.notify_all();
    t.join();
  }
};

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }
struct ScopedMs {                                                  // adds the time it lived to `ms`
  double& ms;
  Clock::time_point t0 = Clock::now();
  ~ScopedMs() { ms += ms_since(t0); }
};

// ---- variants_vcf.cpp -----------------------------------------------------------------------------------------------------------------
// The records of `chrom` (all: null) into `out`, published wave by wave; "" or the error's text.
std::string read_vcf(const char* path, const char* chrom, WorkerPool* pool, VarTable& out);
std::string md5_file(const char* path, std::string& hex);
// ReferenceHit's VCF identifier (RH:175-183): "<file name>:<md5>"; with 32 zeros for an MD5 it is as long as the real one will be
std::string vcf_identifier(const char* vcf_path, const std::string& md5_hex);

// ---- variants_window.cpp --------------------------------------------------------------------------------------------------------------
std::vector<std::vector<int>> allele_combos_counts(const std::vector<int>& counts);
bool is_valid(const std::vector<const Var*>& vs);
std::string build_window(const Var* const* variants, const int* alleles, size_t nv, int contig, const PackedRef& ref, int padding, Arena& A,
                         std::string& tmp, std::vector<CigarEl>& ctmp, Window& w, ArenaMark& mark);
bool ref_offset_at(const Window& w, int offset, bool preceding, int& out);
// lifted coordinates of an alignment of a window (SR:615-620); false: "Query bases can't be present at operator D."
inline bool lift(const Window& w, const calitas_aln_t& a, int& start, int& end, int& gstart, int& gend) {
  return ref_offset_at(w, a.start_offset, true, start) && ref_offset_at(w, a.end_offset, false, end) &&
         ref_offset_at(w, a.guide_start_offset, true, gstart) && ref_offset_at(w, a.guide_end_offset, false, gend);
}
// what an alignment covers of its target: its columns without the insertions
inline int target_length(const calitas_aln_t& a) {
  int n = 0;
  for (int i = 0; i < a.n_ops; i++) if (a.ops[i] != 'I') n++;
  return n;
}
// the variants under a hit with the lifted coordinates [start, end] (RH:211), in the window's order
template <class F>
inline void for_variants_under(const Window& w, int start, int end, F&& f) {
  for (int k = 0; k < w.nv; k++) {
    const Allele& al = w.variants[k];
    if (start <= al.v->pos - 1 && al.v->pos - 1 <= end) f(al);
  }
}

// ---- variants_rows.cpp ----------------------------------------------------------------------------------------------------------------
// Every alignment of every variant window is a hit as far as removeOverlaps goes, but most of them repeat a reference hit (the part
// of the window the variant does not touch) and lose against it there: a hit gets its key when it is lifted -- lifted coordinates, score,
// variant_description -- on the worker pool, and its row only if it is kept (make_row, called back from the row stage of hits_tsv).
struct ExtHit { const Window* w; const calitas_aln_t* a; int gstart, tlen; std::string desc; };
// (in pieces that never move: the helper thread makes rows from entries of a published contig -- through pointers taken when the contig was
// finished -- while the lifter thread appends the next contigs' hits)
struct HitList {
  enum : size_t { kPiece = 1u << 16 };
  std::vector<std::unique_ptr<ExtHit[]>> pieces;
  size_t n = 0;
  size_t size() const { return n; }
  ExtHit& operator[](size_t i) { return pieces[i >> 16][i & (kPiece - 1)]; }
  const ExtHit& operator[](size_t i) const { return pieces[i >> 16][i & (kPiece - 1)]; }
  void resize(size_t m) {                                                                         // (grows only)
    while (pieces.size() * kPiece < m) pieces.emplace_back(new ExtHit[kPiece]);
    n = m;
  }
  void release() { std::vector<std::unique_ptr<ExtHit[]>>().swap(pieces); n = 0; }
};
std::string display_string(const Allele& a);                      // VariantAllele.displayString SR:108
// What a row is made of besides the hit: all of it constant during a call.
struct RowInputs {
  const PackedRef& ref;
  const GuideHost& gh;
  const std::string& gid;
  const RowStrings& rs;                                            // the pieces of a row that do not depend on the hit
  std::string build_with_variants;                                 // genome_build of a row that names a variant (RH:208)
};
// The row of a kept hit (RH:210-254 with the window's own bases, SR:598-613), appended to `row` without a newline.
// compact: without guide_id and protospacer and with "\n" for a tail (post.hpp, compact_row_strings_keep_build) -- what the device's
// row stage is given when the per-contig texts cross PCIe compact; genome_build stays: a row with a variant has "<build>+variants".
// vid: the identifier's text to put into the row -- the real one, or its placeholder for rows that are made before the VCF's MD5 is
// known; vid_at (may be null): where, counted from the row's first byte, it went (0: the row names no variant).
void make_row(const RowInputs& in, const ExtHit& h, const std::string& vid, std::string& row, bool compact, uint32_t* vid_at);

// ---- the state of one call ------------------------------------------------------------------------------------------------------------
struct Batch { std::vector<Window> wins; std::vector<Arena> arenas; };
struct Aligned { calitas_aln_t* out = nullptr; uint64_t n_out = 0; uint32_t* counts = nullptr; };   // what calitas_align_windows gave for a batch
// what each window of a batch to come is made of (variants and alleles), as the walk lists them
struct Spec { std::vector<uint32_t> off{0}; std::vector<const Var*> v; std::vector<int> a, contig; std::vector<uint32_t> chunk; };
// A contig's entries for the device.  cx[c] is the lifter's until finish_contig(c) returns, the finisher's until it publishes c, then
// the helper's and the filler's.
struct ContigExt {
  std::vector<HitsExtKey> keys; std::vector<uint64_t> row_off;
  std::vector<std::string> segs;                                // the rows' text as the workers wrote it: a block of rows each
  std::vector<const char*> seg_ptr; std::vector<uint64_t> seg_off;
  std::vector<const ExtHit*> entry;                              // the entries in tie order: the plain ones, then the placed ones
  std::vector<uint32_t> row_len;
  std::vector<uint32_t> vid_off;                                 // rows filled in on the host: where a row holds the VCF's identifier (0: nowhere)
  std::vector<const char*> row_ptr;                              // ... and where the row stands in its buffer
  size_t n_plain = 0;
  std::vector<std::string> segs_placed;                          // the placed entries' rows (segs: the plain entries')
  HitsExt ext;
};

// One call of calitas_search_variants: its inputs, what each of its threads owns, and the threads themselves.  search_variants_impl
// (variants.cpp) builds one on its stack and calls the steps in order; the stages' jobs and the device's callbacks hold a pointer to it.
struct VariantSearch {
  static constexpr size_t kBatch = 65536;                          // windows per batch

  // -- the call's inputs and what follows from them: set by the constructor, constant once a thread runs
  calitas_ctx* const ctx;
  const calitas_guide_t* const guide;
  const calitas_params_t* const params;
  const char* const vcf_path;
  const char* const chrom;
  char* const user_dst; const uint64_t user_cap;                   // calitas_search_variants_into: the caller's buffer for the text
  const PackedRef& ref;
  const calitas_params_t& p;
  calitas_params_t ap;                                             // the explicit-target pass
  const GuideHost gh;
  const std::string gid;
  std::string version, stamp;
  const RowStrings rs;
  const RowInputs row_in;
  const int padding;                                               // SR:575 (query.length - 1 + d + g)
  const size_t nc;                                                 // contigs of the reference
  std::vector<std::string> order;                                  // contigs the iterator walks
  const bool device_merge;
  bool fill_on_host = false, two_aligners = false;                 // (set_up; compact rows: source.compact_rows)
  calitas_ctx* actx;                                               // where the variant windows are aligned: side contexts beside the
  calitas_ctx* actx2 = nullptr;                                    // reference passes (set_up), the call's own for the merge on the host
  const bool trace_stages;                                         // CALITAS_TRACE >= 3: every batch's way through the stages
  const Clock::time_point t_call = Clock::now();
  const double cpu0;

  // -- the VCF's identifier "name:md5" (RH:175-183): the md5 thread writes it, whoever needs it first joins that thread (need)
  struct Identifier {
    std::string vid, md5_err;
    std::string placeholder;                                       // what a row holds in its place until the MD5 is known: as long as it will be
    std::mutex mu;                                                 // (several stages may ask; one of them joins the thread)
    std::thread md5_thread;
    Identifier(const char* vcf_path, const char* vcf_id);
    bool need() { std::lock_guard<std::mutex> lk(mu); if (md5_thread.joinable()) md5_thread.join(); return md5_err.empty(); }
    ~Identifier() { if (md5_thread.joinable()) md5_thread.join(); }
  } id;

  // -- the VCF: the reader thread fills it, the walk follows record by record (VarTable::have)
  VarTable vcf;
  std::string vcf_err;

  // -- the calling thread's: the walk
  struct Walk {
    Spec spec;                                                     // the windows listed since the last batch went to the builder
    uint32_t chunk_serial = 0;
    size_t contigs_asked = 0;                                      // (this thread's side of lifted.contigs_done)
    uint64_t windows_total = 0;
  } walked;
  std::string err;                                                 // this thread's error, or -- from drain() on -- a stage's own text

  // -- batch k's turn at the lifter (pass_turn): batches_handed is the builder thread's, batches_lifting under mu
  struct Turns { std::mutex mu; std::condition_variable cv; uint64_t batches_handed = 0, batches_lifting = 0; } turns;
  std::atomic<int> batch_serial{0};                                // (batches through align_part, for CALITAS_FAIL_ALIGN_BATCH)

  // -- the lifter thread's; hits[] grows there only, everybody else reads published contigs through the pointers in cx[c].entry
  struct Lifted {
    HitList hits;
    std::deque<Batch> kept_windows;                                // the windows and alignment records behind the hits
    std::vector<calitas_aln_t*> kept_out;
    size_t contigs_done = 0, hits_done = 0;
  } lifted;

  // -- the contigs' entries and their publication to the helper (HitsExtSource::get waits here)
  std::vector<ContigExt> cx;
  struct Publication { std::mutex mu; std::condition_variable cv; size_t published = 0; bool give_up = false; } pub;   // contigs [0, published) have their entries
  HitsExtSource source;
  struct HelperResult { int rc = CALITAS_OK; bool declined = false; char* tsv = nullptr; uint64_t bytes = 0, rows = 0; double ms = 0; } hr;

  // -- CALITAS_TRACE: where the time went.  Each is written by one thread (named behind it) and read after the stages have drained.
  struct Times {
    double parse = 0;                                              // vcf reader
    double wait_builder = 0, walk = 0, drain = 0;                  // caller: its waits for the builder stage (wait: the later stages')
    double build = 0, wait = 0;                                    // builder (wait: the caller too, once the builder has drained)
    double rows = 0, finish = 0, groups = 0;                       // lifter
    double make = 0;                                               // finisher
    double ref = 0, merge = 0, variant_half = 0;                   // caller, after the drain
    std::atomic<long long> ns_align{0};                            // (two aligner threads add to it)
    std::atomic<long long> ns_demand{0}, ns_fill{0};               // rows on demand: the helper thread's time; the filler's
    std::atomic<uint64_t> rows_made{0}, rows_filled{0};
  } tm;

  // -- THE THREADS, declared behind everything their jobs use: members are destroyed in reverse order, so when the calling thread leaves
  // -- early (an error, an exception while it builds a batch) each of these is stopped and joined while what it touches is still there.
  // The order among them: a stage is declared BEFORE the stages that hand it work, so it is joined after them -- the filler before the
  // helper (whose calls hand it the rows to write), the finisher before the lifter, the lifter before the aligners, the builder last;
  // the helper is given up and joined once the stages are gone, and the reader, which only the walk waits for, goes first.
  StageThread filler;
  struct Helper {                                                  // drives the reference's per-contig passes (search_hits.cpp)
    VariantSearch* s;
    std::thread t;
    ~Helper() { if (t.joinable()) { s->publish(s->nc, true); t.join(); } }
  } helper{this, {}};
  StageThread finisher, lifter, aligner, aligner2, builder;
  struct Reader { std::thread t; ~Reader() { if (t.joinable()) t.join(); } } vcf_reader;

  VariantSearch(calitas_ctx* ctx, const calitas_guide_t* guide, const char* guide_id, const calitas_params_t* params, GuideHost&& gh,
                const char* vcf_path, const char* chrom, const char* vcf_id, std::string version, std::string stamp, char* user_dst,
                uint64_t user_cap);

  // variants.cpp: the steps of a call, in the order search_variants_impl takes them
  int set_up();                                                    // side contexts, which rows go where
  void start_threads();                                            // filler, helper, stages, reader
  int drain();                                                     // everything handed over is in hits[]
  int give_up(int rc);                                             // a failed walk or stage: the helper stopped, the error reported
  int deliver(char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows, uint64_t* n_windows, bool* fall_back);   // the device merge's text
  int merge_on_host(char** tsv, uint64_t* tsv_bytes, uint64_t* n_rows, uint64_t* n_windows);
  void twin_stats(const calitas_aln_t* ref_alns, uint64_t n_ref) const;
  void teardown();
  // ... and the stages
  void publish(size_t upto, bool quit);
  int get_contig(int c, const HitsExt** e);                        // HitsExtSource::get
  int pass_turn(uint64_t k, const std::function<int()>& at_turn);
  int hand_over(Batch&& b, size_t n);                              // builder -> aligner -> lifter
  int hand_over_finish(size_t upto);
  int align_part(calitas_ctx* where, Batch& batch, size_t n, Aligned& res);
  int lift_part(Batch& batch, size_t n, const Aligned& res, std::string& err_out);
  int finish_upto(size_t upto);
  int finish_contig(size_t c, size_t h0, size_t h1);

  // variants_window.cpp: the walk (caller) and the building of a listed batch (builder)
  int walk();
  int emit(const Var* const* vs, const int* al, size_t nv, int contig);
  int flush_spec();
  int finish_contigs(size_t upto);
  int build_spec(const Spec& sp, std::string& e_out);

  // variants_rows.cpp: the rows of a contig's entries (finisher, helper, filler)
  void make_rows(size_t c, size_t lo, size_t hi, const uint8_t* kept, std::vector<std::string>& segs);
  int rows_of(size_t c, HitsExtRows* out);
  int finish_rows(size_t c);
  int fill_rows(size_t c, const uint64_t* place, char* text);
};

}  // namespace calitas
