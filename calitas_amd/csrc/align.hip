// align.hip -- the glocal DP on the strips the scan flagged: scan records -> aligner jobs -> filled strips, handed to trace.hip.
//
//  expand_kernel    one lane per scan record: every (record, window) that holds candidate columns becomes a job, and the head of the
//                   job's slab (slab.hpp) is written: geometry, the guide's row sets, the strip's target masks.
//  align_kernel     the glocal DP itself: three score matrices (Diag/Left/Up) with fgbio's tie rules, antidiagonal wavefront with one
//                   lane per query row, neighbours exchanged with DPP wave shifts, trace matrix staged in LDS and copied into the slab
//                   of every job with a passing end column.  Only columns [j - span - 1, j] are filled: by the locality argument in
//                   DESIGN.md this reproduces the value and the trace of every cell on the optimal path of a candidate (L, j) bit
//                   for bit.  Traceback and the PAM extension are trace_kernel's (trace.hip).
//  align_pk_kernel  align_kernel's fill with two jobs per lane group, one in each 16-bit half of the registers.
//  What stands around the two fills (the job range, staging a head, flushing the items, the hand-over) is written once, ahead of them.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "slab.hpp"
#include "tuning.hpp"
#include "refpack.hpp"
#include "kernels.hpp"

namespace calitas {

constexpr int NEG = -(1 << 20);                      // "minus infinity" that survives a few hundred additions
// A job (one scan record: its windows one after the other) takes LPJ lanes of a wave, lane r of them = query row r + 1.  LPJ = 32: two
// jobs per wave, guides up to 32 rows.  LPJ = 21: THREE jobs per wave (lanes 0-20, 21-41, 42-62; lane 63 idles) for guides of up to
// 20 rows -- every search with the usual 20-nt protospacer: 60 of 64 lanes hold a row instead of 40, a third fewer wave instructions
// for the same cells.  (Lane LPJ - 1 of a job is never a row then: it holds "row 0" for the job above it, see the fill.)
// One wave per workgroup: ~11 KB of LDS, which fits on a CU next to four scan workgroups (37 KB each of 160 KB) -- a 256-thread
// workgroup (40 KB) had to wait until the scan of the next range let go of a CU.
// per wave: flush threshold + the most one record iteration can add (jobs x 8 windows x 16 candidates; x 3 when every matrix
// of a cell is an alignment of its own)
constexpr int STAGE_FLUSH = 16;
template <bool PM, int LPJ> constexpr int ITEM_STAGE = STAGE_FLUSH + (PM ? 3 : 1) * (64 / LPJ) * 16;
constexpr int TB_LEN = STRIP_MAX_COLS + 48;          // strip columns + gap + PAM look-ahead
constexpr int TR_STRIDE = 100;                       // bytes per trace row (>= STRIP_MAX_COLS + 4, word aligned; lane r writes byte 99r + t)


__device__ __forceinline__ int shift_up_lane(int v) {
  // value of lane-1 (DPP wave shift right by one); lane 0 keeps its own value, which callers ignore
  return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

__device__ __forceinline__ int comp_mask4(int m) {  // IUPAC set of the complementary base(s)
  return ((m & 1) << 3) | ((m & 2) << 1) | ((m & 4) >> 1) | ((m & 8) >> 3);
}

// ------------------------------------------------------------------------------------------------------------------
// expand_kernel: scan records -> aligner jobs.
//
// Round 5.  align_kernel used to start every record with a chain of five dependent global loads (record -> tile -> contig -> window
// table base -> window bounds) and then fetched the strip's bases column by column: its waves stood in s_waitcnt half their time
// (profiles/r05_pmc_tail_before.txt: SQ_WAIT_ANY 51 % of SQ_WAVE_CYCLES at one or two waves per SIMD) with registers and LDS held
// all the while.  Here that chain runs ONCE per record with a lane per record -- 64 independent chains per wave, thousands of waves --,
// every (record, window) that holds candidate columns gets a number (one atomic per wave and round), and sixteen lanes per job write
// the head of the job's slab: geometry, the guide's row sets, and the strip's target masks decoded from the packed reference (two code
// words and two mask words per sixteen columns; run lookups for exception bases).  align_kernel then needs one 16-byte load per lane
// per job, from an address that depends on nothing but the job's number.
// ------------------------------------------------------------------------------------------------------------------
struct JobSeed {           // phase A -> phase B, through LDS: the job's header words and where its strip starts in the packed reference
  uint32_t slab;           // the job's slab: record x slots_per_rec + window slot
  uint32_t pad;
  uint32_t contig, window_k, n, c0;
  uint32_t cols, what;     // slab_cols(ncols, ntb), slab_what(dir, guide, true_border, L): the header words they become (dir: 0 or 1)
  uint32_t sel;            // the candidate columns inside the window (bits of the record's 16-base word)
  int32_t jbase;
  uint64_t gpos0;          // packed position of strip column c0 + 1 (tb[0]); the columns go up from there (dir 0) or down (dir 1)
};

__device__ __forceinline__ int tmask_at(const Run* runs, int64_t n_runs, uint64_t gpos, uint32_t code, uint32_t exc, int dir) {
  int m;
  if (!exc) {
    m = 1 << code;
  } else {
    int64_t r = run_floor(runs, n_runs, gpos);
    uint8_t ch = 0;
    if (r >= 0 && gpos < runs[r].start + runs[r].len) ch = runs[r].ch;
    m = target_mask(ch);
  }
  if (dir) m = (m & 16) | comp_mask4(m & 15);
  return m;
}

// Sixteen target masks (one 16-byte piece of a strip's tb[]): the bases at packed positions plo .. plo + nv - 1, in column order --
// ascending for the forward strand, descending and complemented for the reverse strand (d2).  cwl / cwh: the code words of plo and of
// plo + nv - 1 (the same word when the piece does not straddle), mwl / mwh likewise for the exception mask.
__device__ __forceinline__ uint4 decode_piece(const Run* runs, int64_t n_runs, uint32_t cwl, uint32_t cwh, uint32_t mwl, uint32_t mwh, uint64_t plo,
                                              int nv, int d2) {
  const uint64_t phi = plo + (uint64_t)(nv - 1);
  const uint64_t cw = ((uint64_t)cwh << 32) | (uint64_t)cwl, mw = ((uint64_t)mwh << 32) | (uint64_t)mwl;
  const uint32_t c32 = (plo >> 4) == (phi >> 4) ? (uint32_t)((uint32_t)cw >> ((plo & 15) * 2)) : (uint32_t)(cw >> ((plo & 15) * 2));
  const uint32_t m16 = ((plo >> 5) == (phi >> 5) ? (uint32_t)((uint32_t)mw >> (plo & 31)) : (uint32_t)(mw >> (plo & 31))) & ((1u << nv) - 1u);
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int ia = d2 ? nv - 1 - i : i;                          // ascending index of column i of the piece (negative beyond it: masked below)
    const uint32_t code = (c32 >> ((ia & 15) * 2)) & 3u;
    uint32_t tm = 1u << (d2 ? 3u - code : code);                 // plain base: its set, complemented for the reverse strand
    if (i >= nv) tm = 0u;
    if (i < 4) w0 |= tm << (i * 8); else if (i < 8) w1 |= tm << ((i - 4) * 8); else if (i < 12) w2 |= tm << ((i - 8) * 8); else w3 |= tm << ((i - 12) * 8);
  }
  // exception bases (N runs, IUPAC codes, padding: rare): their masks come from the run table
  for (uint32_t m = m16; m != 0u; m &= m - 1u) {
    const int ia = __ffs(m) - 1;
    const int tm = tmask_at(runs, n_runs, plo + (uint64_t)ia, 0u, 1u, d2);
    const int i = d2 ? nv - 1 - ia : ia;
    const uint32_t clr = ~(0xFFu << ((i & 3) * 8)), put = (uint32_t)tm << ((i & 3) * 8);
    if ((i >> 2) == 0) w0 = (w0 & clr) | put; else if ((i >> 2) == 1) w1 = (w1 & clr) | put; else if ((i >> 2) == 2) w2 = (w2 & clr) | put; else w3 = (w3 & clr) | put;
  }
  return make_uint4(w0, w1, w2, w3);
}

__global__ __launch_bounds__(256) void expand_kernel(AlignArgs a) {
  CALITAS_TAIL_PRIO();
  if (a.stamps && blockIdx.x == 0 && threadIdx.x == 0) a.stamps[0] = (unsigned long long)wall_clock64();   // (binned.hpp, BIN_BOX_STAMPS)
  __shared__ JobSeed s_seed[4][64];
  __shared__ int s_gint[MAX_GUIDES][4];                           // L, span, min_guide_score, cli_length
  __shared__ __attribute__((aligned(16))) uint8_t s_qmask[MAX_GUIDES][MAX_L];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  for (int i = (int)threadIdx.x; i < a.sp.n_guides; i += (int)blockDim.x) {
    s_gint[i][0] = a.guides[i].L; s_gint[i][1] = a.guides[i].span; s_gint[i][2] = a.guides[i].min_guide_score; s_gint[i][3] = a.guides[i].cli_length;
  }
  for (int i = (int)threadIdx.x; i < a.sp.n_guides * (MAX_L / 4); i += (int)blockDim.x)
    reinterpret_cast<uint32_t*>(s_qmask[i / (MAX_L / 4)])[i % (MAX_L / 4)] = reinterpret_cast<const uint32_t*>(a.guides[i / (MAX_L / 4)].qmask)[i % (MAX_L / 4)];
  __syncthreads();
  uint32_t n_recs = *a.rec_count;
  if (n_recs > a.rec_capacity) n_recs = a.rec_capacity;
  const SearchDev& sp = a.sp;
  const int W = sp.window_size, step = sp.step;
  __shared__ uint32_t s_cnt[4], s_over;
  for (uint32_t blk = blockIdx.x * 256u; blk < n_recs; blk += gridDim.x * 256u) {   // (workgroup-uniform: there are barriers inside)
    // ---- phase A: a lane per record ----
    const uint32_t ri = blk + threadIdx.x;
    ScanRecord rec{0u, 0u};
    if (ri < n_recs) rec = a.recs[ri];
    const uint32_t cmask = rec.info & 0xFFFFu;
    const int dir = (int)((rec.info >> 16) & 1u), gi = (int)((rec.info >> 17) & 0x7Fu);
    uint32_t contig = 0;
    uint64_t gbase = 0, win_lo = 0, win_cnt = 0;
    int L = 0, span = 0, g_cli = 0;
    int64_t p0 = 0, khi = -1, klo = 0;
    if (cmask != 0u && gi < sp.n_guides) {
      L = s_gint[gi][0]; span = s_gint[gi][1]; g_cli = s_gint[gi][3];
      contig = a.tiles[rec.gword / a.tile_words].contig;
      gbase = a.contigs[contig].gbase;
      const uint64_t clen = a.contigs[contig].len;
      win_lo = a.win_base[contig]; win_cnt = a.win_base[contig + 1] - win_lo;
      p0 = (int64_t)((uint64_t)rec.gword * 16 - gbase);          // contig offset of bit 0
      const int64_t plo = p0 + (__ffs(cmask) - 1), phi = p0 + (31 - __clz(cmask));
      klo = (plo - W + 1 + step - 1) / step;                      // ceil((plo - W + 1) / step) for a positive numerator
      if (plo - W + 1 <= 0) klo = 0;
      khi = phi / step;
      if ((uint64_t)plo >= clen) khi = -1;                        // only padding columns: they belong to no window
    }
    // Rounds: round s looks at window klo + s of every record -- a record's candidate columns fall into at most slots_per_rec windows
    // (two with the usual tiling), so this is a loop with a trip count the whole grid shares, and the ballot below is taken in
    // straight-line code.  (A first version let every lane walk to its next window with candidate columns in a `while` with `break`s
    // and took the ballot behind it: the compiler kept the lanes that left the loop empty-handed apart from the others, their ballot
    // came out empty, they left -- and the jobs that phase B hands to THEIR lanes were never written: stale slab heads, at random.)
    for (int round = 0; round < (int)a.slots_per_rec; round++) {
      bool have = false;
      JobSeed seed{};
      const int64_t k = klo + round;
      int2 wab = make_int2(0, 0);
      const bool in_range = k <= khi && (uint64_t)k < win_cnt &&                 // (no such window on this contig: Range(0, len-1, step), SR:52)
                            win_lo + (uint64_t)k >= a.gw_lo && win_lo + (uint64_t)k < a.gw_hi;   // (outside this call's window range)
      if (in_range) wab = a.win[win_lo + (uint64_t)k];            // N-trimmed bounds, precomputed by window_table_kernel
      {
        const int64_t wa = wab.x, wb = wab.y;
        const int n = (int)(wb - wa);
        // candidate columns of this word that fall inside the window
        uint32_t sel = 0;
        for (int b = 0; b < 16; b++) if ((cmask >> b) & 1u) { const int64_t p = p0 + b; if (p >= wa && p < wb) sel |= 1u << b; }
        if (in_range && n >= g_cli && sel != 0u) {                // (n < g_cli: SearchReference.scala:536)
          const int sfirst = __ffs(sel) - 1, slast = 31 - __clz(sel);
          int jmin, jmax, jb;                                     // strand-space columns (1-based)
          if (dir == 0) { jmin = (int)(p0 + sfirst - wa) + 1; jmax = (int)(p0 + slast - wa) + 1; jb = (int)(p0 - wa) + 1; }
          else          { jmin = (int)(wb - (p0 + slast));    jmax = (int)(wb - (p0 + sfirst)); jb = (int)(wb - p0); }
          int c0 = jmin - span - 1;
          if (c0 < 0) c0 = 0;
          const int ncols = jmax - c0;                            // <= 16 + span + 1 <= STRIP_MAX_COLS (host-checked)
          int look = jmax + sp.max_gaps + MAX_PAM_LEN;            // PAM look-ahead, clipped to the window
          if (look > n) look = n;
          const int ntb = look - c0;                              // tb[x] = column c0 + 1 + x
          seed.slab = ri;                                         // (round 0; a later round's jobs get their slabs below)
          seed.contig = contig; seed.window_k = (uint32_t)k; seed.n = (uint32_t)n; seed.c0 = (uint32_t)c0;
          seed.cols = slab_cols(ncols, ntb);
          seed.what = slab_what(dir, gi, c0 == 0, L);
          seed.sel = sel; seed.jbase = jb;
          seed.gpos0 = gbase + (uint64_t)(dir ? wb - c0 - 1 : wa + c0);
          have = true;
        }
      }
      const unsigned long long bal = __ballot(have);
      const bool any_wide = __ballot(have && cols_ntb(seed.cols) > 64) != 0ull;   // (both ballots in straight-line code, see above)

      // Round 0's job lives in slab `record`; a record without one says so there (ncols = 0: align_kernel looks).  The jobs of later
      // rounds -- a second window that holds the same columns: 3 % of the records -- are numbered behind the records' slabs
      // (rec_capacity + k) with ONE atomic per workgroup and round.  (Numbering all jobs with an atomic per wave and round was 3 800
      // returning atomics on one word per hg38-sized pass, 42 of the kernel's 60 us -- DESIGN.md 4.7; a fixed slab per later round
      // instead left align_kernel 120 000 empty slabs to look into, a memory round trip each: +30 us there.)
      if (round == 0 && ri < n_recs && !have) reinterpret_cast<uint32_t*>(a.slab + (uint64_t)ri * a.slab_bytes)[SLAB_W_COLS] = 0u;
      const uint32_t nj = (uint32_t)__popcll(bal), rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      if (round != 0) {                                           // (workgroup-uniform)
        if (lane == 0) s_cnt[wave] = nj;
        __syncthreads();
        if (threadIdx.x == 0) {
          const uint32_t tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
          s_over = tot ? atomicAdd(a.job_count, tot) : 0u;
        }
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; w++) before += s_cnt[w];
        seed.slab = a.rec_capacity + s_over + before + rank;     // (below rec_capacity x slots_per_rec: at most slots_per_rec - 1 later windows per record)
        __syncthreads();                                          // (s_cnt / s_over are rewritten in the next round)
      }
      if (bal == 0ull) continue;                                  // (wave-uniform)
      if (have) s_seed[wave][rank] = seed;
      wave_sync();
      // ---- phase B: four lanes per job write the head of its slab: lane p of the four decodes the target masks of columns 16 p ..
      //      16 p + 15 (a strip has 45-61 columns at d = 5) and writes its share of the header.  Sixteen jobs per pass, the passes unrolled
      //      with ALL their loads issued before the first is used: a wave's round is one trip to memory, not one per pass.  (Eight
      //      lanes per job and a loop of dependent passes took 40-60 us per launch, most of it waiting.)  Strips wider than 64
      //      columns (other limits, explicit targets) get their remaining pieces in a loop behind. ----
      {
        const int p4 = lane & 3;
        constexpr int PASSES = 4;
        uint32_t cwl[PASSES], cwh[PASSES], mwl[PASSES], mwh[PASSES];
#pragma unroll
        for (int it = 0; it < PASSES; it++) {
          const uint32_t q = (uint32_t)(it * 16 + (lane >> 2));
          cwl[it] = cwh[it] = mwl[it] = mwh[it] = 0u;
          if (q < nj) {
            const JobSeed& sd = s_seed[wave][q];
            const int ntb = cols_ntb(sd.cols), d2 = what_dir(sd.what) & 1, x0 = p4 * 16;
            if (x0 < ntb) {
              const int nv = min(16, ntb - x0);
              const uint64_t plo = d2 ? sd.gpos0 - (uint64_t)(x0 + nv - 1) : sd.gpos0 + (uint64_t)x0, phi = plo + (uint64_t)(nv - 1);
              cwl[it] = a.codes[plo >> 4]; cwh[it] = a.codes[phi >> 4]; mwl[it] = a.mask[plo >> 5]; mwh[it] = a.mask[phi >> 5];
            }
          }
        }
#pragma unroll
        for (int it = 0; it < PASSES; it++) {
          const uint32_t q = (uint32_t)(it * 16 + (lane >> 2));
          if (q < nj) {
            const JobSeed sd = s_seed[wave][q];
            const int ntb = cols_ntb(sd.cols), d2 = what_dir(sd.what) & 1, g2 = what_guide(sd.what), x0 = p4 * 16;
            uint8_t* slab = a.slab + (uint64_t)sd.slab * a.slab_bytes;
            if (x0 < ntb) {
              const int nv = min(16, ntb - x0);
              const uint64_t plo = d2 ? sd.gpos0 - (uint64_t)(x0 + nv - 1) : sd.gpos0 + (uint64_t)x0;
              *reinterpret_cast<uint4*>(slab_tb(slab) + x0) = decode_piece(a.runs, a.n_runs, cwl[it], cwh[it], mwl[it], mwh[it], plo, nv, d2);
            }
            uint4* head = reinterpret_cast<uint4*>(slab);
            if (p4 == 0) { head[SLAB_PIECE_WINDOW] = slab_piece_window(sd.contig, sd.window_k, sd.n); head[SLAB_PIECE_SELECT] = slab_piece_select(s_gint[g2][2], sd.sel, sd.jbase); }
            else if (p4 == 1) head[SLAB_PIECE_STRIP] = slab_piece_strip(sd.c0, sd.cols, sd.what);
            else if (p4 == 2) head[SLAB_PIECE_QMASK] = reinterpret_cast<const uint4*>(s_qmask[g2])[0];
            else head[SLAB_PIECE_QMASK + 1] = reinterpret_cast<const uint4*>(s_qmask[g2])[1];
          }
        }
        if (any_wide) {                                           // (wave-uniform) pieces 4 .. 8 of the wide strips: eight jobs per pass, a lane per piece
          for (uint32_t q0 = 0; q0 < nj; q0 += 8u) {
            const uint32_t q = q0 + (uint32_t)(lane >> 3);
            const int x0 = (4 + (lane & 7)) * 16;
            if (q < nj) {
              const JobSeed sd = s_seed[wave][q];
              const int ntb = cols_ntb(sd.cols), d2 = what_dir(sd.what) & 1;
              if (x0 < ntb) {
                const int nv = min(16, ntb - x0);
                const uint64_t plo = d2 ? sd.gpos0 - (uint64_t)(x0 + nv - 1) : sd.gpos0 + (uint64_t)x0, phi = plo + (uint64_t)(nv - 1);
                *reinterpret_cast<uint4*>(slab_tb(a.slab + (uint64_t)sd.slab * a.slab_bytes) + x0) =
                    decode_piece(a.runs, a.n_runs, a.codes[plo >> 4], a.codes[phi >> 4], a.mask[plo >> 5], a.mask[phi >> 5], plo, nv, d2);
              }
            }
          }
        }
      }
      wave_release();
    }
  }
}

// PM: the per-matrix reading of fgbio's enumeration.  A template parameter, not a run-time branch: its LDS
// (s_fin3, the larger item stage) would cost the default reading occupancy.
// A job's inputs are the head of its slab as expand_kernel wrote it: 128 bytes of header + TB_LEN bytes of target masks = 17 x 16
// bytes, lane x of the job's lanes loading piece x -- for the NEXT job while this one is being filled, so the load's latency hides
// behind the fill and the wave never waits on a chain of dependent loads.
constexpr int JOB_HEAD16 = (int)(sizeof(SlabHeader) + TB_LEN) / 16;
static_assert((sizeof(SlabHeader) + TB_LEN) % 16 == 0 && JOB_HEAD16 < 20, "one 16-byte piece of a job's head per lane of the job, and a lane for the second slot's header");

// The jobs of a launch: slab `record` for every scan record (its first window with candidate columns), then the slabs behind them
// (rec_capacity + k: the second windows, numbered by expand_kernel).
struct JobRange {
  uint32_t n_recs, rec_capacity;
  uint64_t n_virtual;
  __device__ __forceinline__ explicit JobRange(const AlignArgs& a) : n_recs(*a.rec_count), rec_capacity(a.rec_capacity) {
    if (n_recs > rec_capacity) n_recs = rec_capacity;
    uint64_t n_over = *a.job_count;
    const uint64_t room = (uint64_t)rec_capacity * (a.slots_per_rec - 1u);
    if (n_over > room) n_over = room;
    n_virtual = (uint64_t)n_recs + n_over;
  }
  __device__ __forceinline__ uint64_t slab_of(uint64_t v) const { return v < n_recs ? v : (uint64_t)rec_capacity + (v - n_recs); }
};

// Passing candidates are staged per wave and appended to a.items with one global atomic per flush: trace_kernel then runs one lane
// per *passing* candidate instead of one per candidate slot (4 % of the slots pass at d = 5).  All lanes of the wave that are still
// in the job loop call this together.
__device__ __forceinline__ void flush_items(const AlignArgs& a, const uint64_t* s_items, uint32_t* s_nitems, uint32_t threshold) {
  const int wlane = threadIdx.x & 63;
  wave_sync();
  const uint32_t n = *s_nitems;
  if (n >= threshold && n != 0) {
    const unsigned long long act = __ballot(1);
    const int leader = __ffsll((long long)act) - 1;
    uint32_t base = 0;
    if (wlane == leader) base = atomicAdd(a.item_count, n);
    base = __shfl(base, leader);
    const int rank = __popcll(act & ((1ull << wlane) - 1ull)), nact = __popcll(act);
    for (uint32_t i = (uint32_t)rank; i < n; i += (uint32_t)nact)
      if (base + i < a.item_capacity) a.items[base + i] = s_items[i];
    wave_release();
    if (wlane == leader) *s_nitems = 0;
    wave_sync();
  }
}

// Lane r of a job stages piece r of the job's head, loaded a job ahead, in LDS: the header as it is, the target masks as "the bases
// this column matches".
__device__ __forceinline__ void stage_head(const uint4& pf, uint8_t* s_hd_row, uint8_t* s_tbm_row, int r) {
  constexpr int HEADER16 = (int)(sizeof(SlabHeader) / 16);
  if (r < HEADER16) reinterpret_cast<uint4*>(s_hd_row)[r] = pf;
  else if (r < JOB_HEAD16) {
    // tb byte: bits 0-3 IUPAC set, bit 4 forced mismatch (N) -> tbm byte: the set, or nothing when forced
    auto conv = [](uint32_t t) { const uint32_t f = (t >> 4) & 0x01010101u; return t & 0x0F0F0F0Fu & ~(f * 0xFFu); };
    reinterpret_cast<uint4*>(s_tbm_row)[r - HEADER16] = make_uint4(conv(pf.x), conv(pf.y), conv(pf.z), conv(pf.w));
  }
}

// The candidate column lane r looks at: the r-th selected bit of `sel` in ascending strand-space column order (-1: there is none).
__device__ __forceinline__ int candidate_bit(uint32_t sel, int dir, int r) {
  const int sfirst = __ffs(sel) - 1, slast = 31 - __clz(sel);
  int myb = -1, cnt = 0;
  if (dir == 0) { for (int b = sfirst; b <= slast; b++) if ((sel >> b) & 1u) { if (cnt == r) myb = b; cnt++; } }
  else          { for (int b = slast; b >= sfirst; b--) if ((sel >> b) & 1u) { if (cnt == r) myb = b; cnt++; } }
  return myb;
}

// Hands a filled strip over to trace_kernel, for the lanes of a job some of whose candidate columns passed (`mine`: their bits): which
// ones, their end columns j[], an item per passing matrix of this lane's column (bit k of item_mask: item[k] goes), and the strip's
// trace rows copied from LDS into the slab behind its target masks, `stride` bytes per row.
template <int N>
__device__ __forceinline__ void hand_over(bool pass, uint32_t mine, uint8_t* slab, int r, int j, int stride, int ntb, int L, const uint8_t (*tr)[TR_STRIDE],
                                          const uint64_t (&item)[N], uint32_t item_mask, uint64_t* s_items, uint32_t* s_nitems, int stage) {
  SlabHeader* hd = reinterpret_cast<SlabHeader*>(slab);
  if (r == 0) hd->pass_mask = mine;
  if (pass) {
    hd->j[r] = (uint16_t)j;
#pragma unroll
    for (int k = 0; k < N; k++) if ((item_mask >> k) & 1u) {
      const uint32_t slot = atomicAdd(s_nitems, 1u);
      if (slot < (uint32_t)stage) s_items[slot] = item[k];
    }
  }
  if (r < L) {
    uint32_t* drow = reinterpret_cast<uint32_t*>(slab_trace(slab, ntb) + (uint32_t)(r * stride));
    const uint32_t* srow = reinterpret_cast<const uint32_t*>(&tr[r][0]);
    for (int x = 0; x < stride / 4; x++) drow[x] = srow[x];
  }
}

template <bool PM, int LPJ>
__global__ __launch_bounds__(64) void align_kernel(AlignArgs a) {
  CALITAS_TAIL_PRIO();
  static_assert(LPJ == 32 || LPJ == 21, "two or three jobs per wave");
  constexpr int JOBS = 64 / LPJ;            // jobs per wave (= per workgroup)
  constexpr int ROWS = LPJ == 32 ? MAX_L : LPJ - 1;   // rows a job can have
  constexpr int STAGE = ITEM_STAGE<PM, LPJ>;
  // trace rows are 100 bytes apart: lane r writes byte 99r + t at step t, which spreads the lanes of a job over the banks
  __shared__ __attribute__((aligned(16))) uint8_t s_tr[JOBS][ROWS][TR_STRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t s_hd[JOBS][sizeof(SlabHeader)];   // the job's header as it came
  __shared__ __attribute__((aligned(16))) uint8_t s_tbm[JOBS][TB_LEN];              // the bases a column matches (none for an N)
  __shared__ int s_fin[JOBS][STRIP_MAX_COLS + 1];
  __shared__ int s_fin3[PM ? JOBS : 1][3][PM ? STRIP_MAX_COLS + 1 : 1];   // per-matrix enumeration only: Diag / Left / Up of the bottom row
  __shared__ uint64_t s_items[STAGE];       // (flush_items)
  __shared__ uint32_t s_nitems;
  const int job = LPJ == 32 ? (int)(threadIdx.x >> 5) : (int)(threadIdx.x >= 21) + (int)(threadIdx.x >= 42) + (int)(threadIdx.x >= 63);
  const int r = (int)threadIdx.x - job * LPJ;   // lane within the job = query row r+1
  if ((threadIdx.x & 63) == 0) s_nitems = 0;
  __syncthreads();
  uint8_t (*tr)[TR_STRIDE] = s_tr[job < JOBS ? job : 0];
  uint8_t* tbm = s_tbm[job < JOBS ? job : 0];
  const SlabHead hd{reinterpret_cast<const uint32_t*>(s_hd[job < JOBS ? job : 0])};
  int* fin = s_fin[job < JOBS ? job : 0];
  int (*fin3)[PM ? STRIP_MAX_COLS + 1 : 1] = s_fin3[PM ? (job < JOBS ? job : 0) : 0];

  const JobRange jobs(a);
  const SearchDev& sp = a.sp;
  const uint32_t total_jobs = gridDim.x * JOBS;
  // (lane 63 of a three-job wave belongs to no job)
  uint64_t vi = job < JOBS ? (uint64_t)blockIdx.x * JOBS + (uint64_t)job : jobs.n_virtual;
  uint4 pf = make_uint4(0u, 0u, 0u, 0u);                       // piece r of the head of the job's slab, loaded a job ahead
  if (vi < jobs.n_virtual && r < JOB_HEAD16) pf = reinterpret_cast<const uint4*>(a.slab + jobs.slab_of(vi) * a.slab_bytes)[r];
  for (; vi < jobs.n_virtual; vi += total_jobs) {
    flush_items(a, s_items, &s_nitems, STAGE_FLUSH);           // a job adds at most 16 candidates (x 3 per-matrix) per job of the wave
    stage_head(pf, s_hd[job], tbm, r);
    if (vi + total_jobs < jobs.n_virtual && r < JOB_HEAD16) pf = reinterpret_cast<const uint4*>(a.slab + jobs.slab_of(vi + total_jobs) * a.slab_bytes)[r];
    wave_sync();
    if (hd.ncols() == 0) continue;                             // (a record whose columns lie in no window of this call: no job in its slab)
    const uint64_t ji = jobs.slab_of(vi);                      // the job's slab
    const int c0 = hd.c0(), ncols = hd.ncols(), ntb = hd.ntb(), dir = hd.dir(), L = hd.L();
    const int g_min_score = hd.min_score(), jb = hd.jbase();
    const uint32_t sel = hd.sel();
    const bool true_border = hd.true_border();
    const int qm = (r < L) ? hd.qmask(r) : 0;

    // ---- fill: antidiagonal wavefront, lane r = row r+1 ----
    // A cell of a matrix is kept as score * 4 + the matrix's code (TR_DIAG 2 > TR_LEFT 1 > TR_UP 0): the max of two cells breaks
    // ties the way fgbio does (Diag over Left over Up) and the code bits of the winner say which one it was -- one max where
    // there was a max, a compare and a select.
    const int i_row = r + 1;
    const int tgap4 = sp.target_gap * 4, qgap4 = sp.query_gap * 4;
    const int match_t = sp.match * 4 + TR_DIAG, mismatch_t = sp.mismatch * 4 + TR_DIAG;
    int curD = NEG * 4 + TR_DIAG, curL = NEG * 4 + TR_LEFT, curU = (true_border ? i_row * sp.target_gap : NEG) * 4 + TR_UP;
    // "Row 0" (score 0 in all three matrices, ties -> Diag) is what row 1 finds above it: lane 0 gets it as the `old` operand of the
    // lane shift; the first lane of a later job reads the last lane of the job before it, which is no row of that job when its guide
    // is shorter than LPJ and then simply holds row 0 -- always so with three jobs per wave (the host picks LPJ = 21 for guides of
    // up to 20 rows only).  Each job decides for its own last lane: with two jobs of different L (guides of several lengths in one
    // launch) lane 63 can be row 32 of the second job while lane 31 holds row 0 for it.  Lane 32 is patched in the loop unless lane
    // 31 is known to hold row 0 -- also when the first job of the wave has nothing to do this round: its lanes are off and their
    // registers (L among them) hold whatever an earlier round left, so nothing may be read from them.
    if (r == LPJ - 1 && r >= L) { curD = TR_DIAG; curL = NEG * 4 + TR_LEFT; curU = TR_UP; }
    const bool row0_in_lane31 = LPJ != 32 || ((__ballot(r == LPJ - 1 && r >= L) >> 31) & 1ull) != 0ull;
    int curP = max(max(curD, curL), curU);
    const int t_first = r + 1, t_last = r < L ? r + ncols : -1;     // the steps at which this row has a column of the strip
    const int nsteps = ncols + L - 1;
    // what the lane above holds: refreshed by a lane shift per step.  Lane 0 has no lane above and keeps what is there -- row 0,
    // put there once; so does a lane whose upper neighbour is switched off (lane 32 when the first job has nothing to do).
    int inD = TR_DIAG, inU = TR_UP, inPa = TR_DIAG, inPb = TR_DIAG;
    int add_match = match_t, add_mismatch = mismatch_t;
    asm volatile("" : "+v"(add_match), "+v"(add_mismatch));        // in vector registers once, not re-materialised per step
    auto shift_in = [](int& dst, int src) { dst = __builtin_amdgcn_update_dpp(dst, src, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); };
    // The column masks travel down the lanes with the wavefront: row r is at column t - r in step t, where row r - 1 was a step
    // earlier, so a row takes its mask from the lane above with the same lane shift that brings it the cells.  Round 5: before, every
    // lane read its column's mask from LDS, "two steps ahead" -- but LDS operations complete in order and s_waitcnt counts them in
    // order, so waiting for this step's mask also waited for the previous step's trace byte to land: an LDS round trip per step,
    // ~460 cycles per step at two waves per SIMD (profiles/r05_pmc_tail_before.txt: the waves parked 51 % of their time).  Now only
    // row 1 of each job reads masks, four at a time (one ds_read_b32 per four steps, issued a round ahead); nothing in a step waits.
    const uint32_t* tbm32 = reinterpret_cast<const uint32_t*>(tbm);
    const bool row1 = r == 0, bottom = r == L - 1;
    uint8_t* const trow = &tr[r < ROWS ? r : ROWS - 1][0];  // (a lane that is no row writes to column 0 of the last row)
    int m = 0;
    uint32_t w_cur = tbm32[0];
    asm volatile("" : "+v"(w_cur));                         // arrived before the loop: otherwise the loop's header waits for "all but the newest" every round
    auto cell = [&](const int t, const int jj, int inPp, auto patch_lane32) {
      shift_in(inD, curD);
      shift_in(inU, curU);
      if (decltype(patch_lane32)::value && threadIdx.x == 32) { inPp = TR_DIAG; inD = TR_DIAG; inU = TR_UP; }
      const int own = (int)((w_cur >> (8 * jj)) & 0xFFu);   // tbm[t - 1]: the column row 1 is at
      m = __builtin_amdgcn_update_dpp(own, m, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
      if (row1) m = own;
      // The two LDS stores of a step stand OUTSIDE the branch, for every lane, every step: a lane that has no column of the strip in
      // this step writes to column 0 of its own trace row and to fin[0], which nothing reads.  With the stores inside the branch the
      // compiler cannot count the LDS operations between the read of the next round's masks and its use, assumes none, and waits for
      // the newest of them (s_waitcnt lgkmcnt(1)): an LDS round trip per round.
      const bool on = t >= t_first && t <= t_last;
      int c = 0, tbyte = 0;
      if (on) {
        c = t - r;                                          // strip column 1..ncols
        const int add_t = (qm & m) ? add_match : add_mismatch;
        const int newD = (inPp & ~3) + add_t;
        const int newU = max(inD, inU) + tgap4;             // code bits: TR_DIAG = from Diag, TR_UP = from Up
        const int newL = max(curD, curL) + qgap4;           // code bits: TR_DIAG = from Diag, TR_LEFT = from Left
        // trace byte: bits 0-1 where Diag came from, bit 2 Up came from Diag (else Up), bit 3 Left came from Left (else Diag)
        tbyte = (((newL & 1) << 3) | (inPp & 3)) | ((newU & 2) << 1);
        curD = newD; curU = newU & ~3; curL = (newL & ~3) | TR_LEFT;
        curP = max(max(curD, curL), curU);
      }
      trow[c] = (uint8_t)tbyte;
      const int fc = bottom ? c : 0;
      fin[fc] = curP;
      if (PM) { fin3[0][fc] = curD >> 2; fin3[1][fc] = curL >> 2; fin3[2][fc] = curU >> 2; }
    };
    auto fill = [&](auto patch_lane32) {
      shift_in(inPa, curP);
      // four steps per round (steps past the last one find no row on the strip): the shifted curP of one step is the "previous" of
      // the step after the next, hence the two registers taking turns
      for (int t = 1; t <= nsteps; t += 4) {
        const uint32_t w_next = tbm32[(t + 3) >> 2];       // the masks of the next round's columns
        shift_in(inPb, curP);
        cell(t, 0, inPa, patch_lane32);
        shift_in(inPa, curP);
        cell(t + 1, 1, inPb, patch_lane32);
        shift_in(inPb, curP);
        cell(t + 2, 2, inPa, patch_lane32);
        shift_in(inPa, curP);
        cell(t + 3, 3, inPb, patch_lane32);
        w_cur = w_next;
      }
    };
    if (LPJ != 32 || row0_in_lane31) fill(std::false_type{}); else fill(std::true_type{});
    wave_sync();

    // ---- hand the strip over to trace_kernel: one item per passing end column (per passing matrix of it with PM) ----
    const int myb = candidate_bit(sel, dir, r);
    int j = 0, P = 0;
    int pm_score[3] = {0, 0, 0};
    uint32_t pm_pass = 0;                                            // per-matrix enumeration: bit k = matrix k (Diag, Left, Up) passes
    bool pass = false;
    if (myb >= 0) {
      j = dir ? jb - myb : jb + myb;                                 // strand-space end column
      P = fin[j - c0];
      if (PM) {                                                      // every bottom-row cell >= minScore is an alignment of its own
#pragma unroll
        for (int k3 = 0; k3 < 3; k3++) { pm_score[k3] = fin3[k3][j - c0]; if (pm_score[k3] >= g_min_score) pm_pass |= 1u << k3; }
        pass = pm_pass != 0;
      } else {
        pass = (P >> 2) >= g_min_score;                              // best of the three matrices >= minScore
      }
    }
    const unsigned long long bal = __ballot(pass);
    const uint32_t mine = (uint32_t)(bal >> (job * LPJ)) & 0xFFFFu;  // this job's lanes (only lanes 0..15 can pass)
    if (mine != 0u) {
      uint64_t item[PM ? 3 : 1] = {item_pack(ji, r, PM ? TR_DIAG : P & 3, PM ? pm_score[0] : P >> 2)};
      if constexpr (PM) { item[1] = item_pack(ji, r, TR_LEFT, pm_score[1]); item[2] = item_pack(ji, r, TR_UP, pm_score[2]); }   // fgbio's order of directions
      hand_over(pass, mine, a.slab + ji * a.slab_bytes, r, j, slab_stride(ncols), ntb, L, tr, item, PM ? pm_pass : 1u, s_items, &s_nitems, STAGE);
    }
    wave_release();
  }
  flush_items(a, s_items, &s_nitems, 1);
}

// ------------------------------------------------------------------------------------------------------------------
// align_pk_kernel: align_kernel with TWO jobs in every lane group, one in each 16-bit half of the lanes' registers.
//
// Round 5.  Alone on the chip align_kernel's waves execute vector instructions 59 % of their time at two waves per SIMD
// (profiles/r05_pmc_align_alone_*.txt): with the prologue's dependent loads and the per-step LDS waits gone, what is left is its
// instruction count -- ~30 vector instructions per antidiagonal step, 7.8e7 per hg38-sized pass.  A cell is score x 4 + matrix code;
// with the reference's costs |score| <= 60 x 20, so a cell fits sixteen bits with room to spare, and v_pk_add_i16 / v_pk_max_i16 /
// v_pk_mad_i16 do two cells per instruction: the same ~31 instructions per step now fill the strips of SIX jobs per wave (three lane
// groups of 21 x two halves).  "Minus infinity" is the bottom of the range and the additions saturate (clamp), so a cell that is
// out of range stays below every cell a passing alignment can go through (those lie within +-4 x max|cost| x L of zero, which the
// host checks fits: AlignArgs::pack16); their code bits are lost, which no traceback can see.  The trace nibbles of the two jobs
// share a byte (low nibble: the even job); each job's slab gets the rows with its header saying which nibble is its own.
// Launched instead of align_kernel<false, 21> when the host says so; anything else (longer guides, per-matrix enumeration, costs out
// of range, explicit targets) takes align_kernel.
// ------------------------------------------------------------------------------------------------------------------
typedef short pk2 __attribute__((ext_vector_type(2)));
typedef unsigned short upk2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int pk_add_sat(int a, int b) { return __builtin_bit_cast(int, __builtin_elementwise_add_sat(__builtin_bit_cast(pk2, a), __builtin_bit_cast(pk2, b))); }
__device__ __forceinline__ int pk_max(int a, int b) { return __builtin_bit_cast(int, __builtin_elementwise_max(__builtin_bit_cast(pk2, a), __builtin_bit_cast(pk2, b))); }
__device__ __forceinline__ int pk_min_u(int a, int b) { return __builtin_bit_cast(int, __builtin_elementwise_min(__builtin_bit_cast(upk2, a), __builtin_bit_cast(upk2, b))); }
__device__ __forceinline__ int pk_mad(int a, int b, int c) { return __builtin_bit_cast(int, (pk2)(__builtin_bit_cast(pk2, a) * __builtin_bit_cast(pk2, b) + __builtin_bit_cast(pk2, c))); }
__device__ __forceinline__ int pk_rep(int x) { return (int)(((uint32_t)x & 0xFFFFu) * 0x00010001u); }
__device__ __forceinline__ int pk_half(int x, int h) { return h ? (x >> 16) : (int)(short)(x & 0xFFFF); }

__global__ __launch_bounds__(64) void align_pk_kernel(AlignArgs a) {
  CALITAS_TAIL_PRIO();
  constexpr int LPJ = 21, GROUPS = 3, JOBS = 6, ROWS = LPJ - 1;
  constexpr int STAGE = STAGE_FLUSH + JOBS * 16;
  constexpr int NEG4 = -32768;                                 // "minus infinity" x 4 in sixteen bits (the additions saturate)
  __shared__ __attribute__((aligned(16))) uint8_t s_tr[GROUPS][ROWS][TR_STRIDE];    // low nibble: the group's even job, high nibble: the odd one
  __shared__ __attribute__((aligned(16))) uint8_t s_hd[JOBS][sizeof(SlabHeader)];
  __shared__ __attribute__((aligned(16))) uint8_t s_tbm[JOBS][TB_LEN];
  __shared__ int s_fin[GROUPS][STRIP_MAX_COLS + 1];             // the bottom row's best of three, both jobs' halves
  __shared__ uint64_t s_items[STAGE];                           // (flush_items)
  __shared__ uint32_t s_nitems;
  const int grp = (int)(threadIdx.x >= 21) + (int)(threadIdx.x >= 42) + (int)(threadIdx.x >= 63);
  const int r = (int)threadIdx.x - grp * LPJ;
  if ((threadIdx.x & 63) == 0) s_nitems = 0;
  __syncthreads();
  const int g = grp < GROUPS ? grp : 0;
  uint8_t (*tr)[TR_STRIDE] = s_tr[g];
  const SlabHead hdA{reinterpret_cast<const uint32_t*>(s_hd[2 * g])}, hdB{reinterpret_cast<const uint32_t*>(s_hd[2 * g + 1])};
  int* fin = s_fin[g];

  const JobRange jobs(a);
  const SearchDev& sp = a.sp;
  const uint32_t total_jobs = gridDim.x * JOBS;
  // the group's pair of jobs: virtual jobs vi (even half) and vi + 1 (odd half)
  uint64_t vi = grp < GROUPS ? ((uint64_t)blockIdx.x * GROUPS + (uint64_t)grp) * 2 : jobs.n_virtual;
  uint4 pfA = make_uint4(0u, 0u, 0u, 0u), pfB = make_uint4(0u, 0u, 0u, 0u);
  auto prefetch = [&](uint64_t v) {
    if (r < JOB_HEAD16) {
      pfA = reinterpret_cast<const uint4*>(a.slab + jobs.slab_of(v) * a.slab_bytes)[r];
      if (v + 1 < jobs.n_virtual) pfB = reinterpret_cast<const uint4*>(a.slab + jobs.slab_of(v + 1) * a.slab_bytes)[r];
      else pfB = make_uint4(0u, 0u, 0u, 0u);                    // (no odd job: a header of zeros says "no job")
    }
  };
  if (vi < jobs.n_virtual) prefetch(vi);
  for (; vi < jobs.n_virtual; vi += total_jobs) {
    flush_items(a, s_items, &s_nitems, STAGE_FLUSH);
    stage_head(pfA, s_hd[2 * g], s_tbm[2 * g], r);
    stage_head(pfB, s_hd[2 * g + 1], s_tbm[2 * g + 1], r);
    if (vi + total_jobs < jobs.n_virtual) prefetch(vi + total_jobs);
    wave_sync();
    const int ncolsA = hdA.ncols(), ncolsB = hdB.ncols();
    if (ncolsA == 0 && ncolsB == 0) continue;                   // (records whose columns lie in no window of this call)
    const int L = ncolsA ? hdA.L() : hdB.L();                   // (one protospacer length per launch: the host checked)
    const int ncols = max(ncolsA, ncolsB);
    const bool tbdA = hdA.true_border(), tbdB = hdB.true_border();
    const int qm = (r < L) ? (hdA.qmask(r) | (hdB.qmask(r) << 16)) : 0;

    // ---- fill: align_kernel's, two cells per register ----
    const int i_row = r + 1;
    const int tgap4 = pk_rep(sp.target_gap * 4), qgap4 = pk_rep(sp.query_gap * 4);
    const int mism_t = pk_rep(sp.mismatch * 4 + TR_DIAG), delta_t = pk_rep((sp.match - sp.mismatch) * 4);
    const int one2 = 0x00010001, keep2 = (int)0xFFFCFFFC;
    int curD = pk_rep(NEG4 + TR_DIAG), curL = pk_rep(NEG4 + TR_LEFT);
    int curU = (int)(((uint32_t)((tbdA ? i_row * sp.target_gap * 4 : NEG4) + TR_UP) & 0xFFFFu) | ((uint32_t)((tbdB ? i_row * sp.target_gap * 4 : NEG4) + TR_UP) << 16));
    if (r == LPJ - 1) { curD = pk_rep(TR_DIAG); curL = pk_rep(NEG4 + TR_LEFT); curU = pk_rep(TR_UP); }   // "row 0" for the group above
    int curP = pk_max(pk_max(curD, curL), curU);
    const int t_first = r + 1, t_last = r < L ? r + ncols : -1;
    const int nsteps = ncols + L - 1;
    int inD = pk_rep(TR_DIAG), inU = pk_rep(TR_UP), inPa = pk_rep(TR_DIAG), inPb = pk_rep(TR_DIAG);
    auto shift_in = [](int& dst, int src) { dst = __builtin_amdgcn_update_dpp(dst, src, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); };
    const uint32_t* tbmA = reinterpret_cast<const uint32_t*>(s_tbm[2 * g]);
    const uint32_t* tbmB = reinterpret_cast<const uint32_t*>(s_tbm[2 * g + 1]);
    const bool row1 = r == 0, bottom = r == L - 1;
    uint8_t* const trow = &tr[r < ROWS ? r : ROWS - 1][0];
    int m = 0;
    uint32_t wA = tbmA[0], wB = tbmB[0];
    asm volatile("" : "+v"(wA), "+v"(wB));
    auto cell = [&](const int t, const int jj, int inPp) {
      shift_in(inD, curD);
      shift_in(inU, curU);
      // the two jobs' masks of the column row 1 is at: byte jj of wA in the low half, of wB in the high half
      const int own = (int)__builtin_amdgcn_perm(wB, wA, 0x0C000C00u | (uint32_t)jj | ((uint32_t)(4 + jj) << 16));
      m = __builtin_amdgcn_update_dpp(own, m, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
      if (row1) m = own;
      const bool on = t >= t_first && t <= t_last;
      int c = 0, tbyte = 0;
      if (on) {
        c = t - r;
        const int hit = pk_min_u(qm & m, one2);             // 1 per half where the row's set meets the column's
        const int add_t = pk_mad(hit, delta_t, mism_t);
        const int newD = pk_add_sat(inPp & keep2, add_t);
        const int newU = pk_add_sat(pk_max(inD, inU), tgap4);
        const int newL = pk_add_sat(pk_max(curD, curL), qgap4);
        // trace nibble per half: bits 0-1 where Diag came from, bit 2 Up came from Diag, bit 3 Left came from Left
        const int tn = (inPp & 0x00030003) | ((newU & 0x00020002) << 1) | ((newL & one2) << 3);
        tbyte = tn | (tn >> 12);                            // low nibble: the even job, high nibble: the odd one
        curD = newD; curU = newU & keep2; curL = (newL & keep2) | one2;
        curP = pk_max(pk_max(curD, curL), curU);
      }
      trow[c] = (uint8_t)tbyte;
      fin[bottom ? c : 0] = curP;
    };
    shift_in(inPa, curP);
    for (int t = 1; t <= nsteps; t += 4) {
      const uint32_t nA = tbmA[(t + 3) >> 2], nB = tbmB[(t + 3) >> 2];
      shift_in(inPb, curP);
      cell(t, 0, inPa);
      shift_in(inPa, curP);
      cell(t + 1, 1, inPb);
      shift_in(inPb, curP);
      cell(t + 2, 2, inPa);
      shift_in(inPa, curP);
      cell(t + 3, 3, inPb);
      wA = nA; wB = nB;
    }
    wave_sync();

    // ---- hand over, one job after the other ----
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const SlabHead hd = h ? hdB : hdA;
      const int c0 = hd.c0(), ntb = hd.ntb(), dir = hd.dir(), g_min_score = hd.min_score();
      const uint32_t sel = (h ? ncolsB : ncolsA) ? hd.sel() : 0u;
      const int jb = hd.jbase();
      const int myb = candidate_bit(sel, dir, r);
      int j = 0, P = 0;
      bool pass = false;
      if (myb >= 0) {
        j = dir ? jb - myb : jb + myb;
        P = pk_half(fin[j - c0], h);
        pass = (P >> 2) >= g_min_score;
      }
      const unsigned long long bal = __ballot(pass);
      const uint32_t mine = (uint32_t)(bal >> (grp * LPJ)) & 0xFFFFu;
      if (mine != 0u) {
        const uint64_t ji = jobs.slab_of(vi + (uint64_t)h);
        uint8_t* slab = a.slab + ji * a.slab_bytes;
        const int stride = slab_stride(ncols);                  // the PAIR's row length: both jobs' rows are the group's rows
        if (r == 0) { SlabHeader* sh = reinterpret_cast<SlabHeader*>(slab); sh->stride = (uint16_t)stride; sh->pad = (uint16_t)h; }   // (pad: the job's nibble)
        const uint64_t item[1] = {item_pack(ji, r, P & 3, P >> 2)};
        hand_over(pass, mine, slab, r, j, stride, ntb, L, tr, item, 1u, s_items, &s_nitems, STAGE);
      }
    }
    wave_release();
  }
  flush_items(a, s_items, &s_nitems, 1);
}

// Self-test of the cross-lane primitive the fill relies on: out[i] = value held by lane i-1.
__global__ void dpp_selftest_kernel(int* out) {
  int v = (int)threadIdx.x * 7 + 3;
  out[threadIdx.x] = shift_up_lane(v);
}

hipError_t launch_align(const AlignArgs& a, uint32_t n_blocks, hipStream_t stream) {
  // n_blocks counts 256-lane units (8 jobs)
  const dim3 grid(n_blocks * 4), block(64);                  // one wave per workgroup
  // scan records -> jobs: a lane per record, 256-lane workgroups striding over the records (their number is on the device)
  const uint32_t expand_blocks = std::max<uint32_t>(1u, std::min<uint32_t>(1024u, (a.rec_capacity + 255u) / 256u));
  hipLaunchKernelGGL(expand_kernel, dim3(expand_blocks), dim3(256), 0, stream, a);
  // three jobs per wave when no guide has more than 20 rows (max_guide_len 0: unknown)
  bool three = a.max_guide_len > 0 && a.max_guide_len <= 20;
  if (const char* env = TUNE_GET("CALITAS_ALIGN_LPJ")) three = three && std::atoi(env) == 21;   // (tests / measurements: 32 forces two jobs)
  bool pack = three && !a.sp.per_matrix && a.pack16 != 0;
  if (const char* env = TUNE_GET("CALITAS_ALIGN_PACK")) pack = pack && std::atoi(env) != 0;    // (tests / measurements: 0 = one job per lane group)
  if (pack) { hipLaunchKernelGGL(align_pk_kernel, grid, block, 0, stream, a); return hipGetLastError(); }
  if (a.sp.per_matrix) {
    if (three) hipLaunchKernelGGL((align_kernel<true, 21>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((align_kernel<true, 32>), grid, block, 0, stream, a);
  } else {
    if (three) hipLaunchKernelGGL((align_kernel<false, 21>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((align_kernel<false, 32>), grid, block, 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_dpp_selftest(int* out, hipStream_t stream) {
  hipLaunchKernelGGL(dpp_selftest_kernel, dim3(1), dim3(64), 0, stream, out);
  return hipGetLastError();
}

}  // namespace calitas
