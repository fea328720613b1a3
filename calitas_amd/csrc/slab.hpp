// slab.hpp -- the one description of an aligner job's slab and of the item word, for the host and for the kernels that hand a
// slab on: expand_kernel -> align_kernel / align_pk_kernel -> trace_kernel (align.hip, trace.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_vector_types.h>

#include "common.hpp"

namespace calitas {

// One aligner job = one scan record x one window that holds some of its candidate columns; one slab per job.  The slab is the job's
// whole life: expand_kernel writes its head (the strip's geometry, the guide's row sets, the target masks tb[ntb]) with one lane
// group per job, align_kernel reads exactly that -- one 16-byte load per lane, issued a job ahead --, fills the strip and adds the
// trace bytes tr[L][stride] and which candidate columns passed, trace_kernel walks it.  Slabs have a fixed size per search and the
// job's number as their address, so the hand-overs need no atomics beyond the one that numbers the jobs.
struct SlabHeader {
  uint32_t pass_mask;     // (align_kernel) bit x: the x-th candidate column of this job reached min_guide_score; 0 from expand_kernel
  uint32_t contig;
  uint32_t window_k;
  int32_t n;              // window length
  int32_t c0;             // strip boundary column (strip columns are c0+1 .. c0+ncols)
  uint16_t ncols, ntb;
  uint8_t dir, guide, true_border, L;
  uint16_t stride, pad;
  uint16_t j[16];         // (align_kernel) strand-space end column (1-based) of candidate x, for the candidates that passed
  // what align_kernel needs besides the geometry above, so that a job is ONE read of its slab's head:
  uint8_t qmask[MAX_L];   // IUPAC set of each query row (GuideDev::qmask of the job's guide)
  int32_t min_score;      // GuideDev::min_guide_score
  uint32_t sel;           // candidate columns of the record's 16-base word that lie inside this window (bit b = base b)
  int32_t jbase;          // strand-space column of bit 0: j = jbase + b (dir 0) or jbase - b (dir 1)
  int32_t reserved[5];
};
static_assert(sizeof(SlabHeader) == 128, "slab header layout");

// A slab: SlabHeader | tb[slab_tb_bytes(ntb)] target masks | tr[L][slab_stride(ncols)] trace bytes (columns 0 .. ncols of a row).
CAL_HD constexpr int slab_stride(int ncols) { return (ncols + 4) & ~3; }
CAL_HD constexpr int slab_tb_bytes(int ntb) { return (ntb + 3) & ~3; }
template <typename Byte> CAL_HD inline Byte* slab_tb(Byte* slab) { return slab + sizeof(SlabHeader); }
template <typename Byte> CAL_HD inline Byte* slab_trace(Byte* slab, int ntb) { return slab_tb(slab) + slab_tb_bytes(ntb); }
// the slab of a guide's widest strip: 16 candidate columns + span + 1, and the PAM look-ahead behind them
inline uint32_t slab_bytes_for(int L, int span, int max_gaps) {
  const int ncols_max = 16 + span + 1;
  return (uint32_t)((sizeof(SlabHeader) + slab_tb_bytes(ncols_max + max_gaps + MAX_PAM_LEN) + L * slab_stride(ncols_max) + 15) & ~15u);
}

// Trace codes of the three matrices, ordered so that max() of (score * 4 + code) breaks ties Diag > Left > Up.
constexpr int TR_UP = 0, TR_LEFT = 1, TR_DIAG = 2;

// A passing candidate on its way to trace_kernel:
// item = candidate slot | slab index << 4 | start matrix << ITEM_MATRIX_SHIFT | (score + ITEM_SCORE_BIAS) << ITEM_SCORE_SHIFT
constexpr int ITEM_SLOT_BITS = 4, ITEM_SLAB_BITS = 36, ITEM_MATRIX_SHIFT = ITEM_SLOT_BITS + ITEM_SLAB_BITS, ITEM_SCORE_SHIFT = ITEM_MATRIX_SHIFT + 2, ITEM_SCORE_BIAS = 1 << 21;
constexpr uint64_t ITEM_SLAB_MASK = (1ull << ITEM_SLAB_BITS) - 1ull;
static_assert((1 << ITEM_SLOT_BITS) == sizeof(SlabHeader::j) / sizeof(uint16_t) && ITEM_MATRIX_SHIFT == 40 && ITEM_SCORE_SHIFT + 22 == 64, "item word layout");
CAL_HD inline uint64_t item_pack(uint64_t slab, int slot, int matrix, int score) {
  return ((slab & ITEM_SLAB_MASK) << ITEM_SLOT_BITS) | (uint64_t)slot | ((uint64_t)matrix << ITEM_MATRIX_SHIFT) |
         ((uint64_t)(uint32_t)(score + ITEM_SCORE_BIAS) << ITEM_SCORE_SHIFT);
}
CAL_HD inline int item_slot(uint64_t it) { return (int)(it & ((1u << ITEM_SLOT_BITS) - 1u)); }
CAL_HD inline uint64_t item_slab(uint64_t it) { return (it >> ITEM_SLOT_BITS) & ITEM_SLAB_MASK; }
CAL_HD inline int item_matrix(uint64_t it) { return (int)((it >> ITEM_MATRIX_SHIFT) & 3u); }
CAL_HD inline int item_score(uint64_t it) { return (int)(uint32_t)(it >> ITEM_SCORE_SHIFT) - ITEM_SCORE_BIAS; }

// ---- the header as 32 words (how the aligners hold it in LDS) and as eight 16-byte pieces (how expand_kernel writes it) ----
constexpr int SLAB_W_C0 = offsetof(SlabHeader, c0) / 4;
constexpr int SLAB_W_COLS = offsetof(SlabHeader, ncols) / 4;        // ncols | ntb << 16
constexpr int SLAB_W_WHAT = offsetof(SlabHeader, dir) / 4;          // dir | guide << 8 | true_border << 16 | L << 24
constexpr int SLAB_W_STRIDE = offsetof(SlabHeader, stride) / 4;     // stride | pad << 16
constexpr int SLAB_W_QMASK = offsetof(SlabHeader, qmask) / 4;
constexpr int SLAB_W_MIN_SCORE = offsetof(SlabHeader, min_score) / 4;
constexpr int SLAB_W_SEL = offsetof(SlabHeader, sel) / 4;
constexpr int SLAB_W_JBASE = offsetof(SlabHeader, jbase) / 4;
static_assert(offsetof(SlabHeader, ncols) == 4 * SLAB_W_COLS && offsetof(SlabHeader, ntb) == 4 * SLAB_W_COLS + 2, "ncols, ntb: the halves of one word");
static_assert(offsetof(SlabHeader, dir) == 4 * SLAB_W_WHAT && offsetof(SlabHeader, guide) == 4 * SLAB_W_WHAT + 1 &&
              offsetof(SlabHeader, true_border) == 4 * SLAB_W_WHAT + 2 && offsetof(SlabHeader, L) == 4 * SLAB_W_WHAT + 3, "dir, guide, true_border, L: the bytes of one word");
static_assert(offsetof(SlabHeader, stride) == 4 * SLAB_W_STRIDE && offsetof(SlabHeader, pad) == 4 * SLAB_W_STRIDE + 2, "stride, pad: the halves of one word");
static_assert(offsetof(SlabHeader, c0) == 4 * SLAB_W_C0 && offsetof(SlabHeader, qmask) == 4 * SLAB_W_QMASK && offsetof(SlabHeader, min_score) == 4 * SLAB_W_MIN_SCORE &&
              offsetof(SlabHeader, sel) == 4 * SLAB_W_SEL && offsetof(SlabHeader, jbase) == 4 * SLAB_W_JBASE, "c0, qmask, min_score, sel, jbase start on words");

CAL_HD constexpr uint32_t slab_cols(int ncols, int ntb) { return (uint32_t)ncols | ((uint32_t)ntb << 16); }
CAL_HD constexpr uint32_t slab_what(int dir, int guide, bool true_border, int L) {
  return (uint32_t)dir | ((uint32_t)guide << 8) | ((true_border ? 1u : 0u) << 16) | ((uint32_t)L << 24);
}
CAL_HD constexpr int cols_ncols(uint32_t cols) { return (int)(cols & 0xFFFFu); }
CAL_HD constexpr int cols_ntb(uint32_t cols) { return (int)(cols >> 16); }
CAL_HD constexpr int what_dir(uint32_t what) { return (int)(what & 0xFFu); }
CAL_HD constexpr int what_guide(uint32_t what) { return (int)((what >> 8) & 0xFFu); }
CAL_HD constexpr bool what_true_border(uint32_t what) { return ((what >> 16) & 0xFFu) != 0u; }
CAL_HD constexpr int what_L(uint32_t what) { return (int)(what >> 24); }

#if defined(__HIPCC__)
struct SlabHead {         // a view over the 32 words of a header staged in LDS
  const uint32_t* w;
  CAL_DEV int c0() const { return (int)w[SLAB_W_C0]; }
  CAL_DEV int ncols() const { return cols_ncols(w[SLAB_W_COLS]); }   // 0: no job in this slab
  CAL_DEV int ntb() const { return cols_ntb(w[SLAB_W_COLS]); }
  CAL_DEV int dir() const { return what_dir(w[SLAB_W_WHAT]); }
  CAL_DEV int L() const { return what_L(w[SLAB_W_WHAT]); }
  CAL_DEV bool true_border() const { return what_true_border(w[SLAB_W_WHAT]); }
  CAL_DEV int min_score() const { return (int)w[SLAB_W_MIN_SCORE]; }
  CAL_DEV uint32_t sel() const { return w[SLAB_W_SEL]; }
  CAL_DEV int jbase() const { return (int)w[SLAB_W_JBASE]; }
  CAL_DEV int qmask(int r) const { return (int)reinterpret_cast<const uint8_t*>(w + SLAB_W_QMASK)[r]; }
};

// The pieces of a header that expand_kernel writes (pieces 2 and 3, j[], belong to the aligner; piece 7 is reserved).
constexpr int SLAB_PIECE_WINDOW = 0, SLAB_PIECE_STRIP = 1, SLAB_PIECE_QMASK = 4, SLAB_PIECE_SELECT = 6;
static_assert(offsetof(SlabHeader, pass_mask) == SLAB_PIECE_WINDOW * 16 && offsetof(SlabHeader, contig) == SLAB_PIECE_WINDOW * 16 + 4 &&
              offsetof(SlabHeader, window_k) == SLAB_PIECE_WINDOW * 16 + 8 && offsetof(SlabHeader, n) == SLAB_PIECE_WINDOW * 16 + 12, "piece: pass_mask, contig, window_k, n");
static_assert(SLAB_W_C0 == SLAB_PIECE_STRIP * 4 && SLAB_W_COLS == SLAB_PIECE_STRIP * 4 + 1 && SLAB_W_WHAT == SLAB_PIECE_STRIP * 4 + 2 &&
              SLAB_W_STRIDE == SLAB_PIECE_STRIP * 4 + 3, "piece: c0, cols, what, stride");
static_assert(offsetof(SlabHeader, qmask) == SLAB_PIECE_QMASK * 16 && sizeof(SlabHeader::qmask) == 2 * 16, "pieces: qmask, two of them");
static_assert(SLAB_W_MIN_SCORE == SLAB_PIECE_SELECT * 4 && SLAB_W_SEL == SLAB_PIECE_SELECT * 4 + 1 && SLAB_W_JBASE == SLAB_PIECE_SELECT * 4 + 2 &&
              offsetof(SlabHeader, reserved) == SLAB_PIECE_SELECT * 16 + 12, "piece: min_score, sel, jbase, reserved[0]");
CAL_DEV uint4 slab_piece_window(uint32_t contig, uint32_t window_k, uint32_t n) { return make_uint4(0u, contig, window_k, n); }
CAL_DEV uint4 slab_piece_strip(uint32_t c0, uint32_t cols, uint32_t what) {
  return make_uint4(c0, cols, what, (uint32_t)slab_stride(cols_ncols(cols)));   // (pad 0; align_pk_kernel sets its nibble there)
}
CAL_DEV uint4 slab_piece_select(int min_score, uint32_t sel, int jbase) { return make_uint4((uint32_t)min_score, sel, (uint32_t)jbase, 0u); }
#endif

}  // namespace calitas
