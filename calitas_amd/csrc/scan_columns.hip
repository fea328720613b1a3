// scan_columns.hip -- the column-wise scan: the test hook's second implementation of the filter.  No search path selects it; it is
// reachable only through calitas_scan_candidates_columnwise, which the tests hold the row-wise scan of scan_rows.hip against.
//
//  scan_kernel   exact filter for "bottom-row glocal score >= minGuideScore" (the enumeration rule of
//                fgbio Aligner.align(query, target, minScore), SequentialGuideAligner.scala:261,278,295,299).
//                With the reference's linear gap costs a bottom-row score >= minGuideScore implies at most E edits
//                (SearchReference.scala:432-441), so the filter is Myers' bit-vector edit distance: one 32-bit
//                column vector per lane, the protospacer rows top-aligned so the row-L delta falls out of the
//                shift as a carry.  Every lane owns CHUNK consecutive bases of a 256-lane tile that the workgroup
//                streams from HBM into LDS with coalesced 16-byte loads; it runs the tile once left-to-right
//                (target as is) and once right-to-left (reverse-complemented target) with 32 warm-up columns.
//                Integer VALU work; no MFMA.  Emits one record per 16-base word that holds a candidate column.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "common.hpp"
#include "kernels.hpp"

namespace calitas {

// ------------------------------------------------------------------------------------------------------------------
// scan_kernel
// ------------------------------------------------------------------------------------------------------------------

// One column of Myers' bit-vector algorithm (search variant: free start in the text, so no carry into row 1).
// Guide rows occupy the top L bits; the padding bits below keep Pv=1, Mv=0 as long as eq has them clear.
// The horizontal deltas of row L sit in bit 31, so the two shifts are written as x+x and their carry-outs update
// the running bottom-row score (v_add_co / v_addc on gfx950).
__device__ __forceinline__ void myers_step(uint32_t eq, uint32_t& pv, uint32_t& mv, int& score, int& smin) {
  // Hand-scheduled: 13 VALU instructions per column (hipcc's own selection of the same expression needs 17).
  // v_min_i32 issues at ~0.6x the rate of v_or_b32 on gfx950 (tools/valu_bench2.hip), hence the sign-bit accumulator.
  //   t  = (eq & pv) + pv
  //   mh = pv & ((t ^ pv) | eq)            bitop3(pv, t, eq)  = 0xb0
  //   xh = (t ^ pv) | eq                   bitop3(t, pv, eq)  = 0xbe
  //   ph = mv | ~(xh | pv)                 bitop3(mv, xh, pv) = 0xf1
  //   xv = eq | mv
  //   ph <<= 1, score += carry;  mh <<= 1, score -= carry
  //   pv = mh | ~(xv | ph)                 bitop3(mh, xv, ph) = 0xf1
  //   mv = ph & xv
  //   sacc |= score          (the caller keeps score biased by -(E+1): the sign bit of sacc = "some column <= E")
  uint32_t t, xh, ph, mh, xv;
  asm("v_and_b32 %5, %9, %0\n\t"
      "v_add_u32 %5, %5, %0\n\t"
      "v_bitop3_b32 %7, %0, %5, %9 bitop3:0xb0\n\t"
      "v_bitop3_b32 %6, %5, %0, %9 bitop3:0xbe\n\t"
      "v_or_b32 %8, %9, %1\n\t"
      "v_bitop3_b32 %4, %1, %6, %0 bitop3:0xf1\n\t"
      "v_add_co_u32 %7, vcc, %7, %7\n\t"
      "v_subb_co_u32 %2, vcc, %2, 0, vcc\n\t"
      "v_add_co_u32 %4, vcc, %4, %4\n\t"
      "v_addc_co_u32 %2, vcc, 0, %2, vcc\n\t"
      "v_bitop3_b32 %0, %7, %8, %4 bitop3:0xf1\n\t"
      "v_and_b32 %1, %4, %8\n\t"
      "v_or_b32 %3, %3, %2"
      : "+v"(pv), "+v"(mv), "+v"(score), "+v"(smin), "=&v"(ph), "=&v"(t), "=&v"(xh), "=&v"(mh), "=&v"(xv)
      : "v"(eq)
      : "vcc");
}

// Two independent columns (pass A and pass B) interleaved instruction by instruction so that dependent VALU
// instructions of one recurrence are never adjacent; pass B carries through an SGPR pair instead of VCC.
__device__ __forceinline__ void myers_step2(uint32_t eqa, uint32_t& pva, uint32_t& mva, int& sca, int& mina,
                                            uint32_t eqb, uint32_t& pvb, uint32_t& mvb, int& scb, int& minb) {
  uint32_t ta, xha, pha, mha, xva, tb, xhb, phb, mhb, xvb;
  unsigned long long cb;
  asm("v_and_b32 %9, %19, %0\n\t"
      "v_and_b32 %14, %20, %4\n\t"
      "v_add_u32 %9, %9, %0\n\t"
      "v_add_u32 %14, %14, %4\n\t"
      "v_bitop3_b32 %11, %0, %9, %19 bitop3:0xb0\n\t"
      "v_bitop3_b32 %16, %4, %14, %20 bitop3:0xb0\n\t"
      "v_bitop3_b32 %10, %9, %0, %19 bitop3:0xbe\n\t"
      "v_bitop3_b32 %15, %14, %4, %20 bitop3:0xbe\n\t"
      "v_or_b32 %12, %19, %1\n\t"
      "v_or_b32 %17, %20, %5\n\t"
      "v_bitop3_b32 %8, %1, %10, %0 bitop3:0xf1\n\t"
      "v_bitop3_b32 %13, %5, %15, %4 bitop3:0xf1\n\t"
      "v_add_co_u32 %11, vcc, %11, %11\n\t"
      "v_add_co_u32 %16, %18, %16, %16\n\t"
      "v_subb_co_u32 %2, vcc, %2, 0, vcc\n\t"
      "v_subb_co_u32 %6, %18, %6, 0, %18\n\t"
      "v_add_co_u32 %8, vcc, %8, %8\n\t"
      "v_add_co_u32 %13, %18, %13, %13\n\t"
      "v_addc_co_u32 %2, vcc, 0, %2, vcc\n\t"
      "v_addc_co_u32 %6, %18, 0, %6, %18\n\t"
      "v_bitop3_b32 %0, %11, %12, %8 bitop3:0xf1\n\t"
      "v_bitop3_b32 %4, %16, %17, %13 bitop3:0xf1\n\t"
      "v_and_b32 %1, %8, %12\n\t"
      "v_and_b32 %5, %13, %17\n\t"
      "v_or_b32 %3, %3, %2\n\t"
      "v_or_b32 %7, %7, %6"
      : "+v"(pva), "+v"(mva), "+v"(sca), "+v"(mina), "+v"(pvb), "+v"(mvb), "+v"(scb), "+v"(minb),
        "=&v"(pha), "=&v"(ta), "=&v"(xha), "=&v"(mha), "=&v"(xva),
        "=&v"(phb), "=&v"(tb), "=&v"(xhb), "=&v"(mhb), "=&v"(xvb), "=&s"(cb)
      : "v"(eqa), "v"(eqb)
      : "vcc");
}

// Pair index of bases 2j and 2j+1 of a code word (+ their exception bits for masked tiles):
// bits 0-1 code of base 2j, bits 2-3 code of base 2j+1, bit 4 / bit 5 their exception bits.
template <bool MASKED>
__device__ __forceinline__ uint32_t pair_index(uint32_t word, uint32_t mbits, int j) {
  uint32_t idx = (word >> (4 * j)) & 15u;
  if (MASKED) idx |= ((mbits >> (2 * j)) & 3u) << 4;
  return idx;
}

// Replays one 16-base word with a per-column threshold test (taken only when the word's minimum score is <= E).
template <bool MASKED, bool FORWARD>
__device__ __noinline__ uint32_t replay_word(const uint2* tab, uint32_t word, uint32_t mbits, uint32_t pv, uint32_t mv, int score) {
  uint32_t hm = 0;   // score is biased by -(E+1): negative = candidate column
  for (int s = 0; s < 16; s++) {
    const int k = FORWARD ? s : 15 - s;
    const uint2 e = tab[pair_index<MASKED>(word, mbits, k >> 1)];
    int unused = 0;
    myers_step((k & 1) ? e.y : e.x, pv, mv, score, unused);
    hm |= (uint32_t)(score < 0) << k;
  }
  return hm;
}

// Records are staged in LDS and flushed once per tile: a returning atomic on ONE global word completes at only
// ~90 per microsecond chip-wide (MI355X_MICROARCH.md, row "dequeue"), which a per-record append would approach.
constexpr int SCAN_STAGE = 192;

__device__ __forceinline__ void stage_record(const ScanArgs& a, ScanRecord* s_recs, uint32_t* s_nrec, uint32_t gword, uint32_t info) {
  ScanRecord r;
  r.gword = gword; r.info = info;
  const uint32_t slot = atomicAdd(s_nrec, 1u);          // LDS atomic
  if (slot < (uint32_t)SCAN_STAGE) { s_recs[slot] = r; return; }
  const uint32_t g = atomicAdd(a.rec_count, 1u);        // stage full (dense tile): append directly
  if (g < a.rec_capacity) a.recs[g] = r;
}

template <int CHUNK, bool MASKED>
__device__ __forceinline__ void scan_tile(const ScanArgs& a, uint32_t tile, uint32_t* s_codes, uint2* s_tab, ScanRecord* s_recs,
                                          uint32_t* s_nrec) {
  constexpr int WPC = CHUNK / 16;           // code words per lane chunk
  constexpr int MPC = CHUNK / 32;           // mask words per lane chunk
  constexpr int CSTR = WPC + 1;             // padded stride: lane l reads word l*CSTR + k -> conflict-free banks
  constexpr int NV = LANES_PER_TILE + 2;    // virtual chunks: left halo, 256 lanes, right halo
  constexpr int TAB = MASKED ? 64 : 16;     // entries of one pair table
  const int tid = threadIdx.x;

  // ---- stream the tile (+ one halo chunk each side) into LDS: 16-byte coalesced loads, padded scatter ----
  const uint64_t w0 = (uint64_t)tile * (LANES_PER_TILE * WPC);  // first code word of the tile
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.codes + (w0 - WPC));
    constexpr int NQ = NV * WPC / 4;
    for (int q = tid; q < NQ; q += LANES_PER_TILE) {
      const uint4 v = src[q];
      const int i = q * 4;
      const int vc = i / WPC, k = i % WPC;  // WPC is a multiple of 4, so the four words stay in one chunk
      uint32_t* d = &s_codes[vc * CSTR + k];
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  }
  const uint32_t* cw = &s_codes[(tid + 1) * CSTR];
  // exception bits are rare (N-run edges, contig ends, IUPAC codes): the few tiles that have them read the 1-bit
  // mask straight from global memory, one word per 32 bases, instead of spending LDS on it
  const uint32_t* gm = a.mask + (w0 / 2 + (uint64_t)tid * MPC);
  const uint32_t gword0 = (uint32_t)(w0 + (uint64_t)tid * WPC);

  for (int gi = 0; gi < a.n_guides; gi++) {
    const GuideDev& g = a.guides[gi];
    __syncthreads();                        // previous guide's table no longer in use / tile data visible
    for (int i = tid; i < 2 * TAB; i += LANES_PER_TILE) {
      const uint32_t* peq = (i >= TAB) ? g.peq_b : g.peq_a;
      const int idx = i & (TAB - 1);
      const int lo = (idx & 3) | ((idx >> 4) & 1) << 2, hi = ((idx >> 2) & 3) | ((idx >> 5) & 1) << 2;
      s_tab[i] = make_uint2(peq[lo], peq[hi]);
    }
    __syncthreads();
    const int L = g.L, E = g.scan_max_edits;
    const int warm = (L + E + 15) >> 4;     // warm-up words (host guarantees warm <= WPC)
    const uint2* tabA = &s_tab[0];
    const uint2* tabB = &s_tab[TAB];

    // Pass A runs left to right over the chunk (target as is); pass B right to left (target complemented = left to
    // right over the reverse complement).  The two recurrences are independent, so they share one loop for ILP.
    // Scores are kept biased by -(E+1): "score <= E" is the sign bit.
    uint32_t pvA = 0xFFFFFFFFu, mvA = 0u, pvB = 0xFFFFFFFFu, mvB = 0u;
    int scA = L - E - 1, scB = L - E - 1;
    const int n_it = WPC + warm;
    for (int it = 0; it < n_it; it++) {
      const int wa = it - warm;             // < 0: tail of the left neighbour's chunk (cw[wa - 1] skips the pad word)
      const int wb = WPC - 1 + warm - it;   // >= WPC: head of the right neighbour's chunk (cw[wb + 1])
      const uint32_t wordA = (wa >= 0) ? cw[wa] : cw[wa - 1];
      const uint32_t wordB = (wb < WPC) ? cw[wb] : cw[wb + 1];
      uint32_t mA = 0, mB = 0;
      if (MASKED) {
        mA = (gm[wa >> 1] >> ((wa & 1) * 16)) & 0xFFFFu;
        mB = (gm[wb >> 1] >> ((wb & 1) * 16)) & 0xFFFFu;
      }
      const uint32_t pvA0 = pvA, mvA0 = mvA, pvB0 = pvB, mvB0 = mvB;
      const int scA0 = scA, scB0 = scB;
      int accA = 0, accB = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint2 ea = tabA[pair_index<MASKED>(wordA, mA, j)];
        const uint2 eb = tabB[pair_index<MASKED>(wordB, mB, 7 - j)];
        myers_step2(ea.x, pvA, mvA, scA, accA, eb.y, pvB, mvB, scB, accB);
        myers_step2(ea.y, pvA, mvA, scA, accA, eb.x, pvB, mvB, scB, accB);
      }
      if (wa >= 0 && accA < 0) {
        const uint32_t hm = replay_word<MASKED, true>(tabA, wordA, mA, pvA0, mvA0, scA0);
        stage_record(a, s_recs, s_nrec, gword0 + (uint32_t)wa, hm | ((uint32_t)gi << 17));
      }
      if (wb < WPC && accB < 0) {
        const uint32_t hm = replay_word<MASKED, false>(tabB, wordB, mB, pvB0, mvB0, scB0);
        stage_record(a, s_recs, s_nrec, gword0 + (uint32_t)wb, hm | (1u << 16) | ((uint32_t)gi << 17));
      }
    }
  }
}

// One workgroup per tile of the packed space.  Dead tiles (nothing but upper-case N / padding, which every window
// trims away) exit at once; tiles with exception bases take the MASKED instantiation (block-uniform branch).
template <int CHUNK>
__global__ __launch_bounds__(LANES_PER_TILE) void scan_kernel(ScanArgs a) {
  __shared__ uint32_t s_codes[(LANES_PER_TILE + 2) * (CHUNK / 16 + 1)];
  __shared__ uint2 s_tab[2 * 64];           // [direction][pair index] -> (Eq of base 2j, Eq of base 2j+1)
  __shared__ ScanRecord s_recs[SCAN_STAGE];
  __shared__ uint32_t s_nrec, s_base;
  const uint32_t tile = blockIdx.x * a.tile_stride + a.tile_offset;
  const TileInfo ti = a.tiles[tile];
  if (ti.flag == 2u || ti.contig == 0xFFFFFFFFu) return;
  if (a.chrom_index >= 0 && ti.contig != (uint32_t)a.chrom_index) return;
  if (threadIdx.x == 0) s_nrec = 0;         // made visible by the first barrier inside scan_tile
  if (ti.flag != 0u) scan_tile<CHUNK, true>(a, tile, s_codes, s_tab, s_recs, &s_nrec);
  else scan_tile<CHUNK, false>(a, tile, s_codes, s_tab, s_recs, &s_nrec);
  // ---- flush the tile's records with one global atomic ----
  __syncthreads();
  const uint32_t n = min(s_nrec, (uint32_t)SCAN_STAGE);
  if (n == 0) return;
  if (threadIdx.x == 0) s_base = atomicAdd(a.rec_count, n);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += LANES_PER_TILE) {
    const uint32_t g = s_base + i;
    if (g < a.rec_capacity) a.recs[g] = s_recs[i];
  }
}

// start / stop (optional): events attached to the dispatch itself -- no marker packets before and after the kernel on the stream.
hipError_t launch_scan(const ScanArgs& a, int chunk, uint32_t n_tiles, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (n_tiles == 0) {
    if (start) { hipError_t e = hipEventRecord(start, stream); if (e != hipSuccess) return e; }
    return stop ? hipEventRecord(stop, stream) : hipSuccess;
  }
  dim3 grid(n_tiles), block(LANES_PER_TILE);
  constexpr unsigned pad = 0;
  switch (chunk) {
    case 64:  hipExtLaunchKernelGGL(scan_kernel<64>, grid, block, pad, stream, start, stop, 0, a); break;
    case 128: hipExtLaunchKernelGGL(scan_kernel<128>, grid, block, pad, stream, start, stop, 0, a); break;
    case 256: hipExtLaunchKernelGGL(scan_kernel<256>, grid, block, pad, stream, start, stop, 0, a); break;
    case 512: hipExtLaunchKernelGGL(scan_kernel<512>, grid, block, pad, stream, start, stop, 0, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace calitas
