// trace.hip -- trace_kernel: one lane per passing candidate end column walks the trace matrix that the aligner left in the job's
// slab (slab.hpp), writes the '='/'X' ops and extends to the PAM; one RawAln per (candidate, PAM).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "common.hpp"
#include "slab.hpp"
#include "kernels.hpp"
#include "mailbox.hpp"

namespace calitas {

constexpr int TRACE_STAGE = 384;                     // RawAln records staged in LDS per trace_kernel workgroup

// Traceback + PAM extension of one candidate end column (the item word: slab.hpp).
template <typename Emit>
__device__ __forceinline__ void trace_one(const AlignArgs& a, const SearchDev& sp, uint64_t it, const uint8_t (*s_qmask)[MAX_L],
                                          const uint8_t (*s_pam)[MAX_PAMS][MAX_PAM_LEN], const uint8_t (*s_pamlen)[MAX_PAMS],
                                          const int (*s_gint)[4], uint32_t* s_ncand, Emit& emit) {
  {
    const int x = item_slot(it);
    const uint8_t* slab = a.slab + item_slab(it) * a.slab_bytes;
    const SlabHeader* hd = reinterpret_cast<const SlabHeader*>(slab);
    if (!((hd->pass_mask >> x) & 1u)) return;
    const uint8_t* tb = slab_tb(slab);
    const uint8_t* tr = slab_trace(slab, hd->ntb);
    const int L = hd->L, c0 = hd->c0, n = hd->n, gi = hd->guide, stride = hd->stride, nib4 = hd->pad ? 4 : 0;
    const bool true_border = hd->true_border != 0;
    const int j = hd->j[x], gscore = item_score(it);   // score and start matrix travel in the item
    const int g_npams = s_gint[gi][0], g_maxd = s_gint[gi][1], g_maxp = s_gint[gi][2], g_maxf = s_gint[gi][3];
    atomicAdd(s_ncand, 1u);

    int m = item_matrix(it), i = L, c = j - c0;
    const int m_start = m;
    uint32_t ops[RAW_MAX_OPS / 16] = {0, 0, 0, 0, 0};
    int nops = 0, diffs = 0;
    bool ok = true;
    while (i > 0) {
      if (nops >= RAW_MAX_OPS) { ok = false; break; }
      int op;
      if (c == 0) {
        // true left border: only the Up matrix is finite there (leading insertions)
        if (!true_border || m != TR_UP) { ok = false; break; }
        op = 2; i--;                                   // 'I'; Up(i,0) traces to Up, Up(1,0) to Diag(0,0)
      } else {
        const int t8 = (tr[(i - 1) * stride + c] >> nib4) & 15;   // (align_pk_kernel: two jobs' trace nibbles share a byte)
        if (m == TR_DIAG) {
          const int tm = tb[c - 1], q = s_qmask[gi][i - 1];
          const bool compat = (q & tm & 15) != 0;
          const bool eq = sp.eqx_by_score ? (compat && !(tm & 16)) : compat;
          op = eq ? 0 : 1;
          m = t8 & 3; i--; c--;
        } else if (m == TR_UP) {
          op = 2; m = ((t8 >> 2) & 1) ? TR_DIAG : TR_UP; i--;       // bit 2: Up came from Diag
        } else {
          op = 3; m = ((t8 >> 3) & 1) ? TR_LEFT : TR_DIAG; c--;
        }
      }
      if (op != 0) diffs++;
      ops[nops >> 4] |= (uint32_t)op << ((nops & 15) * 2);
      nops++;
    }
    if (!ok) { atomicAdd(a.anomalies, 1u); return; }
    if (diffs > g_maxd) return;
    RawAln o;
    o.contig = hd->contig; o.window_k = hd->window_k; o.t_start = (uint16_t)(c0 + c + 1); o.t_end_guide = (uint16_t)j;
    o.dir = hd->dir; o.guide = hd->guide; o.n_ops = (uint8_t)nops;
    o.pad = sp.per_matrix ? (uint8_t)(m_start == TR_DIAG ? 0 : m_start == TR_LEFT ? 1 : 2) : (uint8_t)0;
    uint32_t* ow = reinterpret_cast<uint32_t*>(o.ops);
#pragma unroll
    for (int w = 0; w < RAW_MAX_OPS / 16; w++) ow[w] = ops[w];
    if (g_npams == 0) {
      o.score = gscore; o.pam = -1; o.offset = 0; o.pam_x = 0;
      emit(o);
      return;
    }
    // terminal indel run = first ops of the traceback
    int term = 0;
    {
      const int op0 = ops[0] & 3;
      if (op0 >= 2) { term = 1; while (term < nops && (int)((ops[term >> 4] >> ((term & 15) * 2)) & 3) == op0) term++; }
    }
    int max_extra = sp.max_gaps - term;
    if (g_maxf - diffs < max_extra) max_extra = g_maxf - diffs;
    for (int pi = 0; pi < g_npams; pi++) {
      const int plen = s_pamlen[gi][pi];
      bool have = false; int best_score = 0, best_off = 0; uint32_t best_x = 0;
      for (int off = 0; off <= max_extra; off++) {
        const int toff = j + off;                   // 0-based strand-space offset of the first PAM base
        int limit = g_maxp;
        if (g_maxf - diffs - off < limit) limit = g_maxf - diffs - off;
        if (toff + plen > n || limit < 0) continue;
        int sc = 0, nx = 0; uint32_t xm = 0;
        for (int q = 0; q < plen; q++) {
          const int tm = tb[toff + q - c0];
          const bool match = ((s_pam[gi][pi][q] & tm & 15) != 0) && !(tm & 16);
          const int addend = match ? sp.pam_match : sp.pam_mismatch;
          sc += addend;
          if (!(addend > 0)) { nx++; xm |= 1u << q; }
        }
        if (nx > limit) continue;
        const int total = gscore + sc + off * sp.query_gap;
        if (!have || total > best_score) { have = true; best_score = total; best_off = off; best_x = xm; }
      }
      if (have) {
        o.score = best_score; o.pam = (int8_t)pi; o.offset = (uint8_t)best_off; o.pam_x = (uint16_t)best_x;
        emit(o);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// trace_kernel: one lane per passing candidate end column -- traceback through the strip's trace matrix (slab in HBM),
// '='/'X' ops, extendAndFilterRight (SequentialGuideAligner.scala:433-492), one RawAln per (candidate, PAM).
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trace_kernel(AlignArgs a, uint32_t* box, uint32_t seq) {
  CALITAS_TAIL_PRIO();
  __shared__ uint8_t s_qmask[MAX_GUIDES][MAX_L];
  __shared__ uint8_t s_pam[MAX_GUIDES][MAX_PAMS][MAX_PAM_LEN];
  __shared__ uint8_t s_pamlen[MAX_GUIDES][MAX_PAMS];
  __shared__ int s_gint[MAX_GUIDES][4];     // n_pams, max_guide_diffs, max_pam_mismatches, max_diffs_filtering
  for (int i = threadIdx.x; i < a.sp.n_guides * MAX_L; i += blockDim.x) s_qmask[i / MAX_L][i % MAX_L] = a.guides[i / MAX_L].qmask[i % MAX_L];
  for (int i = threadIdx.x; i < a.sp.n_guides * MAX_PAMS * MAX_PAM_LEN; i += blockDim.x) {
    const int gi = i / (MAX_PAMS * MAX_PAM_LEN), rem = i % (MAX_PAMS * MAX_PAM_LEN);
    s_pam[gi][rem / MAX_PAM_LEN][rem % MAX_PAM_LEN] = a.guides[gi].pam_mask[rem / MAX_PAM_LEN][rem % MAX_PAM_LEN];
  }
  for (int i = threadIdx.x; i < a.sp.n_guides * MAX_PAMS; i += blockDim.x) s_pamlen[i / MAX_PAMS][i % MAX_PAMS] = a.guides[i / MAX_PAMS].pam_len[i % MAX_PAMS];
  for (int i = threadIdx.x; i < a.sp.n_guides; i += blockDim.x) {
    s_gint[i][0] = a.guides[i].n_pams; s_gint[i][1] = a.guides[i].max_guide_diffs;
    s_gint[i][2] = a.guides[i].max_pam_mismatches; s_gint[i][3] = a.guides[i].max_diffs_filtering;
  }
  __syncthreads();

  __shared__ RawAln s_out[TRACE_STAGE];
  __shared__ uint32_t s_nout, s_obase, s_ncand;
  if (threadIdx.x == 0) { s_nout = 0; s_ncand = 0; }
  __syncthreads();

  uint32_t n_items = *a.item_count;                                   // passing candidates appended by align_kernel
  if (n_items > a.item_capacity) n_items = a.item_capacity;
  const SearchDev& sp = a.sp;
  // Results are staged in LDS and flushed with one global atomic per flush (see stage_record in scan_columns.hip for why).
  // ... and where an alignment lands in a.out[] is also listed in the bin its window starts in (binned.hip; returning atomics on
  // distinct words: cheap)
  auto to_bin = [&](uint32_t contig, uint32_t window_k, uint32_t g) {
    const uint32_t bin = a.bin_base[contig] + (uint32_t)(((uint64_t)window_k * (uint64_t)(uint32_t)sp.step) >> a.bin_shift) - a.bin_first;
    if (bin >= a.bin_n) { atomicAdd(a.anomalies, 1u); return; }      // (the host plans the windows from the bins: an internal error, reported)
    const uint32_t at = atomicAdd(a.bin_count + bin, 1u);
    if (at < a.bin_cap) a.bin_idx[(size_t)bin * a.bin_cap + at] = g;
  };
  auto emit = [&](const RawAln& o) {
    const uint32_t slot = atomicAdd(&s_nout, 1u);                     // LDS atomic
    if (slot < (uint32_t)TRACE_STAGE) { s_out[slot] = o; return; }
    const uint32_t g = atomicAdd(a.out_count, 1u);                    // stage full: append directly
    if (g < a.out_capacity) { a.out[g] = o; if (a.bin_idx) to_bin(o.contig, o.window_k, g); }
  };
  auto flush = [&]() {                                                // block-uniform call sites only
    __syncthreads();
    const uint32_t n = min(s_nout, (uint32_t)TRACE_STAGE);
    if (n != 0) {
      if (threadIdx.x == 0) s_obase = atomicAdd(a.out_count, n);
      __syncthreads();
      const uint32_t* src = reinterpret_cast<const uint32_t*>(s_out);
      constexpr uint32_t WPR = sizeof(RawAln) / 4;
      for (uint32_t w = threadIdx.x; w < n * WPR; w += blockDim.x) {
        const uint32_t g = s_obase + w / WPR;
        if (g < a.out_capacity) reinterpret_cast<uint32_t*>(a.out + g)[w % WPR] = src[w];
      }
      if (a.bin_idx)
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x)
          if (s_obase + k < a.out_capacity) to_bin(s_out[k].contig, s_out[k].window_k, s_obase + k);
      __syncthreads();
      if (threadIdx.x == 0) s_nout = 0;
      __syncthreads();
    }
  };

  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n_items; base += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t idx = base + threadIdx.x;
    if (idx < n_items) trace_one(a, sp, a.items[idx], s_qmask, s_pam, s_pamlen, s_gint, &s_ncand, emit);
    __syncthreads();
    const uint32_t staged = s_nout;     // same value in every thread: nobody appends between the two barriers
    __syncthreads();
    if (staged > (uint32_t)(TRACE_STAGE / 2)) flush();
  }
  flush();
  if (threadIdx.x == 0 && s_ncand) atomicAdd(a.cand_count, s_ncand);
  if (box) {
    // the last workgroup to get here posts the call's counters (records, alignments, anomalies, candidates, ...) to the host: no
    // launch of its own for that on the path the host waits on
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      if (atomicAdd(a.trace_done, 1u) == gridDim.x - 1) {
        for (int i = 0; i < 8; i++) box[1 + i] = __hip_atomic_load(a.rec_count + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence_system();
        __hip_atomic_store(box, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

hipError_t launch_trace(const AlignArgs& a, uint32_t n_blocks, hipStream_t stream, hipEvent_t stop, Mailbox* post) {
  uint32_t* box = nullptr;
  uint32_t seq = 0;
  if (post) {
    hipError_t e = mailbox_open(*post);
    if (e != hipSuccess) return e;
    box = post->dev; seq = ++post->seq;
  }
  hipExtLaunchKernelGGL(trace_kernel, dim3(n_blocks), dim3(256), 0, stream, nullptr, stop, 0, a, box, seq);
  return hipGetLastError();
}

}  // namespace calitas
