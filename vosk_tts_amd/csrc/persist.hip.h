// persist.hip.h — the latency-bound three quarters of a single utterance as PERSISTENT step programs (round 3).
//
// What it replaces: at B = 1 the text encoder, the stochastic duration predictor and the flow are ~120 dependent launches on
// [192..768 x 50..160] tensors that carry 21 % of the forward's FLOPs and take 0.9 of its 1.33 ms: every launch pays the dispatch, a
// cold L2 and its own chain of dependent cold misses, 5.5-13 us each.
//
// How: a stage is a STEP PROGRAM run by ONE kernel of P workgroups (one per CU) that never leave the machine.  Between steps there
// is NO barrier and NO flag: every exchanged tensor is an array of 8-byte "LL cells" {float value, u32 epoch} written with one
// agent-scope 8-byte store and polled by the consumers with agent-scope (L1-bypassing, sc1) 8-byte loads until the epoch matches
// this forward -- the data is its own arrival signal (tools/llprobe.hip: 0.32 us one-way inside an XCD, 0.73 us across XCDs,
// coherent chip-wide with sc1 stores).  A worker that is idle in a step simply moves on; a consumer waits only for the cells it
// reads.  Epochs make stale data harmless: every forward uses epoch = (last completed forward) + 1, cells are never reset, every step
// of a forward writes its OWN buffers (no reuse inside a forward, so there is no write-after-read hazard either), and a cell whose
// epoch does not match is simply not there yet.  Every poll loop is bounded (PS_SPIN_LIMIT): a lost worker turns into an error
// word, never into a hung GPU.
//
// What bounds a step (measured, tools/ps_trace.py): (1) how many bytes ONE workgroup must pull through L1-bypassing loads (~30 GB/s
// per CU), (2) how often an element is recomputed, (3) the INSTRUCTIONS every wave issues for bookkeeping (a wave issues at most one
// instruction per 4 cycles: a generic interpreter that decoded its step descriptors on the device ran 15.6 k cycles per matrix step
// against 6.1 k for hand-specialised code).  So:
//   * the HOST resolves everything: per (step, worker) one 128-byte RECORD holds the final pointers of that worker's work item
//     (operand window, weight fragments of its row blocks, epilogue operands, output tile) and a few packed integers; the kernel
//     keeps the record in 4 VGPRs of lanes 0..7 and reads fields with v_readlane -- no divisions, no clamping, no descriptor
//     decode on the device; records and read-only operands are requested two / one steps ahead in straight-line code;
//   * column steps, one worker per COLUMN t of the column-major cells [T][C], thread = channel: LayerNorm (+ K-slice partial
//     sums, bias, residual, speaker vector), the DDSConv elementwise chain (finish the previous layer at t - d, t, t + d,
//     depthwise conv, LN, GELU), embedding lookup, attention merge, coupling tail.  A LayerNorm is a DPP wave reduction + one LDS
//     exchange; every element is computed once;
//   * fused column steps (PF_MV; the duration predictor up to 64 columns at 256 channels, persist_plan.hip.h persist_sdp_split): the
//     worker that owns a column has all its channels anyway, so the 1x1 conv that consumes the column runs in the same step as a
//     matrix-vector product -- the 8 waves split the contraction, lane = output channel, the transposed weights of the worker's <= 64
//     output channels in registers, partial sums added in wave order through LDS.  Up to four workers share a column: each redoes
//     the cheap column work (nothing of it is exchanged) and owns a quarter of the output channels, so no worker streams more than
//     64 KB of weights.  One step per DDSConv layer instead of two, dp.proj and ConvFlow.proj + the spline of ONE column behind the
//     last finish of a stack: 17 dependent steps instead of 33, 115 -> 77 us at T = 50 (profiles/dp_fused_bench.txt);
//   * the attention half of an encoder layer the same way (PK_MERGE | PF_MV; persist_plan.hip.h persist_attn_form): the worker that
//     merges a column has its H attention channels, so conv_o + the residual run in the merge step on that column -- form A: up to 4
//     workers per column with ceil(H / w) <= 64 output channels each (H = 192: up to 80 columns), LN1 stays a step; form B: one worker
//     per column, all H channels in passes of 64 through the same registers, LayerNorm 1 of the column in the step too (up to 256
//     columns).  The merged attention (and in form B y1) is never written.  The planner's rule only ever picks form B: form A alone
//     measured slower than the three steps at the headline workload and is reachable through vits_debug_persist_attn_fused(2) only
//     (same device path, one pass, no LN).  The step is compiled into persist_kernel_fz alone (persist_loop.hip.inc, below);
//   * matrix steps, one worker per (16-column tile, group of 16-row blocks, K-slice): gather the [C_in x (16 + taps - 1)] operand
//     window (<= 40 KB), 16x16x4 fp32 MFMAs with the 8 waves splitting the contraction at tap-unit granularity, epilogue (bias /
//     per-item bias / ReLU / mask / residual, WaveNet gate, spline inverse), cells out.  Contractions over 768 channels are split
//     into K-slices whose partial sums the consuming LayerNorm / coupling column step adds up;
//   * attention = 16 x 16 (query tile, key tile) block steps (each gathers three 16 x d_k tiles, partial softmax with the banded
//     relative-position terms of attentions.py:165-260) + a merge column step.
//   * a step is whatever records the resolver wrote for it: sequences longer than the worker count (T up to PS_MAX_T = 512 with
//     P = 256 workers) run a column step as two rounds of P columns and an attention step as rounds of P blocks -- the kernel is
//     the same (round 4; DESIGN.md "Programs beyond 256 columns").
// (A DDSConv layer in ONE step can be fused in two directions.  v1 of the duration predictor fused the column work into the matrix
// step, like conv16_kernel's PRO == 1: every one of the 16 workgroups of a column tile pulled the full 256-channel x 34-column window
// of two tensors and redid its LayerNorms and 8 k erf evaluations: 12 us per step, 208 us for the predictor against 265 us of launches.
// The fused column steps above go the other way round -- the matrix work moves into the column step, as a matrix-vector product --
// and recompute only what they would otherwise wait for: 4.5 us per step.)
// Reference ops: attentions.py:48-65,133-260,292-317 (Encoder / MultiHeadAttention / FFN), models.py:56-63,93-101 (duration
// predictor), modules.py:96-108,148-176,363-390 (DDSConv, WN, ConvFlow), models.py:374-393 (coupling layer).
#pragma once
#include "conv_small.hip.h"
#include "kernels_misc.hip.h"

typedef unsigned long long ll_t;  // {float value (bits 0..31), u32 epoch (bits 32..63)}

#define PS_THREADS 512
#define PS_WAVES 8
#define PS_MAX_STEPS 320
#define PS_MAX_T 512         // longest sequence of a program (columns beyond the worker count run as further rounds of a step)
#define PS_MAXC 256      // channels of a column step / contraction channels of one K-slice
#define PS_MAXU 8        // tap units (16 channels x 1 tap) per wave
#define PS_TP 21         // LDS pitch of the MFMA operand window [C_in][16 + taps - 1] (odd: the transposing writes are conflict-free)
#define PS_MAXROW 20     // 16 + taps - 1, taps <= 5
#define PS_DKP 128       // attention: head-dimension slots per row of threads (d_k <= 128)
#define PS_MKT 12        // key tiles the attention merge polls per round (3 cells each)
#define PS_SPIN_LIMIT (1 << 18)
#define PS_ERR_TIMEOUT 8  // bit in the session error word

struct PersistCtl {
  unsigned epoch;     // epoch of the last completed forward
  unsigned done;      // workers that finished the current forward (the last one publishes the epoch and resets this)
  unsigned abort;     // a worker timed out: everybody stops polling
  unsigned timeouts;  // diagnostics
};

enum { PK_IDLE = 0, PK_MM = 1, PK_DDS = 2, PK_LN = 3, PK_EMB = 4, PK_ATT = 5, PK_MERGE = 6, PK_COUPLE = 7, PK_DUR = 8, PK_EXPAND = 9 };
// flags (record dword 0, bits 8..)
enum {
  PF_RELU = 1 << 8, PF_INMASK = 1 << 9, PF_OUTMASK = 1 << 10, PF_GATE = 1 << 11, PF_SPLINE = 1 << 12, PF_ZINIT = 1 << 13, PF_LAST = 1 << 14,
  PF_PLAIN_IN = 1 << 15,   // PK_MM: operand = plain floats [channels][pT]; PK_COUPLE: previous z = plain floats
  PF_DW = 1 << 16, PF_FIN_LN = 1 << 17, PF_FIN_PRE = 1 << 18,  // PK_DDS
  PF_LN = 1 << 19,         // PK_LN: normalise (else: plain sum)
  PF_MV = 1 << 20,         // PK_DDS: the conv that consumes the column (the layer's 1x1 / the stack's projection) runs in this step
                           // PK_MERGE: conv_o + residual run in this step (with PF_LN: LayerNorm 1 of the column too)
};

// One work item of one worker in one step, resolved on the host (persist_plan.hip.h): 32 dwords.
//   dword 0      kind | flags
//   dwords 1..3  a1..a3 (kind-specific integers)
//   dwords 4..23 p0..p9 (pointers; p6 = weight fragments, p7 = bias, p8 = per-item bias / vector, p9 = packed per-thread parameters:
//                these four are valid in EVERY record -- zeros when unused -- so that the prefetch is straight-line code)
//   dwords 24..31 b0..b7 (kind-specific integers)
// PK_MM    a1 = Cs | K << 16 ; a2 = cell pitch of the operand * channel direction (signed; plain operands: +-1); a3 = t0 (first window column)
//          p0 operand (cells: (column 0, LOWEST channel of the slice); plain: the row of the slice's first channel),
//          p1 yout tile (cell (n0, first row)), p2 yplain (first row, column n0), p3 res tile, p4 z, p5 zout
//          b0 = n_u | nblk << 7;
//          b1 = floats between consecutive row blocks of the weights; b2 = ypitch; b3 = rows left (Cout - first row);
//          b4 = pT; b5 = rpitch; b6 = n0 | z_row << 16 | ea_row << 20; b7 = gate_H
// PK_DDS   a1 = C | dil << 16; a2 = t; p0 xin, p1 y2, p2 z row, p3 xout (null: not written), p4 bout
//          PF_MV: p4 = output cells of the fused conv (column 0, first channel of this worker), p6 = its slice of the transposed weights
//          (ps_mv_request), p7 = bias of its first channel; b1 = output channels of this worker (<= 64), b2 = bytes between consecutive
//          rows of 4 input channels (16 * C_out), b3 = such rows per wave (C / 32), b5 = channel pitch of the output cells
//          PF_MV | PF_SPLINE (dw == 0, one worker per column): the conv is ConvFlow.proj and the step ends with the inverse spline of its
//          column: p5 = z cells [2][Tp], p2 = zout (null for the last flow), b6 = z_row << 16 | ea_row << 20, PF_LAST as in PK_MM
// PK_LN    a1 = C; a2 = t; a3 = np; p0 part, p1 res, p2 base, p3 out, p4 oplain; b0/b1 = part stride (cells, 64 bit); b4 = pT
// PK_EMB   a1 = C; a2 = t; p0 emb, p3 out, p4 oplain; b0 = scale (float bits); b1 = n_vocab; b4 = pT
// PK_ATT   a1 = dk | nh << 8 | W << 16; a2 = i0 | j0 << 16; a3 = head | key tile << 8; p0 qkv, p1 ap
// PK_MERGE a1 = C; a2 = t; a3 = dk | nh << 8; p0 ap, p3 out; b0 = cells per key tile
//          PF_MV: y1 = x + conv_o(merged column) for this worker's channels: p1 = residual x cells, p3 = output cells (both: column 0,
//          first channel of this worker, channel pitch C), p6 = its slice of the transposed weights (ps_mv_request_at), p7 = bias of its
//          first channel; b1 = output channels of this worker (<= 64 per pass, passes of 64), b2 = bytes between consecutive rows of 4
//          input channels (16 * C), b3 = such rows per wave (C / 32).  PF_MV | PF_LN (one worker per column, b1 = C): the step ends with
//          LayerNorm 1 of its column (p9: gamma, beta) and p3 receives x1
// PK_COUPLE a1 = C (= 2H); a2 = t; a3 = np | H << 16; p0 part, p1 u cells, p2 u plain, p3 out, p4 oplain; b0/b1 = part stride; b4 = pT
// PK_DUR   (one worker) a1 = T_x; a2 = frame capacity (0: none); flag PF_PLAIN_IN: logw is not waited for (no duration predictor in this
//          program); p0 logw cells [T_x], p1 dur (plain int), p2 cum (plain int), p3 cum cells, p4 y_len int32, p5 y_len int64, p6 y_len cell
// PK_EXPAND a1 = I; a2 = frame f; a3 = T_x; flag PF_PLAIN_IN: stats / cum are plain arrays of an earlier launch; p0 stats cells [T_x][2I] or
//          plain [2I][T_x], p1 cum cells or plain int [T_x], p3 out cells [T_y][I], p4 oplain [I][pT]; b4 = pT
struct alignas(16) PRec {
  int kf, a1, a2, a3;
  unsigned long long p[10];
  int b[8];
};
static_assert(sizeof(PRec) == 128, "PRec is 32 dwords");

struct PProgram {
  int n_steps, T, Tp, P;
  int nb; float bound, inv_sqrt_d;      // spline
  const int* len;
  const float* ea_m; const float* ea_logs;
  float* logw;                          // duration predictor result [T] (plain floats)
  int* err;
  const PRec* recs;                     // [n_steps][P]
  // programs that cover both halves of the forward (text side laid out for T_x, frame side for T_y): from step seg_step on the kernel
  // works with (T2, Tp2) and the utterance's frame count, which the PK_DUR step of the SAME launch publishes in the cell len2 (-1: one half only)
  int seg_step, T2, Tp2;
  const ll_t* len2;
  ll_t* logw_cells;                     // duration predictor result as cells for PK_DUR (null: plain only)
};

struct PCall {                          // per-call values (by value: a captured graph re-reads `dv`, not these, when dv != null)
  PersistCtl* ctl;
  const long long* ids;                 // text encoder: token ids [T] (the feed's int64 tensor)
  const float* noise;                   // duration predictor: [2][T] injected noise or null (Philox)
  float nsw;
  unsigned long long seed;
  int solo;
  const SynthDev* dv;
  const unsigned long long* item_seeds;
  long long* trace;                     // tools only (VITS_PS_TRACE): [P][PS_MAX_STEPS][8] cycle stamps, null in production
  const int* forced;                    // PK_DUR: pinned durations [T_x] (null: from logw)
  float length_scale, noise_scale;      // PK_DUR / PK_EXPAND (overridden by dv)
  const float* noise_prior;             // PK_EXPAND: injected prior noise [I][noise_stride] or null (Philox stream 2)
  long long noise_stride;
  int* dbg;                             // device words of the model: [0] poll rounds before a worker gives up (0 = PS_SPIN_LIMIT; tests shrink it to
                                        // force the fallback -- read at run time, so captured graphs follow the hook), [1] completed persistent launches
};

#define PS_G __attribute__((address_space(1)))
__device__ __forceinline__ ll_t ll_pack(float v, unsigned e) { return ((ll_t)e << 32) | (ll_t)__float_as_uint(v); }
__device__ __forceinline__ void ll_store(PS_G ll_t* p, float v, unsigned e) {
  __hip_atomic_store(p, ll_pack(v, e), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_store_dwordx2 ... sc1
}
__device__ __forceinline__ ll_t ll_load(const PS_G ll_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // global_load_dwordx2 ... sc1
}
__device__ __forceinline__ ll_t ll_load_off(const PS_G ll_t* base, unsigned byte_off) {
  return ll_load((const PS_G ll_t*)((const PS_G char*)base + byte_off));
}
__device__ __forceinline__ void ll_store_off(PS_G ll_t* base, unsigned byte_off, float v, unsigned e) {  // uniform base + 32-bit lane offset
  ll_store((PS_G ll_t*)((PS_G char*)base + byte_off), v, e);
}
__device__ __forceinline__ float ll_val(ll_t q) { return __uint_as_float((unsigned)q); }
__device__ __forceinline__ unsigned ll_bad(ll_t q, unsigned epoch) { return (unsigned)(q >> 32) ^ epoch; }

// a record lives in 4 VGPRs (dwordx4 of lanes 0..7); fields are read with v_readlane (wave-uniform results in SGPRs)
typedef int ps_i4 __attribute__((ext_vector_type(4)));
#define PR_I(rv, i) __builtin_amdgcn_readlane((rv)[(i) & 3], (i) >> 2)
#define PR_P(T, rv, k) ((PS_G T*)(((unsigned long long)(unsigned)PR_I(rv, 5 + 2 * (k)) << 32) | (unsigned long long)(unsigned)PR_I(rv, 4 + 2 * (k))))
#define PR_B(rv, k) PR_I(rv, 24 + (k))

#define PS_GELU(v) c16_gelu(v)

struct PsCtx {
  unsigned epoch;
  int aborted;        // this wave gave up (or saw ctl->abort): polls return at once
  int spins;
  int limit;
  PersistCtl* ctl;
};
// one more round of a poll loop: true = keep polling.  `pending` is wave-uniform (a ballot).
__device__ __forceinline__ bool ps_again(PsCtx& cx, bool pending) {
  // The poll state is wave-uniform by construction, but hipcc's uniformity analysis gives up on it (it is carried around the step
  // loop through every kind's control flow) and kept `aborted` / `spins` as per-lane values: the exit test of every poll loop was a
  // vector compare under an exec mask.  readfirstlane at the point of use puts the test back on the scalar unit.
  if (!pending || __builtin_amdgcn_readfirstlane(cx.aborted)) { cx.spins = 0; return false; }
  const int spins = __builtin_amdgcn_readfirstlane(cx.spins) + 1;
  cx.spins = spins;
  // a poll that has failed a few rounds is waiting for something that is far away (another stage of the program, a slow worker): back
  // off instead of hammering the fabric next to the workers that are computing (MI355X_MICROARCH.md "polling-cost")
  if (spins > 8) __builtin_amdgcn_s_sleep(8);
  if ((spins & 1023) == 0 &&
      __builtin_amdgcn_readfirstlane(__hip_atomic_load(&cx.ctl->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) { cx.aborted = 1; return false; }
  if (spins >= cx.limit) {
    cx.aborted = 1;
    if ((threadIdx.x & 63) == 0) {
      __hip_atomic_store(&cx.ctl->abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      atomicAdd(&cx.ctl->timeouts, 1u);
    }
    return false;
  }
  return true;
}
#define PS_PENDING(bad) (__builtin_amdgcn_ballot_w64((bad) != 0) != 0)

// sum / max over lanes (DPP row operations + two row broadcasts: no LDS, ~10 instructions).  Lanes disabled by ROW_MASK contribute 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float ps_dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ float ps_dpp_max(float v) {  // row-local controls only: every lane has a source
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false)));
}
__device__ __forceinline__ float ps_row_sum(float v) {  // sum over each 16-lane row, in every lane of the row
  v = ps_dpp_add<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v = ps_dpp_add<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v = ps_dpp_add<0x141, 0xF>(v);  // row_half_mirror
  v = ps_dpp_add<0x140, 0xF>(v);  // row_mirror
  return v;
}
__device__ __forceinline__ float ps_row_max(float v) {
  v = ps_dpp_max<0xB1>(v);
  v = ps_dpp_max<0x4E>(v);
  v = ps_dpp_max<0x141>(v);
  v = ps_dpp_max<0x140>(v);
  return v;
}
template <int N>
__device__ __forceinline__ float ps_row_shr(float v) {  // lane k <- lane k - N of its 16-lane row (0 where the row has no such lane)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x110 + N, 0xF, 0xF, true));
}
__device__ __forceinline__ float ps_wave_sum(float v) {  // sum over the 64 lanes, in every lane
  v = ps_row_sum(v);
  v = ps_dpp_add<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  v = ps_dpp_add<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3: lane 63 holds the total
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// sums of two values over the 256 threads of each HALF of the workgroup (waves 0-3 / 4-7): one barrier; `red` is a private
// 16-float scratch of this call site (no second barrier: the next call site uses another one)
__device__ __forceinline__ void ps_half_sum2(float& a, float& b, float* red, int wave, int lane) {
  a = ps_wave_sum(a);
  b = ps_wave_sum(b);
  if (lane == 0) { red[wave] = a; red[8 + wave] = b; }
  __syncthreads();
  const int w0 = wave & 4;
  a = (red[w0] + red[w0 + 1]) + (red[w0 + 2] + red[w0 + 3]);
  b = (red[8 + w0] + red[8 + w0 + 1]) + (red[8 + w0 + 2] + red[8 + w0 + 3]);
}

// ---- what a worker requests one step ahead (registers; straight-line: a load behind a branch makes hipcc wait for it at the join,
//      i.e. puts a cold round trip in the middle of a step)
struct PsPre {
  f32x4 a[PS_MAXU];   // weight fragments of the first 16-row block: tap units u = wave + PS_WAVES * i
  f32x4 pk0, pk1;     // packed per-thread parameters: 8 floats of row (tid & 255) -- attention: row tid of the table pack
  float eb0, eb1, ec0, ec1;  // epilogue operands of thread tid < 256 (bias, per-item bias / vector; second pair: the sigmoid row of a gate)
};
// LDS byte offset of tap unit u = wave + 8 i inside the operand window [C_in][PS_TP] for K = 1 / 3 / 5 taps: unit u = (16-channel
// chunk u / K, tap u % K) -> (chunk * 16 * PS_TP + tap) * 4.  One s_load_dwordx8 per step instead of a division-free but
// 8-instruction (chunk, tap) update per unit per wave.
struct PsUnitTab { int off[3][PS_WAVES][PS_MAXU]; };
static constexpr PsUnitTab ps_make_unit_tab() {
  PsUnitTab t{};
  for (int ki = 0; ki < 3; ++ki)
    for (int w = 0; w < PS_WAVES; ++w)
      for (int i = 0; i < PS_MAXU; ++i) {
        const int K = 2 * ki + 1, u = w + PS_WAVES * i;
        t.off[ki][w][i] = ((u / K) * 16 * PS_TP + (u % K)) * 4;
      }
  return t;
}
__constant__ PsUnitTab ps_unit_tab = ps_make_unit_tab();

__device__ __forceinline__ void ps_load_weights(const PS_G float* w, int n_u, int wave, int lane, f32x4 (&a)[PS_MAXU]) {
  // units beyond n_u repeat the last one (an L1 hit; never used: the MFMA loop tests u < n_u).  The unit index is wave-uniform:
  // clamp and scale on the scalar unit, one 32-bit lane offset for all eight loads.
  const PS_G char* base = (const PS_G char*)w;
  const unsigned lane_off = (unsigned)lane * 16u;
#pragma unroll
  for (int i = 0; i < PS_MAXU; ++i) {
    const int u = wave + PS_WAVES * i;
    const unsigned uo = (unsigned)__builtin_amdgcn_readfirstlane(u < n_u ? u : n_u - 1) * 1024u;
    a[i] = *(const PS_G f32x4*)(base + (uo + lane_off));
  }
}
// epilogue operand indices of thread tid relative to the record's bias / vector pointers
__device__ __forceinline__ void ps_epi_idx(int kf, int rows_left, int gate_H, int tid, int blk, int& i0, int& i1) {
  if (kf & PF_GATE) { i0 = blk * 8 + (tid & 7); i1 = gate_H + i0; }   // [8 tanh | 8 sigmoid] rows of channels 8 * mb + ch
  else {
    i0 = blk * 16 + (tid & 15);
    i0 = i0 < rows_left ? i0 : rows_left - 1;
    i1 = i0;
  }
}
// column / attention / merge steps: packed parameters (row tid of the pack; attention: 512 rows) and the per-item vector
__device__ __forceinline__ void ps_prefetch_light(const ps_i4& r, int tid, PsPre& pre) {
  const int kind = PR_I(r, 0) & 0xff;
  const PS_G f32x4* pk = PR_P(const f32x4, r, 9);
  const int row = tid & (kind == PK_ATT ? 511 : 255);
  pre.pk0 = pk[row * 2];
  pre.pk1 = pk[row * 2 + 1];
  const int C = PR_I(r, 1) & 0xffff;
  int i0 = tid & 255; i0 = i0 < C ? i0 : C - 1; i0 = i0 < 0 ? 0 : i0;
  pre.ec0 = PR_P(const float, r, 8)[i0];
}
// matrix steps: weight fragments of the first row block and the epilogue vectors (straight-line: behind a branch the loads cost a
// conservative wait in the epilogue, measured +0.5 .. 1.3 k cycles per step)
__device__ __forceinline__ void ps_prefetch(const ps_i4& r, int tid, int wave, int lane, PsPre& pre) {
  const int kf = PR_I(r, 0);
  int i0, i1;
  ps_epi_idx(kf, PR_B(r, 3), PR_B(r, 7), tid, 0, i0, i1);
  const PS_G float* b = PR_P(const float, r, 7);
  const PS_G float* c = PR_P(const float, r, 8);
  pre.eb0 = b[i0]; pre.eb1 = b[i1]; pre.ec0 = c[i0]; pre.ec1 = c[i1];
  ps_load_weights(PR_P(const float, r, 6), PR_B(r, 0) & 0x7f, wave, lane, pre.a);
}

// Fused column steps (PF_MV): y[o] = bias[o] + sum_k W[o][k] b[k] for the <= 64 output channels o of this worker, the column b in LDS.
// The weights are packed transposed, Wt[k / 4][o][k % 4] (engine_model.hip.h conv_wt4): lane = output channel, one dwordx4 = four
// input channels, consecutive lanes read consecutive 16 bytes.  The 8 waves split the contraction (C / 8 input channels each, C / 32
// dwordx4 <= PS_MAXU), so the whole slice of a worker is ONE request of <= 8 loads per lane at the top of the step.  Rows beyond the
// wave's share repeat its last one, lanes beyond the worker's channels its last channel (L1 hits, never used).
// (Registers of the step, not the PsPre of the step loop: nothing of a column step is carried around the loop.)
struct PsMv { f32x4 a[PS_MAXU]; float bias; };
__device__ __forceinline__ void ps_mv_request(const ps_i4& r, int tid, int wave, int lane, PsMv& pre) {
  const PS_G char* base = (const PS_G char*)PR_P(const float, r, 6);
  const int n = PR_B(r, 1), kq = PR_B(r, 3);
  const unsigned rowb = (unsigned)PR_B(r, 2);
  const unsigned lane_off = (unsigned)(lane < n ? lane : n - 1) * 16u;
#pragma unroll
  for (int i = 0; i < PS_MAXU; ++i) {
    const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane(wave * kq + (i < kq ? i : kq - 1)) * rowb;
    pre.a[i] = *(const PS_G f32x4*)(base + (ro + lane_off));
  }
  pre.bias = PR_P(const float, r, 7)[tid < n ? tid : n - 1];
}
// this wave's share of the contraction; b4 = the column in LDS (16-byte aligned: every lane reads the same address -- a broadcast)
__device__ __forceinline__ float ps_mv_dot(const PsMv& pre, const float* bcol, int wave, int kq) {
  const f32x4* b4 = reinterpret_cast<const f32x4*>(bcol) + wave * kq;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < PS_MAXU; ++i)
    if (i < kq) {
      const f32x4 bb = b4[i];
      acc = fmaf(pre.a[i][0], bb[0], acc); acc = fmaf(pre.a[i][1], bb[1], acc);
      acc = fmaf(pre.a[i][2], bb[2], acc); acc = fmaf(pre.a[i][3], bb[3], acc);
    }
  return acc;
}

// One pass of a fused attention-merge step (PK_MERGE | PF_MV): the weights of output channels [64 pass, 64 pass + 64) of this worker's
// `tot` channels -- the request of ps_mv_request at a channel offset, without the bias (one load per thread for all passes, in the step).
__device__ __forceinline__ void ps_mv_request_at(const ps_i4& r, int wave, int lane, int pass, f32x4 (&a)[PS_MAXU]) {
  const int tot = PR_B(r, 1), kq = PR_B(r, 3), o0 = pass * 64;
  const int n = tot - o0 < 64 ? tot - o0 : 64;
  const PS_G char* base = (const PS_G char*)PR_P(const float, r, 6) + (unsigned)o0 * 16u;
  const unsigned rowb = (unsigned)PR_B(r, 2);
  const unsigned lane_off = (unsigned)(lane < n ? lane : n - 1) * 16u;
#pragma unroll
  for (int i = 0; i < PS_MAXU; ++i) {
    const unsigned ro = (unsigned)__builtin_amdgcn_readfirstlane(wave * kq + (i < kq ? i : kq - 1)) * rowb;
    a[i] = *(const PS_G f32x4*)(base + (ro + lane_off));
  }
}
__device__ __forceinline__ float ps_mv_dot_a(const f32x4 (&a)[PS_MAXU], const float* bcol, int wave, int kq) {
  const f32x4* b4 = reinterpret_cast<const f32x4*>(bcol) + wave * kq;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < PS_MAXU; ++i)
    if (i < kq) {
      const f32x4 bb = b4[i];
      acc = fmaf(a[i][0], bb[0], acc); acc = fmaf(a[i][1], bb[1], acc);
      acc = fmaf(a[i][2], bb[2], acc); acc = fmaf(a[i][3], bb[3], acc);
    }
  return acc;
}

// Inverse rational-quadratic spline of ConvFlow (transforms.py:55-177), the arithmetic of spline_inverse_elem (kernels_misc.hip.h) in
// the two pieces both step forms use: the matrix step for the 16 columns of its tile (h and the knots at pitch 16), the fused column
// step for its one column (pitch 1).
// Knots: softmax over the bins, cumulative sum and knots (transforms.py:96-131) with the 16 lanes of a DPP row = the bins k of ONE
// (column, widths / heights) pair: row maximum, row sum and the inclusive prefix are DPP row operations (no LDS, no loop).
__device__ __forceinline__ void ps_spline_knots(const float* h, int hs, int which, int k, int nb, float isd, float bound, float* cdst, int cs) {
  const bool kok = k < nb;
  const float u = kok ? h[(which * nb + k) * hs] * isd : -3.0e38f;
  const float mx = ps_row_max(u);
  const float e = kok ? expf(u - mx) : 0.f;
  const float sum = ps_row_sum(e);
  const float mn = 1e-3f;  // min_bin_width == min_bin_height
  float c = kok ? mn + (1.f - mn * nb) * (e / sum) : 0.f;
  c += ps_row_shr<1>(c);
  c += ps_row_shr<2>(c);
  c += ps_row_shr<4>(c);
  c += ps_row_shr<8>(c);
  if (k == 0) cdst[0] = -bound;
  if (kok) cdst[(k + 1) * cs] = k == nb - 1 ? bound : 2.f * bound * c - bound;
}
// One column: bin search and the quadratic.  cw / ch: its width / height knots (pitch cs), hd: its derivative parameters (pitch hs)
__device__ __forceinline__ float ps_spline_solve(float y, const float* cw, const float* ch, int cs, const float* hd, int hs, int nb, float bound, float cst) {
  float v1 = y;
  if (y >= -bound && y <= bound) {  // identity outside the interval (transforms.py:65-77)
    int bin = -1;
    for (int k = 0; k <= nb; ++k) {
      const float loc = ch[k * cs] + (k == nb ? 1e-6f : 0.f);
      if (y >= loc) bin++;
    }
    bin = bin < 0 ? 0 : (bin > nb - 1 ? nb - 1 : bin);
    const float in_cw = cw[bin * cs], in_w = cw[(bin + 1) * cs] - in_cw;
    const float in_ch = ch[bin * cs], in_h = ch[(bin + 1) * cs] - in_ch;
    const float min_d = 1e-3f;
    const float ud0 = (bin == 0) ? cst : hd[(bin - 1) * hs];
    const float ud1 = (bin == nb - 1) ? cst : hd[bin * hs];
    const float d0 = min_d + softplus_f(ud0), d1 = min_d + softplus_f(ud1);
    const float delta = in_h / in_w;
    const float t1 = (y - in_ch) * (d0 + d1 - 2.f * delta);
    const float qa = t1 + in_h * (delta - d0);
    const float qb = in_h * d0 - t1;
    const float qc = -delta * (y - in_ch);
    const float disc = qb * qb - 4.f * qa * qc;
    const float root = (2.f * qc) / (-qb - sqrtf(disc));
    v1 = root * in_w + in_cw;
  }
  return v1;
}

// Placed where a poll has just completed: the record of step s + 1 (requested at the top of this step, older than every poll load) is
// certainly there -- touching it HERE makes the compiler account for its wait at a point where it costs nothing.  Without this the
// hand-over rv = rvB at the loop's back edge is the first use, and because loads and stores share the in-order vmcnt counter the
// compiler waits there for vmcnt(0): for the step's own output stores (an sc1 write round trip per step).
#define PS_REC_READY() asm volatile("" : "+v"(rvB))
// cycle stamps for tools/ps_trace.py: only in the -DPS_TRACE build (libvits_mi355_pstrace.so) -- at 2 waves per SIMD every instruction
// of a step is on its critical path, and eight guarded stamps per step were ~40 of them
#ifdef PS_TRACE
#define PS_STAMP(k) do { if (call.trace && tid0 == 0) call.trace[((long long)rank * PS_MAX_STEPS + s) * 8 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define PS_STAMP(k) do { } while (0)
#endif

// LDS of the kernel (floats).  Matrix steps: operand window + partial tiles + spline scratch; attention blocks: Q / K / V tiles and
// the two relative-position tables alias the operand window, scores / probabilities alias the partial tiles.
#define PS_LDS_TILE (3 * 16 * (PS_DKP + 4) + (10 + 12) * (PS_DKP + 4))   // >= PS_MAXC * PS_TP
#define PS_LDS_MRED (PS_WAVES * 256)
static_assert(PS_LDS_TILE >= PS_MAXC * PS_TP, "operand window does not fit");

// The step loop, in two kernels from ONE source (persist_loop.hip.inc).  persist_kernel_fz has the fused merge step compiled in and is
// launched for programs that contain one; persist_kernel has not and runs every other program: the code they ran before that form
// existed.  As one kernel, the longer MERGE branch cost programs WITHOUT a fused step 12.6 us per forward (30 us with two more register
// sets); as one template body instantiated twice, the never-fused instance was still 22 us slower than before (140 instead of 164
// VGPRs: another allocation of the step loop).  profiles/persist_attn_fused_bench.txt; the trap of DESIGN.md section 6 row 4.
#define PS_KERNEL_NAME persist_kernel
#define PS_FZ 0
#include "persist_loop.hip.inc"
#undef PS_KERNEL_NAME
#undef PS_FZ
#define PS_KERNEL_NAME persist_kernel_fz
#define PS_FZ 1
#include "persist_loop.hip.inc"
#undef PS_KERNEL_NAME
#undef PS_FZ

// ---- packed per-thread parameters of a step (built once per model: persist_plan.hip.h): dst[row][k] = src[k][row + add[k]] or 0
struct PsPackArgs { const float* src[8]; int add[8]; int len[8]; };
__global__ void ps_pack_kernel(float* dst, PsPackArgs a, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * 8) return;
  const int row = i >> 3, k = i & 7;
  const int idx = row + a.add[k];
  dst[i] = (a.src[k] && idx >= 0 && idx < a.len[k]) ? a.src[k][idx] : 0.f;
}
