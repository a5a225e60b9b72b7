// Shared helpers of libfaceformer_hip (gfx950 only; wavefront = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "faceformer_hip.h"

#define FF_WAVE 64
#define FF_MAX_STREAMS 8

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- error reporting -------------------------------------------------------------------------
void ff_set_error(const char* fmt, ...);

#define FF_CHECK_ARG(cond, ...)           \
  do {                                    \
    if (!(cond)) {                        \
      ff_set_error(__VA_ARGS__);          \
      return FF_ERR_ARG;                  \
    }                                     \
  } while (0)

#define FF_CHECK_HIP(expr)                                                             \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) {                                                            \
      ff_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return FF_ERR_LAUNCH;                                                            \
    }                                                                                  \
  } while (0)

#define FF_CHECK_LAUNCH() FF_CHECK_HIP(hipGetLastError())

#define FF_RETURN_IF(expr)       \
  do {                           \
    int _s = (expr);             \
    if (_s != FF_OK) return _s;  \
  } while (0)

static inline bool ff_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int ff_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t ff_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- optional per-category event profiling (bench.py's roofline leg) ---------------------------
// When enabled via ff_profile_begin(), every op launch is bracketed by a hipEvent pair on its own
// stream; ff_profile_end() synchronises and sums elapsed time / algorithmic work per category.
enum ff_prof_cat { FF_CAT_GEMM = 0, FF_CAT_ATTN = 1, FF_CAT_LN = 2, FF_CAT_POINTER = 3, FF_CAT_ROWOP = 4, FF_CAT_CHAIN = 5, FF_CAT_GEMM_X3 = 6, FF_NUM_CAT = 7 };
bool ff_prof_enabled();
void ff_prof_open(int cat, double work, hipStream_t st);
void ff_prof_close(hipStream_t st);
void ff_prof_add_bytes(int cat, double bytes);  // algorithmic bytes of the launch (operands read + results written once)
struct FFProfScope {
  hipStream_t st;
  bool on;
  FFProfScope(int cat, double work, hipStream_t s) : st(s), on(ff_prof_enabled()) {
    if (on) ff_prof_open(cat, work, st);
  }
  ~FFProfScope() {
    if (on) ff_prof_close(st);
  }
};

// bumped by every setter that changes how an operator is launched (ff_set_gemm_tuning, ff_set_attention_algo): kept for
// callers that cache launch decisions
unsigned long long ff_tuning_epoch();
void ff_tuning_changed();

// compute units of the current device (cached per device; 256 on an MI355X in SPX mode)
int ff_num_cus();

// ---- tuning knobs (round 6): ONE table, read from the environment once, settable per process through ff_set_tuning() ----------
// Every A/B switch of the library lives here: the name is the environment variable that initialises it, the value
// an int.  Defaults are the product; tests and tools flip them in-process (no child process needed) and the engine takes ONE
// snapshot of the ones that shape a decode at the top of ff_decode / ff_decode_workspace_bytes.
enum FFKnob {
  FF_K_L0_FOLD = 0,               // 1: the pointer launch leaves the appended rows' LayerNorm statistics (0: a LayerNorm launch)
  FF_K_POINTER_FOLD,              // 1: decoder.norm + project + pointer dot products as one GEMM for one-wireframe micro-batches
  FF_K_LAST_QKV_ONE_LAUNCH_ROWS,  // pruned last layer: one q|k|v launch up to this many active rows
  FF_K_PINNED_COUNTERS,           // host-mapped stop-counter slots a decode may use (<= the 65536 allocated)
  FF_K_DEBUG_TIMING,              // ff_decode prints host-side enqueue / wait times
  FF_K_DMA_MIN_ROWS, FF_K_DMA_MIN_ROWS_N512, FF_K_DMA_MIN_ROWS_WIDE,   // rows from which a projection takes the LDS-DMA f32 kernel
  FF_K_SK_HYBRID, FF_K_SK_HYBRID_FIX, FF_K_SK_HYBRID_MAXLEFT8, FF_K_SK_HYBRID_MINU, FF_K_SK_HYBRID_FORCE,
  FF_K_NO_PANEL,                  // 1: small-M launches never take gemm_panel_kernel
  FF_K_X3_SMALL_SPLIT,            // split kernel: K-pieces on idle CUs below one tile per CU
  FF_K_RK_SPLIT_OLD, FF_K_RK_SPLIT_YOUNG, FF_K_RK_PHASE, FF_K_RK_ROTATE,   // K/V-resident attention probes
  FF_K_X3_NEED_N1024, FF_K_X3_NEED_N512,   // split products: rows needed by the 1024- / 512-column projections, in quarters of x3_min_rows
  FF_K_X2H_ATTN,                  // 1: cross-attention launches whose descriptor carries fp16 planes take the 2 x fp16 kernel
  FF_K_LAST_FOLD_MIN_ROWS,        // pruned last layer: k | v folded into the query from this many active rows on (0: never)
  FF_K_COUNT
};
int ff_knob(int id);

// 2 x fp16 cross-attention (ff_attention_x2h.hip)
size_t ff_attention_planes_stride();
bool ff_attention_x2h_ok(const ff_attn_desc& d);
int ff_attention_x2h_launch(const ff_attn_desc& d, const void* planes, long long plane_stride, hipStream_t st);

// ff_pointer_argmax with the decode engine's stop-rule hand-over (ff_pointer.hip)
struct ff_pointer_sync {
  int* seen;        // [B] or null: count_eq counts a sequence's first eq_value only (FF_STOP_EACH_EOS)
  int* arrive;      // device int, zero before the launch: arrivals of the launch's sequences
  int* host_slot;   // device-visible address of a host-mapped pinned int: receives the launch's counter
  int host_which;   // 0: count_ge, 1: count_eq
  float* next_stats;  // [B, E/32, 2] or null: (mean, M2) per 32-column segment of the rows written to next_rows -- the
                      // LayerNorm statistics the folded layer-0 projection of the NEXT step consumes (ff_gemm_f32_ln)
  int logits_ready;   // 1: `logits` already holds the raw dot products (the engine's folded project + pointer GEMM): p is not read
  // FF_RETIRE_FINISHED: launch row b decodes sequence slot[b] (an index into next_tok / best / second / extra_mask rows; logits,
  // next_rows and next_stats stay in launch order), fin[seq] its finish position (> fin_j: none yet).  count_ge counts the
  // unfinished sequences only; a token in [term_lo, term_hi) records fin[seq] = fin_j, the position this launch writes.
  const int* slot;
  int* fin;
  int fin_j, term_lo, term_hi;
};
int ff_pointer_argmax_sync(const float* p, int ldp, const float* memory, int S, int E, const unsigned char* mask,
                           const int* kv_len, const unsigned char* extra_mask, int ldextra, int B, int seqs_per_group,
                           int* next_tok, float* best, float* second, float* logprob, float* logits, int ldlogits,
                           float* next_rows, int ldnext, int* count_ge, int ge_bound, int* count_eq, int eq_value,
                           const ff_pointer_sync* sync, ff_stream_t stream);   // logprob: [B] or null (ff_pointer_argmax_lp)

// What every selection launch of a decode step takes (internal: the extern "C" operators build it from their parameter lists,
// the engine fills it once per step).  ff_step_args (ff_launch.h) checks it and fills the launch's PointerArgs from it.
struct ff_step_io {
  float* logits; int ldlogits;             // [rows, ldlogits] raw logits in, masked logits out
  int S; const unsigned char* mask; const int* kv_len;
  int rows, rows_per_wireframe;            // launch rows (sequences, beams or samples) and how many of them share a wireframe
  int term_lo, term_hi, ge_bound;          // terminator range; count_ge counts the selected tokens >= ge_bound
  const float* memory; int E;
  float* next_rows; int ldnext;            // or null: the next decoder input rows memory[w, token]
  float* next_stats;                       // [rows, E/32, 2] or null: their LayerNorm segment statistics
  int* count_ge;                           // or null: the launch's stop counter
  int *arrive, *host_slot;                 // decode engine only: arrivals of the launch's waves (zero before it), and the host-mapped
                                           // pinned int that receives count_ge from the last one
};

// The selection operators on a descriptor (ff_beam.hip, ff_sample.hip, ff_constrain.hip, ff_constrain_beam.hip, ff_forced.hip), and
// the start state / output packing of each decode mode (kernels' comments).  Beam forms: io.rows = groups * width, and the
// width and sizes are checked by ff_beam_check_sizes before that product is formed (the extern "C" entries; the engine's own checks).
int ff_beam_check_sizes(const char* op, int groups, int width, int groups_per_wireframe, int S);
int ff_beam_select_sync(const ff_step_io& io, int width, const float* scores_in, float* scores_out, const int* fin_in, int* fin_out,
                        int* hist, int ldhist, int t, int* parent, int* next_tok, ff_stream_t stream,
                        int form = 0);   // (1 / 2: the single-sequence decode's forms, count_ge counts "all" / "best")
int ff_sequence_beam_init(int* tok, float* score, int* fin, int* parent, int Bc, int W, int sos, hipStream_t st);
int ff_beam_init(int* tok, float* score, int* fin, int* parent, int Bc, int Fc, int W, int f0, const int* num_input, int pad_tok,
                 int term_lo, int term_hi, hipStream_t st);
int ff_beam_finalize(const int* tok, const int* parent, const float* score, int Btot, int T, const int* steps_dev,
                     const int* num_input, int dedup, int F, int W, int w0, int nw, int Fc, int f0, int b0, int64_t* beams,
                     float* scores, int64_t* predict, int* seq_of_row, hipStream_t st, const int* fin = nullptr,
                     int* finished = nullptr);   // (the finished flags of the stop step's row: the sequence beam decode's output)

// Forced decode (ff_forced.hip): the [rows, T] int64 paths as the engine's position-major int32 tokens (clamped into [0, S)),
// and the output packing (kernels' comments).
int ff_pointer_forced_sync(const ff_step_io& io, const int* forced, float* logprob, int* greedy, int* rank, ff_stream_t stream);
int ff_forced_tokens(const int64_t* paths, int* tok, int rows, int T, int S, hipStream_t st);
int ff_forced_finalize(const int* tok, const float* lp_all, const int* greedy_all, const int* rank_all, const int* lengths, int rows,
                       int T, float* logprob, int64_t* greedy, int* rank, float* seq_logprob, hipStream_t st);

// (sampled decode)  What a draw reads besides the step descriptor, and its check for operator `op` (ff_sample.hip).
struct ff_sample_draw_io { const float* uniforms; int num_uniforms; const int* row_id; float temperature; int top_k; float top_p; };
int ff_sample_draw_check(const char* op, const ff_sample_draw_io& d, int rows);
int ff_pointer_sample_sync(const ff_step_io& io, const float* uniforms, int num_uniforms, const int* row_id, const int* fin_in,
                           float temperature, int top_k, float top_p, int* next_tok, float* logprob, int* fin_out, ff_stream_t stream,
                           bool sequence_form = false);   // (the single-sequence decode's form: count_ge counts the rows unfinished after the step)
int ff_sequence_sample_init(int* tok, float* lp, int* fin, int* row_id, int Bc, int R, int w0, int sos, hipStream_t st);
int ff_sample_init(int* tok, float* lp, int* fin, int* row_id, int Bc, int Fc, int R, int f0, int w0, int F, const int* num_input,
                   int pad_tok, int term_lo, int term_hi, hipStream_t st);
int ff_sample_finalize(const int* tok, const float* lp, const int* fin, int Btot, int T, const int* steps_dev, const int* num_input,
                       int dedup, int F, int R, int w0, int nw, int Fc, int f0, int b0, int64_t* samples, float* logprob,
                       float* scores, int64_t* predict, int* seq_of_row, hipStream_t st);

// The loop rule's operands of a constrained step, and their check for operator `op` (ff_constrain.hip): the flag bits,
// L = S - ntok, the terminator range inside the special tokens, FF_CONSTRAIN_CONNECT with its follow table.
struct ff_loop_rule_io { const unsigned* follows; int L, flags, ntok; };
int ff_loop_rule_check(const char* op, const ff_loop_rule_io& r, int S, int term_lo, int term_hi);
// Constrained decode.  state: what a step reads and writes per row; ahead (or null): the closure look-ahead, or
// with `exact` the exact one (close_dist unused, null).
struct ff_constrained_state {
  const int *fin_in, *first_in, *prev_in;
  unsigned* visited; unsigned char* mask_rows;
  int* next_tok; float* logprob;
  int *fin_out, *dead_end, *first_out, *prev_out;
};
constexpr int FF_EXACT_MAX_S = 2048;   // keys (L + ntok) of a row the exact look-ahead's search takes
struct ff_lookahead_io { const unsigned char *close_dist, *cycle_len; int budget; int exact; };
int ff_lookahead_check(const char* op, const ff_loop_rule_io& rule, int S, const ff_lookahead_io& ahead);
int ff_pointer_constrained_sync(const char* op, const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& st,
                                const ff_lookahead_io* ahead, ff_stream_t stream);
int ff_constrain_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int Bc, int Fc, int f0,
                      const int* num_input, int pad_tok, int term_lo, int term_hi, int ntok, const unsigned* follows, int L,
                      hipStream_t st);
int ff_constrain_finalize(const int* tok, const float* lp, const int* fin, const int* dead, int Btot, int T, const int* steps_dev,
                          const int* num_input, int dedup, int F, int w0, int nw, int Fc, int f0, int b0, int64_t* predict,
                          float* logprob, int* dead_end, int* seq_of_row, hipStream_t st);

// Sequence-constrained decode (ff_constrain_seq.hip): the constrained step's operands with the two tokens of the
// single-sequence rule in place of a terminator range (io's is not read); one sequence per wireframe, every one from SOS.
int ff_sequence_rule_check(const char* op, const ff_loop_rule_io& r, int S, int tok_sep, int tok_eos);
// `ahead`: the closure look-ahead's tables and budget, null = the plain launch.
int ff_pointer_sequence_constrained_sync(const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& st, int tok_sep,
                                         int tok_eos, const ff_lookahead_io* ahead, ff_stream_t stream);
int ff_sequence_constrain_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int Bc, int L, int sos,
                               hipStream_t st);
int ff_sequence_constrain_finalize(const int* tok, const float* lp, const int* fin, const int* dead, const int* first, int Btot, int T,
                                   const int* steps_dev, int w0, int nw, int b0, int64_t* predict, float* logprob, int* dead_end,
                                   int* open_end, int* seq_of_row, hipStream_t st);

// Sequence-constrained sampled decode (ff_constrain_seq.hip): the sequence-constrained step's operands and
// the draw's; R draws per wireframe in the sequence-sampled decode's layout, each with the sequence-constrained decode's state.
int ff_pointer_sequence_constrained_sample_sync(const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& st,
                                                int tok_sep, int tok_eos, const ff_lookahead_io* ahead, const ff_sample_draw_io& draw,
                                                ff_stream_t stream);
int ff_sequence_constrain_sample_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int* row_id,
                                      int Bc, int R, int w0, int L, int sos, hipStream_t st);
int ff_sequence_constrain_sample_finalize(const int* tok, const float* lp, const int* fin, const int* dead, const int* first, int Btot,
                                          int T, const int* steps_dev, int R, int w0, int nw, int b0, int64_t* samples, float* logprob,
                                          float* scores, int* dead_end, int* open_end, int64_t* predict, float* predict_logprob,
                                          int* predict_dead_end, int* predict_open_end, int* seq_of_row, hipStream_t st);

// Sequence-constrained beam decode (ff_constrain_seq.hip): `step` supplies the rule's and the beams' operands, io
// the common ones (io.rows = groups * width); W beams per wireframe in the sequence beam decode's layout.
// `ahead`: the closure look-ahead's tables and budget, null = the plain launch.
int ff_beam_sequence_constrained_select_sync(const ff_step_io& io, const ff_beam_sequence_constrained_step* step,
                                             const ff_lookahead_io* ahead, ff_stream_t stream);
int ff_sequence_constrain_beam_init(int* tok, float* score, int* fin, int* dead, int* open, int* parent, int* first, int* prev,
                                    unsigned* visited, int Bc, int W, int L, int sos, hipStream_t st);
int ff_sequence_constrain_beam_finalize(const int* tok, const int* parent, const float* score, const int* fin, const int* dead,
                                        const int* open, int Btot, int T, const int* steps_dev, int W, int w0, int nw, int b0,
                                        int64_t* beams, float* scores, int* finished, int* beam_dead_end, int* beam_open_end,
                                        int64_t* predict, int* dead_end, int* open_end, int* seq_of_row, hipStream_t st);

// Constrained sampled decode (ff_constrain_sample.hip): the constrained step's operands and the draw's; R draws per
// anchor in the sampled decode's layout, each with the constrained decode's state.
int ff_pointer_constrained_sample_sync(const char* op, const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& st,
                                       const ff_lookahead_io* ahead, const ff_sample_draw_io& draw, ff_stream_t stream);
int ff_constrain_sample_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int* row_id, int Bc,
                             int Fc, int R, int f0, int w0, int F, const int* num_input, int pad_tok, int term_lo, int term_hi,
                             int ntok, const unsigned* follows, int L, hipStream_t st);
int ff_constrain_sample_finalize(const int* tok, const float* lp, const int* fin, const int* dead, int Btot, int T,
                                 const int* steps_dev, const int* num_input, int dedup, int F, int R, int w0, int nw, int Fc, int f0,
                                 int b0, int64_t* samples, float* logprob, float* scores, int* dead_end, int64_t* predict,
                                 float* predict_logprob, int* predict_dead_end, int* seq_of_row, hipStream_t st);

// Constrained beam decode: `step` supplies the rule's and the beams' operands, io the common ones (io.rows = groups * width);
// its beams, scores and predict are packed by ff_beam_finalize.  ahead (or null): the closure look-ahead of every beam's row, or
// with `exact` the exact one; `op` words the errors.
int ff_beam_constrained_select_sync(const char* op, const ff_step_io& io, const ff_beam_constrained_step* step,
                                    const ff_lookahead_io* ahead, ff_stream_t stream);
int ff_constrain_beam_init(int* tok, float* score, int* fin, int* dead, int* parent, int* first, int* prev, unsigned* visited, int Bc,
                           int Fc, int W, int f0, const int* num_input, int pad_tok, int term_lo, int term_hi, int ntok,
                           const unsigned* follows, int L, hipStream_t st);
int ff_constrain_beam_dead(const int* dead, int Btot, const int* steps_dev, const int* num_input, int dedup, int F, int W, int w0,
                           int nw, int Fc, int f0, int b0, int* dead_end, hipStream_t st);

// out[c, r] = in[r, c] for an [rows, cols] fp32 matrix (ff_rowops.hip; the engine's per-call transposes)
int ff_transpose(const float* in, int ld_in, int rows, int cols, float* out, int ld_out, hipStream_t st);

// The per-call tables of the folded last-layer self-attention (ff_attention_fold.hip), ONE block of
// ff_attention_fold_table_floats(E, H, T) floats: kt [H, E + T, 64], the W operand of the head-batched qt | c product, then
// ob [E], the self-attention out-projection's bias with the folded v bias carried through.  Weights only: one launch per call.
size_t ff_attention_fold_table_floats(int E, int H, int T);
int ff_attention_fold_tables(const float* ln1_w, const float* ln1_b, const float* ln1_pos, int pos_rows, const float* out_w,
                             const float* out_b, int E, int H, int T, float* kt, float* ob, hipStream_t st);

// partial-tile workspace of the 3 x bf16 kernel for (current device, stream): allocate now (ff_gemm_x3.hip).  Called across
// translation units only, so hidden: the library exports exactly the ff_* symbols of include/faceformer_hip.h
extern "C" __attribute__((visibility("hidden"))) int ff_x3_prepare_stream(hipStream_t st);
// ... and the same area as scratch memory for another kernel of that stream (at most 24 MB)
int ff_stream_scratch(hipStream_t st, size_t bytes, float** out);

// ---- device helpers --------------------------------------------------------------------------
__device__ __forceinline__ float ff_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, FF_WAVE);
  return v;
}
__device__ __forceinline__ float ff_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, FF_WAVE));
  return v;
}

// Exchange between the two 32-lane halves of a wave without the LDS crossbar: v_permlane32_swap leaves (lower half's value, upper
// half's value) in every lane; `__shfl_xor(v, 32)` is a ds_bpermute round trip (>100 cycles, and a lgkmcnt event in the middle of
// hand-counted LDS reads).  Bitwise the results of v + __shfl_xor(v, 32) / fmaxf(v, __shfl_xor(v, 32)) (both are commutative).
__device__ __forceinline__ float ff_halves_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float ff_halves_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// Bijective XCD-aware remap of a linear block id: blocks are dispatched round-robin over the 8
// XCDs (block b -> XCD b % 8); give every XCD a contiguous range of logical ids so that
// neighbouring tiles (which share operand panels) hit the same L2.  Speed only, never correctness.
__device__ __forceinline__ int ff_xcd_remap(int bid, int nblocks) {
  const int NX = 8;
  int xcd = bid % NX, idx = bid / NX;
  int q = nblocks / NX, r = nblocks % NX;
  int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}
