// Temperature / top-k / top-p sampling over the pointer head (opt-in, parallel variant): one step's draw of every
// sequence, and the start state / output packing of a sampled decode.
//
// pointer_sample_kernel: one wavefront per sequence, four per block, as pointer_reduce_kernel.  A finished sequence appends
// token 0 and draws nothing.  Every other one masks and reduces its raw logit row exactly as the greedy launch does
// (ff_pointer_mask_reduce<true>, ff_device.h: row maximum m, argmax with torch's tie rule, sum exp(l - m)); a row without a live
// key takes token 0, temperature 0 takes the argmax.  Otherwise (ff_sample_draw, ff_select.h: one copy, shared with the
// constrained sampling launch of ff_constrain_sample.hip), with w[s] = exp((l[s] - m) / temperature) over the live keys:
//   top-k   v_K, the K-th largest logit, by bisection on the order-preserving integer image of the fp32 value: 32 rounds, each
//           a count of the keys at or above the candidate (one ballot per 64 keys).  Exact; ties at v_K are all kept.
//   top-p   theta, the largest kept logit at which the mass of the keys >= theta reaches P * (mass of the kept keys), by the same
//           bisection.  A mass is the lane's terms added in key order, then a butterfly: a fixed tree of fp32 additions of
//           non-negative terms, hence monotone in the key set, so the bisection is well defined and the same on every run.
//   draw    inclusive prefix sums c[s] of w over the kept keys in ascending key index: a wave scan per 64 consecutive keys plus
//           the carried total of the chunks before (at most ceil(S / 64) + 6 dependent additions); Z is the last carry.  The
//           scan runs twice -- once for Z, once more for the ballot on c[s] > u * Z -- with the same operations in the same
//           order.  No key crosses: the last kept key.
// The row is re-read from memory in every round (each lane reads the keys it masked itself): no LDS beyond the four counter
// words, no scratch, whatever S and K are.  Lane 0 stores token, log-probability (under the MODEL, (l[tok] - m) - log sum,
// saturated at -FLT_MAX) and the finished flag; the wave appends memory[w, token] through ff_pointer_append_row, so the row
// carries its LayerNorm segment statistics and a sampled decode keeps FF_L0_FOLD.  Stop counter: beam_select_kernel's scheme.
//
// The uniform of a row is uniforms[row_id[b]], clamped into [0, 1 - 2^-24]: a draw is keyed by the OUTPUT row, never by the
// sequence's place in a launch.  There is no random number generator in device code.
//
// Sequence form (opt-in, single-sequence variant): pointer_sample_kernel<true>, the same launch but for what a wave
// adds to the stop counter -- 1 when its row is UNFINISHED AFTER this step (not finished before it, token outside the terminator
// range), not "selected a token >= ge_bound": all draws of a single-sequence decode can select SEP in one step, so the parallel
// rule would stop them.  A compile-time form: pointer_sample_kernel<false> is the launch the parallel decode always made.
// sequence_sample_init_kernel is its start state (every draw at SOS, unfinished, row_id = w * R + k: no anchors, no padding
// groups); the packing is sample_finalize_kernel with F = 1.
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"
#include "ff_select.h"

namespace {

struct SampleArgs {
  PointerArgs p;             // logits / masks / memory / next rows / counters of the B launch rows
  const float* uniforms;     // [num_uniforms] this step's draws
  const int* row_id;         // [B] the draw every launch row reads (null: b); clamped into [0, num_uniforms)
  int num_uniforms;
  const int* fin_in;         // [B] nonzero: finished before this step (null: none)
  int* fin_out;              // [B] out
  int* tok; float* logprob;  // [B] out
  float temperature; int top_k; float top_p;
};

template <bool SEQ>
__global__ __launch_bounds__(256) void pointer_sample_kernel(SampleArgs a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const float FILL = -FLT_MAX;
  int nge = 0;
  if (b < pa.B) {   // (wave-uniform)
    const int S = pa.S;
    const int was_fin = a.fin_in ? ff_ld4i(a.fin_in + b) : 0;
    int tok = 0;
    float lp = 0.f;
    if (!was_fin) {
      float m, b2, lsum;
      int i1;
      ff_pointer_mask_reduce<true>(pa, b, lane, &m, &b2, &i1, &lsum);
      const float* lrow = pa.logits + (size_t)b * pa.ldlogits;
      tok = ff_sample_draw(lrow, S, lane, m, i1, a.temperature, a.top_k, a.top_p, a.uniforms, a.row_id, a.num_uniforms, b);
      // the masked l[tok] was stored by lane tok % 64 a moment ago: that lane reads its own store back and broadcasts it
      const int owner = tok & 63;
      const float mine = lane == owner ? ff_ld4(lrow + tok) : 0.f;
      const float lg = __shfl(mine, owner, FF_WAVE);
      lp = fmaxf((lg - m) - logf(lsum), FILL);   // saturates: no -inf, no NaN (lsum >= 1, every term finite)
      if (SEQ) nge = (tok >= pa.term_lo && tok < pa.term_hi) ? 0 : 1;   // unfinished after this step
      else nge = tok >= pa.ge_bound ? 1 : 0;
    }
    if (lane == 0) {
      ff_st4i(a.tok + b, tok);
      ff_st4(a.logprob + b, lp);
      ff_st4i(a.fin_out + b, (was_fin || (tok >= pa.term_lo && tok < pa.term_hi)) ? 1 : 0);
    }
    if (pa.next_rows) ff_pointer_append_row(pa, b / pa.spg, b, tok, lane);
  }
  ff_pointer_count_waves(pa, pa.B, nge);
}

// ---- engine side: start state and output packing of a sampled decode (ff_engine.hip) ---------------------------------------------
// Start state of one micro-batch of Bc = nw * Fc * R sequences (Fc anchors per wireframe, compact anchors [f0, f0 + Fc)): every
// sample of an anchor holds the anchor's start token (model_para.py:201-205), log-probability 0; a start token in the terminator
// range finishes the sample at position 0 (the padding anchors).  row_id: the output row (w * F + f) * R + k whose draws the
// sequence reads -- whatever micro-batch or compact place it decodes in.
__global__ void sample_init_kernel(int* tok, float* lp, int* fin, int* row_id, int Bc, int Fc, int R, int f0, int w0, int F,
                                   const int* num_input, int pad_tok, int term_lo, int term_hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  const int k = i % R, a = i / R, wl = a / Fc, f = f0 + a % Fc;
  int done;
  tok[i] = ff_start_token(f, num_input[wl], pad_tok, term_lo, term_hi, &done);
  lp[i] = 0.f;
  fin[i] = done;
  row_id[i] = ((w0 + wl) * F + (f < F ? f : F - 1)) * R + k;
}

// Start state of one micro-batch of the sequence form: Bc = nw * R draws, draw k of the chunk's wl-th wireframe at i = wl * R + k.
// Every draw starts from SOS (model.py:191) with log-probability 0, unfinished; row_id: its output row (w0 + wl) * R + k.
__global__ void sequence_sample_init_kernel(int* tok, float* lp, int* fin, int* row_id, int Bc, int R, int w0, int sos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  tok[i] = sos;
  lp[i] = 0.f;
  fin[i] = 0;
  row_id[i] = w0 * R + i;
}

// samples[(w, fo, k), :], logprob (same layout), scores and predict[(w, fo), :] = sample 0, from the per-step records (tok, lp,
// fin: [T, Btot], row s = the state after s steps).  Position j is kept when j <= the stop step and the sample was not finished
// before it: last = min(finish position, stop step); rows behind the stop step are never looked at, so the result does not
// depend on when the host saw the stop.  scores: the kept log-probabilities added in ascending position (fp64 accumulator,
// rounded once, saturated at -FLT_MAX).  Rows fo >= num_input[w] of a de-duplicated decode read the one padding-anchor group.
__global__ void sample_finalize_kernel(const int* __restrict__ tok, const float* __restrict__ lp, const int* __restrict__ fin,
                                       int Btot, int T, const int* __restrict__ steps_p, const int* __restrict__ num_input,
                                       int dedup, int F, int R, int w0, int nw, int Fc, int f0, int b0,
                                       int64_t* __restrict__ samples, float* __restrict__ logprob, float* __restrict__ scores,
                                       int64_t* __restrict__ predict, int* __restrict__ seq_of_row) {
  const int steps = *steps_p;
  const int total = nw * F * R;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int k = i % R, fo = (i / R) % F, wl = i / (R * F);
    int a;
    if (!ff_compact_seq(num_input, dedup, w0, wl, fo, Fc, f0, &a)) continue;
    const int seq = b0 + a * R + k;
    const size_t row = ((size_t)(w0 + wl) * F + fo) * R + k;
    int64_t* out = samples + row * T;
    float* olp = logprob + row * T;
    int64_t* pred = k == 0 ? predict + ((size_t)(w0 + wl) * F + fo) * T : nullptr;
    double sum = 0.0;
    bool done = false;   // finished before position j
    for (int j = 0; j < T; ++j) {
      const bool in = j <= steps && !done;
      const int v = in ? tok[(size_t)j * Btot + seq] : 0;
      const float l = (in && j >= 1) ? lp[(size_t)j * Btot + seq] : 0.f;
      out[j] = v;
      olp[j] = l;
      if (pred) pred[j] = v;
      sum += (double)l;
      if (in) done = fin[(size_t)j * Btot + seq] != 0;
    }
    scores[row] = (float)fmax(sum, -(double)FLT_MAX);
    if (seq_of_row) seq_of_row[row] = seq;
  }
}

}  // namespace

// What a draw adds to a step's checks, for operator `op`: the uniforms and how the B launch rows index them, the parameters' ranges.
int ff_sample_draw_check(const char* op, const ff_sample_draw_io& d, int B) {
  FF_CHECK_ARG(d.uniforms && d.num_uniforms > 0, "%s: null pointer", op);
  FF_CHECK_ARG(d.row_id || d.num_uniforms >= B, "%s: %d uniforms for %d rows without a row_id", op, d.num_uniforms, B);
  FF_CHECK_ARG(d.temperature >= 0.f && d.temperature <= FLT_MAX && d.top_k >= 0 && d.top_p > 0.f && d.top_p <= 1.f,
               "%s: temperature=%g must be finite and >= 0, top_k=%d >= 0, top_p=%g in (0, 1]", op, (double)d.temperature, d.top_k,
               (double)d.top_p);
  return FF_OK;
}

int ff_pointer_sample_sync(const ff_step_io& io, const float* uniforms, int num_uniforms, const int* row_id, const int* fin_in,
                           float temperature, int top_k, float top_p, int* next_tok, float* logprob, int* fin_out, ff_stream_t stream,
                           bool sequence_form) {
  const char* op = sequence_form ? "ff_pointer_sequence_sample" : "ff_pointer_sample";
  const int B = io.rows, S = io.S;
  if (B == 0) return FF_OK;
  FF_CHECK_ARG(B > 0 && S > 0 && io.rows_per_wireframe > 0, "%s: bad sizes B=%d S=%d", op, B, S);
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(ff_step_args(&a.p, op, true, io));
  FF_CHECK_ARG(next_tok && logprob && fin_out, "%s: null pointer", op);
  FF_RETURN_IF(ff_sample_draw_check(op, ff_sample_draw_io{uniforms, num_uniforms, row_id, temperature, top_k, top_p}, B));
  a.uniforms = uniforms; a.num_uniforms = num_uniforms; a.row_id = row_id; a.fin_in = fin_in; a.fin_out = fin_out;
  a.tok = next_tok; a.logprob = logprob;
  a.temperature = temperature; a.top_k = top_k; a.top_p = top_p;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)B * S * 12.0, st);
  if (sequence_form) hipLaunchKernelGGL(pointer_sample_kernel<true>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(pointer_sample_kernel<false>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" int ff_pointer_sample(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                 int seqs_per_group, const float* uniforms, int num_uniforms, const int* row_id, const int* fin_in,
                                 float temperature, int top_k, float top_p, int term_lo, int term_hi, int* next_tok,
                                 float* logprob, int* fin_out, const float* memory, int E, float* next_rows, int ldnext,
                                 float* next_stats, int* count_ge, int ge_bound, ff_stream_t stream) {
  return ff_pointer_sample_sync(ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, term_lo, term_hi, ge_bound, memory, E,
                                           next_rows, ldnext, next_stats, count_ge, nullptr, nullptr},
                                uniforms, num_uniforms, row_id, fin_in, temperature, top_k, top_p, next_tok, logprob, fin_out, stream);
}

// The sequence form of the step (single-sequence variant): ff_pointer_sample's arguments without ge_bound; count_unfinished +=
// the number of rows unfinished after the step.
extern "C" int ff_pointer_sequence_sample(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                          int seqs_per_group, const float* uniforms, int num_uniforms, const int* row_id,
                                          const int* fin_in, float temperature, int top_k, float top_p, int term_lo, int term_hi,
                                          int* next_tok, float* logprob, int* fin_out, const float* memory, int E, float* next_rows,
                                          int ldnext, float* next_stats, int* count_unfinished, ff_stream_t stream) {
  FF_CHECK_ARG(term_lo < term_hi, "ff_pointer_sequence_sample: empty terminator range [%d, %d)", term_lo, term_hi);
  return ff_pointer_sample_sync(ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, term_lo, term_hi, 0, memory, E,
                                           next_rows, ldnext, next_stats, count_unfinished, nullptr, nullptr},
                                uniforms, num_uniforms, row_id, fin_in, temperature, top_k, top_p, next_tok, logprob, fin_out, stream,
                                true);
}

int ff_sequence_sample_init(int* tok, float* lp, int* fin, int* row_id, int Bc, int R, int w0, int sos, hipStream_t st) {
  hipLaunchKernelGGL(sequence_sample_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, lp, fin, row_id, Bc, R, w0, sos);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_sample_init(int* tok, float* lp, int* fin, int* row_id, int Bc, int Fc, int R, int f0, int w0, int F, const int* num_input,
                   int pad_tok, int term_lo, int term_hi, hipStream_t st) {
  hipLaunchKernelGGL(sample_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, lp, fin, row_id, Bc, Fc, R, f0, w0, F,
                     num_input, pad_tok, term_lo, term_hi);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_sample_finalize(const int* tok, const float* lp, const int* fin, int Btot, int T, const int* steps_dev, const int* num_input,
                       int dedup, int F, int R, int w0, int nw, int Fc, int f0, int b0, int64_t* samples, float* logprob,
                       float* scores, int64_t* predict, int* seq_of_row, hipStream_t st) {
  const int total = nw * F * R;
  hipLaunchKernelGGL(sample_finalize_kernel, dim3(ff_cdiv(total, 256) < 1024 ? ff_cdiv(total, 256) : 1024), dim3(256), 0, st, tok,
                     lp, fin, Btot, T, steps_dev, num_input, dedup, F, R, w0, nw, Fc, f0, b0, samples, logprob, scores, predict,
                     seq_of_row);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
