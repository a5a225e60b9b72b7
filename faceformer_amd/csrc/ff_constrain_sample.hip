// Sampling over the loop-constrained pointer decode (opt-in, parallel variant): one step's constrained draw of every
// sequence, and the start state / output packing of a constrained sampled decode.
//
// Nothing of the rule or of the draw is stated here: the byte row of a sequence's constraint mask in its three compile-time
// forms (ff_loop_write_row<FORM>), the state update (ff_loop_advance, ff_loop_start) and the draw (ff_sample_draw) are
// ff_select.h's, the masked reduction with an extra mask (ff_pointer_mask_reduce<true>) is ff_device.h's.  This file is the
// launch that runs them on one row in one wave.
//
// pointer_constrained_sample_kernel<FORM>: pointer_constrained_form_kernel's layout -- one wavefront per sequence, four per
// block, wireframe w = b / spg.  A finished sequence appends token 0 and keeps its state.  Every other one, in order:
//   1. reads (fin, first, prev);
//   2. writes the byte row of ITS constraint mask (the dead-end vote included: on a dead end the terminators are re-opened);
//   3. masks and reduces its logit row with that row as the extra mask: maximum m, argmax, sum exp(l - m);
//   4. draws from the masked row -- top-k and top-p therefore act on the constrained row, and on a dead end the draw is among
//      the re-opened terminators;
//   5. advances (first, prev) and sets the token's bit in the sequence's visited words when the token is an edge;
//   6. lane 0 stores token, log-probability ((l[tok] - m) - log sum over the constrained row, saturated at -FLT_MAX: the
//      model's distribution renormalised over the keys the rule allows), finished, dead end, first and prev;
//   7. the wave appends memory[w, token] through ff_pointer_append_row, so the decode keeps FF_L0_FOLD;
//   8. stop counter: pointer_sample_kernel's scheme.
// Every loop over keys keeps lane = key mod 64: the reduction reads back only bytes its own lane wrote, the draw's re-reads only
// logits its own lane masked.  No barrier, no LDS beyond the four counter words, no scratch.
// With temperature 0 the launch is pointer_constrained_form_kernel<FORM>'s selection: the same reduction, the argmax, and
// (m - m) - logf(lsum) = -logf(lsum), bit for bit.  With both flag bits clear the byte row is zero and it is pointer_sample_kernel's.
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"
#include "ff_select.h"

namespace {

struct ConstrainSampleArgs {
  PointerArgs p;                 // logits / masks / memory / next rows / counters of the B launch rows; p.extra = rows
  unsigned char* rows;           // [B, S] out: the constraint byte row of every unfinished sequence (1 = masked)
  const unsigned* follows;       // [wireframes, L, fw] bits or null
  int L, fw;                     // edges per wireframe (S - ntok), words per row ceil(L / 32)
  int flags, ntok;
  const int *fin_in, *first_in, *prev_in;   // [B] the state before this step (first / prev: -1 = none)
  unsigned* visited;             // [B, fw] in / out: the edges of the prefix
  int *fin_out, *first_out, *prev_out, *dead_out;   // [B] out
  int* tok; float* logprob;      // [B] out
  const unsigned char* close_dist;   // FF_LOOP_AHEAD only: [wireframes, L, L] bytes
  const unsigned char* cycle_len;    // FF_LOOP_AHEAD, FF_LOOP_EXACT: [wireframes, L] bytes
  int budget;                        // FF_LOOP_AHEAD, FF_LOOP_EXACT
  const float* uniforms;         // [num_uniforms] this step's draws
  const int* row_id;             // [B] the draw every launch row reads (null: b); clamped into [0, num_uniforms)
  int num_uniforms;
  float temperature; int top_k; float top_p;
};

template <int FORM>
__global__ __launch_bounds__(256) void pointer_constrained_sample_kernel(ConstrainSampleArgs a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const float FILL = -FLT_MAX;
  int nge = 0;
  if (b < pa.B) {   // (wave-uniform)
    const int ntok = a.ntok;
    const int was_fin = ff_ld4i(a.fin_in + b);
    int first = ff_loop_edge(ff_ld4i(a.first_in + b), a.L), prev = ff_loop_edge(ff_ld4i(a.prev_in + b), a.L);
    int tok = 0, dead = 0;
    float lp = 0.f;
    if (!was_fin) {
      const int w = b / pa.spg;
      int kv = pa.S;
      if (pa.kv_len) { const int k = ff_ldw(pa.kv_len + w); kv = k < kv ? k : kv; }
      const unsigned char* mrow = pa.mask ? pa.mask + (size_t)w * pa.S : nullptr;
      const FFLoopRule rule{a.follows, a.L, a.fw, a.flags, ntok, a.close_dist, a.cycle_len, a.budget};
      dead = ff_loop_write_row<FORM>(pa, rule, lane, w, kv, mrow, first, prev, a.visited + (size_t)b * a.fw, a.rows + (size_t)b * pa.S) ? 1 : 0;
      float m, b2, lsum;
      int i1;
      ff_pointer_mask_reduce<true>(pa, b, lane, &m, &b2, &i1, &lsum);
      const float* lrow = pa.logits + (size_t)b * pa.ldlogits;
      tok = ff_sample_draw(lrow, pa.S, lane, m, i1, a.temperature, a.top_k, a.top_p, a.uniforms, a.row_id, a.num_uniforms, b);
      // the masked l[tok] was stored by lane tok % 64 a moment ago: that lane reads its own store back and broadcasts it
      const int owner = tok & 63;
      const float mine = lane == owner ? ff_ld4(lrow + tok) : 0.f;
      const float lg = __shfl(mine, owner, FF_WAVE);
      // saturates: no -inf, no NaN (lsum >= 1, every term finite).  Temperature 0 selects the maximum, l[tok] = m: the constrained
      // greedy launch's own expression there, so that the two agree in the sign of a zero as well
      lp = a.temperature == 0.f ? -logf(lsum) : fmaxf((lg - m) - logf(lsum), FILL);
      if (tok >= ntok) {
        const int e = tok - ntok;
        nge = 1;
        ff_loop_advance(a.follows, w, a.L, a.fw, e, &first, &prev);
        if (lane == 0) a.visited[(size_t)b * a.fw + (e >> 5)] |= 1u << (e & 31);
      }
    }
    if (lane == 0) {
      ff_st4i(a.tok + b, tok);
      ff_st4(a.logprob + b, lp);
      ff_st4i(a.fin_out + b, (was_fin || dead || (tok >= pa.term_lo && tok < pa.term_hi)) ? 1 : 0);
      ff_st4i(a.dead_out + b, dead);
      ff_st4i(a.first_out + b, first);
      ff_st4i(a.prev_out + b, prev);
    }
    if (pa.next_rows) ff_pointer_append_row(pa, b / pa.spg, b, tok, lane);
  }
  ff_pointer_count_waves(pa, pa.B, nge);
}

// ---- engine side: start state and output packing of a constrained sampled decode (ff_engine.hip) --------------------------------
// Start state of one micro-batch of Bc = nw * Fc * R sequences (Fc anchors per wireframe, compact anchors [f0, f0 + Fc)): every
// draw of an anchor holds the anchor's start token, log-probability 0, no dead end and the rule's state after column 0 -- what
// constrain_init_kernel writes per sequence -- and row_id, the output row (w * F + f) * R + k whose uniforms it reads --
// what sample_init_kernel writes.  A start token in the terminator range finishes the draw at position 0 (the padding anchors).
__global__ void constrain_sample_init_kernel(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited,
                                             int* row_id, int Bc, int Fc, int R, int f0, int w0, int F, const int* num_input,
                                             int pad_tok, int term_lo, int term_hi, int ntok, const unsigned* follows, int L, int fw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  const int k = i % R, a = i / R, wl = a / Fc, f = f0 + a % Fc;
  int done;
  const int t = ff_start_token(f, num_input[wl], pad_tok, term_lo, term_hi, &done);
  tok[i] = t;
  lp[i] = 0.f;
  fin[i] = done;
  dead[i] = 0;
  row_id[i] = ((w0 + wl) * F + (f < F ? f : F - 1)) * R + k;
  int fi, pv;
  ff_loop_start(t, ntok, follows, wl, L, fw, visited + (size_t)i * fw, &fi, &pv);
  first[i] = fi;
  prev[i] = pv;
}

// samples[(w, fo, k), :], logprob (same layout), scores and dead_end[(w, fo, k)] from the per-step records (tok, lp, fin, dead:
// [T, Btot], row s = the state after s steps), and predict[(w, fo), :], predict_logprob (same layout) and predict_dead_end[(w, fo)]
// = draw 0.  Position j is kept when j <= the stop step and the draw was not finished before it: last = min(finish position,
// stop step); rows behind the stop step are never looked at, so the result does not depend on when the host saw the stop.
// scores: the kept log-probabilities added in ascending position (fp64 accumulator, rounded once, saturated at -FLT_MAX).
// Rows fo >= num_input[w] of a de-duplicated decode read the one padding-anchor group.
__global__ void constrain_sample_finalize_kernel(const int* __restrict__ tok, const float* __restrict__ lp, const int* __restrict__ fin,
                                                 const int* __restrict__ dead, int Btot, int T, const int* __restrict__ steps_p,
                                                 const int* __restrict__ num_input, int dedup, int F, int R, int w0, int nw, int Fc,
                                                 int f0, int b0, int64_t* __restrict__ samples, float* __restrict__ logprob,
                                                 float* __restrict__ scores, int* __restrict__ dead_end, int64_t* __restrict__ predict,
                                                 float* __restrict__ predict_logprob, int* __restrict__ predict_dead_end,
                                                 int* __restrict__ seq_of_row) {
  const int steps = *steps_p;
  const int total = nw * F * R;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int k = i % R, fo = (i / R) % F, wl = i / (R * F);
    int a;
    if (!ff_compact_seq(num_input, dedup, w0, wl, fo, Fc, f0, &a)) continue;
    const int seq = b0 + a * R + k;
    const size_t anchor = (size_t)(w0 + wl) * F + fo, row = anchor * R + k;
    int64_t* out = samples + row * T;
    float* olp = logprob + row * T;
    int64_t* pred = k == 0 ? predict + anchor * T : nullptr;
    float* plp = (k == 0 && predict_logprob) ? predict_logprob + anchor * T : nullptr;
    double sum = 0.0;
    int de = 0;
    bool done = false;   // finished before position j
    for (int j = 0; j < T; ++j) {
      const bool in = j <= steps && !done;
      const int v = in ? tok[(size_t)j * Btot + seq] : 0;
      const float l = (in && j >= 1) ? lp[(size_t)j * Btot + seq] : 0.f;
      out[j] = v;
      olp[j] = l;
      if (pred) pred[j] = v;
      if (plp) plp[j] = l;
      sum += (double)l;
      if (in) { de |= dead[(size_t)j * Btot + seq]; done = fin[(size_t)j * Btot + seq] != 0; }
    }
    scores[row] = (float)fmax(sum, -(double)FLT_MAX);
    dead_end[row] = de;
    if (k == 0 && predict_dead_end) predict_dead_end[anchor] = de;
    if (seq_of_row) seq_of_row[row] = seq;
  }
}

}  // namespace

// The one launch behind ff_pointer_constrained_sample and the engine's constrained sampled step: ff_pointer_constrained_sync's
// checks (ff_step_args, ff_loop_rule_check, ff_lookahead_check) and ff_pointer_sample_sync's (ff_sample_draw_check).
int ff_pointer_constrained_sample_sync(const char* op, const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& s,
                                       const ff_lookahead_io* ahead, const ff_sample_draw_io& d, ff_stream_t stream) {
  const int B = io.rows, S = io.S;
  if (B == 0) return FF_OK;
  FF_CHECK_ARG(B > 0 && S > 0 && io.rows_per_wireframe > 0, "%s: bad sizes B=%d S=%d", op, B, S);
  ConstrainSampleArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(ff_step_args(&a.p, op, true, io));
  FF_RETURN_IF(ff_loop_rule_check(op, rule, S, io.term_lo, io.term_hi));
  FF_CHECK_ARG(s.fin_in && s.first_in && s.prev_in && s.visited && s.mask_rows && s.next_tok && s.logprob && s.fin_out && s.dead_end &&
                   s.first_out && s.prev_out, "%s: null pointer", op);
  FF_RETURN_IF(ff_sample_draw_check(op, d, B));
  if (ahead) {
    FF_RETURN_IF(ff_lookahead_check(op, rule, S, *ahead));
    a.close_dist = ahead->exact ? nullptr : ahead->close_dist; a.cycle_len = ahead->cycle_len; a.budget = ahead->budget;
  }
  a.p.extra = s.mask_rows; a.p.ldextra = S;
  a.rows = s.mask_rows; a.follows = rule.follows; a.L = rule.L; a.fw = (rule.L + 31) >> 5; a.flags = rule.flags; a.ntok = rule.ntok;
  a.fin_in = s.fin_in; a.first_in = s.first_in; a.prev_in = s.prev_in; a.visited = s.visited;
  a.fin_out = s.fin_out; a.first_out = s.first_out; a.prev_out = s.prev_out; a.dead_out = s.dead_end;
  a.tok = s.next_tok; a.logprob = s.logprob;
  a.uniforms = d.uniforms; a.num_uniforms = d.num_uniforms; a.row_id = d.row_id;
  a.temperature = d.temperature; a.top_k = d.top_k; a.top_p = d.top_p;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)B * S * 16.0, st);
  const int form = !ahead ? FF_LOOP_PLAIN : (ahead->exact ? FF_LOOP_EXACT : FF_LOOP_AHEAD);
  return ff_dispatch<FF_LOOP_AHEAD, FF_LOOP_EXACT, FF_LOOP_PLAIN>(form, [&](auto f) -> int {
    hipLaunchKernelGGL(pointer_constrained_sample_kernel<decltype(f)::value>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
    FF_CHECK_LAUNCH();
    return FF_OK;
  });
}

extern "C" int ff_pointer_constrained_sample(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                             int seqs_per_group, const unsigned* follows, int L, int flags, int ntok, int term_lo,
                                             int term_hi, const int* fin_in, const int* first_in, const int* prev_in,
                                             unsigned* visited, unsigned char* mask_rows, int* next_tok, float* logprob,
                                             int* fin_out, int* dead_end, int* first_out, int* prev_out, const float* memory, int E,
                                             float* next_rows, int ldnext, float* next_stats, int* count_ge, const float* uniforms,
                                             int num_uniforms, const int* row_id, float temperature, int top_k, float top_p,
                                             int lookahead, const unsigned char* close_dist, const unsigned char* cycle_len,
                                             int budget, ff_stream_t stream) {
  const char* op = "ff_pointer_constrained_sample";
  FF_CHECK_ARG(lookahead >= 0 && lookahead <= 2, "%s: lookahead=%d must be 0 (none), 1 (look-ahead) or 2 (exact)", op, lookahead);
  const ff_lookahead_io ahead{lookahead == 1 ? close_dist : nullptr, cycle_len, budget, lookahead == 2 ? 1 : 0};
  return ff_pointer_constrained_sample_sync(
      op,
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, term_lo, term_hi, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_ge, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      lookahead ? &ahead : nullptr, ff_sample_draw_io{uniforms, num_uniforms, row_id, temperature, top_k, top_p}, stream);
}

int ff_constrain_sample_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int* row_id, int Bc,
                             int Fc, int R, int f0, int w0, int F, const int* num_input, int pad_tok, int term_lo, int term_hi,
                             int ntok, const unsigned* follows, int L, hipStream_t st) {
  hipLaunchKernelGGL(constrain_sample_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, lp, fin, dead, first, prev, visited,
                     row_id, Bc, Fc, R, f0, w0, F, num_input, pad_tok, term_lo, term_hi, ntok, follows, L, (L + 31) >> 5);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_constrain_sample_finalize(const int* tok, const float* lp, const int* fin, const int* dead, int Btot, int T,
                                 const int* steps_dev, const int* num_input, int dedup, int F, int R, int w0, int nw, int Fc, int f0,
                                 int b0, int64_t* samples, float* logprob, float* scores, int* dead_end, int64_t* predict,
                                 float* predict_logprob, int* predict_dead_end, int* seq_of_row, hipStream_t st) {
  const int total = nw * F * R;
  hipLaunchKernelGGL(constrain_sample_finalize_kernel, dim3(ff_cdiv(total, 256) < 1024 ? ff_cdiv(total, 256) : 1024), dim3(256), 0, st,
                     tok, lp, fin, dead, Btot, T, steps_dev, num_input, dedup, F, R, w0, nw, Fc, f0, b0, samples, logprob, scores,
                     dead_end, predict, predict_logprob, predict_dead_end, seq_of_row);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
