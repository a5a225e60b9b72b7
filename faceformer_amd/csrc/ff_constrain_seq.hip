// Loop-constrained greedy selection for the single-sequence model (opt-in, FF_SEQ2SEQ): one step's constrained
// selection of every sequence, and the start state / output packing of that decode.
//
// One row carries every face of a wireframe, split at SEP and ended by EOS, so the loop rule of DESIGN.md 16 runs per FACE: SEP
// ends the current face and resets (first, prev) -- and the visited edges, unless FF_CONSTRAIN_ONCE keeps them for the whole
// row -- and EOS alone finishes the row.  A dead end abandons the face, not the row: SEP alone is re-opened there.
// include/faceformer_hip.h states the rule on tokens.
//
// The rule's device code is ff_select.h's, the one copy the parallel kernels share.  pointer_sequence_constrained_kernel: one
// wavefront per sequence, four per block, as pointer_constrained_kernel.  A finished sequence appends token 0 and keeps its
// state.  Every other one writes its byte row with ff_loop_write_row<FF_LOOP_PLAIN> called with the terminator range
// [SEP, SEP + 1) -- open: every special token masked, SEP re-opened on a dead end; closed: every special token but SEP masked --
// and then the lanes that own the keys SEP and EOS (lane = key mod 64) apply the two fix-ups of the closed state to their own
// bytes: EOS is opened, SEP is masked while the current face has no edge (prev == none).  Every lane still reads back only
// bytes it wrote itself, so ff_pointer_mask_reduce<true> follows without a barrier.  Lane 0 stores token, log-probability, the
// flags and the next (first, prev) and sets the token's bit in the visited words; on SEP the wave clears its visited words
// unless ONCE; the wave appends memory[w, token] through ff_pointer_append_row, so FF_L0_FOLD keeps working.  Stop counter:
// the rows unfinished after the step (ff_pointer_count_waves), DESIGN.md 29's counter.  No LDS beyond the four counter words.
//
// The sampled form is a compile-time form of the same kernel, selected by the argument struct: behind the masked
// reduction the wave draws from the constrained row with ff_sample_draw -- top-k and top-p therefore act on the constrained row,
// and on a dead end the draw is SEP, the only live key -- and the lane that owns the token (lane = key mod 64) reads its own
// masked logit back and broadcasts it for the log-probability (l[tok] - m) - log sum, saturated at -FLT_MAX: the model's
// distribution renormalised over the keys the rule allows.  With temperature 0 the greedy expression -logf(lsum) stays, so
// that the two forms agree bit for bit; with all flag bits clear the byte row is zero and the launch is
// pointer_sample_kernel<true>'s.  Nothing of the rule or of the draw is restated; still no barrier and no further LDS.
//
// The beam form is a kernel of its own at the end of this file: beam_sequence_constrained_select_kernel<W, STOP>,
// beam_constrained_select_kernel's shape (one wavefront per group, four per block) with this file's rule per beam.  For every
// non-empty unfinished beam the wave writes the byte row as above through ff_sequence_write_row (ff_select.h: the plain rule with
// [SEP, SEP + 1), then the two fix-ups of the closed state -- the kernel above keeps its own text of them, which is what keeps
// its registers: DESIGN.md 33), masks and reduces the row, and keeps the W best LIVE keys at c_k + (l[s] - m) - log sum in ff_select.h's sorted list.  Lanes
// 0..W-1 own one new beam each: parent, token, score, the finished flag, this step's dead-end flag, the loop-open flag and the
// rule's update of the PARENT's (first, prev); the wave writes the W * fw words of visited_out from visited_in[parent] together.
// All state is read from *_in and written to *_out.  STOP picks what the wave adds to the stop counter (DESIGN.md 30's "all" or
// "best").  No LDS beyond the four counter words, no barrier.
//
// The beam form's closure look-aheads are compile-time forms of that kernel, <W, STOP, FORM>: the argument struct
// then carries the wireframes' two distance tables and the launch's one budget, and ff_sequence_write_row<FORM> masks every
// unfinished non-empty beam's row from that beam's own (first, prev) and visited_in words -- under FF_LOOP_EXACT one search per
// such beam, W in a row on the one wave.  Candidates, scores, order, the state update and the counters are the plain form's lines.
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"
#include "ff_select.h"

namespace {

struct SeqConstrainArgs {
  PointerArgs p;                 // as ConstrainArgs.p; p.term_lo / p.term_hi = [SEP, SEP + 1): what ff_loop_write_row re-opens
  unsigned char* rows;           // [B, S] out: the constraint byte row of every unfinished sequence (1 = masked)
  const unsigned* follows;       // [wireframes, L, fw] bits or null
  int L, fw;
  int flags, ntok, sep, eos;
  const int* fin_in;             // [B] nonzero: finished before this step
  const int* first_in;           // [B] first edge of the open loop, -1: none (closed)
  const int* prev_in;            // [B] last edge of the current face, -1: none (the face has no edge yet)
  unsigned* visited;             // [B, fw] in / out: the edges of the current face, or under ONCE of every face so far
  int *fin_out, *first_out, *prev_out, *dead_out;   // [B] out
  int* tok; float* logprob;      // [B] out
  static constexpr bool DRAW = false;
};

// The sampled form's operands: the above, and the draw's.
struct SeqConstrainSampleArgs : SeqConstrainArgs {
  const float* uniforms;         // [num_uniforms] this step's draws
  const int* row_id;             // [B] the draw every launch row reads (null: b); clamped into [0, num_uniforms)
  int num_uniforms;
  float temperature; int top_k; float top_p;
  static constexpr bool DRAW = true;
};

// The closure forms' operands: either of the above, and what ff_loop_write_row<FF_LOOP_AHEAD | FF_LOOP_EXACT> reads.
// Structs of their own: the plain forms' argument layout, and with it their device code, stays what it was.
template <class Plain>
struct SeqClosureArgs : Plain {
  const unsigned char* close_dist;   // FF_LOOP_AHEAD only: [wireframes, L, L] bytes
  const unsigned char* cycle_len;    // FF_LOOP_AHEAD, FF_LOOP_EXACT: [wireframes, L] bytes
  int budget;                        // the step's: min(T - 1 - position, 254)
};
// (their launch is defined at the end of this file, behind every kernel that was there before, which keeps those in their places)
template <class Plain>
int seq_constrain_closure_launch(const Plain& plain, const ff_lookahead_io& la, int B, hipStream_t st);

// FORM: FF_LOOP_PLAIN, or one of the closure look-aheads of ff_loop_write_row -- the argument struct then carries
// the two distance tables and the step's budget (SeqClosureArgs<> of the greedy or of the sampled struct).  The rule, the search
// and the two fix-ups are the plain form's lines: nothing is restated.
template <class Args, int FORM = FF_LOOP_PLAIN>
__global__ __launch_bounds__(256) void pointer_sequence_constrained_kernel(Args a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  int unfinished = 0;
  if (b < pa.B) {   // (wave-uniform)
    const int ntok = a.ntok;
    const int was_fin = ff_ld4i(a.fin_in + b);
    int first = ff_loop_edge(ff_ld4i(a.first_in + b), a.L), prev = ff_loop_edge(ff_ld4i(a.prev_in + b), a.L);
    int tok = 0, dead = 0, fin = 1;
    float lp = 0.f;
    if (!was_fin) {
      const int w = b / pa.spg;
      int kv = pa.S;
      if (pa.kv_len) { const int k = ff_ldw(pa.kv_len + w); kv = k < kv ? k : kv; }
      const unsigned char* mrow = pa.mask ? pa.mask + (size_t)w * pa.S : nullptr;
      unsigned* vrow = a.visited + (size_t)b * a.fw;
      unsigned char* xrow = a.rows + (size_t)b * pa.S;
      FFLoopRule rule{a.follows, a.L, a.fw, a.flags, ntok, nullptr, nullptr, 0};
      if constexpr (FORM != FF_LOOP_PLAIN) { rule.close_dist = a.close_dist; rule.cycle_len = a.cycle_len; rule.budget = a.budget; }
      if constexpr (FORM == FF_LOOP_PLAIN)   // (the plain forms keep the line they had)
        dead = ff_loop_write_row<FF_LOOP_PLAIN>(pa, rule, lane, w, kv, mrow, first, prev, vrow, xrow) ? 1 : 0;
      else
        dead = ff_loop_write_row<FORM>(pa, rule, lane, w, kv, mrow, first, prev, vrow, xrow) ? 1 : 0;
      if ((a.flags & FF_CONSTRAIN_CONNECT) && !(first >= 0 && prev >= 0)) {   // closed: EOS may end the row; no empty face
        if (lane == (a.eos & 63)) xrow[a.eos] = 0;
        if (prev < 0 && lane == (a.sep & 63)) xrow[a.sep] = 1;
      }
      float m, b2, lsum;
      ff_pointer_mask_reduce<true>(pa, b, lane, &m, &b2, &tok, &lsum);
      lp = -logf(lsum);
      if constexpr (Args::DRAW) {   // the draw in place of the argmax (ff_select.h's one copy), from the row masked just now
        const float* lrow = pa.logits + (size_t)b * pa.ldlogits;
        tok = ff_sample_draw(lrow, pa.S, lane, m, tok, a.temperature, a.top_k, a.top_p, a.uniforms, a.row_id, a.num_uniforms, b);
        // the masked l[tok] was stored by lane tok % 64 a moment ago: that lane reads its own store back and broadcasts it
        const int owner = tok & 63;
        const float mine = lane == owner ? ff_ld4(lrow + tok) : 0.f;
        const float lg = __shfl(mine, owner, FF_WAVE);
        // saturates: no -inf, no NaN.  Temperature 0 selects the maximum, l[tok] = m: the greedy form's own expression stays
        if (a.temperature != 0.f) lp = fmaxf((lg - m) - logf(lsum), -FLT_MAX);
      }
      if (tok >= ntok) {
        const int e = tok - ntok;
        ff_loop_advance(a.follows, w, a.L, a.fw, e, &first, &prev);
        if (lane == 0) vrow[e >> 5] |= 1u << (e & 31);
      } else if (tok == a.sep) {
        first = prev = -1;
        if (!(a.flags & FF_CONSTRAIN_ONCE))
          for (int k = lane; k < a.fw; k += 64) vrow[k] = 0u;
      }
      fin = tok == a.eos ? 1 : 0;
      unfinished = 1 - fin;
    }
    if (lane == 0) {
      ff_st4i(a.tok + b, tok);
      ff_st4(a.logprob + b, lp);
      ff_st4i(a.fin_out + b, fin);
      ff_st4i(a.dead_out + b, dead);
      ff_st4i(a.first_out + b, first);
      ff_st4i(a.prev_out + b, prev);
    }
    if (pa.next_rows) ff_pointer_append_row(pa, b / pa.spg, b, tok, lane);
  }
  ff_pointer_count_waves(pa, pa.B, unfinished);
}
// (the greedy form is instantiated here, in the place its code has always had in this file's device code)
template __global__ void pointer_sequence_constrained_kernel<SeqConstrainArgs>(SeqConstrainArgs);

// ---- engine side: start state and output packing (ff_engine.hip) ---------------------------------------------------------------------
// Start state of one micro-batch of Bc sequences, one per wireframe: SOS (model.py:191), log-probability 0, unfinished, the
// rule's state empty and closed.
__global__ void sequence_constrain_init_kernel(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited,
                                               int Bc, int fw, int sos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  tok[i] = sos;
  lp[i] = 0.f;
  fin[i] = 0;
  dead[i] = 0;
  first[i] = prev[i] = -1;
  for (int k = 0; k < fw; ++k) visited[(size_t)i * fw + k] = 0u;
}

// predict[w, :], logprob[w, :], dead_end[w, :] and open_end[w] of the chunk's nw wireframes (sequence b0 + wl stands for
// wireframe w0 + wl) from the per-step records (tok, lp, fin, dead, first: [T, Btot], row s = the state after s steps).
// Position j is kept when j <= the stop step and the sequence was not finished before it: last = min(own EOS, stop step).
// open_end: a loop is open after the last kept position.
__global__ void sequence_constrain_finalize_kernel(const int* __restrict__ tok, const float* __restrict__ lp, const int* __restrict__ fin,
                                                   const int* __restrict__ dead, const int* __restrict__ first, int Btot, int T,
                                                   const int* __restrict__ steps_p, int w0, int nw, int b0,
                                                   int64_t* __restrict__ predict, float* __restrict__ logprob,
                                                   int* __restrict__ dead_end, int* __restrict__ open_end, int* __restrict__ seq_of_row) {
  const int steps = *steps_p;
  for (int wl = blockIdx.x * blockDim.x + threadIdx.x; wl < nw; wl += gridDim.x * blockDim.x) {
    const int seq = b0 + wl;
    const size_t row = (size_t)(w0 + wl);
    int64_t* out = predict + row * T;
    float* olp = logprob + row * T;
    int* ode = dead_end + row * T;
    int open = 0;
    bool done = false;   // finished before position j
    for (int j = 0; j < T; ++j) {
      const bool in = j <= steps && !done;
      const size_t r = (size_t)j * Btot + seq;
      out[j] = in ? tok[r] : 0;
      olp[j] = (in && j >= 1) ? lp[r] : 0.f;
      ode[j] = (in && j >= 1) ? dead[r] : 0;
      if (in) { open = first[r] >= 0 ? 1 : 0; done = fin[r] != 0; }
    }
    open_end[row] = open;
    if (seq_of_row) seq_of_row[row] = seq;
  }
}

// ---- engine side of the sampled form: start state and output packing --------------------------------------------------
// Start state of one micro-batch of Bc = nw * R draws, draw k of the chunk's wl-th wireframe at i = wl * R + k: SOS
// (model.py:191), log-probability 0, unfinished, the rule's state empty and closed; row_id: its output row (w0 + wl) * R + k.
__global__ void sequence_constrain_sample_init_kernel(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited,
                                                      int* row_id, int Bc, int R, int w0, int fw, int sos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  tok[i] = sos;
  lp[i] = 0.f;
  fin[i] = 0;
  dead[i] = 0;
  first[i] = prev[i] = -1;
  row_id[i] = w0 * R + i;
  for (int k = 0; k < fw; ++k) visited[(size_t)i * fw + k] = 0u;
}

// samples[(w, k), :], logprob and dead_end (same layout), scores[(w, k)] and open_end[(w, k)] of the chunk's nw wireframes from
// the per-step records (tok, lp, fin, dead, first: [T, Btot], row s = the state after s steps; sequence b0 + wl * R + k stands
// for draw k of wireframe w0 + wl), and draw 0 under the greedy constrained decode's keys: predict[w, :], predict_logprob[w, :],
// predict_dead_end[w, :], predict_open_end[w].  Position j is kept when j <= the stop step and the draw was not finished before
// it: last = min(own EOS, stop step); rows behind the stop step are never looked at, so the result does not depend on when the
// host saw the stop.  scores: the kept log-probabilities added in ascending position (fp64 accumulator, rounded once, saturated
// at -FLT_MAX).  open_end: a loop is open after the last kept position.
__global__ void sequence_constrain_sample_finalize_kernel(const int* __restrict__ tok, const float* __restrict__ lp,
                                                          const int* __restrict__ fin, const int* __restrict__ dead,
                                                          const int* __restrict__ first, int Btot, int T, const int* __restrict__ steps_p,
                                                          int R, int w0, int nw, int b0, int64_t* __restrict__ samples,
                                                          float* __restrict__ logprob, float* __restrict__ scores,
                                                          int* __restrict__ dead_end, int* __restrict__ open_end,
                                                          int64_t* __restrict__ predict, float* __restrict__ predict_logprob,
                                                          int* __restrict__ predict_dead_end, int* __restrict__ predict_open_end,
                                                          int* __restrict__ seq_of_row) {
  const int steps = *steps_p;
  const int total = nw * R;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int k = i % R, wl = i / R;
    const int seq = b0 + i;
    const size_t wf = (size_t)(w0 + wl), row = wf * R + k;
    int64_t* out = samples + row * T;
    float* olp = logprob + row * T;
    int* ode = dead_end + row * T;
    const bool p0 = k == 0;
    double sum = 0.0;
    int open = 0;
    bool done = false;   // finished before position j
    for (int j = 0; j < T; ++j) {
      const bool in = j <= steps && !done;
      const size_t r = (size_t)j * Btot + seq;
      const int v = in ? tok[r] : 0;
      const float l = (in && j >= 1) ? lp[r] : 0.f;
      const int de = (in && j >= 1) ? dead[r] : 0;
      out[j] = v;
      olp[j] = l;
      ode[j] = de;
      if (p0) { predict[wf * T + j] = v; predict_logprob[wf * T + j] = l; predict_dead_end[wf * T + j] = de; }
      sum += (double)l;
      if (in) { open = first[r] >= 0 ? 1 : 0; done = fin[r] != 0; }
    }
    scores[row] = (float)fmax(sum, -(double)FLT_MAX);
    open_end[row] = open;
    if (p0) predict_open_end[wf] = open;
    if (seq_of_row) seq_of_row[row] = seq;
  }
}

}  // namespace

// The flag bits, the two tokens and the follow table of a sequence-constrained step, for operator `op`.
int ff_sequence_rule_check(const char* op, const ff_loop_rule_io& r, int S, int tok_sep, int tok_eos) {
  FF_CHECK_ARG(!(r.flags & ~(FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT | FF_CONSTRAIN_ONCE)), "%s: unknown flag bits %d", op, r.flags);
  FF_CHECK_ARG(!(r.flags & FF_CONSTRAIN_ONCE) || (r.flags & FF_CONSTRAIN_NO_REPEAT), "%s: FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT", op);
  FF_CHECK_ARG(r.ntok >= 0 && r.L >= 0 && r.L == S - r.ntok, "%s: L=%d must be S - ntok = %d - %d", op, r.L, S, r.ntok);
  FF_CHECK_ARG(tok_sep >= 0 && tok_sep < r.ntok && tok_eos >= 0 && tok_eos < r.ntok && tok_sep != tok_eos,
               "%s: tok_sep=%d and tok_eos=%d must be two of the %d special tokens", op, tok_sep, tok_eos, r.ntok);
  FF_CHECK_ARG(r.follows || !(r.flags & FF_CONSTRAIN_CONNECT), "%s: FF_CONSTRAIN_CONNECT needs the follow table", op);
  return FF_OK;
}

// The checks and operands the greedy and the sampled launch share (io's terminator range is not read: the rule has its two
// tokens); `a` zeroed by the caller.
static int seq_constrain_args(SeqConstrainArgs& a, const char* op, const ff_step_io& io_in, const ff_loop_rule_io& rule,
                              const ff_constrained_state& s, int tok_sep, int tok_eos) {
  const int B = io_in.rows, S = io_in.S;
  FF_CHECK_ARG(B > 0 && S > 0 && io_in.rows_per_wireframe > 0, "%s: bad sizes B=%d S=%d", op, B, S);
  ff_step_io io = io_in;
  io.term_lo = tok_sep; io.term_hi = tok_sep + 1;   // (what ff_loop_write_row leaves open with the loop closed and re-opens on a dead end)
  FF_RETURN_IF(ff_step_args(&a.p, op, true, io));
  FF_RETURN_IF(ff_sequence_rule_check(op, rule, S, tok_sep, tok_eos));
  FF_CHECK_ARG(s.fin_in && s.first_in && s.prev_in && s.visited && s.mask_rows && s.next_tok && s.logprob && s.fin_out && s.dead_end &&
                   s.first_out && s.prev_out, "%s: null pointer", op);
  a.p.extra = s.mask_rows; a.p.ldextra = S;
  a.rows = s.mask_rows; a.follows = rule.follows; a.L = rule.L; a.fw = (rule.L + 31) >> 5; a.flags = rule.flags; a.ntok = rule.ntok;
  a.sep = tok_sep; a.eos = tok_eos;
  a.fin_in = s.fin_in; a.first_in = s.first_in; a.prev_in = s.prev_in; a.visited = s.visited;
  a.fin_out = s.fin_out; a.first_out = s.first_out; a.prev_out = s.prev_out; a.dead_out = s.dead_end;
  a.tok = s.next_tok; a.logprob = s.logprob;
  return FF_OK;
}

// The one launch behind ff_pointer_sequence_constrained, ff_pointer_sequence_constrained_ahead (ahead: the closure form's tables
// and budget, checked by ff_lookahead_check; null: the plain launch) and the engine's step.
int ff_pointer_sequence_constrained_sync(const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& s, int tok_sep,
                                         int tok_eos, const ff_lookahead_io* ahead, ff_stream_t stream) {
  const char* op = ahead ? "ff_pointer_sequence_constrained_ahead" : "ff_pointer_sequence_constrained";
  const int B = io.rows, S = io.S;
  if (B == 0) return FF_OK;
  SeqConstrainArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(seq_constrain_args(a, op, io, rule, s, tok_sep, tok_eos));
  if (ahead) FF_RETURN_IF(ff_lookahead_check(op, rule, S, *ahead));
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)B * S * 4.0, st);
  if (ahead) return seq_constrain_closure_launch(a, *ahead, B, st);
  hipLaunchKernelGGL(pointer_sequence_constrained_kernel<SeqConstrainArgs>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

// The one launch behind ff_pointer_sequence_constrained_sample, ff_pointer_sequence_constrained_sample_ahead and the engine's
// sampled step: the checks above and ff_pointer_sample_sync's (ff_sample_draw_check).
int ff_pointer_sequence_constrained_sample_sync(const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& s,
                                                int tok_sep, int tok_eos, const ff_lookahead_io* ahead, const ff_sample_draw_io& d,
                                                ff_stream_t stream) {
  const char* op = ahead ? "ff_pointer_sequence_constrained_sample_ahead" : "ff_pointer_sequence_constrained_sample";
  const int B = io.rows, S = io.S;
  if (B == 0) return FF_OK;
  SeqConstrainSampleArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(seq_constrain_args(a, op, io, rule, s, tok_sep, tok_eos));
  FF_RETURN_IF(ff_sample_draw_check(op, d, B));
  if (ahead) FF_RETURN_IF(ff_lookahead_check(op, rule, S, *ahead));
  a.uniforms = d.uniforms; a.num_uniforms = d.num_uniforms; a.row_id = d.row_id;
  a.temperature = d.temperature; a.top_k = d.top_k; a.top_p = d.top_p;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)B * S * 16.0, st);
  if (ahead) return seq_constrain_closure_launch(a, *ahead, B, st);
  hipLaunchKernelGGL(pointer_sequence_constrained_kernel<SeqConstrainSampleArgs>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

// Restates select_next (model.py:161-167) under the rule, for the loop of model.py:193-210 that starts at SOS (model.py:191).
extern "C" int ff_pointer_sequence_constrained(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                               int seqs_per_group, const unsigned* follows, int L, int flags, int ntok, int tok_sep,
                                               int tok_eos, const int* fin_in, const int* first_in, const int* prev_in,
                                               unsigned* visited, unsigned char* mask_rows, int* next_tok, float* logprob, int* fin_out,
                                               int* dead_end, int* first_out, int* prev_out, const float* memory, int E,
                                               float* next_rows, int ldnext, float* next_stats, int* count_unfinished,
                                               ff_stream_t stream) {
  return ff_pointer_sequence_constrained_sync(
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, 0, 0, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_unfinished, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      tok_sep, tok_eos, nullptr, stream);
}

// The form of a closure entry as the launches take it: 1 = the closure look-ahead, 2 = the exact one (which reads no close_dist).
static int seq_closure_form(const char* op, int form, const unsigned char* close_dist, const unsigned char* cycle_len, int budget,
                            ff_lookahead_io* out) {
  FF_CHECK_ARG(form == 1 || form == 2, "%s: form=%d must be 1 (look-ahead) or 2 (exact)", op, form);
  *out = ff_lookahead_io{form == 1 ? close_dist : nullptr, cycle_len, budget, form == 2 ? 1 : 0};
  return FF_OK;
}

// Restates select_next (model.py:161-167) under the rule with a closure look-ahead, for the loop of model.py:193-210 that starts at
// SOS (model.py:191).
extern "C" int ff_pointer_sequence_constrained_ahead(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len,
                                                     int B, int seqs_per_group, const unsigned* follows, int L, int flags, int ntok,
                                                     int tok_sep, int tok_eos, const int* fin_in, const int* first_in,
                                                     const int* prev_in, unsigned* visited, unsigned char* mask_rows, int* next_tok,
                                                     float* logprob, int* fin_out, int* dead_end, int* first_out, int* prev_out,
                                                     const float* memory, int E, float* next_rows, int ldnext, float* next_stats,
                                                     int* count_unfinished, int form, const unsigned char* close_dist,
                                                     const unsigned char* cycle_len, int budget, ff_stream_t stream) {
  ff_lookahead_io ahead;
  FF_RETURN_IF(seq_closure_form("ff_pointer_sequence_constrained_ahead", form, close_dist, cycle_len, budget, &ahead));
  return ff_pointer_sequence_constrained_sync(
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, 0, 0, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_unfinished, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      tok_sep, tok_eos, &ahead, stream);
}

int ff_sequence_constrain_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int Bc, int L, int sos,
                               hipStream_t st) {
  hipLaunchKernelGGL(sequence_constrain_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, lp, fin, dead, first, prev, visited,
                     Bc, (L + 31) >> 5, sos);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_sequence_constrain_finalize(const int* tok, const float* lp, const int* fin, const int* dead, const int* first, int Btot, int T,
                                   const int* steps_dev, int w0, int nw, int b0, int64_t* predict, float* logprob, int* dead_end,
                                   int* open_end, int* seq_of_row, hipStream_t st) {
  hipLaunchKernelGGL(sequence_constrain_finalize_kernel, dim3(ff_cdiv(nw, 256) < 1024 ? ff_cdiv(nw, 256) : 1024), dim3(256), 0, st, tok, lp,
                     fin, dead, first, Btot, T, steps_dev, w0, nw, b0, predict, logprob, dead_end, open_end, seq_of_row);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

// Restates select_next (model.py:161-167) under the rule and with the draw, for the loop of model.py:193-210 that starts at SOS
// (model.py:191).
extern "C" int ff_pointer_sequence_constrained_sample(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len,
                                                      int B, int seqs_per_group, const unsigned* follows, int L, int flags, int ntok,
                                                      int tok_sep, int tok_eos, const int* fin_in, const int* first_in,
                                                      const int* prev_in, unsigned* visited, unsigned char* mask_rows, int* next_tok,
                                                      float* logprob, int* fin_out, int* dead_end, int* first_out, int* prev_out,
                                                      const float* memory, int E, float* next_rows, int ldnext, float* next_stats,
                                                      int* count_unfinished, const float* uniforms, int num_uniforms, const int* row_id,
                                                      float temperature, int top_k, float top_p, ff_stream_t stream) {
  return ff_pointer_sequence_constrained_sample_sync(
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, 0, 0, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_unfinished, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      tok_sep, tok_eos, nullptr, ff_sample_draw_io{uniforms, num_uniforms, row_id, temperature, top_k, top_p}, stream);
}

// Restates select_next (model.py:161-167) under the rule with a closure look-ahead and with the draw, for the loop of
// model.py:193-210 that starts at SOS (model.py:191).
extern "C" int ff_pointer_sequence_constrained_sample_ahead(float* logits, int ldlogits, int S, const unsigned char* mask,
                                                            const int* kv_len, int B, int seqs_per_group, const unsigned* follows, int L,
                                                            int flags, int ntok, int tok_sep, int tok_eos, const int* fin_in,
                                                            const int* first_in, const int* prev_in, unsigned* visited,
                                                            unsigned char* mask_rows, int* next_tok, float* logprob, int* fin_out,
                                                            int* dead_end, int* first_out, int* prev_out, const float* memory, int E,
                                                            float* next_rows, int ldnext, float* next_stats, int* count_unfinished,
                                                            const float* uniforms, int num_uniforms, const int* row_id,
                                                            float temperature, int top_k, float top_p, int form,
                                                            const unsigned char* close_dist, const unsigned char* cycle_len, int budget,
                                                            ff_stream_t stream) {
  ff_lookahead_io ahead;
  FF_RETURN_IF(seq_closure_form("ff_pointer_sequence_constrained_sample_ahead", form, close_dist, cycle_len, budget, &ahead));
  return ff_pointer_sequence_constrained_sample_sync(
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, 0, 0, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_unfinished, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      tok_sep, tok_eos, &ahead, ff_sample_draw_io{uniforms, num_uniforms, row_id, temperature, top_k, top_p}, stream);
}

int ff_sequence_constrain_sample_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int* row_id,
                                      int Bc, int R, int w0, int L, int sos, hipStream_t st) {
  hipLaunchKernelGGL(sequence_constrain_sample_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, lp, fin, dead, first, prev,
                     visited, row_id, Bc, R, w0, (L + 31) >> 5, sos);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_sequence_constrain_sample_finalize(const int* tok, const float* lp, const int* fin, const int* dead, const int* first, int Btot,
                                          int T, const int* steps_dev, int R, int w0, int nw, int b0, int64_t* samples, float* logprob,
                                          float* scores, int* dead_end, int* open_end, int64_t* predict, float* predict_logprob,
                                          int* predict_dead_end, int* predict_open_end, int* seq_of_row, hipStream_t st) {
  const int total = nw * R;
  hipLaunchKernelGGL(sequence_constrain_sample_finalize_kernel, dim3(ff_cdiv(total, 256) < 1024 ? ff_cdiv(total, 256) : 1024), dim3(256), 0,
                     st, tok, lp, fin, dead, first, Btot, T, steps_dev, R, w0, nw, b0, samples, logprob, scores, dead_end, open_end,
                     predict, predict_logprob, predict_dead_end, predict_open_end, seq_of_row);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

// ==== beam search over the sequence-constrained decode ==================================================================
namespace {
// (the sampled form is instantiated here, where the end of this file used to be: in front of the kernels below, as it was in front
// of nothing, its device code keeps the place and the local labels it had)
template __global__ void pointer_sequence_constrained_kernel<SeqConstrainSampleArgs>(SeqConstrainSampleArgs);

struct SeqConBeamArgs {
  PointerArgs p;                 // as ConBeamArgs.p; p.term_lo / p.term_hi = [SEP, SEP + 1): what ff_loop_write_row re-opens
  int groups;
  unsigned char* rows;           // [B, S] out: the constraint byte row of every non-empty unfinished beam (1 = masked)
  const unsigned* follows;       // [wireframes, L, fw] bits or null
  int L, fw, flags, ntok, sep, eos;
  const float* score_in; float* score_out;
  const int *fin_in, *first_in, *prev_in;
  const unsigned* visited_in;    // [B, fw]
  int *fin_out, *dead_out, *open_out, *first_out, *prev_out;
  unsigned* visited_out;         // [B, fw], not visited_in
  int* parent; int* tok;         // [B] out
};

// The closure forms' operands: the above, and what ff_loop_write_row<FF_LOOP_AHEAD | FF_LOOP_EXACT> reads.  A struct
// of its own: the plain forms' argument layout, and with it their device code, stays what it was.  The tables are per wireframe
// and shared by its W beams; all beams of a launch sit at the same position, so there is one budget.
struct SeqConBeamClosureArgs : SeqConBeamArgs {
  const unsigned char* close_dist;   // FF_LOOP_AHEAD only: [wireframes, L, L] bytes
  const unsigned char* cycle_len;    // FF_LOOP_AHEAD, FF_LOOP_EXACT: [wireframes, L] bytes
  int budget;                        // the step's: min(T - 1 - position, 254)
};
template <int FORM> struct SeqConBeamArgsOf { using type = SeqConBeamClosureArgs; };
template <> struct SeqConBeamArgsOf<FF_LOOP_PLAIN> { using type = SeqConBeamArgs; };

// (the closure forms' launch is defined at the end of this file, behind every kernel that was there before)
int seq_beam_closure_launch(const SeqConBeamArgs& plain, const ff_lookahead_io& la, int W, int stop_best, dim3 grid, dim3 block,
                            hipStream_t st);

// STOP 0 ("all"): the counter is the non-empty beams unfinished after the step; STOP 1 ("best"): the groups whose rank 0 is.
// FORM: FF_LOOP_PLAIN, or one of the closure look-aheads -- every unfinished non-empty beam then forms its byte row
// from its OWN (first, prev) and its OWN visited words against the wireframe's tables and the launch's budget; under FF_LOOP_EXACT
// that is one search per such beam, W in a row on the one wave.  The search, the scores and the state update are the plain form's
// lines: nothing is restated.
template <int W, int STOP, int FORM = FF_LOOP_PLAIN>
__global__ __launch_bounds__(256) void beam_sequence_constrained_select_kernel(typename SeqConBeamArgsOf<FORM>::type a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const float FILL = -FLT_MAX;
  int ncount = 0;
  if (g < a.groups) {   // (wave-uniform)
    const int S = pa.S, ntok = a.ntok, b0 = g * W, fw = a.fw;
    const int w = b0 / pa.spg;   // (the beams of a group share the wireframe)
    int kv = S;
    if (pa.kv_len) { const int k = ff_ldw(pa.kv_len + w); kv = k < kv ? k : kv; }
    const unsigned char* mrow = pa.mask ? pa.mask + (size_t)w * S : nullptr;
    // lane k < W holds beam k's state; the loops below broadcast it
    const float my_c = lane < W ? a.score_in[b0 + lane] : -INFINITY;
    const int my_f = lane < W ? a.fin_in[b0 + lane] : 0;
    const int my_first = ff_loop_edge(lane < W ? a.first_in[b0 + lane] : -1, a.L);
    const int my_prev = ff_loop_edge(lane < W ? a.prev_in[b0 + lane] : -1, a.L);
    FFLoopRule rule{a.follows, a.L, fw, a.flags, ntok, nullptr, nullptr, 0};
    if constexpr (FORM != FF_LOOP_PLAIN) { rule.close_dist = a.close_dist; rule.cycle_len = a.cycle_len; rule.budget = a.budget; }
    unsigned deadmask = 0u;   // bit k: beam k dead-ended at this step (wave-uniform)
    float lsc[W];
    int lix[W];
    ff_beam_list_init<W>(lsc, lix);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float c = __shfl(my_c, k, FF_WAVE);
      const int f = __shfl(my_f, k, FF_WAVE);
      const int first = __shfl(my_first, k, FF_WAVE), prev = __shfl(my_prev, k, FF_WAVE);
      if (c == -INFINITY) continue;                      // empty beam: no candidates (wave-uniform)
      if (f) {                                           // finished: itself, token 0, score unchanged
        if (lane == 0) ff_beam_insert<W>(lsc, lix, c, k * S);
        continue;
      }
      const int b = b0 + k;
      bool dead;
      if constexpr (FORM == FF_LOOP_PLAIN)   // (the plain forms keep the line they had)
        dead = ff_sequence_write_row(pa, rule, lane, w, kv, mrow, first, prev, a.visited_in + (size_t)b * fw, a.rows + (size_t)b * S, a.sep,
                                     a.eos);
      else
        dead = ff_sequence_write_row<FORM>(pa, rule, lane, w, kv, mrow, first, prev, a.visited_in + (size_t)b * fw,
                                           a.rows + (size_t)b * S, a.sep, a.eos);
      if (dead) deadmask |= 1u << k;
      float m, b2, lsum;
      int i1;
      ff_pointer_mask_reduce<true>(pa, b, lane, &m, &b2, &i1, &lsum);
      const float logz = logf(lsum);
      if (!(m > FILL)) {                                 // no live key: token 0 at c - log S (wave-uniform)
        if (lane == 0) ff_beam_insert<W>(lsc, lix, fmaxf(c - logz, FILL), k * S);
        continue;
      }
      // W = 1: the one kept candidate is the row maximum (l[s] = m, the lowest such key: i1), so the score is c + (-log sum), the
      // greedy form's own expression -- identity (a) then holds bit for bit, the sign of a zero log-probability included
      if constexpr (W == 1) {
        if (lane == 0) ff_beam_insert<W>(lsc, lix, fmaxf(c + (-logz), FILL), k * S + i1);
      } else {
        ff_beam_walk<W, true>(lsc, lix, pa.logits + (size_t)b * pa.ldlogits, S, lane, k, c, m, logz);
      }
    }
    ff_beam_merge<W>(lsc, lix);
    float sc;
    int ix;
    ff_beam_rank<W>(lsc, lix, lane, &sc, &ix);
    const bool some = lane < W && ix != FF_BEAM_NONE;
    const int par = some ? ix / S : (lane < W ? lane : 0);
    const int pfin = __shfl(my_f, par, FF_WAVE);
    int first = __shfl(my_first, par, FF_WAVE), prev = __shfl(my_prev, par, FF_WAVE);
    const bool grew = some && !pfin;                     // the parent was unfinished: tk is this step's token
    const int tk = grew ? ix - par * S : 0;
    const int dead_now = grew ? (int)((deadmask >> par) & 1u) : 0;
    const int nfin = some ? ((pfin || tk == a.eos) ? 1 : 0) : 0;
    const int e_new = (grew && tk >= ntok) ? tk - ntok : -1;
    const bool at_sep = grew && tk == a.sep;
    const int wipe = (at_sep && !(a.flags & FF_CONSTRAIN_ONCE)) ? 1 : 0;   // SEP clears the face's edges unless ONCE
    if (e_new >= 0) ff_loop_advance(a.follows, w, a.L, fw, e_new, &first, &prev);   // (of the parent's first, prev)
    if (at_sep) first = prev = -1;
    const unsigned long long live = __ballot(some && !nfin);
    ncount = STOP == 0 ? __popcll(live) : (int)(live & 1ull);
    if (lane < W) {
      a.parent[b0 + lane] = par;
      a.tok[b0 + lane] = tk;
      a.score_out[b0 + lane] = sc;
      a.fin_out[b0 + lane] = nfin;
      a.dead_out[b0 + lane] = dead_now;
      a.open_out[b0 + lane] = (some && first >= 0) ? 1 : 0;
      a.first_out[b0 + lane] = first;
      a.prev_out[b0 + lane] = prev;
    }
    // visited_out[i] = SEP without ONCE: 0; else visited_in[parent[i]] | bit(edge): word (i, j) by lane i * fw + j (wave-uniform
    // bound: the shuffles need every lane)
    for (int i0 = 0; i0 < W * fw; i0 += 64) {
      const int idx = i0 + lane;
      const bool in = idx < W * fw;
      const int i = in ? idx / fw : 0, j = idx - i * fw;
      const int p = __shfl(par, i, FF_WAVE), e = __shfl(e_new, i, FF_WAVE), z = __shfl(wipe, i, FF_WAVE);
      if (in) {
        unsigned v = z ? 0u : a.visited_in[(size_t)(b0 + p) * fw + j];
        if (e >= 0 && (e >> 5) == j) v |= 1u << (e & 31);
        a.visited_out[(size_t)(b0 + i) * fw + j] = v;
      }
    }
    if (pa.next_rows) {
#pragma unroll
      for (int k = 0; k < W; ++k) ff_pointer_append_row(pa, w, b0 + k, __shfl(tk, k, FF_WAVE), lane);
    }
  }
  ff_pointer_count_waves(pa, a.groups, ncount);
}

// Start state of one micro-batch of Bc = nw * W beams, beam k of the chunk's wl-th wireframe at i = wl * W + k: SOS
// (model.py:191), unfinished, beam 0 with score 0 and the others empty (-inf), parent = k, the rule's state empty and closed
// (first, prev, visited: half 0 of the ping-pong, which step 0 reads).
__global__ void sequence_constrain_beam_init_kernel(int* tok, float* score, int* fin, int* dead, int* open, int* parent, int* first,
                                                    int* prev, unsigned* visited, int Bc, int W, int fw, int sos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  const int k = i % W;
  tok[i] = sos;
  score[i] = k == 0 ? 0.f : -INFINITY;
  fin[i] = 0;
  dead[i] = 0;
  open[i] = 0;
  parent[i] = k;
  first[i] = prev[i] = -1;
  for (int j = 0; j < fw; ++j) visited[(size_t)i * fw + j] = 0u;
}

// beams[(w, k), :] and beam_dead_end[(w, k), :] from walking the parents back from the stop step through the per-step records
// (tok, parent, dead: [T, Btot], row s = the state after s steps), scores / finished / open_end [(w, k)] from the stop step's
// row, and beam 0 under the greedy constrained decode's keys: predict[w, :], dead_end[w, :], open_end[w].  Rows behind the stop
// step are never looked at (the ping-pong state is not read at all), so the result does not depend on when the host saw the
// stop.  A finished beam appends token 0 and no dead end, so every row is zero past its EOS.
__global__ void sequence_constrain_beam_finalize_kernel(const int* __restrict__ tok, const int* __restrict__ parent,
                                                        const float* __restrict__ score, const int* __restrict__ fin,
                                                        const int* __restrict__ dead, const int* __restrict__ open, int Btot, int T,
                                                        const int* __restrict__ steps_p, int W, int w0, int nw, int b0,
                                                        int64_t* __restrict__ beams, float* __restrict__ scores,
                                                        int* __restrict__ finished, int* __restrict__ beam_dead_end,
                                                        int* __restrict__ beam_open_end, int64_t* __restrict__ predict,
                                                        int* __restrict__ dead_end, int* __restrict__ open_end,
                                                        int* __restrict__ seq_of_row) {
  const int steps = *steps_p;
  const int total = nw * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int k = i % W, wl = i / W;
    const int grp = b0 + wl * W;
    const size_t wf = (size_t)(w0 + wl), row = wf * W + k;
    int64_t* out = beams + row * T;
    int* ode = beam_dead_end + row * T;
    const bool p0 = k == 0;
    for (int j = steps + 1; j < T; ++j) {
      out[j] = 0; ode[j] = 0;
      if (p0) { predict[wf * T + j] = 0; dead_end[wf * T + j] = 0; }
    }
    int cur = k;
    for (int s = steps; s >= 0; --s) {
      const size_t r = (size_t)s * Btot + grp + cur;
      const int v = tok[r], de = s > 0 ? dead[r] : 0;
      out[s] = v; ode[s] = de;
      if (p0) { predict[wf * T + s] = v; dead_end[wf * T + s] = de; }
      cur = s > 0 ? parent[r] : cur;
    }
    const size_t last = (size_t)steps * Btot + grp + k;
    scores[row] = score[last];
    finished[row] = fin[last];
    beam_open_end[row] = open[last];
    if (p0) open_end[wf] = open[last];
    if (seq_of_row) seq_of_row[row] = grp + k;
  }
}

}  // namespace

// The one launch behind ff_beam_sequence_constrained_select and the engine's step; `io` carries the common operands
// (io.rows = groups * width; its terminator range is not read: the rule has its two tokens).
// `ahead`: the closure forms' tables and budget, checked by ff_lookahead_check; null: the plain launch.
int ff_beam_sequence_constrained_select_sync(const ff_step_io& io_in, const ff_beam_sequence_constrained_step* d,
                                             const ff_lookahead_io* ahead, ff_stream_t stream) {
  const char* op = ahead ? "ff_beam_sequence_constrained_select_ahead" : "ff_beam_sequence_constrained_select";
  const int S = io_in.S, W = d->width, groups = io_in.rows / W;
  SeqConBeamArgs a;
  memset(&a, 0, sizeof(a));
  ff_step_io io = io_in;
  io.term_lo = d->tok_sep; io.term_hi = d->tok_sep + 1;   // (what ff_loop_write_row leaves open with the loop closed and re-opens on a dead end)
  FF_RETURN_IF(ff_step_args(&a.p, op, true, io));
  FF_RETURN_IF(ff_sequence_rule_check(op, ff_loop_rule_io{d->follows, d->L, d->flags, d->ntok}, S, d->tok_sep, d->tok_eos));
  FF_CHECK_ARG(d->stop_best == 0 || d->stop_best == 1, "%s: stop_best=%d must be 0 or 1", op, d->stop_best);
  FF_CHECK_ARG(d->scores_in && d->scores_out && d->fin_in && d->fin_out && d->dead_out && d->open_out && d->first_in && d->first_out &&
                   d->prev_in && d->prev_out && d->visited_in && d->visited_out && d->mask_rows && d->parent && d->next_tok,
               "%s: null pointer", op);
  FF_CHECK_ARG(d->visited_in != d->visited_out, "%s: visited_out must not be visited_in", op);
  // (ONCE is this rule's own bit: the look-aheads' flag checks are about the other two)
  if (ahead) FF_RETURN_IF(ff_lookahead_check(op, ff_loop_rule_io{d->follows, d->L, d->flags, d->ntok}, S, *ahead));
  a.p.extra = d->mask_rows; a.p.ldextra = S;
  a.groups = groups; a.rows = d->mask_rows; a.follows = d->follows; a.L = d->L; a.fw = (d->L + 31) >> 5; a.flags = d->flags; a.ntok = d->ntok;
  a.sep = d->tok_sep; a.eos = d->tok_eos;
  a.score_in = d->scores_in; a.score_out = d->scores_out;
  a.fin_in = d->fin_in; a.first_in = d->first_in; a.prev_in = d->prev_in; a.visited_in = d->visited_in;
  a.fin_out = d->fin_out; a.dead_out = d->dead_out; a.open_out = d->open_out; a.first_out = d->first_out; a.prev_out = d->prev_out;
  a.visited_out = d->visited_out;
  a.parent = d->parent; a.tok = d->next_tok;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)io.rows * S * 14.0, st);
  const dim3 grid(ff_cdiv(groups, 4)), block(256);
  if (ahead) return seq_beam_closure_launch(a, *ahead, W, d->stop_best, grid, block, st);
  const int rc = ff_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(W, [&](auto w) {
    return ff_dispatch<0, 1>(d->stop_best, [&](auto f) {
      hipLaunchKernelGGL((beam_sequence_constrained_select_kernel<decltype(w)::value, decltype(f)::value>), grid, block, 0, st, a);
      return FF_OK;
    });
  });
  FF_RETURN_IF(rc);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" int ff_beam_sequence_constrained_select(const ff_beam_sequence_constrained_step* d, ff_stream_t stream) {
  const char* op = "ff_beam_sequence_constrained_select";
  FF_CHECK_ARG(d != nullptr, "%s: null descriptor", op);
  FF_RETURN_IF(ff_beam_check_sizes(op, d->groups, d->width, d->groups_per_wireframe, d->S));
  return ff_beam_sequence_constrained_select_sync(
      ff_step_io{d->logits, d->ldlogits, d->S, d->mask, d->kv_len, d->groups * d->width, d->groups_per_wireframe * d->width, 0, 0, d->ntok,
                 d->memory, d->E, d->next_rows, d->ldnext, d->next_stats, d->count_unfinished, nullptr, nullptr},
      d, nullptr, stream);
}

// One step of the beam search under the rule with a closure look-ahead: the step descriptor above, unchanged, then the
// form (1 = the closure look-ahead, 2 = the exact one, which reads no close_dist), the wireframes' tables and the step's budget.
extern "C" int ff_beam_sequence_constrained_select_ahead(const ff_beam_sequence_constrained_step* d, int form,
                                                         const unsigned char* close_dist, const unsigned char* cycle_len, int budget,
                                                         ff_stream_t stream) {
  const char* op = "ff_beam_sequence_constrained_select_ahead";
  FF_CHECK_ARG(d != nullptr, "%s: null descriptor", op);
  FF_RETURN_IF(ff_beam_check_sizes(op, d->groups, d->width, d->groups_per_wireframe, d->S));
  ff_lookahead_io ahead;
  FF_RETURN_IF(seq_closure_form(op, form, close_dist, cycle_len, budget, &ahead));
  return ff_beam_sequence_constrained_select_sync(
      ff_step_io{d->logits, d->ldlogits, d->S, d->mask, d->kv_len, d->groups * d->width, d->groups_per_wireframe * d->width, 0, 0, d->ntok,
                 d->memory, d->E, d->next_rows, d->ldnext, d->next_stats, d->count_unfinished, nullptr, nullptr},
      d, &ahead, stream);
}

int ff_sequence_constrain_beam_init(int* tok, float* score, int* fin, int* dead, int* open, int* parent, int* first, int* prev,
                                    unsigned* visited, int Bc, int W, int L, int sos, hipStream_t st) {
  hipLaunchKernelGGL(sequence_constrain_beam_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, score, fin, dead, open, parent,
                     first, prev, visited, Bc, W, (L + 31) >> 5, sos);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_sequence_constrain_beam_finalize(const int* tok, const int* parent, const float* score, const int* fin, const int* dead,
                                        const int* open, int Btot, int T, const int* steps_dev, int W, int w0, int nw, int b0,
                                        int64_t* beams, float* scores, int* finished, int* beam_dead_end, int* beam_open_end,
                                        int64_t* predict, int* dead_end, int* open_end, int* seq_of_row, hipStream_t st) {
  const int total = nw * W;
  hipLaunchKernelGGL(sequence_constrain_beam_finalize_kernel, dim3(ff_cdiv(total, 256) < 1024 ? ff_cdiv(total, 256) : 1024), dim3(256), 0,
                     st, tok, parent, score, fin, dead, open, Btot, T, steps_dev, W, w0, nw, b0, beams, scores, finished, beam_dead_end,
                     beam_open_end, predict, dead_end, open_end, seq_of_row);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

// ==== the closure look-aheads of the sequence-constrained step ===========================================================
namespace {
// (the four closure forms are instantiated here, behind the two plain forms and the engine-side kernels, which keep their places;
// the beam kernels, which the compiler instantiates at the end of the translation unit, follow them with their code unchanged)
template __global__ void pointer_sequence_constrained_kernel<SeqClosureArgs<SeqConstrainArgs>, FF_LOOP_AHEAD>(SeqClosureArgs<SeqConstrainArgs>);
template __global__ void pointer_sequence_constrained_kernel<SeqClosureArgs<SeqConstrainArgs>, FF_LOOP_EXACT>(SeqClosureArgs<SeqConstrainArgs>);
template __global__ void pointer_sequence_constrained_kernel<SeqClosureArgs<SeqConstrainSampleArgs>, FF_LOOP_AHEAD>(
    SeqClosureArgs<SeqConstrainSampleArgs>);
template __global__ void pointer_sequence_constrained_kernel<SeqClosureArgs<SeqConstrainSampleArgs>, FF_LOOP_EXACT>(
    SeqClosureArgs<SeqConstrainSampleArgs>);

// The plain form's operands (checked and filled by the caller) with the look-ahead's, launched in the form `la` names.
template <class Plain>
int seq_constrain_closure_launch(const Plain& plain, const ff_lookahead_io& la, int B, hipStream_t st) {
  SeqClosureArgs<Plain> a;
  memset(&a, 0, sizeof(a));
  static_cast<Plain&>(a) = plain;
  a.close_dist = la.exact ? nullptr : la.close_dist; a.cycle_len = la.cycle_len; a.budget = la.budget;
  if (la.exact)
    hipLaunchKernelGGL((pointer_sequence_constrained_kernel<SeqClosureArgs<Plain>, FF_LOOP_EXACT>), dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((pointer_sequence_constrained_kernel<SeqClosureArgs<Plain>, FF_LOOP_AHEAD>), dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
}  // namespace

// ==== the closure look-aheads of the sequence-constrained beam step =======================================================
namespace {
// The plain form's operands (checked and filled by the caller) with the look-ahead's, launched in the form `la` names.  The 32
// closure forms are instantiated here, behind everything the file had, so that every kernel before them keeps its code.
int seq_beam_closure_launch(const SeqConBeamArgs& plain, const ff_lookahead_io& la, int W, int stop_best, dim3 grid, dim3 block,
                            hipStream_t st) {
  SeqConBeamClosureArgs a;
  memset(&a, 0, sizeof(a));
  static_cast<SeqConBeamArgs&>(a) = plain;
  a.close_dist = la.exact ? nullptr : la.close_dist; a.cycle_len = la.cycle_len; a.budget = la.budget;
  const int rc = ff_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(W, [&](auto w) {
    return ff_dispatch<0, 1>(stop_best, [&](auto f) {
      return ff_dispatch<FF_LOOP_AHEAD, FF_LOOP_EXACT>(la.exact ? FF_LOOP_EXACT : FF_LOOP_AHEAD, [&](auto form) {
        hipLaunchKernelGGL((beam_sequence_constrained_select_kernel<decltype(w)::value, decltype(f)::value, decltype(form)::value>), grid,
                           block, 0, st, a);
        return FF_OK;
      });
    });
  });
  FF_RETURN_IF(rc);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
}  // namespace
