// Beam search over the loop-constrained pointer head (opt-in, parallel variant): one step's top-W selection over
// the LIVE keys of the W constrained rows of every group, with the rule's per-beam state following the parent permutation.
//
// beam_constrained_select_kernel<W, FORM>: one wavefront per group, four per block, as beam_select_kernel.  For each non-empty
// unfinished beam the wave writes the byte row of the beam's constraint mask with the function pointer_constrained_kernel calls
// (ff_loop_write_row<FORM>, ff_select.h: the vote on "any live edge", the terminators re-opened on a dead end; FORM is the plain
// rule, the closure look-ahead or the exact one -- DESIGN.md 28: the beam's own first / prev pick the table row, the exact form
// runs one search per open beam over that beam's visited words, and all beams share the step's budget), masks and
// reduces the logit row with that row as the extra mask (ff_pointer_mask_reduce<true>, ff_device.h: every lane reads back only
// bytes and logits it wrote itself), walks its strided keys once more and keeps the W best LIVE candidates
// c_k + (l[s] - m) - log(sum) in the sorted register list of ff_select.h, beam_select_kernel's -- a masked key
// (l[s] = -FLT_MAX) is never a candidate; a row without a live key contributes token 0 at c_k - log S, what the constrained
// greedy launch selects there.  The beam's dead-end bit goes into a wave-uniform mask.  The list's butterfly merge; lanes
// 0..W-1 then own one new beam each: parent, token, score, the finished and the cumulative dead flag, and the rule's update of
// the PARENT's (first, prev) (ff_loop_advance); the wave writes the W * fw words of visited_out = visited_in[parent] |
// bit(token) together.  All state is read from the *_in arrays and written to the *_out arrays: no beam reads what a sibling
// wrote.  Rows are appended by ff_pointer_append_row (FF_L0_FOLD is kept), the stop counter is ff_pointer_count_waves'.  No LDS
// beyond the four counter words.
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"
#include "ff_select.h"

namespace {

struct ConBeamArgs {
  PointerArgs p;                 // logits / masks / memory / next rows / counters of the B = groups * W launch rows; p.extra = rows
  int groups;
  unsigned char* rows;           // [B, S] out: the constraint byte row of every non-empty unfinished beam (1 = masked)
  const unsigned* follows;       // [wireframes, L, fw] bits or null
  int L, fw, flags, ntok;
  const float* score_in; float* score_out;
  const int *fin_in, *dead_in, *first_in, *prev_in;
  const unsigned* visited_in;    // [B, fw]
  int *fin_out, *dead_out, *first_out, *prev_out;
  unsigned* visited_out;         // [B, fw], not visited_in
  int* parent; int* tok;         // [B] out
  const unsigned char* close_dist;   // FF_LOOP_AHEAD only: [wireframes, L, L] bytes
  const unsigned char* cycle_len;    // FF_LOOP_AHEAD, FF_LOOP_EXACT: [wireframes, L] bytes
  int budget;                        // FF_LOOP_AHEAD, FF_LOOP_EXACT: the step's, shared by every beam of the launch
};

template <int W, int FORM>
__global__ __launch_bounds__(256) void beam_constrained_select_kernel(ConBeamArgs a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const float FILL = -FLT_MAX;
  int nge = 0;
  if (g < a.groups) {   // (wave-uniform)
    const int S = pa.S, ntok = a.ntok, b0 = g * W, fw = a.fw;
    const int w = b0 / pa.spg;   // (the beams of a group share the wireframe)
    int kv = S;
    if (pa.kv_len) { const int k = ff_ldw(pa.kv_len + w); kv = k < kv ? k : kv; }
    const unsigned char* mrow = pa.mask ? pa.mask + (size_t)w * S : nullptr;
    // lane k < W holds beam k's state; the loops below broadcast it
    const float my_c = lane < W ? a.score_in[b0 + lane] : -INFINITY;
    const int my_f = lane < W ? a.fin_in[b0 + lane] : 0;
    const int my_d = lane < W ? a.dead_in[b0 + lane] : 0;
    const int my_first = ff_loop_edge(lane < W ? a.first_in[b0 + lane] : -1, a.L);
    const int my_prev = ff_loop_edge(lane < W ? a.prev_in[b0 + lane] : -1, a.L);
    const FFLoopRule rule{a.follows, a.L, fw, a.flags, ntok, a.close_dist, a.cycle_len, a.budget};
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
      if (ff_loop_write_row<FORM>(pa, rule, lane, w, kv, mrow, first, prev, a.visited_in + (size_t)b * fw, a.rows + (size_t)b * S))
        deadmask |= 1u << k;
      float m, b2, lsum;
      int i1;
      ff_pointer_mask_reduce<true>(pa, b, lane, &m, &b2, &i1, &lsum);
      const float logz = logf(lsum);
      if (!(m > FILL)) {                                 // no live key: token 0 at c - log S (wave-uniform)
        if (lane == 0) ff_beam_insert<W>(lsc, lix, fmaxf(c - logz, FILL), k * S);
        continue;
      }
      ff_beam_walk<W, true>(lsc, lix, pa.logits + (size_t)b * pa.ldlogits, S, lane, k, c, m, logz);
    }
    ff_beam_merge<W>(lsc, lix);
    float sc;
    int ix;
    ff_beam_rank<W>(lsc, lix, lane, &sc, &ix);
    const bool some = lane < W && ix != FF_BEAM_NONE;
    const int par = some ? ix / S : (lane < W ? lane : 0);
    const int pfin = __shfl(my_f, par, FF_WAVE), pdead = __shfl(my_d, par, FF_WAVE);
    int first = __shfl(my_first, par, FF_WAVE), prev = __shfl(my_prev, par, FF_WAVE);
    const int dead_now = some ? (int)((deadmask >> par) & 1u) : 0;
    const int tk = (some && !pfin) ? ix - par * S : 0;
    const int nfin = some ? ((pfin || dead_now || (tk >= pa.term_lo && tk < pa.term_hi)) ? 1 : 0) : 0;
    const int ndead = some ? ((pdead || dead_now) ? 1 : 0) : 0;
    const int e_new = (some && !pfin && tk >= ntok) ? tk - ntok : -1;
    nge = __popcll(__ballot(e_new >= 0));
    if (e_new >= 0) ff_loop_advance(a.follows, w, a.L, fw, e_new, &first, &prev);   // (of the parent's first, prev)
    if (lane < W) {
      a.parent[b0 + lane] = par;
      a.tok[b0 + lane] = tk;
      a.score_out[b0 + lane] = sc;
      a.fin_out[b0 + lane] = nfin;
      a.dead_out[b0 + lane] = ndead;
      a.first_out[b0 + lane] = first;
      a.prev_out[b0 + lane] = prev;
    }
    // visited_out[i] = visited_in[parent[i]] | bit(token): word (i, j) by lane i * fw + j (wave-uniform bound: the shuffles need every lane)
    for (int i0 = 0; i0 < W * fw; i0 += 64) {
      const int idx = i0 + lane;
      const bool in = idx < W * fw;
      const int i = in ? idx / fw : 0, j = idx - i * fw;
      const int p = __shfl(par, i, FF_WAVE), e = __shfl(e_new, i, FF_WAVE);
      if (in) {
        unsigned v = a.visited_in[(size_t)(b0 + p) * fw + j];
        if (e >= 0 && (e >> 5) == j) v |= 1u << (e & 31);
        a.visited_out[(size_t)(b0 + i) * fw + j] = v;
      }
    }
    if (pa.next_rows) {
#pragma unroll
      for (int k = 0; k < W; ++k) ff_pointer_append_row(pa, w, b0 + k, __shfl(tk, k, FF_WAVE), lane);
    }
  }
  ff_pointer_count_waves(pa, a.groups, nge);
}

// ---- engine side: start state and the dead-end output of a constrained beam decode (ff_engine.hip) -------------------------------
// Start state of one micro-batch of Bc = nw * Fc * W beams (beam_init_kernel and constrain_init_kernel in one): every beam of a
// group holds the group's start token and the rule's state after column 0; beam 0 has score 0, the others are empty (-inf); a
// start token in the terminator range finishes the beam at position 0.
__global__ void cbeam_init_kernel(int* tok, float* score, int* fin, int* dead, int* parent, int* first, int* prev, unsigned* visited,
                                  int Bc, int Fc, int W, int f0, const int* num_input, int pad_tok, int term_lo, int term_hi, int ntok,
                                  const unsigned* follows, int L, int fw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  const int k = i % W, an = i / W, wl = an / Fc;
  int done;
  const int t = ff_start_token(f0 + an % Fc, num_input[wl], pad_tok, term_lo, term_hi, &done);
  tok[i] = t;
  score[i] = k == 0 ? 0.f : -INFINITY;
  fin[i] = done;
  dead[i] = 0;
  parent[i] = k;
  int fi, pv;
  ff_loop_start(t, ntok, follows, wl, L, fw, visited + (size_t)i * fw, &fi, &pv);
  first[i] = fi;
  prev[i] = pv;
}

// dead_end[(w, fo, k)] = the cumulative dead flag of beam k in the record of the stop step (dead: [T, Btot]); rows as
// beam_finalize_kernel's.
__global__ void cbeam_dead_kernel(const int* __restrict__ dead, int Btot, const int* __restrict__ steps_p,
                                  const int* __restrict__ num_input, int dedup, int F, int W, int w0, int nw, int Fc, int f0, int b0,
                                  int* __restrict__ dead_end) {
  const int steps = *steps_p;
  const int total = nw * F * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int k = i % W, fo = (i / W) % F, wl = i / (W * F);
    int an;
    if (!ff_compact_seq(num_input, dedup, w0, wl, fo, Fc, f0, &an)) continue;
    dead_end[((size_t)(w0 + wl) * F + fo) * W + k] = dead[(size_t)steps * Btot + b0 + an * W + k];
  }
}

}  // namespace

// The one launch behind ff_beam_constrained_select (ahead = null: the plain rule) and ff_beam_constrained_select_ahead (the
// closure look-ahead, or with ahead->exact the exact one); `op` words the errors.
int ff_beam_constrained_select_sync(const char* op, const ff_step_io& io, const ff_beam_constrained_step* d, const ff_lookahead_io* ahead,
                                    ff_stream_t stream) {
  const int S = io.S, W = d->width, groups = io.rows / W;
  ConBeamArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(ff_step_args(&a.p, op, true, io));
  FF_RETURN_IF(ff_loop_rule_check(op, ff_loop_rule_io{d->follows, d->L, d->flags, d->ntok}, S, io.term_lo, io.term_hi));
  FF_CHECK_ARG(d->scores_in && d->scores_out && d->fin_in && d->fin_out && d->dead_in && d->dead_out && d->first_in && d->first_out &&
                   d->prev_in && d->prev_out && d->visited_in && d->visited_out && d->mask_rows && d->parent && d->next_tok,
               "%s: null pointer", op);
  FF_CHECK_ARG(d->visited_in != d->visited_out, "%s: visited_out must not be visited_in", op);
  if (ahead) {
    FF_RETURN_IF(ff_lookahead_check(op, ff_loop_rule_io{d->follows, d->L, d->flags, d->ntok}, S, *ahead));
    a.close_dist = ahead->exact ? nullptr : ahead->close_dist; a.cycle_len = ahead->cycle_len; a.budget = ahead->budget;
  }
  a.p.extra = d->mask_rows; a.p.ldextra = S;
  a.groups = groups; a.rows = d->mask_rows; a.follows = d->follows; a.L = d->L; a.fw = (d->L + 31) >> 5; a.flags = d->flags; a.ntok = d->ntok;
  a.score_in = d->scores_in; a.score_out = d->scores_out;
  a.fin_in = d->fin_in; a.dead_in = d->dead_in; a.first_in = d->first_in; a.prev_in = d->prev_in; a.visited_in = d->visited_in;
  a.fin_out = d->fin_out; a.dead_out = d->dead_out; a.first_out = d->first_out; a.prev_out = d->prev_out; a.visited_out = d->visited_out;
  a.parent = d->parent; a.tok = d->next_tok;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)io.rows * S * 14.0, st);
  const dim3 grid(ff_cdiv(groups, 4)), block(256);
  const int form = !ahead ? FF_LOOP_PLAIN : (ahead->exact ? FF_LOOP_EXACT : FF_LOOP_AHEAD);
  const int rc = ff_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(W, [&](auto w) {
    return ff_dispatch<FF_LOOP_PLAIN, FF_LOOP_AHEAD, FF_LOOP_EXACT>(form, [&](auto f) {
      hipLaunchKernelGGL((beam_constrained_select_kernel<decltype(w)::value, decltype(f)::value>), grid, block, 0, st, a);
      return FF_OK;
    });
  });
  FF_RETURN_IF(rc);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

namespace {
// the common operands of a one-step descriptor as the launch's step io
ff_step_io cbeam_step_io(const ff_beam_constrained_step* d) {
  return ff_step_io{d->logits, d->ldlogits, d->S, d->mask, d->kv_len, d->groups * d->width, d->groups_per_wireframe * d->width, d->term_lo,
                    d->term_hi, d->ntok, d->memory, d->E, d->next_rows, d->ldnext, d->next_stats, d->count_ge, nullptr, nullptr};
}
}  // namespace

extern "C" int ff_beam_constrained_select(const ff_beam_constrained_step* d, ff_stream_t stream) {
  const char* op = "ff_beam_constrained_select";
  FF_CHECK_ARG(d != nullptr, "%s: null descriptor", op);
  FF_RETURN_IF(ff_beam_check_sizes(op, d->groups, d->width, d->groups_per_wireframe, d->S));
  return ff_beam_constrained_select_sync(op, cbeam_step_io(d), d, nullptr, stream);
}

extern "C" int ff_beam_constrained_select_ahead(const ff_beam_constrained_ahead_step* da, ff_stream_t stream) {
  const char* op = "ff_beam_constrained_select_ahead";
  FF_CHECK_ARG(da != nullptr, "%s: null descriptor", op);
  const ff_beam_constrained_step* d = &da->step;
  FF_RETURN_IF(ff_beam_check_sizes(op, d->groups, d->width, d->groups_per_wireframe, d->S));
  FF_CHECK_ARG(da->lookahead == 1 || da->lookahead == 2, "%s: lookahead=%d must be 1 (look-ahead) or 2 (exact)", op, da->lookahead);
  const ff_lookahead_io ahead{da->lookahead == 1 ? da->close_dist : nullptr, da->cycle_len, da->budget, da->lookahead == 2 ? 1 : 0};
  return ff_beam_constrained_select_sync(op, cbeam_step_io(d), d, &ahead, stream);
}

int ff_constrain_beam_init(int* tok, float* score, int* fin, int* dead, int* parent, int* first, int* prev, unsigned* visited, int Bc,
                           int Fc, int W, int f0, const int* num_input, int pad_tok, int term_lo, int term_hi, int ntok,
                           const unsigned* follows, int L, hipStream_t st) {
  hipLaunchKernelGGL(cbeam_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, score, fin, dead, parent, first, prev, visited,
                     Bc, Fc, W, f0, num_input, pad_tok, term_lo, term_hi, ntok, follows, L, (L + 31) >> 5);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_constrain_beam_dead(const int* dead, int Btot, const int* steps_dev, const int* num_input, int dedup, int F, int W, int w0,
                           int nw, int Fc, int f0, int b0, int* dead_end, hipStream_t st) {
  const int total = nw * F * W;
  hipLaunchKernelGGL(cbeam_dead_kernel, dim3(ff_cdiv(total, 256) < 1024 ? ff_cdiv(total, 256) : 1024), dim3(256), 0, st, dead, Btot,
                     steps_dev, num_input, dedup, F, W, w0, nw, Fc, f0, b0, dead_end);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
