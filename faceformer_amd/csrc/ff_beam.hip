// Beam search over the pointer head (opt-in, parallel variant): one step's top-W selection over the W x S
// candidates of every group (the W beams of one anchor), and the prefix reorder that follows it.
//
// beam_select_kernel<W, FORM>: one wavefront per group.  For each non-empty unfinished beam it masks and reduces the raw logit row
// exactly as pointer_reduce_kernel does (ff_pointer_mask_reduce<true>, ff_device.h: the row maximum m and sum exp(l - m)), every
// lane then walks its strided keys once more and keeps the W best candidates c_k + (l[s] - m) - log(sum) in the sorted register
// list of ff_select.h (insert, walk, butterfly merge, "lane k takes rank k": shared with the constrained beam kernel).
// Lanes 0..W-1 then own one new beam each (parent, token, score, finished flag), the wave permutes the group's token history
// in place, appends the next decoder input rows memory[w, token] and adds to the launch's stop counter.
//
// L0 fold: the appended rows are written by ff_pointer_append_row, the greedy pointer launch's own gather, so they carry their
// LayerNorm segment statistics when the engine asks for them (FF_L0_FOLD): a beam decode folds layer 0 as a greedy one does.
//
// Sequence forms (opt-in, single-sequence variant): beam_select_kernel<W, FORM> is one launch in three compile-time
// forms that differ ONLY in what a wave adds to the stop counter.  FORM 0 is the parallel decode's launch as it always was (kept
// candidates of unfinished beams with a token >= ge_bound).  FORM 1 ("all") adds the group's non-empty beams that are UNFINISHED
// AFTER this step; FORM 2 ("best") adds 1 when the group's rank 0 is unfinished after it.  All W beams of a single-sequence decode
// can select SEP in one step, so the parallel count would stop them.  sequence_beam_init_kernel is the start state (every beam at
// SOS, beam 0 with score 0: no anchors, no padding groups); the packing is beam_finalize_kernel with F = 1, which then also
// writes the finished flags of the stop step's row.
//
// beam_reorder_kernel: one block per (position, group) moves rows[j][g][k] <- rows[j][g][parent[k]] of up to two row arrays
// (the engine's x0 and layer-0 q|k|v) in place through LDS; a group whose parent map is the identity returns at once.
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"
#include "ff_select.h"

namespace {

struct BeamArgs {
  PointerArgs p;            // logits / masks / memory / next rows of the B = groups * W launch rows, spg = beams per wireframe
  int groups;
  const float* score_in; float* score_out;
  const int* fin_in; int* fin_out;
  int* hist; int ldhist, t;  // token history [t, ldhist] (positions 0..t-1 filled; this step writes position t), or null
  int* parent; int* tok;     // [B] out
};

template <int W, int FORM>
__global__ __launch_bounds__(256) void beam_select_kernel(BeamArgs a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  int nge = 0;
  if (g < a.groups) {
    const int S = pa.S, b0 = g * W;
    // lane k < W holds beam k's state; the loops below broadcast it
    const float my_c = lane < W ? a.score_in[b0 + lane] : -INFINITY;
    const int my_f = lane < W ? a.fin_in[b0 + lane] : 0;
    float lsc[W];
    int lix[W];
    ff_beam_list_init<W>(lsc, lix);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float c = __shfl(my_c, k, FF_WAVE);
      const int f = __shfl(my_f, k, FF_WAVE);
      if (c == -INFINITY) continue;                      // empty beam: no candidates (wave-uniform)
      if (f) {                                           // finished: itself, token 0, score unchanged
        if (lane == 0) ff_beam_insert<W>(lsc, lix, c, k * S);
        continue;
      }
      float m, b2, lsum;
      int i1;
      ff_pointer_mask_reduce<true>(pa, b0 + k, lane, &m, &b2, &i1, &lsum);
      const float logz = logf(lsum);
      ff_beam_walk<W, false>(lsc, lix, pa.logits + (size_t)(b0 + k) * pa.ldlogits, S, lane, k, c, m, logz);
    }
    ff_beam_merge<W>(lsc, lix);
    float sc;
    int ix;
    ff_beam_rank<W>(lsc, lix, lane, &sc, &ix);
    const bool some = lane < W && ix != FF_BEAM_NONE;
    const int par = some ? ix / S : (lane < W ? lane : 0);
    const int pfin = __shfl(my_f, par, FF_WAVE);
    const int tk = (some && !pfin) ? ix - par * S : 0;
    const int nfin = some ? (pfin || (tk >= pa.term_lo && tk < pa.term_hi) ? 1 : 0) : 0;
    if (FORM == 0) nge = __popcll(__ballot(some && !pfin && tk >= pa.ge_bound));
    else if (FORM == 1) nge = __popcll(__ballot(some && !nfin));   // non-empty beams unfinished after this step
    else nge = (int)(__ballot(some && !nfin) & 1ull);              // the group's rank 0 unfinished after this step
    if (a.hist) {
      // positions are independent of each other: 64 / W of them per pass, every lane loads its entry before any lane stores
      const int ppp = 64 / W, k = lane % W, jl = lane / W;
      const int src = __shfl(par, k, FF_WAVE);
      for (int j0 = 0; j0 < a.t; j0 += ppp) {
        const int j = j0 + jl;
        const bool in = jl < ppp && j < a.t;
        int v = 0;
        if (in) v = a.hist[(size_t)j * a.ldhist + b0 + src];
        __builtin_amdgcn_wave_barrier();
        if (in) a.hist[(size_t)j * a.ldhist + b0 + k] = v;
      }
      if (lane < W) a.hist[(size_t)a.t * a.ldhist + b0 + lane] = tk;
    }
    if (lane < W) {
      a.parent[b0 + lane] = par;
      a.tok[b0 + lane] = tk;
      a.score_out[b0 + lane] = sc;
      a.fin_out[b0 + lane] = nfin;
    }
    if (pa.next_rows) {
#pragma unroll
      for (int k = 0; k < W; ++k) ff_pointer_append_row(pa, (b0 + k) / pa.spg, b0 + k, __shfl(tk, k, FF_WAVE), lane);
    }
  }
  ff_pointer_count_waves(pa, a.groups, nge);
}

// rows_a [npos, rows_per_pos, wa] and (optional) rows_b [npos, rows_per_pos, wb]; row (j, g * W + k) <- row (j, g * W + parent[k]).
// The group's W source rows of both arrays are staged in LDS (W * (wa + wb) floats), then the rows that move are written back.
__global__ __launch_bounds__(256) void beam_reorder_kernel(float* __restrict__ rows_a, int wa, float* __restrict__ rows_b, int wb,
                                                           int rows_per_pos, const int* __restrict__ parent, int W) {
  extern __shared__ f32x4 lds[];
  const int g = blockIdx.x, j = blockIdx.y;
  int par[FF_BEAM_MAX_W];
  bool ident = true;
#pragma unroll
  for (int k = 0; k < FF_BEAM_MAX_W; ++k) {
    par[k] = k < W ? min(max(parent[g * W + k], 0), W - 1) : k;   // (a caller's parent outside 0..W-1 stays inside the staged rows)
    ident = ident && par[k] == k;
  }
  if (ident) return;   // (block-uniform)
  const int va = wa >> 2, vb = wb >> 2, vw = va + vb;   // 16-byte units per row of a, of b, of a staged row pair
  f32x4* ra = reinterpret_cast<f32x4*>(rows_a) + ((size_t)j * rows_per_pos + (size_t)g * W) * va;
  f32x4* rb = rows_b ? reinterpret_cast<f32x4*>(rows_b) + ((size_t)j * rows_per_pos + (size_t)g * W) * vb : nullptr;
  for (int i = threadIdx.x; i < W * vw; i += blockDim.x) {
    const int k = i / vw, c = i - k * vw;
    lds[i] = c < va ? ra[(size_t)k * va + c] : rb[(size_t)k * vb + (c - va)];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < FF_BEAM_MAX_W; ++k) {
    if (k >= W || par[k] == k) continue;
    const f32x4* src = lds + par[k] * vw;
    for (int c = threadIdx.x; c < vw; c += blockDim.x) {
      if (c < va) ra[(size_t)k * va + c] = src[c];
      else rb[(size_t)k * vb + (c - va)] = src[c];
    }
  }
}

// ---- engine side: start state and output packing of a beam decode (ff_engine.hip) ------------------------------------------------
// Start state of one micro-batch of Bc = nw * Fc * W beams (Fc anchors per wireframe, compact anchors [f0, f0 + Fc)): every beam
// of a group holds the group's start token (model_para.py:201-205); beam 0 has score 0, the others are empty (-inf); a start
// token in the terminator range finishes the beam at position 0.
__global__ void beam_init_kernel(int* tok, float* score, int* fin, int* parent, int Bc, int Fc, int W, int f0,
                                 const int* num_input, int pad_tok, int term_lo, int term_hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  const int k = i % W, a = i / W;
  int done;
  tok[i] = ff_start_token(f0 + a % Fc, num_input[a / Fc], pad_tok, term_lo, term_hi, &done);
  score[i] = k == 0 ? 0.f : -INFINITY;
  fin[i] = done;
  parent[i] = k;
}

// Start state of one micro-batch of the sequence forms: Bc = nw * W beams, beam k of the chunk's wl-th wireframe at i = wl * W + k.
// Every beam holds SOS (model.py:191), unfinished; beam 0 has score 0, the others are empty (-inf).
__global__ void sequence_beam_init_kernel(int* tok, float* score, int* fin, int* parent, int Bc, int W, int sos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  const int k = i % W;
  tok[i] = sos;
  score[i] = k == 0 ? 0.f : -INFINITY;
  fin[i] = 0;
  parent[i] = k;
}

// beams[(w, fo, k), :], scores and predict[(w, fo), :] = beam 0, from the per-step records (tok, parent: [T, Btot]; score:
// [T, Btot], row s = the state after s steps).  The arrangement is the one after `steps` steps, the tokens come from walking
// the parents back -- steps the host had enqueued past the stop step are never looked at, so the result does not depend on
// when the host saw the stop.  Rows fo >= num_input[w] of a de-duplicated decode read the one padding-anchor group.
// finished (optional, with fin [T, Btot]): the beams' finished flags of the stop step's row, in the beams' order.
__global__ void beam_finalize_kernel(const int* __restrict__ tok, const int* __restrict__ parent, const float* __restrict__ score,
                                     int Btot, int T, const int* __restrict__ steps_p, const int* __restrict__ num_input, int dedup,
                                     int F, int W, int w0, int nw, int Fc, int f0, int b0, int64_t* __restrict__ beams,
                                     float* __restrict__ scores, int64_t* __restrict__ predict, int* __restrict__ seq_of_row,
                                     const int* __restrict__ fin, int* __restrict__ finished) {
  const int steps = *steps_p;
  const int total = nw * F * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int k = i % W, fo = (i / W) % F, wl = i / (W * F);
    int a;
    if (!ff_compact_seq(num_input, dedup, w0, wl, fo, Fc, f0, &a)) continue;
    const int grp = b0 + a * W;
    const size_t row = ((size_t)(w0 + wl) * F + fo) * W + k;
    int64_t* out = beams + row * T;
    int64_t* pred = k == 0 ? predict + ((size_t)(w0 + wl) * F + fo) * T : nullptr;
    for (int j = steps + 1; j < T; ++j) { out[j] = 0; if (pred) pred[j] = 0; }
    int cur = k;
    for (int s = steps; s >= 0; --s) {
      const int v = tok[(size_t)s * Btot + grp + cur];
      out[s] = v;
      if (pred) pred[s] = v;
      cur = s > 0 ? parent[(size_t)s * Btot + grp + cur] : cur;
    }
    scores[row] = score[(size_t)steps * Btot + grp + k];
    if (finished) finished[row] = fin[(size_t)steps * Btot + grp + k];
    if (seq_of_row) seq_of_row[row] = grp + k;
  }
}

}  // namespace

int ff_beam_check_sizes(const char* op, int groups, int width, int groups_per_wireframe, int S) {
  FF_CHECK_ARG(width >= 1 && width <= FF_BEAM_MAX_W && width <= S, "%s: width=%d outside 1..%d or above S=%d", op, width, FF_BEAM_MAX_W, S);
  FF_CHECK_ARG(groups > 0 && S > 0 && groups_per_wireframe > 0 && (long long)groups * width < (1LL << 31), "%s: bad sizes groups=%d S=%d", op,
               groups, S);
  return FF_OK;
}

int ff_beam_select_sync(const ff_step_io& io, int width, const float* scores_in, float* scores_out, const int* fin_in, int* fin_out,
                        int* hist, int ldhist, int t, int* parent, int* next_tok, ff_stream_t stream, int form) {
  const char* op = form ? "ff_beam_sequence_select" : "ff_beam_select";
  const int S = io.S, groups = io.rows / width;
  BeamArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(ff_step_args(&a.p, op, false, io));
  FF_CHECK_ARG(scores_in && scores_out && fin_in && fin_out && parent && next_tok, "%s: null pointer", op);
  FF_CHECK_ARG(!hist || (t >= 1 && ldhist >= io.rows), "%s: history needs t >= 1 and ldhist >= groups * width", op);
  a.groups = groups; a.score_in = scores_in; a.score_out = scores_out; a.fin_in = fin_in; a.fin_out = fin_out;
  a.hist = hist; a.ldhist = ldhist; a.t = t; a.parent = parent; a.tok = next_tok;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)io.rows * S * 12.0, st);
  const dim3 grid(ff_cdiv(groups, 4)), block(256);
  const int rc = ff_dispatch<1, 2, 3, 4, 5, 6, 7, 8>(width, [&](auto w) {
    return ff_dispatch<0, 1, 2>(form, [&](auto f) {
      hipLaunchKernelGGL((beam_select_kernel<decltype(w)::value, decltype(f)::value>), grid, block, 0, st, a);
      return FF_OK;
    });
  });
  FF_RETURN_IF(rc);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" int ff_beam_select(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int groups,
                              int width, int groups_per_wireframe, const float* scores_in, float* scores_out, const int* fin_in,
                              int* fin_out, int* hist, int ldhist, int t, int* parent, int* next_tok, int term_lo, int term_hi,
                              const float* memory, int E, float* next_rows, int ldnext, int* count_ge, int ge_bound,
                              ff_stream_t stream) {
  FF_RETURN_IF(ff_beam_check_sizes("ff_beam_select", groups, width, groups_per_wireframe, S));
  return ff_beam_select_sync(ff_step_io{logits, ldlogits, S, mask, kv_len, groups * width, groups_per_wireframe * width, term_lo,
                                        term_hi, ge_bound, memory, E, next_rows, ldnext, nullptr, count_ge, nullptr, nullptr},
                             width, scores_in, scores_out, fin_in, fin_out, hist, ldhist, t, parent, next_tok, stream);
}

// The sequence forms of the step (single-sequence variant): ff_beam_select's arguments without ge_bound; count_unfinished += the
// non-empty beams unfinished after the step, or with stop_best the groups whose rank 0 is unfinished after it.
extern "C" int ff_beam_sequence_select(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int groups,
                                       int width, int groups_per_wireframe, const float* scores_in, float* scores_out,
                                       const int* fin_in, int* fin_out, int* hist, int ldhist, int t, int* parent, int* next_tok,
                                       int term_lo, int term_hi, const float* memory, int E, float* next_rows, int ldnext,
                                       int* count_unfinished, int stop_best, ff_stream_t stream) {
  FF_RETURN_IF(ff_beam_check_sizes("ff_beam_sequence_select", groups, width, groups_per_wireframe, S));
  FF_CHECK_ARG(term_lo < term_hi, "ff_beam_sequence_select: empty terminator range [%d, %d)", term_lo, term_hi);
  FF_CHECK_ARG(stop_best == 0 || stop_best == 1, "ff_beam_sequence_select: stop_best=%d must be 0 or 1", stop_best);
  return ff_beam_select_sync(ff_step_io{logits, ldlogits, S, mask, kv_len, groups * width, groups_per_wireframe * width, term_lo,
                                        term_hi, 0, memory, E, next_rows, ldnext, nullptr, count_unfinished, nullptr, nullptr},
                             width, scores_in, scores_out, fin_in, fin_out, hist, ldhist, t, parent, next_tok, stream,
                             stop_best ? 2 : 1);
}

extern "C" int ff_beam_reorder(float* rows_a, int width_a, float* rows_b, int width_b, int rows_per_pos, int npos,
                               const int* parent, int groups, int width, ff_stream_t stream) {
  if (npos == 0 || groups == 0) return FF_OK;
  FF_CHECK_ARG(width >= 1 && width <= FF_BEAM_MAX_W, "ff_beam_reorder: width=%d outside 1..%d", width, FF_BEAM_MAX_W);
  FF_CHECK_ARG(npos > 0 && npos <= 65535 && groups > 0 && (long long)groups * width <= rows_per_pos, "ff_beam_reorder: bad sizes npos=%d groups=%d", npos, groups);
  FF_CHECK_ARG(rows_a && parent && width_a > 0 && (width_a & 3) == 0 && ff_aligned16(rows_a), "ff_beam_reorder: rows_a must be 16-byte rows");
  FF_CHECK_ARG(rows_b ? (width_b > 0 && (width_b & 3) == 0 && ff_aligned16(rows_b)) : width_b == 0, "ff_beam_reorder: rows_b must be 16-byte rows (or null with width 0)");
  const size_t lds = (size_t)width * (size_t)(width_a + width_b) * sizeof(float);
  FF_CHECK_ARG(lds <= 65536, "ff_beam_reorder: %zu bytes of rows per group exceed the 64 KB staging area", lds);
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_ROWOP, (double)npos * groups * width * (width_a + width_b) * 8.0, st);
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(groups, npos), dim3(256), lds, st, rows_a, width_a, rows_b, width_b, rows_per_pos,
                     parent, width);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_beam_init(int* tok, float* score, int* fin, int* parent, int Bc, int Fc, int W, int f0, const int* num_input, int pad_tok,
                 int term_lo, int term_hi, hipStream_t st) {
  hipLaunchKernelGGL(beam_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, score, fin, parent, Bc, Fc, W, f0, num_input,
                     pad_tok, term_lo, term_hi);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_sequence_beam_init(int* tok, float* score, int* fin, int* parent, int Bc, int W, int sos, hipStream_t st) {
  hipLaunchKernelGGL(sequence_beam_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, score, fin, parent, Bc, W, sos);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_beam_finalize(const int* tok, const int* parent, const float* score, int Btot, int T, const int* steps_dev,
                     const int* num_input, int dedup, int F, int W, int w0, int nw, int Fc, int f0, int b0, int64_t* beams,
                     float* scores, int64_t* predict, int* seq_of_row, hipStream_t st, const int* fin, int* finished) {
  const int total = nw * F * W;
  hipLaunchKernelGGL(beam_finalize_kernel, dim3(ff_cdiv(total, 256) < 1024 ? ff_cdiv(total, 256) : 1024), dim3(256), 0, st, tok,
                     parent, score, Btot, T, steps_dev, num_input, dedup, F, W, w0, nw, Fc, f0, b0, beams, scores, predict, seq_of_row,
                     fin, finished);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
