// Loop-constrained greedy selection over the pointer head (opt-in, parallel variant): the co-edge follow table,
// one step's constrained selection of every sequence, and the start state / output packing of a constrained decode.
//
// The rule (include/faceformer_hip.h states it on tokens): a face is one or more closed chains of co-edges, so a sequence with
// an OPEN loop (first != none) may only continue with an edge that starts where its last edge ends (CONNECT), never with an
// edge it holds already (NO_REPEAT) and never with a special token; when no such edge is left the terminators are opened
// instead and the sequence ends there, flagged as a dead end.  With the loop CLOSED the terminators and every unvisited edge
// are open.
//
// follow_table_kernel: one wavefront per (wireframe, edge a) row, 64 candidate edges b per round; the ballot of
// |end(a) - start(b)| < tol in x and in y (fp32 subtraction, fp32 compare) is the two 32-bit words of the round.
//
// The rule's device code is ff_select.h's, shared with the constrained beam kernel (ff_constrain_beam.hip): the byte row of a
// sequence's constraint mask with the "any live edge" vote and the terminators re-opened on a dead end (ff_loop_write_row), the
// three-step update of (first, prev) (ff_loop_advance) and the state after column 0 (ff_loop_start).
//
// pointer_constrained_form_kernel<FORM> (pointer_constrained_kernel<false> / <true> name its first two forms): one wavefront per
// sequence, four per block, as pointer_reduce_kernel.  A finished sequence appends
// token 0 and keeps its state.  Every other one writes the byte row of ITS constraint mask and then masks and reduces its logit
// row exactly as the greedy launch does with an extra mask (ff_pointer_mask_reduce<true>, ff_device.h): every lane reads back
// the bytes it wrote itself.  Lane 0 stores token, log-probability (-log sum exp(l - l[token]) over the constrained row), the
// flags and the next (first, prev), and sets the token's bit in the sequence's visited words; the wave appends memory[w, token]
// through ff_pointer_append_row, so a constrained decode keeps FF_L0_FOLD.  No LDS beyond the four counter words.  Stop counter:
// pointer_sample_kernel's scheme.
// pointer_constrained_kernel<true> is the same launch with the closure look-ahead: one byte row per sequence
// (close_dist[w][first] with the loop open, cycle_len[w] with it closed), one byte load and one compare per edge key in the loop
// that writes the byte row, in front of the vote.  <false> is what ff_pointer_constrained and ff_decode_constrained launch.
// pointer_constrained_form_kernel<FF_LOOP_EXACT> is the third form: an unfinished sequence with the loop open first
// runs one backward breadth-first search from its first edge over the edges it has not used (ff_loop_closure_reach, ff_select.h:
// a few words per lane, ballots and readlane, no LDS) and masks what cannot reach it within the budget; with the loop closed it
// is <true>'s cycle_len compare.  Layout and tail are the other forms'.
//
// follow_distance_kernel: one wavefront per (wireframe, source edge b), four per block: a breadth-first search FORWARD from b
// over the bit rows, which needs no transposed table.  Lane k holds words k, k + 64, ... of the reached, frontier and next sets
// (FD_CHUNKS of them: L <= 2048 * FD_CHUNKS); a level walks the frontier's set bits wave-uniformly and ORs the successors' rows
// into `next`, every word load coalesced and served from L2 (at most L rows of fw words per wave).  Each level stores the byte
// of the newly reached edges x to close_dist[w][x][b] -- plain byte stores with stride L, one per element of the table -- and
// b reached again is cycle_len[w][b].  What no level reached is stored as 255 at the end.
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"
#include "ff_select.h"

namespace {

struct ConstrainArgs {
  PointerArgs p;                 // logits / masks / memory / next rows / counters of the B launch rows; p.extra = rows
  unsigned char* rows;           // [B, S] out: the constraint byte row of every unfinished sequence (1 = masked)
  const unsigned* follows;       // [wireframes, L, fw] bits or null: bit b of row a = edge b starts where edge a ends
  int L, fw;                     // edges per wireframe (S - ntok), words per row ceil(L / 32)
  int flags, ntok;
  const int* fin_in;             // [B] nonzero: finished before this step
  const int* first_in;           // [B] first edge of the open loop, -1: none (closed)
  const int* prev_in;            // [B] last edge, -1: none
  unsigned* visited;             // [B, fw] in / out: the edges of the prefix
  int *fin_out, *first_out, *prev_out, *dead_out;   // [B] out
  int* tok; float* logprob;      // [B] out
  const unsigned char* close_dist;   // <true> only: [wireframes, L, L] bytes, close_dist[w][f][b] = D(b -> f)
  const unsigned char* cycle_len;    // <true>, exact: [wireframes, L] bytes, D(b -> b)
  int budget;                        // <true>, exact: T - 1 - the position this step selects
};

__global__ __launch_bounds__(256) void follow_table_kernel(const float* __restrict__ starts, const float* __restrict__ ends, int N,
                                                           int L, const int* __restrict__ num_input, float tol,
                                                           unsigned* __restrict__ bits) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + wv;
  if (row >= (long long)N * L) return;   // (wave-uniform)
  const int w = (int)(row / L), a = (int)(row % L), fw = (L + 31) >> 5;
  int n = num_input[w];
  n = n < 0 ? 0 : (n > L ? L : n);
  const float ex = ends[row * 2], ey = ends[row * 2 + 1];
  const float* sp = starts + (size_t)w * L * 2;
  unsigned* out = bits + row * fw;
  for (int c0 = 0; c0 < L; c0 += 64) {
    const int b = c0 + lane;
    bool ok = a < n && b < n;
    if (ok) ok = fabsf(ex - sp[b * 2]) < tol && fabsf(ey - sp[b * 2 + 1]) < tol;
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) {
      out[c0 >> 5] = (unsigned)bal;
      if ((c0 >> 5) + 1 < fw) out[(c0 >> 5) + 1] = (unsigned)(bal >> 32);
    }
  }
}

constexpr int FD_CHUNKS = 4;   // 64-word chunks of a bit row a lane holds: L <= 64 * 32 * FD_CHUNKS = 8192

__global__ __launch_bounds__(256) void follow_distance_kernel(const unsigned* __restrict__ follows, int N, int L,
                                                              const int* __restrict__ num_input, int hmax,
                                                              unsigned char* __restrict__ close_dist,
                                                              unsigned char* __restrict__ cycle_len) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long src = (long long)blockIdx.x * 4 + wv;
  if (src >= (long long)N * L) return;   // (wave-uniform)
  const int w = (int)(src / L), b = (int)(src % L), fw = (L + 31) >> 5;
  int n = num_input[w];
  n = n < 0 ? 0 : (n > L ? L : n);
  const unsigned* rows = follows + (size_t)w * L * fw;
  unsigned char* out = close_dist + (size_t)w * L * L + b;   // element x of this wave's column: out[x * L]
  unsigned valid[FD_CHUNKS], reached[FD_CHUNKS], frontier[FD_CHUNKS];   // (valid: the edges below num_input of this lane's words)
#pragma unroll
  for (int c = 0; c < FD_CHUNKS; ++c) {
    const int x0 = (c * 64 + lane) * 32;
    valid[c] = x0 >= n ? 0u : (n - x0 >= 32 ? 0xffffffffu : (1u << (n - x0)) - 1u);
    reached[c] = 0u;
    frontier[c] = (b < n && (b >> 5) == c * 64 + lane) ? 1u << (b & 31) : 0u;
  }
  int cyc = 255;
  for (int h = 1; h <= hmax; ++h) {
    unsigned next[FD_CHUNKS];
#pragma unroll
    for (int c = 0; c < FD_CHUNKS; ++c) next[c] = 0u;
#pragma unroll
    for (int c = 0; c < FD_CHUNKS; ++c) {
      unsigned long long lanes = __ballot(frontier[c] != 0u);
      while (lanes) {   // (wave-uniform walk: every frontier word, then every set bit of it)
        const int k = __builtin_ctzll(lanes);
        lanes &= lanes - 1;
        unsigned word = (unsigned)__builtin_amdgcn_readlane((int)frontier[c], k);
        while (word) {
          const int x = (c * 64 + k) * 32 + __builtin_ctz(word);   // (< n <= L: valid[] cleared everything else)
          word &= word - 1;
          const unsigned* xr = rows + (size_t)x * fw;
#pragma unroll
          for (int c2 = 0; c2 < FD_CHUNKS; ++c2)
            if (c2 * 64 + lane < fw) next[c2] |= xr[c2 * 64 + lane];
        }
      }
    }
    bool any = false, self = false;   // self: the search came back to b, in the one lane that holds b's word
#pragma unroll
    for (int c = 0; c < FD_CHUNKS; ++c) {
      next[c] &= valid[c] & ~reached[c];
      reached[c] |= next[c];
      frontier[c] = next[c];
      any = any || next[c] != 0u;
      self = self || ((b >> 5) == c * 64 + lane && ((next[c] >> (b & 31)) & 1u) != 0u);
      unsigned word = next[c];
      while (word) {   // the bytes of the newly reached edges
        const int x = (c * 64 + lane) * 32 + __builtin_ctz(word);
        word &= word - 1;
        out[(size_t)x * L] = (unsigned char)h;
      }
    }
    if (__ballot(self) != 0ull) cyc = h;
    if (__ballot(any) == 0ull) break;
  }
#pragma unroll
  for (int c = 0; c < FD_CHUNKS; ++c) {   // what no level reached, the rows at and beyond num_input included
    const int x0 = (c * 64 + lane) * 32;
    for (int j = 0; j < 32 && x0 + j < L; ++j)
      if (!((reached[c] >> j) & 1u)) out[(size_t)(x0 + j) * L] = 255;
  }
  if (lane == 0) cycle_len[(size_t)w * L + b] = (unsigned char)cyc;
}

// One kernel per compile-time form of the rule (FF_LOOP_PLAIN / FF_LOOP_AHEAD / FF_LOOP_EXACT, ff_select.h).
template <int FORM>
__global__ __launch_bounds__(256) void pointer_constrained_form_kernel(ConstrainArgs a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
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
      ff_pointer_mask_reduce<true>(pa, b, lane, &m, &b2, &tok, &lsum);
      lp = -logf(lsum);
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

// The two forms without a search under the names they are launched by: <false> is FF_LOOP_PLAIN, <true> FF_LOOP_AHEAD.
template <bool AHEAD>
constexpr auto pointer_constrained_kernel = pointer_constrained_form_kernel<AHEAD ? FF_LOOP_AHEAD : FF_LOOP_PLAIN>;

// ---- engine side: start state and output packing of a constrained decode (ff_engine.hip) -----------------------------------------
// Start state of one micro-batch of Bc = nw * Fc sequences (compact anchors [f0, f0 + Fc) of every wireframe): the anchor's
// start token (model_para.py:201-205), log-probability 0, and the rule's state after column 0 -- a start token below ntok
// leaves it empty; an edge is visited, is prev and opens a loop unless it closes on itself.  A start token in the terminator
// range finishes the sequence at position 0 (the padding anchors).
__global__ void constrain_init_kernel(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int Bc,
                                      int Fc, int f0, const int* num_input, int pad_tok, int term_lo, int term_hi, int ntok,
                                      const unsigned* follows, int L, int fw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bc) return;
  const int wl = i / Fc, f = f0 + i % Fc;
  int done;
  const int t = ff_start_token(f, num_input[wl], pad_tok, term_lo, term_hi, &done);
  tok[i] = t;
  lp[i] = 0.f;
  fin[i] = done;
  dead[i] = 0;
  int fi, pv;
  ff_loop_start(t, ntok, follows, wl, L, fw, visited + (size_t)i * fw, &fi, &pv);
  first[i] = fi;
  prev[i] = pv;
}

// predict[(w, fo), :], logprob (same layout) and dead_end[(w, fo)] from the per-step records (tok, lp, fin, dead: [T, Btot],
// row s = the state after s steps).  Position j is kept when j <= the stop step and the sequence was not finished before it:
// last = min(finish position, stop step); rows behind the stop step are never looked at, so the result does not depend on
// when the host saw the stop.  Rows fo >= num_input[w] of a de-duplicated decode read the one padding-anchor sequence.
__global__ void constrain_finalize_kernel(const int* __restrict__ tok, const float* __restrict__ lp, const int* __restrict__ fin,
                                          const int* __restrict__ dead, int Btot, int T, const int* __restrict__ steps_p,
                                          const int* __restrict__ num_input, int dedup, int F, int w0, int nw, int Fc, int f0, int b0,
                                          int64_t* __restrict__ predict, float* __restrict__ logprob, int* __restrict__ dead_end,
                                          int* __restrict__ seq_of_row) {
  const int steps = *steps_p;
  const int total = nw * F;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int fo = i % F, wl = i / F;
    int a;
    if (!ff_compact_seq(num_input, dedup, w0, wl, fo, Fc, f0, &a)) continue;
    const int seq = b0 + a;
    const size_t row = (size_t)(w0 + wl) * F + fo;
    int64_t* out = predict + row * T;
    float* olp = logprob + row * T;
    int de = 0;
    bool done = false;   // finished before position j
    for (int j = 0; j < T; ++j) {
      const bool in = j <= steps && !done;
      out[j] = in ? tok[(size_t)j * Btot + seq] : 0;
      olp[j] = (in && j >= 1) ? lp[(size_t)j * Btot + seq] : 0.f;
      if (in) { de |= dead[(size_t)j * Btot + seq]; done = fin[(size_t)j * Btot + seq] != 0; }
    }
    dead_end[row] = de;
    if (seq_of_row) seq_of_row[row] = seq;
  }
}

}  // namespace

extern "C" int ff_follow_table(const float* starts, const float* ends, int N, int L, const int* num_input, float tol,
                               unsigned* bits, ff_stream_t stream) {
  if (N == 0 || L == 0) return FF_OK;
  FF_CHECK_ARG(N > 0 && L > 0 && starts && ends && num_input && bits, "ff_follow_table: bad sizes N=%d L=%d or a null pointer", N, L);
  FF_CHECK_ARG(tol >= 0.f && ((long long)N * L + 3) / 4 < (1LL << 31), "ff_follow_table: tol=%g must be >= 0, N*L below 2^33", (double)tol);
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_ROWOP, (double)N * L * L, st);
  hipLaunchKernelGGL(follow_table_kernel, dim3((unsigned)(((long long)N * L + 3) / 4)), dim3(256), 0, st, starts, ends, N, L,
                     num_input, tol, bits);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_loop_rule_check(const char* op, const ff_loop_rule_io& r, int S, int term_lo, int term_hi) {
  FF_CHECK_ARG(!(r.flags & ~(FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT)), "%s: unknown flag bits %d", op, r.flags);
  FF_CHECK_ARG(r.ntok >= 0 && r.L >= 0 && r.L == S - r.ntok, "%s: L=%d must be S - ntok = %d - %d", op, r.L, S, r.ntok);
  FF_CHECK_ARG(term_lo >= 0 && term_lo < term_hi && term_hi <= r.ntok, "%s: terminator range [%d, %d) empty or outside the %d special tokens",
               op, term_lo, term_hi, r.ntok);
  FF_CHECK_ARG(r.follows || !(r.flags & FF_CONSTRAIN_CONNECT), "%s: FF_CONSTRAIN_CONNECT needs the follow table", op);
  return FF_OK;
}

// What a look-ahead adds to a constrained step's checks, for operator `op`: the flag bits its form needs, its tables, the budget's
// range and, for the exact form, the key limit of its search.
int ff_lookahead_check(const char* op, const ff_loop_rule_io& rule, int S, const ff_lookahead_io& ahead) {
  if (ahead.exact) {
    FF_CHECK_ARG((rule.flags & FF_CONSTRAIN_CONNECT) && (rule.flags & FF_CONSTRAIN_NO_REPEAT),
                 "%s: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT", op);
    FF_CHECK_ARG(ahead.cycle_len, "%s: cycle_len is required", op);
    FF_CHECK_ARG(S <= FF_EXACT_MAX_S, "%s: S=%d above %d keys (L + ntok)", op, S, FF_EXACT_MAX_S);
  } else {
    FF_CHECK_ARG(rule.flags & FF_CONSTRAIN_CONNECT, "%s: the look-ahead needs FF_CONSTRAIN_CONNECT", op);
    FF_CHECK_ARG(ahead.close_dist && ahead.cycle_len, "%s: close_dist and cycle_len are required", op);
  }
  FF_CHECK_ARG(ahead.budget >= 0 && ahead.budget <= 254, "%s: budget=%d outside 0..254", op, ahead.budget);
  return FF_OK;
}

// The one launch behind ff_pointer_constrained (ahead = null), ff_pointer_constrained_ahead and ff_pointer_constrained_exact
// (ahead->exact); `op` words the errors.
int ff_pointer_constrained_sync(const char* op, const ff_step_io& io, const ff_loop_rule_io& rule, const ff_constrained_state& s,
                                const ff_lookahead_io* ahead, ff_stream_t stream) {
  const int B = io.rows, S = io.S;
  if (B == 0) return FF_OK;
  FF_CHECK_ARG(B > 0 && S > 0 && io.rows_per_wireframe > 0, "%s: bad sizes B=%d S=%d", op, B, S);
  ConstrainArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(ff_step_args(&a.p, op, true, io));
  FF_RETURN_IF(ff_loop_rule_check(op, rule, S, io.term_lo, io.term_hi));
  FF_CHECK_ARG(s.fin_in && s.first_in && s.prev_in && s.visited && s.mask_rows && s.next_tok && s.logprob && s.fin_out && s.dead_end &&
                   s.first_out && s.prev_out, "%s: null pointer", op);
  if (ahead) {
    FF_RETURN_IF(ff_lookahead_check(op, rule, S, *ahead));
    a.close_dist = ahead->exact ? nullptr : ahead->close_dist; a.cycle_len = ahead->cycle_len; a.budget = ahead->budget;
  }
  a.p.extra = s.mask_rows; a.p.ldextra = S;
  a.rows = s.mask_rows; a.follows = rule.follows; a.L = rule.L; a.fw = (rule.L + 31) >> 5; a.flags = rule.flags; a.ntok = rule.ntok;
  a.fin_in = s.fin_in; a.first_in = s.first_in; a.prev_in = s.prev_in; a.visited = s.visited;
  a.fin_out = s.fin_out; a.first_out = s.first_out; a.prev_out = s.prev_out; a.dead_out = s.dead_end;
  a.tok = s.next_tok; a.logprob = s.logprob;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)B * S * 4.0, st);
  if (ahead && !ahead->exact)
    hipLaunchKernelGGL(pointer_constrained_kernel<true>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  else if (!ahead)
    hipLaunchKernelGGL(pointer_constrained_kernel<false>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(pointer_constrained_form_kernel<FF_LOOP_EXACT>, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" int ff_pointer_constrained_ahead(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                            int seqs_per_group, const unsigned* follows, int L, int flags, int ntok, int term_lo,
                                            int term_hi, const int* fin_in, const int* first_in, const int* prev_in,
                                            unsigned* visited, unsigned char* mask_rows, int* next_tok, float* logprob, int* fin_out,
                                            int* dead_end, int* first_out, int* prev_out, const float* memory, int E,
                                            float* next_rows, int ldnext, float* next_stats, int* count_ge,
                                            const unsigned char* close_dist, const unsigned char* cycle_len, int budget,
                                            ff_stream_t stream) {
  const ff_lookahead_io ahead{close_dist, cycle_len, budget, 0};
  return ff_pointer_constrained_sync(
      "ff_pointer_constrained_ahead",
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, term_lo, term_hi, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_ge, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      &ahead, stream);
}

extern "C" int ff_pointer_constrained_exact(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                            int seqs_per_group, const unsigned* follows, int L, int flags, int ntok, int term_lo,
                                            int term_hi, const int* fin_in, const int* first_in, const int* prev_in,
                                            unsigned* visited, unsigned char* mask_rows, int* next_tok, float* logprob, int* fin_out,
                                            int* dead_end, int* first_out, int* prev_out, const float* memory, int E,
                                            float* next_rows, int ldnext, float* next_stats, int* count_ge,
                                            const unsigned char* cycle_len, int budget, ff_stream_t stream) {
  const ff_lookahead_io exact{nullptr, cycle_len, budget, 1};
  return ff_pointer_constrained_sync(
      "ff_pointer_constrained_exact",
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, term_lo, term_hi, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_ge, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      &exact, stream);
}

extern "C" int ff_follow_distance(const unsigned* follows, int N, int L, const int* num_input, int hmax, unsigned char* close_dist,
                                  unsigned char* cycle_len, ff_stream_t stream) {
  FF_CHECK_ARG(hmax >= 1 && hmax <= 254, "ff_follow_distance: hmax=%d outside 1..254", hmax);
  if (N == 0 || L == 0) return FF_OK;
  FF_CHECK_ARG(N > 0 && L > 0 && follows && num_input && close_dist && cycle_len, "ff_follow_distance: bad sizes N=%d L=%d or a null pointer", N, L);
  FF_CHECK_ARG(L <= 2048 * FD_CHUNKS && ((long long)N * L + 3) / 4 < (1LL << 31), "ff_follow_distance: L=%d above %d, or N*L not below 2^33", L,
               2048 * FD_CHUNKS);
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_ROWOP, (double)N * L * L, st);
  hipLaunchKernelGGL(follow_distance_kernel, dim3((unsigned)(((long long)N * L + 3) / 4)), dim3(256), 0, st, follows, N, L, num_input,
                     hmax, close_dist, cycle_len);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" int ff_pointer_constrained(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                      int seqs_per_group, const unsigned* follows, int L, int flags, int ntok, int term_lo,
                                      int term_hi, const int* fin_in, const int* first_in, const int* prev_in, unsigned* visited,
                                      unsigned char* mask_rows, int* next_tok, float* logprob, int* fin_out, int* dead_end,
                                      int* first_out, int* prev_out, const float* memory, int E, float* next_rows, int ldnext,
                                      float* next_stats, int* count_ge, ff_stream_t stream) {
  return ff_pointer_constrained_sync(
      "ff_pointer_constrained",
      ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, term_lo, term_hi, ntok, memory, E, next_rows, ldnext, next_stats,
                 count_ge, nullptr, nullptr},
      ff_loop_rule_io{follows, L, flags, ntok},
      ff_constrained_state{fin_in, first_in, prev_in, visited, mask_rows, next_tok, logprob, fin_out, dead_end, first_out, prev_out},
      nullptr, stream);
}

int ff_constrain_init(int* tok, float* lp, int* fin, int* dead, int* first, int* prev, unsigned* visited, int Bc, int Fc, int f0,
                      const int* num_input, int pad_tok, int term_lo, int term_hi, int ntok, const unsigned* follows, int L,
                      hipStream_t st) {
  hipLaunchKernelGGL(constrain_init_kernel, dim3(ff_cdiv(Bc, 256)), dim3(256), 0, st, tok, lp, fin, dead, first, prev, visited, Bc, Fc,
                     f0, num_input, pad_tok, term_lo, term_hi, ntok, follows, L, (L + 31) >> 5);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_constrain_finalize(const int* tok, const float* lp, const int* fin, const int* dead, int Btot, int T, const int* steps_dev,
                          const int* num_input, int dedup, int F, int w0, int nw, int Fc, int f0, int b0, int64_t* predict,
                          float* logprob, int* dead_end, int* seq_of_row, hipStream_t st) {
  const int total = nw * F;
  hipLaunchKernelGGL(constrain_finalize_kernel, dim3(ff_cdiv(total, 256) < 1024 ? ff_cdiv(total, 256) : 1024), dim3(256), 0, st, tok,
                     lp, fin, dead, Btot, T, steps_dev, num_input, dedup, F, w0, nw, Fc, f0, b0, predict, logprob, dead_end, seq_of_row);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
