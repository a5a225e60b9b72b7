// Teacher-forced scoring of given token paths (opt-in): the decode loop fed a path instead of its own argmax.
//
// pointer_forced_kernel: one wavefront per sequence, four per block, as pointer_reduce_kernel.  The wave masks and reduces the
// raw logit row exactly as the greedy launch does (ff_pointer_mask_reduce<true>, ff_device.h: row maximum m, runner-up, argmax
// with torch's tie rule, sum exp(l - m)), reads the forced key's masked logit l[g], walks its strided keys once more for the
// rank of g (keys above l[g], or equal to it at a lower index) and sums the lanes' counts with a butterfly -- a fixed tree of
// integer adds, the same on every run.  Lane 0 stores logprob = (l[g] - m) - log sum, saturated at -FLT_MAX, the argmax and the
// rank; the wave then appends the next decoder input row memory[w, g] -- the FORCED token's row, never the argmax's -- through
// ff_pointer_append_row, so the row carries its LayerNorm segment statistics and a forced decode keeps FF_L0_FOLD.
// No counters, no atomics, no LDS.
//
// forced_tokens_kernel: paths [rows, T] int64 -> tok [T, rows] int32, the position-major order of the engine's token array,
// every token clamped into [0, S) (the C entries cannot see device data: a token outside would index outside `memory`).
//
// forced_finalize_kernel: the per-step records [T-1, rows] -> logprob / greedy / rank [rows, T] under the `lengths` rule, and
// the per-row sums; one thread per row adds its positions in ascending order (fp64 accumulator, rounded once).
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"

namespace {

struct ForcedArgs {
  PointerArgs p;            // logits / masks / memory / next rows of the B launch rows (no counters, no slot map)
  const int* forced;        // [B] the token every row is forced to (clamped into [0, S) here as well)
  float* logprob;           // [B] out
  int* greedy; int* rank;   // [B] out
};

__global__ __launch_bounds__(256) void pointer_forced_kernel(ForcedArgs a) {
  const PointerArgs& pa = a.p;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= pa.B) return;   // (wave-uniform; nothing below synchronises across waves)
  const int S = pa.S;
  float m, b2, lsum;
  int i1;
  ff_pointer_mask_reduce<true>(pa, b, lane, &m, &b2, &i1, &lsum);
  const int g = min(max(ff_ld4i(a.forced + b), 0), S - 1);
  const float* lrow = pa.logits + (size_t)b * pa.ldlogits;
  // the masked l[g] was stored by lane g % 64 a moment ago: that lane reads its own store back and broadcasts it
  const int owner = g & 63;
  const float mine = lane == owner ? ff_ld4(lrow + g) : 0.f;
  const float lg = __shfl(mine, owner, FF_WAVE);
  int above = 0;
  for (int s = lane; s < S; s += 64) {   // (every lane re-reads the keys it masked itself)
    const float v = ff_ld4(lrow + s);
    above += (v > lg || (v == lg && s < g)) ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) above += __shfl_xor(above, off, FF_WAVE);
  if (lane == 0) {
    // saturates: a masked forced key of a row with live keys gives -FLT_MAX (no -inf, no NaN: lsum >= 1, every term finite)
    ff_st4(a.logprob + b, fmaxf((lg - m) - logf(lsum), -FLT_MAX));
    ff_st4i(a.greedy + b, i1);
    ff_st4i(a.rank + b, above);
  }
  if (pa.next_rows) ff_pointer_append_row(pa, b / pa.spg, b, g, lane);
}

__global__ void forced_tokens_kernel(const int64_t* __restrict__ paths, int* __restrict__ tok, int rows, int T, int S) {
  const size_t total = (size_t)rows * T;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % T);
    const size_t r = i / T;
    const int64_t v = paths[i];
    tok[(size_t)j * rows + r] = (int)(v < 0 ? 0 : (v >= S ? S - 1 : v));
  }
}

// Row r: column 0 is special (logprob 0, greedy = the start token, rank 0), column 1 <= j <= len[r] holds step j - 1's record,
// everything behind is 0.  seq_logprob[r] = the sum of the row's scored log-probabilities, saturated at -FLT_MAX.
__global__ void forced_finalize_kernel(const int* __restrict__ tok, const float* __restrict__ lp_all, const int* __restrict__ greedy_all,
                                       const int* __restrict__ rank_all, const int* __restrict__ lengths, int rows, int T,
                                       float* __restrict__ logprob, int64_t* __restrict__ greedy, int* __restrict__ rank,
                                       float* __restrict__ seq_logprob) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int len = min(max(lengths[r], 0), T - 1);
  float* lp = logprob + (size_t)r * T;
  int64_t* gr = greedy + (size_t)r * T;
  int* rk = rank + (size_t)r * T;
  lp[0] = 0.f; gr[0] = (int64_t)tok[r]; rk[0] = 0;
  double sum = 0.0;
  for (int j = 1; j < T; ++j) {
    const bool in = j <= len;
    const size_t k = (size_t)(j - 1) * rows + r;
    const float v = in ? lp_all[k] : 0.f;
    sum += (double)v;
    lp[j] = v;
    gr[j] = in ? (int64_t)greedy_all[k] : (int64_t)0;
    rk[j] = in ? rank_all[k] : 0;
  }
  seq_logprob[r] = (float)fmax(sum, -(double)FLT_MAX);
}

}  // namespace

int ff_pointer_forced_sync(const ff_step_io& io, const int* forced, float* logprob, int* greedy, int* rank, ff_stream_t stream) {
  const int B = io.rows, S = io.S;
  if (B == 0) return FF_OK;
  FF_CHECK_ARG(B > 0 && S > 0 && io.rows_per_wireframe > 0, "ff_pointer_forced: bad sizes B=%d S=%d", B, S);
  ForcedArgs a;
  memset(&a, 0, sizeof(a));
  FF_RETURN_IF(ff_step_args(&a.p, "ff_pointer_forced", true, io));
  FF_CHECK_ARG(forced && logprob && greedy && rank, "ff_pointer_forced: null pointer");
  a.forced = forced; a.logprob = logprob; a.greedy = greedy; a.rank = rank;
  hipStream_t st = (hipStream_t)stream;
  FFProfScope prof(FF_CAT_POINTER, (double)B * S * 12.0, st);
  hipLaunchKernelGGL(pointer_forced_kernel, dim3(ff_cdiv(B, 4)), dim3(256), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

// (no terminator range, no counter: a forced step finishes nothing and counts nothing)
extern "C" int ff_pointer_forced(float* logits, int ldlogits, int S, const unsigned char* mask, const int* kv_len, int B,
                                 int seqs_per_group, const int* forced, float* logprob, int* greedy, int* rank,
                                 const float* memory, int E, float* next_rows, int ldnext, float* next_stats, ff_stream_t stream) {
  return ff_pointer_forced_sync(ff_step_io{logits, ldlogits, S, mask, kv_len, B, seqs_per_group, 0, 0, 0, memory, E, next_rows, ldnext,
                                           next_stats, nullptr, nullptr, nullptr},
                                forced, logprob, greedy, rank, stream);
}

int ff_forced_tokens(const int64_t* paths, int* tok, int rows, int T, int S, hipStream_t st) {
  const size_t total = (size_t)rows * T;
  const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(forced_tokens_kernel, dim3(grid), dim3(256), 0, st, paths, tok, rows, T, S);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

int ff_forced_finalize(const int* tok, const float* lp_all, const int* greedy_all, const int* rank_all, const int* lengths, int rows,
                       int T, float* logprob, int64_t* greedy, int* rank, float* seq_logprob, hipStream_t st) {
  hipLaunchKernelGGL(forced_finalize_kernel, dim3(ff_cdiv(rows, 256)), dim3(256), 0, st, tok, lp_all, greedy_all, rank_all, lengths,
                     rows, T, logprob, greedy, rank, seq_logprob);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
