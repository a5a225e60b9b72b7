// Self-attention of the pruned last decoder layer with k | v folded into the query.
//
// The pruned last layer attends from the newest position only, yet its k | v projection ran over every prefix row of every
// step.  With x^_j = (x_j - mean_j) rstd_j and the LayerNorm-folded weights W', b', P the engine binds (ln1_w, ln1_b, ln1_pos):
//   q_h . k_{j,h} = (q_h W'k_h) . x^_j + q_h . (b'k_h + P[j, E + 64h ...])  =  qt_h . x^_j + c_{h,j}
//   o_h = sum_j p_j v_{j,h} = (sum_j p_j x^_j) W'v_h^T + b'v_h              =  u_h W'v_h^T + b'v_h       (sum_j p_j = 1)
// so the projection moves to the Bc query rows: two small head-batched products around ONE pass over the prefix rows, which is
// this file.  The pass is bandwidth bound (t = 36, E = 512, 256 sequences: 18.9 MB read, 0.15 GFLOP): plain HIP C++ on the VALU,
// no matrix cores, no LDS-DMA, no atomics.  Summation order is fixed -- the lanes of a wave own fixed columns and meet in the
// butterfly of ff_wave_sum, positions are added in ascending order -- so the result depends on the operands alone.
#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"

namespace {

constexpr int FOLD_THREADS = 512;
constexpr int FOLD_WAVES = FOLD_THREADS / FF_WAVE;
constexpr int FOLD_MAX_H = 8;    // E <= 512: at most eight heads of 64 columns
constexpr int FOLD_MAX_V = 2;    // ... and at most two 16-byte columns of a row per lane
constexpr int FOLD_PB = 4;       // positions a wave has in flight in the score pass (their loads are issued together)
constexpr int FOLD_HPG = 2;      // heads one thread accumulates in the u pass (E <= 512: ceil(H / (512 / (E / 4))) <= 2)
constexpr int FOLD_MAX_SMALL_FLOATS = 12000;   // (2 + H) t + H + 3 floats of statistics and scores: 48 KB
constexpr int FOLD_MAX_LDS_BYTES = 150 * 1024; // with the normalised rows staged beside them (a CU has 160 KB)

struct FoldArgs {
  const float* x;       // [t * Bc, E] running rows, row j * Bc + b
  const float* stats;   // [t * Bc, E / 32, 2] (mean, M2) per 32-column segment of those rows
  const float* qt;      // [Bc, H, E + t]: qt | c
  float* u;             // [Bc, H * E]
  float eps, scale;
  int Bc, t, E, H;
  int stage;            // 1: the normalised rows are kept in LDS for the u pass (they fit); 0: the u pass re-reads x (from L2)
};

// One block per sequence.  Pass 1: positions dealt to the waves (wave w takes j = w, w + 8, ...; the loads of FOLD_PB of them
// are issued before the first is used), the lanes of a wave hold 16-byte columns lane and lane + 64 of the row; the row's
// statistics are merged by every aligned group of eight lanes (ff_ln_merge8: the routine of the small-M projection tile),
// x^ = (x - mean) * rstd, and the H scores of the position are H butterfly sums.  Pass 2: wave w normalises heads w, w + 8, ...
// (max-subtracted; the weights stay unnormalised, 1 / sum is applied to u).  Pass 3: thread (column c4, head group g) adds
// column c4 of every x^ row in ascending position order -- from LDS where pass 1 left it (72 KB at t = 36, E = 512), or re-formed
// from x when the rows do not fit -- into up to FOLD_HPG heads.
__global__ __launch_bounds__(FOLD_THREADS) void attention_prefix_fold_kernel(FoldArgs a) {
  extern __shared__ float fold_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int E = a.E, H = a.H, t = a.t, Bc = a.Bc, nv = E >> 2, nseg = E >> 5, W = E + t;
  const size_t b = blockIdx.x;
  float* mr = fold_lds;              // [t][2] (mean, rstd)
  float* sc = fold_lds + 2 * t;      // [H][t] scores, then exp(score - max)
  float* inv = sc + H * t;           // [H] 1 / sum
  float* xs = fold_lds + (((2 + H) * t + H + 3) & ~3);   // [t][E] x^ (stage)
  const float* qrow = a.qt + b * (size_t)H * W;

  // qt of this lane's columns for every head (rows of qt start at any 4-byte offset: t may be odd)
  float qv[FOLD_MAX_H][FOLD_MAX_V][4];
#pragma unroll
  for (int h = 0; h < FOLD_MAX_H; ++h)
#pragma unroll
    for (int v = 0; v < FOLD_MAX_V; ++v) {
      const int c4 = lane + 64 * v;
      const bool ok = h < H && c4 < nv;
#pragma unroll
      for (int i = 0; i < 4; ++i) qv[h][v][i] = ok ? ff_ldw(qrow + (size_t)h * W + c4 * 4 + i) : 0.f;
    }

  const int spart = lane & 7;
  const bool sok = 2 * spart < nseg;
  for (int j0 = wave; j0 < t; j0 += FOLD_WAVES * FOLD_PB) {
    f32x4 sv[FOLD_PB], xv[FOLD_PB][FOLD_MAX_V];
#pragma unroll
    for (int p = 0; p < FOLD_PB; ++p) {
      const int j = j0 + FOLD_WAVES * p;
      sv[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < FOLD_MAX_V; ++v) xv[p][v] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j < t) {   // (wave-uniform)
        const size_t row = (size_t)j * Bc + b;
        if (sok) sv[p] = ff_ld16(a.stats + (row * nseg + 2 * spart) * 2);
#pragma unroll
        for (int v = 0; v < FOLD_MAX_V; ++v)
          if (lane + 64 * v < nv) xv[p][v] = ff_ld16(a.x + row * E + (lane + 64 * v) * 4);
      }
    }
#pragma unroll
    for (int p = 0; p < FOLD_PB; ++p) {
      const int j = j0 + FOLD_WAVES * p;
      if (j < t) {   // (wave-uniform)
        const f32x2 mv = ff_ln_merge8(sv[p], spart, nseg);
        const float mean = mv.x, rstd = 1.0f / sqrtf(mv.y + a.eps);
#pragma unroll
        for (int v = 0; v < FOLD_MAX_V; ++v) {
          const int c4 = lane + 64 * v;
          xv[p][v] = c4 < nv ? (xv[p][v] - mean) * rstd : f32x4{0.f, 0.f, 0.f, 0.f};
          if (a.stage && c4 < nv) ff_st16(xs + (size_t)j * E + c4 * 4, xv[p][v]);
        }
        if (lane == 0) { mr[2 * j] = mean; mr[2 * j + 1] = rstd; }
#pragma unroll
        for (int h = 0; h < FOLD_MAX_H; ++h) {
          if (h < H) {   // (block-uniform)
            float s = 0.f;
#pragma unroll
            for (int v = 0; v < FOLD_MAX_V; ++v)
#pragma unroll
              for (int i = 0; i < 4; ++i) s += qv[h][v][i] * xv[p][v][i];
            s = ff_wave_sum(s);
            if (lane == 0) sc[h * t + j] = a.scale * (s + ff_ldw(qrow + (size_t)h * W + E + j));
          }
        }
      }
    }
  }
  __syncthreads();

  for (int h = wave; h < H; h += FOLD_WAVES) {
    float* s = sc + h * t;
    float mx = -3.402823466e38f;
    for (int j = lane; j < t; j += FF_WAVE) mx = fmaxf(mx, s[j]);
    mx = ff_wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < t; j += FF_WAVE) {
      const float e = expf(s[j] - mx);
      s[j] = e;
      sum += e;
    }
    sum = ff_wave_sum(sum);
    if (lane == 0) inv[h] = 1.0f / sum;
  }
  __syncthreads();

  const int groups = FOLD_THREADS / nv;          // thread groups of nv threads: one 16-byte column each
  const int hpg = (H + groups - 1) / groups;     // heads per group (<= FOLD_HPG)
  const int g = tid / nv, c4 = tid - g * nv, h0 = g * hpg;
  if (g >= groups || h0 >= H) return;
  f32x4 acc[FOLD_HPG];
#pragma unroll
  for (int k = 0; k < FOLD_HPG; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.stage) {
    const float* xc = xs + c4 * 4;
#pragma unroll 4
    for (int j = 0; j < t; ++j) {
      const f32x4 xh = ff_ld16(xc + (size_t)j * E);
#pragma unroll
      for (int k = 0; k < FOLD_HPG; ++k)
        if (k < hpg && h0 + k < H) acc[k] += sc[(h0 + k) * t + j] * xh;
    }
  } else {
    const float* xc = a.x + b * E + c4 * 4;
#pragma unroll 8
    for (int j = 0; j < t; ++j) {
      const f32x4 xh = (ff_ld16(xc + (size_t)j * Bc * E) - mr[2 * j]) * mr[2 * j + 1];
#pragma unroll
      for (int k = 0; k < FOLD_HPG; ++k)
        if (k < hpg && h0 + k < H) acc[k] += sc[(h0 + k) * t + j] * xh;
    }
  }
#pragma unroll
  for (int k = 0; k < FOLD_HPG; ++k)
    if (k < hpg && h0 + k < H) ff_st16(a.u + (b * H + (h0 + k)) * (size_t)E + c4 * 4, acc[k] * inv[h0 + k]);
}

// The per-call tables of the folded form (weights only): kt[h][n][k], the head-batched W operand ([N, K] layout, K = 64) of
// the qt | c product -- rows n < E the transposed k rows of the folded weight, row E + j the folded k bias plus position j's
// table row -- and ob[n] = out_b[n] + sum_k out_w[n][k] b'v[k], the out-projection's bias with the v bias carried through
// (sum_j p_j = 1: every o row holds b'v once).  The first kt_blocks blocks copy, the others reduce one ob entry per wave.
__global__ __launch_bounds__(256) void attention_fold_tables_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                                                    const float* __restrict__ pos, int pos_rows,
                                                                    const float* __restrict__ out_w, const float* __restrict__ out_b,
                                                                    int E, int H, int T, float* __restrict__ kt,
                                                                    float* __restrict__ ob, int kt_blocks) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < kt_blocks) {
    const size_t i = (size_t)blockIdx.x * 256 + tid, total = (size_t)H * (E + T) * 64;
    if (i >= total) return;
    const int k = (int)(i & 63), n = (int)((i >> 6) % (size_t)(E + T)), h = (int)((i >> 6) / (size_t)(E + T));
    const int c = E + 64 * h + k;
    if (n < E) {
      kt[i] = w[(size_t)c * E + n];
    } else {
      const int j = n - E < pos_rows ? n - E : pos_rows - 1;
      kt[i] = bias[c] + pos[(size_t)j * 2 * E + c];
    }
    return;
  }
  const int n = ((int)blockIdx.x - kt_blocks) * 4 + (tid >> 6), lane = tid & 63;
  if (n >= E) return;
  float s = 0.f;
  for (int k = lane; k < E; k += FF_WAVE) s += out_w[(size_t)n * E + k] * bias[2 * E + k];
  s = ff_wave_sum(s);
  if (lane == 0) ob[n] = out_b[n] + s;
}

}  // namespace

size_t ff_attention_fold_table_floats(int E, int H, int T) { return (size_t)H * (E + T) * 64 + (size_t)E; }

int ff_attention_fold_tables(const float* ln1_w, const float* ln1_b, const float* ln1_pos, int pos_rows, const float* out_w,
                             const float* out_b, int E, int H, int T, float* kt, float* ob, hipStream_t st) {
  FF_CHECK_ARG(ln1_w && ln1_b && ln1_pos && out_w && out_b && kt && ob && pos_rows > 0 && T > 0 && E == H * FF_HEAD_DIM,
               "ff_attention_fold_tables: bad arguments");
  const size_t total = (size_t)H * (E + T) * 64;
  const int kt_blocks = (int)((total + 255) / 256);
  FFProfScope prof(FF_CAT_ROWOP, (double)total * 8.0, st);
  hipLaunchKernelGGL(attention_fold_tables_kernel, dim3(kt_blocks + ff_cdiv(E, 4)), dim3(256), 0, st, ln1_w, ln1_b, ln1_pos,
                     pos_rows, out_w, out_b, E, H, T, kt, ob, kt_blocks);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" int ff_attention_prefix_fold(const float* x, const float* stats, float ln_eps, const float* qt, float scale,
                                        int Bc, int t, int E, int H, float* u, ff_stream_t stream) {
  if (Bc == 0) return FF_OK;
  FF_CHECK_ARG(x && stats && qt && u, "ff_attention_prefix_fold: null operand");
  FF_CHECK_ARG(E % 64 == 0 && E >= 128 && E <= 512 && H == E / FF_HEAD_DIM,
               "ff_attention_prefix_fold: needs E %% 64 == 0, 128 <= E <= 512 and H = E / 64 (E=%d H=%d)", E, H);
  FF_CHECK_ARG(Bc > 0 && t > 0 && ln_eps >= 0.f, "ff_attention_prefix_fold: bad Bc=%d t=%d", Bc, t);
  const long small_floats = (((long)(2 + H) * t + H + 3) & ~3L);
  FF_CHECK_ARG(small_floats <= FOLD_MAX_SMALL_FLOATS, "ff_attention_prefix_fold: t=%d is past the %d score floats a block keeps", t,
               FOLD_MAX_SMALL_FLOATS);
  FF_CHECK_ARG(ff_aligned16(x) && ff_aligned16(stats) && ff_aligned16(u), "ff_attention_prefix_fold: x / stats / u must be 16-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const long staged_bytes = (small_floats + (long)t * E) * (long)sizeof(float);
  const int stage = staged_bytes <= FOLD_MAX_LDS_BYTES ? 1 : 0;
  const size_t lds_bytes = stage ? (size_t)staged_bytes : (size_t)small_floats * sizeof(float);
  static FFLdsLimit attr_set = {};
  FF_RETURN_IF(ff_lds_limit_once(&attention_prefix_fold_kernel, FOLD_MAX_LDS_BYTES, &attr_set));
  FoldArgs a{x, stats, qt, u, ln_eps, scale, Bc, t, E, H, stage};
  // work: the scores and the weighted sums, 2 flops per (position, head, column) each
  FFProfScope prof(FF_CAT_ATTN, 4.0 * Bc * (double)t * H * E, st);
  hipLaunchKernelGGL(attention_prefix_fold_kernel, dim3(Bc), dim3(FOLD_THREADS), lds_bytes, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
