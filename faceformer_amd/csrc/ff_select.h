// Device pieces the selection kernels share (ff_beam.hip, ff_constrain.hip, ff_constrain_beam.hip): the sorted candidate list of
// a beam step and the face-loop rule of a constrained step.  One copy of each, so the constrained beam writes its byte rows as
// the constrained greedy launch does because both call the same function.
#pragma once
#include <float.h>

#include "ff_common.h"
#include "ff_device.h"

// ---- beam candidate list ---------------------------------------------------------------------------------------------------------
// W (score, flat index k * S + s) entries per lane, sorted: higher score first, equal scores by the lower index -- a total
// order, so both lanes of a merged pair compute the same list and the result is the same on every run.
// The helpers with a loop around ff_beam_insert work on a copy of the list and store it back at the end, and ff_beam_rank
// selects into locals: the compiler optimises a helper on its own before it inlines it, and conditional stores through the
// references stay branches there (the kernels lose their v_cndmask chains: twice the code).  On copies the kernels come out as
// they did with the loops written in them (profiles/select_shared/device_code.txt).
constexpr int FF_BEAM_MAX_W = 8;
constexpr int FF_BEAM_NONE = 0x7fffffff;   // flat index of a list entry that holds no candidate (score -inf)

template <int W>
__device__ __forceinline__ void ff_beam_list_init(float (&lsc)[W], int (&lix)[W]) {
#pragma unroll
  for (int i = 0; i < W; ++i) { lsc[i] = -INFINITY; lix[i] = FF_BEAM_NONE; }
}

// candidate (sc, ix) into the sorted list when it ranks before an entry
template <int W>
__device__ __forceinline__ void ff_beam_insert(float (&lsc)[W], int (&lix)[W], float sc, int ix) {
#pragma unroll
  for (int i = W - 1; i >= 0; --i) {
    const bool before = sc > lsc[i] || (sc == lsc[i] && ix < lix[i]);
    if (before) {
      if (i < W - 1) { lsc[i + 1] = lsc[i]; lix[i + 1] = lix[i]; }
      lsc[i] = sc; lix[i] = ix;
    }
  }
}

// The candidates of beam k (score c) from its masked and reduced logit row (maximum m, logz = log sum exp(l - m)): every lane
// walks its strided keys.  LIVE: a masked key (l[s] = -FLT_MAX) is never a candidate.
template <int W, bool LIVE>
__device__ __forceinline__ void ff_beam_walk(float (&lsc)[W], int (&lix)[W], const float* lrow, int S, int lane, int k, float c,
                                             float m, float logz) {
  const float FILL = -FLT_MAX;
  float a[W];
  int b[W];
#pragma unroll
  for (int i = 0; i < W; ++i) { a[i] = lsc[i]; b[i] = lix[i]; }
  for (int s = lane; s < S; s += 64) {
    const float v = ff_ld4(lrow + s);
    if (!LIVE || v > FILL) ff_beam_insert<W>(a, b, fmaxf(c + ((v - m) - logz), FILL), k * S + s);   // saturates: no -inf, no NaN
  }
#pragma unroll
  for (int i = 0; i < W; ++i) { lsc[i] = a[i]; lix[i] = b[i]; }
}

// six butterfly rounds merge the lanes' lists in a fixed tree: every lane ends with the wave's W best
template <int W>
__device__ __forceinline__ void ff_beam_merge(float (&lsc)[W], int (&lix)[W]) {
  float a[W];
  int b[W];
#pragma unroll
  for (int i = 0; i < W; ++i) { a[i] = lsc[i]; b[i] = lix[i]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float osc[W];
    int oix[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { osc[i] = __shfl_xor(a[i], off, FF_WAVE); oix[i] = __shfl_xor(b[i], off, FF_WAVE); }
#pragma unroll
    for (int i = 0; i < W; ++i) ff_beam_insert<W>(a, b, osc[i], oix[i]);
  }
#pragma unroll
  for (int i = 0; i < W; ++i) { lsc[i] = a[i]; lix[i] = b[i]; }
}

// lane k takes rank k (the lanes from W on: no candidate)
template <int W>
__device__ __forceinline__ void ff_beam_rank(const float (&lsc)[W], const int (&lix)[W], int lane, float* sc, int* ix) {
  float s = -INFINITY;
  int x = FF_BEAM_NONE;
#pragma unroll
  for (int i = 0; i < W; ++i)
    if (lane == i) { s = lsc[i]; x = lix[i]; }
  *sc = s;
  *ix = x;
}

// ---- face-loop rule (include/faceformer_hip.h states it on tokens) ---------------------------------------------------
// What the rule reads of one launch besides PointerArgs; the kernels fill it from their own arguments.
struct FFLoopRule {
  const unsigned* follows;           // [wireframes, L, fw] bits or null: bit b of row a = edge b starts where edge a ends
  int L, fw, flags, ntok;
  const unsigned char* close_dist;   // look-ahead only: [wireframes, L, L] bytes, close_dist[w][f][b] = D(b -> f)
  const unsigned char* cycle_len;    // look-ahead only: [wireframes, L] bytes, D(b -> b)
  int budget;                        // look-ahead only
};

// first / prev as stored -> an edge of the wireframe or "none" (the entries cannot see device data: anything else is "none")
__device__ __forceinline__ int ff_loop_edge(int e, int L) { return (e < 0 || e >= L) ? -1 : e; }

// The byte row xrow[0..S) of one sequence's constraint mask (1 = masked) from its (first, prev) and visited words vrow, for
// wireframe w with kv keys and padding-mask row mrow: one vote on "any live edge" (it sees padding, kv and visited), and on a
// dead end of an open loop the terminators re-opened; returns the dead-end bit (wave-uniform).  Every loop keeps lane = key
// mod 64: ff_pointer_mask_reduce reads back only bytes its own lane wrote, so there is no barrier.
// AHEAD: the closure look-ahead -- the distance of every edge to the loop's first edge while it is open, else
// the edge's own shortest cycle, against the budget; compiled out for <false>.
template <bool AHEAD>
__device__ __forceinline__ bool ff_loop_write_row(const PointerArgs& pa, const FFLoopRule& r, int lane, int w, int kv,
                                                  const unsigned char* mrow, int first, int prev, const unsigned* vrow,
                                                  unsigned char* xrow) {
  const int S = pa.S, ntok = r.ntok;
  const bool connect = (r.flags & FF_CONSTRAIN_CONNECT) != 0, norep = (r.flags & FF_CONSTRAIN_NO_REPEAT) != 0;
  const bool open = connect && first >= 0 && prev >= 0;
  const unsigned* frow = open ? r.follows + ((size_t)w * r.L + prev) * r.fw : nullptr;
  const unsigned char* drow = nullptr;
  if (AHEAD && connect) drow = open ? r.close_dist + ((size_t)w * r.L + first) * r.L : r.cycle_len + (size_t)w * r.L;
  bool live_edge = false;
  for (int s = lane; s < S; s += 64) {
    bool masked;
    if (s < ntok) {
      masked = connect && (open || s < pa.term_lo || s >= pa.term_hi);
    } else {
      const int e = s - ntok;
      const unsigned bit = 1u << (e & 31);
      masked = (norep && (vrow[e >> 5] & bit) != 0) || (open && (frow[e >> 5] & bit) == 0);
      if (AHEAD && drow) masked = masked || (int)drow[e] > r.budget;
      bool pad = s >= kv;
      if (!pad && mrow) pad = ff_ldw(mrow + s) != 0;
      live_edge = live_edge || (!masked && !pad);
    }
    xrow[s] = masked ? 1 : 0;
  }
  if (!(open && __ballot(live_edge) == 0ull)) return false;
  for (int s = lane; s < pa.term_hi; s += 64)   // dead end: the terminators instead (every lane rewrites its own keys)
    if (s >= pa.term_lo) xrow[s] = 0;
  return true;
}

// (first, prev) after edge e of wireframe w was selected: e opens a loop when none is open, becomes prev, and closes the loop
// when the first edge starts where e ends -- one word of the follow table (a one-edge loop closes on itself).
__device__ __forceinline__ void ff_loop_advance(const unsigned* follows, int w, int L, int fw, int e, int* first, int* prev) {
  if (*first < 0) *first = e;
  *prev = e;
  if (follows) {
    const unsigned word = follows[((size_t)w * L + e) * fw + (*first >> 5)];
    if ((word >> (*first & 31)) & 1u) *first = -1;
  }
}

// The rule's state after column 0 (start token t of a sequence of wireframe w): a token below ntok leaves it empty; an edge is
// visited, is prev and opens a loop unless it closes on itself.
__device__ __forceinline__ void ff_loop_start(int t, int ntok, const unsigned* follows, int w, int L, int fw, unsigned* visited,
                                              int* first, int* prev) {
  for (int k = 0; k < fw; ++k) visited[k] = 0u;
  *first = *prev = -1;
  const int e = t - ntok;
  if (e >= 0 && e < L) {
    visited[e >> 5] = 1u << (e & 31);
    ff_loop_advance(follows, w, L, fw, e, first, prev);
  }
}
