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

// ---- the draw of a sampled step (include/faceformer_hip.h states the rule) --------------------------------------------
// One copy for pointer_sample_kernel (ff_sample.hip) and pointer_constrained_sample_kernel (ff_constrain_sample.hip): what lies
// between the masked reduction of a row and the store of its log-probability.
// fp32 -> unsigned, order preserving (-0 counts as +0); and back
__device__ __forceinline__ unsigned sample_key(float v) {
  const unsigned b = __float_as_uint(v + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// inclusive scan of one value per lane, lanes in ascending order (Hillis-Steele: six rounds)
__device__ __forceinline__ float sample_wave_scan(float c, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float o = __shfl_up(c, off, FF_WAVE);
    if (lane >= off) c += o;
  }
  return c;
}

// The token of launch row b from its masked and reduced logit row lrow[0..S) (maximum m, argmax i1; masked keys hold -FLT_MAX):
// no live key -> 0, temperature 0 -> i1, else the top-k bisection, the top-p bisection and the two scans of the header's rule,
// with the row's uniform uniforms[row_id[b]] (row_id null: b) clamped into [0, 1 - 2^-24].  Wave-uniform.  The row is re-read
// from memory in every round with lane = key mod 64: a lane reads only the keys it masked itself.  Selects into a local and
// returns it (the note above ff_beam_walk: no conditional stores through references).
__device__ __forceinline__ int ff_sample_draw(const float* lrow, int S, int lane, float m, int i1, float tau, int top_k, float top_p,
                                              const float* uniforms, const int* row_id, int num_uniforms, int b) {
  const float FILL = -FLT_MAX;
  const int nchunk = (S + 63) >> 6;
  int tok = 0;
  if (m == FILL) tok = 0;            // no live key (masked keys hold -FLT_MAX)
  else if (tau == 0.f) tok = i1;     // greedy's rule
  else {
    int nlive = 0;
    for (int c = 0; c < nchunk && top_k > 0; ++c) {
      const int s = c * 64 + lane;
      nlive += __popcll(__ballot(s < S && ff_ld4(lrow + s) > FILL));
    }
    // top-k: the largest key image with at least K keys at or above it is the image of the K-th largest logit
    float thr = FILL;
    if (top_k > 0 && top_k < nlive) {
      unsigned th = 0;
      for (unsigned bit = 0x80000000u; bit; bit >>= 1) {
        const unsigned cand = th | bit;
        int cnt = 0;
        for (int c = 0; c < nchunk; ++c) {
          const int s = c * 64 + lane;
          cnt += __popcll(__ballot(s < S && sample_key(ff_ld4(lrow + s)) >= cand));
        }
        if (cnt >= top_k) th = cand;
      }
      thr = sample_unkey(th);
    }
    // top-p over the keys top-k kept
    if (top_p < 1.f) {
      const float vk = thr;
      float target = 0.f;
      unsigned th = 0;
      for (int round = -1; round < 32; ++round) {   // round -1: the mass of everything top-k kept
        const unsigned cand = round < 0 ? 0u : (th | (0x80000000u >> round));
        float mass = 0.f;
        for (int s = lane; s < S; s += 64) {
          const float v = ff_ld4(lrow + s);
          const bool in = v > FILL && v >= vk && sample_key(v) >= cand;
          mass += in ? __expf((v - m) / tau) : 0.f;
        }
        mass = ff_wave_sum(mass);
        if (round < 0) target = top_p * mass;
        else if (mass >= target) th = cand;
      }
      thr = sample_unkey(th);
    }
    // draw
    int rid = row_id ? ff_ld4i(row_id + b) : b;
    rid = min(max(rid, 0), num_uniforms - 1);
    const float u = fminf(fmaxf(ff_ld4(uniforms + rid), 0.f), 0.99999994f);   // 1 - 2^-24
    float Z = 0.f;
    for (int c = 0; c < nchunk; ++c) {
      const int s = c * 64 + lane;
      const float v = s < S ? ff_ld4(lrow + s) : FILL;
      const float w = (v > FILL && v >= thr) ? __expf((v - m) / tau) : 0.f;
      Z = Z + __shfl(sample_wave_scan(w, lane), 63, FF_WAVE);
    }
    const float uz = u * Z;
    float carry = 0.f;
    int last = 0;
    bool found = false;
    for (int c = 0; c < nchunk && !found; ++c) {
      const int s = c * 64 + lane;
      const float v = s < S ? ff_ld4(lrow + s) : FILL;
      const bool kept = v > FILL && v >= thr;
      const float local = sample_wave_scan(kept ? __expf((v - m) / tau) : 0.f, lane);
      const unsigned long long kb = __ballot(kept);
      const unsigned long long hb = __ballot(kept && carry + local > uz);
      if (kb) last = c * 64 + 63 - __clzll(kb);
      if (hb) { tok = c * 64 + __ffsll((long long)hb) - 1; found = true; }
      carry = carry + __shfl(local, 63, FF_WAVE);
    }
    if (!found) tok = last;
  }
  return tok;
}

// ---- face-loop rule (include/faceformer_hip.h states it on tokens) ---------------------------------------------------
// What the rule reads of one launch besides PointerArgs; the kernels fill it from their own arguments.
struct FFLoopRule {
  const unsigned* follows;           // [wireframes, L, fw] bits or null: bit b of row a = edge b starts where edge a ends
  int L, fw, flags, ntok;
  const unsigned char* close_dist;   // look-ahead only: [wireframes, L, L] bytes, close_dist[w][f][b] = D(b -> f)
  const unsigned char* cycle_len;    // look-ahead, exact: [wireframes, L] bytes, D(b -> b)
  int budget;                        // look-ahead, exact
};

// first / prev as stored -> an edge of the wireframe or "none" (the entries cannot see device data: anything else is "none")
__device__ __forceinline__ int ff_loop_edge(int e, int L) { return (e < 0 || e >= L) ? -1 : e; }

// ---- exact closure look-ahead (include/faceformer_hip.h states the rule) ----------------------------------------------
enum { FF_LOOP_PLAIN = 0, FF_LOOP_AHEAD = 1, FF_LOOP_EXACT = 2 };   // the compile-time forms of ff_loop_write_row

// Which edges b reach the open loop's first edge within r.budget hops through unused edges: D_V(b -> first) <= budget, where a
// path's inner nodes are `avail` (an edge key that is not padded and not visited) and b itself is any edge.  One backward
// breadth-first search from `first` per sequence, pull-style over the FORWARD table: level 1 = {x: follows[x][first]}, level
// h + 1 = {x not reached: follows[x] meets the avail nodes of level h}.  Lane (ntok + x) mod 64 owns node x, as in the byte-row
// loop, so the bit this returns (bit c: key c * 64 + lane reached) is in the lane that writes the byte.  A level's frontier is
// the ballots of its new avail nodes, re-cut into the table's words: lane j keeps word j (edges 32j .. 32j + 31) and every
// lane reads it with a wave-uniform readlane; words of an empty frontier part are skipped.  No LDS, no barrier.
// Ends at the first of: an empty frontier, `budget` levels, every unvisited candidate of follows[prev] reached -- the padded
// candidates included: their byte is the rule's as well (D_V is defined for any b), so one that cannot be reached keeps the
// search going to the budget or to an empty frontier; that costs time only.
// Needs S <= FF_EXACT_MAX_S (ff_common.h: bit c of a lane's words is its key c * 64 + lane, c < 32; so fw <= 64), first and prev edges of the wireframe, CONNECT and NO_REPEAT (the entries check).
__device__ __forceinline__ unsigned ff_loop_closure_reach(const PointerArgs& pa, const FFLoopRule& r, int lane, int w, int kv,
                                                          const unsigned char* mrow, int first, int prev, const unsigned* vrow) {
  const int S = pa.S, ntok = r.ntok, fw = r.fw;
  if (r.budget < 1) return 0u;
  const unsigned* rows = r.follows + (size_t)w * r.L * fw;
  const unsigned* prow = rows + (size_t)prev * fw;
  unsigned avail = 0u, want = 0u, reach = 0u;
  for (int s = lane; s < S; s += 64) {   // level 1, and what the levels need of every key
    if (s < ntok) continue;
    const int e = s - ntok;
    const unsigned bit = 1u << (e & 31), cbit = 1u << (s >> 6);
    const bool vis = (vrow[e >> 5] & bit) != 0u;
    bool pad = s >= kv;
    if (!pad && mrow) pad = ff_ldw(mrow + s) != 0;
    if (!vis && !pad) avail |= cbit;
    if (!vis && (prow[e >> 5] & bit) != 0u) want |= cbit;
    if ((rows[(size_t)e * fw + (first >> 5)] >> (first & 31)) & 1u) reach |= cbit;
  }
  unsigned fresh = reach & avail;   // the nodes of the last level that a path may pass through
  const int nch = (S + 63) >> 6, a0 = lane * 32 + ntok;   // a0: the key of bit 0 of this lane's frontier word
  for (int h = 1; h < r.budget && __ballot((want & ~reach) != 0u) != 0ull; ++h) {
    unsigned front = 0u;
    bool any = false;
    for (int c = 0; c < nch; ++c) {
      const unsigned long long bal = __ballot(((fresh >> c) & 1u) != 0u);
      if (bal == 0ull) continue;   // (wave-uniform)
      any = true;
      const int d = a0 - c * 64;   // bit i of the word is bit d + i of this chunk's ballot
      if (d >= 0 && d < 64) front |= (unsigned)(bal >> d);
      if (d < 0 && d > -32) front |= (unsigned)bal << -d;
    }
    if (!any) break;
    fresh = 0u;
    for (int c = 0; c < nch; ++c) {
      const int s = c * 64 + lane;
      const bool todo = s >= ntok && s < S && ((reach >> c) & 1u) == 0u;
      if (__ballot(todo) == 0ull) continue;   // (wave-uniform)
      const unsigned* xr = rows + (size_t)(todo ? s - ntok : 0) * fw;
      unsigned hit = 0u;
      for (int j = 0; j < fw; ++j) {
        const unsigned fj = (unsigned)__builtin_amdgcn_readlane((int)front, j);
        if (fj == 0u) continue;   // (wave-uniform)
        if (todo) hit |= xr[j] & fj;
      }
      if (hit != 0u) { reach |= 1u << c; fresh |= avail & (1u << c); }
    }
  }
  return reach;
}

// The byte row xrow[0..S) of one sequence's constraint mask (1 = masked) from its (first, prev) and visited words vrow, for
// wireframe w with kv keys and padding-mask row mrow: one vote on "any live edge" (it sees padding, kv and visited), and on a
// dead end of an open loop the terminators re-opened; returns the dead-end bit (wave-uniform).  Every loop keeps lane = key
// mod 64: ff_pointer_mask_reduce reads back only bytes its own lane wrote, so there is no barrier.
// FORM (a compile-time form of the one rule): FF_LOOP_PLAIN; FF_LOOP_AHEAD, the closure look-ahead -- the
// distance of every edge to the loop's first edge while it is open, else the edge's own shortest cycle, against the budget;
// FF_LOOP_EXACT, the exact closure look-ahead -- with the loop open the search above in place of the distance
// row, with it closed the look-ahead's cycle_len.  What a form does not use is compiled out: <false> and <true> are PLAIN and AHEAD.
template <int FORM>
__device__ __forceinline__ bool ff_loop_write_row(const PointerArgs& pa, const FFLoopRule& r, int lane, int w, int kv,
                                                  const unsigned char* mrow, int first, int prev, const unsigned* vrow,
                                                  unsigned char* xrow) {
  const int S = pa.S, ntok = r.ntok;
  const bool connect = (r.flags & FF_CONSTRAIN_CONNECT) != 0, norep = (r.flags & FF_CONSTRAIN_NO_REPEAT) != 0;
  const bool open = connect && first >= 0 && prev >= 0;
  const unsigned* frow = open ? r.follows + ((size_t)w * r.L + prev) * r.fw : nullptr;
  const unsigned char* drow = nullptr;
  if (FORM == FF_LOOP_AHEAD && connect) drow = open ? r.close_dist + ((size_t)w * r.L + first) * r.L : r.cycle_len + (size_t)w * r.L;
  if (FORM == FF_LOOP_EXACT && connect && !open) drow = r.cycle_len + (size_t)w * r.L;
  unsigned reach = 0u;
  if (FORM == FF_LOOP_EXACT && open) reach = ff_loop_closure_reach(pa, r, lane, w, kv, mrow, first, prev, vrow);
  bool live_edge = false;
  for (int s = lane; s < S; s += 64) {
    bool masked;
    if (s < ntok) {
      masked = connect && (open || s < pa.term_lo || s >= pa.term_hi);
    } else {
      const int e = s - ntok;
      const unsigned bit = 1u << (e & 31);
      masked = (norep && (vrow[e >> 5] & bit) != 0) || (open && (frow[e >> 5] & bit) == 0);
      if (FORM != FF_LOOP_PLAIN && drow) masked = masked || (int)drow[e] > r.budget;
      if (FORM == FF_LOOP_EXACT && open) masked = masked || ((reach >> (s >> 6)) & 1u) == 0u;
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

// The single-sequence model's byte row as one call, for the beam form: the plain rule with the
// terminator range pa.term_lo / pa.term_hi = [SEP, SEP + 1) -- open: every special token masked, SEP re-opened on a dead end;
// closed: every special token but SEP masked -- and then the two fix-ups of the closed state by the lanes that own the keys
// (lane = key mod 64): EOS is opened, SEP is masked while the current face has no edge (prev == none).  Returns the dead-end bit.
// pointer_sequence_constrained_kernel (ff_constrain_seq.hip) has the same lines in its own body and keeps them there: moving
// them behind this call changed that kernel's register allocation.
// FORM: ff_loop_write_row's compile-time form; the closure forms read r.close_dist / r.cycle_len / r.budget in front
// of the dead-end vote, the two fix-ups stay what they are.
template <int FORM = FF_LOOP_PLAIN>
__device__ __forceinline__ bool ff_sequence_write_row(const PointerArgs& pa, const FFLoopRule& r, int lane, int w, int kv,
                                                      const unsigned char* mrow, int first, int prev, const unsigned* vrow,
                                                      unsigned char* xrow, int sep, int eos) {
  const bool dead = ff_loop_write_row<FORM>(pa, r, lane, w, kv, mrow, first, prev, vrow, xrow);
  if ((r.flags & FF_CONSTRAIN_CONNECT) && !(first >= 0 && prev >= 0)) {   // closed: EOS may end the row; no empty face
    if (lane == (eos & 63)) xrow[eos] = 0;
    if (prev < 0 && lane == (sep & 63)) xrow[sep] = 1;
  }
  return dead;
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
