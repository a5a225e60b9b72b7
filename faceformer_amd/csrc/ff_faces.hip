// Device-side face extraction behind the parallel decode: ff_face_rows parses every decoded row into a face,
// walks the enclosure rule on the follow table, puts closed faces into canonical order and writes the edge-set bitmap;
// ff_face_votes groups the rows of a wireframe by that bitmap.  The contract is in include/faceformer_hip.h; the numpy
// restatement, bit for bit, is faces.face_rows / faces.face_votes.
#include "ff_common.h"

namespace {

constexpr int FACE_T = FF_FACE_MAX_T;      // positions of a row: four per lane
constexpr int FACE_K = FACE_T / FF_WAVE;
constexpr int FACE_WAVES = 4;              // rows of a block

__device__ __forceinline__ int face_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// lanes below this one whose bit is set in a ballot
__device__ __forceinline__ int face_prefix(unsigned long long ballot) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}
// LDS written by some lanes of the wave is read by others behind this
__device__ __forceinline__ void face_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int face_first(unsigned long long ballot) { return ballot ? __ffsll((long long)ballot) - 1 : FF_WAVE; }

// s_w of FF_FACE_OWN_STOP: the least j >= 1 at which every row of the wireframe's own anchors (f < num_input[w], every g) holds a
// token below ntok; T - 1 when there is none.  One block per wireframe, thread j reads column j of every row.
__global__ __launch_bounds__(FACE_T) void face_own_stop_kernel(const int64_t* __restrict__ tokens, const int* __restrict__ num_input,
                                                              int F, int G, int T, int ntok, int* __restrict__ stop) {
  __shared__ int s_min;
  const int w = blockIdx.x, j = threadIdx.x;
  if (j == 0) s_min = T - 1;
  __syncthreads();
  int own = num_input[w];
  own = own < 0 ? 0 : (own > F ? F : own);
  const size_t rows = (size_t)own * G;
  if (j >= 1 && j < T) {
    const int64_t* base = tokens + (size_t)w * F * G * T + j;
    bool edge = false;
    for (size_t r = 0; r < rows && !edge; ++r) edge = base[r * T] >= ntok;
    if (!edge) atomicMin(&s_min, j);
  }
  __syncthreads();
  if (j == 0) stop[w] = s_min;
}

struct FaceRowsArgs {
  const int64_t* tokens; const int* num_input; const int* num_edges; const float* scores; const float* logprob; const int* dead_end;
  const unsigned* follows; const int* edge_map; const int* stop;
  int N, F, G, T, L, fw, off, ntok;
  int *len, *type, *closed, *loops, *edges, *loop_of; unsigned* set_bits; double* score;
};

struct FaceWaveLds {
  int e[FACE_T];        // the face's edges in decode order
  int aux[FACE_T];      // 1: edge i follows edge i-1; later the mapped edge of the key
  int lid[FACE_T];      // loop number of edge i
  int lstart[FACE_T];   // per loop: first position, length, smallest edge and its position, offset and number in canonical order
  int llen[FACE_T];
  int lminv[FACE_T];
  int lminp[FACE_T];
  int loff[FACE_T];
  int lnum[FACE_T];
  float lp[FACE_T];
};

__global__ __launch_bounds__(FACE_WAVES * FF_WAVE) void face_rows_kernel(FaceRowsArgs a) {
  __shared__ FaceWaveLds s_all[FACE_WAVES];
  const int lane = face_lane();
  const int wave = threadIdx.x / FF_WAVE;
  FaceWaveLds& s = s_all[wave];
  const long long R = (long long)a.F * a.G;
  const long long row = (long long)blockIdx.x * FACE_WAVES + wave;
  if (row >= (long long)a.N * R) return;      // (whole waves leave; the kernel has no block-wide barrier)
  const int w = (int)(row / R);
  const int f = (int)((row % R) / a.G);
  const int T = a.T, ntok = a.ntok, off = a.off;
  int ne = a.num_edges ? a.num_edges[w] : a.num_input[w];
  ne = ne < 0 ? 0 : (ne > a.L ? a.L : ne);
  const int stop = a.stop ? a.stop[w] : T - 1;

  bool face = f < a.num_input[w];
  if (a.scores && a.scores[row] == -INFINITY) face = false;
  if (a.dead_end && a.dead_end[row] != 0) face = false;

  // tokens: position p = lane + 64 k, zero behind the wireframe's own stop
  int64_t tok[FACE_K];
  const int64_t* trow = a.tokens + (size_t)row * T;
#pragma unroll
  for (int k = 0; k < FACE_K; ++k) {
    const int p = lane + FF_WAVE * k;
    tok[k] = (face && p < T && p <= stop) ? trow[p] : 0;
  }
  // fin: the first terminator, T - 1 without one
  int fin = T - 1;
  bool found = false;
#pragma unroll
  for (int k = 0; k < FACE_K; ++k) {
    const int p = lane + FF_WAVE * k;
    const unsigned long long b = __ballot(p < T && tok[k] >= off && tok[k] < ntok);
    if (!found && b) { found = true; fin = FF_WAVE * k + face_first(b); }
  }
  int64_t tfin = 0;
#pragma unroll
  for (int k = 0; k < FACE_K; ++k) {
    const long long v = __shfl((long long)tok[k], fin % FF_WAVE, FF_WAVE);
    if (fin / FF_WAVE == k) tfin = v;
  }
  // edges, compacted in order
  int len = 0;
#pragma unroll
  for (int k = 0; k < FACE_K; ++k) {
    const int p = lane + FF_WAVE * k;
    const int64_t v = tok[k] - ntok;
    const bool is_edge = face && p < T && p <= fin && v >= 0 && v < ne;
    const unsigned long long b = __ballot(is_edge);
    if (is_edge) s.e[len + face_prefix(b)] = (int)v;
    len += __popcll(b);
  }
  face_sync();
  if (len == 0) face = false;

  int* out_edges = a.edges + (size_t)row * T;
  int* out_loop = a.loop_of + (size_t)row * T;
  unsigned* out_bits = a.set_bits + (size_t)row * a.fw;
  if (!face) {
    for (int p = lane; p < T; p += FF_WAVE) { out_edges[p] = -1; out_loop[p] = -1; }
    for (int x = lane; x < a.fw; x += FF_WAVE) out_bits[x] = 0u;
    if (lane == 0) {
      a.len[row] = 0; a.type[row] = 0; a.closed[row] = a.follows ? 0 : -1; a.loops[row] = 0; a.score[row] = 0.0;
    }
    return;
  }

  // score: the given one, or the fp64 sum of the log-probabilities over 1 .. fin in ascending order
  double score = 0.0;
  if (a.scores) score = (double)a.scores[row];
  if (a.logprob) {
    const float* lrow = a.logprob + (size_t)row * T;
    for (int p = lane; p < T; p += FF_WAVE) s.lp[p] = (p <= stop) ? lrow[p] : 0.f;
    face_sync();
    if (lane == 0)
      for (int p = 1; p <= fin; ++p) score += (double)s.lp[p];
  }
  face_sync();

  // enclosure walk: sequential in loops.  Per loop and 64 edges: one ballot of "closes onto first", one of "does not follow
  // its predecessor"; a failed connect before or at the closure ends the walk
  int closed = -1, loops = 0;
  if (a.follows) {
    const unsigned* ftab = a.follows + (size_t)w * a.L * a.fw;
    for (int i = lane; i < len; i += FF_WAVE) {
      int c = 0;
      if (i > 0) { const int pe = s.e[i - 1], ce = s.e[i]; c = (ftab[(size_t)pe * a.fw + (ce >> 5)] >> (ce & 31)) & 1u; }
      s.aux[i] = c;
    }
    face_sync();
    int start = 0;
    closed = 1;
    while (start < len && closed == 1) {
      const int first = s.e[start];
      int close_at = -1;
      for (int base = start; base < len; base += FF_WAVE) {
        const int i = base + lane;
        bool closes = false, fails = false;
        if (i < len) {
          const int ce = s.e[i];
          closes = (ftab[(size_t)ce * a.fw + (first >> 5)] >> (first & 31)) & 1u;
          fails = i > start && !s.aux[i];
        }
        const int c = face_first(__ballot(closes)), x = face_first(__ballot(fails));
        if (x < FF_WAVE && x <= c) { closed = 0; break; }
        if (c < FF_WAVE) { close_at = base + c; break; }
      }
      if (closed == 0) break;
      if (close_at < 0) { closed = 0; break; }       // the last edge does not close its loop
      for (int i = start + lane; i <= close_at; i += FF_WAVE) s.lid[i] = loops;
      if (lane == 0) { s.lstart[loops] = start; s.llen[loops] = close_at - start + 1; }
      ++loops;
      start = close_at + 1;
    }
    if (closed == 0) loops = 0;
    face_sync();
  }

  // canonical order of a closed face: every loop rotated to its smallest edge (first occurrence), loops stably sorted by it
  if (closed == 1) {
    for (int l = lane; l < loops; l += FF_WAVE) {
      const int st = s.lstart[l], n = s.llen[l];
      int mv = s.e[st], mp = 0;
      for (int i = 1; i < n; ++i) { const int v = s.e[st + i]; if (v < mv) { mv = v; mp = i; } }
      s.lminv[l] = mv; s.lminp[l] = mp;
    }
    face_sync();
    for (int l = lane; l < loops; l += FF_WAVE) {
      const int mv = s.lminv[l];
      int o = 0, num = 0;
      for (int m = 0; m < loops; ++m) {
        const int v = s.lminv[m];
        if (v < mv || (v == mv && m < l)) { o += s.llen[m]; ++num; }
      }
      s.loff[l] = o; s.lnum[l] = num;
    }
    face_sync();
    for (int i = lane; i < len; i += FF_WAVE) {
      const int l = s.lid[i], n = s.llen[l];
      int q = i - s.lstart[l] - s.lminp[l];
      if (q < 0) q += n;
      const int at = s.loff[l] + q;
      out_edges[at] = s.e[i];
      out_loop[at] = s.lnum[l];
    }
  } else {
    for (int i = lane; i < len; i += FF_WAVE) { out_edges[i] = s.e[i]; out_loop[i] = -1; }
  }
  for (int p = len + lane; p < T; p += FF_WAVE) { out_edges[p] = -1; out_loop[p] = -1; }

  // key: the bitmap of the mapped edges; a lane owns whole words
  const int* emap = a.edge_map ? a.edge_map + (size_t)w * a.L : nullptr;
  face_sync();
  for (int i = lane; i < len; i += FF_WAVE) {
    const int e = s.e[i];
    int m = emap ? emap[e] : e;
    if (m < 0 || m >= a.L) m = e;
    s.aux[i] = m;
  }
  face_sync();
  for (int x = lane; x < a.fw; x += FF_WAVE) {
    unsigned word = 0u;
    for (int i = 0; i < len; ++i) { const int m = s.aux[i]; if ((m >> 5) == x) word |= 1u << (m & 31); }
    out_bits[x] = word;
  }
  if (lane == 0) {
    a.len[row] = len; a.type[row] = (int)(tfin - off); a.closed[row] = closed; a.loops[row] = loops; a.score[row] = score;
  }
}

// ---- votes ---------------------------------------------------------------------------------------------------------------------
constexpr int VOTE_THREADS = 1024;

struct FaceVotesArgs {
  const unsigned* set_bits; const int* len; const int* type; const int* closed; const double* score;
  int R, fw, cap, require_closed;
  int *rep, *votes, *major, *num_faces; unsigned long long* best;   // best: fp64 on return, ordered keys in between
  int* table;                 // per wireframe: claim[cap], least[cap], count[cap]
  unsigned long long* pack;   // per wireframe: [R]
  size_t table_stride, pack_stride;
};

__device__ __forceinline__ int vote_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename V>
__device__ __forceinline__ void vote_store(V* p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned vote_mix(unsigned h) {
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}
// a total order on doubles as unsigned integers (-0 below +0)
__device__ __forceinline__ unsigned long long vote_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double vote_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// One block per wireframe.  Pass 1 groups the participating rows by their bitmap: an open-addressing table of row indices; the
// hash only chooses where the probe starts, a slot is claimed by compare-and-swap and a row joins the slot whose claimant's
// bitmap equals its own, word for word.  Every bitmap therefore ends in exactly one slot, whichever row claimed it, and
// rep = the least row of the slot (atomicMin).  Pass 2 groups by (rep, type) in the same way for the type counts.  Everything
// that leaves the block is a minimum, a maximum or an integer sum: the result does not depend on which row came first.
__global__ __launch_bounds__(VOTE_THREADS) void face_votes_kernel(FaceVotesArgs a) {
  __shared__ int s_faces;
  const int w = blockIdx.x, tid = threadIdx.x;
  const int lane = face_lane(), wave = tid / FF_WAVE, nwaves = VOTE_THREADS / FF_WAVE;
  const int R = a.R, fw = a.fw, cap = a.cap, mask = a.cap - 1;
  const size_t r0 = (size_t)w * R;
  int* claim = a.table + (size_t)w * a.table_stride;
  int* least = claim + cap;
  int* count = least + cap;
  unsigned long long* pack = a.pack + (size_t)w * a.pack_stride;
  const unsigned* bits = a.set_bits + r0 * fw;
  const int* len = a.len + r0;
  const int* type = a.type + r0;
  const int* closed = a.closed + r0;
  int* rep = a.rep + r0;

  if (tid == 0) s_faces = 0;
  for (int i = tid; i < cap; i += VOTE_THREADS) { vote_store(&claim[i], -1); vote_store(&least[i], 0x7fffffff); vote_store(&count[i], 0); }
  for (int r = tid; r < R; r += VOTE_THREADS) {
    vote_store(&pack[r], 0ull); vote_store(&a.best[r0 + r], 0ull); vote_store(&a.votes[r0 + r], 0);
    a.major[r0 + r] = 0;
  }
  __syncthreads();

  // pass 1: one wave per row
  for (int r = wave; r < R; r += nwaves) {
    const bool in = len[r] > 0 && (!a.require_closed || closed[r] == 1);
    int slot = -1;
    if (in) {
      const unsigned* mine = bits + (size_t)r * fw;
      unsigned h = 0u;
      for (int x = lane; x < fw; x += FF_WAVE) h += vote_mix(mine[x] ^ ((unsigned)x * 0x9e3779b9u));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, FF_WAVE);
      slot = (int)(vote_mix(h) & (unsigned)mask);
      for (;;) {                                  // (at most 2 R <= cap slots are ever claimed: an empty one is found)
        int c = 0;
        if (lane == 0) { c = atomicCAS(&claim[slot], -1, r); if (c == -1) c = r; }
        c = __shfl(c, 0, FF_WAVE);
        bool same = true;
        if (c != r) {
          const unsigned* theirs = bits + (size_t)c * fw;
          for (int x = lane; x < fw; x += FF_WAVE) same = same && mine[x] == theirs[x];
        }
        if (__ballot(!same) == 0ull) break;
        slot = (slot + 1) & mask;
      }
      if (lane == 0) atomicMin(&least[slot], r);
    }
    if (lane == 0) rep[r] = slot;                 // (the slot for now)
  }
  __syncthreads();
  for (int r = tid; r < R; r += VOTE_THREADS) { const int sl = rep[r]; rep[r] = sl < 0 ? -1 : vote_load(&least[sl]); }
  __syncthreads();
  for (int i = tid; i < cap; i += VOTE_THREADS) { vote_store(&claim[i], -1); vote_store(&least[i], 0x7fffffff); }
  __syncthreads();

  // pass 2: one thread per row; groups of (rep, type)
  for (int r = tid; r < R; r += VOTE_THREADS) {
    const int p = rep[r];
    if (p < 0) continue;
    const int t = type[r];
    atomicMax(&a.best[r0 + p], vote_key(a.score[r0 + r]));
    int slot = (int)(vote_mix((unsigned)p * 0x9e3779b9u ^ vote_mix((unsigned)t)) & (unsigned)mask);
    for (;;) {
      int c = atomicCAS(&claim[slot], -1, r);
      if (c == -1) c = r;
      if (c == r || (rep[c] == p && type[c] == t)) break;
      slot = (slot + 1) & mask;
    }
    atomicAdd(&count[slot], 1);
    atomicMin(&least[slot], r);
  }
  __syncthreads();
  // the most frequent type of every group; on a tie the type whose first row is the lowest
  for (int i = tid; i < cap; i += VOTE_THREADS) {
    const int c = vote_load(&claim[i]);
    if (c < 0) continue;
    const int p = rep[c], n = vote_load(&count[i]), first = vote_load(&least[i]);
    atomicMax(&pack[p], ((unsigned long long)(unsigned)n << 32) | (unsigned long long)(0xffffffffu - (unsigned)first));
    atomicAdd(&a.votes[r0 + p], n);
  }
  __syncthreads();
  int mine = 0;
  for (int r = tid; r < R; r += VOTE_THREADS) {
    if (rep[r] != r) continue;
    ++mine;
    const unsigned long long pk = __hip_atomic_load(&pack[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int first = (int)(0xffffffffu - (unsigned)(pk & 0xffffffffull));
    if (first >= 0 && first < R) a.major[r0 + r] = type[first];
    const unsigned long long k = __hip_atomic_load(&a.best[r0 + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.best[r0 + r] = (unsigned long long)__double_as_longlong(vote_unkey(k));
  }
  if (mine) atomicAdd(&s_faces, mine);
  __syncthreads();
  if (tid == 0) a.num_faces[w] = s_faces;
}

// ---- the single-sequence model's rows --------------------------------------------------------------------------
constexpr int SEQ_T = FF_FACE_SEQ_MAX_T;   // positions of a row
constexpr int SEQ_P = SEQ_T / 2;           // face slots of a row: a face takes an edge and a boundary
constexpr int SEQ_THREADS = 256;

struct FaceSeqArgs {
  const int64_t* tokens; const int* num_edges; const float* scores; const float* logprob; const int* finished;
  const unsigned* follows; const int* edge_map;
  int G, T, L, fw, ntok, sep, eos, P, closed_only;
  int *count, *len, *start, *type, *closed, *loops, *edges, *loop_of; unsigned* set_bits; double* score;
  int *dup_of, *take; double* row_best;
};

// 57 KB: every index below is under 2048 and held in 16 bits.  The per-loop records of a slot (llen .. lnum, lminv) live at
// [start, start + loops) of the slot's own edge range: a face has at most as many loops as edges.
struct FaceSeqLds {
  int e[SEQ_T];                    // the row's edges in decode order, all slots behind one another
  int aux[SEQ_T];                  // per loop: its smallest edge; later per edge: the mapped edge of the key
  unsigned short lid[SEQ_T];       // per edge: loop number inside its slot
  unsigned short slot_of[SEQ_T];   // per edge: its slot
  unsigned short llen[SEQ_T];      // per loop: length, position of its smallest edge (first occurrence), and in canonical order
  unsigned short lrot[SEQ_T];      //   its offset inside the slot and its number
  unsigned short loff[SEQ_T];
  unsigned short lnum[SEQ_T];
  unsigned short start[SEQ_P];     // per slot: first edge, edges, first and last position of the piece
  unsigned short len[SEQ_P];
  unsigned short pbeg[SEQ_P];
  unsigned short pend[SEQ_P];
  unsigned short loops[SEQ_P];
  short dup[SEQ_P];
  unsigned hash[SEQ_P];
  signed char closed[SEQ_P];
  int count, edges_total;
};

__device__ __forceinline__ unsigned long long seq_below(int lane) { return (1ull << lane) - 1ull; }

// One block per row.  Wave 0 parses (two passes over chunks of 64 positions, every decision a ballot and a prefix count); the slots,
// the edges, the words of the keys and the fold are then spread over the block, one thread per slot wherever a step is sequential.
__global__ __launch_bounds__(SEQ_THREADS) void face_seq_rows_kernel(FaceSeqArgs a) {
  __shared__ FaceSeqLds s;
  const int tid = threadIdx.x, lane = face_lane();
  const size_t row = blockIdx.x;
  const int w = (int)(row / (size_t)a.G);
  const int T = a.T, P = a.P, fw = a.fw, ntok = a.ntok;
  int ne = a.num_edges[w];
  ne = ne < 0 ? 0 : (ne > a.L ? a.L : ne);
  const int64_t* trow = a.tokens + row * (size_t)T;

  if (tid < FF_WAVE) {
    bool face = !(a.scores && a.scores[row] == -INFINITY);
    const bool cut_zeros = a.finished && a.finished[row] == 0;
    // end: T - 1, or the last nonzero position of an unfinished row; then the first EOS at or before it
    int last_nz = -1, first_eos = -1;
    if (face)
      for (int base = 0; base < T; base += FF_WAVE) {
        const int p = base + lane;
        const int64_t v = p < T ? trow[p] : 0;
        const unsigned long long nz = __ballot(p < T && v != 0), eo = __ballot(p < T && v == (int64_t)a.eos);
        if (nz) last_nz = base + 63 - __clzll((long long)nz);
        if (first_eos < 0 && eo) first_eos = base + face_first(eo);
      }
    int end = cut_zeros ? last_nz : T - 1;
    if (end < 0) face = false;
    if (first_eos >= 0 && first_eos <= end) end = first_eos;
    // pieces, faces and edges: running counts over the chunks
    int edges_run = 0, faces_run = 0, last_eb = 0, last_bpos = -1;
    if (face)
      for (int base = 0; base <= end; base += FF_WAVE) {
        const int p = base + lane;
        const int64_t v = p <= end ? trow[p] : 0;
        const bool bound = p <= end && (v == (int64_t)a.sep || p == end);
        const bool is_edge = p <= end && !bound && v >= (int64_t)ntok && v - (int64_t)ntok < (int64_t)ne;
        const unsigned long long bb = __ballot(bound), eb = __ballot(is_edge);
        const int before = edges_run + face_prefix(eb);          // edges in front of this position
        if (is_edge) s.e[before] = (int)(v - ntok);
        // a boundary closes the piece behind the boundary before it
        int prev_eb = last_eb, prev_bpos = last_bpos;
        const unsigned long long lower = bb & seq_below(lane);
        if (lower) {
          const int pl = 63 - __clzll((long long)lower);
          prev_eb = edges_run + __popcll(eb & seq_below(pl));
          prev_bpos = base + pl;
        }
        const bool is_face = bound && before > prev_eb;
        const unsigned long long fb = __ballot(is_face);
        const int slot = faces_run + face_prefix(fb);
        if (is_face && slot < P) {
          s.start[slot] = (unsigned short)prev_eb; s.len[slot] = (unsigned short)(before - prev_eb);
          s.pbeg[slot] = (unsigned short)(prev_bpos + 1); s.pend[slot] = (unsigned short)p;
        }
        if (bb) {
          const int hl = 63 - __clzll((long long)bb);
          last_eb = edges_run + __popcll(eb & seq_below(hl));
          last_bpos = base + hl;
        }
        edges_run += __popcll(eb);
        faces_run += __popcll(fb);
      }
    if (lane == 0) s.count = faces_run;
  }
  __syncthreads();
  const int count = s.count;
  const int filled = count < P ? count : P;
  if (tid == 0) {
    s.edges_total = filled ? (int)s.start[filled - 1] + (int)s.len[filled - 1] : 0;
    a.count[row] = count;
  }
  __syncthreads();
  const int E = s.edges_total;
  const size_t slot0 = row * (size_t)P;
  const unsigned* ftab = a.follows ? a.follows + (size_t)w * a.L * fw : nullptr;

  // per slot, one thread: the score and the enclosure walk with the per-loop minima
  for (int sl = tid; sl < P; sl += SEQ_THREADS) {
    const size_t o = slot0 + sl;
    if (sl >= filled) {
      a.len[o] = 0; a.start[o] = 0; a.type[o] = 0; a.closed[o] = ftab ? 0 : -1; a.loops[o] = 0; a.score[o] = 0.0;
      a.dup_of[o] = -1; a.take[o] = 0; a.row_best[o] = 0.0;
      continue;
    }
    const int st = s.start[sl], n = s.len[sl];
    double score = 0.0;
    if (a.scores) score = (double)a.scores[row];
    if (a.logprob) {
      const float* lrow = a.logprob + row * (size_t)T;
      const int pe = s.pend[sl];
      for (int p = s.pbeg[sl]; p <= pe; ++p) score += (double)lrow[p];
    }
    int closed = -1, loops = 0;
    if (ftab) {
      closed = 1;
      int cur = st, first = 0, prev = 0, mv = 0, mp = 0;
      for (int i = st; i < st + n; ++i) {
        const int ce = s.e[i];
        if (i == cur) { first = ce; mv = ce; mp = i; }
        else {
          if (!((ftab[(size_t)prev * fw + (ce >> 5)] >> (ce & 31)) & 1u)) { closed = 0; break; }
          if (ce < mv) { mv = ce; mp = i; }
        }
        s.lid[i] = (unsigned short)loops;
        s.slot_of[i] = (unsigned short)sl;
        prev = ce;
        if ((ftab[(size_t)ce * fw + (first >> 5)] >> (first & 31)) & 1u) {
          s.llen[st + loops] = (unsigned short)(i - cur + 1); s.lrot[st + loops] = (unsigned short)mp; s.aux[st + loops] = mv;
          ++loops;
          cur = i + 1;
        }
      }
      if (closed == 1 && cur != st + n) closed = 0;      // the last edge does not close its loop
      if (closed == 0) {
        loops = 0;
        for (int i = st; i < st + n; ++i) s.slot_of[i] = (unsigned short)sl;
      }
    }
    s.closed[sl] = (signed char)closed; s.loops[sl] = (unsigned short)loops;
    a.len[o] = n; a.start[o] = st; a.type[o] = 0; a.closed[o] = closed; a.loops[o] = loops; a.score[o] = score;
  }
  __syncthreads();

  // canonical order of the closed faces: every loop rotated to its smallest edge, the loops of a face stably sorted by it
  if (ftab) {
    for (int i = tid; i < E; i += SEQ_THREADS) {
      const int sl = s.slot_of[i], st = s.start[sl], l = i - st, nl = s.closed[sl] == 1 ? (int)s.loops[sl] : 0;
      if (l >= nl) continue;
      const int mv = s.aux[i];
      int o = 0, num = 0;
      for (int m = 0; m < nl; ++m) {
        const int v = s.aux[st + m];
        if (v < mv || (v == mv && m < l)) { o += s.llen[st + m]; ++num; }
      }
      s.loff[i] = (unsigned short)o; s.lnum[i] = (unsigned short)num;
    }
    __syncthreads();
  }
  int* out_edges = a.edges + row * (size_t)T;
  int* out_loop = a.loop_of + row * (size_t)T;
  for (int i = tid; i < T; i += SEQ_THREADS) {
    if (i >= E) { out_edges[i] = -1; out_loop[i] = -1; continue; }
    int at = i, num = -1;
    if (ftab) {
      const int sl = s.slot_of[i];
      if (s.closed[sl] == 1) {
        const int rec = s.start[sl] + s.lid[i], n = s.llen[rec];
        int q = i - (int)s.lrot[rec];
        if (q < 0) q += n;
        at = s.start[sl] + s.loff[rec] + q;
        num = s.lnum[rec];
      }
    }
    out_edges[at] = s.e[i];
    out_loop[at] = num;
  }
  __syncthreads();

  // keys: the mapped edges, then one thread per word
  const int* emap = a.edge_map ? a.edge_map + (size_t)w * a.L : nullptr;
  for (int i = tid; i < E; i += SEQ_THREADS) {
    const int e = s.e[i];
    int m = emap ? emap[e] : e;
    if (m < 0 || m >= a.L) m = e;
    s.aux[i] = m;
  }
  __syncthreads();
  unsigned* out_bits = a.set_bits + slot0 * (size_t)fw;
  for (size_t x = tid; x < (size_t)P * fw; x += SEQ_THREADS) {
    const int sl = (int)(x / fw), wd = (int)(x % fw);
    unsigned word = 0u;
    if (sl < filled) {
      const int st = s.start[sl], n = s.len[sl];
      for (int i = st; i < st + n; ++i) { const int m = s.aux[i]; if ((m >> 5) == wd) word |= 1u << (m & 31); }
    }
    out_bits[x] = word;
  }
  __syncthreads();      // (the words are read back below by other threads of the block)

  // fold the duplicates of the row: the hash only filters, the words decide
  for (int sl = tid; sl < filled; sl += SEQ_THREADS) {
    unsigned h = 0u;
    const unsigned* mine = out_bits + (size_t)sl * fw;
    for (int x = 0; x < fw; ++x) h += vote_mix(mine[x] ^ ((unsigned)x * 0x9e3779b9u));
    s.hash[sl] = h;
  }
  __syncthreads();
  for (int sl = tid; sl < filled; sl += SEQ_THREADS) {
    const bool part = !a.closed_only || s.closed[sl] == 1;
    int dup = -1;
    if (part) {
      const unsigned h = s.hash[sl];
      const unsigned* mine = out_bits + (size_t)sl * fw;
      for (int o = 0; o < sl && dup < 0; ++o) {
        if (s.hash[o] != h || (a.closed_only && s.closed[o] != 1)) continue;
        const unsigned* theirs = out_bits + (size_t)o * fw;
        bool same = true;
        for (int x = 0; x < fw && same; ++x) same = mine[x] == theirs[x];
        if (same) dup = o;
      }
    }
    s.dup[sl] = (short)(part ? dup : -2);      // (-2: takes no part)
  }
  __syncthreads();
  for (int sl = tid; sl < filled; sl += SEQ_THREADS) {
    const size_t o = slot0 + sl;
    const int dup = s.dup[sl];
    const double own = a.score[o];
    double best = own;
    if (dup == -1) {
      unsigned long long k = vote_key(own);
      for (int m = sl + 1; m < filled; ++m)
        if (s.dup[m] == sl) { const unsigned long long km = vote_key(a.score[slot0 + m]); k = km > k ? km : k; }
      best = vote_unkey(k);
    }
    a.dup_of[o] = dup < 0 ? -1 : dup; a.take[o] = dup == -1 ? 1 : 0; a.row_best[o] = best;
  }
}

int votes_cap(int R) {
  int cap = 64;
  while (cap < 2 * R) cap *= 2;
  return cap;
}
size_t votes_table_stride(int R) { return (size_t)3 * votes_cap(R); }                       // ints
size_t votes_pack_stride(int R) { return (size_t)R; }                                       // 8-byte words

}  // namespace

extern "C" int ff_face_rows(const int64_t* tokens, int N, int F, int G, int T, const int* num_input, const int* num_edges, int L,
                            int off, int ntok, const float* scores, const float* logprob, const int* dead_end,
                            const unsigned* follows, const int* edge_map, int flags, int* len, int* type, int* closed, int* loops,
                            int* edges, int* loop_of, unsigned* set_bits, double* score, ff_stream_t stream) {
  FF_CHECK_ARG(T >= 1 && T <= FF_FACE_MAX_T, "ff_face_rows: T=%d outside 1..%d", T, FF_FACE_MAX_T);
  FF_CHECK_ARG(N >= 0 && F >= 0 && G >= 0 && L >= 0, "ff_face_rows: negative size N=%d F=%d G=%d L=%d", N, F, G, L);
  FF_CHECK_ARG(off >= 0 && off < ntok, "ff_face_rows: face_type_offset=%d must be in [0, len=%d)", off, ntok);
  FF_CHECK_ARG(!(flags & ~FF_FACE_OWN_STOP), "ff_face_rows: unknown flag bits %d", flags);
  FF_CHECK_ARG(!(scores && logprob), "ff_face_rows: scores and logprob may not both be given");
  const long long rows = (long long)N * F * G;
  if (rows == 0) return FF_OK;
  FF_CHECK_ARG(tokens && num_input, "ff_face_rows: tokens and num_input are required");
  FF_CHECK_ARG(len && type && closed && loops && edges && loop_of && score && (set_bits || L == 0),
               "ff_face_rows: an output pointer is null");
  FF_CHECK_ARG((rows + FACE_WAVES - 1) / FACE_WAVES < (1LL << 31), "ff_face_rows: %lld rows are too many", rows);
  hipStream_t st = (hipStream_t)stream;
  int* stop = nullptr;
  if (flags & FF_FACE_OWN_STOP) {
    float* area = nullptr;
    FF_RETURN_IF(ff_stream_scratch(st, (size_t)N * sizeof(int), &area));
    stop = reinterpret_cast<int*>(area);
  }
  FFProfScope prof(FF_CAT_ROWOP, (double)rows * T, st);
  if (stop) {
    hipLaunchKernelGGL(face_own_stop_kernel, dim3((unsigned)N), dim3(FACE_T), 0, st, tokens, num_input, F, G, T, ntok, stop);
    FF_CHECK_LAUNCH();
  }
  FaceRowsArgs a;
  a.tokens = tokens; a.num_input = num_input; a.num_edges = num_edges; a.scores = scores; a.logprob = logprob;
  a.dead_end = dead_end; a.follows = follows; a.edge_map = edge_map; a.stop = stop;
  a.N = N; a.F = F; a.G = G; a.T = T; a.L = L; a.fw = (L + 31) / 32; a.off = off; a.ntok = ntok;
  a.len = len; a.type = type; a.closed = closed; a.loops = loops; a.edges = edges; a.loop_of = loop_of; a.set_bits = set_bits;
  a.score = score;
  hipLaunchKernelGGL(face_rows_kernel, dim3((unsigned)((rows + FACE_WAVES - 1) / FACE_WAVES)), dim3(FACE_WAVES * FF_WAVE), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" size_t ff_face_votes_workspace_bytes(int N, int R) {
  if (N <= 0 || R <= 0 || R > FF_FACE_MAX_ROWS) return 0;
  return (size_t)N * (votes_table_stride(R) * sizeof(int) + votes_pack_stride(R) * sizeof(unsigned long long));
}

extern "C" int ff_face_votes(const unsigned* set_bits, const int* len, const int* type, const int* closed, const double* score, int N,
                             int R, int fw, int flags, int* rep, int* votes, double* best, int* major, int* num_faces,
                             void* workspace, size_t workspace_bytes, ff_stream_t stream) {
  FF_CHECK_ARG(N >= 0 && R >= 0 && fw >= 0, "ff_face_votes: negative size N=%d R=%d words=%d", N, R, fw);
  FF_CHECK_ARG(R <= FF_FACE_MAX_ROWS, "ff_face_votes: R=%d rows per wireframe above %d", R, FF_FACE_MAX_ROWS);
  FF_CHECK_ARG(!(flags & ~FF_FACE_REQUIRE_CLOSED), "ff_face_votes: unknown flag bits %d", flags);
  if (N == 0) return FF_OK;
  FF_CHECK_ARG(num_faces, "ff_face_votes: num_faces is null");
  hipStream_t st = (hipStream_t)stream;
  if (R == 0) {
    FF_CHECK_HIP(hipMemsetAsync(num_faces, 0, (size_t)N * sizeof(int), st));
    return FF_OK;
  }
  FF_CHECK_ARG((set_bits || fw == 0) && len && type && closed && score && rep && votes && best && major,
               "ff_face_votes: a null pointer");
  const size_t need = ff_face_votes_workspace_bytes(N, R);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
    ff_set_error("ff_face_votes: workspace of %zu bytes (8-byte aligned) needed, %zu given", need, workspace_bytes);
    return FF_ERR_WORKSPACE;
  }
  FaceVotesArgs a;
  a.set_bits = set_bits; a.len = len; a.type = type; a.closed = closed; a.score = score;
  a.R = R; a.fw = fw; a.cap = votes_cap(R); a.require_closed = (flags & FF_FACE_REQUIRE_CLOSED) ? 1 : 0;
  a.rep = rep; a.votes = votes; a.major = major; a.num_faces = num_faces; a.best = reinterpret_cast<unsigned long long*>(best);
  // the 8-byte words first, then the tables
  a.pack = static_cast<unsigned long long*>(workspace);
  a.pack_stride = votes_pack_stride(R);
  a.table = reinterpret_cast<int*>(a.pack + (size_t)N * a.pack_stride);
  a.table_stride = votes_table_stride(R);
  FFProfScope prof(FF_CAT_ROWOP, (double)N * R * (fw + 1), st);
  hipLaunchKernelGGL(face_votes_kernel, dim3((unsigned)N), dim3(VOTE_THREADS), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}

extern "C" int ff_face_seq_rows(const int64_t* tokens, int N, int G, int T, const int* num_edges, int L, int ntok, int sep, int eos,
                                int P, const float* scores, const float* logprob, const int* finished, const unsigned* follows,
                                const int* edge_map, int flags, int* count, int* len, int* start, int* type, int* closed, int* loops,
                                int* edges, int* loop_of, unsigned* set_bits, double* score, int* dup_of, int* take,
                                double* row_best, ff_stream_t stream) {
  FF_CHECK_ARG(T >= 1 && T <= FF_FACE_SEQ_MAX_T, "ff_face_seq_rows: T=%d outside 1..%d", T, FF_FACE_SEQ_MAX_T);
  FF_CHECK_ARG(P >= 1 && P <= (T / 2 > 1 ? T / 2 : 1), "ff_face_seq_rows: P=%d slots outside 1..max(T/2, 1) at T=%d", P, T);
  FF_CHECK_ARG(N >= 0 && G >= 0 && L >= 0, "ff_face_seq_rows: negative size N=%d G=%d L=%d", N, G, L);
  FF_CHECK_ARG(sep >= 0 && sep < ntok && eos >= 0 && eos < ntok && sep != eos,
               "ff_face_seq_rows: SEP=%d and EOS=%d must be two tokens of [0, len=%d)", sep, eos, ntok);
  FF_CHECK_ARG(!(flags & ~FF_FACE_SEQ_CLOSED_ONLY), "ff_face_seq_rows: unknown flag bits %d", flags);
  FF_CHECK_ARG(!(scores && logprob), "ff_face_seq_rows: scores and logprob may not both be given");
  FF_CHECK_ARG(tokens, "ff_face_seq_rows: tokens is null");
  const long long rows = (long long)N * G;
  if (rows == 0) return FF_OK;
  FF_CHECK_ARG(num_edges, "ff_face_seq_rows: num_edges is null");
  FF_CHECK_ARG(count && len && start && type && closed && loops && edges && loop_of && score && dup_of && take && row_best &&
               (set_bits || L == 0), "ff_face_seq_rows: an output pointer is null");
  FF_CHECK_ARG(rows < (1LL << 31), "ff_face_seq_rows: %lld rows are too many", rows);
  hipStream_t st = (hipStream_t)stream;
  FaceSeqArgs a;
  a.tokens = tokens; a.num_edges = num_edges; a.scores = scores; a.logprob = logprob; a.finished = finished; a.follows = follows;
  a.edge_map = edge_map;
  a.G = G; a.T = T; a.L = L; a.fw = (L + 31) / 32; a.ntok = ntok; a.sep = sep; a.eos = eos; a.P = P;
  a.closed_only = (flags & FF_FACE_SEQ_CLOSED_ONLY) ? 1 : 0;
  a.count = count; a.len = len; a.start = start; a.type = type; a.closed = closed; a.loops = loops; a.edges = edges;
  a.loop_of = loop_of; a.set_bits = set_bits; a.score = score; a.dup_of = dup_of; a.take = take; a.row_best = row_best;
  FFProfScope prof(FF_CAT_ROWOP, (double)rows * T, st);
  hipLaunchKernelGGL(face_seq_rows_kernel, dim3((unsigned)rows), dim3(SEQ_THREADS), 0, st, a);
  FF_CHECK_LAUNCH();
  return FF_OK;
}
