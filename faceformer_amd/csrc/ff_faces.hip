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
