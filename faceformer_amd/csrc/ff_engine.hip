// Whole-path engine: encoder and greedy pointer decode, driven from C++ so that one call enqueues
// every kernel of a wireframe batch (the Python host makes ONE ffi call per batch, not ~2700).
//
// Data layout in HBM (all fp32 unless stated):
//   memory   [N, S, E]          encoder output (post final LayerNorm), S = L + num_token
//   kvc[l]   [N*S, 2E]          cross-attention K | V of decoder layer l, projected ONCE per batch
//                               (the reference re-projects them per step over F copies of memory)
//   x0       [T, Bc, E]         per micro-batch, position-major decoder input: row (j, b) is the
//                               embedding row selected at position j of sequence b (append only)
//   tok      [T, Bc] int32      tokens, same indexing
//   qkv0     [T, Bc, 3E]        layer-0 self-attention q|k|v, filled one position per step
//   x,y,yq,o [R, E], qkv [R,3E], h [R, FF]   scratch for R = t*Bc active rows (position-major, so
//                               the active rows of step t are the first t*Bc rows: every GEMM of
//                               the step is one dense [t*Bc, K] x [K, N] product)
// Sequences b of a micro-batch belong to wireframe w0 + b / F; nothing is replicated per sequence.
//
// FF_RETIRE_FINISHED (opt-in, parallel variant): a micro-batch decodes a SLOT set -- slot i of the chunk holds sequence
// slot[i] (a chunk-local index of the plan above; tokens, traces, extra-mask rows and finish positions stay in that original
// order) -- and every sync_every steps the host drops the finished sequences from it (compact_chunks below).  The slots of a
// chunk keep the w = i / Fc structure with a smaller Fc, so attention, masks and kv_len are addressed as before.
//
// The opt-in decodes are the same run with another selection in place of the greedy pointer launch: a Mode (below) holds how a
// token is picked, which rule masks the row, whether the call is a single-sequence entry, the sequences per anchor and the operands
// and outputs; layout_decode, init_state, select_step and pack branch on those facts, behind one plan (plan_mode), one size query
// (decode_workspace_bytes), one step head (step_head) and one check of the entries' arguments (check_entry).  Their per-step
// records lie last in the workspace, named by role in DecodeBuffers (score, finished, parent, dead, first, prev, visited,
// byte_rows, ...), and the output is packed from the records up to the stop step.  select_step fills ONE ff_step_io (ff_common.h:
// what every selection launch takes) per step; a branch adds its records and operands.  The ruled branches share the rule's
// operands (rule_of) and the look-ahead's, the beam branches the parent trace and the reorder.
//   beam (ff_decode_beam): W sequences per anchor -- beam k of compact anchor a is chunk-local sequence a * W + k,
//     so a chunk's Fc / Bc are W times its anchor counts and w = i / Fc holds.  ff_beam_select (+ ff_beam_reorder of the x0 /
//     qkv0 prefixes); records (token, parent, score, finished).
//   forced (ff_decode_forced, both variants): the token array holds the caller's paths from the start,
//     ff_pointer_forced appends the FORCED token's row, every micro-batch runs max(lengths of its rows) steps, and there is no
//     stop rule: no counters, no check points, a loop and an epilogue of its own.
//   sample (ff_decode_sample): R sequences per anchor in the beam decode's layout, independent of each other -- no
//     reorder.  ff_pointer_sample reads the caller's uniforms through a per-sequence row_id; records (token, log-probability,
//     finished).
//   sequence sample (ff_decode_sequence_sample, single-sequence variant): the sampled decode's plan, records and
//     packing with F = 1 -- R draws per WIREFRAME, every one from SOS -- and the sequence form of ff_pointer_sample, whose counter
//     is "rows unfinished after the step": the decode stops at the first step that leaves 0 (the parallel rule's test on another
//     count; the cumulative EOS rule is not used).
//   sequence beam (ff_decode_sequence_beam, single-sequence variant): the beam decode's plan, records, reorder and
//     packing with F = 1 -- W beams per WIREFRAME, every one from SOS, beam 0 alone non-empty -- and a sequence form of
//     ff_beam_select, whose counter is "non-empty beams unfinished after the step" ("all") or "groups whose rank 0 is unfinished
//     after the step" ("best"): the decode stops at the first step that leaves 0.
//   sequence constrain (ff_decode_sequence_constrained, single-sequence variant): the greedy single-sequence plan
//     (F = 1, one sequence per wireframe, chunk_max_seqs) with constrain's records and state, every sequence from SOS, and
//     ff_pointer_sequence_constrained, whose counter is "rows unfinished after the step".
//   sequence constrain sample (ff_decode_sequence_constrained_sample): sequence sample's plan (R draws per wireframe)
//     with sequence constrain's records and state per draw plus row_id, and ff_pointer_sequence_constrained_sample.
//   constrain (ff_decode_constrained): the default plan, one sequence per anchor.  ff_pointer_constrained masks
//     the keys the enclosure walk could not accept; records and the rule's state (first, prev per step; visited words and the
//     byte mask per sequence).
//   constrain with look-ahead (ff_decode_constrained_ahead): constrain's plan, workspace, start state and packing;
//     only the selection launch differs -- ff_pointer_constrained_ahead with budget = T - 1 - position and the two distance
//     tables, operands offset per chunk as `follows` is.
//   constrain with exact look-ahead (ff_decode_constrained_exact): the same again with
//     ff_pointer_constrained_exact as the selection launch: budget = T - 1 - position and cycle_len as the one operand table.
//   constrained sample (ff_decode_constrained_sample): the sampled decode's plan -- R independent sequences per
//     anchor, no reorder -- with constrain's records and state per sequence (first, prev per step; visited words and the byte
//     mask per sequence) and the sampled decode's row_id.  ff_pointer_constrained_sample in one of its three forms, the
//     look-aheads with budget = T - 1 - position as above.
//   constrained beam (ff_decode_constrained_beam): the beam decode's plan, records and reorder with
//     ff_beam_constrained_select as the selection; also the cumulative dead flag per step, the rule's state in two halves that
//     the steps read and write alternately, and the byte mask per sequence.
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "ff_common.h"
#include "ff_device.h"
#include "ff_launch.h"

namespace {

struct Bump {
  char* base;
  size_t size, off;
  bool ok;
  Bump(void* p, size_t n) : base((char*)p), size(n), off(0), ok(true) {}
  template <typename T>
  T* take(size_t count) {
    size_t bytes = ff_align_up(count * sizeof(T), 256);
    if (off + bytes > size) { ok = false; off += bytes; return nullptr; }
    T* r = reinterpret_cast<T*>(base + off);
    off += bytes;
    return r;
  }
};

size_t bump_bytes(size_t count, size_t elem) { return ff_align_up(count * elem, 256); }

// ---- small kernels -----------------------------------------------------------------------------
// Start tokens of one micro-batch: sequence i belongs to wireframe i / Fc of the chunk and is its compact
// sequence f = f0 + i % Fc.
// With a slot map (FF_RETIRE_FINISHED) it also writes the start token of slot s's sequence to tok_slot[s], s < nslots.
__global__ void init_tokens_kernel(int* tok, int Bc, int Fc, int f0, const int* num_input, int variant,
                                   int pad_tok, int sos, const int* slot = nullptr, int* tok_slot = nullptr, int nslots = 0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot && i < nslots) {
    const int k = slot[i];
    tok_slot[i] = ff_start_token(f0 + k % Fc, num_input[k / Fc], pad_tok);
  }
  if (i >= Bc) return;
  tok[i] = variant == FF_PARALLEL ? ff_start_token(f0 + i % Fc, num_input[i / Fc], pad_tok) : sos;
}

// steps_done from the per-step counters (the reference's stop rules, model_para.py:232 / model.py:207-210)
// The counters are kept per (step, micro-batch) -- every pointer launch owns one, which it also publishes to the host
// (ff_pointer_count_block) -- and summed here into cnt_tot[step].
__global__ void steps_kernel(const int* __restrict__ cnt_ge, const int* __restrict__ cnt_eq, int nch, int variant, int N,
                             int steps_enqueued, int no_stop, int* __restrict__ cnt_tot, int* __restrict__ steps_done_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int* cnt = variant == FF_PARALLEL ? cnt_ge : cnt_eq;
  int steps = steps_enqueued, cum = 0;
  bool found = false;
  for (int s = 0; s < steps_enqueued; ++s) {
    int v = 0;
    for (int c = 0; c < nch; ++c) v += cnt[(size_t)s * nch + c];
    cnt_tot[s] = v;
    cum += v;
    if (!found && !no_stop && (variant == FF_PARALLEL ? v == 0 : cum == N)) { steps = s + 1; found = true; }
  }
  *steps_done_out = steps;
}

// predict[(w, fo), j] (int64) = token of the compact sequence that stands for output row fo of wireframe w,
// or 0 after the stop step.  With padding-anchor de-duplication every row fo >= num_input[w] is the ONE
// padding-anchor sequence stored at compact index num_input[w] (those rows are identical by construction:
// same start token, same memory, same mask; reference model_para.py:204-205).  One launch per micro-batch:
// it writes the rows whose compact sequence lives in [f0, f0 + Fc) of its wireframes.
// logprob (optional, laid out like predict): lp_all[j - 1, seq], the log-probability of the token at position j >= 1, under the
// same `last` rule; 0 in column 0 (the start token is not selected) and wherever predict is zero padded.
__global__ void finalize_chunk_kernel(const int* __restrict__ tok_all, int Btot, int T, const int* __restrict__ steps_p,
                                      const int* __restrict__ num_input, int dedup, int F, int w0, int nw, int Fc,
                                      int f0, int b0, int64_t* __restrict__ predict, int* __restrict__ seq_of_row,
                                      const int* __restrict__ fin, const float* __restrict__ lp_all = nullptr,
                                      float* __restrict__ logprob = nullptr) {
  const int steps = *steps_p;
  const size_t total = (size_t)nw * F * T;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % T);
    const int fo = (int)((i / T) % F), wl = (int)(i / ((size_t)T * F));
    int k;
    if (!ff_compact_seq(num_input, dedup, w0, wl, fo, Fc, f0, &k)) continue;
    const int seq = b0 + k;
    const size_t row = (size_t)(w0 + wl) * F + fo;
    const int last = fin ? (fin[seq] < steps ? fin[seq] : steps) : steps;   // FF_RETIRE_FINISHED: up to the finish position
    predict[row * T + j] = (j <= last) ? (int64_t)tok_all[(size_t)j * Btot + seq] : (int64_t)0;
    if (logprob) logprob[row * T + j] = (j >= 1 && j <= last) ? lp_all[(size_t)(j - 1) * Btot + seq] : 0.f;
    if (seq_of_row && j == 0) seq_of_row[row] = seq;
  }
}

// ---- host-side helpers ---------------------------------------------------------------------------
int check_model(const ff_model* m) {
  FF_CHECK_ARG(m != nullptr, "null model");
  FF_CHECK_ARG(m->E > 0 && m->H > 0 && m->E == m->H * FF_HEAD_DIM, "model: E=%d must equal H=%d * 64", m->E, m->H);
  FF_CHECK_ARG(m->FF > 0 && (m->FF & 3) == 0, "model: bad FF=%d", m->FF);
  FF_CHECK_ARG(m->num_enc_layers >= 0 && m->num_enc_layers <= FF_MAX_LAYERS && m->num_dec_layers > 0 &&
                   m->num_dec_layers <= FF_MAX_LAYERS, "model: bad layer counts");
  FF_CHECK_ARG(m->in_dim > 0 && (m->in_dim & 3) == 0, "model: in_dim=%d must be a multiple of 4", m->in_dim);
  FF_CHECK_ARG(m->num_token > 0, "model: num_token");
  FF_CHECK_ARG(m->split_kind >= 0 && m->split_kind <= 2, "model: split_kind=%d (0 = bf16 x 3 planes, 1 = fp16 x 2 planes, 2 = one fp16 plane)",
               m->split_kind);
  return FF_OK;
}

int gemm(const float* A, int lda, const float* A2, int n_split, const float* W, int ldw,
         const float* bias, const float* res, int ldr, float* C, int ldc, int M, int N, int K, int act,
         hipStream_t st) {
  return ff_gemm_f32(A, lda, A2, n_split, W, ldw, bias, res, ldr, C, ldc, M, N, K, act, 0, st);
}

// Rows from which the 3 x bf16 kernel beats the f32 family, by output width (profiles/r04/gemm_x3_variants.txt, one MI355X:
// N = 1536: 92 vs 65 TF/s at 1024 rows; N = 1024: 122 vs 94 at 2048 (69 vs 80 at 1024); the N = 512 projections, K = 512 or
// 1024: 96 vs 72 / 119 vs 89 at 3072 (67 vs 79 / 84 vs 93 at 2048)): x3_min_rows is the threshold of the widest product, the
// others need 7/4 and 11/4 times as many rows.
inline bool x3_wins(const ff_decode_params* prm, int M, int N, int K, int lda) {
  if (prm->x3_min_rows <= 0 || (K % 32) != 0 || K < 64 || (N & 3) != 0) return false;
  if ((size_t)M * (size_t)lda >= ((size_t)1 << 30)) return false;   // the split kernel's 32-bit byte offsets (x3_check_common): f32 family instead
  const long need = (long)prm->x3_min_rows * (N >= 1536 ? 4 : (N >= 1024 ? ff_knob(FF_K_X3_NEED_N1024) : ff_knob(FF_K_X3_NEED_N512))) / 4;
  return M >= need;
}

// Are the split products of the decoder's projections bound and switched on at all?  (Layer 0 stands for all: a model binds them together.)
inline bool split_bound(const ff_model* m, const ff_decode_params* prm) {
  return prm->x3_min_rows > 0 && m->num_dec_layers > 0 && m->dec[0].in_proj_planes != nullptr;
}

// Does a decode step with R active rows take the split products?  Its widest product decides -- q|k|v, [R, E] x [E, 3E]: the
// steps whose projections take the split kernel also read the fp16 planes of the cross-attention K | V.
inline bool step_splits(const ff_model* m, const ff_decode_params* prm, long R) {
  return split_bound(m, prm) && x3_wins(prm, (int)R, 3 * m->E, m->E, m->E);
}

// One projection of the decoder: C = act(LN?(A) W^T + bias [+ table]) [+ residual], optionally leaving the row statistics of C.
struct Proj {
  const float *A = nullptr, *A2 = nullptr;   // columns >= n_split of the product read A2 (q|k from LN(x) + qpos, v from LN(x))
  const float *W = nullptr, *bias = nullptr, *res = nullptr;
  const void* planes = nullptr;              // (optional) the split planes of the [plane_rows, K] weight whose rows [row0, row0 + N) are W
  const float* colsum = nullptr;             // ... and its row sums (the epilogue form of the normalisation; used with st_in only)
  float* C = nullptr;
  const float *st_in = nullptr, *table = nullptr;   // segment statistics of A's rows (LN folded in); position table added per row
  float* st_out = nullptr;                   // segment statistics of C's rows for the next LayerNorm
  int lda = 0, n_split = 0, ldw = 0, plane_rows = 0, row0 = 0, ldr = 0, ldc = 0, M = 0, N = 0, K = 0, act = 0, ldt = 0, tcols = 0;
  Proj& in(const float* a, int ld, const float* a2 = nullptr, int ns = 0) { A = a; lda = ld; A2 = a2; n_split = ns; return *this; }
  Proj& weight(const float* w, int ld, const float* b) { W = w; ldw = ld; bias = b; return *this; }
  Proj& split(const void* pl, int rows, int r0 = 0, const float* cs = nullptr) { planes = pl; plane_rows = rows; row0 = r0; colsum = cs; return *this; }
  Proj& add(const float* r, int ld) { res = r; ldr = ld; return *this; }
  Proj& out(float* c, int ld, int m_, int n_, int k_, int a = 0) { C = c; ldc = ld; M = m_; N = n_; K = k_; act = a; return *this; }
  Proj& norm(const float* s) { st_in = s; return *this; }
  Proj& pos(const float* t, int ld, int cols) { table = t; ldt = ld; tcols = cols; return *this; }
  Proj& stats(float* s) { st_out = s; return *this; }
};

// The projection through the split kernel of the model's kind when the weight's planes are bound and the launch is in the range
// where it wins, through the f32 family otherwise.  A projection that reads or leaves row statistics, or adds a position table,
// takes the LayerNorm-folded forms (ff_gemm_*_ln; row_div: rows per position of that table); the others the plain forms.
int project(const ff_model* m, const ff_decode_params* prm, int row_div, hipStream_t st, const Proj& d) {
  struct Kernels { decltype(&ff_gemm_x3) plain; decltype(&ff_gemm_x3_ln) ln; };
  static const Kernels by_kind[3] = {{ff_gemm_x3, ff_gemm_x3_ln}, {ff_gemm_x2h, ff_gemm_x2h_ln}, {ff_gemm_h1, ff_gemm_h1_ln}};
  // (0 = bf16 x 3 planes, 1 = fp16 x 2 planes, 2 = one fp16 plane: check_model; any other value takes the bf16 kernels, as before)
  const Kernels& sk = by_kind[m->split_kind == 1 || m->split_kind == 2 ? m->split_kind : 0];
  // what the split kernels do not have: a column split inside a 128-wide tile, folded statistics at K != 512, a table whose
  // width is not a multiple of 4 (each clause names operands of one form only: the other form leaves them null)
  const bool split = d.planes && x3_wins(prm, d.M, d.N, d.K, d.lda) && (!d.A2 || (d.n_split % 128) == 0) &&
                     (!d.st_in || d.K == 512) && (!d.table || (d.tcols & 3) == 0);
  if (!d.st_in && !d.table && !d.st_out) {
    if (split) return sk.plain(d.A, d.lda, d.A2, d.n_split, d.planes, d.bias, d.res, d.ldr, d.C, d.ldc, d.M, d.N, d.K, d.act, st);
    return gemm(d.A, d.lda, d.A2, d.n_split, d.W, d.ldw, d.bias, d.res, d.ldr, d.C, d.ldc, d.M, d.N, d.K, d.act, st);
  }
  ff_gemm_ln_desc g;
  memset(&g, 0, sizeof(g));
  g.A = d.A; g.lda = d.lda; g.W = d.W; g.ldw = d.ldw; g.bias = d.bias; g.residual = d.res; g.ldr = d.ldr; g.C = d.C; g.ldc = d.ldc;
  g.M = d.M; g.N = d.N; g.K = d.K; g.act = d.act; g.tile = 0;
  g.ln_stats_in = d.st_in; g.ln_nseg = d.K / 32; g.ln_eps = m->ln_eps;
  g.row_table = d.table; g.ld_row_table = d.ldt; g.row_div = row_div; g.row_cols = d.tcols;
  g.ln_stats_out = d.st_out;
  if (split) return sk.ln(&g, d.planes, d.plane_rows, d.row0, d.st_in ? d.colsum : nullptr, st);
  return ff_gemm_f32_ln(&g, st);
}

// Scratch of one in-flight micro-batch (one set per stream): R = t*Bc active rows, position-major.
struct Scratch {
  float *x, *y, *yq, *qkv, *o, *h, *p, *logits;
  float* lnstat;   // [R, E/32, 2] per-row segment statistics of x (FF_FUSE_LAYERNORM)
};

struct DecodeBuffers {
  float *mem_pos, *kvc[FF_MAX_LAYERS];
  unsigned char* kvp[FF_MAX_LAYERS];   // fp16 planes of the cross-attention K | V (2 x fp16 attention kernel) or null
  float *x0_all, *qkv0_all;
  float* x0stat_all;   // [Btot, E/32, 2] LayerNorm segment statistics of the NEWEST x0 rows (written by the pointer launches)
  float *fold_kt, *fold_ob;         // folded last-layer self-attention (FF_LAST_FOLD_MIN_ROWS): the per-call tables
                                    // kt [H, E + T, 64] and ob [E] (ff_attention_fold_tables), one block; or null
  float *projT, *pg_all, *pc_all;   // folded project + pointer GEMM of one-wireframe micro-batches (see pointer_fold): the transposed
                                    // folded project weight [E, E]; per micro-batch G = memory_w W' [S, E] and c = memory_w b' [S4]
  int* tok_all;   // [T, Btot] global, position-major
  float* lp_all;  // [T-1, Btot] log-probability of the token every step selected (ff_decode_lp with a logprob output), or null
  Scratch scr[FF_MAX_STREAMS];
  int* zeroed; size_t zeroed_count;   // cnt_ge | cnt_eq | arrive | seen as ONE block of zeroed_count ints: one fill per decode
  int *cnt_ge, *cnt_eq;   // [T, nch] per (step, micro-batch)
  int *arrive;            // [T, nch] arrivals of the pointer launches (counter hand-over to the host)
  int *seen;              // [Btot] FF_STOP_EACH_EOS: the sequence has produced an EOS
  int *cnt_tot;           // [T] per-step totals (steps_kernel)
  int *steps_dev;
  int *fin, *slot_all, *perm_all;   // FF_RETIRE_FINISHED: finish positions [Btot] (when not host-mapped), slot maps [Btot]
  // The opt-in modes' records, one pointer per role (layout_decode: which of them a mode has, and their sizes).  Per step, [T, Btot],
  // row s = the state after s steps (row 0: the start state); the tokens are tok_all's rows:
  float* score;             // beam, constrained beam: the beams' scores; sample, constrain: the log-probability of the step's token
  int *finished, *parent, *dead; // finished (all four); parent beam (the beam modes); dead end (constrain), cumulative (constrained beam)
  int* open;                // sequence-constrained beam: a loop is open after the step (the ping-pong state is overwritten past the stop)
  // The loop rule's state.  constrain: first, prev [T, Btot] per step; visited [Btot, ceil(L/32)] rewritten by every step.
  // constrained beam: two halves that the steps read and write alternately (first, prev: [2, Btot]; visited: [2, Btot, ceil(L/32)]:
  // step s reads half s & 1).  byte_rows [Btot, S]: the constraint byte rows, rewritten by every step.
  int *first, *prev;
  unsigned* visited;
  unsigned char* byte_rows;
  int* row_id;              // sample, constrained sample: [Btot] the draw every sequence reads, written once per call
  // forced: [T-1, Btot] each, row s = what step s scored (the forced token's log-probability is `score`; the argmax, the rank)
  int *greedy, *rank;
};

// A micro-batch is a contiguous range [b0, b0 + Bc) of the COMPACT sequence index: nw >= 1 consecutive
// wireframes with Fc sequences each (compact sequences [f0, f0 + Fc) of every one of them).  Without
// padding-anchor de-duplication the compact width of every wireframe is F and b = w*F + f as in the reference.
struct Chunk {
  int w0, nw, Fc, f0, b0, Bc, sid;
  // (beam decode: Fc, b0, Bc, Fl, Bl count beams -- W per anchor; f0 stays the chunk's first compact ANCHOR)
  int Fl, Bl;    // FF_RETIRE_FINISHED: slots per wireframe / in all of the chunk now (Bl = nw * Fl <= Bc; 0: nothing left)
  int *slot, *perm;   // ... device [Bc]: chunk-local sequence of every slot; the compaction's gather indices
  float* x0;     // [T, Bc, E]
  float* qkv0;   // [T, Bc, 3E] or null
  float* x0stat; // [Bc, E/32, 2] statistics of the rows the last pointer launch appended to x0, or null
  float *pg, *pc; // one-wireframe micro-batch with the folded forms bound: G [S, E] and c [S] (logits = LN(x) G^T + c), or null
};

// Compact width of wireframe w: its num_input real anchors plus ONE padding-anchor sequence when it has fewer
// than F (the reference decodes F - num_input identical copies of it, model_para.py:204-205).
inline bool retiring(const ff_decode_params* p) { return p->variant == FF_PARALLEL && (p->flags & FF_RETIRE_FINISHED); }

inline int compact_width(const ff_decode_params* p, const int* num_input_host, int w) {
  if (p->variant != FF_PARALLEL || !(p->flags & FF_DEDUP_PAD_ANCHORS) || !num_input_host) return p->F;
  int n = num_input_host[w];
  n = n < 0 ? 0 : n;
  return n < p->F ? n + 1 : p->F;
}

// Micro-batches: consecutive wireframes whose compact widths are within 25 % of the widest one share a chunk
// (its Fc = the widest; the narrower ones carry a few surplus padding-anchor copies), at most
// chunk_wireframes of them and at most chunk_max_seqs sequences; chunk_seqs > 0 additionally cuts every
// wireframe into sequence groups.  Callers that want tight chunks pass the wireframes sorted by edge count
// (the Python model does).
void plan_chunks(const ff_decode_params* p, const int* num_input_host, int ns, std::vector<Chunk>* out, int* btot,
                 int* max_bc, int* nchunks = nullptr) {
  const int N = p->N;
  int cw_lim = (p->chunk_wireframes <= 0 || p->chunk_wireframes > N) ? N : p->chunk_wireframes;
  // The single-sequence model decodes ONE sequence per wireframe (reference model.py:193-210: N sequences per step), so a
  // micro-batch of chunk_wireframes = 16 wireframes is 16 rows per position -- 64 wireframes then are 4 x 258 steps of
  // <= 4 128-row launches.  There the micro-batch is cut by SEQUENCES: up to chunk_max_seqs of them (0: chunk_wireframes as
  // before).  The cumulative EOS rule is untouched: every micro-batch adds to the same per-step counters.
  if (p->variant == FF_SEQ2SEQ && p->chunk_max_seqs > 0) cw_lim = p->chunk_max_seqs < N ? p->chunk_max_seqs : N;
  int b0 = 0, mx = 0, nc = 0;
  int w = 0;
  while (w < N) {
    int Fm = compact_width(p, num_input_host, w), Fmin = Fm, nw = 1;
    const bool split = p->chunk_seqs > 0 && p->chunk_seqs < Fm;
    while (!split && w + nw < N && nw < cw_lim) {
      const int c = compact_width(p, num_input_host, w + nw);
      const int nmax = c > Fm ? c : Fm, nmin = c < Fmin ? c : Fmin;
      if (4 * nmin < 3 * nmax) break;
      if (p->chunk_max_seqs > 0 && (long)(nw + 1) * nmax > (long)(p->chunk_max_seqs > nmax ? p->chunk_max_seqs : nmax)) break;
      Fm = nmax; Fmin = nmin; ++nw;
    }
    const int fstep = split ? p->chunk_seqs : Fm;
    for (int f0 = 0; f0 < Fm; f0 += fstep) {
      Chunk c{};   // (views into the workspace: bound by the decode)
      c.w0 = w; c.nw = nw; c.f0 = f0;
      c.Fc = (Fm - f0) < fstep ? (Fm - f0) : fstep;
      c.b0 = b0; c.Bc = nw * c.Fc;
      c.sid = (int)(out ? out->size() % (size_t)ns : 0);
      c.Fl = c.Fc; c.Bl = c.Bc;
      b0 += c.Bc;
      mx = c.Bc > mx ? c.Bc : mx;
      ++nc;
      if (out) out->push_back(c);
    }
    w += nw;
  }
  *btot = b0;
  *max_bc = mx;
  if (nchunks) *nchunks = nc;
}

// The plan of a beam decode: plan_chunks over the anchors (its sequence limits divided by W), every chunk W times as wide.
void plan_beam_chunks(const ff_decode_params* p, const int* num_input_host, int ns, int W, std::vector<Chunk>* out, int* btot,
                      int* max_bc, int* nchunks = nullptr) {
  ff_decode_params q = *p;
  if (q.chunk_max_seqs > 0) q.chunk_max_seqs = q.chunk_max_seqs / W > 1 ? q.chunk_max_seqs / W : 1;
  if (q.chunk_seqs > 0) q.chunk_seqs = q.chunk_seqs / W > 1 ? q.chunk_seqs / W : 1;
  plan_chunks(&q, num_input_host, ns, out, btot, max_bc, nchunks);
  if (out)
    for (Chunk& c : *out) { c.Fc *= W; c.b0 *= W; c.Bc *= W; c.Fl *= W; c.Bl *= W; }
  *btot *= W;
  *max_bc *= W;
}

int plan_streams(const ff_decode_params* p) {
  return p->num_streams < 1 ? 1 : (p->num_streams > FF_MAX_STREAMS ? FF_MAX_STREAMS : p->num_streams);
}

// What a decode call runs in place of the greedy pointer launch, as three independent facts -- how a token is picked, which rule
// masks the row, whether the call is a single-sequence entry -- plus the sequences per anchor G (W beams, R samples, else 1) and
// the operands and outputs that go with them.  Every entry resolves its own parameter struct into this ONCE per call; the engine
// branches on the facts and reads the fields, never on which entry it was.  A size query fills pick, rule, sequence and G only.
// A NEW MODE fills in: pick / rule / sequence / G; the operands of its rule (flags, follows, tok_sep), look-ahead (ahead,
// close_dist, cycle_len) and draw (uniforms, temperature, top_k, top_p); `op`, the name its selection launch reports errors under;
// every output pack() is to write (null: the mode has none).  Its entry also says in its Entry record whether all it requires is
// there.  If the combination of facts is new, layout_decode, init_state, select_step and pack each get the one branch it needs.
struct Mode {
  enum Pick { POINTER, FORCED, ARGMAX, DRAW, BEAM };   // the greedy pointer launch / the caller's token / the rule's arg-max / a draw / top-W
  enum Rule { NONE, LOOP, SEQUENCE };                  // no rule / the parallel loop rule (terminator range) / the sequence rule (SEP, EOS)
  Pick pick;
  Rule rule;
  bool sequence;   // a ff_decode_sequence_* entry: F = 1, every row from SOS, no num_input, stops at the first step whose counter is 0
  int G;
  int flags = 0, tok_sep = 0;         // the rule's operands
  const unsigned* follows = nullptr;
  int ahead = 0;                      // the look-ahead: 0 none, 1 the closure look-ahead, 2 the exact one; the whole batch's tables
  const unsigned char *close_dist = nullptr, *cycle_len = nullptr;
  const char* op = nullptr;           // the operator name the step's *_sync launch words its messages with
  const float* uniforms = nullptr;    // the draw's operands
  float temperature = 0.f, top_p = 0.f;
  int top_k = 0;
  int stop_best = 0;                  // the beam's operands
  int* trace_parent = nullptr;
  int64_t* rows = nullptr;            // the outputs: beams / samples ...
  float *scores = nullptr, *logprob = nullptr, *predict_logprob = nullptr;
  int *finished = nullptr, *dead_end = nullptr, *open_end = nullptr, *beam_dead_end = nullptr, *beam_open_end = nullptr,
      *predict_dead_end = nullptr, *predict_open_end = nullptr;
  const ff_forced_params* forced = nullptr;
  Mode(Pick k = POINTER, Rule r = NONE, bool seq = false, int g = 1) : pick(k), rule(r), sequence(seq), G(g) {}
  bool grouped() const { return pick == DRAW || pick == BEAM; }   // G sequences per anchor: the beam decode's plan and layout
};
// The groups of fields that several parameter structs spell alike, copied by name.
template <typename Q> void take_rule(Mode& md, const Q* q) { md.flags = q->flags; md.follows = q->follows; }
template <typename Q> void take_draw(Mode& md, const Q* q) {
  md.G = q->num_samples; md.uniforms = q->uniforms; md.temperature = q->temperature; md.top_k = q->top_k; md.top_p = q->top_p;
  md.rows = q->samples; md.logprob = q->logprob; md.scores = q->scores;
}
template <typename Q> void take_beam(Mode& md, const Q* q) {
  md.G = q->width; md.rows = q->beams; md.scores = q->scores; md.trace_parent = q->trace_parent;
}
template <typename Q> void take_ahead(Mode& md, int form, const Q* q, const unsigned char* close_dist) {
  md.ahead = form; md.close_dist = close_dist; md.cycle_len = q->cycle_len;
}

// The micro-batch plan of a mode: over the anchors, G times as wide, where G sequences per anchor exist (with FF_SEQ2SEQ a
// micro-batch is cut by sequences: chunk_max_seqs / G wireframes, at least one); without de-duplication for forced (the rows are
// arbitrary paths: sequence b of the plan is row b); the default plan otherwise.
void plan_mode(const ff_decode_params* p, const int* num_input_host, int ns, const Mode& mode, std::vector<Chunk>* out, int* btot,
               int* max_bc, int* nchunks = nullptr) {
  if (mode.grouped()) return plan_beam_chunks(p, num_input_host, ns, mode.G, out, btot, max_bc, nchunks);
  if (mode.pick == Mode::FORCED) {
    ff_decode_params q = *p;
    q.flags &= ~FF_DEDUP_PAD_ANCHORS;
    return plan_chunks(&q, nullptr, ns, out, btot, max_bc, nchunks);
  }
  return plan_chunks(p, num_input_host, ns, out, btot, max_bc, nchunks);
}

// The tuning knobs that shape a decode, read ONCE per ff_decode / ff_decode_workspace_bytes call: the workspace
// layout and every step of that call see the same values whatever ff_set_tuning() does meanwhile.  The two that change the
// LAYOUT can also be switched off per call through ff_decode_params.flags (FF_NO_L0_FOLD, FF_NO_POINTER_FOLD).
constexpr int FF_PINNED_SLOTS = 65536;   // host-mapped stop counters allocated per device (knob FF_PINNED_COUNTERS: how many a decode may use)
struct EngineKnobs {
  bool l0_fold, pointer_fold, dbg_timing;
  bool x2h_attn;             // cross-attention K | V also as fp16 planes (FF_X2H_ATTN, with the fp16 split products in use)
  int one_launch_rows, pinned;
  int last_fold_rows;        // pruned last layer: k | v folded into the query from this many active rows on (0: never)
};
EngineKnobs engine_knobs(const ff_decode_params* p) {
  EngineKnobs k;
  k.l0_fold = ff_knob(FF_K_L0_FOLD) != 0 && !(p->flags & FF_NO_L0_FOLD);
  k.pointer_fold = ff_knob(FF_K_POINTER_FOLD) != 0 && !(p->flags & FF_NO_POINTER_FOLD);
  k.dbg_timing = ff_knob(FF_K_DEBUG_TIMING) != 0;
  k.x2h_attn = ff_knob(FF_K_X2H_ATTN) != 0;
  k.one_launch_rows = ff_knob(FF_K_LAST_QKV_ONE_LAUNCH_ROWS);
  k.last_fold_rows = ff_knob(FF_K_LAST_FOLD_MIN_ROWS);
  const int pc = ff_knob(FF_K_PINNED_COUNTERS);
  k.pinned = pc > 0 && pc < FF_PINNED_SLOTS ? pc : FF_PINNED_SLOTS;
  return k;
}

// LayerNorm fusion is possible when the folded weights are bound and the shapes fit the fused GEMM forms.
bool can_fuse_layernorm(const ff_model* m, const ff_decode_params* prm) {
  if (!(prm->flags & FF_FUSE_LAYERNORM)) return false;
  if (m->E % 64 != 0 || m->E < 128 || m->E > 512 || m->FF % 64 != 0 || m->FF < 128) return false;
  if (!m->proj_fold_w || !m->proj_fold_b) return false;
  for (int l = 0; l < m->num_dec_layers; ++l) {
    const ff_layer_weights& w = m->dec[l];
    if (!w.ln1_w || !w.ln1_b || !w.ln1_pos || !w.ln2_w || !w.ln2_b || !w.ln2_pos || !w.ln3_w || !w.ln3_b) return false;
  }
  return true;
}

// Workspace layout for `btot` compact sequences in micro-batches of at most `max_bc`.
// want_lp: also the log-probability rows (ff_decode_lp) -- taken LAST, so that everything else lies where it lies without them.
// mode: also its per-step records, last as well -- one ordered sequence of takes, each behind the fact that asks for it: score,
// finished; parent under a beam; dead under a rule; open under a beam with the sequence rule; the rule's first and prev (per step,
// or the two ping-pong halves under a beam); row_id for a draw; the rule's visited words (both halves under a beam) and byte rows.
// Forced has three arrays of its own.
size_t layout_decode(const ff_model* m, const ff_decode_params* p, const EngineKnobs& kn, size_t Btot, size_t Bch, size_t nch,
                     Bump& bp, DecodeBuffers* out, const Mode& mode, bool want_lp = false) {
  const int E = m->E, FFd = m->FF, S = p->L + m->num_token, T = p->T;
  const int ns = plan_streams(p);
  const size_t Rmax = (size_t)(T - 1 > 0 ? T - 1 : 1) * Bch;
  DecodeBuffers b;
  memset(&b, 0, sizeof(b));
  b.mem_pos = bp.take<float>((size_t)p->N * S * E);
  for (int l = 0; l < m->num_dec_layers; ++l) b.kvc[l] = bp.take<float>((size_t)p->N * S * 2 * E);
  // the package default's cross-attention runs on the fp16 matrix cores as well (ff_attention_x2h.hip): K | V of every (wireframe,
  // head) pair split once per batch into fp16 planes, 145 KB per pair and layer (key sets of at most 288 rows); the one-term kind
  // ("fp16", split_kind 2) uses the same planes and reads their first terms only
  const bool planes = kn.x2h_attn && (m->split_kind == 1 || m->split_kind == 2) && p->x3_min_rows > 0 && S <= 288 && m->dec[0].in_proj_planes != nullptr;
  for (int l = 0; l < m->num_dec_layers; ++l)
    b.kvp[l] = planes ? bp.take<unsigned char>(ff_attention_planes_bytes(p->N, m->H)) : nullptr;
  b.x0_all = bp.take<float>((size_t)T * Btot * E);
  b.tok_all = bp.take<int>((size_t)T * Btot);
  b.qkv0_all = (p->flags & FF_REUSE_LAYER0_QKV) ? bp.take<float>((size_t)T * Btot * 3 * E) : nullptr;
  // (FF_L0_FOLD=0 / FF_NO_L0_FOLD: the newest rows' LayerNorm as its own launch, as before round 5 -- A/B runs and tests of that form)
  b.x0stat_all = (kn.l0_fold && (p->flags & FF_REUSE_LAYER0_QKV) && can_fuse_layernorm(m, p)) ? bp.take<float>(Btot * (size_t)(E / 32) * 2)
                                                                                 : nullptr;   // (size query: take() returns null)
  // (FF_POINTER_FOLD=0 / FF_NO_POINTER_FOLD: project and the pointer GEMM as two launches, as before round 5)
  const bool pf = kn.pointer_fold && can_fuse_layernorm(m, p);
  b.projT = pf ? bp.take<float>((size_t)E * E) : nullptr;
  // (FF_LAST_FOLD_MIN_ROWS = 0, or more rows than a step of this call can have: no folded last layer, no tables)
  const bool lf = kn.last_fold_rows > 0 && Rmax >= (size_t)kn.last_fold_rows && (p->flags & FF_LAST_LAYER_LAST_ROW) && m->num_dec_layers > 1 && can_fuse_layernorm(m, p);
  b.fold_kt = lf ? bp.take<float>(ff_attention_fold_table_floats(E, m->H, T)) : nullptr;
  b.fold_ob = b.fold_kt ? b.fold_kt + (size_t)m->H * (E + T) * 64 : nullptr;
  b.pg_all = pf ? bp.take<float>(nch * (size_t)S * E) : nullptr;
  b.pc_all = pf ? bp.take<float>(nch * (size_t)((S + 3) & ~3)) : nullptr;
  for (int s = 0; s < ns; ++s) {
    Scratch& c = b.scr[s];
    c.x = bp.take<float>(Rmax * E);
    c.y = bp.take<float>(Rmax * E);
    c.yq = bp.take<float>(Rmax * E);
    c.qkv = bp.take<float>(Rmax * 3 * E);
    c.o = bp.take<float>(Rmax * E);
    c.h = bp.take<float>(Rmax * FFd);
    c.p = bp.take<float>(Bch * E);
    c.logits = bp.take<float>(Bch * (size_t)S);
    c.lnstat = bp.take<float>(Rmax * (size_t)(E / 32 + 1) * 2);
  }
  // the four counter arrays every decode starts from zero: ONE block, one fill (the [T, nch] ones padded to 256-byte units)
  const size_t ncnt = ff_align_up((size_t)T * nch * sizeof(int), 256) / sizeof(int);
  b.zeroed_count = 3 * ncnt + Btot;
  b.zeroed = bp.take<int>(b.zeroed_count);   // (size query: take() returns null)
  if (b.zeroed) { b.cnt_ge = b.zeroed; b.cnt_eq = b.cnt_ge + ncnt; b.arrive = b.cnt_eq + ncnt; b.seen = b.arrive + ncnt; }
  b.cnt_tot = bp.take<int>(T);
  b.steps_dev = bp.take<int>(4);
  if (retiring(p)) {
    b.fin = bp.take<int>(Btot);
    b.slot_all = bp.take<int>(Btot);
    b.perm_all = bp.take<int>(Btot);
  }
  if (want_lp) b.lp_all = bp.take<float>((size_t)(T - 1 > 0 ? T - 1 : 1) * Btot);
  // (every mode's arrays in the order and sizes they always had: tests/test_workspace_layout.py holds the table)
  const size_t TB = (size_t)T * Btot;
  const size_t fw = (size_t)(p->L + 31) / 32, vw = Btot * (fw > 0 ? fw : 1);   // visited words; one word per sequence at L = 0, so that the array is never empty
  const bool beam = mode.pick == Mode::BEAM, ruled = mode.rule != Mode::NONE;
  if (mode.pick == Mode::FORCED) {
    const size_t n = (size_t)(T - 1 > 0 ? T - 1 : 1) * Btot;
    b.score = bp.take<float>(n);
    b.greedy = bp.take<int>(n);
    b.rank = bp.take<int>(n);
  } else if (mode.pick != Mode::POINTER) {   // (the tables of a look-ahead are operands: nothing of it lies here)
    b.score = bp.take<float>(TB);
    b.finished = bp.take<int>(TB);
    if (beam) b.parent = bp.take<int>(TB);
    if (ruled) b.dead = bp.take<int>(TB);
    if (beam && mode.rule == Mode::SEQUENCE) b.open = bp.take<int>(TB);
    if (ruled) {   // (per step; under a beam the two halves)
      b.first = bp.take<int>(beam ? 2 * Btot : TB);
      b.prev = bp.take<int>(beam ? 2 * Btot : TB);
    }
    if (mode.pick == Mode::DRAW) b.row_id = bp.take<int>(Btot);
    if (ruled) {
      b.visited = bp.take<unsigned>(beam ? 2 * vw : vw);
      b.byte_rows = bp.take<unsigned char>(Btot * (size_t)S);
    }
  }
  if (out) *out = b;
  return bp.off;
}

// Workspace bytes of a decode in `mode` (every ff_decode*_workspace_bytes entry, behind its own argument check).
size_t decode_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host, const Mode& mode,
                              bool want_lp = false) {
  if (!m || !p || p->N <= 0 || p->F <= 0 || p->T <= 0) return 0;
  int btot = 0, max_bc = 0, nch = 0;
  plan_mode(p, num_input_host, 1, mode, nullptr, &btot, &max_bc, &nch);
  Bump bp(nullptr, 0);
  return layout_decode(m, p, engine_knobs(p), (size_t)btot, (size_t)max_bc, (size_t)nch, bp, nullptr, mode, want_lp) + 256;
}

// Does a decode step with R active rows take the LayerNorm-folded projections?  (decoder_pass and the engine loop ask.)
bool step_fuses(const ff_model* m, const ff_decode_params* prm, long R) {
  const int E = m->E;
  const bool x3_bound = split_bound(m, prm);
  const bool x3_folds = x3_bound && m->dec[0].ln1_planes != nullptr && m->dec[0].ln2_planes != nullptr &&
                        m->dec[0].ln3_planes != nullptr && E == 512;
  // f32 only: since round 4 the LDS-DMA kernel of the f32 family carries the folded forms at every size too (K = E = 512), so
  // the steps fold at every size as well (128 wireframes per call: 5 053 -> 301 LayerNorm launches, 206 -> 214 k selections/s).
  const int fuse_max = prm->ln_fuse_max_rows > 0 ? prm->ln_fuse_max_rows
                       : ((x3_folds || (!x3_bound && E == 512)) ? (1 << 30)
                          : (x3_bound && prm->x3_min_rows - 1 < 12288 ? prm->x3_min_rows - 1 : 12288));
  return can_fuse_layernorm(m, prm) && R <= fuse_max;
}

// One decoder pass over the current prefix (t positions) of one micro-batch, Bc sequences wide with Fc of them per wireframe
// (the chunk's own widths, or its live widths under FF_RETIRE_FINISHED).
// full_rows: evaluate every layer for all rows and project all rows into proj_all (ld = E rows
// position-major within the chunk); otherwise the result is p[Bc, E] for the newest position.
//
// With FF_FUSE_LAYERNORM only layer 0's norm1 is a standalone launch: every other LayerNorm input x is produced
// by a projection with a residual (out-proj, linear2), which leaves per-row segment statistics in `lnstat`; the
// projection that consumes LN(x) (+ qpos) reads x and the statistics and applies gamma / beta / qpos W^T through
// folded weights (ff_gemm_f32_ln).  19 -> 1 LayerNorm launches per decode step of a 6-layer decoder.
int decoder_pass(const ff_model* m, const ff_decode_params* prm, const EngineKnobs& kn, const DecodeBuffers& bufs, const Scratch& buf,
                 const Chunk& ck, int Fc, int Bc, const unsigned char* mask, const int* kv_len, int t, bool full_rows,
                 float* proj_all, hipStream_t st, float* logits_out = nullptr) {
  const int E = m->E, FFd = m->FF, H = m->H, S = prm->L + m->num_token, F = Fc, T = prm->T;
  const int R = t * Bc, nd = m->num_dec_layers;
  const size_t newoff = (size_t)(t - 1) * Bc;
  const bool reuse0 = (prm->flags & FF_REUSE_LAYER0_QKV) != 0 && ck.qkv0 != nullptr;
  const bool prune_last = (prm->flags & FF_LAST_LAYER_LAST_ROW) != 0 && !full_rows;
  // Folding the LayerNorms into the projections removes 18 launches per step.  On MI355X the normalising consumer costs about
  // what the standalone LayerNorm launch it replaces costs up to ~10^4 rows (round 3, once the position-table term of the
  // epilogue became ONE load per lane: config B 62.1-62.4 ms folded at every step vs 62.6 with the round-2 limit of 4096 rows);
  // above that the plain launches take the 128x64-tile kernel, which the fused forms do not have (config C / E micro-batches),
  // so the fused form is used up to ln_fuse_max_rows active rows (default 12288) -- both forms are parity-tested.
  // With the 3 x bf16 projections bound, the steps that take them (x3_min_rows on) launch the LayerNorms: the split kernel
  // has no folded form, and LayerNorm + split product beats the folded f32 forms there (config B 60.1 vs 61.9 ms).
  // Round 4: the 3 x bf16 kernel has the folded forms as well (ff_gemm_x3_ln).  With the planes of the folded weights bound the
  // steps fold at EVERY size (the large launches then take the split kernel, which has no 128x64-tile problem).
  const bool fuse = step_fuses(m, prm, R);
  const int nseg = E / 32;
  const float* qpos = m->qpos_table;
  const float* qpos_new = qpos + (size_t)(t - 1) * E;
  auto proj = [&](const Proj& d) -> int { return project(m, prm, Bc, st, d); };
  // The pruned last layer needs k | v of every row and q of the newest position only: two launches.  On launch-bound steps
  // (few rows) ONE q | k | v launch over all rows is cheaper than the second launch it saves (FF_LAST_QKV_ONE_LAUNCH_ROWS: up
  // to this many active rows; 0 = never); the q of the older rows is computed and not used.
  const bool last_qkv_one = R <= kn.one_launch_rows;
  for (int l = 0; l < nd; ++l) {
    const ff_layer_weights& w = m->dec[l];
    const ff_mha_weights& sa = w.self_attn;
    const bool last = prune_last && (l == nd - 1);
    const float* xin = (l == 0) ? ck.x0 : buf.x;
    const float* QKV = buf.qkv;
    bool fold_last = false;   // the pruned layer with k | v folded into the query: o is written by its own launches below
    // ---- self attention: q = k = LN1(x) + qpos, v = LN1(x), no mask (transformer.py:242-246) ----
    if (l == 0 && reuse0) {
      if (full_rows) {
        // (the pass behind the loop: every position < t went through a decode step, its layer-0 q|k|v is in the cache)
      } else if (fuse && t > 1 && ck.x0stat) {
        // the newest rows were appended by the previous step's pointer launch together with their segment statistics: the
        // folded projection normalises them itself (no LayerNorm launch left in a decode step after the first)
        FF_RETURN_IF(proj(Proj().in(xin + newoff * E, E).weight(w.ln1_w, E, w.ln1_b).norm(ck.x0stat)
                              .pos(w.ln1_pos + (size_t)(t - 1) * 2 * E, 2 * E, 2 * E).out(ck.qkv0 + newoff * 3 * E, 3 * E, Bc, 3 * E, E)));
      } else {
        FF_RETURN_IF(ff_layernorm(xin + newoff * E, E, w.norm1_w, w.norm1_b, m->ln_eps, buf.y, E, buf.yq, E,
                                  qpos_new, E, Bc, 1, Bc, E, st));
        FF_RETURN_IF(proj(Proj().in(buf.yq, E, buf.y, 2 * E).weight(sa.in_proj_w, E, sa.in_proj_b)
                              .out(ck.qkv0 + newoff * 3 * E, 3 * E, Bc, 3 * E, E)));
      }
      QKV = ck.qkv0;
    } else if (fuse && l > 0) {
      // Third form of the pruned layer, from FF_LAST_FOLD_MIN_ROWS active rows on: k | v of the prefix rows are
      // not projected at all.  q of the newest rows as in the two-launch form (the same launch: q keeps its bits); qt | c =
      // q_h [W'k_h | kb_h] (head-batched, K = 64); ONE pass over the prefix rows and their statistics leaves u_h = sum_j p_j x^_j;
      // o_h = u_h W'v_h^T (head-batched) into the o rows the out-projection reads -- its bias is then the table's ob, which
      // carries b'v.  qt | c and u lie in the feed-forward scratch h, dead until this layer's linear1.
      const size_t qt_floats = ff_align_up((size_t)Bc * H * (E + t), 4);
      fold_last = last && t > 1 && bufs.fold_kt && R >= kn.last_fold_rows && !step_splits(m, prm, R) &&
                  qt_floats + (size_t)Bc * H * E <= (size_t)(T - 1 > 0 ? T - 1 : 1) * Bc * FFd;
      // the LayerNorm-folded projection over all R rows that opens layer l > 0: q|k|v, or k|v alone (weight rows and output
      // columns from c0 = E on) when the layer is pruned to its newest position; its q then covers the last Bc rows only
      const bool kv_only = last && t > 1 && !last_qkv_one;
      const int c0 = kv_only ? E : 0;
      if (!fold_last)
        FF_RETURN_IF(proj(Proj().in(buf.x, E).weight(w.ln1_w + (size_t)c0 * E, E, w.ln1_b + c0).split(w.ln1_planes, 3 * E, c0, w.ln1_csum)
                              .norm(buf.lnstat).pos(w.ln1_pos + c0, 2 * E, 2 * E - c0).out(buf.qkv + c0, 3 * E, R, 3 * E - c0, E)));
      if (kv_only || fold_last)
        FF_RETURN_IF(proj(Proj().in(xin + newoff * E, E).weight(w.ln1_w, E, w.ln1_b).norm(buf.lnstat + newoff * nseg * 2)
                              .pos(w.ln1_pos + (size_t)(t - 1) * 2 * E, 2 * E, E).out(buf.qkv + newoff * 3 * E, 3 * E, Bc, E, E)));
      if (fold_last) {
        float* qt = buf.h;
        float* u = buf.h + qt_floats;
        FF_RETURN_IF(ff_gemm_f32_batched(buf.qkv + newoff * 3 * E, 3 * E, nullptr, 0, bufs.fold_kt, FF_HEAD_DIM, nullptr, nullptr, 0,
                                         qt, H * (E + t), Bc, E + t, FF_HEAD_DIM, 0, 0, H, FF_HEAD_DIM,
                                         (long long)(E + T) * FF_HEAD_DIM, E + t, st));
        FF_RETURN_IF(ff_attention_prefix_fold(buf.x, buf.lnstat, m->ln_eps, qt, 0.125f, Bc, t, E, H, u, st));
        FF_RETURN_IF(ff_gemm_f32_batched(u, H * E, nullptr, 0, w.ln1_w + (size_t)2 * E * E, E, nullptr, nullptr, 0,
                                         buf.o + newoff * E, E, Bc, FF_HEAD_DIM, E, 0, 0, H, E, (long long)FF_HEAD_DIM * E,
                                         FF_HEAD_DIM, st));
      }
    } else {
      FF_RETURN_IF(ff_layernorm(xin, E, w.norm1_w, w.norm1_b, m->ln_eps, buf.y, E, buf.yq, E, qpos, E, Bc, T, R, E, st));
      // Not step_splits(): this picks the launch FORM, not the kernel.  From x3_min_rows rows on (no per-width factor, no
      // shape conditions) the pruned layer keeps ONE q|k|v launch, which project() then routes by its own rule; the planes
      // cover the whole [3E, E] weight (no row ranges), so the two-launch form below never takes the split kernel.
      const bool x3_here = w.in_proj_planes && prm->x3_min_rows > 0 && R >= (long)prm->x3_min_rows;
      if (last && t > 1 && !x3_here && (E % 64) == 0) {
        // pruned last layer: k (from LN(x)+qpos) | v (from LN(x)) for every row, q for the newest position only
        FF_RETURN_IF(proj(Proj().in(buf.yq, E, buf.y, E).weight(sa.in_proj_w + (size_t)E * E, E, sa.in_proj_b + E)
                              .out(buf.qkv + E, 3 * E, R, 2 * E, E)));
        FF_RETURN_IF(proj(Proj().in(buf.yq + newoff * E, E).weight(sa.in_proj_w, E, sa.in_proj_b)
                              .out(buf.qkv + newoff * 3 * E, 3 * E, Bc, E, E)));
      } else {
        FF_RETURN_IF(proj(Proj().in(buf.yq, E, buf.y, 2 * E).weight(sa.in_proj_w, E, sa.in_proj_b).split(w.in_proj_planes, 3 * E)
                              .out(buf.qkv, 3 * E, R, 3 * E, E)));
      }
    }
    // rows that continue through the rest of this layer
    const size_t roff = last ? newoff : 0;
    const int Rl = last ? Bc : R;
    float* x = buf.x + roff * E;      // the layer's running rows, their attention output and FFN hidden rows
    float* o = buf.o + roff * E;
    float* h = buf.h + roff * FFd;
    float* qc = buf.qkv + roff * E;   // cross-attention q: a [rows, E] view of the q|k|v scratch
    // folded steps: every projection with a residual leaves the statistics of its rows, the next projection normalises with them
    float* stat = fuse ? buf.lnstat + roff * nseg * 2 : nullptr;
    if (!fold_last) {
      ff_attn_desc d;
      memset(&d, 0, sizeof(d));
      d.q = QKV + roff * 3 * E; d.k = QKV + E; d.v = QKV + 2 * E; d.o = o;
      d.ldq = d.ldk = d.ldv = 3 * E; d.ldo = E;
      d.num_groups = Bc; d.num_heads = H; d.scale = 0.125f;
      d.nq = last ? 1 : t; d.q_group_stride = 1; d.q_inner = 1; d.q_outer_stride = Bc;
      d.nk = t; d.k_group_stride = 1; d.k_stride = Bc;
      FF_RETURN_IF(ff_attention(&d, st));
    }
    FF_RETURN_IF(proj(Proj().in(o, E).weight(sa.out_w, E, fold_last ? bufs.fold_ob : sa.out_b).split(w.self_out_planes, E).add(xin + roff * E, E)
                          .out(x, E, Rl, E, E).stats(stat)));
    // ---- cross attention: q = LN2(x) + qpos, k = memory + pos, v = memory (transformer.py:247-252);
    //      K/V come from the per-batch cache ----
    if (fuse) {
      FF_RETURN_IF(proj(Proj().in(x, E).weight(w.ln2_w, E, w.ln2_b).split(w.ln2_planes, E, 0, w.ln2_csum).norm(stat)
                            .pos(w.ln2_pos + (last ? (size_t)(t - 1) * E : 0), E, E).out(qc, E, Rl, E, E)));
    } else {
      if (last)
        FF_RETURN_IF(ff_layernorm(x, E, w.norm2_w, w.norm2_b, m->ln_eps, nullptr, 0, buf.yq + roff * E, E, qpos_new, E, Bc, 1, Rl, E, st));
      else
        FF_RETURN_IF(ff_layernorm(buf.x, E, w.norm2_w, w.norm2_b, m->ln_eps, nullptr, 0, buf.yq, E, qpos, E, Bc, T, Rl, E, st));
      FF_RETURN_IF(proj(Proj().in(buf.yq + roff * E, E).weight(w.cross_attn.in_proj_w, E, w.cross_attn.in_proj_b)
                            .split(w.cross_q_planes, E).out(qc, E, Rl, E, E)));
    }
    {
      ff_attn_desc d;
      memset(&d, 0, sizeof(d));
      d.q = qc; d.k = bufs.kvc[l] + (size_t)ck.w0 * S * 2 * E; d.v = d.k + E; d.o = o;
      d.ldq = d.ldo = E; d.ldk = d.ldv = 2 * E;
      d.num_groups = ck.nw; d.num_heads = H; d.scale = 0.125f;
      d.nq = last ? F : F * t; d.q_group_stride = F; d.q_inner = F; d.q_outer_stride = Bc;
      d.nk = S; d.k_group_stride = S; d.k_stride = 1;
      d.kv_len = kv_len + ck.w0; d.key_mask = mask + (size_t)ck.w0 * S; d.mask_stride = S;
      // (layout_decode makes kvp[l] only with the split products bound: step_splits() asks no more here than the row rule)
      if (bufs.kvp[l] && step_splits(m, prm, R))
        d.kv_planes = bufs.kvp[l] + (size_t)ck.w0 * H * (ff_attention_planes_bytes(1, H) / H);
      d.kv_terms = m->split_kind == 2 ? 1 : 0;
      FF_RETURN_IF(ff_attention(&d, st));
    }
    FF_RETURN_IF(proj(Proj().in(o, E).weight(w.cross_attn.out_w, E, w.cross_attn.out_b).split(w.cross_out_planes, E).add(x, E)
                          .out(x, E, Rl, E, E).stats(stat)));
    // ---- feed forward (transformer.py:253-255) ----
    if (fuse) {
      FF_RETURN_IF(proj(Proj().in(x, E).weight(w.ln3_w, E, w.ln3_b).split(w.ln3_planes, FFd, 0, w.ln3_csum).norm(stat)
                            .out(h, FFd, Rl, FFd, E, 1)));
    } else {
      FF_RETURN_IF(ff_layernorm(x, E, w.norm3_w, w.norm3_b, m->ln_eps, buf.y + roff * E, E, nullptr, 0, nullptr, 0, 1, 1, Rl, E, st));
      FF_RETURN_IF(proj(Proj().in(buf.y + roff * E, E).weight(w.lin1_w, E, w.lin1_b).split(w.lin1_planes, FFd)
                            .out(h, FFd, Rl, FFd, E, 1)));
    }
    FF_RETURN_IF(proj(Proj().in(h, FFd).weight(w.lin2_w, FFd, w.lin2_b).split(w.lin2_planes, E).add(x, E)
                          .out(x, E, Rl, E, FFd).stats(stat)));
  }
  // ---- decoder.norm + project (transformer.py:115-116, model_para.py:225): every row, or the newest position's ----
  const size_t hoff = full_rows ? 0 : newoff;
  const int Rh = full_rows ? R : Bc;
  float* dst = full_rows ? proj_all : buf.p;
  if (!fuse) {
    FF_RETURN_IF(ff_layernorm(buf.x + hoff * E, E, m->dec_norm_w, m->dec_norm_b, m->ln_eps, buf.y, E, nullptr, 0, nullptr, 0,
                              1, 1, Rh, E, st));
    return proj(Proj().in(buf.y, E).weight(m->proj_w, E, m->proj_b).out(dst, E, Rh, E, E));
  }
  Proj d = Proj().in(buf.x + hoff * E, E).norm(buf.lnstat + hoff * nseg * 2);
  if (!full_rows && logits_out && ck.pg)
    // pointer_fold: logits = <project(LN(x)), memory_s> = LN(x) (memory W')^T + memory b' -- ONE launch for decoder.norm,
    // project and the pointer's dot products of a one-wireframe micro-batch (G and c are made once per call)
    return proj(d.weight(ck.pg, E, ck.pc).out(logits_out, S, Bc, S, E));
  return proj(d.weight(m->proj_fold_w, E, m->proj_fold_b).out(dst, E, Rh, E, E));
}

// Internal side streams + fork/join events: one pool per device, created on first use.
// host-mapped ints: one per (step, micro-batch) of a decode; a decode with more of them checks its stop rule by draining the
// streams and copying (FF_PINNED_COUNTERS overrides the size: tests run that path with a handful of slots)
// (knob FF_PINNED_COUNTERS: how many of them a decode may use)
struct StreamPool {
  hipStream_t side[FF_MAX_STREAMS];
  hipEvent_t fork_ev, join_ev[FF_MAX_STREAMS];
  hipEvent_t chk_ev[FF_MAX_STREAMS];      // stop-rule check: per-stream progress marks
  int* hpin;                                // host-mapped pinned counters [step][micro-batch], written by the pointer launches
  int* hpin_dev;                            // ... the device-visible address of the same memory
  int* stage;                               // FF_RETIRE_FINISHED: pinned staging of the slot-map uploads (grown on demand)
  size_t stage_cap;
  int created;
  bool events;
};
StreamPool g_pools[FF_MAX_DEVICES];
std::mutex g_pool_mu;
// The pool's side streams, events and pinned counters belong to ONE decode at a time: host threads that
// decode on the same device take turns (different devices run concurrently).
std::mutex g_pool_busy[FF_MAX_DEVICES];

int pool_get(int n, StreamPool** out) {
  int dev = 0;
  FF_CHECK_HIP(hipGetDevice(&dev));
  FF_CHECK_ARG(dev >= 0 && dev < FF_MAX_DEVICES, "device index %d out of range", dev);
  std::lock_guard<std::mutex> lock(g_pool_mu);
  StreamPool& pool = g_pools[dev];
  if (!pool.events) {
    FF_CHECK_HIP(hipEventCreateWithFlags(&pool.fork_ev, hipEventDisableTiming));
    for (int i = 0; i < FF_MAX_STREAMS; ++i) {
      FF_CHECK_HIP(hipEventCreateWithFlags(&pool.join_ev[i], hipEventDisableTiming));
      FF_CHECK_HIP(hipEventCreateWithFlags(&pool.chk_ev[i], hipEventDisableTiming));
    }
    // coherent (fine-grained) host memory mapped into the device's address space: the pointer launches store their stop-rule
    // counters straight into it (system-scope stores; no copy launch between two decode steps)
    FF_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&pool.hpin), sizeof(int) * FF_PINNED_SLOTS,
                               hipHostMallocMapped | hipHostMallocCoherent));
    FF_CHECK_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&pool.hpin_dev), pool.hpin, 0));
    pool.events = true;
  }
  while (pool.created < n) {
    FF_CHECK_HIP(hipStreamCreateWithFlags(&pool.side[pool.created], hipStreamNonBlocking));
    FF_RETURN_IF(ff_gemm_prepare_stream(pool.side[pool.created]));
    pool.created++;
  }
  *out = &pool;
  return FF_OK;
}

std::mutex* pool_busy_mutex() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= FF_MAX_DEVICES) return nullptr;
  return &g_pool_busy[dev];
}

// What the caller hands to ff_decode besides the model, the parameters and the workspace.
struct DecodeIO {
  const float* memory; const unsigned char* mask; const int *kv_len, *num_input, *num_input_host; const unsigned char* extra_mask;
  int64_t* predict; int *steps_done, *step_counts; float *pointer_out, *trace_logits, *trace_best, *trace_second; int* seq_of_row;
  hipStream_t main_st;
  float* logprob;   // [N*F, T] like predict, or null (ff_decode)
};

// FF_RETIRE_FINISHED slot order of a chunk of nw wireframes with `width` entries each, entry i live or finished: per wireframe
// the live entries in order, then finished ones of the same wireframe, up to the chunk's widest live count (returned: every
// wireframe of a chunk keeps the same number of slots).  Appends the entries' indices to `out`, the live count to *nlive.
int ordered_slots(const std::vector<char>& live, int nw, int width, std::vector<int>* out, long* nlive = nullptr) {
  int fl = 0;
  for (int wl = 0; wl < nw; ++wl) {
    int n = 0;
    for (int k = 0; k < width; ++k) n += live[(size_t)wl * width + k] ? 1 : 0;
    fl = n > fl ? n : fl;
    if (nlive) *nlive += n;
  }
  for (int wl = 0; wl < nw; ++wl) {
    int taken = 0;
    for (int want = 1; want >= 0; --want)
      for (int k = 0; k < width && taken < fl; ++k)
        if ((live[(size_t)wl * width + k] ? 1 : 0) == want) { out->push_back(wl * width + k); ++taken; }
  }
  return fl;
}

// One ff_decode call: the state its phases share, and the phases in the order ff_decode calls them.
struct DecodeRun {
  const ff_model* m = nullptr;
  ff_decode_params prm;                       // the caller's parameters; `p` points here
  const ff_decode_params* p = nullptr;
  DecodeIO io;
  EngineKnobs kn;
  int E = 0, S = 0, T = 0, F = 0, N = 0, Btot = 0, nch = 0, ns = 1;
  bool retire = false, dedup = false, forked = false, each_eos = false;
  bool lagged = false;                        // the stop counters fit the host-mapped slots: checked without draining the queue
  std::vector<Chunk> chunks;
  DecodeBuffers buf;
  hipStream_t sts[FF_MAX_STREAMS];
  StreamPool* pool = nullptr;
  int enq = 0, pending_enq = 0;               // steps enqueued so far; > 0: events covering steps [0, pending_enq) are in flight
  bool stopped = false;
  std::vector<int> slots_per_step, tot;
  std::vector<int> hfin;                      // host copy of the finish positions (pageable; filled from fin_host at check points)
  std::vector<std::vector<int>> hslot;        // per chunk: the chunk-local sequence of every slot
  int* fin_host = nullptr;                    // host address of the finish positions when they are host-mapped, else null
  int* fin_dev = nullptr;
  Mode mode;                                  // greedy (ff_decode / ff_decode_lp) or the opt-in decode of the entry
  std::vector<int> chunk_steps;               // forced: steps every micro-batch runs: the largest length among its rows
  int forced_steps = 0;                       // ... and the largest of those
  int validate(const ff_model* m_, const ff_decode_params* p_, const DecodeIO& io_, const void* workspace) {
    m = m_; io = io_;
    const bool forced = mode.pick == Mode::FORCED;
    FF_RETURN_IF(check_model(m));
    FF_CHECK_ARG(p_ != nullptr, "ff_decode: null params");
    FF_CHECK_ARG(p_->variant == FF_PARALLEL || p_->variant == FF_SEQ2SEQ, "ff_decode: bad variant");
    FF_CHECK_ARG(p_->N > 0 && p_->L >= 0 && p_->F > 0 && p_->T >= 1, "ff_decode: bad sizes");
    FF_CHECK_ARG(io.memory && io.mask && io.kv_len && (io.predict || forced) && workspace, "ff_decode: null pointer");
    FF_CHECK_ARG(p_->variant != FF_PARALLEL || io.num_input || forced, "ff_decode: num_input required for the parallel variant");
    FF_CHECK_ARG(p_->variant != FF_SEQ2SEQ || p_->F == 1, "ff_decode: seq2seq decodes one sequence per wireframe");
    FF_CHECK_ARG(!p_->stop_fn || (p_->flags & FF_NO_STOP) || p_->sync_every > 0, "ff_decode: stop_fn needs sync_every > 0");
    // The callback's cadence is a CONTRACT with callers that replay it elsewhere (an idle rank of a sharded decode joins the
    // same host collectives: faceformer_amd/dist.py check_points): the counters of the first n = enq - sync_every steps when
    // enq = 2 sync_every, 3 sync_every, ... steps are enqueued.  Both check paths of check_point() (host-mapped counters; drain +
    // copy when there are more counters than slots) keep that cadence for a stop_fn (tests: FF_PINNED_COUNTERS=8 in a child process).
    FF_CHECK_ARG(!(p_->flags & FF_STOP_EACH_EOS) || p_->variant == FF_SEQ2SEQ, "ff_decode: FF_STOP_EACH_EOS is a seq2seq rule");
    E = m->E; S = p_->L + m->num_token; T = p_->T; F = p_->F; N = p_->N;
    FF_CHECK_ARG(S <= m->pos_len, "ff_decode: S=%d exceeds the position table (%d rows)", S, m->pos_len);
    FF_CHECK_ARG(T - 1 <= m->qpos_len, "ff_decode: T-1=%d exceeds the query position table (%d rows)", T - 1, m->qpos_len);
    FF_CHECK_ARG(p_->variant != FF_PARALLEL || F <= S || forced, "ff_decode: F=%d anchors exceed S=%d", F, S);   // (forced rows are no anchors)
    FF_CHECK_ARG(!(p_->flags & FF_RETURN_POINTER) || io.pointer_out, "ff_decode: pointer_out required");
    if (p_->flags & FF_RETIRE_FINISHED) {
      FF_CHECK_ARG(p_->variant == FF_PARALLEL, "ff_decode: FF_RETIRE_FINISHED is a parallel-variant option");
      FF_CHECK_ARG(!(p_->flags & (FF_RETURN_POINTER | FF_NO_STOP)) && !p_->stop_fn,
                   "ff_decode: FF_RETIRE_FINISHED excludes FF_RETURN_POINTER, FF_NO_STOP and a stop_fn");
      FF_CHECK_ARG(io.num_input_host, "ff_decode: FF_RETIRE_FINISHED needs num_input_host");
      FF_CHECK_ARG(p_->term_lo < p_->term_hi, "ff_decode: empty terminator range [%d, %d)", p_->term_lo, p_->term_hi);
    }
    // every padding-anchor sequence has its own row of an extra mask: no de-duplication then
    prm = *p_;
    if (io.extra_mask || forced) prm.flags &= ~FF_DEDUP_PAD_ANCHORS;   // (forced: the rows are arbitrary paths)
    p = &prm;
    retire = retiring(p);
    dedup = p->variant == FF_PARALLEL && (p->flags & FF_DEDUP_PAD_ANCHORS) && io.num_input_host;
    each_eos = (p->flags & FF_STOP_EACH_EOS) != 0;
    kn = engine_knobs(p);
    return FF_OK;
  }
  // Micro-batch plan, workspace layout and every chunk's views into it.
  int bind_chunks(void* workspace, size_t workspace_bytes) {
    const int ns_req = plan_streams(p);
    int max_bc = 0;
    plan_mode(p, io.num_input_host, ns_req, mode, &chunks, &Btot, &max_bc);
    nch = (int)chunks.size();
    Bump bp(workspace, workspace_bytes);
    layout_decode(m, p, kn, (size_t)Btot, (size_t)max_bc, (size_t)nch, bp, &buf, mode, io.logprob != nullptr);
    if (!bp.ok) { ff_set_error("ff_decode: workspace too small (%zu needed, %zu given)", bp.off, workspace_bytes); return FF_ERR_WORKSPACE; }
    for (Chunk& c : chunks) {
      c.x0 = buf.x0_all + (size_t)T * c.b0 * E;
      c.qkv0 = buf.qkv0_all ? buf.qkv0_all + (size_t)T * c.b0 * 3 * E : nullptr;
      c.x0stat = buf.x0stat_all ? buf.x0stat_all + (size_t)c.b0 * (E / 32) * 2 : nullptr;
      const size_t ci = (size_t)(&c - chunks.data());
      const bool one = c.nw == 1 && buf.pg_all != nullptr;
      c.pg = one ? buf.pg_all + ci * (size_t)S * E : nullptr;
      c.pc = one ? buf.pc_all + ci * (size_t)((S + 3) & ~3) : nullptr;
      if (retire) { c.slot = buf.slot_all + c.b0; c.perm = buf.perm_all + c.b0; }
    }
    ns = ns_req < nch ? ns_req : nch;
    forked = ns > 1;
    lagged = (size_t)T * (size_t)nch <= (size_t)kn.pinned;
    fin_dev = buf.fin;
    slots_per_step.reserve((size_t)T);   // (the loop below allocates nothing per step)
    tot.reserve((size_t)T);
    if (mode.pick == Mode::FORCED) {   // (the plan has no de-duplication: sequence b0 + i of a chunk is row b0 + i of the paths)
      for (const Chunk& c : chunks) {
        int mx = 0;
        for (int i = 0; i < c.Bc; ++i) mx = mode.forced->lengths_host[c.b0 + i] > mx ? mode.forced->lengths_host[c.b0 + i] : mx;
        chunk_steps.push_back(mx);
        forced_steps = mx > forced_steps ? mx : forced_steps;
      }
    }
    return FF_OK;
  }
  // With more than one stream ALL micro-batch work runs on the internal pool (the caller's stream is
  // often the legacy default stream, whose implicit synchronisation would serialise the others).
  int bind_streams() {
    FF_RETURN_IF(pool_get(forked ? ns : 0, &pool));   // (also owns the pinned counter buffer / events of the stop check)
    sts[0] = io.main_st;
    if (forked)
      for (int s = 0; s < ns; ++s) sts[s] = pool->side[s];
    return FF_OK;
  }
  // ---- FF_RETIRE_FINISHED: the initial slot sets (host side) -------------------------------------------------------------------
  // fin[seq] = 0 for the sequences whose start token already ends them (the padding anchors and anchors term_lo.. of the model:
  // reference quirk C-3) and for the surplus padding copies of narrow wireframes; T (none yet) for the others.  Every chunk starts
  // with its live sequences only: per wireframe the live ones in order, then finished ones of the same wireframe up to the
  // chunk's widest live count.
  int init_retirement() {
    if (!retire) return FF_OK;
    const size_t ncnt = (size_t)T * nch;
    if (lagged && ncnt + (size_t)Btot <= (size_t)kn.pinned) {
      fin_host = pool->hpin + ncnt;
      fin_dev = pool->hpin_dev + ncnt;
    }
    if (pool->stage_cap < 2 * (size_t)Btot) {   // (no upload of an earlier decode is in flight: it synchronised before returning)
      if (pool->stage) FF_CHECK_HIP(hipHostFree(pool->stage));
      pool->stage = nullptr; pool->stage_cap = 0;
      FF_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&pool->stage), sizeof(int) * 2 * (size_t)Btot, hipHostMallocDefault));
      pool->stage_cap = 2 * (size_t)Btot;
    }
    hfin.assign((size_t)Btot, T);
    hslot.resize(chunks.size());
    for (Chunk& c : chunks) {
      std::vector<char> live((size_t)c.Bc);
      for (int wl = 0; wl < c.nw; ++wl) {
        const int w = c.w0 + wl, n = io.num_input_host[w], cw = compact_width(p, io.num_input_host, w);
        for (int f = 0; f < c.Fc; ++f) {
          const int fc = c.f0 + f, k = wl * c.Fc + f;
          const int start = fc < n ? fc : m->num_token - 1;
          live[(size_t)k] = !(fc >= cw || (start >= p->term_lo && start < p->term_hi));
          if (!live[(size_t)k]) hfin[(size_t)c.b0 + k] = 0;
        }
      }
      c.Fl = ordered_slots(live, c.nw, c.Fc, &hslot[(size_t)(&c - chunks.data())]);
      c.Bl = c.nw * c.Fl;
    }
    if (lagged) memset(pool->hpin, 0, sizeof(int) * ncnt);   // (counters of launches a finished chunk never makes)
    if (fin_host) memcpy(fin_host, hfin.data(), sizeof(int) * (size_t)Btot);
    return FF_OK;
  }
  int sync_all() { for (int s = 0; s < ns; ++s) FF_CHECK_HIP(hipStreamSynchronize(sts[s])); return FF_OK; }
  // prologue(), greedy_loop() and epilogue() queue kernels that use the caller's workspace.  When one of them fails, ff_decode
  // drains every stream before it returns the error: the caller frees the workspace next.
  void drain() {
    for (int s = 0; s < ns; ++s) (void)hipStreamSynchronize(sts[s]);
    (void)hipStreamSynchronize(io.main_st);
  }
  // the side streams continue behind what the main stream holds now
  int fork() {
    if (!forked) return FF_OK;
    FF_CHECK_HIP(hipEventRecord(pool->fork_ev, io.main_st));
    for (int s = 0; s < ns; ++s) FF_CHECK_HIP(hipStreamWaitEvent(sts[s], pool->fork_ev, 0));
    return FF_OK;
  }
  // n ints of device memory on the host, behind everything enqueued so far (drained: the streams are idle already)
  int read_back(int* dst, const int* src, size_t n, bool drained = false) {
    if (!drained) FF_RETURN_IF(sync_all());
    FF_CHECK_HIP(hipMemcpyAsync(dst, src, sizeof(int) * n, hipMemcpyDeviceToHost, io.main_st));
    FF_CHECK_HIP(hipStreamSynchronize(io.main_st));
    return FF_OK;
  }
  // ---- per-batch invariants (main stream), then the first decoder input rows of every micro-batch ----
  int prologue() {
    const float* memory = io.memory;
    const hipStream_t main_st = io.main_st;
    const int RS = N * S;
    // memory + pos, cross-attention K|V of every layer
    FF_RETURN_IF(ff_add_pos(memory, E, m->pos_table, E, 1, S, buf.mem_pos, E, RS, E, main_st));
    for (int l = 0; l < m->num_dec_layers; ++l) {
      const ff_mha_weights& c = m->dec[l].cross_attn;
      FF_RETURN_IF(gemm(buf.mem_pos, E, memory, E, c.in_proj_w + (size_t)E * E, E, c.in_proj_b + E, nullptr, 0,
                        buf.kvc[l], 2 * E, RS, 2 * E, E, 0, main_st));
      if (buf.kvp[l])
        FF_RETURN_IF(ff_attention_split_kv(buf.kvc[l], buf.kvc[l] + E, 2 * E, 2 * E, N, m->H, S, S, 1, buf.kvp[l], main_st));
    }
    FF_CHECK_HIP(hipMemsetAsync(buf.zeroed, 0, sizeof(int) * buf.zeroed_count, main_st));
    if (retire) {   // initial slot maps (and finish positions when they live in the workspace), from the pinned staging area
      int *st_slot = pool->stage, *st_fin = pool->stage + Btot;
      for (const Chunk& c : chunks) {
        const std::vector<int>& hs = hslot[(size_t)(&c - chunks.data())];
        if (!hs.empty()) memcpy(st_slot + c.b0, hs.data(), sizeof(int) * hs.size());
      }
      FF_CHECK_HIP(hipMemcpyAsync(buf.slot_all, st_slot, sizeof(int) * (size_t)Btot, hipMemcpyHostToDevice, main_st));
      if (!fin_host) {
        memcpy(st_fin, hfin.data(), sizeof(int) * (size_t)Btot);
        FF_CHECK_HIP(hipMemcpyAsync(buf.fin, st_fin, sizeof(int) * (size_t)Btot, hipMemcpyHostToDevice, main_st));
      }
    }
    if (buf.fold_kt) {   // the folded last layer's tables (weights only)
      const ff_layer_weights& w = m->dec[m->num_dec_layers - 1];
      FF_RETURN_IF(ff_attention_fold_tables(w.ln1_w, w.ln1_b, w.ln1_pos, m->qpos_len, w.self_attn.out_w, w.self_attn.out_b, E, m->H, T,
                                            buf.fold_kt, buf.fold_ob, main_st));
    }
    FF_RETURN_IF(fork());
    // pointer_fold operands of the one-wireframe micro-batches: G = memory_w W' ([S, E]; W' = the folded project weight, used
    // transposed), c = memory_w b'
    bool any_pg = false;
    for (const Chunk& c : chunks) any_pg = any_pg || c.pg != nullptr;
    if (any_pg) {
      FF_RETURN_IF(ff_transpose(m->proj_fold_w, E, E, E, buf.projT, E, main_st));
      FF_RETURN_IF(fork());
      for (const Chunk& c : chunks) {
        if (!c.pg) continue;
        const float* mem_w = memory + (size_t)c.w0 * S * E;
        FF_RETURN_IF(gemm(mem_w, E, nullptr, 0, buf.projT, E, nullptr, nullptr, 0, c.pg, E, S, E, E, 0, sts[c.sid]));
        FF_RETURN_IF(gemm(mem_w, E, nullptr, 0, m->proj_fold_b, E, nullptr, nullptr, 0, c.pc, 1, S, 1, E, 0, sts[c.sid]));
      }
    }
    // start tokens (anchors / SOS) and first decoder input rows of every micro-batch
    for (const Chunk& c : chunks) {
      if (mode.pick != Mode::POINTER) {
        FF_RETURN_IF(init_state(c));
        FF_RETURN_IF(ff_gather_rows(memory + (size_t)c.w0 * S * E, S, E, buf.tok_all + c.b0, c.Bc, c.Fc, c.x0, E, sts[c.sid]));
        continue;
      }
      // (retirement: the start tokens of the slots go to the chunk's perm area, free until its first compaction)
      hipLaunchKernelGGL(init_tokens_kernel, dim3(ff_cdiv(c.Bc, 256)), dim3(256), 0, sts[c.sid], buf.tok_all + c.b0,
                         c.Bc, c.Fc, c.f0, io.num_input ? io.num_input + c.w0 : nullptr, p->variant, m->num_token - 1,
                         p->tok_sos, c.slot, c.perm, c.slot ? c.Bl : 0);
      FF_CHECK_LAUNCH();
      if (c.Bl > 0)
        FF_RETURN_IF(ff_gather_rows(memory + (size_t)c.w0 * S * E, S, E, c.slot ? c.perm : buf.tok_all + c.b0, c.Bl, c.Fl, c.x0, E,
                                    sts[c.sid]));
    }
    return FF_OK;
  }
  // The rule's operands of one micro-batch: the flags, the chunk's part of the follow table and the words per row of it (= per
  // sequence of `visited`).
  struct Rule { const unsigned* follows; int L, fw, flags; };
  Rule rule_of(const Chunk& c) const {
    const int L = p->L, fw = (L + 31) / 32;
    return Rule{mode.follows ? mode.follows + (size_t)c.w0 * L * fw : nullptr, L, fw, mode.flags};
  }
  // Row 0 of the mode's per-step records and of the token array for one micro-batch: the start state of its sequences.  The
  // parallel entries start at the anchors (Fc / G of them per wireframe); the sequence entries have Fc = G rows per wireframe,
  // every one at SOS, the rule's state empty and closed.  Under a beam the rule's state is half 0 of the ping-pong: step 0 reads it.
  int init_state(const Chunk& c) {
    const int G = mode.G, pad_tok = m->num_token - 1;
    const int* ni = io.num_input ? io.num_input + c.w0 : nullptr;
    hipStream_t st = sts[c.sid];
    if (mode.pick == Mode::FORCED) return FF_OK;   // (the start tokens are row 0 of the token array, forced_tokens() put the paths there)
    const bool beam = mode.pick == Mode::BEAM, draw = mode.pick == Mode::DRAW, seq = mode.sequence;
    int* tok = buf.tok_all + c.b0;
    float* score = buf.score + c.b0;
    int* fin = buf.finished + c.b0;
    if (mode.rule == Mode::NONE) {
      if (beam)
        return seq ? ff_sequence_beam_init(tok, score, fin, buf.parent + c.b0, c.Bc, G, p->tok_sos, st)
                   : ff_beam_init(tok, score, fin, buf.parent + c.b0, c.Bc, c.Fc / G, G, c.f0, ni, pad_tok, p->term_lo, p->term_hi, st);
      return seq ? ff_sequence_sample_init(tok, score, fin, buf.row_id + c.b0, c.Bc, G, c.w0, p->tok_sos, st)
                 : ff_sample_init(tok, score, fin, buf.row_id + c.b0, c.Bc, c.Fc / G, G, c.f0, c.w0, F, ni, pad_tok, p->term_lo, p->term_hi, st);
    }
    const Rule r = rule_of(c);
    int *dead = buf.dead + c.b0, *first = buf.first + c.b0, *prev = buf.prev + c.b0;
    unsigned* visited = buf.visited + (size_t)c.b0 * r.fw;
    if (seq) {
      if (beam)
        return ff_sequence_constrain_beam_init(tok, score, fin, dead, buf.open + c.b0, buf.parent + c.b0, first, prev, visited, c.Bc, G, p->L,
                                               p->tok_sos, st);
      if (draw)
        return ff_sequence_constrain_sample_init(tok, score, fin, dead, first, prev, visited, buf.row_id + c.b0, c.Bc, G, c.w0, p->L,
                                                 p->tok_sos, st);
      return ff_sequence_constrain_init(tok, score, fin, dead, first, prev, visited, c.Bc, p->L, p->tok_sos, st);
    }
    if (beam)
      return ff_constrain_beam_init(tok, score, fin, dead, buf.parent + c.b0, first, prev, visited, c.Bc, c.Fc / G, G, c.f0, ni, pad_tok,
                                    p->term_lo, p->term_hi, m->num_token, r.follows, r.L, st);
    if (draw)
      return ff_constrain_sample_init(tok, score, fin, dead, first, prev, visited, buf.row_id + c.b0, c.Bc, c.Fc / G, G, c.f0, c.w0, F,
                                      ni, pad_tok, p->term_lo, p->term_hi, m->num_token, r.follows, r.L, st);
    return ff_constrain_init(tok, score, fin, dead, first, prev, visited, c.Bc, c.Fc, c.f0, ni, pad_tok, p->term_lo, p->term_hi,
                             m->num_token, r.follows, r.L, st);
  }
  // Decode step `step` (position t = step + 1) of every micro-batch that has slots left, on the chunk's stream: the slot set
  // decoded now is Fl / Bl wide (the chunk's Fc / Bc without retirement).
  int enqueue_step(int step) {
    const int t = step + 1;
    int nslots = 0;
    for (const Chunk& c : chunks) {
      if (c.Bl == 0) continue;   // (retirement: nothing of this micro-batch is left)
      nslots += c.Bl;
      hipStream_t st = sts[c.sid];
      const Scratch& sc = buf.scr[c.sid];
      const size_t trow = (size_t)step * ((size_t)N * F * mode.G) + c.b0;  // traces: step stride N*F (N*F*W with beams, N*F*R with samples; caller sizes them so)
      const size_t slot = (size_t)step * nch + (size_t)(&c - chunks.data());
      const bool folded_head = c.pg != nullptr && step_fuses(m, p, (long)t * c.Bl);
      // (retirement: the logits rows are in slot order; a traced step scatters them to the sequences' rows below)
      float* logits_dst = (io.trace_logits && !retire) ? io.trace_logits + trow * S : sc.logits;
      // (the greedy pointer launch makes its own dot products when the head is not folded)
      if (mode.pick == Mode::POINTER)
        FF_RETURN_IF(decoder_pass(m, p, kn, buf, sc, c, c.Fl, c.Bl, io.mask, io.kv_len, t, false, nullptr, st,
                                  folded_head ? logits_dst : nullptr));
      else
        FF_RETURN_IF(step_head(c, sc, t, c.Fc, c.Bc, folded_head, logits_dst, st));
      FF_RETURN_IF(select_step(c, sc, step, slot, folded_head, logits_dst, trow, st));
    }
    slots_per_step.push_back(nslots);
    return FF_OK;
  }
  // What every opt-in step opens with: the decoder pass over the prefix, then -- unless the folded head has left them already --
  // the logits by the pointer GEMM (always the GEMM + reduce form, as a decode with log-probabilities):
  // logits[w * Fc + i, s] = < p[w * Fc + i, :], memory[w, s, :] >, one GEMM problem per wireframe, as the pointer launch.
  int step_head(const Chunk& c, const Scratch& sc, int t, int Fc, int Bc, bool folded_head, float* logits_dst, hipStream_t st) {
    FF_RETURN_IF(decoder_pass(m, p, kn, buf, sc, c, Fc, Bc, io.mask, io.kv_len, t, false, nullptr, st, folded_head ? logits_dst : nullptr));
    if (folded_head) return FF_OK;
    return ff_gemm_f32_batched(sc.p, E, nullptr, 0, io.memory + (size_t)c.w0 * S * E, E, nullptr, nullptr, 0, logits_dst, S, Fc, S, E, 0,
                               0, c.nw, (long long)Fc * E, (long long)S * E, (long long)Fc * S, st);
  }
  // What the two constrained-beam step descriptors have in common: the rule, the records of step `step` in and of position
  // t = step + 1 out, the rule's state from half step & 1 to half t & 1, the byte rows, the parent and token rows.
  template <typename D>
  void fill_beam_step(D* d, const Chunk& c, const Rule& r, int step) const {
    const int t = step + 1;
    const size_t in = (size_t)step * Btot + c.b0, out = (size_t)t * Btot + c.b0;
    const size_t hin = (size_t)(step & 1) * Btot + c.b0, hout = (size_t)(t & 1) * Btot + c.b0;
    memset(d, 0, sizeof(*d));
    d->width = mode.G; d->follows = r.follows; d->L = r.L; d->flags = r.flags; d->ntok = m->num_token;
    d->scores_in = buf.score + in; d->fin_in = buf.finished + in;
    d->first_in = buf.first + hin; d->prev_in = buf.prev + hin; d->visited_in = buf.visited + hin * r.fw;
    d->scores_out = buf.score + out; d->fin_out = buf.finished + out; d->dead_out = buf.dead + out;
    d->first_out = buf.first + hout; d->prev_out = buf.prev + hout; d->visited_out = buf.visited + hout * r.fw;
    d->mask_rows = buf.byte_rows + (size_t)c.b0 * S;
    d->parent = buf.parent + out; d->next_tok = buf.tok_all + out;
  }
  // The selection of step `step` (position t = step + 1) of one micro-batch from its logits.  Every opt-in launch reads the
  // mode's state row `step` and writes row t, the chunk's next x0 rows (with their statistics) and -- but for the forced one,
  // which counts nothing -- the stop counter; a step enqueued past the stop writes rows that nothing reads.
  int select_step(const Chunk& c, const Scratch& sc, int step, size_t slot, bool folded_head, float* logits_dst, size_t trow, hipStream_t st) {
    const int t = step + 1;
    const float* mem_w = io.memory + (size_t)c.w0 * S * E;
    const unsigned char* mask_w = io.mask + (size_t)c.w0 * S;
    const int* kv_w = io.kv_len + c.w0;
    const size_t in = (size_t)step * Btot + c.b0, out = (size_t)t * Btot + c.b0;
    float* next_rows = c.x0 + (size_t)t * c.Bl * E;   // (Bl = Bc but under retirement, which every opt-in mode excludes)
    const bool forced = mode.pick == Mode::FORCED, beam = mode.pick == Mode::BEAM, draw = mode.pick == Mode::DRAW;
    const bool hand_over = lagged && !forced;   // (a forced step counts nothing: its slot and trow are not used)
    int* arrive = hand_over ? buf.arrive + slot : nullptr;
    int* host_slot = hand_over ? pool->hpin_dev + slot : nullptr;
    // what every opt-in launch takes: the chunk's logits, masks and memory, its Bc rows, the next x0 rows and the stop counter
    const ff_step_io sio{logits_dst, S, S, mask_w, kv_w, c.Bc, c.Fc, p->term_lo, p->term_hi, m->num_token, mem_w, E, next_rows, E, c.x0stat,
                         !forced ? buf.cnt_ge + slot : nullptr, arrive, host_slot};
    int* tok_out = buf.tok_all + out;
    if (forced)   // scores position t of the paths and appends THAT token's row; its records have T - 1 rows: row `step`
      return ff_pointer_forced_sync(sio, tok_out, buf.score + in, buf.greedy + in, buf.rank + in, st);
    if (mode.pick != Mode::POINTER) {   // (a draw or an arg-max arm returns from its launch; a beam arm goes on to the beam tail below)
      const int W = mode.G, rows = N * F * mode.G;   // (rows: the uniforms of one step, read through the chunk's row_id)
      if (mode.rule == Mode::NONE) {   // (a sequence entry: the same launch in its sequence form, which counts otherwise)
        if (beam)
          FF_RETURN_IF(ff_beam_select_sync(sio, W, buf.score + in, buf.score + out, buf.finished + in, buf.finished + out, nullptr, 0, t,
                                           buf.parent + out, tok_out, st, mode.sequence ? (mode.stop_best ? 2 : 1) : 0));
        else
          return ff_pointer_sample_sync(sio, mode.uniforms + (size_t)step * rows, rows, buf.row_id + c.b0, buf.finished + in,
                                        mode.temperature, mode.top_k, mode.top_p, tok_out, buf.score + out, buf.finished + out, st,
                                        mode.sequence);
      } else {
        const Rule r = rule_of(c);
        const ff_loop_rule_io rio{r.follows, r.L, r.flags, m->num_token};
        // the look-aheads: this step selects position t, so a loop has T - 1 - t further positions to close in; a sequence row
        // is longer than the tables' byte reaches (config A: T = 259), so under the sequence rule the budget is clamped to 254
        const int budget = mode.rule == Mode::SEQUENCE && T - 1 - t > 254 ? 254 : T - 1 - t;
        const ff_lookahead_io ahead{mode.ahead == 1 ? mode.close_dist + (size_t)c.w0 * r.L * r.L : nullptr,
                                    mode.ahead ? mode.cycle_len + (size_t)c.w0 * r.L : nullptr, budget, mode.ahead == 2 ? 1 : 0};
        const ff_lookahead_io* la = mode.ahead ? &ahead : nullptr;
        if (beam) {   // the rule per beam: state half step & 1 -> half t & 1 (the common operands come from sio)
          if (mode.sequence) {
            ff_beam_sequence_constrained_step d;
            fill_beam_step(&d, c, r, step);
            d.tok_sep = mode.tok_sep; d.tok_eos = p->tok_eos; d.stop_best = mode.stop_best;
            d.open_out = buf.open + out;
            FF_RETURN_IF(ff_beam_sequence_constrained_select_sync(sio, &d, la, st));
          } else {
            ff_beam_constrained_step d;
            fill_beam_step(&d, c, r, step);
            d.dead_in = buf.dead + in;
            FF_RETURN_IF(ff_beam_constrained_select_sync(mode.op, sio, &d, la, st));
          }
        } else {   // (the visited words and the byte rows belong to the sequence and are rewritten in stream order)
          const ff_constrained_state cs{buf.finished + in, buf.first + in, buf.prev + in, buf.visited + (size_t)c.b0 * r.fw,
                                        buf.byte_rows + (size_t)c.b0 * S, tok_out, buf.score + out, buf.finished + out, buf.dead + out,
                                        buf.first + out, buf.prev + out};
          if (draw) {   // (this step's uniforms are read through the chunk's row_id)
            const ff_sample_draw_io dio{mode.uniforms + (size_t)step * rows, rows, buf.row_id + c.b0, mode.temperature, mode.top_k, mode.top_p};
            return mode.sequence ? ff_pointer_sequence_constrained_sample_sync(sio, rio, cs, mode.tok_sep, p->tok_eos, la, dio, st)
                                 : ff_pointer_constrained_sample_sync(mode.op, sio, rio, cs, la, dio, st);
          }
          return mode.sequence ? ff_pointer_sequence_constrained_sync(sio, rio, cs, mode.tok_sep, p->tok_eos, la, st)   // (SEP and EOS in place of a terminator range)
                               : ff_pointer_constrained_sync(mode.op, sio, rio, cs, la, st);
        }
      }
      // the beam tail (only the beam arms above get here): behind a top-W selection, the reorder of positions < t of x0 and qkv0 on the same stream: the next decoder pass reads
      // reordered prefixes only.  (Nothing reads the prefixes after the last step: no reorder there.)
      if (mode.trace_parent)
        FF_CHECK_HIP(hipMemcpyAsync(mode.trace_parent + trow, buf.parent + out, sizeof(int) * (size_t)c.Bc, hipMemcpyDeviceToDevice, st));
      if (t < T - 1) FF_RETURN_IF(ff_beam_reorder(c.x0, E, c.qkv0, c.qkv0 ? 3 * E : 0, c.Bc, t, buf.parent + out, c.Bc / W, W, st));
      return FF_OK;
    }
    ff_pointer_sync psync{each_eos ? buf.seen + c.b0 : nullptr, arrive, host_slot, p->variant == FF_PARALLEL ? 0 : 1, c.x0stat,
                          folded_head ? 1 : 0, c.slot, retire ? fin_dev + c.b0 : nullptr, t, p->term_lo, p->term_hi};
    FF_RETURN_IF(ff_pointer_argmax_sync(
        folded_head ? nullptr : sc.p, E, mem_w, S, E, mask_w, kv_w, io.extra_mask ? io.extra_mask + (size_t)c.b0 * S : nullptr, S, c.Bl,
        c.Fl, buf.tok_all + out, io.trace_best ? io.trace_best + trow : nullptr, io.trace_second ? io.trace_second + trow : nullptr,
        buf.lp_all ? buf.lp_all + in : nullptr,   // (indexed by sequence, as the tokens are)
        logits_dst, S, next_rows, E, buf.cnt_ge + slot, m->num_token, buf.cnt_eq + slot, p->tok_eos,
        (each_eos || lagged || c.x0stat || folded_head || retire) ? &psync : nullptr, st));
    if (retire && io.trace_logits)
      FF_RETURN_IF(ff_permute_rows(sc.logits, c.Bl, nullptr, io.trace_logits + trow * S, c.Bc, c.slot, 1, c.Bl, S, st));
    return FF_OK;
  }
  // ---- forced decode ------------------------------------------------------------------------------------------------------------
  // The caller's paths as the token array (main stream, in front of the prologue's fork: every stream sees them).
  int forced_tokens() { return ff_forced_tokens(mode.forced->paths, buf.tok_all, Btot, T, S, io.main_st); }
  // Step `step` of every micro-batch that still has a row to score.  Nothing is read back, nothing is counted.
  int forced_loop() {
    for (int step = 0; step < forced_steps; ++step) {
      const int t = step + 1;
      for (const Chunk& c : chunks) {
        if (step >= chunk_steps[(size_t)(&c - chunks.data())]) continue;
        hipStream_t st = sts[c.sid];
        const Scratch& sc = buf.scr[c.sid];
        const bool folded_head = c.pg != nullptr && step_fuses(m, p, (long)t * c.Bc);
        float* logits_dst = io.trace_logits ? io.trace_logits + ((size_t)step * Btot + c.b0) * S : sc.logits;
        FF_RETURN_IF(step_head(c, sc, t, c.Fc, c.Bc, folded_head, logits_dst, st));
        FF_RETURN_IF(select_step(c, sc, step, 0, folded_head, logits_dst, 0, st));   // (no counter slot, no trace row offset)
      }
    }
    enq = forced_steps;
    return FF_OK;
  }
  // Join, then the packing of the per-step records on the main stream.
  int forced_epilogue() {
    const hipStream_t main_st = io.main_st;
    if (forked && forced_steps > 0)
      for (int s = 0; s < ns; ++s) {
        FF_CHECK_HIP(hipEventRecord(pool->join_ev[s], sts[s]));
        FF_CHECK_HIP(hipStreamWaitEvent(main_st, pool->join_ev[s], 0));
      }
    const ff_forced_params* fp = mode.forced;
    FF_RETURN_IF(ff_forced_finalize(buf.tok_all, buf.score, buf.greedy, buf.rank, fp->lengths, Btot, T, fp->logprob, fp->greedy,
                                    fp->rank, fp->seq_logprob, main_st));
    FF_CHECK_HIP(hipStreamSynchronize(main_st));   // (the caller may free or reuse the workspace next, as after ff_decode)
    if (io.steps_done) *io.steps_done = forced_steps;
    return FF_OK;
  }
  // Which counter the stop rule reads and how: cnt_ge and "the first step that leaves 0" for the parallel variant (tokens >=
  // num_token of unfinished rows), for the sequence sample mode (rows unfinished after the step) and for the sequence beam mode
  // (non-empty beams, or rank-0 beams, unfinished after the step); cnt_eq and the cumulative EOS count otherwise.
  bool zero_rule() const {
    return p->variant == FF_PARALLEL || mode.sequence;
  }
  // the stop rule over the first n steps' counters, per_chunk = [n][nch]
  bool stop_rule(const int* per_chunk, int n) {
    tot.assign((size_t)n, 0);
    const volatile int* v = per_chunk;
    for (int s = 0; s < n; ++s)
      for (int c = 0; c < nch; ++c) tot[(size_t)s] += v[(size_t)s * nch + c];
    const int* cnt = tot.data();
    if (p->stop_fn) return p->stop_fn(p->stop_user, cnt, n) != 0;   // the caller's (batch-global) rule
    if (zero_rule()) {
      for (int s = 0; s < n; ++s) if (cnt[s] == 0) return true;
    } else {
      int cum = 0;
      for (int s = 0; s < n; ++s) { cum += cnt[s]; if (cum == N) return true; }
    }
    return false;
  }
  // FF_RETIRE_FINISHED check point: sequences whose finish position is <= bound leave their micro-batch.  `bound` is a position
  // whose step is already enqueued, and only finish positions <= bound are looked at (later ones may or may not be visible
  // yet): the decision does not depend on timing.  A chunk is compacted when it loses at least retire_min_shrink of its slots.
  // x0 (positions 0..enq), qkv0 (0..enq-1) and the appended rows' statistics are gathered into the stream's scratch in the new
  // slot order and copied back; the maps come from the pinned staging area, whose previous uploads have completed (every check
  // point first waits for events recorded behind them, or drains the streams).  Returns the number of live sequences left.
  int compact_chunks(int bound, long* live_left) {
    *live_left = 0;
    size_t soff = 0;
    for (Chunk& c : chunks) {
      if (c.Bl == 0) continue;
      std::vector<int>& hs = hslot[(size_t)(&c - chunks.data())];
      std::vector<char> live((size_t)c.Bl);
      for (int i = 0; i < c.Bl; ++i) live[(size_t)i] = hfin[(size_t)c.b0 + hs[(size_t)i]] > bound;
      std::vector<int> perm;
      const int fl = ordered_slots(live, c.nw, c.Fl, &perm, live_left), nb = c.nw * fl;
      const int shrink = c.Bl - nb;
      if (shrink == 0 || (double)shrink < (double)p->retire_min_shrink * c.Bl) continue;
      hipStream_t st = sts[c.sid];
      std::vector<int> nhs((size_t)nb);
      for (int i = 0; i < nb; ++i) nhs[(size_t)i] = hs[(size_t)perm[(size_t)i]];
      if (nb > 0) {
        int* sp = pool->stage + soff;
        int* ss = sp + nb;
        soff += 2 * (size_t)nb;
        memcpy(sp, perm.data(), sizeof(int) * (size_t)nb);
        memcpy(ss, nhs.data(), sizeof(int) * (size_t)nb);
        FF_CHECK_HIP(hipMemcpyAsync(c.perm, sp, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, st));
        const Scratch& sc = buf.scr[c.sid];
        auto regather = [&](float* rows, float* scratch, int npos, int width) -> int {   // npos positions of `width` floats per slot
          FF_RETURN_IF(ff_permute_rows(rows, c.Bl, c.perm, scratch, nb, nullptr, npos, nb, width, st));
          FF_CHECK_HIP(hipMemcpyAsync(rows, scratch, sizeof(float) * (size_t)npos * nb * width, hipMemcpyDeviceToDevice, st));
          return FF_OK;
        };
        FF_RETURN_IF(regather(c.x0, sc.x, enq + 1, E));
        if (c.qkv0) FF_RETURN_IF(regather(c.qkv0, sc.qkv, enq, 3 * E));
        if (c.x0stat) FF_RETURN_IF(regather(c.x0stat, sc.y, 1, E / 16));
        // the new slot map: perm and slot are adjacent in the staging area, the device slot map is behind the gather above
        FF_CHECK_HIP(hipMemcpyAsync(c.slot, ss, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, st));
      }
      hs.swap(nhs);
      c.Fl = fl; c.Bl = nb;
    }
    return FF_OK;
  }
  // retirement at a check point: finish positions <= bound, read from host-mapped memory (behind the events just waited for)
  // or -- when they live in the workspace -- after draining the streams (bound = enq - 1: step `bound` is enqueued either way)
  int retire_at(int bound, bool drained) {
    if (fin_host) {
      const volatile int* v = fin_host;
      for (int i = 0; i < Btot; ++i) hfin[(size_t)i] = v[i];
    } else {
      FF_RETURN_IF(read_back(hfin.data(), buf.fin, (size_t)Btot, drained));
      bound = enq - 1;
    }
    long live = 0;
    FF_RETURN_IF(compact_chunks(bound, &live));
    if (live == 0) stopped = true;   // (the steps_kernel finds the step with no unfinished sequence among those enqueued)
    return FF_OK;
  }
  int wait_marks() { for (int s = 0; s < ns; ++s) FF_CHECK_HIP(hipEventSynchronize(pool->chk_ev[s])); return FF_OK; }
  // Stop rule on the host WITHOUT draining the queue and WITHOUT a copy launch: every pointer launch owns the counter of
  // its (step, micro-batch) and its last block stores the total into host-mapped pinned memory (ff_pointer_count_block).
  // Every sync_every steps an event is recorded behind the steps enqueued so far (on every stream); it is waited for
  // when another sync_every steps have been enqueued -- by then the host is a whole period ahead of it, so the wait
  // normally returns at once and the GPU always has a period of steps queued.  A stop is noticed at most
  // 2 * sync_every - 1 steps late; those surplus steps are dropped by the finalize kernels (exact results).
  int check_point() {
    if (lagged) {
      if (pending_enq > 0) {
        FF_RETURN_IF(wait_marks());
        stopped = stop_rule(pool->hpin, pending_enq);
        if (!stopped && retire) FF_RETURN_IF(retire_at(pending_enq, false));
        pending_enq = 0;
      }
      if (!stopped) {
        for (int s = 0; s < ns; ++s) FF_CHECK_HIP(hipEventRecord(pool->chk_ev[s], sts[s]));
        pending_enq = enq;
      }
      return FF_OK;
    }
    // more (step, micro-batch) counters than host slots: drain and copy
    // A caller's stop_fn is asked at the SAME cadence as on the lagged path (the first enq - sync_every steps, from
    // enq = 2 sync_every on): peers and idle ranks of a sharded decode replay exactly that sequence of host collectives
    // (dist.check_points).  The local rule has no such contract and looks at everything that has run.
    const int n_eval = p->stop_fn ? enq - p->sync_every : enq;
    if (n_eval <= 0) return FF_OK;
    std::vector<int> hcnt((size_t)n_eval * nch);
    FF_RETURN_IF(read_back(hcnt.data(), zero_rule() ? buf.cnt_ge : buf.cnt_eq, hcnt.size()));
    stopped = stop_rule(hcnt.data(), n_eval);
    if (!stopped && retire) FF_RETURN_IF(retire_at(enq - 1, true));
    return FF_OK;
  }
  // ---- greedy loop -----------------------------------------------------------------------------------
  int greedy_loop() {
    const int max_steps = T - 1;
    const auto host_t0 = std::chrono::steady_clock::now();
    while (enq < max_steps && !stopped) {
      FF_RETURN_IF(enqueue_step(enq));
      ++enq;
      if (p->sync_every > 0 && !(p->flags & FF_NO_STOP) && (enq % p->sync_every) == 0 && enq < max_steps) FF_RETURN_IF(check_point());
    }
    if (pending_enq > 0) FF_RETURN_IF(wait_marks());   // the slots are reused by the next call
    if (p->slots_per_step)
      for (int s = 0; s < T - 1; ++s) p->slots_per_step[s] = s < (int)slots_per_step.size() ? slots_per_step[(size_t)s] : 0;
    if (kn.dbg_timing) {
      const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
      FF_RETURN_IF(sync_all());
      const double tot_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - host_t0).count();
      fprintf(stderr, "[ff_decode] host enqueue of %d steps x %zu chunks (%d of %d sequences decoded): %.2f ms; until GPU idle: "
                      "%.2f ms\n", enq, chunks.size(), Btot, N * F, host_ms, tot_ms);
    }
    return FF_OK;
  }
  // The outputs of one micro-batch's rows from the per-step records up to the stop step (main stream).
  int pack(const Chunk& c) {
    const hipStream_t main_st = io.main_st;
    const int G = mode.G, dd = dedup ? 1 : 0;
    const bool ruled = mode.rule != Mode::NONE;
    // (the sequence entries: F = 1, no de-duplication, num_input is not read; forced: forced_epilogue packs all rows at once)
    if (mode.pick == Mode::BEAM) {
      if (mode.sequence && ruled)   // (tokens and dead flags along one walk, the rest from the stop step's row)
        return ff_sequence_constrain_beam_finalize(buf.tok_all, buf.parent, buf.score, buf.finished, buf.dead, buf.open, Btot, T,
                                                   buf.steps_dev, G, c.w0, c.nw, c.b0, mode.rows, mode.scores, mode.finished,
                                                   mode.beam_dead_end, mode.beam_open_end, io.predict, mode.dead_end, mode.open_end,
                                                   io.seq_of_row, main_st);
      // (a sequence entry: also the finished flags of the stop step's row)
      FF_RETURN_IF(ff_beam_finalize(buf.tok_all, buf.parent, buf.score, Btot, T, buf.steps_dev, io.num_input, dd, F, G, c.w0, c.nw, c.Fc / G,
                                    c.f0, c.b0, mode.rows, mode.scores, io.predict, io.seq_of_row, main_st,
                                    mode.sequence ? buf.finished : nullptr, mode.finished));
      if (!ruled) return FF_OK;
      return ff_constrain_beam_dead(buf.dead, Btot, buf.steps_dev, io.num_input, dd, F, G, c.w0, c.nw, c.Fc / G, c.f0, c.b0, mode.dead_end,
                                    main_st);
    }
    if (mode.pick == Mode::DRAW) {
      if (!ruled)
        return ff_sample_finalize(buf.tok_all, buf.score, buf.finished, Btot, T, buf.steps_dev, io.num_input, dd, F, G, c.w0, c.nw,
                                  c.Fc / G, c.f0, c.b0, mode.rows, mode.logprob, mode.scores, io.predict, io.seq_of_row, main_st);
      if (mode.sequence)
        return ff_sequence_constrain_sample_finalize(buf.tok_all, buf.score, buf.finished, buf.dead, buf.first, Btot, T, buf.steps_dev, G,
                                                     c.w0, c.nw, c.b0, mode.rows, mode.logprob, mode.scores, mode.dead_end, mode.open_end,
                                                     io.predict, mode.predict_logprob, mode.predict_dead_end, mode.predict_open_end,
                                                     io.seq_of_row, main_st);
      return ff_constrain_sample_finalize(buf.tok_all, buf.score, buf.finished, buf.dead, Btot, T, buf.steps_dev, io.num_input, dd, F, G,
                                          c.w0, c.nw, c.Fc / G, c.f0, c.b0, mode.rows, mode.logprob, mode.scores, mode.dead_end, io.predict,
                                          mode.predict_logprob, mode.predict_dead_end, io.seq_of_row, main_st);
    }
    if (mode.pick == Mode::ARGMAX) {
      if (mode.sequence)
        return ff_sequence_constrain_finalize(buf.tok_all, buf.score, buf.finished, buf.dead, buf.first, Btot, T, buf.steps_dev, c.w0, c.nw,
                                              c.b0, io.predict, mode.logprob, mode.dead_end, mode.open_end, io.seq_of_row, main_st);
      return ff_constrain_finalize(buf.tok_all, buf.score, buf.finished, buf.dead, Btot, T, buf.steps_dev, io.num_input, dd, F, c.w0,
                                   c.nw, c.Fc, c.f0, c.b0, io.predict, mode.logprob, mode.dead_end, io.seq_of_row, main_st);
    }
    const long total = (long)c.nw * F * T;
    const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
    hipLaunchKernelGGL(finalize_chunk_kernel, dim3(grid), dim3(256), 0, main_st, buf.tok_all, Btot, T, buf.steps_dev, io.num_input, dd,
                       F, c.w0, c.nw, c.Fc, c.f0, c.b0, io.predict, io.seq_of_row, retire ? fin_dev : nullptr, buf.lp_all, io.logprob);
    FF_CHECK_LAUNCH();
    return FF_OK;
  }
  // Join, then everything after the greedy loop on the main stream: stop step, packing, the optional return-pointer pass.
  int epilogue() {
    const hipStream_t main_st = io.main_st;
    if (forked)
      for (int s = 0; s < ns; ++s) {
        FF_CHECK_HIP(hipEventRecord(pool->join_ev[s], sts[s]));
        FF_CHECK_HIP(hipStreamWaitEvent(main_st, pool->join_ev[s], 0));
      }
    hipLaunchKernelGGL(steps_kernel, dim3(1), dim3(64), 0, main_st, buf.cnt_ge, buf.cnt_eq, nch, zero_rule() ? FF_PARALLEL : p->variant, N, enq,
                       ((p->flags & FF_NO_STOP) || p->stop_fn) ? 1 : 0, buf.cnt_tot, buf.steps_dev);
    FF_CHECK_LAUNCH();
    for (const Chunk& c : chunks) FF_RETURN_IF(pack(c));
    int steps = 0;
    FF_CHECK_HIP(hipMemcpyAsync(&steps, buf.steps_dev, sizeof(int), hipMemcpyDeviceToHost, main_st));
    if (io.step_counts && enq > 0)
      FF_CHECK_HIP(hipMemcpyAsync(io.step_counts, buf.cnt_tot, sizeof(int) * enq, hipMemcpyDeviceToHost, main_st));
    FF_CHECK_HIP(hipStreamSynchronize(main_st));
    if (io.steps_done) *io.steps_done = steps;

    // ---- optional: project(decoder(...)) of every prefix row at the last executed step
    //      (SurfaceFormer returns it as inputs['pointer'], reference model.py:217) --------------------
    if ((p->flags & FF_RETURN_POINTER) && steps > 0) {
      FF_CHECK_ARG(m->FF >= m->E, "ff_decode: FF_RETURN_POINTER needs FF >= E");
      FF_CHECK_ARG(Btot == N * F, "ff_decode: FF_RETURN_POINTER is not available with de-duplicated sequences");
      for (const Chunk& c : chunks) {
        const Scratch& sc = buf.scr[0];
        // one micro-batch: its [steps * Bc, E] rows ARE pointer_out [steps, Btot, E]; several: through the FF-wide scratch
        // and one strided copy per micro-batch (was one copy launch per position: 258 of them for configs A / D)
        float* proj_all = nch == 1 ? io.pointer_out : sc.h;
        FF_RETURN_IF(decoder_pass(m, p, kn, buf, sc, c, c.Fc, c.Bc, io.mask, io.kv_len, steps, true, proj_all, main_st));
        if (nch > 1)
          FF_CHECK_HIP(hipMemcpy2DAsync(io.pointer_out + (size_t)c.b0 * E, sizeof(float) * (size_t)Btot * E, proj_all,
                                        sizeof(float) * (size_t)c.Bc * E, sizeof(float) * (size_t)c.Bc * E, (size_t)steps,
                                        hipMemcpyDeviceToDevice, main_st));
      }
    }
    return FF_OK;
  }
};

// One decode call from validation to the packed outputs.
int run_decode(const ff_model* m, const ff_decode_params* p, const DecodeIO& io, void* workspace, size_t workspace_bytes,
               const Mode& mode);

// ---- the opt-in entries --------------------------------------------------------------------------------------------------------
// The wording of one entry's refusals, kept next to the entry: its name, the option as the variant message words it (parallel
// entries), the parameter struct as the null message words it, the other variant's entry (sequence entries), the operands and
// outputs it requires as their message names them.
struct Entry {
  const char *name, *subject, *noun, *sibling, *required;
  int ahead_lo = -1;            // the lowest look-ahead form the caller may choose (0: sampled, 1: beam, 2: 1 under the sequence entries' text); -1: the entry fixes the form
  bool own_draw_text = false;   // ff_decode_sample: temperature / top_k / top_p under its own text, in front of the outputs
  bool given = false, have = false;   // filled by the entry: its parameter struct is not null; all it requires of it is there
};
// What a parallel entry takes from the greedy call's signature only to refuse it (the sequence entries have none of it: null).
struct Refused { const unsigned char* extra_mask; const float *trace_best, *trace_second, *pointer_out; };

// The look-ahead of a constrained decode (form 1: the closure look-ahead, 2: the exact one), beyond what the step checks: the
// flag bits and tables of the form, and the limits of the budget's byte and of the exact search.
int check_lookahead(const char* name, int form, int flags, const unsigned char* close_dist, const unsigned char* cycle_len,
                    const ff_model* m, const ff_decode_params* p, bool clamped = false) {
  if (form == 1) {
    FF_CHECK_ARG(flags & FF_CONSTRAIN_CONNECT, "%s: the look-ahead needs FF_CONSTRAIN_CONNECT", name);
    FF_CHECK_ARG(close_dist && cycle_len, "%s: close_dist and cycle_len are required", name);
    FF_CHECK_ARG(clamped || p->T <= 256, "%s: T=%d above 256 (the budget T - 2 must fit the tables' byte)", name, p->T);
  } else if (form == 2) {
    FF_CHECK_ARG((flags & FF_CONSTRAIN_CONNECT) && (flags & FF_CONSTRAIN_NO_REPEAT),
                 "%s: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT", name);
    FF_CHECK_ARG(cycle_len, "%s: cycle_len is required", name);
    FF_CHECK_ARG(clamped || p->T <= 256, "%s: T=%d above 256 (the budget T - 2 must fit the table's byte)", name, p->T);
    FF_CHECK_ARG(p->L + m->num_token <= FF_EXACT_MAX_S, "%s: L=%d above %d (L + num_token keys at most %d)", name, p->L,
                 FF_EXACT_MAX_S - m->num_token, FF_EXACT_MAX_S);
  }
  return FF_OK;
}

bool sequence_query_ok(const ff_decode_params* p) { return p && p->variant == FF_SEQ2SEQ && p->F == 1; }   // (what the sequence size queries refuse)

// Every opt-in entry's checks, in THE order all of them keep (tests/test_entry_checks.py pins it); a check that the mode's facts
// do not call for is skipped.
int check_entry(const Entry& e, const Mode& md, const ff_model* m, const ff_decode_params* p, const Refused& no, const int64_t* predict) {
  const char* name = e.name;
  const bool beam = md.pick == Mode::BEAM, draw = md.pick == Mode::DRAW;
  // 1. the three structs
  FF_CHECK_ARG(m && p && e.given, "%s: null model, params or %s params", name, e.noun);
  // 2. the variant, and the combinations the entry excludes
  if (md.sequence) {
    FF_CHECK_ARG(p->variant == FF_SEQ2SEQ && p->F == 1, "%s: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has %s",
                 name, e.sibling);
    FF_CHECK_ARG(!(p->flags & (FF_RETIRE_FINISHED | FF_RETURN_POINTER | FF_NO_STOP | FF_STOP_EACH_EOS)) && !p->stop_fn,
                 "%s: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn", name);
  } else {
    FF_CHECK_ARG(p->variant == FF_PARALLEL, "%s: %s a parallel-variant option", name, e.subject);
    FF_CHECK_ARG(!(p->flags & (FF_RETIRE_FINISHED | FF_RETURN_POINTER | FF_NO_STOP)) && !p->stop_fn && !no.extra_mask,
                 "%s: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask", name);
  }
  const int S = p->L + m->num_token;
  // 3. the sequences per anchor
  if (beam) FF_CHECK_ARG(md.G >= 1 && md.G <= 8 && md.G <= S, "%s: width=%d outside 1..8 or above S=%d", name, md.G, S);
  if (draw) FF_CHECK_ARG(md.G >= 1 && md.G <= 64, "%s: num_samples=%d outside 1..64", name, md.G);
  if (e.own_draw_text)
    FF_CHECK_ARG(md.temperature >= 0.f && md.temperature <= 3.402823466e+38f && md.top_k >= 0 && md.top_p > 0.f && md.top_p <= 1.f,
                 "%s: temperature=%g must be finite and >= 0, top_k=%d >= 0, top_p=%g in (0, 1]", name, (double)md.temperature, md.top_k,
                 (double)md.top_p);
  // 4. the sequence beam's stop rule
  if (beam && md.sequence) FF_CHECK_ARG(md.stop_best == 0 || md.stop_best == 1, "%s: stop_best=%d must be 0 or 1", name, md.stop_best);
  // 5. the rule's operands (the operators' own checks: flags, follow table, terminator range or SEP / EOS)
  const ff_loop_rule_io rio{md.follows, p->L, md.flags, m->num_token};
  if (md.rule == Mode::LOOP) FF_RETURN_IF(ff_loop_rule_check(name, rio, S, p->term_lo, p->term_hi));
  if (md.rule == Mode::SEQUENCE) FF_RETURN_IF(ff_sequence_rule_check(name, rio, S, md.tok_sep, p->tok_eos));
  // 6. the look-ahead
  if (e.ahead_lo == 0)
    FF_CHECK_ARG(md.ahead >= 0 && md.ahead <= 2, "%s: lookahead=%d must be 0 (none), 1 (look-ahead) or 2 (exact)", name, md.ahead);
  if (e.ahead_lo == 1) FF_CHECK_ARG(md.ahead == 1 || md.ahead == 2, "%s: lookahead=%d must be 1 (look-ahead) or 2 (exact)", name, md.ahead);
  if (e.ahead_lo == 2) FF_CHECK_ARG(md.ahead == 1 || md.ahead == 2, "%s: form=%d must be 1 (look-ahead) or 2 (exact)", name, md.ahead);
  // (a sequence entry's step clamps the budget to the tables' byte: a row longer than 256 positions is accepted)
  FF_RETURN_IF(check_lookahead(name, md.ahead, md.flags, md.close_dist, md.cycle_len, m, p, md.rule == Mode::SEQUENCE));
  // 7. what the entry requires; a parallel entry also a terminator range and none of the greedy call's traces
  if (md.sequence) {
    FF_CHECK_ARG(e.have && predict, "%s: %s are required", name, e.required);
  } else {
    FF_CHECK_ARG(p->term_lo < p->term_hi, "%s: empty terminator range [%d, %d)", name, p->term_lo, p->term_hi);
    FF_CHECK_ARG(e.have && !no.trace_best && !no.trace_second && !no.pointer_out, "%s: %s required; no best / second traces, no pointer_out",
                 name, e.required);
  }
  // 8. the sizes (the parallel beam entries have no such check)
  if (draw || (beam && md.sequence))
    FF_CHECK_ARG(p->N > 0 && p->F > 0 && (long long)p->N * p->F * md.G < (1LL << 31), "%s: bad sizes", name);
  // 9. the draw's own check, with the step's text: the uniforms of one step
  if (draw && !e.own_draw_text) {
    const int rows = p->N * p->F * md.G;
    FF_RETURN_IF(ff_sample_draw_check(name, ff_sample_draw_io{md.uniforms, rows, nullptr, md.temperature, md.top_k, md.top_p}, rows));
  }
  // 10. the staging area of a beam's reorder: ff_beam_reorder stages a group's x0 (+ q|k|v) rows in 64 KB of LDS
  if (beam)
    FF_CHECK_ARG((size_t)md.G * ((p->flags & FF_REUSE_LAYER0_QKV) ? 4 : 1) * (size_t)m->E * sizeof(float) <= 65536,
                 "%s: width=%d at E=%d exceeds the reorder's staging area", name, md.G, m->E);
  return FF_OK;
}

// What every decode entry's arguments have in common.  An opt-in entry hands on no extra mask, no pointer_out, no best / second
// traces and no log-probabilities; a sequence entry has no num_input either.
struct EntryArgs {
  const float* memory; const unsigned char* mask; const int *kv_len, *num_input, *num_input_host;
  int64_t* predict; int *steps_done, *step_counts; float* trace_logits; int* seq_of_row; void* workspace; size_t workspace_bytes;
  ff_stream_t stream;
};

// An opt-in entry behind its mode: the checks, then the decode.  For a sequence entry the terminator range is the EOS token alone
// (SEP and the other special tokens do not finish a draw, a beam or a row).
int run_entry(const Entry& e, const Mode& md, const ff_model* m, const ff_decode_params* p, const Refused& no, const EntryArgs& a) {
  FF_RETURN_IF(check_entry(e, md, m, p, no, a.predict));
  ff_decode_params q;
  if (md.sequence) { q = *p; q.term_lo = p->tok_eos; q.term_hi = p->tok_eos + 1; }
  return run_decode(m, md.sequence ? &q : p, DecodeIO{a.memory, a.mask, a.kv_len, a.num_input, a.num_input_host, nullptr, a.predict, a.steps_done, a.step_counts,
                                    nullptr, a.trace_logits, nullptr, nullptr, a.seq_of_row, (hipStream_t)a.stream, nullptr},
                    a.workspace, a.workspace_bytes, md);
}
const Refused no_refused{nullptr, nullptr, nullptr, nullptr};

}  // namespace

// =================================================================================================
extern "C" size_t ff_encode_workspace_bytes(const ff_model* m, int N, int L) {
  if (!m || N <= 0 || L < 0) return 0;
  const size_t S = (size_t)L + m->num_token, E = m->E;
  size_t tot = 0;
  tot += 2 * bump_bytes((size_t)N * L * E, 4);          // embedding MLP hidden / output
  tot += 4 * bump_bytes((size_t)N * S * E, 4);          // x, y, yq, o
  tot += bump_bytes((size_t)N * S * 3 * E, 4);          // qkv
  tot += bump_bytes((size_t)N * S * m->FF, 4);          // ffn hidden
  return tot + 256;
}

extern "C" int ff_encode(const ff_model* m, const float* input, const unsigned char* mask,
                         const int* kv_len, int N, int L, float* memory, void* workspace,
                         size_t workspace_bytes, ff_stream_t stream) {
  FF_RETURN_IF(check_model(m));
  FF_CHECK_ARG(N > 0 && L >= 0 && input && mask && memory && workspace, "ff_encode: bad arguments");
  const int E = m->E, FFd = m->FF, H = m->H, S = L + m->num_token;
  FF_CHECK_ARG(S <= m->pos_len, "ff_encode: S=%d exceeds the position table (%d rows)", S, m->pos_len);
  hipStream_t st = (hipStream_t)stream;
  FF_RETURN_IF(ff_gemm_prepare_stream(st));
  Bump bp(workspace, workspace_bytes);
  float* h1 = bp.take<float>((size_t)N * L * E);
  float* h2 = bp.take<float>((size_t)N * L * E);
  float* x = bp.take<float>((size_t)N * S * E);
  float* y = bp.take<float>((size_t)N * S * E);
  float* yq = bp.take<float>((size_t)N * S * E);
  float* o = bp.take<float>((size_t)N * S * E);
  float* qkv = bp.take<float>((size_t)N * S * 3 * E);
  float* hb = bp.take<float>((size_t)N * S * FFd);
  if (!bp.ok) { ff_set_error("ff_encode: workspace too small (%zu needed)", bp.off); return FF_ERR_WORKSPACE; }
  const int R = N * S;
  // a1: edge MLP (embedding.py:30-36) + token rows
  if (L > 0) {
    FF_RETURN_IF(gemm(input, m->in_dim, nullptr, 0, m->emb_w1, m->in_dim, m->emb_b1, nullptr, 0, h1, E, N * L, E,
                      m->in_dim, 1, st));
    FF_RETURN_IF(gemm(h1, E, nullptr, 0, m->emb_w2, E, m->emb_b2, nullptr, 0, h2, E, N * L, E, E, 0, st));
  }
  FF_RETURN_IF(ff_assemble_embedding(m->tok_embed, m->num_token, h2, E, N, L, E, x, st));
  // a4: pre-norm encoder layers (transformer.py:164-176)
  for (int l = 0; l < m->num_enc_layers; ++l) {
    const ff_layer_weights& w = m->enc[l];
    FF_RETURN_IF(ff_layernorm(x, E, w.norm1_w, w.norm1_b, m->ln_eps, y, E, yq, E, m->pos_table, E, 1, S, R, E, st));
    FF_RETURN_IF(gemm(yq, E, y, 2 * E, w.self_attn.in_proj_w, E, w.self_attn.in_proj_b, nullptr, 0, qkv, 3 * E, R,
                      3 * E, E, 0, st));
    ff_attn_desc d;
    memset(&d, 0, sizeof(d));
    d.q = qkv; d.k = qkv + E; d.v = qkv + 2 * E; d.o = o;
    d.ldq = d.ldk = d.ldv = 3 * E; d.ldo = E;
    d.num_groups = N; d.num_heads = H;
    d.nq = S; d.q_group_stride = S; d.q_inner = S; d.q_outer_stride = 0;
    d.nk = S; d.k_group_stride = S; d.k_stride = 1;
    d.kv_len = kv_len; d.key_mask = mask; d.mask_stride = S;
    d.scale = 0.125f;
    FF_RETURN_IF(ff_attention(&d, st));
    FF_RETURN_IF(gemm(o, E, nullptr, 0, w.self_attn.out_w, E, w.self_attn.out_b, x, E, x, E, R, E, E, 0, st));
    FF_RETURN_IF(ff_layernorm(x, E, w.norm2_w, w.norm2_b, m->ln_eps, y, E, nullptr, 0, nullptr, 0, 1, 1, R, E, st));
    FF_RETURN_IF(gemm(y, E, nullptr, 0, w.lin1_w, E, w.lin1_b, nullptr, 0, hb, FFd, R, FFd, E, 1, st));
    FF_RETURN_IF(gemm(hb, FFd, nullptr, 0, w.lin2_w, FFd, w.lin2_b, x, E, x, E, R, E, FFd, 0, st));
  }
  FF_RETURN_IF(ff_layernorm(x, E, m->enc_norm_w, m->enc_norm_b, m->ln_eps, memory, E, nullptr, 0, nullptr, 0, 1, 1,
                            R, E, st));
  return FF_OK;
}

// The size queries: their own refusals (a width outside 1..8, num_samples outside 1..64, a sequence query on other than FF_SEQ2SEQ
// with F = 1), then decode_workspace_bytes for the mode's pick, rule, sequence and G.
extern "C" size_t ff_decode_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host) {
  return decode_workspace_bytes(m, p, num_input_host, Mode());
}

extern "C" size_t ff_decode_lp_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host) {
  return decode_workspace_bytes(m, p, num_input_host, Mode(), true);
}

extern "C" size_t ff_decode_beam_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host, int width) {
  if (width < 1 || width > 8) return 0;
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::BEAM, Mode::NONE, false, width));
}

extern "C" int ff_decode(const ff_model* m, const ff_decode_params* p, const float* memory,
                         const unsigned char* mask, const int* kv_len, const int* num_input,
                         const int* num_input_host, const unsigned char* extra_mask, int64_t* predict,
                         int* steps_done, int* step_counts, float* pointer_out, float* trace_logits,
                         float* trace_best, float* trace_second, int* seq_of_row, void* workspace,
                         size_t workspace_bytes, ff_stream_t stream) {
  return ff_decode_lp(m, p, memory, mask, kv_len, num_input, num_input_host, extra_mask, predict, steps_done, step_counts,
                      pointer_out, trace_logits, trace_best, trace_second, seq_of_row, workspace, workspace_bytes, nullptr, stream);
}

extern "C" int ff_decode_lp(const ff_model* m, const ff_decode_params* p, const float* memory,
                            const unsigned char* mask, const int* kv_len, const int* num_input,
                            const int* num_input_host, const unsigned char* extra_mask, int64_t* predict,
                            int* steps_done, int* step_counts, float* pointer_out, float* trace_logits,
                            float* trace_best, float* trace_second, int* seq_of_row, void* workspace,
                            size_t workspace_bytes, float* logprob, ff_stream_t stream) {
  return run_decode(m, p, DecodeIO{memory, mask, kv_len, num_input, num_input_host, extra_mask, predict, steps_done, step_counts,
                                   pointer_out, trace_logits, trace_best, trace_second, seq_of_row, (hipStream_t)stream, logprob},
                    workspace, workspace_bytes, Mode());
}

// ---- the opt-in entries: fill the mode from the entry's own parameter struct, then run_entry -----------------------------
#define FF_PAR_ARGS EntryArgs{memory, mask, kv_len, num_input, num_input_host, predict, steps_done, step_counts, trace_logits, seq_of_row, \
                              workspace, workspace_bytes, stream}
#define FF_SEQ_ARGS EntryArgs{memory, mask, kv_len, nullptr, nullptr, predict, steps_done, step_counts, trace_logits, seq_of_row, workspace, \
                              workspace_bytes, stream}
#define FF_PAR_REFUSED Refused{extra_mask, trace_best, trace_second, pointer_out}

extern "C" int ff_decode_beam(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_beam_params* beam, ff_stream_t stream) {
  Entry e{"ff_decode_beam", "beams are", "beam", nullptr, "beams and scores"};
  Mode md(Mode::BEAM, Mode::NONE, false);
  if ((e.given = beam != nullptr)) {
    take_beam(md, beam);
    e.have = beam->beams && beam->scores;
  }
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

// Forced keeps checks of its own (other exclusions, the host lengths): it is no selection over the greedy call's arguments.
extern "C" size_t ff_decode_forced_workspace_bytes(const ff_model* m, const ff_decode_params* p) {
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::FORCED));
}

extern "C" int ff_decode_forced(const ff_model* m, const ff_decode_params* p, const float* memory, const unsigned char* mask,
                                const int* kv_len, const ff_forced_params* forced, int* steps_done, float* trace_logits,
                                void* workspace, size_t workspace_bytes, ff_stream_t stream) {
  FF_CHECK_ARG(m && p && forced, "ff_decode_forced: null model, params or forced params");
  FF_CHECK_ARG(!(p->flags & (FF_RETIRE_FINISHED | FF_RETURN_POINTER | FF_STOP_EACH_EOS)) && !p->stop_fn,
               "ff_decode_forced: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_STOP_EACH_EOS and a stop_fn");
  FF_CHECK_ARG(forced->paths && forced->lengths && forced->lengths_host && forced->logprob && forced->greedy && forced->rank &&
                   forced->seq_logprob, "ff_decode_forced: paths, lengths (device and host) and the four outputs are required");
  FF_CHECK_ARG(p->N > 0 && p->F > 0 && p->T >= 1 && (long long)p->N * p->F < (1LL << 31) && (p->variant != FF_SEQ2SEQ || p->F == 1),
               "ff_decode_forced: bad sizes (seq2seq scores one row per wireframe)");
  for (long long r = 0; r < (long long)p->N * p->F; ++r)
    FF_CHECK_ARG(forced->lengths_host[r] >= 0 && forced->lengths_host[r] <= p->T - 1, "ff_decode_forced: lengths[%lld]=%d outside 0..%d",
                 r, forced->lengths_host[r], p->T - 1);
  Mode md(Mode::FORCED);
  md.forced = forced;
  return run_decode(m, p, DecodeIO{memory, mask, kv_len, nullptr, nullptr, nullptr, nullptr, steps_done, nullptr, nullptr, trace_logits,
                                   nullptr, nullptr, nullptr, (hipStream_t)stream, nullptr},
                    workspace, workspace_bytes, md);
}

extern "C" size_t ff_decode_sample_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host,
                                                   int num_samples) {
  if (num_samples < 1 || num_samples > 64) return 0;
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::DRAW, Mode::NONE, false, num_samples));
}

extern "C" int ff_decode_sample(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sample_params* sample, ff_stream_t stream) {
  Entry e{"ff_decode_sample", "sampling is", "sample", nullptr, "uniforms, samples, logprob and scores", -1, true};
  Mode md(Mode::DRAW, Mode::NONE, false);
  if ((e.given = sample != nullptr)) {
    take_draw(md, sample);
    e.have = sample->uniforms && sample->samples && sample->logprob && sample->scores;
  }
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

extern "C" size_t ff_decode_sequence_sample_workspace_bytes(const ff_model* m, const ff_decode_params* p, int num_samples) {
  if (num_samples < 1 || num_samples > 64 || !sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::DRAW, Mode::NONE, true, num_samples));
}

extern "C" int ff_decode_sequence_sample(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sample_params* sample, ff_stream_t stream) {
  Entry e{"ff_decode_sequence_sample", nullptr, "sample", "ff_decode_sample", "uniforms, samples, logprob, scores and predict"};
  Mode md(Mode::DRAW, Mode::NONE, true);
  if ((e.given = sample != nullptr)) {
    take_draw(md, sample);
    e.have = sample->uniforms && sample->samples && sample->logprob && sample->scores;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

extern "C" size_t ff_decode_sequence_beam_workspace_bytes(const ff_model* m, const ff_decode_params* p, int width) {
  if (width < 1 || width > 8 || !sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::BEAM, Mode::NONE, true, width));
}

extern "C" int ff_decode_sequence_beam(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sequence_beam_params* beam, ff_stream_t stream) {
  Entry e{"ff_decode_sequence_beam", nullptr, "beam", "ff_decode_beam", "beams, scores, finished and predict"};
  Mode md(Mode::BEAM, Mode::NONE, true);
  if ((e.given = beam != nullptr)) {
    take_beam(md, beam);
    md.stop_best = beam->stop_best; md.finished = beam->finished;
    e.have = beam->beams && beam->scores && beam->finished;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

extern "C" size_t ff_decode_sequence_constrained_workspace_bytes(const ff_model* m, const ff_decode_params* p) {
  if (!sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::ARGMAX, Mode::SEQUENCE, true));
}

// The greedy single-sequence decode (model.py:161-167, 191, 193-210) under the face-loop rule.
extern "C" int ff_decode_sequence_constrained(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sequence_constrain_params* constrain, ff_stream_t stream) {
  Entry e{"ff_decode_sequence_constrained", nullptr, "constrain", "ff_decode_constrained", "logprob, dead_end, open_end and predict"};
  Mode md(Mode::ARGMAX, Mode::SEQUENCE, true);
  if ((e.given = constrain != nullptr)) {
    take_rule(md, constrain);
    md.tok_sep = constrain->tok_sep;
    md.logprob = constrain->logprob; md.dead_end = constrain->dead_end; md.open_end = constrain->open_end;
    e.have = constrain->logprob && constrain->dead_end && constrain->open_end;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

extern "C" size_t ff_decode_sequence_constrained_sample_workspace_bytes(const ff_model* m, const ff_decode_params* p, int num_samples) {
  if (num_samples < 1 || num_samples > 64 || !sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::DRAW, Mode::SEQUENCE, true, num_samples));
}

// R draws per wireframe of the single-sequence decode (model.py:161-167, 191, 193-210) from the row the face-loop rule leaves.
extern "C" int ff_decode_sequence_constrained_sample(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sequence_constrain_sample_params* cs, ff_stream_t stream) {
  Entry e{"ff_decode_sequence_constrained_sample", nullptr, "constrain sample", "ff_decode_constrained_sample",
                "uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict"};
  Mode md(Mode::DRAW, Mode::SEQUENCE, true);
  if ((e.given = cs != nullptr)) {
    take_draw(md, cs);
    take_rule(md, cs);
    md.tok_sep = cs->tok_sep;
    md.dead_end = cs->dead_end; md.open_end = cs->open_end;
    md.predict_logprob = cs->predict_logprob; md.predict_dead_end = cs->predict_dead_end; md.predict_open_end = cs->predict_open_end;
    e.have = cs->uniforms && cs->samples && cs->logprob && cs->scores && cs->dead_end && cs->open_end && cs->predict_logprob &&
              cs->predict_dead_end && cs->predict_open_end;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

// (nothing of a closure look-ahead lies in the workspace: the tables are operands)
extern "C" size_t ff_sequence_decode_constrained_ahead_workspace_bytes(const ff_model* m, const ff_decode_params* p) {
  if (!sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::ARGMAX, Mode::SEQUENCE, true));
}

// The greedy single-sequence decode (model.py:161-167, 191, 193-210) under the face-loop rule with a closure look-ahead.
extern "C" int ff_sequence_decode_constrained_ahead(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sequence_constrain_ahead_params* ahead, ff_stream_t stream) {
  Entry e{"ff_sequence_decode_constrained_ahead", nullptr, "look-ahead", "ff_decode_constrained_ahead",
          "logprob, dead_end, open_end and predict", 2};
  Mode md(Mode::ARGMAX, Mode::SEQUENCE, true);
  if ((e.given = ahead != nullptr)) {
    take_rule(md, ahead);
    take_ahead(md, ahead->form, ahead, ahead->form == 1 ? ahead->close_dist : nullptr);
    md.tok_sep = ahead->tok_sep;
    md.logprob = ahead->logprob; md.dead_end = ahead->dead_end; md.open_end = ahead->open_end;
    e.have = ahead->logprob && ahead->dead_end && ahead->open_end;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

extern "C" size_t ff_sequence_decode_constrained_sample_ahead_workspace_bytes(const ff_model* m, const ff_decode_params* p,
                                                                              int num_samples) {
  if (num_samples < 1 || num_samples > 64 || !sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::DRAW, Mode::SEQUENCE, true, num_samples));
}

// R draws per wireframe of the single-sequence decode (model.py:161-167, 191, 193-210) from the row the face-loop rule with a
// closure look-ahead leaves.
extern "C" int ff_sequence_decode_constrained_sample_ahead(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sequence_constrain_sample_ahead_params* cs, ff_stream_t stream) {
  Entry e{"ff_sequence_decode_constrained_sample_ahead", nullptr, "look-ahead sample", "ff_decode_constrained_sample",
          "uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict", 2};
  Mode md(Mode::DRAW, Mode::SEQUENCE, true);
  if ((e.given = cs != nullptr)) {
    take_draw(md, cs);
    take_rule(md, cs);
    take_ahead(md, cs->form, cs, cs->form == 1 ? cs->close_dist : nullptr);
    md.tok_sep = cs->tok_sep;
    md.dead_end = cs->dead_end; md.open_end = cs->open_end;
    md.predict_logprob = cs->predict_logprob; md.predict_dead_end = cs->predict_dead_end; md.predict_open_end = cs->predict_open_end;
    e.have = cs->uniforms && cs->samples && cs->logprob && cs->scores && cs->dead_end && cs->open_end && cs->predict_logprob &&
              cs->predict_dead_end && cs->predict_open_end;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

extern "C" size_t ff_decode_sequence_constrained_beam_workspace_bytes(const ff_model* m, const ff_decode_params* p, int width) {
  if (width < 1 || width > 8 || !sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::BEAM, Mode::SEQUENCE, true, width));
}

// W beams per wireframe of the single-sequence decode (model.py:161-167, 191, 193-210) over the rows the face-loop rule leaves.
extern "C" int ff_decode_sequence_constrained_beam(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sequence_constrain_beam_params* beam, ff_stream_t stream) {
  Entry e{"ff_decode_sequence_constrained_beam", nullptr, "constrain beam", "ff_decode_constrained_beam",
                "beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict"};
  Mode md(Mode::BEAM, Mode::SEQUENCE, true);
  if ((e.given = beam != nullptr)) {
    take_beam(md, beam);
    take_rule(md, beam);
    md.tok_sep = beam->tok_sep; md.stop_best = beam->stop_best;
    md.finished = beam->finished; md.beam_dead_end = beam->beam_dead_end; md.beam_open_end = beam->beam_open_end;
    md.dead_end = beam->dead_end; md.open_end = beam->open_end;
    e.have = beam->beams && beam->scores && beam->finished && beam->beam_dead_end && beam->beam_open_end && beam->dead_end &&
              beam->open_end;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

// (nothing of a closure look-ahead lies in the workspace: the tables are operands)
extern "C" size_t ff_sequence_decode_constrained_beam_ahead_workspace_bytes(const ff_model* m, const ff_decode_params* p, int width) {
  if (width < 1 || width > 8 || !sequence_query_ok(p)) return 0;
  return decode_workspace_bytes(m, p, nullptr, Mode(Mode::BEAM, Mode::SEQUENCE, true, width));
}

// W beams per wireframe of the single-sequence decode (model.py:161-167, 191, 193-210) over the rows the face-loop rule with a
// closure look-ahead leaves.
extern "C" int ff_sequence_decode_constrained_beam_ahead(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, int64_t* predict, int* steps_done, int* step_counts, float* trace_logits,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_sequence_constrain_beam_ahead_params* beam, ff_stream_t stream) {
  Entry e{"ff_sequence_decode_constrained_beam_ahead", nullptr, "look-ahead beam", "ff_decode_constrained_beam_ahead",
          "beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict", 2};
  Mode md(Mode::BEAM, Mode::SEQUENCE, true);
  if ((e.given = beam != nullptr)) {
    take_beam(md, beam);
    take_rule(md, beam);
    take_ahead(md, beam->form, beam, beam->form == 1 ? beam->close_dist : nullptr);
    md.tok_sep = beam->tok_sep; md.stop_best = beam->stop_best;
    md.finished = beam->finished; md.beam_dead_end = beam->beam_dead_end; md.beam_open_end = beam->beam_open_end;
    md.dead_end = beam->dead_end; md.open_end = beam->open_end;
    e.have = beam->beams && beam->scores && beam->finished && beam->beam_dead_end && beam->beam_open_end && beam->dead_end &&
              beam->open_end;
  }
  return run_entry(e, md, m, p, no_refused, FF_SEQ_ARGS);
}

extern "C" size_t ff_decode_constrained_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host) {
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::ARGMAX, Mode::LOOP, false));
}

// (ff_decode_constrained, _ahead and _exact: the parameters and the required outputs the three share)
template <typename Q>
static bool take_constrain(Entry& e, Mode& md, const Q* q, const char* op) {
  if (!(e.given = q != nullptr)) return false;
  take_rule(md, q);
  md.op = op; md.logprob = q->logprob; md.dead_end = q->dead_end;
  e.have = q->logprob && q->dead_end;
  return true;
}

extern "C" int ff_decode_constrained(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_constrain_params* constrain, ff_stream_t stream) {
  Entry e{"ff_decode_constrained", "the constrained decode is", "constrain", nullptr, "logprob and dead_end"};
  Mode md(Mode::ARGMAX, Mode::LOOP, false);
  take_constrain(e, md, constrain, "ff_pointer_constrained");
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

extern "C" size_t ff_decode_constrained_ahead_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host) {
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::ARGMAX, Mode::LOOP, false));
}

extern "C" int ff_decode_constrained_ahead(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_constrain_ahead_params* ahead, ff_stream_t stream) {
  Entry e{"ff_decode_constrained_ahead", "the constrained decode with look-ahead is", "look-ahead", nullptr, "logprob and dead_end"};
  Mode md(Mode::ARGMAX, Mode::LOOP, false);
  if (take_constrain(e, md, ahead, "ff_pointer_constrained_ahead")) take_ahead(md, 1, ahead, ahead->close_dist);
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

extern "C" size_t ff_decode_constrained_exact_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host) {
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::ARGMAX, Mode::LOOP, false));
}

extern "C" int ff_decode_constrained_exact(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_constrain_exact_params* exact, ff_stream_t stream) {
  Entry e{"ff_decode_constrained_exact", "the constrained decode with exact look-ahead is", "exact look-ahead", nullptr,
                "logprob and dead_end"};
  Mode md(Mode::ARGMAX, Mode::LOOP, false);
  if (take_constrain(e, md, exact, "ff_pointer_constrained_exact")) take_ahead(md, 2, exact, nullptr);
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

extern "C" size_t ff_decode_constrained_beam_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host,
                                                             int width) {
  if (width < 1 || width > 8) return 0;
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::BEAM, Mode::LOOP, false, width));
}

// (ff_decode_constrained_beam and _beam_ahead: the parameters and the required outputs the two share)
template <typename Q>
static bool take_constrain_beam(Entry& e, Mode& md, const Q* q, const char* op) {
  if (!(e.given = q != nullptr)) return false;
  take_beam(md, q);
  take_rule(md, q);
  md.op = op; md.dead_end = q->dead_end;
  e.have = q->beams && q->scores && q->dead_end;
  return true;
}

extern "C" int ff_decode_constrained_beam(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_constrain_beam_params* beam, ff_stream_t stream) {
  Entry e{"ff_decode_constrained_beam", "the constrained beam decode is", "beam", nullptr, "beams, scores and dead_end"};
  Mode md(Mode::BEAM, Mode::LOOP, false);
  take_constrain_beam(e, md, beam, "ff_beam_constrained_select");
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

extern "C" size_t ff_decode_constrained_beam_ahead_workspace_bytes(const ff_model* m, const ff_decode_params* p,
                                                                   const int* num_input_host, int width) {
  if (width < 1 || width > 8) return 0;
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::BEAM, Mode::LOOP, false, width));
}

extern "C" int ff_decode_constrained_beam_ahead(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_constrain_beam_ahead_params* beam, ff_stream_t stream) {
  Entry e{"ff_decode_constrained_beam_ahead", "the constrained beam decode with look-ahead is", "beam", nullptr,
                "beams, scores and dead_end", 1};
  Mode md(Mode::BEAM, Mode::LOOP, false);
  if (take_constrain_beam(e, md, beam, "ff_beam_constrained_select_ahead")) take_ahead(md, beam->lookahead, beam, beam->close_dist);
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

extern "C" size_t ff_decode_constrained_sample_workspace_bytes(const ff_model* m, const ff_decode_params* p, const int* num_input_host,
                                                               int num_samples) {
  if (num_samples < 1 || num_samples > 64) return 0;
  return decode_workspace_bytes(m, p, num_input_host, Mode(Mode::DRAW, Mode::LOOP, false, num_samples));
}

extern "C" int ff_decode_constrained_sample(const ff_model* m, const ff_decode_params* p, const float* memory,
    const unsigned char* mask, const int* kv_len, const int* num_input, const int* num_input_host, const unsigned char* extra_mask,
    int64_t* predict, int* steps_done, int* step_counts, float* pointer_out, float* trace_logits, float* trace_best, float* trace_second,
    int* seq_of_row, void* workspace, size_t workspace_bytes, const ff_constrain_sample_params* cs, ff_stream_t stream) {
  Entry e{"ff_decode_constrained_sample", "the constrained sampled decode is", "constrained sample", nullptr,
                "uniforms, samples, logprob, scores and dead_end", 0};
  Mode md(Mode::DRAW, Mode::LOOP, false);
  if ((e.given = cs != nullptr)) {
    take_draw(md, cs);
    take_rule(md, cs);
    take_ahead(md, cs->lookahead, cs, cs->close_dist);
    md.op = "ff_pointer_constrained_sample";
    md.dead_end = cs->dead_end; md.predict_logprob = cs->predict_logprob; md.predict_dead_end = cs->predict_dead_end;
    e.have = cs->uniforms && cs->samples && cs->logprob && cs->scores && cs->dead_end;
  }
  return run_entry(e, md, m, p, FF_PAR_REFUSED, FF_PAR_ARGS);
}

#undef FF_PAR_ARGS
#undef FF_SEQ_ARGS
#undef FF_PAR_REFUSED

namespace {
int run_decode(const ff_model* m, const ff_decode_params* p, const DecodeIO& io, void* workspace, size_t workspace_bytes,
               const Mode& mode) {
  DecodeRun r;
  r.mode = mode;
  FF_RETURN_IF(r.validate(m, p, io, workspace));
  FF_RETURN_IF(r.bind_chunks(workspace, workspace_bytes));
  FF_RETURN_IF(ff_gemm_prepare_stream(r.io.main_st));
  std::mutex* busy = pool_busy_mutex();
  FF_CHECK_ARG(busy, "ff_decode: no current device");
  std::lock_guard<std::mutex> one_decode_per_device(*busy);
  FF_RETURN_IF(r.bind_streams());
  FF_RETURN_IF(r.init_retirement());
  int rc = FF_OK;
  if (mode.pick == Mode::FORCED) {   // (no row to score: the start tokens are packed, no decoder launch is made)
    rc = r.forced_tokens();
    if (rc == FF_OK && r.forced_steps > 0) rc = r.prologue();
    if (rc == FF_OK) rc = r.forced_loop();
    if (rc == FF_OK) rc = r.forced_epilogue();
  } else {
    rc = r.prologue();
    if (rc == FF_OK) rc = r.greedy_loop();
    if (rc == FF_OK) rc = r.epilogue();
  }
  if (rc != FF_OK) r.drain();
  return rc;
}
}  // namespace
