"""Torch-tensor front end of the C-ABI kernels (device memory + stream plumbing only).

Every function takes fp32 CUDA(ROCm) tensors, hands raw pointers to libfaceformer_hip.so on the
current torch stream and returns torch tensors.  CPU tensors are rejected: there is no fallback.
"""
import ctypes as C

import torch

from . import lib as _L


import functools


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _on_tensor_device(fn):
    """Run `fn` with the CUDA device of its first device tensor argument made current: the C side launches
    on the current HIP device and on torch's current stream OF THAT DEVICE, so a tensor on cuda:1 must
    never be handed over while cuda:0 is current.  Tensors on different devices are rejected."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        devs = {a.device for a in list(args) + list(kwargs.values()) if torch.is_tensor(a) and a.is_cuda}
        if len(devs) > 1:
            raise _L.HipExtensionError("%s: tensors on different devices %s" % (fn.__name__, sorted(map(str, devs))))
        if not devs:
            return fn(*args, **kwargs)   # the op's own checks reject CPU tensors
        with torch.cuda.device(next(iter(devs))):
            return fn(*args, **kwargs)
    return wrapper


def _dev(t, name, dtype=torch.float32):
    if not torch.is_tensor(t):
        raise TypeError("%s must be a tensor" % name)
    if not t.is_cuda:
        raise _L.HipExtensionError(
            "%s is on %s: the faceformer_amd decode path only runs on a ROCm device "
            "(no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t


def _rows(t, name):
    """2-D row-major view [rows, cols] with unit inner stride; returns (tensor, ld)."""
    _dev(t, name)
    if t.dim() != 2:
        raise ValueError("%s must be 2-D" % name)
    if t.stride(1) != 1 and t.size(1) != 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.size(0) > 1 else max(t.size(1), t.stride(0)))


def _p(t):
    return None if t is None else t.data_ptr()


@_on_tensor_device
def layernorm(x, gamma, beta, eps=1e-5, pos=None, pos_div=1, pos_mod=1, want_y=True):
    """(y, ypos): y = LN(x); ypos = y + pos[(row // pos_div) % pos_mod] (None when pos is None)."""
    x, ldx = _rows(x, "x")
    rows, E = x.shape
    y = torch.empty((rows, E), device=x.device, dtype=torch.float32) if want_y else None
    ypos = torch.empty((rows, E), device=x.device, dtype=torch.float32) if pos is not None else None
    if pos is not None:
        pos, ldpos = _rows(pos, "pos")
    else:
        ldpos = 0
    lib = _L.load()
    _L.check(lib.ff_layernorm(_p(x), ldx, _p(_dev(gamma, "gamma")), _p(_dev(beta, "beta")), eps,
                              _p(y), E, _p(ypos), E, _p(pos), ldpos, pos_div, pos_mod, rows, E,
                              _stream()), "ff_layernorm")
    return y, ypos


@_on_tensor_device
def add_pos(x, pos, pos_div=1, pos_mod=1):
    x, ldx = _rows(x, "x")
    pos, ldpos = _rows(pos, "pos")
    out = torch.empty_like(x, memory_format=torch.contiguous_format)
    _L.check(_L.load().ff_add_pos(_p(x), ldx, _p(pos), ldpos, pos_div, pos_mod, _p(out), x.size(1),
                                  x.size(0), x.size(1), _stream()), "ff_add_pos")
    return out


@_on_tensor_device
def gelu_(x):
    """In-place exact (erf) GELU of a 2-D row tensor; returns x."""
    x2, ldx = _rows(x, "x")
    if x2.data_ptr() != x.data_ptr():
        raise ValueError("gelu_ works in place: x needs a unit inner stride")
    _L.check(_L.load().ff_gelu(_p(x2), ldx, x2.size(0), x2.size(1), _stream()), "ff_gelu")
    return x


@_on_tensor_device
def linear(x, weight, bias=None, act=0, residual=None, x2=None, n_split=0, tile=0, out=None):
    """out = act(xsel @ weight.T + bias) + residual on the f32 matrix cores (F.linear layout)."""
    x, lda = _rows(x, "x")
    weight, ldw = _rows(weight, "weight")
    M, K = x.shape
    N = weight.size(0)
    if weight.size(1) != K:
        raise ValueError("linear: x is [%d,%d] but weight is [%d,%d]" % (M, K, N, weight.size(1)))
    if x2 is not None:
        x2, lda2 = _rows(x2, "x2")
        if x2.shape != x.shape or lda2 != lda:
            raise ValueError("linear: x2 must match x")
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    out, ldc = _rows(out, "out")
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(residual, "residual")
    if bias is not None:
        _dev(bias, "bias")
    _L.check(_L.load().ff_gemm_f32(_p(x), lda, _p(x2), n_split, _p(weight), ldw, _p(bias),
                                   _p(residual), ldr, _p(out), ldc, M, N, K, act, tile, _stream()),
             "ff_gemm_f32")
    return out


def _ln_desc(x, lda, bias, act, residual, out, ldc, M, N, K, stats_in, eps, row_table, row_div, row_cols, want_stats):
    """(d, stats, keep): the GemmLnDesc that linear_ln and linear_x3_ln share (everything but the weight), the statistics tensor it
    fills (or None) and the tensors behind its raw pointers, which the caller keeps alive until the launch is enqueued."""
    d = _L.GemmLnDesc()
    d.A, d.lda, d.bias = _p(x), lda, _p(bias)
    if residual is not None:
        residual, ldr = _rows(residual, "residual")
        d.residual, d.ldr = _p(residual), ldr
    d.C, d.ldc, d.M, d.N, d.K, d.act = _p(out), ldc, M, N, K, act
    if stats_in is not None:
        _dev(stats_in, "stats_in")
        stats_in = stats_in.contiguous()
        d.ln_stats_in, d.ln_nseg, d.ln_eps = _p(stats_in), stats_in.size(1), eps
    if row_table is not None:
        row_table, ldt = _rows(row_table, "row_table")
        d.row_table, d.ld_row_table, d.row_div, d.row_cols = _p(row_table), ldt, row_div, row_cols or row_table.size(1)
    stats = None
    if want_stats:
        stats = torch.full((M, N // 32, 2), float("nan"), device=x.device, dtype=torch.float32)
        d.ln_stats_out = _p(stats)
    return d, stats, (residual, stats_in, row_table)   # (the contiguous copies made above: the caller holds them over the launch)


@_on_tensor_device
def linear_ln(x, weight, bias=None, act=0, residual=None, stats_in=None, eps=1e-5, row_table=None, row_div=1,
              row_cols=0, want_stats=False, tile=0, out=None):
    """ff_gemm_f32_ln: out = act(z @ weight.T + bias [+ row_table[row // row_div]]) [+ residual], where z = x, or --
    with `stats_in` ([M, K/32, 2] segment statistics of x's rows) -- the row-normalised x.  `want_stats` also
    returns the [M, N/32, 2] (mean, M2) segment statistics of `out` for the next LayerNorm."""
    x, lda = _rows(x, "x")
    weight, ldw = _rows(weight, "weight")
    M, K = x.shape
    N = weight.size(0)
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    out, ldc = _rows(out, "out")
    d, stats, keep = _ln_desc(x, lda, bias, act, residual, out, ldc, M, N, K, stats_in, eps, row_table, row_div, row_cols, want_stats)
    d.W, d.ldw, d.tile = _p(weight), ldw, tile
    _L.check(_L.load().ff_gemm_f32_ln(C.byref(d), _stream()), "ff_gemm_f32_ln")
    del keep
    return (out, stats) if want_stats else out


@_on_tensor_device
def linear_x3_ln(x, planes, bias=None, act=0, residual=None, stats_in=None, eps=1e-5, row_table=None, row_div=1,
                 row_cols=0, want_stats=False, out=None, row0=0, rows=0, colsum=None):
    """ff_gemm_x3_ln: linear_ln() on the bf16 matrix cores with fp32 accuracy; `planes` = split_weight(folded weight) (fp16 planes:
    ff_gemm_x2h_ln, or ff_gemm_h1_ln -- one fp16 product -- for the one plane of kind "fp16").
    row0 / rows: use only weight rows [row0, row0 + rows) of the planes (bias, table and output then have `rows` columns).
    colsum ([plane rows] row sums of the folded weight): apply the normalisation in the epilogue (plain K loop)."""
    _check_planes(planes, "planes")
    plane_rows, K = planes.size(2), planes.size(1) * 16
    N = rows or plane_rows
    x, lda = _rows(x, "x")
    M = x.size(0)
    if x.size(1) != K:
        raise ValueError("linear_x3_ln: x is [%d,%d] but the weight is [%d,%d]" % (M, x.size(1), N, K))
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    out, ldc = _rows(out, "out")
    d, stats, keep = _ln_desc(x, lda, bias, act, residual, out, ldc, M, N, K, stats_in, eps, row_table, row_div, row_cols, want_stats)
    if colsum is not None:
        _dev(colsum, "colsum")
    lib = _L.load()
    fn, who = _split_fn(planes, lib, "_ln")
    _L.check(fn(C.byref(d), planes.data_ptr(), plane_rows, row0, _p(colsum), _stream()), who)
    del keep
    return (out, stats) if want_stats else out


def set_x3_tuning(shape=0):
    """Launch shape of the 3 x bf16 kernel: 0 the default (whole tiles), 1 whole tiles, 2 equal K-unit ranges."""
    _L.check(_L.load().ff_set_x3_tuning(int(shape)), "ff_set_x3_tuning")


@_on_tensor_device
def fold_layernorm_linear(weight, bias, gamma, beta, pos=None, pos_cols=0):
    """(Wf, bf, P) of ff_fold_layernorm_linear: LN(x) @ weight.T + bias == z @ Wf.T + bf with z the normalised x;
    P = pos @ weight[:pos_cols].T."""
    weight, ldw = _rows(weight, "weight")
    N, K = weight.shape
    Wf = torch.empty((N, K), device=weight.device, dtype=torch.float32)
    bf = torch.empty((N,), device=weight.device, dtype=torch.float32)
    P, ldpos = None, 0
    if pos is not None:
        pos, ldpos = _rows(pos, "pos")
        P = torch.empty((pos.size(0), pos_cols), device=weight.device, dtype=torch.float32)
    _L.check(_L.load().ff_fold_layernorm_linear(_p(weight), ldw, N, K, _p(bias), _p(gamma), _p(beta), _p(pos), ldpos,
                                                pos.size(0) if pos is not None else 0, pos_cols, _p(Wf), _p(bf), _p(P),
                                                _stream()), "ff_fold_layernorm_linear")
    return Wf, bf, P


@_on_tensor_device
def split_kv(k, v, num_groups, num_heads, nk, k_group_stride, k_stride):
    """fp16 planes of K | V for the 2 x fp16 attention kernel (ff_attention_split_kv): a uint8 tensor of
    ff_attention_planes_bytes(num_groups, num_heads) bytes; 1 <= nk <= 288."""
    _dev(k, "k"), _dev(v, "v")
    lib = _L.load()
    planes = torch.empty(int(lib.ff_attention_planes_bytes(num_groups, num_heads)), device=k.device, dtype=torch.uint8)
    _L.check(lib.ff_attention_split_kv(_p(k), _p(v), k.stride(0), v.stride(0), num_groups, num_heads, nk, k_group_stride, k_stride,
                                       planes.data_ptr(), _stream()), "ff_attention_split_kv")
    return planes


_attn_algo = 0      # what set_attention_algo() last set: 4 makes attention() split K | V itself (tests of the 2 x fp16 kernel)


@_on_tensor_device
def attention(q, k, v, num_groups, num_heads, nq, nk, q_group_stride, q_inner, q_outer_stride,
              k_group_stride, k_stride, kv_len=None, key_mask=None, causal=False, scale=0.125,
              out=None, kv_planes=None, kv_terms=0):
    """Raw descriptor-level attention (see ff_attn_desc).  q/k/v/out are 2-D row tensors (views
    into wider buffers are fine: the leading dimension is taken from stride(0)).  kv_planes: split_kv(k, v, ...) of the same
    K | V -- eligible launches then run on the fp16 matrix cores; kv_terms=1 uses their first planes only (one fp16 term per operand,
    the split kind "fp16")."""
    _dev(q, "q"), _dev(k, "k"), _dev(v, "v")
    if kv_planes is None and _attn_algo == 4 and 0 < nk <= 288 and not causal:
        kv_planes = split_kv(k, v, num_groups, num_heads, nk, k_group_stride, k_stride)
    if out is None:
        out = torch.empty((q.size(0), num_heads * _L.FF_HEAD_DIM), device=q.device, dtype=torch.float32)
    d = _L.AttnDesc()
    d.q, d.k, d.v, d.o = _p(q), _p(k), _p(v), _p(out)
    d.ldq, d.ldk, d.ldv, d.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    d.num_groups, d.num_heads, d.nq, d.nk = num_groups, num_heads, nq, nk
    d.q_group_stride, d.q_inner, d.q_outer_stride = q_group_stride, q_inner, q_outer_stride
    d.k_group_stride, d.k_stride = k_group_stride, k_stride
    if kv_len is not None:
        _dev(kv_len, "kv_len", torch.int32)
    if key_mask is not None:
        _dev(key_mask, "key_mask", torch.uint8)
        d.mask_stride = key_mask.stride(0)
    d.kv_len, d.key_mask = _p(kv_len), _p(key_mask)
    d.causal = 1 if causal else 0
    d.scale = scale
    d.kv_planes = _p(kv_planes)
    d.kv_terms = kv_terms
    _L.check(_L.load().ff_attention(C.byref(d), _stream()), "ff_attention")
    return out


@_on_tensor_device
def attention_general(q, k, v, num_groups, num_heads, head_dim, nq, nk, q_group_stride, q_inner, q_outer_stride,
                      k_group_stride, k_stride, kv_len=None, key_mask=None, causal=False, attn_bias=None, attn_mask=None,
                      scale=None, out=None):
    """ff_attention_general: any head width, torch's `attn_mask` forms.  attn_bias: fp32 [nq, nk] or [num_groups*num_heads, nq, nk]
    (added to the scores); attn_mask: uint8 / bool of the same shapes (non-zero = key removed).  A query without keys -> NaN (torch)."""
    _dev(q, "q"), _dev(k, "k"), _dev(v, "v")
    if out is None:
        out = torch.empty((q.size(0), num_heads * head_dim), device=q.device, dtype=torch.float32)
    d = _L.AttnGeneralDesc()
    d.q, d.k, d.v, d.o = _p(q), _p(k), _p(v), _p(out)
    d.ldq, d.ldk, d.ldv, d.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    d.num_groups, d.num_heads, d.head_dim, d.nq, d.nk = num_groups, num_heads, head_dim, nq, nk
    d.q_group_stride, d.q_inner, d.q_outer_stride = q_group_stride, q_inner, q_outer_stride
    d.k_group_stride, d.k_stride = k_group_stride, k_stride
    if kv_len is not None:
        _dev(kv_len, "kv_len", torch.int32)
    if key_mask is not None:
        _dev(key_mask, "key_mask", torch.uint8)
        d.mask_stride = key_mask.stride(0)
    d.kv_len, d.key_mask = _p(kv_len), _p(key_mask)
    d.causal = 1 if causal else 0
    keep = []
    for name, m, dt in (("attn_bias", attn_bias, torch.float32), ("attn_mask", attn_mask, torch.uint8)):
        if m is None:
            continue
        if m.dtype == torch.bool and dt == torch.uint8:
            m = m.to(torch.uint8)
        _dev(m, name, dt)
        if m.dim() == 2:
            want = (nq, nk)
        elif m.dim() == 3:
            want = (num_groups * num_heads, nq, nk)
        else:
            raise ValueError("%s must be 2-D [nq, nk] or 3-D [num_groups*num_heads, nq, nk]" % name)
        if tuple(m.shape) != want:
            raise ValueError("%s must have shape %s, got %s" % (name, want, tuple(m.shape)))
        m = m.contiguous()
        keep.append(m)
        ld, bs = nk, (nq * nk if m.dim() == 3 else 0)
        if (d.attn_bias or d.attn_mask) and (d.attn_ld != ld or d.attn_batch_stride != bs):
            # both given with different batching: expand the shared one (rare; keeps the descriptor to one addressing)
            raise ValueError("attn_bias and attn_mask must both be 2-D or both 3-D")
        d.attn_ld, d.attn_batch_stride = ld, bs
        setattr(d, name, m.data_ptr())
    d.scale = float(head_dim) ** -0.5 if scale is None else scale
    _L.check(_L.load().ff_attention_general(C.byref(d), _stream()), "ff_attention_general")
    del keep
    return out


@_on_tensor_device
def attention_prefix_fold(x, stats, qt, Bc, t, E, H, eps=1e-5, scale=0.125, out=None):
    """ff_attention_prefix_fold: u [Bc, H*E] = sum_j softmax_j(scale (qt . x^_j + c_j)) x^_j over the first t positions of the
    position-major rows x ([>= t*Bc, E], row j*Bc + b) with segment statistics stats ([>= t*Bc, E/32, 2]); qt [Bc, H, E + t] holds
    qt | c.  The tensors are handed over as they are (contiguous; views into larger buffers are fine)."""
    _dev(x, "x"), _dev(stats, "stats"), _dev(qt, "qt")
    for name, a in (("x", x), ("stats", stats), ("qt", qt)):
        if not a.is_contiguous():
            raise ValueError("attention_prefix_fold: %s must be contiguous" % name)
    if out is None:
        out = torch.empty((Bc, H * E), device=x.device, dtype=torch.float32)
    _dev(out, "out")
    _L.check(_L.load().ff_attention_prefix_fold(_p(x), _p(stats), eps, _p(qt), scale, Bc, t, E, H, _p(out), _stream()),
             "ff_attention_prefix_fold")
    return out


@_on_tensor_device
def pointer_argmax(p, memory, mask=None, kv_len=None, extra_mask=None, seqs_per_group=1,
                   want_logits=False, want_rows=False, counters=None, ge_bound=0, eq_value=0, want_logprob=False):
    """select_next: returns dict(next, best, second, [logits], [rows], [logprob]).
    want_logprob: also log_softmax(masked logits)[next] per sequence (ff_pointer_argmax_lp); the other outputs do not change."""
    p, ldp = _rows(p, "p")
    _dev(memory, "memory")
    if memory.dim() != 3 or not memory.is_contiguous():
        raise ValueError("memory must be a contiguous [N, S, E] tensor")
    B, E = p.shape
    S = memory.size(1)
    dev = p.device
    nxt = torch.empty(B, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.float32)
    second = torch.empty(B, device=dev, dtype=torch.float32)
    logits = torch.empty((B, S), device=dev, dtype=torch.float32) if want_logits else None
    rows = torch.empty((B, E), device=dev, dtype=torch.float32) if want_rows else None
    if mask is not None:
        _dev(mask, "mask", torch.uint8)
    if kv_len is not None:
        _dev(kv_len, "kv_len", torch.int32)
    ldextra = 0
    if extra_mask is not None:
        _dev(extra_mask, "extra_mask", torch.uint8)
        ldextra = extra_mask.stride(0)
    cge = ceq = None
    if counters is not None:
        _dev(counters, "counters", torch.int32)
        cge, ceq = counters.data_ptr(), counters.data_ptr() + 4
    args = (_p(p), ldp, _p(memory), S, E, _p(mask), _p(kv_len), _p(extra_mask), ldextra, B,
            seqs_per_group, _p(nxt), _p(best), _p(second), _p(logits), S, _p(rows), E,
            cge, ge_bound, ceq, eq_value)
    out = {"next": nxt, "best": best, "second": second}
    if want_logprob:
        out["logprob"] = torch.empty(B, device=dev, dtype=torch.float32)
        _L.check(_L.load().ff_pointer_argmax_lp(*args, _p(out["logprob"]), _stream()), "ff_pointer_argmax_lp")
    else:
        _L.check(_L.load().ff_pointer_argmax(*args, _stream()), "ff_pointer_argmax")
    if want_logits:
        out["logits"] = logits
    if want_rows:
        out["rows"] = rows
    return out


BEAM_MAX_WIDTH = 8


@_on_tensor_device
def beam_select(logits, scores, fin, width, groups_per_wireframe=None, mask=None, kv_len=None, hist=None, t=0,
                term_range=(1, 4), memory=None, want_rows=False, counter=None, ge_bound=0):
    """One beam-search step of every group (ff_beam_select).  logits [G * width, S] fp32 raw dot products (masked IN PLACE),
    scores [G * width] fp32 (-inf: empty beam) and fin [G * width] int32 (nonzero: finished) are the state before the step;
    hist (optional) [t + 1, G * width] int32 token history, permuted in place, position t written.  Returns dict(parent, next,
    scores, fin, [rows]): the new beams in rank order, best first."""
    return _beam_select("ff_beam_select", ge_bound, logits, scores, fin, width, groups_per_wireframe, mask, kv_len, hist, t, term_range,
                        memory, want_rows, counter)


@_on_tensor_device
def beam_sequence_select(logits, scores, fin, width, groups_per_wireframe=None, mask=None, kv_len=None, hist=None, t=0,
                         term_range=(3, 4), memory=None, want_rows=False, counter=None, stop_best=False):
    """One beam-search step of the single-sequence decode (ff_beam_sequence_select): beam_select's operands,
    selection and outputs; `counter` (int32, one element) += the non-empty beams UNFINISHED AFTER the step -- or, with stop_best,
    the groups whose rank 0 is unfinished after it -- instead of the kept candidates with a token >= ge_bound.  term_range =
    [EOS, EOS + 1)."""
    if not int(term_range[0]) < int(term_range[1]):
        raise ValueError("term_range must be (lo, hi) with lo < hi")
    return _beam_select("ff_beam_sequence_select", int(bool(stop_best)), logits, scores, fin, width, groups_per_wireframe, mask, kv_len,
                        hist, t, term_range, memory, want_rows, counter)


def _beam_select(entry, last, logits, scores, fin, width, groups_per_wireframe, mask, kv_len, hist, t, term_range, memory, want_rows,
                 counter):
    """The two selection entries' common call; `last`: the integer before the stream, ge_bound or stop_best."""
    _dev(logits, "logits"), _dev(scores, "scores"), _dev(fin, "fin", torch.int32)
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be a 2-D tensor with unit inner stride")
    B, S = logits.shape
    if not 1 <= width <= BEAM_MAX_WIDTH or width > S or B % width:
        raise ValueError("beam width %d: must be in 1..%d, at most S = %d, and divide the %d rows" % (width, BEAM_MAX_WIDTH, S, B))
    G = B // width
    gpw = G if groups_per_wireframe is None else int(groups_per_wireframe)
    dev = logits.device
    if mask is not None:
        _dev(mask, "mask", torch.uint8)
    if kv_len is not None:
        _dev(kv_len, "kv_len", torch.int32)
    ldhist = 0
    if hist is not None:
        _dev(hist, "hist", torch.int32)
        if hist.dim() != 2 or hist.size(0) < t + 1 or hist.size(1) < B or hist.stride(1) != 1:
            raise ValueError("hist must be [>= t + 1, >= G * width] int32")
        ldhist = hist.stride(0)
    out = {"parent": torch.empty(B, device=dev, dtype=torch.int32), "next": torch.empty(B, device=dev, dtype=torch.int32),
           "scores": torch.empty(B, device=dev, dtype=torch.float32), "fin": torch.empty(B, device=dev, dtype=torch.int32)}
    rows, E = None, 0
    if memory is not None:
        _dev(memory, "memory")
        if memory.dim() != 3 or not memory.is_contiguous() or memory.size(1) != S:
            raise ValueError("memory must be a contiguous [N, S, E] tensor")
        E = memory.size(2)
        if want_rows:
            rows = out["rows"] = torch.empty((B, E), device=dev, dtype=torch.float32)
    if counter is not None:
        _dev(counter, "counter", torch.int32)
    _L.check(getattr(_L.load(), entry)(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), G, width, gpw, _p(scores.contiguous()), _p(out["scores"]),
        _p(fin.contiguous()), _p(out["fin"]), _p(hist), ldhist, t, _p(out["parent"]), _p(out["next"]), int(term_range[0]),
        int(term_range[1]), _p(memory), E, _p(rows), E, _p(counter), last, _stream()), entry)
    return out


@_on_tensor_device
def beam_reorder(rows_a, parent, width, rows_b=None):
    """rows_a [npos, R, wa] (and rows_b [npos, R, wb]) fp32, in place: row (j, g * width + k) <- row (j, g * width + parent[g *
    width + k]) for every position j and group g < len(parent) / width (ff_beam_reorder)."""
    _dev(rows_a, "rows_a"), _dev(parent, "parent", torch.int32)
    if rows_a.dim() != 3 or not rows_a.is_contiguous():
        raise ValueError("rows_a must be a contiguous [npos, rows, width] tensor")
    npos, R, wa = rows_a.shape
    wb = 0
    if rows_b is not None:
        _dev(rows_b, "rows_b")
        if rows_b.dim() != 3 or not rows_b.is_contiguous() or rows_b.shape[:2] != rows_a.shape[:2]:
            raise ValueError("rows_b must be a contiguous [npos, rows, width] tensor with rows_a's positions and rows")
        wb = rows_b.size(2)
    if not 1 <= width <= BEAM_MAX_WIDTH or parent.numel() % width:
        raise ValueError("beam width %d: must be in 1..%d and divide the %d parents" % (width, BEAM_MAX_WIDTH, parent.numel()))
    _L.check(_L.load().ff_beam_reorder(_p(rows_a), wa, _p(rows_b), wb, R, npos, _p(parent.contiguous()), parent.numel() // width,
                                       width, _stream()), "ff_beam_reorder")
    return rows_a


def _step_operands(logits, seqs_per_group, mask, kv_len, memory, want_rows, want_stats, out):
    """The operands the pointer-step ops share (pointer_forced / pointer_sample / pointer_constrained): logits [B, S] with unit
    inner stride; row b belongs to wireframe b // seqs_per_group of mask [W, S] / kv_len [W] / memory [W, S, E]; `rows` [B, E]
    and `stats` [B, E/32, 2] are made on request and put into `out`, which the caller appends to its own outputs.  Returns (B, S, spg, nw, E, rows, stats)."""
    _dev(logits, "logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be a 2-D tensor with unit inner stride")
    B, S = logits.shape
    spg = int(seqs_per_group)
    if spg < 1:
        raise ValueError("seqs_per_group must be positive")
    nw = (B + spg - 1) // spg
    for t, name, dt in ((mask, "mask", torch.uint8), (kv_len, "kv_len", torch.int32)):
        if t is not None:
            _dev(t, name, dt)
            if not t.is_contiguous() or t.size(0) < nw or (name == "mask" and (t.dim() != 2 or t.size(1) != S)):
                raise ValueError("%s must be contiguous and cover %d wireframes of %d keys" % (name, nw, S))
    rows, stats, E = None, None, 0
    if memory is not None:
        _dev(memory, "memory")
        if memory.dim() != 3 or not memory.is_contiguous() or memory.size(1) != S or memory.size(0) < nw:
            raise ValueError("memory must be a contiguous [>= %d, %d, E] tensor" % (nw, S))
        E = memory.size(2)
    if want_rows or want_stats:
        if memory is None:
            raise ValueError("rows / stats need memory")
        rows = out["rows"] = torch.empty((B, E), device=logits.device, dtype=torch.float32)
        if want_stats:
            if E % 32:
                raise ValueError("stats need E % 32 == 0")
            stats = out["stats"] = torch.empty((B, E // 32, 2), device=logits.device, dtype=torch.float32)
    return B, S, spg, nw, E, rows, stats


@_on_tensor_device
def pointer_forced(logits, forced, memory=None, mask=None, kv_len=None, seqs_per_group=1, want_rows=False, want_stats=False):
    """One teacher-forced pointer step (ff_pointer_forced).  logits [B, S] fp32 raw dot products (masked IN PLACE as
    the pointer launch masks them), forced [B] int32 tokens in [0, S) (ValueError otherwise; the C entry would clamp them).  Row
    b belongs to wireframe b // seqs_per_group of mask [W, S] / kv_len [W] / memory [W, S, E].  Returns dict(logprob [B] fp32:
    log_softmax(masked row)[forced], saturated at -FLT_MAX; greedy [B] int32: the row's argmax, lowest index on ties; rank [B]
    int32: keys ranked before the forced one; [rows [B, E]: memory[w, forced]]; [stats [B, E/32, 2]: their LayerNorm segment
    statistics])."""
    _dev(logits, "logits"), _dev(forced, "forced", torch.int32)
    out = {}
    B, S, spg, nw, E, rows, stats = _step_operands(logits, seqs_per_group, mask, kv_len, memory, want_rows, want_stats, out)
    if forced.dim() != 1 or forced.numel() != B:
        raise ValueError("forced must hold one token per row of logits")
    if B and (int(forced.min()) < 0 or int(forced.max()) >= S):
        raise ValueError("forced tokens must lie in [0, %d)" % S)
    dev = logits.device
    out = dict({"logprob": torch.empty(B, device=dev, dtype=torch.float32), "greedy": torch.empty(B, device=dev, dtype=torch.int32),
                "rank": torch.empty(B, device=dev, dtype=torch.int32)}, **out)
    _L.check(_L.load().ff_pointer_forced(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), B, spg, _p(forced.contiguous()), _p(out["logprob"]),
        _p(out["greedy"]), _p(out["rank"]), _p(memory), E, _p(rows), E, _p(stats), _stream()), "ff_pointer_forced")
    return out


@_on_tensor_device
def pointer_sample(logits, uniforms, temperature=1.0, top_k=0, top_p=1.0, row_id=None, fin=None, memory=None, mask=None, kv_len=None,
                   seqs_per_group=1, term_range=(1, 4), want_rows=False, want_stats=False, counter=None, ge_bound=0):
    """One sampling step of the pointer head (ff_pointer_sample).  logits [B, S] fp32 raw dot products (masked IN
    PLACE as the pointer launch masks them; rows of finished sequences are not touched), uniforms [U] fp32; row b reads
    uniforms[row_id[b]] (row_id [B] int32 in [0, U), ValueError otherwise; None: b), fin (optional) [B] int32, nonzero =
    finished: token 0, log-probability 0, no draw.  Row b belongs to wireframe b // seqs_per_group of mask [W, S] / kv_len [W] /
    memory [W, S, E].  Returns dict(next [B] int32: the drawn tokens; logprob [B] fp32: log_softmax(masked row)[next] under the
    model, saturated at -FLT_MAX; fin [B] int32; [rows [B, E]: memory[w, next]]; [stats [B, E/32, 2]])."""
    _dev(logits, "logits"), _dev(uniforms, "uniforms")
    out = {}
    B, S, spg, nw, E, rows, stats = _step_operands(logits, seqs_per_group, mask, kv_len, memory, want_rows, want_stats, out)
    if uniforms.dim() != 1 or not uniforms.is_contiguous() or uniforms.numel() < 1:
        raise ValueError("uniforms must be a contiguous non-empty 1-D tensor")
    U = uniforms.numel()
    t, k, pp = float(temperature), int(top_k), float(top_p)
    if not (0.0 <= t < float("inf")) or k < 0 or not (0.0 < pp <= 1.0):
        raise ValueError("sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]")
    if row_id is not None:
        _dev(row_id, "row_id", torch.int32)
        if row_id.dim() != 1 or row_id.numel() != B or (B and (int(row_id.min()) < 0 or int(row_id.max()) >= U)):
            raise ValueError("row_id must hold one index in [0, %d) per row of logits" % U)
        row_id = row_id.contiguous()
    elif U < B:
        raise ValueError("%d uniforms for %d rows" % (U, B))
    if fin is not None:
        _dev(fin, "fin", torch.int32)
        if fin.dim() != 1 or fin.numel() != B:
            raise ValueError("fin must hold one flag per row of logits")
        fin = fin.contiguous()
    dev = logits.device
    out = dict({"next": torch.empty(B, device=dev, dtype=torch.int32), "logprob": torch.empty(B, device=dev, dtype=torch.float32),
                "fin": torch.empty(B, device=dev, dtype=torch.int32)}, **out)
    if counter is not None:
        _dev(counter, "counter", torch.int32)
    _L.check(_L.load().ff_pointer_sample(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), B, spg, _p(uniforms), U, _p(row_id), _p(fin), t, k, pp,
        int(term_range[0]), int(term_range[1]), _p(out["next"]), _p(out["logprob"]), _p(out["fin"]), _p(memory), E, _p(rows), E,
        _p(stats), _p(counter), int(ge_bound), _stream()), "ff_pointer_sample")
    return out


@_on_tensor_device
def pointer_sequence_sample(logits, uniforms, temperature=1.0, top_k=0, top_p=1.0, row_id=None, fin=None, memory=None, mask=None,
                            kv_len=None, seqs_per_group=1, term_range=(3, 4), want_rows=False, want_stats=False, counter=None):
    """One sampling step of the single-sequence decode (ff_pointer_sequence_sample): pointer_sample's operands,
    selection and outputs; `counter` (int32, one element) += the number of rows UNFINISHED AFTER the step -- not finished before it
    and with a token outside term_range = [EOS, EOS + 1) -- instead of the rows that selected a token >= ge_bound."""
    _dev(logits, "logits"), _dev(uniforms, "uniforms")
    out = {}
    B, S, spg, nw, E, rows, stats = _step_operands(logits, seqs_per_group, mask, kv_len, memory, want_rows, want_stats, out)
    if uniforms.dim() != 1 or not uniforms.is_contiguous() or uniforms.numel() < 1:
        raise ValueError("uniforms must be a contiguous non-empty 1-D tensor")
    U = uniforms.numel()
    t, k, pp = float(temperature), int(top_k), float(top_p)
    if not (0.0 <= t < float("inf")) or k < 0 or not (0.0 < pp <= 1.0):
        raise ValueError("sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]")
    if not int(term_range[0]) < int(term_range[1]):
        raise ValueError("term_range must be (lo, hi) with lo < hi")
    if row_id is not None:
        _dev(row_id, "row_id", torch.int32)
        if row_id.dim() != 1 or row_id.numel() != B or (B and (int(row_id.min()) < 0 or int(row_id.max()) >= U)):
            raise ValueError("row_id must hold one index in [0, %d) per row of logits" % U)
        row_id = row_id.contiguous()
    elif U < B:
        raise ValueError("%d uniforms for %d rows" % (U, B))
    if fin is not None:
        _dev(fin, "fin", torch.int32)
        if fin.dim() != 1 or fin.numel() != B:
            raise ValueError("fin must hold one flag per row of logits")
        fin = fin.contiguous()
    dev = logits.device
    out = dict({"next": torch.empty(B, device=dev, dtype=torch.int32), "logprob": torch.empty(B, device=dev, dtype=torch.float32),
                "fin": torch.empty(B, device=dev, dtype=torch.int32)}, **out)
    if counter is not None:
        _dev(counter, "counter", torch.int32)
    _L.check(_L.load().ff_pointer_sequence_sample(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), B, spg, _p(uniforms), U, _p(row_id), _p(fin), t, k, pp,
        int(term_range[0]), int(term_range[1]), _p(out["next"]), _p(out["logprob"]), _p(out["fin"]), _p(memory), E, _p(rows), E,
        _p(stats), _p(counter), _stream()), "ff_pointer_sequence_sample")
    return out


@_on_tensor_device
def follow_table(starts, ends, num_input, tol):
    """The co-edge follow table of N wireframes (ff_follow_table).  starts / ends [N, L, 2] fp32: (x, y) of every
    co-edge's first and last point; num_input [N] int32.  Returns bits [N, L, ceil(L/32)] int32 (the uint32 words): bit b of row
    a is set iff a, b < num_input[w] and |ends[a] - starts[b]| < tol in x and in y (fp32 subtraction, fp32 compare)."""
    _dev(starts, "starts"), _dev(ends, "ends"), _dev(num_input, "num_input", torch.int32)
    if starts.dim() != 3 or starts.size(2) != 2 or starts.shape != ends.shape:
        raise ValueError("starts and ends must both be [N, L, 2]")
    N, L = starts.size(0), starts.size(1)
    if num_input.dim() != 1 or num_input.numel() != N:
        raise ValueError("num_input must hold one count per wireframe")
    if not float(tol) >= 0.0:
        raise ValueError("tol must be >= 0")
    starts, ends, num_input = starts.contiguous(), ends.contiguous(), num_input.contiguous()
    bits = torch.zeros((N, L, (L + 31) // 32), device=starts.device, dtype=torch.int32)
    _L.check(_L.load().ff_follow_table(_p(starts), _p(ends), N, L, _p(num_input), float(tol), _p(bits), _stream()), "ff_follow_table")
    return bits


@_on_tensor_device
def pointer_constrained(logits, fin, first, prev, visited, flags, ntok, follows=None, memory=None, mask=None, kv_len=None,
                        seqs_per_group=1, term_range=(1, 4), want_rows=False, want_stats=False, counter=None):
    """One constrained selection step of the pointer head (ff_pointer_constrained).  logits [B, S] fp32 raw dot
    products (masked IN PLACE with the constrained mask; rows of finished sequences are not touched); fin / first / prev [B]
    int32: the state before the step (first / prev: edge index, -1 = none; the loop is open only when both are edges); visited [B, ceil(L/32)] int32 words, L = S - ntok
    (not modified: the updated copy is returned); follows [W, L, ceil(L/32)] int32 words (ops.follow_table) or None when CONNECT
    is clear.  Row b belongs to wireframe b // seqs_per_group of mask / kv_len / memory / follows.  Returns dict(next, fin,
    dead_end, first, prev [B] int32; logprob [B] fp32; visited; mask_rows [B, S] uint8: the rule's own mask of every unfinished
    row; [rows [B, E]]; [stats [B, E/32, 2]])."""
    return _constrained_step(logits, fin, first, prev, visited, flags, ntok, follows, memory, mask, kv_len, seqs_per_group, term_range,
                             want_rows, want_stats, counter, None)


@_on_tensor_device
def pointer_sequence_constrained(logits, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows=None, memory=None,
                                 mask=None, kv_len=None, seqs_per_group=1, want_rows=False, want_stats=False, counter=None):
    """One constrained selection step of the single-sequence model (ff_pointer_sequence_constrained):
    pointer_constrained's operands with the tokens SEP and EOS in place of a terminator range, and FF_CONSTRAIN_ONCE (4, only
    with NO_REPEAT) among the flags.  SEP ends the current face (first = prev = none; the returned visited words are cleared
    unless ONCE), EOS alone finishes the row, a dead end re-opens SEP alone and the row goes on.  counter (optional, [1] int32)
    += the rows unfinished after the step.  Returns pointer_constrained's dict; dead_end is this step's flag."""
    return _sequence_constrained_step(logits, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows, memory, mask, kv_len,
                                      seqs_per_group, want_rows, want_stats, counter, None)


@_on_tensor_device
def pointer_sequence_constrained_sample(logits, uniforms, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows=None,
                                        temperature=1.0, top_k=0, top_p=1.0, row_id=None, memory=None, mask=None, kv_len=None,
                                        seqs_per_group=1, want_rows=False, want_stats=False, counter=None):
    """One constrained sampling step of the single-sequence model (ff_pointer_sequence_constrained_sample):
    pointer_sequence_constrained's byte row and state update with pointer_sample's draw from the constrained masked row in place
    of the argmax: uniforms [U] fp32, row b reads uniforms[row_id[b]] (None: b).  Returns pointer_sequence_constrained's dict;
    logprob is (l[next] - max) - log sum exp(l - max) over the constrained row.  temperature=0 is pointer_sequence_constrained's
    step, bit for bit; flags=0 is pointer_sequence_sample's with term_range = (tok_eos, tok_eos + 1)."""
    return _sequence_constrained_step(logits, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows, memory, mask, kv_len,
                                      seqs_per_group, want_rows, want_stats, counter, (uniforms, row_id, temperature, top_k, top_p))


def _sequence_constrained_step(logits, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows, memory, mask, kv_len,
                               seqs_per_group, want_rows, want_stats, counter, draw, ahead=None):
    """pointer_sequence_constrained (draw None) and pointer_sequence_constrained_sample (draw = (uniforms, row_id, temperature,
    top_k, top_p)): the checks, the outputs and the launch the two share; ahead (as _lookahead_operands takes it): their closure
    forms, pointer_sequence_constrained_ahead and pointer_sequence_constrained_sample_ahead."""
    _dev(logits, "logits")
    out = {}
    B, S, spg, nw, E, rows, stats = _step_operands(logits, seqs_per_group, mask, kv_len, memory, want_rows, want_stats, out)
    flags, ntok, sep, eos = int(flags), int(ntok), int(tok_sep), int(tok_eos)
    L = S - ntok
    fw = (L + 31) // 32
    if flags & ~(_L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT | _L.FF_CONSTRAIN_ONCE):
        raise ValueError("unknown constraint flag bits %d" % flags)
    if flags & _L.FF_CONSTRAIN_ONCE and not flags & _L.FF_CONSTRAIN_NO_REPEAT:
        raise ValueError("FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT")
    if L < 0 or not (0 <= sep < ntok and 0 <= eos < ntok) or sep == eos:
        raise ValueError("tok_sep and tok_eos must be two different tokens below ntok <= S")
    if follows is None and flags & _L.FF_CONSTRAIN_CONNECT:
        raise ValueError("FF_CONSTRAIN_CONNECT needs the follow table")
    for x, name in ((fin, "fin"), (first, "first"), (prev, "prev")):
        _dev(x, name, torch.int32)
        if x.dim() != 1 or x.numel() != B:
            raise ValueError("%s must hold one int32 per row of logits" % name)
    fin, first, prev = fin.contiguous(), first.contiguous(), prev.contiguous()
    _dev(visited, "visited", torch.int32)
    if tuple(visited.shape) != (B, fw):
        raise ValueError("visited must be [%d, %d]" % (B, fw))
    visited = visited.clone().contiguous()
    if follows is not None:
        _dev(follows, "follows", torch.int32)
        if follows.dim() != 3 or not follows.is_contiguous() or follows.size(0) < nw or tuple(follows.shape[1:]) != (L, fw):
            raise ValueError("follows must be a contiguous [>= %d, %d, %d] tensor" % (nw, L, fw))
    dev = logits.device
    i32 = lambda: torch.empty(B, device=dev, dtype=torch.int32)
    out = dict({"next": i32(), "logprob": torch.empty(B, device=dev, dtype=torch.float32), "fin": i32(), "dead_end": i32(),
                "first": i32(), "prev": i32(), "visited": visited, "mask_rows": torch.zeros((B, S), device=dev, dtype=torch.uint8)}, **out)
    if counter is not None:
        _dev(counter, "counter", torch.int32)
    one = torch.zeros(1, device=dev, dtype=torch.int32)   # (L = 0: one word each so that the pointers are not null)
    vis = visited if fw else one
    fol = one if (follows is not None and not (L and fw)) else follows
    entry, tail = "ff_pointer_sequence_constrained", ()
    if draw is not None:
        d = _draw_operands(draw, B)      # (`d` keeps a contiguous copy of row_id alive over the call)
        entry, tail = "ff_pointer_sequence_constrained_sample", (_p(d[0]), d[1], _p(d[2])) + d[3:]
    if ahead is not None:      # (ONCE is this rule's own bit: the look-aheads' flag checks are about the other two)
        form, close_dist, cycle_len, budget = _lookahead_operands(ahead, flags & ~_L.FF_CONSTRAIN_ONCE, S, L, nw, dev,
                                                                  entry[3:] + "_ahead")
        entry, tail = entry + "_ahead", tail + (form, _p(close_dist), _p(cycle_len), budget)
    _L.check(getattr(_L.load(), entry)(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), B, spg, _p(fol), L, flags, ntok, sep, eos, _p(fin), _p(first),
        _p(prev), _p(vis), _p(out["mask_rows"]), _p(out["next"]), _p(out["logprob"]), _p(out["fin"]), _p(out["dead_end"]),
        _p(out["first"]), _p(out["prev"]), _p(memory), E, _p(rows), E, _p(stats), _p(counter), *tail, _stream()), entry)
    return out


SEQUENCE_CLOSURES = {"lookahead": "ahead", "exact": "exact"}      # sequence_constrain_closure -> _lookahead_operands' form


def _sequence_closure(closure, close_dist, cycle_len, budget):
    if closure not in SEQUENCE_CLOSURES:
        raise ValueError("closure=%r: must be 'lookahead' or 'exact'" % (closure,))
    return ("exact", cycle_len, budget) if closure == "exact" else ("ahead", close_dist, cycle_len, budget)


@_on_tensor_device
def pointer_sequence_constrained_ahead(logits, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows, closure, cycle_len,
                                       budget, close_dist=None, memory=None, mask=None, kv_len=None, seqs_per_group=1,
                                       want_rows=False, want_stats=False, counter=None):
    """pointer_sequence_constrained with a closure look-ahead (ff_pointer_sequence_constrained_ahead).  closure
    "lookahead": under CONNECT an edge b is also masked when close_dist[w][first][b] > budget (loop open) or cycle_len[w][b] >
    budget (loop closed); "exact" (NO_REPEAT as well, at most 2048 keys): with the loop open when no path of at most `budget`
    hops leads from b to the loop's first edge through edges that are neither padded nor in the row's visited words (under ONCE:
    the edges of every face so far), with it closed the cycle_len rule; close_dist is not read.  close_dist [W, L, L] / cycle_len
    [W, L] uint8 (ops.follow_distance), budget in 0..254.  The dead-end vote runs after these masks; the two fix-ups of the closed
    state are unchanged.  Operands and results are pointer_sequence_constrained's; "lookahead" with both tables zero gives them
    bit for bit."""
    return _sequence_constrained_step(logits, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows, memory, mask, kv_len,
                                      seqs_per_group, want_rows, want_stats, counter, None,
                                      _sequence_closure(closure, close_dist, cycle_len, budget))


@_on_tensor_device
def pointer_sequence_constrained_sample_ahead(logits, uniforms, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows,
                                              closure, cycle_len, budget, close_dist=None, temperature=1.0, top_k=0, top_p=1.0,
                                              row_id=None, memory=None, mask=None, kv_len=None, seqs_per_group=1, want_rows=False,
                                              want_stats=False, counter=None):
    """pointer_sequence_constrained_sample with a closure look-ahead (ff_pointer_sequence_constrained_sample_ahead):
    pointer_sequence_constrained_ahead's byte row with pointer_sequence_constrained_sample's draw from it.  temperature=0 is
    pointer_sequence_constrained_ahead's step, bit for bit."""
    return _sequence_constrained_step(logits, fin, first, prev, visited, flags, ntok, tok_sep, tok_eos, follows, memory, mask, kv_len,
                                      seqs_per_group, want_rows, want_stats, counter, (uniforms, row_id, temperature, top_k, top_p),
                                      _sequence_closure(closure, close_dist, cycle_len, budget))


def _draw_operands(draw, B):
    """The checks of a step's draw = (uniforms, row_id, temperature, top_k, top_p) for B launch rows -> (uniforms, U, row_id made contiguous or
    None, temperature, top_k, top_p): the entry's arguments, the two tensors still to be taken the address of."""
    uniforms, row_id, temperature, top_k, top_p = draw
    _dev(uniforms, "uniforms")
    if uniforms.dim() != 1 or not uniforms.is_contiguous() or uniforms.numel() < 1:
        raise ValueError("uniforms must be a contiguous non-empty 1-D tensor")
    U = uniforms.numel()
    t, k, pp = float(temperature), int(top_k), float(top_p)
    if not (0.0 <= t < float("inf")) or k < 0 or not (0.0 < pp <= 1.0):
        raise ValueError("sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]")
    if row_id is not None:
        _dev(row_id, "row_id", torch.int32)
        if row_id.dim() != 1 or row_id.numel() != B or (B and (int(row_id.min()) < 0 or int(row_id.max()) >= U)):
            raise ValueError("row_id must hold one index in [0, %d) per row of logits" % U)
        row_id = row_id.contiguous()
    elif U < B:
        raise ValueError("%d uniforms for %d rows" % (U, B))
    return (uniforms, U, row_id, t, k, pp)


def _constrained_step(logits, fin, first, prev, visited, flags, ntok, follows, memory, mask, kv_len, seqs_per_group, term_range,
                      want_rows, want_stats, counter, ahead, draw=None):
    """pointer_constrained (ahead None), pointer_constrained_ahead (ahead = ("ahead", close_dist, cycle_len, budget)) and
    pointer_constrained_exact (ahead = ("exact", cycle_len, budget)): the checks, the outputs and the launch the three share.
    draw = (uniforms, row_id, temperature, top_k, top_p): pointer_constrained_sample, the same step with the draw in place of the
    argmax, in the form `ahead` names."""
    _dev(logits, "logits")
    out = {}
    B, S, spg, nw, E, rows, stats = _step_operands(logits, seqs_per_group, mask, kv_len, memory, want_rows, want_stats, out)
    flags, ntok = int(flags), int(ntok)
    L = S - ntok
    fw = (L + 31) // 32
    lo, hi = int(term_range[0]), int(term_range[1])
    if flags & ~(_L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT):
        raise ValueError("unknown constraint flag bits %d" % flags)
    if L < 0 or not 0 <= lo < hi <= ntok:
        raise ValueError("need 0 <= term_lo < term_hi <= ntok <= S")
    if follows is None and flags & _L.FF_CONSTRAIN_CONNECT:
        raise ValueError("FF_CONSTRAIN_CONNECT needs the follow table")
    for x, name in ((fin, "fin"), (first, "first"), (prev, "prev")):
        _dev(x, name, torch.int32)
        if x.dim() != 1 or x.numel() != B:
            raise ValueError("%s must hold one int32 per row of logits" % name)
    fin, first, prev = fin.contiguous(), first.contiguous(), prev.contiguous()
    _dev(visited, "visited", torch.int32)
    if tuple(visited.shape) != (B, fw):
        raise ValueError("visited must be [%d, %d]" % (B, fw))
    visited = visited.clone().contiguous()
    if follows is not None:
        _dev(follows, "follows", torch.int32)
        if follows.dim() != 3 or not follows.is_contiguous() or follows.size(0) < nw or tuple(follows.shape[1:]) != (L, fw):
            raise ValueError("follows must be a contiguous [>= %d, %d, %d] tensor" % (nw, L, fw))
    dev = logits.device
    i32 = lambda: torch.empty(B, device=dev, dtype=torch.int32)
    out = dict({"next": i32(), "logprob": torch.empty(B, device=dev, dtype=torch.float32), "fin": i32(), "dead_end": i32(),
                "first": i32(), "prev": i32(), "visited": visited, "mask_rows": torch.zeros((B, S), device=dev, dtype=torch.uint8)}, **out)
    if counter is not None:
        _dev(counter, "counter", torch.int32)
    # (L = 0: no edge key, nothing of the table or the visited words is read -- one word each so that the pointers are not null)
    one = torch.zeros(1, device=dev, dtype=torch.int32)
    vis = visited if fw else one
    fol = one if (follows is not None and not (L and fw)) else follows
    entry, tail = "ff_pointer_constrained", ()
    if ahead is not None:
        what = "pointer_constrained_exact" if ahead[0] == "exact" else "pointer_constrained_ahead"
        form, close_dist, cycle_len, budget = _lookahead_operands(ahead, flags, S, L, nw, dev, what)
        entry, tail = "ff_" + what, ((_p(close_dist),) if form == 1 else ()) + (_p(cycle_len), budget)
    if draw is not None:
        d = _draw_operands(draw, B)      # (`d` keeps a contiguous copy of row_id alive over the call)
        form = {"ff_pointer_constrained": 0, "ff_pointer_constrained_ahead": 1, "ff_pointer_constrained_exact": 2}[entry]
        tables = {0: (None, None, 0), 1: tail, 2: (None,) + tail}[form]      # (close_dist, cycle_len, budget)
        entry, tail = "ff_pointer_constrained_sample", (_p(d[0]), d[1], _p(d[2])) + d[3:] + (form,) + tuple(tables)
    _L.check(getattr(_L.load(), entry)(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), B, spg, _p(fol), L, flags, ntok, lo, hi, _p(fin), _p(first),
        _p(prev), _p(vis), _p(out["mask_rows"]), _p(out["next"]), _p(out["logprob"]), _p(out["fin"]), _p(out["dead_end"]),
        _p(out["first"]), _p(out["prev"]), _p(memory), E, _p(rows), E, _p(stats), _p(counter), *tail, _stream()), entry)
    return out


@_on_tensor_device
def pointer_constrained_ahead(logits, fin, first, prev, visited, flags, ntok, follows, close_dist, cycle_len, budget, memory=None,
                              mask=None, kv_len=None, seqs_per_group=1, term_range=(1, 4), want_rows=False, want_stats=False,
                              counter=None):
    """pointer_constrained with the closure look-ahead (ff_pointer_constrained_ahead): under CONNECT an edge b is
    also masked when close_dist[w][first][b] > budget (loop open) or cycle_len[w][b] > budget (loop closed).  close_dist
    [W, L, L] / cycle_len [W, L] uint8 (ops.follow_distance), budget in 0..254: the positions left behind the one this step
    selects.  Operands and results are pointer_constrained's; with both tables zero the results are too."""
    return _constrained_step(logits, fin, first, prev, visited, flags, ntok, follows, memory, mask, kv_len, seqs_per_group, term_range,
                             want_rows, want_stats, counter, ("ahead", close_dist, cycle_len, budget))


EXACT_MAX_KEYS = 2048      # (ff_pointer_constrained_exact: L + ntok)


@_on_tensor_device
def pointer_constrained_sample(logits, uniforms, fin, first, prev, visited, flags, ntok, follows=None, temperature=1.0, top_k=0,
                               top_p=1.0, row_id=None, lookahead=None, close_dist=None, cycle_len=None, budget=0, memory=None,
                               mask=None, kv_len=None, seqs_per_group=1, term_range=(1, 4), want_rows=False, want_stats=False,
                               counter=None):
    """One constrained sampling step of the pointer head (ff_pointer_constrained_sample): pointer_constrained's
    byte row and state update -- lookahead None, "ahead" (pointer_constrained_ahead's, with close_dist / cycle_len / budget) or
    "exact" (pointer_constrained_exact's, with cycle_len / budget) -- with pointer_sample's draw from the constrained masked row
    in place of the argmax: uniforms [U] fp32, row b reads uniforms[row_id[b]] (None: b).  Returns pointer_constrained's dict;
    logprob is (l[next] - max) - log sum exp(l - max) over the constrained row.  temperature=0 is pointer_constrained's step, bit
    for bit; flags=0 is pointer_sample's."""
    if lookahead not in (None, "ahead", "exact"):
        raise ValueError("lookahead=%r: must be None, 'ahead' or 'exact'" % (lookahead,))
    ahead = None if lookahead is None else (("ahead", close_dist, cycle_len, budget) if lookahead == "ahead" else ("exact", cycle_len, budget))
    return _constrained_step(logits, fin, first, prev, visited, flags, ntok, follows, memory, mask, kv_len, seqs_per_group, term_range,
                             want_rows, want_stats, counter, ahead, (uniforms, row_id, temperature, top_k, top_p))


@_on_tensor_device
def pointer_constrained_exact(logits, fin, first, prev, visited, flags, ntok, follows, cycle_len, budget, memory=None, mask=None,
                              kv_len=None, seqs_per_group=1, term_range=(1, 4), want_rows=False, want_stats=False, counter=None):
    """pointer_constrained with the exact closure look-ahead (ff_pointer_constrained_exact): with the loop open an
    edge b is also masked when no path of at most `budget` hops leads from b to the loop's first edge through edges that are
    neither visited nor padded (faces.closure_distance is the numpy restatement); with it closed when cycle_len[w][b] > budget.
    flags must be NO_REPEAT | CONNECT; cycle_len [W, L] uint8 (ops.follow_distance), budget in 0..254; at most 2048 keys.
    Operands and results are pointer_constrained's."""
    return _constrained_step(logits, fin, first, prev, visited, flags, ntok, follows, memory, mask, kv_len, seqs_per_group, term_range,
                             want_rows, want_stats, counter, ("exact", cycle_len, budget))


FOLLOW_DISTANCE_MAX_L = 8192


@_on_tensor_device
def follow_distance(follows, num_input, hmax):
    """The closing distances of N wireframes' follow tables (ff_follow_distance).  follows [N, L, ceil(L/32)] int32
    words (ops.follow_table), num_input [N] int32, hmax in 1..254.  Returns (close_dist [N, L, L] uint8: close_dist[w][f][b] =
    D(b -> f), the least number of "follows" hops from edge b to edge f; cycle_len [N, L] uint8: D(b -> b)); 255: unreachable, more
    than hmax hops, or an edge at or beyond num_input[w].  faces.follow_distance is the numpy restatement."""
    if isinstance(hmax, bool) or not isinstance(hmax, int) or not 1 <= hmax <= 254:
        raise ValueError("hmax=%r: must be in 1..254" % (hmax,))
    _dev(follows, "follows", torch.int32), _dev(num_input, "num_input", torch.int32)
    if follows.dim() != 3 or follows.size(2) != (follows.size(1) + 31) // 32:
        raise ValueError("follows must be [N, L, ceil(L/32)]")
    N, L = follows.size(0), follows.size(1)
    if num_input.dim() != 1 or num_input.numel() != N:
        raise ValueError("num_input must hold one count per wireframe")
    if L > FOLLOW_DISTANCE_MAX_L:
        raise ValueError("follow_distance takes at most %d edges per wireframe (got %d)" % (FOLLOW_DISTANCE_MAX_L, L))
    follows, num_input = follows.contiguous(), num_input.contiguous()
    close_dist = torch.empty((N, L, L), device=follows.device, dtype=torch.uint8)
    cycle_len = torch.empty((N, L), device=follows.device, dtype=torch.uint8)
    _L.check(_L.load().ff_follow_distance(_p(follows), N, L, _p(num_input), hmax, _p(close_dist), _p(cycle_len), _stream()),
             "ff_follow_distance")
    return close_dist, cycle_len


FACE_ROW_KEYS = ("len", "type", "closed", "loops", "edges", "loop_of", "set_bits", "score")
FACE_VOTE_KEYS = ("rep", "votes", "best", "major", "num_faces")


def _tok_field(token, name):
    try:
        return int(getattr(token, name))
    except AttributeError:
        return int(token[name])


@_on_tensor_device
def face_rows(tokens, num_input, token, num_edges=None, scores=None, logprob=None, dead_end=None, own_stop=False, follows=None,
              edge_map=None, num_lines=None):
    """The faces of decoded rows, on the device (ff_face_rows; include/faceformer_hip.h states the rule).  tokens
    [N, F, G, T] int64 (or [N, F, T]: G = 1), T <= 256; num_input [N] int32; token: the config's (face_type_offset, len);
    num_edges [N] int32 or None (= num_input); scores [N, F, G] fp32 or logprob [N, F, G, T] fp32 (not both); dead_end [N, F, G]
    int32; own_stop: every wireframe's own stop rule first; follows [N, L, ceil(L/32)] int32 (ops.follow_table) or None: no walk;
    edge_map [N, L] int32 or None.  L = the table's / the map's, else num_lines, else F.  Returns a dict of device tensors: len,
    type, closed, loops [N, F, G] int32; edges, loop_of [N, F, G, T] int32; set_bits [N, F, G, ceil(L/32)] int32; score [N, F, G]
    fp64.  faces.face_rows is the numpy restatement, bit for bit."""
    if not torch.is_tensor(tokens) or tokens.dim() not in (3, 4):
        raise ValueError("tokens must be a tensor [N, F, T] or [N, F, G, T]")
    if tokens.dim() == 3:
        tokens = tokens.unsqueeze(2)
    N, F, G, T = tokens.shape
    if not 1 <= T <= _L.FF_FACE_MAX_T:
        raise ValueError("face_rows takes 1..%d positions per row (got T=%d)" % (_L.FF_FACE_MAX_T, T))
    off, ntok = _tok_field(token, "face_type_offset"), _tok_field(token, "len")
    if not 0 <= off < ntok:
        raise ValueError("face_type_offset=%d must be in [0, len=%d)" % (off, ntok))
    if scores is not None and logprob is not None:
        raise ValueError("scores and logprob may not both be given")
    _dev(tokens, "tokens", torch.int64), _dev(num_input, "num_input", torch.int32)
    if num_input.dim() != 1 or num_input.numel() != N:
        raise ValueError("num_input must hold one count per wireframe")
    if num_edges is not None:
        _dev(num_edges, "num_edges", torch.int32)
        if num_edges.dim() != 1 or num_edges.numel() != N:
            raise ValueError("num_edges must hold one count per wireframe")
    for t, name, dtype, shape in ((scores, "scores", torch.float32, (N, F, G)), (logprob, "logprob", torch.float32, (N, F, G, T)),
                                  (dead_end, "dead_end", torch.int32, (N, F, G))):
        if t is not None:
            _dev(t, name, dtype)
            if t.numel() != N * F * G * (T if len(shape) == 4 else 1) or (t.dim() == len(shape) and tuple(t.shape) != shape):
                raise ValueError("%s must be [%s]" % (name, ", ".join(str(v) for v in shape)))
    if follows is not None:
        _dev(follows, "follows", torch.int32)
        if follows.dim() != 3 or follows.size(0) != N or follows.size(2) != (follows.size(1) + 31) // 32:
            raise ValueError("follows must be [N, L, ceil(L/32)]")
    L = follows.size(1) if follows is not None else edge_map.size(1) if torch.is_tensor(edge_map) and edge_map.dim() == 2 else \
        F if num_lines is None else int(num_lines)
    if edge_map is not None:
        _dev(edge_map, "edge_map", torch.int32)
        if tuple(edge_map.shape) != (N, L):
            raise ValueError("edge_map must be [N, L] = [%d, %d]" % (N, L))
    if L < 0:
        raise ValueError("num_lines must be >= 0")
    fw = (L + 31) // 32
    c = lambda t: None if t is None else t.contiguous()
    tokens, num_input, num_edges, scores, logprob, dead_end, follows, edge_map = (
        c(t) for t in (tokens, num_input, num_edges, scores, logprob, dead_end, follows, edge_map))
    dev = tokens.device
    out = {k: torch.empty((N, F, G), device=dev, dtype=torch.int32) for k in ("len", "type", "closed", "loops")}
    out["edges"] = torch.empty((N, F, G, T), device=dev, dtype=torch.int32)
    out["loop_of"] = torch.empty((N, F, G, T), device=dev, dtype=torch.int32)
    out["set_bits"] = torch.empty((N, F, G, fw), device=dev, dtype=torch.int32)
    out["score"] = torch.empty((N, F, G), device=dev, dtype=torch.float64)
    _L.check(_L.load().ff_face_rows(_p(tokens), N, F, G, T, _p(num_input), _p(num_edges), L, off, ntok, _p(scores), _p(logprob),
                                    _p(dead_end), _p(follows), _p(edge_map), _L.FF_FACE_OWN_STOP if own_stop else 0,
                                    *[_p(out[k]) for k in FACE_ROW_KEYS], _stream()), "ff_face_rows")
    return out


@_on_tensor_device
def _face_votes(set_bits, ln, ty, closed, score, require_closed):
    N, F, G = ln.shape
    R = F * G
    dev = ln.device
    out = {k: torch.empty((N, F, G), device=dev, dtype=torch.int32) for k in ("rep", "votes", "major")}
    out["best"] = torch.empty((N, F, G), device=dev, dtype=torch.float64)
    out["num_faces"] = torch.empty((N,), device=dev, dtype=torch.int32)
    lib = _L.load()
    nbytes = lib.ff_face_votes_workspace_bytes(N, R)
    ws = torch.empty(((nbytes + 7) // 8,), device=dev, dtype=torch.int64)
    _L.check(lib.ff_face_votes(_p(set_bits), _p(ln), _p(ty), _p(closed), _p(score), N, R, set_bits.size(-1),
                               _L.FF_FACE_REQUIRE_CLOSED if require_closed else 0, *[_p(out[k]) for k in FACE_VOTE_KEYS],
                               _p(ws), ws.numel() * 8, _stream()), "ff_face_votes")
    return out


def face_votes(rows, require_closed=False):
    """The de-duplicated faces of every wireframe, on the device (ff_face_votes).  rows: face_rows' dict (set_bits,
    len, type, closed, score are read).  A row takes part iff len > 0 and, with require_closed, closed == 1.  Returns a dict of
    device tensors: rep [N, F, G] int32 (the least row f*G + g of the wireframe with the same bitmap, -1: takes no part); votes,
    best (fp64), major at the rows with rep == own index, 0 elsewhere; num_faces [N] int32.  At most 65536 rows per wireframe.
    faces.face_votes is the numpy restatement, bit for bit."""
    try:
        set_bits, ln, ty, closed, score = (rows[k] for k in ("set_bits", "len", "type", "closed", "score"))
    except (KeyError, TypeError):
        raise ValueError("face_votes takes the dict face_rows returns")
    if not torch.is_tensor(ln) or ln.dim() != 3:
        raise ValueError("rows['len'] must be a tensor [N, F, G]")
    N, F, G = ln.shape
    if F * G > _L.FF_FACE_MAX_ROWS:
        raise ValueError("face_votes takes at most %d rows per wireframe (got %d)" % (_L.FF_FACE_MAX_ROWS, F * G))
    for t, name, dtype in ((set_bits, "set_bits", torch.int32), (ln, "len", torch.int32), (ty, "type", torch.int32),
                           (closed, "closed", torch.int32), (score, "score", torch.float64)):
        _dev(t, "rows['%s']" % name, dtype)
        if tuple(t.shape[:3]) != (N, F, G) or t.dim() != (4 if name == "set_bits" else 3):
            raise ValueError("rows['%s'] must be [N, F, G%s]" % (name, ", words" if name == "set_bits" else ""))
    return _face_votes(set_bits.contiguous(), ln.contiguous(), ty.contiguous(), closed.contiguous(), score.contiguous(),
                       bool(require_closed))


FACE_SEQ_ROW_KEYS = ("count", "len", "start", "type", "closed", "loops", "edges", "loop_of", "set_bits", "score", "dup_of", "take",
                     "row_best")


def _seq_operand(t, name, dtype, shape):
    """An operand of face_seq_rows / face_seq_votes: ValueError for what is not a tensor of this dtype and shape (None in the
    shape: any size)."""
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != len(shape) or \
            any(s is not None and s != n for s, n in zip(shape, t.shape)):
        raise ValueError("%s must be a %s tensor [%s]" % (name, str(dtype).replace("torch.", ""),
                                                         ", ".join("*" if s is None else str(s) for s in shape)))


@_on_tensor_device
def face_seq_rows(tokens, num_edges, token, slots=None, scores=None, logprob=None, finished=None, follows=None, edge_map=None,
                  closed_only=False, num_lines=None):
    """The faces of the single-sequence model's decoded rows, on the device (ff_face_seq_rows; include/faceformer_hip.h
    states the rule).  tokens [N, G, T] int64 (or [N, T]: G = 1, and the row operands may then leave that axis out too), T <= 2048; num_edges [N] int32; token: the config's (len, SEP,
    EOS); slots = P face slots per row (None: max(T // 2, 1), which never truncates); scores [N, G] fp32 or logprob [N, G, T] fp32
    (not both); finished [N, G] int32; follows [N, L, ceil(L/32)] int32 (ops.follow_table) or None: no walk; edge_map [N, L] int32
    or None; closed_only: only closed faces take part in the fold.  L = the table's / the map's, else num_lines.  Returns a dict
    of device tensors: count [N, G] int32; len, start, type, closed, loops, dup_of, take [N, G, P] int32; edges, loop_of [N, G, T]
    int32; set_bits [N, G, P, ceil(L/32)] int32; score, row_best [N, G, P] fp64.  faces.face_seq_rows is the numpy restatement,
    bit for bit.  Every refusal below is a ValueError raised before the library is touched."""
    if not torch.is_tensor(tokens) or tokens.dim() not in (2, 3) or tokens.dtype != torch.int64:
        raise ValueError("tokens must be an int64 tensor [N, T] or [N, G, T]")
    if tokens.dim() == 2:        # (G = 1: the row operands may leave the axis out as well)
        tokens = tokens.unsqueeze(1)
        scores, finished = (t.unsqueeze(1) if torch.is_tensor(t) and t.dim() == 1 else t for t in (scores, finished))
        logprob = logprob.unsqueeze(1) if torch.is_tensor(logprob) and logprob.dim() == 2 else logprob
    N, G, T = tokens.shape
    if not 1 <= T <= _L.FF_FACE_SEQ_MAX_T:
        raise ValueError("face_seq_rows takes 1..%d positions per row (got T=%d)" % (_L.FF_FACE_SEQ_MAX_T, T))
    pmax = max(T // 2, 1)
    if slots is not None and (isinstance(slots, bool) or not isinstance(slots, int)):
        raise ValueError("slots=%r: must be None or an integer" % (slots,))
    P = pmax if slots is None else slots
    if not 1 <= P <= pmax:
        raise ValueError("slots=%d: must be in 1..max(T // 2, 1) = %d" % (P, pmax))
    if G * P > _L.FF_FACE_MAX_ROWS:
        raise ValueError("face_seq_rows takes at most %d slots per wireframe (got G * P = %d)" % (_L.FF_FACE_MAX_ROWS, G * P))
    ntok, sep, eos = _tok_field(token, "len"), _tok_field(token, "SEP"), _tok_field(token, "EOS")
    if not (0 <= sep < ntok and 0 <= eos < ntok and sep != eos):
        raise ValueError("SEP=%d and EOS=%d must be two tokens of [0, len=%d)" % (sep, eos, ntok))
    if scores is not None and logprob is not None:
        raise ValueError("scores and logprob may not both be given")
    _seq_operand(num_edges, "num_edges", torch.int32, (N,))
    for t, name, dtype, shape in ((scores, "scores", torch.float32, (N, G)), (logprob, "logprob", torch.float32, (N, G, T)),
                                  (finished, "finished", torch.int32, (N, G))):
        if t is not None:
            _seq_operand(t, name, dtype, shape)
    if follows is not None:
        _seq_operand(follows, "follows", torch.int32, (N, None, None))
        if follows.size(2) != (follows.size(1) + 31) // 32:
            raise ValueError("follows must be [N, L, ceil(L/32)]")
    if follows is None and edge_map is None and num_lines is None:
        raise ValueError("num_lines is needed without a follow table and an edge map")
    if edge_map is not None:
        _seq_operand(edge_map, "edge_map", torch.int32, (N, follows.size(1) if follows is not None else None))
    L = follows.size(1) if follows is not None else edge_map.size(1) if edge_map is not None else int(num_lines)      # (the restatement's order)
    if L < 0:
        raise ValueError("num_lines must be >= 0")
    for t, name, dtype in ((tokens, "tokens", torch.int64), (num_edges, "num_edges", torch.int32), (scores, "scores", torch.float32),
                           (logprob, "logprob", torch.float32), (finished, "finished", torch.int32), (follows, "follows", torch.int32),
                           (edge_map, "edge_map", torch.int32)):
        if t is not None:
            _dev(t, name, dtype)
    fw = (L + 31) // 32
    c = lambda t: None if t is None else t.contiguous()
    tokens, num_edges, scores, logprob, finished, follows, edge_map = (
        c(t) for t in (tokens, num_edges, scores, logprob, finished, follows, edge_map))
    dev = tokens.device
    out = {k: torch.empty((N, G, P), device=dev, dtype=torch.int32) for k in ("len", "start", "type", "closed", "loops", "dup_of", "take")}
    out["count"] = torch.empty((N, G), device=dev, dtype=torch.int32)
    out["edges"] = torch.empty((N, G, T), device=dev, dtype=torch.int32)
    out["loop_of"] = torch.empty((N, G, T), device=dev, dtype=torch.int32)
    out["set_bits"] = torch.empty((N, G, P, fw), device=dev, dtype=torch.int32)
    out["score"] = torch.empty((N, G, P), device=dev, dtype=torch.float64)
    out["row_best"] = torch.empty((N, G, P), device=dev, dtype=torch.float64)
    _L.check(_L.load().ff_face_seq_rows(_p(tokens), N, G, T, _p(num_edges), L, ntok, sep, eos, P, _p(scores), _p(logprob), _p(finished),
                                        _p(follows), _p(edge_map), _L.FF_FACE_SEQ_CLOSED_ONLY if closed_only else 0,
                                        *[_p(out[k]) for k in FACE_SEQ_ROW_KEYS], _stream()), "ff_face_seq_rows")
    return {k: out[k] for k in FACE_SEQ_ROW_KEYS}


def face_seq_votes(rows, require_closed=False):
    """The de-duplicated faces of every wireframe behind face_seq_rows, on the device: ff_face_votes, unchanged, over
    the G * P slots of a wireframe with len := take and score := row_best.  rows: face_seq_rows' dict (set_bits, take, type,
    closed, row_best are read).  Returns a dict of device tensors: rep [N, G, P] int32 (the least slot g * P + s of the wireframe
    with the same bitmap, -1: takes no part); votes (the draws or beams that hold the face), best (fp64), major at the slots with
    rep == own index, 0 elsewhere; num_faces [N] int32.  faces.face_seq_votes is the numpy restatement, bit for bit."""
    try:
        set_bits, take, ty, closed, best = (rows[k] for k in ("set_bits", "take", "type", "closed", "row_best"))
    except (KeyError, TypeError):
        raise ValueError("face_seq_votes takes the dict face_seq_rows returns")
    if not torch.is_tensor(take) or take.dim() != 3:
        raise ValueError("rows['take'] must be a tensor [N, G, P]")
    N, G, P = take.shape
    if G * P > _L.FF_FACE_MAX_ROWS:
        raise ValueError("face_seq_votes takes at most %d slots per wireframe (got G * P = %d)" % (_L.FF_FACE_MAX_ROWS, G * P))
    for t, name, dtype in ((take, "take", torch.int32), (ty, "type", torch.int32), (closed, "closed", torch.int32),
                           (best, "row_best", torch.float64)):
        _seq_operand(t, "rows['%s']" % name, dtype, (N, G, P))
    _seq_operand(set_bits, "rows['set_bits']", torch.int32, (N, G, P, None))
    for t, name, dtype in ((set_bits, "set_bits", torch.int32), (take, "take", torch.int32), (ty, "type", torch.int32),
                           (closed, "closed", torch.int32), (best, "row_best", torch.float64)):
        _dev(t, "rows['%s']" % name, dtype)
    flat = lambda t: t.contiguous().view(N, G * P, 1)
    out = _face_votes(set_bits.contiguous().view(N, G * P, 1, set_bits.size(-1)), flat(take), flat(ty), flat(closed), flat(best),
                      bool(require_closed))
    return {k: (v if k == "num_faces" else v.view(N, G, P)) for k, v in out.items()}


@_on_tensor_device
def beam_constrained_select(logits, scores, fin, dead, first, prev, visited, width, flags, ntok, follows=None, memory=None,
                            mask=None, kv_len=None, groups_per_wireframe=None, term_range=(1, 4), want_rows=False, want_stats=False,
                            counter=None):
    """One beam-search step over the constrained rows of every group (ff_beam_constrained_select).  logits
    [G * width, S] fp32 raw dot products (masked IN PLACE with the constrained masks; rows of empty / finished beams are not
    touched); scores [G * width] fp32 (-inf: empty beam), fin / dead / first / prev [G * width] int32 and visited [G * width,
    ceil(L/32)] int32 words, L = S - ntok, are the state before the step (none of them is modified); follows [W, L, ceil(L/32)]
    int32 words (ops.follow_table) or None when CONNECT is clear.  Row b belongs to wireframe b // (groups_per_wireframe * width).
    Returns dict(parent, next, fin, dead, first, prev [G * width] int32; scores fp32; visited; mask_rows [G * width, S] uint8:
    the rule's own mask of every non-empty unfinished beam; [rows]; [stats]): the new beams in rank order, best first."""
    return _beam_constrained_step(logits, scores, fin, dead, first, prev, visited, width, flags, ntok, follows, memory, mask, kv_len,
                                  groups_per_wireframe, term_range, want_rows, want_stats, counter, None)


@_on_tensor_device
def beam_constrained_select_ahead(logits, scores, fin, dead, first, prev, visited, width, flags, ntok, follows, lookahead, cycle_len,
                                  budget, close_dist=None, memory=None, mask=None, kv_len=None, groups_per_wireframe=None,
                                  term_range=(1, 4), want_rows=False, want_stats=False, counter=None):
    """beam_constrained_select with a closure look-ahead in every beam's byte row (ff_beam_constrained_select_ahead, DESIGN.md
    28).  lookahead "lookahead": pointer_constrained_ahead's row per beam (close_dist [W, L, L] and cycle_len [W, L] uint8,
    ops.follow_distance); "exact": pointer_constrained_exact's (cycle_len only; flags must be NO_REPEAT | CONNECT, at most 2048
    keys; one search per open beam over its own visited words).  budget in 0..254, shared by every beam of the launch.  Operands
    and results are beam_constrained_select's; `dead` then also means "cannot close within the budget".  "lookahead" with both
    tables zero is beam_constrained_select, bit for bit; width 1 is the constrained greedy step of the same form."""
    if lookahead not in ("lookahead", "exact"):
        raise ValueError("lookahead=%r: must be 'lookahead' or 'exact'" % (lookahead,))
    ahead = ("ahead", close_dist, cycle_len, budget) if lookahead == "lookahead" else ("exact", cycle_len, budget)
    return _beam_constrained_step(logits, scores, fin, dead, first, prev, visited, width, flags, ntok, follows, memory, mask, kv_len,
                                  groups_per_wireframe, term_range, want_rows, want_stats, counter, ahead)


def _lookahead_operands(ahead, flags, S, L, nw, dev, what):
    """The checks of a look-ahead's operands that the constrained greedy and beam steps share: ahead = ("ahead", close_dist,
    cycle_len, budget) or ("exact", cycle_len, budget) -> (form, close_dist or None, cycle_len, budget), one byte in place of the
    tables at L = 0, where nothing of them is read."""
    byte = torch.zeros(1, device=dev, dtype=torch.uint8)
    if ahead[0] == "exact":
        _, cycle_len, budget = ahead
        if flags != _L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT:
            raise ValueError("the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT")
        if S > EXACT_MAX_KEYS:
            raise ValueError("%s takes at most %d keys (L + ntok; got %d)" % (what, EXACT_MAX_KEYS, S))
        tables = ((cycle_len, "cycle_len", (L,)),)
    else:
        _, close_dist, cycle_len, budget = ahead
        if not flags & _L.FF_CONSTRAIN_CONNECT:
            raise ValueError("the look-ahead needs FF_CONSTRAIN_CONNECT")
        tables = ((close_dist, "close_dist", (L, L)), (cycle_len, "cycle_len", (L,)))
    for x, name, shape in tables:
        _dev(x, name, torch.uint8)
        if x.dim() != 1 + len(shape) or not x.is_contiguous() or x.size(0) < nw or tuple(x.shape[1:]) != shape:
            raise ValueError("%s must be a contiguous uint8 [>= %d, %s] tensor" % (name, nw, ", ".join(str(v) for v in shape)))
    if not 0 <= int(budget) <= 254:
        raise ValueError("budget=%r: must be in 0..254" % (budget,))
    if ahead[0] == "exact":
        return 2, None, (cycle_len if L else byte), int(budget)
    return 1, (close_dist if L else byte), (cycle_len if L else byte), int(budget)


def _beam_constrained_step(logits, scores, fin, dead, first, prev, visited, width, flags, ntok, follows, memory, mask, kv_len,
                           groups_per_wireframe, term_range, want_rows, want_stats, counter, ahead):
    """beam_constrained_select (ahead None) and beam_constrained_select_ahead (ahead as _lookahead_operands takes it): the checks,
    the outputs and the launch the two share."""
    _dev(logits, "logits"), _dev(scores, "scores")
    out = {}
    if logits.dim() != 2:
        raise ValueError("logits must be a 2-D tensor with unit inner stride")
    B = logits.size(0)
    width = int(width)
    if not 1 <= width <= BEAM_MAX_WIDTH or width > logits.size(1) or B % width:
        raise ValueError("beam width %d: must be in 1..%d, at most S = %d, and divide the %d rows"
                         % (width, BEAM_MAX_WIDTH, logits.size(1), B))
    G = B // width
    gpw = max(G, 1) if groups_per_wireframe is None else int(groups_per_wireframe)
    B, S, spg, nw, E, rows, stats = _step_operands(logits, gpw * width, mask, kv_len, memory, want_rows, want_stats, out)
    flags, ntok = int(flags), int(ntok)
    L = S - ntok
    fw = (L + 31) // 32
    lo, hi = int(term_range[0]), int(term_range[1])
    if flags & ~(_L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT):
        raise ValueError("unknown constraint flag bits %d" % flags)
    if L < 0 or not 0 <= lo < hi <= ntok:
        raise ValueError("need 0 <= term_lo < term_hi <= ntok <= S")
    if follows is None and flags & _L.FF_CONSTRAIN_CONNECT:
        raise ValueError("FF_CONSTRAIN_CONNECT needs the follow table")
    if scores.dim() != 1 or scores.numel() != B:
        raise ValueError("scores must hold one fp32 per row of logits")
    for x, name in ((fin, "fin"), (dead, "dead"), (first, "first"), (prev, "prev")):
        _dev(x, name, torch.int32)
        if x.dim() != 1 or x.numel() != B:
            raise ValueError("%s must hold one int32 per row of logits" % name)
    scores, fin, dead, first, prev = scores.contiguous(), fin.contiguous(), dead.contiguous(), first.contiguous(), prev.contiguous()
    _dev(visited, "visited", torch.int32)
    if tuple(visited.shape) != (B, fw):
        raise ValueError("visited must be [%d, %d]" % (B, fw))
    visited = visited.contiguous()
    if follows is not None:
        _dev(follows, "follows", torch.int32)
        if follows.dim() != 3 or not follows.is_contiguous() or follows.size(0) < nw or tuple(follows.shape[1:]) != (L, fw):
            raise ValueError("follows must be a contiguous [>= %d, %d, %d] tensor" % (nw, L, fw))
    dev = logits.device
    i32 = lambda: torch.empty(B, device=dev, dtype=torch.int32)
    out = dict({"parent": i32(), "next": i32(), "scores": torch.empty(B, device=dev, dtype=torch.float32), "fin": i32(), "dead": i32(),
                "first": i32(), "prev": i32(), "visited": torch.empty((B, fw), device=dev, dtype=torch.int32),
                "mask_rows": torch.zeros((B, S), device=dev, dtype=torch.uint8)}, **out)
    if counter is not None:
        _dev(counter, "counter", torch.int32)
    # (L = 0: no edge key, nothing of the table or the visited words is read -- one word each so that the pointers are not null)
    one, two = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
    fol = one if (follows is not None and not (L and fw)) else follows
    d = _L.BeamConstrainedStep(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), G, width, gpw, _p(fol), L, flags, ntok, lo, hi,
        _p(scores), _p(fin), _p(dead), _p(first), _p(prev), _p(visited if fw else one),
        _p(out["scores"]), _p(out["fin"]), _p(out["dead"]), _p(out["first"]), _p(out["prev"]), _p(out["visited"] if fw else two),
        _p(out["mask_rows"]), _p(out["parent"]), _p(out["next"]), _p(memory), E, _p(rows), E, _p(stats), _p(counter))
    if ahead is None:
        _L.check(_L.load().ff_beam_constrained_select(C.byref(d), _stream()), "ff_beam_constrained_select")
        return out
    form, close_dist, cycle_len, budget = _lookahead_operands(ahead, flags, S, L, nw, dev, "beam_constrained_select_ahead")
    da = _L.BeamConstrainedAheadStep(d, form, _p(close_dist), _p(cycle_len), budget)
    _L.check(_L.load().ff_beam_constrained_select_ahead(C.byref(da), _stream()), "ff_beam_constrained_select_ahead")
    return out


@_on_tensor_device
def beam_sequence_constrained_select(logits, scores, fin, first, prev, visited, width, flags, ntok, tok_sep, tok_eos, follows=None,
                                     stop="all", memory=None, mask=None, kv_len=None, groups_per_wireframe=None, want_rows=False,
                                     want_stats=False, counter=None):
    """One beam-search step over the rows the single-sequence model's loop rule leaves (ff_beam_sequence_constrained_select,
    DESIGN.md 34): beam_constrained_select's operands with pointer_sequence_constrained's rule (tok_sep / tok_eos in place of a
    terminator range, FF_CONSTRAIN_ONCE accepted) and beam_sequence_select's stop forms (stop "all" / "best": what `counter`
    receives).  There is no cumulative dead flag: a dead end abandons the face, not the beam.  Returns dict(parent, next, fin,
    dead_end (this step's flag), open (a loop is open after the step), first, prev [G * width] int32; scores fp32; visited;
    mask_rows [G * width, S] uint8; [rows]; [stats]): the new beams in rank order, best first.  No operand is modified but logits."""
    return _beam_sequence_constrained_step(logits, scores, fin, first, prev, visited, width, flags, ntok, tok_sep, tok_eos, follows,
                                           stop, memory, mask, kv_len, groups_per_wireframe, want_rows, want_stats, counter, None)


@_on_tensor_device
def beam_sequence_constrained_select_ahead(logits, scores, fin, first, prev, visited, width, flags, ntok, tok_sep, tok_eos, follows,
                                           closure, cycle_len, budget, close_dist=None, stop="all", memory=None, mask=None,
                                           kv_len=None, groups_per_wireframe=None, want_rows=False, want_stats=False, counter=None):
    """beam_sequence_constrained_select with a closure look-ahead (ff_beam_sequence_constrained_select_ahead): every
    unfinished non-empty beam forms pointer_sequence_constrained_ahead's byte row from its OWN (first, prev) and visited words --
    closure "lookahead": under CONNECT an edge b is also masked when close_dist[w][first_k][b] > budget (loop open) or
    cycle_len[w][b] > budget (loop closed); "exact" (NO_REPEAT as well, at most 2048 keys): with the loop open when no path of at
    most `budget` hops leads from b to the beam's first edge through edges that are neither padded nor in the beam's visited words,
    with it closed the cycle_len rule; close_dist is not read.  close_dist [W, L, L] / cycle_len [W, L] uint8 per wireframe
    (ops.follow_distance), shared by its beams; one budget in 0..254 per launch.  Everything else, operands and results included,
    is beam_sequence_constrained_select's; "lookahead" with both tables zero gives them bit for bit, width 1
    pointer_sequence_constrained_ahead's."""
    return _beam_sequence_constrained_step(logits, scores, fin, first, prev, visited, width, flags, ntok, tok_sep, tok_eos, follows,
                                           stop, memory, mask, kv_len, groups_per_wireframe, want_rows, want_stats, counter,
                                           _sequence_closure(closure, close_dist, cycle_len, budget))


def _beam_sequence_constrained_step(logits, scores, fin, first, prev, visited, width, flags, ntok, tok_sep, tok_eos, follows, stop,
                                    memory, mask, kv_len, groups_per_wireframe, want_rows, want_stats, counter, ahead):
    """beam_sequence_constrained_select (ahead None) and beam_sequence_constrained_select_ahead (ahead as _lookahead_operands takes
    it): the checks, the outputs and the launch the two share."""
    _dev(logits, "logits"), _dev(scores, "scores")
    out = {}
    if logits.dim() != 2:
        raise ValueError("logits must be a 2-D tensor with unit inner stride")
    B = logits.size(0)
    width = int(width)
    if not 1 <= width <= BEAM_MAX_WIDTH or width > logits.size(1) or B % width:
        raise ValueError("beam width %d: must be in 1..%d, at most S = %d, and divide the %d rows"
                         % (width, BEAM_MAX_WIDTH, logits.size(1), B))
    if stop not in ("all", "best"):
        raise ValueError("stop=%r: must be 'all' or 'best'" % (stop,))
    G = B // width
    gpw = max(G, 1) if groups_per_wireframe is None else int(groups_per_wireframe)
    B, S, spg, nw, E, rows, stats = _step_operands(logits, gpw * width, mask, kv_len, memory, want_rows, want_stats, out)
    flags, ntok, sep, eos = int(flags), int(ntok), int(tok_sep), int(tok_eos)
    L = S - ntok
    fw = (L + 31) // 32
    if flags & ~(_L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT | _L.FF_CONSTRAIN_ONCE):
        raise ValueError("unknown constraint flag bits %d" % flags)
    if flags & _L.FF_CONSTRAIN_ONCE and not flags & _L.FF_CONSTRAIN_NO_REPEAT:
        raise ValueError("FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT")
    if L < 0 or not (0 <= sep < ntok and 0 <= eos < ntok) or sep == eos:
        raise ValueError("tok_sep and tok_eos must be two different tokens below ntok <= S")
    if follows is None and flags & _L.FF_CONSTRAIN_CONNECT:
        raise ValueError("FF_CONSTRAIN_CONNECT needs the follow table")
    if scores.dim() != 1 or scores.numel() != B:
        raise ValueError("scores must hold one fp32 per row of logits")
    for x, name in ((fin, "fin"), (first, "first"), (prev, "prev")):
        _dev(x, name, torch.int32)
        if x.dim() != 1 or x.numel() != B:
            raise ValueError("%s must hold one int32 per row of logits" % name)
    scores, fin, first, prev = scores.contiguous(), fin.contiguous(), first.contiguous(), prev.contiguous()
    _dev(visited, "visited", torch.int32)
    if tuple(visited.shape) != (B, fw):
        raise ValueError("visited must be [%d, %d]" % (B, fw))
    visited = visited.contiguous()
    if follows is not None:
        _dev(follows, "follows", torch.int32)
        if follows.dim() != 3 or not follows.is_contiguous() or follows.size(0) < nw or tuple(follows.shape[1:]) != (L, fw):
            raise ValueError("follows must be a contiguous [>= %d, %d, %d] tensor" % (nw, L, fw))
    dev = logits.device
    i32 = lambda: torch.empty(B, device=dev, dtype=torch.int32)
    out = dict({"parent": i32(), "next": i32(), "scores": torch.empty(B, device=dev, dtype=torch.float32), "fin": i32(),
                "dead_end": i32(), "open": i32(), "first": i32(), "prev": i32(),
                "visited": torch.empty((B, fw), device=dev, dtype=torch.int32),
                "mask_rows": torch.zeros((B, S), device=dev, dtype=torch.uint8)}, **out)
    if counter is not None:
        _dev(counter, "counter", torch.int32)
    # (L = 0: no edge key, nothing of the table or the visited words is read -- one word each so that the pointers are not null)
    one, two = torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
    fol = one if (follows is not None and not (L and fw)) else follows
    d = _L.BeamSequenceConstrainedStep(
        _p(logits), logits.stride(0), S, _p(mask), _p(kv_len), G, width, gpw, _p(fol), L, flags, ntok, sep, eos,
        1 if stop == "best" else 0, _p(scores), _p(fin), _p(first), _p(prev), _p(visited if fw else one),
        _p(out["scores"]), _p(out["fin"]), _p(out["dead_end"]), _p(out["open"]), _p(out["first"]), _p(out["prev"]),
        _p(out["visited"] if fw else two), _p(out["mask_rows"]), _p(out["parent"]), _p(out["next"]), _p(memory), E, _p(rows), E,
        _p(stats), _p(counter))
    if ahead is None:
        _L.check(_L.load().ff_beam_sequence_constrained_select(C.byref(d), _stream()), "ff_beam_sequence_constrained_select")
        return out
    # (ONCE is this rule's own bit: the look-aheads' flag checks are about the other two)
    form, close_dist, cycle_len, budget = _lookahead_operands(ahead, flags & ~_L.FF_CONSTRAIN_ONCE, S, L, nw, dev,
                                                              "beam_sequence_constrained_select_ahead")
    _L.check(_L.load().ff_beam_sequence_constrained_select_ahead(C.byref(d), form, _p(close_dist), _p(cycle_len), budget, _stream()),
             "ff_beam_sequence_constrained_select_ahead")
    return out


@_on_tensor_device
def gather_rows(memory, tok, seqs_per_group=1):
    _dev(memory, "memory"), _dev(tok, "tok", torch.int32)
    N, S, E = memory.shape
    out = torch.empty((tok.numel(), E), device=memory.device, dtype=torch.float32)
    _L.check(_L.load().ff_gather_rows(_p(memory.contiguous()), S, E, _p(tok), tok.numel(),
                                      seqs_per_group, _p(out), E, _stream()), "ff_gather_rows")
    return out


def set_attention_algo(algo):
    """0 automatic, 1 block-shared LDS staging, 2 wave-independent, 3 K/V-resident, 4 the 2 x fp16 kernel (attention() then splits
    K | V itself when the caller gives no planes); returns the previous value."""
    global _attn_algo
    _attn_algo = int(algo)
    return _L.load().ff_set_attention_algo(int(algo))


def set_tuning(name, value):
    """One tuning knob of the library (include/faceformer_hip.h: ff_set_tuning), e.g. set_tuning("FF_L0_FOLD", 0);
    returns the previous value.  Process-wide; a decode snapshots the knobs that shape it when it starts."""
    import ctypes
    lib, old = _L.load(), ctypes.c_int(0)
    _L.check(lib.ff_get_tuning(name.encode(), ctypes.byref(old)), "ff_get_tuning")
    _L.check(lib.ff_set_tuning(name.encode(), int(value)), "ff_set_tuning")
    return old.value


def get_tuning(name):
    import ctypes
    v = ctypes.c_int(0)
    _L.check(_L.load().ff_get_tuning(name.encode(), ctypes.byref(v)), "ff_get_tuning")
    return v.value


def reset_tuning():
    """Every knob back to its built-in default."""
    _L.check(_L.load().ff_reset_tuning(), "ff_reset_tuning")


def set_gemm_tuning(min_units=2, two_per_cu_units=2048, fix_tenths=25, small_max_rows=1024):
    """Launch shape of the stream-K projection kernel and row limit of the small-M kernel (see
    include/faceformer_hip.h); no arguments = the defaults."""
    _L.check(_L.load().ff_set_gemm_tuning(int(min_units), int(two_per_cu_units), int(fix_tenths),
                                          int(small_max_rows)), "ff_set_gemm_tuning")


SPLIT_KINDS = {"bf16x3": 0, "fp16x2": 1, "fp16": 2}     # ff_model.split_kind ("fp16": one fp16 product, opt-in)
_SPLIT_TABLE = {"bf16x3": (3, torch.bfloat16, "ff_split_weight_bf16x3"),     # kind: (terms, plane dtype, entry point)
                "fp16x2": (2, torch.float16, "ff_split_weight_fp16x2"),
                "fp16": (1, torch.float16, "ff_split_weight_fp16")}


@_on_tensor_device
def split_weight(weight, kind="bf16x3"):
    """[N, K] fp32 matrix -> its split planes in the K-blocked layout [terms, K/16, N, 16]: three bf16 planes ("bf16x3",
    planes_to_matrix(planes) == weight up to 2^-25 relative), two fp16 planes ("fp16x2": w1 = fp16(w), w2' = fp16((w - w1) 2^11),
    22 mantissa bits; |w| must be < 65504) or ONE fp16 plane ("fp16": fp16(w), plane 0 of "fp16x2"; one fp16 product)."""
    weight, ldw = _rows(weight, "weight")
    N, K = weight.shape
    if K % 16:
        raise ValueError("split_weight: K must be a multiple of 16")
    if kind not in _SPLIT_TABLE:
        raise ValueError("split_weight: kind must be one of %s" % sorted(SPLIT_KINDS))
    terms, dtype, entry = _SPLIT_TABLE[kind]
    planes = torch.empty((terms, K // 16, N, 16), device=weight.device, dtype=dtype)
    _L.check(getattr(_L.load(), entry)(_p(weight), ldw, N, K, planes.data_ptr(), _stream()), entry)
    return planes


def planes_to_matrix(planes):
    """Inverse of split_weight (fp64 sum of the terms), [rows, K]."""
    kb, rows = planes.size(1), planes.size(2)
    p = planes.double()
    if planes.dtype == torch.float16:
        total = p[0] if planes.size(0) == 1 else p[0] + p[1] / 2048.0   # (one plane: kind "fp16", fp16(w) itself)
    else:
        total = p.sum(0)
    return total.permute(1, 0, 2).reshape(rows, kb * 16)


def _check_planes(p, what):
    ok = (p.dtype == torch.bfloat16 and p.size(0) == 3) or (p.dtype == torch.float16 and p.size(0) in (1, 2))
    if not ok or p.dim() != 4 or p.size(3) != 16 or not p.is_contiguous():
        raise ValueError("linear_x3: %s must be a contiguous [3, K/16, rows, 16] bf16 or [2 or 1, K/16, rows, 16] fp16 tensor "
                         "(split_weight)" % what)


def _split_fn(planes, lib, suffix=""):
    """The kernel entry point of a plane set: ff_gemm_x3 (bf16 x 3), ff_gemm_x2h (fp16 x 2) or ff_gemm_h1 (one fp16 plane)."""
    name = "ff_gemm_x3" if planes.dtype == torch.bfloat16 else ("ff_gemm_h1" if planes.size(0) == 1 else "ff_gemm_x2h")
    return getattr(lib, name + suffix), name + suffix


@_on_tensor_device
def linear_x3(x, planes, bias=None, act=0, residual=None, x2=None, n_split=0, out=None):
    """linear() on the bf16 matrix cores with fp32 accuracy; `planes` comes from split_weight() (one fp16 plane, kind "fp16":
    ff_gemm_h1, one fp16 product with fp32 accumulation)."""
    _check_planes(planes, "planes")
    N, K = planes.size(2), planes.size(1) * 16
    x, lda = _rows(x, "x")
    M = x.size(0)
    if x.size(1) != K:
        raise ValueError("linear_x3: x is [%d,%d] but the weight is [%d,%d]" % (M, x.size(1), N, K))
    if x2 is not None:
        x2, lda2 = _rows(x2, "x2")
        if x2.shape != x.shape or lda2 != lda:
            raise ValueError("linear_x3: x2 must match x")
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32)
    out, ldc = _rows(out, "out")
    ldr = 0
    if residual is not None:
        residual, ldr = _rows(residual, "residual")
    if bias is not None:
        _dev(bias, "bias")
    lib = _L.load()
    fn, who = _split_fn(planes, lib)
    _L.check(fn(_p(x), lda, _p(x2), n_split, planes.data_ptr(), _p(bias), _p(residual), ldr,
                _p(out), ldc, M, N, K, act, _stream()), who)
    return out
