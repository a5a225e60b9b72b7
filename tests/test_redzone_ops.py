"""GPU: every C-ABI kernel inside poisoned surroundings (helper: tests/redzone.py).

Every case runs the same call twice with the same geometry (offsets, leading dimensions, alignment: no dispatch decision can
differ): once with all operands and outputs embedded in ZERO bytes, once in POISON bytes (0xFF: NaN as fp32 / fp16 / bf16, -1
as int32, 255 as uint8).  Then
  (a) the outputs of the two runs are bit-equal -- nothing outside an operand reached a result,
  (b) both guards are intact -- nothing was stored outside an output, ld gaps included,
  (c) the POISON run meets the op's existing fp64 bar (tests/test_hip_ops.py: 3e-6 GEMM, 5e-6 attention, 2e-6 LayerNorm, 4e-7
      gelu, exact copies; the pointer-head ops by the rules of their own test files).
Every 2-D operand and output whose entry takes a leading dimension has ld = columns + 8.  Outputs an ops.py wrapper allocates
itself are embedded too: the ops go through the C ABI directly (lib), or -- where the wrapper's argument checks are wanted --
through the wrapper with its allocations (torch.empty / zeros / full inside faceformer_amd.hip.ops) redirected into the guard."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import redzone as RZ
from test_hip_ops import _ref_attention_general, _seg_stats, ref_attention, rel_err, rnd

pytestmark = pytest.mark.gpu
PAD = 8


@pytest.fixture(scope="module")
def ops(hip_lib):
    from faceformer_amd.hip import ops as _ops
    return _ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _GuardedTorch:
    """Stands in for the `torch` name inside faceformer_amd.hip.ops: the allocation calls return guarded embeds (an `empty`
    tensor holds the guard's fill, so an element a kernel leaves unwritten differs between the two runs), everything else is
    torch's."""

    def __init__(self, guard):
        self._g = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def _make(self, shape, dtype, value):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        dtype = dtype or torch.float32
        n = 1
        for s in shape:
            n *= int(s)
        isz = torch.empty(0, dtype=dtype).element_size()
        t = self._g.bytes(n * isz, name="allocated %s %s" % (dtype, shape)).view(dtype).view(shape)
        if value is not None:
            t.fill_(value)
        return t

    def empty(self, *shape, device=None, dtype=None):
        return self._make(shape, dtype, None)

    def zeros(self, *shape, device=None, dtype=None):
        return self._make(shape, dtype, 0)

    def full(self, shape, value, device=None, dtype=None):
        return self._make((shape,), dtype, value)

    def empty_like(self, x, memory_format=None):
        return self._make((x.shape,), x.dtype, None)


@contextlib.contextmanager
def _guarded_allocations(guard):
    from faceformer_amd.hip import ops as _ops
    _ops.torch = _GuardedTorch(guard)
    try:
        yield
    finally:
        _ops.torch = torch


def twice(run, what):
    """run(guard) -> {name: output tensor}, under a ZERO and a POISON guard: (a) and (b); returns the POISON run's outputs."""
    outs = []
    for fill in (RZ.ZERO, RZ.POISON):
        g = RZ.Guard(fill)
        with _guarded_allocations(g):
            res = run(g)
        g.check()
        outs.append({k: v.detach().clone() for k, v in res.items() if torch.is_tensor(v)})
    assert outs[0] and outs[0].keys() == outs[1].keys(), what
    for k in outs[0]:
        RZ.assert_same_bits(outs[0][k], outs[1][k], "%s: %s" % (what, k))
    return outs[1]


# ---- f32 GEMM family ----------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 512, 512), (65, 100, 36), (130, 96, 100), (333, 260, 512)]
HYBRID_SHAPE = (2100, 260, 512)      # more tiles than one round of blocks: the stream-K / hybrid launch shape


def _gemm_variants(call, M, N, K, split_unit, what, bar=3e-6):
    """plain, bias, bias + ReLU, bias + ReLU + residual aliased to the output, split A (columns from n_split on read x2)."""
    a, a2 = rnd(M, K, seed=1), rnd(M, K, seed=5)
    w, bias, res = rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3), rnd(M, N, seed=4)
    prod = a.double() @ w.double().t()
    n_split = split_unit * max(1, N // (2 * split_unit)) if N > split_unit else 0
    variants = [("plain", None, 0, False, 0, prod), ("bias", bias, 0, False, 0, prod + bias.double()),
                ("relu", bias, 1, False, 0, torch.relu(prod + bias.double())),
                ("residual", bias, 1, True, 0, torch.relu(prod + bias.double()) + res.double())]
    if n_split:
        ref = torch.cat([prod[:, :n_split], a2.double() @ w.double()[n_split:].t()], dim=1) + bias.double()
        variants.append(("split_a", bias, 0, False, n_split, ref))
    for name, b, act, alias, ns, ref in variants:
        def run(g):
            A, Wt = g.embed(a, ld=K + PAD, name="A"), g.embed(w, ld=K + PAD, name="W")
            out = g.embed(res if alias else torch.zeros(M, N), ld=N + PAD, name="C")
            call(A, Wt, g.opt(b, name="bias"), act, out if alias else None, g.embed(a2, ld=K + PAD, name="A2") if ns else None, ns, out)
            return {"out": out}
        got = twice(run, "%s %s" % (what, name))
        assert rel_err(got["out"], ref) < bar, (what, name)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6, 7, 9, 10])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_f32(ops, M, N, K, tile):
    call = lambda A, W, b, act, res, A2, ns, out: ops.linear(A, W, b, act=act, residual=res, x2=A2, n_split=ns, tile=tile, out=out)
    _gemm_variants(call, M, N, K, 128 if N >= 256 else 64, "ff_gemm_f32 tile %d (%d, %d, %d)" % (tile, M, N, K))


@pytest.mark.parametrize("tile", [0, 7])
def test_gemm_f32_hybrid_launch_shape(ops, tile):
    M, N, K = HYBRID_SHAPE
    call = lambda A, W, b, act, res, A2, ns, out: ops.linear(A, W, b, act=act, residual=res, x2=A2, n_split=ns, tile=tile, out=out)
    _gemm_variants(call, M, N, K, 128, "ff_gemm_f32 tile %d (%d, %d, %d)" % (tile, M, N, K))


@pytest.mark.parametrize("tile", [11, 12])
@pytest.mark.parametrize("M,N,K", [(1, 96, 64), (65, 260, 512), (130, 96, 64), HYBRID_SHAPE])
def test_gemm_f32_lds_dma(ops, M, N, K, tile):
    call = lambda A, W, b, act, res, A2, ns, out: ops.linear(A, W, b, act=act, residual=res, x2=A2, n_split=ns, tile=tile, out=out)
    _gemm_variants(call, M, N, K, 128, "ff_gemm_f32 tile %d (%d, %d, %d)" % (tile, M, N, K))


# ---- split products -----------------------------------------------------------------------------------------------------------------
def _h(x):
    return x.half().double()


@pytest.mark.parametrize("shape", [0, 1, 2], ids=lambda s: "shape%d" % s)
@pytest.mark.parametrize("kind", ["bf16x3", "fp16x2", "fp16"])
@pytest.mark.parametrize("M,N,K", [(1, 512, 512), (77, 96, 64), (333, 260, 512)])
def test_gemm_split_products(ops, M, N, K, kind, shape):
    """ops.split_weight writes its planes into a guarded buffer of exactly their size (its torch.empty is redirected), then
    ops.linear_x3 in every variant.  "fp16" is ONE fp16 product: its bar is test_fp16_mode's (fp32 accumulation of K exact
    products of the fp16-rounded operands), the other kinds meet the f32 GEMM's 3e-6."""
    assert set(ops.SPLIT_KINDS) == {"bf16x3", "fp16x2", "fp16"}
    a, a2 = rnd(M, K, seed=1), rnd(M, K, seed=5)
    w, bias, res = rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3), rnd(M, N, seed=4)
    n_split = 128 * (N // 256)
    r = _h if kind == "fp16" else (lambda x: x.double())
    prod = r(a) @ r(w).t()
    den = r(a).abs() @ r(w).abs().t()
    variants = [("plain", None, 0, False, 0, prod), ("relu", bias, 1, False, 0, torch.relu(prod + bias.double())),
                ("residual", bias, 1, True, 0, torch.relu(prod + bias.double()) + res.double())]
    if n_split:
        variants.append(("split_a", bias, 0, False, n_split,
                         torch.cat([prod[:, :n_split], r(a2) @ r(w)[n_split:].t()], dim=1) + bias.double()))
    den_split = torch.cat([den[:, :n_split], r(a2).abs() @ r(w).abs()[n_split:].t()], dim=1)
    ops.set_x3_tuning(shape)
    try:
        for name, b, act, alias, ns, ref in variants:
            def run(g):
                planes = ops.split_weight(g.embed(w, ld=K + PAD, name="W"), kind)          # (guarded: its torch.empty)
                out = g.embed(res if alias else torch.zeros(M, N), ld=N + PAD, name="C")
                ops.linear_x3(g.embed(a, ld=K + PAD, name="A"), planes, g.opt(b, name="bias"), act=act, residual=out if alias else None,
                              x2=g.embed(a2, ld=K + PAD, name="A2") if ns else None, n_split=ns, out=out)
                return {"out": out, "planes": planes.view(torch.int16)}
            got = twice(run, "linear_x3 %s shape %d (%d, %d, %d) %s" % (kind, shape, M, N, K, name))
            if kind == "fp16":
                err = (got["out"].cpu().double() - ref).abs()
                bar = K * 2.0 ** -24 * (den_split if ns else den) + 2.0 ** -22 * ref.abs() + 2.0 ** -40
                assert bool((err <= bar).all()), (name, float((err / bar).max()))
            else:
                assert rel_err(got["out"], ref) < 3e-6, name
    finally:
        ops.set_x3_tuning(0)


# ---- LayerNorm-fused forms ----------------------------------------------------------------------------------------------------------
LN_SHAPES = [(37, 512, 512), (300, 512, 1024), (640, 128, 256)]


def _ln_call(ops, family, kind):
    """(emit, consume): the f32 family's ff_gemm_f32_ln or the split products' ff_gemm_x3_ln / x2h_ln / h1_ln."""
    if family == "f32":
        return (lambda A, W, **kw: ops.linear_ln(A, W, **kw)), (lambda x, Wf, in_epilogue, **kw: ops.linear_ln(x, Wf, **kw))

    def consume(x, Wf, in_epilogue, **kw):
        cs = None
        if in_epilogue:
            cs = Wf.double().sum(dim=1).float().contiguous()
            cs = kw.pop("guard").embed(cs.cpu(), name="colsum")
        kw.pop("guard", None)
        return ops.linear_x3_ln(x, ops.split_weight(Wf, kind), colsum=cs, **kw)
    return (lambda A, W, **kw: ops.linear_x3_ln(A, ops.split_weight(W, kind), **kw)), consume


@pytest.mark.parametrize("family,kind", [("f32", None), ("split", "bf16x3"), ("split", "fp16x2")])
@pytest.mark.parametrize("M,N,K", LN_SHAPES)
def test_gemm_ln_emits_segment_statistics(ops, M, N, K, family, kind):
    """Producer form: C = A W^T + b + residual and the (mean, M2) of every 32-column segment of the stored C -- the bars of
    test_gemm_emits_layernorm_segment_statistics.  The statistics output is the wrapper's torch.full, embedded."""
    gen = torch.Generator().manual_seed(M + N + K)
    A, W, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen)
    res = 3.0 + 2.0 * torch.randn(M, N, generator=gen)
    emit, _ = _ln_call(ops, family, kind)

    def run(g):
        out = g.embed(torch.zeros(M, N), ld=N + PAD, name="C")
        _, stats = emit(g.embed(A, ld=K + PAD, name="A"), g.embed(W, ld=K + PAD, name="W"), bias=g.embed(b, name="bias"),
                        residual=g.embed(res, ld=N + PAD, name="residual"), want_stats=True, out=out)
        return {"out": out, "stats": stats}
    got = twice(run, "ln emit %s %s (%d, %d, %d)" % (family, kind, M, N, K))
    ref = A.double() @ W.double().t() + b.double() + res.double()
    out, stats = got["out"].cpu().double(), got["stats"].cpu().double()
    assert (out - ref).abs().max() < 2e-5 * ref.abs().max()
    want = _seg_stats(out)
    assert not torch.isnan(stats).any()
    assert (stats[..., 0] - want[..., 0]).abs().max() < 1e-5
    assert ((stats[..., 1] - want[..., 1]).abs() / want[..., 1].clamp_min(1e-6)).max() < 1e-5


@pytest.mark.parametrize("family,kind,in_epilogue", [("f32", None, False), ("split", "bf16x3", False), ("split", "bf16x3", True),
                                                     ("split", "fp16x2", False), ("split", "fp16x2", True)])
@pytest.mark.parametrize("M,N,K,div", [(37, 512, 512, 5), (300, 512, 1024, 7), (640, 128, 256, 64)])
def test_gemm_ln_consumes_segment_statistics(ops, M, N, K, div, family, kind, in_epilogue):
    """Consumer form: act((LN(x) + pos[row // div]) W^T + b) from raw x, its statistics, the folded weight / bias and the
    pos W^T table; rows normalised first, or (split products) in the epilogue with the row sums of the folded weight -- the
    bar of test_gemm_consumes_layernorm_statistics_with_folded_weights.  x, stats_in and row_table are embedded.  The split
    products' normalising form is built for K = 512 and the f32 family's for K <= 512: elsewhere the library refuses the call
    (and stores nothing)."""
    gen = torch.Generator().manual_seed(M * 3 + N + K)
    x = (1.5 + 2.0 * torch.randn(M, K, generator=gen)) * (1.0 + torch.rand(M, 1, generator=gen))
    W, b = torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen)
    gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=gen), 0.3 * torch.randn(K, generator=gen)
    pos = torch.randn((M + div - 1) // div, K, generator=gen)
    pos_cols = N // 2 if N >= 1024 else N
    Wf, bf, P = (t.cpu() for t in ops.fold_layernorm_linear(W.cuda(), b.cuda(), gamma.cuda(), beta.cuda(), pos.cuda(), pos_cols))
    stats = _seg_stats(x.double()).float().contiguous()
    _, consume = _ln_call(ops, family, kind)

    def run(g):
        out = g.embed(torch.zeros(M, N), ld=N + PAD, name="C")
        kw = dict(guard=g) if family == "split" else {}
        consume(g.embed(x, ld=K + PAD, name="x"), g.embed(Wf, ld=K + PAD, name="Wf"), in_epilogue, bias=g.embed(bf, name="bf"), act=1,
                stats_in=g.embed(stats, name="stats_in"), row_table=g.embed(P, ld=pos_cols + PAD, name="row_table"), row_div=div,
                row_cols=pos_cols, out=out, **kw)
        return {"out": out}
    if (family == "split" and K != 512) or K > 512:
        g = RZ.Guard(RZ.POISON)
        with pytest.raises(ops._L.HipExtensionError), _guarded_allocations(g):
            run(g)
        g.check()
        return
    got = twice(run, "ln consume %s %s epilogue=%s (%d, %d, %d)" % (family, kind, in_epilogue, M, N, K))
    ln = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5)
    addp = torch.zeros(M, N, dtype=torch.float64)
    addp[:, :pos_cols] = pos.double()[torch.arange(M) // div] @ W.double()[:pos_cols].t()
    ref = torch.relu(ln @ W.double().t() + b.double() + addp)
    assert (got["out"].cpu().double() - ref).abs().max() < 3e-5 * max(1.0, float(ref.abs().max()))


def test_fold_layernorm_linear(ops):
    """ff_fold_layernorm_linear with and without the position table: Wf, bf and P are the wrapper's allocations, embedded."""
    N, K, rows, pos_cols = 100, 96, 7, 64
    W, b = rnd(N, K, seed=1, scale=0.1), rnd(N, seed=2)
    gamma, beta, pos = rnd(K, seed=3) + 1.0, rnd(K, seed=4), rnd(rows, K, seed=5)
    for with_pos in (True, False):
        def run(g):
            Wf, bf, P = ops.fold_layernorm_linear(g.embed(W, ld=K + PAD, name="W"), g.embed(b), g.embed(gamma), g.embed(beta),
                                                  g.embed(pos, ld=K + PAD, name="pos") if with_pos else None, pos_cols if with_pos else 0)
            return {"Wf": Wf, "bf": bf, "P": P}
        got = twice(run, "ff_fold_layernorm_linear pos=%s" % with_pos)
        assert rel_err(got["Wf"], W.double() * gamma.double()) < 3e-6
        assert rel_err(got["bf"], b.double() + W.double() @ beta.double()) < 3e-6
        if with_pos:
            assert rel_err(got["P"], pos.double() @ W.double()[:pos_cols].t()) < 3e-6


# ---- attention with 64-wide heads -----------------------------------------------------------------------------------------------------
ALGOS = {0: "auto", 1: "lds", 2: "wave", 3: "resident", 4: "x2h"}


@pytest.fixture(params=list(ALGOS), ids=["attn-%s" % v for v in ALGOS.values()])
def attn_algo(ops, request):
    old = ops.set_attention_algo(request.param)
    yield request.param
    ops.set_attention_algo(old)


def _masks(G, nk):
    """(mask [G, nk] bool, kv_len [G] int32) of test_attention_group_major_with_mask: a short kv_len and a hole per group."""
    mask = torch.zeros(G, nk, dtype=torch.bool)
    kv_len = torch.full((G,), nk, dtype=torch.int32)
    for g in range(G):
        cut = max(1, nk - 3 * g - (nk // 4))
        mask[g, cut:] = True
        kv_len[g] = cut
        if cut > 2:
            mask[g, 1] = True
    return mask, kv_len


def _group_major(ops, g, q, k, v, G, H, nq, nk, mask, kv_len):
    E = H * 64
    out = g.embed(torch.zeros(G * nq, E), ld=E + PAD, name="out")
    ops.attention(g.embed(q, ld=E + PAD, name="q"), g.embed(k, ld=E + PAD, name="k"), g.embed(v, ld=E + PAD, name="v"), G, H, nq, nk,
                  q_group_stride=nq, q_inner=nq, q_outer_stride=0, k_group_stride=nk, k_stride=1,
                  kv_len=g.embed(kv_len, name="kv_len"), key_mask=g.embed(mask.to(torch.uint8), name="key_mask"), out=out)
    return {"out": out}


@pytest.mark.parametrize("G,H,nq,nk", [(4, 1, 1, 1), (2, 2, 33, 33), (3, 2, 5, 100), (1, 1, 65, 129)])
def test_attention_group_major(ops, attn_algo, G, H, nq, nk):
    E = H * 64
    q, k, v = rnd(G * nq, E, seed=1), rnd(G * nk, E, seed=2), rnd(G * nk, E, seed=3)
    mask, kv_len = _masks(G, nk)
    got = twice(lambda g: _group_major(ops, g, q, k, v, G, H, nq, nk, mask, kv_len), "attention group-major %s" % ALGOS[attn_algo])
    qd, kd, vd = (t.double().view(G, -1, H, 64).transpose(1, 2) for t in (q, k, v))
    assert rel_err(got["out"], ref_attention(qd, kd, vd, mask).transpose(1, 2).reshape(G * nq, E)) < 5e-6


@pytest.mark.parametrize("t,B,H,causal", [(1, 5, 2, False), (9, 4, 2, True), (41, 3, 2, False), (37, 129, 8, False)])
def test_attention_position_major_self(ops, attn_algo, t, B, H, causal):
    """Decoder self-attention: rows = j * B + b, q | k | v views of ONE packed parent (ld = 3E + 8)."""
    E = H * 64
    qkv = rnd(t * B, 3 * E, seed=5)

    def run(g):
        d = g.embed(qkv, ld=3 * E + PAD, name="qkv")
        out = g.embed(torch.zeros(t * B, E), ld=E + PAD, name="out")
        ops.attention(d[:, :E], d[:, E:2 * E], d[:, 2 * E:], B, H, t, t, q_group_stride=1, q_inner=1, q_outer_stride=B,
                      k_group_stride=1, k_stride=B, causal=causal, out=out)
        return {"out": out}
    got = twice(run, "attention self %s" % ALGOS[attn_algo])
    x = qkv.double().view(t, B, 3, H, 64).permute(2, 1, 3, 0, 4)
    assert rel_err(got["out"], ref_attention(x[0], x[1], x[2], None, causal).permute(2, 0, 1, 3).reshape(t * B, E)) < 5e-6


@pytest.mark.parametrize("t,F,W,S", [(1, 3, 2, 30), (5, 7, 3, 50), (36, 33, 2, 260), (2, 65, 2, 516)])
def test_attention_cross_shared_kv(ops, attn_algo, t, F, W, S):
    """Decoder cross-attention: the F sequences of a wireframe share its K | V (one packed parent); up to 288 keys the resident
    and 2 x fp16 kernels, above them the block-shared one."""
    H, E = 8, 512
    B = W * F
    q, kv = rnd(t * B, E, seed=1), rnd(W * S, 2 * E, seed=2)
    mask = torch.zeros(W, S, dtype=torch.bool)
    kv_len = torch.full((W,), S, dtype=torch.int32)
    for w in range(W):
        mask[w, S - 5 * w - 3:] = True
        kv_len[w] = S - 5 * w - 3

    def run(g):
        d = g.embed(kv, ld=2 * E + PAD, name="kv")
        out = g.embed(torch.zeros(t * B, E), ld=E + PAD, name="out")
        ops.attention(g.embed(q, ld=E + PAD, name="q"), d[:, :E], d[:, E:], W, H, F * t, S, q_group_stride=F, q_inner=F,
                      q_outer_stride=B, k_group_stride=S, k_stride=1, kv_len=g.embed(kv_len, name="kv_len"),
                      key_mask=g.embed(mask.to(torch.uint8), name="key_mask"), out=out)
        return {"out": out}
    got = twice(run, "attention cross %s" % ALGOS[attn_algo])
    qd = q.double().view(t, W, F, H, 64).permute(1, 3, 0, 2, 4).reshape(W, H, t * F, 64)
    kd, vd = (kv[:, c:c + E].double().view(W, S, H, 64).transpose(1, 2) for c in (0, E))
    ref = ref_attention(qd, kd, vd, mask).view(W, H, t, F, 64).permute(2, 0, 3, 1, 4).reshape(t * B, E)
    assert rel_err(got["out"], ref) < 5e-6


@pytest.mark.parametrize("G,H,nk", [(3, 2, 100), (1, 8, 288), (2, 1, 1)])
def test_attention_split_kv_stays_inside_its_planes(ops, G, H, nk):
    """ops.split_kv writes into a guarded buffer of exactly ff_attention_planes_bytes(G, H) bytes (its torch.empty, redirected);
    the 2 x fp16 kernel then reads those planes: every byte it uses was written (the two fills give the same bits)."""
    E = H * 64
    q, k, v = rnd(G * 7, E, seed=1), rnd(G * nk, E, seed=2), rnd(G * nk, E, seed=3)
    old = ops.set_attention_algo(4)
    try:
        def run(g):
            dk, dv = g.embed(k, ld=E + PAD, name="k"), g.embed(v, ld=E + PAD, name="v")
            planes = ops.split_kv(dk, dv, G, H, nk, nk, 1)
            assert planes.numel() == int(ops._L.load().ff_attention_planes_bytes(G, H))
            out = g.embed(torch.zeros(G * 7, E), ld=E + PAD, name="out")
            ops.attention(g.embed(q, ld=E + PAD, name="q"), dk, dv, G, H, 7, nk, q_group_stride=7, q_inner=7, q_outer_stride=0,
                          k_group_stride=nk, k_stride=1, kv_planes=planes, out=out)
            return {"out": out}
        got = twice(run, "split_kv")
    finally:
        ops.set_attention_algo(old)
    qd, kd, vd = (t.double().view(G, -1, H, 64).transpose(1, 2) for t in (q, k, v))
    assert rel_err(got["out"], ref_attention(qd, kd, vd).transpose(1, 2).reshape(G * 7, E)) < 5e-6


def test_attention_masked_key_rows_have_no_effect(ops, attn_algo):
    """Other finite values in the K and V rows at or past kv_len: the output keeps its bits, under every algo (what
    test_attention_x2h_key_count_edges_and_rows_past_kv_len asserts for the 2 x fp16 kernel).  Finite only: the kernels
    document it, and 0 x NaN on a masked key is NaN in torch as well."""
    for G, H, nq, nk in ((3, 2, 5, 100), (2, 2, 33, 33), (2, 8, 40, 300)):
        E = H * 64
        q, k, v = rnd(G * nq, E, seed=1), rnd(G * nk, E, seed=2), rnd(G * nk, E, seed=3)
        kv_len = torch.tensor([max(1, nk - 7 * (g + 1)) for g in range(G)], dtype=torch.int32)
        mask = torch.arange(nk)[None, :] >= kv_len[:, None]
        past = mask.reshape(-1)
        k2, v2 = k.clone(), v.clone()
        k2[past], v2[past] = rnd(int(past.sum()), E, seed=63, scale=300.0), rnd(int(past.sum()), E, seed=64, scale=300.0)
        g = RZ.Guard(RZ.POISON)
        a = _group_major(ops, g, q, k, v, G, H, nq, nk, mask, kv_len)["out"]
        b = _group_major(ops, g, q, k2, v2, G, H, nq, nk, mask, kv_len)["out"]
        g.check()
        RZ.assert_same_bits(a, b, "%s (%d, %d, %d, %d)" % (ALGOS[attn_algo], G, H, nq, nk))
        assert torch.isfinite(a).all()


def test_attention_nan_in_masked_key_rows_block_shared_kernel(ops):
    """NaN in the K and V rows at or past kv_len, tried once per kernel: the block-shared kernel (algo 1) replaces
    the scores of those keys before they are used and never multiplies their V rows -- bit-equal, asserted here and for
    ff_attention_general below.  The wave-independent kernel survives NaN in K only; the K/V-resident and 2 x fp16 kernels
    survive neither (0 x NaN, as torch): not asserted."""
    old = ops.set_attention_algo(1)
    try:
        for G, H, nq, nk in ((3, 2, 5, 100), (2, 2, 33, 33), (2, 8, 40, 300)):
            E = H * 64
            q, k, v = rnd(G * nq, E, seed=1), rnd(G * nk, E, seed=2), rnd(G * nk, E, seed=3)
            kv_len = torch.tensor([max(1, nk - 7 * (g + 1)) for g in range(G)], dtype=torch.int32)
            mask = torch.arange(nk)[None, :] >= kv_len[:, None]
            k2, v2 = k.clone(), v.clone()
            k2[mask.reshape(-1)] = float("nan")
            v2[mask.reshape(-1)] = float("nan")
            g = RZ.Guard(RZ.POISON)
            a = _group_major(ops, g, q, k, v, G, H, nq, nk, mask, kv_len)["out"]
            b = _group_major(ops, g, q, k2, v2, G, H, nq, nk, mask, kv_len)["out"]
            g.check()
            RZ.assert_same_bits(a, b, "block-shared kernel (%d, %d, %d, %d)" % (G, H, nq, nk))
            assert torch.isfinite(a).all()
    finally:
        ops.set_attention_algo(old)


# ---- ff_attention_general -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,H,hd,nq,nk,form", [(2, 3, 48, 5, 37, "bias2d+mask2d"), (1, 2, 128, 33, 70, "bias3d"),
                                               (2, 4, 16, 3, 65, "mask3d"), (2, 3, 48, 5, 37, "plain")])
def test_attention_general(ops, G, H, hd, nq, nk, form):
    E = H * hd
    q, kv = rnd(nq * G, E, seed=1), rnd(nk * G, 2 * E, seed=2)
    keep = torch.tensor([max(1, nk - 3 * g - nk // 4) for g in range(G)])
    kpm = torch.arange(nk)[None, :] >= keep[:, None]
    kpm[:, 1] = True
    bias = amask = None
    if "bias2d" in form:
        bias = rnd(nq, nk, seed=3, scale=2.0)
    if "bias3d" in form:
        bias = rnd(G * H, nq, nk, seed=4, scale=2.0)
    if "mask2d" in form:
        amask = rnd(nq, nk, seed=5) > 0.5
        amask[:, 0] = False
    if "mask3d" in form:
        amask = rnd(G * H, nq, nk, seed=6) > 0.5
        amask[..., 0] = False

    def run(g, kv=kv):
        d = g.embed(kv, ld=2 * E + PAD, name="kv")
        out = g.embed(torch.zeros(nq * G, E), ld=E + PAD, name="out")
        ops.attention_general(g.embed(q, ld=E + PAD, name="q"), d[:, :E], d[:, E:], G, H, hd, nq, nk, q_group_stride=1, q_inner=1,
                              q_outer_stride=G, k_group_stride=1, k_stride=G, kv_len=g.embed(keep.to(torch.int32), name="kv_len"),
                              key_mask=g.embed(kpm.to(torch.uint8), name="key_mask"),
                              attn_bias=g.opt(bias, name="attn_bias"),
                              attn_mask=None if amask is None else g.embed(amask.to(torch.uint8), name="attn_mask"), out=out)
        return {"out": out}
    got = twice(run, "ff_attention_general %s" % form)
    qd = q.double().view(nq, G, H, hd).permute(1, 2, 0, 3)
    kd, vd = (kv[:, c:c + E].double().view(nk, G, H, hd).permute(1, 2, 0, 3) for c in (0, E))
    ref = _ref_attention_general(qd, kd, vd, hd, kpm, False, bias, amask).permute(2, 0, 1, 3).reshape(nq * G, E)
    assert torch.isfinite(got["out"]).all() and rel_err(got["out"], ref) < 5e-6
    # other finite values in the rows at or past kv_len (position-major: row = j * G + g)
    past = (torch.arange(nk)[:, None] >= keep[None, :]).reshape(-1)
    kv2 = kv.clone()
    kv2[past] = rnd(int(past.sum()), 2 * E, seed=9, scale=300.0)
    g = RZ.Guard(RZ.POISON)
    RZ.assert_same_bits(run(g, kv2)["out"], got["out"], "ff_attention_general %s: rows past kv_len" % form)
    kv2[past] = float("nan")                       # this kernel never touches a masked key's K or V row: NaN there as well
    RZ.assert_same_bits(run(g, kv2)["out"], got["out"], "ff_attention_general %s: NaN past kv_len" % form)
    g.check()


# ---- pointer head -------------------------------------------------------------------------------------------------------------------
POINTER_SHAPES = [(3, 7, 44, 512), (2, 5, 70, 128), (1, 1, 5, 64)]
FILL = torch.finfo(torch.float32).min


def _pointer_case(W, F, S, E):
    B = W * F
    p, mem = rnd(B, E, seed=1), rnd(W, S, E, seed=2)
    mask = torch.zeros(W, S, dtype=torch.bool)
    kv_len = torch.full((W,), S, dtype=torch.int32)
    for w in range(W):
        mask[w, S - 2 * w - 1:] = True
        kv_len[w] = S - 2 * w - 1
    raw = torch.einsum("be,bse->bs", p.double(), mem.double()[torch.arange(B) // F])
    return B, p, mem, mask, kv_len, raw


@pytest.mark.parametrize("lp", [False, True], ids=["argmax", "argmax_lp"])
@pytest.mark.parametrize("W,F,S,E", POINTER_SHAPES)
def test_pointer_argmax(ops, W, F, S, E, lp):
    """ff_pointer_argmax / _lp through lib with every output embedded and logits rows S + 8 apart; the rules of
    test_pointer_argmax, and the log-probability within 2^-16 of fp64 log_softmax of the kernel's own logits (test_logprob)."""
    lib = ops._L.load()
    B, p, mem, mask, kv_len, raw = _pointer_case(W, F, S, E)
    extra = (rnd(B, S, seed=7) > 1.0).to(torch.uint8)
    extra[:, 0] = 0

    def run(g):
        o = {"next": g.embed(torch.zeros(B, dtype=torch.int32), name="next"), "best": g.embed(torch.zeros(B), name="best"),
             "second": g.embed(torch.zeros(B), name="second"), "logits": g.embed(torch.zeros(B, S), ld=S + PAD, name="logits"),
             "rows": g.embed(torch.zeros(B, E), ld=E + PAD, name="rows"), "counters": g.embed(torch.zeros(2, dtype=torch.int32), name="counters")}
        args = (g.embed(p, ld=E + PAD, name="p").data_ptr(), E + PAD, g.embed(mem, name="memory").data_ptr(), S, E,
                g.embed(mask.to(torch.uint8), name="mask").data_ptr(), g.embed(kv_len, name="kv_len").data_ptr(),
                g.embed(extra, ld=S + PAD, name="extra_mask").data_ptr(), S + PAD, B, F, o["next"].data_ptr(), o["best"].data_ptr(),
                o["second"].data_ptr(), o["logits"].data_ptr(), S + PAD, o["rows"].data_ptr(), E + PAD, o["counters"].data_ptr(), 4,
                o["counters"].data_ptr() + 4, 3)
        if lp:
            o["logprob"] = g.embed(torch.zeros(B), name="logprob")
            ops._L.check(lib.ff_pointer_argmax_lp(*args, o["logprob"].data_ptr(), _stream()), "ff_pointer_argmax_lp")
        else:
            ops._L.check(lib.ff_pointer_argmax(*args, _stream()), "ff_pointer_argmax")
        return o
    got = {k: v.cpu() for k, v in twice(run, "ff_pointer_argmax").items()}
    dead = mask[torch.arange(B) // F] | extra.bool()
    want = raw.masked_fill(dead, FILL)
    logits = got["logits"].double()
    assert torch.equal(logits[dead], want[dead])
    assert float((logits[~dead] - want[~dead]).abs().max()) < 1e-4 * float(want[~dead].abs().max())
    nxt = got["next"].long()
    assert torch.equal(nxt, torch.argmax(got["logits"], dim=1))
    top2 = torch.sort(got["logits"], dim=1, descending=True).values
    assert torch.equal(got["best"], top2[:, 0]) and torch.equal(got["second"], top2[:, 1])
    assert torch.equal(got["rows"], mem[torch.arange(B) // F, nxt])
    assert got["counters"].tolist() == [int((nxt >= 4).sum()), int((nxt == 3).sum())]
    if lp:
        ref = torch.log_softmax(logits.masked_fill(dead, float("-inf")), dim=1)[torch.arange(B), nxt]
        assert float((got["logprob"].double() - ref).abs().max()) <= 2.0 ** -16


def _same_as_plain(got, plain, what):
    """(c) for the selection ops: the embedded call returns the bits of the same call on plain tight tensors, whose rules
    against the numpy references are asserted in the op's own test file."""
    for k, v in plain.items():
        if torch.is_tensor(v):
            RZ.assert_same_bits(got[k], v, "%s: %s against the plain call" % (what, k))


def _masked_logits(W, F, S, E):
    B, p, mem, mask, kv_len, raw = _pointer_case(W, F, S, E)
    return B, raw.float(), mem, mask.to(torch.uint8), kv_len


@pytest.mark.parametrize("W,F,S,E", POINTER_SHAPES)
def test_pointer_forced(ops, W, F, S, E):
    """ff_pointer_forced: log_softmax(masked row)[forced] within forced_ref.LP_BAR of fp64 on the kernel's own masked row, the
    argmax and the rank exact on it, the gathered rows exact and their segment statistics."""
    import forced_ref as FR
    B, raw, mem, mask, kv_len = _masked_logits(W, F, S, E)
    forced = (torch.arange(B) * 5 % max(1, S - 2 * W - 1)).to(torch.int32)
    forced[0], forced[-1] = 0, int(kv_len[-1]) - 1

    def run(g):
        lg = g.embed(raw, ld=S + PAD, name="logits")
        o = ops.pointer_forced(lg, g.embed(forced, name="forced"), g.embed(mem, name="memory"), g.embed(mask, name="mask"),
                               g.embed(kv_len, name="kv_len"), seqs_per_group=F, want_rows=True, want_stats=E % 32 == 0)
        return dict(o, logits=lg)
    got = {k: v.cpu() for k, v in twice(run, "ff_pointer_forced").items()}
    dead = mask.bool()[torch.arange(B) // F]
    row = got["logits"].double()
    assert torch.equal(row[dead], raw.double().masked_fill(dead, FILL)[dead]) and torch.equal(row[~dead], raw.double()[~dead])
    lsm = torch.log_softmax(row.masked_fill(dead, float("-inf")), dim=1)
    idx = torch.arange(B)
    assert float((got["logprob"].double() - lsm[idx, forced.long()]).abs().max()) <= FR.LP_BAR
    assert torch.equal(got["greedy"].long(), torch.argmax(got["logits"], dim=1))
    mine = got["logits"][idx, forced.long()][:, None]
    before = (got["logits"] > mine) | ((got["logits"] == mine) & (torch.arange(S)[None, :] < forced.long()[:, None]))
    assert torch.equal(got["rank"].long(), before.sum(dim=1))
    assert torch.equal(got["rows"], mem[idx // F, forced.long()])
    if E % 32 == 0:
        want, st = _seg_stats(got["rows"].double()), got["stats"].double()        # (the bars of test_gemm_emits_layernorm_segment_statistics)
        assert (st[..., 0] - want[..., 0]).abs().max() < 1e-5
        assert ((st[..., 1] - want[..., 1]).abs() / want[..., 1].clamp_min(1e-6)).max() < 1e-5


@pytest.mark.parametrize("W,F,S,E", POINTER_SHAPES)
def test_pointer_sample(ops, W, F, S, E):
    B, raw, mem, mask, kv_len = _masked_logits(W, F, S, E)
    u = torch.rand(B + 3, generator=torch.Generator().manual_seed(3))
    row_id = ((torch.arange(B) * 7) % (B + 3)).to(torch.int32)
    fin = (torch.arange(B) % 4 == 3).to(torch.int32)
    kw = dict(temperature=0.8, top_k=5, top_p=0.9, seqs_per_group=F, term_range=(1, 4), want_rows=True, want_stats=E % 32 == 0, ge_bound=4)

    def call(lg, e):
        o = ops.pointer_sample(lg, e(u), row_id=e(row_id), fin=e(fin), memory=e(mem), mask=e(mask), kv_len=e(kv_len),
                               counter=e(torch.zeros(1, dtype=torch.int32)), **kw)
        return dict(o, logits=lg)
    got = twice(lambda g: call(g.embed(raw, ld=S + PAD, name="logits"), g.embed), "ff_pointer_sample")
    _same_as_plain(got, call(raw.cuda(), lambda t: t.cuda()), "ff_pointer_sample")
    assert torch.isfinite(got["logprob"]).all() and bool((got["next"][fin.bool().cuda()] == 0).all())


@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("W,F,S,E", POINTER_SHAPES)
def test_beam_select_and_reorder(ops, W, F, S, E, width):
    if width > S:
        pytest.skip("more beams than keys")
    Wf = W * F
    B = Wf * width
    p, mem = rnd(B, E, seed=1), rnd(W, S, E, seed=2)
    mask = torch.zeros(W, S, dtype=torch.uint8)
    kv_len = torch.full((W,), S, dtype=torch.int32)
    for w in range(W):
        mask[w, S - 2 * w - 1:] = 1
        kv_len[w] = S - 2 * w - 1
    raw = torch.einsum("be,bse->bs", p, mem[torch.arange(B) // (F * width)])
    scores = -rnd(B, seed=4).abs()
    fin = (torch.arange(B) % 5 == 4).to(torch.int32)
    t = 2
    hist = torch.arange((t + 1) * B, dtype=torch.int32).view(t + 1, B) % S

    def call(lg, e, hist_ld=None):
        h = e(hist) if hist_ld is None else hist_ld
        o = ops.beam_select(lg, e(scores), e(fin), width, groups_per_wireframe=F, mask=e(mask), kv_len=e(kv_len), hist=h, t=t,
                            term_range=(1, 4), memory=e(mem), want_rows=True, counter=e(torch.zeros(1, dtype=torch.int32)), ge_bound=4)
        return dict(o, logits=lg, hist=h)
    got = twice(lambda g: call(g.embed(raw, ld=S + PAD, name="logits"), g.embed, g.embed(hist, ld=B + PAD, name="hist")), "ff_beam_select")
    plain = call(raw.cuda(), lambda x: x.cuda())
    _same_as_plain(got, plain, "ff_beam_select")
    # ff_beam_reorder: cached prefixes [npos, B, w] permuted in place by the parents just selected
    a, b = rnd(t, B, 64, seed=8), rnd(t, B, 12, seed=9)          # (rows of both are multiples of 16 bytes)

    def reorder(g):
        ra, rb = g.embed(a, name="rows_a"), g.embed(b, name="rows_b")
        ops.beam_reorder(ra, g.embed(plain["parent"].cpu(), name="parent"), width, rows_b=rb)
        return {"rows_a": ra, "rows_b": rb}
    got = twice(reorder, "ff_beam_reorder")
    src = (torch.arange(B) // width * width + plain["parent"].cpu().long())
    assert torch.equal(got["rows_a"].cpu(), a[:, src]) and torch.equal(got["rows_b"].cpu(), b[:, src])


@pytest.mark.parametrize("W,F,S,E", POINTER_SHAPES)
def test_follow_table_and_pointer_constrained(ops, W, F, S, E):
    import constrain_ref as CR
    from faceformer_amd import faces
    ntok = 4
    L = S - ntok
    B, raw, mem, mask, kv_len = _masked_logits(W, F, S, E)
    pts = (torch.randint(0, 4, (W, L, 2, 2), generator=torch.Generator().manual_seed(5)).float() * 0.25)
    starts, ends = pts[:, :, 0].contiguous(), pts[:, :, 1].contiguous()
    ni = torch.tensor([max(1, L - 3 * w) for w in range(W)], dtype=torch.int32)
    got = twice(lambda g: {"bits": ops.follow_table(g.embed(starts, name="starts"), g.embed(ends, name="ends"), g.embed(ni, name="num_input"),
                                                     CR.TOL)}, "ff_follow_table")
    want = faces.pack_follow_bits(faces.follow_table((starts.numpy(), ends.numpy()), CR.TOL, ni.tolist()))
    assert np.array_equal(got["bits"].cpu().numpy(), want)
    follows = got["bits"].cpu()
    fw = (L + 31) // 32
    fin = (torch.arange(B) % 4 == 3).to(torch.int32)
    first = (torch.arange(B) % max(1, L)).to(torch.int32)
    prev = ((torch.arange(B) * 3) % max(1, L)).to(torch.int32)
    vis = np.zeros((B, fw), dtype=np.uint32)
    for b in range(B):
        for e_ in (int(first[b]), int(prev[b])):
            vis[b, e_ >> 5] |= np.uint32(1 << (e_ & 31))
    visited = torch.from_numpy(vis.view(np.int32))
    flags = CR.NO_REPEAT | CR.CONNECT

    def call(lg, e):
        o = ops.pointer_constrained(lg, e(fin), e(first), e(prev), e(visited), flags, ntok, follows=e(follows), memory=e(mem),
                                    mask=e(mask), kv_len=e(kv_len), seqs_per_group=F, term_range=(1, 4), want_rows=True,
                                    want_stats=E % 32 == 0, counter=e(torch.zeros(1, dtype=torch.int32)))
        return dict(o, logits=lg)
    got = twice(lambda g: call(g.embed(raw, ld=S + PAD, name="logits"), g.embed), "ff_pointer_constrained")
    _same_as_plain(got, call(raw.cuda(), lambda x: x.cuda()), "ff_pointer_constrained")
    assert torch.isfinite(got["logprob"]).all()


# ---- row ops ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pos", [False, True], ids=["plain", "pos"])
@pytest.mark.parametrize("rows", [1, 5, 37])
@pytest.mark.parametrize("E", [64, 128, 512, 2048])
def test_layernorm(ops, E, rows, with_pos):
    lib = ops._L.load()
    x = rnd(rows, E, seed=1, scale=3.0) + 0.5
    gam, bet = rnd(E, seed=2) + 1.0, rnd(E, seed=3)
    div, mod = 4, 7
    pos = rnd(mod, E, seed=4)

    def run(g):
        y, yp = g.embed(torch.zeros(rows, E), ld=E + PAD, name="y"), g.embed(torch.zeros(rows, E), ld=E + PAD, name="ypos")
        dp = g.embed(pos, ld=E + PAD, name="pos") if with_pos else None
        ops._L.check(lib.ff_layernorm(g.embed(x, ld=E + PAD, name="x").data_ptr(), E + PAD, g.embed(gam).data_ptr(), g.embed(bet).data_ptr(),
                                      1e-5, y.data_ptr(), E + PAD, yp.data_ptr() if with_pos else None, E + PAD,
                                      dp.data_ptr() if with_pos else None, E + PAD if with_pos else 0, div, mod, rows, E, _stream()),
                     "ff_layernorm")
        return {"y": y, "ypos": yp}
    got = twice(run, "ff_layernorm")
    ref = F.layer_norm(x.double(), (E,), gam.double(), bet.double(), 1e-5)
    assert rel_err(got["y"], ref) < 2e-6
    if with_pos:
        assert rel_err(got["ypos"], ref + pos.double()[(torch.arange(rows) // div) % mod]) < 2e-6
    else:
        assert not bool(got["ypos"].any())                    # a null ypos: nothing written


def test_add_pos_gelu_and_gather_rows(ops):
    lib = ops._L.load()
    rows, E, div, mod = 37, 512, 5, 7
    x, pos = rnd(rows, E, seed=1), rnd(mod, E, seed=2)

    def add_pos(g):
        out = g.embed(torch.zeros(rows, E), ld=E + PAD, name="out")
        ops._L.check(lib.ff_add_pos(g.embed(x, ld=E + PAD, name="x").data_ptr(), E + PAD, g.embed(pos, ld=E + PAD, name="pos").data_ptr(),
                                    E + PAD, div, mod, out.data_ptr(), E + PAD, rows, E, _stream()), "ff_add_pos")
        return {"out": out}
    assert torch.equal(twice(add_pos, "ff_add_pos")["out"].cpu(), x + pos[(torch.arange(rows) // div) % mod])
    for r, e in ((1, 256), (37, 1024), (3, 4)):
        v = rnd(r, e, seed=3, scale=2.5)
        got = twice(lambda g: {"x": ops.gelu_(g.embed(v, ld=e + PAD, name="x"))}, "ff_gelu")
        want = F.gelu(v.double())
        assert float((got["x"].cpu().double() - want).abs().max()) < 4e-7 * max(1.0, float(want.abs().max()))
    N, S, spg = 3, 20, 2
    mem = rnd(N, S, E, seed=4)
    tok = torch.tensor([0, S - 1, 5, S - 1, 0, 1], dtype=torch.int32)         # first and last key of a wireframe

    def gather(g):
        out = g.embed(torch.zeros(tok.numel(), E), ld=E + PAD, name="out")
        ops._L.check(lib.ff_gather_rows(g.embed(mem, name="memory").data_ptr(), S, E, g.embed(tok, name="tok").data_ptr(), tok.numel(), spg,
                                        out.data_ptr(), E + PAD, _stream()), "ff_gather_rows")
        return {"out": out}
    assert torch.equal(twice(gather, "ff_gather_rows")["out"].cpu(), torch.stack([mem[i // spg, int(t)] for i, t in enumerate(tok)]))


@pytest.mark.parametrize("width", [512, 6])
@pytest.mark.parametrize("form", ["src_idx", "dst_idx"])
def test_permute_rows(ops, width, form):
    """Both index forms of ff_permute_rows; width 512 takes the 16-byte loads, width 6 the scalar path."""
    lib = ops._L.load()
    npos, src_rows, dst_rows, rows = 3, 11, 9, 7
    src = rnd(npos, src_rows, width, seed=1)
    idx = torch.tensor([10, 0, 3, 8, 1, 6, 4] if form == "src_idx" else [8, 0, 3, 7, 1, 6, 4], dtype=torch.int32)   # (distinct)

    def run(g):
        dst = g.embed(torch.full((npos, dst_rows, width), 7.0), name="dst")
        di = g.embed(idx, name="idx")
        ops._L.check(lib.ff_permute_rows(g.embed(src, name="src").data_ptr(), src_rows, di.data_ptr() if form == "src_idx" else None,
                                         dst.data_ptr(), dst_rows, di.data_ptr() if form == "dst_idx" else None, npos, rows, width, _stream()),
                     "ff_permute_rows")
        return {"dst": dst}
    got = twice(run, "ff_permute_rows")["dst"].cpu()
    want = torch.full((npos, dst_rows, width), 7.0)
    if form == "src_idx":
        want[:, :rows] = src[:, idx.long()]
    else:
        want[:, idx.long()] = src[:, :rows]
    assert torch.equal(got, want)


def test_assemble_embedding_and_prepare_mask(ops):
    lib = ops._L.load()
    N, L, E, nt, ld_edge = 3, 5, 64, 4, 64 + PAD
    tok_embed, edge = rnd(nt, E, seed=1), rnd(N * L, E, seed=2)

    def assemble(g):
        out = g.embed(torch.zeros(N, L + nt, E), name="out")
        ops._L.check(lib.ff_assemble_embedding(g.embed(tok_embed, name="tok_embed").data_ptr(), nt, g.embed(edge, ld=ld_edge, name="edge").data_ptr(),
                                               ld_edge, N, L, E, out.data_ptr(), _stream()), "ff_assemble_embedding")
        return {"out": out}
    want = torch.cat([tok_embed[None].expand(N, nt, E), edge.view(N, L, E)], dim=1)
    assert torch.equal(twice(assemble, "ff_assemble_embedding")["out"].cpu(), want)
    from faceformer_amd.hip.engine import _kv_len_from_mask
    for n in (1, 5):
        for l in (0, 3, 70):
            m = torch.rand(n, l, generator=torch.Generator().manual_seed(n + l)) < 0.4
            if l:
                m[0] = True

            def prepare(g):
                mask_out, kv = g.embed(torch.zeros(n, l + nt, dtype=torch.uint8), name="mask_out"), g.embed(torch.zeros(n, dtype=torch.int32), name="kv_len")
                src = g.embed(m.to(torch.uint8), name="input_mask") if l else g.bytes(1, name="input_mask")     # (L = 0: no byte is read)
                ops._L.check(lib.ff_prepare_mask(src.data_ptr(), n, l, nt, mask_out.data_ptr(), kv.data_ptr(), _stream()), "ff_prepare_mask")
                return {"mask": mask_out, "kv_len": kv}
            got = twice(prepare, "ff_prepare_mask")
            wm = torch.cat([torch.zeros(n, nt, dtype=torch.bool), m], dim=1).to(torch.uint8)
            assert torch.equal(got["mask"].cpu(), wm) and torch.equal(got["kv_len"].cpu(), _kv_len_from_mask(wm))
