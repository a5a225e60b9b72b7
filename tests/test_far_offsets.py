"""GPU: every kernel family and the engine with operand offsets past 2^31 bytes, 2^32 bytes and 2^31 elements (DESIGN.md 19;
helper: tests/farview.py).

The operator tests hand a kernel a SMALL logical operand whose row stride is so large that its last row lies just past the reach
(B31: 2^31 bytes, B32: 2^32 bytes, E31: 2^33 bytes = 2^31 elements), one far operand per call, every other operand compact inside
a red zone (tests/redzone.py).  Every case runs under a ZERO and a POISON fill and asserts
  (a) the result against an fp64 reference computed from the small logical tensors, at the bar tests/test_hip_ops.py already uses
      for that kernel (3e-6 GEMM, 5e-6 attention, 2e-6 LayerNorm, 4e-7 gelu, exact copies; the pointer ops by their own rules),
  (b) that the two fills give the same bits,
  (c) that every byte of a far operand's parent outside its logical elements still holds the fill (farview.check_untouched),
  (d) that the call allocated at most its far operand plus 1 GiB.
Where an entry point refuses a far operand, the test asserts the refusal (FF_ERR_ARG = status -1), its message and that nothing
was written.  The engine test decodes one whole batch whose q|k|v buffer passes 2^32 bytes (and 2^33) as ONE micro-batch and
compares 16-wireframe slices with the same engine run on those slices alone."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import farview as FV
import redzone as RZ
from test_hip_ops import _ref_attention_general, _seg_stats, ref_attention, rel_err, rnd

pytestmark = pytest.mark.gpu
PAD = 8
GIB = 1 << 30
REACH_IDS = list(FV.REACHES)
FILLS = (RZ.ZERO, RZ.POISON)
REFUSED = r"status -1: "


@pytest.fixture(scope="module")
def ops(hip_lib):
    from faceformer_amd.hip import ops as _ops
    return _ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _free():
    torch.cuda.empty_cache()


class Case:
    """One run under one fill: far operands (farview) and compact ones (a red-zone guard of the same fill)."""

    def __init__(self, fill):
        self.fill, self.g, self.fars, self.big = fill, RZ.Guard(fill), [], 0

    def far(self, t, reach, ld=None):
        v = FV.far(t, reach, self.fill, ld=ld)
        self.fars.append(v)
        self.big += v._far.parent.numel()
        return v

    def c(self, t, name=None):
        """Compact: ld = columns + 8 for a 2-D operand."""
        return self.g.embed(t, ld=t.shape[1] + PAD if t.dim() == 2 else None, name=name)

    def opt(self, t, name=None):
        return None if t is None else self.c(t, name)

    def tight(self, t, name=None):
        return self.g.embed(t, name=name)

    def check(self, what):
        self.g.check()
        for v in self.fars:
            FV.check_untouched(v, what)


def both(run, what):
    """run(case) -> {name: tensor} under both fills: (b), (c), (d); returns the POISON run's outputs on the CPU."""
    outs = []
    for fill in FILLS:
        _free()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        c = Case(fill)
        res = run(c)
        c.check("%s (fill 0x%02x)" % (what, fill))
        outs.append({k: v.detach().cpu().clone() for k, v in res.items() if torch.is_tensor(v)})
        peak = torch.cuda.max_memory_allocated() - base
        assert peak - c.big <= GIB, "%s: peak allocation %d bytes, far operands %d" % (what, peak, c.big)
        del c, res
        _free()
    assert outs[0] and outs[0].keys() == outs[1].keys(), what
    for k in outs[0]:
        RZ.assert_same_bits(outs[0][k], outs[1][k], "%s: %s" % (what, k))
    return outs[1]


def refused(call, message, out=None, init=None):
    """The call returns FF_ERR_ARG with `message` in ff_last_error(); `out` (if given) still holds `init`."""
    from faceformer_amd.hip.lib import HipExtensionError
    with pytest.raises(HipExtensionError, match=REFUSED + ".*" + message):
        call()
    torch.cuda.synchronize()
    if out is not None:
        assert torch.equal(out.cpu(), init), "a refused call wrote its output"


@contextlib.contextmanager
def knobs(ops, **kw):
    old = {k: ops.set_tuning(k, v) for k, v in kw.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            ops.set_tuning(k, v)


# ---- f32 GEMM family --------------------------------------------------------------------------------------------------------------
GN, GK, NS = 260, 128, 128          # N is no multiple of a tile, K takes the stream-K launcher and the small-rows kernel
TILE_GROUPS = [(70, (0, 1, 2, 3, 6, 7, 12)), (130, (4, 5, 9, 10, 11)), (5, (8,))]   # 64-row tiles / 128-row tiles (11: 64 x 128,
#                                                                                      run at 130 rows too) / the small-rows kernel
GEMM_FAR = [(w, r) for w in ("A", "residual", "C", "W") for r in REACH_IDS if (w, r) != ("W", "E31")]   # (a far weight: B31 and B32)
LIMIT = 1 << 30                     # elements: M * lda and N * ldw of the LDS-DMA and split kernels (32-bit byte offsets)


def _gemm_data(M, N=GN, K=GK):
    a, a2 = rnd(M, K, seed=1), rnd(M, K, seed=5)
    w, bias, res = rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3), rnd(M, N, seed=4)
    return a, a2, w, bias, res


def _gemm_ref(which, a, a2, w, bias, res, ns=NS):
    prod = a.double() @ w.double().t()
    if which == "A":
        return torch.cat([prod[:, :ns], a2.double() @ w.double()[ns:].t()], dim=1) + bias.double()
    if which == "W":
        return prod + bias.double()
    return torch.relu(prod + bias.double()) + res.double()


def _gemm_place(c, which, reach, a, a2, w, bias, res, ld=None):
    """(A, A2, n_split, W, residual, out, act): the operand under test far, the others compact.  "A": A | A2 side by side in ONE
    far parent (the entry has one lda for both), columns from n_split on read A2.  "C": the residual aliased to the far output."""
    K = a.shape[1]
    A, A2, ns, Wt, R, act = None, None, 0, None, None, 1
    if which == "A":
        big = c.far(torch.cat([a, a2], dim=1), reach, ld=ld)
        A, A2, ns, act = big[:, :K], big[:, K:], NS, 0
    else:
        A = c.c(a, "A")
    Wt = c.far(w, reach, ld=ld) if which == "W" else c.c(w, "W")
    if which == "W":
        act = 0
    if which == "residual":
        R = c.far(res, reach)
    if which == "C":
        out = R = c.far(res, reach)
    else:
        out = c.c(torch.zeros_like(res), "C")
    return A, A2, ns, Wt, R, out, act


@pytest.mark.parametrize("M,tiles", TILE_GROUPS, ids=["m70", "m130", "m5"])
@pytest.mark.parametrize("which,reach", GEMM_FAR)
def test_gemm_f32(ops, which, reach, M, tiles):
    """ff_gemm_f32, every tile: far A and A2 (one parent, split A), far residual, far C (residual aliased), far W.  The LDS-DMA
    tiles 11 / 12 refuse M * lda >= 2^30 and N * ldw >= 2^30 (their 32-bit byte offsets): asserted as a refusal."""
    data = _gemm_data(M)
    a, a2, w, bias, res = data
    ref = _gemm_ref(which, *data)
    init = torch.zeros_like(res)

    def run(c):
        A, A2, ns, Wt, R, out, act = _gemm_place(c, which, FV.REACHES[reach], *data)
        b = c.tight(bias, "bias")
        got = {}
        for tile in tiles:
            what = "ff_gemm_f32 tile %d far %s %s" % (tile, which, reach)
            if which == "C":
                out.copy_(res)
            else:
                out.zero_()
            call = lambda: ops.linear(A, Wt, b, act=act, residual=R, x2=A2, n_split=ns, tile=tile, out=out)
            if tile in (11, 12) and (M * A.stride(0) >= LIMIT or GN * Wt.stride(0) >= LIMIT):
                refused(call, "tile 1[12] needs", out, res if which == "C" else init)
                continue
            call()
            if which == "C":
                FV.check_untouched(out, what)
            got["tile%d" % tile] = out.clone()
        return got
    got = both(run, "ff_gemm_f32 far %s %s M=%d" % (which, reach, M))
    assert set(got) >= {"tile%d" % t for t in tiles if t not in (11, 12)}
    for k, v in got.items():
        assert rel_err(v, ref) < 3e-6, (k, which, reach)


@pytest.mark.parametrize("which", ["A", "W", "C"])
def test_gemm_f32_batched_second_problem_past_2_32(ops, which):
    """ff_gemm_f32_batched, batch = 2: the batch stride of one operand puts the second problem alone past 2^32 bytes."""
    lib = ops._L.load()
    M, N, K = 70, GN, GK
    a, w = rnd(2, M * K, seed=1), rnd(2, N * K, seed=2, scale=0.1)
    bias = rnd(N, seed=3)
    ref = torch.stack([a[z].view(M, K).double() @ w[z].view(N, K).double().t() + bias.double() for z in range(2)])

    def run(c):
        A = c.far(a, FV.B32) if which == "A" else c.tight(a, "A")
        Wt = c.far(w, FV.B32) if which == "W" else c.tight(w, "W")
        out = c.far(torch.zeros(2, M * N), FV.B32) if which == "C" else c.tight(torch.zeros(2, M * N), "C")
        assert (A if which == "A" else Wt if which == "W" else out).stride(0) * 4 > FV.B32
        got = {}
        for tile in (0, 1, 3, 6, 8):
            out.zero_()
            ops._L.check(lib.ff_gemm_f32_batched(A.data_ptr(), K, None, 0, Wt.data_ptr(), K, c.tight(bias).data_ptr(), None, 0,
                                                 out.data_ptr(), N, M, N, K, 0, tile, 2, A.stride(0), Wt.stride(0), out.stride(0),
                                                 _stream()), "ff_gemm_f32_batched")
            if which == "C":
                FV.check_untouched(out, "batched tile %d" % tile)
            got["tile%d" % tile] = out.clone()
        return got
    for k, v in both(run, "ff_gemm_f32_batched far %s" % which).items():
        assert rel_err(v.view(2, M, N), ref) < 3e-6, (k, which)


DMA_KNOBS = dict(FF_DMA_MIN_ROWS=1, FF_DMA_MIN_ROWS_N512=1, FF_DMA_MIN_ROWS_WIDE=1)   # the automatic choice hands every launch to the LDS-DMA kernel


@pytest.mark.parametrize("which", ["A", "W"])
def test_gemm_f32_lds_dma_at_the_2_30_element_limit(ops, which):
    """M * lda (N * ldw) one row below 2^30: the LDS-DMA tiles compute the right result with byte offsets in [2^31, 2^32).  One
    more row reaches 2^30: tiles 11 / 12 refuse, and the automatic choice -- told to prefer the LDS-DMA kernel from one row on --
    routes to the other f32 kernels and is still right."""
    if which == "A":
        rows, ld, under, over = 128, 1 << 23, 127, 128                    # 127 * 2^23 = 2^30 - lda
        M, N = None, GN
    else:
        rows, ld, under, over = 256, 4244040, 252, 256                    # 252 * ld < 2^30 <= 253 * ld (N % 4 == 0)
        M, N = 70, None
    assert under * ld < LIMIT <= (under + 1) * ld and over * ld >= LIMIT and under * ld >= LIMIT - ld
    data = _gemm_data(rows if which == "A" else M, N=GN if which == "A" else rows)
    a, a2, w, bias, res = data
    ref = _gemm_ref(which, *data)

    def run(c):
        A, A2, ns, Wt, R, out, act = _gemm_place(c, which, 0, *data, ld=ld)
        b = c.tight(bias, "bias")
        got = {}
        for n in (under, over):
            Ax, A2x, Wx, bx = (A[:n], A2[:n], Wt, b) if which == "A" else (A, A2, Wt[:n], b[:n])
            o = out[:n] if which == "A" else out[:, :n]
            for tile in (11, 12, 0):
                out.zero_()
                call = lambda: ops.linear(Ax, Wx, bx, act=act, x2=A2x, n_split=ns, tile=tile, out=o)
                if tile and n == over:
                    refused(call, "tile 1[12] needs", out, torch.zeros_like(res))
                    continue
                with knobs(ops, **DMA_KNOBS):
                    call()
                got["%d rows tile %d" % (n, tile)] = o.clone()
        return got
    got = both(run, "LDS-DMA limit far %s" % which)
    assert len(got) == 4
    for k, v in got.items():
        n = int(k.split()[0])
        assert rel_err(v, ref[:n] if which == "A" else ref[:, :n]) < 3e-6, (k, which)


# ---- split products ---------------------------------------------------------------------------------------------------------------
KINDS = ["bf16x3", "fp16x2", "fp16"]


def _h(x):
    return x.half().double()


def _split_bar_ok(kind, got, a, a2, w, bias, res, which, ns=NS):
    """The split kinds' bars of tests/test_redzone_ops.py: 3e-6 against fp64, or (one fp16 product) fp32 accumulation of K exact
    products of the fp16-rounded operands."""
    if kind != "fp16":
        return rel_err(got, _gemm_ref(which, a, a2, w, bias, res, ns)) < 3e-6
    K = a.shape[1]
    prod, den = _h(a) @ _h(w).t(), _h(a).abs() @ _h(w).abs().t()
    if which == "A":
        ref = torch.cat([prod[:, :ns], _h(a2) @ _h(w)[ns:].t()], dim=1) + bias.double()
        den = torch.cat([den[:, :ns], _h(a2).abs() @ _h(w).abs()[ns:].t()], dim=1)
    else:
        ref = torch.relu(prod + bias.double()) + res.double()
    err = (got.double() - ref).abs()
    return bool((err <= K * 2.0 ** -24 * den + 2.0 ** -22 * ref.abs() + 2.0 ** -40).all())


@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["residual", "C"])
@pytest.mark.parametrize("kind", KINDS)
def test_gemm_split_far_output_and_residual(ops, kind, which, reach):
    """ff_gemm_x3 / ff_gemm_x2h / ff_gemm_h1 under both launch shapes of ff_set_x3_tuning: far C (residual aliased), far residual."""
    M = 70
    data = _gemm_data(M)
    a, a2, w, bias, res = data

    def run(c):
        A, A2, ns, Wt, R, out, act = _gemm_place(c, which, FV.REACHES[reach], *data)
        planes = ops.split_weight(Wt, kind)
        b = c.tight(bias, "bias")
        got = {}
        for shape in (1, 2):
            out.copy_(res) if which == "C" else out.zero_()
            ops.set_x3_tuning(shape)
            try:
                ops.linear_x3(A, planes, b, act=act, residual=R, out=out)
            finally:
                ops.set_x3_tuning(0)
            if which == "C":
                FV.check_untouched(out, "linear_x3 %s shape %d" % (kind, shape))
            got["shape%d" % shape] = out.clone()
        return got
    for k, v in both(run, "linear_x3 %s far %s %s" % (kind, which, reach)).items():
        assert _split_bar_ok(kind, v, *data, which), (k, kind, which, reach)


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_split_a_at_the_2_30_element_limit(ops, kind):
    """A | A2 with M * lda = 2^30 - lda: the split kernels' unsigned byte offsets lie in [2^31, 2^32) and the result is right, plain
    and LayerNorm-emitting form, both launch shapes.  One more row (M * lda = 2^30): FF_ERR_ARG naming A, C untouched."""
    rows, ld, under, over = 128, 1 << 23, 127, 128
    data = _gemm_data(rows)
    a, a2, w, bias, res = data
    w64 = w[:64].contiguous()

    def run(c):
        A, A2, ns, Wt, R, out, act = _gemm_place(c, "A", 0, *data, ld=ld)
        planes, planes64 = ops.split_weight(Wt, kind), ops.split_weight(c.c(w64, "W64"), kind)
        b, R64 = c.tight(bias, "bias"), c.c(res[:, :64].contiguous(), "residual")
        out64 = c.c(torch.zeros(rows, 64), "C64")
        got = {}
        for shape in (1, 2):
            ops.set_x3_tuning(shape)
            try:
                out.zero_(), out64.zero_()
                ops.linear_x3(A[:under], planes, b, x2=A2[:under], n_split=ns, out=out[:under])
                _, st = ops.linear_x3_ln(A[:under], planes64, b[:64], residual=R64[:under], want_stats=True, out=out64[:under])
                got["plain shape%d" % shape], got["ln shape%d" % shape], got["stats shape%d" % shape] = out.clone(), out64.clone(), st
                out.zero_(), out64.zero_()
                zero = torch.zeros_like(res)
                refused(lambda: ops.linear_x3(A[:over], planes, b, x2=A2[:over], n_split=ns, out=out), "A is too large", out, zero)
                refused(lambda: ops.linear_x3_ln(A[:over], planes64, b[:64], residual=R64, want_stats=True, out=out64), "A is too large",
                        out64, zero[:, :64])
            finally:
                ops.set_x3_tuning(0)
        return got
    got = both(run, "split products %s at the limit" % kind)
    r = _h if kind == "fp16" else (lambda x: x.double())
    ln_ref = r(a) @ r(w64).t() + bias[:64].double() + res[:, :64].double()
    for shape in (1, 2):
        plain, ln = got["plain shape%d" % shape], got["ln shape%d" % shape]
        assert not bool(plain[under:].any()) and not bool(ln[under:].any())
        assert _split_bar_ok(kind, plain[:under], a[:under], a2[:under], w, bias, res[:under], "A"), (kind, shape)
        bar = 2e-5 if kind != "fp16" else 2e-5 + GK * 2.0 ** -24 * float((_h(a).abs() @ _h(w64).abs().t()).max() / ln_ref.abs().max())
        assert (ln[:under].double() - ln_ref[:under]).abs().max() < bar * ln_ref.abs().max(), (kind, shape)
        want, st = _seg_stats(ln[:under].double()), got["stats shape%d" % shape].double()
        assert (st[..., 0] - want[..., 0]).abs().max() < 1e-5
        assert ((st[..., 1] - want[..., 1]).abs() / want[..., 1].clamp_min(1e-6)).max() < 1e-5


# ---- LayerNorm-fused forms --------------------------------------------------------------------------------------------------------
LN_FAMILIES = [("f32", None), ("split", "bf16x3"), ("split", "fp16x2"), ("split", "fp16")]     # ("fp16": ff_gemm_h1_ln)
LN_TILES = (0, 3, 6, 8, 11, 12)


def _ln_forms(ops, family, kind):
    """[(name, emit(A, W, **kw), consume(x, Wf, colsum, **kw))]: ff_gemm_f32_ln once per tile that carries the fusion, or the
    split products' ff_gemm_x3_ln / ff_gemm_x2h_ln / ff_gemm_h1_ln under both launch shapes."""
    forms = []
    if family == "f32":
        for tile in LN_TILES:
            forms.append(("tile%d" % tile, (lambda A, W, tile=tile, **kw: ops.linear_ln(A, W, tile=tile, **kw)),
                          (lambda x, Wf, cs, tile=tile, **kw: ops.linear_ln(x, Wf, tile=tile, **kw))))
        return forms
    for shape in (1, 2):
        def emit(A, W, shape=shape, **kw):
            ops.set_x3_tuning(shape)
            try:
                return ops.linear_x3_ln(A, ops.split_weight(W, kind), **kw)
            finally:
                ops.set_x3_tuning(0)

        def consume(x, Wf, cs, shape=shape, **kw):
            ops.set_x3_tuning(shape)
            try:
                return ops.linear_x3_ln(x, ops.split_weight(Wf, kind), colsum=cs, **kw)
            finally:
                ops.set_x3_tuning(0)
        forms.append(("shape%d" % shape, emit, consume))
    return forms


@pytest.mark.parametrize("family,kind,which,reach", [(f, k, w, r) for f, k in LN_FAMILIES for w, r in GEMM_FAR if f == "f32" or w in ("residual", "C")])
def test_gemm_ln_emits_segment_statistics(ops, family, kind, which, reach):
    """Producer form (C = A W^T + b + residual and the segment statistics of the stored C) with a far A / W (f32 family), residual
    or C: the bars of test_gemm_emits_layernorm_segment_statistics; ff_gemm_h1_ln (one fp16 product) at test_fp16_mode's bar, fp32
    accumulation of K exact products of the fp16-rounded operands.  (The split products' far A: test_gemm_split_a_at_the_2_30_
    element_limit; their weight is planes and has no ldw.)"""
    M, N, K = 70, 64, 128
    gen = torch.Generator().manual_seed(M + N + K)
    A, W, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen)
    res = 3.0 + 2.0 * torch.randn(M, N, generator=gen)
    R = FV.REACHES[reach]
    ref = A.double() @ W.double().t() + b.double() + res.double()

    def run(c):
        dA = c.far(A, R) if which == "A" else c.c(A, "A")
        dW = c.far(W, R) if which == "W" else c.c(W, "W")
        dR = c.far(res, R) if which == "residual" else c.c(res, "residual")
        out = c.far(torch.zeros(M, N), R) if which == "C" else c.c(torch.zeros(M, N), "C")
        db = c.tight(b, "bias")
        got = {}
        for name, emit, _ in _ln_forms(ops, family, kind):
            out.zero_()
            call = lambda: emit(dA, dW, bias=db, residual=dR, want_stats=True, out=out)
            if name in ("tile11", "tile12") and (M * dA.stride(0) >= LIMIT or N * dW.stride(0) >= LIMIT):
                refused(call, "tile 1[12] needs", out, torch.zeros(M, N))
                continue
            _, stats = call()
            if which == "C":
                FV.check_untouched(out, "ln emit %s" % name)
            got[name], got[name + " stats"] = out.clone(), stats
        return got
    got = both(run, "ln emit %s %s far %s %s" % (family, kind, which, reach))
    for name in [k for k in got if not k.endswith(" stats")]:
        out, stats = got[name].double(), got[name + " stats"].double()
        if kind == "fp16":
            ref_r = _h(A) @ _h(W).t() + b.double() + res.double()
            bar = K * 2.0 ** -24 * (_h(A).abs() @ _h(W).abs().t()) + 2.0 ** -22 * ref_r.abs() + 2.0 ** -40
            assert bool(((out - ref_r).abs() <= bar).all()), (name, float(((out - ref_r).abs() / bar).max()))
        else:
            assert (out - ref).abs().max() < 2e-5 * ref.abs().max(), name
        want = _seg_stats(out)
        assert not torch.isnan(stats).any()
        assert (stats[..., 0] - want[..., 0]).abs().max() < 1e-5, name
        assert ((stats[..., 1] - want[..., 1]).abs() / want[..., 1].clamp_min(1e-6)).max() < 1e-5, name


@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("family,kind,in_epilogue,which", [(f, k, e, w) for f, k, e in (
    ("f32", None, False), ("split", "bf16x3", False), ("split", "bf16x3", True), ("split", "fp16x2", False), ("split", "fp16x2", True),
    ("split", "fp16", False), ("split", "fp16", True))
    for w in ("x", "row_table", "C") if f == "f32" or w != "x"])
def test_gemm_ln_consumes_segment_statistics(ops, family, kind, in_epilogue, which, reach):
    """Consumer form (act((LN(x) + pos[row // div]) W^T + b) from raw x, its statistics and the folded weight) with a far x (f32
    family), a far row_table (ld_row_table) or a far C: the bar of test_gemm_consumes_layernorm_statistics_with_folded_weights;
    ff_gemm_h1_ln at the bars of test_gemm_h1_layernorm_forms_are_one_fp16_product (_h1_consume_bar)."""
    M, N, K, div = 70, 64, 512, 9
    gen = torch.Generator().manual_seed(M * 3 + N + K)
    x = (1.5 + 2.0 * torch.randn(M, K, generator=gen)) * (1.0 + torch.rand(M, 1, generator=gen))
    W, b = torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen)
    gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=gen), 0.3 * torch.randn(K, generator=gen)
    pos = torch.randn((M + div - 1) // div, K, generator=gen)
    Wf, bf, P = (t.cpu() for t in ops.fold_layernorm_linear(W.cuda(), b.cuda(), gamma.cuda(), beta.cuda(), pos.cuda(), N))
    stats = _seg_stats(x.double()).float().contiguous()
    colsum = Wf.double().sum(dim=1).float().contiguous()
    R = FV.REACHES[reach]
    ln = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5)
    ref = torch.relu(ln @ W.double().t() + b.double() + pos.double()[torch.arange(M) // div] @ W.double().t())

    def run(c):
        dx = c.far(x, R) if which == "x" else c.c(x, "x")
        dP = c.far(P, R) if which == "row_table" else c.c(P, "row_table")
        out = c.far(torch.zeros(M, N), R) if which == "C" else c.c(torch.zeros(M, N), "C")
        dW, db, ds = c.c(Wf, "Wf"), c.tight(bf, "bf"), c.tight(stats, "stats_in")
        cs = c.tight(colsum, "colsum") if in_epilogue else None
        got = {}
        for name, _, consume in _ln_forms(ops, family, kind):
            out.zero_()
            call = lambda: consume(dx, dW, cs, bias=db, act=1, stats_in=ds, row_table=dP, row_div=div, row_cols=N, out=out)
            if name in ("tile11", "tile12") and M * dx.stride(0) >= LIMIT:
                refused(call, "tile 1[12] needs", out, torch.zeros(M, N))
                continue
            call()
            if which == "C":
                FV.check_untouched(out, "ln consume %s" % name)
            got[name] = out.clone()
        return got
    for name, v in both(run, "ln consume %s %s epilogue=%s far %s %s" % (family, kind, in_epilogue, which, reach)).items():
        if kind == "fp16":
            ref_r, bar = _h1_consume_bar(x, Wf, bf, P[torch.arange(M) // div], colsum if in_epilogue else None)
            assert bool(((v.double() - ref_r).abs() <= bar).all()), (name, float(((v.double() - ref_r).abs() / bar).max()))
        else:
            assert (v.double() - ref).abs().max() < 3e-5 * max(1.0, float(ref.abs().max())), name


def _h1_consume_bar(x, Wf, bf, table, colsum, eps=1e-5):
    """(reference, bar) of the one-fp16-product consumer, as test_gemm_h1_layernorm_forms_are_one_fp16_product takes them: the fp64
    product of exactly the operands the form rounds -- the normalised rows (colsum None; a value within a few fp32 ulps of an fp16
    rounding boundary may round to the neighbour), or the raw rows at 2^-6 with the LayerNorm in the epilogue -- plus the fp32
    table row, under fp32 accumulation of K products."""
    K = x.shape[1]
    mean = x.double().mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(dim=1, unbiased=False, keepdim=True) + eps)
    add = bf.double() + table.double()
    if colsum is None:
        n = ((x.double() - mean) * rstd).float()
        ref_r = torch.relu(_h(n) @ _h(Wf).t() + add)
        d = 2.0 ** -20
        flip = (_h(n.double() * (1 + d)) - _h(n.double() * (1 - d))).abs()
        den = _h(n).abs() @ _h(Wf).abs().t() + (flip @ _h(Wf).abs().t()) * 2.0 ** 24 / K
    else:
        xs = _h(x / 64.0) * 64.0
        ref_r = torch.relu((xs @ _h(Wf).t() - mean * colsum.double()) * rstd + add)
        den = (xs.abs() @ _h(Wf).abs().t() + mean.abs() * colsum.double().abs()) * rstd
    return ref_r, K * 2.0 ** -24 * den + 1e-6 * (1.0 + ref_r.abs())


@pytest.mark.parametrize("reach", ["B31", "B32"])
def test_fold_layernorm_linear_far_ldpos(ops, reach):
    N, K, rows, pos_cols = 100, 96, 7, 64
    W, b = rnd(N, K, seed=1, scale=0.1), rnd(N, seed=2)
    gamma, beta, pos = rnd(K, seed=3) + 1.0, rnd(K, seed=4), rnd(rows, K, seed=5)

    def run(c):
        Wf, bf, P = ops.fold_layernorm_linear(c.c(W, "W"), c.tight(b), c.tight(gamma), c.tight(beta), c.far(pos, FV.REACHES[reach]), pos_cols)
        return {"P": P, "bf": bf}
    got = both(run, "fold far ldpos %s" % reach)
    assert rel_err(got["P"], pos.double() @ W.double()[:pos_cols].t()) < 3e-6 and rel_err(got["bf"], b.double() + W.double() @ beta.double()) < 3e-6


@pytest.mark.parametrize("reach", ["B31", "B32"])
def test_fold_layernorm_linear_and_split_weight_far_ldw(ops, reach):
    """ff_fold_layernorm_linear and the three ff_split_weight_* entries with a far weight (ldw)."""
    N, K, rows, pos_cols = 100, 96, 7, 64
    W, b = rnd(N, K, seed=1, scale=0.1), rnd(N, seed=2)
    gamma, beta, pos = rnd(K, seed=3) + 1.0, rnd(K, seed=4), rnd(rows, K, seed=5)

    def run(c):
        dW = c.far(W, FV.REACHES[reach])
        Wf, bf, P = ops.fold_layernorm_linear(dW, c.tight(b), c.tight(gamma), c.tight(beta), c.c(pos, "pos"), pos_cols)
        got = {"Wf": Wf, "bf": bf, "P": P}
        for kind in KINDS:
            got[kind] = ops.planes_to_matrix(ops.split_weight(dW, kind)).float()
        return got
    got = both(run, "fold / split far ldw %s" % reach)
    assert rel_err(got["Wf"], W.double() * gamma.double()) < 3e-6
    assert rel_err(got["bf"], b.double() + W.double() @ beta.double()) < 3e-6
    assert rel_err(got["P"], pos.double() @ W.double()[:pos_cols].t()) < 3e-6
    assert rel_err(got["bf16x3"], W) < 2.0 ** -24 and rel_err(got["fp16x2"], W) < 2.0 ** -21
    assert torch.equal(got["fp16"], W.half().float())


# ---- attention with 64-wide heads -------------------------------------------------------------------------------------------------
ALGOS = [(1, 0), (2, 0), (3, 0), (4, 2), (4, 1)]        # (ff_set_attention_algo, kv_terms): LDS-shared, wave, resident, 2 x fp16, one fp16 term


@contextlib.contextmanager
def attention_algo(ops, algo):
    old = ops.set_attention_algo(algo)
    try:
        yield
    finally:
        ops.set_attention_algo(old)


@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["q", "k", "v", "o"])
def test_attention_group_major_far_ld(ops, which, reach):
    """Layout (a): ldq, ldk, ldv, ldo inflated in turn, every kernel, with kv_len and a key mask.  Under algo 4 ops.attention makes
    the fp16 planes itself: ff_attention_split_kv reads the far k / v too."""
    from test_fp16_mode import _h1_check
    from test_redzone_ops import _masks
    G, H, nq, nk = 2, 2, 33, 37
    E = H * 64
    t = {"q": rnd(G * nq, E, seed=1), "k": rnd(G * nk, E, seed=2), "v": rnd(G * nk, E, seed=3), "o": torch.zeros(G * nq, E)}
    mask, kv_len = _masks(G, nk)

    def run(c):
        d = {n: (c.far(x, FV.REACHES[reach]) if n == which else c.c(x, n)) for n, x in t.items()}
        dm, dl = c.tight(mask.to(torch.uint8), "key_mask"), c.tight(kv_len, "kv_len")
        got = {}
        for algo, terms in ALGOS:
            d["o"].zero_()
            with attention_algo(ops, algo):
                ops.attention(d["q"], d["k"], d["v"], G, H, nq, nk, q_group_stride=nq, q_inner=nq, q_outer_stride=0, k_group_stride=nk,
                              k_stride=1, kv_len=dl, key_mask=dm, out=d["o"], kv_terms=terms)
            if which == "o":
                FV.check_untouched(d["o"], "attention algo %d" % algo)
            got["algo%d terms%d" % (algo, terms)] = d["o"].clone()
        return got
    got = both(run, "attention group-major far %s %s" % (which, reach))
    qd, kd, vd = (t[n].double().view(G, -1, H, 64).transpose(1, 2) for n in "qkv")
    ref = ref_attention(qd, kd, vd, mask).transpose(1, 2).reshape(G * nq, E)
    for k, v in got.items():
        if k.endswith("terms1"):
            _h1_check(v, t["q"], t["k"], t["v"], G, H, nq, nk, mask)
        else:
            assert rel_err(v, ref) < 5e-6, (k, which, reach)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("reach", REACH_IDS)
def test_attention_position_major_far_strides(ops, reach, causal):
    """Layout (b), the engine's: rows j * Bc + b of ONE packed q | k | v | o buffer, q_outer_stride = k_stride = Bc so large that the
    last position of the last group lies past the reach, four sequences spread over [0, Bc); t = 7, H = 2 (decoder_pass's
    self-attention on a few sequences of a very large micro-batch).  Bc is what puts the last row JUST past the reach with
    2 KiB packed rows, 155 346 ... 621 380 -- not the tens of millions a first sketch of this test named: at t = 7 those would
    lie 30 to 100 GB out, far past every reach, and need one allocation of that size.  Full: every kernel, the 2 x fp16 one with
    both term counts.  Causal: the block-shared and the wave kernel only -- the resident and fp16 kernels take no causal mask, and
    ff_attention hands such a launch to the block-shared kernel whatever the algo says."""
    from test_fp16_mode import _h1_check
    t, G, H = 7, 4, 2
    E = H * 64
    ld = 4 * E
    R = FV.REACHES[reach]
    Bc = (4 * (R // (ld * 4) + 1) + 26) // 27 + 1        # (t - 1) * Bc + (G - 1) * gs = 6.75 Bc + 9 rows: just past the reach
    gs = Bc // 4 + 3
    at = [j * Bc + g * gs for j in range(t) for g in range(G)]
    assert at == sorted(at) and (G - 1) * gs < Bc and R < at[-1] * ld * 4 < R + R // 8
    offs = [a * ld * 4 for a in at]
    assert len({o % (1 << 32) for o in offs}) == len(offs)
    for th in FV.REACHES.values():
        if th <= R:
            assert offs[0] < th <= offs[-1]
    vals = torch.cat([rnd(t * G, 3 * E, seed=5), torch.zeros(t * G, E)], dim=1)
    idx = torch.tensor(at)

    def run(c):
        buf = FV.far_rows(vals, at, ld, c.fill)
        c.fars.append(buf)
        c.big += buf._far.parent.numel()
        q, k, v, o = (buf[:, i * E:(i + 1) * E] for i in range(4))
        got = {}
        for algo, terms in (ALGOS[:2] if causal else ALGOS):
            buf[idx.cuda(), 3 * E:] = 0.0
            with attention_algo(ops, algo):
                ops.attention(q, k, v, G, H, t, t, q_group_stride=gs, q_inner=1, q_outer_stride=Bc, k_group_stride=gs, k_stride=Bc,
                              causal=causal, out=o, kv_terms=terms)
            FV.check_untouched(buf, "attention position-major algo %d" % algo)
            got["algo%d terms%d" % (algo, terms)] = buf[idx.cuda(), 3 * E:].clone()
        return got
    got = both(run, "attention position-major %s causal=%s" % (reach, causal))
    x = vals[:, :3 * E].double().view(t, G, 3, H, 64).permute(2, 1, 3, 0, 4)
    ref = ref_attention(x[0], x[1], x[2], None, causal).permute(2, 0, 1, 3).reshape(t * G, E)
    assert len(got) == (2 if causal else 5)
    gm = lambda m: m.reshape(t, G, E).transpose(0, 1).reshape(G * t, E).contiguous()      # rows (j, g) -> group-major (g, j)
    for k, v in got.items():
        if k.endswith("terms1"):
            _h1_check(gm(v), gm(vals[:, :E]), gm(vals[:, E:2 * E]), gm(vals[:, 2 * E:3 * E]), G, H, t, t)
        else:
            assert rel_err(v, ref) < 5e-6, (k, reach, causal)


@pytest.mark.parametrize("which", ["q", "k", "v", "o", "attn_bias", "attn_mask"])
def test_attention_general_far_ld(ops, which):
    """ff_attention_general with a far q, k, v or o (ldq ... ldo) and a far 2-D attn_bias / attn_mask (attn_ld) at B32 --
    position-major rows, kv_len and a key mask.  The descriptor is filled here: the wrapper always passes a tight bias / mask."""
    L = ops._L
    G, H, hd, nq, nk = 2, 3, 48, 5, 37
    E = H * hd
    keep = torch.tensor([max(1, nk - 3 * g - nk // 4) for g in range(G)])
    kpm = torch.arange(nk)[None, :] >= keep[:, None]
    kpm[:, 1] = True
    bias = rnd(nq, nk, seed=3, scale=2.0)
    amask = rnd(nq, nk, seed=5) > 0.5
    amask[:, 0] = False
    t = {"q": rnd(nq * G, E, seed=1), "k": rnd(nk * G, E, seed=2), "v": rnd(nk * G, E, seed=3), "o": torch.zeros(nq * G, E),
         "attn_bias": bias, "attn_mask": amask.to(torch.uint8)}

    def run(c):
        x = {n: (c.far(v, FV.B32) if n == which else c.tight(v, n) if n.startswith("attn") else c.c(v, n)) for n, v in t.items()}
        d = L.AttnGeneralDesc()
        d.q, d.k, d.v, d.o = (x[n].data_ptr() for n in "qkvo")
        d.ldq, d.ldk, d.ldv, d.ldo = (x[n].stride(0) for n in "qkvo")
        d.num_groups, d.num_heads, d.head_dim, d.nq, d.nk = G, H, hd, nq, nk
        d.q_group_stride, d.q_inner, d.q_outer_stride, d.k_group_stride, d.k_stride = 1, 1, G, 1, G
        d.kv_len, d.key_mask, d.mask_stride = c.tight(keep.to(torch.int32), "kv_len").data_ptr(), c.tight(kpm.to(torch.uint8), "key_mask").data_ptr(), nk
        d.scale = float(hd) ** -0.5
        outs = {}
        for names in ([(which,)] if which.startswith("attn") else [("attn_bias", "attn_mask")]):   # (one attn_ld for both: a far one goes in alone)
            d.attn_bias = d.attn_mask = None
            d.attn_ld = x[names[0]].stride(0)
            for n in names:
                setattr(d, n, x[n].data_ptr())
            x["o"].zero_()
            L.check(L.load().ff_attention_general(C.byref(d), _stream()), "ff_attention_general")
            outs["+".join(names)] = x["o"].clone()
        return outs
    got = both(run, "ff_attention_general far %s" % which)
    qd = t["q"].double().view(nq, G, H, hd).permute(1, 2, 0, 3)
    kd, vd = (t[n].double().view(nk, G, H, hd).permute(1, 2, 0, 3) for n in "kv")
    for name, out in got.items():
        ref = _ref_attention_general(qd, kd, vd, hd, kpm, False, bias if "attn_bias" in name else None, amask if "attn_mask" in name else None)
        assert torch.isfinite(out).all() and rel_err(out, ref.permute(2, 0, 1, 3).reshape(nq * G, E)) < 5e-6, (which, name)


# ---- row operators ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["x", "y", "ypos", "pos"])
def test_layernorm_far(ops, which, reach):
    """ff_layernorm: far x, y, ypos (ldx, ldy, ldypos) and a far position table (ldpos), E in {64, 128, 512} on the first E columns
    of 512-column operands."""
    lib = ops._L.load()
    rows, div, mod, EM = 7, 2, 3, 512
    x = rnd(rows, EM, seed=1, scale=3.0) + 0.5
    gam, bet, pos = rnd(EM, seed=2) + 1.0, rnd(EM, seed=3), rnd(mod, EM, seed=4)
    t = {"x": x, "y": torch.zeros(rows, EM), "ypos": torch.zeros(rows, EM), "pos": pos}

    def run(c):
        d = {n: (c.far(v, FV.REACHES[reach]) if n == which else c.c(v, n)) for n, v in t.items()}
        got = {}
        for E in (64, 128, 512):
            g, b = c.tight(gam[:E].contiguous()), c.tight(bet[:E].contiguous())
            d["y"].zero_(), d["ypos"].zero_()
            ops._L.check(lib.ff_layernorm(d["x"].data_ptr(), d["x"].stride(0), g.data_ptr(), b.data_ptr(), 1e-5, d["y"].data_ptr(),
                                          d["y"].stride(0), d["ypos"].data_ptr(), d["ypos"].stride(0), d["pos"].data_ptr(), d["pos"].stride(0),
                                          div, mod, rows, E, _stream()), "ff_layernorm")
            got["y%d" % E], got["ypos%d" % E] = d["y"].clone(), d["ypos"].clone()
        return got
    got = both(run, "ff_layernorm far %s %s" % (which, reach))
    for E in (64, 128, 512):
        ref = F.layer_norm(x[:, :E].double(), (E,), gam[:E].double(), bet[:E].double(), 1e-5)
        y, yp = got["y%d" % E], got["ypos%d" % E]
        assert rel_err(y[:, :E], ref) < 2e-6 and rel_err(yp[:, :E], ref + pos[:, :E].double()[(torch.arange(rows) // div) % mod]) < 2e-6
        assert not bool(y[:, E:].any()) and not bool(yp[:, E:].any())


@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["x", "pos", "out"])
def test_add_pos_far(ops, which, reach):
    lib = ops._L.load()
    rows, E, div, mod = 37, 128, 5, 7
    t = {"x": rnd(rows, E, seed=1), "pos": rnd(mod, E, seed=2), "out": torch.zeros(rows, E)}

    def run(c):
        d = {n: (c.far(v, FV.REACHES[reach]) if n == which else c.c(v, n)) for n, v in t.items()}
        ops._L.check(lib.ff_add_pos(d["x"].data_ptr(), d["x"].stride(0), d["pos"].data_ptr(), d["pos"].stride(0), div, mod,
                                    d["out"].data_ptr(), d["out"].stride(0), rows, E, _stream()), "ff_add_pos")
        return {"out": d["out"].clone()}
    assert torch.equal(both(run, "ff_add_pos far %s %s" % (which, reach))["out"], t["x"] + t["pos"][(torch.arange(rows) // div) % mod])


@pytest.mark.parametrize("reach", REACH_IDS)
def test_gelu_far(ops, reach):
    v = rnd(37, 128, seed=3, scale=2.5)
    got = both(lambda c: {"x": ops.gelu_(c.far(v, FV.REACHES[reach])).clone()}, "ff_gelu far %s" % reach)
    want = F.gelu(v.double())
    assert float((got["x"].double() - want).abs().max()) < 4e-7 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["out", "memory"])
def test_gather_rows_far(ops, which, reach):
    """ff_gather_rows: a far out (ldout), and a far memory -- three wireframes whose S * E is so large that the last key of the
    last wireframe lies past the reach (only the gathered rows exist; every other row of the memory is fill)."""
    lib = ops._L.load()
    R = FV.REACHES[reach]
    N, E, spg = 3, 128, 2
    S = 20 if which == "out" else R // (N * E * 4) + 2
    tok = torch.tensor([0, S - 1, 5, S - 1, 0, S - 1], dtype=torch.int32)          # first and last key of a wireframe
    at = sorted({(i // spg) * S + int(k) for i, k in enumerate(tok)})
    rows = rnd(len(at), E, seed=4)
    want = torch.stack([rows[at.index((i // spg) * S + int(k))] for i, k in enumerate(tok)])

    def run(c):
        if which == "memory":
            mem = FV.far_rows(rows, at, E, c.fill)
            c.fars.append(mem)
            c.big += mem._far.parent.numel()
            assert FV.farthest(mem) > R
            out = c.c(torch.zeros(tok.numel(), E), "out")
        else:
            full = torch.zeros(N * S, E)
            full[at] = rows
            mem, out = c.tight(full, "memory"), c.far(torch.zeros(tok.numel(), E), R)
        ops._L.check(lib.ff_gather_rows(mem.data_ptr(), S, E, c.tight(tok, "tok").data_ptr(), tok.numel(), spg, out.data_ptr(),
                                        out.stride(0), _stream()), "ff_gather_rows")
        return {"out": out.clone()}
    assert torch.equal(both(run, "ff_gather_rows far %s %s" % (which, reach))["out"], want)


@pytest.mark.parametrize("width", [512, 6])
@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["src", "dst"])
def test_permute_rows_far(ops, which, reach, width):
    """ff_permute_rows, npos = 3: src_rows (dst_rows) so large that (j * rows + idx) * width passes the reach at the last position;
    width 512 takes the 16-byte loads, width 6 the scalar path."""
    lib = ops._L.load()
    R = FV.REACHES[reach]
    npos, rows, small = 3, 7, 11
    big = R // (npos * width * 4) + 2                     # row (npos - 1) * big + big - 1 starts just past the reach
    idx = torch.tensor([big - 1, 0, 3, big // 2, 1, 6, 4], dtype=torch.int32)             # (distinct; the first and the last row)
    sidx = torch.tensor([10, 0, 3, 8, 1, 6, 4], dtype=torch.int32)
    at = sorted(j * big + int(i) for j in range(npos) for i in idx)
    vals = rnd(npos * rows, width, seed=1)
    compact = rnd(npos, small, width, seed=2)

    def run(c):
        far = FV.far_rows(vals if which == "src" else torch.full((npos * rows, width), 7.0), at, width, c.fill)
        c.fars.append(far)
        c.big += far._far.parent.numel()
        assert FV.farthest(far) > R
        di, ds = c.tight(idx, "far idx"), c.tight(sidx, "small idx")
        if which == "src":          # dst[j, i] = src[j, idx[i]]
            dst = c.tight(torch.full((npos, small, width), 7.0), "dst")
            ops._L.check(lib.ff_permute_rows(far.data_ptr(), big, di.data_ptr(), dst.data_ptr(), small, None, npos, rows, width, _stream()),
                         "ff_permute_rows")
            return {"dst": dst.clone()}
        src = c.tight(compact, "src")   # dst[j, idx[i]] = src[j, sidx[i]]
        ops._L.check(lib.ff_permute_rows(src.data_ptr(), small, ds.data_ptr(), far.data_ptr(), big, di.data_ptr(), npos, rows, width,
                                         _stream()), "ff_permute_rows")
        return {"dst": far[torch.tensor(at).cuda()].clone()}
    got = both(run, "ff_permute_rows far %s %s width %d" % (which, reach, width))["dst"]
    if which == "src":
        want = torch.full((npos, small, width), 7.0)
        for j in range(npos):
            for i, k in enumerate(idx):
                want[j, i] = vals[at.index(j * big + int(k))]
    else:
        want = torch.empty(npos * rows, width)
        for j in range(npos):
            for i, k in enumerate(idx):
                want[at.index(j * big + int(k))] = compact[j, int(sidx[i])]
    assert torch.equal(got, want)


@pytest.mark.parametrize("reach", REACH_IDS)
def test_assemble_embedding_far_ld_edge(ops, reach):
    lib = ops._L.load()
    N, L, E, nt = 3, 5, 64, 4
    tok_embed, edge = rnd(nt, E, seed=1), rnd(N * L, E, seed=2)

    def run(c):
        out, de = c.tight(torch.zeros(N, L + nt, E), "out"), c.far(edge, FV.REACHES[reach])
        ops._L.check(lib.ff_assemble_embedding(c.tight(tok_embed, "tok_embed").data_ptr(), nt, de.data_ptr(), de.stride(0), N, L, E,
                                               out.data_ptr(), _stream()), "ff_assemble_embedding")
        return {"out": out.clone()}
    want = torch.cat([tok_embed[None].expand(N, nt, E), edge.view(N, L, E)], dim=1)
    assert torch.equal(both(run, "ff_assemble_embedding far %s" % reach)["out"], want)


# ---- pointer family ---------------------------------------------------------------------------------------------------------------
FILL = torch.finfo(torch.float32).min


def _pointer_case(W, F_, S, E):
    B = W * F_
    p, mem = rnd(B, E, seed=1), rnd(W, S, E, seed=2)
    mask = torch.zeros(W, S, dtype=torch.bool)
    kv_len = torch.full((W,), S, dtype=torch.int32)
    for w in range(W):
        mask[w, S - w - 1:] = True
        kv_len[w] = S - w - 1
    raw = torch.einsum("be,bse->bs", p.double(), mem.double()[torch.arange(B) // F_])
    return B, p, mem, mask, kv_len, raw


@pytest.mark.parametrize("S", [5, 70])
@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["p", "logits", "extra", "rows"])
def test_pointer_argmax_far(ops, which, reach, S):
    """ff_pointer_argmax and ff_pointer_argmax_lp: far p (ldp), logits (ldlogits), extra_mask (ldextra), next_rows (ldnext); the
    rules of test_pointer_argmax and, for the log-probability, of test_logprob (2^-16 of fp64 on the kernel's own logits)."""
    lib = ops._L.load()
    W, F_, E = 2, 4, 128
    B, p, mem, mask, kv_len, raw = _pointer_case(W, F_, S, E)
    extra = (rnd(B, S, seed=7) > 1.0).to(torch.uint8)
    extra[:, 0] = 0
    t = {"p": p, "logits": torch.zeros(B, S), "extra": extra, "rows": torch.zeros(B, E)}

    def run(c):
        d = {n: (c.far(v, FV.REACHES[reach]) if n == which else c.c(v, n)) for n, v in t.items()}
        dm, dmask, dkv = c.tight(mem, "memory"), c.tight(mask.to(torch.uint8), "mask"), c.tight(kv_len, "kv_len")
        got = {}
        for lp in (False, True):
            o = {"next": c.tight(torch.zeros(B, dtype=torch.int32)), "best": c.tight(torch.zeros(B)), "second": c.tight(torch.zeros(B)),
                 "counters": c.tight(torch.zeros(2, dtype=torch.int32)), "logprob": c.tight(torch.zeros(B))}
            d["logits"].zero_(), d["rows"].zero_()
            args = (d["p"].data_ptr(), d["p"].stride(0), dm.data_ptr(), S, E, dmask.data_ptr(), dkv.data_ptr(), d["extra"].data_ptr(),
                    d["extra"].stride(0), B, F_, o["next"].data_ptr(), o["best"].data_ptr(), o["second"].data_ptr(), d["logits"].data_ptr(),
                    d["logits"].stride(0), d["rows"].data_ptr(), d["rows"].stride(0), o["counters"].data_ptr(), 4,
                    o["counters"].data_ptr() + 4, 3)
            if lp:
                ops._L.check(lib.ff_pointer_argmax_lp(*args, o["logprob"].data_ptr(), _stream()), "ff_pointer_argmax_lp")
            else:
                ops._L.check(lib.ff_pointer_argmax(*args, _stream()), "ff_pointer_argmax")
            for k, v in dict(o, logits=d["logits"], rows=d["rows"]).items():
                got["%s lp=%s" % (k, lp)] = v.clone()
        return got
    got = both(run, "ff_pointer_argmax far %s %s S=%d" % (which, reach, S))
    dead = mask[torch.arange(B) // F_] | extra.bool()
    want = raw.masked_fill(dead, FILL)
    for lp in (False, True):
        g = {k.split()[0]: v for k, v in got.items() if k.endswith("lp=%s" % lp)}
        logits = g["logits"].double()
        assert torch.equal(logits[dead], want[dead])
        assert float((logits[~dead] - want[~dead]).abs().max()) < 1e-4 * float(want[~dead].abs().max())
        nxt = g["next"].long()
        assert torch.equal(nxt, torch.argmax(g["logits"], dim=1))
        top2 = torch.sort(g["logits"], dim=1, descending=True).values
        assert torch.equal(g["best"], top2[:, 0]) and torch.equal(g["second"], top2[:, 1])
        assert torch.equal(g["rows"], mem[torch.arange(B) // F_, nxt])
        assert g["counters"].tolist() == [int((nxt >= 4).sum()), int((nxt == 3).sum())]
        if lp:
            ref = torch.log_softmax(logits.masked_fill(dead, float("-inf")), dim=1)[torch.arange(B), nxt]
            assert float((g["logprob"].double() - ref).abs().max()) <= 2.0 ** -16
    for k in ("next", "best", "second", "logits", "rows"):
        RZ.assert_same_bits(got["%s lp=False" % k], got["%s lp=True" % k], "ff_pointer_argmax_lp changes %s" % k)


def _same_as_plain(got, plain, what):
    """The far call returns the bits of the same call on plain tight tensors, whose rules against the numpy references
    (tests/forced_ref.py, sample_ref.py, constrain_ref.py, beam_ref.py) are asserted in the op's own test file."""
    n = 0
    for k, v in plain.items():
        if torch.is_tensor(v):
            RZ.assert_same_bits(got[k], v.cpu(), "%s: %s against the plain call" % (what, k))
            n += 1
    assert n >= 3


@pytest.mark.parametrize("S", [5, 70])
@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("op", ["forced", "sample", "constrained"])
def test_pointer_selection_ops_far_logits(ops, op, reach, S):
    """ff_pointer_forced / ff_pointer_sample / ff_pointer_constrained with far logits (ldlogits): the masked row they leave, and
    every output, bit-equal to the call on tight tensors; the forced log-probability also within forced_ref.LP_BAR of fp64."""
    import constrain_ref as CR
    import forced_ref as FR
    W, F_, E, ntok = 2, 4, 128, 4
    L = S - ntok
    B, p, mem, mask, kv_len, raw = _pointer_case(W, F_, S, E)
    raw, mask8 = raw.float(), mask.to(torch.uint8)
    fin = (torch.arange(B) % 4 == 3).to(torch.int32)
    forced = (torch.arange(B) * 5 % max(1, S - W - 1)).to(torch.int32)
    u = torch.rand(B + 3, generator=torch.Generator().manual_seed(3))
    row_id = ((torch.arange(B) * 7) % (B + 3)).to(torch.int32)
    first = (torch.arange(B) % max(1, L)).to(torch.int32)
    prev = ((torch.arange(B) * 3) % max(1, L)).to(torch.int32)
    fw = (L + 31) // 32
    vis = np.zeros((B, fw), dtype=np.uint32)
    for b in range(B):
        for e_ in (int(first[b]), int(prev[b])):
            vis[b, e_ >> 5] |= np.uint32(1 << (e_ & 31))
    visited = torch.from_numpy(vis.view(np.int32))

    def call(lg, e):
        if op == "forced":
            o = ops.pointer_forced(lg, e(forced), e(mem), e(mask8), e(kv_len), seqs_per_group=F_, want_rows=True, want_stats=True)
        elif op == "sample":
            o = ops.pointer_sample(lg, e(u), row_id=e(row_id), fin=e(fin), memory=e(mem), mask=e(mask8), kv_len=e(kv_len),
                                   counter=e(torch.zeros(1, dtype=torch.int32)), temperature=0.8, top_k=5, top_p=0.9, seqs_per_group=F_,
                                   term_range=(1, 4), want_rows=True, want_stats=True, ge_bound=4)
        else:
            o = ops.pointer_constrained(lg, e(fin), e(first), e(prev), e(visited), CR.NO_REPEAT, ntok, memory=e(mem), mask=e(mask8),
                                        kv_len=e(kv_len), seqs_per_group=F_, term_range=(1, 4), want_rows=True, want_stats=True,
                                        counter=e(torch.zeros(1, dtype=torch.int32)))
        return dict(o, logits=lg)
    plain = call(raw.cuda(), lambda x: x.cuda())
    got = both(lambda c: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in call(c.far(raw, FV.REACHES[reach]), c.tight).items()},
               "ff_pointer_%s far logits %s S=%d" % (op, reach, S))
    _same_as_plain(got, plain, "ff_pointer_%s" % op)
    assert torch.isfinite(got["logprob"]).all()
    # ... and the numpy rules themselves (tests/forced_ref.py, sample_ref.py, constrain_ref.py), on the masked rows the far call left
    rows64, lp = got["logits"].double().numpy(), got["logprob"].double().numpy()
    w_of = np.arange(B) // F_
    pad = mask.numpy()[w_of] | (np.arange(S)[None, :] >= kv_len.numpy()[w_of][:, None])
    close = lambda a, b: bool((np.abs(a - b) <= FR.LP_BAR + FR.EPS * np.abs(b)).all())
    if op == "forced":
        assert (rows64[pad] == FILL).all() and np.array_equal(rows64[~pad], raw.double().numpy()[~pad])
        rlp, rgreedy, rrank = FR.forced_rule(rows64, forced.numpy().astype(np.int64))
        assert close(lp, rlp) and np.array_equal(got["greedy"].numpy(), rgreedy) and np.array_equal(got["rank"].numpy(), rrank)
        assert torch.equal(got["rows"], mem[torch.arange(B) // F_, forced.long()])
    elif op == "sample":
        import sample_ref as SR
        tok, _, decisive, _ = SR.sample_rows(rows64, u.numpy()[row_id.numpy()], 0.8, 5, 0.9, fin.numpy())
        nxt = got["next"].numpy()
        assert decisive.any() and np.array_equal(nxt[decisive], tok[decisive])
        live = fin.numpy() == 0
        assert (nxt[~live] == 0).all() and (lp[~live] == 0).all()
        assert close(lp[live], np.array([SR.logprob_of(rows64[b], nxt[b]) for b in np.where(live)[0]]))
        assert np.array_equal(got["fin"].numpy() != 0, ~live | ((nxt >= 1) & (nxt < 4) & live))
        assert torch.equal(got["rows"][torch.from_numpy(live)], mem[torch.arange(B) // F_, got["next"].long()][torch.from_numpy(live)])
    else:
        for b in range(B):
            state = (frozenset({int(first[b]), int(prev[b])}), int(first[b]), int(prev[b]))
            r = CR.step_row(raw[b].double().numpy(), pad[b], state, CR.NO_REPEAT, ntok, (1, 4), None, finished=bool(fin[b]))
            assert int(got["next"][b]) == r["tok"] and bool(got["fin"][b]) == bool(r["fin"]) and bool(got["dead_end"][b]) == bool(r["dead"]), b
            assert abs(lp[b] - r["logprob"]) <= CR.LP_BAR + CR.EPS * abs(r["logprob"]), b
            assert np.array_equal(rows64[b], r["row"]), b                                   # (the same fp32 values, masked the same way)
            if not fin[b]:
                assert np.array_equal(got["mask_rows"][b].numpy() != 0, r["masked"]), b


@pytest.mark.parametrize("S", [5, 70])
@pytest.mark.parametrize("reach", REACH_IDS)
@pytest.mark.parametrize("which", ["logits", "hist"])
def test_beam_select_far(ops, which, reach, S):
    """ff_beam_select with far logits (ldlogits) and a far token history (ldhist): bit-equal to the call on tight tensors."""
    W, F_, E, width, t = 2, 2, 128, 2, 2
    B = W * F_ * width
    p, mem = rnd(B, E, seed=1), rnd(W, S, E, seed=2)
    mask = torch.zeros(W, S, dtype=torch.uint8)
    kv_len = torch.full((W,), S, dtype=torch.int32)
    for w in range(W):
        mask[w, S - w - 1:] = 1
        kv_len[w] = S - w - 1
    raw = torch.einsum("be,bse->bs", p, mem[torch.arange(B) // (F_ * width)])
    scores = -rnd(B, seed=4).abs()
    fin = (torch.arange(B) % 5 == 4).to(torch.int32)
    hist = torch.arange((t + 1) * B, dtype=torch.int32).view(t + 1, B) % S

    def call(lg, h, e):
        o = ops.beam_select(lg, e(scores), e(fin), width, groups_per_wireframe=F_, mask=e(mask), kv_len=e(kv_len), hist=h, t=t,
                            term_range=(1, 4), memory=e(mem), want_rows=True, counter=e(torch.zeros(1, dtype=torch.int32)), ge_bound=4)
        return dict(o, logits=lg, hist=h)
    plain = call(raw.cuda(), hist.cuda(), lambda x: x.cuda())
    R = FV.REACHES[reach]
    got = both(lambda c: {k: v.clone() for k, v in call(c.far(raw, R) if which == "logits" else c.c(raw, "logits"),
                                                        c.far(hist, R) if which == "hist" else c.c(hist, "hist"), c.tight).items()},
               "ff_beam_select far %s %s S=%d" % (which, reach, S))
    _same_as_plain(got, plain, "ff_beam_select")
    # ... and the numpy rule (tests/beam_ref.py) on the masked rows the far call left, wherever its gap is decisive
    import beam_ref as BR
    ref = BR.beam_step(got["logits"].double().numpy(), scores.double().numpy(), fin.numpy() != 0, width, 1, 4, ge_bound=4)
    sure = np.repeat(ref["gap"] > 1, width)
    assert sure.any()
    for key, name in (("parent", "parent"), ("next", "tok")):
        assert np.array_equal(got[key].numpy()[sure], ref[name][sure]), key
    assert np.array_equal(got["fin"].numpy()[sure] != 0, ref["fin"][sure])
    sc, rsc = got["scores"].double().numpy()[sure], ref["scores"][sure]
    assert np.array_equal(np.isinf(sc), np.isinf(rsc))
    assert all(abs(a - b) <= BR.score_bound(b) for a, b in zip(sc, rsc) if np.isfinite(b))


@pytest.mark.parametrize("reach", REACH_IDS)
def test_beam_reorder_far_rows_per_pos(ops, reach):
    """ff_beam_reorder, npos = 3: rows_per_pos so large that the last position's rows lie past the reach (the engine's cached
    prefixes of a very large micro-batch; only the first groups * width rows of a position are beams)."""
    lib = ops._L.load()
    R = FV.REACHES[reach]
    npos, groups, width, wa, wb = 3, 3, 2, 64, 12
    B = groups * width
    rpp = R // ((npos - 1) * wb * 4) + 2                      # rows_b (12 floats per row) passes the reach; rows_a (64) well past it
    parent = torch.tensor([1, 1, 0, 0, 1, 0], dtype=torch.int32)
    at = [j * rpp + r for j in range(npos) for r in range(B)]
    a, b = rnd(npos * B, wa, seed=8), rnd(npos * B, wb, seed=9)

    def run(c):
        rb = FV.far_rows(b, at, wb, c.fill)
        c.fars.append(rb)
        c.big += rb._far.parent.numel()
        assert FV.farthest(rb) > R
        ra = c.tight(a.view(npos, B, wa), "rows_a")
        ia = torch.tensor(at).cuda()
        # (one rows_per_pos per call: the far rows go in alone, with rows_per_pos = rpp; the tight ones with rows_per_pos = B)
        ops._L.check(lib.ff_beam_reorder(rb.data_ptr(), wb, None, 0, rpp, npos, c.tight(parent, "parent").data_ptr(), groups, width,
                                         _stream()), "ff_beam_reorder")
        ops._L.check(lib.ff_beam_reorder(ra.data_ptr(), wa, None, 0, B, npos, c.tight(parent, "parent").data_ptr(), groups, width,
                                         _stream()), "ff_beam_reorder")
        return {"rows_a": ra.clone(), "rows_b": rb[ia].clone()}
    got = both(run, "ff_beam_reorder far %s" % reach)
    src = torch.arange(B) // width * width + parent.long()
    assert torch.equal(got["rows_a"], a.view(npos, B, wa)[:, src]) and torch.equal(got["rows_b"].view(npos, B, wb), b.view(npos, B, wb)[:, src])


# ---- one whole-batch decode past 2^32 bytes ---------------------------------------------------------------------------------------
ENG = dict(E=128, H=2, FF=256, enc=1, dec=2, L=60, F=60, T=9, in_dim=100, ntok=4)
LOGIT_TOL, LOGIT_SCALE = 1e-3, 40.0          # tests/test_parity_golden.py
SLICE = 16
_ENGINES = {}


def _engine(planes):
    """E = 128, H = 2, FF = 256, one encoder and two decoder layers, L = 60 (S = 64), T = 9: name-keyed synthetic weights of the
    'gain4' recipe (faceformer_amd.synth), bound once per module in f32 and with the 2 x fp16 planes."""
    if planes not in _ENGINES:
        from faceformer_amd import synth
        from faceformer_amd.hip.engine import PathEngine
        spec = synth.state_dict_spec("parallel", ENG["L"], ENG["T"], ENG["E"], ENG["FF"], ENG["enc"], ENG["dec"], ENG["in_dim"], ENG["ntok"])
        sd = {k: v.cuda() for k, v in synth.make_state_dict(spec, "gain4", 0).items() if v.is_floating_point()}
        _ENGINES[planes] = PathEngine(sd, ENG["H"], ENG["ntok"], bf16_split_planes=planes, split_kind="fp16x2")
    return _ENGINES[planes]


def _encode_in_pieces(eng, inp, mask, piece=512):
    """The encoder is per wireframe: 512 at a time (its size is not what this test is about)."""
    mem = torch.empty((inp.shape[0], mask.shape[1], eng.E), device="cuda", dtype=torch.float32)
    kv = torch.empty(inp.shape[0], device="cuda", dtype=torch.int32)
    for i in range(0, inp.shape[0], piece):
        mem[i:i + piece], kv[i:i + piece] = eng.encode(inp[i:i + piece], mask[i:i + piece])
    eng._ws = None
    return mem, kv


def _decode_kwargs(form):
    from faceformer_amd.hip import lib as L
    from faceformer_amd.hip.engine import DEFAULT_FLAGS
    if form == "f32 folded":
        return dict(flags=DEFAULT_FLAGS, ln_fuse_max_rows=1 << 30)                 # (E = 128: the default folds up to 12288 rows only)
    if form == "f32 unfolded":
        return dict(flags=DEFAULT_FLAGS & ~L.FF_FUSE_LAYERNORM)
    return dict(flags=DEFAULT_FLAGS, x3_min_rows=1024)                             # "planes": the split products from 1024 rows on


def _workspace_bytes(eng, N, kw):
    from faceformer_amd.hip import lib as L
    prm = L.DecodeParams()
    prm.variant, prm.N, prm.L, prm.F, prm.T = L.FF_PARALLEL, N, ENG["L"], ENG["F"], ENG["T"]
    prm.flags = kw["flags"] | L.FF_NO_STOP
    prm.x3_min_rows = kw.get("x3_min_rows", 0) if eng._planes else 0
    prm.ln_fuse_max_rows = kw.get("ln_fuse_max_rows", 0)
    ni = (C.c_int * N)(*([ENG["F"]] * N))
    return int(eng._lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni))


def _decode(eng, mem, mask, kv, kw):
    from faceformer_amd.hip import lib as L
    return eng.decode(mem, mask, kv, L.FF_PARALLEL, T=ENG["T"], F=ENG["F"], num_input=[ENG["F"]] * mem.shape[0], chunk_wireframes=0,
                      chunk_max_seqs=0, sync_every=0, no_stop=True, trace=True, **kw)


def _profiled_decode(eng, mem, mask, kv, kw):
    """(outputs, launches by profile category) of one decode: category 0 the f32 GEMM family, 6 the split kernels."""
    from faceformer_amd.hip import lib as L
    L.check(eng._lib.ff_profile_begin(), "ff_profile_begin")
    try:
        out = _decode(eng, mem, mask, kv, kw)
    finally:
        ncat = 8
        ms, work, launches = (C.c_double * ncat)(), (C.c_double * ncat)(), (C.c_longlong * ncat)()
        L.check(eng._lib.ff_profile_end(ms, work, launches, ncat), "ff_profile_end")
    return out, list(launches)


def _compare_slice(big, ref, w0, what):
    """The rules of test_config_c_batch_of_256_edge_wireframes_full_size: tokens equal wherever the reference's top-2 margin exceeds
    twice the logit tolerance, best logits within the tolerance while the prefixes agree, step 0 logits within it unconditionally;
    at least 90 % of the slice's tokens fall under the decisive-margin rule."""
    F_, T = ENG["F"], ENG["T"]
    steps = T - 1
    assert big["steps"] == ref["steps"] == steps, what
    rows = slice(w0 * F_, (w0 + SLICE) * F_)
    pred = big["predict"][rows].cpu().numpy()
    best = big["best"][:, rows].cpu().numpy()
    rpred, rbest, rsecond = ref["predict"].cpu().numpy(), ref["best"].cpu().numpy(), ref["second"].cpu().numpy()
    tol = LOGIT_TOL * max(1.0, float(np.abs(rbest).max()) / LOGIT_SCALE)
    assert np.array_equal(pred[:, 0], rpred[:, 0]), what
    alive = np.ones(SLICE * F_, dtype=bool)
    n_cmp = 0
    for s in range(steps):
        must = alive & (rbest[s] - rsecond[s] > 2 * tol)
        same = pred[:, s + 1] == rpred[:, s + 1]
        assert same[must].all(), "%s step %d: token mismatch at a decisive margin" % (what, s)
        d = np.abs(best[s] - rbest[s])[alive]
        assert d.size == 0 or d.max() <= tol, "%s step %d: best logit off by %g (tolerance %g)" % (what, s, d.max(), tol)
        n_cmp += int(must.sum())
        alive &= same
    assert n_cmp >= 0.9 * SLICE * F_ * steps, "%s: only %d of %d tokens at a decisive margin" % (what, n_cmp, SLICE * F_ * steps)
    lg, rlg = big["logits"][0, rows].cpu().numpy(), ref["logits"][0].cpu().numpy()
    fill = np.finfo(np.float32).min
    scale = float(np.abs(rlg[rlg > fill]).max())
    assert np.abs(lg - rlg).max() <= LOGIT_TOL * max(1.0, scale / LOGIT_SCALE), "%s: step 0 logits" % what


@pytest.mark.parametrize("reach", ["B32", "E31"])
def test_whole_batch_decode_past_2_32_bytes(hip_lib, reach):
    """FF_PARALLEL, greedy, FF_NO_STOP, ONE micro-batch (chunk_wireframes = chunk_max_seqs = 0) of N distinct wireframes x 60
    sequences whose q|k|v buffer at the last step (8 N 60 x 384 floats) passes 2^32 bytes already where its newest position starts
    (B32: N = 6700, 402 000 sequences, 3.2 M rows) or 2^33 bytes = 2^31 elements (E31: N = 13 400): every grid dimension, row index
    and workspace offset of the decode at a size no other test reaches.  f32 with the LayerNorm-folded projections on and off, and the 2 x fp16 split products.  Reference:
    the same engine on 16-wireframe slices decoded alone (the form the goldens pin) -- the first 16, the last 16, and the 16
    around the wireframes whose q|k|v rows of the last step contain the 2^31-, 2^32- (and 2^33-) byte marks.
    Skips only when the card's free memory is below 1.5 x (workspace + inputs and outputs); on an idle MI355X neither case skips."""
    from faceformer_amd.hip import lib as L
    F_, T, S, E = ENG["F"], ENG["T"], ENG["L"] + ENG["ntok"], ENG["E"]
    row_bytes = 3 * E * 4
    # N: the first hundred at which the NEWEST position of the last step (rows 7 Bc ...; what decoder_pass calls newoff) starts past
    # the reach -- 2^32 / (7 x 60 x 1536) = 6657.7 -- and twice that.  (5900 wireframes would put the END of the buffer past
    # 2^32 bytes, but an offset of the newest position computed in 32 bits would still be right there.)
    N = {"B32": 6700, "E31": 13400}[reach]
    Bc = N * F_
    assert (T - 2) * Bc * row_bytes > FV.REACHES[reach] and Bc > 65535 * 4
    forms = ["f32 folded", "f32 unfolded", "planes"]
    _free()
    need_ws = max(_workspace_bytes(_engine(f == "planes"), N, _decode_kwargs(f)) for f in forms)
    io = N * ENG["L"] * ENG["in_dim"] * 4 + N * S * E * 4 + 2 * ((T - 1) * Bc * (S + 2) * 4) + Bc * T * 8
    free = torch.cuda.mem_get_info()[0]
    if free < 1.5 * (need_ws + io):
        pytest.skip("the decode needs %d bytes of workspace and %d of inputs and outputs; %d bytes are free" % (need_ws, io, free))
    gen = torch.Generator(device="cuda").manual_seed(20 + N)
    inp = torch.randn((N, ENG["L"], ENG["in_dim"]), device="cuda", generator=gen)          # every wireframe distinct
    mask = torch.zeros((N, S), device="cuda", dtype=torch.uint8)
    eng32 = _engine(False)
    mem, kv = _encode_in_pieces(eng32, inp, mask)
    del inp
    # the slices: first, last, and around every byte mark of the last step's q|k|v buffer
    starts = {"first": 0, "last": N - SLICE}
    for name, mark in (("2^31", FV.B31), ("2^32", FV.B32), ("2^33", FV.E31)):
        if mark < (T - 1) * Bc * row_bytes:
            w = (mark // row_bytes) % Bc // F_
            starts["mark " + name] = min(max(0, w - SLICE // 2), N - SLICE)
    assert len(starts) == (4 if reach == "B32" else 5)
    for form in forms:
        eng, kw = _engine(form == "planes"), _decode_kwargs(form)
        if form == "planes":
            assert eng.has_planes and eng.split_kind == "fp16x2"
        refs = {name: _decode(eng, mem[w0:w0 + SLICE], mask[w0:w0 + SLICE], kv[w0:w0 + SLICE], kw) for name, w0 in starts.items()}
        eng._ws = None
        _free()
        if form != "planes":
            big = _decode(eng, mem, mask, kv, kw)
        else:
            nb = 1000            # baseline of the routing: 60 000 sequences, every step far above x3_min_rows, no product near 2^30 elements
            assert (T - 1) * nb * F_ * ENG["FF"] < LIMIT // 8 and nb * F_ >= 16 * kw["x3_min_rows"]
            _, base = _profiled_decode(eng, mem[:nb], mask[:nb], kv[:nb], kw)
            eng._ws = None
            _free()
            big, launches = _profiled_decode(eng, mem, mask, kv, kw)
            assert launches[6] > 0, "no launch of the split kernels although their planes are bound"
            # x3_wins sends a projection with M * lda >= 2^30 to the f32 family.  With E = 128 only linear2 of the unpruned
            # layers (lda = FF = 256; the last layer runs the newest Bc rows) can get there: never at B32 (2.83 M rows x 256 <
            # 2^30), at steps 6, 7, 8 of E31 (t x 708 000 x 256 >= 2^30).  Every other launch decision is the same at both sizes
            # (all steps are far above x3_min_rows), so exactly those launches move from category 6 (split) to 0 (f32), relative
            # to the 1000-wireframe baseline decoded just before.
            moved = (ENG["dec"] - 1) * sum(1 for t in range(1, T) if t * Bc * ENG["FF"] >= LIMIT)
            assert all(t * Bc * ENG["E"] < LIMIT for t in range(1, T)) and moved == {"B32": 0, "E31": 3}[reach]
            assert (launches[0], launches[6]) == (base[0] + moved, base[6] - moved), (reach, list(base), list(launches), moved)
        assert big["slots_per_step"] == [Bc] * (T - 1) and big["decoded_seqs"] == Bc
        assert not bool(torch.isnan(big["best"]).any()) and not bool(torch.isnan(big["logits"]).any())
        for name, w0 in starts.items():
            _compare_slice(big, refs[name], w0, "%s %s, slice %s (wireframes %d..%d)" % (reach, form, name, w0, w0 + SLICE - 1))
        del big, refs
        eng._ws = None
        _free()
