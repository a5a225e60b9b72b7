"""GPU: the pruned last decoder layer with k | v folded into the query (knob FF_LAST_FOLD_MIN_ROWS).

  1  the op ff_attention_prefix_fold inside its chain -- qt | c = q_h [W'k_h | kb_h], the op, o_h = u_h W'v_h^T + b'v_h -- against
     fp64 numpy on the same operands, set against the path it replaces (ff_gemm_f32_ln k | v, then ff_attention with nq = 1) on
     the same operands: both are fp32 chains of the same length that differ in association only, so the fold may take at most
     2 x the existing path's max and rms error -- at every width the op accepts (128 .. 512 in steps of 64), staged and unstaged,
     on both sides of the staging boundary, at the largest t it accepts (the next is refused), with scores past the range of
     expf and with degenerate rows; a sequence's result has the same bits alone and in a batch
  2  the op under poisoned surroundings (tests/redzone.py): nothing outside u is written, nothing outside the t * Bc rows is read
  3  the engine with the fold at EVERY step (FF_LAST_FOLD_MIN_ROWS=1) under the rule of tests/test_parity_golden.py, with the
     profiled launch counts as evidence that the form ran, and bit-equal repeats
  3b the per-step rule across its boundaries, each with the launch counts of exactly the folding (step, micro-batch) pairs: the
     knob crossed inside a call, steps that split beside steps that fold, decodes shorter than the model's seq_len on both sides
     of the scratch guard (on ZERO and POISON workspaces)
  4  the workspace: the size query grows by exactly the per-call tables, and a decode on a poisoned workspace equals a clean one;
     the tables are laid out up to the knob = the rows of the call's longest step, not above
The five decode modes with the fold at every step: the form last_fold of tests/test_mode_forms.py.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import redzone as RZ
from conftest import batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces

pytestmark = pytest.mark.gpu

KNOB = "FF_LAST_FOLD_MIN_ROWS"
EPS = 1e-5
SCALE = 0.125
# (Bc, t, E); the last: more rows than a block keeps in LDS (80 x 512 floats > 150 KB), the u pass re-forms them from x
SHAPES = [(1, 2, 128), (5, 3, 128), (7, 5, 256), (3, 33, 512), (70, 36, 512), (2, 37, 512), (2, 80, 512)]


# ---- 1, 2: the op ---------------------------------------------------------------------------------------------------------------------
_OPERANDS = {}


def _operands(Bc, t, E):
    """Operands of one shape and their fp64 results (made once, never changed): the rows x with scales spread over three decades
    and a mean of the order of their scale, the (mean, M2) statistics per 32-column segment built in fp64 and rounded to fp32,
    folded k | v weights, a k position table (so that c is non-zero) and the newest rows' q."""
    key = (Bc, t, E)
    if key in _OPERANDS:
        return _OPERANDS[key]
    H, R = E // 64, t * Bc
    rng = np.random.default_rng(1000 * E + 37 * t + Bc)
    scale = 10.0 ** rng.uniform(-1.5, 1.5, size=(R, 1))
    x = ((rng.standard_normal((R, E)) + rng.uniform(-1, 1, size=(R, 1))) * scale).astype(np.float32)
    seg = x.astype(np.float64).reshape(R, E // 32, 32)
    mean = seg.mean(axis=2)
    stats = np.stack([mean, ((seg - mean[:, :, None]) ** 2).sum(axis=2)], axis=2).astype(np.float32)
    w = (rng.standard_normal((2 * E, E)) / np.sqrt(E)).astype(np.float32)      # rows [0, E): W'k, rows [E, 2E): W'v
    b = (0.5 * rng.standard_normal(2 * E)).astype(np.float32)
    pos = (0.5 * rng.standard_normal((t, E))).astype(np.float32)                # P[j, k columns]
    q = rng.standard_normal((Bc, E)).astype(np.float32)
    _OPERANDS[key] = _with_fp64(dict(x=x, stats=stats, w=w, b=b, pos=pos, q=q), Bc, t, E)
    return _OPERANDS[key]


def _keys_fp64(d, Bc, t, E):
    """fp64 on the operands d: (x^ [R, E] from the merged statistics, k | v [R, 2E] of every row)."""
    s64 = d["stats"].astype(np.float64)
    mu = s64[:, :, 0].mean(axis=1)
    var = (s64[:, :, 1].sum(axis=1) + 32.0 * ((s64[:, :, 0] - mu[:, None]) ** 2).sum(axis=1)) / E
    xh = (d["x"].astype(np.float64) - mu[:, None]) / np.sqrt(var + EPS)[:, None]
    kv = xh @ d["w"].astype(np.float64).T + d["b"].astype(np.float64)
    kv[:, :E] += np.repeat(d["pos"].astype(np.float64), Bc, axis=0)
    return xh, kv


def _with_fp64(d, Bc, t, E):
    """d with the fp64 results of its operands: the attention of the newest rows (o), the op's own output (u) and the scaled scores."""
    H = E // 64
    xh, kv = _keys_fp64(d, Bc, t, E)
    k = kv[:, :E].reshape(t, Bc, H, 64)
    v = kv[:, E:].reshape(t, Bc, H, 64)
    sc = SCALE * np.einsum("bhd,jbhd->bhj", d["q"].astype(np.float64).reshape(Bc, H, 64), k)
    p = np.exp(sc - sc.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    o = np.einsum("bhj,jbhd->bhd", p, v).reshape(Bc, E)
    u = np.einsum("bhj,jbe->bhe", p, xh.reshape(t, Bc, E)).reshape(Bc, H * E)
    return dict(d, o=o, u=u, scores=sc)


def _existing_path(ops, d, Bc, t, E):
    """What the engine's two-launch form computes: k | v of every row by the LayerNorm-folded projection, then the newest rows'
    attention over their t keys."""
    H = E // 64
    x, stats, w, b, pos, q = (torch.from_numpy(d[n]).cuda() for n in ("x", "stats", "w", "b", "pos", "q"))
    kv = ops.linear_ln(x, w, bias=b, stats_in=stats, eps=EPS, row_table=pos, row_div=Bc, row_cols=E)
    return ops.attention(q, kv[:, :E], kv[:, E:], num_groups=Bc, num_heads=H, nq=1, nk=t, q_group_stride=1, q_inner=1,
                         q_outer_stride=Bc, k_group_stride=1, k_stride=Bc, scale=SCALE)


def _fold_tables(d, t, E):
    """kt [H, E + t, 64] as the engine's per-call table holds it (rows < E: W'k_h transposed; row E + j: b'k_h + P[j, head h])."""
    H = E // 64
    wk, bk = d["w"][:E].reshape(H, 64, E), d["b"][:E].reshape(H, 64)
    kb = bk[:, None, :] + d["pos"].reshape(t, H, 64).transpose(1, 0, 2)
    return np.ascontiguousarray(np.concatenate([wk.transpose(0, 2, 1), kb], axis=1), dtype=np.float32)


def _fold_qt(ops, d, Bc, t, E):
    H = E // 64
    q, kt = torch.from_numpy(d["q"]).cuda(), torch.from_numpy(_fold_tables(d, t, E)).cuda()
    qt = torch.empty((Bc, H, E + t), device="cuda", dtype=torch.float32)
    for h in range(H):
        ops.linear(q[:, 64 * h: 64 * h + 64], kt[h], out=qt[:, h, :])
    return qt


def _fold_path(ops, d, Bc, t, E):
    """(o, u) of the folded chain: the head-batched qt | c product, the op, the head-batched o product."""
    H = E // 64
    x, stats, w, b = (torch.from_numpy(d[n]).cuda() for n in ("x", "stats", "w", "b"))
    u = ops.attention_prefix_fold(x, stats, _fold_qt(ops, d, Bc, t, E), Bc, t, E, H, eps=EPS, scale=SCALE)
    o = torch.empty((Bc, E), device="cuda", dtype=torch.float32)
    for h in range(H):
        ops.linear(u[:, h * E: (h + 1) * E], w[E + 64 * h: E + 64 * h + 64], bias=b[E + 64 * h: E + 64 * h + 64],
                   out=o[:, 64 * h: 64 * h + 64])
    return o, u


def _errors(got, want):
    e = got.double().cpu().numpy() - want
    return float(np.abs(e).max()), float(np.sqrt((e ** 2).mean()))


def _check_2x(ops, d, Bc, t, E, what=""):
    """The rule of this module: o of the folded chain may be at most 2 x as far from fp64 as o of the path it replaces, in max and in
    rms, on the same operands d.  Prints the figures first; returns (o, u) of the folded chain."""
    old_max, old_rms = _errors(_existing_path(ops, d, Bc, t, E), d["o"])
    o, u = _fold_path(ops, d, Bc, t, E)
    new_max, new_rms = _errors(o, d["o"])
    u_max, u_rms = _errors(u, d["u"])
    print("%sBc=%d t=%d E=%d: o against fp64 max / rms  existing %.3g / %.3g  fold %.3g / %.3g   (u of the op alone: %.3g / %.3g)"
          % (what and what + " ", Bc, t, E, old_max, old_rms, new_max, new_rms, u_max, u_rms))
    assert old_max > 0 and old_rms > 0
    assert new_max <= 2 * old_max, (new_max, old_max)
    assert new_rms <= 2 * old_rms, (new_rms, old_rms)
    return o, u


@pytest.mark.parametrize("Bc,t,E", SHAPES)
def test_fold_against_fp64_is_as_close_as_the_path_it_replaces(hip_lib, Bc, t, E):
    from faceformer_amd.hip import ops
    _check_2x(ops, _operands(Bc, t, E), Bc, t, E)


# The launch code of ff_attention_prefix_fold (ff_attention_fold.hip), quoted: a block keeps small = ((2 + H) t + H + 3) & ~3 floats of
# statistics and scores, at most FOLD_MAX_SMALL_FLOATS of them (else FF_ERR_ARG), and stages the normalised rows beside them when
# (small + t E) * 4 <= FOLD_MAX_LDS_BYTES (else the u pass re-forms them from x).  A change of either constant fails the derived
# values below.
FOLD_MAX_SMALL_FLOATS = 12000
FOLD_MAX_LDS_BYTES = 150 * 1024


def _small_floats(t, E):
    return ((2 + E // 64) * t + E // 64 + 3) & ~3


def _staged(t, E):
    return (_small_floats(t, E) + t * E) * 4 <= FOLD_MAX_LDS_BYTES


def _largest_t(E):
    t = 1
    while _small_floats(t + 1, E) <= FOLD_MAX_SMALL_FLOATS:
        t += 1
    return t


# The widths between the tested 128, 256 and 512: the thread groups of the u pass, 512 // (E / 4) = 10, 6, 5, 4, are no power of two
# and leave idle threads behind the last group, a group has 1 head (192, 320) or 2 (384, 448; at 448 the last group has one), lanes
# 64 .. E / 4 - 1 alone have a second 16-byte column, and the statistics merge runs over 6, 10, 12 and 14 segments.
WIDTH_SHAPES = [(3, 5, 192, True), (2, 9, 320, True), (4, 7, 384, True), (3, 6, 448, True),
                (1, 210, 192, False), (1, 130, 320, False), (1, 110, 384, False), (1, 90, 448, False)]


@pytest.mark.parametrize("Bc,t,E,staged", WIDTH_SHAPES)
def test_fold_at_the_widths_between_128_256_and_512(hip_lib, Bc, t, E, staged):
    """The existing-path arm is ops.linear_ln as at the other widths: ff_gemm_f32_ln takes every K % 64 == 0, 128 <= K <= 512."""
    from faceformer_amd.hip import ops
    assert _staged(t, E) == staged and _small_floats(t, E) <= FOLD_MAX_SMALL_FLOATS
    _check_2x(ops, _operands(Bc, t, E), Bc, t, E, "staged" if staged else "unstaged")


def test_fold_on_both_sides_of_the_staging_boundary(hip_lib):
    """E = 512: (((10 t + 11) & ~3) + 512 t) * 4 <= 153600 holds up to t = 73."""
    from faceformer_amd.hip import ops
    E = 512
    last = max(t for t in range(1, 200) if _staged(t, E))
    assert last == 73 and not _staged(last + 1, E)
    for t in (last, last + 1):
        _check_2x(ops, _operands(2, t, E), 2, t, E, "staged" if _staged(t, E) else "unstaged")


@pytest.mark.parametrize("E,limit", [(512, 1199), (128, 2999)])
def test_fold_takes_the_largest_t_and_refuses_the_next(hip_lib, E, limit):
    """((2 + H) t + H + 3) & ~3 <= 12000: t = 1199 at E = 512 and t = 2999 at E = 128 are the last the op accepts."""
    from faceformer_amd.hip import ops
    t = _largest_t(E)
    assert t == limit and not _staged(t, E)
    _check_2x(ops, _operands(1, t, E), 1, t, E, "largest t")
    p = torch.zeros(4096, device="cuda", dtype=torch.float32).data_ptr()    # (refused before anything is launched)
    assert hip_lib.ff_attention_prefix_fold(p, p, EPS, p, SCALE, 1, t + 1, E, E // 64, p, None) == -1           # FF_ERR_ARG
    assert b"ff_attention_prefix_fold" in hip_lib.ff_last_error()


SHARP_ALPHA = 100.0
SHARP_SHAPES = [(5, 3, 128), (3, 33, 512), (2, 80, 512)]
_SHARP = {}


def _sharp(Bc, t, E):
    """The operands of _operands with q of every (sequence, head) = SHARP_ALPHA k64[j*] / |k64[j*]|, k64 the fp64 key of a drawn
    position j*.  Fixture conditions (fp64, here): the largest scaled score of every (sequence, head) is at least 100 -- expf
    overflows past 88.7, so a softmax pass without the max subtraction gives inf / inf -- and the top-2 gap is at least 20, so the
    weights are one-hot to 2e-9: well conditioned, both chains reduce to the projection of one row."""
    key = (Bc, t, E)
    if key not in _SHARP:
        H = E // 64
        d = {n: _operands(Bc, t, E)[n] for n in ("x", "stats", "w", "b", "pos")}
        k = _keys_fp64(d, Bc, t, E)[1][:, :E].reshape(t, Bc, H, 64)
        jstar = np.random.default_rng(7 * E + t + Bc).integers(0, t, size=(Bc, H))
        ks = k[jstar, np.arange(Bc)[:, None], np.arange(H)[None, :]]
        d["q"] = (SHARP_ALPHA * ks / np.linalg.norm(ks, axis=2, keepdims=True)).reshape(Bc, E).astype(np.float32)
        d = _with_fp64(d, Bc, t, E)
        top = np.sort(d["scores"], axis=2)
        assert top[:, :, -1].min() >= 100.0, top[:, :, -1].min()
        assert (top[:, :, -1] - top[:, :, -2]).min() >= 20.0, (top[:, :, -1] - top[:, :, -2]).min()
        print("sharp fixture Bc=%d t=%d E=%d: top score %.1f .. %.1f, smallest top-2 gap %.1f"
              % (Bc, t, E, top[:, :, -1].min(), top[:, :, -1].max(), (top[:, :, -1] - top[:, :, -2]).min()))
        _SHARP[key] = d
    return _SHARP[key]


@pytest.mark.parametrize("Bc,t,E", SHARP_SHAPES)
def test_fold_with_scores_past_the_range_of_expf(hip_lib, Bc, t, E):
    from faceformer_amd.hip import ops
    d = _sharp(Bc, t, E)
    o, u = _fold_path(ops, d, Bc, t, E)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(o).all())
    _check_2x(ops, d, Bc, t, E, "sharp")


_DEGENERATE = {}


def _degenerate():
    """The (7, 5, 256) operands with three rows replaced, their statistics rebuilt in fp64 as _operands does: row 3 constant (M2 = 0
    in every segment: rstd = 1 / sqrt(eps), x^ = 0), row 16 unit values with one element of 1e4, row 33 segments of spread 1 whose
    means differ by 1e3."""
    if not _DEGENERATE:
        Bc, t, E = 7, 5, 256
        d = {n: _operands(Bc, t, E)[n].copy() for n in ("x", "stats", "w", "b", "pos", "q")}
        rng = np.random.default_rng(2300)
        x = d["x"]
        x[3] = 0.75
        x[16] = rng.standard_normal(E)
        x[16, 101] = 1e4
        x[33] = rng.standard_normal(E) + np.repeat(1e3 * rng.standard_normal(E // 32), 32)
        seg = x.astype(np.float64).reshape(-1, E // 32, 32)
        mean = seg.mean(axis=2)
        d["stats"] = np.stack([mean, ((seg - mean[:, :, None]) ** 2).sum(axis=2)], axis=2).astype(np.float32)
        assert (d["stats"][3, :, 1] == 0).all() and np.ptp(d["stats"][33, :, 0]) > 1e3
        _DEGENERATE.update(_with_fp64(d, Bc, t, E))
    return _DEGENERATE


def test_fold_with_degenerate_rows(hip_lib):
    from faceformer_amd.hip import ops
    o, u = _check_2x(ops, _degenerate(), 7, 5, 256, "degenerate rows")
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(o).all())


@pytest.mark.parametrize("Bc,t,E", [(7, 5, 256), (3, 33, 512)])
def test_fold_of_a_sequence_does_not_depend_on_the_others(hip_lib, Bc, t, E):
    """The summation order is fixed (the kernel's header), so these are exact: two launches give equal bits, and sequence b alone
    -- Bc = 1, its rows j * Bc + b and their statistics gathered contiguously, its qt | c rows -- gives the bits of its rows of
    the batched u."""
    from faceformer_amd.hip import ops
    d = _operands(Bc, t, E)
    H = E // 64
    x, stats = torch.from_numpy(d["x"]).cuda(), torch.from_numpy(d["stats"]).cuda()
    qt = _fold_qt(ops, d, Bc, t, E)
    u = ops.attention_prefix_fold(x, stats, qt, Bc, t, E, H, eps=EPS, scale=SCALE)
    RZ.assert_same_bits(ops.attention_prefix_fold(x, stats, qt, Bc, t, E, H, eps=EPS, scale=SCALE), u, "two launches")
    for b in range(Bc):
        alone = ops.attention_prefix_fold(x[b::Bc].contiguous(), stats[b::Bc].contiguous(), qt[b:b + 1].contiguous(), 1, t, E, H,
                                          eps=EPS, scale=SCALE)
        RZ.assert_same_bits(alone, u[b:b + 1], "sequence %d alone / in the batch of %d" % (b, Bc))


def test_fold_rejects_what_it_does_not_support(hip_lib):
    from faceformer_amd.hip import lib as L
    FF_ERR_ARG = -1
    t = torch.zeros(4096, device="cuda", dtype=torch.float32)
    p = t.data_ptr()

    def call(E, H, Bc=1, steps=2, x=p, stats=p, qt=p, u=p, eps=EPS):
        return hip_lib.ff_attention_prefix_fold(x, stats, eps, qt, SCALE, Bc, steps, E, H, u, None)
    for E, H in ((64, 1), (96, 1), (160, 2), (576, 9), (1024, 16), (512, 4), (128, 8)):
        assert call(E, H) == FF_ERR_ARG, (E, H)
        assert b"ff_attention_prefix_fold" in hip_lib.ff_last_error()
    assert call(128, 2, steps=0) == FF_ERR_ARG
    assert call(128, 2, Bc=-1) == FF_ERR_ARG
    assert call(512, 8, steps=1 << 20) == FF_ERR_ARG                      # more scores than a block keeps
    assert call(128, 2, eps=-1.0) == FF_ERR_ARG
    for null in ("x", "stats", "qt", "u"):
        assert call(128, 2, **{null: None}) == FF_ERR_ARG, null
    assert call(128, 2, x=p + 4) == FF_ERR_ARG                            # 16-byte alignment of the rows
    assert call(128, 2, Bc=0) == 0                                        # an empty launch is a no-op, not an error
    torch.cuda.synchronize()
    assert L.FF_HEAD_DIM == 64


@pytest.mark.parametrize("Bc,t,E", [(5, 3, 128), (3, 33, 512)])
def test_fold_stays_inside_its_operands(hip_lib, Bc, t, E):
    """The operands lie in buffers whose every other byte is a fill: rows >= t * Bc of x and of the statistics are that fill
    (NaN as fp32 under POISON), as is everything around qt and u.  Equal bits under both fills: nothing outside was read; the
    fill intact after the launch: nothing outside u was written."""
    from faceformer_amd.hip import ops
    d = _operands(Bc, t, E)
    H = E // 64
    qt_cpu = _fold_qt(ops, d, Bc, t, E).cpu()
    got = {}
    for fill in (RZ.ZERO, RZ.POISON):
        g = RZ.Guard(fill)
        x = g.embed(torch.from_numpy(d["x"]), name="x")
        stats = g.embed(torch.from_numpy(d["stats"]), name="stats")
        qt = g.embed(qt_cpu, name="qt")
        u = g.embed(torch.full((Bc, H * E), float("nan")), name="u")
        ops.attention_prefix_fold(x, stats, qt, Bc, t, E, H, eps=EPS, scale=SCALE, out=u)
        g.check()
        assert not bool(torch.isnan(u).any())
        got[fill] = u.clone()
    RZ.assert_same_bits(got[RZ.ZERO], got[RZ.POISON], "ff_attention_prefix_fold under ZERO / POISON surroundings")
    RZ.assert_same_bits(got[RZ.ZERO], _fold_path(ops, d, Bc, t, E)[1], "ff_attention_prefix_fold embedded / plain")


# ---- 3: the engine with the fold at every step ----------------------------------------------------------------------------------------
@contextlib.contextmanager
def _knobs(**kw):
    from faceformer_amd.hip import ops
    try:
        for k, v in kw.items():
            ops.set_tuning(k, v)
        yield
    finally:
        ops.reset_tuning()


_MODELS = {}


def _model(name):
    """The golden with its model on the f32 matrix cores only (x3_min_rows = 0): no step takes the split products."""
    if name not in _MODELS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        model = build_model(case, sd, "cuda")
        model.x3_min_rows = 0
        _MODELS[name] = (case, z, model, batch_to(batch, "cuda"))
    return _MODELS[name]


def _profiled(hip_lib, call):
    ms, work, cnt = (ctypes.c_double * 7)(), (ctypes.c_double * 7)(), (ctypes.c_longlong * 7)()
    torch.cuda.synchronize()
    hip_lib.ff_profile_begin()
    out = call()
    assert hip_lib.ff_profile_end(ms, work, cnt, 7) == 0
    return out, [int(c) for c in cnt]


def _same_bits(a, b, what):
    assert a["steps"] == b["steps"], what
    for k in ("predict", "logits"):
        RZ.assert_same_bits(a[k], b[k], "%s: %s" % (what, k))


@pytest.mark.parametrize("name", ["par_small_ragged", "par_full_n40_gain4", "seq_full_A4_gain4"])
def test_engine_with_the_fold_at_every_step_meets_the_golden(hip_lib, name):
    from test_parity_golden import check_frozen_bar, compare_with_golden, run_traced
    case, z, model, b = _model(name)
    run = lambda: run_traced(model, case, b)
    run()       # (the first decode of a model also makes its derived weights: not among the launches counted below)
    # FF_LAST_QKV_ONE_LAUNCH_ROWS = 0 in both arms: the form the fold replaces is then the two-launch one at every step, and the
    # fold (q, qt | c and o products) is one category-0 launch more per step and micro-batch
    with _knobs(FF_LAST_QKV_ONE_LAUNCH_ROWS=0, **{KNOB: 0}):
        off, cnt_off = _profiled(hip_lib, run)
        _same_bits(run(), off, "%s: two calls without the fold" % name)
    with _knobs(FF_LAST_QKV_ONE_LAUNCH_ROWS=0, **{KNOB: 1}):
        on, cnt_on = _profiled(hip_lib, run)
        _same_bits(run(), on, "%s: two calls with the fold" % name)
    stats = compare_with_golden(case, z, on)
    print(name, "fold at every step", stats)
    check_frozen_bar(name, stats)
    steps = int(z["steps"])
    assert steps >= 3
    more = cnt_on[0] - cnt_off[0]
    print(name, "launches by category without / with the fold", cnt_off, cnt_on)
    assert more > 0 and more % (steps - 1) == 0, (more, steps)          # every step after the first, every micro-batch
    if len(case["n_edges"]) == 1 and case["kind"] == "parallel":
        assert more == steps - 1, (more, steps)                         # one wireframe: one micro-batch
    assert cnt_on[1] == cnt_off[1], (cnt_on, cnt_off)                   # the prefix pass counts where the launch it replaces did
    assert cnt_on[4] == cnt_off[4] + 1, (cnt_on, cnt_off)               # the per-call tables: one row-op launch


def test_engine_with_the_fold_under_retirement(hip_lib):
    """par_small_ragged with FF_RETIRE_FINISHED: the live widths shrink between steps, the fold follows them.  The rule of
    tests/test_retire_finished.py: tokens equal at decisive margins up to every sequence's last kept position, zero behind it,
    logits within the step tolerance."""
    from test_parity_golden import _tol
    from test_retire_finished import _decode
    name = "par_small_ragged"
    case, z, model, b = _model(name)
    TOK = token_ns()
    with _knobs(**{KNOB: 1}):
        out = _decode(model, b, True, trace=True)
        _same_bits(_decode(model, b, True, trace=True), out, "two retiring calls with the fold")
    T = case["model"]["seq_len"]
    want, s_r = faces.retired_view(z["predict"], TOK, return_steps=True)
    pred, want, gold = out["predict"].cpu().numpy().reshape(-1, T), want.reshape(-1, T), z["predict"].reshape(-1, T)
    assert out["steps"] == s_r
    term = (gold >= 1) & (gold < 4)
    last = np.minimum(np.where(term.any(axis=1), term.argmax(axis=1), T), s_r)
    assert np.array_equal(pred[:, 0], want[:, 0])
    assert (pred[np.arange(T)[None, :] > last[:, None]] == 0).all()
    alive = np.ones(pred.shape[0], dtype=bool)
    logits = out["logits"].cpu().numpy()
    for s in range(s_r):
        tol = _tol(z["logits"][s])
        kept = s + 1 <= last
        same = pred[:, s + 1] == want[:, s + 1]
        must = alive & kept & (z["margin"][s] > 2 * tol)
        assert same[must].all(), (s, np.where(must & ~same)[0][:8])
        alive &= same | ~kept
        for ri, row in enumerate(z["logit_rows"]):
            if kept[row] and alive[row]:
                dlt = np.abs(logits[s, row] - z["logits"][s, ri]).max()
                assert dlt <= tol, (s, int(row), dlt, tol)


def test_engine_with_the_fold_on_two_streams_repeats_its_bits(hip_lib):
    """Two wireframes, each its own micro-batch, on two streams: the result does not depend on the stream or the launch."""
    from test_parity_golden import compare_with_golden, run_traced
    name = "par_small_ragged"
    case, z, model, b = _model(name)
    assert len(case["n_edges"]) >= 2
    old = model.chunk_wireframes, model.num_streams
    try:
        with _knobs(**{KNOB: 1}):
            model.chunk_wireframes, model.num_streams = 1, 1
            one = run_traced(model, case, b)
            model.num_streams = 2
            two = run_traced(model, case, b)
            _same_bits(run_traced(model, case, b), two, "two calls on two streams")
            _same_bits(two, one, "two streams / one stream")
        compare_with_golden(case, z, two)
    finally:
        model.chunk_wireframes, model.num_streams = old


# ---- 3b: the per-step rule across its boundaries --------------------------------------------------------------------------------------
# decoder_pass (ff_engine.hip), quoted:   R = t * Bc, Bc the micro-batch's width;
#   fold_last = last && t > 1 && fold_kt && R >= knob && !step_splits(m, prm, R) &&
#               align4(Bc * H * (E + t)) + Bc * H * E <= (T - 1) * Bc * FF              (qt | c and u inside the feed-forward scratch h)
ONE = "FF_LAST_QKV_ONE_LAUNCH_ROWS"      # 0 in every arm, as above: the unfolded steps are then the two-launch form in both


@contextlib.contextmanager
def _one_wireframe_chunks(model):
    """Every wireframe its own micro-batch: the widths are then the wireframes' compact widths (_widths)."""
    old = model.chunk_wireframes
    model.chunk_wireframes = 1
    try:
        yield
    finally:
        model.chunk_wireframes = old


def _enqueued(out):
    """The positions t = step + 1 whose step the call enqueued, from its own report."""
    return [s + 1 for s, v in enumerate(out["slots_per_step"]) if v > 0]


def _widths(b, out):
    """The micro-batch widths of a decode with one wireframe per micro-batch: a wireframe decodes its num_input anchors and, with
    fewer than F of them, ONE padding-anchor sequence (Chunk, ff_engine.hip) -- held against the widths the decode reports."""
    ni = [int(n) for n in b["num_input"]]
    w = [n + 1 if n < max(ni) else n for n in ni]
    assert all(v == sum(w) for v in out["slots_per_step"][: out["steps"]]), (w, out["slots_per_step"])
    return w


def _golden_rule(name, case, z, out, what):
    from test_parity_golden import check_frozen_bar, compare_with_golden
    stats = compare_with_golden(case, z, out)
    print(name, what, stats)
    check_frozen_bar(name, stats)


def _fold_increment(hip_lib, run, widths):
    """(launch counts of the knob-0 run, that run, category-0 launches one folding (step, micro-batch) pair adds, the positions
    t >= 2 of the call): knob 1 against knob 0, every pair folding."""
    with _knobs(**{ONE: 0, KNOB: 0}):
        off, cnt_off = _profiled(hip_lib, run)
    with _knobs(**{ONE: 0, KNOB: 1}):
        on, cnt_on = _profiled(hip_lib, run)
    ts = [t for t in _enqueued(off) if t >= 2]
    assert _enqueued(on) == _enqueued(off) and len(ts) >= 3
    more = cnt_on[0] - cnt_off[0]
    assert more > 0 and more % (len(ts) * len(widths)) == 0, (cnt_off, cnt_on, ts, widths)
    return cnt_off, off, more // (len(ts) * len(widths)), ts


@pytest.mark.parametrize("name", ["par_full_n40_gain4", "par_small_ragged"])
def test_engine_crossing_the_threshold_inside_a_call(hip_lib, name):
    """The knob at t0 * Bc of a middle step t0 of one micro-batch: the steps before it take the two-launch form, the steps from it on
    fold.  The result meets the golden; the category-0 launches over the knob-0 run are the folding (step, micro-batch) pairs
    t >= 2, t * Bc >= knob, times what one pair adds; with the knob one higher the pair on the boundary no longer folds."""
    from test_parity_golden import run_traced
    case, z, model, b = _model(name)
    run = lambda: run_traced(model, case, b)
    with _one_wireframe_chunks(model):
        run()
        with _knobs(**{ONE: 0, KNOB: 0}):
            widths = _widths(b, run())
        cnt_off, off, per, ts = _fold_increment(hip_lib, run, widths)
        t0 = ts[len(ts) // 2]
        knob = t0 * sorted(widths)[-2:][0]                  # (the second widest micro-batch, where there are several)
        pairs = lambda kn: sum(1 for t in ts for w in widths if t * w >= kn)
        on_boundary = sum(1 for w in widths if t0 * w == knob)
        assert on_boundary == sum(1 for t in ts for w in widths if t * w == knob) >= 1
        assert 0 < pairs(knob + 1) == pairs(knob) - on_boundary < pairs(knob) < pairs(1) == len(ts) * len(widths)
        for kn in (knob, knob + 1):
            with _knobs(**{ONE: 0, KNOB: kn}):
                out, cnt = _profiled(hip_lib, run)
                _same_bits(run(), out, "%s: two calls with the knob at %d" % (name, kn))
            _golden_rule(name, case, z, out, "knob %d (t0 = %d, widths %s)" % (kn, t0, widths))
            print(name, "knob", kn, "folding pairs", pairs(kn), "of", pairs(1), "launches", cnt_off, cnt, "per pair", per)
            assert cnt[0] - cnt_off[0] == per * pairs(kn), (kn, cnt, cnt_off, per, pairs(kn))
            assert cnt[1] == cnt_off[1] and cnt[4] == cnt_off[4] + 1, (cnt, cnt_off)


_SPLIT_MODEL = {}


def test_engine_folds_the_steps_that_do_not_split(hip_lib):
    """par_full_n40_gain4 (one micro-batch of 40 sequences, 11 steps) with the package split kind bound from x3_min_rows = 7 * 40
    rows on (the middle one of the steps t = 2 .. 11) and the fold at every step.  step_splits (ff_engine.hip): the split planes
    bound and x3_wins(R, N = 3E, K = E) -- for N >= 1536 that is R >= x3_min_rows (K % 32 == 0, the operand below 2^30 floats) --
    so the steps t = 7 .. 11 split and the steps t = 2 .. 6 are left to the f32 family: those five fold."""
    from test_parity_golden import run_traced
    name = "par_full_n40_gain4"
    case, z, f32_model, b = _model(name)
    f32_run = lambda: run_traced(f32_model, case, b)
    f32_run()
    with _knobs(**{ONE: 0, KNOB: 0}):
        widths = _widths(b, f32_run())
    assert len(widths) == 1 and 3 * case["model"]["E"] >= 1536
    per, ts = _fold_increment(hip_lib, f32_run, widths)[2:]
    t0 = ts[len(ts) // 2]
    if name not in _SPLIT_MODEL:
        sd, _ = case_weights_and_batch(case)
        _SPLIT_MODEL[name] = build_model(case, sd, "cuda")
        _SPLIT_MODEL[name].x3_min_rows = t0 * widths[0]
    model = _SPLIT_MODEL[name]
    run = lambda: run_traced(model, case, b)
    run()
    assert model.engine().has_planes
    with _knobs(**{ONE: 0, KNOB: 0}):
        off, cnt_off = _profiled(hip_lib, run)
    with _knobs(**{ONE: 0, KNOB: 1}):
        on, cnt_on = _profiled(hip_lib, run)
        _same_bits(run(), on, "two calls")
    folding = [t for t in ts if t * widths[0] < model.x3_min_rows]
    assert (t0, folding, ts[-1]) == (7, [2, 3, 4, 5, 6], 11)
    _golden_rule(name, case, z, on, "split from %d rows on, the fold below" % model.x3_min_rows)
    print(name, "launches by category without / with the fold", cnt_off, cnt_on)
    assert cnt_on[6] == cnt_off[6] > 0, (cnt_on, cnt_off)
    assert cnt_on[0] - cnt_off[0] == per * len(folding), (cnt_on, cnt_off, per)
    assert cnt_on[1] == cnt_off[1] and cnt_on[4] == cnt_off[4] + 1, (cnt_on, cnt_off)


@pytest.mark.parametrize("name", ["par_small_ragged", "par_full_n40_gain4"])
def test_short_decodes_on_both_sides_of_the_scratch_guard(hip_lib, name):
    """Decodes with T' < seq_len (greedy decoding is causal: the reference is the golden's own first T' - 1 steps).  The guard's
    last term, per sequence: H (2E + t) <= (T' - 1) FF.  (The padding of align4 is 0 or 2 floats -- H is even -- and both sides are
    even, so the padding never decides and the term is the same for every micro-batch width.)  It depends on T' far more than on
    t: at the first T' that passes it, EVERY step t >= 2 of the call folds, not the last alone.  Three T': the largest at which no
    step folds (no folding launch, though the tables are laid out and made), the next, and one a few steps longer -- with the
    launches of exactly the folding steps, equal results on ZERO and POISON workspaces, and kt [H, E + T', 64] with another T' than
    the position table has rows."""
    import test_mode_forms as MF
    import test_workspace_poison as WP
    from test_parity_golden import run_traced
    m = MF._bound(name, "f32")
    mm, z = m.case["model"], m.z
    E, H, FF, steps = mm["E"], mm["H"], mm["FF"], int(z["steps"])
    folds = lambda t, Tp: H * (2 * E + t) <= (Tp - 1) * FF
    full = lambda: run_traced(m.model, m.case, m.b)
    full()
    with _knobs(**{ONE: 0, KNOB: 0}):
        _, c0 = _profiled(hip_lib, full)
    with _knobs(**{ONE: 0, KNOB: 1}):
        on, c1 = _profiled(hip_lib, full)
    ts = [t for t in _enqueued(on) if t >= 2]
    assert all(folds(t, m.T) for t in ts) and (c1[0] - c0[0]) % len(ts) == 0
    inc = (c1[0] - c0[0]) // len(ts)                          # what one folding step adds, over its micro-batches
    assert inc > 0
    none = max(Tp for Tp in range(3, steps + 2) if not any(folds(t, Tp) for t in range(2, Tp)))
    assert (name, none) in (("par_small_ragged", 3), ("par_full_n40_gain4", 9)) and none + 1 < m.T
    for Tp in (none, none + 1, min(none + 3, m.T - 1)):
        case = dict(m.case, model=dict(mm, seq_len=Tp))
        zt = {k: z[k] for k in ("logit_rows", "memory", "memory_head") if k in z}
        zt.update(steps=Tp - 1, predict=z["predict"].reshape(-1, m.T)[:, :Tp], margin=z["margin"][: Tp - 1], logits=z["logits"][: Tp - 1])
        call = lambda: run_traced(m.model, case, m.b)
        with _knobs(**{ONE: 0, KNOB: 0}):
            off, cnt_off = _profiled(hip_lib, call)
        with _knobs(**{ONE: 0, KNOB: 1}):
            out, cnt = _profiled(hip_lib, call)
            zero, _ = WP._run([m], call, fill=RZ.ZERO, what="%s T'=%d ZERO" % (name, Tp))
            poison, _ = WP._run([m], call, fill=RZ.POISON, what="%s T'=%d POISON" % (name, Tp))
        WP._assert_equal(poison, zero, "%s T'=%d" % (name, Tp))
        WP._assert_equal(out, zero, "%s T'=%d" % (name, Tp))
        WP._assert_no_nan(poison, "%s T'=%d" % (name, Tp))
        folding = [t for t in _enqueued(out) if t >= 2 and folds(t, Tp)]
        assert _enqueued(out) == list(range(1, Tp)) and folding == ([] if Tp == none else list(range(2, Tp)))
        print(name, "T' = %d: folding steps %s, launches by category without / with the knob" % (Tp, folding), cnt_off, cnt)
        assert cnt[0] - cnt_off[0] == inc * len(folding), (Tp, cnt, cnt_off, inc)
        assert cnt[1] == cnt_off[1] and cnt[4] == cnt_off[4] + 1, (Tp, cnt, cnt_off)
        _golden_rule(name, case, zt, poison, "T' = %d" % Tp)
        if not folding:
            _same_bits(out, off, "%s T'=%d: no step folds" % (name, Tp))


# ---- 4: the workspace -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["par_small_ragged", "par_full_n40_gain4"])
def test_workspace_grows_by_the_tables_and_may_hold_anything(hip_lib, name):
    import test_mode_forms as MF
    import test_workspace_poison as WP
    m = MF._bound(name, "f32")
    call = lambda: WP._plain(m)
    mm = m.case["model"]
    E, T = mm["E"], mm["seq_len"]
    table = -(-4 * ((E // 64) * (E + T) * 64 + E) // 256) * 256          # kt [H, E + T, 64] | ob [E], one 256-byte aligned block
    with _knobs(**{KNOB: 0}):
        _, d0 = WP._run([m], call, fill=RZ.ZERO, what="%s without the fold" % name)
    with _knobs(**{KNOB: 1}):
        zero, d1 = WP._run([m], call, fill=RZ.ZERO, what="%s ZERO" % name)
        poison, _ = WP._run([m], call, fill=RZ.POISON, what="%s POISON" % name)
    WP._assert_equal(poison, zero, name)
    WP._assert_no_nan(poison, name)
    n0, n1 = [n for _, n in d0.taken], [n for _, n in d1.taken]
    assert len(n0) == len(n1) and n0[:-1] == n1[:-1], (n0, n1)          # the encoder's requests are what they were
    assert n1[-1] - n0[-1] == table, (n0, n1, table)                    # the decode's: exactly the tables more


@pytest.mark.parametrize("name", ["par_small_ragged", "par_full_n40_gain4"])
def test_workspace_holds_the_tables_up_to_the_rows_of_the_longest_step(hip_lib, name):
    """layout_decode (ff_engine.hip) lays the tables out when Rmax = (T - 1) * widest micro-batch >= knob: with the knob at Rmax the
    size query gives the knob-1 size, one higher the knob-0 size.  The width comes from a decode's report."""
    import test_mode_forms as MF
    import test_workspace_poison as WP
    m = MF._bound(name, "f32")
    with _one_wireframe_chunks(m.model):
        with _knobs(**{KNOB: 0}):
            rmax = (m.T - 1) * max(_widths(m.b, WP._plain(m)))
            n0 = MF._workspace_bytes(m)
        sizes = {}
        for kn in (1, rmax, rmax + 1):
            with _knobs(**{KNOB: kn}):
                sizes[kn] = MF._workspace_bytes(m)
    print(name, "Rmax", rmax, "workspace bytes: knob 0", n0, sizes)
    assert sizes[1] > n0 and sizes[rmax] == sizes[1] and sizes[rmax + 1] == n0, (n0, sizes)
