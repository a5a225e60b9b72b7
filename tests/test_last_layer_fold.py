"""GPU: the pruned last decoder layer with k | v folded into the query (knob FF_LAST_FOLD_MIN_ROWS).

  1  the op ff_attention_prefix_fold inside its chain -- qt | c = q_h [W'k_h | kb_h], the op, o_h = u_h W'v_h^T + b'v_h -- against
     fp64 numpy on the same operands, set against the path it replaces (ff_gemm_f32_ln k | v, then ff_attention with nq = 1) on
     the same operands: both are fp32 chains of the same length that differ in association only, so the fold may take at most
     2 x the existing path's max and rms error
  2  the op under poisoned surroundings (tests/redzone.py): nothing outside u is written, nothing outside the t * Bc rows is read
  3  the engine with the fold at EVERY step (FF_LAST_FOLD_MIN_ROWS=1) under the rule of tests/test_parity_golden.py, with the
     profiled launch counts as evidence that the form ran, and bit-equal repeats
  4  the workspace: the size query grows by exactly the per-call tables, and a decode on a poisoned workspace equals a clean one
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
    # fp64 on the same operands: the merged statistics, x^, k | v, the attention of the newest rows
    s64 = stats.astype(np.float64)
    mu = s64[:, :, 0].mean(axis=1)
    var = (s64[:, :, 1].sum(axis=1) + 32.0 * ((s64[:, :, 0] - mu[:, None]) ** 2).sum(axis=1)) / E
    xh = (x.astype(np.float64) - mu[:, None]) / np.sqrt(var + EPS)[:, None]
    kv = xh @ w.astype(np.float64).T + b.astype(np.float64)
    kv[:, :E] += np.repeat(pos.astype(np.float64), Bc, axis=0)
    k = kv[:, :E].reshape(t, Bc, H, 64)
    v = kv[:, E:].reshape(t, Bc, H, 64)
    sc = SCALE * np.einsum("bhd,jbhd->bhj", q.astype(np.float64).reshape(Bc, H, 64), k)
    p = np.exp(sc - sc.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    o = np.einsum("bhj,jbhd->bhd", p, v).reshape(Bc, E)
    u = np.einsum("bhj,jbe->bhe", p, xh.reshape(t, Bc, E)).reshape(Bc, H * E)
    _OPERANDS[key] = dict(x=x, stats=stats, w=w, b=b, pos=pos, q=q, o=o, u=u)
    return _OPERANDS[key]


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


@pytest.mark.parametrize("Bc,t,E", SHAPES)
def test_fold_against_fp64_is_as_close_as_the_path_it_replaces(hip_lib, Bc, t, E):
    from faceformer_amd.hip import ops
    d = _operands(Bc, t, E)
    old_max, old_rms = _errors(_existing_path(ops, d, Bc, t, E), d["o"])
    o, u = _fold_path(ops, d, Bc, t, E)
    new_max, new_rms = _errors(o, d["o"])
    u_max, u_rms = _errors(u, d["u"])
    print("Bc=%d t=%d E=%d: o against fp64 max / rms  existing %.3g / %.3g  fold %.3g / %.3g   (u of the op alone: %.3g / %.3g)"
          % (Bc, t, E, old_max, old_rms, new_max, new_rms, u_max, u_rms))
    assert old_max > 0 and old_rms > 0
    assert new_max <= 2 * old_max, (new_max, old_max)
    assert new_rms <= 2 * old_rms, (new_rms, old_rms)


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
