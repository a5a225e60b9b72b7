"""The five decode modes (greedy with log-probabilities, beam, sampling, loop-constrained, teacher-forced scoring) under every
launch form and split kind of the engine.  The mode tests run the package default only; here each mode's own
checks run over a matrix of engine forms.  No new reference rule: the numpy rules, the replay / layout checks and the fp64
oracle comparisons are the mode tests' own helpers.

Forms (FORMS): model attributes, per-call decode options (all read from the model by the mode tests' _decode / _score) and
tuning knobs (set in-process with ops.set_tuning, back with ops.reset_tuning in a `finally`).
  arithmetic forms   f32, last_fold, fp16x2, fp16x2_f32attn, bf16x3, fp16, no_l0_fold, unfused_ln: checks 1, 2, 3
  scheduling forms   no_pointer_fold, last_qkv_apart, drained, two_streams: checks 1, 2 (drained, two_streams also 4)
f32 and last_fold are the two sides of the pruned last layer's third form on the f32 matrix cores: f32 sets
FF_LAST_FOLD_MIN_ROWS = 0, so that no step of any mode folds k | v into the query however many rows beams and samples make of a
step (left at the package's 2048 rows, some steps of the beam and sampling calls folded and the others did not); last_fold sets it
to 1 with FF_LAST_QKV_ONE_LAUNCH_ROWS = 0, so that every step after the first folds, and is compared with f32_unfolded: f32 with
the same FF_LAST_QKV_ONE_LAUNCH_ROWS, i.e. the two-launch form the fold replaces, at every step.  Under last_fold every mode also
profiles its own traced call against that base (_check_fold_ran): the modes multiply rows and reorder sequences between steps.
The last six run on the package kind with x3_min_rows = 1, with one exception: with the split planes bound from row 1 the
engine folds no LayerNorm at E != 512 (ff_engine.hip, step_fuses: the split kernels fold at K = 512 only), and the fold is
what no_l0_fold, no_pointer_fold, unfused_ln and last_qkv_apart switch.  On par_small_ragged (E = 128) these four keep the
package's x3_min_rows, where every step of the golden folds; on the E = 512 goldens they run from row 1 as listed.
two_streams is not run on par_full_n40_gain4: one wireframe is one micro-batch, which takes one stream.
Every form that binds fp16 planes runs with ops.set_attention_algo(4): the automatic choice takes ff_attention_x2h from 512 query
tiles per launch on, which these goldens do not reach; with it the cross-attention of "fp16x2" and "fp16" is that kernel with
two terms and one, and FF_X2H_ATTN=0 (no planes) is the f32 kernel beside it.

Checks per (mode, form, golden):
  1  self-consistency on the call's own traced logits: the mode's _replay / _check_layout / _check_against_own_trace, with the
     caps the mode tests have (sampling SR.CAP, beam 2 %, constrain none).  Independent of the arithmetic: every form.
  2  equality with faces.retired_view of the greedy decode under the SAME form: W = 1 beam, temperature 0, constrain with both
     bits clear (tokens and stop step exact), forcing the decode along its own tokens (exact wherever the greedy decode's own
     top-2 margin exceeds 2 tol: the forced plan has no padding-anchor de-duplication, so the two calls are two evaluations).
     Log-probabilities within 2 tol(step) + LP_BAR, scores within that summed over the row's steps.
  3  against the fp64 teacher-forced oracle (arithmetic forms): the mode tests' own oracle checks.  tol(step) is
     test_parity_golden._tol for the fp32-class forms and, for "fp16", what test_fp16_decode_against_fp64_truth derives:
     EMU_FACTOR e_emu[s] + FP32_FLOOR scale[s], e_emu measured by the fp64 oracle with _emulated_decoder_layer along the mode's
     own tokens -- never from the HIP output.  The left-out caps of the oracle checks (fixture conditions set at the fp32
     tolerance) are asserted for the fp32-class forms and printed for "fp16".
  4  drained, two_streams: torch.equal with the same call without the knob under the same micro-batch plan, on every output.
Every form asserts that it took effect (test_greedy_with_logprob, _took_effect).

FF_FORM_MARGINS=<file>: every test appends its printed figures there (the table of DESIGN.md 17 is made from it)."""
import contextlib
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

import constrain_ref as CR
import forced_ref as FR
import sample_ref as SR
from conftest import batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces
from faceformer_amd.hip import lib as L

pytestmark = pytest.mark.gpu

TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
LP_BAR = 2.0 ** -16
F64_MIN = np.finfo(np.float64).min
BEAM_W = 4
LOOPS = CR.NO_REPEAT | CR.CONNECT

PAR_GOLDENS = ["par_small_ragged", "par_full_n40_gain4"]
SEQ_GOLDEN = "seq_full_A4_gain4"          # forced and greedy-logprob only

# attrs: model attributes; one_wireframe: every wireframe its own micro-batch; flags_set / flags_clear: bits of decode_flags;
# knobs: the tuning table; base: the form it is compared with (LayerNorm / GEMM launch counts, bit equality); fold: switches a
# LayerNorm fold (see the module docstring: package x3_min_rows at E != 512); attention_algo: ops.set_attention_algo -- 4 sends
# every cross-attention launch that has the fp16 planes of K | V to ff_attention_x2h (the automatic choice takes that kernel
# from 512 query tiles on, which no golden of this module reaches), as test_fp16_decode_against_fp64_truth does
X2H = dict(attention_algo=4)
FORMS = {
    "f32": dict(attrs=dict(x3_min_rows=0), knobs=dict(FF_LAST_FOLD_MIN_ROWS=0)),
    "last_fold": dict(attrs=dict(x3_min_rows=0), knobs=dict(FF_LAST_FOLD_MIN_ROWS=1, FF_LAST_QKV_ONE_LAUNCH_ROWS=0), base="f32_unfolded"),
    "fp16x2": dict(attrs=dict(x3_min_rows=1), **X2H),
    "fp16x2_f32attn": dict(attrs=dict(x3_min_rows=1), knobs=dict(FF_X2H_ATTN=0), base="fp16x2", **X2H),
    "bf16x3": dict(attrs=dict(x3_min_rows=1, split_kind="bf16x3")),
    "fp16": dict(attrs=dict(x3_min_rows=1, split_kind="fp16"), **X2H),
    "no_l0_fold": dict(attrs=dict(x3_min_rows=1), flags_set=L.FF_NO_L0_FOLD, base="fp16x2", fold=True, **X2H),
    "no_pointer_fold": dict(attrs=dict(x3_min_rows=1), one_wireframe=True, flags_set=L.FF_NO_POINTER_FOLD, base="one_wireframe",
                            fold=True, **X2H),
    "unfused_ln": dict(attrs=dict(x3_min_rows=1), flags_clear=L.FF_FUSE_LAYERNORM, base="fp16x2", fold=True, **X2H),
    "last_qkv_apart": dict(attrs=dict(x3_min_rows=1), knobs=dict(FF_LAST_QKV_ONE_LAUNCH_ROWS=0), base="fp16x2", fold=True, **X2H),
    "drained": dict(attrs=dict(x3_min_rows=1), one_wireframe=True, knobs=dict(FF_PINNED_COUNTERS=8), base="one_wireframe", **X2H),
    "two_streams": dict(attrs=dict(x3_min_rows=1, num_streams=2), one_wireframe=True, base="one_wireframe", **X2H),
    "one_wireframe": dict(attrs=dict(x3_min_rows=1), one_wireframe=True, **X2H),   # (no form of the matrix: the base of three)
    "f32_unfolded": dict(attrs=dict(x3_min_rows=0), knobs=dict(FF_LAST_FOLD_MIN_ROWS=0, FF_LAST_QKV_ONE_LAUNCH_ROWS=0)),   # (the base of last_fold)
}
MATRIX_FORMS = [f for f in FORMS if f not in ("one_wireframe", "f32_unfolded")]
ARITHMETIC = ("f32", "last_fold", "fp16x2", "fp16x2_f32attn", "bf16x3", "fp16", "no_l0_fold", "unfused_ln")
BIT_EQUAL = ("drained", "two_streams")
SPLIT_KIND = {"bf16x3": "bf16x3", "fp16": "fp16"}                                # (every other form: the package kind)


def _cases(goldens):
    return [(name, form) for name in goldens for form in MATRIX_FORMS
            if not (form == "two_streams" and len(load_golden(name)[0]["n_edges"]) < 2)]


PAR_CASES = _cases(PAR_GOLDENS)
ALL_CASES = _cases(PAR_GOLDENS + [SEQ_GOLDEN])


# ---- the forms ----------------------------------------------------------------------------------------------------------------------
_GOLDENS, _MODELS = {}, {}


def _golden(name):
    if name not in _GOLDENS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        _GOLDENS[name] = (case, z, sd, batch, batch_to(batch, "cuda"))
    return _GOLDENS[name]


def _attrs(name, form, fold):
    """The model attributes of `form` on golden `name`; fold: the form, or the form this one is the base of, switches a fold."""
    from faceformer_amd.hip.engine import DEFAULT_FLAGS
    from faceformer_amd.models.common import X3_MIN_ROWS_DEFAULT
    case = _golden(name)[0]
    f = FORMS[form]
    attrs = dict(f["attrs"])
    if fold and case["model"]["E"] != 512:
        attrs["x3_min_rows"] = X3_MIN_ROWS_DEFAULT
    if f.get("one_wireframe"):
        attrs["chunk_wireframes"] = 1
        if case["kind"] != "parallel":
            attrs["chunk_max_seqs"] = 1       # (the single-sequence model cuts its micro-batches by sequences)
    attrs["decode_flags"] = (DEFAULT_FLAGS | f.get("flags_set", 0)) & ~f.get("flags_clear", 0)
    return attrs


class Bound:
    """A golden with a model set to one form."""

    def __init__(self, name, form, fold):
        self.name, self.form = name, form
        self.case, self.z, self.sd, self.batch, self.b = _golden(name)
        self.attrs = _attrs(name, form, fold)
        self.model = build_model(self.case, self.sd, "cuda")
        for k, v in self.attrs.items():
            setattr(self.model, k, v)
        self.T = self.case["model"]["seq_len"]
        self.parallel = self.case["kind"] == "parallel"
        self.N = len(self.case["n_edges"])
        self.F = max(int(n) for n in self.case["n_edges"]) if self.parallel else 1
        self.what = "%s %s" % (name, form)


def _bound(name, form, fold=None):
    fold = bool(FORMS[form].get("fold")) if fold is None else fold
    key = (name, form, fold)
    if key not in _MODELS:
        _MODELS[key] = Bound(name, form, fold)
    return _MODELS[key]


def _base(m):
    """The same golden under the form's base: the call without the knob, under the same micro-batch plan."""
    return _bound(m.name, FORMS[m.form]["base"], fold=bool(FORMS[m.form].get("fold")))


@contextlib.contextmanager
def _tuned(form):
    from faceformer_amd.hip import ops
    old = ops.set_attention_algo(FORMS[form].get("attention_algo", 0))
    try:
        for k, v in FORMS[form].get("knobs", {}).items():
            ops.set_tuning(k, v)
        yield
    finally:
        ops.reset_tuning()
        ops.set_attention_algo(old)


@contextlib.contextmanager
def _base_knobs(form):
    """Inside _tuned(form): the tuning table of the form's base, and the form's own back afterwards."""
    from faceformer_amd.hip import ops
    saved = {k: ops.get_tuning(k) for k in FORMS[form].get("knobs", {})}
    ops.reset_tuning()
    try:
        for k, v in FORMS[FORMS[form]["base"]].get("knobs", {}).items():
            ops.set_tuning(k, v)
        yield
    finally:
        ops.reset_tuning()
        for k, v in saved.items():
            ops.set_tuning(k, v)


def _record(line):
    print(line)
    path = os.environ.get("FF_FORM_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- the modes' calls, with the parameters of their own engine tests ----------------------------------------------------------------
def _greedy(m, **kw):
    from test_logprob import _decode
    return _decode(m.model, m.case, m.b, logprob=True, trace=True, num_streams=m.model.num_streams, **kw)


def _beam(m, W, **kw):
    from test_beam import _decode
    return _decode(m.model, m.case, m.b, beam_width=W, term_range=TERM, **kw)


def _sample(m, R, params, seed, **kw):
    from test_sample import _sampled, _uniforms
    u = _uniforms(m.case, m.b, R, seed)
    return _sampled(m.model, m.case, m.b, R, *params, u, **kw), u


def _lattice(name):
    """(lattice batch (CPU), on the GPU, follow table) of constrain_ref: the batch the constrained engine tests decode."""
    from test_constrain import _model
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    return lat, b, table


def _constrain(m, flags, lattice=True, **kw):
    from test_constrain import _constrained, _with_pad
    if not lattice:
        return _constrained(m.model, m.case, m.b, flags, **kw)
    lat, b, table = _lattice(m.name)
    return _with_pad(_constrained(m.model, m.case, b, flags, table, **kw), b)


def _own_paths(m, pred, steps):
    """The lengths up to which a decode's own tokens are forced: the finish position (faces.retired_view's) or the stop step."""
    if m.parallel:
        term = (pred >= TERM[0]) & (pred < TERM[1])
        lengths = np.minimum(np.where(term.any(axis=1), term.argmax(axis=1), m.T), steps)
    else:
        eos = pred == TOK.EOS
        lengths = np.where(eos.any(axis=1), eos.argmax(axis=1), steps)
    return np.minimum(lengths, m.T - 1).astype(np.int64)


def _forced(m, paths, lengths, **kw):
    from test_forced import _score
    return _score(m.model, m.case, m.b, paths, lengths, m.F, **kw)


# ---- tolerances and oracles ---------------------------------------------------------------------------------------------------------
_EMULATED = {}


def _digest(pred, steps):
    return hashlib.sha1(np.ascontiguousarray(pred[:, : steps + 1]).tobytes()).hexdigest()[:16]


def _fp16_tol_along(m, batch, monkeypatch):
    """step_tol of the kind "fp16" (test_fp16_decode_against_fp64_truth's derivation): per step EMU_FACTOR e_emu + FP32_FLOOR scale,
    e_emu = the largest distance over the step's live logits between the fp64 oracle and the same oracle with the contract's
    roundings (_emulated_decoder_layer), both teacher-forced along `pred`."""
    from test_fp16_mode import EMU_FACTOR, FP32_FLOOR, _forced_logits

    def make(pred, steps, truth):
        key = (m.name, id(batch), steps, _digest(pred, steps))
        if key not in _EMULATED:
            emu = _forced_logits(m.case, m.sd, batch, np.ascontiguousarray(pred), steps, True, monkeypatch)
            live = truth > F64_MIN
            scale = np.array([max(1.0, float(np.abs(truth[s][live[s]]).max())) for s in range(steps)])
            e_emu = np.array([float(np.abs(emu[s] - truth[s])[live[s]].max()) for s in range(steps)])
            _EMULATED[key] = EMU_FACTOR * e_emu + FP32_FLOOR * scale
        tol = _EMULATED[key]
        return lambda s, ref: float(tol[s])
    return make


def _step_tol(m, batch, monkeypatch):
    """step_tol for the mode tests' oracle checks: None (their default, _tol) for the fp32-class forms."""
    return _fp16_tol_along(m, batch, monkeypatch) if m.form == "fp16" else None


def _truth(m, pred, steps):
    """fp64 oracle logits [steps, B, S] teacher-forced along `pred` on the golden's own batch."""
    if m.parallel:
        from test_parity_golden import _truth_along
        return _truth_along(m.name, m.case, m.sd, m.batch, dict(predict=np.ascontiguousarray(pred), steps=steps))[0]
    from test_forced import _truth as forced_truth
    return forced_truth("forms:%s:%s" % (m.name, _digest(pred, steps)), m.case, m.sd, m.batch, np.ascontiguousarray(pred), steps,
                        list(range(pred.shape[0])))


def _tol_per_position(m, pred, steps, monkeypatch):
    """[T]: the tolerance of the step that decided position j (0 at position 0 and past the steps), for check 2 -- from the
    golden's stored reference logits, as the default-form tests take it, or (fp16) along the greedy decode's own tokens."""
    from test_parity_golden import _tol
    if m.form == "fp16":
        tol_of = _fp16_tol_along(m, m.batch, monkeypatch)(pred, steps, _truth(m, pred, steps))
        per = [tol_of(s, None) for s in range(steps)]
    else:
        per = [_tol(m.z["logits"][s]) for s in range(min(steps, int(m.z["steps"])))]
    return np.array([0.0] + per + [0.0] * m.T)[: m.T]


def _retired_greedy(m, greedy):
    """(the greedy tokens, their faces.retired_view, its stop step, the log-probabilities of the kept positions, the kept positions
    from 1 on -- the steps a row's score sums)."""
    pred = greedy["predict"].cpu().numpy().reshape(-1, m.T)
    want, steps = faces.retired_view(pred, TOK, return_steps=True)
    keep = faces._retired_keep(pred, TOK)
    kept = keep & (np.arange(m.T)[None, :] >= 1)
    return pred, want.reshape(-1, m.T), steps, greedy["logprob"].cpu().numpy().reshape(-1, m.T).astype(np.float64) * keep, kept


# ---- bit equality and "took effect" -------------------------------------------------------------------------------------------------
def _assert_bit_equal(got, ref, what):
    """Check 4: every output of two calls -- tokens, log-probabilities, scores, finish positions / dead-end flags, traced logits,
    stop step."""
    assert got["steps"] == ref["steps"], what
    assert got.get("step_counts") == ref.get("step_counts"), what
    keys = [k for k, v in ref.items() if torch.is_tensor(v)]
    assert keys and set(keys) == {k for k, v in got.items() if torch.is_tensor(v)}, what
    for k in keys:
        a, c = got[k], ref[k]
        if a.is_floating_point():                      # (rows of a trace no micro-batch ran hold NaN in both)
            assert torch.equal(torch.isnan(a), torch.isnan(c)), (what, k)
            a, c = a.nan_to_num(7.0), c.nan_to_num(7.0)
        assert torch.equal(a, c), (what, k)


def _check_bit_equal(m, call, what):
    """drained / two_streams: `call` under the form (the caller holds the knobs) against the base form without them."""
    if m.form not in BIT_EQUAL:
        return
    from faceformer_amd.hip import ops
    got = call(m)
    saved = {k: ops.get_tuning(k) for k in FORMS[m.form].get("knobs", {})}
    ops.reset_tuning()
    try:
        ref = call(_base(m))
    finally:
        for k, v in saved.items():
            ops.set_tuning(k, v)
    _assert_bit_equal(got, ref, what)


def _launches(fn):
    """(result, launch count per category) of fn(): category 0 f32 GEMMs, 2 LayerNorm, 6 split-product GEMMs (bench.py CAT_NAMES)."""
    lib = L.load()
    ms, work, cnt = (C.c_double * 16)(), (C.c_double * 16)(), (C.c_longlong * 16)()
    torch.cuda.synchronize()
    L.check(lib.ff_profile_begin(), "ff_profile_begin")
    try:
        res = fn()
    finally:
        L.check(lib.ff_profile_end(ms, work, cnt, 16), "ff_profile_end")
    return res, [int(v) for v in cnt]


def _workspace_bytes(m, flags=None):
    """ff_decode_workspace_bytes of the greedy call of `m` (under the knobs set now)."""
    eng = m.model.engine()
    prm = L.DecodeParams()
    prm.variant = L.FF_PARALLEL if m.parallel else L.FF_SEQ2SEQ
    prm.N, prm.L, prm.F, prm.T = m.N, m.case["model"]["L"], m.F, m.T
    prm.chunk_wireframes, prm.chunk_seqs, prm.chunk_max_seqs = m.model.chunk_wireframes, m.model.chunk_seqs, m.model.chunk_max_seqs
    prm.num_streams, prm.ln_fuse_max_rows = m.model.num_streams, m.model.ln_fuse_max_rows
    prm.flags = m.model.decode_flags if flags is None else flags
    prm.x3_min_rows = m.model.x3_min_rows if eng.has_planes else 0
    ni = [int(n) for n in m.case["n_edges"]]
    nbytes = L.load().ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), (C.c_int * m.N)(*ni) if m.parallel else None)
    assert nbytes > 0
    return nbytes


def _took_effect(m, out, cnt):
    """The form's own evidence that the greedy call just profiled (result `out`, launch counts `cnt`) ran what the form names."""
    from faceformer_amd.hip import ops
    from faceformer_amd.models.common import SPLIT_KIND_DEFAULT
    eng = m.model.engine()
    x3 = m.model.x3_min_rows
    assert eng.split_kind == eng.requested_kind == SPLIT_KIND.get(m.form, SPLIT_KIND_DEFAULT), (m.what, eng.split_kind)
    assert eng.has_planes == (x3 > 0) and eng.model.split_kind == (ops.SPLIT_KINDS[eng.split_kind] if x3 > 0 else 0), m.what
    if x3 == 1:
        assert cnt[6] > 0, (m.what, cnt)                       # the split kernels ran
    if x3 == 0:
        assert cnt[6] == 0, (m.what, cnt)
    base = FORMS[m.form].get("base")
    if base is None:
        return
    with _base_knobs(m.form):
        ref, base_cnt = _launches(lambda: _greedy(_base(m)))
        base_ws = _workspace_bytes(_base(m))
    if m.form in ("unfused_ln", "no_l0_fold"):
        assert cnt[2] > base_cnt[2], (m.what, cnt, base_cnt)
    if m.form == "last_fold":
        # every step after the first, every micro-batch: the q, qt | c and o products in place of the k | v and q launches; the
        # per-call tables are one row-op launch and exactly one 256-byte aligned block kt [H, E + T, 64] | ob [E] of the workspace
        ran = _steps_run(out)
        assert ran == _steps_run(ref) >= 3, (m.what, ran)
        more = cnt[0] - base_cnt[0]
        assert more > 0 and more % (ran - 1) == 0, (m.what, cnt, base_cnt, ran)
        assert cnt[4] == base_cnt[4] + 1 and cnt[2] == base_cnt[2], (m.what, cnt, base_cnt)
        E = m.case["model"]["E"]
        assert _workspace_bytes(m) - base_ws == -(-4 * ((E // 64) * (E + m.T) * 64 + E) // 256) * 256, m.what
    if m.form == "last_qkv_apart":                             # k|v and q of the pruned last layer: one more GEMM per step
        assert cnt[0] + cnt[6] > base_cnt[0] + base_cnt[6] and cnt[2] == base_cnt[2], (m.what, cnt, base_cnt)
    if m.form == "fp16x2_f32attn":                             # no fp16 planes of the cross-attention K | V in the workspace,
        assert _workspace_bytes(m) < base_ws, m.what           # and other logits than with them: another cross-attention ran
        assert ops.get_tuning("FF_X2H_ATTN") == 0, m.what
        assert not torch.equal(out["logits"].nan_to_num(7.0), ref["logits"].nan_to_num(7.0)), m.what
    if m.form == "no_pointer_fold":
        # the call without the flag is a one-wireframe plan with the folded head's operands in its workspace
        assert m.model.chunk_wireframes == 1 and _workspace_bytes(m, m.model.decode_flags & ~L.FF_NO_POINTER_FOLD) == base_ws
        assert _workspace_bytes(m) < base_ws, m.what
    if m.form == "drained":                                    # more (step, micro-batch) counters than host-mapped slots
        assert m.model.chunk_wireframes == 1 and m.T * m.N > ops.get_tuning("FF_PINNED_COUNTERS") == 8, m.what
    if m.form == "two_streams":                                # at least two micro-batches: the decode forks
        assert m.model.num_streams == 2 and m.model.chunk_wireframes == 1 and m.N >= 2, m.what


def _steps_run(out):
    """The steps a call enqueued, from its own report (the executed steps and those the stop rule noticed late)."""
    return sum(1 for v in out["slots_per_step"] if v > 0)


def _check_fold_ran(m, call, what):
    """last_fold: `call` (a mode's traced call) profiled under the form and under its base's knobs -- more f32 GEMM launches, the
    tables' row-op launch, as many LayerNorm launches: the fold ran in this mode, not only in the greedy decode."""
    if m.form != "last_fold":
        return
    out, cnt = _launches(lambda: call(m))
    with _base_knobs(m.form):
        ref, base_cnt = _launches(lambda: call(_base(m)))
    # (the same steps in both: the launch counts differ by the form alone; a scoring call reports its steps only)
    assert out["steps"] == ref["steps"] and out.get("slots_per_step") == ref.get("slots_per_step"), (m.what, what)
    _record("launch %-17s %-15s %s: by category without / with the fold %s %s" % (m.name, m.form, what, base_cnt[:7], cnt[:7]))
    assert cnt[0] > base_cnt[0] and cnt[4] == base_cnt[4] + 1 and cnt[2] == base_cnt[2], (m.what, what, cnt, base_cnt)


# ---- greedy with log-probabilities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", ALL_CASES)
def test_greedy_with_logprob(hip_lib, name, form, monkeypatch):
    from test_logprob import _check_against_own_trace, _ref_logprob
    from test_parity_golden import _tol_along
    m = _bound(name, form)
    with _tuned(form):
        out, cnt = _launches(lambda: _greedy(m))
        _took_effect(m, out, cnt)
        worst1 = _check_against_own_trace(out, m.T, what=m.what)                                  # check 1
        _check_bit_equal(m, _greedy, m.what)                                                      # check 4
    line = "greedy %-17s %-15s steps %3d  own trace: max |dlogprob| %.3g" % (name, form, out["steps"], worst1)
    if form in ARITHMETIC:                                                                        # check 3
        pred, steps = out["predict"].cpu().numpy().reshape(-1, m.T), out["steps"]
        lp = out["logprob"].cpu().numpy().reshape(-1, m.T).astype(np.float64)
        truth = _truth(m, pred, steps)
        tol_of = (_step_tol(m, m.batch, monkeypatch) or _tol_along)(pred, steps, truth)
        worst = 0.0
        for s in range(steps):
            bar = 2 * tol_of(s, truth[s]) + LP_BAR
            ref = _ref_logprob(torch.from_numpy(np.where(truth[s] > F64_MIN, truth[s], -np.inf)), torch.from_numpy(pred[:, s + 1]))
            err = float(np.abs(lp[:, s + 1] - ref.numpy()).max())
            worst = max(worst, err / bar)
            assert err <= bar, (m.what, s, err, bar)
        line += "  oracle: worst |dlogprob| / bound %.3f" % worst
    _record(line)


# ---- beam ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", PAR_CASES)
def test_beam(hip_lib, name, form, monkeypatch):
    import beam_ref as BR
    from test_beam import _check_scores_against_oracle, _replay
    m = _bound(name, form)
    W = BEAM_W
    with _tuned(form):
        out = _beam(m, W, trace=True)
        one = _beam(m, 1)
        greedy = _greedy(m)
        _check_bit_equal(m, lambda b: _beam(b, W, trace=True), m.what)                            # check 4
        _check_fold_ran(m, lambda b: _beam(b, W, trace=True), "beam")
    # check 1: test_engine_beams_replay_under_the_numpy_rule
    beams = out["beams"].cpu().numpy()
    got_scores = out["beam_scores"].cpu().numpy().astype(np.float64)
    replayed, scores, okb, left = _replay(out, W, m.T, m.what)
    assert left <= 0.02, (m.what, left)
    assert np.array_equal(beams[okb], replayed[okb]), m.what
    assert torch.equal(out["predict"].cpu(), out["beams"].cpu().reshape(-1, W, m.T)[:, 0])
    live = okb & np.isfinite(scores)
    assert np.array_equal(np.isneginf(got_scores[okb]), np.isneginf(scores[okb]))
    assert (np.abs(got_scores[live] - scores[live]) <= out["steps"] * (BR.LP_BAR + BR.ADD_EPS * np.abs(scores[live]))).all(), m.what
    assert (np.diff(np.where(np.isinf(got_scores), -1e300, got_scores).reshape(-1, W), axis=1) <= 0).all()
    # check 2: W = 1 is the retired greedy decode
    pred, want, steps, glp, kept = _retired_greedy(m, greedy)
    assert one["steps"] == steps and np.array_equal(one["beams"].cpu().numpy(), want), m.what
    assert torch.equal(one["predict"], one["beams"])
    tol = _tol_per_position(m, pred, steps, monkeypatch)
    bound = ((2 * tol + LP_BAR)[None, :] * kept).sum(axis=1)         # the sum of 2 tol + LP_BAR over the row's steps
    err = np.abs(one["beam_scores"].cpu().numpy().astype(np.float64) - glp.sum(axis=1))
    worst2 = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (m.what, worst2)
    line = "beam   %-17s %-15s steps %3d  left out %.2f %%  W=1: worst |dscore| / bound %.3f" % (
        name, form, out["steps"], 100 * left, worst2)
    if form in ARITHMETIC:                                                                        # check 3
        worst = _check_scores_against_oracle(name, m.case, m.sd, m.batch, out, W,
                                             step_tol=_step_tol(m, m.batch, monkeypatch), what=m.what)
        line += "  oracle: worst |dscore| / bound %.3f" % worst
    _record(line)


# ---- sampling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", PAR_CASES)
def test_sample(hip_lib, name, form, monkeypatch):
    from test_sample import _check_layout, _check_scores_against_oracle, _replay
    m = _bound(name, form)
    R = SR.REPLAY_R
    with _tuned(form):
        replays = [(params,) + _sample(m, R, params, SR.REPLAY_SEEDS[name], trace=True) for params in SR.REPLAY_PARAMS]
        zero = [(r, _sample(m, r, (0.0, 4, 0.5), 3)[0]) for r in (1, 3)]
        scored = _sample(m, 2, (1.0, 0, 1.0), 5)[0]
        greedy = _greedy(m)
        _check_bit_equal(m, lambda b: _sample(b, R, SR.REPLAY_PARAMS[1], SR.REPLAY_SEEDS[name], trace=True)[0], m.what)  # check 4
        _check_fold_ran(m, lambda b: _sample(b, R, SR.REPLAY_PARAMS[1], SR.REPLAY_SEEDS[name], trace=True)[0], "sample")
    shares = []
    for params, out, u in replays:                                                                # check 1
        dec, left = _replay(out, u, *params, m.T, (m.what, params))
        assert left <= SR.CAP, (m.what, params, left)
        assert torch.equal(out["predict"], out["samples"].view(-1, R, m.T)[:, 0])
        shares.append(100 * left)
    pred, want, steps, glp, kept = _retired_greedy(m, greedy)                                           # check 2
    tol = _tol_per_position(m, pred, steps, monkeypatch)
    worst2 = 0.0
    for r, out in zero:
        assert out["steps"] == steps, (m.what, r)
        smp = out["samples"].cpu().numpy().reshape(-1, r, m.T)
        for k in range(r):
            assert np.array_equal(smp[:, k], want), (m.what, r, k)
        assert torch.equal(out["predict"], out["samples"].view(-1, r, m.T)[:, 0])
        err = np.abs(out["sample_logprob"].cpu().numpy().astype(np.float64).reshape(-1, r, m.T) - glp[:, None, :])
        assert (err <= (2 * tol + SR.LP_BAR)[None, None, :]).all(), (m.what, r, err.max())
        worst2 = max(worst2, float((err / (2 * tol + SR.LP_BAR)[None, None, :]).max()))
        _check_layout(out, m.T)
    line = "sample %-17s %-15s steps %3d  left out %.2f %% / %.2f %%  tau=0: worst |dlogprob| / bound %.3f" % (
        name, form, replays[0][1]["steps"], shares[0], shares[1], worst2)
    if form in ARITHMETIC:                                                                        # check 3
        worst = _check_scores_against_oracle(name, m.case, m.sd, m.batch, scored, 2,
                                             step_tol=_step_tol(m, m.batch, monkeypatch), what=m.what)
        line += "  oracle: worst |dscore| / bound %.3f" % worst
    _record(line)


# ---- loop-constrained ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", PAR_CASES)
def test_constrain(hip_lib, name, form, monkeypatch):
    from test_constrain import _check_against_oracle, _check_layout, _replay
    m = _bound(name, form)
    lat, lat_gpu, table = _lattice(name)
    with _tuned(form):
        out = _constrain(m, LOOPS, trace=True)
        clear = _constrain(m, 0, lattice=False)
        greedy = _greedy(m)
        _check_bit_equal(m, lambda b: _constrain(b, LOOPS, trace=True), m.what)                   # check 4
        _check_fold_ran(m, lambda b: _constrain(b, LOOPS, trace=True), "constrain")
    pairs, _ = _replay(out, LOOPS, table, max(lat["num_input"]), m.T, m.what)                     # check 1: nothing left out
    assert pairs > 0
    pred, want, steps, glp, kept = _retired_greedy(m, greedy)                                           # check 2
    assert clear["steps"] == steps and np.array_equal(clear["predict"].cpu().numpy(), want), m.what
    assert not bool(clear["dead_end"].any())
    tol = _tol_per_position(m, pred, steps, monkeypatch)
    err = np.abs(clear["logprob"].cpu().numpy().astype(np.float64) - glp)
    assert (err <= (2 * tol + CR.LP_BAR)[None, :]).all(), (m.what, err.max())
    _check_layout(clear, m.T)
    line = "constr %-17s %-15s steps %3d  pairs %d, none left out  bits clear: worst |dlogprob| / bound %.3f" % (
        name, form, out["steps"], pairs, float((err / (2 * tol + CR.LP_BAR)[None, :]).max()))
    if form in ARITHMETIC:                                                                        # check 3
        left, npairs, worst = _check_against_oracle(name, m.case, m.sd, lat, out, step_tol=_step_tol(m, lat, monkeypatch), what=m.what)
        if form != "fp16":
            assert left <= CR.CAP * npairs, (m.what, left, npairs)
        line += "  oracle: worst |dlogit| / tol %.3f, left out %.2f %%" % (worst, 100.0 * left / max(1, npairs))
    _record(line)


# ---- teacher-forced scoring ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", ALL_CASES)
def test_forced(hip_lib, name, form, monkeypatch):
    from test_forced import _check_layout
    from test_parity_golden import _tol
    m = _bound(name, form)
    gold = np.ascontiguousarray(m.z["predict"].reshape(-1, m.T))
    lengths = _own_paths(m, gold, int(m.z["steps"]))
    with _tuned(form):
        out = _forced(m, gold, lengths, trace=True)                                               # along the golden's tokens
        greedy = _greedy(m)
        pred, gsteps = greedy["predict"].cpu().numpy().reshape(-1, m.T), greedy["steps"]
        own_len = _own_paths(m, pred, faces.retired_view(pred, TOK, return_steps=True)[1] if m.parallel else gsteps)
        own = _forced(m, pred, own_len)                                                           # along the form's own greedy decode
        _check_bit_equal(m, lambda b: _forced(b, gold, lengths, trace=True), m.what)              # check 4
        _check_fold_ran(m, lambda b: _forced(b, gold, lengths, trace=True), "forced")
    lp, gr, rk = _check_layout(out, gold, lengths)                                                # check 1 (layout; scores below)
    # check 2: forcing the greedy decode of the same form along its own tokens
    olp, ogr, ork = _check_layout(own, pred, own_len)
    glp = greedy["logprob"].cpu().numpy().reshape(-1, m.T).astype(np.float64)
    margin = (greedy["best"] - greedy["second"]).cpu().numpy().astype(np.float64)
    tol = _tol_per_position(m, pred, gsteps, monkeypatch)
    sure_n = worst2 = 0
    for s in range(int(own_len.max())):
        on = own_len > s
        sure = on & (margin[s] > 2 * tol[s + 1])
        assert (ogr[sure, s + 1] == pred[sure, s + 1]).all() and (ork[sure, s + 1] == 0).all(), (m.what, s)
        err = np.abs(olp[on, s + 1] - glp[on, s + 1])
        assert (err <= 2 * tol[s + 1] + FR.LP_BAR).all(), (m.what, s, float(err.max()))
        worst2 = max(worst2, float(err.max()) / (2 * tol[s + 1] + FR.LP_BAR))
        sure_n += int(sure.sum())
    assert sure_n > 0.5 * own_len.sum()
    line = "forced %-17s %-15s steps %3d  own tokens: %d of %d pairs decisive, worst |dlogprob| / bound %.3f" % (
        name, form, out["steps"], sure_n, int(own_len.sum()), worst2)
    if form in ARITHMETIC:                                                                        # check 3
        steps = int(lengths.max())
        rows = list(range(gold.shape[0]))
        truth = _truth(m, gold, steps)
        step_tol = _step_tol(m, m.batch, monkeypatch)
        if step_tol is None:
            tol_fn = _tol
        else:                                                  # (FR.compare asks once per step, in order)
            tol_of = step_tol(gold, steps, truth)
            it = iter(range(steps))
            tol_fn = lambda ref: tol_of(next(it), ref)
        st = FR.compare(truth, rows, gold, lengths, out["logits"].cpu().numpy(), lp, gr, rk, tol_fn=tol_fn, what=m.what)
        assert st["pairs"] == int(lengths.sum())
        if form != "fp16":
            assert st["left_out"] <= FR.CAP, (m.what, st)
        line += "  oracle: worst |dlogit| / tol %.3f, |dlogprob| / bound %.3f, left out %.2f %%" % (
            st["worst_logit"], st["worst_lp"], 100 * st["left_out"])
    _record(line)
