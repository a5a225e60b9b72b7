"""Closure look-ahead (both forms) in the beam search over the loop-constrained decode: the numpy rule against the
greedy rules of both forms and against the plain constrained beam rule, the containment of the two forms, the C ABI, every
rejection at five layers, the one-step operator against the numpy rule on the kernel's own logits, and the engine against the
constrained greedy decodes (W = 1), the plain constrained beam decode (zero tables), the numpy rule replayed on its own trace,
the exact form's guarantee, the launch forms, the model, the device-side faces and the CLI."""
import ctypes as C
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import beam_ref as BR
import constrain_beam_closure_ref as CL
import constrain_beam_ref as CBR
import constrain_ref as CR
import exact_ref as XR
import lookahead_ref as LR
import test_constrain_beam as TCB
from conftest import ROOT, token_ns
from faceformer_amd import faces
from faceformer_amd.hip import modes as MODES

RECORD = MODES.CONSTRAIN_BEAM_AHEAD
TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
NTOK = TOK.len
FILL = CR.FILL
LOOPS = CR.NO_REPEAT | CR.CONNECT
PARALLEL, SEQ2SEQ = 0, 1
CLOSURES = ("lookahead", "exact")
BUDGETS = (0, 1, 2, 5, 254)
GPW = TCB.GPW
NEW_ENTRIES = ("ff_beam_constrained_select_ahead", "ff_decode_constrained_beam_ahead_workspace_bytes",
               "ff_decode_constrained_beam_ahead")
_CASE_TABLES = {}


# ---- the operator cases (also read by tools/constrain_beam_closure_left_out.py) ------------------------------------------------------
def case_tables(c):
    """(close_dist [NW, L, L], cycle_len [NW, L]) uint8 of an operator case's follow tables (faces.follow_distance, hmax 254)."""
    key = (c["S"], c["W"], c["G"])
    if key not in _CASE_TABLES:
        L, NW = c["L"], c["NW"]
        _CASE_TABLES[key] = faces.follow_distance(c["follows"], 254) if L else (np.zeros((NW, 0, 0), np.uint8), np.zeros((NW, 0), np.uint8))
    return _CASE_TABLES[key]


def rule_on_case(c, closure, budget, tables=None):
    """constrain_beam_closure_ref.beam_step on a case's inputs under `closure` (or "plain")."""
    close, cyc = case_tables(c) if tables is None else tables
    return CL.beam_step(CL.FORMS.get(closure, closure), c["logits"].numpy().astype(np.float64), c["pad"], c["scores"].astype(np.float64),
                        c["fin"] != 0, c["dead"] != 0, TCB.case_states(c), c["W"], LOOPS, c["ntok"], c["term"], lambda w: c["follows"][w],
                        np.arange(c["G"]) // GPW, lambda w: close[w], lambda w: cyc[w], budget)


# ---- CPU: the numpy rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 65, 260])
def test_numpy_rule_at_width_1_is_the_greedy_rule_of_the_form(S):
    c = TCB.operator_case(9, 1, S, TCB.op_seed(S, 1, 9), greedy=True)
    close, cyc = case_tables(c)
    sts = TCB.case_states(c)
    for closure in CLOSURES:
        for budget in BUDGETS:
            res = rule_on_case(c, closure, budget)
            for b in range(9):
                w = b // GPW
                raw = c["logits"][b].numpy().astype(np.float64)
                if closure == "lookahead":
                    one = LR.step_row(raw, c["pad"][w], sts[b], LOOPS, c["ntok"], c["term"], c["follows"][w], close[w], cyc[w], budget,
                                      finished=bool(c["fin"][b]))
                else:
                    one = XR.step_row(raw, c["pad"][w], sts[b], c["ntok"], c["term"], c["follows"][w], cyc[w], budget, finished=bool(c["fin"][b]))
                if c["fin"][b]:
                    assert (res["tok"][b], res["scores"][b], bool(res["fin"][b])) == (0, 0.0, True)
                    continue
                got = (res["tok"][b], bool(res["fin"][b]), bool(res["dead"][b]), res["states"][b])
                assert got == (one["tok"], bool(one["fin"]), bool(one["dead"]), one["state"]), (S, closure, budget, b)
                assert res["parent"][b] == 0 and abs(res["scores"][b] - one["logprob"]) <= 1e-12, (S, closure, budget, b)
                assert np.array_equal(res["masked"][b], one["masked"]), (S, closure, budget, b)


@pytest.mark.parametrize("S", [5, 65, 260])
def test_numpy_rule_with_zero_tables_is_the_plain_constrained_beam_rule(S):
    for W in (2, 4, 8):
        if W > S:
            continue
        c = TCB.operator_case(9, W, S, TCB.op_seed(S, W, 9))
        zero = (np.zeros((c["NW"], c["L"], c["L"]), np.uint8), np.zeros((c["NW"], c["L"]), np.uint8))
        want = TCB.rule_on_case(c, LOOPS)
        for budget in (0, 5):
            res = rule_on_case(c, "lookahead", budget, zero)
            for k in ("parent", "tok", "scores", "fin", "dead", "dead_now", "gap"):
                assert np.array_equal(res[k], want[k]), (S, W, budget, k)
            assert res["states"] == want["states"]
            assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(res["masked"], want["masked"]))
        assert np.array_equal(rule_on_case(c, "plain", 3)["scores"], want["scores"])


def _contained(table, st, budget, ntok=NTOK):
    L = table.shape[0]
    close, cyc = faces.follow_distance(table, 254)
    pad = np.zeros(ntok + L, dtype=bool)
    a, da = LR.rule_mask(st, LOOPS, ntok + L, ntok, TERM, table, pad, close, cyc, budget)
    x, dx = XR.rule_mask(st, ntok + L, ntok, TERM, table, pad, cyc, budget)
    assert not (a[ntok:] & ~x[ntok:]).any(), (st, budget)                # every edge key the look-ahead masks, the exact form masks
    assert dx or not da, (st, budget)                                     # ... so a dead end of the look-ahead is one of the exact form
    return int((x[ntok:] & ~a[ntok:]).sum())


def test_the_exact_form_contains_the_lookahead_form():
    more = 0
    for seed in range(4):
        table = CR.random_follows(1, 24, 40 + seed)[0]
        rng = np.random.default_rng(seed)
        for start in range(0, 24, 5):
            for st in XR.walk_states(table, start, 10, rng):
                for budget in (0, 1, 2, 5, 254):
                    more += _contained(table, st, budget)
    assert more > 0                                                       # the exact form does mask more somewhere
    st = (frozenset({0, 1}), 0, 1)
    assert _contained(XR.trap(), st, 5) > 0                               # the hand-written trap: edge 3 is live under the look-ahead only
    # and through the beam rule: one group, two beams in the trap state, equal raw rows
    raw = np.zeros((2, 4))
    close, cyc = faces.follow_distance(XR.trap(), 254)
    args = (raw, np.zeros(4, bool), np.array([0.0, -1.0]), np.zeros(2, bool), np.zeros(2, bool), [st, st], LOOPS, 0, (0, 0), XR.trap(), close, cyc, 5)
    la, ex = CL.group_step("ahead", *args), CL.group_step("exact", *args)
    for k in range(2):
        assert not (la["masked"][k] & ~ex["masked"][k]).any() and (ex["masked"][k] & ~la["masked"][k]).any()


# ---- CPU: the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_fields_agree_within_abi_105():
    from faceformer_amd.hip import lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define FF_ABI_VERSION 105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
    assert "DESIGN.md 28" in header
    doc = header[header.index("closure look-ahead (both forms) in the beam search"): header.index("typedef struct ff_beam_constrained_ahead_step")]
    for phrase in ("All beams of a launch share the step's budget = T - 1 - position", "close_dist[w][first]", "cycle_len[w] while it is",
                   "one backward search per open beam, over that beam's own visited words", "The dead-end vote runs after these masks",
                   "width 1 equals the constrained greedy decode of the same form", "both tables all zero equals ff_decode_constrained_beam",
                   "every edge key that lookahead = 1 masks is masked by lookahead = 2", "only right after the edge that opened a loop",
                   "T > 256", "L + ntok > 2048"):
        assert phrase in doc, phrase
    fields = TCB._struct_fields
    assert [f for f, _ in lib.ConstrainBeamAheadParams._fields_] == fields(header, "ff_constrain_beam_ahead_params") == \
        ["width", "flags", "follows", "lookahead", "close_dist", "cycle_len", "beams", "scores", "dead_end", "trace_parent"]
    assert [f for f, _ in lib.BeamConstrainedAheadStep._fields_] == fields(header, "ff_beam_constrained_ahead_step") == \
        ["step", "lookahead", "close_dist", "cycle_len", "budget"]
    assert lib.BeamConstrainedAheadStep._fields_[0][1] is lib.BeamConstrainedStep
    assert [f for f, _ in lib.ConstrainBeamParams._fields_] == fields(header, "ff_constrain_beam_params")      # (unchanged)
    nargs = lambda name: len(re.search(r"\b%s\s*\((.*?)\)" % name, code, re.S).group(1).split(","))
    for name in NEW_ENTRIES:
        assert len(lib.SIGNATURES[name][1]) == nargs(name), name
    S = lib.SIGNATURES
    assert len(S["ff_decode_constrained_beam_ahead"][1]) == len(S["ff_decode_constrained_beam"][1])
    assert S["ff_decode_constrained_beam_ahead_workspace_bytes"] == S["ff_decode_constrained_beam_workspace_bytes"]


def test_a_library_without_the_new_entries_is_refused(monkeypatch):
    from faceformer_amd.hip import lib

    class Old:
        def __getattr__(self, name):
            if name in NEW_ENTRIES:
                raise AttributeError(name)
            return types.SimpleNamespace(restype=None, argtypes=None)
    monkeypatch.setattr(lib.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="does not export ff_beam_constrained_select_ahead .*rebuild"):
        lib.load()


def test_the_mode_record_is_a_replacement_of_constrain_beam_outside_the_table():
    from faceformer_amd.hip import engine, modes
    rec, base = RECORD, modes.CONSTRAIN_BEAM
    assert rec not in modes.MODES and rec.entry == "ff_decode_constrained_beam_ahead" and rec.per_anchor
    assert (rec.subject, rec.excludes, rec.switches, rec.outs) == (base.subject, base.excludes, base.switches, base.outs)
    assert [n for n, _ in rec.own] == ["follow_table", "close_dist", "cycle_len"]
    of = modes.of_options
    assert of(False, 4, constrain=3, num_samples=0, beam_width=0) == (base, 4)
    assert of(False, 4, constrain_beam_closure=None, constrain=3, num_samples=0, beam_width=0) == (base, 4)
    for closure in CLOSURES:
        assert of(False, 4, constrain_beam_closure=closure, constrain=3, num_samples=0, beam_width=0) == (rec, 4)
        assert of(False, 0, constrain_beam_closure=closure, constrain=3, num_samples=0, beam_width=0) == (modes.CONSTRAIN, 3)
    assert inspect.signature(engine.PathEngine.decode).parameters["constrain_beam_closure"].default is None
    assert inspect.signature(of).parameters["constrain_beam_closure"].default is None


def test_c_entries_reject_bad_arguments_before_any_launch(hip_lib):
    """FF_ERR_ARG with the offending argument named, on a host without a GPU: the checks run in front of every HIP call."""
    from faceformer_amd.hip import lib
    FF_ERR_ARG = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    name = b"ff_beam_constrained_select_ahead"

    def step(look=1, close=p, cyc=p, budget=3, flags=LOOPS, width=2, S=8, L=4, visited_out=None):
        d = lib.BeamConstrainedStep(p, S, S, None, None, 2, width, 1, p, L, flags, 4, 1, 4, p, p, p, p, p, p, p, p, p, p, p,
                                    visited_out or C.addressof(buf) + 64, p, p, p, None, 0, None, 0, None, None)
        return hip_lib.ff_beam_constrained_select_ahead(C.byref(lib.BeamConstrainedAheadStep(d, look, close, cyc, budget)), None)
    for kw, text in ((dict(look=0), b"lookahead=0"), (dict(look=3), b"lookahead=3"), (dict(flags=CR.NO_REPEAT), b"FF_CONSTRAIN_CONNECT"),
                     (dict(close=None), b"close_dist"), (dict(cyc=None), b"cycle_len"), (dict(look=2, cyc=None), b"cycle_len"),
                     (dict(budget=-1), b"budget"), (dict(budget=255), b"budget"), (dict(flags=4 | LOOPS), b"unknown flag bits"),
                     (dict(look=2, flags=CR.CONNECT), b"FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT"),
                     (dict(look=2, S=2052, L=2048), b"2048"), (dict(width=9), b"width"), (dict(visited_out=p), b"visited_out")):
        assert step(**kw) == FF_ERR_ARG and text in hip_lib.ff_last_error(), (kw, hip_lib.ff_last_error())
        assert name in hip_lib.ff_last_error(), kw
    assert hip_lib.ff_beam_constrained_select_ahead(None, None) == FF_ERR_ARG
    m, prm = lib.Model(), lib.DecodeParams()
    m.num_token, m.E = 4, 64
    prm.variant, prm.N, prm.L, prm.F, prm.T, prm.term_lo, prm.term_hi = lib.FF_PARALLEL, 1, 4, 4, 6, 1, 4
    name = b"ff_decode_constrained_beam_ahead"

    def decode(prm=prm, extra=None, best=None, **fields):
        a = lib.ConstrainBeamAheadParams(2, LOOPS, p, 1, p, p, p, p, p, None)
        for k, v in fields.items():
            setattr(a, k, v)
        return hip_lib.ff_decode_constrained_beam_ahead(C.byref(m), C.byref(prm), p, p, p, p, None, extra, p, None, None, None, None, best,
                                                        None, p, p, 1024, C.byref(a), None)
    for fields, text in ((dict(lookahead=0), b"lookahead=0"), (dict(lookahead=3), b"lookahead=3"), (dict(flags=CR.NO_REPEAT), b"FF_CONSTRAIN_CONNECT"),
                         (dict(flags=4 | LOOPS), b"unknown flag bits"), (dict(follows=None), b"follow table"),
                         (dict(close_dist=None), b"close_dist"), (dict(cycle_len=None), b"cycle_len"),
                         (dict(lookahead=2, cycle_len=None), b"cycle_len"),
                         (dict(lookahead=2, flags=CR.CONNECT), b"FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT"),
                         (dict(width=0), b"width=0"), (dict(width=9), b"width=9"), (dict(beams=None), b"beams, scores and dead_end"),
                         (dict(dead_end=None), b"beams, scores and dead_end"), (dict(extra=p), b"extra mask"), (dict(best=p), b"best / second")):
        assert decode(**fields) == FF_ERR_ARG and text in hip_lib.ff_last_error(), (fields, hip_lib.ff_last_error())
        assert name in hip_lib.ff_last_error(), fields

    def changed(**kw):
        q = lib.DecodeParams()
        C.memmove(C.byref(q), C.byref(prm), C.sizeof(prm))
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    for kw, text in ((dict(T=257), b"T=257"), (dict(variant=lib.FF_SEQ2SEQ), b"parallel-variant"), (dict(flags=lib.FF_RETIRE_FINISHED), b"excludes"),
                     (dict(flags=lib.FF_RETURN_POINTER), b"excludes"), (dict(flags=lib.FF_NO_STOP), b"excludes"),
                     (dict(term_lo=4), b"terminator range"), (dict(term_hi=5), b"terminator range")):
        assert decode(prm=changed(**kw)) == FF_ERR_ARG and text in hip_lib.ff_last_error(), kw
    assert decode(prm=changed(L=2045), lookahead=2) == FF_ERR_ARG and b"2048" in hip_lib.ff_last_error()
    assert hip_lib.ff_decode_constrained_beam_ahead_workspace_bytes(C.byref(m), C.byref(prm), None, 9) == 0
    assert hip_lib.ff_decode_constrained_beam_ahead(None, None, p, p, p, p, None, None, p, None, None, None, None, None, None, p, p, 1024,
                                                    None, None) == FF_ERR_ARG


# ---- CPU: every rejection, with its text, before the library is touched ------------------------------------------------------------------
_raises = TCB._raises
VALUE = "constrain_beam_closure='near': must be None, 'lookahead' or 'exact'"
NEEDS_BEAMS = ("constrain_beam_closure='exact' needs constrain_beams: it is the closure look-ahead of the beam search over the "
               "constrained keys")
NEEDS_LOOPS = ("constrain_beam_closure='lookahead' needs constrain='loops' (FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT): without "
               "CONNECT no loop is tracked")
EXCLUDES = "constrain_beams excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width and num_samples"


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


def test_engine_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine, modes
    _untouchable(monkeypatch)
    value = modes.constrain_beam_closure_value
    assert value(None, None) is None and value(None, 3, 4) is None
    assert value("lookahead", 3, 4) == "lookahead" and value("exact", 3, 1) == "exact"
    for bad in ("near", True, 1, ""):
        _raises("constrain_beam_closure=%r: must be None, 'lookahead' or 'exact'" % (bad,), value, bad, 3, 4)
    _raises(NEEDS_BEAMS, value, "exact", 3, 0)
    _raises(NEEDS_LOOPS, value, "lookahead", CR.NO_REPEAT, 4)
    _raises(NEEDS_LOOPS, value, "lookahead", None, 4)
    _raises("constrain_beam_closure='exact' needs constrain='loops' (FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT): without CONNECT no loop "
            "is tracked", value, "exact", CR.CONNECT, 4)
    _raises("constrain_beam_closure excludes constrain_lookahead, constrain_exact and constrain_samples: they are the look-aheads of the "
            "greedy and the sampled decode", value, "exact", 3, 4, True)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng.num_token, eng.device = 4, torch.device("cpu")
    memory = torch.zeros(2, 12, 64)
    table = torch.zeros(2, 8, 1, dtype=torch.int32)
    close, cyc = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.uint8)
    base = dict(T=5, F=4, num_input=[4, 3], term_range=TERM, constrain="loops", follow_table=table, constrain_beams=2,
                constrain_beam_closure="lookahead", close_dist=close, cycle_len=cyc)
    dec = lambda **kw: eng.decode(kw.pop("memory", memory), None, None, kw.pop("variant", PARALLEL), **dict(base, **kw))
    _raises(VALUE, dec, constrain_beam_closure="near")
    _raises(NEEDS_BEAMS, dec, constrain_beam_closure="exact", constrain_beams=None)
    _raises(NEEDS_BEAMS, dec, constrain_beam_closure="exact", constrain_beams=0)
    _raises(NEEDS_LOOPS, dec, constrain="no_repeat")
    _raises("constrain_beams=2 needs constrain ('no_repeat' or 'loops'): it is the beam search over the constrained keys", dec, constrain=None)
    # the pinned rejections keep their texts when the greedy / sampled decode's own look-aheads come with constrain_beams
    _raises("constrain_lookahead excludes constrain_beams: the beam search over the constrained keys has no look-ahead", dec, constrain_lookahead=True)
    _raises("constrain_exact excludes constrain_beams: the beam search over the constrained keys has no look-ahead", dec, constrain_exact=True)
    _raises("constrain_samples excludes constrain_beams: a decode draws from the constrained keys or searches them", dec, constrain_samples=2)
    _raises("constrain_beams is a parallel-variant option", dec, variant=SEQ2SEQ)
    _raises("constrain_beams needs term_range = (lo, hi) with lo < hi", dec, term_range=(3, 3))
    for k, v in (("retire", True), ("return_pointer", True), ("no_stop", True), ("stop_callback", lambda c: False),
                 ("extra_mask", torch.zeros(1)), ("logprob", True), ("beam_width", 2), ("num_samples", 2)):
        _raises(EXCLUDES, dec, **{k: v})
    _raises("constrain_beams=9: must be None, 0 or a width in 1..8", dec, constrain_beams=9)
    _raises("constrain='loops' needs follow_table (ops.follow_table)", dec, follow_table=None)
    _raises("constrain_beam_closure takes T <= 256 (got 257): the budget T - 2 must fit the tables' byte", dec, T=257)
    _raises("constrain_beam_closure='lookahead' needs close_dist and cycle_len (ops.follow_distance)", dec, close_dist=None)
    _raises("constrain_beam_closure='lookahead' needs close_dist and cycle_len (ops.follow_distance)", dec, cycle_len=None)
    _raises("constrain_beam_closure='exact' needs cycle_len (ops.follow_distance)", dec, constrain_beam_closure="exact", cycle_len=None)
    _raises("follow_table must be an int32 tensor of shape [2, 8, 1]", dec, follow_table=torch.zeros(2, 8, 2, dtype=torch.int32))
    _raises("close_dist must be a uint8 tensor of shape [2, 8, 8]", dec, close_dist=torch.zeros(2, 8, 7, dtype=torch.uint8))
    _raises("cycle_len must be a uint8 tensor of shape [2, 8]", dec, cycle_len=torch.zeros(2, 8, dtype=torch.int32))
    _raises("cycle_len must be a uint8 tensor of shape [2, 8]", dec, constrain_beam_closure="exact", close_dist=None, cycle_len=torch.zeros(2, 9, dtype=torch.uint8))
    big = 2046
    _raises("constrain_beam_closure='exact' takes at most 2044 edges per wireframe (got 2046): L + num_token <= 2048 keys", dec,
            memory=torch.zeros(1, big + 4, 64), num_input=[4], constrain_beam_closure="exact",
            follow_table=torch.zeros(1, big, 64, dtype=torch.int32), cycle_len=torch.zeros(1, big, dtype=torch.uint8))


def test_operator_wrapper_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import ops
    _untouchable(monkeypatch)
    monkeypatch.setattr(ops, "_dev", lambda t, name, dtype=torch.float32: None)      # (CPU tensors: the checks behind the device check)
    monkeypatch.setattr(ops, "_on_tensor_device", lambda fn: fn)
    B, S, ntok, W = 4, 12, 4, 2
    L = S - ntok
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    ok = dict(logits=torch.zeros(B, S), scores=torch.zeros(B), fin=i32(B), dead=i32(B), first=i32(B), prev=i32(B), visited=i32(B, 1), width=W,
              flags=LOOPS, ntok=ntok, follows=i32(1, L, 1), lookahead="lookahead", cycle_len=u8(1, L), budget=3, close_dist=u8(1, L, L))
    fn = getattr(ops.beam_constrained_select_ahead, "__wrapped__", ops.beam_constrained_select_ahead)
    run = lambda **kw: fn(**dict(ok, **kw))
    _raises("lookahead='plain': must be 'lookahead' or 'exact'", run, lookahead="plain")
    _raises("lookahead=None: must be 'lookahead' or 'exact'", run, lookahead=None)
    _raises("the look-ahead needs FF_CONSTRAIN_CONNECT", run, flags=CR.NO_REPEAT, follows=None)
    _raises("the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT", run, lookahead="exact", flags=CR.CONNECT)
    _raises("close_dist must be a contiguous uint8 [>= 1, 8, 8] tensor", run, close_dist=u8(1, L, L - 1))
    _raises("cycle_len must be a contiguous uint8 [>= 1, 8] tensor", run, cycle_len=u8(1, L + 1))
    _raises("cycle_len must be a contiguous uint8 [>= 1, 8] tensor", run, lookahead="exact", close_dist=None, cycle_len=u8(L))
    _raises("budget=255: must be in 0..254", run, budget=255)
    _raises("budget=-1: must be in 0..254", run, lookahead="exact", budget=-1)
    _raises("beam_constrained_select_ahead takes at most 2048 keys (L + ntok; got 2052)", run, lookahead="exact", logits=torch.zeros(B, 2052),
            visited=i32(B, 64), follows=i32(1, 2048, 64), cycle_len=u8(1, 2048))
    _raises("beam width 9: must be in 1..8, at most S = 12, and divide the 4 rows", run, width=9)


def test_models_and_decode_sharded_reject_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    model = TCB._tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert model.constrain_beam_closure is None

    def fwd(m, text, inputs=None, **attrs):
        for k, v in attrs.items():
            setattr(m, k, v)
        with torch.no_grad():
            _raises(text, m.forward_eval, inputs or TCB._tiny_inputs())

    fwd(model, NEEDS_BEAMS, constrain="loops", constrain_beam_closure="exact")
    fwd(model, VALUE, constrain_beams=2, constrain_beam_closure="near")
    fwd(model, NEEDS_LOOPS, constrain="no_repeat", constrain_beam_closure="lookahead")
    fwd(model, "constrain_beams=2 needs constrain ('no_repeat' or 'loops'): it is the beam search over the constrained keys", constrain=None)
    model.constrain = "loops"
    fwd(model, "constrain_lookahead excludes constrain_beams: the beam search over the constrained keys has no look-ahead", constrain_lookahead=True)
    model.constrain_lookahead = False
    fwd(model, "constrain_exact excludes constrain_beams: the beam search over the constrained keys has no look-ahead", constrain_exact=True)
    model.constrain_exact = False
    fwd(model, "constrain_samples excludes constrain_beams: a decode draws from the constrained keys or searches them", constrain_samples=2)
    model.constrain_samples = 0
    for attr, val in (("retire_finished", True), ("beam_width", 2), ("num_samples", 2), ("return_logprob", True)):
        old = getattr(model, attr)
        fwd(model, "constrain excludes beam_width, num_samples, retire_finished, return_logprob and an extra mask", **{attr: val})
        setattr(model, attr, old)
    fwd(model, "constrain excludes beam_width, num_samples, retire_finished, return_logprob and an extra mask",
        dict(TCB._tiny_inputs(), extra_mask=torch.zeros(1, 4, 8, dtype=torch.bool)))
    long = TCB._tiny_model(SurfaceFormer_Parallel, max_face_length=257)
    fwd(long, "constrain_beam_closure takes T <= 256 (got 257): the budget T - 2 must fit the tables' byte", constrain="loops",
        constrain_beams=2, constrain_beam_closure="lookahead")
    fwd(model, "cycle_len must be uint8 [1, 8]", dict(TCB._tiny_inputs(), cycle_len=torch.zeros(1, 9, dtype=torch.uint8)), constrain_beam_closure="exact")
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        loop = TCB._tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        inputs = TCB._tiny_inputs()
        fwd(loop, "constrain_beam_closure needs the native engine: this model's constructor arguments take the sub-module loop", inputs,
            constrain="loops", constrain_beams=2, constrain_beam_closure="exact")
        assert "predict" not in inputs
    seq = TCB._tiny_model(SurfaceFormer, label_seq_length=6)
    seq.constrain_beam_closure = "exact"
    sin = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool), "label": torch.zeros(1, 6, dtype=torch.long)}
    with torch.no_grad():
        _raises("constrain_beam_closure is a SurfaceFormer_Parallel option (the single-sequence model emits loops of plain edges)",
                seq.forward_eval, sin)
        seq.constrain_beam_closure = "near"
        _raises(VALUE, seq.forward_eval, sin)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    ns = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain="loops", constrain_beams=2,
                               constrain_beam_closure="exact")
    _raises("decode_sharded does not implement constrain_beam_closure (a constrained decode takes no external stop rule)", dist.decode_sharded,
            ns, {}, NoDist())
    ns.constrain_beam_closure = None
    _raises("decode_sharded does not implement constrain (a constrained decode takes no external stop rule)", dist.decode_sharded, ns, {}, NoDist())


def _cli():
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    return cli


def test_cli_flag_reaches_the_model_and_rejects(monkeypatch):
    cli = _cli()
    _untouchable(monkeypatch)
    parse = cli.build_parser().parse_args
    args = parse(["--test_ckpt", "x.ckpt", "--constrain", "loops", "--constrain-beams", "4", "--constrain-beam-closure", "exact"])
    assert (args.constrain, args.constrain_beams, args.constrain_beam_closure) == ("loops", 4, "exact")
    assert parse(["--test_ckpt", "x.ckpt"]).constrain_beam_closure is None
    with pytest.raises(SystemExit):
        parse(["--test_ckpt", "x.ckpt", "--constrain-beam-closure", "near"])
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--constrain", "loops", "--constrain-beams", "2", "--constrain-beam-closure", "lookahead", "--test_ckpt", "unused.ckpt"])
    cli.main(["--constrain", "loops", "--constrain-beams", "2", "--test_ckpt", "unused.ckpt"])
    assert [(kw["constrain_beams"], kw["constrain_beam_closure"]) for kw in seen] == [(2, "lookahead"), (2, None)]
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3, constrain_beams=4, constrain_beam_closure="exact")
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3, constrain_beams=4, constrain_beam_closure="exact")
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3, constrain_beams=4)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3, constrain_beams=4)                 # no attribute without the flag
    cfg = types.SimpleNamespace(model_class="SurfaceFormer_Parallel")
    run = lambda **kw: run_test(cfg, None, out_dir="unused", device="cpu", model=object(), **kw)
    needs = "--constrain-beam-closure requires --constrain loops --constrain-beams W"
    _raises(needs, run, constrain_beam_closure="exact")
    _raises(needs, run, constrain="loops", constrain_beam_closure="exact")
    _raises(needs, run, constrain="no_repeat", constrain_beams=2, constrain_beam_closure="lookahead")
    _raises("--constrain-beam-closure must be lookahead or exact", run, constrain="loops", constrain_beams=2, constrain_beam_closure="near")
    _raises("--constrain-beam-closure is not implemented for multi-rank runs", run, constrain="loops", constrain_beams=2,
            constrain_beam_closure="exact", dist_mod=types.SimpleNamespace(get_world_size=lambda: 2))
    _raises("--constrain-exact is not implemented with --constrain-beams", run, constrain="loops", constrain_beams=2, constrain_exact=True,
            constrain_beam_closure="exact")
    _raises("--constrain-lookahead is not implemented with --constrain-beams", run, constrain="loops", constrain_beams=2,
            constrain_lookahead=True, constrain_beam_closure="exact")


# ---- GPU: the operator -------------------------------------------------------------------------------------------------------------------
_bits = TCB._bits


def _dev_tables(c, tables=None):
    close, cyc = case_tables(c) if tables is None else tables
    return torch.from_numpy(np.array(close)).cuda(), torch.from_numpy(np.array(cyc)).cuda()


def _operands(c):
    L = c["L"]
    t = lambda k: torch.from_numpy(c[k]).cuda()
    vis = _bits(c["visited"]) if L else torch.zeros(c["G"] * c["W"], 0, dtype=torch.int32).cuda()
    fol = _bits(c["follows"]) if L else torch.zeros(c["NW"], 0, 0, dtype=torch.int32).cuda()
    return t, vis, fol


def _run_ahead(c, closure, budget, tables=None, **kw):
    from faceformer_amd.hip import ops
    lg = c["logits"].clone().cuda()
    t, vis, fol = _operands(c)
    close, cyc = _dev_tables(c, tables)
    res = ops.beam_constrained_select_ahead(lg, t("scores"), t("fin"), t("dead"), t("first"), t("prev"), vis, c["W"], LOOPS, c["ntok"], fol,
                                            closure, cyc, budget, close_dist=close if closure == "lookahead" else None,
                                            memory=c["memory"].cuda(), mask=c["mask"].to(torch.uint8).cuda(), kv_len=c["kv"].cuda(),
                                            groups_per_wireframe=GPW, term_range=c["term"], want_rows=True, want_stats=True, **kw)
    return lg, res


def _check_operator_case(c, closure, budget, seen):
    """One launch against the numpy rule on the kernel's own fp32 logits.  Returns (groups, groups left out as indecisive)."""
    G, W, S, L, ntok = c["G"], c["W"], c["S"], c["L"], c["ntok"]
    B = G * W
    what = (S, W, G, closure, budget)
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_ahead(c, closure, budget, counter=counter)
    own, raw = lg.cpu().numpy(), c["logits"].numpy()
    want = rule_on_case(c, closure, budget)
    plain = TCB.rule_on_case(c, LOOPS)
    got = {k: res[k].cpu().numpy() for k in ("parent", "next", "scores", "fin", "dead", "first", "prev")}
    rows = res["mask_rows"].cpu().numpy() != 0
    sts = TCB.case_states(c)
    for b in range(B):                                                   # the byte rows and the FILL pattern: exact, always
        pad = c["pad"][(b // W) // GPW]
        if want["rows"][b] is None:
            assert np.array_equal(own[b], raw[b]), (what, b)              # empty / finished: untouched
            seen["empty" if c["scores"][b] == -np.inf else "finished"] += 1
            continue
        assert np.array_equal(rows[b], want["masked"][b]), (what, b)
        assert np.array_equal(own[b] == np.float32(FILL), want["masked"][b] | pad), (what, b)
        assert np.array_equal(own[b][own[b] != np.float32(FILL)], raw[b][~(want["masked"][b] | pad)]), (what, b)
        st = sts[b]
        seen["dead" if want["dead_now"][b] else ("open" if (st[1] is not None and st[2] is not None) else "closed")] += 1
        seen["ahead"] += bool((want["masked"][b][ntok:] & ~plain["masked"][b][ntok:]).any())      # the form masked what the plain rule leaves
        seen["much_visited"] += len(st[0]) > L // 2 > 0
        seen["nolive"] += bool((own[b] == np.float32(FILL)).all())
    left = nge = 0
    for gi in range(G):
        sl = slice(gi * W, (gi + 1) * W)
        for r in range(W):                                               # no kept candidate is a masked key: whatever the gaps
            b, p = gi * W + r, int(got["parent"][gi * W + r])
            if got["scores"][b] > -np.inf and not c["fin"][gi * W + p] and not (own[gi * W + p] == np.float32(FILL)).all():
                assert own[gi * W + p, got["next"][b]] > np.float32(FILL), (what, gi, r)
        if not want["gap"][gi] > 1.0:
            left += 1
            continue
        for k, wk in (("parent", "parent"), ("next", "tok")):
            assert np.array_equal(got[k][sl], want[wk][sl]), (what, gi, k, got[k][sl], want[wk][sl])
        assert np.array_equal(got["fin"][sl] != 0, want["fin"][sl]) and np.array_equal(got["dead"][sl] != 0, want["dead"][sl]), (what, gi)
        f, p, v = CL.pack_state(want["states"][sl], L)
        assert np.array_equal(got["first"][sl], f) and np.array_equal(got["prev"][sl], p), (what, gi)
        assert np.array_equal(res["visited"][sl].cpu().numpy(), v), (what, gi)
        ws, gs = want["scores"][sl], got["scores"][sl].astype(np.float64)
        assert np.array_equal(np.isinf(ws), np.isinf(gs)), (what, gi)
        fi = ~np.isinf(ws)
        assert (np.abs(gs[fi] - ws[fi]) <= BR.LP_BAR + BR.ADD_EPS * np.abs(ws[fi])).all(), (what, gi, gs, ws)
        nge += int(((want["tok"][sl] >= ntok) & ~(c["fin"][sl][want["parent"][sl]] != 0) & fi).sum())
    if left == 0:
        assert int(counter.item()) == nge, what
    return G, left


def _check_width_1_is_the_greedy_operator(c, closure, budget):
    from faceformer_amd.hip import ops
    what = (c["S"], c["G"], closure, budget)
    lg, res = _run_ahead(c, closure, budget)
    t, vis, fol = _operands(c)
    close, cyc = _dev_tables(c)
    lg1 = c["logits"].clone().cuda()
    kw = dict(memory=c["memory"].cuda(), mask=c["mask"].to(torch.uint8).cuda(), kv_len=c["kv"].cuda(), seqs_per_group=GPW, term_range=c["term"],
              want_rows=True, want_stats=True)
    if closure == "lookahead":
        one = ops.pointer_constrained_ahead(lg1, t("fin"), t("first"), t("prev"), vis, LOOPS, c["ntok"], fol, close, cyc, budget, **kw)
    else:
        one = ops.pointer_constrained_exact(lg1, t("fin"), t("first"), t("prev"), vis, LOOPS, c["ntok"], fol, cyc, budget, **kw)
    for a, b in (("next", "next"), ("fin", "fin"), ("dead", "dead_end"), ("first", "first"), ("prev", "prev"), ("visited", "visited"),
                 ("rows", "rows"), ("stats", "stats"), ("scores", "logprob"), ("mask_rows", "mask_rows")):
        assert torch.equal(res[a], one[b]), (what, a)                    # (the score bit-equal to the log-probability)
    assert torch.equal(lg, lg1) and not bool(res["parent"].any()), what


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
@pytest.mark.parametrize("S", TCB.OP_S)
def test_operator_against_the_numpy_rule(hip_lib, S, closure):
    seen = dict(open=0, closed=0, dead=0, finished=0, empty=0, nolive=0, ahead=0, much_visited=0)
    groups = left = 0
    for W in TCB.OP_W:
        if W > S:
            continue
        for G in TCB.OP_G:
            c = TCB.operator_case(G, W, S, TCB.op_seed(S, W, G))
            for budget in BUDGETS:
                g, l = _check_operator_case(c, closure, budget, seen)
                groups, left = groups + g, left + l
            lg, res = _run_ahead(c, closure, 2)
            lg2, res2 = _run_ahead(c, closure, 2)                        # two launches: bit-equal
            assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), (S, W, G)
            if closure == "lookahead":                                   # zero tables: the plain constrained beam launch, bit for bit
                zero = (np.zeros_like(case_tables(c)[0]), np.zeros_like(case_tables(c)[1]))
                lgz, rz = _run_ahead(c, closure, 2, zero)
                lgp, rp = TCB._run_operator(c, LOOPS)
                assert all(torch.equal(rz[k], rp[k]) for k in rp) and torch.equal(lgz, lgp), (S, W, G)
            if W == 1:
                cg = TCB.operator_case(G, 1, S, TCB.op_seed(S, W, G), greedy=True)
                for budget in BUDGETS:
                    _check_width_1_is_the_greedy_operator(cg, closure, budget)
    print("S=%d %s: %d groups, %d left out as indecisive (%.2f %%); beams by state: %s" % (S, closure, groups, left, 100.0 * left / groups, seen))
    assert left <= CL.CAP * groups, (S, closure, left, groups)
    if S >= 63:
        assert all(v > 0 for v in seen.values()), seen                   # every state was exercised


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
def test_operator_inside_poisoned_surroundings(hip_lib, closure):
    """Every operand embedded in poison (tests/redzone.py): the results equal the clean run's and nothing around an operand is
    written."""
    import redzone
    from faceformer_amd.hip import lib as L_
    c = TCB.operator_case(9, 4, 65, TCB.op_seed(65, 4, 9))
    budget = 3
    _, clean = _run_ahead(c, closure, budget)
    guard = redzone.Guard()
    e = lambda t, name: redzone.embed(t, guard=guard, name=name)
    B, S, L = 36, 65, c["L"]
    fw = (L + 31) // 32
    lg = e(c["logits"], "logits")
    ins = {k: e(torch.from_numpy(c[k]), k) for k in ("scores", "fin", "dead", "first", "prev")}
    vis, fol = e(_bits(c["visited"]).cpu(), "visited"), e(_bits(c["follows"]).cpu(), "follows")
    mem, mask, kv = e(c["memory"], "memory"), e(c["mask"].to(torch.uint8), "mask"), e(c["kv"], "kv_len")
    close, cyc = (e(torch.from_numpy(np.array(t)), n) for t, n in zip(case_tables(c), ("close_dist", "cycle_len")))
    i32, f32 = torch.int32, torch.float32
    outs = {k: e(torch.zeros(B, dtype=dt), "out_" + k) for k, dt in (("scores", f32), ("fin", i32), ("dead", i32), ("first", i32), ("prev", i32),
                                                                    ("parent", i32), ("next", i32))}
    ovis, orows = e(torch.zeros(B, fw, dtype=i32), "out_visited"), e(torch.zeros(B, S, dtype=torch.uint8), "mask_rows")
    nrows, nstats = e(torch.zeros(B, 64), "rows"), e(torch.zeros(B, 2, 2), "stats")
    p = lambda t: t.data_ptr()
    d = L_.BeamConstrainedStep(p(lg), S, S, p(mask), p(kv), 9, 4, GPW, p(fol), L, LOOPS, c["ntok"], c["term"][0], c["term"][1],
                               p(ins["scores"]), p(ins["fin"]), p(ins["dead"]), p(ins["first"]), p(ins["prev"]), p(vis),
                               p(outs["scores"]), p(outs["fin"]), p(outs["dead"]), p(outs["first"]), p(outs["prev"]), p(ovis), p(orows),
                               p(outs["parent"]), p(outs["next"]), p(mem), 64, p(nrows), 64, p(nstats), None)
    da = L_.BeamConstrainedAheadStep(d, MODES.BEAM_CLOSURES[closure], p(close) if closure == "lookahead" else None, p(cyc), budget)
    L_.check(hip_lib.ff_beam_constrained_select_ahead(C.byref(da), torch.cuda.current_stream().cuda_stream), "ff_beam_constrained_select_ahead")
    torch.cuda.synchronize()
    guard.check()
    for k in outs:
        assert torch.equal(outs[k], clean[k]), k
    assert torch.equal(ovis, clean["visited"]) and torch.equal(nrows, clean["rows"]) and torch.equal(nstats, clean["stats"])
    live = torch.from_numpy((c["scores"] > -np.inf) & (c["fin"] == 0)).cuda()
    assert torch.equal(orows[live], clean["mask_rows"][live])
    for k in ins:                                                        # the inputs are not written
        assert torch.equal(ins[k].cpu(), torch.from_numpy(c[k])), k
    assert torch.equal(vis.cpu(), _bits(c["visited"]).cpu())


@pytest.mark.gpu
def test_close_dist_of_a_wireframe_past_2_31_bytes(hip_lib):
    """close_dist as a far view (tests/farview.py): rows [wireframe, first] of a [NW * L, L] byte matrix whose last wireframes lie
    past 2^31 bytes; only the rows the launch may read hold values, everything else is poison (255: masked at every budget).  Two
    groups of two beams are live, one near and one far; each beam has its own first edge, so its own row of the table."""
    import farview as FV
    import redzone as RZ
    from faceformer_amd.hip import ops
    L, ntok, W = 1024, 4, 2
    S = L + ntok
    NW = (1 << 31) // (L * L) + 2                                                             # 2050 wireframes of 1 MiB each
    B, near, far_w = NW * W, 1, NW - 1
    assert far_w * L * L > (1 << 31)
    g0 = torch.Generator().manual_seed(28)
    first = torch.full((B,), -1, dtype=torch.int32)
    prev = torch.full((B,), -1, dtype=torch.int32)
    fin = torch.ones(B, dtype=torch.int32)                                                    # every beam finished but four
    scores = torch.zeros(B)
    rows_at, values, cases = [], [], []
    follows = torch.zeros(NW, L, (L + 31) // 32, dtype=torch.int32)
    for w, firsts, pv in ((near, (5, 6), 9), (far_w, (700, 701), 33)):
        follows[w, pv] = -1                                                                   # every edge follows prev
        for k, f in enumerate(firsts):
            b = w * W + k
            first[b], prev[b], fin[b] = f, pv, 0
            scores[b] = -float(k)
            rows_at.append(w * L + f)
            values.append(torch.randint(1, 9, (L,), generator=g0, dtype=torch.int64).to(torch.uint8))
            cases.append((b, w, values[-1]))
    rows_at.append(NW * L - 1)                                                                # (the matrix's last row, so that it has NW * L)
    values.append(torch.full((L,), 255, dtype=torch.uint8))
    matrix = FV.far_rows(torch.stack(values), rows_at, L, fill=RZ.POISON)
    close = matrix.view(NW, L, L)
    assert close.is_contiguous() and close.data_ptr() == matrix.data_ptr() and FV.farthest(matrix) > (1 << 31)
    cyc = torch.zeros(NW, L, dtype=torch.uint8)
    logits = torch.randn(B, S, generator=g0)
    visited = torch.zeros(B, (L + 31) // 32, dtype=torch.int32)
    budget = 4
    res = ops.beam_constrained_select_ahead(logits.clone().cuda(), scores.cuda(), fin.cuda(), torch.zeros(B, dtype=torch.int32).cuda(), first.cuda(),
                                            prev.cuda(), visited.cuda(), W, LOOPS, ntok, follows.cuda(), "lookahead", cyc.cuda(), budget,
                                            close_dist=close, groups_per_wireframe=1, term_range=(1, 4))
    FV.check_untouched(matrix, "close_dist")
    rows = res["mask_rows"].cpu().numpy() != 0
    for b, w, dist in cases:
        want = dist.numpy().astype(np.int64) > budget
        assert 0 < want.sum() < L
        assert rows[b, :ntok].all() and np.array_equal(rows[b, ntok:], want), b                # the far row was read, not a wrapped one
    nxt, par = res["next"].cpu().numpy(), res["parent"].cpu().numpy()
    for w in (near, far_w):
        for r in range(W):
            b = w * W + r
            assert not rows[w * W + par[b], nxt[b]] and not bool(res["dead"][b]), (w, r)


# ---- GPU: the engine ---------------------------------------------------------------------------------------------------------------------
ENGINE_GOLDENS = TCB.ENGINE_GOLDENS
_model, _decode, _beam_rows, _pad_of = TCB._model, TCB._decode, TCB._beam_rows, TCB._pad_of


def _tables(name):
    from test_lookahead import _tables as tables
    return tables(name)


def _closure(model, case, b, tables, closure, W, **kw):
    bits, close, cyc = tables
    return _decode(model, case, b, constrain=LOOPS, follow_table=bits, term_range=TERM, constrain_beams=W, constrain_beam_closure=closure,
                   close_dist=close if closure == "lookahead" else None, cycle_len=cyc, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_at_width_1_is_the_constrained_greedy_decode_of_the_form(hip_lib, name, closure):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T = case["model"]["seq_len"]
    bits, close, cyc = tables = _tables(name)
    kw = dict(constrain_lookahead=True, close_dist=close) if closure == "lookahead" else dict(constrain_exact=True)
    one = _decode(model, case, b, constrain=LOOPS, follow_table=bits, term_range=TERM, cycle_len=cyc, trace=True, **kw)
    out = _closure(model, case, b, tables, closure, 1)
    assert out["steps"] == one["steps"] and torch.equal(out["predict"], one["predict"]), (name, closure)
    assert torch.equal(out["beams"], one["predict"]) and torch.equal(out["beam_dead_end"], one["dead_end"]), (name, closure)
    tol = TCB._step_tols(one, T)
    lp = one["logprob"].cpu().numpy().astype(np.float64)
    used = (lp[:, 1:] != 0)
    bound = (used * (2 * tol + CR.LP_BAR)[None, :]).sum(axis=1)
    err = np.abs(out["beam_scores"].cpu().numpy().astype(np.float64) - lp.sum(axis=1))
    print(name, closure, "steps=%d max |score - sum logprob| = %.3g (bound %.3g)" % (out["steps"], err.max(), bound[err.argmax()]))
    assert (err <= bound + 1e-30).all(), (name, closure, err.max())
    assert "logprob" not in out and "dead_end" not in out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_with_zero_tables_is_the_plain_constrained_beam_decode(hip_lib, name):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    bits, close, cyc = _tables(name)
    W = 4
    plain = TCB._cbeam(model, case, b, LOOPS, W, table, trace=True)
    out = _closure(model, case, b, (bits, torch.zeros_like(close), torch.zeros_like(cyc)), "lookahead", W, trace=True)
    assert out["steps"] == plain["steps"]
    for k in ("predict", "beams", "beam_scores", "beam_dead_end", "beam_parent"):
        assert torch.equal(out[k], plain[k]), (name, k)
    assert torch.equal(out["logits"][: out["steps"]], plain["logits"][: out["steps"]]), name


def _replay(out, closure, table, tables, pad, F, W, T, what):
    """test_constrain_beam._replay under the form: the numpy rule carried along the decode's own traced logits (j x the bound at
    step j, budget T - 2 - j).  Returns (pairs, pairs left out, the groups replayed to the end, dead-end steps seen)."""
    logits = out["logits"].cpu().numpy()
    parent = out["beam_parent"].cpu().numpy()
    close, cyc = tables[1].cpu().numpy(), tables[2].cpu().numpy()
    steps = out["steps"]
    beams, scores, dead = _beam_rows(out, W, T)
    pairs = left = 0
    whole = []
    for gi in range(beams.shape[0]):
        w = gi // F
        tok0 = int(beams[gi, 0, 0])
        sc, fin, dd, sts = CL.start_group(tok0, W, NTOK, TERM, table[w])
        toks, pars, alive = [], [], True
        for j in range(steps):
            if fin[~np.isinf(sc)].all():
                break
            pairs += 1
            if not alive:
                left += 1
                continue
            res = CL.group_step(CL.FORMS[closure], logits[j, gi * W:(gi + 1) * W].astype(np.float64), pad[w], sc, fin, dd, sts, LOOPS, NTOK, TERM,
                                table[w], close[w], cyc[w], T - 2 - j, margin=j + 1)
            for k in range(W):
                if res["rows"][k] is not None:
                    assert np.array_equal(logits[j, gi * W + k] == np.float32(FILL), res["masked"][k] | pad[w]), (what, j, gi, k)
            if not res["gap"] > 1.0:
                alive = False
                left += 1
                continue
            assert np.array_equal(parent[j, gi * W:(gi + 1) * W], res["parent"]), (what, j, gi)
            toks.append(res["tok"]); pars.append(res["parent"])
            sc, fin, dd, sts = res["scores"], res["fin"], res["dead"], res["states"]
        if alive:
            whole.append(gi)
            n = len(toks)
            want = BR.backtrack(np.full(W, tok0), toks, pars, W)
            keep = ~np.isinf(sc)
            assert np.array_equal(beams[gi][:, : n + 1][keep], want[keep]), (what, gi)
            assert np.array_equal(dead[gi][keep], dd[keep]), (what, gi)
            assert (np.abs(scores[gi][keep] - sc[keep]) <= max(n, 1) * (BR.LP_BAR + BR.ADD_EPS * np.abs(sc[keep]))).all(), (what, gi)
    return pairs, left, whole


def _check_beams(out, closure, name, ni, edges, table, W, T):
    """Every final beam: no edge twice, scores non-increasing in k (empties last); under "exact" no late dead end and every
    non-empty, not dead beam that ends in a terminator passes faces.is_face_enclosed.  Returns (own-anchor groups whose best
    non-dead beam is enclosed, own-anchor groups)."""
    beams, scores, dead = _beam_rows(out, W, T)
    F = max(ni)
    assert torch.equal(out["predict"], out["beams"].reshape(-1, W, T)[:, 0])
    best = groups = 0
    for w, n in enumerate(ni):
        if closure == "exact":                                             # guarantee (d), on every back-tracked beam of the wireframe
            rows = beams[w * F:(w + 1) * F].reshape(-1, T)
            flags = dead[w * F:(w + 1) * F].reshape(-1) & ~np.isinf(scores[w * F:(w + 1) * F].reshape(-1))
            assert XR.late_dead_ends(rows, flags, NTOK, table[w]) == [], (name, w)
        for f in range(n):
            g = w * F + f
            groups += 1
            gsc = scores[g]
            fin_sc = gsc[~np.isinf(gsc)]
            assert (np.diff(fin_sc) <= 0).all() and not np.isinf(gsc[: fin_sc.size]).any(), (name, w, f, gsc)
            first_live = True
            for k in range(W):
                if np.isinf(gsc[k]):
                    continue
                row = beams[g, k]
                idx = [int(t) - NTOK for t in row if t >= NTOK]
                assert len(idx) == len(set(idx)), (name, w, f, k, row)
                if dead[g, k]:
                    continue
                ended = ((row >= TERM[0]) & (row < TERM[1])).any()
                face = faces._parallel_rows(row[None], TOK, n) if ended else []
                ok = bool(face) and bool(faces.is_face_enclosed(edges[w], face[0][1], CR.TOL))
                if closure == "exact" and ended and face:
                    assert ok, (name, w, f, k, row)
                if first_live:
                    best += ok
                    first_live = False
    return best, groups


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_replays_under_the_numpy_rule_and_its_beams_are_valid(hip_lib, name, closure):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, F, W = case["model"]["seq_len"], max(ni), 4
    tables = _tables(name)
    out = _closure(model, case, b, tables, closure, W, trace=True)
    pairs, left, _ = _replay(out, closure, table, tables, _pad_of(b), F, W, T, (name, closure))
    best, groups = _check_beams(out, closure, name, ni, edges, table, W, T)
    print(name, closure, "steps=%d: %d (step, group) pairs, %d left out (%.2f %%); best non-dead beam enclosed in %d of %d own-anchor groups, "
          "%d dead-ended beams" % (out["steps"], pairs, left, 100.0 * left / max(1, pairs), best, groups, int(out["beam_dead_end"].sum())))
    assert pairs > 0 and left <= CL.CAP * pairs, (name, closure, left, pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_enough_groups_end_enclosed_under_the_exact_form(hip_lib, name):
    """Non-vacuity: at W = 4 under "exact", at least half of the fp64 oracle's own count of own-anchor groups whose best non-dead
    beam is enclosed (constrain_beam_closure_ref.ORACLE_W4, fixed on the CPU); on the STRICT fixtures strictly more than under
    the plain constrain_beams decode."""
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, W = case["model"]["seq_len"], 4
    tables = _tables(name)
    groups, o_plain, o_ahead, o_exact = CL.ORACLE_W4[name]
    got = {}
    for closure in ("plain",) + CLOSURES:
        out = TCB._cbeam(model, case, b, LOOPS, W, table) if closure == "plain" else _closure(model, case, b, tables, closure, W)
        got[closure], n = _check_beams(out, closure, name, ni, edges, table, W, T)
        assert n == groups
    print(name, "W=4 own-anchor groups with an enclosed best beam: plain %d, lookahead %d, exact %d of %d (oracle: %d, %d, %d)"
          % (got["plain"], got["lookahead"], got["exact"], groups, o_plain, o_ahead, o_exact))
    assert o_exact > 0 and 2 * got["exact"] >= o_exact, (name, got, o_exact)
    if name in CL.STRICT:
        assert got["exact"] > got["plain"], (name, got)


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
def test_plan_invariance_and_repeatability(hip_lib, closure):
    name = "par_small_ragged"
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T, F, W = case["model"]["seq_len"], max(lat["num_input"]), 4
    tables = _tables(name)
    whole = _closure(model, case, b, tables, closure, W, trace=True, chunk_wireframes=0)
    again = _closure(model, case, b, tables, closure, W, trace=True, chunk_wireframes=0)
    for k in ("predict", "beams", "beam_scores", "beam_dead_end", "beam_parent"):
        assert torch.equal(whole[k], again[k]), k                        # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"]
    one = _closure(model, case, b, tables, closure, W, trace=True, chunk_wireframes=1)      # (the tables offset per chunk)
    pad = _pad_of(b)
    pw, lw, gw = _replay(whole, closure, table, tables, pad, F, W, T, "whole")
    po, lo, go = _replay(one, closure, table, tables, pad, F, W, T, "one")
    both = sorted(set(gw) & set(go))                                     # the groups decisive to the end under both plans
    assert lw <= CL.CAP * pw and lo <= CL.CAP * po and both
    bw, sw, dw = _beam_rows(whole, W, T)
    bo, so, do = _beam_rows(one, W, T)
    assert np.array_equal(bw[both], bo[both]) and np.array_equal(dw[both], do[both])
    fi = ~np.isinf(sw[both])
    assert np.array_equal(fi, ~np.isinf(so[both]))
    n = max(whole["steps"], 1)
    assert (np.abs(sw[both][fi] - so[both][fi]) <= 2 * n * (BR.LP_BAR + BR.ADD_EPS * np.abs(sw[both][fi].astype(np.float64)))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib, closure):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "par_small_ragged"
    m = WP._bound(name, "default")
    b, table = WP._lattice(m)
    tables = _tables(name)
    call = lambda: _closure(m.model, m.case, b, tables, closure, 4, trace=True)
    clean = call()
    clean.pop("engine", None)
    zero, d = WP._run([m], call, fill=RZ.ZERO, what=closure + " after ZERO")
    poison, _ = WP._run([m], call, fill=RZ.POISON, what=closure + " after POISON")
    WP._assert_equal(poison, zero, closure)
    WP._assert_equal(poison, clean, closure + " against the clean run")
    assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size


@pytest.mark.gpu
def test_workspace_query_is_the_constrained_beam_decodes(hip_lib):
    from faceformer_amd.hip import lib
    m, prm = lib.Model(), lib.DecodeParams()
    m.num_token, m.E, m.H, m.FF, m.num_dec_layers = 4, 64, 1, 64, 1
    prm.variant, prm.N, prm.L, prm.F, prm.T, prm.term_lo, prm.term_hi = lib.FF_PARALLEL, 3, 8, 8, 9, 1, 4
    for W in (1, 4, 8):
        a = hip_lib.ff_decode_constrained_beam_ahead_workspace_bytes(C.byref(m), C.byref(prm), None, W)
        assert a > 0 and a == hip_lib.ff_decode_constrained_beam_workspace_bytes(C.byref(m), C.byref(prm), None, W)


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
@pytest.mark.parametrize("form", ["f32", "fp16x2", "no_l0_fold", "drained", "two_streams"])
def test_replay_under_the_launch_forms(hip_lib, form, closure):
    import test_mode_forms as MF
    name = "par_small_ragged"
    assert form in MF.FORMS
    m = MF._bound(name, form)
    lat, b, table = MF._lattice(name)
    tables = _tables(name)
    call = lambda bound: _closure(bound.model, bound.case, b, tables, closure, 4, trace=True, num_streams=bound.model.num_streams)
    with MF._tuned(form):
        out = call(m)
        MF._check_bit_equal(m, lambda bound: {k: v for k, v in call(bound).items() if k != "engine"}, m.what)
    F = max(lat["num_input"])
    pairs, left, _ = _replay(out, closure, table, tables, _pad_of(b), F, 4, m.T, m.what)
    print("%s %s %s: steps %d, %d pairs replayed, %d left out" % (closure, name, form, out["steps"], pairs, left))
    assert pairs > 0 and left <= CL.CAP * pairs


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
def test_model_keys_in_batch_order_tables_faces_and_option_off(hip_lib, closure):
    case, z, model, gb, sd, lat, b, edges, table = _model("par_small_ragged")
    T, W = case["model"]["seq_len"], 3
    ni = lat["num_input"]
    N, F = len(ni), max(ni)
    order = sorted(range(N), key=lambda i: -ni[i])
    assert order != list(range(N))                                   # the premise: the model does reorder this batch
    idx = torch.tensor(order, device="cuda")
    by_hand = {k: (v.index_select(0, idx) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in b.items()}
    by_hand["num_input"] = [ni[i] for i in order]
    bits, close, cyc = _tables("par_small_ragged")
    assert model.constrain_beam_closure is None
    try:
        with torch.no_grad():
            off = model(dict(b))
            model.constrain, model.constrain_beams = "loops", W
            plain = model(dict(b))
            model.constrain_beam_closure = closure
            on = model(dict(b))
            given = model(dict(b, close_dist=close, cycle_len=cyc) if closure == "lookahead" else dict(b, cycle_len=cyc))
            model.extract_faces = "enclosed"
            faced = model(dict(b))
            model.extract_faces = False
            model.constrain_beams = 1
            one = model(dict(b))
            model.constrain_beams, model.constrain_beam_closure = 0, None
            setattr(model, "constrain_lookahead" if closure == "lookahead" else "constrain_exact", True)
            greedy = model(dict(b))
            model.constrain_lookahead = model.constrain_exact = False
            model.constrain_beams, model.constrain_beam_closure, model.sort_by_edges = W, closure, False
            hand = model(dict(by_hand))
    finally:
        model.constrain, model.constrain_beams, model.constrain_beam_closure, model.sort_by_edges = None, 0, None, True
        model.constrain_lookahead = model.constrain_exact = model.extract_faces = False
    new = {"predict_beams", "predict_beam_scores", "predict_beam_dead_end", "predict_dead_end"}
    assert set(on) == set(plain) == set(off) | new and "predict_logprob" not in on           # the published keys are constrain_beams'
    assert tuple(on["predict_beams"].shape) == (N, F, W, T) and tuple(on["predict_beam_scores"].shape) == (N, F, W)
    assert torch.equal(on["predict"], on["predict_beams"][:, :, 0]) and torch.equal(on["predict_dead_end"], on["predict_beam_dead_end"][:, :, 0])
    for k in new | {"predict"}:
        assert torch.equal(on[k].index_select(0, idx), hand[k]), k       # batch order: the sort undone, the tables permuted with it
        assert torch.equal(on[k], given[k]), k                           # the built tables are the given ones
    assert not torch.equal(on["predict_beams"], plain["predict_beams"])                      # the form changes the search on this fixture
    assert torch.equal(one["predict"], greedy["predict"]) and torch.equal(one["predict_dead_end"], greedy["predict_dead_end"])
    assert model.last_decode_stats["constrain_beams"] == W
    # the device-side faces: ops.face_rows / face_votes of the published beams, held to the numpy restatements
    assert set(faced) == set(on) | {"faces"} and all(torch.equal(faced[k], on[k]) for k in new | {"predict"})
    import test_face_extract as TFE
    want = TFE._expected_faces(on, ni, faces.pack_follow_bits(table), "enclosed", case["model"]["L"])
    for k, v in want.items():
        got = faced["faces"][k].cpu().numpy()
        assert got.shape == v.shape and got.tobytes() == v.tobytes(), k
    assert int(want["num_faces"].sum()) > 0
    with torch.no_grad():
        again = model(dict(b))
    assert torch.equal(again["predict"], off["predict"]) and set(again) == set(off)      # option off again: no key is added


@pytest.mark.gpu
@pytest.mark.parametrize("closure", CLOSURES)
def test_cli_records_with_and_without_device_faces(hip_lib, tmp_path, closure):
    """The CLI on the cli_coedge_case.json set-up: the records gain pred_beam_faces / pred_beam_face_scores, and --device-faces
    gives identical text."""
    import test_face_extract as TFE
    cli = _cli()
    name, cfg, ckpt = TFE._cli_setups(tmp_path)[0]
    assert name == "coedge"
    kw = dict(constrain="loops", constrain_beams=3)
    texts = {}
    for device_faces in (False, True):
        out_dir = cli.run_test(cfg, ckpt, out_dir=str(tmp_path / ("d%d" % device_faces)), batch_size=2, device_faces=device_faces,
                               constrain_beam_closure=closure, **kw)
        texts[device_faces] = {n: open(os.path.join(out_dir, n)).read() for n in sorted(os.listdir(out_dir))}
    assert texts[False] == texts[True] and len(texts[False]) >= 2
    plain_dir = cli.run_test(cfg, ckpt, out_dir=str(tmp_path / "plain"), batch_size=2, **kw)
    for n, text in texts[False].items():
        rec, plain = json.loads(text), json.loads(open(os.path.join(plain_dir, n)).read())
        assert list(rec) == list(plain) and "pred_beam_faces" in rec and "pred_beam_face_scores" in rec and "pred_dead_ends" in rec
