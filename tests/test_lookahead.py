"""Opt-in closure look-ahead of the loop-constrained pointer decode: the numpy rule (tests/lookahead_ref.py, composed
from constrain_ref) on hand-written rows, faces.follow_distance against a brute-force walk, the C ABI, the bindings, every
rejected combination and the CLI on the CPU; ff_follow_distance, ff_pointer_constrained_ahead and the engine's seventh mode against
that rule on the GPU.

Bars (the issue's, none measured): distances, byte rows, FILL patterns, tokens, flags and next states are exact;
log-probabilities within 2^-16 of fp64 log_softmax of the kernel's own masked row (DESIGN.md 12's bar); with both tables zero
every output is bit-equal to the "loops" decode; traced logits within test_parity_golden._tol of the fp64 oracle teacher-forced
along the decode's tokens, at most 2 % of the pairs left out; at least 35 % of the own-anchor rows of every lattice fixture end
enclosed (a condition on the fixtures: tools/lookahead_left_out.py)."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
import lookahead_ref as LR
from conftest import GOLDEN, ROOT, token_ns
from faceformer_amd import faces
from test_constrain import _tiny_inputs, _tiny_model, _untouchable

TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
NTOK = TOK.len
FILL = CR.FILL
LOOPS = CR.NO_REPEAT | CR.CONNECT
NEW_ENTRIES = ("ff_follow_distance", "ff_pointer_constrained_ahead", "ff_decode_constrained_ahead_workspace_bytes",
               "ff_decode_constrained_ahead")


# ---- CPU: the rule ----------------------------------------------------------------------------------------------------------------
def test_rule_on_hand_written_rows():
    ring, chain = LR.ring(4), LR.chain(4)
    S = NTOK + 4
    pad = np.zeros(S, dtype=bool)
    raw = np.arange(S, dtype=np.float64)                       # the last edge carries the largest logit
    rc, rl = faces.follow_distance(ring)
    assert rc.tolist() == [[4, 3, 2, 1], [1, 4, 3, 2], [2, 1, 4, 3], [3, 2, 1, 4]] and rl.tolist() == [4, 4, 4, 4]
    cc, cl = faces.follow_distance(chain)
    assert cl.tolist() == [255] * 4                            # the chain has no cycle
    assert cc.tolist() == [[255] * 4, [1, 255, 255, 255], [2, 1, 255, 255], [3, 2, 1, 255]]
    step = lambda st, f, c, l, budget, **kw: LR.step_row(raw, pad, st, LOOPS, NTOK, TERM, f, c, l, budget, **kw)
    # the ring, open after edge 0: edge 1 closes the loop three edges later, so the terminator needs budget >= 3
    st = CR.start_state(NTOK + 0, NTOK, ring)
    assert st == (frozenset({0}), 0, 0)
    r = step(st, ring, rc, rl, 3)
    assert r["masked"].tolist() == [True] * NTOK + [True, False, True, True] and r["tok"] == NTOK + 1 and not r["dead"]
    d = step(st, ring, rc, rl, 2)                              # one position short: a dead end, the terminators instead
    assert d["dead"] and d["fin"] and d["tok"] == TERM[1] - 1 and d["masked"].tolist() == [True] + [False] * 3 + [True] * 4
    # ... one edge before the closure the last edge needs budget 1 (itself, then the terminator)
    st3 = CR.state_of_prefix([NTOK + 0, NTOK + 1, NTOK + 2], NTOK, ring)
    assert st3 == (frozenset({0, 1, 2}), 0, 2)
    assert step(st3, ring, rc, rl, 1)["tok"] == NTOK + 3 and step(st3, ring, rc, rl, 1)["state"] == (frozenset({0, 1, 2, 3}), None, 3)
    # an open loop at budget 0 is a dead end, on the ring and on the chain: every edge is masked
    for table, c, l in ((ring, rc, rl), (chain, cc, cl)):
        o = step(CR.start_state(NTOK + 0, NTOK, table), table, c, l, 0)
        assert o["dead"] and o["fin"] and o["masked"][NTOK:].all() and TERM[0] <= o["tok"] < TERM[1]
    # a closed loop at budget 0 selects a terminator and is no dead end; with budget 3 the ring still cannot start (cycle 4)
    closed = (frozenset(), None, None)
    for budget in (0, 3):
        o = step(closed, ring, rc, rl, budget)
        assert not o["dead"] and o["fin"] and o["masked"].tolist() == [True] + [False] * 3 + [True] * 4 and o["tok"] == TERM[1] - 1
    o = step(closed, ring, rc, rl, 4)
    assert o["tok"] == NTOK + 3 and not o["fin"] and o["masked"].tolist() == [True] + [False] * 7
    # the chain never closes: with the loop closed no edge starts one at any budget, with it open every step is a dead end
    o = step(closed, chain, cc, cl, 254)
    assert o["masked"][NTOK:].all() and not o["dead"] and o["fin"]
    assert step(CR.start_state(NTOK + 0, NTOK, chain), chain, cc, cl, 254)["dead"]
    # NO_REPEAT alone reads no table, a finished row is constrain_ref's
    n = LR.step_row(raw, pad, st, CR.NO_REPEAT, NTOK, TERM, ring, rc, rl, 0)
    assert n["masked"].tolist() == [False] * NTOK + [True, False, False, False] and n["tok"] == NTOK + 3
    assert LR.step_row(raw, pad, st, LOOPS, NTOK, TERM, ring, rc, rl, 0, finished=True)["tok"] == 0


def test_numpy_follow_distance_against_a_brute_force_walk():
    assert "follow_distance" in faces.__all__
    cases = [("ring", LR.ring(9)), ("ring of 5 among 9", LR.ring(9, 5)), ("chain", LR.chain(9)), ("empty", np.zeros((6, 6), dtype=bool)),
             ("one edge", LR.ring(1)), ("one open edge", np.zeros((1, 1), dtype=bool))]
    own = LR.chain(7)
    own[3, 3] = own[6, 6] = True                                # self-closing edges inside and at the end of a chain
    cases.append(("self-closing", own))
    for L in (2, 33, 70):
        cases += [("random %d/%d" % (L, w), t) for w, t in enumerate(CR.random_follows(2, L, L))]
    for what, t in cases:
        L = t.shape[0]
        for hmax in (254, 3, 1):
            for n in (None, max(L - 2, 0), 1, 0):
                got = faces.follow_distance(t, hmax, n)
                want = LR.brute_distance(t, hmax, n)
                assert got[0].dtype == got[1].dtype == np.uint8 and got[0].shape == (L, L) and got[1].shape == (L,)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, hmax, n)
                assert np.array_equal(np.diagonal(got[0]), got[1])
    close, cyc = faces.follow_distance(own)
    assert cyc.tolist() == [255, 255, 255, 1, 255, 255, 1] and close[3, 3] == 1 and close[6, 0] == 6
    # saturation: a ring longer than hmax
    close, cyc = faces.follow_distance(LR.ring(9), 8)
    assert (cyc == 255).all() and close.max() == 255 and sorted(set(close.ravel().tolist())) == list(range(1, 9)) + [255]
    # batched tables with one count per leading index
    t = CR.random_follows(3, 12, 1)
    close, cyc = faces.follow_distance(t, 5, [12, 7, 0])
    for w, n in enumerate((12, 7, 0)):
        want = LR.brute_distance(t[w], 5, n)
        assert np.array_equal(close[w], want[0]) and np.array_equal(cyc[w], want[1])
    assert (close[2] == 255).all() and (close[1, 7:] == 255).all() and (close[1, :, 7:] == 255).all()
    for bad in (0, 255, True, 1.5):
        with pytest.raises(ValueError, match="hmax"):
            faces.follow_distance(LR.ring(3), bad)
    empty = faces.follow_distance(np.zeros((2, 0, 0), dtype=bool))
    assert empty[0].shape == (2, 0, 0) and empty[1].shape == (2, 0)


def test_reference_with_zero_tables_is_the_constrain_reference():
    rng = np.random.default_rng(3)
    L = 11
    S = NTOK + L
    follows = CR.random_follows(1, L, 9)[0]
    zc, zl = np.zeros((L, L), dtype=np.uint8), np.zeros(L, dtype=np.uint8)
    for trial in range(60):
        raw = rng.normal(size=S) * 3
        pad = rng.random(S) < 0.2
        pad[:NTOK] = False
        visited = frozenset(np.flatnonzero(rng.random(L) < 0.3).tolist())
        first = None if trial % 3 == 0 else int(rng.integers(0, L))
        prev = None if trial % 5 == 0 else int(rng.integers(0, L))
        for flags in (0, CR.NO_REPEAT, CR.CONNECT, LOOPS):
            for budget in (0, 1, 254):
                a = LR.step_row(raw, pad, (visited, first, prev), flags, NTOK, TERM, follows, zc, zl, budget)
                b = CR.step_row(raw, pad, (visited, first, prev), flags, NTOK, TERM, follows)
                assert set(a) == set(b)
                for k in a:
                    assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], (trial, flags, budget, k)


# ---- CPU: C ABI and binding -------------------------------------------------------------------------------------------------------
def test_header_declares_the_lookahead_entries_within_abi_105():
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    doc = header[header.index("closure look-ahead for the loop-constrained pointer decode"): header.index("int ff_follow_distance(")]
    for phrase in ("D(a->a) is the length of the shortest cycle through a", "Stored as uint8", "1 <= hmax <= 254",
                   "close_dist[w][f][b] = D(b->f)", "cycle_len[w][b] = D(b->b)", "budget = T - 1 - p",
                   "close_dist[w][first][b] > budget", "cycle_len[w][b] > budget", "The dead-end vote runs after these masks",
                   "necessary, not sufficient", "With both tables all zero", "T > 256"):
        assert phrase in doc, phrase
    assert re.search(r"typedef struct ff_constrain_ahead_params \{\s*int flags;\s*const unsigned int\* follows;\s*"
                     r"const unsigned char\* close_dist;\s*const unsigned char\* cycle_len;\s*float\* logprob;\s*int\* dead_end;\s*\} "
                     r"ff_constrain_ahead_params;", code)
    assert re.search(r"#define\s+FF_CONSTRAIN_NO_REPEAT\s+1\b", code) and re.search(r"#define\s+FF_CONSTRAIN_CONNECT\s+2\b", code)
    assert not re.search(r"#define\s+FF_CONSTRAIN_\w+\s+4\b", code)                          # no new flag bit

    def args(name):
        return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert args("ff_decode_constrained_ahead").count(",") == args("ff_decode_constrained").count(",")
    assert "const ff_constrain_ahead_params* ahead" in args("ff_decode_constrained_ahead")
    assert args("ff_decode_constrained_ahead_workspace_bytes") == args("ff_decode_constrained_workspace_bytes")
    assert args("ff_pointer_constrained_ahead").count(",") == args("ff_pointer_constrained").count(",") + 3
    tail = [a.strip() for a in args("ff_pointer_constrained_ahead").split(",")[-4:]]
    assert tail == ["const unsigned char* close_dist", "const unsigned char* cycle_len", "int budget", "ff_stream_t stream"]
    assert [a.strip().split()[-1].lstrip("*") for a in args("ff_follow_distance").split(",")] == [
        "follows", "N", "L", "num_input", "hmax", "close_dist", "cycle_len", "stream"]
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", src, flags=re.M)      # no preprocessor conditionals
    assert "template <bool AHEAD>" in src and "pointer_constrained_kernel<false>" in src and "pointer_constrained_kernel<true>" in src
    assert "follow_distance_kernel" in src


def test_binding_lists_the_lookahead_entries_and_refuses_a_library_without_them(monkeypatch):
    from faceformer_amd.hip import lib, modes
    assert lib.FF_ABI_VERSION == 105
    S = lib.SIGNATURES
    for name in NEW_ENTRIES:
        assert name in S, name
    assert len(S["ff_decode_constrained_ahead"][1]) == len(S["ff_decode_constrained"][1])
    assert S["ff_decode_constrained_ahead_workspace_bytes"] == S["ff_decode_constrained_workspace_bytes"]
    assert S["ff_pointer_constrained_ahead"][1][:-1] == S["ff_pointer_constrained"][1][:-1] + [lib.fptr, lib.fptr, lib.C.c_int]
    assert len(S["ff_follow_distance"][1]) == 8
    assert [f for f, _ in lib.ConstrainAheadParams._fields_] == ["flags", "follows", "close_dist", "cycle_len", "logprob", "dead_end"]
    assert (lib.FF_CONSTRAIN_NO_REPEAT, lib.FF_CONSTRAIN_CONNECT) == (1, 2)
    rec = modes.CONSTRAIN_AHEAD
    assert rec not in modes.MODES and rec.entry == "ff_decode_constrained_ahead" and rec.subject == "constrain_lookahead"
    assert rec.excludes == modes.CONSTRAIN.excludes and rec.outs == modes.CONSTRAIN.outs and rec.switches == modes.CONSTRAIN.switches
    assert [n for n, _ in rec.own] == ["follow_table", "close_dist", "cycle_len"] and not rec.per_anchor
    assert modes.of_options(False, 0, True, constrain=LOOPS, num_samples=0, beam_width=0) == (rec, LOOPS)
    assert modes.of_options(False, 0, False, constrain=LOOPS, num_samples=0, beam_width=0) == (modes.CONSTRAIN, LOOPS)
    assert modes.of_options(False, 0, constrain=LOOPS, num_samples=0, beam_width=0) == (modes.CONSTRAIN, LOOPS)
    import _ctypes
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


def test_a_library_without_only_the_new_entries_is_refused(monkeypatch):
    """The parent's library exports everything but the four new entries: load() names the first one it misses."""
    from faceformer_amd.hip import lib

    class Old:
        def __getattr__(self, name):
            if name in NEW_ENTRIES:
                raise AttributeError(name)
            return types.SimpleNamespace(restype=None, argtypes=None)
    monkeypatch.setattr(lib.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="does not export ff_follow_distance .*rebuild"):
        lib.load()


def test_c_entries_reject_bad_arguments_before_any_launch(hip_lib):
    """FF_ERR_ARG with the offending argument named, on a host without a GPU: the checks run in front of every HIP call."""
    import ctypes as C
    from faceformer_amd.hip import lib
    FF_ERR_ARG = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for hmax in (0, 255, -1):
        assert hip_lib.ff_follow_distance(p, 1, 4, p, hmax, p, p, None) == FF_ERR_ARG and b"hmax" in hip_lib.ff_last_error()
    assert hip_lib.ff_follow_distance(None, 1, 4, p, 3, p, p, None) == FF_ERR_ARG
    assert hip_lib.ff_follow_distance(p, 1, 8193, p, 3, p, p, None) == FF_ERR_ARG and b"8192" in hip_lib.ff_last_error()
    assert hip_lib.ff_follow_distance(p, 0, 4, p, 3, p, p, None) == 0                       # an empty problem is a no-op

    def step(flags=LOOPS, close=p, cyc=p, budget=3):
        return hip_lib.ff_pointer_constrained_ahead(p, 8, 8, None, None, 2, 1, p, 4, flags, 4, 1, 4, p, p, p, p, p, p, p, p, p, p, p,
                                                    None, 0, None, 0, None, None, close, cyc, budget, None)
    for kw, text in ((dict(flags=CR.NO_REPEAT), b"FF_CONSTRAIN_CONNECT"), (dict(close=None), b"close_dist"), (dict(cyc=None), b"cycle_len"),
                     (dict(budget=-1), b"budget"), (dict(budget=255), b"budget"), (dict(flags=4 | LOOPS), b"unknown flag bits")):
        assert step(**kw) == FF_ERR_ARG and text in hip_lib.ff_last_error(), kw
        assert b"ff_pointer_constrained_ahead" in hip_lib.ff_last_error()
    m, prm = lib.Model(), lib.DecodeParams()
    m.num_token = 4
    prm.variant, prm.N, prm.L, prm.F, prm.T, prm.term_lo, prm.term_hi = lib.FF_PARALLEL, 1, 4, 4, 6, 1, 4

    def decode(prm=prm, extra=None, best=None, **fields):
        a = lib.ConstrainAheadParams(LOOPS, p, p, p, p, p)
        for k, v in fields.items():
            setattr(a, k, v)
        return hip_lib.ff_decode_constrained_ahead(C.byref(m), C.byref(prm), p, p, p, p, None, extra, p, None, None, None, None, best,
                                                   None, p, p, 1024, C.byref(a), None)
    for fields, text in ((dict(flags=CR.NO_REPEAT), b"FF_CONSTRAIN_CONNECT"), (dict(flags=0), b"FF_CONSTRAIN_CONNECT"),
                         (dict(flags=4 | LOOPS), b"unknown flag bits"), (dict(follows=None), b"follow table"),
                         (dict(close_dist=None), b"close_dist"), (dict(cycle_len=None), b"cycle_len"),
                         (dict(logprob=None), b"logprob and dead_end"), (dict(dead_end=None), b"logprob and dead_end"),
                         (dict(extra=p), b"extra mask"), (dict(best=p), b"best / second")):
        assert decode(**fields) == FF_ERR_ARG and text in hip_lib.ff_last_error(), fields
        assert b"ff_decode_constrained_ahead" in hip_lib.ff_last_error()

    def changed(**kw):
        q = lib.DecodeParams()
        C.memmove(C.byref(q), C.byref(prm), C.sizeof(prm))
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    for kw, text in ((dict(T=257), b"T=257"), (dict(variant=lib.FF_SEQ2SEQ), b"parallel-variant"),
                     (dict(flags=lib.FF_RETIRE_FINISHED), b"excludes"), (dict(flags=lib.FF_RETURN_POINTER), b"excludes"),
                     (dict(flags=lib.FF_NO_STOP), b"excludes"), (dict(term_lo=4), b"terminator range"), (dict(term_hi=5), b"terminator range")):
        assert decode(prm=changed(**kw)) == FF_ERR_ARG and text in hip_lib.ff_last_error(), kw
    assert hip_lib.ff_decode_constrained_ahead(None, None, p, p, p, p, None, None, p, None, None, None, None, None, None, p, p, 1024,
                                               None, None) == FF_ERR_ARG


def test_every_rejected_combination_raises_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine, modes
    lib = _untouchable(monkeypatch)
    assert modes.constrain_lookahead_value(False, None) is False and modes.constrain_lookahead_value(None, LOOPS, 4) is False
    assert modes.constrain_lookahead_value(True, LOOPS) is True and modes.constrain_lookahead_value(True, CR.CONNECT) is True
    with pytest.raises(ValueError, match="constrain_lookahead needs constrain='loops': it is the closure look-ahead"):
        modes.constrain_lookahead_value(True, None)
    for flags in (0, CR.NO_REPEAT):
        with pytest.raises(ValueError, match="constrain_lookahead needs constrain='loops' \\(FF_CONSTRAIN_CONNECT\\)"):
            modes.constrain_lookahead_value(True, flags)
    with pytest.raises(ValueError, match="constrain_lookahead excludes constrain_beams"):
        modes.constrain_lookahead_value(True, LOOPS, 2)
    # PathEngine.decode itself, on an engine object without a constructor call: nothing of it may be needed
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    table = torch.zeros(2, 8, 1, dtype=torch.int32)
    close, cyc = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.uint8)
    ok = dict(T=5, F=4, num_input=[4, 3], constrain="loops", term_range=TERM, follow_table=table, constrain_lookahead=True,
              close_dist=close, cycle_len=cyc)
    decode = lambda **change: eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, **change))
    for change, text in (
            (dict(constrain=None), "constrain_lookahead needs constrain='loops': it is the closure look-ahead"),
            (dict(constrain="no_repeat"), "constrain_lookahead needs constrain='loops' \\(FF_CONSTRAIN_CONNECT\\)"),
            (dict(constrain=0), "constrain_lookahead needs constrain='loops' \\(FF_CONSTRAIN_CONNECT\\)"),
            (dict(constrain_beams=2), "constrain_lookahead excludes constrain_beams"),
            (dict(close_dist=None), "constrain_lookahead needs close_dist and cycle_len"),
            (dict(cycle_len=None), "constrain_lookahead needs close_dist and cycle_len"),
            (dict(follow_table=None), "constrain='loops' needs follow_table"),
            (dict(T=257), "constrain_lookahead takes T <= 256 \\(got 257\\)"),
            (dict(close_dist=torch.zeros(2, 8, 7, dtype=torch.uint8)), "close_dist must be a uint8 tensor of shape \\[2, 8, 8\\]"),
            (dict(close_dist=torch.zeros(1, 8, 8, dtype=torch.uint8)), "close_dist must be a uint8 tensor of shape \\[2, 8, 8\\]"),
            (dict(close_dist=torch.zeros(2, 8, 8, dtype=torch.int32)), "close_dist must be a uint8 tensor of shape \\[2, 8, 8\\]"),
            (dict(close_dist=close.numpy()), "close_dist must be a uint8 tensor of shape \\[2, 8, 8\\]"),
            (dict(cycle_len=torch.zeros(2, 9, dtype=torch.uint8)), "cycle_len must be a uint8 tensor of shape \\[2, 8\\]"),
            (dict(cycle_len=torch.zeros(2, 8, dtype=torch.int8)), "cycle_len must be a uint8 tensor of shape \\[2, 8\\]"),
            (dict(follow_table=torch.zeros(2, 8, 2, dtype=torch.int32)), "follow_table must be an int32 tensor of shape \\[2, 8, 1\\]"),
            # everything the constrained decode excludes, in its record's words
            (dict(retire=True), "constrain_lookahead excludes retire, "), (dict(return_pointer=True), "constrain_lookahead excludes"),
            (dict(no_stop=True), "constrain_lookahead excludes"), (dict(stop_callback=lambda c: False), "constrain_lookahead excludes"),
            (dict(extra_mask=torch.zeros(8, 12, dtype=torch.uint8)), "constrain_lookahead excludes"),
            (dict(logprob=True), "constrain_lookahead excludes"), (dict(beam_width=2), "beam_width and num_samples"),
            (dict(num_samples=2, uniforms=torch.zeros(4, 16)), "beam_width and num_samples"),
            (dict(term_range=None), "constrain_lookahead needs term_range"), (dict(term_range=(4, 4)), "constrain_lookahead needs term_range")):
        with pytest.raises(ValueError, match=text):
            decode(**change)
    with pytest.raises(ValueError, match="constrain_lookahead is a parallel-variant option"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **ok)
    with pytest.raises(ValueError, match="constrain=4"):                                     # no new flag bit
        decode(constrain=4)
    # the ops wrapper's own checks
    from faceformer_amd.hip import ops
    for bad in (0, 255, True, 2.0):
        with pytest.raises(ValueError, match="hmax"):
            ops.follow_distance(torch.zeros(1, 4, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), bad)


def test_models_reject_lookahead_combinations_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        assert not model.engine_supported() and model.constrain_lookahead is False
        model.constrain, model.constrain_lookahead = "loops", True
        inputs = _tiny_inputs()
        with torch.no_grad(), pytest.raises(ValueError, match="constrain needs the native engine"):
            model.forward_eval(inputs)
        assert "predict" not in inputs
    model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert model.constrain_lookahead is False and type(model.constrain_lookahead) is bool
    model.constrain_lookahead = True
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_lookahead needs constrain='loops': it is the closure look-ahead"):
        model.forward_eval(_tiny_inputs())
    model.constrain = "no_repeat"
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_lookahead needs constrain='loops' \\(FF_CONSTRAIN_CONNECT\\)"):
        model.forward_eval(_tiny_inputs())
    model.constrain, model.constrain_beams = "loops", 2
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_lookahead excludes constrain_beams"):
        model.forward_eval(_tiny_inputs())
    model.constrain_beams = 0
    for attr, val in (("retire_finished", True), ("beam_width", 2), ("num_samples", 2), ("return_logprob", True)):
        old = getattr(model, attr)
        setattr(model, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="constrain excludes"):
            model.forward_eval(_tiny_inputs())
        setattr(model, attr, old)
    with torch.no_grad(), pytest.raises(ValueError, match="constrain excludes"):
        model.forward_eval(dict(_tiny_inputs(), extra_mask=torch.zeros(1, 4, 8, dtype=torch.bool)))
    long = _tiny_model(SurfaceFormer_Parallel, max_face_length=257)
    long.constrain, long.constrain_lookahead = "loops", True
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_lookahead takes T <= 256 \\(got 257\\)"):
        long.forward_eval(_tiny_inputs())
    with pytest.raises(ValueError, match="score\\(\\) excludes constrain"):
        model.score(_tiny_inputs(), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.constrain_lookahead is False
    seq.constrain_lookahead = True
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_lookahead is a SurfaceFormer_Parallel option"):
        seq.forward_eval({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})


def test_decode_sharded_rejects_lookahead_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain="loops",
                                  constrain_lookahead=True)
    with pytest.raises(ValueError, match="decode_sharded does not implement constrain_lookahead"):
        dist.decode_sharded(model, {}, NoDist())
    model.constrain = None                                         # (the option alone is an error anywhere)
    with pytest.raises(ValueError, match="decode_sharded does not implement constrain_lookahead"):
        dist.decode_sharded(model, {}, NoDist())
    model.constrain_lookahead = False
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


def test_cli_lookahead_flag_reaches_the_model_and_the_record_is_todays_without_it(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd import datasets as D
    parse = cli.build_parser().parse_args
    assert parse(["--test_ckpt", "x.ckpt", "--constrain", "loops", "--constrain-lookahead"]).constrain_lookahead is True
    assert parse(["--test_ckpt", "x.ckpt", "--constrain", "loops"]).constrain_lookahead is False
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--constrain", "loops", "--constrain-lookahead", "--test_ckpt", "unused.ckpt"])
    cli.main(["--constrain", "loops", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["constrain"], kw["constrain_lookahead"]) for kw in seen] == [("loops", True), ("loops", False), (None, False)]
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3, constrain_lookahead=True)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3, constrain_lookahead=True)
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3)                            # without the flag: today's attributes
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    cfg = types.SimpleNamespace(model_class="SurfaceFormer_Parallel")
    call = lambda **kw: run_test(cfg, None, out_dir="unused", device="cpu", model=object(), constrain_lookahead=True, **kw)
    for kw in (dict(), dict(constrain="no_repeat")):
        with pytest.raises(ValueError, match="--constrain-lookahead requires --constrain loops"):
            call(**kw)
    with pytest.raises(ValueError, match="--constrain-lookahead is not implemented with --constrain-beams"):
        call(constrain="loops", constrain_beams=2)
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--constrain-lookahead is not implemented for multi-rank runs"):
        call(constrain="loops", dist_mod=world2)
    for kw in (dict(scores=True), dict(beam=2), dict(retire_finished=True), dict(score_labels=True), dict(sample=2)):
        with pytest.raises(ValueError, match="--constrain"):
            call(constrain="loops", **kw)
    with pytest.raises(ValueError, match="--constrain applies to SurfaceFormer_Parallel only"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer"), None, out_dir="unused", device="cpu", model=object(),
                 constrain="loops", constrain_lookahead=True)
    # the record: byte-identical without the flag (the golden's text), section 16's two keys with a dead-end array
    gold = json.load(open(os.path.join(GOLDEN, "cli_coedge_case.json")))
    gm = gold["model"]
    cfgm = types.SimpleNamespace(num_points_per_line=50, num_lines=gm["num_lines"], point_dim=2, max_num_faces=42,
                                 max_face_length=gm["max_face_length"], label_seq_length=0, token=TOK)
    cfg = types.SimpleNamespace(model=cfgm, post_process=types.SimpleNamespace(is_coedge=True, enclosedness_tol=gold["tol"]))
    smp = gold["samples"][0]
    dd = tmp_path / "s"
    dd.mkdir()
    json.dump(smp["raw"], open(str(dd / "a.json"), "w"))
    item = D.ABCDataset_Parallel(str(dd), "a.json", cfgm)[0]
    pred = np.asarray(smp["predict"], dtype=np.int64)
    text, _ = cli.record_of(cfg, smp["raw"], item, pred, True)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"] and rec["pred_faces"] == smp["pred_faces"]
    dead = np.zeros(pred.shape[0], dtype=np.int32)
    rec2 = json.loads(cli.record_of(cfg, smp["raw"], item, pred, True, dead_end=dead)[0])
    assert list(rec2) == list(rec) + ["pred_dead_ends", "pred_unclosed"]


# ---- GPU: ff_follow_distance ------------------------------------------------------------------------------------------------------
def _ragged(table, ni):
    """The table with everything at and beyond the wireframes' edge counts cleared (what ff_follow_table would write)."""
    t = table.copy()
    for w, n in enumerate(ni):
        t[w, n:] = False
        t[w, :, n:] = False
    return t


def _graphs(L):
    """(name, tables bool [3, L, L], edge counts, hmax)."""
    three = lambda t: np.stack([t, t, t])
    wide, some = [L, 1, 0], [max(L - 3, 0), L // 2, L]
    lat, _, _ = CR.lattice_batch([L, max(1, L // 2), 1], L, 5, 3)
    out = [("lattice", faces.follow_table(lat["input"].numpy(), CR.TOL, [L, L // 2, 1]), [L, L // 2, 0], 254),
           ("ring, hmax at least its length", three(LR.ring(L)), wide if L > 254 else some, min(max(L, 1), 254)),
           ("ring, hmax below its length", three(LR.ring(L)), wide, max(1, min(L, 254) // 2)),
           ("chain", three(LR.chain(L)), some, 254),
           ("random", CR.random_follows(3, L, L), wide, 254),
           ("random, short search", CR.random_follows(3, L, L + 1), some, 3)]
    own = LR.chain(L)
    own[np.arange(0, L, 3), np.arange(0, L, 3)] = True
    out.append(("self-closing", three(own), wide, 254))
    if L >= 300:
        out.append(("ring of 300", three(LR.ring(L, 300)), [L, 300, 299], 254))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 31, 32, 33, 64, 65, 216, 1024])
def test_follow_distance_equals_the_numpy_restatement(hip_lib, L):
    from faceformer_amd.hip import ops
    seen = set()
    for name, table, ni, hmax in _graphs(L):
        bits = torch.from_numpy(faces.pack_follow_bits(table)).cuda()            # (bits beyond the counts stay: the kernel ignores them)
        nid = torch.tensor(ni, dtype=torch.int32).cuda()
        close, cyc = ops.follow_distance(bits, nid, hmax)
        assert close.dtype == cyc.dtype == torch.uint8 and tuple(close.shape) == (3, L, L) and tuple(cyc.shape) == (3, L)
        want = faces.follow_distance(table, hmax, ni)
        gc, gl = close.cpu().numpy(), cyc.cpu().numpy()
        assert np.array_equal(gc, want[0]), (L, name, int((gc != want[0]).sum()))
        assert np.array_equal(gl, want[1]), (L, name)
        for w, n in enumerate(ni):
            assert (gc[w, n:] == 255).all() and (gc[w, :, n:] == 255).all() and (gl[w, n:] == 255).all(), (L, name, w)
        again = ops.follow_distance(bits, nid, hmax)
        assert torch.equal(again[0], close) and torch.equal(again[1], cyc), (L, name)   # two launches: bit-equal
        seen |= set(np.unique(gc).tolist())
        if name == "ring of 300":
            assert (gl[1, :300] == 255).all() and gc[1, 0, 1] == 255 and gc[1, 254, 0] == 254    # the cycle saturates, 254 hops do not
            assert (gl[0, :300] == 255).all() and gc[2].max() == 255 and (gl[2] == 255).all()     # 299 of the 300: an open chain
        if name == "ring, hmax below its length" and L > 2:
            assert (gl == 255).all() and gc[0].max() == 255 and np.unique(gc[0]).size == hmax + 1
    assert 255 in seen and (L < 2 or 1 in seen)


# ---- GPU: the operator ------------------------------------------------------------------------------------------------------------
SPG = 3
BUDGETS = (0, 1, 2, 5, 254)


def _case(B, S, seed):
    """test_constrain._operator_case (open, closed, finished and much-visited rows; wireframe 0 with kv_len = S - 2, the last of
    three with every key masked) with wireframe 1 cut down to a single live key, and the two distance tables of its follows."""
    from test_constrain import _operator_case
    c = _operator_case(B, S, seed)
    if c["W"] >= 2:
        c["mask"][1] = True
        c["mask"][1, S - 1 if c["L"] else 0] = False
        c["kv"][1] = S
        wf = torch.arange(B) // SPG
        c["pad"] = (c["mask"][wf] | (torch.arange(S)[None, :] >= c["kv"][wf, None])).numpy()
    c["close"], c["cycle"] = faces.follow_distance(c["follows"], 254)
    return c


def _run_ahead(c, flags, close, cycle, budget, **kw):
    from faceformer_amd.hip import ops
    lg = c["logits"].clone().cuda()
    res = ops.pointer_constrained_ahead(
        lg, torch.from_numpy(c["fin"]).cuda(), torch.from_numpy(c["first"]).cuda(), torch.from_numpy(c["prev"]).cuda(),
        torch.from_numpy(faces.pack_follow_bits(c["visited"])).cuda(), flags, c["ntok"],
        torch.from_numpy(faces.pack_follow_bits(c["follows"])).cuda(), torch.from_numpy(close.copy()).cuda(), torch.from_numpy(cycle.copy()).cuda(),
        budget, memory=c["memory"].cuda(), mask=c["mask"].to(torch.uint8).cuda(), kv_len=c["kv"].cuda(), seqs_per_group=SPG,
        term_range=c["term"], want_rows=True, want_stats=True, **kw)
    return lg, res


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 63, 64, 65, 260, 1028])
def test_operator_against_the_numpy_rule(hip_lib, S):
    from test_constrain import _bits_to_bool, _run_operator
    from faceformer_amd.hip import ops
    seen = dict(open=0, closed=0, dead=0, finished=0, nolive=0, ahead=0, ahead_dead=0)
    for B in (1, 3, 9):
        c = _case(B, S, 100 * S + B)
        ntok, term, L = c["ntok"], c["term"], c["L"]
        raw = c["logits"].numpy()
        for budget in BUDGETS:
            for flags in ((LOOPS, CR.CONNECT) if budget == 2 else (LOOPS,)):
                counter = torch.zeros(1, dtype=torch.int32).cuda()
                lg, res = _run_ahead(c, flags, c["close"], c["cycle"], budget, counter=counter)
                own = lg.cpu().numpy()
                got = {k: res[k].cpu().numpy() for k in ("next", "logprob", "fin", "dead_end", "first", "prev")}
                vis = _bits_to_bool(res["visited"], L) if L else np.zeros((B, 0), dtype=bool)
                rows = res["mask_rows"].cpu().numpy() != 0
                what = (S, B, flags, budget)
                nge = 0
                for b in range(B):
                    w = b // SPG
                    st = (frozenset(np.flatnonzero(c["visited"][b]).tolist()), None if c["first"][b] < 0 else int(c["first"][b]),
                          None if c["prev"][b] < 0 else int(c["prev"][b]))
                    args = (raw[b].astype(np.float64), c["pad"][b], st, flags, ntok, term, c["follows"][w])
                    r = LR.step_row(*args, c["close"][w], c["cycle"][w], budget, finished=bool(c["fin"][b]))
                    if c["fin"][b]:
                        assert np.array_equal(own[b], raw[b]), what                                # finished rows untouched
                        assert got["logprob"][b] == 0.0
                        seen["finished"] += 1
                    else:
                        hidden = r["masked"] | c["pad"][b]
                        assert np.array_equal(rows[b], r["masked"]), (what, b)                     # the byte row: the rule's own mask
                        assert np.array_equal(own[b] == np.float32(FILL), hidden), (what, b)       # the FILL pattern: the allowed set
                        assert np.array_equal(own[b][~hidden], raw[b][~hidden]), (what, b)
                        want_lp = CR.select(own[b].astype(np.float64))[1]
                        assert abs(float(got["logprob"][b]) - want_lp) <= CR.LP_BAR, (what, b, got["logprob"][b], want_lp)
                        plain = CR.step_row(*args)
                        seen["ahead"] += bool((r["masked"] & ~plain["masked"]).any())
                        seen["ahead_dead"] += r["dead"] and not plain["dead"]
                        seen["dead" if r["dead"] else ("open" if st[1] is not None and st[2] is not None else "closed")] += 1
                        seen["nolive"] += bool(hidden.all())
                        nge += r["tok"] >= ntok
                    assert got["next"][b] == r["tok"], (what, b, got["next"][b], r["tok"])        # exact, ties included
                    assert bool(got["fin"][b]) == r["fin"] and bool(got["dead_end"][b]) == r["dead"], (what, b)
                    nv, nf, npv = r["state"]
                    assert (got["first"][b], got["prev"][b]) == (-1 if nf is None else nf, -1 if npv is None else npv), (what, b)
                    assert set(np.flatnonzero(vis[b]).tolist()) == set(nv), (what, b)
                assert int(counter.item()) == nge, what
                forced = ops.pointer_forced(c["logits"].clone().cuda(), res["next"], c["memory"].cuda(), c["mask"].to(torch.uint8).cuda(),
                                            c["kv"].cuda(), seqs_per_group=SPG, want_rows=True, want_stats=True)
                assert torch.equal(res["rows"], forced["rows"]) and torch.equal(res["stats"], forced["stats"]), what
                lg2, res2 = _run_ahead(c, flags, c["close"], c["cycle"], budget)                   # two launches: bit-equal
                assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
                # the identity: with both tables zero every output is ops.pointer_constrained's, bit for bit
                lz, rz = _run_ahead(c, flags, np.zeros_like(c["close"]), np.zeros_like(c["cycle"]), budget)
                lp_, rp = _run_operator(c, flags)
                assert set(rz) == set(rp) and all(torch.equal(rz[k], rp[k]) for k in rp) and torch.equal(lz, lp_), what
    print("S=%d rows by state:" % S, seen)
    if S >= 63:
        assert all(v > 0 for v in seen.values()), seen                                           # every state was exercised


# ---- GPU: the engine --------------------------------------------------------------------------------------------------------------
ENGINE_GOLDENS = ["par_small_gain4", "par_small_ragged", "par_full_n40_gain4"]
_TABLES = {}


def _tables(name, table=None, key=None):
    """(bits, close_dist, cycle_len) on the GPU for the lattice of `name` (or `table`, cached under `key`): ops.follow_distance
    with hmax = max(T - 2, 1), as the model builds them -- held to faces.follow_distance here."""
    from test_constrain import _model
    from faceformer_amd.hip import ops
    if (name, key) not in _TABLES:
        case, _, _, _, _, lat, _, _, lattice = _model(name)
        table = lattice if table is None else table
        ni = lat["num_input"]
        hmax = max(case["model"]["seq_len"] - 2, 1)
        bits = torch.from_numpy(faces.pack_follow_bits(table)).cuda()
        close, cyc = ops.follow_distance(bits, torch.tensor(ni, dtype=torch.int32).cuda(), hmax)
        want = faces.follow_distance(table, hmax, ni)
        assert np.array_equal(close.cpu().numpy(), want[0]) and np.array_equal(cyc.cpu().numpy(), want[1]), name
        _TABLES[(name, key)] = (bits, close, cyc)
    return _TABLES[(name, key)]


def _ahead(model, case, b, tables, **kw):
    from test_logprob import _decode
    bits, close, cyc = tables
    return _decode(model, case, b, constrain=LOOPS, follow_table=bits, term_range=TERM, constrain_lookahead=True, close_dist=close,
                   cycle_len=cyc, **kw)


def _replay(out, table, tables, F, T, what):
    """The numpy rule on the decode's own tokens, traced logits and tables: at every (step, unfinished sequence) the FILL
    pattern, the argmax token and the flags; none is left out.  Returns (pairs, margins [steps, rows] of the constrained row, inf
    where finished, pairs at which the look-ahead masked a key section 16 leaves live)."""
    from test_constrain import _check_layout
    pred, lp, fin, steps = _check_layout(out, T)
    close, cyc = tables[1].cpu().numpy(), tables[2].cpu().numpy()
    logits = out["logits"].cpu().numpy()
    dead = out["dead_end"].cpu().numpy() != 0
    want_dead = np.zeros(pred.shape[0], dtype=bool)
    margins = np.full((steps, pred.shape[0]), np.inf)
    pairs = ahead = 0
    for j in range(steps):
        budget = T - 2 - j                                                                    # the step selects position j + 1
        for r in np.flatnonzero(fin > j):
            w = r // F
            st = CR.state_of_prefix(pred[r, : j + 1], NTOK, table[w])
            row = logits[j, r]
            pad = out["_pad"][w]
            masked, is_dead = LR.rule_mask(st, LOOPS, row.size, NTOK, TERM, table[w], pad, close[w], cyc[w], budget)
            assert np.array_equal(row == np.float32(FILL), masked | pad), (what, j, int(r))
            tok, own_lp = CR.select(row.astype(np.float64))
            assert pred[r, j + 1] == tok, (what, j, int(r), int(pred[r, j + 1]), tok)
            assert abs(lp[r, j + 1] - own_lp) <= CR.LP_BAR, (what, j, int(r))
            want_dead[r] |= is_dead
            if is_dead:
                assert fin[r] == j + 1, (what, j, int(r))
            ahead += bool((masked & ~CR.rule_mask(st, LOOPS, row.size, NTOK, TERM, table[w], pad)[0]).any())
            live = np.sort(row[row > np.float32(FILL)].astype(np.float64))
            margins[j, r] = live[-1] - live[-2] if live.size > 1 else np.inf
            pairs += 1
    assert np.array_equal(dead, want_dead), what
    return pairs, margins, ahead


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_with_zero_tables_is_the_loops_decode(hip_lib, name):
    from test_constrain import _constrained, _model
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    bits, close, cyc = _tables(name)
    loops = _constrained(model, case, b, LOOPS, table, trace=True)
    zero = _ahead(model, case, b, (bits, torch.zeros_like(close), torch.zeros_like(cyc)), trace=True)
    assert zero["steps"] == loops["steps"] and zero["step_counts"] == loops["step_counts"], name
    for k in ("predict", "logprob", "dead_end", "seq_of_row"):
        assert torch.equal(zero[k], loops[k]), (name, k)
    assert torch.equal(zero["logits"].nan_to_num(7.0), loops["logits"].nan_to_num(7.0)), name
    on = _ahead(model, case, b, (bits, close, cyc))
    assert not torch.equal(on["predict"], loops["predict"]), name                             # the tables are what changes it


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_replays_under_the_numpy_rule(hip_lib, name):
    from test_constrain import _model, _with_pad
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T, F = case["model"]["seq_len"], max(lat["num_input"])
    tables = _tables(name)
    out = _with_pad(_ahead(model, case, b, tables, trace=True), b)
    pairs, _, ahead = _replay(out, table, tables, F, T, name)
    print(name, "steps=%d, %d (step, sequence) pairs replayed, none left out; the look-ahead masked at %d; dead ends: %d"
          % (out["steps"], pairs, ahead, int(out["dead_end"].sum())))
    assert pairs > 0 and ahead > 0


@pytest.mark.gpu
def test_engine_replays_dead_ends_and_saturated_distances_on_a_sparse_table(hip_lib):
    from test_constrain import _model, _with_pad
    name = "par_small_gain4"
    case, z, model, gb, sd, lat, b, edges, _ = _model(name)
    ni = lat["num_input"]
    T, F = case["model"]["seq_len"], max(ni)
    table = _ragged(CR.random_follows(len(ni), case["model"]["L"], 5), ni)
    tables = _tables(name, table, "sparse")
    out = _with_pad(_ahead(model, case, b, tables, trace=True), b)
    pairs, _, ahead = _replay(out, table, tables, F, T, (name, "sparse"))
    dead = int(out["dead_end"].sum())
    far = faces.follow_distance(table, 254, ni)[0]
    saturated = int(((far != 255) & (tables[1].cpu().numpy() == 255)).sum())
    print(name, "sparse table: steps=%d, %d pairs replayed, look-ahead at %d, dead ends: %d, distances beyond hmax: %d"
          % (out["steps"], pairs, ahead, dead, saturated))
    assert dead > 0 and ahead > 0 and saturated > 0


def _yield(pred, dead, ni, edges, F):
    from test_constrain import _yield as count
    return count(pred, dead, ni, edges, F)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_every_row_ends_closed_or_flagged_and_enough_end_enclosed(hip_lib, name):
    from test_constrain import _check_layout, _constrained, _model
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, F = case["model"]["seq_len"], max(ni)
    out = _ahead(model, case, b, _tables(name))
    pred, _, fin, steps = _check_layout(out, T)
    dead = out["dead_end"].cpu().numpy() != 0
    enclosed = 0
    for w, n in enumerate(ni):
        for f in range(n):
            r = w * F + f
            row = pred[r]
            last = int(min(fin[r], steps))
            state = CR.state_of_prefix(row[: last + 1], NTOK, table[w])
            assert dead[r] or state[1] is None, (name, w, f, row)                            # the guarantee: flagged, or closed
            idx = [int(t) - NTOK for t in row if t >= NTOK]
            assert len(idx) == len(set(idx)), (name, w, f, row)                              # no row holds an edge twice
            if ((row >= TERM[0]) & (row < TERM[1])).any() and not dead[r]:
                face = faces._parallel_rows(row[None], TOK, n)
                if face:                                                                     # (an anchor below ntok that ends at once has no edge)
                    assert faces.is_face_enclosed(edges[w], face[0][1], CR.TOL), (name, w, f, row)
                    enclosed += 1
    own = sum(ni)
    loops = _constrained(model, case, b, LOOPS, table)
    before = _yield(loops["predict"].cpu().numpy(), loops["dead_end"].cpu().numpy() != 0, ni, edges, F)
    after = _yield(pred, dead, ni, edges, F)
    print(name, "enclosed / dead end / other of %d own-anchor rows: loops %d / %d / %d, with look-ahead %d / %d / %d"
          % ((own,) + before + after))
    assert after[0] == enclosed
    assert enclosed >= LR.MIN_ENCLOSED * own, (name, enclosed, own)                          # non-vacuity: a condition on the fixture
    if name == "par_small_ragged":
        assert after[0] > before[0], (name, after, before)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_against_the_teacher_forced_oracle(hip_lib, name):
    from test_constrain import _check_against_oracle, _model, _with_pad
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    out = _with_pad(_ahead(model, case, b, _tables(name), trace=True), b)
    left, pairs, _ = _check_against_oracle(name, case, sd, lat, out, what="look-ahead " + name)
    assert left <= CR.CAP * pairs, (name, left, pairs)


@pytest.mark.gpu
def test_plan_invariance_and_determinism(hip_lib):
    from test_constrain import _model, _same_on_decisive_pairs, _with_pad
    from test_parity_golden import _tol
    from faceformer_amd.hip import lib as L
    name = "par_small_ragged"
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, N, F = case["model"]["seq_len"], len(ni), max(ni)
    tables = _tables(name)
    whole = _with_pad(_ahead(model, case, b, tables, trace=True, chunk_wireframes=0), b)
    again = _ahead(model, case, b, tables, trace=True, chunk_wireframes=0)
    for k in ("predict", "logprob", "dead_end"):
        assert torch.equal(whole[k], again[k]), k                                    # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"] and torch.equal(whole["logits"].nan_to_num(7.0), again["logits"].nan_to_num(7.0))
    one = _with_pad(_ahead(model, case, b, tables, trace=True, chunk_wireframes=1), b)  # (the tables offset per chunk)
    _, mw, _ = _replay(whole, table, tables, F, T, "whole")
    _, mo, _ = _replay(one, table, tables, F, T, "one")
    lw = whole["logits"].cpu().numpy()
    fin_w = CR.stop_and_finish(whole["predict"].cpu().numpy(), TERM, NTOK)[0]
    tol_of = lambda j: _tol(lw[j][fin_w > j]) if (fin_w > j).any() else 0.0
    full = _same_on_decisive_pairs(whole["predict"].cpu().numpy(), mw, one["predict"].cpu().numpy(), mo, tol_of, T, "chunk_wireframes = 1")
    print("chunk_wireframes = 1 against the whole batch: %d of %d rows compared to the end" % (full, N * F))
    assert full > 0
    # two wireframe orders, the three tables moved with the wireframes
    eng, memory, mask, kv_len = model._encode(b)
    perm = list(reversed(range(N)))
    idx = torch.tensor(perm, device="cuda")
    moved = tuple(t.index_select(0, idx).contiguous() for t in tables)
    kw = dict(T=T, F=F, flags=model.decode_flags, x3_min_rows=model.x3_min_rows, constrain=LOOPS, term_range=TERM, trace=True,
              constrain_lookahead=True)
    fwd = _with_pad(eng.decode(memory, mask, kv_len, L.FF_PARALLEL, num_input=ni, follow_table=tables[0], close_dist=tables[1],
                               cycle_len=tables[2], **kw), b)
    rev = eng.decode(memory.index_select(0, idx).contiguous(), mask.index_select(0, idx).contiguous(), kv_len.index_select(0, idx).contiguous(),
                     L.FF_PARALLEL, num_input=[ni[i] for i in perm], follow_table=moved[0], close_dist=moved[1], cycle_len=moved[2], **kw)
    rev["_pad"] = fwd["_pad"][perm]
    _, mf, _ = _replay(fwd, table, tables, F, T, "fwd")
    _, mr, _ = _replay(rev, table[perm], moved, F, T, "rev")
    back = np.argsort(perm)
    rp = rev["predict"].cpu().numpy().reshape(N, F, T)[back].reshape(N * F, T)
    mrb = mr.reshape(mr.shape[0], N, F)[:, back].reshape(mr.shape[0], N * F)
    lf = fwd["logits"].cpu().numpy()
    fin_f = CR.stop_and_finish(fwd["predict"].cpu().numpy(), TERM, NTOK)[0]
    tol_f = lambda j: _tol(lf[j][fin_f > j]) if (fin_f > j).any() else 0.0
    full = _same_on_decisive_pairs(fwd["predict"].cpu().numpy(), mf, rp, mrb, tol_f, T, "two wireframe orders")
    print("two wireframe orders: %d of %d rows compared to the end" % (full, N * F))
    assert full > 0


@pytest.mark.gpu
def test_model_keys_in_batch_order_and_option_off(hip_lib):
    from test_constrain import _model
    case, z, model, gb, sd, lat, b, edges, table = _model("par_small_ragged")
    T = case["model"]["seq_len"]
    ni = lat["num_input"]
    N, F = len(ni), max(ni)
    order = sorted(range(N), key=lambda i: -ni[i])
    assert order != list(range(N))                                   # the premise: the model does reorder this batch
    idx = torch.tensor(order, device="cuda")
    by_hand = {k: (v.index_select(0, idx) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in b.items()}
    by_hand["num_input"] = [ni[i] for i in order]
    bits, close, cyc = _tables("par_small_ragged")
    nothing = torch.full_like(close, 255), torch.full_like(cyc, 255)   # an override: no loop can ever close
    try:
        with torch.no_grad():
            model.constrain = "loops"
            loops = model(dict(b))
            keys_loops = set(loops)
            model.constrain_lookahead = True
            on = model(dict(b))
            given = model(dict(b, close_dist=close, cycle_len=cyc))
            cpu = model(dict(b, close_dist=close.cpu(), cycle_len=cyc.cpu().numpy()))
            none = model(dict(b, close_dist=nothing[0], cycle_len=nothing[1]))
            zero = model(dict(b, close_dist=torch.zeros_like(close), cycle_len=torch.zeros_like(cyc)))
            with pytest.raises(ValueError, match="given together"):
                model(dict(b, close_dist=close))
            with pytest.raises(ValueError, match="cycle_len must be uint8"):
                model(dict(b, close_dist=close, cycle_len=cyc.int()))
            model.sort_by_edges = False
            hand = model(dict(by_hand))
            hand_given = model(dict(by_hand, close_dist=close.index_select(0, idx), cycle_len=cyc.index_select(0, idx)))
    finally:
        model.constrain, model.constrain_lookahead, model.sort_by_edges = None, False, True
    keys = {"predict", "predict_logprob", "predict_dead_end"}
    assert set(on) == keys_loops and keys <= keys_loops                              # the published keys are section 16's
    assert tuple(on["predict"].shape) == tuple(on["predict_logprob"].shape) == (N, F, T) and tuple(on["predict_dead_end"].shape) == (N, F)
    for k in keys:
        assert torch.equal(on[k], given[k]) and torch.equal(on[k], cpu[k]), k            # the built tables are ops.follow_distance's
        assert torch.equal(on[k].index_select(0, idx), hand[k]) and torch.equal(hand[k], hand_given[k]), k   # batch order, rows and tables
        assert torch.equal(zero[k], loops[k]), k                                         # zero tables: the "loops" decode
    assert not torch.equal(on["predict"], loops["predict"])
    # the override is what the decode used: every own anchor that is an edge ends at once, flagged, unless it closes on itself
    dead = none["predict_dead_end"].cpu().numpy() != 0
    own_cycle = cyc.cpu().numpy()
    for w, n in enumerate(ni):
        for f in range(NTOK, n):
            assert dead[w, f] == (not table[w, f - NTOK, f - NTOK]), (w, f)
    assert (own_cycle != 255).any()
    # option off: a model that never had the attribute decodes as before
    with torch.no_grad():
        off = model(dict(b))
    saved = model.__dict__.pop("constrain_lookahead")
    try:
        with torch.no_grad():
            never = model(dict(b))
            model.constrain = "loops"
            never_loops = model(dict(b))
    finally:
        model.constrain = None
        model.__dict__["constrain_lookahead"] = saved
    assert set(never) == set(off) and torch.equal(never["predict"], off["predict"])
    for k in keys:
        assert torch.equal(never_loops[k], loops[k]), k


@pytest.mark.gpu
def test_workspace_query_is_the_constrained_decodes(hip_lib):
    import ctypes as C
    from test_constrain import _model
    from faceformer_amd.hip import lib as L
    case, z, model, gb, sd, lat, b, edges, table = _model("par_small_ragged")
    ni = lat["num_input"]
    eng = model.engine()
    prm = L.DecodeParams()
    prm.variant, prm.N, prm.L, prm.F, prm.T = L.FF_PARALLEL, len(ni), case["model"]["L"], max(ni), case["model"]["seq_len"]
    prm.flags, prm.term_lo, prm.term_hi = model.decode_flags, TERM[0], TERM[1]
    ni_host = (C.c_int * len(ni))(*ni)
    a = hip_lib.ff_decode_constrained_ahead_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host)
    assert a == hip_lib.ff_decode_constrained_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host) > 0   # nothing new in it


# ---- GPU: poisoned surroundings, a far operand, the launch forms --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,F,S", [(2, 3, 70), (3, 1, 37)])
def test_operators_inside_poisoned_surroundings(hip_lib, W, F, S):
    import redzone as RZ
    from test_redzone_ops import PAD, twice
    from faceformer_amd.hip import ops
    E, ntok = 64, 4
    L = S - ntok
    B = W * F
    table = _ragged(CR.random_follows(W, L, 11), [L - 2 * w for w in range(W)])
    ni = torch.tensor([L - 2 * w for w in range(W)], dtype=torch.int32)
    follows = torch.from_numpy(faces.pack_follow_bits(table))
    got = twice(lambda g: dict(zip(("close", "cycle"), ops.follow_distance(g.embed(follows, name="follows"), g.embed(ni, name="num_input"), 9))),
                "ff_follow_distance")
    want = faces.follow_distance(table, 9, ni.tolist())
    assert np.array_equal(got["close"].cpu().numpy(), want[0]) and np.array_equal(got["cycle"].cpu().numpy(), want[1])
    close, cyc = got["close"].cpu(), got["cycle"].cpu()
    g0 = torch.Generator().manual_seed(S)
    raw = torch.randn(B, S, generator=g0) * 3
    mem = torch.randn(W, S, E, generator=g0)
    mask = (torch.rand(W, S, generator=g0) < 0.1).to(torch.uint8)
    mask[:, :ntok] = 0
    kv_len = torch.tensor([S - w for w in range(W)], dtype=torch.int32)
    fin = (torch.arange(B) % 4 == 3).to(torch.int32)
    first = (torch.arange(B) % L).to(torch.int32)
    first[1::3] = -1                                                                           # closed rows: cycle_len is read
    prev = ((torch.arange(B) * 3) % L).to(torch.int32)
    vis = np.zeros((B, L), dtype=bool)
    for i in range(B):
        vis[i, [int(prev[i])] + ([int(first[i])] if first[i] >= 0 else [])] = True
    visited = torch.from_numpy(faces.pack_follow_bits(vis))

    def call(lg, e):
        o = ops.pointer_constrained_ahead(lg, e(fin), e(first), e(prev), e(visited), LOOPS, ntok, e(follows), e(close), e(cyc), 3,
                                          memory=e(mem), mask=e(mask), kv_len=e(kv_len), seqs_per_group=F, term_range=(1, 4),
                                          want_rows=True, want_stats=True, counter=e(torch.zeros(1, dtype=torch.int32)))
        return dict(o, logits=lg)
    got = twice(lambda g: call(g.embed(raw, ld=S + PAD, name="logits"), g.embed), "ff_pointer_constrained_ahead")
    plain = call(raw.cuda(), lambda x: x.cuda())
    for k, v in plain.items():
        if torch.is_tensor(v):
            RZ.assert_same_bits(got[k], v, "ff_pointer_constrained_ahead: %s against the clean call" % k)
    assert torch.isfinite(got["logprob"]).all() and bool(got["mask_rows"].any())


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "par_small_ragged"
    m = WP._bound(name, "default")
    b, table = WP._lattice(m)
    tables = _tables(name)
    call = lambda: _ahead(m.model, m.case, b, tables, trace=True)
    clean = call()
    clean.pop("engine", None)
    zero, d = WP._run([m], call, fill=RZ.ZERO, what="look-ahead after ZERO")
    poison, _ = WP._run([m], call, fill=RZ.POISON, what="look-ahead after POISON")
    WP._assert_equal(poison, zero, "look-ahead")
    WP._assert_equal(poison, clean, "look-ahead against the clean run")
    WP._assert_no_nan(poison, "look-ahead")
    assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size


@pytest.mark.gpu
def test_close_dist_of_a_wireframe_past_2_31_bytes(hip_lib):
    """close_dist as a far view (tests/farview.py): rows [wireframe, first] of a [W * L, L] byte matrix whose last wireframes lie
    past 2^31 bytes; only the rows the launch may read hold values, everything else is poison (255: masked at every budget)."""
    import farview as FV
    import redzone as RZ
    from faceformer_amd.hip import ops
    L, ntok = 1024, 4
    S = L + ntok
    W = (1 << 31) // (L * L) + 2                                                              # 2050 wireframes of 1 MiB each
    B, near, far_w = W, 1, W - 1
    assert far_w * L * L > (1 << 31)
    g0 = torch.Generator().manual_seed(31)
    first = torch.full((B,), -1, dtype=torch.int32)
    prev = torch.full((B,), -1, dtype=torch.int32)
    fin = torch.ones(B, dtype=torch.int32)                                                    # every row finished but two
    rows_at, values = [], []
    follows = torch.zeros(W, L, (L + 31) // 32, dtype=torch.int32)
    cases = ((near, 5, 9), (far_w, 700, 33))
    for w, f, p in cases:
        first[w], prev[w], fin[w] = f, p, 0
        follows[w, p] = -1                                                                    # every edge follows prev
        rows_at.append(w * L + f)
        values.append(torch.randint(1, 9, (L,), generator=g0, dtype=torch.int64).to(torch.uint8))
    rows_at.append(W * L - 1)                                                                 # (the matrix's last row, so that it has W * L)
    values.append(torch.full((L,), 255, dtype=torch.uint8))
    matrix = FV.far_rows(torch.stack(values), rows_at, L, fill=RZ.POISON)
    close = matrix.view(W, L, L)
    assert close.is_contiguous() and close.data_ptr() == matrix.data_ptr() and FV.farthest(matrix) > (1 << 31)
    cyc = torch.zeros(W, L, dtype=torch.uint8)
    logits = torch.randn(B, S, generator=g0)
    visited = torch.zeros(B, (L + 31) // 32, dtype=torch.int32)
    budget = 4
    res = ops.pointer_constrained_ahead(logits.clone().cuda(), fin.cuda(), first.cuda(), prev.cuda(), visited.cuda(), LOOPS, ntok,
                                        follows.cuda(), close, cyc.cuda(), budget, seqs_per_group=1, term_range=(1, 4))
    FV.check_untouched(matrix, "close_dist")
    rows = res["mask_rows"].cpu().numpy() != 0
    nxt = res["next"].cpu().numpy()
    for (w, f, p), dist in zip(cases, values):
        want = dist.numpy().astype(np.int64) > budget
        assert 0 < want.sum() < L
        assert rows[w, :ntok].all() and np.array_equal(rows[w, ntok:], want), w                # the far row was read, not a wrapped one
        allowed = np.where(want, -np.inf, logits[w, ntok:].numpy())
        assert nxt[w] == ntok + int(np.argmax(allowed)) and not bool(res["dead_end"][w]), w
    assert (nxt[fin.numpy() != 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["f32", "fp16x2", "no_l0_fold", "drained", "two_streams"])
def test_replay_under_the_launch_forms(hip_lib, form):
    import test_mode_forms as MF
    from test_constrain import _with_pad
    name = "par_small_ragged"
    assert form in MF.FORMS
    m = MF._bound(name, form)
    lat, b, table = MF._lattice(name)
    tables = _tables(name)
    call = lambda bound: _with_pad(_ahead(bound.model, bound.case, b, tables, trace=True, num_streams=bound.model.num_streams), b)
    with MF._tuned(form):
        out = call(m)
        MF._check_bit_equal(m, lambda bound: {k: v for k, v in call(bound).items() if k not in ("engine", "_pad")}, m.what)
    pairs, _, ahead = _replay(out, table, tables, max(lat["num_input"]), m.T, m.what)
    print("look-ahead %s %s: steps %d, %d pairs replayed, none left out, look-ahead at %d" % (name, form, out["steps"], pairs, ahead))
    assert pairs > 0 and ahead > 0
