"""Opt-in exact closure look-ahead of the loop-constrained pointer decode: the numpy rule (tests/exact_ref.py,
composed from constrain_ref and lookahead_ref) on the hand-written trap and against an exhaustive search, faces.closure_distance,
the C ABI, the bindings, every rejected combination and the CLI on the CPU; ff_pointer_constrained_exact and the engine's
CONSTRAIN_EXACT mode against that rule on the GPU.

Bars (the issue's, none measured): byte rows, FILL patterns, tokens, flags, next states and visited words are exact;
log-probabilities within 2^-16 of fp64 log_softmax of the kernel's own masked row (DESIGN.md 12's bar); appended rows and
statistics bit-equal to ff_pointer_forced's; closed-state rows byte-equal to the look-ahead operator's, open rows mask a superset
of its edge keys; traced logits within test_parity_golden._tol of the fp64 oracle teacher-forced along the decode's tokens, at
most 2 % of the pairs left out; no dead end other than right after a loop-opening position; enclosed(exact) >=
enclosed(look-ahead) on every lattice fixture (conditions on the fixtures: tools/exact_left_out.py)."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
import exact_ref as ER
import lookahead_ref as LR
from conftest import GOLDEN, ROOT, token_ns
from faceformer_amd import faces
from test_constrain import _tiny_inputs, _tiny_model, _untouchable

TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
NTOK = TOK.len
FILL = CR.FILL
LOOPS = ER.LOOPS
NEW_ENTRIES = ("ff_pointer_constrained_exact", "ff_decode_constrained_exact_workspace_bytes", "ff_decode_constrained_exact")


# ---- CPU: the rule ----------------------------------------------------------------------------------------------------------------
def test_the_trap_by_hand():
    """Edges 0 -> 1, 1 -> 2, 1 -> 3, 2 -> 0, 3 -> 1 with first = 0, prev = 1, visited = {0, 1}: the static distance of edge 3 runs
    through the visited edge 1, so the look-ahead leaves it live and dead-ends one step later; the exact rule masks it."""
    t = ER.trap()
    S = NTOK + 4
    pad = np.zeros(S, dtype=bool)
    close, cyc = faces.follow_distance(t)
    assert close[0][3] == 3 and close[0][2] == 1
    st = CR.state_of_prefix([NTOK + 0, NTOK + 1], NTOK, t)
    assert st == (frozenset({0, 1}), 0, 1)
    assert faces.closure_distance(t, [0, 1], 0).tolist() == [255, 2, 1, 255]                  # (b itself may be a visited edge)
    assert faces.closure_distance(t, np.zeros(4, dtype=bool), 0).tolist() == [3, 2, 1, 3]     # nothing visited: the static distances
    raw = np.zeros(S)
    raw[NTOK + 3] = 5.0                                                                   # the logits favour edge 3
    for budget in (3, 5, 254):
        a = LR.step_row(raw, pad, st, LOOPS, NTOK, TERM, t, close, cyc, budget)
        assert a["masked"][NTOK:].tolist() == [True, True, False, False] and a["tok"] == NTOK + 3 and not a["dead"]
        a2 = LR.step_row(raw, pad, a["state"], LOOPS, NTOK, TERM, t, close, cyc, budget - 1)
        assert a2["dead"] and a2["fin"]                                                   # ... and dead-end one step later
        e = ER.step_row(raw, pad, st, NTOK, TERM, t, cyc, budget)
        assert e["masked"][NTOK:].tolist() == [True, True, False, True] and e["tok"] == NTOK + 2 and not e["dead"]
        assert e["state"] == (frozenset({0, 1, 2}), None, 2)                              # the exact rule closes
    # budget 0: nothing can close, a dead end; a padded edge 2 leaves nothing either
    assert ER.step_row(raw, pad, st, NTOK, TERM, t, cyc, 0)["dead"]
    pad2 = pad.copy()
    pad2[NTOK + 2] = True
    assert ER.step_row(raw, pad2, st, NTOK, TERM, t, cyc, 5)["dead"]
    # closed: the static cycle_len rule, unchanged (edges 0, 1, 2 lie on a 3-cycle, edge 3 on the 2-cycle 3 -> 1 -> 3)
    closed = (frozenset(), None, None)
    assert cyc.tolist() == [3, 2, 3, 2]
    for budget in (1, 2, 3):
        e = ER.step_row(raw, pad, closed, NTOK, TERM, t, cyc, budget)
        a = LR.step_row(raw, pad, closed, LOOPS, NTOK, TERM, t, close, cyc, budget)
        assert np.array_equal(e["masked"], a["masked"]) and e["tok"] == a["tok"]
    assert ER.step_row(raw, pad, st, NTOK, TERM, t, cyc, 3, finished=True)["tok"] == 0


def _tables_small():
    out = [("ring", LR.ring(7)), ("ring of 4 among 7", LR.ring(7, 4)), ("chain", LR.chain(6)), ("self-closing", ER.self_closing(8)),
           ("trap", ER.trap()), ("one edge", LR.ring(1)), ("one open edge", np.zeros((1, 1), dtype=bool))]
    for L in (2, 5, 8, 10):
        out += [("random %d/%d" % (L, w), t) for w, t in enumerate(CR.random_follows(3, L, 40 + L))]
    return out


def test_the_reference_is_exact_against_an_exhaustive_search():
    """On walks of the rule, at every budget 0..L: the live edge set under the reference equals the set of connected, unused,
    unpadded edges from which an exhaustive depth-first search finds a simple continuation that closes the loop in time."""
    rng = np.random.default_rng(25)
    states = exact = 0
    for what, t in _tables_small():
        L = t.shape[0]
        S = NTOK + L
        cyc = faces.follow_distance(t)[1]
        for trial in range(6):
            walk = ER.walk_states(t, rng.integers(0, L), int(rng.integers(0, L + 1)), rng, NTOK)
            st = walk[int(rng.integers(0, len(walk)))]
            pad = np.zeros(S, dtype=bool)
            if trial % 3 == 2:
                pad[NTOK:] = rng.random(L) < 0.25
            if st[1] is None:
                continue
            visited, first, prev = st
            avail = ~pad[NTOK:]
            avail[sorted(visited)] = False
            static = faces.follow_distance(t)[0]
            for budget in range(L + 1):
                masked, dead = ER.rule_mask(st, S, NTOK, TERM, t, pad, cyc, budget)
                live = set(np.flatnonzero(~masked[NTOK:] & ~pad[NTOK:]).tolist())
                want = {b for b in range(L) if t[prev, b] and avail[b] and ER.can_close(t, avail, first, b, budget)}
                assert live == want, (what, st, budget, live, want)
                assert dead == (not want) and masked[:TERM[0]].all() and masked[TERM[0]:TERM[1]].all() == (not dead)
                ahead = LR.rule_mask(st, LOOPS, S, NTOK, TERM, t, pad, static, cyc, budget)[0]
                assert not (ahead[NTOK:] & ~masked[NTOK:]).any(), (what, st, budget)       # contains the look-ahead: D_V >= D
                exact += bool((masked[NTOK:] & ~ahead[NTOK:]).any())
            states += 1
    assert states > 40 and exact > 0


def test_numpy_closure_distance_against_the_search():
    assert "closure_distance" in faces.__all__
    rng = np.random.default_rng(7)
    checked = 0
    for what, t in _tables_small():
        L = t.shape[0]
        for trial in range(5):
            visited = rng.random(L) < (0.0 if trial == 0 else 0.3)
            first = int(rng.integers(0, L))
            visited[first] = True
            n = None if trial < 3 else int(rng.integers(0, L + 1))                       # ragged num_input
            pad = None if trial % 2 else rng.random(L) < 0.2
            avail = ~visited & (np.arange(L) < (L if n is None else n)) & (~pad if pad is not None else True)
            for hmax in (254, 3, 1):
                got = faces.closure_distance(t, visited, first, hmax, n, pad)
                assert got.dtype == np.uint8 and got.shape == (L,)
                for b in range(L):
                    want = next((h for h in range(1, min(hmax, L + 1) + 1) if ER.can_close(t, avail, first, b, h)), 255)
                    assert got[b] == want, (what, trial, hmax, b, got[b], want)
                    checked += 1
            assert np.array_equal(faces.closure_distance(t, np.flatnonzero(visited), first, 254, n, pad),
                                  faces.closure_distance(t, visited, first, 254, n, pad))         # visited as a list of edges
    assert checked > 500
    ring = LR.ring(6)
    assert faces.closure_distance(ring, [0], 0).tolist() == [6, 5, 4, 3, 2, 1]
    assert faces.closure_distance(ring, [0, 1, 2], 0).tolist() == [255, 255, 4, 3, 2, 1]      # b itself may be any edge, visited too
    assert faces.closure_distance(ring, [0, 3], 0).tolist() == [255, 255, 255, 3, 2, 1]       # edge 3 used: 1 and 2 are cut off
    assert faces.closure_distance(ring, [0], 0, hmax=3).tolist() == [255, 255, 255, 3, 2, 1]
    assert faces.closure_distance(LR.chain(5), [0], 0).tolist() == [255] * 5
    own = ER.self_closing(4)
    assert faces.closure_distance(own, [3], 3).tolist() == [3, 2, 1, 1]
    assert faces.closure_distance(ring, [0], 0, num_input=4).tolist() == [255, 255, 255, 255, 255, 1]
    for bad in (0, 255, True, 1.5):
        with pytest.raises(ValueError, match="hmax"):
            faces.closure_distance(ring, [0], 0, bad)
    with pytest.raises(ValueError, match="first"):
        faces.closure_distance(ring, [0], 6)
    with pytest.raises(ValueError, match="table must be"):
        faces.closure_distance(np.zeros((2, 3), dtype=bool), [0], 0)


# ---- CPU: C ABI and binding -------------------------------------------------------------------------------------------------------
def test_header_declares_the_exact_entries_within_abi_105():
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    doc = header[header.index("exact closure look-ahead for the loop-constrained pointer decode"): header.index("int ff_pointer_constrained_exact(")]
    for phrase in ("budget = T - 1 - p, so T <= 256", "Let avail(x) hold when all three are true", "x is not in visited",
                   "D_V(b->first) is the least h >= 1", "avail(x_i) for", "first itself is visited; it is the target only",
                   "additionally masked when D_V(b->first) > budget", "Unreachable counts as > budget",
                   "additionally masked when cycle_len[w][b] > budget", "would need one search per candidate", "out of scope",
                   "The dead-end vote sees padding, kv_len, visited and this mask", "Terminators are re-opened on a dead end",
                   "only be raised at a position whose previous position opened the current loop",
                   "Every row without dead_end that reaches a terminator has a closed state", "D_V >= D", "L + ntok <= 2048",
                   "T > 256", "CONNECT or NO_REPEAT clear"):
        assert phrase in doc, phrase
    assert re.search(r"typedef struct ff_constrain_exact_params \{\s*int flags;\s*const unsigned int\* follows;\s*"
                     r"const unsigned char\* cycle_len;\s*float\* logprob;\s*int\* dead_end;\s*\} ff_constrain_exact_params;", code)
    assert not re.search(r"#define\s+FF_CONSTRAIN_\w+\s+4\b", code)                          # no new flag bit

    def args(name):
        return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert args("ff_decode_constrained_exact").count(",") == args("ff_decode_constrained").count(",")
    assert "const ff_constrain_exact_params* exact" in args("ff_decode_constrained_exact")
    assert args("ff_decode_constrained_exact_workspace_bytes") == args("ff_decode_constrained_workspace_bytes")
    assert args("ff_pointer_constrained_exact").count(",") == args("ff_pointer_constrained").count(",") + 2
    tail = [a.strip() for a in args("ff_pointer_constrained_exact").split(",")[-3:]]
    assert tail == ["const unsigned char* cycle_len", "int budget", "ff_stream_t stream"]
    for name in ("ff_constrain.hip", "ff_select.h"):
        src = open(os.path.join(ROOT, "faceformer_amd", "csrc", name)).read()
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", src, flags=re.M), name   # no preprocessor conditionals
    constrain = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain.hip")).read()
    assert "template <int FORM>" in constrain and "pointer_constrained_form_kernel<FF_LOOP_EXACT>" in constrain  # a third form of the launch
    select = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_select.h")).read()
    assert select.count("ff_loop_write_row(") == 1 and "ff_loop_closure_reach(" in select    # the rule stays in one place


def test_binding_lists_the_exact_entries_and_refuses_a_library_without_them(monkeypatch):
    from faceformer_amd.hip import lib, modes
    assert lib.FF_ABI_VERSION == 105
    S = lib.SIGNATURES
    for name in NEW_ENTRIES:
        assert name in S, name
    assert len(S["ff_decode_constrained_exact"][1]) == len(S["ff_decode_constrained"][1])
    assert S["ff_decode_constrained_exact_workspace_bytes"] == S["ff_decode_constrained_workspace_bytes"]
    assert S["ff_pointer_constrained_exact"][1][:-1] == S["ff_pointer_constrained"][1][:-1] + [lib.fptr, lib.C.c_int]
    assert [f for f, _ in lib.ConstrainExactParams._fields_] == ["flags", "follows", "cycle_len", "logprob", "dead_end"]
    rec = modes.CONSTRAIN_EXACT
    assert rec not in modes.MODES and rec.entry == "ff_decode_constrained_exact" and rec.subject == "constrain_exact"
    assert rec.excludes == modes.CONSTRAIN.excludes and rec.outs == modes.CONSTRAIN.outs and rec.switches == modes.CONSTRAIN.switches
    assert [n for n, _ in rec.own] == ["follow_table", "cycle_len"] and not rec.per_anchor
    opts = dict(constrain=LOOPS, num_samples=0, beam_width=0)
    assert modes.of_options(False, 0, False, True, **opts) == (rec, LOOPS)
    assert modes.of_options(constrain_exact=True, **opts) == (rec, LOOPS)
    assert modes.of_options(False, 0, True, **opts) == (modes.CONSTRAIN_AHEAD, LOOPS)          # the signatures of today still hold
    assert modes.of_options(False, 0, **opts) == (modes.CONSTRAIN, LOOPS) and modes.of_options(**opts) == (modes.CONSTRAIN, LOOPS)
    import _ctypes
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


def test_a_library_without_only_the_new_entries_is_refused(monkeypatch):
    """The parent's library exports everything but the three new entries: load() names the first one it misses."""
    from faceformer_amd.hip import lib

    class Old:
        def __getattr__(self, name):
            if name in NEW_ENTRIES:
                raise AttributeError(name)
            return types.SimpleNamespace(restype=None, argtypes=None)
    monkeypatch.setattr(lib.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="does not export ff_pointer_constrained_exact .*rebuild"):
        lib.load()


def test_c_entries_reject_bad_arguments_before_any_launch(hip_lib):
    """FF_ERR_ARG with the offending argument named, on a host without a GPU: the checks run in front of every HIP call."""
    import ctypes as C
    from faceformer_amd.hip import lib
    FF_ERR_ARG = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def step(flags=LOOPS, cyc=p, budget=3, S=8, L=4):
        return hip_lib.ff_pointer_constrained_exact(p, S, S, None, None, 2, 1, p, L, flags, 4, 1, 4, p, p, p, p, p, p, p, p, p, p, p,
                                                    None, 0, None, 0, None, None, cyc, budget, None)
    for kw, text in ((dict(flags=CR.NO_REPEAT), b"FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT"),
                     (dict(flags=CR.CONNECT), b"FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT"), (dict(flags=0), b"FF_CONSTRAIN_NO_REPEAT"),
                     (dict(cyc=None), b"cycle_len"), (dict(budget=-1), b"budget"), (dict(budget=255), b"budget"),
                     (dict(flags=4 | LOOPS), b"unknown flag bits"), (dict(S=2049, L=2045), b"S=2049 above 2048")):
        assert step(**kw) == FF_ERR_ARG and text in hip_lib.ff_last_error(), (kw, hip_lib.ff_last_error())
        assert b"ff_pointer_constrained_exact" in hip_lib.ff_last_error()
    m, prm = lib.Model(), lib.DecodeParams()
    m.num_token = 4
    prm.variant, prm.N, prm.L, prm.F, prm.T, prm.term_lo, prm.term_hi = lib.FF_PARALLEL, 1, 4, 4, 6, 1, 4

    def decode(prm=prm, extra=None, best=None, **fields):
        a = lib.ConstrainExactParams(LOOPS, p, p, p, p)
        for k, v in fields.items():
            setattr(a, k, v)
        return hip_lib.ff_decode_constrained_exact(C.byref(m), C.byref(prm), p, p, p, p, None, extra, p, None, None, None, None, best,
                                                   None, p, p, 1024, C.byref(a), None)
    for fields, text in ((dict(flags=CR.NO_REPEAT), b"FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT"),
                         (dict(flags=CR.CONNECT), b"FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT"), (dict(flags=0), b"FF_CONSTRAIN_CONNECT"),
                         (dict(flags=4 | LOOPS), b"unknown flag bits"), (dict(follows=None), b"follow table"),
                         (dict(cycle_len=None), b"cycle_len"),
                         (dict(logprob=None), b"logprob and dead_end"), (dict(dead_end=None), b"logprob and dead_end"),
                         (dict(extra=p), b"extra mask"), (dict(best=p), b"best / second")):
        assert decode(**fields) == FF_ERR_ARG and text in hip_lib.ff_last_error(), fields
        assert b"ff_decode_constrained_exact" in hip_lib.ff_last_error()

    def changed(**kw):
        q = lib.DecodeParams()
        C.memmove(C.byref(q), C.byref(prm), C.sizeof(prm))
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    for kw, text in ((dict(T=257), b"T=257"), (dict(L=2045), b"L=2045 above 2044"), (dict(variant=lib.FF_SEQ2SEQ), b"parallel-variant"),
                     (dict(flags=lib.FF_RETIRE_FINISHED), b"excludes"), (dict(flags=lib.FF_RETURN_POINTER), b"excludes"),
                     (dict(flags=lib.FF_NO_STOP), b"excludes"), (dict(term_lo=4), b"terminator range"), (dict(term_hi=5), b"terminator range")):
        assert decode(prm=changed(**kw)) == FF_ERR_ARG and text in hip_lib.ff_last_error(), kw
    assert hip_lib.ff_decode_constrained_exact(None, None, p, p, p, p, None, None, p, None, None, None, None, None, None, p, p, 1024,
                                               None, None) == FF_ERR_ARG


def test_every_rejected_combination_raises_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine, modes, ops
    lib = _untouchable(monkeypatch)
    assert modes.constrain_exact_value(False, None) is False and modes.constrain_exact_value(None, LOOPS, 4, True) is False
    assert modes.constrain_exact_value(True, LOOPS) is True
    with pytest.raises(ValueError, match="constrain_exact needs constrain='loops': it is the exact closure look-ahead"):
        modes.constrain_exact_value(True, None)
    for flags in (0, CR.NO_REPEAT, CR.CONNECT):
        with pytest.raises(ValueError, match="constrain_exact needs constrain='loops' \\(FF_CONSTRAIN_NO_REPEAT \\| FF_CONSTRAIN_CONNECT\\)"):
            modes.constrain_exact_value(True, flags)
    with pytest.raises(ValueError, match="constrain_exact excludes constrain_lookahead: it contains it"):
        modes.constrain_exact_value(True, LOOPS, 0, True)
    with pytest.raises(ValueError, match="constrain_exact excludes constrain_beams"):
        modes.constrain_exact_value(True, LOOPS, 2)
    # PathEngine.decode itself, on an engine object without a constructor call: nothing of it may be needed
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    table = torch.zeros(2, 8, 1, dtype=torch.int32)
    close, cyc = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.uint8)
    ok = dict(T=5, F=4, num_input=[4, 3], constrain="loops", term_range=TERM, follow_table=table, constrain_exact=True, cycle_len=cyc)
    decode = lambda **change: eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, **change))
    for change, text in (
            (dict(constrain=None), "constrain_exact needs constrain='loops': it is the exact closure look-ahead"),
            (dict(constrain="no_repeat"), "constrain_exact needs constrain='loops' \\(FF_CONSTRAIN_NO_REPEAT \\| FF_CONSTRAIN_CONNECT\\)"),
            (dict(constrain=2), "constrain_exact needs constrain='loops' \\(FF_CONSTRAIN_NO_REPEAT \\| FF_CONSTRAIN_CONNECT\\)"),
            (dict(constrain=0), "constrain_exact needs constrain='loops' \\(FF_CONSTRAIN_NO_REPEAT \\| FF_CONSTRAIN_CONNECT\\)"),
            (dict(constrain_lookahead=True, close_dist=close), "constrain_exact excludes constrain_lookahead: it contains it"),
            (dict(constrain_beams=2), "constrain_exact excludes constrain_beams"),
            (dict(cycle_len=None), "constrain_exact needs cycle_len"),
            (dict(follow_table=None), "constrain='loops' needs follow_table"),
            (dict(T=257), "constrain_exact takes T <= 256 \\(got 257\\)"),
            (dict(cycle_len=torch.zeros(2, 9, dtype=torch.uint8)), "cycle_len must be a uint8 tensor of shape \\[2, 8\\]"),
            (dict(cycle_len=torch.zeros(1, 8, dtype=torch.uint8)), "cycle_len must be a uint8 tensor of shape \\[2, 8\\]"),
            (dict(cycle_len=torch.zeros(2, 8, dtype=torch.int8)), "cycle_len must be a uint8 tensor of shape \\[2, 8\\]"),
            (dict(cycle_len=cyc.numpy()), "cycle_len must be a uint8 tensor of shape \\[2, 8\\]"),
            (dict(follow_table=torch.zeros(2, 8, 2, dtype=torch.int32)), "follow_table must be an int32 tensor of shape \\[2, 8, 1\\]"),
            # everything the constrained decode excludes, in its record's words
            (dict(retire=True), "constrain_exact excludes retire, "), (dict(return_pointer=True), "constrain_exact excludes"),
            (dict(no_stop=True), "constrain_exact excludes"), (dict(stop_callback=lambda c: False), "constrain_exact excludes"),
            (dict(extra_mask=torch.zeros(8, 12, dtype=torch.uint8)), "constrain_exact excludes"),
            (dict(logprob=True), "constrain_exact excludes"), (dict(beam_width=2), "beam_width and num_samples"),
            (dict(num_samples=2, uniforms=torch.zeros(4, 16)), "beam_width and num_samples"),
            (dict(term_range=None), "constrain_exact needs term_range"), (dict(term_range=(4, 4)), "constrain_exact needs term_range")):
        with pytest.raises(ValueError, match=text):
            decode(**change)
    with pytest.raises(ValueError, match="constrain_exact is a parallel-variant option"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **ok)
    with pytest.raises(ValueError, match="constrain_exact takes at most 2044 edges per wireframe \\(got 2045\\)"):
        eng.decode(torch.zeros(1, 2049, 8), None, None, lib.FF_PARALLEL, **dict(
            ok, num_input=[4], follow_table=torch.zeros(1, 2045, 64, dtype=torch.int32), cycle_len=torch.zeros(1, 2045, dtype=torch.uint8)))
    # the texts of the look-ahead stay as they are
    with pytest.raises(ValueError, match="constrain_lookahead needs constrain='loops': it is the closure look-ahead"):
        decode(constrain=None, constrain_exact=False, constrain_lookahead=True)
    assert ops.EXACT_MAX_KEYS == modes.EXACT_MAX_KEYS == 2048


def test_models_reject_exact_combinations_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        assert not model.engine_supported() and model.constrain_exact is False
        model.constrain, model.constrain_exact = "loops", True
        inputs = _tiny_inputs()
        with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact needs the native engine"):
            model.forward_eval(inputs)
        assert "predict" not in inputs
    model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert model.constrain_exact is False and type(model.constrain_exact) is bool
    model.constrain_exact = True
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact needs constrain='loops': it is the exact closure look-ahead"):
        model.forward_eval(_tiny_inputs())
    model.constrain = "no_repeat"
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact needs constrain='loops' \\(FF_CONSTRAIN_NO_REPEAT"):
        model.forward_eval(_tiny_inputs())
    model.constrain, model.constrain_lookahead = "loops", True
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact excludes constrain_lookahead: it contains it"):
        model.forward_eval(_tiny_inputs())
    model.constrain_lookahead, model.constrain_beams = False, 2
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact excludes constrain_beams"):
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
    for bad in (torch.zeros(1, 7, dtype=torch.uint8), torch.zeros(1, 8, dtype=torch.int32), np.zeros((2, 8), dtype=np.uint8)):
        with torch.no_grad(), pytest.raises(ValueError, match="cycle_len must be uint8 \\[1, 8\\]"):
            model.forward_eval(dict(_tiny_inputs(), cycle_len=bad))
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact takes at most 2044 edges per wireframe \\(got 2045\\)"):
        model.forward_eval(dict(_tiny_inputs(), input=torch.zeros(1, 2045, 50, 2)))       # (the key count, before the encoder runs)
    long = _tiny_model(SurfaceFormer_Parallel, max_face_length=257)
    long.constrain, long.constrain_exact = "loops", True
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact takes T <= 256 \\(got 257\\)"):
        long.forward_eval(_tiny_inputs())
    with pytest.raises(ValueError, match="score\\(\\) excludes constrain"):
        model.score(_tiny_inputs(), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.constrain_exact is False
    seq.constrain_exact = True
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_exact is a SurfaceFormer_Parallel option"):
        seq.forward_eval({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})


def test_decode_sharded_rejects_exact_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain="loops",
                                  constrain_exact=True)
    with pytest.raises(ValueError, match="decode_sharded does not implement constrain_exact"):
        dist.decode_sharded(model, {}, NoDist())
    model.constrain = None                                         # (the option alone is an error anywhere)
    with pytest.raises(ValueError, match="decode_sharded does not implement constrain_exact"):
        dist.decode_sharded(model, {}, NoDist())
    model.constrain_exact = False
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


def test_cli_exact_flag_reaches_the_model_and_the_record_is_todays_without_it(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd import datasets as D
    parse = cli.build_parser().parse_args
    assert parse(["--test_ckpt", "x.ckpt", "--constrain", "loops", "--constrain-exact"]).constrain_exact is True
    assert parse(["--test_ckpt", "x.ckpt", "--constrain", "loops"]).constrain_exact is False
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--constrain", "loops", "--constrain-exact", "--test_ckpt", "unused.ckpt"])
    cli.main(["--constrain", "loops", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["constrain"], kw["constrain_exact"], kw["constrain_lookahead"]) for kw in seen] == [
        ("loops", True, False), ("loops", False, False), (None, False, False)]
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3, constrain_exact=True)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3, constrain_exact=True)
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3)                            # without the flag: today's attributes
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    cfg = types.SimpleNamespace(model_class="SurfaceFormer_Parallel")
    call = lambda **kw: run_test(cfg, None, out_dir="unused", device="cpu", model=object(), constrain_exact=True, **kw)
    for kw in (dict(), dict(constrain="no_repeat")):
        with pytest.raises(ValueError, match="--constrain-exact requires --constrain loops"):
            call(**kw)
    with pytest.raises(ValueError, match="--constrain-exact is not combined with --constrain-lookahead: it contains it"):
        call(constrain="loops", constrain_lookahead=True)
    with pytest.raises(ValueError, match="--constrain-exact is not implemented with --constrain-beams"):
        call(constrain="loops", constrain_beams=2)
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--constrain-exact is not implemented for multi-rank runs"):
        call(constrain="loops", dist_mod=world2)
    for kw in (dict(scores=True), dict(beam=2), dict(retire_finished=True), dict(score_labels=True), dict(sample=2)):
        with pytest.raises(ValueError, match="--constrain"):
            call(constrain="loops", **kw)
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


# ---- GPU: the operator ------------------------------------------------------------------------------------------------------------
SPG = 3
BUDGETS = (0, 1, 2, 5, 254)
KINDS = ("lattice", "ring", "chain", "self-closing", "random", "trap")


def _table(kind, L, seed):
    """One wireframe's follow table bool [L, L]."""
    if L == 0:
        return np.zeros((0, 0), dtype=bool)
    if kind == "lattice":
        lat, _, _ = CR.lattice_batch([L], L, 5, seed)
        return faces.follow_table(lat["input"].numpy(), CR.TOL, [L])[0]
    if kind == "random":
        return CR.random_follows(1, L, seed)[0]
    return {"ring": LR.ring, "chain": LR.chain, "self-closing": ER.self_closing, "trap": ER.trap}[kind](L)


def _case(B, S, seed, kinds, group, long_walk=None):
    """Rows in every state, each the state of a random walk of the rule on its wireframe's table (so visited is consistent):
    b % 5 = 0 open, 1 closed, 2 finished (row 2) or closed, 3 open after a long walk, 4 closed after a long walk.  Wireframe w
    has table kinds[w % 3].  The wireframes of group 0: kv_len = S - 2, whole, every key masked; of group 1 (ragged): L // 2,
    L - 1 and 0 edges, the keys beyond them masked, no bit of the table beyond them; of group 2: whole, a single live key, 1
    edge.  long_walk: the length of the long walks (default: all but at most 40 edges).  -> dict of CPU data."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng([seed, B, S])
    ntok = NTOK if S > NTOK else S
    term = TERM if ntok == NTOK else (0, ntok)
    L = S - ntok
    W = (B + SPG - 1) // SPG
    logits = torch.randn(B, S, generator=g) * 3.0
    if B >= 4:
        logits[B - 1] = 0.75                                             # all-equal logits: ties
    mask = torch.rand(W, S, generator=g) < 0.03                          # (little random padding: it cuts the long paths)
    mask[:, :ntok] = False
    kv = torch.full((W,), S, dtype=torch.int32)
    ni = [L] * W
    if group == 0:
        kv[0] = max(1, S - 2)
        if W > 2:
            kv[2] = 0
    elif group == 1:
        ni = [n for n in (L // 2, max(L - 1, 0), 0)][:W]
    else:
        if W > 1:
            mask[1] = True
            mask[1, S - 1 if L else 0] = False
        if W > 2:
            ni[2] = min(L, 1)
    for w in range(W):
        mask[w, ntok + ni[w]:] = True
    follows = np.zeros((W, L, L), dtype=bool)
    for w in range(W):                                                   # (the table of the wireframe's own edges: a ring stays one)
        follows[w, :ni[w], :ni[w]] = _table(kinds[w % 3], ni[w], seed + w)
    fin = np.zeros(B, dtype=np.int32)
    first = np.full(B, -1, dtype=np.int32)
    prev = np.full(B, -1, dtype=np.int32)
    visited = np.zeros((B, L), dtype=bool)
    for b in range(B):
        w, kind = b // SPG, b % 5
        if ni[w] == 0:
            continue
        steps = int(rng.integers(1, 6)) if kind < 3 else (long_walk or int(rng.integers(max(1, ni[w] - 40), ni[w] + 1)))
        walk = ER.walk_states(follows[w], rng.integers(0, ni[w]), steps, rng)
        want_open = kind in (0, 3)
        hit = [st for st in walk if (st[1] is not None) == want_open]
        vis, f, p = hit[-1] if hit else walk[-1]
        visited[b, sorted(vis)] = True
        first[b], prev[b] = -1 if f is None else f, -1 if p is None else p
    if B > 2:
        fin[2] = 1
    memory = torch.randn(W, S, 64, generator=g)
    wf = torch.arange(B) // SPG
    pad = (mask[wf] | (torch.arange(S)[None, :] >= kv[wf, None])).numpy()
    return dict(logits=logits, mask=mask, kv=kv, follows=follows, fin=fin, first=first, prev=prev, visited=visited, memory=memory,
                pad=pad, ntok=ntok, term=term, L=L, W=W, ni=ni)


def _on_gpu(c):
    """The case's operands on the device, and the two distance tables of its follows (ops.follow_distance, hmax 254)."""
    from faceformer_amd.hip import ops
    d = dict(fin=torch.from_numpy(c["fin"]).cuda(), first=torch.from_numpy(c["first"]).cuda(), prev=torch.from_numpy(c["prev"]).cuda(),
             visited=torch.from_numpy(faces.pack_follow_bits(c["visited"])).cuda(),
             follows=torch.from_numpy(faces.pack_follow_bits(c["follows"])).cuda(), memory=c["memory"].cuda(),
             mask=c["mask"].to(torch.uint8).cuda(), kv=c["kv"].cuda())
    if c["L"]:
        d["close"], d["cycle"] = ops.follow_distance(d["follows"], torch.tensor(c["ni"], dtype=torch.int32).cuda(), 254)
    else:
        d["close"] = torch.zeros((c["W"], 0, 0), dtype=torch.uint8).cuda()
        d["cycle"] = torch.zeros((c["W"], 0), dtype=torch.uint8).cuda()
    return d


def _run_exact(c, d, budget, ahead=False, **kw):
    from faceformer_amd.hip import ops
    lg = c["logits"].clone().cuda()
    common = dict(memory=d["memory"], mask=d["mask"], kv_len=d["kv"], seqs_per_group=SPG, term_range=c["term"], want_rows=True,
                  want_stats=True, **kw)
    if ahead:
        res = ops.pointer_constrained_ahead(lg, d["fin"], d["first"], d["prev"], d["visited"], LOOPS, c["ntok"], d["follows"], d["close"],
                                            d["cycle"], budget, **common)
    else:
        res = ops.pointer_constrained_exact(lg, d["fin"], d["first"], d["prev"], d["visited"], LOOPS, c["ntok"], d["follows"], d["cycle"],
                                            budget, **common)
    return lg, res


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 63, 64, 65, 260, 1028, 2048])
def test_operator_against_the_numpy_rule(hip_lib, S):
    """S = 2048 is the entries' limit: 32 chunks (every bit of the per-lane words) and fw = 64 (every lane a frontier word).  There
    the long walks are 200 edges, to keep the case's numpy side short."""
    from test_constrain import _bits_to_bool
    from faceformer_amd.hip import ops
    seen = dict(open=0, closed=0, dead=0, finished=0, nolive=0, exact=0, exact_dead=0, deep=0, high=0)
    at_limit = S == ops.EXACT_MAX_KEYS
    for bi, B in enumerate((1, 3, 9)):
        for group in (0, 1, 2):
            pool = (KINDS[:3], KINDS[3:], ("ring", "lattice", "random"))[group]
            kinds = [pool[(w + bi) % 3] for w in range(3)]
            c = _case(B, S, 100 * S + 10 * B + group, kinds, group, long_walk=200 if at_limit else None)
            d = _on_gpu(c)
            ntok, term, L = c["ntok"], c["term"], c["L"]
            raw = c["logits"].numpy()
            cycle = d["cycle"].cpu().numpy()
            for budget in BUDGETS:
                counter = torch.zeros(1, dtype=torch.int32).cuda()
                lg, res = _run_exact(c, d, budget, counter=counter)
                la, ra = _run_exact(c, d, budget, ahead=True)
                own = lg.cpu().numpy()
                got = {k: res[k].cpu().numpy() for k in ("next", "logprob", "fin", "dead_end", "first", "prev")}
                vis = _bits_to_bool(res["visited"], L) if L else np.zeros((B, 0), dtype=bool)
                rows = res["mask_rows"].cpu().numpy() != 0
                rows_a = ra["mask_rows"].cpu().numpy() != 0
                what = (S, B, group, budget)
                nge = 0
                for b in range(B):
                    w = b // SPG
                    st = (frozenset(np.flatnonzero(c["visited"][b]).tolist()), None if c["first"][b] < 0 else int(c["first"][b]),
                          None if c["prev"][b] < 0 else int(c["prev"][b]))
                    is_open = st[1] is not None and st[2] is not None
                    r = ER.step_row(raw[b].astype(np.float64), c["pad"][b], st, ntok, term, c["follows"][w], cycle[w], budget,
                                    finished=bool(c["fin"][b]))
                    if c["fin"][b]:
                        assert np.array_equal(own[b], raw[b]), what                                # finished rows untouched
                        assert got["logprob"][b] == 0.0
                        seen["finished"] += 1
                    else:
                        hidden = r["masked"] | c["pad"][b]
                        assert np.array_equal(rows[b], r["masked"]), (what, b, kinds[w % 3])       # the byte row: the rule's own mask
                        assert np.array_equal(own[b] == np.float32(FILL), hidden), (what, b)       # the FILL pattern: the allowed set
                        assert np.array_equal(own[b][~hidden], raw[b][~hidden]), (what, b)
                        want_lp = CR.select(own[b].astype(np.float64))[1]
                        assert abs(float(got["logprob"][b]) - want_lp) <= CR.LP_BAR, (what, b, got["logprob"][b], want_lp)
                        if is_open:                                                                # a superset of the look-ahead's edge keys
                            assert not (rows_a[b, ntok:] & ~rows[b, ntok:]).any(), (what, b)
                            more = rows[b, ntok:] & ~rows_a[b, ntok:]
                            seen["exact"] += bool(more.any())
                            seen["high"] += bool((~rows[b, 17 * 64:]).any())                       # a live key beyond chunk 16
                            seen["exact_dead"] += bool(r["dead"] and not ra["dead_end"][b].item())
                            if L and budget > 2:                                                   # reached beyond the second level
                                dist = ER.closing_distance(st, c["follows"][w], c["pad"][b][ntok:], budget)
                                seen["deep"] += bool(((dist > 2) & (dist <= budget) & ~r["masked"][ntok:]).any())
                        else:                                                                      # closed: the look-ahead's row, byte for byte
                            assert np.array_equal(rows[b], rows_a[b]), (what, b)
                            assert np.array_equal(own[b], la[b].cpu().numpy()), (what, b)
                        seen["dead" if r["dead"] else ("open" if is_open else "closed")] += 1
                        seen["nolive"] += bool(hidden.all())
                        nge += r["tok"] >= ntok
                    assert got["next"][b] == r["tok"], (what, b, got["next"][b], r["tok"])        # exact, ties included
                    assert bool(got["fin"][b]) == r["fin"] and bool(got["dead_end"][b]) == r["dead"], (what, b)
                    nv, nf, npv = r["state"]
                    assert (got["first"][b], got["prev"][b]) == (-1 if nf is None else nf, -1 if npv is None else npv), (what, b)
                    assert set(np.flatnonzero(vis[b]).tolist()) == set(nv), (what, b)
                assert int(counter.item()) == nge, what
                forced = ops.pointer_forced(c["logits"].clone().cuda(), res["next"], d["memory"], d["mask"], d["kv"], seqs_per_group=SPG,
                                            want_rows=True, want_stats=True)
                assert torch.equal(res["rows"], forced["rows"]) and torch.equal(res["stats"], forced["stats"]), what
                lg2, res2 = _run_exact(c, d, budget)                                               # two launches: bit-equal
                assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
    print("S=%d rows by state:" % S, seen)
    if S >= 63:
        assert all(v > 0 for k, v in seen.items() if k not in ("exact_dead", "high")), seen      # every state was exercised
    if at_limit:
        assert seen["high"] > 0, seen                                                            # reach bits 17..31 decided a byte


@pytest.mark.gpu
def test_the_trap_selects_edge_2(hip_lib):
    """The test that fails without the feature: on the trap the look-ahead operator selects edge 3, the exact one edge 2."""
    from faceformer_amd.hip import ops
    t = ER.trap()
    S = NTOK + 4
    logits = torch.zeros(1, S)
    logits[0, NTOK + 3] = 5.0
    bits = torch.from_numpy(faces.pack_follow_bits(t[None])).cuda()
    close, cyc = ops.follow_distance(bits, torch.tensor([4], dtype=torch.int32).cuda(), 254)
    vis = np.zeros((1, 4), dtype=bool)
    vis[0, [0, 1]] = True
    state = [torch.tensor([v], dtype=torch.int32).cuda() for v in (0, 0, 1)] + [torch.from_numpy(faces.pack_follow_bits(vis)).cuda()]
    for budget in (3, 5, 254):
        ahead = ops.pointer_constrained_ahead(logits.clone().cuda(), *state, LOOPS, NTOK, bits, close, cyc, budget, term_range=TERM)
        exact = ops.pointer_constrained_exact(logits.clone().cuda(), *state, LOOPS, NTOK, bits, cyc, budget, term_range=TERM)
        assert int(ahead["next"][0]) == NTOK + 3 and int(exact["next"][0]) == NTOK + 2, budget
        assert exact["mask_rows"][0, NTOK:].tolist() == [1, 1, 0, 1] and ahead["mask_rows"][0, NTOK:].tolist() == [1, 1, 0, 0]
        assert (int(exact["first"][0]), int(exact["prev"][0]), int(exact["dead_end"][0]), int(exact["fin"][0])) == (-1, 2, 0, 0)
        nxt = ops.pointer_constrained_ahead(logits.clone().cuda(), ahead["fin"], ahead["first"], ahead["prev"], ahead["visited"], LOOPS, NTOK,
                                            bits, close, cyc, budget - 1, term_range=TERM)
        assert int(nxt["dead_end"][0]) == 1                                                     # the look-ahead dead-ends one step later
    with pytest.raises(ValueError, match="at most 2048 keys"):
        ops.pointer_constrained_exact(torch.zeros(1, 2049).cuda(), *state[:3], torch.zeros(1, 64, dtype=torch.int32).cuda(), LOOPS, NTOK,
                                      torch.zeros(1, 2045, 64, dtype=torch.int32).cuda(), torch.zeros(1, 2045, dtype=torch.uint8).cuda(), 3)
    with pytest.raises(ValueError, match="FF_CONSTRAIN_NO_REPEAT \\| FF_CONSTRAIN_CONNECT"):
        ops.pointer_constrained_exact(logits.clone().cuda(), *state, CR.CONNECT, NTOK, bits, cyc, 3, term_range=TERM)
    with pytest.raises(TypeError, match="close_dist must be a tensor"):                       # a missing table is no switch to the exact rule
        ops.pointer_constrained_ahead(logits.clone().cuda(), *state, LOOPS, NTOK, bits, None, cyc, 3, term_range=TERM)
    with pytest.raises(TypeError, match="cycle_len must be a tensor"):
        ops.pointer_constrained_exact(logits.clone().cuda(), *state, LOOPS, NTOK, bits, None, 3, term_range=TERM)


# ---- GPU: the engine --------------------------------------------------------------------------------------------------------------
ENGINE_GOLDENS = ["par_small_gain4", "par_small_ragged", "par_full_n40_gain4"]


def _tables(name):
    """(bits, close_dist, cycle_len) on the GPU for the lattice of `name`, as the model builds them (test_lookahead holds them to
    faces.follow_distance); the exact decode reads bits and cycle_len, the comparisons with the look-ahead close_dist too."""
    from test_lookahead import _tables as tables
    assert ER.LATTICE_SEEDS[name] == CR.LATTICE_SEEDS[name]              # (test_constrain._model builds the lattice of that seed)
    return tables(name)


def _exact(model, case, b, tables, **kw):
    from test_logprob import _decode
    return _decode(model, case, b, constrain=LOOPS, follow_table=tables[0], term_range=TERM, constrain_exact=True, cycle_len=tables[2], **kw)


def _replay(out, table, tables, F, T, what):
    """The numpy rule on the decode's own tokens, traced logits and cycle_len: at every (step, unfinished sequence) the FILL
    pattern, the argmax token and the flags; none is left out.  Returns (pairs, margins [steps, rows] of the constrained row, inf
    where finished, pairs at which the exact rule masked an edge key the look-ahead leaves live)."""
    from test_constrain import _check_layout
    pred, lp, fin, steps = _check_layout(out, T)
    close, cyc = tables[1].cpu().numpy(), tables[2].cpu().numpy()
    logits = out["logits"].cpu().numpy()
    dead = out["dead_end"].cpu().numpy() != 0
    want_dead = np.zeros(pred.shape[0], dtype=bool)
    margins = np.full((steps, pred.shape[0]), np.inf)
    pairs = more = 0
    for j in range(steps):
        budget = T - 2 - j                                                                    # the step selects position j + 1
        for r in np.flatnonzero(fin > j):
            w = r // F
            st = CR.state_of_prefix(pred[r, : j + 1], NTOK, table[w])
            row = logits[j, r]
            pad = out["_pad"][w]
            masked, is_dead = ER.rule_mask(st, row.size, NTOK, TERM, table[w], pad, cyc[w], budget)
            assert np.array_equal(row == np.float32(FILL), masked | pad), (what, j, int(r))
            tok, own_lp = CR.select(row.astype(np.float64))
            assert pred[r, j + 1] == tok, (what, j, int(r), int(pred[r, j + 1]), tok)
            assert abs(lp[r, j + 1] - own_lp) <= CR.LP_BAR, (what, j, int(r))
            want_dead[r] |= is_dead
            if is_dead:
                assert fin[r] == j + 1, (what, j, int(r))
            ahead = LR.rule_mask(st, LOOPS, row.size, NTOK, TERM, table[w], pad, close[w], cyc[w], budget)[0]
            assert not (ahead[NTOK:] & ~masked[NTOK:]).any(), (what, j, int(r))               # contains the look-ahead
            more += bool((masked[NTOK:] & ~ahead[NTOK:]).any())
            live = np.sort(row[row > np.float32(FILL)].astype(np.float64))
            margins[j, r] = live[-1] - live[-2] if live.size > 1 else np.inf
            pairs += 1
    assert np.array_equal(dead, want_dead), what
    return pairs, margins, more


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_replays_under_the_numpy_rule(hip_lib, name):
    from test_constrain import _model, _with_pad
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T, F = case["model"]["seq_len"], max(lat["num_input"])
    tables = _tables(name)
    out = _with_pad(_exact(model, case, b, tables, trace=True), b)
    pairs, _, more = _replay(out, table, tables, F, T, name)
    print(name, "steps=%d, %d (step, sequence) pairs replayed, none left out; the exact rule masked more than the look-ahead at %d; "
          "dead ends: %d" % (out["steps"], pairs, more, int(out["dead_end"].sum())))
    assert pairs > 0


def _yield(pred, dead, ni, edges, F):
    from test_constrain import _yield as count
    return count(pred, dead, ni, edges, F)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_the_guarantee_and_the_yield_against_the_lookahead(hip_lib, name):
    """On every own-anchor row: no dead end other than right after a loop-opening position, every row that ends in a terminator
    without the flag is enclosed, no edge twice; and at least as many rows end enclosed as under the static look-ahead."""
    from test_constrain import _check_layout, _model
    from test_lookahead import _ahead
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, F = case["model"]["seq_len"], max(ni)
    tables = _tables(name)
    out = _exact(model, case, b, tables)
    pred, _, fin, steps = _check_layout(out, T)
    dead = out["dead_end"].cpu().numpy() != 0
    own = np.zeros(pred.shape[0], dtype=bool)
    enclosed = 0
    for w, n in enumerate(ni):
        own[w * F: w * F + n] = True
        for f in range(n):
            r = w * F + f
            row = pred[r]
            idx = [int(t) - NTOK for t in row if t >= NTOK]
            assert len(idx) == len(set(idx)), (name, w, f, row)                              # no row holds an edge twice
            if ((row >= TERM[0]) & (row < TERM[1])).any() and not dead[r]:
                last = int(min(fin[r], steps))
                assert CR.state_of_prefix(row[: last + 1], NTOK, table[w])[1] is None, (name, w, f, row)   # a closed state
                face = faces._parallel_rows(row[None], TOK, n)
                if face:                                                                     # (an anchor below ntok that ends at once has no edge)
                    assert faces.is_face_enclosed(edges[w], face[0][1], CR.TOL), (name, w, f, row)
                    enclosed += 1
        late = ER.late_dead_ends(pred[w * F:(w + 1) * F], (dead & own)[w * F:(w + 1) * F], NTOK, table[w])
        assert not late, (name, w, late, pred[w * F:(w + 1) * F][late])                      # the guarantee
    ahead = _ahead(model, case, b, tables)
    pa, da = ahead["predict"].cpu().numpy(), ahead["dead_end"].cpu().numpy() != 0
    late_ahead = sum(len(ER.late_dead_ends(pa[w * F:(w + 1) * F], (da & own)[w * F:(w + 1) * F], NTOK, table[w])) for w in range(len(ni)))
    before, after = _yield(pa, da, ni, edges, F), _yield(pred, dead, ni, edges, F)
    print(name, "enclosed / dead end / other of %d own-anchor rows: look-ahead %d / %d / %d (late dead ends %d), exact %d / %d / %d (late 0)"
          % ((sum(ni),) + before + (late_ahead,) + after))
    assert after[0] == enclosed
    assert after[0] >= before[0], (name, after, before)
    if name in ER.STRICT:
        assert after[0] > before[0], (name, after, before)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_against_the_teacher_forced_oracle(hip_lib, name):
    from test_constrain import _check_against_oracle, _model, _with_pad
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    out = _with_pad(_exact(model, case, b, _tables(name), trace=True), b)
    left, pairs, _ = _check_against_oracle(name, case, sd, lat, out, what="exact " + name)
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
    whole = _with_pad(_exact(model, case, b, tables, trace=True, chunk_wireframes=0), b)
    again = _exact(model, case, b, tables, trace=True, chunk_wireframes=0)
    for k in ("predict", "logprob", "dead_end"):
        assert torch.equal(whole[k], again[k]), k                                    # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"] and torch.equal(whole["logits"].nan_to_num(7.0), again["logits"].nan_to_num(7.0))
    one = _with_pad(_exact(model, case, b, tables, trace=True, chunk_wireframes=1), b)  # (cycle_len offset per chunk)
    _, mw, _ = _replay(whole, table, tables, F, T, "whole")
    _, mo, _ = _replay(one, table, tables, F, T, "one")
    lw = whole["logits"].cpu().numpy()
    fin_w = CR.stop_and_finish(whole["predict"].cpu().numpy(), TERM, NTOK)[0]
    tol_of = lambda j: _tol(lw[j][fin_w > j]) if (fin_w > j).any() else 0.0
    full = _same_on_decisive_pairs(whole["predict"].cpu().numpy(), mw, one["predict"].cpu().numpy(), mo, tol_of, T, "chunk_wireframes = 1")
    print("chunk_wireframes = 1 against the whole batch: %d of %d rows compared to the end" % (full, N * F))
    assert full == N * F                                                         # every row, to the end: no pair is indecisive here
    # two wireframe orders, the tables moved with the wireframes
    eng, memory, mask, kv_len = model._encode(b)
    perm = list(reversed(range(N)))
    idx = torch.tensor(perm, device="cuda")
    moved = tuple(t.index_select(0, idx).contiguous() for t in tables)
    kw = dict(T=T, F=F, flags=model.decode_flags, x3_min_rows=model.x3_min_rows, constrain=LOOPS, term_range=TERM, trace=True,
              constrain_exact=True)
    fwd = _with_pad(eng.decode(memory, mask, kv_len, L.FF_PARALLEL, num_input=ni, follow_table=tables[0], cycle_len=tables[2], **kw), b)
    rev = eng.decode(memory.index_select(0, idx).contiguous(), mask.index_select(0, idx).contiguous(), kv_len.index_select(0, idx).contiguous(),
                     L.FF_PARALLEL, num_input=[ni[i] for i in perm], follow_table=moved[0], cycle_len=moved[2], **kw)
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
    assert full == N * F                                                         # every row, to the end: no pair is indecisive here


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
    try:
        with torch.no_grad():
            model.constrain = "loops"
            loops = model(dict(b))
            keys_loops = set(loops)
            model.constrain_exact = True
            on = model(dict(b))
            given = model(dict(b, cycle_len=cyc))
            cpu = model(dict(b, cycle_len=cyc.cpu().numpy()))
            none = model(dict(b, cycle_len=torch.full_like(cyc, 255)))      # an override: no loop may ever be started
            with pytest.raises(ValueError, match="cycle_len must be uint8"):
                model(dict(b, cycle_len=cyc.int()))
            model.sort_by_edges = False
            hand = model(dict(by_hand))
            hand_given = model(dict(by_hand, cycle_len=cyc.index_select(0, idx)))
    finally:
        model.constrain, model.constrain_exact, model.sort_by_edges = None, False, True
    keys = {"predict", "predict_logprob", "predict_dead_end"}
    assert set(on) == keys_loops and keys <= keys_loops                              # the published keys are section 16's
    assert tuple(on["predict"].shape) == tuple(on["predict_logprob"].shape) == (N, F, T) and tuple(on["predict_dead_end"].shape) == (N, F)
    for k in keys:
        assert torch.equal(on[k], given[k]) and torch.equal(on[k], cpu[k]), k            # the built table is ops.follow_distance's
        assert torch.equal(on[k].index_select(0, idx), hand[k]) and torch.equal(hand[k], hand_given[k]), k   # batch order, rows and table
    assert not torch.equal(on["predict"], loops["predict"])
    # the override is what the decode used: an anchor below ntok starts closed and may start no loop, so it ends at once
    pn = none["predict"].cpu().numpy()
    for w, n in enumerate(ni):
        for f in range(min(NTOK, n)):
            assert (pn[w, f, 1:] < NTOK).all(), (w, f, pn[w, f])
    # option off: a model that never had the attribute decodes as before
    with torch.no_grad():
        off = model(dict(b))
    saved = model.__dict__.pop("constrain_exact")
    try:
        with torch.no_grad():
            never = model(dict(b))
            model.constrain = "loops"
            never_loops = model(dict(b))
    finally:
        model.constrain = None
        model.__dict__["constrain_exact"] = saved
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
    a = hip_lib.ff_decode_constrained_exact_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host)
    assert a == hip_lib.ff_decode_constrained_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host) > 0   # nothing new in it


# ---- GPU: poisoned surroundings, the launch forms -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,F,S", [(2, 3, 70), (3, 1, 37)])
def test_operator_inside_poisoned_surroundings(hip_lib, W, F, S):
    import redzone as RZ
    from test_redzone_ops import PAD, twice
    from faceformer_amd.hip import ops
    E, ntok = 64, 4
    L = S - ntok
    B = W * F
    rng = np.random.default_rng(S)
    table = np.stack([_table(("lattice", "ring", "random")[w % 3], L, 11 + w) for w in range(W)])
    follows = torch.from_numpy(faces.pack_follow_bits(table))
    cyc = torch.from_numpy(faces.follow_distance(table, 9)[1])
    g0 = torch.Generator().manual_seed(S)
    raw = torch.randn(B, S, generator=g0) * 3
    mem = torch.randn(W, S, E, generator=g0)
    mask = (torch.rand(W, S, generator=g0) < 0.1).to(torch.uint8)
    mask[:, :ntok] = 0
    kv_len = torch.tensor([S - w for w in range(W)], dtype=torch.int32)
    fin = (torch.arange(B) % 4 == 3).to(torch.int32)
    first = torch.full((B,), -1, dtype=torch.int32)
    prev = torch.full((B,), -1, dtype=torch.int32)
    vis = np.zeros((B, L), dtype=bool)
    for i in range(B):                                                                         # walks: open rows search, closed ones read cycle_len
        walk = ER.walk_states(table[i // F], rng.integers(0, L), int(rng.integers(1, 6)), rng)
        v, f, p = walk[-1] if i % 3 != 1 else ([st for st in walk if st[1] is None] or walk)[-1]
        vis[i, sorted(v)] = True
        first[i], prev[i] = -1 if f is None else f, -1 if p is None else p
    assert (first >= 0).any()
    visited = torch.from_numpy(faces.pack_follow_bits(vis))

    def call(lg, e):
        o = ops.pointer_constrained_exact(lg, e(fin), e(first), e(prev), e(visited), LOOPS, ntok, e(follows), e(cyc), 6,
                                          memory=e(mem), mask=e(mask), kv_len=e(kv_len), seqs_per_group=F, term_range=(1, 4),
                                          want_rows=True, want_stats=True, counter=e(torch.zeros(1, dtype=torch.int32)))
        return dict(o, logits=lg)
    got = twice(lambda g: call(g.embed(raw, ld=S + PAD, name="logits"), g.embed), "ff_pointer_constrained_exact")
    plain = call(raw.cuda(), lambda x: x.cuda())
    for k, v in plain.items():
        if torch.is_tensor(v):
            RZ.assert_same_bits(got[k], v, "ff_pointer_constrained_exact: %s against the clean call" % k)
    assert torch.isfinite(got["logprob"]).all() and bool(got["mask_rows"].any())


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "par_small_ragged"
    m = WP._bound(name, "default")
    b, table = WP._lattice(m)
    tables = _tables(name)
    call = lambda: _exact(m.model, m.case, b, tables, trace=True)
    clean = call()
    clean.pop("engine", None)
    zero, d = WP._run([m], call, fill=RZ.ZERO, what="exact after ZERO")
    poison, _ = WP._run([m], call, fill=RZ.POISON, what="exact after POISON")
    WP._assert_equal(poison, zero, "exact")
    WP._assert_equal(poison, clean, "exact against the clean run")
    WP._assert_no_nan(poison, "exact")
    assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size


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
    call = lambda bound: _with_pad(_exact(bound.model, bound.case, b, tables, trace=True, num_streams=bound.model.num_streams), b)
    with MF._tuned(form):
        out = call(m)
        MF._check_bit_equal(m, lambda bound: {k: v for k, v in call(bound).items() if k not in ("engine", "_pad")}, m.what)
    pairs, _, more = _replay(out, table, tables, max(lat["num_input"]), m.T, m.what)
    print("exact %s %s: steps %d, %d pairs replayed, none left out, more than the look-ahead at %d" % (name, form, out["steps"], pairs, more))
    assert pairs > 0
