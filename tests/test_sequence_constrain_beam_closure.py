"""Opt-in closure look-ahead of the sequence-constrained beam search (SurfaceFormer.sequence_constrain_beam_closure):
the numpy rule on hand-written groups, its identities and guarantees, every refusal and the CLI on the CPU (library untouched); the
selection step, the engine's entry, the model and the CLI on the GPU, through the C ABI.  The rule is
tests/sequence_constrain_beam_closure_ref.py's, which composes sequence_constrain_beam_ref, sequence_constrain_closure_ref and
faces.sequence_rule_* and restates none of them.

Bars (the issue's, none measured): byte rows, FILL patterns, parents, tokens, flags, states, visited words, appended rows and
counters are exact on every DECISIVE group (every decisive gap above twice beam_ref.score_bound, times the steps accumulated); a
score lies within score_bound of fp64 on the kernel's own masked rows; at most 2 % of a case's groups / (step, group) pairs may be
left out -- a condition on the inputs, fixed on the CPU by tools/sequence_constrain_beam_closure_left_out.py (the operator seeds
leave nothing out); scores within section 34's bar of the fp64 oracle forced along the final beams; identity (a)
|score - sum logprob| <= (T - 1) 2^-16."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import beam_ref as R
import sequence_constrain_beam_closure_ref as BC
import sequence_constrain_beam_ref as CB
import sequence_constrain_closure_ref as QC
import sequence_constrain_ref as SC
import test_sequence_constrain_beam as TB
import test_sequence_constrain_closure as TCL
from conftest import ROOT, batch_to, token_ns
from faceformer_amd import faces
from faceformer_amd.hip.modes import SEQUENCE_CONSTRAIN_BEAM_AHEAD, sequence_constrain_beam_closure_value   # (without them nothing here can pass)
from test_sequence_constrain import E_OP, _fixture, _seq_inputs, _tiny_model, _untouchable, _words

TOK = token_ns()
NTOK, SOS, SEP, EOS = TOK.len, TOK.SOS, TOK.SEP, TOK.EOS
FILL, NEG = BC.FILL, BC.NEG
LOOPS, COEDGE = BC.LOOPS, BC.COEDGE_LOOPS
START = faces.sequence_rule_start()
T_A, T_B = QC.table_of(QC.TRAP_A), QC.table_of(QC.TRAP_B)
_PLAIN_RUN, _PLAIN_WANT = TB._run_beam_op, TB._want_of


# ---- CPU: the numpy rule on hand-written groups -------------------------------------------------------------------------------------
def _both(raw, scores, fin, states, flags, table, form, budget, pad=None):
    """The helper's group step and faces' own beam step under the form on one group: they must agree on everything they share."""
    raw = np.asarray(raw, dtype=np.float64)
    pad = np.zeros(raw.shape[1], bool) if pad is None else np.asarray(pad, bool)
    cd, cl = faces.follow_distance(table, 254)
    kw = QC.closure_kw(form, cd[None], cl[None], 0, budget)
    args = (raw, pad, np.asarray(scores, float), np.asarray(fin, bool), list(states), flags, NTOK, SEP, EOS, table)
    a = BC.group_step(*args, **kw)
    b = faces.sequence_rule_beam_step(*args, **kw)
    for k in ("parent", "tok", "fin", "dead", "open"):
        assert np.array_equal(a[k], b[k]), k
    assert a["states"] == b["states"] and np.allclose(a["scores"], b["scores"], rtol=0, atol=1e-12, equal_nan=True)
    for k in range(raw.shape[0]):
        if a["masked"][k] is not None:
            assert np.array_equal(a["masked"][k], b["masked"][k]) and np.array_equal(a["rows"][k], b["rows"][k])
    return a


def _live(r, k):
    return [] if r["masked"][k] is None else [e for e in range(len(r["masked"][k]) - NTOK) if not r["masked"][k][NTOK + e]]


def test_rule_on_hand_written_groups():
    assert NTOK == 4
    g = np.random.default_rng(5)
    # two beams of ONE group with different `first` on trap A: edge 3 follows edge 1 for both; at budget 2 it is masked for the
    # beam that opened at 0 (close_dist[0][3] = 3) and live for the one that opened at 3 (close_dist[3][3] = D(3 -> 3) = 2: 3 1 3),
    # whose own edge 2 is masked in turn (D(2 -> 3) = 3)
    S = NTOK + 4
    raw = g.standard_normal((2, S))
    cd, cl = faces.follow_distance(T_A, 254)
    assert cl.tolist() == [3, 2, 3, 2] and cd[0][3] == 3 and cd[3][3] == 2 and cd[0][2] == 1 and cd[3][2] == 3
    from_0, from_3 = (frozenset({0, 1}), 0, 1), (frozenset({1}), 3, 1)
    r = _both(raw, [-1.0, -2.0], [False, False], [from_0, from_3], 2, T_A, "lookahead", 2)      # (CONNECT alone: 3 may repeat)
    assert _live(r, 0) == [2] and _live(r, 1) == [3]
    r = _both(raw, [-1.0, -2.0], [False, False], [from_0, from_3], 2, T_A, "lookahead", 3)
    assert _live(r, 0) == [2, 3] and _live(r, 1) == [2, 3]
    # trap A per beam: the static form keeps the trap edge at budget >= 3, the exact form never does -- beside a sibling that is closed
    for form, budget, live0 in (("lookahead", 5, [2, 3]), ("lookahead", 2, [2]), ("exact", 5, [2]), ("exact", 254, [2])):
        r = _both(raw, [-1.0, -2.0], [False, False], [from_0, START], LOOPS, T_A, form, budget)
        assert _live(r, 0) == live0 and _live(r, 1) == [e for e in range(4) if cl[e] <= budget], (form, budget)      # closed: the cycle_len rule
    assert _live(_both(raw, [-1.0, -2.0], [False, False], [from_0, START], LOOPS, T_A, None, None), 0) == [2, 3]      # the plain rule
    # trap B: two beams with DIFFERENT visited under flags 7 -- one holds an earlier face's edge 4, kept under ONCE -- at one budget
    S = NTOK + 5
    raw = g.standard_normal((2, S))
    once, fresh = (frozenset({4, 0, 1}), 0, 1), (frozenset({0, 1}), 0, 1)
    r = _both(raw, [-1.0, -2.0], [False, False], [once, fresh], COEDGE, T_B, "exact", 5)
    assert _live(r, 0) == [2] and _live(r, 1) == [2, 3]
    r = _both(raw, [-1.0, -2.0], [False, False], [once, fresh], COEDGE, T_B, "lookahead", 5)
    assert _live(r, 0) == _live(r, 1) == [2, 3]                                                   # the static form cannot tell
    # budget 0: an open beam -> SEP at unchanged score with the dead flag; a closed beam -> SEP or EOS, no dead flag
    closed = (frozenset({0, 1, 2}), None, 2)
    for form in BC.FORMS:
        for flags in (LOOPS, COEDGE):
            r = _both(raw, [-1.5, NEG], [False, False], [fresh, START], flags, T_B, form, 0)
            assert r["tok"][0] == SEP and r["scores"][0] == -1.5 and r["dead"][0] and not r["fin"][0] and not r["open"][0]
            assert r["scores"][1] == NEG and r["parent"][1] == 1 and not r["dead"][1]
            r = _both(raw, [-1.5, -2.5], [False, False], [closed, START], flags, T_B, form, 0)
            assert _live(r, 0) == _live(r, 1) == [] and not r["dead"].any()
            assert set(r["tok"][r["parent"] == 0].tolist()) <= {SEP, EOS} and set(r["tok"][r["parent"] == 1].tolist()) <= {EOS}
            assert np.isfinite(r["scores"]).all() and (SEP in r["tok"].tolist() or r["fin"].all())
    # a finished rank 0 keeps rank 0 on an exact tie, whatever the form masks beside it
    tie = np.full((2, S), -60.0)
    tie[1, NTOK + 2] = 0.0
    r = _both(tie, [-2.0, -2.0], [True, False], [closed, fresh], LOOPS, T_B, "exact", 5)
    assert r["parent"].tolist() == [0, 1] and r["fin"].tolist() == [True, False] and r["tok"].tolist() == [0, NTOK + 2]


def _prefix_source(S, seed, eos_bias=-3.0):
    """A prefix-dependent logit source: the row of a beam is a function of its whole prefix."""
    def step_logits(prefixes, j):
        rows = np.zeros((prefixes.shape[0], S))
        for r, p in enumerate(prefixes):
            rows[r] = np.random.default_rng([seed, j] + [int(v) for v in p]).standard_normal(S) * 2.5
        rows[:, EOS] += eos_bias
        return rows
    return step_logits


def test_identities_of_the_numpy_rule_on_a_prefix_dependent_source():
    g = np.random.default_rng(17)
    seen = dict(stricter=0, closed=0, dead=0)
    for trial in range(4):
        L, T, W = int(g.integers(5, 10)), int(g.integers(7, 13)), (2, 3)[trial % 2]
        S = NTOK + L
        t = g.random((2, L, L)) < 0.3
        pads = np.zeros((2, S), bool)
        pads[1, S - 1] = True
        cd, cl = BC.tables(t, T)
        src = _prefix_source(S, trial)
        for flags in (LOOPS, COEDGE):
            args = (T, flags, NTOK, SOS, SEP, EOS, t)
            for form in BC.FORMS:
                for stop in BC.STOPS:
                    # (a) W = 1: the sequence_constrain_closure greedy decode of the same form and flags
                    one = BC.decode(src, pads, 1, *args, stop, form, cd, cl)
                    greedy = QC.decode(lambda paths, s: np.where(pads, FILL, src(paths[:, : s + 1], s)), 2, T, flags, NTOK, SOS, SEP, EOS, t,
                                       form, cd, cl)
                    assert np.array_equal(one["beams"], greedy["tokens"]) and np.array_equal(one["dead_end"], greedy["dead"]), (trial, form)
                    assert one["steps"] == greedy["steps"] and np.array_equal(one["open"].astype(int), greedy["open_end"])
                    assert np.abs(one["scores"] - greedy["logprob"].sum(axis=1)).max() < 1e-9
                    # faces' own decode is the helper's
                    mine = faces.sequence_rule_beam_decode(src, pads, W, *args, stop, closure=form, close_dist=cd, cycle_len=cl)
                    ref = BC.decode(src, pads, W, *args, stop, form, cd, cl)
                    assert np.array_equal(mine["beams"], ref["beams"]) and np.array_equal(mine["dead_end"], ref["dead_end"])
                    assert mine["steps"] == ref["steps"] and mine["counts"] == ref["counts"]
                # (e) "best" against "all": beam 0 and its score, no later
                al, be = (BC.decode(src, pads, W, *args, stop, form, cd, cl) for stop in BC.STOPS)
                assert be["steps"] <= al["steps"] and be["steps"] == CB.stop_step(al["best_counts"], T)
                if be["steps"] == al["steps"] or al["fin"][::W].all():
                    assert np.array_equal(be["beams"][::W], al["beams"][::W])
            # (b) "lookahead" with both tables zero: the plain beam decode
            zero = BC.decode(src, pads, W, *args, "all", "lookahead", np.zeros_like(cd), np.zeros_like(cl))
            plain = CB.decode(src, pads, W, *args, "all")
            for k in ("beams", "dead_end", "scores", "fin", "open"):
                assert np.array_equal(zero[k], plain[k]), k
            assert zero["steps"] == plain["steps"] and zero["counts"] == plain["counts"]
            # (c), (d) per beam row and step along the exact decode's own states
            ex = BC.decode(src, pads, W, *args, "all", "exact", cd, cl)
            scores, fin = CB.QB.start(2, W)
            states = [START] * (2 * W)
            for j in range(ex["steps"]):
                prefixes = R.backtrack(np.full(2 * W, SOS), ex["toks"][:j], ex["parents"][:j], W)
                raw = src(prefixes, j)
                budget = BC.budget_of(T, j + 1)
                a = BC.beam_step(raw, pads, scores, fin, states, W, flags, NTOK, SEP, EOS, t, "lookahead", cd, cl, budget)
                e = BC.beam_step(raw, pads, scores, fin, states, W, flags, NTOK, SEP, EOS, t, "exact", cd, cl, budget)
                for b in range(2 * W):
                    if e["masked"][b] is None:
                        continue
                    if not (a["dead_now"][b] or e["dead_now"][b]):
                        assert not (a["masked"][b][NTOK:] & ~e["masked"][b][NTOK:]).any()           # (c)
                    seen["stricter"] += bool((e["masked"][b][NTOK:] & ~a["masked"][b][NTOK:]).any())
                    seen["dead"] += bool(e["dead_now"][b])
                    if states[b][1] is None:
                        assert np.array_equal(a["masked"][b], e["masked"][b])                       # (d)
                        seen["closed"] += 1
                scores, fin, states = e["scores"], e["fin"], e["states"]
    assert all(seen.values()), seen


def test_guarantees_on_scripted_decodes_where_the_plain_beam_rule_ends_open_and_dead_ends_late():
    counts = dict(plain_open=0, plain_late=0)
    for seed in range(10):
        g = np.random.default_rng([0x62, seed])
        L, T, W = int(g.integers(5, 11)), int(g.integers(6, 14)), int(g.integers(2, 5))
        S = NTOK + L
        t = (g.random((1, L, L)) < 0.25)
        pads = np.zeros((1, S), bool)
        src = _prefix_source(S, 100 + seed, eos_bias=-4.0)
        cd, cl = BC.tables(t, T)
        for flags in (LOOPS, COEDGE):
            args = (T, flags, NTOK, SOS, SEP, EOS, t)
            plain = CB.decode(src, pads, W, *args, "all")
            live = np.isfinite(plain["scores"])
            counts["plain_open"] += int(plain["open"][live].sum())
            counts["plain_late"] += len([1 for r, p in BC.late_dead_ends(plain["beams"], plain["dead_end"], flags, NTOK, SEP, t, W) if live[r]])
            for form in BC.FORMS:
                d = BC.decode(src, pads, W, *args, "all", form, cd, cl)
                BC.guarantees(d["beams"], d["dead_end"], d["open"].astype(int), d["scores"], W, [L], flags, NTOK, SEP, EOS, t, None, form)
    assert counts["plain_open"] and counts["plain_late"], counts


# ---- CPU: C ABI, binding, records ---------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_beam_sequence_constrained_select_ahead", "ff_sequence_decode_constrained_beam_ahead_workspace_bytes",
               "ff_sequence_decode_constrained_beam_ahead")


def test_header_binding_and_struct_fields_within_abi_105():
    from faceformer_amd.hip import build, lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
        n_args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).count(",") + 1
        assert n_args == len(lib.SIGNATURES[name][1]), name
    S = lib.SIGNATURES
    assert len(S["ff_beam_sequence_constrained_select_ahead"][1]) == len(S["ff_beam_sequence_constrained_select"][1]) + 4
    assert S["ff_beam_sequence_constrained_select_ahead"][1][0] is S["ff_beam_sequence_constrained_select"][1][0]      # the step descriptor, unchanged
    assert S["ff_sequence_decode_constrained_beam_ahead_workspace_bytes"] == S["ff_decode_sequence_constrained_beam_workspace_bytes"]
    fields = re.search(r"typedef struct ff_sequence_constrain_beam_ahead_params \{(.*?)\}", code, flags=re.S).group(1)
    names = [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()]
    assert names == [n for n, _ in lib.SequenceConstrainBeamAheadParams._fields_] == \
        [n for n, _ in lib.SequenceConstrainBeamParams._fields_] + ["form", "close_dist", "cycle_len"]
    doc = header[header.index("closure look-ahead of the sequence-constrained beam search"):
                 header.index("int ff_beam_sequence_constrained_select_ahead(")]
    for phrase in ("budget = min(T - 1 - p, 254)", "one budget per launch", "hmax = min(max(T - 2, 1), 254)", "shared by its W beams",
                   "from its OWN (first, prev) and its OWN visited words", "close_dist[w][first_k][b] > budget", "cycle_len[w][b] > budget",
                   "D_V(b -> first_k) > budget", "neither\n *       padded nor in beam k's visited", "Under ONCE those words hold every earlier face's edges",
                   "The dead-end vote runs after these masks and re-opens SEP alone", "two closed-state fix-ups are unchanged", "(a) W = 1",
                   "(b) form 1 with both tables zero", "(c)", "(d)", "(e)", "(g1) beam_open_end == 0", "(g2)", "(g3)", "a form outside 1..2",
                   "a budget outside 0..254", "more than 2048 keys"):
        assert phrase in doc, phrase
    assert len(build.SOURCES) == 17 and build.SOURCES[-3:] == ["ff_constrain_seq.hip", "ff_faces.hip", "ff_engine.hip"]
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain_seq.hip")).read()
    assert "template <int W, int STOP, int FORM = FF_LOOP_PLAIN>" in src and "struct SeqConBeamClosureArgs : SeqConBeamArgs" in src
    assert src.count("ff_sequence_write_row(pa, rule, lane") == 1 and src.count("ff_sequence_write_row<FORM>(pa, rule, lane") == 1
    assert "ff_dispatch<FF_LOOP_AHEAD, FF_LOOP_EXACT>" in src and "ff_loop_closure_reach(" not in src
    assert "__syncthreads" not in src and "__shared__" not in src and "asm" not in src          # no barrier, no LDS of its own, plain HIP
    sel = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_select.h")).read()
    assert "template <int FORM = FF_LOOP_PLAIN>\n__device__ __forceinline__ bool ff_sequence_write_row(" in sel
    eng = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_engine.hip")).read()
    at = eng.index('extern "C" int ff_sequence_decode_constrained_beam_ahead(')
    assert "model.py:161-167, 191, 193-210" in eng[at - 400:at]                                  # the entry cites what it replaces
    assert "ff_beam_sequence_constrained_select_sync(sio, &d, la, st)" in eng                   # the step takes the look-ahead it builds


def test_a_library_without_the_new_entries_is_refused(monkeypatch):
    from faceformer_amd.hip import lib

    class Old:
        def __getattr__(self, name):
            if name in NEW_ENTRIES:
                raise AttributeError(name)
            return types.SimpleNamespace(restype=None, argtypes=None)
    monkeypatch.setattr(lib.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib.os.path, "exists", lambda p: True)
    with pytest.raises(lib.HipExtensionError, match="does not export ff_beam_sequence_constrained_select_ahead .*rebuild"):
        lib.load()


def test_record_lies_outside_both_tables_and_the_value_check():
    from faceformer_amd.hip import modes
    rec = modes.SEQUENCE_CONSTRAIN_BEAM_AHEAD
    assert rec is SEQUENCE_CONSTRAIN_BEAM_AHEAD and rec not in modes.MODES and rec not in modes.SEQUENCE_MODES
    assert len(modes.MODES) == 4 and len(modes.SEQUENCE_MODES) == 3                       # the pinned table sizes
    assert modes.SEQUENCE_MODES == (modes.SEQUENCE_SAMPLE, modes.SEQUENCE_BEAM, modes.SEQUENCE_CONSTRAIN)
    assert modes.SEQUENCE_MODEL_ORDER == (modes.SEQUENCE_BEAM, modes.SEQUENCE_SAMPLE, modes.SEQUENCE_CONSTRAIN)
    assert sorted(modes.SWITCH) == sorted(sw.attr for m in modes.MODES for sw in m.switches)
    base = modes.SEQUENCE_CONSTRAIN_BEAM
    assert rec.entry == "ff_sequence_decode_constrained_beam_ahead" and rec.outs == base.outs and rec.subject == base.subject
    assert rec.per_anchor and rec.excludes == base.excludes and rec.switches == base.switches
    assert [n for n, _ in rec.own] == ["follow_table", "close_dist", "cycle_len"]
    v = sequence_constrain_beam_closure_value
    assert v(None, None) is None and v(None, 3, 2) is None
    assert [v("lookahead", f, 2) for f in (2, 3, 7)] == ["lookahead"] * 3 and [v("exact", f, 1) for f in (3, 7)] == ["exact"] * 2
    for bad in ("ahead", True, 1, 0, ""):
        with pytest.raises(ValueError, match="sequence_constrain_beam_closure=.*must be None, 'lookahead' or 'exact'"):
            v(bad, 3, 2)
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure='exact' needs sequence_constrain_beams >= 1"):
        v("exact", 3, 0)
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure='exact' needs sequence_constrain \\('loops' or 'coedge_loops'\\)"):
        v("exact", None, 2)
    for flags in (0, 1, 5):
        with pytest.raises(ValueError, match="needs sequence_constrain with FF_CONSTRAIN_CONNECT"):
            v("lookahead", flags, 2)
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure='exact' needs FF_CONSTRAIN_NO_REPEAT as well"):
        v("exact", 2, 2)
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure excludes sequence_constrain_closure"):
        v("exact", 3, 2, "exact")
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure excludes sequence_constrain_samples"):
        v("exact", 3, 0, None, 2)
    with pytest.raises(ValueError, match="sequence_constrain_closure excludes sequence_constrain_beams"):      # the recorded text stays
        modes.sequence_constrain_closure_value("lookahead", 3, 2)


# ---- CPU: every refusal -------------------------------------------------------------------------------------------------------------
def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes = {}
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    ft = torch.zeros(2, 8, 1, dtype=torch.int32)
    cd, cl = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.uint8)
    ok = dict(T=300, F=1, sequence_constrain="loops", tok_sep=SEP, follow_table=ft, sequence_constrain_beams=2,
              sequence_constrain_beam_closure="lookahead", close_dist=cd, cycle_len=cl)
    dec = lambda **kw: eng.decode(memory, None, None, kw.pop("variant", lib.FF_SEQ2SEQ), **kw)
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure='lookahead' needs sequence_constrain_beams >= 1"):
        dec(**dict(ok, sequence_constrain_beams=None))
    with pytest.raises(ValueError, match="sequence_constrain_beams=2 needs sequence_constrain"):
        dec(**dict(ok, sequence_constrain=None))
    for value in ("no_repeat", 0, 1, 5):
        with pytest.raises(ValueError, match="sequence_constrain_beam_closure='lookahead' needs sequence_constrain with FF_CONSTRAIN_CONNECT"):
            dec(**dict(ok, sequence_constrain=value))
    with pytest.raises(ValueError, match="'exact' needs FF_CONSTRAIN_NO_REPEAT as well"):
        dec(**dict(ok, sequence_constrain=2, sequence_constrain_beam_closure="exact"))
    with pytest.raises(ValueError, match="sequence_constrain_closure excludes sequence_constrain_beams"):      # the recorded refusal, first
        dec(**dict(ok, sequence_constrain_closure="exact"))
    with pytest.raises(ValueError, match="sequence_constrain_beams excludes sequence_samples, sequence_beams and sequence_constrain_samples"):
        dec(**dict(ok, sequence_constrain_samples=2))
    for bad in ("ahead", True, 2):
        with pytest.raises(ValueError, match="sequence_constrain_beam_closure=.*must be None, 'lookahead' or 'exact'"):
            dec(**dict(ok, sequence_constrain_beam_closure=bad))
    with pytest.raises(ValueError, match="is a single-sequence option"):
        dec(variant=lib.FF_PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=2),
                   dict(constrain="no_repeat"), dict(sequence_samples=2), dict(sequence_beams=2)):
        with pytest.raises(ValueError, match="excludes"):                                 # everything sequence_constrain_beams excludes
            dec(**dict(ok, **change))
    with pytest.raises(ValueError, match="sequence_constrain_beams=9"):
        dec(**dict(ok, sequence_constrain_beams=9))
    with pytest.raises(ValueError, match="sequence_beam_stop='first'"):
        dec(**dict(ok, sequence_beam_stop="first"))
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure='lookahead' needs close_dist and cycle_len"):
        dec(**dict(ok, close_dist=None))
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure='exact' needs cycle_len"):
        dec(**dict(ok, sequence_constrain_beam_closure="exact", cycle_len=None, close_dist=None))
    for name, bad, shape in (("close_dist", torch.zeros(2, 8, 7, dtype=torch.uint8), "2, 8, 8"), ("cycle_len", cl.int(), "2, 8"),
                             ("cycle_len", torch.zeros(4, 8, dtype=torch.uint8), "2, 8")):      # per wireframe, not per beam
        with pytest.raises(ValueError, match="%s must be a uint8 tensor of shape \\[%s\\]" % (name, shape)):
            dec(**dict(ok, **{name: bad}))
    big = torch.zeros(1, 2049, 64)
    with pytest.raises(ValueError, match="sequence_constrain_beam_closure='exact' takes at most 2044 edges per wireframe \\(got 2045\\)"):
        eng.decode(big, None, None, lib.FF_SEQ2SEQ, T=5, F=1, sequence_constrain="loops", tok_sep=SEP, sequence_constrain_beams=2,
                   follow_table=torch.zeros(1, 2045, 64, dtype=torch.int32), sequence_constrain_beam_closure="exact",
                   cycle_len=torch.zeros(1, 2045, dtype=torch.uint8))


def test_models_dist_and_score_reject_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    par = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert par.sequence_constrain_beam_closure is None
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    par.sequence_constrain_beam_closure = "exact"
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_beam_closure is a SurfaceFormer option .*constrain_beam_closure"):
        par.forward_eval(inputs)
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.sequence_constrain_beam_closure is None
    seq.sequence_constrain_beam_closure = "lookahead"
    with torch.no_grad(), pytest.raises(ValueError, match="needs sequence_constrain_beams >= 1"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain = "loops"
    with torch.no_grad(), pytest.raises(ValueError, match="needs sequence_constrain_beams >= 1"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_beams = 2
    seq.sequence_constrain = "no_repeat"
    with torch.no_grad(), pytest.raises(ValueError, match="needs sequence_constrain with FF_CONSTRAIN_CONNECT"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain, seq.sequence_constrain_beam_closure = 2, "exact"
    with torch.no_grad(), pytest.raises(ValueError, match="'exact' needs FF_CONSTRAIN_NO_REPEAT as well"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain, seq.sequence_constrain_beam_closure = "loops", "ahead"
    with torch.no_grad(), pytest.raises(ValueError, match="must be None, 'lookahead' or 'exact'"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_beam_closure, seq.sequence_constrain_closure = "exact", "exact"
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_closure excludes sequence_constrain_beams"):      # the recorded text
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_closure = None
    for attr, val, off in (("sequence_samples", 2, 0), ("sequence_beams", 2, 0), ("return_logprob", True, False), ("stop_each_eos", True, False),
                           ("sequence_constrain_samples", 2, 0)):
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="excludes"):
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, off)
    for name, bad in (("close_dist", torch.zeros(1, 8, 7, dtype=torch.uint8)), ("cycle_len", torch.zeros(1, 8))):
        seq.sequence_constrain_beam_closure = "lookahead"
        with torch.no_grad(), pytest.raises(ValueError, match="%s must be uint8" % name):
            seq.forward_eval(_seq_inputs(**{name: bad}))
    seq.sequence_constrain = seq.sequence_constrain_beams = None
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain_beam_closure"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    wide = _tiny_model(SurfaceFormer, label_seq_length=6, num_lines=2045)
    wide.sequence_constrain, wide.sequence_constrain_beams, wide.sequence_constrain_beam_closure = "loops", 2, "exact"
    with torch.no_grad(), pytest.raises(ValueError, match="'exact' takes at most 2044 edges per wireframe \\(got 2045\\)"):
        wide.forward_eval({"input": torch.zeros(1, 2045, 50, 2), "input_mask": torch.zeros(1, 2045, dtype=torch.bool),
                           "label": torch.zeros(1, 6, dtype=torch.long)})
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                  # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_constrain, sub.sequence_constrain_beams, sub.sequence_constrain_beam_closure = "loops", 2, "lookahead"
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain needs the native engine"):
            sub.forward_eval(_seq_inputs())

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, sequence_constrain=None,
                                  sequence_constrain_beam_closure="exact")
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_constrain_beam_closure"):
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_constrain_beam_closure = None
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


def test_cli_flags_reach_the_model_and_every_refusal_raises(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain", "coedge_loops", "--sequence-constrain-beams", "4",
                                       "--sequence-constrain-beam-closure", "exact", "--sequence-beam-stop", "best"])
    assert (a.sequence_constrain, a.sequence_constrain_beams, a.sequence_constrain_beam_closure, a.sequence_beam_stop) == \
        ("coedge_loops", 4, "exact", "best")
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).sequence_constrain_beam_closure is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain-beam-closure", "ahead"])
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-constrain", "loops", "--sequence-constrain-beams", "3", "--sequence-constrain-beam-closure", "lookahead",
              "--test_ckpt", "unused.ckpt"])
    cli.main(["--sequence-constrain", "loops", "--sequence-constrain-beams", "3", "--test_ckpt", "unused.ckpt"])
    assert [(kw["sequence_constrain"], kw["sequence_constrain_beams"], kw["sequence_constrain_beam_closure"], kw["sequence_constrain_closure"])
            for kw in seen] == [("loops", 3, "lookahead", None), ("loops", 3, None, None)]
    m = cli.configure_model(types.SimpleNamespace(), sequence_constrain_beam_closure="exact")
    assert vars(m) == dict(sequence_constrain_beam_closure="exact")
    plain = types.SimpleNamespace()
    cli.configure_model(plain, sequence_constrain_beams=2)
    assert vars(plain) == dict(sequence_constrain_beams=2, sequence_beam_stop="all")          # without the flag: what it was
    seqcfg = types.SimpleNamespace(model_class="SurfaceFormer")
    call = dict(out_dir="unused", device="cpu", model=object())
    with pytest.raises(ValueError, match="--sequence-constrain-beam-closure requires --sequence-constrain-beams W"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beam_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beam-closure requires --sequence-constrain \\{loops,coedge_loops\\}"):
        run_test(seqcfg, None, sequence_constrain_beams=2, sequence_constrain_beam_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beam-closure requires --sequence-constrain loops or coedge_loops: no_repeat"):
        run_test(seqcfg, None, sequence_constrain="no_repeat", sequence_constrain_beams=2, sequence_constrain_beam_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beam-closure is not implemented with --sequence-constrain-closure"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, sequence_constrain_closure="exact",
                 sequence_constrain_beam_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beam-closure is not implemented with --sequence-constrain-samples"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_samples=2, sequence_constrain_beam_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beam-closure must be lookahead or exact"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, sequence_constrain_beam_closure="ahead", **call)
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sequence-constrain-beam-closure is not implemented for multi-rank runs"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, sequence_constrain_beam_closure="exact", dist_mod=world2,
                 **call)
    with pytest.raises(ValueError, match="--sequence-constrain-closure is not implemented with --sequence-constrain-beams"):      # stays refused
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, sequence_constrain_closure="exact", **call)


def test_the_c_entry_refuses_before_any_launch(monkeypatch):
    """The decode entry through test_entry_checks' machinery (no GPU: an entry rejects bad arguments before any HIP call): what
    ff_decode_sequence_constrained_beam refuses, in its order and under this entry's name, then the form, the look-ahead's flags
    and tables and the key limit of the exact search; T = 300 is accepted; the size query equals section 34's."""
    import test_entry_checks as TE
    from faceformer_amd.hip import lib as L
    lib = L.load()
    base = TE.CHECKS["ff_decode_sequence_constrained_beam"]
    D = TE.DUMMY
    form = ("form", {("prm", "form"): 3})
    tables = ("ahead_tables", {("prm", "close_dist"): None})
    plain_fields = dict(base[2])
    at = [c[0] for c in base[3]].index("outputs")      # the look-ahead's checks stand between the rule's and the outputs'
    new = {
        "ff_sequence_decode_constrained_beam_ahead[ahead]": (
            base[0], L.SequenceConstrainBeamAheadParams, dict(plain_fields, form=1, close_dist=D, cycle_len=D),
            base[3][:at] + [form, TE.AHEAD[0], tables] + base[3][at:]),
        "ff_sequence_decode_constrained_beam_ahead[exact]": (
            base[0], L.SequenceConstrainBeamAheadParams, dict(plain_fields, form=2, cycle_len=D),
            base[3][:at] + [form, TE.EXACT[0], TE.EXACT[1], TE.EXACT[3]] + base[3][at:]),
    }
    own = {"form": "form=3 must be 1 (look-ahead) or 2 (exact)", "form:0": "form=0 must be 1 (look-ahead) or 2 (exact)",
           "ahead_flags": "the look-ahead needs FF_CONSTRAIN_CONNECT", "ahead_tables": "close_dist and cycle_len are required",
           "ahead_tables:cycle_len": "close_dist and cycle_len are required",
           "exact_flags": "the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT",
           "exact_flags:no_repeat_only": "the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT",
           "exact_table": "cycle_len is required", "exact_L": "L=2045 above 2044 (L + num_token keys at most 2048)"}
    monkeypatch.setitem(TE.ALTERNATIVES, (None, "form"), [("0", {("prm", "form"): 0})])
    for entry, rec in new.items():
        monkeypatch.setitem(TE.CHECKS, entry, rec)
    name, plain = "ff_sequence_decode_constrained_beam_ahead", "ff_decode_sequence_constrained_beam"
    for entry in new:
        seen = set()
        for case in TE.case_ids():
            if case.split("/")[0] != entry:
                continue
            rc, text = TE.call(lib, case)
            check = case.split("/")[1]
            first = check.split("+")[0]
            seen.add(first.split(":")[0])
            if check == "pass":
                assert (rc, text) == (-1, "ff_decode: null pointer"), case                 # handed on to the decode: accepted
            elif first in own or first.split(":")[0] in own:
                assert (rc, text) == (-1, "%s: %s" % (name, own.get(first, own[first.split(":")[0]]))), (case, text)
            else:      # a check the plain entry makes: its recorded text under this entry's name, noun and sibling
                key = "%s/%s" % (plain, check) if "%s/%s" % (plain, check) in TE.EXPECTED else "%s/%s" % (plain, first)
                want = TE.EXPECTED[key]
                words = want[1].replace(plain + ":", name + ":").replace("or constrain beam params", "or look-ahead beam params").replace(
                    "the parallel variant has ff_decode_constrained_beam", "the parallel variant has ff_decode_constrained_beam_ahead")
                assert (rc, text) == (want[0], words), (case, text)
        assert {"form", "outputs", "rule_flags", "variant"} <= seen, (entry, seen)
    monkeypatch.setitem(TE.CHECKS, name + "[long]", new[name + "[ahead]"][:3] + ([("T", {("p", "T"): 300})],))
    assert TE.call(lib, name + "[long]/T") == (-1, "ff_decode: null pointer")              # T above 256: the step clamps the budget
    m, p = TE.model(False), L.DecodeParams()
    p.N, p.L, p.T, p.sync_every, p.tok_sos, p.tok_eos, p.variant, p.F, p.flags = TE.N, TE.EDGES, TE.T, 4, 0, 1, L.FF_SEQ2SEQ, 1, TE.SEQ_FLAGS
    q = lambda fn, *a: getattr(lib, fn)(m, p, *a)
    for W in (1, 3, 8):
        assert q(name + "_workspace_bytes", W) == q(plain + "_workspace_bytes", W) > 0
    assert q(name + "_workspace_bytes", 0) == 0 and q(name + "_workspace_bytes", 9) == 0
    assert getattr(lib, name + "_workspace_bytes")(None, p, 2) == 0 and getattr(lib, name + "_workspace_bytes")(m, None, 2) == 0
    p.variant = L.FF_PARALLEL
    assert q(name + "_workspace_bytes", 2) == 0


# ---- GPU: the step operator ---------------------------------------------------------------------------------------------------------
def _beam_closure_case(S, W, G, once, kind, seed, hmax=254):
    """test_sequence_constrain_closure's operator case (tables of `kind`, the states re-made for them, mixed over section 32's six
    kinds with finished rows, the traps' own state in row 0, different kv_len and a padding mask) as G groups of W beams, one group
    per wireframe, with section 34's scores (about one beam in six empty)."""
    c = TCL._closure_case(G * W, S, W, seed, kind, once, hmax)
    c["scores"] = CB.beam_scores(c, S, W, G, seed, "mixed")
    c["Wd"], c["G"] = W, G
    return c


def _want_of_closure(c, form, budget, seen=None):
    """The numpy rule per group under the form; `seen` counts, over the unfinished non-empty beams, those masked beyond the plain
    rule, the dead ends and the kept candidates that close a loop."""
    W, st, flags = c["Wd"], TB._states(c), c["flags"]
    out = []
    for g in range(c["G"]):
        sl = slice(g * W, (g + 1) * W)
        args = (c["logits"][sl].astype(np.float64), c["pad"][g], c["scores"][sl], c["fin"][sl] != 0, st[sl], flags, NTOK, SEP, EOS, c["table"][g])
        wg = BC.group_step(*args, **BC.closure_kw(form, c["close_dist"], c["cycle_len"], g, budget))
        out.append(wg)
        if seen is None or form is None:
            continue
        plain = CB.group_step(*args)
        for k in range(W):
            if wg["masked"][k] is not None:
                seen["stricter"] += bool((wg["masked"][k][NTOK:] & ~plain["masked"][k][NTOK:] & ~c["pad"][g][NTOK:]).any())
                seen["dead"] += bool(wg["dead_now"][k])
        for r in range(W):
            p = int(wg["parent"][r])
            if wg["scores"][r] != NEG and not c["fin"][g * W + p] and st[g * W + p][1] is not None:
                seen["closing"] += wg["tok"][r] >= NTOK and wg["states"][r][1] is None
    return out


def _run_ahead(c, form, budget, stop, counter=None, scores=None, want_stats=True, tables=None):
    from faceformer_amd.hip import ops
    lg = torch.from_numpy(c["logits"]).clone().cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sc = c["scores"] if scores is None else scores
    cd, cl = tables if tables is not None else (c["close_dist"], c["cycle_len"])
    res = ops.beam_sequence_constrained_select_ahead(
        lg, dev(sc.astype(np.float32)), dev(c["fin"]), dev(c["first"]), dev(c["prev"]), dev(_words(c["visited"], c["L"])), c["Wd"], c["flags"],
        NTOK, SEP, EOS, dev(faces.pack_follow_bits(c["table"])), form, dev(cl), budget, close_dist=dev(cd), stop=stop, memory=dev(c["memory"]),
        mask=dev(c["mask"].astype(np.uint8)), kv_len=dev(c["kv"]), groups_per_wireframe=1, want_rows=True, want_stats=want_stats,
        counter=counter)
    return lg, res


def _check_ahead(monkeypatch, c, form, budget, stop, seen, mine):
    """Section 34's whole operator check (byte rows, FILL, parents, tokens, flags, (first, prev), visited_out, appended rows,
    counters, scores within score_bound, two launches bit-equal, the cap) with the launch and the numpy rule under the form."""
    monkeypatch.setattr(TB, "_run_beam_op", lambda c_, flags, stop_, counter=None, scores=None, want_stats=True:
                        _run_ahead(c_, form, budget, stop_, counter, scores, want_stats))
    monkeypatch.setattr(TB, "_want_of", lambda c_, flags, own=None: _want_of_closure(c_, form, budget, mine))
    try:
        return TB._check_beam_op(c, c["flags"], stop, seen)
    finally:
        monkeypatch.setattr(TB, "_run_beam_op", _PLAIN_RUN)
        monkeypatch.setattr(TB, "_want_of", _PLAIN_WANT)


def _same_bits(a, b):
    v = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return torch.equal(v(a), v(b))


def _check_width_one_is_the_greedy_ahead_step(c, form, budget, stop):
    """Identity (a) in the operator: W = 1, score zero (-0.0 on the unfinished rows, section 34's note) -- every output bit-equal to
    ops.pointer_sequence_constrained_ahead's."""
    counter, counter2 = torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_ahead(c, form, budget, stop, counter, scores=np.where(c["fin"] != 0, 0.0, -0.0))
    lg2, ref = TCL._run_closure(c, form, budget, counter=counter2)
    assert torch.equal(lg, lg2) and int(counter.item()) == int(counter2.item())
    for k in ("next", "fin", "dead_end", "first", "prev", "visited", "mask_rows", "rows", "stats"):
        assert torch.equal(res[k], ref[k]), (c["S"], form, budget, stop, k)
    assert _same_bits(res["scores"], ref["logprob"]) and not bool(res["parent"].any()), (c["S"], form, budget, stop)


@pytest.mark.gpu
@pytest.mark.parametrize("S,W", [(S, W) for S in BC.OP_S for W in BC.OP_W if W <= S])
def test_operator_against_the_numpy_rule(hip_lib, monkeypatch, S, W):
    seen = dict(dead=0, closing=0, cleared=0, kept=0, eos=0)
    mine = dict(stricter=0, dead=0, closing=0)
    for G, once, form, stop, kind, budget, seed, hmax in BC.op_cases(S, W):
        c = _beam_closure_case(S, W, G, once, kind, seed, hmax)
        _check_ahead(monkeypatch, c, form, budget, stop, seen, mine)
        if W == 1:
            _check_width_one_is_the_greedy_ahead_step(c, form, budget, stop)
        if form == "lookahead":
            # identity (b): both tables zero are the plain operator, bit for bit
            zero = (np.zeros_like(c["close_dist"]), np.zeros_like(c["cycle_len"]))
            ca, cb = torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
            lg0, a0 = _run_ahead(c, "lookahead", budget, stop, ca, tables=zero)
            lg1, a1 = _PLAIN_RUN(c, c["flags"], stop, cb)
            assert all(_same_bits(a0[k], a1[k]) for k in a1) and torch.equal(lg0, lg1) and int(ca.item()) == int(cb.item()), (S, W, kind, once)
            # identity (c): per beam row the edge keys "exact" masks contain those "lookahead" masks
            la, ex = _run_ahead(c, "lookahead", budget, stop)[1], _run_ahead(c, "exact", budget, stop)[1]
            dead = {f: _want_of_closure(c, f, budget) for f in BC.FORMS}
            for b in range(c["B"]):
                g, k = divmod(b, W)
                if dead["exact"][g]["masked"][k] is None or dead["exact"][g]["dead_now"][k] or dead["lookahead"][g]["dead_now"][k]:
                    continue
                assert not bool((la["mask_rows"][b, NTOK:] & ~ex["mask_rows"][b, NTOK:] & 1).any()), (S, W, kind, once, budget, b)
    print("S=%d W=%d:" % (S, W), seen, mine)
    assert mine["stricter"] and mine["dead"], mine
    if S >= 65:
        assert mine["closing"], mine


@pytest.mark.gpu
def test_exact_operator_at_2048_keys_searches_chunk_17_for_one_beam_only(hip_lib, monkeypatch):
    """32 chunks of 64 keys.  A ring of all 2044 edges, one group of two beams: beam 0 is open at edge 1100 with first = 1105 -- its
    one follower, key 4 + 1101 in chunk 17, closes within budget 5 and not within 3 -- beam 1 is closed."""
    S, W = 2048, 2
    c = _beam_closure_case(S, W, 1, False, "ring", 5)
    c["fin"][:] = 0
    c["mask"][:] = False
    c["kv"][:] = S
    c["pad"][:] = False
    c["scores"] = np.array([-1.0, -2.0])
    c["first"][0], c["prev"][0], c["visited"][0] = 1105, 1100, {1100}
    c["first"][1], c["prev"][1], c["visited"][1] = -1, -1, set()
    seen, mine = dict(dead=0, closing=0, cleared=0, kept=0, eos=0), dict(stricter=0, dead=0, closing=0)
    got, own = _check_ahead(monkeypatch, c, "exact", 5, "all", seen, mine)
    kids = [(int(p), int(t)) for p, t in zip(got["parent"], got["next"])]
    assert (0, NTOK + 1101) in kids or all(p == 1 for p, t in kids)
    assert (own[0] > FILL).sum() == 1 and own[0][NTOK + 1101] > FILL and (NTOK + 1101) // 64 == 17
    got, own = _check_ahead(monkeypatch, c, "exact", 3, "all", seen, mine)
    assert (own[0] > FILL).sum() == 1 and own[0][SEP] > FILL                                  # a dead end: SEP alone
    assert mine["dead"] == 1 and mine["stricter"]


class _AheadLib:
    """The library with ff_beam_sequence_constrained_select standing for the _ahead entry, so that section 34's raw call (every
    output a sentinel, optionally inside guarded surroundings) reaches it with the same descriptor."""
    def __init__(self, lib, form, cd, cl, budget):
        self.lib, self.tail = lib, (form, None if cd is None else cd.data_ptr(), None if cl is None else cl.data_ptr(), budget)

    def ff_beam_sequence_constrained_select(self, d, stream):
        return self.lib.ff_beam_sequence_constrained_select_ahead(d, *self.tail, stream)


@pytest.mark.gpu
def test_operator_inside_poisoned_surroundings(hip_lib):
    import redzone as RZ
    c = _beam_closure_case(65, 3, 5, True, "random", 9)
    for form in (1, 2):
        got = {}
        for fill in (RZ.ZERO, RZ.POISON):
            g = RZ.Guard(fill)
            cd, cl = (g.embed(torch.from_numpy(np.ascontiguousarray(c[k]))) for k in ("close_dist", "cycle_len"))
            rc, keep, outs = TB._raw_step(_AheadLib(hip_lib, form, cd if form == 1 else None, cl, 2), c, flags=c["flags"], guard=g)
            assert rc == 0
            g.check()                                                     # nothing outside the operands and outputs is written
            got[fill] = {k: v.clone() for k, v in outs.items()}
        for k in got[RZ.ZERO]:
            if k != "mask_rows":                                          # (rows of empty / finished beams keep the sentinel in both)
                RZ.assert_same_bits(got[RZ.ZERO][k], got[RZ.POISON][k], "%s, form %d" % (k, form))      # nothing outside them is read
        want = _want_of_closure(c, BC.FORMS[form - 1], 2)
        tok = got[RZ.POISON]["next_tok"].cpu().numpy()
        assert all(np.array_equal(tok[g * 3:(g + 1) * 3], w["tok"]) for g, w in enumerate(want) if w["gap"] > 1.0)
        assert sum(int(w["dead_now"].sum()) for w in want) > 0


@pytest.mark.gpu
def test_operator_err_arg_leaves_the_outputs_untouched(hip_lib):
    lib = hip_lib
    c = _beam_closure_case(65, 3, 5, False, "random", 3)
    wide = _beam_closure_case(2052, 2, 1, False, "chain", 3, hmax=8)                  # 2052 keys: above the exact search's limit
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tabs = {id(x): (dev(x["close_dist"]), dev(x["cycle_len"])) for x in (c, wide)}

    def call(case, form=1, budget=2, cd=True, cl=True, over=None, flags=None):
        t = tabs[id(case)]
        return TB._raw_step(_AheadLib(lib, form, t[0] if cd else None, t[1] if cl else None, budget), case,
                            flags=case["flags"] if flags is None else flags, over=over)
    for form in (1, 2):
        rc, keep, outs = call(c, form)
        assert rc == 0 and int(outs["next_tok"].min()) >= 0, form                    # the arguments are good ones
    assert call(c, 2, cd=False)[0] == 0                                              # "exact" reads no close_dist
    assert call(wide, 1)[0] == 0                                                     # the static form has no key limit
    cases = [(c, dict(form=0)), (c, dict(form=3)), (c, dict(form=-1)), (c, dict(flags=1)), (c, dict(flags=5)), (c, dict(flags=0)),
             (c, dict(form=2, flags=2)), (c, dict(cd=False)), (c, dict(cl=False)), (c, dict(form=2, cl=False)), (c, dict(budget=-1)),
             (c, dict(budget=255)), (c, dict(form=2, budget=255)), (wide, dict(form=2))]
    # everything section 34's operator refuses
    cases += [(c, dict(over=o)) for o in (dict(flags=8 | 3), dict(flags=6), dict(follows=None), dict(tok_sep=EOS), dict(tok_eos=NTOK),
                                          dict(L=c["L"] - 1), dict(groups_per_wireframe=0), dict(S=0), dict(groups=0), dict(width=0),
                                          dict(width=9), dict(stop_best=2), dict(visited_out="visited_in"), dict(mask_rows=None),
                                          dict(next_tok=None), dict(parent=None), dict(open_out=None), dict(visited_in=None),
                                          dict(logits=None), dict(ldnext=E_OP - 4))]
    for case, kw in cases:
        rc, keep, outs = call(case, **kw)
        assert rc == -1, (kw, rc)                                                     # FF_ERR_ARG
        assert torch.equal(keep["logits"].cpu(), torch.from_numpy(case["logits"])), kw
        assert torch.equal(keep["visited"].cpu(), torch.from_numpy(_words(case["visited"], case["L"]))), kw
        assert bool((outs["mask_rows"] == 77).all()) and bool((outs["next_rows"] == 7.5).all()) and bool((outs["scores_out"] == 7.5).all()), kw
        assert all(bool((outs[k] == -7).all()) for k in ("next_tok", "parent", "fin_out", "dead_out", "open_out", "first_out", "prev_out",
                                                         "visited_out")), kw
        assert int(outs["count"].item()) == 5, kw
    assert lib.ff_beam_sequence_constrained_select_ahead(None, 1, None, None, 2, None) == -1 and b"null descriptor" in lib.ff_last_error()
    with pytest.raises(ValueError, match="closure='ahead': must be 'lookahead' or 'exact'"):
        _run_ahead(c, "ahead", 2, "all")
    with pytest.raises(ValueError, match="budget=255: must be in 0..254"):
        _run_ahead(c, "exact", 255, "all")
    with pytest.raises(ValueError, match="takes at most 2048 keys"):
        _run_ahead(wide, "exact", 2, "all")


# ---- GPU: the engine ----------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _cbc(fix, flags, W, form, stop="all", tables=None, **kw):
    """The engine's beam decode of a fixture under `form` (None: the plain sequence_constrain_beams decode)."""
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    if form is not None:
        cd, cl = tables if tables is not None else TCL._tables(fix)[2:]
        kw.update(sequence_constrain_beam_closure=form, cycle_len=cl, **({} if form == "exact" else dict(close_dist=cd)))
    return TB._cb(model, case, b, flags, table, W, stop, **kw)


def _run(fix, flags, W, form, stop="all"):
    key = (fix, flags, W, form, stop)
    if key not in _RUNS:
        _RUNS[key] = _cbc(fix, flags, W, form, stop, trace=True)
    return _RUNS[key]


def _guarantees(out, fix, flags, W, form):
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    bm, sc, de, oe = (out[k].cpu().numpy() for k in ("beams", "beam_scores", "beam_dead_end", "beam_open_end"))
    return BC.guarantees(bm, de, oe, sc, W, batch["num_input"], flags, NTOK, SEP, EOS, follows, edges, form)


def _replay_ahead(monkeypatch, out, fix, flags, W, form, stop, what):
    """Section 34's replay (the decode's own trace_logits under the numpy rule, step by step, the same cap) with every step under
    the form, the decode's own tables and the step's budget."""
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    cd, cl = TCL._tables(fix)[:2]
    T = case["model"]["seq_len"]

    def beam_step(lg, pads, scores, fin, states, W_, flags_, ntok, sep, eos, follows_, margin=1):
        return BC.beam_step(lg, pads, scores, fin, states, W_, flags_, ntok, sep, eos, follows_, form, cd, cl, BC.budget_of(T, margin), margin)
    monkeypatch.setattr(CB, "beam_step", beam_step)      # (the replay calls it with margin = step + 1 = the position the step selects)
    try:
        return TB._check_replay(out, case, batch["num_input"], W, flags, follows, stop, what)
    finally:
        monkeypatch.undo()


@pytest.mark.gpu
@pytest.mark.parametrize("form", BC.FORMS)
@pytest.mark.parametrize("flags", BC.FLAGS)
@pytest.mark.parametrize("fix", BC.FIXTURES, ids=lambda f: "%s-%s%d" % f)
def test_engine_with_one_beam_is_the_closure_greedy_decode_and_zero_tables_are_the_plain_beams(hip_lib, fix, flags, form):
    """Identity (a) on both stop rules: tokens, dead_end, open_end and steps exact, |score - sum logprob| <= (T - 1) 2^-16.
    Identity (b) at W = 4: "lookahead" with zero tables is the plain sequence_constrain_beams decode, bit for bit."""
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T = case["model"]["seq_len"]
    greedy = TCL._closure(fix, flags, form)
    want = greedy["logprob"].cpu().numpy().astype(np.float64).sum(axis=1)
    for stop in BC.STOPS:
        out = _cbc(fix, flags, 1, form, stop)
        assert out["steps"] == greedy["steps"] and out["step_counts"] == greedy["step_counts"], (fix, flags, form, stop)
        assert torch.equal(out["beams"], greedy["predict"]) and torch.equal(out["predict"], greedy["predict"]), (fix, flags, form, stop)
        assert torch.equal(out["beam_dead_end"], greedy["dead_end"]) and torch.equal(out["beam_open_end"], greedy["open_end"])
        err = np.abs(out["beam_scores"].cpu().numpy().astype(np.float64) - want).max()
        assert err <= (T - 1) * R.LP_BAR, (fix, flags, form, stop, err)
        TB._check_layout(out, T, 1, stop, flags, follows)
    if form == "lookahead":
        cd, cl = TCL._tables(fix)[2:]
        for stop in BC.STOPS:
            zero = _cbc(fix, flags, 4, form, stop, tables=(torch.zeros_like(cd), torch.zeros_like(cl)), trace=True)
            plain = _cbc(fix, flags, 4, None, stop, trace=True)
            assert zero["steps"] == plain["steps"] and zero["step_counts"] == plain["step_counts"], (fix, flags, stop)
            n = zero["steps"]
            for k in TB.KEYS:
                assert _same_bits(zero[k], plain[k]), (fix, flags, stop, k)
            assert torch.equal(zero["beam_parent"][:n], plain["beam_parent"][:n]) and _same_bits(zero["logits"][:n], plain["logits"][:n])


REPLAY = [f + (flags, W, form) for f in BC.FIXTURES for flags in BC.FLAGS for W in BC.REPLAY_W for form in BC.FORMS]


@pytest.mark.gpu
@pytest.mark.parametrize("tup", REPLAY, ids=lambda t: "%s-%s%d-f%d-W%d-%s" % t)
def test_engine_beams_replay_under_the_numpy_rule_and_keep_the_guarantees(hip_lib, monkeypatch, tup):
    """The (golden, kind, seed, flags, W, form) tuples are the helper's: kept on the CPU by
    tools/sequence_constrain_beam_closure_left_out.py engine."""
    fix, flags, W, form = tup[:3], tup[3], tup[4], tup[5]
    assert tup in BC.KEPT, "not a kept tuple"
    out = _run(fix, flags, W, form)
    enc, par, dead, late = _guarantees(out, fix, flags, W, form)                             # (g1)-(g3) on every non-empty final beam
    live = torch.isfinite(out["beam_scores"])
    opens = int(out["beam_open_end"][live].sum())
    print(tup, "steps=%d enclosed %d of %d parsed; dead ends %d (late %d); open ends %d" % (out["steps"], enc, par, dead, late, opens))
    okb, left = _replay_ahead(monkeypatch, out, fix, flags, W, form, "all", tup)
    kept = BC.KEPT[tup]
    if left == 0 and kept[0] == 0:                                                           # nothing left out on either side
        assert (enc, par, dead, late, opens, out["steps"]) == kept[2:], (tup, (enc, par, dead, late, opens, out["steps"]), kept)
    if flags == LOOPS and fix in BC.OPEN_AT_T and W == 2:                                    # the defect the issue names, gone
        plain = _run(fix, flags, W, None)
        pl = torch.isfinite(plain["beam_scores"])
        assert int(plain["beam_open_end"][pl].sum()) > 0 and opens == 0, tup


@pytest.mark.gpu
@pytest.mark.parametrize("form", BC.FORMS)
@pytest.mark.parametrize("fix", [("seq_small_gain4", "lattice", 2), ("seq_small_eos", "lattice", 1), ("seq_small_repeat_eos", "random", 2)],
                         ids=lambda f: "%s-%s%d" % f)
def test_engine_best_against_all_and_scores_against_the_teacher_forced_oracle(hip_lib, fix, form):
    """Identity (e): "best" stops no later than "all" with the same best beam; scores within section 34's bar of the fp64 oracle
    forced along the final beams, every step under the form's mask."""
    from test_parity_golden import _tol
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, W, flags = case["model"]["seq_len"], 4, COEDGE
    ni = batch["num_input"]
    al, be = _run(fix, flags, W, form, "all"), _run(fix, flags, W, form, "best")
    assert be["steps"] <= al["steps"]
    bm, sc, fin, de, oe, pos, steps = TB._check_layout(be, T, W, "best", flags, follows)
    first_done = (al["beam_finished"].view(-1, W)[:, 0] != 0)
    if bool(first_done.all()):
        assert torch.equal(be["predict"], al["predict"]), (fix, form)
        assert _same_bits(be["beam_scores"].view(-1, W)[:, 0], al["beam_scores"].view(-1, W)[:, 0]), (fix, form)
    # the fp64 oracle forced along the final beams of "all", the rule's renormalisation under the form
    bm, sc, fin, de, oe, pos, steps = TB._check_layout(al, T, W, "all", flags, follows)
    import test_sequence_constrain as TS
    cd, cl = TCL._tables(fix)[:2]
    S = case["model"]["L"] + NTOK
    rep = torch.arange(len(ni)).repeat_interleave(W)
    rb = {k: (v.index_select(0, rep) if torch.is_tensor(v) and v.dim() and v.size(0) == len(ni) else v) for k, v in batch.items()}
    truth = TS._oracle_logits(case, sd, rb, bm, steps)
    states = SC.replay_states(bm, flags, NTOK, SEP, [follows[r // W] for r in range(bm.shape[0])])
    for r in np.flatnonzero(np.isfinite(sc)):
        w, total, bar = r // W, 0.0, 0.0
        pad = np.arange(S) >= NTOK + ni[w]
        for j in range(min(int(pos[r]), steps)):
            masked, _ = faces.sequence_rule_mask(states[r][j], flags, S, NTOK, SEP, EOS, follows[w], pad,
                                                 **BC.closure_kw(form, cd, cl, w, BC.budget_of(T, j + 1)))
            row = np.where(masked | pad, FILL, truth[j, r].astype(np.float64))
            t = int(bm[r, j + 1])
            assert row[t] > FILL, (fix, form, int(r), j)
            total += (row[t] - row.max()) - np.log(np.exp(row - row.max()).sum())
            bar += 2 * _tol(truth[j][r:r + 1]) + R.LP_BAR
        assert abs(sc[r] - total) <= bar + R.ADD_EPS * abs(total) * max(steps, 1), (fix, form, int(r), sc[r], total, bar)


@pytest.mark.gpu
def test_engine_micro_batch_cut_and_repeatability(hip_lib, monkeypatch):
    fix, flags, W = ("seq_small_gain4", "random", 2), COEDGE, 4
    for form in BC.FORMS:
        whole, again = _cbc(fix, flags, W, form, trace=True), _cbc(fix, flags, W, form, trace=True)
        assert whole["steps"] == again["steps"] and whole["step_counts"] == again["step_counts"]
        n = whole["steps"]
        for k in TB.KEYS + ("logits", "beam_parent"):                                         # one plan, two runs: bit-equal
            assert _same_bits(whole[k][:n] if k in ("logits", "beam_parent") else whole[k], again[k][:n] if k in ("logits", "beam_parent") else again[k]), (form, k)
        one = _cbc(fix, flags, W, form, trace=True, chunk_max_seqs=W)                         # one wireframe's beams, and its own table rows, per micro-batch
        okw, lw = _replay_ahead(monkeypatch, whole, fix, flags, W, form, "all", (fix, form, "whole"))
        oko, lo = _replay_ahead(monkeypatch, one, fix, flags, W, form, "all", (fix, form, "cut"))
        if lw == 0 and lo == 0:
            for k in ("beams", "beam_finished", "beam_dead_end", "beam_open_end", "predict"):
                assert torch.equal(whole[k], one[k]), (form, k)


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    m = WP._bound("seq_small_gain4", "default")
    batch, follows, _ = SC.fixture(m.case, m.batch, "random", 2)
    b = batch_to(batch, "cuda")
    table = torch.from_numpy(faces.pack_follow_bits(follows)).cuda()
    cd, cl = (torch.from_numpy(t).cuda() for t in BC.tables(follows, m.case["model"]["seq_len"], batch["num_input"]))
    for form in BC.FORMS:
        call = lambda: TB._cb(m.model, m.case, b, LOOPS, table, 3, "all", trace=True, sequence_constrain_beam_closure=form, cycle_len=cl,
                              **({} if form == "exact" else dict(close_dist=cd)))
        clean = call()
        zero, d = WP._run([m], call, fill=RZ.ZERO, what="sequence beam closure after ZERO")
        poison, _ = WP._run([m], call, fill=RZ.POISON, what="sequence beam closure after POISON")
        WP._assert_equal(poison, zero, "sequence beam closure")
        WP._assert_equal(poison, clean, "sequence beam closure against the clean run")
        assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size
        live = torch.isfinite(zero["beam_scores"])
        assert int(zero["beam_dead_end"].sum()) > 0 and not bool(zero["beam_open_end"][live].any())


@pytest.mark.gpu
def test_engine_takes_a_row_longer_than_256_with_the_clamped_budget(hip_lib, monkeypatch):
    """T = 259 (config A's) on a narrow synthetic model and a lattice wireframe: the entry accepts it, the replay holds with
    budget = min(T - 1 - p, 254), and no non-empty beam ends with a loop open."""
    import constrain_ref as CR
    import test_sequence_constrain as TS
    from conftest import build_model
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    L, T, E = 24, 259, 64
    case = dict(kind="seq2seq", model=dict(L=L, seq_len=T, E=E, FF=128, H=1, enc=1, dec=1), recipe="gain4", wseed=7)
    sd = make_state_dict(state_dict_spec("seq2seq", L, T, E, 128, 1, 1), "gain4", 7)
    model = build_model(case, sd, "cuda")
    ni = [22, 17]
    batch, edges, _ = CR.lattice_batch(ni, L, T, 3)
    batch["label"] = torch.zeros((len(ni), T), dtype=torch.int64)
    follows = faces.follow_table(batch["input"].numpy(), SC.TOL, ni)
    fix = ("t259", "lattice", 3)
    TS._FIX[fix] = (case, model, batch_to(batch, "cuda"), batch, follows, torch.from_numpy(faces.pack_follow_bits(follows)).cuda(), edges, sd)
    assert BC.hmax_of(T) == 254 and BC.budget_of(T, 4) == 254 and BC.budget_of(T, 5) == 253
    try:
        for form in BC.FORMS:
            out = _cbc(fix, COEDGE, 2, form, trace=True)
            _guarantees(out, fix, COEDGE, 2, form)
            okb, left = _replay_ahead(monkeypatch, out, fix, COEDGE, 2, form, "all", (fix, form))
            assert out["steps"] > 0
    finally:
        TS._FIX.pop(fix, None)
        TCL._TABLES.pop(fix, None)


# ---- GPU: the model and the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_publishes_the_keys_builds_or_takes_the_tables_and_sequence_faces_works_behind_it(hip_lib):
    fix = ("seq_small_gain4", "lattice", 2)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N, W = case["model"]["seq_len"], b["input"].size(0), 3
    cd, cl, cd_dev, cl_dev = TCL._tables(fix)
    try:
        with torch.no_grad():
            model.sequence_constrain, model.sequence_constrain_beams = "coedge_loops", W
            plain = model(dict(b))
            for form in BC.FORMS:
                model.sequence_constrain_beam_closure = form
                on = model(dict(b))                                       # the tables are built on the device from the follow table
                given = model(dict(b, follow_table=table, close_dist=torch.from_numpy(cd), cycle_len=cl_dev))
                assert set(on) == set(plain)                              # the published keys are the plain beam decode's
                direct = _cbc(fix, COEDGE, W, form)
                for k, d in (("predict", "predict"), ("predict_beams", "beams"), ("predict_beam_scores", "beam_scores"),
                             ("predict_beam_finished", "beam_finished"), ("predict_beam_dead_end", "beam_dead_end"),
                             ("predict_beam_open_end", "beam_open_end"), ("predict_dead_end", "dead_end"), ("predict_open_end", "open_end")):
                    assert _same_bits(on[k], given[k]) and _same_bits(on[k].reshape(direct[d].shape), direct[d]), (form, k)
                    assert on[k].dtype == plain[k].dtype and on[k].shape == plain[k].shape
                assert tuple(on["predict_beams"].shape) == (N, W, T)
                assert not bool(on["predict_beam_open_end"][torch.isfinite(on["predict_beam_scores"])].any())
                model.sequence_faces = "enclosed"                         # G = W rows per wireframe behind the option
                both = model(dict(b))
                model.sequence_faces = False
                assert int(both["sequence_faces"]["num_faces"].sum()) > 0 and torch.equal(both["predict_beams"], on["predict_beams"])
                model.sequence_faces = "enclosed"
                model.sequence_constrain_beam_closure = None
                ref = model(dict(b))
                model.sequence_faces = False
                assert set(both["sequence_faces"]) == set(ref["sequence_faces"])
    finally:
        model.sequence_constrain = model.sequence_constrain_beam_closure = None
        model.sequence_constrain_beams, model.sequence_faces = 0, False


@pytest.mark.gpu
def test_cli_records_with_and_without_the_flag(hip_lib, tmp_path):
    import constrain_ref as CR
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    root = tmp_path / "data"
    (root / "json").mkdir(parents=True)
    names = []
    for i in range(2):
        polys, _ = CR.lattice_edges(8 + 4 * i, 40 + i)
        raw = {"edges": [[[float(p[0][0]), float(p[0][1])], [float(p[-1][0]), float(p[-1][1])]] for p in polys],
               "faces_indices": [[[0, 1, 2]], [[3, 4, 5]]], "pairings": {}, "dominant_directions": [[1, 0, 0]]}
        json.dump(raw, open(root / "json" / ("%08d.json" % i), "w"))
        names.append("json/%08d.json" % i)
    open(root / "test.txt", "w").write("\n".join(names) + "\n")
    cfg = load_cfg("configs/seq2seq.yml", ["model.num_lines", "16", "model.label_seq_length", "24", "model.num_model", "128",
                                            "model.num_head", "2", "model.num_feedforward", "256", "model.num_encoder_layers", "2",
                                            "model.num_decoder_layers", "2", "root_dir", str(root), "post_process.is_coedge", "False"])
    sd = make_state_dict(state_dict_spec("seq2seq", 16, 24, 128, 256, 2, 2), "gain4", 51)
    ckpt = tmp_path / "last.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(cfg)}, ckpt)
    run = lambda d, **kw: cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / d), **kw)
    beams = run("beams", sequence_constrain="loops", sequence_constrain_beams=3)
    beams2 = run("beams2", sequence_constrain="loops", sequence_constrain_beams=3, sequence_constrain_beam_closure=None)
    for form in BC.FORMS:
        ahead = run("ahead_" + form, sequence_constrain="loops", sequence_constrain_beams=3, sequence_constrain_beam_closure=form,
                    sequence_beam_stop="best")
        for fn in sorted(os.listdir(beams)):
            text = open(os.path.join(beams, fn)).read()
            assert text == open(os.path.join(beams2, fn)).read()          # byte-identical without the flag
            rp, ra = (json.load(open(os.path.join(d, fn))) for d in (beams, ahead))
            assert list(ra) == list(rp)                                   # the record keys are section 34's
            assert ra["pred_unclosed"] <= ra["pred_dead_ends"]            # beam 0 leaves no face open at the end of the row
