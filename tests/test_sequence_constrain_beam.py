"""Opt-in beam search over the loop-constrained single-sequence decode (SurfaceFormer.sequence_constrain_beams): the
numpy rule on hand-written groups, its identities, every refusal and the CLI on the CPU (library untouched); the selection step, the
engine's mode, the model and the CLI on the GPU, through the C ABI.  The rule is tests/sequence_constrain_beam_ref.py's, which
composes faces.sequence_rule_mask / sequence_rule_advance with beam_ref and sequence_beam_ref and restates none of them.

Bars (the issue's, none measured): byte rows, FILL patterns, parents, tokens, flags, states, visited words, appended rows and
counters are exact on every DECISIVE group (every decisive gap above twice beam_ref.score_bound, times the steps accumulated); a
score lies within score_bound of fp64 on the kernel's own masked rows; at most 2 % of a case's groups / (step, group) pairs may be
left out -- a condition on the inputs, fixed on the CPU by tools/sequence_constrain_beam_left_out.py; scores within sum 2 tol(step)
+ 2^-16 of the fp64 oracle forced along the final beams; identity (a) |score - sum logprob| <= (T - 1) 2^-16."""
import json
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import beam_ref as R
import constrain_ref as CR
import sequence_beam_ref as QB
import sequence_constrain_beam_ref as CB
import sequence_constrain_ref as SC
from conftest import ROOT, batch_to, token_ns
from faceformer_amd import faces
from faceformer_amd.hip.modes import SEQUENCE_CONSTRAIN_BEAM, sequence_constrain_beams_value      # (without them nothing here can pass)
from test_sequence_constrain import (E_OP, SMALL, _constrained, _decode, _fixture, _model, _operator_case, _seq_inputs, _table,
                                     _tiny_model, _untouchable, _words)

TOK = token_ns()
NTOK, SOS, SEP, EOS = TOK.len, TOK.SOS, TOK.SEP, TOK.EOS
FILL, NEG = CB.FILL, CB.NEG
LOOPS, COEDGE = CB.LOOPS, CB.COEDGE_LOOPS
START = faces.sequence_rule_start()


# ---- CPU: the numpy rule on hand-written groups -------------------------------------------------------------------------------------
def _both(raw, scores, fin, states, flags, follows, pad=None):
    """The helper's group step and faces' own restatement on one group: they must agree on everything they share."""
    raw = np.asarray(raw, dtype=np.float64)
    pad = np.zeros(raw.shape[1], bool) if pad is None else np.asarray(pad, bool)
    a = CB.group_step(raw, pad, np.asarray(scores, float), np.asarray(fin, bool), list(states), flags, NTOK, SEP, EOS, follows)
    b = faces.sequence_rule_beam_step(raw, pad, np.asarray(scores, float), np.asarray(fin, bool), list(states), flags, NTOK, SEP, EOS, follows)
    for k in ("parent", "tok", "fin", "dead", "open"):
        assert np.array_equal(a[k], b[k]), k
    assert a["states"] == b["states"] and np.allclose(a["scores"], b["scores"], rtol=0, atol=1e-12, equal_nan=True)
    for k in range(raw.shape[0]):
        if a["masked"][k] is not None:
            assert np.array_equal(a["masked"][k], b["masked"][k]) and np.array_equal(a["rows"][k], b["rows"][k])
    return a


def test_rule_on_hand_written_groups():
    L = 6
    S = NTOK + L
    t = _table(L, [(0, 1), (1, 2), (2, 0), (3, 3), (4, 5)])
    g = np.random.default_rng(11)
    raw = g.standard_normal((2, S))
    # two beams of one group in different faces with different visited: each row is masked by its own state
    a_state, b_state = (frozenset({0}), 0, 0), (frozenset({0, 1, 2, 4}), 4, 4)
    r = _both(raw, [-1.0, -2.0], [False, False], [a_state, b_state], LOOPS, t)
    assert r["rows"][0][NTOK + 1] > FILL and (r["rows"][0][[i for i in range(S) if i != NTOK + 1]] <= FILL).all()
    assert r["rows"][1][NTOK + 5] > FILL and (r["rows"][1][[i for i in range(S) if i != NTOK + 5]] <= FILL).all()
    assert r["tok"].tolist() == [NTOK + 1, NTOK + 5] and r["parent"].tolist() == [0, 1] and r["scores"].tolist() == [-1.0, -2.0]
    assert r["states"] == [(frozenset({0, 1}), 0, 1), (frozenset({0, 1, 2, 4, 5}), 4, 5)] and r["open"].all()
    # one parent yields two children, one on SEP and one on an edge: their visited sets diverge (cleared / grown); ONCE keeps them
    closed = (frozenset({0, 1, 2}), None, 2)
    row = np.full(S, -30.0)
    row[SEP], row[NTOK + 3] = 2.0, 1.0
    for flags, sep_vis in ((LOOPS, frozenset()), (COEDGE, frozenset({0, 1, 2}))):
        r = _both(np.stack([row, row]), [0.0, NEG], [False, False], [closed, START], flags, t)
        assert r["parent"].tolist() == [0, 0] and r["tok"].tolist() == [SEP, NTOK + 3]
        assert r["states"][0] == (sep_vis, None, None) and r["states"][1] == (frozenset({0, 1, 2, 3}), None, 3)      # 3 closes on itself
        assert r["open"].tolist() == [False, False] and r["scores"][0] > r["scores"][1] > -2.0
    # a dead-ended beam: its only candidate is SEP at unchanged score, and the closed empty state follows; the face, not the beam, ends
    dead_state = (frozenset({4, 5}), 4, 5)
    r = _both(raw, [-3.5, NEG], [False, False], [dead_state, START], LOOPS, t)
    assert r["tok"][0] == SEP and r["scores"][0] == -3.5 and r["dead"][0] and not r["fin"][0] and r["states"][0] == START
    assert r["scores"][1] == NEG and r["parent"][1] == 1 and not r["dead"][1] and r["states"][1] == START      # an empty rank
    # EOS is never a candidate while a loop is open, however large its logit
    push = raw.copy()
    push[:, EOS] = 1e4
    r = _both(push, [-1.0, -1.5], [False, False], [a_state, b_state], LOOPS, t)
    assert EOS not in r["tok"].tolist() and not r["fin"].any()
    r = _both(push, [-1.0, NEG], [False, False], [closed, START], LOOPS, t)
    assert r["tok"][0] == EOS and r["fin"][0] and abs(r["scores"][0] + 1.0) < 1e-9
    # a finished rank 0 keeps rank 0 on an exact tie: its flat index k * S is the lowest of its score
    tie = np.full((2, S), -60.0)
    tie[1, NTOK + 3] = 0.0                     # beam 1: one live key with log-probability 0 (to 1e-26) -> the finished beam's score
    r = _both(tie, [-2.0, -2.0], [True, False], [closed, closed], 0, None)
    assert r["parent"].tolist() == [0, 1] and r["fin"].tolist() == [True, False] and r["tok"].tolist() == [0, NTOK + 3]
    # a row with no live key: token 0 at c - log S
    r = _both(raw, [-1.0, NEG], [False, False], [START, START], 0, None, pad=np.ones(S, bool))
    assert r["tok"][0] == 0 and abs(r["scores"][0] - (-1.0 - math.log(S))) < 1e-12
    # a group with fewer than W candidates leaves its last ranks empty
    one = np.full((3, S), -50.0)
    r = _both(one, [0.0, NEG, NEG], [False] * 3, [(frozenset({0}), 0, 0)] * 3, LOOPS, t)
    assert np.isfinite(r["scores"]).tolist() == [True, False, False] and r["parent"].tolist() == [0, 1, 2]


def _scripted(scripts, S, W, hot=40.0):
    """A logit source that pushes beam-independent scripts: group g at step j prefers scripts[g][j] (then EOS)."""
    def step_logits(prefixes, j):
        rows = np.zeros((len(scripts) * W, S))
        for g, sc in enumerate(scripts):
            rows[g * W:(g + 1) * W, sc[j] if j < len(sc) else EOS] = hot
        return rows
    return step_logits


def test_best_stops_before_all_and_the_decode_is_laid_out():
    L, T, W = 5, 12, 3
    S = NTOK + L
    t = _table(L, [(0, 1), (1, 2), (2, 0), (3, 3), (4, 1)])
    pads = np.zeros((2, S), bool)
    follows = np.stack([t, t])
    src = _scripted([[NTOK + 0, NTOK + 1, NTOK + 2, EOS], [NTOK + 3, SEP, NTOK + 0, NTOK + 1, NTOK + 2, EOS]], S, W)
    al = CB.decode(src, pads, W, T, COEDGE, NTOK, SOS, SEP, EOS, follows, "all")
    be = CB.decode(src, pads, W, T, COEDGE, NTOK, SOS, SEP, EOS, follows, "best")
    mine = faces.sequence_rule_beam_decode(src, pads, W, T, COEDGE, NTOK, SOS, SEP, EOS, follows, "best")
    assert be["steps"] < al["steps"] and be["steps"] == CB.stop_step(al["best_counts"], T) == mine["steps"]
    assert np.array_equal(be["beams"][::W], al["beams"][::W]) and np.array_equal(be["scores"][::W], al["scores"][::W])
    assert np.array_equal(mine["beams"], be["beams"]) and np.array_equal(mine["dead_end"], be["dead_end"]) and mine["counts"] == be["counts"]
    assert al["beams"][0, :5].tolist() == [SOS, NTOK, NTOK + 1, NTOK + 2, EOS] and (al["beams"][0, 5:] == 0).all()
    assert al["beams"][W, :8].tolist() == [SOS, NTOK + 3, SEP, NTOK, NTOK + 1, NTOK + 2, EOS, 0]
    assert al["counts"][-1] == 0 and all(v > 0 for v in al["counts"][:-1]) and al["fin"][np.isfinite(al["scores"])].all()
    enc, par, de = CB.guarantee(al["beams"], al["dead_end"], al["open"].astype(int), al["scores"], W, [L, L], COEDGE, NTOK, SEP, EOS, follows, None)
    assert enc > 0 and par >= enc


@pytest.mark.parametrize("stop", CB.STOPS)
def test_numpy_identities_a_and_b(stop):
    """(a) W = 1 is sequence_constrain_ref.decode; (b) all flag bits clear is sequence_beam_ref.decode, on a prefix-dependent source."""
    L, T, N = 9, 14, 3
    S = NTOK + L
    follows = CR.random_follows(N, L, 4)
    pads = np.zeros((N, S), bool)
    pads[1, S - 2:] = True
    base = np.random.default_rng(5).standard_normal((T, 64, S)) * 2.0
    base[:, :, EOS] += np.linspace(-3.0, 4.0, T)[:, None]

    def source(W):
        def step_logits(prefixes, j):
            key = (prefixes * np.arange(1, prefixes.shape[1] + 1)).sum(axis=1) % 64      # a function of the prefix
            rows = base[j, key] + 0.01 * (np.arange(prefixes.shape[0]) // W)[:, None]
            return np.where(np.repeat(pads, W, axis=0), FILL, rows)
        return step_logits
    for flags in (LOOPS, COEDGE, SC.NO_REPEAT):
        one = CB.decode(source(1), pads, 1, T, flags, NTOK, SOS, SEP, EOS, follows, stop)
        ref = SC.decode(source(1), N, T, flags, NTOK, SOS, SEP, EOS, follows)
        assert one["steps"] == ref["steps"] and np.array_equal(one["beams"], ref["tokens"]) and np.array_equal(one["dead_end"], ref["dead"])
        assert one["open"].astype(int).tolist() == ref["open_end"].tolist() and np.abs(one["scores"] - ref["logprob"].sum(axis=1)).max() < 1e-9
    W = 3
    zero = CB.decode(source(W), pads, W, T, 0, NTOK, SOS, SEP, EOS, None, stop)
    masked = lambda prefixes, j: source(W)(prefixes, j)
    ref = QB.decode(masked, N, W, T, SOS, EOS, stop)
    assert zero["steps"] == ref["steps"] and zero["counts"] == ref["counts"] and np.array_equal(zero["beams"], ref["beams"])
    assert np.array_equal(zero["scores"], ref["scores"]) and np.array_equal(zero["fin"], ref["fin"]) and not zero["dead_end"].any()


def test_faces_of_the_beams_leave_abandoned_faces_out():
    E, T = NTOK, 14
    rows = np.zeros((3, T), dtype=np.int64)
    rows[0, :8] = [SOS, E + 0, E + 1, E + 2, SEP, E + 4, SEP, EOS]      # a face, then a face abandoned at a dead end
    rows[1, :6] = [SOS, E + 2, E + 1, E + 0, SEP, EOS]                  # the same edge set again, a better score
    rows[2, :5] = [SOS, E + 4, E + 5, SEP, E + 3]                       # unfinished: the open piece loses its last edge
    dead = np.zeros((3, T), dtype=np.int32)
    dead[0, 6] = 1
    sc, fin = np.array([-4.0, -3.0, -5.0]), np.array([1, 1, 0])
    got = faces.parse_faces_constrained_beams_scored(rows, sc, fin, dead, 8, TOK)
    assert [(t, tuple(i), s) for t, i, s in got] == [(0, (0, 1, 2), -3.0), (0, (4, 5), -5.0)]
    same = faces.parse_faces_beams_scored(rows, sc, fin, 8, TOK)          # without the flags the abandoned face counts
    assert len(same) == len(got) + 1
    assert faces.parse_faces_constrained_beams_scored(rows, np.array([NEG, -3.0, NEG]), fin, dead, 8, TOK) == [(0, (2, 1, 0), -3.0)]
    with pytest.raises(ValueError, match="must both be \\[W, T\\]"):
        faces.parse_faces_constrained_beams_scored(rows, sc, fin, dead[:2], 8, TOK)


# ---- CPU: C ABI, binding, sources ---------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_beam_sequence_constrained_select", "ff_decode_sequence_constrained_beam_workspace_bytes",
               "ff_decode_sequence_constrained_beam")


def test_header_binding_and_sources_declare_the_entries_within_abi_105():
    from faceformer_amd.hip import build, lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
        n_args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).count(",") + 1
        assert n_args == len(lib.SIGNATURES[name][1]), name
    assert lib.SIGNATURES[NEW_ENTRIES[1]][1] == lib.SIGNATURES["ff_decode_sequence_beam_workspace_bytes"][1]
    assert len(lib.SIGNATURES[NEW_ENTRIES[2]][1]) == len(lib.SIGNATURES["ff_decode_sequence_sample"][1])
    for struct, cls in (("ff_beam_sequence_constrained_step", lib.BeamSequenceConstrainedStep),
                        ("ff_sequence_constrain_beam_params", lib.SequenceConstrainBeamParams)):
        fields = re.search(r"typedef struct %s \{(.*?)\}" % struct, code, flags=re.S).group(1)
        names = [n.strip().lstrip("*") for f in fields.split(";") if f.strip() for n in f.split(",")]
        assert [n.split()[-1].lstrip("*") for n in names] == [n for n, _ in cls._fields_], struct
    doc = header[header.index("beam search over the loop-constrained single-sequence decode"):]
    for phrase in ("Beam k of wireframe w is row w*W + k", "A masked key is never a candidate", "c_k - log S",
                   "A dead end abandons the face, not the beam", "visited_out must not be visited_in", "every renormalised log-probability is <= 0"):
        assert phrase in doc, phrase                                      # the contract, in the header
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain_seq.hip")).read()
    assert "ff_constrain_seq.hip" in build.SOURCES and len(build.SOURCES) == 17
    assert "beam_sequence_constrained_select_kernel" in src and "ff_sequence_write_row(" in src and "ff_beam_walk<W, true>" in src
    assert "ff_beam_merge<W>" in src and "ff_beam_rank<W>" in src and "asm" not in src and "__syncthreads" not in src and "__shared__" not in src
    assert "ff_dispatch<1, 2, 3, 4, 5, 6, 7, 8>" in src and "ff_dispatch<0, 1>" in src      # 16 instantiations
    for name in ("ff_beam_sequence_select", "ff_decode_sequence_beam", "ff_pointer_sequence_constrained", "ff_decode_sequence_constrained",
                 "ff_decode_sequence_constrained_sample"):
        assert name in lib.SIGNATURES                                     # the existing entries stay


def test_binding_refuses_a_library_without_the_entries(monkeypatch):
    from faceformer_amd.hip import lib

    class Stale:
        def __getattr__(self, name):
            if name in NEW_ENTRIES:
                raise AttributeError(name)
            return types.SimpleNamespace(restype=None, argtypes=None)
    monkeypatch.setattr(lib, "_lib", None, raising=False)
    monkeypatch.setattr(lib.C, "CDLL", lambda path: Stale())
    monkeypatch.setattr(lib.os.path, "exists", lambda p: True)
    with pytest.raises(lib.HipExtensionError, match="does not export ff_(beam_sequence_constrained_select|decode_sequence_constrained_beam)"):
        lib.load()


def test_mode_record_lies_outside_both_tables():
    from faceformer_amd.hip import modes
    rec = SEQUENCE_CONSTRAIN_BEAM
    assert rec not in modes.MODES and rec not in modes.SEQUENCE_MODES and rec not in modes.SEQUENCE_MODEL_ORDER
    assert len(modes.SEQUENCE_MODES) == 3 and len(modes.MODES) == 4 and "sequence_constrain_beams" not in modes.SWITCH
    assert rec.entry == "ff_decode_sequence_constrained_beam" and rec.per_anchor and not rec.term_range and not rec.parallel_only
    assert rec.switches == modes.SEQUENCE_CONSTRAIN.switches             # the option that switches the mode on stays sequence_constrain
    assert [k for k, _, _ in rec.outs] == ["beams", "beam_scores", "beam_finished", "beam_dead_end", "beam_open_end", "dead_end", "open_end"]
    assert [sequence_constrain_beams_value(v, 3) for v in (None, 0, 1, 8)] == [0, 0, 1, 8]
    assert sequence_constrain_beams_value(None, None) == 0 and sequence_constrain_beams_value(0, None, 2, 2, 2) == 0
    for bad in (9, -1, True, 2.0, "4"):
        with pytest.raises(ValueError, match="sequence_constrain_beams=.*must be None, 0 or a width in 1..8"):
            sequence_constrain_beams_value(bad, 3)
    with pytest.raises(ValueError, match="sequence_constrain_beams=4 needs sequence_constrain"):
        sequence_constrain_beams_value(4, None)
    for kw in (dict(sequence_samples=2), dict(sequence_beams=2), dict(sequence_constrain_samples=2)):
        with pytest.raises(ValueError, match="sequence_constrain_beams excludes sequence_samples, sequence_beams and sequence_constrain_samples"):
            sequence_constrain_beams_value(4, 3, **kw)


# ---- CPU: every refusal -------------------------------------------------------------------------------------------------------------
def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes = {}
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    ft = torch.zeros(2, 8, 1, dtype=torch.int32)
    ok = dict(T=5, F=1, sequence_constrain="loops", tok_sep=SEP, follow_table=ft, sequence_constrain_beams=3)
    with pytest.raises(ValueError, match="sequence_constrain_beams is a single-sequence option .* constrain_beams"):
        eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
    with pytest.raises(ValueError, match="sequence_constrain_beams=3 needs sequence_constrain"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_constrain=None))
    for change in (dict(sequence_samples=2), dict(sequence_beams=2), dict(sequence_constrain_samples=2)):
        with pytest.raises(ValueError, match="sequence_constrain_beams excludes sequence_samples, sequence_beams and sequence_constrain_samples"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=2),
                   dict(constrain="no_repeat"), dict(constrain=0)):
        with pytest.raises(ValueError, match="sequence_constrain_beams excludes"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    with pytest.raises(ValueError, match="sequence_constrain_beams excludes stop_each_eos .* every beam"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, flags=engine.DEFAULT_FLAGS | lib.FF_STOP_EACH_EOS, **ok)
    for bad in (9, -1, True, 2.5):
        with pytest.raises(ValueError, match="sequence_constrain_beams="):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_constrain_beams=bad))
    with pytest.raises(ValueError, match="sequence_constrain_beams=6: must be in 1..8 and at most S = 5"):
        eng.decode(torch.zeros(2, 5, 64), None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_constrain_beams=6, follow_table=torch.zeros(2, 1, 1, dtype=torch.int32)))
    for bad in ("first", None, 1, "ALL"):
        with pytest.raises(ValueError, match="sequence_beam_stop=.*must be 'all' or 'best'"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_beam_stop=bad))
    with pytest.raises(ValueError, match="sequence_constrain needs tok_sep"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, tok_sep=None))
    with pytest.raises(ValueError, match="needs follow_table"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, follow_table=None))
    with pytest.raises(ValueError, match="follow_table must be an int32 tensor of shape \\[2, 8, 1\\]"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, follow_table=torch.zeros(2, 8, 2, dtype=torch.int32)))
    # the recorded refusals keep raising exactly what they raise, with the option unused
    plain = dict(T=5, F=1, sequence_constrain="loops", tok_sep=SEP, follow_table=ft)
    for change in (dict(sequence_samples=2), dict(sequence_beams=2)):
        with pytest.raises(ValueError, match="sequence_constrain excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, "
                                             "beam_width, num_samples, constrain, sequence_samples and sequence_beams"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(plain, **change))
    with pytest.raises(ValueError, match="constrain is a parallel-variant option"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, T=5, F=1, constrain="loops", term_range=(1, 4), follow_table=ft)


def test_models_reject_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    par = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert par.sequence_constrain_beams == 0
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    par.sequence_constrain_beams = 4
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_beams is a SurfaceFormer option .* constrain_beams"):
        par.forward_eval(inputs)
    assert "predict" not in inputs
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.sequence_constrain_beams == 0
    seq.sequence_constrain_beams = 4
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_beams=4 needs sequence_constrain"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain = "coedge_loops"
    text = "sequence_constrain excludes sequence_samples, sequence_beams, return_logprob and an extra mask"
    for attr, val, off in (("sequence_samples", 2, 0), ("sequence_beams", 2, 0), ("return_logprob", True, False)):
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match=text):       # the recorded refusal, unchanged, comes first
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, off)
    with torch.no_grad(), pytest.raises(ValueError, match=text):
        seq.forward_eval(_seq_inputs(extra_mask=torch.zeros(1, 8, dtype=torch.bool)))
    seq.stop_each_eos = True
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain excludes stop_each_eos = True"):
        seq.forward_eval(_seq_inputs())
    seq.stop_each_eos = False
    seq.sequence_constrain_samples = 2
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_beams excludes sequence_samples, sequence_beams and sequence_constrain_samples"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_samples = 0
    for bad in (9, True, -2, 1.5):
        seq.sequence_constrain_beams = bad
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_beams=.*must be None, 0 or a width in 1..8"):
            seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_beams, seq.sequence_beam_stop = 4, "first"
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_beam_stop='first': must be 'all' or 'best'"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_beam_stop = "all"
    seq.sequence_constrain_beams = 8
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_beams=8: must be in 1..8 and at most S = 4"):
        seq.forward_eval({"input": torch.zeros(1, 0, 50, 2), "input_mask": torch.zeros(1, 0, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})
    seq.sequence_constrain_beams = 4
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    seq.sequence_constrain = None
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain_beams"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_constrain, sub.sequence_constrain_beams = "loops", 4
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain needs the native engine"):
            sub.forward_eval(_seq_inputs())
    # what the model already refuses stays refused, with its recorded text, and comes first
    seq.sequence_constrain, seq.sequence_constrain_beams = "loops", 4
    for attr, val, off, word in (("constrain", "loops", None, "the single-sequence model emits loops of plain edges"),
                                 ("num_samples", 2, 0, "sampling for the single-sequence model is not implemented"),
                                 ("retire_finished", True, False, "the single-sequence model has one sequence per wireframe")):
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="%s is a SurfaceFormer_Parallel option \\(%s\\)" % (attr, word)):
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, off)
    # sequence_faces counts the option's beams among its rows per wireframe
    seq.sequence_faces, seq.sequence_faces_slots = "parse", 3
    big = faces.FACE_MAX_ROWS // 3 + 1
    if big <= 8:
        seq.sequence_constrain_beams = big
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_faces: %d rows x 3 slots per wireframe are above" % big):
            seq.forward_eval(_seq_inputs())
    seq.sequence_faces, seq.sequence_faces_slots, seq.sequence_constrain_beams = False, None, 4
    # an empty batch publishes the same keys, empty, and touches nothing
    with torch.no_grad():
        out = seq.forward_eval({"input": torch.zeros(0, 8, 50, 2), "input_mask": torch.zeros(0, 8, dtype=torch.bool),
                                "label": torch.zeros(0, 6, dtype=torch.long)})
    want = {"predict_beams": ((0, 4, 6), torch.int64), "predict_beam_scores": ((0, 4), torch.float32), "predict_beam_finished": ((0, 4), torch.int32),
            "predict_beam_dead_end": ((0, 4, 6), torch.int32), "predict_beam_open_end": ((0, 4), torch.int32),
            "predict_dead_end": ((0, 6), torch.int32), "predict_open_end": ((0,), torch.int32), "predict": ((0, 6), torch.int64)}
    for k, (shape, dtype) in want.items():
        assert tuple(out[k].shape) == shape and out[k].dtype == dtype, k
    assert "pointer" not in out and "predict_logprob" not in out and tuple(out["embedding"].shape) == (0, 8 + NTOK, 64)


def test_decode_sharded_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, sequence_constrain=None,
                                  sequence_constrain_beams=2)
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_constrain_beams"):
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_constrain = "loops"
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_constrain "):      # the recorded text comes first
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_constrain, model.sequence_constrain_beams = None, 0
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_model_and_every_refusal_raises(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain", "coedge_loops", "--sequence-constrain-beams", "4",
                                       "--sequence-beam-stop", "best"])
    assert (a.sequence_constrain, a.sequence_constrain_beams, a.sequence_beam_stop) == ("coedge_loops", 4, "best")
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).sequence_constrain_beams == 0
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-constrain", "loops", "--sequence-constrain-beams", "3", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["sequence_constrain"], kw["sequence_constrain_beams"], kw["sequence_beam_stop"]) for kw in seen] == [("loops", 3, "all"), (None, 0, "all")]
    m = cli.configure_model(types.SimpleNamespace(), sequence_beam_stop="best", sequence_constrain_beams=4)
    assert vars(m) == dict(sequence_constrain_beams=4, sequence_beam_stop="best")
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    seqcfg = types.SimpleNamespace(model_class="SurfaceFormer")
    call = dict(out_dir="unused", device="cpu", model=object())
    with pytest.raises(ValueError, match="--sequence-constrain-beams applies to SurfaceFormer only .*--constrain-beams"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer_Parallel"), None, sequence_constrain="loops", sequence_constrain_beams=2, **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beams requires --sequence-constrain"):
        run_test(seqcfg, None, sequence_constrain_beams=2, **call)
    for bad in (9, -1, True):
        with pytest.raises(ValueError, match="--sequence-constrain-beams must be a width in 1..8"):
            run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=bad, **call)
    with pytest.raises(ValueError, match="--sequence-beam-stop must be all or best"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, sequence_beam_stop="first", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beams does not combine with --sequence-constrain-samples"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, sequence_constrain_samples=2, **call)
    for kw in (dict(scores=True), dict(score_labels=True), dict(sample=2), dict(beam=2), dict(constrain="loops"), dict(sequence_samples=2),
               dict(sequence_beams=2), dict(device_faces=True), dict(sequence_device_faces=True)):
        with pytest.raises(ValueError, match="--sequence-constrain does not combine with --scores, --score-labels, --sample, --beam, --constrain, "
                                             "--sequence-samples, --sequence-beams, --device-faces or --sequence-device-faces"):
            run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, **dict(call, **kw))
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sequence-constrain-beams is not implemented for multi-rank runs"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, dist_mod=world2, **call)


def test_record_gains_the_two_keys_and_is_todays_without_them(tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd import datasets as D
    E = NTOK
    cfgm = types.SimpleNamespace(num_points_per_line=50, num_lines=16, point_dim=2, label_seq_length=24, token=TOK)
    cfg = types.SimpleNamespace(model=cfgm, post_process=types.SimpleNamespace(is_coedge=False, enclosedness_tol=1e-4))
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    edges = [[list(sq[i]), list(sq[(i + 1) % 4])] for i in range(4)] + [[[2.0, 2.0], [3.0, 2.0]], [[3.0, 2.0], [4.0, 4.0]]]
    raw = {"edges": edges, "faces_indices": [[[0, 1, 2, 3]]], "pairings": {}, "dominant_directions": [[1, 0, 0]]}
    (tmp_path / "json").mkdir()
    json.dump(raw, open(str(tmp_path / "json" / "a.json"), "w"))
    open(str(tmp_path / "t.txt"), "w").write("json/a.json\n")
    item = D.ABCDataset(str(tmp_path), ["t.txt"], cfgm)[0]
    beams = np.zeros((2, 24), dtype=np.int64)
    beams[0, :9] = [1, E + 0, E + 1, E + 2, E + 3, 2, E + 4, 2, 3]         # a closed square, then a face abandoned at a dead end
    beams[1, :5] = [1, E + 4, E + 5, 2, 3]
    dead = np.zeros((2, 24), dtype=np.int32)
    dead[0, 7] = 1
    pred = beams[0]
    text, st = cli.record_of(cfg, raw, item, pred, False)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
    text2, st2 = cli.record_of(cfg, raw, item, pred, False, sequence_constrained=dead[0],
                               sequence_constrained_beams=(beams, np.array([-1.0, -2.5], np.float32), np.array([1, 1]), dead))
    rec2 = json.loads(text2)
    assert list(rec2) == list(rec) + ["pred_dead_ends", "pred_unclosed", "pred_beam_faces", "pred_beam_face_scores"] and st2 == st
    assert {k: rec2[k] for k in rec} == rec and text == cli.record_of(cfg, raw, item, pred, False, sequence_constrained_beams=None)[0]
    assert rec2["pred_dead_ends"] == 1 and rec2["pred_beam_face_scores"] == [-1.0, -2.5] and len(rec2["pred_beam_faces"]) == 2


# ---- GPU: the operator --------------------------------------------------------------------------------------------------------------
def _beam_case(S, W, G, flags, scenario):
    """One operator case: test_sequence_constrain._operator_case's rows (states of one group mixed over the six kinds, rows pushed
    onto SEP, EOS and an edge that closes a loop, wireframes with different kv_len and a padding mask, a random_follows table) as
    G groups of W beams, one group per wireframe, plus the beams' scores (some empty)."""
    seed = CB.op_seed(S, W, G, flags, scenario)
    c = _operator_case(G * W, S, W, seed, {"mixed": "mixed", "mixed2": "mixed", "sep": "sep", "done": "done"}[scenario])
    c["scores"] = CB.beam_scores(c, S, W, G, seed, scenario)
    c["Wd"], c["G"] = W, G
    return c


def _states(c):
    none = lambda v: None if v < 0 else int(v)
    return [(frozenset(c["visited"][b]), none(c["first"][b]), none(c["prev"][b])) for b in range(c["B"])]


def _run_beam_op(c, flags, stop, counter=None, scores=None, want_stats=True):
    from faceformer_amd.hip import ops
    lg = torch.from_numpy(c["logits"]).clone().cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sc = c["scores"] if scores is None else scores
    res = ops.beam_sequence_constrained_select(
        lg, dev(sc.astype(np.float32)), dev(c["fin"]), dev(c["first"]), dev(c["prev"]), dev(_words(c["visited"], c["L"])), c["Wd"], flags, NTOK,
        SEP, EOS, follows=dev(faces.pack_follow_bits(c["table"])) if flags & SC.CONNECT else None, stop=stop, memory=dev(c["memory"]),
        mask=dev(c["mask"].astype(np.uint8)), kv_len=dev(c["kv"]), groups_per_wireframe=1, want_rows=True, want_stats=want_stats,
        counter=counter)
    return lg, res


def _want_of(c, flags, own=None):
    """The numpy rule per group, on the case's logits (own None) or on the kernel's own masked rows (the FILL pattern as padding)."""
    W, st = c["Wd"], _states(c)
    out = []
    for g in range(c["G"]):
        sl = slice(g * W, (g + 1) * W)
        table = c["table"][g] if flags & SC.CONNECT else None
        raw = c["logits"][sl].astype(np.float64)
        out.append(CB.group_step(raw, c["pad"][g], c["scores"][sl], c["fin"][sl] != 0, st[sl], flags, NTOK, SEP, EOS, table))
    return out


def _check_beam_op(c, flags, stop, seen):
    from faceformer_amd.hip import ops
    S, L, W, G, B = c["S"], c["L"], c["Wd"], c["G"], c["B"]
    what = (S, W, G, flags, stop)
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_beam_op(c, flags, stop, counter)
    own = lg.cpu().numpy()
    got = {k: res[k].cpu().numpy() for k in ("parent", "next", "scores", "fin", "dead_end", "open", "first", "prev", "visited", "mask_rows")}
    want = _want_of(c, flags)
    left = 0
    alls = bests = 0
    for g, wg in enumerate(want):
        for k in range(W):
            b = g * W + k
            if wg["masked"][k] is None:                                   # empty or finished: neither the byte row nor the logits are touched
                assert not got["mask_rows"][b].any() and np.array_equal(own[b], c["logits"][b]), (what, b)
                continue
            assert np.array_equal(got["mask_rows"][b] != 0, wg["masked"][k]), (what, b, c["kinds"][b])      # the byte row, exact
            assert np.array_equal(own[b] <= FILL, wg["masked"][k] | c["pad"][g]), (what, b)                  # the FILL pattern, exact
            live = own[b] > FILL
            assert np.array_equal(own[b][live], c["logits"][b][live]), (what, b)
        if not wg["gap"] > 1.0:
            left += 1
            continue
        sl = slice(g * W, (g + 1) * W)
        assert np.array_equal(got["parent"][sl], wg["parent"]) and np.array_equal(got["next"][sl], wg["tok"]), (what, g, got["parent"][sl], wg["parent"], got["next"][sl], wg["tok"])
        assert np.array_equal(got["fin"][sl] != 0, wg["fin"]) and np.array_equal(got["dead_end"][sl] != 0, wg["dead"]), (what, g)
        assert np.array_equal(got["open"][sl] != 0, wg["open"]), (what, g)
        fi, pv, vis = CB.pack_state(wg["states"], L)
        assert np.array_equal(got["first"][sl], fi) and np.array_equal(got["prev"][sl], pv), (what, g)
        if L:
            assert np.array_equal(got["visited"][sl], vis), (what, g)
        for r in range(W):
            sc, ws = float(got["scores"][g * W + r]), wg["scores"][r]
            if ws == NEG:
                assert sc == NEG, (what, g, r)
                continue
            assert abs(sc - ws) <= R.score_bound(ws), (what, g, r, sc, ws)
            p, tk = int(wg["parent"][r]), int(wg["tok"][r])
            if not c["fin"][g * W + p] and (own[g * W + p] > FILL).any():
                assert own[g * W + p][tk] > FILL, (what, g, r)            # no kept candidate is a masked key
            st0 = _states(c)[g * W + p]
            grew = not c["fin"][g * W + p]
            seen["dead"] += bool(wg["dead"][r])
            seen["closing"] += grew and st0[1] is not None and st0[2] is not None and tk >= NTOK and wg["states"][r][1] is None
            seen["cleared"] += grew and tk == SEP and len(st0[0]) > 0 and len(wg["states"][r][0]) == 0
            seen["kept"] += grew and tk == SEP and len(wg["states"][r][0]) > 0
            seen["eos"] += grew and tk == EOS
        live = np.isfinite(wg["scores"]) & ~wg["fin"]
        alls += int(live.sum())
        bests += int(live[0])
    assert left <= CB.CAP * G, (what, "indecisive groups", left)          # the cap: a condition the tool fixed on the CPU
    if left == 0:
        assert int(counter.item()) == (alls if stop == "all" else bests), (what, int(counter.item()), alls, bests)
    mem = torch.from_numpy(c["memory"]).cuda()
    assert torch.equal(res["rows"], ops.gather_rows(mem, res["next"], seqs_per_group=W)), what      # appended rows: ff_gather_rows' bits
    forced = ops.pointer_forced(torch.from_numpy(c["logits"]).clone().cuda(), res["next"], memory=mem, seqs_per_group=W, want_rows=True, want_stats=True)
    assert torch.equal(res["stats"], forced["stats"]), what
    lg2, res2 = _run_beam_op(c, flags, stop)                               # two launches
    assert all(torch.equal(res[k].view(torch.int32) if res[k].dtype == torch.float32 else res[k],
                           res2[k].view(torch.int32) if res2[k].dtype == torch.float32 else res2[k]) for k in res) and torch.equal(lg, lg2), what
    return got, own


def _check_width_one_is_the_greedy_step(c, flags, stop):
    """W = 1, score zero: every output bit-equal to ops.pointer_sequence_constrained's.  The zero is the one that leaves the sum's
    bits alone: -0.0, IEEE's additive identity (+0.0 + -0.0 is +0.0, and a row with one live key has log-probability -0.0), on the
    unfinished rows; a finished row hands its score on unchanged, and the greedy step reports +0.0 there."""
    from test_sequence_constrain import _run_operator
    counter, counter2 = torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_beam_op(c, flags, stop, counter, scores=np.where(c["fin"] != 0, 0.0, -0.0))
    lg2, ref = _run_operator(c, flags, counter2)
    assert torch.equal(lg, lg2) and int(counter.item()) == int(counter2.item())
    for mine, theirs in (("next", "next"), ("fin", "fin"), ("dead_end", "dead_end"), ("first", "first"), ("prev", "prev"), ("visited", "visited"),
                         ("mask_rows", "mask_rows"), ("rows", "rows"), ("stats", "stats")):
        assert torch.equal(res[mine], ref[theirs]), (c["S"], flags, stop, mine)
    assert torch.equal(res["scores"].view(torch.int32), ref["logprob"].view(torch.int32)), (c["S"], flags, stop)
    assert not bool(res["parent"].any())


def _check_bits_clear_is_the_sequence_beam_step(c, stop):
    """flags 0: every output bit-equal to ops.beam_sequence_select's, wherever the group has at least W live keys."""
    from faceformer_amd.hip import ops
    W = c["Wd"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ca, cb = torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_beam_op(c, 0, stop, ca)
    lg2 = torch.from_numpy(c["logits"]).clone().cuda()
    ref = ops.beam_sequence_select(lg2, dev(c["scores"].astype(np.float32)), dev(c["fin"]), W, groups_per_wireframe=1,
                                   mask=dev(c["mask"].astype(np.uint8)), kv_len=dev(c["kv"]), term_range=(EOS, EOS + 1), memory=dev(c["memory"]),
                                   want_rows=True, counter=cb, stop_best=stop == "best")
    assert torch.equal(lg, lg2) and not bool(res["mask_rows"].any()) and not bool(res["dead_end"].any())
    full = np.ones(c["G"], bool)
    for g in range(c["G"]):
        cands = 0
        for k in range(W):
            b = g * W + k
            if c["scores"][b] != NEG:
                cands += 1 if c["fin"][b] else int((~c["pad"][g]).sum())
        full[g] = cands >= W
    rows = torch.from_numpy(np.repeat(full, W)).cuda()
    for k in ("parent", "next", "fin", "rows"):
        assert torch.equal(res[k][rows], ref[k][rows]), (c["S"], W, stop, k)
    assert torch.equal(res["scores"][rows].view(torch.int32), ref["scores"][rows].view(torch.int32)), (c["S"], W, stop)
    if full.all():
        assert int(ca.item()) == int(cb.item())


@pytest.mark.gpu
@pytest.mark.parametrize("S,W", [(S, W) for S in CB.OP_S for W in CB.OP_W if W <= S])
def test_operator_against_the_numpy_rule(hip_lib, S, W):
    seen = dict(dead=0, closing=0, cleared=0, kept=0, eos=0)
    for G in CB.OP_G:
        for flags in CB.OP_FLAGS:
            for stop in CB.STOPS:
                for scenario in CB.OP_SCENARIOS:
                    c = _beam_case(S, W, G, flags, scenario)
                    _check_beam_op(c, flags, stop, seen)
                    if W == 1:
                        _check_width_one_is_the_greedy_step(c, flags, stop)
                    if flags == 0:
                        _check_bits_clear_is_the_sequence_beam_step(c, stop)
    print("S=%d W=%d:" % (S, W), seen)
    assert seen["eos"] and seen["cleared"] and seen["kept"]
    if S >= 65:
        assert seen["dead"] and seen["closing"], seen


def _raw_step(lib, c, flags=3, stop_best=0, over=None, guard=None):
    """ff_beam_sequence_constrained_select through ctypes with `over` replacing named members; every output holds a sentinel.  With
    a redzone Guard every operand and output lies in poisoned surroundings."""
    from faceformer_amd.hip import lib as L
    B, S, Ln, W = c["B"], c["S"], c["L"], c["Wd"]
    fw = (Ln + 31) // 32
    put = (lambda a: guard.embed(torch.from_numpy(np.ascontiguousarray(a)))) if guard else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    full = lambda shape, v, dt: put(np.full(shape, v, dtype=dt))
    keep = dict(logits=put(c["logits"]), scores=put(c["scores"].astype(np.float32)), fin=put(c["fin"]), first=put(c["first"]), prev=put(c["prev"]),
                visited=put(_words(c["visited"], Ln)), follows=put(faces.pack_follow_bits(c["table"])), mask=put(c["mask"].astype(np.uint8)),
                kv=put(c["kv"]), memory=put(c["memory"]))
    outs = dict(scores_out=full((B,), 7.5, np.float32), fin_out=full((B,), -7, np.int32), dead_out=full((B,), -7, np.int32),
                open_out=full((B,), -7, np.int32), first_out=full((B,), -7, np.int32), prev_out=full((B,), -7, np.int32),
                visited_out=full((B, fw), -7, np.int32), mask_rows=full((B, S), 77, np.uint8), parent=full((B,), -7, np.int32),
                next_tok=full((B,), -7, np.int32), next_rows=full((B, E_OP), 7.5, np.float32), count=full((1,), 5, np.int32))
    p = lambda t: None if t is None else t.data_ptr()
    a = dict(logits=p(keep["logits"]), ldlogits=S, S=S, mask=p(keep["mask"]), kv_len=p(keep["kv"]), groups=c["G"], width=W, groups_per_wireframe=1,
             follows=p(keep["follows"]), L=Ln, flags=flags, ntok=NTOK, tok_sep=SEP, tok_eos=EOS, stop_best=stop_best,
             scores_in=p(keep["scores"]), fin_in=p(keep["fin"]), first_in=p(keep["first"]), prev_in=p(keep["prev"]), visited_in=p(keep["visited"]),
             scores_out=p(outs["scores_out"]), fin_out=p(outs["fin_out"]), dead_out=p(outs["dead_out"]), open_out=p(outs["open_out"]),
             first_out=p(outs["first_out"]), prev_out=p(outs["prev_out"]), visited_out=p(outs["visited_out"]), mask_rows=p(outs["mask_rows"]),
             parent=p(outs["parent"]), next_tok=p(outs["next_tok"]), memory=p(keep["memory"]), E=E_OP, next_rows=p(outs["next_rows"]), ldnext=E_OP,
             next_stats=None, count_unfinished=p(outs["count"]))
    for k, v in (over or {}).items():
        a[k] = p(keep["visited"]) if v == "visited_in" else v
    d = L.BeamSequenceConstrainedStep(*a.values())
    rc = lib.ff_beam_sequence_constrained_select(L.C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, keep, outs


@pytest.mark.gpu
def test_operator_inside_poisoned_surroundings(hip_lib):
    import redzone as RZ
    c = _beam_case(65, 3, 5, 7, "mixed")
    got = {}
    for fill in (RZ.ZERO, RZ.POISON):
        g = RZ.Guard(fill)
        rc, keep, outs = _raw_step(hip_lib, c, flags=7, guard=g)
        assert rc == 0
        g.check()                                                         # nothing outside the operands and outputs is written
        got[fill] = {k: v.clone() for k, v in outs.items()}
    for k in got[RZ.ZERO]:
        if k != "mask_rows":                                              # (rows of empty / finished beams keep the sentinel in both)
            RZ.assert_same_bits(got[RZ.ZERO][k], got[RZ.POISON][k], k)    # nothing outside them is read
    want = _want_of(c, 7)
    tok = got[RZ.POISON]["next_tok"].cpu().numpy()
    assert all(np.array_equal(tok[g * 3:(g + 1) * 3], w["tok"]) for g, w in enumerate(want) if w["gap"] > 1.0)


@pytest.mark.gpu
def test_operator_err_arg_leaves_the_outputs_untouched(hip_lib):
    lib = hip_lib
    c = _beam_case(65, 3, 5, 3, "mixed")
    rc, keep, outs = _raw_step(lib, c)
    assert rc == 0 and int(outs["next_tok"].min()) >= 0 and int(outs["count"].item()) >= 5          # the arguments are good ones
    for over in (dict(flags=8), dict(flags=16 | 3), dict(flags=-1), dict(flags=4), dict(flags=6),           # unknown bits; ONCE without NO_REPEAT
                 dict(follows=None), dict(flags=7, follows=None), dict(tok_sep=NTOK), dict(tok_sep=-1), dict(tok_eos=NTOK), dict(tok_eos=-1),
                 dict(tok_sep=EOS), dict(tok_eos=SEP), dict(L=c["L"] - 1), dict(ntok=NTOK + 1), dict(groups_per_wireframe=0), dict(S=0),
                 dict(groups=0), dict(ldlogits=c["S"] - 1), dict(width=0), dict(width=9), dict(width=-1), dict(stop_best=2), dict(stop_best=-1),
                 dict(visited_out="visited_in"),                                                            # no beam may read a sibling's overwritten state
                 dict(mask_rows=None), dict(next_tok=None), dict(parent=None), dict(scores_out=None), dict(fin_out=None), dict(dead_out=None),
                 dict(open_out=None), dict(first_out=None), dict(prev_out=None), dict(visited_out=None), dict(scores_in=None), dict(fin_in=None),
                 dict(first_in=None), dict(prev_in=None), dict(visited_in=None), dict(logits=None), dict(memory=None), dict(ldnext=E_OP - 4)):
        rc, keep, outs = _raw_step(lib, c, over=over)
        assert rc == -1, (over, rc)                                                   # FF_ERR_ARG
        assert torch.equal(keep["logits"].cpu(), torch.from_numpy(c["logits"])), over
        assert torch.equal(keep["visited"].cpu(), torch.from_numpy(_words(c["visited"], c["L"]))), over
        assert bool((outs["mask_rows"] == 77).all()) and bool((outs["next_rows"] == 7.5).all()) and bool((outs["scores_out"] == 7.5).all()), over
        assert all(bool((outs[k] == -7).all()) for k in ("next_tok", "parent", "fin_out", "dead_out", "open_out", "first_out", "prev_out", "visited_out")), over
        assert int(outs["count"].item()) == 5, over
    small = _beam_case(5, 1, 1, 3, "mixed")                                           # W above S
    rc, keep, outs = _raw_step(lib, dict(small, Wd=6, G=1), over=dict(width=6))
    assert rc == -1 and b"width=6" in lib.ff_last_error()
    assert lib.ff_beam_sequence_constrained_select(None, None) == -1 and b"null descriptor" in lib.ff_last_error()


# ---- GPU: the engine ----------------------------------------------------------------------------------------------------------------
_RUNS = {}
KEYS = ("beams", "beam_scores", "beam_finished", "beam_dead_end", "beam_open_end", "predict", "dead_end", "open_end")


def _cb(model, case, b, flags, table, W, stop="all", **kw):
    return _decode(model, case, b, sequence_constrain=flags, tok_sep=SEP, follow_table=table if flags & SC.CONNECT else None,
                   sequence_constrain_beams=W, sequence_beam_stop=stop, return_pointer=False, **kw)


def _run(fix, flags, W, stop="all"):
    key = (fix, flags, W, stop)
    if key not in _RUNS:
        case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
        _RUNS[key] = _cb(model, case, b, flags, table, W, stop, trace=True)
    return _RUNS[key]


def _check_layout(out, T, W, stop, flags, follows):
    """The outputs' own consistency against the rule applied to the decode's own tokens: shapes and dtypes, SOS, the finished flags,
    the zero padding, best first, what `steps` may be, beam 0 under the greedy keys, open_end from the replayed state."""
    bm, sc, fin, de, oe = (out[k].cpu().numpy() for k in ("beams", "beam_scores", "beam_finished", "beam_dead_end", "beam_open_end"))
    steps = out["steps"]
    B = sc.size
    N = B // W
    assert bm.dtype == np.int64 and sc.dtype == np.float32 and fin.dtype == de.dtype == oe.dtype == np.int32
    assert bm.shape == de.shape == (B, T) and fin.shape == oe.shape == sc.shape
    assert (bm[:, 0] == SOS).all() and 1 <= steps <= T - 1 and len(out["step_counts"]) == steps
    live = np.isfinite(sc)
    assert not np.isnan(sc).any() and (sc[live] <= 0).all() and live.reshape(-1, W)[:, 0].all() and not (fin[~live] != 0).any()
    pos = QB.finish_of(bm, EOS)
    assert np.array_equal(fin[live] != 0, pos[live] <= steps)
    past = np.arange(T)[None, :] > np.minimum(pos, steps)[:, None]
    assert (bm[past] == 0).all() and (de[past] == 0).all() and (de[:, 0] == 0).all() and ((de == 0) | (de == 1)).all()
    gs = np.where(live, sc.astype(np.float64), -1e300).reshape(-1, W)
    assert (np.diff(gs, axis=1) <= 0).all()                                                    # best first
    unfinished = live & (fin == 0)
    first = unfinished.reshape(-1, W)[:, 0]
    assert steps == T - 1 or not (unfinished if stop == "all" else first).any()
    assert out["step_counts"][-1] == int((unfinished if stop == "all" else first).sum()) and all(v > 0 for v in out["step_counts"][:-1])
    assert torch.equal(out["predict"], out["beams"].view(N, W, T)[:, 0]) and torch.equal(out["dead_end"], out["beam_dead_end"].view(N, W, T)[:, 0])
    assert torch.equal(out["open_end"], out["beam_open_end"].view(N, W)[:, 0]) and "logprob" not in out
    rep = None if follows is None else [follows[r // W] for r in range(B)]
    states = SC.replay_states(bm, flags, NTOK, SEP, rep)
    last = np.minimum(pos, steps)
    for r in np.flatnonzero(live):
        assert oe[r] == int(states[r][last[r]][1] is not None), r
        assert (de[r, 1:][bm[r, 1:] != SEP] == 0).all(), r                                     # a dead end is a SEP
    return bm, sc.astype(np.float64), fin != 0, de, oe, pos, steps


@pytest.mark.gpu
@pytest.mark.parametrize("flags", CB.FLAGS)
@pytest.mark.parametrize("fix", CB.FIXTURES, ids=lambda f: "%s-%s%d" % f)
def test_engine_with_one_beam_is_the_constrained_greedy_decode(hip_lib, fix, flags):
    """Identity (a), both stop rules: tokens, dead_end, open_end and steps exact; |score - sum logprob| <= (T - 1) 2^-16."""
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T = case["model"]["seq_len"]
    greedy = _constrained(model, case, b, flags, table)
    want = greedy["logprob"].cpu().numpy().astype(np.float64).sum(axis=1)
    for stop in CB.STOPS:
        out = _cb(model, case, b, flags, table, 1, stop)
        assert out["steps"] == greedy["steps"] and out["step_counts"] == greedy["step_counts"], (fix, flags, stop)
        assert torch.equal(out["beams"], greedy["predict"]) and torch.equal(out["predict"], greedy["predict"]), (fix, flags, stop)
        assert torch.equal(out["beam_dead_end"], greedy["dead_end"]) and torch.equal(out["beam_open_end"], greedy["open_end"]), (fix, flags, stop)
        err = np.abs(out["beam_scores"].cpu().numpy().astype(np.float64) - want).max()
        print(fix, flags, stop, "steps=%d max |score - sum of greedy logprob| = %.3g" % (out["steps"], err))
        assert err <= (T - 1) * R.LP_BAR, (fix, flags, stop, err)
        _check_layout(out, T, 1, stop, flags, follows)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_with_all_bits_clear_is_the_sequence_beams_decode(hip_lib, name):
    """Identity (b) at W = 4, both stop rules: bit for bit; the byte rows are zero, so no dead end occurs."""
    case, z, model, b, sd, batch = _model(name)
    T, W = case["model"]["seq_len"], 4
    for stop in CB.STOPS:
        ref = _decode(model, case, b, sequence_beams=W, sequence_beam_stop=stop, return_pointer=False, trace=True)
        out = _cb(model, case, b, 0, None, W, stop, trace=True)
        assert out["steps"] == ref["steps"] and out["step_counts"] == ref["step_counts"], (name, stop)
        for k in ("beams", "beam_finished", "predict"):
            assert torch.equal(out[k], ref[k]), (name, stop, k)
        assert torch.equal(out["beam_scores"].view(torch.int32), ref["beam_scores"].view(torch.int32)), (name, stop)
        n = out["steps"]
        assert torch.equal(out["beam_parent"][:n], ref["beam_parent"][:n]) and not bool(out["beam_dead_end"].any())
        _check_layout(out, T, W, stop, 0, None)


def _replay(out, case, ni, W, flags, follows, stop, what):
    """The fp64 rule on the decode's own traced logits, step by step, from the rule's own carried state (section 13's scheme: j
    bounds at step j, a group leaves the comparison at its first indecisive step).  Holds, on the groups still compared, the
    constrained rows' FILL pattern, the parents, the dead flags, and -- returned -- the replayed beams / dead flags / scores /
    finished / open flags and counters.  -> (dict, still-compared mask per beam, left-out (step, group) pairs, pairs)."""
    T, S = case["model"]["seq_len"], case["model"]["L"] + NTOK
    steps = out["steps"]
    B = out["beams"].shape[0]
    G = B // W
    logits = out["logits"].cpu().numpy().astype(np.float64)
    par = out["beam_parent"].cpu().numpy()
    pads = np.stack([np.arange(S) >= NTOK + ni[w] for w in range(G)])
    scores, fin = QB.start(G, W)
    states = [START] * B
    opn = np.zeros(B, bool)
    ok = np.ones(G, dtype=bool)
    toks, deads, counts, left = [], [], [], 0
    for j in range(steps):
        lg = np.where(np.isnan(logits[j]), 0.0, logits[j])                  # (rows of empty / finished beams: not read by the rule)
        # the kernel's own masked rows: its FILL pattern must be the rule's, and the values of the live keys are what the rule reads
        res = CB.beam_step(lg, pads, scores, fin, states, W, flags, NTOK, SEP, EOS, follows, margin=j + 1)
        for r in range(B):
            if ok[r // W] and res["rows"][r] is not None:
                assert np.array_equal(logits[j, r] <= FILL, res["masked"][r] | pads[r // W]), (what, j, r)      # the constrained masked row, exact
        ok &= res["gap"] > 1.0
        left += int((~ok).sum())
        okb = np.repeat(ok, W)
        assert np.array_equal(par[j][okb], res["parent"][okb]), (what, j)
        toks.append(res["tok"]); deads.append(res["dead"].astype(np.int64)); counts.append(res[stop])
        scores, fin, states, opn = res["scores"], res["fin"], res["states"], res["open"]
    parents = [par[j] for j in range(steps)]
    beams, dead = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    beams[:, : steps + 1] = R.backtrack(np.full(B, SOS), toks, parents, W)
    dead[:, : steps + 1] = R.backtrack(np.zeros(B, dtype=np.int64), deads, parents, W)
    return dict(beams=beams, dead=dead, scores=scores, fin=fin, open=opn, counts=counts), np.repeat(ok, W), left, steps * G


def _check_replay(out, case, ni, W, flags, follows, stop, what):
    T = case["model"]["seq_len"]
    bm, sc, fin, de, oe, pos, steps = _check_layout(out, T, W, stop, flags, follows)
    rep, okb, left, pairs = _replay(out, case, ni, W, flags, follows, stop, what)
    print(what, "steps=%d left-out (step, group) pairs: %d of %d" % (steps, left, pairs))
    assert left <= CB.CAP * pairs, (what, left, pairs)
    assert np.array_equal(bm[okb], rep["beams"][okb]) and np.array_equal(de[okb], rep["dead"][okb]), what
    live = np.isfinite(rep["scores"])
    assert np.array_equal(fin[okb], (rep["fin"] & live)[okb]) and np.array_equal(oe[okb] != 0, (rep["open"] & live)[okb]), what
    if okb.all():                                                           # steps and the counters are batch-wide
        assert out["step_counts"] == rep["counts"] and CB.stop_step(rep["counts"], T) == steps, (what, out["step_counts"], rep["counts"])
    assert np.array_equal(np.isneginf(sc[okb]), np.isneginf(rep["scores"][okb])), what
    lv = okb & live
    err = np.abs(sc[lv] - rep["scores"][lv])
    bound = steps * (R.LP_BAR + R.ADD_EPS * np.abs(rep["scores"][lv]))
    print(what, "max |score - replayed score| = %.3g" % (err.max() if err.size else 0.0))
    assert (err <= bound).all(), (what, float(err.max()))
    return okb, left


REPLAY = [f + (flags, W) for f in CB.FIXTURES for flags in CB.FLAGS for W in CB.REPLAY_W]


@pytest.mark.gpu
@pytest.mark.parametrize("tup", REPLAY, ids=lambda t: "%s-%s%d-f%d-W%d" % t)
def test_engine_beams_replay_under_the_numpy_rule_and_keep_the_guarantee(hip_lib, tup):
    """The (golden, kind, seed, flags, W) tuples are the helper's: kept or dropped on the CPU by
    tools/sequence_constrain_beam_left_out.py engine; a dropped tuple still has to keep the guarantee."""
    fix, flags, W = tup[:3], tup[3], tup[4]
    assert tup in CB.KEPT or tup in CB.DROPPED, "not a conditioned tuple"
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    ni = batch["num_input"]
    out = _run(fix, flags, W)
    bm, sc, de, oe = (out[k].cpu().numpy() for k in ("beams", "beam_scores", "beam_dead_end", "beam_open_end"))
    enc, par, dead = CB.guarantee(bm, de, oe, sc, W, ni, flags, NTOK, SEP, EOS, follows, edges)      # (c), on every non-empty final beam
    print(tup, "steps=%d enclosed %d of %d parsed; dead ends %d; finished %d of %d non-empty" % (
        out["steps"], enc, par, dead, int((out["beam_finished"] != 0).sum()), int(np.isfinite(sc).sum())))
    if tup in CB.DROPPED:
        return
    okb, left = _check_replay(out, case, ni, W, flags, follows, "all", tup)
    kept = CB.KEPT[tup]
    if left == 0 and kept[0] == 0:                                          # nothing left out on either side: the oracle's own decisions
        assert (enc, par, dead, out["steps"]) == kept[2:], (tup, (enc, par, dead, out["steps"]), kept)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", CB.FLAGS)
@pytest.mark.parametrize("fix", [("seq_small_gain4", "lattice", 2), ("seq_small_eos", "lattice", 1), ("seq_small_repeat_eos", "random", 2),
                                 ("seq_small_gain4", "random", 1)], ids=lambda f: "%s-%s%d" % f)
def test_engine_best_stops_no_later_than_all_with_the_same_best_beam(hip_lib, fix, flags):
    """Identity (d) at W = 4 on one plan."""
    W = 4
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N = case["model"]["seq_len"], b["input"].size(0)
    al, be = _run(fix, flags, W, "all"), _run(fix, flags, W, "best")
    _check_layout(be, T, W, "best", flags, follows)
    assert be["steps"] <= al["steps"]
    if be["steps"] < T - 1:                                                  # every rank 0 finished: exact for the best beam
        assert torch.equal(al["beams"].view(N, W, T)[:, 0], be["beams"].view(N, W, T)[:, 0])
        assert torch.equal(al["beam_scores"].view(N, W)[:, 0].view(torch.int32), be["beam_scores"].view(N, W)[:, 0].view(torch.int32))
        assert (be["beam_finished"].view(N, W)[:, 0] != 0).all()
    # steps_best is the first step after which every group's rank 0 is finished in the "all" decode's own records:
    # replay its traced rows under the rule and read the "best" counter off every step
    rep, okb, left, pairs = _replay(al, case, batch["num_input"], W, flags, follows, "best", (fix, flags, "d"))
    if left == 0:
        assert be["steps"] == min(CB.stop_step(rep["counts"], T), T - 1), (fix, flags, be["steps"], rep["counts"])
    print(fix, flags, "W=%d steps all %d best %d" % (W, al["steps"], be["steps"]))


@pytest.mark.gpu
def test_engine_micro_batch_cut_repeatability_and_the_width_limit(hip_lib, monkeypatch):
    from faceformer_amd.hip import lib as L, modes
    fix, W = ("seq_small_gain4", "lattice", 1), 4
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, ni = case["model"]["seq_len"], batch["num_input"]
    whole = _run(fix, COEDGE, W)
    again = _cb(model, case, b, COEDGE, table, W, trace=True)
    assert whole["steps"] == again["steps"] and whole["step_counts"] == again["step_counts"]
    for k in KEYS + ("logits", "beam_parent"):                                        # one plan, two runs: bit-equal (the traces up to the stop)
        n = whole["steps"] if k in ("logits", "beam_parent") else None
        a, c = whole[k][:n], again[k][:n]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, c.view(torch.int32) if c.dtype == torch.float32 else c), k
    one = _cb(model, case, b, COEDGE, table, W, trace=True, chunk_max_seqs=W)         # one wireframe per micro-batch
    assert len({int(v) // W for v in one["seq_of_row"].cpu()}) == b["input"].size(0)
    ow, lw = _check_replay(whole, case, ni, W, COEDGE, follows, "all", "whole")
    oo, lo = _check_replay(one, case, ni, W, COEDGE, follows, "all", "one")
    both = ow & oo
    for k in ("beams", "beam_dead_end", "beam_finished", "beam_open_end"):
        assert np.array_equal(whole[k].cpu().numpy()[both], one[k].cpu().numpy()[both]), k      # equal on groups decisive in both
    if both.all():
        assert whole["steps"] == one["steps"] and whole["step_counts"] == one["step_counts"]
    # W = 8, the limit, decodes; W = 9 is refused by the C entry itself (the Python checks widened), before any launch
    fix8 = ("seq_small_eos", "lattice", 1)
    case8, model8, b8, batch8, follows8, table8, edges8, sd8 = _fixture(*fix8)
    wide = _cb(model8, case8, b8, COEDGE, table8, 8)
    bm, sc, fin, de, oe, pos, steps = _check_layout(wide, case8["model"]["seq_len"], 8, "all", COEDGE, follows8)
    CB.guarantee(bm, de, oe, sc, 8, batch8["num_input"], COEDGE, NTOK, SEP, EOS, follows8, edges8)
    monkeypatch.setattr(modes, "_sequence_constrain_beam_values", lambda o: None)
    monkeypatch.setattr(modes, "SEQUENCE_CONSTRAIN_BEAM", modes.SEQUENCE_CONSTRAIN_BEAM._replace(values=lambda o: None))
    monkeypatch.setattr(modes, "sequence_constrain_beams_value", lambda W, *a: int(W or 0))
    with pytest.raises(L.HipExtensionError, match="width=9 outside 1..8"):
        _cb(model8, case8, b8, COEDGE, table8, 9)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "seq_small_gain4"
    m = WP._bound(name, "default")
    batch, follows, _ = CB.fixture(m.case, m.batch, "random", 1)
    b = batch_to(batch, "cuda")
    table = torch.from_numpy(faces.pack_follow_bits(follows)).cuda()
    call = lambda: _cb(m.model, m.case, b, COEDGE, table, 4, trace=True)
    clean = call()
    zero, d = WP._run([m], call, fill=RZ.ZERO, what="sequence constrain beam after ZERO")
    poison, _ = WP._run([m], call, fill=RZ.POISON, what="sequence constrain beam after POISON")
    n = clean["steps"]
    for o in (clean, zero, poison):                                       # (the traces behind the stop step hold what the host enqueued)
        o["logits"], o["beam_parent"] = o["logits"][:n], o["beam_parent"][:n]
    WP._assert_equal(poison, zero, "sequence constrain beam")
    WP._assert_equal(poison, clean, "sequence constrain beam against the clean run")
    assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size
    assert int(zero["beam_dead_end"].sum()) > 0                       # dead ends in it
    assert not torch.isnan(poison["beam_scores"]).any()


def _oracle_scores(case, sd, batch, bm, pos, steps, W, flags, follows, ni):
    """fp64 scores of the oracle teacher-forced along the final beams (oracle/refpath.py, forced=), renormalised over the
    constrained row: -> (want [N, W], bound [N, W])."""
    from oracle import refpath
    from test_parity_golden import _tol
    N, T = bm.shape[0] // W, bm.shape[1]
    S = case["model"]["L"] + NTOK
    sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
    b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}
    rows = bm.reshape(N, W, T)
    states = SC.replay_states(bm, flags, NTOK, SEP, [follows[r // W] for r in range(N * W)])
    want, bound = np.zeros((N, W)), np.zeros((N, W))
    for k in range(W):
        tr = {}
        refpath.seq2seq_forward_eval(sd64, dict(b64), num_head=case["model"]["H"], label_seq_length=T, token_sos=SOS, token_eos=EOS,
                                     trace=tr, forced=torch.from_numpy(np.ascontiguousarray(rows[:, k])), steps=steps)
        truth = torch.stack(tr["logits"]).cpu().numpy()                              # [steps, N, S]
        for w in range(N):
            r = w * W + k
            pad = np.arange(S) >= NTOK + ni[w]
            for j in range(1, min(int(pos[r]), steps) + 1):
                masked, _ = faces.sequence_rule_mask(states[r][j - 1], flags, S, NTOK, SEP, EOS, follows[w], pad)
                lgt = np.where(masked | pad, -np.inf, truth[j - 1, w])
                m = lgt.max()
                want[w, k] += (lgt[rows[w, k, j]] - m) - math.log(np.exp(lgt - m).sum())
                bound[w, k] += 2 * _tol(truth[j - 1]) + R.LP_BAR
    return want, bound


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [("seq_small_gain4", "lattice", 2), ("seq_small_eos", "lattice", 1), ("seq_small_repeat_eos", "random", 2)],
                         ids=lambda f: "%s-%s%d" % f)
def test_engine_scores_against_the_teacher_forced_oracle(hip_lib, fix):
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, W = case["model"]["seq_len"], 2
    out = _run(fix, COEDGE, W)
    bm, sc, fin, de, oe, pos, steps = _check_layout(out, T, W, "all", COEDGE, follows)
    want, bound = _oracle_scores(case, sd, batch, bm, pos, steps, W, COEDGE, follows, batch["num_input"])
    got = sc.reshape(-1, W)
    live = np.isfinite(got)
    print(fix, "worst |score - oracle| / bound = %.3f" % (np.abs(got - want)[live] / np.maximum(bound[live], 1e-300)).max())
    assert (np.abs(got - want)[live] <= bound[live]).all(), (fix, got, want, bound)


# ---- GPU: the model and the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_publishes_the_keys_and_sequence_faces_works_behind_it(hip_lib):
    fix, W = ("seq_small_gain4", "lattice", 2), 3
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N = case["model"]["seq_len"], b["input"].size(0)
    gb = _model(fix[0])[3]
    try:
        with torch.no_grad():
            off = model(dict(gb))
            model.sequence_constrain = "coedge_loops"
            greedy = model(dict(b))
            model.sequence_constrain_beams = W
            on = model(dict(b))                                       # the table is built from the end points with constrain_tol
            given = model(dict(b, follow_table=table))
            model.sequence_beam_stop = "best"
            best = model(dict(b))
            model.sequence_beam_stop = "all"
            model.sequence_faces = "enclosed"
            both = model(dict(b))
    finally:
        model.sequence_constrain, model.sequence_constrain_beams, model.sequence_faces, model.sequence_beam_stop = None, 0, False, "all"
    assert np.array_equal(off["predict"].cpu().numpy(), _model(fix[0])[1]["predict"])      # off: today's decode, today's keys
    assert set(greedy) == (set(off) - {"pointer"}) | {"predict_logprob", "predict_dead_end", "predict_open_end"}      # the option unused: section 32's keys
    new = {"predict_beams", "predict_beam_scores", "predict_beam_finished", "predict_beam_dead_end", "predict_beam_open_end", "predict_dead_end",
           "predict_open_end"}
    assert set(on) == (set(off) - {"pointer"}) | new and not new & set(off) and set(best) == set(on)
    shapes = {"predict": ((N, T), torch.int64), "predict_beams": ((N, W, T), torch.int64), "predict_beam_scores": ((N, W), torch.float32),
              "predict_beam_finished": ((N, W), torch.int32), "predict_beam_open_end": ((N, W), torch.int32),
              "predict_beam_dead_end": ((N, W, T), torch.int32), "predict_dead_end": ((N, T), torch.int32), "predict_open_end": ((N,), torch.int32)}
    for k, (shape, dtype) in shapes.items():
        assert tuple(on[k].shape) == shape and on[k].dtype == dtype, k
    assert torch.equal(on["predict"], on["predict_beams"][:, 0]) and torch.equal(on["predict_dead_end"], on["predict_beam_dead_end"][:, 0])
    assert torch.equal(on["predict_open_end"], on["predict_beam_open_end"][:, 0]) and torch.equal(on["embedding"], greedy["embedding"])
    assert torch.equal(best["predict"], best["predict_beams"][:, 0])
    for k in new | {"predict"}:
        assert torch.equal(on[k], given[k]) and torch.equal(on[k], both[k]), k
    direct = _cb(model, case, b, COEDGE, table, W)
    for k in KEYS:
        assert torch.equal(direct[k].reshape(-1), on["predict" if k == "predict" else "predict_" + k].reshape(-1)), k
    assert model.last_constrain_stats["steps"] > 0 and model.last_constrain_stats["slot_rows"] > 0
    # sequence_faces = "enclosed" behind the option: faces.face_seq_rows / face_seq_votes on the published tensors, count [N, W]
    ni = np.asarray(batch["num_input"], dtype=np.int32)
    want = faces.face_seq_rows(both["predict_beams"].cpu().numpy(), ni, TOK, scores=both["predict_beam_scores"].cpu().numpy(),
                               finished=both["predict_beam_finished"].cpu().numpy(), follows=faces.pack_follow_bits(follows), closed_only=True)
    want.update(faces.face_seq_votes(want, require_closed=True))
    found = both["sequence_faces"]
    assert tuple(found["count"].shape) == (N, W)
    for k in want:
        a, w = found[k].cpu().numpy(), np.asarray(want[k])
        assert np.array_equal(a.reshape(w.shape).view(w.dtype) if a.dtype.itemsize == w.dtype.itemsize else a.reshape(w.shape), w), k
    assert int(found["num_faces"].sum()) > 0


@pytest.mark.gpu
def test_cli_records_with_and_without_the_flag(hip_lib, tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    root = tmp_path / "data"
    (root / "json").mkdir(parents=True)
    names = []
    for i in range(2):
        polys, _ = CR.lattice_edges(8 + 4 * i, 40 + i)
        raw = {"edges": [[[float(x), float(y)] for x, y in p] if len(p) == 2 else [[float(p[0][0]), float(p[0][1])], [float(p[-1][0]), float(p[-1][1])]]
                         for p in polys],
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
    plain = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "plain"))
    plain2 = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "plain2"), sequence_constrain_beams=0)
    loops = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "loops"), sequence_constrain="coedge_loops")
    one = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "one"), sequence_constrain="coedge_loops", sequence_constrain_beams=1)
    wide = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "wide"), sequence_constrain="coedge_loops", sequence_constrain_beams=4,
                        sequence_beam_stop="best", batch_size=2)
    new = ["pred_dead_ends", "pred_unclosed", "pred_beam_faces", "pred_beam_face_scores"]
    for fn in sorted(os.listdir(plain)):
        text = open(os.path.join(plain, fn)).read()
        assert text == open(os.path.join(plain2, fn)).read()          # byte-identical without the flag
        rec = json.loads(text)
        assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
        rl, r1, rw = (json.load(open(os.path.join(d, fn))) for d in (loops, one, wide))
        assert list(rl) == list(rec) + new[:2] and list(r1) == list(rec) + new and list(rw) == list(rec) + new
        assert {k: r1[k] for k in rl} == rl                           # W = 1: beam 0 is the constrained greedy row
        assert len(set(r1["pred_beam_face_scores"])) <= 1
        assert rw["pred_beam_face_scores"] == sorted(rw["pred_beam_face_scores"], reverse=True)
        assert len(rw["pred_beam_faces"]) == len(rw["pred_beam_face_scores"])
        for face in rw["pred_faces"]:
            idx = face[1] if isinstance(face, (list, tuple)) and len(face) == 2 and isinstance(face[1], (list, tuple)) else face
            assert len(set(idx)) == len(idx)
