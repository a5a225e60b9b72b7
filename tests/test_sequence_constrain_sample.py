"""Opt-in sampling over the loop-constrained single-sequence decode (SurfaceFormer.sequence_constrain_samples): the
numpy step on hand-written rows, the decode loop, every refusal and the CLI on the CPU (library untouched); the selection step, the
engine's mode, the model and the CLI on the GPU, through the C ABI.  The step is tests/sequence_constrain_sample_ref.py's, which
composes faces.sequence_rule_mask / sequence_rule_advance with sample_ref.sample_row and restates neither.

Bars (the issue's, none measured): byte rows, FILL patterns, flags, states, visited words, appended rows and counters are exact; a
token must equal the rule's on every DECISIVE row or (step, unfinished draw) pair (sample_row's flag: the cut and the draw lie
outside sample_ref's guard band); a log-probability lies within 2^-16 + 2^-23 |lp| of fp64 on the kernel's own masked row; at most
2 % of an engine case's pairs may be left out -- a condition on the tuples, fixed on the CPU by
tools/sequence_constrain_sample_left_out.py; scores within sum 2 tol(step) + 2^-16 of the fp64 oracle forced along every draw."""
import json
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import sample_ref as SR
import sequence_constrain_ref as SC
import sequence_constrain_sample_ref as QC
from conftest import ROOT, batch_to, token_ns
from faceformer_amd import faces
from faceformer_amd.hip.modes import SEQUENCE_CONSTRAIN_SAMPLE, sequence_constrain_samples_value      # (without them nothing here can pass)
from test_sequence_constrain import (E_OP, _constrained, _decode, _fixture, _model, _operator_case, _seq_inputs, _table, _tiny_model,
                                     _untouchable, _words)

TOK = token_ns()
NTOK, SOS, SEP, EOS = TOK.len, TOK.SOS, TOK.SEP, TOK.EOS
FILL = QC.FILL
LOOPS, COEDGE = QC.LOOPS, QC.COEDGE_LOOPS
PARAMS = [(1.0, 0, 1.0), (0.8, 16, 0.9), (0.0, 0, 1.0)]


# ---- CPU: the numpy step on hand-written rows ---------------------------------------------------------------------------------------
def _both(raw, state, flags, follows, u, params=(1.0, 0, 1.0), pad=None, finished=False):
    """The helper's step and faces' own restatement on one row: they must agree on everything they share."""
    raw = np.asarray(raw, dtype=np.float64)
    pad = np.zeros(len(raw), bool) if pad is None else np.asarray(pad, bool)
    a = QC.step(raw, pad, state, flags, NTOK, SEP, EOS, follows, u, *params, finished=finished)
    b = faces.sequence_rule_sample_step(raw, pad, state, flags, NTOK, SEP, EOS, u, *params, follows=follows, finished=finished)
    assert (a["tok"], a["dead"], a["fin"], a["state"]) == (b["tok"], b["dead"], b["fin"], b["state"])
    assert np.array_equal(a["masked"], b["masked"]) and abs(a["logprob"] - b["logprob"]) < 1e-12
    return a


def test_step_on_hand_written_rows():
    L = 6
    S = NTOK + L
    t = _table(L, [(0, 1), (1, 2), (2, 0), (3, 3), (4, 5)])
    g = np.random.default_rng(7)
    raw = g.standard_normal(S)
    start = faces.sequence_rule_start()
    closed = (frozenset({0, 1, 2}), None, 2)                  # the loop closed, a face behind it
    us = np.linspace(0.0, 1.0, 41)
    # closed with a face behind it: the draw is among the live edges plus SEP plus EOS
    drawn = {_both(raw, closed, LOOPS, t, u)["tok"] for u in us}
    assert drawn <= {SEP, EOS, NTOK + 3, NTOK + 4, NTOK + 5} and len(drawn) > 2
    # straight after SOS or SEP, SEP is never drawn (nor PAD / SOS)
    for state in (start, (frozenset({0, 1, 2}), None, None)):
        drawn = {_both(raw, state, COEDGE, t, u)["tok"] for u in us}
        assert SEP not in drawn and 0 not in drawn and SOS not in drawn and EOS in drawn | {EOS}
    # at a dead end the draw is SEP whatever u is, and the next state is closed and empty
    dead_state = (frozenset({4, 5}), 4, 5)                    # open, prev = 5 has no follower
    for u in us:
        r = _both(raw, dead_state, LOOPS, t, u, params=(0.8, 2, 0.5))
        assert r["dead"] and r["tok"] == SEP and not r["fin"] and r["state"] == start and abs(r["logprob"]) < 1e-12
    # visited is cleared at SEP without ONCE and kept with it
    push_sep = np.where(np.arange(S) == SEP, 50.0, raw)
    assert _both(push_sep, closed, LOOPS, t, 0.5)["state"] == (frozenset(), None, None)
    assert _both(push_sep, closed, COEDGE, t, 0.5)["state"] == (frozenset({0, 1, 2}), None, None)
    # top-k = 1 gives the constrained argmax, whatever u is; temperature 0 likewise, and it is the greedy rule's step
    greedy = faces.sequence_rule_step(raw, np.zeros(S, bool), closed, LOOPS, NTOK, SEP, EOS, t)
    for u in us:
        assert _both(raw, closed, LOOPS, t, u, params=(1.0, 1, 1.0))["tok"] == greedy["tok"]
        z = _both(raw, closed, LOOPS, t, u, params=(0.0, 0, 1.0))
        assert (z["tok"], z["state"], z["dead"]) == (greedy["tok"], greedy["state"], greedy["dead"]) and abs(z["logprob"] - greedy["logprob"]) < 1e-12
    # an open loop draws the follower only; the log-probability is renormalised over the constrained row
    r = _both(raw, (frozenset({0}), 0, 0), LOOPS, t, 0.3)
    assert r["tok"] == NTOK + 1 and abs(r["logprob"]) < 1e-12 and r["state"] == (frozenset({0, 1}), 0, 1)
    r = _both(raw, closed, LOOPS, t, 0.9)
    live = raw[[SEP, EOS, NTOK + 3, NTOK + 4, NTOK + 5]]
    assert abs(r["logprob"] - ((raw[r["tok"]] - live.max()) - np.log(np.exp(live - live.max()).sum()))) < 1e-12
    # a finished draw appends 0 with log-probability 0 and keeps its state; all bits clear: sample_row on the padded row
    f = _both(raw, closed, LOOPS, t, 0.5, finished=True)
    assert (f["tok"], f["logprob"], f["fin"], f["state"]) == (0, 0.0, True, closed)
    for u in us:
        assert _both(raw, closed, 0, None, u)["tok"] == SR.sample_row(raw, u)["tok"]


def test_decode_loop_on_a_scripted_model():
    """Finish, stop, steps, the counter and the zero padding on a scripted logit source: two wireframes, R = 2."""
    L, T, R, N = 5, 12, 2, 2
    S = NTOK + L
    t = _table(L, [(0, 1), (1, 2), (2, 0), (3, 3), (4, 1)])
    follows = np.stack([t, t])
    scripts = [[NTOK + 0, NTOK + 1, NTOK + 2, EOS], [NTOK + 3, SEP, NTOK + 4, EOS, EOS, EOS],
               [NTOK + 3, EOS], [NTOK + 0, NTOK + 1, NTOK + 2, SEP, NTOK + 3, SEP, EOS]]

    def step_logits(paths, step):
        rows = np.zeros((N * R, S))
        for r, sc in enumerate(scripts):
            rows[r, sc[min(step, len(sc) - 1)]] = 60.0
        return rows
    u = np.full((T - 1, N * R), 0.5)
    out = QC.decode(step_logits, u, N, T, R, COEDGE, NTOK, SOS, SEP, EOS, follows)
    tok = out["tokens"]
    assert tok[0, :5].tolist() == [SOS, NTOK, NTOK + 1, NTOK + 2, EOS] and (tok[0, 5:] == 0).all()
    # draw 1: the self loop, SEP, edge 4 whose only follower 1 is free here (ONCE keeps {3}): edge 1, then 2, then 0 closes ... the
    # script pushes EOS, masked while the loop is open, so the followers are drawn until the loop closes on edge 4's successor chain
    assert tok[1, :4].tolist() == [SOS, NTOK + 3, SEP, NTOK + 4] and (tok[1] == EOS).sum() <= 1
    assert tok[2, :3].tolist() == [SOS, NTOK + 3, EOS] and (tok[2, 3:] == 0).all()
    assert tok[3, :8].tolist() == [SOS, NTOK, NTOK + 1, NTOK + 2, SEP, NTOK + 3, SEP, EOS] and (tok[3, 8:] == 0).all()
    fin, steps = QC.stop_and_finish(tok, EOS)
    assert out["steps"] == steps and out["step_counts"] == QC.unfinished_after(tok, EOS)[:steps].tolist()
    assert fin[0] == 4 and fin[2] == 2 and fin[3] == 7 and steps == max(min(int(f), T - 1) for f in fin)
    past = np.arange(T)[None, :] > np.minimum(fin, steps)[:, None]
    assert (tok[past] == 0).all() and (out["logprob"][past] == 0).all() and (out["dead"][past] == 0).all()
    assert (out["logprob"][:, 0] == 0).all() and out["decisive"].all()
    states = QC.replay_states(tok, R, COEDGE, NTOK, SEP, follows)
    last = np.minimum(fin, steps)
    assert out["open_end"].tolist() == [int(states[r][last[r]][1] is not None) for r in range(N * R)]
    QC.guarantee(tok, out["dead"], out["open_end"], R, [L, L], COEDGE, NTOK, SEP, EOS, follows, None)


def test_faces_of_the_draws_leave_abandoned_faces_out():
    E = NTOK
    T = 14
    rows = np.zeros((3, T), dtype=np.int64)
    rows[0, :8] = [SOS, E + 0, E + 1, E + 2, SEP, E + 4, SEP, EOS]      # a face, then a face abandoned at a dead end
    rows[1, :6] = [SOS, E + 2, E + 1, E + 0, SEP, EOS]                  # the same edge set again
    rows[2, :5] = [SOS, E + 4, E + 5, SEP, EOS]
    lp = -np.ones((3, T)) * (rows != 0)
    lp[:, 0] = 0
    dead = np.zeros((3, T), dtype=np.int32)
    dead[0, 6] = 1
    got = faces.parse_faces_constrained_samples_scored(rows, lp, dead, 8, TOK)
    assert [(t, tuple(i)) for t, i, _ in got] == [(0, (0, 1, 2)), (0, (2, 1, 0)), (0, (4, 5))]
    assert [s for _, _, s in got] == [-4.0, -4.0, -3.0]
    votes = {k: v for _, k, _, v in faces.unique_faces_with_scores(got)}
    assert votes == {(0, 1, 2): 2, (4, 5): 1}
    same = faces.parse_faces_samples_scored(rows, lp, 8, TOK)             # without the flags the abandoned face counts
    assert len(same) == len(got) + 1
    with pytest.raises(ValueError, match="must all be \\[R, T\\]"):
        faces.parse_faces_constrained_samples_scored(rows, lp, dead[:2], 8, TOK)


# ---- CPU: C ABI, binding, sources ---------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_pointer_sequence_constrained_sample", "ff_decode_sequence_constrained_sample_workspace_bytes",
               "ff_decode_sequence_constrained_sample")


def test_header_binding_and_sources_declare_the_entries_within_abi_105():
    from faceformer_amd.hip import build, lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
        n_args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).count(",") + 1
        assert n_args == len(lib.SIGNATURES[name][1]), name
    # the step's argument list is DESIGN.md 32's operator plus DESIGN.md 29's draw arguments
    assert len(lib.SIGNATURES[NEW_ENTRIES[0]][1]) == len(lib.SIGNATURES["ff_pointer_sequence_constrained"][1]) + 6
    assert lib.SIGNATURES[NEW_ENTRIES[1]][1] == lib.SIGNATURES["ff_decode_sequence_sample_workspace_bytes"][1]
    assert len(lib.SIGNATURES[NEW_ENTRIES[2]][1]) == len(lib.SIGNATURES["ff_decode_sequence_sample"][1])
    fields = re.search(r"typedef struct ff_sequence_constrain_sample_params \{(.*?)\}", code, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == [n for n, _ in lib.SequenceConstrainSampleParams._fields_]
    doc = header[header.index("sampling over the loop-constrained single-sequence decode"):]
    assert "model.py:161-167" in doc and "model.py:193-210" in doc and "model.py:191" in doc      # the reference call sites
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain_seq.hip")).read()
    assert "ff_constrain_seq.hip" in build.SOURCES and "ff_sample_draw(" in src and "asm" not in src and "__syncthreads" not in src
    assert src.count("ff_loop_write_row<FF_LOOP_PLAIN>(") == 1 and src.count("xrow[a.eos] = 0") == 1      # one copy of the rule's launch code
    for name in ("ff_pointer_sequence_constrained", "ff_decode_sequence_constrained", "ff_pointer_sequence_sample", "ff_decode_sequence_sample"):
        assert name in lib.SIGNATURES                                     # the existing entries stay


def test_mode_record_lies_outside_both_tables():
    from faceformer_amd.hip import modes
    rec = SEQUENCE_CONSTRAIN_SAMPLE
    assert rec not in modes.MODES and rec not in modes.SEQUENCE_MODES and rec not in modes.SEQUENCE_MODEL_ORDER
    assert len(modes.SEQUENCE_MODES) == 3 and len(modes.MODES) == 4 and "sequence_constrain_samples" not in modes.SWITCH
    assert rec.entry == "ff_decode_sequence_constrained_sample" and rec.per_anchor and not rec.term_range and not rec.parallel_only
    assert rec.switches == modes.SEQUENCE_CONSTRAIN.switches             # the option that switches the mode on stays sequence_constrain
    assert [k for k, _, _ in rec.outs] == ["samples", "sample_logprob", "sample_scores", "sample_dead_end", "sample_open_end", "logprob",
                                          "dead_end", "open_end"]
    assert [sequence_constrain_samples_value(v, 3) for v in (None, 0, 1, 64)] == [0, 0, 1, 64]
    assert sequence_constrain_samples_value(None, None) == 0 and sequence_constrain_samples_value(0, None, 2, 2) == 0
    for bad in (65, -1, True, 2.0, "4"):
        with pytest.raises(ValueError, match="sequence_constrain_samples=.*must be None, 0 or a count in 1..64"):
            sequence_constrain_samples_value(bad, 3)
    with pytest.raises(ValueError, match="sequence_constrain_samples=4 needs sequence_constrain"):
        sequence_constrain_samples_value(4, None)
    for kw in (dict(sequence_samples=2), dict(sequence_beams=2)):
        with pytest.raises(ValueError, match="sequence_constrain_samples excludes sequence_samples and sequence_beams"):
            sequence_constrain_samples_value(4, 3, **kw)


# ---- CPU: every refusal -------------------------------------------------------------------------------------------------------------
def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes = {}
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    ft = torch.zeros(2, 8, 1, dtype=torch.int32)
    u = torch.zeros(4, 6)
    ok = dict(T=5, F=1, sequence_constrain="loops", tok_sep=SEP, follow_table=ft, sequence_constrain_samples=3, uniforms=u)
    with pytest.raises(ValueError, match="sequence_constrain_samples is a single-sequence option .* constrain_samples"):
        eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
    with pytest.raises(ValueError, match="sequence_constrain_samples=3 needs sequence_constrain"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_constrain=None))
    for change in (dict(sequence_samples=2), dict(sequence_beams=2)):
        with pytest.raises(ValueError, match="sequence_constrain_samples excludes sequence_samples and sequence_beams"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=2),
                   dict(constrain="no_repeat"), dict(constrain=0)):
        with pytest.raises(ValueError, match="sequence_constrain_samples excludes"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    with pytest.raises(ValueError, match="sequence_constrain_samples excludes stop_each_eos .* every draw"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, flags=engine.DEFAULT_FLAGS | lib.FF_STOP_EACH_EOS, **ok)
    for bad in (65, -1, True, 2.5):
        with pytest.raises(ValueError, match="sequence_constrain_samples="):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_constrain_samples=bad))
    for bad in (torch.zeros(4, 5), torch.zeros(3, 6), torch.zeros(4, 6, dtype=torch.float64), None, [[0.0] * 6] * 4):
        with pytest.raises(ValueError, match="uniforms must be a float32 tensor of shape \\[4, 6\\]"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, uniforms=bad))
    text = "sampling needs a finite temperature >= 0, top_k >= 0 and top_p in \\(0, 1\\]"      # DESIGN.md 15's text
    for change in (dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_k=-1), dict(top_p=0.0),
                   dict(top_p=1.5)):
        with pytest.raises(ValueError, match=text):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
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
    assert par.sequence_constrain_samples == 0
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    par.sequence_constrain_samples = 4
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_samples is a SurfaceFormer option .* constrain_samples"):
        par.forward_eval(inputs)
    par.sequence_constrain = "loops"
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain is a SurfaceFormer option .* constrain"):
        par.forward_eval(inputs)
    assert "predict" not in inputs
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.sequence_constrain_samples == 0
    seq.sequence_constrain_samples = 4
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_samples=4 needs sequence_constrain"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain = "coedge_loops"
    text = "sequence_constrain excludes sequence_samples, sequence_beams, return_logprob and an extra mask"
    seq.sequence_samples = 2
    with torch.no_grad(), pytest.raises(ValueError, match=text):       # the recorded refusal, unchanged, comes first
        seq.forward_eval(_seq_inputs())
    seq.sequence_samples = 0
    seq.return_logprob = True
    with torch.no_grad(), pytest.raises(ValueError, match=text):
        seq.forward_eval(_seq_inputs())
    seq.return_logprob = False
    with torch.no_grad(), pytest.raises(ValueError, match=text):
        seq.forward_eval(_seq_inputs(extra_mask=torch.zeros(1, 8, dtype=torch.bool)))
    seq.stop_each_eos = True
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain excludes stop_each_eos = True"):
        seq.forward_eval(_seq_inputs())
    seq.stop_each_eos = False
    for bad in (65, True, -2, 1.5):
        seq.sequence_constrain_samples = bad
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_samples=.*must be None, 0 or a count in 1..64"):
            seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_samples = 4
    for attr, val, off in (("sample_temperature", -1.0, 1.0), ("sample_top_k", -1, 0), ("sample_top_p", 0.0, 1.0)):
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="sampling needs a finite temperature >= 0, top_k >= 0 and top_p in"):
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, off)
    with torch.no_grad(), pytest.raises(ValueError, match="sample_uniforms must have shape \\[5, 4\\]"):
        seq.forward_eval(_seq_inputs(sample_uniforms=torch.zeros(5, 3)))
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    seq.sequence_constrain = None
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain_samples"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_constrain, sub.sequence_constrain_samples = "loops", 4
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain needs the native engine"):
            sub.forward_eval(_seq_inputs())
    # what the model already refuses stays refused, with its recorded text, and comes first
    seq.sequence_constrain, seq.sequence_constrain_samples = "loops", 4
    for attr, val, off, word in (("constrain", "loops", None, "the single-sequence model emits loops of plain edges"),
                                 ("num_samples", 2, 0, "sampling for the single-sequence model is not implemented"),
                                 ("retire_finished", True, False, "the single-sequence model has one sequence per wireframe")):
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="%s is a SurfaceFormer_Parallel option \\(%s\\)" % (attr, word)):
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, off)
    # sequence_faces counts the option's draws among its rows per wireframe
    seq.sequence_faces, seq.sequence_faces_slots, seq.sequence_constrain_samples = "parse", 3, 64
    big = faces.FACE_MAX_ROWS // 3 + 1
    if big <= 64:
        seq.sequence_constrain_samples = big
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_faces: %d rows x 3 slots per wireframe are above" % big):
            seq.forward_eval(_seq_inputs())
    seq.sequence_faces, seq.sequence_faces_slots, seq.sequence_constrain_samples = False, None, 4
    # an empty batch publishes the same keys, empty, and touches nothing
    with torch.no_grad():
        out = seq.forward_eval({"input": torch.zeros(0, 8, 50, 2), "input_mask": torch.zeros(0, 8, dtype=torch.bool),
                                "label": torch.zeros(0, 6, dtype=torch.long)})
    assert "pointer" not in out and tuple(out["predict"].shape) == (0, 6)
    for key, shape, dtype in (("predict_samples", (0, 4, 6), torch.int64), ("predict_sample_logprob", (0, 4, 6), torch.float32),
                              ("predict_sample_scores", (0, 4), torch.float32), ("predict_sample_dead_end", (0, 4, 6), torch.int32),
                              ("predict_sample_open_end", (0, 4), torch.int32), ("predict_logprob", (0, 6), torch.float32),
                              ("predict_dead_end", (0, 6), torch.int32), ("predict_open_end", (0,), torch.int32)):
        assert tuple(out[key].shape) == shape and out[key].dtype == dtype, key


def test_decode_sharded_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, sequence_constrain=None,
                                  sequence_constrain_samples=4)
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_constrain_samples"):
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_constrain = "loops"
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_constrain \\("):      # the recorded one comes first
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_constrain, model.sequence_constrain_samples = None, 0
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_model_and_every_refusal_raises(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain", "coedge_loops", "--sequence-constrain-samples", "8",
                                       "--temperature", "0.8", "--top-k", "16", "--top-p", "0.9", "--seed", "3"])
    assert (a.sequence_constrain, a.sequence_constrain_samples, a.temperature, a.top_k, a.top_p, a.seed) == ("coedge_loops", 8, 0.8, 16, 0.9, 3)
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).sequence_constrain_samples == 0
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-constrain", "loops", "--sequence-constrain-samples", "4", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["sequence_constrain"], kw["sequence_constrain_samples"]) for kw in seen] == [("loops", 4), (None, 0)]
    m = cli.configure_model(types.SimpleNamespace(), temperature=0.8, top_k=16, top_p=0.9, seed=3, sequence_constrain_samples=8)
    assert vars(m) == dict(sequence_constrain_samples=8, sample_temperature=0.8, sample_top_k=16, sample_top_p=0.9, sample_seed=3)
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    seqcfg = types.SimpleNamespace(model_class="SurfaceFormer")
    call = dict(out_dir="unused", device="cpu", model=object())
    with pytest.raises(ValueError, match="--sequence-constrain-samples requires --sequence-constrain"):
        run_test(seqcfg, None, sequence_constrain_samples=4, **call)
    with pytest.raises(ValueError, match="--sequence-constrain-samples applies to SurfaceFormer only .*--constrain-samples"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer_Parallel"), None, sequence_constrain="loops", sequence_constrain_samples=4, **call)
    for bad in (65, -1, True):
        with pytest.raises(ValueError, match="--sequence-constrain-samples must be a count in 1..64"):
            run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_samples=bad, **call)
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sequence-constrain-samples is not implemented for multi-rank runs"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_samples=4, dist_mod=world2, **call)
    # everything --sequence-constrain refuses today, with its text unchanged
    for kw in (dict(scores=True), dict(score_labels=True), dict(sample=2), dict(beam=2), dict(constrain="loops"), dict(sequence_samples=2),
               dict(sequence_beams=2), dict(device_faces=True), dict(sequence_device_faces=True)):
        with pytest.raises(ValueError, match="--sequence-constrain does not combine with --scores, --score-labels, --sample, --beam, --constrain, "
                                             "--sequence-samples, --sequence-beams, --device-faces or --sequence-device-faces"):
            run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_samples=4, **dict(call, **kw))
        with pytest.raises(ValueError, match="--sequence-constrain does not combine with"):
            run_test(seqcfg, None, sequence_constrain="loops", **dict(call, **kw))


def test_record_gains_the_keys_and_is_byte_identical_without_them(tmp_path):
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
    toks = np.zeros((3, 24), dtype=np.int64)
    toks[0, :9] = [1, E + 0, E + 1, E + 2, E + 3, 2, E + 4, 2, 3]            # a closed square, a face abandoned at a dead end
    toks[1, :7] = [1, E + 1, E + 2, E + 3, E + 0, 2, 3]                      # the square again, from another edge
    toks[2, :5] = [1, E + 4, E + 5, 2, 3]                                    # an open chain that was not flagged
    lps = -0.5 * (toks != 0)
    lps[:, 0] = 0
    dead = np.zeros((3, 24), dtype=np.int32)
    dead[0, 7] = 1
    text, st = cli.record_of(cfg, raw, item, toks[0], False)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
    assert text == cli.record_of(cfg, raw, item, toks[0], False, sequence_constrained=None, sequence_constrained_samples=None)[0]
    text2, st2 = cli.record_of(cfg, raw, item, toks[0], False, sequence_constrained=dead[0], sequence_constrained_samples=(toks, lps, dead))
    rec2 = json.loads(text2)
    new = ["pred_sample_faces", "pred_sample_face_scores", "pred_sample_face_votes", "pred_dead_ends", "pred_unclosed"]
    assert sorted(rec2) == sorted(list(rec) + new) and st2 == st and {k: rec2[k] for k in rec} == rec      # pred_faces stays draw 0's
    assert rec2["pred_sample_face_votes"] == [1, 2] and rec2["pred_sample_face_scores"] == [-1.5, -2.5]      # ranked by best score
    assert [sorted(f[1]) for f in rec2["pred_sample_faces"]] == [[4, 5], [0, 1, 2, 3]]
    assert rec2["pred_dead_ends"] == 1 and rec2["pred_unclosed"] == 2           # over all draws: the abandoned face and the open chain


# ---- GPU: the operator --------------------------------------------------------------------------------------------------------------
def _run_op(c, flags, params, u, row_id=None, counter=None, e=None, logits=None, want_stats=False):
    from faceformer_amd.hip import ops
    e = e or (lambda t: t.cuda())
    dev = lambda a: e(torch.from_numpy(np.ascontiguousarray(a)))
    lg = torch.from_numpy(c["logits"]).clone().cuda() if logits is None else logits
    res = ops.pointer_sequence_constrained_sample(
        lg, e(u), dev(c["fin"]), dev(c["first"]), dev(c["prev"]), dev(_words(c["visited"], c["L"])), flags, NTOK, SEP, EOS,
        follows=dev(faces.pack_follow_bits(c["table"])) if flags & QC.CONNECT else None, temperature=params[0], top_k=params[1],
        top_p=params[2], row_id=None if row_id is None else e(row_id), memory=dev(c["memory"]), mask=dev(c["mask"].astype(np.uint8)),
        kv_len=dev(c["kv"]), seqs_per_group=c["spg"], want_rows=True, want_stats=want_stats, counter=counter)
    return lg, res


def _uniforms_of(c, seed):
    """(uniforms [U], row_id or None, the uniform every row reads): rows read their own index, or -- every other case -- a
    reversed index into a longer array."""
    B = c["B"]
    if seed % 2:
        u = torch.rand(B, generator=torch.Generator().manual_seed(seed))
        return u, None, u.numpy()
    u = torch.rand(B + 3, generator=torch.Generator().manual_seed(seed))
    rid = torch.arange(B + 2, 2, -1, dtype=torch.int32)
    return u, rid, u.numpy()[rid.numpy()]


def _check_op(c, flags, params, seed, seen):
    from faceformer_amd.hip import ops
    B, S, L, spg = c["B"], c["S"], c["L"], c["spg"]
    u, rid, mine = _uniforms_of(c, seed)
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_op(c, flags, params, u, rid, counter)
    what = (S, B, spg, flags, params)
    own = lg.cpu().numpy()
    got = {k: res[k].cpu().numpy() for k in ("next", "logprob", "fin", "dead_end", "first", "prev", "visited", "mask_rows")}
    unfinished_after = 0
    for b in range(B):
        w = b // spg
        none = lambda v: None if v < 0 else int(v)
        fi, pv = none(c["first"][b]), none(c["prev"][b])
        state = (frozenset(c["visited"][b]), fi, pv)
        table = c["table"][w] if flags & QC.CONNECT else None
        was_fin = bool(c["fin"][b])
        want = QC.step(c["logits"][b], c["pad"][w], state, flags, NTOK, SEP, EOS, table, mine[b], *params, finished=was_fin)
        # the byte row and the FILL pattern of the masked row, exact
        assert np.array_equal(got["mask_rows"][b] != 0, want["masked"]), (what, b, c["kinds"][b])
        tok = int(got["next"][b])
        if was_fin:
            assert np.array_equal(own[b], c["logits"][b]) and tok == 0 and float(got["logprob"][b]) == 0.0, (what, b)
            assert got["fin"][b] == 1 and got["dead_end"][b] == 0, (what, b)
            assert (got["first"][b], got["prev"][b]) == (c["first"][b], c["prev"][b]) and np.array_equal(got["visited"][b], _words([state[0]], L)[0])
            continue
        assert np.array_equal(own[b] <= FILL, want["masked"] | c["pad"][w]), (what, b)
        live = own[b] > FILL
        assert np.array_equal(own[b][live], c["logits"][b][live]), (what, b)
        # the numpy rule on the kernel's own masked row: the token on every decisive row; the log-probability to the bar
        again = SR.sample_row(own[b].astype(np.float64), mine[b], *params)
        seen["rows"] += 1
        seen["decisive"] += again["decisive"]
        if again["decisive"]:
            assert tok == again["tok"] == want["tok"], (what, b, c["kinds"][b], tok, again["tok"], want["tok"])
        assert live[tok] or not live.any(), (what, b)                               # an indecisive row still draws a live key
        lp, ref = float(got["logprob"][b]), SR.logprob_of(own[b].astype(np.float64), tok)
        assert abs(lp - ref) <= QC.LP_BAR + QC.EPS * abs(ref), (what, b, lp, ref)
        # the dead flag, the finished flag, the next (first, prev) and the visited words: exact, along the kernel's own token
        assert bool(got["dead_end"][b]) == want["dead"] and bool(got["fin"][b]) == (tok == EOS), (what, b, c["kinds"][b])
        if want["dead"]:
            assert tok == SEP, (what, b)                                            # the only live key
        vis, nf, npv = faces.sequence_rule_advance(state, tok, flags, NTOK, SEP, table)
        assert (got["first"][b], got["prev"][b]) == (-1 if nf is None else nf, -1 if npv is None else npv), (what, b, c["kinds"][b])
        if L:
            assert np.array_equal(got["visited"][b], _words([vis], L)[0]), (what, b, c["kinds"][b])
        unfinished_after += tok != EOS
        seen["dead"] += want["dead"]
        seen["closing"] += fi is not None and pv is not None and tok >= NTOK and nf is None
        seen["cleared"] += tok == SEP and len(state[0]) > 0 and len(vis) == 0
        seen["kept"] += tok == SEP and len(vis) > 0
    assert int(counter.item()) == unfinished_after, (what, int(counter.item()), unfinished_after)
    mem = torch.from_numpy(c["memory"]).cuda()
    assert torch.equal(res["rows"], ops.gather_rows(mem, res["next"], seqs_per_group=spg)), what      # memory[b / spg, tok], bit-equal
    lg2, res2 = _run_op(c, flags, params, u, rid)                                    # two launches
    assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
    return lg, res, (u, rid)


def _identities(c, flags, params, lg, res, draw):
    """(a) temperature 0: ops.pointer_sequence_constrained; (b) all bits clear: ops.pointer_sequence_sample -- every output equal."""
    from faceformer_amd.hip import ops
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    common = dict(memory=dev(c["memory"]), mask=dev(c["mask"].astype(np.uint8)), kv_len=dev(c["kv"]), seqs_per_group=c["spg"], want_rows=True)
    if params[0] == 0.0:
        cnt = torch.zeros(1, dtype=torch.int32).cuda()
        lg2 = torch.from_numpy(c["logits"]).clone().cuda()
        ref = ops.pointer_sequence_constrained(lg2, dev(c["fin"]), dev(c["first"]), dev(c["prev"]), dev(_words(c["visited"], c["L"])), flags,
                                               NTOK, SEP, EOS, follows=dev(faces.pack_follow_bits(c["table"])) if flags & QC.CONNECT else None,
                                               counter=cnt, **common)
        assert torch.equal(lg, lg2) and set(ref) == set(res)
        for k in ref:
            assert torch.equal(ref[k].view(torch.int32) if ref[k].dtype == torch.float32 else ref[k],
                               res[k].view(torch.int32) if res[k].dtype == torch.float32 else res[k]), (k, flags)      # bit for bit
        return cnt
    if flags == 0:
        u, rid = draw
        lg2 = torch.from_numpy(c["logits"]).clone().cuda()
        ref = ops.pointer_sequence_sample(lg2, u.cuda(), params[0], params[1], params[2], row_id=None if rid is None else rid.cuda(),
                                          fin=dev(c["fin"]), term_range=(EOS, EOS + 1), **common)
        assert torch.equal(lg, lg2)
        for k in ("next", "logprob", "fin", "rows"):
            assert torch.equal(ref[k], res[k]), k
        assert not bool(res["mask_rows"].any()) and not bool(res["dead_end"].any())


@pytest.mark.gpu
@pytest.mark.parametrize("spg", [1, 4])
@pytest.mark.parametrize("S", [5, 65, 260, 1028])
def test_operator_against_the_numpy_rule_and_both_identities(hip_lib, S, spg):
    seen = dict(dead=0, closing=0, cleared=0, kept=0, rows=0, decisive=0)
    for B in (1, 5, 8):
        for flags in (0, 1, 3, 7):
            for i, params in enumerate(PARAMS):
                seed = 1 + i + 10 * flags
                c = _operator_case(B, S, spg, seed)
                lg, res, draw = _check_op(c, flags, params, seed, seen)
                cnt = _identities(c, flags, params, lg, res, draw)
                c = _operator_case(B, S, spg, 7, "sep")                               # every row closed, non-empty, pushed onto SEP
                _check_op(c, flags, params, 40 + i, seen)
            c = _operator_case(B, S, spg, 8, "done")                                  # every row pushed onto EOS or finished
            counter = torch.zeros(1, dtype=torch.int32).cuda()
            u = torch.rand(B, generator=torch.Generator().manual_seed(9))
            _, res = _run_op(c, flags, PARAMS[1], u, None, counter)
            assert int(counter.item()) == 0 and bool(res["fin"].all()), (S, B, spg, flags)
    print("S=%d spg=%d:" % (S, spg), seen)
    assert seen["cleared"] and seen["kept"] and seen["decisive"] >= 0.98 * seen["rows"]
    if S >= 65:
        assert seen["dead"] and seen["closing"], seen


@pytest.mark.gpu
def test_operator_frequencies_follow_the_fp64_probabilities_of_the_constrained_row(hip_lib):
    """One closed, non-empty row at S = 65 whose visited words leave 5 live edges, plus SEP and EOS; tau = 1, 65 536 rows."""
    from faceformer_amd.hip import ops
    S, B = 65, 65536
    L = S - NTOK
    row = torch.randn(S, generator=torch.Generator().manual_seed(21))
    live = [3, 8, 20, 32, 60]
    vis = np.ones((B, L), dtype=bool)
    vis[:, live] = False
    table = np.zeros((1, L, L), dtype=bool)
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32).cuda()
    u = torch.rand(B, generator=torch.Generator().manual_seed(22))
    res = ops.pointer_sequence_constrained_sample(row[None, :].repeat(B, 1).cuda(), u.cuda(), i32(0), i32(-1), i32(5),
                                                  torch.from_numpy(faces.pack_follow_bits(vis)).cuda(), LOOPS, NTOK, SEP, EOS,
                                                  follows=torch.from_numpy(faces.pack_follow_bits(table)).cuda(), seqs_per_group=B)
    keys = [SEP, EOS] + [NTOK + e for e in live]
    tok = res["next"].cpu().numpy()
    counts = np.bincount(tok, minlength=S).astype(np.float64)
    assert counts.sum() == B and counts[[s for s in range(S) if s not in keys]].sum() == 0          # zero draws on masked keys
    p = np.zeros(S)
    p[keys] = np.exp(row.numpy().astype(np.float64)[keys])
    p /= p.sum()
    sigma = np.sqrt(B * p[keys] * (1 - p[keys]))
    z = np.abs(counts[keys] - B * p[keys]) / sigma
    print("frequency check: worst |count - N p| / sigma = %.2f over %d live keys" % (z.max(), len(keys)))
    assert (z <= 5).all(), z.max()
    assert not bool(res["dead_end"].any()) and np.array_equal(res["fin"].cpu().numpy() != 0, tok == EOS)


@pytest.mark.gpu
def test_operator_inside_poisoned_surroundings(hip_lib):
    import redzone as RZ
    from test_redzone_ops import PAD, twice
    B, S, spg = 6, 70, 3
    c = _operator_case(B, S, spg, 4242)
    u = torch.rand(B, generator=torch.Generator().manual_seed(5))

    def call(lg, e):
        return dict(_run_op(c, COEDGE, (0.8, 16, 0.9), u, None, e(torch.zeros(1, dtype=torch.int32)), e=e, logits=lg, want_stats=True)[1], logits=lg)
    got = twice(lambda g: call(g.embed(torch.from_numpy(c["logits"]), ld=S + PAD, name="logits"), lambda t: g.embed(t.cpu())),
                "ff_pointer_sequence_constrained_sample")
    plain = call(torch.from_numpy(c["logits"]).clone().cuda(), lambda t: t.cuda())
    for k, v in plain.items():
        if torch.is_tensor(v):
            RZ.assert_same_bits(got[k], v, "ff_pointer_sequence_constrained_sample: %s against the clean call" % k)


def _raw_call(lib, c, over=None, flags=3):
    """ff_pointer_sequence_constrained_sample through ctypes with `over` replacing named arguments; every output holds a sentinel."""
    B, S, L = c["B"], c["S"], c["L"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lg = dev(c["logits"])
    keep = dict(fin=dev(c["fin"]), first=dev(c["first"]), prev=dev(c["prev"]), visited=dev(_words(c["visited"], L)),
                follows=dev(faces.pack_follow_bits(c["table"])), mask=dev(c["mask"].astype(np.uint8)), kv=dev(c["kv"]), memory=dev(c["memory"]),
                u=torch.rand(B, generator=torch.Generator().manual_seed(1)).cuda(), rid=torch.arange(B, dtype=torch.int32).cuda())
    outs = dict(mask_rows=torch.full((B, S), 77, dtype=torch.uint8).cuda(), next_tok=torch.full((B,), -7, dtype=torch.int32).cuda(),
                logprob=torch.full((B,), 7.5).cuda(), fin_out=torch.full((B,), -7, dtype=torch.int32).cuda(),
                dead_end=torch.full((B,), -7, dtype=torch.int32).cuda(), first_out=torch.full((B,), -7, dtype=torch.int32).cuda(),
                prev_out=torch.full((B,), -7, dtype=torch.int32).cuda(), next_rows=torch.full((B, E_OP), 7.5).cuda(),
                count=torch.full((1,), 5, dtype=torch.int32).cuda())
    a = dict(logits=lg.data_ptr(), ldlogits=S, S=S, mask=keep["mask"].data_ptr(), kv_len=keep["kv"].data_ptr(), B=B, spg=c["spg"],
             follows=keep["follows"].data_ptr(), L=L, flags=flags, ntok=NTOK, tok_sep=SEP, tok_eos=EOS, fin_in=keep["fin"].data_ptr(),
             first_in=keep["first"].data_ptr(), prev_in=keep["prev"].data_ptr(), visited=keep["visited"].data_ptr(),
             mask_rows=outs["mask_rows"].data_ptr(), next_tok=outs["next_tok"].data_ptr(), logprob=outs["logprob"].data_ptr(),
             fin_out=outs["fin_out"].data_ptr(), dead_end=outs["dead_end"].data_ptr(), first_out=outs["first_out"].data_ptr(),
             prev_out=outs["prev_out"].data_ptr(), memory=keep["memory"].data_ptr(), E=E_OP, next_rows=outs["next_rows"].data_ptr(),
             ldnext=E_OP, next_stats=None, count=outs["count"].data_ptr(), uniforms=keep["u"].data_ptr(), num_uniforms=B,
             row_id=keep["rid"].data_ptr(), temperature=1.0, top_k=0, top_p=1.0, stream=torch.cuda.current_stream().cuda_stream)
    a.update(over or {})
    rc = lib.ff_pointer_sequence_constrained_sample(*a.values())
    torch.cuda.synchronize()
    return rc, lg, keep, outs


@pytest.mark.gpu
def test_operator_err_arg_leaves_the_outputs_untouched(hip_lib):
    lib = hip_lib
    c = _operator_case(5, 65, 4, 3)
    rc, lg, keep, outs = _raw_call(lib, c)
    assert rc == 0 and int(outs["next_tok"].min()) >= 0 and int(outs["count"].item()) >= 5          # the arguments are good ones
    for over in (dict(flags=8), dict(flags=16 | 3), dict(flags=-1), dict(flags=4), dict(flags=6),           # what DESIGN.md 32's step refuses
                 dict(follows=None), dict(flags=2, follows=None), dict(flags=7, follows=None),
                 dict(tok_sep=NTOK), dict(tok_sep=-1), dict(tok_eos=NTOK), dict(tok_eos=-1), dict(tok_sep=EOS), dict(tok_eos=SEP),
                 dict(L=c["L"] - 1), dict(ntok=NTOK + 1), dict(spg=0), dict(S=0), dict(ldlogits=c["S"] - 1),
                 dict(mask_rows=None), dict(next_tok=None), dict(logprob=None), dict(fin_out=None), dict(dead_end=None),
                 dict(first_out=None), dict(prev_out=None), dict(fin_in=None), dict(first_in=None), dict(prev_in=None), dict(visited=None),
                 dict(logits=None), dict(memory=None), dict(ldnext=E_OP - 4),
                 dict(uniforms=None), dict(num_uniforms=0), dict(num_uniforms=4, row_id=None),             # ... and DESIGN.md 29's draw
                 dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_k=-1),
                 dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan"))):
        rc, lg, keep, outs = _raw_call(lib, c, over)
        assert rc == -1, (over, rc)                                                   # FF_ERR_ARG
        assert torch.equal(lg.cpu(), torch.from_numpy(c["logits"])), over
        assert torch.equal(keep["visited"].cpu(), torch.from_numpy(_words(c["visited"], c["L"]))), over
        assert bool((outs["mask_rows"] == 77).all()) and bool((outs["next_rows"] == 7.5).all()) and bool((outs["logprob"] == 7.5).all()), over
        assert all(bool((outs[k] == -7).all()) for k in ("next_tok", "fin_out", "dead_end", "first_out", "prev_out")), over
        assert int(outs["count"].item()) == 5, over


# ---- GPU: the engine ----------------------------------------------------------------------------------------------------------------
SMALL = ["seq_small_gain4", "seq_small_eos", "seq_small_repeat_eos"]
DRAW_KEYS = ("samples", "sample_logprob", "sample_scores", "sample_dead_end", "sample_open_end")
ALL_KEYS = DRAW_KEYS + ("predict", "logprob", "dead_end", "open_end")


def _cs(model, case, b, flags, table, R, params, u, **kw):
    return _decode(model, case, b, sequence_constrain=flags, tok_sep=SEP, follow_table=table if flags & QC.CONNECT else None,
                   sequence_constrain_samples=R, temperature=params[0], top_k=params[1], top_p=params[2], uniforms=u, return_pointer=False, **kw)


def _uniforms(case, b, R, seed):
    return QC.make_uniforms(b["input"].size(0), case["model"]["seq_len"], R, seed).cuda()


def _check_layout(out, T, R, flags, follows):
    """Shapes and dtypes, finish positions, the stop step, the per-step counts, open_end, the zero padding, the scores and draw 0
    against the rule applied to the decode's own tokens.  Returns (tokens, logprob, dead, finish positions, steps, states)."""
    smp, lp, sc, dead, oe = (out[k].cpu().numpy() for k in DRAW_KEYS)
    B = smp.shape[0]
    N = B // R
    assert smp.dtype == np.int64 and lp.dtype == np.float32 and sc.dtype == np.float32 and dead.dtype == np.int32 and oe.dtype == np.int32
    assert smp.shape == lp.shape == dead.shape == (N * R, T) and sc.shape == oe.shape == (N * R,)
    assert (smp[:, 0] == SOS).all()
    fin, steps = QC.stop_and_finish(smp, EOS)
    assert out["steps"] == steps, (out["steps"], steps)
    assert out["step_counts"] == QC.unfinished_after(smp, EOS)[:steps].tolist()
    last = np.minimum(fin, steps)
    past = np.arange(T)[None, :] > last[:, None]
    assert (smp[past] == 0).all() and (lp[past] == 0).all() and (dead[past] == 0).all() and (lp[:, 0] == 0).all() and (dead[:, 0] == 0).all()
    assert np.isfinite(lp).all() and (lp <= 0).all() and ((dead == 0) | (dead == 1)).all()
    want = lp.astype(np.float64).sum(axis=1)
    assert (np.abs(sc.astype(np.float64) - want) <= QC.EPS * np.abs(want)).all()
    states = QC.replay_states(smp, R, flags, NTOK, SEP, follows)
    assert oe.tolist() == [int(states[r][last[r]][1] is not None) for r in range(B)]
    assert torch.equal(out["predict"], out["samples"].view(N, R, T)[:, 0]) and torch.equal(out["logprob"], out["sample_logprob"].view(N, R, T)[:, 0])
    assert torch.equal(out["dead_end"], out["sample_dead_end"].view(N, R, T)[:, 0]) and torch.equal(out["open_end"], out["sample_open_end"].view(N, R)[:, 0])
    return smp, lp.astype(np.float64), dead, fin, steps, states


@pytest.mark.gpu
@pytest.mark.parametrize("flags", QC.FLAGS)
@pytest.mark.parametrize("fix", QC.FIXTURES, ids=lambda f: "%s-%s%d" % f)
def test_engine_with_temperature_zero_is_the_constrained_greedy_decode(hip_lib, fix, flags):
    """Identity (a): every draw equals the sequence_constrain decode with the same flags -- log-probabilities bit for bit."""
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N = case["model"]["seq_len"], b["input"].size(0)
    greedy = _constrained(model, case, b, flags, table)
    for R in (1, 3):
        out = _cs(model, case, b, flags, table, R, (0.0, 4, 0.5), _uniforms(case, b, R, 3))
        assert out["steps"] == greedy["steps"] and out["step_counts"] == [R * v for v in greedy["step_counts"]], (fix, flags, R)
        for k in range(R):
            assert torch.equal(out["samples"].view(N, R, T)[:, k], greedy["predict"]), (fix, flags, R, k)
            assert torch.equal(out["sample_logprob"].view(N, R, T)[:, k].view(torch.int32), greedy["logprob"].view(torch.int32)), (fix, flags, R, k)
            assert torch.equal(out["sample_dead_end"].view(N, R, T)[:, k], greedy["dead_end"]), (fix, flags, R, k)
            assert torch.equal(out["sample_open_end"].view(N, R)[:, k], greedy["open_end"]), (fix, flags, R, k)
        _check_layout(out, T, R, flags, follows)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_with_all_bits_clear_is_the_sequence_samples_decode(hip_lib, name):
    """Identity (b): the same uniforms and parameters; the byte rows are zero, so no dead end occurs."""
    case, z, model, b, sd, batch = _model(name)
    T, R = case["model"]["seq_len"], 4
    u = _uniforms(case, b, R, 5)
    for params in QC.REPLAY_PARAMS:
        ref = _decode(model, case, b, sequence_samples=R, temperature=params[0], top_k=params[1], top_p=params[2], uniforms=u, return_pointer=False)
        out = _cs(model, case, b, 0, None, R, params, u)
        assert out["steps"] == ref["steps"] and out["step_counts"] == ref["step_counts"], (name, params)
        for k in ("samples", "sample_logprob", "sample_scores", "predict"):
            assert torch.equal(out[k], ref[k]), (name, params, k)
        assert not bool(out["sample_dead_end"].any())
        _check_layout(out, T, R, 0, None)                                 # (open_end: without a table no loop closes, as the replayed state says)


def _replay(out, u, params, case, ni, R, flags, follows, what):
    """The numpy rule on the decode's own traced logits, pair by pair: the FILL pattern, the dead flag and the log-probability on
    every pair; the token on every decisive pair.  Returns (left-out pairs, pairs)."""
    T, S = case["model"]["seq_len"], case["model"]["L"] + NTOK
    smp, lp, dead, fin, steps, states = _check_layout(out, T, R, flags, follows)
    logits = out["logits"].cpu().numpy()
    un = u.cpu().numpy()
    pairs = left = 0
    for j in range(steps):
        for r in np.flatnonzero(fin > j):
            w = r // R
            row = logits[j, r].astype(np.float64)
            pad = np.arange(S) >= NTOK + ni[w]                                        # the padding the encoder's mask holds
            masked, is_dead = faces.sequence_rule_mask(states[r][j], flags, S, NTOK, SEP, EOS, None if follows is None else follows[w], pad)
            assert np.array_equal(row <= FILL, masked | pad), (what, j, int(r))        # the constrained masked row, exact
            assert bool(dead[r, j + 1]) == is_dead, (what, j, int(r))
            res = SR.sample_row(row, un[j, r], *params)
            pairs += 1
            tok = int(smp[r, j + 1])
            if res["decisive"]:
                assert tok == res["tok"], (what, j, int(r), tok, res["tok"])
            else:
                left += 1
                assert row[tok] > FILL, (what, j, int(r))                             # an indecisive pair still draws a live key
            if is_dead:
                assert tok == SEP, (what, j, int(r))
            own = SR.logprob_of(row, tok)
            assert abs(lp[r, j + 1] - own) <= QC.LP_BAR + QC.EPS * abs(own), (what, j, int(r))
    return left, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("params", QC.REPLAY_PARAMS)
@pytest.mark.parametrize("flags", QC.FLAGS)
@pytest.mark.parametrize("fix", QC.REPLAY_FIXTURES, ids=lambda f: "%s-%s%d" % f)
def test_engine_draws_replay_under_the_numpy_rule_and_keep_the_guarantee(hip_lib, fix, flags, params):
    """The (golden, kind, seed, flags, parameters) tuples are the helper's: kept on the CPU by tools/sequence_constrain_sample_left_out.py."""
    assert fix + (flags, tuple(params)) in QC.KEPT, "not a kept tuple"
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    ni, R = batch["num_input"], QC.REPLAY_R
    u = _uniforms(case, b, R, QC.REPLAY_SEEDS[fix[0]])
    out = _cs(model, case, b, flags, table, R, params, u, trace=True)
    left, pairs = _replay(out, u, params, case, ni, R, flags, follows, fix + (flags, params))
    smp, dead, oe = (out[k].cpu().numpy() for k in ("samples", "sample_dead_end", "sample_open_end"))
    enc, par = QC.guarantee(smp, dead, oe, R, ni, flags, NTOK, SEP, EOS, follows, edges)      # (c), on every draw
    print(fix, flags, params, "steps=%d left-out pairs: %d of %d; enclosed %d of %d; dead ends %d; draws at EOS %d of %d"
          % (out["steps"], left, pairs, enc, par, int(dead.sum()), int((smp == EOS).any(axis=1).sum()), smp.shape[0]))
    assert left <= QC.CAP * pairs, (fix, flags, params, left, pairs)
    if left == 0 and QC.KEPT[fix + (flags, tuple(params))][0] == 0:
        assert (enc, par, int(dead.sum())) == QC.KEPT[fix + (flags, tuple(params))][2:], (fix, flags, params)      # the oracle's own draws


def _oracle_scores(case, sd, batch, smp, fin, steps, R, flags, follows, ni):
    """fp64 scores of the oracle teacher-forced along every draw (oracle/refpath.py, forced=), renormalised over the constrained
    row: -> (want [N, R], bound [N, R])."""
    from oracle import refpath
    from test_parity_golden import _tol
    N, T = smp.shape[0] // R, smp.shape[1]
    S = case["model"]["L"] + NTOK
    sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
    b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}
    draws = smp.reshape(N, R, T)
    states = QC.replay_states(smp, R, flags, NTOK, SEP, follows)
    want, bound = np.zeros((N, R)), np.zeros((N, R))
    for k in range(R):
        tr = {}
        refpath.seq2seq_forward_eval(sd64, dict(b64), num_head=case["model"]["H"], label_seq_length=T, token_sos=SOS, token_eos=EOS,
                                     trace=tr, forced=torch.from_numpy(np.ascontiguousarray(draws[:, k])), steps=steps)
        truth = torch.stack(tr["logits"]).cpu().numpy()                              # [steps, N, S]
        for w in range(N):
            r = w * R + k
            pad = np.arange(S) >= NTOK + ni[w]
            for j in range(1, min(int(fin[r]), steps) + 1):
                masked, _ = faces.sequence_rule_mask(states[r][j - 1], flags, S, NTOK, SEP, EOS, follows[w], pad)
                lgt = np.where(masked | pad, -np.inf, truth[j - 1, w])
                m = lgt.max()
                want[w, k] += (lgt[draws[w, k, j]] - m) - math.log(np.exp(lgt - m).sum())
                bound[w, k] += 2 * _tol(truth[j - 1]) + QC.LP_BAR
    return want, bound


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [("seq_small_gain4", "lattice", 2), ("seq_small_eos", "lattice", 1), ("seq_small_repeat_eos", "random", 2)],
                         ids=lambda f: "%s-%s%d" % f)
def test_engine_scores_against_the_teacher_forced_oracle(hip_lib, fix):
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, R = case["model"]["seq_len"], 2
    out = _cs(model, case, b, COEDGE, table, R, (1.0, 0, 1.0), _uniforms(case, b, R, 5))
    smp, lp, dead, fin, steps, _ = _check_layout(out, T, R, COEDGE, follows)
    want, bound = _oracle_scores(case, sd, batch, smp, fin, steps, R, COEDGE, follows, batch["num_input"])
    got = out["sample_scores"].cpu().numpy().astype(np.float64).reshape(-1, R)
    print(fix, "worst |score - oracle| / bound = %.3f" % (np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    assert (np.abs(got - want) <= bound).all(), (fix, got, want, bound)


@pytest.mark.gpu
def test_engine_limit_micro_batch_cut_and_repeatability(hip_lib):
    # R = 64, the limit, on the one-wireframe golden
    fix = ("seq_small_eos", "lattice", 1)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T = case["model"]["seq_len"]
    u = _uniforms(case, b, 64, 5)
    out = _cs(model, case, b, COEDGE, table, 64, (1.0, 0, 1.0), u, trace=True)
    left, pairs = _replay(out, u, (1.0, 0, 1.0), case, batch["num_input"], 64, COEDGE, follows, "R = 64")
    assert left <= QC.CAP * pairs and sorted(int(v) for v in out["seq_of_row"].cpu()) == list(range(64))
    smp, dead, oe = (out[k].cpu().numpy() for k in ("samples", "sample_dead_end", "sample_open_end"))
    QC.guarantee(smp, dead, oe, 64, batch["num_input"], COEDGE, NTOK, SEP, EOS, follows, edges)
    # chunk_max_seqs = R (one wireframe per micro-batch) against the whole batch; two runs of one plan
    fix = ("seq_small_gain4", "lattice", 1)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    R, params = 4, (0.8, 16, 0.9)
    u = _uniforms(case, b, R, 5)
    whole = _cs(model, case, b, COEDGE, table, R, params, u, trace=True)
    again = _cs(model, case, b, COEDGE, table, R, params, u, trace=True)
    assert whole["steps"] == again["steps"] and whole["step_counts"] == again["step_counts"]
    for k in ALL_KEYS + ("logits",):                                                  # one plan, two runs: bit-equal (the trace up to the stop)
        n = whole["steps"] if k == "logits" else None
        assert torch.equal(whole[k][:n], again[k][:n]), k
    one = _cs(model, case, b, COEDGE, table, R, params, u, trace=True, chunk_max_seqs=R)
    assert sorted(int(v) for v in one["seq_of_row"].cpu()) == list(range(b["input"].size(0) * R))
    lw, pw = _replay(whole, u, params, case, batch["num_input"], R, COEDGE, follows, "whole")
    lo, po = _replay(one, u, params, case, batch["num_input"], R, COEDGE, follows, "one")
    assert lw <= QC.CAP * pw and lo <= QC.CAP * po
    if lw == 0 and lo == 0:                                                           # every pair decisive in both: the same decode
        for k in ("samples", "sample_dead_end", "sample_open_end", "predict", "dead_end", "open_end"):
            assert torch.equal(whole[k], one[k]), k
        assert whole["steps"] == one["steps"] and whole["step_counts"] == one["step_counts"]


@pytest.mark.gpu
def test_engine_entry_refuses_a_draw_count_outside_1_to_64(hip_lib, monkeypatch):
    """The C entry itself: with the Python checks widened, R = 65 comes back as FF_ERR_ARG (and the size query as 0) before any
    launch -- the outputs, which the wrapper allocates, are never published."""
    from faceformer_amd.hip import lib as L, modes
    fix = ("seq_small_eos", "lattice", 1)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    monkeypatch.setattr(modes, "SAMPLE_MAX", 65)
    with pytest.raises(L.HipExtensionError, match="num_samples=65 outside 1..64"):
        _cs(model, case, b, COEDGE, table, 65, (1.0, 0, 1.0), _uniforms(case, b, 65, 5))
    torch.cuda.synchronize()
    out = _cs(model, case, b, COEDGE, table, 64, (1.0, 0, 1.0), _uniforms(case, b, 64, 5))      # the limit itself decodes
    assert out["steps"] > 0


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "seq_small_gain4"
    m = WP._bound(name, "default")
    batch, follows, _ = QC.fixture(m.case, m.batch, "random", 1)
    b = batch_to(batch, "cuda")
    table = torch.from_numpy(faces.pack_follow_bits(follows)).cuda()
    u = _uniforms(m.case, b, 3, 5)
    call = lambda: _cs(m.model, m.case, b, COEDGE, table, 3, (1.0, 0, 1.0), u, trace=True)
    clean = call()
    zero, d = WP._run([m], call, fill=RZ.ZERO, what="sequence constrain sample after ZERO")
    poison, _ = WP._run([m], call, fill=RZ.POISON, what="sequence constrain sample after POISON")
    WP._assert_equal(poison, zero, "sequence constrain sample")
    WP._assert_equal(poison, clean, "sequence constrain sample against the clean run")
    WP._assert_no_nan(poison, "sequence constrain sample")
    assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size
    assert int(zero["sample_dead_end"].sum()) > 0


# ---- GPU: the model and the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_publishes_the_keys_and_sequence_faces_works_behind_it(hip_lib):
    fix = ("seq_small_gain4", "lattice", 2)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N, R = case["model"]["seq_len"], b["input"].size(0), 4
    gb = _model(fix[0])[3]
    saved = (model.sample_temperature, model.sample_top_k, model.sample_top_p, model.sample_seed)
    try:
        with torch.no_grad():
            off = model(dict(gb))
            model.sequence_constrain = "coedge_loops"
            greedy = model(dict(b))
            model.sequence_constrain_samples, model.sample_seed = R, 9
            on = model(dict(b))
            gen = torch.Generator(device="cuda").manual_seed(9)
            u = torch.rand((T - 1, N * R), generator=gen, device="cuda", dtype=torch.float32)
            given = model(dict(b, sample_uniforms=u, follow_table=table))
            model.sequence_faces = "enclosed"
            both = model(dict(b))
            model.sequence_faces = False
    finally:
        model.sequence_constrain, model.sequence_faces, model.sequence_constrain_samples = None, False, 0
        model.sample_temperature, model.sample_top_k, model.sample_top_p, model.sample_seed = saved
    assert np.array_equal(off["predict"].cpu().numpy(), _model(fix[0])[1]["predict"])      # off: today's decode, today's keys
    new = {"predict_samples", "predict_sample_logprob", "predict_sample_scores", "predict_sample_dead_end", "predict_sample_open_end"}
    assert set(on) == set(greedy) | new and not new & set(greedy) and "pointer" not in on
    for key, shape, dtype in (("predict_samples", (N, R, T), torch.int64), ("predict_sample_logprob", (N, R, T), torch.float32),
                              ("predict_sample_scores", (N, R), torch.float32), ("predict_sample_dead_end", (N, R, T), torch.int32),
                              ("predict_sample_open_end", (N, R), torch.int32), ("predict", (N, T), torch.int64),
                              ("predict_logprob", (N, T), torch.float32), ("predict_dead_end", (N, T), torch.int32),
                              ("predict_open_end", (N,), torch.int32)):
        assert tuple(on[key].shape) == shape and on[key].dtype == dtype, key
    assert torch.equal(on["predict"], on["predict_samples"][:, 0]) and torch.equal(on["predict_logprob"], on["predict_sample_logprob"][:, 0])
    assert torch.equal(on["predict_dead_end"], on["predict_sample_dead_end"][:, 0]) and torch.equal(on["predict_open_end"], on["predict_sample_open_end"][:, 0])
    for k in new | {"predict", "predict_logprob", "predict_dead_end", "predict_open_end", "embedding"}:
        assert torch.equal(on[k], given[k]) and torch.equal(on[k], both[k]), k             # the seeded default = its uniforms handed in
    assert model.last_constrain_stats["steps"] > 0 and model.last_constrain_stats["slot_rows"] > 0
    # sequence_faces = "enclosed" behind the option: faces.face_seq_rows / face_seq_votes on the published tensors, G = R rows
    ni = np.asarray(batch["num_input"], dtype=np.int32)
    want = faces.face_seq_rows(both["predict_samples"].cpu().numpy(), ni, TOK, logprob=both["predict_sample_logprob"].cpu().numpy(),
                               follows=faces.pack_follow_bits(follows), closed_only=True)
    want.update(faces.face_seq_votes(want, require_closed=True))
    found = both["sequence_faces"]
    for k in want:
        a, w = found[k].cpu().numpy(), np.asarray(want[k])
        assert np.array_equal(a.reshape(w.shape).view(w.dtype) if a.dtype.itemsize == w.dtype.itemsize else a.reshape(w.shape), w), k
    assert int(found["num_faces"].sum()) > 0 and tuple(found["count"].shape) == (N, R)


@pytest.mark.gpu
def test_cli_records_with_and_without_the_flag(hip_lib, tmp_path):
    sys.path.insert(0, ROOT)
    import constrain_ref as CR
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
    plain2 = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "plain2"), sequence_constrain=None, sequence_constrain_samples=0)
    loops = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "loops"), sequence_constrain="coedge_loops")
    loops2 = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "loops2"), sequence_constrain="coedge_loops", sequence_constrain_samples=0)
    drawn = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "drawn"), sequence_constrain="coedge_loops", sequence_constrain_samples=6,
                         temperature=0.8, top_k=16, top_p=0.9, seed=3)
    new = ["pred_sample_faces", "pred_sample_face_scores", "pred_sample_face_votes"]
    for fn in sorted(os.listdir(plain)):
        text = open(os.path.join(plain, fn)).read()
        assert text == open(os.path.join(plain2, fn)).read()          # byte-identical without the flags
        assert open(os.path.join(loops, fn)).read() == open(os.path.join(loops2, fn)).read()
        rec, rl, rd = json.loads(text), json.load(open(os.path.join(loops, fn))), json.load(open(os.path.join(drawn, fn)))
        assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
        assert sorted(rd) == sorted(list(rl) + new) and sorted(rl) == sorted(list(rec) + ["pred_dead_ends", "pred_unclosed"])
        assert len(rd["pred_sample_faces"]) == len(rd["pred_sample_face_scores"]) == len(rd["pred_sample_face_votes"])
        assert all(1 <= v <= 6 for v in rd["pred_sample_face_votes"]) and all(s <= 0 for s in rd["pred_sample_face_scores"])
        assert rd["pred_sample_face_scores"] == sorted(rd["pred_sample_face_scores"], reverse=True)
        assert isinstance(rd["pred_dead_ends"], int) and isinstance(rd["pred_unclosed"], int)
