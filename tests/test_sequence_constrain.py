"""Opt-in loop-constrained decode of the single-sequence model (SurfaceFormer.sequence_constrain): the numpy rule on
hand-written rows, every refusal and the CLI on the CPU (library untouched); the selection step, the engine's mode, the model and the
CLI on the GPU, through the C ABI.  The rule is faces.sequence_rule_step; the decode around it tests/sequence_constrain_ref.py.

Bars (the issue's, none measured): byte rows, tokens, flags, states and visited words are exact; a log-probability lies within
2^-16 + 2^-23 |lp| of fp64 on the kernel's own masked row; a token of an engine decode must equal the rule's on every (step,
unfinished row) pair whose margin between the two best live keys exceeds 2 tol(step) (tol: test_parity_golden._tol); at most 2 % of a
case's pairs may be left out -- a condition on the (golden, kind, seed, flags) triples, fixed on the CPU by
tools/sequence_constrain_left_out.py; traced logits within tol(step) of the fp64 oracle forced along the decode's own tokens."""
import ctypes as C
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
import sequence_constrain_ref as SC
from conftest import ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces
from faceformer_amd.hip.modes import SEQUENCE_CONSTRAIN, sequence_constrain_flags      # (the option: without it nothing here can pass)

TOK = token_ns()
NTOK, SOS, SEP, EOS = TOK.len, TOK.SOS, TOK.SEP, TOK.EOS
FILL = SC.FILL
LOOPS, COEDGE = SC.LOOPS, SC.COEDGE_LOOPS


# ---- CPU: the numpy rule on hand-written rows ---------------------------------------------------------------------------------------
def _table(L, pairs):
    t = np.zeros((L, L), dtype=bool)
    for a, b in pairs:
        t[a, b] = True
    return t


def _step(raw, state, flags, follows, pad=None, finished=False):
    raw = np.asarray(raw, dtype=np.float64)
    pad = np.zeros(len(raw), bool) if pad is None else np.asarray(pad, bool)
    return faces.sequence_rule_step(raw, pad, state, flags, NTOK, SEP, EOS, follows, finished)


def test_rule_on_hand_written_rows():
    L = 4
    S = NTOK + L
    t = _table(L, [(0, 1), (1, 2), (2, 0), (3, 3)])          # a triangle 0 -> 1 -> 2 -> 0 and a one-edge loop 3
    flat = np.zeros(S)
    start = faces.sequence_rule_start()
    assert start == (frozenset(), None, None)
    # SEP masked after SOS; EOS open whenever the loop is closed; PAD and SOS masked under CONNECT
    r = _step(flat, start, LOOPS, t)
    assert r["masked"][:NTOK].tolist() == [True, True, True, False] and not r["masked"][NTOK:].any() and not r["dead"]
    assert r["tok"] == EOS and r["fin"]                      # (a flat row: the lowest live index)
    # without CONNECT no special token is touched and no table is read
    r = _step(flat, start, SC.NO_REPEAT, None)
    assert not r["masked"].any() and r["tok"] == 0 and not r["fin"]
    # an edge opens the loop: every special token masked, only the follower of prev live
    push = lambda k: np.where(np.arange(S) == k, 5.0, 0.0)
    r0 = _step(push(NTOK + 0), start, LOOPS, t)
    assert r0["tok"] == NTOK and r0["state"] == (frozenset({0}), 0, 0)
    r1 = _step(push(SEP), r0["state"], LOOPS, t)             # pushed onto SEP, which is masked while the loop is open
    assert r1["masked"].tolist() == [True] * NTOK + [True, False, True, True] and r1["tok"] == NTOK + 1 and not r1["dead"]
    r2 = _step(flat, r1["state"], LOOPS, t)
    assert r2["tok"] == NTOK + 2 and r2["state"] == (frozenset({0, 1, 2}), None, 2)      # 2 -> 0 closes the loop: first = none
    # closed with a non-empty face: SEP and EOS open, visited edges masked
    r3 = _step(push(SEP), r2["state"], LOOPS, t)
    assert r3["masked"].tolist() == [True, True, False, False, True, True, True, False] and r3["tok"] == SEP
    assert r3["state"] == (frozenset(), None, None)          # visited cleared at SEP without ONCE ...
    r3o = _step(push(SEP), r2["state"], COEDGE, t)
    assert r3o["state"] == (frozenset({0, 1, 2}), None, None)      # ... and kept with it
    # straight after SEP: SEP masked again (no empty face, no SEP SEP ... loop), EOS open
    r4 = _step(push(SEP), r3o["state"], COEDGE, t)
    assert r4["masked"].tolist() == [True, True, True, False, True, True, True, False] and r4["tok"] == EOS and r4["fin"]
    # a one-edge self-closing loop
    r5 = _step(push(NTOK + 3), r3o["state"], COEDGE, t)
    assert r5["state"] == (frozenset({0, 1, 2, 3}), None, 3) and not r5["fin"]
    # a dead end re-opens SEP only; the next step is the closed, empty state
    dead_t = _table(L, [(0, 1)])
    st = faces.sequence_rule_advance(faces.sequence_rule_advance(start, NTOK + 0, LOOPS, NTOK, SEP, dead_t), NTOK + 1, LOOPS, NTOK, SEP, dead_t)
    assert st == (frozenset({0, 1}), 0, 1)
    r6 = _step(push(EOS), st, LOOPS, dead_t)
    assert r6["dead"] and r6["masked"].tolist() == [True, True, False, True] + [True] * L and r6["tok"] == SEP and not r6["fin"]
    assert r6["state"] == start
    r7 = _step(flat, r6["state"], LOOPS, dead_t)
    assert r7["masked"][:NTOK].tolist() == [True, True, True, False] and not r7["dead"]
    # the vote sees padding: the only follower padded is a dead end as well; visited followers only under NO_REPEAT
    pad = np.arange(S) == NTOK + 1
    assert _step(flat, (frozenset({0}), 0, 0), LOOPS, dead_t, pad=pad)["dead"]
    assert not _step(flat, (frozenset({0}), 0, 0), LOOPS, dead_t)["dead"]
    assert _step(flat, (frozenset({0, 1}), 0, 0), LOOPS, dead_t)["dead"] and not _step(flat, (frozenset({0, 1}), 0, 0), SC.CONNECT, dead_t)["dead"]
    # log-probability: fp64 log-softmax of the constrained row; no live key: token 0 and -log S; a finished row: 0, 0
    r8 = _step(np.arange(S, dtype=float), r2["state"], LOOPS, t)
    live = np.array([SEP, EOS, NTOK + 3], dtype=float)
    assert r8["tok"] == NTOK + 3 and abs(r8["logprob"] + np.log(np.exp(live - live.max()).sum())) < 1e-12
    r9 = _step(flat, start, LOOPS, t, pad=np.ones(S, bool))
    assert r9["tok"] == 0 and abs(r9["logprob"] + np.log(S)) < 1e-12
    fin = _step(flat, st, LOOPS, t, finished=True)
    assert (fin["tok"], fin["logprob"], fin["fin"], fin["state"]) == (0, 0.0, True, st)
    # other special tokens change nothing
    assert faces.sequence_rule_advance(st, 0, LOOPS, NTOK, SEP, t) == st and faces.sequence_rule_advance(st, EOS, LOOPS, NTOK, SEP, t) == st


def test_decode_loop_and_face_pieces_on_a_scripted_model():
    """sequence_constrain_ref.decode on a scripted logit source: a triangle, SEP, a dead-ended face, the self loop, EOS."""
    L, T = 5, 14
    S = NTOK + L
    t = _table(L, [(0, 1), (1, 2), (2, 0), (3, 3), (4, 1)])
    script = [NTOK + 0, NTOK + 1, NTOK + 2, SEP, NTOK + 4, EOS, NTOK + 3, SEP, EOS]      # after edge 4 -> 1 -> (2 visited? no: cleared) ...

    def step_logits(paths, step):
        row = np.zeros((1, S))
        row[0, script[min(step, len(script) - 1)]] = 9.0
        return row
    out = SC.decode(step_logits, 1, T, COEDGE, NTOK, SOS, SEP, EOS, t[None])
    tok = out["tokens"][0]
    # under ONCE edge 4 is followed by edge 1 only, which the first face holds: a dead end, SEP, flagged; then the self loop, SEP, EOS
    assert tok[:10].tolist() == [SOS, NTOK, NTOK + 1, NTOK + 2, SEP, NTOK + 4, SEP, NTOK + 3, SEP, EOS] and (tok[10:] == 0).all()
    assert out["dead"][0].tolist() == [0] * 6 + [1] + [0] * 7 and out["steps"] == 9 and out["open_end"].tolist() == [0]
    pieces = SC.face_pieces(tok, out["dead"][0], NTOK, SEP, EOS, L)
    assert pieces == [((0, 1, 2), False, False), ((4,), True, False), ((3,), False, False)]
    assert [idx for idx, _, _ in pieces] == [idx for _, idx in faces._seq_faces(tok, TOK, L, True)]
    fin, steps = SC.stop_and_finish(out["tokens"], EOS)
    assert fin.tolist() == [9] and steps == 9 and SC.unfinished_after(out["tokens"], EOS)[:9].tolist() == [1] * 8 + [0]


# ---- CPU: C ABI, binding, sources ---------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_pointer_sequence_constrained", "ff_decode_sequence_constrained_workspace_bytes", "ff_decode_sequence_constrained")


def test_header_binding_and_sources_declare_the_entries_within_abi_105():
    from faceformer_amd.hip import build, lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    assert re.search(r"#define\s+FF_CONSTRAIN_ONCE\s+0x4\b", header) and lib.FF_CONSTRAIN_ONCE == 4
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
        n_args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).count(",") + 1
        assert n_args == len(lib.SIGNATURES[name][1]), name
    fields = re.search(r"typedef struct ff_sequence_constrain_params \{(.*?)\}", code, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == [n for n, _ in lib.SequenceConstrainParams._fields_]
    doc = header[header.index("loop-constrained decode of the single-sequence model"): header.index("#define FF_CONSTRAIN_ONCE")]
    assert "model.py:161-167" in doc and "model.py:193-210" in doc and "model.py:191" in doc      # the reference call sites
    for phrase in ("SEP alone is un-masked", "A dead end ends the face, not the sequence", "SEP is masked as well while prev == none",
                   "Without CONNECT, no special token is touched and no table is read", "only together with NO_REPEAT"):
        assert phrase in doc, phrase
    assert "ff_constrain_seq.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain_seq.hip"))
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain_seq.hip")).read()
    assert "ff_loop_write_row<FF_LOOP_PLAIN>" in src and "ff_pointer_mask_reduce<true>" in src and "ff_pointer_append_row" in src
    assert "ff_pointer_count_waves" in src and "ff_loop_advance" in src and "asm" not in src      # the one copy of the rule, plain HIP
    # the existing entries keep their signatures
    assert len(lib.SIGNATURES["ff_pointer_constrained"][1]) == 31 and len(lib.SIGNATURES["ff_decode_constrained"][1]) == 20


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


# ---- CPU: every refusal -------------------------------------------------------------------------------------------------------------
def test_mode_record_lies_outside_the_mode_table():
    from faceformer_amd.hip import modes
    assert modes.SEQUENCE_CONSTRAIN is SEQUENCE_CONSTRAIN and SEQUENCE_CONSTRAIN not in modes.MODES
    assert "sequence_constrain" not in modes.SWITCH and len(modes.MODES) == 4
    assert [sequence_constrain_flags(v) for v in (None, "no_repeat", "loops", "coedge_loops", 0, 1, 2, 3, 5, 7)] == [None, 1, 3, 7, 0, 1, 2, 3, 5, 7]
    for bad in ("exact", True, 8, -1, 2.0):
        with pytest.raises(ValueError, match="sequence_constrain=.*must be None"):
            sequence_constrain_flags(bad)
    for bad in (4, 6):
        with pytest.raises(ValueError, match="FF_CONSTRAIN_ONCE \\(4\\) needs FF_CONSTRAIN_NO_REPEAT"):
            sequence_constrain_flags(bad)
    assert SEQUENCE_CONSTRAIN.entry == "ff_decode_sequence_constrained" and not SEQUENCE_CONSTRAIN.term_range and not SEQUENCE_CONSTRAIN.per_anchor
    assert [k for k, _, _ in SEQUENCE_CONSTRAIN.outs] == ["logprob", "dead_end", "open_end"]
    # the recorded texts stay
    assert modes.SWITCH["constrain"].seq2seq == "the single-sequence model emits loops of plain edges"
    assert modes.constrain_flags("loops") == 3
    with pytest.raises(ValueError, match="constrain=4: must be None, 'no_repeat', 'loops' or flag bits 0..3"):
        modes.constrain_flags(4)
    with pytest.raises(ValueError, match="constrain='coedge_loops': must be None, 'no_repeat' or 'loops'"):
        modes.constrain_flags("coedge_loops")


def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes = {}
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    ft = torch.zeros(2, 8, 1, dtype=torch.int32)
    ok = dict(T=5, F=1, sequence_constrain="loops", tok_sep=SEP, follow_table=ft)
    with pytest.raises(ValueError, match="sequence_constrain is a single-sequence option .* constrain"):
        eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=2),
                   dict(constrain="no_repeat"), dict(constrain=0), dict(sequence_samples=2), dict(sequence_beams=2)):
        with pytest.raises(ValueError, match="sequence_constrain excludes"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    with pytest.raises(ValueError, match="sequence_constrain excludes stop_each_eos"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, flags=engine.DEFAULT_FLAGS | lib.FF_STOP_EACH_EOS, **ok)
    for bad in ("exact", 8, True, 4, 6):
        with pytest.raises(ValueError, match="sequence_constrain="):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_constrain=bad))
    with pytest.raises(ValueError, match="sequence_constrain needs tok_sep"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, tok_sep=None))
    for sep, eos in ((EOS, EOS), (NTOK, EOS), (-1, EOS), (SEP, NTOK)):
        with pytest.raises(ValueError, match="tok_sep=.* and tok_eos=.* must be two different special tokens"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, tok_sep=sep, tok_eos=eos))
    for flags in ("loops", "coedge_loops", 2):
        with pytest.raises(ValueError, match="needs follow_table"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_constrain=flags, follow_table=None))
    for bad in (torch.zeros(2, 8, 2, dtype=torch.int32), torch.zeros(2, 8, 1), torch.zeros(1, 8, 1, dtype=torch.int32), [[0]]):
        with pytest.raises(ValueError, match="follow_table must be an int32 tensor of shape \\[2, 8, 1\\]"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, follow_table=bad))
    # the recorded rejection of constrain on the single-sequence variant stays what it is
    with pytest.raises(ValueError, match="constrain is a parallel-variant option"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, T=5, F=1, constrain="loops", term_range=(1, 4), follow_table=ft)


def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _seq_inputs(**more):
    return dict({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                 "label": torch.zeros(1, 6, dtype=torch.long)}, **more)


def test_models_reject_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    par = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert par.sequence_constrain is None
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    for value in ("loops", 0):
        par.sequence_constrain = value
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain is a SurfaceFormer option .* constrain"):
            par.forward_eval(inputs)
    assert "predict" not in inputs
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.sequence_constrain is None and seq.constrain_tol == 2e-4
    seq.sequence_constrain = "coedge_loops"
    text = "sequence_constrain excludes sequence_samples, sequence_beams, return_logprob and an extra mask"
    for attr, val, off in (("sequence_samples", 2, 0), ("sequence_beams", 2, 0), ("return_logprob", True, False)):
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="excludes"):      # (sequence_beams' own record reports first: either text)
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, off)
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
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    for bad in ("exact", 8, True, 4):
        seq.sequence_constrain = bad
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain="):
            seq.forward_eval(_seq_inputs())
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_constrain = "loops"
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain needs the native engine"):
            sub.forward_eval(_seq_inputs())
    # what the model already refuses stays refused, with its recorded text, with or without the new option
    for value in (None, "loops"):
        seq.sequence_constrain = value
        for attr, val, off, word in (("constrain", "loops", None, "the single-sequence model emits loops of plain edges"),
                                     ("num_samples", 2, 0, "sampling for the single-sequence model is not implemented"),
                                     ("retire_finished", True, False, "the single-sequence model has one sequence per wireframe")):
            setattr(seq, attr, val)
            with torch.no_grad(), pytest.raises(ValueError, match="%s is a SurfaceFormer_Parallel option \\(%s\\)" % (attr, word)):
                seq.forward_eval(_seq_inputs())
            setattr(seq, attr, off)
    # an empty batch publishes the same keys, empty, and touches nothing
    seq.sequence_constrain = "loops"
    with torch.no_grad():
        out = seq.forward_eval({"input": torch.zeros(0, 8, 50, 2), "input_mask": torch.zeros(0, 8, dtype=torch.bool),
                                "label": torch.zeros(0, 6, dtype=torch.long)})
    assert "pointer" not in out and tuple(out["predict"].shape) == (0, 6) and out["predict"].dtype == torch.int64
    assert tuple(out["predict_logprob"].shape) == (0, 6) and out["predict_logprob"].dtype == torch.float32
    assert tuple(out["predict_dead_end"].shape) == (0, 6) and out["predict_dead_end"].dtype == torch.int32
    assert tuple(out["predict_open_end"].shape) == (0,) and out["predict_open_end"].dtype == torch.int32
    assert tuple(out["embedding"].shape) == (0, 8 + NTOK, 64)


def test_decode_sharded_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, sequence_constrain=0)
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_constrain"):
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_constrain = None
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_flags_reach_the_model_and_every_refusal_raises(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain", "coedge_loops"])
    assert a.sequence_constrain == "coedge_loops" and a.constrain is None
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).sequence_constrain is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain", "exact"])
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-constrain", "loops", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["sequence_constrain"], kw["constrain"]) for kw in seen] == [("loops", None), (None, None)]
    m = cli.configure_model(types.SimpleNamespace(), sequence_constrain="loops", constrain_tol=1e-3)
    assert vars(m) == dict(sequence_constrain="loops", constrain_tol=1e-3)
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    seqcfg = types.SimpleNamespace(model_class="SurfaceFormer")
    call = dict(out_dir="unused", device="cpu", model=object())
    with pytest.raises(ValueError, match="--sequence-constrain applies to SurfaceFormer only .*--constrain"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer_Parallel"), None, sequence_constrain="loops", **call)
    with pytest.raises(ValueError, match="--sequence-constrain must be no_repeat, loops or coedge_loops"):
        run_test(seqcfg, None, sequence_constrain="exact", **call)
    for kw in (dict(scores=True), dict(score_labels=True), dict(sample=2), dict(beam=2), dict(constrain="loops"), dict(sequence_samples=2),
               dict(sequence_beams=2), dict(device_faces=True), dict(sequence_device_faces=True)):
        with pytest.raises(ValueError, match="--sequence-constrain does not combine with --scores, --score-labels, --sample, --beam, --constrain, "
                                             "--sequence-samples, --sequence-beams, --device-faces or --sequence-device-faces"):
            run_test(seqcfg, None, sequence_constrain="loops", **dict(call, **kw))
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sequence-constrain is not implemented for multi-rank runs"):
        run_test(seqcfg, None, sequence_constrain="loops", dist_mod=world2, **call)
    with pytest.raises(ValueError, match="--constrain applies to SurfaceFormer_Parallel only"):      # an existing text, unchanged
        run_test(seqcfg, None, constrain="loops", **call)


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
    pred = np.zeros(24, dtype=np.int64)
    pred[:11] = [1, E + 0, E + 1, E + 2, E + 3, 2, E + 4, E + 5, 2, E + 4, 3]          # a closed square, an abandoned face, an open one
    dead = np.zeros(24, dtype=np.int32)
    dead[8] = 1
    text, st = cli.record_of(cfg, raw, item, pred, False)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
    text2, st2 = cli.record_of(cfg, raw, item, pred, False, sequence_constrained=dead)
    rec2 = json.loads(text2)
    assert list(rec2) == list(rec) + ["pred_dead_ends", "pred_unclosed"] and st2 == st
    assert {k: rec2[k] for k in rec} == rec and text == cli.record_of(cfg, raw, item, pred, False, sequence_constrained=None)[0]
    assert rec2["pred_dead_ends"] == 1 and rec2["pred_unclosed"] == 2


# ---- GPU: the operator --------------------------------------------------------------------------------------------------------------
E_OP = 64
KINDS = ("start", "open", "dead", "closed", "closed_empty", "finished")


def _words(sets, L):
    fw = (L + 31) // 32
    w = np.zeros((len(sets), max(fw, 0)), dtype=np.uint32)
    for r, s in enumerate(sets):
        for e in s:
            w[r, e >> 5] |= np.uint32(1) << np.uint32(e & 31)
    return w.view(np.int32)


def _operator_case(B, S, spg, seed, scenario="mixed"):
    """B rows of W = ceil(B / spg) wireframes with different kv_len and a padding mask, a random_follows table, and one state per
    row: the kinds of KINDS in turn ("mixed"), every row closed with a non-empty face and pushed onto SEP ("sep"), every row
    finished or closed and pushed onto EOS ("done").  Mixed rows are pushed in turn onto nothing, SEP, EOS and an edge that closes
    the loop.  -> dict of CPU tensors / arrays."""
    g = np.random.default_rng([0x5EC0, seed, B, S, spg])
    L, W = S - NTOK, (B + spg - 1) // spg
    t = CR.random_follows(W, L, seed)
    logits = (g.standard_normal((B, S)) * 3.0).astype(np.float32)
    mask = g.random((W, S)) < 0.2
    mask[:, :NTOK] = False
    kv = np.array([S - (w % 2) for w in range(W)], dtype=np.int32)
    pad = mask | (np.arange(S)[None, :] >= kv[:, None])
    fin = np.zeros(B, dtype=np.int32)
    first, prev, visited, kinds = np.full(B, -1, np.int32), np.full(B, -1, np.int32), [set() for _ in range(B)], []
    for b in range(B):
        w = b // spg
        kind = KINDS[(b + seed) % len(KINDS)] if scenario == "mixed" else ("closed" if scenario == "sep" or b % 2 else "finished")
        kinds.append(kind)
        a, f = int(g.integers(0, L)), int(g.integers(0, L))
        push = ("none", "sep", "eos", "close")[(b // 2 + seed) % 4] if scenario == "mixed" else ("sep" if scenario == "sep" else "eos")
        if kind == "open":
            first[b], prev[b], visited[b] = f, a, {f, a}
            c = int(g.integers(0, L))
            t[w, a, c] = True                                     # at least one follower
            if push == "close" and not pad[w, NTOK + c] and c not in visited[b]:
                t[w, c, f] = True                                 # ... which closes the loop
                logits[b, NTOK + c] = 1.0e4
        elif kind == "dead":
            first[b], prev[b], visited[b] = f, a, {f, a}
            way = b % 3
            if way == 0:                                          # every follower visited (a dead end under NO_REPEAT)
                visited[b] |= set(np.flatnonzero(t[w, a]).tolist())
            elif way == 1 and mask[w, NTOK:].any():               # the only follower padded
                t[w, a, :] = False
                t[w, a, int(np.flatnonzero(mask[w, NTOK:])[0])] = True
            elif kv[w] < S:                                       # the only follower beyond kv_len
                t[w, a, :] = False
                t[w, a, L - 1] = True
            else:
                t[w, a, :] = False                                # no follower at all
        elif kind == "closed":
            prev[b], visited[b] = a, {a}
        elif kind == "closed_empty":
            visited[b] = {f}                                      # (as after SEP under ONCE)
        elif kind == "finished":
            fin[b], first[b], prev[b], visited[b] = 1, f, a, {f, a}
        if push == "sep":
            logits[b, SEP] = 1.0e4
        elif push == "eos":
            logits[b, EOS] = 1.0e4
    memory = g.standard_normal((W, S, E_OP)).astype(np.float32)
    return dict(logits=logits, mask=mask, kv=kv, pad=pad, fin=fin, first=first, prev=prev, visited=visited, kinds=kinds, table=t,
                memory=memory, B=B, S=S, L=L, W=W, spg=spg)


def _run_operator(c, flags, counter=None, want_stats=True):
    from faceformer_amd.hip import ops
    lg = torch.from_numpy(c["logits"]).clone().cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    res = ops.pointer_sequence_constrained(
        lg, dev(c["fin"]), dev(c["first"]), dev(c["prev"]), dev(_words(c["visited"], c["L"])), flags, NTOK, SEP, EOS,
        follows=dev(faces.pack_follow_bits(c["table"])) if flags & SC.CONNECT else None, memory=dev(c["memory"]),
        mask=dev(c["mask"].astype(np.uint8)), kv_len=dev(c["kv"]), seqs_per_group=c["spg"], want_rows=True, want_stats=want_stats,
        counter=counter)
    return lg, res


def _check_operator(c, flags, seen):
    from faceformer_amd.hip import ops
    B, S, L, spg = c["B"], c["S"], c["L"], c["spg"]
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_operator(c, flags, counter)
    what = (S, B, spg, flags)
    own = lg.cpu().numpy()
    got = {k: res[k].cpu().numpy() for k in ("next", "logprob", "fin", "dead_end", "first", "prev", "visited", "mask_rows")}
    unfinished_after = 0
    for b in range(B):
        w = b // spg
        none = lambda v: None if v < 0 else int(v)
        fi, pv = none(c["first"][b]), none(c["prev"][b])
        state = (frozenset(c["visited"][b]), fi, pv)
        table = c["table"][w] if flags & SC.CONNECT else None                     # (without CONNECT no table is given: no loop closes)
        want = faces.sequence_rule_step(c["logits"][b], c["pad"][w], state, flags, NTOK, SEP, EOS, table, finished=bool(c["fin"][b]))
        # the byte row and the FILL pattern of the masked row, exact
        assert np.array_equal(got["mask_rows"][b] != 0, want["masked"]), (what, b, c["kinds"][b])
        if c["fin"][b]:
            assert np.array_equal(own[b], c["logits"][b]), (what, b)                # a finished row is not touched
        else:
            assert np.array_equal(own[b] <= FILL, want["masked"] | c["pad"][w]), (what, b)
            live = own[b] > FILL
            assert np.array_equal(own[b][live], c["logits"][b][live]), (what, b)
        # the numpy rule on the kernel's own masked row: token, flags, state, visited words exact; the log-probability to the bar
        again = faces.sequence_rule_step(own[b].astype(np.float64), own[b] <= FILL, state, 0, NTOK, SEP, EOS, None, finished=bool(c["fin"][b]))
        assert got["next"][b] == want["tok"] == again["tok"], (what, b, c["kinds"][b], got["next"][b], want["tok"])
        assert bool(got["dead_end"][b]) == want["dead"] and bool(got["fin"][b]) == want["fin"], (what, b, c["kinds"][b])
        vis, nf, npv = want["state"]
        assert (got["first"][b], got["prev"][b]) == (-1 if nf is None else nf, -1 if npv is None else npv), (what, b, c["kinds"][b])
        if L:
            assert np.array_equal(got["visited"][b], _words([vis], L)[0]), (what, b, c["kinds"][b])
        lp = float(got["logprob"][b])
        assert abs(lp - again["logprob"]) <= SC.LP_BAR + SC.EPS * abs(again["logprob"]), (what, b, lp, again["logprob"])
        if c["fin"][b]:
            assert got["next"][b] == 0 and lp == 0.0
        unfinished_after += not want["fin"]
        seen["dead"] += want["dead"]
        seen["sep"] += (not c["fin"][b]) and want["tok"] == SEP
        seen["eos"] += (not c["fin"][b]) and want["tok"] == EOS
        seen["closing"] += (not c["fin"][b]) and fi is not None and pv is not None and want["tok"] >= NTOK and nf is None
        seen["cleared"] += (not c["fin"][b]) and want["tok"] == SEP and len(state[0]) > 0 and len(vis) == 0
        seen["kept"] += (not c["fin"][b]) and want["tok"] == SEP and len(vis) > 0
    assert int(counter.item()) == unfinished_after, (what, int(counter.item()), unfinished_after)
    # appended rows and statistics: ff_gather_rows of memory[b / spg, tok]; the statistics of the forced step on the same tokens
    mem = torch.from_numpy(c["memory"]).cuda()
    assert torch.equal(res["rows"], ops.gather_rows(mem, res["next"], seqs_per_group=spg)), what
    forced = ops.pointer_forced(torch.from_numpy(c["logits"]).clone().cuda(), res["next"], memory=mem, seqs_per_group=spg, want_rows=True,
                                want_stats=True)
    assert torch.equal(res["rows"], forced["rows"]) and torch.equal(res["stats"], forced["stats"]), what
    lg2, res2 = _run_operator(c, flags)                                             # two launches
    assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
    return int(counter.item())


@pytest.mark.gpu
@pytest.mark.parametrize("spg", [1, 4])
@pytest.mark.parametrize("S", [5, 65, 260, 1028])
def test_operator_against_the_numpy_rule(hip_lib, S, spg):
    seen = dict(dead=0, sep=0, eos=0, closing=0, cleared=0, kept=0)
    for B in (1, 5, 8):
        for flags in (0, 1, 2, 3, 7):
            for seed in (1, 2):
                _check_operator(_operator_case(B, S, spg, seed + 10 * flags), flags, seen)
            c = _operator_case(B, S, spg, 7, "sep")
            assert _check_operator(c, flags, seen) == B, (S, B, spg, flags)          # every row on SEP: nothing stops
            c = _operator_case(B, S, spg, 8, "done")
            assert _check_operator(c, flags, seen) == 0, (S, B, spg, flags)          # every row on EOS or finished
    print("S=%d spg=%d:" % (S, spg), seen)
    assert seen["sep"] and seen["eos"] and seen["cleared"] and seen["kept"]
    if S >= 65:
        assert seen["dead"] and seen["closing"], seen


def _raw_call(lib, c, over=None, flags=3):
    """ff_pointer_sequence_constrained through ctypes with `over` replacing named arguments; every output holds a sentinel."""
    B, S, L = c["B"], c["S"], c["L"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lg = dev(c["logits"])
    keep = dict(fin=dev(c["fin"]), first=dev(c["first"]), prev=dev(c["prev"]), visited=dev(_words(c["visited"], L)),
                follows=dev(faces.pack_follow_bits(c["table"])), mask=dev(c["mask"].astype(np.uint8)), kv=dev(c["kv"]), memory=dev(c["memory"]))
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
             ldnext=E_OP, next_stats=None, count=outs["count"].data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    a.update(over or {})
    rc = lib.ff_pointer_sequence_constrained(*a.values())
    torch.cuda.synchronize()
    return rc, lg, keep, outs


@pytest.mark.gpu
def test_operator_err_arg_leaves_the_outputs_untouched(hip_lib):
    lib = hip_lib
    c = _operator_case(5, 65, 4, 3)
    rc, lg, keep, outs = _raw_call(lib, c)
    assert rc == 0 and int(outs["next_tok"].min()) >= 0 and int(outs["count"].item()) >= 5          # the arguments are good ones
    for over in (dict(flags=8), dict(flags=16 | 3), dict(flags=-1), dict(flags=4), dict(flags=6),           # unknown bits; ONCE without NO_REPEAT
                 dict(follows=None), dict(flags=2, follows=None), dict(flags=7, follows=None),              # CONNECT with a null table
                 dict(tok_sep=NTOK), dict(tok_sep=-1), dict(tok_eos=NTOK), dict(tok_eos=-1), dict(tok_sep=EOS), dict(tok_eos=SEP),
                 dict(L=c["L"] - 1), dict(ntok=NTOK + 1), dict(spg=0), dict(S=0), dict(ldlogits=c["S"] - 1),
                 dict(mask_rows=None), dict(next_tok=None), dict(logprob=None), dict(fin_out=None), dict(dead_end=None),
                 dict(first_out=None), dict(prev_out=None), dict(fin_in=None), dict(first_in=None), dict(prev_in=None), dict(visited=None),
                 dict(logits=None), dict(memory=None), dict(ldnext=E_OP - 4)):
        rc, lg, keep, outs = _raw_call(lib, c, over)
        assert rc == -1, (over, rc)                                                   # FF_ERR_ARG
        assert torch.equal(lg.cpu(), torch.from_numpy(c["logits"])), over
        assert torch.equal(keep["visited"].cpu(), torch.from_numpy(_words(c["visited"], c["L"]))), over
        assert bool((outs["mask_rows"] == 77).all()) and bool((outs["next_rows"] == 7.5).all()) and bool((outs["logprob"] == 7.5).all()), over
        assert all(bool((outs[k] == -7).all()) for k in ("next_tok", "fin_out", "dead_end", "first_out", "prev_out")), over
        assert int(outs["count"].item()) == 5, over
    # the existing entry keeps refusing bit 4 as an unknown flag bit
    from faceformer_amd.hip import ops
    with pytest.raises(ValueError, match="unknown constraint flag bits 5"):
        ops.pointer_constrained(torch.zeros(1, 8).cuda(), *(torch.zeros(1, dtype=torch.int32).cuda() for _ in range(3)),
                                torch.zeros(1, 1, dtype=torch.int32).cuda(), 5, NTOK)
    a = [0] * 31
    z = torch.zeros(64, dtype=torch.int32).cuda()
    args = [z.data_ptr(), 8, 8, None, None, 1, 1, None, 4, 5, NTOK, 1, 4] + [z.data_ptr()] * 11 + [None, 0, None, 0, None, None, None]
    assert len(args) == len(a) and lib.ff_pointer_constrained(*args) == -1
    assert b"unknown flag bits 5" in lib.ff_last_error()


# ---- GPU: the engine ----------------------------------------------------------------------------------------------------------------
_MODELS, _FIX = {}, {}
SMALL = ["seq_small_gain4", "seq_small_eos", "seq_small_repeat_eos"]


def _model(name):
    if name not in _MODELS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        _MODELS[name] = (case, z, build_model(case, sd, "cuda"), batch_to(batch, "cuda"), sd, batch)
    return _MODELS[name]


def _fixture(name, kind, seed):
    """-> (case, model, batch on the device, batch on the CPU, follows bool [N, L, L], packed words on the device, edges, sd)."""
    key = (name, kind, seed)
    if key not in _FIX:
        case, z, model, b, sd, gb = _model(name)
        batch, follows, edges = SC.fixture(case, gb, kind, seed)
        _FIX[key] = (case, model, batch_to(batch, "cuda"), batch, follows, torch.from_numpy(faces.pack_follow_bits(follows)).cuda(), edges, sd)
    return _FIX[key]


def _decode(model, case, batch, **kw):
    from test_logprob import _decode as decode
    out = decode(model, case, batch, **kw)
    out.pop("engine", None)
    return out


def _constrained(model, case, b, flags, table, **kw):
    return _decode(model, case, b, sequence_constrain=flags, tok_sep=SEP, follow_table=table if flags & SC.CONNECT else None,
                   return_pointer=False, **kw)


def _check_layout(out, T, flags, follows):
    """Finish positions, the stop step, the per-step counts, open_end and the zero padding against the rule applied to the decode's
    own tokens.  Returns (tokens, logprob, dead, finish positions, steps, states)."""
    tok, lp, dead, oe = (out[k].cpu().numpy() for k in ("predict", "logprob", "dead_end", "open_end"))
    N = tok.shape[0]
    assert tok.dtype == np.int64 and lp.dtype == np.float32 and dead.dtype == np.int32 and oe.dtype == np.int32
    assert tok.shape == lp.shape == dead.shape == (N, T) and oe.shape == (N,)
    assert (tok[:, 0] == SOS).all()
    fin, steps = SC.stop_and_finish(tok, EOS)
    assert out["steps"] == steps, (out["steps"], steps)
    assert out["step_counts"] == SC.unfinished_after(tok, EOS)[:steps].tolist()
    last = np.minimum(fin, steps)
    past = np.arange(T)[None, :] > last[:, None]
    assert (tok[past] == 0).all() and (lp[past] == 0).all() and (dead[past] == 0).all() and (lp[:, 0] == 0).all() and (dead[:, 0] == 0).all()
    assert np.isfinite(lp).all() and (lp <= 0).all() and ((dead == 0) | (dead == 1)).all()
    states = SC.replay_states(tok, flags, NTOK, SEP, follows)
    assert oe.tolist() == [int(states[r][last[r]][1] is not None) for r in range(N)]
    return tok, lp.astype(np.float64), dead, fin, steps, states


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_with_bits_clear_is_the_greedy_decode_cut_at_every_eos(hip_lib, name):
    from faceformer_amd.hip import lib as L
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    greedy = _decode(model, case, b, logprob=True, flags=model.decode_flags | L.FF_STOP_EACH_EOS)
    pred = greedy["predict"].cpu().numpy()
    N = pred.shape[0]
    want = np.stack([faces.apply_own_stop_rule(pred[w], TOK, parallel=False) for w in range(N)])
    glp = np.stack([faces._apply_own_stop_rule_scored(pred[w], greedy["logprob"][w].cpu().numpy(), TOK, False)[1] for w in range(N)])
    out = _constrained(model, case, b, 0, None)
    tok, lp, dead, fin, steps, _ = _check_layout(out, T, 0, None)
    assert steps == greedy["steps"] and np.array_equal(tok, want), (name, steps, greedy["steps"])
    assert out["step_counts"] == (N - np.cumsum(greedy["step_counts"])).tolist()      # the greedy counter: first EOS tokens per step
    assert np.array_equal(out["logprob"].cpu().numpy(), glp.astype(np.float32)), (name, np.abs(lp - glp).max())      # one reduction, same rows
    assert not dead.any()                                                             # (open_end: _check_layout, on the replayed state)


def _walk_closed(idx, table):
    first = prev = None
    for e in idx:
        if first is None:
            first = e
        elif not table[prev][e]:
            return False
        prev = e
        if table[e][first]:
            first = None
    return first is None


def _replay(out, case, ni, flags, follows, what):
    """The numpy rule on the decode's own traced logits, pair by pair: the FILL pattern, the dead flag, the finish and the
    log-probability everywhere; the token where the margin exceeds 2 tol(step).  Returns (left-out pairs, pairs)."""
    from test_parity_golden import _tol
    T, S = case["model"]["seq_len"], case["model"]["L"] + NTOK
    tok, lp, dead, fin, steps, states = _check_layout(out, T, flags, follows)
    logits = out["logits"].cpu().numpy()
    pairs = left = 0
    for j in range(steps):
        rows = np.flatnonzero(fin > j)
        tol = _tol(logits[j][rows])
        for r in rows:
            row = logits[j, r].astype(np.float64)
            pad = np.arange(S) >= NTOK + ni[r]                                        # the padding the encoder's mask holds
            masked, is_dead = faces.sequence_rule_mask(states[r][j], flags, S, NTOK, SEP, EOS, follows[r], pad)
            assert np.array_equal(row <= FILL, masked | pad), (what, j, int(r))        # the constrained masked row, exact
            assert bool(dead[r, j + 1]) == is_dead, (what, j, int(r))
            res = faces.sequence_rule_step(row, row <= FILL, states[r][j], 0, NTOK, SEP, EOS, None)
            pairs += 1
            if SC.margin(row) > 2 * tol:
                assert tok[r, j + 1] == res["tok"], (what, j, int(r), int(tok[r, j + 1]), res["tok"])
            else:
                left += 1
                assert row[tok[r, j + 1]] > FILL, (what, j, int(r))                   # an indecisive pair still selects a live key
            own = faces.sequence_rule_step(np.where(np.arange(S) == tok[r, j + 1], row + 1e9, row), row <= FILL, states[r][j], 0, NTOK, SEP, EOS, None)
            assert own["tok"] == tok[r, j + 1]
            m = row[tok[r, j + 1]]
            want_lp = -np.log(np.exp(row - m).sum())
            assert abs(lp[r, j + 1] - want_lp) <= SC.LP_BAR + SC.EPS * abs(want_lp), (what, j, int(r))
    return left, pairs


def _oracle_logits(case, sd, batch, tok, steps):
    """fp64 masked logits [steps, N, S] of the oracle teacher-forced along `tok` (oracle/refpath.py, forced=), on the GPU."""
    from oracle import refpath
    sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
    b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}
    tr = {}
    refpath.seq2seq_forward_eval(sd64, dict(b64), num_head=case["model"]["H"], label_seq_length=tok.shape[1], token_sos=SOS, token_eos=EOS,
                                 trace=tr, forced=torch.from_numpy(np.ascontiguousarray(tok)), steps=steps)
    return torch.stack(tr["logits"]).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", SC.FLAGS)
@pytest.mark.parametrize("fix", SC.FIXTURES, ids=lambda f: "%s-%s%d" % f)
def test_engine_replays_under_the_numpy_rule_and_keeps_the_guarantee(hip_lib, fix, flags):
    """The (golden, kind, seed, flags) triples are sequence_constrain_ref's: kept on the CPU by tools/sequence_constrain_left_out.py."""
    from test_parity_golden import _tol
    assert fix + (flags,) in SC.KEPT, "not a kept triple"
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    ni = batch["num_input"]
    T = case["model"]["seq_len"]
    out = _constrained(model, case, b, flags, table, trace=True)
    left, pairs = _replay(out, case, ni, flags, follows, fix + (flags,))
    tok, dead, oe = out["predict"].cpu().numpy(), out["dead_end"].cpu().numpy(), out["open_end"].cpu().numpy()
    print(fix, flags, "steps=%d left-out pairs: %d of %d; dead ends %d; open_end %s" % (out["steps"], left, pairs, int(dead.sum()), oe.tolist()))
    assert left <= SC.CAP * pairs, (fix, flags, left, pairs)
    # the guarantee, exact given the table
    enc = par = 0
    for w, n in enumerate(ni):
        pieces = SC.face_pieces(tok[w], dead[w], NTOK, SEP, EOS, n)
        assert [idx for idx, _, _ in pieces] == [idx for _, idx in faces._seq_faces(tok[w], TOK, n, True)]
        row_edges = [e for idx, _, _ in pieces for e in idx]
        for k, (idx, at_dead_end, unterminated) in enumerate(pieces):
            assert len(set(idx)) == len(idx), (fix, flags, w, idx)                    # no face holds an edge twice
            closed = _walk_closed(idx, follows[w]) if edges is None else bool(faces.is_face_enclosed(edges[w], idx, SC.TOL))
            par += 1
            enc += closed
            open_piece = unterminated or (oe[w] and k == len(pieces) - 1 and (tok[w] == EOS).sum() == 0)
            if not at_dead_end and not open_piece:
                assert closed, (fix, flags, w, idx)
        if flags & SC.ONCE:
            assert len(set(row_edges)) == len(row_edges), (fix, flags, w)             # no edge occurs twice in the row
    kept = SC.KEPT[fix + (flags,)]
    if left == 0:
        assert (enc, par, int(dead.sum())) == kept[2:], (fix, flags, (enc, par, int(dead.sum())), kept)
    if fix[1] == "random":
        assert dead.sum() > 0                                                         # the random tables are what exercise dead ends
    # traced logits against the fp64 oracle forced along the constrained tokens
    steps = out["steps"]
    truth = _oracle_logits(case, sd, batch, tok, steps)
    got = out["logits"].cpu().numpy()
    fin, _ = SC.stop_and_finish(tok, EOS)
    worst = 0.0
    for j in range(steps):
        rows = np.flatnonzero(fin > j)
        tol = _tol(truth[j][rows])
        for r in rows:
            live = got[j, r] > FILL
            err = np.abs(got[j, r][live] - truth[j, r][live]).max()
            worst = max(worst, err / tol)
            assert err <= tol, (fix, flags, j, int(r), err, tol)
    print(fix, flags, "worst |logit - oracle| / tol = %.3f" % worst)


@pytest.mark.gpu
def test_engine_micro_batch_cut_and_repeatability(hip_lib):
    fix = ("seq_small_gain4", "lattice", 1)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    whole = _constrained(model, case, b, COEDGE, table, trace=True)
    again = _constrained(model, case, b, COEDGE, table, trace=True)
    keys = ("predict", "logprob", "dead_end", "open_end", "logits")
    assert whole["steps"] == again["steps"] and whole["step_counts"] == again["step_counts"]
    for k in keys:                                                                    # one plan, two runs: bit-equal (the trace up to the stop)
        n = whole["steps"] if k == "logits" else None
        assert torch.equal(whole[k][:n], again[k][:n]), k
    one = _constrained(model, case, b, COEDGE, table, trace=True, chunk_max_seqs=1)   # one wireframe per micro-batch
    assert sorted(int(v) for v in one["seq_of_row"].cpu()) == list(range(b["input"].size(0)))
    lw, pw = _replay(whole, case, batch["num_input"], COEDGE, follows, "whole")
    lo, po = _replay(one, case, batch["num_input"], COEDGE, follows, "one")
    assert lw <= SC.CAP * pw and lo <= SC.CAP * po
    if lw == 0 and lo == 0:                                                           # every pair decisive in both: the same decode
        for k in ("predict", "dead_end", "open_end"):
            assert torch.equal(whole[k], one[k]), k
        assert whole["steps"] == one["steps"] and whole["step_counts"] == one["step_counts"]


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "seq_small_gain4"
    m = WP._bound(name, "default")
    batch, follows, _ = SC.fixture(m.case, m.batch, "random", 1)
    b = batch_to(batch, "cuda")
    table = torch.from_numpy(faces.pack_follow_bits(follows)).cuda()
    call = lambda: _constrained(m.model, m.case, b, COEDGE, table, trace=True)
    clean = call()
    zero, d = WP._run([m], call, fill=RZ.ZERO, what="sequence constrain after ZERO")
    poison, _ = WP._run([m], call, fill=RZ.POISON, what="sequence constrain after POISON")
    WP._assert_equal(poison, zero, "sequence constrain")
    WP._assert_equal(poison, clean, "sequence constrain against the clean run")
    WP._assert_no_nan(poison, "sequence constrain")
    assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size
    assert int(zero["dead_end"].sum()) > 0


# ---- GPU: the model and the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_publishes_the_keys_and_sequence_faces_works_behind_it(hip_lib):
    fix = ("seq_small_gain4", "lattice", 2)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N = case["model"]["seq_len"], b["input"].size(0)
    gb = _model(fix[0])[3]
    try:
        with torch.no_grad():
            off = model(dict(gb))
            model.sequence_constrain = "coedge_loops"
            on = model(dict(b))                                       # the table is built from the end points with constrain_tol
            given = model(dict(b, follow_table=table))
            as_bool = model(dict(b, follow_table=torch.from_numpy(follows)))
            model.sequence_faces = "enclosed"
            both = model(dict(b))
            model.sequence_faces = False
            model.sequence_constrain = "no_repeat"                    # no table is built without CONNECT
            norep = model(dict(b, follow_table="not a table"))
    finally:
        model.sequence_constrain, model.sequence_faces = None, False
    assert np.array_equal(off["predict"].cpu().numpy(), _model(fix[0])[1]["predict"])      # off: today's decode, today's keys
    new = {"predict_logprob", "predict_dead_end", "predict_open_end"}
    assert set(on) == (set(off) - {"pointer"}) | new and not new & set(off)
    assert tuple(on["predict"].shape) == (N, T) and on["predict"].dtype == torch.int64
    assert tuple(on["predict_logprob"].shape) == (N, T) and on["predict_logprob"].dtype == torch.float32
    assert tuple(on["predict_dead_end"].shape) == (N, T) and on["predict_dead_end"].dtype == torch.int32
    assert tuple(on["predict_open_end"].shape) == (N,) and on["predict_open_end"].dtype == torch.int32
    for k in new | {"predict", "embedding"}:
        assert torch.equal(on[k], given[k]) and torch.equal(on[k], as_bool[k]) and torch.equal(on[k], both[k]), k
    direct = _constrained(model, case, b, COEDGE, table)
    assert torch.equal(direct["predict"], on["predict"]) and torch.equal(direct["logprob"], on["predict_logprob"])
    assert torch.equal(direct["dead_end"], on["predict_dead_end"]) and torch.equal(direct["open_end"], on["predict_open_end"])
    assert model.last_constrain_stats["steps"] > 0 and tuple(norep["predict"].shape) == (N, T)
    # sequence_faces = "enclosed" behind the option: faces.face_seq_rows / face_seq_votes on the published tensors
    ni = np.asarray(batch["num_input"], dtype=np.int32)
    want = faces.face_seq_rows(both["predict"].cpu().numpy(), ni, TOK, logprob=both["predict_logprob"].cpu().numpy(),
                               follows=faces.pack_follow_bits(follows), closed_only=True)
    want.update(faces.face_seq_votes(want, require_closed=True))
    found = both["sequence_faces"]
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
    plain2 = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "plain2"), sequence_constrain=None)
    loops = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "loops"), sequence_constrain="coedge_loops")
    batched = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "batched"), sequence_constrain="coedge_loops", batch_size=2)
    new = ["pred_dead_ends", "pred_unclosed"]
    for fn in sorted(os.listdir(plain)):
        text = open(os.path.join(plain, fn)).read()
        assert text == open(os.path.join(plain2, fn)).read()          # byte-identical without the flag
        rec = json.loads(text)
        assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
        rl, rb = (json.load(open(os.path.join(d, fn))) for d in (loops, batched))
        assert list(rl) == list(rec) + new and list(rb) == list(rec) + new
        assert isinstance(rl["pred_dead_ends"], int) and 0 <= rl["pred_unclosed"] <= len(rl["pred_faces"]) + rl["pred_dead_ends"] + 1
        for face in rl["pred_faces"]:
            idx = face[1] if isinstance(face, (list, tuple)) and len(face) == 2 and isinstance(face[1], (list, tuple)) else face
            assert len(set(idx)) == len(idx)
