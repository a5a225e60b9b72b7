"""Opt-in beam search over the single-sequence decode (SurfaceFormer.sequence_beams): the rule on hand-written rows,
every refusal, the faces of the beams and the CLI flags on the CPU (library untouched); the sequence forms of the selection step,
the engine's mode, the model and the CLI on the GPU, through the C ABI.  The rule is tests/sequence_beam_ref.py (beam_ref's step;
its own start / finish / counters / stop rules).

Bars (the issue's, none measured): parent, token and finished flag must equal the fp64 rule's on every group whose decisive gap
exceeds 1 (beam_ref's criterion; margin j + 1 at step j of a replay, a group leaving the comparison at its first indecisive step);
scores within beam_ref.score_bound per step; oracle scores within the sum over the beam's steps of 2 tol(step) + 2^-16
(tol: test_parity_golden._tol); at most 2 % of a case's groups / (step, group) pairs may be left out -- a condition on the inputs,
fixed on the CPU by tools/sequence_beam_left_out.py (sequence_beam_ref.OP_SEED_OFFSETS, KEPT)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import beam_ref as R
import sequence_beam_ref as BR
from conftest import ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces
from faceformer_amd.hip.modes import SEQUENCE_BEAM, sequence_beam_stop_value, sequence_beams_value      # (the option: without it nothing here can pass)

TOK = token_ns()
TERM = (TOK.EOS, TOK.EOS + 1)
NEG = -np.inf


# ---- CPU: the reference rule on hand-written rows ------------------------------------------------------------------------------------
def _row(S, **at):
    """A logit row that is -30 everywhere but at the given keys (k3=..., the key after the letter)."""
    row = np.full(S, -30.0)
    for k, v in at.items():
        row[int(k[1:])] = v
    return row


def _table_decode(table, G, W, T, stop):
    """BR.decode over a table of rows: table(prefix tuple) -> row [S]."""
    return BR.decode(lambda prefixes, j: np.stack([table(tuple(int(v) for v in p)) for p in prefixes]), G, W, T, TOK.SOS, TOK.EOS, stop)


def test_rule_sep_in_every_beam_does_not_stop():
    S, W, T = 8, 2, 5
    # step 0: edges 4 and 5; step 1: BOTH beams select SEP (the parallel rule's counter -- tokens >= num_token -- would be 0 here);
    # then edges to the end: no EOS, T - 1 steps
    def table(p):
        if len(p) == 1:
            return _row(S, k4=2.0, k5=1.0)
        if len(p) == 2:
            return _row(S, k2=5.0)
        return _row(S, k6=2.0, k7=1.0)
    for stop in BR.STOPS:
        res = _table_decode(table, 1, W, T, stop)
        assert res["steps"] == T - 1 and res["counts"][1] > 0, stop
        assert (res["beams"][:, 2] == TOK.SEP).all() and not res["fin"].any()
        assert res["all_counts"] == [2, 2, 2, 2] and res["best_counts"] == [1, 1, 1, 1]


def test_rule_eos_at_beam_dependent_steps_and_best_stops_before_all():
    S, W, T = 8, 2, 8
    # beam A = (SOS, 4, ...) takes EOS at step 1 with probability ~1; beam B = (SOS, 5, ...) walks edges 6, 6 and takes EOS at step 3
    def table(p):
        if len(p) == 1:
            return _row(S, k4=1.0, k5=0.0)
        if p[1] == 4:
            return _row(S, k3=9.0)
        return _row(S, k3=9.0) if len(p) == 4 else _row(S, k6=9.0)
    al = _table_decode(table, 1, W, T, "all")
    be = _table_decode(table, 1, W, T, "best")
    assert be["steps"] == 2 and al["steps"] == 4 and be["steps"] < al["steps"]
    assert al["all_counts"] == [2, 1, 1, 0] and al["best_counts"][:2] == [1, 0]
    assert al["beams"][0, :3].tolist() == [TOK.SOS, 4, TOK.EOS] and (al["beams"][0, 3:] == 0).all()      # zero past the beam's EOS
    assert al["beams"][1, :5].tolist() == [TOK.SOS, 5, 6, 6, TOK.EOS] and al["fin"].all()
    assert BR.finish_of(al["beams"], TOK.EOS).tolist() == [2, 4]
    # "best": beam 0 and its score are the "all" decode's; beam 1 is returned as it stands, unfinished, zero past the stop step
    assert np.array_equal(be["beams"][0], al["beams"][0]) and be["scores"][0] == al["scores"][0]
    assert be["fin"].tolist() == [True, False] and be["beams"][1].tolist() == [TOK.SOS, 5, 6, 0, 0, 0, 0, 0]
    assert BR.stop_step(al["best_counts"], T) == be["steps"] and BR.stop_step(al["all_counts"], T) == al["steps"]


def test_rule_finished_rank_0_keeps_rank_0_on_an_exact_tie():
    S, W = 4, 2
    # beam 0 finished with score -1; beam 1 unfinished with score -1 and a row whose best log-probability is EXACTLY 0 (one live key)
    masked = np.stack([np.zeros(S), np.array([-R.FLT_MAX, -R.FLT_MAX, 0.0, -R.FLT_MAX])])
    res = BR.step(masked, np.array([-1.0, -1.0]), np.array([True, False]), W, TOK.EOS)
    assert res["scores"].tolist() == [-1.0, -1.0]                          # an exact tie ...
    assert res["parent"].tolist() == [0, 1] and res["tok"].tolist() == [0, 2] and res["fin"].tolist() == [True, False]      # ... flat index 0 wins
    assert (res["all"], res["best"]) == (1, 0)
    # and with every beam finished or empty both counters are 0; an empty rank 0 counts as nothing
    assert BR.counters(np.array([-1.0, NEG, NEG, -2.0]), np.array([True, False, False, True]), 2) == (0, 0)
    assert BR.counters(np.array([-1.0, -2.0, -1.0, -2.0]), np.array([False, False, True, False]), 2) == (3, 1)
    sc, fin = BR.start(2, 3)
    assert sc.tolist() == [0.0, NEG, NEG, 0.0, NEG, NEG] and not fin.any()


def test_rule_in_fp32_rounded_arithmetic_selects_as_fp64_on_a_kept_case():
    c = BR.operator_case(65, 3, 5, "mixed", BR.op_seed(65, 3, 5, "mixed"))
    masked = BR.masked_of(c)
    ref = BR.step(masked, c["scores"], c["fin"], 3, TOK.EOS)
    par, tok = BR.step_fp32(masked, c["scores"], c["fin"], 3, TOK.EOS)
    assert (ref["gap"] > 1.0).all() and np.array_equal(par, ref["parent"]) and np.array_equal(tok, ref["tok"])


# ---- CPU: C ABI and binding --------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_beam_sequence_select", "ff_decode_sequence_beam_workspace_bytes", "ff_decode_sequence_beam")


def test_header_and_binding_declare_the_entries_within_abi_105():
    import re
    from faceformer_amd.hip import lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
        n_args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).count(",") + 1
        assert n_args == len(lib.SIGNATURES[name][1]), name
    doc = header[header.index("beam search over the single-sequence decode"): header.index("typedef struct ff_sequence_beam_params")]
    assert "model.py:161-167" in doc and "model.py:193-210" in doc and "model.py:191" in doc      # the reference call sites
    fields = re.search(r"typedef struct ff_sequence_beam_params \{(.*?)\}", code, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == [n for n, _ in lib.SequenceBeamParams._fields_]
    # the existing entries keep their signatures
    assert len(lib.SIGNATURES["ff_beam_select"][1]) == 26 and len(lib.SIGNATURES["ff_decode_beam"][1]) == 20
    assert [n for n, _ in lib.BeamParams._fields_] == ["width", "beams", "scores", "trace_parent"]


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


# ---- CPU: every refusal ------------------------------------------------------------------------------------------------------------
def test_mode_record_lies_outside_the_mode_table():
    from faceformer_amd.hip import modes
    assert modes.SEQUENCE_BEAM is SEQUENCE_BEAM and SEQUENCE_BEAM not in modes.MODES and "sequence_beams" not in modes.SWITCH
    assert [sequence_beams_value(v) for v in (None, 0, 1, 8)] == [0, 0, 1, 8]
    assert [sequence_beam_stop_value(v) for v in ("all", "best")] == [0, 1]
    assert SEQUENCE_BEAM.entry == "ff_decode_sequence_beam" and not SEQUENCE_BEAM.term_range and not SEQUENCE_BEAM.parallel_only
    assert SEQUENCE_BEAM.per_anchor
    assert modes.SWITCH["beam_width"] is modes.BEAM.switches[0] and modes.BEAM.entry == "ff_decode_beam"      # the recorded mode stays


def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes = {}
    memory = torch.zeros(2, 12, 64)
    ok = dict(T=5, F=1, sequence_beams=3)
    with pytest.raises(ValueError, match="sequence_beams is a single-sequence option .* beam_width"):
        eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=2),
                   dict(constrain="no_repeat"), dict(constrain=0), dict(sequence_samples=2, uniforms=torch.zeros(4, 4))):
        with pytest.raises(ValueError, match="sequence_beams excludes"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    with pytest.raises(ValueError, match="sequence_beams excludes stop_each_eos"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, flags=engine.DEFAULT_FLAGS | lib.FF_STOP_EACH_EOS, **ok)
    for bad in (9, -1, True, 2.0, 13):
        with pytest.raises(ValueError, match="sequence_beams=.*must be in 1..8 and at most S"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_beams=bad))
    with pytest.raises(ValueError, match="sequence_beams=6: must be in 1..8 and at most S = 5"):
        eng.decode(torch.zeros(2, 5, 64), None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_beams=6))
    for bad in ("first", None, 1, "ALL"):
        with pytest.raises(ValueError, match="sequence_beam_stop=.*must be 'all' or 'best'"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_beam_stop=bad))
    # the recorded rejections of beam_width on the single-sequence variant stay what they are
    with pytest.raises(ValueError, match="beam_width is a parallel-variant option"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, T=5, F=1, beam_width=2, term_range=(1, 4))


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
    assert par.sequence_beams == 0 and par.sequence_beam_stop == "all"
    par.sequence_beams = 2
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_beams is a SurfaceFormer option .* beam_width"):
        par.forward_eval(inputs)
    assert "predict" not in inputs
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.sequence_beams == 0 and seq.sequence_beam_stop == "all"
    seq.sequence_beams = 2
    text = "sequence_beams excludes sequence_samples, beam_width, return_logprob and an extra mask"
    seq.return_logprob = True
    with torch.no_grad(), pytest.raises(ValueError, match=text):
        seq.forward_eval(_seq_inputs())
    seq.return_logprob = False
    with torch.no_grad(), pytest.raises(ValueError, match=text):
        seq.forward_eval(_seq_inputs(extra_mask=torch.zeros(1, 8, dtype=torch.bool)))
    seq.sequence_samples = 2
    with torch.no_grad(), pytest.raises(ValueError, match=text):
        seq.forward_eval(_seq_inputs())
    seq.sequence_samples = 0
    seq.beam_width = 2                                                      # (alone, this model does not read beam_width)
    with torch.no_grad(), pytest.raises(ValueError, match=text):
        seq.forward_eval(_seq_inputs())
    seq.beam_width = 0
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_beams"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    for attr, val, msg in (("sequence_beams", 9, "sequence_beams=9: must be in 1..8 and at most S"), ("sequence_beams", -3, "must be in 1..8"),
                           ("sequence_beams", True, "must be in 1..8"), ("sequence_beam_stop", "first", "sequence_beam_stop='first': must be 'all' or 'best'")):
        old = getattr(seq, attr)
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match=msg):
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, old)
    seq.sequence_beams = 8                                                  # above S = 0 edges + 4 tokens
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_beams=8: must be in 1..8 and at most S = 4"):
        seq.forward_eval({"input": torch.zeros(1, 0, 50, 2), "input_mask": torch.zeros(1, 0, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})
    seq.sequence_beams = 2
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_beams = 2
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_beams needs the native engine"):
            sub.forward_eval(_seq_inputs())
    # the recorded rejections on this model stay, with or without the new option
    for W in (0, 2):
        seq.sequence_beams = W
        seq.num_samples = 2
        with torch.no_grad(), pytest.raises(ValueError, match="num_samples is a SurfaceFormer_Parallel option"):
            seq.forward_eval(_seq_inputs())
        seq.num_samples = 0
        seq.retire_finished = True
        with torch.no_grad(), pytest.raises(ValueError, match="retire_finished"):
            seq.forward_eval(_seq_inputs())
        seq.retire_finished = False
        seq.constrain = "loops"
        with torch.no_grad(), pytest.raises(ValueError, match="constrain"):
            seq.forward_eval(_seq_inputs())
        seq.constrain = None


def test_decode_sharded_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, sequence_beams=2)
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_beams"):
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_beams = 0
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: faces and the CLI ---------------------------------------------------------------------------------------------------------
def test_faces_of_the_beams_on_hand_written_rows():
    assert "parse_faces_beams_scored" in faces.__all__
    E = TOK.len      # edge e is token E + e
    beams = np.array([[1, E + 0, E + 1, 2, E + 2, E + 3, 3, 0, 0, 0],              # finished: {0,1}, {2,3}
                      [1, E + 1, E + 0, 2, 2, E + 4, E + 5, 3, 0, 0],              # finished: {0,1} again (worse score), an empty piece, {4,5}
                      [1, E + 2, E + 3, 2, E + 6, E + 7, E + 1, 0, 0, 0],          # UNFINISHED, stopped after 6 steps: {2,3} (better score), {6,7}: the open piece loses its last edge
                      [1, E + 8, E + 9, 3, 0, 0, 0, 0, 0, 0]])                     # empty rank: skipped whatever its row holds
    scores = np.array([-1.0, -2.0, -0.5, NEG])
    fin = np.array([1, 1, 0, 0])
    got = faces.parse_faces_beams_scored(beams, scores, fin, 8, TOK)
    assert got == [(0, (0, 1), -1.0), (0, (2, 3), -0.5), (0, (4, 5), -2.0), (0, (6, 7), -0.5)]      # once each, first place, best score
    uniq = faces.unique_faces_with_scores(got)
    assert [(f[1], f[2], f[3]) for f in uniq] == [((0, 1), -1.0, 1), ((2, 3), -0.5, 1), ((4, 5), -2.0, 1), ((6, 7), -0.5, 1)]
    # per beam it is this model's own parse
    assert faces.parse_faces(beams[0], beams[0], 8, TOK)[0] == [(0, (0, 1)), (0, (2, 3))]
    # the finished flag decides how a row without EOS is read: as finished, the zeros are tokens and the piece loses a zero instead
    as_fin = faces.parse_faces_beams_scored(beams[2:3], scores[2:3], np.array([1]), 8, TOK)
    assert as_fin == [(0, (2, 3), -0.5), (0, (6, 7, 1), -0.5)]
    assert faces.parse_faces_beams_scored(beams[3:], scores[3:], fin[3:], 8, TOK) == []
    with pytest.raises(ValueError):
        faces.parse_faces_beams_scored(beams, scores[:2], fin, 8, TOK)
    with pytest.raises(ValueError):
        faces.parse_faces_beams_scored(beams[0], scores, fin, 8, TOK)


def test_cli_flags_reach_the_model_and_every_refusal_raises(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-beams", "4", "--sequence-beam-stop", "best"])
    assert (a.sequence_beams, a.sequence_beam_stop, a.beam, a.sequence_samples) == (4, "best", 0, 0)
    d = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"])
    assert (d.sequence_beams, d.sequence_beam_stop) == (0, "all")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-beams", "4", "--sequence-beam-stop", "first"])
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-beams", "4", "--sequence-beam-stop", "best", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["sequence_beams"], kw["sequence_beam_stop"], kw["beam"]) for kw in seen] == [(4, "best", 0), (0, "all", 0)]
    m = cli.configure_model(types.SimpleNamespace(), sequence_beams=4, sequence_beam_stop="best")
    assert vars(m) == dict(sequence_beams=4, sequence_beam_stop="best")
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    seqcfg = types.SimpleNamespace(model_class="SurfaceFormer")
    call = dict(out_dir="unused", device="cpu", model=object())
    with pytest.raises(ValueError, match="--sequence-beams applies to SurfaceFormer only .*--beam"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer_Parallel"), None, sequence_beams=2, **call)
    for bad in (9, -1, True):
        with pytest.raises(ValueError, match="--sequence-beams must be a width in 1..8"):
            run_test(seqcfg, None, sequence_beams=bad, **call)
    with pytest.raises(ValueError, match="--sequence-beam-stop must be all or best"):
        run_test(seqcfg, None, sequence_beams=2, sequence_beam_stop="first", **call)
    for kw in (dict(scores=True), dict(score_labels=True), dict(sample=2), dict(sequence_samples=2), dict(beam=2), dict(device_faces=True)):
        with pytest.raises(ValueError, match="--sequence-beams does not combine with --scores, --score-labels, --sample, --sequence-samples, "
                                             "--beam or --device-faces"):
            run_test(seqcfg, None, sequence_beams=2, **dict(call, **kw))
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sequence-beams is not implemented for multi-rank runs"):
        run_test(seqcfg, None, sequence_beams=2, dist_mod=world2, **call)
    with pytest.raises(ValueError, match="--sequence-samples applies to SurfaceFormer only"):      # an existing text, unchanged
        run_test(types.SimpleNamespace(model_class="SurfaceFormer_Parallel"), None, sequence_samples=2, **call)


def test_record_gains_the_two_keys_and_is_todays_without_them(tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd import datasets as D
    E = TOK.len
    cfgm = types.SimpleNamespace(num_points_per_line=50, num_lines=16, point_dim=2, label_seq_length=24, token=TOK)
    cfg = types.SimpleNamespace(model=cfgm, post_process=types.SimpleNamespace(is_coedge=False, enclosedness_tol=1e-4))
    rng = np.random.default_rng(3)
    raw = {"edges": [rng.uniform(-1, 1, size=(2, 2)).tolist() for _ in range(8)], "faces_indices": [[[0, 1, 2]], [[3, 4, 5]]],
           "pairings": {}, "dominant_directions": [[1, 0, 0]]}
    (tmp_path / "json").mkdir()
    json.dump(raw, open(str(tmp_path / "json" / "a.json"), "w"))
    open(str(tmp_path / "t.txt"), "w").write("json/a.json\n")
    item = D.ABCDataset(str(tmp_path), ["t.txt"], cfgm)[0]
    beams = np.zeros((3, 24), dtype=np.int64)
    beams[0, :8] = [1, E + 0, E + 1, E + 2, 2, E + 3, E + 4, 3]
    beams[1, :5] = [1, E + 2, E + 1, E + 0, 3]
    beams[2, :7] = [1, E + 5, E + 6, 2, E + 5, E + 6, E + 7]           # unfinished
    sc, fin = np.array([-0.5, -1.5, -2.5]), np.array([1, 1, 0], dtype=np.int32)
    text, st = cli.record_of(cfg, raw, item, beams[0], False)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
    text2, st2 = cli.record_of(cfg, raw, item, beams[0], False, sequence_beams=(beams, sc, fin))
    rec2 = json.loads(text2)
    assert list(rec2) == list(rec) + ["pred_beam_faces", "pred_beam_face_scores"] and st2 == st
    assert {k: rec2[k] for k in rec} == rec and text == cli.record_of(cfg, raw, item, beams[0], False, sequence_beams=None)[0]      # byte-identical
    assert rec2["pred_beam_face_scores"] == [-0.5, -0.5, -2.5] and len(rec2["pred_beam_faces"]) == 3      # {0,1,2} {3,4} {5,6}


# ---- GPU: the operator (sequence forms of the selection step) -----------------------------------------------------------------------
E_OP = 64


def _run_operator(c, memory, stop_best):
    from faceformer_amd.hip import ops
    dev = "cuda"
    logits = torch.from_numpy(c["logits"]).float().to(dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.beam_sequence_select(logits, torch.from_numpy(c["scores"]).float().to(dev), torch.from_numpy(c["fin"].astype(np.int32)).to(dev),
                                   c["W"], groups_per_wireframe=1, mask=torch.from_numpy(c["mask"].astype(np.uint8)).to(dev),
                                   kv_len=torch.from_numpy(c["kv"]).to(dev), term_range=TERM, memory=memory, want_rows=True,
                                   counter=counter, stop_best=stop_best)
    out = dict(out, logits=logits, count=counter)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S,W,G", [(S, W, G) for S in BR.OP_S for W in BR.OP_W for G in BR.OP_G if W <= S])      # (W > S is refused)
def test_operator_sequence_forms_against_the_numpy_rule(hip_lib, S, W, G):
    from faceformer_amd.hip import ops
    seen = left = 0
    for state in BR.OP_STATES:
        c = BR.operator_case(S, W, G, state, BR.op_seed(S, W, G, state))
        masked = BR.masked_of(c)
        ref = BR.step(masked, c["scores"], c["fin"], W, TOK.EOS)
        memory = torch.randn(G, S, E_OP, generator=torch.Generator().manual_seed(S + W)).cuda()
        what = (S, W, G, state)
        ok = np.repeat(ref["gap"] > 1.0, W)
        seen, left = seen + G, left + int((ref["gap"] <= 1.0).sum())
        for stop_best in (False, True):
            got = _run_operator(c, memory, stop_best)
            par, tok, fin = (got[k].cpu().numpy() for k in ("parent", "next", "fin"))
            assert np.array_equal(par[ok], ref["parent"][ok]) and np.array_equal(tok[ok], ref["tok"][ok]), what
            assert np.array_equal(fin[ok] != 0, ref["fin"][ok]), what
            sc = got["scores"].cpu().numpy().astype(np.float64)
            live = ok & np.isfinite(ref["scores"])
            assert np.array_equal(np.isneginf(sc[ok]), ~np.isfinite(ref["scores"][ok])) and not np.isnan(sc).any(), what
            err = np.abs(sc[live] - ref["scores"][live])
            assert (err <= np.array([R.score_bound(v) for v in ref["scores"][live]])).all(), (what, err.max() if err.size else 0.0)
            # the next rows: the greedy launch's own gather of memory[g, tok]
            assert torch.equal(got["rows"], ops.gather_rows(memory, got["next"], seqs_per_group=W)), what
            # the rows of non-empty unfinished beams were masked in place; the others were not touched
            read = np.isfinite(c["scores"]) & ~c["fin"]
            lg = got["logits"].cpu().numpy().astype(np.float64)
            assert np.array_equal(lg[read], masked[read]) and np.array_equal(lg[~read], c["logits"][~read]), what
            # the counter of the form, from the kernel's OWN state after the step (equal to the rule's where nothing is left out)
            want_all, want_best = BR.counters(sc, fin != 0, W)
            assert int(got["count"].item()) == (want_best if stop_best else want_all), (what, stop_best)
            if ok.all():
                assert int(got["count"].item()) == (ref["best"] if stop_best else ref["all"]), (what, stop_best)
            again = _run_operator(c, memory, stop_best)
            assert all(torch.equal(got[k], again[k]) for k in got), what                 # two launches: bit-equal
        if ok.all():
            if state == "start":
                assert (ref["parent"] == 0).all() and ref["all"] + int(ref["fin"].sum()) == G * W      # W candidates of beam 0 (W <= S)
            if state == "done":
                assert ref["all"] == 0 and ref["best"] == 0 and (ref["tok"] == 0).all()
            if state == "eos":
                assert (ref["tok"] == TOK.EOS).all() and ref["fin"].all() and ref["all"] == 0 and ref["best"] == 0
            if state == "sep":
                assert (ref["tok"].reshape(G, W)[:, 0] == TOK.SEP).all() and ref["best"] == G and ref["all"] == G * W and not ref["fin"].any()
    print("S=%d W=%d G=%d: %d of %d groups left out" % (S, W, G, left, seen))
    assert left <= BR.CAP * seen, (S, W, G, left, seen)


@pytest.mark.gpu
def test_operator_refuses_bad_arguments(hip_lib):
    from faceformer_amd.hip import lib as L, ops
    lg = torch.zeros(4, 8).cuda()
    sc, fin = torch.zeros(4).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="term_range"):
        ops.beam_sequence_select(lg, sc, fin, 2, term_range=(3, 3))
    with pytest.raises(ValueError, match="beam width"):
        ops.beam_sequence_select(lg, sc, fin, 9)
    p = lambda t: t.data_ptr()
    out = [torch.zeros(4).cuda(), torch.zeros(4, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int32).cuda()]
    rc = L.load().ff_beam_sequence_select(p(lg), 8, 8, None, None, 2, 2, 2, p(sc), p(out[0]), p(fin), p(out[1]), None, 0, 0, p(out[2]), p(out[3]),
                                          3, 4, None, 0, None, 0, None, 2, None)
    assert rc != 0 and b"stop_best=2 must be 0 or 1" in L.load().ff_last_error()      # FF_ERR_ARG, before any launch


# ---- GPU: the engine ----------------------------------------------------------------------------------------------------------------
_MODELS = {}
SMALL = ["seq_small_gain4", "seq_small_eos", "seq_small_repeat_eos"]


def _model(name):
    if name not in _MODELS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        _MODELS[name] = (case, z, build_model(case, sd, "cuda"), batch_to(batch, "cuda"), sd, batch)
    return _MODELS[name]


def _decode(model, case, batch, **kw):
    from test_logprob import _decode as decode
    return decode(model, case, batch, **kw)


_RUNS = {}


def _beams(name, W, stop="all", **kw):
    """One traced decode per (golden, W, stop): computed once, shared by the tests that need it, left unchanged."""
    key = (name, W, stop) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        case, z, model, b, sd, batch = _model(name)
        _RUNS[key] = _decode(model, case, b, sequence_beams=W, sequence_beam_stop=stop, return_pointer=False, trace=True, **kw)
    return _RUNS[key]


def _check_layout(out, T, W, stop):
    """The outputs' own consistency: shapes and dtypes, SOS, the finished flags, the zero padding and what `steps` may be, against
    the rule applied to the decode's own tokens.  Returns (beams, scores fp64, finished bool, finish positions, steps)."""
    beams = out["beams"].cpu().numpy()
    sc = out["beam_scores"].cpu().numpy()
    fin = out["beam_finished"].cpu().numpy()
    steps = out["steps"]
    assert beams.dtype == np.int64 and sc.dtype == np.float32 and fin.dtype == np.int32 and beams.shape == (sc.size, T) and fin.shape == sc.shape
    assert (beams[:, 0] == TOK.SOS).all() and 1 <= steps <= T - 1 and len(out["step_counts"]) == steps
    live = np.isfinite(sc)
    assert not np.isnan(sc).any() and (sc[live] <= 0).all() and live.reshape(-1, W)[:, 0].all() and not (fin[~live] != 0).any()
    pos = BR.finish_of(beams, TOK.EOS)
    assert np.array_equal(fin[live] != 0, pos[live] <= steps)                                  # finished = an EOS at a position <= steps
    past = np.arange(T)[None, :] > np.minimum(pos, steps)[:, None]
    assert (beams[past] == 0).all()                                                            # zero past each beam's EOS and past steps
    gs = np.where(live, sc.astype(np.float64), -1e300).reshape(-1, W)
    assert (np.diff(gs, axis=1) <= 0).all()                                                    # best first
    unfinished = live & (fin == 0)
    if stop == "all":
        assert steps == T - 1 or not unfinished.any()
        assert out["step_counts"][-1] == int(unfinished.sum()) and all(v > 0 for v in out["step_counts"][:-1])
    else:
        first = unfinished.reshape(-1, W)[:, 0]
        assert steps == T - 1 or not first.any()
        assert out["step_counts"][-1] == int(first.sum()) and all(v > 0 for v in out["step_counts"][:-1])
    assert torch.equal(out["predict"], out["beams"].view(-1, W, T)[:, 0])
    return beams, sc.astype(np.float64), fin != 0, pos, steps


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_with_one_beam_is_the_greedy_decode_cut_at_every_eos(hip_lib, name):
    from faceformer_amd.hip import lib as L
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    greedy = _decode(model, case, b, logprob=True, flags=model.decode_flags | L.FF_STOP_EACH_EOS)
    pred = greedy["predict"].cpu().numpy()
    want = np.stack([faces.apply_own_stop_rule(pred[w], TOK, parallel=False) for w in range(pred.shape[0])])
    glp = np.stack([faces._apply_own_stop_rule_scored(pred[w], greedy["logprob"][w].cpu().numpy(), TOK, False)[1] for w in range(pred.shape[0])])
    for stop in BR.STOPS:
        out = _beams(name, 1, stop)
        assert out["steps"] == greedy["steps"], (name, stop, out["steps"], greedy["steps"])
        assert np.array_equal(out["beams"].cpu().numpy(), want), (name, stop)                  # token for token
        _check_layout(out, T, 1, stop)
        err = np.abs(out["beam_scores"].cpu().numpy().astype(np.float64) - glp.astype(np.float64).sum(axis=1)).max()
        print(name, stop, "steps=%d max |score - sum of greedy logprob| = %.3g" % (out["steps"], err))
        assert err <= (T - 1) * R.LP_BAR, (name, stop, err)


def _replay(out, W, T, stop, what):
    """The fp64 rule on the decode's own traced logits, step by step, from the rule's own carried state (section 13's scheme: j
    bounds at step j, a group leaves the comparison at its first indecisive step).  Returns (replayed beams, scores, finished,
    per-step counters of `stop`, still-compared mask per beam, left-out share of the (step, group) pairs)."""
    steps = out["steps"]
    B = out["beams"].shape[0]
    G = B // W
    logits = out["logits"].cpu().numpy().astype(np.float64)
    par = out["beam_parent"].cpu().numpy()
    scores, fin = BR.start(G, W)
    ok = np.ones(G, dtype=bool)
    toks, counts, left = [], [], 0
    for j in range(steps):
        lg = np.where(np.isnan(logits[j]), 0.0, logits[j])                  # (rows of empty / finished beams: not read by the rule)
        res = BR.step(lg, scores, fin, W, TOK.EOS, margin=j + 1)
        ok &= res["gap"] > 1.0
        left += int((~ok).sum())
        okb = np.repeat(ok, W)
        assert np.array_equal(par[j][okb], res["parent"][okb]), (what, j)
        toks.append(res["tok"])
        counts.append(res[stop])
        scores, fin = res["scores"], res["fin"]
    replayed = np.zeros((B, T), dtype=np.int64)
    replayed[:, : steps + 1] = R.backtrack(np.full(B, TOK.SOS), toks, [par[j] for j in range(steps)], W)
    return replayed, scores, fin, counts, np.repeat(ok, W), left / max(1, steps * G)


def _check_replay(out, W, T, stop, what):
    beams, sc, fin, pos, steps = _check_layout(out, T, W, stop)
    replayed, rsc, rfin, counts, okb, left = _replay(out, W, T, stop, what)
    print(what, "steps=%d left-out (step, group) pairs: %.2f %%" % (steps, 100 * left))
    assert left <= BR.CAP, (what, left)
    assert np.array_equal(beams[okb], replayed[okb]), what
    assert np.array_equal(fin[okb], rfin[okb] & np.isfinite(rsc[okb])), what
    if okb.all():                                                           # steps and the counters are batch-wide
        assert out["step_counts"] == counts and BR.stop_step(counts, T) == steps, (what, out["step_counts"], counts)
    live = okb & np.isfinite(rsc)
    assert np.array_equal(np.isneginf(sc[okb]), np.isneginf(rsc[okb])), what
    err = np.abs(sc[live] - rsc[live])
    bound = steps * (R.LP_BAR + R.ADD_EPS * np.abs(rsc[live]))
    print(what, "max |score - replayed score| = %.3g" % (err.max() if err.size else 0.0))
    assert (err <= bound).all(), (what, float(err.max()))
    return okb


@pytest.mark.gpu
@pytest.mark.parametrize("name,W", BR.REPLAY)
def test_engine_beams_replay_under_the_numpy_rule(hip_lib, name, W):
    """The (golden, W) cases are sequence_beam_ref's: kept on the CPU by tools/sequence_beam_left_out.py, whose oracle also saw all
    three stop outcomes -- seq_small_eos stops at 4 / 12 / 19, seq_small_repeat_eos at 10 / 13 / 13 with every beam finished,
    seq_small_gain4 runs T - 1 steps with 2 / 4 beams finished."""
    left0, pairs, gap, steps_all, finished = BR.KEPT[(name, W)]
    assert left0 < BR.CAP * pairs, "not a kept case"
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    out = _beams(name, W)
    okb = _check_replay(out, W, T, "all", (name, W))
    if okb.all():       # nothing left out: the decode took the oracle's decisions (its smallest gap is `gap` bounds wide)
        assert out["steps"] == steps_all and int((out["beam_finished"] != 0).sum()) == finished, (name, W, out["steps"], steps_all)


@pytest.mark.gpu
@pytest.mark.parametrize("name,W", [("seq_small_gain4", 4), ("seq_small_eos", 4), ("seq_small_eos", 8), ("seq_small_repeat_eos", 4)])
def test_engine_best_stops_no_later_than_all_with_the_same_best_beam(hip_lib, name, W):
    case, z, model, b, sd, batch = _model(name)
    T, N = case["model"]["seq_len"], b["input"].size(0)
    al, be = _beams(name, W, "all"), _beams(name, W, "best")
    _check_replay(be, W, T, "best", (name, W, "best"))
    assert be["steps"] <= al["steps"]
    a0, b0 = al["beams"].view(N, W, T)[:, 0], be["beams"].view(N, W, T)[:, 0]
    if be["steps"] < T - 1:                                                  # every rank 0 finished: exact for the best beam
        assert torch.equal(a0, b0) and torch.equal(al["beam_scores"].view(N, W)[:, 0], be["beam_scores"].view(N, W)[:, 0])
        assert (be["beam_finished"].view(N, W)[:, 0] != 0).all()
    # steps_best is the first step after which every group's rank 0 is finished in the "all" decode's own records: replay them
    par = al["beam_parent"].cpu().numpy()
    logits = al["logits"].cpu().numpy().astype(np.float64)
    scores, fin = BR.start(N, W)
    first = T - 1
    for j in range(al["steps"]):
        res = BR.step(np.where(np.isnan(logits[j]), 0.0, logits[j]), scores, fin, W, TOK.EOS, margin=j + 1)
        assert (res["gap"] > 1.0).all() and np.array_equal(par[j], res["parent"])      # (kept cases: nothing is left out)
        scores, fin = res["scores"], res["fin"]
        if res["best"] == 0:
            first = j + 1
            break
    assert be["steps"] == min(first, T - 1), (name, W, be["steps"], first)
    print(name, "W=%d steps all %d best %d" % (W, al["steps"], be["steps"]))


@pytest.mark.gpu
def test_engine_rows_of_a_wireframe_share_its_memory_and_wireframes_differ(hip_lib):
    """Step 0: every beam holds SOS, so the traced rows that are read (beam 0's) are their wireframe's golden row -- a wrong
    row-to-wireframe map (i % N, or i / W of another W) shows here."""
    from test_parity_golden import _tol
    name, W = "seq_small_gain4", 4
    case, z, model, b, sd, batch = _model(name)
    out = _beams(name, W)
    lg = out["logits"][0].cpu().numpy().reshape(-1, W, out["logits"].shape[-1])      # [N, W, S]
    tol = _tol(z["logits"][0])
    for w in range(lg.shape[0]):
        live = lg[w, 0] > BR.FILL
        assert np.abs(lg[w, 0][live] - z["logits"][0][w][live]).max() <= tol, w
    both = (lg[0, 0] > BR.FILL) & (lg[1, 0] > BR.FILL)
    assert np.abs(lg[0, 0][both] - lg[1, 0][both]).max() > 100 * tol


@pytest.mark.gpu
def test_engine_micro_batch_cut_and_repeatability(hip_lib):
    name, W = "seq_small_gain4", 4
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    whole = _beams(name, W)
    again = _decode(model, case, b, sequence_beams=W, return_pointer=False, trace=True)
    for k in ("beams", "beam_scores", "beam_finished", "predict", "logits", "beam_parent"):
        assert torch.equal(whole[k], again[k]), k                                    # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"] and whole["step_counts"] == again["step_counts"]
    one = _beams(name, W, chunk_max_seqs=W)                                          # one wireframe per micro-batch
    assert len({int(v) // W for v in one["seq_of_row"].cpu()}) == b["input"].size(0)
    ow = _check_replay(whole, W, T, "all", "whole")
    oo = _check_replay(one, W, T, "all", "one")
    both = ow & oo
    a, c = whole["beams"].cpu().numpy(), one["beams"].cpu().numpy()
    assert np.array_equal(a[both], c[both])                                          # equal on groups decisive in both
    if both.all():
        assert whole["steps"] == one["steps"]
    asc, csc = (o["beam_scores"].cpu().numpy().astype(np.float64) for o in (whole, one))
    live = both & np.isfinite(asc)
    assert np.array_equal(np.isfinite(asc[both]), np.isfinite(csc[both]))
    # each decode is within steps * score_bound of its own replay, and the two replays differ by the logits' own re-evaluation:
    # 2 tol(step) per step (test_parity_golden._tol on the traced logits)
    from test_parity_golden import _tol
    logits = whole["logits"].cpu().numpy()
    n = min(whole["steps"], one["steps"])
    tol = sum(2 * _tol(np.where(np.isnan(logits[j]), 0.0, logits[j])) for j in range(n))
    bound = tol + 2 * max(whole["steps"], one["steps"]) * (R.LP_BAR + R.ADD_EPS * np.abs(asc[live]))
    print("groups compared: %d of %d; worst |dscore| / bound = %.3g" % (both.sum() // W, both.size // W, (np.abs(asc - csc)[live] / bound).max()))
    assert (np.abs(asc - csc)[live] <= bound).all()


def _against_oracle(name, case, sd, batch, beams, sc, steps, W, seqs=None, max_steps=None):
    from test_sequence_sample import _oracle_scores
    N = beams.shape[0] // W
    pos = BR.finish_of(beams, TOK.EOS)
    want, bound = _oracle_scores(case, sd, batch, beams, pos, steps, W, seqs=seqs, max_steps=max_steps)
    rows = list(range(N)) if seqs is None else list(seqs)
    got = sc.reshape(N, W)[rows]
    live = np.isfinite(got)
    assert live[:, 0].all()
    ratio = (np.abs(got - want)[live] / np.maximum(bound[live], 1e-300)).max()
    print(name, "W=%d steps=%d non-empty beams %d: worst |score - oracle| / bound = %.3f" % (W, steps, live.sum(), ratio))
    assert (np.abs(got - want)[live] <= bound[live]).all(), (name, got, want, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_scores_against_the_teacher_forced_oracle(hip_lib, name):
    case, z, model, b, sd, batch = _model(name)
    T, W = case["model"]["seq_len"], 4
    beams, sc, fin, pos, steps = _check_layout(_beams(name, W), T, W, "all")
    _against_oracle(name, case, sd, batch, beams, sc, steps, W)


@pytest.mark.gpu
def test_engine_scores_on_the_full_size_model_against_the_oracle(hip_lib):
    """seq_full_A4_gain4 at W = 4; the oracle side restricted to two wireframes and 24 steps (seqs= / steps=).  The beams give no
    per-position log-probabilities, so the engine's side is a decode of T = 25 positions -- the first 24 steps of any longer
    decode, a step reading its prefix only -- whose scores are the sums over exactly those steps."""
    from faceformer_amd.hip import lib as L
    name = "seq_full_A4_gain4"
    case, z, model, b, sd, batch = _model(name)
    T, W, seqs, first = case["model"]["seq_len"], 4, [0, 3], 24
    eng, memory, mask, kv_len = model._encode(b)
    out = eng.decode(memory, mask, kv_len, L.FF_SEQ2SEQ, T=first + 1, F=1, sync_every=1, flags=model.decode_flags,
                     x3_min_rows=model.x3_min_rows, chunk_wireframes=model.chunk_wireframes, chunk_max_seqs=model.chunk_max_seqs,
                     sequence_beams=W)
    short, sc, fin, pos, steps = _check_layout(out, first + 1, W, "all")
    beams = np.zeros((short.shape[0], T), dtype=np.int64)
    beams[:, : first + 1] = short
    _against_oracle(name, case, sd, batch, beams, sc, steps, W, seqs=seqs, max_steps=first)
    del _MODELS[name]


# ---- GPU: the model and the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_sequence_beams_adds_the_keys(hip_lib):
    case, z, model, b, sd, batch = _model("seq_small_gain4")
    T, N, W = case["model"]["seq_len"], b["input"].size(0), 3
    try:
        with torch.no_grad():
            off = model(dict(b))
            model.sequence_beams = W
            on = model(dict(b))
            model.stop_each_eos = True                                # not looked at
            again = model(dict(b))
            model.stop_each_eos = False
            model.sequence_beam_stop = "best"
            best = model(dict(b))
            model.sequence_beams, model.sequence_beam_stop = 1, "all"
            one = model(dict(b))
    finally:
        model.sequence_beams, model.sequence_beam_stop, model.stop_each_eos = 0, "all", False
    new = {"predict_beams", "predict_beam_scores", "predict_beam_finished"}
    assert set(on) == (set(off) - {"pointer"}) | new and not new & set(off)          # pointer is not published
    assert np.array_equal(off["predict"].cpu().numpy(), z["predict"])                 # off: today's decode
    bm, sc, fin = (on[k] for k in ("predict_beams", "predict_beam_scores", "predict_beam_finished"))
    assert tuple(bm.shape) == (N, W, T) and bm.dtype == torch.int64 and tuple(sc.shape) == tuple(fin.shape) == (N, W)
    assert sc.dtype == torch.float32 and fin.dtype == torch.int32 and tuple(on["predict"].shape) == (N, T)
    assert torch.equal(on["predict"], bm[:, 0]) and torch.equal(on["embedding"], off["embedding"])
    for k in new | {"predict"}:
        assert torch.equal(on[k], again[k]), k
    assert set(best) == set(on) and torch.equal(best["predict"], best["predict_beams"][:, 0])
    # W = 1: the greedy row cut at its EOS (when the greedy decode ran as far)
    want = np.stack([faces.apply_own_stop_rule(r, TOK, parallel=False) for r in z["predict"]])
    if int(z["steps"]) >= model.last_beam_stats["steps"]:
        assert np.array_equal(one["predict_beams"].cpu().numpy()[:, 0], want)


@pytest.mark.gpu
def test_cli_records_with_and_without_the_flag(hip_lib, tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    root = tmp_path / "data"
    (root / "json").mkdir(parents=True)
    rng = np.random.default_rng(21)
    names = []
    for i in range(2):
        raw = {"edges": [rng.uniform(-1, 1, size=(2, 2)).tolist() for _ in range(6 + 3 * i)],
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
    one = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "one"), sequence_beams=1)
    wide = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "wide"), sequence_beams=4, sequence_beam_stop="best", batch_size=2)
    new = ["pred_beam_faces", "pred_beam_face_scores"]
    for fn in sorted(os.listdir(plain)):
        text = open(os.path.join(plain, fn)).read()
        rec = json.loads(text)
        assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
        r1, rw = (json.load(open(os.path.join(d, fn))) for d in (one, wide))
        assert list(r1) == list(rec) + new and list(rw) == list(rec) + new
        assert {k: r1[k] for k in rec} == rec                         # W = 1: beam 0 is the greedy decode
        assert len(r1["pred_beam_faces"]) == len(rec["pred_faces"]) and len(set(r1["pred_beam_face_scores"])) <= 1
        assert rw["pred_beam_face_scores"] == sorted(rw["pred_beam_face_scores"], reverse=True)
        assert len(rw["pred_beam_faces"]) == len(rw["pred_beam_face_scores"])
    again = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "again"))      # without the flag: byte-identical records
    for fn in sorted(os.listdir(plain)):
        assert open(os.path.join(plain, fn), "rb").read() == open(os.path.join(again, fn), "rb").read()
