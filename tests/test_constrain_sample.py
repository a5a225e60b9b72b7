"""Opt-in sampling over the loop-constrained pointer decode (model.constrain_samples): the C ABI, the bindings and
every rejected combination on the CPU; ff_pointer_constrained_sample and the engine's constrained sampled mode against the numpy
rule (tests/constrain_sample_ref.py, which composes constrain_ref / lookahead_ref / exact_ref with sample_ref) on the GPU.

Bars (the issue's, none measured): the byte row, the dead-end bit, the next (first, prev), the visited words and the finished
flag are exact; a token must equal the fp64 rule's on every DECISIVE row (sample_ref's guard band); log-probabilities within
2^-16 + 2^-23 |logprob| of fp64 on the kernel's own masked logits; at most 2 % (sample_ref.CAP) of a case's rows / pairs may be
indecisive; at least constrain_ref.MIN_ENCLOSED of the own-anchor draws end enclosed in the guarantee test.  The seeds and the
(golden, form, parameter set) combinations are fixed on the CPU by tools/constrain_sample_left_out.py."""
import json
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
import constrain_sample_ref as CSR
import sample_ref as SR
from conftest import ROOT, token_ns
from faceformer_amd import faces
from test_sample import PARAMS

TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
NTOK = TOK.len
FILL = SR.FILL
LOOPS = CSR.LOOPS
FORMS = CSR.FORMS
LOOKAHEAD = {"plain": None, "ahead": "ahead", "exact": "exact"}


# ---- CPU: C ABI and binding -------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_pointer_constrained_sample", "ff_decode_constrained_sample_workspace_bytes", "ff_decode_constrained_sample")
PARAM_FIELDS = ["num_samples", "temperature", "top_k", "top_p", "uniforms", "flags", "follows", "lookahead", "close_dist", "cycle_len",
                "samples", "logprob", "scores", "dead_end", "predict_logprob", "predict_dead_end"]


def test_header_declares_the_entries_and_states_the_contract():
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    doc = header[header.index("sampling over the loop-constrained pointer decode"): header.index("int ff_pointer_constrained_sample(")]
    for phrase in ("Draw k of anchor f of", "sequence (w*F + f)*R + k", "Top-k and top-p therefore act on the constrained row",
                   "clamped into [0, 1 - 2^-24]", "saturated at -FLT_MAX", "Padding-anchor groups are finished at 0",
                   "(a) tau = 0", "(b) Both flag bits clear", "(c) Draw k of an R-wide decode"):
        assert phrase in doc, phrase
    body = re.search(r"typedef struct ff_constrain_sample_params \{(.*?)\} ff_constrain_sample_params;", code, flags=re.S).group(1)
    assert [re.split(r"[\s*]+", f.strip())[-1] for f in body.split(";") if f.strip()] == PARAM_FIELDS

    def args(name):
        return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert args("ff_decode_constrained_sample").count(",") == args("ff_decode").count(",") + 1
    assert args("ff_decode_constrained_sample_workspace_bytes").count(",") == args("ff_decode_sample_workspace_bytes").count(",")
    # ff_pointer_constrained's arguments, ff_pointer_sample's six, the selector with its three operands
    assert args("ff_pointer_constrained_sample").count(",") == args("ff_pointer_constrained").count(",") + 10
    for existing in ("ff_sample_params", "ff_constrain_params", "ff_constrain_ahead_params", "ff_constrain_exact_params"):
        assert "} %s;" % existing in code                                 # (the existing structs stand as they did: their own tests pin the fields)


def test_binding_lists_the_entries_and_refuses_a_library_without_them(monkeypatch):
    from faceformer_amd.hip import lib
    S = lib.SIGNATURES
    for name in NEW_ENTRIES:
        assert name in S, name
    assert len(S["ff_decode_constrained_sample"][1]) == len(S["ff_decode"][1]) + 1
    assert len(S["ff_pointer_constrained_sample"][1]) == len(S["ff_pointer_constrained"][1]) + 10
    assert [f for f, _ in lib.ConstrainSampleParams._fields_] == PARAM_FIELDS
    import _ctypes
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


def test_the_source_is_built():
    from faceformer_amd.hip import build
    assert "ff_constrain_sample.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain_sample.hip"))


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


def test_of_options_returns_the_record():
    from faceformer_amd.hip import modes
    assert modes.CONSTRAIN_SAMPLE not in modes.MODES and modes.CONSTRAIN_SAMPLE.per_anchor
    assert modes.CONSTRAIN_SAMPLE.subject == "constrain_samples" and modes.CONSTRAIN_SAMPLE.entry == "ff_decode_constrained_sample"
    assert [k for k, _, _ in modes.CONSTRAIN_SAMPLE.outs][:4] == ["samples", "sample_logprob", "sample_scores", "sample_dead_end"]
    assert [n for n, _ in modes.CONSTRAIN_SAMPLE.own] == ["follow_table", "uniforms", "close_dist", "cycle_len"]
    for la, ex in ((False, False), (True, False), (False, True)):
        assert modes.of_options(False, 0, la, ex, 4, constrain=3, num_samples=0, beam_width=0) == (modes.CONSTRAIN_SAMPLE, 4)
    assert modes.of_options(constrain_samples=2, constrain=1, num_samples=0, beam_width=0) == (modes.CONSTRAIN_SAMPLE, 2)
    # existing positional calls keep working, and without the option the records are the ones they were
    assert modes.of_options(False, 0, False, False, constrain=3, num_samples=0, beam_width=0) == (modes.CONSTRAIN, 3)
    assert modes.of_options(False, 2, False, False, constrain=3, num_samples=0, beam_width=0) == (modes.CONSTRAIN_BEAM, 2)
    assert modes.of_options(False, 0, True, False, 0, constrain=3, num_samples=0, beam_width=0) == (modes.CONSTRAIN_AHEAD, 3)
    assert modes.of_options(False, 0, False, False, 0, constrain=None, num_samples=4, beam_width=0) == (modes.SAMPLE, 4)
    assert modes.constrain_samples_value(None, None) == 0 and modes.constrain_samples_value(0, 3) == 0
    assert modes.constrain_samples_value(64, 1) == 64
    for bad in (65, -1, True, 2.0, "4"):
        with pytest.raises(ValueError, match="constrain_samples=.*1\\.\\.64"):
            modes.constrain_samples_value(bad, 3)
    with pytest.raises(ValueError, match="constrain_samples=4 needs constrain"):
        modes.constrain_samples_value(4, None)
    with pytest.raises(ValueError, match="constrain_samples excludes constrain_beams"):
        modes.constrain_samples_value(4, 3, 2)


def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng.num_token = NTOK
    N, L, F, T, R = 2, 8, 4, 5, 2
    memory = torch.zeros(N, L + NTOK, 64)
    ft = torch.zeros(N, L, 1, dtype=torch.int32)
    cd, cl = torch.zeros(N, L, L, dtype=torch.uint8), torch.zeros(N, L, dtype=torch.uint8)
    ok = dict(T=T, F=F, num_input=[4, 3], constrain="loops", constrain_samples=R, term_range=TERM, follow_table=ft,
              uniforms=torch.zeros(T - 1, N * F * R))

    def refused(match, variant=lib.FF_PARALLEL, mem=memory, **change):
        with pytest.raises(ValueError, match=match):
            eng.decode(mem, None, None, variant, **dict(ok, **change))
    refused("constrain_samples=2 needs constrain", constrain=None)
    for bad in (65, -1, True):
        refused("constrain_samples=.*1\\.\\.64", constrain_samples=bad)
    refused("constrain_samples excludes constrain_beams", constrain_beams=2)
    for change in (dict(num_samples=2), dict(beam_width=2), dict(retire=True), dict(logprob=True), dict(return_pointer=True),
                   dict(no_stop=True), dict(stop_callback=lambda c: False), dict(extra_mask=torch.zeros(8, 12, dtype=torch.uint8))):
        refused("constrain_samples excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width and num_samples",
                **change)
    refused("constrain_samples is a parallel-variant option", variant=lib.FF_SEQ2SEQ)
    refused("constrain_samples needs term_range", term_range=None)
    refused("constrain_exact excludes constrain_lookahead", constrain_lookahead=True, constrain_exact=True, close_dist=cd, cycle_len=cl)
    refused("constrain_lookahead needs constrain='loops'", constrain="no_repeat", constrain_lookahead=True, close_dist=cd, cycle_len=cl)
    refused("constrain_exact needs constrain='loops'", constrain="no_repeat", constrain_exact=True, cycle_len=cl)
    refused("constrain='loops' needs follow_table", follow_table=None)
    refused("constrain_lookahead needs close_dist and cycle_len", constrain_lookahead=True)
    refused("constrain_exact needs cycle_len", constrain_exact=True)
    refused("constrain_lookahead takes T <= 256", constrain_lookahead=True, close_dist=cd, cycle_len=cl, T=257,
            uniforms=torch.zeros(256, N * F * R))
    refused("constrain_exact takes T <= 256", constrain_exact=True, cycle_len=cl, T=257, uniforms=torch.zeros(256, N * F * R))
    big = 2048 - NTOK + 1
    refused("constrain_exact takes at most 2044 edges", mem=torch.zeros(1, big + NTOK, 64), constrain_exact=True, num_input=[4],
            follow_table=torch.zeros(1, big, (big + 31) // 32, dtype=torch.int32), cycle_len=torch.zeros(1, big, dtype=torch.uint8),
            uniforms=torch.zeros(T - 1, F * R))
    for change in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(temperature=float("inf"))):
        refused("temperature", **change)
    for bad in (None, torch.zeros(T - 1, N * F * R - 1), torch.zeros(T - 2, N * F * R), torch.zeros(T - 1, N * F * R, dtype=torch.float64)):
        refused("uniforms must be a float32 tensor of shape \\[4, 16\\]", uniforms=bad)
    refused("follow_table must be an int32 tensor", follow_table=ft.long())
    refused("cycle_len must be a uint8 tensor", constrain_exact=True, cycle_len=cl.int())
    # num_samples together with constrain is still refused, with the text it had
    with pytest.raises(ValueError, match="^constrain excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width and num_samples$"):
        eng.decode(memory, None, None, lib.FF_PARALLEL, T=T, F=F, num_input=[4, 3], constrain="loops", num_samples=2, term_range=TERM,
                   follow_table=ft, uniforms=torch.zeros(T - 1, N * F * R))


def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _tiny_inputs():
    return {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
            "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}


def test_models_reject_the_combinations_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert model.constrain_samples == 0
    model.constrain_samples = 2

    def refused(match, inputs=None, **attrs):
        old = {k: getattr(model, k) for k in attrs}
        for k, v in attrs.items():
            setattr(model, k, v)
        try:
            with torch.no_grad(), pytest.raises(ValueError, match=match):
                model.forward_eval(inputs or _tiny_inputs())
        finally:
            for k, v in old.items():
                setattr(model, k, v)
    refused("constrain_samples=2 needs constrain")
    model.constrain = "loops"
    refused("constrain_samples=.*1\\.\\.64", constrain_samples=65)
    refused("constrain_samples excludes constrain_beams", constrain_beams=2)
    for attr, val in (("num_samples", 2), ("beam_width", 2), ("retire_finished", True), ("return_logprob", True)):
        refused("constrain excludes beam_width, num_samples, retire_finished, return_logprob and an extra mask", **{attr: val})
    refused("constrain excludes", inputs=dict(_tiny_inputs(), extra_mask=torch.zeros(1, 4, 8, dtype=torch.bool)))
    refused("constrain_exact excludes constrain_lookahead", constrain_lookahead=True, constrain_exact=True)
    refused("constrain_lookahead needs constrain='loops'", constrain="no_repeat", constrain_lookahead=True)
    for attr, val in (("sample_temperature", -1.0), ("sample_top_p", 0.0), ("sample_top_k", -2)):
        refused("temperature", **{attr: val})
    refused("constrain_lookahead takes T <= 256", constrain_lookahead=True, max_face_length=257)
    refused("constrain_exact takes T <= 256", constrain_exact=True, max_face_length=257)
    # the exact form above 2048 keys, with the option set: the input's line count is checked before the encoder runs
    wide = {"input": torch.zeros(1, 2045, 50, 2), "input_mask": torch.zeros(1, 2045, dtype=torch.bool),
            "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    refused("constrain_exact takes at most 2044 edges per wireframe \\(got 2045\\)", inputs=wide, constrain_exact=True)
    refused("cycle_len must be uint8 \\[1, 8\\]", inputs=dict(_tiny_inputs(), cycle_len=torch.zeros(1, 8, dtype=torch.int32)), constrain_exact=True)
    # a wrong inputs["sample_uniforms"] shape: [T - 1, N * F * R] = [4, 8]
    for bad in (torch.zeros(4, 7), torch.zeros(3, 8), torch.zeros(4, 16)):
        refused("sample_uniforms must have shape \\[4, 8\\]", inputs=dict(_tiny_inputs(), sample_uniforms=bad))
    with pytest.raises(ValueError, match="score\\(\\) excludes constrain"):
        model.score(_tiny_inputs(), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    model.constrain = None
    with pytest.raises(ValueError, match="score\\(\\) excludes constrain_samples"):
        model.score(_tiny_inputs(), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        sub.constrain, sub.constrain_samples = "loops", 2
        with torch.no_grad(), pytest.raises(ValueError, match="constrain needs the native engine"):
            sub.forward_eval(_tiny_inputs())
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    seq.constrain_samples = 2
    with torch.no_grad(), pytest.raises(ValueError, match="constrain_samples is a SurfaceFormer_Parallel option"):
        seq.forward_eval({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})


def test_decode_sharded_rejects_the_option_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain=None,
                                  constrain_samples=2)
    with pytest.raises(ValueError, match="decode_sharded does not implement constrain_samples"):
        dist.decode_sharded(model, {}, NoDist())
    model.constrain_samples = 0
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: faces and the CLI -------------------------------------------------------------------------------------------------------
def test_scored_constrained_sample_faces_on_hand_written_rows():
    smp = np.array([[[0, 4, 5, 1, 0, 0], [0, 4, 6, 2, 0, 0], [0, 5, 4, 1, 0, 0], [0, 4, 7, 1, 0, 0]],      # anchor 0: {0,1} twice, {0,2}, a dead end
                    [[1, 0, 0, 0, 0, 0]] * 4])                                                              # anchor 1: finished at its start token
    scores = np.array([[-0.5, -1.5, -0.25, -0.125], [0.0, 0.0, 0.0, 0.0]])
    dead = np.array([[0, 0, 0, 1], [0, 0, 0, 0]])
    got = faces.parse_parallel_constrained_samples_scored(smp, scores, dead, 4, TOK)
    assert got == [(0, (0, 1), -0.5), (1, (0, 2), -1.5), (0, (1, 0), -0.25)]                                # the dead-ended draw is dropped
    uniq = faces.unique_faces_with_scores(got)
    assert uniq[0] == (0, (0, 1), -0.25, 2) and uniq[1][2:] == (-1.5, 1)                                    # best score, votes over draws
    assert faces.parse_parallel_constrained_samples_scored(smp, scores, np.zeros_like(dead), 4, TOK)[-1] == (0, (0, 3), -0.125)
    lp = np.zeros(smp.shape)
    lp[0, :, 1] = [-0.25, -1.0, -0.125, -0.0625]
    lp[0, :, 2] = [-0.25, -0.5, -0.125, -0.0625]
    assert faces.parse_parallel_constrained_samples_scored(smp, lp, dead, 4, TOK) == got                    # per-position values: summed
    assert scores[0, 3] == -0.125                                                                           # (the caller's array is not written)
    with pytest.raises(ValueError):
        faces.parse_parallel_constrained_samples_scored(smp, scores[:1], dead, 4, TOK)


def test_cli_flags_reach_the_model_and_the_record_is_todays_without_them(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    from conftest import GOLDEN
    from faceformer_amd import datasets as D
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--constrain", "loops", "--constrain-samples", "8", "--temperature", "0.5",
                                       "--top-k", "16", "--top-p", "0.9", "--seed", "7", "--constrain-exact"])
    assert (a.constrain, a.constrain_samples, a.temperature, a.top_k, a.top_p, a.seed, a.constrain_exact) == ("loops", 8, 0.5, 16, 0.9, 7, True)
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).constrain_samples == 0
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--constrain", "loops", "--constrain-samples", "8", "--constrain-lookahead", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["constrain"], kw["constrain_samples"], kw["constrain_lookahead"]) for kw in seen] == [("loops", 8, True), (None, 0, False)]
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3, constrain_samples=8, temperature=0.5, top_k=16,
                            top_p=0.9, seed=7, constrain_exact=True)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3, constrain_exact=True, constrain_samples=8, sample_temperature=0.5,
                           sample_top_k=16, sample_top_p=0.9, sample_seed=7)
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    cfg = types.SimpleNamespace(model_class="SurfaceFormer_Parallel")
    run = lambda **kw: run_test(cfg, None, out_dir="unused", device="cpu", model=object(), **kw)
    with pytest.raises(ValueError, match="--constrain-samples requires --constrain"):
        run(constrain_samples=2)
    for bad in (0.5, 65, -1, True):
        with pytest.raises(ValueError, match="--constrain-samples must be a count in 1..64"):
            run(constrain="loops", constrain_samples=bad)
    with pytest.raises(ValueError, match="--constrain-samples is not implemented with --constrain-beams"):
        run(constrain="loops", constrain_samples=2, constrain_beams=2)
    with pytest.raises(ValueError, match="--constrain-samples is not implemented for multi-rank runs"):
        run(constrain="loops", constrain_samples=2, dist_mod=types.SimpleNamespace(get_world_size=lambda: 2))
    with pytest.raises(ValueError, match="--constrain-exact is not combined with --constrain-lookahead"):
        run(constrain="loops", constrain_samples=2, constrain_exact=True, constrain_lookahead=True)
    for kw in (dict(sample=2), dict(beam=2), dict(scores=True), dict(retire_finished=True), dict(score_labels=True)):
        with pytest.raises(ValueError, match="--constrain applies to SurfaceFormer_Parallel only, and not together with"):
            run(constrain="loops", constrain_samples=2, **kw)
    with pytest.raises(ValueError, match="--constrain applies to SurfaceFormer_Parallel only"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer"), None, out_dir="unused", device="cpu", model=object(), constrain="loops",
                 constrain_samples=2)
    # the record: byte-identical without the draws; with them the three sample keys, and the two counts over ALL draws
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
    n = int(item["num_input"])
    text, st = cli.record_of(cfg, smp["raw"], item, pred, True)
    assert text == cli.record_of(cfg, smp["raw"], item, pred, True, constrained_samples=None)[0]
    de0 = np.zeros(pred.shape[0], dtype=np.int32)
    base = json.loads(cli.record_of(cfg, smp["raw"], item, pred, True, dead_end=de0)[0])
    tokens = np.stack([pred, pred, pred], axis=1)                                            # R = 3: the greedy rows three times
    scores = np.stack([-np.arange(pred.shape[0]) / 8.0 - k for k in range(3)], axis=1)
    dead = np.zeros(tokens.shape[:2], dtype=np.int32)
    dead[0, 1] = dead[n - 1, 2] = 1
    dead[n:, 0] = 1                                                                          # (a padding-anchor row is not counted)
    text2, st2 = cli.record_of(cfg, smp["raw"], item, pred, True, dead_end=de0, constrained_samples=(tokens, scores, dead))
    rec2 = json.loads(text2)
    assert list(rec2) == list(base) + ["pred_sample_faces", "pred_sample_face_scores", "pred_sample_face_votes"] and st2 == st
    assert {k: rec2[k] for k in base if k not in ("pred_dead_ends", "pred_unclosed")} == \
           {k: base[k] for k in base if k not in ("pred_dead_ends", "pred_unclosed")}
    assert rec2["pred_dead_ends"] == 2 and rec2["pred_unclosed"] == 3 * base["pred_unclosed"]
    sc, votes = rec2["pred_sample_face_scores"], rec2["pred_sample_face_votes"]
    assert len(sc) == len(votes) == len(rec2["pred_sample_faces"]) > 0 and sc == sorted(sc, reverse=True)
    none_dead = json.loads(cli.record_of(cfg, smp["raw"], item, pred, True, dead_end=de0, constrained_samples=(tokens, scores, dead * 0))[0])
    assert sum(none_dead["pred_sample_face_votes"]) >= sum(votes) and all(v % 3 == 0 for v in none_dead["pred_sample_face_votes"])


# ---- the operator's cases (shared with tools/constrain_sample_left_out.py: CPU data only) -------------------------------------------
SIZES = [NTOK + 1, 63, 64, 65, 260, 1028]
SHAPES = [(1, 1), (3, 3), (4, 3), (9, 3), (9, 1), (4, 1)]                # (B, seqs_per_group): w = b / spg with whole and cut groups
BUDGETS = (3, 40)


def flags_of(form):
    return {"plain": (0, CR.NO_REPEAT, CR.CONNECT, LOOPS), "ahead": (CR.CONNECT, LOOPS), "exact": (LOOPS,)}[form]


_CASES = {}


def operator_case(B, S, spg, seed, form="plain", on_gpu=False):
    """The seeded case (made once per process), with the distance tables of its follow tables when the form reads them:
    faces.follow_distance on the CPU, or ops.follow_distance (the same integers: test_lookahead holds one to the other)."""
    key = (B, S, spg, seed)
    if key not in _CASES:
        _CASES[key] = _make_case(B, S, spg, seed)
    c = _CASES[key]
    if form != "plain" and c["close"][0] is None:
        if on_gpu:
            from faceformer_amd.hip import ops
            bits = torch.from_numpy(faces.pack_follow_bits(c["follows"])).cuda()
            close, cycle = ops.follow_distance(bits, torch.full((c["W"],), c["L"], dtype=torch.int32).cuda(), 254)
            c["close"], c["cycle"] = close.cpu().numpy(), cycle.cpu().numpy()
        else:
            c["close"], c["cycle"] = faces.follow_distance(c["follows"], 254)
    return c


def _make_case(B, S, spg, seed):
    """Rows in every state: b % 5 = 0 open with an unused edge that leads on to the first one, 1 closed, 2 finished (row 2) or closed, 3 open with every follower visited (a dead
    end under NO_REPEAT | CONNECT), 4 closed and much visited.  Wireframe 0 has 0 < kv_len < S, wireframe 1 one live key, the
    last of three or more none; padded candidates everywhere.  -> dict of CPU data."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng([seed, B, S, spg])
    L = S - NTOK
    W = (B + spg - 1) // spg
    logits = torch.randn(B, S, generator=g) * 3.0
    if B >= 4:
        logits[B - 1] = 0.75                                             # all-equal logits: ties
    mask = torch.rand(W, S, generator=g) < 0.15
    mask[:, :NTOK] = False
    kv = torch.tensor([S if w % 2 else max(1, S - 2 - w) for w in range(W)], dtype=torch.int32)
    if W > 1:
        mask[1] = True
        mask[1, TERM[0]] = False                                         # one live key: a terminator
    if W > 2:
        kv[W - 1] = 0                                                    # no live key
    follows = CR.random_follows(W, L, seed)
    fin = np.zeros(B, dtype=np.int32)
    first = np.full(B, -1, dtype=np.int32)
    prev = np.full(B, -1, dtype=np.int32)
    visited = np.zeros((B, L), dtype=bool)
    for b in range(B):
        kind = b % 5
        if kind in (0, 3):
            first[b], prev[b] = rng.integers(0, L), rng.integers(0, L)
            visited[b, [first[b], prev[b]]] = True
            if kind == 0 and L >= 3:                                     # a way on that closes: prev -> x -> first, x unused
                x = int(rng.choice([e for e in range(L) if e not in (first[b], prev[b])]))
                follows[b // spg, prev[b], x] = follows[b // spg, x, first[b]] = True
            if kind == 3:
                visited[b] |= follows[b // spg, prev[b]]
        elif kind in (1, 4):
            prev[b] = rng.integers(-1, L)
            visited[b] = rng.random(L) < (0.2 if kind == 1 else 0.9)
            if kind == 4 and prev[b] < 0:
                first[b] = rng.integers(0, L)                            # first without prev: closed (the header's rule)
    if B > 2:
        fin[2] = 1
    memory = torch.randn(W, S, 64, generator=g)
    wf = torch.arange(B) // spg
    pad = (mask[wf] | (torch.arange(S)[None, :] >= kv[wf, None])).numpy()
    u = torch.rand(B + 5, generator=g)
    row_id = torch.randperm(B + 5, generator=g)[:B].to(torch.int32)
    close = cycle = [None] * W                                           # (operator_case makes them for the forms that read them)
    return dict(logits=logits, mask=mask, kv=kv, follows=follows, fin=fin, first=first, prev=prev, visited=visited, memory=memory, pad=pad,
                u=u, row_id=row_id, close=close, cycle=cycle, L=L, W=W, B=B, S=S, spg=spg)


def operator_cases(S, form, on_gpu=False):
    """(case, flags, (tau, K, P), budget) of one (S, form): every shape under every flag combination of the form with the
    parameter sets taken in turn, and every parameter set on the widest shape under "loops"."""
    i = 0
    for flags in flags_of(form):
        for B, spg in SHAPES:
            tau, K, P = PARAMS[i % len(PARAMS)]
            yield operator_case(B, S, spg, 1000 * S + 10 * B + spg, form, on_gpu), flags, (tau, S + 3 if K == "S+3" else K, P), BUDGETS[i % 2]
            i += 1
    for pi, (tau, K, P) in enumerate(PARAMS):
        yield operator_case(9, S, 3, 1000 * S + 97 + pi % 3, form, on_gpu), flags_of(form)[-1], (tau, S + 3 if K == "S+3" else K, P), BUDGETS[pi % 2]


def state_of(c, b):
    return (frozenset(np.flatnonzero(c["visited"][b]).tolist()), None if c["first"][b] < 0 else int(c["first"][b]),
            None if c["prev"][b] < 0 else int(c["prev"][b]))


def reference_rows(c, form, flags, params, budget):
    """constrain_sample_ref.step_row of every row of a case on its raw logits (the kernel's own masked logits are these with
    FILL at the padded and the masked keys: an fp32 row in, the same fp32 row out)."""
    raw = c["logits"].numpy().astype(np.float64)
    u = c["u"].numpy()[c["row_id"].long().numpy()]
    for b in range(c["B"]):
        w = b // c["spg"]
        yield CSR.step_row(form, raw[b], c["pad"][b], state_of(c, b), flags, NTOK, TERM, c["follows"][w], u[b], *params,
                           finished=bool(c["fin"][b]), close_dist=c["close"][w], cycle_len=c["cycle"][w], budget=budget)


def _device(c):
    if "dev" not in c:
        pack = lambda a: torch.from_numpy(faces.pack_follow_bits(a)).cuda()
        c["dev"] = dict(fin=torch.from_numpy(c["fin"]).cuda(), first=torch.from_numpy(c["first"]).cuda(), prev=torch.from_numpy(c["prev"]).cuda(),
                        visited=pack(c["visited"]), follows=pack(c["follows"]), memory=c["memory"].cuda(), mask=c["mask"].to(torch.uint8).cuda(),
                        kv=c["kv"].cuda(), u=c["u"].cuda(), row_id=c["row_id"].cuda())
    if "close" not in c["dev"] and c["close"][0] is not None:
        c["dev"].update(close=torch.from_numpy(c["close"]).cuda(), cycle=torch.from_numpy(c["cycle"]).cuda())
    return c["dev"]


def _run_operator(c, form, flags, params, budget, e=None, logits=None, **kw):
    """ops.pointer_constrained_sample on a case (e: what puts an operand on the device -- the redzone test embeds them)."""
    from faceformer_amd.hip import ops
    d = _device(c) if e is None else {k: e(v) for k, v in _device(c).items()}
    lg = c["logits"].clone().cuda() if logits is None else logits
    res = ops.pointer_constrained_sample(lg, d["u"], d["fin"], d["first"], d["prev"], d["visited"], flags, NTOK, follows=d["follows"],
                                         temperature=params[0], top_k=params[1], top_p=params[2], row_id=d["row_id"],
                                         lookahead=LOOKAHEAD[form], close_dist=d.get("close") if form == "ahead" else None,
                                         cycle_len=d.get("cycle") if form != "plain" else None, budget=budget, memory=d["memory"],
                                         mask=d["mask"], kv_len=d["kv"], seqs_per_group=c["spg"], term_range=TERM, want_rows=True,
                                         want_stats=True, **kw)
    return lg, res


def _run_greedy(c, form, flags, budget):
    """The constrained greedy operator of the same form on the same case."""
    from faceformer_amd.hip import ops
    d = _device(c)
    lg = c["logits"].clone().cuda()
    common = dict(memory=d["memory"], mask=d["mask"], kv_len=d["kv"], seqs_per_group=c["spg"], term_range=TERM, want_rows=True, want_stats=True)
    state = (d["fin"], d["first"], d["prev"], d["visited"], flags, NTOK)
    if form == "plain":
        return lg, ops.pointer_constrained(lg, *state, follows=d["follows"], **common)
    if form == "ahead":
        return lg, ops.pointer_constrained_ahead(lg, *state, d["follows"], d["close"], d["cycle"], budget, **common)
    return lg, ops.pointer_constrained_exact(lg, *state, d["follows"], d["cycle"], budget, **common)


def _bits_to_bool(bits, L):
    from test_constrain import _bits_to_bool as to_bool
    return to_bool(bits, L)


# ---- GPU: the operator ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S", SIZES)
def test_operator_against_the_numpy_rule(hip_lib, S, form):
    from faceformer_amd.hip import ops
    seen = dict(open=0, closed=0, dead=0, finished=0, onelive=0, nolive=0, short_kv=0, padded=0)
    rows_seen = rows_left = 0
    for c, flags, params, budget in operator_cases(S, form, on_gpu=True):
        B, L, spg = c["B"], c["L"], c["spg"]
        counter = torch.zeros(1, dtype=torch.int32).cuda()
        lg, res = _run_operator(c, form, flags, params, budget, counter=counter)
        own, raw = lg.cpu().numpy(), c["logits"].numpy()
        got = {k: res[k].cpu().numpy() for k in ("next", "logprob", "fin", "dead_end", "first", "prev")}
        vis = _bits_to_bool(res["visited"], L)
        byte_rows = res["mask_rows"].cpu().numpy() != 0
        what = (S, form, B, spg, flags, params, budget)
        nge = 0
        for b, r in enumerate(reference_rows(c, form, flags, params, budget)):
            st = state_of(c, b)
            if c["fin"][b]:
                assert np.array_equal(own[b], raw[b]), what                                # finished rows untouched
                assert got["next"][b] == 0 and got["logprob"][b] == 0.0 and got["fin"][b] and not got["dead_end"][b], what
                assert (got["first"][b], got["prev"][b]) == (CSR.none_to(st[1]), CSR.none_to(st[2])), what
                assert set(np.flatnonzero(vis[b]).tolist()) == set(st[0]), what
                seen["finished"] += 1
                continue
            hidden = r["masked"] | c["pad"][b]
            assert np.array_equal(byte_rows[b], r["masked"]), (what, b)                    # the byte row: the rule's own mask, exact
            assert np.array_equal(own[b] == np.float32(FILL), hidden), (what, b)           # the FILL pattern: the allowed set
            assert np.array_equal(own[b][~hidden], raw[b][~hidden]), (what, b)
            assert bool(got["dead_end"][b]) == r["dead"], (what, b)
            tok = int(got["next"][b])
            # the draw on the kernel's OWN masked logits (the state update follows the kernel's token: an indecisive row is still checked)
            k = CSR.draw_row(own[b].astype(np.float64), r["masked"], r["dead"], st, NTOK, TERM, c["follows"][b // spg],
                             c["u"].numpy()[int(c["row_id"][b])], *params)
            assert k["decisive"] == r["decisive"] and k["tok"] == r["tok"], (what, b)
            rows_seen, rows_left = rows_seen + 1, rows_left + (not k["decisive"])
            if k["decisive"]:
                assert tok == k["tok"], (what, b, tok, k["tok"])
            live = ~hidden
            if live.any():
                assert live[tok] and k["kept_k"][tok], (what, b, tok)                      # never a masked key, never outside the top-k set
            else:
                assert tok == 0, (what, b)
            want_lp = SR.logprob_of(own[b].astype(np.float64), tok)
            assert abs(float(got["logprob"][b]) - want_lp) <= SR.LP_BAR + SR.EPS * abs(want_lp), (what, b, got["logprob"][b], want_lp)
            assert bool(got["fin"][b]) == (r["dead"] or TERM[0] <= tok < TERM[1]), (what, b)
            nv, nf, npv = CR.advance(st, tok, NTOK, c["follows"][b // spg])
            assert (got["first"][b], got["prev"][b]) == (CSR.none_to(nf), CSR.none_to(npv)), (what, b)
            assert set(np.flatnonzero(vis[b]).tolist()) == set(nv), (what, b)
            nge += tok >= NTOK
            is_open = bool(flags & CR.CONNECT) and st[1] is not None and st[2] is not None
            seen["dead" if r["dead"] else ("open" if is_open else "closed")] += 1
            seen["onelive"] += int(live.sum() == 1)
            seen["nolive"] += int(not live.any())
            seen["short_kv"] += int(0 < int(c["kv"][b // spg]) < S)
            seen["padded"] += int(c["pad"][b][NTOK:].any() and not c["pad"][b].all())
        assert int(counter.item()) == nge, what
        forced = ops.pointer_forced(c["logits"].clone().cuda(), res["next"], _device(c)["memory"], _device(c)["mask"], _device(c)["kv"],
                                    seqs_per_group=spg, want_rows=True, want_stats=True)
        assert torch.equal(res["rows"], forced["rows"]) and torch.equal(res["stats"], forced["stats"]), what
        lg2, res2 = _run_operator(c, form, flags, params, budget)                          # two launches: bit-equal
        assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
    print("S=%d %s rows by state: %s; %d of %d rows indecisive" % (S, form, seen, rows_left, rows_seen))
    assert rows_left <= SR.CAP * rows_seen, (S, form, rows_left, rows_seen)
    assert all(v > 0 for k, v in seen.items() if S >= 63 or k not in ("open", "dead")), seen           # every state was exercised


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S", SIZES)
def test_operator_identity_a_temperature_zero_is_the_constrained_greedy_step(hip_lib, S, form):
    for flags in flags_of(form):
        for B, spg in SHAPES:
            c = operator_case(B, S, spg, 1000 * S + 10 * B + spg, form, on_gpu=True)
            for budget in BUDGETS if form != "plain" else BUDGETS[:1]:
                lg, res = _run_operator(c, form, flags, (0.0, 3, 0.5), budget)
                gl, ref = _run_greedy(c, form, flags, budget)
                for k in ref:                                                              # token, log-probability, state, byte rows, appended rows
                    assert torch.equal(res[k], ref[k]), (S, form, flags, B, spg, budget, k)
                assert torch.equal(lg, gl) and set(res) == set(ref)
                assert torch.equal(res["logprob"].view(torch.int32), ref["logprob"].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_operator_identity_b_flag_bits_clear_is_pointer_sample(hip_lib, S):
    from faceformer_amd.hip import ops
    for pi, (tau, K, P) in enumerate(PARAMS):
        B, spg = SHAPES[pi % len(SHAPES)]
        c = operator_case(B, S, spg, 1000 * S + 10 * B + spg)
        d = _device(c)
        K = S + 3 if K == "S+3" else K
        cnt = [torch.zeros(1, dtype=torch.int32).cuda() for _ in range(2)]
        lg, res = _run_operator(c, "plain", 0, (tau, K, P), 0, counter=cnt[0])
        sl = c["logits"].clone().cuda()
        ref = ops.pointer_sample(sl, d["u"], temperature=tau, top_k=K, top_p=P, row_id=d["row_id"], fin=d["fin"], memory=d["memory"],
                                 mask=d["mask"], kv_len=d["kv"], seqs_per_group=spg, term_range=TERM, want_rows=True, want_stats=True,
                                 counter=cnt[1], ge_bound=NTOK)
        for k in ref:
            assert torch.equal(res[k], ref[k]), (S, tau, K, P, k)
        assert torch.equal(lg, sl) and torch.equal(cnt[0], cnt[1]) and not bool(res["mask_rows"].any()) and not bool(res["dead_end"].any())


@pytest.mark.gpu
def test_operator_frequencies_follow_the_fp64_probabilities_of_the_constrained_row(hip_lib):
    """One open-loop row at S = 65 whose follow row leaves 7 live edges, tau = 1, 65 536 rows with seeded uniforms."""
    from faceformer_amd.hip import ops
    S, B = 65, 65536
    L = S - NTOK
    g = torch.Generator().manual_seed(11)
    row = torch.randn(S, generator=g)
    table = np.zeros((1, L, L), dtype=bool)
    live = [3, 8, 20, 31, 32, 45, 60]
    table[0, 5, live] = True                                              # prev = 5: seven followers, none of them the first edge
    vis = np.zeros((B, L), dtype=bool)
    vis[:, [2, 5]] = True
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32).cuda()
    u = torch.rand(B, generator=torch.Generator().manual_seed(12))
    res = ops.pointer_constrained_sample(row[None, :].repeat(B, 1).cuda(), u.cuda(), i32(0), i32(2), i32(5),
                                         torch.from_numpy(faces.pack_follow_bits(vis)).cuda(), LOOPS, NTOK,
                                         follows=torch.from_numpy(faces.pack_follow_bits(table)).cuda(), seqs_per_group=B, term_range=TERM)
    keys = [NTOK + e for e in live]
    counts = np.bincount(res["next"].cpu().numpy(), minlength=S).astype(np.float64)
    assert counts.sum() == B and counts[[s for s in range(S) if s not in keys]].sum() == 0          # zero draws on masked keys
    p = np.zeros(S)
    p[keys] = np.exp(row.numpy().astype(np.float64)[keys])
    p /= p.sum()
    sigma = np.sqrt(B * p[keys] * (1 - p[keys]))
    z = np.abs(counts[keys] - B * p[keys]) / sigma
    print("frequency check: worst |count - N p| / sigma = %.2f over %d live keys" % (z.max(), len(keys)))
    assert (z <= 5).all(), z.max()
    assert not bool(res["dead_end"].any()) and not bool(res["fin"].any())


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_operator_inside_poisoned_surroundings(hip_lib, form):
    import redzone as RZ
    from test_redzone_ops import PAD, twice
    S, B, spg = 70, 6, 3
    c = operator_case(B, S, spg, 4242, form, on_gpu=True)
    params, budget = (0.8, 16, 0.9), 6

    def call(lg, e):
        return dict(_run_operator(c, form, LOOPS, params, budget, e=e, logits=lg, counter=e(torch.zeros(1, dtype=torch.int32)))[1], logits=lg)
    got = twice(lambda g: call(g.embed(c["logits"], ld=S + PAD, name="logits"), lambda t: g.embed(t.cpu())), "ff_pointer_constrained_sample")
    plain = call(c["logits"].clone().cuda(), lambda t: t.cuda())
    for k, v in plain.items():
        if torch.is_tensor(v):
            RZ.assert_same_bits(got[k], v, "ff_pointer_constrained_sample %s: %s against the clean call" % (form, k))
    assert torch.isfinite(got["logprob"]).all() and bool(got["mask_rows"].any())


@pytest.mark.gpu
def test_operator_refuses_bad_arguments(hip_lib):
    from faceformer_amd.hip import lib as L, ops
    c = operator_case(3, 9, 3, 1, "exact", on_gpu=True)
    for kw in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0)):
        with pytest.raises(ValueError, match="sampling needs"):
            _run_operator(c, "plain", LOOPS, (kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0)), 0)
    d = _device(c)
    with pytest.raises(ValueError, match="lookahead="):
        ops.pointer_constrained_sample(c["logits"].clone().cuda(), d["u"], d["fin"], d["first"], d["prev"], d["visited"], LOOPS, NTOK,
                                       follows=d["follows"], seqs_per_group=3, lookahead="both")
    with pytest.raises(ValueError, match="the exact look-ahead needs"):
        ops.pointer_constrained_sample(c["logits"].clone().cuda(), d["u"], d["fin"], d["first"], d["prev"], d["visited"], CR.CONNECT, NTOK,
                                       follows=d["follows"], seqs_per_group=3, lookahead="exact", cycle_len=d["cycle"], budget=3)
    with pytest.raises(ValueError, match="3 uniforms for"):
        ops.pointer_constrained_sample(torch.zeros(4, 9).cuda(), d["u"][:3], torch.zeros(4, dtype=torch.int32).cuda(),
                                       torch.zeros(4, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int32).cuda(),
                                       torch.zeros(4, 1, dtype=torch.int32).cuda(), 0, NTOK)
    # the C entry's own checks, behind the Python ones
    lg, z = torch.zeros(2, 9).cuda(), torch.zeros(2, dtype=torch.int32).cuda()
    byte, word, out = torch.zeros(2, 9, dtype=torch.uint8).cuda(), torch.zeros(2, 1, dtype=torch.int32).cuda(), torch.zeros(2).cuda()
    p = ops._p

    def entry(flags=0, follows=None, tau=1.0, top_p=1.0, lookahead=0, cycle=None, budget=0, uniforms=torch.rand(2).cuda()):
        return hip_lib.ff_pointer_constrained_sample(p(lg), 9, 9, None, None, 2, 1, p(follows), 5, flags, NTOK, TERM[0], TERM[1], p(z), p(z), p(z),
                                                     p(word), p(byte), p(z), p(out), p(z), p(z), p(z), p(z), None, 0, None, 0, None, None,
                                                     p(uniforms), 2, None, tau, 0, top_p, lookahead, None, p(cycle), budget, None)
    assert entry() == 0
    torch.cuda.synchronize()
    for kw, text in ((dict(flags=4), "unknown flag bits"), (dict(flags=2), "needs the follow table"), (dict(tau=-1.0), "temperature"),
                     (dict(top_p=0.0), "top_p"), (dict(lookahead=3), "lookahead=3"), (dict(uniforms=None), "null pointer"),
                     (dict(flags=3, follows=word, lookahead=2), "cycle_len is required"),
                     (dict(flags=3, follows=word, lookahead=2, cycle=byte, budget=255), "budget=255"),
                     (dict(flags=1, lookahead=1, cycle=byte), "needs FF_CONSTRAIN_CONNECT")):
        assert entry(**kw) != 0, kw
        assert text in hip_lib.ff_last_error().decode() and "ff_pointer_constrained_sample" in hip_lib.ff_last_error().decode(), (kw, hip_lib.ff_last_error())
    assert L.FF_CONSTRAIN_CONNECT == 2


# ---- GPU: the engine --------------------------------------------------------------------------------------------------------------
ENGINE_GOLDENS = ["par_small_gain4", "par_small_ragged", "par_full_n40_gain4"]
R4 = CSR.REPLAY_R


def _model(name):
    from test_constrain import _model as model
    return model(name)


def _tables(name):
    from test_lookahead import _tables as tables
    return tables(name)


def _uniforms(lat, T, R, seed=CSR.REPLAY_SEED):
    return SR.make_uniforms(lat["num_input"], T, R, seed).cuda()


def _form_kw(form, tables):
    bits, close, cyc = tables
    return {"plain": {}, "ahead": dict(constrain_lookahead=True, close_dist=close, cycle_len=cyc),
            "exact": dict(constrain_exact=True, cycle_len=cyc)}[form]


def _csample(model, case, b, form, tables, R, params, u, flags=LOOPS, **kw):
    from test_logprob import _decode
    return _decode(model, case, b, constrain=flags, follow_table=tables[0], term_range=TERM, constrain_samples=R, temperature=params[0],
                   top_k=params[1], top_p=params[2], uniforms=u, **dict(_form_kw(form, tables), **kw))


def _greedy(model, case, b, form, tables, **kw):
    from test_logprob import _decode
    return _decode(model, case, b, constrain=LOOPS, follow_table=tables[0], term_range=TERM, **dict(_form_kw(form, tables), **kw))


def _check_layout(out, T, R):
    """Finish positions, the stop step and the zero padding against the rule applied to the decode's own tokens; scores against
    the fp64 sum of its own log-probabilities; predict / logprob / dead_end against draw 0.  -> (tokens, logprob, finish, steps)."""
    smp, lp = out["samples"].cpu().numpy(), out["sample_logprob"].cpu().numpy()
    assert smp.dtype == np.int64 and lp.dtype == np.float32 and smp.shape == lp.shape and smp.shape[1] == T
    fin, steps = SR.stop_and_finish(smp, TERM, NTOK)
    dead = out["sample_dead_end"].cpu().numpy() != 0
    # (a dead end finishes a draw at a terminator: the finish position is the first terminator either way)
    assert out["steps"] == steps
    past = np.arange(T)[None, :] > np.minimum(fin, steps)[:, None]
    assert (smp[past] == 0).all() and (lp[past] == 0).all() and (lp[:, 0] == 0).all()
    assert np.isfinite(lp).all() and (lp <= 0).all()
    want = lp.astype(np.float64).sum(axis=1)
    got = out["sample_scores"].cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= SR.EPS * np.abs(want)).all()                       # fp64 accumulator, rounded once
    assert torch.equal(out["predict"], out["samples"].view(-1, R, T)[:, 0])
    assert torch.equal(out["logprob"], out["sample_logprob"].view(-1, R, T)[:, 0])
    assert torch.equal(out["dead_end"], out["sample_dead_end"].view(-1, R)[:, 0])
    assert not (dead & (fin > steps)).any()                                          # a flagged draw did end
    return smp, lp.astype(np.float64), fin, steps


def _pad_of(b):
    mask = b["input_mask"].cpu().numpy()
    return np.concatenate([np.zeros((mask.shape[0], NTOK), dtype=bool), mask], axis=1)


def _replay(out, form, flags, table, tables, pad, u, params, F, T, R, what):
    """The reference on the decode's own traced logits and its own prefixes, pair by pair: the byte row (as the FILL pattern of
    the constrained masked row) exact, the token the rule's on every decisive pair, the dead-end flags and finish positions the
    rule's on the decode's tokens.  -> (decisive [steps, rows], True also where finished; left-out share; pairs)."""
    smp, lp, fin, steps = _check_layout(out, T, R)
    close, cyc = tables[1].cpu().numpy(), tables[2].cpu().numpy()
    logits = out["logits"].cpu().numpy()
    un = u.cpu().numpy()
    dead = out["sample_dead_end"].cpu().numpy() != 0
    want_dead = np.zeros(smp.shape[0], dtype=bool)
    dec = np.ones((steps, smp.shape[0]), dtype=bool)
    pairs = 0
    for j in range(steps):
        for r in np.flatnonzero(fin > j):
            w = r // (F * R)
            fol = None if table is None else table[w]
            st = CR.state_of_prefix(smp[r, : j + 1], NTOK, fol)
            row = logits[j, r]
            masked, is_dead = CSR.rule_mask(form, st, flags, row.size, NTOK, TERM, fol, pad[w], close[w], cyc[w], T - 2 - j)
            assert np.array_equal(row == np.float32(FILL), masked | pad[w]), (what, j, int(r))
            res = SR.sample_row(row.astype(np.float64), un[j, r], *params)
            pairs += 1
            dec[j, r] = res["decisive"]
            tok = int(smp[r, j + 1])
            if res["decisive"]:
                assert tok == res["tok"], (what, j, int(r), tok, res["tok"])
            assert row[tok] > np.float32(FILL) or not (row > np.float32(FILL)).any(), (what, j, int(r))
            own = SR.logprob_of(row.astype(np.float64), tok)
            assert abs(lp[r, j + 1] - own) <= SR.LP_BAR + SR.EPS * abs(own), (what, j, int(r))
            want_dead[r] |= is_dead
            if is_dead:
                assert fin[r] == j + 1, (what, j, int(r))
    assert np.array_equal(dead, want_dead), what
    return dec, (~dec).sum() / max(1, pairs), pairs


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_identity_a_temperature_zero_is_the_constrained_greedy_decode(hip_lib, name, form):
    from test_parity_golden import _tol
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T = case["model"]["seq_len"]
    tables = _tables(name)
    ref = _greedy(model, case, b, form, tables, trace=True)
    pred, steps = ref["predict"].cpu().numpy(), ref["steps"]
    glp = ref["logprob"].cpu().numpy().astype(np.float64)
    rl = ref["logits"].cpu().numpy()
    fin = CR.stop_and_finish(pred, TERM, NTOK)[0]
    tol = np.array([0.0] + [_tol(rl[s][fin > s]) if (fin > s).any() else 0.0 for s in range(steps)] + [0.0] * T)[:T]
    for R in (1, 3):
        out = _csample(model, case, b, form, tables, R, (0.0, 4, 0.5), _uniforms(lat, T, R, 3))
        assert out["steps"] == steps, (name, form, R)
        smp = out["samples"].cpu().numpy().reshape(-1, R, T)
        for k in range(R):
            assert np.array_equal(smp[:, k], pred), (name, form, R, k)
        assert torch.equal(out["sample_dead_end"].view(-1, R), ref["dead_end"][:, None].expand(-1, R))
        lp = out["sample_logprob"].cpu().numpy().astype(np.float64).reshape(-1, R, T)
        err = np.abs(lp - glp[:, None, :])
        print(name, form, "R=%d steps=%d max |logprob - greedy logprob| = %.3g" % (R, steps, err.max()))
        assert (err <= (2 * tol + SR.LP_BAR)[None, None, :]).all(), (name, form, R, err.max())
        _check_layout(out, T, R)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_identity_b_flag_bits_clear_is_the_sampled_decode(hip_lib, name):
    from test_logprob import _decode
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T = case["model"]["seq_len"]
    tables = _tables(name)
    for params in CSR.REPLAY_PARAMS:
        u = _uniforms(lat, T, R4)
        out = _csample(model, case, b, "plain", tables, R4, params, u, flags=0, trace=True)
        ref = _decode(model, case, b, num_samples=R4, temperature=params[0], top_k=params[1], top_p=params[2], uniforms=u, term_range=TERM,
                      trace=True)
        assert out["steps"] == ref["steps"], (name, params)
        for k in ("samples", "sample_logprob", "sample_scores", "predict"):           # the same plan: bit-equal
            assert torch.equal(out[k], ref[k]), (name, params, k)
        assert torch.equal(out["logits"][: out["steps"]].nan_to_num(7.0), ref["logits"][: out["steps"]].nan_to_num(7.0))
        assert not bool(out["sample_dead_end"].any())
        _check_layout(out, T, R4)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_replays_under_the_numpy_rule_and_identity_c(hip_lib, name, form):
    """The (golden, form, parameter set) combinations are constrain_sample_ref's: fixed on the CPU by
    tools/constrain_sample_left_out.py.  Identity (c): draw k of the R-wide decode against the R = 1 decode fed column k."""
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, N, F = case["model"]["seq_len"], len(ni), max(ni)
    tables, pad = _tables(name), _pad_of(b)
    for params in CSR.REPLAY_PARAMS:
        u = _uniforms(lat, T, R4)
        out = _csample(model, case, b, form, tables, R4, params, u, trace=True)
        dec, left, pairs = _replay(out, form, LOOPS, table, tables, pad, u, params, F, T, R4, (name, form, params))
        print(name, form, params, "steps=%d pairs=%d left out %.2f %%; dead ends %d of %d draws"
              % (out["steps"], pairs, 100 * left, int(out["sample_dead_end"].sum()), out["sample_dead_end"].numel()))
        assert pairs > 0 and left <= SR.CAP, (name, form, params, left)
        if params != CSR.REPLAY_PARAMS[0]:
            continue
        smp = out["samples"].cpu().numpy().reshape(N * F, R4, T)
        d4 = dec.reshape(dec.shape[0], N * F, R4)
        compared = 0
        for k in (0, R4 - 1):
            uk = u.view(T - 1, N * F, R4)[:, :, k].contiguous()
            one = _csample(model, case, b, form, tables, 1, params, uk, trace=True)
            d1, l1, _ = _replay(one, form, LOOPS, table, tables, pad, uk, params, F, T, 1, (name, form, "R=1", k))
            assert l1 <= SR.CAP, (name, form, k, l1)
            n = min(d1.shape[0], d4.shape[0])
            both = d1[:n] & d4[:n, :, k]
            jstop = np.where(both.all(axis=0), n, (~both).argmax(axis=0))
            keep = np.arange(T)[None, :] <= jstop[:, None]
            assert (one["samples"].cpu().numpy()[keep] == smp[:, k][keep]).all(), (name, form, k)
            compared += int((jstop == n).sum())
        print(name, form, "identity (c): %d of %d rows compared to the end" % (compared, 2 * N * F))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_scores_against_the_teacher_forced_oracle(hip_lib, name):
    """Every draw's score against the fp64 oracle teacher-forced along that draw with the same byte rows applied (the FILL
    pattern of the decode's own constrained row): bound = the sum over the draw's steps of 2 tol(step) + 2^-16."""
    from test_parity_golden import _tol_along, _truth_along
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T = case["model"]["seq_len"]
    tables = _tables(name)
    form = CSR.GUARANTEE[name]
    out = _csample(model, case, b, form, tables, R4, CSR.REPLAY_PARAMS[0], _uniforms(lat, T, R4), trace=True)
    smp, lp, fin, steps = _check_layout(out, T, R4)
    rows = smp.shape[0] // R4
    logits = out["logits"].cpu().numpy().reshape(T - 1, rows, R4, -1)
    smp, fin = smp.reshape(rows, R4, T), fin.reshape(rows, R4)
    got = out["sample_scores"].cpu().numpy().astype(np.float64).reshape(rows, R4)
    worst = 0.0
    for k in range(R4):
        pred = np.ascontiguousarray(smp[:, k])
        truth, _, _ = _truth_along("constrain_sample:" + name, case, sd, lat, dict(predict=pred, steps=steps))
        tol_of = _tol_along(pred, steps, truth)
        tol = np.array([tol_of(s, truth[s]) for s in range(steps)])
        for r in range(rows):
            want = bound = 0.0
            for j in range(1, min(int(fin[r, k]), steps) + 1):
                live = logits[j - 1, r, k] > np.float32(FILL)
                lg = np.where(live, truth[j - 1, r], -np.inf)
                m = lg.max()
                want += (lg[smp[r, k, j]] - m) - math.log(np.exp(lg - m).sum())
                bound += 2 * tol[j - 1] + SR.LP_BAR
            err = abs(got[r, k] - want)
            worst = max(worst, err / bound) if bound else worst
            assert err <= bound, (name, form, k, r, got[r, k], want, bound)
    print(name, form, "R=%d: worst |score - oracle| / bound = %.3f" % (R4, worst))


def _yield(smp, dead, ni, edges, F, R):
    """(enclosed, dead-ended, unclosed) over the own-anchor draws."""
    enc = de = un = 0
    for w, n in enumerate(ni):
        for f in range(n):
            for k in range(R):
                r = (w * F + f) * R + k
                row = smp[r]
                face = faces._parallel_rows(row[None], TOK, n)
                ends = ((row >= TERM[0]) & (row < TERM[1])).any()
                if dead[r]:
                    de += 1
                elif ends and face and faces.is_face_enclosed(edges[w], face[0][1], CR.TOL):
                    enc += 1
                else:
                    un += 1
    return enc, de, un


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_the_guarantee_under_loops(hip_lib, name):
    """Every own-anchor draw that ends in a terminator without a dead-end flag passes faces.is_face_enclosed, in every form; no
    draw holds an edge twice; with constrain_exact a draw can only dead-end right after the edge that opened a loop.  The floor
    (constrain_ref.MIN_ENCLOSED of the own-anchor draws) is held under the form constrain_sample_ref.GUARANTEE names."""
    import exact_ref as ER
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, F = case["model"]["seq_len"], max(ni)
    tables = _tables(name)
    own = R4 * sum(ni)
    for form in FORMS:
        out = _csample(model, case, b, form, tables, R4, CSR.REPLAY_PARAMS[0], _uniforms(lat, T, R4))
        smp, _, fin, steps = _check_layout(out, T, R4)
        dead = out["sample_dead_end"].cpu().numpy() != 0
        ended = 0
        for w, n in enumerate(ni):
            for f in range(n):
                for k in range(R4):
                    r = (w * F + f) * R4 + k
                    row = smp[r]
                    idx = [int(t) - NTOK for t in row if t >= NTOK]
                    assert len(idx) == len(set(idx)), (name, form, w, f, k, row)                 # no draw holds an edge twice
                    if ((row >= TERM[0]) & (row < TERM[1])).any() and not dead[r]:
                        face = faces._parallel_rows(row[None], TOK, n)
                        if face:                                                                 # (an anchor below ntok that ends at once has no edge)
                            assert faces.is_face_enclosed(edges[w], face[0][1], CR.TOL), (name, form, w, f, k, row)
                            ended += 1
            if form == "exact":
                rows = slice(w * F * R4, (w * F + n) * R4)
                late = ER.late_dead_ends(smp[rows], dead[rows], NTOK, table[w])
                assert not late, (name, w, late, smp[rows][late])
        enc, de, un = _yield(smp, dead, ni, edges, F, R4)
        print(name, form, "tau=1 own-anchor draws enclosed / dead end / unclosed of %d: %d / %d / %d" % (own, enc, de, un))
        assert enc == ended
        if form == CSR.GUARANTEE[name]:
            assert ended >= CR.MIN_ENCLOSED * own, (name, form, ended, own)


@pytest.mark.gpu
def test_plan_and_order_independence_and_determinism(hip_lib):
    from faceformer_amd.hip import lib as L
    name, form, params = "par_small_ragged", "ahead", CSR.REPLAY_PARAMS[0]
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, N, F, R = case["model"]["seq_len"], len(ni), max(ni), R4
    tables, pad = _tables(name), _pad_of(b)
    u = _uniforms(lat, T, R, 9)
    whole = _csample(model, case, b, form, tables, R, params, u, trace=True, chunk_wireframes=0)
    again = _csample(model, case, b, form, tables, R, params, u, trace=True, chunk_wireframes=0)
    for k in ("samples", "sample_logprob", "sample_scores", "sample_dead_end", "predict", "logprob", "dead_end"):
        assert torch.equal(whole[k], again[k]), k                                    # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"]
    one = _csample(model, case, b, form, tables, R, params, u, trace=True, chunk_wireframes=1)      # (the tables are offset per chunk)
    dw, lw, _ = _replay(whole, form, LOOPS, table, tables, pad, u, params, F, T, R, "whole")
    do, lo, _ = _replay(one, form, LOOPS, table, tables, pad, u, params, F, T, R, "one")
    assert lw <= SR.CAP and lo <= SR.CAP, (lw, lo)

    def same(a, da, c, dc, what):
        n = min(da.shape[0], dc.shape[0])
        both = da[:n] & dc[:n]
        jstop = np.where(both.all(axis=0), n, (~both).argmax(axis=0))
        keep = np.arange(T)[None, :] <= jstop[:, None]
        assert (a[keep] == c[keep]).all(), what
        print(what, "%d of %d rows compared to the end" % (int((jstop == n).sum()), a.shape[0]))
    same(whole["samples"].cpu().numpy(), dw, one["samples"].cpu().numpy(), do, "chunk_wireframes = 1 against the whole batch:")
    # two wireframe orders, the uniforms and the tables moved with the wireframes
    eng, memory, mask, kv_len = model._encode(b)
    perm = list(reversed(range(N)))
    idx = torch.tensor(perm, device="cuda")
    moved = tuple(t.index_select(0, idx).contiguous() for t in tables)
    up = u.view(T - 1, N, F * R).index_select(1, idx).reshape(T - 1, -1).contiguous()
    kw = dict(T=T, F=F, flags=model.decode_flags, x3_min_rows=model.x3_min_rows, constrain=LOOPS, term_range=TERM, trace=True,
              constrain_samples=R, temperature=params[0], top_k=params[1], top_p=params[2], constrain_lookahead=True)
    fwd = eng.decode(memory, mask, kv_len, L.FF_PARALLEL, num_input=ni, follow_table=tables[0], close_dist=tables[1], cycle_len=tables[2],
                     uniforms=u, **kw)
    rev = eng.decode(memory.index_select(0, idx).contiguous(), mask.index_select(0, idx).contiguous(), kv_len.index_select(0, idx).contiguous(),
                     L.FF_PARALLEL, num_input=[ni[i] for i in perm], follow_table=moved[0], close_dist=moved[1], cycle_len=moved[2],
                     uniforms=up, **kw)
    df, lf, _ = _replay(fwd, form, LOOPS, table, tables, pad, u, params, F, T, R, "fwd")
    dr, lr, _ = _replay(rev, form, LOOPS, table[perm], moved, pad[perm], up, params, F, T, R, "rev")
    assert lf <= SR.CAP and lr <= SR.CAP, (lf, lr)
    back = np.argsort(perm)
    rp = rev["samples"].cpu().numpy().reshape(N, F * R, T)[back].reshape(N * F * R, T)
    drb = dr.reshape(dr.shape[0], N, F * R)[:, back].reshape(dr.shape[0], N * F * R)
    same(fwd["samples"].cpu().numpy(), df, rp, drb, "two wireframe orders:")


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "par_small_ragged"
    m = WP._bound(name, "default")
    b, table = WP._lattice(m)
    tables = _tables(name)
    u = SR.make_uniforms(b["num_input"], m.case["model"]["seq_len"], R4, CSR.REPLAY_SEED).cuda()
    call = lambda: _csample(m.model, m.case, b, "exact", tables, R4, CSR.REPLAY_PARAMS[1], u, trace=True)
    clean = call()
    clean.pop("engine", None)
    zero, d = WP._run([m], call, fill=RZ.ZERO, what="constrained sample after ZERO")
    poison, _ = WP._run([m], call, fill=RZ.POISON, what="constrained sample after POISON")
    WP._assert_equal(poison, zero, "constrained sample")
    WP._assert_equal(poison, clean, "constrained sample against the clean run")
    WP._assert_no_nan(poison, "constrained sample")
    assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size


@pytest.mark.gpu
def test_model_keys_in_batch_order_and_option_off(hip_lib):
    import ctypes as C
    from faceformer_amd.hip import lib as L
    case, z, model, gb, sd, lat, b, edges, table = _model("par_small_ragged")
    T = case["model"]["seq_len"]
    ni = lat["num_input"]
    N, F, R = len(ni), max(ni), 3
    order = sorted(range(N), key=lambda i: -ni[i])
    assert order != list(range(N))                                   # the premise: the model does reorder this batch
    idx = torch.tensor(order, device="cuda")
    by_hand = {k: (v.index_select(0, idx) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in b.items()}
    by_hand["num_input"] = [ni[i] for i in order]
    u = torch.rand((T - 1, N * F * R), generator=torch.Generator().manual_seed(21)).cuda()
    new = {"predict_samples", "predict_sample_logprob", "predict_sample_scores", "predict_sample_dead_end"}
    try:
        with torch.no_grad():
            off = model(dict(b))
            model.constrain = "loops"
            loops = model(dict(b))
            for look, exact in ((False, False), (True, False), (False, True)):
                model.constrain_lookahead, model.constrain_exact = look, exact
                model.constrain_samples, model.sample_seed, model.sort_by_edges = R, 5, True
                on, again = model(dict(b)), model(dict(b))
                model.sample_seed = 6
                other = model(dict(b))
                given = model(dict(b, sample_uniforms=u))
                model.sort_by_edges = False
                hand = model(dict(by_hand, sample_uniforms=u.view(T - 1, N, F * R).index_select(1, idx).reshape(T - 1, -1)))
                assert set(on) == set(loops) | new and not new & set(loops)
                smp, lp, sc, de = (on[k] for k in ("predict_samples", "predict_sample_logprob", "predict_sample_scores", "predict_sample_dead_end"))
                assert tuple(smp.shape) == tuple(lp.shape) == (N, F, R, T) and tuple(sc.shape) == tuple(de.shape) == (N, F, R)
                assert torch.equal(on["predict"], smp[:, :, 0]) and torch.equal(on["predict_logprob"], lp[:, :, 0])
                assert torch.equal(on["predict_dead_end"], de[:, :, 0])
                for k in new | {"predict"}:
                    assert torch.equal(on[k], again[k]), k                        # sample_seed reproduces
                    assert torch.equal(given[k].index_select(0, idx), hand[k]), k   # batch order: rows, uniforms and tables
                assert not torch.equal(on["predict_samples"], other["predict_samples"])
                assert model.last_decode_stats.get("constrain_samples") == R
            model.constrain_lookahead = model.constrain_exact = False
            model.constrain_samples, model.sort_by_edges = 0, True
            loops_again = model(dict(b))
    finally:
        model.constrain, model.constrain_samples, model.constrain_lookahead, model.constrain_exact = None, 0, False, False
        model.sample_seed, model.sort_by_edges = 0, True
    # option off: the constrained decode and the greedy decode are what they were
    for k in loops:
        if torch.is_tensor(loops[k]) and k.startswith("predict"):
            assert torch.equal(loops[k], loops_again[k]), k
    with torch.no_grad():
        assert torch.equal(model(dict(b))["predict"], off["predict"])
    eng = model.engine()
    prm = L.DecodeParams()
    prm.variant, prm.N, prm.L, prm.F, prm.T = L.FF_PARALLEL, N, case["model"]["L"], F, T
    prm.flags, prm.term_lo, prm.term_hi = model.decode_flags, TERM[0], TERM[1]
    ni_host = (C.c_int * N)(*ni)
    q = lambda entry, *a: getattr(hip_lib, entry)(C.byref(eng.model), C.byref(prm), ni_host, *a)
    assert q("ff_decode_constrained_sample_workspace_bytes", 2) > q("ff_decode_sample_workspace_bytes", 2) > 0
    assert q("ff_decode_constrained_sample_workspace_bytes", 65) == 0 == q("ff_decode_constrained_sample_workspace_bytes", 0)
