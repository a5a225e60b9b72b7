"""Opt-in sampling over the single-sequence decode (SurfaceFormer.sequence_samples): every refusal, the faces of the
draws and the CLI flags on the CPU (library untouched); the sequence form of the sampling step, the engine's mode, the model and
the CLI on the GPU, through the C ABI.  The rule is tests/sequence_sample_ref.py (sample_ref's draw; its own start / finish /
stop).

Bars (the issue's, none measured): a token must equal the fp64 rule's on every DECISIVE row / pair (sample_ref's guard band);
log-probabilities within 2^-16 + 2^-23 |lp| of fp64 on the kernel's own masked logits; scores within the sum over the draw's steps
of 2 tol(step) + 2^-16 of the fp64 oracle (tol: test_parity_golden._tol); at most 2 % of a case's pairs may be left out -- a
condition on the (golden, seed, parameters) triples, fixed on the CPU by tools/sequence_sample_left_out.py."""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import sequence_sample_ref as QR
from conftest import ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces
from faceformer_amd.hip.modes import SEQUENCE_SAMPLE, sequence_samples_value      # (the option: without it nothing here can pass)

TOK = token_ns()
TERM = (TOK.EOS, TOK.EOS + 1)
FILL = QR.FILL


# ---- CPU: the rule's own stop / finish ---------------------------------------------------------------------------------------------
def test_stop_and_finish_on_hand_written_rows():
    rows = np.array([[1, 5, 2, 6, 3, 0, 0, 0],       # SEP does not finish; EOS at 4
                     [1, 3, 0, 0, 0, 0, 0, 0],       # EOS at 1
                     [1, 2, 2, 2, 2, 3, 0, 0]])      # EOS at 5
    fin, steps = QR.stop_and_finish(rows, TOK.EOS)
    assert fin.tolist() == [4, 1, 5] and steps == 5
    assert QR.unfinished_after(rows, TOK.EOS).tolist() == [2, 2, 2, 1, 0, 0, 0]
    fin, steps = QR.stop_and_finish(np.array([[3, 5, 6, 7]]), TOK.EOS)      # position 0 never finishes; no EOS: T - 1 steps
    assert fin.tolist() == [4] and steps == 3


# ---- CPU: C ABI and binding --------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_pointer_sequence_sample", "ff_decode_sequence_sample_workspace_bytes", "ff_decode_sequence_sample")


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
    doc = header[header.index("sampling over the single-sequence decode"): header.index("int ff_pointer_sequence_sample(")]
    assert "model.py:161-167" in doc and "model.py:193-210" in doc and "model.py:191" in doc      # the reference call sites
    # the existing entries keep their signatures
    assert len(lib.SIGNATURES["ff_pointer_sample"][1]) == 27 and len(lib.SIGNATURES["ff_decode_sample"][1]) == 20


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


# ---- CPU: every refusal ------------------------------------------------------------------------------------------------------------
def test_mode_record_lies_outside_the_mode_table():
    from faceformer_amd.hip import modes
    assert modes.SEQUENCE_SAMPLE is SEQUENCE_SAMPLE and SEQUENCE_SAMPLE not in modes.MODES and "sequence_samples" not in modes.SWITCH
    assert [sequence_samples_value(v) for v in (None, 0, 1, 64)] == [0, 0, 1, 64]
    assert modes.SEQUENCE_SAMPLE.entry == "ff_decode_sequence_sample" and not modes.SEQUENCE_SAMPLE.term_range
    assert modes.SWITCH["num_samples"].seq2seq == "sampling for the single-sequence model is not implemented"      # the recorded text stays


def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes = {}
    memory = torch.zeros(2, 12, 64)
    ok = dict(T=5, F=1, sequence_samples=3, uniforms=torch.zeros(4, 6))
    with pytest.raises(ValueError, match="sequence_samples is a single-sequence option .* num_samples"):
        eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=2),
                   dict(constrain="no_repeat"), dict(constrain=0)):
        with pytest.raises(ValueError, match="sequence_samples excludes"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    with pytest.raises(ValueError, match="sequence_samples excludes stop_each_eos"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, flags=engine.DEFAULT_FLAGS | lib.FF_STOP_EACH_EOS, **ok)
    for bad in (65, -1, True, 2.0):
        with pytest.raises(ValueError, match="sequence_samples=.*must be in 1..64"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, sequence_samples=bad))
    for change in (dict(temperature=-1.0), dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(ValueError, match="sampling needs a finite temperature >= 0, top_k >= 0 and top_p in \\(0, 1\\]"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, **change))
    for bad in (None, torch.zeros(4, 5), torch.zeros(3, 6), torch.zeros(4, 6, dtype=torch.float64), [[0.0] * 6] * 4):
        with pytest.raises(ValueError, match="uniforms must be a float32 tensor of shape \\[4, 6\\]"):
            eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **dict(ok, uniforms=bad))
    # the recorded rejections of num_samples on the single-sequence variant stay what they are
    with pytest.raises(ValueError, match="num_samples is a parallel-variant option"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, T=5, F=1, num_samples=2, term_range=(1, 4), uniforms=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="num_samples is a parallel-variant option"):
        engine.check_sample_options(2, 1.0, 0, 1.0, lib.FF_SEQ2SEQ, False, False, False, None, None, False, 0, (1, 4))


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
    assert par.sequence_samples == 0
    par.sequence_samples = 2
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_samples is a SurfaceFormer option .* num_samples"):
        par.forward_eval(inputs)
    assert "predict" not in inputs
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.sequence_samples == 0
    seq.sequence_samples = 2
    seq.return_logprob = True
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_samples excludes return_logprob and an extra mask"):
        seq.forward_eval(_seq_inputs())
    seq.return_logprob = False
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_samples excludes return_logprob and an extra mask"):
        seq.forward_eval(_seq_inputs(extra_mask=torch.zeros(1, 8, dtype=torch.bool)))
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_samples"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    for attr, val, text in (("sequence_samples", 65, "sequence_samples=65: must be in 1..64"), ("sequence_samples", -3, "must be in 1..64"),
                            ("sample_temperature", -1.0, "sampling needs a finite temperature"), ("sample_top_p", 0.0, "sampling needs"),
                            ("sample_top_k", -2, "sampling needs")):
        old = getattr(seq, attr)
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match=text):
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, old)
    for bad in (torch.zeros(5, 3), torch.zeros(4, 2)):
        with torch.no_grad(), pytest.raises(ValueError, match="sample_uniforms must have shape \\[5, 2\\]"):
            seq.forward_eval(_seq_inputs(sample_uniforms=bad))
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_samples = 2
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_samples needs the native engine"):
            sub.forward_eval(_seq_inputs())
    # the recorded rejection of num_samples on this model stays, with or without the new option
    seq.num_samples = 2
    for R in (0, 2):
        seq.sequence_samples = R
        with torch.no_grad(), pytest.raises(ValueError, match="num_samples is a SurfaceFormer_Parallel option \\(sampling for the "
                                                              "single-sequence model is not implemented\\)"):
            seq.forward_eval(_seq_inputs())


def test_decode_sharded_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, sequence_samples=2)
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_samples"):
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_samples = 0
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: faces and the CLI ---------------------------------------------------------------------------------------------------------
def test_faces_of_the_draws_on_hand_written_rows():
    assert "parse_faces_samples_scored" in faces.__all__
    E = TOK.len      # edge e is token E + e
    smp = np.array([[1, E + 0, E + 1, 2, E + 1, E + 0, 2, E + 2, E + 3, 3, 0, 0],      # {0,1} twice in one draw, then {2,3}; EOS
                    [1, E + 1, E + 0, 2, 2, E + 2, E + 3, 3, 0, 0, 0, 0],              # {0,1} again, an empty piece, {2,3}
                    [1, E + 0, E + 2, 2, E + 4, E + 5, E + 6, E + 7, E + 8, E + 9, E + 1, E + 2]])      # no EOS: the last piece loses its last token
    lp = -np.ones(smp.shape) / 8.0
    lp[:, 0] = 0.0
    lp[0, 4:7] = -1.0 / 32.0                                                            # the second {0,1} of draw 0 scores better
    got = faces.parse_faces_samples_scored(smp, lp, 8, TOK)
    assert got == [(0, (0, 1), -3.0 / 32.0), (0, (2, 3), -0.375),                       # once, first place, best score
                   (0, (1, 0), -0.375), (0, (2, 3), -0.375),                            # (the piece [SEP] alone is skipped)
                   (0, (0, 2), -0.375), (0, (4, 5, 6, 7, 1), -1.0)]                     # (edges 8, 9 >= num_edges dropped; token E+2 cut off)
    uniq = faces.unique_faces_with_scores(got)
    assert uniq[0] == (0, (0, 1), -3.0 / 32.0, 2) and uniq[1] == (0, (2, 3), -0.375, 2)  # votes count DRAWS: 2, not 3
    assert [f[3] for f in uniq[2:]] == [1, 1]
    one = faces.parse_faces_scored(smp[0], lp[0], 8, TOK)                                # per draw it is parse_faces_scored
    assert [f[:2] for f in one] == [(0, (0, 1)), (0, (1, 0)), (0, (2, 3))]
    with pytest.raises(ValueError):
        faces.parse_faces_samples_scored(smp, lp[:2], 8, TOK)
    with pytest.raises(ValueError):
        faces.parse_faces_samples_scored(smp[0], lp[0], 8, TOK)


def test_cli_flags_reach_the_model_and_every_refusal_raises(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-samples", "8", "--temperature", "0.5", "--top-k", "16",
                                       "--top-p", "0.9", "--seed", "7"])
    assert (a.sequence_samples, a.temperature, a.top_k, a.top_p, a.seed, a.sample) == (8, 0.5, 16, 0.9, 7, 0)
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).sequence_samples == 0
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-samples", "8", "--seed", "7", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["sequence_samples"], kw["seed"], kw["sample"]) for kw in seen] == [(8, 7, 0), (0, 0, 0)]
    m = cli.configure_model(types.SimpleNamespace(), sequence_samples=8, temperature=0.5, top_k=16, top_p=0.9, seed=7)
    assert vars(m) == dict(sequence_samples=8, sample_temperature=0.5, sample_top_k=16, sample_top_p=0.9, sample_seed=7)
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    seqcfg = types.SimpleNamespace(model_class="SurfaceFormer")
    call = dict(out_dir="unused", device="cpu", model=object())
    with pytest.raises(ValueError, match="--sequence-samples applies to SurfaceFormer only .*--sample"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer_Parallel"), None, sequence_samples=2, **call)
    for bad in (65, -1, True):
        with pytest.raises(ValueError, match="--sequence-samples must be a count in 1..64"):
            run_test(seqcfg, None, sequence_samples=bad, **call)
    for kw in (dict(scores=True), dict(score_labels=True), dict(sample=2), dict(device_faces=True)):
        with pytest.raises(ValueError, match="--sequence-samples does not combine with --scores, --score-labels, --sample or --device-faces"):
            run_test(seqcfg, None, sequence_samples=2, **dict(call, **kw))
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sequence-samples is not implemented for multi-rank runs"):
        run_test(seqcfg, None, sequence_samples=2, dist_mod=world2, **call)
    with pytest.raises(ValueError, match="--sample applies to SurfaceFormer_Parallel only"):      # an existing text, unchanged
        run_test(seqcfg, None, sample=2, **call)


def test_record_gains_the_three_keys_and_is_todays_without_them(tmp_path):
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
    draws = np.zeros((3, 24), dtype=np.int64)
    draws[0, :8] = [1, E + 0, E + 1, E + 2, 2, E + 3, E + 4, 3]
    draws[1, :5] = [1, E + 2, E + 1, E + 0, 3]
    draws[2, :6] = [1, E + 5, E + 6, 2, E + 5, E + 6]                 # no EOS
    lp = np.where(draws > 0, -0.25, 0.0)
    lp[:, 0] = 0.0
    text, st = cli.record_of(cfg, raw, item, draws[0], False)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
    text2, st2 = cli.record_of(cfg, raw, item, draws[0], False, sequence_samples=(draws, lp))
    rec2 = json.loads(text2)
    assert list(rec2) == list(rec) + ["pred_sample_faces", "pred_sample_face_scores", "pred_sample_face_votes"] and st2 == st
    assert {k: rec2[k] for k in rec} == rec and text == cli.record_of(cfg, raw, item, draws[0], False, sequence_samples=None)[0]
    sc, votes = rec2["pred_sample_face_scores"], rec2["pred_sample_face_votes"]
    assert len(sc) == len(votes) == len(rec2["pred_sample_faces"]) == 3 and sc == sorted(sc, reverse=True)
    assert sorted(votes) == [1, 1, 2], rec2                           # {0,1,2}: draws 0 and 1; {3,4}: draw 0; {5,6}: draw 2, once


# ---- GPU: the operator (sequence form of the step) ----------------------------------------------------------------------------------
E_OP = 64


def _operator_case(B, S, R, seed, kind="mixed"):
    """-> raw logits [B, S], u [B + 3], row_id [B], fin [B], memory [W, S, E], mask [W, S], kv_len [W] for B rows of W = ceil(B / R)
    wireframes with different kv_len.  kind "mixed": Gaussian rows, of which row 0 is pushed onto EOS, row 1 onto SEP and row 2 is
    finished already; "sep": every row on SEP; "done": every row finished or on EOS."""
    g = torch.Generator().manual_seed(seed)
    W = (B + R - 1) // R
    logits = torch.randn(B, S, generator=g) * 3.0
    mask = torch.rand(W, S, generator=g) < 0.2
    mask[:, :TOK.len] = False
    kv = torch.tensor([S - (w % 2) for w in range(W)], dtype=torch.int32)      # S, S - 1, S, ...: neighbours differ (S >= 5)
    fin = torch.zeros(B, dtype=torch.int32)
    if kind == "mixed":
        logits[0, TOK.EOS] = 1.0e4
        if B > 1:
            logits[1, TOK.SEP] = 1.0e4
        if B > 2:
            fin[2] = 1
    elif kind == "sep":
        logits[:, TOK.SEP] = 1.0e4
    else:
        fin[::2] = 1
        logits[:, TOK.EOS] = 1.0e4
    u = torch.rand(B + 3, generator=g)
    row_id = torch.randperm(B + 3, generator=g)[:B].to(torch.int32)
    memory = torch.randn(W, S, E_OP, generator=g)
    return logits, u, row_id, fin, memory, mask, kv


def _run_operator(c, R, tau, K, P, counter=None):
    from faceformer_amd.hip import ops
    logits, u, row_id, fin, memory, mask, kv = c
    lg = logits.clone().cuda()
    res = ops.pointer_sequence_sample(lg, u.cuda(), temperature=tau, top_k=K, top_p=P, row_id=row_id.cuda(), fin=fin.cuda(),
                                      memory=memory.cuda(), mask=mask.to(torch.uint8).cuda(), kv_len=kv.cuda(), seqs_per_group=R,
                                      term_range=TERM, want_rows=True, counter=counter)
    return lg, res


OP_PARAMS = [(1.0, 0, 1.0), (0.8, 16, 0.9)]


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("S", [5, 65, 260])
def test_operator_sequence_form_against_the_numpy_rule(hip_lib, S, R):
    from faceformer_amd.hip import ops
    seen = left = 0
    for B in (1, 5, 8):
        for kind in ("mixed", "sep", "done"):
            for pi, (tau, K, P) in enumerate(OP_PARAMS):
                c = _operator_case(B, S, R, 1000 * S + 10 * B + pi, kind)
                logits, u, row_id, fin, memory, mask, kv = c
                counter = torch.zeros(1, dtype=torch.int32).cuda()
                lg, res = _run_operator(c, R, tau, K, P, counter)
                what = (S, B, R, kind, tau, K, P)
                own = lg.cpu()
                wf = torch.arange(B) // R
                dead = mask[wf] | (torch.arange(S)[None, :] >= kv[wf, None])
                unfin = fin.numpy() == 0
                assert torch.equal(own[unfin], logits.masked_fill(dead, FILL)[unfin]) and torch.equal(own[~unfin], logits[~unfin]), what
                tok, lp, dec, _ = QR.sample_rows(own.numpy().astype(np.float64), u.numpy()[row_id.long().numpy()], tau, K, P, fin=fin.numpy())
                got = res["next"].cpu().numpy().astype(np.int64)
                assert np.array_equal(got[dec], tok[dec]), (what, got, tok)
                seen, left = seen + B, left + int((~dec).sum())
                glp = res["logprob"].cpu().numpy().astype(np.float64)
                want_lp = np.array([0.0 if fin[b] else QR.logprob_of(own[b].numpy().astype(np.float64), got[b]) for b in range(B)])
                assert (np.abs(glp - want_lp) <= QR.LP_BAR + QR.EPS * np.abs(want_lp)).all(), (what, np.abs(glp - want_lp).max())
                assert (got[~unfin] == 0).all() and (glp[~unfin] == 0).all(), what
                want_fin = (~unfin) | (got == TOK.EOS)
                assert np.array_equal(res["fin"].cpu().numpy() != 0, want_fin), what
                assert int(counter.item()) == int((~want_fin).sum()), what                    # rows unfinished AFTER the step
                if kind == "mixed":
                    assert got[0] == TOK.EOS and (B < 2 or got[1] == TOK.SEP) and (B < 3 or got[2] == 0), (what, got)
                if kind == "sep":
                    assert (got == TOK.SEP).all() and int(counter.item()) == B, what          # every row on SEP: nothing stops
                if kind == "done":
                    assert int(counter.item()) == 0 and (got[unfin] == TOK.EOS).all(), what
                assert torch.equal(res["rows"], ops.gather_rows(memory.cuda(), res["next"], seqs_per_group=R)), what      # memory[b / R, tok]
                lg2, res2 = _run_operator(c, R, tau, K, P)
                assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what                       # two launches
    print("S=%d R=%d: %d of %d rows indecisive" % (S, R, left, seen))
    assert left <= QR.CAP * seen, (S, R, left, seen)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 65, 260])
def test_operator_sequence_form_with_temperature_zero_is_pointer_argmax(hip_lib, S):
    from faceformer_amd.hip import ops
    B, R = 8, 4
    g = torch.Generator().manual_seed(S)
    p = torch.randn(B, E_OP, generator=g)
    memory = torch.randn(B // R, S, E_OP, generator=g)
    memory[:, S // 2] = memory[:, 0]                                     # exact ties
    p[0] = 0.0
    mask = torch.zeros(memory.size(0), S, dtype=torch.uint8)
    ref = ops.pointer_argmax(p.cuda(), memory.cuda(), mask.cuda(), seqs_per_group=R, want_logits=True)
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    res = ops.pointer_sequence_sample(ref["logits"].clone(), torch.rand(B, generator=g).cuda(), temperature=0.0, top_k=3, top_p=0.5,
                                      mask=mask.cuda(), seqs_per_group=R, term_range=TERM, counter=counter)
    assert torch.equal(res["next"].cpu(), ref["next"].cpu())
    assert int(counter.item()) == int((ref["next"].cpu() != TOK.EOS).sum())


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


def _sampled(model, case, b, R, tau, K, P, u, **kw):
    return _decode(model, case, b, sequence_samples=R, temperature=tau, top_k=K, top_p=P, uniforms=u, return_pointer=False, **kw)


def _uniforms(case, b, R, seed):
    return QR.make_uniforms(b["input"].size(0), case["model"]["seq_len"], R, seed).cuda()


def _check_layout(out, T, R):
    """Finish positions, the stop step, the per-step counts and the zero padding against the rule applied to the decode's own
    tokens; scores against the fp64 sum of its own log-probabilities.  Returns (tokens, logprob, finish positions, steps)."""
    smp, lp = out["samples"].cpu().numpy(), out["sample_logprob"].cpu().numpy()
    assert smp.dtype == np.int64 and lp.dtype == np.float32 and smp.shape == lp.shape and smp.shape[1] == T
    assert (smp[:, 0] == TOK.SOS).all()
    fin, steps = QR.stop_and_finish(smp, TOK.EOS)
    assert out["steps"] == steps, (out["steps"], steps)
    assert out["step_counts"] == QR.unfinished_after(smp, TOK.EOS)[:steps].tolist()
    past = np.arange(T)[None, :] > np.minimum(fin, steps)[:, None]
    assert (smp[past] == 0).all() and (lp[past] == 0).all() and (lp[:, 0] == 0).all()
    assert np.isfinite(lp).all() and (lp <= 0).all()
    want = lp.astype(np.float64).sum(axis=1)
    got = out["sample_scores"].cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= QR.EPS * np.abs(want)).all()
    assert torch.equal(out["predict"], out["samples"].view(-1, R, T)[:, 0])
    return smp, lp.astype(np.float64), fin, steps


def _step_tol(z, own_logits, steps):
    """tol(step) of test_parity_golden over the golden's reference logits; behind the golden's own stop step (the golden ran the
    cumulative EOS rule) over the decode's own traced logits of the step."""
    from test_parity_golden import _tol
    zs = int(z["steps"])
    return np.array([_tol(z["logits"][s]) if s < zs else _tol(own_logits[s]) for s in range(steps)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_with_temperature_zero_is_the_greedy_decode_cut_at_every_eos(hip_lib, name):
    from faceformer_amd.hip import lib as L
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    greedy = _decode(model, case, b, logprob=True, trace=True, flags=model.decode_flags | L.FF_STOP_EACH_EOS)
    pred = greedy["predict"].cpu().numpy()
    steps = greedy["steps"]
    want = np.stack([faces.apply_own_stop_rule(pred[w], TOK, parallel=False) for w in range(pred.shape[0])])
    glp = np.stack([faces._apply_own_stop_rule_scored(pred[w], greedy["logprob"][w].cpu().numpy(), TOK, False)[1] for w in range(pred.shape[0])])
    tol = np.concatenate([[0.0], _step_tol(z, greedy["logits"].cpu().numpy(), steps), np.zeros(T)])[:T]
    for R in (1, 3):
        out = _sampled(model, case, b, R, 0.0, 4, 0.5, _uniforms(case, b, R, 3))
        assert out["steps"] == steps, (name, R, out["steps"], steps)
        smp = out["samples"].cpu().numpy().reshape(-1, R, T)
        for k in range(R):
            assert np.array_equal(smp[:, k], want), (name, R, k)
        lp = out["sample_logprob"].cpu().numpy().astype(np.float64).reshape(-1, R, T)
        err = np.abs(lp - glp[:, None, :])
        print(name, "R=%d steps=%d max |logprob - greedy logprob| = %.3g" % (R, steps, err.max()))
        assert (err <= (2 * tol + QR.LP_BAR)[None, None, :]).all(), (name, R, err.max())
        _check_layout(out, T, R)


@pytest.mark.gpu
def test_engine_rows_of_a_wireframe_share_its_memory_and_wireframes_differ(hip_lib):
    """Step 0: every draw holds SOS, so the R traced rows of one wireframe are one computation on that wireframe's memory, and the
    rows of two wireframes are not -- a wrong row-to-wireframe map (i % N, or i / R of another R) shows here."""
    from test_parity_golden import _tol
    name = "seq_small_gain4"
    case, z, model, b, sd, batch = _model(name)
    R = 3
    out = _sampled(model, case, b, R, 1.0, 0, 1.0, _uniforms(case, b, R, 2), trace=True)
    lg = out["logits"][0].cpu().numpy().reshape(-1, R, out["logits"].shape[-1])      # [N, R, S]
    tol = _tol(z["logits"][0])
    ref = z["logits"][0]                                                              # the golden's step-0 rows, one per wireframe
    for w in range(lg.shape[0]):
        live = lg[w, 0] > FILL
        for k in range(R):
            assert np.array_equal(lg[w, k] > FILL, live) and np.abs(lg[w, k][live] - lg[w, 0][live]).max() <= tol, (w, k)
            assert np.abs(lg[w, k][live] - ref[w][live]).max() <= tol, (w, k)         # ... and they are THIS wireframe's golden row
    both = (lg[0, 0] > FILL) & (lg[1, 0] > FILL)
    assert np.abs(lg[0, 0][both] - lg[1, 0][both]).max() > 100 * tol


def _replay(out, u, tau, K, P, T, R, what):
    """The numpy rule on the decode's own traced logits, pair by pair.  Returns (decisive [steps, rows] -- True also where the row
    was finished --, left-out share of the pairs)."""
    smp, lp, fin, steps = _check_layout(out, T, R)
    logits = out["logits"].cpu().numpy()
    un = u.cpu().numpy()
    dec = np.ones((steps, smp.shape[0]), dtype=bool)
    pairs = 0
    for j in range(steps):
        for r in np.flatnonzero(fin > j):
            res = QR.sample_row(logits[j, r].astype(np.float64), un[j, r], tau, K, P)
            pairs += 1
            dec[j, r] = res["decisive"]
            if res["decisive"]:
                assert smp[r, j + 1] == res["tok"], (what, j, int(r), int(smp[r, j + 1]), res["tok"])
            own = QR.logprob_of(logits[j, r].astype(np.float64), smp[r, j + 1])
            assert abs(lp[r, j + 1] - own) <= QR.LP_BAR + QR.EPS * abs(own), (what, j, int(r))
    return dec, (~dec).sum() / max(1, pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("params", QR.REPLAY_PARAMS)
@pytest.mark.parametrize("name", SMALL)
def test_engine_draws_replay_under_the_numpy_rule(hip_lib, name, params):
    """The (golden, seed, parameter set) triples are sequence_sample_ref's: kept on the CPU by tools/sequence_sample_left_out.py."""
    assert (name, params) in QR.KEPT, "not a kept triple"
    case, z, model, b, sd, batch = _model(name)
    T, R = case["model"]["seq_len"], QR.REPLAY_R
    u = _uniforms(case, b, R, QR.REPLAY_SEEDS[name])
    out = _sampled(model, case, b, R, *params, u, trace=True)
    dec, left = _replay(out, u, *params, T, R, (name, params))
    print(name, params, "steps=%d left-out (step, draw) pairs: %.2f %%" % (out["steps"], 100 * left))
    assert left <= QR.CAP, (name, params, left)


def _steered(case, b, R, plan):
    """Uniforms that steer every draw at temperature 1e6, where the live keys of a wireframe are drawn (all but) uniformly: key i
    of n live keys is drawn for u = (i + 0.5) / n, far from every prefix sum.  plan(step, w, k) -> the key to draw."""
    T = case["model"]["seq_len"]
    N = b["input"].size(0)
    n_live = [TOK.len + int(n) for n in case["n_edges"]]
    u = torch.zeros(T - 1, N * R)
    for s in range(T - 1):
        for w in range(N):
            for k in range(R):
                u[s, w * R + k] = (plan(s, w, k) + 0.5) / n_live[w]
    return u.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name,R", [("seq_small_gain4", 3), ("seq_small_repeat_eos", 3), ("seq_small_eos", 64)])
def test_engine_stop_rule_and_padding(hip_lib, name, R):
    """Every draw is steered: an edge, then SEP for ALL draws in one step (the parallel rule would stop there), then edges until
    draw k of wireframe w draws EOS at step 3 + (w + k) % 5 -- different finish positions, and the stop after the last one."""
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    N = b["input"].size(0)
    eos_step = lambda w, k: 3 + (w + k) % 5
    plan = lambda s, w, k: TOK.SEP if s == 1 else (TOK.EOS if s == eos_step(w, k) else TOK.len + (s + k) % 5)
    u = _steered(case, b, R, plan)
    out = _sampled(model, case, b, R, 1.0e6, 0, 1.0, u, trace=True)
    dec, left = _replay(out, u, 1.0e6, 0, 1.0, T, R, name)
    assert left == 0, left                                                           # the steering is decisive everywhere
    smp, lp, fin, steps = _check_layout(out, T, R)
    assert (smp[:, 2] == TOK.SEP).all() and steps > 2                                # all draws on SEP in one step: no stop
    want_fin = np.array([eos_step(w, k) + 1 for w in range(N) for k in range(R)])
    assert np.array_equal(fin, want_fin) and steps == want_fin.max()
    assert out["step_counts"][1] == N * R and out["step_counts"][-1] == 0
    for r in range(N * R):
        assert smp[r, fin[r]] == TOK.EOS and (smp[r, 1:fin[r]] != TOK.EOS).all()
    # a draw that never draws EOS runs T - 1 steps
    if R <= 3:
        u2 = _steered(case, b, R, lambda s, w, k: TOK.len + (s + k + w) % 5)
        out2 = _sampled(model, case, b, R, 1.0e6, 0, 1.0, u2)
        smp2, _, fin2, steps2 = _check_layout(out2, T, R)
        assert steps2 == T - 1 and (fin2 == T).all() and (smp2[:, 1:] >= TOK.len).all()


@pytest.mark.gpu
def test_engine_micro_batch_cut_and_repeatability(hip_lib):
    from test_parity_golden import _tol
    name = "seq_small_gain4"
    case, z, model, b, sd, batch = _model(name)
    T, R, params = case["model"]["seq_len"], 4, (1.0, 0, 1.0)
    u = _uniforms(case, b, R, 9)
    whole = _sampled(model, case, b, R, *params, u, trace=True)
    again = _sampled(model, case, b, R, *params, u, trace=True)
    for k in ("samples", "sample_logprob", "sample_scores", "predict", "logits"):
        assert torch.equal(whole[k], again[k]), k                                    # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"]
    one = _sampled(model, case, b, R, *params, u, trace=True, chunk_max_seqs=R)      # one wireframe per micro-batch
    assert len({int(v) // R for v in one["seq_of_row"].cpu()}) == b["input"].size(0)
    dw, lw = _replay(whole, u, *params, T, R, "whole")
    do, lo = _replay(one, u, *params, T, R, "one")
    assert lw <= QR.CAP and lo <= QR.CAP, (lw, lo)
    a, c = whole["samples"].cpu().numpy(), one["samples"].cpu().numpy()
    n = min(dw.shape[0], do.shape[0])
    both = dw[:n] & do[:n]
    jstop = np.where(both.all(axis=0), n, (~both).argmax(axis=0))
    keep = np.arange(T)[None, :] <= jstop[:, None]
    assert (a[keep] == c[keep]).all()                                                # equal on pairs decisive in both decodes
    full = jstop == n
    if full.all():
        assert whole["steps"] == one["steps"]
    if whole["steps"] == one["steps"]:
        fin = QR.stop_and_finish(a, TOK.EOS)[0]
        logits = whole["logits"].cpu().numpy()
        tol = np.array([_tol(logits[j][fin > j]) for j in range(n)])
        per = np.concatenate([[0.0], 2 * tol + QR.LP_BAR, np.zeros(T)])[:T]
        asc, csc = (o["sample_scores"].cpu().numpy().astype(np.float64) for o in (whole, one))
        bound = (per[None, :] * (np.arange(T)[None, :] <= np.minimum(fin, n)[:, None])).sum(axis=1) + QR.EPS * np.abs(asc)
        print("rows compared to the end: %d of %d; worst |dscore| / bound = %.3g"
              % (full.sum(), full.size, (np.abs(asc - csc)[full] / np.maximum(bound[full], 1e-300)).max() if full.any() else 0.0))
        assert (np.abs(asc - csc)[full] <= bound[full]).all()


def _oracle_scores(case, sd, batch, smp, fin, steps, R, seqs=None, max_steps=None):
    """fp64 scores of the oracle teacher-forced along every draw (oracle/refpath.py, forced=), on the GPU: -> (want [N', R], bound
    [N', R]) over the wireframes `seqs` (default: all) and the first `max_steps` steps (default: all)."""
    from oracle import refpath
    from test_parity_golden import _tol
    N, T = smp.shape[0] // R, smp.shape[1]
    seqs = list(range(N)) if seqs is None else list(seqs)
    n_steps = steps if max_steps is None else min(steps, max_steps)
    sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
    b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}
    draws = smp.reshape(N, R, T)
    want, bound = np.zeros((len(seqs), R)), np.zeros((len(seqs), R))
    for k in range(R):
        tr = {}
        refpath.seq2seq_forward_eval(sd64, dict(b64), num_head=case["model"]["H"], label_seq_length=T, token_sos=TOK.SOS, token_eos=TOK.EOS,
                                     trace=tr, forced=torch.from_numpy(np.ascontiguousarray(draws[:, k])), steps=n_steps,
                                     seqs=torch.tensor(seqs))
        truth = torch.stack(tr["logits"]).cpu().numpy()                              # [n_steps, N', S]
        for i, w in enumerate(seqs):
            for j in range(1, min(int(fin[w * R + k]), n_steps) + 1):
                row = truth[j - 1, i]
                lgt = np.where(row > np.finfo(np.float64).min, row, -np.inf)
                m = lgt.max()
                want[i, k] += (lgt[draws[w, k, j]] - m) - math.log(np.exp(lgt - m).sum())
                bound[i, k] += 2 * _tol(truth[j - 1]) + QR.LP_BAR
    return want, bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_engine_scores_against_the_teacher_forced_oracle(hip_lib, name):
    case, z, model, b, sd, batch = _model(name)
    T, R = case["model"]["seq_len"], 2
    out = _sampled(model, case, b, R, 1.0, 0, 1.0, _uniforms(case, b, R, 5))
    smp, lp, fin, steps = _check_layout(out, T, R)
    want, bound = _oracle_scores(case, sd, batch, smp, fin, steps, R)
    got = out["sample_scores"].cpu().numpy().astype(np.float64).reshape(-1, R)
    print(name, "worst |score - oracle| / bound = %.3f" % (np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    assert (np.abs(got - want) <= bound).all(), (name, got, want, bound)


@pytest.mark.gpu
def test_engine_scores_on_the_full_size_model_against_the_oracle(hip_lib):
    """seq_full_A4_gain4 at R = 2; the oracle side restricted to two wireframes and the first 24 steps (seqs= / steps=), the
    engine's side of the comparison being the sum of its own log-probabilities over those positions."""
    name = "seq_full_A4_gain4"
    case, z, model, b, sd, batch = _model(name)
    T, R, seqs, first = case["model"]["seq_len"], 2, [0, 3], 24
    out = _sampled(model, case, b, R, 1.0, 0, 1.0, _uniforms(case, b, R, 5))
    smp, lp, fin, steps = _check_layout(out, T, R)
    want, bound = _oracle_scores(case, sd, batch, smp, fin, steps, R, seqs=seqs, max_steps=first)
    n = min(steps, first)
    got = np.array([[lp[w * R + k, 1: min(int(fin[w * R + k]), n) + 1].sum() for k in range(R)] for w in seqs])
    print(name, "steps=%d worst |partial score - oracle| / bound = %.3f" % (steps, (np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    del _MODELS[name]


# ---- GPU: the model and the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_sequence_samples_adds_the_keys(hip_lib):
    case, z, model, b, sd, batch = _model("seq_small_gain4")
    T, N, R = case["model"]["seq_len"], b["input"].size(0), 3
    u = torch.rand((T - 1, N * R), generator=torch.Generator().manual_seed(21)).cuda()
    try:
        with torch.no_grad():
            off = model(dict(b))
            model.sequence_samples, model.sample_seed = R, 5
            on = model(dict(b))
            again = model(dict(b))
            model.sample_seed = 6
            other = model(dict(b))
            given = model(dict(b, sample_uniforms=u))
            model.stop_each_eos = True                                # not looked at
            given2 = model(dict(b, sample_uniforms=u))
            model.sample_seed, model.sample_temperature = 5, 0.0
            cold = model(dict(b))
    finally:
        model.sequence_samples, model.sample_seed, model.sample_temperature, model.stop_each_eos = 0, 0, 1.0, False
    new = {"predict_samples", "predict_sample_logprob", "predict_sample_scores"}
    assert set(on) == (set(off) - {"pointer"}) | new and not new & set(off)          # pointer is not published
    assert np.array_equal(off["predict"].cpu().numpy(), z["predict"])                 # off: today's decode
    smp, lp, sc = (on[k] for k in ("predict_samples", "predict_sample_logprob", "predict_sample_scores"))
    assert tuple(smp.shape) == tuple(lp.shape) == (N, R, T) and smp.dtype == torch.int64 and lp.dtype == torch.float32
    assert tuple(sc.shape) == (N, R) and tuple(on["predict"].shape) == (N, T)
    assert torch.equal(on["predict"], smp[:, 0]) and torch.equal(on["embedding"], off["embedding"])
    for k in new | {"predict"}:
        assert torch.equal(on[k], again[k]), k                        # sample_seed reproduces
        assert torch.equal(given[k], given2[k]), k
    assert not torch.equal(on["predict_samples"], other["predict_samples"])          # another seed differs somewhere
    # the seeded default IS torch.Generator(device).manual_seed(seed) handed in as sample_uniforms
    gen = torch.Generator(device="cuda").manual_seed(5)
    u5 = torch.rand((T - 1, N * R), generator=gen, device="cuda", dtype=torch.float32)
    with torch.no_grad():
        model.sequence_samples = R
        try:
            same = model(dict(b, sample_uniforms=u5))
        finally:
            model.sequence_samples = 0
    for k in new | {"predict"}:
        assert torch.equal(on[k], same[k]), k
    assert not torch.equal(given["predict_samples"], on["predict_samples"])
    # temperature 0: every draw is the greedy row cut at its EOS
    want = np.stack([faces.apply_own_stop_rule(r, TOK, parallel=False) for r in z["predict"]])
    if int(z["steps"]) == model.last_sample_stats["steps"]:
        assert np.array_equal(cold["predict_samples"].cpu().numpy(), np.repeat(want[:, None], R, axis=1))


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
    cold = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "cold"), sequence_samples=3, temperature=0.0)
    warm = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "warm"), sequence_samples=8, temperature=1.5, seed=3, batch_size=2)
    new = ["pred_sample_faces", "pred_sample_face_scores", "pred_sample_face_votes"]
    for fn in sorted(os.listdir(plain)):
        rec = json.load(open(os.path.join(plain, fn)))
        assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]
        rc, rw = (json.load(open(os.path.join(d, fn))) for d in (cold, warm))
        assert list(rc) == list(rec) + new and list(rw) == list(rec) + new
        assert {k: rc[k] for k in rec} == rec                         # temperature 0: draw 0 is the greedy decode
        assert all(v == 3 for v in rc["pred_sample_face_votes"]) and len(rc["pred_sample_faces"]) == len(rec["pred_faces"])
        assert all(1 <= v <= 8 for v in rw["pred_sample_face_votes"])
        assert rw["pred_sample_face_scores"] == sorted(rw["pred_sample_face_scores"], reverse=True)
