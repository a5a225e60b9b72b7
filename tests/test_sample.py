"""Opt-in temperature / top-k / top-p sampling of the parallel pointer decode: the numpy rule
(tests/sample_ref.py) on hand-written rows, the C ABI, the bindings and every rejected combination on the CPU; ff_pointer_sample
and the engine's sampled mode against that rule on the GPU.

Bars (the issue's, none measured): a token must equal the fp64 rule's on every DECISIVE row (sample_ref's guard band: the draw
u Z farther than beta from every prefix sum, the top-p target farther than beta from every value-group boundary); the kept set
under top-k is exact (fp32 compares only); log-probabilities within 2^-16 + 2^-23 |logprob| of fp64 on the kernel's own masked
logits (DESIGN.md 14's bar); at most 2 % of a case's rows / pairs may be indecisive."""
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
from conftest import ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces

TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
FILL = SR.FILL


# ---- CPU: the rule ----------------------------------------------------------------------------------------------------------------
def test_rule_on_hand_written_rows():
    l = np.array([0.0, math.log(2.0), math.log(2.0), FILL, math.log(4.0), 0.0])        # weights 1 2 2 - 4 1 (relative), Z = 10
    r = SR.sample_row(l, 0.0)
    assert r["tok"] == 0 and r["drew"] and abs(r["logprob"] - math.log(0.1)) < 1e-12  # u = 0: the first live key
    assert SR.sample_row(l, 0.29)["tok"] == 1 and SR.sample_row(l, 0.31)["tok"] == 2   # c = 1 3 5 - 9 10 (over Z = 10)
    assert SR.sample_row(l, 0.5)["tok"] == 4                                           # c[2] = 5 is not > 5
    assert SR.sample_row(l, 7.0)["tok"] == 5 and SR.clamp_u(7.0) == SR.U_MAX           # u clamped at the top: the last key
    assert SR.sample_row(l, -1.0)["tok"] == 0 and SR.clamp_u(float("nan")) == 0.0
    # ties at v_K are all kept: K = 2 -> {4} and both keys at log 2
    k2 = SR.sample_row(l, 0.99, K=2)
    assert k2["kept_k"].tolist() == [False, True, True, False, True, False] and k2["tok"] == 4
    assert SR.sample_row(l, 0.0, K=2)["tok"] == 1
    assert SR.sample_row(l, 0.3, K=1)["kept_k"].tolist() == [False, False, False, False, True, False]
    assert SR.sample_row(l, 0.3, K=5)["kept_k"].tolist() == (l > FILL).tolist()        # K >= |A|: everything live
    # top-p: the mass reaches P exactly at a group boundary -- groups 4 | 2 2 | 1 1 of 10: P = 0.8 is reached by the second
    lp2 = np.array([0.0, 1.0, 1.0, FILL, 2.0, 0.0])
    w = np.exp(lp2[[4, 1, 2, 0, 5]] - 2.0)
    at = (w[0] + w[1] + w[2]) / w.sum()
    assert SR.sample_row(lp2, 0.0, P=at)["kept"].tolist() == [False, True, True, False, True, False]
    assert not SR.sample_row(lp2, 0.0, P=at)["decisive"]                               # ... which an fp32 sum may miss
    assert SR.sample_row(lp2, 0.0, P=np.nextafter(at, 1.0) + 1e-9)["kept"].tolist() == (lp2 > FILL).tolist()
    assert SR.sample_row(lp2, 0.0, P=0.01)["kept"].tolist() == [False, False, False, False, True, False]
    # empty A, tau = 0, a finished row: no draw
    e = SR.sample_row(np.full(7, FILL), 0.3)
    assert e["tok"] == 0 and not e["drew"] and abs(e["logprob"] + math.log(7)) < 1e-12
    g = SR.sample_row(np.array([1.0, 3.0, 3.0, FILL]), 0.99, tau=0.0)
    assert g["tok"] == 1 and not g["drew"]
    f = SR.sample_row(l, 0.3, finished=True)
    assert f["tok"] == 0 and f["logprob"] == 0.0 and not f["drew"]
    # the log-probability is the model's, not the shaped distribution's
    assert abs(SR.sample_row(l, 0.3, tau=0.25, K=1)["logprob"] - math.log(0.4)) < 1e-12
    fin, steps = SR.stop_and_finish(np.array([[0, 5, 6, 1, 0, 0], [1, 0, 0, 0, 0, 0], [2, 7, 2, 0, 0, 0]]), TERM, TOK.len)
    assert fin.tolist() == [3, 0, 0] and steps == 3                          # (anchor 2 is a terminator token: quirk C-3)


# ---- CPU: C ABI and binding -------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_pointer_sample", "ff_decode_sample_workspace_bytes", "ff_decode_sample")


def test_header_declares_the_sample_entries_within_abi_105():
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    doc = header[header.index("top-p sampling over the pointer head"): header.index("int ff_pointer_sample(")]
    assert "model_para.py:173-179" in doc and "model_para.py:216-233" in doc
    assert re.search(r"typedef struct ff_sample_params \{\s*int num_samples;\s*float temperature;\s*int top_k;\s*float top_p;\s*"
                     r"const float\* uniforms;\s*int64_t\* samples;\s*float\* logprob;\s*float\* scores;\s*\} ff_sample_params;", code)

    def args(name):
        return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert args("ff_decode_sample").count(",") == args("ff_decode").count(",") + 1
    assert "const ff_sample_params* sample" in args("ff_decode_sample")
    assert args("ff_decode_sample_workspace_bytes").count(",") == args("ff_decode_workspace_bytes").count(",") + 1


def test_binding_lists_the_sample_entries_and_refuses_a_library_without_them(monkeypatch):
    from faceformer_amd.hip import lib
    assert lib.FF_ABI_VERSION == 105
    S = lib.SIGNATURES
    for name in NEW_ENTRIES:
        assert name in S, name
    assert len(S["ff_decode_sample"][1]) == len(S["ff_decode"][1]) + 1
    assert [f for f, _ in lib.SampleParams._fields_] == ["num_samples", "temperature", "top_k", "top_p", "uniforms", "samples",
                                                         "logprob", "scores"]
    import _ctypes
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


def test_every_rejected_combination_raises_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    ok = dict(num_samples=4, temperature=1.0, top_k=0, top_p=1.0, variant=lib.FF_PARALLEL, retire=False, return_pointer=False,
              no_stop=False, stop_callback=None, extra_mask=None, logprob=False, beam_width=0, term_range=TERM)
    engine.check_sample_options(**ok)
    engine.check_sample_options(**dict(ok, num_samples=64, temperature=0.0, top_k=10 ** 6, top_p=1e-6))
    for change in (dict(variant=lib.FF_SEQ2SEQ), dict(retire=True), dict(return_pointer=True), dict(no_stop=True),
                   dict(stop_callback=lambda c: False), dict(extra_mask=torch.zeros(1, 12, dtype=torch.uint8)), dict(logprob=True),
                   dict(beam_width=2), dict(num_samples=0), dict(num_samples=65), dict(term_range=None), dict(term_range=(4, 4))):
        with pytest.raises(ValueError, match="num_samples"):
            engine.check_sample_options(**dict(ok, **change))
    for change in (dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_k=-1),
                   dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan"))):
        with pytest.raises(ValueError, match="temperature"):
            engine.check_sample_options(**dict(ok, **change))


def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    """PathEngine.decode itself: the option check and the uniforms check come first, before any tensor is looked at on a device
    and before the library is loaded (an engine object without a constructor call: nothing of it may be needed)."""
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    memory = torch.zeros(2, 12, 64)
    ok = dict(T=5, F=4, num_input=[4, 3], num_samples=2, term_range=TERM, uniforms=torch.zeros(4, 2 * 4 * 2))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(8, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=65),
                   dict(term_range=None)):
        with pytest.raises(ValueError, match="num_samples"):
            eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, **change))
    with pytest.raises(ValueError, match="num_samples"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **ok)
    for change in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0)):
        with pytest.raises(ValueError, match="temperature"):
            eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, **change))
    for bad in (None, torch.zeros(4, 15), torch.zeros(3, 16), torch.zeros(4, 16, dtype=torch.float64), [[0.0] * 16] * 4):
        with pytest.raises(ValueError, match="uniforms must be a float32 tensor of shape \\[4, 16\\]"):
            eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, uniforms=bad))


def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _tiny_inputs():
    return {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
            "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}


def test_models_reject_num_samples_combinations_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        assert not model.engine_supported() and model.num_samples == 0
        model.num_samples = 2
        inputs = _tiny_inputs()
        with torch.no_grad(), pytest.raises(ValueError, match="num_samples needs the native engine"):
            model.forward_eval(inputs)
        assert "predict" not in inputs
    model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert (model.num_samples, model.sample_temperature, model.sample_top_k, model.sample_top_p, model.sample_seed) == (0, 1.0, 0, 1.0, 0)
    model.num_samples = 2
    for attr, val in (("retire_finished", True), ("beam_width", 2), ("return_logprob", True)):
        old = getattr(model, attr)
        setattr(model, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="num_samples excludes"):
            model.forward_eval(_tiny_inputs())
        setattr(model, attr, old)
    with torch.no_grad(), pytest.raises(ValueError, match="num_samples excludes"):
        model.forward_eval(dict(_tiny_inputs(), extra_mask=torch.zeros(1, 4, 8, dtype=torch.bool)))
    for attr, val in (("num_samples", 65), ("sample_temperature", -1.0), ("sample_top_p", 0.0), ("sample_top_k", -2)):
        old = getattr(model, attr)
        setattr(model, attr, val)
        with torch.no_grad(), pytest.raises(ValueError):
            model.forward_eval(_tiny_inputs())
        setattr(model, attr, old)
    with pytest.raises(ValueError, match="score\\(\\) excludes num_samples"):
        model.score(_tiny_inputs(), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    seq.num_samples = 2
    with torch.no_grad(), pytest.raises(ValueError, match="num_samples is a SurfaceFormer_Parallel option"):
        seq.forward_eval({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})


def test_decode_sharded_rejects_num_samples_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=2)
    with pytest.raises(ValueError, match="decode_sharded does not implement num_samples"):
        dist.decode_sharded(model, {}, NoDist())
    model.num_samples = 0
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: faces and the CLI -------------------------------------------------------------------------------------------------------
def test_scored_sample_faces_on_hand_written_samples():
    assert "parse_parallel_samples_scored" in faces.__all__
    smp = np.array([[[0, 4, 5, 1, 0, 0], [0, 4, 6, 2, 0, 0], [0, 5, 4, 1, 0, 0]],          # anchor 0: {0,1} drawn twice, {0,2} once
                    [[1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]]])         # anchor 1: finished at its start token
    scores = np.array([[-0.5, -1.5, -0.25], [0.0, 0.0, 0.0]])
    got = faces.parse_parallel_samples_scored(smp, scores, 4, TOK)
    assert got == [(0, (0, 1), -0.5), (1, (0, 2), -1.5), (0, (1, 0), -0.25)]
    uniq = faces.unique_faces_with_scores(got)
    assert uniq[0] == (0, (0, 1), -0.25, 2) and uniq[1][2:] == (-1.5, 1)                   # best score, votes over samples
    lp = np.zeros(smp.shape)
    lp[0, :, 1] = [-0.25, -1.0, -0.125]
    lp[0, :, 2] = [-0.25, -0.5, -0.125]
    assert faces.parse_parallel_samples_scored(smp, lp, 4, TOK) == got                     # per-position log-probabilities: summed
    with pytest.raises(ValueError):
        faces.parse_parallel_samples_scored(smp, scores[:1], 4, TOK)


def test_cli_sample_flags_reach_the_model_and_the_record_is_todays_without_them(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    from conftest import GOLDEN
    from faceformer_amd import datasets as D
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sample", "8", "--temperature", "0.5", "--top-k", "16", "--top-p",
                                       "0.9", "--seed", "7"])
    assert (a.sample, a.temperature, a.top_k, a.top_p, a.seed) == (8, 0.5, 16, 0.9, 7)
    d = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"])
    assert (d.sample, d.temperature, d.top_k, d.top_p, d.seed) == (0, 1.0, 0, 1.0, 0)
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sample", "8", "--temperature", "0.5", "--top-k", "16", "--top-p", "0.9", "--seed", "7", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["sample"], kw["temperature"], kw["top_k"], kw["top_p"], kw["seed"]) for kw in seen] == [(8, 0.5, 16, 0.9, 7), (0, 1.0, 0, 1.0, 0)]
    m = cli.configure_model(types.SimpleNamespace(), sample=8, temperature=0.5, top_k=16, top_p=0.9, seed=7)
    assert vars(m) == dict(num_samples=8, sample_temperature=0.5, sample_top_k=16, sample_top_p=0.9, sample_seed=7)
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    from faceformer_amd.config import default_cfg
    cfg = default_cfg()
    with pytest.raises(ValueError, match="--sample applies to SurfaceFormer_Parallel only"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer"), None, out_dir="unused", device="cpu", model=object(), sample=2)
    cfg = types.SimpleNamespace(model_class="SurfaceFormer_Parallel")
    for kw in (dict(scores=True), dict(beam=2), dict(retire_finished=True), dict(score_labels=True)):
        with pytest.raises(ValueError, match="--sample"):
            run_test(cfg, None, out_dir="unused", device="cpu", model=object(), sample=2, **kw)
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sample .* multi-rank"):
        run_test(cfg, None, out_dir="unused", device="cpu", model=object(), sample=2, dist_mod=world2)
    # the record: byte-identical without samples, three more keys with them, pred_faces untouched
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
    text, st = cli.record_of(cfg, smp["raw"], item, pred, True)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"] and rec["pred_faces"] == smp["pred_faces"]
    assert text == cli.record_of(cfg, smp["raw"], item, pred, True, None, None, None, None)[0]
    tokens = np.stack([pred, pred, pred], axis=1)                                            # R = 3: the greedy rows three times
    scores = np.stack([-np.arange(pred.shape[0]) / 8.0 - k for k in range(3)], axis=1)
    text2, st2 = cli.record_of(cfg, smp["raw"], item, pred, True, samples=(tokens, scores))
    rec2 = json.loads(text2)
    assert list(rec2) == list(rec) + ["pred_sample_faces", "pred_sample_face_scores", "pred_sample_face_votes"] and st2 == st
    assert {k: rec2[k] for k in rec} == rec
    sc, votes = rec2["pred_sample_face_scores"], rec2["pred_sample_face_votes"]
    assert len(sc) == len(votes) == len(rec2["pred_sample_faces"]) > 0 and sc == sorted(sc, reverse=True)
    assert all(v >= 3 and v % 3 == 0 for v in votes)


# ---- GPU: the operator ------------------------------------------------------------------------------------------------------------
PARAMS = [(1.0, 0, 1.0), (0.7, 0, 1.0), (1.0, 1, 1.0), (1.0, 5, 1.0), (1.0, "S+3", 1.0), (1.0, 0, 0.9), (0.5, 8, 0.5), (1e-3, 0, 1.0),
          (100.0, 0, 0.99)]
SPG = 3


def _seg_stats(x64):
    seg = x64.reshape(x64.shape[0], -1, 32)
    mean = seg.mean(dim=2)
    return torch.stack([mean, ((seg - mean[..., None]) ** 2).sum(dim=2)], dim=2)


def _operator_case(B, S, kind, seed):
    """-> raw logits [B, S], u [B + 5], row_id [B], fin [B], memory [W, S, E], mask [W, S], kv_len [W], dead [B, S].
    kind: Gaussian at scale 1 / 30, uniform in +-1e4.  Row B - 1 (when B >= 4): all-equal logits; wireframe 1 has one live key,
    the last wireframe (B = 9) none; wireframe 0 has 0 < kv_len = S - 2 < S (S >= 3); finished rows mixed in."""
    g = torch.Generator().manual_seed(seed)
    W = (B + SPG - 1) // SPG
    logits = {"g1": torch.randn(B, S, generator=g), "g30": torch.randn(B, S, generator=g) * 30.0,
              "u1e4": (torch.rand(B, S, generator=g) * 2 - 1) * 1.0e4}[kind]
    if B >= 4:
        logits[B - 1] = 0.75
    mask = torch.rand(W, S, generator=g) < 0.2
    mask[:, 0] = False
    kv = torch.tensor([max(1, S - 2 - 2 * w) for w in range(W)], dtype=torch.int32)
    if W > 1:
        mask[1] = True
        mask[1, min(S - 1, 2)] = False                                    # one live key
        kv[1] = S
    if W > 2:
        kv[W - 1] = 0                                                    # no live key
    wf = torch.arange(B) // SPG
    dead = mask[wf] | (torch.arange(S)[None, :] >= kv[wf, None])
    u = torch.rand(B + 5, generator=g)
    row_id = torch.randperm(B + 5, generator=g)[:B].to(torch.int32)
    fin = torch.zeros(B, dtype=torch.int32)
    if B > 2:
        fin[2] = 1
    memory = torch.randn(W, S, 64, generator=g)
    return logits, u, row_id, fin, memory, mask, kv, dead


def _run_operator(c, tau, K, P, **kw):
    from faceformer_amd.hip import ops
    logits, u, row_id, fin, memory, mask, kv, dead = c
    lg = logits.clone().cuda()
    res = ops.pointer_sample(lg, u.cuda(), temperature=tau, top_k=K, top_p=P, row_id=row_id.cuda(), fin=fin.cuda(),
                             memory=memory.cuda(), mask=mask.to(torch.uint8).cuda(), kv_len=kv.cuda(), seqs_per_group=SPG,
                             term_range=TERM, want_rows=True, want_stats=True, **kw)
    return lg, res


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 63, 64, 65, 260, 1028])
def test_operator_against_the_numpy_rule(hip_lib, S):
    from faceformer_amd.hip import ops
    for pi, (tau, K, P) in enumerate(PARAMS):
        K = S + 3 if K == "S+3" else K
        rows_seen = rows_left = 0                                         # a CASE is one (S, parameter set): all its rows
        for B in (1, 3, 4, 9):
            for kind in ("g1", "g30", "u1e4"):
                c = _operator_case(B, S, kind, 1000 * S + 10 * B + pi)
                logits, u, row_id, fin, memory, mask, kv, dead = c
                counter = torch.zeros(1, dtype=torch.int32).cuda()
                lg, res = _run_operator(c, tau, K, P, counter=counter, ge_bound=TOK.len)
                own = lg.cpu()
                unfin = fin.numpy() == 0
                assert torch.equal(own[unfin], logits.masked_fill(dead, FILL)[unfin])          # masked in place; finished rows untouched
                assert torch.equal(own[~unfin], logits[~unfin])
                tok, lp, dec, kept_k = SR.sample_rows(own.numpy().astype(np.float64), u.numpy()[row_id.long().numpy()], tau, K, P,
                                                      fin=fin.numpy())
                got = res["next"].cpu().numpy().astype(np.int64)
                what = (S, B, tau, K, P, kind)
                live_row = unfin & ~dead.all(dim=1).numpy()
                assert kept_k[np.arange(B), got][live_row].all(), what                        # top-k: never a key outside the kept set
                assert np.array_equal(got[dec], tok[dec]), (what, got, tok)
                rows_seen, rows_left = rows_seen + B, rows_left + int((~dec).sum())
                glp = res["logprob"].cpu().numpy().astype(np.float64)
                want_lp = np.array([0.0 if fin[b] else SR.logprob_of(own[b].numpy().astype(np.float64), got[b]) for b in range(B)])
                assert (np.abs(glp - want_lp) <= SR.LP_BAR + SR.EPS * np.abs(want_lp)).all(), (what, np.abs(glp - want_lp).max())
                assert (got[~unfin] == 0).all() and (glp[~unfin] == 0).all()
                want_fin = (~unfin) | ((got >= TERM[0]) & (got < TERM[1]))
                assert np.array_equal(res["fin"].cpu().numpy() != 0, want_fin), what
                assert int(counter.item()) == int((unfin & (got >= TOK.len)).sum()), what
                # next rows and statistics: bit-equal to the gather's / the forced operator's for the same token
                tk = res["next"]
                assert torch.equal(res["rows"], ops.gather_rows(memory.cuda(), tk, seqs_per_group=SPG)), what
                forced = ops.pointer_forced(logits.clone().cuda(), tk, memory.cuda(), mask.to(torch.uint8).cuda(), kv.cuda(),
                                            seqs_per_group=SPG, want_rows=True, want_stats=True)
                assert torch.equal(res["rows"], forced["rows"]) and torch.equal(res["stats"], forced["stats"]), what
                lg2, res2 = _run_operator(c, tau, K, P)                                      # two launches: bit-equal
                assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
        print("S=%d tau=%g K=%d P=%g: %d of %d rows indecisive" % (S, tau, K, P, rows_left, rows_seen))
        assert rows_left <= SR.CAP * rows_seen, (S, tau, K, P, rows_left, rows_seen)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 65, 260])
def test_operator_with_temperature_zero_is_pointer_argmax(hip_lib, S):
    from faceformer_amd.hip import ops
    B, E = 9, 64
    g = torch.Generator().manual_seed(S)
    p = torch.randn(B, E, generator=g)
    memory = torch.randn((B + SPG - 1) // SPG, S, E, generator=g)
    memory[:, S // 2] = memory[:, 0]                                     # exact ties: keys 0 and S // 2 give the same logit
    p[0] = 0.0                                                           # a row of all-equal (zero) logits
    mask = torch.zeros(memory.size(0), S, dtype=torch.uint8)
    ref = ops.pointer_argmax(p.cuda(), memory.cuda(), mask.cuda(), seqs_per_group=SPG, want_logits=True)
    tok_ref, logits = ref["next"].cpu(), ref["logits"].clone()          # the argmax launch's own masked logits, sampled at tau = 0
    res = ops.pointer_sample(logits, torch.rand(B, generator=g).cuda(), temperature=0.0, top_k=3, top_p=0.5, mask=mask.cuda(),
                             seqs_per_group=SPG, term_range=TERM)
    own = logits.cpu()
    want = np.array([int(np.flatnonzero(own[b].numpy() == own[b].numpy().max())[0]) for b in range(B)])
    assert np.array_equal(res["next"].cpu().numpy(), want)                # the lowest index on ties, on the kernel's own logits
    assert res["next"][0].item() == 0 and tok_ref[0].item() == 0
    assert np.array_equal(want, tok_ref.numpy())                         # ops.pointer_argmax exactly, ties included


@pytest.mark.gpu
def test_operator_frequencies_follow_the_fp64_probabilities(hip_lib):
    from faceformer_amd.hip import ops
    S, B = 65, 65536
    g = torch.Generator().manual_seed(11)
    row = torch.randn(S, generator=g)
    u = torch.rand(B, generator=torch.Generator().manual_seed(12))
    res = ops.pointer_sample(row[None, :].repeat(B, 1).cuda(), u.cuda(), temperature=1.0, term_range=TERM)
    counts = np.bincount(res["next"].cpu().numpy(), minlength=S).astype(np.float64)
    p = np.exp(row.numpy().astype(np.float64))
    p /= p.sum()
    sigma = np.sqrt(B * p * (1 - p))
    z = np.abs(counts - B * p) / sigma
    print("frequency check: worst |count - N p| / sigma = %.2f over %d keys" % (z.max(), S))
    assert (z <= 5).all(), z.max()


@pytest.mark.gpu
def test_operator_refuses_bad_arguments(hip_lib):
    from faceformer_amd.hip import ops
    lg, u = torch.zeros(2, 9).cuda(), torch.zeros(2).cuda()
    for kw in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(row_id=torch.tensor([0, 2], dtype=torch.int32).cuda())):
        with pytest.raises(ValueError):
            ops.pointer_sample(lg, u, **kw)
    with pytest.raises(ValueError):
        ops.pointer_sample(lg, u[:1])


# ---- GPU: the engine --------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        _MODELS[name] = (case, z, build_model(case, sd, "cuda"), batch_to(batch, "cuda"), sd, batch)
    return _MODELS[name]


def _decode(model, case, batch, **kw):
    from test_logprob import _decode as decode
    return decode(model, case, batch, **kw)


def _uniforms(case, b, R, seed):
    return SR.make_uniforms(b["num_input"], case["model"]["seq_len"], R, seed).cuda()


def _sampled(model, case, b, R, tau, K, P, u, **kw):
    return _decode(model, case, b, num_samples=R, temperature=tau, top_k=K, top_p=P, uniforms=u, term_range=TERM, **kw)


def _check_layout(out, T):
    """Finish positions, the stop step and the zero padding against the rule applied to the decode's own tokens; scores against
    the fp64 sum of its own log-probabilities.  Returns (tokens, logprob, finish positions, steps)."""
    smp, lp = out["samples"].cpu().numpy(), out["sample_logprob"].cpu().numpy()
    assert smp.dtype == np.int64 and lp.dtype == np.float32 and smp.shape == lp.shape and smp.shape[1] == T
    fin, steps = SR.stop_and_finish(smp, TERM, TOK.len)
    assert out["steps"] == steps
    past = np.arange(T)[None, :] > np.minimum(fin, steps)[:, None]
    assert (smp[past] == 0).all() and (lp[past] == 0).all() and (lp[:, 0] == 0).all()
    assert np.isfinite(lp).all() and (lp <= 0).all()
    want = lp.astype(np.float64).sum(axis=1)
    got = out["sample_scores"].cpu().numpy().astype(np.float64)
    assert (np.abs(got - want) <= SR.EPS * np.abs(want)).all()                       # fp64 accumulator, rounded once
    return smp, lp.astype(np.float64), fin, steps


def _replay(out, u, tau, K, P, T, what):
    """The numpy rule on the decode's own traced logits, pair by pair (the trace follows the decode's own prefix, so pairs are
    independent).  Returns (decisive [steps, rows] -- True also where the row was finished --, left-out share of the pairs)."""
    smp, lp, fin, steps = _check_layout(out, T)
    logits = out["logits"].cpu().numpy()
    un = u.cpu().numpy()
    rows = smp.shape[0]
    dec = np.ones((steps, rows), dtype=bool)
    pairs = 0
    for j in range(steps):
        for r in np.flatnonzero(fin > j):
            res = SR.sample_row(logits[j, r].astype(np.float64), un[j, r], tau, K, P)
            pairs += 1
            dec[j, r] = res["decisive"]
            if res["decisive"]:
                assert smp[r, j + 1] == res["tok"], (what, j, int(r), int(smp[r, j + 1]), res["tok"])
            own = SR.logprob_of(logits[j, r].astype(np.float64), smp[r, j + 1])
            assert abs(lp[r, j + 1] - own) <= SR.LP_BAR + SR.EPS * abs(own), (what, j, int(r))
    return dec, (~dec).sum() / max(1, pairs)


ENGINE_GOLDENS = ["par_small_gain4", "par_small_ragged", "par_full_n40_gain4"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_with_temperature_zero_is_the_retired_greedy_decode(hip_lib, name):
    from test_parity_golden import _tol
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    greedy = _decode(model, case, b, logprob=True)
    pred = greedy["predict"].cpu().numpy()
    want, steps = faces.retired_view(pred, TOK, return_steps=True)
    keep = faces._retired_keep(pred, TOK)
    glp = greedy["logprob"].cpu().numpy().astype(np.float64) * keep
    tol = np.array([0.0] + [_tol(z["logits"][s]) for s in range(min(steps, int(z["steps"])))] + [0.0] * T)[:T]
    for R in (1, 3):
        out = _sampled(model, case, b, R, 0.0, 4, 0.5, _uniforms(case, b, R, 3))
        assert out["steps"] == steps, (name, R)
        smp = out["samples"].cpu().numpy().reshape(-1, R, T)
        for k in range(R):
            assert np.array_equal(smp[:, k], want), (name, R, k)
        assert torch.equal(out["predict"], out["samples"].view(-1, R, T)[:, 0])
        lp = out["sample_logprob"].cpu().numpy().astype(np.float64).reshape(-1, R, T)
        err = np.abs(lp - glp[:, None, :])
        print(name, "R=%d steps=%d max |logprob - greedy logprob| = %.3g" % (R, steps, err.max()))
        assert (err <= (2 * tol + SR.LP_BAR)[None, None, :]).all(), (name, R, err.max())
        _check_layout(out, T)


@pytest.mark.gpu
@pytest.mark.parametrize("params", SR.REPLAY_PARAMS)
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_samples_replay_under_the_numpy_rule(hip_lib, name, params):
    """The (golden, seed, parameter set) triples are sample_ref's: fixed on the CPU by tools/sample_left_out.py."""
    case, z, model, b, sd, batch = _model(name)
    T, R = case["model"]["seq_len"], SR.REPLAY_R
    u = _uniforms(case, b, R, SR.REPLAY_SEEDS[name])
    out = _sampled(model, case, b, R, *params, u, trace=True)
    dec, left = _replay(out, u, *params, T, (name, params))
    print(name, params, "steps=%d left-out (step, sequence) pairs: %.2f %%" % (out["steps"], 100 * left))
    assert left <= SR.CAP, (name, params, left)
    assert torch.equal(out["predict"], out["samples"].view(-1, R, T)[:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_sample_scores_against_the_teacher_forced_oracle(hip_lib, name):
    """Every sample's score against the fp64 oracle teacher-forced along that sample: bound = the sum over the sample's steps
    of 2 tol(step) + 2^-16 (DESIGN.md 13's derivation)."""
    case, z, model, b, sd, batch = _model(name)
    R = 2
    out = _sampled(model, case, b, R, 1.0, 0, 1.0, _uniforms(case, b, R, 5))
    _check_scores_against_oracle(name, case, sd, batch, out, R)


def _check_scores_against_oracle(name, case, sd, batch, out, R, step_tol=None, what=None):
    """The body of test_engine_sample_scores_against_the_teacher_forced_oracle for a sampled decode `out`.  step_tol(pred, steps,
    truth) -> fn(step, oracle logits of the step): the tolerance of a step along the tokens `pred` (default:
    test_parity_golden._tol_along).  Returns the worst error / bound."""
    from test_parity_golden import _tol_along, _truth_along
    what = what or name
    T = case["model"]["seq_len"]
    smp, lp, fin, steps = _check_layout(out, T)
    smp = smp.reshape(-1, R, T)
    got = out["sample_scores"].cpu().numpy().astype(np.float64).reshape(-1, R)
    fin = fin.reshape(-1, R)
    worst = 0.0
    for k in range(R):
        pred = np.ascontiguousarray(smp[:, k])
        truth, _, _ = _truth_along(name, case, sd, batch, dict(predict=pred, steps=steps))
        tol_of = (step_tol or _tol_along)(pred, steps, truth)
        tol = np.array([tol_of(s, truth[s]) for s in range(steps)])
        for r in range(smp.shape[0]):
            want, bound = 0.0, 0.0
            for j in range(1, min(int(fin[r, k]), steps) + 1):
                lg = np.where(truth[j - 1, r] > np.finfo(np.float64).min, truth[j - 1, r], -np.inf)
                m = lg.max()
                want += (lg[smp[r, k, j]] - m) - math.log(np.exp(lg - m).sum())
                bound += 2 * tol[j - 1] + SR.LP_BAR
            err = abs(got[r, k] - want)
            worst = max(worst, err / bound) if bound else worst
            assert err <= bound, (what, k, r, got[r, k], want, bound)
    print(what, "R=%d: worst |score - oracle| / bound = %.3f" % (R, worst))
    return worst


def _same_on_decisive_pairs(A, dA, fin_a, c, clp, csc, c_steps, dB, T, what):
    """Two decodes of the same sequences with the same uniforms (A: the out dict of one; c / clp / csc: tokens, log-probabilities
    and scores of the other in A's row order; dA / dB: _replay's decisive masks).  A row's tokens must be equal up to and including
    the position decided by its first pair that is indecisive in either decode -- every pair decisive in both is compared.  Rows
    compared to the end: per-position log-probabilities within 2 tol(step) + 2^-16 and scores within the sum of that over the
    row's steps (tol of test_parity_golden on A's own traced logits of the step; the two plans are two fp32 evaluations of the
    same logits).  Returns the number of rows compared to the end."""
    from test_parity_golden import _tol
    a, alp = A["samples"].cpu().numpy(), A["sample_logprob"].cpu().numpy().astype(np.float64)
    asc = A["sample_scores"].cpu().numpy().astype(np.float64)
    n = min(dA.shape[0], dB.shape[0])
    both = dA[:n] & dB[:n]
    jstop = np.where(both.all(axis=0), n, (~both).argmax(axis=0))
    keep = np.arange(T)[None, :] <= jstop[:, None]
    assert (a[keep] == c[keep]).all(), what
    full = jstop == n
    if full.all():
        assert A["steps"] == c_steps, what
    if A["steps"] != c_steps:
        return 0
    logits = A["logits"].cpu().numpy()
    tol = np.array([_tol(logits[j][fin_a > j]) for j in range(n)])
    per = np.concatenate([[0.0], 2 * tol + SR.LP_BAR, np.zeros(T)])[:T]
    assert (np.abs(alp[full] - clp[full]) <= per[None, :] + SR.EPS * np.abs(alp[full])).all(), what
    bound = (per[None, :] * (np.arange(T)[None, :] <= np.minimum(fin_a, n)[:, None])).sum(axis=1) + SR.EPS * np.abs(asc)
    err = np.abs(asc - csc)
    print(what, "rows compared to the end: %d of %d; worst |dscore| / bound = %.3g" % (full.sum(), full.size, (err[full] / np.maximum(bound[full], 1e-300)).max()))
    assert (err[full] <= bound[full]).all(), what
    return int(full.sum())


@pytest.mark.gpu
def test_micro_batching_determinism_and_batch_order(hip_lib):
    name = "par_small_ragged"
    case, z, model, b, sd, batch = _model(name)
    T, R, params = case["model"]["seq_len"], 4, (1.0, 0, 1.0)
    u = _uniforms(case, b, R, 9)
    whole = _sampled(model, case, b, R, *params, u, trace=True, chunk_wireframes=0)
    again = _sampled(model, case, b, R, *params, u, trace=True, chunk_wireframes=0)
    for k in ("samples", "sample_logprob", "sample_scores", "predict"):
        assert torch.equal(whole[k], again[k]), k                                    # one plan, two runs: bit-equal
    one = _sampled(model, case, b, R, *params, u, trace=True, chunk_wireframes=1)
    dw, lw = _replay(whole, u, *params, T, "whole")
    do, lo = _replay(one, u, *params, T, "one")
    assert lw <= SR.CAP and lo <= SR.CAP, (lw, lo)                                   # left-out pairs of either plan: the issue's cap
    fin_w = SR.stop_and_finish(whole["samples"].cpu().numpy(), TERM, TOK.len)[0]
    _same_on_decisive_pairs(whole, dw, fin_w, one["samples"].cpu().numpy(), one["sample_logprob"].cpu().numpy().astype(np.float64),
                            one["sample_scores"].cpu().numpy().astype(np.float64), one["steps"], do, T,
                            "chunk_wireframes = 1 against the whole batch:")
    # two wireframe orders, the uniforms moved with the wireframes: per wireframe the same tokens
    eng, memory, mask, kv_len = model._encode(b)
    ni = [int(v) for v in b["num_input"]]
    N, F = len(ni), max(ni)
    perm = list(reversed(range(N)))
    idx = torch.tensor(perm, device="cuda")
    up = u.view(T - 1, N, F * R).index_select(1, idx).reshape(T - 1, -1).contiguous()
    from faceformer_amd.hip import lib as L
    kw = dict(T=T, F=F, flags=model.decode_flags, x3_min_rows=model.x3_min_rows, num_samples=R, temperature=params[0],
              top_k=params[1], top_p=params[2], term_range=TERM, trace=True)
    fwd = eng.decode(memory, mask, kv_len, L.FF_PARALLEL, num_input=ni, uniforms=u, **kw)
    rev = eng.decode(memory.index_select(0, idx).contiguous(), mask.index_select(0, idx).contiguous(), kv_len.index_select(0, idx).contiguous(),
                     L.FF_PARALLEL, num_input=[ni[i] for i in perm], uniforms=up, **kw)
    df, lf = _replay(fwd, u, *params, T, "fwd")
    dr, lr = _replay(rev, up, *params, T, "rev")
    assert lf <= SR.CAP and lr <= SR.CAP, (lf, lr)
    back = torch.tensor(perm).argsort()

    def in_fwd_order(t, cols):                                                        # [.., N * F * R, ..] of rev, wireframes put back
        return t.cpu().view(N, F * R, *cols).index_select(0, back).reshape(N * F * R, *cols).numpy()
    drb = torch.from_numpy(dr).view(dr.shape[0], N, F * R).index_select(1, back).reshape(dr.shape[0], -1).numpy()
    fin_f = SR.stop_and_finish(fwd["samples"].cpu().numpy(), TERM, TOK.len)[0]
    _same_on_decisive_pairs(fwd, df, fin_f, in_fwd_order(rev["samples"], (T,)), in_fwd_order(rev["sample_logprob"], (T,)).astype(np.float64),
                            in_fwd_order(rev["sample_scores"], ()).astype(np.float64), rev["steps"], drb, T, "two wireframe orders:")


@pytest.mark.gpu
def test_model_num_samples_adds_the_keys_in_batch_order(hip_lib):
    case, z, model, b, sd, batch = _model("par_small_ragged")
    T = case["model"]["seq_len"]
    ni = [int(n) for n in b["num_input"]]
    N, F, R = len(ni), max(ni), 3
    order = sorted(range(N), key=lambda i: -ni[i])
    assert order != list(range(N))                                   # the premise: the model does reorder this batch
    idx = torch.tensor(order, device="cuda")
    by_hand = {k: (v.index_select(0, idx) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in b.items()}
    by_hand["num_input"] = [ni[i] for i in order]
    u = torch.rand((T - 1, N * F * R), generator=torch.Generator().manual_seed(21)).cuda()
    try:
        with torch.no_grad():
            off = model(dict(b))
            keys_off = set(off)
            model.num_samples, model.sample_seed = R, 5
            on = model(dict(b))
            again = model(dict(b))
            model.sample_seed = 6
            other = model(dict(b))
            given = model(dict(b, sample_uniforms=u))
            model.sort_by_edges = False
            hand = model(dict(by_hand, sample_uniforms=u.view(T - 1, N, F * R).index_select(1, idx).reshape(T - 1, -1)))
    finally:
        model.num_samples, model.sample_seed, model.sort_by_edges = 0, 0, True
    new = {"predict_samples", "predict_sample_logprob", "predict_sample_scores"}
    assert set(on) == keys_off | new and not new & keys_off
    smp, lp, sc = (on[k] for k in ("predict_samples", "predict_sample_logprob", "predict_sample_scores"))
    assert tuple(smp.shape) == tuple(lp.shape) == (N, F, R, T) and smp.dtype == torch.int64 and tuple(sc.shape) == (N, F, R)
    assert torch.equal(on["predict"], smp[:, :, 0])
    assert np.array_equal(smp[:, :, :, 0].cpu().numpy(), np.repeat(off["predict"][:, :, :1].cpu().numpy(), R, axis=2))
    for k in new | {"predict"}:
        assert torch.equal(on[k], again[k]), k                        # sample_seed reproduces
    assert not torch.equal(on["predict_samples"], other["predict_samples"])          # another seed differs somewhere
    # batch order, the sort_by_edges permutation undone -- of the rows AND of the uniforms' columns: bit for bit the decode of
    # the hand-sorted batch with hand-sorted uniforms (the same micro-batches, so the same arithmetic)
    for k in new | {"predict"}:
        assert torch.equal(given[k].index_select(0, idx), hand[k]), k
    assert model.last_decode_stats.get("num_samples") == R
    # another seed differs somewhere on par_small_gain4 too (the golden the issue names), and the seed reproduces there
    case, z, model, b, sd, batch = _model("par_small_gain4")
    try:
        with torch.no_grad():
            model.num_samples, model.sample_seed = R, 5
            s5, s5b = model(dict(b))["predict_samples"], model(dict(b))["predict_samples"]
            model.sample_seed = 6
            s6 = model(dict(b))["predict_samples"]
    finally:
        model.num_samples, model.sample_seed = 0, 0
    assert torch.equal(s5, s5b) and not torch.equal(s5, s6)


@pytest.mark.gpu
def test_option_off_changes_nothing(hip_lib):
    import ctypes as C
    from faceformer_amd.hip import lib as L
    case, z, model, b, sd, batch = _model("par_small_gain4")
    assert model.num_samples == 0
    with torch.no_grad():
        out = model(dict(b))
    assert not {"predict_samples", "predict_sample_logprob", "predict_sample_scores"} & set(out)
    T = case["model"]["seq_len"]
    assert np.array_equal(out["predict"].cpu().numpy().reshape(-1, T), z["predict"].reshape(-1, T))
    plain = _decode(model, case, b)
    assert not {"samples", "sample_logprob", "sample_scores"} & set(plain)
    eng = plain["engine"]
    ni = [int(n) for n in b["num_input"]]
    N, F = len(ni), max(ni)
    prm = L.DecodeParams()
    prm.variant, prm.N, prm.L, prm.F, prm.T = L.FF_PARALLEL, N, case["model"]["L"], F, T
    prm.flags, prm.term_lo, prm.term_hi = model.decode_flags, TERM[0], TERM[1]
    ni_host = (C.c_int * N)(*ni)
    before = hip_lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host)

    def launches():                                                  # launch counts per category of one greedy decode
        torch.cuda.synchronize()
        L.check(hip_lib.ff_profile_begin(), "ff_profile_begin")
        try:
            res = _decode(model, case, b)
        finally:
            ms, work, cnt = (C.c_double * 16)(), (C.c_double * 16)(), (C.c_longlong * 16)()
            L.check(hip_lib.ff_profile_end(ms, work, cnt, 16), "ff_profile_end")
        return res, [int(v) for v in cnt]
    first = launches()
    _sampled(model, case, b, 2, 1.0, 0, 1.0, _uniforms(case, b, 2, 1))
    assert hip_lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host) == before > 0
    assert hip_lib.ff_decode_sample_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host, 2) > before
    assert hip_lib.ff_decode_sample_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host, 65) == 0
    second = launches()
    assert torch.equal(first[0]["predict"], plain["predict"]) and torch.equal(second[0]["predict"], plain["predict"])
    assert second[0]["steps"] == plain["steps"] and first[1] == second[1] and sum(first[1]) > 0
