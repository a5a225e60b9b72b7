"""Opt-in beam search of the parallel pointer decode: the numpy rule (tests/beam_ref.py) on hand-written rows, the
C ABI and the bindings on the CPU; ff_beam_select / ff_beam_reorder and the engine's beam mode against that rule on the GPU.

Score bound (the issue's): 2^-16 + 2^-23 |score| per step -- the project's log-probability bar plus one fp32
addition.  A selection is required to equal the fp64 rule's wherever every decisive gap (between consecutive kept ranks, and
between rank W and rank W + 1) exceeds twice that bound; the replay test, whose fp32 scores have accumulated j steps of it,
uses j times the bound at step j."""
import math
import os
import re

import numpy as np
import pytest
import torch

import beam_ref as R
from conftest import ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces

TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
FILL = -R.FLT_MAX
NEG = -np.inf


# ---- CPU: the rule ----------------------------------------------------------------------------------------------------------------
def _rows(*rows):
    return np.array(rows, dtype=np.float64)


def test_rule_breaks_ties_by_the_lower_flat_index():
    # two identical rows, equal scores: every candidate of beam 0 ties with the same key of beam 1; keys 5 and 7 tie within a row
    row = [0.0] * 8
    row[5] = row[7] = 3.0
    res = R.group_step(_rows(row, row), np.array([-1.0, -1.0]), np.array([False, False]), *TERM, ge_bound=4)
    assert res["parent"].tolist() == [0, 0] and res["tok"].tolist() == [5, 7]
    assert res["scores"][0] == res["scores"][1] and res["gap"] == 0.0 and res["count"] == 2
    res = R.group_step(_rows(row, row, row), np.array([-1.0, -1.0, -1.0]), np.zeros(3, dtype=bool), *TERM)
    assert res["parent"].tolist() == [0, 0, 1] and res["tok"].tolist() == [5, 7, 5]


def test_rule_keeps_a_finished_beam_that_outranks_live_ones():
    # beam 1 is finished at -0.1; the best live candidate scores -1 + log(1/2) at the earliest
    row = [2.0, 2.0, 0.0, 0.0, 0.0, 0.0]
    res = R.group_step(_rows(row, row), np.array([-1.0, -0.1]), np.array([False, True]), *TERM, ge_bound=4)
    assert res["parent"].tolist() == [1, 0] and res["tok"].tolist() == [0, 0]
    assert res["fin"].tolist() == [True, False] and res["scores"][0] == -0.1 and res["count"] == 0
    assert abs(res["scores"][1] - (-1.0 + math.log(math.exp(2) / (2 * math.exp(2) + 4)))) < 1e-12


def test_rule_on_a_group_finished_at_start_and_on_empty_beams():
    # the start token finishes the group: its one candidate is itself, the other ranks stay empty at every later step
    res = R.group_step(_rows([1.0] * 6, [1.0] * 6, [1.0] * 6), np.array([0.0, NEG, NEG]), np.array([True, True, True]), *TERM, ge_bound=4)
    assert res["parent"].tolist() == [0, 1, 2] and res["tok"].tolist() == [0, 0, 0]
    assert res["scores"].tolist() == [0.0, NEG, NEG] and res["fin"].tolist() == [True, False, False] and res["count"] == 0
    beams, scores, steps = R.beam_decode(lambda pre: np.zeros((3, 6)), [3], 3, 5, *TERM, 4)
    assert steps == 1 and beams.tolist() == [[3, 0, 0, 0, 0]] * 3 and scores.tolist() == [0.0, NEG, NEG]
    # one live beam at the first step: W candidates from beam 0, masked keys stay candidates at finfo.min and saturate
    res = R.group_step(_rows([FILL, 1.0, FILL], [9.0] * 3), np.array([0.0, NEG]), np.zeros(2, dtype=bool), *TERM)
    assert res["parent"].tolist() == [0, 0] and res["tok"].tolist() == [1, 0] and res["scores"][1] == FILL


def _table_logits(S, seed):
    """A first-order 'model': the next logits depend on the newest token only."""
    table = np.random.RandomState(seed).randn(S, S) * 3.0
    return lambda prefixes: table[np.asarray(prefixes)[:, -1]]


@pytest.mark.parametrize("seed", range(6))
def test_rule_with_one_beam_is_the_retired_view_of_the_greedy_decode(seed):
    S, T, F = 12, 9, 7
    fn = _table_logits(S, seed)
    start = [f if f < 5 else TOK.len - 1 for f in range(F)]          # anchors 0..4 (1..3 finish at once), two padding anchors
    greedy = np.zeros((F, T), dtype=np.int64)
    greedy[:, 0] = start
    for j in range(1, T):                                            # the reference's loop: argmax, stop when no row selects an edge
        greedy[:, j] = np.argmax(fn(greedy[:, :j]), axis=1)
        if (greedy[:, j] < TOK.len).all():
            break
    want, steps = faces.retired_view(greedy, TOK, return_steps=True)
    beams, scores, got_steps = R.beam_decode(fn, start, 1, T, *TERM, TOK.len)
    assert got_steps == steps and np.array_equal(beams, want)
    lp = np.zeros((F, T))
    for j in range(1, T):
        lg = fn(greedy[:, :j])
        lp[:, j] = (lg - lg.max(1, keepdims=True) - np.log(np.exp(lg - lg.max(1, keepdims=True)).sum(1, keepdims=True)))[np.arange(F), greedy[:, j]]
    keep = faces._retired_keep(greedy, TOK)
    keep[:, 0] = False
    assert np.allclose(scores, (lp * keep).sum(1), atol=1e-12)
    # wider beams: rank 0 never scores below the greedy loop of the same anchor, ranks are in descending order
    b4, s4, _ = R.beam_decode(fn, start, 4, T, *TERM, TOK.len)
    s4 = s4.reshape(F, 4)
    assert (np.diff(np.where(np.isinf(s4), -1e300, s4), axis=1) <= 0).all()


# ---- CPU: C ABI and binding -------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_beam_select", "ff_beam_reorder", "ff_decode_beam_workspace_bytes", "ff_decode_beam")


def test_header_declares_the_beam_entries_within_abi_105():
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    doc = header[header.index("beam search over the pointer head"): header.index("int ff_beam_select(")]
    assert "model_para.py:173-179" in doc and "model_para.py:216-233" in doc
    assert re.search(r"typedef struct ff_beam_params \{\s*int width;\s*int64_t\* beams;\s*float\* scores;\s*int\* trace_parent;\s*\} ff_beam_params;", code)

    def args(name):
        return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert args("ff_decode_beam").count(",") == args("ff_decode").count(",") + 1 and "const ff_beam_params* beam" in args("ff_decode_beam")
    assert args("ff_decode_beam_workspace_bytes").count(",") == args("ff_decode_workspace_bytes").count(",") + 1


def test_binding_lists_the_beam_entries_and_refuses_a_library_without_them(monkeypatch):
    from faceformer_amd.hip import lib
    assert lib.FF_ABI_VERSION == 105
    S = lib.SIGNATURES
    for name in NEW_ENTRIES:
        assert name in S, name
    assert len(S["ff_decode_beam"][1]) == len(S["ff_decode"][1]) + 1
    assert [f for f, _ in lib.BeamParams._fields_] == ["width", "beams", "scores", "trace_parent"]
    import _ctypes
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


def test_every_rejected_combination_raises_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine, lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    ok = dict(width=2, S=12, variant=lib.FF_PARALLEL, retire=False, return_pointer=False, no_stop=False, stop_callback=None,
              extra_mask=None, logprob=False, term_range=TERM)
    engine.check_beam_options(**ok)
    for change in (dict(variant=lib.FF_SEQ2SEQ), dict(retire=True), dict(return_pointer=True), dict(no_stop=True),
                   dict(stop_callback=lambda c: False), dict(extra_mask=torch.zeros(1, 12, dtype=torch.uint8)), dict(logprob=True),
                   dict(width=0), dict(width=9), dict(width=8, S=7), dict(term_range=None), dict(term_range=(4, 4))):
        with pytest.raises(ValueError, match="beam_width"):
            engine.check_beam_options(**dict(ok, **change))


@pytest.mark.parametrize("ctor", [dict(activation="gelu"), dict(normalize_before=False), dict(num_head=2)])
def test_a_model_on_the_sub_module_loop_rejects_beam_width_before_the_library_is_touched(monkeypatch, ctor):
    from faceformer_amd.hip import lib
    from faceformer_amd.models import SurfaceFormer_Parallel
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8,
              max_face_length=5, token=TOK)
    kw.update(ctor)
    model = SurfaceFormer_Parallel(**kw).eval()
    assert not model.engine_supported() and model.beam_width == 0
    model.beam_width = 2
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    with torch.no_grad(), pytest.raises(ValueError, match="beam_width needs the native engine"):
        model.forward_eval(inputs)
    assert "predict" not in inputs                                   # (not after the fall-back either)


def test_decode_sharded_rejects_beam_width_before_the_library_is_touched(monkeypatch):
    import types
    from faceformer_amd import dist
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))

    class NoDist:                                                    # (any use of the process group is a use after the check)
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=2)
    with pytest.raises(ValueError, match="decode_sharded does not implement beam_width"):
        dist.decode_sharded(model, {}, NoDist())
    model.beam_width = 0
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


# ---- CPU: faces and the CLI -------------------------------------------------------------------------------------------------------
def test_scored_beam_faces_on_hand_written_beams():
    assert "parse_parallel_beams_scored" in faces.__all__
    beams = np.array([[[0, 4, 5, 1, 0, 0], [0, 4, 6, 2, 0, 0], [0, 0, 0, 0, 0, 0]],          # anchor 0: two loops, one empty beam
                      [[1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]],          # anchor 1: finished at its start token
                      [[4, 5, 4, 1, 0, 0], [4, 9, 4, 3, 0, 0], [4, 7, 0, 0, 0, 0]]])         # edge 9 - 4 = 5 is out of range: dropped
    scores = np.array([[-0.5, -1.5, NEG], [0.0, NEG, NEG], [-0.25, -2.0, -3.0]])
    got = faces.parse_parallel_beams_scored(beams, scores, 4, TOK)
    assert got == [(0, (0, 1), -0.5), (1, (0, 2), -1.5), (0, (0, 1, 0), -0.25), (2, (0, 0), -2.0), (-1, (0, 3, 0, 0, 0, 0), -3.0)][:4] + got[4:]
    assert len(got) == 5 and got[4][1][:2] == (0, 3) and got[4][2] == -3.0                   # (no face-type token: the whole row)
    uniq = faces.unique_faces_with_scores(got)
    assert uniq[0] == (0, (0, 1), -0.25, 2)                                                   # the same edge set twice: the best score
    flat = faces.parse_parallel_beams_scored(beams.reshape(-1, 6), scores.reshape(-1), 4, TOK)
    assert flat == got


def test_cli_beam_flag_reaches_the_model_and_the_record_is_todays_without_it(tmp_path, monkeypatch):
    import json
    import sys
    import types
    sys.path.insert(0, ROOT)
    import main as cli
    from conftest import GOLDEN
    from faceformer_amd import datasets as D
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--beam", "4"])
    assert a.beam == 4 and cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).beam == 0
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--beam", "4", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [kw["beam"] for kw in seen] == [4, 0]
    m = types.SimpleNamespace(beam_width=0)
    assert cli.configure_model(m, beam=4).beam_width == 4
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    from faceformer_amd.config import default_cfg
    cfg = default_cfg()
    with pytest.raises(ValueError, match="--beam"):
        run_test(cfg, None, out_dir="unused", device="cpu", model=object(), scores=True, beam=2)
    # the record: byte-identical without beams, two more keys with them, pred_faces untouched
    gold = json.load(open(os.path.join(GOLDEN, "cli_coedge_case.json")))
    gm = gold["model"]
    cfgm = types.SimpleNamespace(num_points_per_line=50, num_lines=gm["num_lines"], point_dim=2, max_num_faces=42,
                                 max_face_length=gm["max_face_length"], label_seq_length=0, token=TOK)
    cfg = types.SimpleNamespace(model=cfgm, post_process=types.SimpleNamespace(is_coedge=True, enclosedness_tol=gold["tol"]))
    smp = gold["samples"][0]
    d = tmp_path / "s"
    d.mkdir()
    json.dump(smp["raw"], open(str(d / "a.json"), "w"))
    item = D.ABCDataset_Parallel(str(d), "a.json", cfgm)[0]
    pred = np.asarray(smp["predict"], dtype=np.int64)
    text, st = cli.record_of(cfg, smp["raw"], item, pred, True)
    rec = json.loads(text)
    assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"] and rec["pred_faces"] == smp["pred_faces"]
    assert text == cli.record_of(cfg, smp["raw"], item, pred, True, None, None)[0]
    beams = np.stack([pred, pred], axis=1)                                                   # W = 2: the greedy rows twice
    bscores = np.stack([-np.arange(pred.shape[0]) / 8.0, -1.0 - np.arange(pred.shape[0]) / 8.0], axis=1)
    text2, st2 = cli.record_of(cfg, smp["raw"], item, pred, True, None, (beams, bscores))
    rec2 = json.loads(text2)
    assert list(rec2) == list(rec) + ["pred_beam_faces", "pred_beam_face_scores"] and st2 == st
    assert {k: rec2[k] for k in rec} == rec
    sc = rec2["pred_beam_face_scores"]
    assert len(sc) == len(rec2["pred_beam_faces"]) > 0 and sc == sorted(sc, reverse=True)


# ---- GPU: ff_beam_select ----------------------------------------------------------------------------------------------------------
def _select_case(W, S, G, t, seed, short_kv):
    """fp32-exact operands of one launch: logits = 21-bit integers * 2^-17 (|l| < 8), scores multiples of 2^-10; finished and
    empty beams mixed in; a key-padding mask per wireframe (3 wireframes when G = 33) and, with short_kv, kv_len < S."""
    g = np.random.RandomState(seed)
    B = G * W
    gpw = 11 if G % 11 == 0 else G
    nw = G // gpw
    logits = g.randint(-2 ** 20, 2 ** 20, size=(B, S)).astype(np.float64) * 2.0 ** -17
    scores = -g.randint(0, 2 ** 13, size=B).astype(np.float64) * 2.0 ** -10
    fin = g.rand(B) < 0.2
    scores[g.rand(B) < 0.15] = NEG
    mask = g.rand(nw, S) < 0.2
    mask[:, 0] = False
    kv = np.full(nw, S, dtype=np.int32)
    if short_kv:
        for w in range(nw):
            kv[w] = max(1, S - 1 - 3 * w)
    hist = g.randint(0, S, size=(t + 1, B)).astype(np.int32)
    return dict(W=W, S=S, G=G, t=t, gpw=gpw, logits=logits, scores=scores, fin=fin, mask=mask, kv=kv, hist=hist)


def _select_ref(c):
    W, gpw = c["W"], c["gpw"]
    masked = np.concatenate([R.mask_logits(c["logits"][g * W:(g + 1) * W], c["mask"][g // gpw], c["kv"][g // gpw]) for g in range(c["G"])])
    return masked, R.beam_step(masked, c["scores"], c["fin"], W, *TERM, ge_bound=TOK.len)


def _decisive_case(W, S, G, t, short_kv):
    """The first seed (searched on the CPU) at which the reference leaves out no group."""
    for seed in range(1000 * W + S, 1000 * W + S + 50):
        c = _select_case(W, S, G, t, seed, short_kv)
        masked, ref = _select_ref(c)
        if (ref["gap"] > 1.0).all():
            return c, masked, ref
    raise AssertionError("no decisive seed")


def _run_select(c, memory=None):
    from faceformer_amd.hip import ops
    dev = "cuda"
    hist = torch.from_numpy(c["hist"]).to(dev)
    logits = torch.from_numpy(c["logits"]).float().to(dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.beam_select(logits, torch.from_numpy(c["scores"]).float().to(dev), torch.from_numpy(c["fin"].astype(np.int32)).to(dev),
                          c["W"], groups_per_wireframe=c["gpw"], mask=torch.from_numpy(c["mask"].astype(np.uint8)).to(dev),
                          kv_len=torch.from_numpy(c["kv"]).to(dev), hist=hist, t=c["t"], term_range=TERM, memory=memory,
                          want_rows=memory is not None, counter=counter, ge_bound=TOK.len)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["hist"], out["logits"], out["count"] = hist.cpu().numpy(), logits.cpu().numpy(), int(counter.item())
    return out


def _check_select(c, masked, ref, got, what):
    W, B = c["W"], c["G"] * c["W"]
    left_out = float((ref["gap"] <= 1.0).mean())
    assert left_out == 0.0, (what, left_out)
    assert np.array_equal(got["parent"], ref["parent"]), what
    assert np.array_equal(got["next"], ref["tok"]), what
    assert np.array_equal(got["fin"] != 0, ref["fin"]), what
    assert got["count"] == ref["count"], what
    live = np.isfinite(ref["scores"])
    assert np.array_equal(np.isneginf(got["scores"]), ~live) and not np.isnan(got["scores"]).any(), what
    err = np.abs(got["scores"][live].astype(np.float64) - ref["scores"][live])
    bound = R.LP_BAR + R.ADD_EPS * np.abs(ref["scores"][live])
    print(what, "max score error %.3g (bound %.3g), smallest decisive gap %.3g bounds" % (err.max() if err.size else 0.0, bound.min() if bound.size else 0.0,
                                                                                         ref["gap"].min()))
    assert (err <= bound).all(), (what, float(err.max()))
    # history: permuted by the parents, the new tokens appended
    src = (np.arange(B) // W) * W + ref["parent"]
    assert np.array_equal(got["hist"][: c["t"]], c["hist"][: c["t"]][:, src]) and np.array_equal(got["hist"][c["t"]], ref["tok"]), what
    # the rows of live unfinished beams were masked in place; the others were not touched
    read = np.isfinite(c["scores"]) & ~c["fin"]
    assert np.array_equal(got["logits"][read].astype(np.float64), masked[read]), what
    assert np.array_equal(got["logits"][~read].astype(np.float64), c["logits"][~read]), what


@pytest.mark.gpu
@pytest.mark.parametrize("S", [8, 64, 65, 260, 292, 1028])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 8])
def test_beam_select_against_the_numpy_rule(hip_lib, W, S):
    for G in (1, 33):
        for t in (1, 37):
            short_kv = t == 37
            c, masked, ref = _decisive_case(W, S, G, t, short_kv)
            memory = torch.randn(G // c["gpw"], S, 64, generator=torch.Generator().manual_seed(S + W)).cuda() if t == 1 else None
            got = _run_select(c, memory)
            _check_select(c, masked, ref, got, "W=%d S=%d G=%d t=%d short_kv=%d" % (W, S, G, t, short_kv))
            if memory is not None:
                w = np.arange(G * W) // (c["gpw"] * W)
                assert np.array_equal(got["rows"], memory.cpu().numpy()[w, ref["tok"]])


@pytest.mark.gpu
@pytest.mark.parametrize("W,S", [(2, 8), (4, 65), (8, 292)])
def test_beam_select_tie_rule_on_equal_rows_and_equal_scores(hip_lib, W, S):
    # every beam holds the same row and the same score: each key ties across all W beams, and two keys tie within the row
    row = np.zeros(S)
    lo, hi = S // 3, S - 1
    row[lo] = row[hi] = 3.0
    row[1] = 2.0
    c = dict(W=W, S=S, G=2, t=1, gpw=2, logits=np.tile(row, (2 * W, 1)), scores=np.full(2 * W, -0.5), fin=np.zeros(2 * W, dtype=bool),
             mask=np.zeros((1, S), dtype=bool), kv=np.full(1, S, dtype=np.int32), hist=np.zeros((2, 2 * W), dtype=np.int32))
    masked, ref = _select_ref(c)
    got = _run_select(c)
    flat = sorted((-(3.0 if s in (lo, hi) else 2.0 if s == 1 else 0.0), k * S + s) for k in range(W) for s in range(S))[:W]
    assert ref["parent"][:W].tolist() == [ix // S for _, ix in flat] and ref["tok"][:W].tolist() == [ix % S for _, ix in flat]
    assert np.array_equal(got["parent"], ref["parent"]) and np.array_equal(got["next"], ref["tok"])
    assert (np.abs(got["scores"] - ref["scores"]) <= R.LP_BAR + R.ADD_EPS * np.abs(ref["scores"])).all()
    top = got["scores"][: min(W, 2)]
    assert (top == top[0]).all()                        # equal candidates: bit-equal fp32 scores


@pytest.mark.gpu
def test_beam_select_saturates_on_large_logits_and_masked_rows(hip_lib):
    W, S, G = 4, 65, 2
    g = np.random.RandomState(5)
    logits = np.where(g.rand(G * W, S) < 0.5, 1.0e4, -1.0e4) + g.randint(0, 64, size=(G * W, S))
    scores = -np.arange(G * W, dtype=np.float64)
    scores[W - 1] = NEG
    c = dict(W=W, S=S, G=G, t=1, gpw=1, logits=logits, scores=scores, fin=np.zeros(G * W, dtype=bool),
             mask=g.rand(G, S) < 0.3, kv=np.array([S - 3, 0], dtype=np.int32), hist=np.zeros((2, G * W), dtype=np.int32))
    masked, ref = _select_ref(c)
    assert (masked[W:] == FILL).all()                   # the second wireframe: every key masked
    got = _run_select(c)
    live = np.isfinite(ref["scores"])
    assert not np.isnan(got["scores"]).any() and np.array_equal(np.isneginf(got["scores"]), ~live)
    assert (got["scores"][live] >= np.float32(FILL)).all()
    # the all-masked group: S equal candidates per beam at c_k - log S, the lowest keys of the best beam
    assert got["parent"][W:].tolist() == [0] * W and got["next"][W:].tolist() == list(range(W))
    assert np.abs(got["scores"][W:] - (scores[W] - math.log(S))).max() <= R.LP_BAR + R.ADD_EPS * abs(scores[W] - math.log(S))
    ok = ref["gap"] > 1.0
    for gi in np.flatnonzero(ok):
        sl = slice(gi * W, (gi + 1) * W)
        assert np.array_equal(got["parent"][sl], ref["parent"][sl]) and np.array_equal(got["next"][sl], ref["tok"][sl])
    err = np.abs(got["scores"][live] - ref["scores"][live])
    assert (err <= R.LP_BAR + R.ADD_EPS * np.abs(ref["scores"][live])).all(), err.max()


# ---- GPU: ff_beam_reorder ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W,wa,wb,npos,R_extra", [(8, 512, 1536, 37, 0), (3, 64, 0, 1, 5), (4, 512, 1536, 5, 4), (1, 128, 384, 3, 0)])
def test_beam_reorder_against_index_select(hip_lib, W, wa, wb, npos, R_extra):
    from faceformer_amd.hip import ops
    G = 9
    g = torch.Generator().manual_seed(W * 100 + wa)
    rows = G * W + R_extra
    a = torch.randn(npos, rows, wa, generator=g).cuda()
    b = torch.randn(npos, rows, wb, generator=g).cuda() if wb else None
    parent = torch.randint(0, W, (G * W,), generator=g, dtype=torch.int32)          # duplicated parents
    parent[:W] = torch.arange(W, dtype=torch.int32)                                   # group 0: the identity
    parent[W:2 * W] = 0                                                               # group 1: every beam from beam 0
    src = torch.cat([(torch.arange(G * W) // W) * W + parent.long(), torch.arange(G * W, rows)]).cuda()
    want_a = a.index_select(1, src)
    want_b = b.index_select(1, src) if wb else None
    ops.beam_reorder(a, parent.cuda(), W, rows_b=b)
    assert torch.equal(a, want_a)
    if wb:
        assert torch.equal(b, want_b)


# ---- GPU: the engine --------------------------------------------------------------------------------------------------------------
def _model(name, form):
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    if form == "f32":
        model.x3_min_rows = 0
    return case, model, batch_to(batch, "cuda")


def _decode(model, case, batch, **kw):
    from test_logprob import _decode as decode
    return decode(model, case, batch, **kw)


W1_GOLDENS = ["par_small_default", "par_small_gain4", "par_small_ragged", "par_small_ragged300", "par_full_n40_gain4"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "f32"])
@pytest.mark.parametrize("name", W1_GOLDENS)
def test_engine_with_one_beam_is_the_retired_greedy_decode(hip_lib, name, form):
    from faceformer_amd.hip import lib as L
    case, model, b = _model(name, form)
    T = case["model"]["seq_len"]
    greedy = _decode(model, case, b, logprob=True)
    pred = greedy["predict"].cpu().numpy()
    want, steps = faces.retired_view(pred, TOK, return_steps=True)
    keep = faces._retired_keep(pred, TOK)
    want_score = (greedy["logprob"].cpu().numpy().astype(np.float64) * keep).sum(axis=1)
    for dedup in (True, False):
        flags = model.decode_flags | L.FF_DEDUP_PAD_ANCHORS if dedup else model.decode_flags & ~L.FF_DEDUP_PAD_ANCHORS
        out = _decode(model, case, b, beam_width=1, term_range=TERM, flags=flags)
        assert out["steps"] == steps, (name, form, dedup)
        assert np.array_equal(out["beams"].cpu().numpy(), want), (name, form, dedup)
        assert torch.equal(out["predict"], out["beams"])
        err = np.abs(out["beam_scores"].cpu().numpy().astype(np.float64) - want_score).max()
        print(name, form, "dedup=%d steps=%d max |score - sum of greedy logprob| = %.3g" % (dedup, steps, err))
        assert err <= (T - 1) * R.LP_BAR, (name, form, dedup, err)


def _replay(out, W, T, what):
    """The numpy rule applied to the decode's own logits, step by step, from the rule's own previous state.  Returns (replayed
    beams, replayed scores, still-compared group mask, left-out share of the (step, group) pairs)."""
    steps = out["steps"]
    beams = out["beams"].cpu().numpy()
    B = beams.shape[0]
    G = B // W
    logits = out["logits"].cpu().numpy().astype(np.float64)
    par = out["beam_parent"].cpu().numpy()
    tok0 = beams[:, 0].copy()
    assert (tok0.reshape(G, W) == tok0.reshape(G, W)[:, :1]).all()
    scores = np.where(np.arange(B) % W == 0, 0.0, NEG)
    fin = (tok0 >= TERM[0]) & (tok0 < TERM[1])
    ok = np.ones(G, dtype=bool)
    toks, left = [], 0
    for j in range(steps):
        lg = np.where(np.isnan(logits[j]), 0.0, logits[j])
        res = R.beam_step(lg, scores, fin, W, *TERM, ge_bound=TOK.len, margin=j + 1)
        ok &= res["gap"] > 1.0
        left += int((~ok).sum())
        okb = np.repeat(ok, W)
        assert np.array_equal(par[j][okb], res["parent"][okb]), (what, j)
        toks.append(res["tok"])
        scores, fin = res["scores"], res["fin"]
    replayed = np.zeros((B, T), dtype=np.int64)
    replayed[:, : steps + 1] = R.backtrack(tok0, toks, [par[j] for j in range(steps)], W)
    return replayed, scores, np.repeat(ok, W), left / max(1, steps * G)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("name", ["par_small_gain4", "par_small_ragged", "par_full_n40_gain4"])
def test_engine_beams_replay_under_the_numpy_rule(hip_lib, name, W):
    case, model, b = _model(name, "default")
    T = case["model"]["seq_len"]
    out = _decode(model, case, b, beam_width=W, term_range=TERM, trace=True)
    beams = out["beams"].cpu().numpy()
    got_scores = out["beam_scores"].cpu().numpy().astype(np.float64)
    replayed, scores, okb, left = _replay(out, W, T, (name, W))
    print(name, "W=%d steps=%d left-out (step, group) pairs: %.2f %%" % (W, out["steps"], 100 * left))
    assert left <= 0.02, (name, W, left)
    assert np.array_equal(beams[okb], replayed[okb]), (name, W)
    assert torch.equal(out["predict"].cpu(), out["beams"].cpu().reshape(-1, W, T)[:, 0])
    live = okb & np.isfinite(scores)
    assert np.array_equal(np.isneginf(got_scores[okb]), np.isneginf(scores[okb]))
    err = np.abs(got_scores[live] - scores[live])
    bound = out["steps"] * (R.LP_BAR + R.ADD_EPS * np.abs(scores[live]))
    print(name, "W=%d max |score - replayed score| = %.3g" % (W, err.max() if err.size else 0.0))
    assert (err <= bound).all(), (name, W, float(err.max()))
    # beams of a group are distinct sequences in descending score order
    gs = np.where(np.isinf(got_scores), -1e300, got_scores).reshape(-1, W)
    assert (np.diff(gs, axis=1) <= 0).all()


@pytest.mark.gpu
def test_engine_beams_do_not_depend_on_the_micro_batching(hip_lib):
    case, model, b = _model("par_small_ragged", "default")
    whole = _decode(model, case, b, beam_width=4, term_range=TERM, chunk_wireframes=0)
    one = _decode(model, case, b, beam_width=4, term_range=TERM, chunk_wireframes=1)
    assert whole["steps"] == one["steps"] and torch.equal(whole["beams"], one["beams"])
    assert torch.equal(whole["beam_scores"], one["beam_scores"])


@pytest.mark.gpu
def test_model_beam_width_adds_the_beams_in_batch_order(hip_lib):
    """The inverse permutation is pinned bit for bit against a decode of the batch sorted by hand (the same micro-batches, so
    the same arithmetic).  A decode in the given order plans other micro-batches (plan_chunks groups CONSECUTIVE wireframes of
    similar width), its launches have other row counts and the engine picks its GEMM forms by row count: two fp32
    evaluations of the same logits.  Each is within tol of the reference per logit (test_parity_golden._tol) and so within
    2 tol + 2^-16 per log-probability (test_engine_logprob_against_the_reference_logits), a score sums `steps` of them and two
    runs are compared: 2 steps (2 tol + 2^-16), on the groups whose beams are the same tokens; at most 2 % may differ (the
    replay test's cap)."""
    from test_parity_golden import _tol
    case, model, b = _model("par_small_ragged", "default")
    _, z = load_golden("par_small_ragged")
    T = case["model"]["seq_len"]
    ni = [int(n) for n in b["num_input"]]
    N, F, W = len(ni), max(ni), 3
    order = sorted(range(N), key=lambda i: -ni[i])
    assert order != list(range(N))                                   # the premise: the model does reorder this batch
    idx = torch.tensor(order, device="cuda")
    by_hand = {k: (v.index_select(0, idx) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in b.items()}
    by_hand["num_input"] = [ni[i] for i in order]
    with torch.no_grad():
        off = model(dict(b))
        keys_off = set(off)
        greedy = off["predict"].cpu().numpy()
        model.beam_width = W
        on = model(dict(b))
        steps = model.last_decode_stats["steps"]
        model.sort_by_edges = False
        hand = model(by_hand)
        unsorted = model(dict(b))
    assert set(on) == keys_off | {"predict_beams", "predict_beam_scores"}
    beams, scores = on["predict_beams"], on["predict_beam_scores"]
    assert tuple(beams.shape) == (N, F, W, T) and beams.dtype == torch.int64 and tuple(scores.shape) == (N, F, W)
    assert torch.equal(on["predict"], beams[:, :, 0])
    # rows come back in batch order: row order[i] of the result is row i of the decode of the hand-sorted batch
    assert torch.equal(beams.index_select(0, idx), hand["predict_beams"])
    assert torch.equal(scores.index_select(0, idx), hand["predict_beam_scores"])
    assert torch.equal(on["predict"].index_select(0, idx), hand["predict"])
    # wireframes are independent: decoded in the given order, the same beams and the same scores up to the fp32 evaluation
    same = (beams == unsorted["predict_beams"]).all(dim=3).all(dim=2).cpu().numpy()
    print("groups with other beams in the given order: %d of %d" % ((~same).sum(), same.size))
    assert (~same).mean() <= 0.02
    sa, sb = scores.cpu().numpy().astype(np.float64)[same], unsorted["predict_beam_scores"].cpu().numpy().astype(np.float64)[same]
    assert np.array_equal(np.isneginf(sa), np.isneginf(sb))
    live = np.isfinite(sa)
    bound = 2 * steps * (2 * max(_tol(z["logits"][s]) for s in range(int(z["steps"]))) + R.LP_BAR)
    print("max |score sorted - score in the given order| = %.3g (bound %.3g)" % (np.abs(sa[live] - sb[live]).max(), bound))
    assert (np.abs(sa[live] - sb[live]) <= bound).all()
    # every anchor starts every beam from its own start token, as the greedy decode does
    assert np.array_equal(beams[:, :, :, 0].cpu().numpy(), np.repeat(greedy[:, :, :1], W, axis=2))
    sc = scores.cpu().numpy().astype(np.float64)                    # (-1e300 below is no fp32 number)
    assert (np.diff(np.where(np.isinf(sc), -1e300, sc), axis=2) <= 0).all() and np.isfinite(sc[:, :, 0]).all()
    model.retire_finished = True
    with pytest.raises(ValueError, match="beam_width"):
        model(dict(b))


# ---- GPU: the engine against the reference ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_gain4", "par_full_n40_gain4"])
def test_engine_beam_scores_against_the_teacher_forced_oracle(hip_lib, name):
    """Every non-empty final beam's score against the fp64 oracle teacher-forced along that beam: the sum of the oracle's
    log_softmax at the beam's tokens, over the steps up to the beam's terminator (or the stop step).  Bound per beam: the sum over
    those steps of 2 tol(step) + 2^-16 (tol of test_parity_golden on the oracle's logits of the step; the derivation of
    test_engine_logprob_against_the_reference_logits)."""
    W = 4
    case, model, b = _model(name, "default")
    sd, batch = case_weights_and_batch(case)
    out = _decode(model, case, b, beam_width=W, term_range=TERM)
    _check_scores_against_oracle(name, case, sd, batch, out, W)


def _check_scores_against_oracle(name, case, sd, batch, out, W, step_tol=None, what=None):
    """The body of test_engine_beam_scores_against_the_teacher_forced_oracle for a beam decode `out`.  step_tol(pred, steps,
    truth) -> fn(step, oracle logits of the step): the tolerance of a step along the tokens `pred` (default:
    test_parity_golden._tol_along).  Returns the worst error / bound."""
    from test_parity_golden import _tol_along, _truth_along
    what = what or name
    T = case["model"]["seq_len"]
    steps = out["steps"]
    beams = out["beams"].cpu().numpy().reshape(-1, W, T)
    got = out["beam_scores"].cpu().numpy().astype(np.float64).reshape(-1, W)
    assert np.isfinite(got[:, 0]).all() and steps >= 1
    term = (beams >= TERM[0]) & (beams < TERM[1])
    worst, checked = 0.0, 0
    for k in range(W):
        pred = np.ascontiguousarray(beams[:, k])
        truth, _, _ = _truth_along(name, case, sd, batch, dict(predict=pred, steps=steps))   # [steps, B, S]
        tol_of = (step_tol or _tol_along)(pred, steps, truth)
        tol = np.array([tol_of(s, truth[s]) for s in range(steps)])
        for r in np.where(np.isfinite(got[:, k]))[0]:
            want, bound = 0.0, 0.0
            for j in range(1, steps + 1):
                if term[r, k, :j].any():
                    break
                lg = np.where(truth[j - 1, r] > np.finfo(np.float64).min, truth[j - 1, r], NEG)      # masked keys: exp -> 0
                m = lg.max()
                want += (lg[beams[r, k, j]] - m) - math.log(np.exp(lg - m).sum())
                bound += 2 * tol[j - 1] + R.LP_BAR
            err = abs(got[r, k] - want)
            worst = max(worst, err / bound) if bound else worst
            checked += 1
            assert err <= bound, (what, k, int(r), got[r, k], want, bound)
    print(what, "W=%d: %d beams, worst |score - oracle| / bound = %.3f" % (W, checked, worst))
    assert checked > beams.shape[0]                                  # more than the best beams were compared
    return worst


# ---- GPU: the option off ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_option_off_changes_nothing(hip_lib):
    import ctypes as C
    from faceformer_amd.hip import lib as L
    case, model, b = _model("par_small_ragged300", "default")
    from conftest import GOLDEN
    assert model.beam_width == 0
    with torch.no_grad():
        out = model(dict(b))
    assert "predict_beams" not in out and "predict_beam_scores" not in out
    T = case["model"]["seq_len"]
    fx = np.load(os.path.join(GOLDEN, "par_small_ragged300_hip_rows.npz"))      # the stored rows of the HIP's greedy decode
    assert np.array_equal(out["predict"].cpu().numpy().reshape(-1, T)[fx["rows"]], fx["predict"])
    plain = _decode(model, case, b)
    assert not {"beams", "beam_scores", "beam_parent"} & set(plain)
    # the plain workspace query does not know about the option: the same bytes before and after a beam decode, fewer than
    # the beam decode's own (W times the sequences plus the per-step records)
    eng = plain["engine"]
    ni = [int(n) for n in b["num_input"]]
    N, F, T = len(ni), max(ni), case["model"]["seq_len"]
    prm = L.DecodeParams()
    prm.variant, prm.N, prm.L, prm.F, prm.T = L.FF_PARALLEL, N, case["model"]["L"], F, T
    prm.flags, prm.term_lo, prm.term_hi = model.decode_flags, TERM[0], TERM[1]
    ni_host = (C.c_int * N)(*ni)
    before = hip_lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host)
    _decode(model, case, b, beam_width=2, term_range=TERM)
    assert hip_lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host) == before > 0
    assert hip_lib.ff_decode_beam_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host, 2) > before
    assert hip_lib.ff_decode_beam_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host, 9) == 0
    again = _decode(model, case, b)
    assert torch.equal(again["predict"], plain["predict"]) and again["steps"] == plain["steps"]
