"""Opt-in loop-constrained greedy decode of the parallel pointer head: the numpy rule (tests/constrain_ref.py) on
hand-written rows, faces.follow_table, the C ABI, the bindings, every rejected combination and the CLI on the CPU;
ff_follow_table, ff_pointer_constrained and the engine's constrained mode against that rule on the GPU.

Bars (the issue's, none measured): follow bits, FILL patterns, tokens, flags and next states are exact; log-probabilities within
2^-16 of fp64 log_softmax of the kernel's own masked row (DESIGN.md 12's bar); traced logits within test_parity_golden._tol of
the fp64 oracle teacher-forced along the constrained tokens, tokens equal to the oracle's constrained argmax wherever its margin
among live keys exceeds 2 tol, at most 2 % of the pairs left out (a condition on the fixtures: tools/constrained_left_out.py)."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
from conftest import ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces

TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
NTOK = TOK.len
FILL = CR.FILL
LOOPS = CR.NO_REPEAT | CR.CONNECT


# ---- CPU: the rule ----------------------------------------------------------------------------------------------------------------
def _hand_table():
    t = np.zeros((6, 6), dtype=bool)                       # 0 -> 1 -> 2 -> 0 (a triangle), 3 -> 3 (closes on itself), 4 -> 5 -> nothing
    t[0, 1] = t[1, 2] = t[2, 0] = t[3, 3] = t[4, 5] = True
    return t


def test_rule_on_hand_written_rows():
    f = _hand_table()
    S = NTOK + 6
    pad = np.zeros(S, dtype=bool)
    # a self-closing edge: the loop is closed after column 0
    assert CR.start_state(NTOK + 3, NTOK, f) == (frozenset({3}), None, 3)
    # anchor tokens below ntok leave the state empty (closed, nothing visited)
    assert CR.start_state(0, NTOK, f) == (frozenset(), None, None) == CR.start_state(NTOK - 1, NTOK, f)
    empty = CR.step_row(np.zeros(S), pad, CR.start_state(0, NTOK, f), LOOPS, NTOK, TERM, f)
    assert empty["masked"].tolist() == [True] + [False] * (S - 1) and empty["tok"] == 1      # closed: PAD masked, ties -> lowest index
    # a terminator refused while the loop is open: only the follower of prev is live
    raw = np.arange(S, dtype=np.float64)[::-1].copy()      # the specials carry the largest logits
    st = CR.start_state(NTOK + 0, NTOK, f)
    assert st == (frozenset({0}), 0, 0)
    r = CR.step_row(raw, pad, st, LOOPS, NTOK, TERM, f)
    assert r["masked"].tolist() == [True] * NTOK + [True, False, True, True, True, True]
    assert r["tok"] == NTOK + 1 and not r["dead"] and not r["fin"] and abs(r["logprob"]) < 1e-12 and r["state"] == (frozenset({0, 1}), 0, 1)
    assert (r["row"][r["masked"]] == FILL).all()
    # ... under NO_REPEAT alone the terminator wins, and only the visited edge is masked
    n = CR.step_row(raw, pad, st, CR.NO_REPEAT, NTOK, TERM, f)
    assert n["masked"].tolist() == [False] * NTOK + [True] + [False] * 5 and n["tok"] == 0
    # ... CONNECT alone: the visited follower stays live
    back = CR.step_row(raw, pad, (frozenset({0, 1}), 1, 0), CR.CONNECT, NTOK, TERM, f)
    assert back["tok"] == NTOK + 1 and not back["dead"] and back["state"] == (frozenset({0, 1}), 1, 1)
    # closing the triangle, then a second loop after the closure
    st = CR.state_of_prefix([NTOK + 0, NTOK + 1, NTOK + 2], NTOK, f)
    assert st == (frozenset({0, 1, 2}), None, 2)
    c = CR.step_row(-raw, pad, st, LOOPS, NTOK, TERM, f)   # the largest logit: the last edge
    assert c["masked"].tolist() == [True, False, False, False, True, True, True, False, False, False]
    assert c["tok"] == NTOK + 5 and c["state"] == (frozenset({0, 1, 2, 5}), 5, 5)
    t = CR.step_row(raw, pad, st, LOOPS, NTOK, TERM, f)    # closed: the best terminator is allowed, and ends the row
    assert t["tok"] == 1 and t["fin"] and not t["dead"]
    # a dead end: prev = 5 has no follower -> the terminators instead, the row ends, flagged
    st = CR.state_of_prefix([NTOK + 4, NTOK + 5], NTOK, f)
    assert st == (frozenset({4, 5}), 4, 5)
    d = CR.step_row(-raw, pad, st, LOOPS, NTOK, TERM, f)
    assert d["dead"] and d["fin"] and d["tok"] == 3 and d["masked"].tolist() == [True, False, False, False] + [True] * 6
    # a dead end made by NO_REPEAT (the only follower is visited) and one made by padding (the only follower is padded)
    assert CR.step_row(raw, pad, (frozenset({0, 1}), 1, 0), LOOPS, NTOK, TERM, f)["dead"]
    padded = pad.copy()
    padded[NTOK + 1] = True
    assert CR.step_row(raw, padded, (frozenset({0}), 0, 0), LOOPS, NTOK, TERM, f)["dead"]
    assert not CR.step_row(raw, padded, (frozenset({0}), 0, 0), CR.NO_REPEAT, NTOK, TERM, f)["dead"]
    # first without prev reads as closed (the open-loop rules need both)
    half = CR.step_row(raw, pad, (frozenset(), 0, None), LOOPS, NTOK, TERM, f)
    assert half["masked"].tolist() == [True, False, False, False] + [False] * 6 and half["tok"] == 1 and not half["dead"]
    # no live key at all: token 0 and -log S
    e = CR.step_row(raw, np.ones(S, dtype=bool), (frozenset(), None, None), 0, NTOK, TERM, f)
    assert e["tok"] == 0 and abs(e["logprob"] + np.log(S)) < 1e-12
    # a finished row
    fr = CR.step_row(raw, pad, st, LOOPS, NTOK, TERM, f, finished=True)
    assert fr["tok"] == 0 and fr["logprob"] == 0.0 and fr["state"] == st
    fin, steps = CR.stop_and_finish(np.array([[0, 5, 6, 1, 0, 0], [1, 0, 0, 0, 0, 0], [2, 7, 2, 0, 0, 0]]), TERM, NTOK)
    assert fin.tolist() == [3, 0, 0] and steps == 3


def test_numpy_follow_table_against_connects():
    assert "follow_table" in faces.__all__ and "pack_follow_bits" in faces.__all__
    for n, seed in ((1, 1), (7, 2), (13, 3), (40, 4)):
        batch, edges, loops = CR.lattice_batch([n], 48, 9, seed)
        t = faces.follow_table(batch["input"].numpy(), CR.TOL, [n])[0]
        want = np.array([[faces._connects(edges[0][a], edges[0][b], CR.TOL) for b in range(n)] for a in range(n)])
        assert np.array_equal(t[:n, :n], want) and not t[n:].any() and not t[:, n:].any()
        assert np.array_equal(faces.follow_table(edges[0], CR.TOL), want)                 # a list of point lists
        for loop in loops[0]:
            assert faces.is_face_enclosed(edges[0], loop, CR.TOL)
        if n >= 20:
            assert faces.is_face_enclosed(edges[0], loops[0][0] + loops[0][-2], CR.TOL)   # a square and the triangle: two loops
            assert t.sum(axis=1).max() >= 2                                               # shared corners: a choice of followers
    from conftest import GOLDEN
    gold = json.load(open(os.path.join(GOLDEN, "cli_coedge_case.json")))
    raw = gold["samples"][0]["raw"]["edges"]
    t = faces.follow_table(raw, gold["tol"])
    want = np.array([[faces._connects(a, b, gold["tol"]) for b in raw] for a in raw])
    assert np.array_equal(t, want) and want.any()
    bits = faces.pack_follow_bits(t).view(np.uint32)
    L = len(raw)
    assert bits.shape == (L, (L + 31) // 32)
    back = ((bits[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(L, -1)[:, :L].astype(bool)
    assert np.array_equal(back, t)


# ---- CPU: C ABI and binding -------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_follow_table", "ff_pointer_constrained", "ff_decode_constrained_workspace_bytes", "ff_decode_constrained")


def test_header_declares_the_constrain_entries_within_abi_105():
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
    doc = header[header.index("loop-constrained greedy decode of the pointer head"): header.index("int ff_follow_table(")]
    assert "model_para.py:173-179" in doc and "model_para.py:216-233" in doc and "post_processing.py" in doc
    for phrase in ("follows[prev][first]", "Dead end", "A one-edge loop closes on itself", "lowest index on ties"):
        assert phrase in doc, phrase
    assert re.search(r"#define\s+FF_CONSTRAIN_NO_REPEAT\s+1\b", code) and re.search(r"#define\s+FF_CONSTRAIN_CONNECT\s+2\b", code)
    assert re.search(r"typedef struct ff_constrain_params \{\s*int flags;\s*const unsigned int\* follows;\s*float\* logprob;\s*"
                     r"int\* dead_end;\s*\} ff_constrain_params;", code)

    def args(name):
        return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert args("ff_decode_constrained").count(",") == args("ff_decode").count(",") + 1
    assert "const ff_constrain_params* constrain" in args("ff_decode_constrained")
    assert args("ff_decode_constrained_workspace_bytes").count(",") == args("ff_decode_workspace_bytes").count(",")
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b", src, flags=re.M)      # no preprocessor conditionals
    from faceformer_amd.hip import build
    assert "ff_constrain.hip" in build.SOURCES


def test_binding_lists_the_constrain_entries_and_refuses_a_library_without_them(monkeypatch):
    from faceformer_amd.hip import lib
    assert lib.FF_ABI_VERSION == 105
    S = lib.SIGNATURES
    for name in NEW_ENTRIES:
        assert name in S, name
    assert len(S["ff_decode_constrained"][1]) == len(S["ff_decode"][1]) + 1
    assert len(S["ff_decode_constrained_workspace_bytes"][1]) == len(S["ff_decode_workspace_bytes"][1])
    assert [f for f, _ in lib.ConstrainParams._fields_] == ["flags", "follows", "logprob", "dead_end"]
    assert (lib.FF_CONSTRAIN_NO_REPEAT, lib.FF_CONSTRAIN_CONNECT) == (CR.NO_REPEAT, CR.CONNECT) == (1, 2)
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
    assert engine.constrain_flags(None) is None
    assert (engine.constrain_flags("no_repeat"), engine.constrain_flags("loops")) == (CR.NO_REPEAT, LOOPS)
    assert [engine.constrain_flags(v) for v in (0, 1, 2, 3)] == [0, 1, 2, 3]
    for bad in ("loop", "", 4, -1, True, 1.0):
        with pytest.raises(ValueError, match="constrain"):
            engine.constrain_flags(bad)
    table = torch.zeros(2, 8, 1, dtype=torch.int32)
    ok = dict(flags=LOOPS, variant=lib.FF_PARALLEL, retire=False, return_pointer=False, no_stop=False, stop_callback=None,
              extra_mask=None, logprob=False, beam_width=0, num_samples=0, term_range=TERM, follow_table=table)
    engine.check_constrain_options(**ok)
    engine.check_constrain_options(**dict(ok, flags=CR.NO_REPEAT, follow_table=None))
    for change in (dict(variant=lib.FF_SEQ2SEQ), dict(retire=True), dict(return_pointer=True), dict(no_stop=True),
                   dict(stop_callback=lambda c: False), dict(extra_mask=torch.zeros(1, 12, dtype=torch.uint8)), dict(logprob=True),
                   dict(beam_width=2), dict(num_samples=2), dict(term_range=None), dict(term_range=(4, 4)), dict(follow_table=None),
                   dict(flags=CR.CONNECT, follow_table=None)):
        with pytest.raises(ValueError, match="constrain"):
            engine.check_constrain_options(**dict(ok, **change))
    # PathEngine.decode itself, on an engine object without a constructor call: nothing of it may be needed
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    ok = dict(T=5, F=4, num_input=[4, 3], constrain="loops", term_range=TERM, follow_table=table)
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(8, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2),
                   dict(num_samples=2, uniforms=torch.zeros(4, 16)), dict(term_range=None), dict(follow_table=None), dict(constrain="both")):
        with pytest.raises(ValueError, match="constrain|num_samples"):
            eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, **change))
    with pytest.raises(ValueError, match="constrain"):
        eng.decode(memory, None, None, lib.FF_SEQ2SEQ, **ok)
    for bad in (torch.zeros(2, 8, 2, dtype=torch.int32), torch.zeros(2, 8, 1), torch.zeros(1, 8, 1, dtype=torch.int32), [[0]]):
        with pytest.raises(ValueError, match="follow_table must be an int32 tensor of shape \\[2, 8, 1\\]"):
            eng.decode(memory, None, None, lib.FF_PARALLEL, **dict(ok, follow_table=bad))


def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _tiny_inputs():
    return {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
            "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}


def test_models_reject_constrain_combinations_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        assert not model.engine_supported() and model.constrain is None
        model.constrain = "loops"
        inputs = _tiny_inputs()
        with torch.no_grad(), pytest.raises(ValueError, match="constrain needs the native engine"):
            model.forward_eval(inputs)
        assert "predict" not in inputs
    model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert (model.constrain, model.constrain_tol) == (None, 2e-4)
    model.constrain = "loops"
    for attr, val in (("retire_finished", True), ("beam_width", 2), ("num_samples", 2), ("return_logprob", True)):
        old = getattr(model, attr)
        setattr(model, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="excludes"):
            model.forward_eval(_tiny_inputs())
        setattr(model, attr, old)
    with torch.no_grad(), pytest.raises(ValueError, match="constrain excludes"):
        model.forward_eval(dict(_tiny_inputs(), extra_mask=torch.zeros(1, 4, 8, dtype=torch.bool)))
    model.constrain = "everything"
    with torch.no_grad(), pytest.raises(ValueError, match="constrain"):
        model.forward_eval(_tiny_inputs())
    model.constrain = "no_repeat"
    with pytest.raises(ValueError, match="score\\(\\) excludes constrain"):
        model.score(_tiny_inputs(), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    seq.constrain = "loops"
    with torch.no_grad(), pytest.raises(ValueError, match="constrain is a SurfaceFormer_Parallel option"):
        seq.forward_eval({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})


def test_decode_sharded_rejects_constrain_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    _untouchable(monkeypatch)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain="loops")
    with pytest.raises(ValueError, match="decode_sharded does not implement constrain"):
        dist.decode_sharded(model, {}, NoDist())
    model.constrain = None
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


def test_cli_constrain_flag_reaches_the_model_and_the_record_is_todays_without_it(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    from conftest import GOLDEN
    from faceformer_amd import datasets as D
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--constrain", "loops"]).constrain == "loops"
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).constrain is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--constrain", "closed"])
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--constrain", "no_repeat", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [kw["constrain"] for kw in seen] == ["no_repeat", None]
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3)
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}
    with pytest.raises(ValueError, match="--constrain applies to SurfaceFormer_Parallel only"):
        run_test(types.SimpleNamespace(model_class="SurfaceFormer"), None, out_dir="unused", device="cpu", model=object(), constrain="loops")
    cfg = types.SimpleNamespace(model_class="SurfaceFormer_Parallel")
    for kw in (dict(scores=True), dict(beam=2), dict(retire_finished=True), dict(score_labels=True), dict(sample=2)):
        with pytest.raises(ValueError, match="--constrain"):
            run_test(cfg, None, out_dir="unused", device="cpu", model=object(), constrain="loops", **kw)
    with pytest.raises(ValueError, match="--constrain must be"):
        run_test(cfg, None, out_dir="unused", device="cpu", model=object(), constrain="closed")
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--constrain .* multi-rank"):
        run_test(cfg, None, out_dir="unused", device="cpu", model=object(), constrain="loops", dist_mod=world2)
    # the record: byte-identical without the flag, two more keys with it
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
    assert text == cli.record_of(cfg, smp["raw"], item, pred, True, None, None, None, None, None)[0]
    n = int(item["num_input"])
    dead = np.zeros(pred.shape[0], dtype=np.int32)
    dead[[0, n - 1]] = 1
    dead[n:] = 1                                                                             # padding anchors are not counted
    text2, st2 = cli.record_of(cfg, smp["raw"], item, pred, True, dead_end=dead)
    rec2 = json.loads(text2)
    assert list(rec2) == list(rec) + ["pred_dead_ends", "pred_unclosed"] and st2 == st and {k: rec2[k] for k in rec} == rec
    assert rec2["pred_dead_ends"] == (2 if n > 1 else 1)
    own = [f for i in range(n) for f in faces._parallel_rows(pred[i:i + 1], TOK, len(smp["raw"]["edges"]))]
    assert rec2["pred_unclosed"] == sum(1 for _, idx in own if not faces.is_face_enclosed(smp["raw"]["edges"], idx, gold["tol"]))


# ---- GPU: ff_follow_table ---------------------------------------------------------------------------------------------------------
def _bits_to_bool(bits, L):
    u = bits.cpu().numpy().view(np.uint32)
    return ((u[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(u.shape[:-1] + (-1,))[..., :L].astype(bool)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 65, 216])
def test_follow_table_bits_equal_the_float32_rule(hip_lib, L):
    from faceformer_amd.hip import ops
    g = np.random.default_rng([7, L])
    tol = np.float32(CR.TOL)
    # lattice geometry: ragged counts, including 0 and L
    counts = sorted({0, L, max(1, L // 2), max(1, L - 1)})
    batch, _, _ = CR.lattice_batch([max(1, c) for c in counts], L, 5, 3)
    starts, ends = batch["input"][:, :, 0, :2].contiguous(), batch["input"][:, :, -1, :2].contiguous()
    # random end points with coincidences planted at distance 0 and at 10 tol (and just inside / outside tol)
    rs = g.uniform(-1, 1, size=(2, L, 2)).astype(np.float32)
    re_ = g.uniform(-1, 1, size=(2, L, 2)).astype(np.float32)
    for k, d in enumerate((0.0, 10 * CR.TOL, 0.5 * CR.TOL, 1.5 * CR.TOL, 0.0, 10 * CR.TOL)):
        a, b = int(g.integers(0, L)), int(g.integers(0, L))
        re_[k % 2, a] = rs[k % 2, b] + np.float32(d) * np.array([1, -1], dtype=np.float32)
    starts = torch.cat([starts, torch.from_numpy(rs)])
    ends = torch.cat([ends, torch.from_numpy(re_)])
    ni = counts + [L, max(0, L - 3)]
    got = ops.follow_table(starts.cuda(), ends.cuda(), torch.tensor(ni, dtype=torch.int32).cuda(), float(tol))
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(ni), L, (L + 31) // 32)
    want = faces.follow_table((starts.numpy(), ends.numpy()), tol, ni)
    assert np.array_equal(_bits_to_bool(got, L), want), L
    assert np.array_equal(got.cpu().numpy(), faces.pack_follow_bits(want))                # the bits beyond L are zero
    assert want[len(counts)].any()                                                        # the planted coincidences are seen
    assert torch.equal(got, ops.follow_table(starts.cuda(), ends.cuda(), torch.tensor(ni, dtype=torch.int32).cuda(), float(tol)))


# ---- GPU: the operator ------------------------------------------------------------------------------------------------------------
SPG = 3


def _operator_case(B, S, seed):
    """Rows in every state.  -> dict of CPU tensors / arrays."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng([seed, B, S])
    ntok = NTOK if S > NTOK else S
    term = TERM if ntok == NTOK else (0, ntok)
    L = S - ntok
    W = (B + SPG - 1) // SPG
    logits = torch.randn(B, S, generator=g) * 3.0
    if B >= 4:
        logits[B - 1] = 0.75                                             # all-equal logits: ties
    mask = torch.rand(W, S, generator=g) < 0.15
    mask[:, :ntok] = False
    kv = torch.tensor([S if w % 2 else max(1, S - 2 - w) for w in range(W)], dtype=torch.int32)
    if W > 2:
        kv[W - 1] = 0                                                    # all keys masked
    follows = CR.random_follows(W, L, seed)
    fin = np.zeros(B, dtype=np.int32)
    first = np.full(B, -1, dtype=np.int32)
    prev = np.full(B, -1, dtype=np.int32)
    visited = np.zeros((B, L), dtype=bool)
    for b in range(B):
        kind = b % 5                                                     # 0 open, 1 closed, 2 finished, 3 open with a likely dead end, 4 closed, much visited
        if L == 0:
            continue
        if kind in (0, 3):
            first[b], prev[b] = rng.integers(0, L), rng.integers(0, L)
            visited[b, [first[b], prev[b]]] = True
            if kind == 3:
                visited[b] |= follows[b // SPG, prev[b]]                 # every follower visited: a dead end under NO_REPEAT + CONNECT
        elif kind in (1, 4):
            prev[b] = rng.integers(-1, L)
            visited[b] = rng.random(L) < (0.2 if kind == 1 else 0.9)
            if kind == 4 and prev[b] < 0:
                first[b] = rng.integers(0, L)                            # first without prev: closed (the header's rule)
    if B > 2:
        fin[2] = 1
    memory = torch.randn(W, S, 64, generator=g)
    wf = torch.arange(B) // SPG
    pad = (mask[wf] | (torch.arange(S)[None, :] >= kv[wf, None])).numpy()
    return dict(logits=logits, mask=mask, kv=kv, follows=follows, fin=fin, first=first, prev=prev, visited=visited, memory=memory,
                pad=pad, ntok=ntok, term=term, L=L, W=W)


def _run_operator(c, flags, **kw):
    from faceformer_amd.hip import ops
    lg = c["logits"].clone().cuda()
    res = ops.pointer_constrained(lg, torch.from_numpy(c["fin"]).cuda(), torch.from_numpy(c["first"]).cuda(),
                                  torch.from_numpy(c["prev"]).cuda(), torch.from_numpy(faces.pack_follow_bits(c["visited"])).cuda(),
                                  flags, c["ntok"], follows=torch.from_numpy(faces.pack_follow_bits(c["follows"])).cuda(),
                                  memory=c["memory"].cuda(), mask=c["mask"].to(torch.uint8).cuda(), kv_len=c["kv"].cuda(),
                                  seqs_per_group=SPG, term_range=c["term"], want_rows=True, want_stats=True, **kw)
    return lg, res


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 63, 64, 65, 260, 1028])
def test_operator_against_the_numpy_rule(hip_lib, S):
    from faceformer_amd.hip import ops
    seen = dict(open=0, closed=0, dead=0, finished=0, nolive=0)
    for flags in (0, CR.NO_REPEAT, CR.CONNECT, LOOPS):
        for B in (1, 3, 4, 9):
            c = _operator_case(B, S, 100 * S + B)
            ntok, term, L = c["ntok"], c["term"], c["L"]
            counter = torch.zeros(1, dtype=torch.int32).cuda()
            lg, res = _run_operator(c, flags, counter=counter)
            own = lg.cpu().numpy()
            raw = c["logits"].numpy()
            got = {k: res[k].cpu().numpy() for k in ("next", "logprob", "fin", "dead_end", "first", "prev")}
            vis = _bits_to_bool(res["visited"], L) if L else np.zeros((B, 0), dtype=bool)
            what = (S, B, flags)
            nge = 0
            for b in range(B):
                w = b // SPG
                fset = frozenset(np.flatnonzero(c["visited"][b]).tolist())
                st = (fset, None if c["first"][b] < 0 else int(c["first"][b]), None if c["prev"][b] < 0 else int(c["prev"][b]))
                r = CR.step_row(raw[b].astype(np.float64), c["pad"][b], st, flags, ntok, term, c["follows"][w], finished=bool(c["fin"][b]))
                if c["fin"][b]:
                    assert np.array_equal(own[b], raw[b]), what                                # finished rows untouched
                    seen["finished"] += 1
                else:
                    assert np.array_equal(own[b] == np.float32(FILL), r["masked"] | c["pad"][b]), (what, b)    # the FILL pattern: the allowed set
                    assert np.array_equal(own[b][own[b] != np.float32(FILL)], raw[b][~(r["masked"] | c["pad"][b])]), (what, b)
                    assert np.array_equal(res["mask_rows"][b].cpu().numpy() != 0, r["masked"]), (what, b)
                    want_lp = CR.select(own[b].astype(np.float64))[1]
                    assert abs(float(got["logprob"][b]) - want_lp) <= CR.LP_BAR, (what, b, got["logprob"][b], want_lp)
                    seen["dead" if r["dead"] else ("open" if (flags & CR.CONNECT and st[1] is not None and st[2] is not None) else "closed")] += 1
                    seen["nolive"] += bool((own[b] == np.float32(FILL)).all())
                    nge += r["tok"] >= ntok
                assert got["next"][b] == r["tok"], (what, b, got["next"][b], r["tok"])        # exact, ties included
                assert bool(got["fin"][b]) == r["fin"] and bool(got["dead_end"][b]) == r["dead"], (what, b)
                nv, nf, npv = r["state"]
                assert (got["first"][b], got["prev"][b]) == (-1 if nf is None else nf, -1 if npv is None else npv), (what, b)
                assert set(np.flatnonzero(vis[b]).tolist()) == set(nv), (what, b)
                if c["fin"][b]:
                    assert got["logprob"][b] == 0.0
            assert int(counter.item()) == nge, what
            tk = res["next"]
            forced = ops.pointer_forced(c["logits"].clone().cuda(), tk, c["memory"].cuda(), c["mask"].to(torch.uint8).cuda(), c["kv"].cuda(),
                                        seqs_per_group=SPG, want_rows=True, want_stats=True)
            assert torch.equal(res["rows"], forced["rows"]) and torch.equal(res["stats"], forced["stats"]), what
            lg2, res2 = _run_operator(c, flags)                                              # two launches: bit-equal
            assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
    print("S=%d rows by state:" % S, seen)
    if S >= 63:
        assert all(v > 0 for v in seen.values()), seen                                       # every state was exercised


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 65, 260])
def test_operator_with_both_bits_clear_is_pointer_argmax(hip_lib, S):
    from faceformer_amd.hip import ops
    B, E = 9, 64
    g = torch.Generator().manual_seed(S)
    p = torch.randn(B, E, generator=g)
    W = (B + SPG - 1) // SPG
    memory = torch.randn(W, S, E, generator=g)
    memory[:, S // 2] = memory[:, 0]                                     # exact ties: keys 0 and S // 2 give the same logit
    p[0] = 0.0                                                           # a row of all-equal (zero) logits
    mask = (torch.rand(W, S, generator=g) < 0.2).to(torch.uint8)
    mask[:, 0] = 0
    ref = ops.pointer_argmax(p.cuda(), memory.cuda(), mask.cuda(), seqs_per_group=SPG, want_logits=True)
    raw = ref["logits"].clone()                                          # the argmax launch's own masked logits
    L = S - NTOK
    z = torch.zeros(B, dtype=torch.int32).cuda()
    res = ops.pointer_constrained(raw, z, z - 1, z - 1, torch.zeros(B, (L + 31) // 32, dtype=torch.int32).cuda(), 0, NTOK,
                                  mask=mask.cuda(), seqs_per_group=SPG, term_range=TERM)
    assert torch.equal(res["next"], ref["next"])                          # ties included
    assert res["next"][0].item() == 0
    assert torch.equal(raw, ref["logits"]) and not bool(res["dead_end"].any())          # nothing more is masked
    own = raw.cpu().numpy().astype(np.float64)
    want_lp = np.array([CR.select(own[b])[1] for b in range(B)])
    assert (np.abs(res["logprob"].cpu().numpy() - want_lp) <= CR.LP_BAR).all()


# ---- GPU: the engine --------------------------------------------------------------------------------------------------------------
ENGINE_GOLDENS = ["par_small_gain4", "par_small_ragged", "par_full_n40_gain4"]
_MODELS = {}


def _model(name):
    """(case, z, model, the golden's own batch on the GPU, state dict, lattice batch (CPU), lattice batch on the GPU, lattice edges,
    follow table [N, L, L] bool)."""
    if name not in _MODELS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        m = case["model"]
        lat, edges, _ = CR.lattice_batch(batch["num_input"], m["L"], m["seq_len"], CR.LATTICE_SEEDS[name])
        table = faces.follow_table(lat["input"].numpy(), CR.TOL, lat["num_input"])
        _MODELS[name] = (case, z, build_model(case, sd, "cuda"), batch_to(batch, "cuda"), sd, lat, batch_to(lat, "cuda"), edges, table)
    return _MODELS[name]


def _decode(model, case, batch, **kw):
    from test_logprob import _decode as decode
    return decode(model, case, batch, **kw)


def _constrained(model, case, b, flags, table=None, **kw):
    ft = None if table is None else torch.from_numpy(faces.pack_follow_bits(table)).cuda()
    return _decode(model, case, b, constrain=flags, follow_table=ft, term_range=TERM, **kw)


def _check_layout(out, T):
    pred, lp = out["predict"].cpu().numpy(), out["logprob"].cpu().numpy()
    assert pred.dtype == np.int64 and lp.dtype == np.float32 and pred.shape == lp.shape and pred.shape[1] == T
    fin, steps = CR.stop_and_finish(pred, TERM, NTOK)
    assert out["steps"] == steps
    past = np.arange(T)[None, :] > np.minimum(fin, steps)[:, None]
    assert (pred[past] == 0).all() and (lp[past] == 0).all() and (lp[:, 0] == 0).all()
    assert np.isfinite(lp).all() and (lp <= 0).all()
    return pred, lp.astype(np.float64), fin, steps


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_with_both_bits_clear_is_the_retired_greedy_decode(hip_lib, name):
    from test_parity_golden import _tol
    case, z, model, b = _model(name)[:4]
    T = case["model"]["seq_len"]
    greedy = _decode(model, case, b, logprob=True)
    pred = greedy["predict"].cpu().numpy()
    want, steps = faces.retired_view(pred, TOK, return_steps=True)
    keep = faces._retired_keep(pred, TOK)
    glp = greedy["logprob"].cpu().numpy().astype(np.float64) * keep
    tol = np.array([0.0] + [_tol(z["logits"][s]) for s in range(min(steps, int(z["steps"])))] + [0.0] * T)[:T]
    out = _constrained(model, case, b, 0)
    assert out["steps"] == steps, name
    assert np.array_equal(out["predict"].cpu().numpy(), want), name
    assert not bool(out["dead_end"].any())
    err = np.abs(out["logprob"].cpu().numpy().astype(np.float64) - glp)
    print(name, "steps=%d max |logprob - greedy logprob| = %.3g" % (steps, err.max()))
    assert (err <= (2 * tol + CR.LP_BAR)[None, :]).all(), (name, err.max())
    _check_layout(out, T)


def _replay(out, flags, table, F, T, what):
    """The numpy rule on the decode's own tokens and traced logits: at every (step, unfinished sequence) the FILL pattern, the
    argmax token and the flags.  Returns (pairs, margins [steps, rows] of the constrained row, inf where finished)."""
    pred, lp, fin, steps = _check_layout(out, T)
    logits = out["logits"].cpu().numpy()
    dead = out["dead_end"].cpu().numpy() != 0
    want_dead = np.zeros(pred.shape[0], dtype=bool)
    margins = np.full((steps, pred.shape[0]), np.inf)
    pairs = 0
    for j in range(steps):
        for r in np.flatnonzero(fin > j):
            fol = None if table is None else table[r // F]
            st = CR.state_of_prefix(pred[r, : j + 1], NTOK, fol)
            row = logits[j, r]
            # (the FILL pattern is the rule's own mask plus the wireframe's padding, exactly)
            masked, is_dead = CR.rule_mask(st, flags, row.size, NTOK, TERM, fol, out["_pad"][r // F])
            assert np.array_equal(row == np.float32(FILL), masked | out["_pad"][r // F]), (what, j, int(r))
            tok, own_lp = CR.select(row.astype(np.float64))
            assert pred[r, j + 1] == tok, (what, j, int(r), int(pred[r, j + 1]), tok)
            assert abs(lp[r, j + 1] - own_lp) <= CR.LP_BAR, (what, j, int(r))
            want_dead[r] |= is_dead
            if is_dead:
                assert fin[r] == j + 1, (what, j, int(r))
            live = np.sort(row[row > np.float32(FILL)].astype(np.float64))
            margins[j, r] = live[-1] - live[-2] if live.size > 1 else np.inf
            pairs += 1
    assert np.array_equal(dead, want_dead), what
    return pairs, margins


def _with_pad(out, b):
    """The wireframes' own padding [N, S] (True = masked by padding / kv_len), which the replay needs beside the trace."""
    mask = b["input_mask"].cpu().numpy()
    out["_pad"] = np.concatenate([np.zeros((mask.shape[0], NTOK), dtype=bool), mask], axis=1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [CR.NO_REPEAT, CR.CONNECT, LOOPS])
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_replays_under_the_numpy_rule(hip_lib, name, flags):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T, F = case["model"]["seq_len"], max(lat["num_input"])
    out = _with_pad(_constrained(model, case, b, flags, table, trace=True), b)
    pairs, _ = _replay(out, flags, table, F, T, (name, flags))
    print(name, flags, "steps=%d, %d (step, sequence) pairs replayed, none left out; dead ends: %d" % (out["steps"], pairs, int(out["dead_end"].sum())))
    assert pairs > 0


@pytest.mark.gpu
def test_engine_replays_dead_ends_on_a_sparse_table(hip_lib):
    """The lattice leaves no dead end; a random table of out-degree 0..4 does: the same replay, with dead ends required."""
    name = "par_small_gain4"
    case, z, model, gb, sd, lat, b, edges, _ = _model(name)
    ni = lat["num_input"]
    T, F = case["model"]["seq_len"], max(ni)
    table = CR.random_follows(len(ni), case["model"]["L"], 5)
    for w, n in enumerate(ni):
        table[w, n:] = False
        table[w, :, n:] = False
    out = _with_pad(_constrained(model, case, b, LOOPS, table, trace=True), b)
    pairs, _ = _replay(out, LOOPS, table, F, T, (name, "sparse"))
    dead = int(out["dead_end"].sum())
    print(name, "sparse table: steps=%d, %d pairs replayed, dead ends: %d" % (out["steps"], pairs, dead))
    assert dead > 0


def _yield(pred, dead, ni, edges, F):
    enc = de = un = 0
    for w, n in enumerate(ni):
        for f in range(n):
            row = pred[w * F + f]
            face = faces._parallel_rows(row[None], TOK, n)
            ends = ((row >= TERM[0]) & (row < TERM[1])).any()
            if dead[w * F + f]:
                de += 1
            elif ends and face and faces.is_face_enclosed(edges[w], face[0][1], CR.TOL):
                enc += 1
            else:
                un += 1
    return enc, de, un


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_loops_guarantee_every_ended_row_is_enclosed(hip_lib, name):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, F = case["model"]["seq_len"], max(ni)
    out = _constrained(model, case, b, LOOPS, table)
    pred, dead = out["predict"].cpu().numpy(), out["dead_end"].cpu().numpy() != 0
    ended = 0
    for w, n in enumerate(ni):
        for f in range(n):
            row = pred[w * F + f]
            idx = [int(t) - NTOK for t in row if t >= NTOK]
            assert len(idx) == len(set(idx)), (name, w, f, row)                              # no row holds an edge twice
            if ((row >= TERM[0]) & (row < TERM[1])).any() and not dead[w * F + f]:
                face = faces._parallel_rows(row[None], TOK, n)
                if face:                                                                     # (an anchor below ntok that ends at once has no edge)
                    assert faces.is_face_enclosed(edges[w], face[0][1], CR.TOL), (name, w, f, row)
                    ended += 1
    own = sum(ni)
    for label, fl in (("greedy", 0), ("no_repeat", CR.NO_REPEAT)):
        o = _constrained(model, case, b, fl, table)
        print(name, label, "enclosed / dead end / unclosed of %d own-anchor rows: %d / %d / %d"
              % ((own,) + _yield(o["predict"].cpu().numpy(), o["dead_end"].cpu().numpy() != 0, ni, edges, F)))
    print(name, "loops enclosed / dead end / unclosed of %d own-anchor rows: %d / %d / %d" % ((own,) + _yield(pred, dead, ni, edges, F)))
    assert ended >= CR.MIN_ENCLOSED * own, (name, ended, own)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_against_the_teacher_forced_oracle(hip_lib, name):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    out = _with_pad(_constrained(model, case, b, LOOPS, table, trace=True), b)
    left, pairs, _ = _check_against_oracle(name, case, sd, lat, out)
    assert left <= CR.CAP * pairs, (name, left, pairs)


def _check_against_oracle(name, case, sd, lat, out, step_tol=None, what=None):
    """The body of test_engine_against_the_teacher_forced_oracle for a traced constrained decode `out` of the lattice batch
    `lat`.  step_tol(pred, steps, truth) -> fn(step, oracle logits of the step's unfinished rows with the keys the decode masked
    at finfo.min): the tolerance of a step along the tokens `pred` (default: test_parity_golden._tol_along).  Returns (pairs left
    out, pairs, worst error / tolerance); the caller holds the left-out pairs against its cap."""
    from test_parity_golden import _tol_along, _truth_along
    what = what or name
    T = case["model"]["seq_len"]
    pred, lp, fin, steps = _check_layout(out, T)
    truth, _, _ = _truth_along("constrain:" + name, case, sd, lat, dict(predict=pred, steps=steps))
    tol_of = (step_tol or _tol_along)(pred, steps, truth)
    logits = out["logits"].cpu().numpy()
    pairs = left = 0
    worst = 0.0
    for j in range(steps):
        rows = np.flatnonzero(fin > j)
        if not rows.size:
            continue
        tol = tol_of(j, np.where(logits[j][rows] > np.float32(FILL), truth[j][rows], np.finfo(np.float32).min).astype(np.float32))
        for r in rows:
            live = logits[j, r] > np.float32(FILL)
            err = np.abs(logits[j, r][live].astype(np.float64) - truth[j, r][live])
            worst = max(worst, float(err.max()) / tol if err.size else 0.0)
            assert (err <= tol).all(), (what, j, int(r), float(err.max()), tol)
            t64 = np.where(live, truth[j, r], -np.inf)
            order = np.sort(t64[live])
            margin = order[-1] - order[-2] if order.size > 1 else np.inf
            pairs += 1
            if margin > 2 * tol:
                assert pred[r, j + 1] == int(np.argmax(t64)), (what, j, int(r))
            else:
                left += 1
    print(what, "steps=%d pairs=%d left out %.2f %%; worst |logit - oracle| / tol = %.3f" % (steps, pairs, 100.0 * left / max(1, pairs), worst))
    return left, pairs, worst


def _same_on_decisive_pairs(a, ma, c, mc, tol_of, T, what):
    """Two decodes of the same sequences: tokens equal on every pair decisive in both (margin of the constrained row above
    2 tol(step)); a row leaves the comparison at its first indecisive step."""
    n = min(ma.shape[0], mc.shape[0])
    tol = np.array([tol_of(j) for j in range(n)])
    both = (ma[:n] > 2 * tol[:, None]) & (mc[:n] > 2 * tol[:, None])
    jstop = np.where(both.all(axis=0), n, (~both).argmax(axis=0))
    keep = np.arange(T)[None, :] <= jstop[:, None]
    assert (a[keep] == c[keep]).all(), what
    return int((jstop == n).sum())


@pytest.mark.gpu
def test_plan_invariance_and_determinism(hip_lib):
    from test_parity_golden import _tol
    from faceformer_amd.hip import lib as L
    name = "par_small_ragged"
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, N, F = case["model"]["seq_len"], len(ni), max(ni)
    whole = _with_pad(_constrained(model, case, b, LOOPS, table, trace=True, chunk_wireframes=0), b)
    again = _constrained(model, case, b, LOOPS, table, trace=True, chunk_wireframes=0)
    for k in ("predict", "logprob", "dead_end"):
        assert torch.equal(whole[k], again[k]), k                                    # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"]
    one = _with_pad(_constrained(model, case, b, LOOPS, table, trace=True, chunk_wireframes=1), b)
    _, mw = _replay(whole, LOOPS, table, F, T, "whole")
    _, mo = _replay(one, LOOPS, table, F, T, "one")
    lw = whole["logits"].cpu().numpy()
    fin_w = CR.stop_and_finish(whole["predict"].cpu().numpy(), TERM, NTOK)[0]
    tol_of = lambda j: _tol(lw[j][fin_w > j]) if (fin_w > j).any() else 0.0
    full = _same_on_decisive_pairs(whole["predict"].cpu().numpy(), mw, one["predict"].cpu().numpy(), mo, tol_of, T, "chunk_wireframes = 1")
    print("chunk_wireframes = 1 against the whole batch: %d of %d rows compared to the end" % (full, N * F))
    # two wireframe orders, the table moved with the wireframes
    eng, memory, mask, kv_len = model._encode(b)
    perm = list(reversed(range(N)))
    idx = torch.tensor(perm, device="cuda")
    bits = torch.from_numpy(faces.pack_follow_bits(table)).cuda()
    kw = dict(T=T, F=F, flags=model.decode_flags, x3_min_rows=model.x3_min_rows, constrain=LOOPS, term_range=TERM, trace=True)
    fwd = _with_pad(eng.decode(memory, mask, kv_len, L.FF_PARALLEL, num_input=ni, follow_table=bits, **kw), b)
    rev = eng.decode(memory.index_select(0, idx).contiguous(), mask.index_select(0, idx).contiguous(), kv_len.index_select(0, idx).contiguous(),
                     L.FF_PARALLEL, num_input=[ni[i] for i in perm], follow_table=bits.index_select(0, idx).contiguous(), **kw)
    rev["_pad"] = fwd["_pad"][perm]
    _, mf = _replay(fwd, LOOPS, table, F, T, "fwd")
    _, mr = _replay(rev, LOOPS, table[perm], F, T, "rev")
    back = np.argsort(perm)
    rp = rev["predict"].cpu().numpy().reshape(N, F, T)[back].reshape(N * F, T)
    mrb = mr.reshape(mr.shape[0], N, F)[:, back].reshape(mr.shape[0], N * F)
    lf = fwd["logits"].cpu().numpy()
    fin_f = CR.stop_and_finish(fwd["predict"].cpu().numpy(), TERM, NTOK)[0]
    tol_f = lambda j: _tol(lf[j][fin_f > j]) if (fin_f > j).any() else 0.0
    full = _same_on_decisive_pairs(fwd["predict"].cpu().numpy(), mf, rp, mrb, tol_f, T, "two wireframe orders")
    print("two wireframe orders: %d of %d rows compared to the end" % (full, N * F))


@pytest.mark.gpu
def test_model_keys_in_batch_order_and_option_off(hip_lib):
    import ctypes as C
    from faceformer_amd.hip import lib as L
    case, z, model, gb, sd, lat, b, edges, table = _model("par_small_ragged")
    T = case["model"]["seq_len"]
    ni = lat["num_input"]
    N, F = len(ni), max(ni)
    order = sorted(range(N), key=lambda i: -ni[i])
    assert order != list(range(N))                                   # the premise: the model does reorder this batch
    idx = torch.tensor(order, device="cuda")
    by_hand = {k: (v.index_select(0, idx) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in b.items()}
    by_hand["num_input"] = [ni[i] for i in order]
    empty = np.zeros_like(table)                                     # an override: no edge follows any edge -> every open loop dead-ends
    try:
        with torch.no_grad():
            off = model(dict(b))
            keys_off = set(off)
            model.constrain = "loops"
            on = model(dict(b))
            given = model(dict(b, follow_table=table))
            packed = model(dict(b, follow_table=torch.from_numpy(faces.pack_follow_bits(table))))
            none = model(dict(b, follow_table=empty))
            model.sort_by_edges = False
            hand = model(dict(by_hand))
    finally:
        model.constrain, model.sort_by_edges = None, True
    new = {"predict_logprob", "predict_dead_end"}
    assert set(on) == keys_off | new and not new & keys_off
    assert tuple(on["predict"].shape) == tuple(on["predict_logprob"].shape) == (N, F, T) and tuple(on["predict_dead_end"].shape) == (N, F)
    direct = _constrained(model, case, b, LOOPS, table)
    assert model.sort_by_edges
    for k in new | {"predict"}:
        assert torch.equal(on[k], given[k]) and torch.equal(on[k], packed[k]), k     # the built table is the numpy table
        assert torch.equal(on[k].index_select(0, idx), hand[k]), k                   # batch order: the sort undone, rows and table
    assert not bool(on["predict_dead_end"].all()) and not torch.equal(none["predict"], on["predict"])
    own_open = torch.tensor([[f < n and f >= NTOK for f in range(F)] for n in ni], device="cuda")
    assert bool(none["predict_dead_end"][own_open].all())                            # the override is what the decode used
    assert direct["predict"].shape[0] == N * F
    # option off: keys, tokens and workspace bytes of a model that never had the attribute
    saved = {k: model.__dict__.pop(k) for k in ("constrain", "constrain_tol")}
    try:
        with torch.no_grad():
            never = model(dict(b))
    finally:
        model.__dict__.update(saved)
    assert set(never) == keys_off and torch.equal(never["predict"], off["predict"])
    eng = direct["engine"]
    prm = L.DecodeParams()
    prm.variant, prm.N, prm.L, prm.F, prm.T = L.FF_PARALLEL, N, case["model"]["L"], F, T
    prm.flags, prm.term_lo, prm.term_hi = model.decode_flags, TERM[0], TERM[1]
    ni_host = (C.c_int * N)(*ni)
    before = hip_lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host)
    _constrained(model, case, b, LOOPS, table)
    assert hip_lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host) == before > 0
    assert hip_lib.ff_decode_constrained_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host) > before
    plain = _decode(model, case, b)
    assert not {"dead_end", "logprob"} & set(plain)
    with torch.no_grad():
        assert torch.equal(model(dict(b))["predict"].reshape(-1, T), plain["predict"].reshape(-1, T))
