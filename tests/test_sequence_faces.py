"""Opt-in device-side face extraction for the single-sequence model (ff_face_seq_rows, model.sequence_faces).

CPU: header / binding / build agree; the numpy restatements faces.face_seq_rows / face_seq_votes / faces_of_seq_rows reproduce the
reference's 14 recorded `seq` cases (tests/golden/faces_cases.json) and, on seeded random rows whose coverage is asserted, the
existing list functions; every rejection is raised before the library is touched.  GPU: the entry bit for bit against the
restatement through the C ABI, twice, inside poisoned surroundings, past 2^31 bytes, FF_ERR_ARG before any launch, ff_face_votes
on its result, the model option on the goldens.

Everything is integer-exact except the fp64 score summed from fp32 log-probabilities: the kernel (and the restatement) add one by
one in ascending order, and a sequential fp64 sum of n terms is within n * 2^-52 * sum|x| of any other order's -- the bound
used against the list functions' sum(), with n = T."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import face_extract_ref as FR
import sequence_faces_ref as SR
from conftest import GOLDEN, ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces

TOK = token_ns()
NTOK, SEP, EOS = TOK.len, TOK.SEP, TOK.EOS
ROW_KEYS = ("count", "len", "start", "type", "closed", "loops", "edges", "loop_of", "set_bits", "score", "dup_of", "take", "row_best")
VOTE_KEYS = ("rep", "votes", "best", "major", "num_faces")
SEEDS = tuple(range(1, 20))          # (every kind of row at every place of a 3 x 3 batch at least once)
assert (SR.NTOK, SR.SEP, SR.EOS) == (NTOK, SEP, EOS)


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(GOLDEN, "faces_cases.json")) as f:
        return json.load(f)


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


# ---- 1. header, binding and build ----------------------------------------------------------------------------------------------------
def test_header_binding_and_build_agree():
    from faceformer_amd.hip import build, lib, ops
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    assert "device-side face extraction behind the single-sequence decode (opt-in; entries added within ABI 105; DESIGN.md 31)" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    args = re.search(r"\bff_face_seq_rows\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert args.count(",") + 1 == 30 == len(lib.SIGNATURES["ff_face_seq_rows"][1])
    for macro, value in (("FF_FACE_SEQ_CLOSED_ONLY", 1), ("FF_FACE_SEQ_MAX_T", 2048), ("FF_FACE_MAX_T", 256), ("FF_FACE_MAX_ROWS", 65536)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code) and getattr(lib, macro) == value
    assert faces.FACE_SEQ_MAX_T == lib.FF_FACE_SEQ_MAX_T and faces.FACE_SEQ_ROW_KEYS == ops.FACE_SEQ_ROW_KEYS == ROW_KEYS
    assert 64 * (faces.FACE_SEQ_MAX_T // 2) <= lib.FF_FACE_MAX_ROWS            # (G = 64 draws at T = 2048 fit ff_face_votes)
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_faces.hip")).read()
    assert "ff_faces.hip" in build.SOURCES and 'extern "C" int ff_face_seq_rows(' in src and "face_seq_rows_kernel" in src


def test_a_library_without_the_entry_is_refused(monkeypatch):
    from faceformer_amd.hip import lib
    import _ctypes
    assert "ff_face_seq_rows" in lib.SIGNATURES
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


# ---- 2. the restatement against the reference's recorded results --------------------------------------------------------------------
def _as_faces(x):
    return [(int(t), tuple(int(i) for i in idx)) for t, idx in x]


def test_restatement_reproduces_the_recorded_sequence_faces(cases):
    assert len(cases["seq"]) == 14
    some = 0
    for c in cases["seq"]:
        row = np.asarray(c["predicts"], dtype=np.int64)
        assert row.ndim == 1
        rows = faces.face_seq_rows(row[None, None, :], [c["num_edges"]], TOK, num_lines=max(int(c["num_edges"]), 1))
        votes = faces.face_seq_votes(rows)
        got = faces.faces_of_seq_rows(rows, votes, 0)
        want = _as_faces(c["pred_faces"])
        assert got["parsed"] == [want]
        assert int(rows["count"][0, 0]) == len(want)
        assert [k for _, k, _, _ in got["unique"]] == [k for _, k in faces.unique_faces_with_majority_type(want)]
        some += len(want)
    assert some > 0


# ---- 3. the restatement against the list functions on random rows ---------------------------------------------------------------------
SHAPES = ((40, 11), (70, 33))        # (T, L): the second has positions 63 .. 65 and two words


@pytest.fixture(scope="module")
def random_cases():
    return [(T, L, seed, SR.random_case(seed, N=3, G=3, T=T, L=L)) for T, L in SHAPES for seed in SEEDS]


def test_generator_coverage(random_cases):
    total = sum((SR.coverage(case) for _, _, _, case in random_cases), SR.Counter())
    assert all(total[k] >= 5 for k in SR.COVERAGE), {k: total[k] for k in SR.COVERAGE if total[k] < 5}
    kinds = {k for _, _, _, case in random_cases for k in case["kinds"].reshape(-1)}
    assert kinds == set(SR.KINDS)


def _bound(lp_row, T):
    return T * 2.0 ** -52 * float(np.abs(lp_row.astype(np.float64)).sum())


def test_restatement_equals_parse_faces_and_parse_faces_scored(random_cases):
    seen = 0
    for T, L, seed, case in random_cases:
        rows = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, logprob=case["logprob"], num_lines=L)
        for w in range(3):
            got = faces.faces_of_seq_rows(rows, None, w)
            for g in range(3):
                ne, row, lp = int(case["num_edges"][w]), case["tokens"][w, g], case["logprob"][w, g]
                want = faces.parse_faces(row, row, ne, TOK)[0]
                assert got["parsed"][g] == want, (T, L, seed, w, g)
                assert int(rows["count"][w, g]) == len(want) <= T // 2
                scored = faces.parse_faces_scored(row, lp, ne, TOK)
                assert [(t, e) for t, e, _ in got["scored"][g]] == [(t, e) for t, e, _ in scored]
                for (_, _, a), (_, _, b) in zip(got["scored"][g], scored):
                    assert abs(a - b) <= _bound(lp, T), (a, b)
                seen += len(want)
    assert seen > 500                                              # (faces compared, not a property of the code under test)


def test_truncated_slots_keep_the_true_count(random_cases):
    hit = 0
    for T, L, seed, case in random_cases[::3]:
        full = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, num_lines=L)
        cut = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, slots=2, num_lines=L)
        assert np.array_equal(full["count"], cut["count"])
        for k in ("len", "start", "score", "take", "dup_of"):
            assert np.array_equal(full[k][:, :, :2], cut[k])
        filled = cut["len"].sum(axis=2)
        for w, g in np.ndindex(filled.shape):
            assert np.array_equal(cut["edges"][w, g, : filled[w, g]], full["edges"][w, g, : filled[w, g]])
            assert (cut["edges"][w, g, filled[w, g]:] == -1).all()
        hit += int((full["count"] > 2).sum())
    assert hit >= 5                                                # count > P


def test_restatement_equals_the_sampled_list_path(random_cases):
    for T, L, seed, case in random_cases:
        rows = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, logprob=case["logprob"], num_lines=L)
        votes = faces.face_seq_votes(rows)
        for w in range(3):
            ne = int(case["num_edges"][w])
            want = faces.unique_faces_with_scores(faces.parse_faces_samples_scored(case["tokens"][w], case["logprob"][w], ne, TOK))
            got = faces.faces_of_seq_rows(rows, votes, w)["unique"]
            assert [(t, k, v) for t, k, _, v in got] == [(t, k, v) for t, k, _, v in want], (T, L, seed, w)
            bound = max(_bound(case["logprob"][w, g], T) for g in range(3))
            assert all(abs(a[2] - b[2]) <= bound for a, b in zip(got, want))
            assert int(votes["num_faces"][w]) == len(want)


def test_restatement_equals_the_beam_list_path(random_cases):
    empty = unfinished = 0
    for T, L, seed, case in random_cases:
        rows = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, scores=case["scores"], finished=case["finished"], num_lines=L)
        votes = faces.face_seq_votes(rows)
        for w in range(3):
            ne = int(case["num_edges"][w])
            want = faces.parse_faces_beams_scored(case["tokens"][w], case["scores"][w], case["finished"][w], ne, TOK)
            got = faces.faces_of_seq_rows(rows, votes, w)["unique"]
            assert [(k, s) for _, k, s, _ in got] == [(tuple(sorted(set(e))), s) for _, e, s in want], (T, L, seed, w)
        empty += int((case["scores"] == -np.inf).sum())
        unfinished += int((case["finished"] == 0).sum())
        assert (rows["count"][case["scores"] == -np.inf] == 0).all()
    assert empty >= 5 and unfinished >= 10


def test_restatement_equals_postprocess_faces_on_the_table(random_cases):
    closed = merged = 0
    for T, L, seed, case in random_cases:
        rows = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, logprob=case["logprob"], follows=case["follows"],
                                   edge_map=case["edge_map"], closed_only=True)
        votes = faces.face_seq_votes(rows, require_closed=True)
        plain = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, follows=case["follows"])
        for w in range(3):
            ne, table, emap = int(case["num_edges"][w]), case["table"][w], case["edge_map"][w]
            got = faces.faces_of_seq_rows(rows, votes, w)
            kept = []
            for g in range(3):
                parsed = faces.parse_faces(case["tokens"][w, g], case["tokens"][w, g], ne, TOK)[0]
                assert got["enclosed"][g] == faces.filter_faces_by_encloseness(FR.table_edges(table), parsed, FR.TABLE_TOL)
                want = SR.enclosed_and_mapped(parsed, table, emap)
                mine = [(t, list(SR.mapped([x for lp in loops for x in lp], emap))) for t, loops in got["enclosed"][g]]
                assert mine == want, (T, L, seed, w, g)
                closed += len(want)
                once = {}
                for t, idx in want:                                     # (a draw counts once for a face)
                    once.setdefault(tuple(sorted(set(idx))), (t, idx))
                kept += list(once.values())
            want_unique = faces.unique_faces_with_majority_type(kept)
            assert [(t, k) for t, k, _, _ in got["unique"]] == want_unique
            counts = SR.Counter(tuple(sorted(set(idx))) for _, idx in kept)
            assert [v for _, _, _, v in got["unique"]] == [counts[k] for _, k in want_unique]
            # an open face does not shadow a closed one with the same edge set: under CLOSED_ONLY it takes no part
            assert (rows["take"][w][rows["closed"][w] != 1] == 0).all() and (rows["dup_of"][w][rows["closed"][w] != 1] == -1).all()
            unmapped = faces.faces_of_seq_rows(plain, faces.face_seq_votes(plain, require_closed=True), w)["unique"]
            merged += len(unmapped) > len(got["unique"])
    assert closed > 300 and merged >= 5


def test_votes_restatement_shapes_and_first_seen_order():
    case = SR.random_case(3, N=2, G=4, T=30, L=9)
    rows = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, num_lines=9)
    votes = faces.face_seq_votes(rows)
    N, G, P = rows["take"].shape
    assert all(votes[k].shape == (N, G, P) for k in ("rep", "votes", "best", "major")) and votes["num_faces"].shape == (N,)
    rep = votes["rep"].reshape(N, -1)
    assert ((rep >= 0) == (rows["take"].reshape(N, -1) == 1)).all()
    assert (votes["votes"] <= G).all()


# ---- 4. rejections ---------------------------------------------------------------------------------------------------------------------
def test_ops_reject_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import ops
    _untouchable(monkeypatch)
    ne = torch.zeros(2, dtype=torch.int32)
    tok = torch.zeros(2, 3, 10, dtype=torch.int64)
    ok = dict(num_lines=8)
    for bad, text in ((torch.zeros(2, dtype=torch.int64), "tokens must be an int64 tensor"), (tok.to(torch.int32), "tokens must be an int64 tensor"),
                      (torch.zeros(2, 3, 0, dtype=torch.int64), r"1\.\.2048 positions per row \(got T=0\)"),
                      (torch.zeros(1, 1, 2049, dtype=torch.int64), r"1\.\.2048 positions per row \(got T=2049\)")):
        with pytest.raises(ValueError, match=text):
            ops.face_seq_rows(bad, ne, TOK, **ok)
    for kw, text in ((dict(slots=0), "slots=0: must be in 1..max"), (dict(slots=6), "slots=6: must be in 1..max"), (dict(slots=2.0), "slots=2.0: must be None or an integer"),
                     (dict(scores=torch.zeros(2, 3), logprob=torch.zeros(2, 3, 10)), "scores and logprob may not both be given"),
                     (dict(scores=torch.zeros(2, 4)), "scores must be a float32 tensor"), (dict(scores=torch.zeros(2, 3, dtype=torch.float64)), "scores must be a float32 tensor"),
                     (dict(logprob=torch.zeros(2, 3, 9)), "logprob must be a float32 tensor"), (dict(finished=torch.zeros(2, 3, dtype=torch.int64)), "finished must be a int32 tensor"),
                     (dict(follows=torch.zeros(2, 8, 2, dtype=torch.int32)), r"follows must be \[N, L, ceil\(L/32\)\]"),
                     (dict(follows=torch.zeros(2, 8, 1, dtype=torch.int32), edge_map=torch.zeros(2, 7, dtype=torch.int32)), "edge_map must be a int32 tensor"),
                     (dict(edge_map=torch.zeros(3, 8, dtype=torch.int32)), "edge_map must be a int32 tensor"),
                     (dict(edge_map=torch.zeros(2, 8, dtype=torch.int64)), "edge_map must be a int32 tensor")):
        with pytest.raises(ValueError, match=text):
            ops.face_seq_rows(tok, ne, TOK, **dict(ok, **kw))
    with pytest.raises(ValueError, match="num_edges must be a int32 tensor"):
        ops.face_seq_rows(tok, torch.zeros(3, dtype=torch.int32), TOK, **ok)
    with pytest.raises(ValueError, match="num_lines is needed"):
        ops.face_seq_rows(tok, ne, TOK)
    for sep, eos, ln in ((2, 2, 4), (4, 3, 4), (2, -1, 4), (2, 3, 3)):
        with pytest.raises(ValueError, match="must be two tokens of"):
            ops.face_seq_rows(tok, ne, types.SimpleNamespace(SEP=sep, EOS=eos, len=ln), **ok)
    with pytest.raises(ValueError, match=r"at most 65536 slots per wireframe \(got G \* P = 66560\)"):
        ops.face_seq_rows(torch.zeros(1, 65, 2048, dtype=torch.int64), ne[:1], TOK, **ok)
    with pytest.raises(ValueError, match="takes the dict face_seq_rows returns"):
        ops.face_seq_votes({"take": tok})
    rows = {k: torch.zeros(1, 65, 1024, dtype=torch.int32) for k in ("take", "type", "closed")}
    rows.update(set_bits=torch.zeros(1, 65, 1024, 1, dtype=torch.int32), row_best=torch.zeros(1, 65, 1024, dtype=torch.float64))
    with pytest.raises(ValueError, match="at most 65536 slots per wireframe"):
        ops.face_seq_votes(rows)
    rows = {k: v[:, :2, :4] for k, v in rows.items()}
    with pytest.raises(ValueError, match=r"rows\['closed'\] must be a int32 tensor"):
        ops.face_seq_votes(dict(rows, closed=rows["closed"].to(torch.int64)))
    # the numpy restatement refuses the same sizes
    for kw in (dict(slots=0), dict(slots=6), dict(scores=np.zeros((2, 3)), logprob=np.zeros((2, 3, 10)))):
        with pytest.raises(ValueError):
            faces.face_seq_rows(tok.numpy(), ne.numpy(), TOK, **dict(ok, **kw))
    with pytest.raises(ValueError, match="T=2049"):
        faces.face_seq_rows(np.zeros((1, 1, 2049), np.int64), [0], TOK, **ok)


def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _seq_inputs(**more):
    return dict({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                 "label": torch.zeros(1, 6, dtype=torch.long)}, **more)


def test_models_reject_the_option_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    from faceformer_amd.hip import lib
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    from faceformer_amd.models.common import SurfaceFormerBase
    _untouchable(monkeypatch)
    assert "_follow_table" in vars(SurfaceFormerBase) and "_follow_table" not in vars(SurfaceFormer_Parallel)      # moved, not copied
    model = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert model.sequence_faces is False and model.sequence_faces_slots is None
    for bad in (True, "closed", 1, "Parse"):
        model.sequence_faces = bad
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_faces=.*must be False, 'parse' or 'enclosed'"):
            model.forward_eval(_seq_inputs())
    model.sequence_faces = "enclosed"
    for em in (torch.zeros(1, 8, dtype=torch.int64), torch.zeros(1, 7, dtype=torch.int32), np.zeros((1, 8), np.int32)):
        with torch.no_grad(), pytest.raises(ValueError, match=r"edge_map must be an int32 tensor of shape \[1, 8\]"):
            model.forward_eval(_seq_inputs(edge_map=em))
    for slots in (0, 4, True, 2.0):
        model.sequence_faces_slots = slots
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_faces_slots=.*must be None or in 1..max"):
            model.forward_eval(_seq_inputs())
    model.sequence_faces_slots = None
    with torch.no_grad(), pytest.raises(lib.HipExtensionError, match="model parameters are on cpu"):    # (a valid call gets as far as the engine)
        model.forward_eval(_seq_inputs(edge_map=torch.zeros(1, 8, dtype=torch.int32)))
    big = _tiny_model(SurfaceFormer, label_seq_length=2048)
    big.sequence_faces, big.sequence_samples = "parse", 64
    big._sequence_faces_value(_seq_inputs(), parallel=False)                                             # 64 x 1024 fits
    big.sequence_faces_slots, big.num_labels = None, 2050
    with pytest.raises(ValueError, match="label_seq_length in 1..2048"):
        big._sequence_faces_value(_seq_inputs(), parallel=False)
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_faces = "parse"
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_faces needs the native engine"):
            sub.forward_eval(_seq_inputs())
    par = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    par.sequence_faces = "parse"
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_faces is a SurfaceFormer option"):
        par.forward_eval({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                          "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]})

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    ns = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain=None,
                               extract_faces=False, sequence_faces="parse")
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_faces"):
        dist.decode_sharded(ns, {}, NoDist())


def test_an_empty_batch_publishes_the_keys_as_empty_tensors(monkeypatch):
    from faceformer_amd.models import SurfaceFormer
    _untouchable(monkeypatch)
    model = _tiny_model(SurfaceFormer, label_seq_length=6)
    empty = {"input": torch.zeros(0, 8, 50, 2), "input_mask": torch.zeros(0, 8, dtype=torch.bool), "label": torch.zeros(0, 6, dtype=torch.long)}
    with torch.no_grad():
        assert "sequence_faces" not in model.forward_eval(dict(empty))
        model.sequence_faces, model.sequence_samples = "parse", 4
        found = model.forward_eval(dict(empty))["sequence_faces"]
    want = faces.face_seq_rows(np.zeros((1, 4, 6), np.int64), [0], TOK, num_lines=8)
    want.update(faces.face_seq_votes(want))
    assert set(found) == set(ROW_KEYS) | set(VOTE_KEYS)
    for k, v in want.items():
        assert tuple(found[k].shape) == (0,) + v.shape[1:] and found[k].numpy().dtype == v.dtype, k


def test_the_recorded_rejections_keep_their_text(monkeypatch):
    import sys
    from faceformer_amd.models import SurfaceFormer
    _untouchable(monkeypatch)
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    seq.extract_faces = "parse"
    with torch.no_grad(), pytest.raises(ValueError, match=r"extract_faces is a SurfaceFormer_Parallel option \(the single-sequence model's faces are split at SEP\)"):
        seq.forward_eval(_seq_inputs())
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    cfg = load_cfg(os.path.join(ROOT, "configs", "seq2seq.yml"), ["root_dir", "unused"])
    run = lambda **kw: cli.run_test(cfg, None, device="cpu", model=object(), **kw)
    with pytest.raises(ValueError, match="--device-faces applies to SurfaceFormer_Parallel only"):
        run(device_faces=True)
    with pytest.raises(ValueError, match="--device-faces applies to SurfaceFormer_Parallel only"):
        run(device_faces=True, sequence_device_faces=True)
    with pytest.raises(ValueError, match="--sequence-samples does not combine with --scores, --score-labels, --sample or --device-faces"):
        run(sequence_samples=4, device_faces=True)
    with pytest.raises(ValueError, match="--sequence-beams does not combine with --scores, --score-labels, --sample, --sequence-samples, --beam or "
                                         "--device-faces"):
        run(sequence_beams=4, device_faces=True)


def test_cli_flag_reaches_run_test_and_is_refused_where_it_does_not_apply(monkeypatch, tmp_path):
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    _untouchable(monkeypatch)
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).sequence_device_faces is False
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-device-faces"]).sequence_device_faces is True
    seen = []
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw["sequence_device_faces"]))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-device-faces", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert seen == [True, False]
    monkeypatch.undo()
    _untouchable(monkeypatch)
    par = load_cfg(os.path.join(ROOT, "configs", "ours.yml"), ["root_dir", str(tmp_path)])
    with pytest.raises(ValueError, match="--sequence-device-faces applies to SurfaceFormer only"):
        cli.run_test(par, None, device="cpu", model=object(), sequence_device_faces=True)
    seq = load_cfg(os.path.join(ROOT, "configs", "seq2seq.yml"), ["root_dir", str(tmp_path)])
    with pytest.raises(ValueError, match="--sequence-device-faces does not combine with --device-faces or --score-labels"):
        cli.run_test(seq, None, device="cpu", model=object(), sequence_device_faces=True, score_labels=True)
    two = types.SimpleNamespace(get_world_size=lambda: 2, get_rank=lambda: 0)
    with pytest.raises(ValueError, match="--sequence-device-faces is not implemented for multi-rank runs"):
        cli.run_test(seq, None, device="cpu", model=object(), sequence_device_faces=True, dist_mod=two)


def test_record_from_sequence_face_arrays_is_the_host_record():
    """record_of from the restatement's arrays equals record_of from the tokens: a plain config and a co-edge one with pairings;
    a greedy row with scores, draws with votes, beams with an empty rank and an unfinished beam (CPU; the GPU runs follow)."""
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    T = 24
    pts = {0: ((0, 0), (1, 0)), 1: ((1, 0), (1, 1)), 2: ((1, 1), (0, 1)), 3: ((0, 1), (0, 0)), 4: ((1, 0), (0, 0)), 5: ((1, 1), (1, 0)),
           6: ((0, 0), (1, 1)), 7: ((1, 1), (0, 0))}
    raw = {"edges": [[list(map(float, a)), list(map(float, b))] for a, b in pts.values()], "pairings": {"4": 0, "5": 1},
           "dominant_directions": []}
    L = len(pts)
    E = lambda *e: [NTOK + x for x in e]
    row = lambda *parts: np.array((sum(parts, [TOK.SOS]) + [0] * T)[:T], dtype=np.int64)
    draws = np.stack([row(E(0, 1, 2, 3), [SEP], E(1, 2, 3, 0), [SEP], E(4, 2), [SEP], E(6, 7), [EOS]),
                      row(E(2, 3, 0, 1), [SEP], E(5, 4), [SEP], E(0, 1, 7), [SEP], E(7, 6), [EOS], E(3)),
                      row(E(6, 2, 3), [SEP], E(4, 3), [SEP], E(1, 0), [EOS]),
                      row(E(0, 1, 2, 3), [SEP], E(6, 7, 0))])                    # (unterminated: zeros behind it)
    label = row(E(0, 1, 2, 3), [SEP], E(6, 7), [EOS])[1:]
    item = {"label": label}
    g = np.random.default_rng(8)
    lps = -np.abs(g.standard_normal(draws.shape)).astype(np.float32)
    lps[:, 0] = 0
    lps[draws == 0] = 0
    bound = lambda x: T * 2.0 ** -52 * abs(x)
    emap = np.arange(L, dtype=np.int32)[None].copy()
    emap[0, 4], emap[0, 5] = 0, 1
    closed_faces = 0
    for coedge in (False, True):
        cfg = load_cfg(os.path.join(ROOT, "configs", "seq2seq.yml"), ["model.num_lines", str(L), "model.label_seq_length", str(T),
                                                                        "post_process.is_coedge", str(coedge)])
        words = faces.pack_follow_bits(faces.follow_table(raw["edges"], cfg.post_process.enclosedness_tol))[None]
        form = dict(follows=words, edge_map=emap, closed_only=True) if coedge else dict(num_lines=L)

        def arrays(tokens, form, **kw):
            rows = faces.face_seq_rows(tokens, [L], cfg.model.token, **form, **kw)
            rows.update(faces.face_seq_votes(rows, require_closed=bool(form.get("closed_only"))))
            return rows
        # greedy + scores
        rows = arrays(draws[None, :1], form, logprob=lps[None, :1])
        host = cli.record_of(cfg, raw, item, draws[0], False, logprob=lps[0])
        dev = cli.record_of(cfg, raw, item, None, False, logprob=True, sequence_device_faces=rows)
        a, b = json.loads(host[0]), json.loads(dev[0])
        assert len(a["pred_faces"]) > 0 and len(a["pred_face_scores"]) == len(a["pred_faces"])
        for x, y in zip(a.pop("pred_face_scores"), b.pop("pred_face_scores")):
            assert abs(x - y) <= bound(x)
        assert json.dumps(a) == json.dumps(b) and host[1] == dev[1]
        closed_faces += coedge * len(a["pred_faces"])
        # draws: pred_faces from draw 0 in the config's form, the draws' faces unfiltered and unmapped
        rows = arrays(draws[None], dict(num_lines=L), logprob=lps[None])
        rows = dict(arrays(draws[None], form, logprob=lps[None]), every=rows) if coedge else rows
        rows["first"] = arrays(draws[None, :1], form)
        host = cli.record_of(cfg, raw, item, draws[0], False, sequence_samples=(draws, lps))
        dev = cli.record_of(cfg, raw, item, None, False, sequence_samples=True, sequence_device_faces=rows)
        a, b = json.loads(host[0]), json.loads(dev[0])
        assert len(a["pred_sample_faces"]) > 3 and max(a["pred_sample_face_votes"]) >= 3
        for x, y in zip(a.pop("pred_sample_face_scores"), b.pop("pred_sample_face_scores")):
            assert abs(x - y) <= bound(x)
        assert json.dumps(a) == json.dumps(b) and host[1] == dev[1]
        # beams: an empty rank and an unfinished beam
        sc = np.array([-1.5, -2.25, -np.inf, -4.0], np.float32)
        fin = np.array([1, 1, 0, 0], np.int32)
        rows = arrays(draws[None], dict(num_lines=L), scores=sc[None], finished=fin[None])
        rows = dict(arrays(draws[None], form, scores=sc[None], finished=fin[None]), every=rows) if coedge else rows
        rows["first"] = arrays(draws[None, :1], form)
        host = cli.record_of(cfg, raw, item, draws[0], False, sequence_beams=(draws, sc, fin))
        dev = cli.record_of(cfg, raw, item, None, False, sequence_beams=True, sequence_device_faces=rows)
        assert host == dev and len(json.loads(host[0])["pred_beam_faces"]) > 3
    assert closed_faces > 0


# ---- 5. GPU: the entry through the C ABI -----------------------------------------------------------------------------------------------
OPERANDS = ((), ("scores", "finished", "follows", "edge_map", "closed_only"), ("logprob", "follows"), ("scores", "edge_map"))
TS, LS, GS = (1, 2, 3, 63, 64, 65, 129, 259, 2048), (1, 31, 32, 33, 70, 216), (1, 3, 8)


def _grid():
    out = []
    for i, T in enumerate(TS):
        for j, L in enumerate(LS):
            G = GS[(i + j) % 3]
            P = (1, 2, max(T // 2, 1))[(i + 2 * j) % 3]
            out.append((T, L, G, min(P, max(T // 2, 1)), (i + j) % 4))
    return out


def test_the_grid_meets_every_value_with_every_T_and_every_L():
    grid = _grid()
    assert len(grid) == 54
    for axis, values in ((0, TS), (1, LS)):
        for v in values:
            sub = [c for c in grid if c[axis] == v]
            assert {c[2] for c in sub} == set(GS), (axis, v)
            assert {c[4] for c in sub} == {0, 1, 2, 3}, (axis, v)
            # P: 1, 2 and T // 2 (clamped to what T admits) meet every T; the three choices meet every L
            if axis == 0:
                assert {max(min(p, v // 2), 1) for p in (1, 2, v // 2)} == {c[3] for c in sub}, v
            else:
                assert {1, 2} <= {c[3] for c in sub} and any(c[3] == c[0] // 2 > 2 for c in sub), v


def _kwargs(case, names):
    return {k: (True if k == "closed_only" else case[k]) for k in names}


def _c_seq_rows(lib, case, names, P, L, guard=None, flags=None, fill=77):
    """ff_face_seq_rows through the C ABI; exact-size outputs holding `fill` (inside red zones with a guard).  Returns (status,
    outputs as device tensors)."""
    emb = (lambda t: guard.embed(t)) if guard is not None else (lambda t: t.cuda())
    N, G, T = case["tokens"].shape
    fw = (L + 31) // 32
    t = lambda k, dt: emb(torch.as_tensor(case[k]).to(dt))
    tokens, ne = t("tokens", torch.int64), t("num_edges", torch.int32)
    opt = {k: (t(k, dt) if k in names else None) for k, dt in (("scores", torch.float32), ("logprob", torch.float32),
                                                              ("finished", torch.int32), ("follows", torch.int32), ("edge_map", torch.int32))}
    i32 = lambda *shape: emb(torch.full(shape, fill, dtype=torch.int32))
    out = {k: i32(N, G, P) for k in ("len", "start", "type", "closed", "loops", "dup_of", "take")}
    out.update(count=i32(N, G), edges=i32(N, G, T), loop_of=i32(N, G, T), set_bits=i32(N, G, P, fw), score=i32(N, G, P, 2), row_best=i32(N, G, P, 2))
    p = lambda x: None if x is None else x.data_ptr()
    st = lib.ff_face_seq_rows(p(tokens), N, G, T, p(ne), L, NTOK, SEP, EOS, P, p(opt["scores"]), p(opt["logprob"]), p(opt["finished"]),
                              p(opt["follows"]), p(opt["edge_map"]), ("closed_only" in names) * 1 if flags is None else flags,
                              *[p(out[k]) for k in ROW_KEYS], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, out


def _as_numpy(out):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("score", "row_best"):
        got[k] = np.ascontiguousarray(got[k]).view(np.float64).reshape(got[k].shape[:-1])
    return got


def _assert_rows_equal(got, want, what=""):
    for k in ROW_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape, got[k].dtype)
        if got[k].tobytes() != want[k].tobytes():
            at = np.argwhere(got[k].view(np.int64 if got[k].itemsize == 8 else np.int32) != want[k].view(np.int64 if got[k].itemsize == 8 else np.int32))[0]
            raise AssertionError("%s %s differs first at %s: %r vs %r" % (what, k, tuple(at), got[k][tuple(at)], want[k][tuple(at)]))


def _run_twice(lib, case, names, P, L):
    st, a = _c_seq_rows(lib, case, names, P, L)
    assert st == 0, lib.ff_last_error()
    st, b = _c_seq_rows(lib, case, names, P, L, fill=-5)
    assert st == 0, lib.ff_last_error()
    a, b = _as_numpy(a), _as_numpy(b)
    for k in ROW_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), ("two runs differ", k)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,G,P,variant", _grid(), ids=lambda v: str(v))
def test_face_seq_rows_bit_for_bit(hip_lib, T, L, G, P, variant):
    names = OPERANDS[variant]
    case = SR.random_case(T + L, N=3, G=G, T=T, L=L)
    assert int(case["num_edges"][2]) == 0 and len(set(case["num_edges"].tolist())) >= 2
    want = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, slots=P, num_lines=L, **_kwargs(case, names))
    got = _run_twice(hip_lib, case, names, P, L)
    _assert_rows_equal(got, want, (T, L, G, P, names))


@pytest.mark.gpu
def test_face_seq_rows_on_the_reference_fixtures(hip_lib, cases):
    for i, c in enumerate(cases["seq"]):
        row = np.asarray(c["predicts"], dtype=np.int64)[None, None, :]
        L = max(int(c["num_edges"]), 1)
        case = dict(tokens=row, num_edges=np.array([c["num_edges"]], np.int32))
        want = faces.face_seq_rows(row, case["num_edges"], TOK, num_lines=L)
        got = _run_twice(hip_lib, case, (), max(row.shape[2] // 2, 1), L)
        _assert_rows_equal(got, want, i)
        assert faces.faces_of_seq_rows(got, None, 0)["parsed"] == [_as_faces(c["pred_faces"])]


@pytest.mark.gpu
def test_the_two_worst_cases(hip_lib):
    T, L = 2048, 216
    chain = np.zeros((1, L, L), dtype=bool)                        # edge e is followed by e + 1 (mod L): one loop of L edges
    chain[0, np.arange(L), (np.arange(L) + 1) % L] = True
    ones = np.ones((1, L, L), dtype=bool)                          # every edge closes on itself: 2047 loops of one edge
    e = np.arange(T - 1) % L
    piece = np.concatenate((NTOK + e, [EOS]))[None, None, :].astype(np.int64)
    lp = -np.abs(np.random.default_rng(7).standard_normal((1, 1, T))).astype(np.float32)
    for table in (chain, ones):
        case = dict(tokens=piece, num_edges=np.array([L], np.int32), follows=faces.pack_follow_bits(table), logprob=lp)
        want = faces.face_seq_rows(piece, case["num_edges"], TOK, follows=case["follows"], logprob=lp)
        assert want["len"][0, 0, 0] == T - 1 and want["count"][0, 0] == 1
        _assert_rows_equal(_run_twice(hip_lib, case, ("follows", "logprob"), T // 2, L), want, "one piece")
    assert want["loops"][0, 0, 0] == T - 1 and want["closed"][0, 0, 0] == 1
    # 1024 one-edge faces: all distinct (as far as L goes, two words differ), then all equal
    big = 1024
    for edges in (np.arange(big), np.zeros(big, dtype=np.int64)):
        row = np.stack((NTOK + edges, np.full(big, SEP)), axis=1).reshape(1, 1, T).astype(np.int64)
        case = dict(tokens=row, num_edges=np.array([big], np.int32), logprob=lp)
        want = faces.face_seq_rows(row, case["num_edges"], TOK, logprob=lp, num_lines=big)
        assert want["count"][0, 0] == big and want["take"].sum() == len(set(edges.tolist()))
        _assert_rows_equal(_run_twice(hip_lib, case, ("logprob",), big, big), want, "1024 faces")


def _c_votes(lib, rows, require_closed):
    N, G, P = rows["take"].shape
    R, fw = G * P, rows["set_bits"].shape[-1]
    ins = [torch.as_tensor(np.ascontiguousarray(rows[k])).cuda() for k in ("set_bits", "take", "type", "closed", "row_best")]
    outs = {k: torch.full((N, R), 77, dtype=torch.int32).cuda() for k in ("rep", "votes", "major")}
    best = torch.full((N, R), 77.0, dtype=torch.float64).cuda()
    num = torch.full((N,), 77, dtype=torch.int32).cuda()
    nbytes = lib.ff_face_votes_workspace_bytes(N, R)
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64).cuda()
    st = lib.ff_face_votes(*[x.data_ptr() for x in ins], N, R, fw, 1 if require_closed else 0, outs["rep"].data_ptr(), outs["votes"].data_ptr(),
                           best.data_ptr(), outs["major"].data_ptr(), num.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.ff_last_error()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().reshape(N, G, P) for k, v in outs.items()}
    got.update(best=best.cpu().numpy().reshape(N, G, P), num_faces=num.cpu().numpy())
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("G,T,P", [(1, 2, 1), (1, 129, 64), (1, 131, 65), (64, 259, 129), (64, 2048, 1024)], ids=lambda v: str(v))
def test_votes_on_the_result(hip_lib, G, T, P):
    assert G * P in (1, 64, 65, 8256, 65536)
    L = 33
    case = SR.random_case(G + T, N=2, G=G, T=T, L=L)
    names = ("logprob", "follows", "edge_map", "closed_only")
    st, out = _c_seq_rows(hip_lib, case, names, P, L)
    assert st == 0, hip_lib.ff_last_error()
    rows = _as_numpy(out)
    for closed in (True, False):
        want = faces.face_seq_votes(rows, require_closed=closed)
        got = _c_votes(hip_lib, rows, closed)
        for k in VOTE_KEYS:
            assert got[k].tobytes() == want[k].astype(got[k].dtype).tobytes() and got[k].dtype == want[k].dtype, (closed, k)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", (0, 1, 2), ids=["bare", "scores", "logprob"])
def test_entry_inside_poisoned_surroundings(hip_lib, variant):
    import redzone
    T, L, P = 70, 33, 35
    names = OPERANDS[variant]
    case = SR.random_case(11, N=3, G=3, T=T, L=L)
    want = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, slots=P, num_lines=L, **_kwargs(case, names))
    results = []
    for fill in (redzone.POISON, redzone.ZERO):
        g = redzone.Guard(fill)
        st, out = _c_seq_rows(hip_lib, case, names, P, L, guard=g)
        assert st == 0, hip_lib.ff_last_error()
        g.check()
        _assert_rows_equal(_as_numpy(out), want, fill)
        results.append(out)
    for k in ROW_KEYS:
        redzone.assert_same_bits(results[0][k], results[1][k], k)


@pytest.mark.gpu
def test_views_past_2_31_bytes(hip_lib):
    """tokens and set_bits are the LAST rows of allocations whose earlier rows fill more than 2^31 bytes: the kernel's offsets
    are size_t, and nothing in front of the views is touched."""
    import farview
    import redzone
    N, G, T, L = 2, 3, 70, 33
    P, fw = T // 2, 2
    case = SR.random_case(17, N=N, G=G, T=T, L=L)
    want = faces.face_seq_rows(case["tokens"], case["num_edges"], TOK, follows=case["follows"], logprob=case["logprob"])
    tok_far = farview.far(torch.zeros(2, N * G * T, dtype=torch.int64), farview.B31, redzone.POISON)
    tok_far[1].copy_(torch.as_tensor(case["tokens"]).reshape(-1))
    bits_far = farview.far(torch.full((2, N * G * P * fw), 77, dtype=torch.int32), farview.B31, redzone.POISON)
    assert farview.farthest(tok_far) > 1 << 31 and farview.farthest(bits_far) > 1 << 31
    dev = lambda k, dt: torch.as_tensor(case[k]).to(dt).cuda()
    ne, lp, fol = dev("num_edges", torch.int32), dev("logprob", torch.float32), dev("follows", torch.int32)
    i32 = lambda *shape: torch.full(shape, 77, dtype=torch.int32).cuda()
    out = {k: i32(N, G, P) for k in ("len", "start", "type", "closed", "loops", "dup_of", "take")}
    out.update(count=i32(N, G), edges=i32(N, G, T), loop_of=i32(N, G, T), set_bits=bits_far[1], score=i32(N, G, P, 2), row_best=i32(N, G, P, 2))
    st = hip_lib.ff_face_seq_rows(tok_far[1].data_ptr(), N, G, T, ne.data_ptr(), L, NTOK, SEP, EOS, P, None, lp.data_ptr(), None,
                                  fol.data_ptr(), None, 0, *[out[k].data_ptr() for k in ROW_KEYS], torch.cuda.current_stream().cuda_stream)
    assert st == 0, hip_lib.ff_last_error()
    farview.check_untouched(bits_far, "set_bits")
    farview.check_untouched(tok_far, "tokens")
    assert (bits_far[0] == 77).all()
    out["set_bits"] = bits_far[1].reshape(N, G, P, fw)
    _assert_rows_equal(_as_numpy(out), want, "far")


@pytest.mark.gpu
def test_err_arg_leaves_the_outputs_untouched(hip_lib):
    lib = hip_lib
    case = SR.random_case(2, N=1, G=2, T=12, L=8)
    big = dict(case, tokens=np.zeros((1, 2, 2049), np.int64), logprob=np.zeros((1, 2, 2049), np.float32))
    st, out = _c_seq_rows(lib, case, ("scores",), 6, 8)
    assert st == 0
    raw = torch.cuda.current_stream().cuda_stream

    def call(tokens=True, T=12, P=6, sep=SEP, eos=EOS, ntok=NTOK, scores=False, logprob=False, flags=0):
        tok = torch.as_tensor(big["tokens"]).cuda()
        ne = torch.as_tensor(case["num_edges"]).cuda()
        sc, lp = torch.zeros(1, 2).cuda(), torch.zeros(1, 2, 2049).cuda()
        outs = [torch.full((2 * 2049,), 77, dtype=torch.int32).cuda() for _ in range(13)]
        st = lib.ff_face_seq_rows(tok.data_ptr() if tokens else None, 1, 2, T, ne.data_ptr(), 8, ntok, sep, eos, P, sc.data_ptr() if scores else None,
                                  lp.data_ptr() if logprob else None, None, None, None, flags, *[o.data_ptr() for o in outs], raw)
        torch.cuda.synchronize()
        return st, all(bool((o == 77).all()) for o in outs)
    assert call() == (0, False)
    for what, kw in (("T=0", dict(T=0)), ("T=2049", dict(T=2049, P=1)), ("P=0", dict(P=0)), ("P=7", dict(P=7)), ("P=2 at T=1", dict(T=1, P=2)),
                     ("sep >= ntok", dict(sep=4)), ("eos < 0", dict(eos=-1)), ("sep == eos", dict(sep=3)), ("ntok", dict(ntok=3)),
                     ("scores with logprob", dict(scores=True, logprob=True)), ("NULL tokens", dict(tokens=False)), ("flags", dict(flags=2))):
        assert call(**kw) == (-1, True), what
        assert b"ff_face_seq_rows" in lib.ff_last_error(), what


# ---- 6. GPU: the model option on the goldens ----------------------------------------------------------------------------------------------
_MODELS = {}
MODEL_MODES = {
    "greedy": {},
    "greedy_logprob": {"return_logprob": True},
    "samples4": {"sequence_samples": 4, "sample_seed": 3},
    "beams4_all": {"sequence_beams": 4, "sequence_beam_stop": "all"},
    "beams4_best": {"sequence_beams": 4, "sequence_beam_stop": "best"},
}


def _model(name):
    if name not in _MODELS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        _MODELS[name] = (case, z, build_model(case, sd, "cuda"), batch_to(batch, "cuda"))
    return _MODELS[name]


def _expected(out, ni, extract, words, emap, L, slots):
    np_ = lambda k: out[k].cpu().numpy()
    if "predict_samples" in out:
        tokens, kw = np_("predict_samples"), dict(logprob=np_("predict_sample_logprob"))
    elif "predict_beams" in out:
        tokens, kw = np_("predict_beams"), dict(scores=np_("predict_beam_scores"), finished=np_("predict_beam_finished"))
    else:
        tokens, kw = np_("predict"), (dict(logprob=np_("predict_logprob")) if "predict_logprob" in out else {})
    enclosed = extract == "enclosed"
    rows = faces.face_seq_rows(tokens, ni, TOK, slots=slots, follows=words if enclosed else None, edge_map=emap, closed_only=enclosed, num_lines=L,
                               **kw)
    rows.update(faces.face_seq_votes(rows, require_closed=enclosed))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODEL_MODES))
@pytest.mark.parametrize("name", ("seq_small_gain4", "seq_small_eos", "seq_small_repeat_eos"))
def test_model_publishes_the_faces_of_its_rows(hip_lib, name, mode):
    case, z, model, b = _model(name)
    N, L = b["input"].size(0), b["input"].size(1)
    ni = (~b["input_mask"].bool()).sum(dim=1).cpu().numpy().astype(np.int32) if "num_input" not in b else \
        np.asarray(torch.as_tensor(b["num_input"]).cpu()).astype(np.int32).reshape(-1)
    attrs = MODEL_MODES[mode]
    saved = {k: getattr(model, k) for k in list(attrs) + ["sequence_faces", "sequence_faces_slots"]}
    rnd = np.random.default_rng(5).random((N, L, L)) < 0.3
    emap = np.tile(np.arange(L, dtype=np.int32), (N, 1))
    emap[:, 1::2] -= 1
    try:
        for k, v in attrs.items():
            setattr(model, k, v)
        with torch.no_grad():
            off = model(dict(b))
        assert "sequence_faces" not in off
        faces_seen = closed_seen = 0
        for extract, table, use_map, slots in (("parse", None, False, None), ("parse", None, True, 2), ("enclosed", np.ones((N, L, L), bool), False, None),
                                               ("enclosed", rnd, True, None), ("enclosed", None, False, None)):
            model.sequence_faces, model.sequence_faces_slots = extract, slots
            more = {}
            if table is not None:
                more["follow_table"] = torch.as_tensor(table).cuda()
            if use_map:
                more["edge_map"] = torch.as_tensor(emap).cuda()
            with torch.no_grad():
                out = model(dict(b, **more))
            for k in off:
                if torch.is_tensor(off[k]) and k.startswith("predict"):
                    assert torch.equal(off[k], out[k]), k                    # (nothing of the decode changes)
            assert set(out) - set(off) - set(more) == {"sequence_faces"}
            if table is None and extract == "enclosed":                      # the table the model builds from the end points
                x = b["input"].cpu().numpy()
                table = faces.follow_table((x[:, :, 0, :2], x[:, :, -1, :2]), model.constrain_tol, ni)
            words = None if table is None else faces.pack_follow_bits(table)
            want = _expected(out, ni, extract, words, emap if use_map else None, L, slots)
            assert set(out["sequence_faces"]) == set(ROW_KEYS) | set(VOTE_KEYS)
            for k, v in want.items():
                got = out["sequence_faces"][k].cpu().numpy()
                assert got.shape == v.shape and got.dtype == v.dtype, (k, got.shape, v.shape)
                assert got.tobytes() == v.tobytes(), (extract, k)
            faces_seen += int(want["count"].sum())
            closed_seen += int((want["closed"] == 1).sum())
            if extract == "enclosed" and table.all():
                assert ((want["closed"] == 1) == (want["len"] > 0)).all()    # every edge its own loop: every face is closed
        assert faces_seen > 0 and closed_seen > 0
    finally:
        for k, v in saved.items():
            setattr(model, k, v)


# ---- 7. GPU: the CLI ------------------------------------------------------------------------------------------------------------------
def _cli_setups(tmp_path):
    """(name, cfg, checkpoint path) of a plain and of a co-edge single-sequence set-up over the same small wireframes: a closed
    square with two co-edges, two diagonals and random edges."""
    import sys
    sys.path.insert(0, ROOT)
    from faceformer_amd.config import load_cfg
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    root = tmp_path / "data"
    (root / "json").mkdir(parents=True)
    rng = np.random.default_rng(21)
    square = [[[0, 0], [1, 0]], [[1, 0], [1, 1]], [[1, 1], [0, 1]], [[0, 1], [0, 0]], [[1, 0], [0, 0]], [[1, 1], [1, 0]], [[0, 0], [1, 1]], [[1, 1], [0, 0]]]
    names = []
    for i in range(3):
        raw = {"edges": [[[float(v) for v in p] for p in e] for e in square] + [rng.uniform(-1, 1, size=(2, 2)).tolist() for _ in range(2 * i)],
               "faces_indices": [[[0, 1, 2, 3]], [[6, 7]]], "pairings": {"4": 0, "5": 1}, "dominant_directions": [[1, 0, 0]]}
        json.dump(raw, open(root / "json" / ("%08d.json" % i), "w"))
        names.append("json/%08d.json" % i)
    open(root / "test.txt", "w").write("\n".join(names) + "\n")
    out = []
    for name, coedge in (("plain", False), ("coedge", True)):
        cfg = load_cfg("configs/seq2seq.yml", ["model.num_lines", "16", "model.label_seq_length", "24", "model.num_model", "128",
                                                "model.num_head", "2", "model.num_feedforward", "256", "model.num_encoder_layers", "2",
                                                "model.num_decoder_layers", "2", "root_dir", str(root), "post_process.is_coedge", str(coedge)])
        sd = make_state_dict(state_dict_spec("seq2seq", 16, 24, 128, 256, 2, 2), "gain4", 51)
        ckpt = tmp_path / (name + ".ckpt")
        torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(cfg)}, ckpt)
        out.append((name, cfg, str(ckpt)))
    return out


CLI_VARIANTS = {"alone": {}, "scores": {"scores": True}, "samples4": {"sequence_samples": 4, "seed": 2}, "beams4": {"sequence_beams": 4}}
SUMMED = {"scores": "pred_face_scores", "samples4": "pred_sample_face_scores"}      # fp64 sums of log-probabilities: within the bound


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(CLI_VARIANTS))
def test_cli_sequence_device_faces_writes_the_same_records(hip_lib, tmp_path, capsys, variant):
    """Record text and metrics identical to the run without the flag.  The scores that are SUMS of log-probabilities (--scores;
    the draws' under --sequence-samples, which the host adds pairwise and the device one by one) are held to T * 2^-52 * |score|,
    the rest of those records as text; beam scores are the decode's own and are compared as text."""
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    kw = CLI_VARIANTS[variant]
    faces_seen = 0
    for name, cfg, ckpt in _cli_setups(tmp_path):
        runs = {}
        for flag in (False, True):
            capsys.readouterr()
            out_dir = cli.run_test(cfg, ckpt, out_dir=str(tmp_path / ("%s_%d" % (name, flag))), batch_size=2, sequence_device_faces=flag, **kw)
            metrics = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("test_precision")]
            assert len(metrics) == 1
            runs[flag] = ({n: open(os.path.join(out_dir, n)).read() for n in sorted(os.listdir(out_dir))}, metrics[0])
        host, dev = runs[False], runs[True]
        assert host[1] == dev[1], (name, host[1], dev[1])
        assert sorted(host[0]) == sorted(dev[0]) and len(host[0]) == 3
        T = int(cfg.model.label_seq_length)
        for n in host[0]:
            a, b = json.loads(host[0][n]), json.loads(dev[0][n])
            faces_seen += len(a["pred_faces"]) + len(a.get("pred_sample_faces", [])) + len(a.get("pred_beam_faces", []))
            if variant not in SUMMED:
                assert host[0][n] == dev[0][n], (name, n)
                continue
            sa, sb = a.pop(SUMMED[variant]), b.pop(SUMMED[variant])
            assert len(sa) == len(sb)
            for x, y in zip(sa, sb):       # sums of non-positive terms: sum|lp| = |score|
                assert abs(x - y) <= T * 2.0 ** -52 * abs(x), (name, n, x, y)
            assert json.dumps(a) == json.dumps(b), (name, n)
    assert faces_seen > 0
