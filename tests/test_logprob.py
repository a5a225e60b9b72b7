"""Log-probabilities of the greedy pointer selections (ff_pointer_argmax_lp / ff_decode_lp, models' return_logprob).

The contract: for a step's masked logit row l (masked entries at finfo.min) and the selected index i* = argmax (lowest index on
ties), logprob = l[i*] - logsumexp(l) = -log sum_s exp(l[s] - l[i*]); in `ff_decode_lp`'s output it stands at the token's
position, 0 at the start token and wherever `predict` is zero padded.

Two bars, neither measured:
  LP_BAR   against the kernel's OWN masked logits (fp64 log_softmax of the fp32 logits it reduced): only the new arithmetic is
           under test -- at most 1028 non-negative terms, the largest exactly 1: a few ulp per exp, ~20 ulp of tree summation, one
           log: a few 1e-6 absolute.  Bar 2^-16.
  against the goldens' stored reference logits: the parity bar lets the HIP logits differ from the reference's by
           tol = _tol(step), and l[i*] - logsumexp(l) moves by at most 2 max|dl|.  Bar 2 _tol(step) + 2^-16.
"""
import json
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces

TOK = token_ns()
LP_BAR = 2.0 ** -16
FILL = float(torch.finfo(torch.float32).min)


def _ref_logprob(logits, index):
    """fp64 log_softmax of fp32 masked logits [..., S], taken at index [...]."""
    ls = torch.log_softmax(logits.double(), dim=-1)
    return ls.gather(-1, index.long().unsqueeze(-1)).squeeze(-1)


# ---- CPU: scored face parsing ---------------------------------------------------------------------------------------------------
def test_scored_parallel_faces_on_hand_written_rows():
    p = np.array([
        [0, 5, 6, 2, 7, 8, 0],     # face (1, (1, 2)), finished at 3: positions 1..3 are scored
        [3, 9, 9, 9, 9, 9, 0],     # finished at position 0: no face
        [0, 6, 5, 2, 0, 0, 0],     # the same edge set as row 0 in another order, another score
        [0, 4, 5, 6, 0, 0, 0],     # never finishes: the whole row is the face, every position is scored
        [2, 0, 0, 0, 0, 0, 0],     # finished at position 0
        [0, 7, 1, 0, 0, 0, 0],     # type 0, a third edge set
    ], dtype=np.int64)
    lp = -np.arange(p.size, dtype=np.float64).reshape(p.shape) / 8.0
    lp[:, 0] = 0.0
    got = faces.parse_parallel_faces_scored(p, lp, 6, TOK)
    plain, _ = faces.parse_parallel_faces(p, p, 6, TOK)
    assert [(t, e) for t, e, _ in got] == plain           # the rows and the filters of the unscored function
    want = [lp[0, 1:4].sum(), lp[2, 1:4].sum(), lp[3, 1:].sum(), lp[5, 1:3].sum()]
    assert [s for _, _, s in got] == pytest.approx(want, abs=0, rel=1e-15)
    uniq = faces.unique_faces_with_scores(got)
    assert [(t, e) for t, e, _, _ in uniq] == faces.unique_faces_with_majority_type(plain)
    assert [v for _, _, _, v in uniq] == [2, 1, 1]         # rows 0 and 2 vote for one face
    assert uniq[0][2] == max(want[0], want[1]) == want[0]  # ... whose score is the better of the two
    # num_edges filters the scored faces as it filters the unscored ones
    assert [(t, e) for t, e, _ in faces.parse_parallel_faces_scored(p, lp, 2, TOK)] == faces.parse_parallel_faces(p, p, 2, TOK)[0]
    assert faces.parse_parallel_faces_scored(p[:0], lp[:0], 6, TOK) == []


def test_scored_seq2seq_faces_on_hand_written_tokens():
    #             SOS  e0 e1 SEP SEP e2 e3 e1 SEP e0 EOS  (after the EOS: ignored)
    seq = np.array([1, 4, 5, 2, 2, 6, 7, 5, 2, 4, 3, 9, 2, 0], dtype=np.int64)
    lp = -(1.0 + np.arange(seq.size, dtype=np.float64)) / 16.0
    lp[0] = 0.0
    got = faces.parse_faces_scored(seq, lp, 4, TOK)
    plain, _ = faces.parse_faces(seq, seq, 4, TOK)
    assert [(t, e) for t, e, _ in got] == plain == [(0, (0, 1)), (0, (2, 3, 1)), (0, (0,))]
    # a face's piece with its separator: [SOS e0 e1 SEP], (the lone SEP is skipped), [e2 e3 e1 SEP], [e0 EOS]
    assert [s for _, _, s in got] == pytest.approx([lp[0:4].sum(), lp[5:9].sum(), lp[9:11].sum()], abs=0, rel=1e-15)
    uniq = faces.unique_faces_with_scores(got + [(0, (1, 0), -0.25)])
    assert [(t, e) for t, e, _, _ in uniq] == faces.unique_faces_with_majority_type(plain + [(0, (1, 0))])
    assert uniq[0][2:] == (-0.25, 2)


def test_retired_keep_is_the_padding_of_retired_view():
    rng = np.random.default_rng(5)
    for _ in range(20):
        p = rng.integers(0, 9, size=(3, 4, 7))
        keep = faces._retired_keep(p, TOK)
        assert keep.shape == p.shape and keep.dtype == bool
        assert np.array_equal(np.where(keep, p, 0), faces.retired_view(p, TOK))


def test_own_stop_rule_scored_cuts_tokens_and_scores_alike():
    rows = np.array([[5, 6, 2, 9, 1, 0], [6, 7, 0, 8, 2, 0]])
    lp = -np.ones(rows.shape)
    cut, clp = faces._apply_own_stop_rule_scored(rows, lp, TOK, True)
    assert np.array_equal(cut, faces.apply_own_stop_rule(rows, TOK, True))
    assert clp.tolist() == [[-1, -1, -1, 0, 0, 0]] * 2 and lp[0, 3] == -1      # copies
    s = np.array([1, 7, 8, 3, 9, 3, 0])
    cut, clp = faces._apply_own_stop_rule_scored(s, -np.ones(7), TOK, False)
    assert np.array_equal(cut, faces.apply_own_stop_rule(s, TOK, False)) and clp.tolist() == [-1, -1, -1, -1, 0, 0, 0]


# ---- CPU: C ABI and binding -----------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_within_abi_105():
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ff_pointer_argmax_lp", "ff_decode_lp", "ff_decode_lp_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        # ... and its comment cites the reference's select_next
        doc = header[: re.search(r"\b%s\s*\(" % name, header).start()].rsplit("/*", 1)[1]
        assert "select_next" in doc and "model_para.py:173-179" in doc and "model.py:161-167" in doc, name
    # float* logprob is the one argument the new entries add
    def args(name):
        return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
    assert "float* logprob" in args("ff_pointer_argmax_lp") and "float* logprob" in args("ff_decode_lp")
    assert args("ff_pointer_argmax_lp").count(",") == args("ff_pointer_argmax").count(",") + 1
    assert args("ff_decode_lp").count(",") == args("ff_decode").count(",") + 1
    assert re.sub(r"\s+", " ", args("ff_decode_lp_workspace_bytes")) == re.sub(r"\s+", " ", args("ff_decode_workspace_bytes"))


def test_binding_lists_the_entries_and_refuses_a_library_without_them(tmp_path, monkeypatch):
    from faceformer_amd.hip import lib
    assert lib.FF_ABI_VERSION == 105
    S = lib.SIGNATURES
    assert len(S["ff_pointer_argmax_lp"][1]) == len(S["ff_pointer_argmax"][1]) + 1
    assert len(S["ff_decode_lp"][1]) == len(S["ff_decode"][1]) + 1
    assert S["ff_decode_lp_workspace_bytes"] == S["ff_decode_workspace_bytes"]
    # a stale library -- here: a shared object without the symbols, the interpreter's own _ctypes module -- is refused when it
    # is loaded, with the rebuild hint
    import _ctypes
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


def test_sharded_decode_rejects_return_logprob():
    from faceformer_amd import dist
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    for m in (SurfaceFormer_Parallel(max_face_length=6, **kw), SurfaceFormer(label_seq_length=6, **kw)):
        assert m.return_logprob is False
        m.return_logprob = True
        with pytest.raises(ValueError, match="return_logprob"):
            dist.decode_sharded(m, {"input": torch.zeros(1, 8, 50, 2)}, dist_mod=None)


# ---- CPU: the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_scores_flag_reaches_configure_model(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--scores", "model.num_lines", "256"])
    assert a.scores is True and a.opts == ["model.num_lines", "256"]
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).scores is False
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--scores", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [kw["scores"] for kw in seen] == [True, False]
    m = types.SimpleNamespace(return_logprob=False)
    assert cli.configure_model(m, scores=True).return_logprob is True
    plain = types.SimpleNamespace()
    cli.configure_model(plain)
    assert vars(plain) == {}                              # without the flags nothing is set

    class TwoRanks:                                       # --scores under the multi-rank mode: refused before anything is built
        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def get_rank():
            return 0
    from faceformer_amd.config import default_cfg
    with pytest.raises(ValueError, match="return_logprob"):
        run_test(default_cfg(), None, out_dir="unused", device="cpu", model=object(), dist_mod=TwoRanks, scores=True)


def test_cli_record_is_todays_without_the_flag_and_gains_scores_with_it(tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd import datasets as D
    gold = json.load(open(os.path.join(GOLDEN, "cli_coedge_case.json")))
    gm = gold["model"]
    cfgm = types.SimpleNamespace(num_points_per_line=50, num_lines=gm["num_lines"], point_dim=2, max_num_faces=42,
                                 max_face_length=gm["max_face_length"], label_seq_length=0, token=TOK)
    for is_coedge in (True, False):
        cfg = types.SimpleNamespace(model=cfgm, post_process=types.SimpleNamespace(is_coedge=is_coedge, enclosedness_tol=gold["tol"]))
        for k, smp in enumerate(gold["samples"]):
            raw = smp["raw"]
            d = tmp_path / ("s%d_%d" % (k, is_coedge))
            d.mkdir()
            json.dump(raw, open(str(d / "a.json"), "w"))
            item = D.ABCDataset_Parallel(str(d), "a.json", cfgm)[0]
            pred = np.asarray(smp["predict"], dtype=np.int64)
            text, st = cli.record_of(cfg, raw, item, pred, True)
            rec = json.loads(text)
            assert list(rec) == ["edges", "dominant_directions", "pred_faces", "label_faces"]      # today's keys, today's order
            if is_coedge:                                                                          # ... and today's fixture
                assert rec["pred_faces"] == smp["pred_faces"]
                assert sorted(rec["label_faces"]) == sorted(smp["label_faces"])
                assert st[0] == smp["precision"] and st[1] == smp["recall"]
            lp = -np.arange(pred.size, dtype=np.float64).reshape(pred.shape) / 64.0
            lp[:, 0] = 0
            text2, st2 = cli.record_of(cfg, raw, item, pred, True, lp)
            rec2 = json.loads(text2)
            assert list(rec2) == list(rec) + ["pred_face_scores"] and st2 == st
            scores = rec2.pop("pred_face_scores")
            assert rec2 == rec
            assert len(scores) == len(rec["pred_faces"]) and all(s <= 0 for s in scores)
            if not is_coedge:
                n = int(item["num_input"])
                cut, clp = faces._apply_own_stop_rule_scored(pred[:n], lp[:n], TOK, True)
                uniq = faces.unique_faces_with_scores(faces.parse_parallel_faces_scored(cut, clp, len(raw["edges"]), TOK))
                assert scores == [s for _, _, s, _ in uniq]


# ---- GPU: the operator ----------------------------------------------------------------------------------------------------------
def _exact_operands(B, W, S, E, seed, scale_log2=None):
    """Small-integer p and memory: every dot product is an integer below 2^24, exact in fp32 in ANY summation order, so both code
    paths reduce exactly the logits this function returns (p carries a power-of-two scale that brings them to a softmax-sized
    spread: standard deviation ~4).  -> p [B, E], memory [W, S, E], exact fp64 logits [B, S]."""
    g = torch.Generator().manual_seed(seed)
    pi = torch.randint(-3, 4, (B, E), generator=g).double()
    mem = torch.randint(-3, 4, (W, S, E), generator=g).double()
    if scale_log2 is None:
        scale_log2 = -int(round(math.log2(4.0 * math.sqrt(E)))) + 2
    p = pi * 2.0 ** scale_log2
    logits = torch.einsum("be,bse->bs", p, mem[torch.arange(B) // (B // W)])
    return p.float(), mem.float(), logits


def _masks(B, W, S, seed, short_kv):
    """Padding mask [W, S] (with kv_len: full, or shorter than S and 0 for the last wireframe), extra mask [B, S] with row 1
    masked entirely.  Key 0 of every other row stays live."""
    g = torch.Generator().manual_seed(seed + 77)
    mask = torch.rand(W, S, generator=g) < 0.2
    extra = torch.rand(B, S, generator=g) < 0.2
    mask[:, 0] = False
    extra[:, 0] = False
    extra[1, :] = True
    kv = torch.full((W,), S, dtype=torch.int32)
    if short_kv:
        for w in range(W):
            kv[w] = max(1, S - 1 - 3 * w)
            mask[w, kv[w]:] = True
        if W > 1:
            kv[W - 1] = 0
            mask[W - 1, :] = True
    return mask, extra, kv


@pytest.mark.gpu
@pytest.mark.parametrize("E", [64, 512, 1028])
@pytest.mark.parametrize("S", [1, 4, 63, 64, 65, 130, 292])
def test_operator_logprob_on_both_code_paths(hip_lib, S, E):
    from faceformer_amd.hip import ops
    for B, spg in ((5, 1), (8, 4)):
        W = B // spg
        p, mem, exact = _exact_operands(B, W, S, E, seed=S * 7 + E + B)
        for short_kv in (False, True):
            mask, extra, kv = _masks(B, W, S, S + E + B, short_kv)
            dead = mask[torch.arange(B) // spg] | extra | (torch.arange(S)[None, :] >= kv[torch.arange(B) // spg, None])
            want_logits = exact.masked_fill(dead, FILL).float()
            assert torch.equal(want_logits.double(), exact.masked_fill(dead, FILL))        # the premise: exact in fp32
            args = (p.cuda(), mem.cuda(), mask.to(torch.uint8).cuda(), kv.cuda(), extra.to(torch.uint8).cuda())
            for gemm_path in (False, True):
                base = ops.pointer_argmax(*args, seqs_per_group=spg, want_logits=gemm_path)
                res = ops.pointer_argmax(*args, seqs_per_group=spg, want_logits=gemm_path, want_logprob=True)
                assert "logprob" not in base and tuple(res["logprob"].shape) == (B,)
                for key in base:                       # next, best, second (and logits): bit-equal with and without
                    assert torch.equal(base[key], res[key]), (key, B, short_kv, gemm_path)
                # the logits the kernel reduced: its own output (GEMM path); the exact ones (streaming path keeps none)
                logits = res["logits"].cpu() if gemm_path else want_logits
                assert torch.equal(logits, want_logits)
                nxt = res["next"].cpu().long()
                assert torch.equal(nxt, torch.argmax(logits, dim=1))
                assert torch.equal(res["best"].cpu(), logits.max(dim=1).values)
                ref = _ref_logprob(logits, nxt)
                got = res["logprob"].cpu().double()
                err = float((got - ref).abs().max())
                print("S=%d E=%d B=%d kv<S=%d gemm=%d  max |dlogprob| = %.3g" % (S, E, B, short_kv, gemm_path, err))
                assert torch.isfinite(got).all() and float(got.max()) <= 0.0
                assert err <= LP_BAR, (B, short_kv, gemm_path, err)
                all_dead = dead.all(dim=1)
                assert bool(all_dead[1]) and (not short_kv or W == 1 or bool(all_dead[-1]))
                assert float((got[all_dead] + math.log(S)).abs().max()) <= LP_BAR           # every key masked: -log S
                assert nxt[all_dead].tolist() == [0] * int(all_dead.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("S,E", [(9, 64), (130, 512), (292, 1028)])
def test_operator_logprob_of_an_exact_tie_and_of_large_logits(hip_lib, S, E):
    from faceformer_amd.hip import ops
    # two identical memory rows at the maximum: the lower index, and at most log(1/2)
    mem = torch.zeros(1, S, E)
    lo, hi = S // 3, S - 1
    mem[0, lo] = 1.0
    mem[0, hi] = 1.0
    mem[0, 0, 0] = 0.5
    p = torch.full((2, E), 2.0 ** -4)
    for gemm_path in (False, True):
        res = ops.pointer_argmax(p.cuda(), mem.cuda(), seqs_per_group=2, want_logits=gemm_path, want_logprob=True)
        assert res["next"].cpu().tolist() == [lo, lo]
        got = res["logprob"].cpu().double()
        assert float(got.max()) <= -math.log(2.0)
        logits = torch.einsum("be,se->bs", p.double(), mem[0].double()).float()              # (exact: sums of 2^-4)
        assert float((got - _ref_logprob(logits, res["next"].cpu())).abs().max()) <= LP_BAR
    # logits scaled to +-1e4: finite, <= 0, and the bar still holds (nothing overflows, nothing cancels)
    pb, memb, exact = _exact_operands(4, 2, S, E, seed=S + E, scale_log2=3)
    scale = float(exact.abs().max())
    k = int(math.floor(math.log2(1.0e4 / scale)))
    pb, exact = pb * 2.0 ** k, exact * 2.0 ** k
    assert 5.0e3 <= float(exact.abs().max()) <= 1.0e4 and torch.equal(exact.float().double(), exact)
    for gemm_path in (False, True):
        res = ops.pointer_argmax(pb.cuda(), memb.cuda(), seqs_per_group=2, want_logits=gemm_path, want_logprob=True)
        got = res["logprob"].cpu().double()
        assert torch.isfinite(got).all() and float(got.max()) <= 0.0
        assert torch.equal(res["best"].cpu().double(), exact.max(dim=1).values)
        assert float((got - _ref_logprob(exact.float(), res["next"].cpu())).abs().max()) <= LP_BAR


# ---- GPU: the engine ------------------------------------------------------------------------------------------------------------
ENGINE_GOLDENS = ["par_small_gain4", "par_small_ragged300", "par_small_extramask", "par_small_earlybreak",
                  "seq_small_repeat_eos", "seq_small_extramask"]


def _decode(model, case, batch, **kw):
    from faceformer_amd.hip import lib as L
    eng, memory, mask, kv_len = model._encode(batch)
    T = case["model"]["seq_len"]
    opts = dict(extra_mask=model._extra_mask(batch), flags=model.decode_flags, x3_min_rows=model.x3_min_rows,
                chunk_wireframes=model.chunk_wireframes, chunk_max_seqs=model.chunk_max_seqs)
    if case["kind"] == "parallel":
        ni = [int(n) for n in batch["num_input"]]
        opts.update(F=max(ni), num_input=ni, sync_every=model.sync_every, chunk_seqs=model.chunk_seqs,
                    num_streams=model.num_streams, ln_fuse_max_rows=model.ln_fuse_max_rows)
        variant = L.FF_PARALLEL
    else:
        opts.update(F=1, sync_every=1, return_pointer=True)
        variant = L.FF_SEQ2SEQ
    opts.update(kw)
    out = eng.decode(memory, mask, kv_len, variant, T=T, **opts)
    out["engine"] = eng
    return out


def _check_against_own_trace(out, T, keep=None, what=""):
    """logprob[b, j + 1] against fp64 log_softmax of the call's own traced logits [j, b] at the call's own token; exact zeros in
    column 0 and outside `keep` (default: positions <= steps).  Returns the largest error."""
    steps = out["steps"]
    pred = out["predict"].reshape(-1, T)
    lp = out["logprob"].reshape(-1, T)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == tuple(pred.shape)
    if keep is None:
        keep = (torch.arange(T) <= steps)[None, :].expand(pred.shape[0], T)
    keep = torch.as_tensor(keep).to(lp.device)
    assert bool((lp[:, 0] == 0).all()) and bool((lp[~keep] == 0).all())
    assert bool((lp <= 0).all()) and bool(torch.isfinite(lp).all())
    worst = 0.0
    for j in range(steps):
        rows = keep[:, j + 1]
        if not bool(rows.any()):
            continue
        logits = out["logits"][j][rows]
        assert bool(torch.isfinite(logits).all())
        tok = pred[rows, j + 1]
        assert torch.equal(tok, torch.argmax(logits, dim=1))
        err = float((lp[rows, j + 1].double() - _ref_logprob(logits, tok)).abs().max())
        worst = max(worst, err)
        assert err <= LP_BAR, (what, j, err)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "f32"])
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_logprob_is_the_log_softmax_of_its_own_logits(hip_lib, name, form):
    from faceformer_amd.hip import lib as L
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    if form == "f32":
        model.x3_min_rows = 0
    b = batch_to(batch, "cuda")
    T = case["model"]["seq_len"]
    try:
        for fold in (1, 0):
            L.check(hip_lib.ff_set_tuning(b"FF_POINTER_FOLD", fold), "ff_set_tuning")
            base = _decode(model, case, b)
            out = _decode(model, case, b, logprob=True, trace=True)
            assert "logprob" not in base
            assert out["steps"] == base["steps"] and torch.equal(out["predict"], base["predict"])
            worst = _check_against_own_trace(out, T, what=(name, form, fold))
            print(name, form, "FF_POINTER_FOLD=%d" % fold, "steps", out["steps"], "max |dlogprob| = %.3g" % worst)
    finally:
        L.check(hip_lib.ff_reset_tuning(), "ff_reset_tuning")


@pytest.mark.gpu
def test_workspace_without_the_option_is_the_plain_one(hip_lib):
    """ff_decode_lp_workspace_bytes = ff_decode_workspace_bytes + the 256-byte-aligned [T-1, sequences] fp32 array: the plain
    query does not know about the option.  `sequences` is the plan's compact count: N * F without padding-anchor
    de-duplication, sum(min(F, n + 1)) with it when every wireframe is its own micro-batch (both exact); a micro-batch of
    several wireframes is as wide as its widest one, so there the count lies between that sum and N * F."""
    import ctypes as C
    from faceformer_amd.hip import lib as L
    case, z = load_golden("par_small_ragged300")
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    eng = model.engine()
    ni = [int(n) for n in batch["num_input"]]
    N, F, T = len(ni), max(ni), case["model"]["seq_len"]
    ni_host = (C.c_int * N)(*ni)
    compact = sum(min(F, n + 1) for n in ni)
    assert compact < N * F
    DD, RET = L.FF_DEDUP_PAD_ANCHORS, L.FF_RETIRE_FINISHED

    def lp_rows(seqs):
        return ((T - 1) * seqs * 4 + 255) // 256 * 256
    for flags, cw, cs, lo, hi in ((35, 1, 0, N * F, N * F), (3, 0, 7, N * F, N * F), (DD | 35, 1, 0, compact, compact),
                                  (DD | RET | 35, 1, 0, compact, compact), (DD | 35, 16, 0, compact, N * F),
                                  (DD | RET | 35, 2, 0, compact, N * F)):
        prm = L.DecodeParams()
        prm.variant, prm.N, prm.L, prm.F, prm.T = L.FF_PARALLEL, N, case["model"]["L"], F, T
        prm.chunk_wireframes, prm.chunk_seqs, prm.flags, prm.term_lo, prm.term_hi = cw, cs, flags, 1, 4
        plain = hip_lib.ff_decode_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host)
        with_lp = hip_lib.ff_decode_lp_workspace_bytes(C.byref(eng.model), C.byref(prm), ni_host)
        assert plain > 0 and lp_rows(lo) <= with_lp - plain <= lp_rows(hi), (flags, cw, cs, plain, with_lp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS + ["par_full_B256_gain4"])
def test_engine_logprob_against_the_reference_logits(hip_lib, name):
    """The stored rows of the golden, while the sequence's prefix equals the reference's (the rule of compare_with_golden: a row
    leaves only from the first step at which the reference's own top-2 margin is <= 2 tol and the tokens differ)."""
    from test_parity_golden import _tol
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    T = case["model"]["seq_len"]
    out = _decode(model, case, batch_to(batch, "cuda"), logprob=True)
    steps = int(z["steps"])
    assert out["steps"] == steps
    pred = out["predict"].cpu().numpy().reshape(-1, T)
    lp = out["logprob"].cpu().numpy().reshape(-1, T).astype(np.float64)
    gold = z["predict"].reshape(-1, T)
    alive = np.ones(gold.shape[0], dtype=bool)
    through = {int(b): -1 for b in z["logit_rows"]}
    worst = 0.0
    for s in range(steps):
        tol = _tol(z["logits"][s])
        for ri, b in enumerate(z["logit_rows"]):
            if alive[b]:
                ref = float(_ref_logprob(torch.from_numpy(z["logits"][s, ri]), torch.tensor(int(gold[b, s + 1]))))
                d = abs(lp[b, s + 1] - ref)
                worst = max(worst, d / (2 * tol + LP_BAR))
                assert d <= 2 * tol + LP_BAR, "step %d seq %d: |dlogprob| = %g > %g" % (s, b, d, 2 * tol + LP_BAR)
                through[int(b)] = s
        same = pred[:, s + 1] == gold[:, s + 1]
        must = alive & (z["margin"][s] > 2 * tol)
        assert same[must].all(), (s, np.where(must & ~same)[0][:8])
        alive &= same
    print(name, "worst |dlogprob| / bar = %.3f" % worst, "rows compared through their last step:",
          sum(v == steps - 1 for v in through.values()), "of", len(through))
    assert any(v == steps - 1 for v in through.values())
    assert (lp[:, 0] == 0).all() and (lp[:, steps + 1:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_gain4", "par_small_ragged300"])
def test_retired_decode_logprob(hip_lib, name):
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    b = batch_to(batch, "cuda")
    T = case["model"]["seq_len"]
    base = _decode(model, case, b)
    full = base["predict"].cpu().numpy().reshape(-1, T)
    want, s_r = faces.retired_view(full, TOK, return_steps=True)
    out = _decode(model, case, b, retire=True, term_range=(1, 4), logprob=True, trace=True)
    assert out["steps"] == s_r
    assert np.array_equal(out["predict"].cpu().numpy().reshape(-1, T), want)
    if "gain4" in name:
        assert np.array_equal(want, faces.retired_view(z["predict"], TOK).reshape(-1, T))
    keep = faces._retired_keep(full, TOK)
    assert not keep.all()
    worst = _check_against_own_trace(out, T, keep=keep, what=name)
    print(name, "retired: max |dlogprob| = %.3g" % worst)


# ---- GPU: the models ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_gain4", "seq_small_repeat_eos", "par_small_postnorm_gelu"])
def test_model_return_logprob(hip_lib, name):
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    T = case["model"]["seq_len"]
    assert model.return_logprob is False
    with torch.no_grad():
        off = model(batch_to(batch, "cuda"))
        model.return_logprob = True
        if not model.engine_supported():
            model._module_trace = []
        on = model(batch_to(batch, "cuda"))
    assert "predict_logprob" not in off and set(on) == set(off) | {"predict_logprob"}      # off: exactly today's keys
    assert torch.equal(on["predict"], off["predict"])
    lp = on["predict_logprob"]
    assert lp.dtype == torch.float32 and tuple(lp.shape) == tuple(on["predict"].shape) and lp.is_cuda
    if model.engine_supported():
        traced = _decode(model, case, batch_to(batch, "cuda"), trace=True, logprob=True)
        assert torch.equal(traced["predict"].reshape(-1, T), on["predict"].reshape(-1, T))
        logits, steps = traced["logits"], traced["steps"]
    else:
        logits, steps = torch.stack(model._module_trace), len(model._module_trace)
    out = dict(steps=steps, predict=on["predict"], logprob=lp, logits=logits)
    worst = _check_against_own_trace(out, T, what=name)
    print(name, "model: steps", steps, "max |dlogprob| = %.3g" % worst)
