"""Teacher-forced scoring of given face loops (ff_pointer_forced / ff_decode_forced, PathEngine.score, the models' score();
DESIGN.md 14).

The contract is the decode loop fed a given path: step t re-encodes the forced prefix 0..t with the unmasked decoder, forms the
masked logit row l as select_next leaves it, scores g = paths[:, t + 1] and appends g (never the argmax):
  logprob = (l[g] - m) - log sum exp(l - m), fp32, saturated at -FLT_MAX;  greedy = argmax l (lowest index on ties);
  rank = #{s : l[s] > l[g], or l[s] == l[g] and s < g}.

Bars, none measured:
  operator, against numpy fp64 on the kernel's OWN masked fp32 logits: greedy and rank exact; logprob within
      2^-16 + 2^-23 |logprob| (DESIGN.md 12's bar for the sum, plus one fp32 subtraction l[g] - m and one fp32 addition, each
      half an ulp of a value no larger than |logprob| + log S);
  engine, against the fp64 oracle forced along the same paths (oracle/refpath.py forced= / steps= / seqs=): traced logits within
      tol = test_parity_golden._tol(step); logprob within 2 tol + 2^-16 + 2^-23 |logprob| (every term of l[g] - logsumexp(l)
      moves by at most tol); greedy equal wherever the oracle's top-2 margin exceeds 2 tol; rank equal wherever no other logit
      lies within 2 tol of l[g]; at most 2 % of the scored pairs may leave the greedy / rank comparison (tests/forced_ref.py CAP;
      the shares of the seeds used here, from tools/forced_left_out.py on the CPU, are in DESIGN.md 14).
"""
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import forced_ref as FR
from conftest import ROOT, batch_to, build_model, case_weights_and_batch, load_golden, token_ns
from faceformer_amd import faces

TOK = token_ns()
FILL = FR.FILL32


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_score_summary_on_a_hand_written_case():
    #  wireframe 0: two rows (3 and 1 scored tokens); wireframe 1: nothing scored
    paths = np.array([[[5, 6, 7, 2, 0], [4, 9, 0, 0, 0]], [[3, 0, 0, 0, 0], [3, 0, 0, 0, 0]]])
    lengths = np.array([[3, 1], [0, 0]])
    logprob = np.array([[[0, -0.5, -1.0, -0.25, 0], [0, -2.0, 0, 0, 0]], [[0.0] * 5, [0.0] * 5]])
    rank = np.array([[[0, 0, 2, 0, 0], [0, 5, 0, 0, 0]], [[0] * 5, [0] * 5]])
    greedy = np.where(rank == 0, paths, 99)
    greedy[..., 0] = paths[..., 0]
    sm = faces.score_summary(logprob, greedy, rank, paths, lengths)
    assert sm["tokens"].tolist() == [4, 0]
    assert sm["nll"][0] == pytest.approx(3.75 / 4, abs=0, rel=1e-15) and math.isnan(sm["nll"][1])
    assert sm["tf_accuracy"][0] == 0.5 and sm["mean_rank"][0] == 7 / 4
    assert math.isnan(sm["tf_accuracy"][1]) and math.isnan(sm["mean_rank"][1])
    # seq2seq layout: [N, T] with lengths [N]
    s2 = faces.score_summary(logprob[0], greedy[0], rank[0], paths[0], lengths[0])
    assert s2["tokens"].tolist() == [3, 1] and s2["nll"].tolist() == [1.75 / 3, 2.0] and s2["tf_accuracy"].tolist() == [2 / 3, 0.0]
    bad = greedy.copy()
    bad[0, 0, 1] = 98                                       # rank 0 where greedy differs from the path: inconsistent inputs
    with pytest.raises(ValueError):
        faces.score_summary(logprob, bad, rank, paths, lengths)
    with pytest.raises(ValueError):
        faces.score_summary(logprob, greedy, rank, paths, lengths[0])


def test_numpy_rule_on_a_hand_written_row():
    l = np.array([[1.0, 3.0, 3.0, FILL, 2.0]], dtype=np.float32)
    z = math.log(math.exp(-2) + 2 + math.exp(-1))
    for g, lp, rk in ((1, -z, 0), (2, -z, 1), (4, -1 - z, 2), (0, -2 - z, 3), (3, -FR.FLT_MAX, 4)):
        got = FR.forced_rule(l, [g])
        assert got[0][0] == pytest.approx(lp, rel=1e-15) and got[1][0] == 1 and got[2][0] == rk
    dead = np.full((1, 7), FILL, dtype=np.float32)
    lp, gr, rk = FR.forced_rule(dead, [4])
    assert lp[0] == pytest.approx(-math.log(7)) and gr[0] == 0 and rk[0] == 4


def test_header_and_binding_declare_the_forced_entries():
    import re
    from faceformer_amd.hip import lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ff_pointer_forced", "ff_decode_forced", "ff_decode_forced_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in lib.SIGNATURES
        nargs = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).count(",") + 1
        assert len(lib.SIGNATURES[name][1]) == nargs, name
    doc = header[: re.search(r"\bint ff_pointer_forced\s*\(", header).start()].rsplit("/* ----", 1)[1]
    for cite in ("model_para.py:216-233", "model.py:169-219", "model_para.py:173-179", "model.py:161-167", "CLAMPED"):
        assert cite in doc, cite
    assert [f[0] for f in lib.ForcedParams._fields_] == re.findall(r"(\w+);", re.search(
        r"typedef struct ff_forced_params \{(.*?)\}", code, flags=re.S).group(1))


def test_cli_flag_reaches_run_test_and_is_refused_in_combinations(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import default_cfg
    assert cli.build_parser().parse_args(["--test_ckpt", "x", "--score-labels"]).score_labels is True
    assert cli.build_parser().parse_args(["--test_ckpt", "x"]).score_labels is False
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--score-labels", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [kw["score_labels"] for kw in seen] == [True, False]

    class TwoRanks:
        get_world_size = staticmethod(lambda: 2)
        get_rank = staticmethod(lambda: 0)
    with pytest.raises(ValueError, match="multi-rank"):
        run_test(default_cfg(), None, out_dir="unused", device="cpu", model=object(), dist_mod=TwoRanks, score_labels=True)
    for kw in (dict(scores=True), dict(beam=2), dict(retire_finished=True)):
        with pytest.raises(ValueError, match="score-labels"):
            run_test(default_cfg(), None, out_dir="unused", device="cpu", model=object(), score_labels=True, **kw)


# ---- GPU: the operator ----------------------------------------------------------------------------------------------------------
def _seg_stats(x64):
    seg = x64.reshape(x64.shape[0], -1, 32)
    mean = seg.mean(dim=2)
    return torch.stack([mean, ((seg - mean[..., None]) ** 2).sum(dim=2)], dim=2)


def _operator_case(B, spg, S, E, seed, masks, ties):
    """-> raw logits [B, S], forced [B], memory [W, S, E], mask [W, S] or None, kv_len [W] or None, dead [B, S] bool."""
    g = torch.Generator().manual_seed(seed)
    W = (B + spg - 1) // spg
    logits = (torch.rand(B, S, generator=g) * 2 - 1) * 1.0e4
    logits[1::2] = torch.randn(B, S, generator=g)[1::2] * 4.0            # every other row at a softmax-sized spread
    forced = torch.randint(0, S, (B,), generator=g, dtype=torch.int32)
    memory = torch.randn(W, S, E, generator=g)
    mask = kv = None
    dead = torch.zeros(B, S, dtype=torch.bool)
    wf = torch.arange(B) // spg
    if masks:
        mask = torch.rand(W, S, generator=g) < 0.25
        mask[:, 0] = False
        kv = torch.tensor([max(1, S - 1 - 2 * w) for w in range(W)], dtype=torch.int32)
        if W > 1:                                                        # the last wireframe: every key masked
            kv[W - 1] = 0
        dead = mask[wf] | (torch.arange(S)[None, :] >= kv[wf, None])
        for b in range(B):                                               # forced keys on both sides of kv_len, live and masked
            k = int(kv[wf[b]])
            forced[b] = [min(k, S - 1), max(k - 1, 0), S - 1, 0][b % 4]
    if ties:
        for b in range(B):                                               # exact ties of the forced value, below and above it
            v = float(logits[b, forced[b]])
            logits[b, torch.randperm(S, generator=g)[: max(1, S // 3)]] = v
    live = logits.masked_fill(dead, FILL)
    forced[0] = int(live[0].argmax())                                    # row 0: the forced token is the argmax
    return logits, forced, memory, mask, kv, dead


@pytest.mark.gpu
@pytest.mark.parametrize("E", [64, 512])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 292])
def test_operator_against_numpy_fp64(hip_lib, S, E):
    from faceformer_amd.hip import ops
    spg = 3
    for B in (1, 5, 9):
        for masks, ties in ((False, False), (True, False), (False, True), (True, True)):
            raw, forced, memory, mask, kv, dead = _operator_case(B, spg, S, E, S * 131 + E + B + 2 * masks + ties, masks, ties)
            lg = raw.clone().cuda()
            res = ops.pointer_forced(lg, forced.cuda(), memory.cuda(), None if mask is None else mask.to(torch.uint8).cuda(),
                                     None if kv is None else kv.cuda(), seqs_per_group=spg, want_rows=True, want_stats=True)
            own = lg.cpu()
            assert torch.equal(own, raw.masked_fill(dead, FILL))          # masked in place, as select_next leaves the row
            lp, gr, rk = FR.forced_rule(own.numpy(), forced.numpy())
            what = (B, masks, ties)
            assert np.array_equal(res["greedy"].cpu().numpy(), gr), what  # exact, ties included
            assert np.array_equal(res["rank"].cpu().numpy(), rk), what
            got = res["logprob"].cpu().numpy().astype(np.float64)
            err = np.abs(got - lp)
            bar = FR.LP_BAR + FR.EPS * np.abs(lp)
            print("S=%d E=%d B=%d masks=%d ties=%d max |dlogprob| / bar = %.3g" % (S, E, B, masks, ties, (err / bar).max()))
            assert (err <= bar).all(), (what, err.max())
            assert rk[0] == 0 and gr[0] == forced[0]                      # the forced token that is the argmax
            all_dead = dead.all(dim=1).numpy()
            fdead = dead[torch.arange(B), forced.long()].numpy()
            assert (got[fdead & ~all_dead] == -FR.FLT_MAX).all()           # a masked forced key: exactly -FLT_MAX
            assert (np.abs(got[all_dead] + math.log(S)) <= FR.LP_BAR + FR.EPS * math.log(S)).all()   # every key masked: -log S
            if masks and B > spg and S > 3:                               # (the cases the shapes are there for)
                assert all_dead.any() and (fdead & ~all_dead).any() and (~fdead).any()
            want_rows = memory[torch.arange(B) // spg, forced.long()]
            assert torch.equal(res["rows"].cpu(), want_rows), what        # bit for bit
            want = _seg_stats(want_rows.double())
            st = res["stats"].cpu().double()
            assert (st[..., 0] - want[..., 0]).abs().max() < 1e-5
            assert ((st[..., 1] - want[..., 1]).abs() / want[..., 1].clamp_min(1e-6)).max() < 1e-5


@pytest.mark.gpu
def test_operator_refuses_tokens_outside_the_keys(hip_lib):
    from faceformer_amd.hip import ops
    lg = torch.zeros(2, 9).cuda()
    for bad in ([0, 9], [-1, 3]):
        with pytest.raises(ValueError, match=r"\[0, 9\)"):
            ops.pointer_forced(lg, torch.tensor(bad, dtype=torch.int32).cuda())


# ---- GPU: the engine ------------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name):
    """(case, z, model, cuda batch, sd, cpu batch) of a golden, built once per session."""
    if name not in _MODELS:
        case, z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        _MODELS[name] = (case, z, build_model(case, sd, "cuda"), batch_to(batch, "cuda"), sd, batch)
    return _MODELS[name]


def _score(model, case, b, paths, lengths, F, encoded=None, **kw):
    from faceformer_amd.hip import lib as L
    eng, memory, mask, kv_len = encoded or model._encode(b)
    opts = dict(flags=model.decode_flags, x3_min_rows=model.x3_min_rows, chunk_wireframes=model.chunk_wireframes,
                chunk_max_seqs=model.chunk_max_seqs, chunk_seqs=model.chunk_seqs, num_streams=model.num_streams,
                ln_fuse_max_rows=model.ln_fuse_max_rows)
    opts.update(kw)
    variant = L.FF_PARALLEL if case["kind"] == "parallel" else L.FF_SEQ2SEQ
    return eng.score(memory, mask, kv_len, variant, case["model"]["seq_len"], torch.as_tensor(paths).cuda(), lengths, F=F, **opts)


_TRUTH = {}


def _truth(name, case, sd, batch, paths, steps, rows):
    """fp64 masked logits [steps, len(rows), S] of the oracle forced along `paths`, evaluated on the GPU once per golden."""
    if name not in _TRUTH:
        from oracle import refpath
        sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
        b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}
        fn = refpath.parallel_forward_eval if case["kind"] == "parallel" else refpath.seq2seq_forward_eval
        tr = {}
        fn(sd64, b64, num_head=case["model"]["H"], trace=tr, forced=torch.from_numpy(paths).cuda(), steps=steps,
           seqs=torch.tensor(rows).cuda() if name in FR.SUBSET else None)
        _TRUTH[name] = torch.stack(tr["logits"]).cpu().numpy()
    return _TRUTH[name]


def _check_layout(out, paths, lengths):
    """Column 0 and everything past lengths[r]; seq_logprob against the fp64 sum of the run's own per-token values."""
    T = paths.shape[1]
    lp, gr, rk = (out[k].cpu().numpy() for k in ("logprob", "greedy", "rank"))
    assert lp.dtype == np.float32 and gr.dtype == np.int64 and rk.dtype == np.int32 and lp.shape == gr.shape == rk.shape == paths.shape
    past = np.arange(T)[None, :] > lengths[:, None]
    assert (lp[past] == 0).all() and (gr[past] == 0).all() and (rk[past] == 0).all()
    assert (lp[:, 0] == 0).all() and (rk[:, 0] == 0).all() and np.array_equal(gr[:, 0], paths[:, 0])
    assert np.isfinite(lp).all() and (lp <= 0).all()
    assert out["steps"] == int(lengths.max())
    want = lp.astype(np.float64).sum(axis=1)
    bound = lengths * FR.EPS * np.abs(lp).max(axis=1)
    assert (np.abs(out["seq_logprob"].cpu().numpy().astype(np.float64) - want) <= bound).all()
    assert ((rk == 0) == (gr == paths))[~past & (np.arange(T)[None, :] >= 1)].all()       # rank 0 <=> greedy == g
    return lp, gr, rk


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_gain4", "par_small_ragged", "seq_full_A4_gain4", "par_full_n40_gain4"])
def test_engine_against_the_forced_fp64_oracle(hip_lib, name):
    from test_parity_golden import _tol
    case, z, model, b, sd, batch = _model(name)
    paths, lengths, F = FR.make_paths(case, FR.SEEDS[name])
    rows = FR.SUBSET.get(name) or list(range(paths.shape[0]))
    assert {0, 1, case["model"]["seq_len"] - 1} <= set(lengths[rows].tolist())
    out = _score(model, case, b, paths, lengths, F, trace=True)
    lp, gr, rk = _check_layout(out, paths, lengths)
    steps = int(lengths[rows].max())
    truth = _truth(name, case, sd, batch, paths, steps, rows)
    st = FR.compare(truth, rows, paths, lengths, out["logits"].cpu().numpy(), lp, gr, rk, tol_fn=_tol, what=name)
    print(name, "scored pairs %d, left out of greedy / rank %.2f %%, worst |dlogit| / tol %.3f, worst |dlogprob| / bar %.3f"
          % (st["pairs"], 100 * st["left_out"], st["worst_logit"], st["worst_lp"]))
    assert st["pairs"] == int(lengths[rows].sum()) and st["left_out"] <= FR.CAP


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_gain4", "seq_full_A4_gain4"])
def test_forcing_a_decode_along_its_own_tokens(hip_lib, name):
    """The golden's own `predict` as the path: greedy == paths and rank 0 wherever the golden's margin is decisive, and the
    log-probabilities of the greedy decode (return_logprob) within 2 tol + 2^-16: the two runs may be planned into different
    micro-batches, so they agree to the bar and not to the bit."""
    from test_logprob import _decode
    from test_parity_golden import _tol
    case, z, model, b, sd, batch = _model(name)
    T = case["model"]["seq_len"]
    gold = z["predict"].reshape(-1, T)
    steps = int(z["steps"])
    if case["kind"] == "parallel":
        term = (gold >= TOK.face_type_offset) & (gold < TOK.len)
        fin = np.where(term.any(axis=1), term.argmax(axis=1), T)          # faces.retired_view's fin
        assert np.array_equal(np.where(np.arange(T)[None, :] <= np.minimum(fin, steps)[:, None], gold, 0), faces.retired_view(gold, TOK))
        lengths, F = np.minimum(fin, steps), gold.shape[0] // len(case["n_edges"])
    else:
        eos = gold == TOK.EOS
        lengths, F = np.where(eos.any(axis=1), eos.argmax(axis=1), steps), 1
    lengths = np.minimum(lengths, T - 1).astype(np.int64)
    out = _score(model, case, b, gold, lengths, F)
    lp, gr, rk = _check_layout(out, gold, lengths)
    greedy = _decode(model, case, b, logprob=True)
    glp = greedy["logprob"].cpu().numpy().reshape(-1, T).astype(np.float64)
    gpred = greedy["predict"].cpu().numpy().reshape(-1, T)
    checked = 0
    for s in range(int(lengths.max())):
        tol = _tol(z["logits"][s])
        on = (lengths > s) & (gpred[:, : s + 2] == gold[:, : s + 2]).all(axis=1)       # scored here, and the greedy run took this path
        sure = on & (z["margin"][s] > 2 * tol)
        assert (gr[sure, s + 1] == gold[sure, s + 1]).all() and (rk[sure, s + 1] == 0).all()
        assert (np.abs(lp[on, s + 1] - glp[on, s + 1]) <= 2 * tol + FR.LP_BAR).all(), (name, s)
        checked += int(sure.sum())
    print(name, "decisive pairs checked:", checked, "of", int(lengths.sum()))
    assert checked > 0.5 * lengths.sum()


@pytest.mark.gpu
def test_micro_batching_and_repeatability(hip_lib):
    from test_parity_golden import _tol
    name = "par_small_ragged"
    case, z, model, b, sd, batch = _model(name)
    paths, lengths, F = FR.make_paths(case, FR.SEEDS[name])
    whole = _score(model, case, b, paths, lengths, F, chunk_wireframes=0, trace=True)
    again = _score(model, case, b, paths, lengths, F, chunk_wireframes=0, trace=True)
    one = _score(model, case, b, paths, lengths, F, chunk_wireframes=1)
    for k in ("logprob", "greedy", "rank", "seq_logprob"):
        assert torch.equal(whole[k], again[k]), k                        # one plan, two runs: bit-equal
    assert torch.equal(whole["logits"].nan_to_num(7.0), again["logits"].nan_to_num(7.0))
    a, c = whole["logprob"].cpu().numpy().astype(np.float64), one["logprob"].cpu().numpy().astype(np.float64)
    truth = _truth(name, case, sd, batch, paths, int(lengths.max()), list(range(paths.shape[0])))
    worst = 0.0
    for s in range(int(lengths.max())):
        rows = lengths > s
        tol = _tol(truth[s])                                             # (from the oracle's logits, as the engine test takes it)
        bar = 2 * tol + FR.LP_BAR + FR.EPS * np.abs(a[rows, s + 1])      # ONE bar: the two plans differ by summation order only
        d = np.abs(a[rows, s + 1] - c[rows, s + 1])
        worst = max(worst, float((d / bar).max()))
        assert (d <= bar).all(), s
    print("chunk_wireframes = 1 against the whole batch: worst |dlogprob| / bar = %.3g" % worst)
    _check_layout(one, paths, lengths)


@pytest.mark.gpu
def test_nothing_to_score_makes_no_decoder_launch(hip_lib):
    from faceformer_amd.hip import lib as L
    case, z, model, b, sd, batch = _model("par_small_gain4")
    paths, lengths, F = FR.make_paths(case, 5)
    zero = np.zeros_like(lengths)
    encoded = model._encode(b)                                           # (the encoder's launches stay outside the bracket)
    torch.cuda.synchronize()
    L.check(hip_lib.ff_profile_begin(), "ff_profile_begin")
    try:
        out = _score(model, case, b, paths, zero, F, encoded=encoded)
    finally:
        import ctypes as C
        ms, work, launches = (C.c_double * 16)(), (C.c_double * 16)(), (C.c_longlong * 16)()
        L.check(hip_lib.ff_profile_end(ms, work, launches, 16), "ff_profile_end")
    _check_layout(out, paths, zero)
    assert out["steps"] == 0 and float(out["seq_logprob"].abs().max()) == 0.0
    # no operator launch of any category: no prologue (cross-attention K | V, gathers), no decoder pass, no pointer step -- the
    # call is the token transpose and the packing launch alone, which are no operators and carry no bracket
    assert [int(v) for v in launches] == [0] * 16, list(launches)
    L.check(hip_lib.ff_profile_begin(), "ff_profile_begin")              # ... and with one token to score the bracket does count
    try:
        _score(model, case, b, paths, np.minimum(lengths, 1), F, encoded=encoded)
    finally:
        L.check(hip_lib.ff_profile_end(ms, work, launches, 16), "ff_profile_end")
    assert launches[0] > 0 and launches[1] > 0 and launches[3] > 0, list(launches)


@pytest.mark.gpu
def test_every_excluded_combination_raises_before_a_launch(hip_lib):
    import ctypes as C
    from faceformer_amd.hip import lib as L
    case, z, model, b, sd, batch = _model("par_small_gain4")
    paths, lengths, F = FR.make_paths(case, 5)
    T = case["model"]["seq_len"]
    for kw in (dict(retire=True), dict(beam_width=2), dict(logprob=True), dict(return_pointer=True), dict(stop_callback=lambda c: False),
               dict(stop_each_eos=True), dict(extra_mask=torch.zeros(paths.shape[0], 28, dtype=torch.uint8).cuda()),
               dict(flags=model.decode_flags | L.FF_RETIRE_FINISHED), dict(flags=model.decode_flags | L.FF_RETURN_POINTER),
               dict(flags=model.decode_flags | L.FF_STOP_EACH_EOS)):
        with pytest.raises(ValueError, match="excludes"):
            _score(model, case, b, paths, lengths, F, **kw)
    for bad in (np.full_like(lengths, T), np.full_like(lengths, -1)):                     # lengths outside 0..T-1
        with pytest.raises(ValueError, match="lengths"):
            _score(model, case, b, paths, bad, F)
    worse = paths.copy()
    worse[3, 2] = 28                                                                     # S = 28: one token outside [0, S)
    with pytest.raises(ValueError, match=r"paths\[3, 2\] = 28"):
        _score(model, case, b, worse, np.full_like(lengths, T - 1), F)
    # ... the C entry's own checks: FF_ERR_ARG for the flags, a stop_fn and lengths outside 0..T-1
    eng, memory, mask, kv_len = model._encode(b)
    B = paths.shape[0]
    pt, ln = torch.from_numpy(paths).cuda(), torch.from_numpy(lengths.astype(np.int32)).cuda()
    outs = [torch.empty((B, T), device="cuda", dtype=dt) for dt in (torch.float32, torch.int64, torch.int32)] + [torch.empty(B, device="cuda")]

    def call(flags=model.decode_flags, host=lengths, stop=None):
        prm = L.DecodeParams()
        prm.variant, prm.N, prm.L, prm.F, prm.T, prm.flags = L.FF_PARALLEL, memory.size(0), memory.size(1) - 4, F, T, flags
        if stop is not None:
            prm.stop_fn, prm.sync_every = C.cast(stop, C.c_void_p), 1
        hl = (C.c_int * B)(*[int(v) for v in host])
        fp = L.ForcedParams(pt.data_ptr(), ln.data_ptr(), C.cast(hl, C.POINTER(C.c_int)), *[t.data_ptr() for t in outs])
        ws = torch.empty(hip_lib.ff_decode_forced_workspace_bytes(C.byref(eng.model), C.byref(prm)), device="cuda", dtype=torch.uint8)
        return hip_lib.ff_decode_forced(C.byref(eng.model), C.byref(prm), memory.data_ptr(), mask.data_ptr(), kv_len.data_ptr(),
                                        C.byref(fp), None, None, ws.data_ptr(), ws.numel(), None)
    FF_OK, FF_ERR_ARG = 0, -1                                            # (ff_status of include/faceformer_hip.h)
    cb = L.STOP_FN(lambda u, c, n: 0)
    for kw in (dict(flags=model.decode_flags | L.FF_RETIRE_FINISHED), dict(flags=model.decode_flags | L.FF_RETURN_POINTER),
               dict(flags=model.decode_flags | L.FF_STOP_EACH_EOS), dict(stop=cb), dict(host=np.full_like(lengths, T)),
               dict(host=np.full_like(lengths, -1))):
        assert call(**kw) == FF_ERR_ARG, kw
    torch.cuda.synchronize()
    assert call() == FF_OK
    torch.cuda.synchronize()
    # the models: options of the greedy decode that a forced decode excludes, and the sub-module loop
    for attr, val in (("retire_finished", True), ("beam_width", 2), ("return_logprob", True)):
        old = getattr(model, attr)
        setattr(model, attr, val)
        try:
            with pytest.raises(ValueError, match="excludes"):
                model.score(dict(b), torch.from_numpy(paths).view(-1, F, T), lengths)
        finally:
            setattr(model, attr, old)
    with pytest.raises(ValueError, match="excludes"):
        model.score(dict(b, extra_mask=torch.zeros(B, 24, dtype=torch.bool).cuda()), torch.from_numpy(paths).view(-1, F, T), lengths)
    pcase, _ = load_golden("par_small_postnorm_gelu")
    psd, pbatch = case_weights_and_batch(pcase)
    with pytest.raises(ValueError, match="sub-module loop"):
        build_model(pcase, psd, "cuda").score(batch_to(pbatch, "cuda"))


# ---- GPU: the models and the CLI ------------------------------------------------------------------------------------------------
def _labelled(case, batch, seed):
    """The batch with synthetic data-set labels: rows of live edge tokens ended by a face-type token, PAD behind; unused rows hold
    the one token len - 1 (datasets.pack_parallel_item's layout) -- or SOS ... EOS (pack_seq2seq_item)."""
    rng = np.random.default_rng(seed)
    T, n_edges = case["model"]["seq_len"], case["n_edges"]
    b = dict(batch)
    if case["kind"] == "parallel":
        label = np.zeros(tuple(batch["label"].shape), dtype=np.int64)
        for w, n in enumerate(n_edges):
            used = max(1, n // 2)
            for r in range(used):
                k = int(rng.integers(1, T - 1))
                label[w, r, :k] = TOK.len + rng.integers(0, n, size=k)
                label[w, r, k] = TOK.face_type_offset + int(rng.integers(0, 3))
            label[w, used:, 0] = TOK.len - 1
        b["label"] = torch.from_numpy(label)
        b["label_mask"] = b["label"] == TOK.PAD
    else:
        label = np.zeros(tuple(batch["label"].shape), dtype=np.int64)
        num = []
        for w, n in enumerate(n_edges):
            k = int(rng.integers(3, 12))
            label[w, 0] = TOK.SOS
            label[w, 1:k] = TOK.len + rng.integers(0, n, size=k - 1)
            label[w, k] = TOK.EOS
            num.append(k + 1)
        b["label"], b["num_label"] = torch.from_numpy(label), torch.tensor(num)
        b["label_mask"] = b["label"] == TOK.PAD
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_ragged", "seq_small_gain4"])
def test_model_score_with_the_default_label_paths(hip_lib, name):
    """(The goldens' batches ARE synth batches -- conftest.case_weights_and_batch calls synth.make_wireframes -- with label rows
    filled in the data sets' layout, since synth leaves the labels zero.)"""
    case, z, model, b, sd, batch = _model(name)
    lb = batch_to(_labelled(case, batch, 3), "cuda")
    T = case["model"]["seq_len"]
    with torch.no_grad():
        before = model(dict(lb))
    out = model.score(dict(lb))
    assert set(out) == set(lb) | {"score_logprob", "score_greedy", "score_rank", "score_seq_logprob"}
    if case["kind"] == "parallel":
        F = max(case["n_edges"])
        paths = lb["label"][:, :F].reshape(-1, T)
        lengths = (lb["label"][:, :F, 1:] != TOK.PAD).sum(dim=-1).reshape(-1).cpu().numpy()
        assert (lengths[(paths[:, 0] == TOK.len - 1).cpu().numpy()] == 0).all() and lengths.max() > 1
        shape = (len(case["n_edges"]), F, T)
    else:
        F, paths, lengths, shape = 1, lb["label"], (lb["num_label"] - 1).cpu().numpy(), (len(case["n_edges"]), T)
    want = _score(model, case, lb, paths, lengths, F)
    for k in ("logprob", "greedy", "rank"):
        assert tuple(out["score_" + k].shape) == shape and torch.equal(out["score_" + k].reshape(-1, T), want[k]), k
    assert torch.equal(out["score_seq_logprob"].reshape(-1), want["seq_logprob"])
    sm = faces.score_summary(*(out["score_" + k].cpu().numpy() for k in ("logprob", "greedy", "rank")),
                             paths.view(shape).cpu().numpy(), lengths.reshape(shape[:-1]))
    assert (sm["tokens"] == lengths.reshape(shape[0], -1).sum(axis=1)).all() and (sm["nll"] > 0).all()
    with torch.no_grad():
        after = model(dict(lb))
    assert set(after) == set(before) and torch.equal(after["predict"], before["predict"])    # forward_eval is untouched
    # explicit paths with another F than max(num_input): two rows per wireframe
    if case["kind"] == "parallel":
        two = model.score(dict(lb), lb["label"][:, :2], torch.as_tensor(lengths).view(shape[:2])[:, :2])
        assert tuple(two["score_logprob"].shape) == (shape[0], 2, T)
        # (another plan of the same fp32 arithmetic: one bar, as in test_micro_batching_and_repeatability; tol's floor, since
        #  no oracle is run along the label paths: the smallest bar _tol can give)
        d = (two["score_logprob"] - out["score_logprob"][:, :2]).abs().double()
        assert bool((d <= 2 * 1e-3 + FR.LP_BAR + FR.EPS * out["score_logprob"][:, :2].abs().double()).all()), float(d.max())


@pytest.mark.gpu
def test_cli_score_labels_adds_three_keys_and_changes_nothing_else(hip_lib, tmp_path):
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd import models
    from test_cli import _files, _setup
    root = str(tmp_path / "data")
    cfg, sd = _setup(root)
    model = models.SurfaceFormer_Parallel(**cfg.model)
    model.load_state_dict(sd)
    model = model.eval().cuda()
    plain = _files(cli.run_test(cfg, None, out_dir=str(tmp_path / "plain"), device="cuda", batch_size=3, model=model))
    again = _files(cli.run_test(cfg, None, out_dir=str(tmp_path / "again"), device="cuda", batch_size=3, model=model))
    scored = _files(cli.run_test(cfg, None, out_dir=str(tmp_path / "scored"), device="cuda", batch_size=3, model=model, score_labels=True))
    assert plain == again and sorted(scored) == sorted(plain) and len(plain) == 5          # without the flag: byte-identical
    for fname, text in scored.items():
        rec = json.loads(text)
        assert list(rec)[-3:] == ["label_logprob", "label_nll", "label_tf_accuracy"]
        ll, nll, acc = rec.pop("label_logprob"), rec.pop("label_nll"), rec.pop("label_tf_accuracy")
        assert json.dumps(rec).encode() == plain[fname]                                  # the rest of the record: byte-identical
        assert len(ll) == 7 and all(v < 0 for v in ll)         # 3 + 4 label rows (one per rotation), 3 and 4 scored tokens each
        assert nll == pytest.approx(-sum(ll) / (3 * 3 + 4 * 4), rel=1e-6) and 0.0 <= acc <= 1.0
