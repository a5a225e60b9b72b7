"""The package default's "2 x fp16" products at the edges of fp16's range, on whole models against the fp64 oracle.

split_kind='fp16x2' splits every operand x into x1 = fp16(x) and x2' = fp16((x - x1) 2^11); fp16 has five exponent bits, so the
engine bounds every operand class a priori (faceformer_amd.hip.engine.fp16_operand_bounds) and binds the bf16x3 planes with a
warning when a bound reaches FP16_LIM.  Here each variant of a small model pushes exactly one operand class out of fp16's range
-- where possible by a reparametrisation that leaves the model's function unchanged in exact arithmetic -- and every form of the
engine must then decode finite logits within the fp32-class bars of test_error_against_fp64_truth_is_fp32_class, teacher-forced
along its own tokens.  A large batch decodes more than 65535 (wireframe, head) pairs, more than one launch's grid.y.
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import batch_to, build_model, case_weights_and_batch, golden_names, load_golden
from faceformer_amd.hip.engine import ATTN_Q_SCALE, FP16_LIM, fp16_operand_bounds

TARGET = 2.0 * 65504          # what the pushed operand is aimed at (between 1.5x and 3x fp16's largest value)
CS_SLACK = 3.5                # a Cauchy-Schwarz bound sqrt(E) ||w|| is ~3.5x the largest |x . w| over the rows at E = 128
HEAD = slice(0, 64)           # the head the reparametrisations move


def _ff160_case():
    case, _ = load_golden("par_small_gain4")
    case = dict(case, name="par_small_gain4_ff160", model=dict(case["model"], FF=160))
    return case


def _row_bound(W, gamma, beta, b, table=None):
    """sqrt(E) ||W_n * gamma|| + max |W_n . (beta + t) + b_n| of every row n (the engine's bound)."""
    W, gamma, beta, b = (t.double() for t in (W, gamma, beta, b))
    off = W @ beta + b
    if table is not None:
        off = (off[:, None] + W @ table.double().t()).abs().amax(dim=1)
    return (W * gamma).norm(dim=1) * W.shape[1] ** 0.5 + off.abs()


def make_variant(name):
    """(case, state_dict, batch, operand classes the variant pushes) of one reparametrised model."""
    if name in ("ff up, unfolded", "self V up, unfolded"):
        from faceformer_amd.synth import make_state_dict, state_dict_spec
        case = _ff160_case()
        m = case["model"]
        sd = make_state_dict(state_dict_spec("parallel", m["L"], m["seq_len"], m["E"], m["FF"], m["enc"], m["dec"]),
                             case["recipe"], case["wseed"])
        _, batch = case_weights_and_batch(load_golden("par_small_gain4")[0])
    else:
        case, _ = load_golden("par_small_gain4")
        sd, batch = case_weights_and_batch(case)
    sd = {k: v.clone() for k, v in sd.items()}
    case = dict(case, name="fp16_range: " + name)
    E = case["model"]["E"]
    p = "decoder.layers.0."
    W, b = sd[p + "multihead_attn.in_proj_weight"], sd[p + "multihead_attn.in_proj_bias"]
    ge, be = sd["encoder.norm.weight"], sd["encoder.norm.bias"]
    g1, b1 = sd[p + "norm1.weight"], sd[p + "norm1.bias"]
    g2, b2 = sd[p + "norm2.weight"], sd[p + "norm2.bias"]
    g3, b3 = sd[p + "norm3.weight"], sd[p + "norm3.bias"]
    qpos, pos = sd["query_pos_enc.pos_embed.weight"], sd["pos_enc.pos_embed.weight"]
    q_rows, k_rows = slice(HEAD.start, HEAD.stop), slice(E + HEAD.start, E + HEAD.stop)
    if name == "cross K up":              # q . k unchanged: K of head 0 by c, its q by 1 / c
        c = CS_SLACK * TARGET / float(_row_bound(W[k_rows], ge, be, b[k_rows], pos).max())
        W[k_rows] *= c; b[k_rows] *= c; W[q_rows] /= c; b[q_rows] /= c
        pushed = {"cross-attention keys"}
    elif name == "cross q up":
        c = CS_SLACK * TARGET / (ATTN_Q_SCALE * float(_row_bound(W[q_rows], g2, b2, b[q_rows], qpos).max()))
        W[q_rows] *= c; b[q_rows] *= c; W[k_rows] /= c; b[k_rows] /= c
        pushed = {"cross-attention queries"}
    elif name == "memory pos":            # the function changes: K = (memory + pos) Wk^T + bk, the pos term dominating
        c = TARGET / max(float((pos.double() @ sd["decoder.layers.%d.multihead_attn.in_proj_weight" % i][E:2 * E].double().t())
                               .abs().max()) for i in range(case["model"]["dec"]))
        pos *= c
        pushed = {"cross-attention keys"}
    elif name == "query pos":             # the function changes: yq = LN(x) + qpos of the un-fused steps
        c = TARGET / float(qpos.abs().max())
        qpos *= c
        pushed = {"LayerNorm + query pos", "cross-attention queries"}
    elif name == "ff up, unfolded":       # relu(c h) = c relu(h): linear1 by c, linear2 by 1 / c
        c = CS_SLACK * TARGET / float(_row_bound(sd[p + "linear1.weight"], g3, b3, sd[p + "linear1.bias"]).max())
        sd[p + "linear1.weight"] *= c; sd[p + "linear1.bias"] *= c; sd[p + "linear2.weight"] /= c
        pushed = {"feed-forward hidden"}
    elif name == "self V up, unfolded":   # the attention output is linear in v: v of head 0 by c, out_proj's columns by 1 / c
        Ws, bs = sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"]
        v_rows = slice(2 * E + HEAD.start, 2 * E + HEAD.stop)
        c = CS_SLACK * TARGET / float(_row_bound(Ws[v_rows], g1, b1, bs[v_rows]).max())
        Ws[v_rows] *= c; bs[v_rows] *= c; sd[p + "self_attn.out_proj.weight"][:, HEAD] /= c
        pushed = {"self-attention values"}
    else:
        raise KeyError(name)
    return case, sd, batch, pushed


VARIANTS = ["cross K up", "cross q up", "memory pos", "query pos", "ff up, unfolded", "self V up, unfolded"]


# ---- CPU: the bounds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VARIANTS)
def test_each_variant_pushes_exactly_its_operand_class_past_the_limit(name):
    """The bounds see every variant: the pushed classes reach the limit, the others stay where the unmodified model has them
    (below it) -- so the engine falls back for the right reason, and the shrunk operand stays well above fp16's floor."""
    case, sd, _batch, pushed = make_variant(name)
    m = case["model"]
    got = fp16_operand_bounds(sd, m["dec"], m["E"])
    assert {k for k, v in got.items() if v >= FP16_LIM} == pushed, got


@pytest.mark.parametrize("name", golden_names())
def test_every_golden_is_inside_fp16_range(name):
    """The goldens (and with them bench.py's weight recipes, which they share) keep every bound far below the limit: the package
    default binds fp16x2 on all of them, not the slower bf16x3 fallback."""
    case, _ = load_golden(name)
    sd, _ = case_weights_and_batch(case)
    got = fp16_operand_bounds(sd, case["model"]["dec"], case["model"]["E"])
    assert max(got.values()) < FP16_LIM / 100, got


# ---- GPU: the variants against fp64 truth ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["package default", "f32 MFMA only", "fp16x2 from 1 row"])
@pytest.mark.parametrize("name", VARIANTS)
def test_variant_outside_fp16_range_is_fp32_class_against_fp64_truth(hip_lib, name, form):
    """Every logit finite, within 1 x tol and 4 x the host fp32 reference's error of the fp64 truth teacher-forced along the HIP's
    tokens; an engine bound with planes falls back to bf16x3 with exactly one warning naming the pushed class."""
    from oracle import truth as TR
    from test_parity_golden import TRUTH_FORMS, TRUTH_REF_FACTOR, _e_ref, _tol, _truth_along, run_traced
    case, sd, batch, pushed = make_variant(name)
    model = build_model(case, sd, "cuda")
    for k, v in TRUTH_FORMS[form].items():
        setattr(model, k, v)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            out = run_traced(model, case, batch_to(batch, "cuda"))
    eng = model.engine()
    msgs = [str(x.message) for x in w if "fp16" in str(x.message)]
    if eng.has_planes and eng.requested_kind == "fp16x2":
        assert eng.split_kind == "bf16x3" and len(msgs) == 1, (eng.split_kind, msgs)
        assert all(cls in msgs[0] for cls in pushed), msgs[0]
        assert {k for k, v in eng.fp16_operand_bounds.items() if v >= FP16_LIM} == pushed
    else:
        assert not msgs
    T = case["model"]["seq_len"]
    hip = dict(predict=out["predict"].cpu().numpy().reshape(-1, T), steps=int(out["steps"]), logits=out["logits"].cpu().numpy(),
               best=out["best"].cpu().numpy(), second=out["second"].cpu().numpy())
    assert np.isfinite(hip["logits"][: hip["steps"]][hip["logits"][: hip["steps"]] != TR.FILL32]).all()
    truth, _secs, _peak = _truth_along(case["name"], case, sd, batch, hip)
    tol = np.array([_tol(truth[s]) for s in range(hip["steps"])])
    e_ref = _e_ref(case["name"], case, None, sd, batch, hip, truth)
    first = TR.anchor_column("parallel", batch["num_input"], max(int(n) for n in batch["num_input"]))
    st = TR.check_trace_against_truth(hip, truth, tol, e_ref=e_ref, ref_factor=TRUTH_REF_FACTOR, first_column=first)
    print(name, form, eng.split_kind, st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_gain4", "par_full_n40_gain4", "par_full_n40_default", "par_small_ragged300",
                                  "par_full_B256_default", "par_full_B256_gain4", "par_full_C4x256_gain4", "par_full_E1024_gain4",
                                  "par_small_ragged", "par_small_earlybreak", "par_small_break1", "par_small_extramask"])
def test_cross_attention_bounds_hold_on_the_goldens(hip_lib, name):
    """The engine's bounds are sound where they are exercised: the true max |k| and max |v| of every decoder layer's cross
    attention, from the fp64 oracle's encoder memory, the position table and the weights, lie below the corresponding entries of
    fp16_operand_bounds; the golden binds fp16x2 with no warning."""
    from oracle import refpath
    case, _ = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    model.x3_min_rows, model.split_kind = 1, "fp16x2"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        eng = model.engine()
    assert eng.split_kind == "fp16x2" and not [x for x in w if "fp16" in str(x.message)]
    bounds = eng.fp16_operand_bounds
    assert max(bounds.values()) < FP16_LIM
    sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
    b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v)
           for k, v in batch.items()}
    T, F = case["model"]["seq_len"], max(int(n) for n in batch["num_input"])
    from oracle import truth as TR
    forced = torch.zeros(len(batch["num_input"]) * F, T, dtype=torch.long)
    forced[:, 0] = torch.from_numpy(TR.anchor_column("parallel", batch["num_input"], F))
    tr = {}
    with torch.no_grad():
        refpath.parallel_forward_eval(sd64, b64, num_head=case["model"]["H"], trace=tr, forced=forced.cuda(), steps=1,
                                      seqs=torch.zeros(1, dtype=torch.long, device="cuda"), num_anchors=F)
    mem = tr["memory"]                                            # [N, S, E] fp64
    E, S = case["model"]["E"], mem.shape[1]
    pos = sd64["pos_enc.pos_embed.weight"][:S]
    for i in range(case["model"]["dec"]):
        W = sd64["decoder.layers.%d.multihead_attn.in_proj_weight" % i]
        b = sd64["decoder.layers.%d.multihead_attn.in_proj_bias" % i]
        k = (mem + pos) @ W[E:2 * E].t() + b[E:2 * E]
        v = mem @ W[2 * E:].t() + b[2 * E:]
        assert float(k.abs().max()) <= bounds["cross-attention keys"], (i, float(k.abs().max()), bounds)
        assert float(v.abs().max()) <= bounds["cross-attention values"], (i, float(v.abs().max()), bounds)


# ---- GPU: more than 65535 (wireframe, head) pairs -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [8191, 8193])
def test_decode_of_more_than_65535_head_pairs(hip_lib, N):
    """H = 8: 8191 wireframes are 65528 (wireframe, head) pairs, 8193 are 65544 -- past the 65535 blocks of one launch's grid.y
    that the package default's K | V split used to reject.  Both decode; sampled rows, the last wireframes (pairs past 65535)
    among them, match the fp64 oracle teacher-forced along the HIP's tokens within the step's bar."""
    from faceformer_amd.synth import make_state_dict, make_wireframes, state_dict_spec
    from oracle import refpath
    from oracle import truth as TR
    from test_parity_golden import _tol, run_traced
    L, T = 4, 5
    case = dict(name="wide%d" % N, kind="parallel", model=dict(E=512, H=8, FF=1024, enc=1, dec=1, L=L, seq_len=T))
    sd = make_state_dict(state_dict_spec("parallel", L, T, 512, 1024, 1, 1), "gain4", 5)
    n_edges = [1 + (w % L) for w in range(N)]
    batch = make_wireframes(n_edges, L, T, "parallel", seeds=range(N), num_points=50)
    model = build_model(case, sd, "cuda")
    assert model.split_kind == "fp16x2" and model.x3_min_rows > 0      # the package default
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            out = run_traced(model, case, batch_to(batch, "cuda"))
    assert model.engine().split_kind == "fp16x2" and not [x for x in w if "fp16" in str(x.message)]
    del out["memory"]
    steps = int(out["steps"])
    pred = out["predict"].cpu().reshape(-1, T)
    F = L
    assert pred.shape[0] == N * F
    rows = np.unique(np.concatenate([np.linspace(0, N * F - 1, 48).round().astype(np.int64),
                                     np.arange((N - 2) * F, N * F)]))           # every row of the last two wireframes
    logits = out["logits"][:steps, torch.from_numpy(rows).cuda()].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
    b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v)
           for k, v in batch.items()}
    tr = {}
    with torch.no_grad():
        refpath.parallel_forward_eval(sd64, b64, num_head=8, trace=tr, forced=pred.cuda(), steps=steps,
                                      seqs=torch.from_numpy(rows).cuda(), num_anchors=F)
    truth = torch.stack(tr["logits"], dim=1).cpu().numpy().transpose(1, 0, 2)    # [steps, rows, S]
    first = TR.anchor_column("parallel", batch["num_input"], F)
    assert np.array_equal(pred[:, 0].numpy(), first)
    for s in range(steps):
        masked_h, masked_t = logits[s] == TR.FILL32, truth[s] == TR.FILL64
        assert np.array_equal(masked_h, masked_t), s
        assert np.isfinite(logits[s]).all(), s
        d = np.where(masked_t, 0.0, np.abs(logits[s].astype(np.float64) - truth[s])).max(axis=1)
        tol = _tol(truth[s])
        assert d.max() <= tol, (s, int(rows[int(np.argmax(d))]), float(d.max()), tol)
        assert np.array_equal(np.argmax(logits[s], axis=1), pred[rows, s + 1].numpy()), s
