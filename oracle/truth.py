"""ORACLE TOOLING (tests only): check a traced HIP decode against fp64 truth logits evaluated along the HIP's own tokens.

`oracle/refpath.py` run in float64 with `forced=<the HIP predict>` gives, for every sequence and every executed step, the
exact-arithmetic logits of the prefix the HIP decoded.  Nothing depends on a stored golden row or on the reference having
taken the same branch, so every logit of every row can be held to a bar -- a row-local error (a sequence in the wrong
tile row, a stale KV-cache row, a wrong appended row) cannot hide behind the token checks.

`check_trace_against_truth` raises AssertionError with the failing (step, row) and returns the worst errors.
"""
import numpy as np

FILL32 = np.finfo(np.float32).min   # the HIP's (and the fp32 reference's) masked logit
FILL64 = np.finfo(np.float64).min   # the fp64 oracle's


def stop_steps(predict, kind, num_token=4, tok_eos=3):
    """Steps the reference's stop rule executes on the token path `predict` [B, T] (column 0: anchors / SOS).
    parallel (model_para.py:236-237): stop after the first step whose tokens are all special (< num_token);
    seq2seq (model.py:206-210): stop once the cumulative EOS count (repeats included) reaches the batch size."""
    B, T = predict.shape
    eos_found = 0
    for s in range(T - 1):
        nxt = predict[:, s + 1]
        if kind == "parallel":
            if (nxt < num_token).all():
                return s + 1
        else:
            eos_found += int((nxt == tok_eos).sum())
            if eos_found == B:
                return s + 1
    return T - 1


def anchor_column(kind, num_input=None, F=None, num_token=4, tok_sos=1, B=None):
    """Column 0 of `predict` the reference starts from: per wireframe arange(F) with the anchors past its edge count replaced by
    num_token - 1 (model_para.py:198-200), or SOS for every wireframe of the single-sequence model."""
    if kind != "parallel":
        return np.full(B, tok_sos, dtype=np.int64)
    col = np.tile(np.arange(F, dtype=np.int64), len(num_input)).reshape(len(num_input), F)
    for i, n in enumerate(num_input):
        col[i, int(n):] = num_token - 1
    return col.reshape(-1)


def top2(x):
    """(argmax with the lowest index on ties, largest, second largest -- equal to the largest on a tie) of every row."""
    srt = np.sort(x, axis=-1)
    return np.argmax(x, axis=-1), srt[..., -1], srt[..., -2]


def check_trace_against_truth(hip, truth, tol, kind="parallel", num_token=4, tok_eos=3, e_ref=None, ref_factor=None,
                              ref_floor=1e-6, first_column=None, row_exceptions=None):
    """hip: dict of numpy arrays from a traced decode -- logits [>= steps, B, S] float32, best / second [>= steps, B],
    predict [B, T] int, steps int.  truth: [steps, B, S] float64 logits along hip['predict'].  tol: [steps] bar of every step
    (|hip - truth| <= tol[s] on every live logit).  e_ref / ref_factor: optional fp32-class bar
    |hip - truth| <= ref_factor * e_ref[s] + ref_floor * scale_s (scale_s = max |truth| of the step's live logits);
    steps with e_ref[s] = NaN are not held to it.  first_column: the expected predict[:, 0] (`anchor_column`): the truth is
    forced along the HIP's own column 0, so a wrong anchor would otherwise go unseen.  row_exceptions: {row: (tol multiple,
    ref_factor)} for single named rows; every other row is held to tol and ref_factor.

    Checks, on every row at every executed step: the masked positions are the same; the HIP logits are finite; the bars;
    predict[:, s + 1] is the argmax of the HIP logits (lowest index on ties) and best / second their top two; the HIP
    token equals the truth's argmax wherever the truth's own top-2 margin exceeds 2 tol; and steps is the stop rule
    evaluated on the HIP tokens, with zero padding after it."""
    steps = int(hip["steps"])
    pred = np.asarray(hip["predict"])
    pred = pred.reshape(-1, pred.shape[-1])
    B, T = pred.shape
    want = stop_steps(pred, kind, num_token, tok_eos)
    assert steps == want, "steps = %d, the stop rule on the HIP tokens gives %d" % (steps, want)
    assert (pred[:, steps + 1:] == 0).all(), "predict is not zero after the stop step"
    if first_column is not None:
        bad = np.where(pred[:, 0] != np.asarray(first_column))[0]
        assert bad.size == 0, "row %d starts from %d, the reference from %d" % (bad[0], pred[bad[0], 0], first_column[bad[0]])
    truth = np.asarray(truth, dtype=np.float64)
    assert truth.shape[:2] == (steps, B), "truth has shape %s for %d steps x %d rows" % (truth.shape, steps, B)
    logits = np.asarray(hip["logits"])[:steps]
    assert logits.shape == truth.shape, "HIP logits %s, truth %s" % (logits.shape, truth.shape)
    best, second = np.asarray(hip["best"])[:steps], np.asarray(hip["second"])[:steps]
    tol = np.asarray(tol, dtype=np.float64)

    masked_h, masked_t = logits == FILL32, truth == FILL64
    bad = masked_h != masked_t
    if bad.any():
        s, b, k = np.argwhere(bad)[0]
        raise AssertionError("mask differs at step %d row %d key %d (HIP %s, truth %s)" % (s, b, k, logits[s, b, k], truth[s, b, k]))
    bad = ~np.isfinite(logits)
    if bad.any():
        s, b, k = np.argwhere(bad)[0]
        raise AssertionError("non-finite HIP logit at step %d row %d key %d: %s" % (s, b, k, logits[s, b, k]))
    assert np.isfinite(truth).all(), "non-finite truth logit"

    st = dict(worst_over_tol=0.0, worst_at=(0, 0), worst_over_ref=0.0, worst_ref_at=(0, 0), tokens_checked=0,
              tokens_skipped=0)
    tol_mult, factor = np.ones(B), np.full(B, np.nan if ref_factor is None else float(ref_factor))
    for row, (m, f) in (row_exceptions or {}).items():
        tol_mult[row], factor[row] = m, f
    for s in range(steps):
        live = ~masked_t[s]
        d = np.where(live, np.abs(logits[s].astype(np.float64) - truth[s]), 0.0).max(axis=1)     # [B]
        b = int(np.argmax(d))
        if d[b] / tol[s] > st["worst_over_tol"]:
            st["worst_over_tol"], st["worst_at"] = float(d[b] / tol[s]), (s, b)
        over = np.where(d > tol[s] * tol_mult)[0]
        if over.size:
            b = int(over[np.argmax(d[over] / tol_mult[over])])
            raise AssertionError("bar (a): step %d row %d: |hip - truth| = %.4g > %g x tol %.4g" % (s, b, d[b], tol_mult[b], tol[s]))
        if e_ref is not None and np.isfinite(e_ref[s]):
            scale = np.abs(np.where(live, truth[s], 0.0)).max()
            bound = factor * e_ref[s] + ref_floor * scale
            b = int(np.argmax(d))
            r = d[b] / max(e_ref[s], 1e-300)
            if r > st["worst_over_ref"]:
                st["worst_over_ref"], st["worst_ref_at"] = float(r), (s, b)
            over = np.where(d > bound)[0]
            if over.size:
                b = int(over[np.argmax(d[over] - bound[over])])
                raise AssertionError("bar (b): step %d row %d: |hip - truth| = %.4g > %g x e_ref %.4g + %g x scale %.4g"
                                     % (s, b, d[b], factor[b], e_ref[s], ref_floor, scale))
        # the HIP's own selection
        arg, b1, b2 = top2(logits[s])
        bad = np.where(arg != pred[:, s + 1])[0]
        assert bad.size == 0, "step %d row %d: predict %d is not the argmax %d of the HIP logits" % (
            s, bad[0], pred[bad[0], s + 1], arg[bad[0]])
        bad = np.where((best[s] != b1) | (second[s] != b2))[0]
        assert bad.size == 0, "step %d row %d: best / second %r / %r, the HIP logits' top two %r / %r" % (
            s, bad[0], best[s, bad[0]], second[s, bad[0]], b1[bad[0]], b2[bad[0]])
        # the truth's selection wherever it is decisive
        targ, t1, t2 = top2(truth[s])
        must = (t1 - t2) > 2 * tol[s]
        bad = np.where(must & (targ != pred[:, s + 1]))[0]
        assert bad.size == 0, "step %d row %d: HIP token %d, truth's argmax %d at margin %.4g > 2 tol" % (
            s, bad[0], pred[bad[0], s + 1], targ[bad[0]], (t1 - t2)[bad[0]])
        st["tokens_checked"] += int(must.sum())
        st["tokens_skipped"] += int((~must).sum())
    return st
