"""Numpy fp64 restatement of the beam search over the pointer head: one step (`beam_step`), and the whole
rule over a caller-given logit function (`beam_decode`).  Test helper; nothing here is imported by the package."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
LP_BAR = 2.0 ** -16          # the project's log-probability bar
ADD_EPS = 2.0 ** -23         # one fp32 addition


def score_bound(score):
    """|fp32 score - fp64 score| after one step: one log-probability plus one fp32 addition."""
    return LP_BAR + ADD_EPS * abs(float(score))


def mask_logits(logits, mask=None, kv_len=None):
    """select_next's masking of a [rows, S] block of ONE wireframe: masked keys and keys >= kv_len at finfo(float32).min."""
    lg = np.array(logits, dtype=np.float64, copy=True)
    S = lg.shape[-1]
    dead = np.zeros(S, dtype=bool) if mask is None else np.asarray(mask).astype(bool).copy()
    if kv_len is not None:
        dead |= np.arange(S) >= int(kv_len)
    lg[..., dead] = -FLT_MAX
    return lg


def group_step(logits, scores, fin, term_lo, term_hi, ge_bound=None, margin=1):
    """One step of ONE group.  logits [W, S] masked fp64 (rows of empty / finished beams are not read), scores [W] (-inf: empty),
    fin [W] bool.  Returns dict(parent, tok, scores, fin [W each], count, gap): the kept candidates in rank order (a rank past the
    number of candidates: parent = the rank, token 0, score -inf, not finished); count = kept candidates of unfinished beams with
    a token >= ge_bound.  gap: the smallest decisive gap -- between consecutive kept ranks, and between rank W and rank W + 1 --
    divided by twice the larger bound of its two scores (`margin` times score_bound: the steps a caller's fp32 scores have
    accumulated).  gap > 1: fp32 scores inside their bounds select and order as fp64 does; inf when nothing competes.  Two
    candidates saturated at -FLT_MAX are not a gap: they are equal in fp32 too, and the index decides in both."""
    W, S = logits.shape
    scs, ixs = [], []
    for k in range(W):
        if scores[k] == -np.inf:
            continue
        if fin[k]:
            scs.append(np.array([float(scores[k])])); ixs.append(np.array([k * S]))
            continue
        row = logits[k]
        m = row.max()
        lp = (row - m) - np.log(np.exp(row - m).sum())
        scs.append(np.maximum(scores[k] + lp, -FLT_MAX)); ixs.append(k * S + np.arange(S))
    sc_all = np.concatenate(scs) if scs else np.zeros(0)
    ix_all = np.concatenate(ixs) if ixs else np.zeros(0, dtype=np.int64)
    order = np.lexsort((ix_all, -sc_all))[: W + 1]
    cand = [(float(sc_all[i]), int(ix_all[i])) for i in order]
    kept = cand[:W]
    ratio = np.inf
    for i in range(len(cand) - 1):
        a, b = cand[i][0], cand[i + 1][0]
        if a == b == -FLT_MAX:      # both saturated: exactly equal in fp32 as well, the tie rule decides in both
            continue
        ratio = min(ratio, (a - b) / (2.0 * margin * max(score_bound(a), score_bound(b))))
    out = {"parent": np.arange(W), "tok": np.zeros(W, dtype=np.int64), "scores": np.full(W, -np.inf), "fin": np.zeros(W, dtype=bool),
           "count": 0, "gap": ratio}
    for r, (sc, ix) in enumerate(kept):
        k, s = divmod(ix, S)
        out["parent"][r], out["scores"][r] = k, sc
        if fin[k]:
            out["fin"][r] = True
        else:
            out["tok"][r] = s
            out["fin"][r] = term_lo <= s < term_hi
            if ge_bound is not None and s >= ge_bound:
                out["count"] += 1
    return out


def beam_step(logits, scores, fin, W, term_lo, term_hi, ge_bound=None, margin=1):
    """group_step over [G * W, S] logits: arrays of G * W entries, count summed, gap [G]."""
    G = logits.shape[0] // W
    res = [group_step(logits[g * W:(g + 1) * W], scores[g * W:(g + 1) * W], fin[g * W:(g + 1) * W], term_lo, term_hi, ge_bound, margin)
           for g in range(G)]
    out = {k: np.concatenate([r[k] for r in res]) for k in ("parent", "tok", "scores", "fin")}
    out["count"] = sum(r["count"] for r in res)
    out["gap"] = np.array([r["gap"] for r in res])
    return out


def backtrack(start, toks, parents, W):
    """beams [G * W, len(toks) + 1] from the start tokens [G * W] and the per-step tokens / group-local parents [steps][G * W]."""
    B, steps = len(start), len(toks)
    beams = np.zeros((B, steps + 1), dtype=np.int64)
    for b in range(B):
        g, cur = b // W, b % W
        for s in range(steps, 0, -1):
            beams[b, s] = toks[s - 1][g * W + cur]
            cur = int(parents[s - 1][g * W + cur])
        beams[b, 0] = start[g * W + cur]
    return beams


def beam_decode(logit_fn, start, W, T, term_lo, term_hi, ntok):
    """The whole rule for G = len(start) anchors.  logit_fn(prefixes [G * W, j + 1]) -> masked logits [G * W, S] of the next
    step.  Returns (beams [G * W, T], scores [G * W], steps)."""
    G = len(start)
    tok0 = np.repeat(np.asarray(start, dtype=np.int64), W)
    scores = np.where(np.arange(G * W) % W == 0, 0.0, -np.inf)
    fin = (tok0 >= term_lo) & (tok0 < term_hi)
    toks, parents = [], []
    steps = T - 1
    for j in range(1, T):
        prefixes = backtrack(tok0, toks, parents, W)
        res = beam_step(np.asarray(logit_fn(prefixes), dtype=np.float64), scores, fin, W, term_lo, term_hi, ntok)
        toks.append(res["tok"]); parents.append(res["parent"])
        scores, fin = res["scores"], res["fin"]
        if res["count"] == 0:
            steps = j
            break
    beams = np.zeros((G * W, T), dtype=np.int64)
    beams[:, : steps + 1] = backtrack(tok0, toks, parents, W)
    return beams, scores, steps
