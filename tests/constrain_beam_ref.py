"""Numpy fp64 restatement of the beam search over the loop-constrained pointer decode, composed from beam_ref (the
order, the gaps, the back-tracking) and constrain_ref (the rule's mask and state).  Test helper; nothing here is imported by the
package.

Per step and group: an empty beam (score -inf) contributes nothing, a finished one itself (token 0, score unchanged); an
unfinished beam k forms its constrained row as constrain_ref.step_row does and contributes its LIVE keys (row > FILL) at c_k +
log_softmax(constrained row), or -- with no live key at all -- token 0 at c_k - log S.  Higher score first, then the lower flat
index k * S + s.  New beam i with parent p and token tk: state = advance(state[p], tk); dead = dead[p] | p dead-ended now; fin =
fin[p] | p dead-ended now | tk is a terminator.  A rank past the number of candidates: parent = the rank, token 0, score -inf,
flags clear, the state of its own index.
"""
import numpy as np

import beam_ref
import constrain_ref as cr

FLT_MAX = beam_ref.FLT_MAX
FILL = cr.FILL
CAP = 0.02      # the cap on (group) cases / (step, group) pairs left out as indecisive


def start_group(tok0, W, ntok, term, follows=None):
    """Start state of one group from its start token: (scores [W], fin [W], dead [W], states [W])."""
    scores = np.where(np.arange(W) == 0, 0.0, -np.inf)
    fin = np.full(W, term[0] <= int(tok0) < term[1])
    st = cr.start_state(int(tok0), ntok, follows)
    return scores, fin, np.zeros(W, dtype=bool), [st] * W


def group_step(raw, pad, scores, fin, dead, states, flags, ntok, term, follows, margin=1):
    """One step of ONE group on RAW logits [W, S] (rows of empty / finished beams are not read); pad [S] bool: the keys masked by
    padding / kv_len.  Returns dict(parent, tok, scores, fin, dead [W each], states [W], rows [W]: the constrained masked fp64 row
    of every non-empty unfinished beam (None otherwise), masked [W]: the rule's own mask (None likewise), dead_now [W] (of the OLD
    beams), count, gap: beam_ref.group_step's)."""
    W, S = raw.shape
    lo, hi = term
    scs, ixs = [], []
    rows, masks, dead_now = [None] * W, [None] * W, np.zeros(W, dtype=bool)
    for k in range(W):
        if scores[k] == -np.inf:
            continue
        if fin[k]:
            scs.append(np.array([float(scores[k])])); ixs.append(np.array([k * S]))
            continue
        masked, dn = cr.rule_mask(states[k], flags, S, ntok, term, follows, pad)
        row = np.where(masked | pad, FILL, np.asarray(raw[k], dtype=np.float64))
        rows[k], masks[k], dead_now[k] = row, masked, dn
        m = row.max()
        lp = (row - m) - np.log(np.exp(row - m).sum())
        live = row > FILL
        if not live.any():
            scs.append(np.array([max(scores[k] - np.log(S), -FLT_MAX)])); ixs.append(np.array([k * S]))
            continue
        scs.append(np.maximum(scores[k] + lp[live], -FLT_MAX)); ixs.append(k * S + np.nonzero(live)[0])
    sc_all = np.concatenate(scs) if scs else np.zeros(0)
    ix_all = np.concatenate(ixs) if ixs else np.zeros(0, dtype=np.int64)
    order = np.lexsort((ix_all, -sc_all))[: W + 1]
    cand = [(float(sc_all[i]), int(ix_all[i])) for i in order]
    ratio = np.inf
    for i in range(len(cand) - 1):
        a, b = cand[i][0], cand[i + 1][0]
        if a == b == -FLT_MAX:
            continue
        ratio = min(ratio, (a - b) / (2.0 * margin * max(beam_ref.score_bound(a), beam_ref.score_bound(b))))
    out = {"parent": np.arange(W), "tok": np.zeros(W, dtype=np.int64), "scores": np.full(W, -np.inf), "fin": np.zeros(W, dtype=bool),
           "dead": np.zeros(W, dtype=bool), "states": list(states), "rows": rows, "masked": masks, "dead_now": dead_now, "count": 0,
           "gap": ratio}
    for r, (sc, ix) in enumerate(cand[:W]):
        k, s = divmod(ix, S)
        out["parent"][r], out["scores"][r] = k, sc
        out["states"][r] = states[k]
        if fin[k]:
            out["fin"][r], out["dead"][r] = True, dead[k]
            continue
        out["tok"][r] = s
        out["fin"][r] = bool(dead_now[k]) or lo <= s < hi
        out["dead"][r] = bool(dead[k]) or bool(dead_now[k])
        out["states"][r] = cr.advance(states[k], s, ntok, follows)
        if s >= ntok:
            out["count"] += 1
    return out


def beam_step(raw, pads, scores, fin, dead, states, W, flags, ntok, term, follows_of, group_wireframe, margin=1):
    """group_step over [G * W, S] raw logits.  pads [wireframes, S] bool, follows_of(w) -> the wireframe's table (or None),
    group_wireframe [G].  Arrays of G * W entries (states, rows, masked: lists), count summed, gap [G]."""
    G = raw.shape[0] // W
    res = []
    for g in range(G):
        sl = slice(g * W, (g + 1) * W)
        w = int(group_wireframe[g])
        res.append(group_step(raw[sl], pads[w], scores[sl], fin[sl], dead[sl], states[sl], flags, ntok, term, follows_of(w), margin))
    out = {k: np.concatenate([r[k] for r in res]) for k in ("parent", "tok", "scores", "fin", "dead", "dead_now")}
    for k in ("states", "rows", "masked"):
        out[k] = [x for r in res for x in r[k]]
    out["count"] = sum(r["count"] for r in res)
    out["gap"] = np.array([r["gap"] for r in res])
    return out


def greedy_row(raw, pad, state, flags, ntok, term, follows):
    """constrain_ref's greedy rule on one row, in this module's terms: (tok, logprob, fin, dead, state)."""
    r = cr.step_row(raw, pad, state, flags, ntok, term, follows)
    return r["tok"], r["logprob"], r["fin"], r["dead"], r["state"]


def pack_state(states, L):
    """(first [B] int32, prev [B] int32, visited [B, ceil(L/32)] int32 words) of a list of states."""
    fw = (L + 31) // 32
    first = np.array([-1 if s[1] is None else s[1] for s in states], dtype=np.int32)
    prev = np.array([-1 if s[2] is None else s[2] for s in states], dtype=np.int32)
    vis = np.zeros((len(states), fw), dtype=np.uint32)
    for b, s in enumerate(states):
        for e in s[0]:
            vis[b, e >> 5] |= np.uint32(1 << (e & 31))
    return first, prev, vis.view(np.int32)
