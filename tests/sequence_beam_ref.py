"""The beam search over the single-sequence decode in numpy fp64: one step is beam_ref.group_step, unchanged (the
device has one copy of the list and its order as well); what is stated here is what differs from the parallel beam decode --
layout, start, finish, the two counters and the two stop rules.  Test helper; nothing here is imported by the package.

  layout   N * W rows; beam k of wireframe w is row w * W + k.  One group is one wireframe.
  start    every row holds SOS at position 0; beam 0 has score 0, the others are empty (-inf, no candidates), none is finished.
  finish   a beam is finished from the first position >= 1 that holds EOS: the terminator range is [EOS, EOS + 1).  SEP and the
           other special tokens do not finish it.  A finished beam contributes one candidate: itself, token 0, score unchanged.
  counters after a step, "all": the non-empty beams that are unfinished; "best": the groups whose rank 0 is non-empty and unfinished.
  stop     after the first step that leaves the rule's counter at 0 (steps = that step + 1), else after T - 1 steps.
           "best" is exact for rank 0: log-probabilities are <= 0 and the list is sorted, so a finished rank 0 re-enters as flat
           index 0 with its score unchanged -- no candidate can pass it or win a tie against it.
"""
import numpy as np

import beam_ref as R

FILL, LP_BAR, ADD_EPS, NEG = -R.FLT_MAX, R.LP_BAR, R.ADD_EPS, -np.inf
CAP = 0.02      # the cap on groups / (step, group) pairs left out as indecisive (constrain_beam_ref.CAP's value)
STOPS = ("all", "best")

# The engine's (golden, W) cases.  The 2 % cap on left-out (step, group) pairs is a CONDITION on the case, not a measurement of
# the engine: tools/sequence_beam_left_out.py forces the fp32 oracle along its own beams on the CPU, and a case is replayed only if
# the oracle alone leaves out less than the cap.  KEPT: (golden, W) -> (left-out pairs, pairs, smallest kept gap in units of twice
# the bound, steps under "all", non-empty beams finished at that stop) of the oracle's own decode, as the tool prints them.
# REPLAY: the cases the replay test uses.  seq_small_gain4 at W = 8 is not replayed: a smallest gap of 3.0 is too close to an fp32
# re-evaluation of the logits.
KEPT = {
    ("seq_small_gain4", 1): (0, 58, 1154.0, 29, 1), ("seq_small_gain4", 2): (0, 58, 238.9, 29, 2),
    ("seq_small_gain4", 4): (0, 58, 41.11, 29, 4), ("seq_small_gain4", 8): (0, 58, 3.035, 29, 6),
    ("seq_small_eos", 1): (0, 2, 165700.0, 2, 1), ("seq_small_eos", 2): (0, 4, 3241.0, 4, 2),
    ("seq_small_eos", 4): (0, 12, 1248.0, 12, 4), ("seq_small_eos", 8): (0, 19, 25.46, 19, 7),
    ("seq_small_repeat_eos", 1): (0, 20, 4165.0, 10, 2), ("seq_small_repeat_eos", 2): (0, 20, 2789.0, 10, 4),
    ("seq_small_repeat_eos", 4): (0, 26, 404.7, 13, 8), ("seq_small_repeat_eos", 8): (0, 26, 15.63, 13, 16),
}
REPLAY = [("seq_small_gain4", 2), ("seq_small_gain4", 4), ("seq_small_eos", 2), ("seq_small_eos", 4), ("seq_small_eos", 8),
          ("seq_small_repeat_eos", 2), ("seq_small_repeat_eos", 4), ("seq_small_repeat_eos", 8)]

# The operator test's cases: (S, W, groups, state) -> the seed of operator_case.  Kept by tools/sequence_beam_left_out.py: the
# first seed from op_seed_base() on at which the rule, applied in fp32-rounded and in fp64 arithmetic on the CPU, leaves out less
# than CAP of the case's groups (every kept seed below leaves out none).
OP_S, OP_W, OP_G = (5, 65, 260), (1, 3, 8), (1, 5)
OP_STATES = ("start", "mixed", "done", "eos", "sep")
OP_SEED_OFFSETS = {}      # (S, W, groups, state) -> offset from op_seed_base; none: every case kept its base seed


def op_seed_base(S, W, G, state):
    return 100000 * OP_STATES.index(state) + 100 * S + 10 * W + G


def op_seed(S, W, G, state):
    return op_seed_base(S, W, G, state) + OP_SEED_OFFSETS.get((S, W, G, state), 0)


def operator_case(S, W, G, state, seed, sep=2, eos=3, ntok=4):
    """fp32-exact operands of one launch of G groups (= wireframes) of W beams: logits = 21-bit integers * 2^-17 (|l| < 8), scores
    distinct multiples of 2^-10, a key-padding mask per wireframe (special tokens never masked) and different kv_len.  state:
    "start" beam 0 alone (score 0); "mixed" finished / unfinished / empty beams; "done" every beam finished or empty; "eos" / "sep"
    every beam unfinished and pushed onto EOS / SEP by a logit of 1e4."""
    g = np.random.RandomState(seed)
    B = G * W
    logits = g.randint(-2 ** 20, 2 ** 20, size=(B, S)).astype(np.float64) * 2.0 ** -17
    scores = -(g.permutation(2 ** 13)[:B]).astype(np.float64) * 2.0 ** -10
    fin = np.zeros(B, dtype=bool)
    mask = g.rand(G, S) < 0.2
    mask[:, :ntok] = False
    kv = np.array([S - (w % 2) for w in range(G)], dtype=np.int32)      # S, S - 1, S, ...: neighbours differ (S >= 5)
    empty = g.rand(B) < 0.15
    some_fin = g.rand(B) < 0.3
    if state == "start":
        scores = np.where(np.arange(B) % W == 0, 0.0, NEG)
    elif state == "mixed":
        scores[empty] = NEG
        fin = some_fin
    elif state == "done":
        scores[empty] = NEG
        fin[:] = True
    elif state == "eos":
        logits[:, eos] = 1.0e4
    elif state == "sep":
        logits[:, sep] = 1.0e4
    else:
        raise ValueError(state)
    return dict(S=S, W=W, G=G, state=state, logits=logits, scores=scores, fin=fin, mask=mask, kv=kv)


def masked_of(c):
    W = c["W"]
    return np.concatenate([R.mask_logits(c["logits"][g * W:(g + 1) * W], c["mask"][g], c["kv"][g]) for g in range(c["G"])])


def start(G, W):
    """(scores [G * W], fin [G * W]) of the start state."""
    return np.where(np.arange(G * W) % W == 0, 0.0, NEG), np.zeros(G * W, dtype=bool)


def counters(scores, fin, W):
    """(all, best) from the state AFTER a step: the non-empty unfinished beams; the groups whose rank 0 is non-empty and unfinished."""
    live = np.isfinite(np.asarray(scores, dtype=np.float64)) & ~np.asarray(fin, dtype=bool)
    return int(live.sum()), int(live.reshape(-1, W)[:, 0].sum())


def step(masked, scores, fin, W, eos, margin=1):
    """beam_ref.beam_step over [G * W, S] masked fp64 logits with the terminator range [eos, eos + 1), plus the two counters:
    dict(parent, tok, scores, fin [G * W each], gap [G], all, best)."""
    out = R.beam_step(np.asarray(masked, dtype=np.float64), scores, fin, W, eos, eos + 1, None, margin)
    out["all"], out["best"] = counters(out["scores"], out["fin"], W)
    return out


def step_fp32(masked, scores, fin, W, eos):
    """The step in fp32-ROUNDED arithmetic (every operation rounded to fp32; numpy's exp / log, not the device's): (parent, tok)
    [G * W each].  The left-out tool's second opinion on a seed: a group where this and the fp64 rule select differently is one an
    fp32 kernel may legitimately decide either way."""
    f = np.float32
    B, S = masked.shape
    par, tok = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for g in range(B // W):
        cand = []
        for k in range(W):
            b = g * W + k
            if scores[b] == NEG:
                continue
            if fin[b]:
                cand.append((-float(f(scores[b])), k * S))
                continue
            row = masked[b].astype(f)
            d = row - row.max()
            logz = np.log(np.exp(d).sum(dtype=f), dtype=f)
            sc = np.maximum(f(scores[b]) + (d - logz), f(FILL))
            cand.extend((-float(v), k * S + s) for s, v in enumerate(sc))
        cand.sort()
        for r in range(W):
            if r < len(cand):
                k, s = divmod(cand[r][1], S)
                par[g * W + r], tok[g * W + r] = k, 0 if fin[g * W + k] else s
            else:
                par[g * W + r] = r
    return par, tok


def finish_of(tokens, eos):
    """Finish position of every row of tokens [rows, T]: the first position >= 1 holding eos; T when there is none."""
    tokens = np.asarray(tokens)
    hit = tokens[:, 1:] == eos
    return np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, tokens.shape[1])


def stop_step(counts, T):
    """steps of a decode from its per-step counters: s + 1 for the first step s that leaves 0, else T - 1."""
    for s, v in enumerate(list(counts)[: T - 1]):
        if v == 0:
            return s + 1
    return T - 1


def decode(step_logits, G, W, T, sos, eos, stop="all"):
    """The whole rule as a loop.  step_logits(prefixes [G * W, j + 1], step j) -> masked logits [G * W, S] (rows of empty and
    finished beams are not read).  Returns dict(beams [G * W, T] (zero past each beam's EOS and past steps), scores, fin, steps,
    counts (of `stop`, one per executed step), all_counts, best_counts, parents, toks, gaps [steps][G] (margin = step + 1))."""
    assert stop in STOPS
    scores, fin = start(G, W)
    tok0 = np.full(G * W, sos, dtype=np.int64)
    toks, parents, gaps, alls, bests = [], [], [], [], []
    steps = T - 1
    for j in range(T - 1):
        prefixes = R.backtrack(tok0, toks, parents, W)
        res = step(step_logits(prefixes, j), scores, fin, W, eos, margin=j + 1)
        toks.append(res["tok"]); parents.append(res["parent"]); gaps.append(res["gap"])
        alls.append(res["all"]); bests.append(res["best"])
        scores, fin = res["scores"], res["fin"]
        if (res["all"] if stop == "all" else res["best"]) == 0:
            steps = j + 1
            break
    beams = np.zeros((G * W, T), dtype=np.int64)
    beams[:, : steps + 1] = R.backtrack(tok0, toks, parents, W)
    return dict(beams=beams, scores=scores, fin=fin, steps=steps, counts=alls if stop == "all" else bests, all_counts=alls,
                best_counts=bests, parents=parents, toks=toks, gaps=gaps)
