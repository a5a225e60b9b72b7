"""Sampling over the loop-constrained pointer decode in numpy, composed from the existing references: the byte row
is constrain_ref's / lookahead_ref's / exact_ref's rule_mask, the state update constrain_ref.advance, the draw sample_ref.sample_row
with its guard band and its `decisive` flag.  Nothing of either rule is restated here.

One step of one unfinished sequence: masked, dead = the form's rule_mask of the sequence's own state; l = the logit row with the
padded and the masked keys at -FLT_MAX; the token is sample_row(l, u, tau, K, P)'s, its log-probability sample_row's (under l:
the model's distribution renormalised over the keys the rule allows); the sequence is finished by a terminator or by the dead end.
"""
import numpy as np

import constrain_ref as CR
import exact_ref as XR
import lookahead_ref as LR
import sample_ref as SR

FORMS = ("plain", "ahead", "exact")
LOOPS = CR.NO_REPEAT | CR.CONNECT
REPLAY_R = 4                 # draws per anchor of the engine tests

# (golden, form) -> (uniform seed, parameter sets) kept by tools/constrain_sample_left_out.py on the lattice of
# constrain_ref.LATTICE_SEEDS: the fp32 oracle alone, forced along its own constrained sampled paths, leaves out less than
# sample_ref.CAP of the pairs.  GUARANTEE: the form each golden's guarantee test runs under -- the first form, in the order plain,
# ahead, exact, under which the oracle alone encloses at least twice constrain_ref.MIN_ENCLOSED of the own-anchor draws at tau = 1.
# DESIGN.md 26 lists the shares and what was dropped.
REPLAY_SEED = 5
REPLAY_PARAMS = [(1.0, 0, 1.0), (0.8, 16, 0.9)]
GUARANTEE = {"par_small_gain4": "plain", "par_small_ragged": "plain", "par_full_n40_gain4": "plain"}


def rule_mask(form, state, flags, S, ntok, term, follows, pad, close_dist=None, cycle_len=None, budget=0):
    """The form's rule_mask.  -> (masked [S] bool: the keys the RULE masks, dead_end)."""
    if form == "plain":
        return CR.rule_mask(state, flags, S, ntok, term, follows, pad)
    if form == "ahead":
        return LR.rule_mask(state, flags, S, ntok, term, follows, pad, close_dist, cycle_len, budget)
    if form == "exact":
        assert flags == LOOPS
        return XR.rule_mask(state, S, ntok, term, follows, pad, cycle_len, budget)
    raise ValueError(form)


def masked_row(raw, pad, masked):
    return np.where(masked | pad, CR.FILL, np.asarray(raw, dtype=np.float64))


def step_row(form, raw, pad, state, flags, ntok, term, follows, u, tau=1.0, K=0, P=1.0, finished=False, close_dist=None, cycle_len=None,
             budget=0):
    """One row of one step on RAW logits.  -> dict(tok, logprob, row (masked fp64), masked (the rule's own), dead, fin, state,
    decisive, kept_k)."""
    S = len(raw)
    if finished:
        return dict(tok=0, logprob=0.0, row=np.asarray(raw, dtype=np.float64), masked=np.zeros(S, bool), dead=False, fin=True,
                    state=state, decisive=True, kept_k=np.zeros(S, bool))
    masked, dead = rule_mask(form, state, flags, S, ntok, term, follows, pad, close_dist, cycle_len, budget)
    return draw_row(masked_row(raw, pad, masked), masked, dead, state, ntok, term, follows, u, tau, K, P)


def draw_row(row, masked, dead, state, ntok, term, follows, u, tau=1.0, K=0, P=1.0):
    """The draw and the state update on a MASKED row (a test hands the kernel's own masked logits in)."""
    r = SR.sample_row(row, u, tau, K, P)
    tok = r["tok"]
    fin = bool(dead) or term[0] <= tok < term[1]
    return dict(tok=tok, logprob=r["logprob"], row=row, masked=masked, dead=bool(dead), fin=fin,
                state=CR.advance(state, tok, ntok, follows), decisive=r["decisive"], kept_k=r["kept_k"])


def visited_words(visited, L):
    """The uint32 words (as int32) of a visited set."""
    fw = (L + 31) // 32
    w = np.zeros(max(fw, 0), dtype=np.uint32)
    for e in visited:
        w[e >> 5] |= np.uint32(1) << np.uint32(e & 31)
    return w.view(np.int32)


def none_to(x):
    return -1 if x is None else int(x)
