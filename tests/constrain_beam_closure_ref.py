"""Numpy fp64 restatement of the closure look-ahead (both forms) in the beam search over the loop-constrained pointer decode
(DESIGN.md 28).  Test helper; nothing here is imported by the package.

It is constrain_beam_ref.group_step with ONE change: the mask of an unfinished, non-empty beam comes from
constrain_sample_ref.rule_mask(form, ...) -- "plain" (constrain_ref's), "ahead" (lookahead_ref's: close_dist[first] while the
beam's loop is open, cycle_len while it is closed, against the step's budget) or "exact" (exact_ref's: one search per open beam
over that beam's own visited set; cycle_len while the loop is closed).  Every beam of a step shares the budget.  The candidates,
the order, the ties, the empty and finished beams and the state update are constrain_beam_ref's, by calling it: the module's
rule_mask is swapped for the duration of the call, nothing of group_step is restated.
"""
import contextlib

import numpy as np

import constrain_beam_ref as CBR
import constrain_ref as CR
import constrain_sample_ref as CSR

FORMS = {"lookahead": "ahead", "exact": "exact"}      # constrain_beam_closure -> constrain_sample_ref's form names
LOOPS = CR.NO_REPEAT | CR.CONNECT
CAP = CBR.CAP
pack_state = CBR.pack_state
start_group = CBR.start_group

# Non-vacuity of the engine tests under "exact" at W = 4 (profiles/constrain_beam_closure/yield.json, written by
# tools/constrain_beam_closure_left_out.py with the fp64 oracle on the CPU): own-anchor groups whose best non-dead beam is enclosed,
# as (groups, plain, "lookahead", "exact").  The GPU test asserts at least half of the oracle's "exact" count, and strictly more
# than the plain constrain_beams count on STRICT.
ORACLE_W4 = {"par_small_gain4": (33, 22, 25, 26), "par_small_ragged": (91, 22, 80, 80), "par_full_n40_gain4": (40, 23, 36, 36)}
STRICT = ("par_small_ragged",)      # (the oracle shows strictly more on all three; the widest margin is asserted)


class _FormRule:
    """constrain_ref's rule_mask signature, answering with the form's mask."""

    def __init__(self, form, close_dist, cycle_len, budget):
        self.form, self.close_dist, self.cycle_len, self.budget = form, close_dist, cycle_len, budget
        self.advance, self.start_state, self.step_row = CR.advance, CR.start_state, CR.step_row

    def rule_mask(self, state, flags, S, ntok, term, follows, pad):
        return CSR.rule_mask(self.form, state, flags, S, ntok, term, follows, pad, self.close_dist, self.cycle_len, self.budget)


@contextlib.contextmanager
def _rule(form, close_dist, cycle_len, budget):
    saved = CBR.cr
    CBR.cr = _FormRule(form, close_dist, cycle_len, budget)
    try:
        yield
    finally:
        CBR.cr = saved


def group_step(form, raw, pad, scores, fin, dead, states, flags, ntok, term, follows, close_dist=None, cycle_len=None, budget=0,
               margin=1):
    """constrain_beam_ref.group_step of ONE group under `form` ("plain", "ahead", "exact"); close_dist [L, L] / cycle_len [L] uint8
    are the group's wireframe's."""
    with _rule(form, close_dist, cycle_len, budget):
        return CBR.group_step(raw, pad, scores, fin, dead, states, flags, ntok, term, follows, margin)


def beam_step(form, raw, pads, scores, fin, dead, states, W, flags, ntok, term, follows_of, group_wireframe, close_dist_of=None,
              cycle_len_of=None, budget=0, margin=1):
    """group_step over [G * W, S] raw logits; *_of(w) -> the wireframe's table.  constrain_beam_ref.beam_step's dict."""
    G = raw.shape[0] // W
    res = []
    for g in range(G):
        sl = slice(g * W, (g + 1) * W)
        w = int(group_wireframe[g])
        res.append(group_step(form, raw[sl], pads[w], scores[sl], fin[sl], dead[sl], states[sl], flags, ntok, term, follows_of(w),
                              None if close_dist_of is None else close_dist_of(w), None if cycle_len_of is None else cycle_len_of(w),
                              budget, margin))
    out = {k: np.concatenate([r[k] for r in res]) for k in ("parent", "tok", "scores", "fin", "dead", "dead_now")}
    for k in ("states", "rows", "masked"):
        out[k] = [x for r in res for x in r[k]]
    out["count"] = sum(r["count"] for r in res)
    out["gap"] = np.array([r["gap"] for r in res])
    return out


def enclosed_best(beams, scores, dead, ntok, term, follows):
    """Of one group's final beams [W, T]: is its best non-empty, non-dead beam a closed face?  (It ends in a terminator and the
    rule's state after its edges is closed: first is None with at least one edge.)"""
    for k in range(beams.shape[0]):
        if np.isinf(scores[k]) or dead[k]:
            continue
        row = [int(t) for t in beams[k]]
        ends = [j for j, t in enumerate(row) if term[0] <= t < term[1]]
        if not ends:
            return False
        st = CR.state_of_prefix(row[: ends[0]], ntok, follows) if ends[0] > 0 else (frozenset(), None, None)
        return st[1] is None and len(st[0]) > 0
    return False
