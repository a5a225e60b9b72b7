"""The closure look-ahead of the sequence-constrained beam search in numpy fp64, and the cases the tests use.

Nothing of the rule, of the search or of the layout is restated.  A group's step is sequence_constrain_beam_ref.group_step -- its
candidates, order, gap and inheritance -- called with faces.sequence_rule_mask bound to the closure keywords of the group's
wireframe and the step's budget (sequence_constrain_closure_ref.closure_kw / budget_of); start, counters, stop and back-tracking
are sequence_beam_ref's and beam_ref's.  What is added: which wireframe's tables and which budget a group's beams are masked
with -- one pair of tables per wireframe, shared by its W beams, and one budget per step.
"""
import functools
import types

import numpy as np

import beam_ref as R
import sequence_beam_ref as QB
import sequence_constrain_beam_ref as CB
import sequence_constrain_closure_ref as QC
from faceformer_amd import faces

FORMS, FORM_ID = QC.FORMS, QC.FORM_ID
FILL, NEG, CAP = CB.FILL, CB.NEG, CB.CAP
LOOPS, COEDGE_LOOPS, FLAGS, FIXTURES, STOPS = CB.LOOPS, CB.COEDGE_LOOPS, CB.FLAGS, CB.FIXTURES, CB.STOPS
budget_of, hmax_of, tables, closure_kw, late_dead_ends = QC.budget_of, QC.hmax_of, QC.tables, QC.closure_kw, QC.late_dead_ends
OPEN_AT_T = QC.OPEN_AT_T


def group_step(raw, pad, scores, fin, states, flags, ntok, sep, eos, follows, margin=1, **closure):
    """sequence_constrain_beam_ref.group_step with every beam's mask under sequence_rule_mask's closure keywords (none: the plain
    step).  The helper reads the rule through its module's `faces`; for the call that name is the rule with the keywords bound."""
    if not closure:
        return CB.group_step(raw, pad, scores, fin, states, flags, ntok, sep, eos, follows, margin)
    bound = types.SimpleNamespace(sequence_rule_mask=functools.partial(faces.sequence_rule_mask, **closure),
                                  sequence_rule_advance=faces.sequence_rule_advance)
    saved, CB.faces = CB.faces, bound
    try:
        return CB.group_step(raw, pad, scores, fin, states, flags, ntok, sep, eos, follows, margin)
    finally:
        CB.faces = saved


def beam_step(raw, pads, scores, fin, states, W, flags, ntok, sep, eos, follows, form, close_dist, cycle_len, budget, margin=1):
    """sequence_constrain_beam_ref.beam_step with group g under wireframe g's tables at `budget`."""
    G = raw.shape[0] // W
    res = [group_step(raw[g * W:(g + 1) * W], pads[g], scores[g * W:(g + 1) * W], fin[g * W:(g + 1) * W], states[g * W:(g + 1) * W],
                      flags, ntok, sep, eos, None if follows is None else follows[g], margin,
                      **closure_kw(form, close_dist, cycle_len, g, budget)) for g in range(G)]
    out = {k: np.concatenate([r[k] for r in res]) for k in ("parent", "tok", "scores", "fin", "dead", "open", "dead_now")}
    for k in ("states", "rows", "masked"):
        out[k] = [x for r in res for x in r[k]]
    out["gap"] = np.array([r["gap"] for r in res])
    out["candidates"] = np.array([r["candidates"] for r in res])
    out["all"], out["best"] = CB.counters(out["scores"], out["fin"], W)
    return out


def decode(step_logits, pads, W, T, flags, ntok, sos, sep, eos, follows, stop="all", form=None, close_dist=None, cycle_len=None):
    """sequence_constrain_beam_ref.decode with step j (which selects position j + 1) under budget_of(T, j + 1)."""
    assert stop in STOPS
    G = len(pads)
    scores, fin = QB.start(G, W)
    states = [faces.sequence_rule_start()] * (G * W)
    opn = np.zeros(G * W, dtype=bool)
    tok0 = np.full(G * W, sos, dtype=np.int64)
    toks, parents, deads, gaps, rows, alls, bests = [], [], [], [], [], [], []
    steps = T - 1
    for j in range(T - 1):
        prefixes = R.backtrack(tok0, toks, parents, W)
        res = beam_step(np.asarray(step_logits(prefixes, j), dtype=np.float64), pads, scores, fin, states, W, flags, ntok, sep, eos,
                        follows, form, close_dist, cycle_len, budget_of(T, j + 1), margin=j + 1)
        toks.append(res["tok"]); parents.append(res["parent"]); deads.append(res["dead"].astype(np.int64)); gaps.append(res["gap"])
        rows.append(res["rows"]); alls.append(res["all"]); bests.append(res["best"])
        scores, fin, states, opn = res["scores"], res["fin"], res["states"], res["open"]
        if (res["all"] if stop == "all" else res["best"]) == 0:
            steps = j + 1
            break
    beams, dead_end = np.zeros((G * W, T), dtype=np.int64), np.zeros((G * W, T), dtype=np.int64)
    beams[:, : steps + 1] = R.backtrack(tok0, toks, parents, W)
    dead_end[:, : steps + 1] = R.backtrack(np.zeros(G * W, dtype=np.int64), deads, parents, W)
    return dict(beams=beams, dead_end=dead_end, scores=scores, fin=fin, open=opn, steps=steps, counts=alls if stop == "all" else bests,
                all_counts=alls, best_counts=bests, parents=parents, toks=toks, deads=deads, gaps=gaps, rows=rows, states=states)


def guarantees(beams, dead, open_end, scores, W, ni, flags, ntok, sep, eos, follows, edges, form):
    """(g1) no non-empty beam ends with a loop open; (g2) under "exact" no non-empty beam holds a late dead end along its own
    back-tracked path; (g3) sequence_constrain_beam_ref.guarantee.  -> (enclosed, parsed, dead ends, late dead ends)."""
    live = np.isfinite(np.asarray(scores, dtype=np.float64))
    assert not np.asarray(open_end)[live].any(), ("g1", np.asarray(open_end).tolist())
    late = [(r, p) for r, p in late_dead_ends(np.asarray(beams), np.asarray(dead), flags, ntok, sep, follows, W) if live[r]]
    if form == "exact":
        assert late == [], ("g2", late)
    enc, par, de = CB.guarantee(beams, dead, open_end, scores, W, ni, flags, ntok, sep, eos, follows, edges)
    return enc, par, de, len(late)


# ---- the operator test's grid ---------------------------------------------------------------------------------------------------------
# S x W (W <= S) x groups x flags {3, 7} x both forms x both stop forms (the issue's); the table kinds and the budgets rotate over
# the cases of a cell so that every kind meets every budget somewhere in the grid.  tools/sequence_constrain_beam_closure_left_out.py
# operator applies the rule in fp64 and in fp32-rounded arithmetic to every case: a seed is kept only if no group is left out.
OP_S, OP_W, OP_G = (5, 65, 260, 1028), (1, 3, 8), (1, 5)
OP_KINDS = ("lattice", "ring", "chain", "random", "trap_a", "trap_b")
OP_BUDGETS = (0, 1, 2, 5, 254)
OP_SEED_OFFSETS = {}      # (S, W, G, once, form, stop) -> offset from the base seed; empty: every base seed left nothing out


def op_cases(S, W):
    """The cases of one (S, W) cell: (G, once, form, stop, kind, budget, seed, hmax).  At S = 1028 the tables with long paths run at
    budget <= 5 with distances built to 8 hops: every entry a budget is compared against is exact, and the searches stay short."""
    out = []
    cell = OP_S.index(S) * len(OP_W) + OP_W.index(W)
    n = cell
    for G in OP_G:
        for once in (False, True):
            for form in FORMS:
                for stop in STOPS:
                    kind = OP_KINDS[n % len(OP_KINDS)]
                    if kind.startswith("trap") and S < 65:
                        kind = "random"
                    budget = OP_BUDGETS[(n // 2 + cell) % len(OP_BUDGETS)]
                    short = S >= 1028 and kind in ("ring", "chain")
                    if short and budget > 5:
                        budget = 5
                    seed = 7 * cell + n + OP_SEED_OFFSETS.get((S, W, G, once, form, stop), 0)
                    out.append((G, once, form, stop, kind, budget, seed, 8 if short else 254))
                    n += 1
    return out


# ---- the engine's replay tuples --------------------------------------------------------------------------------------------------------
# (golden, kind, seed, flags, W, form) -> (left-out pairs, pairs, enclosed faces, parsed faces, dead ends, late dead ends, open ends over
# the non-empty final beams, steps under "all") of the ORACLE's own decode under the form, as
# tools/sequence_constrain_beam_closure_left_out.py engine prints them; a tuple is kept only within CAP.  The GPU decode must
# reproduce the counts of a tuple that leaves nothing out on either side.
REPLAY_W = CB.REPLAY_W
KEPT = {
    ('seq_small_eos', 'lattice', 1, 3, 2, 'exact'): (0, 19, 6, 6, 0, 0, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 1, 3, 2, 'lookahead'): (0, 19, 6, 6, 0, 0, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 1, 3, 4, 'exact'): (0, 19, 12, 12, 0, 0, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 1, 3, 4, 'lookahead'): (0, 19, 12, 12, 0, 0, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 1, 7, 2, 'exact'): (0, 14, 6, 6, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 1, 7, 2, 'lookahead'): (0, 14, 6, 6, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 1, 7, 4, 'exact'): (0, 14, 10, 10, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 1, 7, 4, 'lookahead'): (0, 14, 10, 10, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 2, 3, 2, 'exact'): (0, 19, 5, 5, 0, 0, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 2, 3, 2, 'lookahead'): (0, 19, 5, 5, 0, 0, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 2, 3, 4, 'exact'): (0, 19, 10, 10, 0, 0, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 2, 3, 4, 'lookahead'): (0, 19, 10, 11, 1, 1, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 2, 7, 2, 'exact'): (0, 16, 6, 6, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 2, 7, 2, 'lookahead'): (0, 16, 6, 6, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 2, 7, 4, 'exact'): (0, 16, 9, 9, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 2, 7, 4, 'lookahead'): (0, 16, 9, 9, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 1, 3, 2, 'exact'): (0, 6, 1, 1, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 1, 3, 2, 'lookahead'): (0, 6, 1, 1, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 1, 3, 4, 'exact'): (0, 11, 3, 4, 1, 0, 0, 11),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 1, 3, 4, 'lookahead'): (0, 11, 3, 4, 1, 0, 0, 11),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 1, 7, 2, 'exact'): (0, 6, 1, 1, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 1, 7, 2, 'lookahead'): (0, 6, 1, 1, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 1, 7, 4, 'exact'): (0, 8, 2, 4, 2, 0, 0, 8),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 1, 7, 4, 'lookahead'): (0, 8, 2, 4, 2, 0, 0, 8),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 2, 3, 2, 'exact'): (0, 16, 3, 3, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 2, 3, 2, 'lookahead'): (0, 16, 3, 3, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 2, 3, 4, 'exact'): (0, 16, 8, 8, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 2, 3, 4, 'lookahead'): (0, 16, 8, 8, 0, 0, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 2, 7, 2, 'exact'): (0, 6, 1, 1, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 2, 7, 2, 'lookahead'): (0, 6, 1, 1, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 2, 7, 4, 'exact'): (0, 6, 3, 3, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 2, 7, 4, 'lookahead'): (0, 6, 3, 3, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 3, 2, 'exact'): (0, 58, 16, 16, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 3, 2, 'lookahead'): (0, 58, 16, 16, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 3, 4, 'exact'): (0, 58, 27, 27, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 3, 4, 'lookahead'): (0, 58, 27, 27, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 7, 2, 'exact'): (0, 52, 13, 13, 0, 0, 0, 26),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 7, 2, 'lookahead'): (0, 52, 13, 13, 0, 0, 0, 26),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 7, 4, 'exact'): (0, 52, 28, 28, 0, 0, 0, 26),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 7, 4, 'lookahead'): (0, 52, 28, 28, 0, 0, 0, 26),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 3, 2, 'exact'): (0, 58, 18, 18, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 3, 2, 'lookahead'): (0, 58, 18, 18, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 3, 4, 'exact'): (0, 58, 38, 38, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 3, 4, 'lookahead'): (0, 58, 38, 38, 0, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 7, 2, 'exact'): (0, 50, 13, 13, 0, 0, 0, 25),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 7, 2, 'lookahead'): (0, 50, 13, 13, 0, 0, 0, 25),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 7, 4, 'exact'): (0, 50, 28, 28, 0, 0, 0, 25),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 7, 4, 'lookahead'): (0, 50, 28, 28, 0, 0, 0, 25),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 1, 3, 2, 'exact'): (0, 34, 3, 4, 1, 0, 0, 17),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 1, 3, 2, 'lookahead'): (0, 34, 3, 4, 1, 0, 0, 17),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 1, 3, 4, 'exact'): (0, 34, 8, 10, 2, 0, 0, 17),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 1, 3, 4, 'lookahead'): (0, 34, 8, 10, 2, 0, 0, 17),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 1, 7, 2, 'exact'): (0, 18, 2, 3, 1, 0, 0, 9),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 1, 7, 2, 'lookahead'): (0, 18, 2, 3, 1, 0, 0, 9),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 1, 7, 4, 'exact'): (0, 18, 5, 6, 1, 0, 0, 9),   # decisive fp64 decisions = fp32 decisions: True; finished 7 of 7 non-empty beams
    ('seq_small_gain4', 'random', 1, 7, 4, 'lookahead'): (0, 18, 5, 6, 1, 0, 0, 9),   # decisive fp64 decisions = fp32 decisions: True; finished 7 of 7 non-empty beams
    ('seq_small_gain4', 'random', 2, 3, 2, 'exact'): (0, 58, 3, 8, 5, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 2, 3, 2, 'lookahead'): (0, 58, 3, 8, 5, 4, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 2, 3, 4, 'exact'): (0, 58, 7, 16, 9, 0, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 2, 3, 4, 'lookahead'): (0, 58, 7, 16, 9, 7, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 2, 7, 2, 'exact'): (0, 28, 2, 7, 5, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 2, 7, 2, 'lookahead'): (0, 28, 1, 5, 4, 4, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 2, 7, 4, 'exact'): (0, 28, 4, 15, 11, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 2, 7, 4, 'lookahead'): (0, 30, 4, 12, 8, 8, 0, 15),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 3, 2, 'exact'): (0, 10, 2, 2, 0, 0, 0, 5),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 3, 2, 'lookahead'): (0, 10, 2, 2, 0, 0, 0, 5),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 3, 4, 'exact'): (0, 28, 7, 7, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 3, 4, 'lookahead'): (0, 28, 7, 7, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 7, 2, 'exact'): (0, 10, 2, 2, 0, 0, 0, 5),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 7, 2, 'lookahead'): (0, 10, 2, 2, 0, 0, 0, 5),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 7, 4, 'exact'): (0, 28, 7, 7, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 7, 4, 'lookahead'): (0, 28, 7, 7, 0, 0, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 3, 2, 'exact'): (0, 12, 3, 3, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 3, 2, 'lookahead'): (0, 12, 3, 3, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 3, 4, 'exact'): (0, 22, 10, 10, 0, 0, 0, 11),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 3, 4, 'lookahead'): (0, 22, 10, 10, 0, 0, 0, 11),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 7, 2, 'exact'): (0, 12, 3, 3, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 7, 2, 'lookahead'): (0, 12, 3, 3, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 7, 4, 'exact'): (0, 12, 6, 6, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 7 of 7 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 7, 4, 'lookahead'): (0, 12, 6, 6, 0, 0, 0, 6),   # decisive fp64 decisions = fp32 decisions: True; finished 7 of 7 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 3, 2, 'exact'): (0, 22, 3, 3, 0, 0, 0, 11),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 3 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 3, 2, 'lookahead'): (0, 22, 3, 3, 0, 0, 0, 11),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 3 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 3, 4, 'exact'): (0, 24, 7, 7, 0, 0, 0, 12),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 5 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 3, 4, 'lookahead'): (0, 24, 7, 7, 0, 0, 0, 12),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 5 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 7, 2, 'exact'): (0, 16, 2, 3, 1, 0, 0, 8),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 3 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 7, 2, 'lookahead'): (0, 16, 2, 3, 1, 0, 0, 8),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 3 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 7, 4, 'exact'): (0, 16, 4, 5, 1, 0, 0, 8),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 5 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 7, 4, 'lookahead'): (0, 16, 3, 5, 2, 1, 0, 8),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 5 non-empty beams
}
DROPPED = {}      # none: every tuple tried stayed within the cap
