"""The closure look-ahead of the loop-constrained single-sequence decode as a numpy loop, its traps and the tuples
the engine tests use.

Nothing of the rule is stated here: one step is faces.sequence_rule_step / sequence_rule_sample_step with their closure keywords
(built on faces.follow_distance and faces.closure_distance), the decode around it is sequence_constrain_ref's (start, finish, stop,
layout), the tables and the exhaustive search are lookahead_ref's and exact_ref's, the replay parameters sample_ref's.  What is
added: the budget of a step, min(T - 1 - position, 254), and the bookkeeping of the guarantees.
"""
import numpy as np

import exact_ref as XR
import lookahead_ref as LR
import sample_ref as SR
import sequence_constrain_ref as SC
from faceformer_amd import faces

FORMS = ("lookahead", "exact")
FORM_ID = {"lookahead": 1, "exact": 2}
FILL, EPS, LP_BAR, CAP = SC.FILL, SC.EPS, SC.LP_BAR, SC.CAP
LOOPS, COEDGE_LOOPS = SC.LOOPS, SC.COEDGE_LOOPS
FIXTURES, FLAGS = SC.FIXTURES, SC.FLAGS
REPLAY_PARAMS = SR.REPLAY_PARAMS
ring, chain, self_closing, can_close = LR.ring, LR.chain, XR.self_closing, XR.can_close

# Trap A (exact_ref's): edges 0 -> 1, 1 -> 2, 1 -> 3, 2 -> 0, 3 -> 1.  With visited = {0, 1}, first = 0, prev = 1 the plain rule
# leaves edges 2 and 3 live and 3 is a dead end one step later; close_dist[0] = [3, 2, 1, 3] keeps 3 at budget >= 3; no path from 3
# avoids the visited edge 1, so the exact form masks it at every budget.
TRAP_A = XR.TRAP_EDGES
# Trap B (the ONCE interplay): 0 -> 1, 1 -> 2, 2 -> 0, 1 -> 3, 3 -> 4, 4 -> 0.  first = 0, prev = 1: edge 3 closes through 4 only.
# With 4 among the visited edges (an earlier face's, kept under ONCE) D_V(3 -> 0) = 255; with visited = {0, 1} it is 2.  The static
# close_dist[0][3] = 2 cannot tell the two states apart.
TRAP_B = ((0, 1), (1, 2), (2, 0), (1, 3), (3, 4), (4, 0))


def table_of(pairs, L=None):
    L = 1 + max(max(p) for p in pairs) if L is None else L
    t = np.zeros((L, L), dtype=bool)
    for a, b in pairs:
        t[a, b] = True
    return t


def budget_of(T, position):
    """The budget of the step that selects `position`."""
    return min(T - 1 - position, 254)


def hmax_of(T):
    """What the model builds the tables with."""
    return min(max(T - 2, 1), 254)


def tables(follows, T, num_input=None):
    """(close_dist [N, L, L], cycle_len [N, L]) uint8 of a batch's tables, as the model builds them."""
    return faces.follow_distance(np.asarray(follows, dtype=bool), hmax_of(T), num_input)


def closure_kw(form, close_dist, cycle_len, w, budget):
    """sequence_rule_*'s closure keywords of wireframe w at `budget` (form None: none)."""
    if form is None:
        return {}
    return dict(closure=form, budget=int(budget), close_dist=None if form == "exact" else close_dist[w], cycle_len=cycle_len[w])


def decode(step_logits, N, T, flags, ntok, sos, sep, eos, follows, form=None, close_dist=None, cycle_len=None, draw=None, G=1):
    """sequence_constrain_ref.decode under a closure form, greedy or (draw = (uniforms [T-1, N*G], temperature, top_k, top_p))
    sampled with G rows per wireframe: row r belongs to wireframe r // G.  step_logits(paths [N*G, T], step) -> masked logits
    [N*G, S].  Returns sequence_constrain_ref.decode's dict."""
    B = N * G
    tok = np.zeros((B, T), dtype=np.int64)
    lp = np.zeros((B, T))
    dead = np.zeros((B, T), dtype=np.int32)
    tok[:, 0] = sos
    state = [faces.sequence_rule_start() for _ in range(B)]
    fin = np.zeros(B, dtype=bool)
    rows = None
    steps = T - 1
    for s in range(T - 1):
        lg = np.asarray(step_logits(tok, s), dtype=np.float64)
        if rows is None:
            rows = np.full((max(T - 1, 1),) + lg.shape, np.nan)
        for r in np.flatnonzero(~fin):
            w = r // G
            kw = closure_kw(form, close_dist, cycle_len, w, budget_of(T, s + 1))
            args = (lg[r], lg[r] <= FILL, state[r], flags, ntok, sep, eos)
            if draw is None:
                res = faces.sequence_rule_step(*args, None if follows is None else follows[w], **kw)
            else:
                res = faces.sequence_rule_sample_step(*args, draw[0][s, r], draw[1], draw[2], draw[3], None if follows is None else follows[w],
                                                      **kw)
            tok[r, s + 1], lp[r, s + 1], dead[r, s + 1], state[r], fin[r] = res["tok"], res["logprob"], res["dead"], res["state"], res["fin"]
            rows[s, r] = res["row"]
        if fin.all():
            steps = s + 1
            break
    return dict(tokens=tok, logprob=lp, dead=dead, open_end=np.array([int(st[1] is not None) for st in state]), steps=steps, rows=rows)


def late_dead_ends(tokens, dead, flags, ntok, sep, follows, G=1):
    """The (row, position) pairs of dead ends that are LATE: raised at a position whose previous position did not open the current
    loop -- the state is replayed from the tokens; a dead end at p is early when the loop was closed after position p - 2 and
    position p - 1 holds the edge that opened it."""
    late = []
    for r in range(tokens.shape[0]):
        at = np.flatnonzero(dead[r])
        if not at.size:
            continue
        st = SC.replay_states(tokens[r:r + 1], flags, ntok, sep, None if follows is None else follows[r // G:r // G + 1])[0]
        for p in at:
            opened = p >= 2 and st[p - 2][1] is None and tokens[r, p - 1] >= ntok and st[p - 1][1] is not None
            if not opened:
                late.append((int(r), int(p)))
    return late


def walk_states(table, rng, flags, ntok, sep, eos, steps, p_sep=0.25):
    """The states of a random walk of the plain rule on `table` from the start state: a random live key per step (SEP with
    probability p_sep where it is live, never EOS), until `steps` tokens.  -> [state], the start state first."""
    S = ntok + table.shape[0]
    st, out = faces.sequence_rule_start(), []
    nopad = np.zeros(S, dtype=bool)
    out.append(st)
    for _ in range(steps):
        masked, dead = faces.sequence_rule_mask(st, flags, S, ntok, sep, eos, table, nopad)
        live = np.flatnonzero(~masked[ntok:])
        if dead or not live.size or (not masked[sep] and rng.random() < p_sep):
            if masked[sep]:
                break
            tok = sep
        else:
            tok = ntok + int(rng.choice(live))
        st = faces.sequence_rule_advance(st, tok, flags, ntok, sep, table)
        out.append(st)
    return out


# (golden, kind, seed, flags, form) -> (left-out pairs, pairs, enclosed faces, parsed faces, dead ends, late dead ends, open ends) of
# the ORACLE's own decode under the form: tools/sequence_closure_left_out.py keeps a tuple only if the fp32 oracle against the fp64
# oracle forced along it leaves out at most CAP of the (step, unfinished row) pairs.  A seed is changed, never the cap.
KEPT = {
    ('seq_small_gain4', 'lattice', 1, 3, 'lookahead'): (0, 33, 5, 5, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 29; rows at EOS 2; EOS at 29, EOS at 4
    ('seq_small_gain4', 'lattice', 1, 3, 'exact'): (0, 33, 5, 5, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 29; rows at EOS 2; EOS at 29, EOS at 4
    ('seq_small_gain4', 'lattice', 1, 7, 'lookahead'): (0, 26, 6, 6, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 22; rows at EOS 2; EOS at 22, EOS at 4
    ('seq_small_gain4', 'lattice', 1, 7, 'exact'): (0, 26, 6, 6, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 22; rows at EOS 2; EOS at 22, EOS at 4
    ('seq_small_gain4', 'lattice', 2, 3, 'lookahead'): (0, 58, 9, 9, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 29; rows at EOS 0; closed at T, closed at T
    ('seq_small_gain4', 'lattice', 2, 3, 'exact'): (0, 58, 9, 9, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 29; rows at EOS 0; closed at T, closed at T
    ('seq_small_gain4', 'lattice', 2, 7, 'lookahead'): (0, 38, 6, 6, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 22; rows at EOS 2; EOS at 22, EOS at 16
    ('seq_small_gain4', 'lattice', 2, 7, 'exact'): (0, 38, 6, 6, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 22; rows at EOS 2; EOS at 22, EOS at 16
    ('seq_small_eos', 'lattice', 1, 3, 'lookahead'): (0, 19, 3, 3, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 19; rows at EOS 0; closed at T
    ('seq_small_eos', 'lattice', 1, 3, 'exact'): (0, 19, 3, 3, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 19; rows at EOS 0; closed at T
    ('seq_small_eos', 'lattice', 1, 7, 'lookahead'): (0, 14, 3, 3, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 14; rows at EOS 1; EOS at 14
    ('seq_small_eos', 'lattice', 1, 7, 'exact'): (0, 14, 3, 3, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 14; rows at EOS 1; EOS at 14
    ('seq_small_eos', 'lattice', 2, 3, 'lookahead'): (0, 19, 2, 2, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 19; rows at EOS 1; EOS at 19
    ('seq_small_eos', 'lattice', 2, 3, 'exact'): (0, 19, 2, 2, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 19; rows at EOS 1; EOS at 19
    ('seq_small_eos', 'lattice', 2, 7, 'lookahead'): (0, 16, 3, 3, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 16; rows at EOS 1; EOS at 16
    ('seq_small_eos', 'lattice', 2, 7, 'exact'): (0, 16, 3, 3, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 16; rows at EOS 1; EOS at 16
    ('seq_small_repeat_eos', 'lattice', 2, 3, 'lookahead'): (0, 5, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 4; rows at EOS 2; EOS at 4, EOS at 1
    ('seq_small_repeat_eos', 'lattice', 2, 3, 'exact'): (0, 5, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 4; rows at EOS 2; EOS at 4, EOS at 1
    ('seq_small_repeat_eos', 'lattice', 2, 7, 'lookahead'): (0, 5, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 4; rows at EOS 2; EOS at 4, EOS at 1
    ('seq_small_repeat_eos', 'lattice', 2, 7, 'exact'): (0, 5, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 4; rows at EOS 2; EOS at 4, EOS at 1
    ('seq_small_gain4', 'random', 1, 3, 'lookahead'): (0, 8, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 7; rows at EOS 2; EOS at 7, EOS at 1
    ('seq_small_gain4', 'random', 1, 3, 'exact'): (0, 8, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 7; rows at EOS 2; EOS at 7, EOS at 1
    ('seq_small_gain4', 'random', 1, 7, 'lookahead'): (0, 8, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 7; rows at EOS 2; EOS at 7, EOS at 1
    ('seq_small_gain4', 'random', 1, 7, 'exact'): (0, 8, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 7; rows at EOS 2; EOS at 7, EOS at 1
    ('seq_small_gain4', 'random', 2, 3, 'lookahead'): (0, 33, 2, 5, 3, 2, 0),   # fp32 = fp64 tokens: True; steps 29; rows at EOS 2; EOS at 29, EOS at 4
    ('seq_small_gain4', 'random', 2, 3, 'exact'): (0, 27, 2, 4, 2, 0, 0),   # fp32 = fp64 tokens: True; steps 23; rows at EOS 2; EOS at 23, EOS at 4
    ('seq_small_gain4', 'random', 2, 7, 'lookahead'): (0, 18, 1, 3, 2, 2, 0),   # fp32 = fp64 tokens: True; steps 14; rows at EOS 2; EOS at 14, EOS at 4
    ('seq_small_gain4', 'random', 2, 7, 'exact'): (0, 18, 2, 5, 3, 0, 0),   # fp32 = fp64 tokens: True; steps 14; rows at EOS 2; EOS at 14, EOS at 4
    ('seq_small_eos', 'random', 1, 3, 'lookahead'): (0, 6, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 1; EOS at 6
    ('seq_small_eos', 'random', 1, 3, 'exact'): (0, 6, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 1; EOS at 6
    ('seq_small_eos', 'random', 1, 7, 'lookahead'): (0, 6, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 1; EOS at 6
    ('seq_small_eos', 'random', 1, 7, 'exact'): (0, 6, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 1; EOS at 6
    ('seq_small_eos', 'random', 2, 3, 'lookahead'): (0, 1, 0, 0, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 1; rows at EOS 1; EOS at 1
    ('seq_small_eos', 'random', 2, 3, 'exact'): (0, 1, 0, 0, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 1; rows at EOS 1; EOS at 1
    ('seq_small_eos', 'random', 2, 7, 'lookahead'): (0, 1, 0, 0, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 1; rows at EOS 1; EOS at 1
    ('seq_small_eos', 'random', 2, 7, 'exact'): (0, 1, 0, 0, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 1; rows at EOS 1; EOS at 1
    ('seq_small_repeat_eos', 'random', 1, 3, 'lookahead'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
    ('seq_small_repeat_eos', 'random', 1, 3, 'exact'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
    ('seq_small_repeat_eos', 'random', 1, 7, 'lookahead'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
    ('seq_small_repeat_eos', 'random', 1, 7, 'exact'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
    ('seq_small_repeat_eos', 'random', 2, 3, 'lookahead'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
    ('seq_small_repeat_eos', 'random', 2, 3, 'exact'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
    ('seq_small_repeat_eos', 'random', 2, 7, 'lookahead'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
    ('seq_small_repeat_eos', 'random', 2, 7, 'exact'): (0, 7, 1, 1, 0, 0, 0),   # fp32 = fp64 tokens: True; steps 6; rows at EOS 2; EOS at 1, EOS at 6
}

# The flag-3 fixtures sequence_constrain_ref.KEPT records as "open at T": under either form open_end is all 0 there.
OPEN_AT_T = [("seq_small_gain4", "lattice", 2), ("seq_small_eos", "lattice", 1), ("seq_small_eos", "lattice", 2),
             ("seq_small_gain4", "random", 1), ("seq_small_gain4", "random", 2), ("seq_small_repeat_eos", "random", 1)]
# The random fixtures on which the fp64 oracle under the plain rule meets a late dead end and under "exact" none (the tool's table).
LATE_PLAIN = [('seq_small_gain4', 'random', 1, 3),
              ('seq_small_gain4', 'random', 1, 7),
              ('seq_small_gain4', 'random', 2, 3),
              ('seq_small_gain4', 'random', 2, 7),
              ('seq_small_eos', 'random', 1, 7),
              ('seq_small_eos', 'random', 2, 3),
              ('seq_small_eos', 'random', 2, 7),
              ('seq_small_repeat_eos', 'random', 1, 3),
              ('seq_small_repeat_eos', 'random', 1, 7),
              ('seq_small_repeat_eos', 'random', 2, 3),
              ('seq_small_repeat_eos', 'random', 2, 7)]
