"""The sampled loop-constrained single-sequence decode as a numpy loop, and the tuples the engine tests use.

Nothing of the rule or of the draw is restated: one step is faces.sequence_rule_mask (DESIGN.md 32's byte row), sample_ref.sample_row
on the constrained row (DESIGN.md 15's draw, with its guard band) and faces.sequence_rule_advance; what is stated here is the
decode around it, which is sequence_sample_ref's layout with sequence_constrain_ref's state per draw.

  layout   N * R rows; draw k of wireframe w is row w * R + k, reads uniforms[t, w * R + k] at step t and wireframe w's table.
  start    every draw holds SOS at position 0, log-probability 0, the state empty and closed.
  finish   a draw is finished from the first position >= 1 that holds EOS.  A finished draw appends 0 with log-probability 0.
  stop     after the first step after which every draw is finished (steps = that step + 1), else after T - 1 steps.
  open_end a loop is open (first != none) after the draw's last kept position min(own EOS, stop step).
"""
import numpy as np

import sample_ref as SR
import sequence_constrain_ref as SC
import sequence_sample_ref as QR
from faceformer_amd import faces

FILL, EPS, LP_BAR, CAP, TOL = SC.FILL, SC.EPS, SC.LP_BAR, SR.CAP, SC.TOL
NO_REPEAT, CONNECT, ONCE, LOOPS, COEDGE_LOOPS = SC.NO_REPEAT, SC.CONNECT, SC.ONCE, SC.LOOPS, SC.COEDGE_LOOPS
stop_and_finish, unfinished_after, make_uniforms = QR.stop_and_finish, QR.unfinished_after, QR.make_uniforms
FIXTURES, FLAGS, fixture, face_pieces = SC.FIXTURES, SC.FLAGS, SC.fixture, SC.face_pieces

# The engine replay: R draws per wireframe, the seed of the uniforms per golden, the parameter sets (sample_ref's), on every
# fixture of FIXTURES.
REPLAY_FIXTURES = FIXTURES
REPLAY_R = 4
REPLAY_PARAMS = SR.REPLAY_PARAMS
REPLAY_SEEDS = {"seq_small_gain4": 5, "seq_small_eos": 5, "seq_small_repeat_eos": 5}

# (golden, kind, seed, flags, (tau, K, P)) -> (left-out pairs, pairs, enclosed faces, parsed faces, dead ends) of the ORACLE's own
# constrained sampled decode at REPLAY_R draws with the uniforms of REPLAY_SEEDS: tools/sequence_constrain_sample_left_out.py keeps
# a tuple only if the fp64 oracle forced along the fp32 oracle's draws leaves out at most CAP of the (step, unfinished draw) pairs
# (a pair is left out inside sample_ref's guard band).  A seed is changed, never the cap.  DROPPED: tried and above the cap.
KEPT = {
    ('seq_small_eos', 'lattice', 1, 3, (0.8, 16, 0.9)): (0, 76, 8, 12, 0),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 0 of 4
    ('seq_small_eos', 'lattice', 1, 3, (1.0, 0, 1.0)): (0, 76, 8, 12, 0),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 0 of 4
    ('seq_small_eos', 'lattice', 1, 7, (0.8, 16, 0.9)): (0, 56, 12, 12, 0),   # decisive fp64 draws = fp32 draws: True; steps 14; draws at EOS 4 of 4
    ('seq_small_eos', 'lattice', 1, 7, (1.0, 0, 1.0)): (0, 56, 12, 12, 0),   # decisive fp64 draws = fp32 draws: True; steps 14; draws at EOS 4 of 4
    ('seq_small_eos', 'lattice', 2, 3, (0.8, 16, 0.9)): (0, 76, 4, 8, 0),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 0 of 4
    ('seq_small_eos', 'lattice', 2, 3, (1.0, 0, 1.0)): (0, 76, 4, 8, 0),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 0 of 4
    ('seq_small_eos', 'lattice', 2, 7, (0.8, 16, 0.9)): (0, 64, 12, 12, 0),   # decisive fp64 draws = fp32 draws: True; steps 16; draws at EOS 4 of 4
    ('seq_small_eos', 'lattice', 2, 7, (1.0, 0, 1.0)): (0, 64, 12, 12, 0),   # decisive fp64 draws = fp32 draws: True; steps 16; draws at EOS 4 of 4
    ('seq_small_eos', 'random', 1, 3, (0.8, 16, 0.9)): (0, 76, 0, 12, 8),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 0 of 4
    ('seq_small_eos', 'random', 1, 3, (1.0, 0, 1.0)): (0, 76, 0, 12, 8),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 0 of 4
    ('seq_small_eos', 'random', 1, 7, (0.8, 16, 0.9)): (0, 52, 0, 12, 12),   # decisive fp64 draws = fp32 draws: True; steps 13; draws at EOS 4 of 4
    ('seq_small_eos', 'random', 1, 7, (1.0, 0, 1.0)): (0, 52, 0, 12, 12),   # decisive fp64 draws = fp32 draws: True; steps 13; draws at EOS 4 of 4
    ('seq_small_eos', 'random', 2, 3, (0.8, 16, 0.9)): (0, 16, 0, 4, 4),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 4 of 4
    ('seq_small_eos', 'random', 2, 3, (1.0, 0, 1.0)): (0, 16, 0, 4, 4),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 4 of 4
    ('seq_small_eos', 'random', 2, 7, (0.8, 16, 0.9)): (0, 16, 0, 4, 4),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 4 of 4
    ('seq_small_eos', 'random', 2, 7, (1.0, 0, 1.0)): (0, 16, 0, 4, 4),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 4 of 4
    ('seq_small_gain4', 'lattice', 1, 3, (0.8, 16, 0.9)): (0, 132, 18, 20, 0),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 4 of 8
    ('seq_small_gain4', 'lattice', 1, 3, (1.0, 0, 1.0)): (0, 132, 20, 22, 0),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 4 of 8
    ('seq_small_gain4', 'lattice', 1, 7, (0.8, 16, 0.9)): (0, 108, 24, 24, 0),   # decisive fp64 draws = fp32 draws: True; steps 26; draws at EOS 8 of 8
    ('seq_small_gain4', 'lattice', 1, 7, (1.0, 0, 1.0)): (0, 108, 24, 24, 0),   # decisive fp64 draws = fp32 draws: True; steps 26; draws at EOS 8 of 8
    ('seq_small_gain4', 'lattice', 2, 3, (0.8, 16, 0.9)): (0, 232, 34, 40, 0),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 0 of 8
    ('seq_small_gain4', 'lattice', 2, 3, (1.0, 0, 1.0)): (0, 232, 40, 46, 0),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 0 of 8
    ('seq_small_gain4', 'lattice', 2, 7, (0.8, 16, 0.9)): (0, 153, 27, 27, 0),   # decisive fp64 draws = fp32 draws: True; steps 25; draws at EOS 8 of 8
    ('seq_small_gain4', 'lattice', 2, 7, (1.0, 0, 1.0)): (0, 151, 27, 27, 0),   # decisive fp64 draws = fp32 draws: True; steps 25; draws at EOS 8 of 8
    ('seq_small_gain4', 'random', 1, 3, (0.8, 16, 0.9)): (0, 132, 0, 32, 28),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 4 of 8
    ('seq_small_gain4', 'random', 1, 3, (1.0, 0, 1.0)): (0, 132, 0, 32, 28),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 4 of 8
    ('seq_small_gain4', 'random', 1, 7, (0.8, 16, 0.9)): (0, 72, 0, 16, 16),   # decisive fp64 draws = fp32 draws: True; steps 14; draws at EOS 8 of 8
    ('seq_small_gain4', 'random', 1, 7, (1.0, 0, 1.0)): (0, 72, 0, 16, 16),   # decisive fp64 draws = fp32 draws: True; steps 14; draws at EOS 8 of 8
    ('seq_small_gain4', 'random', 2, 3, (0.8, 16, 0.9)): (0, 227, 4, 35, 27),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 1 of 8
    ('seq_small_gain4', 'random', 2, 3, (1.0, 0, 1.0)): (0, 222, 4, 35, 27),   # decisive fp64 draws = fp32 draws: True; steps 29; draws at EOS 2 of 8
    ('seq_small_gain4', 'random', 2, 7, (0.8, 16, 0.9)): (0, 136, 4, 34, 30),   # decisive fp64 draws = fp32 draws: True; steps 22; draws at EOS 8 of 8
    ('seq_small_gain4', 'random', 2, 7, (1.0, 0, 1.0)): (0, 138, 2, 33, 31),   # decisive fp64 draws = fp32 draws: True; steps 24; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'lattice', 2, 3, (0.8, 16, 0.9)): (0, 17, 3, 3, 0),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'lattice', 2, 3, (1.0, 0, 1.0)): (0, 17, 3, 3, 0),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'lattice', 2, 7, (0.8, 16, 0.9)): (0, 17, 3, 3, 0),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'lattice', 2, 7, (1.0, 0, 1.0)): (0, 17, 3, 3, 0),   # decisive fp64 draws = fp32 draws: True; steps 4; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'random', 1, 3, (0.8, 16, 0.9)): (0, 82, 0, 18, 18),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 5 of 8
    ('seq_small_repeat_eos', 'random', 1, 3, (1.0, 0, 1.0)): (0, 82, 0, 18, 18),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 5 of 8
    ('seq_small_repeat_eos', 'random', 1, 7, (0.8, 16, 0.9)): (0, 52, 0, 12, 12),   # decisive fp64 draws = fp32 draws: True; steps 9; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'random', 1, 7, (1.0, 0, 1.0)): (0, 52, 0, 12, 12),   # decisive fp64 draws = fp32 draws: True; steps 9; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'random', 2, 3, (0.8, 16, 0.9)): (0, 102, 4, 33, 29),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 7 of 8
    ('seq_small_repeat_eos', 'random', 2, 3, (1.0, 0, 1.0)): (0, 102, 4, 33, 29),   # decisive fp64 draws = fp32 draws: True; steps 19; draws at EOS 7 of 8
    ('seq_small_repeat_eos', 'random', 2, 7, (0.8, 16, 0.9)): (0, 76, 4, 24, 20),   # decisive fp64 draws = fp32 draws: True; steps 11; draws at EOS 8 of 8
    ('seq_small_repeat_eos', 'random', 2, 7, (1.0, 0, 1.0)): (0, 76, 4, 24, 20),   # decisive fp64 draws = fp32 draws: True; steps 11; draws at EOS 8 of 8
}
DROPPED = {}      # none: every tuple tried stayed within the cap


def step(row, pad, state, flags, ntok, sep, eos, follows, u, tau=1.0, K=0, P=1.0, finished=False):
    """One draw of one step on a RAW (or already masked) logit row.  -> dict(tok, logprob, row (the constrained masked row, fp64),
    masked (the rule's own byte row), dead, fin, state (after the step), decisive (sample_row's flag: the cut and the draw lie
    outside the guard band)).  A finished draw appends token 0 with log-probability 0 and keeps its state."""
    row = np.asarray(row, dtype=np.float64)
    S = len(row)
    if finished:
        return dict(tok=0, logprob=0.0, row=row, masked=np.zeros(S, bool), dead=False, fin=True, state=state, decisive=True)
    pad = np.asarray(pad, dtype=bool)
    masked, dead = faces.sequence_rule_mask(state, flags, S, ntok, sep, eos, follows, pad)
    con = np.where(masked | pad, FILL, row)
    res = SR.sample_row(con, u, tau, K, P)
    return dict(tok=res["tok"], logprob=float(res["logprob"]), row=con, masked=masked, dead=dead, fin=res["tok"] == eos,
                state=faces.sequence_rule_advance(state, res["tok"], flags, ntok, sep, follows), decisive=res["decisive"])


def decode(step_logits, u, N, T, R, flags, ntok, sos, sep, eos, follows, tau=1.0, K=0, P=1.0):
    """The whole rule as a loop: step_logits(paths [N*R, T], step) -> masked logits [N*R, S] (fp64, padded keys at or below FILL) of
    `step` along the tokens so far.  Returns dict(tokens, logprob, dead [N*R, T], open_end [N*R], steps, step_counts, decisive
    [T-1, N*R] (True where the draw was finished))."""
    B = N * R
    tok = np.zeros((B, T), dtype=np.int64)
    lp = np.zeros((B, T))
    dead = np.zeros((B, T), dtype=np.int32)
    tok[:, 0] = sos
    state = [faces.sequence_rule_start() for _ in range(B)]
    fin = np.zeros(B, dtype=bool)
    dec = np.ones((max(T - 1, 1), B), dtype=bool)
    counts, steps = [], T - 1
    for s in range(T - 1):
        lg = np.asarray(step_logits(tok, s), dtype=np.float64)
        for r in np.flatnonzero(~fin):
            res = step(lg[r], lg[r] <= FILL, state[r], flags, ntok, sep, eos, None if follows is None else follows[r // R], u[s, r],
                       tau, K, P)
            tok[r, s + 1], lp[r, s + 1], dead[r, s + 1], state[r], fin[r] = res["tok"], res["logprob"], res["dead"], res["state"], res["fin"]
            dec[s, r] = res["decisive"]
        counts.append(int((~fin).sum()))
        if fin.all():
            steps = s + 1
            break
    return dict(tokens=tok, logprob=lp, dead=dead, open_end=np.array([int(st[1] is not None) for st in state]), steps=steps,
                step_counts=counts, decisive=dec)


def replay_states(tokens, R, flags, ntok, sep, follows):
    """state[r][j]: the rule's state of draw r (of wireframe r // R) after position j of `tokens` [N*R, T]."""
    rep = None if follows is None else [follows[r // R] for r in range(tokens.shape[0])]
    return SC.replay_states(tokens, flags, ntok, sep, rep)


def walk_closed(idx, table):
    """faces.is_face_enclosed's walk on a follow table (the random tables have no end points)."""
    first = prev = None
    for e in idx:
        if first is None:
            first = e
        elif not table[prev][e]:
            return False
        prev = e
        if table[e][first]:
            first = None
    return first is None


def guarantee(tokens, dead, open_end, R, ni, flags, ntok, sep, eos, follows, edges):
    """Guarantee (c) on every draw, asserted: every parsed face whose boundary was not selected at a dead end, and that is not the
    open piece of an open_end draw, passes the enclosure walk (faces.is_face_enclosed on the lattice's end points; the table's own
    walk for a random table); no face holds an edge twice; under ONCE no edge occurs twice in a draw.
    -> (enclosed faces, parsed faces) over all draws."""
    enc = par = 0
    for r in range(tokens.shape[0]):
        w = r // R
        pieces = face_pieces(tokens[r], dead[r], ntok, sep, eos, ni[w])
        row_edges = [e for idx, _, _ in pieces for e in idx]
        for k, (idx, at_dead_end, unterminated) in enumerate(pieces):
            assert len(set(idx)) == len(idx), (r, idx)
            closed = walk_closed(idx, follows[w]) if edges is None else bool(faces.is_face_enclosed(edges[w], idx, TOL))
            par += 1
            enc += closed
            open_piece = unterminated or (open_end[r] and k == len(pieces) - 1 and (tokens[r] == eos).sum() == 0)
            if flags & CONNECT and not at_dead_end and not open_piece:
                assert closed, (r, idx)
        if flags & ONCE:
            assert len(set(row_edges)) == len(row_edges), r
    return enc, par
