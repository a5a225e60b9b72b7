"""The loop-constrained single-sequence decode as a numpy loop, its fixtures, and the triples the engine tests use.

The rule of one step is faces.sequence_rule_step (the header's text; the device has one copy of the rule as well); what is stated
here is the decode around it -- start, finish, stop, layout -- and the fixtures.

  start    every row holds SOS at position 0, log-probability 0, the state empty and closed.
  finish   a row is finished from the first position >= 1 that holds EOS.  A finished row appends 0 with log-probability 0.
  stop     after the first step after which every row is finished (steps = that step + 1), else after T - 1 steps.  The count the
           engine keeps per step is "rows unfinished after the step".
  open_end a loop is open (first != none) after the row's last kept position min(own EOS, stop step).
"""
import numpy as np

import constrain_ref as CR
import sequence_sample_ref as QR
from faceformer_amd import faces

FILL, EPS, LP_BAR, CAP, TOL = CR.FILL, CR.EPS, CR.LP_BAR, CR.CAP, CR.TOL
NO_REPEAT, CONNECT, ONCE = faces.SEQ_NO_REPEAT, faces.SEQ_CONNECT, faces.SEQ_ONCE
LOOPS, COEDGE_LOOPS = NO_REPEAT | CONNECT, NO_REPEAT | CONNECT | ONCE
stop_and_finish, unfinished_after = QR.stop_and_finish, QR.unfinished_after

# The fixtures of the engine tests: (golden, kind, seed).  "lattice": connected lattice wireframes shaped like the golden
# (constrain_ref.lattice_batch) with the table of their own float32 end points -- they exercise closure; "random": the golden's
# own inputs with a constrain_ref.random_follows table -- they exercise dead ends.  (seq_small_repeat_eos / lattice seed 1 is
# left out: both rows select EOS at step 1 in every mode.)
FIXTURES = [("seq_small_gain4", "lattice", 1), ("seq_small_gain4", "lattice", 2), ("seq_small_eos", "lattice", 1),
            ("seq_small_eos", "lattice", 2), ("seq_small_repeat_eos", "lattice", 2),
            ("seq_small_gain4", "random", 1), ("seq_small_gain4", "random", 2), ("seq_small_eos", "random", 1),
            ("seq_small_eos", "random", 2), ("seq_small_repeat_eos", "random", 1), ("seq_small_repeat_eos", "random", 2)]
FLAGS = (LOOPS, COEDGE_LOOPS)

# (golden, kind, seed, flags) -> (left-out pairs, pairs, enclosed faces, parsed faces, dead ends) of the ORACLE's own constrained
# decode: tools/sequence_constrain_left_out.py keeps a triple only if the fp32 oracle against the fp64 oracle forced along it leaves
# out at most CAP of the (step, unfinished row) pairs.  A seed is changed, never a cap.
KEPT = {
    ('seq_small_gain4', 'lattice', 1, 3): (0, 33, 4, 5, 0),   # greedy 0 of 6; fp32 = fp64 tokens: True; steps 29; closed at T, EOS at 4
    ('seq_small_gain4', 'lattice', 1, 7): (0, 26, 6, 6, 0),   # greedy 0 of 6; fp32 = fp64 tokens: True; steps 22; EOS at 22, EOS at 4
    ('seq_small_gain4', 'lattice', 2, 3): (0, 58, 8, 9, 0),   # greedy 1 of 6; fp32 = fp64 tokens: True; steps 29; open at T, closed at T
    ('seq_small_gain4', 'lattice', 2, 7): (0, 38, 6, 6, 0),   # greedy 1 of 6; fp32 = fp64 tokens: True; steps 22; EOS at 22, EOS at 16
    ('seq_small_eos', 'lattice', 1, 3): (0, 19, 2, 3, 0),   # greedy 0 of 3; fp32 = fp64 tokens: True; steps 19; open at T
    ('seq_small_eos', 'lattice', 1, 7): (0, 14, 3, 3, 0),   # greedy 0 of 3; fp32 = fp64 tokens: True; steps 14; EOS at 14
    ('seq_small_eos', 'lattice', 2, 3): (0, 19, 1, 2, 0),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 19; open at T
    ('seq_small_eos', 'lattice', 2, 7): (0, 16, 3, 3, 0),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 16; EOS at 16
    ('seq_small_repeat_eos', 'lattice', 2, 3): (0, 5, 1, 1, 0),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 4; EOS at 4, EOS at 1
    ('seq_small_repeat_eos', 'lattice', 2, 7): (0, 5, 1, 1, 0),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 4; EOS at 4, EOS at 1
    ('seq_small_gain4', 'random', 1, 3): (0, 33, 0, 8, 7),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 29; open at T, EOS at 4
    ('seq_small_gain4', 'random', 1, 7): (0, 18, 0, 4, 4),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 14; EOS at 14, EOS at 4
    ('seq_small_gain4', 'random', 2, 3): (0, 58, 1, 9, 7),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 29; open at T, open at T
    ('seq_small_gain4', 'random', 2, 7): (0, 35, 1, 9, 8),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 22; EOS at 22, EOS at 13
    ('seq_small_eos', 'random', 1, 3): (0, 19, 0, 3, 2),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 19; closed at T
    ('seq_small_eos', 'random', 1, 7): (0, 13, 0, 3, 3),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 13; EOS at 13
    ('seq_small_eos', 'random', 2, 3): (0, 4, 0, 1, 1),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 4; EOS at 4
    ('seq_small_eos', 'random', 2, 7): (0, 4, 0, 1, 1),   # greedy 0 of 1; fp32 = fp64 tokens: True; steps 4; EOS at 4
    ('seq_small_repeat_eos', 'random', 1, 3): (0, 23, 0, 5, 5),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 19; EOS at 4, open at T
    ('seq_small_repeat_eos', 'random', 1, 7): (0, 13, 0, 3, 3),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 9; EOS at 4, EOS at 9
    ('seq_small_repeat_eos', 'random', 2, 3): (0, 23, 1, 7, 6),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 14; EOS at 9, EOS at 14
    ('seq_small_repeat_eos', 'random', 2, 7): (0, 19, 1, 6, 5),   # greedy 0 of 2; fp32 = fp64 tokens: True; steps 11; EOS at 11, EOS at 8
}


def fixture(case, gb, kind, seed):
    """-> (batch dict of CPU tensors: input, input_mask, label [N, T], num_input; follows bool [N, L, L]; edges: per wireframe the
    float32 point lists the enclosure walk reads, or None for a random table)."""
    import torch
    m = case["model"]
    ni = [int(n) for n in case["n_edges"]]
    if kind == "lattice":
        batch, edges, _ = CR.lattice_batch(ni, m["L"], m["seq_len"], seed)
        batch["label"] = torch.zeros((len(ni), m["seq_len"]), dtype=torch.int64)
        follows = faces.follow_table(batch["input"].numpy(), TOL, ni)
        return batch, follows, edges
    batch = dict(gb)
    batch["num_input"] = ni
    return batch, CR.random_follows(len(ni), m["L"], seed), None


def decode(step_logits, N, T, flags, ntok, sos, sep, eos, follows):
    """The whole rule as a loop: step_logits(paths [N, T], step) -> masked logits [N, S] (fp64, padded keys at or below FILL) of
    `step` along the tokens so far.  Returns dict(tokens [N, T], logprob [N, T], dead [N, T], open_end [N], steps, rows [T-1, N, S]
    the constrained rows it selected from (NaN where the row was finished))."""
    tok = np.zeros((N, T), dtype=np.int64)
    lp = np.zeros((N, T))
    dead = np.zeros((N, T), dtype=np.int32)
    tok[:, 0] = sos
    state = [faces.sequence_rule_start() for _ in range(N)]
    fin = np.zeros(N, dtype=bool)
    rows = None
    steps = T - 1
    for s in range(T - 1):
        lg = np.asarray(step_logits(tok, s), dtype=np.float64)
        if rows is None:
            rows = np.full((max(T - 1, 1),) + lg.shape, np.nan)
        for r in np.flatnonzero(~fin):
            res = faces.sequence_rule_step(lg[r], lg[r] <= FILL, state[r], flags, ntok, sep, eos, None if follows is None else follows[r])
            tok[r, s + 1], lp[r, s + 1], dead[r, s + 1], state[r], fin[r] = res["tok"], res["logprob"], res["dead"], res["state"], res["fin"]
            rows[s, r] = res["row"]
        if fin.all():
            steps = s + 1
            break
    return dict(tokens=tok, logprob=lp, dead=dead, open_end=np.array([int(st[1] is not None) for st in state]), steps=steps, rows=rows)


def replay_states(tokens, flags, ntok, sep, follows):
    """state[r][j]: the rule's state of row r after position j of `tokens` [N, T]."""
    out = []
    for r in range(tokens.shape[0]):
        st, row = faces.sequence_rule_start(), []
        for j in range(tokens.shape[1]):
            if j:
                st = faces.sequence_rule_advance(st, int(tokens[r, j]), flags, ntok, sep, None if follows is None else follows[r])
            row.append(st)
        out.append(row)
    return out


def margin(row):
    """The margin between the two best LIVE keys of a constrained row (inf with fewer than two)."""
    live = np.sort(row[row > FILL])
    return live[-1] - live[-2] if live.size > 1 else np.inf


def face_pieces(tokens, dead, ntok, sep, eos, num_edges):
    """The parsed faces of one row exactly as faces._seq_faces cuts them (the prefix through the first EOS, split after every SEP,
    the last token of a piece dropped, edges in [0, num_edges) kept, pieces without an edge skipped), each with two flags: its
    boundary token was a SEP selected at a dead end; the piece is the row's last and ends in neither SEP nor EOS (the open piece
    of a row that ran out of positions): [(edges tuple, at_dead_end, unterminated)]."""
    seq = np.asarray(tokens, dtype=np.int64)
    hit = np.flatnonzero(seq == eos)
    if hit.size:
        seq = seq[: hit[0] + 1]
    out, start = [], 0
    cuts = list(np.flatnonzero(seq == sep) + 1) + [len(seq)]
    for c in cuts:
        piece = seq[start:c]
        if piece.size > 1:
            v = piece[:-1] - ntok
            idx = tuple(int(x) for x in v[(v >= 0) & (v < num_edges)])
            last = int(piece[-1])
            if idx:
                out.append((idx, last == sep and bool(dead[c - 1]), last != sep and last != eos))
        start = c
    return out
