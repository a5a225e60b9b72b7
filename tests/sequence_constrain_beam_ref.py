"""The beam search over the loop-constrained single-sequence decode in numpy fp64, and the cases the tests use.

Nothing of the rule, of the order or of the layout is restated: a beam's row is faces.sequence_rule_mask's, its state
moves by faces.sequence_rule_advance, the gap of a group is measured in beam_ref.score_bound's units with beam_ref.group_step's
expression, the back-tracking is beam_ref.backtrack, and start, counters and stop are sequence_beam_ref's.  What is stated here is
what the combination adds -- which keys are candidates, and what a new beam inherits.

  candidates  an empty beam none; a finished beam itself (token 0, score unchanged); an unfinished beam its LIVE keys (row > FILL)
              at c_k + log_softmax(constrained row), or -- with no live key at all -- token 0 at c_k - log S.
  new beam    parent p, token tk: state = advance(state[p], tk); fin = fin[p] | tk == EOS; dead = p dead-ended at this step (a dead
              end abandons the face, not the beam); open = the new state's loop is open.  A finished parent hands everything on.
  empty rank  parent = the rank, token 0, score -inf, flags clear, the state of its own index.
"""
import numpy as np

import beam_ref as R
import sequence_beam_ref as QB
import sequence_constrain_ref as SC
from faceformer_amd import faces

FILL, FLT_MAX, NEG, CAP, TOL = SC.FILL, R.FLT_MAX, -np.inf, QB.CAP, SC.TOL
NO_REPEAT, CONNECT, ONCE, LOOPS, COEDGE_LOOPS = SC.NO_REPEAT, SC.CONNECT, SC.ONCE, SC.LOOPS, SC.COEDGE_LOOPS
STOPS, FIXTURES, FLAGS, fixture, face_pieces = QB.STOPS, SC.FIXTURES, SC.FLAGS, SC.fixture, SC.face_pieces
counters, stop_step = QB.counters, QB.stop_step

# The operator test's grid (the issue's): S x W (W <= S) x groups x flags x both stop forms, one seed per (S, W, groups, flags).
# tools/sequence_constrain_beam_left_out.py operator keeps a seed only if the rule alone -- applied in fp64 and in fp32-rounded
# arithmetic on the CPU -- leaves out at most CAP of the case's groups; otherwise the offset below changes.
OP_S, OP_W, OP_G, OP_FLAGS = (5, 65, 260, 1028), (1, 3, 8), (1, 5), (0, 1, 3, 7)
OP_SCENARIOS = ("mixed", "mixed2", "sep", "done")
# (S, W, groups, flags, scenario) -> offset from op_seed_base.  Every case kept its base seed under the cap; the two offsets are
# there for coverage: at W = 1 a cell has 1 + 5 rows per case, and with the base seeds no open row of the S = 260 / 1028 cells
# closed its loop -- the first offset (searched on the CPU, under the same cap) at which one does.
OP_SEED_OFFSETS = {(260, 1, 5, 7, "mixed"): 1, (1028, 1, 5, 3, "mixed"): 1}


def op_seed_base(S, W, G, flags, scenario):
    return 1000 * OP_SCENARIOS.index(scenario) + 100 * flags + 10 * W + G + S % 7


def op_seed(S, W, G, flags, scenario):
    return op_seed_base(S, W, G, flags, scenario) + OP_SEED_OFFSETS.get((S, W, G, flags, scenario), 0)


# The engine's replay tuples: (golden, kind, seed, flags, W) -> (left-out pairs, pairs, enclosed faces, parsed faces, dead ends over
# the non-empty final beams, steps under "all") of the ORACLE's own constrained beam decode, as
# tools/sequence_constrain_beam_left_out.py engine prints them: the fp32 oracle searches its own constrained beams, the fp64 oracle
# is forced along them, and a (step, group) pair is left out when its fp64 gap is at most 1 (twice the accumulated bound).  A tuple
# is kept only if the oracle alone leaves out at most CAP of its pairs.  DROPPED: tried and above the cap.
REPLAY_W = (2, 4)
KEPT = {
    ('seq_small_eos', 'lattice', 1, 3, 2): (0, 19, 4, 6, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 1, 3, 4): (0, 19, 8, 12, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 1, 7, 2): (0, 14, 6, 6, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 1, 7, 4): (0, 14, 10, 10, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 2, 3, 2): (0, 19, 2, 4, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 2, 3, 4): (0, 19, 7, 10, 0, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 4 non-empty beams
    ('seq_small_eos', 'lattice', 2, 7, 2): (0, 16, 6, 6, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'lattice', 2, 7, 4): (0, 16, 9, 9, 0, 16),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 1, 3, 2): (0, 19, 0, 6, 4, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 2 non-empty beams
    ('seq_small_eos', 'random', 1, 3, 4): (0, 19, 1, 11, 7, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 4 non-empty beams
    ('seq_small_eos', 'random', 1, 7, 2): (0, 13, 1, 4, 3, 13),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 1, 7, 4): (0, 13, 1, 8, 7, 13),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_eos', 'random', 2, 3, 2): (0, 19, 0, 7, 7, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 2 non-empty beams
    ('seq_small_eos', 'random', 2, 3, 4): (0, 19, 0, 17, 16, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 4 non-empty beams
    ('seq_small_eos', 'random', 2, 7, 2): (0, 12, 0, 4, 4, 12),   # decisive fp64 decisions = fp32 decisions: True; finished 2 of 2 non-empty beams
    ('seq_small_eos', 'random', 2, 7, 4): (0, 12, 0, 5, 5, 12),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 3, 2): (0, 58, 13, 15, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 3, 4): (0, 58, 23, 25, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 7, 2): (0, 52, 13, 13, 0, 26),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 1, 7, 4): (0, 52, 28, 28, 0, 26),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 3, 2): (0, 58, 16, 18, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 3, 4): (0, 58, 34, 38, 0, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 0 of 8 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 7, 2): (0, 50, 13, 13, 0, 25),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'lattice', 2, 7, 4): (0, 50, 28, 28, 0, 25),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 1, 3, 2): (0, 58, 0, 25, 23, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 4 non-empty beams
    ('seq_small_gain4', 'random', 1, 3, 4): (0, 58, 0, 58, 56, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 8 non-empty beams
    ('seq_small_gain4', 'random', 1, 7, 2): (0, 44, 0, 13, 13, 22),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 1, 7, 4): (0, 48, 1, 31, 30, 24),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_gain4', 'random', 2, 3, 2): (0, 58, 2, 18, 14, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 1 of 4 non-empty beams
    ('seq_small_gain4', 'random', 2, 3, 4): (0, 58, 4, 34, 26, 29),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 8 non-empty beams
    ('seq_small_gain4', 'random', 2, 7, 2): (0, 48, 1, 17, 16, 24),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_gain4', 'random', 2, 7, 4): (0, 48, 1, 33, 32, 24),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 3, 2): (0, 10, 2, 2, 0, 5),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 3, 4): (0, 28, 7, 7, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 7, 2): (0, 10, 2, 2, 0, 5),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'lattice', 2, 7, 4): (0, 28, 7, 7, 0, 14),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 3, 2): (0, 38, 0, 7, 7, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 3, 4): (0, 38, 0, 20, 20, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 8 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 7, 2): (0, 18, 0, 4, 4, 9),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 1, 7, 4): (0, 18, 0, 12, 12, 9),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 3, 2): (0, 38, 2, 18, 16, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 3 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 3, 4): (0, 38, 4, 42, 37, 19),   # decisive fp64 decisions = fp32 decisions: True; finished 5 of 8 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 7, 2): (0, 26, 1, 12, 11, 13),   # decisive fp64 decisions = fp32 decisions: True; finished 4 of 4 non-empty beams
    ('seq_small_repeat_eos', 'random', 2, 7, 4): (0, 26, 3, 25, 22, 13),   # decisive fp64 decisions = fp32 decisions: True; finished 8 of 8 non-empty beams
}
DROPPED = {}      # none: every tuple tried stayed within the cap


def group_step(raw, pad, scores, fin, states, flags, ntok, sep, eos, follows, margin=1):
    """One step of ONE group on RAW logits [W, S] (rows of empty / finished beams are not read); pad [S] bool.  -> dict(parent, tok,
    scores, fin, dead, open [W each], states [W], rows / masked [W]: the constrained masked fp64 row and the rule's own mask of every
    non-empty unfinished beam (None otherwise), dead_now [W] (of the OLD beams), gap: beam_ref.group_step's -- the smallest
    decisive gap among the first W + 1 candidates in units of twice `margin` x score_bound)."""
    raw = np.asarray(raw, dtype=np.float64)
    W, S = raw.shape
    scs, ixs = [], []
    rows, masks, dead_now = [None] * W, [None] * W, np.zeros(W, dtype=bool)
    for k in range(W):
        if scores[k] == NEG:
            continue
        if fin[k]:
            scs.append(np.array([float(scores[k])])); ixs.append(np.array([k * S]))
            continue
        masked, dn = faces.sequence_rule_mask(states[k], flags, S, ntok, sep, eos, follows, pad)
        row = np.where(masked | pad, FILL, raw[k])
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
        ratio = min(ratio, (a - b) / (2.0 * margin * max(R.score_bound(a), R.score_bound(b))))
    out = dict(parent=np.arange(W), tok=np.zeros(W, dtype=np.int64), scores=np.full(W, NEG), fin=np.zeros(W, dtype=bool),
               dead=np.zeros(W, dtype=bool), open=np.zeros(W, dtype=bool), states=list(states), rows=rows, masked=masks,
               dead_now=dead_now, gap=ratio, candidates=len(sc_all))
    for r, (sc, ix) in enumerate(cand[:W]):
        k, s = divmod(ix, S)
        out["parent"][r], out["scores"][r], out["states"][r] = k, sc, states[k]
        if fin[k]:
            out["fin"][r] = True
        else:
            out["tok"][r], out["fin"][r], out["dead"][r] = s, s == eos, dead_now[k]
            out["states"][r] = faces.sequence_rule_advance(states[k], s, flags, ntok, sep, follows)
        out["open"][r] = out["states"][r][1] is not None
    return out


def beam_step(raw, pads, scores, fin, states, W, flags, ntok, sep, eos, follows, margin=1):
    """group_step over [G * W, S] raw logits, group g = wireframe g: pads [G, S] bool, follows [G] tables (or None).  Arrays of
    G * W entries (states, rows, masked: lists), gap [G], and sequence_beam_ref's two counters of the state after the step."""
    G = raw.shape[0] // W
    res = [group_step(raw[g * W:(g + 1) * W], pads[g], scores[g * W:(g + 1) * W], fin[g * W:(g + 1) * W], states[g * W:(g + 1) * W],
                      flags, ntok, sep, eos, None if follows is None else follows[g], margin) for g in range(G)]
    out = {k: np.concatenate([r[k] for r in res]) for k in ("parent", "tok", "scores", "fin", "dead", "open", "dead_now")}
    for k in ("states", "rows", "masked"):
        out[k] = [x for r in res for x in r[k]]
    out["gap"] = np.array([r["gap"] for r in res])
    out["candidates"] = np.array([r["candidates"] for r in res])
    out["all"], out["best"] = counters(out["scores"], out["fin"], W)
    return out


def decode(step_logits, pads, W, T, flags, ntok, sos, sep, eos, follows, stop="all"):
    """The whole rule as a loop over G = len(pads) wireframes.  step_logits(prefixes [G * W, j + 1], step j) -> RAW logits [G * W, S]
    (padded keys may hold anything at or below FILL: pads decides).  -> dict(beams, dead_end [G * W, T] (zero past each beam's EOS
    and past steps), scores, fin, open [G * W], steps, counts (of `stop`), all_counts, best_counts, parents, toks, deads, gaps
    [steps][G] (margin = step + 1), rows [steps][G * W], states)."""
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
                        follows, margin=j + 1)
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


def beam_scores(base, S, W, G, seed, scenario):
    """The beams' scores of an operator case over `base` (test_sequence_constrain._operator_case with B = G * W, spg = W): distinct
    multiples of 2^-10 (fp32-exact), about one beam in six EMPTY under "mixed" (-inf; never a group's every beam).  -> [G * W]."""
    g = np.random.RandomState(seed + 77)
    sc = -(g.permutation(2 ** 13)[: G * W] + 1).astype(np.float64) * 2.0 ** -10      # (strictly negative: no signed zero among them)
    if scenario.startswith("mixed") and W > 1:
        empty = g.rand(G * W) < 1.0 / 6.0
        empty[::W] = False
        sc[empty] = NEG
    return sc


def guarantee(beams, dead, open_end, scores, W, ni, flags, ntok, sep, eos, follows, edges):
    """Guarantee (c) on every NON-EMPTY beam, asserted (sequence_constrain_sample_ref.guarantee's checks, which are per row): every
    parsed face passes the enclosure walk unless its boundary was selected at a dead end or it is the open piece of an open_end
    beam; no face holds an edge twice; under ONCE no edge occurs twice in a beam.  -> (enclosed, parsed, dead ends) over them."""
    import sequence_constrain_sample_ref as QC
    enc = par = de = 0
    for r in range(beams.shape[0]):
        if scores[r] == NEG:
            continue
        w = r // W
        e, p = QC.guarantee(beams[r:r + 1], dead[r:r + 1], open_end[r:r + 1], 1, [ni[w]], flags, ntok, sep, eos, [follows[w]],
                            None if edges is None else [edges[w]])
        enc, par, de = enc + e, par + p, de + int(np.asarray(dead[r]).astype(bool).sum())
    return enc, par, de
