"""The exact closure look-ahead of the loop-constrained pointer decode in numpy, composed from constrain_ref and
lookahead_ref: the rule of DESIGN.md 16 under NO_REPEAT | CONNECT with one more mask in front of the dead-end vote.

The step that selects position p has budget = T - 1 - p.  With the loop open an edge b is also masked when D_V(b -> first) >
budget (faces.closure_distance: the least number of hops from b to the loop's first edge through edges that are neither visited
nor padded); with it closed when cycle_len[b] > budget, DESIGN.md 22's static rule.  The dead-end vote then sees padding, visited
and this mask.  cycle_len [L] uint8 is one wireframe's (faces.follow_distance).  Everything else is constrain_ref's.
"""
import numpy as np

import constrain_ref as CR
from faceformer_amd import faces

LOOPS = CR.NO_REPEAT | CR.CONNECT

# (golden, lattice seed) pairs kept by tools/exact_left_out.py (profiles/exact/left_out.txt): the fp32 oracle against the fp64
# oracle along the fp64 oracle's own exact decode leaves no pair out; under the static look-ahead the fp64 oracle has a late dead
# end, under the exact rule none and strictly more rows enclosed.  STRICT: the fixtures on which the tool found strictly more.
LATTICE_SEEDS = dict(CR.LATTICE_SEEDS)
STRICT = ("par_small_gain4", "par_small_ragged", "par_full_n40_gain4")

# The hand-written trap: edges 0 -> 1, 1 -> 2, 1 -> 3, 2 -> 0, 3 -> 1.  With first = 0, prev = 1 and visited = {0, 1} the static
# distance D(3 -> 0) = 3 (through the visited edge 1) leaves edge 3 live; no path from 3 avoids edge 1, so the exact rule masks it.
TRAP_EDGES = ((0, 1), (1, 2), (1, 3), (2, 0), (3, 1))


def trap(L=4):
    t = np.zeros((L, L), dtype=bool)
    if L >= 4:
        for a, b in TRAP_EDGES:
            t[a, b] = True
    return t


def self_closing(L):
    """An open chain with every third edge closing on itself."""
    from lookahead_ref import chain
    t = chain(L)
    t[np.arange(0, L, 3), np.arange(0, L, 3)] = True
    return t


def closing_distance(state, follows, pad_edges, hmax=254):
    """D_V(b -> first) [L] uint8 of an open state (faces.closure_distance on the state's visited set and the padded edges)."""
    visited, first, _ = state
    L = len(pad_edges)
    v = np.zeros(L, dtype=bool)
    v[sorted(visited)] = True
    return faces.closure_distance(np.asarray(follows)[:L, :L], v, first, hmax=hmax, pad=pad_edges)


def rule_mask(state, S, ntok, term, follows, pad, cycle_len, budget):
    """constrain_ref.rule_mask under LOOPS with the exact look-ahead.  -> (masked [S] bool, dead_end)."""
    masked, dead = CR.rule_mask(state, LOOPS, S, ntok, term, follows, pad)
    _, first, prev = state
    is_open = first is not None and prev is not None
    L = S - ntok
    if is_open:
        dist = closing_distance(state, follows, pad[ntok:], hmax=min(max(int(budget), 1), 254)).astype(np.int64)
    else:
        dist = np.asarray(cycle_len)[:L].astype(np.int64)
    masked = masked.copy()
    masked[ntok:] |= dist > int(budget)
    if is_open and not dead and not (~masked[ntok:] & ~pad[ntok:]).any():
        dead = True
        masked[term[0]:term[1]] = False
    return masked, dead


def step_row(raw, pad, state, ntok, term, follows, cycle_len, budget, finished=False):
    """constrain_ref.step_row under the exact look-ahead: the same dict."""
    if finished:
        return CR.step_row(raw, pad, state, LOOPS, ntok, term, follows, finished=True)
    masked, dead = rule_mask(state, len(raw), ntok, term, follows, pad, cycle_len, budget)
    row = np.where(masked | pad, CR.FILL, np.asarray(raw, dtype=np.float64))
    tok, lp = CR.select(row)
    fin = dead or term[0] <= tok < term[1]
    return dict(tok=tok, logprob=lp, row=row, masked=masked, dead=dead, fin=fin, state=CR.advance(state, tok, ntok, follows))


def can_close(table, avail, first, b, budget):
    """Exhaustive depth-first search: is there a simple continuation b = x_0, x_1, ... of at most `budget` hops whose last edge
    is followed by `first`, every x_i behind b available and none used twice?"""
    table = np.asarray(table, dtype=bool)

    def go(x, used, left):
        if left < 1:
            return False
        if table[x, first]:
            return True
        return any(go(int(y), used | {int(y)}, left - 1) for y in np.flatnonzero(table[x]) if avail[y] and int(y) not in used)
    return go(int(b), {int(b)}, int(budget))


def walk_states(table, start, steps, rng, ntok=0):
    """The states of a random walk of the "loops" rule from anchor edge `start`: a random live edge per step (no padding), until
    a dead end or `steps` edges.  -> [(visited, first, prev)], the state after column 0 first."""
    table = np.asarray(table, dtype=bool)
    L = table.shape[0]
    st = CR.start_state(ntok + int(start), ntok, table)
    out = [st]
    nopad = np.zeros(ntok + L, dtype=bool)
    for _ in range(steps):
        masked, dead = CR.rule_mask(st, LOOPS, ntok + L, ntok, (0, max(ntok, 1)), table, nopad)
        live = np.flatnonzero(~masked[ntok:])
        if dead or not live.size:
            break
        st = CR.advance(st, ntok + int(rng.choice(live)), ntok, table)
        out.append(st)
    return out


def late_dead_ends(tokens, dead, ntok, follows):
    """Of the rows [rows, T] flagged `dead`: those whose dead end is LATE -- raised at a position whose previous position did not
    open the current loop.  The state is replayed from the tokens (the row's last edge token is the last one before the dead
    end); a row without an edge cannot be flagged.  -> the row indices."""
    late = []
    for r in np.flatnonzero(np.asarray(dead)):
        row = [int(t) for t in tokens[r]]
        at = [j for j, t in enumerate(row) if t >= ntok]
        if not at:
            continue
        last = at[-1]                                                      # the position of the last edge: the dead end is raised behind it
        before = CR.state_of_prefix(row[:last], ntok, follows) if last > 0 else (frozenset(), None, None)
        if before[1] is not None:                                          # a loop was open already: position `last` did not open it
            late.append(int(r))
    return late
