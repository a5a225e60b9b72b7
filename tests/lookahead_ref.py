"""The closure look-ahead of the loop-constrained pointer decode in numpy, composed from constrain_ref: the rule of
DESIGN.md 16 with one more mask in front of the dead-end vote.

The step that selects position p has budget = T - 1 - p.  Under CONNECT an edge b is also masked when close_dist[first][b] >
budget (loop open) or cycle_len[b] > budget (loop closed); the dead-end vote then sees padding, visited and the look-ahead.
close_dist [L, L] / cycle_len [L] uint8 are one wireframe's (faces.follow_distance).  Everything else is constrain_ref's.
"""
import numpy as np

import constrain_ref as CR

# Non-vacuity of the guarantee test (a condition on the FIXTURE, fixed on the CPU by tools/lookahead_left_out.py): at least this
# share of the own-anchor rows must end enclosed under the look-ahead.  The fp64 oracle alone reaches 75.8 %, 81.3 % and 85.0 % on
# the three lattice fixtures, more than twice this; an fp32 decode differs from it on indecisive pairs only (at most CR.CAP of
# them, one row each), which cannot halve the share.
MIN_ENCLOSED = 0.35


def rule_mask(state, flags, S, ntok, term, follows, pad, close_dist, cycle_len, budget):
    """constrain_ref.rule_mask with the look-ahead.  -> (masked [S] bool, dead_end)."""
    masked, dead = CR.rule_mask(state, flags, S, ntok, term, follows, pad)
    if not flags & CR.CONNECT:
        return masked, dead
    _, first, prev = state
    is_open = first is not None and prev is not None
    L = S - ntok
    dist = np.asarray(close_dist[first] if is_open else cycle_len)[:L].astype(np.int64)
    masked = masked.copy()
    masked[ntok:] |= dist > int(budget)
    # (a dead end of DESIGN.md 16's masks stays one: the look-ahead only masks more edges)
    if is_open and not dead and not (~masked[ntok:] & ~pad[ntok:]).any():
        dead = True
        masked[term[0]:term[1]] = False
    return masked, dead


def step_row(raw, pad, state, flags, ntok, term, follows, close_dist, cycle_len, budget, finished=False):
    """constrain_ref.step_row under the look-ahead: the same dict."""
    if finished:
        return CR.step_row(raw, pad, state, flags, ntok, term, follows, finished=True)
    masked, dead = rule_mask(state, flags, len(raw), ntok, term, follows, pad, close_dist, cycle_len, budget)
    row = np.where(masked | pad, CR.FILL, np.asarray(raw, dtype=np.float64))
    tok, lp = CR.select(row)
    fin = dead or term[0] <= tok < term[1]
    return dict(tok=tok, logprob=lp, row=row, masked=masked, dead=dead, fin=fin, state=CR.advance(state, tok, ntok, follows))


def ring(L, n=None):
    """bool [L, L]: edges 0 -> 1 -> ... -> n - 1 -> 0 (n = L by default)."""
    n = L if n is None else n
    t = np.zeros((L, L), dtype=bool)
    for i in range(n):
        t[i, (i + 1) % n] = True
    return t


def chain(L, n=None):
    """bool [L, L]: edges 0 -> 1 -> ... -> n - 1, open."""
    t = ring(L, n)
    n = L if n is None else n
    if n:
        t[n - 1, 0] = False
    return t


def brute_distance(table, hmax, n=None):
    """faces.follow_distance of ONE table by walking: a breadth-first search from every source over adjacency lists."""
    table = np.asarray(table, dtype=bool)
    L = table.shape[-1]
    n = L if n is None else max(0, min(int(n), L))
    succ = [[int(y) for y in np.flatnonzero(table[x]) if y < n] for x in range(L)]
    dist = np.full((L, L), 255, dtype=np.uint8)
    for b in range(n):
        front, seen = [b], set()
        for h in range(1, hmax + 1):
            nxt = {y for x in front for y in succ[x]} - seen
            if not nxt:
                break
            for y in nxt:
                dist[b, y] = h
            seen |= nxt
            front = sorted(nxt)
    return np.ascontiguousarray(dist.T), np.diagonal(dist).copy()
