"""The loop-constrained pointer decode restated in numpy, and a generator of connected co-edge wireframes.

The rule, on tokens (include/faceformer_hip.h carries the same text).  ntok = token.len; [term_lo, term_hi) =
[face_type_offset, len); edge e is token ntok + e; follows[a][b]: edge b starts where edge a ends.  State of a sequence, a
function of its prefix (column 0 included): visited (the edge tokens in the prefix), prev (the last edge), first (the first edge
of the open loop, or None).  Appending edge e: first = e if first is None; prev = e; if follows[prev][first] the loop is closed
and first = None.  Masked for an unfinished row, on top of padding: NO_REPEAT -- the visited edges; CONNECT with an open loop --
every special token and every edge b without follows[prev][b], and when no edge is left live the terminators are un-masked
instead (dead end, the sequence ends); CONNECT with a closed loop -- every special token outside the terminator range.  The
token is the argmax of the constrained row (lowest index on ties), its log-probability the log-softmax of that row.
"""
import math

import numpy as np

FILL = float(np.finfo(np.float32).min)
NO_REPEAT, CONNECT = 1, 2
LP_BAR = 2.0 ** -16          # DESIGN.md 12's bar on a log-probability against fp64 log_softmax of the kernel's own masked row
EPS = 2.0 ** -23
CAP = 0.02                   # the issue's cap on (step, sequence) pairs left out of the oracle comparison
TOL = 2e-4                   # model.constrain_tol's default: post_process.enclosedness_tol of the reference's configs
MIN_ENCLOSED = 0.1           # non-vacuity of the guarantee test: at least this share of the own-anchor rows must end enclosed under
                             # "loops".  A condition on the FIXTURE, fixed on the CPU: tools/constrained_left_out.py keeps a (golden,
                             # seed) pair only if the fp64 oracle's own constrained decode reaches TWICE this share -- an fp32
                             # decode differs from it on indecisive pairs only (at most CAP of them, one row each), which cannot
                             # halve the share

# (golden, lattice seed) pairs kept by tools/constrained_left_out.py: the fp32 oracle against the fp64 oracle along the fp64
# oracle's own constrained decode leaves at most CAP of the pairs out, and the oracle's enclosed share is above MIN_ENCLOSED
LATTICE_SEEDS = {"par_small_gain4": 1, "par_small_ragged": 1, "par_full_n40_gain4": 1}


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def start_state(tok0, ntok, follows=None):
    """(visited, first, prev) after column 0: a start token below ntok leaves the state empty."""
    return advance((frozenset(), None, None), tok0, ntok, follows)


def advance(state, tok, ntok, follows=None):
    visited, first, prev = state
    if tok < ntok:
        return state
    e = int(tok) - ntok
    if first is None:
        first = e
    prev = e
    if follows is not None and follows[prev][first]:
        first = None
    return (visited | {e}, first, prev)


def state_of_prefix(tokens, ntok, follows=None):
    st = start_state(int(tokens[0]), ntok, follows)
    for t in tokens[1:]:
        st = advance(st, int(t), ntok, follows)
    return st


def rule_mask(state, flags, S, ntok, term, follows, pad):
    """-> (masked [S] bool: the keys the RULE masks, padding not included; dead_end).  pad [S] bool: keys masked by padding /
    kv_len, which the dead-end test has to see."""
    visited, first, prev = state
    lo, hi = term
    masked = np.zeros(S, dtype=bool)
    is_open = bool(flags & CONNECT) and first is not None and prev is not None    # (either none: closed, as the header states)
    if flags & CONNECT:
        masked[:ntok] = True
        if not is_open:
            masked[lo:hi] = False
    if flags & NO_REPEAT:
        for e in visited:
            masked[ntok + e] = True
    dead = False
    if is_open:
        L = S - ntok
        masked[ntok:] |= ~np.asarray(follows[prev][:L], dtype=bool)
        if not (~masked[ntok:] & ~pad[ntok:]).any():
            dead = True
            masked[lo:hi] = False
    return masked, dead


def select(row, S=None):
    """(argmax with the lowest index on ties, log-softmax at it) of a masked fp64 row; no live key: (0, -log S)."""
    row = np.asarray(row, dtype=np.float64)
    i = int(np.argmax(row))
    return i, -math.log(np.exp(row - row[i]).sum())


def step_row(raw, pad, state, flags, ntok, term, follows, finished=False):
    """One row of one step on RAW logits.  -> dict(tok, logprob, row (masked fp64), masked (the rule's own), dead, fin, state)."""
    S = len(raw)
    if finished:
        return dict(tok=0, logprob=0.0, row=np.asarray(raw, dtype=np.float64), masked=np.zeros(S, bool), dead=False, fin=True,
                    state=state)
    masked, dead = rule_mask(state, flags, S, ntok, term, follows, pad)
    row = np.where(masked | pad, FILL, np.asarray(raw, dtype=np.float64))
    tok, lp = select(row)
    fin = dead or term[0] <= tok < term[1]
    return dict(tok=tok, logprob=lp, row=row, masked=masked, dead=dead, fin=fin, state=advance(state, tok, ntok, follows))


def stop_and_finish(tokens, term, ntok):
    """Finish positions (first position holding a terminator, column 0 included; T: none) and the stop step of [rows, T] tokens:
    the first step j >= 1 at which no row with fin >= j holds a token >= ntok, else T - 1 (faces.retired_view's rule)."""
    t = np.asarray(tokens)
    T = t.shape[1]
    hit = (t >= term[0]) & (t < term[1])
    fin = np.where(hit.any(axis=1), hit.argmax(axis=1), T)
    steps = T - 1
    for j in range(1, T):
        if not ((t[:, j] >= ntok) & (fin >= j)).any():
            steps = j
            break
    return fin, steps


def pack_bits(table):
    from faceformer_amd import faces
    return faces.pack_follow_bits(table)


# ---- connected co-edge wireframes ---------------------------------------------------------------------------------------------------
def _resample(poly, num_points):
    """A polyline resampled to num_points by arc length; point 0 and point -1 are its exact end points (as synth._segment_points
    keeps a segment's)."""
    poly = np.asarray(poly, dtype=np.float64)
    if len(poly) == 2:
        t = np.linspace(0, 1, num_points)
        out = poly[0][None, :] + (poly[1] - poly[0])[None, :] * t[:, None]
    else:
        seg = np.sqrt(((poly[1:] - poly[:-1]) ** 2).sum(axis=1))
        s = np.concatenate([[0.0], np.cumsum(seg)])
        t = np.linspace(0, s[-1], num_points)
        out = np.stack([np.interp(t, s, poly[:, 0]), np.interp(t, s, poly[:, 1])], axis=1)
    out[0], out[-1] = poly[0], poly[-1]
    return out


def lattice_edges(n, seed, h=0.25):
    """n directed co-edges: a = (n - 3 b) // 4 counter-clockwise square cells of a lattice (four co-edges each; neighbouring
    cells share corners, so a corner has up to four outgoing co-edges), b = 1 clockwise triangular inner loop inside cell 0 when
    n >= 7 (a face with two loops), and the remaining c = n - 4 a - 3 b co-edges as one-edge loops (closed curves: they close
    on themselves).  The co-edges are shuffled by `seed`.  Returns (polylines, loops): loops are lists of edge indices in
    walking order."""
    b = 1 if n >= 7 else 0
    a = (n - 3 * b) // 4
    c = n - 4 * a - 3 * b
    width = max(1, int(math.ceil(math.sqrt(max(a, 1)))))
    h = min(h, 1.5 / width)                                                  # (the lattice stays inside [-0.75, 0.75]^2)
    polys, loops = [], []
    for k in range(a):
        x0, y0 = -0.75 + h * (k % width), -0.75 + h * (k // width)
        corners = [(x0, y0), (x0 + h, y0), (x0 + h, y0 + h), (x0, y0 + h)]
        loops.append(list(range(len(polys), len(polys) + 4)))
        polys += [[corners[i], corners[(i + 1) % 4]] for i in range(4)]
    if b:
        x0, y0 = -0.75, -0.75
        tri = [(x0 + 0.25 * h, y0 + 0.25 * h), (x0 + 0.5 * h, y0 + 0.75 * h), (x0 + 0.75 * h, y0 + 0.25 * h)]   # clockwise
        loops.append(list(range(len(polys), len(polys) + 3)))
        polys += [[tri[i], tri[(i + 1) % 3]] for i in range(3)]
    for k in range(c):
        cx, cy, r = 0.5 + 0.15 * k, 0.8, 0.05
        ang = np.linspace(0.0, 2 * math.pi, 33)
        circ = [(cx + r * math.cos(t), cy + r * math.sin(t)) for t in ang]
        circ[-1] = circ[0]
        loops.append([len(polys)])
        polys.append(circ)
    perm = np.random.default_rng([0x1A77, int(seed), n]).permutation(n)      # new index i holds old edge perm[i]
    inv = np.argsort(perm)
    return [polys[j] for j in perm], [[int(inv[e]) for e in loop] for loop in loops]


def lattice_batch(num_edges, num_lines, seq_len, seed, num_points=50):
    """The batch dict of synth.make_wireframes with lattice wireframes: one of num_edges[w] co-edges per entry, padded to
    num_lines.  Also returns the per-wireframe edge lists (float32 points, as the model sees them) and loops."""
    import torch
    n_wf = len(num_edges)
    inp = np.zeros((n_wf, num_lines, num_points, 2), dtype=np.float32)
    mask = np.ones((n_wf, num_lines), dtype=bool)
    edges, loops = [], []
    for w, n in enumerate(num_edges):
        polys, lp = lattice_edges(int(n), 1000 * int(seed) + w)
        for i, poly in enumerate(polys):
            inp[w, i] = _resample(poly, num_points).astype(np.float32)
        mask[w, :n] = False
        edges.append([inp[w, i] for i in range(int(n))])
        loops.append(lp)
    batch = {"input": torch.from_numpy(inp), "input_mask": torch.from_numpy(mask),
             "label": torch.zeros((n_wf, num_lines, seq_len), dtype=torch.int64), "num_input": [int(n) for n in num_edges]}
    return batch, edges, loops


def random_follows(W, L, seed):
    """Random bit tables of out-degree 0..4: bool [W, L, L]."""
    g = np.random.default_rng([0xF011, int(seed), W, L])
    t = np.zeros((W, L, L), dtype=bool)
    for w in range(W):
        for a in range(L):
            deg = int(g.integers(0, 5))
            if deg and L:
                t[w, a, g.integers(0, L, size=deg)] = True
    return t
