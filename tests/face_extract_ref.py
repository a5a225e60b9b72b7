"""Helpers of tests/test_face_extract.py: the list functions of faceformer_amd/faces.py as the oracle of the array
forms, and a seeded generator of decoded rows -- random walks on a random follow table -- whose coverage is counted here.

The oracle reads the enclosure walk ON THE TABLE: `table_edges` builds edge objects whose end-point "coordinates" subtract to 0
where the table says "follows" and to 1 where it does not, so faces.is_face_enclosed / filter_faces_by_encloseness run as they
are, with tol = 0.5."""
from collections import Counter

import numpy as np

import constrain_ref as CR
from faceformer_amd import faces

TABLE_TOL = 0.5


class _Coord:
    def __init__(self, table, i):
        self.table, self.i = table, i

    def __sub__(self, other):            # (an end coordinate of edge i) - (a start coordinate of edge j)
        return 0.0 if self.table[self.i][other.i] else 1.0


class _Point:
    def __init__(self, table, i):
        self.c = _Coord(table, i)

    def __getitem__(self, k):
        return self.c


class _Edge:
    def __init__(self, table, i):
        self.p = _Point(table, i)

    def __getitem__(self, k):
        assert k in (0, -1)
        return self.p


def table_edges(table):
    """`edges` for is_face_enclosed such that _connects(edges[a], edges[b], 0.5) == table[a][b]."""
    return [_Edge(table, i) for i in range(len(table))]


def unpack_bits(words, L):
    """int32 / uint32 words [..., L, ceil(L/32)] -> bool [..., L, L]."""
    w = np.asarray(words).view(np.uint32)
    bits = (w[..., :, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[:-1] + (-1,))[..., :L].astype(bool)


def oracle(tokens, num_input, token, num_edges=None, scores=None, logprob=None, dead_end=None, own_stop=False, table=None,
           edge_map=None, require_closed=False):
    """What the existing list functions make of wireframe rows, per wireframe: dict(parsed, scored, enclosed, unique,
    unique_unscored).  tokens [N, F, G, T]; table bool [N, L, L] or None.  The rows taken are the wireframe's own anchors."""
    t = np.asarray(tokens, dtype=np.int64)
    N, F, G, T = t.shape
    out = []
    for w in range(N):
        n = max(0, min(int(num_input[w]), F))
        ne = int(num_input[w] if num_edges is None else num_edges[w])
        if table is not None:
            ne = max(0, min(ne, table.shape[1]))
        rows = t[w, :n].reshape(-1, T)
        lp = None if logprob is None else np.asarray(logprob, dtype=np.float32)[w, :n].reshape(-1, T)
        if own_stop:
            if lp is not None:
                rows, lp = faces._apply_own_stop_rule_scored(rows, lp, token, True)
            else:
                rows = faces.apply_own_stop_rule(rows, token, True)
        sc = np.zeros(rows.shape[0], np.float64)
        if scores is not None:
            sc = np.asarray(scores, dtype=np.float32)[w, :n].reshape(-1).astype(np.float64)
        if dead_end is not None:
            sc = sc.copy()
            sc[np.asarray(dead_end)[w, :n].reshape(-1) != 0] = -np.inf
        if lp is not None:
            scored = faces.parse_parallel_faces_scored(rows, lp, ne, token)
            if dead_end is not None:     # (that function has no dead-end argument: drop those rows first)
                keep = np.asarray(dead_end)[w, :n].reshape(-1) == 0
                scored = faces.parse_parallel_faces_scored(rows[keep], lp[keep], ne, token)
        else:
            scored = faces.parse_parallel_beams_scored(rows, sc, ne, token)
        parsed = [(ty, e) for ty, e, _ in scored]
        rec = {"parsed": parsed, "scored": scored}
        mapped = scored
        if table is not None:
            edges = table_edges(table[w])
            rec["enclosed"] = faces.filter_faces_by_encloseness(edges, parsed, TABLE_TOL)
            rec["is_closed"] = [bool(faces.is_face_enclosed(edges, e, TABLE_TOL)) for _, e in parsed]
            if require_closed:
                mapped = [f for f, ok in zip(scored, rec["is_closed"]) if ok]

        def m(e):
            if edge_map is None:
                return e
            v = int(edge_map[w][e])
            return v if 0 <= v < len(edge_map[w]) else e
        mapped = [(ty, tuple(m(e) for e in idx), s) for ty, idx, s in mapped]
        rec["unique"] = faces.unique_faces_with_scores(mapped)
        rec["unique_unscored"] = faces.unique_faces_with_majority_type([(ty, idx) for ty, idx, _ in mapped])
        out.append(rec)
    return out


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _walk_loop(g, tab, L, cap=6):
    """One loop as the enclosure walk reads it: from a random edge along random successors until an edge closes onto the
    first; None when it runs into an edge without successors or past `cap` edges."""
    first = int(g.integers(0, L))
    loop = [first]
    while not tab[loop[-1], first]:
        nxt = np.flatnonzero(tab[loop[-1]])
        if nxt.size == 0 or len(loop) >= cap:
            return None
        loop.append(int(g.choice(nxt)))
    return loop


def random_case(seed, N=3, L=11, F=8, G=3, T=14, ntok=4, off=1):
    """dict(tokens [N, F, G, T] int64, num_input, num_edges, scores, logprob, dead_end, table bool [N, L, L], follows (packed),
    edge_map).  Rows are closed faces put together from walked loops (in random rotations, so that equal edge sets recur),
    open random walks and random tokens, with the disturbances the parse has rules for mixed in."""
    g = np.random.default_rng([0xFACE, int(seed), N, L])
    table = CR.random_follows(N, L, seed)
    num_input = np.array([F, max(F - 3, 1), 0][:N] + [F] * max(0, N - 3), dtype=np.int32)
    num_edges = np.array([L, L - 2, L][:N] + [L] * max(0, N - 3), dtype=np.int32)
    tokens = np.zeros((N, F, G, T), dtype=np.int64)
    for w in range(N):
        tab = table[w]
        pool = [lp for lp in (_walk_loop(g, tab, L) for _ in range(40)) if lp is not None]
        faces_pool = []
        for _ in range(6):
            if pool:
                faces_pool.append([pool[int(g.integers(0, len(pool)))] for _ in range(int(g.integers(1, max(4, T // 5))))])
        for f in range(F):
            for k in range(G):
                u = g.random()
                if u < 0.6 and faces_pool:
                    face = faces_pool[int(g.integers(0, len(faces_pool)))]
                    seq = []
                    for lp in face:
                        r = int(g.integers(0, len(lp))) if g.random() < 0.5 else 0
                        lp = lp[r:] + lp[:r]
                        if len(lp) >= 3 and g.random() < 0.08:
                            lp = [lp[0], lp[-1]]                       # (the closing edge right behind the first)
                        seq += lp
                elif u < 0.8:
                    seq = [int(g.integers(0, L))]
                    for _ in range(int(g.integers(0, max(7, T // 2)))):
                        nxt = np.flatnonzero(tab[seq[-1]])
                        seq.append(int(g.choice(nxt)) if nxt.size and g.random() < 0.9 else int(g.integers(0, L)))
                else:
                    seq = [int(x) for x in g.integers(0, L, size=int(g.integers(0, 6)))]
                row = [ntok + e for e in seq][: T - 2]
                if g.random() < 0.12:
                    row.insert(int(g.integers(0, len(row) + 1)), ntok + L + int(g.integers(0, 3)))      # beyond every edge
                if g.random() < 0.12 and len(row) >= 2 and off > 0:
                    row.insert(int(g.integers(1, len(row))), int(g.integers(0, off)))                    # special, below off
                row = row[: T - 1]
                if g.random() < 0.06:
                    row = [off + int(g.integers(0, ntok - off))] + row                                  # terminator at 0
                if g.random() < 0.9:
                    row.append(off + int(g.integers(0, 2 if g.random() < 0.8 else ntok - off)))
                    row += [int(x) for x in g.integers(0, ntok + L, size=T)]                            # (never read)
                else:
                    row += [ntok + int(x) for x in g.integers(0, L, size=T)]                            # no terminator
                tokens[w, f, k] = row[:T]
    scores = g.standard_normal((N, F, G)).astype(np.float32) * 3
    scores[g.random((N, F, G)) < 0.06] = -np.inf
    logprob = -np.abs(g.standard_normal((N, F, G, T))).astype(np.float32)
    logprob[..., 0] = 0
    dead_end = (g.random((N, F, G)) < 0.06).astype(np.int32) * int(g.integers(1, 5))
    edge_map = np.tile(np.arange(L, dtype=np.int32), (N, 1))
    for w in range(N):
        for e in g.choice(L, size=max(1, L // 4), replace=False):
            edge_map[w, e] = int(g.integers(-1, L + 1))                 # (-1 and L: outside, read as the edge itself)
    return dict(tokens=tokens, num_input=num_input, num_edges=num_edges, scores=scores, logprob=logprob, dead_end=dead_end,
                table=table, follows=faces.pack_follow_bits(table), edge_map=edge_map)


COVERAGE = ("multi_loop_closed", "self_closing_edge", "repeated_edge", "connect_failure_at_closure", "token_beyond_edges",
            "special_below_off_mid_row", "terminator_at_0", "no_terminator", "neg_inf_score", "dead_end", "padding_anchor",
            "same_set_other_rotation", "type_tie_in_group", "group_of_3")


def coverage(case, token, ntok=4, off=1):
    """Counter over COVERAGE, plus `rows` (own-anchor rows) and `closed` (enclosed ones): what the generator produced, counted
    with code of its own (no function under test)."""
    c = Counter()
    t = case["tokens"]
    N, F, G, T = t.shape
    for w in range(N):
        tab, ne, n = case["table"][w], int(case["num_edges"][w]), int(case["num_input"][w])
        groups = {}
        for f in range(F):
            for k in range(G):
                if f >= n:
                    c["padding_anchor"] += 1
                    continue
                c["rows"] += 1
                row = [int(x) for x in t[w, f, k]]
                if case["scores"][w, f, k] == -np.inf:
                    c["neg_inf_score"] += 1
                if case["dead_end"][w, f, k]:
                    c["dead_end"] += 1
                term = [j for j, x in enumerate(row) if off <= x < ntok]
                fin = term[0] if term else T - 1
                c["no_terminator"] += not term
                c["terminator_at_0"] += bool(term) and term[0] == 0
                pre = row[: fin + 1]
                e = [x - ntok for x in pre if 0 <= x - ntok < ne]
                if not e:
                    continue
                c["token_beyond_edges"] += any(x - ntok >= ne for x in pre)
                c["special_below_off_mid_row"] += any(x < off for x in pre[1:-1])
                c["repeated_edge"] += len(set(e)) < len(e)
                first, loops, ok, cur = None, [], True, []
                for i, x in enumerate(e):
                    if first is None:
                        first = x
                    elif not tab[e[i - 1], x]:
                        c["connect_failure_at_closure"] += bool(tab[x, first])
                        ok = False
                        break
                    cur.append(x)
                    if tab[x, first]:
                        loops.append(cur)
                        cur, first = [], None
                ok = ok and first is None
                if ok:
                    c["closed"] += 1
                    c["multi_loop_closed"] += len(loops) >= 2
                    c["self_closing_edge"] += any(len(lp) == 1 for lp in loops)
                if case["scores"][w, f, k] != -np.inf and not case["dead_end"][w, f, k]:
                    groups.setdefault(tuple(sorted(set(e))), []).append((tuple(e), row[fin] - off))
        for members in groups.values():
            c["group_of_3"] += len(members) >= 3
            top = Counter(ty for _, ty in members).most_common(2)
            c["type_tie_in_group"] += len(top) == 2 and top[0][1] == top[1][1]
            seqs = sorted(set(s for s, _ in members))
            c["same_set_other_rotation"] += any(a != b and len(a) == len(b) and any(a[r:] + a[:r] == b for r in range(1, len(a)))
                                                for i, a in enumerate(seqs) for b in seqs[i + 1:])
    return c
