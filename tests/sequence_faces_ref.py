"""Helpers of tests/test_sequence_faces.py: a seeded generator of single-sequence rows -- faces walked on a random
follow table and joined by SEP, with every disturbance the parse has a rule for -- whose coverage is counted here with code of
its own, and the list functions of faceformer_amd/faces.py as the oracle of the array forms.

The enclosure walk of the oracle is read ON THE TABLE through face_extract_ref.table_edges (tol = 0.5), as in DESIGN.md 27."""
from collections import Counter

import numpy as np

import constrain_ref as CR
import face_extract_ref as FR
from faceformer_amd import faces

NTOK, SEP, EOS = 4, 2, 3
KINDS = ("plain", "no_sep_no_eos", "eos_at_0", "eos_at_1", "sep_runs", "sep_at_last", "all_sep", "half_one_edge_faces",
         "boundary_63_64_65", "unterminated", "unfinished_zeros", "unfinished_interior_zeros", "neg_inf_score", "strange_tokens",
         "dup_rotation", "dup_permutation", "dup_open_and_closed", "map_merges", "multi_loop")
COVERAGE = ("no_sep_no_eos", "eos_at_0", "eos_at_1", "sep_run", "sep_at_last", "all_sep", "one_piece_fills_row", "half_one_edge_faces",
            "boundary_63", "boundary_64", "boundary_65", "unterminated_loses_edge", "unfinished_zeros", "unfinished_interior_zeros",
            "neg_inf_score", "negative_token", "token_beyond_edges", "token_above_2_31", "dup_rotation", "dup_permutation",
            "dup_open_and_closed", "map_merges", "multi_loop_closed")


def _loops(g, tab, L, want):
    out = []
    for _ in range(200):
        lp = FR._walk_loop(g, tab, L)
        if lp is not None and len(set(lp)) == len(lp):
            out.append(lp)
            if len(out) == want:
                break
    return out


def _join(pieces, T, end=EOS):
    row = []
    for p in pieces:
        row += [NTOK + e for e in p] + [SEP]
    if end is not None and row:
        row[-1] = end
    return row[:T]


def random_case(seed, N=3, G=3, T=40, L=11):
    """dict(tokens [N, G, T] int64, num_edges, scores [N, G], logprob [N, G, T], finished [N, G], table bool [N, L, L], follows
    (packed), edge_map [N, L], kinds [N, G]).  The kind of row (w, g) is KINDS[(seed + w * G + g) % len(KINDS)]; the last wireframe
    of a batch of three or more has no edges."""
    g = np.random.default_rng([0x5E9, int(seed), N, G, T, L])
    table = CR.random_follows(N, L, seed)
    num_edges = np.full(N, L, dtype=np.int32)
    if N >= 2:
        num_edges[1] = max(L - 2, 1)
    if N >= 3:
        num_edges[N - 1] = 0
    tokens = np.zeros((N, G, T), dtype=np.int64)
    finished = np.ones((N, G), dtype=np.int32)
    scores = (g.standard_normal((N, G)) * 3).astype(np.float32)
    kinds = np.empty((N, G), dtype=object)
    edge_map = np.tile(np.arange(L, dtype=np.int32), (N, 1))
    edge_map[:, 1::2] -= 1                                       # (co-edge pairs 2k, 2k + 1 -> 2k)
    edge_map[:, L - 1] = L if L % 2 else -1                      # (outside: read as the edge itself)
    for w in range(N):
        tab, ne = table[w], int(num_edges[w])
        pool = _loops(g, tab, max(ne, 1), 12) or [[0]]
        for k in range(G):
            kind = KINDS[(seed + w * G + k) % len(KINDS)]
            kinds[w, k] = kind
            rnd = lambda n: [int(x) for x in g.integers(0, max(ne, 1), size=n)]
            pick = lambda: list(pool[int(g.integers(0, len(pool)))])
            rot = lambda lp: lp[(r := int(g.integers(0, len(lp)))):] + lp[:r]
            some = [rot(pick()) if g.random() < 0.7 else rnd(int(g.integers(1, 6))) for _ in range(int(g.integers(1, max(2, T // 6))))]
            tail = [int(x) for x in g.integers(0, NTOK + L, size=T)]              # (behind EOS: never read)
            if kind == "plain":
                row = _join(some, T) + tail
            elif kind == "no_sep_no_eos":
                row = [NTOK + e for e in rnd(T)]
            elif kind == "eos_at_0":
                row = [EOS] + _join(some, T) + tail
            elif kind == "eos_at_1":
                row = [NTOK + rnd(1)[0], EOS] + _join(some, T) + tail
            elif kind == "sep_runs":
                row = []
                for p in some:
                    row += [NTOK + e for e in p] + [SEP] * int(g.integers(2, 4))
                row = [SEP] + row + [EOS] + tail
            elif kind == "sep_at_last":
                row = (_join(some, T, end=SEP) + [NTOK + e for e in rnd(T)])[: T - 1] + [SEP]
            elif kind == "all_sep":
                row = [SEP] * T
            elif kind == "half_one_edge_faces":
                row = [x for e in rnd(T // 2) for x in (NTOK + e, SEP)] + [NTOK + rnd(1)[0]]
            elif kind == "boundary_63_64_65":
                row = [NTOK + e for e in rnd(T)]
                for p in (63, 64, 65):
                    if p < T:
                        row[p] = SEP
                if T > 70:
                    row[70:] = [EOS] + tail
            elif kind == "unterminated":
                row = _join(some, T, end=SEP) + [NTOK + e for e in rnd(T)]
            elif kind == "unfinished_zeros":
                row, finished[w, k] = [0] * T, 0
            elif kind == "unfinished_interior_zeros":
                row = _join(some, max(T - 4, 1), end=None)
                if len(row) >= 3:
                    row[len(row) // 2] = 0
                row, finished[w, k] = row + [0] * T, 0
            elif kind == "neg_inf_score":
                row, scores[w, k] = _join(some, T) + tail, -np.inf
            elif kind == "strange_tokens":
                row = _join(some, max(T - 3, 1))
                for bad in (-int(g.integers(1, 50)), NTOK + ne + int(g.integers(0, 3)), (1 << 31) + NTOK + int(g.integers(0, max(ne, 1))),
                            (1 << 32) + NTOK):
                    row.insert(int(g.integers(0, max(len(row) - 1, 1))), bad)
                row = row[: T - 1] + [EOS] + tail if len(row) >= T else row + tail
            elif kind == "dup_rotation":
                lp = max(pool, key=len)
                row = _join([lp, some[0], lp[1:] + lp[:1], lp], T) + tail
            elif kind == "dup_permutation":
                lp = rnd(4)
                row = _join([lp, lp[::-1], some[0], [lp[1], lp[0]] + lp[2:]], T) + tail
            elif kind == "dup_open_and_closed":
                lp = max(pool, key=len)
                row = _join([lp[::-1] if len(lp) > 2 else lp + lp, lp, some[0]], T) + tail
            elif kind == "map_merges":
                e = 2 * int(g.integers(0, max(ne // 2, 1)))
                row = _join([[e], some[0], [e + 1] if e + 1 < ne else [e]], T) + tail
            else:   # multi_loop
                row = _join([pick() + pick() + pick(), some[0], pick() + pick()], T) + tail
            row = (row + [0] * T)[:T]
            tokens[w, k] = row
    logprob = -np.abs(g.standard_normal((N, G, T))).astype(np.float32)
    logprob[..., 0] = 0
    return dict(tokens=tokens, num_edges=num_edges, scores=scores, logprob=logprob, finished=finished, table=table,
                follows=faces.pack_follow_bits(table), edge_map=edge_map, kinds=kinds)


def _split(row, ne, finished=True):
    """Own restatement for the coverage counts: (end, [(first, last, [edge, ...])] of every piece), or None for an unfinished
    row of zeros."""
    T = len(row)
    end = T - 1
    if not finished:
        nz = [p for p, x in enumerate(row) if x != 0]
        if not nz:
            return None
        end = nz[-1]
    for p in range(end + 1):
        if row[p] == EOS:
            end = p
            break
    pieces, first = [], 0
    for p in range(end + 1):
        if row[p] == SEP or p == end:
            pieces.append((first, p, [x - NTOK for x in row[first:p] if 0 <= x - NTOK < ne]))
            first = p + 1
    return end, pieces


def _closed(e, tab):
    first, prev = None, None
    loops = 0
    for x in e:
        if first is None:
            first = x
        elif not tab[prev, x]:
            return 0
        prev = x
        if tab[x, first]:
            first, loops = None, loops + 1
    return loops if first is None else 0


def coverage(case):
    """Counter over COVERAGE: what the generator produced, counted with code of its own (no function under test)."""
    c = Counter()
    t = case["tokens"]
    N, G, T = t.shape
    L = case["table"].shape[1]
    for w in range(N):
        ne, tab, emap = int(case["num_edges"][w]), case["table"][w], case["edge_map"][w]
        for k in range(G):
            row = [int(x) for x in t[w, k]]
            c["neg_inf_score"] += case["scores"][w, k] == -np.inf
            fin = bool(case["finished"][w, k])
            got = _split(row, ne, fin)
            if got is None:
                c["unfinished_zeros"] += 1
                continue
            end, pieces = got
            read = row[: end + 1]
            c["unfinished_interior_zeros"] += (not fin) and 0 in read
            c["no_sep_no_eos"] += SEP not in row and EOS not in row
            c["eos_at_0"] += row[0] == EOS
            c["eos_at_1"] += row[0] != EOS and row[1:2] == [EOS]
            c["sep_run"] += any(a == SEP and b == SEP for a, b in zip(read, read[1:])) and not all(x == SEP for x in row)
            c["sep_at_last"] += end == T - 1 and row[T - 1] == SEP and not all(x == SEP for x in row)
            c["all_sep"] += all(x == SEP for x in row)
            c["one_piece_fills_row"] += len(pieces) == 1 and pieces[0][:2] == (0, T - 1) and T > 1
            faces_ = [e for _, _, e in pieces if e]
            c["half_one_edge_faces"] += T >= 2 and len(faces_) == T // 2 and all(len(e) == 1 for e in faces_)
            for p in (63, 64, 65):
                c["boundary_%d" % p] += p <= end and (row[p] == SEP or p == end)
            c["unterminated_loses_edge"] += row[end] not in (SEP, EOS) and 0 <= row[end] - NTOK < ne
            c["negative_token"] += any(x < 0 for x in read)
            c["token_beyond_edges"] += any(NTOK + ne <= x < (1 << 31) for x in read)
            c["token_above_2_31"] += any(x >= (1 << 31) for x in read)
            c["multi_loop_closed"] += any(_closed(e, tab) > 1 for e in faces_)
            m = lambda x: int(emap[x]) if 0 <= int(emap[x]) < L else x
            for i, a in enumerate(faces_):
                for b in faces_[:i]:
                    if set(a) == set(b) and a != b:
                        rots = any(a[r:] + a[:r] == b for r in range(1, len(a))) if len(a) == len(b) else False
                        c["dup_rotation"] += rots
                        c["dup_permutation"] += not rots
                        c["dup_open_and_closed"] += bool(_closed(a, tab)) != bool(_closed(b, tab))
                    if set(a) != set(b) and {m(x) for x in a} == {m(x) for x in b}:
                        c["map_merges"] += 1
    return c


# ---- the oracle: the list functions ------------------------------------------------------------------------------------------------
def mapped(idx, emap):
    L = len(emap)
    return tuple(int(emap[e]) if 0 <= int(emap[e]) < L else int(e) for e in idx)


def enclosed_and_mapped(parsed, table, emap):
    """faces.postprocess_faces on the table: the enclosure filter, the loops flattened, the co-edges mapped (pairings = the map
    as a dict of strings, the form the data set's JSON has)."""
    pairings = {str(i): int(v) for i, v in enumerate(emap) if 0 <= int(v) < len(emap) and int(v) != i}
    return faces.postprocess_faces(parsed, FR.table_edges(table), pairings, FR.TABLE_TOL)
