"""Opt-in device-side face extraction (ff_face_rows / ff_face_votes, model.extract_faces, --device-faces).

CPU: header / binding / build agree; the numpy restatements faces.face_rows / face_votes / faces_of_rows reproduce the reference's
recorded results (tests/golden/faces_cases.json) and, on seeded random rows whose coverage is asserted, the existing list
functions; every rejection is raised before the library is touched.  GPU: both entries bit for bit against the restatements,
inside poisoned surroundings, FF_ERR_ARG before any launch, the model option on the goldens, the CLI flag against no flag.

Everything is integer-exact except the fp64 score summed from fp32 log-probabilities: the kernel adds one by one in ascending
order, and a sequential fp64 sum of n terms is within n * 2^-52 * sum|x| of the exact sum (math.fsum) -- the bound used here,
with n = T."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import constrain_ref as CR
import face_extract_ref as FR
from conftest import GOLDEN, ROOT, token_ns
from faceformer_amd import faces

TOK = token_ns()
NTOK, OFF = TOK.len, TOK.face_type_offset
ROW_KEYS = ("len", "type", "closed", "loops", "edges", "loop_of", "set_bits", "score")
VOTE_KEYS = ("rep", "votes", "best", "major", "num_faces")
ENTRIES = {"ff_face_rows": 25, "ff_face_votes_workspace_bytes": 2, "ff_face_votes": 17}
SEEDS = tuple(range(1, 13))


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(GOLDEN, "faces_cases.json")) as f:
        return json.load(f)


# ---- 1. header, binding and build ----------------------------------------------------------------------------------------------------
def test_header_binding_and_build_agree():
    from faceformer_amd.hip import build, lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    assert "device-side face extraction behind the parallel decode (opt-in; entries added within ABI 105; DESIGN.md 27)" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in ENTRIES.items():
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        assert args.count(",") + 1 == nargs == len(lib.SIGNATURES[name][1]), name
    for macro, value in (("FF_FACE_OWN_STOP", 1), ("FF_FACE_REQUIRE_CLOSED", 1), ("FF_FACE_MAX_T", 256), ("FF_FACE_MAX_ROWS", 65536)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code) and getattr(lib, macro) == value
    assert faces.FACE_MAX_T == lib.FF_FACE_MAX_T and faces.FACE_MAX_ROWS == lib.FF_FACE_MAX_ROWS
    assert "ff_faces.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_faces.hip"))


def test_a_library_without_the_entries_is_refused(monkeypatch):
    from faceformer_amd.hip import lib
    import _ctypes
    assert all(name in lib.SIGNATURES for name in ENTRIES)
    monkeypatch.setattr(lib, "LIB_PATH", _ctypes.__file__)
    monkeypatch.setattr(lib, "_lib", None)
    with pytest.raises(lib.HipExtensionError, match="rebuild"):
        lib.load()


# ---- 2. the numpy restatement against the reference's recorded results ------------------------------------------------------------
def _rows_of_faces(face_list, T=None):
    """Token rows [1, F, 1, T] of faces [(type, (edge, ...))]: the edge tokens, then the terminator."""
    T = T or max(len(e) for _, e in face_list) + 1
    t = np.zeros((1, len(face_list), 1, T), dtype=np.int64)
    for f, (ty, e) in enumerate(face_list):
        t[0, f, 0, : len(e) + 1] = [NTOK + int(x) for x in e] + [OFF + int(ty)]
    return t


def _canonical(loops):
    rolled = [tuple(int(x) for x in np.roll(lp, -int(np.argmin(lp)))) for lp in loops]
    return tuple(sorted(rolled, key=lambda lp: lp[0]))


def _fixture_enclosed(cases):
    """The enclosed / filter fixtures as (tokens, table words, num_edges, expected `enclosed` list) per case, with the
    precondition the issue states: the float32 table walk equals the recorded float64 walk on every `enclosed` case."""
    out = []
    stats = {"closed": 0, "multi": 0}
    for c in cases["enclosed"]:
        if any(isinstance(i, (list, tuple)) for i in c["face"]):
            continue                                                        # (oriented items are out of scope)
        table = faces.follow_table(c["edges"], c["tol"])
        want = c["result"]
        walked = faces.is_face_enclosed(FR.table_edges(table), c["face"], FR.TABLE_TOL)
        assert (walked is False and want is False) or [list(lp) for lp in walked] == want, "float32 table walk != recorded walk"
        if want:
            stats["closed"] += 1
            stats["multi"] += len(want) > 1
        face = [(1, tuple(c["face"]))]
        out.append((_rows_of_faces(face), faces.pack_follow_bits(table)[None], len(c["edges"]),
                    [(1, _canonical(want))] if want else []))
    assert len(out) == 33 and stats == {"closed": 21, "multi": 4}, (len(out), stats)
    for c in cases["filter"]:
        table = faces.follow_table(c["edges"], c["tol"])
        face = [(int(t), tuple(f)) for t, f in c["faces"]]
        out.append((_rows_of_faces(face), faces.pack_follow_bits(table)[None], len(c["edges"]),
                    [(t, tuple(tuple(lp) for lp in loops)) for t, loops in c["result"]]))
    assert len(out) == 39
    return out


def test_restatement_reproduces_the_recorded_parallel_faces(cases):
    assert len(cases["parallel"]) == 17
    for c in cases["parallel"]:
        pred = np.asarray(c["predicts"], dtype=np.int64)
        rows = faces.face_rows(pred[None], [pred.shape[0]], TOK, num_edges=[c["num_edges"]], num_lines=c["num_edges"])
        got = faces.faces_of_rows(rows, faces.face_votes(rows), 0)
        want = [(int(t), tuple(int(i) for i in idx)) for t, idx in c["pred_faces"]]
        assert got["parsed"] == want
        assert [(t, k) for t, k, _, _ in got["unique"]] == faces.unique_faces_with_majority_type(want)
        assert (rows["closed"] == -1).all() and (rows["loops"] == 0).all() and (rows["loop_of"] == -1).all()


def test_restatement_reproduces_the_recorded_enclosed_and_filter_results(cases):
    for tokens, words, ne, want in _fixture_enclosed(cases):
        rows = faces.face_rows(tokens, [tokens.shape[1]], TOK, num_edges=[ne], follows=words)
        got = faces.faces_of_rows(rows, faces.face_votes(rows, require_closed=True), 0)
        assert got["enclosed"] == want
        assert int(faces.face_votes(rows, require_closed=True)["num_faces"][0]) == len({tuple(sorted(set(x for lp in l for x in lp)))
                                                                                        for _, l in want})


# ---- 3. seeded random rows against the existing list functions -------------------------------------------------------------------
OPERANDS = {"plain": {}, "scores": {"scores", "dead_end"}, "logprob_own_stop": {"logprob", "own_stop"},
            "logprob_all": {"logprob", "dead_end", "num_edges", "edge_map", "own_stop"}}


def _kwargs(case, names):
    kw = {k: case[k] for k in names if k != "own_stop"}
    kw["own_stop"] = "own_stop" in names
    return kw


def _same_scored(got, want, bar):
    assert [(t, e) for t, e, _ in got] == [(t, e) for t, e, _ in want]
    for (_, _, a), (_, _, b) in zip(got, want):
        assert a == b or abs(a - b) <= bar, (a, b, bar)


def test_generator_coverage():
    from collections import Counter
    total = Counter()
    for seed in SEEDS:
        total += FR.coverage(FR.random_case(seed), TOK)
    for name in FR.COVERAGE:
        assert total[name] >= 5, (name, total[name])
    assert total["closed"] >= 0.2 * total["rows"], (total["closed"], total["rows"])


@pytest.mark.parametrize("operands", sorted(OPERANDS))
def test_restatement_equals_the_list_functions_on_random_rows(operands):
    for seed in SEEDS:
        case = FR.random_case(seed)
        kw = _kwargs(case, OPERANDS[operands])
        T = case["tokens"].shape[-1]
        bar = T * 2.0 ** -52 * float(np.abs(case["logprob"].astype(np.float64)).sum(axis=-1).max())
        for walk, require_closed in ((False, False), (True, False), (True, True)):
            rows = faces.face_rows(case["tokens"], case["num_input"], TOK, follows=case["follows"] if walk else None,
                                   num_lines=case["table"].shape[1], **kw)
            votes = faces.face_votes(rows, require_closed=require_closed)
            want = FR.oracle(case["tokens"], case["num_input"], TOK, table=case["table"] if walk else None,
                             require_closed=require_closed, **kw)
            for w in range(case["tokens"].shape[0]):
                got = faces.faces_of_rows(rows, votes, w)
                assert [t for t, _ in got["parsed"]] == [t for t, _ in want[w]["parsed"]]
                if walk:
                    assert got["enclosed"] == want[w]["enclosed"]
                    open_rows = [f for f, ok in zip(got["parsed"], want[w]["is_closed"]) if not ok]
                    assert open_rows == [f for f, ok in zip(want[w]["parsed"], want[w]["is_closed"]) if not ok]
                else:
                    _same_scored(got["scored"], want[w]["scored"], bar)
                assert [u[:2] + u[3:] for u in got["unique"]] == [u[:2] + u[3:] for u in want[w]["unique"]]
                assert [u[:2] for u in got["unique"]] == want[w]["unique_unscored"]
                for a, b in zip(got["unique"], want[w]["unique"]):
                    assert a[2] == b[2] or abs(a[2] - b[2]) <= bar


def test_own_stop_is_the_list_rule():
    for seed in SEEDS[:4]:
        case = FR.random_case(seed)
        rows = faces.face_rows(case["tokens"], case["num_input"], TOK, own_stop=True, num_lines=11)
        for w, n in enumerate(case["num_input"]):
            cut = faces.apply_own_stop_rule(case["tokens"][w, :n].reshape(-1, case["tokens"].shape[-1]), TOK, True)
            assert faces.faces_of_rows(rows, None, w)["parsed"] == faces._parallel_rows(cut, TOK, int(n))


# ---- 4. rejections, before the library is touched ---------------------------------------------------------------------------------
def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    return lib


def test_ops_reject_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import ops
    _untouchable(monkeypatch)
    ni = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="tokens must be a tensor"):
        ops.face_rows(torch.zeros(2, 3, dtype=torch.int64), ni, TOK)
    with pytest.raises(ValueError, match=r"1\.\.256 positions per row \(got T=257\)"):
        ops.face_rows(torch.zeros(2, 3, 1, 257, dtype=torch.int64), ni, TOK)
    with pytest.raises(ValueError, match=r"1\.\.256 positions per row \(got T=0\)"):
        ops.face_rows(torch.zeros(2, 3, 1, 0, dtype=torch.int64), ni, TOK)
    with pytest.raises(ValueError, match=r"face_type_offset=4 must be in \[0, len=4\)"):
        ops.face_rows(torch.zeros(2, 3, 5, dtype=torch.int64), ni, {"face_type_offset": 4, "len": 4})
    with pytest.raises(ValueError, match="scores and logprob may not both be given"):
        ops.face_rows(torch.zeros(2, 3, 5, dtype=torch.int64), ni, TOK, scores=torch.zeros(2, 3, 1), logprob=torch.zeros(2, 3, 1, 5))
    with pytest.raises(ValueError, match="takes the dict face_rows returns"):
        ops.face_votes({"len": torch.zeros(1, 1, 1, dtype=torch.int32)})
    big = {k: torch.zeros(1, 65537, 1, dtype=torch.float64 if k == "score" else torch.int32) for k in ("len", "type", "closed", "score")}
    big["set_bits"] = torch.zeros(1, 65537, 1, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 65536 rows per wireframe \\(got 65537\\)"):
        ops.face_votes(big)
    with pytest.raises(ValueError, match="at most 65536 rows"):
        faces.face_votes({k: v.numpy() for k, v in big.items()})
    with pytest.raises(ValueError, match="scores and logprob"):
        faces.face_rows(np.zeros((1, 2, 1, 4)), [2], TOK, scores=np.zeros((1, 2, 1)), logprob=np.zeros((1, 2, 1, 4)))
    with pytest.raises(ValueError, match=r"T=257 positions: 1\.\.256"):
        faces.face_rows(np.zeros((1, 2, 1, 257)), [2], TOK)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _cuda(case, names, walk, G=None):
    kw = {}
    for k in names:
        if k == "own_stop":
            continue
        kw[k] = torch.as_tensor(case[k]).cuda()
    kw["own_stop"] = "own_stop" in names
    kw["follows"] = torch.as_tensor(case["follows"]).cuda() if walk else None
    return kw


def _assert_rows_equal(got, want, T, what=""):
    for k in ROW_KEYS:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].dtype, want[k].shape)
        assert np.array_equal(g, want[k]), (what, k, np.argwhere(g != want[k])[:4])


def _fsum_scores(rows, logprob, tokens, own_stop_applied_lp):
    """math.fsum of logprob over 1 .. fin for every face row (fin recovered from the tokens as the restatement does)."""
    out = np.zeros(rows["len"].shape, np.float64)
    N, F, G = out.shape
    for w in range(N):
        for f in range(F):
            for g in range(G):
                if rows["len"][w, f, g] == 0:
                    continue
                row = tokens[w, f, g]
                hit = np.flatnonzero((row >= OFF) & (row < NTOK))
                fin = int(hit[0]) if hit.size else row.size - 1
                out[w, f, g] = math.fsum(float(x) for x in own_stop_applied_lp[w, f, g, 1: fin + 1])
    return out


GRID_T = (2, 10, 63, 64, 65, 130, 256)
GRID_L = (1, 31, 32, 33, 70)
OPERAND_SETS = (set(), {"scores", "dead_end"}, {"logprob", "own_stop"}, {"logprob", "dead_end", "num_edges", "edge_map"},
                {"scores", "num_edges", "own_stop"}, {"edge_map", "own_stop"}, {"dead_end"})


def _grid():
    """Every T with every L; G, N, the walk and the optional operands cycle so that each value meets each T and each L."""
    out = []
    for i, T in enumerate(GRID_T):
        for j, L in enumerate(GRID_L):
            k = i * len(GRID_L) + j
            out.append((T, L, (1, 3)[(i + j) % 2], (1, 3)[(i + 2 * j + (j > 2)) % 2], k % 3 != 0, OPERAND_SETS[k % len(OPERAND_SETS)]))
    return out


def test_the_grid_meets_every_value_pairwise():
    g = _grid()
    for T in GRID_T:
        rows = [r for r in g if r[0] == T]
        assert {r[1] for r in rows} == set(GRID_L) and {r[2] for r in rows} == {1, 3} and {r[3] for r in rows} == {1, 3}
        assert {r[4] for r in rows} == {True, False}
    for L in GRID_L:
        rows = [r for r in g if r[1] == L]
        assert {r[2] for r in rows} == {1, 3} and {r[3] for r in rows} == {1, 3} and {r[4] for r in rows} == {True, False}
    for name in ("scores", "logprob", "dead_end", "num_edges", "edge_map", "own_stop"):
        assert any(name in r[5] for r in g) and any(name not in r[5] for r in g)


@pytest.mark.gpu
@pytest.mark.parametrize("T,L,G,N,walk,names", _grid(), ids=lambda v: str(sorted(v)) if isinstance(v, set) else str(v))
def test_face_rows_bit_for_bit(T, L, G, N, walk, names):
    from faceformer_amd.hip import ops
    case = FR.random_case(100 + T + L, N=N, L=L, F=6, G=G, T=T)
    kw_np = _kwargs(case, names)
    want = faces.face_rows(case["tokens"], case["num_input"], TOK, follows=case["follows"] if walk else None, num_lines=L, **kw_np)
    kw = _cuda(case, names, walk)
    got = ops.face_rows(torch.as_tensor(case["tokens"]).cuda(), torch.as_tensor(case["num_input"]).cuda(), TOK, num_lines=L, **kw)
    _assert_rows_equal(got, want, T, what=(T, L, G, N))          # (the restatement's sum is sequential as well: equal bits)
    if "logprob" in names:
        lp = case["logprob"].copy()
        if kw_np["own_stop"]:
            for w in range(N):
                n = int(case["num_input"][w])
                _, cut = faces._apply_own_stop_rule_scored(case["tokens"][w, :n].reshape(-1, T), lp[w, :n].reshape(-1, T), TOK, True)
                lp[w, :n] = cut.reshape(n, G, T)
        toks = case["tokens"].copy()
        if kw_np["own_stop"]:
            for w in range(N):
                n = int(case["num_input"][w])
                toks[w, :n] = faces.apply_own_stop_rule(toks[w, :n].reshape(-1, T), TOK, True).reshape(n, G, T)
        exact = _fsum_scores(want, lp, toks, lp)
        bar = T * 2.0 ** -52 * np.abs(lp.astype(np.float64)).sum(axis=-1)
        assert (np.abs(got["score"].cpu().numpy() - exact) <= bar).all()
    votes = ops.face_votes(got, require_closed=walk)
    want_votes = faces.face_votes(want, require_closed=walk)
    for k in VOTE_KEYS:
        assert np.array_equal(votes[k].cpu().numpy(), want_votes[k]), k


@pytest.mark.gpu
def test_face_rows_on_the_reference_fixtures(cases):
    from faceformer_amd.hip import ops
    for c in cases["parallel"]:
        pred = np.asarray(c["predicts"], dtype=np.int64)[None]
        ni, ne = np.array([pred.shape[1]], np.int32), np.array([c["num_edges"]], np.int32)
        want = faces.face_rows(pred, ni, TOK, num_edges=ne, num_lines=c["num_edges"])
        got = ops.face_rows(torch.as_tensor(pred).cuda(), torch.as_tensor(ni).cuda(), TOK, num_edges=torch.as_tensor(ne).cuda(),
                            num_lines=c["num_edges"])
        _assert_rows_equal(got, want, pred.shape[-1])
    for tokens, words, ne, want_list in _fixture_enclosed(cases):
        ni, ne = np.array([tokens.shape[1]], np.int32), np.array([ne], np.int32)
        want = faces.face_rows(tokens, ni, TOK, num_edges=ne, follows=words)
        got = ops.face_rows(torch.as_tensor(tokens).cuda(), torch.as_tensor(ni).cuda(), TOK, num_edges=torch.as_tensor(ne).cuda(),
                            follows=torch.as_tensor(words).cuda())
        _assert_rows_equal(got, want, tokens.shape[-1])
        votes = {k: v.cpu().numpy() for k, v in ops.face_votes(got, require_closed=True).items()}
        assert faces.faces_of_rows({k: v.cpu().numpy() for k, v in got.items()}, votes, 0)["enclosed"] == want_list


def _vote_rows(seed, N, R, fw, pool, all_equal=False):
    """A face_rows dict [N, R, 1] made directly: keys from a pool of `pool` bitmaps (0: all distinct)."""
    g = np.random.default_rng([0x707E, seed, N, R, fw, pool])
    if pool:
        keys = g.integers(0, 2 ** 32, size=(N, pool, fw), dtype=np.uint64).astype(np.uint32)
        bits = np.stack([keys[w][g.integers(0, pool, size=R)] for w in range(N)])
    else:
        bits = g.integers(0, 2 ** 32, size=(N, R, fw), dtype=np.uint64).astype(np.uint32)
        bits[..., 0] = (bits[..., 0] & np.uint32(0xFFFF0000)) | np.arange(R, dtype=np.uint32)[None, :] % 65536
    if all_equal:
        bits[:] = bits[:, :1]
    rows = {"set_bits": bits.reshape(N, R, 1, fw).view(np.int32),
            "len": (g.random((N, R, 1)) < 0.9).astype(np.int32) * g.integers(1, 9, size=(N, R, 1)).astype(np.int32),
            "type": g.integers(0, 3, size=(N, R, 1)).astype(np.int32),
            "closed": (g.random((N, R, 1)) < 0.7).astype(np.int32),
            "score": np.round(g.standard_normal((N, R, 1)) * 4, 1)}       # (rounded: equal scores occur)
    if all_equal:
        rows["len"][:] = 3
    return rows


def _run_votes_twice(rows, require_closed):
    from faceformer_amd.hip import ops
    dev = {k: torch.as_tensor(v).cuda() for k, v in rows.items()}
    a = {k: v.cpu().numpy() for k, v in ops.face_votes(dev, require_closed=require_closed).items()}
    b = {k: v.cpu().numpy() for k, v in ops.face_votes(dev, require_closed=require_closed).items()}
    for k in VOTE_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    return a


def _assert_votes_equal(got, want):
    for k in VOTE_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.argwhere(got[k] != want[k])[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("require_closed", (False, True))
@pytest.mark.parametrize("pool", (5, 0))
@pytest.mark.parametrize("fw", (1, 2, 3))
@pytest.mark.parametrize("R", (1, 63, 64, 65, 700))
def test_face_votes_bit_for_bit(R, fw, pool, require_closed):
    rows = _vote_rows(7, 2, R, fw, pool)
    _assert_votes_equal(_run_votes_twice(rows, require_closed), faces.face_votes(rows, require_closed=require_closed))


@pytest.mark.gpu
def test_face_votes_capacity_all_equal_and_shuffled():
    # L = 1024 (32 words), R = 4096, about half of the rows duplicates
    rows = _vote_rows(11, 1, 4096, 32, 2048)
    got = _run_votes_twice(rows, False)
    want = faces.face_votes(rows)
    _assert_votes_equal(got, want)
    dup = 1.0 - int(want["num_faces"][0]) / float((rows["len"] > 0).sum())
    assert 0.3 < dup < 0.7, dup
    # every row equal
    rows = _vote_rows(12, 2, 700, 3, 1, all_equal=True)
    got = _run_votes_twice(rows, False)
    _assert_votes_equal(got, faces.face_votes(rows))
    assert got["num_faces"].tolist() == [1, 1] and got["votes"][:, 0, 0].tolist() == [700, 700] and (got["rep"] == 0).all()
    # shuffled inside the wireframe: the groups are the same sets of (original) rows
    rows = _vote_rows(13, 2, 700, 2, 5)
    base = _run_votes_twice(rows, True)
    perm = np.stack([np.random.default_rng([13, w]).permutation(700) for w in range(2)])       # new row i holds old row perm[i]
    shuffled = {k: np.stack([v[w][perm[w]] for w in range(2)]) for k, v in rows.items()}
    got = _run_votes_twice(shuffled, True)
    _assert_votes_equal(got, faces.face_votes(shuffled, require_closed=True))

    def groups(rep, old_of_new):
        out = {}
        for i, p in enumerate(rep.reshape(-1)):
            if p >= 0:
                out.setdefault(int(p), set()).add(int(old_of_new[i]))
        return {frozenset(s) for s in out.values()}
    for w in range(2):
        assert groups(got["rep"][w], perm[w]) == groups(base["rep"][w], np.arange(700))


def _c_rows(lib, g, case, names, walk, L, flags_own_stop):
    """ff_face_rows through the C ABI on guarded operands; returns the outputs (device tensors)."""
    import redzone  # noqa: F401
    N, F, G, T = case["tokens"].shape
    fw = (L + 31) // 32
    t = lambda k, dt: g.embed(torch.as_tensor(case[k]).to(dt))
    tokens, ni = t("tokens", torch.int64), t("num_input", torch.int32)
    opt = {k: (t(k, dt) if k in names else None) for k, dt in (("num_edges", torch.int32), ("scores", torch.float32),
                                                              ("logprob", torch.float32), ("dead_end", torch.int32),
                                                              ("edge_map", torch.int32))}
    follows = g.embed(torch.as_tensor(case["follows"])) if walk else None
    out = {k: g.embed(torch.full((N, F, G), 77, dtype=torch.int32)) for k in ("len", "type", "closed", "loops")}
    out["edges"] = g.embed(torch.full((N, F, G, T), 77, dtype=torch.int32))
    out["loop_of"] = g.embed(torch.full((N, F, G, T), 77, dtype=torch.int32))
    out["set_bits"] = g.embed(torch.full((N, F, G, fw), 77, dtype=torch.int32))
    score = g.embed(torch.full((N, F, G, 2), 77, dtype=torch.int32))           # fp64 [N, F, G] as pairs of words
    p = lambda x: None if x is None else x.data_ptr()
    st = lib.ff_face_rows(p(tokens), N, F, G, T, p(ni), p(opt["num_edges"]), L, OFF, NTOK, p(opt["scores"]), p(opt["logprob"]),
                          p(opt["dead_end"]), p(follows), p(opt["edge_map"]), 1 if flags_own_stop else 0,
                          *[p(out[k]) for k in ROW_KEYS[:-1]], p(score), torch.cuda.current_stream().cuda_stream)
    assert st == 0, lib.ff_last_error()
    torch.cuda.synchronize()
    out["score"] = score.view(torch.float64).reshape(N, F, G)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("names,walk", [(set(), False), ({"scores", "dead_end", "num_edges", "edge_map", "own_stop"}, True),
                                        ({"logprob", "own_stop"}, True)], ids=["bare", "scores", "logprob"])
def test_entries_inside_poisoned_surroundings(hip_lib, names, walk):
    import redzone
    T, L = 65, 33
    case = FR.random_case(5, N=3, L=L, F=6, G=3, T=T)
    want = faces.face_rows(case["tokens"], case["num_input"], TOK, follows=case["follows"] if walk else None, num_lines=L,
                           **_kwargs(case, names))
    want_votes = faces.face_votes(want, require_closed=walk)
    results = []
    for fill in (redzone.POISON, redzone.ZERO):
        g = redzone.Guard(fill)
        got = _c_rows(hip_lib, g, case, names, walk, L, "own_stop" in names)
        g.check()
        _assert_rows_equal(got, want, T, what=fill)
        # the votes entry on guarded operands and an exact-size workspace that holds the fill
        N, F, G = want["len"].shape
        R, fw = F * G, (L + 31) // 32
        gv = redzone.Guard(fill)
        ins = [gv.embed(got[k].contiguous().cpu() if k != "score" else got[k].contiguous().cpu().view(torch.int32).reshape(N, R, 2))
               for k in ("set_bits", "len", "type", "closed", "score")]
        outs = {k: gv.embed(torch.full((N, R), 77, dtype=torch.int32)) for k in ("rep", "votes", "major")}
        best = gv.embed(torch.full((N, R, 2), 77, dtype=torch.int32))
        num = gv.embed(torch.full((N,), 77, dtype=torch.int32))
        nbytes = hip_lib.ff_face_votes_workspace_bytes(N, R)
        assert nbytes > 0 and nbytes % 8 == 0
        ws = gv.bytes(nbytes)
        st = hip_lib.ff_face_votes(*[x.data_ptr() for x in ins], N, R, fw, 1 if walk else 0, outs["rep"].data_ptr(),
                                   outs["votes"].data_ptr(), best.data_ptr(), outs["major"].data_ptr(), num.data_ptr(),
                                   ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        assert st == 0, hip_lib.ff_last_error()
        gv.check()
        got_votes = {"rep": outs["rep"], "votes": outs["votes"], "major": outs["major"], "best": best.view(torch.float64).reshape(N, R),
                     "num_faces": num}
        for k in VOTE_KEYS:
            assert np.array_equal(got_votes[k].cpu().numpy().reshape(want_votes[k].shape), want_votes[k]), (fill, k)
        # a workspace one byte short is refused
        st = hip_lib.ff_face_votes(*[x.data_ptr() for x in ins], N, R, fw, 0, outs["rep"].data_ptr(), outs["votes"].data_ptr(),
                                   best.data_ptr(), outs["major"].data_ptr(), num.data_ptr(), ws.data_ptr(), nbytes - 1,
                                   torch.cuda.current_stream().cuda_stream)
        assert st == -3 and b"workspace" in hip_lib.ff_last_error()
        results.append(got)
    for k in ROW_KEYS:
        redzone.assert_same_bits(results[0][k], results[1][k], k)


@pytest.mark.gpu
def test_err_arg_before_any_launch(hip_lib):
    """Every refusal returns FF_ERR_ARG with the outputs untouched (they hold the fill: nothing was launched)."""
    lib = hip_lib
    N, F, G, T, L = 1, 2, 1, 4, 8
    tokens = torch.zeros(N, F, G, 257, dtype=torch.int64).cuda()
    ni = torch.full((N,), F, dtype=torch.int32).cuda()
    sc, lp = torch.zeros(N, F, G).cuda(), torch.zeros(N, F, G, 257).cuda()
    outs = [torch.full((N * F * G * 257,), 77, dtype=torch.int32).cuda() for _ in range(7)] + [torch.full((N * F * G,), 77.0, dtype=torch.float64).cuda()]
    stream = torch.cuda.current_stream().cuda_stream

    def rows(tok=tokens, T=T, off=OFF, ntok=NTOK, scores=None, logprob=None, flags=0):
        return lib.ff_face_rows(None if tok is None else tok.data_ptr(), N, F, G, T, ni.data_ptr(), None, L, off, ntok,
                                None if scores is None else scores.data_ptr(), None if logprob is None else logprob.data_ptr(),
                                None, None, None, flags, *[o.data_ptr() for o in outs], stream)
    assert rows() == 0
    torch.cuda.synchronize()
    for o in outs:
        o.fill_(77)
    for what, kw in (("T=0", dict(T=0)), ("T=257", dict(T=257)), ("off >= ntok", dict(off=4, ntok=4)), ("off < 0", dict(off=-1)),
                     ("scores with logprob", dict(scores=sc, logprob=lp)), ("NULL tokens", dict(tok=None)), ("flags", dict(flags=2))):
        assert rows(**kw) == -1, what
        assert b"ff_face_rows" in lib.ff_last_error(), what
    torch.cuda.synchronize()
    assert all(bool((o == 77).all()) for o in outs)
    # votes: R past the limit
    R = 65537
    assert lib.ff_face_votes_workspace_bytes(1, R) == 0 and lib.ff_face_votes_workspace_bytes(1, 65536) > 0
    ins = [torch.zeros(R, dtype=torch.int32).cuda() for _ in range(4)] + [torch.zeros(R, dtype=torch.float64).cuda()]
    vout = [torch.full((R,), 77, dtype=torch.int32).cuda() for _ in range(2)] + [torch.full((R,), 77.0, dtype=torch.float64).cuda()] + \
           [torch.full((R,), 77, dtype=torch.int32).cuda() for _ in range(2)]
    ws = torch.zeros(1 << 16, dtype=torch.int64).cuda()
    st = lib.ff_face_votes(*[x.data_ptr() for x in ins], 1, R, 1, 0, *[o.data_ptr() for o in vout], ws.data_ptr(), ws.numel() * 8, stream)
    assert st == -1 and b"above 65536" in lib.ff_last_error()
    st = lib.ff_face_votes(*[x.data_ptr() for x in ins], 1, 8, 1, 2, *[o.data_ptr() for o in vout], ws.data_ptr(), ws.numel() * 8, stream)
    assert st == -1 and b"unknown flag bits" in lib.ff_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 77).all()) for o in vout)


# ---- 4b. the model option: rejections on the CPU ----------------------------------------------------------------------------------
def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _tiny_inputs(**more):
    return dict({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                 "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}, **more)


def test_models_reject_the_option_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert model.extract_faces is False
    for bad in (True, "closed", 1, "Parse"):
        model.extract_faces = bad
        with torch.no_grad(), pytest.raises(ValueError, match="extract_faces=.*must be False, 'parse' or 'enclosed'"):
            model.forward_eval(_tiny_inputs())
    model.extract_faces = "enclosed"
    for em in (torch.zeros(1, 8, dtype=torch.int64), torch.zeros(1, 7, dtype=torch.int32), np.zeros((1, 8), np.int32)):
        with torch.no_grad(), pytest.raises(ValueError, match=r"edge_map must be an int32 tensor of shape \[1, 8\]"):
            model.forward_eval(_tiny_inputs(edge_map=em))
    from faceformer_amd.hip import lib
    with torch.no_grad(), pytest.raises(lib.HipExtensionError, match="model parameters are on cpu"):   # (a valid call gets as far as the engine)
        model.forward_eval(_tiny_inputs(edge_map=torch.zeros(1, 8, dtype=torch.int32)))
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        sub = _tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        sub.extract_faces = "parse"
        with torch.no_grad(), pytest.raises(ValueError, match="extract_faces needs the native engine"):
            sub.forward_eval(_tiny_inputs())
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    seq.extract_faces = "parse"
    with torch.no_grad(), pytest.raises(ValueError, match="extract_faces is a SurfaceFormer_Parallel option"):
        seq.forward_eval({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                          "label": torch.zeros(1, 6, dtype=torch.long)})

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    ns = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain=None,
                               extract_faces="parse")
    with pytest.raises(ValueError, match="decode_sharded does not implement extract_faces"):
        dist.decode_sharded(ns, {}, NoDist())
    ns.extract_faces = False
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(ns, {}, NoDist())


# ---- 9. the model option on the goldens -------------------------------------------------------------------------------------------
MODEL_MODES = {
    "greedy": {},
    "greedy_logprob": {"return_logprob": True},
    "beam4": {"beam_width": 4},
    "sample4": {"num_samples": 4, "sample_seed": 3},
    "loops": {"constrain": "loops"},
    "loops_exact_samples4": {"constrain": "loops", "constrain_exact": True, "constrain_samples": 4, "sample_seed": 5},
    "retire": {"retire_finished": True},
}


def _expected_faces(out, ni, table_words, extract, L, edge_map=None):
    np_ = lambda k: out[k].cpu().numpy()
    for kind in ("beam", "sample"):
        if "predict_%ss" % kind in out:
            tokens = np_("predict_%ss" % kind)
            kw = dict(scores=np_("predict_%s_scores" % kind))
            if "predict_%s_dead_end" % kind in out:
                kw["dead_end"] = np_("predict_%s_dead_end" % kind)
            break
    else:
        tokens = np_("predict")
        kw = dict(own_stop=True)
        if "predict_logprob" in out:
            kw["logprob"] = np_("predict_logprob")
    rows = faces.face_rows(tokens, ni, TOK, follows=table_words if extract == "enclosed" else None, edge_map=edge_map, num_lines=L, **kw)
    rows.update(faces.face_votes(rows, require_closed=extract == "enclosed"))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODEL_MODES))
@pytest.mark.parametrize("name", ("par_small_gain4", "par_small_ragged", "par_full_n40_gain4"))
def test_model_publishes_the_faces_of_its_rows(name, mode):
    from test_constrain import _model
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni, L = lat["num_input"], case["model"]["L"]
    words = faces.pack_follow_bits(table)
    attrs = MODEL_MODES[mode]
    saved = {k: getattr(model, k) for k in list(attrs) + ["extract_faces"]}
    try:
        for k, v in attrs.items():
            setattr(model, k, v)
        with torch.no_grad():
            off = model(dict(b))
        assert "faces" not in off
        closed_rows = 0
        for extract in ("parse", "enclosed"):
            model.extract_faces = extract
            emap = None
            if extract == "enclosed":
                emap = np.tile(np.arange(L, dtype=np.int32), (len(ni), 1))
                emap[:, 1::2] -= 1                                           # (co-edge pairs 2k, 2k + 1 -> 2k)
            with torch.no_grad():
                out = model(dict(b) if emap is None else dict(b, edge_map=torch.as_tensor(emap).cuda()))
            for k in off:
                if torch.is_tensor(off[k]) and k.startswith("predict"):
                    assert torch.equal(off[k], out[k]), k                    # (nothing of the decode changes)
            assert set(out) - set(off) - {"edge_map"} == {"faces"}
            want = _expected_faces(out, ni, words, extract, L, emap)
            assert set(out["faces"]) == set(ROW_KEYS) | set(VOTE_KEYS)
            for k, v in want.items():
                got = out["faces"][k].cpu().numpy()
                assert got.shape == v.shape and got.dtype == v.dtype, (k, got.shape, v.shape)
                assert got.tobytes() == v.tobytes(), (extract, k)
            closed_rows += int((want["closed"] == 1).sum())
            assert int(want["num_faces"].sum()) > 0 or extract == "enclosed"
        if attrs.get("constrain") == "loops":
            assert closed_rows > 0                                           # (the constrained decode does close loops on the lattice)
    finally:
        for k, v in saved.items():
            setattr(model, k, v)


# ---- 10. the CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_flag_reaches_run_test_and_is_refused_where_it_does_not_apply(monkeypatch, tmp_path):
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    _untouchable(monkeypatch)
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).device_faces is False
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--device-faces"]).device_faces is True
    seen = []
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw["device_faces"]))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--device-faces", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert seen == [True, False]
    monkeypatch.undo()
    _untouchable(monkeypatch)
    seq = load_cfg(os.path.join(ROOT, "configs", "seq2seq.yml"), ["root_dir", str(tmp_path)])
    with pytest.raises(ValueError, match="--device-faces applies to SurfaceFormer_Parallel only"):
        cli.run_test(seq, None, device="cpu", model=object(), device_faces=True)
    par = load_cfg(os.path.join(ROOT, "configs", "ours.yml"), ["root_dir", str(tmp_path)])
    two = types.SimpleNamespace(get_world_size=lambda: 2, get_rank=lambda: 0)
    with pytest.raises(ValueError, match="--device-faces is not implemented for multi-rank runs"):
        cli.run_test(par, None, device="cpu", model=object(), device_faces=True, dist_mod=two)


def test_record_from_face_arrays_is_the_host_record():
    """record_of from the restatement's arrays equals record_of from the tokens: a co-edge config with pairings and a plain
    one, greedy rows with scores and draws with votes (CPU; the GPU runs of the same driver follow)."""
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    L, T = 16, 8
    for coedge in (False, True):
        cfg = load_cfg(os.path.join(ROOT, "configs", "ours.yml"), ["model.num_lines", str(L), "model.max_face_length", str(T),
                                                                     "post_process.is_coedge", str(coedge)])
        lat, edges, loops = CR.lattice_batch([11], L, T, 3)
        raw = {"edges": [e.astype(np.float64).tolist() for e in edges[0]], "pairings": {"1": 0, "5": 4}, "dominant_directions": []}
        item = {"num_input": 11, "label": np.zeros((L, T), np.int64)}
        table = faces.follow_table(lat["input"].numpy(), cfg.post_process.enclosedness_tol, [11])
        case = FR.random_case(21, N=1, L=11, F=11, G=4, T=T)
        case["table"], case["follows"] = table[:, :11, :11], None
        tokens = FR.random_case(21, N=1, L=11, F=11, G=4, T=T)["tokens"]
        g = np.random.default_rng(4)
        for f in range(11):                      # (rows that do close on the lattice: its own loops, rotated)
            lp = loops[0][f % len(loops[0])]
            r = int(g.integers(0, len(lp)))
            for k in range(2):
                tokens[0, f, k, : len(lp) + 1] = [NTOK + e for e in (lp[r:] + lp[:r])] + [OFF + (f + k) % 3]
        stop = next((j for j in range(1, T) if (tokens[0, :, 0, j] < NTOK).all()), T - 1)
        tokens[..., stop + 1:] = 0               # (what a decode publishes: nothing behind the stop step)
        emap = np.arange(L, dtype=np.int32)[None].copy()
        emap[0, 1], emap[0, 5] = 0, 4
        words = faces.pack_follow_bits(table)
        mode_enclosed = coedge
        # greedy + scores
        pred, lp = tokens[0, :, 0], -np.abs(g.standard_normal((11, T))).astype(np.float32)
        lp[:, 0] = 0
        rows = faces.face_rows(pred[None], [11], cfg.model.token, logprob=lp[None], own_stop=True, follows=words if mode_enclosed else None,
                               edge_map=emap if coedge else None, num_lines=L)
        rows.update(faces.face_votes(rows, require_closed=mode_enclosed))
        host = cli.record_of(cfg, raw, item, pred, True, logprob=lp)
        dev = cli.record_of(cfg, raw, item, None, True, logprob=True, device_faces=rows)
        a, b = json.loads(host[0]), json.loads(dev[0])
        assert len(a["pred_faces"]) > 0 and len(a["pred_face_scores"]) == len(a["pred_faces"])
        for x, y in zip(a.pop("pred_face_scores"), b.pop("pred_face_scores")):
            assert abs(x - y) <= T * 2.0 ** -52 * abs(x)
        assert json.dumps(a) == json.dumps(b) and host[1] == dev[1]
        # draws with scores: --sample
        sc = g.standard_normal((11, 4)).astype(np.float32)
        rows = faces.face_rows(tokens, [11], cfg.model.token, scores=sc[None], follows=words if mode_enclosed else None,
                               edge_map=emap if coedge else None, num_lines=L)
        rows.update(faces.face_votes(rows, require_closed=mode_enclosed))
        rows["first"] = faces.face_rows(tokens[:, :, 0], [11], cfg.model.token, own_stop=True, follows=words if mode_enclosed else None,
                                        edge_map=emap if coedge else None, num_lines=L)
        rows["first"].update(faces.face_votes(rows["first"], require_closed=mode_enclosed))
        assert np.array_equal(faces.apply_own_stop_rule(tokens[0, :, 0], cfg.model.token, True), tokens[0, :, 0])
        host = cli.record_of(cfg, raw, item, tokens[0, :, 0], True, samples=(tokens[0], sc))
        dev = cli.record_of(cfg, raw, item, None, True, samples=(None, sc), device_faces=rows)
        assert host == dev and len(json.loads(host[0])["pred_sample_faces"]) > 0


def _cli_setups(tmp_path):
    """(name, cfg, checkpoint path) of the co-edge golden set-up (tests/golden/cli_coedge_case.json, post_process.is_coedge at its
    default) and of a plain config over random wireframes."""
    import sys
    sys.path.insert(0, ROOT)
    from faceformer_amd.config import load_cfg
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    gold = json.load(open(os.path.join(GOLDEN, "cli_coedge_case.json")))
    m = gold["model"]
    out = []
    root = tmp_path / "coedge"
    (root / "json").mkdir(parents=True)
    names = []
    for i, smp in enumerate(gold["samples"]):
        json.dump(smp["raw"], open(root / "json" / ("%08d.json" % i), "w"))
        names.append("json/%08d.json" % i)
    open(root / "test.txt", "w").write("\n".join(names) + "\n")
    dims = ["model.num_lines", str(m["num_lines"]), "model.max_face_length", str(m["max_face_length"]), "model.num_model",
            str(m["num_model"]), "model.num_head", str(m["num_head"]), "model.num_feedforward", str(m["num_feedforward"]),
            "model.num_encoder_layers", str(m["num_encoder_layers"]), "model.num_decoder_layers", str(m["num_decoder_layers"])]
    cfg = load_cfg(os.path.join(ROOT, "configs", "ours.yml"), dims + ["root_dir", str(root)])
    assert cfg.post_process.is_coedge is True
    sd = make_state_dict(state_dict_spec("parallel", m["num_lines"], m["max_face_length"], m["num_model"], m["num_feedforward"],
                                         m["num_encoder_layers"], m["num_decoder_layers"]), gold["recipe"], gold["wseed"])
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(cfg)}, tmp_path / "coedge.ckpt")
    out.append(("coedge", cfg, str(tmp_path / "coedge.ckpt")))
    from test_cli import _setup
    cfg, sd = _setup(str(tmp_path / "plain"))
    assert cfg.post_process.is_coedge is False
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(cfg)}, tmp_path / "plain.ckpt")
    out.append(("plain", cfg, str(tmp_path / "plain.ckpt")))
    return out


CLI_VARIANTS = {"alone": {}, "beam4": {"beam": 4}, "sample4": {"sample": 4, "seed": 2},
                "loops_samples4": {"constrain": "loops", "constrain_samples": 4, "seed": 2}, "scores": {"scores": True}}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(CLI_VARIANTS))
def test_cli_device_faces_writes_the_same_records(hip_lib, tmp_path, capsys, variant):
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    kw = CLI_VARIANTS[variant]
    for name, cfg, ckpt in _cli_setups(tmp_path):
        runs = {}
        for flag in (False, True):
            capsys.readouterr()
            out_dir = cli.run_test(cfg, ckpt, out_dir=str(tmp_path / ("%s_%d" % (name, flag))), batch_size=2, device_faces=flag, **kw)
            metrics = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("test_precision")]
            assert len(metrics) == 1
            runs[flag] = ({n: open(os.path.join(out_dir, n)).read() for n in sorted(os.listdir(out_dir))}, metrics[0])
        host, dev = runs[False], runs[True]
        assert host[1] == dev[1], (name, host[1], dev[1])
        assert sorted(host[0]) == sorted(dev[0]) and len(host[0]) >= 2
        T = int(cfg.model.max_face_length)
        for n in host[0]:
            if variant != "scores":
                assert host[0][n] == dev[0][n], (name, n)
                continue
            a, b = json.loads(host[0][n]), json.loads(dev[0][n])
            sa, sb = a.pop("pred_face_scores"), b.pop("pred_face_scores")
            assert len(sa) == len(sb) == len(a["pred_faces"])
            for x, y in zip(sa, sb):       # sums of non-positive terms: sum|lp| = |score|
                assert abs(x - y) <= T * 2.0 ** -52 * abs(x), (name, n, x, y)
            assert json.dumps(a) == json.dumps(b), (name, n)
