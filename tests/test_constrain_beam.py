"""Beam search over the loop-constrained pointer decode: the numpy rule against its two parents, every rejection,
the C ABI, the one-step operator against the numpy rule on the kernel's own logits, and the engine against the constrained
greedy decode (W = 1), the plain beam decode (both bits clear), the numpy rule replayed on its own trace, the enclosure walk,
and its own repetition under two plans and inside poisoned surroundings."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import beam_ref as BR
import constrain_beam_ref as CBR
import constrain_ref as CR
from conftest import ROOT, token_ns
from faceformer_amd import faces
from faceformer_amd.hip import modes as MODES

RECORD = MODES.CONSTRAIN_BEAM        # the feature's record of the mode table: the widths and the entry the tests below go through
TOK = token_ns()
TERM = (TOK.face_type_offset, TOK.len)
NTOK = TOK.len
FILL = CR.FILL
LOOPS = CR.NO_REPEAT | CR.CONNECT
ALL_FLAGS = (0, CR.NO_REPEAT, CR.CONNECT, LOOPS)
PARALLEL, SEQ2SEQ = 0, 1

OP_S = (1, 5, 63, 64, 65, 260, 1028)
OP_W = (1, 2, 3, 4, 8)
OP_G = (1, 3, 9)
GPW = 2                      # groups per wireframe of the operator cases


# ---- the operator cases (also read by tools/constrain_beam_left_out.py) ----------------------------------------------------------------
def op_seed(S, W, G):
    return 1000 * S + 10 * W + G


def operator_case(G, W, S, seed, greedy=False):
    """One launch: G groups of W beams in mixed states.  greedy: every beam non-empty with score 0 and the dead flag clear -- the
    inputs ops.pointer_constrained takes as well (W = 1).  -> dict of numpy arrays / CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng([seed, G, W, S])
    ntok = NTOK if S > NTOK else S
    term = TERM if ntok == NTOK else (0, ntok)
    L, B = S - ntok, G * W
    NW = (G + GPW - 1) // GPW
    logits = torch.randn(B, S, generator=g) * 3.0
    mask = torch.rand(NW, S, generator=g) < 0.15
    mask[:, :ntok] = False
    kv = torch.full((NW,), S, dtype=torch.int32)
    kv[0] = max(1, S - 2)                                                # kv_len = S - 2
    if NW > 2 and L > 0:
        mask[2] = True                                                   # a one-live-key wireframe: one edge (the rule may mask it too)
        mask[2, ntok + int(rng.integers(0, L))] = False
    if NW > 3:
        kv[NW - 1] = 0                                                   # an all-masked wireframe
    follows = CR.random_follows(NW, L, seed)
    scores = -5.0 * rng.random(B)
    fin = np.zeros(B, dtype=np.int32)
    dead = np.zeros(B, dtype=np.int32)
    first = np.full(B, -1, dtype=np.int32)
    prev = np.full(B, -1, dtype=np.int32)
    visited = np.zeros((B, L), dtype=bool)
    for b in range(B):
        kind = (b + b // W) % 6              # 0 open, 1 closed, 2 finished, 3 open with a planted dead end, 4 empty, 5 closed, much visited
        w = (b // W) // GPW
        if kind == 2:
            fin[b] = 1
            dead[b] = rng.integers(0, 2)
        if kind == 4 and not greedy and b % W:
            scores[b] = -np.inf
        if L == 0:
            continue
        if kind in (0, 3, 2):
            first[b], prev[b] = rng.integers(0, L), rng.integers(0, L)
            visited[b, [first[b], prev[b]]] = True
            if kind == 3:
                visited[b] |= follows[w, prev[b]]                        # every follower visited: a dead end under NO_REPEAT + CONNECT
        else:
            prev[b] = rng.integers(-1, L)
            visited[b] = rng.random(L) < (0.2 if kind == 1 else 0.9)
    if greedy:
        scores[:] = 0.0
        dead[:] = 0
    memory = torch.randn(NW, S, 64, generator=g)
    wf = torch.arange(NW)
    pad = (mask | (torch.arange(S)[None, :] >= kv[wf, None])).numpy()
    return dict(logits=logits, mask=mask, kv=kv, follows=follows, scores=scores.astype(np.float32), fin=fin, dead=dead, first=first, prev=prev,
                visited=visited, memory=memory, pad=pad, ntok=ntok, term=term, L=L, NW=NW, G=G, W=W, S=S)


def case_states(c):
    return [(frozenset(np.flatnonzero(c["visited"][b]).tolist()), None if c["first"][b] < 0 else int(c["first"][b]),
             None if c["prev"][b] < 0 else int(c["prev"][b])) for b in range(c["G"] * c["W"])]


def rule_on_case(c, flags, logits=None, dtype=np.float64):
    """CBR.beam_step on a case's inputs (`logits`: the raw rows, default the case's own)."""
    raw = (c["logits"].numpy() if logits is None else logits).astype(dtype)
    return CBR.beam_step(raw, c["pad"], c["scores"].astype(np.float64), c["fin"] != 0, c["dead"] != 0, case_states(c), c["W"], flags,
                         c["ntok"], c["term"], lambda w: c["follows"][w], np.arange(c["G"]) // GPW)


# ---- CPU: the numpy rule against its two parents -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 65, 260])
def test_numpy_rule_at_width_1_is_the_greedy_rule(S):
    for flags in ALL_FLAGS:
        c = operator_case(9, 1, S, op_seed(S, 1, 9), greedy=True)
        res = rule_on_case(c, flags)
        sts = case_states(c)
        for b in range(9):
            if c["fin"][b]:
                assert (res["tok"][b], res["scores"][b], bool(res["fin"][b])) == (0, 0.0, True)
                continue
            tok, lp, fin, dead, st = CBR.greedy_row(c["logits"][b].numpy().astype(np.float64), c["pad"][b // GPW], sts[b], flags, c["ntok"],
                                                    c["term"], c["follows"][b // GPW])
            assert (res["tok"][b], bool(res["fin"][b]), bool(res["dead"][b]), res["states"][b]) == (tok, fin, dead, st), (S, flags, b)
            assert res["parent"][b] == 0 and abs(res["scores"][b] - lp) <= 1e-12, (S, flags, b)


@pytest.mark.parametrize("S", [5, 65, 260])
def test_numpy_rule_with_both_bits_clear_is_the_beam_rule(S):
    seen = 0
    assert RECORD.per_anchor
    for W in (2, 4, 8):
        if W > S:
            continue
        c = operator_case(9, W, S, op_seed(S, W, 9))
        res = rule_on_case(c, 0)
        raw = c["logits"].numpy().astype(np.float64)
        for gi in range(9):
            sl = slice(gi * W, (gi + 1) * W)
            lg = np.where(c["pad"][gi // GPW][None, :], -BR.FLT_MAX, raw[sl])
            want = BR.group_step(lg, c["scores"][sl].astype(np.float64), c["fin"][sl] != 0, c["term"][0], c["term"][1], c["ntok"])
            kept_masked = any(want["scores"][r] > -np.inf and not c["fin"][sl][want["parent"][r]] and
                              lg[want["parent"][r], want["tok"][r]] == -BR.FLT_MAX for r in range(W))
            if kept_masked:
                continue
            seen += 1
            for k in ("parent", "tok", "fin"):
                assert np.array_equal(res[k][sl], want[k]), (S, W, gi, k)
            assert np.array_equal(res["scores"][sl], want["scores"]), (S, W, gi)
    assert seen > 0


# ---- CPU: the C ABI ----------------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_beam_constrained_select", "ff_decode_constrained_beam_workspace_bytes", "ff_decode_constrained_beam")


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"^\**", "", part.strip().split()[-1].lstrip("*")) for decl in body.split(";") if decl.strip()
            for part in decl.split(",")]


def test_header_binding_and_struct_fields_agree_within_abi_105():
    from faceformer_amd.hip import lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define FF_ABI_VERSION 105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
    assert "DESIGN.md 21" in header and "entries added within ABI 105" in header
    assert [f for f, _ in lib.ConstrainBeamParams._fields_] == _struct_fields(header, "ff_constrain_beam_params") == \
        ["width", "flags", "follows", "beams", "scores", "dead_end", "trace_parent"]
    assert [f for f, _ in lib.BeamConstrainedStep._fields_] == _struct_fields(header, "ff_beam_constrained_step")
    nargs = lambda name: len(re.search(r"\b%s\s*\((.*?)\)" % name, code, re.S).group(1).split(","))
    for name in NEW_ENTRIES:
        assert len(lib.SIGNATURES[name][1]) == nargs(name), name
    assert len(lib.SIGNATURES["ff_decode_constrained_beam"][1]) == len(lib.SIGNATURES["ff_decode_beam"][1])


def test_the_mode_record_is_a_replacement_of_constrain_outside_the_table():
    from faceformer_amd.hip import engine, modes
    rec = RECORD
    assert rec not in modes.MODES and rec.entry == "ff_decode_constrained_beam" and rec.per_anchor
    assert rec.excludes == modes.CONSTRAIN.excludes and rec.switches == modes.CONSTRAIN.switches and rec.own == modes.CONSTRAIN.own
    assert modes.of_options(False, 0, constrain=3, num_samples=0, beam_width=0) == (modes.CONSTRAIN, 3)
    assert modes.of_options(False, 4, constrain=3, num_samples=0, beam_width=0) == (rec, 4)
    assert modes.of_options(False, 4, constrain=0, num_samples=0, beam_width=0) == (rec, 4)
    assert inspect.signature(engine.PathEngine.decode).parameters["constrain_beams"].default is None
    assert inspect.signature(engine.check_constrain_options).parameters["constrain_beams"].default == 0


# ---- CPU: every rejection, with its text ---------------------------------------------------------------------------------------------------
def _raises(text, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == text, str(e.value)


EXCLUDES = "constrain_beams excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width and num_samples"


def test_every_rejected_combination_raises_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine, lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    table = torch.zeros(2, 8, 1, dtype=torch.int32)
    ok = dict(flags=3, variant=PARALLEL, retire=False, return_pointer=False, no_stop=False, stop_callback=None, extra_mask=None,
              logprob=False, beam_width=0, num_samples=0, term_range=TERM, follow_table=table, constrain_beams=4, S=12)
    check = engine.check_constrain_options
    check(**ok)
    check(**dict(ok, constrain_beams=0)), check(**dict(ok, constrain_beams=None))      # off: constrain's own checks
    _raises("constrain_beams is a parallel-variant option", check, **dict(ok, variant=SEQ2SEQ))
    _raises("constrain_beams needs term_range = (lo, hi) with lo < hi", check, **dict(ok, term_range=None))
    for k, v in (("retire", True), ("return_pointer", True), ("no_stop", True), ("stop_callback", lambda c: False),
                 ("extra_mask", torch.zeros(1)), ("logprob", True), ("beam_width", 2), ("num_samples", 2)):
        _raises(EXCLUDES, check, **dict(ok, **{k: v}))
    _raises("constrain='loops' needs follow_table (ops.follow_table)", check, **dict(ok, follow_table=None))
    _raises("constrain_beams=9: must be None, 0 or a width in 1..8", check, **dict(ok, constrain_beams=9))
    _raises("constrain_beams=-1: must be None, 0 or a width in 1..8", check, **dict(ok, constrain_beams=-1))
    _raises("constrain_beams=True: must be None, 0 or a width in 1..8", check, **dict(ok, constrain_beams=True))
    _raises("constrain_beams=4: must be in 1..8 and at most S = 3", check, **dict(ok, S=3))
    _raises("constrain_beams=4 needs constrain ('no_repeat' or 'loops'): it is the beam search over the constrained keys", check,
            **dict(ok, flags=None))
    # PathEngine.decode on an engine object without a constructor call
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng.num_token, eng.device = 4, torch.device("cpu")
    memory = torch.zeros(2, 12, 64)
    base = dict(T=5, F=4, num_input=[4, 3], term_range=TERM, constrain="loops", follow_table=table, constrain_beams=2)
    dec = lambda **kw: eng.decode(memory, None, None, kw.pop("variant", PARALLEL), **dict(base, **kw))
    _raises("constrain_beams=2 needs constrain ('no_repeat' or 'loops'): it is the beam search over the constrained keys", dec, constrain=None)
    _raises("constrain_beams=9: must be None, 0 or a width in 1..8", dec, constrain_beams=9)
    _raises("constrain_beams is a parallel-variant option", dec, variant=SEQ2SEQ)
    _raises("constrain_beams needs term_range = (lo, hi) with lo < hi", dec, term_range=(3, 3))
    for k, v in (("retire", True), ("return_pointer", True), ("no_stop", True), ("stop_callback", lambda c: False),
                 ("extra_mask", torch.zeros(1)), ("logprob", True), ("beam_width", 2), ("num_samples", 2)):
        _raises(EXCLUDES, dec, **{k: v})
    _raises("constrain='loops' needs follow_table (ops.follow_table)", dec, follow_table=None)
    _raises("follow_table must be an int32 tensor of shape [2, 8, 1]", dec, follow_table=torch.zeros(2, 8, 2, dtype=torch.int32))
    _raises("constrain_beams=7: must be in 1..8 and at most S = 6",
            lambda: eng.decode(torch.zeros(2, 6, 64), None, None, PARALLEL, **dict(base, constrain="no_repeat", follow_table=None, constrain_beams=7)))


# ---- GPU: the operator -------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return torch.from_numpy(faces.pack_follow_bits(a)).cuda()


def _bits_to_bool(words, L):
    w = words.cpu().numpy().view(np.uint32)
    return ((w[..., np.arange(L) >> 5] >> (np.arange(L) & 31).astype(np.uint32)) & 1).astype(bool)


def _run_operator(c, flags, **kw):
    from faceformer_amd.hip import ops
    lg = c["logits"].clone().cuda()
    t = lambda k: torch.from_numpy(c[k]).cuda()
    L = c["L"]
    vis = _bits(c["visited"]) if L else torch.zeros(c["G"] * c["W"], 0, dtype=torch.int32).cuda()
    fol = _bits(c["follows"]) if L else torch.zeros(c["NW"], 0, 0, dtype=torch.int32).cuda()
    res = ops.beam_constrained_select(lg, t("scores"), t("fin"), t("dead"), t("first"), t("prev"), vis, c["W"], flags, c["ntok"],
                                      follows=fol, memory=c["memory"].cuda(), mask=c["mask"].to(torch.uint8).cuda(), kv_len=c["kv"].cuda(),
                                      groups_per_wireframe=GPW, term_range=c["term"], want_rows=True, want_stats=True, **kw)
    return lg, res


def _check_operator_case(c, flags, seen):
    """One launch against the numpy rule on the kernel's own fp32 logits.  Returns (groups, groups left out as indecisive)."""
    G, W, S, L, ntok = c["G"], c["W"], c["S"], c["L"], c["ntok"]
    B = G * W
    what = (S, W, G, flags)
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_operator(c, flags, counter=counter)
    own, raw = lg.cpu().numpy(), c["logits"].numpy()
    want = rule_on_case(c, flags)
    got = {k: res[k].cpu().numpy() for k in ("parent", "next", "scores", "fin", "dead", "first", "prev")}
    vis = _bits_to_bool(res["visited"], L) if L else np.zeros((B, 0), dtype=bool)
    rows = res["mask_rows"].cpu().numpy() != 0
    for b in range(B):                                                   # the byte rows and the FILL pattern: exact, always
        pad = c["pad"][(b // W) // GPW]
        if want["rows"][b] is None:
            assert np.array_equal(own[b], raw[b]), (what, b)              # empty / finished: untouched
            seen["empty" if c["scores"][b] == -np.inf else "finished"] += 1
            continue
        assert np.array_equal(rows[b], want["masked"][b]), (what, b)
        assert np.array_equal(own[b] == np.float32(FILL), want["masked"][b] | pad), (what, b)
        assert np.array_equal(own[b][own[b] != np.float32(FILL)], raw[b][~(want["masked"][b] | pad)]), (what, b)
        st = case_states(c)[b]
        seen["dead" if want["dead_now"][b] else ("open" if (flags & CR.CONNECT and st[1] is not None and st[2] is not None) else "closed")] += 1
        seen["nolive"] += bool((own[b] == np.float32(FILL)).all())
    left = nge = 0
    for gi in range(G):
        sl = slice(gi * W, (gi + 1) * W)
        for r in range(W):                                               # no kept candidate is a masked key: whatever the gaps
            b, p = gi * W + r, int(got["parent"][gi * W + r])
            if got["scores"][b] > -np.inf and not c["fin"][gi * W + p] and not (own[gi * W + p] == np.float32(FILL)).all():
                assert own[gi * W + p, got["next"][b]] > np.float32(FILL), (what, gi, r)
        seen["short"] += int((got["scores"][sl] == -np.inf).any() and (c["scores"][sl] > -np.inf).any())
        if not want["gap"][gi] > 1.0:
            left += 1
            continue
        for k, wk in (("parent", "parent"), ("next", "tok")):
            assert np.array_equal(got[k][sl], want[wk][sl]), (what, gi, k, got[k][sl], want[wk][sl])
        assert np.array_equal(got["fin"][sl] != 0, want["fin"][sl]) and np.array_equal(got["dead"][sl] != 0, want["dead"][sl]), (what, gi)
        f, p, v = CBR.pack_state(want["states"][sl], L)
        assert np.array_equal(got["first"][sl], f) and np.array_equal(got["prev"][sl], p), (what, gi)
        assert np.array_equal(res["visited"][sl].cpu().numpy(), v), (what, gi)
        ws, gs = want["scores"][sl], got["scores"][sl].astype(np.float64)
        assert np.array_equal(np.isinf(ws), np.isinf(gs)), (what, gi)
        fi = ~np.isinf(ws)
        assert (np.abs(gs[fi] - ws[fi]) <= BR.LP_BAR + BR.ADD_EPS * np.abs(ws[fi])).all(), (what, gi, gs, ws)
        nge += int(((want["tok"][sl] >= ntok) & ~(c["fin"][sl][want["parent"][sl]] != 0) & fi).sum())
    if left == 0:
        assert int(counter.item()) == nge, what
    lg2, res2 = _run_operator(c, flags)                                  # two launches: bit-equal
    assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
    return G, left


def _check_width_1_is_pointer_constrained(c, flags):
    from faceformer_amd.hip import ops
    what = (c["S"], c["G"], flags)
    lg, res = _run_operator(c, flags)
    t = lambda k: torch.from_numpy(c[k]).cuda()
    L = c["L"]
    lg1 = c["logits"].clone().cuda()
    one = ops.pointer_constrained(lg1, t("fin"), t("first"), t("prev"), _bits(c["visited"]) if L else torch.zeros(c["G"], 0, dtype=torch.int32).cuda(),
                                  flags, c["ntok"], follows=_bits(c["follows"]) if L else torch.zeros(c["NW"], 0, 0, dtype=torch.int32).cuda(),
                                  memory=c["memory"].cuda(), mask=c["mask"].to(torch.uint8).cuda(), kv_len=c["kv"].cuda(),
                                  seqs_per_group=GPW, term_range=c["term"], want_rows=True, want_stats=True)
    for a, b in (("next", "next"), ("fin", "fin"), ("dead", "dead_end"), ("first", "first"), ("prev", "prev"), ("visited", "visited"),
                 ("rows", "rows"), ("stats", "stats"), ("scores", "logprob"), ("mask_rows", "mask_rows")):
        assert torch.equal(res[a], one[b]), (what, a)                    # (the score bit-equal to the log-probability)
    assert torch.equal(lg, lg1) and not bool(res["parent"].any()), what


@pytest.mark.gpu
@pytest.mark.parametrize("S", OP_S)
def test_operator_against_the_numpy_rule(hip_lib, S):
    seen = dict(open=0, closed=0, dead=0, finished=0, empty=0, nolive=0, short=0)
    groups = left = 0
    for W in OP_W:
        if W > S:
            continue
        for G in OP_G:
            c = operator_case(G, W, S, op_seed(S, W, G))
            for flags in ALL_FLAGS:
                g, l = _check_operator_case(c, flags, seen)
                groups, left = groups + g, left + l
            if W == 1:
                cg = operator_case(G, 1, S, op_seed(S, W, G), greedy=True)
                for flags in ALL_FLAGS:
                    _check_width_1_is_pointer_constrained(cg, flags)
    print("S=%d: %d groups, %d left out as indecisive (%.2f %%); beams by state: %s" % (S, groups, left, 100.0 * left / groups, seen))
    assert left <= CBR.CAP * groups, (S, left, groups)
    if S >= 63:
        assert all(v > 0 for v in seen.values()), seen                   # every state was exercised


@pytest.mark.gpu
def test_operator_inside_poisoned_surroundings(hip_lib):
    """Every operand embedded in poison (tests/redzone.py): the results equal the clean run's and nothing around an operand is
    written."""
    import redzone
    from faceformer_amd.hip import lib as L_, ops
    c = operator_case(9, 4, 65, op_seed(65, 4, 9))
    _, clean = _run_operator(c, LOOPS)
    guard = redzone.Guard()
    e = lambda t, name: redzone.embed(t, guard=guard, name=name)
    B, S, L = 36, 65, c["L"]
    fw = (L + 31) // 32
    lg = e(c["logits"], "logits")
    ins = {k: e(torch.from_numpy(c[k]), k) for k in ("scores", "fin", "dead", "first", "prev")}
    vis, fol = e(_bits(c["visited"]).cpu(), "visited"), e(_bits(c["follows"]).cpu(), "follows")
    mem, mask, kv = e(c["memory"], "memory"), e(c["mask"].to(torch.uint8), "mask"), e(c["kv"], "kv_len")
    i32, f32 = torch.int32, torch.float32
    outs = {k: e(torch.zeros(B, dtype=dt), "out_" + k) for k, dt in (("scores", f32), ("fin", i32), ("dead", i32), ("first", i32), ("prev", i32),
                                                                    ("parent", i32), ("next", i32))}
    ovis, orows = e(torch.zeros(B, fw, dtype=i32), "out_visited"), e(torch.zeros(B, S, dtype=torch.uint8), "mask_rows")
    nrows, nstats = e(torch.zeros(B, 64), "rows"), e(torch.zeros(B, 2, 2), "stats")
    p = lambda t: t.data_ptr()
    d = L_.BeamConstrainedStep(p(lg), S, S, p(mask), p(kv), 9, 4, GPW, p(fol), L, LOOPS, c["ntok"], c["term"][0], c["term"][1],
                               p(ins["scores"]), p(ins["fin"]), p(ins["dead"]), p(ins["first"]), p(ins["prev"]), p(vis),
                               p(outs["scores"]), p(outs["fin"]), p(outs["dead"]), p(outs["first"]), p(outs["prev"]), p(ovis), p(orows),
                               p(outs["parent"]), p(outs["next"]), p(mem), 64, p(nrows), 64, p(nstats), None)
    L_.check(hip_lib.ff_beam_constrained_select(C.byref(d), torch.cuda.current_stream().cuda_stream), "ff_beam_constrained_select")
    torch.cuda.synchronize()
    guard.check()
    for k in outs:
        assert torch.equal(outs[k], clean[k]), k
    assert torch.equal(ovis, clean["visited"]) and torch.equal(nrows, clean["rows"]) and torch.equal(nstats, clean["stats"])
    live = torch.from_numpy((c["scores"] > -np.inf) & (c["fin"] == 0)).cuda()
    assert torch.equal(orows[live], clean["mask_rows"][live])
    for k in ins:                                                        # the inputs are not written
        assert torch.equal(ins[k].cpu(), torch.from_numpy(c[k])), k
    assert torch.equal(vis.cpu(), _bits(c["visited"]).cpu())
    del ops


# ---- GPU: the engine ---------------------------------------------------------------------------------------------------------------------
ENGINE_GOLDENS = ["par_small_gain4", "par_small_ragged", "par_full_n40_gain4"]


def _model(name):
    from test_constrain import _model as model
    return model(name)


def _decode(model, case, batch, **kw):
    from test_logprob import _decode as decode
    return decode(model, case, batch, **kw)


def _cbeam(model, case, b, flags, W, table=None, **kw):
    ft = None if table is None else _bits(table)
    return _decode(model, case, b, constrain=flags, follow_table=ft, constrain_beams=W, term_range=TERM, **kw)


def _step_tols(out, T):
    """tol(step) of a traced decode from its own logits (test_parity_golden._tol), [T - 1]."""
    from test_parity_golden import _tol
    lg = out["logits"].cpu().numpy()
    return np.array([_tol(lg[j]) if j < out["steps"] else 0.0 for j in range(T - 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [LOOPS, CR.NO_REPEAT])
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_at_width_1_is_the_constrained_greedy_decode(hip_lib, name, flags):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T = case["model"]["seq_len"]
    one = _decode(model, case, b, constrain=flags, follow_table=_bits(table), term_range=TERM, trace=True)
    out = _cbeam(model, case, b, flags, 1, table)
    assert out["steps"] == one["steps"] and torch.equal(out["predict"], one["predict"]), (name, flags)
    assert torch.equal(out["beams"], one["predict"]) and torch.equal(out["beam_dead_end"], one["dead_end"]), (name, flags)
    tol = _step_tols(one, T)
    lp = one["logprob"].cpu().numpy().astype(np.float64)
    used = (lp[:, 1:] != 0)
    bound = (used * (2 * tol + CR.LP_BAR)[None, :]).sum(axis=1)
    err = np.abs(out["beam_scores"].cpu().numpy().astype(np.float64) - lp.sum(axis=1))
    print(name, flags, "steps=%d max |score - sum logprob| = %.3g (bound %.3g)" % (out["steps"], err.max(), bound[err.argmax()]))
    assert (err <= bound + 1e-30).all(), (name, flags, err.max())
    assert "logprob" not in out and "dead_end" not in out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_with_both_bits_clear_is_the_plain_beam_decode(hip_lib, name):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    W = 4
    plain = _decode(model, case, b, beam_width=W, term_range=TERM)
    out = _cbeam(model, case, b, 0, W)
    sc = plain["beam_scores"].reshape(-1, W)
    ok = ((sc > -BR.FLT_MAX / 2) | torch.isinf(sc)).all(dim=1)           # groups whose plain beams kept no masked candidate
    assert bool(ok.any())
    print(name, "%d of %d groups compared; steps %d / %d" % (int(ok.sum()), ok.numel(), out["steps"], plain["steps"]))
    if bool(ok.all()):
        assert out["steps"] == plain["steps"]
    T = plain["beams"].shape[1]
    assert torch.equal(out["beams"].reshape(-1, W, T)[ok], plain["beams"].reshape(-1, W, T)[ok]), name
    assert torch.equal(out["beam_scores"].reshape(-1, W)[ok], sc[ok]), name
    assert not bool(out["beam_dead_end"].any())


def _beam_rows(out, W, T):
    return out["beams"].cpu().numpy().reshape(-1, W, T), out["beam_scores"].cpu().numpy().reshape(-1, W), \
        out["beam_dead_end"].cpu().numpy().reshape(-1, W) != 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_loops_beams_are_valid(hip_lib, name):
    """Every non-empty final beam that ends in a terminator without the dead flag passes the enclosure walk; no beam holds an
    edge twice; the scores are non-increasing in k."""
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, F, W = case["model"]["seq_len"], max(ni), 4
    out = _cbeam(model, case, b, LOOPS, W, table)
    beams, scores, dead = _beam_rows(out, W, T)
    assert torch.equal(out["predict"], out["beams"].reshape(-1, W, T)[:, 0])
    ended = 0
    for w, n in enumerate(ni):
        for f in range(n):
            gsc = scores[w * F + f]
            fin_sc = gsc[~np.isinf(gsc)]
            assert (np.diff(fin_sc) <= 0).all() and not np.isinf(gsc[: fin_sc.size]).any(), (name, w, f, gsc)    # empties last
            for k in range(W):
                if np.isinf(gsc[k]):
                    continue
                row = beams[w * F + f, k]
                idx = [int(t) - NTOK for t in row if t >= NTOK]
                assert len(idx) == len(set(idx)), (name, w, f, k, row)
                if ((row >= TERM[0]) & (row < TERM[1])).any() and not dead[w * F + f, k]:
                    face = faces._parallel_rows(row[None], TOK, n)
                    if face:
                        assert faces.is_face_enclosed(edges[w], face[0][1], CR.TOL), (name, w, f, k, row)
                        ended += 1
    print(name, "W=%d: %d closed beams passed the enclosure walk, %d dead-ended beams" % (W, ended, int(dead.sum())))
    assert ended > 0


def _replay(out, flags, table, pad, F, W, T, what):
    """The numpy rule carried along the decode's own traced logits (fp64 state; j x the bound at step j): the FILL pattern always;
    parents, tokens and flags on every (step, group) decisive so far.  A group leaves at its first indecisive step.  Returns
    (pairs, pairs left out, the groups replayed to the end)."""
    logits = out["logits"].cpu().numpy()
    parent = out["beam_parent"].cpu().numpy()
    steps = out["steps"]
    beams, scores, dead = _beam_rows(out, W, T)
    G = beams.shape[0]
    pairs = left = 0
    whole = []
    for gi in range(G):
        w = gi // F
        fol = None if table is None else table[w]
        tok0 = int(beams[gi, 0, 0])
        sc, fin, dd, sts = CBR.start_group(tok0, W, NTOK, TERM, fol)
        toks, pars, alive = [], [], True
        for j in range(steps):
            if fin[~np.isinf(sc)].all():
                break
            pairs += 1
            if not alive:
                left += 1
                continue
            res = CBR.group_step(logits[j, gi * W:(gi + 1) * W].astype(np.float64), pad[w], sc, fin, dd, sts, flags, NTOK, TERM, fol, margin=j + 1)
            for k in range(W):
                if res["rows"][k] is not None:
                    assert np.array_equal(logits[j, gi * W + k] == np.float32(FILL), res["masked"][k] | pad[w]), (what, j, gi, k)
            if not res["gap"] > 1.0:
                alive = False
                left += 1
                continue
            assert np.array_equal(parent[j, gi * W:(gi + 1) * W], res["parent"]), (what, j, gi)
            toks.append(res["tok"]); pars.append(res["parent"])
            sc, fin, dd, sts = res["scores"], res["fin"], res["dead"], res["states"]
        if alive:
            whole.append(gi)
            n = len(toks)
            want = BR.backtrack(np.full(W, tok0), toks, pars, W)
            keep = ~np.isinf(sc)
            assert np.array_equal(beams[gi][:, : n + 1][keep], want[keep]), (what, gi)
            assert np.array_equal(dead[gi][keep], dd[keep]), (what, gi)
            assert (np.abs(scores[gi][keep] - sc[keep]) <= max(n, 1) * (BR.LP_BAR + BR.ADD_EPS * np.abs(sc[keep]))).all(), (what, gi)
    return pairs, left, whole


def _pad_of(b):
    mask = b["input_mask"].cpu().numpy()
    return np.concatenate([np.zeros((mask.shape[0], NTOK), dtype=bool), mask], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_replays_under_the_numpy_rule(hip_lib, name):
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T, F, W = case["model"]["seq_len"], max(lat["num_input"]), 4
    out = _cbeam(model, case, b, LOOPS, W, table, trace=True)
    pairs, left, _ = _replay(out, LOOPS, table, _pad_of(b), F, W, T, name)
    print(name, "steps=%d: %d (step, group) pairs, %d left out (%.2f %%)" % (out["steps"], pairs, left, 100.0 * left / max(1, pairs)))
    assert pairs > 0 and left <= CBR.CAP * pairs, (name, left, pairs)


@pytest.mark.gpu
def test_plan_invariance_and_repeatability(hip_lib):
    name = "par_small_ragged"
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    T, F, W = case["model"]["seq_len"], max(lat["num_input"]), 4
    whole = _cbeam(model, case, b, LOOPS, W, table, trace=True, chunk_wireframes=0)
    again = _cbeam(model, case, b, LOOPS, W, table, trace=True, chunk_wireframes=0)
    for k in ("predict", "beams", "beam_scores", "beam_dead_end", "beam_parent"):
        assert torch.equal(whole[k], again[k]), k                        # one plan, two runs: bit-equal
    assert whole["steps"] == again["steps"]
    one = _cbeam(model, case, b, LOOPS, W, table, trace=True, chunk_wireframes=1)
    pad = _pad_of(b)
    pw, lw, gw = _replay(whole, LOOPS, table, pad, F, W, T, "whole")
    po, lo, go = _replay(one, LOOPS, table, pad, F, W, T, "one")
    both = sorted(set(gw) & set(go))                                     # the groups decisive to the end under both plans
    print("chunk_wireframes = 1 against the whole batch: left out %d of %d and %d of %d pairs; %d of %d groups compared"
          % (lw, pw, lo, po, len(both), whole["beams"].shape[0] // W))
    assert lw <= CBR.CAP * pw and lo <= CBR.CAP * po and both
    bw, sw, dw = _beam_rows(whole, W, T)
    bo, so, do = _beam_rows(one, W, T)
    assert np.array_equal(bw[both], bo[both]) and np.array_equal(dw[both], do[both])
    fi = ~np.isinf(sw[both])
    assert np.array_equal(fi, ~np.isinf(so[both]))
    n = max(whole["steps"], 1)
    assert (np.abs(sw[both][fi] - so[both][fi]) <= 2 * n * (BR.LP_BAR + BR.ADD_EPS * np.abs(sw[both][fi].astype(np.float64)))).all()


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    """The workspace is exactly what the size query reports, filled with 0x00 and with 0xFF, a canary behind it: the results are
    those of the clean run, and nothing behind the workspace is written."""
    from test_workspace_poison import Dirty
    name = "par_small_ragged"
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    W = 4
    clean = _cbeam(model, case, b, LOOPS, W, table, trace=True)
    eng = clean["engine"]
    for fill in (0x00, 0xFF):
        with Dirty([eng], fill=fill) as dirty:
            out = _cbeam(model, case, b, LOOPS, W, table, trace=True)
            dirty.check("%s fill 0x%02x" % (name, fill))
        assert out["steps"] == clean["steps"]
        for k in ("predict", "beams", "beam_scores", "beam_dead_end", "beam_parent"):
            assert torch.equal(out[k], clean[k]), (k, fill)


@pytest.mark.gpu
def test_engine_replays_dead_ends_on_a_sparse_table(hip_lib):
    """The lattice leaves no dead end; a random table of out-degree 0..4 does: the same replay, with dead-ended beams required."""
    name = "par_small_gain4"
    case, z, model, gb, sd, lat, b, edges, _ = _model(name)
    ni = lat["num_input"]
    T, F, W = case["model"]["seq_len"], max(ni), 4
    table = CR.random_follows(len(ni), case["model"]["L"], 5)
    for w, n in enumerate(ni):
        table[w, n:] = False
        table[w, :, n:] = False
    out = _cbeam(model, case, b, LOOPS, W, table, trace=True)
    pairs, left, _ = _replay(out, LOOPS, table, _pad_of(b), F, W, T, (name, "sparse"))
    dead = int(out["beam_dead_end"].sum())
    print(name, "sparse table: steps=%d, %d pairs, %d left out, dead-ended beams: %d" % (out["steps"], pairs, left, dead))
    assert dead > 0 and left <= CBR.CAP * pairs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENGINE_GOLDENS)
def test_engine_against_the_teacher_forced_oracle(hip_lib, name):
    """The fp64 oracle teacher-forced along every non-empty final beam, the rule's mask applied to ITS logits: the beam's score
    within the sum over its steps of 2 tol(step) + 2^-16 of the oracle's summed log_softmax."""
    from test_parity_golden import _tol, _truth_along
    case, z, model, gb, sd, lat, b, edges, table = _model(name)
    ni = lat["num_input"]
    T, F, W = case["model"]["seq_len"], max(ni), 4
    out = _cbeam(model, case, b, LOOPS, W, table)
    beams, scores, dead = _beam_rows(out, W, T)
    steps, pad = out["steps"], _pad_of(b)
    checked, worst = 0, 0.0
    for k in range(W):
        pred = np.ascontiguousarray(beams[:, k])
        truth, _, _ = _truth_along("constrain_beam:" + name, case, sd, lat, dict(predict=pred, steps=steps))
        fin, _ = CR.stop_and_finish(pred, TERM, NTOK)
        for r in range(pred.shape[0]):
            if np.isinf(scores[r, k]):
                continue
            w = r // F
            total = bound = 0.0
            for j in range(min(int(fin[r]), steps)):
                st = CR.state_of_prefix(pred[r, : j + 1], NTOK, table[w])
                masked, _ = CR.rule_mask(st, LOOPS, truth.shape[2], NTOK, TERM, table[w], pad[w])
                row = np.where(masked | pad[w], FILL, truth[j, r])
                m = row.max()
                total += (row[pred[r, j + 1]] - m) - np.log(np.exp(row - m).sum())
                bound += 2 * _tol(row.astype(np.float32)) + CR.LP_BAR
            err = abs(float(scores[r, k]) - total)
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (name, r, k, float(scores[r, k]), total, bound)
            checked += 1
    print(name, "%d beams against the oracle, worst |score - oracle| / bound = %.3g" % (checked, worst))
    assert checked > 0


@pytest.mark.gpu
def test_model_keys_in_batch_order_and_option_off(hip_lib):
    case, z, model, gb, sd, lat, b, edges, table = _model("par_small_ragged")
    T, W = case["model"]["seq_len"], 3
    ni = lat["num_input"]
    N, F = len(ni), max(ni)
    order = sorted(range(N), key=lambda i: -ni[i])
    assert order != list(range(N))                                   # the premise: the model does reorder this batch
    idx = torch.tensor(order, device="cuda")
    by_hand = {k: (v.index_select(0, idx) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in b.items()}
    by_hand["num_input"] = [ni[i] for i in order]
    assert model.constrain_beams == 0
    try:
        with torch.no_grad():
            off = model(dict(b))
            model.constrain = "loops"
            greedy = model(dict(b))
            model.constrain_beams = W
            on = model(dict(b))
            model.constrain_beams = 1
            one = model(dict(b))
            model.constrain_beams, model.sort_by_edges = W, False
            hand = model(dict(by_hand))
    finally:
        model.constrain, model.constrain_beams, model.sort_by_edges = None, 0, True
    new = {"predict_beams", "predict_beam_scores", "predict_beam_dead_end", "predict_dead_end"}
    assert set(on) == set(off) | new and not new & set(off) and "predict_logprob" not in on
    assert tuple(on["predict_beams"].shape) == (N, F, W, T) and on["predict_beams"].dtype == torch.int64
    assert tuple(on["predict_beam_scores"].shape) == tuple(on["predict_beam_dead_end"].shape) == (N, F, W)
    assert tuple(on["predict"].shape) == (N, F, T) and tuple(on["predict_dead_end"].shape) == (N, F)
    assert torch.equal(on["predict"], on["predict_beams"][:, :, 0]) and torch.equal(on["predict_dead_end"], on["predict_beam_dead_end"][:, :, 0])
    for k in new | {"predict"}:
        assert torch.equal(on[k].index_select(0, idx), hand[k]), k       # batch order: the sort undone
    assert torch.equal(one["predict"], greedy["predict"]) and torch.equal(one["predict_dead_end"], greedy["predict_dead_end"])
    assert model.last_decode_stats["constrain_beams"] == W
    with torch.no_grad():
        assert torch.equal(model(dict(b))["predict"], off["predict"]) and set(model(dict(b))) == set(off)      # option off again


# ---- CPU: the models, decode_sharded, the faces helper and the CLI -----------------------------------------------------------------------
def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _tiny_inputs():
    return {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
            "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}


NEEDS = "constrain_beams=2 needs constrain ('no_repeat' or 'loops'): it is the beam search over the constrained keys"


def test_models_and_decode_sharded_reject_before_the_library_is_touched(monkeypatch):
    import types
    from faceformer_amd import dist
    from faceformer_amd.hip import lib
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))
    model = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert model.constrain_beams == 0

    def fwd(m, text, inputs=None, **attrs):
        for k, v in attrs.items():
            setattr(m, k, v)
        with torch.no_grad():
            _raises(text, m.forward_eval, inputs or _tiny_inputs())

    fwd(model, NEEDS, constrain_beams=2)
    fwd(model, "constrain_beams=9: must be None, 0 or a width in 1..8", constrain="loops", constrain_beams=9)
    model.constrain_beams = 2
    for attr, val in (("retire_finished", True), ("beam_width", 2), ("num_samples", 2), ("return_logprob", True)):
        old = getattr(model, attr)
        fwd(model, "constrain excludes beam_width, num_samples, retire_finished, return_logprob and an extra mask", **{attr: val})
        setattr(model, attr, old)
    fwd(model, "constrain excludes beam_width, num_samples, retire_finished, return_logprob and an extra mask",
        dict(_tiny_inputs(), extra_mask=torch.zeros(1, 4, 8, dtype=torch.bool)))
    _raises("score() excludes constrain: set model.constrain = None to score given paths", model.score, _tiny_inputs(),
            torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                 # the sub-module loop
        loop = _tiny_model(SurfaceFormer_Parallel, max_face_length=5, **ctor)
        inputs = _tiny_inputs()
        fwd(loop, "constrain needs the native engine: this model's constructor arguments take the sub-module loop", inputs,
            constrain="loops", constrain_beams=2)
        assert "predict" not in inputs
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    seq.constrain_beams = 2
    sin = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool), "label": torch.zeros(1, 6, dtype=torch.long)}
    with torch.no_grad():
        _raises("constrain_beams is a SurfaceFormer_Parallel option (the single-sequence model emits loops of plain edges)",
                seq.forward_eval, sin)

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    ns = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain="loops", constrain_beams=2)
    _raises("decode_sharded does not implement constrain (a constrained decode takes no external stop rule)", dist.decode_sharded, ns, {}, NoDist())
    ns.constrain = None
    _raises("decode_sharded does not implement constrain_beams (a constrained decode takes no external stop rule)", dist.decode_sharded, ns, {},
            NoDist())


def test_faces_helper_leaves_dead_ended_and_empty_beams_out():
    beams = np.zeros((2, 3, 6), dtype=np.int64)
    beams[0, 0, :4] = [NTOK + 0, NTOK + 1, NTOK + 2, TERM[0]]
    beams[0, 1, :3] = [NTOK + 0, NTOK + 3, TERM[0]]
    beams[0, 2, :3] = [NTOK + 0, NTOK + 2, TERM[0]]
    beams[1, 0, :3] = [NTOK + 1, NTOK + 2, TERM[0] + 1]
    scores = np.array([[-0.5, -1.0, -np.inf], [-0.25, -np.inf, -np.inf]])
    dead = np.array([[0, 1, 0], [0, 0, 0]])
    every = faces.parse_parallel_beams_scored(beams, scores, 8, TOK)
    kept = faces.parse_parallel_constrained_beams_scored(beams, scores, dead, 8, TOK)
    assert [f[1] for f in every] == [(0, 1, 2), (0, 3), (1, 2)] or len(every) == 3
    assert kept == [every[0], every[2]] and np.isfinite(scores[0, 1])                        # (the caller's scores are not written)


def test_cli_flag_reaches_the_model_and_the_record_is_todays_without_it(tmp_path, monkeypatch):
    import json
    import sys
    import types
    sys.path.insert(0, ROOT)
    import main as cli
    from conftest import GOLDEN
    from faceformer_amd import datasets as D
    args = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--constrain", "loops", "--constrain-beams", "4"])
    assert (args.constrain, args.constrain_beams) == ("loops", 4)
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).constrain_beams == 0
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--constrain", "loops", "--constrain-beams", "2", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [(kw["constrain"], kw["constrain_beams"]) for kw in seen] == [("loops", 2), (None, 0)]
    m = cli.configure_model(types.SimpleNamespace(), constrain="loops", constrain_tol=1e-3, constrain_beams=4)
    assert vars(m) == dict(constrain="loops", constrain_tol=1e-3, constrain_beams=4)
    cfg = types.SimpleNamespace(model_class="SurfaceFormer_Parallel")
    run = lambda **kw: run_test(cfg, None, out_dir="unused", device="cpu", model=object(), **kw)
    _raises("--constrain-beams requires --constrain", run, constrain_beams=2)
    _raises("--constrain-beams must be a width in 1..8", run, constrain="loops", constrain_beams=9)
    _raises("--constrain-beams is not implemented for multi-rank runs", run, constrain="loops", constrain_beams=2,
            dist_mod=types.SimpleNamespace(get_world_size=lambda: 2))
    _raises("--constrain applies to SurfaceFormer_Parallel only, and not together with --retire-finished, --scores, --beam, --sample or "
            "--score-labels", run, constrain="loops", constrain_beams=2, beam=2)
    # the record: byte-identical without the flag, the beam keys with it, beam 0's counts unchanged
    gold = json.load(open(os.path.join(GOLDEN, "cli_coedge_case.json")))
    gm = gold["model"]
    cfgm = types.SimpleNamespace(num_points_per_line=50, num_lines=gm["num_lines"], point_dim=2, max_num_faces=42,
                                 max_face_length=gm["max_face_length"], label_seq_length=0, token=TOK)
    cfg = types.SimpleNamespace(model=cfgm, post_process=types.SimpleNamespace(is_coedge=True, enclosedness_tol=gold["tol"]))
    smp = gold["samples"][0]
    dd = tmp_path / "s"
    dd.mkdir()
    json.dump(smp["raw"], open(str(dd / "a.json"), "w"))
    item = D.ABCDataset_Parallel(str(dd), "a.json", cfgm)[0]
    pred = np.asarray(smp["predict"], dtype=np.int64)
    text, st = cli.record_of(cfg, smp["raw"], item, pred, True)
    assert text == cli.record_of(cfg, smp["raw"], item, pred, True, constrained_beams=None)[0]
    dead = np.zeros(pred.shape[0], dtype=np.int32)
    text1, _ = cli.record_of(cfg, smp["raw"], item, pred, True, dead_end=dead)
    Wd = 2
    beams = np.stack([pred, np.roll(pred, 1, axis=0)], axis=1)
    bsc = np.stack([-np.arange(pred.shape[0], dtype=np.float64), -50.0 - np.arange(pred.shape[0])], axis=1)
    bdead = np.zeros((pred.shape[0], Wd), dtype=np.int32)
    bdead[:, 1] = 1                                                                          # every second beam dead-ended: left out
    text2, st2 = cli.record_of(cfg, smp["raw"], item, pred, True, dead_end=dead, constrained_beams=(beams, bsc, bdead))
    rec1, rec2 = json.loads(text1), json.loads(text2)
    assert list(rec2) == list(rec1) + ["pred_beam_faces", "pred_beam_face_scores"] and st2 == st and {k: rec2[k] for k in rec1} == rec1
    n = int(item["num_input"])
    want = sorted(faces.unique_faces_with_scores(faces.parse_parallel_beams_scored(pred[:n, None], bsc[:n, :1], len(smp["raw"]["edges"]), TOK)),
                  key=lambda f: -f[2])
    assert rec2["pred_beam_face_scores"] == [s for _, _, s, _ in want] and len(rec2["pred_beam_faces"]) == len(want)
