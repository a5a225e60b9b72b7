"""Opt-in closure look-ahead of the loop-constrained single-sequence decode (SurfaceFormer.sequence_constrain_closure):
the numpy rule on hand-written traps, its identities and guarantees, every refusal and the CLI on the CPU (library untouched); the
two step operators, the engine's entries and the model on the GPU, through the C ABI.  The rule is faces.sequence_rule_step with
its closure keywords; the decode around it tests/sequence_constrain_closure_ref.py.

Bars (the issue's, none measured): byte rows, tokens, flags, states and visited words are exact; a log-probability lies within
2^-16 + 2^-23 |lp| of fp64 on the kernel's own masked row; a token of an engine decode must equal the rule's on every (step,
unfinished row) pair whose margin between the two best live keys exceeds 2 tol(step) (tol: test_parity_golden._tol); at most 2 % of
a tuple's pairs may be left out -- a condition on the (golden, kind, seed, flags, form) tuples, fixed on the CPU by
tools/sequence_closure_left_out.py."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import sequence_constrain_closure_ref as QC
import sequence_constrain_ref as SC
from conftest import ROOT, batch_to, token_ns
from faceformer_amd import faces
from faceformer_amd.hip.modes import SEQUENCE_CONSTRAIN_AHEAD, sequence_constrain_closure_value   # (the option: without it nothing here can pass)
from test_sequence_constrain import (E_OP, _constrained, _fixture, _operator_case, _seq_inputs, _tiny_model, _untouchable, _words)

TOK = token_ns()
NTOK, SOS, SEP, EOS = TOK.len, TOK.SOS, TOK.SEP, TOK.EOS
FILL = SC.FILL
LOOPS, COEDGE = SC.LOOPS, SC.COEDGE_LOOPS
T_A = QC.table_of(QC.TRAP_A)
T_B = QC.table_of(QC.TRAP_B)


def _mask(state, flags, table, form=None, budget=None, pad=None):
    L = table.shape[0]
    S = NTOK + L
    pad = np.zeros(S, bool) if pad is None else pad
    cd, cl = faces.follow_distance(table, 254)
    kw = {} if form is None else dict(closure=form, budget=budget, close_dist=None if form == "exact" else cd, cycle_len=cl)
    masked, dead = faces.sequence_rule_mask(state, flags, S, NTOK, SEP, EOS, table, pad, **kw)
    return masked, dead, [e for e in range(L) if not masked[NTOK + e]]


# ---- CPU: the numpy rule on the traps -----------------------------------------------------------------------------------------------
def test_trap_a_the_static_distance_passes_through_a_visited_edge():
    assert NTOK == 4
    st = (frozenset({0, 1}), 0, 1)
    cd, _ = faces.follow_distance(T_A, 254)
    assert cd[0].tolist() == [3, 2, 1, 3]
    assert faces.closure_distance(T_A, [0, 1], 0).tolist() == [255, 2, 1, 255]
    assert _mask(st, LOOPS, T_A)[2] == [2, 3]                                   # the plain rule leaves the trap edge live
    after = faces.sequence_rule_advance(st, NTOK + 3, LOOPS, NTOK, SEP, T_A)
    masked, dead, live = _mask(after, LOOPS, T_A)
    assert dead and live == [] and not masked[SEP] and masked[EOS]              # ... a dead end one step later: SEP alone
    for budget in (3, 4, 254):
        assert _mask(st, LOOPS, T_A, "lookahead", budget)[2] == [2, 3]
    assert _mask(st, LOOPS, T_A, "lookahead", 2)[2] == [2]
    for budget in (1, 2, 3, 254):
        assert _mask(st, LOOPS, T_A, "exact", budget)[2] == [2]                 # no path from 3 avoids the visited edge 1


def test_trap_b_once_keeps_an_earlier_faces_edge_out_of_the_search():
    cd, _ = faces.follow_distance(T_B, 254)
    assert cd[0][3] == 2
    once = (frozenset({4, 0, 1}), 0, 1)                                         # edge 4 belongs to an earlier face, kept under ONCE
    fresh = (frozenset({0, 1}), 0, 1)                                           # flags 3: cleared at the SEP
    assert faces.closure_distance(T_B, [4, 0, 1], 0)[3] == 255 and faces.closure_distance(T_B, [0, 1], 0)[3] == 2
    assert _mask(once, COEDGE, T_B, "exact", 5)[2] == [2]
    assert _mask(fresh, LOOPS, T_B, "exact", 5)[2] == [2, 3]
    assert _mask(once, COEDGE, T_B, "lookahead", 5)[2] == _mask(fresh, LOOPS, T_B, "lookahead", 5)[2] == [2, 3]      # the static form cannot tell


def test_budget_zero_and_the_self_closing_edge():
    for form in QC.FORMS:
        for flags in (LOOPS, COEDGE):
            masked, dead, live = _mask((frozenset({0, 1}), 0, 1), flags, T_A, form, 0)       # open: a dead end, SEP alone
            assert dead and live == [] and not masked[SEP] and masked[EOS] and masked[SOS]
            masked, dead, live = _mask((frozenset({0}), None, 0), flags, T_A, form, 0)        # closed with a face behind it: SEP or EOS
            assert not dead and live == [] and not masked[SEP] and not masked[EOS]
            masked, dead, live = _mask(faces.sequence_rule_start(), flags, T_A, form, 0)      # straight after SOS: EOS only
            assert not dead and live == [] and masked[SEP] and not masked[EOS]
        t = QC.self_closing(7)
        assert _mask(faces.sequence_rule_start(), LOOPS, t, form, 1)[2] == [0, 3, 6]          # a self-closing edge is live at budget 1
        assert _mask(faces.sequence_rule_start(), LOOPS, t, form, 0)[2] == []
    with pytest.raises(ValueError, match="closure='exact' needs SEQ_CONNECT \\| SEQ_NO_REPEAT"):
        _mask(faces.sequence_rule_start(), 2, T_A, "exact", 3)
    with pytest.raises(ValueError, match="closure='lookahead' needs SEQ_CONNECT"):
        _mask(faces.sequence_rule_start(), 1, T_A, "lookahead", 3)
    for bad in (-1, 255, True, 2.0):
        with pytest.raises(ValueError, match="budget="):
            _mask(faces.sequence_rule_start(), LOOPS, T_A, "lookahead", bad)
    with pytest.raises(ValueError, match="closure='ahead'"):
        _mask(faces.sequence_rule_start(), LOOPS, T_A, "ahead", 3)
    assert _mask(faces.sequence_rule_start(), 2, T_A, "lookahead", 1)[2] == []                # CONNECT alone takes the static form


def _scripted(table, prefer, T):
    """step_logits of a scripted model: the keys of `prefer` in descending order of preference, everything else level."""
    S = NTOK + table.shape[0]

    def step_logits(paths, step):
        row = np.zeros(S)
        for rank, key in enumerate(prefer):
            row[key] = 10.0 - rank
        return np.tile(row, (paths.shape[0], 1))
    return step_logits


def test_scripted_decode_prefers_the_trap_edge():
    """Trap A with a model that likes edge 0, 1, then the trap edge 3: the plain rule walks into the dead end and abandons the face;
    the forms take edge 2 and complete 0 1 2.  With a short row the plain rule ends open at T; the forms never do."""
    prefer = [NTOK + 0, NTOK + 1, NTOK + 3, NTOK + 2, SEP, EOS]
    for T, forms in ((6, QC.FORMS), (12, ("exact",))):      # (T = 6: budget 2 where the trap edge is offered, which the static form needs)
        cd, cl = QC.tables(T_A[None], T)
        args = (1, T, LOOPS, NTOK, SOS, SEP, EOS, T_A[None])
        plain = QC.decode(_scripted(T_A, prefer, T), *args)
        assert plain["tokens"][0, 1:5].tolist() == [NTOK, NTOK + 1, NTOK + 3, SEP] and plain["dead"][0, 4] == 1      # abandons the face
        assert (0, 4) in QC.late_dead_ends(plain["tokens"], plain["dead"], LOOPS, NTOK, SEP, T_A[None])
        if T == 6:
            assert plain["open_end"].tolist() == [1] and plain["tokens"][0, 5] == NTOK                              # ... and ends open at T
        for form in forms:
            d = QC.decode(_scripted(T_A, prefer, T), *args, form, cd, cl)
            assert d["tokens"][0, 1:4].tolist() == [NTOK, NTOK + 1, NTOK + 2], (T, form)                          # the loop 0 1 2 closes
            assert d["open_end"].tolist() == [0], (T, form)
            assert QC.late_dead_ends(d["tokens"], d["dead"], LOOPS, NTOK, SEP, T_A[None]) == [], (T, form)
            if T == 6:
                assert d["tokens"][0, 4] == SEP and not d["dead"].any()
                assert SC.face_pieces(d["tokens"][0], d["dead"][0], NTOK, SEP, EOS, 4) == [((0, 1, 2), False, False)]
                assert d["tokens"][0, 5] == EOS and d["steps"] == 5                                              # budget 0 after SEP: EOS only
    # T = 3: two positions.  The plain rule opens a loop at position 1 and is open at T; the forms have no edge that closes in time.
    short = (1, 3, LOOPS, NTOK, SOS, SEP, EOS, T_A[None])
    assert QC.decode(_scripted(T_A, prefer, 3), *short)["open_end"].tolist() == [1]
    cd3, cl3 = QC.tables(T_A[None], 3)
    for form in QC.FORMS:
        d = QC.decode(_scripted(T_A, prefer, 3), *short, form, cd3, cl3)
        assert d["open_end"].tolist() == [0] and d["tokens"][0].tolist() == [SOS, EOS, 0], (form, d["tokens"])


def _walks(seed, count=6):
    """(table, flags, states) of random walks of the plain rule on small tables."""
    g = np.random.default_rng([0xC105, seed])
    out = []
    for k in range(count):
        L = int(g.integers(3, 11))
        kind = k % 4
        t = (g.random((L, L)) < 0.3) if kind == 0 else (QC.ring(L) if kind == 1 else (QC.self_closing(L) if kind == 2 else QC.chain(L)))
        if kind == 3:
            t |= g.random((L, L)) < 0.15
        flags = (LOOPS, COEDGE)[k % 2]
        out.append((t, flags, QC.walk_states(t, g, flags, NTOK, SEP, EOS, 3 * L)))
    return out


def test_identities_of_the_numpy_rule():
    seen = dict(stricter=0, open=0, closed=0, dead=0)
    for seed in (1, 2, 3):
        for t, flags, states in _walks(seed):
            L = t.shape[0]
            S = NTOK + L
            pad = np.zeros(S, bool)
            cd, cl = faces.follow_distance(t, 254)
            zero_cd, zero_cl = np.zeros_like(cd), np.zeros_like(cl)
            for st in states:
                plain = faces.sequence_rule_mask(st, flags, S, NTOK, SEP, EOS, t, pad)
                is_open = st[1] is not None and st[2] is not None
                for budget in range(0, L + 1):
                    a = faces.sequence_rule_mask(st, flags, S, NTOK, SEP, EOS, t, pad, closure="lookahead", budget=budget, close_dist=zero_cd,
                                                 cycle_len=zero_cl)
                    assert np.array_equal(a[0], plain[0]) and a[1] == plain[1]                     # (a) zero tables: the plain rule
                    la = faces.sequence_rule_mask(st, flags, S, NTOK, SEP, EOS, t, pad, closure="lookahead", budget=budget, close_dist=cd,
                                                  cycle_len=cl)
                    ex = faces.sequence_rule_mask(st, flags, S, NTOK, SEP, EOS, t, pad, closure="exact", budget=budget, cycle_len=cl)
                    if not (la[1] or ex[1]):
                        assert not (la[0][NTOK:] & ~ex[0][NTOK:]).any()                           # (b) exact contains lookahead
                    else:
                        assert ex[1] or not la[1]                                                 # (a dead end of the static form is one of the exact form)
                    assert not (plain[0][NTOK:] & ~la[0][NTOK:]).any()
                    if not is_open:
                        assert np.array_equal(la[0], ex[0]) and not la[1] and not ex[1]            # (d) a closed state: one byte row
                        seen["closed"] += 1
                    else:
                        seen["open"] += 1
                        seen["stricter"] += bool((ex[0][NTOK:] & ~la[0][NTOK:]).any())
                        seen["dead"] += ex[1]
                        # the live edge set under "exact" equals what an exhaustive search over simple continuations finds
                        vis = np.zeros(L, bool)
                        vis[sorted(st[0])] = True
                        want = [b for b in range(L) if t[st[2], b] and not vis[b] and QC.can_close(t, ~vis, st[1], b, budget)]
                        got = [] if ex[1] else [b for b in range(L) if not ex[0][NTOK + b]]
                        assert got == want, (seed, flags, st, budget, got, want)
                # (c) temperature 0: the draw is the greedy step, under either form
                raw = np.random.default_rng([seed, L, len(st[0])]).standard_normal(S) * 3
                for form in QC.FORMS:
                    kw = QC.closure_kw(form, cd[None], cl[None], 0, min(L, 5))
                    g = faces.sequence_rule_step(raw, pad, st, flags, NTOK, SEP, EOS, t, **kw)
                    s = faces.sequence_rule_sample_step(raw, pad, st, flags, NTOK, SEP, EOS, 0.37, 0.0, 0, 1.0, t, **kw)
                    assert (g["tok"], g["dead"], g["fin"], g["state"]) == (s["tok"], s["dead"], s["fin"], s["state"])
                    assert abs(g["logprob"] - s["logprob"]) < 1e-12
    assert all(seen.values()), seen


def test_guarantees_of_the_numpy_decode_on_random_tables():
    """(g1) no loop open at the end under either form, (g2) no late dead end under "exact", on decodes of a random scripted model --
    where the plain rule has both."""
    counts = dict(plain_open=0, plain_late=0)
    for seed in range(12):
        g = np.random.default_rng([0x61, seed])
        L, T = int(g.integers(5, 12)), int(g.integers(6, 16))
        t = g.random((L, L)) < 0.25
        pref = g.standard_normal((T, NTOK + L)) * 2
        pref[:, EOS] -= 4
        step = lambda paths, s: np.tile(pref[s], (paths.shape[0], 1))
        cd, cl = QC.tables(t[None], T)
        for flags in (LOOPS, COEDGE):
            args = (1, T, flags, NTOK, SOS, SEP, EOS, t[None])
            plain = QC.decode(step, *args)
            counts["plain_open"] += int(plain["open_end"][0])
            counts["plain_late"] += len(QC.late_dead_ends(plain["tokens"], plain["dead"], flags, NTOK, SEP, t[None]))
            for form in QC.FORMS:
                d = QC.decode(step, *args, form, cd, cl)
                assert d["open_end"].tolist() == [0], (seed, flags, form)
                if form == "exact":
                    assert QC.late_dead_ends(d["tokens"], d["dead"], flags, NTOK, SEP, t[None]) == [], (seed, flags)
                for idx, at_dead, unterminated in SC.face_pieces(d["tokens"][0], d["dead"][0], NTOK, SEP, EOS, L):      # (g3)
                    if not at_dead and not unterminated:
                        first = prev = None
                        for e in idx:
                            assert first is None or t[prev, e]
                            first, prev = (e if first is None else first), e
                            first = None if t[e, first] else first
                        assert first is None, (seed, flags, form, idx)
    assert counts["plain_open"] and counts["plain_late"], counts


# ---- CPU: C ABI, binding, records ---------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ff_pointer_sequence_constrained_ahead", "ff_pointer_sequence_constrained_sample_ahead",
               "ff_sequence_decode_constrained_ahead_workspace_bytes", "ff_sequence_decode_constrained_ahead",
               "ff_sequence_decode_constrained_sample_ahead_workspace_bytes", "ff_sequence_decode_constrained_sample_ahead")


def test_header_binding_and_struct_fields_within_abi_105():
    from faceformer_amd.hip import build, lib
    header = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert re.search(r"#define\s+FF_ABI_VERSION\s+105\b", header) and lib.FF_ABI_VERSION == 105
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES, name
        n_args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).count(",") + 1
        assert n_args == len(lib.SIGNATURES[name][1]), name
    S = lib.SIGNATURES
    assert len(S["ff_pointer_sequence_constrained_ahead"][1]) == len(S["ff_pointer_sequence_constrained"][1]) + 4
    assert len(S["ff_pointer_sequence_constrained_sample_ahead"][1]) == len(S["ff_pointer_sequence_constrained_sample"][1]) + 4
    assert S["ff_sequence_decode_constrained_ahead_workspace_bytes"] == S["ff_decode_sequence_constrained_workspace_bytes"]
    assert S["ff_sequence_decode_constrained_sample_ahead_workspace_bytes"] == S["ff_decode_sequence_constrained_sample_workspace_bytes"]
    for struct, cls, base in (("ff_sequence_constrain_ahead_params", lib.SequenceConstrainAheadParams, lib.SequenceConstrainParams),
                              ("ff_sequence_constrain_sample_ahead_params", lib.SequenceConstrainSampleAheadParams,
                               lib.SequenceConstrainSampleParams)):
        fields = re.search(r"typedef struct %s \{(.*?)\}" % struct, code, flags=re.S).group(1)
        names = [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()]
        assert names == [n for n, _ in cls._fields_] == [n for n, _ in base._fields_] + ["form", "close_dist", "cycle_len"]
    doc = header[header.index("closure look-ahead of the loop-constrained single-sequence decode"):
                 header.index("int ff_pointer_sequence_constrained_ahead(")]
    assert "model.py:161-167" in doc and "model.py:193-210" in doc and "model.py:191" in doc      # the reference call sites
    for phrase in ("budget = min(T - 1 - p, 254)", "a loop of more than 254 edges counts as not closable",
                   "close_dist[w][first][b] > budget", "cycle_len[w][b] > budget", "D_V(b -> first) > budget",
                   "an edge an earlier\n *     face used cannot carry this loop home", "The dead-end vote runs after these masks",
                   "and that is not a dead end", "hmax = min(max(T - 2, 1), 254)", "(g1)", "(g2)", "(g3)", "a form outside 1..2"):
        assert phrase in doc, phrase
    assert build.SOURCES[-3:] == ["ff_constrain_seq.hip", "ff_faces.hip", "ff_engine.hip"] and len(build.SOURCES) == 17
    src = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_constrain_seq.hip")).read()
    assert src.count("ff_loop_write_row<FORM>(pa, rule, lane") == 1                             # one call, the plain form's line
    assert "ff_loop_write_row<FF_LOOP_AHEAD>(" not in src and "ff_loop_write_row<FF_LOOP_EXACT>(" not in src and "ff_loop_closure_reach(" not in src
    assert "__syncthreads" not in src and "__shared__" not in src and "asm" not in src          # no barrier, no LDS of its own, plain HIP
    eng = open(os.path.join(ROOT, "faceformer_amd", "csrc", "ff_engine.hip")).read()
    for name in ("ff_sequence_decode_constrained_ahead", "ff_sequence_decode_constrained_sample_ahead"):
        at = eng.index('extern "C" int %s(' % name)
        assert "model.py:161-167, 191, 193-210" in eng[at - 400:at], name                          # each entry cites what it replaces


def test_a_library_without_the_new_entries_is_refused(monkeypatch):
    from faceformer_amd.hip import lib

    class Old:
        def __getattr__(self, name):
            if name in NEW_ENTRIES:
                raise AttributeError(name)
            return types.SimpleNamespace(restype=None, argtypes=None)
    monkeypatch.setattr(lib.C, "CDLL", lambda path: Old())
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib.os.path, "exists", lambda p: True)
    with pytest.raises(lib.HipExtensionError, match="does not export ff_pointer_sequence_constrained_ahead .*rebuild"):
        lib.load()


def test_records_lie_outside_both_tables_and_the_value_check():
    from faceformer_amd.hip import modes
    assert modes.SEQUENCE_CONSTRAIN_AHEAD is SEQUENCE_CONSTRAIN_AHEAD
    for rec in (modes.SEQUENCE_CONSTRAIN_AHEAD, modes.SEQUENCE_CONSTRAIN_SAMPLE_AHEAD):
        assert rec not in modes.MODES and rec not in modes.SEQUENCE_MODES
    assert len(modes.MODES) == 4 and len(modes.SEQUENCE_MODES) == 3                       # the pinned table sizes
    assert modes.SEQUENCE_MODES == (modes.SEQUENCE_SAMPLE, modes.SEQUENCE_BEAM, modes.SEQUENCE_CONSTRAIN)
    a, s = modes.SEQUENCE_CONSTRAIN_AHEAD, modes.SEQUENCE_CONSTRAIN_SAMPLE_AHEAD
    assert a.entry == "ff_sequence_decode_constrained_ahead" and s.entry == "ff_sequence_decode_constrained_sample_ahead"
    assert a.outs == modes.SEQUENCE_CONSTRAIN.outs and s.outs == modes.SEQUENCE_CONSTRAIN_SAMPLE.outs      # the published keys stay
    assert not a.per_anchor and s.per_anchor and s.subject == "sequence_constrain_samples"
    assert a.excludes == modes.SEQUENCE_CONSTRAIN.excludes and a.switches == modes.SEQUENCE_CONSTRAIN.switches
    assert [n for n, _ in a.own] == ["follow_table", "close_dist", "cycle_len"]
    assert [n for n, _ in s.own] == ["follow_table", "uniforms", "close_dist", "cycle_len"]
    v = sequence_constrain_closure_value
    assert v(None, None) is None and v(None, 3) is None
    assert [v("lookahead", f) for f in (2, 3, 6 | 1, 7)] == ["lookahead"] * 4 and [v("exact", f) for f in (3, 7)] == ["exact"] * 2
    for bad in ("ahead", True, 1, 0, ""):
        with pytest.raises(ValueError, match="sequence_constrain_closure=.*must be None, 'lookahead' or 'exact'"):
            v(bad, 3)
    with pytest.raises(ValueError, match="sequence_constrain_closure='exact' needs sequence_constrain \\('loops' or 'coedge_loops'\\)"):
        v("exact", None)
    for flags in (0, 1, 5):
        with pytest.raises(ValueError, match="needs sequence_constrain with FF_CONSTRAIN_CONNECT"):
            v("lookahead", flags)
    with pytest.raises(ValueError, match="sequence_constrain_closure='exact' needs FF_CONSTRAIN_NO_REPEAT as well"):
        v("exact", 2)
    with pytest.raises(ValueError, match="sequence_constrain_closure excludes sequence_constrain_beams"):
        v("lookahead", 3, 2)
    # the recorded texts stay
    with pytest.raises(ValueError, match="constrain_beam_closure='ahead': must be None, 'lookahead' or 'exact'"):
        modes.constrain_beam_closure_value("ahead", 3, 2)
    with pytest.raises(ValueError, match="constrain_lookahead needs constrain='loops': it is the closure look-ahead"):
        modes.constrain_lookahead_value(True, None)
    assert modes.sequence_constrain_flags("coedge_loops") == 7


# ---- CPU: every refusal -------------------------------------------------------------------------------------------------------------
def test_path_engine_decode_rejects_before_the_library_is_touched(monkeypatch):
    from faceformer_amd.hip import engine
    lib = _untouchable(monkeypatch)
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes = {}
    eng.num_token = NTOK
    memory = torch.zeros(2, 12, 64)
    ft = torch.zeros(2, 8, 1, dtype=torch.int32)
    cd, cl = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, dtype=torch.uint8)
    ok = dict(T=300, F=1, sequence_constrain="loops", tok_sep=SEP, follow_table=ft, sequence_constrain_closure="lookahead", close_dist=cd,
              cycle_len=cl)
    dec = lambda **kw: eng.decode(memory, None, None, kw.pop("variant", lib.FF_SEQ2SEQ), **kw)
    with pytest.raises(ValueError, match="needs sequence_constrain \\('loops' or 'coedge_loops'\\)"):
        dec(**dict(ok, sequence_constrain=None))
    for value in ("no_repeat", 0, 1, 5):
        with pytest.raises(ValueError, match="needs sequence_constrain with FF_CONSTRAIN_CONNECT"):
            dec(**dict(ok, sequence_constrain=value))
    with pytest.raises(ValueError, match="'exact' needs FF_CONSTRAIN_NO_REPEAT as well"):
        dec(**dict(ok, sequence_constrain=2, sequence_constrain_closure="exact"))
    with pytest.raises(ValueError, match="sequence_constrain_closure excludes sequence_constrain_beams"):
        dec(**dict(ok, sequence_constrain_beams=2))
    for bad in ("ahead", True, 2):
        with pytest.raises(ValueError, match="sequence_constrain_closure=.*must be None, 'lookahead' or 'exact'"):
            dec(**dict(ok, sequence_constrain_closure=bad))
    with pytest.raises(ValueError, match="is a single-sequence option"):
        dec(variant=lib.FF_PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
    for change in (dict(retire=True), dict(return_pointer=True), dict(no_stop=True), dict(stop_callback=lambda c: False),
                   dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8)), dict(logprob=True), dict(beam_width=2), dict(num_samples=2),
                   dict(constrain="no_repeat"), dict(sequence_samples=2), dict(sequence_beams=2)):
        for more in ({}, dict(sequence_constrain_samples=2, uniforms=torch.zeros(299, 4))):
            with pytest.raises(ValueError, match="excludes"):                             # everything sequence_constrain excludes
                dec(**dict(ok, **change, **more))
    with pytest.raises(ValueError, match="excludes stop_each_eos"):
        dec(flags=engine.DEFAULT_FLAGS | lib.FF_STOP_EACH_EOS, **ok)
    with pytest.raises(ValueError, match="sequence_constrain_closure='lookahead' needs close_dist and cycle_len"):
        dec(**dict(ok, close_dist=None))
    with pytest.raises(ValueError, match="sequence_constrain_closure='lookahead' needs close_dist and cycle_len"):
        dec(**dict(ok, cycle_len=None))
    with pytest.raises(ValueError, match="sequence_constrain_closure='exact' needs cycle_len"):
        dec(**dict(ok, sequence_constrain_closure="exact", cycle_len=None, close_dist=None))
    for name, bad, shape in (("close_dist", torch.zeros(2, 8, 7, dtype=torch.uint8), "2, 8, 8"), ("close_dist", torch.zeros(2, 8, 8), "2, 8, 8"),
                             ("cycle_len", torch.zeros(1, 8, dtype=torch.uint8), "2, 8"), ("cycle_len", cl.int(), "2, 8"),
                             ("cycle_len", [[0] * 8] * 2, "2, 8")):
        with pytest.raises(ValueError, match="%s must be a uint8 tensor of shape \\[%s\\]" % (name, shape)):
            dec(**dict(ok, **{name: bad}))
    with pytest.raises(ValueError, match="follow_table must be an int32 tensor"):
        dec(**dict(ok, follow_table=ft.float()))
    big = torch.zeros(1, 2049, 64)                                                            # 2049 keys: above the exact search's limit
    with pytest.raises(ValueError, match="sequence_constrain_closure='exact' takes at most 2044 edges per wireframe \\(got 2045\\)"):
        eng.decode(big, None, None, lib.FF_SEQ2SEQ, T=5, F=1, sequence_constrain="loops", tok_sep=SEP,
                   follow_table=torch.zeros(1, 2045, 64, dtype=torch.int32), sequence_constrain_closure="exact",
                   cycle_len=torch.zeros(1, 2045, dtype=torch.uint8))
    # the recorded refusals stay what they are
    with pytest.raises(ValueError, match="constrain_lookahead takes T <= 256"):
        eng.decode(memory, None, None, lib.FF_PARALLEL, T=300, F=4, num_input=[4, 3], constrain="loops", term_range=(1, 4), follow_table=ft,
                   constrain_lookahead=True, close_dist=cd, cycle_len=cl)
    with pytest.raises(ValueError, match="sequence_constrain_samples=2 needs sequence_constrain"):
        dec(T=5, F=1, sequence_constrain_samples=2)


def test_models_dist_and_score_reject_before_the_library_is_touched(monkeypatch):
    from faceformer_amd import dist
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    _untouchable(monkeypatch)
    par = _tiny_model(SurfaceFormer_Parallel, max_face_length=5)
    assert par.sequence_constrain_closure is None
    inputs = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
              "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}
    par.sequence_constrain_closure = "exact"
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_closure is a SurfaceFormer option .*constrain_lookahead / constrain_exact"):
        par.forward_eval(inputs)
    seq = _tiny_model(SurfaceFormer, label_seq_length=6)
    assert seq.sequence_constrain_closure is None
    seq.sequence_constrain_closure = "lookahead"
    with torch.no_grad(), pytest.raises(ValueError, match="needs sequence_constrain \\('loops' or 'coedge_loops'\\)"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain = "no_repeat"
    with torch.no_grad(), pytest.raises(ValueError, match="needs sequence_constrain with FF_CONSTRAIN_CONNECT"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain, seq.sequence_constrain_closure = 2, "exact"
    with torch.no_grad(), pytest.raises(ValueError, match="'exact' needs FF_CONSTRAIN_NO_REPEAT as well"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain, seq.sequence_constrain_closure = "loops", "ahead"
    with torch.no_grad(), pytest.raises(ValueError, match="must be None, 'lookahead' or 'exact'"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_closure = "exact"
    seq.sequence_constrain_beams = 2
    with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain_closure excludes sequence_constrain_beams"):
        seq.forward_eval(_seq_inputs())
    seq.sequence_constrain_beams = 0
    for attr, val, off in (("sequence_samples", 2, 0), ("sequence_beams", 2, 0), ("return_logprob", True, False), ("stop_each_eos", True, False)):
        setattr(seq, attr, val)
        with torch.no_grad(), pytest.raises(ValueError, match="excludes"):                # everything sequence_constrain excludes
            seq.forward_eval(_seq_inputs())
        setattr(seq, attr, off)
    for name, bad in (("close_dist", torch.zeros(1, 8, 7, dtype=torch.uint8)), ("cycle_len", torch.zeros(1, 8))):
        seq.sequence_constrain_closure = "lookahead"
        with torch.no_grad(), pytest.raises(ValueError, match="%s must be uint8" % name):
            seq.forward_eval(_seq_inputs(**{name: bad}))
    seq.sequence_constrain_closure = "exact"
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    seq.sequence_constrain = None
    with pytest.raises(ValueError, match="score\\(\\) excludes sequence_constrain_closure"):
        seq.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    wide = _tiny_model(SurfaceFormer, label_seq_length=6, num_lines=2045)                   # more than 2048 keys: before the encoder runs
    wide.sequence_constrain, wide.sequence_constrain_closure = "loops", "exact"
    with torch.no_grad(), pytest.raises(ValueError, match="'exact' takes at most 2044 edges per wireframe \\(got 2045\\)"):
        wide.forward_eval({"input": torch.zeros(1, 2045, 50, 2), "input_mask": torch.zeros(1, 2045, dtype=torch.bool),
                           "label": torch.zeros(1, 6, dtype=torch.long)})
    for ctor in (dict(activation="gelu"), dict(normalize_before=False)):                  # the sub-module loop
        sub = _tiny_model(SurfaceFormer, label_seq_length=6, **ctor)
        sub.sequence_constrain, sub.sequence_constrain_closure = "loops", "lookahead"
        with torch.no_grad(), pytest.raises(ValueError, match="sequence_constrain needs the native engine"):
            sub.forward_eval(_seq_inputs())

    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    model = types.SimpleNamespace(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, sequence_constrain=None,
                                  sequence_constrain_closure="exact")
    with pytest.raises(ValueError, match="decode_sharded does not implement sequence_constrain_closure"):
        dist.decode_sharded(model, {}, NoDist())
    model.sequence_constrain_closure = None
    with pytest.raises(AssertionError, match="process group touched"):
        dist.decode_sharded(model, {}, NoDist())


def test_cli_flags_reach_the_model_and_every_refusal_raises(monkeypatch):
    sys.path.insert(0, ROOT)
    import main as cli
    a = cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain", "coedge_loops", "--sequence-constrain-closure", "exact"])
    assert a.sequence_constrain == "coedge_loops" and a.sequence_constrain_closure == "exact"
    assert cli.build_parser().parse_args(["--test_ckpt", "x.ckpt"]).sequence_constrain_closure is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--test_ckpt", "x.ckpt", "--sequence-constrain-closure", "ahead"])
    seen, run_test = [], cli.run_test
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--sequence-constrain", "loops", "--sequence-constrain-closure", "lookahead", "--sequence-constrain-samples", "3",
              "--test_ckpt", "unused.ckpt"])
    cli.main(["--sequence-constrain", "loops", "--test_ckpt", "unused.ckpt"])
    assert [(kw["sequence_constrain"], kw["sequence_constrain_closure"], kw["sequence_constrain_samples"]) for kw in seen] == \
        [("loops", "lookahead", 3), ("loops", None, 0)]
    m = cli.configure_model(types.SimpleNamespace(), sequence_constrain_closure="exact")
    assert vars(m) == dict(sequence_constrain_closure="exact")
    plain = types.SimpleNamespace()
    cli.configure_model(plain, sequence_constrain="loops")
    assert vars(plain) == dict(sequence_constrain="loops")                                   # without the flag: what it was
    seqcfg = types.SimpleNamespace(model_class="SurfaceFormer")
    call = dict(out_dir="unused", device="cpu", model=object())
    with pytest.raises(ValueError, match="--sequence-constrain-closure requires --sequence-constrain \\{loops,coedge_loops\\}"):
        run_test(seqcfg, None, sequence_constrain_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-closure requires --sequence-constrain loops or coedge_loops: no_repeat"):
        run_test(seqcfg, None, sequence_constrain="no_repeat", sequence_constrain_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-closure is not implemented with --sequence-constrain-beams"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_beams=2, sequence_constrain_closure="exact", **call)
    with pytest.raises(ValueError, match="--sequence-constrain-closure must be lookahead or exact"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_closure="ahead", **call)
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    with pytest.raises(ValueError, match="--sequence-constrain-closure is not implemented for multi-rank runs"):
        run_test(seqcfg, None, sequence_constrain="loops", sequence_constrain_closure="exact", dist_mod=world2, **call)
    with pytest.raises(ValueError, match="--sequence-constrain applies to SurfaceFormer only"):      # an existing text, unchanged
        run_test(types.SimpleNamespace(model_class="SurfaceFormer_Parallel"), None, sequence_constrain="loops", sequence_constrain_closure="exact",
                 **call)
    with pytest.raises(ValueError, match="--sequence-constrain-beams requires --sequence-constrain"):
        run_test(seqcfg, None, sequence_constrain_beams=2, **call)


def test_the_c_entries_refuse_before_any_launch(monkeypatch):
    """The two decode entries through test_entry_checks' machinery (no GPU: an entry rejects bad arguments before any HIP call):
    everything the plain entries refuse in their order, then the form, the look-ahead's flags and tables, the key limit of the
    exact search -- and T = 300 is accepted, where the parallel look-ahead entries refuse T > 256."""
    import test_entry_checks as TE
    from faceformer_amd.hip import lib as L
    lib = L.load()
    D = TE.DUMMY
    form = ("form", {("prm", "form"): 3})
    tables = ("ahead_tables", {("prm", "close_dist"): None})
    sample_outs = ("samples", "logprob", "scores", "dead_end", "open_end", "predict_logprob", "predict_dead_end", "predict_open_end")
    new = {
        "ff_sequence_decode_constrained_ahead[ahead]": (
            "seq", L.SequenceConstrainAheadParams,
            TE.rule_fields(tok_sep=2, open_end=D, form=1, close_dist=D, cycle_len=D, **TE.CON_OUT),
            TE.HEAD_SEQ + TE.SEQ_RULE + [form, TE.AHEAD[0], tables, TE.outputs("open_end")]),
        "ff_sequence_decode_constrained_ahead[exact]": (
            "seq", L.SequenceConstrainAheadParams, TE.rule_fields(tok_sep=2, open_end=D, form=2, cycle_len=D, **TE.CON_OUT),
            TE.HEAD_SEQ + TE.SEQ_RULE + [form, TE.EXACT[0], TE.EXACT[1], TE.EXACT[3], TE.outputs("open_end")]),
        "ff_sequence_decode_constrained_sample_ahead[ahead]": (
            "seq", L.SequenceConstrainSampleAheadParams,
            TE.rule_fields(tok_sep=2, form=1, close_dist=D, cycle_len=D, **TE.draw_fields(*sample_outs)),
            TE.HEAD_SEQ + [TE.SAMPLES] + TE.SEQ_RULE + [form, TE.AHEAD[0], tables, TE.outputs("predict_open_end"), TE.SIZES, TE.DRAW]),
        "ff_sequence_decode_constrained_sample_ahead[exact]": (
            "seq", L.SequenceConstrainSampleAheadParams, TE.rule_fields(tok_sep=2, form=2, cycle_len=D, **TE.draw_fields(*sample_outs)),
            TE.HEAD_SEQ + [TE.SAMPLES] + TE.SEQ_RULE + [form, TE.EXACT[0], TE.EXACT[1], TE.EXACT[3], TE.outputs("predict_open_end"),
                                                        TE.SIZES, TE.DRAW]),
    }
    own = {"form": "form=3 must be 1 (look-ahead) or 2 (exact)", "form:0": "form=0 must be 1 (look-ahead) or 2 (exact)",
           "ahead_flags": "the look-ahead needs FF_CONSTRAIN_CONNECT", "ahead_tables": "close_dist and cycle_len are required",
           "ahead_tables:cycle_len": "close_dist and cycle_len are required",
           "exact_flags": "the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT",
           "exact_flags:no_repeat_only": "the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT",
           "exact_table": "cycle_len is required", "exact_L": "L=2045 above 2044 (L + num_token keys at most 2048)"}
    monkeypatch.setitem(TE.ALTERNATIVES, (None, "form"), [("0", {("prm", "form"): 0})])
    for entry, rec in new.items():
        monkeypatch.setitem(TE.CHECKS, entry, rec)
    for entry, rec in new.items():
        name = entry.split("[")[0]
        plain = name.replace("_ahead", "").replace("ff_sequence_decode_", "ff_decode_sequence_")      # the plain entry, whose texts are recorded
        seen = set()
        for case in TE.case_ids():
            if case.split("/")[0] != entry:
                continue
            rc, text = TE.call(lib, case)
            check = case.split("/")[1]
            first = check.split("+")[0]
            seen.add(first.split(":")[0])
            if check == "pass":
                assert (rc, text) == (-1, "ff_decode: null pointer"), case                 # handed on to the decode: accepted
            elif first in own or first.split(":")[0] in own:
                assert (rc, text) == (-1, "%s: %s" % (name, own.get(first, own[first.split(":")[0]]))), (case, text)
            else:      # a check the plain entry makes: its recorded text under this entry's name
                want = TE.EXPECTED["%s/%s" % (plain, check)] if "%s/%s" % (plain, check) in TE.EXPECTED else None
                if want is None:      # (a pair whose later half is one of this entry's own checks: the earlier one reports)
                    want = TE.EXPECTED["%s/%s" % (plain, first)]
                words = want[1].replace(plain + ":", name + ":")      # ... with this entry's noun and sibling
                if "sample" in name:
                    words = words.replace("or constrain sample params", "or look-ahead sample params")
                else:
                    words = words.replace("or constrain params", "or look-ahead params").replace(
                        "the parallel variant has ff_decode_constrained", "the parallel variant has ff_decode_constrained_ahead")
                assert (rc, text) == (want[0], words), (case, text)
        assert {"form", "outputs", "rule_flags", "variant"} <= seen, (entry, seen)
    # T above 256 is accepted (the step clamps the budget)
    monkeypatch.setitem(TE.CHECKS, "ff_sequence_decode_constrained_ahead[long]",
                        new["ff_sequence_decode_constrained_ahead[ahead]"][:3] + ([("T", {("p", "T"): 300})],))
    assert TE.call(lib, "ff_sequence_decode_constrained_ahead[long]/T") == (-1, "ff_decode: null pointer")
    monkeypatch.setitem(TE.CHECKS, "ff_decode_constrained_ahead[long]", TE.CHECKS["ff_decode_constrained_ahead"][:3] + ([("T", {("p", "T"): 300})],))
    assert "T=300 above 256" in TE.call(lib, "ff_decode_constrained_ahead[long]/T")[1]      # the recorded refusal stays
    # the size queries equal the plain ones, and refuse what they refuse
    m, p = TE.model(False), L.DecodeParams()
    p.N, p.L, p.T, p.sync_every, p.tok_sos, p.tok_eos, p.variant, p.F, p.flags = TE.N, TE.EDGES, TE.T, 4, 0, 1, L.FF_SEQ2SEQ, 1, TE.SEQ_FLAGS
    q = lambda name, *a: getattr(lib, name)(m, p, *a)
    assert q("ff_sequence_decode_constrained_ahead_workspace_bytes") == q("ff_decode_sequence_constrained_workspace_bytes") > 0
    for R in (1, 16):
        assert q("ff_sequence_decode_constrained_sample_ahead_workspace_bytes", R) == \
            q("ff_decode_sequence_constrained_sample_workspace_bytes", R) > 0
    assert q("ff_sequence_decode_constrained_sample_ahead_workspace_bytes", 65) == 0
    assert q("ff_sequence_decode_constrained_sample_ahead_workspace_bytes", 0) == 0
    assert lib.ff_sequence_decode_constrained_ahead_workspace_bytes(None, p) == 0 and lib.ff_sequence_decode_constrained_ahead_workspace_bytes(m, None) == 0
    assert lib.ff_sequence_decode_constrained_sample_ahead_workspace_bytes(None, p, 3) == 0
    for field in ("N", "T"):
        old = getattr(p, field)
        setattr(p, field, 0)
        assert q("ff_sequence_decode_constrained_ahead_workspace_bytes") == q("ff_decode_sequence_constrained_workspace_bytes")
        setattr(p, field, old)
    p.variant = L.FF_PARALLEL
    assert q("ff_sequence_decode_constrained_ahead_workspace_bytes") == 0


# ---- GPU: the two step operators ----------------------------------------------------------------------------------------------------
TABLE_KINDS = ("lattice", "ring", "chain", "self_closing", "random", "trap_a", "trap_b")
BUDGETS = (0, 1, 2, 5, 254)
DRAWS = ((1.0, 0, 1.0), (0.8, 16, 0.9), (0.0, 0, 1.0))


def _table_of_kind(kind, L, seed):
    import constrain_ref as CR
    if kind == "lattice":
        polys, _ = CR.lattice_edges(L, seed) if L else ([], None)
        pts = np.array([[p[0][:2], p[-1][:2]] for p in polys], dtype=np.float32).reshape(L, 2, 2)
        return faces.follow_table((pts[:, 0], pts[:, 1]), SC.TOL)
    if kind == "ring":
        return QC.ring(L)
    if kind == "chain":
        return QC.chain(L)
    if kind == "self_closing":
        return QC.self_closing(L)
    if kind == "random":
        return CR.random_follows(1, L, seed)[0]
    pairs = QC.TRAP_A if kind == "trap_a" else QC.TRAP_B
    return QC.table_of(pairs, L) if L > max(max(p) for p in pairs) else np.zeros((L, L), bool)


def _closure_case(B, S, spg, seed, kind, once, hmax=254):
    """test_sequence_constrain's operator case (logits, kv_len, padding mask, memory, one state per row in the kinds of its KINDS)
    on tables of `kind`, the states re-made for them: an open or dead row is a state of a random walk of the plain rule on its
    wireframe's table where the walk has one, every third row much visited (as late in a row under ONCE), and on the traps row 0
    is the trap's own state with the trap edge preferred."""
    c = _operator_case(B, S, spg, seed)
    L, W = c["L"], c["W"]
    g = np.random.default_rng([0xC1, seed, B, S, spg])
    c["table"] = np.stack([_table_of_kind(kind, L, seed + w) for w in range(W)]) if L else np.zeros((W, 0, 0), bool)
    flags = COEDGE if once else LOOPS
    for b in range(B):
        w = b // spg
        if c["kinds"][b] in ("open", "dead") and L:
            walk = [st for st in QC.walk_states(c["table"][w], g, flags, NTOK, SEP, EOS, min(3 * L, 40)) if st[1] is not None]
            if walk:
                vis, first, prev = walk[int(g.integers(0, len(walk)))]
                c["first"][b], c["prev"][b], c["visited"][b] = first, prev, set(vis)
            if c["kinds"][b] == "dead":
                c["visited"][b] |= set(np.flatnonzero(c["table"][w, c["prev"][b]]).tolist())
        if b % 3 == 2 and L:
            c["visited"][b] |= set(np.flatnonzero(g.random(L) < 0.7).tolist())
    if kind in ("trap_a", "trap_b") and L >= 5:
        c["fin"][0], c["first"][0], c["prev"][0] = 0, 0, 1
        c["visited"][0] = {0, 1} | ({4} if kind == "trap_b" and once else set())
        c["mask"][0, NTOK:NTOK + 5] = False
        c["pad"][0, NTOK:NTOK + 5] = False
        c["logits"][0] = -5.0
        c["logits"][0, NTOK + 3], c["logits"][0, NTOK + 2] = 9.0, 8.0
        c["kinds"][0] = "trap"
    cd, cl = faces.follow_distance(c["table"], hmax) if L else (np.zeros((W, 0, 0), np.uint8), np.zeros((W, 0), np.uint8))
    c["close_dist"], c["cycle_len"], c["flags"] = cd, cl, flags
    return c


def _run_closure(c, form, budget, draw=None, tables=None, counter=None, plain=False):
    from faceformer_amd.hip import ops
    lg = torch.from_numpy(c["logits"]).clone().cuda()
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    cd, cl = tables if tables is not None else (c["close_dist"], c["cycle_len"])
    args = (dev(c["fin"]), dev(c["first"]), dev(c["prev"]), dev(_words(c["visited"], c["L"])), c["flags"], NTOK, SEP, EOS)
    kw = dict(memory=dev(c["memory"]), mask=dev(c["mask"].astype(np.uint8)), kv_len=dev(c["kv"]), seqs_per_group=c["spg"], want_rows=True,
              want_stats=True, counter=counter)
    follows = dev(faces.pack_follow_bits(c["table"]))
    if draw is not None:
        u, (tau, k, pp) = draw
        kw.update(temperature=tau, top_k=k, top_p=pp)
    if plain:
        res = ops.pointer_sequence_constrained(lg, *args, follows=follows, **kw) if draw is None else \
            ops.pointer_sequence_constrained_sample(lg, dev(u), *args, follows=follows, **kw)
    elif draw is None:
        res = ops.pointer_sequence_constrained_ahead(lg, *args, follows, form, dev(cl), budget, close_dist=dev(cd), **kw)
    else:
        res = ops.pointer_sequence_constrained_sample_ahead(lg, dev(u), *args, follows, form, dev(cl), budget, close_dist=dev(cd), **kw)
    return lg, res


def _check_closure(c, form, budget, seen, draw=None):
    from faceformer_amd.hip import ops
    B, S, L, spg, flags = c["B"], c["S"], c["L"], c["spg"], c["flags"]
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    lg, res = _run_closure(c, form, budget, draw, counter=counter)
    what = (S, B, spg, flags, form, budget, draw and draw[1])
    own = lg.cpu().numpy()
    got = {k: res[k].cpu().numpy() for k in ("next", "logprob", "fin", "dead_end", "first", "prev", "visited", "mask_rows")}
    unfinished_after = 0
    for b in range(B):
        w = b // spg
        none = lambda v: None if v < 0 else int(v)
        state = (frozenset(c["visited"][b]), none(c["first"][b]), none(c["prev"][b]))
        kw = QC.closure_kw(form, c["close_dist"], c["cycle_len"], w, budget)
        fin = bool(c["fin"][b])
        masked, dead = (np.zeros(S, bool), False) if fin else \
            faces.sequence_rule_mask(state, flags, S, NTOK, SEP, EOS, c["table"][w], c["pad"][w], **kw)
        assert np.array_equal(got["mask_rows"][b] != 0, masked), (what, b, c["kinds"][b])           # the byte row, exact
        if fin:
            assert np.array_equal(own[b], c["logits"][b]), (what, b)
        else:
            assert np.array_equal(own[b] <= FILL, masked | c["pad"][w]), (what, b)                   # the FILL pattern
            live = own[b] > FILL
            assert np.array_equal(own[b][live], c["logits"][b][live]), (what, b)
        # the numpy rule on the kernel's own masked row: token, flags, state, visited words exact; the log-probability to the bar
        row = own[b].astype(np.float64)
        if draw is None:
            again = faces.sequence_rule_step(row, row <= FILL, state, 0, NTOK, SEP, EOS, None, finished=fin)
        else:
            again = faces.sequence_rule_sample_step(row, row <= FILL, state, 0, NTOK, SEP, EOS, draw[0][b], *draw[1], None, finished=fin)
        tok = int(got["next"][b])
        if draw is None or draw[1][0] == 0:
            assert tok == again["tok"], (what, b, tok, again["tok"])
        elif not fin:      # a draw on fp32 sums: a live key the sampling rule keeps (the draw itself is ff_sample_draw's, tested with it)
            assert row[tok] > FILL, (what, b)
            again = dict(again, tok=tok, fin=tok == EOS,
                         logprob=max(float((row[tok] - row.max()) - np.log(np.exp(row - row.max()).sum())), FILL))
        assert bool(got["dead_end"][b]) == dead and bool(got["fin"][b]) == (fin or tok == EOS), (what, b, c["kinds"][b])
        vis, nf, npv = state if fin else faces.sequence_rule_advance(state, tok, flags, NTOK, SEP, c["table"][w])
        assert (got["first"][b], got["prev"][b]) == (-1 if nf is None else nf, -1 if npv is None else npv), (what, b, c["kinds"][b])
        if L:
            assert np.array_equal(got["visited"][b], _words([vis], L)[0]), (what, b, c["kinds"][b])
        lp = float(got["logprob"][b])
        assert abs(lp - again["logprob"]) <= SC.LP_BAR + SC.EPS * abs(again["logprob"]), (what, b, lp, again["logprob"])
        if fin:
            assert tok == 0 and lp == 0.0
            continue
        unfinished_after += tok != EOS
        plain_masked, _ = faces.sequence_rule_mask(state, flags, S, NTOK, SEP, EOS, c["table"][w], c["pad"][w])
        seen["stricter"] += bool((masked[NTOK:] & ~plain_masked[NTOK:] & ~c["pad"][w][NTOK:]).any())
        seen["dead"] += dead
        seen["closing"] += tok >= NTOK and nf is None
    assert int(counter.item()) == unfinished_after, (what, int(counter.item()), unfinished_after)
    mem = torch.from_numpy(c["memory"]).cuda()
    assert torch.equal(res["rows"], ops.gather_rows(mem, res["next"], seqs_per_group=spg)), what      # the appended rows
    lg2, res2 = _run_closure(c, form, budget, draw)                                                  # two launches
    assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(lg, lg2), what
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("spg", [1, 4])
@pytest.mark.parametrize("S", [5, 65, 260, 1028])
def test_operators_against_the_numpy_rule(hip_lib, S, spg):
    seen = dict(stricter=0, dead=0, closing=0)
    n = 0
    for ki, kind in enumerate(TABLE_KINDS):
        if kind.startswith("trap") and S < 65:
            continue
        for once in (False, True):
            B = (1, 5, 8)[(ki + once) % 3]
            # keep the searches and the tables' builds short: at S = 1028 the tables with long paths run at budget <= 5 only, with
            # distances built to 8 hops (every entry the budgets compare against is exact), and every kind under one of the flags
            short = S >= 1028 and kind in ("ring", "chain", "self_closing")
            if S >= 1028 and once != bool(ki % 2):
                continue
            c = _closure_case(B, S, spg, 3 + ki, kind, once, hmax=8 if short else 254)
            budgets = [b for b in BUDGETS if not (short and b > 5)]
            for form in QC.FORMS:
                for budget in budgets if S <= 260 else budgets[(ki + once) % 2::2]:
                    n += 1
                    greedy = _check_closure(c, form, budget, seen)
                    if (n + ki) % 5 == 0:                                  # the sampled operator: identity (c), and a real draw
                        g = np.random.default_rng([n, S, spg])
                        u = g.random(B).astype(np.float32)
                        for params in DRAWS:
                            drawn = _check_closure(c, form, budget, seen, (u, params))
                            if params[0] == 0:
                                assert all(torch.equal(drawn[k], greedy[k]) for k in greedy), (kind, form, budget)
            # identity (a): zero tables are the plain operators, bit for bit; identity (b): exact contains lookahead, per row
            zero = (np.zeros_like(c["close_dist"]), np.zeros_like(c["cycle_len"]))
            u = np.random.default_rng([S, spg, ki]).random(B).astype(np.float32)
            for draw in (None, (u, DRAWS[1])):
                lg0, a0 = _run_closure(c, "lookahead", 2, draw, tables=zero)
                lg1, a1 = _run_closure(c, None, None, draw, plain=True)
                assert all(torch.equal(a0[k], a1[k]) for k in a1) and torch.equal(lg0, lg1), (kind, once, draw is not None)
            for budget in (1, 5):
                la = _run_closure(c, "lookahead", budget)[1]
                ex = _run_closure(c, "exact", budget)[1]
                for b in range(B):
                    if not c["fin"][b] and not (la["dead_end"][b] or ex["dead_end"][b]):
                        assert not bool((la["mask_rows"][b, NTOK:] & ~ex["mask_rows"][b, NTOK:] & 1).any()), (kind, once, budget, b)
            if kind == "trap_a" and not once:                              # the trap: the plain operator takes edge 3, the forms edge 2
                assert int(_run_closure(c, None, None, plain=True)[1]["next"][0]) == NTOK + 3
                assert int(_run_closure(c, "lookahead", 2)[1]["next"][0]) == NTOK + 2 and int(_run_closure(c, "lookahead", 5)[1]["next"][0]) == NTOK + 3
                assert int(_run_closure(c, "exact", 5)[1]["next"][0]) == NTOK + 2
            if kind == "trap_b":                                           # ONCE keeps edge 4 out of the search: edge 3 cannot close
                assert int(_run_closure(c, "exact", 5)[1]["next"][0]) == (NTOK + 2 if once else NTOK + 3)
                assert int(_run_closure(c, "lookahead", 5)[1]["next"][0]) == NTOK + 3
    print("S=%d spg=%d: %d launches checked," % (S, spg, n), seen)
    assert seen["stricter"] and seen["dead"], seen
    if S >= 65:      # (with the one edge of S = 5 a closure needs that edge to follow itself, be unpadded and win the row)
        assert seen["closing"], seen


@pytest.mark.gpu
def test_exact_operator_at_2048_keys_with_a_live_key_beyond_chunk_16(hip_lib):
    """32 chunks of 64 keys: the search's reach words use every bit.  A ring of all 2044 edges; row 0 is open at edge 1100 with
    first = 1105: the one follower, key 4 + 1101 in chunk 17, closes within budget 5 and not within 3."""
    S, B = 2048, 2
    c = _closure_case(B, S, 1, 5, "ring", False)
    c["fin"][:] = 0
    c["mask"][:] = False
    c["kv"][:] = S
    c["pad"][:] = False
    c["first"][0], c["prev"][0], c["visited"][0] = 1105, 1100, {1100}
    c["first"][1], c["prev"][1], c["visited"][1] = -1, -1, set()
    seen = dict(stricter=0, dead=0, closing=0)
    res = _check_closure(c, "exact", 5, seen)
    assert int(res["next"][0]) == NTOK + 1101 and (NTOK + 1101) // 64 == 17 and not int(res["dead_end"][0])
    res = _check_closure(c, "exact", 3, seen)
    assert int(res["next"][0]) == SEP and int(res["dead_end"][0]) == 1
    assert seen["dead"] == 1 and seen["stricter"]


def _raw_closure_call(lib, c, over=None, form=1, budget=2, sample=False):
    """ff_pointer_sequence_constrained_ahead / _sample_ahead through ctypes with `over` replacing named arguments; every output holds
    a sentinel."""
    B, S, L = c["B"], c["S"], c["L"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lg = dev(c["logits"])
    keep = dict(fin=dev(c["fin"]), first=dev(c["first"]), prev=dev(c["prev"]), visited=dev(_words(c["visited"], L)),
                follows=dev(faces.pack_follow_bits(c["table"])), mask=dev(c["mask"].astype(np.uint8)), kv=dev(c["kv"]), memory=dev(c["memory"]),
                cd=dev(c["close_dist"]), cl=dev(c["cycle_len"]), u=torch.full((B,), 0.5).cuda())
    i32 = lambda: torch.full((B,), -7, dtype=torch.int32).cuda()
    outs = dict(mask_rows=torch.full((B, S), 77, dtype=torch.uint8).cuda(), next_tok=i32(), logprob=torch.full((B,), 7.5).cuda(), fin_out=i32(),
                dead_end=i32(), first_out=i32(), prev_out=i32(), next_rows=torch.full((B, E_OP), 7.5).cuda(),
                count=torch.full((1,), 5, dtype=torch.int32).cuda())
    a = dict(logits=lg.data_ptr(), ldlogits=S, S=S, mask=keep["mask"].data_ptr(), kv_len=keep["kv"].data_ptr(), B=B, spg=c["spg"],
             follows=keep["follows"].data_ptr(), L=L, flags=c["flags"], ntok=NTOK, tok_sep=SEP, tok_eos=EOS, fin_in=keep["fin"].data_ptr(),
             first_in=keep["first"].data_ptr(), prev_in=keep["prev"].data_ptr(), visited=keep["visited"].data_ptr(),
             mask_rows=outs["mask_rows"].data_ptr(), next_tok=outs["next_tok"].data_ptr(), logprob=outs["logprob"].data_ptr(),
             fin_out=outs["fin_out"].data_ptr(), dead_end=outs["dead_end"].data_ptr(), first_out=outs["first_out"].data_ptr(),
             prev_out=outs["prev_out"].data_ptr(), memory=keep["memory"].data_ptr(), E=E_OP, next_rows=outs["next_rows"].data_ptr(),
             ldnext=E_OP, next_stats=None, count=outs["count"].data_ptr())
    if sample:
        a.update(uniforms=keep["u"].data_ptr(), num_uniforms=B, row_id=None, temperature=1.0, top_k=0, top_p=1.0)
    a.update(form=form, close_dist=keep["cd"].data_ptr(), cycle_len=keep["cl"].data_ptr(), budget=budget,
             stream=torch.cuda.current_stream().cuda_stream)
    a.update(over or {})
    rc = getattr(lib, "ff_pointer_sequence_constrained_sample_ahead" if sample else "ff_pointer_sequence_constrained_ahead")(*a.values())
    torch.cuda.synchronize()
    return rc, lg, keep, outs


@pytest.mark.gpu
def test_operators_err_arg_leaves_the_outputs_untouched(hip_lib):
    lib = hip_lib
    c = _closure_case(5, 65, 4, 3, "random", False)
    wide = _closure_case(1, 2052, 1, 3, "chain", False)                            # 2052 keys: above the exact search's limit
    for sample in (False, True):
        for form in (1, 2):
            rc, lg, keep, outs = _raw_closure_call(lib, c, None, form, 2, sample)
            assert rc == 0 and int(outs["next_tok"].min()) >= 0, (sample, form)       # the arguments are good ones
        cases = [(c, dict(form=0)), (c, dict(form=3)), (c, dict(form=-1)), (c, dict(flags=1)), (c, dict(flags=5)), (c, dict(flags=0)),
                 (c, dict(form=2, flags=2)), (c, dict(close_dist=None)), (c, dict(cycle_len=None)), (c, dict(form=2, cycle_len=None)),
                 (c, dict(budget=-1)), (c, dict(budget=255)), (c, dict(form=2, budget=255)), (wide, dict(form=2)),
                 (c, dict(flags=8 | 3)), (c, dict(flags=6)), (c, dict(follows=None)), (c, dict(tok_sep=EOS)), (c, dict(tok_eos=NTOK)),
                 (c, dict(L=c["L"] - 1)), (c, dict(spg=0)), (c, dict(S=0)), (c, dict(mask_rows=None)), (c, dict(next_tok=None)),
                 (c, dict(dead_end=None)), (c, dict(visited=None)), (c, dict(logits=None)), (c, dict(ldnext=E_OP - 4))]
        if sample:
            cases += [(c, dict(temperature=-1.0)), (c, dict(top_p=0.0)), (c, dict(uniforms=None)), (c, dict(num_uniforms=2))]
        for case, over in cases:
            rc, lg, keep, outs = _raw_closure_call(lib, case, over, over.get("form", 1), over.get("budget", 2), sample)
            assert rc == -1, (sample, over, rc)                                       # FF_ERR_ARG
            assert torch.equal(lg.cpu(), torch.from_numpy(case["logits"])), over
            assert torch.equal(keep["visited"].cpu(), torch.from_numpy(_words(case["visited"], case["L"]))), over
            assert bool((outs["mask_rows"] == 77).all()) and bool((outs["next_rows"] == 7.5).all()) and bool((outs["logprob"] == 7.5).all()), over
            assert all(bool((outs[k] == -7).all()) for k in ("next_tok", "fin_out", "dead_end", "first_out", "prev_out")), over
            assert int(outs["count"].item()) == 5, over
    rc, *_ = _raw_closure_call(lib, wide, None, 1, 2)                                 # the static form has no key limit
    assert rc == 0
    from faceformer_amd.hip import ops
    with pytest.raises(ValueError, match="closure='ahead': must be 'lookahead' or 'exact'"):
        _run_closure(c, "ahead", 2)
    with pytest.raises(ValueError, match="budget=255: must be in 0..254"):
        _run_closure(c, "exact", 255)
    with pytest.raises(ValueError, match="takes at most 2048 keys"):
        _run_closure(wide, "exact", 2)


@pytest.mark.gpu
def test_operator_inside_poisoned_surroundings(hip_lib):
    """One launch of each form with every operand and output inside guarded, poisoned surroundings (tests/redzone.py)."""
    import redzone as RZ
    c = _closure_case(5, 65, 4, 9, "random", True)
    B, S, L = c["B"], c["S"], c["L"]
    for form in (1, 2):
        got = {}
        for fill in (RZ.ZERO, RZ.POISON):
            g = RZ.Guard(fill)
            t = lambda a: g.embed(torch.from_numpy(np.ascontiguousarray(a)))
            lg = t(c["logits"])
            ins = [t(c["fin"]), t(c["first"]), t(c["prev"])]
            vis, fol = t(_words(c["visited"], L)), t(faces.pack_follow_bits(c["table"]))
            mask, kv, mem, cd, cl = t(c["mask"].astype(np.uint8)), t(c["kv"]), t(c["memory"]), t(c["close_dist"]), t(c["cycle_len"])
            i32 = lambda: g.embed(torch.zeros(B, dtype=torch.int32))
            rows, nxt, lp = g.embed(torch.zeros(B, S, dtype=torch.uint8)), i32(), g.embed(torch.zeros(B))
            fin, dead, first, prev = i32(), i32(), i32(), i32()
            out_rows, cnt = g.embed(torch.zeros(B, E_OP)), g.embed(torch.zeros(1, dtype=torch.int32))
            rc = hip_lib.ff_pointer_sequence_constrained_ahead(
                lg.data_ptr(), S, S, mask.data_ptr(), kv.data_ptr(), B, c["spg"], fol.data_ptr(), L, c["flags"], NTOK, SEP, EOS,
                ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), vis.data_ptr(), rows.data_ptr(), nxt.data_ptr(), lp.data_ptr(),
                fin.data_ptr(), dead.data_ptr(), first.data_ptr(), prev.data_ptr(), mem.data_ptr(), E_OP, out_rows.data_ptr(), E_OP, None,
                cnt.data_ptr(), form, cd.data_ptr(), cl.data_ptr(), 2, torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            g.check()                                                      # nothing written outside the views
            got[fill] = [x.clone() for x in (nxt, rows, lp, fin, dead, first, prev, out_rows, cnt, vis, lg)]
        for a, b in zip(got[RZ.ZERO], got[RZ.POISON]):                     # nothing read outside them
            RZ.assert_same_bits(a, b, "sequence closure form %d" % form)
        want = _run_closure(c, QC.FORMS[form - 1], 2)[1]
        nxt, rows, lp = got[RZ.POISON][:3]
        assert torch.equal(nxt, want["next"]) and torch.equal(rows, want["mask_rows"]) and torch.equal(lp, want["logprob"])
        assert int(got[RZ.POISON][4].sum()) > 0 or form == 1               # (a dead end among the rows)


# ---- GPU: the engine ----------------------------------------------------------------------------------------------------------------
_TABLES = {}
R_DRAWS, DRAW_SEED = 3, 5


def _tables(fix):
    """(close_dist, cycle_len) of a fixture as the model builds them: numpy, and on the device."""
    if fix not in _TABLES:
        case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
        cd, cl = QC.tables(follows, case["model"]["seq_len"], batch["num_input"])
        _TABLES[fix] = (cd, cl, torch.from_numpy(cd).cuda(), torch.from_numpy(cl).cuda())
    return _TABLES[fix]


def _closure(fix, flags, form, tables=None, R=0, params=None, u=None, **kw):
    """The engine's decode of a fixture under `form` (None: the plain decode), greedy or with R draws."""
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    if form is not None:
        cd, cl = tables if tables is not None else _tables(fix)[2:]
        kw.update(sequence_constrain_closure=form, cycle_len=cl, **({} if form == "exact" else dict(close_dist=cd)))
    if R:
        kw.update(sequence_constrain_samples=R, temperature=params[0], top_k=params[1], top_p=params[2], uniforms=u)
    return _constrained(model, case, b, flags, table, **kw)


def _replay_closure(out, fix, flags, form, R=1, u=None, params=None):
    """The numpy rule under `form`, with the decode's own tables and the clamped budget, on the decode's own traced logits, pair by
    pair: the FILL pattern, the dead flag, the finish and the log-probability everywhere; the token where the pair is decisive
    (greedy: margin above 2 tol(step); a draw: sample_ref.sample_row's).  Returns (left-out pairs, pairs, tokens, dead, open_end)."""
    import sample_ref as SR
    import test_sequence_constrain as TS
    import test_sequence_constrain_sample as TSS
    from test_parity_golden import _tol
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    cd, cl = _tables(fix)[:2]
    ni = batch["num_input"]
    T, S = case["model"]["seq_len"], case["model"]["L"] + NTOK
    if u is None:
        tok, lp, dead, fin, steps, states = TS._check_layout(out, T, flags, follows)
        oe = out["open_end"].cpu().numpy()
    else:
        tok, lp, dead, fin, steps, states = TSS._check_layout(out, T, R, flags, follows)
        oe, un = out["sample_open_end"].cpu().numpy(), u.cpu().numpy()
    logits = out["logits"].cpu().numpy()
    pairs = left = 0
    for j in range(steps):
        rows = np.flatnonzero(fin > j)
        tol = _tol(logits[j][rows])
        for r in rows:
            w = r // R
            row = logits[j, r].astype(np.float64)
            pad = np.arange(S) >= NTOK + ni[w]
            masked, is_dead = faces.sequence_rule_mask(states[r][j], flags, S, NTOK, SEP, EOS, follows[w], pad,
                                                       **QC.closure_kw(form, cd, cl, w, QC.budget_of(T, j + 1)))
            assert np.array_equal(row <= FILL, masked | pad), (fix, flags, form, j, int(r))      # the constrained masked row, exact
            assert bool(dead[r, j + 1]) == is_dead, (fix, flags, form, j, int(r))
            pairs += 1
            t = int(tok[r, j + 1])
            if u is None:
                want, decisive = int(np.argmax(row)), SC.margin(row) > 2 * tol
            else:
                res = SR.sample_row(row, un[j, r], *params)
                want, decisive = res["tok"], res["decisive"]
            if decisive:
                assert t == want, (fix, flags, form, j, int(r), t, want)
            else:
                left += 1
                assert row[t] > FILL, (fix, flags, form, j, int(r))
            if is_dead:
                assert t == SEP
            own = SR.logprob_of(row, t)
            assert abs(lp[r, j + 1] - own) <= SC.LP_BAR + SC.EPS * abs(own), (fix, flags, form, j, int(r))
    return left, pairs, tok, dead, oe


def _guarantees(fix, flags, form, tok, dead, oe, R=1):
    """(g1), (g2), (g3) on every row; returns (enclosed, parsed)."""
    import test_sequence_constrain as TS
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    ni = batch["num_input"]
    assert not oe.any(), (fix, flags, form, oe.tolist())                                              # (g1)
    late = QC.late_dead_ends(tok, dead, flags, NTOK, SEP, follows, R)
    if form == "exact":
        assert late == [], (fix, flags, late)                                                         # (g2)
    enc = par = 0
    for r in range(tok.shape[0]):
        w = r // R
        row_edges = []
        for idx, at_dead_end, unterminated in SC.face_pieces(tok[r], dead[r], NTOK, SEP, EOS, ni[w]):
            assert len(set(idx)) == len(idx)
            closed = TS._walk_closed(idx, follows[w]) if edges is None else bool(faces.is_face_enclosed(edges[w], idx, SC.TOL))
            par += 1
            enc += closed
            row_edges += list(idx)
            if not at_dead_end and not unterminated:
                assert closed, (fix, flags, form, r, idx)                                             # (g3)
        if flags & SC.ONCE:
            assert len(set(row_edges)) == len(row_edges), (fix, flags, form, r)
    return enc, par, len(late)


@pytest.mark.gpu
@pytest.mark.parametrize("form", QC.FORMS)
@pytest.mark.parametrize("flags", QC.FLAGS)
@pytest.mark.parametrize("fix", QC.FIXTURES, ids=lambda f: "%s-%s%d" % f)
def test_engine_replays_under_the_numpy_rule_and_keeps_the_guarantees(hip_lib, fix, flags, form):
    """The (golden, kind, seed, flags, form) tuples are the helper's: kept on the CPU by tools/sequence_closure_left_out.py."""
    import test_sequence_constrain as TS
    from test_parity_golden import _tol
    key = fix + (flags, form)
    assert key in QC.KEPT, "not a kept tuple"
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    out = _closure(fix, flags, form, trace=True)
    left, pairs, tok, dead, oe = _replay_closure(out, fix, flags, form)
    enc, par, late = _guarantees(fix, flags, form, tok, dead, oe)
    print(key, "steps=%d left-out pairs: %d of %d; enclosed %d of %d; dead ends %d (late %d); open_end %s"
          % (out["steps"], left, pairs, enc, par, int(dead.sum()), late, oe.tolist()))
    assert left <= QC.CAP * pairs, (key, left, pairs)
    kept = QC.KEPT[key]
    if left == 0 and kept[0] == 0:
        assert (enc, par, int(dead.sum()), late, int(oe.sum())) == kept[2:], (key, (enc, par, int(dead.sum()), late), kept)      # the oracle's counts
    plain = _closure(fix, flags, None)
    if flags == LOOPS and fix in QC.OPEN_AT_T:
        assert int(plain["open_end"].sum()) > 0 and not oe.any(), key                                  # the defect the issue names, gone
    # identity (a): zero tables are the plain decode, bit for bit
    if form == "lookahead":
        cd, cl = _tables(fix)[2:]
        zero = _closure(fix, flags, form, tables=(torch.zeros_like(cd), torch.zeros_like(cl)))
        assert zero["steps"] == plain["steps"] and zero["step_counts"] == plain["step_counts"]
        for k in ("predict", "dead_end", "open_end"):
            assert torch.equal(zero[k], plain[k]), (key, k)
        assert torch.equal(zero["logprob"].view(torch.int32), plain["logprob"].view(torch.int32)), key
    # traced logits against the fp64 oracle forced along the decode's tokens
    steps = out["steps"]
    truth = TS._oracle_logits(case, sd, batch, tok, steps)
    got = out["logits"].cpu().numpy()
    fin, _ = SC.stop_and_finish(tok, EOS)
    for j in range(steps):
        rows = np.flatnonzero(fin > j)
        tol = _tol(truth[j][rows])
        for r in rows:
            live = got[j, r] > FILL
            assert np.abs(got[j, r][live] - truth[j, r][live]).max() <= tol, (key, j, int(r))


@pytest.mark.gpu
@pytest.mark.parametrize("form", QC.FORMS)
@pytest.mark.parametrize("flags", QC.FLAGS)
@pytest.mark.parametrize("fix", QC.FIXTURES, ids=lambda f: "%s-%s%d" % f)
def test_engine_draws_under_a_closure_form(hip_lib, fix, flags, form):
    """R = 3 draws, seed 5, both replay parameter sets: the replay, the guarantees on every draw, identity (a) with zero tables
    and identity (c) at R in {1, 3}."""
    import test_sequence_constrain_sample as TSS
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N = case["model"]["seq_len"], b["input"].size(0)
    u = TSS._uniforms(case, b, R_DRAWS, DRAW_SEED)
    for params in QC.REPLAY_PARAMS:
        out = _closure(fix, flags, form, R=R_DRAWS, params=params, u=u, trace=True)
        left, pairs, smp, dead, oe = _replay_closure(out, fix, flags, form, R_DRAWS, u, params)
        enc, par, late = _guarantees(fix, flags, form, smp, dead, oe, R_DRAWS)
        print(fix, flags, form, params, "steps=%d left-out pairs: %d of %d; enclosed %d of %d; dead ends %d (late %d)"
              % (out["steps"], left, pairs, enc, par, int(dead.sum()), late))
        assert left <= QC.CAP * pairs, (fix, flags, form, params, left, pairs)
    if form == "lookahead":                                                    # (a): zero tables, the plain sampled decode
        cd, cl = _tables(fix)[2:]
        params = QC.REPLAY_PARAMS[1]
        zero = _closure(fix, flags, form, tables=(torch.zeros_like(cd), torch.zeros_like(cl)), R=R_DRAWS, params=params, u=u)
        plain = _closure(fix, flags, None, R=R_DRAWS, params=params, u=u)
        assert zero["steps"] == plain["steps"] and zero["step_counts"] == plain["step_counts"]
        for k in ("samples", "sample_dead_end", "sample_open_end", "predict", "dead_end", "open_end"):
            assert torch.equal(zero[k], plain[k]), (fix, flags, k)
        for k in ("sample_logprob", "sample_scores", "logprob"):
            assert torch.equal(zero[k].view(torch.int32), plain[k].view(torch.int32)), (fix, flags, k)
    greedy = _closure(fix, flags, form)                                        # (c): temperature 0 at any R
    for R in (1, 3):
        out = _closure(fix, flags, form, R=R, params=(0.0, 4, 0.5), u=TSS._uniforms(case, b, R, 3))
        assert out["steps"] == greedy["steps"] and out["step_counts"] == [R * v for v in greedy["step_counts"]], (fix, flags, form, R)
        for k in range(R):
            assert torch.equal(out["samples"].view(N, R, T)[:, k], greedy["predict"]), (fix, flags, form, R, k)
            assert torch.equal(out["sample_logprob"].view(N, R, T)[:, k].view(torch.int32), greedy["logprob"].view(torch.int32))
            assert torch.equal(out["sample_dead_end"].view(N, R, T)[:, k], greedy["dead_end"])
            assert torch.equal(out["sample_open_end"].view(N, R)[:, k], greedy["open_end"])


@pytest.mark.gpu
def test_engine_late_dead_ends_of_the_plain_decode_are_gone_under_exact(hip_lib):
    """On the random fixtures the CPU tool lists (LATE_PLAIN) the plain decode meets a dead end that is not right after the position
    that opened the loop; under "exact" there is none."""
    assert QC.LATE_PLAIN
    some = 0
    for name, kind, seed, flags in QC.LATE_PLAIN[:4]:
        fix = (name, kind, seed)
        case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
        plain = _closure(fix, flags, None)
        late = QC.late_dead_ends(plain["predict"].cpu().numpy(), plain["dead_end"].cpu().numpy(), flags, NTOK, SEP, follows)
        exact = _closure(fix, flags, "exact")
        assert QC.late_dead_ends(exact["predict"].cpu().numpy(), exact["dead_end"].cpu().numpy(), flags, NTOK, SEP, follows) == []
        some += len(late)
    assert some > 0


@pytest.mark.gpu
def test_engine_micro_batch_cut_repeatability_and_given_tables(hip_lib):
    fix = ("seq_small_gain4", "random", 2)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    import test_sequence_constrain_sample as TSS
    for form in QC.FORMS:
        whole = _closure(fix, COEDGE, form, trace=True)
        again = _closure(fix, COEDGE, form, trace=True)
        assert whole["steps"] == again["steps"] and whole["step_counts"] == again["step_counts"]
        for k in ("predict", "logprob", "dead_end", "open_end", "logits"):                      # one plan, two runs: bit-equal
            n = whole["steps"] if k == "logits" else None
            assert torch.equal(whole[k][:n], again[k][:n]), (form, k)
        one = _closure(fix, COEDGE, form, trace=True, chunk_max_seqs=1)                           # one wireframe per micro-batch: its own table rows
        lw, pw, *_ = _replay_closure(whole, fix, COEDGE, form)
        lo, po, *_ = _replay_closure(one, fix, COEDGE, form)
        assert lw <= QC.CAP * pw and lo <= QC.CAP * po
        if lw == 0 and lo == 0:
            for k in ("predict", "dead_end", "open_end"):
                assert torch.equal(whole[k], one[k]), (form, k)
        R = R_DRAWS
        u = TSS._uniforms(case, b, R, DRAW_SEED)
        params = QC.REPLAY_PARAMS[1]
        dw = _closure(fix, COEDGE, form, R=R, params=params, u=u, trace=True)
        dr = _closure(fix, COEDGE, form, R=R, params=params, u=u, trace=True, chunk_max_seqs=R)   # one wireframe's draws per micro-batch
        lw, pw, *_ = _replay_closure(dw, fix, COEDGE, form, R, u, params)
        lo, po, *_ = _replay_closure(dr, fix, COEDGE, form, R, u, params)
        if lw == 0 and lo == 0:
            for k in ("samples", "sample_dead_end", "sample_open_end"):
                assert torch.equal(dw[k], dr[k]), (form, k)


@pytest.mark.gpu
def test_engine_on_a_poisoned_exact_size_workspace(hip_lib):
    import redzone as RZ
    import test_workspace_poison as WP
    name = "seq_small_gain4"
    m = WP._bound(name, "default")
    batch, follows, _ = SC.fixture(m.case, m.batch, "random", 2)      # (KEPT: dead ends under either form)
    b = batch_to(batch, "cuda")
    table = torch.from_numpy(faces.pack_follow_bits(follows)).cuda()
    cd, cl = (torch.from_numpy(t).cuda() for t in QC.tables(follows, m.case["model"]["seq_len"], batch["num_input"]))
    for form in QC.FORMS:
        call = lambda: _constrained(m.model, m.case, b, LOOPS, table, trace=True, sequence_constrain_closure=form, cycle_len=cl,
                                    **({} if form == "exact" else dict(close_dist=cd)))
        clean = call()
        zero, d = WP._run([m], call, fill=RZ.ZERO, what="sequence closure after ZERO")
        poison, _ = WP._run([m], call, fill=RZ.POISON, what="sequence closure after POISON")
        WP._assert_equal(poison, zero, "sequence closure")
        WP._assert_equal(poison, clean, "sequence closure against the clean run")
        WP._assert_no_nan(poison, "sequence closure")
        assert zero["steps"] > 0 and len(d.taken) == 2                    # the encoder's and the decode's, each of its own query's size
        assert int(zero["dead_end"].sum()) > 0 and not bool(zero["open_end"].any())


@pytest.mark.gpu
def test_engine_takes_a_row_longer_than_256_with_the_clamped_budget(hip_lib):
    """T = 259 (config A's) on a narrow synthetic model and a lattice wireframe: the entry accepts it, the replay holds with
    budget = min(T - 1 - p, 254), and no row ends with a loop open."""
    import constrain_ref as CR
    from conftest import build_model
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    L, T, E = 24, 259, 64
    case = dict(kind="seq2seq", model=dict(L=L, seq_len=T, E=E, FF=128, H=1, enc=1, dec=1), recipe="gain4", wseed=7)
    sd = make_state_dict(state_dict_spec("seq2seq", L, T, E, 128, 1, 1), "gain4", 7)
    model = build_model(case, sd, "cuda")
    ni = [22, 17]
    batch, edges, _ = CR.lattice_batch(ni, L, T, 3)
    batch["label"] = torch.zeros((len(ni), T), dtype=torch.int64)
    follows = faces.follow_table(batch["input"].numpy(), SC.TOL, ni)
    fix = ("t259", "lattice", 3)
    import test_sequence_constrain as TS
    TS._FIX[fix] = (case, model, batch_to(batch, "cuda"), batch, follows, torch.from_numpy(faces.pack_follow_bits(follows)).cuda(), edges, sd)
    assert QC.hmax_of(T) == 254 and QC.budget_of(T, 1) == 254 and QC.budget_of(T, 4) == 254 and QC.budget_of(T, 5) == 253
    try:
        for form in QC.FORMS:
            for flags in QC.FLAGS:
                out = _closure(fix, flags, form, trace=True)
                left, pairs, tok, dead, oe = _replay_closure(out, fix, flags, form)
                _guarantees(fix, flags, form, tok, dead, oe)
                assert pairs > 0 and not oe.any(), (form, flags)
    finally:
        TS._FIX.pop(fix, None)
        _TABLES.pop(fix, None)


# ---- GPU: the model and the CLI -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_model_publishes_the_keys_builds_or_takes_the_tables_and_sequence_faces_works_behind_it(hip_lib):
    fix = ("seq_small_gain4", "lattice", 2)
    case, model, b, batch, follows, table, edges, sd = _fixture(*fix)
    T, N = case["model"]["seq_len"], b["input"].size(0)
    cd, cl, cd_dev, cl_dev = _tables(fix)
    ni = np.asarray(batch["num_input"], dtype=np.int32)
    try:
        with torch.no_grad():
            model.sequence_constrain = "coedge_loops"
            plain = model(dict(b))
            for form in QC.FORMS:
                model.sequence_constrain_closure = form
                on = model(dict(b))                                       # the tables are built on the device from the follow table
                given = model(dict(b, follow_table=table, close_dist=torch.from_numpy(cd), cycle_len=cl_dev))
                assert set(on) == set(plain)                              # the published keys are the plain decode's
                direct = _closure(fix, COEDGE, form)
                for k, d in (("predict", "predict"), ("predict_logprob", "logprob"), ("predict_dead_end", "dead_end"),
                             ("predict_open_end", "open_end")):
                    assert torch.equal(on[k], given[k]) and torch.equal(on[k], direct[d]), (form, k)
                    assert on[k].dtype == plain[k].dtype and on[k].shape == plain[k].shape
                assert not bool(on["predict_open_end"].any())
                model.sequence_constrain_samples = 3
                drawn = model(dict(b))
                model.sequence_constrain_samples = 0
                assert tuple(drawn["predict_samples"].shape) == (N, 3, T) and not bool(drawn["predict_sample_open_end"].any())
                model.sequence_faces = "enclosed"
                both = model(dict(b))
                model.sequence_faces = False
                want = faces.face_seq_rows(both["predict"].cpu().numpy(), ni, TOK, logprob=both["predict_logprob"].cpu().numpy(),
                                           follows=faces.pack_follow_bits(follows), closed_only=True)
                want.update(faces.face_seq_votes(want, require_closed=True))
                for k in want:
                    a, w = both["sequence_faces"][k].cpu().numpy(), np.asarray(want[k])
                    assert np.array_equal(a.reshape(w.shape).view(w.dtype) if a.dtype.itemsize == w.dtype.itemsize else a.reshape(w.shape), w), k
                assert int(both["sequence_faces"]["num_faces"].sum()) > 0 and torch.equal(both["predict"], on["predict"])
            # the built tables are faces.follow_distance's
            from faceformer_amd.hip import ops
            got_cd, got_cl = ops.follow_distance(table, torch.from_numpy(ni).cuda(), QC.hmax_of(T))
            assert np.array_equal(got_cd.cpu().numpy(), cd) and np.array_equal(got_cl.cpu().numpy(), cl)
    finally:
        model.sequence_constrain = model.sequence_constrain_closure = None
        model.sequence_constrain_samples, model.sequence_faces = 0, False


@pytest.mark.gpu
def test_cli_records_with_and_without_the_flag(hip_lib, tmp_path):
    import json
    import constrain_ref as CR
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.config import load_cfg
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    root = tmp_path / "data"
    (root / "json").mkdir(parents=True)
    names = []
    for i in range(2):
        polys, _ = CR.lattice_edges(8 + 4 * i, 40 + i)
        raw = {"edges": [[[float(p[0][0]), float(p[0][1])], [float(p[-1][0]), float(p[-1][1])]] for p in polys],
               "faces_indices": [[[0, 1, 2]], [[3, 4, 5]]], "pairings": {}, "dominant_directions": [[1, 0, 0]]}
        json.dump(raw, open(root / "json" / ("%08d.json" % i), "w"))
        names.append("json/%08d.json" % i)
    open(root / "test.txt", "w").write("\n".join(names) + "\n")
    cfg = load_cfg("configs/seq2seq.yml", ["model.num_lines", "16", "model.label_seq_length", "24", "model.num_model", "128",
                                            "model.num_head", "2", "model.num_feedforward", "256", "model.num_encoder_layers", "2",
                                            "model.num_decoder_layers", "2", "root_dir", str(root), "post_process.is_coedge", "False"])
    sd = make_state_dict(state_dict_spec("seq2seq", 16, 24, 128, 256, 2, 2), "gain4", 51)
    ckpt = tmp_path / "last.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(cfg)}, ckpt)
    run = lambda d, **kw: cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / d), **kw)
    loops = run("loops", sequence_constrain="loops")
    loops2 = run("loops2", sequence_constrain="loops", sequence_constrain_closure=None)
    drawn = run("drawn", sequence_constrain="loops", sequence_constrain_samples=2, seed=3)
    for form in QC.FORMS:
        ahead = run("ahead_" + form, sequence_constrain="loops", sequence_constrain_closure=form)
        both = run("both_" + form, sequence_constrain="loops", sequence_constrain_closure=form, sequence_constrain_samples=2, seed=3)
        for fn in sorted(os.listdir(loops)):
            text = open(os.path.join(loops, fn)).read()
            assert text == open(os.path.join(loops2, fn)).read()          # byte-identical without the flag
            rl, ra, rd, rb = (json.load(open(os.path.join(d, fn))) for d in (loops, ahead, drawn, both))
            assert list(ra) == list(rl) and list(rb) == list(rd)          # the record keys are the plain decode's
            assert ra["pred_unclosed"] <= ra["pred_dead_ends"]            # no face is left open at the end of the row
