"""What the fourteen opt-in decode entries (ff_decode_beam ... ff_decode_sequence_constrained_beam) refuse, in which order and in
which words, against literals recorded from the library of the commit BEFORE the entries got one check routine (check_entry,
ff_engine.hip): a refactor of the engine must leave every status and every ff_last_error() text alone.

No GPU: an entry rejects bad arguments before any HIP call, so it is driven through ctypes on the hand-filled `lib.Model` of
test_workspace_layout with null or dummy pointers.  Per entry, CHECKS lists its checks in the order it makes them, each as the
change to an otherwise acceptable call that violates exactly that check.  The cases are
  <entry>/<check>           that one violation: its own message;
  <entry>/<check>+<next>    two consecutive ones at once: the EARLIER check's message, which pins the order;
  <entry>/<check>:<operand> the same check violated through another of its operands (ALTERNATIVES: every flag and pointer an
                            exclusion names, F != 1, a null model or decode params, every required output on its own, each
                            refused trace, both ends of every range);
  <entry>/pass              no violation: the entry hands on to the decode, which ends in its own "ff_decode: null pointer"
                            (memory is null) before it touches the device.
ff_decode_constrained_beam_ahead and ff_decode_constrained_sample are listed once per look-ahead form ([ahead], [exact]).

`python tests/test_entry_checks.py` prints EXPECTED for the library it loads (FF_HIP_LIB selects another build); the table below
was printed that way by the parent commit's library and holds no value computed by the code under test.

Left out:
  - pairs whose two changes touch the same field, or where the later change removes the earlier violation (the rule's flag
    checks among themselves and against the look-ahead's flag check; "CONNECT needs the follow table" against any flag change);
  - the rule checks' "L must be S - ntok" (the entries compute S as L + num_token; only a negative num_token reaches it, which also
    breaks the check behind it);
  - in the ruled parallel entries "empty terminator range" (the rule's own range check in front of it refuses the same);
  - ff_sample_draw_check's "null pointer" and "uniforms ... without a row_id" (the required-outputs and the size checks in front
    of it refuse a null `uniforms` and leave num_uniforms = rows);
  - everything behind the checks: it dereferences device pointers or calls HIP."""
import ctypes as C

import pytest

from faceformer_amd.hip import engine, lib as L
from test_workspace_layout import DUMMY, EDGES, F, N, T, model

NO_REPEAT, CONNECT, ONCE = L.FF_CONSTRAIN_NO_REPEAT, L.FF_CONSTRAIN_CONNECT, L.FF_CONSTRAIN_ONCE
SEQ_FLAGS = engine.DEFAULT_FLAGS & ~L.FF_DEDUP_PAD_ANCHORS
PAR_ARGS = ("memory", "mask", "kv_len", "num_input", "num_input_host", "extra_mask", "predict", "steps_done", "step_counts", "pointer_out",
            "trace_logits", "trace_best", "trace_second", "seq_of_row", "workspace", "workspace_bytes", "prm", "stream")
SEQ_ARGS = ("memory", "mask", "kv_len", "predict", "steps_done", "step_counts", "trace_logits", "seq_of_row", "workspace",
            "workspace_bytes", "prm", "stream")
FORCED_ARGS = ("memory", "mask", "kv_len", "prm", "steps_done", "trace_logits", "workspace", "workspace_bytes", "stream")

# A check: (name, {(struct, field): new value or function of the old one}).  struct: "m", "p", "prm" or "arg" (a call argument).
# A field set to its old value marks what the violation depends on, so that a pair with a change of that field is left out.
same = lambda old: old   # noqa: E731
NULL = ("null", {("arg", "prm"): None})
PAR_VARIANT = ("variant", {("p", "variant"): L.FF_SEQ2SEQ})
SEQ_VARIANT = ("variant", {("p", "variant"): L.FF_PARALLEL})
EXCLUDED = ("excluded", {("p", "flags"): lambda old: old | L.FF_NO_STOP})
WIDTH = ("width", {("prm", "width"): 9})
SAMPLES = ("num_samples", {("prm", "num_samples"): 65})
OWN_DRAW = ("temperature", {("prm", "temperature"): -1.0})
STOP_BEST = ("stop_best", {("prm", "stop_best"): 2})
LOOP_RULE = [("rule_flags", {("prm", "flags"): 64}), ("rule_range", {("p", "term_hi"): 9}),
             ("rule_follows", {("prm", "follows"): None, ("prm", "flags"): same})]
SEQ_RULE = [("rule_flags", {("prm", "flags"): 64}), ("rule_once", {("prm", "flags"): ONCE | CONNECT}),
            ("rule_tokens", {("prm", "tok_sep"): 1}), ("rule_follows", {("prm", "follows"): None, ("prm", "flags"): same})]
LOOKAHEAD = ("lookahead", {("prm", "lookahead"): 3})
AHEAD = [("ahead_flags", {("prm", "flags"): NO_REPEAT}), ("ahead_tables", {("prm", "close_dist"): None}), ("ahead_T", {("p", "T"): 257})]
EXACT = [("exact_flags", {("prm", "flags"): CONNECT}), ("exact_table", {("prm", "cycle_len"): None}), ("exact_T", {("p", "T"): 257}),
         ("exact_L", {("p", "L"): 2045})]
TERM_EMPTY = ("term_empty", {("p", "term_hi"): 2})
SIZES = ("sizes", {("p", "N"): 1 << 30})
DRAW = ("draw", {("prm", "temperature"): -1.0})
STAGING = ("staging", {("m", "E"): 8192})


# The other operands of a check, by (kind of entry or None for all, check): [(operand, change)].
ALTERNATIVES = {
    (None, "null"): [("model", {("arg", "m"): None}), ("params", {("arg", "p"): None})],
    ("seq", "variant"): [("F", {("p", "F"): 2})],
    ("par", "excluded"): [("retire", {("p", "flags"): lambda old: old | L.FF_RETIRE_FINISHED}),
                          ("return_pointer", {("p", "flags"): lambda old: old | L.FF_RETURN_POINTER}),
                          ("stop_fn", {("p", "stop_fn"): DUMMY}), ("extra_mask", {("arg", "extra_mask"): DUMMY})],
    ("seq", "excluded"): [("retire", {("p", "flags"): lambda old: old | L.FF_RETIRE_FINISHED}),
                          ("return_pointer", {("p", "flags"): lambda old: old | L.FF_RETURN_POINTER}),
                          ("each_eos", {("p", "flags"): lambda old: old | L.FF_STOP_EACH_EOS}), ("stop_fn", {("p", "stop_fn"): DUMMY})],
    ("forced", "excluded"): [("return_pointer", {("p", "flags"): lambda old: old | L.FF_RETURN_POINTER}),
                             ("each_eos", {("p", "flags"): lambda old: old | L.FF_STOP_EACH_EOS}), ("stop_fn", {("p", "stop_fn"): DUMMY})],
    (None, "width"): [("0", {("prm", "width"): 0}), ("S", {("prm", "width"): 5, ("p", "L"): 0})],
    (None, "num_samples"): [("0", {("prm", "num_samples"): 0})],
    (None, "temperature"): [("top_k", {("prm", "top_k"): -1}), ("top_p_0", {("prm", "top_p"): 0.0}), ("top_p_2", {("prm", "top_p"): 2.0})],
    (None, "draw"): [("top_k", {("prm", "top_k"): -1}), ("top_p_0", {("prm", "top_p"): 0.0}), ("top_p_2", {("prm", "top_p"): 2.0})],
    (None, "stop_best"): [("-1", {("prm", "stop_best"): -1})],
    (None, "rule_range"): [("lo", {("p", "term_lo"): -1}), ("empty", {("p", "term_hi"): 2})],
    (None, "rule_tokens"): [("sep_-1", {("prm", "tok_sep"): -1}), ("sep_4", {("prm", "tok_sep"): 4}), ("eos_-1", {("p", "tok_eos"): -1}),
                            ("eos_4", {("p", "tok_eos"): 4})],
    (None, "lookahead"): [("-1", {("prm", "lookahead"): -1})],
    (None, "ahead_tables"): [("cycle_len", {("prm", "cycle_len"): None})],
    (None, "exact_flags"): [("no_repeat_only", {("prm", "flags"): NO_REPEAT})],
    ("par", "outputs"): [("trace_best", {("arg", "trace_best"): DUMMY}), ("trace_second", {("arg", "trace_second"): DUMMY}),
                         ("pointer_out", {("arg", "pointer_out"): DUMMY})],
    ("seq", "outputs"): [("predict", {("arg", "predict"): None})],
    ("par", "sizes"): [("N_0", {("p", "N"): 0}), ("F_0", {("p", "F"): 0})],
    ("seq", "sizes"): [("N_0", {("p", "N"): 0})],
    ("forced", "sizes"): [("F_0", {("p", "F"): 0}), ("T_0", {("p", "T"): 0}), ("rows", {("p", "N"): 1 << 30}),
                          ("seq2seq_F", {("p", "variant"): L.FF_SEQ2SEQ})],
    ("forced", "lengths"): [("negative", {("arg", "negative_length"): True})],
}
NOT_REQUIRED = ("follows", "close_dist", "cycle_len")   # (operands a rule or look-ahead check asks for, not the required-outputs check)


def alternatives(entry):
    """[(check, operand, change)] of one entry: ALTERNATIVES for the checks it has, and every required pointer of its struct alone."""
    kind, _, fields, checks = CHECKS[entry]
    out = []
    for name, _ in checks:
        for key in ((None, name), (kind, name)):
            out += [(name, operand, change) for operand, change in ALTERNATIVES.get(key, [])]
        if name == "outputs":
            out += [(name, f, {("prm", f): None}) for f, v in fields.items() if v == DUMMY and f not in NOT_REQUIRED]
    return out


def outputs(field):
    return ("outputs", {("prm", field): None})


def rule_fields(**more):
    return dict(flags=NO_REPEAT | CONNECT, follows=DUMMY, **more)


def draw_fields(*outs):
    return dict(num_samples=5, temperature=1.0, top_k=0, top_p=1.0, uniforms=DUMMY, **{k: DUMMY for k in outs})


# entry: (variant, parameter struct, its acceptable fields, the checks in order)
HEAD_PAR, HEAD_SEQ = [NULL, PAR_VARIANT, EXCLUDED], [NULL, SEQ_VARIANT, EXCLUDED]
CON_OUT = dict(logprob=DUMMY, dead_end=DUMMY)
CBEAM = dict(width=3, beams=DUMMY, scores=DUMMY, dead_end=DUMMY)
CSAMPLE = draw_fields("samples", "logprob", "scores", "dead_end")
CHECKS = {
    "ff_decode_beam": ("par", L.BeamParams, dict(width=3, beams=DUMMY, scores=DUMMY),
                       HEAD_PAR + [WIDTH, TERM_EMPTY, outputs("scores"), STAGING]),
    "ff_decode_forced": ("forced", L.ForcedParams, {k: DUMMY for k in ("paths", "lengths", "logprob", "greedy", "rank", "seq_logprob")},
                         [NULL, ("excluded", {("p", "flags"): lambda old: old | L.FF_RETIRE_FINISHED}), outputs("paths"),
                          ("sizes", {("p", "N"): 0}), ("lengths", {("arg", "bad_length"): True})]),
    "ff_decode_sample": ("par", L.SampleParams, draw_fields("samples", "logprob", "scores"),
                         HEAD_PAR + [SAMPLES, OWN_DRAW, TERM_EMPTY, outputs("scores"), SIZES]),
    "ff_decode_sequence_sample": ("seq", L.SampleParams, draw_fields("samples", "logprob", "scores"),
                                  HEAD_SEQ + [SAMPLES, outputs("scores"), SIZES, DRAW]),
    "ff_decode_sequence_beam": ("seq", L.SequenceBeamParams, dict(width=3, stop_best=1, beams=DUMMY, scores=DUMMY, finished=DUMMY),
                                HEAD_SEQ + [WIDTH, STOP_BEST, outputs("finished"), SIZES, STAGING]),
    "ff_decode_sequence_constrained": ("seq", L.SequenceConstrainParams, rule_fields(tok_sep=2, open_end=DUMMY, **CON_OUT),
                                       HEAD_SEQ + SEQ_RULE + [outputs("open_end")]),
    "ff_decode_sequence_constrained_sample": (
        "seq", L.SequenceConstrainSampleParams,
        rule_fields(tok_sep=2, **draw_fields("samples", "logprob", "scores", "dead_end", "open_end", "predict_logprob", "predict_dead_end",
                                             "predict_open_end")),
        HEAD_SEQ + [SAMPLES] + SEQ_RULE + [outputs("predict_open_end"), SIZES, DRAW]),
    "ff_decode_sequence_constrained_beam": (
        "seq", L.SequenceConstrainBeamParams,
        rule_fields(width=3, stop_best=0, tok_sep=2, **{k: DUMMY for k in ("beams", "scores", "finished", "beam_dead_end", "beam_open_end",
                                                                           "dead_end", "open_end")}),
        HEAD_SEQ + [WIDTH, STOP_BEST] + SEQ_RULE + [outputs("beam_open_end"), SIZES, STAGING]),
    "ff_decode_constrained": ("par", L.ConstrainParams, rule_fields(**CON_OUT), HEAD_PAR + LOOP_RULE + [outputs("dead_end")]),
    "ff_decode_constrained_ahead": ("par", L.ConstrainAheadParams, rule_fields(close_dist=DUMMY, cycle_len=DUMMY, **CON_OUT),
                                    HEAD_PAR + LOOP_RULE + AHEAD + [outputs("dead_end")]),
    "ff_decode_constrained_exact": ("par", L.ConstrainExactParams, rule_fields(cycle_len=DUMMY, **CON_OUT),
                                    HEAD_PAR + LOOP_RULE + EXACT + [outputs("dead_end")]),
    "ff_decode_constrained_beam": ("par", L.ConstrainBeamParams, rule_fields(**CBEAM),
                                   HEAD_PAR + [WIDTH] + LOOP_RULE + [outputs("dead_end"), STAGING]),
    "ff_decode_constrained_beam_ahead[ahead]": ("par", L.ConstrainBeamAheadParams,
                                                rule_fields(lookahead=1, close_dist=DUMMY, cycle_len=DUMMY, **CBEAM),
                                                HEAD_PAR + [WIDTH] + LOOP_RULE + [LOOKAHEAD] + AHEAD + [outputs("dead_end"), STAGING]),
    "ff_decode_constrained_beam_ahead[exact]": ("par", L.ConstrainBeamAheadParams, rule_fields(lookahead=2, cycle_len=DUMMY, **CBEAM),
                                                HEAD_PAR + [WIDTH] + LOOP_RULE + [LOOKAHEAD] + EXACT + [outputs("dead_end"), STAGING]),
    "ff_decode_constrained_sample[ahead]": ("par", L.ConstrainSampleParams,
                                            rule_fields(lookahead=1, close_dist=DUMMY, cycle_len=DUMMY, **CSAMPLE),
                                            HEAD_PAR + [SAMPLES] + LOOP_RULE + [LOOKAHEAD] + AHEAD + [outputs("dead_end"), SIZES, DRAW]),
    "ff_decode_constrained_sample[exact]": ("par", L.ConstrainSampleParams, rule_fields(lookahead=2, cycle_len=DUMMY, **CSAMPLE),
                                            HEAD_PAR + [SAMPLES] + LOOP_RULE + [LOOKAHEAD] + EXACT + [outputs("dead_end"), SIZES, DRAW]),
}


def case_ids():
    """Every case, in a fixed order: <entry>/<check>, <entry>/<check>+<next> where the two changes are independent, <entry>/pass."""
    for entry, (_, _, _, checks) in CHECKS.items():
        for i, (name, change) in enumerate(checks):
            yield "%s/%s" % (entry, name)
            if i + 1 < len(checks) and not set(change) & set(checks[i + 1][1]):
                yield "%s/%s+%s" % (entry, name, checks[i + 1][0])
        for name, operand, _ in alternatives(entry):
            yield "%s/%s:%s" % (entry, name, operand)
        yield entry + "/pass"


def call(lib, case):
    """(status, ff_last_error() text) of the case's call."""
    entry, names = case.split("/")
    kind, struct, fields, checks = CHECKS[entry]
    m, p, prm = model(False), L.DecodeParams(), struct()
    p.N, p.L, p.T, p.sync_every, p.tok_sos, p.tok_eos, p.term_lo, p.term_hi = N, EDGES, T, 4, 0, 1, 2, 4
    p.variant, p.F, p.flags = (L.FF_SEQ2SEQ, 1, SEQ_FLAGS) if kind == "seq" else (L.FF_PARALLEL, F, engine.DEFAULT_FLAGS)
    for k, v in fields.items():
        setattr(prm, k, v)
    lengths = (C.c_int * (N * F))(*([1] * (N * F)))   # (forced: the host lengths are read by its last check)
    if kind == "forced":
        prm.lengths_host = lengths
    arg = {"prm": C.byref(prm), "predict": DUMMY}
    structs = {"m": m, "p": p, "prm": prm}
    changes = [dict(checks)[name] for name in names.split("+")] if ":" not in names and names != "pass" else []
    changes += [change for name, operand, change in alternatives(entry) if names == "%s:%s" % (name, operand)]
    for change in changes:
        for (where, field), v in change.items():
            if where == "arg" and field in ("bad_length", "negative_length"):
                lengths[N * F - 1] = T if field == "bad_length" else -1
            elif where == "arg":
                arg[field] = v
            else:
                setattr(structs[where], field, v(getattr(structs[where], field)) if callable(v) else v)
    order = {"par": PAR_ARGS, "seq": SEQ_ARGS, "forced": FORCED_ARGS}[kind]
    mp, pp = (arg.pop(k, C.byref(v)) for k, v in (("m", m), ("p", p)))
    rc = getattr(lib, entry.split("[")[0])(mp, pp, *[arg.get(a, 0 if a == "workspace_bytes" else None) for a in order])
    return rc, lib.ff_last_error().decode()


EXPECTED = {
    'ff_decode_beam/null': (-1, 'ff_decode_beam: null model, params or beam params'),
    'ff_decode_beam/null+variant': (-1, 'ff_decode_beam: null model, params or beam params'),
    'ff_decode_beam/variant': (-1, 'ff_decode_beam: beams are a parallel-variant option'),
    'ff_decode_beam/variant+excluded': (-1, 'ff_decode_beam: beams are a parallel-variant option'),
    'ff_decode_beam/excluded': (-1, 'ff_decode_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_beam/excluded+width': (-1, 'ff_decode_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_beam/width': (-1, 'ff_decode_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_beam/width+term_empty': (-1, 'ff_decode_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_beam/term_empty': (-1, 'ff_decode_beam: empty terminator range [2, 2)'),
    'ff_decode_beam/term_empty+outputs': (-1, 'ff_decode_beam: empty terminator range [2, 2)'),
    'ff_decode_beam/outputs': (-1, 'ff_decode_beam: beams and scores required; no best / second traces, no pointer_out'),
    'ff_decode_beam/outputs+staging': (-1, 'ff_decode_beam: beams and scores required; no best / second traces, no pointer_out'),
    'ff_decode_beam/staging': (-1, "ff_decode_beam: width=3 at E=8192 exceeds the reorder's staging area"),
    'ff_decode_beam/null:model': (-1, 'ff_decode_beam: null model, params or beam params'),
    'ff_decode_beam/null:params': (-1, 'ff_decode_beam: null model, params or beam params'),
    'ff_decode_beam/excluded:retire': (-1, 'ff_decode_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_beam/excluded:return_pointer': (-1, 'ff_decode_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_beam/excluded:stop_fn': (-1, 'ff_decode_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_beam/excluded:extra_mask': (-1, 'ff_decode_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_beam/width:0': (-1, 'ff_decode_beam: width=0 outside 1..8 or above S=16'),
    'ff_decode_beam/width:S': (-1, 'ff_decode_beam: width=5 outside 1..8 or above S=4'),
    'ff_decode_beam/outputs:trace_best': (-1, 'ff_decode_beam: beams and scores required; no best / second traces, no pointer_out'),
    'ff_decode_beam/outputs:trace_second': (-1, 'ff_decode_beam: beams and scores required; no best / second traces, no pointer_out'),
    'ff_decode_beam/outputs:pointer_out': (-1, 'ff_decode_beam: beams and scores required; no best / second traces, no pointer_out'),
    'ff_decode_beam/outputs:beams': (-1, 'ff_decode_beam: beams and scores required; no best / second traces, no pointer_out'),
    'ff_decode_beam/outputs:scores': (-1, 'ff_decode_beam: beams and scores required; no best / second traces, no pointer_out'),
    'ff_decode_beam/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_forced/null': (-1, 'ff_decode_forced: null model, params or forced params'),
    'ff_decode_forced/null+excluded': (-1, 'ff_decode_forced: null model, params or forced params'),
    'ff_decode_forced/excluded': (-1, 'ff_decode_forced: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_forced/excluded+outputs': (-1, 'ff_decode_forced: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_forced/outputs': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/outputs+sizes': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/sizes': (-1, 'ff_decode_forced: bad sizes (seq2seq scores one row per wireframe)'),
    'ff_decode_forced/sizes+lengths': (-1, 'ff_decode_forced: bad sizes (seq2seq scores one row per wireframe)'),
    'ff_decode_forced/lengths': (-1, 'ff_decode_forced: lengths[35]=6 outside 0..5'),
    'ff_decode_forced/null:model': (-1, 'ff_decode_forced: null model, params or forced params'),
    'ff_decode_forced/null:params': (-1, 'ff_decode_forced: null model, params or forced params'),
    'ff_decode_forced/excluded:return_pointer': (-1, 'ff_decode_forced: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_forced/excluded:each_eos': (-1, 'ff_decode_forced: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_forced/excluded:stop_fn': (-1, 'ff_decode_forced: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_forced/outputs:paths': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/outputs:lengths': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/outputs:logprob': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/outputs:greedy': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/outputs:rank': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/outputs:seq_logprob': (-1, 'ff_decode_forced: paths, lengths (device and host) and the four outputs are required'),
    'ff_decode_forced/sizes:F_0': (-1, 'ff_decode_forced: bad sizes (seq2seq scores one row per wireframe)'),
    'ff_decode_forced/sizes:T_0': (-1, 'ff_decode_forced: bad sizes (seq2seq scores one row per wireframe)'),
    'ff_decode_forced/sizes:rows': (-1, 'ff_decode_forced: bad sizes (seq2seq scores one row per wireframe)'),
    'ff_decode_forced/sizes:seq2seq_F': (-1, 'ff_decode_forced: bad sizes (seq2seq scores one row per wireframe)'),
    'ff_decode_forced/lengths:negative': (-1, 'ff_decode_forced: lengths[35]=-1 outside 0..5'),
    'ff_decode_forced/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_sample/null': (-1, 'ff_decode_sample: null model, params or sample params'),
    'ff_decode_sample/null+variant': (-1, 'ff_decode_sample: null model, params or sample params'),
    'ff_decode_sample/variant': (-1, 'ff_decode_sample: sampling is a parallel-variant option'),
    'ff_decode_sample/variant+excluded': (-1, 'ff_decode_sample: sampling is a parallel-variant option'),
    'ff_decode_sample/excluded': (-1, 'ff_decode_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_sample/excluded+num_samples': (-1, 'ff_decode_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_sample/num_samples': (-1, 'ff_decode_sample: num_samples=65 outside 1..64'),
    'ff_decode_sample/num_samples+temperature': (-1, 'ff_decode_sample: num_samples=65 outside 1..64'),
    'ff_decode_sample/temperature': (-1, 'ff_decode_sample: temperature=-1 must be finite and >= 0, top_k=0 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_sample/temperature+term_empty': (-1, 'ff_decode_sample: temperature=-1 must be finite and >= 0, top_k=0 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_sample/term_empty': (-1, 'ff_decode_sample: empty terminator range [2, 2)'),
    'ff_decode_sample/term_empty+outputs': (-1, 'ff_decode_sample: empty terminator range [2, 2)'),
    'ff_decode_sample/outputs': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/outputs+sizes': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/sizes': (-1, 'ff_decode_sample: bad sizes'),
    'ff_decode_sample/null:model': (-1, 'ff_decode_sample: null model, params or sample params'),
    'ff_decode_sample/null:params': (-1, 'ff_decode_sample: null model, params or sample params'),
    'ff_decode_sample/excluded:retire': (-1, 'ff_decode_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_sample/excluded:return_pointer': (-1, 'ff_decode_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_sample/excluded:stop_fn': (-1, 'ff_decode_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_sample/excluded:extra_mask': (-1, 'ff_decode_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_sample/num_samples:0': (-1, 'ff_decode_sample: num_samples=0 outside 1..64'),
    'ff_decode_sample/temperature:top_k': (-1, 'ff_decode_sample: temperature=1 must be finite and >= 0, top_k=-1 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_sample/temperature:top_p_0': (-1, 'ff_decode_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=0 in (0, 1]'),
    'ff_decode_sample/temperature:top_p_2': (-1, 'ff_decode_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=2 in (0, 1]'),
    'ff_decode_sample/outputs:trace_best': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/outputs:trace_second': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/outputs:pointer_out': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/outputs:uniforms': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/outputs:samples': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/outputs:logprob': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/outputs:scores': (-1, 'ff_decode_sample: uniforms, samples, logprob and scores required; no best / second traces, no pointer_out'),
    'ff_decode_sample/sizes:N_0': (-1, 'ff_decode_sample: bad sizes'),
    'ff_decode_sample/sizes:F_0': (-1, 'ff_decode_sample: bad sizes'),
    'ff_decode_sample/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_sequence_sample/null': (-1, 'ff_decode_sequence_sample: null model, params or sample params'),
    'ff_decode_sequence_sample/null+variant': (-1, 'ff_decode_sequence_sample: null model, params or sample params'),
    'ff_decode_sequence_sample/variant': (-1, 'ff_decode_sequence_sample: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_sample'),
    'ff_decode_sequence_sample/variant+excluded': (-1, 'ff_decode_sequence_sample: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_sample'),
    'ff_decode_sequence_sample/excluded': (-1, 'ff_decode_sequence_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_sample/excluded+num_samples': (-1, 'ff_decode_sequence_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_sample/num_samples': (-1, 'ff_decode_sequence_sample: num_samples=65 outside 1..64'),
    'ff_decode_sequence_sample/num_samples+outputs': (-1, 'ff_decode_sequence_sample: num_samples=65 outside 1..64'),
    'ff_decode_sequence_sample/outputs': (-1, 'ff_decode_sequence_sample: uniforms, samples, logprob, scores and predict are required'),
    'ff_decode_sequence_sample/outputs+sizes': (-1, 'ff_decode_sequence_sample: uniforms, samples, logprob, scores and predict are required'),
    'ff_decode_sequence_sample/sizes': (-1, 'ff_decode_sequence_sample: bad sizes'),
    'ff_decode_sequence_sample/sizes+draw': (-1, 'ff_decode_sequence_sample: bad sizes'),
    'ff_decode_sequence_sample/draw': (-1, 'ff_decode_sequence_sample: temperature=-1 must be finite and >= 0, top_k=0 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_sequence_sample/null:model': (-1, 'ff_decode_sequence_sample: null model, params or sample params'),
    'ff_decode_sequence_sample/null:params': (-1, 'ff_decode_sequence_sample: null model, params or sample params'),
    'ff_decode_sequence_sample/variant:F': (-1, 'ff_decode_sequence_sample: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_sample'),
    'ff_decode_sequence_sample/excluded:retire': (-1, 'ff_decode_sequence_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_sample/excluded:return_pointer': (-1, 'ff_decode_sequence_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_sample/excluded:each_eos': (-1, 'ff_decode_sequence_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_sample/excluded:stop_fn': (-1, 'ff_decode_sequence_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_sample/num_samples:0': (-1, 'ff_decode_sequence_sample: num_samples=0 outside 1..64'),
    'ff_decode_sequence_sample/outputs:predict': (-1, 'ff_decode_sequence_sample: uniforms, samples, logprob, scores and predict are required'),
    'ff_decode_sequence_sample/outputs:uniforms': (-1, 'ff_decode_sequence_sample: uniforms, samples, logprob, scores and predict are required'),
    'ff_decode_sequence_sample/outputs:samples': (-1, 'ff_decode_sequence_sample: uniforms, samples, logprob, scores and predict are required'),
    'ff_decode_sequence_sample/outputs:logprob': (-1, 'ff_decode_sequence_sample: uniforms, samples, logprob, scores and predict are required'),
    'ff_decode_sequence_sample/outputs:scores': (-1, 'ff_decode_sequence_sample: uniforms, samples, logprob, scores and predict are required'),
    'ff_decode_sequence_sample/sizes:N_0': (-1, 'ff_decode_sequence_sample: bad sizes'),
    'ff_decode_sequence_sample/draw:top_k': (-1, 'ff_decode_sequence_sample: temperature=1 must be finite and >= 0, top_k=-1 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_sequence_sample/draw:top_p_0': (-1, 'ff_decode_sequence_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=0 in (0, 1]'),
    'ff_decode_sequence_sample/draw:top_p_2': (-1, 'ff_decode_sequence_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=2 in (0, 1]'),
    'ff_decode_sequence_sample/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_sequence_beam/null': (-1, 'ff_decode_sequence_beam: null model, params or beam params'),
    'ff_decode_sequence_beam/null+variant': (-1, 'ff_decode_sequence_beam: null model, params or beam params'),
    'ff_decode_sequence_beam/variant': (-1, 'ff_decode_sequence_beam: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_beam'),
    'ff_decode_sequence_beam/variant+excluded': (-1, 'ff_decode_sequence_beam: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_beam'),
    'ff_decode_sequence_beam/excluded': (-1, 'ff_decode_sequence_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_beam/excluded+width': (-1, 'ff_decode_sequence_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_beam/width': (-1, 'ff_decode_sequence_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_sequence_beam/width+stop_best': (-1, 'ff_decode_sequence_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_sequence_beam/stop_best': (-1, 'ff_decode_sequence_beam: stop_best=2 must be 0 or 1'),
    'ff_decode_sequence_beam/stop_best+outputs': (-1, 'ff_decode_sequence_beam: stop_best=2 must be 0 or 1'),
    'ff_decode_sequence_beam/outputs': (-1, 'ff_decode_sequence_beam: beams, scores, finished and predict are required'),
    'ff_decode_sequence_beam/outputs+sizes': (-1, 'ff_decode_sequence_beam: beams, scores, finished and predict are required'),
    'ff_decode_sequence_beam/sizes': (-1, 'ff_decode_sequence_beam: bad sizes'),
    'ff_decode_sequence_beam/sizes+staging': (-1, 'ff_decode_sequence_beam: bad sizes'),
    'ff_decode_sequence_beam/staging': (-1, "ff_decode_sequence_beam: width=3 at E=8192 exceeds the reorder's staging area"),
    'ff_decode_sequence_beam/null:model': (-1, 'ff_decode_sequence_beam: null model, params or beam params'),
    'ff_decode_sequence_beam/null:params': (-1, 'ff_decode_sequence_beam: null model, params or beam params'),
    'ff_decode_sequence_beam/variant:F': (-1, 'ff_decode_sequence_beam: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_beam'),
    'ff_decode_sequence_beam/excluded:retire': (-1, 'ff_decode_sequence_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_beam/excluded:return_pointer': (-1, 'ff_decode_sequence_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_beam/excluded:each_eos': (-1, 'ff_decode_sequence_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_beam/excluded:stop_fn': (-1, 'ff_decode_sequence_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_beam/width:0': (-1, 'ff_decode_sequence_beam: width=0 outside 1..8 or above S=16'),
    'ff_decode_sequence_beam/width:S': (-1, 'ff_decode_sequence_beam: width=5 outside 1..8 or above S=4'),
    'ff_decode_sequence_beam/stop_best:-1': (-1, 'ff_decode_sequence_beam: stop_best=-1 must be 0 or 1'),
    'ff_decode_sequence_beam/outputs:predict': (-1, 'ff_decode_sequence_beam: beams, scores, finished and predict are required'),
    'ff_decode_sequence_beam/outputs:beams': (-1, 'ff_decode_sequence_beam: beams, scores, finished and predict are required'),
    'ff_decode_sequence_beam/outputs:scores': (-1, 'ff_decode_sequence_beam: beams, scores, finished and predict are required'),
    'ff_decode_sequence_beam/outputs:finished': (-1, 'ff_decode_sequence_beam: beams, scores, finished and predict are required'),
    'ff_decode_sequence_beam/sizes:N_0': (-1, 'ff_decode_sequence_beam: bad sizes'),
    'ff_decode_sequence_beam/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_sequence_constrained/null': (-1, 'ff_decode_sequence_constrained: null model, params or constrain params'),
    'ff_decode_sequence_constrained/null+variant': (-1, 'ff_decode_sequence_constrained: null model, params or constrain params'),
    'ff_decode_sequence_constrained/variant': (-1, 'ff_decode_sequence_constrained: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained'),
    'ff_decode_sequence_constrained/variant+excluded': (-1, 'ff_decode_sequence_constrained: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained'),
    'ff_decode_sequence_constrained/excluded': (-1, 'ff_decode_sequence_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained/excluded+rule_flags': (-1, 'ff_decode_sequence_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained/rule_flags': (-1, 'ff_decode_sequence_constrained: unknown flag bits 64'),
    'ff_decode_sequence_constrained/rule_once': (-1, 'ff_decode_sequence_constrained: FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT'),
    'ff_decode_sequence_constrained/rule_once+rule_tokens': (-1, 'ff_decode_sequence_constrained: FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT'),
    'ff_decode_sequence_constrained/rule_tokens': (-1, 'ff_decode_sequence_constrained: tok_sep=1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained/rule_tokens+rule_follows': (-1, 'ff_decode_sequence_constrained: tok_sep=1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained/rule_follows': (-1, 'ff_decode_sequence_constrained: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_sequence_constrained/rule_follows+outputs': (-1, 'ff_decode_sequence_constrained: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_sequence_constrained/outputs': (-1, 'ff_decode_sequence_constrained: logprob, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained/null:model': (-1, 'ff_decode_sequence_constrained: null model, params or constrain params'),
    'ff_decode_sequence_constrained/null:params': (-1, 'ff_decode_sequence_constrained: null model, params or constrain params'),
    'ff_decode_sequence_constrained/variant:F': (-1, 'ff_decode_sequence_constrained: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained'),
    'ff_decode_sequence_constrained/excluded:retire': (-1, 'ff_decode_sequence_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained/excluded:return_pointer': (-1, 'ff_decode_sequence_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained/excluded:each_eos': (-1, 'ff_decode_sequence_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained/excluded:stop_fn': (-1, 'ff_decode_sequence_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained/rule_tokens:sep_-1': (-1, 'ff_decode_sequence_constrained: tok_sep=-1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained/rule_tokens:sep_4': (-1, 'ff_decode_sequence_constrained: tok_sep=4 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained/rule_tokens:eos_-1': (-1, 'ff_decode_sequence_constrained: tok_sep=2 and tok_eos=-1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained/rule_tokens:eos_4': (-1, 'ff_decode_sequence_constrained: tok_sep=2 and tok_eos=4 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained/outputs:predict': (-1, 'ff_decode_sequence_constrained: logprob, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained/outputs:open_end': (-1, 'ff_decode_sequence_constrained: logprob, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained/outputs:logprob': (-1, 'ff_decode_sequence_constrained: logprob, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained/outputs:dead_end': (-1, 'ff_decode_sequence_constrained: logprob, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_sequence_constrained_sample/null': (-1, 'ff_decode_sequence_constrained_sample: null model, params or constrain sample params'),
    'ff_decode_sequence_constrained_sample/null+variant': (-1, 'ff_decode_sequence_constrained_sample: null model, params or constrain sample params'),
    'ff_decode_sequence_constrained_sample/variant': (-1, 'ff_decode_sequence_constrained_sample: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained_sample'),
    'ff_decode_sequence_constrained_sample/variant+excluded': (-1, 'ff_decode_sequence_constrained_sample: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained_sample'),
    'ff_decode_sequence_constrained_sample/excluded': (-1, 'ff_decode_sequence_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_sample/excluded+num_samples': (-1, 'ff_decode_sequence_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_sample/num_samples': (-1, 'ff_decode_sequence_constrained_sample: num_samples=65 outside 1..64'),
    'ff_decode_sequence_constrained_sample/num_samples+rule_flags': (-1, 'ff_decode_sequence_constrained_sample: num_samples=65 outside 1..64'),
    'ff_decode_sequence_constrained_sample/rule_flags': (-1, 'ff_decode_sequence_constrained_sample: unknown flag bits 64'),
    'ff_decode_sequence_constrained_sample/rule_once': (-1, 'ff_decode_sequence_constrained_sample: FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT'),
    'ff_decode_sequence_constrained_sample/rule_once+rule_tokens': (-1, 'ff_decode_sequence_constrained_sample: FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT'),
    'ff_decode_sequence_constrained_sample/rule_tokens': (-1, 'ff_decode_sequence_constrained_sample: tok_sep=1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_sample/rule_tokens+rule_follows': (-1, 'ff_decode_sequence_constrained_sample: tok_sep=1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_sample/rule_follows': (-1, 'ff_decode_sequence_constrained_sample: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_sequence_constrained_sample/rule_follows+outputs': (-1, 'ff_decode_sequence_constrained_sample: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_sequence_constrained_sample/outputs': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs+sizes': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/sizes': (-1, 'ff_decode_sequence_constrained_sample: bad sizes'),
    'ff_decode_sequence_constrained_sample/sizes+draw': (-1, 'ff_decode_sequence_constrained_sample: bad sizes'),
    'ff_decode_sequence_constrained_sample/draw': (-1, 'ff_decode_sequence_constrained_sample: temperature=-1 must be finite and >= 0, top_k=0 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_sequence_constrained_sample/null:model': (-1, 'ff_decode_sequence_constrained_sample: null model, params or constrain sample params'),
    'ff_decode_sequence_constrained_sample/null:params': (-1, 'ff_decode_sequence_constrained_sample: null model, params or constrain sample params'),
    'ff_decode_sequence_constrained_sample/variant:F': (-1, 'ff_decode_sequence_constrained_sample: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained_sample'),
    'ff_decode_sequence_constrained_sample/excluded:retire': (-1, 'ff_decode_sequence_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_sample/excluded:return_pointer': (-1, 'ff_decode_sequence_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_sample/excluded:each_eos': (-1, 'ff_decode_sequence_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_sample/excluded:stop_fn': (-1, 'ff_decode_sequence_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_sample/num_samples:0': (-1, 'ff_decode_sequence_constrained_sample: num_samples=0 outside 1..64'),
    'ff_decode_sequence_constrained_sample/rule_tokens:sep_-1': (-1, 'ff_decode_sequence_constrained_sample: tok_sep=-1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_sample/rule_tokens:sep_4': (-1, 'ff_decode_sequence_constrained_sample: tok_sep=4 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_sample/rule_tokens:eos_-1': (-1, 'ff_decode_sequence_constrained_sample: tok_sep=2 and tok_eos=-1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_sample/rule_tokens:eos_4': (-1, 'ff_decode_sequence_constrained_sample: tok_sep=2 and tok_eos=4 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_sample/outputs:predict': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:uniforms': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:samples': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:logprob': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:scores': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:dead_end': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:open_end': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:predict_logprob': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:predict_dead_end': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/outputs:predict_open_end': (-1, 'ff_decode_sequence_constrained_sample: uniforms, samples, logprob, scores, dead_end, open_end, the three predict_ outputs and predict are required'),
    'ff_decode_sequence_constrained_sample/sizes:N_0': (-1, 'ff_decode_sequence_constrained_sample: bad sizes'),
    'ff_decode_sequence_constrained_sample/draw:top_k': (-1, 'ff_decode_sequence_constrained_sample: temperature=1 must be finite and >= 0, top_k=-1 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_sequence_constrained_sample/draw:top_p_0': (-1, 'ff_decode_sequence_constrained_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=0 in (0, 1]'),
    'ff_decode_sequence_constrained_sample/draw:top_p_2': (-1, 'ff_decode_sequence_constrained_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=2 in (0, 1]'),
    'ff_decode_sequence_constrained_sample/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_sequence_constrained_beam/null': (-1, 'ff_decode_sequence_constrained_beam: null model, params or constrain beam params'),
    'ff_decode_sequence_constrained_beam/null+variant': (-1, 'ff_decode_sequence_constrained_beam: null model, params or constrain beam params'),
    'ff_decode_sequence_constrained_beam/variant': (-1, 'ff_decode_sequence_constrained_beam: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained_beam'),
    'ff_decode_sequence_constrained_beam/variant+excluded': (-1, 'ff_decode_sequence_constrained_beam: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained_beam'),
    'ff_decode_sequence_constrained_beam/excluded': (-1, 'ff_decode_sequence_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_beam/excluded+width': (-1, 'ff_decode_sequence_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_beam/width': (-1, 'ff_decode_sequence_constrained_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_sequence_constrained_beam/width+stop_best': (-1, 'ff_decode_sequence_constrained_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_sequence_constrained_beam/stop_best': (-1, 'ff_decode_sequence_constrained_beam: stop_best=2 must be 0 or 1'),
    'ff_decode_sequence_constrained_beam/stop_best+rule_flags': (-1, 'ff_decode_sequence_constrained_beam: stop_best=2 must be 0 or 1'),
    'ff_decode_sequence_constrained_beam/rule_flags': (-1, 'ff_decode_sequence_constrained_beam: unknown flag bits 64'),
    'ff_decode_sequence_constrained_beam/rule_once': (-1, 'ff_decode_sequence_constrained_beam: FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT'),
    'ff_decode_sequence_constrained_beam/rule_once+rule_tokens': (-1, 'ff_decode_sequence_constrained_beam: FF_CONSTRAIN_ONCE needs FF_CONSTRAIN_NO_REPEAT'),
    'ff_decode_sequence_constrained_beam/rule_tokens': (-1, 'ff_decode_sequence_constrained_beam: tok_sep=1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_beam/rule_tokens+rule_follows': (-1, 'ff_decode_sequence_constrained_beam: tok_sep=1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_beam/rule_follows': (-1, 'ff_decode_sequence_constrained_beam: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_sequence_constrained_beam/rule_follows+outputs': (-1, 'ff_decode_sequence_constrained_beam: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_sequence_constrained_beam/outputs': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs+sizes': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/sizes': (-1, 'ff_decode_sequence_constrained_beam: bad sizes'),
    'ff_decode_sequence_constrained_beam/sizes+staging': (-1, 'ff_decode_sequence_constrained_beam: bad sizes'),
    'ff_decode_sequence_constrained_beam/staging': (-1, "ff_decode_sequence_constrained_beam: width=3 at E=8192 exceeds the reorder's staging area"),
    'ff_decode_sequence_constrained_beam/null:model': (-1, 'ff_decode_sequence_constrained_beam: null model, params or constrain beam params'),
    'ff_decode_sequence_constrained_beam/null:params': (-1, 'ff_decode_sequence_constrained_beam: null model, params or constrain beam params'),
    'ff_decode_sequence_constrained_beam/variant:F': (-1, 'ff_decode_sequence_constrained_beam: a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant has ff_decode_constrained_beam'),
    'ff_decode_sequence_constrained_beam/excluded:retire': (-1, 'ff_decode_sequence_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_beam/excluded:return_pointer': (-1, 'ff_decode_sequence_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_beam/excluded:each_eos': (-1, 'ff_decode_sequence_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_beam/excluded:stop_fn': (-1, 'ff_decode_sequence_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, FF_STOP_EACH_EOS and a stop_fn'),
    'ff_decode_sequence_constrained_beam/width:0': (-1, 'ff_decode_sequence_constrained_beam: width=0 outside 1..8 or above S=16'),
    'ff_decode_sequence_constrained_beam/width:S': (-1, 'ff_decode_sequence_constrained_beam: width=5 outside 1..8 or above S=4'),
    'ff_decode_sequence_constrained_beam/stop_best:-1': (-1, 'ff_decode_sequence_constrained_beam: stop_best=-1 must be 0 or 1'),
    'ff_decode_sequence_constrained_beam/rule_tokens:sep_-1': (-1, 'ff_decode_sequence_constrained_beam: tok_sep=-1 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_beam/rule_tokens:sep_4': (-1, 'ff_decode_sequence_constrained_beam: tok_sep=4 and tok_eos=1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_beam/rule_tokens:eos_-1': (-1, 'ff_decode_sequence_constrained_beam: tok_sep=2 and tok_eos=-1 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_beam/rule_tokens:eos_4': (-1, 'ff_decode_sequence_constrained_beam: tok_sep=2 and tok_eos=4 must be two of the 4 special tokens'),
    'ff_decode_sequence_constrained_beam/outputs:predict': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs:beams': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs:scores': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs:finished': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs:beam_dead_end': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs:beam_open_end': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs:dead_end': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/outputs:open_end': (-1, 'ff_decode_sequence_constrained_beam: beams, scores, finished, beam_dead_end, beam_open_end, dead_end, open_end and predict are required'),
    'ff_decode_sequence_constrained_beam/sizes:N_0': (-1, 'ff_decode_sequence_constrained_beam: bad sizes'),
    'ff_decode_sequence_constrained_beam/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained/null': (-1, 'ff_decode_constrained: null model, params or constrain params'),
    'ff_decode_constrained/null+variant': (-1, 'ff_decode_constrained: null model, params or constrain params'),
    'ff_decode_constrained/variant': (-1, 'ff_decode_constrained: the constrained decode is a parallel-variant option'),
    'ff_decode_constrained/variant+excluded': (-1, 'ff_decode_constrained: the constrained decode is a parallel-variant option'),
    'ff_decode_constrained/excluded': (-1, 'ff_decode_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained/excluded+rule_flags': (-1, 'ff_decode_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained/rule_flags': (-1, 'ff_decode_constrained: unknown flag bits 64'),
    'ff_decode_constrained/rule_flags+rule_range': (-1, 'ff_decode_constrained: unknown flag bits 64'),
    'ff_decode_constrained/rule_range': (-1, 'ff_decode_constrained: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained/rule_range+rule_follows': (-1, 'ff_decode_constrained: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained/rule_follows': (-1, 'ff_decode_constrained: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained/rule_follows+outputs': (-1, 'ff_decode_constrained: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained/outputs': (-1, 'ff_decode_constrained: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained/null:model': (-1, 'ff_decode_constrained: null model, params or constrain params'),
    'ff_decode_constrained/null:params': (-1, 'ff_decode_constrained: null model, params or constrain params'),
    'ff_decode_constrained/excluded:retire': (-1, 'ff_decode_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained/excluded:return_pointer': (-1, 'ff_decode_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained/excluded:stop_fn': (-1, 'ff_decode_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained/excluded:extra_mask': (-1, 'ff_decode_constrained: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained/rule_range:lo': (-1, 'ff_decode_constrained: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained/rule_range:empty': (-1, 'ff_decode_constrained: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained/outputs:trace_best': (-1, 'ff_decode_constrained: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained/outputs:trace_second': (-1, 'ff_decode_constrained: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained/outputs:pointer_out': (-1, 'ff_decode_constrained: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained/outputs:logprob': (-1, 'ff_decode_constrained: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained/outputs:dead_end': (-1, 'ff_decode_constrained: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained_ahead/null': (-1, 'ff_decode_constrained_ahead: null model, params or look-ahead params'),
    'ff_decode_constrained_ahead/null+variant': (-1, 'ff_decode_constrained_ahead: null model, params or look-ahead params'),
    'ff_decode_constrained_ahead/variant': (-1, 'ff_decode_constrained_ahead: the constrained decode with look-ahead is a parallel-variant option'),
    'ff_decode_constrained_ahead/variant+excluded': (-1, 'ff_decode_constrained_ahead: the constrained decode with look-ahead is a parallel-variant option'),
    'ff_decode_constrained_ahead/excluded': (-1, 'ff_decode_constrained_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_ahead/excluded+rule_flags': (-1, 'ff_decode_constrained_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_ahead/rule_flags': (-1, 'ff_decode_constrained_ahead: unknown flag bits 64'),
    'ff_decode_constrained_ahead/rule_flags+rule_range': (-1, 'ff_decode_constrained_ahead: unknown flag bits 64'),
    'ff_decode_constrained_ahead/rule_range': (-1, 'ff_decode_constrained_ahead: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_ahead/rule_range+rule_follows': (-1, 'ff_decode_constrained_ahead: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_ahead/rule_follows': (-1, 'ff_decode_constrained_ahead: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_ahead/ahead_flags': (-1, 'ff_decode_constrained_ahead: the look-ahead needs FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_ahead/ahead_flags+ahead_tables': (-1, 'ff_decode_constrained_ahead: the look-ahead needs FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_ahead/ahead_tables': (-1, 'ff_decode_constrained_ahead: close_dist and cycle_len are required'),
    'ff_decode_constrained_ahead/ahead_tables+ahead_T': (-1, 'ff_decode_constrained_ahead: close_dist and cycle_len are required'),
    'ff_decode_constrained_ahead/ahead_T': (-1, "ff_decode_constrained_ahead: T=257 above 256 (the budget T - 2 must fit the tables' byte)"),
    'ff_decode_constrained_ahead/ahead_T+outputs': (-1, "ff_decode_constrained_ahead: T=257 above 256 (the budget T - 2 must fit the tables' byte)"),
    'ff_decode_constrained_ahead/outputs': (-1, 'ff_decode_constrained_ahead: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_ahead/null:model': (-1, 'ff_decode_constrained_ahead: null model, params or look-ahead params'),
    'ff_decode_constrained_ahead/null:params': (-1, 'ff_decode_constrained_ahead: null model, params or look-ahead params'),
    'ff_decode_constrained_ahead/excluded:retire': (-1, 'ff_decode_constrained_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_ahead/excluded:return_pointer': (-1, 'ff_decode_constrained_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_ahead/excluded:stop_fn': (-1, 'ff_decode_constrained_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_ahead/excluded:extra_mask': (-1, 'ff_decode_constrained_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_ahead/rule_range:lo': (-1, 'ff_decode_constrained_ahead: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained_ahead/rule_range:empty': (-1, 'ff_decode_constrained_ahead: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained_ahead/ahead_tables:cycle_len': (-1, 'ff_decode_constrained_ahead: close_dist and cycle_len are required'),
    'ff_decode_constrained_ahead/outputs:trace_best': (-1, 'ff_decode_constrained_ahead: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_ahead/outputs:trace_second': (-1, 'ff_decode_constrained_ahead: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_ahead/outputs:pointer_out': (-1, 'ff_decode_constrained_ahead: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_ahead/outputs:logprob': (-1, 'ff_decode_constrained_ahead: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_ahead/outputs:dead_end': (-1, 'ff_decode_constrained_ahead: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_ahead/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained_exact/null': (-1, 'ff_decode_constrained_exact: null model, params or exact look-ahead params'),
    'ff_decode_constrained_exact/null+variant': (-1, 'ff_decode_constrained_exact: null model, params or exact look-ahead params'),
    'ff_decode_constrained_exact/variant': (-1, 'ff_decode_constrained_exact: the constrained decode with exact look-ahead is a parallel-variant option'),
    'ff_decode_constrained_exact/variant+excluded': (-1, 'ff_decode_constrained_exact: the constrained decode with exact look-ahead is a parallel-variant option'),
    'ff_decode_constrained_exact/excluded': (-1, 'ff_decode_constrained_exact: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_exact/excluded+rule_flags': (-1, 'ff_decode_constrained_exact: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_exact/rule_flags': (-1, 'ff_decode_constrained_exact: unknown flag bits 64'),
    'ff_decode_constrained_exact/rule_flags+rule_range': (-1, 'ff_decode_constrained_exact: unknown flag bits 64'),
    'ff_decode_constrained_exact/rule_range': (-1, 'ff_decode_constrained_exact: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_exact/rule_range+rule_follows': (-1, 'ff_decode_constrained_exact: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_exact/rule_follows': (-1, 'ff_decode_constrained_exact: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_exact/exact_flags': (-1, 'ff_decode_constrained_exact: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_exact/exact_flags+exact_table': (-1, 'ff_decode_constrained_exact: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_exact/exact_table': (-1, 'ff_decode_constrained_exact: cycle_len is required'),
    'ff_decode_constrained_exact/exact_table+exact_T': (-1, 'ff_decode_constrained_exact: cycle_len is required'),
    'ff_decode_constrained_exact/exact_T': (-1, "ff_decode_constrained_exact: T=257 above 256 (the budget T - 2 must fit the table's byte)"),
    'ff_decode_constrained_exact/exact_T+exact_L': (-1, "ff_decode_constrained_exact: T=257 above 256 (the budget T - 2 must fit the table's byte)"),
    'ff_decode_constrained_exact/exact_L': (-1, 'ff_decode_constrained_exact: L=2045 above 2044 (L + num_token keys at most 2048)'),
    'ff_decode_constrained_exact/exact_L+outputs': (-1, 'ff_decode_constrained_exact: L=2045 above 2044 (L + num_token keys at most 2048)'),
    'ff_decode_constrained_exact/outputs': (-1, 'ff_decode_constrained_exact: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_exact/null:model': (-1, 'ff_decode_constrained_exact: null model, params or exact look-ahead params'),
    'ff_decode_constrained_exact/null:params': (-1, 'ff_decode_constrained_exact: null model, params or exact look-ahead params'),
    'ff_decode_constrained_exact/excluded:retire': (-1, 'ff_decode_constrained_exact: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_exact/excluded:return_pointer': (-1, 'ff_decode_constrained_exact: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_exact/excluded:stop_fn': (-1, 'ff_decode_constrained_exact: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_exact/excluded:extra_mask': (-1, 'ff_decode_constrained_exact: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_exact/rule_range:lo': (-1, 'ff_decode_constrained_exact: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained_exact/rule_range:empty': (-1, 'ff_decode_constrained_exact: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained_exact/exact_flags:no_repeat_only': (-1, 'ff_decode_constrained_exact: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_exact/outputs:trace_best': (-1, 'ff_decode_constrained_exact: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_exact/outputs:trace_second': (-1, 'ff_decode_constrained_exact: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_exact/outputs:pointer_out': (-1, 'ff_decode_constrained_exact: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_exact/outputs:logprob': (-1, 'ff_decode_constrained_exact: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_exact/outputs:dead_end': (-1, 'ff_decode_constrained_exact: logprob and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_exact/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained_beam/null': (-1, 'ff_decode_constrained_beam: null model, params or beam params'),
    'ff_decode_constrained_beam/null+variant': (-1, 'ff_decode_constrained_beam: null model, params or beam params'),
    'ff_decode_constrained_beam/variant': (-1, 'ff_decode_constrained_beam: the constrained beam decode is a parallel-variant option'),
    'ff_decode_constrained_beam/variant+excluded': (-1, 'ff_decode_constrained_beam: the constrained beam decode is a parallel-variant option'),
    'ff_decode_constrained_beam/excluded': (-1, 'ff_decode_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam/excluded+width': (-1, 'ff_decode_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam/width': (-1, 'ff_decode_constrained_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam/width+rule_flags': (-1, 'ff_decode_constrained_beam: width=9 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam/rule_flags': (-1, 'ff_decode_constrained_beam: unknown flag bits 64'),
    'ff_decode_constrained_beam/rule_flags+rule_range': (-1, 'ff_decode_constrained_beam: unknown flag bits 64'),
    'ff_decode_constrained_beam/rule_range': (-1, 'ff_decode_constrained_beam: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam/rule_range+rule_follows': (-1, 'ff_decode_constrained_beam: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam/rule_follows': (-1, 'ff_decode_constrained_beam: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_beam/rule_follows+outputs': (-1, 'ff_decode_constrained_beam: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_beam/outputs': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/outputs+staging': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/staging': (-1, "ff_decode_constrained_beam: width=3 at E=8192 exceeds the reorder's staging area"),
    'ff_decode_constrained_beam/null:model': (-1, 'ff_decode_constrained_beam: null model, params or beam params'),
    'ff_decode_constrained_beam/null:params': (-1, 'ff_decode_constrained_beam: null model, params or beam params'),
    'ff_decode_constrained_beam/excluded:retire': (-1, 'ff_decode_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam/excluded:return_pointer': (-1, 'ff_decode_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam/excluded:stop_fn': (-1, 'ff_decode_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam/excluded:extra_mask': (-1, 'ff_decode_constrained_beam: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam/width:0': (-1, 'ff_decode_constrained_beam: width=0 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam/width:S': (-1, 'ff_decode_constrained_beam: width=5 outside 1..8 or above S=4'),
    'ff_decode_constrained_beam/rule_range:lo': (-1, 'ff_decode_constrained_beam: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam/rule_range:empty': (-1, 'ff_decode_constrained_beam: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam/outputs:trace_best': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/outputs:trace_second': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/outputs:pointer_out': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/outputs:beams': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/outputs:scores': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/outputs:dead_end': (-1, 'ff_decode_constrained_beam: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained_beam_ahead[ahead]/null': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[ahead]/null+variant': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[ahead]/variant': (-1, 'ff_decode_constrained_beam_ahead: the constrained beam decode with look-ahead is a parallel-variant option'),
    'ff_decode_constrained_beam_ahead[ahead]/variant+excluded': (-1, 'ff_decode_constrained_beam_ahead: the constrained beam decode with look-ahead is a parallel-variant option'),
    'ff_decode_constrained_beam_ahead[ahead]/excluded': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[ahead]/excluded+width': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[ahead]/width': (-1, 'ff_decode_constrained_beam_ahead: width=9 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam_ahead[ahead]/width+rule_flags': (-1, 'ff_decode_constrained_beam_ahead: width=9 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_flags': (-1, 'ff_decode_constrained_beam_ahead: unknown flag bits 64'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_flags+rule_range': (-1, 'ff_decode_constrained_beam_ahead: unknown flag bits 64'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_range': (-1, 'ff_decode_constrained_beam_ahead: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_range+rule_follows': (-1, 'ff_decode_constrained_beam_ahead: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_follows': (-1, 'ff_decode_constrained_beam_ahead: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_follows+lookahead': (-1, 'ff_decode_constrained_beam_ahead: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_beam_ahead[ahead]/lookahead': (-1, 'ff_decode_constrained_beam_ahead: lookahead=3 must be 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_beam_ahead[ahead]/lookahead+ahead_flags': (-1, 'ff_decode_constrained_beam_ahead: lookahead=3 must be 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_beam_ahead[ahead]/ahead_flags': (-1, 'ff_decode_constrained_beam_ahead: the look-ahead needs FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_beam_ahead[ahead]/ahead_flags+ahead_tables': (-1, 'ff_decode_constrained_beam_ahead: the look-ahead needs FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_beam_ahead[ahead]/ahead_tables': (-1, 'ff_decode_constrained_beam_ahead: close_dist and cycle_len are required'),
    'ff_decode_constrained_beam_ahead[ahead]/ahead_tables+ahead_T': (-1, 'ff_decode_constrained_beam_ahead: close_dist and cycle_len are required'),
    'ff_decode_constrained_beam_ahead[ahead]/ahead_T': (-1, "ff_decode_constrained_beam_ahead: T=257 above 256 (the budget T - 2 must fit the tables' byte)"),
    'ff_decode_constrained_beam_ahead[ahead]/ahead_T+outputs': (-1, "ff_decode_constrained_beam_ahead: T=257 above 256 (the budget T - 2 must fit the tables' byte)"),
    'ff_decode_constrained_beam_ahead[ahead]/outputs': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/outputs+staging': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/staging': (-1, "ff_decode_constrained_beam_ahead: width=3 at E=8192 exceeds the reorder's staging area"),
    'ff_decode_constrained_beam_ahead[ahead]/null:model': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[ahead]/null:params': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[ahead]/excluded:retire': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[ahead]/excluded:return_pointer': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[ahead]/excluded:stop_fn': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[ahead]/excluded:extra_mask': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[ahead]/width:0': (-1, 'ff_decode_constrained_beam_ahead: width=0 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam_ahead[ahead]/width:S': (-1, 'ff_decode_constrained_beam_ahead: width=5 outside 1..8 or above S=4'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_range:lo': (-1, 'ff_decode_constrained_beam_ahead: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[ahead]/rule_range:empty': (-1, 'ff_decode_constrained_beam_ahead: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[ahead]/lookahead:-1': (-1, 'ff_decode_constrained_beam_ahead: lookahead=-1 must be 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_beam_ahead[ahead]/ahead_tables:cycle_len': (-1, 'ff_decode_constrained_beam_ahead: close_dist and cycle_len are required'),
    'ff_decode_constrained_beam_ahead[ahead]/outputs:trace_best': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/outputs:trace_second': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/outputs:pointer_out': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/outputs:beams': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/outputs:scores': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/outputs:dead_end': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[ahead]/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained_beam_ahead[exact]/null': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[exact]/null+variant': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[exact]/variant': (-1, 'ff_decode_constrained_beam_ahead: the constrained beam decode with look-ahead is a parallel-variant option'),
    'ff_decode_constrained_beam_ahead[exact]/variant+excluded': (-1, 'ff_decode_constrained_beam_ahead: the constrained beam decode with look-ahead is a parallel-variant option'),
    'ff_decode_constrained_beam_ahead[exact]/excluded': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[exact]/excluded+width': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[exact]/width': (-1, 'ff_decode_constrained_beam_ahead: width=9 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam_ahead[exact]/width+rule_flags': (-1, 'ff_decode_constrained_beam_ahead: width=9 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam_ahead[exact]/rule_flags': (-1, 'ff_decode_constrained_beam_ahead: unknown flag bits 64'),
    'ff_decode_constrained_beam_ahead[exact]/rule_flags+rule_range': (-1, 'ff_decode_constrained_beam_ahead: unknown flag bits 64'),
    'ff_decode_constrained_beam_ahead[exact]/rule_range': (-1, 'ff_decode_constrained_beam_ahead: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[exact]/rule_range+rule_follows': (-1, 'ff_decode_constrained_beam_ahead: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[exact]/rule_follows': (-1, 'ff_decode_constrained_beam_ahead: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_beam_ahead[exact]/rule_follows+lookahead': (-1, 'ff_decode_constrained_beam_ahead: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_beam_ahead[exact]/lookahead': (-1, 'ff_decode_constrained_beam_ahead: lookahead=3 must be 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_beam_ahead[exact]/lookahead+exact_flags': (-1, 'ff_decode_constrained_beam_ahead: lookahead=3 must be 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_beam_ahead[exact]/exact_flags': (-1, 'ff_decode_constrained_beam_ahead: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_beam_ahead[exact]/exact_flags+exact_table': (-1, 'ff_decode_constrained_beam_ahead: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_beam_ahead[exact]/exact_table': (-1, 'ff_decode_constrained_beam_ahead: cycle_len is required'),
    'ff_decode_constrained_beam_ahead[exact]/exact_table+exact_T': (-1, 'ff_decode_constrained_beam_ahead: cycle_len is required'),
    'ff_decode_constrained_beam_ahead[exact]/exact_T': (-1, "ff_decode_constrained_beam_ahead: T=257 above 256 (the budget T - 2 must fit the table's byte)"),
    'ff_decode_constrained_beam_ahead[exact]/exact_T+exact_L': (-1, "ff_decode_constrained_beam_ahead: T=257 above 256 (the budget T - 2 must fit the table's byte)"),
    'ff_decode_constrained_beam_ahead[exact]/exact_L': (-1, 'ff_decode_constrained_beam_ahead: L=2045 above 2044 (L + num_token keys at most 2048)'),
    'ff_decode_constrained_beam_ahead[exact]/exact_L+outputs': (-1, 'ff_decode_constrained_beam_ahead: L=2045 above 2044 (L + num_token keys at most 2048)'),
    'ff_decode_constrained_beam_ahead[exact]/outputs': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/outputs+staging': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/staging': (-1, "ff_decode_constrained_beam_ahead: width=3 at E=8192 exceeds the reorder's staging area"),
    'ff_decode_constrained_beam_ahead[exact]/null:model': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[exact]/null:params': (-1, 'ff_decode_constrained_beam_ahead: null model, params or beam params'),
    'ff_decode_constrained_beam_ahead[exact]/excluded:retire': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[exact]/excluded:return_pointer': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[exact]/excluded:stop_fn': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[exact]/excluded:extra_mask': (-1, 'ff_decode_constrained_beam_ahead: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_beam_ahead[exact]/width:0': (-1, 'ff_decode_constrained_beam_ahead: width=0 outside 1..8 or above S=16'),
    'ff_decode_constrained_beam_ahead[exact]/width:S': (-1, 'ff_decode_constrained_beam_ahead: width=5 outside 1..8 or above S=4'),
    'ff_decode_constrained_beam_ahead[exact]/rule_range:lo': (-1, 'ff_decode_constrained_beam_ahead: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[exact]/rule_range:empty': (-1, 'ff_decode_constrained_beam_ahead: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained_beam_ahead[exact]/lookahead:-1': (-1, 'ff_decode_constrained_beam_ahead: lookahead=-1 must be 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_beam_ahead[exact]/exact_flags:no_repeat_only': (-1, 'ff_decode_constrained_beam_ahead: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_beam_ahead[exact]/outputs:trace_best': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/outputs:trace_second': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/outputs:pointer_out': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/outputs:beams': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/outputs:scores': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/outputs:dead_end': (-1, 'ff_decode_constrained_beam_ahead: beams, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_beam_ahead[exact]/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained_sample[ahead]/null': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[ahead]/null+variant': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[ahead]/variant': (-1, 'ff_decode_constrained_sample: the constrained sampled decode is a parallel-variant option'),
    'ff_decode_constrained_sample[ahead]/variant+excluded': (-1, 'ff_decode_constrained_sample: the constrained sampled decode is a parallel-variant option'),
    'ff_decode_constrained_sample[ahead]/excluded': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[ahead]/excluded+num_samples': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[ahead]/num_samples': (-1, 'ff_decode_constrained_sample: num_samples=65 outside 1..64'),
    'ff_decode_constrained_sample[ahead]/num_samples+rule_flags': (-1, 'ff_decode_constrained_sample: num_samples=65 outside 1..64'),
    'ff_decode_constrained_sample[ahead]/rule_flags': (-1, 'ff_decode_constrained_sample: unknown flag bits 64'),
    'ff_decode_constrained_sample[ahead]/rule_flags+rule_range': (-1, 'ff_decode_constrained_sample: unknown flag bits 64'),
    'ff_decode_constrained_sample[ahead]/rule_range': (-1, 'ff_decode_constrained_sample: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[ahead]/rule_range+rule_follows': (-1, 'ff_decode_constrained_sample: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[ahead]/rule_follows': (-1, 'ff_decode_constrained_sample: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_sample[ahead]/rule_follows+lookahead': (-1, 'ff_decode_constrained_sample: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_sample[ahead]/lookahead': (-1, 'ff_decode_constrained_sample: lookahead=3 must be 0 (none), 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_sample[ahead]/lookahead+ahead_flags': (-1, 'ff_decode_constrained_sample: lookahead=3 must be 0 (none), 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_sample[ahead]/ahead_flags': (-1, 'ff_decode_constrained_sample: the look-ahead needs FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_sample[ahead]/ahead_flags+ahead_tables': (-1, 'ff_decode_constrained_sample: the look-ahead needs FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_sample[ahead]/ahead_tables': (-1, 'ff_decode_constrained_sample: close_dist and cycle_len are required'),
    'ff_decode_constrained_sample[ahead]/ahead_tables+ahead_T': (-1, 'ff_decode_constrained_sample: close_dist and cycle_len are required'),
    'ff_decode_constrained_sample[ahead]/ahead_T': (-1, "ff_decode_constrained_sample: T=257 above 256 (the budget T - 2 must fit the tables' byte)"),
    'ff_decode_constrained_sample[ahead]/ahead_T+outputs': (-1, "ff_decode_constrained_sample: T=257 above 256 (the budget T - 2 must fit the tables' byte)"),
    'ff_decode_constrained_sample[ahead]/outputs': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs+sizes': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/sizes': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[ahead]/sizes+draw': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[ahead]/draw': (-1, 'ff_decode_constrained_sample: temperature=-1 must be finite and >= 0, top_k=0 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_constrained_sample[ahead]/null:model': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[ahead]/null:params': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[ahead]/excluded:retire': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[ahead]/excluded:return_pointer': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[ahead]/excluded:stop_fn': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[ahead]/excluded:extra_mask': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[ahead]/num_samples:0': (-1, 'ff_decode_constrained_sample: num_samples=0 outside 1..64'),
    'ff_decode_constrained_sample[ahead]/rule_range:lo': (-1, 'ff_decode_constrained_sample: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[ahead]/rule_range:empty': (-1, 'ff_decode_constrained_sample: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[ahead]/lookahead:-1': (-1, 'ff_decode_constrained_sample: lookahead=-1 must be 0 (none), 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_sample[ahead]/ahead_tables:cycle_len': (-1, 'ff_decode_constrained_sample: close_dist and cycle_len are required'),
    'ff_decode_constrained_sample[ahead]/outputs:trace_best': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs:trace_second': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs:pointer_out': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs:uniforms': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs:samples': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs:logprob': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs:scores': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/outputs:dead_end': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[ahead]/sizes:N_0': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[ahead]/sizes:F_0': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[ahead]/draw:top_k': (-1, 'ff_decode_constrained_sample: temperature=1 must be finite and >= 0, top_k=-1 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_constrained_sample[ahead]/draw:top_p_0': (-1, 'ff_decode_constrained_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=0 in (0, 1]'),
    'ff_decode_constrained_sample[ahead]/draw:top_p_2': (-1, 'ff_decode_constrained_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=2 in (0, 1]'),
    'ff_decode_constrained_sample[ahead]/pass': (-1, 'ff_decode: null pointer'),
    'ff_decode_constrained_sample[exact]/null': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[exact]/null+variant': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[exact]/variant': (-1, 'ff_decode_constrained_sample: the constrained sampled decode is a parallel-variant option'),
    'ff_decode_constrained_sample[exact]/variant+excluded': (-1, 'ff_decode_constrained_sample: the constrained sampled decode is a parallel-variant option'),
    'ff_decode_constrained_sample[exact]/excluded': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[exact]/excluded+num_samples': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[exact]/num_samples': (-1, 'ff_decode_constrained_sample: num_samples=65 outside 1..64'),
    'ff_decode_constrained_sample[exact]/num_samples+rule_flags': (-1, 'ff_decode_constrained_sample: num_samples=65 outside 1..64'),
    'ff_decode_constrained_sample[exact]/rule_flags': (-1, 'ff_decode_constrained_sample: unknown flag bits 64'),
    'ff_decode_constrained_sample[exact]/rule_flags+rule_range': (-1, 'ff_decode_constrained_sample: unknown flag bits 64'),
    'ff_decode_constrained_sample[exact]/rule_range': (-1, 'ff_decode_constrained_sample: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[exact]/rule_range+rule_follows': (-1, 'ff_decode_constrained_sample: terminator range [2, 9) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[exact]/rule_follows': (-1, 'ff_decode_constrained_sample: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_sample[exact]/rule_follows+lookahead': (-1, 'ff_decode_constrained_sample: FF_CONSTRAIN_CONNECT needs the follow table'),
    'ff_decode_constrained_sample[exact]/lookahead': (-1, 'ff_decode_constrained_sample: lookahead=3 must be 0 (none), 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_sample[exact]/lookahead+exact_flags': (-1, 'ff_decode_constrained_sample: lookahead=3 must be 0 (none), 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_sample[exact]/exact_flags': (-1, 'ff_decode_constrained_sample: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_sample[exact]/exact_flags+exact_table': (-1, 'ff_decode_constrained_sample: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_sample[exact]/exact_table': (-1, 'ff_decode_constrained_sample: cycle_len is required'),
    'ff_decode_constrained_sample[exact]/exact_table+exact_T': (-1, 'ff_decode_constrained_sample: cycle_len is required'),
    'ff_decode_constrained_sample[exact]/exact_T': (-1, "ff_decode_constrained_sample: T=257 above 256 (the budget T - 2 must fit the table's byte)"),
    'ff_decode_constrained_sample[exact]/exact_T+exact_L': (-1, "ff_decode_constrained_sample: T=257 above 256 (the budget T - 2 must fit the table's byte)"),
    'ff_decode_constrained_sample[exact]/exact_L': (-1, 'ff_decode_constrained_sample: L=2045 above 2044 (L + num_token keys at most 2048)'),
    'ff_decode_constrained_sample[exact]/exact_L+outputs': (-1, 'ff_decode_constrained_sample: L=2045 above 2044 (L + num_token keys at most 2048)'),
    'ff_decode_constrained_sample[exact]/outputs': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs+sizes': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/sizes': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[exact]/sizes+draw': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[exact]/draw': (-1, 'ff_decode_constrained_sample: temperature=-1 must be finite and >= 0, top_k=0 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_constrained_sample[exact]/null:model': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[exact]/null:params': (-1, 'ff_decode_constrained_sample: null model, params or constrained sample params'),
    'ff_decode_constrained_sample[exact]/excluded:retire': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[exact]/excluded:return_pointer': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[exact]/excluded:stop_fn': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[exact]/excluded:extra_mask': (-1, 'ff_decode_constrained_sample: excludes FF_RETIRE_FINISHED, FF_RETURN_POINTER, FF_NO_STOP, a stop_fn and an extra mask'),
    'ff_decode_constrained_sample[exact]/num_samples:0': (-1, 'ff_decode_constrained_sample: num_samples=0 outside 1..64'),
    'ff_decode_constrained_sample[exact]/rule_range:lo': (-1, 'ff_decode_constrained_sample: terminator range [-1, 4) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[exact]/rule_range:empty': (-1, 'ff_decode_constrained_sample: terminator range [2, 2) empty or outside the 4 special tokens'),
    'ff_decode_constrained_sample[exact]/lookahead:-1': (-1, 'ff_decode_constrained_sample: lookahead=-1 must be 0 (none), 1 (look-ahead) or 2 (exact)'),
    'ff_decode_constrained_sample[exact]/exact_flags:no_repeat_only': (-1, 'ff_decode_constrained_sample: the exact look-ahead needs FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT'),
    'ff_decode_constrained_sample[exact]/outputs:trace_best': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs:trace_second': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs:pointer_out': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs:uniforms': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs:samples': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs:logprob': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs:scores': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/outputs:dead_end': (-1, 'ff_decode_constrained_sample: uniforms, samples, logprob, scores and dead_end required; no best / second traces, no pointer_out'),
    'ff_decode_constrained_sample[exact]/sizes:N_0': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[exact]/sizes:F_0': (-1, 'ff_decode_constrained_sample: bad sizes'),
    'ff_decode_constrained_sample[exact]/draw:top_k': (-1, 'ff_decode_constrained_sample: temperature=1 must be finite and >= 0, top_k=-1 >= 0, top_p=1 in (0, 1]'),
    'ff_decode_constrained_sample[exact]/draw:top_p_0': (-1, 'ff_decode_constrained_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=0 in (0, 1]'),
    'ff_decode_constrained_sample[exact]/draw:top_p_2': (-1, 'ff_decode_constrained_sample: temperature=1 must be finite and >= 0, top_k=0 >= 0, top_p=2 in (0, 1]'),
    'ff_decode_constrained_sample[exact]/pass': (-1, 'ff_decode: null pointer'),
}


def test_every_case_is_recorded():
    assert list(case_ids()) == list(EXPECTED)
    assert {e.split("[")[0] for e in CHECKS} == {k for k in L.SIGNATURES if k.startswith("ff_decode_") and not k.endswith("_bytes")
                                                 and k != "ff_decode_lp"}


@pytest.mark.parametrize("entry", list(CHECKS))
def test_entry_refuses_as_recorded(hip_lib, entry):
    for case in case_ids():
        if case.split("/")[0] == entry:
            assert call(hip_lib, case) == EXPECTED[case], case


def test_a_pair_reports_the_earlier_check():
    """The recorded table itself has the property the pairs are there for; and an entry that passes hands on to the decode."""
    for case, want in EXPECTED.items():
        entry, names = case.split("/")
        if ":" in names:
            assert want[0] == -1 and want != EXPECTED[entry + "/pass"], case
        elif "+" in names:
            assert want == EXPECTED["%s/%s" % (entry, names.split("+")[0])], case
            assert want != EXPECTED["%s/%s" % (entry, names.split("+")[1])], case
        if names == "pass":
            assert want == (-1, "ff_decode: null pointer"), case


if __name__ == "__main__":
    lib = L.load()
    print("EXPECTED = {")
    for case in case_ids():
        print("    %r: %r," % (case, call(lib, case)))
    print("}")
