"""The one place the Python side describes a decode mode: greedy (with its options retire and logprob), beam,
sample, constrained, and forced (score()).  A `Mode` record holds what PathEngine.decode / score, the models, dist.decode_sharded
and main.py need to know about a mode; `check_options` words every combination error from it.  The C side's counterpart is the
`Mode` descriptor of ff_decode (csrc/ff_engine.hip); the per-mode entries and their parameter structs are lib.py's."""
import collections
import ctypes as C

import torch

from . import lib as _L
from .ops import EXACT_MAX_KEYS, _dev, _p      # (EXACT_MAX_KEYS: L + num_token the exact look-ahead's search takes)

SAMPLE_MAX = 64
CONSTRAIN_MODES = {"no_repeat": _L.FF_CONSTRAIN_NO_REPEAT, "loops": _L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT}


class Switch(collections.namedtuple("Switch", "attr off sharded seq2seq scored")):
    """A model attribute that switches a mode (or an option of the greedy mode) on: its name and `off` value, why decode_sharded /
    the single-sequence model do not take it (None: they do), whether score() hands it to the engine (False: rejects it itself)."""

    def on(self, model):
        v = getattr(model, self.attr, self.off)
        return v is not None if self.off is None else bool(v)      # (constrain = 0, the flag bits of no rule, is on)


# subject        the mode as the error texts name it (beam, sample, constrain: the option of decode() that switches it on)
# excludes       the options of decode() / score() it cannot be combined with, in the order the text lists them
# term_range     needs term_range = (lo, hi);  parallel_only: a parallel-variant option
# entry          the C entry (its size query is <entry>_workspace_bytes)
# per_anchor     the option's value is G, the sequences per anchor: the size query's extra argument, the factor of the trace rows
# row_traces     the per-row fp32 traces beside `logits` (beam's beam_parent, an int32 one, is made by its `tail`)
# values / values_first   the mode's value check over the options `o`, and whether it runs before the exclusions or after them
# operand        (engine, o): decode()'s shape check of the operand only this mode reads
# own, outs, tail   see outputs(): (name, dtype) of the operand only this mode reads; the outputs as (key, dimensions, dtype) --
#                a model publishes them as inputs["predict_" + key], viewed N x F x the dimensions; (o, the outputs' addresses,
#                traced) -> the arguments only this entry takes
# switches       the model attributes: [0] switches the mode on (greedy: its two options)
# model_excludes the model-level exclusions in the words of that text;  model_checked: forward_eval runs check_options itself
# prepare        (model, value, inputs, device, T, N, F, num_input, order) -> the keyword arguments of decode()
# sequence       a single-sequence mode's companion record (SEQUENCE_MODES below); None for every other mode
Mode = collections.namedtuple(
    "Mode", "subject excludes entry term_range parallel_only per_anchor row_traces values values_first operand own outs tail "
            "switches model_excludes model_checked prepare sequence",
    defaults=(True, True, False, (), lambda *a: None, False, lambda *a: None, (), (), lambda *a: (), (), (), False, lambda *a: {}, None))

# What only a single-sequence mode has:
# value          the option's value check: the decode() argument / model attribute -> the value, or the switch's `off` value
# parallel_has   (verb, option): "the parallel variant <verb> with <option>", "SurfaceFormer_Parallel <verb> per anchor with <option>"
# model_has      the words of "is a SurfaceFormer option (...)";  each: what its own EOS finishes (the noun of the stop_each_eos text)
# early          (engine, o): decode()'s check in front of the variant check (None: none)
# model_values   (model, value, inputs): the value checks only the model can make, behind the native-engine check and the exclusions
# stats          the model attribute that receives steps and slot_rows
Sequence = collections.namedtuple("Sequence", "value parallel_has model_has each model_values stats early", defaults=(None,))


def check_options(mode, variant, o, term_range):
    """Every variant, exclusion and term_range error of a mode, with the mode's value check (`o`: the options by decode()'s
    names), as ValueError before anything is launched.  Returns what the value check returns."""
    if mode.parallel_only and variant != _L.FF_PARALLEL:
        raise ValueError("%s is a parallel-variant option" % mode.subject)
    if mode.values_first:
        mode.values(o)
    if any(o.get(k) is not None if k in ("stop_callback", "extra_mask") else o.get(k) for k in mode.excludes):
        raise ValueError("%s excludes %s and %s" % (mode.subject, ", ".join(mode.excludes[:-1]), mode.excludes[-1]))
    if mode.term_range and (term_range is None or len(term_range) != 2 or not int(term_range[0]) < int(term_range[1])):
        raise ValueError("%s needs term_range = (lo, hi) with lo < hi" % mode.subject)
    if not mode.values_first:
        return mode.values(o)


def constrain_flags(constrain):
    """The flag bits of a `constrain` value: None -> None (the option is off), "no_repeat" / "loops", or the bits themselves
    (0..3: the C entries also take CONNECT alone, and 0, which is the plumbing's identity with the retired greedy decode)."""
    if constrain is None:
        return None
    if isinstance(constrain, str):
        if constrain not in CONSTRAIN_MODES:
            raise ValueError("constrain=%r: must be None, 'no_repeat' or 'loops'" % (constrain,))
        return CONSTRAIN_MODES[constrain]
    if isinstance(constrain, bool) or not isinstance(constrain, int) or not 0 <= constrain <= 3:
        raise ValueError("constrain=%r: must be None, 'no_repeat', 'loops' or flag bits 0..3" % (constrain,))
    return int(constrain)


# ---- the value checks ------------------------------------------------------------------------------------------------------------
def _beam_values(o):
    if not 1 <= o["beam_width"] <= 8 or o["beam_width"] > o["S"]:
        raise ValueError("beam_width=%d: must be in 1..8 and at most S = %d" % (o["beam_width"], o["S"]))


def _sample_values(o):
    if not 1 <= o["num_samples"] <= SAMPLE_MAX:
        raise ValueError("num_samples=%d: must be in 1..%d" % (o["num_samples"], SAMPLE_MAX))
    t, k, pp = float(o["temperature"]), int(o["top_k"]), float(o["top_p"])
    if not (0.0 <= t < float("inf")) or k < 0 or not (0.0 < pp <= 1.0):
        raise ValueError("sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]: got %r, %r, %r"
                         % (o["temperature"], o["top_k"], o["top_p"]))


def _sample_operand(eng, o):
    shape = (max(o["T"] - 1, 1), o["N"] * o["F"] * o["num_samples"])
    u = o["uniforms"]
    if not torch.is_tensor(u) or u.dtype != torch.float32 or tuple(u.shape) != shape:
        raise ValueError("uniforms must be a float32 tensor of shape [%d, %d]" % shape)


def _constrain_values(o):
    if o["constrain"] & _L.FF_CONSTRAIN_CONNECT and o["follow_table"] is None:
        raise ValueError("constrain='loops' needs follow_table (ops.follow_table)")


def constrain_beams_value(constrain_beams, flags):
    """The width of a `constrain_beams` value: None / 0 -> 0 (the option is off); else 1..8, and only with `constrain` set
    (`flags`: constrain_flags of it)."""
    if constrain_beams is None or (not isinstance(constrain_beams, bool) and constrain_beams == 0):
        return 0
    if isinstance(constrain_beams, bool) or not isinstance(constrain_beams, int) or not 1 <= constrain_beams <= 8:
        raise ValueError("constrain_beams=%r: must be None, 0 or a width in 1..8" % (constrain_beams,))
    if flags is None:
        raise ValueError("constrain_beams=%d needs constrain ('no_repeat' or 'loops'): it is the beam search over the constrained keys"
                         % constrain_beams)
    return int(constrain_beams)


def _constrain_beam_values(o):
    if not 1 <= o["constrain_beams"] <= 8 or o["constrain_beams"] > o["S"]:
        raise ValueError("constrain_beams=%d: must be in 1..8 and at most S = %d" % (o["constrain_beams"], o["S"]))
    _constrain_values(o)


BEAM_CLOSURES = {"lookahead": 1, "exact": 2}      # constrain_beam_closure -> the `lookahead` form of the C entries


def constrain_beam_closure_value(closure, flags, constrain_beams=0, constrain_lookahead=False, constrain_exact=False,
                                 constrain_samples=0):
    """The form of a `constrain_beam_closure` value: None -> None (the option is off); else "lookahead" or "exact",
    only with constrain='loops' (`flags`: constrain_flags of it) and constrain_beams >= 1, and not with the greedy / sampled
    decode's own look-ahead options (which exclude constrain_beams with their own texts before this is asked)."""
    if closure is None:
        return None
    if not isinstance(closure, str) or closure not in BEAM_CLOSURES:
        raise ValueError("constrain_beam_closure=%r: must be None, 'lookahead' or 'exact'" % (closure,))
    if not constrain_beams:
        raise ValueError("constrain_beam_closure=%r needs constrain_beams: it is the closure look-ahead of the beam search over the "
                         "constrained keys" % closure)
    if flags != CONSTRAIN_MODES["loops"]:
        raise ValueError("constrain_beam_closure=%r needs constrain='loops' (FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT): without "
                         "CONNECT no loop is tracked" % closure)
    if constrain_lookahead or constrain_exact or constrain_samples:
        raise ValueError("constrain_beam_closure excludes constrain_lookahead, constrain_exact and constrain_samples: they are the "
                         "look-aheads of the greedy and the sampled decode")
    return closure


def _constrain_beam_ahead_values(o):
    _constrain_beam_values(o)
    exact = o["constrain_beam_closure"] == "exact"
    if o["T"] > 256:
        raise ValueError("constrain_beam_closure takes T <= 256 (got %d): the budget T - 2 must fit the tables' byte" % o["T"])
    for name in ("cycle_len",) if exact else ("close_dist", "cycle_len"):
        if o[name] is None:
            raise ValueError("constrain_beam_closure=%r needs %s (ops.follow_distance)"
                             % (o["constrain_beam_closure"], "cycle_len" if exact else "close_dist and cycle_len"))


def _constrain_beam_ahead_operand(eng, o):
    _constrain_operand(eng, o)
    L = o["S"] - eng.num_token
    exact = o["constrain_beam_closure"] == "exact"
    if exact and o["S"] > EXACT_MAX_KEYS:
        raise ValueError("constrain_beam_closure='exact' takes at most %d edges per wireframe (got %d): L + num_token <= %d keys"
                         % (EXACT_MAX_KEYS - eng.num_token, L, EXACT_MAX_KEYS))
    for name, shape in (("cycle_len", (o["N"], L)),) if exact else (("close_dist", (o["N"], L, L)), ("cycle_len", (o["N"], L))):
        t = o[name]
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != shape:
            raise ValueError("%s must be a uint8 tensor of shape [%s]" % (name, ", ".join(str(v) for v in shape)))


def constrain_lookahead_value(lookahead, flags, constrain_beams=0):
    """Whether the closure look-ahead is on (`constrain_lookahead`): only with constrain='loops' (`flags`:
    constrain_flags of it -- the look-ahead masks under CONNECT) and not with constrain_beams."""
    if not lookahead:
        return False
    if flags is None:
        raise ValueError("constrain_lookahead needs constrain='loops': it is the closure look-ahead of the loop-constrained decode")
    if not flags & _L.FF_CONSTRAIN_CONNECT:
        raise ValueError("constrain_lookahead needs constrain='loops' (FF_CONSTRAIN_CONNECT): without it no loop is tracked")
    if constrain_beams:
        raise ValueError("constrain_lookahead excludes constrain_beams: the beam search over the constrained keys has no look-ahead")
    return True


def _constrain_ahead_values(o):
    _constrain_values(o)
    if o["T"] > 256:
        raise ValueError("constrain_lookahead takes T <= 256 (got %d): the budget T - 2 must fit the tables' byte" % o["T"])
    for name in ("close_dist", "cycle_len"):
        if o[name] is None:
            raise ValueError("constrain_lookahead needs close_dist and cycle_len (ops.follow_distance)")


def _constrain_ahead_operand(eng, o):
    _constrain_operand(eng, o)
    L = o["S"] - eng.num_token
    for name, shape in (("close_dist", (o["N"], L, L)), ("cycle_len", (o["N"], L))):
        t = o[name]
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != shape:
            raise ValueError("%s must be a uint8 tensor of shape [%s]" % (name, ", ".join(str(v) for v in shape)))


def constrain_exact_value(exact, flags, constrain_beams=0, constrain_lookahead=False):
    """Whether the exact closure look-ahead is on (`constrain_exact`): only with constrain='loops' (`flags`:
    constrain_flags of it -- it needs CONNECT for the loop and NO_REPEAT for `visited`), not with constrain_lookahead, which it
    contains, and not with constrain_beams."""
    if not exact:
        return False
    if flags is None:
        raise ValueError("constrain_exact needs constrain='loops': it is the exact closure look-ahead of the loop-constrained decode")
    if flags != CONSTRAIN_MODES["loops"]:
        raise ValueError("constrain_exact needs constrain='loops' (FF_CONSTRAIN_NO_REPEAT | FF_CONSTRAIN_CONNECT): without CONNECT "
                         "no loop is tracked, without NO_REPEAT there is no visited set to be exact about")
    if constrain_lookahead:
        raise ValueError("constrain_exact excludes constrain_lookahead: it contains it (every edge the look-ahead masks is masked)")
    if constrain_beams:
        raise ValueError("constrain_exact excludes constrain_beams: the beam search over the constrained keys has no look-ahead")
    return True


def _constrain_exact_values(o):
    _constrain_values(o)
    if o["T"] > 256:
        raise ValueError("constrain_exact takes T <= 256 (got %d): the budget T - 2 must fit the table's byte" % o["T"])
    if o["cycle_len"] is None:
        raise ValueError("constrain_exact needs cycle_len (ops.follow_distance)")


def _constrain_exact_operand(eng, o):
    _constrain_operand(eng, o)
    L = o["S"] - eng.num_token
    if o["S"] > EXACT_MAX_KEYS:
        raise ValueError("constrain_exact takes at most %d edges per wireframe (got %d): L + num_token <= %d keys"
                         % (EXACT_MAX_KEYS - eng.num_token, L, EXACT_MAX_KEYS))
    t = o["cycle_len"]
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != (o["N"], L):
        raise ValueError("cycle_len must be a uint8 tensor of shape [%d, %d]" % (o["N"], L))


def constrain_samples_value(constrain_samples, flags, constrain_beams=0):
    """The count of a `constrain_samples` value: None / 0 -> 0 (the option is off); else 1..SAMPLE_MAX, only with
    `constrain` set (`flags`: constrain_flags of it) and not with constrain_beams."""
    if constrain_samples is None or (not isinstance(constrain_samples, bool) and constrain_samples == 0):
        return 0
    if isinstance(constrain_samples, bool) or not isinstance(constrain_samples, int) or not 1 <= constrain_samples <= SAMPLE_MAX:
        raise ValueError("constrain_samples=%r: must be None, 0 or a count in 1..%d" % (constrain_samples, SAMPLE_MAX))
    if flags is None:
        raise ValueError("constrain_samples=%d needs constrain ('no_repeat' or 'loops'): it is the sampling over the constrained keys"
                         % constrain_samples)
    if constrain_beams:
        raise ValueError("constrain_samples excludes constrain_beams: a decode draws from the constrained keys or searches them")
    return int(constrain_samples)


def _constrain_sample_values(o):
    """constrain's value check, the sampled decode's on constrain_samples and the parameters, and the selected look-ahead's."""
    _sample_values(dict(o, num_samples=o["constrain_samples"]))
    if o["constrain_exact"]:
        _constrain_exact_values(o)
    elif o["constrain_lookahead"]:
        _constrain_ahead_values(o)
    else:
        _constrain_values(o)


def _constrain_sample_operand(eng, o):
    if o["constrain_exact"]:
        _constrain_exact_operand(eng, o)
    elif o["constrain_lookahead"]:
        _constrain_ahead_operand(eng, o)
    else:
        _constrain_operand(eng, o)
    _sample_operand(eng, dict(o, num_samples=o["constrain_samples"]))


def _constrain_operand(eng, o):
    L = o["S"] - eng.num_token
    shape = (o["N"], L, (L + 31) // 32)
    ft = o["follow_table"]
    if ft is not None and (not torch.is_tensor(ft) or ft.dtype != torch.int32 or tuple(ft.shape) != shape):
        raise ValueError("follow_table must be an int32 tensor of shape [%d, %d, %d]" % shape)


def _retire_values(o):
    if o["num_input"] is None and o["staged_num_input"] is None:
        raise ValueError("retire=True needs num_input")


def _forced_values(o):
    """The one pass over the paths: every token of positions 0..lengths[r] must lie in [0, S) -- the C entry cannot see them and
    would clamp.  Returns (paths int64 [rows, T], lengths as a list)."""
    paths, lengths, rows, T, S = o["paths"], o["lengths"], o["rows"], o["T"], o["S"]
    if not torch.is_tensor(paths) or paths.dtype != torch.int64 or paths.dim() != 2 or tuple(paths.shape) != (rows, T):
        raise ValueError("paths must be an int64 tensor of shape [%d, %d]" % (rows, T))
    lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
    if len(lens) != rows or any(not 0 <= v <= T - 1 for v in lens):
        raise ValueError("lengths must hold %d values in 0..%d" % (rows, T - 1))
    if rows:
        used = torch.arange(T, device=paths.device)[None, :] <= torch.tensor(lens, device=paths.device)[:, None]
        bad = used & ((paths < 0) | (paths >= S))
        if bool(bad.any()):
            r, j = [int(v) for v in bad.nonzero()[0]]
            raise ValueError("paths[%d, %d] = %d lies outside [0, %d)" % (r, j, int(paths[r, j]), S))
    return paths, lens


# ---- the outputs -----------------------------------------------------------------------------------------------------------------
def _beam_parent(o, traced):
    """The address of a beam decode's int32 trace `beam_parent` [T-1, rows], made beside `logits` with trace=True (else None)."""
    if o["trace"]:
        logits = traced["logits"]
        traced["beam_parent"] = torch.full(logits.shape[:2], -1, device=logits.device, dtype=torch.int32)
    return _p(traced.get("beam_parent"))


def _beam_tail(o, ptrs, traced):
    return (C.byref(_L.BeamParams(o["beam_width"], *ptrs, _beam_parent(o, traced))),)


def _constrain_beam_tail(o, ptrs, traced):
    return (C.byref(_L.ConstrainBeamParams(o["constrain_beams"], o["constrain"], _p(o["follow_table"]), *ptrs,
                                           _beam_parent(o, traced))),)


def _constrain_beam_ahead_tail(o, ptrs, traced):
    form = BEAM_CLOSURES[o["constrain_beam_closure"]]
    return (C.byref(_L.ConstrainBeamAheadParams(o["constrain_beams"], o["constrain"], _p(o["follow_table"]), form,
                                                _p(o["close_dist"]) if form == 1 else None, _p(o["cycle_len"]), *ptrs,
                                                _beam_parent(o, traced))),)


def outputs(mode, eng, o, B, traced):
    """(the mode's outputs by key: [B * G if "G" is among the dimensions else B, T if "T" is], the arguments only its entry takes:
    its parameter struct, or the log-probability output).  The mode's own operand is checked and made contiguous first."""
    for name, dtype in mode.own:
        if o[name] is not None:
            _dev(o[name], name, dtype)
            eng._same_device(o[name], name)
            o[name] = o[name].contiguous()      # (`o`, which lives as long as the call, keeps a copy alive)
    G = o[mode.subject] if mode.per_anchor else 1
    out = {key: torch.empty((B * G if "G" in dims else B,) + ((o["T"],) if "T" in dims else ()), device=eng.device, dtype=dtype)
           for key, dims, dtype in mode.outs}
    return out, mode.tail(o, [t.data_ptr() for t in out.values()], traced)


# ---- the records -----------------------------------------------------------------------------------------------------------------
_COMMON = ("retire", "return_pointer", "no_stop", "stop_callback", "extra_mask", "logprob")
_NO_STOP_RULE = "a %s decode takes no external stop rule"
_F32, _I32, _I64 = torch.float32, torch.int32, torch.int64

CONSTRAIN = Mode(
    subject="constrain", excludes=_COMMON + ("beam_width", "num_samples"), entry="ff_decode_constrained", values=_constrain_values,
    operand=_constrain_operand, own=(("follow_table", _I32),),
    outs=(("logprob", "T", _F32), ("dead_end", "", _I32)),
    tail=lambda o, ptrs, traced: (C.byref(_L.ConstrainParams(o["constrain"], _p(o["follow_table"]), *ptrs)),),
    switches=(Switch("constrain", None, _NO_STOP_RULE % "constrained", "the single-sequence model emits loops of plain edges", False),),
    model_excludes=("beam_width", "num_samples", "retire_finished", "return_logprob", "an extra mask"),
    # (without CONNECT nothing reads the table: neither the mask nor, first being unused, the closure test)
    prepare=lambda m, CF, inputs, dev, T, N, F, ni, order: dict(
        constrain=CF, follow_table=m._follow_table(inputs, dev, ni, order) if CF & _L.FF_CONSTRAIN_CONNECT else None))

# constrain with its option constrain_beams = W: the beam search over the constrained keys.  Outside MODES, as
# GREEDY_LOGPROB is: the option that switches the mode on stays `constrain`, whose record reports every error without the option.
CONSTRAIN_BEAM = CONSTRAIN._replace(
    subject="constrain_beams", entry="ff_decode_constrained_beam", per_anchor=True, values=_constrain_beam_values,
    outs=(("beams", "GT", _I64), ("beam_scores", "G", _F32), ("beam_dead_end", "G", _I32)), tail=_constrain_beam_tail,
    prepare=lambda m, W, inputs, dev, T, N, F, ni, order: dict(
        CONSTRAIN.prepare(m, constrain_flags(m.constrain), inputs, dev, T, N, F, ni, order), constrain_beams=W))

def _constrain_beam_ahead_prepare(m, W, inputs, dev, T, N, F, ni, order):
    kw = CONSTRAIN_BEAM.prepare(m, W, inputs, dev, T, N, F, ni, order)
    closure = m.constrain_beam_closure
    if closure == "exact":      # (only cycle_len is needed)
        return dict(kw, constrain_beam_closure=closure, cycle_len=m._cycle_len(inputs, dev, T, ni, order, kw["follow_table"]))
    return dict(kw, constrain_beam_closure=closure, **m._follow_distance(inputs, dev, T, ni, order, kw["follow_table"]))


# constrain='loops' with constrain_beams = W and its option constrain_beam_closure: the same beam search with the
# closure look-ahead, or the exact one, in every beam's row of the selection launch.  Outside MODES, as CONSTRAIN_BEAM is; the
# tables are operands beside follow_table.
CONSTRAIN_BEAM_AHEAD = CONSTRAIN_BEAM._replace(
    entry="ff_decode_constrained_beam_ahead", values=_constrain_beam_ahead_values, operand=_constrain_beam_ahead_operand,
    own=(("follow_table", _I32), ("close_dist", torch.uint8), ("cycle_len", torch.uint8)), tail=_constrain_beam_ahead_tail,
    prepare=lambda *a: _constrain_beam_ahead_prepare(*a))


def _constrain_ahead_prepare(m, CF, inputs, dev, T, N, F, ni, order):
    kw = CONSTRAIN.prepare(m, CF, inputs, dev, T, N, F, ni, order)
    return dict(kw, constrain_lookahead=True, **m._follow_distance(inputs, dev, T, ni, order, kw["follow_table"]))


# constrain='loops' with its option constrain_lookahead: the same decode with the closure look-ahead in the
# selection launch.  Outside MODES, as CONSTRAIN_BEAM is; the two tables are operands beside follow_table.
CONSTRAIN_AHEAD = CONSTRAIN._replace(
    subject="constrain_lookahead", entry="ff_decode_constrained_ahead", values=_constrain_ahead_values, operand=_constrain_ahead_operand,
    own=(("follow_table", _I32), ("close_dist", torch.uint8), ("cycle_len", torch.uint8)),
    tail=lambda o, ptrs, traced: (C.byref(_L.ConstrainAheadParams(o["constrain"], _p(o["follow_table"]), _p(o["close_dist"]),
                                                                  _p(o["cycle_len"]), *ptrs)),),
    prepare=lambda *a: _constrain_ahead_prepare(*a))

def _constrain_exact_prepare(m, CF, inputs, dev, T, N, F, ni, order):
    kw = CONSTRAIN.prepare(m, CF, inputs, dev, T, N, F, ni, order)
    return dict(kw, constrain_exact=True, cycle_len=m._cycle_len(inputs, dev, T, ni, order, kw["follow_table"]))


# constrain='loops' with its option constrain_exact: the same decode with the exact closure look-ahead -- a search
# over the unused edges per open row -- in the selection launch.  Outside MODES, as CONSTRAIN_AHEAD is; cycle_len is an operand.
CONSTRAIN_EXACT = CONSTRAIN._replace(
    subject="constrain_exact", entry="ff_decode_constrained_exact", values=_constrain_exact_values, operand=_constrain_exact_operand,
    own=(("follow_table", _I32), ("cycle_len", torch.uint8)),
    tail=lambda o, ptrs, traced: (C.byref(_L.ConstrainExactParams(o["constrain"], _p(o["follow_table"]), _p(o["cycle_len"]), *ptrs)),),
    prepare=lambda *a: _constrain_exact_prepare(*a))

def _constrain_sample_tail(o, ptrs, traced):
    form = 2 if o["constrain_exact"] else (1 if o["constrain_lookahead"] else 0)
    return (C.byref(_L.ConstrainSampleParams(
        o["constrain_samples"], float(o["temperature"]), int(o["top_k"]), float(o["top_p"]), _p(o["uniforms"]), o["constrain"],
        _p(o["follow_table"]), form, _p(o["close_dist"]) if form == 1 else None, _p(o["cycle_len"]) if form else None, *ptrs)),)


def _constrain_sample_prepare(m, R, inputs, dev, T, N, F, ni, order):
    CF = constrain_flags(m.constrain)
    if getattr(m, "constrain_exact", False):
        kw = _constrain_exact_prepare(m, CF, inputs, dev, T, N, F, ni, order)
    elif getattr(m, "constrain_lookahead", False):
        kw = _constrain_ahead_prepare(m, CF, inputs, dev, T, N, F, ni, order)
    else:
        kw = CONSTRAIN.prepare(m, CF, inputs, dev, T, N, F, ni, order)
    return dict(kw, constrain_samples=R, temperature=float(m.sample_temperature), top_k=int(m.sample_top_k),
                top_p=float(m.sample_top_p), uniforms=m._sample_uniforms(inputs, dev, T, N, F, R, order))


# constrain with its option constrain_samples = R: R draws per anchor from the constrained row, in the plain form
# or with constrain_lookahead / constrain_exact.  Outside MODES, as CONSTRAIN_BEAM is.  The outputs: the draws, and draw 0 under
# constrain's own keys (logprob, dead_end).
CONSTRAIN_SAMPLE = CONSTRAIN._replace(
    subject="constrain_samples", entry="ff_decode_constrained_sample", per_anchor=True, values=_constrain_sample_values,
    operand=_constrain_sample_operand,
    own=(("follow_table", _I32), ("uniforms", _F32), ("close_dist", torch.uint8), ("cycle_len", torch.uint8)),
    outs=(("samples", "GT", _I64), ("sample_logprob", "GT", _F32), ("sample_scores", "G", _F32), ("sample_dead_end", "G", _I32),
          ("logprob", "T", _F32), ("dead_end", "", _I32)),
    tail=_constrain_sample_tail, prepare=lambda *a: _constrain_sample_prepare(*a))

SAMPLE = Mode(
    subject="num_samples", excludes=_COMMON + ("beam_width",), entry="ff_decode_sample", per_anchor=True, values=_sample_values,
    values_first=True, operand=_sample_operand, own=(("uniforms", _F32),),
    outs=(("samples", "GT", _I64), ("sample_logprob", "GT", _F32), ("sample_scores", "G", _F32)),
    tail=lambda o, ptrs, traced: (C.byref(_L.SampleParams(o["num_samples"], float(o["temperature"]), int(o["top_k"]),
                                                          float(o["top_p"]), _p(o["uniforms"]), *ptrs)),),
    switches=(Switch("num_samples", 0, _NO_STOP_RULE % "sampled", "sampling for the single-sequence model is not implemented", False),),
    model_excludes=("beam_width", "retire_finished", "return_logprob", "an extra mask"), model_checked=True,
    prepare=lambda m, R, inputs, dev, T, N, F, ni, order: dict(
        num_samples=R, temperature=float(m.sample_temperature), top_k=int(m.sample_top_k), top_p=float(m.sample_top_p),
        uniforms=m._sample_uniforms(inputs, dev, T, N, F, R, order)))

BEAM = Mode(
    subject="beam_width", excludes=_COMMON, entry="ff_decode_beam", per_anchor=True, values=_beam_values, values_first=True,
    outs=(("beams", "GT", _I64), ("beam_scores", "G", _F32)), tail=_beam_tail,
    switches=(Switch("beam_width", 0, _NO_STOP_RULE % "beam", None, True),),
    prepare=lambda m, W, inputs, dev, T, N, F, ni, order: dict(beam_width=W))

# greedy: the exclusions, the variant and the term_range are those of its option retire=True and are checked only with it
GREEDY = Mode(
    subject="retire=True", excludes=("return_pointer", "no_stop", "stop_callback"), entry="ff_decode", row_traces=("best", "second"),
    values=_retire_values,
    switches=(Switch("retire_finished", False, "the batch-global stop rule counts every sequence",
                     "the single-sequence model has one sequence per wireframe", True),
              Switch("return_logprob", False, "the log-probabilities are not gathered across ranks", None, True)))
GREEDY_LOGPROB = GREEDY._replace(entry="ff_decode_lp", outs=(("logprob", "T", _F32),), tail=lambda o, ptrs, traced: tuple(ptrs))

FORCED = Mode(
    subject="scoring given paths", excludes=("retire", "beam_width", "logprob", "return_pointer", "stop_callback", "stop_each_eos", "extra_mask"),
    term_range=False, parallel_only=False, entry="ff_decode_forced", values=_forced_values,
    outs=(("logprob", "T", _F32), ("greedy", "T", _I64), ("rank", "T", _I32), ("seq_logprob", "", _F32)),
    tail=lambda o, ptrs, traced: (C.byref(_L.ForcedParams(_p(o["paths"]), _p(o["lengths_dev"]),
                                                          C.cast(o["lengths_host"], C.POINTER(C.c_int)), *ptrs)),))

# ---- the single-sequence modes (SEQUENCE_MODES) -------------------------------------------------------------------------------------
# The single-sequence model's sampling (R draws per WIREFRAME), beam search (30: W beams per WIREFRAME) and loop
# constraint (32: the face-loop rule per face of the row -- SEP ends a face, a dead end re-opens SEP alone), every sequence from
# SOS and finished by EOS alone.  The three records lie outside MODES, in a table of their own: num_samples, beam_width and
# constrain on that model stay the recorded rejections they are (SWITCH and every recorded text stay), and the options are read
# where the single-sequence model decodes (SurfaceFormer.forward_eval) and refused everywhere else, by loops over SEQUENCE_MODES.
# The terminator range is the entries' own ([tok_eos, tok_eos + 1)): no term_range.  The entries share an argument list of their
# own, shorter than ff_decode's (PathEngine._decode_sequence); one sequence per wireframe under the constraint, so that size
# query takes no count.
def _sequence_sample_values(o):
    R = o["sequence_samples"]
    if isinstance(R, bool) or not isinstance(R, int) or not 1 <= R <= SAMPLE_MAX:
        raise ValueError("sequence_samples=%r: must be in 1..%d" % (R, SAMPLE_MAX))
    _sample_values(dict(o, num_samples=R))      # (temperature, top_k, top_p: the sampled decode's text)


def _sequence_sample_operand(eng, o):
    _sample_operand(eng, dict(o, F=1, num_samples=o["sequence_samples"]))


def sequence_samples_value(sequence_samples):
    """The count of a `sequence_samples` value: None / 0 -> 0 (the option is off); else 1..SAMPLE_MAX."""
    if sequence_samples is None or (not isinstance(sequence_samples, bool) and sequence_samples == 0):
        return 0
    _sequence_sample_values(dict(sequence_samples=sequence_samples, temperature=1.0, top_k=0, top_p=1.0))
    return int(sequence_samples)


def _sequence_sample_model_values(m, R, inputs):
    check_options(SEQUENCE_SAMPLE, _L.FF_SEQ2SEQ, dict(sequence_samples=R, temperature=m.sample_temperature, top_k=m.sample_top_k,
                                                      top_p=m.sample_top_p), None)
    u = inputs.get("sample_uniforms")
    shape = (max(m.num_labels - 1, 1), inputs["input"].size(0) * R)
    if u is not None and tuple(torch.as_tensor(u).shape) != shape:
        raise ValueError("sample_uniforms must have shape [%d, %d]" % shape)


SEQUENCE_SAMPLE = Mode(
    subject="sequence_samples", excludes=_COMMON + ("beam_width", "num_samples", "constrain"), entry="ff_decode_sequence_sample",
    term_range=False, parallel_only=False, per_anchor=True, values=_sequence_sample_values, values_first=True,
    operand=_sequence_sample_operand, own=(("uniforms", _F32),), outs=SAMPLE.outs,
    tail=lambda o, ptrs, traced: (C.byref(_L.SampleParams(o["sequence_samples"], float(o["temperature"]), int(o["top_k"]),
                                                          float(o["top_p"]), _p(o["uniforms"]), *ptrs)),),
    switches=(Switch("sequence_samples", 0, _NO_STOP_RULE % "sequence-sampled", None, False),),
    model_excludes=("return_logprob", "an extra mask"),
    # (the wireframes are decoded in batch order: column w*R + k of the uniforms is draw k of wireframe w as given)
    prepare=lambda m, R, inputs, dev, T, N, F, ni, order: dict(
        sequence_samples=R, temperature=float(m.sample_temperature), top_k=int(m.sample_top_k), top_p=float(m.sample_top_p),
        uniforms=m._sample_uniforms(inputs, dev, T, N, F, R, order)),
    sequence=Sequence(sequence_samples_value, ("draws", "num_samples"), "draws per wireframe of the single-sequence model", "draw",
                      _sequence_sample_model_values, "last_sample_stats"))

SEQUENCE_BEAM_STOPS = {"all": 0, "best": 1}      # sequence_beam_stop -> stop_best of the C entries


def _sequence_beam_values(o):
    W = o["sequence_beams"]
    if isinstance(W, bool) or not isinstance(W, int) or not 1 <= W <= 8 or ("S" in o and W > o["S"]):
        raise ValueError("sequence_beams=%r: must be in 1..8 and at most S%s" % (W, " = %d" % o["S"] if "S" in o else ""))
    sequence_beam_stop_value(o.get("sequence_beam_stop", "all"))


def sequence_beams_value(sequence_beams):
    """The width of a `sequence_beams` value: None / 0 -> 0 (the option is off); else 1..8."""
    if sequence_beams is None or (not isinstance(sequence_beams, bool) and sequence_beams == 0):
        return 0
    _sequence_beam_values(dict(sequence_beams=sequence_beams))
    return int(sequence_beams)


def sequence_beam_stop_value(stop):
    """stop_best of a `sequence_beam_stop` value: "all" -> 0 (stop once no non-empty beam is unfinished), "best" ->
    1 (stop once rank 0 of every wireframe is finished: exact for beam 0, the others are returned as they stand)."""
    if not isinstance(stop, str) or stop not in SEQUENCE_BEAM_STOPS:
        raise ValueError("sequence_beam_stop=%r: must be 'all' or 'best'" % (stop,))
    return SEQUENCE_BEAM_STOPS[stop]


def _sequence_beam_tail(o, ptrs, traced):
    return (C.byref(_L.SequenceBeamParams(o["sequence_beams"], sequence_beam_stop_value(o["sequence_beam_stop"]), *ptrs,
                                          _beam_parent(o, traced))),)


SEQUENCE_BEAM = Mode(
    subject="sequence_beams", excludes=_COMMON + ("beam_width", "num_samples", "constrain", "sequence_samples"),
    entry="ff_decode_sequence_beam", term_range=False, parallel_only=False, per_anchor=True, values=_sequence_beam_values,
    values_first=True, outs=(("beams", "GT", _I64), ("beam_scores", "G", _F32), ("beam_finished", "G", _I32)),
    tail=_sequence_beam_tail, switches=(Switch("sequence_beams", 0, _NO_STOP_RULE % "sequence-beam", None, False),),
    model_excludes=("sequence_samples", "beam_width", "return_logprob", "an extra mask"),
    prepare=lambda m, W, inputs, dev, T, N, F, ni, order: dict(sequence_beams=W, sequence_beam_stop=m.sequence_beam_stop),
    sequence=Sequence(sequence_beams_value, ("searches", "beam_width"), "beams per wireframe of the single-sequence model", "beam",
                      lambda m, W, inputs: check_options(
                          SEQUENCE_BEAM, _L.FF_SEQ2SEQ, dict(sequence_beams=W, sequence_beam_stop=getattr(m, "sequence_beam_stop", "all"),
                                                             S=inputs["input"].size(1) + m.num_token), None), "last_beam_stats"))

SEQUENCE_CONSTRAIN_MODES = {"no_repeat": _L.FF_CONSTRAIN_NO_REPEAT, "loops": _L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT,
                            "coedge_loops": _L.FF_CONSTRAIN_NO_REPEAT | _L.FF_CONSTRAIN_CONNECT | _L.FF_CONSTRAIN_ONCE}


def sequence_constrain_flags(sequence_constrain):
    """The flag bits of a `sequence_constrain` value: None -> None (the option is off), "no_repeat" (1), "loops"
    (3), "coedge_loops" (7: also no co-edge twice in the row), or the bits themselves, 0..7 -- FF_CONSTRAIN_ONCE (4) only together
    with FF_CONSTRAIN_NO_REPEAT, as the C entries take it; 0 is the plumbing's identity with the greedy decode."""
    if sequence_constrain is None:
        return None
    if isinstance(sequence_constrain, str):
        if sequence_constrain not in SEQUENCE_CONSTRAIN_MODES:
            raise ValueError("sequence_constrain=%r: must be None, 'no_repeat', 'loops' or 'coedge_loops'" % (sequence_constrain,))
        return SEQUENCE_CONSTRAIN_MODES[sequence_constrain]
    if isinstance(sequence_constrain, bool) or not isinstance(sequence_constrain, int) or not 0 <= sequence_constrain <= 7:
        raise ValueError("sequence_constrain=%r: must be None, 'no_repeat', 'loops', 'coedge_loops' or flag bits 0..7"
                         % (sequence_constrain,))
    if sequence_constrain & _L.FF_CONSTRAIN_ONCE and not sequence_constrain & _L.FF_CONSTRAIN_NO_REPEAT:
        raise ValueError("sequence_constrain=%d: FF_CONSTRAIN_ONCE (4) needs FF_CONSTRAIN_NO_REPEAT (1)" % sequence_constrain)
    return int(sequence_constrain)


def _sequence_constrain_values(o):
    if o["sequence_constrain"] & _L.FF_CONSTRAIN_CONNECT and o["follow_table"] is None:
        raise ValueError("sequence_constrain with FF_CONSTRAIN_CONNECT ('loops', 'coedge_loops') needs follow_table (ops.follow_table)")


def _sequence_constrain_early(eng, o):
    sep, eos = o["tok_sep"], int(o["tok_eos"])
    if sep is None:
        raise ValueError("sequence_constrain needs tok_sep, the token that ends a face")
    if not (0 <= int(sep) < eng.num_token and 0 <= eos < eng.num_token) or int(sep) == eos:
        raise ValueError("sequence_constrain: tok_sep=%d and tok_eos=%d must be two different special tokens (below %d)"
                         % (int(sep), eos, eng.num_token))


def _sequence_constrain_model_values(m, SC, inputs):
    if getattr(m, "stop_each_eos", False):
        raise ValueError("sequence_constrain excludes stop_each_eos = True: every row is finished by its own EOS already")


SEQUENCE_CONSTRAIN = Mode(
    subject="sequence_constrain", excludes=_COMMON + ("beam_width", "num_samples", "constrain", "sequence_samples", "sequence_beams"),
    entry="ff_decode_sequence_constrained", term_range=False, parallel_only=False, values=_sequence_constrain_values,
    operand=_constrain_operand, own=(("follow_table", _I32),),
    outs=(("logprob", "T", _F32), ("dead_end", "T", _I32), ("open_end", "", _I32)),
    tail=lambda o, ptrs, traced: (C.byref(_L.SequenceConstrainParams(o["sequence_constrain"], _p(o["follow_table"]), int(o["tok_sep"]),
                                                                     *ptrs)),),
    switches=(Switch("sequence_constrain", None, _NO_STOP_RULE % "sequence-constrained", None, False),),
    model_excludes=("sequence_samples", "sequence_beams", "return_logprob", "an extra mask"),
    # (batch order again: the follow table is taken as built or given; without CONNECT nothing reads one)
    prepare=lambda m, SC, inputs, dev, T, N, F, ni, order: dict(
        sequence_constrain=SC, tok_sep=int(getattr(m.token, "SEP", 2)),
        follow_table=m._follow_table(inputs, dev, m._edge_counts(inputs, dev), None) if SC & _L.FF_CONSTRAIN_CONNECT else None),
    sequence=Sequence(sequence_constrain_flags, ("constrains", "constrain"), "the loop rule per face of the single-sequence model's row",
                      "row", _sequence_constrain_model_values, "last_constrain_stats", _sequence_constrain_early))

def sequence_constrain_samples_value(sequence_constrain_samples, flags, sequence_samples=0, sequence_beams=0):
    """The count of a `sequence_constrain_samples` value: None / 0 -> 0 (the option is off); else 1..SAMPLE_MAX,
    only with `sequence_constrain` set (`flags`: sequence_constrain_flags of it) and not with sequence_samples or sequence_beams."""
    if sequence_constrain_samples is None or (not isinstance(sequence_constrain_samples, bool) and sequence_constrain_samples == 0):
        return 0
    if isinstance(sequence_constrain_samples, bool) or not isinstance(sequence_constrain_samples, int) \
            or not 1 <= sequence_constrain_samples <= SAMPLE_MAX:
        raise ValueError("sequence_constrain_samples=%r: must be None, 0 or a count in 1..%d" % (sequence_constrain_samples, SAMPLE_MAX))
    if flags is None:
        raise ValueError("sequence_constrain_samples=%d needs sequence_constrain ('no_repeat', 'loops' or 'coedge_loops'): it is the "
                         "sampling over the keys the face-loop rule allows" % sequence_constrain_samples)
    if sequence_samples or sequence_beams:
        raise ValueError("sequence_constrain_samples excludes sequence_samples and sequence_beams: they draw from / search the "
                         "unconstrained row")
    return int(sequence_constrain_samples)


def _sequence_constrain_sample_values(o):
    """sequence_constrain's value check and the sampled decode's on the count and the parameters."""
    R = o["sequence_constrain_samples"]
    if isinstance(R, bool) or not isinstance(R, int) or not 1 <= R <= SAMPLE_MAX:
        raise ValueError("sequence_constrain_samples=%r: must be in 1..%d" % (R, SAMPLE_MAX))
    _sample_values(dict(o, num_samples=R))      # (temperature, top_k, top_p: the sampled decode's text)
    _sequence_constrain_values(o)


def _sequence_constrain_sample_operand(eng, o):
    _constrain_operand(eng, o)
    _sample_operand(eng, dict(o, F=1, num_samples=o["sequence_constrain_samples"]))


def _sequence_constrain_sample_model_values(m, R, inputs):
    _sample_values(dict(num_samples=R, temperature=m.sample_temperature, top_k=m.sample_top_k, top_p=m.sample_top_p))
    u = inputs.get("sample_uniforms")
    shape = (max(m.num_labels - 1, 1), inputs["input"].size(0) * R)
    if u is not None and tuple(torch.as_tensor(u).shape) != shape:
        raise ValueError("sample_uniforms must have shape [%d, %d]" % shape)


# sequence_constrain with its option sequence_constrain_samples = R: R draws per wireframe from the row the
# face-loop rule leaves.  Outside SEQUENCE_MODES (and MODES), as CONSTRAIN_SAMPLE is outside MODES: the option that switches the
# mode on stays `sequence_constrain`, whose record reports every error without the option -- sequence_constrain with
# sequence_samples stays the recorded refusal it is.  The outputs: the draws, and draw 0 under sequence_constrain's own keys.
SEQUENCE_CONSTRAIN_SAMPLE = SEQUENCE_CONSTRAIN._replace(
    subject="sequence_constrain_samples", entry="ff_decode_sequence_constrained_sample", per_anchor=True,
    values=_sequence_constrain_sample_values, operand=_sequence_constrain_sample_operand,
    own=(("follow_table", _I32), ("uniforms", _F32)),
    outs=(("samples", "GT", _I64), ("sample_logprob", "GT", _F32), ("sample_scores", "G", _F32), ("sample_dead_end", "GT", _I32),
          ("sample_open_end", "G", _I32)) + SEQUENCE_CONSTRAIN.outs,
    tail=lambda o, ptrs, traced: (C.byref(_L.SequenceConstrainSampleParams(
        o["sequence_constrain_samples"], float(o["temperature"]), int(o["top_k"]), float(o["top_p"]), _p(o["uniforms"]),
        o["sequence_constrain"], _p(o["follow_table"]), int(o["tok_sep"]), *ptrs)),),
    # (batch order, as the two records it combines: column w*R + k of the uniforms is draw k of wireframe w as given)
    prepare=lambda m, R, inputs, dev, T, N, F, ni, order: dict(
        SEQUENCE_CONSTRAIN.prepare(m, sequence_constrain_flags(m.sequence_constrain), inputs, dev, T, N, F, ni, order),
        sequence_constrain_samples=R, temperature=float(m.sample_temperature), top_k=int(m.sample_top_k), top_p=float(m.sample_top_p),
        uniforms=m._sample_uniforms(inputs, dev, T, N, F, R, order)),
    sequence=SEQUENCE_CONSTRAIN.sequence._replace(parallel_has=("draws under the rule", "constrain_samples"), each="draw",
                                                  model_has="draws per wireframe under the loop rule of the single-sequence model's row",
                                                  model_values=_sequence_constrain_sample_model_values))

def sequence_constrain_beams_value(sequence_constrain_beams, flags, sequence_samples=0, sequence_beams=0, sequence_constrain_samples=0):
    """The width of a `sequence_constrain_beams` value: None / 0 -> 0 (the option is off); else 1..8, only with
    `sequence_constrain` set (`flags`: sequence_constrain_flags of it) and not with sequence_samples, sequence_beams or
    sequence_constrain_samples."""
    W = sequence_constrain_beams
    if W is None or (not isinstance(W, bool) and W == 0):
        return 0
    if isinstance(W, bool) or not isinstance(W, int) or not 1 <= W <= 8:
        raise ValueError("sequence_constrain_beams=%r: must be None, 0 or a width in 1..8" % (W,))
    if flags is None:
        raise ValueError("sequence_constrain_beams=%d needs sequence_constrain ('no_repeat', 'loops' or 'coedge_loops'): it is the "
                         "beam search over the keys the face-loop rule allows" % W)
    if sequence_samples or sequence_beams or sequence_constrain_samples:
        raise ValueError("sequence_constrain_beams excludes sequence_samples, sequence_beams and sequence_constrain_samples: they draw "
                         "from / search the unconstrained row, or draw under the rule")
    return int(W)


def _sequence_constrain_beam_values(o):
    """sequence_constrain's value check and the sequence beam decode's on the width and the stop rule."""
    W = o["sequence_constrain_beams"]
    if isinstance(W, bool) or not isinstance(W, int) or not 1 <= W <= 8 or ("S" in o and W > o["S"]):
        raise ValueError("sequence_constrain_beams=%r: must be in 1..8 and at most S%s" % (W, " = %d" % o["S"] if "S" in o else ""))
    sequence_beam_stop_value(o.get("sequence_beam_stop", "all"))
    _sequence_constrain_values(o)


def _sequence_constrain_beam_tail(o, ptrs, traced):
    return (C.byref(_L.SequenceConstrainBeamParams(
        o["sequence_constrain_beams"], sequence_beam_stop_value(o["sequence_beam_stop"]), o["sequence_constrain"],
        _p(o["follow_table"]), int(o["tok_sep"]), *ptrs, _beam_parent(o, traced))),)


def _sequence_constrain_beam_model_values(m, W, inputs):
    _sequence_constrain_beam_values(dict(sequence_constrain_beams=W, sequence_beam_stop=getattr(m, "sequence_beam_stop", "all"),
                                         S=inputs["input"].size(1) + m.num_token, sequence_constrain=0, follow_table=None))


# sequence_constrain with its option sequence_constrain_beams = W: the W best rows per wireframe among the rows
# the face-loop rule leaves.  Outside SEQUENCE_MODES (and MODES), as SEQUENCE_CONSTRAIN_SAMPLE is: the option that switches the
# mode on stays `sequence_constrain` -- sequence_constrain with sequence_beams stays the recorded refusal it is.  The outputs:
# the beams, and beam 0 under sequence_constrain's own keys (no per-position log-probability: the beams carry scores).
SEQUENCE_CONSTRAIN_BEAM = SEQUENCE_CONSTRAIN._replace(
    subject="sequence_constrain_beams", entry="ff_decode_sequence_constrained_beam", per_anchor=True,
    values=_sequence_constrain_beam_values,
    outs=(("beams", "GT", _I64), ("beam_scores", "G", _F32), ("beam_finished", "G", _I32), ("beam_dead_end", "GT", _I32),
          ("beam_open_end", "G", _I32), ("dead_end", "T", _I32), ("open_end", "", _I32)),
    tail=_sequence_constrain_beam_tail,
    # (batch order, as the record it extends: beam k of wireframe w as given is row w*W + k)
    prepare=lambda m, W, inputs, dev, T, N, F, ni, order: dict(
        SEQUENCE_CONSTRAIN.prepare(m, sequence_constrain_flags(m.sequence_constrain), inputs, dev, T, N, F, ni, order),
        sequence_constrain_beams=W, sequence_beam_stop=m.sequence_beam_stop),
    sequence=SEQUENCE_CONSTRAIN.sequence._replace(parallel_has=("searches under the rule", "constrain_beams"), each="beam",
                                                  model_has="beams per wireframe under the loop rule of the single-sequence model's row",
                                                  model_values=_sequence_constrain_beam_model_values))

SEQUENCE_CLOSURES = {"lookahead": 1, "exact": 2}      # sequence_constrain_closure -> the `form` of the C entries


def sequence_constrain_closure_value(closure, flags, sequence_constrain_beams=0):
    """The form of a `sequence_constrain_closure` value: None -> None (the option is off); else "lookahead" or
    "exact", only with `sequence_constrain` set to a form that has FF_CONSTRAIN_CONNECT (`flags`: sequence_constrain_flags of it;
    "exact" needs FF_CONSTRAIN_NO_REPEAT as well) and not with sequence_constrain_beams."""
    if closure is None:
        return None
    if not isinstance(closure, str) or closure not in SEQUENCE_CLOSURES:
        raise ValueError("sequence_constrain_closure=%r: must be None, 'lookahead' or 'exact'" % (closure,))
    if flags is None:
        raise ValueError("sequence_constrain_closure=%r needs sequence_constrain ('loops' or 'coedge_loops'): it is the closure "
                         "look-ahead of the face-loop rule" % closure)
    if not flags & _L.FF_CONSTRAIN_CONNECT:
        raise ValueError("sequence_constrain_closure=%r needs sequence_constrain with FF_CONSTRAIN_CONNECT ('loops', 'coedge_loops' or "
                         "the flag bits 3 / 7): without it no loop is tracked" % closure)
    if closure == "exact" and not flags & _L.FF_CONSTRAIN_NO_REPEAT:
        raise ValueError("sequence_constrain_closure='exact' needs FF_CONSTRAIN_NO_REPEAT as well: without it there is no visited set "
                         "to be exact about")
    if sequence_constrain_beams:
        raise ValueError("sequence_constrain_closure excludes sequence_constrain_beams: the beam search over the rows the face-loop "
                         "rule leaves has no look-ahead")
    return closure


def _sequence_closure_values(o, option="sequence_constrain_closure"):
    closure = o[option]
    exact = closure == "exact"
    for name in ("cycle_len",) if exact else ("close_dist", "cycle_len"):
        if o[name] is None:
            raise ValueError("%s=%r needs %s (ops.follow_distance)"
                             % (option, closure, "cycle_len" if exact else "close_dist and cycle_len"))


def _sequence_closure_operand(eng, o, option="sequence_constrain_closure"):
    L = o["S"] - eng.num_token
    exact = o[option] == "exact"
    if exact and o["S"] > EXACT_MAX_KEYS:
        raise ValueError("%s='exact' takes at most %d edges per wireframe (got %d): L + num_token <= %d keys"
                         % (option, EXACT_MAX_KEYS - eng.num_token, L, EXACT_MAX_KEYS))
    for name, shape in (("cycle_len", (o["N"], L)),) if exact else (("close_dist", (o["N"], L, L)), ("cycle_len", (o["N"], L))):
        t = o[name]
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != shape:
            raise ValueError("%s must be a uint8 tensor of shape [%s]" % (name, ", ".join(str(v) for v in shape)))


def _sequence_closure_tail(o, option="sequence_constrain_closure"):
    """(form, close_dist, cycle_len): what the closure entries' parameter structs add."""
    form = SEQUENCE_CLOSURES[o[option]]
    return (form, _p(o["close_dist"]) if form == 1 else None, _p(o["cycle_len"]))


def _sequence_closure_prepare(base, option, m, value, inputs, dev, T, N, F, ni, order):
    """The plain record's keyword arguments, and the tables: built on the device from the follow table (hmax = min(max(T - 2, 1),
    254), the largest budget a step compares against) or taken from inputs["close_dist"] / inputs["cycle_len"]; "exact" builds and
    reads cycle_len only.  Batch order, as the follow table."""
    from . import ops as _ops
    kw = base.prepare(m, value, inputs, dev, T, N, F, ni, order)
    closure = getattr(m, option)
    names = ("cycle_len",) if closure == "exact" else ("close_dist", "cycle_len")
    given = {name: inputs.get(name) for name in names}
    if all(t is None for t in given.values()):
        built = _ops.follow_distance(kw["follow_table"], m._edge_counts(inputs, dev), min(max(T - 2, 1), 254))
        tables = dict(zip(("close_dist", "cycle_len"), built))
    elif any(t is None for t in given.values()):
        raise ValueError("inputs['close_dist'] and inputs['cycle_len'] are given together")
    else:      # (model_values has checked shape and dtype)
        tables = {name: torch.as_tensor(t).to(dev).contiguous() for name, t in given.items()}
    return dict(kw, **{option: closure}, **{name: tables[name] for name in names})


def _sequence_closure_model_values(base, option="sequence_constrain_closure"):
    def check(m, value, inputs):
        base.sequence.model_values(m, value, inputs)
        N, L = inputs["input"].size(0), inputs["input"].size(1)
        closure = getattr(m, option)
        if closure == "exact" and L + m.num_token > EXACT_MAX_KEYS:      # (before the encoder runs)
            raise ValueError("%s='exact' takes at most %d edges per wireframe (got %d): L + num_token <= %d keys"
                             % (option, EXACT_MAX_KEYS - m.num_token, L, EXACT_MAX_KEYS))
        for name, shape in (("close_dist", (N, L, L)), ("cycle_len", (N, L))):
            t = inputs.get(name)
            if t is not None and (torch.as_tensor(t).dtype != torch.uint8 or tuple(torch.as_tensor(t).shape) != shape):
                raise ValueError("%s must be uint8 [%s]" % (name, ", ".join(str(v) for v in shape)))
    return check


def _sequence_closure_record(base, params, entry, option="sequence_constrain_closure"):
    """`base` (SEQUENCE_CONSTRAIN, SEQUENCE_CONSTRAIN_SAMPLE or SEQUENCE_CONSTRAIN_BEAM) with `option` (sequence_constrain_closure;
    the beam record's: sequence_constrain_beam_closure) on: the same outputs under the same keys from the `_ahead` entry, whose
    parameter struct ends in (form, close_dist, cycle_len)."""
    def values(o):
        base.values(o)
        _sequence_closure_values(o, option)

    def operand(eng, o):
        base.operand(eng, o)
        _sequence_closure_operand(eng, o, option)

    def tail(o, ptrs, traced):
        plain = base.tail(o, ptrs, traced)[0]._obj      # (the plain struct, filled as the plain record fills it)
        return (C.byref(params(*[getattr(plain, f) for f, _ in plain._fields_], *_sequence_closure_tail(o, option))),)
    return base._replace(
        entry=entry, values=values, operand=operand, own=base.own + (("close_dist", torch.uint8), ("cycle_len", torch.uint8)), tail=tail,
        prepare=lambda *a: _sequence_closure_prepare(base, option, *a),
        sequence=base.sequence._replace(model_values=_sequence_closure_model_values(base, option)))


# sequence_constrain ('loops' / 'coedge_loops') with its option sequence_constrain_closure: the same greedy / sampled
# decode with the closure look-ahead, or the exact one, in the selection launch.  Outside SEQUENCE_MODES (and MODES), as
# SEQUENCE_CONSTRAIN_SAMPLE is; the tables are operands beside follow_table; the published keys are the plain records'.
SEQUENCE_CONSTRAIN_AHEAD = _sequence_closure_record(
    SEQUENCE_CONSTRAIN, _L.SequenceConstrainAheadParams, "ff_sequence_decode_constrained_ahead")._replace(
        subject="sequence_constrain_closure")
SEQUENCE_CONSTRAIN_SAMPLE_AHEAD = _sequence_closure_record(
    SEQUENCE_CONSTRAIN_SAMPLE, _L.SequenceConstrainSampleAheadParams, "ff_sequence_decode_constrained_sample_ahead")



def sequence_constrain_beam_closure_value(closure, flags, sequence_constrain_beams=0, sequence_constrain_closure=None,
                                          sequence_constrain_samples=0):
    """The form of a `sequence_constrain_beam_closure` value: None -> None (the option is off); else "lookahead" or
    "exact", only with sequence_constrain_beams >= 1 and `sequence_constrain` set to a form that has FF_CONSTRAIN_CONNECT (`flags`:
    sequence_constrain_flags of it; "exact" needs FF_CONSTRAIN_NO_REPEAT as well), and not with sequence_constrain_closure (the
    greedy and the sampled decode's option, which stays refused with beams) or sequence_constrain_samples."""
    if closure is None:
        return None
    if not isinstance(closure, str) or closure not in SEQUENCE_CLOSURES:
        raise ValueError("sequence_constrain_beam_closure=%r: must be None, 'lookahead' or 'exact'" % (closure,))
    if sequence_constrain_closure is not None:
        raise ValueError("sequence_constrain_beam_closure excludes sequence_constrain_closure: that is the look-ahead of the greedy and "
                         "the sampled decode; under sequence_constrain_beams set sequence_constrain_beam_closure alone")
    if sequence_constrain_samples:
        raise ValueError("sequence_constrain_beam_closure excludes sequence_constrain_samples: the sampled decode looks ahead with "
                         "sequence_constrain_closure")
    if not sequence_constrain_beams:
        raise ValueError("sequence_constrain_beam_closure=%r needs sequence_constrain_beams >= 1: it is the closure look-ahead of the "
                         "beam search over the rows the face-loop rule leaves (the greedy decode's is sequence_constrain_closure)"
                         % closure)
    if flags is None:
        raise ValueError("sequence_constrain_beam_closure=%r needs sequence_constrain ('loops' or 'coedge_loops'): it is the closure "
                         "look-ahead of the face-loop rule" % closure)
    if not flags & _L.FF_CONSTRAIN_CONNECT:
        raise ValueError("sequence_constrain_beam_closure=%r needs sequence_constrain with FF_CONSTRAIN_CONNECT ('loops', "
                         "'coedge_loops' or the flag bits 3 / 7): without it no loop is tracked" % closure)
    if closure == "exact" and not flags & _L.FF_CONSTRAIN_NO_REPEAT:
        raise ValueError("sequence_constrain_beam_closure='exact' needs FF_CONSTRAIN_NO_REPEAT as well: without it there is no visited "
                         "set to be exact about")
    return closure


# sequence_constrain_beams with its option sequence_constrain_beam_closure: the same beam search with the closure
# look-ahead, or the exact one, per beam in the selection launch.  Outside SEQUENCE_MODES (and MODES), as SEQUENCE_CONSTRAIN_BEAM
# is; the tables are operands beside follow_table, per wireframe and shared by its beams; the published keys are the plain record's.
SEQUENCE_CONSTRAIN_BEAM_AHEAD = _sequence_closure_record(
    SEQUENCE_CONSTRAIN_BEAM, _L.SequenceConstrainBeamAheadParams, "ff_sequence_decode_constrained_beam_ahead",
    "sequence_constrain_beam_closure")

# in the order the refusals name them; of several set together, decode() lets the last one's record report, SurfaceFormer the
# first of SEQUENCE_MODEL_ORDER that is on (a record excludes every record before it in SEQUENCE_MODES, by its option's name)
SEQUENCE_MODES = (SEQUENCE_SAMPLE, SEQUENCE_BEAM, SEQUENCE_CONSTRAIN)
SEQUENCE_MODEL_ORDER = (SEQUENCE_BEAM, SEQUENCE_SAMPLE, SEQUENCE_CONSTRAIN)

MODES =(CONSTRAIN, SAMPLE, BEAM, GREEDY)      # in precedence order: of several mode options, the first one's record reports
SWITCH = {sw.attr: sw for mode in MODES for sw in mode.switches}


def of_options(logprob=False, constrain_beams=0, constrain_lookahead=False, constrain_exact=False, constrain_samples=0,
               constrain_beam_closure=None, **values):
    """(record, value) of the first of MODES whose option is set in `values` (constrain: the flag bits or None; num_samples;
    beam_width); else the greedy record (its logprob form with `logprob`) and None.  constrain with constrain_beams = W > 0:
    the CONSTRAIN_BEAM record and W; with constrain_samples = R > 0: the CONSTRAIN_SAMPLE record and R (whatever look-ahead is
    set: the record reads it); with constrain_lookahead: the CONSTRAIN_AHEAD record and the flag bits; with constrain_exact: the
    CONSTRAIN_EXACT record and the flag bits; with constrain_beams = W > 0 and constrain_beam_closure: the CONSTRAIN_BEAM_AHEAD
    record and W."""
    for mode in MODES[:-1]:
        v = values[mode.subject]
        if v is not None and (v or mode is CONSTRAIN):
            if mode is CONSTRAIN and constrain_beams:
                return (CONSTRAIN_BEAM_AHEAD if constrain_beam_closure else CONSTRAIN_BEAM), constrain_beams
            if mode is CONSTRAIN and constrain_samples:
                return CONSTRAIN_SAMPLE, constrain_samples
            if mode is CONSTRAIN and constrain_lookahead:
                return CONSTRAIN_AHEAD, v
            if mode is CONSTRAIN and constrain_exact:
                return CONSTRAIN_EXACT, v
            return mode, v
    return (GREEDY_LOGPROB if logprob else GREEDY), None
