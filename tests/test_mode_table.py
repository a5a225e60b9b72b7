"""Characterization of what the Python layers of the five decode modes reject, and with which words (CPU; nothing is launched).

EXPECTED holds the exception of every case below as the layers raised it BEFORE the mode table (faceformer_amd/hip/modes.py)
existed: the texts were recorded from that commit and are literals here, not computed from the table.  A case is one mode with
one offending option at one layer -- the check_*_options functions, PathEngine.decode / score, the two models, dist.decode_sharded,
main.run_test -- or several mode options set together, which pins the precedence (constrain, sample, beam, then greedy inside
decode() and SurfaceFormer_Parallel; the reverse in the lists that reject a mode outright).  The last tests check the table itself
against the binding, the signatures and the models' defaults."""
import inspect
import os
import sys
import types

import torch

from conftest import token_ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK = token_ns()
TERM = (1, 4)
PARALLEL, SEQ2SEQ = 0, 1      # FF_PARALLEL / FF_SEQ2SEQ (asserted below)


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on a device: decode() looks at retire's combinations after its operands' devices."""
    is_cuda = property(lambda self: True)


def _cb(counts):
    return False


# the offending value of every option a mode can exclude
BAD = dict(retire=True, return_pointer=True, no_stop=True, stop_callback=_cb, extra_mask=torch.zeros(8, 12, dtype=torch.uint8), logprob=True,
           beam_width=2, num_samples=2, stop_each_eos=True)


def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _par_inputs(**more):
    return dict({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                 "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}, **more)


def _seq_inputs():
    return {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool), "label": torch.zeros(1, 6, dtype=torch.long)}


def _cases():
    """[(id, thunk)]: every thunk must raise."""
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd import dist
    from faceformer_amd.hip import engine, lib
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    assert (lib.FF_PARALLEL, lib.FF_SEQ2SEQ) == (PARALLEL, SEQ2SEQ)
    cases = []

    def add(name, fn, *args, **kw):
        cases.append((name, lambda: fn(*args, **kw)))

    # ---- the check functions --------------------------------------------------------------------------------------------------
    table = torch.zeros(2, 8, 1, dtype=torch.int32)
    common = dict(variant=PARALLEL, retire=False, return_pointer=False, no_stop=False, stop_callback=None, extra_mask=None, logprob=False,
                  term_range=TERM)
    oks = {"beam": (engine.check_beam_options, dict(common, width=2, S=12)),
           "sample": (engine.check_sample_options, dict(common, num_samples=4, temperature=1.0, top_k=0, top_p=1.0, beam_width=0)),
           "constrain": (engine.check_constrain_options, dict(common, flags=3, beam_width=0, num_samples=0, follow_table=table))}
    values = {"beam": (dict(width=0), dict(width=9), dict(width=4, S=3)),
              "sample": (dict(num_samples=0), dict(num_samples=65), dict(temperature=-0.5), dict(top_k=-1), dict(top_p=0.0)),
              "constrain": (dict(follow_table=None), dict(flags=2, follow_table=None))}
    for mode, (fn, ok) in oks.items():
        fn(**ok)
        changes = [dict(variant=SEQ2SEQ), dict(term_range=None), dict(term_range=(4, 4)), dict(term_range=(1, 2, 3))]
        changes += [{k: BAD[k]} for k in ok if k in BAD and not (mode == "sample" and k == "num_samples")]
        for ch in changes + list(values[mode]):
            add("check_%s[%s]" % (mode, ",".join("%s=%s" % (k, "cb" if callable(v) else "mask" if torch.is_tensor(v) else v)
                                                 for k, v in ch.items())), fn, **dict(ok, **ch))
    paths, lengths = torch.zeros(3, 5, dtype=torch.int64), [4, 0, 2]
    engine.check_forced_options(paths, lengths, 3, 5, 12)
    for k in ("retire", "beam_width", "logprob", "return_pointer", "stop_callback", "stop_each_eos", "extra_mask"):
        add("check_forced[%s]" % k, engine.check_forced_options, paths, lengths, 3, 5, 12, **{k: BAD[k]})
    add("check_forced[paths int32]", engine.check_forced_options, paths.int(), lengths, 3, 5, 12)
    add("check_forced[paths shape]", engine.check_forced_options, paths[:2], lengths, 3, 5, 12)
    add("check_forced[lengths count]", engine.check_forced_options, paths, [4, 0], 3, 5, 12)
    add("check_forced[length 5]", engine.check_forced_options, paths, [5, 0, 2], 3, 5, 12)
    add("check_forced[token 12]", engine.check_forced_options, torch.tensor([[0, 1], [3, 12]]), [1, 1], 2, 2, 12)
    add("check_forced[token -1]", engine.check_forced_options, torch.tensor([[0, 1], [-1, 2]]), [1, 0], 2, 2, 12)
    for bad in ("loop", "", 4, -1, True, 1.0):
        add("constrain_flags[%r]" % (bad,), engine.constrain_flags, bad)

    # ---- PathEngine.decode / score on an engine object without a constructor call --------------------------------------------------
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng.num_token, eng.device = 4, torch.device("cpu")
    memory = torch.zeros(2, 12, 64)
    set_ = {"constrain": dict(constrain="loops", follow_table=table), "sample": dict(num_samples=2, uniforms=torch.zeros(4, 16)),
            "beam": dict(beam_width=2), "retire": dict(retire=True)}
    base = dict(T=5, F=4, num_input=[4, 3], term_range=TERM)
    excl = ("retire", "return_pointer", "no_stop", "stop_callback", "extra_mask", "logprob")
    for mode, on in set_.items():
        mem = memory if mode != "retire" else memory.as_subclass(_OnDevice)
        ok = dict(base, **on)
        for k in excl:
            if not (mode == "retire" and k in ("retire", "extra_mask", "logprob")):     # (retire takes an extra mask and logprob)
                add("decode[%s,%s]" % (mode, k), eng.decode, mem, None, None, PARALLEL, **dict(ok, **{k: BAD[k]}))
        add("decode[%s,seq2seq]" % mode, eng.decode, mem, None, None, SEQ2SEQ, **ok)
        add("decode[%s,term_range=None]" % mode, eng.decode, mem, None, None, PARALLEL, **dict(ok, term_range=None))
        add("decode[%s,term_range=(3,3)]" % mode, eng.decode, mem, None, None, PARALLEL, **dict(ok, term_range=(3, 3)))
    add("decode[retire,no num_input]", eng.decode, memory.as_subclass(_OnDevice), None, None, PARALLEL, **dict(base, retire=True, num_input=None))
    for name, more in (("beam+sample", ("beam", "sample")), ("beam+constrain", ("beam", "constrain")),
                       ("sample+constrain", ("sample", "constrain")), ("beam+sample+constrain", ("beam", "sample", "constrain"))):
        kw = dict(base)
        for m in more:
            kw.update(set_[m])
        add("decode[%s]" % name, eng.decode, memory, None, None, PARALLEL, **kw)
    add("decode[beam_width=9]", eng.decode, memory, None, None, PARALLEL, **dict(base, beam_width=9))
    add("decode[beam_width=7>S=6]", eng.decode, torch.zeros(2, 6, 64), None, None, PARALLEL, **dict(base, beam_width=7))
    add("decode[num_samples=65]", eng.decode, memory, None, None, PARALLEL, **dict(base, num_samples=65, uniforms=torch.zeros(4, 16)))
    add("decode[temperature=-1]", eng.decode, memory, None, None, PARALLEL, **dict(base, **set_["sample"], temperature=-1.0))
    add("decode[uniforms None]", eng.decode, memory, None, None, PARALLEL, **dict(base, num_samples=2))
    add("decode[uniforms shape]", eng.decode, memory, None, None, PARALLEL, **dict(base, num_samples=2, uniforms=torch.zeros(4, 15)))
    add("decode[constrain='both']", eng.decode, memory, None, None, PARALLEL, **dict(base, constrain="both"))
    add("decode[loops, no table]", eng.decode, memory, None, None, PARALLEL, **dict(base, constrain="loops"))
    add("decode[follow_table shape]", eng.decode, memory, None, None, PARALLEL, **dict(base, constrain="loops", follow_table=torch.zeros(2, 8, 2, dtype=torch.int32)))
    add("decode[follow_table dtype]", eng.decode, memory, None, None, PARALLEL, **dict(base, constrain=1, follow_table=torch.zeros(2, 8, 1)))
    dmem = memory.as_subclass(_OnDevice)
    for k in ("retire", "beam_width", "logprob", "return_pointer", "stop_callback", "stop_each_eos", "extra_mask"):
        add("score[%s]" % k, eng.score, dmem, None, None, PARALLEL, 5, torch.zeros(8, 5, dtype=torch.int64), [0] * 8, F=4, **{k: BAD[k]})
    for bit in ("FF_RETIRE_FINISHED", "FF_RETURN_POINTER", "FF_STOP_EACH_EOS"):
        add("score[flags %s]" % bit, eng.score, dmem, None, None, PARALLEL, 5, torch.zeros(8, 5, dtype=torch.int64), [0] * 8, F=4,
            flags=getattr(lib, bit))
    add("score[seq2seq F=4]", eng.score, dmem, None, None, SEQ2SEQ, 5, torch.zeros(8, 5, dtype=torch.int64), [0] * 8, F=4)
    add("score[paths shape]", eng.score, dmem, None, None, PARALLEL, 5, torch.zeros(7, 5, dtype=torch.int64), [0] * 8, F=4)

    # ---- the models -------------------------------------------------------------------------------------------------------------
    def forward(cls, attrs, inputs=None, ctor=None):
        model = _tiny_model(cls, **dict(dict(max_face_length=5) if cls is SurfaceFormer_Parallel else dict(label_seq_length=6), **(ctor or {})))
        for k, v in attrs.items():
            setattr(model, k, v)
        with torch.no_grad():
            model.forward_eval(inputs if inputs is not None else (_par_inputs() if cls is SurfaceFormer_Parallel else _seq_inputs()))

    def score(cls, attrs, ctor=None, **more):
        par = cls is SurfaceFormer_Parallel
        model = _tiny_model(cls, **dict(dict(max_face_length=5) if par else dict(label_seq_length=6), **(ctor or {})))
        for k, v in attrs.items():
            setattr(model, k, v)
        if par:
            model.score(_par_inputs(**more), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
        else:
            model.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))

    mset = {"constrain": dict(constrain="loops"), "sample": dict(num_samples=2), "beam": dict(beam_width=2), "retire": dict(retire_finished=True),
            "logprob": dict(return_logprob=True)}
    emask = torch.zeros(4, 8, dtype=torch.bool)
    for mode in ("constrain", "sample", "beam"):
        for other in mset:
            if other != mode:
                add("parallel[%s,%s]" % (mode, other), forward, SurfaceFormer_Parallel, dict(mset[mode], **mset[other]))
        add("parallel[%s,extra_mask]" % mode, forward, SurfaceFormer_Parallel, mset[mode], _par_inputs(extra_mask=emask))
        for cname, ctor in (("gelu", dict(activation="gelu")), ("post-norm", dict(normalize_before=False)), ("head 32", dict(num_head=2))):
            add("parallel[%s,%s]" % (mode, cname), forward, SurfaceFormer_Parallel, mset[mode], None, ctor)
    add("parallel[beam+sample+constrain]", forward, SurfaceFormer_Parallel, dict(beam_width=2, num_samples=2, constrain="no_repeat"))
    add("parallel[constrain='everything']", forward, SurfaceFormer_Parallel, dict(constrain="everything"))
    add("parallel[constrain=4]", forward, SurfaceFormer_Parallel, dict(constrain=4))
    add("parallel[num_samples=65]", forward, SurfaceFormer_Parallel, dict(num_samples=65))
    add("parallel[sample_temperature=-1]", forward, SurfaceFormer_Parallel, dict(num_samples=2, sample_temperature=-1.0))
    add("parallel[sample_top_p=0]", forward, SurfaceFormer_Parallel, dict(num_samples=2, sample_top_p=0.0))
    add("parallel[sample_top_k=-2]", forward, SurfaceFormer_Parallel, dict(num_samples=2, sample_top_k=-2))
    for name, attrs in mset.items():
        add("seq2seq[%s]" % name, forward, SurfaceFormer, attrs)
        add("parallel.score[%s]" % name, score, SurfaceFormer_Parallel, attrs)
        add("seq2seq.score[%s]" % name, score, SurfaceFormer, attrs)
    add("seq2seq[retire+sample+constrain]", forward, SurfaceFormer, dict(retire_finished=True, num_samples=2, constrain="loops"))
    add("seq2seq[sample+constrain]", forward, SurfaceFormer, dict(num_samples=2, constrain="loops"))
    add("parallel.score[sample+constrain]", score, SurfaceFormer_Parallel, dict(num_samples=2, constrain="loops"))
    add("parallel.score[extra_mask]", score, SurfaceFormer_Parallel, {}, extra_mask=emask)
    add("parallel.score[gelu]", score, SurfaceFormer_Parallel, {}, dict(activation="gelu"))
    add("parallel.score[gelu,sample]", score, SurfaceFormer_Parallel, dict(num_samples=2), dict(activation="gelu"))
    add("seq2seq.score[post-norm]", score, SurfaceFormer, {}, dict(normalize_before=False))

    # ---- dist.decode_sharded ------------------------------------------------------------------------------------------------------
    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    off = dict(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain=None)
    for name, attrs in list(mset.items()) + [("retire+logprob", dict(retire_finished=True, return_logprob=True)),
                                             ("logprob+beam", dict(return_logprob=True, beam_width=2)),
                                             ("beam+sample", dict(beam_width=2, num_samples=2)),
                                             ("beam+constrain", dict(beam_width=2, constrain="loops")),
                                             ("sample+constrain", dict(num_samples=2, constrain="loops")),
                                             ("none", {})]:
        add("sharded[%s]" % name, dist.decode_sharded, types.SimpleNamespace(**dict(off, **attrs)), {}, NoDist())
    add("sharded[no attributes]", dist.decode_sharded, types.SimpleNamespace(), {}, NoDist())

    # ---- main.run_test --------------------------------------------------------------------------------------------------------------
    flags = {"constrain": dict(constrain="loops"), "sample": dict(sample=2), "score_labels": dict(score_labels=True), "beam": dict(beam=2),
             "retire": dict(retire_finished=True), "scores": dict(scores=True)}
    world2 = types.SimpleNamespace(get_world_size=lambda: 2)
    world1 = types.SimpleNamespace(get_world_size=lambda: 1, get_rank=lambda: (_ for _ in ()).throw(AssertionError("passed the flag checks")))

    def run(model_class="SurfaceFormer_Parallel", dist_mod=None, **kw):
        class Cfg:                                                       # anything past the flag checks asks for cfg.dataset_class
            def __getattr__(self, name):
                raise AssertionError("passed the flag checks: cfg." + name)
        cfg = Cfg()
        cfg.__dict__["model_class"] = model_class
        cli.run_test(cfg, None, out_dir="unused", device="cpu", model=object(), dist_mod=dist_mod, **kw)

    names = list(flags)
    for i, a in enumerate(names):
        add("cli[%s,SurfaceFormer]" % a, run, "SurfaceFormer", **flags[a])
        add("cli[%s,2 ranks]" % a, run, dist_mod=world2, **flags[a])
        add("cli[%s,1 rank]" % a, run, dist_mod=world1, **flags[a])
        for b in names[i + 1:]:
            add("cli[%s,%s]" % (a, b), run, **dict(flags[a], **flags[b]))
    add("cli[constrain='closed']", run, constrain="closed")
    add("cli[constrain,sample,beam]", run, constrain="loops", sample=2, beam=2)
    add("cli[all six,SurfaceFormer,2 ranks]", run, "SurfaceFormer", world2, **{k: v for f in flags.values() for k, v in f.items()})
    return cases


def _outcome(thunk):
    try:
        thunk()
    except Exception as e:       # the type and the text, byte for byte
        return "%s: %s" % (type(e).__name__, e)
    return "no exception"


def _untouchable(monkeypatch):
    from faceformer_amd.hip import lib
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("library touched")))


# what every case of _cases() raised before the mode table existed: ("Type: text", the cases that raise it)
RECORDED = [
    ('ValueError: beam_width is a parallel-variant option', (
      'check_beam[variant=1]', 'decode[beam,seq2seq]',)),
    ('ValueError: beam_width needs term_range = (lo, hi) with lo < hi', (
      'check_beam[term_range=None]', 'check_beam[term_range=(4, 4)]', 'check_beam[term_range=(1, 2, 3)]',
      'decode[beam,term_range=None]', 'decode[beam,term_range=(3,3)]',)),
    ('ValueError: beam_width excludes retire, return_pointer, no_stop, stop_callback, extra_mask and logprob', (
      'check_beam[retire=True]', 'check_beam[return_pointer=True]', 'check_beam[no_stop=True]',
      'check_beam[stop_callback=cb]', 'check_beam[extra_mask=mask]', 'check_beam[logprob=True]', 'decode[beam,retire]',
      'decode[beam,return_pointer]', 'decode[beam,no_stop]', 'decode[beam,stop_callback]', 'decode[beam,extra_mask]',
      'decode[beam,logprob]',)),
    ('ValueError: beam_width=0: must be in 1..8 and at most S = 12', (
      'check_beam[width=0]',)),
    ('ValueError: beam_width=9: must be in 1..8 and at most S = 12', (
      'check_beam[width=9]', 'decode[beam_width=9]',)),
    ('ValueError: beam_width=4: must be in 1..8 and at most S = 3', (
      'check_beam[width=4,S=3]',)),
    ('ValueError: num_samples is a parallel-variant option', (
      'check_sample[variant=1]', 'decode[sample,seq2seq]',)),
    ('ValueError: num_samples needs term_range = (lo, hi) with lo < hi', (
      'check_sample[term_range=None]', 'check_sample[term_range=(4, 4)]', 'check_sample[term_range=(1, 2, 3)]',
      'decode[sample,term_range=None]', 'decode[sample,term_range=(3,3)]',)),
    ('ValueError: num_samples excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob and beam_width', (
      'check_sample[retire=True]', 'check_sample[return_pointer=True]', 'check_sample[no_stop=True]',
      'check_sample[stop_callback=cb]', 'check_sample[extra_mask=mask]', 'check_sample[logprob=True]',
      'check_sample[beam_width=2]', 'decode[sample,retire]', 'decode[sample,return_pointer]', 'decode[sample,no_stop]',
      'decode[sample,stop_callback]', 'decode[sample,extra_mask]', 'decode[sample,logprob]', 'decode[beam+sample]',)),
    ('ValueError: num_samples=0: must be in 1..64', (
      'check_sample[num_samples=0]',)),
    ('ValueError: num_samples=65: must be in 1..64', (
      'check_sample[num_samples=65]', 'decode[num_samples=65]', 'parallel[num_samples=65]',)),
    ('ValueError: sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]: got -0.5, 0, 1.0', (
      'check_sample[temperature=-0.5]',)),
    ('ValueError: sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]: got 1.0, -1, 1.0', (
      'check_sample[top_k=-1]',)),
    ('ValueError: sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]: got 1.0, 0, 0.0', (
      'check_sample[top_p=0.0]', 'parallel[sample_top_p=0]',)),
    ('ValueError: constrain is a parallel-variant option', (
      'check_constrain[variant=1]', 'decode[constrain,seq2seq]',)),
    ('ValueError: constrain needs term_range = (lo, hi) with lo < hi', (
      'check_constrain[term_range=None]', 'check_constrain[term_range=(4, 4)]', 'check_constrain[term_range=(1, 2, 3)]',
      'decode[constrain,term_range=None]', 'decode[constrain,term_range=(3,3)]',)),
    ('ValueError: constrain excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width and num_samples', (
      'check_constrain[retire=True]', 'check_constrain[return_pointer=True]', 'check_constrain[no_stop=True]',
      'check_constrain[stop_callback=cb]', 'check_constrain[extra_mask=mask]', 'check_constrain[logprob=True]',
      'check_constrain[beam_width=2]', 'check_constrain[num_samples=2]', 'decode[constrain,retire]',
      'decode[constrain,return_pointer]', 'decode[constrain,no_stop]', 'decode[constrain,stop_callback]',
      'decode[constrain,extra_mask]', 'decode[constrain,logprob]', 'decode[beam+constrain]', 'decode[sample+constrain]',
      'decode[beam+sample+constrain]',)),
    ("ValueError: constrain='loops' needs follow_table (ops.follow_table)", (
      'check_constrain[follow_table=None]', 'check_constrain[flags=2,follow_table=None]', 'decode[loops, no table]',)),
    ('ValueError: scoring given paths excludes retire, beam_width, logprob, return_pointer, stop_callback, stop_each_eos and extra_mask', (
      'check_forced[retire]', 'check_forced[beam_width]', 'check_forced[logprob]', 'check_forced[return_pointer]',
      'check_forced[stop_callback]', 'check_forced[stop_each_eos]', 'check_forced[extra_mask]', 'score[retire]',
      'score[beam_width]', 'score[logprob]', 'score[return_pointer]', 'score[stop_callback]', 'score[stop_each_eos]',
      'score[extra_mask]',)),
    ('ValueError: paths must be an int64 tensor of shape [3, 5]', (
      'check_forced[paths int32]', 'check_forced[paths shape]',)),
    ('ValueError: lengths must hold 3 values in 0..4', (
      'check_forced[lengths count]', 'check_forced[length 5]',)),
    ('ValueError: paths[1, 1] = 12 lies outside [0, 12)', (
      'check_forced[token 12]',)),
    ('ValueError: paths[1, 0] = -1 lies outside [0, 12)', (
      'check_forced[token -1]',)),
    ("ValueError: constrain='loop': must be None, 'no_repeat' or 'loops'", (
      "constrain_flags['loop']",)),
    ("ValueError: constrain='': must be None, 'no_repeat' or 'loops'", (
      "constrain_flags['']",)),
    ("ValueError: constrain=4: must be None, 'no_repeat', 'loops' or flag bits 0..3", (
      'constrain_flags[4]', 'parallel[constrain=4]',)),
    ("ValueError: constrain=-1: must be None, 'no_repeat', 'loops' or flag bits 0..3", (
      'constrain_flags[-1]',)),
    ("ValueError: constrain=True: must be None, 'no_repeat', 'loops' or flag bits 0..3", (
      'constrain_flags[True]',)),
    ("ValueError: constrain=1.0: must be None, 'no_repeat', 'loops' or flag bits 0..3", (
      'constrain_flags[1.0]',)),
    ('ValueError: retire=True excludes return_pointer, no_stop and stop_callback', (
      'decode[retire,return_pointer]', 'decode[retire,no_stop]', 'decode[retire,stop_callback]',)),
    ('ValueError: retire=True is a parallel-variant option', (
      'decode[retire,seq2seq]',)),
    ('ValueError: retire=True needs term_range = (lo, hi) with lo < hi', (
      'decode[retire,term_range=None]', 'decode[retire,term_range=(3,3)]',)),
    ('ValueError: retire=True needs num_input', (
      'decode[retire,no num_input]',)),
    ('ValueError: beam_width=7: must be in 1..8 and at most S = 6', (
      'decode[beam_width=7>S=6]',)),
    ('ValueError: sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]: got -1.0, 0, 1.0', (
      'decode[temperature=-1]', 'parallel[sample_temperature=-1]',)),
    ('ValueError: uniforms must be a float32 tensor of shape [4, 16]', (
      'decode[uniforms None]', 'decode[uniforms shape]',)),
    ("ValueError: constrain='both': must be None, 'no_repeat' or 'loops'", (
      "decode[constrain='both']",)),
    ('ValueError: follow_table must be an int32 tensor of shape [2, 8, 1]', (
      'decode[follow_table shape]', 'decode[follow_table dtype]',)),
    ('ValueError: scoring given paths excludes the flag FF_RETIRE_FINISHED', (
      'score[flags FF_RETIRE_FINISHED]',)),
    ('ValueError: scoring given paths excludes the flag FF_RETURN_POINTER', (
      'score[flags FF_RETURN_POINTER]',)),
    ('ValueError: scoring given paths excludes the flag FF_STOP_EACH_EOS', (
      'score[flags FF_STOP_EACH_EOS]',)),
    ('ValueError: the seq2seq variant scores one row per wireframe (F = 1)', (
      'score[seq2seq F=4]',)),
    ('ValueError: paths must be an int64 tensor of shape [8, 5]', (
      'score[paths shape]',)),
    ('ValueError: constrain excludes beam_width, num_samples, retire_finished, return_logprob and an extra mask', (
      'parallel[constrain,sample]', 'parallel[constrain,beam]', 'parallel[constrain,retire]', 'parallel[constrain,logprob]',
      'parallel[constrain,extra_mask]', 'parallel[sample,constrain]', 'parallel[beam,constrain]',
      'parallel[beam+sample+constrain]',)),
    ("ValueError: constrain needs the native engine: this model's constructor arguments take the sub-module loop", (
      'parallel[constrain,gelu]', 'parallel[constrain,post-norm]', 'parallel[constrain,head 32]',)),
    ('ValueError: num_samples excludes beam_width, retire_finished, return_logprob and an extra mask', (
      'parallel[sample,beam]', 'parallel[sample,retire]', 'parallel[sample,logprob]', 'parallel[sample,extra_mask]',
      'parallel[beam,sample]',)),
    ("ValueError: num_samples needs the native engine: this model's constructor arguments take the sub-module loop", (
      'parallel[sample,gelu]', 'parallel[sample,post-norm]', 'parallel[sample,head 32]',)),
    ('HipExtensionError: model parameters are on cpu: the faceformer_amd decode path runs only on a ROCm device through libfaceformer_hip.so (no CPU fallback). Move the model with .cuda().', (
      'parallel[beam,retire]', 'parallel[beam,logprob]', 'parallel[beam,extra_mask]', 'seq2seq[beam]',
      'parallel.score[beam]', 'seq2seq.score[beam]', 'parallel.score[retire]', 'seq2seq.score[retire]', 'seq2seq[logprob]',
      'parallel.score[logprob]', 'seq2seq.score[logprob]', 'parallel.score[extra_mask]',)),
    ("ValueError: beam_width needs the native engine: this model's constructor arguments take the sub-module loop", (
      'parallel[beam,gelu]', 'parallel[beam,post-norm]', 'parallel[beam,head 32]',)),
    ("ValueError: constrain='everything': must be None, 'no_repeat' or 'loops'", (
      "parallel[constrain='everything']",)),
    ('ValueError: sampling needs a finite temperature >= 0, top_k >= 0 and top_p in (0, 1]: got 1.0, -2, 1.0', (
      'parallel[sample_top_k=-2]',)),
    ('ValueError: constrain is a SurfaceFormer_Parallel option (the single-sequence model emits loops of plain edges)', (
      'seq2seq[constrain]',)),
    ('ValueError: score() excludes constrain: set model.constrain = None to score given paths', (
      'parallel.score[constrain]', 'seq2seq.score[constrain]',)),
    ('ValueError: num_samples is a SurfaceFormer_Parallel option (sampling for the single-sequence model is not implemented)', (
      'seq2seq[sample]', 'seq2seq[sample+constrain]',)),
    ('ValueError: score() excludes num_samples: set model.num_samples = 0 to score given paths', (
      'parallel.score[sample]', 'seq2seq.score[sample]', 'parallel.score[sample+constrain]', 'parallel.score[gelu,sample]',)),
    ('ValueError: retire_finished is a SurfaceFormer_Parallel option (the single-sequence model has one sequence per wireframe)', (
      'seq2seq[retire]', 'seq2seq[retire+sample+constrain]',)),
    ("ValueError: score() needs the native engine: this model's constructor arguments take the sub-module loop", (
      'parallel.score[gelu]', 'seq2seq.score[post-norm]',)),
    ('ValueError: decode_sharded does not implement constrain (a constrained decode takes no external stop rule)', (
      'sharded[constrain]',)),
    ('ValueError: decode_sharded does not implement num_samples (a sampled decode takes no external stop rule)', (
      'sharded[sample]', 'sharded[sample+constrain]',)),
    ('ValueError: decode_sharded does not implement beam_width (a beam decode takes no external stop rule)', (
      'sharded[beam]', 'sharded[beam+sample]', 'sharded[beam+constrain]',)),
    ('ValueError: decode_sharded does not implement retire_finished (the batch-global stop rule counts every sequence)', (
      'sharded[retire]', 'sharded[retire+logprob]',)),
    ('ValueError: decode_sharded does not implement return_logprob (the log-probabilities are not gathered across ranks)', (
      'sharded[logprob]', 'sharded[logprob+beam]',)),
    ('AssertionError: process group touched: get_rank', (
      'sharded[none]', 'sharded[no attributes]',)),
    ('ValueError: --constrain applies to SurfaceFormer_Parallel only, and not together with --retire-finished, --scores, --beam, --sample or --score-labels', (
      'cli[constrain,SurfaceFormer]', 'cli[constrain,sample]', 'cli[constrain,score_labels]', 'cli[constrain,beam]',
      'cli[constrain,retire]', 'cli[constrain,scores]', 'cli[constrain,sample,beam]', 'cli[all six,SurfaceFormer,2 ranks]',)),
    ('ValueError: --constrain is not implemented for multi-rank runs', (
      'cli[constrain,2 ranks]',)),
    ('AssertionError: passed the flag checks: cfg.dataset_class', (
      'cli[constrain,1 rank]', 'cli[sample,1 rank]', 'cli[score_labels,SurfaceFormer]', 'cli[score_labels,1 rank]',
      'cli[beam,1 rank]', 'cli[retire,2 ranks]', 'cli[retire,1 rank]', 'cli[retire,scores]', 'cli[scores,SurfaceFormer]',
      'cli[scores,1 rank]',)),
    ('ValueError: --sample applies to SurfaceFormer_Parallel only, and not together with --retire-finished, --scores, --beam or --score-labels', (
      'cli[sample,SurfaceFormer]', 'cli[sample,score_labels]', 'cli[sample,beam]', 'cli[sample,retire]',
      'cli[sample,scores]',)),
    ('ValueError: --sample (num_samples) is not implemented for multi-rank runs', (
      'cli[sample,2 ranks]',)),
    ('ValueError: --score-labels (score) is not implemented for multi-rank runs: the scores are not gathered across ranks', (
      'cli[score_labels,2 ranks]',)),
    ('ValueError: --score-labels does not combine with --retire-finished, --scores or --beam (a forced decode excludes them)', (
      'cli[score_labels,beam]', 'cli[score_labels,retire]', 'cli[score_labels,scores]',)),
    ('ValueError: --beam applies to SurfaceFormer_Parallel only, and not together with --retire-finished or --scores', (
      'cli[beam,SurfaceFormer]', 'cli[beam,retire]', 'cli[beam,scores]',)),
    ('ValueError: --beam (beam_width) is not implemented for multi-rank runs', (
      'cli[beam,2 ranks]',)),
    ('ValueError: --retire-finished applies to SurfaceFormer_Parallel only', (
      'cli[retire,SurfaceFormer]',)),
    ('ValueError: --scores (return_logprob) is not implemented for multi-rank runs: the log-probabilities are not gathered across ranks', (
      'cli[scores,2 ranks]',)),
    ("ValueError: --constrain must be 'no_repeat' or 'loops'", (
      "cli[constrain='closed']",)),
]


def test_every_rejection_has_the_recorded_type_and_text(monkeypatch):
    _untouchable(monkeypatch)
    expected = {name: text for text, names in RECORDED for name in names}
    cases = _cases()
    assert sorted(name for name, _ in cases) == sorted(expected) and len(expected) == sum(len(names) for _, names in RECORDED)
    got = {name: _outcome(thunk) for name, thunk in cases}
    wrong = ["%s\n  raised   %s\n  recorded %s" % (name, got[name], expected[name]) for name, _ in cases if got[name] != expected[name]]
    assert not wrong, "\n".join(wrong)


# ---- the table itself ---------------------------------------------------------------------------------------------------------------
def _records():
    from faceformer_amd.hip import modes
    assert modes.MODES == (modes.CONSTRAIN, modes.SAMPLE, modes.BEAM, modes.GREEDY)
    return modes.MODES + (modes.GREEDY_LOGPROB, modes.FORCED)


def test_every_entry_of_the_table_is_bound_with_its_size_query():
    from faceformer_amd.hip import lib
    entries = [m.entry for m in _records()]
    assert sorted(entries) == ["ff_decode", "ff_decode_beam", "ff_decode_constrained", "ff_decode_forced", "ff_decode_lp", "ff_decode_sample"]
    for name in entries:
        assert name in lib.SIGNATURES and name + "_workspace_bytes" in lib.SIGNATURES, name
    for m in _records():       # the size query takes G where the record says so, and only there
        assert len(lib.SIGNATURES[m.entry + "_workspace_bytes"][1]) == (2 if m.entry == "ff_decode_forced" else 3) + bool(m.per_anchor)


def test_every_excluded_name_is_a_parameter_of_decode_or_score():
    from faceformer_amd.hip import engine, modes
    decode = set(inspect.signature(engine.PathEngine.decode).parameters)
    score = set(inspect.signature(engine.PathEngine.score).parameters)
    for m in _records():
        params = score if m is modes.FORCED else decode
        assert m.excludes and set(m.excludes) <= params, m.subject
        assert len(set(m.excludes)) == len(m.excludes)
        if m.per_anchor:
            assert m.subject in decode
    for m in modes.MODES[:3]:      # a mode excludes every mode after it in the precedence order, by its option's name
        later = [n.subject for n in modes.MODES[modes.MODES.index(m) + 1:3]]
        assert sorted(k for k in m.excludes if k in ("constrain", "num_samples", "beam_width")) == sorted(later)


def test_every_model_attribute_of_the_table_exists_with_its_off_value_on_a_fresh_model():
    from faceformer_amd.hip import modes
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    switches = [sw for m in modes.MODES for sw in m.switches]
    assert [sw.attr for sw in switches] == ["constrain", "num_samples", "beam_width", "retire_finished", "return_logprob"]
    assert modes.SWITCH == {sw.attr: sw for sw in switches}
    for model in (_tiny_model(SurfaceFormer_Parallel, max_face_length=5), _tiny_model(SurfaceFormer, label_seq_length=6)):
        for sw in switches:
            assert hasattr(model, sw.attr) and getattr(model, sw.attr) == sw.off and type(getattr(model, sw.attr)) is type(sw.off)
            assert not sw.on(model)
    for m in modes.MODES:
        assert set(m.model_excludes) <= set(modes.SWITCH) | {"an extra mask"}
