"""The three single-sequence decode modes (sequence_samples, sequence_beams, sequence_constrain; faceformer_amd/hip/modes.py:
SEQUENCE_MODES) as one table: what every layer refuses and with which words, the table against the binding and the models, and
forward_eval against a direct PathEngine.decode call.

RECORDED holds the exception of every case of _cases() as the layers raised it BEFORE SEQUENCE_MODES existed, when every layer
had one hand-written block per option: the texts were recorded from that commit and are literals here, not computed from the
table.  A case is one option, or two of them set together, with one thing its record excludes, at one layer: PathEngine.decode,
SurfaceFormer.forward_eval, SurfaceFormer_Parallel.forward_eval, both models' score(), dist.decode_sharded.  With two options set
the text also pins which record reports: constrain, beams, samples inside decode(); beams, samples, constrain in SurfaceFormer;
samples, beams, constrain where the option is refused outright (SurfaceFormer_Parallel, score(), decode_sharded).  Every one is
raised before the library is loaded (CPU; nothing is launched)."""
import inspect
import itertools
import types

import pytest
import torch

from conftest import token_ns

TOK = token_ns()
PARALLEL, SEQ2SEQ = 0, 1      # FF_PARALLEL / FF_SEQ2SEQ (asserted below)
OPTIONS = ("sequence_samples", "sequence_beams", "sequence_constrain")
SHORT = {"sequence_samples": "samples", "sequence_beams": "beams", "sequence_constrain": "constrain"}
COMBOS = [(o,) for o in OPTIONS] + list(itertools.combinations(OPTIONS, 2))


def _cb(counts):
    return False


def _tiny_model(cls, **ctor):
    kw = dict(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1, num_lines=8, token=TOK)
    kw.update(ctor)
    return cls(**kw).eval()


def _par_inputs(**more):
    return dict({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                 "label": torch.zeros(1, 4, 4, dtype=torch.long), "num_input": [4]}, **more)


def _seq_inputs(**more):
    return dict({"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
                 "label": torch.zeros(1, 6, dtype=torch.long)}, **more)


def _cases():
    """[(id, thunk)]: every thunk must raise."""
    from faceformer_amd import dist
    from faceformer_amd.hip import engine, lib
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    assert (lib.FF_PARALLEL, lib.FF_SEQ2SEQ) == (PARALLEL, SEQ2SEQ)
    cases = []

    def add(name, fn, *args, **kw):
        cases.append((name, lambda: fn(*args, **kw)))

    # ---- PathEngine.decode on an engine object without a constructor call -------------------------------------------------------
    eng = engine.PathEngine.__new__(engine.PathEngine)
    eng._planes, eng.num_token, eng.device = {}, 4, torch.device("cpu")
    memory = torch.zeros(2, 12, 64)
    on = {"sequence_samples": dict(sequence_samples=3, uniforms=torch.zeros(4, 6)), "sequence_beams": dict(sequence_beams=3),
          "sequence_constrain": dict(sequence_constrain="loops", tok_sep=2, follow_table=torch.zeros(2, 8, 1, dtype=torch.int32))}
    bad = [("retire", dict(retire=True)), ("return_pointer", dict(return_pointer=True)), ("no_stop", dict(no_stop=True)),
           ("stop_callback", dict(stop_callback=_cb)), ("extra_mask", dict(extra_mask=torch.zeros(2, 12, dtype=torch.uint8))),
           ("logprob", dict(logprob=True)), ("beam_width", dict(beam_width=2)), ("num_samples", dict(num_samples=2)),
           ("constrain", dict(constrain="no_repeat")), ("constrain=0", dict(constrain=0)),
           ("FF_STOP_EACH_EOS", dict(flags=engine.DEFAULT_FLAGS | lib.FF_STOP_EACH_EOS))]
    for combo in COMBOS:
        tag = "+".join(SHORT[o] for o in combo)
        ok = dict(T=5, F=1)
        for o in combo:
            ok.update(on[o])
        for name, change in bad:
            add("decode[%s,%s]" % (tag, name), eng.decode, memory, None, None, SEQ2SEQ, **dict(ok, **change))
        add("decode[%s,parallel F=4]" % tag, eng.decode, memory, None, None, PARALLEL, **dict(ok, F=4, num_input=[4, 3]))
        add("decode[%s,seq2seq F=4]" % tag, eng.decode, memory, None, None, SEQ2SEQ, **dict(ok, F=4))
        if len(combo) == 2:
            add("decode[%s]" % tag, eng.decode, memory, None, None, SEQ2SEQ, **ok)

    # ---- the models -------------------------------------------------------------------------------------------------------------
    def forward(cls, attrs, inputs=None, ctor=None):
        model = _tiny_model(cls, **dict(dict(max_face_length=5) if cls is SurfaceFormer_Parallel else dict(label_seq_length=6), **(ctor or {})))
        for k, v in attrs.items():
            setattr(model, k, v)
        with torch.no_grad():
            model.forward_eval(inputs if inputs is not None else (_par_inputs() if cls is SurfaceFormer_Parallel else _seq_inputs()))

    def score(cls, attrs):
        par = cls is SurfaceFormer_Parallel
        model = _tiny_model(cls, **(dict(max_face_length=5) if par else dict(label_seq_length=6)))
        for k, v in attrs.items():
            setattr(model, k, v)
        if par:
            model.score(_par_inputs(), torch.zeros(1, 4, 5, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long))
        else:
            model.score(_seq_inputs(), torch.zeros(1, 6, dtype=torch.long), torch.zeros(1, dtype=torch.long))

    mon = {"sequence_samples": dict(sequence_samples=3), "sequence_beams": dict(sequence_beams=3),
           "sequence_constrain": dict(sequence_constrain="loops")}
    mbad = [("retire_finished", dict(retire_finished=True)), ("return_logprob", dict(return_logprob=True)), ("beam_width", dict(beam_width=2)),
            ("num_samples", dict(num_samples=2)), ("constrain", dict(constrain="loops")), ("constrain=0", dict(constrain=0)),
            ("stop_each_eos", dict(stop_each_eos=True))]
    for combo in COMBOS:
        tag = "+".join(SHORT[o] for o in combo)
        attrs = {}
        for o in combo:
            attrs.update(mon[o])
        for name, change in mbad:
            add("seq2seq[%s,%s]" % (tag, name), forward, SurfaceFormer, dict(attrs, **change))
        add("seq2seq[%s,extra_mask]" % tag, forward, SurfaceFormer, attrs, _seq_inputs(extra_mask=torch.zeros(1, 8, dtype=torch.bool)))
        add("seq2seq[%s,gelu]" % tag, forward, SurfaceFormer, attrs, None, dict(activation="gelu"))
        add("seq2seq[%s]" % tag, forward, SurfaceFormer, attrs)      # (one option alone is not refused: the encoder asks for a device)
        add("parallel[%s]" % tag, forward, SurfaceFormer_Parallel, attrs)
        add("parallel.score[%s]" % tag, score, SurfaceFormer_Parallel, attrs)
        add("seq2seq.score[%s]" % tag, score, SurfaceFormer, attrs)
    add("seq2seq[constrain=0,samples]", forward, SurfaceFormer, dict(sequence_constrain=0, sequence_samples=3))
    add("parallel[constrain=0]", forward, SurfaceFormer_Parallel, dict(sequence_constrain=0))
    add("seq2seq.score[constrain=0]", score, SurfaceFormer, dict(sequence_constrain=0))
    for name, change in mbad[:6]:      # the parallel model's own modes do not hide the refusal, nor does score()'s table
        add("parallel[samples,%s]" % name, forward, SurfaceFormer_Parallel, dict(mon["sequence_samples"], **change))
        add("parallel.score[constrain,%s]" % name, score, SurfaceFormer_Parallel, dict(mon["sequence_constrain"], **change))

    # ---- dist.decode_sharded ------------------------------------------------------------------------------------------------------
    class NoDist:
        def __getattr__(self, name):
            raise AssertionError("process group touched: " + name)
    off = dict(retire_finished=False, return_logprob=False, beam_width=0, num_samples=0, constrain=None)
    for combo in COMBOS:
        tag = "+".join(SHORT[o] for o in combo)
        attrs = {}
        for o in combo:
            attrs.update(mon[o])
        add("sharded[%s]" % tag, dist.decode_sharded, types.SimpleNamespace(**dict(off, **attrs)), {}, NoDist())
        for name, change in mbad[:6] + [("sequence_faces", dict(sequence_faces="parse")), ("constrain_lookahead", dict(constrain_lookahead=True)),
                                        ("constrain_samples", dict(constrain_samples=2)), ("constrain_beams", dict(constrain_beams=2))]:
            add("sharded[%s,%s]" % (tag, name), dist.decode_sharded, types.SimpleNamespace(**dict(off, **dict(attrs, **change))), {}, NoDist())
    add("sharded[constrain=0]", dist.decode_sharded, types.SimpleNamespace(**dict(off, sequence_constrain=0)), {}, NoDist())
    add("sharded[all off]", dist.decode_sharded, types.SimpleNamespace(**dict(off, sequence_samples=0, sequence_beams=0, sequence_constrain=None)),
        {}, NoDist())
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


# what every case of _cases() raised before SEQUENCE_MODES existed: ("Type: text", the cases that raise it)
RECORDED = [
    ('ValueError: sequence_samples excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width, num_samples and constrain', (
      'decode[samples,retire]', 'decode[samples,return_pointer]', 'decode[samples,no_stop]', 'decode[samples,stop_callback]',
      'decode[samples,extra_mask]', 'decode[samples,logprob]', 'decode[samples,beam_width]', 'decode[samples,num_samples]',
      'decode[samples,constrain]', 'decode[samples,constrain=0]',)),
    ('ValueError: sequence_samples excludes stop_each_eos (FF_STOP_EACH_EOS): every draw is finished by its own EOS already', (
      'decode[samples,FF_STOP_EACH_EOS]',)),
    ('ValueError: sequence_samples is a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant draws with num_samples', (
      'decode[samples,parallel F=4]', 'decode[samples,seq2seq F=4]',)),
    ('ValueError: sequence_beams excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width, num_samples, constrain and sequence_samples', (
      'decode[beams,retire]', 'decode[beams,return_pointer]', 'decode[beams,no_stop]', 'decode[beams,stop_callback]',
      'decode[beams,extra_mask]', 'decode[beams,logprob]', 'decode[beams,beam_width]', 'decode[beams,num_samples]',
      'decode[beams,constrain]', 'decode[beams,constrain=0]', 'decode[samples+beams,retire]',
      'decode[samples+beams,return_pointer]', 'decode[samples+beams,no_stop]', 'decode[samples+beams,stop_callback]',
      'decode[samples+beams,extra_mask]', 'decode[samples+beams,logprob]', 'decode[samples+beams,beam_width]',
      'decode[samples+beams,num_samples]', 'decode[samples+beams,constrain]', 'decode[samples+beams,constrain=0]',
      'decode[samples+beams,FF_STOP_EACH_EOS]', 'decode[samples+beams]',)),
    ('ValueError: sequence_beams excludes stop_each_eos (FF_STOP_EACH_EOS): every beam is finished by its own EOS already', (
      'decode[beams,FF_STOP_EACH_EOS]',)),
    ('ValueError: sequence_beams is a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant searches with beam_width', (
      'decode[beams,parallel F=4]', 'decode[beams,seq2seq F=4]', 'decode[samples+beams,parallel F=4]',
      'decode[samples+beams,seq2seq F=4]',)),
    ('ValueError: sequence_constrain excludes retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width, num_samples, constrain, sequence_samples and sequence_beams', (
      'decode[constrain,retire]', 'decode[constrain,return_pointer]', 'decode[constrain,no_stop]',
      'decode[constrain,stop_callback]', 'decode[constrain,extra_mask]', 'decode[constrain,logprob]',
      'decode[constrain,beam_width]', 'decode[constrain,num_samples]', 'decode[constrain,constrain]',
      'decode[constrain,constrain=0]', 'decode[samples+constrain,retire]', 'decode[samples+constrain,return_pointer]',
      'decode[samples+constrain,no_stop]', 'decode[samples+constrain,stop_callback]', 'decode[samples+constrain,extra_mask]',
      'decode[samples+constrain,logprob]', 'decode[samples+constrain,beam_width]', 'decode[samples+constrain,num_samples]',
      'decode[samples+constrain,constrain]', 'decode[samples+constrain,constrain=0]',
      'decode[samples+constrain,FF_STOP_EACH_EOS]', 'decode[samples+constrain]', 'decode[beams+constrain,retire]',
      'decode[beams+constrain,return_pointer]', 'decode[beams+constrain,no_stop]', 'decode[beams+constrain,stop_callback]',
      'decode[beams+constrain,extra_mask]', 'decode[beams+constrain,logprob]', 'decode[beams+constrain,beam_width]',
      'decode[beams+constrain,num_samples]', 'decode[beams+constrain,constrain]', 'decode[beams+constrain,constrain=0]',
      'decode[beams+constrain,FF_STOP_EACH_EOS]', 'decode[beams+constrain]',)),
    ('ValueError: sequence_constrain excludes stop_each_eos (FF_STOP_EACH_EOS): every row is finished by its own EOS already', (
      'decode[constrain,FF_STOP_EACH_EOS]',)),
    ('ValueError: sequence_constrain is a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant constrains with constrain', (
      'decode[constrain,parallel F=4]', 'decode[constrain,seq2seq F=4]', 'decode[samples+constrain,parallel F=4]',
      'decode[samples+constrain,seq2seq F=4]', 'decode[beams+constrain,parallel F=4]', 'decode[beams+constrain,seq2seq F=4]',)),
    ('ValueError: retire_finished is a SurfaceFormer_Parallel option (the single-sequence model has one sequence per wireframe)', (
      'seq2seq[samples,retire_finished]', 'seq2seq[beams,retire_finished]', 'seq2seq[constrain,retire_finished]',
      'seq2seq[samples+beams,retire_finished]', 'seq2seq[samples+constrain,retire_finished]',
      'seq2seq[beams+constrain,retire_finished]',)),
    ('ValueError: sequence_samples excludes return_logprob and an extra mask', (
      'seq2seq[samples,return_logprob]', 'seq2seq[samples,extra_mask]', 'seq2seq[samples+constrain,return_logprob]',
      'seq2seq[samples+constrain,extra_mask]',)),
    ('HipExtensionError: model parameters are on cpu: the faceformer_amd decode path runs only on a ROCm device through libfaceformer_hip.so (no CPU fallback). Move the model with .cuda().', (
      'seq2seq[samples,beam_width]', 'seq2seq[samples,stop_each_eos]', 'seq2seq[samples]', 'seq2seq[beams,stop_each_eos]',
      'seq2seq[beams]', 'seq2seq[constrain,beam_width]', 'seq2seq[constrain]',)),
    ('ValueError: num_samples is a SurfaceFormer_Parallel option (sampling for the single-sequence model is not implemented)', (
      'seq2seq[samples,num_samples]', 'seq2seq[beams,num_samples]', 'seq2seq[constrain,num_samples]',
      'seq2seq[samples+beams,num_samples]', 'seq2seq[samples+constrain,num_samples]', 'seq2seq[beams+constrain,num_samples]',)),
    ('ValueError: constrain is a SurfaceFormer_Parallel option (the single-sequence model emits loops of plain edges)', (
      'seq2seq[samples,constrain]', 'seq2seq[samples,constrain=0]', 'seq2seq[beams,constrain]', 'seq2seq[beams,constrain=0]',
      'seq2seq[constrain,constrain]', 'seq2seq[constrain,constrain=0]', 'seq2seq[samples+beams,constrain]',
      'seq2seq[samples+beams,constrain=0]', 'seq2seq[samples+constrain,constrain]', 'seq2seq[samples+constrain,constrain=0]',
      'seq2seq[beams+constrain,constrain]', 'seq2seq[beams+constrain,constrain=0]',)),
    ("ValueError: sequence_samples needs the native engine: this model's constructor arguments take the sub-module loop", (
      'seq2seq[samples,gelu]', 'seq2seq[samples+constrain,gelu]',)),
    ('ValueError: sequence_samples is a SurfaceFormer option (draws per wireframe of the single-sequence model); SurfaceFormer_Parallel draws per anchor with num_samples', (
      'parallel[samples]', 'parallel[samples+beams]', 'parallel[samples+constrain]', 'parallel[samples,retire_finished]',
      'parallel[samples,return_logprob]', 'parallel[samples,beam_width]', 'parallel[samples,num_samples]',
      'parallel[samples,constrain]', 'parallel[samples,constrain=0]',)),
    ('ValueError: score() excludes sequence_samples: set model.sequence_samples = 0 to score given paths', (
      'parallel.score[samples]', 'seq2seq.score[samples]', 'parallel.score[samples+beams]', 'seq2seq.score[samples+beams]',
      'parallel.score[samples+constrain]', 'seq2seq.score[samples+constrain]',)),
    ('ValueError: sequence_beams excludes sequence_samples, beam_width, return_logprob and an extra mask', (
      'seq2seq[beams,return_logprob]', 'seq2seq[beams,beam_width]', 'seq2seq[beams,extra_mask]',
      'seq2seq[samples+beams,return_logprob]', 'seq2seq[samples+beams,beam_width]', 'seq2seq[samples+beams,stop_each_eos]',
      'seq2seq[samples+beams,extra_mask]', 'seq2seq[samples+beams]', 'seq2seq[beams+constrain,return_logprob]',
      'seq2seq[beams+constrain,beam_width]', 'seq2seq[beams+constrain,extra_mask]',)),
    ("ValueError: sequence_beams needs the native engine: this model's constructor arguments take the sub-module loop", (
      'seq2seq[beams,gelu]', 'seq2seq[samples+beams,gelu]', 'seq2seq[beams+constrain,gelu]',)),
    ('ValueError: sequence_beams is a SurfaceFormer option (beams per wireframe of the single-sequence model); SurfaceFormer_Parallel searches per anchor with beam_width', (
      'parallel[beams]', 'parallel[beams+constrain]',)),
    ('ValueError: score() excludes sequence_beams: set model.sequence_beams = 0 to score given paths', (
      'parallel.score[beams]', 'seq2seq.score[beams]', 'parallel.score[beams+constrain]', 'seq2seq.score[beams+constrain]',)),
    ('ValueError: sequence_constrain excludes sequence_samples, sequence_beams, return_logprob and an extra mask', (
      'seq2seq[constrain,return_logprob]', 'seq2seq[constrain,extra_mask]', 'seq2seq[samples+constrain,beam_width]',
      'seq2seq[samples+constrain,stop_each_eos]', 'seq2seq[samples+constrain]', 'seq2seq[beams+constrain,stop_each_eos]',
      'seq2seq[beams+constrain]', 'seq2seq[constrain=0,samples]',)),
    ('ValueError: sequence_constrain excludes stop_each_eos = True: every row is finished by its own EOS already', (
      'seq2seq[constrain,stop_each_eos]',)),
    ("ValueError: sequence_constrain needs the native engine: this model's constructor arguments take the sub-module loop", (
      'seq2seq[constrain,gelu]',)),
    ("ValueError: sequence_constrain is a SurfaceFormer option (the loop rule per face of the single-sequence model's row); SurfaceFormer_Parallel constrains per anchor with constrain", (
      'parallel[constrain]', 'parallel[constrain=0]',)),
    ('ValueError: score() excludes sequence_constrain: set model.sequence_constrain = None to score given paths', (
      'parallel.score[constrain]', 'seq2seq.score[constrain]', 'seq2seq.score[constrain=0]',
      'parallel.score[constrain,retire_finished]', 'parallel.score[constrain,return_logprob]',
      'parallel.score[constrain,beam_width]',)),
    ('ValueError: score() excludes num_samples: set model.num_samples = 0 to score given paths', (
      'parallel.score[constrain,num_samples]',)),
    ('ValueError: score() excludes constrain: set model.constrain = None to score given paths', (
      'parallel.score[constrain,constrain]', 'parallel.score[constrain,constrain=0]',)),
    ('ValueError: decode_sharded does not implement sequence_samples (a sequence-sampled decode takes no external stop rule)', (
      'sharded[samples]', 'sharded[samples,retire_finished]', 'sharded[samples,return_logprob]', 'sharded[samples,beam_width]',
      'sharded[samples,num_samples]', 'sharded[samples,constrain]', 'sharded[samples,constrain=0]',
      'sharded[samples,constrain_samples]', 'sharded[samples,constrain_beams]', 'sharded[samples+beams]',
      'sharded[samples+beams,retire_finished]', 'sharded[samples+beams,return_logprob]', 'sharded[samples+beams,beam_width]',
      'sharded[samples+beams,num_samples]', 'sharded[samples+beams,constrain]', 'sharded[samples+beams,constrain=0]',
      'sharded[samples+beams,constrain_samples]', 'sharded[samples+beams,constrain_beams]', 'sharded[samples+constrain]',
      'sharded[samples+constrain,retire_finished]', 'sharded[samples+constrain,return_logprob]',
      'sharded[samples+constrain,beam_width]', 'sharded[samples+constrain,num_samples]', 'sharded[samples+constrain,constrain]',
      'sharded[samples+constrain,constrain=0]', 'sharded[samples+constrain,constrain_samples]',
      'sharded[samples+constrain,constrain_beams]',)),
    ('ValueError: decode_sharded does not implement sequence_faces (the faces of a wireframe are made on the rank that decoded it)', (
      'sharded[samples,sequence_faces]', 'sharded[beams,sequence_faces]', 'sharded[constrain,sequence_faces]',
      'sharded[samples+beams,sequence_faces]', 'sharded[samples+constrain,sequence_faces]',
      'sharded[beams+constrain,sequence_faces]',)),
    ('ValueError: decode_sharded does not implement constrain_lookahead (a constrained decode takes no external stop rule)', (
      'sharded[samples,constrain_lookahead]', 'sharded[beams,constrain_lookahead]', 'sharded[constrain,constrain_lookahead]',
      'sharded[samples+beams,constrain_lookahead]', 'sharded[samples+constrain,constrain_lookahead]',
      'sharded[beams+constrain,constrain_lookahead]',)),
    ('ValueError: decode_sharded does not implement sequence_beams (a sequence-beam decode takes no external stop rule)', (
      'sharded[beams]', 'sharded[beams,retire_finished]', 'sharded[beams,return_logprob]', 'sharded[beams,beam_width]',
      'sharded[beams,num_samples]', 'sharded[beams,constrain]', 'sharded[beams,constrain=0]',
      'sharded[beams,constrain_samples]', 'sharded[beams,constrain_beams]', 'sharded[beams+constrain]',
      'sharded[beams+constrain,retire_finished]', 'sharded[beams+constrain,return_logprob]',
      'sharded[beams+constrain,beam_width]', 'sharded[beams+constrain,num_samples]', 'sharded[beams+constrain,constrain]',
      'sharded[beams+constrain,constrain=0]', 'sharded[beams+constrain,constrain_samples]',
      'sharded[beams+constrain,constrain_beams]',)),
    ('ValueError: decode_sharded does not implement sequence_constrain (a sequence-constrained decode takes no external stop rule)', (
      'sharded[constrain]', 'sharded[constrain,retire_finished]', 'sharded[constrain,return_logprob]',
      'sharded[constrain,beam_width]', 'sharded[constrain,num_samples]', 'sharded[constrain,constrain]',
      'sharded[constrain,constrain=0]', 'sharded[constrain,constrain_samples]', 'sharded[constrain,constrain_beams]',
      'sharded[constrain=0]',)),
    ('AssertionError: process group touched: get_rank', (
      'sharded[all off]',)),
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
    assert modes.SEQUENCE_MODES == (modes.SEQUENCE_SAMPLE, modes.SEQUENCE_BEAM, modes.SEQUENCE_CONSTRAIN)
    assert [m.subject for m in modes.SEQUENCE_MODES] == list(OPTIONS)
    # the parallel modes' table is what it was: the three records and their attributes lie outside it
    assert modes.MODES == (modes.CONSTRAIN, modes.SAMPLE, modes.BEAM, modes.GREEDY) and len(modes.MODES) == 4
    assert not set(modes.SEQUENCE_MODES) & set(modes.MODES) and not set(OPTIONS) & set(modes.SWITCH)
    return modes.SEQUENCE_MODES


def test_every_entry_of_the_table_is_bound_with_its_size_query():
    from faceformer_amd.hip import lib
    assert [m.entry for m in _records()] == ["ff_decode_sequence_sample", "ff_decode_sequence_beam", "ff_decode_sequence_constrained"]
    for m in _records():       # the size query takes G where the record says so, and only there; no num_input
        assert m.entry in lib.SIGNATURES and m.entry + "_workspace_bytes" in lib.SIGNATURES, m.entry
        assert len(lib.SIGNATURES[m.entry + "_workspace_bytes"][1]) == 2 + bool(m.per_anchor)
        assert len(lib.SIGNATURES[m.entry][1]) == 14 and not m.term_range and not m.parallel_only


def test_every_excluded_name_is_a_parameter_of_decode_and_the_records_exclude_each_other():
    from faceformer_amd.hip import engine, modes
    decode = set(inspect.signature(engine.PathEngine.decode).parameters)
    records = _records()
    for i, m in enumerate(records):
        assert m.excludes and set(m.excludes) <= decode and len(set(m.excludes)) == len(m.excludes), m.subject
        assert m.subject in decode and m.sequence.parallel_has[1] in decode
        # today's exact relation: a record excludes the option of every record before it in the table, and of no record behind it --
        # so whichever order a layer asks in (decode(): the table's reversed; SurfaceFormer: SEQUENCE_MODEL_ORDER), one of two
        # options set together is refused by the other's record
        assert [k for k in m.excludes if k in OPTIONS] == [n.subject for n in records[:i]]
        assert [k for k in m.model_excludes if k in OPTIONS] == [n.subject for n in records[:i]]
        assert set(m.model_excludes) <= set(OPTIONS) | set(modes.SWITCH) | {"an extra mask"}
    assert sorted(modes.SEQUENCE_MODEL_ORDER, key=records.index) == list(records)
    assert [m.subject for m in modes.SEQUENCE_MODEL_ORDER] == ["sequence_beams", "sequence_samples", "sequence_constrain"]


def test_every_model_attribute_of_the_table_exists_with_its_off_value_on_a_fresh_model():
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    switches = [sw for m in _records() for sw in m.switches]
    assert [(sw.attr, sw.off) for sw in switches] == [("sequence_samples", 0), ("sequence_beams", 0), ("sequence_constrain", None)]
    for model in (_tiny_model(SurfaceFormer_Parallel, max_face_length=5), _tiny_model(SurfaceFormer, label_seq_length=6)):
        for m, sw in zip(_records(), switches):
            assert hasattr(model, sw.attr) and getattr(model, sw.attr) == sw.off and type(getattr(model, sw.attr)) is type(sw.off)
            assert not sw.on(model) and m.sequence.value(sw.off) == sw.off
            assert not hasattr(model, m.sequence.stats)       # (set by the first decode with the option)


ON = {"sequence_samples": 3, "sequence_beams": 3, "sequence_constrain": "loops"}


def _published(out, inputs):
    return {k: (v.dtype, tuple(v.shape[1:])) for k, v in out.items() if k not in inputs}


def _expected_keys(mode, T, S, E=64):
    G = ON[mode.subject] if mode.per_anchor else None
    want = {"embedding": (torch.float32, (S, E)), "predict": (torch.int64, (T,))}
    for key, dims, dtype in mode.outs:
        want["predict_" + key] = (dtype, tuple({"G": G, "T": T}[d] for d in dims))
    return want


@pytest.mark.parametrize("option", OPTIONS)
def test_the_empty_batch_publishes_every_key_of_outs_with_the_recorded_dtype(monkeypatch, option):
    from faceformer_amd.models import SurfaceFormer
    _untouchable(monkeypatch)
    mode = _records()[OPTIONS.index(option)]
    model = _tiny_model(SurfaceFormer, label_seq_length=6)
    setattr(model, option, ON[option])
    inputs = {"input": torch.zeros(0, 8, 50, 2), "input_mask": torch.zeros(0, 8, dtype=torch.bool), "label": torch.zeros(0, 6, dtype=torch.long)}
    with torch.no_grad():
        out = model.forward_eval(dict(inputs))
    assert _published(out, inputs) == _expected_keys(mode, 6, 8 + TOK.len) and "pointer" not in out
    assert [k for k, _, _ in mode.outs] == {"sequence_samples": ["samples", "sample_logprob", "sample_scores"],
                                            "sequence_beams": ["beams", "beam_scores", "beam_finished"],
                                            "sequence_constrain": ["logprob", "dead_end", "open_end"]}[option]


# ---- GPU: forward_eval is the direct decode call, published through the record's outs ------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("option", OPTIONS)
def test_forward_eval_publishes_what_a_direct_decode_call_returns(hip_lib, option):
    """A tiny SurfaceFormer on three wireframes of 8, 5 and 1 edges, G = 3 draws / beams, "loops" on a given follow table: the
    published predict and predict_* tensors against PathEngine.decode on the same encoding, bit for bit (the same launches); and
    the N = 0 batch publishes the same keys, dtypes and trailing shapes."""
    from faceformer_amd import faces
    from faceformer_amd.hip import lib
    from faceformer_amd.models import SurfaceFormer
    mode = _records()[OPTIONS.index(option)]
    torch.manual_seed(7)
    model = _tiny_model(SurfaceFormer, label_seq_length=6).cuda()
    N, L, T, G = 3, 8, 6, 3
    counts = [8, 5, 1]
    gen = torch.Generator().manual_seed(11)
    mask = torch.arange(L)[None, :] >= torch.tensor(counts)[:, None]
    follows = torch.rand((N, L, L), generator=gen) < 0.4
    inputs = {"input": torch.rand((N, L, 50, 2), generator=gen).cuda(), "input_mask": mask.cuda(),
              "label": torch.zeros(N, T, dtype=torch.long).cuda(), "num_input": counts, "follow_table": follows,
              "sample_uniforms": torch.rand((T - 1, N * G), generator=gen)}
    setattr(model, option, ON[option])
    with torch.no_grad():
        out = model.forward_eval(dict(inputs))
        eng, memory, mask_u8, kv_len = model._encode(inputs)
        words = torch.from_numpy(faces.pack_follow_bits(follows.numpy()))
        own = {"sequence_samples": dict(sequence_samples=G, temperature=model.sample_temperature, top_k=model.sample_top_k,
                                        top_p=model.sample_top_p, uniforms=inputs["sample_uniforms"].cuda()),
               "sequence_beams": dict(sequence_beams=G, sequence_beam_stop="all"),
               "sequence_constrain": dict(sequence_constrain=3, tok_sep=TOK.SEP, follow_table=words.cuda())}[option]
        direct = eng.decode(memory, mask_u8, kv_len, lib.FF_SEQ2SEQ, T=T, F=1, chunk_wireframes=model.chunk_wireframes,
                            chunk_seqs=model.chunk_seqs, chunk_max_seqs=model.chunk_max_seqs, num_streams=model.num_streams, sync_every=1,
                            flags=model.decode_flags, x3_min_rows=model.x3_min_rows, ln_fuse_max_rows=model.ln_fuse_max_rows,
                            tok_sos=TOK.SOS, tok_eos=TOK.EOS, **own)
        empty_in = {"input": inputs["input"][:0], "input_mask": inputs["input_mask"][:0], "label": inputs["label"][:0]}
        empty = model.forward_eval(dict(empty_in))
    assert torch.equal(out["embedding"], memory) and torch.equal(out["predict"], direct["predict"])
    assert tuple(out["predict"].shape) == (N, T) and bool((out["predict"][:, 0] == TOK.SOS).all()) and direct["steps"] >= 1
    for key, dims, dtype in mode.outs:
        got = out["predict_" + key]
        assert got.dtype == dtype and tuple(got.shape) == (N,) + tuple({"G": G, "T": T}[d] for d in dims), key
        assert torch.equal(got.reshape(-1), direct[key].reshape(-1)), key
    assert getattr(model, mode.sequence.stats) == {"steps": direct["steps"], "slot_rows": direct["slot_rows"]}
    want = _expected_keys(mode, T, L + TOK.len)
    assert _published(out, inputs) == want and _published(empty, empty_in) == want
    assert all(v.size(0) == 0 for k, v in empty.items() if k not in empty_in)
