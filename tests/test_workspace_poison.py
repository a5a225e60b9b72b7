"""GPU: the engine on a dirty workspace.

PathEngine keeps ONE byte tensor for ff_encode and every decode entry; it only grows and is never cleared, so every call runs on
what the call before left there.  Here every workspace the engine asks for is the leading slice, of exactly the size its own
size query reported, of a parent that continues with 64 KiB of canary bytes, and it is filled before the call:

  1  fill independence   every returned tensor after a ZERO (0x00) fill is bit-equal to the one after a POISON (0xFF: NaN as
                         fp32 / fp16, -1 as int32) fill, and holds no NaN
  2  order independence  the result after ANOTHER call (another mode, golden or split kind) has run on the same memory is
                         bit-equal to the one after a ZERO fill
  3  bounds              the canary behind the reported size is untouched after every call
  4  direct calls        eng.encode and eng.decode with `_ws` set by hand to the size of their own query: 1 and 3 again

over the decode modes (greedy with and without log-probabilities, retirement, beam, sampling, both constraints, teacher-forced
scoring), the f32-only engine, the package default and split_kind "fp16", and the drained / two-stream forms of
test_mode_forms.py.  Traces are compared as well (trace=True), so the per-step logits take part, not only the tokens."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import constrain_ref as CR
import redzone as RZ
import sample_ref as SR
import test_mode_forms as MF
from conftest import build_model
from faceformer_amd import faces
from faceformer_amd.hip import lib as L
from faceformer_amd.hip.engine import PathEngine

pytestmark = pytest.mark.gpu

TAIL = 64 << 10
CANARY = 0xA5
PAR = ["par_small_ragged", "par_small_earlybreak", "par_full_n40_gain4"]   # (the last: one wireframe, the folded pointer head)
SEQ = "seq_small_gain4"
KINDS = ["f32", "default", "fp16"]             # f32-only, the package default (fp16x2 planes from 1024 rows), one fp16 product
SAMPLE = (0.8, 5, 0.9)                         # temperature, top-k, top-p
_BOUND, _LATTICE = {}, {}


class _Default(MF.Bound):
    """A golden with the model as the package builds it (no attribute of test_mode_forms.FORMS set)."""

    def __init__(self, name):
        self.name, self.form, self.attrs = name, "default", {}
        self.case, self.z, self.sd, self.batch, self.b = MF._golden(name)
        self.model = build_model(self.case, self.sd, "cuda")
        self.T = self.case["model"]["seq_len"]
        self.parallel = self.case["kind"] == "parallel"
        self.N = len(self.case["n_edges"])
        self.F = max(int(n) for n in self.case["n_edges"]) if self.parallel else 1
        self.what = "%s default" % name


def _bound(name, form):
    if form != "default":
        return MF._bound(name, form)
    if name not in _BOUND:
        _BOUND[name] = _Default(name)
    return _BOUND[name]


def _tuned(form):
    return contextlib.nullcontext() if form == "default" else MF._tuned(form)


# ---- the workspace under test -------------------------------------------------------------------------------------------------------
class Dirty:
    """While installed on engines, every workspace they ask for (PathEngine._workspace(nbytes), nbytes from the entry's own size
    query) is `_ws` = the leading nbytes of a parent with the canary behind them.  fill: a fresh parent per request, its slice
    filled with that byte; shared: ONE parent for every request, never refilled -- each call runs on what the one before left."""

    def __init__(self, engines, fill=None, shared=None):
        self.engines, self.fill, self.shared, self.taken = list(engines), fill, shared, []

    def __enter__(self):
        for eng in self.engines:
            eng._ws = None
            eng._workspace = lambda nbytes, eng=eng: self._take(eng, int(nbytes))
        return self

    def __exit__(self, *exc):
        for eng in self.engines:
            del eng._workspace
            eng._ws = None

    def _take(self, eng, nbytes):
        assert nbytes > 0
        if self.shared is None:
            parent = torch.empty(nbytes + TAIL, device=eng.device, dtype=torch.uint8)
            parent[:nbytes].fill_(self.fill)
            parent[nbytes:].fill_(CANARY)
        else:
            parent = self.shared
            assert parent.numel() >= nbytes + TAIL
        self.taken.append((parent, nbytes))
        eng._ws = parent[:nbytes]
        ws = PathEngine._workspace(eng, nbytes)          # the product's own path: it finds a workspace of exactly that size
        assert ws.data_ptr() == parent.data_ptr() and ws.numel() == nbytes
        return ws

    def check(self, what):
        torch.cuda.synchronize()
        assert self.taken, what
        if self.shared is not None:
            assert bool((self.shared[-TAIL:] == CANARY).all()), (what, "shared parent")
            return
        for parent, nbytes in self.taken:
            bad = torch.nonzero(parent[nbytes:] != CANARY)
            assert bad.numel() == 0, "%s: a workspace of %d bytes was written %d bytes behind its end" % (what, nbytes, int(bad[0]))


def _engines(*ms):
    engines = []
    for m in ms:                                  # (two forms of one golden may share a model: each engine once)
        eng = m.model.engine()
        if not any(eng is e for e in engines):
            engines.append(eng)
    return engines


def _tensors(out):
    return {k: v for k, v in out.items() if torch.is_tensor(v)}


def _assert_equal(got, ref, what):
    assert got.get("steps") == ref.get("steps") and got.get("step_counts") == ref.get("step_counts"), what
    a, b = _tensors(got), _tensors(ref)
    assert a and set(a) == set(b), what
    for k in a:
        RZ.assert_same_bits(a[k], b[k], "%s: %s" % (what, k))


TRACES = ("logits", "best", "second")


def _assert_no_nan(out, what, traces_whole=True):
    """No NaN in any output.  A trace holds the NaN the caller filled it with where no micro-batch ran: behind the executed steps
    and, under retirement or scoring, in the rows of sequences that had left; up to the stop step every other decode fills it."""
    for k, v in _tensors(out).items():
        if not v.is_floating_point():
            continue
        if k in TRACES:
            if not traces_whole:
                continue
            v = v[: out["steps"]]
        assert not bool(torch.isnan(v).any()), (what, k)


# ---- the calls ----------------------------------------------------------------------------------------------------------------------
def _lattice(m):
    if m.name not in _LATTICE:
        mm = m.case["model"]
        lat, _, _ = CR.lattice_batch(m.batch["num_input"], mm["L"], mm["seq_len"], CR.LATTICE_SEEDS.get(m.name, 1))
        table = faces.follow_table(lat["input"].numpy(), CR.TOL, lat["num_input"])
        _LATTICE[m.name] = ({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}, table)
    return _LATTICE[m.name]


def _plain(m):
    from test_logprob import _decode
    return _decode(m.model, m.case, m.b, trace=True, num_streams=m.model.num_streams)


def _retire(m):
    from test_retire_finished import _decode
    return _decode(m.model, m.b, True, trace=True)


def _sample(m):
    from test_sample import _sampled
    u = SR.make_uniforms(m.b["num_input"], m.T, 2, 11).cuda()
    return _sampled(m.model, m.case, m.b, 2, *SAMPLE, u, trace=True)


def _constrain(flags):
    def call(m):
        from test_constrain import _constrained
        b, table = _lattice(m)
        return _constrained(m.model, m.case, b, flags, table, trace=True)
    return call


def _score(m):
    gold = np.ascontiguousarray(m.z["predict"].reshape(-1, m.T))
    return MF._forced(m, gold, MF._own_paths(m, gold, int(m.z["steps"])), trace=True)


MODES = {
    "greedy": _plain,
    "greedy_logprob": MF._greedy,
    "retire": _retire,
    "beam1": lambda m: MF._beam(m, 1, trace=True),
    "beam3": lambda m: MF._beam(m, 3, trace=True),
    "sample": _sample,
    "no_repeat": _constrain(CR.NO_REPEAT),
    "loops": _constrain(MF.LOOPS),
    "score": _score,
}
SEQ_MODES = ("greedy", "greedy_logprob", "score")
PARTIAL_TRACES = ("retire", "score")


def _run(ms, call, fill=None, shared=None, what=""):
    with Dirty(_engines(*ms), fill=fill, shared=shared) as d:
        out = call()
        d.check(what)
    out.pop("engine", None)
    return out, d


def _check_fills(m, mode, what):
    """1 and 3 for one (golden, form, mode); returns the result after the ZERO fill and the sizes the engine asked for."""
    call = lambda: MODES[mode](m)
    with _tuned(m.form):
        zero, d = _run([m], call, fill=RZ.ZERO, what=what + " after ZERO")
        poison, _ = _run([m], call, fill=RZ.POISON, what=what + " after POISON")
    _assert_equal(poison, zero, what)
    _assert_no_nan(poison, what, traces_whole=mode not in PARTIAL_TRACES)
    assert zero["steps"] > 0, what
    return zero, [n for _, n in d.taken]


# ---- 1, 3: every mode under the three kinds -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("form", KINDS)
@pytest.mark.parametrize("name", PAR)
def test_parallel_decode_does_not_depend_on_what_the_workspace_held(hip_lib, name, form, mode):
    _check_fills(_bound(name, form), mode, "%s %s %s" % (name, form, mode))


@pytest.mark.parametrize("mode", SEQ_MODES)
@pytest.mark.parametrize("form", KINDS)
def test_seq2seq_decode_does_not_depend_on_what_the_workspace_held(hip_lib, form, mode):
    _check_fills(_bound(SEQ, form), mode, "%s %s %s" % (SEQ, form, mode))


@pytest.mark.parametrize("form", ["drained", "two_streams"])
@pytest.mark.parametrize("name", ["par_small_ragged", "par_small_earlybreak"])
def test_greedy_launch_forms_do_not_depend_on_what_the_workspace_held(hip_lib, name, form):
    """One wireframe per micro-batch: with more (step, micro-batch) counters than host-mapped slots (the stop rule drains the
    streams and copies the counters out of the workspace) and on two streams (one scratch set per stream)."""
    m = _bound(name, form)
    for mode in ("greedy_logprob", "retire"):
        _check_fills(m, mode, "%s %s %s" % (name, form, mode))


def test_stagger_retirement_does_not_depend_on_what_the_workspace_held(hip_lib):
    """The weights that end most loops early: chunks are compacted at the check points (ff_permute_rows through the scratch of
    the chunk's stream), one 256-edge wireframe."""
    from test_retire_finished import _decode, _stagger_model
    from faceformer_amd.synth import make_wireframes
    model = _stagger_model()
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in make_wireframes(256, 256, 37, "parallel", seeds=[0]).items()}
    outs = []
    for fill in (RZ.ZERO, RZ.POISON):
        with Dirty([model.engine()], fill=fill) as d:
            outs.append(_decode(model, b, True, trace=True))
            d.check("stagger retire")
    _assert_equal(outs[1], outs[0], "stagger retire")
    _assert_no_nan(outs[1], "stagger retire", traces_whole=False)
    sps = outs[0]["slots_per_step"]
    assert 0 < min(v for v in sps if v > 0) < sps[0], sps          # slots were retired


def test_whole_model_call_does_not_depend_on_what_the_workspace_held(hip_lib):
    """model(batch): ff_prepare_mask, ff_encode and ff_decode behind the model's own sorting of the wireframes, each on a
    workspace of its own query's size; the tokens are the golden's."""
    m = _bound("par_small_ragged", "default")
    outs = []
    for fill in (RZ.ZERO, RZ.POISON):
        with Dirty(_engines(m), fill=fill) as d, torch.no_grad():
            outs.append(m.model(dict(m.b))["predict"].clone())
            d.check("model()")
        assert len(d.taken) == 2 and d.taken[0][1] != d.taken[1][1]          # the encoder's and the decode's
    RZ.assert_same_bits(outs[0], outs[1], "model()")
    assert np.array_equal(outs[1].cpu().numpy().reshape(m.z["predict"].shape), m.z["predict"])


# ---- 2: order independence ----------------------------------------------------------------------------------------------------------
ORDERS = [
    # (first: golden, form, mode) -> (then: golden, form, mode)
    (("par_small_ragged", "default", "beam3"), ("par_small_ragged", "default", "greedy_logprob")),
    (("par_small_ragged", "f32", "sample"), ("par_small_ragged", "f32", "loops")),
    (("par_small_ragged", "default", "score"), ("par_small_ragged", "default", "retire")),
    (("par_small_ragged", "f32", "greedy"), ("par_full_n40_gain4", "f32", "greedy_logprob")),   # more wireframes -> one
    (("par_full_n40_gain4", "fp16", "beam3"), ("par_full_n40_gain4", "f32", "sample")),         # fp16 -> f32-only
    (("par_full_n40_gain4", "fp16", "loops"), ("par_small_earlybreak", "fp16", "no_repeat")),
    (("par_small_ragged", "fp16", "retire"), ("par_small_ragged", "fp16", "beam1")),
    (("seq_small_gain4", "default", "score"), ("seq_small_gain4", "default", "greedy")),
]


@pytest.mark.parametrize("first,then", ORDERS, ids=["%s.%s.%s-then-%s.%s.%s" % (a + b) for a, b in ORDERS])
def test_a_decode_does_not_depend_on_the_call_that_used_the_workspace_before(hip_lib, first, then):
    m1, m2 = _bound(*first[:2]), _bound(*then[:2])
    what = "%s after %s" % (then, first)
    ref, sizes2 = _check_fills(m2, then[2], what)
    with _tuned(m1.form):
        _, d1 = _run([m1], lambda: MODES[first[2]](m1), fill=RZ.POISON, what=what)
    cap = max(sizes2 + [n for _, n in d1.taken])
    shared = torch.empty(cap + TAIL, device="cuda", dtype=torch.uint8)
    shared[:cap].fill_(RZ.POISON)
    shared[cap:].fill_(CANARY)
    with Dirty(_engines(m1, m2), shared=shared) as d:
        with _tuned(m1.form):
            MODES[first[2]](m1)
        with _tuned(m2.form):
            got = MODES[then[2]](m2)
        d.check(what)
    got.pop("engine", None)
    _assert_equal(got, ref, what)


# ---- 4: direct calls, `_ws` set by hand --------------------------------------------------------------------------------------------
def _by_hand(eng, nbytes, fill):
    parent = torch.empty(nbytes + TAIL, device="cuda", dtype=torch.uint8)
    parent[:nbytes].fill_(fill)
    parent[nbytes:].fill_(CANARY)
    eng._ws = parent[:nbytes]
    return parent


@pytest.mark.parametrize("form", KINDS)
@pytest.mark.parametrize("name", ["par_small_ragged", "par_full_n40_gain4", SEQ])
def test_encode_and_decode_stay_inside_the_size_their_own_query_reports(hip_lib, name, form):
    m = _bound(name, form)
    eng = m.model.engine()
    mask, kv_len = eng.prepare_mask(m.b["input_mask"])
    inp = m.b["input"].to(torch.float32).flatten(-2, -1)
    enc_bytes = int(L.load().ff_encode_workspace_bytes(C.byref(eng.model), inp.shape[0], inp.shape[1]))
    with _tuned(form):
        dec_bytes = int(MF._workspace_bytes(m))
        assert enc_bytes > 0 and dec_bytes > 0 and enc_bytes != dec_bytes
        mems, outs = [], []
        try:
            for fill in (RZ.ZERO, RZ.POISON):
                parent = _by_hand(eng, enc_bytes, fill)
                memory, _ = eng.encode(inp, mask, kv_len)
                torch.cuda.synchronize()
                assert eng._ws.data_ptr() == parent.data_ptr() and eng._ws.numel() == enc_bytes      # no regrowth: the size sufficed
                assert bool((parent[enc_bytes:] == CANARY).all()), (m.what, "ff_encode wrote behind its workspace")
                mems.append(memory)
                parent = _by_hand(eng, dec_bytes, fill)
                opts = dict(flags=m.model.decode_flags, x3_min_rows=m.model.x3_min_rows, chunk_wireframes=m.model.chunk_wireframes,
                            chunk_max_seqs=m.model.chunk_max_seqs, chunk_seqs=m.model.chunk_seqs, num_streams=m.model.num_streams,
                            ln_fuse_max_rows=m.model.ln_fuse_max_rows, sync_every=m.model.sync_every, trace=True)
                if m.parallel:
                    ni = [int(n) for n in m.b["num_input"]]
                    out = eng.decode(mems[0], mask, kv_len, L.FF_PARALLEL, T=m.T, F=max(ni), num_input=ni, **opts)
                else:
                    out = eng.decode(mems[0], mask, kv_len, L.FF_SEQ2SEQ, T=m.T, F=1, **opts)
                torch.cuda.synchronize()
                assert eng._ws.data_ptr() == parent.data_ptr() and eng._ws.numel() == dec_bytes
                assert bool((parent[dec_bytes:] == CANARY).all()), (m.what, "ff_decode wrote behind its workspace")
                outs.append(out)
        finally:
            eng._ws = None
    RZ.assert_same_bits(mems[0], mems[1], m.what + ": memory")
    assert not bool(torch.isnan(mems[1]).any())
    _assert_equal(outs[1], outs[0], m.what)
    _assert_no_nan(outs[1], m.what)
    if form != "fp16":                       # (one fp16 product: not the golden's tokens everywhere)
        assert np.array_equal(outs[1]["predict"].cpu().numpy().reshape(m.z["predict"].shape), m.z["predict"]), m.what
