"""Retirement of finished face loops in the parallel decoder (FF_RETIRE_FINISHED).

The contract: with retirement on, `predict` is `faces.retired_view` of the reference's `predict` of the same batch -- the tokens
up to min(finish position, retire stop step), zero after -- and `steps` is that stop step.  CPU tests pin retired_view itself
and its face equality on every parallel golden; GPU tests decode through the engine with retirement on and compare exactly."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import batch_to, build_model, case_weights_and_batch, golden_names, load_golden, token_ns
from faceformer_amd import faces

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOK = token_ns()          # len = 4, face_type_offset = 1: tokens 1..3 end a face loop, >= 4 are edges


# ---- CPU: the oracle ------------------------------------------------------------------------------------------------------------
def test_retired_view_on_hand_made_rows():
    p = np.array([
        [0, 5, 6, 2, 7, 8, 0],    # finishes at 3; edges after the terminator are dropped
        [3, 9, 9, 9, 9, 9, 0],    # padding anchor: finished at the start token
        [2, 4, 4, 4, 4, 4, 0],    # anchor 2 (quirk C-3: a face-type token without the offset): finished at 0
        [0, 4, 5, 6, 0, 0, 0],    # never finishes; stops selecting edges at position 4
        [4, 5, 6, 7, 0, 0, 0],    # never finishes; last edge at position 3
    ], dtype=np.int64)
    out, s = faces.retired_view(p, TOK, return_steps=True)
    # reference rule: first j with every row < 4 is j = 6; over unfinished rows (0, 3, 4) position 4 has none
    assert s == 4
    want = np.array([
        [0, 5, 6, 2, 0, 0, 0],
        [3, 0, 0, 0, 0, 0, 0],
        [2, 0, 0, 0, 0, 0, 0],
        [0, 4, 5, 6, 0, 0, 0],
        [4, 5, 6, 7, 0, 0, 0],
    ])
    assert np.array_equal(out, want)
    assert out.shape == p.shape and out.dtype == np.int64
    # shape is kept ([N, F, T]) and the input is not modified
    p3 = p.reshape(1, 5, 7).copy()
    assert np.array_equal(faces.retired_view(p3, TOK), want.reshape(1, 5, 7))
    assert np.array_equal(p3.reshape(5, 7), p)


def test_retired_view_stops_earlier_than_the_reference():
    # row 1 finished at 1 but keeps selecting edges: the reference runs on to position 4, retirement stops at 2
    p = np.array([[0, 5, 0, 0, 0], [0, 1, 6, 7, 8]], dtype=np.int64)
    out, s = faces.retired_view(p, TOK, return_steps=True)
    assert s == 2
    assert np.array_equal(out, [[0, 5, 0, 0, 0], [0, 1, 0, 0, 0]])


def test_retired_view_without_a_stop():
    p = np.array([[0, 4, 5, 6], [7, 8, 9, 10]], dtype=np.int64)
    out, s = faces.retired_view(p, TOK, return_steps=True)
    assert s == 3 and np.array_equal(out, p)


def _par_goldens():
    return sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "par_*.npz"))
                  if "steps" in np.load(f).files)


@pytest.mark.parametrize("name", _par_goldens())
def test_retired_view_keeps_every_face_of_the_parallel_goldens(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    p = z["predict"]
    out, s = faces.retired_view(p, TOK, return_steps=True)
    assert s <= int(z["steps"])
    for w in range(p.shape[0]):
        assert faces._parallel_rows(out[w], TOK, None) == faces._parallel_rows(p[w], TOK, None), (name, w)


def test_retire_is_rejected_where_it_is_not_implemented():
    from faceformer_amd import dist
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    m = SurfaceFormer(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1,
                      num_lines=8, label_seq_length=6, token=TOK)
    m.retire_finished = True
    batch = {"input": torch.zeros(1, 8, 50, 2), "input_mask": torch.zeros(1, 8, dtype=torch.bool),
             "label": torch.zeros(1, 6, dtype=torch.long)}
    with pytest.raises(ValueError):
        m.forward_eval(batch)
    mp = SurfaceFormer_Parallel(num_model=64, num_head=1, num_feedforward=64, num_encoder_layers=1, num_decoder_layers=1,
                                num_lines=8, max_face_length=6, token=TOK)
    assert mp.retire_finished is False
    mp.retire_finished = True
    with pytest.raises(ValueError):
        dist.decode_sharded(mp, batch, dist_mod=None)


def test_cli_flag_is_parallel_only():
    import main as cli
    from faceformer_amd.config import default_cfg
    cfg = default_cfg()
    cfg.model_class = "SurfaceFormer"
    with pytest.raises(ValueError):
        cli.run_test(cfg, None, out_dir="unused", device="cpu", model=object(), retire_finished=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _decode(model, batch, retire, trace=False, **kw):
    from faceformer_amd.hip import lib as L
    eng, memory, mask, kv_len = model._encode(batch)
    ni = [int(n) for n in batch["num_input"]]
    opts = dict(sync_every=model.sync_every, flags=model.decode_flags, x3_min_rows=model.x3_min_rows,
                chunk_wireframes=model.chunk_wireframes, chunk_seqs=model.chunk_seqs, chunk_max_seqs=model.chunk_max_seqs,
                num_streams=model.num_streams, ln_fuse_max_rows=model.ln_fuse_max_rows)
    opts.update(kw)
    return eng.decode(memory, mask, kv_len, L.FF_PARALLEL, T=model.max_face_length, F=max(ni), num_input=ni, trace=trace,
                      extra_mask=model._extra_mask(batch), retire=retire, term_range=(1, 4), **opts)


def _parallel_engine_goldens():
    return [n for n in golden_names() if n.startswith("par_")]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "f32"])
@pytest.mark.parametrize("name", _parallel_engine_goldens())
def test_retired_decode_equals_the_retired_golden(hip_lib, name, form):
    from test_parity_golden import _tol
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    if form == "f32":
        model.x3_min_rows = 0
    out = _decode(model, batch_to(batch, "cuda"), True, trace=True)
    T = case["model"]["seq_len"]
    want, s_r = faces.retired_view(z["predict"], TOK, return_steps=True)
    pred = out["predict"].cpu().numpy().reshape(-1, T)
    want = want.reshape(-1, T)
    assert out["steps"] == s_r
    gold = z["predict"].reshape(-1, T)
    term = (gold >= 1) & (gold < 4)
    fin = np.where(term.any(axis=1), term.argmax(axis=1), T)
    last = np.minimum(fin, s_r)
    assert np.array_equal(pred[:, 0], want[:, 0])
    assert (pred[np.arange(T)[None, :] > last[:, None]] == 0).all()
    # tokens: the bar of test_parity_golden -- equal wherever the reference's top-2 margin is decisive, while the sequence's
    # prefix equals the reference's (the gain-4 goldens are decisive everywhere: there this is exact equality)
    alive = np.ones(pred.shape[0], dtype=bool)
    for s in range(s_r):
        tol = _tol(z["logits"][s])
        kept = s + 1 <= last
        same = pred[:, s + 1] == want[:, s + 1]
        must = alive & kept & (z["margin"][s] > 2 * tol)
        assert same[must].all(), (s, np.where(must & ~same)[0][:8])
        alive &= same | ~kept
    if "gain4" in name:
        assert np.array_equal(pred, want), np.argwhere(pred != want)[:8]
    # logits of every traced row up to its last kept position
    logits = out["logits"].cpu().numpy()
    for s in range(s_r):
        tol = _tol(z["logits"][s])
        for ri, b in enumerate(z["logit_rows"]):
            if s + 1 <= last[b]:
                d = np.abs(logits[s, b] - z["logits"][s, ri]).max()
                assert d <= tol, (s, int(b), d, tol)
    # fewer decoder rows than the default decode of the same batch
    # strictly fewer decoder rows than the default decode of the same batch: every golden has padding anchors or anchors
    # 1..3, which are finished at their start token
    base = _decode(model, batch_to(batch, "cuda"), False)
    assert out["slot_rows"] < base["slot_rows"]


ENGINE_OPTIONS = [
    dict(sync_every=1),
    dict(sync_every=4),
    dict(chunk_seqs=8),
    dict(num_streams=2, chunk_wireframes=1),
    dict(chunk_wireframes=16),
    dict(retire_min_shrink=0.0, sync_every=1),
    dict(retire_min_shrink=0.0, sync_every=2, chunk_wireframes=1, num_streams=2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ENGINE_OPTIONS, ids=lambda o: "-".join("%s%s" % kv for kv in sorted(o.items())))
@pytest.mark.parametrize("name", ["par_small_ragged", "par_small_earlybreak", "par_full_n40_gain4", "par_small_extramask"])
def test_retired_decode_under_engine_options(hip_lib, name, opts):
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    b = batch_to(batch, "cuda")
    dec_opts = {k: v for k, v in opts.items() if k != "retire_min_shrink"}
    base = _decode(model, b, False, **dec_opts)
    T = case["model"]["seq_len"]
    want, s_r = faces.retired_view(base["predict"].cpu().numpy().reshape(-1, T), TOK, return_steps=True)
    out = _decode(model, b, True, **opts)
    assert out["steps"] == s_r
    assert np.array_equal(out["predict"].cpu().numpy().reshape(-1, T), want)


@pytest.mark.gpu
def test_retired_decode_without_host_slots_drains_and_copies(hip_lib):
    """FF_PINNED_COUNTERS=8 (a child process): neither the counters nor the finish positions fit the host-mapped slots, the
    check points drain the streams and copy them."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import batch_to, build_model, case_weights_and_batch, load_golden, token_ns\n"
        "from faceformer_amd import faces\n"
        "for name in ('par_small_earlybreak', 'par_small_ragged', 'par_full_n40_gain4'):\n"
        "    case, z = load_golden(name)\n"
        "    sd, batch = case_weights_and_batch(case)\n"
        "    model = build_model(case, sd, 'cuda')\n"
        "    for cw in (1, 16):\n"
        "        model.chunk_wireframes = cw\n"
        "        model.retire_finished = True\n"
        "        with torch.no_grad():\n"
        "            pred = model(batch_to(batch, 'cuda'))['predict'].cpu().numpy()\n"
        "        assert np.array_equal(pred, faces.retired_view(z['predict'], token_ns())), (name, cw)\n"
        "print('ok')\n" % (os.path.dirname(here), here))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FF_PINNED_COUNTERS="8"))
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stderr[-2000:]


@pytest.mark.gpu
def test_model_knob_and_decode_stats(hip_lib):
    case, z = load_golden("par_small_ragged")
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    with torch.no_grad():
        ref = model(batch_to(batch, "cuda"))["predict"].cpu().numpy()
        stats0 = dict(model.last_decode_stats)
        model.retire_finished = True
        got = model(batch_to(batch, "cuda"))["predict"].cpu().numpy()
        stats1 = dict(model.last_decode_stats)
    assert np.array_equal(ref, z["predict"])
    assert np.array_equal(got, faces.retired_view(z["predict"], TOK))
    assert set(stats0) >= {"decoded_seqs", "rows", "slot_rows", "steps"}
    assert stats1["slot_rows"] < stats0["slot_rows"]
    assert stats0["steps"] == int(z["steps"])


@pytest.mark.gpu
@pytest.mark.parametrize("npos,src_rows,keep", [(5, 37, 20), (3, 64, 64), (4, 16, 0), (1, 300, 1), (2, 33, 17)])
@pytest.mark.parametrize("width", [512, 1536, 32, 44])
def test_permute_rows_against_index_select(hip_lib, npos, src_rows, keep, width):
    from faceformer_amd.hip import lib as L
    from faceformer_amd.hip.ops import _p, _stream
    g = torch.Generator().manual_seed(npos * 1000 + src_rows + width)
    src = torch.randn(npos, src_rows, width, generator=g).cuda()
    idx = torch.randperm(src_rows, generator=g)[:keep].to(torch.int32).cuda()
    dst = torch.full((npos, max(keep, 1), width), float("nan"), device="cuda")
    L.check(hip_lib.ff_permute_rows(_p(src), src_rows, _p(idx), _p(dst), max(keep, 1), None, npos, keep, width, _stream()),
            "ff_permute_rows")
    torch.cuda.synchronize()
    if keep:
        assert torch.equal(dst, src.index_select(1, idx.long()))
    else:
        assert torch.isnan(dst).all()
    # scatter form: dst rows named by the index
    back = torch.zeros_like(src)
    L.check(hip_lib.ff_permute_rows(_p(dst), max(keep, 1), None, _p(back), src_rows, _p(idx), npos, keep, width, _stream()),
            "ff_permute_rows")
    torch.cuda.synchronize()
    if keep:
        assert torch.equal(back.index_select(1, idx.long()), src.index_select(1, idx.long()))


@pytest.mark.gpu
def test_rejected_combinations_return_ff_err_arg(hip_lib):
    from faceformer_amd.hip import lib as L
    case, z = load_golden("par_small_ragged")
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    b = batch_to(batch, "cuda")
    eng, memory, mask, kv_len = model._encode(b)
    ni = [int(n) for n in b["num_input"]]
    T, F = model.max_face_length, max(ni)
    base = dict(T=T, F=F, num_input=ni, flags=model.decode_flags | L.FF_RETIRE_FINISHED)
    for kw in (dict(no_stop=True), dict(return_pointer=True), dict(stop_callback=lambda c: False)):
        with pytest.raises(L.HipExtensionError, match="FF_RETIRE_FINISHED"):
            eng.decode(memory, mask, kv_len, L.FF_PARALLEL, **base, **kw)
    with pytest.raises(L.HipExtensionError, match="parallel-variant"):
        eng.decode(memory, mask, kv_len, L.FF_SEQ2SEQ, T=T, F=1, flags=model.decode_flags | L.FF_RETIRE_FINISHED)
    with pytest.raises(ValueError):
        eng.decode(memory, mask, kv_len, L.FF_PARALLEL, T=T, F=F, num_input=ni, retire=True, term_range=(1, 4), no_stop=True)


def _stagger_model():
    from faceformer_amd.models import SurfaceFormer_Parallel
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    m = SurfaceFormer_Parallel(num_model=512, num_head=8, num_feedforward=1024, num_encoder_layers=6, num_decoder_layers=6,
                               num_lines=256, max_face_length=37, token=TOK)
    m.load_state_dict(make_state_dict(state_dict_spec("parallel", 256, 37, 512, 1024, 6, 6), "stagger", 0))
    return m.eval().cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "f32"])
@pytest.mark.parametrize("n", [1, 16])
def test_stagger_recipe_retires_and_keeps_the_tokens(hip_lib, n, form):
    """The 'stagger' weights end most loops early (profiles/retire/stagger_tuning.txt): the retired decode equals retired_view
    of the default decode of the same batch and computes clearly fewer decoder rows."""
    from faceformer_amd.synth import make_wireframes
    model = _stagger_model()
    if form == "f32":
        model.x3_min_rows = 0
    b = batch_to(make_wireframes(256, 256, 37, "parallel", seeds=list(range(n))), "cuda")
    with torch.no_grad():
        ref = model(dict(b))["predict"].cpu().numpy()
        st0 = dict(model.last_decode_stats)
        model.retire_finished = True
        got = model(dict(b))["predict"].cpu().numpy()
        st1 = dict(model.last_decode_stats)
    want, s_r = faces.retired_view(ref, TOK, return_steps=True)
    assert st1["steps"] == s_r
    assert np.array_equal(got, want)
    # one wireframe: the chunk narrows with its own live count.  Sixteen in one micro-batch: the chunk keeps the widest live
    # count of its wireframes, so the saving is what the slowest wireframe allows -- smaller, still present
    bound = 0.75 if n == 1 else 1.0
    assert st1["slot_rows"] < bound * st0["slot_rows"], (st1["slot_rows"], st0["slot_rows"])


@pytest.mark.gpu
def test_cli_retire_finished_writes_the_default_records(hip_lib, tmp_path):
    """main.py --retire-finished on the co-edge CLI case (post-processing on): byte-identical JSON records to the default run."""
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import main as cli
    from faceformer_amd.config import load_cfg
    from faceformer_amd.synth import make_state_dict, state_dict_spec
    gold = json.load(open(os.path.join(GOLDEN, "cli_coedge_case.json")))
    m = gold["model"]
    root = tmp_path / "data"
    (root / "json").mkdir(parents=True)
    names = []
    for i, smp in enumerate(gold["samples"]):
        json.dump(smp["raw"], open(root / "json" / ("%08d.json" % i), "w"))
        names.append("json/%08d.json" % i)
    open(root / "test.txt", "w").write("\n".join(names) + "\n")
    cfg = load_cfg("configs/ours.yml", ["model.num_lines", str(m["num_lines"]), "model.max_face_length",
                                         str(m["max_face_length"]), "model.num_model", str(m["num_model"]),
                                         "model.num_head", str(m["num_head"]), "model.num_feedforward",
                                         str(m["num_feedforward"]), "model.num_encoder_layers",
                                         str(m["num_encoder_layers"]), "model.num_decoder_layers",
                                         str(m["num_decoder_layers"]), "root_dir", str(root)])
    spec = state_dict_spec("parallel", m["num_lines"], m["max_face_length"], m["num_model"], m["num_feedforward"],
                           m["num_encoder_layers"], m["num_decoder_layers"])
    sd = make_state_dict(spec, gold["recipe"], gold["wseed"])
    ckpt = tmp_path / "last.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "hyper_parameters": dict(cfg)}, ckpt)
    a = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "default"))
    b = cli.run_test(cfg, str(ckpt), out_dir=str(tmp_path / "retire"), retire_finished=True)
    for i, smp in enumerate(gold["samples"]):
        ra = open(os.path.join(a, "%08d.json" % i), "rb").read()
        rb = open(os.path.join(b, "%08d.json" % i), "rb").read()
        assert ra == rb
        assert json.loads(ra)["pred_faces"] == smp["pred_faces"]
