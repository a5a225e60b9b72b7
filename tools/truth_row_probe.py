"""Where does one row of a golden leave the fp64 truth?  (GPU; used for TRUTH_ROW_EXCEPTIONS in tests/test_parity_golden.py.)

    python tools/truth_row_probe.py [--name par_small_ragged300] [--row 141] [--out DIR]

Prints, for the HIP trace of the golden (package default) against the oracle in fp64 teacher-forced along the HIP's tokens:
the row's error per step and the worst rows of every step with their position in a 64-row tile; the worst error by tile
position at the row's worst step; the encoder output's per-row error; an fp64 decoder fed the HIP's encoder output (how much
of the error is the encoder's); torch's fp32 on the GPU along the same tokens; and the row under other engine options.
Writes DIR/truth_row_probe.npz (trace, truth, both encoder outputs)."""
import argparse
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import conftest  # noqa
import numpy as np, torch
import test_parity_golden as P  # noqa: E402
from oracle import refpath
from faceformer_amd.hip import lib as L
L.load()
ap = argparse.ArgumentParser()
ap.add_argument("--name", default="par_small_ragged300")
ap.add_argument("--row", type=int, default=141)
ap.add_argument("--out", default=".")
args = ap.parse_args()
out_dir, name, ROW = args.out, args.name, args.row
os.makedirs(out_dir, exist_ok=True)
case, z = P.load_golden(name)
sd, batch = P.case_weights_and_batch(case)
T = case["model"]["seq_len"]; H = case["model"]["H"]
F = max(int(n) for n in batch["num_input"])
def trace(model):
    o = P.run_traced(model, case, P.batch_to(batch, "cuda"))
    return o["predict"].cpu().numpy().reshape(-1, T), int(o["steps"]), o["logits"].cpu().numpy(), o["memory"].float().cpu().numpy()
model = P.build_model(case, sd, "cuda")
pred, steps, lg, mem = trace(model)
sd64 = {k: (v.to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda")) for k, v in sd.items()}
b64 = {k: (v.to("cuda", torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}
forced = torch.from_numpy(pred).to("cuda")
def oracle(encoder_out=None, sdx=sd64, bx=b64):
    orig = refpath.encoder
    if encoder_out is not None:
        refpath.encoder = lambda *a, **k: encoder_out
    try:
        tr = {}
        refpath.parallel_forward_eval(sdx, dict(bx), num_head=H, trace=tr, forced=forced, steps=steps, num_anchors=F)
    finally:
        refpath.encoder = orig
    return torch.stack(tr["logits"]).double().cpu().numpy(), tr["memory"].double().cpu().numpy()
truth, mem64 = oracle()
live = truth > np.finfo(np.float64).min
tol = np.array([P._tol(truth[s]) for s in range(steps)])
def ratio(x):
    return np.where(live, np.abs(x.astype(np.float64) - truth), 0).max(axis=2) / tol[:, None]
r = ratio(lg)
np.savez_compressed(os.path.join(out_dir, "truth_row_probe.npz"), pred=pred, logits=lg, truth=truth, mem=mem, mem64=mem64)
print("HIP tokens row %d:" % ROW, pred[ROW], " golden:", z["predict"].reshape(-1, T)[ROW])
print("HIP ratio per step, row %d:" % ROW, np.round(r[:, ROW], 3), " worst per step:", np.round(r.max(axis=1), 3), "argmax rows", r.argmax(axis=1))
for s in range(steps):
    top = np.argsort(r[s])[::-1][:8]
    print(" step %d top rows %s" % (s, [(int(i), round(float(r[s, i]), 3), "tilepos %d" % (i % 64)) for i in top]))
# tile position pattern at step 1 (rows of wireframe 0, which are not deduplicated)
sw, wf = int(np.argmax(r[:, ROW])), ROW // F
rw = r[sw, wf * F:(wf + 1) * F]
bypos = [rw[np.arange(F) % 64 == p].max() for p in range(64)]
print("step %d, wireframe %d: max ratio by position in a 64-row tile:" % (sw, wf), np.round(bypos, 2))
print("step %d all rows: median %.3f p99 %.3f p99.9 %.3f max %.3f" % ((sw,) + tuple(np.percentile(r[sw], [50, 99, 99.9, 100]))))
# encoder: memory error per memory row (relative to the row's norm)
me = np.abs(mem - mem64).max(axis=2) / np.abs(mem64).max(axis=2)
print("encoder output rel err per memory row: median %.2e max %.2e at (wireframe, row) %s; the row's anchor: %.2e"
      % (np.median(me), me.max(), tuple(int(i) for i in np.unravel_index(me.argmax(), me.shape)), me[wf, pred[ROW, 0]]))
# fp64 decoder on the HIP's encoder output: how much of the error is the encoder's?
hm = torch.from_numpy(mem).to("cuda", torch.float64).transpose(0, 1).contiguous()
dec_on_hipmem, _ = oracle(encoder_out=hm)
rd = np.where(live, np.abs(dec_on_hipmem - truth), 0).max(axis=2) / tol[:, None]
rh = np.where(live, np.abs(lg[:steps].astype(np.float64) - dec_on_hipmem), 0).max(axis=2) / tol[:, None]
print("fp64 decoder on HIP memory vs truth, row %d:" % ROW, np.round(rd[:, ROW], 3), "worst", np.round(rd.max(axis=1), 3), rd.argmax(axis=1))
print("HIP vs fp64 decoder on HIP memory (decoder's own error), row %d:" % ROW, np.round(rh[:, ROW], 3), "worst", np.round(rh.max(axis=1), 3), rh.argmax(axis=1))
# torch fp32 on GPU
sd32 = {k: v.to("cuda") for k, v in sd.items()}
b32 = {k: (v.to("cuda") if torch.is_tensor(v) else v) for k, v in batch.items()}
torch.backends.cuda.matmul.allow_tf32 = False
l32, m32 = oracle(sdx=sd32, bx=b32)
r32 = ratio(l32)
print("torch fp32 GPU, row %d:" % ROW, np.round(r32[:, ROW], 3), "worst", np.round(r32.max(axis=1), 3), r32.argmax(axis=1))
me32 = np.abs(m32 - mem64).max(axis=2) / np.abs(mem64).max(axis=2)
print("torch fp32 encoder output rel err, the row's anchor: %.2e, max %.2e" % (me32[wf, pred[ROW, 0]], me32.max()))
# engine options
for label, kw in [("f32 only", dict(x3_min_rows=0)), ("flags 0", dict(decode_flags=0)), ("flags 3", dict(decode_flags=3)),
                  ("flags 19", dict(decode_flags=19)), ("flags 32", dict(decode_flags=32)), ("chunk_seqs 5", dict(chunk_seqs=5))]:
    m = P.build_model(case, sd, "cuda")
    for k, v in kw.items():
        setattr(m, k, v)
    p2, s2, l2, mm2 = trace(m)
    if s2 != steps or not np.array_equal(p2, pred):
        print(label, "different tokens/steps"); continue
    r2 = ratio(l2)
    print("%-14s row %d: %s worst %s at %s  encoder output bit-equal %s" % (label, ROW, np.round(r2[:, ROW], 3), np.round(r2.max(axis=1), 3), r2.argmax(axis=1), np.array_equal(mm2, mem)))
