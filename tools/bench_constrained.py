"""Cost of the opt-in constrained decode (the parallel model's constrain, ff_decode_constrained): whole-decode ms
of a config B-shaped LATTICE wireframe (256 connected co-edges, tests/constrain_ref.py) under constrain = "no_repeat" and
"loops", beside the sampled decode at temperature 0, R = 1 on the same input -- the mode with the same stop semantics and the
same launch structure (decoder pass, pointer GEMM, one selection launch), whose tokens are the retired greedy decode's.  The
decodes stop at different steps (a constrained row cannot end before its loop closes), so the per-step figures are the ones to
compare.  The constrained time includes building the follow table on the device, as a model call does.  Also printed: the
share of own-anchor rows enclosed / dead-ended / unclosed per mode (synthetic weights: this says nothing about trained yield).
The input comes from the TESTS' lattice generator (tests/constrain_ref.lattice_batch): a change to that fixture changes this
benchmark's input, and the numbers recorded under profiles/constrain/ belong to the generator as it was when they were taken.

    python tools/bench_constrained.py [--steps 5] [--forms default,f32] [--out profiles/constrain]

For the kernel's own cost run one setting per process under a kernel trace and read the mean duration of
pointer_constrained_kernel next to pointer_reduce_kernel:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_constrained.py --modes loops --forms default --no-write
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constrain_ref as CR  # noqa: E402
from bench_beam import setup  # noqa: E402
from bench_logprob import time_decode  # noqa: E402
from faceformer_amd import faces  # noqa: E402


def yield_of(pred, dead, n, edges, token):
    enc = de = un = 0
    for f in range(n):
        row = pred[f]
        face = faces._parallel_rows(row[None], token, n)
        ends = ((row >= token.face_type_offset) & (row < token.len)).any()
        if dead is not None and dead[f]:
            de += 1
        elif ends and face and faces.is_face_enclosed(edges, face[0][1], CR.TOL):
            enc += 1
        else:
            un += 1
    return {"enclosed": enc, "dead_end": de, "unclosed": un, "rows": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain"))
    ap.add_argument("--modes", default="greedy,sample0,no_repeat,loops")
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    model, _ = setup()
    T = model.max_face_length
    lat, edges, _ = CR.lattice_batch([256], 256, T, args.seed)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}
    x3 = model.x3_min_rows
    timing = {}
    for form in args.forms.split(","):
        model.x3_min_rows = 0 if form == "f32" else x3
        for mode in args.modes.split(","):
            model.constrain, model.num_samples, model.sample_temperature = None, 0, 1.0
            if mode == "sample0":
                model.num_samples, model.sample_temperature = 1, 0.0
            elif mode != "greedy":
                model.constrain = mode
            ms, mmin, spread, out = time_decode(model, batch, args.steps)
            steps = model.last_decode_stats["steps"]
            dead = out["predict_dead_end"][0].cpu().numpy() != 0 if "predict_dead_end" in out else None
            row = {"ms": ms, "ms_min": mmin, "ms_spread": spread, "steps": steps, "ms_per_step": ms / max(steps, 1)}
            row.update(yield_of(out["predict"][0].cpu().numpy(), dead, 256, edges[0], model.token))
            timing.setdefault(form, {})[mode] = row
            print(form, mode, "%.2f ms, %d steps, %.3f ms/step; own-anchor rows enclosed / dead end / unclosed: %d / %d / %d"
                  % (ms, steps, row["ms_per_step"], row["enclosed"], row["dead_end"], row["unclosed"]), flush=True)
        t = timing[form]
        for mode in ("no_repeat", "loops"):
            if mode in t and "sample0" in t:
                t[mode]["ratio_per_step_vs_sample0"] = t[mode]["ms_per_step"] / t["sample0"]["ms_per_step"]
                print(form, mode, "per step against the sampled decode at temperature 0: %.3f" % t[mode]["ratio_per_step_vs_sample0"])
    model.constrain, model.num_samples, model.sample_temperature = None, 0, 1.0
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_constrained.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
