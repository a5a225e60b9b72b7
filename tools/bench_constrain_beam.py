"""Cost and yield of the opt-in beam search over the constrained keys (the parallel model's constrain_beams,
ff_decode_constrained_beam): whole-decode ms of the config B-shaped LATTICE wireframe (256 connected co-edges,
tests/constrain_ref.py) under constrain = "loops" with W = 1, 2, 4, 8 beams per anchor, beside the plain beam decode
(beam_width = W) of the same input in the same process -- the yardstick: a constrained beam is a plain beam plus the byte rows
and the state.  The decodes stop at different steps (a constrained beam cannot end before its loop closes), so the per-step
figures are the ones to compare.  The constrained time includes building the follow table on the device, as a model call does.
Also printed per W: the own-anchor groups whose best non-dead closed beam is enclosed, the groups with only dead-ended beams and
the groups with only unclosed beams (synthetic weights: this says nothing about trained yield).

    python tools/bench_constrain_beam.py [--steps 5] [--widths 1,2,4,8] [--forms default,f32] [--out profiles/constrain_beam]
    python tools/bench_constrain_beam.py --yield-only        (the three lattice goldens and config B: the yield table alone)

For the kernel's own cost run one width per process under a kernel trace and read the mean duration of
beam_constrained_select_kernel next to beam_select_kernel:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_constrain_beam.py --widths 4 --forms default --no-write
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


def group_yield(beams, scores, dead, ni, edges, token):
    """Own-anchor groups by their best usable beam: beams [N, F, W, T], scores / dead [N, F, W], in rank order."""
    enc = only_dead = only_open = 0
    lo, hi = token.face_type_offset, token.len
    for w, n in enumerate(ni):
        for f in range(n):
            kinds = []
            for k in range(beams.shape[2]):
                if np.isinf(scores[w, f, k]):
                    continue
                row = beams[w, f, k]
                face = faces._parallel_rows(row[None], token, n)
                ends = ((row >= lo) & (row < hi)).any()
                kinds.append("dead" if dead[w, f, k] else
                             "enclosed" if ends and face and faces.is_face_enclosed(edges[w], face[0][1], CR.TOL) else "open")
            if "enclosed" in kinds:
                enc += 1
            elif kinds and all(k == "dead" for k in kinds):
                only_dead += 1
            else:
                only_open += 1
    return {"enclosed": enc, "only_dead_end": only_dead, "unclosed": only_open, "groups": int(sum(ni))}


def decode_yield(model, batch, ni, edges, W):
    model.constrain, model.constrain_beams = "loops", W
    try:
        with torch.no_grad():
            out = model(dict(batch))
    finally:
        model.constrain, model.constrain_beams = None, 0
    return group_yield(out["predict_beams"].cpu().numpy(), out["predict_beam_scores"].cpu().numpy(),
                       out["predict_beam_dead_end"].cpu().numpy() != 0, ni, edges, model.token)


def yield_table(widths):
    from conftest import batch_to, build_model, case_weights_and_batch, load_golden
    table = {}
    for name in ("par_small_gain4", "par_small_ragged", "par_full_n40_gain4"):
        case, _ = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        m = case["model"]
        lat, edges, _ = CR.lattice_batch(batch["num_input"], m["L"], m["seq_len"], CR.LATTICE_SEEDS[name])
        model = build_model(case, sd, "cuda")
        for W in widths:
            table.setdefault(name, {})["W%d" % W] = decode_yield(model, batch_to(lat, "cuda"), lat["num_input"], edges, W)
            print(name, "W=%d" % W, table[name]["W%d" % W], flush=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_beam"))
    ap.add_argument("--widths", default="1,2,4,8")
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--yield-only", action="store_true", help="the yield table of the lattice fixtures, no timing")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]
    model, _ = setup()
    T = model.max_face_length
    lat, edges, _ = CR.lattice_batch([256], 256, T, args.seed)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}
    result = {}
    if args.yield_only:
        result["yield"] = yield_table(widths)
        result["yield"]["config_b_lattice"] = {"W%d" % W: decode_yield(model, batch, [256], edges, W) for W in widths}
        print("config_b_lattice", result["yield"]["config_b_lattice"], flush=True)
    else:
        x3 = model.x3_min_rows
        for form in args.forms.split(","):
            model.x3_min_rows = 0 if form == "f32" else x3
            for W in widths:
                model.constrain, model.constrain_beams = "loops", W
                cm, cmin, cspread, out = time_decode(model, batch, args.steps)
                csteps = model.last_decode_stats["steps"]
                y = group_yield(out["predict_beams"].cpu().numpy(), out["predict_beam_scores"].cpu().numpy(),
                                out["predict_beam_dead_end"].cpu().numpy() != 0, [256], edges, model.token)
                model.constrain, model.constrain_beams, model.beam_width = None, 0, W
                bm, bmin, bspread, _ = time_decode(model, batch, args.steps)
                bsteps = model.last_decode_stats["steps"]
                model.beam_width = 0
                row = {"constrained_beam_ms": cm, "constrained_beam_ms_min": cmin, "constrained_beam_ms_spread": cspread,
                       "constrained_beam_steps": csteps, "constrained_beam_ms_per_step": cm / max(csteps, 1),
                       "beam_ms": bm, "beam_ms_min": bmin, "beam_ms_spread": bspread, "beam_steps": bsteps,
                       "beam_ms_per_step": bm / max(bsteps, 1), "ratio_per_step": (cm / max(csteps, 1)) / (bm / max(bsteps, 1))}
                row.update(y)
                result.setdefault(form, {})["W%d" % W] = row
                print(form, "W=%d constrained beam %.2f ms (%d steps, %.3f ms/step) | plain beam %.2f ms (%d steps, %.3f ms/step) | "
                      "per-step ratio %.3f | %s" % (W, cm, csteps, row["constrained_beam_ms_per_step"], bm, bsteps, row["beam_ms_per_step"],
                                                   row["ratio_per_step"], y), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "yield.json" if args.yield_only else "bench_constrain_beam.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
