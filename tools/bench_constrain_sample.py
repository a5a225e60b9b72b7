"""Cost and yield of the opt-in sampling over the constrained decode (the parallel model's constrain_samples,
ff_decode_constrained_sample): whole-decode ms of the config B-shaped LATTICE wireframe (256 connected co-edges,
tests/constrain_ref.py) under constrain = "loops" with R = 1, 2, 4, 8 draws per anchor, in the plain form and with
constrain_lookahead / constrain_exact, beside the two paths it is made of, timed in the same process on the same input: the
plain sampled decode at the same R (num_samples) and the constrained greedy decode of the same form (one sequence per anchor).
The decodes stop at different steps, so the per-step figures are the ones to compare; the ratios are of ms / step.  Every time
includes what a model call makes on the device: the uniforms, the follow table and the form's distance tables.
Also printed: enclosed / dead-ended / unclosed own-anchor draws (synthetic weights say nothing about trained yield).

    python tools/bench_constrain_sample.py [--steps 5] [--samples 1,2,4,8] [--forms default,f32] [--out profiles/constrain_sample]
    python tools/bench_constrain_sample.py --yield-only     (the three lattice goldens and config B at R = 4, tau = 1: the yield table)

For the kernel's own cost run one setting per process under a kernel trace and read the mean duration of
pointer_constrained_sample_kernel<FORM> next to pointer_sample_kernel and pointer_constrained_form_kernel<FORM>:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_constrain_sample.py --samples 4 --forms default --no-write
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
from bench_lookahead import row_yield  # noqa: E402
from faceformer_amd import faces  # noqa: E402

RULES = (("plain", {}), ("lookahead", {"constrain_lookahead": True}), ("exact", {"constrain_exact": True}))


def _set(model, constrain, opts, R=0):
    model.constrain = constrain
    model.constrain_lookahead = bool(opts.get("constrain_lookahead"))
    model.constrain_exact = bool(opts.get("constrain_exact"))
    model.constrain_samples = R


def draw_yield(out, ni, edges, token):
    """enclosed / dead_end / other over ALL draws of the own anchors: predict_samples [N, F, R, T], predict_sample_dead_end [N, F, R]."""
    smp, dead = out["predict_samples"].cpu().numpy(), out["predict_sample_dead_end"].cpu().numpy() != 0
    tot = {}
    for k in range(smp.shape[2]):
        for key, v in row_yield(smp[:, :, k], dead[:, :, k], ni, edges, token).items():
            if isinstance(v, (int, np.integer)):
                tot[key] = tot.get(key, 0) + int(v)
    return tot


def decode_yield(model, batch, ni, edges, opts, R):
    res = {}
    try:
        with torch.no_grad():
            _set(model, "loops", opts, 0)
            g = model(dict(batch))
            res["greedy"] = {k: v for k, v in row_yield(g["predict"].cpu().numpy(), g["predict_dead_end"].cpu().numpy() != 0, ni, edges,
                                                        model.token).items() if isinstance(v, (int, np.integer))}
            _set(model, "loops", opts, R)
            res["draws"] = draw_yield(model(dict(batch)), ni, edges, model.token)
    finally:
        _set(model, None, {})
    return res


def yield_table(R):
    from conftest import batch_to, build_model, case_weights_and_batch, load_golden
    table = {}
    for name in ("par_small_gain4", "par_small_ragged", "par_full_n40_gain4"):
        case, _ = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        m = case["model"]
        lat, edges, _ = CR.lattice_batch(batch["num_input"], m["L"], m["seq_len"], CR.LATTICE_SEEDS[name])
        model = build_model(case, sd, "cuda")
        model.sample_temperature, model.sample_top_k, model.sample_top_p, model.sample_seed = 1.0, 0, 1.0, 5
        table[name] = {key: decode_yield(model, batch_to(lat, "cuda"), lat["num_input"], edges, opts, R) for key, opts in RULES}
        print(name, table[name], flush=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_sample"))
    ap.add_argument("--samples", default="1,2,4,8")
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--rules", default="plain,lookahead,exact")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--yield-only", action="store_true", help="the yield table of the lattice fixtures at R = 4, no timing")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    model, _ = setup()
    T = model.max_face_length
    lat, edges, _ = CR.lattice_batch([256], 256, T, args.seed)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}
    model.sample_temperature, model.sample_top_k, model.sample_top_p, model.sample_seed = 1.0, 0, 1.0, 5
    result, name = {}, "bench_constrain_sample.json"
    if args.yield_only:
        name = "yield.json"
        result["yield"] = yield_table(4)
        result["yield"]["config_b_lattice"] = {key: decode_yield(model, batch, [256], edges, opts, 4) for key, opts in RULES}
        print("config_b_lattice (T = %d)" % T, result["yield"]["config_b_lattice"], flush=True)
    else:
        x3 = model.x3_min_rows
        rules = [r for r in RULES if r[0] in args.rules.split(",")]
        for form in args.forms.split(","):
            model.x3_min_rows = 0 if form == "f32" else x3
            greedy = {}
            for key, opts in rules:       # the constrained greedy decode of every form, once
                _set(model, "loops", opts)
                ms, ms_min, spread, _ = time_decode(model, batch, args.steps)
                greedy[key] = {"ms": ms, "ms_min": ms_min, "ms_spread": spread, "steps": model.last_decode_stats["steps"]}
                greedy[key]["ms_per_step"] = ms / max(greedy[key]["steps"], 1)
                _set(model, None, {})
            for R in (int(r) for r in args.samples.split(",")):
                model.num_samples = R
                ms, ms_min, spread, _ = time_decode(model, batch, args.steps)
                steps = model.last_decode_stats["steps"]
                model.num_samples = 0
                row = {"sampled": {"ms": ms, "ms_min": ms_min, "ms_spread": spread, "steps": steps, "ms_per_step": ms / max(steps, 1)}}
                for key, opts in rules:
                    _set(model, "loops", opts, R)
                    ms, ms_min, spread, out = time_decode(model, batch, args.steps)
                    steps = model.last_decode_stats["steps"]
                    _set(model, None, {})
                    cell = {"ms": ms, "ms_min": ms_min, "ms_spread": spread, "steps": steps, "ms_per_step": ms / max(steps, 1)}
                    cell["per_step_over_sampled"] = cell["ms_per_step"] / row["sampled"]["ms_per_step"]
                    cell["per_step_over_constrained_greedy"] = cell["ms_per_step"] / greedy[key]["ms_per_step"]
                    cell.update(draw_yield(out, [256], edges, model.token))
                    row[key] = cell
                    print(form, "R=%d %s: %.2f ms (%d steps, %.3f ms/step) | sampled R=%d %.3f ms/step, ratio %.3f | constrained greedy "
                          "%.3f ms/step, ratio %.3f | draws %s"
                          % (R, key, cell["ms"], steps, cell["ms_per_step"], R, row["sampled"]["ms_per_step"], cell["per_step_over_sampled"],
                             greedy[key]["ms_per_step"], cell["per_step_over_constrained_greedy"],
                             {k: cell[k] for k in ("enclosed", "dead_end", "other") if k in cell}), flush=True)
                result.setdefault(form, {"constrained_greedy": greedy})["R%d" % R] = row
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, name), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
