"""Cost of the opt-in sampled decode (the parallel model's num_samples, ff_decode_sample): whole-decode ms of config B (one
256-edge wireframe) with R = 1, 2, 4, 8 draws per anchor, beside the greedy decode of the same number of sequences on the same
build (R wireframes of 256 edges: a sampled decode computes R times the decoder rows plus the sample launch, no reorder).
Compare with tools/bench_beam.py at W = R.  The two decodes stop at different steps (random weights; a sampled decode ends
when its last draw ends), so the per-step figures are the ones to compare; `ratio` is of whole decodes, `ratio_per_step` of
ms / steps.  The sampled time includes making the uniforms (torch.rand) on the device, as a model call does.

    python tools/bench_sample.py [--steps 5] [--samples 1,2,4,8] [--forms default,f32] [--out profiles/sample]

For the kernel's own cost run one setting per process under a kernel trace and read the mean duration of pointer_sample_kernel
next to pointer_reduce_kernel<true>:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sample.py --samples 4 --forms default --no-write
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_beam import setup  # noqa: E402
from bench_logprob import time_decode  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample"))
    ap.add_argument("--samples", default="1,2,4,8")
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    model, batch = setup()
    x3 = model.x3_min_rows
    model.sample_temperature, model.sample_top_k, model.sample_top_p = args.temperature, args.top_k, args.top_p
    timing = {}
    for form in args.forms.split(","):
        model.x3_min_rows = 0 if form == "f32" else x3
        for R in (int(r) for r in args.samples.split(",")):
            model.num_samples = R
            sm, smin, sspread, _ = time_decode(model, batch(1), args.steps)
            steps = model.last_decode_stats["steps"]
            model.num_samples = 0
            gm, gmin, gspread, _ = time_decode(model, batch(R), args.steps)
            row = {"sample_ms": sm, "sample_ms_min": smin, "sample_ms_spread": sspread, "sample_steps": steps,
                   "greedy_same_seqs_ms": gm, "greedy_same_seqs_ms_min": gmin, "greedy_same_seqs_ms_spread": gspread,
                   "greedy_steps": model.last_decode_stats["steps"], "ratio": sm / gm}
            row["sample_ms_per_step"], row["greedy_ms_per_step"] = sm / max(steps, 1), gm / max(row["greedy_steps"], 1)
            row["ratio_per_step"] = row["sample_ms_per_step"] / row["greedy_ms_per_step"]
            timing.setdefault(form, {})["R%d" % R] = row
            print(form, "R=%d sampled %.2f ms (%d steps, %.3f ms/step) | greedy, %d wireframes: %.2f ms (%d steps, %.3f ms/step) | "
                  "ratio %.3f, per step %.3f" % (R, sm, steps, row["sample_ms_per_step"], R, gm, row["greedy_steps"],
                                                 row["greedy_ms_per_step"], row["ratio"], row["ratio_per_step"]), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sample.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
