"""Cost of the opt-in beam search (the parallel model's beam_width, ff_decode_beam): whole-decode ms of config B (one 256-edge
wireframe) with W = 1, 2, 4, 8 beams per anchor, beside the greedy decode of the same number of sequences on the same build
(W wireframes of 256 edges: a beam decode computes W times the decoder rows plus the selection and the prefix reorder).

    python tools/bench_beam.py [--steps 5] [--widths 1,2,4,8] [--forms default,f32] [--out profiles/beam]

For the kernels' own cost run one width per process under a kernel trace and read the mean duration of beam_select_kernel /
beam_reorder_kernel:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_beam.py --widths 4 --forms default --no-write
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_logprob import time_decode  # noqa: E402


def setup():
    from faceformer_amd.config import load_cfg
    from faceformer_amd.models import SurfaceFormer_Parallel
    from faceformer_amd.synth import make_state_dict, make_wireframes, state_dict_spec
    cfg = load_cfg(os.path.join(ROOT, "configs", "ours.yml"), ["model.num_lines", "256"])
    T = cfg.model.max_face_length
    spec = state_dict_spec("parallel", 256, T, cfg.model.num_model, cfg.model.num_feedforward,
                           cfg.model.num_encoder_layers, cfg.model.num_decoder_layers)
    model = SurfaceFormer_Parallel(**cfg.model)
    model.load_state_dict(make_state_dict(spec, "default", 0))

    def batch(n):
        b = make_wireframes([256] * n, 256, T, seeds=list(range(n)))
        return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return model.eval().cuda(), batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam"))
    ap.add_argument("--widths", default="1,2,4,8")
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    model, batch = setup()
    x3 = model.x3_min_rows
    timing = {}
    for form in args.forms.split(","):
        model.x3_min_rows = 0 if form == "f32" else x3
        for W in (int(w) for w in args.widths.split(",")):
            model.beam_width = W
            bm, bmin, bspread, out = time_decode(model, batch(1), args.steps)
            steps = model.last_decode_stats["steps"]
            model.beam_width = 0
            gm, gmin, gspread, _ = time_decode(model, batch(W), args.steps)
            row = {"beam_ms": bm, "beam_ms_min": bmin, "beam_ms_spread": bspread, "beam_steps": steps,
                   "greedy_same_seqs_ms": gm, "greedy_same_seqs_ms_min": gmin, "greedy_same_seqs_ms_spread": gspread,
                   "greedy_steps": model.last_decode_stats["steps"], "ratio": bm / gm,
                   "live_beams": int(torch.isfinite(out["predict_beam_scores"]).sum())}
            timing.setdefault(form, {})["W%d" % W] = row
            print(form, "W=%d beam %.2f ms (%d steps) | greedy, %d wireframes: %.2f ms (%d steps) | ratio %.3f"
                  % (W, bm, steps, W, gm, row["greedy_steps"], row["ratio"]), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_beam.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
