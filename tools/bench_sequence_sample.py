"""Cost of the opt-in sampled single-sequence decode (SurfaceFormer.sequence_samples, ff_decode_sequence_sample) on
the config A shape: configs/seq2seq.yml (num_lines 110, label_seq_length 259), ONE 110-edge wireframe, gain-4 synthetic weights.
Whole-decode ms with R = 1, 4, 16, 64 draws, in the package default form and on the f32 matrix cores only, beside two yardsticks:

  R x greedy      R times the greedy one-wireframe decode: what a user who wants R candidates does today;
  greedy batch    the greedy decode of a batch of R copies of that wireframe: the same decoder rows, without the shared encoder
                  and cross-attention K | V (and with the greedy pointer launch in place of the draw).

The weights and the temperature are chosen so that every decode compared runs the same number of steps: with these weights the
greedy sequence never emits EOS (T - 1 = 258 steps), and at the default temperature 0.25 no draw does either, while every step
still runs the whole draw (temperature 0 would take the argmax short cut).  `steps` is printed for every decode; a ratio is
printed only when the steps are equal.  The sampled time includes making the uniforms (torch.rand) on the device, as a model
call does; the greedy single-wireframe time includes return_pointer's extra pass, as today's model call does.

    python tools/bench_sequence_sample.py [--steps 3] [--samples 1,4,16,64] [--forms default,f32] [--out profiles/sequence_sample]

For the launch's own cost run one setting per process under a kernel trace and read the mean duration of
pointer_sample_kernel<true> (and, from tools/bench_sample.py, pointer_sample_kernel<false>):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sequence_sample.py --samples 16 --forms default --no-write

--op-trace N: instead of the decodes, N launches each of the two forms of the sampling step (ops.pointer_sample,
ops.pointer_sequence_sample) on ONE shape -- 64 rows of one wireframe, S = 114 keys, E = 512 -- so that a kernel trace shows the
two forms' mean durations side by side.
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


def setup(edges=110):
    from faceformer_amd.config import load_cfg
    from faceformer_amd.models import SurfaceFormer
    from faceformer_amd.synth import make_state_dict, make_wireframes, state_dict_spec
    cfg = load_cfg(os.path.join(ROOT, "configs", "seq2seq.yml"))
    L, T = cfg.model.num_lines, cfg.model.label_seq_length
    model = SurfaceFormer(**cfg.model)
    model.load_state_dict(make_state_dict(state_dict_spec("seq2seq", L, T), "gain4", 0))
    model = model.eval().cuda()

    def batch(n):
        b = make_wireframes([edges] * n, L, T, "seq2seq", seeds=[3] * n)      # n copies of ONE wireframe
        return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    return model, batch, T


def steps_of(predict):
    """Executed steps of a greedy decode, from its zero padding (the last position that holds a token)."""
    nz = (predict != 0).any(dim=0).nonzero()
    return int(nz.max().item()) if nz.numel() else 0


def op_trace(n, tau, K, P, B=64, S=114, E=512):
    from faceformer_amd.hip import ops
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, S, generator=g) * 3.0).cuda()
    u, memory = torch.rand(B, generator=g).cuda(), torch.randn(1, S, E, generator=g).cuda()
    mask = torch.zeros(1, S, dtype=torch.uint8).cuda()
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    for _ in range(n):
        kw = dict(temperature=tau, top_k=K, top_p=P, memory=memory, mask=mask, seqs_per_group=B, want_rows=True, want_stats=True,
                  counter=counter)
        ops.pointer_sample(logits.clone(), u, term_range=(1, 4), ge_bound=4, **kw)
        ops.pointer_sequence_sample(logits.clone(), u, term_range=(3, 4), **kw)
    torch.cuda.synchronize()
    print("op trace: %d launches of each form, B=%d S=%d E=%d" % (n, B, S, E))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="timed calls per setting")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_sample"))
    ap.add_argument("--samples", default="1,4,16,64")
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--temperature", type=float, default=0.25)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    ap.add_argument("--op-trace", type=int, default=0, metavar="N", help="N launches of each form of the step on one shape; no decode")
    args = ap.parse_args()
    if args.op_trace:
        return op_trace(args.op_trace, args.temperature, args.top_k, args.top_p)
    model, batch, T = setup()
    x3 = model.x3_min_rows
    model.sample_temperature, model.sample_top_k, model.sample_top_p = args.temperature, args.top_k, args.top_p
    timing = {}
    for form in args.forms.split(","):
        model.x3_min_rows = 0 if form == "f32" else x3
        model.sequence_samples = 0
        g1, g1min, g1spread, out = time_decode(model, batch(1), args.steps)
        g1_steps = steps_of(out["predict"])
        print(form, "greedy, one wireframe: %.2f ms (%d steps)" % (g1, g1_steps), flush=True)
        for R in (int(r) for r in args.samples.split(",")):
            model.sequence_samples = R
            sm, smin, sspread, _ = time_decode(model, batch(1), args.steps)
            steps = model.last_sample_stats["steps"]
            model.sequence_samples = 0
            model.stop_each_eos = True      # (a batch of copies: every copy up to its own EOS, as the draws are)
            gm, gmin, gspread, out = time_decode(model, batch(R), args.steps)
            model.stop_each_eos = False
            gsteps = steps_of(out["predict"])
            row = {"sample_ms": sm, "sample_ms_min": smin, "sample_ms_spread": sspread, "sample_steps": steps,
                   "greedy_one_ms": g1, "greedy_one_steps": g1_steps, "r_times_greedy_one_ms": R * g1,
                   "greedy_batch_ms": gm, "greedy_batch_ms_min": gmin, "greedy_batch_ms_spread": gspread, "greedy_batch_steps": gsteps,
                   "selections_per_s": R * steps / (sm * 1e-3)}
            same = steps == g1_steps == gsteps
            if same:
                row["ratio_to_r_times_greedy_one"], row["ratio_to_greedy_batch"] = sm / (R * g1), sm / gm
            timing.setdefault(form, {})["R%d" % R] = row
            print(form, "R=%d sampled %.2f ms (%d steps, %.1f k selections/s) | R x greedy one: %.2f ms (%d steps) | greedy batch of %d: "
                  "%.2f ms (%d steps) | %s" % (R, sm, steps, row["selections_per_s"] / 1e3, R * g1, g1_steps, R, gm, gsteps,
                                               "ratios %.3f, %.3f" % (sm / (R * g1), sm / gm) if same else "steps differ: no ratio"),
                  flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_sample.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
