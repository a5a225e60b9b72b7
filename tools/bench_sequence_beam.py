"""Cost of the opt-in beam search over the single-sequence decode (SurfaceFormer.sequence_beams, ff_decode_sequence_beam; DESIGN.md
30) on the config A shape: configs/seq2seq.yml (num_lines 110, label_seq_length 259), ONE 110-edge wireframe, gain-4 synthetic
weights.  Whole-decode ms with W = 1, 2, 4, 8 beams under both stop rules, beside one yardstick:

  sampled W       the sequence_samples = W decode of the same wireframe: the same N * W decoder rows off the same
                  encoding and cross-attention K | V.  Beams add only the prefix reorder and one selection over W rows in place of
                  W selections over one row each.

With these weights the greedy sequence never emits EOS (T - 1 = 258 steps), and at the yardstick's temperature 0.25 no draw does
either.  `steps` is printed for every decode; a ratio is printed only when the steps are equal.  The sampled time includes making
the uniforms (torch.rand) on the device, as a model call does.

    python tools/bench_sequence_beam.py [--steps 3] [--beams 1,2,4,8] [--stops all,best] [--out profiles/sequence_beam]

For the launches' own cost run one setting per process under a kernel trace and read the mean durations of
beam_select_kernel<W, 1 | 2> and beam_reorder_kernel:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sequence_beam.py --beams 4 --stops all --no-write

--op-trace N: instead of the decodes, N launches each of the three forms of the selection step (ops.beam_select,
ops.beam_sequence_select with stop_best False / True) and of ops.beam_reorder on ONE shape -- one wireframe of W = 8 beams, S = 114
keys, E = 512, 128 prefix positions -- so that a kernel trace shows the forms' mean durations side by side.
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
from bench_sequence_sample import setup  # noqa: E402


def op_trace(n, W=8, S=114, E=512, npos=128):
    from faceformer_amd.hip import ops
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(W, S, generator=g) * 3.0).cuda()
    scores = (-torch.arange(W, dtype=torch.float32)).cuda()
    fin = torch.zeros(W, dtype=torch.int32).cuda()
    memory = torch.randn(1, S, E, generator=g).cuda()
    mask = torch.zeros(1, S, dtype=torch.uint8).cuda()
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    x0, qkv0 = torch.randn(npos, W, E, generator=g).cuda(), torch.randn(npos, W, 3 * E, generator=g).cuda()
    parent = torch.tensor([(k + 1) % W for k in range(W)], dtype=torch.int32).cuda()      # every row moves
    for _ in range(n):
        kw = dict(mask=mask, memory=memory, want_rows=True, counter=counter)
        ops.beam_select(logits.clone(), scores, fin, W, term_range=(1, 4), ge_bound=4, **kw)
        ops.beam_sequence_select(logits.clone(), scores, fin, W, term_range=(3, 4), stop_best=False, **kw)
        ops.beam_sequence_select(logits.clone(), scores, fin, W, term_range=(3, 4), stop_best=True, **kw)
        ops.beam_reorder(x0, parent, W, rows_b=qkv0)
    torch.cuda.synchronize()
    print("op trace: %d launches of each form and of the reorder, W=%d S=%d E=%d npos=%d" % (n, W, S, E, npos))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="timed calls per setting")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_beam"))
    ap.add_argument("--beams", default="1,2,4,8")
    ap.add_argument("--stops", default="all,best")
    ap.add_argument("--temperature", type=float, default=0.25, help="of the sampled yardstick")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    ap.add_argument("--op-trace", type=int, default=0, metavar="N", help="N launches of each form of the step on one shape; no decode")
    args = ap.parse_args()
    if args.op_trace:
        return op_trace(args.op_trace)
    model, batch, T = setup()
    model.sample_temperature = args.temperature
    timing = {}
    for W in (int(w) for w in args.beams.split(",")):
        model.sequence_beams, model.sequence_samples = 0, W
        sm, smin, sspread, _ = time_decode(model, batch(1), args.steps)
        ssteps = model.last_sample_stats["steps"]
        model.sequence_samples = 0
        print("W=%d sampled yardstick (sequence_samples = %d): %.2f ms (%d steps)" % (W, W, sm, ssteps), flush=True)
        for stop in args.stops.split(","):
            model.sequence_beams, model.sequence_beam_stop = W, stop
            bm, bmin, bspread, _ = time_decode(model, batch(1), args.steps)
            steps = model.last_beam_stats["steps"]
            model.sequence_beams, model.sequence_beam_stop = 0, "all"
            row = {"beam_ms": bm, "beam_ms_min": bmin, "beam_ms_spread": bspread, "beam_steps": steps, "sampled_ms": sm,
                   "sampled_ms_min": smin, "sampled_ms_spread": sspread, "sampled_steps": ssteps}
            if steps == ssteps:
                row["ratio_to_sampled"] = bm / sm
            timing.setdefault("W%d" % W, {})[stop] = row
            print("W=%d stop=%s beams %.2f ms (%d steps) | %s" % (W, stop, bm, steps, "ratio to the sampled decode %.3f" % (bm / sm)
                                                                   if steps == ssteps else "steps differ: no ratio"), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_beam.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
