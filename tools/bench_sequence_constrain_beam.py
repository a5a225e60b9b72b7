"""Cost of the opt-in beam search over the loop-constrained single-sequence decode (SurfaceFormer.sequence_constrain_beams,
ff_decode_sequence_constrained_beam) on the config A shape: configs/seq2seq.yml (num_lines 110, label_seq_length
259), ONE 110-edge lattice wireframe (tests/constrain_ref.lattice_batch), gain-4 synthetic weights.  Whole-decode ms by device
events around PathEngine.decode (the encoder runs once, outside), 3 timed calls after a warm-up, for W = 1 / 2 / 4 / 8:

  sequence_beams = W        the unconstrained beams: the decode that exists without the option
  loops / coedge_loops      sequence_constrain with sequence_constrain_beams = W, stop rule "all" (and "best" with --best)
  greedy                    one sequence_constrain decode of the same form

`steps` and ms per step are printed for every form; a whole-decode ratio only where the step counts are equal.

    python tools/bench_sequence_constrain_beam.py [--calls 3] [--out profiles/sequence_constrain_beam]

--op-trace N: instead of the decodes, N launches each of ops.beam_sequence_select (beam_select_kernel<W, 1>) and of
ops.beam_sequence_constrained_select under "coedge_loops" on the SAME rows -- one wireframe, W beams (--width, default 8), S = 114
keys, E = 512 -- so that a kernel trace shows the two selection launches' mean durations side by side:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sequence_constrain_beam.py --op-trace 200
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_sequence_constrain import time_call  # noqa: E402
from bench_sequence_sample import setup  # noqa: E402


def op_trace(n, W=8, S=114, E=512, ntok=4):
    import numpy as np
    import constrain_ref as CR
    from faceformer_amd import faces
    from faceformer_amd.hip import ops
    g = torch.Generator().manual_seed(0)
    L = S - ntok
    raw, memory = (torch.randn(W, S, generator=g) * 3).cuda(), torch.randn(1, S, E, generator=g).cuda()
    mask = torch.zeros(1, S, dtype=torch.uint8).cuda()
    table = torch.from_numpy(faces.pack_follow_bits(CR.random_follows(1, L, 1))).cuda()
    fin = torch.zeros(W, dtype=torch.int32).cuda()
    scores = -torch.arange(W, dtype=torch.float32).cuda()
    first, prev = torch.full((W,), 3, dtype=torch.int32).cuda(), torch.full((W,), 5, dtype=torch.int32).cuda()      # open loops
    visited = torch.from_numpy(np.array([[0x28] + [0] * ((L + 31) // 32 - 1)] * W, dtype=np.int32)).cuda()
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    for _ in range(n):
        ops.beam_sequence_select(raw.clone(), scores, fin, W, groups_per_wireframe=1, mask=mask, term_range=(3, 4), memory=memory,
                                 want_rows=True, counter=counter)
        ops.beam_sequence_constrained_select(raw.clone(), scores, fin, first, prev, visited, W, 7, ntok, 2, 3, follows=table, memory=memory,
                                             mask=mask, groups_per_wireframe=1, want_rows=True, want_stats=True, counter=counter)
    torch.cuda.synchronize()
    print("op trace: %d launches of each selection, W=%d S=%d E=%d" % (n, W, S, E))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="timed calls per form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_constrain_beam"))
    ap.add_argument("--no-write", action="store_true", help="print only")
    ap.add_argument("--best", action="store_true", help="also the stop rule 'best'")
    ap.add_argument("--op-trace", type=int, default=0, metavar="N", help="N launches of each selection on one shape; no decode")
    ap.add_argument("--width", type=int, default=8, help="beams of the op trace")
    ap.add_argument("--widths", type=int, nargs="*", default=[1, 2, 4, 8])
    args = ap.parse_args()
    if args.op_trace:
        return op_trace(args.op_trace, W=args.width)
    import constrain_ref as CR
    from faceformer_amd.hip import lib as L
    model, plain, T = setup()
    lines = plain(1)["input"].size(1)
    batch, _, _ = CR.lattice_batch([110], lines, T, 1)
    batch["label"] = torch.zeros((1, T), dtype=torch.int64)
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    with torch.no_grad():
        eng, memory, mask, kv_len = model._encode(b)
        ni = torch.tensor(batch["num_input"], dtype=torch.int32).cuda()
        table = model._follow_table(b, memory.device, ni, None)
    common = dict(T=T, F=1, chunk_wireframes=model.chunk_wireframes, chunk_seqs=model.chunk_seqs, chunk_max_seqs=model.chunk_max_seqs,
                  num_streams=model.num_streams, sync_every=1, x3_min_rows=model.x3_min_rows, ln_fuse_max_rows=model.ln_fuse_max_rows,
                  tok_sos=model.token.SOS, tok_eos=model.token.EOS, flags=model.decode_flags)
    con = lambda form: dict(sequence_constrain=form, tok_sep=model.token.SEP, follow_table=table)
    decode = lambda kw: eng.decode(memory, mask, kv_len, L.FF_SEQ2SEQ, **dict(common, **kw))
    timing, greedy = {}, {}
    for form in ("loops", "coedge_loops"):
        with torch.no_grad():
            mean, mn, spread, out = time_call(lambda: decode(con(form)), args.calls)
        greedy[form] = (mean, out["steps"], float(out["logprob"].double().sum()))
        timing["greedy " + form] = {"ms": mean, "ms_min": mn, "ms_spread": spread, "steps": out["steps"], "ms_per_step": mean / max(out["steps"], 1),
                                    "score": greedy[form][2]}
        print("greedy %-13s             %8.2f ms (min %.2f, spread %.2f)  %3d steps  %.3f ms/step  score %.3f" % (
            form, mean, mn, spread, out["steps"], mean / max(out["steps"], 1), greedy[form][2]), flush=True)
    for W in args.widths:
        forms = [("sequence_beams", "all", dict(sequence_beams=W))]
        for stop in ("all", "best") if args.best else ("all",):
            forms += [(form, stop, dict(sequence_constrain_beams=W, sequence_beam_stop=stop, **con(form))) for form in ("loops", "coedge_loops")]
        base = None
        for name, stop, kw in forms:
            with torch.no_grad():
                mean, mn, spread, out = time_call(lambda: decode(kw), args.calls)
            steps = out["steps"]
            row = {"W": W, "stop": stop, "ms": mean, "ms_min": mn, "ms_spread": spread, "steps": steps, "ms_per_step": mean / max(steps, 1),
                   "beam0_score": float(out["beam_scores"][0]), "finished": int((out["beam_finished"] != 0).sum())}
            note = "beam 0 score %.3f; finished %d of %d" % (row["beam0_score"], row["finished"], W)
            if name == "sequence_beams":
                base = (mean, steps)
            else:
                row["dead_ends"], row["open_end"] = int(out["beam_dead_end"].sum()), int(out["beam_open_end"].sum())
                row["ms_per_step_vs_sequence_beams"] = (mean / max(steps, 1)) / (base[0] / max(base[1], 1))
                gm, gs, gsc = greedy[name]
                row["ms_per_step_vs_greedy"] = (mean / max(steps, 1)) / (gm / max(gs, 1))
                note += "; greedy row's score %.3f; per step %.3fx sequence_beams, %.3fx the greedy decode" % (
                    gsc, row["ms_per_step_vs_sequence_beams"], row["ms_per_step_vs_greedy"])
                if steps == base[1]:
                    row["ratio_to_sequence_beams"] = mean / base[0]
                    note += "; whole decode %.3fx sequence_beams" % row["ratio_to_sequence_beams"]
                else:
                    note += "; steps differ: no whole-decode ratio"
            timing["W=%d %s %s" % (W, name, stop)] = row
            print("W=%d %-14s %-4s %8.2f ms (min %.2f, spread %.2f)  %3d steps  %.3f ms/step  %s" % (
                W, name, stop, mean, mn, spread, steps, mean / max(steps, 1), note), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_constrain_beam.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
