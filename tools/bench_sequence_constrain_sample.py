"""Cost of the opt-in sampling over the loop-constrained single-sequence decode (SurfaceFormer.sequence_constrain_samples,
ff_decode_sequence_constrained_sample) on the config A shape: configs/seq2seq.yml (num_lines 110, label_seq_length
259), ONE 110-edge lattice wireframe (tests/constrain_ref.lattice_batch), gain-4 synthetic weights, tau = 1.  Whole-decode ms by
device events around PathEngine.decode (the encoder runs once, outside), 3 timed calls after a warm-up, for R = 1 / 4 / 16 / 64:

  sequence_samples = R      the unconstrained draws: the decode that exists without the option
  loops / coedge_loops      sequence_constrain with sequence_constrain_samples = R
  R x greedy                R separate sequence_constrain decodes of the same form, one after the other (R x the measured one)

`steps` and ms per step are printed for every form; a whole-decode ratio only where the step counts are equal.

    python tools/bench_sequence_constrain_sample.py [--calls 3] [--out profiles/sequence_constrain_sample]

--op-trace N: instead of the decodes, N launches each of ops.pointer_sequence_sample (pointer_sample_kernel<true>), of
ops.pointer_sequence_constrained and of ops.pointer_sequence_constrained_sample under "coedge_loops" on the SAME rows -- one
wireframe, B rows (--rows, default 16), S = 114 keys, E = 512 -- so that a kernel trace shows the three selection launches' mean
durations side by side:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sequence_constrain_sample.py --op-trace 200
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


def op_trace(n, B=16, S=114, E=512, ntok=4):
    import numpy as np
    import constrain_ref as CR
    from faceformer_amd import faces
    from faceformer_amd.hip import ops
    g = torch.Generator().manual_seed(0)
    L = S - ntok
    raw, memory = (torch.randn(B, S, generator=g) * 3).cuda(), torch.randn(1, S, E, generator=g).cuda()
    mask = torch.zeros(1, S, dtype=torch.uint8).cuda()
    table = torch.from_numpy(faces.pack_follow_bits(CR.random_follows(1, L, 1))).cuda()
    fin = torch.zeros(B, dtype=torch.int32).cuda()
    first, prev = torch.full((B,), 3, dtype=torch.int32).cuda(), torch.full((B,), 5, dtype=torch.int32).cuda()      # an open loop
    visited = torch.from_numpy(np.array([[0x28] + [0] * ((L + 31) // 32 - 1)] * B, dtype=np.int32)).cuda()
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    u = torch.rand(B, generator=g).cuda()
    kw = dict(memory=memory, mask=mask, seqs_per_group=B, want_rows=True, want_stats=True, counter=counter)
    for _ in range(n):
        ops.pointer_sequence_sample(raw.clone(), u, 1.0, 0, 1.0, fin=fin, term_range=(3, 4), **kw)
        ops.pointer_sequence_constrained(raw.clone(), fin, first, prev, visited, 7, ntok, 2, 3, follows=table, **kw)
        ops.pointer_sequence_constrained_sample(raw.clone(), u, fin, first, prev, visited, 7, ntok, 2, 3, follows=table, **kw)
    torch.cuda.synchronize()
    print("op trace: %d launches of each selection, B=%d S=%d E=%d" % (n, B, S, E))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="timed calls per form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_constrain_sample"))
    ap.add_argument("--no-write", action="store_true", help="print only")
    ap.add_argument("--op-trace", type=int, default=0, metavar="N", help="N launches of each selection on one shape; no decode")
    ap.add_argument("--rows", type=int, default=16, help="launch rows of the op trace")
    ap.add_argument("--draws", type=int, nargs="*", default=[1, 4, 16, 64])
    args = ap.parse_args()
    if args.op_trace:
        return op_trace(args.op_trace, B=args.rows)
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
    timing = {}
    greedy = {}
    for form in ("loops", "coedge_loops"):
        with torch.no_grad():
            mean, mn, spread, out = time_call(lambda: decode(con(form)), args.calls)
        greedy[form] = (mean, out["steps"])
        timing["greedy " + form] = {"ms": mean, "ms_min": mn, "ms_spread": spread, "steps": out["steps"], "ms_per_step": mean / max(out["steps"], 1)}
        print("greedy %-13s        %8.2f ms (min %.2f, spread %.2f)  %3d steps  %.3f ms/step" % (
            form, mean, mn, spread, out["steps"], mean / max(out["steps"], 1)), flush=True)
    for R in args.draws:
        u = torch.rand((T - 1, R), generator=torch.Generator().manual_seed(5)).cuda()
        draw = dict(temperature=1.0, top_k=0, top_p=1.0, uniforms=u)
        forms = [("sequence_samples", dict(draw, sequence_samples=R))] + \
                [(form, dict(draw, sequence_constrain_samples=R, **con(form))) for form in ("loops", "coedge_loops")]
        base = None
        for name, kw in forms:
            with torch.no_grad():
                mean, mn, spread, out = time_call(lambda: decode(kw), args.calls)
            steps = out["steps"]
            row = {"R": R, "ms": mean, "ms_min": mn, "ms_spread": spread, "steps": steps, "ms_per_step": mean / max(steps, 1)}
            note = ""
            if name == "sequence_samples":
                base = (mean, steps)
            else:
                row["dead_ends"], row["open_end"] = int(out["sample_dead_end"].sum()), int(out["sample_open_end"].sum())
                row["draws_at_eos"] = int((out["samples"] == model.token.EOS).any(dim=1).sum())
                row["ms_per_step_vs_sequence_samples"] = (mean / max(steps, 1)) / (base[0] / max(base[1], 1))
                gm, gs = greedy[name]
                row["ms_R_greedy_decodes"] = R * gm
                row["ms_per_step_vs_greedy"] = (mean / max(steps, 1)) / (gm / max(gs, 1))
                note = "per step %.3fx sequence_samples, %.3fx one greedy decode; R greedy decodes %.1f ms (%d steps each)" % (
                    row["ms_per_step_vs_sequence_samples"], row["ms_per_step_vs_greedy"], R * gm, gs)
                if steps == base[1]:
                    row["ratio_to_sequence_samples"] = mean / base[0]
                    note += "; whole decode %.3fx sequence_samples" % row["ratio_to_sequence_samples"]
                else:
                    note += "; steps differ: no whole-decode ratio"
                note += "; draws at EOS %d of %d" % (row["draws_at_eos"], R)
            timing["R=%d %s" % (R, name)] = row
            print("R=%-2d %-17s %8.2f ms (min %.2f, spread %.2f)  %3d steps  %.3f ms/step  %s" % (
                R, name, mean, mn, spread, steps, mean / max(steps, 1), note), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_constrain_sample.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
