"""Cost of the opt-in loop-constrained decode of the single-sequence model (SurfaceFormer.sequence_constrain,
ff_decode_sequence_constrained) on the config A shape: configs/seq2seq.yml (num_lines 110, label_seq_length 259), ONE
110-edge lattice wireframe (tests/constrain_ref.lattice_batch: connected co-edges, so that "loops" has loops to close), gain-4
synthetic weights.  Whole-decode ms by device events around PathEngine.decode (the encoder runs once, outside), for four forms:

  greedy        the greedy decode with logprob=True and FF_STOP_EACH_EOS: the yardstick, which exists without the option
  bits clear    sequence_constrain = 0: the same tokens and steps, so the ratio is the launch's cost
  loops         sequence_constrain = "loops"
  coedge_loops  sequence_constrain = "coedge_loops"

`steps` and ms per step are printed for every form; a ratio to the yardstick only where the step counts are equal.

    python tools/bench_sequence_constrain.py [--calls 3] [--out profiles/sequence_constrain]

--op-trace N: instead of the decodes, N launches each of ops.pointer_argmax (logprob form: the pointer GEMM and
pointer_reduce_kernel) and of ops.pointer_sequence_constrained under "coedge_loops" on the SAME rows -- one wireframe, S = 114 keys,
E = 512 -- so that a kernel trace shows the two selection launches' mean durations side by side:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sequence_constrain.py --op-trace 200
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

from bench_sequence_sample import setup  # noqa: E402


def op_trace(n, B=1, S=114, E=512, ntok=4):
    import numpy as np
    import constrain_ref as CR
    from faceformer_amd import faces
    from faceformer_amd.hip import ops
    g = torch.Generator().manual_seed(0)
    L = S - ntok
    p, memory = torch.randn(B, E, generator=g).cuda(), torch.randn(1, S, E, generator=g).cuda()
    mask = torch.zeros(1, S, dtype=torch.uint8).cuda()
    table = torch.from_numpy(faces.pack_follow_bits(CR.random_follows(1, L, 1))).cuda()
    fin = torch.zeros(B, dtype=torch.int32).cuda()
    first, prev = torch.full((B,), 3, dtype=torch.int32).cuda(), torch.full((B,), 5, dtype=torch.int32).cuda()      # an open loop
    visited = torch.from_numpy(np.array([[0x28] + [0] * ((L + 31) // 32 - 1)] * B, dtype=np.int32)).cuda()
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    for _ in range(n):
        ref = ops.pointer_argmax(p, memory, mask, seqs_per_group=B, want_logits=True, want_rows=True, want_logprob=True)
        ops.pointer_sequence_constrained(ref["logits"], fin, first, prev, visited, 7, ntok, 2, 3, follows=table, memory=memory, mask=mask,
                                         seqs_per_group=B, want_rows=True, want_stats=True, counter=counter)
    torch.cuda.synchronize()
    print("op trace: %d launches of each selection, B=%d S=%d E=%d" % (n, B, S, E))


def time_call(call, calls):
    """(mean ms, min ms, spread, the last output) of `calls` timed calls after one warm-up, by device events."""
    out = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sum(ms) / len(ms), min(ms), max(ms) - min(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="timed calls per form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_constrain"))
    ap.add_argument("--no-write", action="store_true", help="print only")
    ap.add_argument("--op-trace", type=int, default=0, metavar="N", help="N launches of each selection on one shape; no decode")
    args = ap.parse_args()
    if args.op_trace:
        return op_trace(args.op_trace)
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
                  tok_sos=model.token.SOS, tok_eos=model.token.EOS)
    forms = [("greedy", dict(flags=model.decode_flags | L.FF_STOP_EACH_EOS, logprob=True)),
             ("bits clear", dict(flags=model.decode_flags, sequence_constrain=0, tok_sep=model.token.SEP)),
             ("loops", dict(flags=model.decode_flags, sequence_constrain="loops", tok_sep=model.token.SEP, follow_table=table)),
             ("coedge_loops", dict(flags=model.decode_flags, sequence_constrain="coedge_loops", tok_sep=model.token.SEP, follow_table=table))]
    timing, base = {}, None
    for name, kw in forms:
        with torch.no_grad():
            mean, mn, spread, out = time_call(lambda: eng.decode(memory, mask, kv_len, L.FF_SEQ2SEQ, **dict(common, **kw)), args.calls)
        steps = out["steps"]
        row = {"ms": mean, "ms_min": mn, "ms_spread": spread, "steps": steps, "ms_per_step": mean / max(steps, 1)}
        if "dead_end" in out:
            row["dead_ends"], row["open_end"] = int(out["dead_end"].sum()), int(out["open_end"].sum())
            row["eos"] = bool((out["predict"] == model.token.EOS).any())
        if base is None:
            base = (mean, steps)
        elif steps == base[1]:
            row["ratio_to_greedy"] = mean / base[0]
        timing[name] = row
        print("%-13s %8.2f ms (min %.2f, spread %.2f)  %3d steps  %.3f ms/step  %s" % (
            name, mean, mn, spread, steps, mean / max(steps, 1),
            ("ratio to the greedy decode %.3f" % row["ratio_to_greedy"]) if "ratio_to_greedy" in row else
            ("" if name == "greedy" else "steps differ: no ratio")), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_constrain.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
