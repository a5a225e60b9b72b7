"""Cost and yield of the opt-in closure look-ahead of the loop-constrained single-sequence decode
(SurfaceFormer.sequence_constrain_closure, ff_sequence_decode_constrained_ahead / _sample_ahead) on the config A
shape: tools/bench_sequence_constrain.py's recipe -- configs/seq2seq.yml (num_lines 110, label_seq_length 259), ONE 110-edge
lattice wireframe, gain-4 SYNTHETIC weights (the counts below say what the rule does on this table, not what a trained model
yields).  Whole-decode ms by device events around PathEngine.decode (the encoder runs once, outside); a closure form's time
INCLUDES the build of its tables (ops.follow_distance) on every call, as the model pays it.  Per flags ("loops",
"coedge_loops"), greedy and R = 16 draws:

  plain      sequence_constrain alone: the yardstick, in the same process
  lookahead  sequence_constrain_closure = "lookahead"
  exact      sequence_constrain_closure = "exact"

Printed per form: ms, steps, ms per step, the ratio of the per-step ms to the plain decode's (and of the whole decode where the
step counts agree), rows at EOS, parsed / enclosed faces, dead ends, late dead ends, open ends.

    python tools/bench_sequence_closure.py [--calls 3] [--out profiles/sequence_closure]

--op-trace N: instead of the decodes, N launches each of ops.pointer_sequence_constrained and of its two closure forms, greedy
and sampled, on the SAME rows -- one wireframe, S = 114 keys, an open loop -- so that a kernel trace shows the launches' mean
durations side by side:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sequence_closure.py --op-trace 200
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
    polys, _ = CR.lattice_edges(L, 1)
    pts = np.array([[p[0][:2], p[-1][:2]] for p in polys], dtype=np.float32)
    bits = torch.from_numpy(faces.pack_follow_bits(faces.follow_table((pts[:, 0], pts[:, 1]), 1e-4)[None])).cuda()
    cd, cl = ops.follow_distance(bits, torch.tensor([L], dtype=torch.int32).cuda(), 254)
    logits, memory = torch.randn(B, S, generator=g).cuda(), torch.randn(1, S, E, generator=g).cuda()
    mask = torch.zeros(1, S, dtype=torch.uint8).cuda()
    fin = torch.zeros(B, dtype=torch.int32).cuda()
    first, prev = torch.full((B,), 3, dtype=torch.int32).cuda(), torch.full((B,), 5, dtype=torch.int32).cuda()      # an open loop
    visited = torch.from_numpy(np.array([[0x28] + [0] * ((L + 31) // 32 - 1)] * B, dtype=np.int32)).cuda()
    u = torch.rand(B, generator=g).cuda()
    kw = dict(memory=memory, mask=mask, seqs_per_group=B, want_rows=True, want_stats=True)
    for _ in range(n):
        ops.pointer_sequence_constrained(logits.clone(), fin, first, prev, visited, 7, ntok, 2, 3, follows=bits, **kw)
        ops.pointer_sequence_constrained_sample(logits.clone(), u, fin, first, prev, visited, 7, ntok, 2, 3, follows=bits, **kw)
        for form in ("lookahead", "exact"):
            ops.pointer_sequence_constrained_ahead(logits.clone(), fin, first, prev, visited, 7, ntok, 2, 3, bits, form, cl, 100,
                                                   close_dist=cd, **kw)
            ops.pointer_sequence_constrained_sample_ahead(logits.clone(), u, fin, first, prev, visited, 7, ntok, 2, 3, bits, form, cl, 100,
                                                          close_dist=cd, **kw)
    torch.cuda.synchronize()
    print("op trace: %d launches of each of the six forms, B=%d S=%d" % (n, B, S))


def counts(out, R, flags, tok, follows, ni):
    """rows at EOS, parsed / enclosed faces (on the table), dead ends, late dead ends, open ends of one decode."""
    import sequence_constrain_closure_ref as QC
    import sequence_constrain_ref as SC
    from sequence_constrain_left_out import walk_closed
    t, dead, oe = (out[k].cpu().numpy() for k in (("samples", "sample_dead_end", "sample_open_end") if R else ("predict", "dead_end", "open_end")))
    enc = par = 0
    for r in range(t.shape[0]):
        for idx, _, _ in SC.face_pieces(t[r], dead[r], tok.len, tok.SEP, tok.EOS, ni[0]):
            par += 1
            enc += bool(walk_closed(idx, follows[0]))
    late = QC.late_dead_ends(t, dead, flags, tok.len, tok.SEP, follows, max(R, 1))
    return dict(rows=int(t.shape[0]), at_eos=int((t == tok.EOS).any(axis=1).sum()), parsed=par, enclosed=enc, dead_ends=int(dead.sum()),
                late_dead_ends=len(late), open_end=int(oe.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="timed calls per form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_closure"))
    ap.add_argument("--no-write", action="store_true", help="print only")
    ap.add_argument("--op-trace", type=int, default=0, metavar="N", help="N launches of each selection on one shape; no decode")
    args = ap.parse_args()
    if args.op_trace:
        return op_trace(args.op_trace)
    import constrain_ref as CR
    from faceformer_amd import faces
    from faceformer_amd.hip import lib as L, ops
    from faceformer_amd.hip.modes import sequence_constrain_flags
    model, plain, T = setup()
    lines = plain(1)["input"].size(1)
    batch, _, _ = CR.lattice_batch([110], lines, T, 1)
    batch["label"] = torch.zeros((1, T), dtype=torch.int64)
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    with torch.no_grad():
        eng, memory, mask, kv_len = model._encode(b)
        ni = torch.tensor(batch["num_input"], dtype=torch.int32).cuda()
        table = model._follow_table(b, memory.device, ni, None)
    follows = faces.follow_table(batch["input"].numpy(), float(model.constrain_tol), batch["num_input"])
    common = dict(T=T, F=1, chunk_wireframes=model.chunk_wireframes, chunk_seqs=model.chunk_seqs, chunk_max_seqs=model.chunk_max_seqs,
                  num_streams=model.num_streams, sync_every=1, x3_min_rows=model.x3_min_rows, ln_fuse_max_rows=model.ln_fuse_max_rows,
                  tok_sos=model.token.SOS, tok_eos=model.token.EOS, flags=model.decode_flags, tok_sep=model.token.SEP, follow_table=table)
    hmax = min(max(T - 2, 1), 254)
    timing = {}
    for R in (0, 16):
        draw = {}
        if R:
            gen = torch.Generator(device="cuda").manual_seed(5)
            draw = dict(sequence_constrain_samples=R, temperature=1.0, top_k=0, top_p=1.0,
                        uniforms=torch.rand((T - 1, R), generator=gen, device="cuda"))
        for name in ("loops", "coedge_loops"):
            base = None
            for form in (None, "lookahead", "exact"):
                def call():
                    kw = dict(common, sequence_constrain=name, **draw)
                    if form is not None:      # (the tables are built inside the timed call)
                        cd, cl = ops.follow_distance(table, ni, hmax)
                        kw.update(sequence_constrain_closure=form, cycle_len=cl, **({} if form == "exact" else dict(close_dist=cd)))
                    return eng.decode(memory, mask, kv_len, L.FF_SEQ2SEQ, **kw)
                with torch.no_grad():
                    mean, mn, spread, out = time_call(call, args.calls)
                steps = out["steps"]
                row = {"ms": mean, "ms_min": mn, "ms_spread": spread, "steps": steps, "ms_per_step": mean / max(steps, 1)}
                row.update(counts(out, R, sequence_constrain_flags(name), model.token, follows, batch["num_input"]))
                if base is None:
                    base = row
                else:
                    row["per_step_ratio_to_plain"] = row["ms_per_step"] / base["ms_per_step"]
                    if steps == base["steps"]:
                        row["ratio_to_plain"] = mean / base["ms"]
                key = "%s%s %s" % (name, " R=%d" % R if R else "", form or "plain")
                timing[key] = row
                print("%-30s %8.2f ms (min %.2f, spread %.2f) %3d steps %.3f ms/step %s| at EOS %d of %d, enclosed %d of %d, dead %d (late %d), "
                      "open %d" % (key, mean, mn, spread, steps, row["ms_per_step"],
                                   ("per-step ratio %.3f%s " % (row["per_step_ratio_to_plain"],
                                                                (", whole %.3f" % row["ratio_to_plain"]) if "ratio_to_plain" in row else ""))
                                   if form else "", row["at_eos"], row["rows"], row["enclosed"], row["parsed"], row["dead_ends"],
                                   row["late_dead_ends"], row["open_end"]), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_closure.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
