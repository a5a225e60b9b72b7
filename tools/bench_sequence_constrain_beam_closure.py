"""Cost and yield of the opt-in closure look-ahead of the sequence-constrained beam search
(SurfaceFormer.sequence_constrain_beam_closure, ff_sequence_decode_constrained_beam_ahead) on the config A shape:
configs/seq2seq.yml (num_lines 110, label_seq_length 259), ONE 110-edge lattice wireframe (tests/constrain_ref.lattice_batch),
gain-4 synthetic weights.  Whole-decode ms by device events around PathEngine.decode (the encoder runs once, outside), 3 timed
calls after a warm-up, per flags ("loops", "coedge_loops") and W = 1 / 2 / 4 / 8, in ONE process:

  plain                     sequence_constrain_beams = W: the decode that exists without the option
  lookahead / exact         the option; the tables are built (ops.follow_distance, hmax 254) INSIDE the timed call

Printed per form: ms, steps, ms per step, the per-step ratio to the plain decode (a whole-decode ratio only where the step counts
agree), and the yield over beam 0 and over all non-empty beams: rows at EOS, enclosed / parsed faces, dead ends, late dead ends,
open ends.  The weights are synthetic: no threshold is set on the yield.

    python tools/bench_sequence_constrain_beam_closure.py [--calls 3] [--out profiles/sequence_constrain_beam_closure]

--op-trace N: instead of the decodes, N launches each of ops.beam_sequence_constrained_select and of both forms of
ops.beam_sequence_constrained_select_ahead under "coedge_loops" on the SAME rows -- one wireframe, W open beams (--width, default
8), S = 114 keys, E = 512, budget 200 -- so that a kernel trace shows the three selection launches' mean durations side by side:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sequence_constrain_beam_closure.py --op-trace 200
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


def op_trace(n, W=8, S=114, E=512, ntok=4, budget=200):
    import numpy as np
    import constrain_ref as CR
    from faceformer_amd import faces
    from faceformer_amd.hip import ops
    g = torch.Generator().manual_seed(0)
    L = S - ntok
    raw, memory = (torch.randn(W, S, generator=g) * 3).cuda(), torch.randn(1, S, E, generator=g).cuda()
    mask = torch.zeros(1, S, dtype=torch.uint8).cuda()
    follows = CR.random_follows(1, L, 1)
    table = torch.from_numpy(faces.pack_follow_bits(follows)).cuda()
    cd, cl = (torch.from_numpy(t).cuda() for t in faces.follow_distance(follows, 254))
    fin = torch.zeros(W, dtype=torch.int32).cuda()
    scores = -torch.arange(W, dtype=torch.float32).cuda()
    first, prev = torch.full((W,), 3, dtype=torch.int32).cuda(), torch.full((W,), 5, dtype=torch.int32).cuda()      # open loops
    visited = torch.from_numpy(np.array([[0x28] + [0] * ((L + 31) // 32 - 1)] * W, dtype=np.int32)).cuda()
    counter = torch.zeros(1, dtype=torch.int32).cuda()
    kw = dict(memory=memory, mask=mask, groups_per_wireframe=1, want_rows=True, want_stats=True, counter=counter)
    for _ in range(n):
        ops.beam_sequence_constrained_select(raw.clone(), scores, fin, first, prev, visited, W, 7, ntok, 2, 3, follows=table, **kw)
        for form in ("lookahead", "exact"):
            ops.beam_sequence_constrained_select_ahead(raw.clone(), scores, fin, first, prev, visited, W, 7, ntok, 2, 3, table, form, cl, budget,
                                                       close_dist=cd, **kw)
    torch.cuda.synchronize()
    print("op trace: %d launches of each of the three selections, W=%d S=%d E=%d budget=%d" % (n, W, S, E, budget))


def yield_of(out, W, ni, flags, tok, follows, edges):
    """{beam 0 / all: rows at EOS, enclosed, parsed, dead ends, late dead ends, open ends} over the non-empty final beams."""
    import numpy as np
    import sequence_constrain_beam_closure_ref as BC
    import sequence_constrain_beam_ref as CB
    bm, sc, de, oe, fin = (out[k].cpu().numpy() for k in ("beams", "beam_scores", "beam_dead_end", "beam_open_end", "beam_finished"))
    res = {}
    for name, rows in (("beam0", np.arange(0, bm.shape[0], W)), ("all", np.flatnonzero(np.isfinite(sc)))):
        enc = par = dead = 0
        for r in rows:
            e, p, d = CB.guarantee(bm[r:r + 1], de[r:r + 1], oe[r:r + 1], sc[r:r + 1], 1, [ni[r // W]], flags, tok.len, tok.SEP, tok.EOS,
                                   [follows[r // W]], None if edges is None else [edges[r // W]])
            enc, par, dead = enc + e, par + p, dead + d
        late = [x for x in BC.late_dead_ends(bm, de, flags, tok.len, tok.SEP, follows, W) if x[0] in set(rows.tolist())]
        res[name] = dict(rows=int(len(rows)), at_eos=int((fin[rows] != 0).sum()), enclosed=int(enc), parsed=int(par), dead_ends=int(dead),
                         late_dead_ends=len(late), open_ends=int(oe[rows].sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3, help="timed calls per form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_constrain_beam_closure"))
    ap.add_argument("--no-write", action="store_true", help="print only")
    ap.add_argument("--op-trace", type=int, default=0, metavar="N", help="N launches of each selection on one shape; no decode")
    ap.add_argument("--width", type=int, default=8, help="beams of the op trace")
    ap.add_argument("--widths", type=int, nargs="*", default=[1, 2, 4, 8])
    args = ap.parse_args()
    if args.op_trace:
        return op_trace(args.op_trace, W=args.width)
    import constrain_ref as CR
    from faceformer_amd import faces
    from faceformer_amd.hip import lib as L, modes, ops
    model, plain, T = setup()
    lines = plain(1)["input"].size(1)
    batch, edges, _ = CR.lattice_batch([110], lines, T, 1)
    batch["label"] = torch.zeros((1, T), dtype=torch.int64)
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    with torch.no_grad():
        eng, memory, mask, kv_len = model._encode(b)
        ni = torch.tensor(batch["num_input"], dtype=torch.int32).cuda()
        table = model._follow_table(b, memory.device, ni, None)
    follows = faces.follow_table(batch["input"].numpy(), float(model.constrain_tol), batch["num_input"])
    common = dict(T=T, F=1, chunk_wireframes=model.chunk_wireframes, chunk_seqs=model.chunk_seqs, chunk_max_seqs=model.chunk_max_seqs,
                  num_streams=model.num_streams, sync_every=1, x3_min_rows=model.x3_min_rows, ln_fuse_max_rows=model.ln_fuse_max_rows,
                  tok_sos=model.token.SOS, tok_eos=model.token.EOS, flags=model.decode_flags)
    hmax = min(max(T - 2, 1), 254)

    def decode(mode, W, form):
        kw = dict(common, sequence_constrain=mode, tok_sep=model.token.SEP, follow_table=table, sequence_constrain_beams=W)
        if form is not None:      # (the table build is part of the option's cost)
            cd, cl = ops.follow_distance(table, ni, hmax)
            kw.update(sequence_constrain_beam_closure=form, cycle_len=cl, **({} if form == "exact" else dict(close_dist=cd)))
        return eng.decode(memory, mask, kv_len, L.FF_SEQ2SEQ, **kw)
    record = {}
    for mode in ("loops", "coedge_loops"):
        flags = modes.sequence_constrain_flags(mode)
        for W in args.widths:
            base = None
            for form in (None, "lookahead", "exact"):
                with torch.no_grad():
                    mean, mn, spread, out = time_call(lambda: decode(mode, W, form), args.calls)
                steps = out["steps"]
                row = {"ms": mean, "ms_min": mn, "ms_spread": spread, "steps": steps, "ms_per_step": mean / max(steps, 1),
                       "beam0_score": float(out["beam_scores"][0]), "yield": yield_of(out, W, batch["num_input"], flags, model.token, follows, edges)}
                note = ""
                if form is None:
                    base = (mean, steps)
                else:
                    row["ms_per_step_vs_plain"] = row["ms_per_step"] / (base[0] / max(base[1], 1))
                    note = "per step %.3fx plain" % row["ms_per_step_vs_plain"]
                    if steps == base[1]:
                        row["ratio_to_plain"] = mean / base[0]
                        note += "; whole decode %.3fx plain" % row["ratio_to_plain"]
                    else:
                        note += "; steps differ: no whole-decode ratio"
                record["%s W=%d %s" % (mode, W, form or "plain")] = row
                y = row["yield"]
                print("%-12s W=%d %-9s %8.2f ms (min %.2f, spread %.2f)  %3d steps  %.3f ms/step  %s" % (
                    mode, W, form or "plain", mean, mn, spread, steps, row["ms_per_step"], note), flush=True)
                for name in ("beam0", "all"):
                    print("    %-5s rows %d at EOS %d; enclosed %d of %d parsed; dead ends %d (late %d); open ends %d" % (
                        name, y[name]["rows"], y[name]["at_eos"], y[name]["enclosed"], y[name]["parsed"], y[name]["dead_ends"],
                        y[name]["late_dead_ends"], y[name]["open_ends"]), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_constrain_beam_closure.json"), "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
