"""Cost of teacher-forced scoring (the models' score(), ff_decode_forced): whole-call ms of scoring every row of
config B (one 256-edge wireframe: 256 rows x T-1 steps) and C128 (128 of them) over all T-1 positions, in the package default and
in f32, beside the greedy decode of the same shapes with FF_NO_STOP -- which makes the same launches apart from the pointer step
(and plans its micro-batches with padding-anchor de-duplication, which changes nothing when every wireframe has F edges).  The
scored paths are that greedy decode's own tokens.

    python tools/bench_forced.py [--steps 5] [--only B] [--forms default,f32] [--out profiles/forced]

For the kernel's own cost run one setting per process under a kernel trace and compare the mean duration of
pointer_forced_kernel with pointer_reduce_kernel<true> (tools/bench_logprob.py --modes on):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_forced.py --only B --forms default --no-write
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_logprob import time_decode, workloads  # noqa: E402


def time_score(model, batch, paths, lengths, steps):
    """(mean ms, min ms, spread of the timed calls, the last call's output dict)"""
    out = model.score(dict(batch), paths, lengths)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = model.score(dict(batch), paths, lengths)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return sum(ms) / len(ms), min(ms), max(ms) - min(ms), out


def main():
    from faceformer_amd.hip import lib as L
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forced"))
    ap.add_argument("--only", default="", help="comma list of workloads (B, C128)")
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else None
    timing = {}
    for name, ctor, sd, batch in workloads():
        if only and name not in only:
            continue
        b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
        model = ctor()
        model.load_state_dict(sd)
        model = model.eval().cuda()
        model.decode_flags |= L.FF_NO_STOP
        x3 = model.x3_min_rows
        T = model.max_face_length
        for form in args.forms.split(","):
            model.x3_min_rows = 0 if form == "f32" else x3
            gm, gmin, gspread, out = time_decode(model, b, args.steps)
            paths = out["predict"]
            lengths = torch.full(tuple(paths.shape[:2]), T - 1, dtype=torch.int64)
            sm, smin, sspread, sc = time_score(model, b, paths, lengths, args.steps)
            row = {"greedy_no_stop_ms": gm, "greedy_no_stop_ms_min": gmin, "greedy_no_stop_ms_spread": gspread,
                   "score_ms": sm, "score_ms_min": smin, "score_ms_spread": sspread, "ratio": sm / gm,
                   "rows": int(paths.shape[0] * paths.shape[1]), "steps": model.last_score_stats["steps"],
                   "rank0_share": float((sc["score_rank"][..., 1:] == 0).float().mean())}
            timing.setdefault(name, {})[form] = row
            print(name, form, "greedy (FF_NO_STOP) %.2f ms | score %.2f ms | ratio %.3f | %d rows x %d steps, rank 0 at %.1f %%"
                  % (gm, sm, row["ratio"], row["rows"], row["steps"], 100 * row["rank0_share"]), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_forced.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
