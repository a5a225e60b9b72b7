"""Cost and yield of the opt-in closure look-ahead of the constrained decode (the parallel model's constrain_lookahead,
ff_decode_constrained_ahead): whole-decode ms of the config B-shaped LATTICE wireframe (256 connected co-edges,
tests/constrain_ref.py) under constrain = "loops" with the look-ahead, beside the "loops" decode of the same input in the same
process, package default and f32.  The two decodes may stop at different steps, so the per-step figures are the ones to compare.
Both times include building the follow table on the device, the look-ahead's also the two distance tables, as a model call
does; the table build (ops.follow_distance) is also timed alone.  Also printed: enclosed / dead-ended / other own-anchor rows of
both decodes (synthetic weights: this says nothing about trained yield).

    python tools/bench_lookahead.py [--steps 5] [--forms default,f32] [--out profiles/lookahead]
    python tools/bench_lookahead.py --yield-only        (the three lattice goldens and config B: the yield table alone)

For the kernels' own cost run one form per process under a kernel trace and read the mean duration of
pointer_constrained_kernel<true> next to <false>, and follow_distance_kernel:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_lookahead.py --forms default --no-write
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constrain_ref as CR  # noqa: E402
from bench_beam import setup  # noqa: E402
from bench_logprob import time_decode  # noqa: E402
from faceformer_amd import faces  # noqa: E402


def row_yield(pred, dead, ni, edges, token):
    """Own-anchor rows enclosed / dead-ended / other: pred [N, F, T], dead [N, F]."""
    enc = de = other = 0
    lo, hi = token.face_type_offset, token.len
    for w, n in enumerate(ni):
        for f in range(n):
            row = pred[w, f]
            face = faces._parallel_rows(row[None], token, n)
            if dead[w, f]:
                de += 1
            elif ((row >= lo) & (row < hi)).any() and face and faces.is_face_enclosed(edges[w], face[0][1], CR.TOL):
                enc += 1
            else:
                other += 1
    return {"enclosed": enc, "dead_end": de, "other": other, "rows": int(sum(ni))}


def decode_yield(model, batch, ni, edges, look):
    model.constrain, model.constrain_lookahead = "loops", look
    try:
        with torch.no_grad():
            out = model(dict(batch))
    finally:
        model.constrain, model.constrain_lookahead = None, False
    return row_yield(out["predict"].cpu().numpy(), out["predict_dead_end"].cpu().numpy() != 0, ni, edges, model.token)


def yield_table():
    from conftest import batch_to, build_model, case_weights_and_batch, load_golden
    table = {}
    for name in ("par_small_gain4", "par_small_ragged", "par_full_n40_gain4"):
        case, _ = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        m = case["model"]
        lat, edges, _ = CR.lattice_batch(batch["num_input"], m["L"], m["seq_len"], CR.LATTICE_SEEDS[name])
        model = build_model(case, sd, "cuda")
        table[name] = {key: decode_yield(model, batch_to(lat, "cuda"), lat["num_input"], edges, look)
                       for key, look in (("loops", False), ("lookahead", True))}
        print(name, table[name], flush=True)
    return table


def time_tables(model, batch, T, steps):
    """ms of ops.follow_distance alone on the batch's follow table (hmax = max(T - 2, 1)), mean of `steps` calls."""
    from faceformer_amd.hip import ops
    ni = torch.tensor(batch["num_input"], dtype=torch.int32).cuda()
    bits = model._follow_table(batch, torch.device("cuda"), batch["num_input"], None)
    ops.follow_distance(bits, ni, max(T - 2, 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ops.follow_distance(bits, ni, max(T - 2, 1))
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookahead"))
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--yield-only", action="store_true", help="the yield table of the lattice fixtures, no timing")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    model, _ = setup()
    T = model.max_face_length
    lat, edges, _ = CR.lattice_batch([256], 256, T, args.seed)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}
    result = {}
    if args.yield_only:
        result["yield"] = yield_table()
        result["yield"]["config_b_lattice"] = {key: decode_yield(model, batch, [256], edges, look)
                                               for key, look in (("loops", False), ("lookahead", True))}
        print("config_b_lattice (T = %d)" % T, result["yield"]["config_b_lattice"], flush=True)
    else:
        x3 = model.x3_min_rows
        for form in args.forms.split(","):
            model.x3_min_rows = 0 if form == "f32" else x3
            row = {}
            for key, look in (("loops", False), ("lookahead", True)):
                model.constrain, model.constrain_lookahead = "loops", look
                ms, ms_min, spread, out = time_decode(model, batch, args.steps)
                steps = model.last_decode_stats["steps"]
                model.constrain, model.constrain_lookahead = None, False
                row[key] = {"ms": ms, "ms_min": ms_min, "ms_spread": spread, "steps": steps, "ms_per_step": ms / max(steps, 1)}
                row[key].update(row_yield(out["predict"].cpu().numpy(), out["predict_dead_end"].cpu().numpy() != 0, [256], edges,
                                          model.token))
            row["follow_distance_ms"] = time_tables(model, batch, T, args.steps)
            row["ratio_per_step"] = row["lookahead"]["ms_per_step"] / row["loops"]["ms_per_step"]
            result[form] = row
            print(form, "look-ahead %.2f ms (%d steps, %.3f ms/step) | loops %.2f ms (%d steps, %.3f ms/step) | per-step ratio %.3f | "
                  "table build alone %.3f ms | look-ahead %s | loops %s"
                  % (row["lookahead"]["ms"], row["lookahead"]["steps"], row["lookahead"]["ms_per_step"], row["loops"]["ms"],
                     row["loops"]["steps"], row["loops"]["ms_per_step"], row["ratio_per_step"], row["follow_distance_ms"],
                     {k: row["lookahead"][k] for k in ("enclosed", "dead_end", "other")},
                     {k: row["loops"][k] for k in ("enclosed", "dead_end", "other")}), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "yield.json" if args.yield_only else "bench_lookahead.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
