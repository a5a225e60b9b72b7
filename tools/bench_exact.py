"""Cost and yield of the opt-in exact closure look-ahead of the constrained decode (the parallel model's constrain_exact,
ff_decode_constrained_exact): whole-decode ms of the config B-shaped LATTICE wireframe (256 connected co-edges,
tests/constrain_ref.py) under constrain = "loops" with the exact look-ahead, beside the constrain_lookahead decode of the same
input in the same process, package default and f32.  The two decodes may stop at different steps, so the per-step figures are the
ones to compare.  Both times include building the follow table and the distance tables on the device, as a model call does.
Also printed: enclosed / dead-ended / other own-anchor rows and the late dead ends of both decodes (synthetic weights: this says
nothing about trained yield).

    python tools/bench_exact.py [--steps 5] [--forms default,f32] [--out profiles/exact]
    python tools/bench_exact.py --yield-only        (the three lattice goldens and config B: the yield table alone)
    python tools/bench_exact.py --worst-case        (the operator alone at L = 1024, S = 1028, budget 35: every level runs; host-timed)

For the kernels' own cost run one form per process under a kernel trace and read the mean duration of
pointer_constrained_form_kernel<2> next to <1>:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_exact.py --forms default --no-write
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constrain_ref as CR  # noqa: E402
import exact_ref as ER  # noqa: E402
from bench_beam import setup  # noqa: E402
from bench_logprob import time_decode  # noqa: E402
from bench_lookahead import row_yield  # noqa: E402
from faceformer_amd import faces  # noqa: E402

OPTIONS = (("loops", {}), ("lookahead", {"constrain_lookahead": True}), ("exact", {"constrain_exact": True}))


def _set(model, constrain, opts):
    model.constrain = constrain
    model.constrain_lookahead = bool(opts.get("constrain_lookahead"))
    model.constrain_exact = bool(opts.get("constrain_exact"))


def rows_of(out, ni, edges, table, token):
    """row_yield plus the late dead ends (exact_ref.late_dead_ends) of the own-anchor rows: pred [N, F, T], dead [N, F]."""
    pred, dead = out["predict"].cpu().numpy(), out["predict_dead_end"].cpu().numpy() != 0
    res = row_yield(pred, dead, ni, edges, token)
    late = 0
    for w, n in enumerate(ni):
        own = dead[w].copy()
        own[n:] = False
        late += len(ER.late_dead_ends(pred[w], own, token.len, table[w]))
    res["late_dead_ends"] = late
    return res


def decode_yield(model, batch, ni, edges, table, opts):
    _set(model, "loops", opts)
    try:
        with torch.no_grad():
            out = model(dict(batch))
    finally:
        _set(model, None, {})
    return rows_of(out, ni, edges, table, model.token)


def yield_table():
    from conftest import batch_to, build_model, case_weights_and_batch, load_golden
    table = {}
    for name in ("par_small_gain4", "par_small_ragged", "par_full_n40_gain4"):
        case, _ = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        m = case["model"]
        lat, edges, _ = CR.lattice_batch(batch["num_input"], m["L"], m["seq_len"], ER.LATTICE_SEEDS[name])
        follows = faces.follow_table(lat["input"].numpy(), CR.TOL, lat["num_input"])
        model = build_model(case, sd, "cuda")
        table[name] = {key: decode_yield(model, batch_to(lat, "cuda"), lat["num_input"], edges, follows, opts) for key, opts in OPTIONS}
        print(name, table[name], flush=True)
    return table


def worst_case(steps):
    """Host-timed ms per ops call (call and launch overhead included: take the kernels' own durations from a kernel trace of this
    mode) of the two look-ahead operators alone at L = 1024 (S = 1028), 256 open rows of one ring of all edges, budget 35: no
    candidate is within reach, so the search runs all 35 levels."""
    from faceformer_amd.hip import ops
    L, ntok, B, budget = 1024, 4, 256, 35
    table = np.zeros((1, L, L), dtype=bool)
    table[0, np.arange(L), (np.arange(L) + 1) % L] = True
    bits = torch.from_numpy(faces.pack_follow_bits(table)).cuda()
    close, cyc = ops.follow_distance(bits, torch.tensor([L], dtype=torch.int32).cuda(), 254)
    first = torch.arange(B, dtype=torch.int32) * 4
    prev = first + 1
    vis = np.zeros((B, L), dtype=bool)
    vis[np.arange(B), first.numpy()] = vis[np.arange(B), prev.numpy()] = True
    state = [torch.zeros(B, dtype=torch.int32).cuda(), first.cuda(), prev.cuda(), torch.from_numpy(faces.pack_follow_bits(vis)).cuda()]
    logits = torch.randn(B, L + ntok, generator=torch.Generator().manual_seed(1)).cuda()
    res = {}
    for key, call in (("lookahead", lambda lg: ops.pointer_constrained_ahead(lg, *state, 3, ntok, bits, close, cyc, budget, seqs_per_group=B)),
                      ("exact", lambda lg: ops.pointer_constrained_exact(lg, *state, 3, ntok, bits, cyc, budget, seqs_per_group=B))):
        copies = [logits.clone() for _ in range(steps + 1)]
        out = call(copies[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for lg in copies[1:]:
            call(lg)
        torch.cuda.synchronize()
        res[key] = {"host_ms_per_call": 1e3 * (time.perf_counter() - t0) / steps, "dead_ends": int(out["dead_end"].sum()), "rows": B}
    res["shape"] = {"L": L, "S": L + ntok, "rows": B, "budget": budget, "levels": budget}
    print("worst case", res, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact"))
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--yield-only", action="store_true", help="the yield table of the lattice fixtures, no timing")
    ap.add_argument("--worst-case", action="store_true", help="the operator alone at L = 1024, budget 35")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    result, name = {}, "bench_exact.json"
    if args.worst_case:
        result, name = worst_case(max(args.steps, 20)), "worst_case.json"
    else:
        model, _ = setup()
        T = model.max_face_length
        lat, edges, _ = CR.lattice_batch([256], 256, T, args.seed)
        follows = faces.follow_table(lat["input"].numpy(), CR.TOL, [256])
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}
    if args.yield_only:
        name = "yield.json"
        result["yield"] = yield_table()
        result["yield"]["config_b_lattice"] = {key: decode_yield(model, batch, [256], edges, follows, opts) for key, opts in OPTIONS}
        print("config_b_lattice (T = %d)" % T, result["yield"]["config_b_lattice"], flush=True)
    elif not args.worst_case:
        x3 = model.x3_min_rows
        for form in args.forms.split(","):
            model.x3_min_rows = 0 if form == "f32" else x3
            row = {}
            for key, opts in OPTIONS[1:]:
                _set(model, "loops", opts)
                ms, ms_min, spread, out = time_decode(model, batch, args.steps)
                steps = model.last_decode_stats["steps"]
                _set(model, None, {})
                row[key] = {"ms": ms, "ms_min": ms_min, "ms_spread": spread, "steps": steps, "ms_per_step": ms / max(steps, 1)}
                row[key].update(rows_of(out, [256], edges, follows, model.token))
            row["ratio_per_step"] = row["exact"]["ms_per_step"] / row["lookahead"]["ms_per_step"]
            result[form] = row
            print(form, "exact %.2f ms (%d steps, %.3f ms/step) | look-ahead %.2f ms (%d steps, %.3f ms/step) | per-step ratio %.3f | "
                  "exact %s | look-ahead %s"
                  % (row["exact"]["ms"], row["exact"]["steps"], row["exact"]["ms_per_step"], row["lookahead"]["ms"],
                     row["lookahead"]["steps"], row["lookahead"]["ms_per_step"], row["ratio_per_step"],
                     {k: row["exact"][k] for k in ("enclosed", "dead_end", "other", "late_dead_ends")},
                     {k: row["lookahead"][k] for k in ("enclosed", "dead_end", "other", "late_dead_ends")}), flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, name), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
