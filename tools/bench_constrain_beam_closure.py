"""Cost and yield of the closure look-ahead in the constrained beam search (the parallel model's constrain_beam_closure,
ff_decode_constrained_beam_ahead): ms per decode step of the config B-shaped LATTICE wireframe (256 connected
co-edges, tests/constrain_ref.py) under constrain = "loops" with W = 1, 2, 4, 8 beams per anchor, "lookahead" and "exact", beside
the plain constrain_beams decode at the same W in the same process -- the yardstick: the same launch with the plain rule.  The
decodes stop at different steps, so the per-step figures are the ones to compare.  Every time includes building the follow table
and, with the option on, the distance tables on the device, as a model call does.  Shapes are warmed up; median of --steps runs
with min .. max.  Also printed per W and form: the own-anchor groups whose best non-dead beam is enclosed (synthetic weights: this
says nothing about trained yield).

    python tools/bench_constrain_beam_closure.py [--steps 7] [--widths 1,2,4,8] [--forms default,f32]
    python tools/bench_constrain_beam_closure.py --yield-only     (the three lattice goldens and config B at W = 1, 4, 8: the yield table alone)

For the kernel's own cost run one setting per process under a kernel trace and read the mean duration of
beam_constrained_select_kernel<W, FORM> (FORM 0 plain, 1 look-ahead, 2 exact):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_constrain_beam_closure.py --widths 8 --forms default --no-write
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
from bench_beam import setup  # noqa: E402
from faceformer_amd import faces  # noqa: E402

CLOSURES = (None, "lookahead", "exact")


def time_decode(model, batch, steps):
    """(median ms, min ms, max ms, the last call's output dict) of `steps` timed calls behind one warm-up call."""
    def run():
        with torch.no_grad():
            return model(dict(batch))
    out = run()                                    # warm-up (binds the engine, splits the planes)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), min(ms), max(ms), out


def best_beam_yield(beams, scores, dead, ni, edges, token):
    """Own-anchor groups by their best non-empty, non-dead beam: beams [N, F, W, T], scores / dead [N, F, W], in rank order."""
    enc = none = 0
    lo, hi = token.face_type_offset, token.len
    for w, n in enumerate(ni):
        for f in range(n):
            live = [k for k in range(beams.shape[2]) if not np.isinf(scores[w, f, k]) and not dead[w, f, k]]
            if not live:
                none += 1
                continue
            row = beams[w, f, live[0]]
            face = faces._parallel_rows(row[None], token, n)
            ends = ((row >= lo) & (row < hi)).any()
            enc += bool(ends and face and faces.is_face_enclosed(edges[w], face[0][1], CR.TOL))
    return {"best_enclosed": enc, "only_dead_end": none, "groups": int(sum(ni))}


def _set(model, W, closure):
    model.constrain, model.constrain_beams, model.constrain_beam_closure = ("loops", W, closure) if W else (None, 0, None)


def decode_yield(model, batch, ni, edges, W, closure):
    _set(model, W, closure)
    try:
        with torch.no_grad():
            out = model(dict(batch))
    finally:
        _set(model, 0, None)
    return best_beam_yield(out["predict_beams"].cpu().numpy(), out["predict_beam_scores"].cpu().numpy(),
                           out["predict_beam_dead_end"].cpu().numpy() != 0, ni, edges, model.token)


def yield_table(widths, model_b, batch_b, edges_b):
    from conftest import batch_to, build_model, case_weights_and_batch, load_golden
    table = {}
    fixtures = []
    for name in ("par_small_gain4", "par_small_ragged", "par_full_n40_gain4"):
        case, _ = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        m = case["model"]
        lat, edges, _ = CR.lattice_batch(batch["num_input"], m["L"], m["seq_len"], CR.LATTICE_SEEDS[name])
        fixtures.append((name, build_model(case, sd, "cuda"), batch_to(lat, "cuda"), lat["num_input"], edges))
    fixtures.append(("config_b_lattice", model_b, batch_b, [256], edges_b))
    for name, model, batch, ni, edges in fixtures:
        for W in widths:
            row = {str(c or "plain"): decode_yield(model, batch, ni, edges, W, c) for c in CLOSURES}
            table.setdefault(name, {})["W%d" % W] = row
            print(name, "W=%d" % W, {k: "%d / %d" % (v["best_enclosed"], v["groups"]) for k, v in row.items()}, flush=True)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_beam_closure"))
    ap.add_argument("--widths", default=None)
    ap.add_argument("--forms", default="default,f32", help="comma list: default (the package's split products), f32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--yield-only", action="store_true", help="the yield table of the lattice fixtures, no timing")
    ap.add_argument("--no-write", action="store_true", help="print only (a kernel trace of one setting)")
    args = ap.parse_args()
    widths = [int(w) for w in (args.widths or ("1,4,8" if args.yield_only else "1,2,4,8")).split(",")]
    model, _ = setup()
    T = model.max_face_length
    lat, edges, _ = CR.lattice_batch([256], 256, T, args.seed)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}
    os.makedirs(args.out, exist_ok=True)
    if args.yield_only:
        table = yield_table(widths, model, batch, edges)
        if not args.no_write:
            path = os.path.join(args.out, "yield.json")
            doc = json.load(open(path)) if os.path.exists(path) else {}
            doc["yield"] = table
            json.dump(doc, open(path, "w"), indent=1)
        return
    result, x3 = {}, model.x3_min_rows
    for form in args.forms.split(","):
        model.x3_min_rows = 0 if form == "f32" else x3
        for W in widths:
            row = {}
            for closure in CLOSURES:
                _set(model, W, closure)
                ms, lo, hi, out = time_decode(model, batch, args.steps)
                steps = model.last_decode_stats["steps"]
                y = best_beam_yield(out["predict_beams"].cpu().numpy(), out["predict_beam_scores"].cpu().numpy(),
                                    out["predict_beam_dead_end"].cpu().numpy() != 0, [256], edges, model.token)
                row[str(closure or "plain")] = dict(ms=ms, ms_min=lo, ms_max=hi, steps=steps, ms_per_step=ms / max(steps, 1), **y)
            _set(model, 0, None)
            for c in ("lookahead", "exact"):
                row[c]["ratio_per_step"] = row[c]["ms_per_step"] / row["plain"]["ms_per_step"]
            result.setdefault(form, {})["W%d" % W] = row
            print(form, "W=%d" % W, " | ".join("%s %.2f ms (%.2f .. %.2f), %d steps, %.3f ms/step%s, best enclosed %d / %d"
                  % (c, r["ms"], r["ms_min"], r["ms_max"], r["steps"], r["ms_per_step"], (" (x %.3f)" % r["ratio_per_step"]) if "ratio_per_step" in r else "",
                     r["best_enclosed"], r["groups"]) for c, r in row.items()), flush=True)
    model.x3_min_rows = x3
    if not args.no_write:
        with open(os.path.join(args.out, "bench_constrain_beam_closure.json"), "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
