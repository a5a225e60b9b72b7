"""Cost of the opt-in device-side face extraction (ops.face_rows + ops.face_votes) beside the two things it stands
next to, on the config B-shaped LATTICE wireframe (256 connected co-edges, tests/constrain_ref.lattice_batch; F = 256 anchors)
under constrain = "loops" with R = 1 (the constrained greedy decode), 4 and 64 draws per anchor (constrain_samples):

    (a) the two launches on the rows the decode published, with the enclosure walk on the decode's follow table;
    (b) the host path on the same rows: the device-to-host copy of tokens, scores and dead-end flags, then
        faces.parse_parallel_constrained_samples_scored + faces.unique_faces_with_scores (no enclosure walk: less work than (a));
    (c) the decode of that batch, option off.

(a) and (c) are timed with device events, (b) with the host clock around work that ends synchronised; every shape is warmed up
first, and every figure is the median of --reps runs with min and max beside it.  Prints a/b and a/c and writes
profiles/faces/bench_faces.json / .txt.

    python tools/bench_faces.py [--reps 7] [--samples 1,4,64] [--out profiles/faces]
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
from faceformer_amd import faces  # noqa: E402
from faceformer_amd.hip import ops  # noqa: E402


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def host_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", default="1,4,64")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faces"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    model, _ = setup()
    T = model.max_face_length
    lat, _, _ = CR.lattice_batch([256], 256, T, args.seed)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in lat.items()}
    ni = torch.tensor([256], dtype=torch.int32).cuda()
    model.sample_temperature, model.sample_top_k, model.sample_top_p, model.sample_seed = 1.0, 0, 1.0, 5
    model.constrain = "loops"
    table = model._follow_table(batch, ni.device, [256], None)
    result, lines = {"T": T, "F": 256, "L": 256, "reps": args.reps}, []
    for R in (int(r) for r in args.samples.split(",")):
        model.constrain_samples = R if R > 1 else 0

        def decode():
            with torch.no_grad():
                return model(dict(batch))
        out = decode()
        if R > 1:
            tokens, scores, dead = out["predict_samples"], out["predict_sample_scores"], out["predict_sample_dead_end"]
            kw = dict(scores=scores, dead_end=dead)
        else:
            tokens, scores, dead = out["predict"].unsqueeze(2), out["predict_logprob"].unsqueeze(2), out["predict_dead_end"].unsqueeze(2)
            kw = dict(logprob=scores, own_stop=True)

        def device_path():
            rows = ops.face_rows(tokens, ni, model.token, follows=table, **kw)
            rows.update(ops.face_votes(rows, require_closed=True))
            return rows

        def host_path():
            t, s, d = tokens.cpu().numpy(), scores.cpu().numpy(), dead.cpu().numpy()
            return faces.unique_faces_with_scores(faces.parse_parallel_constrained_samples_scored(t[0], s[0], d[0], 256, model.token))
        a = device_ms(device_path, args.reps)
        b = host_ms(host_path, max(3, args.reps // 2) if R >= 64 else args.reps)
        c = device_ms(decode, args.reps)
        found = device_path()
        cell = {"rows": 256 * R, "device_ms": a, "host_ms": b, "decode_ms": c, "steps": model.last_decode_stats["steps"],
                "a_over_b": {"median": a["median"] / b["median"], "min": a["min"] / b["max"], "max": a["max"] / b["min"]},
                "a_over_c": {"median": a["median"] / c["median"], "min": a["min"] / c["max"], "max": a["max"] / c["min"]},
                "faces_with_edges": int((found["len"] > 0).sum()), "closed_rows": int((found["closed"] == 1).sum()),
                "unique_closed_faces": int(found["num_faces"].sum()), "host_unique_faces": len(host_path())}
        result["R%d" % R] = cell
        lines.append("R=%-3d rows %5d | (a) device %.3f ms [%.3f .. %.3f] | (b) host %.2f ms [%.2f .. %.2f] | (c) decode %.2f ms [%.2f .. %.2f] "
                     "(%d steps) | a/b %.4f [%.4f .. %.4f] | a/c %.4f [%.4f .. %.4f] | rows with a face %d, closed %d, unique closed %d"
                     % (R, cell["rows"], a["median"], a["min"], a["max"], b["median"], b["min"], b["max"], c["median"], c["min"], c["max"],
                        cell["steps"], cell["a_over_b"]["median"], cell["a_over_b"]["min"], cell["a_over_b"]["max"],
                        cell["a_over_c"]["median"], cell["a_over_c"]["min"], cell["a_over_c"]["max"], cell["faces_with_edges"],
                        cell["closed_rows"], cell["unique_closed_faces"]))
        print(lines[-1], flush=True)
    model.constrain, model.constrain_samples = None, 0
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_faces.json"), "w") as f:
            json.dump(result, f, indent=1)
        with open(os.path.join(args.out, "bench_faces.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
