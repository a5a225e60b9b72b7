"""Cost of the opt-in device-side face extraction of the single-sequence model (ops.face_seq_rows + ops.face_seq_votes, DESIGN.md
31) beside the two things it stands next to, at the config A shape (configs/seq2seq.yml: ONE 110-edge wireframe, T = 259, gain-4
synthetic weights) with R = 1 (the greedy decode with return_logprob), 4, 16 and 64 draws (sequence_samples):

    (a) the two launches on the rows the decode published (no enclosure walk: the host path below has none either);
    (b) the host path on the same rows: the device-to-host copy of tokens and log-probabilities, then
        faces.parse_faces_samples_scored + faces.unique_faces_with_scores;
    (c) the decode of that batch, option off.

(a) and (c) are timed with device events, (b) with the host clock around work that ends synchronised; every shape is warmed up
first, and every figure is the median of --reps runs with min and max beside it.  The synthetic weights never select SEP, so
those rows hold one face each; (a) and (b) are therefore also measured on synthetic rows of about 40 faces each, fed to the two
launches directly ("many faces").  Prints a/b and a/c and writes
profiles/sequence_faces/bench_sequence_faces.json / .txt.

    python tools/bench_sequence_faces.py [--reps 7] [--samples 1,4,16,64] [--out profiles/sequence_faces]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_faces import device_ms, host_ms  # noqa: E402
from bench_sequence_sample import setup  # noqa: E402
from faceformer_amd import faces  # noqa: E402
from faceformer_amd.hip import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", default="1,4,16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_faces"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    model, batch, T = setup()
    b = batch(1)
    L = b["input"].size(1)
    ni = torch.tensor([L], dtype=torch.int32).cuda()
    model.sample_temperature, model.sample_top_k, model.sample_top_p, model.sample_seed = 1.0, 0, 1.0, 5
    result, lines = {"T": T, "L": L, "reps": args.reps}, []
    for R in (int(r) for r in args.samples.split(",")):
        model.sequence_samples, model.return_logprob = (R, False) if R > 1 else (0, True)

        def decode():
            with torch.no_grad():
                return model(dict(b))
        out = decode()
        tokens, lp = (out["predict_samples"], out["predict_sample_logprob"]) if R > 1 else \
            (out["predict"].unsqueeze(1), out["predict_logprob"].unsqueeze(1))

        def device_path():
            rows = ops.face_seq_rows(tokens, ni, model.token, logprob=lp, num_lines=L)
            rows.update(ops.face_seq_votes(rows))
            return rows

        def host_path():
            t, s = tokens.cpu().numpy(), lp.cpu().numpy()
            return faces.unique_faces_with_scores(faces.parse_faces_samples_scored(t[0], s[0], L, model.token))
        a = device_ms(device_path, args.reps)
        h = host_ms(host_path, args.reps)
        c = device_ms(decode, args.reps)
        found = device_path()
        cell = {"rows": R, "device_ms": a, "host_ms": h, "decode_ms": c,
                "a_over_b": {"median": a["median"] / h["median"], "min": a["min"] / h["max"], "max": a["max"] / h["min"]},
                "a_over_c": {"median": a["median"] / c["median"], "min": a["min"] / c["max"], "max": a["max"] / c["min"]},
                "faces": int(found["count"].sum()), "unique_faces": int(found["num_faces"].sum()), "host_unique_faces": len(host_path())}
        result["R%d" % R] = cell
        lines.append("R=%-3d | (a) device %.3f ms [%.3f .. %.3f] | (b) host %.3f ms [%.3f .. %.3f] | (c) decode %.2f ms [%.2f .. %.2f] | "
                     "a/b %.4f [%.4f .. %.4f] | a/c %.5f [%.5f .. %.5f] | faces %d, unique %d (host %d)"
                     % (R, a["median"], a["min"], a["max"], h["median"], h["min"], h["max"], c["median"], c["min"], c["max"],
                        cell["a_over_b"]["median"], cell["a_over_b"]["min"], cell["a_over_b"]["max"], cell["a_over_c"]["median"],
                        cell["a_over_c"]["min"], cell["a_over_c"]["max"], cell["faces"], cell["unique_faces"], cell["host_unique_faces"]))
        print(lines[-1], flush=True)
    model.sequence_samples, model.return_logprob = 0, False
    # The synthetic weights never select SEP, so every decoded row above is ONE face.  The same two paths on rows of the shape a
    # trained model decodes: about 40 faces of 3 .. 8 edges per row, drawn from a pool of 60 faces so that faces recur within a
    # row and across rows, fed to the launches directly (no decode: there is no (c)).
    import numpy as np
    g = np.random.default_rng(5)
    tok = model.token
    pool = [[int(tok.len) + int(e) for e in g.choice(L, size=int(g.integers(3, 9)), replace=False)] for _ in range(60)]
    for R in (int(r) for r in args.samples.split(",")):
        rows_np = np.zeros((1, R, T), dtype=np.int64)
        for r in range(R):
            seq = [int(tok.SOS)]
            while True:
                face = pool[int(g.integers(0, len(pool)))]
                if len(seq) + len(face) + 2 > T:
                    break
                seq += face + [int(tok.SEP)]
            seq[-1] = int(tok.EOS)
            rows_np[0, r, : len(seq)] = seq
        tokens = torch.as_tensor(rows_np).cuda()
        lp = -torch.rand((1, R, T), device="cuda") * (tokens != 0)

        def device_path():
            rows = ops.face_seq_rows(tokens, ni, model.token, logprob=lp, num_lines=L)
            rows.update(ops.face_seq_votes(rows))
            return rows

        def host_path():
            t, s = tokens.cpu().numpy(), lp.cpu().numpy()
            return faces.unique_faces_with_scores(faces.parse_faces_samples_scored(t[0], s[0], L, model.token))
        a = device_ms(device_path, args.reps)
        h = host_ms(host_path, args.reps)
        found = device_path()
        cell = {"rows": R, "device_ms": a, "host_ms": h,
                "a_over_b": {"median": a["median"] / h["median"], "min": a["min"] / h["max"], "max": a["max"] / h["min"]},
                "faces": int(found["count"].sum()), "unique_faces": int(found["num_faces"].sum()), "host_unique_faces": len(host_path())}
        result["many_faces_R%d" % R] = cell
        lines.append("many faces R=%-3d | (a) device %.3f ms [%.3f .. %.3f] | (b) host %.3f ms [%.3f .. %.3f] | a/b %.4f [%.4f .. %.4f] | "
                     "faces %d, unique %d (host %d)" % (R, a["median"], a["min"], a["max"], h["median"], h["min"], h["max"],
                                                        cell["a_over_b"]["median"], cell["a_over_b"]["min"], cell["a_over_b"]["max"],
                                                        cell["faces"], cell["unique_faces"], cell["host_unique_faces"]))
        print(lines[-1], flush=True)
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_sequence_faces.json"), "w") as f:
            json.dump(result, f, indent=1)
        with open(os.path.join(args.out, "bench_sequence_faces.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
