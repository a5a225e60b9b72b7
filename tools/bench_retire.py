"""Default decode vs finished-loop retirement (SurfaceFormer_Parallel.retire_finished) on the 'stagger' weights,
whose face loops end at staggered steps: 1 x 256 and 16 x 256 edges, f32 matrix cores only and the package default.

Prints ONE JSON line: per (size, form) the median ms of both modes, slot_rows of both (decoder rows computed) and whether the
retired tokens equal faces.retired_view of the default decode's.  Usage: python tools/bench_retire.py [--reps 5] [--sizes 1,16]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from faceformer_amd import faces, synth            # noqa: E402
from faceformer_amd.models import SurfaceFormer_Parallel  # noqa: E402
from faceformer_amd.models.common import X3_MIN_ROWS_DEFAULT  # noqa: E402

TOKEN = types.SimpleNamespace(PAD=0, SOS=1, SEP=2, EOS=3, DIR0=4, DIR1=5, len=4, face_type_offset=1)


def build(L=256, T=37):
    m = SurfaceFormer_Parallel(num_model=512, num_head=8, num_feedforward=1024, num_encoder_layers=6, num_decoder_layers=6,
                               num_lines=L, max_face_length=T, token=TOKEN)
    m.load_state_dict(synth.make_state_dict(synth.state_dict_spec("parallel", L, T, 512, 1024, 6, 6), "stagger", 0))
    return m.eval().cuda()


def timed(model, batch, reps):
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model(dict(batch))["predict"]
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out.cpu().numpy(), dict(model.last_decode_stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,16")
    args = ap.parse_args()
    model = build()
    res = {"recipe": "stagger", "edges_per_wireframe": 256, "T": 37, "reps": args.reps, "runs": []}
    for n in [int(x) for x in args.sizes.split(",")]:
        batch = synth.make_wireframes(256, 256, 37, "parallel", seeds=list(range(n)))
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
        for form, x3 in (("f32", 0), ("package default", X3_MIN_ROWS_DEFAULT)):
            model.x3_min_rows = x3
            model.retire_finished = False
            timed(model, batch, 1)                           # warm-up (workspace, planes)
            ms0, p0, st0 = timed(model, batch, args.reps)
            model.retire_finished = True
            timed(model, batch, 1)
            ms1, p1, st1 = timed(model, batch, args.reps)
            model.retire_finished = False
            res["runs"].append({"wireframes": n, "form": form, "default_ms": round(ms0, 3), "retire_ms": round(ms1, 3),
                                "speedup": round(ms0 / ms1, 3), "default_slot_rows": st0["slot_rows"],
                                "retire_slot_rows": st1["slot_rows"], "default_steps": st0["steps"], "retire_steps": st1["steps"],
                                "tokens_equal_retired_view": bool(np.array_equal(p1, faces.retired_view(p0, TOKEN)))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
