"""Cost of the opt-in log-probabilities (models' return_logprob, ff_decode_lp): whole-decode ms of the package default with the
option off and on, on config B (one 256-edge wireframe) and C128 (128 of them).

    python tools/bench_logprob.py [--steps 5] [--only B] [--modes off,on] [--out profiles/logprob]

For the kernel's own cost run one setting per process under a kernel trace and compare the mean duration of
pointer_reduce_kernel<false> / <true>:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_logprob.py --only B --modes on --no-write
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workloads():
    from faceformer_amd.config import load_cfg
    from faceformer_amd.models import SurfaceFormer_Parallel
    from faceformer_amd.synth import make_state_dict, make_wireframes, state_dict_spec
    cfg = load_cfg(os.path.join(ROOT, "configs", "ours.yml"), ["model.num_lines", "256"])
    T = cfg.model.max_face_length
    spec = state_dict_spec("parallel", 256, T, cfg.model.num_model, cfg.model.num_feedforward,
                           cfg.model.num_encoder_layers, cfg.model.num_decoder_layers)
    sd = make_state_dict(spec, "default", 0)
    for name, n in (("B", 1), ("C128", 128)):
        yield name, (lambda: SurfaceFormer_Parallel(**cfg.model)), sd, make_wireframes([256] * n, 256, T, seeds=list(range(n)))


def time_decode(model, batch, steps):
    """(mean ms, min ms, spread of the timed calls, the last call's output dict)"""
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
    return sum(ms) / len(ms), min(ms), max(ms) - min(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logprob"))
    ap.add_argument("--only", default="", help="comma list of workloads (B, C128)")
    ap.add_argument("--modes", default="off,on", help="comma list of settings (off, on)")
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
        preds = {}
        for mode in args.modes.split(","):
            model.return_logprob = mode == "on"
            mean, best, spread, out = time_decode(model, b, args.steps if name != "C128" else max(1, args.steps // 2))
            preds[mode] = out["predict"].cpu()
            row = {"ms": mean, "ms_min": best, "ms_spread": spread, "steps": model.last_decode_stats["steps"]}
            if mode == "on":
                lp = out["predict_logprob"]
                row["mean_logprob_of_kept_selections"] = float(lp.sum() / (lp != 0).sum().clamp(min=1))
            timing.setdefault(name, {})[mode] = row
            print(name, "return_logprob", mode, "%.2f ms (min %.2f, spread %.2f)" % (mean, best, spread), flush=True)
        if len(preds) == 2:
            assert torch.equal(preds["off"], preds["on"]), "the option changed the tokens"
        del model
        torch.cuda.empty_cache()
    if not args.no_write:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bench_logprob.json"), "w") as f:
            json.dump(timing, f, indent=1)


if __name__ == "__main__":
    main()
