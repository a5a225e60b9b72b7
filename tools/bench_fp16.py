"""Time the three decode forms -- f32 (every product on the f32 matrix cores), the package default (fp16x2 split products) and the
opt-in one-fp16-product kind "fp16" -- on config B (one 256-edge wireframe), C128 (128 of them) and seq2seq A64 (one 64-edge
wireframe, gain-4 weights), and the fp16 GEMM next to fp16x2 on the decode's projection shapes (TF/s fp32-equivalent, as
profiles/r06/gemm_split_kinds.txt).  Also writes the per-workload token / sequence agreement of the 16-bit forms with f32.

    python tools/bench_fp16.py [--steps 3] [--out profiles/fp16]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = {"f32": dict(x3_min_rows=0), "default": dict(split_kind="fp16x2"), "fp16": dict(split_kind="fp16")}


def workloads():
    from faceformer_amd.config import load_cfg
    from faceformer_amd.models import SurfaceFormer, SurfaceFormer_Parallel
    from faceformer_amd.synth import make_state_dict, make_wireframes, state_dict_spec
    cfg = load_cfg(os.path.join(ROOT, "configs", "ours.yml"), ["model.num_lines", "256"])
    T = cfg.model.max_face_length
    spec = state_dict_spec("parallel", 256, T, cfg.model.num_model, cfg.model.num_feedforward,
                           cfg.model.num_encoder_layers, cfg.model.num_decoder_layers)
    sd_p = make_state_dict(spec, "default", 0)
    for name, n in (("B", 1), ("C128", 128)):
        yield name, (lambda: SurfaceFormer_Parallel(**cfg.model)), sd_p, make_wireframes([256] * n, 256, T, seeds=list(range(n)))
    c1 = load_cfg(os.path.join(ROOT, "configs", "seq2seq.yml"))
    L1, T1 = c1.model.num_lines, c1.model.label_seq_length
    sd_s = make_state_dict(state_dict_spec("seq2seq", L1, T1), "gain4", 0)
    yield "A64", (lambda: SurfaceFormer(**c1.model)), sd_s, make_wireframes([64], L1, T1, "seq2seq", seeds=[3])


def time_decode(model, batch, steps):
    def run():
        with torch.no_grad():
            return model(dict(batch))["predict"]
    pred = run()                                   # warm-up (binds the engine, splits the planes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        pred = run()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, pred.cpu()


def gemm_rows(steps=20):
    """fp32-equivalent TF/s of ff_gemm_x2h and ff_gemm_h1 (plain form) on the decode's shapes."""
    from faceformer_amd.hip import ops
    out = []
    for M, N, K in ((9216, 1536, 512), (9216, 1024, 512), (9216, 512, 1024), (9216, 512, 512), (4608, 1536, 512),
                    (4608, 512, 512), (2304, 512, 512), (32768, 1536, 512), (32768, 512, 1024)):
        a = torch.randn(M, K, device="cuda")
        w = torch.randn(N, K, device="cuda") / K ** 0.5
        row = {"M": M, "N": N, "K": K}
        for kind in ("fp16x2", "fp16"):
            pl = ops.split_weight(w, kind)
            c = torch.empty(M, N, device="cuda")
            for _ in range(3):
                ops.linear_x3(a, pl, out=c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ops.linear_x3(a, pl, out=c)
            torch.cuda.synchronize()
            sec = (time.perf_counter() - t0) / steps
            row[kind + "_us"] = 1e6 * sec
            row[kind + "_tfs"] = 2.0 * M * N * K / sec / 1e12
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp16"))
    ap.add_argument("--only", default="", help="comma list of workloads (B, C128, A64)")
    ap.add_argument("--forms", default="f32,default,fp16", help="comma list of forms (f32, default, fp16); agreement needs f32")
    ap.add_argument("--no-gemm", action="store_true", help="skip the GEMM rows (e.g. a kernel trace of the decode alone)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    timing, agree = {}, []
    only = set(args.only.split(",")) if args.only else None
    for name, ctor, sd, batch in workloads():
        if only and name not in only:
            continue
        b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
        preds = {}
        for form, attrs in FORMS.items():
            if form not in args.forms.split(","):
                continue
            model = ctor()
            model.load_state_dict(sd)
            model = model.eval().cuda()
            for k, v in attrs.items():
                setattr(model, k, v)
            ms, preds[form] = time_decode(model, b, args.steps if name != "C128" else 1)
            timing.setdefault(name, {})[form] = {"ms": ms, "split_kind_bound": model.engine().split_kind}
            print(name, form, "%.2f ms" % ms, flush=True)
            del model
            torch.cuda.empty_cache()
        ref = preds.get("f32")
        for form in ("default", "fp16"):
            if ref is None or form not in preds:
                continue
            p = preds[form]
            T = p.shape[-1]
            same_tok = float((p.reshape(-1, T) == ref.reshape(-1, T)).float().mean())
            same_seq = float((p.reshape(-1, T) == ref.reshape(-1, T)).all(dim=1).float().mean())
            line = "%-5s %-8s tokens equal to f32: %.5f  sequences equal: %.4f" % (name, form, same_tok, same_seq)
            agree.append(line)
            print(line, flush=True)
    with open(os.path.join(args.out, "bench_fp16.json"), "w") as f:
        json.dump(timing, f, indent=1)
    if agree:
        with open(os.path.join(args.out, "agreement.txt"), "w") as f:
            f.write("# token / sequence agreement of the 16-bit forms with the f32 form on the same inputs (tools/bench_fp16.py)\n")
            f.write("\n".join(agree) + "\n")
    if args.no_gemm:
        return
    rows = gemm_rows()
    with open(os.path.join(args.out, "gemm_split_kinds.txt"), "w") as f:
        f.write("# ff_gemm_x2h (fp16x2) vs ff_gemm_h1 (fp16): us per launch and fp32-equivalent TF/s, random operands\n")
        for r in rows:
            f.write("M=%5d N=%4d K=%4d  fp16x2 %8.1f us %6.1f TF/s   fp16 %8.1f us %6.1f TF/s   x%.2f\n" % (
                r["M"], r["N"], r["K"], r["fp16x2_us"], r["fp16x2_tfs"], r["fp16_us"], r["fp16_tfs"], r["fp16x2_us"] / r["fp16_us"]))
    print(open(os.path.join(args.out, "gemm_split_kinds.txt")).read())


if __name__ == "__main__":
    main()
