"""Which seeds tests/test_sample.py may use.

Operator half: which seeded rows the operator test may use: the sampling rule of tests/sample_ref.py in fp64 on the CPU,
applied to the test's own seeded rows (the masked fp32 logits are inputs, so the GPU is not needed to know them).  Prints, per
case (one key count S and one parameter set: all its batch sizes and logit kinds), the share of rows whose draw or top-p cut is
indecisive -- inside the guard band, where an fp32 evaluation may legitimately take the neighbouring key -- and exits non-zero
when a case is above sample_ref.CAP.  A seed is changed, never the cap.

Engine half: which (golden, seed, parameter set) triples the replay test may use.  The fp32 oracle (oracle/refpath.py, forced=)
samples its own paths on the CPU: at every step it is forced along the tokens drawn so far, the fp64 rule is applied to its
masked fp32 logits with the seeded uniforms of sample_ref.make_uniforms, and the drawn token is appended.  Counted: the share
of (step, unfinished row) pairs that are indecisive.  Every row runs to its own finish position or T - 1 steps (the batch's
stop step is not applied: a superset of the pairs a decode makes).  A triple is kept only when the share is below the cap.

    python tools/sample_left_out.py [--operator [S ...]] [--engine [golden ...]]        (default: both, everything)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sample_ref as SR  # noqa: E402
import test_sample as TS  # noqa: E402


def oracle_step_logits(case, sd32, b32, paths, step, seqs, F):
    """[rows', S] masked fp32 logits (as fp64 numpy) of step `step` of the oracle forced along `paths`."""
    import torch
    from oracle import refpath
    tr = {}
    refpath.parallel_forward_eval(sd32, dict(b32), num_head=case["model"]["H"], trace=tr, forced=torch.from_numpy(paths), steps=step + 1,
                                  seqs=None if seqs is None else torch.as_tensor(seqs), num_anchors=F)
    lg = tr["logits"][step].double().numpy()
    return np.where(lg > SR.FILL, lg, SR.FILL)


def engine(names):
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    tok = token_ns()
    term, ntok = (tok.face_type_offset, tok.len), tok.len
    worst = 0.0
    for name in names:
        case, _ = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
        b32 = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
        ni = [int(n) for n in batch["num_input"]]
        N, F, T, R = len(ni), max(ni), case["model"]["seq_len"], SR.REPLAY_R
        seed = SR.REPLAY_SEEDS[name]
        u = SR.make_uniforms(ni, T, R, seed).numpy()
        seqs = SR.SUBSET.get(name)
        rows = np.array(seqs if seqs is not None else range(N * F))
        for tau, K, P in SR.REPLAY_PARAMS:
            pairs = left = 0
            for k in range(R):
                paths = np.zeros((N * F, T), dtype=np.int64)
                f = np.arange(N * F) % F
                paths[:, 0] = np.where(f < np.repeat(ni, F), f, ntok - 1)
                fin = (paths[:, 0] >= term[0]) & (paths[:, 0] < term[1])
                for s in range(T - 1):
                    if fin[rows].all():
                        break
                    lg = oracle_step_logits(case, sd32, b32, paths, s, seqs, F)
                    for i, r in enumerate(rows):
                        if fin[r]:
                            continue
                        res = SR.sample_row(lg[i], u[s, r * R + k], tau, K, P)
                        pairs, left = pairs + 1, left + (not res["decisive"])
                        paths[r, s + 1] = res["tok"]
                        fin[r] = term[0] <= res["tok"] < term[1]
            share = left / max(1, pairs)
            worst = max(worst, share)
            print("%s seed %d R=%d tau=%g K=%d P=%g: %d of %d pairs indecisive (%.2f %%, cap %.0f %%)%s"
                  % (name, seed, R, tau, K, P, left, pairs, 100 * share, 100 * SR.CAP, "  <-- above the cap" if share >= SR.CAP else ""),
                  flush=True)
    return worst


def operator(sizes):
    worst = 0.0
    for S in sizes or [1, 5, 63, 64, 65, 260, 1028]:
        for pi, (tau, K, P) in enumerate(TS.PARAMS):
            K = S + 3 if K == "S+3" else K
            seen = left = 0
            for B in (1, 3, 4, 9):
                for kind in ("g1", "g30", "u1e4"):
                    logits, u, row_id, fin, memory, mask, kv, dead = TS._operator_case(B, S, kind, 1000 * S + 10 * B + pi)
                    own = logits.masked_fill(dead, SR.FILL).numpy().astype(np.float64)
                    _, _, dec, _ = SR.sample_rows(own, u.numpy()[row_id.long().numpy()], tau, K, P, fin=fin.numpy())
                    seen, left = seen + B, left + int((~dec).sum())
            share = left / seen
            worst = max(worst, share)
            print("S=%d tau=%g K=%d P=%g: %d of %d rows indecisive (%.2f %%, cap %.0f %%)%s"
                  % (S, tau, K, P, left, seen, 100 * share, 100 * SR.CAP, "  <-- above the cap" if share > SR.CAP else ""), flush=True)
    return worst


def main():
    args = sys.argv[1:]
    both = not args
    worst = 0.0
    if both or "--operator" in args:
        i = args.index("--operator") + 1 if "--operator" in args else 0
        vals = []
        while i and i < len(args) and not args[i].startswith("--"):
            vals.append(int(args[i]))
            i += 1
        worst = max(worst, operator(vals))
    if both or "--engine" in args:
        i = args.index("--engine") + 1 if "--engine" in args else 0
        vals = []
        while i and i < len(args) and not args[i].startswith("--"):
            vals.append(args[i])
            i += 1
        worst = max(worst, engine(vals or list(SR.REPLAY_SEEDS)))
    sys.exit(1 if worst > SR.CAP else 0)


if __name__ == "__main__":
    main()
