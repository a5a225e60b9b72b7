"""Which (golden, seed) pairs tests/test_forced.py may use: the fp32 oracle against the fp64 oracle on the CPU, teacher-forced
along the seeded paths of tests/forced_ref.py.  Prints, per golden, the share of scored (row, position) pairs that leave the
greedy / rank comparison (the truth's top-2 margin, or another logit's distance from the forced one, is within 2 tol) -- it must
stay below forced_ref.CAP -- and the fp32 oracle's worst logit and log-probability error in units of the test's bars.

A seed is kept only when the share is below the cap AND the fp32 oracle itself stays inside both bars (one fp32 evaluation in
several hundred rows of these goldens lands just outside tol: tests/test_oracle_forced.py); the script exits non-zero otherwise.

    python tools/forced_left_out.py [golden[:seed] ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forced_ref as FR  # noqa: E402
from conftest import case_weights_and_batch, load_golden  # noqa: E402
from oracle import refpath  # noqa: E402


def oracle_logits(case, sd, batch, paths, steps, seqs, dtype, device="cpu"):
    """[steps, rows', S] masked logits of the oracle forced along `paths` (rows' = seqs or every row), in fp64 numpy."""
    sd = {k: (v.to(device, dtype) if v.is_floating_point() else v.to(device)) for k, v in sd.items()}
    b = {k: (v.to(device, dtype if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v) for k, v in batch.items()}
    fn = refpath.parallel_forward_eval if case["kind"] == "parallel" else refpath.seq2seq_forward_eval
    tr = {}
    fn(sd, b, num_head=case["model"]["H"], trace=tr, forced=torch.from_numpy(paths).to(device), steps=steps,
       seqs=None if seqs is None else torch.as_tensor(seqs, device=device))
    return torch.stack(tr["logits"]).double().cpu().numpy()


def main():
    for arg in sys.argv[1:] or list(FR.SEEDS):
        name, _, seed = arg.partition(":")
        seed = int(seed) if seed else FR.SEEDS[name]
        case, _ = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        paths, lengths, F = FR.make_paths(case, seed)
        rows = FR.SUBSET.get(name) or list(range(paths.shape[0]))
        steps = int(lengths[rows].max())
        seqs = FR.SUBSET.get(name)
        truth = oracle_logits(case, sd, batch, paths, steps, seqs, torch.float64)
        f32 = oracle_logits(case, sd, batch, paths, steps, seqs, torch.float32)
        B, T = paths.shape
        S = truth.shape[-1]
        lg = np.full((steps, B, S), np.nan)
        lp, gr, rk = np.zeros((B, T)), np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
        for s in range(steps):
            lg[s, rows] = np.where(f32[s] > FR.FILL32, f32[s], FR.FILL32)
            a, b_, c = FR.forced_rule(lg[s, rows], paths[rows, s + 1])
            lp[rows, s + 1], gr[rows, s + 1], rk[rows, s + 1] = a, b_, c
        st = FR.compare(truth, rows, paths, lengths, lg, lp, gr, rk, what=name, check=False)
        print("%s seed %d: %d scored pairs, left out %.2f %% (cap %.0f %%), fp32 oracle worst |dlogit| / tol = %.3f, "
              "|dlogprob| / bar = %.3f" % (name, seed, st["pairs"], 100 * st["left_out"], 100 * FR.CAP, st["worst_logit"],
                                            st["worst_lp"]), flush=True)
        assert st["left_out"] < FR.CAP and st["worst_logit"] <= 1.0 and st["worst_lp"] <= 1.0, arg


if __name__ == "__main__":
    main()
