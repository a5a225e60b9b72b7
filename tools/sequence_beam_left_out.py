"""Which inputs the tests of tests/test_sequence_beam.py may use.

The 2 % cap on what a comparison against the fp64 rule leaves out is a condition on the test's inputs, not a measurement of the
kernel or the engine.  Two parts, both on the CPU:

  operator   for every (S, W, groups, state) of sequence_beam_ref the rule is applied to the seeded operands in fp64 and in
             fp32-rounded arithmetic; a group is left out when its decisive gap is at most 1 (beam_ref's criterion) or when the
             two arithmetics select differently.  The first seed from op_seed_base() on that leaves out less than the cap is kept;
             printed: OP_SEED_OFFSETS for the ref file (cases that keep their base seed are not listed).
  engine     the fp32 oracle (oracle/refpath.py: seq2seq_forward_eval, forced=) decodes its own beams: at every step it is forced
             along the W prefixes of every wireframe (W rows of its batch, the wireframe repeated), the fp64 rule of
             sequence_beam_ref is applied to its masked fp32 logits and the state carried.  Counted: the (step, group) pairs
             behind a group's first indecisive step (gap <= 1 with margin = step + 1, section 13's scheme), the smallest kept gap,
             the stop step under "all" and under "best", the beams finished at the stop.  Printed: KEPT for the ref file.

    python tools/sequence_beam_left_out.py operator
    python tools/sequence_beam_left_out.py engine [golden ...]      (default: the three small single-sequence goldens, W = 1 2 4 8)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sequence_beam_ref as BR  # noqa: E402

GOLDENS = ("seq_small_gain4", "seq_small_eos", "seq_small_repeat_eos")
WIDTHS = (1, 2, 4, 8)


def operator_left_out(c, eos):
    """Groups of case `c` left out: gap <= 1 under the fp64 rule, or another selection in fp32-rounded arithmetic."""
    masked = BR.masked_of(c)
    W = c["W"]
    ref = BR.step(masked, c["scores"], c["fin"], W, eos)
    par32, tok32 = BR.step_fp32(masked, c["scores"], c["fin"], W, eos)
    same = ((par32 == ref["parent"]) & (tok32 == ref["tok"])).reshape(-1, W).all(axis=1)
    return int(((ref["gap"] <= 1.0) | ~same).sum())


def operator_seeds(eos=3):
    offsets = {}
    for S in BR.OP_S:
        for W in BR.OP_W:
            if W > S:
                continue
            for G in BR.OP_G:
                for state in BR.OP_STATES:
                    base = BR.op_seed_base(S, W, G, state)
                    for off in range(50):
                        left = operator_left_out(BR.operator_case(S, W, G, state, base + off), eos)
                        if left < BR.CAP * G:
                            break
                    else:
                        raise SystemExit("no seed under the cap for %r" % ((S, W, G, state),))
                    if off:
                        offsets[(S, W, G, state)] = off
                    print("S=%d W=%d G=%d %-5s seed %d (+%d): %d of %d groups left out" % (S, W, G, state, base + off, off, left, G), flush=True)
    print("OP_SEED_OFFSETS = %r" % (offsets,))


def oracle_decode(name, W):
    """-> dict(left, pairs, min_gap, steps_all, steps_best, finished) of the fp32 oracle's own beam decode of golden `name`."""
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    from oracle import refpath
    tok = token_ns()
    case, _ = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    N, T = batch["input"].size(0), case["model"]["seq_len"]
    rep = torch.arange(N).repeat_interleave(W)
    b32 = {k: ((v.float() if v.is_floating_point() else v).index_select(0, rep) if torch.is_tensor(v) and v.dim() and v.size(0) == N
               else v) for k, v in batch.items()}

    def step_logits(prefixes, step):
        paths = np.zeros((N * W, T), dtype=np.int64)
        paths[:, : prefixes.shape[1]] = prefixes
        tr = {}
        refpath.seq2seq_forward_eval(sd32, dict(b32), num_head=case["model"]["H"], label_seq_length=T, token_sos=tok.SOS,
                                     token_eos=tok.EOS, trace=tr, forced=torch.from_numpy(paths), steps=step + 1)
        lg = tr["logits"][step].double().numpy()
        return np.where(lg > BR.FILL, lg, BR.FILL)

    res = BR.decode(step_logits, N, W, T, tok.SOS, tok.EOS, "all")
    steps = res["steps"]
    ok = np.ones(N, dtype=bool)
    left, min_gap = 0, np.inf
    for j in range(steps):
        ok &= res["gaps"][j] > 1.0
        left += int((~ok).sum())
        if ok.any():
            min_gap = min(min_gap, float(res["gaps"][j][ok].min()))
    return dict(left=left, pairs=steps * N, min_gap=min_gap, steps_all=steps, steps_best=BR.stop_step(res["best_counts"], T),
                finished=int((res["fin"] & np.isfinite(res["scores"])).sum()))


def engine_cases(names):
    kept, worst = {}, 0.0
    for name in names:
        for W in WIDTHS:
            r = oracle_decode(name, W)
            share = r["left"] / max(1, r["pairs"])
            worst = max(worst, share)
            kept[(name, W)] = (r["left"], r["pairs"], float("%.4g" % r["min_gap"]), r["steps_all"], r["finished"])
            print("%s W=%d: %d of %d (step, group) pairs left out (%.2f %%, cap %.0f %%); smallest kept gap %.4g; steps all %d best %d; "
                  "%d beams finished%s" % (name, W, r["left"], r["pairs"], 100 * share, 100 * BR.CAP, r["min_gap"], r["steps_all"],
                                           r["steps_best"], r["finished"], "  <-- above the cap: drop the case" if share >= BR.CAP else ""),
                  flush=True)
    print("KEPT = %r" % (kept,))
    return worst


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "operator":
        operator_seeds()
    elif what == "engine":
        sys.exit(1 if engine_cases(sys.argv[2:] or GOLDENS) >= BR.CAP else 0)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
