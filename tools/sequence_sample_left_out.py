"""Which (golden, seed, tau / K / P) triples the replay test of tests/test_sequence_sample.py may use.

The 2 % cap on the left-out (step, unfinished draw) pairs is a condition on the test's inputs, not a measurement of the engine.
Here the fp32 oracle (oracle/refpath.py: seq2seq_forward_eval, forced=) samples its own paths on the CPU: at every step it is
forced along the tokens drawn so far, the fp64 rule of tests/sequence_sample_ref.py is applied to its masked fp32 logits with the
seeded uniforms of sequence_sample_ref.make_uniforms, and the drawn token is appended.  Counted: the share of (step, unfinished
draw) pairs that are indecisive -- inside sample_ref's guard band, where an fp32 evaluation may legitimately take the neighbouring
key.  A triple is kept only when the oracle alone leaves out less than the cap; a seed is changed, never the cap.  The R draws of a
wireframe are R rows of the oracle's batch (the wireframe repeated), so one oracle call per step serves them all.

    python tools/sequence_sample_left_out.py [golden ...]        (default: every golden of sequence_sample_ref.REPLAY_SEEDS)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sequence_sample_ref as QR  # noqa: E402


def oracle_decode(name, seed, R, tau, K, P):
    """-> (indecisive pairs, pairs) of the oracle's own sampled decode of golden `name`."""
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    from oracle import refpath
    tok = token_ns()
    case, _ = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    N, T = batch["input"].size(0), case["model"]["seq_len"]
    rep = torch.arange(N).repeat_interleave(R)
    b32 = {k: ((v.float() if v.is_floating_point() else v).index_select(0, rep) if torch.is_tensor(v) and v.dim() and v.size(0) == N
               else v) for k, v in batch.items()}
    u = QR.make_uniforms(N, T, R, seed).numpy()

    def step_logits(paths, step):
        tr = {}
        refpath.seq2seq_forward_eval(sd32, dict(b32), num_head=case["model"]["H"], label_seq_length=T, token_sos=tok.SOS,
                                     token_eos=tok.EOS, trace=tr, forced=torch.from_numpy(paths), steps=step + 1)
        lg = tr["logits"][step].double().numpy()
        return np.where(lg > QR.FILL, lg, QR.FILL)

    toks, _, dec, steps = QR.decode(step_logits, u, N, T, R, tok.EOS, tok.SOS, tau, K, P)
    fin, _ = QR.stop_and_finish(toks, tok.EOS)
    pairs = sum(int((fin > s).sum()) for s in range(steps))
    return int((~dec[:steps]).sum()), pairs


def main():
    names = sys.argv[1:] or list(QR.REPLAY_SEEDS)
    worst = 0.0
    for name in names:
        seed = QR.REPLAY_SEEDS[name]
        for tau, K, P in QR.REPLAY_PARAMS:
            left, pairs = oracle_decode(name, seed, QR.REPLAY_R, tau, K, P)
            share = left / max(1, pairs)
            worst = max(worst, share)
            print("%s seed %d R=%d tau=%g K=%d P=%g: %d of %d pairs indecisive (%.2f %%, cap %.0f %%)%s"
                  % (name, seed, QR.REPLAY_R, tau, K, P, left, pairs, 100 * share, 100 * QR.CAP,
                     "  <-- above the cap: drop the triple" if share >= QR.CAP else ""), flush=True)
    sys.exit(1 if worst >= QR.CAP else 0)


if __name__ == "__main__":
    main()
