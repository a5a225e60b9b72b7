"""The sampled single-sequence decode in numpy fp64: the selection rule is sample_ref's, unchanged (the device has
one copy of it as well); what is stated here is what differs from the parallel sampled decode -- start, finish, stop, layout.

  layout   N * R rows; draw k of wireframe w is row w * R + k and reads uniforms[t, w * R + k] at step t.
  start    every row holds SOS at position 0, log-probability 0.
  finish   a row is finished from the first position >= 1 that holds EOS; SEP and the other special tokens do not finish it.
           A finished row appends 0, draws nothing, log-probability 0.
  stop     after the first step after which every row is finished (steps = that step + 1), else after T - 1 steps.  The count the
           engine keeps per step is "rows unfinished after the step".
"""
import numpy as np

import sample_ref as SR

FILL, EPS, LP_BAR, CAP = SR.FILL, SR.EPS, SR.LP_BAR, SR.CAP
sample_row, sample_rows, logprob_of = SR.sample_row, SR.sample_rows, SR.logprob_of

# The engine replay's (golden, seed, tau / K / P) triples at REPLAY_R draws per wireframe.  The 2 % cap on left-out pairs is a
# CONDITION on the triple, not a measurement of the engine: tools/sequence_sample_left_out.py lets the fp32 oracle sample its own
# paths on the CPU with these seeded uniforms, and a triple is kept only if the oracle alone leaves out less than the cap.
# KEPT: the triples the test uses, with the oracle's share (indecisive pairs of all pairs); DROPPED: tried and above the cap.
REPLAY_R = 4
REPLAY_PARAMS = [(1.0, 0, 1.0), (0.8, 16, 0.9)]
REPLAY_SEEDS = {"seq_small_gain4": 5, "seq_small_eos": 5, "seq_small_repeat_eos": 5}
KEPT = {      # (golden, (tau, K, P)) -> (indecisive pairs, pairs) of the oracle's own sampled decode, seed REPLAY_SEEDS[golden]
    ("seq_small_gain4", (1.0, 0, 1.0)): (0, 124), ("seq_small_gain4", (0.8, 16, 0.9)): (0, 124),
    ("seq_small_eos", (1.0, 0, 1.0)): (0, 8), ("seq_small_eos", (0.8, 16, 0.9)): (0, 8),
    ("seq_small_repeat_eos", (1.0, 0, 1.0)): (0, 65), ("seq_small_repeat_eos", (0.8, 16, 0.9)): (0, 64),
}
DROPPED = {}      # none: every triple tried stayed below the cap


def make_uniforms(N, T, R, seed):
    """uniforms [max(T-1, 1), N*R] fp32 (CPU tensor) of a seeded decode: column w*R + k."""
    import torch
    return torch.rand((max(T - 1, 1), N * R), generator=torch.Generator().manual_seed(seed))


def stop_and_finish(tokens, eos):
    """From decoded tokens [rows, T]: (finish position of every row -- the first position >= 1 holding eos; T when there is none
    -- and the stop step: steps = s + 1 for the first step s after which every row is finished, else T - 1)."""
    tokens = np.asarray(tokens)
    T = tokens.shape[1]
    hit = tokens[:, 1:] == eos
    fin = np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, T)
    steps = T - 1
    for s in range(T - 1):
        if (fin <= s + 1).all():
            steps = s + 1
            break
    return fin, steps


def unfinished_after(tokens, eos):
    """[T-1] the rows unfinished after every step: what the engine's per-step counter holds up to the stop step."""
    fin, _ = stop_and_finish(tokens, eos)
    return np.array([(fin > s + 1).sum() for s in range(np.asarray(tokens).shape[1] - 1)])


def decode(step_logits, u, N, T, R, eos, sos, tau=1.0, K=0, P=1.0):
    """The whole rule as a loop: step_logits(paths [N*R, T], step) -> masked logits [N*R, S] (fp64) of `step` along the tokens so
    far.  Returns (tokens [N*R, T], logprob [N*R, T], decisive [T-1, N*R] -- True where the row was finished --, steps)."""
    B = N * R
    tok = np.zeros((B, T), dtype=np.int64)
    lp = np.zeros((B, T))
    tok[:, 0] = sos
    fin = np.zeros(B, dtype=bool)
    dec = np.ones((max(T - 1, 1), B), dtype=bool)
    steps = T - 1
    for s in range(T - 1):
        lg = step_logits(tok, s)
        for r in range(B):
            if fin[r]:
                continue
            res = sample_row(lg[r], u[s, r], tau, K, P)
            tok[r, s + 1], lp[r, s + 1], dec[s, r] = res["tok"], res["logprob"], res["decisive"]
            fin[r] = res["tok"] == eos
        if fin.all():
            steps = s + 1
            break
    return tok, lp, dec, steps
