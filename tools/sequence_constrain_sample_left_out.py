"""Which (golden, kind, seed, flags, tau / K / P) tuples tests/test_sequence_constrain_sample.py may use, and what the option buys
(CPU only).

The 2 % cap on the left-out (step, unfinished draw) pairs is a condition on the test's inputs, not a measurement of the engine.
The fp32 oracle (oracle/refpath.seq2seq_forward_eval, forced= / trace=) samples its own constrained paths on the fixtures of
tests/sequence_constrain_ref.py: at every step it is forced along the tokens drawn so far, the step of
tests/sequence_constrain_sample_ref.py (faces.sequence_rule_mask, sample_ref.sample_row, faces.sequence_rule_advance) is applied
to its masked logits with the test's seeded uniforms, and the drawn token is appended.  The fp64 oracle is then teacher-forced
along those draws; a (step, unfinished draw) pair is left out when the fp64 constrained row is indecisive for the pair's uniform
(inside sample_ref's guard band, where an fp32 evaluation may legitimately take the neighbouring key).  A tuple is kept only when
the share is at most CAP; a seed is changed, never the cap.  The R draws of a wireframe are R rows of the oracle's batch.  The
oracle recomputes every prefix at every step, so the tuples (sequence_constrain_sample_ref.REPLAY_FIXTURES x FLAGS x REPLAY_PARAMS)
run in parallel worker processes of one thread each (--jobs, default 8).

Printed per tuple, in the form of sequence_constrain_sample_ref.KEPT: left-out pairs, pairs, enclosed faces, parsed faces, dead
ends over all draws; whether the fp64 rule draws the fp32 oracle's tokens on every decisive pair; steps.  Non-zero exit when a
listed tuple fails or KEPT differs (without --write).

    python tools/sequence_constrain_sample_left_out.py [--write] [--jobs 8]
    python tools/sequence_constrain_sample_left_out.py --yield      the table of DESIGN.md 33: the five lattice fixtures at R = 16,
        tau = 1, for sequence_samples and for the option under "loops" and "coedge_loops" -- draws reaching EOS, enclosed faces
        over parsed faces across draws, faces with more than R / 2 votes (closed faces only).  Synthetic weights: no threshold.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sequence_constrain_sample_ref as QC  # noqa: E402


def _setup(name, kind, seed, R):
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    tok = token_ns()
    case, _ = load_golden(name)
    sd, gb = case_weights_and_batch(case)
    batch, follows, edges = QC.fixture(case, gb, kind, seed)
    N = len(batch["num_input"])
    rep = torch.arange(N).repeat_interleave(R)
    rb = {k: (v.index_select(0, rep) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in batch.items()}
    return tok, case, sd, rb, batch["num_input"], follows, edges


def _oracle_step(case, sd, b, tok, dtype):
    import torch
    from oracle import refpath
    sdx = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    bx = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
    fill = float(torch.finfo(dtype).min)

    def step_logits(paths, step):
        tr = {}
        refpath.seq2seq_forward_eval(sdx, dict(bx), num_head=case["model"]["H"], label_seq_length=case["model"]["seq_len"],
                                     token_sos=tok.SOS, token_eos=tok.EOS, trace=tr, forced=torch.from_numpy(paths), steps=step + 1)
        lg = tr["logits"][step].double().numpy()
        return np.where(lg > fill, lg, QC.FILL)
    return step_logits


def _enclosed(tokens, dead, R, ni, tok, follows, edges):
    from faceformer_amd import faces
    enc = par = 0
    for r in range(tokens.shape[0]):
        w = r // R
        for idx, _, _ in QC.face_pieces(tokens[r], dead[r], tok.len, tok.SEP, tok.EOS, ni[w]):
            par += 1
            enc += bool(QC.walk_closed(idx, follows[w]) if edges is None else faces.is_face_enclosed(edges[w], idx, QC.TOL))
    return enc, par


def check(name, kind, seed, flags, params):
    import torch
    R = QC.REPLAY_R
    tok, case, sd, rb, ni, follows, edges = _setup(name, kind, seed, R)
    N, T = len(ni), case["model"]["seq_len"]
    u = QC.make_uniforms(N, T, R, QC.REPLAY_SEEDS[name]).numpy()
    d32 = QC.decode(_oracle_step(case, sd, rb, tok, torch.float32), u, N, T, R, flags, tok.len, tok.SOS, tok.SEP, tok.EOS, follows, *params)
    p32, steps = d32["tokens"], d32["steps"]
    fin, _ = QC.stop_and_finish(p32, tok.EOS)
    step64 = _oracle_step(case, sd, rb, tok, torch.float64)
    states = QC.replay_states(p32, R, flags, tok.len, tok.SEP, follows)
    pairs = left = 0
    same = True
    for j in range(steps):
        lg = step64(p32, j)
        for r in np.flatnonzero(fin > j):
            res = QC.step(lg[r], lg[r] <= QC.FILL, states[r][j], flags, tok.len, tok.SEP, tok.EOS, follows[r // R], u[j, r], *params)
            pairs += 1
            left += not res["decisive"]
            same = same and (not res["decisive"] or res["tok"] == p32[r, j + 1])
    enc, par = _enclosed(p32, d32["dead"], R, ni, tok, follows, edges)
    rec = (int(left), int(pairs), int(enc), int(par), int(d32["dead"].sum()))
    ok = left <= QC.CAP * max(1, pairs)
    print("    (%r, %r, %d, %d, %r): %r,   # decisive fp64 draws = fp32 draws: %s; steps %d; draws at EOS %d of %d%s"
          % (name, kind, seed, flags, tuple(params), rec, same, steps, int((fin < T).sum()), N * R, "" if ok else "  NOT kept"), flush=True)
    return ok, rec


def yield_row(job):
    """One row of DESIGN.md 33's table on the oracle (fp64), R = 16, tau = 1, seed 5: a lattice fixture under one mode."""
    import torch
    torch.set_num_threads(1)
    (name, kind, seed), (mode, flags) = job
    R, params = 16, (1.0, 0, 1.0)
    if True:
        tok, case, sd, rb, ni, follows, edges = _setup(name, kind, seed, R)
        N, T = len(ni), case["model"]["seq_len"]
        u = QC.make_uniforms(N, T, R, 5).numpy()
        step64 = _oracle_step(case, sd, rb, tok, torch.float64)
        if True:
            d = QC.decode(step64, u, N, T, R, flags, tok.len, tok.SOS, tok.SEP, tok.EOS, follows, *params)
            fin, _ = QC.stop_and_finish(d["tokens"], tok.EOS)
            enc, par = _enclosed(d["tokens"], d["dead"], R, ni, tok, follows, edges)
            from faceformer_amd import faces
            major = 0
            for w in range(N):
                votes = {}
                for r in range(w * R, (w + 1) * R):
                    seen = set()
                    for idx, at_dead_end, _ in QC.face_pieces(d["tokens"][r], d["dead"][r], tok.len, tok.SEP, tok.EOS, ni[w]):
                        key = tuple(sorted(set(idx)))
                        if not at_dead_end and key not in seen and faces.is_face_enclosed(edges[w], idx, QC.TOL):
                            seen.add(key)
                            votes[key] = votes.get(key, 0) + 1
                major += sum(1 for v in votes.values() if 2 * v > R)
            return "%s/%s%d | %s | %d of %d | %d / %d | %d" % (name, kind, seed, mode, int((fin < T).sum()), N * R, enc, par, major)


def _check_job(job):
    import torch
    torch.set_num_threads(1)
    return job, check(*job)


def _jobs(argv):
    return int(argv[argv.index("--jobs") + 1]) if "--jobs" in argv else 8


def main(argv):
    import multiprocessing as mp
    if "--yield" in argv:
        modes = (("sequence_samples", 0), ("loops", QC.LOOPS), ("coedge_loops", QC.COEDGE_LOOPS))
        print("fixture | mode | draws at EOS | enclosed / parsed faces over draws | closed faces with > R/2 votes")
        with mp.get_context("spawn").Pool(_jobs(argv)) as pool:
            for line in pool.imap(yield_row, [(f, m) for f in QC.FIXTURES if f[1] == "lattice" for m in modes]):
                print(line, flush=True)
        return 0
    bad = 0
    jobs = [f + (flags, tuple(params)) for f in QC.REPLAY_FIXTURES for flags in QC.FLAGS for params in QC.REPLAY_PARAMS]
    with mp.get_context("spawn").Pool(_jobs(argv)) as pool:
        for key, (ok, rec) in pool.imap(_check_job, jobs):
            bad += not ok
            if "--write" not in argv and QC.KEPT.get(key) != rec:
                print("      ^ differs from sequence_constrain_sample_ref.KEPT: %r" % (QC.KEPT.get(key),))
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
