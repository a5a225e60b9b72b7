"""Which operator seeds and which (golden, kind, seed, flags, W) tuples tests/test_sequence_constrain_beam.py may use, and what the
option buys (CPU only).

The 2 % cap on what a test leaves out as indecisive is a condition on the test's inputs, not a measurement of the kernels.

    python tools/sequence_constrain_beam_left_out.py operator
        Every case of the operator test's grid (sequence_constrain_beam_ref.OP_*): the rule is applied to the test's seeded
        operands in fp64 and in fp32-ROUNDED arithmetic (sequence_beam_ref.step_fp32 on the constrained rows).  A group is left
        out when its smallest decisive gap is at most twice beam_ref.score_bound, or when the two evaluations select differently.
        A seed is kept only if at most CAP of the case's groups are left out; otherwise the offset in OP_SEED_OFFSETS changes.
    python tools/sequence_constrain_beam_left_out.py engine [--write] [--jobs 8]
        The fp32 oracle (oracle/refpath.seq2seq_forward_eval, forced= / trace=) searches its own constrained beams on the fixtures
        of tests/sequence_constrain_ref.py: at every step it is forced along the W prefixes of every wireframe, the step of
        tests/sequence_constrain_beam_ref.py is applied to its logits, and the kept candidates become the next prefixes.  The fp64
        oracle is then forced along those decisions; a (step, group) pair is left out from the group's first step whose fp64 gap
        is at most 1 (twice the bound accumulated over the steps so far) on.  A tuple is KEPT only if the oracle alone leaves out
        at most CAP of its pairs, else DROPPED.  Printed per tuple, in the form of sequence_constrain_beam_ref.KEPT: left-out
        pairs, pairs, enclosed faces, parsed faces and dead ends over the non-empty final beams, steps under "all".
    python tools/sequence_constrain_beam_left_out.py --yield [--jobs 8]
        The table of DESIGN.md 34 on the fp64 oracle: the five lattice fixtures at W = 1 / 4 / 8 under "loops" and "coedge_loops"
        -- whether beam 0 reaches EOS, its enclosed / parsed faces, its dead ends and its score, beside the greedy constrained
        row's.  Synthetic weights: no threshold.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import beam_ref as R  # noqa: E402
import sequence_beam_ref as QB  # noqa: E402
import sequence_constrain_beam_ref as CB  # noqa: E402
import sequence_constrain_ref as SC  # noqa: E402


# ---- operator -----------------------------------------------------------------------------------------------------------------------
def operator():
    import test_sequence_constrain_beam as TB
    from faceformer_amd import faces
    bad = cases = 0
    for S in CB.OP_S:
        for W in CB.OP_W:
            if W > S:
                continue
            for G in CB.OP_G:
                for flags in CB.OP_FLAGS:
                    for scenario in CB.OP_SCENARIOS:
                        c = TB._beam_case(S, W, G, flags, scenario)
                        want = TB._want_of(c, flags)
                        left, gaps = 0, []
                        for g, wg in enumerate(want):
                            sl = slice(g * W, (g + 1) * W)
                            rows = np.stack([c["logits"][g * W + k].astype(np.float64) if wg["rows"][k] is None else wg["rows"][k] for k in range(W)])
                            par, tok = QB.step_fp32(rows, c["scores"][sl], c["fin"][sl] != 0, W, TB.EOS)
                            n = min(W, int(wg["candidates"]))
                            same = np.array_equal(par[:n], wg["parent"][:n]) and np.array_equal(tok[:n], wg["tok"][:n])
                            left += (not wg["gap"] > 1.0) or not same
                            gaps.append(wg["gap"])
                        cases += 1
                        ok = left <= CB.CAP * G
                        bad += not ok
                        print("S=%-4d W=%d G=%d flags=%d %-6s seed %-5d left out %d of %d groups, smallest gap %.3g%s"
                              % (S, W, G, flags, scenario, CB.op_seed(S, W, G, flags, scenario), left, G, min(gaps), "" if ok else "  NOT kept"))
    print("%d cases, %d above the cap" % (cases, bad))
    return 1 if bad else 0


# ---- engine -------------------------------------------------------------------------------------------------------------------------
def _setup(name, kind, seed, W):
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    tok = token_ns()
    case, _ = load_golden(name)
    sd, gb = case_weights_and_batch(case)
    batch, follows, edges = CB.fixture(case, gb, kind, seed)
    N = len(batch["num_input"])
    rep = torch.arange(N).repeat_interleave(W)
    rb = {k: (v.index_select(0, rep) if torch.is_tensor(v) and v.dim() and v.size(0) == N else v) for k, v in batch.items()}
    return tok, case, sd, rb, batch["num_input"], follows, edges


def _oracle_step(case, sd, b, tok, dtype):
    """step_logits(prefixes [B, j + 1], j) -> the oracle's logits [B, S] of step j, forced along the prefixes (padded keys at FILL)."""
    import torch
    from oracle import refpath
    sdx = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    bx = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in b.items()}
    fill = float(torch.finfo(dtype).min)
    T = case["model"]["seq_len"]

    def step_logits(prefixes, step):
        paths = np.zeros((prefixes.shape[0], T), dtype=np.int64)
        paths[:, : prefixes.shape[1]] = prefixes
        tr = {}
        refpath.seq2seq_forward_eval(sdx, dict(bx), num_head=case["model"]["H"], label_seq_length=T, token_sos=tok.SOS, token_eos=tok.EOS,
                                     trace=tr, forced=torch.from_numpy(paths), steps=step + 1)
        lg = tr["logits"][step].double().numpy()
        return np.where(lg > fill, lg, CB.FILL)
    return step_logits


def _pads(case, ni, ntok):
    S = case["model"]["L"] + ntok
    return np.stack([np.arange(S) >= ntok + n for n in ni])


def check(name, kind, seed, flags, W):
    import torch
    from faceformer_amd import faces
    tok, case, sd, rb, ni, follows, edges = _setup(name, kind, seed, W)
    N, T = len(ni), case["model"]["seq_len"]
    pads = _pads(case, ni, tok.len)
    d32 = CB.decode(_oracle_step(case, sd, rb, tok, torch.float32), pads, W, T, flags, tok.len, tok.SOS, tok.SEP, tok.EOS, follows, "all")
    steps = d32["steps"]
    step64 = _oracle_step(case, sd, rb, tok, torch.float64)
    scores, fin = QB.start(N, W)
    states = [faces.sequence_rule_start()] * (N * W)
    ok = np.ones(N, dtype=bool)
    left, same = 0, True
    tok0 = np.full(N * W, tok.SOS, dtype=np.int64)
    for j in range(steps):
        prefixes = R.backtrack(tok0, d32["toks"][:j], d32["parents"][:j], W)
        lg = step64(prefixes, j)
        res = CB.beam_step(lg, pads, scores, fin, states, W, flags, tok.len, tok.SEP, tok.EOS, follows, margin=j + 1)
        ok &= res["gap"] > 1.0
        left += int((~ok).sum())
        okb = np.repeat(ok, W)
        same = same and np.array_equal(res["parent"][okb], d32["parents"][j][okb]) and np.array_equal(res["tok"][okb], d32["toks"][j][okb])
        # forced along the fp32 oracle's decisions: its parents and tokens, the fp64 scores of exactly those candidates
        nsc, nfin, nst = np.full(N * W, CB.NEG), np.zeros(N * W, dtype=bool), list(states)
        for r in range(N * W):
            g = r // W
            p, s = g * W + int(d32["parents"][j][r]), int(d32["toks"][j][r])
            if r % W >= res["candidates"][g]:      # (the number of candidates is a function of the integer state: the same in both)
                nst[r] = states[r]                 # an empty rank keeps the state of its own index
                continue
            if fin[p]:
                nsc[r], nfin[r], nst[r] = scores[p], True, states[p]
                continue
            row = res["rows"][p]
            m = row.max()
            nsc[r] = max(scores[p] + ((row[s] - m) - np.log(np.exp(row - m).sum())), -R.FLT_MAX)
            nfin[r] = s == tok.EOS
            nst[r] = faces.sequence_rule_advance(states[p], s, flags, tok.len, tok.SEP, None if follows is None else follows[g])
        scores, fin, states = nsc, nfin, nst
    enc, par, dead = CB.guarantee(d32["beams"], d32["dead_end"], d32["open"].astype(int), d32["scores"], W, ni, flags, tok.len, tok.SEP, tok.EOS,
                                  follows, edges)
    pairs = steps * N
    rec = (int(left), int(pairs), int(enc), int(par), int(dead), int(steps))
    ok_all = left <= CB.CAP * max(1, pairs)
    live = np.isfinite(d32["scores"])
    print("    (%r, %r, %d, %d, %d): %r,   # decisive fp64 decisions = fp32 decisions: %s; finished %d of %d non-empty beams%s"
          % (name, kind, seed, flags, W, rec, same, int((d32["fin"] & live).sum()), int(live.sum()), "" if ok_all else "  DROPPED"), flush=True)
    return ok_all, rec


def _check_job(job):
    import torch
    torch.set_num_threads(1)
    return job, check(*job)


def yield_row(job):
    """One row of DESIGN.md 34's table on the fp64 oracle: a lattice fixture at one width under one mode, beam 0 of every wireframe
    beside the greedy constrained row."""
    import torch
    from faceformer_amd import faces
    torch.set_num_threads(1)
    (name, kind, seed), (mode, flags), W = job
    tok, case, sd, rb, ni, follows, edges = _setup(name, kind, seed, W)
    N, T = len(ni), case["model"]["seq_len"]
    pads = _pads(case, ni, tok.len)
    d = CB.decode(_oracle_step(case, sd, rb, tok, torch.float64), pads, W, T, flags, tok.len, tok.SOS, tok.SEP, tok.EOS, follows, "all")
    _, _, _, rb1, _, _, _ = _setup(name, kind, seed, 1)
    g1 = _oracle_step(case, sd, rb1, tok, torch.float64)
    greedy = SC.decode(lambda paths, s: g1(paths[:, : s + 1], s), N, T, flags, tok.len, tok.SOS, tok.SEP, tok.EOS, follows)
    b0 = np.arange(N) * W
    enc, par, dead = CB.guarantee(d["beams"][b0], d["dead_end"][b0], d["open"][b0].astype(int), d["scores"][b0], 1, ni, flags, tok.len, tok.SEP,
                                  tok.EOS, follows, edges)
    genc, gpar, gdead = CB.guarantee(greedy["tokens"], greedy["dead"], greedy["open_end"], np.zeros(N), 1, ni, flags, tok.len, tok.SEP, tok.EOS,
                                     follows, edges)
    at_eos = int((d["beams"][b0] == tok.EOS).any(axis=1).sum())
    g_eos = int((greedy["tokens"] == tok.EOS).any(axis=1).sum())
    return "%s/%s%d | %s | %d | %d of %d | %d / %d | %d | %s | %d of %d | %d / %d | %d | %s" % (
        name, kind, seed, mode, W, at_eos, N, enc, par, dead, " ".join("%.2f" % v for v in d["scores"][b0]), g_eos, N, genc, gpar, gdead,
        " ".join("%.2f" % v for v in greedy["logprob"].sum(axis=1)))


def _jobs(argv):
    return int(argv[argv.index("--jobs") + 1]) if "--jobs" in argv else 8


def main(argv):
    import multiprocessing as mp
    if "--yield" in argv:
        modes = (("loops", CB.LOOPS), ("coedge_loops", CB.COEDGE_LOOPS))
        print("fixture | mode | W | beam 0 at EOS | enclosed / parsed | dead ends | scores || greedy at EOS | enclosed / parsed | dead ends | scores")
        with mp.get_context("spawn").Pool(_jobs(argv)) as pool:
            for line in pool.imap(yield_row, [(f, m, W) for f in CB.FIXTURES if f[1] == "lattice" for m in modes for W in (1, 4, 8)]):
                print(line, flush=True)
        return 0
    if argv and argv[0] == "operator":
        return operator()
    if not argv or argv[0] != "engine":
        print(__doc__)
        return 2
    bad = 0
    jobs = [f + (flags, W) for f in CB.FIXTURES for flags in CB.FLAGS for W in CB.REPLAY_W]
    with mp.get_context("spawn").Pool(_jobs(argv)) as pool:
        for key, (ok, rec) in pool.imap(_check_job, jobs):
            table = CB.KEPT if ok else CB.DROPPED
            if "--write" not in argv and table.get(key) != rec:
                print("      ^ differs from sequence_constrain_beam_ref.%s: %r" % ("KEPT" if ok else "DROPPED", table.get(key)))
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
