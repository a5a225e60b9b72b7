"""Which operator seeds and which (golden, kind, seed, flags, W, form) tuples tests/test_sequence_constrain_beam_closure.py may use
(CPU only).  The 2 % cap on what a test leaves out as indecisive is a condition on the test's inputs, not a
measurement of the kernels.  In the style of sequence_constrain_beam_left_out.py, whose set-up and oracle steps this reuses.

    python tools/sequence_constrain_beam_closure_left_out.py operator
        Every case of the operator test's grid (sequence_constrain_beam_closure_ref.op_cases): the rule under the case's form and
        budget is applied to the test's seeded operands in fp64 and in fp32-ROUNDED arithmetic (sequence_beam_ref.step_fp32 on the
        constrained rows).  A group is left out when its smallest decisive gap is at most twice beam_ref.score_bound, or when the
        two evaluations select differently.  A seed is kept only if NO group is left out; otherwise its offset in OP_SEED_OFFSETS
        changes.  Also printed per cell: the beams masked beyond the plain rule, the dead ends and the closures the numpy rule
        meets -- the test asserts them non-zero.
    python tools/sequence_constrain_beam_closure_left_out.py engine [--write] [--jobs 8]
        The fp32 oracle searches its own beams under the form on the fixtures of tests/sequence_constrain_ref.py, the fp64 oracle
        is forced along them (section 34's scheme); a tuple is KEPT only if the oracle alone leaves out at most CAP of its (step,
        group) pairs.  Printed per tuple in the form of sequence_constrain_beam_closure_ref.KEPT: left-out pairs, pairs, enclosed
        faces, parsed faces, dead ends, late dead ends and open ends over the non-empty final beams, steps under "all".
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import beam_ref as R  # noqa: E402
import sequence_beam_ref as QB  # noqa: E402
import sequence_constrain_beam_closure_ref as BC  # noqa: E402


def operator():
    import test_sequence_constrain_beam_closure as TC
    bad = cases = 0
    for S in BC.OP_S:
        for W in BC.OP_W:
            if W > S:
                continue
            seen = dict(stricter=0, dead=0, closing=0)
            for case in BC.op_cases(S, W):
                G, once, form, stop, kind, budget, seed, hmax = case
                c = TC._beam_closure_case(S, W, G, once, kind, seed, hmax)
                want = TC._want_of_closure(c, form, budget, seen)
                left, gaps = 0, []
                for g, wg in enumerate(want):
                    sl = slice(g * W, (g + 1) * W)
                    rows = np.stack([c["logits"][g * W + k].astype(np.float64) if wg["rows"][k] is None else wg["rows"][k] for k in range(W)])
                    par, tok = QB.step_fp32(rows, c["scores"][sl], c["fin"][sl] != 0, W, TC.EOS)
                    n = min(W, int(wg["candidates"]))
                    same = np.array_equal(par[:n], wg["parent"][:n]) and np.array_equal(tok[:n], wg["tok"][:n])
                    left += (not wg["gap"] > 1.0) or not same
                    gaps.append(wg["gap"])
                cases += 1
                bad += left > 0
                print("S=%-4d W=%d G=%d once=%d %-9s %-4s %-7s budget %-3d seed %-4d left out %d of %d groups, smallest gap %.3g%s"
                      % (S, W, G, once, form, stop, kind, budget, seed, left, G, min(gaps), "" if not left else "  NOT kept"))
            print("S=%-4d W=%d cell: %r" % (S, W, seen))
    print("%d cases, %d leave a group out" % (cases, bad))
    return 1 if bad else 0


def check(name, kind, seed, flags, W, form):
    import torch
    import sequence_constrain_beam_left_out as PL
    from faceformer_amd import faces
    tok, case, sd, rb, ni, follows, edges = PL._setup(name, kind, seed, W)
    N, T = len(ni), case["model"]["seq_len"]
    pads = PL._pads(case, ni, tok.len)
    cd, cl = BC.tables(follows, T, ni)
    d32 = BC.decode(PL._oracle_step(case, sd, rb, tok, torch.float32), pads, W, T, flags, tok.len, tok.SOS, tok.SEP, tok.EOS, follows, "all",
                    form, cd, cl)
    steps = d32["steps"]
    step64 = PL._oracle_step(case, sd, rb, tok, torch.float64)
    scores, fin = QB.start(N, W)
    states = [faces.sequence_rule_start()] * (N * W)
    ok = np.ones(N, dtype=bool)
    left, same = 0, True
    tok0 = np.full(N * W, tok.SOS, dtype=np.int64)
    for j in range(steps):
        prefixes = R.backtrack(tok0, d32["toks"][:j], d32["parents"][:j], W)
        res = BC.beam_step(step64(prefixes, j), pads, scores, fin, states, W, flags, tok.len, tok.SEP, tok.EOS, follows, form, cd, cl,
                           BC.budget_of(T, j + 1), margin=j + 1)
        ok &= res["gap"] > 1.0
        left += int((~ok).sum())
        okb = np.repeat(ok, W)
        same = same and np.array_equal(res["parent"][okb], d32["parents"][j][okb]) and np.array_equal(res["tok"][okb], d32["toks"][j][okb])
        # forced along the fp32 oracle's decisions: its parents and tokens, the fp64 scores of exactly those candidates
        nsc, nfin, nst = np.full(N * W, BC.NEG), np.zeros(N * W, dtype=bool), list(states)
        for r in range(N * W):
            g = r // W
            p, s = g * W + int(d32["parents"][j][r]), int(d32["toks"][j][r])
            if r % W >= res["candidates"][g]:
                nst[r] = states[r]
                continue
            if fin[p]:
                nsc[r], nfin[r], nst[r] = scores[p], True, states[p]
                continue
            row = res["rows"][p]
            m = row.max()
            nsc[r] = max(scores[p] + ((row[s] - m) - np.log(np.exp(row - m).sum())), -R.FLT_MAX)
            nfin[r] = s == tok.EOS
            nst[r] = faces.sequence_rule_advance(states[p], s, flags, tok.len, tok.SEP, follows[g])
        scores, fin, states = nsc, nfin, nst
    live = np.isfinite(d32["scores"])
    opens = int(d32["open"][live].sum())
    enc, par, dead, late = BC.guarantees(d32["beams"], d32["dead_end"], d32["open"].astype(int), d32["scores"], W, ni, flags, tok.len, tok.SEP,
                                         tok.EOS, follows, edges, form)
    pairs = steps * N
    rec = (int(left), int(pairs), int(enc), int(par), int(dead), int(late), opens, int(steps))
    ok_all = left <= BC.CAP * max(1, pairs)
    print("    (%r, %r, %d, %d, %d, %r): %r,   # decisive fp64 decisions = fp32 decisions: %s; finished %d of %d non-empty beams%s"
          % (name, kind, seed, flags, W, form, rec, same, int((d32["fin"] & live).sum()), int(live.sum()), "" if ok_all else "  DROPPED"),
          flush=True)
    return ok_all, rec


def _check_job(job):
    import torch
    torch.set_num_threads(1)
    return job, check(*job)


def main(argv):
    import multiprocessing as mp
    if argv and argv[0] == "operator":
        return operator()
    if not argv or argv[0] != "engine":
        print(__doc__)
        return 2
    bad = 0
    jobs = [f + (flags, W, form) for f in BC.FIXTURES for flags in BC.FLAGS for W in BC.REPLAY_W for form in BC.FORMS]
    with mp.get_context("spawn").Pool(int(argv[argv.index("--jobs") + 1]) if "--jobs" in argv else 8) as pool:
        for key, (ok, rec) in pool.imap(_check_job, jobs):
            table = BC.KEPT if ok else BC.DROPPED
            if "--write" not in argv and table.get(key) != rec:
                print("      ^ differs from sequence_constrain_beam_closure_ref.%s: %r" % ("KEPT" if ok else "DROPPED", table.get(key)))
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
