"""Which seeds and combinations tests/test_constrain_sample.py may use (CPU only).

Operator half: the reference of tests/constrain_sample_ref.py -- the byte row of constrain_ref / lookahead_ref / exact_ref, then
sample_ref.sample_row -- applied to the test's own seeded rows (the raw fp32 logits, the states and the uniforms are inputs, so
the GPU is not needed to know them).  Prints, per case (one key count S and one form: all its shapes, flag combinations and
parameter sets, test_constrain_sample.operator_cases), the share of unfinished rows whose draw or top-p cut is indecisive, and
exits non-zero when a case is above sample_ref.CAP.  A seed is changed, never the cap.

Engine half: which (golden, form, parameter set) combinations the engine tests may use, on the lattice of
constrain_ref.LATTICE_SEEDS with constrain_sample_ref.REPLAY_SEED and R = REPLAY_R draws per anchor.  The fp32 oracle
(oracle/refpath.py, forced=) draws its own constrained paths: at every step it is forced along the tokens so far, the fp64 rule
is applied to its masked fp32 logits with the test's uniforms, and the drawn token is appended.  Counted per combination: the
share of (step, unfinished draw) pairs that are indecisive, and enclosed / dead-ended / unclosed over the own-anchor draws.  A
combination is kept when the oracle alone leaves out less than the cap; a golden's guarantee test runs under the first form, in
the order plain, ahead, exact, under which the oracle alone encloses at least twice constrain_ref.MIN_ENCLOSED of its own-anchor
draws at tau = 1 (the first parameter set).  The exit status is non-zero when a combination of constrain_sample_ref is above the
cap or its GUARANTEE entry is not that form.

    python tools/constrain_sample_left_out.py [--operator [S ...]] [--engine [golden ...]]        (default: both, everything)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constrain_ref as CR  # noqa: E402
import constrain_sample_ref as CSR  # noqa: E402
import sample_ref as SR  # noqa: E402


def oracle_step_logits(case, sd32, b32, paths, step, seqs, F):
    """[rows', S] masked fp32 logits (as fp64 numpy, masked keys at FILL) of step `step` of the oracle forced along `paths`."""
    import torch
    from oracle import refpath
    tr = {}
    refpath.parallel_forward_eval(sd32, dict(b32), num_head=case["model"]["H"], trace=tr, forced=torch.from_numpy(paths), steps=step + 1,
                                  seqs=None if seqs is None else torch.as_tensor(seqs), num_anchors=F)
    lg = tr["logits"][step].double().numpy()
    return np.where(lg > SR.FILL, lg, SR.FILL)


def oracle_draws(case, sd32, b32, ni, follows, close, cycle, form, u, R, params, rows, seqs, tok):
    """The oracle's own constrained sampled paths of the anchor rows `rows`, draw by draw.  -> (paths [R, N*F, T], dead [R, N*F],
    pairs, indecisive pairs)."""
    N, F, T = len(ni), max(ni), case["model"]["seq_len"]
    term, ntok = (tok.face_type_offset, tok.len), tok.len
    tau, K, P = params
    all_paths, all_dead = [], []
    pairs = left = 0
    for k in range(R):
        paths = np.zeros((N * F, T), dtype=np.int64)
        f = np.arange(N * F) % F
        paths[:, 0] = np.where(f < np.repeat(ni, F), f, ntok - 1)
        state = [CR.start_state(int(paths[r, 0]), ntok, follows[r // F]) for r in range(N * F)]
        fin = (paths[:, 0] >= term[0]) & (paths[:, 0] < term[1])
        dead = np.zeros(N * F, dtype=bool)
        for s in range(T - 1):
            if fin[rows].all():
                break
            lg = oracle_step_logits(case, sd32, b32, paths, s, seqs, F)
            for i, r in enumerate(rows):
                if fin[r]:
                    continue
                w = r // F
                res = CSR.step_row(form, lg[i], lg[i] <= SR.FILL, state[r], CSR.LOOPS, ntok, term, follows[w], u[s, r * R + k], tau, K, P,
                                   close_dist=close[w], cycle_len=cycle[w], budget=T - 2 - s)
                pairs, left = pairs + 1, left + (not res["decisive"])
                paths[r, s + 1], state[r], fin[r] = res["tok"], res["state"], res["fin"]
                dead[r] |= res["dead"]
        all_paths.append(paths)
        all_dead.append(dead)
    return np.stack(all_paths), np.stack(all_dead), pairs, left


def yield_of(paths, dead, ni, edges, rows, tok):
    """(enclosed, dead-ended, unclosed, own-anchor draws) over the draws of the own-anchor rows among `rows`."""
    from faceformer_amd import faces
    F = paths.shape[1] // len(ni)
    enc = de = un = 0
    for r in rows:
        w, f = r // F, r % F
        if f >= ni[w]:
            continue
        for k in range(paths.shape[0]):
            row = paths[k, r]
            face = faces._parallel_rows(row[None], tok, ni[w])
            ends = ((row >= tok.face_type_offset) & (row < tok.len)).any()
            if dead[k, r]:
                de += 1
            elif ends and face and faces.is_face_enclosed(edges[w], face[0][1], CR.TOL):
                enc += 1
            else:
                un += 1
    return enc, de, un, enc + de + un


def engine(names):
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    from faceformer_amd import faces
    tok = token_ns()
    bad = 0
    for name in names:
        case, _ = load_golden(name)
        sd, gb = case_weights_and_batch(case)
        m = case["model"]
        batch, edges, _ = CR.lattice_batch(gb["num_input"], m["L"], m["seq_len"], CR.LATTICE_SEEDS[name])
        ni = batch["num_input"]
        N, F, T, R = len(ni), max(ni), m["seq_len"], CSR.REPLAY_R
        follows = faces.follow_table(batch["input"].numpy(), CR.TOL, ni)
        close, cycle = faces.follow_distance(follows, max(T - 2, 1), ni)
        sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
        b32 = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
        u = SR.make_uniforms(ni, T, R, CSR.REPLAY_SEED).numpy()
        seqs = SR.SUBSET.get(name)
        rows = np.array(seqs if seqs is not None else range(N * F))
        first_ok = None
        for form in CSR.FORMS:
            for pi, params in enumerate(CSR.REPLAY_PARAMS):
                paths, dead, pairs, left = oracle_draws(case, sd32, b32, ni, follows, close, cycle, form, u, R, params, rows, seqs, tok)
                share = left / max(1, pairs)
                enc, de, un, own = yield_of(paths, dead, ni, edges, rows, tok)
                kept = share < SR.CAP
                bad += not kept
                floor = enc >= 2 * CR.MIN_ENCLOSED * own
                if pi == 0 and floor and first_ok is None:
                    first_ok = form
                print("%s lattice seed %d uniforms seed %d R=%d %s tau=%g K=%d P=%g: %d of %d pairs indecisive (%.2f %%, cap %.0f %%): %s; "
                      "own-anchor draws enclosed / dead end / unclosed of %d: %d / %d / %d (%.1f %% enclosed%s)"
                      % (name, CR.LATTICE_SEEDS[name], CSR.REPLAY_SEED, R, form, params[0], params[1], params[2], left, pairs, 100 * share,
                         100 * SR.CAP, "kept" if kept else "NOT kept", own, enc, de, un, 100.0 * enc / max(1, own),
                         ", reaches twice the floor" if floor else ""), flush=True)
        print("%s: the guarantee test runs under %r (constrain_sample_ref.GUARANTEE: %r)" % (name, first_ok, CSR.GUARANTEE.get(name)), flush=True)
        bad += first_ok != CSR.GUARANTEE.get(name)
    return bad


def operator(sizes):
    import test_constrain_sample as TCS
    bad = 0
    for S in sizes or TCS.SIZES:
        for form in CSR.FORMS:      # a CASE is one (S, form), as in the test: all its shapes, flag combinations and parameter sets
            seen = left = 0
            for c, flags, params, budget in TCS.operator_cases(S, form):
                for b, r in enumerate(TCS.reference_rows(c, form, flags, params, budget)):
                    if not c["fin"][b]:
                        seen, left = seen + 1, left + (not r["decisive"])
            share = left / max(1, seen)
            bad += share > SR.CAP
            print("S=%d %s: %d of %d rows indecisive (%.2f %%, cap %.0f %%)%s"
                  % (S, form, left, seen, 100 * share, 100 * SR.CAP, "  <-- above the cap" if share > SR.CAP else ""), flush=True)
    return bad


def main():
    args = sys.argv[1:]
    both = not args
    bad = 0

    def values(flag, conv):
        i = args.index(flag) + 1 if flag in args else 0
        vals = []
        while i and i < len(args) and not args[i].startswith("--"):
            vals.append(conv(args[i]))
            i += 1
        return vals
    if both or "--operator" in args:
        bad += operator(values("--operator", int))
    if both or "--engine" in args:
        bad += engine(values("--engine", str) or list(CR.LATTICE_SEEDS))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
