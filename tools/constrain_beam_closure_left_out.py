"""Which seeds tests/test_constrain_beam_closure.py may use, and what its non-vacuity thresholds are (CPU only): both are
conditions on the RULE, fixed here before any GPU result is looked at.

  operator   (default) exactly the test's launches (test_constrain_beam.operator_case over OP_S x OP_W x OP_G x BUDGETS x the two
             forms, seed op_seed(S, W, G), the tables of test_constrain_beam_closure.case_tables): the numpy rule
             (constrain_beam_closure_ref.beam_step) evaluated on the fp32 logits in fp64 gives every group's smallest decisive gap
             in units of twice the score bound; a group is left out when that is at most 1.  The rule is also evaluated with
             fp32 arithmetic (constrain_beam_left_out.group_step_f32 under the form's mask), and its parents and tokens must
             equal the fp64 rule's on every kept group.  Kept when the share per (S, form) is at most the cap.
  --engine   per (golden, lattice seed) of constrain_ref.LATTICE_SEEDS and form in plain / lookahead / exact: the fp64 oracle
             decodes the lattice wireframes under "loops" with W = 4 beams on the CPU, forced along the back-tracked prefixes
             of its own beams, with budget = T - 2 - j at step j and the tables of faces.follow_distance (hmax = max(T - 2, 1));
             the fp32 oracle is forced along the same prefixes.  A (step, group) pair is left out when the fp64 rule's gap is
             at most 1 (j x the bound at step j), and from a group's first such pair on.  Kept when the share is at most the cap.
             Also counted: the own-anchor groups whose best non-dead beam is enclosed -- the thresholds of the non-vacuity test
             (constrain_beam_closure_ref.ORACLE_W4, STRICT).

A seed is changed, never the cap.  Non-zero exit when a listed seed fails.  The counts go to
profiles/constrain_beam_closure/left_out.txt and yield.json (key "oracle_W4").

    python tools/constrain_beam_closure_left_out.py [--engine [golden ...]]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import beam_ref as BR  # noqa: E402
import constrain_beam_closure_ref as CL  # noqa: E402
import constrain_beam_left_out as PLAIN  # noqa: E402
import constrain_ref as CR  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "constrain_beam_closure")


def _say(lines, text):
    print(text, flush=True)
    lines.append(text)


def group_step_f32(form, close, cyc, budget, *args):
    """constrain_beam_left_out.group_step_f32 with the form's mask in place of the plain rule's."""
    saved = PLAIN.CR
    rule = CL._FormRule(form, close, cyc, budget)
    rule.FILL = CR.FILL
    PLAIN.CR = rule
    try:
        return PLAIN.group_step_f32(*args)
    finally:
        PLAIN.CR = saved


def operator(lines):
    import test_constrain_beam as T
    import test_constrain_beam_closure as TC
    bad = 0
    for S in T.OP_S:
        for closure in TC.CLOSURES:
            form = CL.FORMS[closure]
            groups = left = 0
            for W in T.OP_W:
                if W > S:
                    continue
                for G in T.OP_G:
                    c = T.operator_case(G, W, S, T.op_seed(S, W, G))
                    close, cyc = TC.case_tables(c)
                    sts = T.case_states(c)
                    raw = c["logits"].numpy()
                    for budget in TC.BUDGETS:
                        want = TC.rule_on_case(c, closure, budget)
                        for gi in range(G):
                            sl = slice(gi * W, (gi + 1) * W)
                            groups += 1
                            if not want["gap"][gi] > 1.0:
                                left += 1
                                continue
                            w = gi // T.GPW
                            par, tok = group_step_f32(form, close[w], cyc[w], budget, raw[sl], c["pad"][w], c["scores"][sl], c["fin"][sl] != 0,
                                                      sts[sl], CL.LOOPS, c["ntok"], c["term"], c["follows"][w])
                            assert np.array_equal(par, want["parent"][sl]) and np.array_equal(tok, want["tok"][sl]), (S, W, G, closure, budget, gi)
            ok = left <= CL.CAP * groups
            bad += not ok
            _say(lines, "operator S=%d %s seeds op_seed(S, W, G): left out %d of %d groups (%.2f %%) -> %s"
                 % (S, closure, left, groups, 100.0 * left / groups, "kept" if ok else "NOT kept"))
    return bad


def engine(lines, name, seed, form, W=4):
    """-> (not kept, own-anchor groups, of them with an enclosed best non-dead beam)."""
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    from constrained_left_out import oracle_step_logits
    from faceformer_amd import faces
    tok = token_ns()
    term, ntok = (tok.face_type_offset, tok.len), tok.len
    case, _ = load_golden(name)
    sd, gb = case_weights_and_batch(case)
    m = case["model"]
    batch, edges, _ = CR.lattice_batch(gb["num_input"], m["L"], m["seq_len"], seed)
    ni = batch["num_input"]
    follows = faces.follow_table(batch["input"].numpy(), CR.TOL, ni)
    N, F, T = len(ni), max(ni), m["seq_len"]
    close, cyc = faces.follow_distance(follows, max(T - 2, 1), ni)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    f32, f64 = float(np.finfo(np.float32).min), float(np.finfo(np.float64).min)
    G = N * F
    start = np.array([f if f < ni[w] else ntok - 1 for w in range(N) for f in range(F)], dtype=np.int64)
    st = [CL.start_group(start[g], W, ntok, term, follows[g // F]) for g in range(G)]
    sc = np.concatenate([s[0] for s in st]); fin = np.concatenate([s[1] for s in st]); dead = np.concatenate([s[2] for s in st])
    states = [x for s in st for x in s[3]]
    mask = batch["input_mask"].numpy().astype(bool)
    pads = np.concatenate([np.zeros((N, ntok), dtype=bool), mask], axis=1)
    toks, pars = [], []
    alive = np.ones(G, dtype=bool)
    pairs = left = 0
    for j in range(T - 1):
        prefixes = BR.backtrack(np.repeat(start, W), toks, pars, W)
        paths = np.zeros((G * W, T), dtype=np.int64)
        paths[:, : j + 1] = prefixes
        lg64 = np.stack([oracle_step_logits(case, sd64, b64, np.ascontiguousarray(paths[k::W]), j, F, f64) for k in range(W)], axis=1)
        lg32 = np.stack([oracle_step_logits(case, sd32, dict(batch), np.ascontiguousarray(paths[k::W]), j, F, f32) for k in range(W)], axis=1)
        ntok_j, npar_j, count = np.zeros(G * W, np.int64), np.tile(np.arange(W), G), 0
        for g in range(G):
            sl = slice(g * W, (g + 1) * W)
            if fin[sl][~np.isinf(sc[sl])].all():
                continue
            w = g // F
            a = (form, lg64[g], pads[w], sc[sl], fin[sl], dead[sl], states[sl], CL.LOOPS, ntok, term, follows[w], close[w], cyc[w], T - 2 - j)
            res = CL.group_step(*a, margin=j + 1)
            pairs += 1
            if alive[g] and res["gap"] > 1.0:
                r32 = CL.group_step(form, lg32[g].astype(np.float64), *a[2:])
                assert np.array_equal(r32["parent"], res["parent"]) and np.array_equal(r32["tok"], res["tok"]), (name, seed, form, j, g)
            else:
                alive[g] = False
                left += 1
            ntok_j[sl], npar_j[sl] = res["tok"], res["parent"]
            sc[sl], fin[sl], dead[sl] = res["scores"], res["fin"], res["dead"]
            states[sl] = res["states"]
            count += res["count"]
        toks.append(ntok_j); pars.append(npar_j)
        if count == 0:
            break
    beams = BR.backtrack(np.repeat(start, W), toks, pars, W).reshape(G, W, -1)
    own = [g for g in range(G) if g % F < ni[g // F]]
    enclosed = sum(CL.enclosed_best(beams[g], sc[g * W:(g + 1) * W], dead[g * W:(g + 1) * W], ntok, term, follows[g // F]) for g in own)
    ok = left <= CL.CAP * max(1, pairs)
    _say(lines, "engine %s seed %d %s, W = %d: %d steps, left out %d of %d (step, group) pairs (%.2f %%) -> %s; best non-dead beam "
                "enclosed in %d of %d own-anchor groups"
         % (name, seed, form, W, len(toks), left, pairs, 100.0 * left / max(1, pairs), "kept" if ok else "NOT kept", enclosed, len(own)))
    return (not ok), len(own), enclosed


def main(argv):
    os.makedirs(OUT, exist_ok=True)
    lines = []
    if "--engine" in argv:
        names = [a for a in argv if a != "--engine"] or list(CR.LATTICE_SEEDS)
        bad, counts = 0, {}
        for n in names:
            row = {}
            for closure, form in (("plain", "plain"), ("lookahead", "ahead"), ("exact", "exact")):
                b, groups, enclosed = engine(lines, n, CR.LATTICE_SEEDS[n], form)
                bad += b
                row["groups"], row[closure] = groups, enclosed
            counts[n] = row
        path = os.path.join(OUT, "yield.json")
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("oracle_W4", {}).update(counts)
        json.dump(doc, open(path, "w"), indent=1)
        open(os.path.join(OUT, "left_out_engine.txt"), "w").write("\n".join(lines) + "\n")
        return 1 if bad else 0
    bad = operator(lines)
    open(os.path.join(OUT, "left_out.txt"), "w").write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
