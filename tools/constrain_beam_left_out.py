"""Which seeds tests/test_constrain_beam.py may use (CPU only): the share of cases left out as indecisive is a condition on the
RULE, fixed here before any GPU result is looked at.

  operator   (default) exactly the test's launches (test_constrain_beam.operator_case over OP_S x OP_W x OP_G x the four flag
             combinations, seed op_seed(S, W, G)): the numpy rule evaluated on the fp32 logits in fp64 gives every group's
             smallest decisive gap in units of twice the score bound (constrain_beam_ref.group_step); a group is left out when
             that is at most 1.  The rule is also evaluated with fp32 arithmetic (the row's log-softmax and the score additions
             in float32), and its parents and tokens must equal the fp64 rule's on every kept group.  Kept when the share per S
             is at most constrain_beam_ref.CAP.
  --engine   per (golden, lattice seed) of constrain_ref.LATTICE_SEEDS: the fp64 oracle (oracle/refpath.py, forced=) decodes
             the lattice wireframes under "loops" with W = 4 beams on the CPU -- at every step it is forced along the
             back-tracked prefixes of the beams, the numpy rule is applied to its logits with j x the bound at step j -- and
             the fp32 oracle is forced along the same prefixes: a (step, group) pair is left out when the fp64 rule's gap is at
             most 1, and from a group's first such pair on; on every kept pair the fp32 oracle's logits must select what the
             fp64 oracle's do.  Kept when the share is at most CAP.

A seed is changed, never the cap.  Non-zero exit when a listed seed fails.

    python tools/constrain_beam_left_out.py [--engine [golden ...]]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import beam_ref as BR  # noqa: E402
import constrain_beam_ref as CBR  # noqa: E402
import constrain_ref as CR  # noqa: E402


def group_step_f32(raw, pad, scores, fin, states, flags, ntok, term, follows):
    """(parent, tok) of constrain_beam_ref.group_step's selection with the kernel's arithmetic in float32."""
    W, S = raw.shape
    scs, ixs = [], []
    for k in range(W):
        if scores[k] == -np.inf:
            continue
        if fin[k]:
            scs.append(np.array([scores[k]], dtype=np.float32)); ixs.append(np.array([k * S]))
            continue
        masked, _ = CR.rule_mask(states[k], flags, S, ntok, term, follows, pad)
        row = np.where(masked | pad, np.float32(CR.FILL), raw[k].astype(np.float32))
        m = row.max()
        logz = np.log(np.exp(row - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32)
        live = row > np.float32(CR.FILL)
        c = np.float32(scores[k])
        if not live.any():
            scs.append(np.array([c - logz], dtype=np.float32)); ixs.append(np.array([k * S]))
            continue
        scs.append(np.maximum(c + ((row[live] - m) - logz), np.float32(CR.FILL))); ixs.append(k * S + np.nonzero(live)[0])
    sc = np.concatenate(scs) if scs else np.zeros(0, np.float32)
    ix = np.concatenate(ixs) if ixs else np.zeros(0, np.int64)
    order = np.lexsort((ix, -sc.astype(np.float64)))[:W]
    par, tok = np.arange(W), np.zeros(W, dtype=np.int64)
    for r, i in enumerate(order):
        k, s = divmod(int(ix[i]), S)
        par[r], tok[r] = k, (0 if fin[k] else s)
    return par, tok


def operator():
    import test_constrain_beam as T
    bad = 0
    for S in T.OP_S:
        groups = left = 0
        for W in T.OP_W:
            if W > S:
                continue
            for G in T.OP_G:
                c = T.operator_case(G, W, S, T.op_seed(S, W, G))
                sts = T.case_states(c)
                raw = c["logits"].numpy()
                for flags in T.ALL_FLAGS:
                    want = T.rule_on_case(c, flags)
                    for gi in range(G):
                        sl = slice(gi * W, (gi + 1) * W)
                        groups += 1
                        if not want["gap"][gi] > 1.0:
                            left += 1
                            continue
                        w = gi // T.GPW
                        par, tok = group_step_f32(raw[sl], c["pad"][w], c["scores"][sl], c["fin"][sl] != 0, sts[sl], flags, c["ntok"],
                                                  c["term"], c["follows"][w])
                        assert np.array_equal(par, want["parent"][sl]) and np.array_equal(tok, want["tok"][sl]), (S, W, G, flags, gi)
        ok = left <= CBR.CAP * groups
        bad += not ok
        print("operator S=%d seeds op_seed(S, W, G): left out %d of %d groups (%.2f %%) -> %s"
              % (S, left, groups, 100.0 * left / groups, "kept" if ok else "NOT kept"))
    return bad


def engine(name, seed, W=4):
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
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    f32, f64 = float(np.finfo(np.float32).min), float(np.finfo(np.float64).min)
    loops = CR.NO_REPEAT | CR.CONNECT
    N, F, T = len(ni), max(ni), m["seq_len"]
    G = N * F
    start = np.array([f if f < ni[w] else ntok - 1 for w in range(N) for f in range(F)], dtype=np.int64)
    st = [CBR.start_group(start[g], W, ntok, term, follows[g // F]) for g in range(G)]
    sc = np.concatenate([s[0] for s in st]); fin = np.concatenate([s[1] for s in st]); dead = np.concatenate([s[2] for s in st])
    states = [x for s in st for x in s[3]]
    mask = batch["input_mask"].numpy().astype(bool)
    pads = np.concatenate([np.zeros((N, ntok), dtype=bool), mask], axis=1)       # the keys masked by padding, [N, S]
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
            pad = pads[g // F]
            res = CBR.group_step(lg64[g], pad, sc[sl], fin[sl], dead[sl], states[sl], loops, ntok, term, follows[g // F], margin=j + 1)
            pairs += 1
            if alive[g] and res["gap"] > 1.0:
                r32 = CBR.group_step(lg32[g].astype(np.float64), pad, sc[sl], fin[sl], dead[sl], states[sl], loops, ntok, term, follows[g // F])
                assert np.array_equal(r32["parent"], res["parent"]) and np.array_equal(r32["tok"], res["tok"]), (name, seed, j, g)
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
    ok = left <= CBR.CAP * max(1, pairs)
    print("engine %s seed %d, W = %d: %d steps, left out %d of %d (step, group) pairs (%.2f %%) -> %s"
          % (name, seed, W, len(toks), left, pairs, 100.0 * left / max(1, pairs), "kept" if ok else "NOT kept"))
    return not ok


def main(argv):
    if "--engine" in argv:
        names = [a for a in argv if a != "--engine"] or list(CR.LATTICE_SEEDS)
        return 1 if sum(engine(n, CR.LATTICE_SEEDS[n]) for n in names) else 0
    return 1 if operator() else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
