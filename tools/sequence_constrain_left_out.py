"""Which (golden, kind, seed, flags) triples tests/test_sequence_constrain.py may use (CPU only).

The oracle (oracle/refpath.seq2seq_forward_eval, forced= / trace=) decodes the fixtures of tests/sequence_constrain_ref.py under the
single-sequence loop rule on the CPU: at every step it is forced along the tokens selected so far, the numpy rule
(faces.sequence_rule_step) is applied to its masked logits, and the selected token is appended.  One condition per triple, on the
oracle ALONE:

  left out   the fp32 oracle decodes under the rule; the fp64 oracle is teacher-forced along those tokens; a (step, unfinished row)
             pair is left out of the token comparison when the fp64 row's margin between its two best LIVE keys of the constrained
             row is at most 2 tol(step) (tests/test_parity_golden._tol on the fp64 rows of the step).  Kept when the share is at
             most sequence_constrain_ref.CAP.

Printed per triple, in the form of sequence_constrain_ref.KEPT: left-out pairs, pairs, enclosed faces (faces.is_face_enclosed on the
lattice's float32 end points; on the table itself for a random table), parsed faces (faces.parse_faces), dead ends; and whether
the fp32 and the fp64 oracle select the same tokens, with how the rows ended.  Also the greedy decode's enclosed / parsed counts
(the yield table of DESIGN.md 32).  A seed is changed, never a cap.  Non-zero exit when a listed triple fails or KEPT differs.

    python tools/sequence_constrain_left_out.py [--write]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sequence_constrain_ref as SC  # noqa: E402


def oracle_step(case, sd, b, tok, fill):
    """step_logits(paths, step) of sequence_constrain_ref.decode on the oracle: masked keys at SC.FILL."""
    import torch
    from oracle import refpath

    def step_logits(paths, step):
        tr = {}
        refpath.seq2seq_forward_eval(sd, dict(b), num_head=case["model"]["H"], label_seq_length=case["model"]["seq_len"],
                                     token_sos=tok.SOS, token_eos=tok.EOS, trace=tr, forced=torch.from_numpy(paths), steps=step + 1)
        lg = tr["logits"][step].double().numpy()
        return np.where(lg > fill, lg, SC.FILL)
    return step_logits


def enclosed_of(tokens, dead, ni, tok, edges, follows):
    """(enclosed, parsed) over the rows' parsed faces; without edges the walk runs on the table itself."""
    from faceformer_amd import faces
    enc = par = 0
    for w, n in enumerate(ni):
        for idx, _, _ in SC.face_pieces(tokens[w], dead[w], tok.len, tok.SEP, tok.EOS, n):
            par += 1
            enc += bool(walk_closed(idx, follows[w]) if edges is None else faces.is_face_enclosed(edges[w], idx, SC.TOL))
    return enc, par


def walk_closed(idx, table):
    """faces.is_face_enclosed's walk on a follow table."""
    first = prev = None
    for e in idx:
        if first is None:
            first = e
        elif not table[prev][e]:
            return False
        prev = e
        if table[e][first]:
            first = None
    return first is None


def check(name, kind, seed, flags):
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    from test_parity_golden import _tol
    tok = token_ns()
    case, _ = load_golden(name)
    sd, gb = case_weights_and_batch(case)
    m = case["model"]
    batch, follows, edges = SC.fixture(case, gb, kind, seed)
    ni, N, T = batch["num_input"], len(batch["num_input"]), m["seq_len"]
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    f32, f64 = float(np.finfo(np.float32).min), float(np.finfo(np.float64).min)
    args = (N, T, flags, tok.len, tok.SOS, tok.SEP, tok.EOS, follows)
    d32 = SC.decode(oracle_step(case, sd32, batch, tok, f32), *args)
    p32 = d32["tokens"]
    fin, steps = SC.stop_and_finish(p32, tok.EOS)
    step64 = oracle_step(case, sd64, b64, tok, f64)
    states = SC.replay_states(p32, flags, tok.len, tok.SEP, follows)
    from faceformer_amd import faces
    pairs = left = 0
    same = True
    for j in range(steps):
        lg = step64(p32, j)
        live_rows = np.flatnonzero(fin > j)
        tol = _tol(np.where(lg[live_rows] > SC.FILL, lg[live_rows], np.finfo(np.float32).min))
        for r in live_rows:
            res = faces.sequence_rule_step(lg[r], lg[r] <= SC.FILL, states[r][j], flags, tok.len, tok.SEP, tok.EOS, follows[r])
            pairs += 1
            left += SC.margin(res["row"]) <= 2 * tol
            same = same and res["tok"] == p32[r, j + 1]
    enc, par = enclosed_of(p32, d32["dead"], ni, tok, edges, follows)
    g = SC.decode(oracle_step(case, sd64, b64, tok, f64), N, T, 0, tok.len, tok.SOS, tok.SEP, tok.EOS, follows)
    genc, gpar = enclosed_of(g["tokens"], g["dead"], ni, tok, edges, follows)
    ends = ", ".join("EOS at %d" % f if f < T else ("open at T" if o else "closed at T") for f, o in zip(fin, d32["open_end"]))
    rec = (int(left), int(pairs), int(enc), int(par), int(d32["dead"].sum()))
    ok = left <= SC.CAP * max(1, pairs)
    print("    (%r, %r, %d, %d): %r,   # greedy %d of %d; fp32 = fp64 tokens: %s; steps %d; %s%s"
          % (name, kind, seed, flags, rec, genc, gpar, same, steps, ends, "" if ok else "  NOT kept"))
    return ok, rec


def main(argv):
    bad = 0
    for name, kind, seed in SC.FIXTURES:
        for flags in SC.FLAGS:
            ok, rec = check(name, kind, seed, flags)
            key = (name, kind, seed, flags)
            bad += not ok
            if "--write" not in argv and SC.KEPT.get(key) != rec:
                print("      ^ differs from sequence_constrain_ref.KEPT: %r" % (SC.KEPT.get(key),))
                bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
