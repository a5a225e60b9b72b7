"""Which (golden, lattice seed) pairs tests/test_constrain.py may use (CPU only).

The oracle (oracle/refpath.py, forced=) decodes the lattice wireframes of tests/constrain_ref.py under the constrained rule on
the CPU: at every step it is forced along the tokens selected so far, the numpy rule (constrain_ref.step_row) is applied to
its masked logits, and the selected token is appended.  Every row runs to its own finish position or T - 1 steps (the batch's
stop step is not applied: a superset of the pairs a decode makes).  Two conditions per pair, both on the oracle ALONE:

  left out   the fp32 oracle decodes under "loops"; the fp64 oracle is teacher-forced along those tokens; a (step, unfinished
             row) pair is left out of the token comparison when the fp64 row's margin between its two best LIVE keys of the
             constrained row is at most 2 tol(step) (tests/test_parity_golden._tol on the fp64 row).  Kept when the share is
             at most constrain_ref.CAP.
  enclosed   of the fp64 oracle's own "loops" decode: the share of own-anchor rows that end in a terminator without a dead-end
             flag and pass faces.is_face_enclosed on the lattice's edges.  Kept when at least TWICE constrain_ref.MIN_ENCLOSED
             (the test asks the GPU decode for MIN_ENCLOSED: see constrain_ref).

Also printed: the share of rows enclosed / dead-ended / unclosed with and without "loops" (the yield table of DESIGN.md 16).
A seed is changed, never a cap.  Non-zero exit when a listed pair fails.

    python tools/constrained_left_out.py [golden ...] [--seeds 1 2 3]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import constrain_ref as CR  # noqa: E402


def oracle_step_logits(case, sd, b, paths, step, F, fill):
    """[rows, S] masked logits (as fp64 numpy, masked keys at constrain_ref.FILL) of step `step` of the oracle forced along `paths`."""
    import torch
    from oracle import refpath
    tr = {}
    refpath.parallel_forward_eval(sd, dict(b), num_head=case["model"]["H"], trace=tr, forced=torch.from_numpy(paths), steps=step + 1,
                                  num_anchors=F)
    lg = tr["logits"][step].double().numpy()
    return np.where(lg > fill, lg, CR.FILL)


def constrained_decode(case, sd, b, ni, follows, flags, tok, fill):
    """The oracle's own constrained decode.  -> (paths [N*F, T], dead [N*F], rows [T-1, N*F, S] the constrained rows it selected from)."""
    N, F, T = len(ni), max(ni), case["model"]["seq_len"]
    term, ntok = (tok.face_type_offset, tok.len), tok.len
    paths = np.zeros((N * F, T), dtype=np.int64)
    for w in range(N):
        for f in range(F):
            paths[w * F + f, 0] = f if f < ni[w] else ntok - 1
    state = [CR.start_state(int(paths[r, 0]), ntok, follows[r // F]) for r in range(N * F)]
    fin = np.array([term[0] <= paths[r, 0] < term[1] for r in range(N * F)])
    dead = np.zeros(N * F, dtype=bool)
    rows = None
    for j in range(T - 1):
        if fin.all():
            break
        lg = oracle_step_logits(case, sd, b, paths, j, F, fill)
        if rows is None:
            rows = np.full((T - 1,) + lg.shape, np.nan)
        for r in np.flatnonzero(~fin):
            pad = lg[r] <= CR.FILL
            res = CR.step_row(lg[r], pad, state[r], flags, ntok, term, follows[r // F])
            paths[r, j + 1], state[r], fin[r], rows[j, r] = res["tok"], res["state"], res["fin"], res["row"]
            dead[r] |= res["dead"]
    return paths, dead, rows


def yield_of(paths, dead, ni, edges, tok, tol):
    """(enclosed, dead-ended, unclosed) counts over the own-anchor rows."""
    from faceformer_amd import faces
    F = paths.shape[0] // len(ni)
    enc = de = un = 0
    for w, n in enumerate(ni):
        for f in range(n):
            row = paths[w * F + f]
            face = faces._parallel_rows(row[None], tok, n)
            ends = ((row >= tok.face_type_offset) & (row < tok.len)).any()
            if dead[w * F + f]:
                de += 1
            elif ends and face and faces.is_face_enclosed(edges[w], face[0][1], tol):
                enc += 1
            else:
                un += 1
    return enc, de, un


def check(name, seed):
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    from faceformer_amd import faces
    from test_parity_golden import _tol
    tok = token_ns()
    case, _ = load_golden(name)
    sd, gb = case_weights_and_batch(case)
    m = case["model"]
    batch, edges, _ = CR.lattice_batch(gb["num_input"], m["L"], m["seq_len"], seed)
    ni = batch["num_input"]
    follows = faces.follow_table(batch["input"].numpy(), CR.TOL, ni)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b32 = dict(batch)
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    f32, f64 = float(np.finfo(np.float32).min), float(np.finfo(np.float64).min)
    loops = CR.NO_REPEAT | CR.CONNECT
    # left out: the fp32 oracle's decode, the fp64 oracle along it
    p32, d32, _ = constrained_decode(case, sd32, b32, ni, follows, loops, tok, f32)
    F, T = max(ni), m["seq_len"]
    fin, _ = CR.stop_and_finish(p32, (tok.face_type_offset, tok.len), tok.len)
    pairs = left = 0
    last = int(min(T - 1, fin.max()))
    for j in range(last):
        lg = oracle_step_logits(case, sd64, b64, p32, j, F, f64)
        live_rows = np.flatnonzero(fin > j)
        if not live_rows.size:
            continue
        tol = _tol(np.where(lg[live_rows] > CR.FILL, lg[live_rows], np.finfo(np.float32).min))
        for r in live_rows:
            st = CR.state_of_prefix(p32[r, : j + 1], tok.len, follows[r // F])
            res = CR.step_row(lg[r], lg[r] <= CR.FILL, st, loops, tok.len, (tok.face_type_offset, tok.len), follows[r // F])
            live = np.sort(res["row"][res["row"] > CR.FILL])
            margin = live[-1] - live[-2] if live.size > 1 else np.inf
            pairs += 1
            left += margin <= 2 * tol
    share = left / max(1, pairs)
    # enclosed: the fp64 oracle's own decode, with and without the constraint
    out = {}
    for label, flags in (("greedy", 0), ("no_repeat", CR.NO_REPEAT), ("loops", loops)):
        p64, d64, _ = constrained_decode(case, sd64, b64, ni, follows, flags, tok, f64)
        out[label] = yield_of(p64, d64, ni, edges, tok, CR.TOL)
    own = sum(ni)
    enclosed = out["loops"][0] / own
    ok = share <= CR.CAP and enclosed >= 2 * CR.MIN_ENCLOSED
    print("%s seed %d: left out %d of %d pairs (%.2f %%); own-anchor rows enclosed / dead end / unclosed of %d: %s  -> %s"
          % (name, seed, left, pairs, 100 * share, own,
             ", ".join("%s %d / %d / %d" % ((k,) + v) for k, v in out.items()), "kept" if ok else "NOT kept"))
    return ok


def main(argv):
    seeds = None
    if "--seeds" in argv:
        i = argv.index("--seeds")
        seeds = [int(s) for s in argv[i + 1:]]
        argv = argv[:i]
    names = argv or list(CR.LATTICE_SEEDS)
    bad = 0
    for name in names:
        for seed in (seeds if seeds is not None else [CR.LATTICE_SEEDS[name]]):
            ok = check(name, seed)
            bad += (not ok) and seeds is None
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
