"""Whether tests/test_lookahead.py may use the (golden, lattice seed) pairs of constrain_ref.LATTICE_SEEDS (CPU only).

tools/constrained_left_out.py under the closure look-ahead: the oracle (oracle/refpath.py, forced=) decodes the
lattice wireframes under constrain "loops" with the look-ahead of tests/lookahead_ref.py -- the step that selects position p
masks with budget = T - 1 - p against faces.follow_distance(follows, hmax = max(T - 2, 1)).  Every row runs to its own finish
position or T - 1 steps.  Two conditions per pair, both on the oracle ALONE:

  left out   the fp32 oracle decodes under the rule; the fp64 oracle is teacher-forced along those tokens; a (step, unfinished
             row) pair is left out of the token comparison when the fp64 row's margin between its two best LIVE keys of the
             constrained row is at most 2 tol(step) (tests/test_parity_golden._tol on the fp64 row).  Kept when the share is
             at most constrain_ref.CAP.
  enclosed   of the fp64 oracle's own decode under the rule: the share of own-anchor rows that end in a terminator without a
             dead-end flag and pass faces.is_face_enclosed.  Kept when at least TWICE lookahead_ref.MIN_ENCLOSED; on
             par_small_ragged also strictly more rows than under "loops" alone (the test asks the GPU decode for both).

Also printed: enclosed / dead-ended / other own-anchor rows under "loops" and with the look-ahead, the rows whose tokens change
(the yield table of DESIGN.md 22), and whether every row ends closed or flagged.  Non-zero exit when a listed pair fails.

    python tools/lookahead_left_out.py [golden ...] [--seeds 1 2 3]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import constrain_ref as CR  # noqa: E402
import lookahead_ref as LR  # noqa: E402
from constrained_left_out import constrained_decode, oracle_step_logits, yield_of  # noqa: E402

LOOPS = CR.NO_REPEAT | CR.CONNECT


def lookahead_decode(case, sd, b, ni, follows, close, cycle, tok, fill):
    """The oracle's own decode under "loops" with the look-ahead.  -> (paths [N*F, T], dead [N*F])."""
    N, F, T = len(ni), max(ni), case["model"]["seq_len"]
    term, ntok = (tok.face_type_offset, tok.len), tok.len
    paths = np.zeros((N * F, T), dtype=np.int64)
    for w in range(N):
        for f in range(F):
            paths[w * F + f, 0] = f if f < ni[w] else ntok - 1
    state = [CR.start_state(int(paths[r, 0]), ntok, follows[r // F]) for r in range(N * F)]
    fin = np.array([term[0] <= paths[r, 0] < term[1] for r in range(N * F)])
    dead = np.zeros(N * F, dtype=bool)
    for j in range(T - 1):
        if fin.all():
            break
        lg = oracle_step_logits(case, sd, b, paths, j, F, fill)
        for r in np.flatnonzero(~fin):
            w = r // F
            res = LR.step_row(lg[r], lg[r] <= CR.FILL, state[r], LOOPS, ntok, term, follows[w], close[w], cycle[w], T - 2 - j)
            paths[r, j + 1], state[r], fin[r] = res["tok"], res["state"], res["fin"]
            dead[r] |= res["dead"]
    return paths, dead


def check(name, seed):
    import torch
    from conftest import case_weights_and_batch, load_golden, token_ns
    from faceformer_amd import faces
    from test_parity_golden import _tol
    tok = token_ns()
    term, ntok = (tok.face_type_offset, tok.len), tok.len
    case, _ = load_golden(name)
    sd, gb = case_weights_and_batch(case)
    m = case["model"]
    batch, edges, _ = CR.lattice_batch(gb["num_input"], m["L"], m["seq_len"], seed)
    ni = batch["num_input"]
    F, T = max(ni), m["seq_len"]
    follows = faces.follow_table(batch["input"].numpy(), CR.TOL, ni)
    close, cycle = faces.follow_distance(follows, max(T - 2, 1), ni)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in batch.items()}
    f32, f64 = float(np.finfo(np.float32).min), float(np.finfo(np.float64).min)
    # left out: the fp32 oracle's decode, the fp64 oracle along it
    p32, _ = lookahead_decode(case, sd32, dict(batch), ni, follows, close, cycle, tok, f32)
    fin, _ = CR.stop_and_finish(p32, term, ntok)
    pairs = left = 0
    for j in range(int(min(T - 1, fin.max()))):
        lg = oracle_step_logits(case, sd64, b64, p32, j, F, f64)
        live_rows = np.flatnonzero(fin > j)
        if not live_rows.size:
            continue
        tol = _tol(np.where(lg[live_rows] > CR.FILL, lg[live_rows], np.finfo(np.float32).min))
        for r in live_rows:
            w = r // F
            st = CR.state_of_prefix(p32[r, : j + 1], ntok, follows[w])
            res = LR.step_row(lg[r], lg[r] <= CR.FILL, st, LOOPS, ntok, term, follows[w], close[w], cycle[w], T - 2 - j)
            live = np.sort(res["row"][res["row"] > CR.FILL])
            pairs += 1
            left += (live[-1] - live[-2] if live.size > 1 else np.inf) <= 2 * tol
    share = left / max(1, pairs)
    # yield: the fp64 oracle's own decodes under "loops" and with the look-ahead
    p_loops, d_loops, _ = constrained_decode(case, sd64, b64, ni, follows, LOOPS, tok, f64)
    p_ahead, d_ahead = lookahead_decode(case, sd64, b64, ni, follows, close, cycle, tok, f64)
    before = yield_of(p_loops, d_loops, ni, edges, tok, CR.TOL)
    after = yield_of(p_ahead, d_ahead, ni, edges, tok, CR.TOL)
    own_rows = [w * F + f for w, n in enumerate(ni) for f in range(n)]
    changed = sum(1 for r in own_rows if not np.array_equal(p_loops[r], p_ahead[r]))
    fin64, _ = CR.stop_and_finish(p_ahead, term, ntok)
    open_rows = [r for r in own_rows if not d_ahead[r]
                 and CR.state_of_prefix(p_ahead[r, : int(min(fin64[r], T - 1)) + 1], ntok, follows[r // F])[1] is not None]
    own = sum(ni)
    ok = share <= CR.CAP and after[0] >= 2 * LR.MIN_ENCLOSED * own and not open_rows
    if name == "par_small_ragged":
        ok = ok and after[0] > before[0]
    print("%s seed %d (T = %d): left out %d of %d pairs (%.2f %%); own-anchor rows enclosed / dead end / other of %d: loops %d / %d / %d, "
          "with look-ahead %d / %d / %d (%.1f %% enclosed); rows whose tokens change: %d; rows ending open without the flag: %d  -> %s"
          % ((name, seed, T, left, pairs, 100 * share, own) + before + after
             + (100.0 * after[0] / own, changed, len(open_rows), "kept" if ok else "NOT kept")))
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
