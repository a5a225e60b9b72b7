"""Which (golden, lattice seed) pairs tests/test_constrain_exact.py may use (CPU only).

tools/lookahead_left_out.py under the exact closure look-ahead: the oracle (oracle/refpath.py, forced=) decodes the
lattice wireframes under constrain "loops" with the rule of tests/exact_ref.py -- the step that selects position p masks with
budget = T - 1 - p: while a loop is open by faces.closure_distance on the row's own visited set, with it closed by cycle_len of
faces.follow_distance(follows, hmax = max(T - 2, 1)).  Three conditions per pair, all on the oracle ALONE:

  (a) left out   the fp32 oracle decodes under the exact rule; the fp64 oracle is teacher-forced along those tokens; a (step,
                 unfinished row) pair is left out when the fp64 row's margin between its two best LIVE keys is at most
                 2 tol(step) (tests/test_parity_golden._tol on the fp64 row).  Kept when NO pair is left out.
  (b) late       under the STATIC look-ahead (tests/lookahead_ref.py) the fp64 oracle's own decode has at least one late dead
                 end: a dead end raised at a position whose previous position did not open the current loop.
  (c) exact      under the exact rule it has none, and strictly more own-anchor rows end enclosed than under the static one.

A pair is "kept" on (a), (b) and (c); "kept on (a)" when only (a) holds -- one fixture may be used that way if the other two are
kept in full.  Also printed: enclosed / dead-ended / other own-anchor rows and the late dead ends under "loops", the static
look-ahead and the exact rule (the oracle column of DESIGN.md 25's yield table).

    python tools/exact_left_out.py [golden ...] [--seeds 1 2 3]

Without --seeds the seeds of exact_ref.LATTICE_SEEDS are checked and the exit status is non-zero when one fails (a), or more than
one fails (b) or (c)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import constrain_ref as CR  # noqa: E402
import exact_ref as ER  # noqa: E402
from constrained_left_out import constrained_decode, oracle_step_logits, yield_of  # noqa: E402
from lookahead_left_out import lookahead_decode  # noqa: E402

LOOPS = ER.LOOPS


def exact_decode(case, sd, b, ni, follows, cycle, tok, fill):
    """The oracle's own decode under "loops" with the exact look-ahead.  -> (paths [N*F, T], dead [N*F])."""
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
            res = ER.step_row(lg[r], lg[r] <= CR.FILL, state[r], ntok, term, follows[w], cycle[w], T - 2 - j)
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
    # (a) left out: the fp32 oracle's decode, the fp64 oracle along it
    p32, _ = exact_decode(case, sd32, dict(batch), ni, follows, cycle, tok, f32)
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
            res = ER.step_row(lg[r], lg[r] <= CR.FILL, st, ntok, term, follows[w], cycle[w], T - 2 - j)
            live = np.sort(res["row"][res["row"] > CR.FILL])
            pairs += 1
            left += (live[-1] - live[-2] if live.size > 1 else np.inf) <= 2 * tol
    # (b), (c): the fp64 oracle's own decodes under "loops", the static look-ahead and the exact rule
    own_rows = [w * F + f for w, n in enumerate(ni) for f in range(n)]
    p_loops, d_loops, _ = constrained_decode(case, sd64, b64, ni, follows, LOOPS, tok, f64)
    p_ahead, d_ahead = lookahead_decode(case, sd64, b64, ni, follows, close, cycle, tok, f64)
    p_exact, d_exact = exact_decode(case, sd64, b64, ni, follows, cycle, tok, f64)
    rows = {}
    for what, (p, d) in (("loops", (p_loops, d_loops)), ("look-ahead", (p_ahead, d_ahead)), ("exact", (p_exact, d_exact))):
        own_dead = np.zeros(len(d), dtype=bool)
        own_dead[own_rows] = np.asarray(d)[own_rows]
        late = [r for w in range(len(ni)) for r in ER.late_dead_ends(p[w * F:(w + 1) * F], own_dead[w * F:(w + 1) * F], ntok, follows[w])]
        rows[what] = yield_of(p, d, ni, edges, tok, CR.TOL) + (len(late),)
    a = left == 0
    b = rows["look-ahead"][3] >= 1
    c = rows["exact"][3] == 0 and rows["exact"][0] > rows["look-ahead"][0]
    verdict = "kept" if a and b and c else ("kept on (a)" if a else "NOT kept")
    print("%s seed %d (T = %d): left out %d of %d pairs; own-anchor rows enclosed / dead end / other / late dead ends of %d: "
          "loops %d / %d / %d / %d, look-ahead %d / %d / %d / %d, exact %d / %d / %d / %d  -> (a) %s (b) %s (c) %s: %s"
          % ((name, seed, T, left, pairs, sum(ni)) + rows["loops"] + rows["look-ahead"] + rows["exact"]
             + ("yes" if a else "no", "yes" if b else "no", "yes" if c else "no", verdict)))
    return a, a and b and c


def main(argv):
    seeds = None
    if "--seeds" in argv:
        i = argv.index("--seeds")
        seeds = [int(s) for s in argv[i + 1:]]
        argv = argv[:i]
    names = argv or list(ER.LATTICE_SEEDS)
    fail_a = partial = 0
    for name in names:
        for seed in (seeds if seeds is not None else [ER.LATTICE_SEEDS[name]]):
            a, full = check(name, seed)
            if seeds is None:
                fail_a += not a
                partial += a and not full
    return 1 if fail_a or partial > 1 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
