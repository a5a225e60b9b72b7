"""Shared by tests/test_forced.py and tools/forced_left_out.py: the numpy fp64 statement of what a teacher-forced step scores
(DESIGN.md 14), the seeded paths the engine tests force, and the comparison of a scored run with the fp64 oracle's logits."""
import numpy as np

FILL32 = float(np.finfo(np.float32).min)
FLT_MAX = float(np.finfo(np.float32).max)
LP_BAR = 2.0 ** -16
EPS = 2.0 ** -23
CAP = 0.02                    # share of scored (row, position) pairs that may leave the greedy / rank comparison, per golden
SEEDS = {"par_small_gain4": 11, "par_small_ragged": 32, "seq_full_A4_gain4": 13, "par_full_n40_gain4": 14}
SUBSET = {"par_full_n40_gain4": list(range(16))}      # rows the oracle evaluates (the HIP side scores the whole batch)


def forced_rule(masked, g):
    """masked [B, S] masked logits (masked keys at finfo.min of their dtype, or below), g [B] forced keys -> (logprob, greedy,
    rank) in fp64 / int64: logprob = (l[g] - m) - log sum exp(l - m) saturated at -FLT_MAX, greedy = first argmax, rank = keys
    above l[g] plus equal keys at a lower index."""
    l = np.maximum(np.asarray(masked, dtype=np.float64), -FLT_MAX)
    g = np.asarray(g, dtype=np.int64)
    rows = np.arange(l.shape[0])
    m = l.max(axis=1)
    with np.errstate(under="ignore"):
        lse = np.log(np.exp(l - m[:, None]).sum(axis=1))
    lg = l[rows, g]
    lp = np.maximum((lg - m) - lse, -FLT_MAX)
    rank = (l > lg[:, None]).sum(axis=1) + ((l == lg[:, None]) & (np.arange(l.shape[1])[None, :] < g[:, None])).sum(axis=1)
    return lp, l.argmax(axis=1), rank


def make_paths(case, seed, num_token=4, sos=1):
    """Seeded paths of a golden case: (paths [rows, T] int64, lengths [rows] int64, F).  Every token (the start tokens of the
    parallel model included; the seq2seq rows start from SOS) is drawn from the live keys of the row's wireframe -- the special
    tokens and its real edges: below kv_len, never padding -- at EVERY position, so that rows past their own length feed both
    sides the same tokens.  Lengths are drawn from 0..T-1; rows 0, 1, 2 get 0, 1 and T-1."""
    rng = np.random.default_rng([0xF0CED, int(seed)])
    T, n_edges = case["model"]["seq_len"], [int(n) for n in case["n_edges"]]
    parallel = case["kind"] == "parallel"
    F = max(n_edges) if parallel else 1
    rows = len(n_edges) * F
    live = np.array([num_token + n_edges[r // F] for r in range(rows)])
    paths = (rng.random((rows, T)) * live[:, None]).astype(np.int64)
    if not parallel:
        paths[:, 0] = sos
    lengths = rng.integers(0, T, size=rows)
    lengths[:3] = [0, 1, T - 1]
    return paths, lengths.astype(np.int64), F


def tol_of(truth_step, scale=40.0, base=1e-3):
    """tests/test_parity_golden.py's _tol of one step's reference logits (restated for the CPU tool, which imports no test)."""
    live = truth_step[truth_step > FILL32]
    return base * max(1.0, (float(np.abs(live).max()) if live.size else 1.0) / scale)


def compare(truth, rows, paths, lengths, got_logits, got_lp, got_greedy, got_rank, tol_fn=tol_of, what="", check=True):
    """truth [steps, len(rows), S] fp64 masked logits of the oracle forced along paths[rows]; got_* the scored run's traced
    logits [>= steps, B, S] and outputs [B, T].  Asserts the logit and logprob bars on every scored pair and greedy / rank
    equality wherever the truth is decisive (check=False, the seed tool: the two bars are measured only); returns dict(pairs,
    left_out (share), worst_logit, worst_lp: error / bar)."""
    pairs = left = 0
    worst_logit = worst_lp = 0.0
    for s in range(truth.shape[0]):
        tol = tol_fn(truth[s])
        for i, r in enumerate(rows):
            if s >= lengths[r]:
                continue
            t = truth[s, i]
            g = int(paths[r, s + 1])
            livek = t > FILL32
            h = np.asarray(got_logits[s, r], dtype=np.float64)
            assert np.array_equal(h > FILL32, livek), "%s: mask differs at step %d row %d" % (what, s, r)
            d = float(np.abs(h[livek] - t[livek]).max())
            worst_logit = max(worst_logit, d / tol)
            assert d <= tol or not check, "%s: step %d row %d: |dlogit| = %g > %g" % (what, s, r, d, tol)
            lp, gr, rk = forced_rule(t[None], [g])
            bar = 2 * tol + LP_BAR + EPS * abs(lp[0])
            e = abs(float(got_lp[r, s + 1]) - lp[0])
            worst_lp = max(worst_lp, e / bar)
            assert e <= bar or not check, "%s: step %d row %d: |dlogprob| = %g > %g" % (what, s, r, e, bar)
            srt = np.sort(t)
            margin = srt[-1] - srt[-2] if t.size > 1 else np.inf
            others = np.delete(t, g)
            near = others.size and float(np.abs(others - t[g]).min()) <= 2 * tol
            pairs += 1
            if margin <= 2 * tol or near:
                left += 1
            if margin > 2 * tol:
                assert int(got_greedy[r, s + 1]) == gr[0], "%s: step %d row %d: greedy %d, oracle %d" % (what, s, r, got_greedy[r, s + 1], gr[0])
            if not near:
                assert int(got_rank[r, s + 1]) == rk[0], "%s: step %d row %d: rank %d, oracle %d" % (what, s, r, got_rank[r, s + 1], rk[0])
    return dict(pairs=pairs, left_out=left / max(pairs, 1), worst_logit=worst_logit, worst_lp=worst_lp)
