"""The sampling rule of the pointer head in numpy fp64, with the guard band that says where an fp32 evaluation
may legitimately differ.

One unfinished row: l[0..S) the masked logit row (masked keys at -FLT_MAX), A the live keys, m = max l, u in [0, 1 - 2^-24]:
  A empty -> token 0, logprob -log S;  tau == 0 -> argmax (lowest index);  else w = exp((l - m) / tau) over A,
  top-k (0 < K < |A|): keep l >= v_K (K-th largest with multiplicity, ties kept);  top-p (P < 1): theta = the first distinct
  value, descending, whose mass reaches P * (kept mass), keep l >= theta;  c = inclusive prefix sums of w over the kept keys in
  index order, Z the last; token = first kept s with c[s] > u Z, else the last kept key.
  logprob = (l[tok] - m) - log sum_s exp(l[s] - m) over all S keys (under the model, not the shaped distribution).

Guard band (the issue's): beta = 2^-22 (sum_{kept} w (1 + |x|) + 8 Z), x = (l - m) / tau.  First term: the fp32 rounding of x (a
subtraction, a division, the log2(e) product: |x| 2^-22 relative on w) and v_exp_f32's ~2 ulp; second: at most 32 dependent fp32
additions and the product u Z.  The kernel's scan is a six-round wave scan per 64 keys plus one carried addition per chunk,
ceil(S / 64) + 6 <= 32 for S <= 1664, and its top-p mass is ceil(S / 64) sequential additions plus six butterfly rounds, the same
depth: the term stands as stated.  A DRAW is decisive when u Z is farther than beta from every c[s]; a top-p CUT when
P * (kept mass) is farther than beta (taken over the keys top-k kept) from every value-group boundary.  top-k is exact."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
FILL = -FLT_MAX
EPS = 2.0 ** -23
LP_BAR = 2.0 ** -16          # |logprob - fp64| <= LP_BAR + EPS |logprob| on the kernel's own logits
U_MAX = 1.0 - 2.0 ** -24
CAP = 0.02                   # at most this share of a case's rows / pairs may be indecisive

# The engine replay's (golden, seed, parameter set) triples at R = REPLAY_R draws per anchor: kept only because the fp32 oracle
# alone, forced along its own sampled paths on the CPU, leaves out less than CAP of the pairs (tools/sample_left_out.py; the
# shares are listed in DESIGN.md 15).  SUBSET: the anchor rows the CPU oracle evaluates (the GPU side decodes the whole batch).
REPLAY_R = 4
REPLAY_PARAMS = [(1.0, 0, 1.0), (0.8, 16, 0.9)]
REPLAY_SEEDS = {"par_small_gain4": 5, "par_small_ragged": 5, "par_full_n40_gain4": 5}
SUBSET = {"par_full_n40_gain4": list(range(16))}


def make_uniforms(num_input, T, R, seed):
    """uniforms [T-1, N*F*R] fp32 (CPU tensor) of a seeded sampled decode: column (w*F + f)*R + k."""
    import torch
    ni = [int(n) for n in num_input]
    return torch.rand((T - 1, len(ni) * max(ni) * R), generator=torch.Generator().manual_seed(seed))


def clamp_u(u):
    u = float(u)
    return min(max(u if u == u else 0.0, 0.0), U_MAX)


def logprob_of(l, tok):
    l = np.asarray(l, dtype=np.float64)
    m = l.max()
    return max((l[tok] - m) - np.log(np.exp(l - m).sum()), FILL)


def sample_row(l, u, tau=1.0, K=0, P=1.0, finished=False):
    """-> dict(tok, logprob, kept_k [S] bool, kept [S] bool, decisive, drew).  `decisive` covers the cut and the draw."""
    l = np.asarray(l, dtype=np.float64)
    S = l.shape[0]
    none = np.zeros(S, dtype=bool)
    if finished:
        return dict(tok=0, logprob=0.0, kept_k=none, kept=none, decisive=True, drew=False)
    live = l > FILL
    if not live.any():
        return dict(tok=0, logprob=-np.log(S), kept_k=none, kept=none, decisive=True, drew=False)
    m = l.max()
    if tau == 0:
        tok = int(np.argmax(l))
        return dict(tok=tok, logprob=logprob_of(l, tok), kept_k=live, kept=live, decisive=True, drew=False)
    x = np.where(live, (l - m) / tau, -np.inf)
    w = np.where(live, np.exp(x), 0.0)
    kept = live.copy()
    nA = int(live.sum())
    if 0 < K < nA:
        vK = np.sort(l[live])[::-1][K - 1]
        kept &= l >= vK
    kept_k = kept.copy()
    decisive = True
    if P < 1:
        xa = np.where(kept_k, np.abs(x), 0.0)
        zk = w[kept_k].sum()
        beta_k = 2.0 ** -22 * ((w * (1 + xa))[kept_k].sum() + 8 * zk)
        vals = np.unique(l[kept_k])[::-1]
        cum = np.array([w[kept_k & (l >= v)].sum() for v in vals])
        target = P * zk
        g = int(np.argmax(cum >= target)) if (cum >= target).any() else len(vals) - 1
        kept &= l >= vals[g]
        decisive = bool((np.abs(cum - target) > beta_k).all())
    idx = np.where(kept)[0]
    c = np.cumsum(w[idx])
    Z = c[-1]
    xa = np.abs(x[idx])
    beta = 2.0 ** -22 * ((w[idx] * (1 + xa)).sum() + 8 * Z)
    t = clamp_u(u) * Z
    hit = np.where(c > t)[0]
    tok = int(idx[hit[0]]) if hit.size else int(idx[-1])
    decisive = decisive and bool((np.abs(c - t) > beta).all())
    return dict(tok=tok, logprob=logprob_of(l, tok), kept_k=kept_k, kept=kept, decisive=decisive, drew=True)


def sample_rows(logits, u, tau=1.0, K=0, P=1.0, fin=None):
    """The rule on every row of logits [B, S] with uniforms u [B].  -> tok [B], logprob [B], decisive [B], kept_k [B, S]."""
    B = logits.shape[0]
    res = [sample_row(logits[b], u[b], tau, K, P, finished=bool(fin[b]) if fin is not None else False) for b in range(B)]
    return (np.array([r["tok"] for r in res], dtype=np.int64), np.array([r["logprob"] for r in res]),
            np.array([r["decisive"] for r in res], dtype=bool), np.stack([r["kept_k"] for r in res]))


def stop_and_finish(tokens, term, num_token):
    """From decoded tokens [rows, T]: (finish position of every row -- the first position, the start token included, holding a
    token in term = (lo, hi); T when there is none -- and the stop step: steps = s + 1 for the first step s at which no row
    unfinished before it selected a token >= num_token, else T - 1)."""
    tokens = np.asarray(tokens)
    T = tokens.shape[1]
    t = (tokens >= term[0]) & (tokens < term[1])
    fin = np.where(t.any(axis=1), t.argmax(axis=1), T)
    steps = T - 1
    for s in range(T - 1):
        if not ((fin > s) & (tokens[:, s + 1] >= num_token)).any():
            steps = s + 1
            break
    return fin, steps
