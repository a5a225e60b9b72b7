"""From decoded token tensors to face loops and the per-wireframe JSON record.

Host-side integer / list logic that follows the decode path in the reference harness:

* `parse_parallel_faces` / `parse_faces`          reference faceformer/trainer.py:181-208 / 153-177
* `unique_faces_with_majority_type`, `face_metrics` reference trainer.py:257-293 (precision / recall /
  type accuracy of de-duplicated faces; majority vote over the types predicted for the same edge set)
* `is_face_enclosed`                               reference dataset/tests/check_faces_enclosed.py:11-46
* `filter_faces_by_encloseness`, `map_coedge_into_edges`, `filter_faces_by_coedge`
                                                   reference faceformer/post_processing.py:8-48
* `faces_record` / `dumps_record`                  the JSON written per sample, trainer.py:118-136
  (`edges`, `dominant_directions`, `pred_faces`, `label_faces`)

Unlike the reference, nothing here mutates its inputs (the reference subtracts the token offset in
place on views of `predict`).  Pinned by goldens captured from the imported reference
(`oracle/make_golden_faces.py` -> `tests/golden/faces_*.json`).
"""
import json
from collections import Counter

import numpy as np

__all__ = ["parse_parallel_faces", "retired_view", "parse_faces", "unique_faces_with_majority_type", "face_metrics",
           "is_face_enclosed", "filter_faces_by_encloseness", "map_coedge_into_edges",
           "filter_faces_by_coedge", "postprocess_faces", "faces_record", "dumps_record",
           "parse_parallel_faces_scored", "parse_faces_scored", "unique_faces_with_scores", "parse_parallel_beams_scored", "score_summary",
           "parse_parallel_samples_scored", "parse_parallel_constrained_samples_scored", "follow_table", "pack_follow_bits", "follow_distance", "closure_distance",
           "face_rows", "face_votes", "faces_of_rows", "parse_faces_samples_scored", "parse_faces_beams_scored",
           "face_seq_rows", "face_seq_votes", "faces_of_seq_rows",
           "sequence_rule_start", "sequence_rule_advance", "sequence_rule_mask", "sequence_rule_step",
           "sequence_rule_sample_step", "parse_faces_constrained_samples_scored"]


def _tok(token, name, default):
    try:
        return int(getattr(token, name))
    except AttributeError:
        try:
            return int(token[name])
        except (KeyError, TypeError):
            return default


def _prefix_through_first(row, hit):
    """row[: first index where hit is True, inclusive]; the whole row if there is no hit."""
    idx = np.flatnonzero(hit)
    return row if idx.size == 0 else row[: idx[0] + 1]


def _edge_indices(tokens, offset, num_edges=None):
    v = np.asarray(tokens, dtype=np.int64) - offset
    v = v[v >= 0]
    if num_edges is not None:
        v = v[v < num_edges]
    return tuple(int(x) for x in v)


def _parallel_rows(rows, token, num_edges):
    off, ntok = _tok(token, "face_type_offset", 1), _tok(token, "len", 4)
    faces = []
    for row in np.asarray(rows):
        row = np.asarray(row, dtype=np.int64)
        seq = _prefix_through_first(row, (row >= off) & (row < ntok))
        if seq.size == 0:
            continue
        face_type = int(seq[-1]) - off
        idx = _edge_indices(seq, ntok, num_edges)
        if idx:
            faces.append((face_type, idx))
    return faces


def retired_view(predict, token, return_steps=False):
    """What the parallel decode with finished-loop retirement (FF_RETIRE_FINISHED) returns, as a function of the reference's
    `predict` of the same batch ([..., T]; every row of the batch, padding anchors included):
      fin[r]  first position j >= 0 of row r holding a face-type token (face_type_offset <= t < len), the start token included;
              T when there is none;
      s       the first position j >= 1 at which no row with fin >= j holds an edge token (>= len): the reference's stop rule
              over the unfinished rows (never later than the reference's own stop); T - 1 when there is none;
      out[r, j] = predict[r, j] for j <= min(fin[r], s), 0 after.
    parse_parallel_faces reads nothing after fin[r], so the faces equal the reference's except where a finished row's later edge
    tokens kept the reference's loop going while an unfinished row had stopped selecting edges.
    Returns a new int64 array of predict's shape (and s with return_steps=True)."""
    p = np.asarray(predict, dtype=np.int64)
    shape = p.shape
    rows = p.reshape(-1, shape[-1])
    T = rows.shape[1]
    off, ntok = _tok(token, "face_type_offset", 1), _tok(token, "len", 4)
    term = (rows >= off) & (rows < ntok)
    fin = np.where(term.any(axis=1), term.argmax(axis=1), T)
    steps = T - 1
    for j in range(1, T):
        if not ((rows[:, j] >= ntok) & (fin >= j)).any():
            steps = j
            break
    keep = np.arange(T)[None, :] <= np.minimum(fin, steps)[:, None]
    out = np.where(keep, rows, 0).reshape(shape)
    return (out, steps) if return_steps else out


def apply_own_stop_rule(predict, token, parallel, eos=None):
    """Tokens of ONE wireframe as a one-sample decode leaves them: zero behind the step at which the reference's loop would
    have stopped had the batch held only this wireframe.  In a batch the loop runs until EVERY wireframe is done (parallel
    model: the first step at which no sequence of the batch selects an edge, model_para.py:232; seq2seq: all EOS emitted,
    model.py:207-210), so a sequence that had not produced its terminator when its own wireframe's rule fired keeps decoding and
    may still produce one -- the one-sample decode (the reference's test loader, trainer.py:51) never sees those tokens.
    predict: [F, T] (parallel: the wireframe's own anchor rows) or [T] (seq2seq).  Returns a copy."""
    p = np.array(predict, dtype=np.int64, copy=True)
    ntok = _tok(token, "len", 4)
    if parallel:
        rows = p.reshape(-1, p.shape[-1])
        for j in range(1, rows.shape[1]):
            if (rows[:, j] < ntok).all():
                rows[:, j + 1:] = 0
                break
        return rows.reshape(p.shape)
    e = _tok(token, "EOS", 3) if eos is None else eos
    hit = np.nonzero(p[1:] == e)[0]
    if hit.size:
        p[hit[0] + 2:] = 0
    return p


def parse_parallel_faces(predicts, labels, num_edges, token):
    """One face per row: tokens up to and including the first face-type token (a special token in
    [face_type_offset, len)); the face type is that token minus the offset; edge indices are the
    tokens minus `len`, negatives dropped, and -- for predictions only -- indices >= num_edges dropped.
    Returns (predict_faces, label_faces) as lists of (type, (edge, ...))."""
    return _parallel_rows(predicts, token, num_edges), _parallel_rows(labels, token, None)


def _seq_faces(seq, token, num_edges, skip_single):
    eos, sep, ntok = _tok(token, "EOS", 3), _tok(token, "SEP", 2), _tok(token, "len", 4)
    seq = np.asarray(seq, dtype=np.int64)
    seq = _prefix_through_first(seq, seq == eos)
    cuts = np.flatnonzero(seq == sep) + 1
    faces = []
    for piece in np.split(seq, cuts):
        if skip_single and piece.size <= 1:
            continue
        idx = _edge_indices(piece[:-1], ntok, num_edges)   # the last token of a piece is its separator
        if idx:
            faces.append((0, idx))
    return faces


def parse_faces(predicts, labels, num_edges, token):
    """Single-sequence variant: cut after the first EOS, split after every SEP, drop the last token of
    every piece, subtract `len`, keep 0 <= index < num_edges.  Faces are typed 0."""
    return _seq_faces(predicts, token, num_edges, True), _seq_faces(labels, token, num_edges, False)


def unique_faces_with_majority_type(faces):
    """Group faces by their SET of edge indices; type = most common predicted type (first seen wins
    ties).  Returns [(type, sorted_unique_edges)] in first-seen order."""
    votes = {}
    for ftype, idx in faces:
        key = tuple(sorted(set(idx)))
        votes.setdefault(key, []).append(ftype)
    return [(Counter(types).most_common(1)[0][0], key) for key, types in votes.items()]


def face_metrics(predict_faces, label_faces):
    """precision, recall, type accuracy over de-duplicated faces (reference trainer.py:257-293).
    Also returns the two de-duplicated lists."""
    label_set = list(set((ftype, tuple(sorted(set(idx)))) for ftype, idx in label_faces))
    pred_set = unique_faces_with_majority_type(predict_faces)
    face_tp = type_tp = 0
    for ptype, pface in pred_set:
        for ltype, lface in label_set:
            if pface == lface:
                face_tp += 1
                type_tp += int(ptype == ltype)
                break
    if not pred_set or not label_set:
        prec = rec = tacc = 0
    else:
        prec, rec = face_tp / len(pred_set), face_tp / len(label_set)
        tacc = type_tp / face_tp if face_tp else 0
    return {"precision": prec, "recall": rec, "type_acc": tacc, "predictions": pred_set, "labels": label_set}


# ---- scored faces: the decode's log-probabilities (models' return_logprob) summed per face -------------------------------------
# New functions beside the unscored ones, which stay as they are: the same rows, filters, grouping and order, plus a score.
# logprobs are laid out like the tokens: entry j is log_softmax(masked logits)[token j], 0 at the start token and in the padding.
def parse_parallel_faces_scored(predicts, logprobs, num_edges, token):
    """parse_parallel_faces' predicted faces with a score each: [(type, (edge, ...), score)], the rows and filters of
    `_parallel_rows`.  score = sum of the row's log-probabilities over positions 1 .. fin, fin the position of the first
    face-type token (the terminator included; the start token at position 0 is given, not selected)."""
    off, ntok = _tok(token, "face_type_offset", 1), _tok(token, "len", 4)
    faces = []
    for row, lp in zip(np.asarray(predicts), np.asarray(logprobs, dtype=np.float64)):
        row = np.asarray(row, dtype=np.int64)
        seq = _prefix_through_first(row, (row >= off) & (row < ntok))
        if seq.size == 0:
            continue
        idx = _edge_indices(seq, ntok, num_edges)
        if idx:
            faces.append((int(seq[-1]) - off, idx, float(lp[1: seq.size].sum())))
    return faces


def parse_faces_scored(predicts, logprobs, num_edges, token):
    """parse_faces' predicted faces with a score each: [(0, (edge, ...), score)], the pieces and filters of `_seq_faces`.
    score = sum of the log-probabilities over the face's piece, its SEP / EOS included (SOS, in the first piece, carries 0)."""
    eos, sep, ntok = _tok(token, "EOS", 3), _tok(token, "SEP", 2), _tok(token, "len", 4)
    seq = np.asarray(predicts, dtype=np.int64)
    seq = _prefix_through_first(seq, seq == eos)
    lp = np.asarray(logprobs, dtype=np.float64)[: seq.size]
    cuts = np.flatnonzero(seq == sep) + 1
    faces = []
    for piece, plp in zip(np.split(seq, cuts), np.split(lp, cuts)):
        if piece.size <= 1:
            continue
        idx = _edge_indices(piece[:-1], ntok, num_edges)
        if idx:
            faces.append((0, idx, float(plp.sum())))
    return faces


def parse_faces_samples_scored(samples, logprobs, num_edges, token):
    """The faces of a sampled single-sequence decode (SurfaceFormer.sequence_samples): samples [R, T] tokens and
    logprobs [R, T] (predict_samples[w] / predict_sample_logprob[w]).  parse_faces_scored per draw; a face (as a SET of edge
    indices) that occurs more than once in ONE draw is kept once, at its first place in the draw, with the best of its scores.
    Returns [(0, (edge, ...), score)] in draw order, the form unique_faces_with_scores takes -- whose vote count is then the
    number of DRAWS that produced the face."""
    rows = np.asarray(samples, dtype=np.int64)
    lps = np.asarray(logprobs, dtype=np.float64)
    if rows.ndim != 2 or lps.shape != rows.shape:
        raise ValueError("samples and logprobs must both be [R, T]")
    faces = []
    for row, lp in zip(rows, lps):
        best = {}      # (insertion-ordered: the first place of every edge set in this draw)
        for ftype, idx, score in parse_faces_scored(row, lp, num_edges, token):
            key = tuple(sorted(set(idx)))
            if key not in best or score > best[key][2]:
                best[key] = (ftype, best[key][1] if key in best else idx, score)
        faces.extend(best.values())
    return faces


def parse_faces_constrained_samples_scored(samples, logprobs, dead_end, num_edges, token):
    """The faces of a constrained sampled single-sequence decode (SurfaceFormer.sequence_constrain_samples): samples,
    logprobs and dead_end [R, T] (predict_samples[w] / predict_sample_logprob[w] / predict_sample_dead_end[w]).
    parse_faces_samples_scored with the faces abandoned at a dead end left out -- a piece whose SEP carries the dead-end flag
    ends in a separator the rule opened for want of an edge: its loop is open.  Returns [(0, (edge, ...), score)] in draw order;
    unique_faces_with_scores then gives every face's best score and the number of DRAWS that produced it."""
    rows = np.asarray(samples, dtype=np.int64)
    lps = np.asarray(logprobs, dtype=np.float64)
    dead = np.asarray(dead_end) != 0
    if rows.ndim != 2 or lps.shape != rows.shape or dead.shape != rows.shape:
        raise ValueError("samples, logprobs and dead_end must all be [R, T]")
    eos, sep, ntok = _tok(token, "EOS", 3), _tok(token, "SEP", 2), _tok(token, "len", 4)
    faces = []
    for row, lp, de in zip(rows, lps, dead):
        seq = _prefix_through_first(row, row == eos)
        cuts = np.flatnonzero(seq == sep) + 1
        best = {}      # (insertion-ordered: the first place of every edge set in this draw)
        for piece, plp, pde in zip(np.split(seq, cuts), np.split(lp[: seq.size], cuts), np.split(de[: seq.size], cuts)):
            if piece.size <= 1 or pde[-1]:
                continue
            idx = _edge_indices(piece[:-1], ntok, num_edges)
            if not idx:
                continue
            key, score = tuple(sorted(set(idx))), float(plp.sum())
            if key not in best or score > best[key][2]:
                best[key] = (0, best[key][1] if key in best else idx, score)
        faces.extend(best.values())
    return faces


def parse_faces_beams_scored(beams, scores, finished, num_edges, token):
    """The faces of a beam decode of the single-sequence model (SurfaceFormer.sequence_beams): beams [W, T] tokens,
    scores [W] the beams' summed log-probabilities (-inf: an empty rank, skipped), finished [W] (predict_beams[w] /
    predict_beam_scores[w] / predict_beam_finished[w]).  Every non-empty beam is read by this model's own parse (`_seq_faces`):
    cut after the first EOS, split after every SEP, the last token of every piece dropped, edge filters applied, a piece of one
    token skipped.  An UNFINISHED beam has no EOS; its zeros behind the stop step are padding, not tokens, and are cut off first,
    so its last, unterminated piece loses its last edge as it does in parse_faces.  Every face carries its BEAM's score; a face
    (as a SET of edge indices) that occurs in several beams, or twice in one, is kept once, at its first place, with the best of
    its scores.  Returns [(0, (edge, ...), score)] in beam order, the form unique_faces_with_scores takes."""
    rows = np.asarray(beams, dtype=np.int64)
    sc = np.asarray(scores, dtype=np.float64).reshape(-1)
    fin = np.asarray(finished).reshape(-1)
    if rows.ndim != 2 or sc.shape != rows.shape[:1] or fin.shape != sc.shape:
        raise ValueError("beams must be [W, T], scores and finished [W]")
    best = {}      # (insertion-ordered: the first place of every edge set)
    for row, score, done in zip(rows, sc, fin):
        if score == -np.inf:
            continue
        if not done:
            used = np.flatnonzero(row)
            row = row[: used[-1] + 1] if used.size else row[:0]
        for ftype, idx in _seq_faces(row, token, num_edges, True):
            key = tuple(sorted(set(idx)))
            if key not in best or score > best[key][2]:
                best[key] = (ftype, best[key][1] if key in best else idx, float(score))
    return list(best.values())


def parse_faces_constrained_beams_scored(beams, scores, finished, dead_end, num_edges, token):
    """The faces of a constrained beam decode of the single-sequence model (SurfaceFormer.sequence_constrain_beams):
    beams and dead_end [W, T], scores and finished [W] (predict_beams[w] / predict_beam_dead_end[w] / predict_beam_scores[w] /
    predict_beam_finished[w]).  parse_faces_beams_scored with the faces abandoned at a dead end left out -- a piece whose SEP
    carries the dead-end flag ends in a separator the rule opened for want of an edge: its loop is open.  The pieces that stay
    are read in place, as one row.  Returns [(0, (edge, ...), score)] in beam order, every face with its BEAM's score."""
    rows = np.asarray(beams, dtype=np.int64)
    dead = np.asarray(dead_end) != 0
    if rows.ndim != 2 or dead.shape != rows.shape:
        raise ValueError("beams and dead_end must both be [W, T]")
    eos, sep = _tok(token, "EOS", 3), _tok(token, "SEP", 2)
    kept = np.zeros_like(rows)
    for i, (row, de) in enumerate(zip(rows, dead)):
        n = _prefix_through_first(row, row == eos).size
        cuts = np.flatnonzero(row[:n] == sep) + 1
        pieces = [p for p, d in zip(np.split(row[:n], cuts), np.split(de[:n], cuts)) if not (p.size and d[-1])]
        flat = np.concatenate(pieces) if pieces else row[:0]
        kept[i, : flat.size] = flat
    return parse_faces_beams_scored(kept, scores, finished, num_edges, token)


def parse_parallel_beams_scored(beams, scores, num_edges, token):
    """The faces of a beam decode (the parallel model's beam_width): beams [..., W, T] tokens, scores [..., W] the
    beams' summed log-probabilities (-inf: an empty beam, skipped).  Every other beam is read as `_parallel_rows` reads a row --
    tokens through the first face-type token, edge filters included -- and carries its beam score: [(type, (edge, ...), score)]
    in row order, the form unique_faces_with_scores takes."""
    off, ntok = _tok(token, "face_type_offset", 1), _tok(token, "len", 4)
    rows = np.asarray(beams, dtype=np.int64)
    rows = rows.reshape(-1, rows.shape[-1])
    faces = []
    for row, score in zip(rows, np.asarray(scores, dtype=np.float64).reshape(-1)):
        if score == -np.inf:
            continue
        seq = _prefix_through_first(row, (row >= off) & (row < ntok))
        if seq.size == 0:
            continue
        idx = _edge_indices(seq, ntok, num_edges)
        if idx:
            faces.append((int(seq[-1]) - off, idx, float(score)))
    return faces


def parse_parallel_constrained_beams_scored(beams, scores, dead_end, num_edges, token):
    """The faces of a constrained beam decode (the parallel model's constrain_beams): parse_parallel_beams_scored
    over the beams that did not run into a dead end -- dead_end [..., W] nonzero: the beam is left out, as an empty one is (a
    dead-ended beam ends in a terminator the rule opened for want of an edge: its loop is open)."""
    sc = np.array(scores, dtype=np.float64, copy=True)
    sc[np.asarray(dead_end).reshape(sc.shape) != 0] = -np.inf
    return parse_parallel_beams_scored(beams, sc, num_edges, token)


def parse_parallel_samples_scored(samples, scores, num_edges, token):
    """The faces of a sampled decode (the parallel model's num_samples): samples [..., R, T] tokens; scores either
    [..., R], the samples' summed log-probabilities (predict_sample_scores), or [..., R, T], their per-position
    log-probabilities (predict_sample_logprob), which are summed here.  Every sample is read as parse_parallel_beams_scored
    reads a beam and carries its score: [(type, (edge, ...), score)] in row order, the form unique_faces_with_scores takes --
    whose vote count is then the number of SAMPLES that drew the face."""
    rows = np.asarray(samples, dtype=np.int64)
    sc = np.asarray(scores, dtype=np.float64)
    if sc.shape == rows.shape:
        sc = sc.sum(axis=-1)
    if sc.shape != rows.shape[:-1]:
        raise ValueError("scores must be shaped like samples, or like samples without the position axis")
    return parse_parallel_beams_scored(rows, sc, num_edges, token)


def parse_parallel_constrained_samples_scored(samples, scores, dead_end, num_edges, token):
    """The faces of a constrained sampled decode (the parallel model's constrain_samples): parse_parallel_samples_scored
    over the draws that did not run into a dead end -- dead_end [..., R] nonzero: the draw is left out (it ends in a terminator
    the rule opened for want of an edge: its loop is open).  scores [..., R] or [..., R, T] as there.  unique_faces_with_scores
    then gives every face's best score and the number of DRAWS that produced it."""
    rows = np.asarray(samples, dtype=np.int64)
    sc = np.array(scores, dtype=np.float64, copy=True)
    if sc.shape == rows.shape:
        sc = sc.sum(axis=-1)
    if sc.shape != rows.shape[:-1]:
        raise ValueError("scores must be shaped like samples, or like samples without the position axis")
    sc[np.asarray(dead_end).reshape(sc.shape) != 0] = -np.inf
    return parse_parallel_beams_scored(rows, sc, num_edges, token)


def score_summary(logprob, greedy, rank, paths, lengths):
    """Likelihood metrics of teacher-forced scores (the models' score()), per wireframe.  logprob / greedy / rank /
    paths [N, ..., T] as score() returns them (parallel: N x F x T, seq2seq: N x T), lengths [N, ...]: positions 1..lengths of a
    row were scored.  Returns dict of length-N arrays: `tokens` (scored positions, int64), `nll` (- sum of their log-probabilities
    / tokens), `tf_accuracy` (share with rank 0: the model's own argmax, given the true prefix, was the path's token) and
    `mean_rank`; NaN where a wireframe has no scored position."""
    lp = np.asarray(logprob, dtype=np.float64)
    rk, gr, pa = np.asarray(rank, dtype=np.int64), np.asarray(greedy, dtype=np.int64), np.asarray(paths, dtype=np.int64)
    ln = np.asarray(lengths, dtype=np.int64)
    if not (lp.shape == rk.shape == gr.shape == pa.shape) or lp.ndim < 2 or ln.shape != lp.shape[:-1]:
        raise ValueError("logprob, greedy, rank and paths must share one [N, ..., T] shape, lengths its leading dimensions")
    N, T = lp.shape[0], lp.shape[-1]
    j = np.arange(T)
    scored = ((j >= 1) & (j <= ln[..., None])).reshape(N, -1)
    lp, rk, hit = lp.reshape(N, -1), rk.reshape(N, -1), (gr == pa).reshape(N, -1)
    if ((rk == 0) != hit)[scored].any():
        raise ValueError("rank and greedy disagree: rank 0 means greedy == paths")
    tokens = scored.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where(tokens > 0, tokens, 1).astype(np.float64)
        none = np.where(tokens > 0, 0.0, np.nan)
        nll = -np.where(scored, lp, 0.0).sum(axis=1) / den + none
        acc = (scored & (rk == 0)).sum(axis=1) / den + none
        mean_rank = np.where(scored, rk, 0).sum(axis=1) / den + none
    return {"tokens": tokens.astype(np.int64), "nll": nll, "tf_accuracy": acc, "mean_rank": mean_rank}


def unique_faces_with_scores(faces):
    """unique_faces_with_majority_type over scored faces [(type, edges, score)]: the same grouping (by the SET of edge indices)
    and first-seen order.  Returns [(majority type, sorted_unique_edges, best score, votes)]: the highest score and the number
    of the faces that share the edge set."""
    groups = {}
    for ftype, idx, score in faces:
        groups.setdefault(tuple(sorted(set(idx))), []).append((ftype, score))
    return [(Counter(t for t, _ in g).most_common(1)[0][0], key, max(s for _, s in g), len(g)) for key, g in groups.items()]


# Two private helpers of the scored paths (the CLI's --scores, the parallel model's return_logprob).  They restate the rules of
# retired_view / apply_own_stop_rule for a second array, because those functions return tokens only and stay as they are here;
# tests/test_logprob.py pins each pair against the other.  Follow-up: derive retired_view / apply_own_stop_rule from these.
def _retired_keep(predict, token):
    """Boolean array of predict's shape: True where retired_view keeps predict's entry, False where it writes its zero padding
    (tokens cannot tell: 0 is a token too).  retired_view(p) == np.where(_retired_keep(p), p, 0)."""
    p = np.asarray(predict, dtype=np.int64)
    rows = p.reshape(-1, p.shape[-1])
    T = rows.shape[1]
    off, ntok = _tok(token, "face_type_offset", 1), _tok(token, "len", 4)
    term = (rows >= off) & (rows < ntok)
    fin = np.where(term.any(axis=1), term.argmax(axis=1), T)
    steps = T - 1
    for j in range(1, T):
        if not ((rows[:, j] >= ntok) & (fin >= j)).any():
            steps = j
            break
    return (np.arange(T)[None, :] <= np.minimum(fin, steps)[:, None]).reshape(p.shape)


def _apply_own_stop_rule_scored(predict, logprob, token, parallel, eos=None):
    """apply_own_stop_rule on the tokens, and the log-probabilities zeroed at the positions it cuts off.  Returns copies
    (tokens, logprobs)."""
    p = np.array(predict, dtype=np.int64, copy=True)
    lp = np.array(logprob, dtype=np.float64, copy=True)
    ntok = _tok(token, "len", 4)
    if parallel:
        rows, lrows = p.reshape(-1, p.shape[-1]), lp.reshape(-1, p.shape[-1])
        for j in range(1, rows.shape[1]):
            if (rows[:, j] < ntok).all():
                rows[:, j + 1:] = 0
                lrows[:, j + 1:] = 0
                break
        return rows.reshape(p.shape), lrows.reshape(p.shape)
    e = _tok(token, "EOS", 3) if eos is None else eos
    hit = np.nonzero(p[1:] == e)[0]
    if hit.size:
        p[hit[0] + 2:] = 0
        lp[hit[0] + 2:] = 0
    return p, lp


# ---- geometric post-processing (co-edge configs) ---------------------------------------------------
def _connects(e1, e2, tol):
    return abs(e1[-1][0] - e2[0][0]) < tol and abs(e1[-1][1] - e2[0][1]) < tol


def follow_table(edges, tol, num_input=None):
    """The co-edge follow table the constrained decode walks, in numpy: table[a, b] is True iff edge b starts
    where edge a ends -- _connects(edges[a], edges[b], tol), evaluated in float32 (one float32 subtraction and one float32
    compare per coordinate, as ff_follow_table does, so the two agree bit for bit).  edges: a list of point lists (a record's
    "edges"), or an array [L, P, D], or the pair (starts, ends) of float32 end points [..., L, 2]; leading batch axes are kept.
    num_input (optional, one count per leading index): rows and columns at and beyond it are False."""
    if isinstance(edges, tuple) and len(edges) == 2:
        starts, ends = (np.asarray(x, dtype=np.float32) for x in edges)
    else:
        pts = [np.asarray(e, dtype=np.float32) for e in edges] if isinstance(edges, list) else np.asarray(edges, dtype=np.float32)
        if isinstance(pts, list):
            starts = np.stack([e[0][:2] for e in pts]) if pts else np.zeros((0, 2), np.float32)
            ends = np.stack([e[-1][:2] for e in pts]) if pts else np.zeros((0, 2), np.float32)
        else:
            starts, ends = pts[..., 0, :2], pts[..., -1, :2]
    t = np.float32(tol)
    d = np.abs(ends[..., :, None, :] - starts[..., None, :, :])          # float32 throughout
    table = (d[..., 0] < t) & (d[..., 1] < t)
    if num_input is not None:
        n = np.asarray(num_input).reshape(table.shape[:-2] + (1,))
        ok = np.arange(table.shape[-1]) < n
        table = table & ok[..., :, None] & ok[..., None, :]
    return table


def pack_follow_bits(table):
    """A boolean follow table [..., L, L] as the words ff_follow_table writes: int32 [..., L, ceil(L/32)], bit b % 32 of word
    b // 32 of row a = table[a, b] (the uint32 words, viewed as int32 for torch)."""
    table = np.asarray(table, dtype=bool)
    L = table.shape[-1]
    fw = (L + 31) // 32
    padded = np.zeros(table.shape[:-1] + (fw * 32,), dtype=np.uint64)
    padded[..., :L] = table
    words = (padded.reshape(table.shape[:-1] + (fw, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return words.astype(np.uint32).view(np.int32)


def follow_distance(table, hmax=254, num_input=None):
    """The closing distances of a follow table, the numpy restatement of ff_follow_distance: the integers are the
    kernel's.  table: bool [..., L, L], table[a, b] = edge b starts where edge a ends.  D(a -> b) is the least h >= 1 for which
    there are a = x_0, ..., x_h = b with table[x_i, x_i+1] for every i; 255 = unreachable or more than hmax hops (1 <= hmax <=
    254).  num_input (optional, one count per leading index): only edges below it take part; rows and columns at or beyond it are
    255.  Returns (close_dist uint8 [..., L, L] with close_dist[f, b] = D(b -> f), cycle_len uint8 [..., L] = D(b -> b))."""
    if isinstance(hmax, bool) or not isinstance(hmax, (int, np.integer)) or not 1 <= hmax <= 254:
        raise ValueError("hmax=%r: must be in 1..254" % (hmax,))
    t = np.asarray(table, dtype=bool)
    L = t.shape[-1]
    if t.ndim < 2 or t.shape[-2] != L:
        raise ValueError("table must be [..., L, L]")
    if num_input is not None:
        ok = np.arange(L) < np.clip(np.asarray(num_input), 0, L).reshape(t.shape[:-2] + (1,))
        t = t & ok[..., :, None] & ok[..., None, :]
    if L == 0:
        return np.zeros(t.shape, dtype=np.uint8), np.zeros(t.shape[:-1], dtype=np.uint8)
    flat = t.reshape((-1, L, L))
    dist = np.full(flat.shape, 255, dtype=np.uint8)       # dist[w, b, x] = D(b -> x): a breadth-first search from every b at once
    nbytes = (L + 7) // 8
    for w in range(flat.shape[0]):
        packed = np.packbits(flat[w], axis=-1, bitorder="little")          # row x: the successors of x, eight to the byte
        reach = np.zeros((L, L), dtype=bool)
        new = flat[w].copy()                                                # level 1: the successors of every source
        for h in range(1, int(hmax) + 1):
            new &= ~reach
            if not new.any():
                break
            dist[w][new] = h
            reach |= new
            rows, cols = np.nonzero(new)                                    # (sorted by source): OR the rows of the new edges
            first = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]])
            front = np.zeros((L, nbytes), dtype=np.uint8)
            front[rows[first]] = np.bitwise_or.reduceat(packed[cols], first, axis=0)
            new = np.unpackbits(front, axis=-1, count=L, bitorder="little").astype(bool)
    dist = dist.reshape(t.shape)
    close = np.ascontiguousarray(np.swapaxes(dist, -1, -2))
    return close, np.ascontiguousarray(np.diagonal(dist, axis1=-2, axis2=-1))


def closure_distance(table, visited, first, hmax=254, num_input=None, pad=None):
    """The closing distances of one sequence with an open loop, the numpy restatement of the search in
    ff_pointer_constrained_exact.  table: bool [L, L], table[a, b] = edge b starts where edge a ends; visited: bool [L] or the
    indices of the edges the row holds; first: the loop's first edge; num_input: only edges below it are available; pad: bool [L],
    edges whose key is padded.  avail(x) = x < num_input, not padded, not visited.  D_V(b -> first) is the least h >= 1 with
    b = x_0, ..., x_h = first, table[x_i, x_i+1] for every i and avail(x_i) for 1 <= i < h (b itself may be any edge; first is the
    target only).  Returns uint8 [L]: D_V(b -> first), 255 for unreachable or more than hmax hops (1 <= hmax <= 254)."""
    if isinstance(hmax, bool) or not isinstance(hmax, (int, np.integer)) or not 1 <= hmax <= 254:
        raise ValueError("hmax=%r: must be in 1..254" % (hmax,))
    t = np.asarray(table, dtype=bool)
    if t.ndim != 2 or t.shape[0] != t.shape[1]:
        raise ValueError("table must be [L, L]")
    L = t.shape[0]
    v = np.asarray(visited)
    if v.dtype != np.bool_:
        idx, v = v.astype(np.int64).reshape(-1), np.zeros(L, dtype=bool)
        v[idx] = True
    if v.shape != (L,):
        raise ValueError("visited must be bool [L] or a list of edges")
    if not 0 <= int(first) < L:
        raise ValueError("first=%r: must be an edge of the table" % (first,))
    avail = ~v
    if num_input is not None:
        avail &= np.arange(L) < int(num_input)
    if pad is not None:
        avail &= ~np.asarray(pad, dtype=bool).reshape(L)
    dist = np.full(L, 255, dtype=np.uint8)
    new = t[:, int(first)].copy()                   # level 1: every edge the first edge follows
    reached = np.zeros(L, dtype=bool)
    for h in range(1, int(hmax) + 1):
        new &= ~reached
        if not new.any():
            break
        dist[new] = h
        reached |= new
        new = t[:, new & avail].any(axis=1)         # the edges with a successor among the available ones of this level
    return dist


# ---- the single-sequence model's loop rule, the numpy restatement of ff_pointer_sequence_constrained -------------------
# include/faceformer_hip.h states the rule on tokens.  State of a row, a function of its prefix: (visited frozenset of edges,
# first, prev); None = none.  One step on a RAW row plus the state update; the integers are the kernel's, the log-probability is fp64.
SEQ_NO_REPEAT, SEQ_CONNECT, SEQ_ONCE = 1, 2, 4
SEQ_FILL = float(np.finfo(np.float32).min)


def sequence_rule_start():
    """The state after column 0 (SOS): nothing visited, the loop closed, the current face without an edge."""
    return (frozenset(), None, None)


def sequence_rule_advance(state, tok, flags, ntok, sep, follows=None):
    """The state after `tok` was appended.  An edge: first = e if first is none, prev = e, the loop closes when
    follows[prev][first] (a one-edge loop closes on itself), visited |= e.  SEP: first = prev = none, visited cleared unless ONCE.
    Any other special token, EOS included: nothing."""
    visited, first, prev = state
    tok = int(tok)
    if tok >= ntok:
        e = tok - ntok
        if first is None:
            first = e
        prev = e
        if follows is not None and follows[prev][first]:
            first = None
        return (visited | {e}, first, prev)
    if tok == sep:
        return (visited if flags & SEQ_ONCE else frozenset(), None, None)
    return state


def sequence_rule_mask(state, flags, S, ntok, sep, eos, follows, pad, closure=None, budget=None, close_dist=None, cycle_len=None):
    """-> (masked [S] bool: the keys the RULE masks, padding not included; dead_end).  pad [S] bool: the keys masked by padding /
    kv_len, which the dead-end vote has to see.

    closure (None: the rule above, unchanged): under CONNECT one more edge mask in front of the dead-end vote, against
    budget = min(T - 1 - position, 254) in 0..254.  "lookahead": with the loop open edge b is masked when close_dist[first][b] >
    budget, with it closed when cycle_len[b] > budget (one wireframe's follow_distance tables, [L, L] and [L] uint8).  "exact"
    (NO_REPEAT as well): with the loop open when D_V(b -> first) > budget -- closure_distance over the edges that are neither
    padded nor visited (under ONCE: the edges of every face so far) -- with it closed the cycle_len rule; close_dist is not read.
    The two fix-ups of the closed state are unchanged, so a closed row whose edges are all masked keeps SEP or EOS live and is
    no dead end."""
    if closure is not None:
        if closure not in ("lookahead", "exact"):
            raise ValueError("closure=%r: must be None, 'lookahead' or 'exact'" % (closure,))
        if not flags & SEQ_CONNECT or (closure == "exact" and not flags & SEQ_NO_REPEAT):
            raise ValueError("closure=%r needs SEQ_CONNECT%s" % (closure, " | SEQ_NO_REPEAT" if closure == "exact" else ""))
        if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)) or not 0 <= budget <= 254:
            raise ValueError("budget=%r: must be in 0..254" % (budget,))
    visited, first, prev = state
    masked = np.zeros(S, dtype=bool)
    connect = bool(flags & SEQ_CONNECT)
    is_open = connect and first is not None and prev is not None
    if connect:
        masked[:ntok] = True
        if not is_open:
            masked[eos] = False
            masked[sep] = prev is None           # no empty face, no SEP SEP ... loop
    if flags & SEQ_NO_REPEAT:
        for e in visited:
            masked[ntok + e] = True
    if closure is not None:
        L = S - ntok
        if is_open and closure == "exact":
            vis = np.zeros(L, dtype=bool)
            vis[sorted(visited)] = True
            dist = closure_distance(np.asarray(follows, dtype=bool)[:L, :L], vis, first, hmax=min(max(int(budget), 1), 254),
                                    pad=np.asarray(pad, dtype=bool)[ntok:])
        else:
            dist = np.asarray(close_dist[first] if is_open else cycle_len)[:L]
        masked[ntok:] |= dist.astype(np.int64) > int(budget)
    dead = False
    if is_open:
        masked[ntok:] |= ~np.asarray(follows[prev][: S - ntok], dtype=bool)
        if not (~masked[ntok:] & ~pad[ntok:]).any():
            dead = True
            masked[sep] = False                  # SEP alone: the face is abandoned, the row goes on
    return masked, dead


def sequence_rule_step(raw, pad, state, flags, ntok, sep, eos, follows=None, finished=False, **closure):
    """One row of one step on RAW logits; **closure: sequence_rule_mask's closure, budget, close_dist and cycle_len.  -> dict(tok, logprob, row (the constrained masked row, fp64), masked (the rule's own
    byte row), dead, fin (finished after the step), state (after the step)).  A finished row appends token 0 with log-probability
    0 and keeps its state; a row with no live key gives token 0 and -log S."""
    raw = np.asarray(raw, dtype=np.float64)
    S = len(raw)
    if finished:
        return dict(tok=0, logprob=0.0, row=raw, masked=np.zeros(S, bool), dead=False, fin=True, state=state)
    pad = np.asarray(pad, dtype=bool)
    masked, dead = sequence_rule_mask(state, flags, S, ntok, sep, eos, follows, pad, **closure)
    row = np.where(masked | pad, SEQ_FILL, raw)
    tok = int(np.argmax(row))                    # (lowest index on ties)
    lp = -float(np.log(np.exp(row - row[tok]).sum()))
    return dict(tok=tok, logprob=lp, row=row, masked=masked, dead=dead, fin=tok == eos,
                state=sequence_rule_advance(state, tok, flags, ntok, sep, follows))


def sequence_rule_sample_step(raw, pad, state, flags, ntok, sep, eos, u, temperature=1.0, top_k=0, top_p=1.0, follows=None,
                              finished=False, **closure):
    """One row of one step of the sampled form (ff_pointer_sequence_constrained_sample) on RAW logits:
    sequence_rule_mask's row, then the sampling rule of DESIGN.md 15 on it with the uniform u -- top-k and top-p act on the
    constrained row, and at a dead end SEP, the only live key, is drawn whatever u is.  -> sequence_rule_step's dict.  logprob:
    (l[tok] - max) - log sum exp(l - max) over the constrained row, fp64."""
    raw = np.asarray(raw, dtype=np.float64)
    S = len(raw)
    if finished:
        return dict(tok=0, logprob=0.0, row=raw, masked=np.zeros(S, bool), dead=False, fin=True, state=state)
    pad = np.asarray(pad, dtype=bool)
    masked, dead = sequence_rule_mask(state, flags, S, ntok, sep, eos, follows, pad, **closure)      # (DESIGN.md 35's closure keywords)
    row = np.where(masked | pad, SEQ_FILL, raw)
    live = row > SEQ_FILL
    m = row.max()
    if not live.any():
        tok, lp = 0, -float(np.log(S))
    else:
        if temperature == 0:
            tok = int(np.argmax(row))                # (lowest index on ties)
        else:
            w = np.where(live, np.exp(np.where(live, (row - m) / temperature, 0.0)), 0.0)
            kept = live.copy()
            if 0 < top_k < int(live.sum()):
                kept &= row >= np.sort(row[live])[::-1][top_k - 1]
            if top_p < 1:
                vals = np.unique(row[kept])[::-1]
                cum = np.array([w[kept & (row >= v)].sum() for v in vals])
                hit = cum >= top_p * w[kept].sum()
                kept &= row >= vals[int(np.argmax(hit)) if hit.any() else len(vals) - 1]
            idx = np.flatnonzero(kept)
            c = np.cumsum(w[idx])
            uu = min(max(float(u) if u == u else 0.0, 0.0), 1.0 - 2.0 ** -24)
            over = np.flatnonzero(c > uu * c[-1])
            tok = int(idx[over[0]]) if over.size else int(idx[-1])
        lp = max(float((row[tok] - m) - np.log(np.exp(row - m).sum())), SEQ_FILL)
    return dict(tok=tok, logprob=lp, row=row, masked=masked, dead=dead, fin=tok == eos,
                state=sequence_rule_advance(state, tok, flags, ntok, sep, follows))


def sequence_rule_beam_step(raw, pad, scores, fin, states, flags, ntok, sep, eos, follows=None, closure=None, budget=None,
                            close_dist=None, cycle_len=None):
    """One step of ONE group (the W beams of one wireframe) of the beam form (ff_beam_sequence_constrained_select)
    on RAW logits [W, S]: scores [W] (-inf: an empty beam, no candidates), fin [W], states [W] (sequence_rule_start's form), pad
    [S] the wireframe's padding / kv_len keys.  An unfinished beam's row is sequence_rule_mask's; its candidates are the LIVE
    keys only, each at score + (l[s] - max) - log sum exp(l - max) over the constrained row, saturated at SEQ_FILL (a row with no
    live key: token 0 at score - log S); a finished beam is its own single candidate, token 0, score unchanged.  Order: higher
    score first, then the lower flat index k * S + s.  -> dict(parent, tok, scores, fin, dead (this step's flag), open [W each],
    states [W], rows [W, S] (the constrained masked rows, fp64; raw for empty / finished beams), masked [W, S] (the rule's own
    byte rows), cand: the first W + 1 candidates (score, flat index) in order).  A rank past the number of candidates is empty:
    parent = the rank, token 0, score -inf, flags clear, the state of the own index.

    closure, budget, close_dist, cycle_len (closure None: the rule above, unchanged): sequence_rule_mask's closure
    keywords, handed to every unfinished non-empty beam's own mask -- the wireframe's tables ([L, L] and [L] uint8) are shared by
    its beams, the budget is the step's, and each beam is looked ahead from its OWN (first, prev) and visited set."""
    ahead = {} if closure is None else dict(closure=closure, budget=budget, close_dist=close_dist, cycle_len=cycle_len)
    raw = np.asarray(raw, dtype=np.float64)
    W, S = raw.shape
    pad = np.asarray(pad, dtype=bool)
    rows, masks, dead_of = raw.copy(), np.zeros((W, S), dtype=bool), [False] * W
    cand = []
    for k in range(W):
        if scores[k] == -np.inf:
            continue
        if fin[k]:
            cand.append((float(scores[k]), k * S))
            continue
        masks[k], dead_of[k] = sequence_rule_mask(states[k], flags, S, ntok, sep, eos, follows, pad, **ahead)
        row = rows[k] = np.where(masks[k] | pad, SEQ_FILL, raw[k])
        m = row.max()
        logz = np.log(np.exp(row - m).sum())
        live = np.flatnonzero(row > SEQ_FILL)
        if not live.size:
            cand.append((max(float(scores[k] - logz), SEQ_FILL), k * S))
            continue
        sc = np.maximum(scores[k] + ((row - m) - logz), SEQ_FILL)
        cand.extend((float(sc[s]), k * S + int(s)) for s in live)
    cand.sort(key=lambda c: (-c[0], c[1]))
    out = dict(parent=np.arange(W), tok=np.zeros(W, dtype=np.int64), scores=np.full(W, -np.inf), fin=np.zeros(W, dtype=bool),
               dead=np.zeros(W, dtype=bool), open=np.zeros(W, dtype=bool), states=list(states), rows=rows, masked=masks,
               cand=cand[: W + 1])
    for r, (sc, ix) in enumerate(cand[:W]):
        k, s = divmod(ix, S)
        out["parent"][r], out["scores"][r] = k, sc
        if fin[k]:
            out["fin"][r], out["states"][r] = True, states[k]
        else:
            out["tok"][r], out["fin"][r], out["dead"][r] = s, s == eos, dead_of[k]
            out["states"][r] = sequence_rule_advance(states[k], s, flags, ntok, sep, follows)
        out["open"][r] = out["states"][r][1] is not None
    return out


def sequence_rule_beam_decode(step_logits, pad, W, T, flags, ntok, sos, sep, eos, follows=None, stop="all", closure=None,
                              close_dist=None, cycle_len=None):
    """The whole rule of the beam form as a loop over G = len(pad) wireframes.  step_logits(prefixes [G * W, j + 1], j) -> RAW
    logits [G * W, S] of step j (rows of empty and finished beams are not read); pad [G, S]; follows: one table per wireframe
    (or None).  Start: every beam at sos, beam 0 with score 0, the others empty, the rule's state empty and closed.  Stop: after
    the first step that leaves `stop`'s counter at 0 ("all": the non-empty beams unfinished after the step; "best": the groups
    whose rank 0 is), else after T - 1 steps.  -> dict(beams, dead_end [G * W, T] (walked back along the parents, zero past each
    beam's EOS and past steps), scores, fin, open [G * W], steps, counts, all_counts, best_counts, parents, toks, deads, cands
    (per step, per group), states).

    closure (None: the rule above, unchanged) with close_dist [G, L, L] / cycle_len [G, L] (one pair of
    follow_distance tables per wireframe; "exact" reads cycle_len only): sequence_rule_beam_step's look-ahead, the step that
    selects position p under budget = min(T - 1 - p, 254)."""
    if stop not in ("all", "best"):
        raise ValueError("stop=%r: must be 'all' or 'best'" % (stop,))
    pad = np.asarray(pad, dtype=bool)
    G, B = len(pad), len(pad) * W
    scores = np.where(np.arange(B) % W == 0, 0.0, -np.inf)
    fin, opn = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    states = [sequence_rule_start()] * B
    toks, parents, deads, cands, alls, bests = [], [], [], [], [], []

    def walk(cols):      # [B, len(cols[0..]) + 1]: column j of every beam through its parents; column 0 is given
        res = np.zeros((B, len(toks) + 1), dtype=np.int64)
        for b in range(B):
            g, cur = b // W, b % W
            for s in range(len(toks), 0, -1):
                res[b, s] = cols[s - 1][g * W + cur]
                cur = int(parents[s - 1][g * W + cur])
        return res

    steps = T - 1
    for j in range(T - 1):
        prefixes = walk(toks)
        prefixes[:, 0] = sos
        raw = np.asarray(step_logits(prefixes, j), dtype=np.float64)
        ahead = lambda g: {} if closure is None else dict(      # (step j selects position j + 1)
            closure=closure, budget=min(T - 2 - j, 254), close_dist=None if close_dist is None else close_dist[g],
            cycle_len=None if cycle_len is None else cycle_len[g])
        res = [sequence_rule_beam_step(raw[g * W:(g + 1) * W], pad[g], scores[g * W:(g + 1) * W], fin[g * W:(g + 1) * W],
                                       states[g * W:(g + 1) * W], flags, ntok, sep, eos, None if follows is None else follows[g],
                                       **ahead(g))
               for g in range(G)]
        scores, fin, opn = (np.concatenate([r[k] for r in res]) for k in ("scores", "fin", "open"))
        states = [s for r in res for s in r["states"]]
        toks.append(np.concatenate([r["tok"] for r in res]))
        parents.append(np.concatenate([r["parent"] for r in res]))
        deads.append(np.concatenate([r["dead"] for r in res]).astype(np.int64))
        cands.append([r["cand"] for r in res])
        live = np.isfinite(scores) & ~fin
        alls.append(int(live.sum()))
        bests.append(int(live.reshape(G, W)[:, 0].sum()))
        if (alls if stop == "all" else bests)[-1] == 0:
            steps = j + 1
            break
    beams, dead_end = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    beams[:, : steps + 1] = walk(toks)
    beams[:, 0] = sos
    dead_end[:, : steps + 1] = walk(deads)
    return dict(beams=beams, dead_end=dead_end, scores=scores, fin=fin, open=opn, steps=steps,
                counts=alls if stop == "all" else bests, all_counts=alls, best_counts=bests, parents=parents, toks=toks, deads=deads,
                cands=cands, states=states)


def is_face_enclosed(edges, face_indices, tol):
    """Walk the face's edges in order; every edge must start where the previous one ended, and a loop
    closes when an edge ends at the loop's first start point.  Items may be `(index, reversed)` pairs.
    Returns the list of loops (lists of the original items) or False."""
    loops, current = [], []
    first = prev = None
    for item in face_indices:
        if isinstance(item, tuple):
            i, rev = item
            edge = edges[i][::-1] if rev else edges[i]
        elif item < len(edges):
            edge = edges[item]
        else:
            continue
        if first is None:
            first = edge
        elif not _connects(prev, edge, tol):
            return False
        prev = edge
        current.append(item)
        if _connects(edge, first, tol):
            loops.append(current)
            current, first = [], None
    return loops if first is None else False


def filter_faces_by_encloseness(edges, faces, tol):
    """Keep faces whose edges chain into closed loops; each loop is rotated so its smallest index comes
    first, loops are ordered by that index.  [(type, (edges...))] -> [(type, ((loop...), ...))]."""
    kept = []
    for ftype, face in faces:
        loops = is_face_enclosed(edges, face, tol)
        if not loops:
            continue
        rolled = []
        for loop in loops:
            arr = np.asarray(loop)
            rolled.append(tuple(np.roll(arr, -int(np.argmin(arr)), axis=0).astype(int).tolist()))
        kept.append((ftype, tuple(sorted(rolled, key=lambda lp: lp[0]))))
    return kept


def map_coedge_into_edges(pairings, indices):
    """Replace every co-edge index by its partner edge (pairings keys are strings in the JSON)."""
    return [pairings[str(i)] if str(i) in pairings else i for i in indices]


def filter_faces_by_coedge(pairings, faces):
    """Drop a face that reuses an edge already claimed through its co-edge partner (the reference
    defines it, post_processing.py:23-39, but never calls it)."""
    kept, used = [], set()
    for face in faces:
        drop = False
        for index in (i for loop in face[1] for i in loop):
            if index in pairings:
                index = pairings[index]
                if index in used:
                    drop = True
                    break
            used.add(index)
        if not drop:
            kept.append(face)
    return kept


def postprocess_faces(faces, edges, pairings, tol):
    """The is_coedge branch of the harness (trainer.py:226-255): enclosure filter, then flatten the
    loops and map co-edges onto edges."""
    closed = filter_faces_by_encloseness(edges, faces, tol)
    return [(ftype, map_coedge_into_edges(pairings, [i for loop in loops for i in loop]))
            for ftype, loops in closed]


# ---- face extraction as arrays: the numpy restatements of ff_face_rows / ff_face_votes ----------------------------
# The same arguments, keys, dtypes and bits as ops.face_rows / ops.face_votes; faces_of_rows turns the arrays of one wireframe
# back into the list forms above, which makes the whole contract testable on the CPU.
FACE_MAX_T = 256
FACE_MAX_ROWS = 65536


def _face_tokens4(tokens):
    t = np.asarray(tokens, dtype=np.int64)
    if t.ndim == 3:
        t = t[:, :, None, :]
    if t.ndim != 4:
        raise ValueError("tokens must be [N, F, T] or [N, F, G, T]")
    if not 1 <= t.shape[3] <= FACE_MAX_T:
        raise ValueError("tokens hold T=%d positions: 1..%d are taken" % (t.shape[3], FACE_MAX_T))
    return t


def face_rows(tokens, num_input, token, num_edges=None, scores=None, logprob=None, dead_end=None, own_stop=False, follows=None,
              edge_map=None, num_lines=None):
    """ff_face_rows in numpy (include/faceformer_hip.h states the rule): every row of tokens [N, F, G, T] (or [N, F, T]: G = 1)
    parsed as `_parallel_rows` parses it, walked as is_face_enclosed walks it on the packed follow table `follows`
    [N, L, ceil(L/32)] int32, ordered as filter_faces_by_encloseness orders it, and keyed by the bitmap of its (mapped) edge set.
    num_input [N]; num_edges [N] or None (= num_input), clamped into [0, L]; scores [N, F, G] or logprob [N, F, G, T] (not both);
    dead_end [N, F, G]; own_stop: apply_own_stop_rule over every wireframe's own rows; edge_map [N, L] int32 or None.
    L = the table's / the map's, else num_lines, else F.  Returns dict of arrays: len, type, closed, loops [N, F, G] int32; edges,
    loop_of [N, F, G, T] int32 (-1 behind len); set_bits [N, F, G, ceil(L/32)] int32 (the uint32 words); score [N, F, G] float64."""
    t = _face_tokens4(tokens)
    N, F, G, T = t.shape
    off, ntok = _tok(token, "face_type_offset", 1), _tok(token, "len", 4)
    if not 0 <= off < ntok:
        raise ValueError("face_type_offset=%d must be in [0, len=%d)" % (off, ntok))
    if scores is not None and logprob is not None:
        raise ValueError("scores and logprob may not both be given")
    ni = np.asarray(num_input, dtype=np.int64).reshape(N)
    fol = None if follows is None else np.asarray(follows).view(np.uint32) if np.asarray(follows).dtype == np.int32 else np.asarray(follows, dtype=np.uint32)
    emap = None if edge_map is None else np.asarray(edge_map, dtype=np.int64)
    L = fol.shape[1] if fol is not None else emap.shape[1] if emap is not None else F if num_lines is None else int(num_lines)
    fw = (L + 31) // 32
    if fol is not None and fol.shape != (N, L, fw):
        raise ValueError("follows must be [N, L, ceil(L/32)]")
    if emap is not None and emap.shape != (N, L):
        raise ValueError("edge_map must be [N, L]")
    ne = np.clip(ni if num_edges is None else np.asarray(num_edges, dtype=np.int64).reshape(N), 0, L)
    sc = None if scores is None else np.asarray(scores, dtype=np.float32).reshape(N, F, G)
    lp = None if logprob is None else np.asarray(logprob, dtype=np.float32).reshape(N, F, G, T)
    de = None if dead_end is None else np.asarray(dead_end).reshape(N, F, G)
    out = {"len": np.zeros((N, F, G), np.int32), "type": np.zeros((N, F, G), np.int32),
           "closed": np.full((N, F, G), 0 if fol is not None else -1, np.int32), "loops": np.zeros((N, F, G), np.int32),
           "edges": np.full((N, F, G, T), -1, np.int32), "loop_of": np.full((N, F, G, T), -1, np.int32),
           "set_bits": np.zeros((N, F, G, fw), np.uint32), "score": np.zeros((N, F, G), np.float64)}

    def bit(w, a, b):
        return bool((int(fol[w, a, b >> 5]) >> (b & 31)) & 1)

    for w in range(N):
        stop = T - 1
        if own_stop:
            own = t[w, :max(0, min(int(ni[w]), F))].reshape(-1, T)
            for j in range(1, T):
                if (own[:, j] < ntok).all():
                    stop = j
                    break
        for f in range(min(F, max(int(ni[w]), 0))):
            for g in range(G):
                if sc is not None and sc[w, f, g] == -np.inf:
                    continue
                if de is not None and de[w, f, g] != 0:
                    continue
                row = t[w, f, g].copy()
                row[stop + 1:] = 0
                hit = np.flatnonzero((row >= off) & (row < ntok))
                fin = int(hit[0]) if hit.size else T - 1
                v = row[: fin + 1] - ntok
                e = [int(x) for x in v[(v >= 0) & (v < ne[w])]]
                if not e:
                    continue
                n = len(e)
                out["len"][w, f, g] = n
                out["type"][w, f, g] = np.int64(row[fin] - off).astype(np.int32)
                if sc is not None:
                    out["score"][w, f, g] = np.float64(sc[w, f, g])
                elif lp is not None:
                    terms = lp[w, f, g].astype(np.float64)
                    terms[stop + 1:] = 0.0
                    out["score"][w, f, g] = np.cumsum(np.concatenate(([0.0], terms[1: fin + 1])))[-1]     # (0 + x1 + x2 + ..., one by one)
                order, loop_of = e, [-1] * n
                if fol is not None:
                    loops, start, ok = [], None, True
                    for i, x in enumerate(e):
                        if start is None:
                            start = i
                        elif not bit(w, e[i - 1], x):
                            ok = False
                            break
                        if bit(w, x, e[start]):
                            loops.append(e[start: i + 1])
                            start = None
                    ok = ok and start is None
                    out["closed"][w, f, g] = int(ok)
                    if ok:
                        out["loops"][w, f, g] = len(loops)
                        rolled = []
                        for lo in loops:
                            m = lo.index(min(lo))
                            rolled.append(lo[m:] + lo[:m])
                        rolled.sort(key=lambda lo: lo[0])                     # (stable)
                        order = [x for lo in rolled for x in lo]
                        loop_of = [k for k, lo in enumerate(rolled) for _ in lo]
                out["edges"][w, f, g, :n] = order
                out["loop_of"][w, f, g, :n] = loop_of
                for x in e:
                    m = int(emap[w, x]) if emap is not None else x
                    if not 0 <= m < L:
                        m = x
                    out["set_bits"][w, f, g, m >> 5] |= np.uint32(1 << (m & 31))
    out["set_bits"] = out["set_bits"].view(np.int32)
    return out


def _score_order(v):
    """float64 -> uint64 keys of ff_face_votes' total order (-0 below +0)."""
    b = np.asarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def face_votes(rows, require_closed=False):
    """ff_face_votes in numpy: the rows of every wireframe grouped by their set_bits row.  rows: face_rows' dict.  A row takes part
    iff len > 0 and, with require_closed, closed == 1.  Returns dict: rep [N, F, G] int32 (the least row f*G + g of the wireframe
    with the same bitmap; -1: takes no part); for rep == own row: votes (group size), best (float64 highest score), major (most
    frequent type, on a tie the one whose first row is the lowest: Counter.most_common), 0 elsewhere; num_faces [N] int32."""
    ln = np.asarray(rows["len"])
    N, F, G = ln.shape
    R = F * G
    if R > FACE_MAX_ROWS:
        raise ValueError("face_votes takes at most %d rows per wireframe (got %d)" % (FACE_MAX_ROWS, R))
    bits = np.asarray(rows["set_bits"]).reshape(N, R, -1)
    ty, cl = np.asarray(rows["type"]).reshape(N, R), np.asarray(rows["closed"]).reshape(N, R)
    sc = np.asarray(rows["score"], dtype=np.float64).reshape(N, R)
    ln = ln.reshape(N, R)
    rep = np.full((N, R), -1, np.int32)
    votes, major = np.zeros((N, R), np.int32), np.zeros((N, R), np.int32)
    best = np.zeros((N, R), np.float64)
    num = np.zeros(N, np.int32)
    for w in range(N):
        groups = {}
        for r in range(R):
            if ln[w, r] > 0 and (not require_closed or cl[w, r] == 1):
                groups.setdefault(bits[w, r].tobytes(), []).append(r)
        num[w] = len(groups)
        for members in groups.values():
            p = members[0]
            rep[w, members] = p
            votes[w, p] = len(members)
            s = sc[w, members]
            best[w, p] = s[int(np.argmax(_score_order(s)))]
            major[w, p] = Counter(int(ty[w, r]) for r in members).most_common(1)[0][0]
    shape = (N, F, G)
    return {"rep": rep.reshape(shape), "votes": votes.reshape(shape), "best": best.reshape(shape), "major": major.reshape(shape),
            "num_faces": num}


def faces_of_rows(rows, votes, w):
    """The arrays of wireframe w (face_rows' and face_votes' dicts, numpy or anything np.asarray takes) as the list forms:
    `parsed` [(type, (edge, ...))] in row order, the edges in decode order for an open or unwalked face and in canonical order
    for a closed one; `scored` [(type, edges, score)] beside it; `enclosed` [(type, ((edge, ...), ...))], the closed faces as
    filter_faces_by_encloseness returns them; `unique` [(major, sorted edge set, best, votes)] in first-seen order -- the edge
    set is read back from the bitmap, so with an edge_map it holds the mapped edges.  votes may be None (no `unique`)."""
    ln = np.asarray(rows["len"])[w].reshape(-1)
    R = ln.size
    ty = np.asarray(rows["type"])[w].reshape(-1)
    cl = np.asarray(rows["closed"])[w].reshape(-1)
    sc = np.asarray(rows["score"])[w].reshape(-1)
    ed = np.asarray(rows["edges"])[w].reshape(R, -1)
    lo = np.asarray(rows["loop_of"])[w].reshape(R, -1)
    parsed, scored, enclosed = [], [], []
    for r in range(R):
        n = int(ln[r])
        if n == 0:
            continue
        e = tuple(int(x) for x in ed[r, :n])
        parsed.append((int(ty[r]), e))
        scored.append((int(ty[r]), e, float(sc[r])))
        if cl[r] == 1:
            k = lo[r, :n]
            enclosed.append((int(ty[r]), tuple(tuple(int(x) for x in ed[r, :n][k == i]) for i in range(int(k.max()) + 1))))
    out = {"parsed": parsed, "scored": scored, "enclosed": enclosed}
    if votes is not None:
        bits = np.asarray(rows["set_bits"])[w].reshape(R, -1).view(np.uint32)
        rep = np.asarray(votes["rep"])[w].reshape(-1)
        vt, bs, mj = (np.asarray(votes[k])[w].reshape(-1) for k in ("votes", "best", "major"))
        unique = []
        for r in np.flatnonzero(rep == np.arange(R)):
            word = bits[r]
            key = tuple(int(32 * x + b) for x in range(word.size) for b in range(32) if (int(word[x]) >> b) & 1)
            unique.append((int(mj[r]), key, float(bs[r]), int(vt[r])))
        out["unique"] = unique
    return out


# ---- the single-sequence model's rows as arrays: the numpy restatements of ff_face_seq_rows and its grouping ------
# A row holds ALL faces of a wireframe (or of one draw / beam of it), split at SEP: every row gets P face slots.
FACE_SEQ_MAX_T = 2048
FACE_SEQ_ROW_KEYS = ("count", "len", "start", "type", "closed", "loops", "edges", "loop_of", "set_bits", "score", "dup_of", "take",
                     "row_best")


def face_seq_rows(tokens, num_edges, token, slots=None, scores=None, logprob=None, finished=None, follows=None, edge_map=None,
                  closed_only=False, num_lines=None):
    """ff_face_seq_rows in numpy (include/faceformer_hip.h states the rule): every row of tokens [N, G, T] (or [N, T]: G = 1) split
    into faces as `_seq_faces` splits it (cut after the first EOS, split after every SEP, the last token of a piece dropped; an
    unfinished row -- finished [N, G] zero -- cut behind its last nonzero token first, as parse_faces_beams_scored does), every
    face walked, ordered and keyed as face_rows does a row, duplicates inside a row folded.  num_edges [N], clamped into [0, L];
    token: the config's (len, SEP, EOS); slots = P face slots per row (None: max(T // 2, 1)); scores [N, G] or logprob [N, G, T]
    (not both); follows [N, L, ceil(L/32)] int32 or None; edge_map [N, L] int32 or None; closed_only: only closed faces take
    part in the fold.  L = the table's / the map's, else num_lines.  Returns dict of arrays: count [N, G] int32; len, start, type,
    closed, loops, dup_of, take [N, G, P] int32; edges, loop_of [N, G, T] int32; set_bits [N, G, P, ceil(L/32)] int32 (the uint32
    words); score, row_best [N, G, P] float64."""
    t = np.asarray(tokens, dtype=np.int64)
    if t.ndim == 2:
        t = t[:, None, :]
    if t.ndim != 3:
        raise ValueError("tokens must be [N, T] or [N, G, T]")
    N, G, T = t.shape
    if not 1 <= T <= FACE_SEQ_MAX_T:
        raise ValueError("tokens hold T=%d positions: 1..%d are taken" % (T, FACE_SEQ_MAX_T))
    P = max(T // 2, 1) if slots is None else int(slots)
    if not 1 <= P <= max(T // 2, 1):
        raise ValueError("slots=%d: must be in 1..max(T // 2, 1) = %d" % (P, max(T // 2, 1)))
    ntok, sep, eos = _tok(token, "len", 4), _tok(token, "SEP", 2), _tok(token, "EOS", 3)
    if not (0 <= sep < ntok and 0 <= eos < ntok and sep != eos):
        raise ValueError("SEP=%d and EOS=%d must be two tokens of [0, len=%d)" % (sep, eos, ntok))
    if scores is not None and logprob is not None:
        raise ValueError("scores and logprob may not both be given")
    fol = None if follows is None else np.asarray(follows).view(np.uint32) if np.asarray(follows).dtype == np.int32 else np.asarray(follows, dtype=np.uint32)
    emap = None if edge_map is None else np.asarray(edge_map, dtype=np.int64)
    if fol is None and emap is None and num_lines is None:
        raise ValueError("num_lines is needed without a follow table and an edge map")
    L = fol.shape[1] if fol is not None else emap.shape[1] if emap is not None else int(num_lines)
    fw = (L + 31) // 32
    if fol is not None and fol.shape != (N, L, fw):
        raise ValueError("follows must be [N, L, ceil(L/32)]")
    if emap is not None and emap.shape != (N, L):
        raise ValueError("edge_map must be [N, L]")
    ne = np.clip(np.asarray(num_edges, dtype=np.int64).reshape(N), 0, L)
    sc = None if scores is None else np.asarray(scores, dtype=np.float32).reshape(N, G)
    lp = None if logprob is None else np.asarray(logprob, dtype=np.float32).reshape(N, G, T)
    fin = None if finished is None else np.asarray(finished).reshape(N, G)
    i32 = lambda fill: np.full((N, G, P), fill, np.int32)
    out = {"count": np.zeros((N, G), np.int32), "len": i32(0), "start": i32(0), "type": i32(0),
           "closed": i32(0 if fol is not None else -1), "loops": i32(0), "edges": np.full((N, G, T), -1, np.int32),
           "loop_of": np.full((N, G, T), -1, np.int32), "set_bits": np.zeros((N, G, P, fw), np.uint32),
           "score": np.zeros((N, G, P), np.float64), "dup_of": i32(-1), "take": i32(0), "row_best": np.zeros((N, G, P), np.float64)}

    def bit(w, a, b):
        return bool((int(fol[w, a, b >> 5]) >> (b & 31)) & 1)

    for w in range(N):
        for g in range(G):
            if sc is not None and sc[w, g] == -np.inf:
                continue
            row = t[w, g]
            end = T - 1
            if fin is not None and fin[w, g] == 0:
                used = np.flatnonzero(row)
                if used.size == 0:
                    continue
                end = int(used[-1])
            hit = np.flatnonzero(row[: end + 1] == eos)
            if hit.size:
                end = int(hit[0])
            s, at, first = 0, 0, 0                     # the next slot, its start, the first position of the running piece
            for p in range(end + 1):
                if row[p] != sep and p != end:
                    continue
                v = row[first: p] - ntok                # (the boundary token is dropped)
                e = [int(x) for x in v[(v >= 0) & (v < ne[w])]]
                a, first = first, p + 1
                if not e:
                    continue
                if s >= P:
                    s += 1
                    continue
                n = len(e)
                out["len"][w, g, s], out["start"][w, g, s] = n, at
                if sc is not None:
                    out["score"][w, g, s] = np.float64(sc[w, g])
                elif lp is not None:
                    out["score"][w, g, s] = np.cumsum(np.concatenate(([0.0], lp[w, g, a: p + 1].astype(np.float64))))[-1]
                order, loop_of = e, [-1] * n
                if fol is not None:
                    loops, start, ok = [], None, True
                    for i, x in enumerate(e):
                        if start is None:
                            start = i
                        elif not bit(w, e[i - 1], x):
                            ok = False
                            break
                        if bit(w, x, e[start]):
                            loops.append(e[start: i + 1])
                            start = None
                    ok = ok and start is None
                    out["closed"][w, g, s] = int(ok)
                    if ok:
                        out["loops"][w, g, s] = len(loops)
                        rolled = []
                        for lo in loops:
                            m = lo.index(min(lo))
                            rolled.append(lo[m:] + lo[:m])
                        rolled.sort(key=lambda lo: lo[0])                     # (stable)
                        order = [x for lo in rolled for x in lo]
                        loop_of = [k for k, lo in enumerate(rolled) for _ in lo]
                out["edges"][w, g, at: at + n] = order
                out["loop_of"][w, g, at: at + n] = loop_of
                for x in e:
                    m = int(emap[w, x]) if emap is not None else x
                    if not 0 <= m < L:
                        m = x
                    out["set_bits"][w, g, s, m >> 5] |= np.uint32(1 << (m & 31))
                s, at = s + 1, at + n
            out["count"][w, g] = s
            # the fold: a draw counts once for a face
            seen = {}
            for k in range(min(s, P)):
                out["row_best"][w, g, k] = out["score"][w, g, k]
                if closed_only and out["closed"][w, g, k] != 1:
                    continue
                key = out["set_bits"][w, g, k].tobytes()
                if key in seen:
                    out["dup_of"][w, g, k] = seen[key][0]
                    seen[key].append(k)
                else:
                    seen[key] = [k]
                    out["take"][w, g, k] = 1
            for members in seen.values():
                v = out["score"][w, g, members]
                out["row_best"][w, g, members[0]] = v[int(np.argmax(_score_order(v)))]
    out["set_bits"] = out["set_bits"].view(np.int32)
    return out


def face_seq_votes(rows, require_closed=False):
    """The grouping behind face_seq_rows: face_votes, unchanged, over the G * P slots of every wireframe with len := take and
    score := row_best -- `votes` is then the number of draws (beams) that hold the face, `rep` the first draw's first slot that
    holds it (slot index g * P + s), `best` the best score.  Returns face_votes' dict shaped [N, G, P] (num_faces [N])."""
    take = np.asarray(rows["take"])
    N, G, P = take.shape
    flat = lambda k: np.asarray(rows[k]).reshape(N, G * P, 1)
    votes = face_votes({"len": flat("take"), "type": flat("type"), "closed": flat("closed"), "score": flat("row_best"),
                        "set_bits": np.asarray(rows["set_bits"]).reshape(N, G * P, 1, -1)}, require_closed=require_closed)
    return {k: (v if k == "num_faces" else v.reshape(N, G, P)) for k, v in votes.items()}


def faces_of_seq_rows(rows, votes, w):
    """The arrays of wireframe w (face_seq_rows' and face_seq_votes' dicts) as the list forms: `parsed` and `scored`, one list per
    row g of [(0, (edge, ...))] / [(0, edges, score)] in slot order (decode order for an open or unwalked face, canonical order
    for a closed one); `enclosed`, one list per row of the closed faces [(0, ((edge, ...), ...))] as filter_faces_by_encloseness
    returns them; `unique` [(0, sorted edge set, best, votes)] over all rows in first-seen order -- the edge set is read back from
    the bitmap, so with an edge_map it holds the mapped edges.  votes may be None (no `unique`)."""
    ln, st, cl = (np.asarray(rows[k])[w] for k in ("len", "start", "closed"))
    sc, ed, lo = (np.asarray(rows[k])[w] for k in ("score", "edges", "loop_of"))
    G, P = ln.shape
    parsed, scored, enclosed = [], [], []
    for g in range(G):
        parsed.append([])
        scored.append([])
        enclosed.append([])
        for s in range(P):
            n, a = int(ln[g, s]), int(st[g, s])
            if n == 0:
                continue
            e = tuple(int(x) for x in ed[g, a: a + n])
            parsed[g].append((0, e))
            scored[g].append((0, e, float(sc[g, s])))
            if cl[g, s] == 1:
                k = lo[g, a: a + n]
                enclosed[g].append((0, tuple(tuple(int(x) for x in ed[g, a: a + n][k == i]) for i in range(int(k.max()) + 1))))
    out = {"parsed": parsed, "scored": scored, "enclosed": enclosed}
    if votes is not None:
        bits = np.asarray(rows["set_bits"])[w].reshape(G * P, -1).view(np.uint32)
        rep = np.asarray(votes["rep"])[w].reshape(-1)
        vt, bs = (np.asarray(votes[k])[w].reshape(-1) for k in ("votes", "best"))
        unique = []
        for r in np.flatnonzero(rep == np.arange(G * P)):
            word = bits[r]
            key = tuple(int(32 * x + b) for x in range(word.size) for b in range(32) if (int(word[x]) >> b) & 1)
            unique.append((0, key, float(bs[r]), int(vt[r])))
        out["unique"] = unique
    return out


# ---- JSON record -------------------------------------------------------------------------------------
def _plain(obj):
    if isinstance(obj, (np.integer,)):
        return int(obj)
    if isinstance(obj, (np.floating,)):
        return float(obj)
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    if isinstance(obj, (list, tuple)):
        return [_plain(x) for x in obj]
    if isinstance(obj, dict):
        return {str(k): _plain(v) for k, v in obj.items()}
    return obj


def faces_record(edges, dominant_directions, pred_faces, label_faces):
    """The per-sample dict the reference dumps for `reconstruction/` (trainer.py:126-133)."""
    return {"edges": _plain(edges), "dominant_directions": _plain(dominant_directions),
            "pred_faces": _plain(pred_faces), "label_faces": _plain(label_faces)}


def dumps_record(record):
    return json.dumps(_plain(record))
