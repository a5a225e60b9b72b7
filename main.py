#!/usr/bin/env python
"""Thin decode driver with the reference CLI's flags (reference main.py:24-51, test branch only):

    python main.py --config-file configs/ours.yml --test_ckpt last.ckpt [--batch-size N] [KEY VALUE ...]
    python -m torch.distributed.run --nproc-per-node G --master-addr 127.0.0.1 main.py ...   (one rank per GPU)

loads the checkpoint's weights into the MI355X-native model, decodes every sample of `cfg.datasets_test` and
writes one JSON per sample (`edges`, `dominant_directions`, `pred_faces`, `label_faces`; trainer.py:118-136)
under logs/<name>/<version>/json/, printing the running mean decode time and precision / recall.

--batch-size N (extension; the reference's test loader is fixed at 1, trainer.py:51): N samples per `model(batch)`
call, i.e. the micro-batched engine -- 128 wireframes per call run at 0.84 of the f32 matrix peak, one at 0.63
(DESIGN.md 5).  The records do not depend on N: a wireframe's faces are parsed from its OWN anchor rows (not the
batch-wide padding-anchor rows behind them) up to its OWN stop step (faces.apply_own_stop_rule: in a batch the
loop runs on until every wireframe is done), i.e. from exactly the tokens a one-sample decode leaves.  For the
single-sequence model that needs another batch rule than the reference's: its loop stops when the CUMULATIVE number
of EOS tokens equals the batch size (model.py:207-210), which a sample that repeats its EOS reaches before another
sample has produced its own; with N > 1 the decode therefore runs until EVERY wireframe has produced an EOS
(SurfaceFormer.stop_each_eos, ff_decode flag FF_STOP_EACH_EOS).

Under torch.distributed.run every rank decodes a contiguous share of the samples on its own GPU; the JSON
records are all-gathered (faceformer_amd.dist.gather_json_records: RCCL on GPUs, gloo on CPU) and rank 0
writes the files, so a G-rank run leaves exactly the files of a single-process run.
Training / validation / resume (Lightning) are out of scope of this build.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from faceformer_amd import datasets as D  # noqa: E402
from faceformer_amd import faces as FZ  # noqa: E402
from faceformer_amd import models  # noqa: E402
from faceformer_amd.checkpoint import load_lightning_checkpoint  # noqa: E402
from faceformer_amd.config import get_cfg, get_parser  # noqa: E402
from faceformer_amd.dist import gather_json_records, shard_range  # noqa: E402


def decode_batch(model, batch):
    """`model(batch)['predict']` as a numpy array (the one step of run_test that needs the GPU)."""
    with torch.no_grad():
        return model(batch)["predict"].cpu().numpy()


# The decode flags of run_test, in the order their rejections report: (run_test parameter, CLI name, SurfaceFormer_Parallel only,
# the parameters it does not combine with in the order the message lists them, the values it takes (None: any), the text behind
# the name when multi-rank runs do not take it (else None), what a record gains: (record_of parameter, the model's output keys))
CLI_FLAGS = (
    ("constrain", "--constrain", True, ("retire_finished", "scores", "beam", "sample", "score_labels"), ("no_repeat", "loops"), "",
     ("dead_end", ("predict_dead_end",))),
    ("sample", "--sample", True, ("retire_finished", "scores", "beam", "score_labels"), None, " (num_samples)",
     ("samples", ("predict_samples", "predict_sample_scores"))),
    ("score_labels", "--score-labels", False, ("retire_finished", "scores", "beam"), None, " (score)", None),
    ("beam", "--beam", True, ("retire_finished", "scores"), None, " (beam_width)", ("beams", ("predict_beams", "predict_beam_scores"))),
    ("retire_finished", "--retire-finished", True, (), None, None, None),
    ("scores", "--scores", False, (), None, " (return_logprob)", ("logprob", ("predict_logprob",))),
)
NOT_GATHERED = {"score_labels": ": the scores are not gathered across ranks", "scores": ": the log-probabilities are not gathered across ranks"}


def check_cli_flags(given, model_class, world):
    """run_test's rejections, one pass over CLI_FLAGS (`given`: the flags by run_test's parameter names)."""
    cli = {flag: name for flag, name, *_ in CLI_FLAGS}
    for flag, name, parallel_only, excludes, choices, multi, _ in CLI_FLAGS:
        if not given[flag]:
            continue
        others = [cli[f] for f in excludes]
        together = ", ".join(others[:-1]) + " or " + others[-1] if others else ""
        if parallel_only and (model_class != "SurfaceFormer_Parallel" or any(given[f] for f in excludes)):
            raise ValueError("%s applies to SurfaceFormer_Parallel only%s" % (name, ", and not together with " + together if others else ""))
        if any(given[f] for f in excludes):      # (--score-labels, the one flag of both models that excludes others)
            raise ValueError("%s does not combine with %s (a forced decode excludes them)" % (name, together))
        if choices and given[flag] not in choices:
            raise ValueError("%s must be %s" % (name, " or ".join(repr(c) for c in choices)))
        if multi is not None and world > 1:
            raise ValueError("%s%s is not implemented for multi-rank runs%s" % (name, multi, NOT_GATHERED.get(flag, "")))


def decode_batch_with(model, batch, wanted):
    """(`predict`, {record_of parameter: one entry per sample}) of `model(batch)` as numpy arrays; `wanted`: the
    (record_of parameter, output keys) of CLI_FLAGS whose flag is set -- several keys come as one tuple per sample."""
    faces = ("device_faces", ("faces",)) in wanted
    seq_faces = ("sequence_device_faces", ("sequence_faces",)) in wanted
    wanted = [w for w in wanted if w[0] not in ("device_faces", "sequence_device_faces")]
    if not wanted and not faces and not seq_faces:
        return decode_batch(model, batch), {}
    with torch.no_grad():
        out = model(batch)
    extras = {}
    if seq_faces:   # (--sequence-device-faces: the face arrays come over, not the token rows; one wireframe's slice per sample)
        n = out["predict"].size(0)
        for param, _ in wanted:          # (record_of only asks whether they exist)
            extras[param] = [True] * n
        cut = lambda d: [{k: v[i:i + 1] for k, v in d.items()} for i in range(n)]
        to_host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
        extras["sequence_device_faces"] = cut(to_host(out["sequence_faces"]))
        if "predict_samples" in out or "predict_beams" in out:
            # draws / beams: `pred_faces` comes from `predict` alone in the model's form (filtered and mapped for a co-edge
            # config) -- a second, N-row extraction -- and the faces of all draws are the record's unfiltered, unmapped ones:
            # for a co-edge config a third extraction in the "parse" form without the edge map
            with torch.no_grad():
                first = cut(to_host(model._sequence_faces_of_decode(out, model.sequence_faces, out["predict"].device, greedy_only=True)))
                every = None
                if model.sequence_faces == "enclosed":
                    plain = {k: v for k, v in out.items() if k != "edge_map"}
                    every = cut(to_host(model._sequence_faces_of_decode(plain, "parse", out["predict"].device)))
            for i in range(n):
                extras["sequence_device_faces"][i]["first"] = first[i]
                if every is not None:
                    extras["sequence_device_faces"][i]["every"] = every[i]
        return [None] * n, extras
    for param, keys in wanted:
        # (--device-faces: token rows and log-probabilities stay on the device -- record_of only asks whether they exist)
        arrays = [[True] * out[k].size(0) if faces and (k == "predict_logprob" or (i == 0 and len(keys) > 1)) else out[k].cpu().numpy()
                  for i, k in enumerate(keys)]
        extras[param] = arrays[0] if len(arrays) == 1 else list(zip(*arrays))
    if faces:       # (--device-faces: the face arrays come over, not the token rows; one wireframe's slice per sample)
        arrays = {k: v.cpu().numpy() for k, v in out["faces"].items()}
        n = arrays["num_faces"].shape[0]
        extras["device_faces"] = [{k: v[i:i + 1] for k, v in arrays.items()} for i in range(n)]
        if arrays["len"].shape[2] > 1 or "predict_beams" in out:
            # beams / draws: `pred_faces` comes from `predict` under the wireframe's OWN stop rule, as record_of reads it on the
            # host -- a second, small extraction over the N x F rows of predict (the beams and draws are published as decoded)
            sub = {k: out[k] for k in ("predict", "input", "edge_map") if out.get(k) is not None}
            ni = [int(v) for v in (out["num_input"].tolist() if torch.is_tensor(out["num_input"]) else out["num_input"])]
            with torch.no_grad():
                first = {k: v.cpu().numpy() for k, v in model._faces_of_decode(sub, model.extract_faces, ni, out["predict"].device, None).items()}
            for i in range(n):
                extras["device_faces"][i]["first"] = {k: v[i:i + 1] for k, v in first.items()}
        return [None] * n, extras
    return out["predict"].cpu().numpy(), extras


def _edge_bitmap(edges, words):
    """set_bits of the UNMAPPED edge sets of face arrays: edges [..., T] int32 (-1 behind a face) -> [..., words] int32."""
    e = np.asarray(edges)
    bits = np.zeros(e.shape[:-1] + (words,), dtype=np.uint32)
    at = np.nonzero(e >= 0)
    v = e[at]
    np.bitwise_or.at(bits, at[:-1] + (v >> 5,), (np.uint32(1) << (v & 31).astype(np.uint32)))
    return bits.view(np.int32)


def _device_unique(rows, require_closed, unmapped, device_votes):
    """[(majority type, sorted edge set, best score, votes)] in first-seen order of ONE wireframe's face arrays (`rows`: the
    model's inputs["faces"] cut to the sample, 1 x F x G ...).  unmapped: keyed by the edges themselves although the arrays
    were keyed through an edge map.  device_votes: the grouping the device made is the one asked for; otherwise
    faces.face_votes groups the same arrays here."""
    if device_votes:
        return FZ.faces_of_rows(rows, rows, 0)["unique"]
    sub = dict(rows)
    if unmapped:
        sub["set_bits"] = _edge_bitmap(sub["edges"], sub["set_bits"].shape[-1])
    return FZ.faces_of_rows(sub, FZ.face_votes(sub, require_closed=require_closed), 0)["unique"]


def score_batch(model, batch):
    """`model.score(batch)` on the data set's own label rows (--score-labels) as numpy arrays: dict(logprob, greedy, rank, paths
    [N, ..., T], lengths, seq_logprob [N, ...])."""
    out = model.score(dict(batch))
    paths, lengths = model.label_paths(batch)
    lp = out["score_logprob"]
    return {"logprob": lp.cpu().numpy(), "greedy": out["score_greedy"].cpu().numpy(), "rank": out["score_rank"].cpu().numpy(),
            "paths": paths.cpu().numpy(), "lengths": lengths.reshape(lp.shape[:-1]).cpu().numpy(), "seq_logprob": out["score_seq_logprob"].cpu().numpy()}


def record_of(cfg, raw, item, pred, parallel, logprob=None, beams=None, label_scores=None, samples=None, dead_end=None,
              constrained_beams=None, constrained_samples=None, device_faces=None, sequence_samples=None, sequence_beams=None,
              sequence_device_faces=None, sequence_constrained=None, sequence_constrained_samples=None,
              sequence_constrained_beams=None):
    """(JSON text, (precision, recall, type accuracy)) of one decoded sample (reference trainer.py:118-136, 210-300).
    logprob (--scores; laid out like pred): the record also gets `pred_face_scores`, parallel to `pred_faces` -- for every
    de-duplicated face the best sum of log-probabilities among the decoded faces with its edge set (faces.py: *_scored).
    beams (--beam; (tokens [F, W, T], scores [F, W]) of this sample): the record also gets `pred_beam_faces` and
    `pred_beam_face_scores`, the de-duplicated faces over ALL beams of the wireframe's own anchors ranked by their best beam
    score; `pred_faces` stays what beam 0 (pred) gives.
    label_scores (--score-labels; this sample's slice of score_batch): the record also gets `label_logprob` (the summed
    log-probability of every scored label row, in row order), `label_nll` (per token) and `label_tf_accuracy`
    (faces.score_summary; null when the sample has no scored label token).
    samples (--sample; (tokens [F, R, T], scores [F, R]) of this sample): the record also gets `pred_sample_faces`,
    `pred_sample_face_scores` and `pred_sample_face_votes`, the de-duplicated faces over ALL draws of the wireframe's own anchors
    ranked by their best score, with the number of draws that produced each; `pred_faces` stays what sample 0 (pred) gives.
    dead_end (--constrain; the dead-end flags [F] of this sample): the record also gets `pred_dead_ends`, the number of the
    wireframe's own anchor rows the constrained decode ended at a dead end, and `pred_unclosed`, the number of own anchor rows
    whose face does not pass the enclosure walk (dead ends, and loops still open at the last position).
    constrained_beams (--constrain-beams; (tokens [F, W, T], scores [F, W], dead-end flags [F, W]) of this sample): the record
    also gets `pred_beam_faces` and `pred_beam_face_scores` as under --beam, over the beams that did not run into a dead end;
    `pred_faces`, `pred_dead_ends` and `pred_unclosed` stay what beam 0 (pred, dead_end) gives.
    constrained_samples (--constrain-samples; (tokens [F, R, T], scores [F, R], dead-end flags [F, R]) of this sample): the record
    also gets `pred_sample_faces`, `pred_sample_face_scores` and `pred_sample_face_votes` as under --sample, over the draws that
    did not run into a dead end; `pred_faces` stays what draw 0 (pred) gives, and `pred_dead_ends` / `pred_unclosed` are counted
    over ALL draws of the wireframe's own anchors.
    sequence_samples (--sequence-samples, single-sequence model; (tokens [R, T], log-probabilities [R, T]) of this sample): the
    record also gets `pred_sample_faces`, `pred_sample_face_scores` and `pred_sample_face_votes`, the de-duplicated faces over ALL
    draws ranked by their best score, with the number of DRAWS that produced each (a face twice in one draw counts once);
    `pred_faces` stays what draw 0 (pred) gives.
    sequence_beams (--sequence-beams, single-sequence model; (tokens [W, T], scores [W], finished [W]) of this sample): the record
    also gets `pred_beam_faces` and `pred_beam_face_scores`, the de-duplicated faces over ALL non-empty beams ranked by their best
    beam score (faces.parse_faces_beams_scored); `pred_faces` stays what beam 0 (pred) gives.
    device_faces (--device-faces; this sample's slice of the model's inputs["faces"]): the predicted faces of
    every key above come from these arrays (faces.faces_of_rows) instead of from pred, beams and samples, which are then not
    read; label faces, the metrics and the JSON text are made here as before.
    sequence_device_faces (--sequence-device-faces, single-sequence model; this sample's slice of the model's
    inputs["sequence_faces"]): the same for that model -- the predicted faces come from these arrays
    (faces.faces_of_seq_rows) instead of from pred, the draws and the beams, which are then not read.
    sequence_constrained (--sequence-constrain, single-sequence model; the dead-end flags [T] of this sample's row): the record
    also gets `pred_dead_ends`, the number of faces the constrained decode abandoned at a dead end (the sum of the row's flags),
    and `pred_unclosed`, the number of parsed faces that do not pass the enclosure walk.
    sequence_constrained_samples (--sequence-constrain-samples, single-sequence model; (tokens [R, T], log-probabilities [R, T],
    dead-end flags [R, T]) of this sample): the record also gets `pred_sample_faces`, `pred_sample_face_scores` and
    `pred_sample_face_votes` as under --sequence-samples, over the faces that were not abandoned at a dead end
    (faces.parse_faces_constrained_samples_scored); `pred_faces` stays what draw 0 (pred) gives, and `pred_dead_ends` /
    `pred_unclosed` are counted over ALL draws.
    sequence_constrained_beams (--sequence-constrain-beams, single-sequence model; (tokens [W, T], scores [W], finished flags [W],
    dead-end flags [W, T]) of this sample): the record also gets `pred_beam_faces` and `pred_beam_face_scores` as under
    --sequence-beams, over the faces that were not abandoned at a dead end (faces.parse_faces_constrained_beams_scored);
    `pred_faces` stays what beam 0 (pred) gives, and `pred_dead_ends` / `pred_unclosed` are counted over beam 0."""
    if sequence_device_faces is not None:
        return _record_of_sequence_device(cfg, raw, item, sequence_device_faces, logprob is not None, sequence_beams is not None,
                                          sequence_samples is not None)
    if device_faces is not None:
        return _record_of_device(cfg, raw, item, device_faces, logprob is not None, beams is not None or constrained_beams is not None,
                                 samples is not None or constrained_samples is not None, dead_end,
                                 constrained_samples[2] if constrained_samples is not None else None, label_scores)
    scored = logprob is not None
    parse = FZ.parse_parallel_faces if parallel else FZ.parse_faces
    if parallel:
        # the wireframe's OWN anchor sequences: in a batch `predict` is padded to F = max(num_input) rows per wireframe with
        # padding-anchor sequences (reference model_para.py:204-205), which the reference's one-sample test batches never contain
        n = int(item["num_input"])
        pred, logprob = pred[:n], (logprob[:n] if scored else None)
    # ... and their tokens up to the wireframe's OWN stop step (in a batch the loop runs on until every wireframe is done)
    if scored:
        pred, logprob = FZ._apply_own_stop_rule_scored(pred, logprob, cfg.model.token, parallel)
    else:
        pred = FZ.apply_own_stop_rule(pred, cfg.model.token, parallel)
    pf, lf = parse(pred, item["label"], len(raw["edges"]), cfg.model.token)
    sf = None
    if scored:      # the same faces in the same order, with a score each
        sf = (FZ.parse_parallel_faces_scored if parallel else FZ.parse_faces_scored)(pred, logprob, len(raw["edges"]), cfg.model.token)
    if cfg.post_process.is_coedge:
        pairings = raw.get("pairings", {})
        tol = cfg.post_process.enclosedness_tol
        pf = FZ.postprocess_faces(pf, raw["edges"], pairings, tol)
        lf = FZ.postprocess_faces(lf, raw["edges"], pairings, tol)
        if scored:  # the filters work face by face, so a face keeps its score or leaves with it (checked against pf below)
            sf = [(t, idx, s) for ftype, face, s in sf
                  for t, idx in FZ.postprocess_faces([(ftype, face)], raw["edges"], pairings, tol)]
    if scored and [(t, idx) for t, idx, _ in sf] != pf:
        raise RuntimeError("--scores: the scored faces are not the record's faces (a post-processing step is no longer face by face?)")
    m = FZ.face_metrics(pf, lf)
    rec = FZ.faces_record(raw["edges"], raw.get("dominant_directions", []), m["predictions"], m["labels"])
    if scored:      # (unique_faces_with_scores groups like unique_faces_with_majority_type: parallel to m["predictions"])
        rec["pred_face_scores"] = [s for _, _, s, _ in FZ.unique_faces_with_scores(sf)]
    if beams is not None:
        n = int(item["num_input"])
        bf = FZ.parse_parallel_beams_scored(beams[0][:n], beams[1][:n], len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(bf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_beam_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_beam_face_scores"] = [s for _, _, s, _ in ranked]
    if label_scores is not None:
        ls = {k: np.asarray(v)[None] for k, v in label_scores.items()}
        sm = FZ.score_summary(ls["logprob"], ls["greedy"], ls["rank"], ls["paths"], ls["lengths"])
        rec["label_logprob"] = [float(v) for v, n in zip(ls["seq_logprob"].reshape(-1), ls["lengths"].reshape(-1)) if n > 0]
        rec["label_nll"] = float(sm["nll"][0]) if sm["tokens"][0] else None
        rec["label_tf_accuracy"] = float(sm["tf_accuracy"][0]) if sm["tokens"][0] else None
    if dead_end is not None:
        n = int(item["num_input"])
        own = [f for i in range(len(pred)) for f in FZ._parallel_rows(pred[i:i + 1], cfg.model.token, len(raw["edges"]))]
        rec["pred_dead_ends"] = int(np.asarray(dead_end[:n]).astype(bool).sum())
        rec["pred_unclosed"] = sum(1 for _, idx in own
                                   if not FZ.is_face_enclosed(raw["edges"], idx, cfg.post_process.enclosedness_tol))
    if constrained_beams is not None:
        n = int(item["num_input"])
        bf = FZ.parse_parallel_constrained_beams_scored(constrained_beams[0][:n], constrained_beams[1][:n], constrained_beams[2][:n],
                                                        len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(bf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_beam_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_beam_face_scores"] = [s for _, _, s, _ in ranked]
    if constrained_samples is not None:
        n = int(item["num_input"])
        toks, scs, dead = (np.asarray(v[:n]) for v in constrained_samples)
        sf = FZ.parse_parallel_constrained_samples_scored(toks, scs, dead, len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(sf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_sample_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_sample_face_scores"] = [s for _, _, s, _ in ranked]
        rec["pred_sample_face_votes"] = [int(v) for _, _, _, v in ranked]
        draws = FZ.apply_own_stop_rule(toks.reshape(-1, toks.shape[-1]), cfg.model.token, parallel)
        own = [f for i in range(len(draws)) for f in FZ._parallel_rows(draws[i:i + 1], cfg.model.token, len(raw["edges"]))]
        rec["pred_dead_ends"] = int(dead.astype(bool).sum())
        rec["pred_unclosed"] = sum(1 for _, idx in own
                                   if not FZ.is_face_enclosed(raw["edges"], idx, cfg.post_process.enclosedness_tol))
    if samples is not None:
        n = int(item["num_input"])
        sf = FZ.parse_parallel_samples_scored(samples[0][:n], samples[1][:n], len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(sf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_sample_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_sample_face_scores"] = [s for _, _, s, _ in ranked]
        rec["pred_sample_face_votes"] = [int(v) for _, _, _, v in ranked]
    if sequence_samples is not None:
        sf = FZ.parse_faces_samples_scored(sequence_samples[0], sequence_samples[1], len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(sf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_sample_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_sample_face_scores"] = [s for _, _, s, _ in ranked]
        rec["pred_sample_face_votes"] = [int(v) for _, _, _, v in ranked]
    if sequence_constrained is not None:
        own = FZ._seq_faces(pred, cfg.model.token, len(raw["edges"]), True)      # (before any post-processing: what the decode emitted)
        rec["pred_dead_ends"] = int(np.asarray(sequence_constrained).astype(bool).sum())
        rec["pred_unclosed"] = sum(1 for _, idx in own
                                   if not FZ.is_face_enclosed(raw["edges"], idx, cfg.post_process.enclosedness_tol))
    if sequence_constrained_samples is not None:
        toks, lps, dead = (np.asarray(v) for v in sequence_constrained_samples)
        sf = FZ.parse_faces_constrained_samples_scored(toks, lps, dead, len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(sf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_sample_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_sample_face_scores"] = [s for _, _, s, _ in ranked]
        rec["pred_sample_face_votes"] = [int(v) for _, _, _, v in ranked]
        own = [f for row in toks for f in FZ._seq_faces(row, cfg.model.token, len(raw["edges"]), True)]
        rec["pred_dead_ends"] = int(dead.astype(bool).sum())
        rec["pred_unclosed"] = sum(1 for _, idx in own
                                   if not FZ.is_face_enclosed(raw["edges"], idx, cfg.post_process.enclosedness_tol))
    if sequence_constrained_beams is not None:
        toks, bsc, bfin, dead = (np.asarray(v) for v in sequence_constrained_beams)
        bf = FZ.parse_faces_constrained_beams_scored(toks, bsc, bfin, dead, len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(bf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_beam_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_beam_face_scores"] = [s for _, _, s, _ in ranked]
    if sequence_beams is not None:
        bf = FZ.parse_faces_beams_scored(sequence_beams[0], sequence_beams[1], sequence_beams[2], len(raw["edges"]), cfg.model.token)
        ranked = sorted(FZ.unique_faces_with_scores(bf), key=lambda f: -f[2])       # (stable: first seen wins among equal scores)
        rec["pred_beam_faces"] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_beam_face_scores"] = [s for _, _, s, _ in ranked]
    return FZ.dumps_record(rec), (m["precision"], m["recall"], m["type_acc"])


def _record_of_device(cfg, raw, item, rows, scored, beams, samples, dead_end, sample_dead_end, label_scores):
    """record_of for --device-faces: the same record, key for key, from the face arrays `rows` (1 x F x G ...) of this sample.
    beams / samples: the decode published beams / draws; dead_end: --constrain's flags of `predict` (else None);
    sample_dead_end: --constrain-samples' flags of every draw."""
    coedge = bool(cfg.post_process.is_coedge)
    walked = bool((rows["closed"] >= 0).all())           # extract_faces "enclosed": the device counted closed faces only
    n = int(item["num_input"])
    lf = FZ._parallel_rows(item["label"], cfg.model.token, None)
    if coedge:
        lf = FZ.postprocess_faces(lf, raw["edges"], raw.get("pairings", {}), cfg.post_process.enclosedness_tol)
    own = rows.get("first", rows)                        # (beams / draws: the extraction over `predict` alone)
    first = _device_unique(own, coedge, False, walked == coedge)
    m = FZ.face_metrics([(t, key) for t, key, _, _ in first], lf)
    rec = FZ.faces_record(raw["edges"], raw.get("dominant_directions", []), m["predictions"], m["labels"])

    def every_row(kind, votes):      # every beam / draw of the own anchors, unfiltered and keyed by the edges themselves
        ranked = sorted(_device_unique(rows, False, coedge, not walked), key=lambda f: -f[2])
        rec["pred_%s_faces" % kind] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_%s_face_scores" % kind] = [s for _, _, s, _ in ranked]
        if votes:
            rec["pred_sample_face_votes"] = [int(v) for _, _, _, v in ranked]
    if scored:
        rec["pred_face_scores"] = [s for _, _, s, _ in first]
    if beams and dead_end is None:
        every_row("beam", False)
    if label_scores is not None:
        ls = {k: np.asarray(v)[None] for k, v in label_scores.items()}
        sm = FZ.score_summary(ls["logprob"], ls["greedy"], ls["rank"], ls["paths"], ls["lengths"])
        rec["label_logprob"] = [float(v) for v, k in zip(ls["seq_logprob"].reshape(-1), ls["lengths"].reshape(-1)) if k > 0]
        rec["label_nll"] = float(sm["nll"][0]) if sm["tokens"][0] else None
        rec["label_tf_accuracy"] = float(sm["tf_accuracy"][0]) if sm["tokens"][0] else None
    if dead_end is not None:
        # own rows whose face does not pass the walk: `predict`'s, or under --constrain-samples those of every draw -- where a
        # dead-ended draw was left out of the arrays, and its loop is open
        every = sample_dead_end is not None
        dead = np.asarray(sample_dead_end[:n] if every else dead_end[:n]).astype(bool)
        ln, cl = ((rows if every else own)[k][0, :n] for k in ("len", "closed"))
        rec["pred_dead_ends"] = int(dead.sum())
        rec["pred_unclosed"] = int(((ln > 0) & (cl != 1)).sum()) + (int(dead.sum()) if every else 0)
        if beams:
            every_row("beam", False)
        if samples:
            every_row("sample", True)
    elif samples:
        every_row("sample", True)
    return FZ.dumps_record(rec), (m["precision"], m["recall"], m["type_acc"])


def _record_of_sequence_device(cfg, raw, item, rows, scored, beams, samples):
    """record_of for --sequence-device-faces: the same record, key for key, from the face arrays `rows` (1 x G x P ...) of this
    sample.  Under draws / beams, rows["first"] is the extraction over `predict` alone (pred_faces: filtered and mapped for a
    co-edge config) and rows["every"], for a co-edge config, the one over all draws / beams unfiltered and unmapped."""
    lf = FZ._seq_faces(item["label"], cfg.model.token, len(raw["edges"]), False)
    if cfg.post_process.is_coedge:
        lf = FZ.postprocess_faces(lf, raw["edges"], raw.get("pairings", {}), cfg.post_process.enclosedness_tol)
    own = rows.get("first", rows)
    first = FZ.faces_of_seq_rows(own, own, 0)["unique"]
    m = FZ.face_metrics([(t, key) for t, key, _, _ in first], lf)
    rec = FZ.faces_record(raw["edges"], raw.get("dominant_directions", []), m["predictions"], m["labels"])
    if scored:
        rec["pred_face_scores"] = [s for _, _, s, _ in first]
    if samples or beams:
        every = rows.get("every", rows)
        ranked = sorted(FZ.faces_of_seq_rows(every, every, 0)["unique"], key=lambda f: -f[2])     # (stable: first seen wins among equal scores)
        kind = "sample" if samples else "beam"
        rec["pred_%s_faces" % kind] = FZ._plain([(t, idx) for t, idx, _, _ in ranked])
        rec["pred_%s_face_scores" % kind] = [s for _, _, s, _ in ranked]
        if samples:
            rec["pred_sample_face_votes"] = [int(v) for _, _, _, v in ranked]
    return FZ.dumps_record(rec), (m["precision"], m["recall"], m["type_acc"])


def configure_model(model, retire_finished=False, fp16=False, scores=False, beam=0, sample=0, temperature=1.0, top_k=0, top_p=1.0,
                    seed=0, constrain=None, constrain_tol=None, constrain_beams=0, constrain_lookahead=False, constrain_exact=False,
                    constrain_samples=0, constrain_beam_closure=None, sequence_samples=0, sequence_beams=0, sequence_beam_stop="all",
                    sequence_constrain=None, sequence_constrain_samples=0, sequence_constrain_beams=0,
                    sequence_constrain_closure=None, sequence_constrain_beam_closure=None):
    """The CLI's decode options on a built model: retirement of finished face loops, the opt-in one-fp16-product
    projections and cross-attention (split_kind "fp16"), and the log-probabilities of the selections
    (return_logprob), beam search with `beam` beams per anchor (beam_width), `sample` draws per anchor
    under temperature / top_k / top_p from the seeded generator (num_samples), the loop-constrained greedy decode
    (constrain "no_repeat" / "loops" with the end-point tolerance constrain_tol), the beam search over its keys
    with `constrain_beams` beams per anchor, the closure look-ahead of "loops" (constrain_lookahead), its exact form
    (constrain_exact), `constrain_samples` draws per anchor from the constrained keys under temperature / top_k /
    top_p / seed, the closure look-ahead of the constrained beam search (constrain_beam_closure "lookahead" /
    "exact"), `sequence_samples` draws per wireframe of the single-sequence model under temperature / top_k / top_p /
    seed, beam search with `sequence_beams` beams per wireframe of the single-sequence model under the stop rule
    `sequence_beam_stop`, the loop-constrained greedy decode of the single-sequence model (sequence_constrain
    "no_repeat" / "loops" / "coedge_loops" with the end-point tolerance constrain_tol), `sequence_constrain_samples`
    draws per wireframe from the keys that rule allows under temperature / top_k / top_p / seed,
    `sequence_constrain_beams` beams per wireframe over those keys under the stop rule `sequence_beam_stop`, the
    closure look-ahead of that rule and of its sampled form (sequence_constrain_closure "lookahead" / "exact") and of
    its beam search (sequence_constrain_beam_closure).
    Without them the model keeps its defaults."""
    if retire_finished:
        model.retire_finished = True
    if fp16:
        model.split_kind = "fp16"
    if scores:
        model.return_logprob = True
    if beam:
        model.beam_width = int(beam)
    if sample:
        model.num_samples = int(sample)
        model.sample_temperature, model.sample_top_k, model.sample_top_p = float(temperature), int(top_k), float(top_p)
        model.sample_seed = int(seed)
    if constrain:
        model.constrain = str(constrain)
        if constrain_tol is not None:
            model.constrain_tol = float(constrain_tol)
    if constrain_beams:
        model.constrain_beams = int(constrain_beams)
    if constrain_lookahead:
        model.constrain_lookahead = True
    if constrain_exact:
        model.constrain_exact = True
    if constrain_samples:
        model.constrain_samples = int(constrain_samples)
        model.sample_temperature, model.sample_top_k, model.sample_top_p = float(temperature), int(top_k), float(top_p)
        model.sample_seed = int(seed)
    if constrain_beam_closure:
        model.constrain_beam_closure = str(constrain_beam_closure)
    if sequence_samples:
        model.sequence_samples = int(sequence_samples)
        model.sample_temperature, model.sample_top_k, model.sample_top_p = float(temperature), int(top_k), float(top_p)
        model.sample_seed = int(seed)
    if sequence_beams:
        model.sequence_beams = int(sequence_beams)
        model.sequence_beam_stop = str(sequence_beam_stop)
    if sequence_constrain:
        model.sequence_constrain = str(sequence_constrain)
        if constrain_tol is not None:
            model.constrain_tol = float(constrain_tol)
    if sequence_constrain_samples:
        model.sequence_constrain_samples = int(sequence_constrain_samples)
        model.sample_temperature, model.sample_top_k, model.sample_top_p = float(temperature), int(top_k), float(top_p)
        model.sample_seed = int(seed)
    if sequence_constrain_beams:
        model.sequence_constrain_beams = int(sequence_constrain_beams)
        model.sequence_beam_stop = str(sequence_beam_stop)
    if sequence_constrain_closure:
        model.sequence_constrain_closure = str(sequence_constrain_closure)
    if sequence_constrain_beam_closure:
        model.sequence_constrain_beam_closure = str(sequence_constrain_beam_closure)
    return model


def run_test(cfg, ckpt_path, out_dir=None, device="cuda", limit=None, batch_size=1, dist_mod=None, model=None,
             retire_finished=False, fp16=False, scores=False, beam=0, score_labels=False, sample=0, temperature=1.0, top_k=0,
             top_p=1.0, seed=0, constrain=None, constrain_beams=0, constrain_lookahead=False, constrain_exact=False,
             constrain_samples=0, device_faces=False, constrain_beam_closure=None, sequence_samples=0, sequence_beams=0,
             sequence_beam_stop="all", sequence_device_faces=False, sequence_constrain=None, sequence_constrain_samples=0,
             sequence_constrain_beams=0, sequence_constrain_closure=None, sequence_constrain_beam_closure=None):
    """Decode cfg.datasets_test and write the per-sample JSON files; returns the output directory.
    dist_mod: an initialised torch.distributed (or None): the samples are sharded over its ranks, the records gathered,
    rank 0 writes.  model: a ready model object (tests), else built from cfg + checkpoint.
    The decode flags (CLI_FLAGS holds which model, which other flags and whether multi-rank runs take each; build_parser's help
    and configure_model say what each does) -- scores / beam / score_labels / sample / constrain add keys to every record: see
    record_of; sample draws under temperature / top_k / top_p with uniforms from a generator seeded with `seed`; constrain uses
    cfg.post_process.enclosedness_tol as the end-point tolerance; constrain_beams = W (1..8, only with constrain, single-rank
    runs only) decodes W constrained beams per anchor and adds pred_beam_faces / pred_beam_face_scores; constrain_lookahead (only
    with constrain "loops", not with constrain_beams, single-rank runs only) also masks the edges from which a loop cannot close
    in time -- the record keys stay constrain's; constrain_exact (only with constrain "loops", not with constrain_lookahead or
    constrain_beams, single-rank runs only) is the exact form of that look-ahead, with the same record keys; constrain_samples = R
    (1..64, only with constrain, not with constrain_beams, single-rank runs only; with constrain_lookahead or constrain_exact in
    that form) draws R loops per anchor from the constrained keys under temperature / top_k / top_p / seed and adds
    pred_sample_faces / pred_sample_face_scores / pred_sample_face_votes, with pred_dead_ends / pred_unclosed over all draws;
    device_faces (parallel model, single-rank runs only): the predicted faces of every record are extracted on the
    device (model.extract_faces: "enclosed" with the pairings as edge map for co-edge configs and under constrain, "parse"
    otherwise) and the records are made from those arrays -- the same records; constrain_beam_closure ("lookahead" / "exact",
    only with constrain "loops" and constrain_beams, single-rank runs only) runs the constrained beam search
    under the closure look-ahead or its exact form -- the record keys stay constrain_beams'; sequence_samples = R (1..64,
    single-sequence model, single-rank runs only, not with scores, score_labels, sample or device_faces) draws R
    sequences per wireframe under temperature / top_k / top_p / seed and adds pred_sample_faces / pred_sample_face_scores /
    pred_sample_face_votes; pred_faces stays draw 0's; sequence_beams = W (1..8, single-sequence model, single-rank runs only, not
    with scores, score_labels, sample, sequence_samples, beam or device_faces) searches W beams per wireframe under
    sequence_beam_stop ("all" / "best") and adds pred_beam_faces / pred_beam_face_scores; pred_faces stays beam 0's;
    sequence_device_faces (single-sequence model, single-rank runs only, not with device_faces or score_labels; alone or with
    scores, sequence_samples or sequence_beams): the predicted faces of every record are extracted on the device
    (model.sequence_faces: "enclosed" with the pairings as edge map for co-edge configs, "parse" otherwise) and the records are
    made from those arrays -- the same records; sequence_constrain ("no_repeat" / "loops" / "coedge_loops", single-sequence model,
    single-rank runs only, not with scores, score_labels, sample, beam, constrain, sequence_samples, sequence_beams, device_faces
    or sequence_device_faces) decodes under the face-loop rule per face of the row with
    cfg.post_process.enclosedness_tol as the end-point tolerance and adds pred_dead_ends / pred_unclosed;
    sequence_constrain_samples = R (1..64, only with sequence_constrain and refused with whatever it refuses, single-rank runs
    only) draws R rows per wireframe from the keys that rule allows under temperature / top_k / top_p / seed and
    adds pred_sample_faces / pred_sample_face_scores / pred_sample_face_votes, with pred_dead_ends / pred_unclosed over all
    draws; pred_faces stays draw 0's; sequence_constrain_beams = W (1..8, only with sequence_constrain and refused with whatever it
    refuses and with sequence_constrain_samples, single-rank runs only) searches the W best rows per wireframe over
    the keys that rule allows under sequence_beam_stop and adds pred_beam_faces / pred_beam_face_scores, with pred_dead_ends /
    pred_unclosed over beam 0; pred_faces stays beam 0's; sequence_constrain_closure ("lookahead" / "exact", only with
    sequence_constrain "loops" / "coedge_loops", alone or with sequence_constrain_samples, not with sequence_constrain_beams,
    single-rank runs only) also masks the edges from which a loop cannot close inside the row -- the record keys
    stay sequence_constrain's / sequence_constrain_samples'; sequence_constrain_beam_closure ("lookahead" / "exact", only with
    sequence_constrain "loops" / "coedge_loops" and sequence_constrain_beams, single-rank runs only) is that
    look-ahead per beam of the beam search -- the record keys stay sequence_constrain_beams'."""
    if sequence_constrain_beam_closure is not None:
        if sequence_constrain_beam_closure not in ("lookahead", "exact"):
            raise ValueError("--sequence-constrain-beam-closure must be lookahead or exact")
        if sequence_constrain_closure is not None:
            raise ValueError("--sequence-constrain-beam-closure is not implemented with --sequence-constrain-closure: that is the "
                             "greedy and the sampled decode's look-ahead")
        if sequence_constrain_samples:
            raise ValueError("--sequence-constrain-beam-closure is not implemented with --sequence-constrain-samples")
        if not sequence_constrain_beams:
            raise ValueError("--sequence-constrain-beam-closure requires --sequence-constrain-beams W")
        if sequence_constrain is None:
            raise ValueError("--sequence-constrain-beam-closure requires --sequence-constrain {loops,coedge_loops}")
        if sequence_constrain == "no_repeat":
            raise ValueError("--sequence-constrain-beam-closure requires --sequence-constrain loops or coedge_loops: no_repeat tracks "
                             "no loop")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-constrain-beam-closure is not implemented for multi-rank runs")
    if sequence_constrain_closure is not None:
        if sequence_constrain_closure not in ("lookahead", "exact"):
            raise ValueError("--sequence-constrain-closure must be lookahead or exact")
        if sequence_constrain is None:
            raise ValueError("--sequence-constrain-closure requires --sequence-constrain {loops,coedge_loops}")
        if sequence_constrain == "no_repeat":
            raise ValueError("--sequence-constrain-closure requires --sequence-constrain loops or coedge_loops: no_repeat tracks no loop")
        if sequence_constrain_beams:
            raise ValueError("--sequence-constrain-closure is not implemented with --sequence-constrain-beams")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-constrain-closure is not implemented for multi-rank runs")
    if sequence_constrain_beams:
        if isinstance(sequence_constrain_beams, bool) or not isinstance(sequence_constrain_beams, int) \
                or not 1 <= sequence_constrain_beams <= 8:
            raise ValueError("--sequence-constrain-beams must be a width in 1..8")
        if sequence_beam_stop not in ("all", "best"):
            raise ValueError("--sequence-beam-stop must be all or best")
        if cfg.model_class != "SurfaceFormer":
            raise ValueError("--sequence-constrain-beams applies to SurfaceFormer only (SurfaceFormer_Parallel searches under its rule "
                             "with --constrain-beams)")
        if sequence_constrain is None:
            raise ValueError("--sequence-constrain-beams requires --sequence-constrain")
        if sequence_constrain_samples:
            raise ValueError("--sequence-constrain-beams does not combine with --sequence-constrain-samples")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-constrain-beams is not implemented for multi-rank runs")
    if sequence_constrain_samples:
        if isinstance(sequence_constrain_samples, bool) or not isinstance(sequence_constrain_samples, int) \
                or not 1 <= sequence_constrain_samples <= 64:
            raise ValueError("--sequence-constrain-samples must be a count in 1..64")
        if cfg.model_class != "SurfaceFormer":
            raise ValueError("--sequence-constrain-samples applies to SurfaceFormer only (SurfaceFormer_Parallel draws under its rule "
                             "with --constrain-samples)")
        if sequence_constrain is None:
            raise ValueError("--sequence-constrain-samples requires --sequence-constrain")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-constrain-samples is not implemented for multi-rank runs")
    if sequence_constrain is not None:
        if sequence_constrain not in ("no_repeat", "loops", "coedge_loops"):
            raise ValueError("--sequence-constrain must be no_repeat, loops or coedge_loops")
        if cfg.model_class != "SurfaceFormer":
            raise ValueError("--sequence-constrain applies to SurfaceFormer only (SurfaceFormer_Parallel constrains per anchor with --constrain)")
        if scores or score_labels or sample or beam or constrain or sequence_samples or sequence_beams or device_faces or \
                sequence_device_faces:
            raise ValueError("--sequence-constrain does not combine with --scores, --score-labels, --sample, --beam, --constrain, "
                             "--sequence-samples, --sequence-beams, --device-faces or --sequence-device-faces")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-constrain is not implemented for multi-rank runs")
    if sequence_beams:
        if isinstance(sequence_beams, bool) or not isinstance(sequence_beams, int) or not 1 <= sequence_beams <= 8:
            raise ValueError("--sequence-beams must be a width in 1..8")
        if sequence_beam_stop not in ("all", "best"):
            raise ValueError("--sequence-beam-stop must be all or best")
        if cfg.model_class != "SurfaceFormer":
            raise ValueError("--sequence-beams applies to SurfaceFormer only (SurfaceFormer_Parallel searches per anchor with --beam)")
        if scores or score_labels or sample or sequence_samples or beam or device_faces:
            raise ValueError("--sequence-beams does not combine with --scores, --score-labels, --sample, --sequence-samples, --beam or "
                             "--device-faces")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-beams is not implemented for multi-rank runs")
    if sequence_samples:
        if isinstance(sequence_samples, bool) or not isinstance(sequence_samples, int) or not 1 <= sequence_samples <= 64:
            raise ValueError("--sequence-samples must be a count in 1..64")
        if cfg.model_class != "SurfaceFormer":
            raise ValueError("--sequence-samples applies to SurfaceFormer only (SurfaceFormer_Parallel draws per anchor with --sample)")
        if scores or score_labels or sample or device_faces:
            raise ValueError("--sequence-samples does not combine with --scores, --score-labels, --sample or --device-faces")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-samples is not implemented for multi-rank runs")
    if constrain_beam_closure is not None:
        if constrain_beam_closure not in ("lookahead", "exact"):
            raise ValueError("--constrain-beam-closure must be lookahead or exact")
        if constrain != "loops" or not constrain_beams:
            raise ValueError("--constrain-beam-closure requires --constrain loops --constrain-beams W")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--constrain-beam-closure is not implemented for multi-rank runs")
    if device_faces:
        if cfg.model_class != "SurfaceFormer_Parallel":
            raise ValueError("--device-faces applies to SurfaceFormer_Parallel only")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--device-faces is not implemented for multi-rank runs")
    if sequence_device_faces:
        if cfg.model_class != "SurfaceFormer":
            raise ValueError("--sequence-device-faces applies to SurfaceFormer only (SurfaceFormer_Parallel extracts with --device-faces)")
        if device_faces or score_labels:
            raise ValueError("--sequence-device-faces does not combine with --device-faces or --score-labels")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--sequence-device-faces is not implemented for multi-rank runs")
    if constrain_samples:
        if not constrain:
            raise ValueError("--constrain-samples requires --constrain")
        if isinstance(constrain_samples, bool) or not isinstance(constrain_samples, int) or not 1 <= constrain_samples <= 64:
            raise ValueError("--constrain-samples must be a count in 1..64")
        if constrain_beams:
            raise ValueError("--constrain-samples is not implemented with --constrain-beams")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--constrain-samples is not implemented for multi-rank runs")
    if constrain_exact:
        if constrain != "loops":
            raise ValueError("--constrain-exact requires --constrain loops")
        if constrain_lookahead:
            raise ValueError("--constrain-exact is not combined with --constrain-lookahead: it contains it")
        if constrain_beams:
            raise ValueError("--constrain-exact is not implemented with --constrain-beams")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--constrain-exact is not implemented for multi-rank runs")
    if constrain_lookahead:
        if constrain != "loops":
            raise ValueError("--constrain-lookahead requires --constrain loops")
        if constrain_beams:
            raise ValueError("--constrain-lookahead is not implemented with --constrain-beams")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--constrain-lookahead is not implemented for multi-rank runs")
    if constrain_beams:
        if not constrain:
            raise ValueError("--constrain-beams requires --constrain")
        if isinstance(constrain_beams, bool) or not isinstance(constrain_beams, int) or not 1 <= constrain_beams <= 8:
            raise ValueError("--constrain-beams must be a width in 1..8")
        if dist_mod is not None and dist_mod.get_world_size() > 1:
            raise ValueError("--constrain-beams is not implemented for multi-rank runs")
    given = dict(constrain=constrain, sample=sample, score_labels=score_labels, beam=beam, retire_finished=retire_finished, scores=scores)
    check_cli_flags(given, cfg.model_class, dist_mod.get_world_size() if dist_mod is not None else 1)
    model_class = getattr(models, cfg.model_class)
    dataset_class = getattr(D, cfg.dataset_class)
    if model is None:
        model = model_class(**cfg.model)
        sd, _ = load_lightning_checkpoint(ckpt_path)
        model.load_state_dict(sd)
        model = model.eval().to(device)
    configure_model(model, retire_finished, fp16, scores, beam, sample, temperature, top_k, top_p, seed, constrain,
                    cfg.post_process.enclosedness_tol if constrain else None, constrain_beams, constrain_lookahead, constrain_exact,
                    constrain_samples, constrain_beam_closure, sequence_samples, sequence_beams, sequence_beam_stop)
    if sequence_constrain:
        configure_model(model, sequence_constrain=sequence_constrain, constrain_tol=cfg.post_process.enclosedness_tol)
    if sequence_constrain_samples:
        configure_model(model, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                        sequence_constrain_samples=sequence_constrain_samples)
    if sequence_constrain_beams:
        configure_model(model, sequence_beam_stop=sequence_beam_stop, sequence_constrain_beams=sequence_constrain_beams)
    if sequence_constrain_closure:
        configure_model(model, sequence_constrain_closure=sequence_constrain_closure)
    if sequence_constrain_beam_closure:
        configure_model(model, sequence_constrain_beam_closure=sequence_constrain_beam_closure)
    if device_faces:
        model.extract_faces = "enclosed" if cfg.post_process.is_coedge or constrain else "parse"
        model.constrain_tol = float(cfg.post_process.enclosedness_tol)
    if sequence_device_faces:
        model.sequence_faces = "enclosed" if cfg.post_process.is_coedge else "parse"
        model.constrain_tol = float(cfg.post_process.enclosedness_tol)
    ds = dataset_class(cfg.root_dir, cfg.datasets_test, cfg.model)
    out_dir = out_dir or os.path.join("logs", cfg.trainer.name, str(cfg.trainer.version), "json")
    parallel = cfg.model_class == "SurfaceFormer_Parallel"
    batch_size = max(1, int(batch_size))
    if not parallel and batch_size > 1 and hasattr(model, "stop_each_eos") and not sequence_constrain:      # (that decode's rule is per row already)
        model.stop_each_eos = True      # every wireframe decodes up to its own EOS (module docstring)
    rank = dist_mod.get_rank() if dist_mod is not None else 0
    world = dist_mod.get_world_size() if dist_mod is not None else 1
    n_all = len(ds) if limit is None else min(limit, len(ds))
    lo, hi, _ = shard_range(n_all, rank, world)
    batch_size = max(1, int(batch_size))
    total, done, stats, records = 0.0, 0, [], []
    wanted = [gain for flag, *_, gain in CLI_FLAGS if given[flag] and gain]
    if constrain_beams:
        wanted.append(("constrained_beams", ("predict_beams", "predict_beam_scores", "predict_beam_dead_end")))
    if constrain_samples:
        wanted.append(("constrained_samples", ("predict_samples", "predict_sample_scores", "predict_sample_dead_end")))
    if sequence_samples:
        wanted.append(("sequence_samples", ("predict_samples", "predict_sample_logprob")))
    if sequence_beams:
        wanted.append(("sequence_beams", ("predict_beams", "predict_beam_scores", "predict_beam_finished")))
    if sequence_constrain:
        wanted.append(("sequence_constrained", ("predict_dead_end",)))
    if sequence_constrain_samples:
        wanted.append(("sequence_constrained_samples", ("predict_samples", "predict_sample_logprob", "predict_sample_dead_end")))
    if sequence_constrain_beams:
        wanted.append(("sequence_constrained_beams", ("predict_beams", "predict_beam_scores", "predict_beam_finished",
                                                      "predict_beam_dead_end")))
    if device_faces:
        wanted.append(("device_faces", ("faces",)))
    if sequence_device_faces:
        wanted.append(("sequence_device_faces", ("sequence_faces",)))
    for b0 in range(lo, hi, batch_size):
        idx = list(range(b0, min(hi, b0 + batch_size)))
        items = [ds[i] for i in idx]
        batch = D.collate(items)
        if (device_faces or sequence_device_faces) and cfg.post_process.is_coedge:      # map_coedge_into_edges as a table: a co-edge counts as its partner
            emap = torch.arange(batch["input"].size(1), dtype=torch.int32).repeat(len(idx), 1)
            for k, i in enumerate(idx):
                for a, b in ds.raw_datas[i].get("pairings", {}).items():
                    if 0 <= int(a) < emap.size(1):
                        emap[k, int(a)] = int(b)
            batch["edge_map"] = emap
        batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
        if torch.cuda.is_available() and str(device).startswith("cuda"):
            torch.cuda.synchronize()
        t0 = time.time()
        pred, extras = decode_batch_with(model, batch, wanted)
        lsc = score_batch(model, batch) if score_labels else None
        total += time.time() - t0
        done += len(idx)
        for k, i in enumerate(idx):
            text, st = record_of(cfg, ds.raw_datas[i], items[k], pred[k], parallel,
                                 label_scores={n: v[k] for n, v in lsc.items()} if score_labels else None,
                                 **{param: v[k] for param, v in extras.items()})
            stats.append(st)
            records.append((os.path.splitext(os.path.basename(items[k]["name"]))[0], text))
        print("Avg Time", total / done, "seconds.")
    if dist_mod is not None and world > 1:
        # names and records travel the same way (two gathers of length-prefixed utf-8); rank order = sample order
        dev = torch.device(device) if dist_mod.get_backend() == "nccl" else None
        names = gather_json_records([n for n, _ in records], dist_mod, device=dev)
        texts = gather_json_records([t for _, t in records], dist_mod, device=dev)
        flat = [v for s in stats for v in s]
        allstats = [None] * world
        dist_mod.all_gather_object(allstats, flat)
        stats = [tuple(fl[i:i + 3]) for fl in allstats for i in range(0, len(fl), 3)]
        records = list(zip(names, texts))
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        for name, text in records:
            with open(os.path.join(out_dir, name + ".json"), "w") as f:
                f.write(text)
        if stats:
            n = len(stats)
            print("test_precision %.4f test_recall %.4f test_type_acc %.4f over %d samples"
                  % (sum(s[0] for s in stats) / n, sum(s[1] for s in stats) / n, sum(s[2] for s in stats) / n, n))
    if dist_mod is not None and world > 1:
        dist_mod.barrier()
    return out_dir


def build_parser():
    parser = get_parser()
    parser.add_argument("--batch-size", type=int, default=1,
                        help="samples per model(batch) call (the reference's test loader is fixed at 1); the records do not depend on it")
    parser.add_argument("--retire-finished", action="store_true",
                        help="parallel model: stop decoding a face loop once it has produced its face-type token (DESIGN.md 10)")
    parser.add_argument("--fp16", action="store_true",
                        help="decode the decoder's large projections and its cross-attention with ONE fp16 product each, fp32 "
                             "accumulation (split_kind 'fp16', DESIGN.md 11): the arithmetic of the reference's 16-bit GPU decode. "
                             "cfg.trainer.precision is NOT read for this -- honouring it by default would change today's records")
    parser.add_argument("--scores", action="store_true",
                        help="every JSON record gains pred_face_scores, parallel to pred_faces: the summed log-probability of the "
                             "face's greedy selections (DESIGN.md 12); single-process runs only")
    parser.add_argument("--beam", type=int, default=0, metavar="W",
                        help="parallel model: beam search with W (1..8) beams per anchor edge (DESIGN.md 13); pred_faces come from "
                             "the best beam, and every JSON record gains pred_beam_faces / pred_beam_face_scores: the faces of all "
                             "beams, de-duplicated and ranked by score; single-process runs only")
    parser.add_argument("--score-labels", action="store_true",
                        help="every JSON record gains label_logprob (per label row), label_nll (per token) and label_tf_accuracy: "
                             "the model's teacher-forced scores of the sample's own label rows (DESIGN.md 14); single-process runs "
                             "only, not with --retire-finished, --scores or --beam")
    parser.add_argument("--sample", type=int, default=0, metavar="R",
                        help="parallel model: R (1..64) independent draws per anchor edge instead of the argmax (DESIGN.md 15); "
                             "pred_faces come from draw 0, and every JSON record gains pred_sample_faces / pred_sample_face_scores / "
                             "pred_sample_face_votes: the faces of all draws, de-duplicated, ranked by score, with their vote counts; "
                             "single-process runs only, not with --retire-finished, --scores, --beam or --score-labels")
    parser.add_argument("--temperature", type=float, default=1.0, help="--sample: the logits are divided by it (0: the argmax)")
    parser.add_argument("--top-k", type=int, default=0, help="--sample: draw among the K most probable keys (0: all)")
    parser.add_argument("--top-p", type=float, default=1.0, help="--sample: draw among the most probable keys up to this share of the mass")
    parser.add_argument("--seed", type=int, default=0, help="--sample: seed of the generator that makes the uniforms.  The generator is seeded anew for every "
                                                                 "model(batch) call and a draw belongs to the wireframe's place in its batch, so wireframes at the "
                                                                 "same place of different batches (with --batch-size 1: all of them) read the same uniform stream")
    parser.add_argument("--constrain", choices=("no_repeat", "loops"), default=None,
                        help="parallel model: the greedy decode over the keys the enclosure filter can accept (DESIGN.md 16) -- "
                             "no_repeat: never an edge the row holds already; loops: also only an edge that starts where the last "
                             "one ended while a loop is open, and no face-type token before the loop is closed; every JSON record "
                             "gains pred_dead_ends / pred_unclosed; single-process runs only, not with --retire-finished, --scores, "
                             "--beam, --sample or --score-labels")
    parser.add_argument("--constrain-beams", type=int, default=0, metavar="W",
                        help="with --constrain: beam search with W (1..8) beams per anchor edge over the constrained keys "
                             "(DESIGN.md 21); pred_faces, pred_dead_ends and pred_unclosed come from the best beam, and every JSON "
                             "record gains pred_beam_faces / pred_beam_face_scores: the faces of all beams that did not run into a "
                             "dead end, de-duplicated and ranked by score; single-process runs only")
    parser.add_argument("--constrain-lookahead", action="store_true",
                        help="with --constrain loops: also never an edge from which the loop cannot close before the row runs out "
                             "of positions (DESIGN.md 22); pred_dead_ends then also counts rows that could not close in time; "
                             "single-process runs only, not with --constrain-beams")
    parser.add_argument("--constrain-exact", action="store_true",
                        help="with --constrain loops: the exact form of --constrain-lookahead (DESIGN.md 25) -- while a loop is open, "
                             "never an edge from which it cannot close in time through edges the row has not used, so a row can "
                             "only dead-end right after the edge that opened a loop; same record keys; single-process runs only, "
                             "not with --constrain-lookahead or --constrain-beams")
    parser.add_argument("--device-faces", action="store_true",
                        help="parallel model: the predicted faces of every record -- parse, enclosure filter, co-edge mapping, "
                             "de-duplication with type votes, best score and vote count -- are extracted on the device behind the "
                             "decode (DESIGN.md 27) instead of row by row on the host; the records are the same; single-process runs only")
    parser.add_argument("--constrain-samples", type=int, default=0, metavar="R",
                        help="with --constrain: R (1..64) independent draws per anchor edge from the constrained keys under "
                             "--temperature / --top-k / --top-p / --seed (DESIGN.md 26), in the plain form or with "
                             "--constrain-lookahead / --constrain-exact in that form; pred_faces come from draw 0, every JSON record "
                             "gains pred_sample_faces / pred_sample_face_scores / pred_sample_face_votes over the draws that did not "
                             "run into a dead end, and pred_dead_ends / pred_unclosed count all draws; single-process runs only, not "
                             "with --constrain-beams")
    parser.add_argument("--sequence-samples", type=int, default=0, metavar="R",
                        help="single-sequence model: R (1..64) independent draws per wireframe instead of the argmax, decoded "
                             "together off one encoding under --temperature / --top-k / --top-p / --seed (DESIGN.md 29); pred_faces "
                             "come from draw 0, and every JSON record gains pred_sample_faces / pred_sample_face_scores / "
                             "pred_sample_face_votes: the faces of all draws, de-duplicated, ranked by score, with the number of "
                             "draws that produced each; single-process runs only, not with --scores, --score-labels, --sample or "
                             "--device-faces")
    parser.add_argument("--sequence-beams", type=int, default=0, metavar="W",
                        help="single-sequence model: beam search with W (1..8) beams per wireframe instead of the argmax, decoded "
                             "together off one encoding (DESIGN.md 30); pred_faces come from beam 0, and every JSON record gains "
                             "pred_beam_faces / pred_beam_face_scores: the faces of all beams, de-duplicated, ranked by their best "
                             "beam score; single-process runs only, not with --scores, --score-labels, --sample, "
                             "--sequence-samples, --beam or --device-faces")
    parser.add_argument("--sequence-beam-stop", choices=("all", "best"), default="all",
                        help="with --sequence-beams: stop once every non-empty beam is finished (all), or once the best beam of "
                             "every wireframe is finished (best: exact for that beam, the others are written as they stand)")
    parser.add_argument("--sequence-device-faces", action="store_true",
                        help="single-sequence model: the predicted faces of every record -- the split at SEP / EOS, enclosure filter, "
                             "co-edge mapping, de-duplication with best score and vote count -- are extracted on the device behind "
                             "the decode (DESIGN.md 31) instead of row by row on the host; alone or with --scores, "
                             "--sequence-samples or --sequence-beams; the records are the same; single-process runs only, not with "
                             "--device-faces or --score-labels")
    parser.add_argument("--sequence-constrain", choices=("no_repeat", "loops", "coedge_loops"), default=None,
                        help="single-sequence model: the greedy decode under the face-loop rule applied per face of the row "
                             "(DESIGN.md 32) -- no_repeat: never an edge the current face holds already; loops: also only an edge "
                             "that starts where the last one ended while a loop is open, SEP only behind a closed non-empty loop "
                             "(or alone at a dead end, where the face is abandoned) and EOS only with the loop closed; coedge_loops: "
                             "also never a co-edge an earlier face of the row holds; every JSON record gains pred_dead_ends / "
                             "pred_unclosed; single-process runs only, not with --scores, --score-labels, --sample, --beam, "
                             "--constrain, --sequence-samples, --sequence-beams, --device-faces or --sequence-device-faces")
    parser.add_argument("--sequence-constrain-samples", type=int, default=0, metavar="R",
                        help="with --sequence-constrain {no_repeat,loops,coedge_loops}: draw R (1..64) rows per wireframe from the keys "
                             "the face-loop rule allows, under --temperature / --top-k / --top-p with uniforms from --seed "
                             "(DESIGN.md 33); every JSON record gains pred_sample_faces / pred_sample_face_scores / "
                             "pred_sample_face_votes (faces abandoned at a dead end left out), pred_dead_ends / pred_unclosed count "
                             "over all draws, pred_faces stays draw 0's; single-process runs only, refused with whatever "
                             "--sequence-constrain refuses")
    parser.add_argument("--sequence-constrain-closure", choices=["lookahead", "exact"], default=None,
                        help="with --sequence-constrain {loops,coedge_loops}, alone or with --sequence-constrain-samples R: also mask "
                             "every edge from which the current loop cannot close inside the row (DESIGN.md 35) -- lookahead: by the "
                             "follow table's closing distances; exact: by a search over the edges the row has not used; the record "
                             "keys stay --sequence-constrain's; single-process runs only, refused with --sequence-constrain-beams")
    parser.add_argument("--sequence-constrain-beam-closure", choices=["lookahead", "exact"], default=None,
                        help="with --sequence-constrain {loops,coedge_loops} --sequence-constrain-beams W: every beam also masks the "
                             "edges from which its current loop cannot close inside the row (DESIGN.md 36) -- lookahead: by the follow "
                             "table's closing distances; exact: by a search over the edges the beam has not used; the record keys "
                             "stay --sequence-constrain-beams'; single-process runs only, refused with --sequence-constrain-closure "
                             "and --sequence-constrain-samples")
    parser.add_argument("--sequence-constrain-beams", type=int, default=0, metavar="W",
                        help="with --sequence-constrain {no_repeat,loops,coedge_loops}: search the W (1..8) best rows per wireframe "
                             "over the keys the face-loop rule allows, under --sequence-beam-stop (DESIGN.md 34); every JSON record "
                             "gains pred_beam_faces / pred_beam_face_scores (faces abandoned at a dead end left out), pred_dead_ends / "
                             "pred_unclosed count over beam 0, pred_faces stays beam 0's; single-process runs only, refused with "
                             "whatever --sequence-constrain refuses and with --sequence-constrain-samples")
    parser.add_argument("--constrain-beam-closure", choices=("lookahead", "exact"), default=None,
                        help="with --constrain loops --constrain-beams W: the beam search forms every beam's row under the closure "
                             "look-ahead (lookahead) or its exact form (exact), so that the W beams are searched among loops that "
                             "can still close in time (DESIGN.md 28); same record keys as --constrain-beams; single-process runs only")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    cfg = get_cfg(args)
    if args.test_ckpt == "":
        raise SystemExit("only --test_ckpt (greedy decode + JSON dump) is implemented; training, "
                         "validation and resume are out of scope of the MI355X decode build")
    dist_mod, device = None, "cuda"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist_mod
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        device = "cuda:%d" % local_rank
        dist_mod.init_process_group("nccl", device_id=torch.device(device))
    run_test(cfg, args.test_ckpt, device=device, batch_size=args.batch_size, dist_mod=dist_mod,
             retire_finished=args.retire_finished, fp16=args.fp16, scores=args.scores, beam=args.beam,
             score_labels=args.score_labels, sample=args.sample, temperature=args.temperature, top_k=args.top_k,
             top_p=args.top_p, seed=args.seed, constrain=args.constrain, constrain_beams=args.constrain_beams,
             constrain_lookahead=args.constrain_lookahead, constrain_exact=args.constrain_exact,
             constrain_samples=args.constrain_samples, device_faces=args.device_faces,
             constrain_beam_closure=args.constrain_beam_closure, sequence_samples=args.sequence_samples,
             sequence_beams=args.sequence_beams, sequence_beam_stop=args.sequence_beam_stop,
             sequence_device_faces=args.sequence_device_faces, sequence_constrain=args.sequence_constrain,
             sequence_constrain_samples=args.sequence_constrain_samples, sequence_constrain_beams=args.sequence_constrain_beams,
             sequence_constrain_closure=args.sequence_constrain_closure,
             sequence_constrain_beam_closure=args.sequence_constrain_beam_closure)
    if dist_mod is not None:
        dist_mod.destroy_process_group()


if __name__ == "__main__":
    main()
