"""SurfaceFormer_Parallel: one token sequence per anchor edge, all decoded together (surface of
reference `faceformer/models/model_para.py`; greedy eval path 181-241, pointer head 173-179).

`forward_eval` runs on the native engine (ff_encode + ff_decode, variant FF_PARALLEL).  What the engine
keeps from the reference, quirks included: anchors are arange(F) WITHOUT the special-token offset and
padding anchors start from token num_token-1 (model_para.py:201-205); the decoder is re-run,
unmasked, over the whole prefix each step (222-223); masked logits are finfo.min and ties go to the
lowest index (173-179); the loop stops after the first step whose tokens are all special
(232-233) and the rest is zero padded (236).  What it does differently (results unchanged): memory
and masks are never replicated per sequence (212-214), cross-attention K/V are projected once, the
last layer and the output projection are evaluated for the newest position only.
"""
import numpy as _np
import torch

from .. import faces as _faces
from ..hip import lib as _L
from .common import SurfaceFormerBase


class SurfaceFormer_Parallel(SurfaceFormerBase):

    def __init__(self, num_model=512, num_head=8, num_feedforward=2048, num_encoder_layers=6,
                 num_decoder_layers=6, dropout=0.1, activation="relu", normalize_before=True,
                 num_points_per_line=50, num_lines=64, point_dim=2, max_face_length=10, token=None,
                 teacher_forcing_ratio=0, **kwargs):
        super().__init__()
        self.max_face_length = max_face_length
        self._build(num_model, num_head, num_feedforward, num_encoder_layers, num_decoder_layers,
                    dropout, activation, normalize_before, num_points_per_line, num_lines, point_dim,
                    max_face_length, token, teacher_forcing_ratio)

    def get_embeddings(self, input, label):
        val_embed = self.val_enc(input)
        return val_embed, self.pos_enc(val_embed), self.query_pos_enc(label.transpose(1, 2))

    def forward_eval(self, inputs):
        """inputs: input N x L x P x D, input_mask N x L (True = padding), label N x F' x T (shape
        only), num_input: N edge counts.  Adds predict N x F x T (int64), F = max(num_input).
        beam_width = W >= 1 (default 0: the greedy decode): beam search with W beams per anchor -- also predict_beams
        N x F x W x T (best first; zero after a beam's face-type token and after the stop step) and predict_beam_scores
        N x F x W (summed log-probabilities, -inf for empty beams); predict is beam 0.
        num_samples = R >= 1 (default 0): R independent draws per anchor under sample_temperature / sample_top_k / sample_top_p
         -- also predict_samples and predict_sample_logprob N x F x R x T (zero after a sample's face-type token and
        after the stop step) and predict_sample_scores N x F x R (summed log-probabilities under the model); predict is sample 0.
        The uniforms come from torch.Generator(device).manual_seed(sample_seed), or from inputs["sample_uniforms"]
        [T-1, N*F*R]; either way column (w*F + f)*R + k belongs to wireframe w of the batch AS GIVEN.
        constrain = "no_repeat" / "loops" (default None): the greedy decode over the keys the enclosure filter can accept
         -- predict is the constrained decode (zero after a row's face-type token and after the stop step), also
        predict_logprob N x F x T (under the renormalised distribution) and predict_dead_end N x F.  The follow table is built
        from the end points input[:, :, 0, :2] / input[:, :, -1, :2] with constrain_tol, or taken from inputs["follow_table"]
        (bool N x L x L, or the packed int32 words N x L x ceil(L/32)), for the batch AS GIVEN.
        constrain_beams = W in 1..8 (default 0; only with constrain): the beam search over the constrained keys --
        predict_beams N x F x W x T, predict_beam_scores and predict_beam_dead_end N x F x W in place of predict_logprob; predict
        and predict_dead_end are beam 0's.
        constrain_lookahead = True (default False; only with constrain = "loops", not with constrain_beams): the
        constrained decode also masks every edge from which the loop cannot close within max_face_length; predict_dead_end then
        also means "cannot close in time".  The two distance tables are built on the device from the follow table
        (ops.follow_distance, hmax = max(T - 2, 1)), or taken from inputs["close_dist"] (uint8 N x L x L) and inputs["cycle_len"]
        (uint8 N x L), for the batch AS GIVEN.  The published keys are constrain's.
        constrain_exact = True (default False; only with constrain = "loops", not with constrain_lookahead, which it contains, nor
        with constrain_beams): while a loop is open the constrained decode also masks every edge from which it
        cannot close within max_face_length through edges the row has not used, so a row can only dead-end right after the
        position that opened a loop.  cycle_len is built on the device (ops.follow_distance, hmax = max(T - 2, 1)) or taken from
        inputs["cycle_len"] (uint8 N x L) for the batch AS GIVEN.  The published keys are constrain's.
        constrain_beam_closure = "lookahead" / "exact" (default None; only with constrain = "loops" and constrain_beams = W;
        DESIGN.md 28): the beam search forms every beam's row with the closure look-ahead or the exact one, so that the W beams
        are searched among continuations that can still close within max_face_length.  The tables are built on the device or
        taken from inputs["close_dist"] / inputs["cycle_len"] as for constrain_lookahead / constrain_exact ("exact" needs
        cycle_len only).  The published keys are constrain_beams'.
        constrain_samples = R in 1..64 (default 0; only with constrain, not with constrain_beams): R independent draws
        per anchor from the constrained row -- in the plain form, or with constrain_lookahead / constrain_exact in that form's
        -- under sample_temperature / sample_top_k / sample_top_p, with the uniforms of num_samples (sample_seed, or
        inputs["sample_uniforms"] [T-1, N*F*R]).  Also predict_samples and predict_sample_logprob N x F x R x T,
        predict_sample_scores and predict_sample_dead_end N x F x R; predict, predict_logprob and predict_dead_end are draw 0.
        extract_faces = "parse" / "enclosed" (default False): also inputs["faces"], a dict of device tensors -- len,
        type, closed, loops, score, rep, votes, best, major N x F x G, edges, loop_of N x F x G x T, set_bits N x F x G x
        ceil(L/32), num_faces N -- made by two launches behind the decode from the rows it published (G = the beam width, the
        number of draws, or 1); faces.faces_of_rows turns one wireframe's arrays into the list forms."""
        label = inputs["label"]
        T = self.max_face_length
        mode, value = self._decode_mode(inputs, parallel=True)
        extract = self._extract_faces_value(inputs, parallel=True)
        if not self.engine_supported():      # post-norm / gelu constructor arguments: the sub-module loop (models/common.py)
            inputs = self._forward_eval_modules(inputs, parallel=True)
            if self.retire_finished:         # (that loop decodes every sequence; the result is the same function of its tokens)
                full = inputs["predict"].cpu().numpy()
                inputs["predict"] = torch.as_tensor(_faces.retired_view(full, self.token), device=inputs["predict"].device)
                if "predict_logprob" in inputs:
                    keep = torch.as_tensor(_faces._retired_keep(full, self.token), device=inputs["predict"].device)
                    inputs["predict_logprob"] = inputs["predict_logprob"] * keep
            return inputs
        if label.size(2) < T - 1:
            raise ValueError("label has %d positions but max_face_length-1=%d query positions are "
                             "needed" % (label.size(2), T - 1))
        ni_in = inputs["num_input"]
        # (a device tensor of counts comes over in ONE copy: int() per element is a synchronising copy per wireframe)
        num_input = [int(n) for n in (ni_in.tolist() if torch.is_tensor(ni_in) else ni_in)]
        F = max(num_input)
        N = len(num_input)
        if N != inputs["input"].size(0):
            raise ValueError("num_input has %d entries for a batch of %d" % (N, inputs["input"].size(0)))
        extra = self._extra_mask(inputs)
        want_lp = bool(getattr(self, "return_logprob", False))
        # Ragged batch: decode the wireframes sorted by edge count so that a micro-batch holds wireframes of
        # (nearly) the same width; wireframes are independent, the result rows are put back in batch order.
        order, sub, ni = None, inputs, num_input
        if self.sort_by_edges and extra is None and len(set(num_input)) > 1:
            order = sorted(range(N), key=lambda i: -num_input[i])
            idx = torch.tensor(order, device=inputs["input"].device)
            sub = {"input": inputs["input"].index_select(0, idx), "input_mask": inputs["input_mask"].index_select(0, idx)}
            ni = [num_input[i] for i in order]
        eng = self.engine()
        staged = eng.stage_num_input(ni)       # (before the encoder is enqueued: see stage_num_input)
        eng, memory, mask, kv_len = self._encode(sub, eng)
        prepared = mode.prepare(self, value, inputs, memory.device, T, N, F, num_input, order)
        out = eng.decode(memory, mask, kv_len, _L.FF_PARALLEL, T=T, F=F, num_input=ni, staged_num_input=staged,
                         chunk_wireframes=self.chunk_wireframes, chunk_seqs=self.chunk_seqs,
                         chunk_max_seqs=self.chunk_max_seqs,
                         num_streams=self.num_streams, sync_every=self.sync_every,
                         flags=self.decode_flags, x3_min_rows=self.x3_min_rows, ln_fuse_max_rows=self.ln_fuse_max_rows, extra_mask=extra,
                         retire=self.retire_finished, term_range=(int(self.token.face_type_offset), int(self.token.len)),
                         logprob=want_lp, **prepared)
        # predict and the mode's outputs (predict is beam 0 / sample 0 of every anchor: a fair draw, not a selected one), N x F x ...
        G = value if mode.per_anchor else 1
        views = [("predict", out["predict"].view(N, F, T))]
        views += [("predict_" + key, out[key].view((N, F) + tuple({"G": G, "T": T}[d] for d in dims))) for key, dims, _ in mode.outs]
        if order is not None:
            inv = torch.empty(N, dtype=torch.long, device=memory.device)
            inv[torch.tensor(order, device=memory.device)] = torch.arange(N, device=memory.device)
            views = [(key, t.index_select(0, inv)) for key, t in views]
        inputs.update(views)
        if "predict_beam_dead_end" in inputs:     # (constrain_beams: the constrained decode's key, for beam 0)
            inputs["predict_dead_end"] = inputs["predict_beam_dead_end"][:, :, 0]
        if extract:
            table = prepared.get("follow_table") if extract == "enclosed" else None
            if table is not None and order is not None:      # (made in the decode's wireframe order: back into the batch's)
                table = table.index_select(0, inv)
            inputs["faces"] = self._faces_of_decode(inputs, extract, num_input, memory.device, table)
        self.last_decode_stats = {"decoded_seqs": G * sum(min(F, n + 1) for n in num_input), "rows": N * F,
                                  "slot_rows": out["slot_rows"], "steps": out["steps"]}
        if mode.per_anchor:   # (G sequences per decoded anchor; `rows` stays the reference's N * F)
            self.last_decode_stats[mode.subject if mode.subject in ("constrain_beams", "constrain_samples") else mode.switches[0].attr] = G
        return inputs

    def _faces_of_decode(self, inputs, extract, num_input, device, table):
        """inputs["faces"]: ops.face_rows + ops.face_votes on the rows the decode published, in batch order --
        predict_beams / predict_samples with their scores and dead-end flags when the mode has them, else predict under every
        wireframe's own stop rule (with predict_logprob when there is one).  "enclosed": the enclosure walk on `table` (the
        constrained decode's follow table in batch order) or on the table built from the end points with constrain_tol, and
        only closed faces are counted.  Returns a dict of device tensors N x F x G ..., num_faces N."""
        from ..hip import ops as _ops
        for rows in ("beam", "sample"):
            if "predict_%ss" % rows in inputs:
                tokens = inputs["predict_%ss" % rows]
                kw = dict(scores=inputs["predict_%s_scores" % rows], dead_end=inputs.get("predict_%s_dead_end" % rows))
                break
        else:
            tokens = inputs["predict"]
            kw = dict(logprob=inputs.get("predict_logprob"), own_stop=True)
        if extract == "enclosed" and table is None:
            table = self._follow_table(inputs, device, num_input, None)
        edge_map = inputs.get("edge_map")
        ni = torch.tensor(num_input, dtype=torch.int32).to(device)
        found = _ops.face_rows(tokens, ni, self.token, follows=table, edge_map=None if edge_map is None else edge_map.to(device),
                               num_lines=inputs["input"].size(1), **kw)
        found.update(_ops.face_votes(found, require_closed=extract == "enclosed"))
        return found

    def _follow_distance(self, inputs, device, T, num_input, order, bits):
        """dict(close_dist [N, L, L], cycle_len [N, L]) uint8 of a decode with look-ahead in the DECODE's wireframe order: built on
        the device from `bits` (the follow table, in that order already) with hmax = max(T - 2, 1), the largest budget a step
        compares against; or inputs["close_dist"] / inputs["cycle_len"] for the batch as given, permuted like the wireframes
        when they are decoded sorted by edge count (the edges of a wireframe keep their order: only the leading axis moves)."""
        from ..hip import ops as _ops
        N, L = inputs["input"].size(0), inputs["input"].size(1)
        given = [inputs.get("close_dist"), inputs.get("cycle_len")]
        if given[0] is None and given[1] is None:
            ni = torch.tensor(num_input if order is None else [num_input[i] for i in order], dtype=torch.int32).to(device)
            cd, cl = _ops.follow_distance(bits, ni, min(max(T - 2, 1), 254))
            return {"close_dist": cd, "cycle_len": cl}
        out = {}
        for name, t, shape in (("close_dist", given[0], (N, L, L)), ("cycle_len", given[1], (N, L))):
            if t is None:
                raise ValueError("inputs['close_dist'] and inputs['cycle_len'] are given together")
            t = torch.as_tensor(t)
            if t.dtype != torch.uint8 or tuple(t.shape) != shape:
                raise ValueError("%s must be uint8 [%s]" % (name, ", ".join(str(v) for v in shape)))
            t = t.to(device)
            if order is not None:
                t = t.index_select(0, torch.tensor(order, device=device))
            out[name] = t.contiguous()
        return out

    def _cycle_len(self, inputs, device, T, num_input, order, bits):
        """cycle_len [N, L] uint8 of a decode with the exact look-ahead in the DECODE's wireframe order: built on the device from
        `bits` (the follow table, in that order already) with hmax = max(T - 2, 1), or inputs["cycle_len"] for the batch as
        given (_decode_mode has checked its shape), permuted like the wireframes when they are decoded sorted by edge count."""
        from ..hip import ops as _ops
        given = inputs.get("cycle_len")
        if given is None:
            ni = torch.tensor(num_input if order is None else [num_input[i] for i in order], dtype=torch.int32).to(device)
            return _ops.follow_distance(bits, ni, min(max(T - 2, 1), 254))[1]
        t = torch.as_tensor(given).to(device)
        if order is not None:
            t = t.index_select(0, torch.tensor(order, device=device))
        return t.contiguous()

    def label_paths(self, inputs):
        """score()'s defaults, the data set's own labels: (paths N x F x T = label[:, :max(num_input)], lengths N x F = the
        non-PAD tokens after column 0 by label_mask; unused rows, which hold one token, get 0)."""
        T = self.max_face_length
        ni_in = inputs["num_input"]
        F = max(int(n) for n in (ni_in.tolist() if torch.is_tensor(ni_in) else ni_in))
        label = inputs["label"]
        lmask = inputs["label_mask"] if "label_mask" in inputs else label == self.token.PAD
        return label[:, :F, :T], (~lmask[:, :F, 1:T].to(torch.bool)).sum(dim=-1)

    @torch.no_grad()
    def score(self, inputs, paths=None, lengths=None):
        """Teacher-forced scoring of face loops: how probable is a GIVEN path under the model as it decodes?
        paths N x F x T int64 shaped like predict -- column 0 is the row's own start token (an edge token, not the anchor
        index), F is whatever the caller passes -- and lengths N x F in 0..T-1: positions 1..lengths of a row are scored.
        Defaults: the data set's own labels, paths = label[:, :max(num_input)], lengths = the non-PAD tokens after column 0
        (label_mask; unused rows get 0).  Adds score_logprob / score_greedy / score_rank N x F x T (column j belongs to
        paths[..., j]; zero past the row's length; score_greedy's column 0 repeats the start token) and score_seq_logprob
        N x F.  Not with retire_finished, beam_width, return_logprob, an extra mask or the sub-module loop (ValueError); tokens
        outside [0, S) raise ValueError.  forward / forward_eval are untouched."""
        T = self.max_face_length
        if paths is None:
            paths, default_lengths = self.label_paths(inputs)
            lengths = default_lengths if lengths is None else lengths
        elif lengths is None:
            raise ValueError("score(): paths need lengths")
        paths = torch.as_tensor(paths).to(torch.int64)
        if paths.dim() != 3 or paths.size(0) != inputs["input"].size(0) or paths.size(2) != T:
            raise ValueError("paths must be N x F x %d" % T)
        F = paths.size(1)
        lengths = torch.as_tensor(lengths).reshape(-1)
        return self._score(inputs, _L.FF_PARALLEL, T, F, paths.reshape(-1, T), lengths)
