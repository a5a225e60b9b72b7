"""SurfaceFormer: all faces of a wireframe as ONE token sequence (surface of reference
`faceformer/models/model.py`; greedy eval path 169-219, pointer head 161-167).

Constructor arguments, `state_dict` layout and the `forward(inputs: dict) -> dict` contract match the
reference; `forward_eval` runs on the native engine (ff_encode + ff_decode, variant FF_SEQ2SEQ):
start token SOS, at most label_seq_length-1 steps, stop when the cumulative EOS count equals the
batch size (reference model.py:191,207-210), zero padding afterwards.
"""
import torch

from ..hip import lib as _L
from ..hip import modes as _modes
from .common import SurfaceFormerBase


class SurfaceFormer(SurfaceFormerBase):

    def __init__(self, num_model=512, num_head=8, num_feedforward=2048, num_encoder_layers=6,
                 num_decoder_layers=6, dropout=0.1, activation="relu", normalize_before=True,
                 num_points_per_line=50, num_lines=1000, point_dim=2, label_seq_length=2000,
                 token=None, teacher_forcing_ratio=0, **kwargs):
        super().__init__()
        self.num_labels = label_seq_length
        self._build(num_model, num_head, num_feedforward, num_encoder_layers, num_decoder_layers,
                    dropout, activation, normalize_before, num_points_per_line, num_lines, point_dim,
                    label_seq_length, token, teacher_forcing_ratio)
        # One sequence per wireframe: a micro-batch is cut by sequences, not by `chunk_wireframes` wireframes.  256 sequences
        # x (label_seq_length - 1) positions = 66 k active rows at the last step of configs A / D (1.6 GB of scratch).
        self.chunk_max_seqs = 256
        # False: the reference's batch rule -- stop when the CUMULATIVE count of EOS tokens equals the batch size
        # (model.py:191,207-210; a sample that repeats its EOS can end a batch before another sample has produced its own).
        # True: stop at the first step by which EVERY wireframe has produced an EOS (FF_STOP_EACH_EOS) -- what a caller needs
        # when the records of a batch must equal those of one-wireframe decodes (main.py --batch-size, dist.decode_to_face_json).
        self.stop_each_eos = False

    def get_embeddings(self, input, label):
        val_embed = self.val_enc(input)
        return val_embed, self.pos_enc(val_embed), self.query_pos_enc(label)

    def forward_eval(self, inputs):
        """inputs: input N x L x P x D, input_mask N x L (True = padding), label N x T (shape only).
        Adds predict N x T (int64), embedding N x S x E, pointer N x t_last x E.

        sequence_samples = R in 1..64 (0: the greedy decode above): R independent draws per wireframe under
        sample_temperature / sample_top_k / sample_top_p, decoded together off one encoding.  The uniforms come from
        torch.Generator(device).manual_seed(sample_seed), or from inputs["sample_uniforms"] [T-1, N*R] fp32 (column w*R + k).
        Every draw starts from SOS and is finished by its own EOS; the decode stops once every draw is.  Adds predict_samples
        N x R x T (zero behind a draw's EOS and the stop step), predict_sample_logprob N x R x T (the model's log-probability of
        every drawn token) and predict_sample_scores N x R (their sums); predict is draw 0; embedding as above; no pointer.
        stop_each_eos is not looked at.  Not with return_logprob, an extra mask or the sub-module loop (ValueError).

        sequence_beams = W in 1..8, at most S (0: the greedy decode above): beam search with W beams per wireframe,
        decoded together off one encoding.  Every beam starts from SOS (beam 0 alone non-empty) and is finished by its own EOS;
        sequence_beam_stop "all" stops once no non-empty beam is unfinished, "best" once every wireframe's best beam is finished
        (exact for that beam; the others are returned as they stand).  Adds predict_beams N x W x T (best first, zero behind a
        beam's EOS and the stop step), predict_beam_scores N x W (summed log-probabilities; -inf: an empty rank) and
        predict_beam_finished N x W (int32); predict is beam 0; embedding as above; no pointer.  stop_each_eos is not looked at.
        Not with sequence_samples, beam_width, return_logprob, an extra mask or the sub-module loop (ValueError).

        sequence_constrain = "no_repeat" / "loops" / "coedge_loops" (None: the greedy decode above; the flag bits
        0..7 are taken too): the greedy decode under the face-loop rule applied per face of the row -- no edge twice in a face,
        under "loops" every edge starts where the last one ended, SEP only behind a closed non-empty loop (or alone at a dead end,
        where the face is abandoned and the row goes on), EOS only with the loop closed; "coedge_loops" also takes no co-edge
        twice in the row.  The table comes from inputs["follow_table"] or from the end points of inputs["input"] with
        constrain_tol; none is built without CONNECT.  Every row is finished by its own EOS; the decode stops once every row is.
        Adds predict N x T (zero behind the row's EOS and the stop step), predict_logprob N x T (under the renormalised
        distribution), predict_dead_end N x T (int32: 1 where the SEP was selected at a dead end), predict_open_end N (int32: a
        loop is open after the last kept position); embedding as above; no pointer.  Not with sequence_samples, sequence_beams,
        return_logprob, an extra mask, stop_each_eos = True or the sub-module loop (ValueError).

        sequence_constrain_samples = R in 1..64 (only with sequence_constrain; 0: the decode above): R independent
        draws per wireframe from the row the rule leaves, under sample_temperature / sample_top_k / sample_top_p and with the
        uniforms of sequence_samples (sample_seed, or inputs["sample_uniforms"] [T-1, N*R]).  Every draw carries its own state of
        the rule and is finished by its own EOS.  Adds predict_samples, predict_sample_logprob, predict_sample_dead_end N x R x T,
        predict_sample_scores, predict_sample_open_end N x R; predict, predict_logprob, predict_dead_end and predict_open_end are
        draw 0; embedding as above; no pointer.  Refused wherever sequence_constrain is, and with sequence_samples or
        sequence_beams (ValueError).

        sequence_constrain_beams = W in 1..8 (only with sequence_constrain; 0: the decode above): the W best rows per
        wireframe among the rows the rule leaves, under sequence_beam_stop ("all" / "best").  Every beam carries its own state of the
        rule.  Adds predict_beams, predict_beam_dead_end N x W x T, predict_beam_scores, predict_beam_finished,
        predict_beam_open_end N x W; predict, predict_dead_end and predict_open_end are beam 0 (no predict_logprob); embedding as
        above; no pointer.  Refused wherever sequence_constrain is, and with sequence_samples, sequence_beams or
        sequence_constrain_samples (ValueError).

        sequence_faces = "parse" / "enclosed" (default False): also inputs["sequence_faces"], a dict of device
        tensors -- len, start, type, closed, loops, score, dup_of, take, row_best, rep, votes, best, major N x G x P, edges, loop_of
        N x G x T, set_bits N x G x P x ceil(L/32), count N x G, num_faces N -- made by two launches behind the decode from the rows
        it published (G = the number of draws, the beam width, or 1; P = sequence_faces_slots, None: T // 2);
        faces.faces_of_seq_rows turns one wireframe's arrays into the list forms.  Nothing of the decode changes; an empty batch
        publishes the same keys as empty tensors.  Not with the sub-module loop (ValueError)."""
        label = inputs["label"]
        T = self.num_labels
        self._decode_mode(inputs, parallel=False)       # (the records' reasons: hip/modes.py)
        extract = self._sequence_faces_value(inputs, parallel=False)
        mode, value = self._sequence_mode(inputs)
        G = value if mode is not None and mode.per_anchor else 1       # draws or beams per wireframe
        if inputs["input"].size(0) == 0:     # an empty batch: the reference's loop stops after its first step (0 EOS == batch size 0, model.py:207)
            dev, S = inputs["input"].device, inputs["input"].size(1) + self.num_token
            inputs["embedding"] = torch.zeros((0, S, self.num_model), device=dev)
            inputs["pointer"] = torch.zeros((0, 1, self.num_model), device=dev)
            inputs["predict"] = torch.zeros((0, T), dtype=torch.long, device=dev)
            if getattr(self, "return_logprob", False):
                inputs["predict_logprob"] = torch.zeros((0, T), device=dev)
            if mode is not None:             # (the keys, dtypes and trailing shapes of a non-empty batch)
                del inputs["pointer"]
                for key, dims, dtype in mode.outs:
                    inputs["predict_" + key] = torch.zeros((0,) + tuple({"G": G, "T": T}[d] for d in dims), dtype=dtype, device=dev)
            if extract:                      # (the keys, dtypes and trailing shapes of a non-empty batch; nothing is launched)
                P = getattr(self, "sequence_faces_slots", None) or max(T // 2, 1)
                z = lambda dtype, *shape: torch.zeros((0,) + shape, dtype=dtype, device=dev)
                found = {k: z(torch.int32, G, P) for k in ("len", "start", "type", "closed", "loops", "dup_of", "take", "rep", "votes", "major")}
                found.update({k: z(torch.float64, G, P) for k in ("score", "row_best", "best")})
                found.update(count=z(torch.int32, G), edges=z(torch.int32, G, T), loop_of=z(torch.int32, G, T), num_faces=z(torch.int32),
                             set_bits=z(torch.int32, G, P, (inputs["input"].size(1) + 31) // 32))
                inputs["sequence_faces"] = found
            return inputs
        if not self.engine_supported():      # post-norm / gelu constructor arguments: the sub-module loop (models/common.py)
            return self._forward_eval_modules(inputs, parallel=False)
        if label.size(1) < T - 1:
            raise ValueError("label has %d positions but label_seq_length-1=%d query positions are "
                             "needed" % (label.size(1), T - 1))
        want_lp = bool(getattr(self, "return_logprob", False))
        eng, memory, mask, kv_len = self._encode(inputs)
        if mode is not None:
            inputs = self._forward_eval_sequence(inputs, eng, memory, mask, kv_len, T, mode, value, G)
        else:
            out = eng.decode(memory, mask, kv_len, _L.FF_SEQ2SEQ, T=T, F=1,
                             chunk_wireframes=self.chunk_wireframes, chunk_seqs=self.chunk_seqs,
                             chunk_max_seqs=self.chunk_max_seqs, num_streams=self.num_streams, sync_every=1,
                             flags=self.decode_flags | (_L.FF_STOP_EACH_EOS if self.stop_each_eos else 0),
                             x3_min_rows=self.x3_min_rows, ln_fuse_max_rows=self.ln_fuse_max_rows, tok_sos=self.token.SOS, tok_eos=self.token.EOS,
                             return_pointer=True, extra_mask=self._extra_mask(inputs), logprob=want_lp)
            inputs["embedding"] = memory
            inputs["pointer"] = out["pointer"].transpose(0, 1)
            inputs["predict"] = out["predict"]
            if want_lp:
                inputs["predict_logprob"] = out["logprob"]
        if extract:
            inputs["sequence_faces"] = self._sequence_faces_of_decode(inputs, extract, memory.device)
        return inputs

    def _sequence_faces_of_decode(self, inputs, extract, device, greedy_only=False):
        """inputs["sequence_faces"]: ops.face_seq_rows + ops.face_seq_votes on the rows the decode published --
        predict_samples with predict_sample_logprob, or predict_beams with predict_beam_scores and predict_beam_finished, else
        predict (with predict_logprob when there is one; greedy_only: predict alone, whatever else was published).  "enclosed":
        the enclosure walk on inputs["follow_table"] or on the table built from the end points with constrain_tol, only closed
        faces are counted, and inputs["edge_map"] maps the edges of the key.  The edge count of a wireframe is inputs["num_input"]
        when given, else its unmasked edges.  Returns a dict of device tensors N x G x P ..., count N x G, num_faces N."""
        from ..hip import ops as _ops
        if "predict_samples" in inputs and not greedy_only:
            tokens, kw = inputs["predict_samples"], dict(logprob=inputs["predict_sample_logprob"])
        elif "predict_beams" in inputs and not greedy_only:
            tokens = inputs["predict_beams"]
            kw = dict(scores=inputs["predict_beam_scores"], finished=inputs["predict_beam_finished"])
        else:
            tokens, kw = inputs["predict"], dict(logprob=inputs.get("predict_logprob"))
        ni = self._edge_counts(inputs, device)
        enclosed = extract == "enclosed"
        edge_map = inputs.get("edge_map")
        found = _ops.face_seq_rows(tokens, ni, self.token, slots=getattr(self, "sequence_faces_slots", None),
                                   follows=self._follow_table(inputs, device, ni, None) if enclosed else None,
                                   edge_map=None if edge_map is None else edge_map.to(device), closed_only=enclosed,
                                   num_lines=inputs["input"].size(1), **kw)
        found.update(_ops.face_seq_votes(found, require_closed=enclosed))
        return found

    def _edge_counts(self, inputs, device):
        """The edge count of every wireframe, int32 [N] on `device`: inputs["num_input"] when given, else its unmasked edges."""
        ni = inputs.get("num_input")
        if ni is None:
            ni = (~inputs["input_mask"].to(device=device, dtype=torch.bool)).sum(dim=1)
        return torch.as_tensor(ni).to(device=device, dtype=torch.int32).reshape(-1)

    def _sequence_mode(self, inputs):
        """(record, value) of the one of SEQUENCE_MODES this model's attributes switch on (hip/modes.py; value: the draws, the
        width or the flag bits), else (None, None), after the rules only the model can check (ValueError, before anything is
        launched): the native engine, what the record excludes, its own value checks."""
        found = (None, None)
        for mode in _modes.SEQUENCE_MODEL_ORDER:
            sw = mode.switches[0]
            value = mode.sequence.value(getattr(self, sw.attr, sw.off))
            if value == sw.off:
                continue
            if not self.engine_supported():
                raise ValueError("%s needs the native engine: this model's constructor arguments take the sub-module loop" % sw.attr)
            if any(inputs.get("extra_mask") is not None if word == "an extra mask" else getattr(self, word, False)
                   for word in mode.model_excludes):
                raise ValueError("%s excludes %s and %s" % (sw.attr, ", ".join(mode.model_excludes[:-1]), mode.model_excludes[-1]))
            mode.sequence.model_values(self, value, inputs)
            found = (mode, value)
        # sequence_constrain's option: read behind the recorded refusals above, which keep their texts
        SC = found[1] if found[0] is _modes.SEQUENCE_CONSTRAIN else None
        R = _modes.sequence_constrain_samples_value(getattr(self, "sequence_constrain_samples", 0), SC,
                                                    getattr(self, "sequence_samples", 0), getattr(self, "sequence_beams", 0))
        if R:
            found = (_modes.SEQUENCE_CONSTRAIN_SAMPLE, R)
            found[0].sequence.model_values(self, R, inputs)
        # sequence_constrain's other option, likewise behind the recorded refusals
        W = _modes.sequence_constrain_beams_value(getattr(self, "sequence_constrain_beams", 0), SC,
                                                  getattr(self, "sequence_samples", 0), getattr(self, "sequence_beams", 0),
                                                  getattr(self, "sequence_constrain_samples", 0))
        if W:
            found = (_modes.SEQUENCE_CONSTRAIN_BEAM, W)
            found[0].sequence.model_values(self, W, inputs)
        # the closure look-ahead of sequence_constrain and of its sampled form, likewise behind the recorded refusals
        closure = _modes.sequence_constrain_closure_value(getattr(self, "sequence_constrain_closure", None), SC, W)
        if closure is not None:
            found = ((_modes.SEQUENCE_CONSTRAIN_SAMPLE_AHEAD, R) if R else (_modes.SEQUENCE_CONSTRAIN_AHEAD, SC))
            found[0].sequence.model_values(self, found[1], inputs)
        # the closure look-ahead of the beam search, a name of its own, likewise behind the recorded refusals
        beam_closure = _modes.sequence_constrain_beam_closure_value(
            getattr(self, "sequence_constrain_beam_closure", None), SC, W, getattr(self, "sequence_constrain_closure", None), R)
        if beam_closure is not None:
            found = (_modes.SEQUENCE_CONSTRAIN_BEAM_AHEAD, W)
            found[0].sequence.model_values(self, W, inputs)
        return found

    def _forward_eval_sequence(self, inputs, eng, memory, mask, kv_len, T, mode, value, G):
        """forward_eval with one of SEQUENCE_MODES on behind the encoder.  The wireframes are decoded in batch order (this model
        applies no permutation): row w*G + k of the engine's outputs is draw / beam k of wireframe w as given."""
        N = memory.size(0)
        out = eng.decode(memory, mask, kv_len, _L.FF_SEQ2SEQ, T=T, F=1,
                         chunk_wireframes=self.chunk_wireframes, chunk_seqs=self.chunk_seqs,
                         chunk_max_seqs=self.chunk_max_seqs, num_streams=self.num_streams, sync_every=1, flags=self.decode_flags,
                         x3_min_rows=self.x3_min_rows, ln_fuse_max_rows=self.ln_fuse_max_rows, tok_sos=self.token.SOS,
                         tok_eos=self.token.EOS, **mode.prepare(self, value, inputs, memory.device, T, N, 1, None, None))
        inputs["embedding"] = memory
        inputs["predict"] = out["predict"]
        for key, dims, _ in mode.outs:
            inputs["predict_" + key] = out[key].view((N,) + tuple({"G": G, "T": T}[d] for d in dims))
        setattr(self, mode.sequence.stats, {"steps": out["steps"], "slot_rows": out["slot_rows"]})
        return inputs

    def label_paths(self, inputs):
        """score()'s defaults, the data set's own labels: (paths N x T = label, lengths N = num_label - 1)."""
        return inputs["label"][:, :self.num_labels], torch.as_tensor(inputs["num_label"]).reshape(-1) - 1

    @torch.no_grad()
    def score(self, inputs, paths=None, lengths=None):
        """Teacher-forced scoring of token sequences.  paths N x T int64 shaped like predict (column 0: SOS),
        lengths N in 0..T-1: positions 1..lengths are scored.  Defaults: the data set's own labels, paths = label and lengths =
        num_label - 1.  Adds score_logprob / score_greedy / score_rank N x T and score_seq_logprob N; see
        SurfaceFormer_Parallel.score.  Not with return_logprob, an extra mask or the sub-module loop; stop_each_eos, a rule of the
        greedy decode, is not looked at."""
        T = self.num_labels
        if paths is None:
            paths, default_lengths = self.label_paths(inputs)
            lengths = default_lengths if lengths is None else lengths
        elif lengths is None:
            raise ValueError("score(): paths need lengths")
        paths = torch.as_tensor(paths).to(torch.int64)
        if paths.dim() != 2 or paths.size(0) != inputs["input"].size(0) or paths.size(1) != T:
            raise ValueError("paths must be N x %d" % T)
        return self._score(inputs, _L.FF_SEQ2SEQ, T, 1, paths, torch.as_tensor(lengths).reshape(-1))
