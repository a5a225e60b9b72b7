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
        W = self._sequence_beams_value(inputs)
        R = self._sequence_samples_value(inputs)
        SC = self._sequence_constrain_value(inputs)
        if inputs["input"].size(0) == 0:     # an empty batch: the reference's loop stops after its first step (0 EOS == batch size 0, model.py:207)
            dev, S = inputs["input"].device, inputs["input"].size(1) + self.num_token
            inputs["embedding"] = torch.zeros((0, S, self.num_model), device=dev)
            inputs["pointer"] = torch.zeros((0, 1, self.num_model), device=dev)
            inputs["predict"] = torch.zeros((0, T), dtype=torch.long, device=dev)
            if getattr(self, "return_logprob", False):
                inputs["predict_logprob"] = torch.zeros((0, T), device=dev)
            if R:
                del inputs["pointer"]
                inputs["predict_samples"] = torch.zeros((0, R, T), dtype=torch.long, device=dev)
                inputs["predict_sample_logprob"] = torch.zeros((0, R, T), device=dev)
                inputs["predict_sample_scores"] = torch.zeros((0, R), device=dev)
            if W:
                del inputs["pointer"]
                inputs["predict_beams"] = torch.zeros((0, W, T), dtype=torch.long, device=dev)
                inputs["predict_beam_scores"] = torch.zeros((0, W), device=dev)
                inputs["predict_beam_finished"] = torch.zeros((0, W), dtype=torch.int32, device=dev)
            if SC is not None:
                del inputs["pointer"]
                inputs["predict_logprob"] = torch.zeros((0, T), device=dev)
                inputs["predict_dead_end"] = torch.zeros((0, T), dtype=torch.int32, device=dev)
                inputs["predict_open_end"] = torch.zeros((0,), dtype=torch.int32, device=dev)
            if extract:                      # (the keys, dtypes and trailing shapes of a non-empty batch; nothing is launched)
                G, P = max(R, W, 1), getattr(self, "sequence_faces_slots", None) or max(T // 2, 1)
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
        if W or R:
            inputs = self._forward_eval_beams(inputs, eng, memory, mask, kv_len, T, W) if W else \
                self._forward_eval_samples(inputs, eng, memory, mask, kv_len, T, R)
            if extract:
                inputs["sequence_faces"] = self._sequence_faces_of_decode(inputs, extract, memory.device)
            return inputs
        if SC is not None:
            inputs = self._forward_eval_constrained(inputs, eng, memory, mask, kv_len, T, SC)
            if extract:
                inputs["sequence_faces"] = self._sequence_faces_of_decode(inputs, extract, memory.device)
            return inputs
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
        ni = inputs.get("num_input")
        if ni is None:
            ni = (~inputs["input_mask"].to(device=device, dtype=torch.bool)).sum(dim=1)
        ni = torch.as_tensor(ni).to(device=device, dtype=torch.int32).reshape(-1)
        enclosed = extract == "enclosed"
        edge_map = inputs.get("edge_map")
        found = _ops.face_seq_rows(tokens, ni, self.token, slots=getattr(self, "sequence_faces_slots", None),
                                   follows=self._follow_table(inputs, device, ni, None) if enclosed else None,
                                   edge_map=None if edge_map is None else edge_map.to(device), closed_only=enclosed,
                                   num_lines=inputs["input"].size(1), **kw)
        found.update(_ops.face_seq_votes(found, require_closed=enclosed))
        return found

    def _sequence_constrain_value(self, inputs):
        """sequence_constrain as None or its flag bits, after the rules only the model can check (ValueError, before anything is
        launched): the native engine, what the record excludes, stop_each_eos."""
        SC = _modes.sequence_constrain_flags(getattr(self, "sequence_constrain", None))
        if SC is None:
            return None
        mode = _modes.SEQUENCE_CONSTRAIN
        if not self.engine_supported():
            raise ValueError("sequence_constrain needs the native engine: this model's constructor arguments take the sub-module loop")
        if getattr(self, "sequence_samples", 0) or getattr(self, "sequence_beams", 0) or getattr(self, "return_logprob", False) or \
                inputs.get("extra_mask") is not None:
            raise ValueError("sequence_constrain excludes %s, %s, %s and %s" % mode.model_excludes)
        if getattr(self, "stop_each_eos", False):
            raise ValueError("sequence_constrain excludes stop_each_eos = True: every row is finished by its own EOS already")
        return SC

    def _forward_eval_constrained(self, inputs, eng, memory, mask, kv_len, T, SC):
        """forward_eval with sequence_constrain (flag bits SC) behind the encoder.  The wireframes are decoded in batch order
        (this model applies no permutation), so the follow table is taken as built or given."""
        dev = memory.device
        table = None
        if SC & _L.FF_CONSTRAIN_CONNECT:
            ni = inputs.get("num_input")
            if ni is None:
                ni = (~inputs["input_mask"].to(device=dev, dtype=torch.bool)).sum(dim=1)
            ni = torch.as_tensor(ni).to(device=dev, dtype=torch.int32).reshape(-1)
            table = self._follow_table(inputs, dev, ni, None)
        out = eng.decode(memory, mask, kv_len, _L.FF_SEQ2SEQ, T=T, F=1,
                         chunk_wireframes=self.chunk_wireframes, chunk_seqs=self.chunk_seqs,
                         chunk_max_seqs=self.chunk_max_seqs, num_streams=self.num_streams, sync_every=1, flags=self.decode_flags,
                         x3_min_rows=self.x3_min_rows, ln_fuse_max_rows=self.ln_fuse_max_rows, tok_sos=self.token.SOS,
                         tok_eos=self.token.EOS, tok_sep=int(getattr(self.token, "SEP", 2)), sequence_constrain=SC, follow_table=table)
        inputs["embedding"] = memory
        inputs["predict"] = out["predict"]
        inputs["predict_logprob"] = out["logprob"]
        inputs["predict_dead_end"] = out["dead_end"]
        inputs["predict_open_end"] = out["open_end"]
        self.last_constrain_stats = {"steps": out["steps"], "slot_rows": out["slot_rows"]}
        return inputs

    def _sequence_beams_value(self, inputs):
        """sequence_beams as 0 or W in 1..8, after the rules only the model can check (ValueError, before anything is launched):
        the native engine, what the record excludes, the width against S, the stop value."""
        W = _modes.sequence_beams_value(getattr(self, "sequence_beams", 0))
        if not W:
            return 0
        mode = _modes.SEQUENCE_BEAM
        if not self.engine_supported():
            raise ValueError("sequence_beams needs the native engine: this model's constructor arguments take the sub-module loop")
        if getattr(self, "sequence_samples", 0) or getattr(self, "beam_width", 0) or getattr(self, "return_logprob", False) or \
                inputs.get("extra_mask") is not None:
            raise ValueError("sequence_beams excludes %s, %s, %s and %s" % mode.model_excludes)
        _modes.check_options(mode, _L.FF_SEQ2SEQ, dict(sequence_beams=W, sequence_beam_stop=getattr(self, "sequence_beam_stop", "all"),
                                                      S=inputs["input"].size(1) + self.num_token), None)
        return W

    def _forward_eval_beams(self, inputs, eng, memory, mask, kv_len, T, W):
        """forward_eval with sequence_beams = W behind the encoder.  The wireframes are decoded in batch order (this model applies
        no permutation): row w*W + k of the engine's outputs is beam k of wireframe w as given."""
        N = memory.size(0)
        out = eng.decode(memory, mask, kv_len, _L.FF_SEQ2SEQ, T=T, F=1,
                         chunk_wireframes=self.chunk_wireframes, chunk_seqs=self.chunk_seqs,
                         chunk_max_seqs=self.chunk_max_seqs, num_streams=self.num_streams, sync_every=1, flags=self.decode_flags,
                         x3_min_rows=self.x3_min_rows, ln_fuse_max_rows=self.ln_fuse_max_rows, tok_sos=self.token.SOS,
                         tok_eos=self.token.EOS, sequence_beams=W, sequence_beam_stop=self.sequence_beam_stop)
        inputs["embedding"] = memory
        inputs["predict"] = out["predict"]
        inputs["predict_beams"] = out["beams"].view(N, W, T)
        inputs["predict_beam_scores"] = out["beam_scores"].view(N, W)
        inputs["predict_beam_finished"] = out["beam_finished"].view(N, W)
        self.last_beam_stats = {"steps": out["steps"], "slot_rows": out["slot_rows"]}
        return inputs

    def _sequence_samples_value(self, inputs):
        """sequence_samples as 0 or R in 1..64, after the rules only the model can check (ValueError, before anything is
        launched): the native engine, what the record excludes, the parameters' ranges, the shape of inputs["sample_uniforms"]."""
        R = _modes.sequence_samples_value(getattr(self, "sequence_samples", 0))
        if not R:
            return 0
        mode = _modes.SEQUENCE_SAMPLE
        if not self.engine_supported():
            raise ValueError("sequence_samples needs the native engine: this model's constructor arguments take the sub-module loop")
        if getattr(self, "return_logprob", False) or inputs.get("extra_mask") is not None:
            raise ValueError("sequence_samples excludes %s and %s" % mode.model_excludes)
        _modes.check_options(mode, _L.FF_SEQ2SEQ, dict(sequence_samples=R, temperature=self.sample_temperature,
                                                      top_k=self.sample_top_k, top_p=self.sample_top_p), None)
        u = inputs.get("sample_uniforms")
        shape = (max(self.num_labels - 1, 1), inputs["input"].size(0) * R)
        if u is not None and tuple(torch.as_tensor(u).shape) != shape:
            raise ValueError("sample_uniforms must have shape [%d, %d]" % shape)
        return R

    def _forward_eval_samples(self, inputs, eng, memory, mask, kv_len, T, R):
        """forward_eval with sequence_samples = R behind the encoder.  The wireframes are decoded in batch order (this model
        applies no permutation), so column w*R + k of the uniforms is draw k of wireframe w as given."""
        N, dev = memory.size(0), memory.device
        u = inputs.get("sample_uniforms")
        if u is None:
            gen = torch.Generator(device=dev).manual_seed(int(self.sample_seed))
            u = torch.rand((max(T - 1, 1), N * R), generator=gen, device=dev, dtype=torch.float32)
        else:
            u = torch.as_tensor(u).to(device=dev, dtype=torch.float32).contiguous()
        out = eng.decode(memory, mask, kv_len, _L.FF_SEQ2SEQ, T=T, F=1,
                         chunk_wireframes=self.chunk_wireframes, chunk_seqs=self.chunk_seqs,
                         chunk_max_seqs=self.chunk_max_seqs, num_streams=self.num_streams, sync_every=1, flags=self.decode_flags,
                         x3_min_rows=self.x3_min_rows, ln_fuse_max_rows=self.ln_fuse_max_rows, tok_sos=self.token.SOS,
                         tok_eos=self.token.EOS, sequence_samples=R, temperature=float(self.sample_temperature),
                         top_k=int(self.sample_top_k), top_p=float(self.sample_top_p), uniforms=u)
        inputs["embedding"] = memory
        inputs["predict"] = out["predict"]
        inputs["predict_samples"] = out["samples"].view(N, R, T)
        inputs["predict_sample_logprob"] = out["sample_logprob"].view(N, R, T)
        inputs["predict_sample_scores"] = out["sample_scores"].view(N, R)
        self.last_sample_stats = {"steps": out["steps"], "slot_rows": out["slot_rows"]}
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
