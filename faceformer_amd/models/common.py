"""Shared plumbing of the two model classes: parameter containers with the reference's names, lazy
binding of those parameters into the native engine, mask/embedding helpers."""
import numpy as _np
import torch
import torch.nn as nn

from .. import faces as _faces
from ..embedding import PositionEmbeddingLearned, VanillaEmedding
from ..hip import lib as _L
from ..hip import modes as _modes
from ..hip import ops
from ..hip.engine import DEFAULT_FLAGS, PathEngine
from ..transformer import (HipLinear, TransformerDecoder, TransformerDecoderLayer, TransformerEncoder,
                           TransformerEncoderLayer)
from ..utils import min_value_of_dtype


SPLIT_KIND_DEFAULT = "fp16x2"   # round 6 (profiles/r06/split_kinds_ab.txt: config B 50.9 -> 45.4 ms, C128 256 k -> 302 k edges/s, margins unchanged)
X3_MIN_ROWS_DEFAULT = 1024   # package default of SurfaceFormerBase.x3_min_rows (bench.py reports this form beside the f32 headline)


class SurfaceFormerBase(nn.Module):
    """Everything SurfaceFormer and SurfaceFormer_Parallel have in common (reference
    models/model.py:14-69 and models/model_para.py:14-70 build identical sub-modules)."""

    def _build(self, num_model, num_head, num_feedforward, num_encoder_layers, num_decoder_layers,
               dropout, activation, normalize_before, num_points_per_line, num_lines, point_dim,
               seq_len, token, teacher_forcing_ratio):
        if token is None:
            raise ValueError("`token` (cfg.model.token) is required")
        self.num_model = num_model
        self.num_head = num_head
        self.teacher_forcing_ratio = teacher_forcing_ratio
        self.token = token
        self.num_token = token.len
        self.normalize_before = normalize_before
        self.activation_name = activation

        self.val_enc = VanillaEmedding(num_points_per_line * point_dim, num_model, token)
        self.pos_enc = PositionEmbeddingLearned(num_model, max_len=num_lines + self.num_token)
        self.query_pos_enc = PositionEmbeddingLearned(num_model, max_len=seq_len)

        enc_layer = TransformerEncoderLayer(num_model, num_head, num_feedforward, dropout, activation,
                                            normalize_before)
        self.encoder = TransformerEncoder(enc_layer, num_encoder_layers,
                                          nn.LayerNorm(num_model) if normalize_before else None)
        dec_layer = TransformerDecoderLayer(num_model, num_head, num_feedforward, dropout, activation,
                                            normalize_before)
        self.decoder = TransformerDecoder(dec_layer, num_decoder_layers, nn.LayerNorm(num_model))
        self.project = HipLinear(num_model, num_model)
        self._reset_parameters()

        # engine knobs (not part of the reference surface)
        self.decode_flags = DEFAULT_FLAGS
        self.chunk_wireframes = 16     # micro-batch size in wireframes (0 = whole batch); 8-32 measured best
        self.chunk_seqs = 0            # >0: split every wireframe into groups of this many sequences
        self.num_streams = 1           # micro-batches are issued round-robin on this many HIP streams
        self.chunk_max_seqs = 8192     # ... and at most this many sequences per micro-batch of several wireframes
        self.sort_by_edges = True      # ragged batches: decode the wireframes sorted by edge count (tight micro-batches)
        self.ln_fuse_max_rows = 0      # LayerNorm folded into the projections on steps with at most this many rows (0: 12288)
        self.sync_every = 1            # the host looks at the stop rule every k steps, one period behind the enqueued steps
                                       # (the queue never drains: free at every step, tools/run_sync_probe.sh); a decode
                                       # that stops at step s executes s + k ... s + 2k - 1 steps
        self.sharded_sync_every = 2    # ... period of the batch-global rule in dist.decode_sharded (a host all-reduce per check)
        # The opt-in decode modes and options (SurfaceFormer_Parallel.forward_eval's docstring says what each adds; hip/modes.py
        # holds what each excludes and where it is not taken: dist.decode_sharded, the single-sequence model, score() -- ValueError)
        self.retire_finished = False   # parallel model: a face loop stops being decoded once it has produced its face-type token;
                                       # `predict` is then faces.retired_view of the reference's (same faces: DESIGN.md 10)
        self.return_logprob = False    # forward_eval also returns inputs["predict_logprob"], shaped like inputs["predict"]: the
                                       # log-probability log_softmax(masked logits)[token] of every greedy selection, 0 at the
                                       # start token and wherever predict is zero padded
        self.last_score_stats = None   # score(): {"rows", "steps"} of the last call
        self.beam_width = 0            # parallel model: >= 1 = beam search with this many beams per anchor; 0 = greedy
        self.num_samples = 0           # parallel model: R >= 1 (at most 64) independent DRAWS per anchor; 0 = greedy
        self.constrain = None          # parallel model: "no_repeat" / "loops", the greedy decode over the keys the harness's
                                       # enclosure filter can accept; None = greedy
        self.constrain_tol = 2e-4      # ... two end points coincide below this distance in x and in y (the harness's
                                       # post_process.enclosedness_tol); inputs["follow_table"] overrides the built table
        self.constrain_beams = 0       # ... W in 1..8 = the beam search over the constrained keys, W beams per anchor;
                                       # 0 = the constrained greedy decode; only with constrain
        self.constrain_beam_closure = None   # ... with "loops" and constrain_beams: "lookahead" / "exact" = the beam search under the
                                       # closure look-ahead or the exact one; None = under the plain rule;
                                       # inputs["close_dist"] / ["cycle_len"] override the built tables
        self.constrain_samples = 0     # ... R in 1..64 = R draws per anchor from the constrained keys under sample_temperature / sample_top_k /
                                       # sample_top_p; 0 = the constrained greedy decode; only with constrain, not with constrain_beams
        self.constrain_lookahead = False   # ... with "loops": also mask every edge from which the loop cannot close within
                                       # max_face_length; inputs["close_dist"] / ["cycle_len"] override the built tables
        self.constrain_exact = False   # ... with "loops": the exact closure look-ahead -- while a loop is open, also mask
                                       # every edge from which it cannot close within max_face_length through edges the row has
                                       # not used; contains constrain_lookahead; inputs["cycle_len"] overrides the built table
        self.extract_faces = False     # parallel model: "parse" / "enclosed" = the decoded rows also leave as faces, on the device
                                       # (inputs["faces"]: ops.face_rows + ops.face_votes behind the decode);
                                       # "enclosed" walks the enclosure rule on the follow table (constrain_tol) and counts
                                       # closed faces only; inputs["edge_map"] (int32 N x L) maps edges before the grouping
        self.sequence_samples = 0      # single-sequence model: R in 1..64 = R independent draws per WIREFRAME under sample_temperature /
                                       # sample_top_k / sample_top_p, decoded together off one encoding; 0 = greedy
        self.sequence_beams = 0        # single-sequence model: W in 1..8 = beam search with W beams per WIREFRAME, decoded together off one
                                       # encoding; 0 = greedy
        self.sequence_beam_stop = "all"  # ... "all": stop once every non-empty beam is finished; "best": once every wireframe's best is
        self.sequence_constrain = None  # single-sequence model: "no_repeat" / "loops" / "coedge_loops" = the greedy decode under the face-loop
                                       # rule applied per face of the row: SEP ends a face, EOS the row, a dead end re-opens
                                       # SEP alone; "coedge_loops" also takes no co-edge twice in the row; None = greedy.  The table is
                                       # built with constrain_tol; inputs["follow_table"] overrides it
        self.sequence_constrain_samples = 0   # ... with sequence_constrain: R in 1..64 = R independent draws per WIREFRAME from the row
                                       # the rule leaves, under sample_temperature / sample_top_k / sample_top_p; 0 = greedy
        self.sequence_constrain_beams = 0     # ... with sequence_constrain: W in 1..8 = the W best rows per WIREFRAME among the rows the
                                       # rule leaves, under sequence_beam_stop; 0 = greedy
        self.sequence_constrain_closure = None   # ... with sequence_constrain "loops" / "coedge_loops", alone or with
                                       # sequence_constrain_samples: "lookahead" / "exact" = the closure look-ahead of the rule (DESIGN.md
                                       # 35): an edge from which the loop cannot close inside the row is masked; the tables are built
                                       # with ops.follow_distance; inputs["close_dist"] / inputs["cycle_len"] override them; None = off
        self.sequence_constrain_beam_closure = None   # ... with sequence_constrain_beams and sequence_constrain "loops" /
                                       # "coedge_loops": "lookahead" / "exact" = that look-ahead per beam of the beam search (DESIGN.md
                                       # 36), every beam against its own (first, prev) and visited edges; tables as above; None = off
        self.sequence_faces = False    # single-sequence model: "parse" / "enclosed" = the decoded rows also leave as faces, on the device
                                       # (inputs["sequence_faces"]: ops.face_seq_rows + ops.face_seq_votes behind the decode,
                                       # DESIGN.md 31); "enclosed" walks the enclosure rule on the follow table (constrain_tol) and
                                       # counts closed faces only; inputs["edge_map"] (int32 N x L) maps edges before the grouping
        self.sequence_faces_slots = None   # ... P face slots per row; None = label_seq_length // 2, which never truncates
        self.sample_temperature = 1.0  # ... logits are divided by it; 0 = the argmax
        self.sample_top_k = 0          # ... keep the K most probable keys (ties at the threshold included); 0 = all
        self.sample_top_p = 1.0        # ... keep the most probable keys up to this share of the mass; 1 = all
        self.sample_seed = 0           # ... seed of the torch.Generator that makes the uniforms; inputs["sample_uniforms"]
                                       # [T-1, N*F*R] fp32, column (w*F + f)*R + k in the batch's own order, overrides it
        # Decoder projections of launches with at least this many rows (q|k|v; linear1 from 7/4 x, the 512-column ones from
        # 11/4 x as many) run as 3 x bf16 split products on the bf16 matrix cores: fp32-accurate (error vs fp64 = an fp32 dot
        # product's, tests/test_hip_ops.py), LayerNorm folding included (ff_gemm_x3_ln), and 1.3-1.6x the f32-MFMA kernel
        # from ~3000 rows on (profiles/r04/gemm_x3_variants.txt).  0 = off.
        self.x3_min_rows = X3_MIN_ROWS_DEFAULT
        # ... their LayerNorm applied in the consumer's EPILOGUE (rstd (x W'^T - mean colsum(W'))): the K loop then is the plain
        # split product.  Error factor (1 + |mean| / sigma) of the row -- 0.06 median, 0.15 maximum on this model's LayerNorm
        # inputs; False = rows normalised before the product (ff_gemm_x3.hip: x3_ln_linear).  Read when the engine is bound.
        # None = by split kind: True for the bf16 terms (+5-13 % there), False for the fp16 terms (config B 44.3-44.8 vs 44.9 ms, C128 313 k vs
        # 309 k edges/s with the rows normalised first: profiles/r06/fp16x2_ln_form_ab.txt -- and normalised rows are bounded by sqrt(E),
        # so nothing un-normalised ever meets fp16's range).
        self.x3_ln_in_epilogue = None
        # how those projections split an fp32 operand: "bf16x3" (three bf16 terms, six products) or "fp16x2" (two fp16 terms, three
        # products: half the matrix-core work; the engine checks at bind time that the model's operand bounds fit fp16's range).
        # "fp16" (opt-in, main.py --fp16): ONE fp16 product with fp32 accumulation, the reference's 16-bit GPU arithmetic -- for
        # these projections and the cross-attention only; same range check and bf16x3 fallback
        self.split_kind = SPLIT_KIND_DEFAULT
        self._engine_obj = None

    def _reset_parameters(self):
        # every tensor with more than one dim is re-drawn xavier-uniform (reference model.py:49-52)
        for _, param in self.named_parameters():
            if param.dim() > 1:
                nn.init.xavier_uniform_(param)

    # ---- helpers that exist on the reference classes -------------------------------------------
    def process_masks(self, input_mask, tgt_mask=None):
        """Prepend `num_token` never-masked columns (reference model.py:61-69)."""
        pad = torch.zeros((len(input_mask), self.num_token), device=input_mask.device).type_as(input_mask)
        input_mask = torch.cat([pad, input_mask], dim=1)
        if tgt_mask is None:
            return input_mask
        return input_mask, tgt_mask[..., :-1].contiguous()

    def generate_square_subsequent_mask(self, sz):
        return torch.triu(torch.ones(sz, sz, dtype=torch.bool), diagonal=1)

    def patch_source(self, src, pos):
        return src.transpose(0, 1), pos.transpose(0, 1)

    def select_next(self, embedding, pointer, input_mask):
        """embedding S x B x E, pointer t x B x E, input_mask B x S (True = masked) -> 1 x B tokens
        (reference model.py:161-167); runs the HIP pointer kernel."""
        mem = embedding.transpose(0, 1).contiguous()
        res = ops.pointer_argmax(pointer[-1].contiguous(), mem, mask=input_mask.to(torch.uint8).contiguous(),
                                 seqs_per_group=1)
        return res["next"].to(torch.long).unsqueeze(0)

    def forward_train(self, inputs, scheduled_sampling_ratio=0):
        raise NotImplementedError(
            "teacher-forced training (reference forward_train) is out of scope of the MI355X decode "
            "build; this package implements the greedy eval path")

    # ---- native engine binding --------------------------------------------------------------------
    def engine_supported(self):
        """The native engine (ff_encode / ff_decode) implements what every reference config uses: pre-norm layers with relu
        feed-forward blocks and 64-wide attention heads (num_model / num_head = 512 / 8).  The other constructor arguments of
        the reference (model.py:14-18: `normalize_before=False`, `activation="gelu"`, any head width) decode through
        `_forward_eval_modules`."""
        return bool(self.normalize_before) and self.activation_name == "relu" and \
            self.num_model == self.num_head * _L.FF_HEAD_DIM

    def _check_supported(self):
        if not self.normalize_before:
            raise NotImplementedError("the native decode engine implements the pre-norm path "
                                      "(normalize_before=True, what every reference config uses)")
        if self.activation_name != "relu":
            raise NotImplementedError("the native decode engine implements relu feed-forward layers")
        if self.num_model != self.num_head * _L.FF_HEAD_DIM:
            raise NotImplementedError("the native decode engine implements %d-wide attention heads (num_model / num_head = 512 / 8 in "
                                      "every reference config); other widths decode through the sub-module loop" % _L.FF_HEAD_DIM)

    def _forward_eval_modules(self, inputs, parallel):
        """Greedy decode of a model the native engine does not implement (post-norm layers, gelu, head widths other than 64), driven from Python over
        this package's HIP sub-modules: `encoder` / `decoder` / `project` run ff_layernorm / ff_gemm_f32 / ff_attention /
        ff_gelu, the pointer head is ff_pointer_argmax.  Same semantics as the reference's loops (model_para.py:181-241,
        model.py:169-219): whole prefix re-decoded every step, `finfo.min` mask fill, lowest index on ties, the parallel
        model's current-step stop rule / the single-sequence model's cumulative EOS count, zero padding afterwards.
        One launch per operator and a host synchronisation per step (the stop rule): a module-level path for constructor
        arguments no reference config uses, not the tuned engine -- still HIP kernels only, no CPU fallback."""
        inp, label = inputs["input"], inputs["label"]
        if not inp.is_cuda:
            raise _L.HipExtensionError("inputs['input'] is on %s; expected a ROCm device tensor" % inp.device)
        N, E, nt = inp.size(0), self.num_model, self.num_token
        T = self.max_face_length if parallel else self.num_labels
        mask = self.process_masks(inputs["input_mask"]).to(torch.bool)               # N x S, True = never a key / never selected
        val, pos, qpos = self.get_embeddings(inp.to(torch.float32), label)
        src, pos = self.patch_source(val, pos)                                          # S x N x E, S x 1 x E
        qpos = qpos.transpose(0, 1)[: T - 1]                                            # (T-1) x 1 x E
        memory = self.encoder(src, src_key_padding_mask=mask, pos=pos)                  # S x N x E
        mem_rows = memory.transpose(0, 1).contiguous()                                  # N x S x E: pointer keys, one copy per wireframe
        if parallel:
            ni_in = inputs["num_input"]
            num_input = [int(n) for n in (ni_in.tolist() if torch.is_tensor(ni_in) else ni_in)]
            F = max(num_input)
            start = torch.arange(F, device=inp.device, dtype=torch.long).repeat(N, 1)   # anchors WITHOUT the token offset
            for i, n in enumerate(num_input):
                start[i, n:] = nt - 1                                                    # padding anchors (model_para.py:204-205)
            tokens = start.reshape(1, N * F)
            mem_seq, mask_seq = memory.repeat_interleave(F, 1), mask.repeat_interleave(F, 0)
        else:
            F = 1
            tokens = torch.full((1, N), self.token.SOS, dtype=torch.long, device=inp.device)
            mem_seq, mask_seq = memory, mask
        mask_u8 = mask.to(torch.uint8).contiguous()
        extra = self._extra_mask(inputs)
        eos_seen, pointer = 0, None
        trace = getattr(self, "_module_trace", None)        # tests: a list that receives the masked logits of every step
        want_lp = bool(getattr(self, "return_logprob", False))
        lps = [torch.zeros(tokens.size(1), device=inp.device)] if want_lp else []   # position 0: the start token is not selected
        if trace is not None:
            self._module_memory = mem_rows
        for step in range(T - 1):
            tgt = torch.gather(mem_seq, 0, tokens.unsqueeze(-1).expand(-1, -1, E))        # (step+1) x B x E
            pointer = self.project(self.decoder(tgt, mem_seq, memory_key_padding_mask=mask_seq, pos=pos,
                                                query_pos=qpos[: step + 1]))
            res = ops.pointer_argmax(pointer[-1].contiguous(), mem_rows, mask=mask_u8, extra_mask=extra,
                                     seqs_per_group=F, want_logits=trace is not None, want_logprob=want_lp)
            nxt = res["next"].to(torch.long).unsqueeze(0)
            if want_lp:
                lps.append(res["logprob"])
            if trace is not None:
                trace.append(res["logits"])
            tokens = torch.cat((tokens, nxt), dim=0)
            if parallel:
                if bool((nxt < nt).all()):
                    break
            else:
                eos_seen += int((nxt == self.token.EOS).sum())
                if eos_seen == N:
                    break
        pad = torch.zeros((T - tokens.size(0), tokens.size(1)), dtype=torch.long, device=inp.device)
        predict = torch.cat((tokens, pad), dim=0).transpose(0, 1)
        if want_lp:
            lp = torch.cat((torch.stack(lps), pad.to(torch.float32)), dim=0).transpose(0, 1)
            inputs["predict_logprob"] = lp.reshape(N, F, T) if parallel else lp.contiguous()
        if parallel:
            inputs["predict"] = predict.reshape(N, F, T)
        else:
            inputs["embedding"] = mem_rows
            inputs["pointer"] = pointer.transpose(0, 1)
            inputs["predict"] = predict
        return inputs

    def _ln_in_epilogue(self):
        v = getattr(self, "x3_ln_in_epilogue", None)
        return (getattr(self, "split_kind", SPLIT_KIND_DEFAULT) == "bf16x3") if v is None else bool(v)

    def engine(self):
        """PathEngine bound to this module's parameters (rebuilt when they moved, e.g. after .to())."""
        self._check_supported()
        eng = self._engine_obj
        if eng is None or not eng.pointers_current() or eng.has_planes != (self.x3_min_rows > 0) or \
                eng.ln_in_epilogue != self._ln_in_epilogue() or \
                eng.requested_kind != getattr(self, "split_kind", SPLIT_KIND_DEFAULT):
            tensors = {k: v for k, v in self.state_dict(keep_vars=True).items() if v.dtype == torch.float32}
            dev = tensors["project.weight"].device
            if dev.type != "cuda":
                raise _L.HipExtensionError(
                    "model parameters are on %s: the faceformer_amd decode path runs only on a ROCm "
                    "device through libfaceformer_hip.so (no CPU fallback). Move the model with "
                    ".cuda()." % dev)
            eng = PathEngine(tensors, self.num_head, self.num_token, self.encoder.norm.eps,
                             bf16_split_planes=self.x3_min_rows > 0, fold_layernorm=True,
                             ln_in_epilogue=self._ln_in_epilogue(),
                             split_kind=getattr(self, "split_kind", SPLIT_KIND_DEFAULT))
            self._engine_obj = eng
        return eng

    def _encode(self, inputs, eng=None):
        """(engine, memory [N,S,E], mask_u8 [N,S], kv_len [N])"""
        inp, input_mask = inputs["input"], inputs["input_mask"]
        eng = self.engine() if eng is None else eng
        if not inp.is_cuda:
            raise _L.HipExtensionError("inputs['input'] is on %s; expected a ROCm device tensor" % inp.device)
        if input_mask.dtype in (torch.bool, torch.uint8) and input_mask.dim() == 2 and input_mask.is_cuda:
            mask, kv_len = eng.prepare_mask(input_mask)      # process_masks + key lengths in one launch
        else:
            mask, kv_len = self.process_masks(input_mask).to(torch.uint8).contiguous(), None
        memory, kv_len = eng.encode(inp.to(torch.float32).flatten(-2, -1), mask, kv_len)
        return eng, memory, mask, kv_len

    def _extra_mask(self, inputs):
        """Optional `inputs['extra_mask']` (bool, one row per decoded sequence, True = edge the pointer
        may not select, e.g. a co-edge adjacency rule; not a reference key): the never-masked
        special-token columns are prepended and the mask is OR-ed into the pointer's padding mask
        inside the kernel."""
        extra = inputs.get("extra_mask")
        if extra is None:
            return None
        pad = torch.zeros((extra.size(0), self.num_token), dtype=torch.bool, device=extra.device)
        return torch.cat([pad, extra.to(torch.bool)], dim=1).to(torch.uint8).contiguous()

    def _extract_faces_value(self, inputs, parallel):
        """extract_faces as None / "parse" / "enclosed", after its rules (ValueError, before anything is launched): a
        SurfaceFormer_Parallel option of the native engine; inputs["edge_map"], when given, is int32 N x L."""
        ef = getattr(self, "extract_faces", False)
        if ef is False or ef is None:
            return None
        if ef not in ("parse", "enclosed") or not isinstance(ef, str):
            raise ValueError("extract_faces=%r: must be False, 'parse' or 'enclosed'" % (ef,))
        if not parallel:
            raise ValueError("extract_faces is a SurfaceFormer_Parallel option (the single-sequence model's faces are split at SEP)")
        if not self.engine_supported():
            raise ValueError("extract_faces needs the native engine: this model's constructor arguments take the sub-module loop")
        em = inputs.get("edge_map")
        if em is not None:
            x = inputs["input"]
            if not torch.is_tensor(em) or em.dtype != torch.int32 or tuple(em.shape) != (x.size(0), x.size(1)):
                raise ValueError("edge_map must be an int32 tensor of shape [%d, %d]" % (x.size(0), x.size(1)))
        return ef

    def _sequence_faces_value(self, inputs, parallel):
        """sequence_faces as None / "parse" / "enclosed", after its rules (ValueError, before anything is launched): a SurfaceFormer
        option of the native engine; sequence_faces_slots = P in 1..max(T // 2, 1) with G * P slots per wireframe inside
        ff_face_votes' limit (G: the draws or beams of the call); inputs["edge_map"], when given, is int32 N x L."""
        sf = getattr(self, "sequence_faces", False)
        if sf is False or sf is None:
            return None
        if sf not in ("parse", "enclosed") or not isinstance(sf, str):
            raise ValueError("sequence_faces=%r: must be False, 'parse' or 'enclosed'" % (sf,))
        if parallel:
            raise ValueError("sequence_faces is a SurfaceFormer option (faces split at SEP); SurfaceFormer_Parallel extracts with extract_faces")
        if not self.engine_supported():
            raise ValueError("sequence_faces needs the native engine: this model's constructor arguments take the sub-module loop")
        T = self.num_labels
        if not 1 <= T <= _faces.FACE_SEQ_MAX_T:
            raise ValueError("sequence_faces takes label_seq_length in 1..%d (got %d)" % (_faces.FACE_SEQ_MAX_T, T))
        P = getattr(self, "sequence_faces_slots", None)
        if P is not None and (isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= max(T // 2, 1)):
            raise ValueError("sequence_faces_slots=%r: must be None or in 1..max(label_seq_length // 2, 1) = %d" % (P, max(T // 2, 1)))
        G = max(int(getattr(self, "sequence_samples", 0) or 0), int(getattr(self, "sequence_beams", 0) or 0),
                int(getattr(self, "sequence_constrain_samples", 0) or 0), int(getattr(self, "sequence_constrain_beams", 0) or 0), 1)
        if G * (max(T // 2, 1) if P is None else P) > _faces.FACE_MAX_ROWS:
            raise ValueError("sequence_faces: %d rows x %d slots per wireframe are above %d; lower sequence_faces_slots" % (
                G, max(T // 2, 1) if P is None else P, _faces.FACE_MAX_ROWS))
        em = inputs.get("edge_map")
        if em is not None:
            x = inputs["input"]
            if not torch.is_tensor(em) or em.dtype != torch.int32 or tuple(em.shape) != (x.size(0), x.size(1)):
                raise ValueError("edge_map must be an int32 tensor of shape [%d, %d]" % (x.size(0), x.size(1)))
        return sf

    def _follow_table(self, inputs, device, num_input, order):
        """The follow table [N, L, ceil(L/32)] int32 of a constrained decode in the DECODE's wireframe order: built on the device
        from the edges' end points (ops.follow_table with constrain_tol), or inputs["follow_table"] -- bool [N, L, L] or the
        packed words -- for the batch as given; then permuted like the wireframes when they are decoded sorted by edge count.
        num_input: a list of counts or an int32 tensor [N]."""
        x = inputs["input"]
        N, L = x.size(0), x.size(1)
        fw = (L + 31) // 32
        given = inputs.get("follow_table")
        if given is None:
            ni = num_input.to(device=device, dtype=torch.int32) if torch.is_tensor(num_input) else \
                torch.tensor(num_input, dtype=torch.int32).to(device)
            bits = ops.follow_table(x[:, :, 0, :2].to(device=device, dtype=torch.float32).contiguous(),
                                    x[:, :, -1, :2].to(device=device, dtype=torch.float32).contiguous(), ni, float(self.constrain_tol))
        else:
            if torch.is_tensor(given) and given.dtype == torch.int32 and tuple(given.shape) == (N, L, fw):
                bits = given.to(device)                          # packed words: taken as they are (no copy when on the device)
            else:
                g = _np.asarray(given.cpu().numpy() if torch.is_tensor(given) else given)
                if g.dtype == _np.bool_ and g.shape == (N, L, L):
                    g = _faces.pack_follow_bits(g)
                if g.dtype != _np.int32 or g.shape != (N, L, fw):
                    raise ValueError("follow_table must be bool [%d, %d, %d] or packed int32 [%d, %d, %d]" % (N, L, L, N, L, fw))
                bits = torch.as_tensor(g).to(device)
        if order is not None:
            bits = bits.index_select(0, torch.tensor(order, device=device))
        return bits.contiguous()

    def _sample_uniforms(self, inputs, device, T, N, F, R, order):
        """The uniforms [T-1, N*F*R] of a sampled decode in the DECODE's wireframe order: made (or given) for the batch as given,
        column (w*F + f)*R + k, then permuted like the wireframes when they are decoded sorted by edge count -- a draw belongs
        to the wireframe's place in the batch, not to its sorted place."""
        shape = (max(T - 1, 1), N * F * R)
        u = inputs.get("sample_uniforms")
        if u is None:
            gen = torch.Generator(device=device).manual_seed(int(self.sample_seed))
            u = torch.rand(shape, generator=gen, device=device, dtype=torch.float32)
        else:
            u = torch.as_tensor(u)
            if tuple(u.shape) != shape:
                raise ValueError("sample_uniforms must have shape [%d, %d]" % shape)
            u = u.to(device=device, dtype=torch.float32)
        if order is not None:
            u = u.view(shape[0], N, F * R).index_select(1, torch.tensor(order, device=device)).reshape(shape)
        return u.contiguous()

    def _decode_mode(self, inputs, parallel):
        """(record, value) of the mode this model's attributes select (hip/modes.py: the first of MODES switched on; value: beam
        width / number of samples / constraint flag bits, None for greedy), after the rules only the model can check: what the
        single-sequence model does not take; an opt-in mode needs the native engine and excludes what its record lists."""
        self._extract_faces_value(inputs, parallel)
        self._sequence_faces_value(inputs, parallel)
        for mode in _modes.SEQUENCE_MODES if parallel else ():
            if mode.switches[0].on(self):
                raise ValueError("%s is a SurfaceFormer option (%s); SurfaceFormer_Parallel %s per anchor with %s"
                                 % ((mode.subject, mode.sequence.model_has) + mode.sequence.parallel_has))
        if parallel and getattr(self, "sequence_constrain_samples", 0):      # (an option of sequence_constrain, refused above)
            mode = _modes.SEQUENCE_CONSTRAIN_SAMPLE
            raise ValueError("%s is a SurfaceFormer option (%s); SurfaceFormer_Parallel %s per anchor with %s"
                             % ((mode.subject, mode.sequence.model_has) + mode.sequence.parallel_has))
        if parallel and getattr(self, "sequence_constrain_beams", 0):        # (likewise)
            mode = _modes.SEQUENCE_CONSTRAIN_BEAM
            raise ValueError("%s is a SurfaceFormer option (%s); SurfaceFormer_Parallel %s per anchor with %s"
                             % ((mode.subject, mode.sequence.model_has) + mode.sequence.parallel_has))
        if parallel and getattr(self, "sequence_constrain_closure", None) is not None:      # (likewise)
            raise ValueError("sequence_constrain_closure is a SurfaceFormer option (the closure look-ahead of the loop rule of the "
                             "single-sequence model's row); SurfaceFormer_Parallel looks ahead per anchor with constrain_lookahead / "
                             "constrain_exact")
        if parallel and getattr(self, "sequence_constrain_beam_closure", None) is not None:      # (likewise)
            raise ValueError("sequence_constrain_beam_closure is a SurfaceFormer option (the closure look-ahead of the beam search "
                             "under the loop rule of the single-sequence model's row); SurfaceFormer_Parallel looks ahead per anchor "
                             "with constrain_beam_closure")
        CF = _modes.constrain_flags(getattr(self, "constrain", None))
        CB = _modes.constrain_beams_value(getattr(self, "constrain_beams", 0), CF if parallel else 0)     # (read next to constrain_tol: no Switch)
        look = getattr(self, "constrain_lookahead", False)      # (read next to constrain_tol as well)
        exact = getattr(self, "constrain_exact", False)         # (and this)
        CS = _modes.constrain_samples_value(getattr(self, "constrain_samples", 0), CF if parallel else 0, CB)     # (and this)
        closure = getattr(self, "constrain_beam_closure", None)      # (and this)
        if not parallel:
            if closure is not None:
                _modes.constrain_beam_closure_value(closure, _modes.CONSTRAIN_MODES["loops"], 1)      # (the value alone)
                raise ValueError("constrain_beam_closure is a SurfaceFormer_Parallel option (%s)" % _modes.SWITCH["constrain"].seq2seq)
            if CS:
                raise ValueError("constrain_samples is a SurfaceFormer_Parallel option (%s)" % _modes.SWITCH["constrain"].seq2seq)
            if CB:
                raise ValueError("constrain_beams is a SurfaceFormer_Parallel option (%s)" % _modes.SWITCH["constrain"].seq2seq)
            if look:
                raise ValueError("constrain_lookahead is a SurfaceFormer_Parallel option (%s)" % _modes.SWITCH["constrain"].seq2seq)
            if exact:
                raise ValueError("constrain_exact is a SurfaceFormer_Parallel option (%s)" % _modes.SWITCH["constrain"].seq2seq)
            for mode in reversed(_modes.MODES):
                for sw in mode.switches:
                    if sw.seq2seq and sw.on(self):
                        raise ValueError("%s is a SurfaceFormer_Parallel option (%s)" % (sw.attr, sw.seq2seq))
            return (_modes.GREEDY_LOGPROB if getattr(self, "return_logprob", False) else _modes.GREEDY), None
        LA = _modes.constrain_lookahead_value(look, CF, CB)
        EX = _modes.constrain_exact_value(exact, CF, CB, LA)
        if EX and not self.engine_supported():
            raise ValueError("constrain_exact needs the native engine: this model's constructor arguments take the sub-module loop")
        CL = _modes.constrain_beam_closure_value(closure, CF, CB, LA, EX, CS)
        if CL and not self.engine_supported():
            raise ValueError("constrain_beam_closure needs the native engine: this model's constructor arguments take the sub-module loop")
        mode, value = _modes.of_options(getattr(self, "return_logprob", False), CB, LA, EX, CS, CL, constrain=CF,
                                        num_samples=int(getattr(self, "num_samples", 0) or 0), beam_width=int(getattr(self, "beam_width", 0) or 0))
        if value is not None:
            attr = mode.switches[0].attr
            if not self.engine_supported():
                raise ValueError("%s needs the native engine: this model's constructor arguments take the sub-module loop" % attr)
            if any(inputs.get("extra_mask") is not None if word == "an extra mask" else _modes.SWITCH[word].on(self)
                   for word in mode.model_excludes):
                raise ValueError("%s excludes %s and %s" % (attr, ", ".join(mode.model_excludes[:-1]), mode.model_excludes[-1]))
            if mode.model_checked:
                _modes.check_options(mode, _L.FF_PARALLEL, dict(num_samples=value, temperature=self.sample_temperature,
                                                               top_k=self.sample_top_k, top_p=self.sample_top_p),
                                     (int(self.token.face_type_offset), int(self.token.len)))
            if mode is _modes.CONSTRAIN_BEAM:
                _modes.check_options(mode, _L.FF_PARALLEL, dict(constrain=CF, constrain_beams=value, follow_table=True,
                                                               S=inputs["input"].size(1) + self.num_token),
                                     (int(self.token.face_type_offset), int(self.token.len)))
            if mode is _modes.CONSTRAIN_BEAM_AHEAD:      # (the tables are made behind the encoder: the width and T are checked here)
                _modes.check_options(mode, _L.FF_PARALLEL, dict(constrain=CF, constrain_beams=value, constrain_beam_closure=CL,
                                                               follow_table=True, close_dist=True, cycle_len=True,
                                                               S=inputs["input"].size(1) + self.num_token, T=self.max_face_length),
                                     (int(self.token.face_type_offset), int(self.token.len)))
            if mode is _modes.CONSTRAIN_SAMPLE:     # (the operands are made behind the encoder: the values and T are checked here)
                _modes.check_options(mode, _L.FF_PARALLEL, dict(constrain=CF, constrain_samples=value, follow_table=True, close_dist=True,
                                                               cycle_len=True, constrain_lookahead=LA, constrain_exact=EX,
                                                               temperature=self.sample_temperature, top_k=self.sample_top_k,
                                                               top_p=self.sample_top_p, T=self.max_face_length),
                                     (int(self.token.face_type_offset), int(self.token.len)))
            if mode is _modes.CONSTRAIN_AHEAD:      # (the tables are made behind the encoder: only T is checked here)
                _modes.check_options(mode, _L.FF_PARALLEL, dict(constrain=CF, follow_table=True, close_dist=True, cycle_len=True,
                                                               T=self.max_face_length),
                                     (int(self.token.face_type_offset), int(self.token.len)))
            if mode is _modes.CONSTRAIN_EXACT:      # (the table is made behind the encoder: only T is checked here)
                _modes.check_options(mode, _L.FF_PARALLEL, dict(constrain=CF, follow_table=True, cycle_len=True, T=self.max_face_length),
                                     (int(self.token.face_type_offset), int(self.token.len)))
            if mode is _modes.CONSTRAIN_SAMPLE and inputs.get("sample_uniforms") is not None:      # (made behind the encoder otherwise)
                ni = inputs["num_input"]
                ni = [int(n) for n in (ni.tolist() if torch.is_tensor(ni) else ni)]
                shape = (max(self.max_face_length - 1, 1), len(ni) * max(ni) * value)
                if tuple(torch.as_tensor(inputs["sample_uniforms"]).shape) != shape:
                    raise ValueError("sample_uniforms must have shape [%d, %d]" % shape)
            if mode is _modes.CONSTRAIN_BEAM_AHEAD and CL == "exact":
                L = inputs["input"].size(1)
                if L + self.num_token > _modes.EXACT_MAX_KEYS:
                    raise ValueError("constrain_beam_closure='exact' takes at most %d edges per wireframe (got %d): L + num_token <= %d keys"
                                     % (_modes.EXACT_MAX_KEYS - self.num_token, L, _modes.EXACT_MAX_KEYS))
                given = inputs.get("cycle_len")
                shape = tuple(inputs["input"].shape[:2])
                if given is not None and (torch.as_tensor(given).dtype != torch.uint8 or tuple(torch.as_tensor(given).shape) != shape):
                    raise ValueError("cycle_len must be uint8 [%d, %d]" % shape)
            if mode is _modes.CONSTRAIN_EXACT or (mode is _modes.CONSTRAIN_SAMPLE and EX):
                L = inputs["input"].size(1)
                if L + self.num_token > _modes.EXACT_MAX_KEYS:
                    raise ValueError("constrain_exact takes at most %d edges per wireframe (got %d): L + num_token <= %d keys"
                                     % (_modes.EXACT_MAX_KEYS - self.num_token, L, _modes.EXACT_MAX_KEYS))
                given = inputs.get("cycle_len")
                shape = tuple(inputs["input"].shape[:2])
                if given is not None and (torch.as_tensor(given).dtype != torch.uint8 or tuple(torch.as_tensor(given).shape) != shape):
                    raise ValueError("cycle_len must be uint8 [%d, %d]" % shape)
        return mode, value

    def _score(self, inputs, variant, T, F, paths, lengths):
        """Teacher-forced scoring of `paths` (PathEngine.score) with this model's decode options; adds the score_*
        keys to `inputs`.  The wireframes are scored in batch order: a forced decode has no padding-anchor de-duplication, so
        every wireframe is F rows wide whatever its edge count -- the micro-batches forward_eval gets by sorting are the ones
        this plan has already -- and there is no sort_by_edges permutation to undo.  stop_each_eos (seq2seq) is a rule of the
        greedy decode and is not looked at: a forced decode has no stop rule."""
        for mode in tuple(reversed(_modes.MODES)) + _modes.SEQUENCE_MODES:
            for sw in mode.switches:
                if not sw.scored and sw.on(self):
                    raise ValueError("score() excludes %s: set model.%s = %r to score given paths" % (sw.attr, sw.attr, sw.off))
        if getattr(self, "constrain_samples", 0):     # (an option of constrain: without constrain the lines above have not raised)
            raise ValueError("score() excludes constrain_samples: set model.constrain_samples = 0 to score given paths")
        if getattr(self, "sequence_constrain_samples", 0):     # (likewise an option of sequence_constrain)
            raise ValueError("score() excludes sequence_constrain_samples: set model.sequence_constrain_samples = 0 to score given paths")
        if getattr(self, "sequence_constrain_beams", 0):
            raise ValueError("score() excludes sequence_constrain_beams: set model.sequence_constrain_beams = 0 to score given paths")
        if getattr(self, "sequence_constrain_closure", None) is not None:
            raise ValueError("score() excludes sequence_constrain_closure: set model.sequence_constrain_closure = None to score given "
                             "paths")
        if getattr(self, "sequence_constrain_beam_closure", None) is not None:
            raise ValueError("score() excludes sequence_constrain_beam_closure: set model.sequence_constrain_beam_closure = None to "
                             "score given paths")
        if not self.engine_supported():
            raise ValueError("score() needs the native engine: this model's constructor arguments take the sub-module loop")
        eng, memory, mask, kv_len = self._encode(inputs)
        out = eng.score(memory, mask, kv_len, variant, T, paths.to(memory.device), lengths, F=F,
                        chunk_wireframes=self.chunk_wireframes, chunk_seqs=self.chunk_seqs, chunk_max_seqs=self.chunk_max_seqs,
                        num_streams=self.num_streams, flags=self.decode_flags, x3_min_rows=self.x3_min_rows,
                        ln_fuse_max_rows=self.ln_fuse_max_rows,
                        retire=bool(getattr(self, "retire_finished", False)), beam_width=int(getattr(self, "beam_width", 0) or 0),
                        logprob=bool(getattr(self, "return_logprob", False)), extra_mask=inputs.get("extra_mask"))
        N = memory.size(0)
        shape = (N, F, T) if variant == _L.FF_PARALLEL else (N, T)
        for key, dims, _ in _modes.FORCED.outs:
            inputs["score_" + key] = out[key].view(shape if dims else shape[:-1])
        self.last_score_stats = {"rows": out["logprob"].size(0), "steps": out["steps"]}
        return inputs

    def forward(self, inputs):
        if self.training:
            return self.forward_train(inputs)
        return self.forward_eval(inputs)


__all__ = ["SurfaceFormerBase", "min_value_of_dtype"]
