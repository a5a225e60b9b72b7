"""Host side of the whole-path engine: binds a model's parameters (by reference, no repacking) into
the C `ff_model` struct and runs ff_encode / ff_decode on torch-owned device memory."""
import ctypes as C

import torch

from . import lib as _L
from . import modes as _modes
from .modes import CONSTRAIN_MODES, SAMPLE_MAX, constrain_flags  # noqa: F401  (importers find them here)
from .ops import SPLIT_KINDS, _dev, _p, _stream, split_weight

import operator

_VERSION_OF = operator.attrgetter("_version")

RETIRE_MIN_SHRINK = 0.125   # retire=True: a check point compacts a micro-batch that loses at least this fraction of its slots

DEFAULT_FLAGS = (_L.FF_REUSE_LAYER0_QKV | _L.FF_LAST_LAYER_LAST_ROW | _L.FF_DEDUP_PAD_ANCHORS
                 | _L.FF_FUSE_LAYERNORM)


def _kv_len_from_mask(mask_u8):
    """1 + index of the last unmasked key per row (0 if every key is masked)."""
    S = mask_u8.size(1)
    idx = torch.arange(1, S + 1, device=mask_u8.device, dtype=torch.int32)
    return ((mask_u8 == 0).to(torch.int32) * idx).amax(dim=1).to(torch.int32).contiguous()


FP16_LIM = 6.0e4     # bound every operand of the "2 x fp16" products must stay below (fp16's largest finite value is 65504)
ATTN_Q_SCALE = 0.125 * 1.4426950408889634   # the 2 x fp16 attention kernel splits q * scale * log2(e) (ff_attention_x2h.hip)


def fp16_operand_bounds(tensors, n_dec, E, weights=0.0):
    """A-priori bounds of every operand the split-kind "fp16x2" decode feeds to fp16 terms, by operand class (CPU or GPU tensors).

    A LayerNorm output is y = gamma * n + beta with ||n||_2 <= sqrt(E), so a projection of it is bounded row by row:
        |(y + t) . W_n + b_n| <= sqrt(E) ||W_n * gamma||_2 + max over t |W_n . (beta + t) + b_n|      (Cauchy-Schwarz)
    for t ranging over the rows of a position table added to y (or t = 0).  The classes:
      weights                  max |w| of the planes (`weights`: the caller's; raw and LayerNorm-folded weights)
      LayerNorm outputs        y of the un-folded steps (into linear1 and the self-attention v rows): max |gamma| sqrt(E) + max |beta|
      LayerNorm + query pos    yq = y + qpos of the un-folded steps (into the self-attention q|k rows and the cross-attention q)
      self-attention values    v = LN1(x) Wv^T + bv: the attention output is a convex mixture of v rows (into the self out-projection)
      feed-forward hidden      relu(LN3(x) W1^T + b1) (into linear2)
      cross-attention values   v = memory Wv^T + bv, memory = the encoder's final LayerNorm (the K|V planes; into the cross out-projection)
      cross-attention keys     k = (memory + pos) Wk^T + bk (the K|V planes)
      cross-attention queries  q = (LN2(x) + qpos) Wq^T + bq, times 0.125 log2(e): the kernel splits the scaled q
    Returns {class: bound}.  The LayerNorm-folded weights are W * gamma / W . beta + b: the same bounds (up to rounding).  The
    folded steps' normalise-first form multiplies n itself (|n_i| <= sqrt(E)); their epilogue form feeds the raw residual rows at
    2^-6 (exact; 4.2e6 before fp16's range) -- the residual stream has no a-priori bound and is not one of these classes."""
    root = float(E) ** 0.5

    def bound(W, gamma, beta, b, table=None):
        W, gamma, beta, b = (t.detach().double() for t in (W, gamma, beta, b))
        off = W @ beta + b                                                  # [N]
        if table is not None:
            off = (off[:, None] + W @ table.detach().double().t()).abs().amax(dim=1)
        return float(((W * gamma).norm(dim=1) * root + off.abs()).max())

    def ln_bound(gamma, beta, table=None):
        gamma, beta = gamma.detach().double(), beta.detach().double()
        shift = beta.abs() if table is None else (beta[None, :] + table.detach().double()).abs().amax(dim=0)
        return float((gamma.abs() * root + shift).max())

    worst = {"weights": float(weights)}

    def put(name, v):
        worst[name] = max(worst.get(name, 0.0), v)
    ge, be = tensors["encoder.norm.weight"], tensors["encoder.norm.bias"]
    pos, qpos = tensors["pos_enc.pos_embed.weight"], tensors["query_pos_enc.pos_embed.weight"]
    for i in range(n_dec):
        p = "decoder.layers.%d." % i
        g1, b1 = tensors[p + "norm1.weight"], tensors[p + "norm1.bias"]
        g2, b2 = tensors[p + "norm2.weight"], tensors[p + "norm2.bias"]
        g3, b3 = tensors[p + "norm3.weight"], tensors[p + "norm3.bias"]
        Ws, bs = tensors[p + "self_attn.in_proj_weight"], tensors[p + "self_attn.in_proj_bias"]
        Wc, bc = tensors[p + "multihead_attn.in_proj_weight"], tensors[p + "multihead_attn.in_proj_bias"]
        for g_, b_ in ((g1, b1), (g2, b2), (g3, b3)):
            put("LayerNorm outputs", ln_bound(g_, b_))
        for g_, b_ in ((g1, b1), (g2, b2)):
            put("LayerNorm + query pos", ln_bound(g_, b_, qpos))
        put("self-attention values", bound(Ws[2 * E:], g1, b1, bs[2 * E:]))
        put("feed-forward hidden", bound(tensors[p + "linear1.weight"], g3, b3, tensors[p + "linear1.bias"]))
        put("cross-attention values", bound(Wc[2 * E:], ge, be, bc[2 * E:]))
        put("cross-attention keys", bound(Wc[E:2 * E], ge, be, bc[E:2 * E], pos))
        put("cross-attention queries", ATTN_Q_SCALE * bound(Wc[:E], g2, b2, bc[:E], qpos))
    return worst


# The per-mode checks as functions: calls into the table, which reads the options by decode()'s names -- these parameters' names.
def check_beam_options(width, S, variant, retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, term_range):
    """The combinations a beam decode rejects (ff_decode_beam's FF_ERR_ARG list), as ValueError before anything is launched."""
    _modes.check_options(_modes.BEAM, variant, dict(locals(), beam_width=width), term_range)


def check_sample_options(num_samples, temperature, top_k, top_p, variant, retire, return_pointer, no_stop, stop_callback, extra_mask,
                         logprob, beam_width, term_range):
    """The combinations a sampled decode rejects (ff_decode_sample's FF_ERR_ARG list, and the options of decode() it cannot be
    combined with), as ValueError before anything is launched."""
    _modes.check_options(_modes.SAMPLE, variant, locals(), term_range)


def check_constrain_options(flags, variant, retire, return_pointer, no_stop, stop_callback, extra_mask, logprob, beam_width,
                            num_samples, term_range, follow_table, constrain_beams=0, S=None):
    """The combinations a constrained decode rejects (ff_decode_constrained's FF_ERR_ARG list, and the options of decode() it
    cannot be combined with), as ValueError before anything is launched.  constrain_beams = W > 0 (with S, the keys per row):
    those of the beam search over the constrained keys (ff_decode_constrained_beam)."""
    W = _modes.constrain_beams_value(constrain_beams, flags)
    if W:      # (S not given: the width is held to 1..8 alone)
        return _modes.check_options(_modes.CONSTRAIN_BEAM, variant, dict(locals(), constrain=flags, constrain_beams=W,
                                                                         S=8 if S is None else S), term_range)
    _modes.check_options(_modes.CONSTRAIN, variant, dict(locals(), constrain=flags), term_range)


def check_forced_options(paths, lengths, rows, T, S, retire=False, beam_width=None, logprob=False, return_pointer=False,
                         stop_callback=None, stop_each_eos=False, extra_mask=None):
    """What a forced decode rejects (ff_decode_forced's FF_ERR_ARG list, and the options of decode() it has no argument for), as
    ValueError before anything is launched; and the one pass over the paths.  Returns (paths int64 [rows, T], lengths as a list)."""
    return _modes.check_options(_modes.FORCED, None, locals(), None)


class PathEngine:
    """Encoder + greedy pointer decode of one model instance on one ROCm device.

    `tensors` is a mapping name -> fp32 CUDA tensor with the reference state_dict names
    (SURVEY.md Appendix B).  Tensors are referenced, not copied: in-place weight updates are seen.
    """

    def __init__(self, tensors, num_head, num_token=4, ln_eps=1e-5, bf16_split_planes=False, fold_layernorm=True,
                 ln_in_epilogue=True, split_kind="bf16x3"):
        self._lib = _L.load()
        if split_kind not in SPLIT_KINDS:
            raise ValueError("split_kind must be one of %s" % sorted(SPLIT_KINDS))
        self.split_kind = split_kind
        self._keep = {}
        self._bound_at = {}
        self._planes = {}
        self._want_planes = bool(bf16_split_planes)
        self.ln_in_epilogue = bool(ln_in_epilogue)
        self._folded = {}
        m = _L.Model()
        get = self._get
        self.tensors = tensors
        E = tensors["project.weight"].shape[0]
        m.E, m.H = E, num_head
        m.FF = tensors["decoder.layers.0.linear1.weight"].shape[0]
        n_enc = 1 + max([int(k.split(".")[2]) for k in tensors if k.startswith("encoder.layers.")] or [-1])
        n_dec = 1 + max(int(k.split(".")[2]) for k in tensors if k.startswith("decoder.layers."))
        if n_enc > _L.FF_MAX_LAYERS or n_dec > _L.FF_MAX_LAYERS:
            raise ValueError("at most %d layers are supported" % _L.FF_MAX_LAYERS)
        if E != num_head * _L.FF_HEAD_DIM:
            raise _L.HipExtensionError(
                "the HIP attention kernels need num_model == num_head * 64 (got %d, %d)" % (E, num_head))
        m.num_enc_layers, m.num_dec_layers = n_enc, n_dec
        m.in_dim = tensors["val_enc.embedding_value.0.weight"].shape[1]
        m.num_token = num_token
        m.pos_len = tensors["pos_enc.pos_embed.weight"].shape[0]
        m.qpos_len = tensors["query_pos_enc.pos_embed.weight"].shape[0]
        m.ln_eps = ln_eps
        m.tok_embed = get("val_enc.embedding_token.weight")
        m.emb_w1, m.emb_b1 = get("val_enc.embedding_value.0.weight"), get("val_enc.embedding_value.0.bias")
        m.emb_w2, m.emb_b2 = get("val_enc.embedding_value.2.weight"), get("val_enc.embedding_value.2.bias")
        m.pos_table, m.qpos_table = get("pos_enc.pos_embed.weight"), get("query_pos_enc.pos_embed.weight")

        def mha(dst, p):
            dst.in_proj_w, dst.in_proj_b = get(p + ".in_proj_weight"), get(p + ".in_proj_bias")
            dst.out_w, dst.out_b = get(p + ".out_proj.weight"), get(p + ".out_proj.bias")

        def layer(dst, p, decoder):
            mha(dst.self_attn, p + ".self_attn")
            if decoder:
                mha(dst.cross_attn, p + ".multihead_attn")
            dst.lin1_w, dst.lin1_b = get(p + ".linear1.weight"), get(p + ".linear1.bias")
            dst.lin2_w, dst.lin2_b = get(p + ".linear2.weight"), get(p + ".linear2.bias")
            dst.norm1_w, dst.norm1_b = get(p + ".norm1.weight"), get(p + ".norm1.bias")
            dst.norm2_w, dst.norm2_b = get(p + ".norm2.weight"), get(p + ".norm2.bias")
            if decoder:
                dst.norm3_w, dst.norm3_b = get(p + ".norm3.weight"), get(p + ".norm3.bias")

        for i in range(n_enc):
            layer(m.enc[i], "encoder.layers.%d" % i, False)
        m.enc_norm_w, m.enc_norm_b = get("encoder.norm.weight"), get("encoder.norm.bias")
        for i in range(n_dec):
            layer(m.dec[i], "decoder.layers.%d" % i, True)
        m.dec_norm_w, m.dec_norm_b = get("decoder.norm.weight"), get("decoder.norm.bias")
        m.proj_w, m.proj_b = get("project.weight"), get("project.bias")
        if fold_layernorm and E % 64 == 0 and E >= 128 and m.FF % 64 == 0 and m.FF >= 128:
            # FF_FUSE_LAYERNORM: gamma / beta of every decoder LayerNorm and the query-position table are folded
            # ONCE into the projection that consumes them (derived copies: re-made when a weight is updated in place)
            dev = tensors["project.weight"].device
            qpos = tensors["query_pos_enc.pos_embed.weight"]
            with torch.cuda.device(dev):
                for i in range(n_dec):
                    p = "decoder.layers.%d." % i
                    lw = m.dec[i]
                    lw.ln1_w, lw.ln1_b, lw.ln1_pos = self._fold(
                        (i, 1), tensors[p + "self_attn.in_proj_weight"], tensors[p + "self_attn.in_proj_bias"],
                        tensors[p + "norm1.weight"], tensors[p + "norm1.bias"], qpos, 2 * E)
                    lw.ln2_w, lw.ln2_b, lw.ln2_pos = self._fold(
                        (i, 2), tensors[p + "multihead_attn.in_proj_weight"][:E], tensors[p + "multihead_attn.in_proj_bias"][:E],
                        tensors[p + "norm2.weight"], tensors[p + "norm2.bias"], qpos, E)
                    lw.ln3_w, lw.ln3_b, _ = self._fold(
                        (i, 3), tensors[p + "linear1.weight"], tensors[p + "linear1.bias"],
                        tensors[p + "norm3.weight"], tensors[p + "norm3.bias"], None, 0)
                m.proj_fold_w, m.proj_fold_b, _ = self._fold(
                    ("proj",), tensors["project.weight"], tensors["project.bias"],
                    tensors["decoder.norm.weight"], tensors["decoder.norm.bias"], None, 0)
        # Split planes (x3_min_rows > 0): of the raw weights (steps that launch their LayerNorms) and of the LayerNorm-folded ones.
        # A model whose operand bounds (fp16_operand_bounds: every operand class, folded or not) leave fp16's range gets the bf16
        # terms instead of the fp16 ones (with a warning): the range of bf16 is fp32's.  `requested_kind` is what the caller asked
        # for, `split_kind` what was bound.
        self.requested_kind = split_kind
        if bf16_split_planes:
            self._make_planes(m, tensors, n_dec, E, split_kind, ln_in_epilogue)
            if split_kind in ("fp16x2", "fp16"):   # (both kinds feed the same operand classes to fp16 terms: the same bounds)
                bad = self._check_fp16_range(tensors, n_dec, E)
                if bad:
                    import warnings
                    warnings.warn("faceformer_amd: split_kind=%r needs every operand of the split products inside fp16's range; "
                                  "this model's bounds are not (%s) -- binding the bf16x3 planes instead" % (split_kind, bad))
                    self.split_kind = "bf16x3"
                    self._planes = {}
                    self._make_planes(m, tensors, n_dec, E, "bf16x3", ln_in_epilogue)
        m.split_kind = SPLIT_KINDS[self.split_kind] if self._planes else 0
        self.model = m
        self.E, self.H, self.num_token = E, num_head, num_token
        self.device = tensors["project.weight"].device
        self._ws = None
        # address and in-place version of every bound tensor AS CAPTURED WHEN IT WAS BOUND (_get): a parameter moved or updated
        # between that moment and the first forward is then seen as stale by pointers_current(), not recorded as current
        self._versions = {k: self._bound_at[k][1] for k in self._keep} if (self._planes or self._folded) else {}
        self._fast_check = ([self.tensors[k] for k in self._keep], tuple(self._bound_at[k][0] for k in self._keep),
                            [self.tensors[k] for k in self._versions], tuple(self._versions.values()))
        # the stream-K exchange buffer of the launch stream is allocated here, not inside the first decode
        with torch.cuda.device(self.device):
            _L.check(self._lib.ff_gemm_prepare_stream(_stream()), "ff_gemm_prepare_stream")

    def _make_planes(self, m, tensors, n_dec, E, kind, ln_in_epilogue):
        """Split planes of the decoder projections: three exact bf16 planes per weight (+1.5x their bytes), two fp16 planes
        (+1x) or one fp16 plane (kind "fp16", +0.5x), split once here -- ff_decode then runs the large steps' projections on the 16-bit matrix cores (x3_min_rows);
        re-bound after in-place weight updates (pointers_current)."""
        for i in range(n_dec):
            for field, name in (("in_proj_planes", "self_attn.in_proj_weight"), ("lin1_planes", "linear1.weight"),
                                ("lin2_planes", "linear2.weight"), ("self_out_planes", "self_attn.out_proj.weight"),
                                ("cross_q_planes", "multihead_attn.in_proj_weight"),
                                ("cross_out_planes", "multihead_attn.out_proj.weight")):
                wt = tensors["decoder.layers.%d.%s" % (i, name)]
                if field == "cross_q_planes":
                    wt = wt[:E]       # q rows only: k|v of the cross attention are projected once per batch
                if wt.shape[1] % 32 or wt.shape[1] < 64:
                    setattr(m.dec[i], field, None)
                    continue          # the split kernel needs K % 32 == 0: this weight stays f32-only (null planes)
                pl = split_weight(wt, kind)
                self._planes[(i, field)] = pl
                setattr(m.dec[i], field, pl.data_ptr())
            if E % 32 == 0:
                # planes of the FOLDED weights: the steps that take the split projections keep the LayerNorm folding
                # (ff_gemm_x3_ln / ff_gemm_x2h_ln) instead of launching their LayerNorms
                for field, cfield, key in (("ln1_planes", "ln1_csum", (i, 1)), ("ln2_planes", "ln2_csum", (i, 2)),
                                           ("ln3_planes", "ln3_csum", (i, 3))):
                    if key not in self._folded:
                        continue
                    pl = split_weight(self._folded[key][0], kind)
                    self._planes[(i, field)] = pl
                    setattr(m.dec[i], field, pl.data_ptr())
                    if ln_in_epilogue:
                        # row sums of the folded weight (fp64 sum, rounded once): LN(x) W'^T = rstd (x W'^T - mean s)
                        cs = self._folded[key][0].double().sum(dim=1).float().contiguous()
                        self._planes[(i, cfield)] = cs
                        setattr(m.dec[i], cfield, cs.data_ptr())

    def _check_fp16_range(self, tensors, n_dec, E):
        """fp16 has five exponent bits: every operand of a "2 x fp16" product must stay below FP16_LIM in magnitude
        (fp16_operand_bounds).  A model whose bounds do not fit gets the bf16 terms instead (the caller warns).  Returns "" or the
        offending bounds."""
        weights = max(float(t.float().abs().max()) for (_i, f), t in self._planes.items() if t.dim() == 4)
        worst = fp16_operand_bounds(tensors, n_dec, E, weights)
        self.fp16_operand_bounds = worst
        bad = {k: v for k, v in worst.items() if not v < FP16_LIM}
        return ", ".join("%s <= %.3g" % kv for kv in sorted(bad.items()))

    def _fold(self, key, W, bias, gamma, beta, pos, pos_cols):
        """(Wf, bf, P) device pointers of ff_fold_layernorm_linear for one LayerNorm -> Linear pair."""
        N, K = W.shape
        Wf = torch.empty((N, K), device=W.device, dtype=torch.float32)
        bf = torch.empty((N,), device=W.device, dtype=torch.float32)
        P = torch.empty((pos.shape[0], pos_cols), device=W.device, dtype=torch.float32) if pos is not None else None
        _L.check(self._lib.ff_fold_layernorm_linear(
            _p(W), W.stride(0), N, K, _p(bias), _p(gamma), _p(beta), _p(pos), pos.stride(0) if pos is not None else 0,
            pos.shape[0] if pos is not None else 0, pos_cols, _p(Wf), _p(bf), _p(P), _stream()),
            "ff_fold_layernorm_linear")
        self._folded[key] = (Wf, bf, P)
        return Wf.data_ptr(), bf.data_ptr(), (P.data_ptr() if P is not None else None)

    def _get(self, name):
        t = self.tensors[name]
        _dev(t, name)
        if not t.is_contiguous():
            raise ValueError("parameter %s must be contiguous" % name)
        if t.data_ptr() % 16:
            raise ValueError("parameter %s is not 16-byte aligned" % name)
        self._keep[name] = t
        self._bound_at[name] = (t.data_ptr(), t._version)      # what the struct / the derived copies were made from
        return t.data_ptr()

    def pointers_current(self):
        """True while every bound tensor still lives at the address captured in the struct -- and, when
        derived copies of the weights exist (the bf16 planes), while no bound tensor was updated in place
        since they were made (load_state_dict / optimizer.step bump `_version`).  Runs in front of EVERY forward:
        two C-level passes over the ~200 tensors (33 us; the dict / generator form took 60 us of a 58.6 ms call)."""
        kt, ptrs, vt, vers = self._fast_check
        return tuple(map(torch.Tensor.data_ptr, kt)) == ptrs and tuple(map(_VERSION_OF, vt)) == vers

    @property
    def has_planes(self):
        """True when the engine was bound WITH the bf16 planes (weights whose K the split kernel cannot take have none)."""
        return self._want_planes

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), device=self.device, dtype=torch.uint8)
        return self._ws

    # ---------------------------------------------------------------------------------------------
    def prepare_mask(self, input_mask):
        """input_mask [N, L] bool / uint8 (True = padding) -> (mask_u8 [N, S] with the never-masked special-token columns in
        front, kv_len [N] int32): process_masks + key lengths as ONE launch (ff_prepare_mask)."""
        if input_mask.dtype not in (torch.bool, torch.uint8) or input_mask.dim() != 2:
            raise ValueError("input_mask must be a 2-D bool / uint8 tensor")
        self._same_device(input_mask, "input_mask")
        m = input_mask.contiguous()
        N, L = m.shape
        S = L + self.num_token
        mask_u8 = torch.empty((N, S), device=self.device, dtype=torch.uint8)
        kv_len = torch.empty((N,), device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _L.check(self._lib.ff_prepare_mask(_p(m), N, L, self.num_token, _p(mask_u8), _p(kv_len), _stream()), "ff_prepare_mask")
        return mask_u8, kv_len

    def stage_num_input(self, num_input):
        """(host int array, device int32 tensor) of the per-wireframe edge counts for decode(): made BEFORE the encoder is
        enqueued -- the pageable host-to-device copy inside decode() waited for the encoder's kernels on the same stream and
        left the GPU idle until the host had caught up (~40 us per call)."""
        vals = [int(x) for x in num_input]
        return (C.c_int * len(vals))(*vals), torch.tensor(vals, dtype=torch.int32).to(self.device), vals

    def encode(self, inp, mask_u8, kv_len=None):
        """inp [N, L, in_dim] fp32, mask_u8 [N, S] uint8 (1 = padding) -> (memory [N,S,E], kv_len)."""
        _dev(inp, "input"), _dev(mask_u8, "mask", torch.uint8)
        N, L = inp.shape[0], inp.shape[1]
        S = L + self.num_token
        inp = inp.reshape(N, L, -1).contiguous()
        if inp.shape[2] != self.model.in_dim:
            raise ValueError("input has %d values per edge, model expects %d" % (inp.shape[2], self.model.in_dim))
        mask_u8 = mask_u8.contiguous()
        if kv_len is None:
            kv_len = _kv_len_from_mask(mask_u8)
        memory = torch.empty((N, S, self.E), device=self.device, dtype=torch.float32)
        self._same_device(inp, "input"), self._same_device(mask_u8, "mask")
        nbytes = self._lib.ff_encode_workspace_bytes(C.byref(self.model), N, L)
        ws = self._workspace(nbytes)
        with torch.cuda.device(self.device):   # the C side launches on the CURRENT device / stream
            _L.check(self._lib.ff_encode(C.byref(self.model), _p(inp), _p(mask_u8), _p(kv_len), N, L,
                                         _p(memory), _p(ws), ws.numel(), _stream()), "ff_encode")
        return memory, kv_len

    def _same_device(self, t, name):
        if t is not None and t.device != self.device:
            raise _L.HipExtensionError("%s is on %s but the engine's weights are on %s" % (name, t.device, self.device))

    def decode(self, memory, mask_u8, kv_len, variant, T, F=1, num_input=None, extra_mask=None,
               chunk_wireframes=0, chunk_seqs=0, num_streams=1, sync_every=4, flags=DEFAULT_FLAGS,
               tok_sos=1, tok_eos=3, x3_min_rows=0, chunk_max_seqs=0, ln_fuse_max_rows=0,
               trace=False, return_pointer=False, no_stop=False, stop_callback=None, staged_num_input=None,
               retire=False, term_range=None, retire_min_shrink=RETIRE_MIN_SHRINK, logprob=False, beam_width=None,
               num_samples=None, temperature=1.0, top_k=0, top_p=1.0, uniforms=None, constrain=None, follow_table=None,
               constrain_beams=None, constrain_lookahead=False, close_dist=None, cycle_len=None, constrain_exact=False,
               constrain_samples=None, constrain_beam_closure=None, sequence_samples=None, sequence_beams=None,
               sequence_beam_stop="all", sequence_constrain=None, tok_sep=None, sequence_constrain_samples=None,
               sequence_constrain_beams=None, sequence_constrain_closure=None, sequence_constrain_beam_closure=None):
        """Greedy decode. Returns dict(predict [N*F, T] int64, steps, decoded_seqs, [pointer], [trace
        tensors indexed like predict's rows], slots_per_step, slot_rows, [logprob]).  The opt-in modes below are parallel-variant
        options that need term_range; what each excludes is its record's list in modes.py (ValueError before anything is launched).

        logprob=True (ff_decode_lp): also `logprob` [N*F, T] fp32, laid out like predict -- column j >= 1 is
        log_softmax(masked logits of step j-1)[predict[:, j]], 0 in column 0 and wherever predict is zero padded.  Tokens, steps
        and traces are those of the call without it.

        retire=True (parallel variant, FF_RETIRE_FINISHED): a sequence is finished from the first position holding a token in
        term_range = (lo, hi); the stop rule looks at unfinished sequences only, `predict` is zero after min(finish position,
        stop step) -- faces.retired_view of the default decode -- and finished sequences leave their micro-batch at the check
        points.  slot_rows = sum over executed steps of (step + 1) * slots: the decoder rows the call computed.

        beam_width=W >= 1 (parallel variant, ff_decode_beam; None or 0: the greedy decode above): W beams per anchor.  Also
        `beams` [N*F*W, T] int64 (row (w*F + f)*W + k is beam k of anchor f, best first, zero after the beam's finish position
        and the stop step), `beam_scores` [N*F*W] fp32 (-inf: empty beam); `predict` is beam 0; with trace=True `logits` is
        [T-1, N*F*W, S] and `beam_parent` [T-1, N*F*W] int32, both in output-row order.  Excludes retire, return_pointer, no_stop,
        stop_callback, extra_mask and logprob.  beam_width=1 equals the retire=True decode.

        num_samples=R >= 1 (parallel variant, ff_decode_sample; None or 0: the greedy decode above): R independent
        draws per anchor under temperature / top_k / top_p, driven by `uniforms` [T-1, N*F*R] fp32 on the device (step t of
        output row r reads uniforms[t, r]).  Also `samples` [N*F*R, T] int64 (row (w*F + f)*R + k is sample k of anchor f, zero
        after the sample's finish position and the stop step), `sample_logprob` (same layout, fp32: the model's log-probability
        of every drawn token) and `sample_scores` [N*F*R] (their sums); `predict` is sample 0; with trace=True `logits` is
        [T-1, N*F*R, S] in output-row order.  Excludes those and beam_width.  temperature=0 equals the retire=True decode, R times.

        constrain="no_repeat" / "loops" (parallel variant, ff_decode_constrained; None: the greedy decode above; the
        flag bits 0..3 are taken too): the greedy decode over keys the enclosure filter can accept.  follow_table [N, L,
        ceil(L/32)] int32 on the device (ops.follow_table), required by "loops".  `predict` is the constrained decode (zero after
        the row's finish position and the stop step); also `logprob` [N*F, T] fp32 (under the renormalised distribution) and
        `dead_end` [N*F] int32; with trace=True `logits` [T-1, N*F, S] holds the constrained masked rows.  Excludes those, beam_width
        and num_samples.  Bits 0 equal the retire=True decode.

        constrain_beams=W in 1..8, W <= S (only with constrain; ff_decode_constrained_beam; None or 0: the
        constrained greedy decode above): the beam search over the constrained keys, W beams per anchor.  Also `beams`
        [N*F*W, T] int64 and `beam_scores` [N*F*W] fp32 as beam_width's, `beam_dead_end` [N*F*W] int32 (the beam ran into a dead
        end); `predict` is beam 0; with trace=True `logits` [T-1, N*F*W, S] (the constrained masked rows) and `beam_parent`.
        No `logprob` / `dead_end`.  W = 1 equals the constrained greedy decode.

        constrain_lookahead=True (only with constrain="loops", not with constrain_beams, T <= 256; ff_decode_constrained_ahead,
        DESIGN.md 22): the constrained decode also masks every edge from which the loop cannot close within T -- close_dist
        [N, L, L] / cycle_len [N, L] uint8 on the device (ops.follow_distance of follow_table), both required.  Outputs are
        constrain's; `dead_end` then also means "cannot close within T".  With both tables zero it equals the "loops" decode.

        constrain_exact=True (only with constrain="loops", not with constrain_lookahead -- it contains it -- nor constrain_beams,
        T <= 256, at most 2048 keys; ff_decode_constrained_exact): while a loop is open the constrained decode also
        masks every edge from which it cannot close within T through edges the row has not used (one search per open row and
        step); with it closed, every edge with cycle_len > the positions left.  cycle_len [N, L] uint8 on the device
        (ops.follow_distance) is required, close_dist is not read.  Outputs are constrain's; a dead end is then only possible
        right after the position that opened the loop.

        constrain_samples=R in 1..64 (only with constrain, not with constrain_beams; ff_decode_constrained_sample, DESIGN.md 26;
        None or 0: the constrained greedy decode above): R independent draws per anchor from the CONSTRAINED row under
        temperature / top_k / top_p, driven by `uniforms` [T-1, N*F*R] as num_samples' are; with constrain_lookahead or
        constrain_exact (and their tables) the row is that form's.  Also `samples` [N*F*R, T] int64, `sample_logprob` (same
        layout: the log-probability under the model renormalised over the keys the rule allows), `sample_scores` [N*F*R] and
        `sample_dead_end` [N*F*R] int32; `predict`, `logprob` and `dead_end` are draw 0; with trace=True `logits`
        [T-1, N*F*R, S] holds the constrained masked rows.  temperature=0 equals the constrained greedy decode of the same form,
        R times; flag bits 0 equal the num_samples decode.

        constrain_beam_closure="lookahead" / "exact" (only with constrain="loops" and constrain_beams=W, T <= 256;
        ff_decode_constrained_beam_ahead; None: the constrain_beams decode above): every beam's row is formed with
        the closure look-ahead (close_dist and cycle_len required) or the exact one (cycle_len required, at most 2048 keys, one
        search per open beam and step).  Outputs are constrain_beams'; `beam_dead_end` then also means "cannot close within T".
        W = 1 equals the constrain_lookahead / constrain_exact decode; "lookahead" with both tables zero equals the
        constrain_beams decode.

        sequence_samples=R in 1..64 (single-sequence variant only, ff_decode_sequence_sample; None or 0: the greedy
        decode above): R independent draws per WIREFRAME under temperature / top_k / top_p, all from tok_sos, off one encoding
        and one set of cross-attention K | V; `uniforms` [T-1, N*R] fp32 on the device (step t of output row r reads
        uniforms[t, r]).  A draw is finished by tok_eos alone; the decode stops after the first step that leaves no draw
        unfinished (`steps`; `step_counts`: the draws unfinished after every step).  Also `samples` [N*R, T] int64 (row w*R + k is
        draw k of wireframe w, zero behind its EOS and the stop step), `sample_logprob` (same layout) and `sample_scores` [N*R];
        `predict` [N, T] is draw 0; with trace=True `logits` is [T-1, N*R, S] in output-row order.  No term_range.  Excludes every
        other mode and option above, and stop_each_eos (the flag FF_STOP_EACH_EOS): the rule is per draw already.  temperature=0
        equals, R times, the greedy FF_STOP_EACH_EOS decode cut behind every row's first EOS.

        sequence_beams=W in 1..8, at most S (single-sequence variant only, ff_decode_sequence_beam; None or 0: the
        greedy decode above): beam search with W beams per WIREFRAME, all from tok_sos (beam 0 alone non-empty), off one encoding
        and one set of cross-attention K | V.  A beam is finished by tok_eos alone.  sequence_beam_stop="all": the decode stops
        after the first step that leaves no non-empty beam unfinished (`step_counts`: those beams after every step); "best": after
        the first step that leaves rank 0 of every wireframe finished (`step_counts`: the wireframes whose rank 0 is not) -- exact
        for beam 0, the other beams are returned as they stand.  Also `beams` [N*W, T] int64 (row w*W + k is beam k of wireframe
        w, best first, zero behind its EOS and the stop step), `beam_scores` [N*W] (-inf: an empty rank) and `beam_finished`
        [N*W] int32; `predict` [N, T] is beam 0; with trace=True `logits` [T-1, N*W, S] and `beam_parent` [T-1, N*W] in
        output-row order.  No term_range.  Excludes every other mode and option above, and stop_each_eos.  W=1 equals the greedy
        FF_STOP_EACH_EOS decode cut behind every row's first EOS.

        sequence_constrain="no_repeat" / "loops" / "coedge_loops" (single-sequence variant only, ff_decode_sequence_constrained,
        DESIGN.md 32; None: the greedy decode above; the flag bits 0..7 are taken too) with tok_sep: the greedy decode under the
        face-loop rule applied per face of the row.  SEP ends a face, tok_eos alone the row; a dead end re-opens SEP alone and the
        row goes on; "coedge_loops" also forbids a co-edge twice in the row.  follow_table [N, L, ceil(L/32)] int32 on the device,
        required by "loops" and "coedge_loops".  The decode stops after the first step that leaves no row unfinished
        (`step_counts`: the rows unfinished after every step).  `predict` [N, T] is zero behind the row's EOS and the stop step;
        also `logprob` [N, T] fp32 (under the renormalised distribution), `dead_end` [N, T] int32 (1 where the SEP was selected at
        a dead end) and `open_end` [N] int32 (a loop is open after the last kept position); with trace=True `logits` [T-1, N, S]
        holds the constrained masked rows.  No term_range.  Excludes every other mode and option above, and stop_each_eos.  Bits
        0 equal the greedy FF_STOP_EACH_EOS decode cut behind every row's first EOS, with logprob=True's log-probabilities.

        sequence_constrain_samples=R in 1..64 (only with sequence_constrain, not with sequence_samples or sequence_beams;
        ff_decode_sequence_constrained_sample; None or 0: the sequence_constrain decode above): R independent draws
        per WIREFRAME from the CONSTRAINED row under temperature / top_k / top_p, driven by `uniforms` [T-1, N*R] as
        sequence_samples' are; every draw carries its own state of the rule and is finished by its own EOS.  Also `samples`
        [N*R, T] int64 (row w*R + k is draw k of wireframe w), `sample_logprob` (same layout: the log-probability under the model
        renormalised over the keys the rule allows), `sample_scores` [N*R], `sample_dead_end` [N*R, T] int32 and `sample_open_end`
        [N*R] int32; `predict`, `logprob`, `dead_end` and `open_end` are draw 0; with trace=True `logits` [T-1, N*R, S] holds the
        constrained masked rows.  temperature=0 equals the sequence_constrain decode, R times; flag bits 0 equal the
        sequence_samples decode.

        sequence_constrain_beams=W in 1..8, at most S (only with sequence_constrain, not with sequence_samples, sequence_beams or
        sequence_constrain_samples; ff_decode_sequence_constrained_beam; None or 0: the sequence_constrain decode
        above): the W best rows per WIREFRAME among the rows the rule leaves, every beam carrying its own state of the rule through
        the parent permutation, scored by the model's distribution renormalised over the allowed keys; sequence_beam_stop "all" /
        "best" as sequence_beams'.  Also `beams` [N*W, T] int64 (row w*W + k is rank k of wireframe w, best first), `beam_scores`,
        `beam_finished` and `beam_open_end` [N*W], `beam_dead_end` [N*W, T] int32 (walked back along the tokens' parents);
        `predict`, `dead_end` and `open_end` are beam 0; no `logprob`; with trace=True `logits` [T-1, N*W, S] holds the constrained
        masked rows and `beam_parent` the parents.  W = 1 equals the sequence_constrain decode; flag bits 0 equal the
        sequence_beams decode wherever every wireframe has W live keys.

        sequence_constrain_closure="lookahead" / "exact" (only with sequence_constrain "loops" / "coedge_loops" or the flag bits 3 /
        7 -- "lookahead" also with CONNECT alone -- alone or with sequence_constrain_samples, not with sequence_constrain_beams;
        ff_sequence_decode_constrained_ahead / ff_sequence_decode_constrained_sample_ahead; None: the decodes above):
        the step that selects position p also masks every edge from which the current loop cannot close within budget =
        min(T - 1 - p, 254) further positions -- "lookahead" by close_dist [N, L, L] / cycle_len [N, L] uint8 on the device
        (ops.follow_distance of follow_table, both required), "exact" by one search per open row and step over the edges that are
        neither padded nor in the row's visited words (cycle_len required, at most 2048 keys).  T may exceed 256: the budget is
        clamped, so a loop of more than 254 edges counts as not closable.  Outputs are the plain decode's under the same keys;
        `open_end` is then 0 everywhere and `dead_end` also means "cannot close within the row".  "lookahead" with both tables
        zero equals the plain decode, bit for bit.

        sequence_constrain_beam_closure="lookahead" / "exact" (only with sequence_constrain_beams >= 1 and sequence_constrain "loops" /
        "coedge_loops" or the flag bits 3 / 7 -- "lookahead" also with CONNECT alone; not with sequence_constrain_closure, which stays
        refused with beams; ff_sequence_decode_constrained_beam_ahead; None: the beam decode above): every beam forms
        its byte row under sequence_constrain_closure's masks from its OWN (first, prev) and visited words, against its wireframe's
        close_dist [N, L, L] / cycle_len [N, L] uint8 on the device ("exact": cycle_len only, at most 2048 keys) and the step's one
        budget min(T - 1 - p, 254).  The search, the scores and the outputs are sequence_constrain_beams'; `beam_open_end` is then 0
        on every non-empty beam.  W = 1 equals the sequence_constrain_closure greedy decode; "lookahead" with both tables zero equals
        the plain beam decode, bit for bit."""
        SCB = _modes.sequence_constrain_beams_value(sequence_constrain_beams, _modes.sequence_constrain_flags(sequence_constrain),
                                                    sequence_samples, sequence_beams, sequence_constrain_samples) \
            if sequence_constrain_beams else 0
        SCS = _modes.sequence_constrain_samples_value(sequence_constrain_samples, _modes.sequence_constrain_flags(sequence_constrain),
                                                      sequence_samples, sequence_beams) if sequence_constrain_samples else 0
        SCC = _modes.sequence_constrain_closure_value(sequence_constrain_closure, _modes.sequence_constrain_flags(sequence_constrain),
                                                      sequence_constrain_beams) if sequence_constrain_closure is not None else None
        SCBC = _modes.sequence_constrain_beam_closure_value(
            sequence_constrain_beam_closure, _modes.sequence_constrain_flags(sequence_constrain), SCB, sequence_constrain_closure,
            sequence_constrain_samples) if sequence_constrain_beam_closure is not None else None
        seq = dict(sequence_samples=sequence_samples, sequence_beams=sequence_beams, sequence_constrain=sequence_constrain)
        for mode in reversed(_modes.SEQUENCE_MODES):      # (of several set together, the last one's record reports)
            value = mode.sequence.value(seq[mode.subject])
            if value != mode.switches[0].off:
                o = dict(seq, retire=retire, return_pointer=return_pointer, no_stop=no_stop, stop_callback=stop_callback,
                         extra_mask=extra_mask, logprob=logprob, beam_width=int(beam_width or 0), num_samples=int(num_samples or 0),
                         constrain=constrain is not None, temperature=temperature, top_k=top_k, top_p=top_p, uniforms=uniforms,
                         sequence_beam_stop=sequence_beam_stop, follow_table=follow_table, tok_sep=tok_sep, tok_eos=tok_eos,
                         trace=trace, N=memory.shape[0], S=memory.shape[1], F=F, T=T, sequence_constrain_closure=SCC,
                         sequence_constrain_beam_closure=SCBC, close_dist=close_dist, cycle_len=cycle_len)
                o[mode.subject] = value
                if SCC and mode is _modes.SEQUENCE_CONSTRAIN:      # (an option of sequence_constrain and of its sampled form)
                    mode = _modes.SEQUENCE_CONSTRAIN_AHEAD
                if SCS:      # (an option of sequence_constrain, the first record this loop looks at)
                    mode, o["sequence_constrain_samples"] = (_modes.SEQUENCE_CONSTRAIN_SAMPLE_AHEAD if SCC else
                                                             _modes.SEQUENCE_CONSTRAIN_SAMPLE), SCS
                if SCB:      # (likewise)
                    mode, o["sequence_constrain_beams"] = (_modes.SEQUENCE_CONSTRAIN_BEAM_AHEAD if SCBC else
                                                           _modes.SEQUENCE_CONSTRAIN_BEAM), SCB
                return self._decode_sequence(mode, memory, mask_u8, kv_len, variant, o,
                                             (variant, memory.shape[0], memory.shape[1], F, T, chunk_wireframes, chunk_seqs, num_streams,
                                              chunk_max_seqs, ln_fuse_max_rows, flags, x3_min_rows), sync_every, tok_sos)
        W, R, CF = int(beam_width or 0), int(num_samples or 0), constrain_flags(constrain)
        CB = _modes.constrain_beams_value(constrain_beams, CF)
        LA = _modes.constrain_lookahead_value(constrain_lookahead, CF, CB)
        EX = _modes.constrain_exact_value(constrain_exact, CF, CB, LA)
        CS = _modes.constrain_samples_value(constrain_samples, CF, CB)
        CL = _modes.constrain_beam_closure_value(constrain_beam_closure, CF, CB, LA, EX, CS)
        mode, value = _modes.of_options(logprob, CB, LA, EX, CS, CL, constrain=CF, num_samples=R, beam_width=W)   # (value None: the greedy record)
        o = dict(retire=retire, return_pointer=return_pointer, no_stop=no_stop, stop_callback=stop_callback, extra_mask=extra_mask,
                 logprob=logprob, beam_width=W, num_samples=R, constrain=CF, constrain_beams=CB, constrain_samples=CS, temperature=temperature, top_k=top_k, top_p=top_p,
                 uniforms=uniforms, follow_table=follow_table, constrain_lookahead=LA, constrain_exact=EX, constrain_beam_closure=CL, close_dist=close_dist, cycle_len=cycle_len, num_input=num_input, staged_num_input=staged_num_input, trace=trace,
                 N=memory.shape[0], S=memory.shape[1], F=F, T=T)
        if value is not None:    # (retire, an option of the greedy record, is checked behind the operands)
            _modes.check_options(mode, variant, o, term_range)
            mode.operand(self, o)
        _dev(memory, "memory")
        self._same_device(memory, "memory"), self._same_device(mask_u8, "mask"), self._same_device(kv_len, "kv_len")
        N, S, E = memory.shape
        flags |= (_L.FF_RETURN_POINTER if return_pointer else 0) | (_L.FF_NO_STOP if no_stop else 0)
        if retire:
            _modes.check_options(_modes.GREEDY, variant, o, term_range)
            flags |= _L.FF_RETIRE_FINISHED
            if extra_mask is None:     # (retirement supersedes the padding-anchor de-duplication: both on)
                flags |= _L.FF_DEDUP_PAD_ANCHORS
        if return_pointer or extra_mask is not None:   # (every padding-anchor row has its own extra-mask row)
            flags &= ~_L.FF_DEDUP_PAD_ANCHORS
        prm = self._params(variant, N, S, F, T, chunk_wireframes, chunk_seqs, num_streams, chunk_max_seqs, ln_fuse_max_rows, flags,
                           x3_min_rows)
        prm.sync_every, prm.tok_sos, prm.tok_eos = sync_every, tok_sos, tok_eos
        if retire or value is not None:
            prm.term_lo, prm.term_hi = int(term_range[0]), int(term_range[1])
        if retire:
            prm.retire_min_shrink = float(retire_min_shrink)
        dev = self.device
        ni = ni_host = None
        if staged_num_input is not None:
            ni_host, ni, vals = staged_num_input
            if len(vals) != N or (num_input is not None and [int(x) for x in num_input] != vals):
                raise ValueError("staged num_input does not belong to this batch")
        elif num_input is not None:
            vals = [int(x) for x in num_input]
            if len(vals) != N:
                raise ValueError("num_input has %d entries for %d wireframes" % (len(vals), N))
            ni_host = (C.c_int * N)(*vals)
            ni = torch.tensor(vals, dtype=torch.int32).to(dev)
        if extra_mask is not None:
            _dev(extra_mask, "extra_mask", torch.uint8)
            self._same_device(extra_mask, "extra_mask")
            extra_mask = extra_mask.contiguous()
        pointer = torch.zeros((max(T - 1, 1), N * F, E), device=dev, dtype=torch.float32) if return_pointer else None
        cb_error, cb = [], None
        if stop_callback is not None and not no_stop:
            # external stop rule (sharded decodes): `stop_callback(counts)` gets this call's per-step counters of the steps a
            # period behind the enqueued ones and returns True to end the decode; `predict` keeps every executed step
            def _stop(_user, cnt, n):
                try:
                    return 1 if stop_callback([cnt[i] for i in range(n)]) else 0
                except BaseException as e:   # never unwind through the C frames: stop, re-raise below
                    cb_error.append(e)
                    return 1
            cb = _L.STOP_FN(_stop)
            prm.stop_fn = C.cast(cb, C.c_void_p)
        out = self._launch(mode, o, prm, N * F, S, (ni_host,), pointer, lambda predict, steps, counts, traced, rows: (
            _p(memory), _p(mask_u8), _p(kv_len), _p(ni), ni_host, _p(extra_mask), _p(predict), C.byref(steps), counts, _p(pointer),
            _p(traced.get("logits")), _p(traced.get("best")), _p(traced.get("second")), _p(rows)))
        if cb_error:
            raise cb_error[0]
        return out

    def _launch(self, mode, o, prm, B, S, size_args, pointer, args):
        """The one call of `mode`'s entry for B rows of `predict` and what surrounds it, for decode() and _decode_sequence: the
        traces, the mode's outputs, the workspace (size_args: what the size query takes behind the parameters), the host counters;
        args(predict, steps, counts, traced, rows) -> the entry's arguments between the parameters and the workspace.  Returns
        decode()'s dict."""
        T, dev = o["T"], self.device
        G = o[mode.subject] if mode.per_anchor else 1       # sequences per anchor (per wireframe of a single-sequence mode)
        steps_max = max(T - 1, 1)
        predict = torch.empty((B, T), device=dev, dtype=torch.int64)
        traced = {}   # the traces, which the C side indexes by decoded sequence
        if o["trace"]:
            traced["logits"] = torch.full((steps_max, B * G, S), float("nan"), device=dev, dtype=torch.float32)
            for key in mode.row_traces:
                traced[key] = torch.full((steps_max, B), float("nan"), device=dev, dtype=torch.float32)
        rows = torch.empty(B * G, device=dev, dtype=torch.int32)
        # the mode's outputs, and the arguments only its entry takes (its parameter struct, or the log-probability output)
        extra, tail = _modes.outputs(mode, self, o, B, traced)
        ws = self._workspace(getattr(self._lib, mode.entry + "_workspace_bytes")(C.byref(self.model), C.byref(prm), *size_args,
                                                                                 *((G,) if mode.per_anchor else ())))
        steps = C.c_int(0)
        counts = (C.c_int * steps_max)()
        slots = (C.c_int * steps_max)()
        prm.slots_per_step = C.cast(slots, C.POINTER(C.c_int))
        with torch.cuda.device(dev):
            _L.check(getattr(self._lib, mode.entry)(C.byref(self.model), C.byref(prm), *args(predict, steps, counts, traced, rows),
                                                    _p(ws), ws.numel(), *tail, _stream()), mode.entry)
        sps = [int(v) for v in slots]
        out = {"predict": predict, "steps": steps.value, "step_counts": list(counts)[: steps.value],
               "seq_of_row": rows, "slots_per_step": sps, "slot_rows": sum((s + 1) * v for s, v in enumerate(sps))}
        if pointer is not None:
            out["pointer"] = pointer[: steps.value]
        out.update(extra)
        if o["trace"]:
            # the C side indexes its traces by DECODED sequence (padding-anchor rows share one); expand to
            # one entry per row of `predict` (per output row of a beam / sampled decode)
            idx = rows.long()
            out["decoded_seqs"] = int(idx.max().item()) + 1 if B else 0
            out.update((key, t[:, idx]) for key, t in traced.items())
        return out

    def _decode_sequence(self, mode, memory, mask_u8, kv_len, variant, o, params, sync_every, tok_sos):
        """decode() with one of SEQUENCE_MODES on, `mode` its record: the checks (ValueError before anything is launched) and
        the call of its entry, whose argument list has no num_input, extra mask, pointer or best / second traces.  params:
        _params' arguments."""
        if mode.sequence.early:
            mode.sequence.early(self, o)
        if variant != _L.FF_SEQ2SEQ or o["F"] != 1:
            raise ValueError("%s is a single-sequence option (FF_SEQ2SEQ, F = 1); the parallel variant %s with %s"
                             % ((mode.subject,) + mode.sequence.parallel_has))
        _modes.check_options(mode, variant, o, None)
        if params[-2] & _L.FF_STOP_EACH_EOS:
            raise ValueError("%s excludes stop_each_eos (FF_STOP_EACH_EOS): every %s is finished by its own EOS already"
                             % (mode.subject, mode.sequence.each))
        mode.operand(self, o)
        prm = self._params(*params)
        _dev(memory, "memory")
        self._same_device(memory, "memory"), self._same_device(mask_u8, "mask"), self._same_device(kv_len, "kv_len")
        prm.sync_every, prm.tok_sos, prm.tok_eos = sync_every, tok_sos, o["tok_eos"]
        return self._launch(mode, o, prm, o["N"], o["S"], (), None, lambda predict, steps, counts, traced, rows: (
            _p(memory), _p(mask_u8), _p(kv_len), _p(predict), C.byref(steps), counts, _p(traced.get("logits")), _p(rows)))

    def _params(self, variant, N, S, F, T, chunk_wireframes, chunk_seqs, num_streams, chunk_max_seqs, ln_fuse_max_rows, flags,
                x3_min_rows):
        """The DecodeParams every entry takes (decode() adds its stop rule's, score() has none)."""
        prm = _L.DecodeParams()
        prm.variant, prm.N, prm.L, prm.F, prm.T = variant, N, S - self.num_token, F, T
        prm.chunk_wireframes, prm.chunk_seqs, prm.num_streams = chunk_wireframes, chunk_seqs, num_streams
        prm.chunk_max_seqs, prm.ln_fuse_max_rows = int(chunk_max_seqs), int(ln_fuse_max_rows)
        prm.flags = flags
        prm.x3_min_rows = int(x3_min_rows) if self._planes else 0
        return prm

    def score(self, memory, mask_u8, kv_len, variant, T, paths, lengths, F=1, trace=False,
              chunk_wireframes=0, chunk_seqs=0, num_streams=1, flags=DEFAULT_FLAGS, x3_min_rows=0, chunk_max_seqs=0,
              ln_fuse_max_rows=0, retire=False, beam_width=None, logprob=False, return_pointer=False, stop_callback=None,
              stop_each_eos=False, extra_mask=None):
        """Teacher-forced scoring of given paths (ff_decode_forced): the decode loop of decode(), fed `paths` instead
        of its argmax.  paths [N*F, T] int64 shaped like predict (column 0: the row's own start token), lengths [N*F] in 0..T-1:
        positions 1..lengths[r] of row r are scored; row r belongs to wireframe r // F.  Returns dict(logprob [N*F, T] fp32,
        greedy [N*F, T] int64, rank [N*F, T] int32 -- column j belongs to paths[:, j], zero past lengths[r] -- seq_logprob [N*F]
        fp32, steps = max(lengths), [logits [T-1, N*F, S] with trace=True: the masked rows, NaN where a micro-batch did not run]).
        The options of decode() that a forced decode excludes (retire, beam_width, logprob, return_pointer, stop_callback,
        extra_mask, stop_each_eos) raise ValueError; tokens outside [0, S) too."""
        _dev(memory, "memory")
        self._same_device(memory, "memory"), self._same_device(mask_u8, "mask"), self._same_device(kv_len, "kv_len")
        N, S, E = memory.shape
        if variant == _L.FF_SEQ2SEQ and F != 1:
            raise ValueError("the seq2seq variant scores one row per wireframe (F = 1)")
        for bit, name in ((_L.FF_RETIRE_FINISHED, "FF_RETIRE_FINISHED"), (_L.FF_RETURN_POINTER, "FF_RETURN_POINTER"),
                          (_L.FF_STOP_EACH_EOS, "FF_STOP_EACH_EOS")):
            if flags & bit:
                raise ValueError("scoring given paths excludes the flag %s" % name)
        B = N * F
        if torch.is_tensor(paths):
            self._same_device(paths, "paths")
        paths, lens = check_forced_options(paths, lengths, B, T, S, retire=retire, beam_width=beam_width, logprob=logprob,
                                           return_pointer=return_pointer, stop_callback=stop_callback, stop_each_eos=stop_each_eos,
                                           extra_mask=extra_mask)
        mode = _modes.FORCED
        o = dict(paths=paths.contiguous(), T=T, lengths_host=(C.c_int * max(B, 1))(*lens))
        prm = self._params(variant, N, S, F, T, chunk_wireframes, chunk_seqs, num_streams, chunk_max_seqs, ln_fuse_max_rows,
                           flags & ~_L.FF_DEDUP_PAD_ANCHORS, x3_min_rows)
        dev = self.device
        o["lengths_dev"] = torch.tensor(lens, dtype=torch.int32).to(dev)
        out, tail = _modes.outputs(mode, self, o, B, None)
        tl = torch.full((max(T - 1, 1), B, S), float("nan"), device=dev, dtype=torch.float32) if trace else None
        ws = self._workspace(getattr(self._lib, mode.entry + "_workspace_bytes")(C.byref(self.model), C.byref(prm)))
        steps = C.c_int(0)
        with torch.cuda.device(dev):
            _L.check(getattr(self._lib, mode.entry)(C.byref(self.model), C.byref(prm), _p(memory), _p(mask_u8), _p(kv_len), *tail,
                                                    C.byref(steps), _p(tl), _p(ws), ws.numel(), _stream()), mode.entry)
        out["steps"] = steps.value
        if trace:
            out["logits"] = tl
        return out
