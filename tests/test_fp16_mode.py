"""The opt-in split kind "fp16" (DESIGN.md 11): one fp16 product per fp32 product, fp32 accumulation.

Kernels against fp64 products of the fp16-ROUNDED operands (an fp32-accumulation bar) and, to show that one product and not a
silent "2 x fp16" ran, against the unrounded operands (a clearly larger error than the fp16x2 kernel's); whole decodes against
the fp64 truth teacher-forced along their own tokens at a 16-bit-class bar; determinism and the engine options; the range
fallback; the CPU surface (split kinds, ctypes layout, CLI flag).
"""
import multiprocessing as mp
import os
import socket
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import batch_to, build_model, case_weights_and_batch, load_golden, token_ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _h(x):
    """round to nearest fp16, back in fp64"""
    return x.to(torch.float16).double()


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------
def test_split_kinds_and_unknown_kinds():
    from faceformer_amd.hip.ops import SPLIT_KINDS
    from faceformer_amd.models.common import SPLIT_KIND_DEFAULT
    assert SPLIT_KINDS == {"bf16x3": 0, "fp16x2": 1, "fp16": 2}
    assert SPLIT_KIND_DEFAULT == "fp16x2"
    from faceformer_amd.hip.engine import PathEngine
    with pytest.raises(ValueError):
        PathEngine({}, 8, split_kind="fp8")


def test_header_declares_the_one_term_abi():
    """ABI 105: the header's version, kv_terms appended as the LAST field of ff_attn_desc (zero = today's two terms), and the
    ctypes mirror with the same field order and every new entry point."""
    from faceformer_amd.hip import lib as L
    h = open(os.path.join(ROOT, "include", "faceformer_hip.h")).read()
    assert "#define FF_ABI_VERSION 105" in h and L.FF_ABI_VERSION == 105
    body = h[h.index("typedef struct ff_attn_desc {"):h.index("} ff_attn_desc;")]
    fields = [f for f in ("kv_planes", "kv_terms") if f in body]
    assert fields == ["kv_planes", "kv_terms"] and body.index("kv_terms") > body.index("kv_planes")
    assert [n for n, _ in L.AttnDesc._fields_][-2:] == ["kv_planes", "kv_terms"]
    assert L.AttnDesc.kv_terms.offset > L.AttnDesc.kv_planes.offset
    for fn in ("ff_split_weight_fp16_bytes", "ff_split_weight_fp16", "ff_gemm_h1", "ff_gemm_h1_ln"):
        assert fn + "(" in h and fn in L.SIGNATURES


def test_cli_fp16_flag_sets_the_split_kind():
    sys.path.insert(0, ROOT)
    import main as cli
    from faceformer_amd.models import SurfaceFormer_Parallel
    args = cli.build_parser().parse_args(["--fp16"])
    assert args.fp16
    assert not cli.build_parser().parse_args([]).fp16
    kw = dict(num_model=128, num_head=2, num_feedforward=256, num_encoder_layers=1, num_decoder_layers=1, num_lines=20,
              max_face_length=8, token=token_ns())
    m = cli.configure_model(SurfaceFormer_Parallel(**kw), fp16=True)
    assert m.split_kind == "fp16"
    m = cli.configure_model(SurfaceFormer_Parallel(**kw))
    assert m.split_kind == "fp16x2"


def test_cli_main_passes_fp16_to_the_decode(monkeypatch):
    """main.py's entry point hands --fp16 to run_test (which applies it through configure_model); without the flag it does not."""
    sys.path.insert(0, ROOT)
    import main as cli
    seen = []
    monkeypatch.setattr(cli, "run_test", lambda cfg, ckpt, **kw: seen.append(kw))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    cli.main(["--fp16", "--test_ckpt", "unused.ckpt"])
    cli.main(["--test_ckpt", "unused.ckpt"])
    assert [kw["fp16"] for kw in seen] == [True, False]


# ---- GPU: the one-term GEMM ---------------------------------------------------------------------------------------------------------
def _fp16_w(N, K, seed, scale=0.05):
    return (torch.rand(N, K, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * scale


def _check_one_product(got, a_used, w, ref_rounded, ref_exact, den, x2h=None):
    """fp32-accumulation bar against the rounded operands; and a larger error than fp16x2 against the exact ones."""
    K = a_used.shape[1]
    assert torch.isfinite(got).all()
    err = (got - ref_rounded).abs()
    bar = K * 2.0 ** -24 * den + 2.0 ** -22 * ref_rounded.abs() + 2.0 ** -40   # (fp32 accumulation of K exact products)
    assert bool((err <= bar).all()), float((err / bar).max())
    if x2h is not None:
        e1 = ((got - ref_exact).abs() / den).max()
        e2 = ((x2h - ref_exact).abs() / den).max()
        assert e1 > 8 * e2, (float(e1), float(e2))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(37, 512, 512), (300, 1536, 512), (1300, 1024, 512), (2050, 512, 1024), (513, 512, 512),
                                   (4864, 512, 1024)])
def test_gemm_h1_plain_is_one_fp16_product(hip_lib, M, N, K):
    from faceformer_amd.hip import ops
    a = _rnd(M, K, seed=M + N)
    w = _fp16_w(N, K, seed=K)
    b = _rnd(N, seed=3)
    res = _rnd(M, N, seed=4)
    plane = ops.split_weight(w.cuda(), "fp16")
    assert plane.shape == (1, K // 16, N, 16) and plane.dtype == torch.float16
    got = ops.linear_x3(a.cuda(), plane, b.cuda(), act=1, residual=res.cuda()).cpu().double()
    ref_r = torch.relu(_h(a) @ _h(w).t() + b.double()) + res.double()
    ref_e = torch.relu(a.double() @ w.double().t() + b.double()) + res.double()
    den = _h(a).abs() @ _h(w).abs().t() + 1e-30
    x2h = ops.linear_x3(a.cuda(), ops.split_weight(w.cuda(), "fp16x2"), b.cuda(), act=1, residual=res.cuda()).cpu().double()
    _check_one_product(got, a, w, ref_r, ref_e, den, x2h)
    # the plane is plane 0 of the fp16x2 planes
    assert torch.equal(plane[0].cpu(), ops.split_weight(w.cuda(), "fp16x2")[0].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("row_max", [6.0e4, 1.0])
def test_gemm_h1_at_the_range_bound(hip_lib, row_max):
    from test_hip_ops import rows_with_max
    from faceformer_amd.hip import ops
    M, N, K = 512, 512, 512
    a = rows_with_max(M, K, row_max, seed=31)
    w = _fp16_w(N, K, seed=22)
    got = ops.linear_x3(a.cuda(), ops.split_weight(w.cuda(), "fp16"), None).cpu().double()
    den = _h(a).abs() @ _h(w).abs().t()
    _check_one_product(got, a, w, _h(a) @ _h(w).t(), a.double() @ w.double().t(), den)


def _seg_stats(x64):
    M, N = x64.shape
    seg = x64.view(M, N // 32, 32)
    mean = seg.mean(dim=2)
    return torch.stack([mean, ((seg - mean[..., None]) ** 2).sum(dim=2)], dim=2)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["normalise first", "epilogue", "statistics out"])
@pytest.mark.parametrize("M,N", [(300, 512), (1300, 1536), (5000, 1024)])
def test_gemm_h1_layernorm_forms_are_one_fp16_product(hip_lib, form, M, N):
    """MODE 1 (rows normalised, then rounded), MODE 3 (raw rows at 2^-6, rounded; LayerNorm in the epilogue), MODE 2 (statistics of
    the stored rows) -- each against the fp64 product of exactly the operands its contract rounds."""
    from faceformer_amd.hip import ops
    K = 512
    g = torch.Generator().manual_seed(M + N)
    x = (1.5 + 2.0 * torch.randn(M, K, generator=g)) * (1.0 + torch.rand(M, 1, generator=g))
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    xd = x.cuda()
    if form == "statistics out":
        plane = ops.split_weight(W.cuda(), "fp16")
        res = torch.randn(M, N, generator=g)
        out, st = ops.linear_x3_ln(xd, plane, b.cuda(), residual=res.cuda(), want_stats=True)
        got = out.cpu().double()
        ref_r = _h(x) @ _h(W).t() + b.double() + res.double()
        den = _h(x).abs() @ _h(W).abs().t()
        x2h = ops.linear_x3_ln(xd, ops.split_weight(W.cuda(), "fp16x2"), b.cuda(), residual=res.cuda()).cpu().double()
        _check_one_product(got, x, W, ref_r, x.double() @ W.double().t() + b.double() + res.double(), den, x2h)
        want = _seg_stats(out.double())
        assert (st[..., 0].double() - want[..., 0]).abs().max() < 1e-5 * max(1.0, float(want[..., 0].abs().max()))
        return
    gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    Wf, bf, _ = ops.fold_layernorm_linear(W.cuda(), b.cuda(), gamma.cuda(), beta.cuda(), None, 0)
    stats = _seg_stats(xd.double()).float().contiguous()
    plane = ops.split_weight(Wf, "fp16")
    Wf64 = Wf.cpu()
    mean = x.double().mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(dim=1, unbiased=False, keepdim=True) + 1e-5)
    if form == "normalise first":
        n = ((x.double() - mean) * rstd).float()
        got = ops.linear_x3_ln(xd, plane, bf, act=1, stats_in=stats).cpu().double()
        x2h = ops.linear_x3_ln(xd, ops.split_weight(Wf, "fp16x2"), bf, act=1, stats_in=stats).cpu().double()
        ref_e = torch.relu(((x.double() - mean) * rstd) @ Wf64.double().t() + bf.cpu().double())
        ref_r = torch.relu(_h(n) @ _h(Wf64).t() + bf.cpu().double())
        # the kernel normalises in fp32 with its own merged statistics: a row value a few fp32 ulps from an fp16 rounding
        # boundary may round to the neighbouring fp16 value -- one fp16 ulp of that value times |w| per such element
        d = 2.0 ** -20
        flip = (_h(n.double() * (1 + d)) - _h(n.double() * (1 - d))).abs()
        den = _h(n).abs() @ _h(Wf64).abs().t() + (flip @ _h(Wf64).abs().t()) * 2.0 ** 24 / K
    else:
        colsum = Wf.double().sum(dim=1).float().contiguous()
        got = ops.linear_x3_ln(xd, plane, bf, act=1, stats_in=stats, colsum=colsum).cpu().double()
        x2h = ops.linear_x3_ln(xd, ops.split_weight(Wf, "fp16x2"), bf, act=1, stats_in=stats, colsum=colsum).cpu().double()
        ref_e = torch.relu(((x.double() - mean) * rstd) @ Wf64.double().t() + bf.cpu().double())
        xs = _h(x / 64.0) * 64.0
        ref_r = torch.relu((xs @ _h(Wf64).t() - mean * colsum.cpu().double()) * rstd + bf.cpu().double())
        den = (xs.abs() @ _h(Wf64).abs().t() + mean.abs() * colsum.cpu().double().abs()) * rstd
    err = (got - ref_r).abs()
    bar = K * 2.0 ** -24 * den + 1e-6 * (1.0 + ref_r.abs())
    assert bool((err <= bar).all()), float((err / bar).max())
    # one product ran, not a silent fp16x2: clearly farther from the product of the unrounded operands
    e1, e2 = ((got - ref_e).abs() / (den + 1e-30)).max(), ((x2h - ref_e).abs() / (den + 1e-30)).max()
    assert e1 > 8 * e2, (float(e1), float(e2))


# ---- GPU: the one-term attention ---------------------------------------------------------------------------------------------------
def _h1_attention(ops, q, k, v, G, H, nq, nk, kv_len=None, mask=None):
    planes = ops.split_kv(k.cuda(), v.cuda(), G, H, nk, nk, 1)
    old = ops.set_attention_algo(4)
    try:
        return ops.attention(q.cuda(), k.cuda(), v.cuda(), G, H, nq, nk, q_group_stride=nq, q_inner=nq, q_outer_stride=0,
                             k_group_stride=nk, k_stride=1, kv_len=None if kv_len is None else kv_len.cuda(),
                             key_mask=None if mask is None else mask.to(torch.uint8).cuda(), kv_planes=planes, kv_terms=1)
    finally:
        ops.set_attention_algo(old)


def _h1_reference(q, k, v, G, H, nq, nk, mask=None):
    """fp64 attention on fp16(q 0.125), fp16(K), fp16(V), with P rounded to fp16 before P V (the softmax itself exact)."""
    qd = _h(q.double() * 0.125).view(G, nq, H, 64).transpose(1, 2)
    kd = _h(k).view(G, nk, H, 64).transpose(1, 2)
    vd = _h(v).view(G, nk, H, 64).transpose(1, 2)
    s = qd @ kd.transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    mx = s.amax(dim=-1, keepdim=True)
    p = torch.exp(s - mx)
    l = p.sum(dim=-1, keepdim=True)
    o = (_h(p) @ vd) / l
    return o, vd, p / l


def _h1_check(out, q, k, v, G, H, nq, nk, mask=None):
    ref, vd, pn = _h1_reference(q, k, v, G, H, nq, nk, mask)
    got = out.cpu().double().view(G, nq, H, 64).transpose(1, 2)
    # the kernel's P is relative to a running (per-tile) maximum, the reference's to the row maximum: the rounding of P differs
    # by up to one fp16 ulp per weight, 2^-11 of sum_j p_j |v_j|; plus the fp32 exp2 / accumulation
    bar = 2.0 ** -10 * (pn @ vd.abs()) + 2e-6 * vd.abs().amax(dim=-2, keepdim=True)
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    assert bool((err <= bar).all()), float((err / bar).max())


@pytest.mark.gpu
@pytest.mark.parametrize("nk", [1, 31, 32, 33, 287, 288])
def test_attention_h1_is_one_fp16_product_per_key_count(hip_lib, nk):
    from faceformer_amd.hip import ops
    G, H, nq = 4, 2, 40
    E = H * 64
    q, k, v = _rnd(G * nq, E, seed=60), _rnd(G * nk, E, seed=61), _rnd(G * nk, E, seed=62)
    kv_len = torch.tensor([nk, max(1, nk - 1), max(1, nk // 2), max(1, nk - 32)], dtype=torch.int32)
    mask = torch.arange(nk)[None, :] >= kv_len[:, None]
    if nk > 2:
        mask[0, 1] = True
    out = _h1_attention(ops, q, k, v, G, H, nq, nk, kv_len, mask)
    _h1_check(out, q, k, v, G, H, nq, nk, mask)
    # keys past kv_len have no effect
    past = (torch.arange(nk)[None, :] >= kv_len[:, None]).reshape(-1)
    if past.any():
        k2, v2 = k.clone(), v.clone()
        k2[past] = _rnd(int(past.sum()), E, seed=63, scale=300.0)
        v2[past] = _rnd(int(past.sum()), E, seed=64, scale=300.0)
        assert torch.equal(_h1_attention(ops, q, k2, v2, G, H, nq, nk, kv_len, mask), out)
    # not a silent 2 x fp16: clearly farther from the unrounded attention than the two-term kernel
    planes = ops.split_kv(k.cuda(), v.cuda(), G, H, nk, nk, 1)
    old = ops.set_attention_algo(4)
    try:
        two = ops.attention(q.cuda(), k.cuda(), v.cuda(), G, H, nq, nk, q_group_stride=nq, q_inner=nq, q_outer_stride=0,
                            k_group_stride=nk, k_stride=1, kv_len=kv_len.cuda(), key_mask=mask.to(torch.uint8).cuda(),
                            kv_planes=planes)
    finally:
        ops.set_attention_algo(old)
    from test_hip_ops import ref_attention
    exact = ref_attention(q.double().view(G, nq, H, 64).transpose(1, 2), k.double().view(G, nk, H, 64).transpose(1, 2),
                          v.double().view(G, nk, H, 64).transpose(1, 2), mask)
    e1 = (out.cpu().double().view(G, nq, H, 64).transpose(1, 2) - exact).abs().max()
    e2 = (two.cpu().double().view(G, nq, H, 64).transpose(1, 2) - exact).abs().max()
    if nk > 1:
        assert e1 > 8 * e2, (float(e1), float(e2))


@pytest.mark.gpu
def test_attention_h1_more_than_65535_head_pairs(hip_lib):
    from faceformer_amd.hip import ops
    G, H, nq, nk = 8193, 8, 2, 5
    E = H * 64
    q, k, v = _rnd(G * nq, E, seed=70), _rnd(G * nk, E, seed=71), _rnd(G * nk, E, seed=72)
    kv_len = torch.tensor([nk - (g % 3) for g in range(G)], dtype=torch.int32)
    mask = torch.arange(nk)[None, :] >= kv_len[:, None]
    out = _h1_attention(ops, q, k, v, G, H, nq, nk, kv_len, mask)
    torch.cuda.empty_cache()
    _h1_check(out, q, k, v, G, H, nq, nk, mask)


# ---- GPU: whole decodes -------------------------------------------------------------------------------------------------------------
def _fp16_model(name, **attrs):
    case, z = load_golden(name)
    sd, batch = case_weights_and_batch(case)
    model = build_model(case, sd, "cuda")
    model.split_kind = "fp16"
    model.x3_min_rows = 1          # every decoder projection and cross-attention launch takes the fp16 products
    for k, v in attrs.items():
        setattr(model, k, v)
    return case, z, sd, batch, model


def _r16(t):
    return t.to(torch.float16).to(t.dtype)


def _attend(q, k, v, num_head, key_padding_mask, cross):
    """softmax(q k^T / sqrt(hd) + mask) v over [L, B, E] rows (nn.MultiheadAttention's core, eval mode); cross=True: the two
    products take fp16 operands, fp16(q scale) fp16(K)^T and fp16(P) fp16(V), the softmax stays exact."""
    import torch.nn.functional as F
    Lq, B, E = q.shape
    Lk, hd = k.shape[0], E // num_head
    q = q.reshape(Lq, B * num_head, hd).transpose(0, 1) * (1.0 / hd ** 0.5)
    k = k.reshape(Lk, B * num_head, hd).transpose(0, 1)
    v = v.reshape(Lk, B * num_head, hd).transpose(0, 1)
    s = (_r16(q) @ _r16(k).transpose(1, 2)) if cross else q @ k.transpose(1, 2)
    if key_padding_mask is not None:
        kpm = F._canonical_mask(mask=key_padding_mask, mask_name="key_padding_mask", other_type=None, other_name="attn_mask",
                                target_type=q.dtype)
        s = (s.view(B, num_head, Lq, Lk) + kpm[:, None, None, :]).view(B * num_head, Lq, Lk)
    p = torch.softmax(s, dim=-1)
    o = (_r16(p) @ _r16(v)) if cross else p @ v
    return o.transpose(0, 1).reshape(Lq, B, E)


def _emulated_decoder_layer(sd, p, tgt, memory, memory_key_padding_mask, pos, query_pos, num_head, tgt_mask=None):
    """refpath.decoder_layer (reference transformer.py:235-256, pre-norm) with the "fp16" contract as the engine binds it
    (fp64 otherwise).  The LayerNorm-consuming projections take the NORMALISED rows n and the folded weight
    W gamma as their fp16 operands (LN(x) W^T + b = n (W gamma)^T + W beta + b, the query-position term qpos W^T exact); the
    out-projections and linear2 take fp16(their input) and fp16(W); the cross-attention K | V of the memory are projected
    exactly and enter the products as fp16(K), fp16(V) (_attend).  LayerNorm statistics, biases, ReLU, residuals, softmax exact."""
    import torch.nn.functional as F
    from oracle import refpath
    assert tgt_mask is None
    E = tgt.shape[-1]
    g = lambda n: sd[p + "." + n]
    norm = lambda x: F.layer_norm(x, (E,), None, None, refpath.LN_EPS)

    def folded(n, W, b, gamma, beta, table=None):
        out = _r16(n) @ _r16(W * gamma).t() + (W @ beta + b)
        return out if table is None else out + table @ W.t()

    def plain(x, W, b):
        return _r16(x) @ _r16(W).t() + b
    W, b = g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias")
    n1 = norm(tgt)
    qk = folded(n1, W[:2 * E], b[:2 * E], g("norm1.weight"), g("norm1.bias"), query_pos)
    v = folded(n1, W[2 * E:], b[2 * E:], g("norm1.weight"), g("norm1.bias"))
    a = _attend(qk[..., :E], qk[..., E:], v, num_head, None, cross=False)
    tgt = tgt + plain(a, g("self_attn.out_proj.weight"), g("self_attn.out_proj.bias"))
    W, b = g("multihead_attn.in_proj_weight"), g("multihead_attn.in_proj_bias")
    q = folded(norm(tgt), W[:E], b[:E], g("norm2.weight"), g("norm2.bias"), query_pos)
    k = (memory + pos) @ W[E:2 * E].t() + b[E:2 * E]
    v = memory @ W[2 * E:].t() + b[2 * E:]
    a = _attend(q, k, v, num_head, memory_key_padding_mask, cross=True)
    tgt = tgt + plain(a, g("multihead_attn.out_proj.weight"), g("multihead_attn.out_proj.bias"))
    h = torch.relu(folded(norm(tgt), g("linear1.weight"), g("linear1.bias"), g("norm3.weight"), g("norm3.bias")))
    _emulated_decoder_layer.calls += 1
    return tgt + plain(h, g("linear2.weight"), g("linear2.bias"))


_emulated_decoder_layer.calls = 0


def _forced_logits(case, sd, batch, pred, steps, emulate, monkeypatch, device="cuda"):
    """fp64 logits [steps, B, S] of the oracle teacher-forced along `pred` [B, T]; emulate=True runs the fp16 contract inside it."""
    from oracle import refpath
    sd64 = {k: (v.to(device, torch.float64) if v.is_floating_point() else v.to(device)) for k, v in sd.items()}
    b64 = {k: (v.to(device, torch.float64 if v.is_floating_point() else v.dtype) if torch.is_tensor(v) else v)
           for k, v in batch.items()}
    if emulate:
        monkeypatch.setattr(refpath, "decoder_layer", _emulated_decoder_layer)
        _emulated_decoder_layer.calls = 0
    forced = torch.from_numpy(pred).to(device)
    H = case["model"]["H"]
    out = []
    try:
        if case["kind"] == "parallel":
            F = max(int(n) for n in batch["num_input"])
            for c in range(0, pred.shape[0], 256):
                tr = {}
                seqs = torch.arange(c, min(c + 256, pred.shape[0]), device=device)
                refpath.parallel_forward_eval(sd64, dict(b64), num_head=H, trace=tr, forced=forced, steps=steps, seqs=seqs,
                                              num_anchors=F)
                out.append(torch.stack(tr["logits"], dim=0).cpu().numpy())
        else:
            tr = {}
            refpath.seq2seq_forward_eval(sd64, dict(b64), num_head=H, trace=tr, forced=forced, steps=steps,
                                         extra_mask=b64.get("extra_mask"))
            out.append(torch.stack(tr["logits"], dim=0).cpu().numpy())
    finally:
        if emulate:
            monkeypatch.undo()
    if emulate:   # every decoder layer of every step took the emulated form
        n_steps = steps * (1 if case["kind"] != "parallel" else -(-pred.shape[0] // 256))
        assert _emulated_decoder_layer.calls == case["model"]["dec"] * n_steps, _emulated_decoder_layer.calls
    return np.concatenate(out, axis=1)


# The model-level bar is DERIVED from the contract, per step s: the same forced run with the contract's roundings emulated in fp64
# (_emulated_decoder_layer in place of refpath.decoder_layer) is e_emu[s] = max |emulated - truth| over the step's live logits away from the truth; the HIP decode must stay
# within 2 e_emu[s] + an fp32 floor of 2^-17 max(1, max |truth|): the emulation rounds the same operands as the engine, but the
# engine's fp32 arithmetic around them (statistics, accumulation order) moves individual roundings to the neighbouring fp16 value.
# An extra 16-bit rounding where the contract keeps fp32 (the pointer head, the residual stream) would not fit under it.
EMU_FACTOR, FP32_FLOOR = 2.0, 2.0 ** -17


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_full_B256_default", "par_full_B256_gain4", "par_small_ragged300", "seq_full_A4_gain4"])
def test_fp16_decode_against_fp64_truth(hip_lib, name, monkeypatch):
    from oracle import truth as TR
    from test_parity_golden import run_traced
    from faceformer_amd.hip import ops
    case, z, sd, batch, model = _fp16_model(name)
    old = ops.set_attention_algo(4)        # every cross-attention launch on the one-term kernel, as the emulation assumes
    try:
        with torch.no_grad():
            out = run_traced(model, case, batch_to(batch, "cuda"))
    finally:
        ops.set_attention_algo(old)
    eng = model.engine()
    assert eng.split_kind == "fp16" and eng.model.split_kind == 2
    T = case["model"]["seq_len"]
    kind = case["kind"]
    hip = dict(predict=out["predict"].cpu().numpy().reshape(-1, T), steps=int(out["steps"]), logits=out["logits"].cpu().numpy(),
               best=out["best"].cpu().numpy(), second=out["second"].cpu().numpy())
    steps = hip["steps"]
    truth = _forced_logits(case, sd, batch, hip["predict"], steps, False, monkeypatch)
    emu = _forced_logits(case, sd, batch, hip["predict"], steps, True, monkeypatch)
    fill = np.finfo(np.float64).min
    live = truth > fill
    scale = np.array([max(1.0, float(np.abs(truth[s][live[s]]).max())) for s in range(steps)])
    e_emu = np.array([float(np.abs(emu[s] - truth[s])[live[s]].max()) for s in range(steps)])
    assert (e_emu > 16 * FP32_FLOOR * scale).any(), "the emulation rounded nothing"
    tol = EMU_FACTOR * e_emu + FP32_FLOOR * scale
    first = TR.anchor_column(kind, batch["num_input"], max(int(n) for n in batch["num_input"])) if kind == "parallel" else None
    st = TR.check_trace_against_truth(hip, truth, tol, kind=kind, e_ref=e_emu, ref_factor=EMU_FACTOR, ref_floor=FP32_FLOOR,
                                      first_column=first)
    e_hip = np.array([float(np.abs(hip["logits"][s].astype(np.float64) - truth[s])[live[s]].max()) for s in range(steps)])
    print(name, "hip/emulated error, worst step %.3f, median %.3f" % ((e_hip / e_emu).max(), np.median(e_hip / e_emu)),
          "emulated error / scale max %.2e" % (e_emu / scale).max(), st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["par_small_ragged", "par_full_n40_gain4"])
def test_fp16_decode_is_deterministic_across_engine_options(hip_lib, name):
    from faceformer_amd import faces
    from faceformer_amd.hip import lib as L
    case, z, sd, batch, model = _fp16_model(name)
    b = batch_to(batch, "cuda")
    T = case["model"]["seq_len"]

    def run(retire=False, **kw):
        eng, memory, mask, kv_len = model._encode(b)
        ni = [int(n) for n in b["num_input"]]
        opts = dict(sync_every=model.sync_every, flags=model.decode_flags, x3_min_rows=model.x3_min_rows,
                    chunk_wireframes=model.chunk_wireframes, chunk_seqs=model.chunk_seqs, chunk_max_seqs=model.chunk_max_seqs,
                    num_streams=model.num_streams, ln_fuse_max_rows=model.ln_fuse_max_rows)
        opts.update(kw)
        out = eng.decode(memory, mask, kv_len, L.FF_PARALLEL, T=T, F=max(ni), num_input=ni,
                         extra_mask=model._extra_mask(b), retire=retire, **opts)
        return out["predict"].cpu().numpy().reshape(-1, T), int(out["steps"])

    base, steps = run()
    assert np.array_equal(run()[0], base)
    for kw in (dict(num_streams=1, chunk_wireframes=1), dict(num_streams=2, chunk_wireframes=1), dict(sync_every=1),
               dict(chunk_seqs=8)):
        got, s = run(**kw)
        assert s == steps and np.array_equal(got, base), kw
    got, s = run(retire=True, term_range=(1, 4))
    want, s_r = faces.retired_view(base, token_ns(), return_steps=True)
    assert s == s_r and np.array_equal(got, want.reshape(-1, T))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dist_worker(rank, world, port, name, ret):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from conftest import batch_to, build_model
    from faceformer_amd import dist as ffd
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        case, _z = load_golden(name)
        sd, batch = case_weights_and_batch(case)
        model = build_model(case, sd, "cuda:0")
        model.split_kind = "fp16"
        model.x3_min_rows = 1
        out = ffd.decode_sharded(model, batch_to(batch, "cuda:0"), dist)
        ret[rank] = out["predict"].cpu().numpy()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_fp16_sharded_decode_equals_single_process(hip_lib):
    name = "par_small_ragged"
    case, z, sd, batch, model = _fp16_model(name)
    with torch.no_grad():
        single = model(batch_to(batch, "cuda"))["predict"].cpu().numpy()
    ctx = mp.get_context("spawn")
    manager = ctx.Manager()
    try:
        ret = manager.dict()
        port = _free_port()
        procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, name, ret)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
        for p in procs:            # a rank that did not finish holds the GPU: end it before any assertion
            if p.is_alive():
                p.kill()
                p.join(30)
        assert [p.exitcode for p in procs] == [0, 0]
        got = {r: ret[r] for r in range(2)}
    finally:
        manager.shutdown()
    for r in range(2):
        assert np.array_equal(got[r], single), r


@pytest.mark.gpu
def test_fp16_out_of_range_variant_falls_back_to_bf16x3(hip_lib):
    from test_fp16_range import make_variant
    from faceformer_amd.hip.engine import FP16_LIM
    case, sd, batch, pushed = make_variant("cross K up")
    model = build_model(case, sd, "cuda")
    model.split_kind = "fp16"
    model.x3_min_rows = 1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        eng = model.engine()
    msgs = [str(x.message) for x in w if "fp16" in str(x.message)]
    assert len(msgs) == 1 and "'fp16'" in msgs[0] and all(c in msgs[0] for c in pushed), msgs
    assert eng.split_kind == "bf16x3" and eng.requested_kind == "fp16" and eng.model.split_kind == 0
    assert {k for k, v in eng.fp16_operand_bounds.items() if v >= FP16_LIM} == pushed
    with torch.no_grad():
        out = model(batch_to(batch, "cuda"))
    assert model.engine() is eng           # requested_kind still matches: the engine is not rebuilt
    assert out["predict"].shape[0] == batch["input"].shape[0]
