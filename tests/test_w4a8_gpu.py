"""``dnn_gemm_w4a8``: the MXFP4 prefill GEMM on MX e4m3 activations (the codes on the scaled MFMA, no
expansion) against fp64 references, and the mxfp4 stage with ``mxfp4_prefill="e4m3"`` (MI355X only)."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_transformer_gpu import _gpt2_fp8_golden
from test_w4_mid_gpu import _snapped  # a tiny checkpoint whose layer projections lie on the MXFP4 grid

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _mx_dequant(q, sx, M, kp):
    """fp64 values of MX e4m3 rows: byte x 2^(e - 127), e the e8m0 scale of (row, 128-column block) at
    csrc/kernels/common.h mx_index (the decode of tests/test_gemm_exact_prefill_gpu.py)."""
    mpad = (M + 63) // 64 * 64
    t, m = torch.arange(kp // 128), torch.arange(M)
    idx = (t[None, :] * (mpad // 64) + (m[:, None] // 64)) * 64 + (m[:, None] % 16) * 4 + (m[:, None] // 16) % 4
    sc = torch.exp2(sx.reshape(-1)[idx.to(sx.device)].double() - 127.0).repeat_interleave(128, dim=1)
    return q.reshape(-1)[:M * kp].view(M, kp).view(torch.float8_e4m3fn).double() * sc


def _buffers(M, kp):
    from distributed_neural_networks_amd.ops.fp8 import mx_scale_bytes
    return (torch.zeros(M * kp, dtype=torch.uint8, device=DEV),
            torch.zeros(mx_scale_bytes(M, kp), dtype=torch.uint8, device=DEV))


# N = 16400 (65 column tiles of 256): at M = 257 / 300 the launcher takes the 256-row tile kernel (2 x 65 > 128
# tiles), with 1, 2, 3 and 9 K-tiles (9: the 4-stage ring wraps twice); every other shape runs the 128-row kernel
NK = [(16, 128), (40, 160), (272, 384), (544, 1152), (4800, 416),
      (16400, 128), (16400, 160), (16400, 384), (16400, 1152)]


@pytest.mark.parametrize("N,K,epi", [(N, K, e) for N, K in NK for e in ("none", "bias_relu_res", "silu_mul")
                                     if e != "silu_mul" or N % 16 == 0])  # SILU_MUL: N % 16 == 0 is its contract
@pytest.mark.parametrize("M", [65, 128, 257, 300])
def test_gemm_w4a8_exact(M, N, K, epi):
    """Codes uniform in 0..15, block exponents in {126, 127, 128}; activations integers in [-3, 3] x 2^s, s in
    {-1, 0, 1} per (row, 128 columns), which quant_rows_mx must encode exactly (asserted on its decoded output);
    bias in quarters, integer residual, strided rows.  Products are multiples of 1 / 8 and sum |x| |w| stays
    under 2^24 of them (asserted), so fp32 is exact in any order: out == bf16(fp64 reference), guard rows and
    columns keep their sentinel.  SILU_MUL (pack_gate_up weights): fp64 reference, 2^-7 relative."""
    from distributed_neural_networks_amd.ops.gemm import pack_gate_up
    from distributed_neural_networks_amd.ops.w4 import dequantize, linear_w4a8, pack_mxfp4, quantize_weight_mxfp4
    g = torch.Generator().manual_seed(1000 * M + N)
    w = pack_mxfp4(torch.randint(0, 16, (N, K), generator=g).to(DEV),
                   torch.randint(126, 129, (N, K // 32), generator=g).to(DEV))
    if epi == "silu_mul":
        wd = dequantize(w)
        w = quantize_weight_mxfp4(pack_gate_up(wd[:N // 2], wd[N // 2:]), DEV)  # on the grid: a row permutation
    wd = dequantize(w).double()
    kp = w.kpad
    s = torch.randint(-1, 2, (M, kp // 128), generator=g).repeat_interleave(128, dim=1)[:, :K]
    xw = torch.zeros(M, K + 64)
    xw[:, :K] = torch.randint(-3, 4, (M, K), generator=g) * torch.exp2(s.float())
    x = xw.to(DEV, BF)[:, :K]
    q8, sx = _buffers(M, kp)
    act = {"none": 0, "bias_relu_res": 1, "silu_mul": 3}[epi]
    No = N // 2 if act == 3 else N
    bias = (torch.randint(-8, 9, (N,), generator=g) * 0.25).to(DEV) if act == 1 else None
    R = torch.randint(-4, 5, (M, No + 8), generator=g).to(DEV, BF)[:, :No] if act == 1 else None
    buf = torch.full((M + 2, No + 8), 7.0, device=DEV, dtype=BF)
    out = buf[1:M + 1, :No]
    linear_w4a8(x, w, bias, act, R, out, q8, sx)
    xq = _mx_dequant(q8, sx, M, kp)
    assert torch.equal(xq[:, :K], x.double()) and bool((xq[:, K:] == 0).all())
    assert float((x.double().abs() @ wd.abs().t()).max()) * 8 < 2 ** 24
    y = x.double() @ wd.t()
    assert bool((buf[0] == 7.0).all()) and bool((buf[M + 1] == 7.0).all()) and bool((buf[:, No:] == 7.0).all())
    if act == 3:
        cols = torch.arange(N, device=DEV).view(-1, 16)
        gt, up = y[:, cols[:, :8].reshape(-1)], y[:, cols[:, 8:].reshape(-1)]
        y = F.silu(gt) * up
        # the floor: fp32 silu is g / (1 + e^-g), whose e^-g passes 2^128 below g = -88.7, where the true
        # |silu(g) u| < |g u| 2^-128; and results below 2^-126 leave bf16's normal range
        floor = 2.0 ** -126 * (1 + (gt * up).abs())
        err = ((out.double() - y).abs() - floor).clamp_min(0) / y.abs().clamp_min(2.0 ** -126)
        print(f"w4a8 silu_mul M {M} N {N} K {K}: max rel {err.max().item():.3e}")
        assert bool(((out.double() - y).abs() <= 2.0 ** -7 * y.abs() + floor).all()), err.max().item()
        return
    if act == 1:
        y = (y + bias.double()).clamp_min(0) + R.double()
    assert torch.equal(out, y.to(BF))


@pytest.mark.parametrize("norm,act", [(1, 0), (1, 3), (2, 0), (2, 2)])
@pytest.mark.parametrize("M", [65, 300])
def test_gemm_w4a8_norm_epilogues(M, norm, act):
    """The cases of test_gemm_w4_mid_norm_epilogues through linear_norm(..., q8=, sx=), against fp64 on the
    dequantised weight and the DECODED q8 / sx of the norm pass: only fp32 accumulation and the bf16 output rounding
    remain, |err| <= 2^-8 |y| + K 2^-24 sum_k |a| |w| (half a bf16 ulp; K roundings on partial sums bounded by
    sum |a| |w|, carried through GELU / SwiGLU by the derivative bound)."""
    from distributed_neural_networks_amd.ops.gemm import fold_norm, linear_norm, pack_gate_up
    from distributed_neural_networks_amd.ops.w4 import dequantize
    torch.manual_seed(11)
    N, K = 544, 1152
    x = (torch.randn(M, K, device=DEV) + 0.3).bfloat16()
    W = torch.randn(N, K, device=DEV) / math.sqrt(K)
    Wk = pack_gate_up(W[: N // 2], W[N // 2:]) if act == 3 else W
    gamma = torch.rand(K, device=DEV) + 0.5
    beta = torch.randn(K, device=DEV) * 0.1 if norm == 2 else None
    bias = torch.randn(N, device=DEV) * 0.1 if act != 3 else None
    f = fold_norm(Wk, gamma, beta, bias, norm == 1, 1e-5, DEV, quant="mxfp4")
    Nout = N // 2 if act == 3 else N
    R = torch.randn(M, Nout, device=DEV).bfloat16() if act == 0 else None
    out = torch.empty(M, Nout, device=DEV, dtype=BF)
    q8, sx = _buffers(M, f.w.kpad)
    linear_norm(x, f, act, R, out, ones=torch.ones(K, device=DEV), q8=q8, sx=sx)
    a = _mx_dequant(q8, sx, M, f.w.kpad)[:, :K]
    wd = dequantize(f.w).double()
    y = a @ wd.t()
    slack = K * 2.0 ** -24 * (a.abs() @ wd.abs().t())
    if f.bias is not None:
        y = y + f.bias.double()
    if act == 3:
        cols = torch.arange(N, device=DEV).view(-1, 16)
        gi, ui = cols[:, :8].reshape(-1), cols[:, 8:].reshape(-1)
        # d(silu(g) u) <= 1.1 |u| dg + |silu(g)| du (|silu'| <= 1.1)
        slack = 1.1 * y[:, ui].abs() * slack[:, gi] + F.silu(y[:, gi]).abs() * slack[:, ui]
        y = F.silu(y[:, gi]) * y[:, ui]
    else:
        if act == 2:
            y = F.gelu(y)
            slack = 1.13 * slack  # |gelu'| <= 1.13
        if R is not None:
            y = y + R.double()
    tol = 2.0 ** -8 * y.abs() + slack
    err = (out.double() - y).abs()
    print(f"w4a8 norm {norm} act {act} M {M}: max err / tol {(err / tol.clamp_min(1e-30)).max().item():.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("key,val,rc", [("M", 0, -2), ("N", 0, -3), ("K", 48, -3), ("act", 4, -3), ("Ws", 0, -1),
                                        ("sx", 0, -1), ("A8", "+2", -5), ("sx", "+2", -5), ("ldc", 39, -4),
                                        ("ldr", 39, -4)])
def test_gemm_w4a8_rejections(key, val, rc):
    """The negative returns of dnn_gemm_w4a8; nothing is launched, so ``out`` keeps its content."""
    from distributed_neural_networks_amd.ops._lib import lib, stream_ptr
    from distributed_neural_networks_amd.ops.w4 import pack_mxfp4
    w = pack_mxfp4(torch.zeros(40, 128, dtype=torch.uint8, device=DEV),
                   torch.full((40, 4), 127, dtype=torch.uint8, device=DEV))
    q8, sx = _buffers(128, 128)
    out = torch.full((80, 40), 7.0, device=DEV, dtype=BF)
    a = dict(A8=q8.data_ptr(), sx=sx.data_ptr(), Wq=w.q.data_ptr(), Ws=w.scales.data_ptr(), C=out.data_ptr(), ldc=40,
             bias=0, R=out.data_ptr(), ldr=40, M=80, N=40, K=128, act=0, st=stream_ptr())
    a[key] = a[key] + 2 if val == "+2" else val
    assert lib().gemm_w4a8(**a) == rc
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _gpt2_golden(st, sd):
    """test_transformer_gpu's fp32 GPT-2 golden (no activation quantiser) on the stage's own dequantised (folded)
    MXFP4 projections and bf16 head, each presented as that golden reads a weight: values x unit channel scales."""
    from types import SimpleNamespace as NS
    from distributed_neural_networks_amd.ops.w4 import Mxfp4Weight, dequantize

    def as8(w):
        v = dequantize(w) if isinstance(w, Mxfp4Weight) else w.float()
        return NS(q=v, k=v.shape[1], scale=torch.ones(v.shape[0], device=DEV))

    def folded(f):
        return NS(w=as8(f.w), bias=f.bias)
    layers = [NS(w_qkv=folded(L.w_qkv), w_o=as8(L.w_o), b_o=L.b_o, w_up=folded(L.w_up), w_down=as8(L.w_down),
                 b_down=L.b_down) for L in st.layers]
    return _gpt2_fp8_golden(NS(cfg=st.cfg, eps=st.eps, layers=layers, w_head=folded(st.w_head)), sd)


@pytest.mark.parametrize("prefill", ["e4m3", "bf16"])
def test_gpt2_xl_mxfp4_two_blocks_full_width_vs_golden(prefill):
    """GPT-2 XL at real width (kpad 1664; N 4800 / 1600 / 6400), 2 blocks, (B, T) = (2, 192) + 8 decode steps
    against the fp32 golden on the dequantised MXFP4 weights, held to the bounds of
    test_gpt2_xl_fp8_two_blocks_full_width_vs_golden (same activation format, same kind of golden): 8e-2 prefill,
    4e-2 decode.  "e4m3": the expand scratch keeps its sentinel (no expansion ran), a second prefill is bit-equal.
    Measured: "e4m3" 5.8e-2 prefill, 2.5e-2 .. 2.7e-2 decode; "bf16" 5.6e-3 and 5.3e-3 .. 5.7e-3."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    B, T, steps = 2, 192, 8
    sd = ckpt.random_stage_state_dict("gpt2-xl", 0, 1, True, True, 17, device=DEV, nontrivial=True)
    st = TransformerStage("gpt2-xl", sd, 0, 1, True, True, DEV, max_batch=B, max_seq=T + steps + 1, w4=True,
                          mxfp4_prefill=prefill)
    gold = _gpt2_golden(st, sd)
    ids = torch.randint(0, 50257, (B, T), generator=torch.Generator().manual_seed(6))
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    if prefill == "e4m3":
        st.w4_scratch.fill_(7.0)
        first = st.step(ids.to(DEV, torch.int32), pos, B, T).probs.float().clone()
        assert bool((st.w4_scratch == 7.0).all())
    x, Tn, p = ids, T, 0
    for step in range(steps + 1):
        out = st.step(x.to(DEV, torch.int32), pos, B, Tn)
        if step == 0 and prefill == "e4m3":
            assert torch.equal(out.probs.float(), first)
        pos.add_(Tn)
        rel = _rel(out.probs.float(), gold(x.to(DEV), p).float())
        print(f"mxfp4_prefill {prefill} step {step}: rel {rel:.3e}")
        assert rel < (8e-2 if step == 0 else 4e-2), (step, rel)
        x, p, Tn = out.pred.long().view(B, 1), p + Tn, 1


def test_llama3_tiny_w4a8_prefill_matches_bf16_prefill():
    """llama3-tiny (RMS, RoPE, SwiGLU, GQA) at (3, 43) = 129 rows: the prefill logits of the "e4m3" stage within
    8e-2 of the "bf16" stage of the same snapped checkpoint."""
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd, n = _snapped("llama3-tiny")
    ids = torch.randint(0, 512, (3, 43), generator=torch.Generator().manual_seed(5)).to(DEV, torch.int32)
    lg = {}
    for pf in ("e4m3", "bf16"):
        st = build_device_stage("llama3-tiny", sd, 0, n - 1, True, True, DEV, dtype="mxfp4", max_batch=3, max_seq=64,
                                mxfp4_prefill=pf)
        lg[pf] = st.step(ids, torch.zeros(3, dtype=torch.int32, device=DEV), 3, 43).probs.float().clone()
    rel = _rel(lg["e4m3"], lg["bf16"])
    print(f"llama3-tiny w4a8 vs bf16 prefill: rel {rel:.3e}")
    assert rel < 8e-2, rel


def test_mxfp4_prefill_bf16_is_neutral():
    """mxfp4_prefill="bf16" allocates no q8 / sx8 and its prefill logits are bit-equal to a stage built without
    the key."""
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd, n = _snapped("gpt2-tiny")
    ids = torch.randint(0, 512, (3, 43), generator=torch.Generator().manual_seed(5)).to(DEV, torch.int32)
    lg = []
    for kw in ({}, {"mxfp4_prefill": "bf16"}):
        st = build_device_stage("gpt2-tiny", sd, 0, n - 1, True, True, DEV, dtype="mxfp4", max_batch=3, max_seq=64, **kw)
        assert st.q8 is None and st.sx8 is None
        lg.append(st.step(ids, torch.zeros(3, dtype=torch.int32, device=DEV), 3, 43).probs.float().clone())
    assert torch.equal(lg[0], lg[1])
