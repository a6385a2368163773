"""MXFP4 weights on the device: the W4A16 decode GEMM, the expansion and the
``dtype: "mxfp4"`` stage against fp64 references (MI355X only)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _packed(N, K, seed=0):
    """Random codes (all 16 occur) with block exponents in {126, 127, 128}."""
    from distributed_neural_networks_amd.ops.w4 import pack_mxfp4
    g = torch.Generator().manual_seed(seed)
    return pack_mxfp4(torch.randint(0, 16, (N, K), generator=g).to(DEV),
                      torch.randint(126, 129, (N, K // 32), generator=g).to(DEV))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("N,K", [(40, 128), (40, 160), (544, 1152)])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_gemm_w4_exact(M, N, K, act):
    """Integer activations in [-3, 3], weights k / 4 with |w| <= 12, bias in quarters, integer residual: every
    partial sum is a multiple of 0.25 below 1152 * 36 < 2^16, so fp32 accumulates exactly in any order and the
    output is bf16(fp64 reference) bit for bit.  Rows are strided (lda = K + 64)."""
    from distributed_neural_networks_amd.ops.w4 import dequantize, linear_w4
    w = _packed(N, K)
    g = torch.Generator().manual_seed(M)
    x = torch.randint(-3, 4, (M, K + 64), generator=g).to(DEV, BF)[:, :K]
    bias = (torch.randint(-8, 9, (N,), generator=g) * 0.25).to(DEV)
    R = torch.randint(-4, 5, (M, N), generator=g).to(DEV, BF)
    out = torch.zeros(M, N, device=DEV, dtype=BF)
    linear_w4(x, w, bias, act, R, out)
    y = x.double() @ dequantize(w).double().t() + bias.double()
    y = (y.clamp_min(0) if act else y) + R.double()
    assert torch.equal(out, y.to(BF))


@pytest.mark.parametrize("norm,act", [(1, 0), (1, 3), (2, 0), (2, 2)])
@pytest.mark.parametrize("M", [1, 17, 64])
def test_gemm_w4_norm_epilogues(M, norm, act):
    """Folded RMS / LayerNorm with SwiGLU, GELU and residual epilogues against the same algebra in fp64 on the
    dequantised weight: the measure and bound of test_transformer_gpu.py::test_linear_w8."""
    from distributed_neural_networks_amd.ops.gemm import fold_norm, pack_gate_up
    from distributed_neural_networks_amd.ops.w4 import dequantize, linear_w4
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
    linear_w4(x, f.w, f.bias, act, R, out, norm, f.colsum, 1e-5)
    xd = x.double()
    mean = xd.mean(1, keepdim=True) if norm == 2 else torch.zeros_like(xd[:, :1])
    var = xd.pow(2).mean(1, keepdim=True) - mean ** 2
    y = xd @ dequantize(f.w).double().t()
    if norm == 2:
        y = y - mean * f.colsum.double()[None, :]
    y = torch.rsqrt(var + 1e-5) * y
    if f.bias is not None:
        y = y + f.bias.double()
    if act == 3:
        cols = torch.arange(N, device=DEV).view(-1, 16)
        y = F.silu(y[:, cols[:, :8].reshape(-1)]) * y[:, cols[:, 8:].reshape(-1)]
    elif act == 2:
        y = F.gelu(y)
    if R is not None:
        y = y + R.double()
    err = _rel(out, y)
    print(f"w4 norm {norm} act {act} M {M}: rel {err:.3e}")
    assert err < 1e-2, err


@pytest.mark.parametrize("N,K", [(40, 160), (544, 1152)])
def test_w4_expand(N, K):
    """The expansion is bf16(dequantize) bit for bit with ldw > K (the columns past K keep their content); at
    80 rows linear_w4 is the bf16 GEMM on that weight: the same kernel on the same operands."""
    from distributed_neural_networks_amd.ops._lib import lib, stream_ptr
    from distributed_neural_networks_amd.ops.gemm import linear
    from distributed_neural_networks_amd.ops.w4 import dequantize, linear_w4
    w = _packed(N, K, 3)
    wb = dequantize(w).bfloat16()
    buf = torch.full((N, K + 8), 7.0, device=DEV, dtype=BF)
    assert lib().w4_expand(w.q.data_ptr(), w.scales.data_ptr(), buf.data_ptr(), K + 8, N, K, stream_ptr()) == 0
    assert torch.equal(buf[:, :K], wb) and bool((buf[:, K:] == 7.0).all())
    if K % 64 == 0:
        torch.manual_seed(2)
        x, bias = torch.randn(80, K, device=DEV).bfloat16(), torch.randn(N, device=DEV)
        got = linear_w4(x, w, bias, 2, scratch=torch.empty(N * K, device=DEV, dtype=BF))
        assert torch.equal(got, linear(x, wb, bias, 2))


@pytest.mark.parametrize("key,val,rc", [("A", 0, -1), ("Wq", 0, -1), ("Ws", 0, -1), ("C", 0, -1), ("norm", 2, -1),
                                        ("M", 0, -2), ("M", 65, -2), ("K", 48, -3), ("ldc", 39, -4),
                                        ("A", "+2", -5), ("lda", 132, -5)])
def test_gemm_w4_rejections(key, val, rc):
    """The negative returns listed in api.h (null pointers, LayerNorm without colsum, M outside 1..64, K % 32,
    ldc below N, a misaligned A or lda); nothing is launched, so ``out`` keeps its content."""
    from distributed_neural_networks_amd.ops._lib import lib, stream_ptr
    w = _packed(40, 128)
    x = torch.ones(64, 136, device=DEV, dtype=BF)
    out = torch.full((64, 40), 7.0, device=DEV, dtype=BF)
    a = dict(A=x.data_ptr(), lda=136, Wq=w.q.data_ptr(), Ws=w.scales.data_ptr(), C=out.data_ptr(), ldc=40, bias=0, R=0,
             ldr=0, M=4, N=40, K=128, act=0, norm=0, colsum=0, eps=1e-5, st=stream_ptr())
    a[key] = a[key] + 2 if val == "+2" else val
    assert lib().gemm_w4(**a) == rc
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _snapped(model):
    """A tiny checkpoint (norm gains 1, biases 0) whose layer projections lie on the MXFP4 grid."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.ops.w4 import dequantize, quantize_weight_mxfp4
    n = model_info(model).num_layers
    sd = ckpt.random_stage_state_dict(model, 0, n - 1, True, True, 11)
    for k, v in sd.items():
        if k.split(".")[0] in ("h", "layers") and v.dim() == 2:
            sd[k] = dequantize(quantize_weight_mxfp4(v, "cpu"))
    return sd, n


@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_mxfp4_stage_matches_bf16_stage(model):
    """An mxfp4 stage and a bf16 stage of one snapped checkpoint hold identical weight values (the quantiser is
    idempotent): prefill logits of 2 x 40 tokens (80 rows: expand + bf16 GEMMs) and of the next decode step (2
    rows: the W4 kernel) agree within the 3e-2 that test_gpt2_stage_logits_close grants a bf16 stage."""
    from distributed_neural_networks_amd.ops.w4 import Mxfp4Weight
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd, n = _snapped(model)
    ids = torch.randint(0, 512, (2, 41), generator=torch.Generator().manual_seed(5)).to(DEV, torch.int32)
    logits = {}
    for dt in ("mxfp4", "bf16"):
        st = build_device_stage(model, sd, 0, n - 1, True, True, DEV, dtype=dt, max_batch=2, max_seq=128)
        pos = torch.zeros(2, dtype=torch.int32, device=DEV)
        pre = st.step(ids[:, :40].contiguous(), pos, 2, 40, last_only=False).probs.float().clone()
        dec = st.step(ids[:, 40:].contiguous(), pos + 40, 2, 1).probs.float().clone()
        logits[dt] = (pre, dec)
        if dt == "mxfp4":
            for L in st.layers:
                assert all(isinstance(w, Mxfp4Weight) for w in (L.w_qkv.w, L.w_o, L.w_up.w, L.w_down))
                assert L.w_qkv.ws is None and L.w_up.ws is None and L.w_o_s is None and L.w_down_s is None
    for got, ref in zip(logits["mxfp4"], logits["bf16"]):
        assert _rel(got, ref) < 3e-2, _rel(got, ref)
