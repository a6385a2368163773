"""``dnn_gemm_w4_mn``: the MXFP4 W4A16 GEMM of 65..256-row decode steps on narrow projections (an M x N grid of
workgroups whose waves split K) against fp64 references, and the mxfp4 stage's decode step on it (MI355X only)."""
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
@pytest.mark.parametrize("N,K", [(40, 128), (40, 160), (48, 384), (544, 1152)])
@pytest.mark.parametrize("M", [65, 80, 128, 129, 256])
def test_gemm_w4_mn_exact(M, N, K, act):
    """The fixture of test_gemm_w4_mid_exact (integer activations in [-3, 3] on strided rows, weights and bias in
    quarters, integer residual): every partial sum is a multiple of 0.25 below 2^16, so fp32 is exact in any order
    (the parity split included) and the output is bf16(fp64 reference) bit for bit.  K = 128: the odd-parity waves
    add nothing; 160: a partial odd chunk; 384: an odd chunk count; N = 40 / 48: a column block of one real tile."""
    from distributed_neural_networks_amd.ops.w4 import dequantize, linear_w4
    w = _packed(N, K)
    g = torch.Generator().manual_seed(M)
    x = torch.randint(-3, 4, (M, K + 64), generator=g).to(DEV, BF)[:, :K]
    bias = (torch.randint(-8, 9, (N,), generator=g) * 0.25).to(DEV)
    R = torch.randint(-4, 5, (M, N), generator=g).to(DEV, BF)
    out = torch.zeros(M, N, device=DEV, dtype=BF)
    linear_w4(x, w, bias, act, R, out, mn=True)
    y = x.double() @ dequantize(w).double().t() + bias.double()
    y = (y.clamp_min(0) if act else y) + R.double()
    assert torch.equal(out, y.to(BF))


@pytest.mark.parametrize("norm,act", [(1, 0), (1, 3), (2, 0), (2, 2)])
@pytest.mark.parametrize("M", [65, 256])
def test_gemm_w4_mn_norm_epilogues(M, norm, act):
    """The cases, fp64 algebra and bound (rel < 1e-2) of test_gemm_w4_mid_norm_epilogues."""
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
    linear_w4(x, f.w, f.bias, act, R, out, norm, f.colsum, 1e-5, mn=True)
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
    print(f"w4 mn norm {norm} act {act} M {M}: rel {err:.3e}")
    assert err < 1e-2, err


@pytest.mark.parametrize("key,val", [("M", 0), ("M", 257), ("Ws", 0), ("K", 48), ("A", "+2")])
def test_gemm_w4_mn_rejections(key, val):
    """The five cases of test_gemm_w4_mid_rejections: the mid kernel's return code, nothing launched (``out``
    keeps its content)."""
    from distributed_neural_networks_amd.ops._lib import lib, stream_ptr
    w = _packed(40, 128)
    x = torch.ones(264, 136, device=DEV, dtype=BF)
    out = torch.full((264, 40), 7.0, device=DEV, dtype=BF)
    a = dict(A=x.data_ptr(), lda=136, Wq=w.q.data_ptr(), Ws=w.scales.data_ptr(), C=out.data_ptr(), ldc=40, bias=0, R=0,
             ldr=0, M=80, N=40, K=128, act=0, norm=0, colsum=0, eps=1e-5, st=stream_ptr())
    a[key] = a[key] + 2 if val == "+2" else val
    rc = lib().gemm_w4_mn(**a)
    assert rc < 0 and rc == lib().gemm_w4_mid(**a)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_mxfp4_stage_decode_80_rows_mn():
    """A GPT-2 small middle stage (one layer, no vocabulary tables) on a checkpoint snapped to the MXFP4 grid: an
    80-row decode step after a 4-token prefill leaves the expand scratch untouched (every projection runs on the
    codes; before dnn_gemm_w4_mn these shapes expanded into it), lies within 3e-2 of the bf16 stage, and one replay
    captured in a graph is bit-equal to the eager step (the reduction order is fixed)."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.ops.w4 import dequantize, quantize_weight_mxfp4, w4_mn_ok
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    if not w4_mn_ok(80, 2304, 768):
        pytest.skip("w4_mn_ok(80, 2304, 768) is False: the measurement left GPT-2 small's shapes off the mn kernel")
    sd = ckpt.random_stage_state_dict("gpt2", 1, 1, False, False, 11)
    for k, v in sd.items():
        if k.split(".")[0] == "h" and v.dim() == 2:
            sd[k] = dequantize(quantize_weight_mxfp4(v, "cpu"))
    B = 80
    x = (torch.randn(B, 5, 768, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV, BF)
    nxt, pos4 = x[:, 4:].contiguous(), torch.full((B,), 4, dtype=torch.int32, device=DEV)
    dec = {}
    for dt in ("mxfp4", "bf16"):
        st = build_device_stage("gpt2", sd, 1, 1, False, False, DEV, dtype=dt, max_batch=B, max_seq=128)
        st.step(x[:, :4].contiguous(), torch.zeros(B, dtype=torch.int32, device=DEV), B, 4)
        if dt == "mxfp4":
            st.w4_scratch.fill_(7.0)
        dec[dt] = st.step(nxt, pos4, B, 1).float().clone()
        if dt == "mxfp4":
            assert bool((st.w4_scratch == 7.0).all())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cap = st.step(nxt, pos4, B, 1)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(cap.float(), dec[dt])
    assert _rel(dec["mxfp4"], dec["bf16"]) < 3e-2, _rel(dec["mxfp4"], dec["bf16"])
