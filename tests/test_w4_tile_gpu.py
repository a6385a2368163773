"""``dnn_gemm_w4_tile``: the MXFP4 W4A16 tile GEMM for any number of rows (128 x 128 output blocks over the whole of K)
against fp64 references, and the ``mxfp4_prefill: "w4a16"`` stage that runs it wherever the other modes expand the
weight (MI355X only; the config test at the end needs no GPU)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from test_w4_mid_gpu import _snapped  # a tiny checkpoint whose layer projections lie on the MXFP4 grid
from test_w4_mn_gpu import _packed, _rel

gpu = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _tile(x, w, bias=None, act=0, R=None, out=None, norm=0, colsum=None, M=None):
    """One ``dnn_gemm_w4_tile`` launch through the binding (``linear_w4(tile=True)`` keeps M <= 64 on dnn_gemm_w4)."""
    from distributed_neural_networks_amd.ops._lib import lib, ptr, stream_ptr
    rc = lib().gemm_w4_tile(ptr(x), x.stride(0), ptr(w.q), ptr(w.scales), ptr(out), out.stride(0), ptr(bias), ptr(R),
                            0 if R is None else R.stride(0), x.shape[0] if M is None else M, w.n, w.k, act, norm,
                            ptr(colsum), 1e-5, stream_ptr())
    assert rc == 0, rc
    return out


def _exact(M, N, K, act, alias=False):
    from distributed_neural_networks_amd.ops.w4 import dequantize
    w = _packed(N, K)
    g = torch.Generator().manual_seed(M)
    x = torch.randint(-3, 4, (M, K + 64), generator=g).to(DEV, BF)[:, :K]
    bias = (torch.randint(-8, 9, (N,), generator=g) * 0.25).to(DEV)
    R = torch.randint(-4, 5, (M, N), generator=g).to(DEV, BF)
    y = x.double() @ dequantize(w).double().t() + bias.double()
    y = (y.clamp_min(0) if act else y) + R.double()
    out = R if alias else torch.zeros(M, N, device=DEV, dtype=BF)
    _tile(x, w, bias, act, R, out)
    assert torch.equal(out, y.to(BF))


@gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("N,K", [(40, 160), (136, 384), (544, 1152)])
@pytest.mark.parametrize("M", [1, 129, 257, 400])
def test_gemm_w4_tile_exact(M, N, K, act):
    """The fixture of test_gemm_w4_mn_exact (fp32 is exact in any order: the output is bf16(fp64 reference) bit for
    bit).  BM = BN = 128.  M: one partial block, the block edge + 1, three blocks with a one-row last block, a
    partial fourth.  (40, 160): a column block of one real tile of three, a partial chunk; (136, 384): a second
    column block of one tile, an odd chunk count (both LDS stages); (544, 1152): five column blocks, nine chunks."""
    _exact(M, N, K, act)


@gpu
def test_gemm_w4_tile_aliased_residual():
    """R = C, as the residual projections pass it: each lane reads the residual values it overwrites."""
    _exact(257, 136, 384, 0, alias=True)


@gpu
@pytest.mark.parametrize("norm,act", [(1, 0), (1, 3), (2, 0), (2, 2)])
@pytest.mark.parametrize("M", [257, 400])
def test_gemm_w4_tile_norm_epilogues(M, norm, act):
    """The cases, fp64 algebra and bound (rel < 1e-2) of test_gemm_w4_mn_norm_epilogues."""
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
    linear_w4(x, f.w, f.bias, act, R, out, norm, f.colsum, 1e-5, tile=True)
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
    print(f"w4 tile norm {norm} act {act} M {M}: rel {err:.3e}")
    assert err < 1e-2, err


@gpu
@pytest.mark.parametrize("key,val", [("M", 0), ("Ws", 0), ("K", 48), ("A", "+2"), ("M", 257)])
def test_gemm_w4_tile_rejections(key, val):
    """A negative return launches nothing (``out`` keeps its sentinel); 257 rows, which dnn_gemm_w4_mid rejects,
    are accepted."""
    from distributed_neural_networks_amd.ops._lib import lib, stream_ptr
    w = _packed(40, 128)
    x = torch.ones(264, 136, device=DEV, dtype=BF)
    out = torch.full((264, 40), 7.0, device=DEV, dtype=BF)
    a = dict(A=x.data_ptr(), lda=136, Wq=w.q.data_ptr(), Ws=w.scales.data_ptr(), C=out.data_ptr(), ldc=40, bias=0, R=0,
             ldr=0, M=80, N=40, K=128, act=0, norm=0, colsum=0, eps=1e-5, st=stream_ptr())
    a[key] = a[key] + 2 if val == "+2" else val
    rc = lib().gemm_w4_tile(**a)
    torch.cuda.synchronize()
    if val == 257:
        # (the rows of x are equal, so the 257 written rows are too)
        assert rc == 0 and not torch.equal(out[0], out[257]) and bool((out[:257] == out[0]).all())
        assert bool((out[257:] == 7.0).all())
    else:
        assert rc < 0 and bool((out == 7.0).all())


@gpu
@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_mxfp4_w4a16_prefill_matches_bf16_prefill(model):
    """LayerNorm + GELU and RMS + RoPE + SwiGLU + GQA at (3, 90) = 270 rows (three M blocks, the last of 14 rows),
    with the MXFP4 head and all-position logits (270 head rows): the "w4a16" stage holds no expand scratch, lies
    within 3e-2 of the "bf16"-prefill stage of the same snapped checkpoint, and repeats bit for bit."""
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd, n = _snapped(model)
    ids = torch.randint(0, 512, (3, 90), generator=torch.Generator().manual_seed(5)).to(DEV, torch.int32)
    pos, lg = torch.zeros(3, dtype=torch.int32, device=DEV), {}
    for pf in ("w4a16", "bf16"):
        st = build_device_stage(model, sd, 0, n - 1, True, True, DEV, dtype="mxfp4", max_batch=3, max_seq=128,
                                mxfp4_prefill=pf, mxfp4_head="mxfp4")
        lg[pf] = st.step(ids, pos, 3, 90, last_only=False).probs.float().clone()
        if pf == "w4a16":
            assert st.w4_scratch is None and st.q8 is None and st.sx8 is None
            assert torch.equal(st.step(ids, pos, 3, 90, last_only=False).probs.float(), lg[pf])
    rel = _rel(lg["w4a16"], lg["bf16"])
    print(f"{model} w4a16 vs bf16 prefill: rel {rel:.3e}")
    assert rel < 3e-2, rel


@gpu
def test_mxfp4_w4a16_stage_decode_272_rows():
    """A GPT-2 small middle stage of one layer (as test_mxfp4_stage_decode_80_rows_mn) at B = 272: a decode step
    above 256 rows after a 4-token prefill (1088 rows), both on the tile kernel, lies within 3e-2 of the bf16 stage,
    and three replays of its captured graph are bit-equal to the eager step."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.ops.w4 import dequantize, quantize_weight_mxfp4
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd = ckpt.random_stage_state_dict("gpt2", 1, 1, False, False, 11)
    for k, v in sd.items():
        if k.split(".")[0] == "h" and v.dim() == 2:
            sd[k] = dequantize(quantize_weight_mxfp4(v, "cpu"))
    B = 272
    x = (torch.randn(B, 5, 768, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV, BF)
    nxt, pos4 = x[:, 4:].contiguous(), torch.full((B,), 4, dtype=torch.int32, device=DEV)
    dec = {}
    for dt, kw in (("mxfp4", {"mxfp4_prefill": "w4a16"}), ("bf16", {})):
        st = build_device_stage("gpt2", sd, 1, 1, False, False, DEV, dtype=dt, max_batch=B, max_seq=128, **kw)
        st.step(x[:, :4].contiguous(), torch.zeros(B, dtype=torch.int32, device=DEV), B, 4)
        dec[dt] = st.step(nxt, pos4, B, 1).float().clone()
        if dt == "mxfp4":
            assert st.w4_scratch is None
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cap = st.step(nxt, pos4, B, 1)
            for _ in range(3):
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(cap.float(), dec[dt])
    rel = _rel(dec["mxfp4"], dec["bf16"])
    print(f"gpt2 w4a16 decode 272 rows vs bf16: rel {rel:.3e}")
    assert rel < 3e-2, rel


def test_mxfp4_prefill_w4a16_config():
    """``mxfp4_prefill: "w4a16"`` resolves, in the shipped config too."""
    from distributed_neural_networks_amd.config import load_node
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                       "gpt2_4stage_1gpu_mxfp4_w4a16.json")
    p = load_node(cfg, "node1").pipeline
    assert p.dtype == "mxfp4" and p.mxfp4_prefill == "w4a16"
