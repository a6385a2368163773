"""The MXFP4 vocabulary head on the device: ``dnn_gemm_w4_head`` / ``head_w4`` against fp64 references, and the
``mxfp4_head="mxfp4"`` stage against the torch golden (MI355X only)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
I32 = torch.int32


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _first_argmax(y):
    """argmax with ties to the smallest index."""
    n = y.shape[1]
    return torch.where(y == y.max(1, keepdim=True).values, torch.arange(n, device=y.device), n).min(1).values.to(I32)


def _part(M):
    from distributed_neural_networks_amd.ops.gemm import HEAD_PART_PER_ROW
    return torch.zeros(2 * HEAD_PART_PER_ROW * M, dtype=I32, device=DEV)


@pytest.mark.parametrize("N,K", [(40, 128), (40, 160), (544, 1152), (65584, 128), (48, None)])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_gemm_w4_head_exact(M, N, K):
    """The grids of test_gemm_w4_exact (integer activations in [-3, 3], weights k / 4 with |w| <= 12, bias in
    quarters): every partial sum is a multiple of 0.25 below 4640 * 36 < 2^18, exact in fp32 in any order, so the
    logits are bf16(fp64 reference) bit for bit.  K = None: 32 past one LDS pass at this M (36 // ceil(M / 16)
    chunks of 128).  Rows 5 and N - 3 (first and last tile) hold +12 everywhere, rows 17 and min(145, N - 7) hold
    -12, with equal biases; activation row 0 is all 3 and row 1 all -3, so their maxima are exact ties across
    tiles, waves and workgroups."""
    from distributed_neural_networks_amd.ops.gemm import FoldedLinear
    from distributed_neural_networks_amd.ops.w4 import Mxfp4Weight, dequantize, head_w4, pack_mxfp4
    K = K or 128 * (36 // -(-M // 16)) + 32
    g = torch.Generator().manual_seed(M)
    codes = torch.randint(0, 16, (N, K), generator=g)
    exps = torch.randint(126, 129, (N, K // 32), generator=g)
    dup = ((5, N - 3, 7), (17, min(145, N - 7), 15))
    bias = torch.randint(-8, 9, (N,), generator=g) * 0.25
    for a, b, code in dup:
        codes[[a, b]], exps[[a, b]], bias[b] = code, 128, bias[a]
    x = torch.randint(-3, 4, (M, K + 64), generator=g)
    x[0], x[1:2] = 3, -3
    wc = pack_mxfp4(codes, exps)
    y = (x[:, :K].double() @ dequantize(wc).double().t() + bias.double()).to(BF)
    want = _first_argmax(y.float())
    assert int((y.float() == y.float().max(1, keepdim=True).values).sum(1).max()) >= 2  # real ties
    assert int(want[0]) == 5 and (M == 1 or int(want[1]) == 17)

    f = FoldedLinear(Mxfp4Weight(wc.q.to(DEV), wc.scales.to(DEV), N, K), bias.to(DEV), None, 0, 0.0)
    xd = x.to(DEV, BF)[:, :K]
    ldc = -(-N // 8) * 8 + 8
    bufs = [torch.full((M, ldc), 7.0, device=DEV, dtype=BF) for _ in range(2)]
    ids = torch.full((M,), -1, dtype=I32, device=DEV)
    head_w4(xd, f, bufs[0][:, :N], _part(M), ids)
    head_w4(xd, f, bufs[1][:, :N])
    assert torch.equal(bufs[0][:, :N].cpu(), y) and bool((bufs[0][:, N:] == 7.0).all())
    assert torch.equal(ids.cpu(), want)
    assert torch.equal(bufs[1], bufs[0])


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("M", [1, 64])
def test_gemm_w4_head_norm(M, norm):
    """Folded RMSNorm / LayerNorm (+ the bias LayerNorm's beta folds into) against the same algebra in fp64 on
    the dequantised weight: the measure and bound of test_gemm_w4_norm_epilogues.  The ids are the first argmax
    of the logits the kernel itself wrote."""
    from distributed_neural_networks_amd.ops.gemm import fold_norm
    from distributed_neural_networks_amd.ops.w4 import dequantize, head_w4
    torch.manual_seed(11)
    N, K = 544, 1152
    x = (torch.randn(M, K, device=DEV) + 0.3).bfloat16()
    W = torch.randn(N, K, device=DEV) / math.sqrt(K)
    gamma = torch.rand(K, device=DEV) + 0.5
    beta = torch.randn(K, device=DEV) * 0.1 if norm == 2 else None
    f = fold_norm(W, gamma, beta, None, norm == 1, 1e-5, DEV, quant="mxfp4")
    out = torch.empty(M, N, device=DEV, dtype=BF)
    ids = torch.full((M,), -1, dtype=I32, device=DEV)
    head_w4(x, f, out, _part(M), ids)
    xd = x.double()
    mean = xd.mean(1, keepdim=True) if norm == 2 else torch.zeros_like(xd[:, :1])
    var = xd.pow(2).mean(1, keepdim=True) - mean ** 2
    y = xd @ dequantize(f.w).double().t()
    if norm == 2:
        y = y - mean * f.colsum.double()[None, :]
    y = torch.rsqrt(var + 1e-5) * y
    if f.bias is not None:
        y = y + f.bias.double()
    err = _rel(out, y)
    print(f"w4 head norm {norm} M {M}: rel {err:.3e}")
    assert err < 1e-2, err
    assert torch.equal(ids, _first_argmax(out.float()))


@pytest.mark.parametrize("key,val,rc", [("A", 0, -1), ("Wq", 0, -1), ("Ws", 0, -1), ("C", 0, -1), ("norm", 2, -1),
                                        ("M", 0, -2), ("M", 65, -2), ("K", 48, -3), ("N", 0, -3), ("norm", 3, -3),
                                        ("part_cap", 0, -3), ("ldc", 32, -4), ("lda", 120, -4), ("A", "+2", -5),
                                        ("C", "+2", -5), ("lda", 132, -5), ("ldc", 44, -5)])
def test_gemm_w4_head_rejections(key, val, rc):
    """The negative returns listed in api.h; nothing is launched, so ``out`` keeps its content."""
    from distributed_neural_networks_amd.ops._lib import lib, stream_ptr
    from distributed_neural_networks_amd.ops.w4 import pack_mxfp4
    w = pack_mxfp4(torch.zeros(40, 128, dtype=torch.uint8, device=DEV),
                   torch.full((40, 4), 127, dtype=torch.uint8, device=DEV))
    x = torch.ones(64, 136, device=DEV, dtype=BF)
    out = torch.full((64, 48), 7.0, device=DEV, dtype=BF)
    part = _part(64)
    a = dict(A=x.data_ptr(), lda=136, Wq=w.q.data_ptr(), Ws=w.scales.data_ptr(), C=out.data_ptr(), ldc=48, bias=0,
             M=4, N=40, K=128, norm=0, colsum=0, eps=1e-5, part=part.data_ptr(), part_cap=256, st=stream_ptr())
    a[key] = a[key] + 2 if val == "+2" else val
    assert lib().gemm_w4_head(**a) == rc
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _snapped(model):
    """A tiny checkpoint (norm gains 1, biases 0) whose layer projections and head lie on the MXFP4 grid, its
    fp32 torch golden, and the layer count.  A tied wte keeps its own values (the embedding stays bf16)."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import build_golden_stage, model_info
    from distributed_neural_networks_amd.ops.w4 import dequantize, quantize_weight_mxfp4
    n = model_info(model).num_layers
    sd = dict(ckpt.random_stage_state_dict(model, 0, n - 1, True, True, 11))
    for k, v in sd.items():
        if (k.split(".")[0] in ("h", "layers") and v.dim() == 2) or k == "lm_head.weight":
            sd[k] = dequantize(quantize_weight_mxfp4(v, "cpu"))
    gold = build_golden_stage(model, 0, n - 1, True, True)
    gold.load_state_dict(sd)
    return sd, gold.eval(), n


def _gold_last(gold, seq):
    with torch.no_grad():
        return gold(seq.cpu().long())[:, -1].float()


@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_mxfp4_head_stage(model):
    """Last stage with mxfp4_head="mxfp4": a 6-token prefill and 4 greedy decode steps at 8 rows.  The logits stay
    within 3e-2 (the bound of test_mxfp4_stage_matches_bf16_stage) of the golden that holds the same dequantised
    layer and head weights, the tokens are the first argmax of the stage's own logits, a decode step captured in
    a graph is bit-equal to the eager step, and a sampling stage (logits-only head) writes the same logits."""
    from distributed_neural_networks_amd.ops.w4 import Mxfp4Weight
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd, gold, n = _snapped(model)
    B, T = 8, 6
    kw = dict(dtype="mxfp4", max_batch=B, max_seq=64, mxfp4_head="mxfp4")
    st = build_device_stage(model, sd, 0, n - 1, True, True, DEV, **kw)
    assert isinstance(st.w_head.w, Mxfp4Weight)
    seq = torch.randint(0, 512, (B, T), generator=torch.Generator().manual_seed(5)).to(DEV, I32)
    pos = torch.zeros(B, dtype=I32, device=DEV)
    o = st.step(seq, pos, B, T)
    pre = o.probs.clone()
    for step in range(5):
        rel = _rel(o.probs.cpu(), _gold_last(gold, seq))
        print(f"{model} step {step}: rel {rel:.3e}")
        assert rel < 3e-2, rel
        assert torch.equal(o.pred, _first_argmax(o.probs.float()))
        if step == 4:
            break
        nxt = o.pred.clone().view(B, 1)
        seq = torch.cat([seq, nxt], 1)
        o = st.step(nxt, pos + (T + step), B, 1)
    eager, p3, g = o.probs.clone(), pos + (T + 3), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = st.step(nxt, p3, B, 1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.probs, eager) and torch.equal(cap.pred, o.pred)
    smp = build_device_stage(model, sd, 0, n - 1, True, True, DEV, temperature=0.8, seed=1, **kw)
    got = smp.step(seq[:, :T].contiguous(), pos, B, T).probs
    assert bool(torch.isfinite(got.float()).all()) and torch.equal(got, pre)


def test_mxfp4_head_65_rows_and_forward():
    """gpt2-tiny: 80 decode rows (the head on dnn_gemm_w4_mid) and a forward of (3, 100) (all-position logits of
    300 rows: the head expanded into the scratch), within 3e-2 of the same golden."""
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd, gold, n = _snapped("gpt2-tiny")
    B = 80
    st = build_device_stage("gpt2-tiny", sd, 0, n - 1, True, True, DEV, dtype="mxfp4", max_batch=B, max_seq=128,
                            max_tokens=B * 4, mxfp4_head="mxfp4")
    ids = torch.randint(0, 512, (B, 100), generator=torch.Generator().manual_seed(6)).to(DEV, I32)
    st.step(ids[:, :4].contiguous(), torch.zeros(B, dtype=I32, device=DEV), B, 4)
    dec = st.step(ids[:, 4:5].contiguous(), torch.full((B,), 4, dtype=I32, device=DEV), B, 1).probs
    rel = _rel(dec.cpu(), _gold_last(gold, ids[:, :5]))
    with torch.no_grad():
        full = gold(ids[:3].cpu().long()).float()
    rel_f = _rel(st.forward(ids[:3]).probs.cpu(), full)
    print(f"80 decode rows: rel {rel:.3e}; forward (3, 100): rel {rel_f:.3e}")
    assert rel < 3e-2 and rel_f < 3e-2, (rel, rel_f)


def test_mxfp4_head_bf16_is_neutral():
    """mxfp4_head="bf16" is the stage built without the argument: bit-equal logits, a bf16 head, the same scratch."""
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    sd, _, n = _snapped("gpt2-tiny")
    ids = torch.randint(0, 512, (3, 8), generator=torch.Generator().manual_seed(7)).to(DEV, I32)
    got = []
    for kw in ({}, {"mxfp4_head": "bf16"}):
        st = build_device_stage("gpt2-tiny", sd, 0, n - 1, True, True, DEV, dtype="mxfp4", max_batch=3, max_seq=64, **kw)
        assert isinstance(st.w_head.w, torch.Tensor) and not st.head_w4
        got.append((st.step(ids, torch.zeros(3, dtype=I32, device=DEV), 3, 8).probs.clone(), st.w4_scratch.numel()))
    assert torch.equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
