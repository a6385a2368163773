"""Device sampler with top-p / min-p and the fused decode step tail
(csrc/kernels/sample_filter.hip) — MI355X only."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 48
SEED = 1234
CASES = [(512, 0, 1.0, 0.5),        # NV = 1
         (1000, 0, 1.0, 0.9),       # N not a multiple of 8, ld 1024
         (50257, 0, 1.0, 0.9),      # pad path
         (50257, 40, 0.7, 0.95),    # top-k and top-p both active
         (128256, 0, 1.3, 0.9)]     # 512-thread instantiation


def _key(x_bf16):
    """Order-preserving 16-bit key of a bf16 tensor (written out here: the
    threshold test does not lean on the mirror)."""
    u = x_bf16.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    return torch.where((u & 0x8000) != 0, (~u) & 0xFFFF, u | 0x8000)


def _logits(N):
    torch.manual_seed(3)
    ld = -(-N // 64) * 64
    return (torch.randn(M, ld, device=DEV) * 3).bfloat16()


def _step():
    return torch.arange(M, device=DEV, dtype=torch.int32) * 7


@functools.lru_cache(maxsize=None)
def _run(N, k, T, top_p, min_p=0.0):
    """One device call per case, shared by the tests: (bf16 logits (M, N) on the
    host, tokens, final key thresholds)."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    logits = _logits(N)
    out = torch.full((M,), -1, device=DEV, dtype=torch.int32)
    thr = torch.full((M,), -1, device=DEV, dtype=torch.int32)
    Tops.sample_rows(logits, out, N, T, k, top_p, min_p, seed=SEED, step=_step(), thr_out=thr)
    torch.cuda.synchronize()
    return logits[:, :N].cpu(), out.cpu(), thr.cpu()


@pytest.mark.parametrize("N,k,T,top_p", CASES)
def test_nucleus_threshold_two_sided(N, k, T, top_p):
    """With t the device's threshold key, in fp64 on the host:
    mass(key >= t) >= top_p - eps (the nucleus is large enough),
    mass(key > t) < top_p + eps (and minimal: dropping the boundary key falls
    short), the token is in it, and inside the top-k.  eps = 1e-4: the fp32 sum
    of <= 128 terms per lane plus the reduction tree is good to ~150 x 2^-24 ~
    1e-5 relative, the fast exponential adds a few ulp; 10x headroom over that
    is still below the mass of one key step at the boundary (~1e-3 of Z at
    N = 50257).  A kernel that ignores top_p fails the second bound by ~0.1."""
    x, out, thr = _run(N, k, T, top_p)
    eps = 1e-4
    keys = _key(x)
    xd = x.double()
    z = xd / T
    if k:
        kth = xd.topk(k, dim=1).values[:, -1:]
        z = torch.where(xd >= kth, z, torch.full_like(z, float("-inf")))
    p = torch.softmax(z, dim=1)
    t = thr.long()[:, None]
    m_ge = torch.where(keys >= t, p, torch.zeros_like(p)).sum(1)
    m_gt = torch.where(keys > t, p, torch.zeros_like(p)).sum(1)
    print(f"N={N} k={k}: min mass(>=t)-top_p {float((m_ge - top_p).min()):.3e}, "
          f"max mass(>t)-top_p {float((m_gt - top_p).max()):.3e}, kept {int((keys >= t).sum(1).min())}.."
          f"{int((keys >= t).sum(1).max())}")
    assert bool((out >= 0).all()) and bool((out < N).all())
    assert bool((m_ge >= top_p - eps).all()), (m_ge - top_p).min()
    assert bool((m_gt < top_p + eps).all()), (m_gt - top_p).max()
    kj = keys.gather(1, out[:, None].long())
    assert bool((kj >= t).all())
    if k:
        assert bool((xd.gather(1, out[:, None].long()) >= kth).all())


@pytest.mark.parametrize("N,k,T,top_p", CASES)
def test_draw_matches_mirror_at_device_threshold(N, k, T, top_p):
    from distributed_neural_networks_amd.runtime.sampling import sample_ref
    x, out, thr = _run(N, k, T, top_p)
    ref = sample_ref(x, T, k, top_p, seed=SEED, step=_step(), thr=thr)
    agree = (out == ref).float().mean().item()
    assert agree >= 0.95, agree  # __logf vs log: rare near-ties may flip


def test_min_p_threshold_is_bit_exact():
    from distributed_neural_networks_amd.runtime.sampling import sample_ref
    N, T, min_p = 50257, 0.7, 0.05
    x, out, thr = _run(N, 0, T, 1.0, min_p)
    ref, rthr = sample_ref(x, T, 0, 1.0, min_p, seed=SEED, step=_step(), return_thr=True)
    assert torch.equal(thr, rthr)
    assert (out == ref).float().mean().item() >= 0.95
    # first principles: kept <=> (x - x_max) / T >= log(min_p), in fp32
    xf = x.float()
    it = torch.tensor(1.0) / torch.tensor(T)
    keep = (xf - xf.max(1, keepdim=True).values) * it >= torch.log(torch.tensor(min_p))
    assert torch.equal(_key(x) >= thr.long()[:, None], keep)
    assert 1 < int(keep.sum(1).max()) < N  # the filter bites, and is no argmax


@pytest.mark.parametrize("N,k,T", [(50257, 40, 0.7), (128256, 0, 0.5)])
def test_filters_off_equal_sample_topk(N, k, T):
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    logits = _logits(N)
    a = torch.empty(M, device=DEV, dtype=torch.int32)
    b = torch.empty(M, device=DEV, dtype=torch.int32)
    Tops.sample_topk(logits, a, N, T, k, seed=SEED, step=_step())
    Tops.sample_rows(logits, b, N, T, k, 1.0, 0.0, seed=SEED, step=_step())
    assert torch.equal(a, b)


def test_fused_tail():
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    torch.manual_seed(5)
    Mr, N, L, G = 5, 1000, 16, 0x5A5A5A5A
    logits = (torch.randn(Mr, 1024, device=DEV) * 3).bfloat16()
    old = torch.tensor([0, 3, 7, 7, 15], dtype=torch.int32)
    pos = old.to(DEV)
    guard = torch.full((Mr + 2, L), G, device=DEV, dtype=torch.int32)
    hist = guard[1:Mr + 1]  # rows 1..5 of the guard buffer: out-of-range writes land in a guard row or column
    hist.zero_()
    out = torch.full((Mr,), -1, device=DEV, dtype=torch.int32)
    also = torch.full((Mr,), -2, device=DEV, dtype=torch.int32)
    args = dict(top_k=20, top_p=0.9, min_p=0.01, seed=9)
    Tops.sample_rows(logits, out, N, 0.8, also=also, advance=pos, hist=hist, **args)
    unfused = torch.empty(Mr, device=DEV, dtype=torch.int32)
    Tops.sample_rows(logits, unfused, N, 0.8, step=old.to(DEV), **args)
    assert torch.equal(out, also) and torch.equal(out, unfused)
    assert torch.equal(pos.cpu(), old + 1)
    want = torch.zeros(Mr, L, dtype=torch.int32)
    want[torch.arange(Mr), old.long()] = out.cpu()
    assert torch.equal(hist.cpu(), want)
    # second step: row 4 is at position 16 = L, outside the history: nothing is written for it
    out2 = torch.empty(Mr, device=DEV, dtype=torch.int32)
    Tops.sample_rows(logits, out2, N, 0.8, also=also, advance=pos, hist=hist, **args)
    assert torch.equal(pos.cpu(), old + 2)
    want[torch.arange(4), old[:4].long() + 1] = out2.cpu()[:4]
    assert torch.equal(hist.cpu(), want)
    assert bool((guard[0] == G).all()) and bool((guard[Mr + 1] == G).all())


def test_deterministic():
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    N, k, T, top_p = 50257, 40, 0.7, 0.95
    _, out0, thr0 = _run(N, k, T, top_p)
    logits = _logits(N)
    for _ in range(3):
        out = torch.empty(M, device=DEV, dtype=torch.int32)
        thr = torch.empty(M, device=DEV, dtype=torch.int32)
        Tops.sample_rows(logits, out, N, T, k, top_p, seed=SEED, step=_step(), thr_out=thr)
        assert torch.equal(out.cpu(), out0) and torch.equal(thr.cpu(), thr0)


@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_decode_ring_sampled_tokens(model):
    """Sampled decoding (top-k + top-p) gives the same tokens eagerly, with
    single-step graphs, with K = 4 steps per graph (fused tail, device token
    history) and with the unfused three-launch tail."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    n = model_info(model).num_layers
    ranges = [(0, n // 2 - 1), (n // 2, n - 1)]
    Mb, B, T, steps, K = 2, 2, 16, 9, 4
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 9, nontrivial=True)
           for i, (a, b) in enumerate(ranges)]
    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(0, model_info(model).cfg.vocab_size, (B, T), generator=g) for _ in range(Mb)]

    def generate(graphs, ms):
        st = [TransformerStage(model, sds[i], a, b, i == 0, i == 1, DEV, max_batch=Mb * B,
                               max_seq=T + steps + K + 2, temperature=0.8, top_k=20, seed=5, top_p=0.9)
              for i, (a, b) in enumerate(ranges)]
        ring = DecodeRing(st, RingLinks(), 1, Mb, B, use_graphs=graphs, multi_step=ms)
        toks = ring.generate(prompts, T, steps)
        torch.cuda.synchronize()
        return toks, ring

    ref, _ = generate(False, 0)
    assert ref.shape == (Mb * B, steps)
    one, ring1 = generate(True, 0)
    assert ring1.graph_k is None and ring1.hist is not None
    multi, ringk = generate(True, K)
    assert ringk.graph_k is not None and ringk.hist is not None
    assert Tops.SAMPLE_FUSED_TAIL
    Tops.SAMPLE_FUSED_TAIL = False
    try:
        unfused, ringu = generate(True, 0)
        assert ringu.hist is None
    finally:
        Tops.SAMPLE_FUSED_TAIL = True
    assert torch.equal(one, ref) and torch.equal(multi, ref) and torch.equal(unfused, ref)


def test_rejections_and_empty_batch():
    from distributed_neural_networks_amd.ops import _lib
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    logits = _logits(512)
    out = torch.full((M,), -1, device=DEV, dtype=torch.int32)
    for kw in ({"top_p": 0.0}, {"top_p": 1.5}, {"min_p": 1.0}, {"temperature": 0.0}):
        a = dict(temperature=1.0)
        a.update(kw)
        with pytest.raises((ValueError, RuntimeError)):
            Tops.sample_rows(logits, out, 512, **a)
    # the C entry point rejects them too (-1), and a history without positions
    p, o, s = logits.data_ptr(), out.data_ptr(), _lib.stream_ptr()
    lib = _lib.lib()
    assert lib.sample_rows(p, 512, M, 512, o, 1.0, 0, 0.0, 0.0, 1, 0, s) == -1
    assert lib.sample_rows(p, 512, M, 512, o, 1.0, 0, float("nan"), 0.0, 1, 0, s) == -1
    assert lib.sample_rows(p, 512, M, 512, o, 1.0, 0, 1.0, 1.0, 1, 0, s) == -1
    assert lib.sample_rows(p, 512, M, 512, o, 0.0, 0, 1.0, 0.0, 1, 0, s) == -1
    assert lib.sample_rows(p, 508, M, 508, o, 1.0, 0, 1.0, 0.0, 1, 0, s) == -1
    assert lib.sample_rows(p, 512, M, 512, o, 1.0, 0, 1.0, 0.0, 1, 0, s, hist=o, hist_ld=4) == -1
    assert lib.sample_rows(p, 512, M, 1 << 18, o, 1.0, 0, 1.0, 0.0, 1, 0, s) == -2
    Tops.sample_rows(logits[:0], out, 512, 1.0, top_p=0.9)  # M = 0: no launch
    torch.cuda.synchronize()
    assert bool((out == -1).all())
