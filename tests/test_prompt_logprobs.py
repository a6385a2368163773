"""Prompt log-probabilities without a GPU: the config key ``prompt_logprobs``, the
torch mirror of the kernel (runtime/sampling.py prompt_logprobs_ref), a
``TorchStage`` ring, and the random kernel cases' share of near-tie rows."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(base="gpt2_4stage_1gpu_prompt_logprobs.json", **kw):
    c = json.load(open(os.path.join(ROOT, "configs", base)))
    c.update(kw)
    return c


def test_config_key_resolves():
    from distributed_neural_networks_amd.config import parse_pipeline
    assert parse_pipeline(_cfg()).prompt_logprobs == 1
    assert parse_pipeline(_cfg(prompt_logprobs=0)).prompt_logprobs == 0
    assert parse_pipeline(_cfg(dtype="mxfp4")).prompt_logprobs == 1  # MXFP4 blocks under the bf16 head


@pytest.mark.parametrize("kw,msg", [
    (dict(prompt_logprobs=2), "only 1 exists"), (dict(prompt_logprobs=-1), "must be 0 or 1"),
    (dict(prompt_logprobs=True), "must be 0 or 1"), (dict(prompt_logprobs="1"), "must be 0 or 1"),
    (dict(dtype="fp8"), "not with dtype 'fp8'"), (dict(dtype="mxfp4", mxfp4_head="mxfp4"), "not with mxfp4_head"),
    (dict(transport="grpc"), "not 'grpc'"),
    (dict(base="cifar_1gpu_colocated.json", prompt_logprobs=1), "generating models only"),
])
def test_config_rejections(kw, msg):
    from distributed_neural_networks_amd.config import ConfigError, parse_pipeline
    with pytest.raises(ConfigError, match=msg):
        parse_pipeline(_cfg(**kw))


def test_mirror_against_a_loop():
    from distributed_neural_networks_amd.runtime.sampling import prompt_logprobs_ref
    g = torch.Generator().manual_seed(0)
    M, V = 9, 37
    logits = (3 * torch.randn(M, V, generator=g)).bfloat16()
    logits[2, 5] = logits[2, 30] = logits[2].max() + 1  # a tie at the top: the smaller index wins
    tg = torch.tensor([0, V - 1, 30, -1, V, 7, 8, 9, 10])
    tok, tid, top = prompt_logprobs_ref(logits.float(), tg)
    for m in range(M):
        row = logits[m].double()
        lse = torch.log(torch.exp(row - row.max()).sum()) + row.max()
        if not 0 <= int(tg[m]) < V:
            assert (float(tok[m]), int(tid[m]), float(top[m])) == (0.0, -1, 0.0)
            continue
        best = max(range(V), key=lambda v: (float(row[v]), -v))
        assert int(tid[m]) == best
        assert abs(float(tok[m]) - float(row[int(tg[m])] - lse)) < 1e-6
        assert abs(float(top[m]) - float(row[best] - lse)) < 1e-6
    assert int(tid[2]) == 5


# ---------------------------------------------------------------------- rings (shared with the device test)
LENS = [1, 16, 9, 5, 12, 2, 16, 7]
R_T, R_CHUNK, R_STEPS = 16, 6, 4


def ring_ids(V, lens):
    ids = torch.randint(0, V, (len(LENS), R_T), generator=torch.Generator().manual_seed(3))
    for b, n in enumerate(lens):
        ids[b, n:] = 0
    return ids


def check_ring(got, lg, ids, lens, band):
    """``ring.prompt_logprobs()[0]`` against the fp64 log-softmax of the bf16-rounded reference logits ``lg``
    (B, T, V) on each row's own prompt; ``band(V, max|l|)`` + one bf16 ulp of the row's largest |logit| (the two
    routes may round a logit to neighbouring bf16).  top_id is compared where the reference's two largest
    logits are more than 2 ulp apart (either may have moved by one).  For V near-gaussian logits the gap of the
    top two is about exponential with mean sigma / sqrt(2 ln V) (sigma / 3.5 at V = 512) and 2 ulp of a maximum
    near 3 sigma are at most 3 sigma / 64, so about 15 % of positions are expected inside: the cap is 25 %."""
    V = lg.shape[2]
    lsm = torch.log_softmax(lg, dim=2)
    left = total = 0
    for b, n in enumerate(lens):
        assert got["tok_lp"][b].numel() == n and got["tok_lp"][b][0] == 0 and got["top_id"][b][0] == -1
        if n == 1:
            continue
        l, r = lg[b, :n - 1], lsm[b, :n - 1]
        amax = l.abs().max(dim=1).values
        ulp = torch.exp2(torch.floor(torch.log2(amax)) - 7)
        tol = torch.tensor([band(V, a) for a in amax.tolist()]) + ulp
        want = r.gather(1, ids[b, 1:n, None])[:, 0]
        assert ((got["tok_lp"][b][1:].double() - want).abs() <= tol).all(), (b, got["tok_lp"][b], want)
        assert ((got["top_lp"][b][1:].double() - r.max(dim=1).values).abs() <= tol).all()
        top2 = l.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 2 * ulp
        left, total = left + int((~clear).sum()), total + n - 1
        assert torch.equal(got["top_id"][b][1:][clear].long(), l.argmax(dim=1)[clear])
    print(f"top_id: {left} of {total} positions left out")
    assert left <= 0.25 * total


@pytest.mark.parametrize("lens", [LENS, None], ids=["ragged", "equal"])
def test_torch_ring_chunked(lens):
    """A ``TorchStage`` ring with a chunked prompt against each row's own unchunked full-prefix forward."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, B = "gpt2-tiny", len(LENS)
    V, n = model_info(model).cfg.vocab_size, model_info(model).num_layers
    ranges = [(0, n // 2 - 1), (n // 2, n - 1)]
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 7) for i, (a, b) in enumerate(ranges)]

    def stages(key):
        return [TorchStage(model, sds[i], a, b, i == 0, i == 1, prompt_logprobs=key) for i, (a, b) in enumerate(ranges)]
    ls = lens or [R_T] * B
    ids = ring_ids(V, ls)
    ring = DecodeRing(stages(1), RingLinks(), 1, 1, B, use_graphs=False, early_exit=False)
    ring.generate([ids], R_T, R_STEPS, R_CHUNK, lens=None if lens is None else [torch.tensor(lens)])
    lg = torch.zeros((B, R_T, V), dtype=torch.float64)
    for b, m in enumerate(ls):
        s0, s1 = stages(0)
        out = s1.step(s0.step(ids[b:b + 1, :m], 0, 1, m), 0, 1, m, last_only=False)
        lg[b, :m] = out.probs.reshape(m, V).bfloat16().double()
    check_ring(ring.prompt_logprobs()[0], lg, ids, ls, lambda V, a: 1e-5)  # (fp64 mirror: the band is the ulp)


def test_random_kernel_cases_leave_few_rows_out():
    """The device test's random operands, before any GPU run: rows whose two largest fp64 logits lie within
    one bf16 ulp (left out of its top_id comparison) stay within 2 % of every case's rows."""
    import test_prompt_logprobs_gpu as t
    for M, V, d, form in t.CASES:
        x, w, colsum, bias, _ = t._random_case(M, V, d, form)
        xd = x.double()
        st = None
        if form in ("ln", "rms"):
            mean = xd.mean(1, keepdim=True) if form == "ln" else torch.zeros(M, 1, dtype=torch.float64)
            rstd = torch.rsqrt(((xd - mean) ** 2).mean(1, keepdim=True) + 1e-5)
            st = torch.cat([rstd, -mean * rstd], 1)
        lb, *_, top2 = t._reference(x, w, st, colsum, bias, torch.zeros(M, dtype=torch.int32), dev="cpu")
        amax = lb.abs().max(dim=1).values
        close = (top2[:, 0] - top2[:, -1]) <= torch.exp2(torch.floor(torch.log2(amax)) - 7)
        assert int(close.sum()) <= 0.02 * M, (M, V, d, form, int(close.sum()))
