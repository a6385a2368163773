"""Nucleus (top-p) and min-p filters: the torch mirror against first
principles, the config keys and the CPU golden stage."""
import os

import pytest
import torch

from distributed_neural_networks_amd.runtime.sampling import _keys, pick, sample_ref, sample_topk_ref

ROW = [2.0, 1.0, 0.5, 0.0, -1.0, -3.0]


def test_filters_off_reproduce_the_topk_mirror():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 1000, generator=g).bfloat16()
    step = torch.arange(64, dtype=torch.int32) * 3
    for k in (0, 7):
        assert torch.equal(sample_ref(x, 0.9, k, seed=5, step=step), sample_topk_ref(x, 0.9, k, 5, step))
        assert torch.equal(pick(x, 0.9, k, 5, step), sample_topk_ref(x, 0.9, k, 5, step))


def test_nucleus_matches_sorted_cumsum_oracle():
    """Kept set of the mirror (key >= thr) == the textbook nucleus: fp64
    softmax, sort descending, cumulative sum, the minimal prefix that reaches
    top_p, extended over ties at the boundary value.  Rows whose cumulative
    mass comes within 1e-9 of top_p on either side of the boundary are left out
    (at most 2 of 48)."""
    torch.manual_seed(3)
    top_p = 0.9
    x = (torch.randn(48, 1000) * 3).bfloat16()
    _, thr = sample_ref(x, 1.0, top_p=top_p, return_thr=True)
    kept = _keys(x) >= thr[:, None].long()
    p = torch.softmax(x.double(), dim=1)
    sp, order = p.sort(dim=1, descending=True)
    cum = sp.cumsum(dim=1)
    checked, sizes = 0, []
    for r in range(48):
        n = int((cum[r] < top_p).sum().item()) + 1  # minimal prefix with mass >= top_p
        before = cum[r, n - 2].item() if n > 1 else 0.0
        if min(abs(cum[r, n - 1].item() - top_p), abs(before - top_p)) < 1e-9:
            continue
        want = x[r].double() >= x[r, order[r, n - 1]].double()  # ties at the boundary value stay
        assert torch.equal(kept[r], want), r
        checked += 1
        sizes.append(int(want.sum()))
    assert checked >= 46
    assert min(sizes) < 10 and max(sizes) > 50  # the filter bites, and differently per row


def _freq(ids, n):
    return torch.bincount(ids.long(), minlength=6).float() / n


def test_nucleus_frequencies():
    """Row with cumulative probabilities .646, .831, .930, ... at T = 0.8:
    top_p = 0.9 keeps the first three (margins .03 / .07); the draws follow the
    softmax renormalised over them."""
    x = torch.tensor([ROW]).bfloat16()
    n = 20000
    ids = sample_ref(x.repeat(n, 1), 0.8, top_p=0.9, seed=11, step=torch.arange(n, dtype=torch.int32))
    f = _freq(ids, n)
    p3 = torch.softmax(x.float()[0, :3] / 0.8, 0)
    assert (f[:3] - p3).abs().max().item() < 0.015 and f[3:].sum().item() == 0


def test_min_p_support_and_frequencies():
    """p_i / p_max at T = 0.8: 1, .287, .153, .082, ...: min_p = 0.1 keeps three."""
    x = torch.tensor([ROW]).bfloat16()
    n = 20000
    ids, thr = sample_ref(x.repeat(n, 1), 0.8, min_p=0.1, seed=12, step=torch.arange(n, dtype=torch.int32),
                          return_thr=True)
    assert torch.equal(_keys(x)[0] >= int(thr[0]), torch.tensor([True, True, True, False, False, False]))
    f = _freq(ids, n)
    p3 = torch.softmax(x.float()[0, :3] / 0.8, 0)
    assert (f[:3] - p3).abs().max().item() < 0.015 and f[3:].sum().item() == 0


def test_tiny_top_p_and_large_min_p_are_greedy():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, 1000, generator=g).bfloat16()
    xf = x.float()
    greedy = xf.argmax(1).to(torch.int32)
    unique = (xf == xf.max(1, keepdim=True).values).sum(1) == 1
    assert int(unique.sum()) > 32
    a = sample_ref(x, 1.0, top_p=1e-6, seed=4)
    b = sample_ref(x, 1.0, top_p=1.0, min_p=0.999999, seed=4)
    assert torch.equal(a[unique], greedy[unique])
    assert torch.equal(b[unique], greedy[unique])
    # ties at the maximum: still a maximiser
    assert torch.equal(xf.gather(1, a[:, None].long())[:, 0], xf.max(1).values)


def test_thr_override_and_bad_arguments():
    x = torch.randn(4, 50).bfloat16()
    ids, thr = sample_ref(x, 1.0, top_p=0.5, seed=2, return_thr=True)
    assert thr.dtype == torch.int32 and thr.shape == (4,)
    assert torch.equal(sample_ref(x, 1.0, seed=2, thr=thr), ids)
    for kw in ({"top_p": 0.0}, {"top_p": 1.5}, {"min_p": 1.0}, {"min_p": -0.1}):
        with pytest.raises(ValueError):
            sample_ref(x, 1.0, **kw)


def _cfg(**kw):
    d = {"nodes": [{"id": "a", "address": "127.0.0.1:1", "part_index": 0}], "model_weights": "synthetic:0",
         "num_parts": 1, "model": "gpt2-tiny"}
    d.update(kw)
    return d


def test_config_keys():
    from distributed_neural_networks_amd.config import ConfigError, load_json, parse_pipeline
    p = parse_pipeline(_cfg())
    assert p.top_p == 1.0 and p.min_p == 0.0
    p = parse_pipeline(_cfg(top_p=0.9, min_p=0.05, temperature=0.8))
    assert p.top_p == 0.9 and p.min_p == 0.05
    for v in (0, -0.1, 1.5, True, "x"):
        with pytest.raises(ConfigError, match=r"'top_p' must be in \(0, 1\]"):
            parse_pipeline(_cfg(top_p=v))
    for v in (1.0, -0.1, True):
        with pytest.raises(ConfigError, match=r"'min_p' must be in \[0, 1\)"):
            parse_pipeline(_cfg(min_p=v))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                        "gpt2_4stage_1gpu_sampled.json")
    p = parse_pipeline(load_json(path), path)
    assert (p.temperature, p.top_k, p.top_p, p.min_p, p.seed) == (0.8, 50, 0.95, 0.0, 1)
    assert p.model == "gpt2" and p.num_parts == 4


def test_torch_stage_samples_with_filters():
    """CPU golden stage with the 5-tuple sampling argument: the tokens of
    ``step`` are ``sample_ref`` of the logits it returns."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model = "gpt2-tiny"
    n = model_info(model).num_layers
    sd = ckpt.random_stage_state_dict(model, 0, n - 1, True, True, 5)
    B, T = 3, 6
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, model_info(model).cfg.vocab_size, (B, T), generator=g)
    pos = torch.zeros(B, dtype=torch.int32)
    st = TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.8, 20, 7, 0.9, 0.02))
    assert (st.top_p, st.min_p) == (0.9, 0.02)
    y = st.step(ids, pos, B, T)
    ref = sample_ref(y.probs, 0.8, 20, 0.9, 0.02, seed=7, step=pos)
    assert torch.equal(y.pred, ref)
    plain = TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.8, 20, 7))
    assert (plain.top_p, plain.min_p) == (1.0, 0.0)
    # the filters reach the draw: a vanishing nucleus picks a maximiser of the bf16 logits
    narrow = TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.8, 20, 7, 1e-6, 0.0))
    xb = y.probs.bfloat16().float()
    got = narrow.step(ids, pos, B, T).pred
    assert torch.equal(xb.gather(1, got[:, None].long())[:, 0], xb.max(1).values)
