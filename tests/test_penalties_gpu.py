"""Repetition / presence / frequency penalties on the device
(csrc/kernels/penalties.hip, the last stage's hooks, the decode ring's
capture-restore) — MI355X only.  The kernel is held bitwise to the torch
mirror (runtime/sampling.py): the file is built without FP contraction."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 5
SENT_X = -123.0      # sentinel logit of the guard rows and of the columns [N, ld)
SENT_C = 0x1234      # sentinel state there (non-zero: a kernel that read it would penalise)
PENS = [(2.0, 0.25, 0.5), (0.5, -0.5, 0.0), (1.3, 0.37, 0.21)]  # (rep, freq, pres); the last one non-dyadic
SIZES = [(1000, 1024), (1003, 1024), (50257, 50304), (128256, 128256)]


def _bits(t):
    """bf16 / int16 tensors as their 16-bit patterns (0.0 and -0.0 differ, unlike torch.equal on floats)."""
    return t.cpu().contiguous().view(torch.int16)


def _to16(u):
    return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(N, ld):
    """Host inputs shared by the tests: logits (M + 2, ld) bf16 and state
    (M + 2, ld) int16, both with a guard row above and below and sentinels in
    the columns [N, ld); rows 1..M are the kernel's."""
    g = torch.Generator().manual_seed(1000 + N)
    x = torch.full((M + 2, ld), SENT_X).bfloat16()
    x[1:M + 1, :N] = (torch.randn(M, N, generator=g) * 3).bfloat16()
    u = torch.zeros((M, N), dtype=torch.int64)
    r = torch.rand(M, N, generator=g)
    cnt = torch.randint(1, 6, (M, N), generator=g)
    u[r < 0.0033] = 0x8000                                  # P only
    gen = (r >= 0.0033) & (r < 0.0066)
    u[gen] = cnt[gen]                                       # g only
    both = (r >= 0.0066) & (r < 0.01)
    u[both] = 0x8000 | cnt[both]                            # both
    u[0, 0], u[0, N - 1] = 0x8000 | 2, 3                    # the first and the last entry
    u[1, 0], u[1, N - 1] = 1, 0x8000
    u[2, N // 2] = 0x7FFF                                   # g saturated
    u[3] = 0                                                # one row entirely unseen
    xs = x[1:M + 1]
    # planted values at seen positions
    xs[0, 0], xs[0, N - 1], xs[1, 0], xs[1, N - 1] = 0.0, -0.0, float("inf"), -4.5
    xs[2, N // 2] = -1.75
    st = torch.full((M + 2, ld), SENT_C, dtype=torch.int16)
    st[1:M + 1, :N] = _to16(u)
    return x, st


def _expect(x, st, N, pen, state_rows=None):
    """The whole logits buffer after the call: the mirror on rows 1..M, columns [0, N)."""
    from distributed_neural_networks_amd.runtime.sampling import apply_penalties_ref
    rep, freq, pres = pen
    want = x.clone()
    s = st[1:M + 1, :N] if state_rows is None else state_rows
    want[1:M + 1, :N] = apply_penalties_ref(x[1:M + 1, :N], s, rep, freq, pres)
    return want


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("N,ld", SIZES)
def test_kernel_equals_mirror(N, ld, pen):
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    x, st = _case(N, ld)
    xd, sd = x.to(DEV), st.to(DEV)
    Tops.logit_penalties(xd[1:M + 1], sd[1:M + 1], None, pen[0], pen[1], pen[2], N)
    torch.cuda.synchronize()
    want = _expect(x, st, N, pen)
    assert torch.equal(_bits(xd), _bits(want))            # guards and sentinels included
    assert torch.equal(_bits(sd), _bits(st))              # prev = None: the state is only read
    moved = (_bits(want) != _bits(x))[1:M + 1].sum(1)
    assert bool((moved[[0, 1, 2, 4]] > 0).all()) and int(moved[3]) == 0  # no no-op; the unseen row untouched


def test_uint16_state_and_single_row():
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    N, ld = 1003, 1024
    x, st = _case(N, ld)
    xd, sd = x.to(DEV), st.to(DEV)
    Tops.logit_penalties(xd[1:2], sd.view(torch.uint16)[1:2], None, 1.3, 0.37, 0.21, N)
    torch.cuda.synchronize()
    want = x.clone()
    want[1:2] = _expect(x, st, N, (1.3, 0.37, 0.21))[1:2]
    assert torch.equal(_bits(xd), _bits(want))


def test_counting():
    """``prev`` = a fresh token, a prompt token, a token at g = 0x7FFF, -1, N:
    two calls; the state follows ``penalty_count`` and the logits the mirror on
    the updated state."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.sampling import penalty_count
    N, ld, pen = 50257, 50304, (1.3, 0.37, 0.21)
    x, st = _case(N, ld)
    st = st.clone()
    rows = st[1:M + 1, :N]
    fresh = int((rows[0] == 0).nonzero()[7])              # unseen so far
    prompt_tok = int((rows[1] == -0x8000).nonzero()[3])   # P only
    rows[2, 4242] = -1                                    # 0xFFFF: P and g = 0x7FFF
    prev = torch.tensor([fresh, prompt_tok, 4242, -1, N], dtype=torch.int32)
    xd, sd, pd = x.to(DEV), st.to(DEV), prev.to(DEV)
    s1 = penalty_count(rows, prev)
    u1 = s1.to(torch.int64) & 0xFFFF
    assert int(u1[0, fresh]) == 1 and int(u1[1, prompt_tok]) == 0x8001 and int(u1[2, 4242]) == 0xFFFF
    assert torch.equal(s1[3:], rows[3:])                  # the two out-of-range rows
    Tops.logit_penalties(xd[1:M + 1], sd[1:M + 1], pd, pen[0], pen[1], pen[2], N)
    torch.cuda.synchronize()
    want_s = st.clone()
    want_s[1:M + 1, :N] = s1
    want_x1 = _expect(x, st, N, pen, s1)
    assert torch.equal(_bits(sd), _bits(want_s))
    assert torch.equal(_bits(xd), _bits(want_x1))
    Tops.logit_penalties(xd[1:M + 1], sd[1:M + 1], pd, pen[0], pen[1], pen[2], N)
    torch.cuda.synchronize()
    s2 = penalty_count(s1, prev)
    u2 = s2.to(torch.int64) & 0xFFFF
    assert int(u2[0, fresh]) == 2 and int(u2[1, prompt_tok]) == 0x8002 and int(u2[2, 4242]) == 0xFFFF
    want_s[1:M + 1, :N] = s2
    assert torch.equal(_bits(sd), _bits(want_s))
    assert torch.equal(_bits(xd), _bits(_expect(want_x1, st, N, pen, s2)))
    # prev = None: the state stays
    Tops.logit_penalties(xd[1:M + 1], sd[1:M + 1], None, pen[0], pen[1], pen[2], N)
    torch.cuda.synchronize()
    assert torch.equal(_bits(sd), _bits(want_s))


def test_rejections_and_empty_batch():
    from distributed_neural_networks_amd.ops import _lib
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    N, ld = 1000, 1024
    x, st = _case(N, ld)
    xd, sd = x.to(DEV), st.to(DEV)
    p, c, s = xd[1:].data_ptr(), sd[1:].data_ptr(), _lib.stream_ptr()
    f = _lib.lib().logit_penalties
    nan, inf = float("nan"), float("inf")
    assert f(0, ld, M, N, c, ld, 0, 1.3, 0.1, 0.1, s) == -1            # null logits
    assert f(p, ld, M, N, 0, ld, 0, 1.3, 0.1, 0.1, s) == -1            # null state
    assert f(p, ld - 4, M, N, c, ld, 0, 1.3, 0.1, 0.1, s) == -1        # ld % 8
    assert f(p, ld, M, N, c, ld - 4, 0, 1.3, 0.1, 0.1, s) == -1        # cnt_ld % 8
    assert f(p, ld, M, N, c, N - 8, 0, 1.3, 0.1, 0.1, s) == -1         # cnt_ld < N
    for rep in (0.0, -1.0, nan):
        assert f(p, ld, M, N, c, ld, 0, rep, 0.1, 0.1, s) == -1
    for bad in (nan, inf, -inf):
        assert f(p, ld, M, N, c, ld, 0, 1.3, bad, 0.1, s) == -1
        assert f(p, ld, M, N, c, ld, 0, 1.3, 0.1, bad, s) == -1
    assert f(x=p, ld=ld, M=0, N=N, cnt=c, cnt_ld=ld, prev=0, rep=1.3, freq=0.1, pres=0.1, st=s) == 0  # by keyword
    assert f(p, ld, -3, N, c, ld, 0, nan, 0.1, 0.1, s) == 0            # M <= 0 comes first: nothing to do
    rows, srows = xd[1:M + 1], sd[1:M + 1]
    with pytest.raises(TypeError):
        Tops.logit_penalties(rows.float(), srows, None, 1.3, 0.1, 0.1, N)
    with pytest.raises(TypeError):
        Tops.logit_penalties(rows, srows.int(), None, 1.3, 0.1, 0.1, N)
    with pytest.raises(TypeError):
        Tops.logit_penalties(rows[:, ::2], srows, None, 1.3, 0.1, 0.1, 8)
    with pytest.raises(ValueError):
        Tops.logit_penalties(rows, srows[:, :N - 8], None, 1.3, 0.1, 0.1, N)      # state narrower than n
    with pytest.raises(ValueError):
        Tops.logit_penalties(rows, srows[:M - 1], None, 1.3, 0.1, 0.1, N)         # fewer state rows
    with pytest.raises(ValueError):
        Tops.logit_penalties(rows, srows, None, 1.3, 0.1, 0.1, ld + 1)            # n past the row
    with pytest.raises(ValueError):
        Tops.logit_penalties(rows, srows, torch.zeros(M, dtype=torch.int64, device=DEV), 1.3, 0.1, 0.1, N)
    with pytest.raises(ValueError):
        Tops.logit_penalties(rows, srows, torch.zeros(M - 1, dtype=torch.int32, device=DEV), 1.3, 0.1, 0.1, N)
    with pytest.raises(ValueError):
        Tops.logit_penalties(rows[:, 1:], srows, None, 1.3, 0.1, 0.1, 8)          # rows not 16-byte aligned
    for rep, fr, pr in ((0.0, 0.1, 0.1), (nan, 0.1, 0.1), (1.3, inf, 0.1), (1.3, 0.1, nan)):
        with pytest.raises(ValueError):
            Tops.logit_penalties(rows, srows, None, rep, fr, pr, N)
    Tops.logit_penalties(rows[:0], srows[:0], None, 1.3, 0.1, 0.1, N)  # M = 0: no launch
    torch.cuda.synchronize()
    assert torch.equal(_bits(xd), _bits(x)) and torch.equal(_bits(sd), _bits(st))  # nothing above ran a kernel


# ---------------------------------------------------------------------- the last stage against its raw logits
def _stage_pair(model, last_kw, seed=7, max_batch=3, max_seq=64):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    n = model_info(model).num_layers
    ranges = [(0, n // 2 - 1), (n // 2, n - 1)]
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, seed, nontrivial=True)
           for i, (a, b) in enumerate(ranges)]
    first = TransformerStage(model, sds[0], *ranges[0], True, False, DEV, max_batch=max_batch, max_seq=max_seq)
    lasts = [TransformerStage(model, sds[1], *ranges[1], False, True, DEV, max_batch=max_batch, max_seq=max_seq, **kw)
             for kw in last_kw]
    return first, lasts


def _first_argmax(x):
    """Per-row argmax of a bf16 tensor, ties to the smallest index."""
    xf = x.float()
    idx = torch.arange(xf.shape[1]).expand_as(xf)
    return torch.where(xf == xf.max(1, keepdim=True).values, idx, torch.full_like(idx, 1 << 30)).min(1).values.int()


def _without_last(state, last):
    """The device counts a token at the start of the next step: its state lags
    the host's by the last token."""
    u = state.to(torch.int64) & 0xFFFF
    for r, t in enumerate(last.cpu().tolist()):
        u[r, t] -= 1
    return _to16(u)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_stage_probs_are_the_penalised_raw_logits(model, sampled):
    """Stage A (penalties) and stage B (none; sampling, so it takes the same
    unfused head) see the same inputs: A's logits are the mirror of B's on the
    host-kept state, after the prefill and after each teacher-forced decode step."""
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.sampling import (apply_penalties_ref, penalty_count, penalty_state,
                                                                  sample_ref)
    pen = dict(repetition_penalty=2.0, frequency_penalty=0.25, presence_penalty=0.5)
    samp = dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)
    first, (A, Bst) = _stage_pair(model, [dict(pen, **(samp if sampled else {})), dict(temperature=0.8)])
    assert A.penalties_on and not Bst.penalties_on and Bst.pen_state is None
    V = model_info(model).cfg.vocab_size
    B, T, steps = 3, 16, 6
    g = torch.Generator().manual_seed(31)
    prompt = torch.randint(0, V, (B, T), generator=g)
    prompt[:, 9] = prompt[:, 2]  # a repeated token in each row
    state = penalty_state(prompt, V)
    A.penalty_begin(0, prompt)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    x = prompt.to(device=DEV, dtype=torch.int32)
    agree = []
    for t in range(steps + 1):
        Tn = T if t == 0 else 1
        h = first.step(x, pos, B, Tn)
        ya = A.step(h, pos, B, Tn)
        pa, ta = ya.probs.clone(), ya.pred.clone()
        raw = Bst.step(h, pos, B, Tn).probs.clone()
        torch.cuda.synchronize()
        want = apply_penalties_ref(raw, state, 2.0, 0.25, 0.5)
        assert torch.equal(_bits(pa), _bits(want)), t
        assert bool(((_bits(pa) != _bits(raw)).sum(1) > 0).all()), t  # no no-op in any row
        if not sampled:
            assert torch.equal(ta.cpu(), _first_argmax(want)), t
        else:
            # the draw at the device's own threshold (the nucleus mass is a fast-math sum), as
            # test_sampling_filters_gpu.py compares it
            out = torch.empty(B, dtype=torch.int32, device=DEV)
            thr = torch.empty(B, dtype=torch.int32, device=DEV)
            Tops.sample_rows(A.logits[:B], out, V, 0.8, 20, 0.9, 0.0, seed=5, step=pos, thr_out=thr)
            torch.cuda.synchronize()
            assert torch.equal(out, ta), t
            ref = sample_ref(want, 0.8, 20, 0.9, seed=5, step=pos.cpu(), thr=thr.cpu())
            agree.append((ref == ta.cpu()).float())
        state = penalty_count(state, ta)
        pos += Tn
        x = ta.view(B, 1).clone()
    assert torch.equal(_bits(A.pen_state[:B, :V]), _bits(_without_last(state, ta)))
    if sampled:
        a = torch.cat(agree).mean().item()
        assert a >= 0.95, a  # __logf vs log: rare near-ties may flip


# ---------------------------------------------------------------------- decode ring
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_decode_ring_penalised_tokens(model, sampled):
    """With penalties the tokens are the same eagerly, with single-step graphs,
    with K = 4 steps per graph and (sampled) with the unfused tail: the warm-up
    and capture runs leave no counts behind.  A second generation on the same
    ring repeats the first: the state starts from the prompt."""
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
    for p in prompts:
        p[:, 11] = p[:, 4]
    kw = dict(repetition_penalty=2.0, frequency_penalty=0.25, presence_penalty=0.5)
    if sampled:
        kw.update(temperature=0.8, top_k=20, seed=5, top_p=0.9)

    def generate(graphs, ms, **over):
        a = dict(kw, **over)
        st = [TransformerStage(model, sds[i], lo, hi, i == 0, i == 1, DEV, max_batch=Mb * B,
                               max_seq=T + steps + K + 2, **a) for i, (lo, hi) in enumerate(ranges)]
        ring = DecodeRing(st, RingLinks(), 1, Mb, B, use_graphs=graphs, multi_step=ms)
        toks = ring.generate(prompts, T, steps)
        torch.cuda.synchronize()
        return toks, ring

    ref, ring0 = generate(False, 0)
    assert ref.shape == (Mb * B, steps) and ring0.pen is ring0.stages[-1] and not ring0.stages[0].penalties_on
    one, ring1 = generate(True, 0)
    assert ring1.graph_k is None and ring1.graphs
    multi, ringk = generate(True, K)
    assert ringk.graph_k is not None
    assert torch.equal(one, ref) and torch.equal(multi, ref)
    if sampled:
        assert Tops.SAMPLE_FUSED_TAIL
        Tops.SAMPLE_FUSED_TAIL = False
        try:
            unfused, ringu = generate(True, 0)
            assert ringu.hist is None
        finally:
            Tops.SAMPLE_FUSED_TAIL = True
        assert torch.equal(unfused, ref)
    again = ringk.generate(prompts, T, steps)
    torch.cuda.synchronize()
    assert torch.equal(again, ref)
    plain, _ = generate(False, 0, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)
    assert not torch.equal(plain, ref)  # the penalties change the generation


# ---------------------------------------------------------------------- neutral values, arguments
def test_neutral_values_change_nothing():
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage, build_device_stage
    model = "gpt2-tiny"
    n = model_info(model).num_layers
    ranges = [(0, n // 2 - 1), (n // 2, n - 1)]
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 9, nontrivial=True)
           for i, (a, b) in enumerate(ranges)]
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, model_info(model).cfg.vocab_size, (2, 16), generator=g)]
    toks = []
    for kw in ({}, dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)):
        st = [TransformerStage(model, sds[i], a, b, i == 0, i == 1, DEV, max_batch=2, max_seq=32, **kw)
              for i, (a, b) in enumerate(ranges)]
        assert not st[1].penalties_on and st[1].pen_state is None and st[1].pen_prev is None
        ring = DecodeRing(st, RingLinks(), 1, 1, 2, use_graphs=False)
        assert ring.pen is None
        toks.append(ring.generate(prompts, 16, 5))
    assert torch.equal(toks[0], toks[1])
    # a non-last stage never holds state; bad values and a 15-bit-overflowing cache are refused
    a, b = ranges[0]
    st0 = build_device_stage(model, sds[0], a, b, True, False, DEV, max_batch=2, max_seq=32, repetition_penalty=1.5)
    assert not st0.penalties_on and st0.pen_state is None
    a, b = ranges[1]
    on = build_device_stage(model, sds[1], a, b, False, True, DEV, max_batch=2, max_seq=32, presence_penalty=0.5)
    assert on.penalties_on and on.pen_state.shape == (2, on.Vpad) and on.pen_state.dtype == torch.int16
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
               dict(presence_penalty=float("inf")), dict(frequency_penalty=float("nan"))):
        with pytest.raises(ValueError):
            TransformerStage(model, sds[1], a, b, False, True, DEV, max_batch=2, max_seq=32, **kw)
    with pytest.raises(ValueError, match="32768"):
        TransformerStage(model, sds[1], a, b, False, True, DEV, max_batch=1, max_seq=32768, frequency_penalty=0.1)


# ---------------------------------------------------------------------- the config keys reach the device stages
def test_cli_colocated_penalised_equals_ring(tmp_path):
    """``node.py`` on a colocated 2-stage config with the three keys generates
    what a ring of stages built with the same arguments generates."""
    import json
    import os
    import subprocess
    import sys
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model, ids, steps, Mb, B = "gpt2-tiny", [5, 17, 99, 17, 42, 17, 1, 250], 6, 2, 2
    samp = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7)
    pen = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.3)
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{51000 + i}", "part_index": i, "device": 0}
                   for i in range(2)],
         "model_weights": "synthetic:3", "num_parts": 2, "return_to_node_id": "node1", "transport": "colocated",
         "model": model, "seq_len": 32, "decode_steps": steps, "micro_batch_size": B, "num_microbatches": Mb}
    c.update(samp)
    c.update(pen)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(c))
    r = subprocess.run([sys.executable, os.path.join(root, "node.py"), "--node_id", "node1", "--config", str(cfg),
                        "--prompt", ",".join(map(str, ids))], env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    toks = torch.tensor(json.loads(r.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    T = len(ids)
    ranges = default_ranges(model, 2)

    def ring_tokens(**kw):
        # the CLI's cache sizes (decode attention splits follow them) and its device-side synthetic weights
        st = [build_device_stage(model, ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 3, device=DEV), a, b,
                                 i == 0, i == 1, torch.device(DEV, 0), max_batch=Mb * B, max_seq=T + steps,
                                 max_tokens=B * (T + steps), **samp, **kw) for i, (a, b) in enumerate(ranges)]
        prompt = torch.tensor([ids]).repeat(B, 1)
        out = DecodeRing(st, RingLinks(), 1, Mb, B).generate([prompt] * Mb, T, steps)
        torch.cuda.synchronize()
        return out

    want = ring_tokens(**pen)
    assert toks.shape == (Mb * B, steps) and torch.equal(toks, want)
    assert not torch.equal(ring_tokens(), want)
