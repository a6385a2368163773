"""Logit constraints on the device (csrc/kernels/constraints.hip): the kernel
bitwise against the torch mirror with guard rows and sentinels, the rejections,
replay hygiene in a captured graph, the last stage's logits against the mirror,
rings (eager, single-step graphs, K-step graphs, the unfused tail) with the
invariants checked by plain loops, the neutral config, ragged prompts and the
CLI with the shipped config file."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import test_constraints as tc
from distributed_neural_networks_amd.config import ConstraintConfig
from distributed_neural_networks_amd.runtime.sampling import constraints_ref, constraints_store_prev

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX_LD = 48
LENS = [0, 1, 2, 3, 5, 17, 47, 48]  # per row, cycled: empty, shorter than every n, ..., len == ctx_ld
POISON = 11  # the id behind every row's context: its logit must come back untouched
SENTINEL = -123.0
NEG_INF = float("-inf")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _symbols(N):
    """The 5-symbol alphabet of the contexts: ids in the first vector, the middle
    of the row, and the last (partial, when N % 8) vector of the row."""
    return [0, 7, N // 2, N - 2, N - 1]


def _case(N, M, phase, seed):
    """(cons, contexts as lists, logits (M, N) bf16 on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    sym = _symbols(N)
    contexts = []
    for r in range(M):
        L = LENS[r % len(LENS)]
        c = [sym[i] for i in torch.randint(0, 5, (L,), generator=g).tolist()]
        if L >= 3:
            c[L - 1] = c[0]  # the newest token repeats the first: n = 2 bans c[1] (a match at j = 0)
        if L == 17:
            c[5] = N + 3  # ids outside [0, N): compared, never indexed
            c[9] = -4
        contexts.append(c)
    x = (torch.randn((M, N), generator=g) * 3).to(torch.bfloat16)
    x[:, 1] = float("inf")
    x[:, 2] = NEG_INF
    x[:, 3] = 0.0
    x[:, 4] = -0.0
    ids = [1, 2, 3, 4, sym[1], sym[4]] + [int(v) for v in torch.randperm(N - 40, generator=g)[:34] + 20]
    ids = [i for k, i in enumerate(ids) if i not in ids[:k] and i != POISON]
    bias = tuple((i, float(b)) for i, b in zip(ids, (torch.rand(len(ids), generator=g) * 10 - 5).tolist()))
    keep = torch.rand(N, generator=g) < 0.5
    keep[POISON] = True
    keep[[sym[0], sym[1], sym[3], sym[4]]] = True
    keep[sym[2]] = False
    keep[-9:] = torch.tensor([True, False] * 4 + [True])
    allowed = tuple(torch.nonzero(keep).flatten().tolist())
    bad = ((sym[3],), (sym[1], sym[2]), (sym[0], sym[0], sym[4]), (sym[4], sym[1]), (sym[2], sym[2], sym[2], sym[0]),
           tuple(sym[i % 5] for i in range(16)), (N - 3,))
    n = 2
    cons = {"bias": ConstraintConfig(bias, None, (), 0),
            "allowed": ConstraintConfig((), allowed, (), 0),
            "bad": ConstraintConfig((), None, bad, 0),
            "ngram": ConstraintConfig((), None, (), n),
            "all": ConstraintConfig(bias, allowed, bad, n)}[phase]
    return cons, contexts, x


def _launch(cons, contexts, x, N, ld, prev, ctx_ld=CTX_LD):
    """Run the kernel on guarded buffers: (logits block, ctx block, M)."""
    from distributed_neural_networks_amd.ops import transformer_ops as T_
    M = len(contexts)
    xs = torch.full((M + 2, ld), SENTINEL, dtype=torch.bfloat16, device=DEV)  # guard rows 0 and M + 1
    xs[1:M + 1, :N] = x.to(DEV)
    tab = torch.full((M + 2, ctx_ld), POISON, dtype=torch.int32, device=DEV)
    pv = torch.full((M + 2,), -1, dtype=torch.int32, device=DEV)
    lens = torch.zeros((M + 2,), dtype=torch.int32, device=DEV)
    for r, c in enumerate(contexts):
        keep = c[:-1] if (prev and c and 0 <= c[-1] < N) else c
        if keep:
            tab[r + 1, :len(keep)] = torch.tensor(keep, dtype=torch.int32, device=DEV)
        if len(keep) != len(c):
            pv[r + 1] = c[-1]
        lens[r + 1] = len(c)
    lens[0] = lens[M + 1] = 7  # the guard rows would be scanned if they were touched
    tables = T_.constraint_tables(cons, N, DEV)
    ctx = tab[1:M + 1] if (tables.needs_context or prev) else None
    y = T_.logit_constraints(xs[1:M + 1], N, tables, ctx=ctx, pos=lens[1:M + 1], pos_off=0,
                             prev=pv[1:M + 1] if prev else None)
    torch.cuda.synchronize()
    assert y.data_ptr() == xs[1:M + 1].data_ptr()
    return xs, tab, pv


def _expected_ctx(contexts, N, prev, ctx_ld=CTX_LD):
    M = len(contexts)
    tab = torch.full((M, ctx_ld), POISON, dtype=torch.int32)
    pv = torch.full((M,), -1, dtype=torch.int32)
    for r, c in enumerate(contexts):
        keep = c[:-1] if (prev and c and 0 <= c[-1] < N) else c
        if keep:
            tab[r, :len(keep)] = torch.tensor(keep, dtype=torch.int32)
        if len(keep) != len(c):
            pv[r] = c[-1]
    lens = [len(c) for c in contexts]
    return tab, (constraints_store_prev(tab, lens, pv, N) if prev else tab), lens, pv


@pytest.mark.parametrize("phase", ["bias", "allowed", "bad", "ngram", "all"])
@pytest.mark.parametrize("M", [1, 5, 65])
@pytest.mark.parametrize("N,ld", [(1000, 1024), (1003, 1024), (50257, 50304), (128256, 128256)])
def test_kernel_bitwise_equals_mirror(N, ld, M, phase):
    cons, contexts, x = _case(N, M, phase, 1000 * M + N % 977 + len(phase))
    if M == 1:
        contexts = [contexts[0] + [_symbols(N)[k] for k in (0, 1, 2, 1, 2, 3, 0, 0, 4, 4, 1)]]  # a row that fires
    for prev in (False, True):
        tab0, tab1, lens, pv = _expected_ctx(contexts, N, prev)
        want = constraints_ref(x, cons, tab0, lens, pv if prev else None)
        xs, tab, _ = _launch(cons, contexts, x, N, ld, prev)
        got = xs[1:M + 1, :N]
        assert torch.equal(_bits(got), _bits(want)), (prev, int((_bits(got) != _bits(want)).sum()))
        # guard rows above and below, the sentinels behind N, the context table
        assert bool((xs[0] == SENTINEL).all()) and bool((xs[M + 1] == SENTINEL).all())
        assert bool((xs[1:M + 1, N:] == SENTINEL).all())
        assert torch.equal(tab[1:M + 1].cpu(), tab1)
        assert bool((tab[0] == POISON).all()) and bool((tab[M + 1] == POISON).all())
        if prev:
            assert not torch.equal(tab0, tab1)  # a previous token was stored
        # the poison id behind every context: its logit is untouched
        assert torch.equal(_bits(got[:, POISON]), _bits(x[:, POISON]))
        # never vacuous: something was banned (the bias alone bans nothing: something changed), something was not
        new_inf = (want.float() == NEG_INF) & (x.float() != NEG_INF)
        if phase == "bias":
            assert int((_bits(want) != _bits(x)).sum()) >= M
        else:
            assert int(new_inf.sum()) >= 1, phase
        assert bool((want.float() != NEG_INF).any(1).all())
        assert bool((_bits(want) == _bits(x)).any(1).all())


@pytest.mark.parametrize("n", [1, 3, 16])
def test_kernel_ngram_sizes_and_full_context(n):
    """n = 1, 3, 16 on contexts up to len == ctx_ld, with planted repeats."""
    N, ld, M = 1003, 1024, 9
    sym = _symbols(N)
    g = torch.Generator().manual_seed(n)
    contexts = []
    for r in range(M):
        L = [CTX_LD, CTX_LD - 1, n, n + 1, max(n - 1, 0), 2 * n, 33, 40, CTX_LD][r]
        c = [sym[i] for i in torch.randint(0, 5, (L,), generator=g).tolist()]
        if L >= 2 * n + 2:
            c[L - (n - 1):] = c[1:n]  # the suffix repeats c[1 .. n): the entry c[n] is banned
        contexts.append(c)
    x = (torch.randn((M, N), generator=g) * 3).to(torch.bfloat16)
    cons = ConstraintConfig((), None, (), n)
    for prev in (False, True):
        tab0, tab1, lens, pv = _expected_ctx(contexts, N, prev)
        assert max(lens) == CTX_LD
        want = constraints_ref(x, cons, tab0, lens, pv if prev else None)
        assert tc.same(want, tc.loop_apply(x, cons, contexts))
        xs, tab, _ = _launch(cons, contexts, x, N, ld, prev)
        assert torch.equal(_bits(xs[1:M + 1, :N]), _bits(want))
        assert torch.equal(tab[1:M + 1].cpu(), tab1) and bool((xs[[0, M + 1]] == SENTINEL).all())
        new_inf = (want.float() == NEG_INF).sum(1)
        assert int(new_inf[0]) >= 1 and int(new_inf[-1]) >= 1 and int(new_inf[4]) == 0  # len = n - 1 bans nothing
        assert bool((want.float() != NEG_INF).any(1).all())


def test_rejections_and_empty_batch_launch_nothing():
    from distributed_neural_networks_amd.ops import transformer_ops as T_
    from distributed_neural_networks_amd.ops._lib import lib, ptr, stream_ptr
    N, ld, M = 1003, 1008, 4
    x = torch.full((M, ld), 1.0, dtype=torch.bfloat16, device=DEV)
    ctx = torch.full((M, 8), 2, dtype=torch.int32, device=DEV)
    pos = torch.full((M,), 5, dtype=torch.int32, device=DEV)
    prev = torch.full((M,), 9, dtype=torch.int32, device=DEV)
    cons = ConstraintConfig(((3, 1.0),), (1, 2, 3), ((2, 2), (5,)), 1)
    t = T_.constraint_tables(cons, N, DEV)
    good = dict(x=ptr(x), ld=ld, M=M, N=N, ctx=ptr(ctx), ctx_ld=8, pos=ptr(pos), pos_off=0, prev=ptr(prev),
                bias_ids=ptr(t.bias_ids), bias_vals=ptr(t.bias_vals), allow=ptr(t.allow), bad_ids=ptr(t.bad_ids),
                bad_len=ptr(t.bad_len), ngram=1, h_bias_ids=[3], h_bias_vals=[1.0], h_bad=[[2, 2], [5]],
                st=stream_ptr())
    many = list(range(257))
    bad = [dict(x=0), dict(ctx=0), dict(ld=1004), dict(ld=1000), dict(x=ptr(x) + 2), dict(ctx_ld=0),
           dict(h_bias_ids=many, h_bias_vals=[0.5] * 257), dict(h_bad=[[1]] * 65), dict(h_bad=[[]]),
           dict(h_bad=[list(range(17))]), dict(ngram=-1), dict(ngram=17), dict(h_bias_ids=[N]), dict(h_bias_ids=[-1]),
           dict(h_bad=[[1, N]]), dict(h_bad=[[-1]]), dict(h_bias_vals=[float("inf")]), dict(h_bias_vals=[float("nan")]),
           dict(h_bias_ids=[3, 4]), dict(bias_ids=0), dict(bad_ids=0), dict(bad_len=0), dict(N=0)]
    for kw in bad:
        assert lib().logit_constraints(**dict(good, **kw)) == -1, kw
    assert lib().logit_constraints(**dict(good, M=65536)) == -2
    # an empty batch is no error and launches nothing, even with arguments a launch would reject
    assert lib().logit_constraints(**dict(good, M=0, x=0)) == 0 and lib().logit_constraints(**dict(good, M=-3)) == 0
    torch.cuda.synchronize()
    assert bool((x == 1.0).all()) and bool((ctx == 2).all())
    # a null ctx is fine for rules that read no context
    t2 = T_.constraint_tables(ConstraintConfig(((3, 1.0),), (1, 2, 3), ((5,),), 0), N, DEV)
    flat = dict(good, ctx=0, ctx_ld=0, ngram=0, h_bad=[[5]], bad_ids=ptr(t2.bad_ids), bad_len=ptr(t2.bad_len))
    assert lib().logit_constraints(**flat) == 0
    torch.cuda.synchronize()
    assert int((x[:, :N].float() == NEG_INF).sum()) == M * (N - 3) and bool((x[:, N:] == 1.0).all())
    assert bool((x[:, 3] == 2.0).all()) and bool((x[:, 1:3] == 1.0).all())
    assert bool((ctx == 2).all())
    # the wrappers refuse the same before the library is called
    for c in (ConstraintConfig(((N, 1.0),), None, (), 0), ConstraintConfig(((1, 1.0), (1, 2.0)), None, (), 0),
              ConstraintConfig(((1, float("nan")),), None, (), 0), ConstraintConfig((), (), (), 0),
              ConstraintConfig((), None, ((),), 0), ConstraintConfig((), None, (), 17),
              ConstraintConfig((), (N,), (), 0)):
        with pytest.raises(ValueError, match="constraint_tables"):
            T_.constraint_tables(c, N, DEV)
    with pytest.raises(ValueError, match="need the context"):
        T_.logit_constraints(x, N, t)
    with pytest.raises(ValueError, match="n_vocab"):
        T_.logit_constraints(x, N - 1, t, ctx=ctx, pos=pos)


def test_replay_hygiene_same_launch_twice_in_a_graph():
    """The launch keeps no state of its own between replays: two launches in a
    captured graph give the mirror applied twice (the bias twice, the stored
    previous token once more at the same place)."""
    from distributed_neural_networks_amd.ops import transformer_ops as T_
    from distributed_neural_networks_amd.runtime.graph import GraphedStep
    N, ld, M = 1003, 1024, 5
    cons, contexts, x = _case(N, M, "all", 77)
    tab0, tab1, lens, pv = _expected_ctx(contexts, N, True)
    once = constraints_ref(x, cons, tab0, lens, pv)
    twice = constraints_ref(once, cons, tab1, lens, pv)
    assert not tc.same(once, twice)
    tables = T_.constraint_tables(cons, N, DEV)
    xs = torch.zeros((M, ld), dtype=torch.bfloat16, device=DEV)
    tab, pvd = tab0.to(DEV), pv.to(DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)

    def body():
        for _ in range(2):
            T_.logit_constraints(xs, N, tables, ctx=tab, pos=ln, prev=pvd)

    g = GraphedStep(body, torch.device(DEV, torch.cuda.current_device()), warmup=1)
    for _ in range(2):  # the same graph, replayed: each replay starts from fresh logits
        xs[:, :N] = x.to(DEV)
        tab.copy_(tab0.to(DEV))
        g()
        torch.cuda.synchronize()
        assert torch.equal(_bits(xs[:, :N]), _bits(twice)) and torch.equal(tab.cpu(), tab1)


# ---------------------------------------------------------------------- stages and rings
KINDS = {"greedy": {}, "sampled": dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)}
Mb, B, T, K, STEPS = 2, 4, 5, 4, 14  # 14 tokens: the prefill's, three K = 4 replays and one single step


@functools.lru_cache(maxsize=None)
def _weights(model, seed=9):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    n = model_info(model).num_layers
    ranges = [(0, n // 2 - 1), (n // 2, n - 1)]
    return ranges, [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, seed, nontrivial=True)
                    for i, (a, b) in enumerate(ranges)]


def _stages(model, max_batch, max_seq, **last_kw):
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    ranges, sds = _weights(model)
    return [TransformerStage(model, sds[i], a, b, i == 0, i == 1, DEV, max_batch=max_batch, max_seq=max_seq,
                             **(last_kw if i == 1 else {})) for i, (a, b) in enumerate(ranges)]


def _prompts(seed=12):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 512, (B, T), generator=g) for _ in range(Mb)]


def _ring(model, kind, cons, graphs, ms, **kw):
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    st = _stages(model, Mb * B, T + STEPS + K + 2, constraints=cons, **KINDS[kind], **kw)
    return DecodeRing(st, RingLinks(), 1, Mb, B, use_graphs=graphs, multi_step=ms)


def _generate(model, kind, cons, graphs, ms, lens=None, **kw):
    ring = _ring(model, kind, cons, graphs, ms, **kw)
    toks = ring.generate(_prompts(), T, STEPS, lens=lens)
    torch.cuda.synchronize()
    return toks, ring


@functools.lru_cache(maxsize=None)
def _free_run(model, kind):
    """The eager run without the keys: the reference, computed once and left unchanged."""
    toks, ring = _generate(model, kind, None, False, 0)
    return toks.clone()


def _rows(toks, lens=None):
    p = torch.cat(_prompts(), 0)
    lens = [T] * (Mb * B) if lens is None else lens
    return [p[b, :lens[b]].tolist() + toks[b].tolist() for b in range(Mb * B)], lens


def _choose(free, lens=None):
    """Constraints that the free run violates, each in at least one row: the
    largest n in (3, 2, 1) with a repeated n-gram ending at a generated token,
    bad words it produced (one across row 0's prompt / generation boundary),
    allowed ids without two ids it produced, and a bias."""
    rows, lens = _rows(free, lens)
    n = next((k for k in (3, 2, 1) if any(tc.repeats(r, k, lens[b]) for b, r in enumerate(rows))), None)
    assert n is not None, rows
    gen = free.flatten().tolist()
    common = max(set(gen), key=gen.count)
    out = sorted({common, int(free[3, 2])})
    bad = ((int(free[1, 1]),), (rows[0][lens[0] - 1], int(free[0, 0])),
           (int(free[2, 0]), int(free[2, 1]), int(free[2, 2])))
    bias = {}
    for i, v in ((int(free[5, 0]), -6.0), (int(free[6, 0]), 1.5), (3, 2.0)):
        bias.setdefault(i, v)
    cons = ConstraintConfig(tuple(bias.items()), tuple(i for i in range(512) if i not in out), bad, n)
    # the same config without the keys violates each invariant in at least one row
    assert any(tc.repeats(r, n, lens[b]) for b, r in enumerate(rows))
    assert any(tc.ends_bad(r, bad, lens[b]) for b, r in enumerate(rows))
    assert any(t in out for t in gen)
    return cons


def _check_invariants(toks, cons, lens=None):
    rows, lens = _rows(toks, lens)
    allowed = set(cons.allowed_token_ids)
    for b, r in enumerate(rows):
        assert not tc.repeats(r, cons.no_repeat_ngram_size, lens[b]), (b, r)  # no repeated n-gram ends at a generated token
        assert not tc.ends_bad(r, cons.bad_words_ids, lens[b]), (b, r)  # no bad word ends at a generated token
        assert all(t in allowed for t in r[lens[b]:]), (b, r)  # every token is allowed


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_rings_token_equal_and_invariants(model, kind):
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    free = _free_run(model, kind)
    cons = _choose(free)
    ntop = 3
    runs = {"eager": (False, 0), "single-step graphs": (True, 0), "K-step graphs": (True, K)}
    ref = None
    for name, (graphs, ms) in runs.items():
        toks, ring = _generate(model, kind, cons, graphs, ms, logprobs=ntop)
        last = ring.stages[-1]
        assert ring.con is last and last.con_ctx is not None and last.con_ctx.shape == (Mb * B, T + STEPS + K + 2)
        if name == "K-step graphs":
            assert ring.graph_k is not None and ring.graph_k_steps == K and ring.hist is not None
        lp = ring.logprobs()
        if ref is None:
            ref = (toks, lp)
            assert not torch.equal(toks, free)
            _check_invariants(toks, cons)
            assert bool(torch.isfinite(lp["chosen"]).all())  # taken after the constraints: never a banned token
            # the context table holds prompt + generated tokens (the last one is stored by the step that follows)
            rows, _ = _rows(toks)
            got = last.con_ctx[:, :T + STEPS - 1].cpu().tolist()
            assert got == [r[:T + STEPS - 1] for r in rows]
        assert torch.equal(toks, ref[0]), (name, toks.tolist(), ref[0].tolist())
        assert all(torch.equal(lp[k], ref[1][k]) for k in lp), name
        if name == "K-step graphs":  # a second generation on the same ring (the graphs are replayed) repeats it
            again = ring.generate(_prompts(), T, STEPS)
            torch.cuda.synchronize()
            assert torch.equal(again, ref[0])
    if "temperature" in KINDS[kind]:
        assert Tops.SAMPLE_FUSED_TAIL
        Tops.SAMPLE_FUSED_TAIL = False
        try:
            toks, ring = _generate(model, kind, cons, True, 0, logprobs=ntop)
            assert ring.hist is None
        finally:
            Tops.SAMPLE_FUSED_TAIL = True
        lp = ring.logprobs()
        assert torch.equal(toks, ref[0]) and all(torch.equal(lp[k], ref[1][k]) for k in lp)


@pytest.mark.parametrize("kind", list(KINDS))
def test_stage_logits_equal_mirror_of_unconstrained_logits(kind):
    """One prefill step and one decode step: the last stage's logits with the
    keys on are the mirror applied to the same step's logits with the keys off
    (the off stage samples, so that it takes the same unfused head, and is fed
    the on ring's first token)."""
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    model = "gpt2-tiny"
    cons = _choose(_free_run(model, kind))
    prompts = _prompts()[:1]
    rings = {}
    for key, c in (("on", cons), ("off", None)):
        st = _stages(model, B, T + 4, constraints=c, **(KINDS[kind] if c is not None else KINDS["sampled"]))
        rings[key] = DecodeRing(st, RingLinks(), 1, 1, B, use_graphs=False)
        rings[key].prefill(prompts, T)
    torch.cuda.synchronize()
    V = 512
    on, off = rings["on"].stages[-1], rings["off"].stages[-1]
    ctx = torch.full((B, T + 4), -1, dtype=torch.int32)
    ctx[:, :T] = prompts[0]
    want = constraints_ref(off.logits[:B, :V], cons, ctx, [T] * B)
    assert torch.equal(_bits(on.logits[:B, :V]), _bits(want))
    assert int((want.float() == NEG_INF).sum()) > int((off.logits[:B, :V].float() == NEG_INF).sum())
    first = rings["on"].out[0].clone()
    rings["off"].cur[0].copy_(first.view(B, 1))
    for r in rings.values():
        r.decode_round()
    torch.cuda.synchronize()
    ctx[:, T] = first.cpu()
    want = constraints_ref(off.logits[:B, :V], cons, ctx, [T + 1] * B)
    assert torch.equal(_bits(on.logits[:B, :V]), _bits(want))
    assert torch.equal(on.con_ctx[:B, :T + 1].cpu(), ctx[:, :T + 1])


def test_neutral_config_allocates_nothing():
    from distributed_neural_networks_amd.config import parse_pipeline
    model = "gpt2-tiny"
    assert parse_pipeline(tc._cfg(logit_bias={}, bad_words_ids=[], no_repeat_ngram_size=0)).constraints is None
    free = _free_run(model, "greedy")
    for kw in ({}, dict(constraints=None)):
        from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
        st = _stages(model, Mb * B, T + STEPS + K + 2, **kw)
        last = st[-1]
        assert last.constraints is None and last.con_tables is None and last.con_ctx is None and last.pen_prev is None
        assert not last.constraints_need_context
        ring = DecodeRing(st, RingLinks(), 1, Mb, B, multi_step=K)
        toks = ring.generate(_prompts(), T, STEPS)
        torch.cuda.synchronize()
        assert ring.con is None and ring.graph_k is not None and torch.equal(toks, free)
        with pytest.raises(ValueError, match="keeps no context"):
            last.constraint_begin(0, _prompts()[0])
    # only a last stage acts on the keys; rules without a context keep none
    st = _stages(model, Mb * B, T + STEPS, constraints=ConstraintConfig(((1, 1.0),), (1, 2, 3), ((2,),), 0))
    assert st[0].constraints is None and st[1].con_tables is not None and st[1].con_ctx is None
    assert st[1].pen_prev is None
    with pytest.raises(ValueError, match="constraint_tables"):
        _stages(model, 2, 16, constraints=ConstraintConfig(((512, 1.0),), None, (), 0))


@pytest.mark.parametrize("kind", list(KINDS))
def test_ragged_prompts_two_microbatches(kind):
    """Each row's context starts at its own length; eager and K-step graphs agree
    and the invariants hold against each row's own unpadded prompt."""
    model = "gpt2-tiny"
    lens = [1, 5, 3, 4, 5, 2, 5, 1]
    lt = [torch.tensor(lens[m * B:(m + 1) * B]) for m in range(Mb)]
    free, _ = _generate(model, kind, None, False, 0, lens=lt)
    cons = _choose(free, lens)
    eager, ring = _generate(model, kind, cons, False, 0, lens=lt)
    _check_invariants(eager, cons, lens)
    assert not torch.equal(eager, free)
    graphed, ring_k = _generate(model, kind, cons, True, K, lens=lt)
    assert ring_k.graph_k is not None and torch.equal(graphed, eager)
    rows, _ = _rows(eager, lens)
    got = ring_k.stages[-1].con_ctx.cpu()
    for b, r in enumerate(rows):
        assert got[b, :len(r) - 1].tolist() == r[:-1]


# ---------------------------------------------------------------------- the CLI with the shipped config file
def test_cli_with_the_constrained_config_file():
    from distributed_neural_networks_amd.config import load_json, parse_pipeline
    from distributed_neural_networks_amd.runtime.generate import make_prompts
    path = os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_constrained.json")
    pipe = parse_pipeline(load_json(path), path)
    cons = pipe.constraints
    prompt = make_prompts(pipe, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", path],
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    toks = json.loads(r.stdout.split("generated tokens:")[1].strip().splitlines()[0])
    assert len(toks) == prompt.shape[0] and all(len(t) == pipe.decode_steps for t in toks)
    allowed, Tp = set(cons.allowed_token_ids), prompt.shape[1]
    for b, t in enumerate(toks):
        seq = prompt[b].tolist() + t
        assert all(v in allowed for v in t), (b, t)
        assert not tc.repeats(seq, cons.no_repeat_ngram_size, Tp) and not tc.ends_bad(seq, cons.bad_words_ids, Tp)
