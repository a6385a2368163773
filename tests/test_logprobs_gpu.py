"""Per-token log-probabilities and top-n alternatives on the device
(csrc/kernels/logprobs.hip, the last stage's launch behind the argmax /
sampler, the decode ring's histories) — MI355X only.  The ids are held exactly
to the torch mirror (runtime/sampling.py logprobs_ref), the values to 2^-15;
the one-hot fixtures are exact bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 5
L = 6                 # positions per history row in the op-level tests
SENT_X = -123.0       # sentinel logit of the guard rows and of the columns [N, ld)
SENT_C, SENT_I, SENT_T = 777.0, -7, 555.0  # sentinels of the three histories
SIZES = [(1000, 1024), (1003, 1024), (50257, 50304), (128256, 128256)]
NS = [0, 1, 5, 20]
# |x| <= 32 and N <= 2^17 give |lp| < 128, so the fp32 rounding of a result is <= 2^-18; the fp32
# sum of exponentials adds about log2(N) 2^-24 relative error, the same absolute error in its log:
# 2^-15 leaves about 4x over the two together
TOL = 2.0 ** -15
NINF = float("-inf")

# a GPT-2-shaped model whose vocabulary is odd and spans three of the kernel's 2048-column chunks
LP_MODEL = "gpt2-logprobs-test"


@pytest.fixture(scope="module", autouse=True)
def _lp_model():
    """LP_MODEL exists while this module's tests run, and only then."""
    from distributed_neural_networks_amd.models import gpt2
    gpt2.GPT_CONFIGS[LP_MODEL] = gpt2.GPTConfig(block_size=64, vocab_size=5003, n_layer=2, n_head=4, n_embd=256)
    yield
    del gpt2.GPT_CONFIGS[LP_MODEL]


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def _case(N, ld):
    """Host inputs shared by the tests: logits (M + 2, ld) bf16 with a guard row
    above and below and sentinels in [N, ld); rows 1..M are the kernel's:
    3 randn with the row maximum planted three more times (next to it, in the
    row's middle and at N - 2), one -inf, and the chosen tokens at column 0, at
    column N - 1, at the (first) argmax and at two random places.  Returns
    (logits, tokens, the mirror's results for n = 20)."""
    from distributed_neural_networks_amd.runtime.sampling import logprobs_ref
    g = torch.Generator().manual_seed(2000 + N)
    x = torch.full((M + 2, ld), SENT_X).bfloat16()
    xs = (torch.randn(M, N, generator=g) * 3).bfloat16()
    for r in range(M):
        top = xs[r].float().max()
        am = int(xs[r].float().argmax())
        for c in (min(am + 1, N - 1), N // 2, N - 2):
            xs[r, c] = top
        xs[r, (7 * r + 3) % N] = NINF
    assert float(xs[xs > NINF].float().abs().max()) <= 32
    x[1:M + 1, :N] = xs
    first_max = torch.where(xs.float() == xs.float().max(1, keepdim=True).values,
                            torch.arange(N).expand(M, N), torch.full((M, N), 1 << 30)).min(1).values
    tok = torch.tensor([0, N - 1, int(first_max[2]), int(torch.randint(0, N, (1,), generator=g)),
                        int(torch.randint(0, N, (1,), generator=g))], dtype=torch.int32)
    return x, tok, logprobs_ref(xs, tok, 20)


def _hists(n, rows=M + 2):
    c = torch.full((rows, L), SENT_C, dtype=torch.float32, device=DEV)
    i = torch.full((rows, L, max(n, 1)), SENT_I, dtype=torch.int32, device=DEV)
    t = torch.full((rows, L, max(n, 1)), SENT_T, dtype=torch.float32, device=DEV)
    return c, i, t


def _call(xd, tokd, N, n, hists, ws, pos, off):
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    c, i, t = hists
    Tops.logprobs_rows(xd[1:M + 1], tokd, N, n, c[1:M + 1], i[1:M + 1] if n else None, t[1:M + 1] if n else None, ws,
                       pos=pos, pos_off=off)


def _check_slot(hists, p, n, ref, what=""):
    """Position p of rows 1..M holds the mirror's results (ids exact, values to
    TOL, -inf exactly); everything else keeps its sentinel.  Returns the
    largest |device - mirror| over the finite values."""
    c, i, t = (h.cpu() for h in hists)
    chosen, ids, lps = ref
    err = 0.0
    got = c[1:M + 1, p]
    fin = torch.isfinite(chosen)
    assert torch.equal(got[~fin], chosen[~fin]), what
    if bool(fin.any()):
        err = max(err, float((got[fin].double() - chosen[fin].double()).abs().max()))
    if n:
        assert torch.equal(i[1:M + 1, p, :n], ids[:, :n]), what
        gt, wt = t[1:M + 1, p, :n], lps[:, :n]
        fin = torch.isfinite(wt)
        assert torch.equal(gt[~fin], wt[~fin]), what
        if bool(fin.any()):
            err = max(err, float((gt[fin].double() - wt[fin].double()).abs().max()))
    assert err <= TOL, (what, err)
    keep = torch.ones((M + 2, L), dtype=torch.bool)
    keep[1:M + 1, p] = False
    assert bool((c[keep] == SENT_C).all()), what
    wide = torch.ones(i.shape, dtype=torch.bool)
    wide[1:M + 1, p, :n] = False
    assert bool((i[wide] == SENT_I).all()) and bool((t[wide] == SENT_T).all()), what
    return err


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("N,ld", SIZES)
def test_kernel_against_mirror(N, ld, n):
    """Observed maximum |device - fp64 mirror| on an MI355X (``_check_slot`` returns it):
    9.5e-7 at N = 1000 and 1003, 2.4e-7 at N = 50257, 1.9e-6 (2^-19) at
    N = 128256, for every n; the bound is 2^-15 = 3.05e-5."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    x, tok, ref = _case(N, ld)
    xd, tokd = x.to(DEV), tok.to(DEV)
    ws = Tops.logprobs_workspace(M, N, n, DEV)
    pos = torch.full((M,), 3, dtype=torch.int32, device=DEV)
    hists = _hists(n)
    _call(xd, tokd, N, n, hists, ws, pos, 0)
    torch.cuda.synchronize()
    _check_slot(hists, 3, n, ref, "offset 0")
    assert torch.equal(_bits(xd), _bits(x))                    # the logits are only read, guards and [N, ld) included
    assert torch.equal(pos.cpu(), torch.full((M,), 3, dtype=torch.int32)) and torch.equal(tokd.cpu(), tok)
    assert bool((ws[:, :32] == 0).all())                           # the arrival counters are back at zero
    # a fused tail has advanced the position already: offset -1 writes the same slot, the same bits
    h2 = _hists(n)
    _call(xd, tokd, N, n, h2, ws, pos + 1, -1)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(hists, h2))
    # no position tensor: the offset alone is the position
    h3 = _hists(n)
    _call(xd, tokd, N, n, h3, ws, None, 3)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(hists, h3))
    # a position outside [0, L) writes nothing (and leaves the counters clean)
    h4 = _hists(n)
    _call(xd, tokd, N, n, h4, ws, torch.full((M,), L, dtype=torch.int32, device=DEV), 0)
    _call(xd, tokd, N, n, h4, ws, torch.zeros((M,), dtype=torch.int32, device=DEV), -1)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(h4, _hists(n)))
    assert bool((ws[:, :32] == 0).all())


def test_rows_at_different_positions_and_bad_token():
    """Every row writes its own position; a row outside [0, L) is skipped alone;
    a token outside the vocabulary gives NaN for the chosen value only."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    N, ld, n = 1003, 1024, 5
    x, tok, ref = _case(N, ld)
    xd = x.to(DEV)
    tok2 = tok.clone()
    tok2[4] = N  # one past the vocabulary: inside the row's padding, never read
    ws = Tops.logprobs_workspace(M, N, n, DEV)
    pos = torch.tensor([0, 5, 2, 6, 1], dtype=torch.int32, device=DEV)  # row 3: outside
    c, i, t = _hists(n)
    _call(xd, tok2.to(DEV), N, n, (c, i, t), ws, pos, 0)
    torch.cuda.synchronize()
    c, i, t = c.cpu(), i.cpu(), t.cpu()
    for r, p in enumerate(pos.cpu().tolist()):
        if p >= L:
            assert bool((c[r + 1] == SENT_C).all()) and bool((i[r + 1] == SENT_I).all())
            continue
        assert torch.equal(i[r + 1, p], ref[1][r, :n])
        assert float((t[r + 1, p].double() - ref[2][r, :n].double()).abs().max()) <= TOL
        if r == 4:
            assert bool(torch.isnan(c[r + 1, p]))
        else:
            assert abs(float(c[r + 1, p]) - float(ref[0][r])) <= TOL
        assert int((c[r + 1] != SENT_C).sum()) == 1  # NaN != sentinel counts as written


def test_minus_inf_reaches_the_list():
    """A row with 12 finite entries and n = 20: the -inf entries follow in index
    order with lp = -inf; a token at -inf has lp = -inf."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.sampling import logprobs_ref
    N, ld, n = 5003, 5056, 20
    g = torch.Generator().manual_seed(8)
    xs = torch.full((M, N), NINF).bfloat16()
    for r in range(M):
        cols = torch.randperm(N, generator=g)[:12]
        xs[r, cols] = (torch.randn(12, generator=g) * 2).bfloat16()
        xs[r, cols[:3]] = 1.5  # a three-way tie among the finite ones
    tok = torch.tensor([int((xs[r] == NINF).nonzero()[5 * r]) for r in range(M)], dtype=torch.int32)
    x = torch.full((M + 2, ld), SENT_X).bfloat16()
    x[1:M + 1, :N] = xs
    ref = logprobs_ref(xs, tok, n)
    assert bool((ref[2][:, 12:] == NINF).all()) and bool((ref[0] == NINF).all())
    assert torch.equal(ref[1][0, 12:].long(), (xs[0] == NINF).nonzero().flatten()[:8])
    hists = _hists(n)
    _call(x.to(DEV), tok.to(DEV), N, n, hists, Tops.logprobs_workspace(M, N, n, DEV), None, 2)
    torch.cuda.synchronize()
    _check_slot(hists, 2, n, ref)


def test_short_last_chunk_and_signed_zeros():
    """N = 2050, n = 20: the second chunk holds two entries, so its other 18
    candidate slots are empty in the merge.  Row 0 puts the row's two largest
    values there; row 1 is all zeros of both signs: the order is the one of the
    bf16 bits, +0.0 before -0.0, each by index (the mirror sorts on the same key)."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.sampling import logprobs_ref
    N, ld, n = 2050, 2056, 20
    g = torch.Generator().manual_seed(5)
    xs = (torch.randn(M, N, generator=g) * 3).bfloat16()
    xs[0, 2048], xs[0, 2049] = 20.0, 19.0
    xs[1] = 0.0
    xs[1, ::3] = -0.0
    xs[2, 2049] = NINF
    tok = torch.tensor([2049, 2049, 2049, 2048, 0], dtype=torch.int32)
    x = torch.full((M + 2, ld), SENT_X).bfloat16()
    x[1:M + 1, :N] = xs
    ref = logprobs_ref(xs, tok, n)
    assert ref[1][0, :2].tolist() == [2048, 2049]
    assert ref[1][1].tolist() == [i for i in range(N) if i % 3][:n] and float(ref[0][2]) == NINF
    hists = _hists(n)
    ws = Tops.logprobs_workspace(M, N, n, DEV)
    _call(x.to(DEV), tok.to(DEV), N, n, hists, ws, None, 0)
    torch.cuda.synchronize()
    _check_slot(hists, 0, n, ref)
    assert bool((ws[:, :32] == 0).all())


def test_calls_of_different_shapes_share_a_workspace():
    """One workspace sized for the largest call serves M = 2, then M = 5, then
    M = 2 rows (and other n and vocabulary sizes in between): a counter's place
    depends on the workspace alone, so no call's partial results land on another
    call's counters; every call gives the mirror's results and leaves every
    counter at zero."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    big = (50257, 50304)
    ws = Tops.logprobs_workspace(M + 1, big[0], 20, DEV)
    plan = [(2, big, 20), (5, big, 20), (2, big, 20), (5, (1003, 1024), 5), (3, big, 1), (5, big, 0), (1, big, 20),
            (4, (1000, 1024), 20), (5, big, 20)]
    for k, (rows, (N, ld), n) in enumerate(plan):
        x, tok, ref = _case(N, ld)
        xd, tokd = x.to(DEV), tok.to(DEV)
        c, i, t = _hists(n)
        Tops.logprobs_rows(xd[1:rows + 1], tokd, N, n, c[1:rows + 1], i[1:rows + 1] if n else None,
                           t[1:rows + 1] if n else None, ws, pos=None, pos_off=2)
        torch.cuda.synchronize()
        assert bool((ws[:, :32] == 0).all()), k
        c, i, t = c.cpu(), i.cpu(), t.cpu()
        fin = torch.isfinite(ref[0][:rows])
        assert torch.equal(c[1:rows + 1, 2][~fin], ref[0][:rows][~fin]), k
        assert float((c[1:rows + 1, 2][fin].double() - ref[0][:rows][fin].double()).abs().max()) <= TOL, k
        assert bool((c[rows + 1:] == SENT_C).all()) and bool((c[0] == SENT_C).all()), k
        if n:
            assert torch.equal(i[1:rows + 1, 2, :n], ref[1][:rows, :n]), k
            gt, wt = t[1:rows + 1, 2, :n], ref[2][:rows, :n]
            assert float((gt.double() - wt.double()).abs().max()) <= TOL, k
            assert bool((i[rows + 1:] == SENT_I).all()), k


# ---------------------------------------------------------------------- exact fixtures
@pytest.mark.parametrize("N,ld", [(50257, 50304), (128256, 128256)])
def test_one_hot_rows_are_exact(N, ld):
    """One entry a = 8.0 per row, every other an integer in [-150, -121]:
    exp(x - a) is exactly 0 in fp32 in the entry's own chunk, and every other
    chunk's sum is scaled by exp(m - a) = 0 in the merge, so sum = 1, log = 0:
    lp is bitwise +0 for the maximum and bitwise x_i - a elsewhere, wherever
    the entry lies among the chunks (first and last column, both sides of a
    chunk boundary, a middle chunk).  tests/test_logprobs.py checks the
    preconditions in fp32 on the host."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.sampling import logprobs_ref
    n = 20
    g = torch.Generator().manual_seed(N)
    xs = torch.randint(-150, -120, (M, N), generator=g).float()
    hot = [0, N - 1, 2047, 2048, (N // 2048 // 2) * 2048 + 1001]
    for r, c in enumerate(hot):
        xs[r, c] = 8.0
    xs = xs.bfloat16()
    assert torch.equal(xs.float(), xs.float().round())
    # rows 0..2 ask for the maximum itself, rows 3..4 for another entry
    tok = torch.tensor([hot[0], hot[1], hot[2], 5, N - 3], dtype=torch.int32)
    x = torch.full((M + 2, ld), SENT_X).bfloat16()
    x[1:M + 1, :N] = xs
    hists = _hists(n)
    _call(x.to(DEV), tok.to(DEV), N, n, hists, Tops.logprobs_workspace(M, N, n, DEV), None, 4)
    torch.cuda.synchronize()
    c, i, t = (h.cpu() for h in hists)
    want_c = xs.float()[torch.arange(M), tok.long()] - 8.0
    assert torch.equal(_bits(c[1:M + 1, 4]), _bits(want_c))            # bitwise: +0.0 for rows 0..2
    assert _bits(c[1:M + 1, 4])[:3].tolist() == [0, 0, 0]
    ids = logprobs_ref(xs, tok, n)[1]                                  # the tie rule on exact integers
    assert ids[:, 0].tolist() == hot
    assert torch.equal(i[1:M + 1, 4], ids)
    assert torch.equal(_bits(t[1:M + 1, 4]), _bits(xs.float().gather(1, ids.long()) - 8.0))
    assert int(_bits(t[1:M + 1, 4])[:, 0].abs().sum()) == 0


# ---------------------------------------------------------------------- rejections
def test_rejections():
    from distributed_neural_networks_amd.ops import _lib
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    N, ld, n = 1000, 1024, 5
    x, tok, _ = _case(N, ld)
    xd, tokd = x.to(DEV), tok.to(DEV)
    rows = xd[1:M + 1]
    c, i, t = (h[1:M + 1] for h in _hists(n))
    ws = Tops.logprobs_workspace(M, N, n, DEV)
    f = Tops.logprobs_rows
    with pytest.raises(ValueError, match="n = 21"):
        f(rows, tokd, N, 21, c, i, t, ws)
    with pytest.raises(ValueError, match="n = -1"):
        f(rows, tokd, N, -1, c, i, t, ws)
    with pytest.raises(TypeError):
        f(rows.float(), tokd, N, n, c, i, t, ws)                       # the wrong dtype
    with pytest.raises(TypeError):
        f(rows[:, ::2], tokd, 8, n, c, i, t, ws)                       # a strided last dimension
    with pytest.raises(ValueError):
        f(rows[:, 1:], tokd, 8, n, c, i, t, ws)                        # rows not 16-byte aligned
    with pytest.raises(ValueError):
        f(rows, tokd, ld + 1, n, c, i, t, ws)                          # the vocabulary past the row
    with pytest.raises(ValueError, match="chosen"):
        f(rows, tokd, N, n, c[:M - 1], i, t, ws)                       # histories too small: rows
    with pytest.raises(ValueError, match="top_ids"):
        f(rows, tokd, N, n, c, i[:, :, :n - 1].contiguous(), t, ws)    # ... alternatives
    with pytest.raises(ValueError, match="top_lps"):
        f(rows, tokd, N, n, c, i, t[:, :L - 1].contiguous(), ws)       # ... positions
    with pytest.raises(ValueError, match="top_ids"):
        f(rows, tokd, N, n, c, i.float(), t, ws)
    with pytest.raises(ValueError, match="top_ids and top_lps"):
        f(rows, tokd, N, n, c, None, None, ws)
    with pytest.raises(ValueError, match="tokens"):
        f(rows, tokd.long(), N, n, c, i, t, ws)
    with pytest.raises(ValueError, match="tokens"):
        f(rows, tokd[:M - 1], N, n, c, i, t, ws)
    with pytest.raises(ValueError, match="pos"):
        f(rows, tokd, N, n, c, i, t, ws, pos=torch.zeros(M, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="workspace"):
        f(rows, tokd, N, n, c, i, t, ws[:M - 1])                       # fewer blocks than rows
    with pytest.raises(ValueError, match="workspace"):
        f(rows, tokd, N, n, c, i, t, ws.flatten())
    with pytest.raises(ValueError, match="workspace"):
        f(rows, tokd, N, n, c, i, t, ws[:, :32])                       # strided blocks
    with pytest.raises(ValueError, match="workspace"):
        f(rows, tokd, N, 20, *(h[1:M + 1] for h in _hists(20)), ws)    # sized for n = 5
    with pytest.raises(ValueError, match="logprobs_workspace"):
        Tops.logprobs_workspace(M, 103 * 2048, n, DEV)
    assert ws.shape == (M, 64) and Tops.logprobs_workspace(3, 50257, 20, DEV).shape == (3, 1088)
    # the library's own checks
    g, s = _lib.lib().logprobs_rows, _lib.stream_ptr()
    a = dict(x=rows.data_ptr(), ld=ld, M=M, N=N, tok=tokd.data_ptr(), pos=0, pos_off=0, n=n, lp_hist=c.data_ptr(),
             top_id_hist=i.data_ptr(), top_lp_hist=t.data_ptr(), hist_ld=L, top_ld=n, ws=ws.data_ptr(),
             ws_rows=M, ws_ld=ws.shape[1], st=s)
    for bad in (dict(x=0), dict(tok=0), dict(lp_hist=0), dict(ws=0), dict(ld=ld - 4), dict(ld=N - 8), dict(n=21),
                dict(n=-1), dict(top_id_hist=0), dict(top_lp_hist=0), dict(top_ld=n - 1), dict(hist_ld=0),
                dict(ws_rows=M - 1), dict(ws_ld=32), dict(ws_ld=ws.shape[1] + 8), dict(ws=ws.data_ptr() + 2),
                dict(x=rows.data_ptr() + 2)):
        assert g(**dict(a, **bad)) == -1, bad
    assert g(**dict(a, N=103 * 2048, ld=103 * 2048, ws_ld=1 << 20)) == -2  # more chunks than candidate slots
    assert g(**dict(a, M=0)) == 0
    torch.cuda.synchronize()
    assert bool((c == SENT_C).all()) and bool((ws == 0).all())           # nothing above ran a kernel


# ---------------------------------------------------------------------- replay hygiene
def test_back_to_back_calls_and_graph_replays():
    """The workspace and its counters are left clean: two calls in a row and a
    captured graph replayed three times give the same bits."""
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.graph import GraphedStep
    N, ld, n = 50257, 50304, 20
    x, tok, ref = _case(N, ld)
    xd, tokd = x.to(DEV), tok.to(DEV)
    ws = Tops.logprobs_workspace(M, N, n, DEV)
    pos = torch.full((M,), 1, dtype=torch.int32, device=DEV)
    first = _hists(n)
    _call(xd, tokd, N, n, first, ws, pos, 0)
    second = _hists(n)
    _call(xd, tokd, N, n, second, ws, pos, 0)
    torch.cuda.synchronize()
    _check_slot(first, 1, n, ref)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, second))
    hists = _hists(n)
    graph = GraphedStep(lambda: _call(xd, tokd, N, n, hists, ws, pos, 0), torch.device(DEV, 0), warmup=1)
    for k in range(3):
        for h, fresh in zip(hists, _hists(n)):
            h.copy_(fresh)  # the replay itself must write the slot again
        graph()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, hists)), k
        assert bool((ws[:, :32] == 0).all())


# ---------------------------------------------------------------------- the last stage and the rings
KINDS = {"greedy": {}, "sampled": dict(temperature=0.8, top_k=20, top_p=0.9, seed=5),
         "penalised": dict(temperature=0.8, top_k=20, top_p=0.9, seed=5, repetition_penalty=2.0,
                           frequency_penalty=0.25, presence_penalty=0.5),
         "greedy_penalised": dict(repetition_penalty=2.0, frequency_penalty=0.25, presence_penalty=0.5)}


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


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("model", ["gpt2-tiny", LP_MODEL])
def test_stage_records_the_mirror_of_its_own_logits(model, kind):
    """Eager steps of the last stage (the prefill's first token, then decode
    steps): the bound histories hold, at the position the token was sampled at,
    the mirror of the stage's own logits row (``StageOutput.probs``, after the
    penalties) and token."""
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.runtime.sampling import logprobs_ref
    n, B, T, steps = 5, 3, 5, 4
    first, last = _stages(model, B, 32, logprobs=n, **KINDS[kind])
    assert last.logprobs == n and first.logprobs == 0 and first.lp_ws is None and last.lp_ws is not None
    V = model_info(model).cfg.vocab_size
    g = torch.Generator().manual_seed(31)
    prompt = torch.randint(0, V, (B, T), generator=g)
    prompt[:, 3] = prompt[:, 1]
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    x = prompt.to(device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError, match="no bind_logprobs"):
        last.step(first.step(x, pos, B, T), pos, B, T)
    c = torch.full((B, 32), SENT_C, dtype=torch.float32, device=DEV)
    i = torch.full((B, 32, n), SENT_I, dtype=torch.int32, device=DEV)
    t = torch.full((B, 32, n), SENT_T, dtype=torch.float32, device=DEV)
    last.bind_logprobs(0, c, i, t)
    if last.penalties_on:
        last.penalty_begin(0, prompt)
    written = []
    for s in range(steps + 1):
        Tn = T if s == 0 else 1
        y = last.step(first.step(x, pos, B, Tn), pos, B, Tn)
        torch.cuda.synchronize()
        p = int(pos[0]) + Tn - 1
        written.append(p)
        chosen, ids, lps = logprobs_ref(y.probs, y.pred, n)
        assert torch.equal(i[:, p].cpu(), ids), (s, p)
        assert float((c[:, p].cpu().double() - chosen.double()).abs().max()) <= TOL, (s, p)
        assert float((t[:, p].cpu().double() - lps.double()).abs().max()) <= TOL, (s, p)
        if "temperature" not in KINDS[kind]:  # greedy: the token heads its own list
            assert torch.equal(ids[:, 0], y.pred.cpu()) and torch.equal(_bits(c[:, p]), _bits(t[:, p, 0]))
        pos += Tn
        x = y.pred.view(B, 1).clone()
    assert written == list(range(T - 1, T + steps))
    keep = torch.ones(32, dtype=torch.bool)
    keep[written] = False
    assert bool((c[:, keep] == SENT_C).all()) and bool((i[:, keep] == SENT_I).all()) and \
        bool((t[:, keep] == SENT_T).all())


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("model", ["gpt2-tiny", LP_MODEL])
def test_rings_agree(model, kind):
    """Eager, single-step graphs, K = 8 steps per graph (11 tokens: one K-step
    replay and two single steps) and, when sampling, the unfused step tail: the
    same tokens and bitwise the same histories (the same kernel on the same
    bits; the fused tail's position offset and the unfused one address the same
    slot).  The warm-up and capture runs write positions past the current one,
    as they do in the token history; the replay overwrites each before it is
    read, so nothing of them shows.  A second prefill starts a clean history."""
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    n, Mb, B, T, steps, K = 5, 2, 3, 5, 11, 8
    V = model_info(model).cfg.vocab_size
    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(0, V, (B, T), generator=g) for _ in range(Mb)]
    for p in prompts:
        p[:, 3] = p[:, 1]

    def generate(graphs, ms, nlp=n):
        st = _stages(model, Mb * B, T + steps + K + 2, logprobs=nlp, **KINDS[kind])
        ring = DecodeRing(st, RingLinks(), 1, Mb, B, use_graphs=graphs, multi_step=ms)
        toks = ring.generate(prompts, T, steps)
        torch.cuda.synchronize()
        return toks, ring

    ref, ring0 = generate(False, 0)
    lp0 = ring0.logprobs()
    assert lp0["chosen"].shape == (Mb * B, steps) and lp0["top_ids"].shape == (Mb * B, steps, n) and \
        lp0["top_lps"].shape == (Mb * B, steps, n) and not lp0["chosen"].is_cuda
    assert bool(torch.isfinite(lp0["chosen"]).all()) and bool((lp0["chosen"] <= 0).all())
    assert bool((lp0["top_lps"][..., :-1] >= lp0["top_lps"][..., 1:]).all())
    assert bool((lp0["chosen"][..., None] <= lp0["top_lps"][..., :1] + 0).all())
    if "temperature" not in KINDS[kind]:
        assert torch.equal(lp0["top_ids"][..., 0], ref) and torch.equal(lp0["chosen"], lp0["top_lps"][..., 0])
    one, ring1 = generate(True, 0)
    assert ring1.graph_k is None and ring1.graphs
    multi, ringk = generate(True, K)
    assert ringk.graph_k is not None and ringk.graph_k_steps == K
    rings = {"single-step graphs": (one, ring1), "K-step graph": (multi, ringk)}
    if "temperature" in KINDS[kind]:
        assert Tops.SAMPLE_FUSED_TAIL
        Tops.SAMPLE_FUSED_TAIL = False
        try:
            unfused, ringu = generate(True, 0)
            assert ringu.hist is None
        finally:
            Tops.SAMPLE_FUSED_TAIL = True
        rings["unfused tail"] = (unfused, ringu)
    for name, (toks, ring) in rings.items():
        assert torch.equal(toks, ref), name
        lp = ring.logprobs()
        for k in lp0:
            assert torch.equal(_bits(lp[k]), _bits(lp0[k])), (name, k)
    # logprobs = 0: nothing allocated, the same tokens
    off, ring_off = generate(True, K, nlp=0)
    assert torch.equal(off, ref)
    assert ring_off.stages[-1].lp_ws is None and ring_off.lp_chosen is None and ring_off.lp_top_ids is None and \
        ring_off.lp_top_lps is None and ring_off.stages[-1].logprobs == 0
    with pytest.raises(ValueError, match="records none"):
        ring_off.logprobs()
    # a second, shorter generation on the K-step ring: a clean history aligned with its own tokens
    again = ringk.generate(prompts, T, 4)
    torch.cuda.synchronize()
    assert torch.equal(again, ref[:, :4])
    lp2 = ringk.logprobs()
    for k in lp0:
        assert torch.equal(_bits(lp2[k]), _bits(lp0[k][:, :4])), k
    assert int((ringk.lp_chosen[0][:, T + 3:] != 0).sum()) == 0  # nothing of the first generation is left


def test_neutral_key_and_arguments():
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage, build_device_stage
    model = "gpt2-tiny"
    ranges, sds = _weights(model)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 512, (2, 16), generator=g)]
    toks = []
    for kw in ({}, dict(logprobs=0)):
        st = [TransformerStage(model, sds[i], a, b, i == 0, i == 1, DEV, max_batch=2, max_seq=32, **kw)
              for i, (a, b) in enumerate(ranges)]
        assert st[1].logprobs == 0 and st[1].lp_ws is None
        ring = DecodeRing(st, RingLinks(), 1, 1, 2, use_graphs=False)
        assert ring.lp_chosen is None
        toks.append(ring.generate(prompts, 16, 5))
    assert torch.equal(toks[0], toks[1])
    a, b = ranges[1]
    on = build_device_stage(model, sds[1], a, b, False, True, DEV, max_batch=4, max_seq=32, logprobs=20)
    assert on.logprobs == 20 and on.lp_ws.dtype == torch.int32 and int(on.lp_ws.abs().sum()) == 0
    for bad in (-1, 21, 2.5, True):
        with pytest.raises(ValueError, match="logprobs must be an integer"):
            TransformerStage(model, sds[1], a, b, False, True, DEV, max_batch=2, max_seq=32, logprobs=bad)
    c = torch.zeros((2, 32), dtype=torch.float32, device=DEV)
    i = torch.zeros((2, 32, 20), dtype=torch.int32, device=DEV)
    t = torch.zeros((2, 32, 20), dtype=torch.float32, device=DEV)
    on.bind_logprobs(2, c, i, t)
    for args in ((3, c, i, t), (0, c, i[:, :, :5].contiguous(), t), (0, c, i, t[:, :31].contiguous()),
                 (0, c.double(), i, t), (0, c.cpu(), i.cpu(), t.cpu())):
        with pytest.raises(ValueError, match="bind_logprobs"):
            on.bind_logprobs(*args)
    # lanes are not supported with log-probabilities: a clear error
    first = TransformerStage(model, sds[0], *ranges[0], True, False, DEV, max_batch=4, max_seq=32)
    with pytest.raises(ValueError, match="lanes"):
        DecodeRing([first, on], RingLinks(), 1, 2, 2, lanes=2)


# ---------------------------------------------------------------------- the config key reaches the device stages
def test_cli_colocated_logprobs_line(tmp_path):
    """``node.py`` on a colocated 2-stage config with ``logprobs``: the
    ``LOGPROBS`` line next to the tokens holds what a ring of stages built with
    the same arguments records, bit for bit (the line's numbers read back exactly)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model, ids, steps, Mb, B, n = "gpt2-tiny", [5, 17, 99, 17, 42, 17, 1, 250], 6, 2, 2, 3
    ports = []
    for _ in range(2):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            ports.append(sk.getsockname()[1])
    samp = dict(temperature=0.8, top_k=20, top_p=0.9, seed=7)
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{ports[i]}", "part_index": i, "device": 0}
                   for i in range(2)],
         "model_weights": "synthetic:3", "num_parts": 2, "return_to_node_id": "node1", "transport": "colocated",
         "model": model, "seq_len": 32, "decode_steps": steps, "micro_batch_size": B, "num_microbatches": Mb,
         "logprobs": n}
    c.update(samp)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(c))
    r = subprocess.run([sys.executable, os.path.join(root, "node.py"), "--node_id", "node1", "--config", str(cfg),
                        "--prompt", ",".join(map(str, ids))], env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    toks = torch.tensor(json.loads(r.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    line = json.loads(r.stdout.split("LOGPROBS ")[1].splitlines()[0])
    T = len(ids)
    ranges = default_ranges(model, 2)
    st = [build_device_stage(model, ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 3, device=DEV), a, b,
                             i == 0, i == 1, torch.device(DEV, 0), max_batch=Mb * B, max_seq=T + steps,
                             max_tokens=B * (T + steps), logprobs=n, **samp) for i, (a, b) in enumerate(ranges)]
    prompt = torch.tensor([ids]).repeat(B, 1)
    ring = DecodeRing(st, RingLinks(), 1, Mb, B)
    want_t = ring.generate([prompt] * Mb, T, steps)
    torch.cuda.synchronize()
    want = ring.logprobs()
    assert torch.equal(toks, want_t)
    assert line["n"] == n and line["top_ids_seq0"] == want["top_ids"][0].tolist()
    assert torch.equal(torch.tensor(line["chosen"], dtype=torch.float32), want["chosen"])
    assert torch.equal(torch.tensor(line["top_logprobs_seq0"], dtype=torch.float32), want["top_lps"][0])
    assert "top_ids" not in line  # every sequence's top-n only on request (DNN_LOGPROBS_ALL=1)
