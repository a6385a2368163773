"""Prompt log-probabilities on the device (csrc/kernels/head_lse.hip, ops/gemm.py
head_lse): the head GEMM with the log-sum-exp, the argmax and the target's
logit in its epilogue, against a plain fp64 reference on the same operands.

The log-sum-exp band (``_lse_band``), with e = 2^-24, for a row of V logits:
  * a term exp(t), t = l - max <= 0, is one v_exp_f32 of t * log2(e): the
    product's rounding moves the exponent by |t| e relative, the instruction
    adds about one ulp, and terms with |t| > 88 are below the sum's last bit:
    at most 90 e relative per term;
  * adding V positive terms in fp32 in any order: at most V e relative;
  * the running sum is rescaled when the max moves, at most once per 128-column
    tile and slice merge, each by a factor with the 90 e above: (V / 128 + 1) *
    90 e <= (V + 128) e;
  * log of the sum, the two subtractions of (l - max) - log(sum), each within
    an ulp or two of values bounded by 2 max|l| + ln V.
So |lp - lp64| <= (2 V + 128 + 90 + 8 (1 + 2 max|l| + ln V)) e.  On exact
operands (every product and partial sum a multiple of 2^-7 below 2^17, the
fold's factors powers of two) the fp32 logit is the fp64 logit, so its bf16
rounding is too, and the band above is the whole error.  On random operands
an fp32-accumulated logit may round to the neighbouring bf16: one bf16 ulp of
the row's largest |logit| is added."""
import math

import pytest
import torch
from test_prompt_logprobs import LENS, R_CHUNK, R_STEPS, R_T, check_ring, ring_ids

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KEEP = 777.0  # what an output slot holds before the call

# (M, V, d, head form): row-block edges and more than one block; vocabularies that are no tile multiple,
# with two or more slices, and V = 100 with a single one; one, 12 and 25 K steps; the four head forms
CASES = [(1, 1000, 128, "ln"), (127, 4099, 768, "rms"), (129, 1000, 1600, "plain_bias"), (300, 4099, 128, "plain"),
         (300, 100, 768, "ln"), (129, 4099, 1600, "ln")]


def _lse_band(V, mag):
    return (2 * V + 128 + 90 + 8 * (1 + 2 * mag + math.log(V))) * 2.0 ** -24


def _guarded(t, pad_rows=1, pad_cols=8, fill=float("nan")):
    """``t`` inside a larger poisoned buffer (16-byte aligned rows): (view, buffer)."""
    if t.dim() == 1:
        buf = torch.full((t.numel() + 8,), fill, dtype=t.dtype, device=DEV)
        buf[4:4 + t.numel()] = t
        return buf[4:4 + t.numel()], buf
    buf = torch.full((t.shape[0] + 2 * pad_rows, t.shape[1] + pad_cols), fill, dtype=t.dtype, device=DEV)
    buf[pad_rows:pad_rows + t.shape[0], :t.shape[1]] = t
    return buf[pad_rows:pad_rows + t.shape[0], :t.shape[1]], buf


def _targets(M, V):
    from distributed_neural_networks_amd.ops._lib import lib
    ns = lib().head_lse_slices(M, V)
    ntile = -(-V // 128)
    per = -(-ntile // ns) * 128  # first column of the second slice
    cyc = [V - 1, -1, 0, 127, 128, per - 1, per, V // 2, -1, V + 5]  # V + 5: outside the vocabulary, "nothing"
    cols = [cyc[i % len(cyc)] for i in range(M)]
    return torch.tensor([c if c < V or c == V + 5 else V - 1 for c in cols], dtype=torch.int32, device=DEV)


def _run(x, w, form, target, rowstat=None, fold=(None, None)):
    """One head_lse call with every buffer guarded; returns (tok_lp, top_id, top_lp) per row, the slot of a
    row that must stay unwritten holding KEEP, after the guards have been checked."""
    from distributed_neural_networks_amd.ops.gemm import FoldedLinear, head_lse, head_lse_workspace
    M, V = x.shape[0], w.shape[0]
    xv, _ = _guarded(x)
    wv, _ = _guarded(w)
    colsum, bias = fold
    gb = None if bias is None else _guarded(bias)
    gc = None if colsum is None else _guarded(colsum)
    ws_need = head_lse_workspace(M, V, DEV).numel()
    wsb = torch.full((ws_need + 64,), KEEP, dtype=torch.float32, device=DEV)
    out_idx = (4 + torch.randperm(M, device=DEV)).to(torch.int32)  # a scatter, with four guard slots either side
    outs = [torch.full((M + 8,), int(KEEP), dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.float32)]
    if form in ("ln", "rms"):
        f = FoldedLinear(wv, None if gb is None else gb[0], None if gc is None else gc[0], 2 if form == "ln" else 1,
                         1e-5)
        stats = torch.full((2 * M + 16,), KEEP, dtype=torch.float32, device=DEV)
        head_lse(xv, f, target, out_idx, *outs, wsb[:ws_need], stats=stats, rowstat=rowstat)
        if rowstat is None:
            rowstat = stats[:2 * M].view(M, 2).clone()
        assert (stats[2 * M:] == KEEP).all()
    else:
        head_lse(xv, wv, target, out_idx, *outs, wsb[:ws_need], bias=None if gb is None else gb[0])
    torch.cuda.synchronize()
    assert (wsb[ws_need:] == KEEP).all(), "workspace guard overwritten"
    for o in outs:
        assert (o[:4] == KEEP).all() and (o[M + 4:] == KEEP).all(), "output guard overwritten"
    idx = out_idx.long()
    return [o[idx] for o in outs], rowstat


def _reference(x, w, rowstat, colsum, bias, target, dev=DEV):
    """fp64 on the same operands, the logits rounded to bf16: (logits64, tok_lp, top_id, top_lp, raw top-2 gap)."""
    V = w.shape[0]
    l = x.double() @ w.double().t()
    if rowstat is not None:
        l = l * rowstat[:, :1].double()
        if colsum is not None:
            l = l + rowstat[:, 1:].double() * colsum.double()[None]
    if bias is not None:
        l = l + bias.double()[None]
    top2 = l.topk(min(2, V), dim=1).values
    lb = l.float().bfloat16().double()
    lse = torch.logsumexp(lb, dim=1)
    mx = lb.max(dim=1, keepdim=True).values
    ar = torch.arange(V, device=dev)[None].expand_as(lb)
    top_id = torch.where(lb == mx, ar, V).min(dim=1).values  # ties: the smallest index
    tg = target.long().clamp(0, V - 1)
    tok_lp = lb.gather(1, tg[:, None])[:, 0] - lse
    return lb, tok_lp, top_id, mx[:, 0] - lse, top2


def _check(got, ref, target, V, extra_ulp):
    (tok_lp, top_id, top_lp), (lb, r_tok, r_id, r_top, top2) = got, ref
    live = (target >= 0) & (target < V)
    assert (tok_lp[~live] == KEEP).all() and (top_id[~live] == int(KEEP)).all() and (top_lp[~live] == KEEP).all(), \
        "a row with no target wrote"
    amax = lb.abs().max(dim=1).values
    band = torch.tensor([_lse_band(V, a) for a in amax.tolist()], dtype=torch.float64, device=DEV)
    ulp = torch.exp2(torch.floor(torch.log2(amax.clamp(min=2.0 ** -126))) - 7)
    if extra_ulp:
        band = band + ulp
    e_tok, e_top = (tok_lp.double() - r_tok).abs()[live], (top_lp.double() - r_top).abs()[live]
    print(f"V={V} rows={int(live.sum())}: worst tok_lp error {e_tok.max().item():.3g}, top_lp {e_top.max().item():.3g}, "
          f"smallest band {band[live].min().item():.3g}")
    assert torch.isfinite(tok_lp[live]).all() and (e_tok <= band[live]).all()
    assert (e_top <= band[live]).all()
    if extra_ulp:  # rows whose two largest logits are within one bf16 ulp may resolve either way
        close = (top2[:, 0] - top2[:, -1]) <= ulp
        assert int(close.sum()) <= 0.02 * lb.shape[0], f"{int(close.sum())} of {lb.shape[0]} rows left out"
        live = live & ~close
    assert torch.equal(top_id[live].long(), r_id[live])


def _fold(form, w, g):
    V = w.shape[0]
    bias = (torch.randint(-8, 9, (V,), generator=g) / 4.0).float() if form in ("ln", "plain_bias") else None
    colsum = w.float().sum(dim=1) if form == "ln" else None
    return colsum, bias


def _exact_case(M, V, d, form):
    """Sparse operands on a grid of quarters, power-of-two row statistics {rstd, -mean rstd}: rstd 1/2 or 2,
    mean 1/4 (RMS: no shift).  Made on the host, so the same numbers on every device."""
    g = torch.Generator().manual_seed(M * 7 + V)
    x = (torch.randint(-4, 5, (M, d), generator=g) / 4.0).bfloat16()
    w = torch.randint(-4, 5, (V, d), generator=g) / 4.0
    w = (w * (torch.rand(V, d, generator=g) < 16.0 / d)).bfloat16()  # about 16 terms per dot product
    colsum, bias = _fold(form, w, g)
    rowstat = None
    if form in ("ln", "rms"):
        rstd = torch.where(torch.arange(M) % 2 == 0, 0.5, 2.0)
        rowstat = torch.stack([rstd, -0.25 * rstd if form == "ln" else torch.zeros_like(rstd)], dim=1).float()
    return x, w, colsum, bias, rowstat


def _random_case(M, V, d, form):
    """Random rows, each leaning towards one column of a random head as a language model's do: that column's
    logit stands about 8 above a noise of about 1, so few rows have their two largest logits within a bf16 ulp
    (the share is asserted by ``_check``)."""
    g = torch.Generator().manual_seed(1000 + M + V + d)
    w = (torch.randn(V, d, generator=g) / d ** 0.5).bfloat16()
    wc = w.float()[torch.randint(0, V, (M,), generator=g)]
    x = (0.5 + torch.randn(M, d, generator=g) + 8.0 * wc / wc.pow(2).sum(1, keepdim=True)).bfloat16()
    return (x, w) + _fold(form, w, g) + (None,)


def _dev(*ts):
    return [None if t is None else t.to(DEV).contiguous() for t in ts]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("M,V,d,form", CASES)
def test_against_fp64(M, V, d, form, kind):
    """exact: every fp32 logit is the fp64 logit, so top_id is the reference's (ties included) and the values
    differ by the log-sum-exp band alone.  random: the device's own row statistics, one bf16 ulp more, and two
    runs are the same bits."""
    x, w, colsum, bias, rowstat = _dev(*(_exact_case if kind == "exact" else _random_case)(M, V, d, form))
    target = _targets(M, V)
    got, rowstat = _run(x, w, form, target, rowstat=rowstat, fold=(colsum, bias))
    if kind == "random":
        again, _ = _run(x, w, form, target, fold=(colsum, bias))
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    _check(got, _reference(x, w, rowstat, colsum, bias, target), target, V, extra_ulp=kind == "random")


def test_rejections():
    """Every rejected call returns -1 and leaves the outputs alone."""
    from distributed_neural_networks_amd.ops._lib import lib, stream_ptr
    M, V, d = 5, 300, 128
    x = torch.zeros((M, d), dtype=torch.bfloat16, device=DEV)
    w = torch.zeros((V, d), dtype=torch.bfloat16, device=DEV)
    f32 = torch.zeros((V + 2 * M,), dtype=torch.float32, device=DEV)
    tgt = torch.zeros((M,), dtype=torch.int32, device=DEV)
    ws = torch.zeros((M * lib().head_lse_slices(M, V) * 4,), dtype=torch.float32, device=DEV)
    outs = [torch.full((M,), int(KEEP), dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.float32)]
    ok = dict(A=x.data_ptr(), lda=d, W=w.data_ptr(), ldw=d, rowstat=f32.data_ptr(), colsum=f32.data_ptr(),
              bias=f32.data_ptr(), target=tgt.data_ptr(), out_idx=tgt.data_ptr(), M=M, V=V, d=d, ws=ws.data_ptr(),
              ws_bytes=ws.numel() * 4, tok_lp=outs[0].data_ptr(), top_id=outs[1].data_ptr(),
              top_lp=outs[2].data_ptr(), out_len=M, st=stream_ptr())
    bad = [dict(A=0), dict(W=0), dict(target=0), dict(out_idx=0), dict(ws=0), dict(tok_lp=0), dict(top_id=0),
           dict(top_lp=0), dict(d=96), dict(d=0), dict(lda=d - 8), dict(ldw=d - 8), dict(lda=d + 4),
           dict(A=x.data_ptr() + 2), dict(W=w.data_ptr() + 8), dict(bias=f32.data_ptr() + 4),
           dict(ws=ws.data_ptr() + 4), dict(M=0), dict(V=0), dict(rowstat=0), dict(ws_bytes=ws.numel() * 4 - 16),
           dict(out_len=0)]
    for b in bad:
        assert lib().head_lse(**{**ok, **b}) == -1, b
    torch.cuda.synchronize()
    for o in outs:
        assert (o == KEEP).all()
    assert lib().head_lse(**ok) == 0  # the unmodified call is accepted
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- end to end: chunked prompts on a ring
@pytest.mark.parametrize("lens", [LENS, None], ids=["ragged", "equal"])
@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_ring_chunked(model, lens):
    """``ring.prompt_logprobs()`` against the fp64 log-softmax of the stages' own all-position logits of the same
    prefill pieces (``check_ring``, the random case's band); tokens and ``logprobs`` are those of the run with
    the key off."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    V, n, B = model_info(model).cfg.vocab_size, model_info(model).num_layers, len(LENS)
    ranges = [(0, n // 2 - 1), (n // 2, n - 1)]
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 7, nontrivial=True) for i, (a, b) in enumerate(ranges)]

    def stages(**last_kw):
        return [TransformerStage(model, sds[i], a, b, i == 0, i == 1, DEV, max_batch=B, max_seq=R_T + R_STEPS + 10,
                                 **(last_kw if i == 1 else {})) for i, (a, b) in enumerate(ranges)]
    ls = lens or [R_T] * B
    ids = ring_ids(V, ls)
    res = {}
    for key in (0, 1):
        ring = DecodeRing(stages(logprobs=3, prompt_logprobs=key), RingLinks(), 1, 1, B, early_exit=False)
        toks = ring.generate([ids], R_T, R_STEPS, R_CHUNK, lens=None if lens is None else [torch.tensor(lens)])
        torch.cuda.synchronize()
        res[key] = (toks, ring.logprobs(), ring)
    assert torch.equal(res[0][0], res[1][0])
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k
    s0, s1 = stages()
    pos = torch.zeros((B,), dtype=torch.int32, device=DEV)
    lg = torch.empty((B, R_T, V), dtype=torch.float64)
    for t0 in range(0, R_T, R_CHUNK):
        Tc = min(R_CHUNK, R_T - t0)
        h = s0.step(ids[:, t0:t0 + Tc].to(DEV, torch.int32).contiguous(), pos, B, Tc)
        lg[:, t0:t0 + Tc] = s1.step(h, pos, B, Tc, last_only=False).probs.double().reshape(B, Tc, V).cpu()
        pos += Tc
    check_ring(res[1][2].prompt_logprobs()[0], lg, ids, ls, _lse_band)
