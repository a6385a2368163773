"""Fused fp32 units 2-3 (``cifar_fc1_head_x3``): fc1 with fc2 in its epilogue, partial logits in a
(2,M,16) workspace, then the finish kernel (bias, softmax, argmax).  The hidden rows never exist.

Shapes (M, 512, K): K = 32, 64, 96 are nk = 1, 2, 3, the barrier-count edges of the two wave groups;
M = 1, 255, 257, 300 the row edges and the two-M-tile case; K = 4096 the workload's depth.  Both A
encodings (``split_in``).

* exact: fc1 operands from ``cifar_exact.fc1_fixture``, fc2 from ``cifar_fc1_head_fixtures.exact_fc2``
  (per class every term a multiple of one quantum and sum|terms| + |bias| < 2^24 quanta, asserted
  there in fp64; wide fc2 rows need ``w_lo``, hidden values need ``hid_lo``; classes 3 and 7 are
  identical).  Every logit is then exact in any summation order, so ``probs`` and ``pred`` must be
  bitwise those of ``cifar_fc1_x3`` + ``cifar_head_tail_x3``, and ``pred`` the first-index argmax of the
  exact logits (the fp64 sum of the three terms the kernels form; the part of a hidden value below
  ``hid_lo`` is dropped by both paths).
* random data against fp64 (fp64 fc1, fp64 fc2, fp64 softmax).  The logit error bound E (per row,
  the largest over classes) comes from the number formats, not from the kernels.  bf16 keeps 8
  significant bits, so a rounding to it is off by at most 2^-9 relative: |x_lo| <= 2^-9 |x| and
  |x - x_hi - x_lo| <= 2^-18 |x|.  A product of the three-term split is therefore off by at most
  eps = 3 * 2^-18 of |a w| (the dropped lo*lo term and the two operands' split residues, 2^-18
  each), and each of the 3 K / 32 fp32 accumulations of an MFMA chain rounds by at most 2^-24 of
  a partial sum, itself at most S = sum|a w| + |b|.  A worst-case sum of these over K = 4096 and
  again over 512 columns bounds a logit to about 0.1 and decides nothing, so the errors are taken
  as independent, zero-mean and bounded as above; by Hoeffding's inequality their sum passes
  LAM sqrt(sum of squared bounds) with probability below 2 exp(-LAM^2 / 2), 3e-8 at LAM = 6,
  against the 2e5 logits the largest test checks:
      d hid = LAM (eps sqrt(sum (a w)^2) + 2^-24 sqrt(3 K / 32) S),
      d z   = sqrt(sum (d hid w2)^2) + LAM (eps sqrt(sum (hid w2)^2) + 2^-24 sqrt(48) S2) + 2^-24 |z|
  (the last term: the logit itself is an fp32 number).  That is 1-2e-3 on logits of size 3; a
  dropped lo*hi term is 2^-9 per product, 5e-3 on the same logits.  A logit error of at most E
  moves a probability by a factor within exp(+-2E), so |p - ref| <= (BOUND + expm1(2E)) ref +
  2^-149 with BOUND = 4 x the relative error of the fp32 torch CPU softmax on fp32 logits, as
  in test_cifar_head_tail_gpu.py.  ``pred`` equals the fp64 argmax on every row whose top-2 gap
  exceeds 2E; at most 1 % of the rows may fall below that, and at the binding's shapes the seeds
  leave none.  The literal bound of the head-tail test (BOUND alone) cannot hold against fp64
  fc1: both paths carry fc1's bf16x3 error.  It does hold where the logits are given: the finish
  kernel is held to BOUND alone against the fp64 softmax of ``(part[0] + part[1]) + b2`` formed in
  fp32 from the workspace it read, and its ``pred`` to the first-index argmax of those logits.
* guards: ``probs``, ``pred`` and ``part`` are the middle of sentinel-filled buffers whose margins
  stay untouched, A's rows on either side of the batch are NaN and no NaN comes out.
* rejections return their api.h codes and leave the outputs untouched.
* two launches are bitwise equal.
* ``ops.cifar.head_forward`` and a unit-2-3 ``CifarHipStage`` at B = FC1_X3_MIN_ROWS take the fused
  path with ``set_head_fusion(True)`` and the unfused one with it off (seen from which workspace is
  written); both are within the bound above and their ``pred`` is equal in every row.  The switch
  is on by default.
"""
import functools
import math

import pytest
import torch

import cifar_exact as ce
import cifar_fc1_head_fixtures as hf

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 512, 32), (255, 512, 64), (257, 512, 96), (300, 512, 4096)]
MARGIN = 64
DENORMAL = 2.0**-149
P_SENTINEL = 0x7FC5A5A5   # int32 bits of a NaN with a payload that no arithmetic produces
PRED_SENTINEL = -12345
EPS = 3 * 2.0**-18
LAM = 6.0


def _cops():
    from distributed_neural_networks_amd.ops import cifar as cops
    return cops


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Bufs:
    """probs, pred and part in the middle of sentinel-filled buffers."""

    def __init__(self, M):
        self.M = M
        self.p = torch.full((M + 2 * MARGIN, 10), P_SENTINEL, dtype=torch.int32, device=DEV)
        self.d = torch.full((M + 2 * MARGIN,), PRED_SENTINEL, dtype=torch.int32, device=DEV)
        self.w = torch.full((2 * M + 2 * MARGIN, 16), P_SENTINEL, dtype=torch.int32, device=DEV)
        self.probs = self.p.view(torch.float32)[MARGIN:MARGIN + M]
        self.pred = self.d[MARGIN:MARGIN + M]
        self.part = self.w.view(torch.float32)[MARGIN:MARGIN + 2 * M]

    def untouched(self):
        return all(bool((t == s).all()) for t, s in ((self.p, P_SENTINEL), (self.d, PRED_SENTINEL), (self.w, P_SENTINEL)))

    def margins_ok(self):
        M = self.M
        for what, t, s, n in (("probs", self.p, P_SENTINEL, M), ("pred", self.d, PRED_SENTINEL, M),
                              ("part", self.w, P_SENTINEL, 2 * M)):
            assert bool((t[:MARGIN] == s).all()), f"{what}: rows before the batch were written"
            assert bool((t[MARGIN + n:] == s).all()), f"{what}: rows past the batch were written"
        for what, t in (("probs", self.probs), ("part", self.part)):
            assert bool(torch.isfinite(t).all()), f"{what}: NaN or inf"


def _guarded_a(a, split_in):
    """A (fp32 or, split_in, its blocked encoding) with NaN rows on either side."""
    M, K = a.shape
    buf = torch.full((M + 2 * MARGIN, K), float("nan"), device=DEV)
    buf[MARGIN:MARGIN + M] = _cops().encode_boundary(a) if split_in else a
    return buf[MARGIN:MARGIN + M]


def _fused(a_in, wh, wl, b1, hw, M, K, split_in, bufs, N=512, part="buf", m=None):
    from distributed_neural_networks_amd.ops import _lib
    part_ptr = bufs.part.data_ptr() if part == "buf" else 0
    return _lib.lib().cifar_fc1_head_x3(a_in.data_ptr(), K, wh.data_ptr(), wl.data_ptr(), K, b1.data_ptr(),
                                        hw.w_fc2h.data_ptr(), hw.w_fc2l.data_ptr(), hw.b_fc2.data_ptr(), part_ptr,
                                        bufs.probs.data_ptr(), bufs.pred.data_ptr(), M if m is None else m, N, K,
                                        _stream(), split_in)


def _unfused(a_in, wh, wl, b1, hw, M, K, split_in):
    from distributed_neural_networks_amd.ops import _lib
    hid = torch.empty((M, 512), device=DEV)
    assert _lib.lib().cifar_fc1_x3(a_in.data_ptr(), K, wh.data_ptr(), wl.data_ptr(), K, b1.data_ptr(), hid.data_ptr(),
                                   512, M, 512, K, _stream(), split_in) == 0
    probs, pred = _cops().head_tail(hid, hw)
    return hid, probs, pred


def _bits(t):
    return t.contiguous().view(torch.int32)


def rel_err(p, ref64):
    """Per-element relative error against ref64 beyond the one-denormal-step floor."""
    excess = ((p.double() - ref64).abs() - DENORMAL).clamp_min(0.0)
    return torch.where(excess > 0, excess / ref64, excess)


# ---------------------------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact(name, M, K):
    cops = _cops()
    e = hf.exact_fc2(name, M, K)
    wh, wl = cops.split_bf16(e.fx.w)
    hw = cops.pack_head({"fc2.weight": e.w2, "fc2.bias": e.b2}, DEV, fc1=False)
    return e, e.fx.a.to(DEV), wh.to(DEV), wl.to(DEV), e.fx.b.to(DEV), hw, ce.first_argmax(e.z64)


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("name", ce.FC1_NAMES)
def test_exact_bitwise_unfused(name, M, N, K, split_in):
    e, a, wh, wl, b1, hw, pred_ref = _exact(name, M, K)
    a_in = _guarded_a(a, split_in)
    bufs = Bufs(M)
    assert _fused(a_in, wh, wl, b1, hw, M, K, split_in, bufs) == 0
    hid, probs_u, pred_u = _unfused(a_in, wh, wl, b1, hw, M, K, split_in)
    torch.cuda.synchronize()
    bufs.margins_ok()
    assert torch.equal(hid.cpu(), e.hid)  # the unfused path's hidden rows are the exact ones
    # the two column tiles' partial logits add up to the exact logits less the bias
    z = (bufs.part[:M].double() + bufs.part[M:].double()).cpu()[:, :10] + e.b2.double()
    assert torch.equal(z, e.z64)
    assert not bool(bufs.part[:, 10:].any())
    pred = bufs.pred.cpu().long()
    wrong = (pred != pred_ref).nonzero().flatten()
    assert wrong.numel() == 0, f"pred differs from the exact argmax in {wrong.numel()} rows, first {wrong[:1].tolist()}"
    assert torch.equal(bufs.pred, pred_u)
    assert torch.equal(_bits(bufs.probs), _bits(probs_u))
    assert torch.equal(_bits(bufs.probs[:, 3]), _bits(bufs.probs[:, 7]))
    if M >= 257:  # the tie rule is exercised: the tied pair is the maximum and class 3 is reported
        assert int((pred_ref == 3).sum()) >= 20 and int((pred_ref == 7).sum()) == 0


# ---------------------------------------------------------------------------------------------
# random data
# ---------------------------------------------------------------------------------------------
def _golden(a, w, b1, w2, b2, K):
    """fp64 probabilities and argmax, the per-row logit error bound E, and BOUND (see the docstring)."""
    a64, w64, w2_64 = a.double(), w.double(), w2.double()
    hid64 = torch.relu(a64 @ w64.t() + b1.double())
    z64 = hid64 @ w2_64.t() + b2.double()
    u = 2.0**-24
    d_hid = LAM * (EPS * torch.sqrt(a64.square() @ w64.square().t())
                   + u * math.sqrt(3 * K / 32) * (a64.abs() @ w64.abs().t() + b1.double().abs()))
    d_z = torch.sqrt(d_hid.square() @ w2_64.square().t()) \
        + LAM * (EPS * torch.sqrt(hid64.square() @ w2_64.square().t())
                 + u * math.sqrt(3 * 512 / 32) * (hid64 @ w2_64.abs().t() + b2.double().abs())) \
        + u * z64.abs()
    E = d_z.max(dim=1).values.cpu()
    z = z64.cpu()
    ref = torch.softmax(z, dim=1)
    bound = _softmax_bound(z.float())
    top2 = z.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * E
    return {"ref": ref, "pred": z.argmax(dim=1), "E": E, "bound": bound, "decided": decided}


def _softmax_bound(z32):
    """BOUND of test_cifar_head_tail_gpu.py: 4 x the largest relative error of the fp32 torch CPU softmax
    on the fp32 logits ``z32`` against the fp64 softmax of the same numbers."""
    measured = rel_err(torch.softmax(z32, dim=1), torch.softmax(z32.double(), dim=1)).max().item()
    # The yardstick itself is sane.  torch's fp32 exp reduces its argument in fp32, so its relative error
    # grows with the distance g to the row maximum, about g 2^-24 plus a few ulps (1.1e-6 at g = 16.7 on
    # these logits; the head-tail test's window of 1e-6 fits its grid logits, whose reduction is exact).
    gap = min((z32.max(dim=1, keepdim=True).values - z32).max().item(), 104.0)
    assert 1e-8 < measured < (gap + 4.0) * 2.0**-23, (measured, gap)
    return 4.0 * measured


def _check_finish(what, bufs, b2):
    """The finish kernel on the logits it was given: z = (part[0] + part[1]) + b2 in fp32, as it adds
    them; probabilities within BOUND alone of the fp64 softmax of z, pred its first-index argmax."""
    M = bufs.M
    part = bufs.part.cpu()
    z = (part[:M, :10] + part[M:, :10]) + b2.cpu()
    assert z.dtype == torch.float32
    bound = _softmax_bound(z)
    probs, pred = bufs.probs.cpu(), bufs.pred.cpu().long()
    rel = rel_err(probs, torch.softmax(z.double(), dim=1))
    print(f"{what}: finish kernel max relative error {rel.max().item():.3e}, BOUND {bound:.3e}")
    assert rel.max().item() <= bound, (what, rel.max().item(), bound)
    assert (probs.double().sum(dim=1) - 1.0).abs().max().item() <= 10.0 * bound
    assert torch.equal(pred, ce.first_argmax(z.double())), what


def _check_random(what, probs, pred, gold):
    probs, pred = probs.cpu(), pred.cpu().long()
    assert bool(torch.isfinite(probs).all()), what
    allowed = (gold["bound"] + torch.expm1(2 * gold["E"]))[:, None]
    rel = rel_err(probs, gold["ref"])
    n_undecided = int((~gold["decided"]).sum())
    print(f"{what}: max relative error {rel.max().item():.3e}, allowed per row {allowed.min().item():.3e}.."
          f"{allowed.max().item():.3e} (BOUND {gold['bound']:.3e}, E max {gold['E'].max().item():.3e}); "
          f"{n_undecided} of {pred.numel()} rows below the top-2 gap")
    assert bool((rel <= allowed).all()), (what, rel.max().item())
    assert n_undecided <= pred.numel() // 100, (what, n_undecided)
    d = gold["decided"]
    assert torch.equal(pred[d], gold["pred"][d]), what


@functools.lru_cache(maxsize=None)
def _random(M, K):
    cops = _cops()
    a, w, b1, w2, b2 = _random_cpu(M, K)
    gold = _golden(a, w, b1, w2, b2, K)
    wh, wl = cops.split_bf16(w)
    hw = cops.pack_head({"fc2.weight": w2, "fc2.bias": b2}, DEV, fc1=False)
    return a.to(DEV), wh.to(DEV), wl.to(DEV), b1.to(DEV), hw, gold


def _random_cpu(M, K, seed=1):  # seed 1: no row of any shape falls below the top-2 gap (0 leaves one at three shapes)
    g = torch.Generator().manual_seed(1000 * M + K + seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(512, K, generator=g) / K ** 0.5
    b1 = torch.randn(512, generator=g) * 0.1
    w2 = torch.randn(10, 512, generator=g) * 0.25
    b2 = torch.randn(10, generator=g)
    return a, w, b1, w2, b2


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_random_against_fp64(M, N, K, split_in):
    a, wh, wl, b1, hw, gold = _random(M, K)
    a_in = _guarded_a(a, split_in)
    bufs = Bufs(M)
    assert _fused(a_in, wh, wl, b1, hw, M, K, split_in, bufs) == 0
    _, probs_u, pred_u = _unfused(a_in, wh, wl, b1, hw, M, K, split_in)
    torch.cuda.synchronize()
    bufs.margins_ok()
    assert int((~gold["decided"]).sum()) == 0  # the seed: no row is excluded at these shapes
    _check_random(f"unfused M={M} K={K} split_in={split_in}", probs_u, pred_u, gold)
    _check_random(f"fused M={M} K={K} split_in={split_in}", bufs.probs, bufs.pred, gold)
    _check_finish(f"fused M={M} K={K} split_in={split_in}", bufs, hw.b_fc2)
    # determinism: a second launch into fresh buffers gives the same bits
    again = Bufs(M)
    assert _fused(a_in, wh, wl, b1, hw, M, K, split_in, again) == 0
    torch.cuda.synchronize()
    for x, y in ((bufs.p, again.p), (bufs.d, again.d), (bufs.w, again.w)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,code", [("N", -2), ("K", -1), ("part", -3), ("M", -4)])
def test_rejections(what, code):
    M, K = 257, 96
    a, wh, wl, b1, hw, _ = _random(M, K)
    bufs = Bufs(M)
    kw = {"N": {"N": 256}, "K": {}, "part": {"part": None}, "M": {"m": 0}}[what]
    rc = _fused(a, wh, wl, b1, hw, M, 80 if what == "K" else K, 0, bufs, **kw)
    torch.cuda.synchronize()
    assert rc == code, (what, rc)
    assert bufs.untouched()


# ---------------------------------------------------------------------------------------------
# ops and stage level
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def fusion():
    """Set the switch for the test; the previous setting comes back afterwards."""
    cops = _cops()
    prev = []

    def force(on):
        prev.append(cops.set_head_fusion(on))
        return prev[-1]

    yield force
    if prev:
        cops.set_head_fusion(prev[0])


@functools.lru_cache(maxsize=None)
def _big():
    B = _cops().FC1_X3_MIN_ROWS
    g = torch.Generator(device=DEV).manual_seed(11)
    h = torch.relu(torch.randn(B, 4096, device=DEV, generator=g))  # a stage-0 boundary is non-negative
    dv = {"fc1.weight": torch.randn(512, 4096, device=DEV, generator=g) / 64,
          "fc1.bias": torch.randn(512, device=DEV, generator=g) * 0.1,
          "fc2.weight": torch.randn(10, 512, device=DEV, generator=g) * 0.25,
          "fc2.bias": torch.randn(10, device=DEV, generator=g)}
    gold = _golden(h, dv["fc1.weight"], dv["fc1.bias"], dv["fc2.weight"], dv["fc2.bias"], 4096)  # fp64 on the device
    return {k: v.cpu() for k, v in dv.items()}, h, gold


def test_head_forward_switch(fusion):
    cops = _cops()
    sd, h, gold = _big()
    B = h.shape[0]
    assert fusion(True) is True  # what the switch was before this test touched it: on by default
    assert fusion(False) is True and fusion(True) is False  # each call returns the previous setting
    w = cops.pack_head(sd, DEV)
    out = {}
    for on in (True, False):
        fusion(on)
        part = torch.full((2, B, 16), float("nan"), device=DEV)
        hid = torch.full((B, 512), float("nan"), device=DEV)
        probs, pred = cops.head_forward(h, w, hid=hid, part=part)
        torch.cuda.synchronize()
        # the path taken shows in the workspace it wrote
        assert bool(torch.isfinite(part).all()) == on and bool(torch.isfinite(hid).all()) == (not on)
        _check_random(f"head_forward fusion={on}", probs, pred, gold)
        out[on] = pred
    assert torch.equal(out[True], out[False])  # every row, the near-ties included


def test_stage_switch(fusion):
    from distributed_neural_networks_amd.runtime.stages import CifarHipStage
    sd, h, gold = _big()
    out = {}
    for on in (True, False):
        fusion(on)
        st = CifarHipStage(sd, 2, 3, torch.device(DEV))
        y = st.forward(h)
        torch.cuda.synchronize()
        buf = st._scratch[h.shape[0]]
        assert ("part" in buf) == on and ("hid" in buf) == (not on)
        _check_random(f"stage fusion={on}", y.probs, y.pred, gold)
        out[on] = y.pred
    assert torch.equal(out[True], out[False])  # every row, the near-ties included
