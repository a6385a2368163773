"""`ops.cifar.head_tail` (fc2 + softmax + argmax) on its own, both precisions.

The fixtures of tests/cifar_exact.py (`head_fixture`; preconditions asserted on
the CPU in tests/test_cifar_exact.py) put the hidden rows and fc2 on grids such
that the logits are exact in fp32 in any summation order: `hid_wide` (wide hid,
bf16-exact weights: the `hid_lo * w_hi` term) and `w_wide` (bf16-exact hid,
wide weights: `hid_hi * w_lo`) for `cifar_head_tail_x3_kernel`, and `bf16`
(both bf16-exact) for `cifar_head_tail_kernel`, which accumulates its one bf16
product per k in fp32 as well (`f32x4 acc`, mfma_f32_16x16x32_bf16).  The
logits have a standard deviation of about 30 and every 8th row has a gap to
its maximum above 104, so the max subtraction matters and the smallest
probabilities underflow to exactly 0.

Ties: fc2 rows 3 and 7 are identical, bias included, and so are rows 0 and 9.
`pred` must be the first index of the fp64 argmax in every row, none excluded
(class 0 or 3 wins about a third of the rows, 7 and 9 never may), and
`probs[:, 3] == probs[:, 7]`, `probs[:, 0] == probs[:, 9]` bitwise.

Probabilities: against `torch.softmax` of the exact logits in fp64, relative
per element, |p - ref| <= BOUND * ref + 2^-149 (one fp32 denormal step, for
the underflowed entries).  BOUND is 4 times the largest relative error,
measured with the same floor, of the fp32 torch CPU softmax on the same
logits; the test computes it so, and on the 300 rows it measured
2.449e-07 (hid_wide), 2.688e-07 (w_wide) and 2.482e-07 (bf16), so BOUND is
9.79e-07, 1.08e-06 and 9.93e-07.  Each row's sum is within 10 * BOUND of 1.
On the MI355X the kernels' largest errors were 2.33e-07, 1.93e-07 and
2.05e-07, the sums within 1.85e-07 of 1.  The bf16 kernel first missed the
bound: with `__expf` it returned 0 for every probability below 2^-126 (7.5e-39
expected) and was 1.02e-06 off on normal ones, and `expf` under its file's
-ffast-math still was 3.5e-06 off (4.19e-32 expected); it now sits in
cifar_x3.hip, built with IEEE exp and division like the fp32 kernel.

Batch edges: B in {1, 15, 16, 17, 300} (a wave takes 16 rows; 300 = 18 full
tiles and one of 12 rows, five workgroups).  `probs` and `pred` are the middle
of sentinel-filled buffers whose margins must stay untouched, and the `hid`
rows on either side of the batch are NaN, so a row read past `B` (the
`row < B ? row : B - 1` clamp) or written past it shows.
"""
import functools

import pytest
import torch

import cifar_exact as ce

pytestmark = pytest.mark.gpu

DEV = "cuda"
BATCHES = [1, 15, 16, 17, 300]
MARGIN = 64
DENORMAL = 2.0**-149
P_SENTINEL = 0x7FC5A5A5   # int32 bits of a NaN with a payload that no arithmetic produces
PRED_SENTINEL = -12345


def rel_err(p, ref64):
    """Per-element relative error against ref64 beyond the one-denormal-step floor (0 where ref64 == 0
    and the floor covers the difference)."""
    excess = ((p.double() - ref64).abs() - DENORMAL).clamp_min(0.0)
    return torch.where(excess > 0, excess / ref64, excess)


@functools.lru_cache(maxsize=None)
def _golden(name):
    """Per fixture, once (CPU): exact logits, fp64 probabilities, first-index argmax, BOUND, and the
    packed head weights and hidden rows on the device."""
    from distributed_neural_networks_amd.ops import cifar as cops
    fx = ce.head_fixture(name)
    z = ce.head_logits64(fx)
    assert torch.equal(z.float().double(), z)
    ref = torch.softmax(z, dim=1)
    measured = rel_err(torch.softmax(z.float(), dim=1), ref).max().item()
    bound = 4.0 * measured
    print(f"{name}: fp32 torch CPU softmax max relative error {measured:.3e}, BOUND {bound:.3e}")
    assert 1e-8 < measured < 1e-6  # the yardstick itself is sane
    wh = cops.pack_head(fx.sd, DEV, fc1=False, precision=fx.precision)
    hid = fx.hid.to(device=DEV, dtype=cops.act_dtype(fx.precision))
    assert torch.equal(hid.float().cpu(), fx.hid)
    return fx, wh, hid, ref, ce.first_argmax(z), bound


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", ce.HEAD_NAMES)
def test_head_tail(name, B):
    from distributed_neural_networks_amd.ops import cifar as cops
    fx, wh, hid, ref, pred_ref, bound = _golden(name)
    ref, pred_ref = ref[:B], pred_ref[:B]

    hbuf = torch.full((B + 2 * MARGIN, 512), float("nan"), dtype=hid.dtype, device=DEV)
    hbuf[MARGIN:MARGIN + B] = hid[:B]
    pbuf = torch.full((B + 2 * MARGIN, 10), P_SENTINEL, dtype=torch.int32, device=DEV)
    dbuf = torch.full((B + 2 * MARGIN,), PRED_SENTINEL, dtype=torch.int32, device=DEV)
    cops.head_tail(hbuf[MARGIN:MARGIN + B], wh, pbuf.view(torch.float32)[MARGIN:MARGIN + B], dbuf[MARGIN:MARGIN + B])
    torch.cuda.synchronize()
    pbits, dall = pbuf.cpu(), dbuf.cpu()

    for what, t, s in (("probs", pbits, P_SENTINEL), ("pred", dall, PRED_SENTINEL)):
        assert bool((t[:MARGIN] == s).all()), f"{what}: rows before the batch were written"
        assert bool((t[MARGIN + B:] == s).all()), f"{what}: rows past the batch were written"
    probs = pbits[MARGIN:MARGIN + B].view(torch.float32)
    pred = dall[MARGIN:MARGIN + B].long()

    # argmax: the first index attaining the maximum of the exact logits, in every row
    wrong = (pred != pred_ref).nonzero().flatten()
    assert wrong.numel() == 0, (f"pred differs in {wrong.numel()} rows; first row {wrong[0].item()}: got "
                                f"{pred[wrong[0]].item()}, expected {pred_ref[wrong[0]].item()}")
    if B == ce.HEAD_B_MAX:  # the tie rule is exercised: a tied class is the maximum in many rows
        assert int((pred_ref == 0).sum()) >= 20 and int((pred_ref == 3).sum()) >= 20

    # exact ties give bitwise equal probabilities
    assert torch.equal(probs[:, 3].view(torch.int32), probs[:, 7].view(torch.int32))
    assert torch.equal(probs[:, 0].view(torch.int32), probs[:, 9].view(torch.int32))

    # probabilities: finite, relative bound per element with the denormal floor, rows sum to 1
    assert bool(torch.isfinite(probs).all())
    rel = rel_err(probs, ref)
    i = int(rel.argmax())
    sum_err = (probs.double().sum(dim=1) - 1.0).abs().max().item()
    n_zero = int((probs == 0).sum())
    print(f"{name} B {B}: max relative error {rel.max().item():.3e} at row {i // 10} class {i % 10} "
          f"(got {probs.flatten()[i].item():.9e}, expected {ref.flatten()[i].item():.9e}); BOUND {bound:.3e}; "
          f"max|sum - 1| {sum_err:.3e}; {n_zero} probabilities are exactly 0")
    assert n_zero >= 1  # every batch has a row whose smallest probabilities underflow
    assert rel.max().item() <= bound, (rel.max().item(), bound)
    assert sum_err <= 10.0 * bound, (sum_err, bound)
