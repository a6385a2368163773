"""Fused fp32 fc1 (``cifar_fc1_x3``), every compiled k-loop arm (``FC1_SCHED``;
all run the staggered schedule: waves 4-7 half a k-step behind waves 0-3).
Every shape runs with A as fp32 and in the blocked hi/lo encoding.

* random data against fp64 torch with the bound of ``test_cifar_fc1_x3_kernel``;
  C carries 64 sentinel rows past M that must come back untouched;
* the exact fixtures of tests/cifar_exact.py (preconditions asserted on the CPU
  in tests/test_cifar_exact.py): every product and partial sum is exact in
  fp32, so the fp64 result cast to fp32 is the expected output of every arm bit
  for bit, on every shape, contiguous and with NaN in padded pitches.  This is
  the reference that the arms are held to, in place of a comparison with the
  lockstep loop that the kernel no longer has;
* race screen of the staggered arm (the lean arm's is in
  test_cifar_fc1_lean_gpu.py): 20 launches, every output bitwise the first."""
import pytest
import torch

import cifar_exact as ce

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.0
# M x N x K: one row and nk = 1 (prologue and drain only); nk = 2; a second M
# tile of one row, two column tiles and odd nk (both buffer parities, the
# wrap); the real K
SHAPES = [(1, 256, 32), (255, 256, 64), (257, 512, 96), (300, 512, 4096)]
PAD = 32  # pad columns of the padded launches (lda % 4 == 0, ldw % 8 == 0)


@pytest.fixture
def sched():
    """Force a schedule arm for the test; the default comes back afterwards."""
    from distributed_neural_networks_amd.ops import cifar as cops
    prev = []

    def force(name):
        prev.append(cops.set_fc1_sched(name))

    yield force
    if prev:
        cops.set_fc1_sched(prev[0])


_CASES = {}


def _case(M, N, K):
    """Inputs and the fp64 reference of one shape, made once and left unchanged."""
    if (M, N, K) not in _CASES:
        from distributed_neural_networks_amd.ops.cifar import encode_boundary, split_bf16
        g = torch.Generator(device=DEV).manual_seed(1000 * M + K)
        a = torch.randn(M, K, device=DEV, generator=g)
        w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
        b = torch.randn(N, device=DEV, generator=g) * 0.1
        wh, wl = split_bf16(w)
        ref = torch.relu(a.double() @ w.double().t() + b.double())
        _CASES[(M, N, K)] = {"a": (a, encode_boundary(a)), "wh": wh, "wl": wl, "b": b, "ref": ref,
                             "bound": 2e-5 * ref.abs().max().item()}
    return _CASES[(M, N, K)]


def _launch(a, lda, wh, wl, ldw, b, M, N, K, split_in, out=None):
    from distributed_neural_networks_amd.ops import _lib
    if out is None:
        out = torch.full((M + 64, N), SENTINEL, device=DEV)
    rc = _lib.lib().cifar_fc1_x3(a.data_ptr(), lda, wh.data_ptr(), wl.data_ptr(), ldw, b.data_ptr(), out.data_ptr(),
                                 N, M, N, K, torch.cuda.current_stream().cuda_stream, split_in)
    assert rc == 0
    return out


def _run(c, M, N, K, split_in, out=None):
    return _launch(c["a"][split_in], K, c["wh"], c["wl"], K, c["b"], M, N, K, split_in, out)


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fc1_sched_arms(M, N, K, split_in, sched):
    from distributed_neural_networks_amd.ops.cifar import FC1_SCHED
    assert sorted(FC1_SCHED) == ["lean", "staggered"]  # every compiled arm is covered here
    c = _case(M, N, K)
    outs = {}
    for name in FC1_SCHED:
        sched(name)
        outs[name] = _run(c, M, N, K, split_in)
    torch.cuda.synchronize()
    for name, out in outs.items():
        err = (out[:M].double() - c["ref"]).abs().max().item()
        print(f"{name} M={M} N={N} K={K} split_in={split_in}: max|err| {err:.3e} (bound {c['bound']:.3e})")
        assert err <= c["bound"], (name, err)
        assert bool((out[M:] == SENTINEL).all()), f"{name}: rows past M were written"


_EXACT = {}


def _exact(name):
    """One exact fixture on the device, once: A, W split, b, and per shape of SHAPES the expected
    bits with 64 sentinel rows below."""
    if name not in _EXACT:
        from distributed_neural_networks_amd.ops.cifar import split_bf16
        fx = ce.fc1_fixture(name)
        want = {}
        for M, N, K in SHAPES:
            ref64 = ce.fc1_reference64(ce.fc1_fixture(name, M, N, K))
            ref = ref64.float()
            assert torch.equal(ref.double(), ref64)
            full = torch.full((M + 64, N), SENTINEL)
            full[:M] = ref
            want[(M, N, K)] = full.to(DEV).view(torch.int32)
        wh, wl = split_bf16(fx.w.to(DEV))
        assert torch.equal(wh.float() + wl.float(), fx.w.to(DEV))
        _EXACT[name] = {"a": fx.a.to(DEV), "wh": wh, "wl": wl, "b": fx.b.to(DEV), "want": want}
    return _EXACT[name]


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("name", ce.FC1_NAMES)
def test_fc1_arms_are_bitwise_the_fp64_reference(name, M, N, K, split_in, sched):
    """K-prefixes of an exact fixture, contiguous and with NaN pad columns in the pitch (A's for fp32
    A; W's for blocked A, whose rows are 32-k blocks without room for a pad): on every arm, rows [:M]
    are the fp64 result bit for bit and the 64 rows past M keep the sentinel."""
    from distributed_neural_networks_amd.ops.cifar import FC1_SCHED, encode_boundary
    e = _exact(name)
    a32 = e["a"][:M, :K].contiguous()
    wh, wl, b = e["wh"][:N, :K].contiguous(), e["wl"][:N, :K].contiguous(), e["b"][:N].contiguous()
    want = e["want"][(M, N, K)]
    nan = float("nan")
    if split_in == 0:
        a, ap, lda_p = a32, torch.full((M, K + PAD), nan, device=DEV), K + PAD
        ap[:, :K] = a32
        whp, wlp, ldw_p = wh, wl, K
    else:
        a = ap = encode_boundary(a32)  # the blocked encoding is per 32-k block: encode the prefix itself
        lda_p, ldw_p = K, K + PAD
        whp = torch.full((N, K + PAD), nan, device=DEV, dtype=torch.bfloat16)
        wlp = torch.full((N, K + PAD), nan, device=DEV, dtype=torch.bfloat16)
        whp[:, :K] = wh
        wlp[:, :K] = wl
    outs = {}
    for arm in FC1_SCHED:
        sched(arm)
        outs[arm, "contiguous"] = _launch(a, K, wh, wl, K, b, M, N, K, split_in)
        outs[arm, "padded"] = _launch(ap, lda_p, whp, wlp, ldw_p, b, M, N, K, split_in)
    torch.cuda.synchronize()
    for (arm, what), got in outs.items():
        g = got.view(torch.int32)
        if not torch.equal(g, want):
            bad = (g != want).nonzero()
            r, col = bad[0].tolist()
            pytest.fail(f"{arm} {name} M={M} N={N} K={K} split_in={split_in} {what}: {bad.shape[0]} elements differ; "
                        f"first at row {r} column {col}: got {got[r, col].item()!r}, expected "
                        f"{want.view(torch.float32)[r, col].item()!r}")


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("name", ["staggered"])
def test_fc1_sched_race_screen(name, split_in, sched):
    """20 launches on the same input: every output bitwise the first."""
    M, N, K = 300, 512, 4096
    c = _case(M, N, K)
    sched(name)
    first = _run(c, M, N, K, split_in)
    out = torch.empty_like(first)
    for i in range(1, 20):
        out.fill_(SENTINEL)
        _run(c, M, N, K, split_in, out)
        assert torch.equal(out.view(torch.int32), first.view(torch.int32)), f"launch {i} differs"
    err = (first[:M].double() - c["ref"]).abs().max().item()
    assert err <= c["bound"], err
