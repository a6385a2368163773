"""The lean arm of the fused fp32 fc1 (``cifar_fc1_x3``, ``FC1_SCHED["lean"]``):
the staggered schedule with the packed bf16 split (one v_cvt_pk_bf16_f32 per
pair) and buffer-descriptor addressing (one loop-invariant lane offset per
stream, rows past M dropped by the descriptor's range check).

* lean is bitwise staggered on the shapes of the schedule test, A as fp32 and
  in the blocked hi/lo encoding; 64 sentinel rows past M come back untouched;
* padded pitches with NaN in the pad columns (lda > K for fp32 A, ldw > K for
  blocked A): every arm agrees bitwise and stays within the bound of
  ``test_cifar_fc1_x3_kernel`` against fp64 torch;
* an adversarial A (bf16 rounding ties on even and odd upper halves, their
  neighbours, +-0, zero low halves, magnitudes 2^-100..2^100): lean is bitwise
  staggered, i.e. the packed split equals the scalar split; through a W that
  selects one element per output, each arm's split is bitwise torch's
  ``split_bf16`` hi + lo; and the blocked encoding of the same values decodes
  to the same;
* race screen: 20 launches of lean on one input, every output bitwise the first."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.0
# full tile + edge tiles of 1 and 44 rows, nk = 1, 2, 3 and 128, both column tiles
SHAPES = [(1, 256, 32), (255, 256, 64), (257, 512, 96), (300, 512, 4096)]
PAD = 32  # pad columns of the pitch tests (lda % 4 == 0, ldw % 8 == 0)


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


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fc1_lean_bitwise_staggered(M, N, K, split_in, sched):
    c = _case(M, N, K)
    outs = {}
    for name in ("staggered", "lean"):
        sched(name)
        outs[name] = _run(c, M, N, K, split_in)
    torch.cuda.synchronize()
    for name, out in outs.items():
        assert bool((out[M:] == SENTINEL).all()), f"{name}: rows past M were written"
    err = (outs["lean"][:M].double() - c["ref"]).abs().max().item()
    print(f"lean M={M} N={N} K={K} split_in={split_in}: max|err| {err:.3e} (bound {c['bound']:.3e})")
    assert torch.equal(_bits(outs["lean"]), _bits(outs["staggered"]))
    assert err <= c["bound"], err


@pytest.mark.parametrize("split_in", [0, 1])
def test_fc1_lean_padded_pitch(split_in, sched):
    """A wrong pitch or k offset reaches a NaN pad column."""
    from distributed_neural_networks_amd.ops.cifar import FC1_SCHED
    M, N, K = 257, 512, 96
    c = _case(M, N, K)
    nan = float("nan")
    if split_in == 0:
        a = torch.full((M, K + PAD), nan, device=DEV)
        a[:, :K] = c["a"][0]
        lda, wh, wl, ldw = K + PAD, c["wh"], c["wl"], K
    else:
        a, lda, ldw = c["a"][1], K, K + PAD
        wh = torch.full((N, K + PAD), nan, device=DEV, dtype=torch.bfloat16)
        wl = torch.full((N, K + PAD), nan, device=DEV, dtype=torch.bfloat16)
        wh[:, :K] = c["wh"]
        wl[:, :K] = c["wl"]
    outs = {}
    for name in FC1_SCHED:
        sched(name)
        outs[name] = _launch(a, lda, wh, wl, ldw, c["b"], M, N, K, split_in)
    torch.cuda.synchronize()
    for name, out in outs.items():
        err = (out[:M].double() - c["ref"]).abs().max().item()
        print(f"{name} padded split_in={split_in}: max|err| {err:.3e} (bound {c['bound']:.3e})")
        assert err <= c["bound"], (name, err)  # a NaN fails this comparison too
        assert bool((out[M:] == SENTINEL).all()), f"{name}: rows past M were written"
        assert torch.equal(_bits(out), _bits(outs["staggered"])), name
    # the contiguous case of the same shape gives the same bits
    sched("lean")
    assert torch.equal(_bits(_run(c, M, N, K, split_in)), _bits(outs["lean"]))


def _adversarial(M, K):
    """fp32 values that exercise the bf16 conversion; all finite, exponents 2^-100..2^100."""
    rng = np.random.default_rng(7)
    n = M * K
    sign = rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
    exp = rng.integers(127 - 100, 127 + 101, n, dtype=np.uint32) << np.uint32(23)
    bits = sign | exp | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    top = bits & np.uint32(0xffff0000)
    kind = rng.integers(0, 8, n)
    bits = np.where(kind == 1, top | np.uint32(0x8000), bits)  # exact tie, upper half even or odd
    bits = np.where(kind == 2, top | np.uint32(0x7fff), bits)  # just below the tie
    bits = np.where(kind == 3, top | np.uint32(0x8001), bits)  # just above the tie
    bits = np.where(kind == 4, top, bits)                      # zero low half: lo == 0
    bits = np.where(kind == 5, sign, bits)                     # +0 and -0
    bits = bits.astype(np.uint32)
    ties = bits[kind == 1]
    assert ((ties >> 16) & 1).min() == 0 and ((ties >> 16) & 1).max() == 1  # even and odd upper halves
    return torch.from_numpy(bits.view(np.float32).reshape(M, K).copy()).to(DEV)


_ADV = {}


def _adv():
    if not _ADV:
        _ADV["a"] = _adversarial(300, 4096)
    return _ADV["a"]


def test_fc1_lean_adversarial_split(sched):
    M, N, K = 300, 512, 4096
    c = _case(M, N, K)
    a = _adv()
    assert bool(torch.isfinite(a).all())
    outs = {}
    for name in ("staggered", "lean"):
        sched(name)
        outs[name] = _launch(a, K, c["wh"], c["wl"], K, c["b"], M, N, K, 0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs["lean"][:M]).all())
    assert bool((outs["lean"][M:] == SENTINEL).all())
    assert torch.equal(_bits(outs["lean"]), _bits(outs["staggered"]))


@pytest.mark.parametrize("split_in", [0, 1])
def test_fc1_split_matches_torch_split(split_in, sched):
    """The split of A inside the kernel (fp32 A; the packed one on lean, the scalar one on
    staggered) or in ``encode_boundary`` (blocked A) against torch's ``split_bf16``, with no other arm
    as the reference: W is bf16-exact with one nonzero per row, +1 at column n for n < 256 and -1 at
    column n - 256 for n >= 256, and the bias is zero, so output (m, n) is relu(+-fl(hi + lo)) of one
    element of A and every element is covered once with each sign.  0.0 is added to both sides first:
    the sign of a zero is not asserted (the accumulator starts at +0 and takes 255 zero products)."""
    from distributed_neural_networks_amd.ops.cifar import FC1_SCHED, encode_boundary, split_bf16
    M, N, K = 300, 512, 256
    a = _adv()[:, :K].contiguous()
    assert bool(torch.isfinite(a).all())
    w = torch.zeros(N, K, device=DEV)
    w[torch.arange(256), torch.arange(256)] = 1.0
    w[torch.arange(256, 512), torch.arange(256)] = -1.0
    wh, wl = split_bf16(w)
    assert torch.equal(wh.float(), w) and not bool(wl.float().any())
    hi, lo = split_bf16(a)
    s = hi.float() + lo.float()
    want = torch.relu(torch.cat([s, -s], dim=1)) + 0.0
    a_in = encode_boundary(a) if split_in else a
    for name in FC1_SCHED:
        sched(name)
        out = _launch(a_in, K, wh, wl, K, torch.zeros(N, device=DEV), M, N, K, split_in)
        torch.cuda.synchronize()
        assert bool((out[M:] == SENTINEL).all()), name
        assert torch.equal(_bits(out[:M] + 0.0), _bits(want)), name


def test_boundary_encoding_matches_torch_split():
    from distributed_neural_networks_amd.ops.cifar import decode_boundary, encode_boundary, split_bf16
    a = _adv()
    hi, lo = split_bf16(a)
    dec = decode_boundary(encode_boundary(a))
    torch.cuda.synchronize()
    assert torch.equal(_bits(dec), _bits(hi.float() + lo.float()))


@pytest.mark.parametrize("split_in", [0, 1])
def test_fc1_lean_race_screen(split_in, sched):
    """20 launches on the same input: every output bitwise the first."""
    M, N, K = 300, 512, 4096
    c = _case(M, N, K)
    sched("lean")
    first = _run(c, M, N, K, split_in)
    out = torch.empty_like(first)
    for i in range(1, 20):
        out.fill_(SENTINEL)
        _run(c, M, N, K, split_in, out)
        assert torch.equal(_bits(out), _bits(first)), f"launch {i} differs"
    err = (first[:M].double() - c["ref"]).abs().max().item()
    assert err <= c["bound"], err
