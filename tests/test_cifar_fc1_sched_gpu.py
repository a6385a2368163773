"""Fused fp32 fc1 (``cifar_fc1_x3``) under both k-loop schedules: the lockstep
one (all eight waves read, multiply and restage together) and the staggered
one (waves 4-7 half a k-step behind waves 0-3).  Every shape runs with A as
fp32 and in the blocked hi/lo encoding, is checked against fp64 torch with the
bound of ``test_cifar_fc1_x3_kernel``, and the staggered output must be bitwise
the lockstep one.  C carries 64 sentinel rows past M that must come back
untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.0
# M x N x K: one row and nk = 1 (prologue and drain only); nk = 2; a second M
# tile of one row, two column tiles and odd nk (both buffer parities, the
# wrap); the real K
SHAPES = [(1, 256, 32), (255, 256, 64), (257, 512, 96), (300, 512, 4096)]


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


def _run(c, M, N, K, split_in, out=None):
    from distributed_neural_networks_amd.ops import _lib
    if out is None:
        out = torch.full((M + 64, N), SENTINEL, device=DEV)
    rc = _lib.lib().cifar_fc1_x3(c["a"][split_in].data_ptr(), K, c["wh"].data_ptr(), c["wl"].data_ptr(), K,
                                 c["b"].data_ptr(), out.data_ptr(), N, M, N, K,
                                 torch.cuda.current_stream().cuda_stream, split_in)
    assert rc == 0
    return out


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fc1_sched_arms(M, N, K, split_in, sched):
    from distributed_neural_networks_amd.ops.cifar import FC1_SCHED
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
    assert torch.equal(outs["staggered"].view(torch.int32), outs["lockstep"].view(torch.int32))


@pytest.mark.parametrize("split_in", [0, 1])
@pytest.mark.parametrize("name", ["lockstep", "staggered"])
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
