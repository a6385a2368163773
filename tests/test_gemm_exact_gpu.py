"""Decode GEMM routes held to the exact-arithmetic fixtures of tests/gemm_exact.py:
the skinny dispatch table and its pins, W8A16, the stream kernel, the one-shot
kernel and the fused vocabulary head.  Every product and partial sum of these
fixtures is exact in fp32, so the fp64 result (rounded once for bf16 outputs of
``dense``, unrounded for ``thin``) is the expected output in every tiling,
summation order, split-K and workgroup reduction: the comparison is
``torch.equal``, and a difference names the element.  Every output lands in a
NaN-filled buffer taller and wider than (M, N) whose margin must stay NaN.

Epilogues: none, bias + residual, and ReLU where the route has it.  The folded
norms round by design: tests/test_norm_exact_gpu.py holds them to the fp64 result
element by element outside a narrow band around the bf16 rounding boundaries.
GELU and SwiGLU go through erf / exp and stay with the tolerance tests.

Branch names in the tables below are those of ``launch_skinny``
(csrc/kernels/gemm_skinny.hip): ``CFG(MT, NT, U, PIPE, KS)`` and the M-split
``CFG_MS(NT, U, PIPE, KS)``.
"""
import pytest
import torch

import gemm_exact as ge

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

EPIS = (("none", None, False, False), ("bias_res", None, True, True), ("relu", "relu", True, True))


def _m_cap(M):
    return 64 if M <= 64 else 256


_SHUF = {}


def _shuf(case, key):
    """The fragment-order copy of ``case.w`` (made once per weight)."""
    from distributed_neural_networks_amd.ops.gemm import shuffle_weight
    if key not in _SHUF:
        _SHUF[key] = shuffle_weight(case.w)
    return _SHUF[key]


_W8 = {}


def _fp8_weight(case, key):
    """``Fp8Weight(q, scale, k)`` built directly from the fixture's bytes and power-of-two scales
    (K zero-padded to a multiple of 128), with its fragment-order copy.  Made once per weight."""
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight, kpad_of
    from distributed_neural_networks_amd.ops.gemm import shuffle_weight
    if key not in _W8:
        N, K = case.w.shape
        q = torch.zeros((N, kpad_of(K)), dtype=torch.uint8, device=case.w.device)
        q[:, :K] = case.w.view(torch.uint8)
        q = q.view(torch.float8_e4m3fn)
        _W8[key] = (Fp8Weight(q, case.sw.contiguous(), K), shuffle_weight(q[:, :K]))
    return _W8[key]


def _w8(case, key, shuf):
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight
    w, sh = _fp8_weight(case, key)
    return Fp8Weight(w.q, w.scale, w.k, sh if shuf else None)


@pytest.fixture
def table_only():
    """Stream and one-shot kernels off: every call takes the skinny table."""
    from distributed_neural_networks_amd.ops.gemm import set_oneshot_gemm, set_stream_gemm
    set_stream_gemm(0)
    set_oneshot_gemm(0)
    try:
        yield
    finally:
        set_stream_gemm(1, 8 << 20, 0)
        set_oneshot_gemm(1)


# ----------------------------------------------------------------------------- 1. the skinny table
# (M, N, K, weights, branch of launch_skinny reached with bf16 operands)
SKINNY = [
    (1, 100, 64, "rm", "M<=8: CFG(1,1,4,false,8), 1 wave (K = 64 is one chunk)"),
    (1, 4112, 768, "shuf", "M<=8, Wsh, 4096<N<16384: CFG(1,1,4,false,4)"),
    (1, 100, 128, "shuf", "M<=8: CFG(1,1,4,false,8), 4 waves (K = 128 is four chunks)"),
    (8, 2306, 192, "rm", "M<=8: CFG(1,1,4,false,8); ldc % 4 != 0, scalar epilogue"),
    (8, 16400, 64, "shuf", "M<=8, N >= 16384 (bf16): CFG(1,1,4,false,8)"),
    (9, 1040, 768, "rm", "M<=16: CFG(1,2,2,true,4)"),
    (9, 16400, 128, "shuf", "M<=16, wide: CFG(1,4,2,false,2)"),
    (16, 16400, 64, "rm", "M<=16, wide: CFG(1,4,2,false,2)"),
    (16, 2308, 192, "shuf", "M<=16: CFG(1,2,2,true,4); vector epilogue, ragged last tile"),
    (17, 16400, 192, "shuf", "Wsh, wide, M<=32: CFG(2,4,2,false,2)"),
    (17, 100, 192, "shuf", "Wsh, N<=1024: CFG_MS(1,4,false,4)"),
    (17, 4112, 768, "shuf", "Wsh, N>4096, M<=32: CFG(2,2,2,true,4)"),
    (17, 2064, 8192, "shuf", "Wsh, kbytes>=8192: CFG_MS(2,4,false,4)"),
    (17, 2306, 768, "shuf", "Wsh: CFG_MS(2,2,false,4)"),
    (17, 100, 64, "rm", "row-major, N<=1024: CFG_MS(1,2,true,4), 1 wave"),
    (17, 2064, 128, "rm", "row-major, N<=2048: CFG_MS(2,2,true,4), 4 waves"),
    (17, 16400, 64, "rm", "M<=32, wide: CFG(2,4,2,false,2)"),
    (17, 2306, 8192, "rm", "M<=32, deep: CFG(2,1,8,false,2)"),
    (17, 2308, 192, "rm", "M<=32, narrow: CFG(2,1,2,false,4)"),
    (17, 4112, 192, "rm", "M<=32: CFG(2,2,2,true,4)"),
    (32, 16400, 64, "shuf", "Wsh, wide, M<=32: CFG(2,4,2,false,2)"),
    (32, 4112, 192, "shuf", "Wsh, N>4096, M<=32: CFG(2,2,2,true,4)"),
    (32, 1040, 768, "rm", "row-major, N<=2048: CFG_MS(2,2,true,4)"),
    (33, 16400, 128, "shuf", "Wsh, wide, M>32: CFG(4,4,2,false,2)"),
    (33, 4112, 8192, "shuf", "Wsh, kbytes>=8192: CFG_MS(2,4,false,4)"),
    (33, 4112, 768, "shuf", "Wsh: CFG_MS(2,2,false,4)"),
    (33, 16400, 64, "rm", "M>32, wide: CFG(4,4,2,false,2)"),
    (33, 2306, 8192, "rm", "M>32, deep: CFG(4,1,8,false,2)"),
    (33, 2308, 768, "rm", "M>32, narrow: CFG(4,1,2,false,4)"),
    (33, 4112, 192, "rm", "M>32: CFG(4,2,2,false,4)"),
    (33, 100, 192, "rm", "row-major, N<=1024: CFG_MS(1,2,true,4)"),
    (64, 1040, 768, "shuf", "Wsh: CFG_MS(2,2,false,4)"),
    (64, 16400, 64, "shuf", "Wsh, wide, M>32: CFG(4,4,2,false,2)"),
    (64, 4112, 128, "rm", "M>32: CFG(4,2,2,false,4)"),
    (64, 2306, 192, "rm", "M>32, narrow: CFG(4,1,2,false,4); scalar epilogue"),
    (65, 100, 192, "rm", "M>64, N<=1024: CFG_MS(1,4,false,4)"),
    (65, 1040, 768, "shuf", "M>64: CFG_MS(2,2,false,4)"),
    (100, 2306, 192, "rm", "M>64: CFG_MS(2,2,false,4)"),
    (100, 100, 64, "shuf", "M>64, N<=1024: CFG_MS(1,4,false,4)"),
    (256, 1040, 128, "rm", "M>64: CFG_MS(2,2,false,4)"),
    (256, 2308, 768, "shuf", "M>64: CFG_MS(2,2,false,4)"),
]


@pytest.mark.parametrize("M,N,K,layout,branch", SKINNY, ids=[f"{m}x{n}x{k}-{l}" for m, n, k, l, _ in SKINNY])
def test_skinny_table(table_only, M, N, K, layout, branch):
    """``linear`` on the skinny table, row-major and fragment-order weights: fp32 output on
    ``dense``, bf16 output on ``dense`` and ``thin``; no epilogue, bias + residual, bias + ReLU +
    residual.  The branch each case reaches is the last column of ``SKINNY`` above (read off
    ``launch_skinny`` for bf16 operands: kbytes = 2 K, so K = 8192 is the deep class and K = 64 /
    128 shrink the wave count in ``launch_skinny_cfg``).  Lines of the table these cases do not
    reach, and where they are reached instead:

      W8 && Wsh && N >= 65536: CFG(1,2,4,false,8)   test_w8a16_vocabulary_wide, N = 65552
      W8 && Wsh && N >= 16384: CFG(1,2,2,false,2)   test_w8a16, N = 16400
      W8 && N > 4096: CFG_MS(4,2,false,4)           test_w8a16
      the six pinned lines                          test_skinny_pins
    """
    from distributed_neural_networks_amd.ops.gemm import linear
    for kind, dtype in (("dense", F32), ("dense", BF16), ("thin", BF16)):
        c = ge.device_case(kind, M, N, K, device=DEV, m_cap=_m_cap(M))
        wsh = _shuf(c, (kind, N, K)) if layout == "shuf" else None
        for name, act, bias, res in EPIS:
            buf = ge.nan_buffer(M, N, dtype, DEV)
            linear(c.a, c.w, c.bias if bias else None, act, c.res if res else None, out=buf[:M, :N], w_shuf=wsh)
            ge.assert_exact(buf, M, N, ge.want(c, dtype, act, bias, res), f"{kind} {dtype} {name} [{branch}]")


@pytest.mark.parametrize("what", ["strided_a", "strided_out"])
@pytest.mark.parametrize("layout", ["rm", "shuf"])
def test_skinny_strided(table_only, what, layout):
    """A with a row stride of K + 64 elements, and an output (and residual) with a row stride of
    2 N + 8, at (33, 2306, 768): row-major M>32 narrow CFG(4,1,2,false,4), fragment order
    CFG_MS(2,2,false,4)."""
    from distributed_neural_networks_amd.ops.gemm import linear
    M, N, K = 33, 2306, 768
    for kind, dtype in (("dense", F32), ("thin", BF16)):
        c = ge.device_case(kind, M, N, K, device=DEV, m_cap=64)
        a, r, ldc = c.a, c.res, None
        if what == "strided_a":
            wide = torch.full((M, K + 64), float("nan"), dtype=BF16, device=DEV)
            wide[:, :K] = c.a
            a = wide[:, :K]
        else:
            ldc = 2 * N + 8
            rw = torch.full((M, ldc), float("nan"), dtype=BF16, device=DEV)
            rw[:, :N] = c.res
            r = rw[:, :N]
        buf = ge.nan_buffer(M, N, dtype, DEV, ldc)
        linear(a, c.w, c.bias, None, r, out=buf[:M, :N], w_shuf=_shuf(c, (kind, N, K)) if layout == "shuf" else None)
        ge.assert_exact(buf, M, N, ge.want(c, dtype), f"{kind} {what}")


# ----------------------------------------------------------------------------- 2. the pins
@pytest.mark.parametrize("pin", [1, 2, 3, 4, 5, 6])
def test_skinny_pins(pin):
    """``gemm_set_skinny_pin(id, ks)`` on fragment-order bf16 weights, ``thin``, bias + residual:

      id   M = 17             M = 64 (33..64 rows: the table's 4-row-tile sibling of the line)
      1    CFG(2,1,2,false)   CFG(4,1,2,false)
      2    CFG(2,1,8,false)   CFG(4,1,8,false)
      3    CFG(2,2,2,true)    CFG(4,2,2,false)
      4    CFG(2,4,2,false)   CFG(4,4,2,false)
      5    CFG_MS(2,4,false)  the same: one 16-row tile per workgroup
      6    CFG_MS(1,4,false)  the same

    each with ks = 1, 2, 4, 8 waves per workgroup; at K = 192 (6 chunks) 8 runs as 4, and id 4 at
    M = 64 runs 8 as 4 (64 KiB of LDS).  Before this test ids 1-4 ran their 2-row-tile kernel at
    every M and left rows 32.. of a 33..64-row output unwritten.

    A pinned call bypasses the one-shot and stream plans, so no other switch is needed."""
    from distributed_neural_networks_amd.ops._lib import lib
    from distributed_neural_networks_amd.ops.gemm import linear
    try:
        for ks in (1, 2, 4, 8):
            assert lib().gemm_set_skinny_pin(pin, ks, 0, 0) == 0
            for M in (17, 64):
                for N, K in ((1040, 768), (4112, 192)):
                    c = ge.device_case("thin", M, N, K, device=DEV, m_cap=64)
                    buf = ge.nan_buffer(M, N, BF16, DEV)
                    linear(c.a, c.w, c.bias, None, c.res, out=buf[:M, :N], w_shuf=_shuf(c, ("thin", N, K)))
                    ge.assert_exact(buf, M, N, ge.want(c, BF16), f"pin {pin} ks {ks} ({M}, {N}, {K})")
    finally:
        lib().gemm_set_skinny_pin(0, 4, 0, 0)


# ----------------------------------------------------------------------------- 3. W8A16
W8A16 = [
    (1, 16400, 64, "shuf", "M<=8, W8, Wsh, N>=16384: CFG(1,2,2,false,2)"),
    (1, 4112, 192, "shuf", "M<=8, Wsh, 4096<N<16384: CFG(1,1,4,false,4)"),
    (1, 100, 128, "rm", "M<=8: CFG(1,1,4,false,8)"),
    (8, 16400, 128, "shuf", "M<=8, W8, Wsh, N>=16384: CFG(1,2,2,false,2)"),
    (8, 2306, 192, "rm", "M<=8: CFG(1,1,4,false,8); scalar epilogue"),
    (9, 16400, 64, "shuf", "M<=16, wide: CFG(1,4,2,false,2)"),
    (9, 1040, 768, "rm", "M<=16: CFG(1,2,2,true,4)"),
    (16, 2308, 192, "shuf", "M<=16: CFG(1,2,2,true,4)"),
    (17, 16400, 64, "shuf", "Wsh, wide, M<=32: CFG(2,4,2,false,2)"),
    (17, 100, 192, "shuf", "Wsh, N<=1024: CFG_MS(1,4,false,4)"),
    (17, 4112, 768, "shuf", "Wsh, W8, N>4096: CFG_MS(4,2,false,4)"),
    (17, 2064, 8192, "shuf", "Wsh, kbytes>=8192 (W8: kbytes = K): CFG_MS(2,4,false,4)"),
    (17, 2306, 768, "shuf", "Wsh: CFG_MS(2,2,false,4)"),
    (17, 100, 64, "rm", "row-major, N<=1024: CFG_MS(1,2,true,4)"),
    (17, 2308, 192, "rm", "row-major, W8, N<=4096: CFG_MS(2,2,true,4)"),
    (17, 4112, 192, "rm", "M<=32: CFG(2,2,2,true,4)"),
    (17, 16400, 64, "rm", "M<=32, wide: CFG(2,4,2,false,2)"),
    (32, 4112, 192, "rm", "M<=32: CFG(2,2,2,true,4)"),
    (33, 16400, 128, "shuf", "Wsh, wide, M>32: CFG(4,4,2,false,2)"),
    (33, 4112, 8192, "shuf", "Wsh, W8, N>4096: CFG_MS(4,2,false,4)"),
    (33, 4112, 768, "rm", "M>32: CFG(4,2,2,false,4)"),
    (33, 16400, 64, "rm", "M>32, wide: CFG(4,4,2,false,2)"),
    (64, 1040, 768, "shuf", "Wsh: CFG_MS(2,2,false,4)"),
    (64, 2064, 128, "rm", "row-major, N<=2048: CFG_MS(2,2,true,4)"),
    (65, 100, 192, "rm", "M>64, N<=1024: CFG_MS(1,4,false,4)"),
    (100, 2306, 192, "shuf", "M>64: CFG_MS(2,2,false,4)"),
    (256, 1040, 128, "rm", "M>64: CFG_MS(2,2,false,4)"),
]


@pytest.mark.parametrize("M,N,K,layout,branch", W8A16, ids=[f"{m}x{n}x{k}-{l}" for m, n, k, l, _ in W8A16])
def test_w8a16(table_only, M, N, K, layout, branch):
    """``linear_w8`` with norm 0 on ``w8`` (``dense`` and ``thin`` ints as e4m3 bytes, channel
    scale 2^-(3 + n % 3)), with and without the fragment-order copy; no epilogue and bias +
    residual (the W8A16 entry has no ReLU).  Branches: the last column of ``W8A16`` (W8: kbytes = K,
    so the deep class, kbytes >= 16384, is beyond these fixtures; the bf16 cases reach its lines)."""
    from distributed_neural_networks_amd.ops.fp8 import linear_w8
    for kind in ("dense", "thin"):
        c = ge.device_case(kind, M, N, K, "w8", device=DEV, m_cap=_m_cap(M))
        w = _w8(c, (kind, N, K), layout == "shuf")
        for name, act, bias, res in EPIS[:2]:
            buf = ge.nan_buffer(M, N, BF16, DEV)
            linear_w8(c.a, w, c.bias if bias else None, 0, c.res if res else None, buf[:M, :N])
            ge.assert_exact(buf, M, N, ge.want(c, BF16, act, bias, res), f"{kind} {name} [{branch}]")


@pytest.mark.parametrize("M", [1, 8])
def test_w8a16_vocabulary_wide(table_only, M):
    """M<=8, W8, Wsh, N >= 65536: CFG(1,2,4,false,8).  N = 65552 (a ragged last tile) at K = 128;
    the weight rows are the ``thin`` fixture's 16400 rows tiled, so that generation stays cheap:
    row n holds fixture row n % 16400, scale and bias included."""
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight, linear_w8
    from distributed_neural_networks_amd.ops.gemm import shuffle_weight
    N, K, N0 = 65552, 128, ge.N_MAX
    c = ge.device_case("thin", M, N0, K, "w8", device=DEV, m_cap=64)
    idx = torch.arange(N, device=DEV) % N0
    q = c.w.view(torch.uint8)[idx].contiguous().view(torch.float8_e4m3fn)
    sw, bias = c.sw[idx].contiguous(), c.bias[idx].contiguous()
    w = Fp8Weight(q, sw, K, shuffle_weight(q))
    y = ge.expected(c.prod64[:, idx] + bias.double() + 0.0, BF16, exact=True)
    buf = ge.nan_buffer(M, N, BF16, DEV)
    linear_w8(c.a, w, bias, 0, None, buf[:M, :N])
    ge.assert_exact(buf, M, N, y, "N = 65552")


@pytest.mark.parametrize("M", [1, 16, 17, 64])
@pytest.mark.parametrize("route", ["rm", "shuf", "stream", "oneshot"])
def test_w8_codes(M, route):
    """The in-register e4m3 -> bf16 conversion on all 254 finite bytes (subnormals, +-0, +-448):
    one-hot rows +-2^j select one weight byte per output, output = W[n, k(m)] scale_n A[m, k(m)],
    exact in bf16.  (M, 300, 256):

      route     M = 1               M = 16              M = 17, 64
      rm        CFG(1,1,4,false,8)  CFG(1,2,2,true,4)   CFG_MS(1,2,true,4)
      shuf      CFG(1,1,4,false,8)  CFG(1,2,2,true,4)   CFG_MS(1,4,false,4)
      stream    as shuf (the stream and one-shot        gemm_stream_kernel W8, one slice
      oneshot   kernels start at 17 rows)               gemm_oneshot_kernel W8, forced plan
    """
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight, linear_w8
    from distributed_neural_networks_amd.ops.gemm import set_oneshot_gemm, set_stream_gemm, shuffle_weight
    f = ge.codes_fixture(M)
    y = ge.codes_reference64(f).to(BF16).to(DEV)
    q = f.wq.to(DEV).view(torch.float8_e4m3fn)
    w = Fp8Weight(q, f.sw.to(DEV), ge.CODES_K, None if route == "rm" else shuffle_weight(q))
    buf = ge.nan_buffer(M, ge.CODES_N, BF16, DEV)
    try:
        set_stream_gemm(2 if route == "stream" else 0, 1, 0)
        set_oneshot_gemm(2 if route == "oneshot" else 0)
        linear_w8(f.a.to(BF16).to(DEV), w, None, 0, None, buf[:M, :ge.CODES_N])
    finally:
        set_stream_gemm(1, 8 << 20, 0)
        set_oneshot_gemm(1)
    ge.assert_exact(buf, M, ge.CODES_N, y, f"codes {route}")


# ----------------------------------------------------------------------------- 4. the stream kernel
STREAM_SHAPES = ((640, 1024), (100, 192), (2306, 4096), (2306, 3840))


@pytest.mark.parametrize("fold", [0, 1], ids=["reduce", "fold"])
@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("split", [False, True], ids=["one_slice", "split"])
def test_stream(fold, w8, split):
    """The stream kernel forced (``set_stream_gemm(2, 1, fold)``, one-shot off), M in {17, 32}
    (``launch_stream_mt`` MT 2) and {33, 64} (MT 4), ``thin`` and ``dense`` on bf16 output, no
    epilogue and bias + residual.  A K-step is 256 k (bf16: 8 chunks, W8: 4); forced, with the
    workspace, ``stream_plan`` gives

      (N, K)         column tiles   K-steps   slices with the workspace
      (640, 1024)    5              4         4 of 1 step
      (100, 192)     1              1         1 (nothing to split; a partial K-step)
      (2306, 4096)   19             16        8 of 2 steps
      (2306, 3840)   19             15        8: seven of 2 steps and a last one of 1

    and one slice each without it.  Split slices are combined in the launch by the last-arriving
    workgroup (fold) or by ``gemm_stream_reduce`` (reduce).  The calls of one test follow each
    other on one workspace without a synchronisation, shapes and slice counts alternating, so
    each runs on the tickets the one before re-armed; they must all be zero afterwards."""
    from distributed_neural_networks_amd.ops.fp8 import linear_w8
    from distributed_neural_networks_amd.ops.gemm import decode_workspace, linear, set_oneshot_gemm, set_stream_gemm
    ws = decode_workspace(DEV, 6) if split else None
    runs = []
    try:
        set_oneshot_gemm(0)
        set_stream_gemm(2, 1, fold)
        for M in (17, 32, 33, 64):
            for N, K in STREAM_SHAPES:
                for kind in ("thin", "dense"):
                    c = ge.device_case(kind, M, N, K, "w8" if w8 else "bf16", device=DEV, m_cap=64)
                    for name, act, bias, res in EPIS[:2]:
                        buf = ge.nan_buffer(M, N, BF16, DEV)
                        b, r = c.bias if bias else None, c.res if res else None
                        if w8:
                            linear_w8(c.a, _w8(c, (kind, N, K), True), b, 0, r, buf[:M, :N], ws=ws)
                        else:
                            linear(c.a, c.w, b, None, r, out=buf[:M, :N], w_shuf=_shuf(c, (kind, N, K)), ws=ws)
                        runs.append((buf, M, N, ge.want(c, BF16, act, bias, res), f"{kind} {name} ({M}, {N}, {K})"))
        torch.cuda.synchronize()
    finally:
        set_stream_gemm(1, 8 << 20, 0)
        set_oneshot_gemm(1)
    for run in runs:
        ge.assert_exact(*run)
    if split:
        assert int(ws[-4096:].view(torch.int32).abs().sum()) == 0  # every ticket re-armed


# ----------------------------------------------------------------------------- 5. the one-shot kernel
OS_SHAPES = ((200, 512), (1000, 2048), (2306, 768))
OS_ROWS = (17, 33, 50, 64)
OS_CONFIGS = [(1, 1, 1, 1), (1, 4, 2, 3), (2, 2, 1, 2), (2, 4, 2, 1), (4, 1, 1, 1), (4, 4, 1, 4), (1, 1, 1, 2), (4, 4, 2, 4)]


def _os_covers(cfg, w8, K):
    """``os_plan`` for a pinned configuration: the weight registers fit (NTW x STEPS x CS x 4 <=
    128), MT 4 has one LDS step, and a slice of ceil(chunks / split-K) chunks fits the 4 waves x
    STEPS x CS chunks of a workgroup."""
    mt, ntw, steps, sk = cfg
    cs = 4 if w8 else 8
    nch = (K if w8 else 2 * K) // 64
    if (mt == 4 and steps == 2) or ntw * steps * cs > 32:
        return False
    return -(-nch // sk) <= 4 * steps * cs


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_oneshot_forced(w8):
    """``set_oneshot_gemm(2)``: the forced plan (MT 2; STEPS 1 up to 4 x CS chunks, else 2;
    split-K = ceil(chunks / (4 STEPS CS)); NTW 4 or 2 where that still gives 256 workgroups,
    else 1) with bias + residual, on ``thin`` and ``dense``:

      (N, K)         bf16 (CS 8): chunks, STEPS, split-K   W8 (CS 4): chunks, STEPS, split-K
      (200, 512)     16, 1, 1                              8, 1, 1
      (1000, 2048)   64, 2, 1                              32, 2, 1
      (2306, 768)    24, 1, 1                              12, 1, 1
    """
    from distributed_neural_networks_amd.ops.fp8 import linear_w8
    from distributed_neural_networks_amd.ops.gemm import decode_workspace, linear, set_oneshot_gemm
    ws = decode_workspace(DEV)
    try:
        set_oneshot_gemm(2)
        for M in OS_ROWS:
            for N, K in OS_SHAPES:
                for kind in ("thin", "dense"):
                    c = ge.device_case(kind, M, N, K, "w8" if w8 else "bf16", device=DEV, m_cap=64)
                    buf = ge.nan_buffer(M, N, BF16, DEV)
                    if w8:
                        linear_w8(c.a, _w8(c, (kind, N, K), True), c.bias, 0, c.res, buf[:M, :N], ws=ws)
                    else:
                        linear(c.a, c.w, c.bias, None, c.res, out=buf[:M, :N], w_shuf=_shuf(c, (kind, N, K)), ws=ws)
                    ge.assert_exact(buf, M, N, ge.want(c, BF16), f"{kind} ({M}, {N}, {K})")
    finally:
        set_oneshot_gemm(1)


@pytest.mark.parametrize("cfg", OS_CONFIGS, ids=["-".join(map(str, c)) for c in OS_CONFIGS])
def test_oneshot_pinned(cfg):
    """``gemm_oneshot_sweep`` with an explicit (rows / 16, column tiles, LDS steps, split-K), plain
    product on ``thin``, every M in {17, 33, 50, 64}.  The return code is asserted: 0 where
    ``os_plan`` covers the (configuration, K), else -1 with the output untouched.

      configuration   bf16: K 512 / 2048 / 768                W8: K 512 / 2048 / 768
      1-1-1-1         runs / 64 chunks > 32 / runs            runs / 32 chunks > 16 / runs
      1-4-2-3         64 weight registers over the 32 cap     runs at every K
      2-2-1-2         runs at every K                         runs at every K
      2-4-2-1         over the register cap                   runs at every K
      4-1-1-1         runs / declined / runs                  runs / declined / runs
      4-4-1-4         runs at every K                         runs at every K
      1-1-1-2         runs at every K                         runs at every K
      4-4-2-4         declined everywhere: ``os_plan`` refuses MT 4 with two LDS steps (256 KB of
                      LDS) and the kernel is not instantiated, so there is nothing to run; the
                      case asserts the refusal and that nothing is written.
    """
    from distributed_neural_networks_amd.ops._lib import lib, ptr, stream_ptr
    from distributed_neural_networks_amd.ops.gemm import decode_workspace
    mt, ntw, steps, sk = cfg
    ws = decode_workspace(DEV)
    ran = 0
    for w8 in (False, True):
        for N, K in OS_SHAPES:
            for M in OS_ROWS:
                c = ge.device_case("thin", M, N, K, "w8" if w8 else "bf16", device=DEV, m_cap=64)
                wsh = _fp8_weight(c, ("thin", N, K))[1] if w8 else _shuf(c, ("thin", N, K))
                buf = ge.nan_buffer(M, N, BF16, DEV)
                rc = lib().gemm_oneshot_sweep(ptr(c.a), K, ptr(wsh), ptr(c.sw), ptr(buf), buf.stride(0), M, N, K, mt,
                                              ntw, steps, sk, int(w8), ptr(ws), ws.numel(), stream_ptr())
                what = f"{cfg} w8={w8} ({M}, {N}, {K})"
                if _os_covers(cfg, w8, K):
                    assert rc == 0, what
                    ge.assert_exact(buf, M, N, ge.want(c, BF16, None, False, False), what)
                    ran += 1
                else:
                    assert rc == -1, what
                    assert bool(buf.isnan().all()), what
    assert (ran > 0) != (cfg == (4, 4, 2, 4)), f"{cfg} ran {ran} times"


# ----------------------------------------------------------------------------- 6. the fused head
@pytest.mark.parametrize("K", [256, 768, 1024, 1280, 1600])
@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_head(K, w8):
    """``gemm_head`` with norm 0 and no column sums, then ``argmax_final``; ``thin``, M in
    {1, 17, 64}, N in {512, 3000}.  Every instantiated width (``launch_head``):

      K      bf16 (chunks, per K pass, per group)   W8
      256    8, 8, 8                                4, 4, 4
      768    24, 24, 12                             12, 12, 4
      1024   32, 32, 8                              16, 16, 4
      1280   40, 20, 10 (two K passes)              20, 10, 5 (two K passes)
      1600   50, 28, 7  (two K passes)              25, 14, 5 (two K passes)

    The grid is ceil(N / 128) workgroups (4 and 24: asserted from the return value), each owning a
    contiguous range of 16-column tiles.  Rows n1 < n2 < n3 of W are identical (bias and channel
    scale included), lie in different workgroups' ranges and carry a bias that makes them the
    maximum of every row: the logits are exact, the merged argmax is n1 in every row, and
    ``argmax_final``'s copy (``out2``) and position increment (``pos_inc``) are exact."""
    from distributed_neural_networks_amd.ops._lib import lib, ptr, stream_ptr
    from distributed_neural_networks_amd.ops.gemm import HEAD_PART_PER_ROW, shuffle_weight
    for N, tied in ((512, (6, 201, 420)), (3000, (9, 1500, 2991))):
        base = ge.device_case("thin", 64, N, K, "w8" if w8 else "bf16", device=DEV)
        n1, n2, n3 = tied
        w = base.w.clone().view(torch.uint8)  # (N, row bytes): rows copied as bytes, bf16 and e4m3 alike
        w[n2], w[n3] = w[n1], w[n1]
        bias = base.bias.clone()
        unit = 1.0
        if w8:
            assert base.sw[n1] == base.sw[n2] == base.sw[n3] == 2.0**-3  # n % 3 == 0: the largest channel scale
            unit = 2.0**-3
        bias[[n1, n2, n3]] = 180.0 * unit
        prod = base.prod64.clone()
        prod[:, n2], prod[:, n3] = prod[:, n1], prod[:, n1]
        y64 = prod + bias.double() + 0.0
        ntile16 = -(-N // 16)
        grid = -(-ntile16 // 8)
        owner = {max(b for b in range(grid) if b * ntile16 // grid <= n // 16) for n in tied}
        assert len(owner) == 3  # three different workgroups' tile ranges (gemm_head.h wt0 / wt1)
        assert bool((y64.argmax(1) == n1).all()) and bool((y64.max(1).values == y64[:, n3]).all())
        assert bool((y64.topk(4, dim=1).values[:, 3] < y64[:, n1]).all())  # the tied three are alone at the top
        wsh = shuffle_weight(w)
        for M in (1, 17, 64):
            want = ge.expected(y64[:M], BF16, exact=True)
            logits = ge.nan_buffer(M, N, BF16, DEV)
            part = torch.zeros(2 * HEAD_PART_PER_ROW * M, dtype=torch.int32, device=DEV)
            out = torch.full((M,), -1, dtype=torch.int32, device=DEV)
            also = torch.full((M,), -1, dtype=torch.int32, device=DEV)
            adv = torch.arange(M, dtype=torch.int32, device=DEV) * 3
            S = lib().gemm_head(ptr(base.a), base.a.stride(0), ptr(wsh), ptr(base.sw) if w8 else 0, 0, ptr(bias), 0.0, 0,
                                ptr(logits), logits.stride(0), M, N, K, int(w8), ptr(part), HEAD_PART_PER_ROW,
                                stream_ptr())
            assert S == grid, (S, grid)
            assert lib().argmax_final(ptr(part), S, M, ptr(out), ptr(also), ptr(adv), stream_ptr(), 0, 0) == 0
            what = f"head K={K} w8={w8} ({M}, {N})"
            ge.assert_exact(logits, M, N, want, what)
            assert bool((out == n1).all()), (what, out)
            assert torch.equal(also, out), what
            assert torch.equal(adv, torch.arange(M, dtype=torch.int32, device=DEV) * 3 + 1), what
