"""Prefill GEMM routes held to the exact-arithmetic fixtures of tests/gemm_exact.py:
the three bf16 tile kernels and the tail split, the fp8 128 / 256 tiles, the
row-major fp8 skinny route, the split activation planes and the MX path.  As in
tests/test_gemm_exact_gpu.py the expected output is the fp64 result (rounded
once for bf16 outputs of ``dense``, unrounded for ``thin``), the comparison is
``torch.equal``, and every output lands in a NaN-filled buffer taller and wider
than (M, N) whose margin must stay NaN.

The fp8 and scaled-fp8 MFMA instructions were the one unknown: whether they sum
grid operands exactly, as the bf16 MFMA does.  ``test_fp8_mfma_sums_exactly``
answers it on the smallest cases (one tile, K = 128) and runs first; the width
it established is ``gemm_exact.FP8_INT_MAX``.
"""
import pytest
import torch

import gemm_exact as ge

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F8 = torch.float32, torch.bfloat16, torch.float8_e4m3fn

EPIS = (("none", None, False, False), ("bias_res", None, True, True), ("relu", "relu", True, True))
ACT_ID = {None: 0, "relu": 1}


def _fp8_weight(c):
    """``Fp8Weight(q, scale, k)`` built directly from the fixture's bytes and power-of-two scales."""
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight, kpad_of
    N, K = c.w.shape
    assert kpad_of(K) == K
    return Fp8Weight(c.w.contiguous(), c.sw.contiguous(), K)


def _run_fp8(c, w, M, N, K, act, bias, res, what, sx=None, a=None, sa=None):
    """``linear_fp8(..., prequantized=True)`` on the fixture's e4m3 rows and row scales."""
    from distributed_neural_networks_amd.ops.fp8 import linear_fp8
    buf = ge.nan_buffer(M, N, BF16, DEV)
    shape_only = torch.empty((M, K), dtype=BF16, device=DEV)  # prequantized: x only gives M and K
    linear_fp8(shape_only, w, c.bias if bias else None, ACT_ID[act], c.res if res else None, buf[:M, :N],
               (c.a if a is None else a).contiguous(), None if sx is not None else (c.sa if sa is None else sa).contiguous(),
               prequantized=True, sx=sx)
    ge.assert_exact(buf, M, N, ge.want(c, BF16, act, bias, res), what)


# ----------------------------------------------------------------------------- the one unknown
@pytest.mark.parametrize("route,M,N", [("tile128", 128, 128), ("tile256", 256, 256), ("skinny", 16, 16)])
def test_fp8_mfma_sums_exactly(route, M, N):
    """The smallest a8w8 cases, one tile at K = 128, no epilogue: ``dense`` ints in [-15, 15] as
    e4m3 bytes with power-of-two row and channel scales.  tile128: ``gemm_fp8_kernel``; tile256:
    ``dnn_gemm_fp8_256``; skinny: the fp8 arm of ``gemm_skinny_kernel``, M<=16 CFG(1,2,2,true,4).
    (The scaled MFMA of the MX path has its own smallest case in ``test_mx``.)"""
    from distributed_neural_networks_amd.ops.fp8 import set_fp8_tile
    c = ge.device_case("dense", M, N, 128, "w8", "a8", device=DEV)
    try:
        set_fp8_tile({"tile128": 128, "tile256": 256, "skinny": 0}[route])
        _run_fp8(c, _fp8_weight(c), M, N, 128, None, False, False, route)
    finally:
        set_fp8_tile(0)


# ----------------------------------------------------------------------------- 7. the bf16 tiles
TILE_SHAPES = ((65, 300, 128), (257, 520, 192), (300, 2306, 768), (512, 512, 4096))


@pytest.mark.parametrize("tile", [128, 256, 255, 0], ids=["128", "256", "256x128", "auto"])
@pytest.mark.parametrize("M,N,K", TILE_SHAPES, ids=["x".join(map(str, s)) for s in TILE_SHAPES])
def test_bf16_tiles(tile, M, N, K):
    """``linear`` with ``set_gemm_tile``: fp32 output on ``dense``, bf16 output on ``dense`` and
    ``thin``; no epilogue, bias + residual, bias + ReLU + residual; on the 256^2 and 256x128 tiles
    both ``gemm_set_res_prefetch`` settings.  Kernel reached (``launch_gemm``):

      shape              128                   256                    255                        auto
      (65, 300, 128)     every setting: the skinny table, row-major M>64 N<=1024 CFG_MS(1,4,false,4):
                         at M <= 256 ``launch_gemm`` streams while 128^2 tiles number under 192 (3)
      (257, 520, 192)    gemm_bf16_tn_kernel   gemm_bf16_256_kernel   gemm_bf16_256_kernel<.,1>  256^2 (6 tiles against 15)
      (300, 2306, 768)   57 tiles, ragged      20 tiles, ragged       38 half tiles              128^2 (57 tiles against 20)
      (512, 512, 4096)   16 tiles              4 tiles, 64 K-tiles    8 half tiles               128^2
    """
    from distributed_neural_networks_amd.ops._lib import lib
    from distributed_neural_networks_amd.ops.gemm import linear, set_gemm_tile
    try:
        set_gemm_tile(tile)
        for prefetch in ((0, 1) if tile in (256, 255) else (1,)):
            lib().gemm_set_res_prefetch(prefetch)
            for kind, dtype in (("dense", F32), ("dense", BF16), ("thin", BF16)):
                c = ge.device_case(kind, M, N, K, device=DEV)
                for name, act, bias, res in EPIS:
                    buf = ge.nan_buffer(M, N, dtype, DEV)
                    linear(c.a, c.w, c.bias if bias else None, act, c.res if res else None, out=buf[:M, :N])
                    ge.assert_exact(buf, M, N, ge.want(c, dtype, act, bias, res),
                                    f"tile {tile} prefetch {prefetch} {kind} {dtype} {name}")
    finally:
        lib().gemm_set_res_prefetch(1)
        set_gemm_tile(0)


@pytest.mark.parametrize("split", [True, False], ids=["split", "single_grid"])
@pytest.mark.parametrize("N", [384, 640])
def test_bf16_tail_split(split, N):
    """The prefill tail split at M = 32768, K = 128, bf16 output on ``thin``, bias + residual.
    A (and the residual) are the fixture's 512 rows tiled 64 times, so that generation and the
    reference stay cheap: row m holds fixture row m % 512.

      N     ``tail_split_cols`` (128 row tiles of 256)
      384   two column tiles: 128 x 1 is no whole round of 256, so no split: one 256^2 grid of 256
            tiles, with the switch on or off
      640   three column tiles: 128 x 2 = 256 tiles are one round, the last 128 columns run as 128
            256x128 tiles in a second launch; off: one 256^2 grid of 384 tiles
    """
    from distributed_neural_networks_amd.ops.gemm import linear, set_gemm_split_tail
    M, K, reps = 32768, 128, 64
    c = ge.device_case("thin", ge.M_MAX, N, K, device=DEV)
    a, r = c.a.repeat(reps, 1), c.res.repeat(reps, 1)
    want = ge.want(c, BF16).repeat(reps, 1)
    buf = ge.nan_buffer(M, N, BF16, DEV)
    try:
        set_gemm_split_tail(split)
        linear(a, c.w, c.bias, None, r, out=buf[:M, :N])
    finally:
        set_gemm_split_tail(True)
    ge.assert_exact(buf, M, N, want, f"tail split {split} N {N}")


# ----------------------------------------------------------------------------- 8. the fp8 tiles
FP8_SHAPES = ((300, 520, 256), (512, 1600, 1664))


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("M,N,K", FP8_SHAPES, ids=["x".join(map(str, s)) for s in FP8_SHAPES])
def test_fp8_tiles(tile, M, N, K):
    """``linear_fp8(..., prequantized=True)`` on ``a8w8`` (``dense`` and ``thin`` ints as e4m3
    bytes, row scale 2^-(2 + m % 3), channel scale 2^-(3 + n % 3)); no epilogue, bias + residual,
    bias + ReLU + residual.  ``set_fp8_tile(128)``: ``gemm_fp8_kernel``; 256:
    ``dnn_gemm_fp8_256`` (both shapes have M, N >= 256)."""
    from distributed_neural_networks_amd.ops.fp8 import set_fp8_tile
    try:
        set_fp8_tile(tile)
        for kind in ("dense", "thin"):
            c = ge.device_case(kind, M, N, K, "w8", "a8", device=DEV)
            w = _fp8_weight(c)
            for name, act, bias, res in EPIS:
                _run_fp8(c, w, M, N, K, act, bias, res, f"fp8 tile {tile} {kind} {name}")
    finally:
        set_fp8_tile(0)


@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("N,K", [(520, 256), (4112, 256), (16400, 128)])
def test_fp8_skinny(M, N, K):
    """The row-major fp8 skinny route (``linear_fp8`` at M <= 64: ``gemm_skinny`` with fp8
    operands, no fragment-order copy).  Branch of ``launch_skinny`` (FP8: kbytes = K):

      N       M = 1               M = 17                          M = 64
      520     CFG(1,1,4,false,8)  narrow: CFG(2,1,2,false,4)      narrow: CFG(4,1,2,false,4)
      4112    CFG(1,1,4,false,8)  CFG(2,2,2,true,4)               CFG(4,2,2,false,4)
      16400   CFG(1,1,4,false,8)  wide: CFG(2,4,2,false,2)        wide: CFG(4,4,2,false,2)
    """
    for kind in ("dense", "thin"):
        c = ge.device_case(kind, M, N, K, "w8", "a8", device=DEV, m_cap=64)
        w = _fp8_weight(c)
        for name, act, bias, res in EPIS:
            _run_fp8(c, w, M, N, K, act, bias, res, f"fp8 skinny {kind} {name}")


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("M,N,K", FP8_SHAPES, ids=["x".join(map(str, s)) for s in FP8_SHAPES])
def test_fp8_split_planes(tile, M, N, K):
    """The split-plane GEMM called directly (``gemm_fp8`` over 2 K): hand-built [hi | lo]
    activation planes against ``attach_split``'s ``[q | q / 16]``.  hi is the ``dense`` a8w8
    fixture's A, lo the fixture's next K columns (ints in [-15, 15] too); q / 16 is exact for these
    ints, so the output is ((hi + lo / 16) . q^T) sa sw + bias + residual, a whole number of
    sixteenths of the element's unit: at most 17 x 225 K + 16 (4 x 2^12 + 127 x 64 x 16) of them,
    below 2^24 at K = 1664."""
    from distributed_neural_networks_amd.ops._lib import lib, ptr, stream_ptr
    from distributed_neural_networks_amd.ops.fp8 import attach_split, set_fp8_tile
    assert 17 * 225 * K + 16 * (4 * 2**12 + 127 * 64 * 16) < 2**24
    c = ge.device_case("dense", M, N, K, "w8", "a8", device=DEV)
    lo = ge.fixture("dense", M, 16, 2 * K, "w8", "a8").a[:, K:].to(F8).to(DEV)
    w = attach_split(_fp8_weight(c))
    assert torch.equal(w.q2[:, K:].double() * 16, c.w.double())  # q / 16, exactly
    planes = torch.cat([c.a, lo], dim=1).contiguous()
    w64 = c.w.double() * c.sw.double()[:, None]
    prod = c.prod64 + (lo.double() * c.sa.double()[:, None]) @ (w64 / 16).t()
    want = ge.expected(ge.epilogue64(prod, c.fx), BF16, exact=False)
    buf = ge.nan_buffer(M, N, BF16, DEV)
    try:
        set_fp8_tile(tile)
        rc = lib().gemm_fp8(ptr(planes), ptr(c.sa), ptr(w.q2), ptr(w.scale), ptr(buf), buf.stride(0), ptr(c.bias),
                            ptr(c.res), c.res.stride(0), M, N, 2 * K, 0, stream_ptr())
    finally:
        set_fp8_tile(0)
    assert rc == 0
    ge.assert_exact(buf, M, N, want, f"split planes tile {tile}")


@pytest.mark.parametrize("route", ["tile128", "tile256", "skinny"])
def test_fp8_codes_both_operands(route):
    """Every finite e4m3 byte as a weight and as an activation through the fp8 MFMA's operand
    decoding: one-hot rows holding an e4m3 code select one weight byte per output,
    output = A[m, k(m)] sa_m W[n, k(m)] sw_n, exact in bf16.  (300, 300, 256) on both tiles,
    (64, 300, 256) on the skinny route."""
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight, linear_fp8, set_fp8_tile
    M = 64 if route == "skinny" else ge.CODES_M_MAX
    f = ge.codes_fixture(M, a8=True)
    N, K = ge.CODES_N, ge.CODES_K
    y = ge.codes_reference64(f).to(BF16).to(DEV)
    w = Fp8Weight(f.wq.to(DEV).view(F8), f.sw.to(DEV), K)
    buf = ge.nan_buffer(M, N, BF16, DEV)
    try:
        set_fp8_tile({"tile128": 128, "tile256": 256, "skinny": 0}[route])
        linear_fp8(torch.empty((M, K), dtype=BF16, device=DEV), w, None, 0, None, buf[:M, :N],
                   f.a.to(F8).to(DEV), f.sa.to(DEV), prequantized=True)
    finally:
        set_fp8_tile(0)
    ge.assert_exact(buf, M, N, y, f"codes {route}")


# ----------------------------------------------------------------------------- 9. the MX path
def _mx_dequant(q, sx, M, kp):
    """fp64 values of MX e4m3 rows: byte x 2^(e - 127), e the e8m0 scale of (row, 128-column
    block) at csrc/kernels/common.h mx_index (as tests/test_transformer_gpu.py decodes them)."""
    mpad = (M + 63) // 64 * 64
    t = torch.arange(kp // 128)
    m = torch.arange(M)
    idx = (t[None, :] * (mpad // 64) + (m[:, None] // 64)) * 64 + (m[:, None] % 16) * 4 + (m[:, None] // 16) % 4
    e = sx.reshape(-1)[idx.to(sx.device)].double()
    sc = torch.exp2(e - 127.0).repeat_interleave(128, dim=1)
    return q.reshape(-1)[:M * kp].view(M, kp).view(F8).double() * sc


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (256, 512, 256), (512, 1600, 1664)],
                         ids=["smallest", "256x512x256", "512x1600x1664"])
def test_mx(M, N, K):
    """``quant_rows_mx`` then ``gemm_fp8_mx`` (the scaled MFMA applies the e8m0 block scales).
    The activation is ``thin``-style: the ``thin`` a8w8 fixture's values {0, +-2^-(2 + m % 3)} as
    bf16, so that the block scales differ from row to row; then the ``dense`` a8w8 values, ints
    in [-15, 15] times the same row scales (full-width operands on the scaled MFMA, the block
    maxima differ from block to block).  First the precondition, which does not depend on the
    GEMM: bytes and e8m0 scales decode to the activation **exactly**.  Then the GEMM output
    (bias + residual, and without) must be exact; (256, 256, 128) is the smallest case the path
    takes, one 256^2 tile and one scale block per row."""
    from distributed_neural_networks_amd.ops.fp8 import kpad_of, mx_ok, mx_scale_bytes, quant_rows_mx
    for kind in ("thin", "dense"):
        c = ge.device_case(kind, M, N, K, "w8", "a8", device=DEV)
        w = _fp8_weight(c)
        assert mx_ok(M, N, w)
        x = (c.a.float() * c.sa[:, None]).to(BF16)
        assert torch.equal(x.double(), c.a.double() * c.sa.double()[:, None])
        kp = kpad_of(K)
        q = torch.full((M * kp,), 7, dtype=torch.uint8, device=DEV)
        sx = torch.zeros(mx_scale_bytes(M, kp), dtype=torch.uint8, device=DEV)
        quant_rows_mx(x, q, sx)
        torch.cuda.synchronize()
        assert torch.equal(_mx_dequant(q, sx, M, kp), x.double()), f"{kind}: the MX round trip is not exact"
        for name, act, bias, res in EPIS[:2]:
            _run_fp8(c, w, M, N, K, act, bias, res, f"mx {kind} {name}", sx=sx, a=q)
