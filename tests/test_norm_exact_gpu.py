"""LayerNorm / RMSNorm and every folded-norm GEMM route held to the element-exact fixtures of
tests/norm_exact.py: the plain norm and row-statistics kernels, the prefill fold (row statistics + tile
GEMM epilogue, QKV scatter), the skinny kernels, the stream kernel, the one-shot kernel, W8A16, the
fused vocabulary head, the producer / consumer row statistics and graph replay.

The expected output is bf16(y64), y64 the fp64 value of ``rstd (acc - mean colsum) + bias' -> act
(+ residual)``; the device must equal it bit for bit at every element whose y64 is further than
``tau S`` from a bf16 rounding boundary (``norm_exact.TAU``, 16 times the need of the fp32 mirrors, set
on the CPU by tests/test_norm_exact.py).  Every output lands in a NaN-filled buffer taller and wider
than (M, N) whose margin must stay NaN.  Each test prints the number of elements it compared and left
out.

Forms of ``S`` (norm_exact.condition): ``two_pass`` for the plain norm, the row statistics and the
prefill fold; ``one_pass`` for the skinny, stream, one-shot and head kernels, which shift by the row's
first element; ``partials`` for the one-shot kernel merging its producer's tile partials.

The stream and one-shot kernels are not instantiated for ReLU (``launch_skinny``: ACT_RELU goes to the
skinny table), so their cases run without an activation.  Which kernel ran is read from what the
library reports: a skinny or unsplit one-shot launch writes the armed ``rs_out`` partials and the
stream kernel and the split-K one-shot launch do not (``gemm_rowstats_written``); only the one-shot
kernel reads ``rs_in``, so a poisoned partial that moves its row shows that it ran; the head returns
its grid.  The quantising norms (``layernorm_q8``, ``layernorm_q8_mx``) are not covered here.
"""
import pytest
import torch

import gemm_exact as ge
import norm_exact as ne

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
TAU = ne.TAU

_COUNT = {}


def _tally(route, r):
    c = _COUNT.setdefault(route, [0, 0])
    c[0] += r[0]
    c[1] += r[1]


def _report(route):
    c = _COUNT.get(route, [0, 0])
    print(f"norm_exact[{route}]: {c[0]} elements compared, {c[1]} left out")


class _Case:
    """One fixture on the device: activations, the folded layer (row-major and with its fragment-order
    copy), the residual and the fp64 terms, made once at ``M`` rows; smaller M are prefixes."""

    def __init__(self, kind, M, N, K, rms, wfmt, bias, x=None):
        from distributed_neural_networks_amd.ops.fp8 import Fp8Weight
        from distributed_neural_networks_amd.ops.gemm import FoldedLinear, shuffle_weight
        fx = ne.fixture(kind, M, N, K, wfmt) if x is None else ne.fixture_from_x(kind, x, N, wfmt)
        self.fx, self.rms, self.M, self.N, self.K = fx, rms, M, N, K
        self.x = fx.x.to(BF16).to(DEV)
        self.res = fx.res.to(BF16).to(DEV)
        f = ne.folded(fx, rms, DEV, bias)
        ne.assert_fold_exact(f, fx, rms, bias)
        self.f_rm = f
        if wfmt == "w8":
            w = Fp8Weight(f.w.q, f.w.scale, f.w.k, shuffle_weight(f.w.q[:, :K]))
            self.f_sh = FoldedLinear(w, f.bias, f.colsum, f.norm, f.eps)
        else:
            self.f_sh = FoldedLinear(f.w, f.bias, f.colsum, f.norm, f.eps)
            self.f_sh.ws = shuffle_weight(f.w)
        self.base = ne.terms(fx, rms, bias=bias, res=True, device=DEV)
        x64 = fx.x.double()
        self.cond = {}
        for form in ne.FORMS:
            c = ne.condition(x64, form, rms)
            self.cond[form] = None if c is None else c.to(DEV)

    def terms(self, M, act=None, res=True, form="one_pass"):
        t = self.base.with_(act=None if act in (None, "none") else act, res=self.base.res if res else None,
                            cond=self.cond[form])
        return t.rows(M)


_CASES = {}


def _case(kind, M, N, K, rms, wfmt="bf16", bias=True):
    key = (kind, M, N, K, rms, wfmt, bias)
    if key not in _CASES:
        _CASES[key] = _Case(*key)
    return _CASES[key]


@pytest.fixture
def table_only():
    """Stream and one-shot kernels off: every decode call takes the skinny table."""
    from distributed_neural_networks_amd.ops.gemm import set_oneshot_gemm, set_stream_gemm
    set_stream_gemm(0)
    set_oneshot_gemm(0)
    try:
        yield
    finally:
        set_stream_gemm(1, 8 << 20, 0)
        set_oneshot_gemm(1)


def _arm_rs_out(M, N, rs_in=None):
    """Arm the next decode GEMM with an ``rs_out`` buffer (and ``rs_in`` partials); ``_wrote()`` after the
    call tells whether its kernel wrote the partials (skinny, unsplit one-shot) or not (stream, split-K
    one-shot).  The caller keeps the returned buffer until then."""
    from distributed_neural_networks_amd.ops._lib import lib, ptr
    from distributed_neural_networks_amd.ops.gemm import rowstats_buffer
    rs = rowstats_buffer(M, N, DEV)
    lib().gemm_rowstats(ptr(rs), rs.stride(0) // 2, ptr(rs_in), 0 if rs_in is None else rs_in.stride(0) // 2)
    return rs


def _wrote():
    from distributed_neural_networks_amd.ops._lib import lib
    return bool(lib().gemm_rowstats_written())


# ----------------------------------------------------------------------------- 1. the plain norm
NORM_WIDTHS = list(ne.PLAIN_WIDTHS)


def _plain(N, variant):
    rms = variant == "rms"
    x, gamma, beta, y64, S = ne.plain_case(N, variant)
    return rms, x, gamma, beta, y64.to(DEV), S.to(DEV)


@pytest.mark.parametrize("variant", ["ln_beta", "ln", "rms"])
@pytest.mark.parametrize("N", NORM_WIDTHS)
def test_plain_norm(N, variant):
    """``layernorm`` (norm_kernel): one lane (N = 8), a partial 512-column chunk (520, 1600), both sides
    of the gamma / beta prefetch split (NC <= 8: 4096; NC 16: 8192); M in {1, 5, 37} (a last block with
    one live wave); contiguous, and strided ``ldx`` / ``ldy`` with NaN between the rows.  The band is
    ``TAU_PLAIN``: the plain norm's own mirror sets it, at widths up to 8192."""
    from distributed_neural_networks_amd.ops._lib import check, lib, ptr, stream_ptr
    from distributed_neural_networks_amd.ops.transformer_ops import layernorm
    rms, x, gamma, beta, y64, S = _plain(N, variant)
    xd = x.to(BF16).to(DEV)
    w = gamma.float().to(DEV)
    b = None if beta is None else beta.float().to(DEV)
    for M in (1, 5, 37):
        out = torch.full((M + 3, N), float("nan"), dtype=BF16, device=DEV)
        layernorm(xd[:M], w, b, out, ne.EPS, rms)
        _tally("plain", ne.compare(out[:M], y64[:M], S[:M], ne.TAU_PLAIN, f"{variant} ({M}, {N})"))
        assert bool(out[M:].isnan().all())
        xw = torch.full((M, N + 64), float("nan"), dtype=BF16, device=DEV)
        xw[:, :N] = xd[:M]
        buf = ge.nan_buffer(M, N, BF16, DEV)
        check(lib().layernorm(ptr(xw), xw.stride(0), ptr(w), ptr(b), ptr(buf), buf.stride(0), M, N, ne.EPS, int(rms),
                              stream_ptr()), "layernorm")
        _tally("plain", ne.compare(buf[:M, :N], y64[:M], S[:M], ne.TAU_PLAIN, f"{variant} strided ({M}, {N})"))
        assert bool(buf[M:].isnan().all()) and bool(buf[:M, N:].isnan().all())
    _report("plain")


# ----------------------------------------------------------------------------- 2. row statistics
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("N", NORM_WIDTHS)
def test_row_stats(monkeypatch, N, rms):
    """``row_stats`` at M = 37 with one and four rows per wave (``DNN_ROWSTATS_R``; the last block of
    R = 4 has a wave with one live row): {rstd, -mean rstd} against fp64 to ``ROWSTAT_TOL_LOG2``, 16 times
    the fp32 two-pass mirror's own worst relative error on the same rows, rounded up to a power of two
    and recorded on the CPU (tests/test_norm_exact.py); zeros exactly, a guard row untouched.  Where
    four rows per wave exist (NC <= 4: N <= 2048; wider rows run one row per wave under either setting)
    R = 1 is bitwise equal to R = 4."""
    from distributed_neural_networks_amd.ops.transformer_ops import row_stats
    M = 37
    x = ne.activations(N)[:M]
    xd = x.to(BF16).to(DEV)
    want = ne.stats_of(x.double(), rms).rowstat.to(DEV)
    tol = 2.0 ** ne.ROWSTAT_TOL_LOG2[N][int(rms)]
    got = {}
    for R in (1, 4):
        monkeypatch.setenv("DNN_ROWSTATS_R", str(R))
        st = torch.full((M + 1, 2), 7.0, dtype=torch.float32, device=DEV)
        xw = torch.full((M, N + 64), float("nan"), dtype=BF16, device=DEV)
        xw[:, :N] = xd
        row_stats(xw[:, :N], st, ne.EPS, rms, rows=M, ldx=xw.stride(0))
        err = ((st[:M].double() - want).abs() / want.abs().clamp(min=1e-300))
        err = torch.where(want == 0, (st[:M] != 0).double(), err)
        worst = float(err.max())
        print(f"row_stats N={N} R={R} {'rms' if rms else 'ln'}: worst relative error 2^{torch.log2(err.max().clamp(min=2.0**-60)).item():.1f}, "
              f"tolerance 2^{torch.log2(torch.tensor(tol)).item():.1f}")
        assert worst <= tol, (R, worst, tol, err.argmax().item())
        assert bool((st[M] == 7.0).all())
        got[R] = st[:M].clone()
    if N <= 2048:
        assert torch.equal(got[1], got[4])


# ----------------------------------------------------------------------------- 3. the prefill fold
def _prefill(c, M, N, act, res, through_linear_norm):
    from distributed_neural_networks_amd.ops.gemm import linear, linear_norm, skinny_rows
    from distributed_neural_networks_amd.ops.transformer_ops import row_stats
    buf = ge.nan_buffer(M, N, BF16, DEV)
    r = c.res[:M] if res else None
    std_buf = torch.full((M, c.K), float("nan"), dtype=BF16, device=DEV)
    if through_linear_norm:
        assert not skinny_rows(M, N)
        linear_norm(c.x[:M], c.f_rm, act, r, buf[:M, :N], std_buf=std_buf, ones=torch.ones(c.K, device=DEV))
    else:  # the two calls linear_norm makes above the skinny sizes, at a row count it would send to the skinny kernels
        st = std_buf.reshape(-1)[:4 * M].view(torch.float32).view(M, 2)
        row_stats(c.x[:M], st, ne.EPS, c.rms, rows=M, ldx=c.x.stride(0))
        linear(c.x[:M], c.f_rm.w, c.f_rm.bias, act, r, buf[:M, :N], rowstat=st, colsum=c.f_rm.colsum)
    return buf


@pytest.mark.parametrize("split", [True, False], ids=["tail_split", "no_split"])
@pytest.mark.parametrize("tile", [128, 256, 255])
def test_prefill_fold(tile, split):
    """``row_stats`` + ``linear(..., rowstat=, colsum=)`` (a folded-norm GEMM always takes the tile
    kernels, ``launch_gemm``): the 128^2, 256^2 and 256x128 kernels forced, the tail split on and off;
    M = 65 (odd: the epilogue operands come from global memory) and 300 (even: from their LDS copy,
    through ``linear_norm``); (N, K) = (256, 64) and (520, 768); LayerNorm and RMSNorm; none / ReLU;
    with and without the residual."""
    from distributed_neural_networks_amd.ops.gemm import set_gemm_split_tail, set_gemm_tile
    try:
        set_gemm_tile(tile)
        set_gemm_split_tail(split)
        for kind, N, K in (("dense", 256, 64), ("thin", 520, 768)):
            for rms in (False, True):
                c = _case(kind, 300, N, K, rms)
                for M in (65, 300):
                    for act in (None, "relu"):
                        for res in (True, False):
                            buf = _prefill(c, M, N, act, res, M == 300)
                            what = f"tile {tile} split {split} ({M}, {N}, {K}) rms={rms} {act} res={res}"
                            _tally("prefill", ne.assert_rounded(buf, M, N, c.terms(M, act, res, "two_pass"), TAU, what))
    finally:
        set_gemm_tile(0)
        set_gemm_split_tail(True)
    _report("prefill")


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("B", [2, 3])
def test_qkv_scatter_norm(B, pos0):
    """``qkv_scatter_norm`` (bf16) at T = 128, H = Hkv = 4, hd = 64, K = 256.  B = 2 is 256 rows, which
    ``skinny_rows`` sends to the M-split skinny kernels: the documented decline, False with nothing
    written.  B = 3 (384 rows) must run: q and the cache rows pos .. pos + T - 1 through the mask, the
    other cache rows still NaN."""
    from distributed_neural_networks_amd.ops.gemm import qkv_scatter_norm, skinny_rows
    T, H, hd, K = 128, 4, 64, 256
    M, N, S = B * T, 3 * H * hd, T + 8
    c = _case("dense", 384, N, K, False)
    q = torch.full((B, H, T, hd), float("nan"), dtype=BF16, device=DEV)
    kc = torch.full((B, H, S, hd), float("nan"), dtype=BF16, device=DEV)
    vc = torch.full_like(kc, float("nan"))
    pos = torch.tensor([pos0 + (b % 2) for b in range(B)], dtype=torch.int32, device=DEV)
    std_buf = torch.empty((M, K), dtype=BF16, device=DEV)
    ran = qkv_scatter_norm(c.x[:M], c.f_rm, std_buf, q, kc, vc, pos, B, T, H, H, hd)
    if skinny_rows(M, N):
        assert B == 2 and not ran
        assert bool(q.isnan().all()) and bool(kc.isnan().all()) and bool(vc.isnan().all())
        return
    assert ran
    rows = torch.arange(T, device=DEV)
    got = torch.empty((M, N), dtype=BF16, device=DEV)
    live = torch.zeros((B, S), dtype=torch.bool, device=DEV)
    for b in range(B):
        p = int(pos[b])
        live[b, p:p + T] = True
        got[b * T:(b + 1) * T, :H * hd] = q[b].permute(1, 0, 2).reshape(T, H * hd)
        got[b * T:(b + 1) * T, H * hd:2 * H * hd] = kc[b][:, p + rows].permute(1, 0, 2).reshape(T, H * hd)
        got[b * T:(b + 1) * T, 2 * H * hd:] = vc[b][:, p + rows].permute(1, 0, 2).reshape(T, H * hd)
    t = c.terms(M, None, False, "two_pass")
    _tally("qkv_scatter", ne.compare(got, ne.truth_of(t), ne.magnitude_of(t), TAU, f"qkv scatter B={B} pos0={pos0}"))
    for cache in (kc, vc):
        assert bool(cache.permute(0, 2, 1, 3)[~live].isnan().all()), "a cache row outside [pos, pos + T) was written"
    _report("qkv_scatter")


# ----------------------------------------------------------------------------- 4. the skinny kernels
SKINNY_ROWS = (1, 7, 16, 17, 33, 64)
SKINNY_SHAPES = {"gpt2": ("thin", 1024, 768), "xl": ("dense", 400, 1600)}


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("layout", ["rm", "shuf"])
@pytest.mark.parametrize("shape", list(SKINNY_SHAPES))
def test_skinny_norm(table_only, shape, layout, rms):
    """``gemm_skinny_norm`` through ``linear_norm`` on the skinny table (stream and one-shot off; the
    armed ``rs_out`` comes back written, which only the skinny and one-shot kernels do): M in {1, 7, 16,
    17, 33, 64}, row-major and ``attach_shuffled`` weights, with and without the residual.  The route has
    no ReLU (``dnn_gemm_skinny_norm`` instantiates none, GELU and SwiGLU): the call is rejected, which is
    asserted; ReLU on a folded norm is covered on the prefill fold."""
    from distributed_neural_networks_amd.ops.gemm import linear_norm
    kind, N, K = SKINNY_SHAPES[shape]
    c = _case(kind, 64, N, K, rms)
    f = c.f_sh if layout == "shuf" else c.f_rm
    for M in SKINNY_ROWS:
        for res in (True, False):
            buf = ge.nan_buffer(M, N, BF16, DEV)
            if res:  # armed: the epilogue that also writes the partials; unarmed: the plain one
                armed = _arm_rs_out(M, N)
            linear_norm(c.x[:M], f, None, c.res[:M] if res else None, buf[:M, :N])
            assert not res or _wrote(), "the skinny kernel did not run"
            what = f"skinny {shape} {layout} rms={rms} M={M} res={res}"
            _tally("skinny", ne.assert_rounded(buf, M, N, c.terms(M, None, res), TAU, what))
    with pytest.raises(RuntimeError):  # no ReLU on this route: gemm_skinny_norm instantiates none / GELU / SwiGLU only
        linear_norm(c.x[:7], f, "relu", None, ge.nan_buffer(7, N, BF16, DEV)[:7, :N])
    _report("skinny")


@pytest.mark.parametrize("layout", ["rm", "shuf"])
def test_skinny_norm_strided_rows(table_only, layout):
    """The last position of every sequence: rows of x at a stride of T K elements with NaN in between,
    as ``test_linear_norm_strided_rows``."""
    from distributed_neural_networks_amd.ops.gemm import linear_norm
    kind, N, K = SKINNY_SHAPES["gpt2"]
    T = 5
    for rms in (False, True):
        c = _case(kind, 64, N, K, rms)
        for M in (7, 33):
            h = torch.full((M, T, K), float("nan"), dtype=BF16, device=DEV)
            h[:, T - 1] = c.x[:M]
            buf = ge.nan_buffer(M, N, BF16, DEV)
            linear_norm(h[:, T - 1], c.f_sh if layout == "shuf" else c.f_rm, None, c.res[:M], buf[:M, :N])
            _tally("skinny", ne.assert_rounded(buf, M, N, c.terms(M), TAU, f"strided rows {layout} rms={rms} M={M}"))
    _report("skinny")


# ----------------------------------------------------------------------------- 5. the stream kernel
STREAM_SHAPES = (("thin", 640, 1024), ("dense", 2048, 2048))


@pytest.mark.parametrize("fold", [0, 1], ids=["reduce", "fold"])
@pytest.mark.parametrize("split", [False, True], ids=["one_slice", "split"])
def test_stream_norm(fold, split):
    """The stream kernel forced (``set_stream_gemm(2, 1, fold)``, one-shot off): M in {17, 32, 64},
    (N, K) = (640, 1024) and (2048, 2048), LayerNorm and RMSNorm, with and without the residual; one
    slice, and K split into ``decode_workspace`` (combined in the launch or by the reduce launch).
    The armed ``rs_out`` must come back unwritten: the skinny kernels would have written it."""
    from distributed_neural_networks_amd.ops.gemm import decode_workspace, linear_norm, set_oneshot_gemm, set_stream_gemm
    ws = decode_workspace(DEV, 6) if split else None
    runs = []
    try:
        set_oneshot_gemm(0)
        set_stream_gemm(2, 1, fold)
        for kind, N, K in STREAM_SHAPES:
            for rms in (False, True):
                c = _case(kind, 64, N, K, rms)
                for M in (17, 32, 64):
                    for res in (True, False):
                        buf = ge.nan_buffer(M, N, BF16, DEV)
                        armed = _arm_rs_out(M, N)  # held until _wrote()
                        linear_norm(c.x[:M], c.f_sh, None, c.res[:M] if res else None, buf[:M, :N], ws=ws)
                        assert not _wrote(), "the stream kernel did not run"
                        runs.append((buf, M, N, c.terms(M, None, res), TAU, f"stream ({M}, {N}, {K}) rms={rms} res={res}"))
        torch.cuda.synchronize()
    finally:
        set_stream_gemm(1, 8 << 20, 0)
        set_oneshot_gemm(1)
    for run in runs:
        _tally("stream", ne.assert_rounded(*run))
    if split:
        assert int(ws[-4096:].view(torch.int32).abs().sum()) == 0  # every ticket re-armed
    _report("stream")


# ----------------------------------------------------------------------------- 6. the one-shot kernel
OS_SHAPES = (("thin", 200, 512), ("dense", 1000, 2048), ("thin", 2306, 768))
OS_ROWS = (17, 33, 50, 64)
OS_PINNED = [(1, 1, 1, 1), (2, 2, 1, 2), (4, 1, 1, 1), (4, 4, 1, 4), (1, 1, 1, 2)]  # bf16 configs of test_oneshot_pinned


def _os_covers(cfg, K):
    mt, ntw, steps, sk = cfg
    nch = 2 * K // 64
    if (mt == 4 and steps == 2) or ntw * steps * 8 > 32:
        return False
    return -(-nch // sk) <= 4 * steps * 8


def _os_splitk(cfg, K):
    """The slices a configuration runs with: ceil(chunks / ceil(chunks / split-K)) (launch_os_cfg)."""
    nch = 2 * K // 64
    cps = -(-nch // cfg[3])
    return -(-nch // cps)


def _os_forced(K):
    nch = 2 * K // 64
    steps = 1 if nch <= 32 else 2
    return (2, 0, steps, -(-nch // (32 * steps)))


def _poison_check(c, M, N, K, what):
    """Only the one-shot kernel reads ``rs_in``: with the true partials of x the output meets the
    ``partials`` truth; with one tile partial of one row replaced, that row changes and no other."""
    from distributed_neural_networks_amd.ops.gemm import decode_workspace, linear_norm
    ws = decode_workspace(DEV)
    p = ne.partials32(c.fx.x[:M]).reshape(M, -1).contiguous().to(DEV)
    buf = ge.nan_buffer(M, N, BF16, DEV)
    linear_norm(c.x[:M], c.f_sh, None, c.res[:M], buf[:M, :N], ws=ws, rs_in=p)
    _tally("oneshot_rs_in", ne.assert_rounded(buf, M, N, c.terms(M, None, True, "partials"), TAU, what + " rs_in"))
    row = min(M - 1, 19)  # class (d): a constant but for its spikes, every tile mean matters
    bad = p.clone()
    bad[row, 2 * 3] += 64.0  # tile 3's mean
    buf2 = ge.nan_buffer(M, N, BF16, DEV)
    linear_norm(c.x[:M], c.f_sh, None, c.res[:M], buf2[:M, :N], ws=ws, rs_in=bad)
    diff = (buf[:M, :N] != buf2[:M, :N]).any(1).nonzero().flatten().tolist()
    assert diff == [row], f"{what}: a wrong partial in row {row} changed rows {diff}: rs_in is not read, or rows leak"


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_oneshot_forced_norm(rms):
    """``set_oneshot_gemm(2)``, the shapes of ``test_oneshot_forced``, M in {17, 33, 50, 64}, with and
    without the residual.  All three run unsplit ((1000, 2048) at two LDS steps): the armed ``rs_out`` is
    written, and at every M a poisoned ``rs_in`` partial moves its row, which only the one-shot kernel
    does (the skinny table, the fallback of a declined plan, does not read ``rs_in``)."""
    from distributed_neural_networks_amd.ops.gemm import decode_workspace, linear_norm, set_oneshot_gemm, set_stream_gemm
    ws = decode_workspace(DEV)
    try:
        set_stream_gemm(0)
        set_oneshot_gemm(2)
        for kind, N, K in OS_SHAPES:
            c = _case(kind, 64, N, K, rms)
            unsplit = _os_forced(K)[3] == 1
            for M in OS_ROWS:
                for res in (True, False):
                    buf = ge.nan_buffer(M, N, BF16, DEV)
                    armed = _arm_rs_out(M, N)  # held until _wrote()
                    linear_norm(c.x[:M], c.f_sh, None, c.res[:M] if res else None, buf[:M, :N], ws=ws)
                    assert _wrote() == unsplit
                    what = f"oneshot forced ({M}, {N}, {K}) rms={rms} res={res}"
                    _tally("oneshot", ne.assert_rounded(buf, M, N, c.terms(M, None, res), TAU, what))
                if unsplit:
                    _poison_check(c, M, N, K, f"oneshot forced ({M}, {N}, {K}) rms={rms}")
    finally:
        set_oneshot_gemm(1)
        set_stream_gemm(1, 8 << 20, 0)
    _report("oneshot")
    _report("oneshot_rs_in")


@pytest.mark.parametrize("cfg", OS_PINNED, ids=["-".join(map(str, c)) for c in OS_PINNED])
def test_oneshot_pinned_norm(cfg):
    """A pinned (rows / 16, column tiles, LDS steps, split-K) through ``set_oneshot_gemm``, LayerNorm
    and RMSNorm with the residual, on the (shape, configuration) pairs ``os_plan`` covers (stream off:
    a declined plan would fall to the skinny table, which writes the armed ``rs_out``).  Unsplit: the
    poisoned ``rs_in`` partial shows the one-shot kernel ran (where its partials fit: K / 16 <= 16 x 256 /
    rows); split-K: ``rs_out`` stays unwritten."""
    from distributed_neural_networks_amd.ops.gemm import decode_workspace, linear_norm, set_oneshot_gemm, set_stream_gemm
    ws = decode_workspace(DEV)
    ran = 0
    try:
        set_stream_gemm(0)
        set_oneshot_gemm(1, *cfg)
        for kind, N, K in OS_SHAPES:
            if not _os_covers(cfg, K):
                continue
            split = _os_splitk(cfg, K) > 1
            for rms in (False, True):
                c = _case(kind, 64, N, K, rms)
                for M in OS_ROWS:
                    buf = ge.nan_buffer(M, N, BF16, DEV)
                    armed = _arm_rs_out(M, N)  # held until _wrote()
                    linear_norm(c.x[:M], c.f_sh, None, c.res[:M], buf[:M, :N], ws=ws)
                    assert _wrote() == (not split)
                    what = f"oneshot {cfg} ({M}, {N}, {K}) rms={rms}"
                    _tally("oneshot", ne.assert_rounded(buf, M, N, c.terms(M), TAU, what))
                    ran += 1
                if not split and -(-K // 16) <= 16 * (256 // (16 * cfg[0])):
                    _poison_check(c, 33, N, K, f"oneshot {cfg} ({N}, {K}) rms={rms}")
    finally:
        set_oneshot_gemm(1)
        set_stream_gemm(1, 8 << 20, 0)
    assert ran > 0
    _report("oneshot")


# ----------------------------------------------------------------------------- 7. W8A16
@pytest.mark.parametrize("norm", [1, 2], ids=["rms", "ln"])
@pytest.mark.parametrize("route", ["rm", "shuf", "stream", "oneshot"])
def test_w8_norm(route, norm):
    """``linear_w8`` with norm 1 (RMSNorm) and 2 (LayerNorm; ``colsum`` of the dequantised weight) on
    e4m3 weights with channel scales 2^-(3 + n % 3), (N, K) = (1024, 768), M in {1, 17, 64}, with and
    without the residual.  Routes: the skinny table with row-major and fragment-order weights, the
    stream kernel forced and the one-shot kernel forced (both start at 17 rows: M = 1 takes the table
    on every route).  Evidence of the route: ``rs_out`` (unwritten by the stream kernel alone) and a
    poisoned ``rs_in`` partial at M = 64, which moves its row on the one-shot route alone."""
    from distributed_neural_networks_amd.ops.fp8 import linear_w8
    from distributed_neural_networks_amd.ops.gemm import (decode_workspace, rowstats_buffer, rowstats_written,
                                                         set_oneshot_gemm, set_stream_gemm)
    rms = norm == 1
    N, K = 1024, 768
    c = _case("thin", 64, N, K, rms, "w8")
    f = c.f_rm if route == "rm" else c.f_sh
    ws = decode_workspace(DEV)
    try:
        set_stream_gemm(2 if route == "stream" else 0, 1, 0)
        set_oneshot_gemm(2 if route == "oneshot" else 0)
        for M in (1, 17, 64):
            for res in (True, False):
                buf = ge.nan_buffer(M, N, BF16, DEV)
                rs = rowstats_buffer(M, N, DEV)
                linear_w8(c.x[:M], f.w, f.bias, 0, c.res[:M] if res else None, buf[:M, :N], norm, f.colsum, ne.EPS, ws=ws,
                          rs_out=rs)
                assert rowstats_written() == (not (route == "stream" and M >= 17)), (route, M)
                what = f"w8 {route} norm={norm} M={M} res={res}"
                _tally(f"w8_{route}", ne.assert_rounded(buf, M, N, c.terms(M, None, res), TAU, what))
        # rs_in: only the one-shot kernel reads it.  One poisoned tile partial moves its row there and nothing elsewhere.
        M = 64
        p = ne.partials32(c.fx.x[:M]).reshape(M, -1).contiguous().to(DEV)
        bad = p.clone()
        bad[19, 2 * 3] += 64.0
        outs = []
        for part in (p, bad):
            buf = ge.nan_buffer(M, N, BF16, DEV)
            linear_w8(c.x[:M], f.w, f.bias, 0, c.res[:M], buf[:M, :N], norm, f.colsum, ne.EPS, ws=ws, rs_in=part)
            outs.append(buf)
        form = "partials" if route == "oneshot" else "one_pass"
        _tally(f"w8_{route}", ne.assert_rounded(outs[0], M, N, c.terms(M, None, True, form), TAU, f"w8 {route} rs_in"))
        moved = (outs[0][:M, :N] != outs[1][:M, :N]).any(1).nonzero().flatten().tolist()
        assert moved == ([19] if route == "oneshot" else []), (route, moved)
    finally:
        set_stream_gemm(1, 8 << 20, 0)
        set_oneshot_gemm(1)
    _report(f"w8_{route}")


# ----------------------------------------------------------------------------- 8. the fused head
HEAD_SPIKE = 1024.0
HEAD_N = 1000
HEAD_SPIKES = (0, 17, 500, 992, 999)  # the first column, three workgroups' ranges, the ragged last tile's first and last


def _spiked(f, t, n):
    """The folded head ``f`` and its terms ``t`` with the folded bias of column ``n`` set to
    ``HEAD_SPIKE``: that column wins every row, clear of the runner-up by far more than the band."""
    from distributed_neural_networks_amd.ops.gemm import FoldedLinear
    bias = f.bias.clone()
    bias[n] = HEAD_SPIKE
    g = FoldedLinear(f.w, bias, f.colsum, f.norm, f.eps)
    g.ws = f.ws
    b64 = t.bias.clone()
    b64[n] = HEAD_SPIKE
    return g, t.with_(bias=b64)


def _head_check(t, M, N, logits, out, n, what):
    """Logits through the mask, and the token exactly: in fp64 column ``n`` leads every row by more than
    the two elements' bands and two bf16 ulps, so whatever the device rounds it must return ``n``; the
    token is also the first maximum of the logits as stored (the kernel's own rule)."""
    y, S = ne.truth_of(t), ne.magnitude_of(t)
    r = ne.assert_rounded(logits, M, N, t, TAU, what)
    top = y.topk(2, dim=1)
    band = TAU * (S.gather(1, top.indices).sum(1)) + 2 * ne._ulp(top.values[:, 0], ne.BF16_FMT)
    assert bool((top.indices[:, 0] == n).all()) and bool(((top.values[:, 0] - top.values[:, 1]) > band).all()), what
    assert bool((out[:M] == n).all()), f"{what}: tokens {out[:M].tolist()} for the winner {n}"
    stored = logits[:M, :N].float()
    first = (stored == stored.max(1).values[:, None]).float().argmax(1)
    assert torch.equal(out[:M].long(), first), f"{what}: the token is not the first maximum of the stored logits"
    return r


@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("K", [256, 768, 1600])
def test_head_norm(K, w8, rms):
    """``head_argmax`` (gemm_head.h with the folded norm): K in {256, 768, 1600} (one and two K passes),
    M in {1, 33, 64}, N = 1000 (a ragged last tile), bf16 and W8A16 weights; it must return True.  The
    folded bias is one value per column, so a call has one winner for all its rows; the winner moves
    from call to call over ``HEAD_SPIKES`` (column 0, interior workgroup ranges, columns 992 and 999 of
    the ragged tile), clear of the runner-up in every row, and the token is asserted in every row."""
    from distributed_neural_networks_amd.ops.gemm import HEAD_PART_PER_ROW, head_argmax
    N = HEAD_N
    c = _case("thin", 64, N, K, rms, "w8" if w8 else "bf16")
    for M in (1, 33, 64):
        for n in HEAD_SPIKES:
            f, t = _spiked(c.f_sh, c.terms(M, None, False), n)
            logits = ge.nan_buffer(M, N, BF16, DEV)
            part = torch.zeros(2 * HEAD_PART_PER_ROW * M, dtype=torch.int32, device=DEV)
            out = torch.full((M,), -1, dtype=torch.int32, device=DEV)
            assert head_argmax(c.x[:M], f, logits, part, out), "the fused head declined"
            _tally("head", _head_check(t, M, N, logits, out, n, f"head K={K} w8={w8} rms={rms} M={M} winner {n}"))
    _report("head")


# ----------------------------------------------------------------------------- 9. producer / consumer
@pytest.mark.parametrize("route", ["skinny", "oneshot"])
@pytest.mark.parametrize("N", [392, 768])
def test_rowstats_producer_exact(route, N):
    """A residual-writing projection with ``rs_out=`` on the ``thin`` fixture of gemm_exact.py: the
    stored outputs are whole numbers, so a tile's mean (sum / 16, or / 8 for the last tile of N = 392)
    is exact and so is its M2 wherever 256 M2 stays below 2^24 (whole numbers of 1 / 256, all
    non-negative: every partial sum is exact); those are compared with ``torch.equal``, the rest to
    2^-22.  A guard row and the partials past ceil(N / 16) stay untouched (one surplus tile: 392 is
    24.5 tiles against column tiles of 32 and 64)."""
    from distributed_neural_networks_amd.ops.gemm import (decode_workspace, linear, rowstats_buffer, rowstats_written,
                                                         set_oneshot_gemm, set_stream_gemm, shuffle_weight)
    M, K = 64, 768
    c = ge.device_case("thin", M, N, K, device=DEV)
    nt = -(-N // 16)
    rs = rowstats_buffer(M + 1, N + 32, DEV)
    rs.fill_(7.0)
    buf = ge.nan_buffer(M, N, BF16, DEV)
    try:
        set_stream_gemm(0)
        set_oneshot_gemm(2 if route == "oneshot" else 0)
        linear(c.a, c.w, c.bias, None, c.res, out=buf[:M, :N], w_shuf=shuffle_weight(c.w), ws=decode_workspace(DEV),
               rs_out=rs)
        assert rowstats_written()
    finally:
        set_oneshot_gemm(1)
        set_stream_gemm(1, 8 << 20, 0)
    ge.assert_exact(buf, M, N, ge.want(c, BF16), f"producer {route}")
    st = ne.stats_of(buf[:M, :N].double())
    got = rs[:M, :2 * nt].view(M, nt, 2).double()
    assert torch.equal(got[..., 0], st.partials[..., 0]), "a tile mean is not exact"
    exact = st.partials[..., 1] * 256 < 2**24
    assert torch.equal(got[..., 1][exact], st.partials[..., 1][exact]), "a tile M2 is not exact"
    rel = ((got[..., 1] - st.partials[..., 1]).abs() / st.partials[..., 1].clamp(min=1e-300))[~exact]
    assert rel.numel() == 0 or float(rel.max()) <= 2.0**-22
    print(f"producer {route} N={N}: {int(exact.sum())} of {exact.numel()} tile M2 compared exactly")
    assert int(exact.sum()) >= exact.numel() // 2
    assert bool((rs[M] == 7.0).all()) and bool((rs[:M, 2 * nt:] == 7.0).all()), "written outside the row's partials"


@pytest.mark.parametrize("route", ["skinny", "stream", "oneshot"])
def test_rowstats_consumer(route):
    """The consumer: a folded LayerNorm projection (1024 columns) of the producer's 768-wide output with
    ``rs_in=`` its partials.  The one-shot kernel merges them (``partials`` truth; a poisoned partial
    moves its row and no other); the skinny and stream kernels derive their own statistics (``one_pass``
    truth).  The elements in which the call differs from the same call without ``rs_in`` are counted."""
    from distributed_neural_networks_amd.ops.gemm import (decode_workspace, linear, linear_norm, rowstats_buffer,
                                                         set_oneshot_gemm, set_stream_gemm, shuffle_weight)
    M, N0, K0, N = 64, 768, 768, 1024
    p = ge.device_case("thin", M, N0, K0, device=DEV)
    rs = rowstats_buffer(M, N0, DEV)
    h = torch.empty((M, N0), dtype=BF16, device=DEV)
    ws = decode_workspace(DEV)
    try:
        set_stream_gemm(0)
        set_oneshot_gemm(0)
        linear(p.a, p.w, p.bias, None, p.res, out=h, w_shuf=shuffle_weight(p.w), rs_out=rs)
        torch.cuda.synchronize()
        key = ("consumer", M, N, N0)
        if key not in _CASES:
            _CASES[key] = _Case("thin", M, N, N0, False, "bf16", True, x=h.float().cpu())
        c = _CASES[key]
        set_stream_gemm(2 if route == "stream" else 0, 1, 0)
        set_oneshot_gemm(2 if route == "oneshot" else 0)
        form = "partials" if route == "oneshot" else "one_pass"
        for Mc in (33, 64):
            with_rs, without = ge.nan_buffer(Mc, N, BF16, DEV), ge.nan_buffer(Mc, N, BF16, DEV)
            armed = _arm_rs_out(Mc, N, rs)  # rs_in = rs, and an rs_out that tells the stream kernel from the others
            linear_norm(h[:Mc], c.f_sh, None, c.res[:Mc], with_rs[:Mc, :N], ws=ws)
            assert _wrote() == (route != "stream"), route
            linear_norm(h[:Mc], c.f_sh, None, c.res[:Mc], without[:Mc, :N], ws=ws)
            _tally(f"consumer_{route}", ne.assert_rounded(with_rs, Mc, N, c.terms(Mc, None, True, form), TAU,
                                                          f"consumer {route} M={Mc} rs_in"))
            ne.assert_rounded(without, Mc, N, c.terms(Mc), TAU, f"consumer {route} M={Mc} own statistics")
            n = int((with_rs[:Mc, :N] != without[:Mc, :N]).sum())
            print(f"consumer {route} M={Mc}: {n} of {Mc * N} elements differ between rs_in and own statistics")
            assert route == "oneshot" or n == 0  # the skinny and stream kernels do not read rs_in
        if route == "oneshot":
            bad = rs.clone()
            bad[19, 2 * 5] += 3.0
            a, b = ge.nan_buffer(M, N, BF16, DEV), ge.nan_buffer(M, N, BF16, DEV)
            linear_norm(h, c.f_sh, None, c.res, a[:M, :N], ws=ws, rs_in=rs)
            linear_norm(h, c.f_sh, None, c.res, b[:M, :N], ws=ws, rs_in=bad)
            assert (a[:M, :N] != b[:M, :N]).any(1).nonzero().flatten().tolist() == [19]
    finally:
        set_oneshot_gemm(1)
        set_stream_gemm(1, 8 << 20, 0)
    _report(f"consumer_{route}")


# ----------------------------------------------------------------------------- 10. graph replay
def test_graph_replay(table_only):
    """One skinny LayerNorm projection and the fused head captured in one ``torch.cuda.graph`` and
    replayed three times on inputs changed in place (the rows rotated by 8, 16 and 24, which keeps the
    classes and changes every row; the head's winning column moved in its bias): each replay equals its
    own truth, token included."""
    from distributed_neural_networks_amd.ops.gemm import HEAD_PART_PER_ROW, head_argmax, linear_norm
    M, N, K = 64, 1024, 768
    c = _case("thin", M, N, K, False)
    ch = _case("thin", M, HEAD_N, K, False)
    fh, _ = _spiked(ch.f_sh, ch.terms(M, None, False), 0)
    bias0 = ch.f_sh.bias.clone()
    x = c.x.clone()
    buf, logits = ge.nan_buffer(M, N, BF16, DEV), ge.nan_buffer(M, HEAD_N, BF16, DEV)
    part = torch.zeros(2 * HEAD_PART_PER_ROW * M, dtype=torch.int32, device=DEV)
    out = torch.full((M,), -1, dtype=torch.int32, device=DEV)

    def step():
        linear_norm(x, c.f_sh, None, c.res, buf[:M, :N])
        assert head_argmax(x, fh, logits, part, out)

    step()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for shift, winner in ((8, 999), (16, 0), (24, 500)):
        perm = (torch.arange(M, device=DEV) + shift) % M
        x.copy_(c.x[perm])
        fh.bias.copy_(bias0)
        fh.bias[winner] = HEAD_SPIKE
        buf.fill_(float("nan"))
        logits.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        t = c.terms(M)
        t = t.with_(acc=t.acc[perm], mean=t.mean[perm], rstd=t.rstd[perm], cond=t.cond[perm])
        _tally("graph", ne.assert_rounded(buf, M, N, t, TAU, f"graph replay, rows + {shift}"))
        th = ch.terms(M, None, False)
        th = _spiked(ch.f_sh, th.with_(acc=th.acc[perm], mean=th.mean[perm], rstd=th.rstd[perm], cond=th.cond[perm]),
                     winner)[1]
        _tally("graph", _head_check(th, M, HEAD_N, logits, out, winner, f"graph replay head, rows + {shift}"))
    _report("graph")
