"""CPU checks of tests/norm_exact.py: the preconditions of the element-exact norm tests, the fp32
mirrors' need (which sets ``tau``), the masked shares against their caps, and a sensitivity self-test:
every fault the tolerance tests cannot see must show outside the band."""
import math

import pytest
import torch

import gemm_exact as ge
import norm_exact as ne

# (kind, M, N, K): GPT-2's width on the thin grid, GPT-2 XL's and Llama-3's on the dense grid
FIXTURES = [("thin", 64, 1024, 768), ("dense", 64, 400, 1600), ("dense", 33, 512, 4096)]
IDS = [f"{k}-{m}x{n}x{kk}" for k, m, n, kk in FIXTURES]
# log2 of each fixture's worst need over the three mirrors, LayerNorm and RMSNorm, none and ReLU
# (bias + residual), and of the class (e) rows alone under the one-pass mirror; two decimals
RECORDED = {IDS[0]: (-24.15, -25.58), IDS[1]: (-24.58, -26.17), IDS[2]: (-24.05, -30.04)}
# the worst masked shares at TAU over the forms, norms and activations: all, ordinary row, c / f row, column
RECORDED_SHARES = {IDS[0]: [0.03, 0.04, 0.14, 0.141], IDS[1]: [0.028, 0.065, 0.147, 0.109], IDS[2]: [0.031, 0.051, 0.139, 0.182]}


def _lg(v):
    return None if not v else round(math.log2(v), 2)


@pytest.mark.parametrize("fxs", FIXTURES, ids=IDS)
@pytest.mark.parametrize("wfmt", ["bf16", "w8"])
def test_operands_round_trip_and_fold(fxs, wfmt):
    """Activations, gamma-folded weights, bias and residual round-trip through their storage types, the
    worst-case accumulator stays below 2^24 units, and ``fold_norm`` (w8: the (q, scale) construction)
    returns the fp64 fold exactly: weight, bias and column sums."""
    kind, M, N, K = fxs
    fx = ne.fixture(kind, M, N, K, wfmt)
    assert fx.bound_units < 2**24
    assert torch.equal(fx.x.to(torch.bfloat16).float(), fx.x) and torch.equal(fx.x, fx.x.round())
    assert float(fx.x.abs().max()) <= ne.xmax(K)
    assert torch.equal(fx.res.to(torch.bfloat16).float(), fx.res)
    assert set(fx.gamma.abs().tolist()) <= {0.5, 1.0, 2.0}
    for rms in (False, True):
        f64 = ne.fold64(fx, rms)
        unit = (2.0**-5 if kind == "dense" and wfmt == "bf16" else 0.5)
        q_units = ge.units(f64.q, unit)
        acc_units = fx.x.double().abs() @ q_units.abs().t()
        assert float(acc_units.max()) <= fx.bound_units
        for bias in (True, False):
            ne.assert_fold_exact(ne.folded(fx, rms, "cpu", bias), fx, rms, bias)
    cls = ne.row_classes(M)
    x = fx.x.double()
    sd, mu = x.std(1, unbiased=False), x.mean(1)
    for m in range(M):
        if cls[m] == "c":
            assert abs(mu[m]) / sd[m] >= 50
        if cls[m] == "f":
            assert sd[m] == 0
        if cls[m] == "g":
            assert not bool(x[m, :K - 8].any()) and bool(x[m, K - 8:].all())
        if cls[m] == "e":
            assert 4.5 <= abs(x[m, 0] - mu[m]) / sd[m] <= 7.5
        if cls[m] == "d":
            assert int((x[m] != x[m].median()).sum()) == len(ne.spike_positions(K)) == 12


@pytest.mark.parametrize("fxs", FIXTURES[:2], ids=IDS[:2])
def test_accumulator_exact_in_any_order(fxs):
    """x . W'^T in fp32 equals the fp64 product in natural order, shuffled k-chunks and split-K."""
    kind, M, N, K = fxs
    fx = ne.fixture(kind, M, N, K)
    f = ne.fold64(fx, False)
    g = ge.Fixture(kind, "bf16", "bf16", fx.x, None, f.w.float(), None, fx.bias, fx.res, 1.0, fx.bound_units)
    want = fx.x.double() @ f.w.t()
    for seed, slabs in ((None, 1), (1, 1), (2, 4)):
        assert torch.equal(ge.accumulate_fp32(g, seed, slabs).double(), want)


def test_boundary_distance_and_rounding():
    """``round_to`` is torch's own fp32 -> bf16 / e4m3 rounding, and ``boundary_distance`` is the
    distance to the nearest midpoint: worked values, binade edges and the subnormal range."""
    g = torch.Generator().manual_seed(5)
    v = (torch.randn(20000, generator=g) * torch.exp(4 * torch.randn(20000, generator=g))).double()
    assert torch.equal(ne.round_to(v).float().to(torch.bfloat16), v.float().to(torch.bfloat16))
    v8 = v.clamp(-440, 440)
    assert torch.equal(ne.round_to(v8, ne.E4M3_FMT).float(), v8.float().to(torch.float8_e4m3fn).float())
    t = torch.tensor([1.0, 1.00390625, 1.0 + 2.0**-9, 0.998046875, 3.0, 0.0, 2.0**-130], dtype=torch.float64)
    # 1: the boundary below is 1 - 2^-9 (the ulp halves below a power of two); 1 + 2^-8 and 1 - 2^-9: midpoints;
    # 1 + 2^-9: 2^-9 below the midpoint 1 + 2^-8; 3: half an ulp of 2^-6; 0 and 2^-130: half the subnormal ulp
    want = [2.0**-9, 0.0, 2.0**-9, 0.0, 2.0**-7, 2.0**-134, 2.0**-134]
    assert ne.boundary_distance(t).tolist() == want
    e = torch.tensor([1.0, 1.0625, 17.0, 2.0**-9, 2.0**-6], dtype=torch.float64)
    assert ne.boundary_distance(e, ne.E4M3_FMT).tolist() == [2.0**-5, 0.0, 0.0, 2.0**-10, 2.0**-10]
    # the distance is exact: moving y by less than it never changes the rounded value
    d = ne.boundary_distance(v)
    for s in (-0.999, 0.999):
        assert torch.equal(ne.round_to(v + s * d), ne.round_to(v))


@pytest.mark.parametrize("fxs", FIXTURES, ids=IDS)
def test_mirrors_need_tau_and_masked_shares(fxs):
    """The three fp32 mirrors against bf16(y64): their need (the largest boundary distance / S over the
    elements that differ), ``tau`` = 16 x the worst need rounded up to a power of two, and the masked
    shares at that ``tau`` against the caps.  The constants of norm_exact.py equal the computed ones."""
    kind, M, N, K = fxs
    fx = ne.fixture(kind, M, N, K)
    cls = ne.row_classes(M)
    e_rows = [m for m in range(M) if cls[m] == "e"]
    worst, worst_e = 0.0, 0.0
    shares = [0.0, 0.0, 0.0, 0.0]
    for rms in (False, True):
        for act in (None, "relu"):
            for which in ne.MIRRORS:
                t = ne.terms(fx, rms, act=act, form=which)
                y, S = ne.truth_of(t), ne.magnitude_of(t)
                got = ne.mirror(fx, which, rms, act=act)
                need = ne.need_of(got, y, S)
                ndiff = int((got != ne.want_bf16(y)).sum())
                worst = max(worst, need)
                if which == "one_pass":
                    worst_e = max(worst_e, ne.need_of(got, y, S, rows=e_rows))
                masked = ne.mask_of(t, ne.TAU)
                assert not bool(((got != ne.want_bf16(y)) & ~masked).any()), "a mirror differs outside the band"
                share = masked.double()
                rows = share.mean(1)
                ordinary = max(rows[m].item() for m in range(M) if cls[m] not in "cf")
                special = max(rows[m].item() for m in range(M) if cls[m] in "cf")
                print(f"{kind} ({M}, {N}, {K}) {'rms' if rms else 'ln'} {act} {which}: {ndiff} differ, need 2^{_lg(need)}; "
                      f"masked {share.mean().item():.4f} all, {ordinary:.3f} worst ordinary row, {special:.3f} worst "
                      f"large-mean / constant row, {share.mean(0).max().item():.3f} worst column")
                shares = [max(a, b) for a, b in zip(shares, (share.mean().item(), ordinary, special,
                                                            share.mean(0).max().item()))]
                assert share.mean().item() <= ne.CAPS["all"]
                assert ordinary <= ne.CAPS["row"] and special <= ne.CAPS["row_cf"]
                assert share.mean(0).max().item() <= ne.CAPS["col"]
                assert not bool(masked.all(1).any()) and not bool(masked.all(0).any())
    print(f"{kind} ({M}, {N}, {K}): worst need 2^{_lg(worst)}, class (e) rows under one_pass 2^{_lg(worst_e)}")
    print(f"{kind} ({M}, {N}, {K}): worst masked shares {[round(v, 3) for v in shares]}")
    assert (_lg(worst), _lg(worst_e)) == RECORDED[f"{kind}-{M}x{N}x{K}"]
    assert [round(v, 3) for v in shares] == RECORDED_SHARES[f"{kind}-{M}x{N}x{K}"]
    assert math.ceil(math.log2(worst)) <= ne.NEED_LOG2


def test_tau_is_sixteen_times_the_worst_need():
    worst = max(v[0] for v in RECORDED.values())
    assert math.ceil(worst) == ne.NEED_LOG2 and ne.TAU_LOG2 == ne.NEED_LOG2 + 4 and ne.TAU == 2.0 ** ne.TAU_LOG2


# log2 of the plain-norm mirror's worst need per width (None: it differs nowhere)
RECORDED_PLAIN = {8: None, 256: -24.16, 520: -32.6, 768: -25.73, 1600: -25.6, 4096: -25.0, 8192: -24.18}


def test_plain_mirror_need_tau_and_masked_shares():
    """The plain norm's fp32 mirror (two-pass statistics, ``(x - mean) rstd gamma + beta``) against
    bf16(y64) at every width of the GPU test, LayerNorm with and without beta and RMSNorm: its need,
    ``TAU_PLAIN`` = 16 x the worst rounded up to a power of two, and at that band the caps of the GEMM
    forms for every width and variant: 5 % overall, 10 % in an ordinary row (at N = 8 one element of the
    eight), 50 % in a large-mean or zero row, 25 % in a column, no row or column fully masked."""
    cls = ne.row_classes(ne.PLAIN_ROWS)
    worst = 0.0
    for N in ne.PLAIN_WIDTHS:
        at_n = 0.0
        for variant in ("ln_beta", "ln", "rms"):
            x, gamma, beta, y64, S = ne.plain_case(N, variant)
            got = ne.mirror_plain(x, gamma.float(), None if beta is None else beta.float(), variant == "rms")
            need = ne.need_of(got, y64, S)
            masked = ne.boundary_distance(y64) < ne.TAU_PLAIN * S
            assert not bool(((got != ne.want_bf16(y64)) & ~masked).any())
            share = masked.double()
            rows = share.mean(1)
            ordinary = max(rows[m].item() for m in range(len(cls)) if cls[m] not in "cf")
            special = max(rows[m].item() for m in range(len(cls)) if cls[m] in "cf")
            print(f"plain N={N} {variant}: need 2^{_lg(need)}; masked {share.mean().item():.4f} all, {ordinary:.3f} worst "
                  f"ordinary row, {special:.3f} worst large-mean / zero row, {share.mean(0).max().item():.3f} worst column")
            assert share.mean().item() <= ne.CAPS["all"]
            assert ordinary <= max(ne.CAPS["row"], 1.0 / N) and special <= ne.CAPS["row_cf"]
            assert share.mean(0).max().item() <= ne.CAPS["col"]
            assert not bool(masked.all(1).any()) and not bool(masked.all(0).any())
            at_n = max(at_n, need)
        assert _lg(at_n) == RECORDED_PLAIN[N]
        worst = max(worst, at_n)
    assert math.ceil(math.log2(worst)) == ne.NEED_PLAIN_LOG2 and ne.TAU_PLAIN == 2.0 ** (ne.NEED_PLAIN_LOG2 + 4)


def test_rowstat_tolerance_is_sixteen_times_the_mirror_error():
    """``ROWSTAT_TOL_LOG2``: per width, 16 x the two-pass mirror's worst relative error in {rstd,
    -mean rstd} on the rows the GPU test uses, rounded up to a power of two."""
    for N in ne.PLAIN_WIDTHS:
        x = ne.activations(N)[:ne.PLAIN_ROWS]
        got = tuple(math.ceil(math.log2(16 * ne.rowstat_mirror_error(x, rms))) for rms in (False, True))
        print(f"row statistics N={N}: tolerance 2^{got[0]} (LayerNorm), 2^{got[1]} (RMSNorm)")
        assert got == ne.ROWSTAT_TOL_LOG2.get(N), (N, got)


def _shows(fx, got, form, rms=False):
    """(rows, columns) in which ``got`` differs from bf16(y64) outside the band."""
    t = ne.terms(fx, rms, form=form)
    bad = (got != ne.want_bf16(ne.truth_of(t))) & ~ne.mask_of(t, ne.TAU)
    return set(bad.any(1).nonzero().flatten().tolist()), set(bad.any(0).nonzero().flatten().tolist())


@pytest.mark.parametrize("fxs", FIXTURES[:2], ids=IDS[:2])
def test_sensitivity(fxs):
    """Each fault, injected into a mirror, produces mismatches outside the band, in exactly the rows or
    columns it touches (LayerNorm, bias + residual)."""
    kind, M, N, K = fxs
    fx = ne.fixture(kind, M, N, K)
    cls = ne.row_classes(M)
    f = ne.fold64(fx, False)
    for which in ne.MIRRORS:  # the clean mirrors show nowhere
        assert _shows(fx, ne.mirror(fx, which, False), which) == (set(), set())

    # 1. one element dropped from the variance: every row whose last element carries variance, which is
    # every row but the constant ones (f) and those whose last element sits on the mean by chance
    live = {m for m in range(M) if cls[m] != "f"}
    for which, st in (("two_pass", ne.stats_two_pass(fx.x, False, drop_last=True)),
                      ("one_pass", ne.stats_one_pass(fx.x, False, drop_last=True))):
        rows, _ = _shows(fx, ne.mirror(fx, which, False, stats=st), which)
        print(f"drop one element of {K} ({which}): shows in {len(rows)} of {M} rows")
        assert rows <= live and len(rows) >= 0.75 * len(live)
        assert {m for m in range(M) if cls[m] in "dg"} <= rows  # the last element is a spike / one of 8 live ones

    # 2, 3, 4, 6 under the two_pass S and under the wider S of the one_pass form (``condition``)
    cs = ne._f32(f.colsum)
    wb = f.bias - fx.bias.double()
    for which, good in (("two_pass", ne.stats_two_pass(fx.x, False)), ("one_pass", ne.stats_one_pass(fx.x, False))):
        # 2. the neighbour row's statistics, once per class: that row only
        for r in range(8, 16):
            st = (good[0].clone(), good[1].clone())
            st[0][r], st[1][r] = good[0][r + 1], good[1][r + 1]
            rows, cols = _shows(fx, ne.mirror(fx, which, False, stats=st), which)
            assert rows == {r}, (which, r, cls[r], rows)
        # 3. one column reading the next column's colsum: that column only
        for n0 in (0, 17, N - 2):
            assert cs[n0] != cs[n0 + 1]
            c2 = cs.clone()
            c2[n0] = cs[n0 + 1]
            rows, cols = _shows(fx, ne.mirror(fx, which, False, colsum=c2), which)
            assert cols == {n0} and len(rows) >= M // 4, (which, n0, cols, len(rows))
        # 4. beta omitted from the folded bias: every column whose W beta is not zero, and no other
        rows, cols = _shows(fx, ne.mirror(fx, which, False, fbias=ne._f32(fx.bias.double())), which)
        print(f"beta omitted ({which}): shows in {len(cols)} columns; W beta != 0 in {int((wb != 0).sum())} of {N}")
        assert cols == set((wb != 0).nonzero().flatten().tolist()) and len(cols) >= 0.9 * N
        # 6. rowstat[M - 1] used for the row before it: that row only
        st = (good[0].clone(), good[1].clone())
        st[0][M - 2], st[1][M - 2] = good[0][M - 1], good[1][M - 1]
        rows, _ = _shows(fx, ne.mirror(fx, which, False, stats=st), which)
        assert rows == {M - 2}, (which, rows)
    print("neighbour row's statistics, rowstat[M - 1] for row M - 2: exactly that row; colsum shifted by one column: "
          "exactly that column; under both forms of S")

    # 5. the unshifted E[x^2] - mean^2 in fp32: the large-mean rows (c), and only they.  The sums are whole
    # numbers below 2^24, so the fault's whole error is two or three roundings of 2^-24 mean^2 against a
    # variance of mean^2 / 3000: it is of either sign and now and then near zero, so most c rows, not all
    rows, _ = _shows(fx, ne.mirror(fx, "two_pass", False, stats=ne.stats_two_pass(fx.x, False, unshifted=True)), "two_pass")
    crow = {m for m in range(M) if cls[m] == "c"}
    print(f"unshifted variance: shows in {len(rows)} rows, {len(rows & crow)} of them the {len(crow)} of class (c)")
    assert rows <= crow and len(rows) >= len(crow) // 2 + 1

    # 7. one stale tile partial (a tile holding its neighbour tile's {mean, M2}): that row only
    p = ne.partials32(fx.x)
    for r, tile in ((8, 3), (9, K // 16 - 1), (11, 0), (15, 7)):
        assert not torch.equal(p[r, tile], p[r, tile - 1])
        p2 = p.clone()
        p2[r, tile] = p[r, tile - 1]
        rows, _ = _shows(fx, ne.mirror(fx, "partials", False, stats=ne.stats_partials(p2, K, False)), "partials")
        assert rows == {r}, (r, tile, rows)
    print("one stale tile partial: shows in exactly that row")


def test_stats64_partials_merge_to_the_row_statistics():
    """``stats64``'s per-16-column {mean, M2} partials merge (Chan's formula, in fp64) to its own mean
    and variance, including a last tile of 8 columns (K = 520)."""
    x = ne.activations(768)[:16, :520].double()
    st = ne.stats_of(x)
    n = torch.full((33,), 16.0, dtype=torch.float64)
    n[-1] = 8
    mean = (st.partials[..., 0] * n).sum(1) / 520
    m2 = st.partials[..., 1].sum(1) + (n * (st.partials[..., 0] - mean[:, None]) ** 2).sum(1)
    assert torch.allclose(mean, st.mean, rtol=0, atol=1e-12) and torch.allclose(m2 / 520, st.var, rtol=1e-12, atol=1e-12)
    assert torch.allclose(st.rowstat[:, 1], -st.mean * st.rstd)
