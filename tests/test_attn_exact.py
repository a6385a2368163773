"""The selector fixtures of tests/attn_exact.py, checked on the CPU: operands exact
in bf16 and e4m3, scores of three values with a gap that flushes to 0 in fp32,
selected counts powers of two, the fp64 result a bf16 number, the coverage the
constructions promise (diagonal and first-masked-key queries, two-block queries
per wave slab, split boundaries, tile edges), and fp32 emulations of the
kernels' summation (64-key online softmax walked forwards and backwards, split
and combine) equal to the expected tensor bit for bit.

Shares of the queries that select their own position / whose code is that of
the first masked key, over the 40 prefill fixtures with T > 1 (the floor is one
tenth, and 8 queries): 0.115 .. 0.518 / 0.110 .. 0.390; the lowest are the G = 4
groups, where one head in four can take either role at a position.
"""
import math

import pytest
import torch

import attn_exact as ax

PF = [(c, h, hd) for c in ax.PREFILL_CASES for h in ax.PREFILL_HEADS for hd in (64, 128)]
PF_IDS = [f"{ax.prefill_id(c)}-H{h[0]}kv{h[1]}-hd{hd}" for c, h, hd in PF]
# the emulations: the shapes (T, pos0) = (193, 0), (130, 63), (129, 64), (300, 250) at both head dims, MHA and G = 4
EMU = [(c, h, hd) for c in ax.PREFILL_CASES[2:] for h in ((4, 4), (8, 2)) for hd in (64, 128)]


def _pf(case, heads, hd):
    B, T, pos, S = case
    return ax.prefill(B, T, heads[0], heads[1], hd, pos, S)


def _bf16_number(x64):
    return (x64 - x64.to(torch.bfloat16).double()).abs().max().item()


@pytest.mark.parametrize("hd", [64, 128])
def test_hadamard_codes_and_score_gap(hd):
    had = ax.hadamard(hd)
    assert torch.equal(had @ had.T, hd * torch.eye(hd))
    k = ax.code_vec(torch.arange(hd), hd)
    for t in (torch.bfloat16, ax.F8):
        assert torch.equal(k.to(t).float(), k) and torch.equal((2 * k).to(t).float(), 2 * k)
    v = torch.arange(-ax.VMAX, ax.VMAX + 1).float()
    assert torch.equal(v.to(torch.bfloat16).float(), v) and torch.equal(v.to(ax.F8).float(), v)
    gap = 16 * hd / math.sqrt(hd) * ax.LOG2E  # selected minus non-selected, in exp2 units
    assert gap >= 184
    assert torch.exp2(torch.tensor(-gap, dtype=torch.float32)).item() == 0.0
    # a block's weight-1 sum before its first selected key is exact in fp32
    assert 2048 * ax.VMAX < 2**24


def test_rope_tables_are_exact_signed_permutations():
    S, hd = 300, 128
    cos, sin = ax.rope_tables(S, hd)
    assert set(cos.unique().tolist()) <= {-1.0, 0.0, 1.0} and torch.equal(cos.abs() + sin.abs(), torch.ones(S, hd // 2))
    assert torch.unique(torch.cat([cos, sin], 1), dim=0).shape[0] == S, "every table row differs"
    assert torch.unique(torch.cat([cos, sin], 0), dim=1).shape[1] == hd // 2, "every table column differs"
    x = ax.code_vec(torch.randint(0, hd, (S,), generator=torch.Generator().manual_seed(0)), hd)
    y = ax.rope_inv(x, cos, sin)
    assert torch.equal(ax.rope(y, cos, sin), x) and torch.equal(y.abs(), torch.full_like(y, 4.0))
    # a wrong table row breaks the orthogonality: the rotated vector is no longer its own code
    wrong = ax.rope(y[:-1], cos[1:], sin[1:])
    dots = (wrong * x[:-1]).sum(-1)
    assert (dots != 16 * hd).all()


@pytest.mark.parametrize("case,heads,hd", PF, ids=PF_IDS)
def test_prefill_fixture_preconditions(case, heads, hd):
    fx = _pf(case, heads, hd)
    B, T, H, G, S = fx.B, fx.T, fx.H, fx.G, fx.S
    assert _bf16_number(fx.out64) < 1e-12
    x = fx.qkv.float().view(B, T, H + 2 * fx.Hkv, hd)
    assert torch.equal(x.to(ax.F8).float(), x)
    own = nxt = total = 0
    for b in range(B):
        L = fx.pos[b] + T
        for h in range(H):
            kc = fx.kcode[b][h // G]
            two_blocks = torch.zeros(T, dtype=torch.bool)
            for t in range(T):
                p = fx.pos[b] + t
                sel = fx.selected(b, h, t)
                assert sel.numel() in ax.OK_COUNTS, (b, h, t)
                own += int(kc[p] == fx.qcode[b, h, t])
                nxt += int(p + 1 < L and kc[p + 1] == fx.qcode[b, h, t])
                total += 1
                two_blocks[t] = (sel >> 6).unique().numel() >= 2
            for t0 in range(0, T, 32):  # every 32-row wave slab that can see two 64-key blocks has such a query
                if fx.pos[b] + min(t0 + 31, T - 1) >= 64 + 1:
                    assert two_blocks[t0:t0 + 32].any(), (b, h, t0)
        for kvh in range(fx.Hkv):  # heads of one kv group take different codes (once the keys carry G codes)
            q = fx.qcode[b, kvh * G:(kvh + 1) * G]
            assert all(q[:, t].unique().numel() == G for t in range(T) if fx.pos[b] + t >= 32)
    if T == 1:  # a single key: every query selects it, and there is no key p + 1
        assert own == total
    else:
        assert own >= max(8, total / 10) and nxt >= max(8, total / 10), (own, nxt, total)
    # poison from pos[b] on, written rows as the chunk gives them, nothing else moved
    for b in range(B):
        p0, n = fx.pos[b], min(fx.pos[b] + T, S) - fx.pos[b]
        assert torch.isnan(fx.v0[b, :, p0:]).all() and (fx.k0[b, :, p0:].abs() == 8).all()
        assert torch.equal(fx.k1[b, :, :p0], fx.k0[b, :, :p0]) and torch.equal(fx.k1[b, :, p0 + n:], fx.k0[b, :, p0 + n:])
        assert (fx.k1[b, :, p0:p0 + n].abs() == 4).all() and not torch.isnan(fx.v1[b, :, :p0 + n]).any()
        assert torch.isnan(fx.v1[b, :, p0 + n:]).all()
    assert fx.rows.sum().item() == sum(min(p + T, S) - p for p in fx.pos)


@pytest.mark.parametrize("case,heads,hd", EMU, ids=[f"{ax.prefill_id(c)}-H{h[0]}kv{h[1]}-hd{hd}" for c, h, hd in EMU])
def test_prefill_online_softmax_emulation_is_bitwise(case, heads, hd):
    """fp32, 64-key blocks, forwards and backwards: the bf16-rounded fp64 reference bit for bit."""
    fx = _pf(case, heads, hd)
    had = ax.hadamard(hd)
    want = fx.out.view(fx.B, fx.T, fx.H, hd)
    for b in range(fx.B):
        qpos = fx.pos[b] + torch.arange(fx.T)
        for h in range(0, fx.H, max(1, fx.H // 2)):
            k = 4.0 * had[fx.kcode[b][h // fx.G]]
            v = fx.vals[b][h // fx.G]
            q = 4.0 * had[fx.qcode[b, h]]
            for order in (1, -1):
                got = ax.emulate_online(q, k, v, qpos, order)
                assert torch.equal(got, want[b, :, h]), (b, h, order)


DEC = [(64, 1, 1), (64, 1, 3), (64, 4, 4), (64, 8, 9), (128, 1, 2), (128, 2, 5), (128, 4, 8), (128, 8, 9)]


@pytest.mark.parametrize("hd,G,splits", DEC)
@pytest.mark.parametrize("fused,rope", [(False, False), (True, False), (True, True)])
def test_decode_fixture_preconditions_and_split_emulation(hd, G, splits, fused, rope):
    S, Hkv = 300, 2
    batch = 256 if hd == 64 else 128
    lens = ax.decode_lens(S, splits, batch, fused)
    fx = ax.decode(len(lens), G * Hkv, Hkv, hd, S, lens, splits, fused, rope, edges=(16, batch))
    had = ax.hadamard(hd)
    assert _bf16_number(fx.out64) < 1e-12
    covered = set()
    for b in range(fx.B):
        n = fx.lens[b]
        for kvh in range(Hkv):
            kc = fx.kcode[b][kvh]
            seen = []
            for h in range(kvh * G, (kvh + 1) * G):
                sel = (kc == fx.qcode[b, h]).nonzero().flatten().tolist()
                assert sel == fx.sel[b][h] and len(sel) in ax.OK_COUNTS
                seen += sel if h - kvh * G < min(G, n) else []
            assert len(seen) == len(set(seen))
            assert 0 in seen and n - 1 in seen
            covered |= {(b, x) for e in ax.boundaries(n, splits) + [16, batch] for x in (e - 1, e)
                        if e < n and x in seen}
            assert fx.qcode[b, kvh * G:(kvh + 1) * G].unique().numel() == min(G, n)
        assert torch.isnan(fx.v0[b, :, n:]).all() and (fx.k0[b, :, n:].abs() == 8).all()
        for h in range(fx.H):
            k, v = 4.0 * had[fx.kcode[b][h // G]], fx.vals[b][h // G]
            got = ax.emulate_split(4.0 * had[fx.qcode[b, h]], k, v, splits)
            assert torch.equal(got, fx.out[b].view(fx.H, hd)[h]), (b, h)
    # both sides of every split boundary, of the tile edge and of the batch edge are selected somewhere in the case
    for b in range(fx.B):
        n = fx.lens[b]
        if n >= 64 and G * 16 >= 2 + 2 * (len(ax.boundaries(n, splits)) + 2):  # neither the 16-key cap nor a dry pool bit
            for e in ax.boundaries(n, splits) + [16, batch]:
                if e < n:
                    assert (b, e - 1) in covered and (b, e) in covered, (b, e)
    if fused:
        for b, p in enumerate(fx.pos):
            x = fx.qkv[b].float()
            assert torch.isnan(x[(fx.H + 2 * Hkv) * hd:]).all()
            if p < S:  # the stale row is poison before the step and the new row after it
                assert (fx.k0[b, :, p].abs() == 8).all() and torch.isnan(fx.v0[b, :, p]).all()
                assert (fx.k1[b, :, p].abs() == 4).all() and not torch.isnan(fx.v1[b, :, p]).any()
                kn = x[fx.H * hd:(fx.H + Hkv) * hd].view(Hkv, hd)
                if rope:
                    kn = ax.rope(kn, fx.cos[p], fx.sin[p])
                assert torch.equal(kn, fx.k1[b, :, p])
            else:
                assert torch.equal(fx.k1[b], fx.k0[b])
            assert torch.equal(fx.k1[b, :, :min(p, S)], fx.k0[b, :, :min(p, S)])
