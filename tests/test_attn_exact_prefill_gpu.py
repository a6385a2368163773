"""qkv_split and the flash-attention prefill routes held to the selector fixtures of
tests/attn_exact.py (MI355X only).

Every softmax weight of these fixtures is exactly 0 or 1/n, so the fp64
attention rounded once to bf16 is the expected output of every route and block
order: the comparison is ``torch.equal`` and a difference
names the query.  One key too many or too few (a causal mask off by one, a
tile tail taken from a clamped row, a cache row past the length) changes the
selected set of some query: in every fixture a share of the queries select
their own position, and a share would match the first masked key.

Cache rows from ``pos[b]`` on hold poison before the launch (K: twice the
selected score; V: NaN), caches and outputs sit between NaN sentinel slabs, and
caches are compared before and after as integers: only the chunk's rows may
change, to exactly the chunk's rows.

Routes: ``qkv_split`` + ``flash_attn`` and ``flash_attn_qkv``, on the bf16 and
the e4m3 cache, at both head dims.  In the
case with S = pos + T - 1 the overflow row is dropped and the clipped query is
excluded, as in test_flash_attn_qkv_matches_split.

Found by this file: in that case ``flash_attn`` clamped the tail of its last key
tile to row kv_len - 1 = S, the first row of the next head's cache or, for the
last head, whatever follows the allocation.  The masked key's probability is 0,
but 0 x NaN from that row reached every query of the tile (43 of 2392 queries
per kv head of the last sequence here).  The tail is now clamped to the cache.
"""
import pytest
import torch

import attn_exact as ax

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(c, h, hd) for c in ax.PREFILL_CASES for h in ax.PREFILL_HEADS for hd in (64, 128)]
IDS = [f"{ax.prefill_id(c)}-H{h[0]}kv{h[1]}-hd{hd}" for c, h, hd in CASES]


def _fx(case, heads, hd):
    B, T, pos, S = case
    return ax.prefill(B, T, heads[0], heads[1], hd, pos, S)


def _caches(fx, kv8):
    kb, kc = ax.guarded(ax.to_cache(fx.k0, kv8), DEV)
    vb, vc = ax.guarded(ax.to_cache(fx.v0, kv8), DEV)
    return kb, kc, vb, vc


def _assert_cache(fx, kv8, kb, kc, vb, vc, written, who):
    want_k, want_v = (fx.k1, fx.v1) if written else (fx.k0, fx.v0)
    assert ax.guards_intact(kb) and ax.guards_intact(vb), f"{who}: wrote outside the cache"
    for got, want, name in ((kc, want_k, "K"), (vc, want_v, "V")):
        bad = (ax.bits(got).cpu() != ax.bits(ax.to_cache(want, kv8))).any(-1).nonzero()
        assert bad.numel() == 0, f"{who}: {name} cache rows (b, kvh, s) differ: {bad[:8].tolist()}"


def _assert_out(fx, ob, out, who):
    assert ax.guards_intact(ob), f"{who}: wrote outside the output"
    rows = fx.rows.to(DEV)
    got, want = out[rows], fx.out.to(DEV)[rows]
    if not torch.equal(got, want):
        bad = (got.view(-1, fx.H, fx.hd) != want.view(-1, fx.H, fx.hd)).any(-1).nonzero()
        idx = rows.nonzero().flatten()[bad[:, 0]]
        first = [(int(i) // fx.T, int(h), int(i) % fx.T) for i, h in zip(idx[:8], bad[:8, 1])]
        raise AssertionError(f"{who}: {bad.shape[0]} of {got.shape[0] * fx.H} queries differ; first (b, h, t): {first}")


def _split_q(fx, qkv, kc, vc, pos, cos=None, sin=None):
    """qkv_split into a NaN-filled q: the buffer, and q as (B, H, T, hd)."""
    from distributed_neural_networks_amd.ops import transformer_ops as T
    qb, q = ax.nan_like((fx.B, fx.H, fx.T, fx.hd), torch.bfloat16, DEV)
    T.qkv_split(qkv, q, kc, vc, fx.B, fx.T, fx.H, fx.Hkv, fx.hd, pos, cos, sin)
    return qb, q


def _assert_q(fx, qb, q, who):
    assert ax.guards_intact(qb), f"{who}: wrote outside q"
    want = fx.qkv.view(fx.B, fx.T, fx.H + 2 * fx.Hkv, fx.hd)[:, :, :fx.H].transpose(1, 2).to(DEV)
    keep = fx.rows.view(fx.B, 1, fx.T).expand(fx.B, fx.H, fx.T).to(DEV)
    assert torch.equal(q[keep], want[keep]), f"{who}: q"


@pytest.mark.parametrize("case,heads,hd", CASES, ids=IDS)
def test_flash_routes_select_exactly(case, heads, hd):
    from distributed_neural_networks_amd.ops import transformer_ops as T
    fx = _fx(case, heads, hd)
    B, Tn, H, Hkv = fx.B, fx.T, fx.H, fx.Hkv
    qkv = fx.qkv.to(DEV)
    pos = torch.tensor(fx.pos, device=DEV, dtype=torch.int32)
    for kv8 in (False, True):
        who = "e4m3" if kv8 else "bf16"
        # qkv_split, then flash_attn over the cache
        kb, kc, vb, vc = _caches(fx, kv8)
        qb, q = _split_q(fx, qkv, kc, vc, pos)
        ob, out = ax.nan_like((B * Tn, H * hd), torch.bfloat16, DEV)
        T.flash_attn(q, kc, vc, out, B, Tn, H, Hkv, hd, pos)
        torch.cuda.synchronize()
        _assert_q(fx, qb, q, "qkv_split " + who)
        _assert_cache(fx, kv8, kb, kc, vb, vc, True, "qkv_split + flash_attn " + who)
        _assert_out(fx, ob, out, "flash_attn " + who)
        # flash_attn_qkv: the chunk's keys from the qkv rows, the cache written on the way
        kb, kc, vb, vc = _caches(fx, kv8)
        ob, out = ax.nan_like((B * Tn, H * hd), torch.bfloat16, DEV)
        T.flash_attn_qkv(qkv, kc, vc, out, B, Tn, H, Hkv, hd, pos)
        torch.cuda.synchronize()
        _assert_cache(fx, kv8, kb, kc, vb, vc, True, "flash_attn_qkv " + who)
        _assert_out(fx, ob, out, "flash_attn_qkv " + who)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("case,heads,hd", [(ax.PREFILL_CASES[3], (4, 2), 64), (ax.PREFILL_CASES[3], (8, 2), 128),
                                           (ax.PREFILL_CASES[5], (4, 4), 128), (ax.PREFILL_CASES[0], (4, 1), 64)],
                         ids=["T130-G2-hd64", "T130-G4-hd128", "T300-clipped-hd128", "T1-hd64"])
def test_qkv_split_alone(case, heads, hd, rope, kv8):
    """q and the written cache rows bit for bit, every other cache row untouched (poison and guards included); with
    the quarter-turn tables the stored rows are inverse-rotated, so a wrong table row (or a rotated V) shows."""
    fx = _fx(case, heads, hd)
    cos = sin = None
    qkv = fx.qkv
    if rope:
        cos, sin = ax.rope_tables(fx.S, hd)
        qkv = ax.prefill_rope_rows(fx, cos, sin)
        assert not torch.equal(qkv, fx.qkv)
        cos, sin = cos.to(DEV), sin.to(DEV)
    pos = torch.tensor(fx.pos, device=DEV, dtype=torch.int32)
    kb, kc, vb, vc = _caches(fx, kv8)
    qb, q = _split_q(fx, qkv.to(DEV), kc, vc, pos, cos, sin)
    torch.cuda.synchronize()
    _assert_q(fx, qb, q, "qkv_split")
    _assert_cache(fx, kv8, kb, kc, vb, vc, True, "qkv_split")
