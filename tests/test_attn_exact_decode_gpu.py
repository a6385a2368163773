"""Every decode-attention route held to the selector fixtures of tests/attn_exact.py
(MI355X only): the batched split-K kernel (DPP scores at MHA, MFMA scores at
GQA; head-major q, fused QKV rows, fused + RoPE; bf16 and e4m3 caches), the
one-pass kernel (MFMA scores at GQA, row-layout scores at MHA) with forced
split counts, both combine kernels, and the non-temporal instantiations.

Each (sequence, head) selects a hand-placed set of 1, 2, 4, 8 or 16 keys: key
0, key len - 1 (the new key of a fused step), both sides of every split
boundary s * ceil(len / NS), of a 16-key MFMA tile edge and of a batch of rows
in flight.  The expected output is the fp64 softmax rounded once to bf16 and
the comparison is ``torch.equal``: a split that drops or doubles its boundary
key, a tile tail taken from the clamped row, a stale cache row scored instead
of the register copy of the new key, or a combine that misses a split changes
the output of a known (sequence, head).

Cache rows at or past the length, and the stale row a fused step overwrites,
hold poison (K: twice the selected score; V: NaN).  ``ws`` is NaN-filled and
sized for exactly the splits of the call; outputs and caches sit between NaN
sentinel slabs; caches are compared before and after as integers, so only the
new row may change, to exactly the expected bits.

Rows in flight per batch (``GPB * DEC_U`` of attn_decode_kernel): bf16 256 keys
at hd 64 and 128 at hd 128 (DPP scores), 256 (MFMA scores: 4 waves x 4 tiles);
e4m3 640 at hd 64 and 320 at hd 128.  The one-pass kernel holds a whole split
of up to 640 keys.

Found by this file: every fused route (batched and one-pass, bf16 and e4m3)
loads the value rows of a batch past the context from the clamped row len - 1,
which in a fused step is the stale cache row pos[b], and used to multiply them
by a probability of 0: NaN or Inf left in that row by an earlier occupant of
the cache slot reached the whole output (every fused case here whose context
did not fill its last batch of rows).  Those rows now take the register copy of
the new value, so NaN poison passes on every route and none needs finite poison.
"""
import pytest
import torch

import attn_exact as ax

pytestmark = pytest.mark.gpu
DEV = "cuda"

SPLITS = [1, 2, 3, 4, 5, 8, 9]  # combine: none, fast<2>, fast<4> (3, 4), fast<8> (5, 8), the loop kernel (9)
FMS = [(False, False), (True, False), (True, True)]  # FM 0, 1, 2: (fused, rope)


def _run(fx, kv8=False, ws_splits=None, who=""):
    """One launch of the route the environment selects; asserts output, sentinels and caches; returns ws."""
    from distributed_neural_networks_amd.ops import transformer_ops as T
    B, H, Hkv, hd, G = fx.B, fx.H, fx.Hkv, fx.hd, fx.G
    ns = ws_splits or fx.splits
    kb, kc = ax.guarded(ax.to_cache(fx.k0, kv8), DEV)
    vb, vc = ax.guarded(ax.to_cache(fx.v0, kv8), DEV)
    wb, ws = ax.nan_like((B * Hkv * ns, G * (hd + 2)), torch.float32, DEV)
    ws = ws.view(-1)
    ob, out = ax.nan_like((B, H * hd), torch.bfloat16, DEV)
    if fx.fused:
        pos = torch.tensor(fx.pos, device=DEV, dtype=torch.int32)
        cos, sin = (fx.cos.to(DEV), fx.sin.to(DEV)) if fx.rope else (None, None)
        T.attn_decode_qkv(fx.qkv.to(DEV), kc, vc, out, B, H, Hkv, hd, pos, ws, ns, cos, sin)
    else:
        lens = torch.tensor(fx.lens, device=DEV, dtype=torch.int32)
        T.attn_decode(fx.q.to(DEV), kc, vc, out, B, H, Hkv, hd, lens, ws, ns)
    torch.cuda.synchronize()
    assert ax.guards_intact(ob) and ax.guards_intact(wb), f"{who}: wrote outside the output or the workspace"
    assert ax.guards_intact(kb) and ax.guards_intact(vb), f"{who}: wrote outside the cache"
    for got, want, name in ((kc, fx.k1, "K"), (vc, fx.v1, "V")):
        bad = (ax.bits(got).cpu() != ax.bits(ax.to_cache(want, kv8))).any(-1).nonzero()
        assert bad.numel() == 0, f"{who}: {name} cache rows (b, kvh, s) differ: {bad[:8].tolist()}"
    want = fx.out.to(DEV)
    if not torch.equal(out, want):
        bad = (out.view(B, H, hd) != want.view(B, H, hd)).any(-1).nonzero().tolist()
        lens = [fx.lens[b] for b, _ in bad[:8]]
        raise AssertionError(f"{who}: {len(bad)} of {B * H} (b, h) differ; first {bad[:8]}, lens {lens}")
    return ws, out


def _batched(monkeypatch):
    monkeypatch.setenv("DNN_DECODE_1P", "0")


def _lens(S, splits, batches, fused):
    """``decode_lens`` around every batch size of ``batches``; fused: as positions, plus pos = S."""
    ls = list(dict.fromkeys(n for bt in batches for n in ax.decode_lens(S, splits, bt)))
    return tuple([n - 1 for n in ls] + [S]) if fused else tuple(ls)


# ---------------------------------------------------------------------------------------------------------------
# the batched kernel, bf16 cache: every (hd, G) of the launch table x splits x FM
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("hd,G", [(64, 1), (64, 2), (64, 4), (64, 8), (128, 1), (128, 2), (128, 4), (128, 8)])
def test_batched_bf16(hd, G, splits, monkeypatch):
    S, Hkv = 300, 2
    batches = (256,) if hd == 64 else (128, 256)
    for fused, rope in FMS:
        lens = _lens(S, splits, batches, fused)
        fx = ax.decode(len(lens), G * Hkv, Hkv, hd, S, lens, splits, fused, rope, edges=(16,) + batches)
        _batched(monkeypatch)
        ws, _ = _run(fx, who=f"FM={int(fused) + int(rope)}")
        if splits > 1:
            assert not torch.isnan(ws).any(), "a split slot nobody wrote"


# ---------------------------------------------------------------------------------------------------------------
# the batched kernel, e4m3 cache: every line of the e4m3 launch table
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("hd", [64, 128])
def test_batched_e4m3_mha(hd, splits, monkeypatch):
    """MHA (10 rows in flight); FM 0 and 1 (the e4m3 MHA kernel has no RoPE)."""
    S, Hkv = (700, 2) if hd == 64 else (400, 2)
    batches = (512, 640) if hd == 64 else (256, 320)
    for fused in (False, True):
        lens = _lens(S, splits, batches, fused)
        fx = ax.decode(len(lens), Hkv, Hkv, hd, S, lens, splits, fused, False, edges=(16,) + batches)
        _batched(monkeypatch)
        _run(fx, kv8=True, who=f"FM={int(fused)}")


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("G", [2, 4])
def test_batched_e4m3_gqa(G, splits, monkeypatch):
    """GQA at hd 128 (MFMA key tiles), head-major, fused and fused + RoPE; the new row's e4m3 bytes are part of
    the cache comparison."""
    S, Hkv, hd = 300, 2, 128
    for fused, rope in FMS:
        lens = _lens(S, splits, (256,), fused)
        fx = ax.decode(len(lens), G * Hkv, Hkv, hd, S, lens, splits, fused, rope, edges=(16, 256))
        _batched(monkeypatch)
        _run(fx, kv8=True, who=f"FM={int(fused) + int(rope)}")


def test_e4m3_refuses_gqa_at_hd64():
    """The e4m3 cache has no GQA kernel at hd 64: the launcher says so instead of computing something else."""
    fx = ax.decode(2, 4, 2, 64, 40, (17, 40), 1)
    with pytest.raises(RuntimeError, match="attn_decode"):
        _run(fx, kv8=True)


# ---------------------------------------------------------------------------------------------------------------
# the one-pass kernel
# ---------------------------------------------------------------------------------------------------------------
def _one_pass(monkeypatch, ns=None):
    monkeypatch.setenv("DNN_DECODE_1P", "2")
    if ns is None:
        monkeypatch.delenv("DNN_DECODE_1P_NS", raising=False)
    else:
        monkeypatch.setenv("DNN_DECODE_1P_NS", str(ns))


def _1p_lens(S, fused):
    ls = [n for n in (1, 639, 640, 641, S) if n <= S]
    ls = list(dict.fromkeys(ls))
    return tuple([n - 1 for n in ls] + [S]) if fused else tuple(ls)


def _assert_one_pass_ran(fx, ws, ns, ws_splits):
    """The one-pass kernel fills ``ns`` split slots per kv head, packed; the batched kernel would fill all of them."""
    used = fx.B * fx.Hkv * ns * fx.G * (fx.hd + 2)
    assert not torch.isnan(ws[:used]).any() and ax.untouched(ws[used:]).all(), "not the one-pass kernel's workspace"


@pytest.mark.parametrize("S,force_ns", [(641, None), (1300, None), (600, 2), (600, 3)])
# explicit ids: the ids these three shapes have always had
@pytest.mark.parametrize("hd,G", [pytest.param(128, 4, id="128-4-None"), pytest.param(128, 2, id="128-2-None"),
                                  pytest.param(64, 1, id="64-1-1")])
def test_one_pass(hd, G, S, force_ns, monkeypatch):
    """The three shapes attn_decode_1p_launch takes (GQA: MFMA scores, K/V issued before q; MHA: row-layout
    scores, K/V after q), ns from the capacity (641 -> 2, 1300 -> 3) or forced, lengths around the 640-key split
    capacity, every FM."""
    Hkv = 2
    ns = force_ns or -(-S // 640)
    for fused, rope in FMS:
        lens = _1p_lens(S, fused)
        fx = ax.decode(len(lens), G * Hkv, Hkv, hd, S, lens, ns, fused, rope, edges=(16, 128, 320))
        _one_pass(monkeypatch, ns=force_ns)
        ws, _ = _run(fx, ws_splits=ns + 2, who=f"FM={int(fused) + int(rope)}")
        _assert_one_pass_ran(fx, ws, ns, ns + 2)


@pytest.mark.parametrize("hd,G", [(64, 2), (128, 1), (128, 8)])
def test_one_pass_refused_shape_falls_back(hd, G, monkeypatch):
    """A shape the one-pass launcher does not build goes to the batched kernel: every split slot of the call's
    workspace is written, and the output is still exact."""
    S, Hkv, splits = 641, 2, 4
    for fused, rope in FMS:
        lens = _1p_lens(S, fused)
        fx = ax.decode(len(lens), G * Hkv, Hkv, hd, S, lens, splits, fused, rope, edges=(16, 128))
        _one_pass(monkeypatch)
        ws, _ = _run(fx, who=f"FM={int(fused) + int(rope)}")
        assert not torch.isnan(ws).any()


def test_one_pass_without_workspace_falls_back(monkeypatch):
    """Two splits from the capacity but a one-split workspace: the launcher refuses, the batched kernel runs."""
    lens = _1p_lens(641, False)
    fx = ax.decode(len(lens), 2, 2, 64, 641, lens, 1, edges=(16, 256))
    _one_pass(monkeypatch)
    _run(fx)


# ---------------------------------------------------------------------------------------------------------------
# non-temporal instantiations: the smallest capacity past the 32 MB rule at B * Hkv = 16
# ---------------------------------------------------------------------------------------------------------------
def test_non_temporal_batched_bf16(monkeypatch):
    """G = 4 (MFMA scores) and G = 1 (DPP scores) at the same cache size, head-major and fused."""
    S, B, Hkv, hd, splits = 4097, 2, 8, 128, 3  # 16 * 4097 * 128 * 4 B > 32 MiB
    for G in (4, 1):
        for fused, rope in ((False, False), (True, True)):
            lens = (S - 1, 4000) if fused else (S, 4001)
            fx = ax.decode(B, G * Hkv, Hkv, hd, S, lens, splits, fused, rope, edges=(16, 256))
            _batched(monkeypatch)
            _run(fx, who=f"NT G={G} fused={fused}")


@pytest.mark.parametrize("G", [1, 2])
def test_non_temporal_batched_e4m3(G, monkeypatch):
    S, B, Hkv, hd, splits = 8193, 2, 8, 128, 5  # 16 * 8193 * 128 * 2 B > 32 MiB
    lens = (S - 1, 8000)
    fx = ax.decode(B, G * Hkv, Hkv, hd, S, lens, splits, True, G > 1, edges=(16, 256, 320))
    _batched(monkeypatch)
    _run(fx, kv8=True, who="NT e4m3")


@pytest.mark.parametrize("hd,G,S", [pytest.param(128, 4, 4097, id="128-4-None-4097"),  # ids: as test_one_pass
                                    pytest.param(64, 1, 8193, id="64-1-1-8193")])
def test_non_temporal_one_pass(hd, G, S, monkeypatch):
    """ns = 7 (fast combine) and 13 (the loop combine kernel) from the capacity; the key loads keep the default
    policy at G = 4 and are non-temporal, as the value loads, at G = 1."""
    B, Hkv = 2, 8
    ns = -(-S // 640)
    lens = (S - 1, S - 700)
    fx = ax.decode(B, G * Hkv, Hkv, hd, S, lens, ns, True, hd == 128, edges=(16, 128, 320))
    _one_pass(monkeypatch)
    ws, _ = _run(fx, ws_splits=ns + 1, who="NT 1p")
    _assert_one_pass_ran(fx, ws, ns, ns + 1)


# ---------------------------------------------------------------------------------------------------------------
# determinism: the densest case of each family, 20 launches into fresh NaN buffers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["batched_dpp", "batched_mfma", "e4m3_mha", "e4m3_gqa", "one_pass_mfma", "one_pass_rs"])
def test_repeated_launches_are_bit_identical(family, monkeypatch):
    kv8 = family.startswith("e4m3")
    ws_splits = None
    if family in ("batched_dpp", "batched_mfma"):
        H = 16 if family == "batched_mfma" else 2  # G = 8: MFMA scores; G = 1: DPP scores
        lens = _lens(300, 9, (128, 256), True)
        fx = ax.decode(len(lens), H, 2, 128, 300, lens, 9, True, True, edges=(16, 128, 256))
        _batched(monkeypatch)
    elif family == "e4m3_mha":
        lens = _lens(700, 9, (512, 640), True)
        fx = ax.decode(len(lens), 2, 2, 64, 700, lens, 9, True, False, edges=(16, 512, 640))
        _batched(monkeypatch)
    elif family == "e4m3_gqa":
        lens = _lens(300, 9, (256,), True)
        fx = ax.decode(len(lens), 8, 2, 128, 300, lens, 9, True, True, edges=(16, 256))
        _batched(monkeypatch)
    else:
        hd, G = (128, 4) if family == "one_pass_mfma" else (64, 1)  # GQA: MFMA scores; MHA: row-layout scores
        lens = _1p_lens(1300, True)
        fx = ax.decode(len(lens), G * 2, 2, hd, 1300, lens, 3, True, hd == 128, edges=(16, 128, 320))
        _one_pass(monkeypatch)
        ws_splits = 3
    first = None
    for i in range(20):
        _, out = _run(fx, kv8=kv8, ws_splits=ws_splits, who=f"{family} launch {i}")
        first = out.clone() if first is None else first
        assert torch.equal(out, first), i
