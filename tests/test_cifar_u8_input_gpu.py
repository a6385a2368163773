"""uint8 image input of the fp32 CIFAR stage 0 on the device, bit for bit.

The kernel's uint8 arm looks every byte up in a packed table whose entries are the hi/lo halves
the fp32 arm's split would produce for the normalised float, so its LDS planes, and with them
its output, are bitwise those of the fp32 arm fed ``normalize_u8(x, table)``.  Two criteria, both
on int32 bit patterns with no tolerance: equality with the fp32 arm (random weights and bytes,
both boundaries, every conv2 variant), and equality with the fp64 reference on the exact uint8
fixtures (tests/cifar_u8_exact.py), which does not lean on the fp32 arm being right.

Shapes are those of test_cifar_stage0_exact_gpu.py: one image (prologue and drain only), two
images in one workgroup (both double-buffer parities), 4 + 3 images in two workgroups, 257
images on the default grid.  Guards: the batch is the middle of a byte buffer whose other bytes
are 255 with table[:, 255] = NaN, and of a sentinel-filled output.  Race screen: 20 launches.
Two tables in one process: nothing is cached across launches.  Rejections raise before a launch.
"""
import functools

import pytest
import torch

import cifar_exact as ce
import cifar_u8_exact as cu

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(1, 0), (2, 1), (7, 2), (257, 0)]  # (B, grid); grid 0 = the default, one workgroup per CU
CONV2 = {"16x16x32": ("16x16x32", 1), "32x32x16": ("32x32x16", 1), "32x32x16-store8": ("32x32x16", 0)}
BOUNDARIES = ("fp32", "split")
CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)
MARGIN = 64
SENTINEL = 0x7FC5A5A5  # int32 bits of a NaN with a payload that no arithmetic produces
B_MAX = 257


@pytest.fixture(params=list(CONV2))
def conv2(request):
    """Force one compiled conv2 consumer (MFMA shape and store width); restore both afterwards."""
    from distributed_neural_networks_amd.ops import cifar as cops
    shape, wide = CONV2[request.param]
    prev_mfma = cops.set_stage0_mfma(shape)
    prev_wide = cops.set_stage0_wide_store(wide)
    yield request.param
    cops.set_stage0_wide_store(prev_wide)
    cops.set_stage0_mfma(prev_mfma)


def _assert_bits(got, want, what):
    """got, want: int32 bit patterns of the same shape on the device."""
    if torch.equal(got, want):
        return
    g, w = got.cpu().reshape(got.shape[0], -1), want.cpu().reshape(want.shape[0], -1)
    bad = (g != w).nonzero()
    img, el = bad[0].tolist()
    gv, wv = g[img, el].view(torch.float32).item(), w[img, el].view(torch.float32).item()
    print(f"{what}: {bad.shape[0]} of {g.numel()} elements differ in {bad[:, 0].unique().numel()} images; first at "
          f"image {img} element {el}: got {gv!r} ({g[img, el].item() & 0xFFFFFFFF:#010x}), "
          f"expected {wv!r} ({w[img, el].item() & 0xFFFFFFFF:#010x})")
    pytest.fail(f"{what}: image {img} element {el}: got {gv!r}, expected {wv!r} ({bad.shape[0]} elements differ)")


def _tables():
    from distributed_neural_networks_amd.ops import cifar as cops
    return {"default": cops.make_input_table(), "cifar": cops.make_input_table(CIFAR_MEAN, CIFAR_STD)}


@functools.lru_cache(maxsize=None)
def _random_setup():
    """Once: random reference-layout weights (the draw of tools/make_checkpoint), 257 random byte
    images and, per table, the packed table and the normalised fp32 images on the device."""
    from distributed_neural_networks_amd.models import cifar
    from distributed_neural_networks_amd.ops import cifar as cops
    w0 = cops.pack_stage0(cifar.random_state_dict(3), DEV)
    u8 = torch.randint(0, 256, (B_MAX, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(17))
    per = {k: (cops.pack_input_table(t, DEV), cops.normalize_u8(u8, t).to(DEV)) for k, t in _tables().items()}
    return w0, u8.to(DEV), per


@pytest.mark.parametrize("B,grid", CASES)
@pytest.mark.parametrize("table", ["default", "cifar"])
def test_u8_is_bitwise_the_fp32_arm(table, conv2, B, grid):
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, u8, per = _random_setup()
    packed, xf = per[table]
    for boundary in BOUNDARIES:
        want = cops.stage0_forward(xf[:B], w0, grid=grid, boundary=boundary)
        got = cops.stage0_forward(u8[:B], w0, grid=grid, boundary=boundary, table=packed)
        torch.cuda.synchronize()
        assert got.shape == (B, 4096) and got.dtype == torch.float32
        _assert_bits(got.view(torch.int32), want.view(torch.int32),
                     f"table {table} conv2 {conv2} B {B} grid {grid} {boundary} boundary, uint8 vs fp32 arm")


@functools.lru_cache(maxsize=None)
def _golden(name):
    """Per uint8 fixture, once: packed weights and table, the 257 byte images and the expected
    boundary (int32 bits, fp32 and blocked hi/lo encoding) on the device."""
    from distributed_neural_networks_amd.ops import cifar as cops
    f = cu.u8_fixture(name)
    m1, m2 = ce.magnitude_bounds(f.fx)
    assert m1 < 2**16 and m2 < 2**22, (name, m1, m2)
    ref = cu.u8_reference(name)
    assert ref.unique(dim=0).shape[0] == ce.B_MAX
    w0 = cops.pack_stage0(f.fx.sd, DEV)
    refd = ref.to(DEV)
    encd = cops.encode_boundary(refd)
    torch.cuda.synchronize()
    return w0, f.u8.to(DEV), cops.pack_input_table(f.table, DEV), refd.view(torch.int32), encd.view(torch.int32), f.table


@pytest.mark.parametrize("B,grid", CASES)
@pytest.mark.parametrize("name", ce.NAMES)
def test_u8_is_bitwise_the_fp64_reference(name, B, grid):
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, u8, packed, ref, enc, _ = _golden(name)
    what = f"{name} B {B} grid {grid}"
    h = cops.stage0_forward(u8[:B], w0, grid=grid, table=packed)
    hs = cops.stage0_forward(u8[:B], w0, grid=grid, boundary="split", table=packed)
    torch.cuda.synchronize()
    _assert_bits(h.view(torch.int32), ref[:B], what + " fp32 boundary")
    _assert_bits(hs.view(torch.int32), enc[:B], what + " split boundary")


@functools.lru_cache(maxsize=None)
def _guarded_setup():
    """Bytes 0..254 only and table[:, 255] = NaN, so a byte read from outside the batch poisons
    the output: the byte images, the packed table and the normalised fp32 images on the device."""
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, _, _ = _random_setup()
    t = cops.make_input_table(CIFAR_MEAN, CIFAR_STD).clone()
    t[:, 255] = float("nan")
    u8 = torch.randint(0, 255, (B_MAX, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(23))
    assert int(u8.max()) == 254
    xf = cops.normalize_u8(u8, t)
    assert bool(torch.isfinite(xf).all())
    return w0, u8.to(DEV), cops.pack_input_table(t, DEV), xf.to(DEV)


@pytest.mark.parametrize("B,grid", CASES)
def test_u8_stays_inside_its_batch(conv2, B, grid):
    """Images [64 : 64 + B] of a byte buffer whose other bytes are 255 (NaN in the table), rows
    [64 : 64 + B] of a sentinel-filled output: the margins keep the sentinel and the result is
    still the expected one (the fp32 arm of the same conv2 variant on the normalised images)."""
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, u8, packed, xf = _guarded_setup()
    xin = torch.full((B + 2 * MARGIN, 32, 32, 3), 255, dtype=torch.uint8, device=DEV)
    xin[MARGIN:MARGIN + B] = u8[:B]
    for boundary in BOUNDARIES:
        what = f"conv2 {conv2} B {B} grid {grid} {boundary} boundary, guarded"
        expect = cops.stage0_forward(xf[:B], w0, grid=grid, boundary=boundary).view(torch.int32)
        buf = torch.full((B + 2 * MARGIN, 4096), SENTINEL, dtype=torch.int32, device=DEV)
        out = buf.view(torch.float32)[MARGIN:MARGIN + B]
        cops.stage0_forward(xin[MARGIN:MARGIN + B], w0, out=out, grid=grid, boundary=boundary, table=packed)
        torch.cuda.synchronize()
        if boundary == "fp32":
            assert not bool(torch.isnan(expect.view(torch.float32)).any())
        assert bool((buf[:MARGIN] == SENTINEL).all()), what + ": rows before the batch were written"
        assert bool((buf[MARGIN + B:] == SENTINEL).all()), what + ": rows past the batch were written"
        _assert_bits(buf[MARGIN:MARGIN + B], expect, what)


@pytest.mark.parametrize("B,grid", [(7, 2), (257, 0)])
@pytest.mark.parametrize("name", ce.NAMES)
def test_u8_repeated_launches(name, B, grid):
    """Race screen on the default arms: 20 launches into a buffer re-filled with the sentinel,
    every one bitwise the fp64 reference."""
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, u8, packed, ref, _, _ = _golden(name)
    buf = torch.empty((B, 4096), dtype=torch.int32, device=DEV)
    for i in range(20):
        buf.fill_(SENTINEL)
        cops.stage0_forward(u8[:B], w0, out=buf.view(torch.float32), grid=grid, table=packed)
        torch.cuda.synchronize()
        _assert_bits(buf, ref[:B], f"{name} B {B} grid {grid} launch {i}")


def test_two_tables_in_one_process():
    """Table A, then table B on other images, then table A again: each result is its own table's
    expected output, so no table is kept across launches."""
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, u8, per = _random_setup()
    (pa, xa), (pb, xb) = per["default"], per["cifar"]
    B = 7
    want_a = cops.stage0_forward(xa[:B], w0, grid=2).view(torch.int32)
    want_b = cops.stage0_forward(xb[100:100 + B], w0, grid=2).view(torch.int32)
    got_a1 = cops.stage0_forward(u8[:B], w0, grid=2, table=pa)
    got_b = cops.stage0_forward(u8[100:100 + B], w0, grid=2, table=pb)
    got_a2 = cops.stage0_forward(u8[:B], w0, grid=2, table=pa)
    torch.cuda.synchronize()
    assert not torch.equal(want_a, want_b)
    _assert_bits(got_a1.view(torch.int32), want_a, "table A, first launch")
    _assert_bits(got_b.view(torch.int32), want_b, "table B")
    _assert_bits(got_a2.view(torch.int32), want_a, "table A, after table B")


class _NoLaunch:
    """The library with the uint8 launch replaced by a counter: a rejection must come first."""

    def __init__(self, real):
        self._real, self.launches = real, 0

    def __getattr__(self, k):
        return getattr(self._real, k)

    def cifar_stage0_x3_u8(self, *a, **kw):
        self.launches += 1
        return 0


@pytest.fixture
def no_launch(monkeypatch):
    from distributed_neural_networks_amd.ops import cifar as cops
    spy = _NoLaunch(cops.lib())
    monkeypatch.setattr(cops, "lib", lambda: spy)
    return spy


def test_rejections_raise_before_any_launch(no_launch):
    from distributed_neural_networks_amd.models import cifar
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, u8, per = _random_setup()
    packed = per["default"][0]
    x = u8[:2]
    with pytest.raises(ValueError, match="fp32 precision"):
        cops.stage0_forward(x, cops.pack_stage0(cifar.random_state_dict(3), DEV, "bf16"), table=packed)
    with pytest.raises(ValueError, match="table"):
        cops.stage0_forward(x, w0)
    with pytest.raises(ValueError, match="NHWC"):
        cops.stage0_forward(x.permute(0, 3, 1, 2).contiguous(), w0, table=packed)
    flat = torch.zeros(2 * 3072 + 4, dtype=torch.uint8, device=DEV)
    off1 = flat[1:1 + 2 * 3072].view(2, 32, 32, 3)
    assert off1.is_contiguous() and off1.data_ptr() % 4 == 1
    with pytest.raises(ValueError, match="aligned"):
        cops.stage0_forward(off1, w0, table=packed)
    prev = cops.set_stage0_conv1("k48")
    try:
        with pytest.raises(ValueError, match="k48"):
            cops.stage0_forward(x, w0, table=packed)
    finally:
        cops.set_stage0_conv1(prev)
    assert no_launch.launches == 0
    cops.stage0_forward(x, w0, table=packed)  # the spy does see an accepted call
    assert no_launch.launches == 1


def test_library_rejects_k48_and_misalignment():
    """The C entry point's own rejection codes (negative, nothing launched)."""
    from distributed_neural_networks_amd.ops import cifar as cops
    from distributed_neural_networks_amd.ops._lib import lib, ptr, stream_ptr
    w0, u8, per = _random_setup()
    packed = per["default"][0]
    out = torch.full((2, 4096), SENTINEL, dtype=torch.int32, device=DEV)

    def call(xp):
        return lib().cifar_stage0_x3_u8(xp, ptr(packed), ptr(out), ptr(w0.w1h32), ptr(w0.w1l32), ptr(w0.b1),
                                        ptr(w0.w2h), ptr(w0.w2l), ptr(w0.b2), 2, 0, stream_ptr(), 0)
    assert call(ptr(u8) + 1) == -3
    prev = cops.set_stage0_conv1("k48")
    try:
        assert call(ptr(u8)) == -2
    finally:
        cops.set_stage0_conv1(prev)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_pipeline_uint8_equals_default_pipeline():
    """Two CifarHipStages in a captured ColocatedPipeline at B = 64, replayed on two byte
    batches: bitwise the default pipeline on the normalised inputs, and within the tolerance of
    tests/test_pipeline_gpu.py (2e-2 on probabilities) of the fp32 torch model."""
    from distributed_neural_networks_amd.models import cifar
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    from distributed_neural_networks_amd.ops import cifar as cops
    from distributed_neural_networks_amd.runtime.pipeline import ColocatedPipeline
    from distributed_neural_networks_amd.runtime.stages import CifarHipStage
    B = 64
    sd = cifar.random_state_dict(5)
    full = NeuralNetwork().eval()
    full.load_state_dict(sd)
    u = ColocatedPipeline([CifarHipStage(sd, 0, 1, DEV, input_dtype="uint8"), CifarHipStage(sd, 2, 3, DEV)], B)
    d = ColocatedPipeline([CifarHipStage(sd, 0, 1, DEV), CifarHipStage(sd, 2, 3, DEV)], B)
    assert u.x.dtype == torch.uint8 and tuple(u.x.shape) == (B, 32, 32, 3)
    u.capture()
    d.capture()
    table = cops.make_input_table()
    g = torch.Generator().manual_seed(29)
    for rnd in range(2):
        x8 = torch.randint(0, 256, (B, 32, 32, 3), dtype=torch.uint8, generator=g)
        xf = cops.normalize_u8(x8, table)
        got = u(x8.to(DEV))
        gp, gk = got.probs.clone(), got.pred.clone()
        want = d(xf.to(DEV))
        torch.cuda.synchronize()
        _assert_bits(gp.view(torch.int32), want.probs.view(torch.int32), f"replay {rnd}: probabilities")
        assert torch.equal(gk, want.pred), f"replay {rnd}: predictions"
        with torch.no_grad():
            ref = full(xf)
        err = (gp.cpu() - ref).abs().max().item()
        print(f"replay {rnd}: max |p - p_torch| = {err:.3e}")
        assert err < 2e-2
        top2 = ref.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 4e-2  # rows whose winner the tolerance cannot change
        assert torch.equal(gk.cpu()[clear].long(), ref.argmax(1)[clear])


def test_cli_colocated_uint8_matches_golden(tmp_path):
    """node.py on a colocated 2-stage config with ``input_dtype: "uint8"``, a real .pth and a
    PNG (the CLI is what this test is about): the prediction is the torch model's on the image
    as cli.load_image normalises it."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    from PIL import Image
    from distributed_neural_networks_amd.cli import load_image
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(11)
    m = NeuralNetwork().eval()
    pth, img, cfg = tmp_path / "cifar10_model.pth", tmp_path / "x.png", tmp_path / "c.json"
    torch.save(m.state_dict(), pth)
    Image.fromarray(np.random.default_rng(0).integers(0, 255, (40, 40, 3), dtype=np.uint8)).save(img)
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{51000 + i}", "part_index": i, "device": 0}
                   for i in range(2)],
         "model_weights": str(pth), "num_parts": 2, "return_to_node_id": "node1", "transport": "colocated",
         "model": "cifar10", "input_dtype": "uint8"}
    cfg.write_text(json.dumps(c))
    r = subprocess.run([sys.executable, os.path.join(root, "node.py"), "--node_id", "node1", "--config", str(cfg),
                        "--input_image", str(img)], env=dict(os.environ, PYTHONPATH=root, PYTHONUNBUFFERED="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if "***** FINAL PREDICTION (Index):" in l]
    assert line, r.stdout[-2000:]
    pred = int(line[-1].split(":")[-1].strip().strip("*").strip())
    with torch.no_grad():
        ref = int(m(load_image(str(img), "t")).argmax(1))
    assert pred == ref
