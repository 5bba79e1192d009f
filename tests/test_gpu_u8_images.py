"""uint8 page images through every image-list entry.  The governing property: for any uint8 image list, planar or
interleaved, at any byte alignment, each entry gives BIT FOR BIT what the fp32 entry gives on ``img.cpu().float().div(255)`` uploaded
as a planar fp32 image.  Every reference is formed on the CPU (a GPU division by a scalar may itself multiply by the reciprocal, which
is wrong at 126 of the 256 codes) and uploaded; every comparison is ``torch.equal``."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import DiTConfig, _lib, config as cfgs, evaluate, ops, stage_images, synth   # noqa: E402
from layoutdit_amd.detector_training import DetectorTrainStep                                                      # noqa: E402
from layoutdit_amd.modeling import DetectorInputTransform, DiTEncoder, LayoutDetectionModel                       # noqa: E402
from tests import guarded                                                                                          # noqa: E402
from tests import roi_oracle as roi                                                                                # noqa: E402
from tests.guarded import In, Out, Scratch                                                                         # noqa: E402

DEV = "cuda:0"
LAYOUTS = ("planar", "interleaved")


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu-marked test running without a GPU"
    _lib.load()


def _codes(seed, h, w, c=3):
    """A page as a decoder leaves it: uint8 [h, w, c] on the CPU."""
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8))


def _as_f32(hwc):
    """The planar fp32 image the codes stand for, formed on the CPU (ToTensor()) and uploaded."""
    return hwc.permute(2, 0, 1).contiguous().float().div(255).to(DEV)


def _as_u8(hwc, layout, offset=None):
    """The codes on the GPU as a [C, h, w] image in `layout`; `offset`: a view starting that many bytes into a larger buffer."""
    h, w, c = hwc.shape
    src = hwc if layout == "interleaved" else hwc.permute(2, 0, 1)
    if offset is None:
        flat = src.contiguous().to(DEV)
    else:
        buf = torch.full((offset + src.numel() + 5,), 0x5A, dtype=torch.uint8, device=DEV)
        flat = buf[offset:offset + src.numel()].view(src.shape)
        flat.copy_(src)
        assert flat.data_ptr() % 4 == offset % 4
    return flat.permute(2, 0, 1) if layout == "interleaved" else flat


# sizes h x w: single pixels and lines, an upsampled page whose 3 w is no multiple of 4, a downsampled one; two of them misaligned
RAGGED = [((1, 1), None), ((1, 7), None), ((7, 1), None), ((31, 17), 1), ((129, 80), 3), ((5, 9), None)]


@pytest.fixture(scope="module")
def ragged():
    return [_codes(100 + i, h, w) for i, ((h, w), _) in enumerate(RAGGED)]


@pytest.fixture(scope="module")
def tiny49():
    """More images than one launch's descriptors hold (PRE_MAX = 48)."""
    return [_codes(200 + i, 1 + i % 5, 1 + (3 * i) % 7) for i in range(49)]


# ---- the pixel contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_all_codes_identity_resize(layout):
    """Every code in every channel, resized 16 x 16 -> 16 x 16 with mean 0, std 1 (every blend weight is exactly 0 or 1): the output
    IS the value a code stands for, and must be the correctly rounded c / 255 of the CPU - not c * (1 / 255)."""
    rng = np.random.default_rng(7)
    chans = [np.arange(256), np.arange(255, -1, -1), rng.permutation(256)]
    hwc = torch.from_numpy(np.stack([c.reshape(16, 16) for c in chans], axis=-1).astype(np.uint8))
    want = hwc.permute(2, 0, 1).contiguous().float().div(255)
    assert np.array_equal(want.numpy(), hwc.permute(2, 0, 1).numpy().astype(np.float32) / np.float32(255))      # torch's CPU division is numpy's
    recip = hwc.permute(2, 0, 1).float() * (1.0 / 255.0)
    assert int((recip[0] != want[0]).sum()) == 126                                                               # the test tells the two apart
    got = ops.preprocess([_as_u8(hwc, layout, offset=1)], size=(16, 16), mean=0.0, std=1.0)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 16, 16)
    assert torch.equal(got[0].cpu(), want)


# ---- bit-equality with the fp32 entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (20, 18)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_preprocess_equals_the_fp32_entry(ragged, layout, size):
    u8 = [_as_u8(p, layout, off) for p, (_, off) in zip(ragged, RAGGED)]
    assert [t.data_ptr() % 4 for t in u8][3:5] == [1, 3]
    if layout == "interleaved":
        assert not u8[4].is_contiguous() and u8[4].stride() == (1, 240, 3)
    want = ops.preprocess([_as_f32(p) for p in ragged], size=size)
    got = ops.preprocess(u8, size=size)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert float(want.abs().max()) > 0.9                                       # (normalised pixels, not zeros)


@pytest.mark.parametrize("size", [(64, 64), (20, 18)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_preprocess_across_the_descriptor_chunk(tiny49, layout, size):
    want = ops.preprocess([_as_f32(p) for p in tiny49], size=size)
    got = ops.preprocess([_as_u8(p, layout, offset=i % 4 if i % 3 else None) for i, p in enumerate(tiny49)], size=size)
    assert torch.equal(got, want) and not torch.equal(got[48], got[47])


def test_gpu_lists_are_checked_image_by_image(ragged):
    inter, planar = _as_u8(ragged[3], "interleaved"), _as_u8(ragged[4], "planar")
    f32 = _as_f32(ragged[3])
    with pytest.raises(ValueError, match=r"images\[1\].*one memory layout"):
        ops.preprocess([inter, planar])
    with pytest.raises(ValueError, match=r"images\[1\].*uint8"):
        ops.preprocess([planar, f32])
    with pytest.raises(ValueError, match=r"images\[1\].*float32"):
        ops.preprocess([f32, planar])
    with pytest.raises(ValueError, match=r"images\[0\].*strides"):
        ops.preprocess([planar[:, :, ::2]])
    for dtype in (torch.int8, torch.bfloat16):                                 # still refused
        with pytest.raises(ValueError, match=r"images\[0\].*float32"):
            ops.preprocess([torch.zeros(3, 4, 4, dtype=dtype, device=DEV)])


# ---- fused paths ---------------------------------------------------------------------------------------------------------------------
def _embed_weights(Cc=32, T=17):
    rng = np.random.default_rng(1001)
    f = lambda *s: torch.from_numpy((0.02 * rng.standard_normal(s)).astype(np.float32)).to(DEV)      # noqa: E731
    return ops.cast_bf16(f(Cc, 768)), f(Cc), f(Cc), f(T, Cc)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_embed_bf16_images_equals_preprocess_then_embed(ragged, tiny49, layout):
    pw16, pb, cls, pos = _embed_weights()
    for pages, offs in ((ragged, [o for _, o in RAGGED]), (tiny49, [i % 4 if i % 3 else None for i in range(49)])):
        u8 = [_as_u8(p, layout, o) for p, o in zip(pages, offs)]
        two_step = ops.embed_bf16(ops.preprocess(u8, size=64), pw16, pb, cls, pos, 16)
        fused = ops.embed_bf16_images(u8, pw16, pb, cls, pos, 16, size=64)
        assert torch.equal(fused, two_step)
        assert torch.equal(fused, ops.embed_bf16_images([_as_f32(p) for p in pages], pw16, pb, cls, pos, 16, size=64))


@pytest.mark.parametrize("build", ["f32", "bf16", "f32x3", "f32x6", "fp8", "mxfp8"])
def test_forward_image_list_equals_transform_then_forward(ragged, build):
    """ViT-micro at 64 x 64, every build ldit_vit_forward_images serves: the taps of the two-step path bit for bit, fp32."""
    cfg = cfgs.vit_micro()
    m = DiTEncoder(cfg, compute_dtype=build).load_numpy(synth.synth_weights(cfg, 4)).to(DEV).eval()
    t = DetectorInputTransform(fixed_size=(64, 64))
    offs = [o for _, o in RAGGED]
    with torch.no_grad():
        batch = t([_as_f32(p) for p in ragged])[0].tensors
        if build == "fp8":
            m.calibrate_fp8(batch)
        want = m(batch).hidden_states
        for layout in LAYOUTS:
            u8 = [_as_u8(p, layout, o) for p, o in zip(ragged, offs)]
            assert torch.equal(t(u8)[0].tensors, batch)
            got = t.encode(m, u8).hidden_states
            for tp in cfg.taps:
                assert got[tp].dtype == torch.float32 and torch.equal(got[tp], want[tp]), (build, layout, tp)
    with pytest.raises(ValueError, match="float32 or float16"):               # a BATCH is still fp32 / fp16
        m(torch.zeros(1, 3, 64, 64, dtype=torch.uint8, device=DEV))


# ---- guard bands ---------------------------------------------------------------------------------------------------------------------
GUARD_PAGES = [((33, 17), 1), ((64, 64), 3), ((1, 7), 5)]


def _guard_specs(layout):
    """Each image at an odd offset inside a parent of its own: the bytes in front of and behind it hold the run's fill."""
    specs, pages = {}, []
    for i, ((h, w), off) in enumerate(GUARD_PAGES):
        hwc = _codes(300 + i, h, w)
        flat = (hwc if layout == "interleaved" else hwc.permute(2, 0, 1)).contiguous().reshape(-1)
        data = torch.zeros(off + flat.numel() + 7, dtype=torch.uint8)
        data[off:off + flat.numel()] = flat
        pad = torch.ones(data.numel(), dtype=torch.bool)
        pad[off:off + flat.numel()] = False
        specs[f"img{i}"] = In(data, pad=pad)
        pages.append(hwc)
    return specs, pages


def _guard_list(t):
    n = len(GUARD_PAGES)
    return ((C.c_void_p * n)(*[t[f"img{i}"].data_ptr() + off for i, (_, off) in enumerate(GUARD_PAGES)]),
            (C.c_int32 * n)(*[h for (h, _), _ in GUARD_PAGES]), (C.c_int32 * n)(*[w for (_, w), _ in GUARD_PAGES]))


def _twin(specs, call):
    return guarded.twin_run(specs, call, device=DEV, sync=torch.cuda.synchronize)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("size", [(64, 64), (20, 18)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_guard_bands_preprocess_u8(layout, size):
    lib = _lib.load()
    specs, pages = _guard_specs(layout)
    specs["out"] = Out((3, 3, *size), torch.float32)

    def call(t):
        ptrs, hs, ws = _guard_list(t)
        assert [p % 2 for p in ptrs] == [1, 1, 1]
        _lib.check(lib.ldit_preprocess_u8(ptrs, hs, ws, int(layout == "interleaved"), 3, 3, 0.5, 0.5, size[0], size[1], t["out"].data_ptr(),
                                          _stream()))

    res = _twin(specs, call)
    guarded.assert_written(res.poisoned["out"], "out")
    guarded.assert_finite(res.poisoned["out"], "out")
    assert torch.equal(res.clean["out"], ops.preprocess([_as_f32(p) for p in pages], size=size).cpu())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_guard_bands_embed_bf16_images_u8(layout):
    lib = _lib.load()
    pw16, pb, cls, pos = (x.cpu() for x in _embed_weights())
    specs, pages = _guard_specs(layout)
    specs.update(pw=In(pw16), pb=In(pb), cls=In(cls), pos=In(pos), out=Out((3, 17, 32), torch.float32), scratch=Scratch(3 * 16 * 768 * 2))

    def call(t):
        ptrs, hs, ws = _guard_list(t)
        _lib.check(lib.ldit_embed_bf16_images_u8(ptrs, hs, ws, int(layout == "interleaved"), 0.5, 0.5, t["pw"].data_ptr(), t["pb"].data_ptr(),
                                                 t["cls"].data_ptr(), t["pos"].data_ptr(), t["out"].data_ptr(), t["scratch"].data_ptr(),
                                                 3, 3, 64, 64, 16, 32, _stream()))

    res = _twin(specs, call)
    guarded.assert_written(res.poisoned["out"], "out")
    guarded.assert_finite(res.poisoned["out"], "out")
    want = ops.embed_bf16_images([_as_f32(p) for p in pages], pw16.to(DEV), pb.to(DEV), cls.to(DEV), pos.to(DEV), 16, size=64)
    assert torch.equal(res.clean["out"], want.cpu())


@pytest.mark.parametrize("build", ["f32", "bf16"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_guard_bands_vit_forward_images_u8(layout, build):
    """The fp32 build produces the batch with preprocess_images in its workspace; the bf16 build blends inside the im2col pass."""
    lib = _lib.load()
    cfg = cfgs.vit_micro()
    m = DiTEncoder(cfg, compute_dtype=build).load_numpy(synth.synth_weights(cfg, 4)).to(DEV).eval()
    taps = list(cfg.taps)
    lcfg = m._lcfg(64, 64, taps)
    packed = m._pack(lcfg, m._position_table(4, 4), torch.device(DEV))
    specs, pages = _guard_specs(layout)
    for i in range(len(taps)):
        specs[f"tap{i}"] = Out((3, 17, cfg.hidden_size), torch.float32)

    def call(t):
        ptrs, hs, ws = _guard_list(t)
        work = m._scratch(lcfg, 3, torch.device(DEV))
        tap_ptrs = (C.c_void_p * len(taps))(*[t[f"tap{i}"].data_ptr() for i in range(len(taps))])
        _lib.check(lib.ldit_vit_forward_images_u8(C.byref(lcfg), packed.data_ptr(), ptrs, hs, ws, int(layout == "interleaved"), 0.5, 0.5, 3,
                                                  tap_ptrs, work.data_ptr(), work.numel(), _stream()))

    res = _twin(specs, call)
    with torch.no_grad():
        want = m.forward_image_list([_as_f32(p) for p in pages], size=(64, 64)).hidden_states
    for i, tp in enumerate(taps):
        guarded.assert_written(res.poisoned[f"tap{i}"], f"tap{i}")
        guarded.assert_finite(res.poisoned[f"tap{i}"], f"tap{i}")
        assert torch.equal(res.clean[f"tap{i}"], want[tp].cpu()), (build, layout, tp)


# ---- detector ------------------------------------------------------------------------------------------------------------------------
PAGE_SIZES = ((91, 149), (167, 105), (91, 149), (167, 105))


@pytest.fixture(scope="module")
def detector():
    """The ViT-micro detector of tests/test_gpu_coco_eval.py (hidden 128, 3 layers; its recipe for weights that let a few dozen
    detections per image through), eval mode, and four uint8 pages of two sizes."""
    NC = 6
    cfg = DiTConfig(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512)
    torch.manual_seed(11)
    model = LayoutDetectionModel(config=cfg)
    model.model.backbone.backbone.dit.load_numpy(synth.synth_weights(cfg, seed=4))
    m = model.model
    with torch.no_grad():
        for p in m.rpn.head.parameters():
            p.copy_(torch.randn_like(p) * (0.03 if p.dim() == 4 and p.shape[-1] == 3 else 0.08 if p.dim() == 4 else 0.2))
        pred = m.roi_heads.box_predictor
        pred.cls_score.weight.copy_(torch.randn_like(pred.cls_score.weight) * 0.3)
        pred.bbox_pred.weight.copy_(torch.randn_like(pred.bbox_pred.weight) * 0.2)
        pred.cls_score.bias.zero_()
    model = model.to(DEV).eval()
    pages = [_codes(400 + i, h, w) for i, (h, w) in enumerate(PAGE_SIZES)]
    with torch.no_grad():
        batch = m.transform([_as_f32(p) for p in pages])[0].tensors
        feats = m.backbone(batch)
        proposals, _, count = m.rpn(feats, (224, 224), padded=True)
        y = m.roi_heads.head_padded(feats, proposals, count, (224, 224)).cpu().double().numpy()
        cnt = count.cpu().numpy()
        R = proposals.shape[1]
        valid = [y[b * R:b * R + cnt[b], :NC] for b in range(len(pages))]
        bias = 0.0
        while max(int((roi.softmax64(v + np.eye(NC)[0] * bias)[:, 1:] > 0.05).sum()) for v in valid) > 60:
            bias += 0.25
        pred.cls_score.bias[0] = bias
    return model, pages


def _same_detections(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == ["boxes", "labels", "scores"]
        for k in x:
            assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("feed", ["planar", "interleaved", "staged"])
def test_detector_forward_equals_the_fp32_list(detector, feed):
    """Boxes come back in the pages' OWN coordinates: img.shape[-2:] of a uint8 image is still the page size."""
    model, pages = detector
    with torch.no_grad():
        want = model([_as_f32(p) for p in pages])
        if feed == "staged":
            u8 = stage_images([p.numpy() for p in pages], DEV, layout="hwc")
            assert len({t.untyped_storage().data_ptr() for t in u8}) == 1 and u8[1].data_ptr() % 4 == (3 * 91 * 149) % 4 == 1
        else:
            u8 = [_as_u8(p, feed, offset=1 + i % 3) for i, p in enumerate(pages)]
        assert [tuple(t.shape) for t in u8] == [(3, h, w) for h, w in PAGE_SIZES]
        got = model(u8)
    assert sum(len(o["scores"]) for o in want) >= 8
    for o, (h, w) in zip(got, PAGE_SIZES):                                     # (the page's coordinates, not the 224 x 224 frame's)
        assert float(o["boxes"][:, 0::2].max()) <= w + 1e-3 and float(o["boxes"][:, 1::2].max()) <= h + 1e-3
    _same_detections(got, want)


def _targets():
    return [{"boxes": torch.tensor([[10.0, 12.0, 90.0, 70.0], [30.0, 20.0, 100.0, 85.0]], device=DEV), "labels": torch.tensor([1, 3], device=DEV)},
            {"boxes": torch.tensor([[5.0, 20.0, 80.0, 90.0]], device=DEV), "labels": torch.tensor([2], device=DEV)}]


def test_evaluate_equals_the_fp32_list(detector):
    model, pages = detector
    with torch.no_grad():
        first = model([_as_f32(p) for p in pages])
    targets = [{"boxes": o["boxes"][::2] + 3.0, "labels": o["labels"][::2]} for o in first]
    f32 = [_as_f32(p) for p in pages]
    u8 = [_as_u8(p, "interleaved", offset=1) for p in pages[:2]] + stage_images([p.numpy() for p in pages[2:]], DEV, layout="hwc")
    want = evaluate(model, [(f32[:2], targets[:2]), (f32[2:], targets[2:])])
    got = evaluate(model, [(u8[:2], targets[:2]), (u8[2:], targets[2:])])
    assert got == want and want["AR100"] > 0


def test_losses_and_train_step_equal_the_fp32_list():
    from tests.test_gpu_detector_step import _model, _seeded
    pages = [_codes(500, 120, 200), _codes(501, 97, 131)]
    targets = _targets()
    f32 = [_as_f32(p) for p in pages]
    u8 = stage_images([p.numpy() for p in pages], DEV, layout="hwc")
    a, b = _model(), _model()
    for fn in ("rpn_losses", "losses"):
        want, got = getattr(a, fn)(f32, targets, generator=_seeded(2)), getattr(b, fn)(u8, targets, generator=_seeded(2))
        assert sorted(got) == sorted(want) and len(want) == (2 if fn == "rpn_losses" else 4)
        for k in want:
            assert torch.equal(got[k], want[k]), (fn, k)
    sa, sb = DetectorTrainStep(a, lr=1e-3, weight_decay=0.0), DetectorTrainStep(b, lr=1e-3, weight_decay=0.0)
    la, lb = sa.step(f32, targets, generator=_seeded(3)), sb.step(u8, targets, generator=_seeded(3))
    torch.cuda.synchronize()
    assert all(torch.equal(la[k], lb[k]) for k in la) and (sa.steps, sb.steps) == (1, 1)
    pa, pb_ = a.state_dict(), b.state_dict()
    assert all(torch.equal(pa[k], pb_[k]) for k in pa)


def test_stage_images_on_the_gpu_reuses_its_pinned_buffer():
    from layoutdit_amd import StagingBuffer
    buf = StagingBuffer()
    pages = [_codes(600 + i, h, w) for i, (h, w) in enumerate(((31, 17), (12, 20), (1, 1)))]
    out = stage_images(pages, DEV, buf, layout="hwc")
    host = buf.host
    assert host.is_pinned() and all(t.is_cuda for t in out) and len({t.untyped_storage().data_ptr() for t in out}) == 1
    again = stage_images(list(reversed(pages)), DEV, buf, layout="hwc")
    assert buf.host is host
    for t, p in zip(out, pages):
        assert torch.equal(t.cpu(), p.permute(2, 0, 1))
    for t, p in zip(again, reversed(pages)):
        assert torch.equal(t.cpu(), p.permute(2, 0, 1))
    assert torch.equal(ops.preprocess(out, size=(20, 18)), ops.preprocess([_as_f32(p) for p in pages], size=(20, 18)))
