"""Video framing on the GPU (csrc/framing.hip through motion324_amd.framing / ops): kernel output against the numpy model of
tests/framing_cases.py and against the digests of the reference's own files (tests/golden/framing.npz).  The arithmetic is
integer, so every comparison is torch.equal: there is no tolerance anywhere in this file."""
import os

import numpy as np
import pytest
import torch

import framing_cases as fc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAMED = [n for n, c in fc.CASES.items() if c["box"] is not None]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "framing.npz")))


def hand_over(name):
    """the clip of a case the way its layout says: (video, alpha) for frame_video"""
    rgb, alpha = fc.make_video(name)
    layout = fc.CASES[name]["layout"]
    if layout == "rgba":                                         # host-resident RGBA: frame_video uploads it
        return np.concatenate([rgb, alpha[..., None]], axis=3), None
    if layout == "rgb+alpha":                                    # host RGB, device alpha
        return rgb, torch.from_numpy(alpha).to(DEV)
    # "padded": device views -- RGB at a pixel stride of 4 in rows with 7 pixels of junk behind them, alpha in a padded plane of its own
    T, H, W = alpha.shape
    buf = torch.full((T, H, W + 7, 4), 0xAB, dtype=torch.uint8, device=DEV)
    buf[:, :, :W, :3] = torch.from_numpy(rgb).to(DEV)
    plane = torch.full((T, H + 2, W + 5), 0xFF, dtype=torch.uint8, device=DEV)
    plane[:, 1:H + 1, 3:W + 3] = torch.from_numpy(alpha).to(DEV)
    return buf[:, :, :W, :3], plane[:, 1:H + 1, 3:W + 3]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared model results are read-only


@pytest.mark.parametrize("name", FRAMED)
def test_frame_video_equals_the_model_and_the_reference_files(golden, name):
    from motion324_amd import framing
    video, alpha = hand_over(name)
    out = framing.frame_video(video, alpha, device=DEV)
    m = fc.model_of(name)
    assert out.box == m["box"] == fc.CASES[name]["box"] and out.placement == m["placement"]
    assert out.frames.dtype == out.mask.dtype == torch.uint8 and out.frames.is_cuda and out.mask.is_cuda
    assert tuple(out.frames.shape) == (len(m["frames"]), 512, 512, 3) and tuple(out.mask.shape) == (len(m["frames"]), 512, 512)
    assert out.frames.is_contiguous() and out.mask.is_contiguous()
    assert torch.equal(out.frames, dev(m["frames"]))
    assert torch.equal(out.mask, dev(m["mask"]))
    ref = fc.CASES[name].get("same_as", name)                    # the padded hand-over of a clip gives that clip's canvases
    frames, mask = out.frames.cpu().numpy(), out.mask.cpu().numpy()
    for t in range(len(frames)):
        assert fc.digest(frames[t]) == str(golden[f"{ref}.frames_sha256"][t])
        assert fc.digest(mask[t]) == str(golden[f"{ref}.mask_sha256"][t])


def test_all_frames_empty_returns_none():
    from motion324_amd import framing
    video, alpha = hand_over("all_empty")
    assert framing.frame_video(video, alpha, device=DEV) is None


def test_device_resident_video_and_the_same_input_twice():
    from motion324_amd import framing
    video, _ = hand_over("union")
    resident = torch.from_numpy(video).to(DEV)
    a = framing.frame_video(resident)                            # no device=: the video's own
    b = framing.frame_video(resident)
    m = fc.model_of("union")
    assert a.box == b.box == m["box"] and a.placement == b.placement
    assert torch.equal(a.frames, b.frames) and torch.equal(a.mask, b.mask)
    assert torch.equal(a.frames, dev(m["frames"])) and torch.equal(a.mask, dev(m["mask"]))


def test_soft_mode_uses_every_table_entry():
    from motion324_amd import framing, ops
    rgb, alpha = fc.soft_video()
    out = framing.frame_video(rgb, alpha, mode="soft", device=DEV)
    m = fc.model_frame(rgb, alpha, mode="soft")
    assert out.box == m["box"] == (1, 0, 256, 256) and out.placement == m["placement"]          # column 0 has alpha 0
    assert torch.equal(out.frames, dev(m["frames"])) and torch.equal(out.mask, dev(m["mask"]))
    # the masking kernel on its own: the full-size masked video and the mask, W * 3 and W both multiples of 16
    masked, mask, boxes = ops.frame_mask(dev(rgb), dev(alpha), mode="soft", table=dev(framing.soft_table()))
    m_masked, m_mask = fc.model_mask(rgb, alpha, "soft")
    assert torch.equal(masked, dev(m_masked)) and torch.equal(mask, dev(m_mask)) and torch.equal(boxes, dev(fc.model_boxes(m_mask)))


@pytest.mark.parametrize("name", ["upscale", "interior", "down_wide", "padded", "empty_middle", "thr_edge", "half5"])
def test_frame_mask_outputs_and_boxes(name):
    """masked video, mask and boxes of the masking kernel alone, on rows that start on a 16-byte boundary (W = 120, 700 RGBA),
    rows that do not (W = 53 RGB: pitch 159), a tail shorter than a group, and views with padding"""
    from motion324_amd import ops
    rgb, alpha = fc.make_video(name)
    video, plane = hand_over(name)
    video = dev(video) if isinstance(video, np.ndarray) else video
    m_masked, m_mask = fc.model_mask(rgb, alpha)
    m_boxes = dev(fc.model_boxes(m_mask))
    masked, mask, boxes = ops.frame_mask(video, plane)
    assert torch.equal(masked, dev(m_masked)) and torch.equal(mask, dev(m_mask)) and torch.equal(boxes, m_boxes)
    assert boxes.dtype == torch.int32 and tuple(boxes.shape) == (len(rgb), 4)
    none_a, none_b, only = ops.frame_mask(video, plane, want_masked=False, want_mask=False)      # both outputs are optional
    assert none_a is None and none_b is None and torch.equal(only, m_boxes)
    lower = ops.frame_mask(video, plane, threshold=100)                                          # another threshold, another answer
    m2 = fc.model_mask(rgb, alpha, threshold=100)
    assert torch.equal(lower[0], dev(m2[0])) and torch.equal(lower[1], dev(m2[1])) and torch.equal(lower[2], dev(fc.model_boxes(m2[1])))


@pytest.mark.parametrize("channels", [1, 3])
def test_frame_resample_alone(channels):
    """one pass at a time through the entry point: a crop, both axes, one and three channels, region-only writes that leave the
    rest of the destination alone, and a fill that writes all of it"""
    from motion324_amd import framing, ops
    rng = np.random.default_rng(channels)
    img = rng.integers(0, 256, size=(2, 37, 53, channels), dtype=np.uint8)
    cx, cy, cw, ch = 4, 3, 45, 30
    crop = img[:, cy:cy + ch, cx:cx + cw]
    for axis, n_in, n_out in (("x", cw, 19), ("x", cw, 130), ("y", ch, 80), ("y", ch, 7), ("x", cw, cw), ("y", ch, ch)):
        coef, bounds = framing.resample_tables(n_in, n_out)
        expect = fc.model_pass(crop, coef, bounds, axis=1 if axis == "x" else 0)
        if n_in == n_out:
            assert np.array_equal(expect, crop)                  # an unchanged side reproduces its input
        src = dev(img if channels == 3 else img[..., 0])
        got = ops.frame_resample(src, dev(coef), dev(bounds), axis, channels=channels, crop=(cx, cy, cw, ch))
        assert tuple(got.shape) == expect.shape and torch.equal(got, dev(expect)), (axis, n_in, n_out)
        h, w = expect.shape[1:3]
        for fill in (-1, 9):
            out = torch.full((2, h + 5, w + 8, channels), 200, dtype=torch.uint8, device=DEV)
            ops.frame_resample(src, dev(coef), dev(bounds), axis, channels=channels, crop=(cx, cy, cw, ch), out=out, paste=(6, 2), fill=fill)
            want = np.full((2, h + 5, w + 8, channels), 200 if fill < 0 else fill, dtype=np.uint8)
            want[:, 2:2 + h, 6:6 + w] = expect
            assert torch.equal(out, dev(want)), (axis, n_in, n_out, fill)


def test_frame_resample_with_a_table_of_its_callers():
    """the tables are the caller's: windows far longer than a Lanczos pass of these sizes would have (so a workgroup cannot stage
    all of a span and reads the rest from memory), and entries outside the line, which are clamped -- never read out of bounds"""
    from motion324_amd import ops
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(1, 6, 700, 3), dtype=np.uint8)
    n_out, ksize = 700, 60
    coef = rng.integers(-400000, 600000, size=(n_out, ksize)).astype(np.int32)
    first = rng.integers(0, 700 - ksize, size=n_out)
    bounds = np.stack([first, np.full(n_out, ksize)], axis=1).astype(np.int32)
    for axis, src in (("x", img), ("y", np.ascontiguousarray(img.transpose(0, 2, 1, 3)))):
        expect = fc.model_pass(src, coef, bounds, axis=1 if axis == "x" else 0)
        assert 0 < np.count_nonzero(expect == 0) and 0 < np.count_nonzero(expect == 255)          # both ends of the clamp are met
        assert torch.equal(ops.frame_resample(dev(src), dev(coef), dev(bounds), axis), dev(expect)), axis
    wild = bounds.copy()
    wild[0] = (-5, 3)                                            # clamped to start 0
    wild[1] = (698, 9)                                           # cut at the end of the line: 2 taps
    wild[2] = (800, 4)                                           # outside: no tap, the rounding constant alone -> 0
    wild[3] = (10, 100000)                                       # at most ksize taps
    tame = wild.copy()
    tame[0], tame[1], tame[2], tame[3] = (0, 3), (698, 2), (700, 0), (10, ksize)
    assert torch.equal(ops.frame_resample(dev(img), dev(coef), dev(wild), "x"), dev(fc.model_pass(img, coef, tame, axis=1)))


def test_framed_clip_has_the_layout_the_driver_takes():
    """ops.patchify of frame_video(...).frames equals ops.patchify of the same bytes uploaded from the model's host result"""
    from motion324_amd import framing, ops
    video, alpha = hand_over("interior")
    out = framing.frame_video(video, alpha, device=DEV)
    host = torch.from_numpy(np.array(fc.model_of("interior")["frames"]))
    assert out.frames.dtype == host.dtype and tuple(out.frames.shape) == tuple(host.shape)
    for dtype in (torch.float32, torch.bfloat16):
        a = ops.patchify(out.frames, 224, 14, 640, dtype)
        b = ops.patchify(host.to(DEV), 224, 14, 640, dtype)
        assert torch.equal(a, b) and bool(a.float().abs().sum() > 0)
