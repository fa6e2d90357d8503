"""Video framing, the part that needs no GPU: the C ABI's argument validation and plan query (csrc/framing.hip), the host
arithmetic of motion324_amd/framing.py (tables, placement, pass order, union box) against the independent numpy model of
tests/framing_cases.py, and that model against the reference's own output files (tests/golden/framing.npz)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import framing_cases as fc
from conftest import GOLDEN, REPO

FRAMING = ("m324_frame_plan", "m324_frame_mask", "m324_frame_resample")
P = 4096                                                         # a stand-in address: nothing is dereferenced
MAX_SIDE = 16384


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "framing.npz")))


def test_framing_entry_points_are_declared_and_bound_at_abi_23():
    from motion324_amd import build, lib, ops
    text = open(os.path.join(REPO, "include", "m324.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in FRAMING:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert lib.ABI_VERSION == 23 and lib.load().m324_abi_version() == 23
    assert "framing.hip" in build.SOURCES                        # build() and build_sanitized() both walk SOURCES
    assert int(re.search(r"#define\s+M324_FRAME_MAX_SIDE\s+(\d+)", header).group(1)) == MAX_SIDE
    for word, code in ops.FRAME_MODES.items():                   # the wrappers' codes are the header's
        assert int(re.search(r"#define\s+M324_FRAME_" + word.upper() + r"\s+(\d+)", header).group(1)) == code
    for word, code in ops.FRAME_AXES.items():
        assert int(re.search(r"#define\s+M324_FRAME_AXIS_" + word.upper() + r"\s+(\d+)", header).group(1)) == code


@pytest.mark.parametrize("in_size,out_size,ksize", [(36, 512, 7), (512, 512, 7), (1, 512, 7), (680, 512, 9), (2100, 512, 27), (1024, 512, 13),
                                                   (5, 2, 17), (7, 4, 13), (1920, 512, 25), (MAX_SIDE, 1, 6 * MAX_SIDE + 1)])
def test_frame_plan_ksize_and_scratch(in_size, out_size, ksize):
    from motion324_amd import lib, ops
    assert ksize == 2 * math.ceil(3 * max(in_size / out_size, 1.0)) + 1
    need = C.c_long(-1)
    assert lib.load().m324_frame_plan(in_size, out_size, 37, 3, 5, C.addressof(need)) == ksize
    assert need.value == 5 * 37 * out_size * 3
    assert lib.load().m324_frame_plan(in_size, out_size, 37, 1, 5, None) == ksize                # the size is optional
    assert ops.frame_plan(in_size, out_size, 37, 1, 5) == (ksize, 5 * 37 * out_size)
    assert fc.model_tables(in_size, out_size)[0].shape == (out_size, ksize) or in_size == MAX_SIDE


def test_frame_plan_refusals():
    from motion324_amd import lib, ops
    for args, word in (((0, 8, 1, 3, 1), "positive"), ((8, 0, 1, 3, 1), "positive"), ((-3, 8, 1, 3, 1), "positive"), ((8, 8, 0, 3, 1), "positive"),
                       ((8, 8, 1, 3, 0), "positive"), ((8, 8, 1, 2, 1), "channels"), ((8, 8, 1, 4, 1), "channels"),
                       ((MAX_SIDE + 1, 8, 1, 3, 1), "at most"), ((8, MAX_SIDE + 1, 1, 3, 1), "at most"), ((8, 8, MAX_SIDE + 1, 3, 1), "at most")):
        assert lib.load().m324_frame_plan(*args, None) == -1, args
        assert "m324_frame_plan" in lib.last_error() and word in lib.last_error(), (args, lib.last_error())
    with pytest.raises(lib.M324Error, match="m324_frame_plan"):
        ops.frame_plan(0, 8)


def test_frame_mask_validates_before_any_hip_call():
    """every refusal returns -1 with a message on a machine without a GPU: the checks run before the first HIP call"""
    from motion324_amd import lib
    h = lib.load()
    ok = dict(src=P, sf=40 * 30 * 4, sp=30 * 4, spx=4, alpha=None, af=0, ap=0, apx=0, T=2, H=40, W=30, mode=1, thr=204, table=None, masked=None,
              mask=None, boxes=P)

    def call(**kw):
        a = dict(ok, **kw)
        return h.m324_frame_mask(a["src"], a["sf"], a["sp"], a["spx"], a["alpha"], a["af"], a["ap"], a["apx"], a["T"], a["H"], a["W"], a["mode"],
                                 a["thr"], a["table"], a["masked"], a["mask"], a["boxes"], None)
    for kw, word in ((dict(src=None), "null"), (dict(boxes=None), "null"),
                     (dict(T=0), "positive"), (dict(H=0), "positive"), (dict(W=-1), "positive"),
                     (dict(spx=2), "pixel stride"), (dict(spx=5), "pixel stride"),
                     (dict(sp=30 * 4 - 2), "strides too short"), (dict(sf=40 * 30 * 4 - 1), "strides too short"), (dict(sf=-1), "strides too short"),
                     (dict(spx=3, sp=90, sf=3600), "RGBA"),                                      # RGB without an alpha plane
                     (dict(sp=30 * 4 - 1), "strides too short"),                                 # holds RGB at stride 4, not RGBA
                     (dict(spx=3, sp=90, sf=3600, alpha=P, af=1200, ap=30, apx=0), "alpha strides"),
                     (dict(spx=3, sp=90, sf=3600, alpha=P, af=1200, ap=29, apx=1), "alpha strides"),
                     (dict(spx=3, sp=90, sf=3600, alpha=P, af=1199, ap=30, apx=1), "alpha strides"),
                     (dict(mode=0), "mode"), (dict(mode=3), "mode"), (dict(mode=7), "mode"),
                     (dict(thr=-1), "threshold"), (dict(thr=256), "threshold"),
                     (dict(mode=2, table=None), "table"),
                     (dict(T=70000, H=16384, W=16384, sp=16384 * 4, sf=16384 * 16384 * 4), "too large")):
        assert call(**kw) == -1, kw
        assert "m324_frame_mask" in lib.last_error() and word in lib.last_error(), (kw, lib.last_error())


def test_frame_resample_validates_before_any_hip_call():
    from motion324_amd import lib
    h = lib.load()
    ok = dict(src=P, sf=40 * 90, sp=90, spx=3, sw=30, sh=40, cx=2, cy=3, cw=20, ch=30, C=3, T=2, axis=0, coef=P, bounds=P, out=50, ksize=7,
              alpha=None, af=0, ap=0, apx=0, mode=0, thr=204, table=None, dst=P, df=64 * 64 * 3, dp=64 * 3, dpx=3, dw=64, dh=64, px=5, py=7, fill=0)

    def call(**kw):
        a = dict(ok, **kw)
        return h.m324_frame_resample(a["src"], a["sf"], a["sp"], a["spx"], a["sw"], a["sh"], a["cx"], a["cy"], a["cw"], a["ch"], a["C"], a["T"],
                                     a["axis"], a["coef"], a["bounds"], a["out"], a["ksize"], a["alpha"], a["af"], a["ap"], a["apx"], a["mode"],
                                     a["thr"], a["table"], a["dst"], a["df"], a["dp"], a["dpx"], a["dw"], a["dh"], a["px"], a["py"], a["fill"], None)
    masked = dict(alpha=P, af=40 * 30, ap=30, apx=1)
    for kw, word in ((dict(src=None), "null"), (dict(coef=None), "null"), (dict(bounds=None), "null"), (dict(dst=None), "null"),
                     (dict(C=2), "channels"), (dict(C=4), "channels"), (dict(axis=2), "axis"), (dict(axis=-1), "axis"),
                     (dict(T=0), "positive"), (dict(cw=0), "positive"), (dict(ch=-4), "positive"), (dict(out=0), "positive"),
                     (dict(ksize=0), "positive"), (dict(dw=0), "positive"), (dict(sh=0), "positive"),
                     (dict(cx=-1), "leaves"), (dict(cx=11), "leaves"), (dict(cy=11), "leaves"), (dict(cw=31, cx=0), "leaves"),
                     (dict(sw=MAX_SIDE + 1, cw=MAX_SIDE + 1, cx=0, sp=3 * (MAX_SIDE + 1), sf=120 * (MAX_SIDE + 1)), "at most"),
                     (dict(out=MAX_SIDE + 1), "at most"), (dict(ksize=6 * MAX_SIDE + 4), "at most"), (dict(dw=MAX_SIDE + 1), "at most"),
                     (dict(spx=2), "source strides"), (dict(sp=89), "source strides"), (dict(sf=40 * 90 - 1), "source strides"),
                     (dict(dpx=2), "destination strides"), (dict(dp=64 * 3 - 1), "destination strides"), (dict(df=5), "destination strides"),
                     (dict(mode=4), "masking mode"), (dict(mode=-1), "masking mode"),
                     (dict(mode=1), "alpha plane"), (dict(mode=3), "alpha plane"), (dict(mode=1, **dict(masked, ap=29)), "alpha plane"),
                     (dict(mode=1, **dict(masked, apx=0)), "alpha plane"),
                     (dict(mode=1, thr=256, **masked), "threshold"), (dict(mode=3, thr=-1, **masked), "threshold"),
                     (dict(mode=2, **masked), "table"),
                     (dict(px=15), "pasted"), (dict(py=35), "pasted"), (dict(px=-1), "pasted"),              # 50 x 30 at (px, py) in 64 x 64
                     (dict(axis=1, px=45), "pasted"), (dict(axis=1, py=15), "pasted"),                       # 20 x 50
                     (dict(fill=-2), "fill"), (dict(fill=256), "fill")):
        assert call(**kw) == -1, kw
        assert "m324_frame_resample" in lib.last_error() and word in lib.last_error(), (kw, lib.last_error())


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from motion324_amd import framing, ops
    from motion324_amd.lib import M324Error
    rgba = torch.zeros(1, 8, 8, 4, dtype=torch.uint8)
    with pytest.raises(M324Error, match="HIP device"):
        ops.frame_mask(rgba)
    with pytest.raises(M324Error, match="HIP device"):
        ops.frame_resample(rgba[..., :3], torch.zeros(4, 7, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int32), "x")
    with pytest.raises(M324Error, match="mode"):
        ops.frame_mask(rgba, mode="binary")
    with pytest.raises(M324Error, match="axis"):
        ops.frame_resample(rgba, rgba, rgba, "z")
    with pytest.raises(M324Error, match="device="):
        framing.frame_video(rgba)                                                                # a host video and no device
    with pytest.raises(M324Error, match="device="):
        framing.frame_video(rgba.numpy())
    with pytest.raises(M324Error, match="mode"):
        framing.frame_video(rgba, mode="hard", device="cuda")
    with pytest.raises(M324Error, match="threshold"):
        framing.frame_video(rgba, threshold=300, device="cuda")
    with pytest.raises(M324Error, match="size"):
        framing.frame_video(rgba, size=0, device="cuda")
    with pytest.raises(M324Error, match="positive"):
        framing.resample_tables(0, 4)
    with pytest.raises(M324Error, match="empty box"):
        framing.placement((4, 4, 4, 9))


@pytest.mark.parametrize("in_size,out_size", [(36, 512), (26, 370), (680, 512), (34, 26), (37, 33), (570, 512), (2100, 512), (8, 2), (512, 512),
                                              (40, 40), (1, 512), (1, 1), (100, 512), (1, 5), (5, 2), (7, 4), (1024, 512), (33, 169), (1920, 512),
                                              (1080, 288), (3, 1), (1000, 1)])
def test_resample_tables_equal_the_models(in_size, out_size):
    from motion324_amd import framing
    coef, bounds = framing.resample_tables(in_size, out_size)
    m_coef, m_bounds = fc.model_tables(in_size, out_size)
    assert coef.dtype == bounds.dtype == np.int32 and coef.shape == m_coef.shape and bounds.shape == (out_size, 2)
    assert np.array_equal(coef, m_coef) and np.array_equal(bounds, m_bounds)
    # what every table must satisfy whoever built it: windows inside the line, no more taps than columns, zeros past the window,
    # and weights that add up to one within the rounding of their taps
    assert np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 1] >= 1) and np.all(bounds.sum(axis=1) <= in_size) and np.all(bounds[:, 1] <= coef.shape[1])
    for i in range(out_size):
        assert not coef[i, bounds[i, 1]:].any()
        assert abs(int(coef[i].astype(np.int64).sum()) - (1 << 22)) <= bounds[i, 1]
    if in_size == out_size:                                      # an unchanged side: the pass is the identity
        assert np.array_equal(coef.argmax(axis=1) + bounds[:, 0], np.arange(out_size)) and np.all(coef.max(axis=1) == 1 << 22)
        assert np.count_nonzero(coef) == out_size


def test_soft_table_equals_the_models_and_threshold_masking_is_keep_or_zero():
    from motion324_amd import framing
    table = framing.soft_table()
    assert table.dtype == np.uint8 and table.shape == (256, 256) and np.array_equal(table, fc.model_soft_table())
    assert np.array_equal(table[255], np.arange(256)) and not table[0].any()
    x = np.arange(256, dtype=np.uint8)                           # the reference's float round trip is the identity on a kept value
    assert np.array_equal(((x.astype(np.float32) / 255.0) * 255).astype(np.uint8), x)


def test_placement_on_the_half_way_cases():
    from motion324_amd import framing
    assert framing.placement((2, 0, 7, 1024)) == (2, 512, 255, 0)              # 5 * 0.5 = 2.5 -> 2 (half to even)
    assert framing.placement((1, 0, 8, 1024)) == (4, 512, 254, 0)              # 7 * 0.5 = 3.5 -> 4
    assert framing.placement((0, 0, 1024, 3)) == (512, 2, 0, 255)              # 1.5 -> 2
    assert framing.placement((0, 0, 1024, 1)) == (512, 1, 0, 255)              # 0.5 -> 0 -> at least one pixel
    assert framing.placement((9, 5, 10, 105)) == (5, 512, 253, 0)              # 5.12 -> 5; (512 - 5) // 2 floors
    assert framing.placement((10, 8, 43, 108)) == (169, 512, 171, 0)           # odd leftover space: the offset floors
    assert framing.placement((7, 9, 8, 10)) == (512, 512, 0, 0)
    assert framing.placement((4, 10, 516, 50)) == (512, 40, 0, 236)
    assert framing.placement((0, 0, 30, 20), size=64) == (64, 43, 0, 10)       # 42.67 -> 43
    for name, c in fc.CASES.items():
        if c["box"] is not None:
            assert framing.placement(c["box"]) == fc.model_placement(c["box"]) == c.get("place", fc.model_placement(c["box"])), name


def test_pass_order_and_union_box():
    from motion324_amd import framing
    assert framing.pass_order(5, 1024, 512) == "yx" and framing.pass_order(7, 1024, 512) == "yx"
    assert framing.pass_order(5, 500, 250) == "xy"               # exactly a hundred times: not more
    assert framing.pass_order(5, 501, 250) == "yx"
    assert framing.pass_order(5, 1024, 1024) == "xy" and framing.pass_order(5, 1024, 2000) == "xy"          # the height does not shrink
    assert framing.pass_order(36, 570, 512) == "xy" and framing.pass_order(1920, 1080, 288) == "xy"
    boxes = np.array([[30, 20, 50, 40], [96, 70, 0, 0], [8, 25, 40, 35], [35, 5, 90, 61]], dtype=np.int32)
    assert framing.union_box(boxes) == (8, 5, 90, 61)
    assert framing.union_box(boxes[1:2]) is None and framing.union_box(np.zeros((0, 4), dtype=np.int32)) is None
    for name in fc.CASES:
        m = fc.model_of(name)
        assert (None if m is None else framing.union_box(m["boxes"])) == fc.CASES[name]["box"], name


@pytest.mark.parametrize("name", fc.GOLDEN_CASES)
def test_model_reproduces_the_reference_files(golden, name):
    """the reference's process_images_in_folder wrote these canvases (tests/golden/make_framing_golden.py)"""
    m = fc.model_of(name)
    assert m["box"] == tuple(golden[f"{name}.box"]) == fc.CASES[name]["box"]
    assert m["placement"] == tuple(golden[f"{name}.placement"])
    T = fc.CASES[name]["T"]
    assert len(golden[f"{name}.frames_sha256"]) == len(golden[f"{name}.mask_sha256"]) == T
    new_w, new_h, off_x, off_y = m["placement"]
    win = (slice(off_y, off_y + min(new_h, fc.WINDOW)), slice(off_x, off_x + min(new_w, fc.WINDOW)))
    for tag, t in (("first", 0), ("last", T - 1)):
        assert np.array_equal(m["frames"][t][win], golden[f"{name}.{tag}_frame"])
        assert np.array_equal(m["mask"][t][win], golden[f"{name}.{tag}_mask"])
    for t in range(T):
        assert fc.digest(m["frames"][t]) == str(golden[f"{name}.frames_sha256"][t])
        assert fc.digest(m["mask"][t]) == str(golden[f"{name}.mask_sha256"][t])


def test_cases_exercise_what_they_claim():
    assert fc.model_of("all_empty") is None
    assert fc.model_tables(2100, 512)[0].shape[1] == fc.CASES["long_kernel"]["ksize_x"] == 27
    assert fc.model_tables(36, 512)[0].shape[1] == 7 and fc.CASES["upscale"]["W"] * 3 == 159
    coef, bounds = fc.model_tables(80, 512)                      # a box that touches the edges: windows cut short at both ends
    assert bounds[0, 0] == 0 and bounds[0, 1] < coef.shape[1] and bounds[-1].sum() == 80 and bounds[-1, 1] < coef.shape[1]
    _, alpha = fc.make_video("thr_edge")
    assert (alpha[0, 2:21, 3:36] == 204).sum() > 200 and (alpha[0, 2:21, 3:36] == 205).sum() > 200 and alpha.max() == 205
    assert np.array_equal(fc.model_of("empty_middle")["boxes"][1], (66, 48, 0, 0))
    assert not fc.model_of("empty_middle")["frames"][1].any() and not fc.model_of("empty_middle")["mask"][1].any()
    boxes = fc.model_of("union")["boxes"]                        # each extreme from a different frame
    assert (boxes[:, 0].argmin(), boxes[:, 1].argmin(), boxes[:, 2].argmax(), boxes[:, 3].argmax()) == (1, 0, 2, 3)
    rgb, alpha = fc.soft_video()
    assert len(np.unique(alpha.astype(np.int32)[0][..., None] * 256 + rgb[0, ..., :1])) == 65536
    for name in ("half5", "half7"):                              # over a hundred times as tall as wide: the other pass order
        box = fc.CASES[name]["box"]
        assert box[3] - box[1] > 100 * (box[2] - box[0])


def test_model_equals_pillow_where_pillow_is_installed():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    shapes = [(int(rng.integers(1, 70)), int(rng.integers(1, 70)), int(rng.integers(1, 90)), int(rng.integers(1, 90))) for _ in range(10)]
    shapes += [(640, 5, 320, 2), (40, 40, 40, 17)]               # the turned pass order; an unchanged side
    for n, (h, w, new_h, new_w) in enumerate(shapes):
        C_ = (1, 3)[n % 2]
        img = rng.integers(0, 256, size=(h, w, C_), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img[..., 0] if C_ == 1 else img).resize((new_w, new_h), Image.Resampling.LANCZOS)).reshape(new_h, new_w, C_)
        assert np.array_equal(fc.model_resize(img[None], new_w, new_h)[0], ref), (h, w, new_h, new_w, C_)
