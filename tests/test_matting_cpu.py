"""Matting without a GPU: the layer table and the loader, the batch-norm folding, the composite table against Pillow, the numpy model of
the normalisation, every host-side refusal, the committed band, the conditions of the quantised-mask check, and the power of the gate
against six planted faults (tests/ERROR_BOUNDS_MATTING.md)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

import framing_cases as FC
import matting_cases as MC
from motion324_amd import matting as M
from motion324_amd.lib import M324Error

ENTRY_POINTS = ("m324_conv3x3_ex", "m324_conv3x3_ex_tile", "m324_maxpool2x2_ceil", "m324_upsample_bilinear", "m324_matte_prepare",
                "m324_matte_fuse", "m324_matte_quantise")


# ------------------------------------------------------------------------------------------------ binding
def test_entry_points_are_declared_bound_and_built():
    from motion324_amd import build, lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "m324.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert lib.ABI_VERSION == 23 and lib.load().m324_abi_version() == 23          # added entry points: no bump
    assert "matting.hip" in build.SOURCES and "conv.hip" in build.SOURCES
    for macro, value in (("M324_CONV_MAX_DILATION", ops.CONV_MAX_DILATION), ("M324_MATTE_SIDES", ops.MATTE_SIDES),
                         ("M324_MATTE_MAX_SIDE", ops.MATTE_MAX_SIDE), ("M324_MATTE_CHUNKS", ops.MATTE_CHUNKS)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", header).group(1)) == value, macro


def test_c_abi_refuses_what_is_outside_the_shape_contract():
    """validation comes before the first HIP call, so it shows without a GPU"""
    from motion324_amd import lib
    h = lib.load()
    p = 4096                                             # an aligned stand-in: no call below gets as far as using it
    ok = dict(a=p, Ca=4, b=None, Cb=0, res=None, images=1, H=4, W=4, Cout=4, dilation=1, relu=1)

    def conv(**kw):
        a = dict(ok, **kw)
        return h.m324_conv3x3_ex(a["a"], a["Ca"], a["b"], a["Cb"], p, p, a["res"], p, a["images"], a["H"], a["W"], a["Cout"], a["dilation"],
                                 a["relu"], None)

    for bad, word in ((dict(Ca=3), "Ca must be"), (dict(Ca=0), "Ca must be"), (dict(Cb=4), "Cb must be"), (dict(b=p, Cb=0), "Cb must be"),
                      (dict(b=p, Cb=6), "Cb must be"), (dict(Cout=2), "Cout must be"), (dict(Cout=8192), "at most"),
                      (dict(Ca=4096, b=p, Cb=4), "at most"), (dict(H=0), "at least 1"), (dict(images=0), "at least 1"),
                      (dict(images=2 ** 15, H=2 ** 8, W=2 ** 8), "2^31"), (dict(dilation=0), "dilation"), (dict(dilation=65), "dilation"),
                      (dict(relu=2), "relu"), (dict(a=None), "null"), (dict(a=p + 4), "aligned"), (dict(b=p + 8, Cb=4), "aligned"),
                      (dict(res=p + 2), "aligned")):
        assert conv(**bad) == -1 and word in lib.last_error(), (bad, lib.last_error())
    assert h.m324_conv3x3_ex_tile(1, 4, 4, 6) == -1 and h.m324_conv3x3_ex_tile(0, 4, 4, 4) == -1 and h.m324_conv3x3_ex_tile(1, 4, 4, 4) == 32
    assert h.m324_maxpool2x2_ceil(p, p, 1, 0, 4, 4, None) == -1 and "at least 1" in lib.last_error()
    assert h.m324_maxpool2x2_ceil(p, p, 1, 3, 5, 6, None) == -1 and "multiple of 4" in lib.last_error()
    assert h.m324_maxpool2x2_ceil(p, None, 1, 3, 5, 4, None) == -1 and "null" in lib.last_error()
    assert h.m324_upsample_bilinear(p, p, 1, 2, 2, 0, 3, 4, None) == -1 and "at least 1" in lib.last_error()
    assert h.m324_upsample_bilinear(p, p, 1, 2, 2, 3, 20000, 4, None) == -1 and "sizes up to" in lib.last_error()
    assert h.m324_upsample_bilinear(p, p, 1, 2, 2, 3, 3, 5, None) == -1 and "multiple of 4" in lib.last_error()
    assert h.m324_upsample_bilinear(p, p + 4, 1, 2, 2, 3, 3, 4, None) == -1 and "aligned" in lib.last_error()
    assert h.m324_matte_prepare(p, 1, 4, 4, p, None, p, None) == -1 and "null" in lib.last_error()
    assert h.m324_matte_prepare(p, 1, 4, 4, None, p, p, None) == -1 and "null" in lib.last_error()
    assert h.m324_matte_prepare(p, 0, 4, 4, p, p, p, None) == -1 and ">= 1" in lib.last_error()
    assert h.m324_matte_prepare(p, 1, 4, 4, p, p, p + 4, None) == -1 and "aligned" in lib.last_error()
    assert h.m324_matte_prepare(p, 1, 4, 4, p + 2, p, p, None) == -1 and "aligned" in lib.last_error()
    assert h.m324_matte_quantise(p, 1, 0, p, p, p, None) == -1 and ">= 1" in lib.last_error()
    assert h.m324_matte_quantise(p, 2 ** 16, 2 ** 16, p, p, p, None) == -1 and "2^31" in lib.last_error()
    assert h.m324_matte_quantise(p, 1, 16, p, None, p, None) == -1 and "null" in lib.last_error()
    assert h.m324_matte_quantise(p, 1, 16, None, p, p, None) == -1 and "null" in lib.last_error()
    ptrs, hs, ws = (ctypes.c_void_p * 6)(*[p] * 6), (ctypes.c_int * 6)(*[4] * 6), (ctypes.c_int * 6)(*[4] * 6)
    oc = (ctypes.c_float * 7)(*[1.0] * 7)
    A = ctypes.addressof

    def fuse(ptrs=ptrs, hs=hs, ws=ws, stride=4, oc=oc, images=1, Ho=4, Wo=4, prob=p):
        return h.m324_matte_fuse(A(ptrs), A(hs), A(ws), stride, A(oc), images, Ho, Wo, prob, None, None)

    assert fuse(Ho=0) == -1 and "Ho and Wo" in lib.last_error()
    assert fuse(stride=0) == -1 and "side_stride" in lib.last_error()
    assert fuse(prob=None) == -1 and "null" in lib.last_error()
    assert fuse(hs=(ctypes.c_int * 6)(4, 4, 4, 4, 4, 5)) == -1 and "side map 5" in lib.last_error()
    assert fuse(ptrs=(ctypes.c_void_p * 6)(p, p, None, p, p, p)) == -1 and "side map 2" in lib.last_error()
    assert fuse(oc=(ctypes.c_float * 7)(1, 1, 1, float("nan"), 1, 1, 1)) == -1 and "outconv weight 3" in lib.last_error()
    assert fuse(oc=(ctypes.c_float * 7)(1, 1, 1, 1, 1, 1, float("inf"))) == -1 and "bias" in lib.last_error()


def test_every_new_wrapper_refuses_a_cpu_tensor():
    from motion324_amd import ops
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(M324Error, match="HIP device"):
        ops.conv3x3_ex(x, torch.zeros(48, 4), torch.zeros(4))
    with pytest.raises(M324Error, match="HIP device"):
        ops.maxpool2x2_ceil(x)
    with pytest.raises(M324Error, match="HIP device"):
        ops.upsample_bilinear(x, (8, 8))
    with pytest.raises(M324Error, match="HIP device"):
        ops.matte_prepare(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(M324Error, match="HIP device"):
        ops.matte_fuse([x] * 6, [1.0] * 6, 0.0, (4, 4))
    with pytest.raises(M324Error, match="HIP device"):
        ops.matte_quantise(torch.zeros(1, 4, 4))
    with pytest.raises(M324Error, match="6 side maps"):
        ops.matte_fuse([x] * 5, [1.0] * 6, 0.0, (4, 4))
    assert ops.conv3x3_ex_tile(1, 5, 5, 16) == 32 and ops.conv3x3_ex_tile(32, 320, 320, 32) == 32 and ops.conv3x3_ex_tile(32, 320, 320, 64) == 64
    assert ops.conv3x3_ex_tile(1, 20, 20, 512) == 64 and ops.conv3x3_ex_tile(32, 40, 40, 512) == 128      # the narrower tile until the chip is full
    with pytest.raises(M324Error):
        ops.conv3x3_ex_tile(1, 4, 4, 6)


def test_module_refusals():
    state = MC.state_dict("u2netp")
    weights = M.load_u2net_weights(state)
    with pytest.raises(M324Error, match="HIP device"):
        M.U2Net(weights, "cpu")
    with pytest.raises(M324Error, match="must be a U2Net"):
        M.matte_video(np.zeros((1, 8, 8, 3), np.uint8), None)
    with pytest.raises(M324Error, match="needs device="):
        M._device_video(np.zeros((1, 8, 8, 3), np.uint8), None, "matte_video")
    with pytest.raises(M324Error, match=r"uint8 frames \[T,H,W,3\]"):
        M._device_video(np.zeros((1, 8, 8, 4), np.uint8), "cpu", "matte_video")
    per_frame = 4 * M.FLOATS_PER_FRAME_PIXEL * 320 * 320
    with pytest.raises(M324Error, match=f"needs {per_frame} scratch bytes, max_scratch_bytes is 1000"):
        M.frames_per_chunk(4, 320, 1000)
    assert M.frames_per_chunk(4, 320, per_frame) == 1 and M.frames_per_chunk(4, 320, 3 * per_frame) == 3
    assert M.frames_per_chunk(4, 320, 100 * per_frame) == 4 and M.frames_per_chunk(256, 320, M.DEFAULT_MAX_SCRATCH_BYTES) == 40


# ------------------------------------------------------------------------------------------------ the layer table and the loader
@pytest.mark.parametrize("variant", ["u2net", "u2netp"])
def test_layer_table_parameter_count_and_keys(variant):
    layers = M.network_layers(variant)
    assert len(layers) == 112 and len({p for p, *_ in layers}) == 112
    assert M.parameter_count(variant) == M.PARAMETERS[variant] == {"u2net": 44009869, "u2netp": 1131181}[variant]
    keys = M.state_dict_keys(variant)
    assert len(keys) == 112 * 6 + 14
    state = MC.state_dict(variant)
    assert set(state) == set(keys) | {p + ".bn_s1.num_batches_tracked" for p, *_ in layers}
    assert all(tuple(state[k].shape) == shape for k, shape in keys.items())
    for key in ("stage1.rebnconvin.conv_s1.weight", "stage1.rebnconv7.bn_s1.running_var", "stage5d.rebnconv3d.conv_s1.bias", "stage6.rebnconv4.bn_s1.weight",
                "stage1d.rebnconv6d.conv_s1.weight", "stage4.rebnconv3d.bn_s1.bias", "side6.weight", "outconv.bias"):
        assert key in keys, key
    dil = {p: d for p, _, _, d in layers}
    assert dil["stage1.rebnconv7"] == 2 and dil["stage1.rebnconv6"] == 1 and dil["stage4.rebnconv4"] == 2 and dil["stage2d.rebnconv6"] == 2
    assert [dil[f"stage5.rebnconv{n}"] for n in ("1", "2", "3", "4", "3d", "2d", "1d")] == [1, 2, 4, 8, 4, 2, 1]
    for stage, spec in M.VARIANTS[variant].items():              # the oracle's own table against the module's, every layer
        assert spec[0] == MC.STAGE_KIND[stage]
        assert all(d == MC.oracle_dilation(spec[0], name) for name, _, _, d in M.stage_layers(*spec)), stage
    w = M.load_u2net_weights(state)
    assert w.variant == variant and M.infer_variant(state) == variant and len(w.layers) == 112 and len(w.sides) == 6 and len(w.outconv) == 7
    cin = {p: c for p, c, _, _ in layers}
    for p, (wp, b, d) in w.layers.items():
        c4 = (cin[p] + 3) // 4 * 4
        assert wp.dtype == b.dtype == torch.float32 and wp.shape[0] == (9 * c4 + 15) // 16 * 16 and wp.shape[1] == b.shape[0] and d == dil[p]
        assert not wp[9 * c4:].any()
    for (wp, b), c in zip(w.sides, M.SIDE_CHANNELS[variant]):
        assert tuple(wp.shape) == (9 * c, 4) and tuple(b.shape) == (4,) and not wp[:, 1:].any() and not b[1:].any()


def test_loader_refusals(tmp_path):
    state = dict(MC.state_dict("u2netp"))
    missing = {k: v for k, v in state.items() if k != "stage3.rebnconv2.bn_s1.running_mean"}
    with pytest.raises(M324Error, match="no key 'stage3.rebnconv2.bn_s1.running_mean'"):
        M.load_u2net_weights(missing)
    wrong = dict(state, **{"side4.weight": torch.zeros(1, 32, 3, 3)})
    with pytest.raises(M324Error, match=r"'side4.weight' has shape \(1, 32, 3, 3\), expected \(1, 64, 3, 3\)"):
        M.load_u2net_weights(wrong)
    with pytest.raises(M324Error, match="'stage1.rebnconv1.conv_s1.weight' has shape"):
        M.load_u2net_weights(state, variant="u2net")
    nan = dict(state, **{"outconv.bias": torch.tensor([float("nan")])})
    with pytest.raises(M324Error, match="not finite"):
        M.load_u2net_weights(nan)
    negvar = dict(state, **{"stage2.rebnconv1.bn_s1.running_var": torch.full((16,), -1.0)})
    with pytest.raises(M324Error, match="folding the batch-norm of 'stage2.rebnconv1'"):
        M.load_u2net_weights(negvar)
    with pytest.raises(M324Error, match="no such file"):
        M.load_u2net_weights(str(tmp_path / "absent.pth"))
    (tmp_path / "u2net.onnx").write_bytes(b"\x08\x07")
    with pytest.raises(M324Error, match="ONNX"):
        M.load_u2net_weights(str(tmp_path / "u2net.onnx"))
    with pytest.raises(M324Error, match="variant must be one of"):
        M.network_layers("isnet")
    torch.save({"state_dict": state}, tmp_path / "p.pth")
    assert M.load_u2net_weights(str(tmp_path / "p.pth")).variant == "u2netp"


def test_batchnorm_folding_against_the_unfolded_fp64_layer():
    """running_var near 0 (the eps decides) and a negative batch-norm weight among the channels.  The folded weights are rounded once
    to fp32, so the fp64 convolution with them is within U32 (|x| (*) |w'| + |b'|) of the unfolded fp64 layer, plus the fp64 noise."""
    g = torch.Generator().manual_seed(5)
    cin, cout = 8, 6
    w, b = torch.randn((cout, cin, 3, 3), generator=g) * 0.2, torch.randn((cout,), generator=g)
    gamma = torch.tensor([1.0, -0.7, 0.3, 1.5, -1.2, 0.9])
    beta, mean = torch.randn((cout,), generator=g), torch.randn((cout,), generator=g)
    var = torch.tensor([1.0, 1e-7, 0.0, 0.5, 2.0, 3e-6])
    x = (torch.randn((2, cin, 7, 5), generator=g) + 0.5).double()
    want = F.batch_norm(F.conv2d(x, w.double(), b.double(), padding=2, dilation=2), mean.double(), var.double(), gamma.double(), beta.double(),
                        training=False, eps=1e-5)
    wf, bf = M.fold_batchnorm(w, b, gamma, beta, mean, var)
    assert wf.dtype == bf.dtype == torch.float32
    got = F.conv2d(x, wf.double(), bf.double(), padding=2, dilation=2)
    bound = MC.U32 * (F.conv2d(x.abs(), wf.double().abs(), padding=2, dilation=2) + bf.double().abs().reshape(1, -1, 1, 1)) * (1 + 1e-6)
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())
    assert float((got - want).abs().max()) > 0                                # the rounding is there: the bound is not vacuous
    assert float(wf[2].abs().max() / w[2].abs().max()) == pytest.approx(0.3 / 1e-5 ** 0.5, rel=1e-6)      # var 0: eps alone


# ------------------------------------------------------------------------------------------------ what rembg does
def test_composite_table_against_pillow_exhaustively():
    from PIL import Image
    value, alpha = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))     # [alpha, value]
    img = Image.fromarray(np.stack([value, value[:, ::-1], np.full_like(value, 255)], axis=-1))
    mask = Image.fromarray(alpha)
    cutout = np.asarray(Image.composite(img, Image.new("RGBA", img.size, 0), mask))
    table = M.composite_table()
    assert cutout.shape == (256, 256, 4) and table.shape == (256, 256) and table.dtype == np.uint8
    assert np.array_equal(cutout[..., 0], table) and np.array_equal(cutout[..., 1], table[:, ::-1])
    assert np.array_equal(cutout[..., 2], table[:, 255:256].repeat(256, 1))
    assert np.array_equal(cutout[..., 3], alpha) and np.array_equal(table[:, 255], np.arange(256))        # the cutout's alpha is the mask
    # the folded table: the composite, then the reference's rgb * (alpha / 255.0) on the cutout, as it writes it
    mask01 = cutout[:, :, 3:4] / 255.0
    want = (cutout[:, :, :1] * mask01).astype(np.uint8)[..., 0]
    assert np.array_equal(M.cutout_table(), want) and np.array_equal(MC.model_cutout_table(), want)
    assert np.array_equal(M.mask_levels(), mask01[:, 0, 0].astype(np.float32)) and M.mask_levels().dtype == np.float32
    assert not np.array_equal(M.cutout_table(), FC.model_soft_table())           # masking twice is not masking once


def test_normalisation_model_is_rembgs_formula_bit_for_bit():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 200, (3, 9, 7, 3), dtype=np.uint8)
    frames[1] = 0                                                               # an all-black frame: m = 1e-6
    frames[2, 4, 3, 1] = 255
    got = MC.model_prepare(frames)
    assert got.dtype == np.float32 and got.shape == (3, 9, 7, 4) and not got[..., 3].any()
    for t in range(3):
        im_ary = np.array(frames[t])
        im_ary = im_ary / max(np.max(im_ary), 1e-6)
        tmp = np.zeros((im_ary.shape[0], im_ary.shape[1], 3))
        tmp[:, :, 0] = (im_ary[:, :, 0] - 0.485) / 0.229
        tmp[:, :, 1] = (im_ary[:, :, 1] - 0.456) / 0.224
        tmp[:, :, 2] = (im_ary[:, :, 2] - 0.406) / 0.225
        want = np.expand_dims(tmp.transpose((2, 0, 1)), 0).astype(np.float32)
        assert np.array_equal(got[t, :, :, :3].transpose(2, 0, 1)[None], want)
    assert np.array_equal(got[1, 0, 0, :3], np.array([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]).astype(np.float32))
    q = MC.model_quantise(np.array([[[0.25, 0.5], [0.75, 0.25]], [[0.5, 0.5], [0.5, 0.5]]], dtype=np.float32))
    assert np.array_equal(q, np.array([[[0, 127], [255, 0]], [[0, 0], [0, 0]]], dtype=np.uint8))          # a constant frame: 0, not NaN


def test_segment_foreground_without_a_network_is_the_references_passthrough():
    frames = np.random.default_rng(2).integers(0, 256, (3, 6, 5, 3), dtype=np.uint8)
    masked, masks = M.segment_foreground_with_u2net(frames, None)
    assert masked is frames
    assert isinstance(masks, torch.Tensor) and masks.dtype == torch.float32 and tuple(masks.shape) == (3, 6, 5, 1) and bool((masks == 1).all())
    with pytest.raises(M324Error, match=r"\[T,H,W,3\]"):
        M.segment_foreground_with_u2net(frames[..., :2], None)
    alpha, cut, m = MC.model_from_mask(np.full((3, 4, 4), 255, np.uint8), frames)     # a full mask keeps the frames
    assert alpha.shape == (3, 6, 5) and cut.dtype == np.uint8 and np.array_equal(cut, frames) and m.dtype == np.float32 and m.shape == (3, 6, 5, 1)


# ------------------------------------------------------------------------------------------------ the band, the conditions, the power
def test_committed_band_covers_the_cases_and_the_document():
    band = MC.golden()
    assert set(band) == set(MC.CASES) and len(MC.CASES) == 8
    doc = open(os.path.join(REPO, "tests", "ERROR_BOUNDS_MATTING.md")).read()
    for name, b in band.items():
        assert b.shape == (len(MC.TENSORS),) and (b > 0).all() and (b < 1e-4).all(), (name, b)
        assert f"| {name} | {MC.CASES[name][1]} | {MC.CASES[name][2]} | {b[0]:.2e} |" in doc, name


@pytest.mark.parametrize("name", list(MC.CASES))
def test_fp32_cpu_oracle_passes_the_gate_and_the_quantised_check(name):
    """the recorded band re-derived on this machine stays inside the gate, the conditions of the quantised-mask check hold, and the
    fp32 CPU oracle alone passes that check: the cap on ambiguous pixels hides nothing"""
    variant = MC.CASES[name][0]
    x, ref = MC.reference(name)
    got = MC.oracle(variant, x, torch.float32)
    assert (MC.deviation(got, ref) <= MC.gate(name)).all()
    q, delta, R = MC.quantised_reference(name)
    assert R.min() >= MC.MIN_RANGE, R
    q32 = MC.model_quantise(MC.sigmoid64(got["d0"]).astype(np.float32))
    ambiguous, wrong, far = MC.check_quantised(name, q32)
    assert ambiguous <= MC.MAX_AMBIGUOUS and wrong == 0 and far == 0, (ambiguous, wrong, far, delta)
    assert MC.check_quantised(name, MC.model_quantise(MC.sigmoid64(ref["d0"])))[1:] == (0, 0)


@pytest.mark.parametrize("fault", MC.FAULTS)
def test_gate_sees_a_planted_fault(fault):
    hit = []
    for name, (variant, size, T) in MC.CASES.items():
        if T != 1:
            continue
        x, ref = MC.reference(name)
        dev = MC.deviation(MC.oracle(variant, x, torch.float64, fault=fault), ref)
        outside = ~(dev <= MC.gate(name))
        if outside.any():
            hit.append((name, [n for n, o in zip(MC.TENSORS, outside) if o]))
    assert hit, fault
    assert any("d0" in tensors for _, tensors in hit), (fault, hit)               # every fault reaches the logits
