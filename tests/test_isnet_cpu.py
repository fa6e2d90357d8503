"""ISNet without a GPU: the three new entry points in the header and the binding, their refusals, the layer table, the parameter
count and the key list, every loader refusal, conv_in left as the file has it, the numpy model of the normalisation with given
constants, the committed band, the conditions of the quantised-mask check, and the power of the gate against eight planted faults
(tests/ERROR_BOUNDS_ISNET.md)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

import isnet_cases as IC
import matting_cases as MC
from motion324_amd import matting as M
from motion324_amd.lib import M324Error

ENTRY_POINTS = ("m324_conv3x3_s2", "m324_matte_prepare_ex", "m324_matte_side")


# ------------------------------------------------------------------------------------------------ binding
def test_entry_points_are_declared_bound_and_built_with_matching_arity():
    from motion324_amd import lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "m324.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert proto, name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
        assert len(proto.group(1).split(",")) == len(lib.SIGNATURES[name]), name
    assert lib.ABI_VERSION == 23 and lib.load().m324_abi_version() == 23          # added entry points: no bump


def test_c_abi_refuses_what_is_outside_the_shape_contract():
    """validation comes before the first HIP call, so it shows without a GPU"""
    from motion324_amd import lib
    h = lib.load()
    p = 4096                                             # an aligned stand-in: no call below gets as far as using it
    ok = dict(x=p, wp=p, bias=p, out=p, images=1, H=5, W=4, Cin=4, Cout=4, relu=0)

    def conv(**kw):
        a = dict(ok, **kw)
        return h.m324_conv3x3_s2(a["x"], a["wp"], a["bias"], a["out"], a["images"], a["H"], a["W"], a["Cin"], a["Cout"], a["relu"], None)

    for bad, word in ((dict(Cin=3), "Ca must be"), (dict(Cin=0), "Ca must be"), (dict(Cout=2), "Cout must be"), (dict(Cout=8192), "at most"),
                      (dict(H=0), "at least 1"), (dict(images=0), "at least 1"), (dict(images=2 ** 15, H=2 ** 8, W=2 ** 8), "2^31"),
                      (dict(relu=2), "relu"), (dict(x=None), "null"), (dict(out=None), "null"), (dict(x=p + 4), "aligned"), (dict(out=p + 8), "aligned")):
        assert conv(**bad) == -1 and "m324_conv3x3_s2" in lib.last_error() and word in lib.last_error(), (bad, lib.last_error())

    ms = (ctypes.c_double * 6)(0.5, 0.5, 0.5, 1.0, 1.0, 1.0)
    A = ctypes.addressof

    def prepare(src=p, images=1, H=4, W=4, ms=ms, partial=p, frame_max=p, dst=p):
        return h.m324_matte_prepare_ex(src, images, H, W, A(ms) if ms is not None else None, partial, frame_max, dst, None)

    assert prepare(ms=None) == -1 and "null mean_std" in lib.last_error()
    assert prepare(src=None) == -1 and "null" in lib.last_error()
    assert prepare(images=0) == -1 and ">= 1" in lib.last_error()
    assert prepare(dst=p + 4) == -1 and "aligned" in lib.last_error()
    for bad, word in (((0.5, 0.5, 0.5, 1.0, 0.0, 1.0), "std 1"), ((0.5, 0.5, 0.5, 1.0, 1.0, -2.0), "std 2"), ((0.5, 0.5, 0.5, float("inf"), 1.0, 1.0), "std 0"),
                      ((0.5, 0.5, 0.5, 1.0, float("nan"), 1.0), "std 1"), ((0.5, float("nan"), 0.5, 1.0, 1.0, 1.0), "mean 1")):
        assert prepare(ms=(ctypes.c_double * 6)(*bad)) == -1 and word in lib.last_error(), (bad, lib.last_error())

    def side(s=p, h_=4, w=4, stride=4, images=1, Ho=8, Wo=8, prob=p, logit=None):
        return h.m324_matte_side(s, h_, w, stride, images, Ho, Wo, prob, logit, None)

    assert side(s=None) == -1 and "null" in lib.last_error()
    assert side(prob=None) == -1 and "null" in lib.last_error()
    assert side(Ho=0) == -1 and "Ho and Wo" in lib.last_error()
    assert side(Ho=20000) == -1 and "Ho and Wo" in lib.last_error()
    assert side(stride=0) == -1 and "side_stride" in lib.last_error()
    assert side(h_=9) == -1 and "side map" in lib.last_error()                   # Ho >= side_h
    assert side(w=0) == -1 and "side map" in lib.last_error()
    assert side(logit=p + 2) == -1 and "aligned" in lib.last_error()


def test_every_new_wrapper_refuses_a_cpu_tensor_and_bad_constants():
    from motion324_amd import ops
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(M324Error, match="HIP device"):
        ops.conv3x3_s2(x, torch.zeros(48, 4), torch.zeros(4))
    with pytest.raises(M324Error, match="HIP device"):
        ops.matte_side(x, (8, 8))
    with pytest.raises(M324Error, match="HIP device"):
        ops.matte_prepare(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), mean=IC.MEAN, std=IC.STD)
    with pytest.raises(M324Error, match="HIP device"):
        M.ISNet(M.load_isnet_weights(IC.state_dict()), "cpu")


# ------------------------------------------------------------------------------------------------ the layer table and the loader
def test_layer_table_parameter_count_and_keys():
    layers = M.isnet_layers()
    assert len(layers) == 112 and len({p for p, *_ in layers}) == 112
    assert M.isnet_parameter_count() == M.ISNET_PARAMETERS == 44046790
    assert M.ISNET_PARAMETERS == M.PARAMETERS["u2net"] + 35136 + 1792 - 7
    assert M.ISNET_STAGES == {"stage1": (7, 64, 32, 64), "stage2": (6, 64, 32, 128), "stage3": (5, 128, 64, 256), "stage4": (4, 256, 128, 512),
                              "stage5": ("4F", 512, 256, 512), "stage6": ("4F", 512, 256, 512), "stage5d": ("4F", 1024, 256, 512),
                              "stage4d": (4, 1024, 128, 256), "stage3d": (5, 512, 64, 128), "stage2d": (6, 256, 32, 64), "stage1d": (7, 128, 16, 64)}
    assert M.VARIANTS["u2net"]["stage1"] == (7, 3, 32, 64)                       # U2-Net's own table is not touched
    keys = M.isnet_state_dict_keys()
    assert len(keys) == 2 + 112 * 6 + 12 and "outconv.weight" not in keys and "pool_in.weight" not in keys
    assert list(keys)[:3] == ["conv_in.weight", "conv_in.bias", "stage1.rebnconvin.conv_s1.weight"] and list(keys)[-1] == "side6.bias"
    assert keys["conv_in.weight"] == (64, 3, 3, 3) and keys["stage1.rebnconvin.conv_s1.weight"] == (64, 64, 3, 3)
    assert [keys[f"side{k}.weight"][1] for k in range(1, 7)] == [64, 64, 128, 256, 512, 512]
    state = IC.state_dict()
    assert set(state) == set(keys) | {p + ".bn_s1.num_batches_tracked" for p, *_ in layers}
    assert all(tuple(state[k].shape) == shape for k, shape in keys.items())
    for stage, spec in M.ISNET_STAGES.items():                   # the oracle's own table against the module's, every layer
        assert spec[0] == MC.STAGE_KIND[stage]
        assert all(d == MC.oracle_dilation(spec[0], name) for name, _, _, d in M.stage_layers(*spec)), stage
    w = M.load_isnet_weights(state)
    assert len(w.layers) == 112 and len(w.sides) == 6 and M.is_isnet_state(state) and not M.is_isnet_state(MC.state_dict("u2net"))
    for (wp, b), c in zip(w.sides, M.ISNET_SIDE_CHANNELS):
        assert tuple(wp.shape) == (9 * c, 4) and tuple(b.shape) == (4,) and not wp[:, 1:].any() and not b[1:].any()
    assert (M.U2Net.input_size, M.U2Net.mean, M.U2Net.std) == (320, M.MEAN, M.STD) and M.ISNet.input_size == 1024
    assert (M.ISNET_MEAN, M.ISNET_STD) == (IC.MEAN, IC.STD) == ((0.485, 0.456, 0.406), (1.0, 1.0, 1.0))


def test_conv_in_is_not_folded():
    """no batch-norm follows conv_in: its weights reach the kernel as the file has them, repacked, and fold_batchnorm is what it was"""
    state = IC.state_dict()
    w = M.load_isnet_weights(state)
    wp, b = w.conv_in
    assert wp.dtype == b.dtype == torch.float32 and tuple(wp.shape) == (48, 64) and not wp[36:].any()
    taps = wp[:36].reshape(9, 4, 64)
    assert torch.equal(taps[:, :3], state["conv_in.weight"].permute(2, 3, 1, 0).reshape(9, 3, 64)) and not taps[:, 3].any()
    assert torch.equal(b, state["conv_in.bias"])
    g = torch.Generator().manual_seed(4)
    cw, cb, gamma, beta, mean, var = (torch.randn((6, 4, 3, 3), generator=g), torch.randn((6,), generator=g), torch.randn((6,), generator=g),
                                      torch.randn((6,), generator=g), torch.randn((6,), generator=g), torch.rand((6,), generator=g) + 0.5)
    wf, bf = M.fold_batchnorm(cw, cb, gamma, beta, mean, var)
    s = gamma.double() / torch.sqrt(var.double() + 1e-5)
    assert torch.equal(wf, (cw.double() * s.reshape(-1, 1, 1, 1)).float()) and torch.equal(bf, ((cb.double() - mean.double()) * s + beta.double()).float())
    prefix = "stage1.rebnconvin"
    wf, bf = M.fold_batchnorm(*(state[f"{prefix}.{k}"] for k in ("conv_s1.weight", "conv_s1.bias", "bn_s1.weight", "bn_s1.bias", "bn_s1.running_mean",
                                                                 "bn_s1.running_var")))
    assert torch.equal(w.layers[prefix][0], M.pack_conv_weight(wf)) and torch.equal(w.layers[prefix][1], bf) and w.layers[prefix][2] == 1


def test_loader_refusals(tmp_path):
    state = dict(IC.state_dict())
    for key in ("conv_in.bias", "stage3.rebnconv2.bn_s1.running_mean", "side5.weight"):
        with pytest.raises(M324Error, match=f"load_isnet_weights: the state dict has no key '{key}'"):
            M.load_isnet_weights({k: v for k, v in state.items() if k != key})
    with pytest.raises(M324Error, match=r"'conv_in.weight' has shape \(64, 4, 3, 3\), expected \(64, 3, 3, 3\)"):
        M.load_isnet_weights(dict(state, **{"conv_in.weight": torch.zeros(64, 4, 3, 3)}))
    with pytest.raises(M324Error, match=r"'side4.weight' has shape \(1, 32, 3, 3\), expected \(1, 256, 3, 3\)"):
        M.load_isnet_weights(dict(state, **{"side4.weight": torch.zeros(1, 32, 3, 3)}))      # a side that is never computed
    with pytest.raises(M324Error, match="'side6.bias' holds values that are not finite"):
        M.load_isnet_weights(dict(state, **{"side6.bias": torch.tensor([float("nan")])}))
    with pytest.raises(M324Error, match="folding the batch-norm of 'stage2.rebnconv1'"):
        M.load_isnet_weights(dict(state, **{"stage2.rebnconv1.bn_s1.running_var": torch.full((32,), -1.0)}))
    with pytest.raises(M324Error, match="load_isnet_weights: no such file"):
        M.load_isnet_weights(str(tmp_path / "absent.pth"))
    (tmp_path / "isnet-general-use.onnx").write_bytes(b"\x08\x07")
    with pytest.raises(M324Error, match="isnet-general-use.onnx' is an ONNX file"):
        M.load_isnet_weights(str(tmp_path / "isnet-general-use.onnx"))
    with pytest.raises(M324Error, match="no key 'conv_in.weight'"):               # a U2-Net dict handed to the ISNet loader
        M.load_isnet_weights(MC.state_dict("u2net"))
    with pytest.raises(M324Error, match="no key 'outconv.weight'"):               # an ISNet dict handed to the U2-Net loader
        M.load_u2net_weights(state)
    with pytest.raises(M324Error, match="no key 'outconv.weight'"):
        M.load_u2net_weights(state, variant="u2net")
    torch.save({"state_dict": state}, tmp_path / "p.pth")
    assert len(M.load_isnet_weights(str(tmp_path / "p.pth")).layers) == 112


def test_module_refusals_and_the_per_network_estimate():
    with pytest.raises(M324Error, match="must be a U2Net or an ISNet"):
        M.matte_video(np.zeros((1, 8, 8, 3), np.uint8), object())
    assert M.ISNet.floats_per_frame_pixel == M.ISNET_FLOATS_PER_FRAME_PIXEL and M.U2Net.floats_per_frame_pixel == M.FLOATS_PER_FRAME_PIXEL
    per_frame = 4 * M.ISNET_FLOATS_PER_FRAME_PIXEL * 1024 * 1024
    assert M.frames_per_chunk(32, 1024, 3 * per_frame, M.ISNET_FLOATS_PER_FRAME_PIXEL) == 3
    assert M.frames_per_chunk(32, 1024, M.DEFAULT_MAX_SCRATCH_BYTES, M.ISNET_FLOATS_PER_FRAME_PIXEL) == M.DEFAULT_MAX_SCRATCH_BYTES // per_frame >= 1
    assert M.frames_per_chunk(256, 320, M.DEFAULT_MAX_SCRATCH_BYTES) == 40       # U2-Net's figure is what it was
    with pytest.raises(M324Error, match=f"needs {per_frame} scratch bytes"):
        M.frames_per_chunk(4, 1024, per_frame - 1, M.ISNET_FLOATS_PER_FRAME_PIXEL)
    # the estimate from the stage table, per pixel of the half-size map at its widest point (stage1d), as the comment in matting.py
    # counts it: both inputs, hxin, hx1 and an upsampled decoder map at mid width, the result, and the stem's output kept as a tap
    _, cin, mid, cout = M.ISNET_STAGES["stage1d"]
    widest = cin + cout + 2 * mid + cout + M.ISNET_STEM[1]
    assert widest == 352 and M.ISNET_FLOATS_PER_FRAME_PIXEL >= (widest + 70) / 4 + 7


# ------------------------------------------------------------------------------------------------ what rembg's DIS session does
def test_normalisation_model_with_given_constants_bit_for_bit():
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 200, (3, 9, 7, 3), dtype=np.uint8)
    frames[1] = 0                                                               # an all-black frame: m = 1e-6
    frames[2, 4, 3, 1] = 255
    for mean, std in ((IC.MEAN, IC.STD), ((0.5, 0.25, 0.125), (1.0, 0.3, 2.0))):
        got = IC.model_prepare(frames, mean, std)
        assert got.dtype == np.float32 and got.shape == (3, 9, 7, 4) and not got[..., 3].any()
        for t in range(3):
            im_ary = np.array(frames[t])
            im_ary = im_ary / max(np.max(im_ary), 1e-6)
            tmp = np.zeros((im_ary.shape[0], im_ary.shape[1], 3))
            tmp[:, :, 0] = (im_ary[:, :, 0] - mean[0]) / std[0]
            tmp[:, :, 1] = (im_ary[:, :, 1] - mean[1]) / std[1]
            tmp[:, :, 2] = (im_ary[:, :, 2] - mean[2]) / std[2]
            want = np.expand_dims(tmp.transpose((2, 0, 1)), 0).astype(np.float32)
            assert np.array_equal(got[t, :, :, :3].transpose(2, 0, 1)[None], want)
        assert np.array_equal(got[1, 0, 0, :3], (-np.array(mean) / np.array(std)).astype(np.float32))
    assert np.array_equal(IC.model_prepare(frames, M.MEAN, M.STD), MC.model_prepare(frames))       # the ImageNet constants: U2-Net's model
    assert np.array_equal(IC.model_prepare(frames)[2, 4, 3, :3], np.array([frames[2, 4, 3, 0] / 255 - 0.485, 1 - 0.456, frames[2, 4, 3, 2] / 255 - 0.406]).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the band, the conditions, the power
def test_committed_band_matches_its_generator_and_the_document():
    spec = importlib.util.spec_from_file_location("make_isnet_band", os.path.join(REPO, "tests", "golden", "make_isnet_band.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    band = IC.golden()
    assert list(band) == gen.CASE_LIST == list(IC.CASES) == ["isnet_40x1", "isnet_40x3", "isnet_37x1", "isnet_37x3"]
    doc = open(os.path.join(REPO, "tests", "ERROR_BOUNDS_ISNET.md")).read()
    for name, b in band.items():
        assert b.shape == (len(IC.TENSORS),) == (13,) and (b > 0).all() and (b < 1e-4).all(), (name, b)
        assert gen.row(name, b) in doc, name


@pytest.mark.parametrize("name", list(IC.CASES))
def test_fp32_cpu_oracle_passes_the_gate_and_the_quantised_check(name):
    """the recorded band re-derived on this machine stays inside the gate, the conditions of the quantised-mask check hold, and the
    fp32 CPU oracle alone passes that check within its caps: the cap on ambiguous pixels hides nothing"""
    x, ref = IC.reference(name)
    size, T = IC.CASES[name]
    half = (size - 1) // 2 + 1
    assert ref["d1"].shape == (T, size, size) and ref["hxin"].shape == (T, half, half, 64) and ref["hx1d"].shape == (T, half, half, 64)
    assert ref["hx6"].shape == (T, 1, 1, 512)                                    # stage6 on 1 x 1 maps
    got = IC.fp32_run(name)
    assert (IC.deviation(got, ref) <= IC.gate(name)).all()
    q, delta, R = IC.quantised_reference(name)
    assert R.min() >= IC.MIN_RANGE, R
    q32 = MC.model_quantise(MC.sigmoid64(got["d1"]).astype(np.float32))
    ambiguous, wrong, far = IC.check_quantised(name, q32)
    assert ambiguous <= IC.MAX_AMBIGUOUS and wrong == 0 and far == 0, (ambiguous, wrong, far, delta)
    assert IC.check_quantised(name, MC.model_quantise(MC.sigmoid64(ref["d1"])))[1:] == (0, 0)


@pytest.mark.parametrize("fault", IC.FAULTS)
def test_gate_sees_a_planted_fault(fault):
    """outside the gate, or another shape (deviation inf), for at least one case and tensor"""
    hit = []
    for name, (size, T) in IC.CASES.items():
        if T != 1:
            continue
        x, ref = IC.reference(name)
        dev = IC.deviation(IC.oracle(x, torch.float64, fault=fault), ref)
        outside = ~(dev <= IC.gate(name))
        if outside.any():
            hit.append((name, [n for n, o in zip(IC.TENSORS, outside) if o]))
    assert hit, fault
    assert any("d1" in tensors for _, tensors in hit), (fault, hit)               # every fault reaches the logits
