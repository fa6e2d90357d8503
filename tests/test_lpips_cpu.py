"""LPIPS without a GPU: the weight loader, the clip rule of evaluate_clips, every host-side refusal, the oracle's mean identity, the
committed band, and the power of the gate against four planted faults (tests/ERROR_BOUNDS_LPIPS.md)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

import lpips_cases as LC
from motion324_amd import perceptual as P
from motion324_amd.lib import M324Error

ENTRY_POINTS = ("m324_conv3x3", "m324_maxpool2x2", "m324_lpips_prepare", "m324_lpips_layer")


@pytest.fixture(scope="module")
def clean():
    """{case: (low, up)} of the fp64 oracle, computed once"""
    return {name: LC.oracle(*LC.clips(name)) for name in LC.CASES}


# ------------------------------------------------------------------------------------------------ binding
def test_entry_points_are_declared_bound_and_built():
    from motion324_amd import build, lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "m324.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert lib.ABI_VERSION == 23 and lib.load().m324_abi_version() == 23          # added entry points: no bump
    assert "perceptual.hip" in build.SOURCES and "conv.hip" in build.SOURCES
    for macro, value in (("M324_CONV_KPAD", ops.CONV_KPAD), ("M324_CONV_MAX_CHANNELS", ops.CONV_MAX_CHANNELS),
                         ("M324_LPIPS_MAX_CHANNELS", ops.LPIPS_MAX_CHANNELS), ("M324_LPIPS_CHUNKS", ops.LPIPS_CHUNKS),
                         ("M324_LPIPS_U8_NHWC", ops.LPIPS_MODES["u8_nhwc"]), ("M324_LPIPS_F32_NCHW", ops.LPIPS_MODES["f32_nchw"])):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", header).group(1)) == value, macro


def test_c_abi_refuses_what_is_outside_the_shape_contract():
    """validation comes before the first HIP call, so it shows without a GPU"""
    from motion324_amd import lib
    h = lib.load()
    p = 4096                                             # an aligned stand-in: no call below gets as far as using it
    ok = dict(images=1, H=4, W=4, Cin=4, Cout=32, relu=1)

    def conv(**kw):
        a = dict(ok, **kw)
        return h.m324_conv3x3(p, p, p, p, a["images"], a["H"], a["W"], a["Cin"], a["Cout"], a["relu"], None)

    for bad, word in ((dict(Cin=3), "multiple of 4"), (dict(Cin=0), "multiple of 4"), (dict(Cout=48), "multiple of 32"),
                      (dict(Cout=8192), "at most"), (dict(H=0), "at least 1"), (dict(images=0), "at least 1"),
                      (dict(images=2 ** 15, H=2 ** 8, W=2 ** 8), "2^31"), (dict(relu=2), "relu")):
        assert conv(**bad) == -1 and word in lib.last_error(), (bad, lib.last_error())
    assert h.m324_conv3x3(None, p, p, p, 1, 4, 4, 4, 32, 1, None) == -1 and "null" in lib.last_error()
    assert h.m324_conv3x3(p + 4, p, p, p, 1, 4, 4, 4, 32, 1, None) == -1 and "aligned" in lib.last_error()
    assert h.m324_maxpool2x2(p, p, 1, 3, 4, 4, None) == -1 and "even" in lib.last_error()
    assert h.m324_maxpool2x2(p, p, 1, 4, 4, 6, None) == -1 and "multiple of 4" in lib.last_error()
    assert h.m324_lpips_prepare(p, 2, 0, 1, 4, 4, p, None) == -1 and "mode" in lib.last_error()
    assert h.m324_lpips_prepare(p, 0, 1, 1, 4, 4, p, None) == -1 and "normalize" in lib.last_error()
    assert h.m324_lpips_layer(p, p, p, 1, 16, 2048, p, p, None) == -1 and "channels" in lib.last_error()
    assert h.m324_lpips_layer(p, p, p, 1, 2 ** 25, 64, p, p, None) == -1 and "pixels" in lib.last_error()
    assert h.m324_lpips_layer(p, p, p, 0, 16, 64, p, p, None) == -1
    assert h.m324_lpips_layer(p, p, p, 1, 16, 64, None, p, None) == -1 and "null" in lib.last_error()


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from motion324_amd import ops
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(M324Error, match="HIP device"):
        ops.conv3x3(x, torch.zeros(48, 32), torch.zeros(32))
    with pytest.raises(M324Error, match="HIP device"):
        ops.maxpool2x2(x)
    with pytest.raises(M324Error, match="HIP device"):
        ops.lpips_prepare(torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(M324Error, match="HIP device"):
        ops.lpips_layer(x, x, torch.zeros(4))
    assert ops.conv_kpad(4) == 48 and ops.conv_kpad(64) == 576 and ops.conv_kpad(512) == 4608
    with pytest.raises(M324Error, match="HIP device"):
        P.LPIPS(P.load_lpips_weights(LC.state_dict()), "cpu")


# ------------------------------------------------------------------------------------------------ weights
def _torchvision_form(state):
    vgg = {}
    for key, idx in zip(P.CONV_KEYS, P.FEATURE_INDEX):
        vgg[f"features.{idx}.weight"], vgg[f"features.{idx}.bias"] = state[key + ".weight"], state[key + ".bias"]
    vgg["classifier.0.weight"] = torch.zeros(2, 2)                       # ignored
    return vgg, {k: state[k] for k in P.LIN_KEYS}


def _same(w1, w2):
    return all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(w1.conv, w2.conv)) and \
        all(torch.equal(a, b) for a, b in zip(w1.lin, w2.lin))


def test_loader_accepts_the_three_forms(tmp_path):
    state = LC.state_dict()
    w = P.load_lpips_weights(state)
    assert len(w.conv) == 13 and len(w.lin) == 5
    assert [tuple(wp.shape) for wp, _ in w.conv][:3] == [(48, 64), (576, 64), (576, 128)]
    assert [tuple(v.shape) for v in w.lin] == [(64,), (128,), (256,), (512,), (512,)]
    vgg, lin = _torchvision_form(state)
    assert _same(w, P.load_lpips_weights(vgg, lin))
    torch.save(state, tmp_path / "lpips.pth")
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    assert _same(w, P.load_lpips_weights(str(tmp_path / "lpips.pth")))
    assert _same(w, P.load_lpips_weights(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth")))
    assert P.synth_lpips_state_dict(LC.WEIGHT_SEED)["net.slice3.12.weight"].equal(state["net.slice3.12.weight"])       # seeded
    assert not P.synth_lpips_state_dict(LC.WEIGHT_SEED + 1)["net.slice3.12.weight"].equal(state["net.slice3.12.weight"])


def test_loader_refusals_name_the_key(tmp_path):
    state = LC.state_dict()
    vgg, lin = _torchvision_form(state)
    missing = {k: v for k, v in state.items() if k != "net.slice4.19.bias"}
    with pytest.raises(M324Error, match=r"no key 'net\.slice4\.19\.bias'"):
        P.load_lpips_weights(missing)
    bad = dict(state)
    bad["net.slice2.5.weight"] = torch.zeros(128, 64, 3, 1)
    with pytest.raises(M324Error, match=r"'net\.slice2\.5\.weight'.*\(128, 64, 3, 1\).*\(128, 64, 3, 3\)"):
        P.load_lpips_weights(bad)
    bad = dict(state)
    bad["lin3.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(M324Error, match=r"'lin3\.model\.1\.weight'"):
        P.load_lpips_weights(bad)
    bad = dict(state)
    bad["net.slice1.0.bias"] = torch.full((64,), float("nan"))
    with pytest.raises(M324Error, match="not finite"):
        P.load_lpips_weights(bad)
    with pytest.raises(M324Error, match="needs lin_state"):
        P.load_lpips_weights(vgg)
    with pytest.raises(M324Error, match=r"no key 'lin4\.model\.1\.weight'"):
        P.load_lpips_weights(vgg, {k: v for k, v in lin.items() if k != "lin4.model.1.weight"})
    with pytest.raises(M324Error, match=r"no key 'features\.28\.weight'"):
        P.load_lpips_weights({k: v for k, v in vgg.items() if k != "features.28.weight"}, lin)
    with pytest.raises(M324Error, match="lin_state goes with"):
        P.load_lpips_weights(state, lin)
    with pytest.raises(M324Error, match="no such file"):
        P.load_lpips_weights(str(tmp_path / "absent.pth"))
    torch.save([1, 2], tmp_path / "list.pth")
    with pytest.raises(M324Error, match="not a state dict"):
        P.load_lpips_weights(str(tmp_path / "list.pth"))
    with pytest.raises(M324Error, match="state dicts or paths"):
        P.load_lpips_weights(3)


@pytest.mark.parametrize("cin,cout", [(3, 64), (8, 32), (64, 96)])
def test_packed_layout_is_the_convolution(cin, cout):
    """out[pixel, n] = sum_k A[pixel, k] wp[k, n] with A's columns in (tap, channel) order over the zero-padded NHWC input -- the
    product m324_conv3x3 forms -- against conv2d, in fp64"""
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    w = torch.randn((cout, cin, 3, 3), generator=g)
    wp = P.pack_conv_weight(w)
    cin4 = (cin + 3) // 4 * 4
    from motion324_amd import ops
    assert tuple(wp.shape) == (ops.conv_kpad(cin4), cout) and not wp[9 * cin4:].any()
    x = torch.randn((2, cin, 5, 7), generator=g)
    nhwc = torch.zeros((2, 5, 7, cin4), dtype=torch.float64)
    nhwc[..., :cin] = x.permute(0, 2, 3, 1)
    padded = F.pad(nhwc, (0, 0, 1, 1, 1, 1))
    cols = torch.cat([padded[:, dy:dy + 5, dx:dx + 7, :] for dy in range(3) for dx in range(3)], dim=-1)        # [2,5,7,9 cin4]
    got = cols.reshape(-1, 9 * cin4) @ wp[:9 * cin4].double()
    want = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ clips
def _numpy_rule(values):
    """a literal transcription of the reference's process_single_video and only_final=True on per-frame values"""
    v = np.asarray(values, dtype=np.float64)
    if v.shape[0] < 32:
        needed = 32 - v.shape[0]
        v = np.concatenate([v, v[-needed:][::-1]])
    subs = [v[i:i + 32] for i in range(0, v.shape[0] - 32 + 1, 32)]
    results = np.array(subs)
    return np.mean(results), np.std(results), results.mean(axis=1)


@pytest.mark.parametrize("T", [16, 31, 32, 33, 64, 70])
def test_evaluate_clips_follows_the_rule(T):
    rng = np.random.default_rng(T)
    values = rng.random(T).astype(np.float32)
    gt = torch.zeros((T, 16, 16, 3), dtype=torch.uint8)
    calls = []

    def metric(a, b):
        calls.append((a.shape, b.shape))
        return torch.from_numpy(values)

    score = P.evaluate_clips(gt, gt.clone(), metric)
    mean, std, per_video = _numpy_rule(values)
    assert len(calls) == 1 and calls[0][0] == gt.shape                   # every frame pair once: padding repeats values, not work
    assert score.value == pytest.approx(mean, rel=1e-15) and score.value_std == pytest.approx(std, rel=1e-13)
    assert np.allclose(score.per_video, per_video, rtol=1e-15, atol=0) and len(score.per_video) == max(1, T // 32)
    assert np.array_equal(score.per_frame, values.astype(np.float64))
    kept = P.subvideo_frames(T)
    assert all(len(k) == 32 for k in kept)
    if T == 31:
        assert kept[0][-1] == 30 and kept[0][30] == 30                   # 0..30 then the last frame again


def test_evaluate_clips_refusals():
    gt = torch.zeros((15, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(M324Error, match="reference crashes"):
        P.evaluate_clips(gt, gt, lambda a, b: torch.zeros(15))
    with pytest.raises(M324Error, match="equal shapes"):
        P.evaluate_clips(torch.zeros((32, 16, 16, 3), dtype=torch.uint8), torch.zeros((32, 16, 32, 3), dtype=torch.uint8), None)


@pytest.mark.parametrize("shape,dtype,word", [
    ((2, 24, 16, 3), torch.uint8, "multiples of 16"), ((2, 16, 8, 3), torch.uint8, "multiples of 16"),
    ((2, 3, 40, 32), torch.float32, "multiples of 16"), ((2, 16, 16, 4), torch.uint8, r"uint8 \[T,H,W,3\]"),
    ((2, 16, 16, 3), torch.float32, r"fp32 \[T,3,H,W\]"), ((16, 16, 3), torch.uint8, "tensors"), ((0, 16, 16, 3), torch.uint8, "no frames")])
def test_size_and_shape_refusals(shape, dtype, word):
    x = torch.zeros(shape, dtype=dtype)
    with pytest.raises(M324Error, match=word):
        P.check_clip_pair(x, x)


def test_clip_pair_and_chunk_arithmetic():
    a = torch.zeros((2, 16, 32, 3), dtype=torch.uint8)
    with pytest.raises(M324Error, match="one shape and dtype"):
        P.check_clip_pair(a, torch.zeros((3, 16, 32, 3), dtype=torch.uint8))
    with pytest.raises(M324Error, match="one shape and dtype"):
        P.check_clip_pair(a, torch.zeros((2, 16, 32, 3), dtype=torch.float32))
    assert P.check_clip_pair(a, a) == (2, 16, 32, True)
    assert P.check_clip_pair(torch.zeros(5, 3, 48, 80), torch.zeros(5, 3, 48, 80)) == (5, 48, 80, False)
    per_pair = 512 * 512 * 1024                                          # two 64-channel maps of two frames: 268 MB
    assert P.BYTES_PER_PAIR_PIXEL == 1024
    assert P.pairs_per_chunk(32, 512, 512, 4 << 30) == 16 and P.pairs_per_chunk(32, 512, 512, per_pair) == 1
    assert P.pairs_per_chunk(3, 16, 16, 1 << 30) == 3
    with pytest.raises(M324Error, match="one 512 x 512 frame pair needs 268435456"):
        P.pairs_per_chunk(32, 512, 512, per_pair - 1)


def test_load_frames(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (3, 16, 32, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", frames)
    assert np.array_equal(P.load_frames(str(tmp_path / "clip.npy")), frames)
    d = tmp_path / "frames"
    d.mkdir()
    for i in (2, 0, 1):
        Image.fromarray(frames[i]).save(d / f"f_{i:03d}.png")
    assert np.array_equal(P.load_frames(str(d)), frames)                 # sorted by name
    with pytest.raises(M324Error, match="video files and resizing are out of scope"):
        P.load_frames(str(tmp_path / "clip.mp4"))
    np.save(tmp_path / "floats.npy", frames.astype(np.float32))
    with pytest.raises(M324Error, match="expected uint8"):
        P.load_frames(str(tmp_path / "floats.npy"))


# ------------------------------------------------------------------------------------------------ oracle, band, power
@pytest.mark.parametrize("name", list(LC.CASES))
def test_upsampled_mean_is_the_taps_own_mean(clean, name):
    low, up = clean[name]
    assert np.all(np.abs(up - low) <= 1e-12 * np.abs(low)), np.abs(up / low - 1).max()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_committed_band_is_todays_oracle(clean, name):
    ref, band = LC.golden()[name]
    assert ref.shape == (LC.CASES[name][2], 5) and band.shape == (6,)
    assert np.allclose(clean[name][0], ref, rtol=1e-12, atol=0)
    assert np.all(band > 0) and np.all(band < 1e-4)                      # an fp32 run: small, and never exactly the fp64 value
    assert np.array_equal(LC.gate(name) >= LC.GATE_FACTOR * band, np.ones(6, bool))
    if name != "blackwhite32":
        assert np.array_equal(LC.gate(name), LC.GATE_FACTOR * band)


def test_clips_are_what_the_cases_say():
    a, b = LC.clips("near32")
    diff = a.astype(np.int64) - b.astype(np.int64)
    assert np.abs(diff).max() == 1 and 0.03 < (diff != 0).mean() < 0.07
    for name, (H, W, T, _) in LC.CASES.items():
        a, b = LC.clips(name)
        assert a.shape == b.shape == (T, H, W, 3) and a.dtype == b.dtype == np.uint8 and (a != b).any()
    a, b = LC.clips("blackwhite32")
    assert not a.any() and (b == 255).all()


@pytest.mark.parametrize("fault", LC.FAULTS)
def test_gate_sees_the_planted_fault(clean, fault):
    """each fault must land outside the gate for at least one case and layer"""
    seen = []
    for name in LC.CASES:
        low, _ = LC.oracle(*LC.clips(name), fault=fault)
        hit = LC.outside_gate(low, LC.golden()[name][0], LC.gate(name))
        seen += [(name, k) for k in range(6) if hit[k]]
    assert seen, fault
    if fault in ("relu5_3_before_relu", "shifted_tap"):                  # deep faults: only layer 5 (and with it the total) may move
        assert all(k >= 4 for _, k in seen), seen


def test_clean_oracle_is_inside_its_own_gate(clean):
    for name in LC.CASES:
        assert not LC.outside_gate(clean[name][0], LC.golden()[name][0], LC.gate(name)).any()
