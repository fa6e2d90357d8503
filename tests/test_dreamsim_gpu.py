"""DreamSim on the device: the float resize and the QuickGELU epilogue element by element against fp64, the fp32 patch rows bit
for bit, the three small towers inside the recorded band, and the distance against the fp64 oracle under the propagated bound
(tests/dreamsim_cases.py, tests/ERROR_BOUNDS_DREAMSIM.md)."""
import numpy as np
import pytest
import torch

import clipsim_cases as CC
import dreamsim_cases as DC
import error_bounds as EB

from motion324_amd import dreamsim as D
from motion324_amd import lib, ops
from motion324_amd.lib import M324Error

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7777.0


def tables(n_in, n_out, antialias=True):
    w, first = D.resize_tables(n_in, n_out, antialias)
    return w, first, torch.from_numpy(w).to(DEV), torch.from_numpy(first).to(DEV)


# ------------------------------------------------------------------------------------------------ m324_resample_f32
# F, H, W -> out_h, out_w: tiny, enlarging, shrinking by 3 (6 taps), odd widths (53, 130), one whole 512 x 512 frame, and one small
# shape whose width is a multiple of 4 (the 16-byte forms of the y pass)
RESAMPLE_SHAPES = [(2, 5, 7, 3, 2), (2, 37, 53, 32, 32), (2, 96, 130, 32, 48), (1, 512, 512, 224, 224), (3, 40, 64, 24, 32)]


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("F_, H, W, oh, ow", RESAMPLE_SHAPES)
def test_resample_pass_against_fp64_in_both_source_forms(F_, H, W, oh, ow, axis):
    frames = CC.make_frames(F_, H, W, 7000 + H + W)
    samples = CC.bytes_to_float(frames)                             # fp32 [F,3,H,W]: v.float() / 255
    w, first, wd, fd = tables(W, ow) if axis == "x" else tables(H, oh)
    ref, bound, _ = DC.resample_pass(samples, w, first, axis)
    from_bytes = ops.resample_f32(torch.from_numpy(frames).to(DEV), wd, fd, axis)
    from_float = ops.resample_f32(torch.from_numpy(samples).to(DEV), wd, fd, axis)
    assert from_bytes.shape == ((F_, 3, H, ow) if axis == "x" else (F_, 3, oh, W)) and from_bytes.dtype == torch.float32
    worst = EB.assert_within(from_float, torch.from_numpy(ref), torch.from_numpy(bound), f"resample_f32 {H}x{W} {axis}")
    print(f"resample {F_}x{H}x{W} -> {oh}x{ow} axis {axis} ksize {w.shape[1]}: worst err / bound {worst:.3f}")
    assert torch.equal(from_bytes, from_float)                      # a byte is (float)v / 255, one fp32 division
    free = torch.rand((F_, 3, H, W), generator=torch.Generator().manual_seed(H)) * 1.2 - 0.1       # no byte / 255, some outside [0, 1]
    ref, bound, _ = DC.resample_pass(free.numpy(), w, first, axis)
    EB.assert_within(ops.resample_f32(free.to(DEV), wd, fd, axis), torch.from_numpy(ref), torch.from_numpy(bound), "resample_f32 free values")


@pytest.mark.parametrize("axis", ["x", "y"])
def test_resample_identity_and_unaligned_views(axis):
    x = torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    _, _, wd, fd = tables(64, 64)
    assert torch.equal(ops.resample_f32(x.to(DEV), wd, fd, axis).cpu(), x)
    # a frame of this byte clip is 41 * 20 * 3 = 2460 bytes: frames 1.. start off a 16-byte boundary -- the scalar form, the same chain
    frames = torch.from_numpy(CC.make_frames(3, 41, 20, 9)).to(DEV)
    w, first, wd, fd = tables(20, 8) if axis == "x" else tables(41, 8)
    whole = ops.resample_f32(frames, wd, fd, axis)
    assert frames[1:].data_ptr() % 16 != 0 and torch.equal(ops.resample_f32(frames[1:], wd, fd, axis), whole[1:])


@pytest.mark.parametrize("H, W, oh, ow", [(96, 130, 32, 48), (37, 53, 32, 32), (512, 512, 224, 224)])
def test_resize_two_passes_against_fp64(H, W, oh, ow):
    frames = CC.make_frames(1, H, W, 8000 + H)
    wy, fy, _, _ = tables(H, oh)
    wx, fx, _, _ = tables(W, ow)
    order = D.pass_order(H, W, oh, ow, wy.shape[1], wx.shape[1])
    tabs = {"x": (wx, fx), "y": (wy, fy)}
    ref1, b1, _ = DC.resample_pass(CC.bytes_to_float(frames), *tabs[order[0]], order[0])
    ref2, b2, _ = DC.resample_pass(ref1, *tabs[order[1]], order[1])
    carried, _, _ = DC.resample_pass(b1, *tabs[order[1]], order[1])          # the weights are non-negative: sum |w| e1
    got = D.resize(torch.from_numpy(frames).to(DEV), (oh, ow))
    assert got.shape == (1, 3, oh, ow)
    worst = EB.assert_within(got, torch.from_numpy(ref2), torch.from_numpy(1.01 * b2 + carried), f"resize {H}x{W}")
    print(f"resize {H}x{W} -> {oh}x{ow} order {order}: worst err / bound {worst:.3f}")
    # against the float64 tables: rounding a weight to fp32 moves it by U32 relative, a pass's sum by U32 sum |w| |x| <= U32 max |x|
    model = DC.resize_model(frames, oh, ow)
    assert (np.abs(got.cpu().numpy() - model) <= 1.01 * b2 + carried + 2.02 * EB.U32).all()


# ------------------------------------------------------------------------------------------------ m324_vit_patches_f32
@pytest.mark.parametrize("patch, S, F_, pad", [(16, 64, 3, 0), (16, 224, 1, 32), (14, 56, 2, 0)])
def test_vit_patches_f32_equal_the_host_formula(patch, S, F_, pad):
    img = torch.rand((F_, 3, S, S), generator=torch.Generator().manual_seed(patch + S)) * 1.2 - 0.1
    Kp = (3 * patch * patch + 31) // 32 * 32 + pad
    mean_std = torch.tensor(D.IMAGENET_MEAN + D.IMAGENET_STD, dtype=torch.float32, device=DEV)
    got = ops.vit_patches_f32(img.to(DEV), patch, mean_std, Kp).cpu()
    want = DC.patch_rows_model(img, patch, Kp, D.IMAGENET_MEAN, D.IMAGENET_STD)
    assert torch.equal(got, want)
    assert Kp > 3 * patch * patch or patch == 16
    assert bool((got[:, 3 * patch * patch:] == 0).all())
    if patch == 16 and S == 64:                                     # an image that is not 16-byte aligned: the scalar form, the same bits
        flat = torch.empty(img.numel() + 1, dtype=torch.float32, device=DEV)
        view = flat[1:].view(img.shape)
        view.copy_(img)
        assert view.data_ptr() % 16 != 0 and torch.equal(ops.vit_patches_f32(view, patch, mean_std, Kp).cpu(), want)


# ------------------------------------------------------------------------------------------------ QuickGELU epilogue
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M, N, K", [(70, 96, 64), (197, 320, 160)])
def test_quick_gelu_gemm_against_fp64(M, N, K, with_bias):
    g = torch.Generator().manual_seed(M + N + K)
    a, w = torch.randn((M, K), generator=g), torch.randn((N, K), generator=g) * (2.0 / K ** 0.5)
    bias = torch.randn((N,), generator=g) * 0.5 if with_bias else None
    whole = torch.full((M + 6, N + 4), SENTINEL, dtype=torch.float32, device=DEV)
    out = whole[3:3 + M, :N]
    ops.gemm(a.to(DEV), w.to(DEV), out, bias=None if bias is None else bias.to(DEV), act=lib.ACT_QUICK_GELU)
    z, dz = EB.gemm(a, w, bias=bias, out_dtype=torch.float32, parts=True)
    ref, bound = DC.quick_gelu(z), DC.quick_gelu_bound(z, dz)
    worst = EB.assert_within(out, ref, bound, f"quick gelu {M}x{N}x{K}")
    print(f"quick gelu {M}x{N}x{K} bias={with_bias}: worst err / bound {worst:.3f}")
    wcpu = whole.cpu()
    assert (wcpu[:3] == SENTINEL).all() and (wcpu[3 + M:] == SENTINEL).all() and (wcpu[:, N:] == SENTINEL).all()
    # the bound tells the two activations apart: for 1.5 <= |z| <= 2.5 erf-GELU and QuickGELU differ by 0.0081 to 0.0203
    # (ERROR_BOUNDS_DREAMSIM.md), and every such element's erf-GELU value must lie outside the bound around QuickGELU
    band = (z.abs() >= 1.5) & (z.abs() <= 2.5)
    gap = (EB.gelu(z) - ref).abs()
    assert int(band.sum()) > M * N // 10 and bool((gap[band] > bound[band]).all()) and float(gap[band].min()) >= 0.0081


def test_quick_gelu_at_large_arguments():
    M, N, K = 70, 96, 64
    bias = torch.tensor([100.0, -100.0] * (N // 2))
    out = torch.full((M, N), SENTINEL, dtype=torch.float32, device=DEV)
    ops.gemm(torch.zeros((M, K), device=DEV), torch.zeros((N, K), device=DEV), out, bias=bias.to(DEV), act=lib.ACT_QUICK_GELU)
    got = out.cpu()
    assert not torch.isnan(got).any()
    assert bool((got[:, 1::2] == 0).all()) and bool(((got[:, 0::2] - 100.0).abs() <= 2 * EB.U32 * 100.0).all())


def test_quick_gelu_refuses_what_is_not_built():
    M, N, K = 70, 96, 64
    f32 = dict(dtype=torch.float32, device=DEV)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    a, w, bias = torch.zeros((M, K), **f32), torch.zeros((N, K), **f32), torch.zeros((N,), **f32)
    out = torch.full((M, N), SENTINEL, **f32)
    other = torch.full((M, N), SENTINEL, **f32)
    obf = torch.full((M, N), 3.0, **bf)
    calls = [lambda: ops.gemm(torch.zeros((M, K), **bf), torch.zeros((N, K), **bf), obf, act=lib.ACT_QUICK_GELU),
             lambda: ops.gemm(torch.zeros((M, K), **bf), torch.zeros((N, K), **bf), out, act=lib.ACT_QUICK_GELU),
             lambda: ops.gemm(a, w, out, bias=bias, residual=other, act=lib.ACT_QUICK_GELU),
             lambda: ops.gemm(a, w, out, bias=bias, preact_out=other, act=lib.ACT_QUICK_GELU),
             lambda: ops.gemm(a, w, out, bias=bias, mul_by=other, act=lib.ACT_QUICK_GELU),
             lambda: ops.gemm(a, w, out, gamma=bias, act=lib.ACT_QUICK_GELU)]
    for call in calls:
        with pytest.raises(M324Error, match=r"\(-3\).*M324_ACT_QUICK_GELU"):
            call()
    with lib.tunable("M324_GEMM", 1):                               # the scalar-store schedule has no such epilogue
        with pytest.raises(M324Error, match=r"\(-3\).*QuickGELU"):
            ops.gemm(a, w, out, bias=bias, act=lib.ACT_QUICK_GELU)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((other == SENTINEL).all()) and bool((obf == 3.0).all())


# ------------------------------------------------------------------------------------------------ the band cases end to end
@pytest.fixture(scope="module")
def towers():
    return {}


def tower(towers, name):
    if name not in towers:
        towers[name] = D.VitTower(DC.weights(name), DEV, **DC.tower_kwargs(name))
    return towers[name]


@pytest.mark.parametrize("name", list(DC.CASES))
def test_tower_inside_the_band(name, towers):
    model = tower(towers, name)
    feats, taps = model.features(DC.images(name).to(DEV), taps=True)
    table = DC.golden()[name]
    got = dict(taps, features=feats)
    report = {k: (table[k].deviation(got[k].cpu().numpy()), DC.gate(name, k)) for k in DC.KEYS}
    print(name, {k: f"{d:.2e} / {g:.2e}" for k, (d, g) in report.items()})
    for k, (d, g) in report.items():
        assert d <= g, (name, k, d, g)


@pytest.mark.parametrize("name", ["dino_cls", "clip_quick"])
def test_tower_does_not_depend_on_the_chunking(name, towers):
    model = tower(towers, name)
    img = DC.images(name).to(DEV)
    per = model.bytes_per_image()
    assert model.images_per_chunk(3, per) == 1 and model.images_per_chunk(3, 3 * per) == 3
    one, taps1 = model.features(img, taps=True, max_scratch_bytes=per)
    three, taps3 = model.features(img, taps=True, max_scratch_bytes=3 * per)
    assert torch.equal(one, three) and all(torch.equal(taps1[k], taps3[k]) for k in DC.TAPS)
    assert DC.golden()[name]["features"].deviation(one.cpu().numpy()) <= DC.gate(name, "features")
    with pytest.raises(M324Error, match="scratch bytes"):
        model.features(img, max_scratch_bytes=per - 1)
    with pytest.raises(M324Error, match="expected fp32"):
        model.features(img[:, :, :-16])


@pytest.mark.parametrize("H, W", DC.DISTANCE_SOURCES)
def test_distance_against_the_fp64_oracle(H, W, towers):
    metric = D.DreamSim([tower(towers, n) for n in DC.CASES], size=None)
    a, b = DC.distance_frames(H, W)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = metric(ta, tb)
    assert got.dtype == torch.float64 and got.shape == (3,) and got.is_cuda
    fa, fb = DC.distance_features(a), DC.distance_features(b)
    devs = [DC.gate(n, "features") * DC.golden()[n]["features"].rms for n in DC.CASES]
    want, bound = DC.distance_model(fa, fb), DC.distance_bound(fa, fb, devs)
    err = np.abs(got.cpu().numpy() - want)
    print("distance", got.cpu().numpy(), "err", err, "bound", bound)
    assert (err <= bound).all(), (err, bound)
    assert float(metric(ta, ta.clone()).abs().max()) <= 1e-12
    assert torch.equal(metric(tb, ta), got)                         # no kernel's arithmetic depends on an image's place in the batch
    as_float = torch.from_numpy(CC.bytes_to_float(a)).to(DEV), torch.from_numpy(CC.bytes_to_float(b)).to(DEV)
    assert torch.equal(metric(*as_float), got)                      # bytes / 255 in fp32 are the same samples in both forms


def test_dreamsim_wants_one_size_unless_told_otherwise(towers):
    pair = [tower(towers, "dino_cls"), tower(towers, "clip_quick")]
    with pytest.raises(M324Error, match="every tower must take 224 x 224"):
        D.DreamSim(pair)
    with pytest.raises(M324Error, match="one shape and dtype"):
        D.DreamSim(pair, size=None)(torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV), torch.zeros((2, 8, 9, 3), dtype=torch.uint8, device=DEV))


def test_evaluate_clips_dreamsim_on_a_20_frame_clip(towers):
    metric = D.DreamSim([tower(towers, "dino_cls")], size=64)
    gt = torch.from_numpy(CC.make_frames(20, 72, 80, 91)).to(DEV)
    result = torch.from_numpy(CC.make_frames(20, 72, 80, 92)).to(DEV)
    score = D.evaluate_clips_dreamsim(gt, result, metric)
    per_frame = metric(gt, result).cpu().numpy()
    want = D.clip_statistics(per_frame)
    assert np.array_equal(score.per_frame, per_frame) and score.value == want.value and score.value_std == want.value_std
    kept = np.concatenate([per_frame, per_frame[-12:][::-1]])       # the padding repeats values
    assert score.per_video.shape == (1,) and abs(score.value - kept.mean()) <= 1e-15 and (per_frame > 0).all() and (per_frame < 2).all()


# ------------------------------------------------------------------------------------------------ refusals without a launch
def test_entry_points_refuse_without_a_launch():
    h = lib.load()
    buf = torch.full((4096,), SENTINEL, dtype=torch.float32, device=DEV)
    src = torch.zeros((65536,), dtype=torch.float32, device=DEV)
    first = torch.zeros((64,), dtype=torch.int32, device=DEV)
    o, s, f = buf.data_ptr(), src.data_ptr(), first.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    cases = [
        ("null src", h.m324_resample_f32(None, 0, 1, 8, 8, 0, s, f, 2, 4, o, stream), -1),
        ("null dst", h.m324_resample_f32(s, 0, 1, 8, 8, 0, s, f, 2, 4, None, stream), -1),
        ("axis", h.m324_resample_f32(s, 0, 1, 8, 8, 2, s, f, 2, 4, o, stream), -1),
        ("ksize 0", h.m324_resample_f32(s, 0, 1, 8, 8, 0, s, f, 0, 4, o, stream), -1),
        ("ksize 65", h.m324_resample_f32(s, 0, 1, 8, 8, 0, s, f, 65, 4, o, stream), -1),
        ("side", h.m324_resample_f32(s, 0, 1, 8, 16385, 0, s, f, 2, 4, o, stream), -1),
        ("n_out 0", h.m324_resample_f32(s, 0, 1, 8, 8, 1, s, f, 2, 0, o, stream), -1),
        ("Kp % 32", h.m324_vit_patches_f32(s, 1, 56, 14, s, o, 600, stream), -3),
        ("Kp short", h.m324_vit_patches_f32(s, 1, 56, 14, s, o, 576, stream), -3),
        ("S % patch", h.m324_vit_patches_f32(s, 1, 56, 15, s, o, 704, stream), -1),
        ("null mean_std", h.m324_vit_patches_f32(s, 1, 56, 14, None, o, 608, stream), -1),
    ]
    for what, rc, want in cases:
        assert rc == want, (what, rc, lib.last_error())
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
