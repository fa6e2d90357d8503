"""ISNet on the GPU: ops.conv3x3_s2 bit for bit against the strided view of ops.conv3x3_ex and element by element against fp64, the
normalisation with given constants, the one-map head, the network (logits and twelve taps) against the fp64 oracle inside the
recorded gate, the quantised mask, everything behind it bit for bit against the host models, the exact properties and the command
line (tests/ERROR_BOUNDS_ISNET.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import error_bounds as EB
import framing_cases as FC
import isnet_cases as IC
import matting_cases as MC
from motion324_amd import framing, ops
from motion324_amd import matting as M
from motion324_amd.lib import M324Error

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (images, H, W, Cin, Cout): odd sizes and several tiles; the stem at the cases' size; K = 612 crosses four run boundaries with a ragged
# channel tile; one pixel with every tap but the centre outside
CONV_SHAPES = [(2, 37, 41, 4, 64), (1, 40, 40, 4, 64), (1, 2, 3, 68, 36), (3, 1, 1, 8, 32)]

_NETS = {}


def isnet():
    if "isnet" not in _NETS:
        _NETS["isnet"] = M.ISNet(M.load_isnet_weights(IC.state_dict()), DEV)
    return _NETS["isnet"]


def u2netp():
    if "u2netp" not in _NETS:
        _NETS["u2netp"] = M.U2Net(M.load_u2net_weights(MC.state_dict("u2netp")), DEV)
    return _NETS["u2netp"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _video(T, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    video = 120 + 80 * np.sin(7 * xx[None, :, :, None] + np.arange(3)[None, None, None, :] + np.arange(T)[:, None, None, None]) * np.cos(5 * yy)[None, :, :, None]
    return np.clip(np.rint(video + rng.normal(0, 15, video.shape)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the strided convolution alone
@pytest.mark.parametrize("images,H,W,cin,cout", CONV_SHAPES)
def test_conv3x3_s2_bits_and_values(images, H, W, cin, cout):
    """the bits of the stride-1 kernel at every second pixel, and every element against fp64 conv2d(stride=2, padding=1) under the
    derived bound with K = 9 Cin"""
    g = torch.Generator().manual_seed(images * 1000 + H * 100 + W * 10 + cin + cout)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = 0.05 * torch.randn((cout,), generator=g)
    x = torch.randn((images, cin, H, W), generator=g) + 0.5                     # a non-zero mean: a wrong border shows
    wp, bd = ops.pack_conv_weight(w).to(DEV), b.to(DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    s = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    bound = 2 * (9 * cin + 1) * EB.U32 * (F.conv2d(x.double().abs(), w.double().abs(), stride=2, padding=1) + b.double().abs().reshape(1, -1, 1, 1))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for relu in (False, True):
        out = ops.conv3x3_s2(xd, wp, bd, relu=relu)
        assert out.shape == (images, Ho, Wo, cout) and out.dtype == torch.float32 and out.is_contiguous()
        assert torch.equal(out, ops.conv3x3_ex(xd, wp, bd, relu=relu)[:, ::2, ::2])
        ref = s.clamp_min(0) if relu else s
        r = EB.assert_within(out, ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1), f"conv3x3_s2 {(images, H, W, cin, cout)} relu={relu}")
        print(f"conv3x3_s2 {(images, H, W, cin, cout)} relu={relu}: worst err / bound {r:.3g}")
    assert torch.equal(ops.conv3x3_s2(xd, wp, bd), ops.conv3x3_s2(xd, wp, bd, relu=False))         # the default is the stem's: no activation
    into = torch.full((images, Ho, Wo, cout), float("nan"), device=DEV)
    assert ops.conv3x3_s2(xd, wp, bd, out=into) is into and torch.equal(into, ops.conv3x3_s2(xd, wp, bd))


def test_conv3x3_s2_refusals_on_device():
    x = torch.zeros((1, 5, 4, 8), device=DEV)
    wp, b = torch.zeros((ops.conv_kpad(8), 8), device=DEV), torch.zeros((8,), device=DEV)
    with pytest.raises(M324Error, match="wp must be"):
        ops.conv3x3_s2(x, wp[:64], b)
    with pytest.raises(M324Error, match="multiple of 4"):
        ops.conv3x3_s2(x, torch.zeros((ops.conv_kpad(8), 6), device=DEV), torch.zeros((6,), device=DEV))
    with pytest.raises(M324Error, match=r"out must be a contiguous fp32 device tensor \(1, 3, 2, 8\)"):
        ops.conv3x3_s2(x, wp, b, out=torch.zeros((1, 5, 4, 8), device=DEV))


# ------------------------------------------------------------------------------------------------ normalisation and head
def test_normalisation_with_given_constants():
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 200, (4, 37, 41, 3), dtype=np.uint8)
    frames[1] = 0                                                               # an all-black frame: m = 1e-6
    frames[2, 30, 7, 1] = 255
    fd = _dev(frames)
    for mean, std in ((IC.MEAN, IC.STD), ((0.5, 0.25, 0.125), (1.0, 0.3, 2.0))):
        got = ops.matte_prepare(fd, mean=mean, std=std)
        assert got.shape == (4, 37, 41, 4) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), IC.model_prepare(frames, mean, std)), (mean, std)
    assert torch.equal(ops.matte_prepare(fd, mean=M.MEAN, std=M.STD), ops.matte_prepare(fd))
    assert np.array_equal(ops.matte_prepare(fd).cpu().numpy(), MC.model_prepare(frames))
    black = ops.matte_prepare(fd, mean=IC.MEAN, std=IC.STD)[1]
    assert np.array_equal(black[0, 0].cpu().numpy(), np.array([-0.485, -0.456, -0.406, 0.0], dtype=np.float32)) and bool((black == black[0, 0]).all())
    assert torch.equal(isnet().prepare(fd), ops.matte_prepare(fd, mean=IC.MEAN, std=IC.STD)) and torch.equal(u2netp().prepare(fd), ops.matte_prepare(fd))
    for bad in (dict(mean=IC.MEAN), dict(mean=IC.MEAN, std=(1.0, 0.0, 1.0)), dict(mean=(0.1, 0.2), std=IC.STD), dict(mean=IC.MEAN, std=(1.0, float("nan"), 1.0))):
        with pytest.raises(M324Error, match="matte_prepare"):
            ops.matte_prepare(fd, **bad)


@pytest.mark.parametrize("shape,size", [((1, 19, 19, 4), (37, 37)), ((2, 20, 20, 4), (40, 40))])
def test_one_map_head(shape, size):
    g = torch.Generator().manual_seed(shape[1])
    side = (2.0 * torch.randn(shape, generator=g)).to(DEV)
    prob, logit = ops.matte_side(side, size, want_logits=True)
    assert prob.shape == logit.shape == (shape[0],) + size and prob.dtype == logit.dtype == torch.float32
    assert torch.equal(logit, ops.upsample_bilinear(side, size)[..., 0])
    p_err = np.abs(prob.double().cpu().numpy() - MC.sigmoid64(logit.double().cpu().numpy())).max()
    print(f"matte_side {shape} -> {size}: sigmoid error {p_err:.3g} of {MC.SIGMOID_ERROR:.3g}")
    assert p_err <= MC.SIGMOID_ERROR
    alone, none = ops.matte_side(side, size)
    assert none is None and torch.equal(alone, prob)
    same, same_logit = ops.matte_side(side, shape[1:3], want_logits=True)       # equal sizes: the map itself
    assert torch.equal(same_logit, side[..., 0])
    with pytest.raises(M324Error, match="no smaller than the side map"):
        ops.matte_side(side, (shape[1] - 1, shape[2]))


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("name", list(IC.CASES))
def test_network_against_the_fp64_oracle(name):
    """the logits and all twelve taps inside the recorded gate, each on its own, then the quantised mask under the derived delta"""
    size, T = IC.CASES[name]
    x, ref = IC.reference(name)
    prob, d1, taps = isnet()(_dev(x), return_logits=True, taps=True)
    assert prob.shape == d1.shape == (T, size, size) and prob.dtype == torch.float32 and set(taps) == set(M.ISNET_TAPS) and len(taps) == 12
    got = {n: t.double().cpu().numpy() for n, t in taps.items()}
    got["d1"] = d1.double().cpu().numpy()
    dev, allowed = IC.deviation(got, ref), IC.gate(name)
    print(f"{name}: deviation {np.array2string(dev, precision=2)}; gate {np.array2string(allowed, precision=2)}; "
          f"ratio {np.array2string(dev / allowed, precision=2)}")
    assert (dev <= allowed).all(), (name, dict(zip(IC.TENSORS, dev / allowed)))
    p_err = np.abs(prob.double().cpu().numpy() - MC.sigmoid64(got["d1"])).max()
    assert p_err <= IC.SIGMOID_ERROR, p_err
    assert torch.equal(isnet()(_dev(x)), prob)                                   # the call without logits and taps: the same bits
    q, _ = ops.matte_quantise(prob)
    assert np.array_equal(q.cpu().numpy(), MC.model_quantise(prob.cpu().numpy()))          # step 4 itself: numpy's fp32 arithmetic
    ambiguous, wrong, far = IC.check_quantised(name, q.cpu().numpy())
    print(f"{name}: quantised mask: {100 * ambiguous:.2f} % ambiguous, {wrong} wrong outside the zone, {far} off by more than one level")
    assert ambiguous <= IC.MAX_AMBIGUOUS and wrong == 0 and far == 0


# ------------------------------------------------------------------------------------------------ around the network: exact
def test_everything_around_the_network_is_exact():
    """steps 1 and 2 against the host models; then the GPU's own mask through the host model of steps 5 and 6, and through the framing
    model in the threshold mode of utils/rmbg_for_black_bg.py"""
    T, H, W, size = 3, 53, 71, 40
    video = _video(T, H, W, 5)
    v = _dev(video)
    net = isnet()
    small = M._resize(v, 3, W, H, size, size)
    want_small = FC.model_resize(video, size, size)
    assert np.array_equal(small.cpu().numpy(), want_small)
    x = net.prepare(small)
    assert np.array_equal(x.cpu().numpy(), IC.model_prepare(want_small))
    matte = M.matte_video(v, net, size=size)
    assert matte.alpha.shape == (T, H, W) and matte.mask320.shape == (T, size, size) and matte.alpha.dtype == matte.mask320.dtype == torch.uint8
    assert torch.equal(matte.mask320, ops.matte_quantise(net(x))[0])
    assert int(matte.mask320.max()) == 255 and int(matte.mask320.min()) == 0
    alpha, masked, masks = MC.model_from_mask(matte.mask320.cpu().numpy(), video)
    assert torch.equal(matte.alpha.cpu(), torch.from_numpy(alpha))
    got_masked, got_masks = M.cut_out(v, matte.alpha)
    assert torch.equal(got_masked.cpu(), torch.from_numpy(masked)) and torch.equal(got_masks.cpu(), torch.from_numpy(masks))
    framed = framing.frame_video(v, matte.alpha)                                 # the defaults: threshold at 204, 512 x 512
    want = FC.model_frame(video, alpha)
    assert want is not None and framed is not None
    assert framed.box == want["box"] and framed.placement == want["placement"]
    assert np.array_equal(framed.frames.cpu().numpy(), want["frames"]) and np.array_equal(framed.mask.cpu().numpy(), want["mask"])


def test_exact_properties():
    net = isnet()
    size = 40
    rng = np.random.default_rng(78)
    video = rng.integers(0, 256, (5, 33, 52, 3), dtype=np.uint8)
    video[3] = 97                                                           # a constant frame
    video[4] = 0                                                            # an all-black frame: m = 1e-6
    v = _dev(video)
    whole = M.matte_video(v, net, size=size)
    per_frame = 4 * M.ISNET_FLOATS_PER_FRAME_PIXEL * size * size
    for n in (1, 2, 5):                                                     # one, two and all frames per chunk
        assert M.frames_per_chunk(5, size, n * per_frame, net.floats_per_frame_pixel) == n
        part = M.matte_video(v, net, size=size, max_scratch_bytes=n * per_frame)
        assert torch.equal(part.alpha, whole.alpha) and torch.equal(part.mask320, whole.mask320)
    with pytest.raises(M324Error, match="max_scratch_bytes is 1000"):
        M.matte_video(v, net, size=size, max_scratch_bytes=1000)
    perm = torch.tensor([2, 4, 0, 3, 1], device=DEV)
    moved = M.matte_video(v[perm], net, size=size)
    assert torch.equal(moved.alpha, whole.alpha[perm]) and torch.equal(moved.mask320, whole.mask320[perm])
    again = M.matte_video(v, net, size=size)
    assert torch.equal(again.alpha, whole.alpha) and torch.equal(again.mask320, whole.mask320)
    # a constant input gives a constant network input, but the zero padding still structures the output: the documented path
    # (alpha 0) is the quantiser's, reached with constant probabilities, here those of a constant side map through the head
    prob, _ = ops.matte_side(torch.full((2, 5, 5, 4), 0.5, device=DEV), (9, 11))
    q, minmax = ops.matte_quantise(prob)
    assert not q.any() and bool((minmax[:, 0] == minmax[:, 1]).all())
    alpha = M._resize(q, 1, 11, 9, 52, 33)
    assert alpha.reshape(2, 33, 52).shape == (2, 33, 52) and not alpha.any()
    small = M._resize(v[3:5], 3, 52, 33, size, size)
    assert bool((small[0] == 97).all()) and not small[1].any()
    x = net.prepare(small)
    assert bool((x[0, ..., :3] == _dev((1.0 - np.array(IC.MEAN)).astype(np.float32))).all())       # 97 / 97 = 1
    assert bool((x[1, ..., :3] == _dev((-np.array(IC.MEAN)).astype(np.float32))).all())            # 0 / 1e-6 = 0
    assert int(whole.mask320[0].max()) == 255 and int(whole.mask320[0].min()) == 0
    other = M.ISNet(M.load_isnet_weights(IC.state_dict()), DEV, mean=(0.5, 0.5, 0.5), std=(0.5, 0.25, 1.0))      # the constants are the caller's
    assert torch.equal(other.prepare(small), ops.matte_prepare(small, mean=(0.5, 0.5, 0.5), std=(0.5, 0.25, 1.0)))
    with pytest.raises(M324Error, match="every std above 0"):
        M.ISNet(M.load_isnet_weights(IC.state_dict()), DEV, std=(1.0, 0.0, 1.0))


def test_u2net_through_the_widened_matte_video_gives_its_own_bits():
    """the steps of U2-Net's path strung together by hand, ops.matte_prepare() without constants among them"""
    net = u2netp()
    assert (net.input_size, net.mean, net.std, net.variant) == (320, M.MEAN, M.STD, "u2netp")
    T, H, W, size = 3, 45, 70, 40
    video = _video(T, H, W, 115)
    v = _dev(video)
    x = ops.matte_prepare(M._resize(v, 3, W, H, size, size))
    assert np.array_equal(x.cpu().numpy(), MC.model_prepare(FC.model_resize(video, size, size)))
    mask, _ = ops.matte_quantise(net(x))
    alpha = M._resize(mask, 1, size, size, W, H).reshape(T, H, W)
    matte = M.matte_video(v, net, size=size)
    assert torch.equal(matte.mask320, mask) and torch.equal(matte.alpha, alpha)
    got_masked, got_masks = M.segment_foreground_with_u2net(v[:1], isnet())    # either network, each at its own size: ISNet at 1024
    want_masked, want_masks = M.cut_out(v[:1], M.matte_video(v[:1], isnet(), size=1024).alpha)
    assert got_masked.shape == (1, H, W, 3) and torch.equal(got_masked, want_masked) and torch.equal(got_masks, want_masks)


def test_command_line_infers_the_network_and_frames_by_threshold(tmp_path, capsys):
    """a tiny .npy clip through main() with ISNet weights saved to disk: the network is read from the file's keys, and --frame with
    --frame_mode threshold writes frame_video's default mode"""
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.linspace(-1, 1, 36), np.linspace(-1, 1, 48), indexing="ij")
    blob = np.exp(-(xx ** 2 + yy ** 2) / 0.2)
    clip = np.clip(40 + 180 * blob[None, :, :, None] + rng.normal(0, 10, (2, 36, 48, 3)), 0, 255).astype(np.uint8)
    np.save(tmp_path / "clip.npy", clip)
    torch.save(IC.state_dict(), tmp_path / "isnet.pth")
    written = M.main(["--video", str(tmp_path / "clip.npy"), "--weights", str(tmp_path / "isnet.pth"), "--out", str(tmp_path / "out"),
                      "--size", "40", "--frame", "64", "--frame_mode", "threshold"])
    assert "2 frames of 48 x 36, isnet at 40" in capsys.readouterr().out
    v = _dev(clip)
    matte = M.matte_video(v, isnet(), size=40)
    alpha, masked, masks = MC.model_from_mask(matte.mask320.cpu().numpy(), clip)
    assert np.array_equal(np.load(written["alpha.npy"]), alpha) and np.array_equal(np.load(written["masked_frames.npy"]), masked)
    assert np.array_equal(np.load(written["masks.npy"]), masks)
    want = FC.model_frame(clip, alpha, size=64)
    if want is None:
        assert set(written) == {"alpha.npy", "masked_frames.npy", "masks.npy"}
    else:
        assert np.array_equal(np.load(written["framed.npy"]), want["frames"]) and np.array_equal(np.load(written["framed_mask.npy"]), want["mask"])
