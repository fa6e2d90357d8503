"""Matting on the GPU: ops.conv3x3_ex element by element against fp64 under a derived bound, the pool exactly, the upsample under its
bound, U2-Net (logits and every tap) against the fp64 oracle inside the recorded gate, the quantised mask, everything behind it bit
for bit against the host model, the exact properties and the command line (tests/ERROR_BOUNDS_MATTING.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import error_bounds as EB
import framing_cases as FC
import matting_cases as MC
from motion324_amd import framing, ops
from motion324_amd import matting as M
from motion324_amd import perceptual as P
from motion324_amd.lib import M324Error

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(1, 1), (5, 7), (9, 17), (16, 24)]       # at (5, 7) with d = 8 every off-centre tap is outside; at (9, 17) some are

_NETS = {}


def net_of(variant):
    if variant not in _NETS:
        _NETS[variant] = M.U2Net(M.load_u2net_weights(MC.state_dict(variant)), DEV)
    return _NETS[variant]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the convolution alone
@pytest.mark.parametrize("dilation", [1, 2, 4, 8])
@pytest.mark.parametrize("cout", [4, 16, 32, 64, 256])
@pytest.mark.parametrize("ca,cb", [(4, 0), (16, 16), (64, 0), (64, 64), (512, 512)])
def test_conv3x3_ex_elementwise(ca, cb, cout, dilation):
    """every size and batch of the table, ReLU and residual on and off, against the fp64 convolution of the same fp32 data"""
    cin = ca + cb
    g = torch.Generator().manual_seed(ca * 7 + cb * 5 + cout * 3 + dilation)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = 0.05 * torch.randn((cout,), generator=g)
    wp, bd = P.pack_conv_weight(w).to(DEV), b.to(DEV)
    to_nhwc = lambda t: t.permute(0, 2, 3, 1)
    worst = 0.0
    for H, W in SIZES:
        for images in (1, 3):
            x = torch.randn((images, cin, H, W), generator=g) + 0.5         # a non-zero mean: a wrong border shows
            res = torch.randn((images, cout, H, W), generator=g)
            s = F.conv2d(x.double(), w.double(), b.double(), padding=dilation, dilation=dilation)
            bound = 2 * (9 * cin + 1) * EB.U32 * (F.conv2d(x.double().abs(), w.double().abs(), padding=dilation, dilation=dilation)
                                                  + b.double().abs().reshape(1, -1, 1, 1))
            nhwc = to_nhwc(x).contiguous().to(DEV)
            xa, xb = (nhwc[..., :ca].contiguous(), nhwc[..., ca:].contiguous()) if cb else (nhwc, None)
            rd = to_nhwc(res).contiguous().to(DEV)
            what = f"conv3x3_ex {ca}+{cb}->{cout} d{dilation} {H}x{W} x{images}"
            outs = {}
            for relu in (False, True):
                for with_res in (False, True):
                    ref = s.clamp_min(0) if relu else s
                    bnd = bound
                    if with_res:
                        ref = ref + res.double()
                        bnd = bound + EB.U32 * res.double().abs()
                    out = ops.conv3x3_ex(xa, wp, bd, b=xb, dilation=dilation, relu=relu, res=rd if with_res else None)
                    assert out.shape == (images, H, W, cout) and out.dtype == torch.float32
                    worst = max(worst, EB.assert_within(out, to_nhwc(ref), to_nhwc(bnd), f"{what} relu={relu} res={with_res}"))
                    outs[relu, with_res] = out
            assert torch.equal(outs[True, False], outs[False, False].clamp_min(0))
            assert torch.equal(outs[True, True], outs[True, False] + rd) and torch.equal(outs[False, True], outs[False, False] + rd)
            if cb:                                                          # the concatenation, materialised: the same bits
                assert torch.equal(ops.conv3x3_ex(nhwc, wp, bd, dilation=dilation, relu=False), outs[False, False])
            if dilation == 1 and cout % 32 == 0:                            # the old kernel wherever its contract allows the call
                assert torch.equal(ops.conv3x3(nhwc, wp, bd, relu=False), outs[False, False])
                assert torch.equal(ops.conv3x3(nhwc, wp, bd), outs[True, False])
    print(f"conv3x3_ex {ca}+{cb}->{cout} d{dilation}: worst err / bound {worst:.3g}")


@pytest.mark.parametrize("cout,images,alone,batch", [(128, 17, 64, 128), (48, 33, 64, 64), (16, 5, 32, 32)])
def test_conv3x3_ex_bits_do_not_depend_on_the_tile_or_the_batch(cout, images, alone, batch):
    """Cout = 128 takes the 64-wide tile for a few pixels and the 128-wide one once the grid is full; an image's bits are the same in
    both, and in every tile alone or in a batch.  63 x 65 pixels: no multiple of the tile"""
    g = torch.Generator().manual_seed(9 + cout)
    w = torch.randn((cout, 12, 3, 3), generator=g) * 0.1
    wp, bd = P.pack_conv_weight(w).to(DEV), torch.randn((cout,), generator=g).to(DEV)
    x = (torch.randn((images, 63, 65, 12), generator=g) + 0.5).to(DEV)
    xa, xb = x[..., :8].contiguous(), x[..., 8:].contiguous()
    assert ops.conv3x3_ex_tile(1, 63, 65, cout) == alone and ops.conv3x3_ex_tile(images, 63, 65, cout) == batch
    whole = ops.conv3x3_ex(xa, wp, bd, b=xb, dilation=2)
    for i in (0, images // 2, images - 1):
        assert torch.equal(ops.conv3x3_ex(xa[i:i + 1].contiguous(), wp, bd, b=xb[i:i + 1].contiguous(), dilation=2), whole[i:i + 1])
    assert torch.equal(ops.conv3x3_ex(xa, wp, bd, b=xb, dilation=2), whole)
    ref = F.conv2d(x[:2].cpu().permute(0, 3, 1, 2).double(), w.double(), bd.cpu().double(), padding=2, dilation=2).clamp_min(0).permute(0, 2, 3, 1)
    bound = 2 * (9 * 12 + 1) * EB.U32 * (F.conv2d(x[:2].cpu().permute(0, 3, 1, 2).double().abs(), w.double().abs(), padding=2, dilation=2)
                                         + bd.cpu().double().abs().reshape(1, -1, 1, 1)).permute(0, 2, 3, 1)
    EB.assert_within(whole[:2], ref, bound, f"conv3x3_ex 8+4->{cout} in the batch tile {batch}")


def test_conv3x3_ex_refusals_on_device():
    x = torch.zeros((1, 4, 4, 8), device=DEV)
    wp, b = torch.zeros((ops.conv_kpad(8), 8), device=DEV), torch.zeros((8,), device=DEV)
    with pytest.raises(M324Error, match="wp must be"):
        ops.conv3x3_ex(x, wp, b, b=x)
    with pytest.raises(M324Error, match="does not match"):
        ops.conv3x3_ex(x, wp, b, b=torch.zeros((1, 4, 5, 8), device=DEV))
    with pytest.raises(M324Error, match="dilation"):
        ops.conv3x3_ex(x, wp, b, dilation=0)
    with pytest.raises(M324Error, match="res must be"):
        ops.conv3x3_ex(x, wp, b, res=torch.zeros((1, 4, 4, 4), device=DEV))
    with pytest.raises(M324Error, match="multiple of 4"):
        ops.conv3x3_ex(x, torch.zeros((ops.conv_kpad(8), 6), device=DEV), torch.zeros((6,), device=DEV))


# ------------------------------------------------------------------------------------------------ pool and upsample
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (10, 10)])
def test_maxpool2x2_ceil_is_exact(H, W):
    g = torch.Generator().manual_seed(H * 13 + W)
    x = torch.randn((3, 8, H, W), generator=g) - 1.0                          # mostly negative: a zero-padded window would win
    out = ops.maxpool2x2_ceil(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    want = F.max_pool2d(x, 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    assert out.shape == (3, (H + 1) // 2, (W + 1) // 2, 8) and torch.equal(out.cpu(), want)


@pytest.mark.parametrize("src,dst", [(2, 3), (3, 5), (5, 10), (10, 20), (1, 4)])
def test_upsample_bilinear_against_fp64(src, dst):
    """both axes at once, with another transition on the second axis; the bound is derived in tests/ERROR_BOUNDS_MATTING.md"""
    src_w, dst_w = {2: (3, 5), 3: (5, 10), 5: (10, 20), 10: (2, 3), 1: (1, 4)}[src]
    g = torch.Generator().manual_seed(src * 31 + dst)
    x = torch.randn((2, 8, src, src_w), generator=g) + 0.5
    out = ops.upsample_bilinear(x.permute(0, 2, 3, 1).contiguous().to(DEV), (dst, dst_w))
    ref = F.interpolate(x.double(), size=(dst, dst_w), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    bound = torch.full_like(ref, (6 * (src + src_w + 2) + 10) * EB.U32 * float(x.abs().max()))
    r = EB.assert_within(out, ref, bound, f"upsample {src}x{src_w} -> {dst}x{dst_w}")
    print(f"upsample {src}x{src_w} -> {dst}x{dst_w}: worst err / bound {r:.3g}")
    same = ops.upsample_bilinear(out, (dst, dst_w))
    assert torch.equal(same, out)                                             # equal sizes: the identity


@pytest.mark.parametrize("H,W", [(1, 1), (37, 37), (61, 67), (97, 131)])
def test_per_frame_reductions_across_their_runs(H, W):
    """the byte maximum and the fp32 extremes are reduced in runs of a frame (one run at 37 x 37, several above): the extreme planted
    in the first place, the last place and in the middle is found, frame by frame, and the results are numpy's"""
    rng = np.random.default_rng(H * W)
    frames = rng.integers(0, 180, (3, H, W, 3), dtype=np.uint8)
    prob = rng.uniform(0.2, 0.8, (3, H, W)).astype(np.float32)
    for t, at in enumerate((0, H * W - 1, (H * W) // 2)):
        frames[t].reshape(-1)[3 * at + 2 if at else 0] = 181 + t
        prob[t].reshape(-1)[at] = 0.9 + 0.01 * t
        prob[t].reshape(-1)[H * W - 1 - at] = 0.1 - 0.01 * t if H * W > 1 else prob[t].reshape(-1)[at]
    assert np.array_equal(ops.matte_prepare(_dev(frames)).cpu().numpy(), MC.model_prepare(frames))
    q, minmax = ops.matte_quantise(_dev(prob))
    assert np.array_equal(minmax.cpu().numpy(), np.stack([prob.min(axis=(1, 2)), prob.max(axis=(1, 2))], axis=1))
    assert np.array_equal(q.cpu().numpy(), MC.model_quantise(prob))


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("name", list(MC.CASES))
def test_network_against_the_fp64_oracle(name):
    """the logits and all eleven taps inside the recorded gate, then the quantised mask under the derived delta"""
    variant, size, T = MC.CASES[name]
    x, ref = MC.reference(name)
    prob, d0, taps = net_of(variant)(_dev(x), return_logits=True, taps=True)
    assert prob.shape == d0.shape == (T, size, size) and prob.dtype == torch.float32 and set(taps) == set(M.TAPS)
    got = {n: t.double().cpu().numpy() for n, t in taps.items()}
    got["d0"] = d0.double().cpu().numpy()
    dev, allowed = MC.deviation(got, ref), MC.gate(name)
    print(f"{name}: deviation {np.array2string(dev, precision=2)}; gate {np.array2string(allowed, precision=2)}; "
          f"ratio {np.array2string(dev / allowed, precision=2)}")
    assert (dev <= allowed).all(), (name, dict(zip(MC.TENSORS, dev / allowed)))
    p_err = np.abs(prob.double().cpu().numpy() - MC.sigmoid64(got["d0"])).max()
    assert p_err <= MC.SIGMOID_ERROR, p_err
    q, minmax = ops.matte_quantise(prob)
    assert torch.equal(minmax, torch.stack([prob.amin(dim=(1, 2)), prob.amax(dim=(1, 2))], dim=1))
    assert np.array_equal(q.cpu().numpy(), MC.model_quantise(prob.cpu().numpy()))          # step 4 itself: numpy's fp32 arithmetic
    ambiguous, wrong, far = MC.check_quantised(name, q.cpu().numpy())
    print(f"{name}: quantised mask: {100 * ambiguous:.2f} % ambiguous, {wrong} wrong outside the zone, {far} off by more than one level")
    assert ambiguous <= MC.MAX_AMBIGUOUS and wrong == 0 and far == 0


# ------------------------------------------------------------------------------------------------ around the network: exact
@pytest.mark.parametrize("H,W,size,T", [(45, 70, 40, 3), (320, 200, 320, 2)])
def test_everything_around_the_network_is_exact(H, W, size, T):
    """steps 1 and 2 against the host model; then the GPU's own mask through the host model of steps 5 and 6.  320 x 200 at size 320 is
    the pass Pillow skips"""
    rng = np.random.default_rng(H + W)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    video = 120 + 80 * np.sin(7 * xx[None, :, :, None] + np.arange(3)[None, None, None, :] + np.arange(T)[:, None, None, None]) * np.cos(5 * yy)[None, :, :, None]
    video = np.clip(np.rint(video + rng.normal(0, 15, video.shape)), 0, 255).astype(np.uint8)
    v = _dev(video)
    small = M._resize(v, 3, W, H, size, size)
    want_small = FC.model_resize(video, size, size)
    assert np.array_equal(small.cpu().numpy(), want_small)
    x = ops.matte_prepare(small)
    assert np.array_equal(x.cpu().numpy(), MC.model_prepare(want_small))
    net = net_of("u2netp")
    matte = M.matte_video(v, net, size=size)
    assert matte.alpha.shape == (T, H, W) and matte.mask320.shape == (T, size, size) and matte.alpha.dtype == matte.mask320.dtype == torch.uint8
    assert torch.equal(matte.mask320, ops.matte_quantise(net(x))[0])
    assert int(matte.mask320.max()) == 255 and int(matte.mask320.min()) == 0
    alpha, masked, masks = MC.model_from_mask(matte.mask320.cpu().numpy(), video)
    assert torch.equal(matte.alpha.cpu(), torch.from_numpy(alpha))
    if size == M.SIZE:
        got_masked, got_masks = M.segment_foreground_with_u2net(v, net)
        assert got_masked.dtype == torch.uint8 and got_masked.shape == (T, H, W, 3) and got_masks.dtype == torch.float32 and got_masks.shape == (T, H, W, 1)
        assert torch.equal(got_masked.cpu(), torch.from_numpy(masked)) and torch.equal(got_masks.cpu(), torch.from_numpy(masks))
        host_masked, _ = M.segment_foreground_with_u2net(video, net)        # a host array goes to the network's device
        assert torch.equal(host_masked, got_masked)
    else:
        table = _dev(M.cutout_table())
        got_masked = ops.frame_mask(v, matte.alpha, mode="soft", table=table, want_mask=False)[0]
        assert torch.equal(got_masked.cpu(), torch.from_numpy(masked))
        assert torch.equal(_dev(M.mask_levels())[matte.alpha.long()].unsqueeze(-1).cpu(), torch.from_numpy(masks))


def test_exact_properties():
    net = net_of("u2netp")
    size = 40
    rng = np.random.default_rng(77)
    video = rng.integers(0, 256, (5, 33, 52, 3), dtype=np.uint8)
    video[3] = 97                                                           # a constant frame: ma == mi
    video[4] = 0                                                            # an all-black frame: m = 1e-6
    v = _dev(video)
    whole = M.matte_video(v, net, size=size)
    per_frame = 4 * M.FLOATS_PER_FRAME_PIXEL * size * size
    for n in (1, 2, 5):                                                     # one, two and all frames per chunk
        assert M.frames_per_chunk(5, size, n * per_frame) == n
        part = M.matte_video(v, net, size=size, max_scratch_bytes=n * per_frame)
        assert torch.equal(part.alpha, whole.alpha) and torch.equal(part.mask320, whole.mask320)
    with pytest.raises(M324Error, match="max_scratch_bytes is 1000"):
        M.matte_video(v, net, size=size, max_scratch_bytes=1000)
    perm = torch.tensor([2, 4, 0, 3, 1], device=DEV)
    moved = M.matte_video(v[perm], net, size=size)
    assert torch.equal(moved.alpha, whole.alpha[perm]) and torch.equal(moved.mask320, whole.mask320[perm])
    again = M.matte_video(v, net, size=size)
    assert torch.equal(again.alpha, whole.alpha) and torch.equal(again.mask320, whole.mask320)
    # a constant input gives a constant network input, but the zero padding still structures the output: the documented path is
    # the quantiser's, reached with constant probabilities
    q, minmax = ops.matte_quantise(torch.full((2, 7, 9), 0.625, device=DEV))
    assert not q.any() and torch.equal(minmax, torch.full((2, 2), 0.625, device=DEV))
    small = M._resize(v[3:5], 3, 52, 33, size, size)
    assert bool((small[0] == 97).all()) and not small[1].any()
    x = ops.matte_prepare(small)
    assert np.array_equal(x.cpu().numpy(), MC.model_prepare(small.cpu().numpy()))
    black = np.array([-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, 0.0]).astype(np.float32)     # 0 / 1e-6 = 0
    assert np.array_equal(x[1, 0, 0].cpu().numpy(), black) and bool((x[1] == x[1, 0, 0]).all())
    assert bool((x[0, ..., :3] == _dev(((1.0 - np.array(M.MEAN)) / np.array(M.STD)).astype(np.float32))).all())     # 97 / 97 = 1
    assert int(whole.mask320[0].max()) == 255 and int(whole.mask320[0].min()) == 0


def test_module_refusals_on_device():
    net = net_of("u2netp")
    with pytest.raises(M324Error, match="must be on"):
        net(torch.zeros((1, 8, 8, 4)))
    with pytest.raises(M324Error, match=r"fp32 NHWC \[T,H,W,4\]"):
        net(torch.zeros((1, 8, 8, 3), device=DEV))
    with pytest.raises(M324Error, match="size must be"):
        M.matte_video(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV), net, size=0)
    with pytest.raises(M324Error, match="needs device="):
        M.matte_video(np.zeros((1, 8, 8, 3), np.uint8), net)


def test_command_line(tmp_path, capsys):
    """a tiny .npy clip through main() with u2netp weights saved to disk: the files it writes, and --frame against frame_video"""
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.linspace(-1, 1, 36), np.linspace(-1, 1, 48), indexing="ij")
    blob = np.exp(-(xx ** 2 + yy ** 2) / 0.2)
    clip = np.clip(40 + 180 * blob[None, :, :, None] + rng.normal(0, 10, (2, 36, 48, 3)), 0, 255).astype(np.uint8)
    np.save(tmp_path / "clip.npy", clip)
    torch.save(MC.state_dict("u2netp"), tmp_path / "u2netp.pth")
    written = M.main(["--video", str(tmp_path / "clip.npy"), "--weights", str(tmp_path / "u2netp.pth"), "--out", str(tmp_path / "out"),
                      "--size", "40", "--frame", "64"])
    assert "2 frames of 48 x 36, u2netp at 40" in capsys.readouterr().out
    net = net_of("u2netp")
    v = _dev(clip)
    matte = M.matte_video(v, net, size=40)
    alpha, masked, masks = MC.model_from_mask(matte.mask320.cpu().numpy(), clip)
    assert np.array_equal(np.load(written["alpha.npy"]), matte.alpha.cpu().numpy()) and np.array_equal(np.load(written["alpha.npy"]), alpha)
    assert np.array_equal(np.load(written["masked_frames.npy"]), masked)
    got_masks = np.load(written["masks.npy"])
    assert got_masks.dtype == np.float32 and np.array_equal(got_masks, masks)
    framed = framing.frame_video(v, matte.alpha, size=64, mode="soft")
    assert framed is not None and set(written) == {"alpha.npy", "masked_frames.npy", "masks.npy", "framed.npy", "framed_mask.npy"}
    assert np.array_equal(np.load(written["framed.npy"]), framed.frames.cpu().numpy()) and np.load(written["framed.npy"]).shape == (2, 64, 64, 3)
    assert np.array_equal(np.load(written["framed_mask.npy"]), framed.mask.cpu().numpy())
