"""FVD on the GPU: the 3D convolution, the 3D max-pool, the prepare kernel and the head against fp64 under derived bounds and in
their exact properties, the I3D trunk end to end against the recorded fp64 values, and the clip rule and the command line
(tests/ERROR_BOUNDS_FVD.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fvd_cases as FC
from error_bounds import U32
from motion324_amd import fvd as V
from motion324_amd import ops
from motion324_amd.lib import M324Error

pytestmark = pytest.mark.gpu

VOLUMES = ((1, 1, 1), (2, 3, 5), (5, 7, 6), (4, 8, 8))         # the odd sizes exercise SAME's asymmetry
# (box, Cin, Cout): the large pairs stay off the 7 x 7 x 7 box (I3D has no such layer)
CONV_CASES = ((7, 4, 64), (3, 16, 48), (3, 24, 64), (3, 96, 208), (3, 192, 384), (3, 16, 24), (1, 16, 48), (1, 24, 64), (1, 96, 208),
              (1, 832, 384), (1, 16, 24))


def _dev(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).to("cuda")


def _ncdhw(x):
    return x.permute(0, 4, 1, 2, 3)


def _ndhwc(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _front_pad(x, box, stride, padding):
    """x [N,C,T,H,W] zero padded in front by `padding` and behind by what the SAME output size ceil(n / s) needs"""
    pads = []
    for n, s, p in zip(x.shape[2:], stride, padding):
        out = -(-n // s)
        pads.append((p, max((out - 1) * s + box - p - n, 0)))
    return F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))


def conv_reference(x, w, b, stride, padding=None):
    """(ref, bound) fp64 NDHWC of the convolution of x fp32 NDHWC (CPU) with w [Cout,Cin,k,k,k], b: the bound is
    2 (K + 1) U32 (|x| (*) |w| + |b|)"""
    box = w.shape[2]
    if padding is None:
        padding = tuple(ops.same_padding(n, box, s)[0] for n, s in zip(x.shape[1:4], stride))
    xd, wd, bd = _ncdhw(x).double(), w.double(), b.double()
    sizes = tuple(-(-n // s) for n, s in zip(x.shape[1:4], stride))
    ref = F.conv3d(_front_pad(xd, box, stride, padding), wd, bd, stride=stride)[:, :, :sizes[0], :sizes[1], :sizes[2]]
    mag = F.conv3d(_front_pad(xd.abs(), box, stride, padding), wd.abs(), bd.abs(), stride=stride)[:, :, :sizes[0], :sizes[1], :sizes[2]]
    K = box ** 3 * w.shape[1]
    return _ndhwc(ref), 2 * (K + 1) * U32 * _ndhwc(mag)


def _weights(g, box, cin, cout):
    w = torch.randn((cout, cin, box, box, box), generator=g) * (2.0 / (box ** 3 * cin)) ** 0.5
    return w, 0.1 * torch.randn((cout,), generator=g)


# ------------------------------------------------------------------------------------------------ conv3d, element by element
@pytest.mark.parametrize("box,cin,cout", CONV_CASES)
def test_conv3d_against_fp64(box, cin, cout):
    g = torch.Generator().manual_seed(100 * box + cin + cout)
    w, b = _weights(g, box, cin, cout)
    wp, bd = _dev(ops.pack_conv3d_weight(w)), _dev(b)
    combos = [(vol, stride) for vol in VOLUMES for stride in ((1, 1, 1), (2, 2, 2))] + [((5, 7, 6), (1, 2, 2)), ((2, 3, 5), (2, 1, 2))]
    for i, (vol, stride) in enumerate(combos):
        batch = 3 if i % 2 else 1
        x = torch.randn((batch,) + vol + (cin,), generator=g)
        ref, bound = conv_reference(x, w, b, stride)
        out = ops.conv3d(_dev(x), wp, bd, box=box, stride=stride, relu=False).cpu().double()
        assert out.shape == ref.shape, (vol, stride, out.shape, ref.shape)
        err = (out - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"conv3d box {box} {cin}->{cout} vol {vol} stride {stride} batch {batch}: worst error / bound {worst:.3f}")
        assert (err <= bound).all(), (vol, stride, batch, worst)
        out = ops.conv3d(_dev(x), wp, bd, box=box, stride=stride, relu=True).cpu().double()
        assert ((out - ref.clamp_min(0)).abs() <= bound).all(), (vol, stride, batch)


def test_conv3d_three_channel_stem_is_the_padded_four_channel_one():
    """pack_conv3d_weight pads Cin 3 to 4 with zero rows: whatever the fourth input channel holds, it does not count"""
    g = torch.Generator().manual_seed(11)
    w, b = _weights(g, 7, 3, 64)
    x = torch.randn((2, 5, 9, 8, 4), generator=g)
    ref, bound = conv_reference(x[..., :3].contiguous(), w, b, (2, 2, 2))
    out = ops.conv3d(_dev(x), _dev(ops.pack_conv3d_weight(w)), _dev(b), box=7, stride=(2, 2, 2), relu=False).cpu().double()
    assert ((out - ref).abs() <= bound).all()


def test_conv3d_explicit_front_padding():
    """the front padding is an argument: any value in 0..k - 1, not only SAME's"""
    g = torch.Generator().manual_seed(12)
    w, b = _weights(g, 3, 16, 48)
    x = torch.randn((2, 4, 5, 6, 16), generator=g)
    for stride, padding in (((1, 1, 1), (0, 2, 1)), ((2, 2, 2), (2, 0, 0)), ((2, 1, 2), (1, 1, 1))):
        ref, bound = conv_reference(x, w, b, stride, padding)
        out = ops.conv3d(_dev(x), _dev(ops.pack_conv3d_weight(w)), _dev(b), box=3, stride=stride, padding=padding, relu=False).cpu().double()
        assert out.shape == ref.shape and ((out - ref).abs() <= bound).all(), (stride, padding)


# ------------------------------------------------------------------------------------------------ conv3d, exact properties
@pytest.fixture(scope="module")
def layer():
    """a 3 x 3 x 3 layer 96 -> 208 (two ragged 128-wide tiles, more than one 128-voxel tile) and its input, on the device"""
    g = torch.Generator().manual_seed(21)
    w, b = _weights(g, 3, 96, 208)
    return _dev(torch.randn((3, 5, 7, 6, 96), generator=g)), _dev(ops.pack_conv3d_weight(w)), _dev(b)


def test_conv3d_relu_is_the_clamp_of_the_plain_output(layer):
    x, wp, b = layer
    assert torch.equal(ops.conv3d(x, wp, b, box=3, relu=True), ops.conv3d(x, wp, b, box=3, relu=False).clamp_min(0))


@pytest.mark.parametrize("box,cin,cout", ((7, 4, 64), (3, 96, 208), (1, 96, 208)))
def test_conv3d_stride_2_is_every_second_voxel_of_stride_1(box, cin, cout):
    g = torch.Generator().manual_seed(22 + box)
    w, b = _weights(g, box, cin, cout)
    wp, b = _dev(ops.pack_conv3d_weight(w)), _dev(b)
    for vol in ((5, 7, 6), (4, 8, 8), (2, 3, 5)):
        x = _dev(torch.randn((2,) + vol + (cin,), generator=g))
        for stride in ((2, 2, 2), (1, 2, 2), (2, 1, 1)):
            padding = tuple(ops.same_padding(n, box, s)[0] for n, s in zip(vol, stride))
            full = ops.conv3d(x, wp, b, box=box, stride=(1, 1, 1), padding=padding)
            assert torch.equal(ops.conv3d(x, wp, b, box=box, stride=stride, padding=padding), full[:, ::stride[0], ::stride[1], ::stride[2]]), (vol, stride)


def test_conv3d_sample_does_not_depend_on_its_batch_position(layer):
    x, wp, b = layer
    whole = ops.conv3d(x, wp, b, box=3, stride=(1, 2, 2))
    for i in range(x.shape[0]):
        assert torch.equal(ops.conv3d(x[i:i + 1].contiguous(), wp, b, box=3, stride=(1, 2, 2))[0], whole[i])
    assert torch.equal(ops.conv3d(x.flip(0).contiguous(), wp, b, box=3, stride=(1, 2, 2)), whole.flip(0))


def test_conv3d_bits_do_not_depend_on_the_tile(layer):
    x, wp, b = layer
    auto = ops.conv3d(x, wp, b, box=3)
    for tile in (32, 64, 128):
        assert torch.equal(ops.conv3d(x, wp, b, box=3, tile=tile), auto), tile
    assert ops.conv3d_tile(10 ** 6, 208) == 128 and ops.conv3d_tile(630, 208) == 64 and ops.conv3d_tile(10 ** 6, 24) == 32


def test_conv3d_slice_output_leaves_the_other_channels_alone(layer):
    x, wp, b = layer
    dense = ops.conv3d(x, wp, b, box=3)
    wide = torch.full(tuple(dense.shape[:4]) + (256,), -7.5, device="cuda")
    got = ops.conv3d(x, wp, b, box=3, out=wide[..., 24:232])
    assert got.data_ptr() == wide[..., 24:232].data_ptr()
    assert torch.equal(wide[..., 24:232], dense)
    assert (wide[..., :24] == -7.5).all() and (wide[..., 232:] == -7.5).all()
    with pytest.raises(M324Error, match="out must be"):
        ops.conv3d(x, wp, b, box=3, out=wide[..., :200])
    with pytest.raises(M324Error, match="aligned"):
        ops.conv3d(x, wp, b, box=3, out=wide[..., 2:210])


def test_conv3d_slice_input_equals_its_contiguous_copy(layer):
    x, wp, b = layer
    wide = torch.randn(tuple(x.shape[:4]) + (160,), device="cuda")
    wide[..., 32:128] = x
    assert torch.equal(ops.conv3d(wide[..., 32:128], wp, b, box=3), ops.conv3d(x, wp, b, box=3))
    with pytest.raises(M324Error, match="dense NDHWC"):
        ops.conv3d(wide[:, :, ::2, :, 32:128], wp, b, box=3)


def test_conv3d_repeats_bit_for_bit(layer):
    x, wp, b = layer
    assert torch.equal(ops.conv3d(x, wp, b, box=3), ops.conv3d(x, wp, b, box=3))


def test_conv3d_refusals_on_the_device(layer):
    x, wp, b = layer
    with pytest.raises(M324Error, match=r"wp must be \[2592,Cout\]"):
        ops.conv3d(x, wp[:96], b, box=3)
    with pytest.raises(M324Error, match="multiple of 8"):
        ops.conv3d(x, wp[:, :12].contiguous(), b[:12].contiguous(), box=3)
    with pytest.raises(M324Error, match="stride is 1 or 2"):
        ops.conv3d(x, wp, b, box=3, stride=(1, 3, 1))
    with pytest.raises(M324Error, match="front padding"):
        ops.conv3d(x, wp, b, box=3, padding=(1, 3, 1))
    with pytest.raises(M324Error, match="fp32 NDHWC"):
        ops.conv3d(x.double(), wp, b, box=3)
    with pytest.raises(M324Error, match="tile is"):
        ops.conv3d(x, wp, b, box=3, tile=48)


# ------------------------------------------------------------------------------------------------ maxpool3d
def _pool_reference(x, window, stride):
    return _ndhwc(FC._pool(_ncdhw(x), window, stride))


@pytest.mark.parametrize("window,stride", (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((2, 2, 2), (2, 2, 2)),
                                           ((3, 3, 3), (1, 2, 1)), ((2, 2, 2), (1, 1, 1))))
def test_maxpool3d_bit_for_bit_on_mostly_negative_data(window, stride):
    """padding is excluded from the maximum: on negative data a zero-padded pool would return zeros at the border"""
    g = torch.Generator().manual_seed(31)
    for vol in VOLUMES + ((3, 9, 4), (6, 6, 6)):
        x = torch.randn((2,) + vol + (20,), generator=g) - 2.0
        assert torch.equal(ops.maxpool3d(_dev(x), window, stride).cpu(), _pool_reference(x, window, stride)), vol


def test_maxpool3d_slice_output_and_refusals():
    g = torch.Generator().manual_seed(32)
    x = torch.randn((2, 5, 7, 6, 16), generator=g) - 1.0
    want = _pool_reference(x, (3, 3, 3), (2, 2, 2))
    wide = torch.full(tuple(want.shape[:4]) + (32,), 3.25, device="cuda")
    ops.maxpool3d(_dev(x), (3, 3, 3), (2, 2, 2), out=wide[..., 8:24])
    assert torch.equal(wide[..., 8:24].cpu(), want) and (wide[..., :8] == 3.25).all() and (wide[..., 24:] == 3.25).all()
    with pytest.raises(M324Error, match="window"):
        ops.maxpool3d(_dev(x), (3, 3, 1), (1, 1, 1))
    with pytest.raises(M324Error, match="dense NDHWC"):
        ops.maxpool3d(_dev(x)[..., :8], (3, 3, 3), (1, 1, 1))
    with pytest.raises(M324Error, match="multiple of 4"):
        ops.maxpool3d(_dev(torch.zeros(1, 2, 2, 2, 6)), (2, 2, 2), (2, 2, 2))


# ------------------------------------------------------------------------------------------------ fvd_prepare
def _prepare_reference(frames, resolution=224):
    """fp64 [N,T,res,res,3] of uint8 frames [N,T,H,W,3]: preprocess_single in float64"""
    N, T, H, W, _ = frames.shape
    Hr, Wr, y0, x0, Ho, Wo = ops.fvd_geometry(H, W, resolution)
    x = torch.from_numpy(frames).reshape(N * T, H, W, 3).permute(0, 3, 1, 2).double() / 255.0
    x = F.interpolate(x, size=(Hr, Wr), mode="bilinear", align_corners=False)[:, :, y0:y0 + Ho, x0:x0 + Wo]
    return ((x - 0.5) * 2).permute(0, 2, 3, 1).reshape(N, T, Ho, Wo, 3)


@pytest.mark.parametrize("H,W", ((512, 512), (224, 224), (48, 80), (80, 48)))
def test_fvd_prepare_against_fp64(H, W):
    rng = np.random.default_rng(H + W)
    frames = rng.integers(0, 256, (1, 2, H, W, 3), dtype=np.uint8)
    out = ops.fvd_prepare(_dev(frames))
    assert tuple(out.shape) == (1, 2, 224, 224, 4) and not out[..., 3].any()
    bound = 2 * (2 * 4 * U32 * max(H, W) + 2 * 10 * U32)
    err = float((out[..., :3].cpu().double() - _prepare_reference(frames)).abs().max())
    print(f"fvd_prepare {H} x {W}: worst error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    floats = _dev(torch.from_numpy(frames).to(torch.float32) / 255.0)        # divided on the host: a true division, as in the kernel
    assert torch.equal(ops.fvd_prepare(floats), out)                     # bytes against the floats built from them
    if (H, W) == (224, 224):                                             # the identity on the bytes
        assert torch.equal(out[..., :3], (floats - 0.5) * 2.0)
    own = ops.fvd_prepare(_dev(frames), None)
    assert tuple(own.shape) == (1, 2, H, W, 4) and torch.equal(own[..., :3], (floats - 0.5) * 2.0)


def test_fvd_prepare_refusals():
    with pytest.raises(M324Error, match=r"uint8 or fp32 \[samples,T,H,W,3\]"):
        ops.fvd_prepare(_dev(torch.zeros(1, 2, 3, 8, 8)))
    with pytest.raises(M324Error, match=r"uint8 or fp32 \[samples,T,H,W,3\]"):
        ops.fvd_prepare(_dev(torch.zeros(1, 2, 8, 8, 3)).double())
    with pytest.raises(M324Error, match="out must be"):
        ops.fvd_prepare(_dev(torch.zeros(1, 2, 8, 8, 3)), 16, out=torch.zeros(1, 2, 16, 16, 3, device="cuda"))


# ------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("T", (2, 4))
def test_i3d_head_against_fp64(T):
    """time steps 1 and 3 behind the (2, hw, hw) window"""
    g = torch.Generator().manual_seed(41 + T)
    hw, C, classes, N = 3, 1024, 400, 3
    x = torch.randn((N, T, hw, hw, C), generator=g).clamp_min(0)
    w, b = torch.randn((C, classes), generator=g) / 32.0, 0.1 * torch.randn((classes,), generator=g)
    out = ops.i3d_head(_dev(x), _dev(w), _dev(b))
    pooled = F.avg_pool3d(_ncdhw(x).double(), (2, hw, hw), stride=1).reshape(N, C, T - 1).permute(0, 2, 1)         # [N, steps, C]
    ref = (pooled @ w.double() + b.double()).mean(1)
    mag = (pooled.abs() @ w.double().abs() + b.double().abs()).mean(1)
    bound = 2 * (2 * hw * hw + 1 + C // 4 + 4 + (T - 1) + 1) * U32 * mag
    err = (out.cpu().double() - ref).abs()
    print(f"i3d_head T {T}: worst error / bound {float((err / bound).max()):.3f}")
    assert tuple(out.shape) == (N, classes) and (err <= bound).all()
    perm = torch.tensor([2, 0, 1])
    assert torch.equal(ops.i3d_head(_dev(x[perm]), _dev(w), _dev(b)), out[perm.cuda()])            # exact under permutation
    assert torch.equal(ops.i3d_head(_dev(x), _dev(w), _dev(b)), out)
    with pytest.raises(M324Error, match="T in 2"):
        ops.i3d_head(_dev(x[:, :1].contiguous()), _dev(w), _dev(b))
    with pytest.raises(M324Error, match="w must be"):
        ops.i3d_head(_dev(x), _dev(w[:512]), _dev(b))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def weights():
    return V.load_i3d_weights(FC.state_dict())


@pytest.fixture(scope="module")
def small_model(weights):
    return V.I3D(weights, "cuda", head_window=(2, 2, 2), resolution=None)


@pytest.mark.parametrize("name", tuple(FC.CASES))
def test_features_and_taps_against_the_recorded_fp64_values(name, weights, small_model):
    """tests/ERROR_BOUNDS_FVD.md: within 8 times the fp32 CPU run's own deviation, per tap and for the 400 features"""
    N, T, H, W, window, resolution = FC.CASES[name]
    model = small_model if window == (2, 2, 2) else V.I3D(weights, "cuda", head_window=window, resolution=resolution)
    feats, taps = model.features(_dev(FC.videos(name)), taps=True)
    assert tuple(feats.shape) == (N, 400) and set(taps) == set(FC.TAPS)
    got = dict({k: v.cpu().numpy() for k, v in taps.items()}, features=feats.cpu().numpy())
    table, outside = FC.golden()[name], []
    for key in FC.KEYS:
        d = table[key].deviation(got[key])
        print(f"{name} {key}: deviation {d:.3e}, band {table[key].band:.3e}, gate {FC.gate(name, key):.3e}")
        if not d <= FC.gate(name, key):
            outside.append((key, d))
    assert not outside, outside


def test_model_refuses_a_final_map_that_is_not_the_head_window(small_model):
    N, T, H, W, _, _ = FC.REFUSED
    with pytest.raises(M324Error, match=r"96 x 64.*3 x 2"):
        small_model.features(_dev(FC.make_videos(N, T, H, W, 1)))
    with pytest.raises(M324Error, match="at least 10 frames"):
        small_model.features(_dev(FC.make_videos(1, 9, 64, 64, 1)))
    with pytest.raises(M324Error, match="must be on"):
        small_model.features(torch.from_numpy(FC.make_videos(1, 10, 64, 64, 1)))
    with pytest.raises(M324Error, match="scratch bytes"):
        small_model.features(_dev(FC.make_videos(1, 10, 64, 64, 1)), max_scratch_bytes=1 << 16)


def test_model_exact_properties(small_model):
    videos = _dev(FC.make_videos(3, 10, 64, 64, 5))
    feats, taps = small_model.features(videos, taps=True)
    per = V.scratch_bytes_per_video(10, 64, 64)
    for budget in (per, 2 * per):                                        # chunks of one and of two sub-videos
        f2, t2 = small_model.features(videos, taps=True, max_scratch_bytes=budget)
        assert torch.equal(f2, feats) and all(torch.equal(t2[k], taps[k]) for k in taps), budget
    perm = torch.tensor([1, 2, 0], device="cuda")
    assert torch.equal(small_model.features(videos[perm]), feats[perm])
    assert torch.equal(small_model.features(videos), feats)
    assert torch.equal(small_model.features(_dev(videos.cpu().to(torch.float32) / 255.0)), feats)             # bytes against their floats


# ------------------------------------------------------------------------------------------------ clips and the command line
def test_evaluate_clips_fvd(small_model):
    gt = FC.make_videos(1, 64, 64, 64, 8)[0]
    rng = np.random.default_rng(9)
    res = np.clip(gt.astype(np.int64) + rng.integers(-30, 31, gt.shape), 0, 255).astype(np.uint8)
    score = V.evaluate_clips_fvd(_dev(gt), _dev(res), small_model)                               # 64 frames: N = 2
    assert score.feats_gt.shape == (2, 400) and score.value == V.frechet_distance(score.feats_result, score.feats_gt) and score.value > 0
    direct = small_model.features(_dev(np.stack([res[:32], res[32:]]))).double().cpu().numpy()
    assert np.array_equal(direct, score.feats_result)
    short = V.evaluate_clips_fvd(_dev(gt[:32]), _dev(res[:32]), small_model)                     # 32 frames: N = 1
    assert short.value == float(np.square(short.feats_result - short.feats_gt).sum()) and short.value > 0
    assert np.array_equal(short.feats_gt[0], score.feats_gt[0])
    assert V.evaluate_clips_fvd(_dev(gt), _dev(gt.copy()), small_model).value == 0.0
    assert V.evaluate_clips_fvd(_dev(gt[:20]), _dev(gt[:20].copy()), small_model).value == 0.0   # padded by the reversed tail
    with pytest.raises(M324Error, match="at least 16"):
        V.evaluate_clips_fvd(_dev(gt[:12]), _dev(res[:12]), small_model)
    with pytest.raises(M324Error, match="equal shapes"):
        V.evaluate_clips_fvd(_dev(gt[:32]), _dev(res[:33]), small_model)


def test_command_line(weights, tmp_path, capsys):
    """two .npy clips, one missing pair and a state-dict file through main(): the result file and the summary line"""
    rng = np.random.default_rng(7)
    gt = FC.make_videos(1, 16, 48, 64, 10)[0]
    res = np.clip(gt.astype(np.int64) + rng.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
    np.save(tmp_path / "gt.npy", gt)
    (tmp_path / "results").mkdir()
    np.save(tmp_path / "results" / "clip_a.npy", res)
    torch.save(FC.state_dict(), tmp_path / "i3d.pth")
    values = V.main(["--gt_paths", str(tmp_path / "gt.npy"), str(tmp_path / "absent.npy"), "--result_paths",
                     str(tmp_path / "results" / "clip_a.npy"), str(tmp_path / "results" / "clip_b.npy"), "--weights", str(tmp_path / "i3d.pth")])
    out = capsys.readouterr().out
    want = V.evaluate_clips_fvd(_dev(gt), _dev(res), V.I3D(weights, "cuda")).value               # 16 frames: padded to 32 by the reversed clip
    assert values == [want] and want > 0
    assert "absent.npy not found, skipping" in out and f"Summary: processed 1/2 pairs; Average FVD: {want:.6f}" in out
    lines = (tmp_path / "results" / "clip_a.txt").read_text().splitlines()
    assert lines[:3] == [f"GT Source: {tmp_path / 'gt.npy'}", f"Result Source: {tmp_path / 'results' / 'clip_a.npy'}", f"FVD: {want}"]
    V.main(["--gt_paths", str(tmp_path / "gt.npy"), "--result_paths", str(tmp_path / "results" / "clip_a.npy"), "--weights",
            str(tmp_path / "i3d.pth"), "--output_dir", str(tmp_path / "out")])
    assert (tmp_path / "out" / "clip_a.txt").read_text().splitlines()[2] == f"FVD: {want}"
