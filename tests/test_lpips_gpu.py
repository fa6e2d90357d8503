"""LPIPS on the GPU: ops.conv3x3 element by element against fp64 under a derived bound, the metric end to end against the fp64
oracle inside the recorded gate, and the exact properties (tests/ERROR_BOUNDS_LPIPS.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import error_bounds as EB
import lpips_cases as LC
from motion324_amd import ops
from motion324_amd import perceptual as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def metric():
    return P.LPIPS(P.load_lpips_weights(LC.state_dict()), DEV)


def _dev(frames):
    return torch.from_numpy(frames).to(DEV)


# ------------------------------------------------------------------------------------------------ the convolution alone
@pytest.mark.parametrize("images", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 7), (16, 24)])
# Cout = 32 is a 64-wide tile with half its columns past Cout, Cout = 96 one with a ragged second column tile
@pytest.mark.parametrize("cin,cout", [(4, 64), (64, 64), (64, 128), (256, 512), (512, 512), (8, 32), (4, 96)])
def test_conv3x3_elementwise(cin, cout, H, W, images):
    g = torch.Generator().manual_seed(cin * 7 + cout * 3 + H * 11 + images)
    x = torch.randn((images, cin, H, W), generator=g) + 0.5                 # a non-zero mean: a wrong border shows
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = 0.05 * torch.randn((cout,), generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    bound = 2 * (9 * cin + 1) * EB.U32 * (F.conv2d(x.double().abs(), w.double().abs(), padding=1) + b.double().abs().reshape(1, -1, 1, 1))
    nhwc = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wp, bd = P.pack_conv_weight(w).to(DEV), b.to(DEV)
    to_nhwc = lambda t: t.permute(0, 2, 3, 1)
    plain = ops.conv3x3(nhwc, wp, bd, relu=False)
    out = ops.conv3x3(nhwc, wp, bd)
    what = f"conv3x3 {cin}->{cout} {H}x{W} x{images}"
    r0 = EB.assert_within(plain, to_nhwc(ref), to_nhwc(bound), what + " (no ReLU)")
    r1 = EB.assert_within(out, to_nhwc(ref.clamp_min(0)), to_nhwc(bound), what)
    print(f"{what}: worst err / bound {r0:.3g} (plain) {r1:.3g} (ReLU)")
    assert torch.equal(out, plain.clamp_min(0))
    if H % 2 == 0 and W % 2 == 0:
        pooled = ops.maxpool2x2(out)
        EB.assert_within(pooled, to_nhwc(F.max_pool2d(ref.clamp_min(0), 2, 2)), to_nhwc(F.max_pool2d(bound, 2, 2)), what + " pooled")
        assert torch.equal(pooled.cpu(), to_nhwc(F.max_pool2d(out.cpu().permute(0, 3, 1, 2), 2, 2)))       # the pool adds no error


@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (16, 24)])
def test_maxpool2x2_is_the_ceil_pool_at_even_sizes(H, W):
    g = torch.Generator().manual_seed(H * 13 + W)
    x = (torch.randn((3, H, W, 8), generator=g) - 1.0).to(DEV)              # mostly negative: a zero-padded window would win
    out = ops.maxpool2x2(x)
    assert out.shape == (3, H // 2, W // 2, 8) and torch.equal(out, ops.maxpool2x2_ceil(x))


@pytest.mark.parametrize("channels,pixels", [(4, 1), (96, 65), (200, 130), (1024, 4200)])
def test_lpips_layer_alone(channels, pixels):
    """the head at channel counts of every lane grouping and at pixel counts around the run boundaries, against fp64.
    Bound, per term w d^2 with d = a / |a| - b / |b|: the norm is a sum of C squares under a root (relative (C + 4) U32 with the
    factor 2 of an order not relied on), the quotient rounds once more, so each quotient is off by e = ((C + 6) U32) of its own
    size and d by e_d = e (|a / |a|| + |b / |b||) + U32 |d|; the term by w (2 |d| e_d + e_d^2) + 2 U32 w d^2; the sum of the
    non-negative terms over channels and pixels passes at most 128 + pixels / 64 additions (lane, butterfly, run, runs), factor 2."""
    g = torch.Generator().manual_seed(channels + pixels)
    fa = torch.randn((2, pixels, 1, channels), generator=g).clamp_min(0)
    fb = (fa + 0.1 * torch.randn(fa.shape, generator=g)).clamp_min(0)
    fa[0, 0], fb[0, 0] = 0.0, 0.0                                            # a dead pixel: 0 / (0 + 1e-10)
    w = torch.rand((channels,), generator=g) / channels
    a, b, wd = fa.double(), fb.double(), w.double()
    na = a / (a.square().sum(-1, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.square().sum(-1, keepdim=True).sqrt() + 1e-10)
    d = na - nb
    ref = (wd * d * d).sum(-1).mean(dim=(1, 2))
    e_d = (channels + 6) * EB.U32 * (na.abs() + nb.abs()) + EB.U32 * d.abs()
    e = (wd * (2 * d.abs() * e_d + e_d * e_d + 2 * EB.U32 * d * d)).sum(-1).mean(dim=(1, 2)) + 2 * (128 + pixels / 64 + 2) * EB.U32 * ref
    out = ops.lpips_layer(fa.to(DEV), fb.to(DEV), w.to(DEV))
    EB.assert_within(out, ref, e, f"lpips_layer C={channels} pixels={pixels}")
    assert torch.equal(out, ops.lpips_layer(fb.to(DEV), fa.to(DEV), w.to(DEV)))
    assert torch.equal(ops.lpips_layer(fa.to(DEV), fa.to(DEV), w.to(DEV)), torch.zeros(2, device=DEV))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", list(LC.CASES))
def test_metric_against_the_fp64_oracle(metric, name):
    """per_layer and the total inside the recorded gate; `blackwhite32` is the padding-after-scaling check at model level"""
    a, b = LC.clips(name)
    ref, band = LC.golden()[name]
    total, layers = metric(_dev(a), _dev(b), per_layer=True)
    assert total.shape == (a.shape[0],) and layers.shape == (a.shape[0], 5) and total.dtype == layers.dtype == torch.float32
    got = layers.double().cpu().numpy()
    dev = LC.relative_deviation(got, ref)
    dev_total = np.abs(total.double().cpu().numpy() - ref.sum(1)) / np.abs(ref.sum(1))
    allowed = LC.gate(name)
    print(f"{name}: deviation per layer and total {np.array2string(dev, precision=3)}; returned total {dev_total.max():.3e}; "
          f"gate {np.array2string(allowed, precision=3)}; ratio {np.array2string(dev / allowed, precision=2)}")
    assert not LC.outside_gate(got, ref, allowed).any(), (name, dev, allowed)
    assert dev_total.max() <= allowed[5], (name, dev_total, allowed[5])


def test_exact_properties(metric):
    a, b = (_dev(x) for x in LC.clips("ragged48x80"))
    a3, b3 = (_dev(x) for x in LC.clips("square32"))
    total, layers = metric(a3, b3, per_layer=True)
    # the same frame on both sides: exactly zero, every layer
    zero_total, zero_layers = metric(a3, a3, per_layer=True)
    assert torch.equal(zero_total, torch.zeros_like(zero_total)) and torch.equal(zero_layers, torch.zeros_like(zero_layers))
    # one chunk or one pair per chunk
    per_pair = P.BYTES_PER_PAIR_PIXEL * 32 * 32
    assert P.pairs_per_chunk(3, 32, 32, per_pair) == 1
    t1, l1 = metric(a3, b3, per_layer=True, max_scratch_bytes=per_pair)
    assert torch.equal(t1, total) and torch.equal(l1, layers)
    t2, l2 = metric(a3, b3, per_layer=True, max_scratch_bytes=2 * per_pair)      # chunks of 2 and 1
    assert torch.equal(t2, total) and torch.equal(l2, layers)
    # a permutation of the frames
    perm = torch.tensor([2, 0, 1], device=DEV)
    tp, lp = metric(a3[perm], b3[perm], per_layer=True)
    assert torch.equal(tp, total[perm]) and torch.equal(lp, layers[perm])
    # a second call
    again, again_layers = metric(a3, b3, per_layer=True)
    assert torch.equal(again, total) and torch.equal(again_layers, layers)
    # bytes against the floats built from them, in [-1, 1] and in [0, 1]
    ragged = metric(a, b)
    fa, fb = LC.to_float_nchw(a.cpu().numpy()).to(DEV), LC.to_float_nchw(b.cpu().numpy()).to(DEV)
    assert torch.equal(metric(fa, fb), ragged)
    # v / 255 formed on the host: a device division by a Python scalar multiplies by the rounded reciprocal instead
    ua, ub = (torch.from_numpy(x.cpu().numpy().astype(np.float32) / np.float32(255)).permute(0, 3, 1, 2).contiguous().to(DEV) for x in (a, b))
    assert torch.equal(metric(ua, ub, normalize=True), ragged)
    # symmetry
    assert torch.equal(metric(b, a), ragged) and torch.equal(metric(b3, a3, per_layer=True)[1], layers)
    assert float(ragged.min()) > 0


def test_metric_refusals_on_device(metric):
    from motion324_amd.lib import M324Error
    a = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(M324Error, match="normalize"):
        metric(a, a, normalize=True)
    with pytest.raises(M324Error, match="must be on"):
        metric(a, a.cpu())
    with pytest.raises(M324Error, match="max_scratch_bytes is 1000"):
        metric(a, a, max_scratch_bytes=1000)
    with pytest.raises(M324Error, match="multiples of 16"):
        metric(a[:, :12], a[:, :12])


def test_evaluate_clips_on_a_40_frame_clip(metric):
    rng = np.random.default_rng(40)
    gt = rng.integers(0, 256, (40, 16, 16, 3), dtype=np.uint8)
    res = np.clip(gt.astype(np.int64) + rng.integers(-30, 31, gt.shape), 0, 255).astype(np.uint8)
    score = P.evaluate_clips(_dev(gt), _dev(res), metric)
    assert score.per_frame.shape == (40,) and np.array_equal(score.per_frame, metric(_dev(gt), _dev(res)).double().cpu().numpy())
    kept = score.per_frame[:32]                                             # one sub-video; frames 32..39 are the dropped remainder
    assert score.value == pytest.approx(np.mean(kept), rel=1e-15) and score.value_std == pytest.approx(np.std(kept), rel=1e-13)
    assert score.per_video.shape == (1,) and score.per_video[0] == pytest.approx(np.mean(kept), rel=1e-15)


def test_command_line(metric, tmp_path, capsys):
    """two .npy clips, one missing pair and the one-file weights form through main(): the result file and the summary line"""
    rng = np.random.default_rng(7)
    gt = rng.integers(0, 256, (16, 16, 32, 3), dtype=np.uint8)
    res = np.clip(gt.astype(np.int64) + rng.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
    np.save(tmp_path / "gt.npy", gt)
    (tmp_path / "results").mkdir()
    np.save(tmp_path / "results" / "clip_a.npy", res)
    torch.save(LC.state_dict(), tmp_path / "lpips.pth")
    values = P.main(["--gt_paths", str(tmp_path / "gt.npy"), str(tmp_path / "absent.npy"), "--result_paths",
                     str(tmp_path / "results" / "clip_a.npy"), str(tmp_path / "results" / "clip_b.npy"), "--weights", str(tmp_path / "lpips.pth")])
    out = capsys.readouterr().out
    want = P.evaluate_clips(_dev(gt), _dev(res), metric).value              # 16 frames: padded to 32 by the reversed clip
    assert values == [want] and want > 0
    assert "absent.npy not found, skipping" in out and f"Summary: processed 1/2 pairs; Average LPIPS: {want:.6f}" in out
    lines = (tmp_path / "results" / "clip_a.txt").read_text().splitlines()
    assert lines[:3] == [f"GT Source: {tmp_path / 'gt.npy'}", f"Result Source: {tmp_path / 'results' / 'clip_a.npy'}", f"LPIPS: {want}"]
    P.main(["--gt_paths", str(tmp_path / "gt.npy"), "--result_paths", str(tmp_path / "results" / "clip_a.npy"), "--weights",
            str(tmp_path / "lpips.pth"), "--output_dir", str(tmp_path / "out")])
    assert (tmp_path / "out" / "clip_a.txt").read_text().splitlines()[2] == f"LPIPS: {want}"
