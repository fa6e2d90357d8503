"""Cases, oracle and gate of the LPIPS tests (tests/test_lpips_cpu.py, tests/test_lpips_gpu.py, tests/golden/make_lpips_band.py).

The oracle is a torch CPU model of the metric written from its definition: conv2d / max_pool2d at a chosen precision, and the
bilinear upsample to H x W exactly as the reference takes it, next to the mean at the tap's own resolution.  Four faults can be
planted into it; the CPU tests require the gate to see each of them.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from motion324_amd import perceptual as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_band.npz")
WEIGHT_SEED = 324
GATE_FACTOR = 8.0           # times the recorded deviation of the fp32 CPU run; the reason is in tests/ERROR_BOUNDS_LPIPS.md
FAULTS = ("pad_before_scaling", "relu5_3_before_relu", "weight_before_square", "shifted_tap")
SHIFTED_TAP_LAYER = 10      # conv5_1: a deep layer, which contributes about 1 % of the total

# name: (H, W, T, kind)
CASES = {
    "border16": (16, 16, 3, "noise"),           # conv5 works on 1 x 1: every tap but the centre is padding
    "square32": (32, 32, 3, "noise"),
    "ragged48x80": (48, 80, 2, "noise"),        # 3840, 960, 240, 60, 15 pixels per frame: no multiple of any tile
    "near32": (32, 32, 1, "near"),              # b = a but for one level in 5 % of the bytes: the worst cancellation
    "blackwhite32": (32, 32, 1, "blackwhite"),  # constant images: the border is the only structure
}

_STATE = {}


def state_dict():
    if "sd" not in _STATE:
        _STATE["sd"] = P.synth_lpips_state_dict(WEIGHT_SEED)
    return _STATE["sd"]


def clips(name):
    """(a, b) uint8 [T,H,W,3] numpy of a case; seeded by the case's position"""
    H, W, T, kind = CASES[name]
    rng = np.random.default_rng(1000 + list(CASES).index(name))
    if kind == "blackwhite":
        return np.zeros((T, H, W, 3), np.uint8), np.full((T, H, W, 3), 255, np.uint8)
    # smooth content plus texture, so that the deep taps see structure and not only noise
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = np.stack([np.sin(6.0 * xx + c) * np.cos(4.0 * yy - t) for t in range(T) for c in range(3)]).reshape(T, 3, H, W)
    a = 128 + 70 * base.transpose(0, 2, 3, 1) + rng.normal(0, 25, (T, H, W, 3))
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    if kind == "near":
        step = np.where(rng.random(a.shape) < 0.05, rng.choice([-1, 1], a.shape), 0)
        b = np.clip(a.astype(np.int64) + step, 0, 255).astype(np.uint8)
    else:
        b = np.clip(np.rint(a + rng.normal(0, 20, a.shape)), 0, 255).astype(np.uint8)
    return a, b


def to_float_nchw(frames):
    """fp32 [T,3,H,W] in [-1, 1] from bytes, by the formula of the prepare kernel: (v / 255) * 2 - 1 in fp32"""
    x = torch.from_numpy(np.ascontiguousarray(frames)).permute(0, 3, 1, 2).to(torch.float32)
    return ((x / 255.0) * 2.0 - 1.0).contiguous()


def _trunk(state, x, dtype, fault):
    """the five taps of x [T,3,H,W] (already in [-1, 1])"""
    shift = torch.tensor(P.SHIFT, dtype=dtype).reshape(1, 3, 1, 1)
    scale = torch.tensor(P.SCALE, dtype=dtype).reshape(1, 3, 1, 1)
    first_padding = 1
    if fault == "pad_before_scaling":
        x = F.pad(x, (1, 1, 1, 1))
        first_padding = 0
    x = (x - shift) / scale
    taps, i = [], 0
    for s, stage in enumerate(P.STAGES):
        if s > 0:
            x = F.max_pool2d(x, 2, 2)
        for j, _ in enumerate(stage):
            w = state[P.CONV_KEYS[i] + ".weight"].to(dtype)
            b = state[P.CONV_KEYS[i] + ".bias"].to(dtype)
            if fault == "shifted_tap" and i == SHIFTED_TAP_LAYER:
                w = w.clone()
                w[:, :, 0, 0], w[:, :, 0, 1] = w[:, :, 0, 1].clone(), w[:, :, 0, 0].clone()
            x = F.conv2d(x, w, b, padding=first_padding if i == 0 else 1)
            last = s == 4 and j == len(stage) - 1
            if last and fault == "relu5_3_before_relu":
                taps.append(x)
                x = F.relu(x)
                i += 1
                continue
            x = F.relu(x)
            i += 1
        if len(taps) == s:
            taps.append(x)
    return taps


def oracle(a, b, dtype=torch.float64, fault=None, state=None):
    """(low [T,5], up [T,5]) as numpy float64: per frame and tap, the mean of d_k over the tap's own pixels, and the mean of d_k
    upsampled bilinearly (align_corners=False) to H x W as the reference builds it.  a, b: uint8 [T,H,W,3] numpy."""
    state = state_dict() if state is None else state
    H, W = a.shape[1], a.shape[2]
    with torch.no_grad():
        fa = _trunk(state, to_float_nchw(a).to(dtype), dtype, fault)
        fb = _trunk(state, to_float_nchw(b).to(dtype), dtype, fault)
        low, up = [], []
        for k, (ta, tb) in enumerate(zip(fa, fb)):
            w = state[P.LIN_KEYS[k]].to(dtype)
            na = ta / (torch.sqrt((ta * ta).sum(1, keepdim=True)) + 1e-10)
            nb = tb / (torch.sqrt((tb * tb).sum(1, keepdim=True)) + 1e-10)
            if fault == "weight_before_square":
                d = ((w * (na - nb)) ** 2).sum(1, keepdim=True)
            else:
                d = F.conv2d((na - nb) ** 2, w)
            low.append(d.mean(dim=(1, 2, 3)))
            up.append(F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False).mean(dim=(1, 2, 3)))
    return torch.stack(low, 1).double().numpy(), torch.stack(up, 1).double().numpy()


def with_total(per_layer):
    """[T,5] -> [T,6]: the five layers and their sum"""
    per_layer = np.asarray(per_layer, dtype=np.float64)
    return np.concatenate([per_layer, per_layer.sum(1, keepdims=True)], axis=1)


def relative_deviation(values, ref):
    """[6]: per layer (and total) the largest |values - ref| / |ref| over the frames; values, ref [T,5]"""
    v, r = with_total(values), with_total(ref)
    return (np.abs(v - r) / np.abs(r)).max(0)             # no case has a zero reference: the clips of every case differ


def golden():
    """{case: (ref [T,5] fp64, band [6])} from tests/golden/lpips_band.npz"""
    z = np.load(GOLDEN)
    return {name: (z[name + ".ref"], z[name + ".band"]) for name in CASES}


def gate(name):
    """[6]: the largest relative deviation allowed per layer (and for the total) in a case: GATE_FACTOR times the recorded band.
    blackwhite32 alone floors its band at one unit roundoff: its single frame makes the recorded deviation the luck of one fp32
    rounding (3e-9 on layer 2, a twentieth of an ulp), which no fp32 result can be held to."""
    band = golden()[name][1]
    if name == "blackwhite32":
        band = np.maximum(band, 2.0 ** -24)
    return GATE_FACTOR * band


def outside_gate(values, ref, allowed):
    """boolean [6]: layers (and the total) where some frame deviates by more than `allowed` (gate(name))"""
    return ~(relative_deviation(values, ref) <= allowed)
