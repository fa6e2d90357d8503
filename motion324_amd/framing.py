"""Video framing: a matted video becomes the foreground-centred square clip the model was trained on.

replaces: utils/rmbg_for_black_bg.py (compute_mask_bbox, merge_bbox, crop_and_center_to_512 and the masking inside
remove_background / process_images_in_folder; a PIL loop per frame that scripts/4D_from_video.sh runs before inference) and the
soft masking of utils/inference_utils.py:segment_foreground_with_u2net.  The matting network is not part of this module: the
input is RGBA frames, or RGB plus alpha -- from motion324_amd.matting (matte_video(...).alpha, U2-Net on the device) or from
whichever other tool made the matte.

What runs where.  The kernels of csrc/framing.hip do everything that touches a pixel: masking, per-frame boxes, the first pass
(crop + masking + resampling into a uint8 intermediate; the horizontal one, see pass_order) and the second pass (resampling +
paste + canvas fill).  The host does what depends on a handful of numbers only: the union of the boxes, the placement on the
canvas, the order of the passes and the two coefficient tables, which depend on the union box -- hence ONE device-to-host
transfer, the [T, 4] boxes, between the first kernel and the rest.  The tables are built here in float64 because they are a few kilobytes of libm arithmetic (sin, a division, a rounding)
whose every bit decides a coefficient; on the host they are the published construction evaluated the way the reference
library evaluates it, and the device then does integer arithmetic only, so the frames equal the reference's bit for bit.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops
from .lib import M324Error

PRECISION_BITS = 22                       # fixed-point position of the 8-bit resampling coefficients
LANCZOS_SUPPORT = 3.0
BICUBIC_SUPPORT = 2.0
BICUBIC_A = -0.5                          # the cubic's free parameter in the reference library's 8-bit resampling


class FramedVideo(NamedTuple):
    frames: torch.Tensor                  # uint8 [T, size, size, 3], device: what run_model_inference takes as its video
    mask: torch.Tensor                    # uint8 [T, size, size], device: the resampled mask (0 / 255 before resampling, or alpha)
    box: Tuple[int, int, int, int]        # (left, top, right, bottom) of the foreground over all frames, right / bottom open
    placement: Tuple[int, int, int, int]  # (new_w, new_h, off_x, off_y) of the resized crop on the canvas


def _lanczos(t: float) -> float:
    if not -LANCZOS_SUPPORT <= t < LANCZOS_SUPPORT:
        return 0.0
    if t == 0.0:
        return 1.0
    a, b = t * math.pi, (t / LANCZOS_SUPPORT) * math.pi      # sinc(t) * sinc(t / 3), each argument rounded before the product with pi
    return (math.sin(a) / a) * (math.sin(b) / b)


def _bicubic(t: float) -> float:
    a = BICUBIC_A
    t = -t if t < 0.0 else t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


FILTERS = {"lanczos": (_lanczos, LANCZOS_SUPPORT), "bicubic": (_bicubic, BICUBIC_SUPPORT)}


def resample_tables(in_size: int, out_size: int, filter: str = "lanczos") -> Tuple[np.ndarray, np.ndarray]:
    """(coef int32 [out_size, ksize], bounds int32 [out_size, 2] = (first source sample, number of taps)) of one 8-bit Lanczos
    pass from in_size to out_size samples.  The filter is stretched by the scale when shrinking; every output's window is cut
    at the ends of the line, its weights are normalised by their sum (added in tap order) and rounded half away from zero to
    22 fractional bits.  Unused taps are zero.  filter "bicubic": the reference library's cubic (a = -0.5, support 2) under the
    same window, normalisation and rounding rules."""
    if in_size <= 0 or out_size <= 0:
        raise M324Error(f"resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    if filter not in FILTERS:
        raise M324Error(f"resample_tables: filter must be one of {sorted(FILTERS)}, got {filter!r}")
    kernel, kernel_support = FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = kernel_support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    inv = 1.0 / fs
    one = float(1 << PRECISION_BITS)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        weights = [kernel((x + xmin - center + 0.5) * inv) for x in range(xmax - xmin)]
        total = 0.0
        for w in weights:
            total += w
        for x, w in enumerate(weights):
            if total != 0.0:
                w /= total
            coef[i, x] = int(w * one + 0.5) if w >= 0 else int(w * one - 0.5)
        bounds[i] = (xmin, xmax - xmin)
    return coef, bounds


def placement(box, size: int = 512) -> Tuple[int, int, int, int]:
    """(new_w, new_h, off_x, off_y): the box scaled so that its longer side is `size` (round half to even, at least one pixel)
    and centred on a size x size canvas, the offsets rounded down"""
    left, top, right, bottom = (int(v) for v in box)
    w, h = right - left, bottom - top
    if w <= 0 or h <= 0 or size <= 0:
        raise M324Error(f"placement: an empty box {tuple(box)} or canvas {size}")
    s = size / max(w, h)
    new_w, new_h = max(1, int(round(w * s))), max(1, int(round(h * s)))
    return new_w, new_h, (size - new_w) // 2, (size - new_h) // 2


def pass_order(w: int, h: int, new_h: int) -> str:
    """"xy": the horizontal pass first, the rule of the reference library -- except for an image more than a hundred times as tall
    as it is wide whose height shrinks, which its Image.resize resamples vertically first ("yx").  The uint8 intermediate makes
    the two orders differ in the last bit, so the order is part of the contract."""
    return "yx" if h > w * 100 and new_h < h else "xy"


def soft_table() -> np.ndarray:
    """uint8 [256, 256]: table[alpha, value] = uint8(value * (alpha / 255.0)), the reference's soft masking in float64"""
    a = np.arange(256, dtype=np.float64)[:, None] / 255.0
    return (np.arange(256, dtype=np.uint8)[None, :] * a).astype(np.uint8)


def union_box(boxes) -> Optional[Tuple[int, int, int, int]]:
    """the union of the non-empty per-frame boxes [T, 4] (left < right), or None when every frame is empty"""
    b = np.asarray(boxes).reshape(-1, 4)
    b = b[(b[:, 0] < b[:, 2]) & (b[:, 1] < b[:, 3])]
    if len(b) == 0:
        return None
    return int(b[:, 0].min()), int(b[:, 1].min()), int(b[:, 2].max()), int(b[:, 3].max())


def _as_device_u8(x, device, name: str) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype != torch.uint8:
        raise M324Error(f"frame_video: {name} must be uint8, got {t.dtype}")
    return t if t.is_cuda and (device is None or t.device == torch.device(device)) else t.to(device)


def frame_video(video, alpha=None, *, size: int = 512, mode: str = "threshold", threshold: int = 204, device=None) -> Optional[FramedVideo]:
    """video: uint8 [T,H,W,4] (RGBA), or [T,H,W,3] with alpha uint8 [T,H,W]; a host array / tensor (uploaded to `device`) or a
    device tensor (used where it is).  mode "threshold": foreground = alpha > threshold, background zeroed, mask 0 / 255
    (rmbg_for_black_bg.py); mode "soft": rgb * alpha / 255 and the alpha itself (inference_utils.py).  Every frame is cropped to
    the union of the per-frame foreground boxes, resized with 8-bit Lanczos so that the longer side becomes `size`, and pasted
    centred on a black canvas.  Returns None when no frame has foreground (the reference writes no 512 outputs then).

    Everything runs on the caller's stream; the only synchronisation is the read-back of the [T, 4] boxes."""
    if mode not in ("threshold", "soft"):
        raise M324Error(f"frame_video: mode must be 'threshold' or 'soft', got {mode!r}")
    if not 0 <= int(threshold) <= 255 or not 0 < int(size) <= 16384:
        raise M324Error(f"frame_video: threshold must be in 0..255 and size in 1..16384, got {threshold}, {size}")
    if device is None:
        if not (isinstance(video, torch.Tensor) and video.is_cuda):
            raise M324Error("frame_video: a host video needs device= (the framing runs on the GPU; there is no host path)")
        device = video.device
    v = _as_device_u8(video, device, "video")
    if v.dim() != 4 or v.shape[3] not in (3, 4) or 0 in v.shape:
        raise M324Error(f"frame_video: expected video [T,H,W,4] or [T,H,W,3], got {tuple(v.shape)}")
    if alpha is None:
        if v.shape[3] != 4:
            raise M324Error("frame_video: an RGB video needs alpha [T,H,W]")
        if v.stride(3) != 1 or v.stride(2) != 4:
            v = v.contiguous()
        rgb, a = v[..., :3], v[..., 3]
    else:
        a = _as_device_u8(alpha, device, "alpha")
        if tuple(a.shape) != tuple(v.shape[:3]):
            raise M324Error(f"frame_video: alpha {tuple(a.shape)} does not match video {tuple(v.shape)}")
        rgb = v[..., :3]
        if rgb.stride(3) != 1 or rgb.stride(2) not in (3, 4):
            rgb = rgb.contiguous()
    T, H, W = a.shape
    table = torch.from_numpy(soft_table()).to(device) if mode == "soft" else None

    boxes = ops.frame_mask(rgb, a, mode=mode, threshold=threshold, table=table, want_masked=False, want_mask=False)[2]
    box = union_box(boxes.cpu().numpy())                   # the one device-to-host transfer: the tables depend on the union box
    if box is None:
        return None
    left, top, right, bottom = box
    w, h = right - left, bottom - top
    new_w, new_h, off_x, off_y = place = placement(box, size)
    tabs = {axis: tuple(torch.from_numpy(t).to(device) for t in resample_tables(n_in, n_out))
            for axis, n_in, n_out in (("x", w, new_w), ("y", h, new_h))}
    frames = torch.empty((T, size, size, 3), dtype=torch.uint8, device=device)
    mask = torch.empty((T, size, size), dtype=torch.uint8, device=device)
    crop = (left, top, w, h)
    order = pass_order(w, h, new_h)
    # first pass: crop + masking + resampling into a uint8 intermediate; second pass: resampling + paste + fill of the whole canvas.
    # Colour first; then the mask: the 0 / 255 image of the threshold mode is made from the alpha plane on the fly, the soft
    # mode's mask is the alpha itself.
    for src, channels, m, out in ((rgb, 3, mode, frames), (a, 1, "binary" if mode == "threshold" else "none", mask)):
        mid = ops.frame_resample(src, *tabs[order[0]], order[0], channels=channels, crop=crop, alpha=a, mode=m, threshold=threshold,
                                 table=table if m == "soft" else None)
        ops.frame_resample(mid, *tabs[order[1]], order[1], channels=channels, out=out, paste=(off_x, off_y), fill=0)
    return FramedVideo(frames, mask, box, place)
