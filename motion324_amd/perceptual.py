"""Perceptual evaluation on the GPU: LPIPS (VGG16, version 0.1) between two clips, frame by frame.

The image-space half of the reference's evaluation (evaluation/evaluation.py, `lpips.LPIPS(net='vgg', spatial=True)` followed by
`.mean()`): a scaling layer, the thirteen 3 x 3 convolutions of torchvision's VGG16 `features[0..29]`, five taps behind
relu1_2, relu2_2, relu3_3, relu4_3 and relu5_3, and per tap the channel-normalised squared difference weighted by a 1 x 1 layer.
The score of a frame pair is the sum over the taps of the mean over that tap's own pixels: for sizes that are multiples of 16
the reference's bilinear upsampling to H x W preserves the mean, so no upsampled map is built.  Everything is fp32 on the fp32
MFMA (csrc/conv.hip, the head in csrc/perceptual.hip; include/m324.h has the arithmetic).  The weights are the user's: a
torchvision VGG16 state dict and the LPIPS package's `vgg.pth`, or the state dict of the reference's LPIPS module.

    python -m motion324_amd.perceptual --gt_paths A ... --result_paths B ... --weights vgg16.pth [lin.pth] [--output_dir DIR]
"""
from __future__ import annotations

import argparse
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .lib import M324Error
from .ops import pack_conv_weight         # re-exported: perceptual.pack_conv_weight is the name tests and tools know

# (input channels, output channels) of the thirteen convolutions; a pool follows each stage but the last
STAGES = (((3, 64), (64, 64)), ((64, 128), (128, 128)), ((128, 256), (256, 256), (256, 256)),
          ((256, 512), (512, 512), (512, 512)), ((512, 512), (512, 512), (512, 512)))
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)         # torchvision vgg16().features
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
SIZE_MULTIPLE = 16                      # four 2 x 2 pools: every pool exact, and the upsampled mean equals the tap's own
SUBVIDEO = 32                           # the reference's TIMESTAMP_LIMIT
# activations of one frame pair: two buffers of 2 frames x H x W x 64 channels x 4 bytes (the two 64-channel maps of stage 1)
BYTES_PER_PAIR_PIXEL = 2 * 2 * 64 * 4
DEFAULT_MAX_SCRATCH_BYTES = 4 << 30     # 16 pairs of 512 x 512 per chunk; the sweep is in profiles/perceptual_lpips.md


def _slice_names():
    """key of every convolution in the reference's LPIPS module: net.slice<s>.<features index>"""
    names, i = [], 0
    for s, stage in enumerate(STAGES):
        for _ in stage:
            names.append(f"net.slice{s + 1}.{FEATURE_INDEX[i]}")
            i += 1
    return names


CONV_KEYS = tuple(_slice_names())
LIN_KEYS = tuple(f"lin{k}.model.1.weight" for k in range(5))


class LpipsWeights(NamedTuple):
    conv: tuple          # thirteen (wp fp32 [Kpad, Cout], bias fp32 [Cout]): the K-major layout of ops.conv3x3
    lin: tuple           # five fp32 [C]


def _load_file(path: str) -> dict:
    if not os.path.isfile(path):
        raise M324Error(f"load_lpips_weights: no such file {path!r}")
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    if not isinstance(state, dict):
        raise M324Error(f"load_lpips_weights: {path!r} holds a {type(state).__name__}, not a state dict")
    return state


def _tensor(state, key: str, shape, source: str) -> torch.Tensor:
    if key not in state:
        raise M324Error(f"load_lpips_weights: {source} has no key {key!r}")
    t = state[key]
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
    if tuple(t.shape) != tuple(shape):
        raise M324Error(f"load_lpips_weights: {key!r} of {source} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not torch.isfinite(t).all():
        raise M324Error(f"load_lpips_weights: {key!r} of {source} holds values that are not finite")
    return t.detach().to(torch.float32).cpu()


def load_lpips_weights(state, lin_state=None) -> LpipsWeights:
    """The trunk and the five 1 x 1 layers, checked and repacked once (CPU tensors; LPIPS(...) moves them to its device).
      * `state` the state dict of the reference's LPIPS module (net.slice1.0.weight .. net.slice5.28.bias and
        lin0.model.1.weight .. lin4.model.1.weight; scaling_layer.* is ignored: those values are constants), lin_state None;
      * `state` a torchvision VGG16 state dict (features.0.weight .. features.28.bias; classifier.* ignored) and `lin_state` the
        five lin<k>.model.1.weight tensors of the LPIPS package's vgg.pth;
      * either of them as the path of a file torch.load reads.
    A missing or mis-shaped key is named in the error."""
    if isinstance(state, (str, os.PathLike)):
        state = _load_file(os.fspath(state))
    if isinstance(lin_state, (str, os.PathLike)):
        lin_state = _load_file(os.fspath(lin_state))
    if not isinstance(state, dict) or (lin_state is not None and not isinstance(lin_state, dict)):
        raise M324Error("load_lpips_weights: expected state dicts or paths to them")
    if any(k.startswith("features.") for k in state):
        if lin_state is None:
            raise M324Error("load_lpips_weights: a torchvision VGG16 state dict needs lin_state, the five lin<k>.model.1.weight tensors "
                            "of the LPIPS package's vgg.pth")
        names, trunk, heads = tuple(f"features.{i}" for i in FEATURE_INDEX), "the VGG16 state dict", "lin_state"
    else:
        if lin_state is not None:
            raise M324Error("load_lpips_weights: lin_state goes with a torchvision VGG16 state dict (features.*); this state dict has "
                            "no features.* key")
        names, trunk, heads, lin_state = CONV_KEYS, "the LPIPS state dict", "the LPIPS state dict", state
    conv = []
    for name, (cin, cout) in zip(names, [io for stage in STAGES for io in stage]):
        w = _tensor(state, name + ".weight", (cout, cin, 3, 3), trunk)
        b = _tensor(state, name + ".bias", (cout,), trunk)
        conv.append((pack_conv_weight(w), b.contiguous()))
    lin = []
    for key, c in zip(LIN_KEYS, TAP_CHANNELS):
        lin.append(_tensor(lin_state, key, (1, c, 1, 1), heads).reshape(c).contiguous())
    return LpipsWeights(tuple(conv), tuple(lin))


def synth_lpips_state_dict(seed: int) -> dict:
    """Seeded weights in the form of the reference's LPIPS state dict, for tests and timing: convolutions randn * sqrt(2 / (9 Cin)),
    biases 0.05 randn, lin weights rand / C -- about half of every tap's activations are alive."""
    g = torch.Generator().manual_seed(int(seed))
    state = {"scaling_layer.shift": torch.tensor(SHIFT).reshape(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(SCALE).reshape(1, 3, 1, 1)}
    for name, (cin, cout) in zip(CONV_KEYS, [io for stage in STAGES for io in stage]):
        state[name + ".weight"] = torch.randn((cout, cin, 3, 3), generator=g) * math.sqrt(2.0 / (9 * cin))
        state[name + ".bias"] = 0.05 * torch.randn((cout,), generator=g)
    for key, c in zip(LIN_KEYS, TAP_CHANNELS):
        state[key] = torch.rand((1, c, 1, 1), generator=g) / c
    return state


def check_clip_pair(a, b, name: str = "LPIPS"):
    """(T, H, W, is_bytes) of two clips in one of the two accepted forms, or an M324Error that says what is wrong.  Host-only."""
    for x in (a, b):
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise M324Error(f"{name}: expected uint8 [T,H,W,3] or fp32 [T,3,H,W] tensors")
    if a.shape != b.shape or a.dtype != b.dtype:
        raise M324Error(f"{name}: the two clips must have one shape and dtype, got {a.dtype} {tuple(a.shape)} and {b.dtype} {tuple(b.shape)}")
    if a.dtype == torch.uint8 and a.shape[3] == 3:
        T, H, W, is_bytes = a.shape[0], a.shape[1], a.shape[2], True
    elif a.dtype == torch.float32 and a.shape[1] == 3:
        T, H, W, is_bytes = a.shape[0], a.shape[2], a.shape[3], False
    else:
        raise M324Error(f"{name}: expected uint8 [T,H,W,3] or fp32 [T,3,H,W], got {a.dtype} {tuple(a.shape)}")
    if T < 1:
        raise M324Error(f"{name}: the clips have no frames")
    if H < SIZE_MULTIPLE or W < SIZE_MULTIPLE or H % SIZE_MULTIPLE or W % SIZE_MULTIPLE:
        raise M324Error(f"{name}: H and W must be multiples of {SIZE_MULTIPLE} and at least {SIZE_MULTIPLE} (four exact 2 x 2 pools; "
                        f"resizing is not part of this metric), got {H} x {W}")
    return T, H, W, is_bytes


def pairs_per_chunk(T: int, H: int, W: int, max_scratch_bytes: int) -> int:
    """frame pairs whose activations stay under max_scratch_bytes, or an M324Error when one pair does not fit"""
    per_pair = BYTES_PER_PAIR_PIXEL * H * W
    if per_pair > int(max_scratch_bytes):
        raise M324Error(f"LPIPS: one {H} x {W} frame pair needs {per_pair} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
    return max(1, min(int(T), int(max_scratch_bytes) // per_pair))


class LPIPS:
    """metric = LPIPS(weights, device); metric(a, b) -> fp32 [T] on the device, one value per frame pair.
    weights: a LpipsWeights, or whatever load_lpips_weights accepts (a tuple (state, lin_state) for the two-file form)."""

    def __init__(self, weights, device="cuda"):
        if not isinstance(weights, LpipsWeights):
            weights = load_lpips_weights(*weights) if isinstance(weights, (tuple, list)) else load_lpips_weights(weights)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise M324Error("LPIPS: needs a HIP device (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.conv = tuple((wp.to(self.device), b.to(self.device)) for wp, b in weights.conv)
        self.lin = tuple(w.to(self.device) for w in weights.lin)

    def __call__(self, a, b, *, normalize: bool = False, per_layer: bool = False, max_scratch_bytes: int = DEFAULT_MAX_SCRATCH_BYTES,
                 stage_events=None):
        """a, b: uint8 [T,H,W,3] (RenderedClip.frames, FramedVideo.frames) or fp32 [T,3,H,W] in [-1, 1] ([0, 1] with normalize),
        device tensors of one shape with H, W multiples of 16.  Returns fp32 [T]; with per_layer also fp32 [T,5], the five
        taps' means whose sum (in tap order) the score is.  Both clips pass the trunk as one batch, `pairs_per_chunk` frame
        pairs at a time; nothing synchronises.  stage_events: a list that receives (label, start, end) device events per
        stage and head of every chunk (tools/lpips_time.py)."""
        T, H, W, is_bytes = check_clip_pair(a, b)
        if not a.is_cuda or not b.is_cuda or a.device != self.device or b.device != self.device:
            raise M324Error(f"LPIPS: both clips must be on {self.device} (there is no CPU path)")
        if is_bytes and normalize:
            raise M324Error("LPIPS: normalize applies to fp32 input in [0, 1]; bytes are always 0..255")
        n = pairs_per_chunk(T, H, W, max_scratch_bytes)
        half = 2 * n * H * W * 64                       # elements of one of the two activation buffers
        scratch = torch.empty((2 * half,), dtype=torch.float32, device=self.device)
        layers = torch.empty((5, T), dtype=torch.float32, device=self.device)
        for t0 in range(0, T, n):
            t1 = min(T, t0 + n)
            self._chunk(a[t0:t1], b[t0:t1], normalize, scratch, half, layers[:, t0:t1], stage_events)
        total = (((layers[0] + layers[1]) + layers[2]) + layers[3]) + layers[4]
        return (total, layers.t().contiguous()) if per_layer else total

    def _chunk(self, a, b, normalize, scratch, half, layers, stage_events):
        n = a.shape[0]
        H, W = (a.shape[1], a.shape[2]) if a.dtype == torch.uint8 else (a.shape[2], a.shape[3])
        bufs = (scratch[:half], scratch[half:])

        def view(which, h, w, c):
            return bufs[which][:2 * n * h * w * c].view(2 * n, h, w, c)

        def mark(label, start):
            if stage_events is not None:
                end = torch.cuda.Event(enable_timing=True)
                end.record()
                stage_events.append((label, start, end))

        def begin():
            if stage_events is None:
                return None
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        start = begin()
        cur = 1
        x = view(cur, H, W, 4)
        ops.lpips_prepare(a, normalize=normalize, out=x[:n])
        ops.lpips_prepare(b, normalize=normalize, out=x[n:])
        h, w, i = H, W, 0
        for s, stage in enumerate(STAGES):
            if s > 0:
                start = begin()
                h, w = h // 2, w // 2
                x = ops.maxpool2x2(x, out=view(1 - cur, h, w, x.shape[3]))
                cur = 1 - cur
            for _ in stage:
                wp, bias = self.conv[i]
                x = ops.conv3x3(x, wp, bias, relu=True, out=view(1 - cur, h, w, wp.shape[1]))
                cur = 1 - cur
                i += 1
            mark(f"stage{s + 1}", start)
            start = begin()
            ops.lpips_layer(x[:n], x[n:], self.lin[s], out=layers[s])
            mark("head", start)


def subvideo_frames(T: int):
    """The frame indices the reference's process_single_video keeps, as a list of 32-frame sub-videos: a clip shorter than 32
    frames is extended by its last 32 - T frames reversed, then cut into 32-frame pieces; the remainder is dropped."""
    T = int(T)
    if T < SUBVIDEO // 2:
        raise M324Error(f"evaluate_clips: a clip of {T} frames cannot be extended to {SUBVIDEO} by its reversed tail (the reference "
                        f"crashes on an empty stack there); at least {SUBVIDEO // 2} frames are needed")
    index = list(range(T))
    if T < SUBVIDEO:
        index += index[-(SUBVIDEO - T):][::-1]
    return [index[i:i + SUBVIDEO] for i in range(0, len(index) - SUBVIDEO + 1, SUBVIDEO)]


class ClipScore(NamedTuple):
    value: float                # mean over all kept frames
    value_std: float            # population standard deviation over them
    per_video: np.ndarray       # [n_sub] mean per 32-frame sub-video
    per_frame: np.ndarray       # [T] the metric of every input frame pair, kept or not


def clip_statistics(per_frame: np.ndarray) -> ClipScore:
    """The reference's statistics (only_final=True) of the per-frame values of one clip: host-only, fp64."""
    per_frame = np.asarray(per_frame, dtype=np.float64)
    kept = np.stack([per_frame[idx] for idx in subvideo_frames(per_frame.shape[0])])
    return ClipScore(float(kept.mean()), float(kept.std()), kept.mean(axis=1), per_frame)


def evaluate_clips(gt, result, metric, **kw) -> ClipScore:
    """Scores `result` against `gt` as the reference's evaluation.py does for LPIPS.  Every frame pair is evaluated once; the
    padding repeats values, not work.  The one synchronisation of the path is the copy of the [T] values to the host."""
    if tuple(gt.shape) != tuple(result.shape):
        raise M324Error(f"evaluate_clips: the clips must have equal shapes, got {tuple(gt.shape)} and {tuple(result.shape)}")
    T = check_clip_pair(gt, result, "evaluate_clips")[0]
    subvideo_frames(T)                                  # refuses T < 16 before any work
    return clip_statistics(metric(gt, result, **kw).double().cpu().numpy())


IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg")


def load_frames(path: str) -> np.ndarray:
    """uint8 [T,H,W,3] from a directory of PNG / JPG frames (sorted by name, read with PIL) or a .npy of that shape"""
    if os.path.isdir(path):
        from PIL import Image
        names = sorted(f for f in os.listdir(path) if f.lower().endswith(IMAGE_SUFFIXES))
        if not names:
            raise M324Error(f"{path}: no PNG / JPG frames")
        frames = [np.asarray(Image.open(os.path.join(path, f)).convert("RGB")) for f in names]
        if any(f.shape != frames[0].shape for f in frames):
            raise M324Error(f"{path}: the frames have different sizes")
        return np.stack(frames)
    if path.lower().endswith(".npy"):
        frames = np.load(path)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
            raise M324Error(f"{path}: expected uint8 [T,H,W,3], got {frames.dtype} {frames.shape}")
        return frames
    raise M324Error(f"{path}: expected a directory of PNG / JPG frames or a .npy of uint8 [T,H,W,3]; video files and resizing are out "
                    f"of scope here -- decode first, to equal sizes that are multiples of {SIZE_MULTIPLE}")


def main(argv=None):
    parser = argparse.ArgumentParser(description="LPIPS (VGG16) between ground-truth and result clips on the GPU")
    parser.add_argument("--gt_paths", type=str, required=True, nargs="+", help="frame directories or .npy clips")
    parser.add_argument("--result_paths", type=str, required=True, nargs="+")
    parser.add_argument("--weights", type=str, required=True, nargs="+",
                        help="one file: the LPIPS module's state dict; two: torchvision's VGG16 state dict and the LPIPS package's vgg.pth")
    parser.add_argument("--output_dir", type=str, default=None)
    args = parser.parse_args(argv)
    if len(args.gt_paths) != len(args.result_paths):
        raise M324Error(f"{len(args.gt_paths)} gt paths but {len(args.result_paths)} result paths: pairs are matched by position")
    if len(args.weights) > 2:
        raise M324Error("--weights takes one file or two")
    weights = load_lpips_weights(*args.weights)
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.perceptual needs a HIP device (there is no CPU path)")
    metric = LPIPS(weights, "cuda")
    results = []
    for gt_path, result_path in zip(args.gt_paths, args.result_paths):
        missing = [p for p in (gt_path, result_path) if not os.path.exists(p)]
        if missing:
            print(f"Warning: {missing[0]} not found, skipping")
            continue
        gt, result = (torch.from_numpy(load_frames(p)).to("cuda") for p in (gt_path, result_path))
        score = evaluate_clips(gt, result, metric)
        results.append(score.value)
        base = os.path.basename(result_path.rstrip("/"))
        if os.path.isfile(result_path):
            base = os.path.splitext(base)[0]
        out_dir = args.output_dir if args.output_dir else os.path.dirname(result_path.rstrip("/"))
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        out_file = os.path.join(out_dir, base + ".txt")
        with open(out_file, "w") as f:
            f.write(f"GT Source: {gt_path}\nResult Source: {result_path}\nLPIPS: {score.value}\n" + "-" * 50 + "\n")
        print(f"{result_path}: LPIPS {score.value:.6f} (std {score.value_std:.6f}, {len(score.per_video)} sub-video(s)) -> {out_file}")
    print(f"Summary: processed {len(results)}/{len(args.gt_paths)} pairs" + (f"; Average LPIPS: {np.mean(results):.6f}" if results else ""))
    return results


if __name__ == "__main__":
    main()
