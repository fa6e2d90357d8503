"""Video evaluation on the GPU: FVD, the Frechet distance between I3D features of two sets of 32-frame sub-videos.

The video half of the reference's image-space evaluation (evaluation/evaluation.py, `calculate_fvd` over
evaluation/fvd/styleganv/fvd.py): every sub-video is resized and cropped to 224 x 224 (preprocess_single), passed through I3D
(Inception-v1 inflated to 3D, Kinetics-400: 57 convolutions with batch norm and ReLU, four max-pools outside and nine inside
the Mixed blocks, TensorFlow "SAME" padding) with `return_features=True`, and the 400 logits of the two sides enter the Frechet
distance.  Everything on the device is fp32 on the fp32 MFMA (csrc/conv3d.hip; include/m324.h has the arithmetic): the batch
norm is folded into the convolutions once, in float64, and the four branches of a Mixed block write their slices of the block's
output in place.  The distance itself is a few hundred numbers and runs on the host in float64.  The weights are the user's:
a state dict under the names of the common PyTorch port of I3D, or the TorchScript file the reference downloads.

    python -m motion324_amd.fvd --gt_paths A ... --result_paths B ... --weights i3d_torchscript.pt [--output_dir DIR]
"""
from __future__ import annotations

import argparse
import os
import zipfile
from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .lib import M324Error
from .perceptual import SUBVIDEO, load_frames, subvideo_frames

BN_EPS = 1e-3
CLASSES = 400
MIN_FRAMES = 10                         # the reference's assertion on a sub-video's length
TAPS = ("Conv3d_2c_3x3", "Mixed_3c", "Mixed_4f", "Mixed_5c")
# block: (input channels, (b0, b1a, b1b, b2a, b2b, b3b))
MIXED = {
    "Mixed_3b": (192, (64, 96, 128, 16, 32, 32)),
    "Mixed_3c": (256, (128, 128, 192, 32, 96, 64)),
    "Mixed_4b": (480, (192, 96, 208, 16, 48, 64)),
    "Mixed_4c": (512, (160, 112, 224, 24, 64, 64)),
    "Mixed_4d": (512, (128, 128, 256, 24, 64, 64)),
    "Mixed_4e": (512, (112, 144, 288, 32, 64, 64)),
    "Mixed_4f": (528, (256, 160, 320, 32, 128, 128)),
    "Mixed_5b": (832, (256, 160, 320, 32, 128, 128)),
    "Mixed_5c": (832, (384, 192, 384, 48, 128, 128)),
}
BRANCHES = ("b0", "b1a", "b1b", "b2a", "b2b", "b3b")
# the trunk in order: ("conv", unit, stride), ("pool", window, stride) or ("mixed", block)
TRUNK = (("conv", "Conv3d_1a_7x7", (2, 2, 2)), ("pool", (1, 3, 3), (1, 2, 2)), ("conv", "Conv3d_2b_1x1", (1, 1, 1)),
         ("conv", "Conv3d_2c_3x3", (1, 1, 1)), ("pool", (1, 3, 3), (1, 2, 2)), ("mixed", "Mixed_3b"), ("mixed", "Mixed_3c"),
         ("pool", (3, 3, 3), (2, 2, 2)), ("mixed", "Mixed_4b"), ("mixed", "Mixed_4c"), ("mixed", "Mixed_4d"), ("mixed", "Mixed_4e"),
         ("mixed", "Mixed_4f"), ("pool", (2, 2, 2), (2, 2, 2)), ("mixed", "Mixed_5b"), ("mixed", "Mixed_5c"))
# the stage a trunk step is timed under (tools/fvd_time.py): the stem, then the stages the pools open
STAGE_OF = ("stem", "stage2", "stage2", "stage2", "stage3", "stage3", "stage3", "stage4", "stage4", "stage4", "stage4", "stage4", "stage4",
            "stage5", "stage5", "stage5")
DEFAULT_MAX_SCRATCH_BYTES = 4 << 30


def _units():
    """{unit: (Cin, Cout, box)} of the 57 conv + batch-norm + ReLU units, in the order they run"""
    units = {"Conv3d_1a_7x7": (3, 64, 7), "Conv3d_2b_1x1": (64, 64, 1), "Conv3d_2c_3x3": (64, 192, 3)}
    for block, (cin, (b0, b1a, b1b, b2a, b2b, b3b)) in MIXED.items():
        for branch, ci, co, box in (("b0", cin, b0, 1), ("b1a", cin, b1a, 1), ("b1b", b1a, b1b, 3), ("b2a", cin, b2a, 1),
                                    ("b2b", b2a, b2b, 3), ("b3b", cin, b3b, 1)):
            units[f"{block}.{branch}"] = (ci, co, box)
    return units


UNITS = _units()
FEATURE_CHANNELS = 1024                 # Mixed_5c: 384 + 384 + 128 + 128
LOGITS = "logits.conv3d"


def mixed_width(block: str) -> int:
    b = MIXED[block][1]
    return b[0] + b[2] + b[4] + b[5]


class I3DWeights(NamedTuple):
    units: dict          # unit -> (wp fp32 [Kpad, Cout], bias fp32 [Cout]): batch norm folded, the K-major layout of ops.conv3d
    logits: tuple        # (w fp32 [1024, 400], b fp32 [400])


def fold_batch_norm(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """(w', b') in float64 with conv(x, w') + b' = batch_norm(conv(x, w)): w' = w gamma / sqrt(var + eps) per output channel,
    b' = beta - mean gamma / sqrt(var + eps)"""
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * scale.reshape(-1, 1, 1, 1, 1), beta.double() - mean.double() * scale


def _is_torchscript(path: str) -> bool:
    if not zipfile.is_zipfile(path):
        return False
    with zipfile.ZipFile(path) as z:
        return any("/code/" in n or n.endswith("constants.pkl") for n in z.namelist())


def _load_file(path: str) -> dict:
    if not os.path.isfile(path):
        raise M324Error(f"load_i3d_weights: no such file {path!r}")
    if _is_torchscript(path):
        return dict(torch.jit.load(path, map_location="cpu").state_dict())
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    if not isinstance(state, dict):
        raise M324Error(f"load_i3d_weights: {path!r} holds a {type(state).__name__}, not a state dict")
    return state


def _strip(key: str) -> str:
    while key.startswith(("module.", "model.")):
        key = key.split(".", 1)[1]
    return key


def load_i3d_weights(state_or_path) -> I3DWeights:
    """The 57 units and the logits layer, checked, folded and repacked once (CPU tensors; I3D(...) moves them to its device).
      * a state dict under the names of the common PyTorch port: <unit>.conv3d.weight and <unit>.bn.{weight, bias, running_mean,
        running_var} for Conv3d_1a_7x7, Conv3d_2b_1x1, Conv3d_2c_3x3 and Mixed_<3b..5c>.<b0, b1a, b1b, b2a, b2b, b3b>, and
        logits.conv3d.{weight, bias}; a missing bn.weight counts as ones; `module.` / `model.` prefixes are stripped and
        bn.num_batches_tracked is ignored;
      * the path of a file torch.load reads as such a dict;
      * the path of a TorchScript file (the reference's i3d_torchscript.pt), through torch.jit.load(...).state_dict().
    Every shape is checked; a missing key is named, and keys that match nothing are a refusal that lists them."""
    state = _load_file(os.fspath(state_or_path)) if isinstance(state_or_path, (str, os.PathLike)) else state_or_path
    if not isinstance(state, dict):
        raise M324Error("load_i3d_weights: expected a state dict or the path of one")
    state = {_strip(k): v for k, v in state.items() if not k.endswith("num_batches_tracked")}
    used = set()

    def tensor(key, shape, default=None):
        if key not in state:
            if default is not None:
                return default
            raise M324Error(f"load_i3d_weights: the state dict has no key {key!r}")
        used.add(key)
        t = state[key]
        t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
        if tuple(t.shape) != tuple(shape):
            raise M324Error(f"load_i3d_weights: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        if not torch.isfinite(t).all():
            raise M324Error(f"load_i3d_weights: {key!r} holds values that are not finite")
        return t.detach().cpu()

    units = {}
    for unit, (cin, cout, box) in UNITS.items():
        w = tensor(f"{unit}.conv3d.weight", (cout, cin, box, box, box))
        gamma = tensor(f"{unit}.bn.weight", (cout,), default=torch.ones(cout))
        beta, mean, var = (tensor(f"{unit}.bn.{k}", (cout,)) for k in ("bias", "running_mean", "running_var"))
        if (var < 0).any():
            raise M324Error(f"load_i3d_weights: {unit}.bn.running_var holds negative values")
        wf, bf = fold_batch_norm(w, gamma, beta, mean, var)
        units[unit] = (ops.pack_conv3d_weight(wf.to(torch.float32)), bf.to(torch.float32).contiguous())
    lw = tensor(LOGITS + ".weight", (CLASSES, FEATURE_CHANNELS, 1, 1, 1))
    lb = tensor(LOGITS + ".bias", (CLASSES,))
    foreign = sorted(set(state) - used)
    if foreign:
        raise M324Error(f"load_i3d_weights: {len(foreign)} keys match no part of I3D: {', '.join(foreign[:8])}" + (" ..." if len(foreign) > 8 else ""))
    return I3DWeights(units, (lw.reshape(CLASSES, FEATURE_CHANNELS).t().to(torch.float32).contiguous(), lb.to(torch.float32).contiguous()))


def synth_i3d_state_dict(seed: int) -> dict:
    """Seeded weights in the form of the PyTorch port's state dict, for tests and timing.  Convolutions randn * sqrt(2 / (k^3 Cin)),
    so that a unit keeps the second moment of a rectified input; batch norm with weight in [0.9, 1.1], bias and running mean
    0.1 randn and running variance in [0.8, 1.2]: about half of every tap's activations are alive and their RMS stays between 0.5
    and 1.5 through the 57 layers (tests/ERROR_BOUNDS_FVD.md has the numbers; a variance of [0.7, 1.1] already grows it twentyfold)."""
    g = torch.Generator().manual_seed(int(seed))
    state = {}
    for unit, (cin, cout, box) in UNITS.items():
        state[f"{unit}.conv3d.weight"] = torch.randn((cout, cin, box, box, box), generator=g) * (2.0 / (box ** 3 * cin)) ** 0.5
        state[f"{unit}.bn.weight"] = 0.9 + 0.2 * torch.rand((cout,), generator=g)
        state[f"{unit}.bn.bias"] = 0.1 * torch.randn((cout,), generator=g)
        state[f"{unit}.bn.running_mean"] = 0.1 * torch.randn((cout,), generator=g)
        state[f"{unit}.bn.running_var"] = 0.8 + 0.4 * torch.rand((cout,), generator=g)
    state[LOGITS + ".weight"] = torch.randn((CLASSES, FEATURE_CHANNELS, 1, 1, 1), generator=g) * (1.0 / FEATURE_CHANNELS) ** 0.5
    state[LOGITS + ".bias"] = 0.1 * torch.randn((CLASSES,), generator=g)
    return state


def trunk_shapes(T: int, H: int, W: int):
    """[(label, (T, H, W), channels)] of the trunk's input and of the map behind every trunk step, by the SAME rule"""
    size, c = (int(T), int(H), int(W)), 4
    shapes = [("input", size, c)]
    for step in TRUNK:
        if step[0] == "conv":
            size = tuple(ops.same_padding(n, UNITS[step[1]][2], s)[1] for n, s in zip(size, step[2]))
            c = UNITS[step[1]][1]
        elif step[0] == "pool":
            size = tuple(ops.same_padding(n, k, s)[1] for n, k, s in zip(size, step[1], step[2]))
        else:
            c = mixed_width(step[1])
        shapes.append((step[1] if step[0] != "pool" else "pool", size, c))
    return shapes


def scratch_bytes_per_video(T: int, H: int, W: int) -> int:
    """an upper bound of the activations one sub-video keeps alive at a time: a step's input and output, and inside a Mixed block
    the two reduced maps and the pooled copy of the input"""
    shapes = trunk_shapes(T, H, W)
    peak = 0
    for (_, s0, c0), (label, s1, c1) in zip(shapes[:-1], shapes[1:]):
        extra = 0
        if label in MIXED:
            b = MIXED[label][1]
            extra = (b[1] + b[3] + c0) * s1[0] * s1[1] * s1[2]
        peak = max(peak, c0 * s0[0] * s0[1] * s0[2] + c1 * s1[0] * s1[1] * s1[2] + extra)
    return 4 * peak


def trunk_macs(T: int, H: int, W: int) -> dict:
    """{stage: multiply-adds per sub-video} of the executed convolutions, K counted as the kernel runs it (the stem's padded
    fourth channel included), for the utilisation tools/fvd_time.py reports"""
    shapes = trunk_shapes(T, H, W)
    macs = {}
    for stage, (_, _, c0), (label, s1, _), step in zip(STAGE_OF, shapes[:-1], shapes[1:], TRUNK):
        vox = s1[0] * s1[1] * s1[2]
        if step[0] == "conv":
            cin, cout, box = UNITS[label]
            n = vox * box ** 3 * ((cin + 3) // 4 * 4) * cout
        elif step[0] == "mixed":
            n = sum(vox * UNITS[f"{label}.{b}"][2] ** 3 * UNITS[f"{label}.{b}"][0] * UNITS[f"{label}.{b}"][1] for b in BRANCHES)
        else:
            n = 0
        macs[stage] = macs.get(stage, 0) + n
    return macs


class I3D:
    """model = I3D(weights, device); model.features(videos) -> fp32 [N, 400] on the device, the logits before the softmax
    (the reference's return_features=True).  weights: an I3DWeights, or whatever load_i3d_weights accepts.  head_window: the
    (2, hw, hw) average window of the head, which the trunk's final map must match spatially: (2, 7, 7) for the published model on
    224 x 224 input.  resolution: the side the frames are resized and cropped to in front of the trunk (preprocess_single), 32 hw
    by default; None takes the frames at their own size."""

    def __init__(self, weights, device="cuda", head_window=(2, 7, 7), resolution="auto"):
        if not isinstance(weights, I3DWeights):
            weights = load_i3d_weights(weights)
        head_window = tuple(int(v) for v in head_window)
        if len(head_window) != 3 or head_window[0] != 2 or head_window[1] != head_window[2] or not 1 <= head_window[1] <= ops.I3D_HEAD_MAX_SIDE:
            raise M324Error(f"I3D: head_window must be (2, hw, hw) with hw in 1..{ops.I3D_HEAD_MAX_SIDE}, got {head_window}")
        self.head_window = head_window
        self.resolution = 32 * head_window[1] if resolution == "auto" else (None if resolution is None else int(resolution))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise M324Error("I3D: needs a HIP device (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.units = {k: (wp.to(self.device), b.to(self.device)) for k, (wp, b) in weights.units.items()}
        self.logits = tuple(t.to(self.device) for t in weights.logits)

    def check_videos(self, videos):
        """(N, T, trunk input H, W) of a batch of sub-videos this model accepts, or an M324Error that names the sizes.  Host-only."""
        if not isinstance(videos, torch.Tensor) or videos.dim() != 5 or videos.shape[4] != 3 or videos.dtype not in (torch.uint8, torch.float32) \
                or 0 in videos.shape:
            raise M324Error("I3D: expected sub-videos uint8 [N,T,H,W,3], or fp32 in [0, 1] of that shape, got "
                            + (f"{videos.dtype} {tuple(videos.shape)}" if isinstance(videos, torch.Tensor) else type(videos).__name__))
        N, T, H, W = (int(v) for v in videos.shape[:4])
        if T < MIN_FRAMES:
            raise M324Error(f"I3D: a sub-video needs at least {MIN_FRAMES} frames, got {T}")
        Hi, Wi = ops.fvd_geometry(H, W, self.resolution)[4:]
        final = trunk_shapes(T, Hi, Wi)[-1][1]
        if final[1:] != self.head_window[1:] or final[0] < 2:
            raise M324Error(f"I3D: {H} x {W} frames enter the trunk as {Hi} x {Wi} and reach a final map of {final[1]} x {final[2]} over "
                            f"{final[0]} time steps; the head's window is {self.head_window}")
        return N, T, Hi, Wi

    def features(self, videos, *, taps: bool = False, max_scratch_bytes: int = DEFAULT_MAX_SCRATCH_BYTES, stage_events=None):
        """videos: uint8 [N,T,H,W,3] or fp32 in [0, 1] of that shape on the model's device, T >= 10.  Returns fp32 [N,400]; with
        taps also {name: fp32 NDHWC map} behind Conv3d_2c_3x3, Mixed_3c, Mixed_4f and Mixed_5c.  The sub-videos pass the trunk in
        chunks whose activations stay under max_scratch_bytes; a sub-video's result does not depend on the chunking or on its
        place in the batch.  Nothing synchronises.  stage_events: a list that receives (label, start, end) device events per
        stage of every chunk (tools/fvd_time.py)."""
        N, T, Hi, Wi = self.check_videos(videos)
        if not videos.is_cuda or videos.device != self.device:
            raise M324Error(f"I3D: the sub-videos must be on {self.device} (there is no CPU path)")
        per = scratch_bytes_per_video(T, Hi, Wi)
        if per > int(max_scratch_bytes):
            raise M324Error(f"I3D: one sub-video of {T} x {Hi} x {Wi} needs {per} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
        n = max(1, min(N, int(max_scratch_bytes) // per))
        out = torch.empty((N, CLASSES), dtype=torch.float32, device=self.device)
        kept = {k: [] for k in TAPS} if taps else None
        for i in range(0, N, n):
            self._chunk(videos[i:i + n], out[i:i + n], kept, stage_events)
        return (out, {k: torch.cat(v) for k, v in kept.items()}) if taps else out

    def _unit(self, unit, x, stride=(1, 1, 1), out=None):
        wp, b = self.units[unit]
        return ops.conv3d(x, wp, b, box=UNITS[unit][2], stride=stride, relu=True, out=out)

    def _mixed(self, block, x):
        """the four branches write their slices of the block's output in place: no concatenation, no copy"""
        b0, _, b1b, _, b2b, b3b = MIXED[block][1]
        y = torch.empty(tuple(x.shape[:4]) + (b0 + b1b + b2b + b3b,), dtype=torch.float32, device=x.device)
        self._unit(f"{block}.b0", x, out=y[..., :b0])
        self._unit(f"{block}.b1b", self._unit(f"{block}.b1a", x), out=y[..., b0:b0 + b1b])
        self._unit(f"{block}.b2b", self._unit(f"{block}.b2a", x), out=y[..., b0 + b1b:b0 + b1b + b2b])
        self._unit(f"{block}.b3b", ops.maxpool3d(x, (3, 3, 3), (1, 1, 1)), out=y[..., b0 + b1b + b2b:])
        return y

    def _chunk(self, videos, out, kept, stage_events):
        def event():
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        def timed(label, start):
            if stage_events is not None:
                stage_events.append((label, start, event()))
            return event() if stage_events is not None else None

        start = event() if stage_events is not None else None
        x = ops.fvd_prepare(videos, self.resolution)
        start = timed("prepare", start)
        for i, step in enumerate(TRUNK):
            if step[0] == "conv":
                x = self._unit(step[1], x, stride=step[2])
            elif step[0] == "pool":
                x = ops.maxpool3d(x, step[1], step[2])
            else:
                x = self._mixed(step[1], x)
            if kept is not None and step[1] in TAPS:
                kept[step[1]].append(x)
            if i + 1 == len(TRUNK) or STAGE_OF[i + 1] != STAGE_OF[i]:
                start = timed(STAGE_OF[i], start)
        ops.i3d_head(x, self.logits[0], self.logits[1], out=out)
        timed("head", start)


def frechet_distance(feats_fake, feats_real) -> float:
    """The reference's frechet_distance of two feature sets [N, d], on the host in float64 with numpy only.  N == 1: the squared
    distance of the two rows, as the reference does.  N > 1: |mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr sqrt(S1 S2) with np.cov's
    N - 1 normalisation, where tr sqrt(S1 S2) is the sum of the singular values of A2 A1^T, A = centred feats / sqrt(N - 1): S = A^T A,
    so the non-zero eigenvalues of S1 S2 are those of (A2 A1^T)^T (A2 A1^T), the squared singular values.  The identity is exact
    and needs no matrix square root.  Deviation from the reference: for N <= d (N sub-videos against d = 400, the usual case) S1 S2
    is rank-deficient and scipy's sqrtm of it returns noise of the size of the result with a warning; this value is the one that
    formula defines.  Two equal sets have distance 0.0 exactly."""
    f1, f2 = (np.asarray(f, dtype=np.float64) for f in (feats_fake, feats_real))
    if f1.ndim != 2 or f2.ndim != 2 or f1.shape[1] != f2.shape[1] or f1.shape[0] < 1 or f2.shape[0] < 1:
        raise M324Error(f"frechet_distance: expected two feature sets [N, d] of one d, got {f1.shape} and {f2.shape}")
    if (f1.shape[0] == 1) != (f2.shape[0] == 1):
        raise M324Error(f"frechet_distance: one set has a single row, the other {max(f1.shape[0], f2.shape[0])}: a single row has no covariance")
    if not (np.isfinite(f1).all() and np.isfinite(f2).all()):
        raise M324Error("frechet_distance: the features hold values that are not finite")
    if f1.shape == f2.shape and np.array_equal(f1, f2):
        return 0.0
    mu1, mu2 = f1.mean(axis=0), f2.mean(axis=0)
    m = float(np.square(mu1 - mu2).sum())
    if f1.shape[0] == 1:
        return m
    a1 = (f1 - mu1) / np.sqrt(f1.shape[0] - 1)
    a2 = (f2 - mu2) / np.sqrt(f2.shape[0] - 1)
    cross = np.linalg.svd(a2 @ a1.T, compute_uv=False).sum()
    return float(m + np.square(a1).sum() + np.square(a2).sum() - 2.0 * cross)


class FvdScore(NamedTuple):
    value: float                # frechet_distance(result features, gt features)
    feats_result: np.ndarray    # [n_sub, 400] float64
    feats_gt: np.ndarray


def check_clip_pair(gt, result, name: str = "evaluate_clips_fvd") -> int:
    """T of two clips uint8 [T,H,W,3] of one shape, or an M324Error.  Host-only."""
    for x in (gt, result):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.uint8 or x.shape[3] != 3:
            raise M324Error(f"{name}: expected uint8 [T,H,W,3] clips")
    if tuple(gt.shape) != tuple(result.shape):
        raise M324Error(f"{name}: the clips must have equal shapes, got {tuple(gt.shape)} and {tuple(result.shape)}")
    return int(gt.shape[0])


def evaluate_clips_fvd(gt, result, model: I3D, **kw) -> FvdScore:
    """Scores `result` against `gt` as the reference's evaluation.py does for FVD: both clips are cut into 32-frame sub-videos by
    perceptual.subvideo_frames (a short clip is extended by its reversed tail), the N sub-videos of each side give N feature rows,
    and the value is frechet_distance(result rows, gt rows).  The one synchronisation is the copy of the features to the host."""
    T = check_clip_pair(gt, result)
    index = torch.as_tensor(subvideo_frames(T), dtype=torch.long, device=gt.device)        # refuses T < 16 before any work
    both = torch.cat([result[index], gt[index]])
    feats = model.features(both, **kw).double().cpu().numpy()
    n = index.shape[0]
    return FvdScore(frechet_distance(feats[:n], feats[n:]), feats[:n], feats[n:])


def main(argv=None):
    parser = argparse.ArgumentParser(description="FVD (I3D, Kinetics-400) between ground-truth and result clips on the GPU")
    parser.add_argument("--gt_paths", type=str, required=True, nargs="+", help="frame directories or .npy clips")
    parser.add_argument("--result_paths", type=str, required=True, nargs="+")
    parser.add_argument("--weights", type=str, required=True, help="i3d_torchscript.pt, or a state dict of the PyTorch port of I3D")
    parser.add_argument("--output_dir", type=str, default=None)
    args = parser.parse_args(argv)
    if len(args.gt_paths) != len(args.result_paths):
        raise M324Error(f"{len(args.gt_paths)} gt paths but {len(args.result_paths)} result paths: pairs are matched by position")
    weights = load_i3d_weights(args.weights)
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.fvd needs a HIP device (there is no CPU path)")
    model = I3D(weights, "cuda")
    results = []
    for gt_path, result_path in zip(args.gt_paths, args.result_paths):
        missing = [p for p in (gt_path, result_path) if not os.path.exists(p)]
        if missing:
            print(f"Warning: {missing[0]} not found, skipping")
            continue
        gt, result = (torch.from_numpy(load_frames(p)).to("cuda") for p in (gt_path, result_path))
        score = evaluate_clips_fvd(gt, result, model)
        results.append(score.value)
        base = os.path.basename(result_path.rstrip("/"))
        if os.path.isfile(result_path):
            base = os.path.splitext(base)[0]
        out_dir = args.output_dir if args.output_dir else os.path.dirname(result_path.rstrip("/"))
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        out_file = os.path.join(out_dir, base + ".txt")
        with open(out_file, "w") as f:
            f.write(f"GT Source: {gt_path}\nResult Source: {result_path}\nFVD: {score.value}\n" + "-" * 50 + "\n")
        print(f"{result_path}: FVD {score.value:.6f} ({len(score.feats_gt)} sub-video(s)) -> {out_file}")
    print(f"Summary: processed {len(results)}/{len(args.gt_paths)} pairs" + (f"; Average FVD: {np.mean(results):.6f}" if results else ""))
    return results


if __name__ == "__main__":
    main()
