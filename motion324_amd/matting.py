"""Foreground matting on the GPU: U2-Net or ISNet from raw frames to a masked clip.

replaces: utils/inference_utils.py:segment_foreground_with_u2net of the reference -- a Python loop with one
`rembg.remove(frame, session='u2net')` per frame (onnxruntime, a PIL round trip) -- which scripts/inference_with_video_mesh.py
calls just before run_model_inference.  Per frame, what `rembg` does and what runs here:

  1. resize to size x size (320) with Pillow's 8-bit Lanczos            ops.frame_resample, two passes (framing.resample_tables)
  2. divide by the frame's largest byte, ImageNet mean / deviation        ops.matte_prepare (float64, rounded once: numpy's bits)
  3. U2-Net, the first output sigmoid(d0)                                 U2Net below: ops.conv3x3_ex on the fp32 MFMA, the
                                                                          ceil-mode pool, the bilinear upsample, ops.matte_fuse
  4. (p - min) / (max - min) * 255, truncated to a byte                   ops.matte_quantise
  5. resize the 8-bit mask back to W x H with Lanczos                     ops.frame_resample, one channel
  6. Image.composite(img, empty, mask), then rgb * (alpha / 255)          one 256 x 256 table (cutout_table), ops.frame_mask soft mode

The network is the published `u2net.py` (U-2-Net; variants u2net, u2netp; u2net_human_seg has u2net's layout).  The weights are
the user's: the `.pth` state dict of that module.  Eval-mode batch-norm is folded into the convolution in float64 on the host and
the result rounded ONCE to fp32 (fold_batchnorm); that rounding, and fp32 convolutions summed in another order than the ONNX
runtime's, are why the matte can differ from rembg's in the last level of a pixel whose value lies next to an integer.
Differences from `rembg` that are decisions: a frame whose probabilities are all equal (numpy: 0 / 0 = NaN, an undefined cast) has
alpha 0; `post_process_mask` and alpha matting (both off by default there) are not provided; ONNX files are not read.  From the
320 x 320 mask on, every byte equals what Pillow and numpy give for that mask.

ISNet (the IS-Net of DIS, `isnet.py`, class ISNetDIS; `rembg`'s session 'isnet-general-use', which the reference's
utils/rmbg_for_black_bg.py:26 and scripts/hunyuan_Gen.py:39 select) is the same pipeline around another network: 1024 x 1024 in
step 1, the mean (0.485, 0.456, 0.406) with a deviation of (1, 1, 1) in step 2, and in step 3 a stride-2 stem (ops.conv3x3_s2), the
same eleven RSU blocks with stage1 reading 64 channels, and sigmoid(d1) of the one side map that is used (ops.matte_side).
matte_video(video, ISNet(...)) followed by framing.frame_video(video, alpha) in its threshold mode is rmbg_for_black_bg.py on the
device.  Neither `rembg` nor the published isnet-general-use.pth was at hand when this was written: the network, the constants and
the input size are as read from the published module and package, and the constants are parameters of ISNet(...) for that reason.

    python -m motion324_amd.matting --video DIR|clip.npy --weights u2net.pth|isnet.pth --out DIR [--size S] [--frame 512 [--frame_mode threshold]]
"""
from __future__ import annotations

import argparse
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import framing, ops
from .lib import M324Error
from .ops import pack_conv_weight

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BN_EPS = 1e-5
SIZE = 320
# stage: (kind, in, mid, out); kind 7, 6, 5, 4 = RSU-L, "4F" = the dilated block without pools
VARIANTS = {
    "u2net": {"stage1": (7, 3, 32, 64), "stage2": (6, 64, 32, 128), "stage3": (5, 128, 64, 256), "stage4": (4, 256, 128, 512),
              "stage5": ("4F", 512, 256, 512), "stage6": ("4F", 512, 256, 512), "stage5d": ("4F", 1024, 256, 512),
              "stage4d": (4, 1024, 128, 256), "stage3d": (5, 512, 64, 128), "stage2d": (6, 256, 32, 64), "stage1d": (7, 128, 16, 64)},
    "u2netp": {"stage1": (7, 3, 16, 64), "stage2": (6, 64, 16, 64), "stage3": (5, 64, 16, 64), "stage4": (4, 64, 16, 64),
               "stage5": ("4F", 64, 16, 64), "stage6": ("4F", 64, 16, 64), "stage5d": ("4F", 128, 16, 64),
               "stage4d": (4, 128, 16, 64), "stage3d": (5, 128, 16, 64), "stage2d": (6, 128, 16, 64), "stage1d": (7, 128, 16, 64)},
}
SIDE_CHANNELS = {"u2net": (64, 64, 128, 256, 512, 512), "u2netp": (64,) * 6}      # side1..6 read hx1d, hx2d, hx3d, hx4d, hx5d, hx6
PARAMETERS = {"u2net": 44009869, "u2netp": 1131181}                               # trainable, as published
TAPS = ("hx1", "hx2", "hx3", "hx4", "hx5", "hx6", "hx5d", "hx4d", "hx3d", "hx2d", "hx1d")
# Live activations of one frame, in floats per pixel of the size x size input, as an upper estimate: at full resolution stage1d
# holds hx1 and the upsampled hx2d (64 each), its hxin (64), hx1 and an upsampled decoder map (16 each), its result (64) and the
# input (4), 292; the trunk's taps at 1/4, 1/16, ... of the pixels and the block's own pyramid add about 70.
FLOATS_PER_FRAME_PIXEL = 512
DEFAULT_MAX_SCRATCH_BYTES = 8 << 30     # 40 frames of 320 x 320 per chunk: a 32-frame window in one; the sweep is in profiles/matting.md

# ISNet: U2-Net's table with stage1 reading the 64 channels of the stem conv_in = Conv2d(3, 64, 3, stride=2, padding=1), which no
# batch-norm and no ReLU follow; the module's pool_in is not used in its forward.  No outconv: d1 of side1 alone is the output.
ISNET_STAGES = dict(VARIANTS["u2net"], stage1=(7, 64, 32, 64))
ISNET_STEM = (3, 64)
ISNET_SIDE_CHANNELS = SIDE_CHANNELS["u2net"]
ISNET_PARAMETERS = 44046790             # U2-Net's 44,009,869 + 35,136 (the wider stage1.rebnconvin) + 1,792 (conv_in) - 7 (outconv)
ISNET_SIZE = 1024
ISNET_MEAN = (0.485, 0.456, 0.406)      # the DIS session of `rembg`, as read from the package: parameters of ISNet(...), not literals
ISNET_STD = (1.0, 1.0, 1.0)
ISNET_TAPS = ("hxin",) + TAPS
# Live activations of one frame in floats per pixel of the size x size INPUT, as an upper estimate.  Everything behind the stem
# has a quarter of the input's pixels.  Per pixel of that half-size map, at the widest point (stage1d): hx1 and the upsampled hx2d
# (64 each), the block's hxin (64), its hx1 and an upsampled decoder map (16 each), its result (64) and the stem's output, which
# stays alive as a tap (64): 352; the trunk's taps at 1/4, 1/16, ... of those pixels and the block's own pyramid add about 70:
# 422, a quarter of which is 106 per input pixel.  The input (4), the side map, the probabilities and the bytes add about 7: 113,
# taken with the headroom U2-Net's figure has over its own count (512 over 362).  tools/matting_time.py --model isnet sets the
# allocator's peak against it (profiles/matting_isnet.md).
ISNET_FLOATS_PER_FRAME_PIXEL = 160


def stage_layers(kind, cin: int, mid: int, cout: int):
    """[(name, in channels, out channels, dilation)] of one RSU block, in the order the block runs them"""
    if kind == "4F":
        return [("rebnconvin", cin, cout, 1), ("rebnconv1", cout, mid, 1), ("rebnconv2", mid, mid, 2), ("rebnconv3", mid, mid, 4),
                ("rebnconv4", mid, mid, 8), ("rebnconv3d", 2 * mid, mid, 4), ("rebnconv2d", 2 * mid, mid, 2), ("rebnconv1d", 2 * mid, cout, 1)]
    L = int(kind)
    layers = [("rebnconvin", cin, cout, 1), ("rebnconv1", cout, mid, 1)]
    layers += [(f"rebnconv{k}", mid, mid, 1) for k in range(2, L)]
    layers += [(f"rebnconv{L}", mid, mid, 2)]
    layers += [(f"rebnconv{k}d", 2 * mid, mid, 1) for k in range(L - 1, 1, -1)]
    layers += [("rebnconv1d", 2 * mid, cout, 1)]
    return layers


def network_layers(variant: str):
    """[(key prefix "stage.rebnconv", in, out, dilation)] of all 112 REBNCONV layers of a variant"""
    if variant not in VARIANTS:
        raise M324Error(f"U2-Net: variant must be one of {sorted(VARIANTS)}, got {variant!r}")
    return [(f"{stage}.{name}", cin, cout, d) for stage, spec in VARIANTS[variant].items() for name, cin, cout, d in stage_layers(*spec)]


def state_dict_keys(variant: str):
    """{key: shape} of every tensor load_u2net_weights reads (num_batches_tracked is ignored)"""
    keys = {}
    for prefix, cin, cout, _ in network_layers(variant):
        keys[prefix + ".conv_s1.weight"] = (cout, cin, 3, 3)
        keys[prefix + ".conv_s1.bias"] = (cout,)
        for name in ("weight", "bias", "running_mean", "running_var"):
            keys[f"{prefix}.bn_s1.{name}"] = (cout,)
    for k, c in enumerate(SIDE_CHANNELS[variant]):
        keys[f"side{k + 1}.weight"] = (1, c, 3, 3)
        keys[f"side{k + 1}.bias"] = (1,)
    keys["outconv.weight"] = (1, 6, 1, 1)
    keys["outconv.bias"] = (1,)
    return keys


def parameter_count(variant: str) -> int:
    """trainable parameters: everything but the batch-norm running statistics"""
    return sum(int(np.prod(shape)) for key, shape in state_dict_keys(variant).items() if "running_" not in key)


class U2NetWeights(NamedTuple):
    variant: str
    layers: dict         # "stage1.rebnconvin" -> (wp fp32 [Kpad, Cout], bias fp32 [Cout], dilation): batch-norm folded, ops.conv3x3_ex's layout
    sides: tuple         # six (wp fp32 [Kpad, 4], bias fp32 [4]): column 0 is the side output, columns 1..3 are zero
    outconv: tuple       # seven floats: the 1 x 1 convolution over the six side maps, and its bias


def fold_batchnorm(w, b, gamma, beta, mean, var, eps: float = BN_EPS):
    """Conv2d followed by eval-mode BatchNorm2d as one convolution: w' = w g, b' = (b - mean) g + beta with g = gamma / sqrt(var +
    eps), evaluated in float64 and rounded ONCE to fp32 -- the one place where these weights leave the user's values."""
    g = gamma.double() / torch.sqrt(var.double() + eps)
    return (w.double() * g.reshape(-1, 1, 1, 1)).to(torch.float32), ((b.double() - mean.double()) * g + beta.double()).to(torch.float32)


def _load_file(path: str, who: str = "load_u2net_weights", module: str = "U-2-Net") -> dict:
    if not os.path.isfile(path):
        raise M324Error(f"{who}: no such file {path!r}")
    if path.lower().endswith(".onnx"):
        raise M324Error(f"{who}: {path!r} is an ONNX file; the `.pth` state dict of the published {module} module is needed")
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    if not isinstance(state, dict):
        raise M324Error(f"{who}: {path!r} holds a {type(state).__name__}, not a state dict")
    return state


def _tensor(state, key: str, shape, who: str = "load_u2net_weights") -> torch.Tensor:
    if key not in state:
        raise M324Error(f"{who}: the state dict has no key {key!r}")
    t = state[key]
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
    if tuple(t.shape) != tuple(shape):
        raise M324Error(f"{who}: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not torch.isfinite(t).all():
        raise M324Error(f"{who}: {key!r} holds values that are not finite")
    return t.detach().cpu()


def _folded_layers(get, layers, who: str) -> dict:
    """{prefix: (wp, bias, dilation)} of REBNCONV layers [(prefix, in, out, dilation)]: batch-norm folded, repacked"""
    out = {}
    for prefix, _, _, dilation in layers:
        w, b = fold_batchnorm(get(prefix + ".conv_s1.weight"), get(prefix + ".conv_s1.bias"), get(prefix + ".bn_s1.weight"), get(prefix + ".bn_s1.bias"),
                              get(prefix + ".bn_s1.running_mean"), get(prefix + ".bn_s1.running_var"))
        if not (torch.isfinite(w).all() and torch.isfinite(b).all()):
            raise M324Error(f"{who}: folding the batch-norm of {prefix!r} gives values that are not finite (running_var + eps <= 0?)")
        out[prefix] = (pack_conv_weight(w), b.contiguous(), dilation)
    return out


def _packed_sides(get) -> tuple:
    """six (wp [Kpad, 4], bias [4]): the one-channel side convolutions with zero columns up to four"""
    sides = []
    for k in range(6):
        wp = pack_conv_weight(get(f"side{k + 1}.weight"))
        sides.append((torch.nn.functional.pad(wp, (0, 3)).contiguous(), torch.nn.functional.pad(get(f"side{k + 1}.bias").to(torch.float32), (0, 3)).contiguous()))
    return tuple(sides)


def infer_variant(state) -> str:
    key = "stage1.rebnconv1.conv_s1.weight"
    if key not in state:
        raise M324Error(f"load_u2net_weights: the state dict has no key {key!r}")
    mid = int(state[key].shape[0])
    for variant, stages in VARIANTS.items():
        if stages["stage1"][2] == mid:
            return variant
    raise M324Error(f"load_u2net_weights: {key!r} has {mid} output channels; u2net has 32 and u2netp 16")


def load_u2net_weights(state_or_path, variant: Optional[str] = None) -> U2NetWeights:
    """The state dict of the published U2NET / U2NETP module (stage1.rebnconvin.conv_s1.weight ... outconv.bias), or the path of
    a `.pth` holding it, checked, folded and repacked once (CPU tensors; U2Net(...) moves them to its device).  The variant is
    inferred from the shapes unless given.  A missing or mis-shaped key is named in the error."""
    state = _load_file(os.fspath(state_or_path)) if isinstance(state_or_path, (str, os.PathLike)) else state_or_path
    if not isinstance(state, dict):
        raise M324Error("load_u2net_weights: expected a state dict or the path of one")
    if "outconv.weight" not in state:       # first, so that an IS-Net dict (which has every stage key, one of another shape) is refused by what it lacks
        raise M324Error("load_u2net_weights: the state dict has no key 'outconv.weight' (an IS-Net state dict has none: load_isnet_weights reads it)")
    variant = infer_variant(state) if variant is None else variant
    shapes = state_dict_keys(variant)
    get = lambda key: _tensor(state, key, shapes[key])
    layers = _folded_layers(get, network_layers(variant), "load_u2net_weights")
    sides = _packed_sides(get)
    outconv = tuple(float(v) for v in get("outconv.weight").to(torch.float32).reshape(6)) + (float(get("outconv.bias").to(torch.float32)[0]),)
    return U2NetWeights(variant, layers, sides, outconv)


def synth_u2net_state_dict(variant: str, seed: int, side_gain: float = 1.0, outconv_bias: float = 0.0) -> dict:
    """Seeded weights in the form of the published state dict, for tests and timing: convolutions randn * sqrt(2 / (9 Cin)), biases
    0.05 randn, batch-norm scale 1 + 0.1 randn, shift 0.05 randn, running mean 0.1 randn and variance in 0.75 .. 1.25.  The residual
    sums let the taps grow to some tens through the eleven blocks, and the logits with them: side_gain scales the side weights and
    outconv_bias shifts the logits, for a caller that needs a matte without saturated plateaus (tests/matting_cases.py)."""
    g = torch.Generator().manual_seed(int(seed))
    state = {}
    for prefix, cin, cout, _ in network_layers(variant):
        state[prefix + ".conv_s1.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * math.sqrt(2.0 / (9 * cin))
        state[prefix + ".conv_s1.bias"] = 0.05 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.weight"] = 1.0 + 0.1 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.bias"] = 0.05 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.running_mean"] = 0.1 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.running_var"] = 0.75 + 0.5 * torch.rand((cout,), generator=g)
        state[prefix + ".bn_s1.num_batches_tracked"] = torch.tensor(1000)
    for k, c in enumerate(SIDE_CHANNELS[variant]):
        state[f"side{k + 1}.weight"] = torch.randn((1, c, 3, 3), generator=g) * (side_gain * math.sqrt(2.0 / (9 * c)))
        state[f"side{k + 1}.bias"] = 0.05 * torch.randn((1,), generator=g)
    state["outconv.weight"] = (0.5 + torch.rand((1, 6, 1, 1), generator=g)) * torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, -1.0]).reshape(1, 6, 1, 1)
    state["outconv.bias"] = outconv_bias + 0.05 * torch.randn((1,), generator=g)
    return state


def isnet_layers():
    """[(key prefix "stage.rebnconv", in, out, dilation)] of the 112 REBNCONV layers of ISNet"""
    return [(f"{stage}.{name}", cin, cout, d) for stage, spec in ISNET_STAGES.items() for name, cin, cout, d in stage_layers(*spec)]


def isnet_state_dict_keys():
    """{key: shape} of every tensor load_isnet_weights reads, in the module's order: conv_in, the stages, side1..side6"""
    keys = {"conv_in.weight": (ISNET_STEM[1], ISNET_STEM[0], 3, 3), "conv_in.bias": (ISNET_STEM[1],)}
    for prefix, cin, cout, _ in isnet_layers():
        keys[prefix + ".conv_s1.weight"] = (cout, cin, 3, 3)
        keys[prefix + ".conv_s1.bias"] = (cout,)
        for name in ("weight", "bias", "running_mean", "running_var"):
            keys[f"{prefix}.bn_s1.{name}"] = (cout,)
    for k, c in enumerate(ISNET_SIDE_CHANNELS):
        keys[f"side{k + 1}.weight"] = (1, c, 3, 3)
        keys[f"side{k + 1}.bias"] = (1,)
    return keys


def isnet_parameter_count() -> int:
    return sum(int(np.prod(shape)) for key, shape in isnet_state_dict_keys().items() if "running_" not in key)


class ISNetWeights(NamedTuple):
    conv_in: tuple       # (wp fp32 [Kpad, 64], bias fp32 [64]) of the stride-2 stem, as the file has them: there is no batch-norm to fold
    layers: dict         # as U2NetWeights.layers
    sides: tuple         # as U2NetWeights.sides; all six are validated, the network computes the first


def load_isnet_weights(state_or_path) -> ISNetWeights:
    """The state dict of the published ISNetDIS module (conv_in.weight, conv_in.bias, stage1.rebnconvin.conv_s1.weight ...
    side6.bias), or the path of a `.pth` holding it, checked, folded and repacked once.  A missing or mis-shaped key is named in
    the error; side2..side6 are read so that a wrong file is refused, although the network never computes them."""
    who = "load_isnet_weights"
    state = _load_file(os.fspath(state_or_path), who, "IS-Net (isnet.py, ISNetDIS)") if isinstance(state_or_path, (str, os.PathLike)) else state_or_path
    if not isinstance(state, dict):
        raise M324Error(f"{who}: expected a state dict or the path of one")
    shapes = isnet_state_dict_keys()
    get = lambda key: _tensor(state, key, shapes[key], who)
    conv_in = (pack_conv_weight(get("conv_in.weight")), get("conv_in.bias").to(torch.float32).contiguous())
    return ISNetWeights(conv_in, _folded_layers(get, isnet_layers(), who), _packed_sides(get))


def synth_isnet_state_dict(seed: int, side_gain: float = 1.0, side_bias: float = 0.0) -> dict:
    """Seeded weights in the form of the published ISNetDIS state dict, drawn as synth_u2net_state_dict draws them in the order
    conv_in, stages, sides.  side_gain scales the side weights and side_bias shifts the logits."""
    g = torch.Generator().manual_seed(int(seed))
    cin, cout = ISNET_STEM
    state = {"conv_in.weight": torch.randn((cout, cin, 3, 3), generator=g) * math.sqrt(2.0 / (9 * cin)), "conv_in.bias": 0.05 * torch.randn((cout,), generator=g)}
    for prefix, cin, cout, _ in isnet_layers():
        state[prefix + ".conv_s1.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * math.sqrt(2.0 / (9 * cin))
        state[prefix + ".conv_s1.bias"] = 0.05 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.weight"] = 1.0 + 0.1 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.bias"] = 0.05 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.running_mean"] = 0.1 * torch.randn((cout,), generator=g)
        state[prefix + ".bn_s1.running_var"] = 0.75 + 0.5 * torch.rand((cout,), generator=g)
        state[prefix + ".bn_s1.num_batches_tracked"] = torch.tensor(1000)
    for k, c in enumerate(ISNET_SIDE_CHANNELS):
        state[f"side{k + 1}.weight"] = torch.randn((1, c, 3, 3), generator=g) * (side_gain * math.sqrt(2.0 / (9 * c)))
        state[f"side{k + 1}.bias"] = side_bias + 0.05 * torch.randn((1,), generator=g)
    return state


def is_isnet_state(state) -> bool:
    """conv_in.weight present: the file is ISNet's (the command line infers the network from it)"""
    return isinstance(state, dict) and "conv_in.weight" in state


class _RSUNet:
    """What U2Net and ISNet share: the device, the folded layers, and the eleven RSU blocks of a stage table with the pools,
    upsamples and concatenations between them."""
    name = "RSUNet"

    def __init__(self, stages: dict, layers: dict, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise M324Error(f"{self.name}: needs a HIP device (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.stages = stages
        self.layers = {k: (wp.to(self.device), b.to(self.device), d) for k, (wp, b, d) in layers.items()}

    def _check_input(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != self.device:
            raise M324Error(f"{self.name}: the input must be on {self.device} (there is no CPU path)")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[3] != 4 or 0 in x.shape:
            raise M324Error(f"{self.name}: expected fp32 NHWC [T,H,W,4] (ops.matte_prepare writes it), got {x.dtype} {tuple(x.shape)}")

    def _conv(self, name, a, b=None, res=None):
        wp, bias, dilation = self.layers[name]
        return ops.conv3x3_ex(a, wp, bias, b=b, dilation=dilation, relu=True, res=res)

    @staticmethod
    def _up(x, like):
        return x if x.shape[1:3] == like.shape[1:3] else ops.upsample_bilinear(x, like.shape[1:3])      # equal sizes: the resize is the identity

    def _rsu(self, stage, a, b=None):
        kind = self.stages[stage][0]
        conv = lambda name, *args, **kw: self._conv(f"{stage}.{name}", *args, **kw)
        hxin = conv("rebnconvin", a, b)
        if kind == "4F":
            hx1 = conv("rebnconv1", hxin)
            hx2 = conv("rebnconv2", hx1)
            hx3 = conv("rebnconv3", hx2)
            hx4 = conv("rebnconv4", hx3)
            d = conv("rebnconv3d", hx4, hx3)
            d = conv("rebnconv2d", d, hx2)
            return conv("rebnconv1d", d, hx1, res=hxin)
        L = int(kind)
        hx = [None, conv("rebnconv1", hxin)]
        for k in range(2, L):
            hx.append(conv(f"rebnconv{k}", ops.maxpool2x2_ceil(hx[k - 1])))
        d = conv(f"rebnconv{L - 1}d", conv(f"rebnconv{L}", hx[L - 1]), hx[L - 1])
        for k in range(L - 2, 1, -1):
            d = conv(f"rebnconv{k}d", self._up(d, hx[k]), hx[k])
        return conv("rebnconv1d", self._up(d, hx[1]), hx[1], res=hxin)

    def _trunk(self, x, stage_events=None) -> dict:
        """{hx1..hx6, hx5d..hx1d} of the eleven blocks on x, the input of stage1.  stage_events: a list that receives (stage, start,
        end) device events (tools/matting_time.py)."""
        def run(stage, a, b=None):
            if stage_events is None:
                return self._rsu(stage, a, b)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            y = self._rsu(stage, a, b)
            end.record()
            stage_events.append((stage, start, end))
            return y

        t = {}
        t["hx1"] = run("stage1", x)
        for k in range(2, 7):
            t[f"hx{k}"] = run(f"stage{k}", ops.maxpool2x2_ceil(t[f"hx{k - 1}"]))
        d = t["hx6"]
        for k in range(5, 0, -1):
            d = t[f"hx{k}d"] = run(f"stage{k}d", self._up(d, t[f"hx{k}"]), t[f"hx{k}"])
        return t

    @staticmethod
    def _result(prob, logit, return_logits: bool, taps):
        result = (prob, logit) if return_logits else (prob,)
        if taps is not None:
            result += (taps,)
        return result if len(result) > 1 else prob


class U2Net(_RSUNet):
    """net = U2Net(weights, device); net(x) -> fp32 [T,S,S] on the device, sigmoid(d0) of every frame.
    weights: a U2NetWeights, or whatever load_u2net_weights accepts."""
    name = "U2Net"
    input_size = SIZE
    mean, std = MEAN, STD
    floats_per_frame_pixel = FLOATS_PER_FRAME_PIXEL

    def __init__(self, weights, device="cuda"):
        if not isinstance(weights, U2NetWeights):
            weights = load_u2net_weights(weights)
        super().__init__(VARIANTS[weights.variant], weights.layers, device)
        self.variant = weights.variant
        self.sides = tuple((wp.to(self.device), b.to(self.device)) for wp, b in weights.sides)
        self.outconv = weights.outconv

    def prepare(self, small):
        """the network's input of resized frames uint8 [T,S,S',3]: `rembg`'s normalisation with the ImageNet constants"""
        return ops.matte_prepare(small)

    def __call__(self, x, return_logits: bool = False, taps: bool = False, stage_events=None):
        """x: fp32 NHWC [T,S,S',4] on the device, the normalised frames with a zero fourth channel (ops.matte_prepare).  Returns
        the probabilities fp32 [T,S,S']; with return_logits (prob, d0); with taps also the dict of hx1..hx6 and hx5d..hx1d (NHWC).
        stage_events: a list that receives (stage, start, end) device events (tools/matting_time.py)."""
        self._check_input(x)
        t = self._trunk(x, stage_events)
        sources = [t["hx1d"], t["hx2d"], t["hx3d"], t["hx4d"], t["hx5d"], t["hx6"]]
        sides = [ops.conv3x3_ex(s, wp, b, relu=False) for s, (wp, b) in zip(sources, self.sides)]
        prob, logit = ops.matte_fuse(sides, self.outconv[:6], self.outconv[6], sides[0].shape[1:3], want_logits=return_logits)
        return self._result(prob, logit, return_logits, {name: t[name] for name in TAPS} if taps else None)


class ISNet(_RSUNet):
    """net = ISNet(weights, device, mean=, std=); net(x) -> fp32 [T,S,S'] on the device, sigmoid(d1) of every frame.
    weights: an ISNetWeights, or whatever load_isnet_weights accepts.  mean, std: the constants of the normalisation in front of
    the network (the defaults are those of `rembg`'s DIS session, as read from the package)."""
    name = "ISNet"
    variant = "isnet"
    input_size = ISNET_SIZE
    floats_per_frame_pixel = ISNET_FLOATS_PER_FRAME_PIXEL

    def __init__(self, weights, device="cuda", mean=ISNET_MEAN, std=ISNET_STD):
        if not isinstance(weights, ISNetWeights):
            weights = load_isnet_weights(weights)
        super().__init__(ISNET_STAGES, weights.layers, device)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or not all(math.isfinite(v) for v in self.mean) or not all(math.isfinite(v) and v > 0 for v in self.std):
            raise M324Error(f"ISNet: mean and std must be three finite numbers each, every std above 0, got {mean} and {std}")
        self.conv_in = tuple(t.to(self.device) for t in weights.conv_in)
        self.side1 = tuple(t.to(self.device) for t in weights.sides[0])

    def prepare(self, small):
        """the network's input of resized frames uint8 [T,S,S',3]: `rembg`'s normalisation with this network's constants"""
        return ops.matte_prepare(small, mean=self.mean, std=self.std)

    def __call__(self, x, return_logits: bool = False, taps: bool = False, stage_events=None):
        """x: fp32 NHWC [T,S,S',4] on the device, the normalised frames with a zero fourth channel (self.prepare).  Returns the
        probabilities fp32 [T,S,S'] = sigmoid(d1), d1 = side1(hx1d) resized to the input's size; with return_logits (prob, d1); with
        taps also the dict of hxin (the stem's output), hx1..hx6 and hx5d..hx1d (NHWC, from half the input's size down).
        stage_events: as U2Net; the stem is reported as "conv_in"."""
        self._check_input(x)
        if stage_events is not None:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
        hxin = ops.conv3x3_s2(x, *self.conv_in, relu=False)
        if stage_events is not None:
            end.record()
            stage_events.append(("conv_in", start, end))
        t = self._trunk(hxin, stage_events)
        side = ops.conv3x3_ex(t["hx1d"], *self.side1, relu=False)
        prob, logit = ops.matte_side(side, x.shape[1:3], want_logits=return_logits)
        return self._result(prob, logit, return_logits, dict({name: t[name] for name in TAPS}, hxin=hxin) if taps else None)


class Matte(NamedTuple):
    alpha: torch.Tensor       # uint8 [T,H,W], device: the matte at the video's size, what framing.frame_video takes as alpha
    mask320: torch.Tensor     # uint8 [T,size,size], device: the quantised network output before the resize back


def frames_per_chunk(T: int, size: int, max_scratch_bytes: int, floats_per_frame_pixel: int = FLOATS_PER_FRAME_PIXEL) -> int:
    """frames whose activations stay under max_scratch_bytes, or an M324Error when one frame does not fit.
    floats_per_frame_pixel: the network's live-activation estimate (net.floats_per_frame_pixel; U2-Net's by default)"""
    per_frame = 4 * int(floats_per_frame_pixel) * int(size) * int(size)
    if per_frame > int(max_scratch_bytes):
        raise M324Error(f"matte_video: one {size} x {size} frame needs {per_frame} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
    return max(1, min(int(T), int(max_scratch_bytes) // per_frame))


def composite_table() -> np.ndarray:
    """uint8 [256, 256]: table[alpha, value] = what Image.composite(img, empty, mask) leaves of a colour byte (Pillow's paste
    through an 8-bit mask onto zeros): t = value * alpha + 128, (t + (t >> 8)) >> 8"""
    t = np.arange(256, dtype=np.int64)[None, :] * np.arange(256, dtype=np.int64)[:, None] + 128
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def cutout_table() -> np.ndarray:
    """uint8 [256, 256]: the composite followed by the reference's soft masking, as one table of (mask byte, colour byte):
    rgb' = composite[a, v], alpha' = composite[a, 255] (the RGBA cutout), result = uint8(rgb' * (alpha' / 255.0))"""
    comp, soft = composite_table(), framing.soft_table()
    return soft[comp[:, 255][:, None], comp]


def mask_levels() -> np.ndarray:
    """fp32 [256]: the reference's `mask` of a mask byte a: float32(composite[a, 255] / 255.0), the division in float64"""
    return (composite_table()[:, 255].astype(np.float64) / 255.0).astype(np.float32)


def _device_video(video, device, who: str) -> torch.Tensor:
    if device is None:
        if not (isinstance(video, torch.Tensor) and video.is_cuda):
            raise M324Error(f"{who}: a host video needs device= (the matting runs on the GPU; there is no host path)")
        device = video.device
    v = video if isinstance(video, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(video))
    if v.dtype != torch.uint8 or v.dim() != 4 or v.shape[3] != 3 or 0 in v.shape:
        raise M324Error(f"{who}: expected uint8 frames [T,H,W,3], got {v.dtype} {tuple(v.shape)}")
    return v.to(device).contiguous()


def _resize(src, channels: int, w: int, h: int, new_w: int, new_h: int, out=None):
    """Pillow's two-pass 8-bit Lanczos of whole images, in the order framing.pass_order gives.  A pass between equal lengths,
    which Pillow skips, runs here as it does in framing.frame_video: its table is the identity (one coefficient of 1.0 per
    output), so the bytes are the same."""
    order = framing.pass_order(w, h, new_h)
    tabs = {"x": framing.resample_tables(w, new_w), "y": framing.resample_tables(h, new_h)}
    tabs = {axis: tuple(torch.from_numpy(t).to(src.device) for t in tab) for axis, tab in tabs.items()}
    mid = ops.frame_resample(src, *tabs[order[0]], order[0], channels=channels)
    return ops.frame_resample(mid, *tabs[order[1]], order[1], channels=channels, out=out)


def matte_video(video, net, *, size: Optional[int] = None, max_scratch_bytes: int = DEFAULT_MAX_SCRATCH_BYTES, device=None, stage_events=None) -> Matte:
    """video: uint8 [T,H,W,3], a device tensor (used where it is) or a host array with device=.  net: a U2Net or an ISNet; size: the
    side of the network's input, None for the network's own (320, 1024).  Steps 1 to 5 of the module's first paragraph with the
    network's constants, `frames_per_chunk` frames at a time; the result does not depend on the chunking.  Nothing synchronises.
    stage_events: handed to the network (tools/matting_time.py)."""
    if not isinstance(net, (U2Net, ISNet)):
        raise M324Error("matte_video: net must be a U2Net or an ISNet")
    size = net.input_size if size is None else size
    if not 1 <= int(size) <= ops.MATTE_MAX_SIDE:
        raise M324Error(f"matte_video: size must be in 1..{ops.MATTE_MAX_SIDE}, got {size}")
    v = _device_video(video, device, "matte_video")
    if v.device != net.device:
        raise M324Error(f"matte_video: the video is on {v.device}, the network on {net.device}")
    T, H, W, _ = v.shape
    size = int(size)
    n = frames_per_chunk(T, size, max_scratch_bytes, net.floats_per_frame_pixel)
    alpha = torch.empty((T, H, W), dtype=torch.uint8, device=v.device)
    mask = torch.empty((T, size, size), dtype=torch.uint8, device=v.device)
    for t0 in range(0, T, n):
        t1 = min(T, t0 + n)
        small = _resize(v[t0:t1], 3, W, H, size, size)
        prob = net(net.prepare(small), stage_events=stage_events)
        ops.matte_quantise(prob, out=mask[t0:t1])
        _resize(mask[t0:t1], 1, size, size, W, H, out=alpha[t0:t1])
    return Matte(alpha, mask)


def cut_out(video: torch.Tensor, alpha: torch.Tensor):
    """Step 6 and the reference's mask: (masked_frames uint8 [T,H,W,3], masks float32 [T,H,W,1]) of device frames and their matte"""
    table = torch.from_numpy(cutout_table()).to(video.device)
    masked = ops.frame_mask(video, alpha, mode="soft", table=table, want_mask=False)[0]
    return masked, torch.from_numpy(mask_levels()).to(video.device)[alpha.long()].unsqueeze(-1)


def segment_foreground_with_u2net(frames, net=None, device=None):
    """The reference's function of that name: (masked_frames uint8 [T,H,W,3], masks float32 [T,H,W,1] in 0..1).  Device tensors
    when a network is given (a U2Net, as in the reference, or an ISNet, each at its own size and constants); without one the frames
    come back as they are with masks of ones, as in the reference."""
    if net is None:
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        if t.dim() != 4 or t.shape[3] != 3:
            raise M324Error(f"segment_foreground_with_u2net: expected frames [T,H,W,3], got {tuple(t.shape)}")
        return frames, torch.ones(tuple(t.shape[:3]) + (1,), dtype=torch.float32, device=t.device)
    v = _device_video(frames, device if device is not None else net.device, "segment_foreground_with_u2net")
    return cut_out(v, matte_video(v, net).alpha)


def main(argv=None):
    from .perceptual import load_frames
    parser = argparse.ArgumentParser(description="U2-Net or ISNet foreground matting of a clip on the GPU")
    parser.add_argument("--video", type=str, required=True, help="a directory of PNG / JPG frames or a .npy of uint8 [T,H,W,3]")
    parser.add_argument("--weights", type=str, required=True, help="the .pth state dict of U2NET, U2NETP or ISNetDIS; which one is read from its keys")
    parser.add_argument("--out", type=str, required=True, help="directory for masked_frames.npy, masks.npy and alpha.npy")
    parser.add_argument("--size", type=int, default=None, help="side of the network's input (default: the network's own, 320 or 1024)")
    parser.add_argument("--frame", type=int, default=None, help="also write the foreground-centred square clip of this side (framed.npy, framed_mask.npy)")
    parser.add_argument("--frame_mode", choices=("soft", "threshold"), default="soft",
                        help="masking of the framed clip: soft, or the threshold at 204 of utils/rmbg_for_black_bg.py (its masked_rgb and mask_512)")
    args = parser.parse_args(argv)
    state = _load_file(args.weights, "motion324_amd.matting")
    weights = load_isnet_weights(state) if is_isnet_state(state) else load_u2net_weights(state)
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.matting needs a HIP device (there is no CPU path)")
    net = ISNet(weights, "cuda") if isinstance(weights, ISNetWeights) else U2Net(weights, "cuda")
    size = net.input_size if args.size is None else args.size
    video = torch.from_numpy(load_frames(args.video)).to(net.device)
    matte = matte_video(video, net, size=size)
    masked, masks = cut_out(video, matte.alpha)
    os.makedirs(args.out, exist_ok=True)
    written = {"masked_frames.npy": masked, "masks.npy": masks, "alpha.npy": matte.alpha}
    if args.frame is not None:
        framed = framing.frame_video(video, matte.alpha, size=args.frame, mode=args.frame_mode)
        if framed is None:
            print("no frame has foreground: no framed clip written")
        else:
            written["framed.npy"], written["framed_mask.npy"] = framed.frames, framed.mask
    for name, t in written.items():
        np.save(os.path.join(args.out, name), t.cpu().numpy())
    print(f"{args.video}: {video.shape[0]} frames of {video.shape[2]} x {video.shape[1]}, {net.variant} at {size} -> " + ", ".join(sorted(written)))
    return {name: os.path.join(args.out, name) for name in written}


if __name__ == "__main__":
    main()
