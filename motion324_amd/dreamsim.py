"""DreamSim on the GPU: one minus the cosine of the concatenated, normalised class features of an ensemble of ViT towers.

The "DreamSim" line of the reference's evaluation (evaluation/calculate_lpips.py:34-87: transforms.Resize((224, 224)) on a float
tensor, then the `dreamsim` package's ensemble model per frame pair).  The published ensemble is three ViT-B/16 towers -- DINO
(timm layout, feature = class row), OpenAI CLIP (open_clip layout, QuickGELU) and open_clip's own CLIP (open_clip layout, GELU),
the latter two with feature = embedding -- plus LoRA adapters on attn.qkv, which merge_lora folds into the weights.  Everything on
the device is fp32: the resize is two m324_resample_f32 passes under the float64-built tables of resize_tables (F.interpolate's
bilinear, align_corners=False, antialias as asked), the Linears are m324_gemm on the fp32 MFMA (QuickGELU its epilogue), attention,
LayerNorm, patch rows and the token assembly are csrc/vit.hip.  The weights are the user's files; nothing is downloaded.

What cannot be checked here: the `dreamsim`, `open_clip`, `timm`, `peft` and `torchvision` packages are not available to the
tests, so parity with the published checkpoint rests on the description above.  Two points are arguments because they could not
be settled: whether the DINO feature is the class row after the final norm (feature="cls", the default) or before it
("cls_prenorm"), and the adapter's alpha (adapter_config.json has it).

    python -m motion324_amd.dreamsim --gt_paths A ... --result_paths B ... --dino FILE --clip FILE --open_clip FILE
                                     [--lora FILE --lora_alpha X] [--output_dir DIR]
"""
from __future__ import annotations

import argparse
import math
import os
import re
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .clipsim import (GEMM_K, MAX_HEAD, MAX_WIDTH, OPENAI_MEAN, OPENAI_STD, ClipBlock, ClipVisionWeights, _load_file, _pad_k, _round_up,
                      frames_form, load_clip_vision_weights)
from .lib import ACT_GELU, ACT_QUICK_GELU, M324Error
from .perceptual import ClipScore, clip_statistics, load_frames, subvideo_frames

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
DINO_LN_EPS = 1e-6                      # timm's VisionTransformer: partial(nn.LayerNorm, eps=1e-6)
CLIP_LN_EPS = 1e-5
DEFAULT_MAX_SCRATCH_BYTES = 2 << 30
RESIZE_SCRATCH_BYTES = 256 << 20        # the intermediate of the first resize pass, per chunk of frames
TAPS = ("embed", "block0", "last_block", "cls_row")
FEATURES = ("embedding", "cls", "cls_prenorm")
ACTS = {"gelu": ACT_GELU, "quick_gelu": ACT_QUICK_GELU}
DINO_HEADS_BY_WIDTH = {192: 3, 384: 6, 768: 12, 1024: 16}             # timm's ViT-Ti / S / B / L


# ------------------------------------------------------------------------------------------- resize tables
def resize_tables64(n_in: int, n_out: int, antialias: bool = True):
    """(weights float64 [n_out, ksize], first int64 [n_out]) of F.interpolate(mode="bilinear", align_corners=False, antialias=...)
    along one axis, in float64: scale = n_in / n_out; support = scale and inv = 1 / scale when antialias and scale >= 1, else 1;
    the centre of output i is c = scale (i + 0.5); its taps are j in [lo, hi), lo = max(0, int(c - support + 0.5)), hi =
    min(int(c + support + 0.5), n_in), with w_j = max(0, 1 - |(j - c + 0.5) inv|) divided by the row's sum.  Zeros behind a row's taps."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise M324Error(f"resize_tables: sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    wide = bool(antialias) and scale >= 1.0
    support = scale if wide else 1.0
    inv = 1.0 / scale if wide else 1.0
    rows, first = [], np.empty(n_out, np.int64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in)
        j = np.arange(lo, hi, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j - c + 0.5) * inv))
        rows.append(w / w.sum())
        first[i] = lo
    ksize = max(len(r) for r in rows)
    weights = np.zeros((n_out, ksize), np.float64)
    for i, r in enumerate(rows):
        weights[i, :len(r)] = r
    return weights, first


def resize_tables(n_in: int, n_out: int, antialias: bool = True):
    """The tables m324_resample_f32 takes: (weights fp32 [n_out, ksize], first int32 [n_out]), resize_tables64 rounded once"""
    w, first = resize_tables64(n_in, n_out, antialias)
    if w.shape[1] > ops.RESAMPLE_MAX_KSIZE:
        raise M324Error(f"resize_tables: {n_in} -> {n_out} needs {w.shape[1]} taps, m324_resample_f32 takes {ops.RESAMPLE_MAX_KSIZE}")
    return w.astype(np.float32), first.astype(np.int32)


def resize_matrix(n_in: int, n_out: int, antialias: bool = True, rounded: bool = False) -> np.ndarray:
    """the tables as a dense float64 [n_out, n_in] matrix (rounded: from the fp32 tables the kernel reads); host-only, for checks"""
    w, first = resize_tables(n_in, n_out, antialias) if rounded else resize_tables64(n_in, n_out, antialias)
    m = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
        n = min(w.shape[1], n_in - int(first[i]))
        m[i, first[i]:first[i] + n] = w[i, :n]
    return m


def pass_order(H: int, W: int, out_h: int, out_w: int, ky: int, kx: int):
    """("y", "x") or ("x", "y"): the cheaper order of the two passes, counted in multiply-adds -- y first costs out_h W ky +
    out_h out_w kx, x first H out_w kx + out_h out_w ky.  A tie goes to y first: the y pass reads whole source rows (16-byte
    loads, 12-byte pixel groups of a byte source), the x pass gathers, and gathering from the smaller intermediate is cheaper."""
    y_first = out_h * W * ky + out_h * out_w * kx
    x_first = H * out_w * kx + out_h * out_w * ky
    return ("y", "x") if y_first <= x_first else ("x", "y")


_TABLES = {}


def _device_tables(n_in: int, n_out: int, antialias: bool, device):
    key = (n_in, n_out, bool(antialias), str(device))
    if key not in _TABLES:
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = tuple(torch.from_numpy(t).to(device) for t in resize_tables(n_in, n_out, antialias))
    return _TABLES[key]


def resize(frames: torch.Tensor, size, antialias: bool = True) -> torch.Tensor:
    """fp32 planar [T,3,out_h,out_w] of uint8 [T,H,W,3] (each byte / 255: ToTensor) or fp32 [T,3,H,W] frames on the device:
    transforms.Resize((out_h, out_w)) on a float tensor.  Two m324_resample_f32 passes in pass_order's order, a bounded number of
    frames at a time; nothing synchronises."""
    T, H, W, _ = frames_form(frames, "resize")
    out_h, out_w = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if not frames.is_cuda:
        raise M324Error("resize: the frames must be on a HIP device (there is no CPU path)")
    if not 1 <= out_h <= ops.RESAMPLE_MAX_SIDE or not 1 <= out_w <= ops.RESAMPLE_MAX_SIDE:
        raise M324Error(f"resize: the output sides must be 1 to {ops.RESAMPLE_MAX_SIDE}, got {out_h} x {out_w}")
    tabs = {"y": _device_tables(H, out_h, antialias, frames.device), "x": _device_tables(W, out_w, antialias, frames.device)}
    order = pass_order(H, W, out_h, out_w, tabs["y"][0].shape[1], tabs["x"][0].shape[1])
    per_frame = 12 * (out_h * W if order[0] == "y" else H * out_w)
    n = max(1, min(T, RESIZE_SCRATCH_BYTES // per_frame))
    if n >= 16:
        n -= n % 16                     # chunks of a byte source stay 16-byte aligned
    src = frames.detach().contiguous()
    out = torch.empty((T, 3, out_h, out_w), dtype=torch.float32, device=frames.device)
    mid = None
    for t0 in range(0, T, n):
        t1 = min(T, t0 + n)
        mid = ops.resample_f32(src[t0:t1], *tabs[order[0]], order[0], out=mid if mid is not None and mid.shape[0] == t1 - t0 else None)
        ops.resample_f32(mid, *tabs[order[1]], order[1], out=out[t0:t1])
    return out


# ------------------------------------------------------------------------------------------- weights
class VitWeights(NamedTuple):
    """fp32 CPU tensors in the layouts the kernels take; every GEMM weight is [N, K padded to a multiple of 32 with zeros]"""
    width: int
    heads: int
    layers: int
    mlp: int
    patch: int
    image: int
    tokens: int
    embed: int             # 0: no projection
    patch_w: torch.Tensor  # [W, Kp]
    patch_b: Optional[torch.Tensor]     # [W] or None
    cls: torch.Tensor      # [W]
    pos: torch.Tensor      # [L, W]
    ln_pre: Optional[tuple]
    blocks: tuple          # of ClipBlock: (ln_1, in_proj, out_proj, ln_2, c_fc, c_proj)
    ln_post: tuple         # the final norm
    proj_t: Optional[torch.Tensor]      # [E, Wp] or None


def _from_clip(w: ClipVisionWeights) -> VitWeights:
    return VitWeights(w.width, w.heads, w.layers, w.mlp, w.patch, w.image, w.tokens, w.embed, w.patch_w, None, w.cls, w.pos, w.ln_pre,
                      w.blocks, w.ln_post, w.proj_t)


def _tensor(v) -> torch.Tensor:
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))


_DINO_ANCHOR = "patch_embed.proj.weight"


def _layout_of(state: dict) -> str:
    if any(k.endswith(_DINO_ANCHOR) for k in state):
        return "dino"
    if any(k.endswith("conv1.weight") for k in state):
        return "open_clip"
    raise M324Error("load_vit_weights: the state dict has neither 'conv1.weight' (open_clip layout) nor 'patch_embed.proj.weight' "
                    "(DINO / timm layout)")


def load_vit_weights(state_or_path, layout: Optional[str] = None, heads: Optional[int] = None) -> VitWeights:
    """A ViT tower's weights, checked and repacked once.  Two layouts, told apart by their keys (or `layout`): "open_clip"
    (conv1.weight, transformer.resblocks.*, ln_pre, ln_post, proj: load_clip_vision_weights does it) and "dino" (timm's
    VisionTransformer: cls_token [1,1,W], pos_embed [1,L,W], patch_embed.proj.{weight,bias}, blocks.{i}.norm1 / attn.qkv /
    attn.proj / norm2 / mlp.fc1 / mlp.fc2, norm, and optionally norm_pre.* and proj [W, E]).  attn.qkv's rows are q | k | v, each
    head-major: nn.MultiheadAttention's in-projection order.  Whatever prefix stands in front of patch_embed.proj.weight is
    stripped from every key.  The head count is not in a state dict: `heads`, or the named towers by width.  What the tower
    does not do is refused by the key or shape that shows it."""
    who = "load_vit_weights"
    state = _load_file(os.fspath(state_or_path)) if isinstance(state_or_path, (str, os.PathLike)) else state_or_path
    if not isinstance(state, dict):
        raise M324Error(f"{who}: expected a state dict or a path to one")
    layout = _layout_of(state) if layout is None else layout
    if layout == "open_clip":
        return _from_clip(load_clip_vision_weights(state, heads=heads))
    if layout != "dino":
        raise M324Error(f"{who}: layout must be 'open_clip' or 'dino', got {layout!r}")
    anchors = [k for k in state if k.endswith(_DINO_ANCHOR)]
    if len(anchors) != 1:
        raise M324Error(f"{who}: expected one key ending in {_DINO_ANCHOR!r}, found {sorted(anchors)}")
    prefix = anchors[0][:-len(_DINO_ANCHOR)]
    vis = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    for k in vis:
        if re.search(r"(^|\.)(ls1|ls2|gamma_1|gamma_2)(\.|$)", k):
            raise M324Error(f"{who}: key {k!r}: layer scale is not part of this tower")
        if k.startswith(("reg_token", "register_tokens", "dist_token")):
            raise M324Error(f"{who}: key {k!r}: register / distillation tokens are not part of this tower")

    def get(key, shape=None, dims=None):
        if key not in vis:
            raise M324Error(f"{who}: the state dict has no key {key!r}")
        t = _tensor(vis[key])
        if (shape is not None and tuple(t.shape) != tuple(shape)) or (dims is not None and t.dim() != dims):
            want = tuple(shape) if shape is not None else f"{dims} dimensions"
            raise M324Error(f"{who}: {key!r} has shape {tuple(t.shape)}, expected {want}")
        t = t.detach().to(torch.float32).cpu()
        if not torch.isfinite(t).all():
            raise M324Error(f"{who}: {key!r} holds values that are not finite")
        return t.contiguous()

    conv = get(_DINO_ANCHOR, dims=4)
    W, cin, p, p2 = conv.shape
    if cin != 3 or p != p2:
        raise M324Error(f"{who}: {_DINO_ANCHOR!r} has shape {tuple(conv.shape)}, expected [W, 3, patch, patch]")
    if W > MAX_WIDTH:
        raise M324Error(f"{who}: {_DINO_ANCHOR!r} {tuple(conv.shape)}: width {W}: W > {MAX_WIDTH} is not supported")
    if W % 4:
        raise M324Error(f"{who}: {_DINO_ANCHOR!r} {tuple(conv.shape)}: width {W} is no multiple of 4")
    pos = get("pos_embed", dims=3)
    L = pos.shape[1]
    g = math.isqrt(max(L - 1, 0))
    if pos.shape[0] != 1 or pos.shape[2] != W or L < 2 or g * g != L - 1:
        raise M324Error(f"{who}: 'pos_embed' has shape {tuple(pos.shape)}: expected [1, 1 + g * g, {W}], a class token and a square grid "
                        f"(a non-square grid is not supported)")
    if heads is None:
        if W not in DINO_HEADS_BY_WIDTH:
            raise M324Error(f"{who}: the head count is not part of a state dict and width {W} is none of the named towers "
                            f"{sorted(DINO_HEADS_BY_WIDTH)}; pass heads=")
        heads = DINO_HEADS_BY_WIDTH[W]
    heads = int(heads)
    if heads < 1 or W % heads:
        raise M324Error(f"{who}: width {W} is not divisible by heads={heads} (W % heads != 0)")
    D = W // heads
    if D % 8:
        raise M324Error(f"{who}: 'blocks.0.attn.qkv.weight': head width {D} = {W} / {heads}: D % 8 != 0 is not supported")
    if D > MAX_HEAD:
        raise M324Error(f"{who}: 'blocks.0.attn.qkv.weight': head width {D} = {W} / {heads}: D > {MAX_HEAD} is not supported")
    layers = 0
    while f"blocks.{layers}.norm1.weight" in vis:
        layers += 1
    if layers == 0:
        raise M324Error(f"{who}: the state dict has no key 'blocks.0.norm1.weight'")
    mlp = get("blocks.0.mlp.fc1.weight", dims=2).shape[0]
    if mlp % 4:
        raise M324Error(f"{who}: 'blocks.0.mlp.fc1.weight': an MLP width of {mlp} is no multiple of 4")

    def ln(name):
        return get(name + ".weight", (W,)), get(name + ".bias", (W,))

    def linear(name, n, k):
        return _pad_k(get(name + ".weight", (n, k))), get(name + ".bias", (n,))

    blocks = []
    for i in range(layers):
        b = f"blocks.{i}."
        blocks.append(ClipBlock(ln(b + "norm1"), linear(b + "attn.qkv", 3 * W, W), linear(b + "attn.proj", W, W), ln(b + "norm2"),
                                linear(b + "mlp.fc1", mlp, W), linear(b + "mlp.fc2", W, mlp)))
    ln_pre = ln("norm_pre") if "norm_pre.weight" in vis else None
    proj_t, embed = None, 0
    if "proj" in vis:
        proj = get("proj", dims=2)
        if proj.shape[0] != W or proj.shape[1] % 4:
            raise M324Error(f"{who}: 'proj' has shape {tuple(proj.shape)}, expected [{W}, E] with E a multiple of 4")
        proj_t, embed = _pad_k(proj.t()), proj.shape[1]
    return VitWeights(W, heads, layers, mlp, p, g * p, L, embed, _pad_k(conv.reshape(W, 3 * p * p)), get("patch_embed.proj.bias", (W,)),
                      get("cls_token", (1, 1, W)).reshape(W).contiguous(), pos.reshape(L, W).contiguous(), ln_pre, tuple(blocks),
                      ln("norm"), proj_t)


_LORA_KEY = re.compile(r"^(?P<module>.+)\.lora_(?P<which>[AB])(?:\.[^.]+)?\.weight$")


def merge_lora(state: dict, adapter_state: dict, alpha: float) -> dict:
    """A copy of `state` with the LoRA adapters of `adapter_state` (peft keys: <module>.lora_A[.<name>].weight [r, in] and
    <module>.lora_B[.<name>].weight [out, r]) merged into their Linear weights: W + (alpha / r) B A, in float64, r from the
    shapes.  A module is matched to the one key of `state` that ends with its path from `blocks.` on (peft's and the wrapper's
    prefixes differ) + `.weight`; an adapter key that matches no base weight, or more than one, is refused by name."""
    who = "merge_lora"
    pairs = {}
    for k, v in adapter_state.items():
        m = _LORA_KEY.match(k)
        if m is None:
            if "lora_" in k:
                raise M324Error(f"{who}: adapter key {k!r} is not <module>.lora_A / lora_B[.<name>].weight")
            continue
        pairs.setdefault(m["module"], {})[m["which"]] = (k, _tensor(v).detach().to(torch.float64).cpu())
    out = dict(state)
    for module, ab in sorted(pairs.items()):
        if set(ab) != {"A", "B"}:
            raise M324Error(f"{who}: adapter key {next(iter(ab.values()))[0]!r} has no lora_{'B' if 'A' in ab else 'A'} partner")
        (ka, A), (kb, B) = ab["A"], ab["B"]
        tail = module[module.index("blocks."):] if "blocks." in module else module
        tail = tail.replace(".base_layer", "")
        hits = [k for k in state if k == tail + ".weight" or k.endswith("." + tail + ".weight")]
        if len(hits) != 1:
            raise M324Error(f"{who}: adapter key {ka!r} matches {'no' if not hits else 'more than one'} base weight "
                            f"(looked for a key ending in {tail + '.weight'!r})")
        base = _tensor(state[hits[0]])
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1] or A.shape[0] < 1 or tuple(base.shape) != (B.shape[0], A.shape[1]):
            raise M324Error(f"{who}: adapter key {ka!r}: lora_A {tuple(A.shape)} and lora_B {tuple(B.shape)} do not fit the base weight "
                            f"{hits[0]!r} {tuple(base.shape)}")
        r = A.shape[0]
        merged = base.detach().to(torch.float64).cpu() + (float(alpha) / r) * (B @ A)
        if not torch.isfinite(merged).all():
            raise M324Error(f"{who}: adapter key {ka!r}: the merged weight is not finite")
        out[hits[0]] = merged.to(base.dtype if base.dtype.is_floating_point else torch.float32)
    return out


def synth_dino_state_dict(seed: int, width: int, layers: int, heads: int, mlp: int, patch: int, image: int, embed: int = 0,
                          norm_pre: bool = False) -> dict:
    """Seeded weights in the form of a timm VisionTransformer state dict (no prefix), of trained-like scale, for tests and timing,
    in the manner of clipsim.synth_clip_state_dict: Linear weights randn / sqrt(fan-in) (the q and k rows of attn.qkv twice that,
    so that the softmax is not flat), LayerNorm weights around 1, small biases.  The patch projection, its bias, the class token
    and the positions have size 0.1 and nothing normalises them before block 0: norm1 of block 0 sees a variance near 0.03, where
    an eps of 1e-5 in place of 1e-6 moves the result by 1e-4 relative -- far outside an fp32 band."""
    if width % heads or image % patch:
        raise M324Error(f"synth_dino_state_dict: width {width} / heads {heads} or image {image} / patch {patch} does not divide")
    g = torch.Generator().manual_seed(int(seed))

    def randn(*shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale

    L = (image // patch) ** 2 + 1
    sd = {"cls_token": randn(1, 1, width, scale=0.1), "pos_embed": randn(1, L, width, scale=0.1),
          "patch_embed.proj.weight": randn(width, 3, patch, patch, scale=0.1 / math.sqrt(3 * patch * patch)),
          "patch_embed.proj.bias": randn(width, scale=0.1)}
    if norm_pre:
        sd["norm_pre.weight"] = 1.0 + randn(width, scale=0.1)
        sd["norm_pre.bias"] = randn(width, scale=0.05)
    for i in range(layers):
        b = f"blocks.{i}."
        for n in ("norm1", "norm2"):
            sd[b + n + ".weight"] = 1.0 + randn(width, scale=0.1)
            sd[b + n + ".bias"] = randn(width, scale=0.05)
        w = randn(3 * width, width, scale=1.0 / math.sqrt(width))
        w[:2 * width] *= 2.0
        sd[b + "attn.qkv.weight"] = w
        sd[b + "attn.qkv.bias"] = randn(3 * width, scale=0.05)
        sd[b + "attn.proj.weight"] = randn(width, width, scale=1.0 / math.sqrt(width))
        sd[b + "attn.proj.bias"] = randn(width, scale=0.05)
        sd[b + "mlp.fc1.weight"] = randn(mlp, width, scale=1.0 / math.sqrt(width))
        sd[b + "mlp.fc1.bias"] = randn(mlp, scale=0.05)
        sd[b + "mlp.fc2.weight"] = randn(width, mlp, scale=1.0 / math.sqrt(mlp))
        sd[b + "mlp.fc2.bias"] = randn(width, scale=0.05)
    sd["norm.weight"] = 1.0 + randn(width, scale=0.1)
    sd["norm.bias"] = randn(width, scale=0.05)
    if embed:
        sd["proj"] = randn(width, embed, scale=1.0 / math.sqrt(width))
    return sd


# ------------------------------------------------------------------------------------------- the tower
class VitTower:
    """tower = VitTower(weights, device, act=, ln_eps=, mean=, std=, feature=); tower.features(img) -> fp32 [F, E] of fp32 planar
    images [F,3,S,S] that are already S = tower.image pixels a side and in [0, 1]: the tower normalises them itself, in its patch
    rows.  feature: "embedding" = the class row after the last LayerNorm times proj (open_clip's encode_image), "cls" = the
    class row after the final norm, "cls_prenorm" = the class row of the last block's output.  weights: a VitWeights, or whatever
    load_vit_weights accepts."""

    def __init__(self, weights, device="cuda", act: str = "gelu", ln_eps: float = CLIP_LN_EPS, mean=OPENAI_MEAN, std=OPENAI_STD,
                 feature: str = "embedding"):
        if act not in ACTS:
            raise M324Error(f"VitTower: act must be 'gelu' or 'quick_gelu', got {act!r}")
        if feature not in FEATURES:
            raise M324Error(f"VitTower: feature must be one of {FEATURES}, got {feature!r}")
        if not isinstance(weights, VitWeights):
            weights = load_vit_weights(weights)
        if feature == "embedding" and weights.proj_t is None:
            raise M324Error("VitTower: feature='embedding' needs a 'proj' in the weights")
        if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std) or not float(ln_eps) > 0.0:
            raise M324Error("VitTower: mean and std are three numbers each (std not zero) and ln_eps is positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise M324Error("VitTower: needs a HIP device (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        w = weights
        self.width, self.heads, self.layers, self.mlp, self.patch, self.image, self.tokens, self.embed = w[:8]
        self.head_dim = self.width // self.heads
        self.act, self.act_code, self.ln_eps, self.feature = act, ACTS[act], float(ln_eps), feature
        self.out_dim = self.embed if feature == "embedding" else self.width
        dev = self.device

        def to(t):
            return None if t is None else tuple(x.to(dev) for x in t) if isinstance(t, tuple) else t.to(dev)

        self.patch_w, self.patch_b, self.cls, self.pos, self.proj_t = to(w.patch_w), to(w.patch_b), to(w.cls), to(w.pos), to(w.proj_t)
        self.ln_pre, self.ln_post = to(w.ln_pre), to(w.ln_post)
        self.blocks = tuple(ClipBlock(*(to(part) for part in blk)) for blk in w.blocks)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.mean_std = torch.tensor(self.mean + self.std, dtype=torch.float32, device=dev)
        self.Kp, self.Wp, self.Mp = self.patch_w.shape[1], _round_up(self.width, GEMM_K), _round_up(self.mlp, GEMM_K)

    def bytes_per_image(self) -> int:
        """scratch of one image in a chunk: the patch rows and their projection, the stream, the normalised / attended rows,
        q|k|v and the MLP's hidden rows"""
        L, W = self.tokens, self.width
        return 4 * ((L - 1) * (self.Kp + W) + L * (W + self.Wp + 3 * W + self.Mp))

    def images_per_chunk(self, n_images: int, max_scratch_bytes: int) -> int:
        per = self.bytes_per_image()
        if per > int(max_scratch_bytes):
            raise M324Error(f"VitTower: one image needs {per} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
        return max(1, min(int(n_images), int(max_scratch_bytes) // per))

    def features(self, img, taps: bool = False, max_scratch_bytes: int = DEFAULT_MAX_SCRATCH_BYTES, stage_events=None):
        """img: fp32 planar [F,3,S,S], S = self.image, on the tower's device.  Returns fp32 [F, out_dim]; with taps also a dict of
        the stream [F, L, W] after the embedding or norm_pre ("embed"), after block 0 ("block0") and after the last block
        ("last_block"), and the class rows [F, W] the feature is made of ("cls_row").  The images pass the tower
        `images_per_chunk` at a time; the result does not depend on the chunking and nothing synchronises.  stage_events: a list
        that receives (label, start, end) device events."""
        if not isinstance(img, torch.Tensor) or not img.is_cuda or img.device != self.device:
            raise M324Error(f"VitTower: the images must be on {self.device} (there is no CPU path)")
        if img.dtype != torch.float32 or img.dim() != 4 or tuple(img.shape[1:]) != (3, self.image, self.image) or img.shape[0] < 1:
            raise M324Error(f"VitTower: expected fp32 [F,3,{self.image},{self.image}], got {img.dtype} {tuple(img.shape)}")
        T = img.shape[0]
        img = img.detach().contiguous()
        n = self.images_per_chunk(T, max_scratch_bytes)
        L, W, dev = self.tokens, self.width, self.device
        f32 = torch.float32
        # y and hid keep zeros in their K-padding columns: the kernels write the first W (mlp) columns only
        bufs = {"rows": torch.empty((n * (L - 1), self.Kp), dtype=f32, device=dev), "pe": torch.empty((n * (L - 1), W), dtype=f32, device=dev),
                "x": torch.empty((n * L, W), dtype=f32, device=dev), "y": torch.zeros((n * L, self.Wp), dtype=f32, device=dev),
                "qkv": torch.empty((n * L, 3 * W), dtype=f32, device=dev), "hid": torch.zeros((n * L, self.Mp), dtype=f32, device=dev),
                "pooled": torch.zeros((n, self.Wp), dtype=f32, device=dev)}
        out = torch.empty((T, self.out_dim), dtype=f32, device=dev)
        tap = {k: torch.empty((T, L, W) if k != "cls_row" else (T, W), dtype=f32, device=dev) for k in TAPS} if taps else None
        for t0 in range(0, T, n):
            t1 = min(T, t0 + n)
            self._chunk(img[t0:t1], bufs, out[t0:t1], {k: v[t0:t1] for k, v in tap.items()} if taps else None, stage_events)
        return (out, tap) if taps else out

    def _chunk(self, img, bufs, out, tap, stage_events):
        n, L, W, H, D = img.shape[0], self.tokens, self.width, self.heads, self.head_dim
        M, eps = n * L, self.ln_eps

        def staged(label, fn):
            if stage_events is None:
                return fn()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            r = fn()
            end.record()
            stage_events.append((label, start, end))
            return r

        x, y, qkv, hid = bufs["x"][:M], bufs["y"][:M], bufs["qkv"][:M], bufs["hid"][:M]
        rows, pe, pooled = bufs["rows"][:n * (L - 1)], bufs["pe"][:n * (L - 1)], bufs["pooled"][:n]
        yw, hw = y[:, :W], hid[:, :self.mlp]
        staged("patch_rows", lambda: ops.vit_patches_f32(img, self.patch, self.mean_std, self.Kp, out=rows))
        staged("gemm_patch", lambda: ops.gemm(rows, self.patch_w, pe, bias=self.patch_b))
        if self.ln_pre is not None:
            tokens = qkv.view(-1)[:M * W].view(M, W)      # q|k|v is free until block 0: the stream starts at norm_pre's output
            staged("tokens", lambda: ops.vit_tokens(pe, self.cls, self.pos, out=tokens))
            staged("layernorm", lambda: ops.layernorm_wide(tokens, *self.ln_pre, eps, out=x))
        else:
            staged("tokens", lambda: ops.vit_tokens(pe, self.cls, self.pos, out=x))
        if tap is not None:
            tap["embed"].copy_(x.view(n, L, W))
        for i, blk in enumerate(self.blocks):
            staged("layernorm", lambda: ops.layernorm_wide(x, *blk.ln_1, eps, out=yw))
            staged("gemm_qkv", lambda: ops.gemm(y, blk.in_proj[0], qkv, bias=blk.in_proj[1]))
            staged("attention", lambda: ops.attention_tok(qkv, n, L, H, D, D ** -0.5, out=yw))
            staged("gemm_proj", lambda: ops.gemm(y, blk.out_proj[0], x, bias=blk.out_proj[1], residual=x))
            staged("layernorm", lambda: ops.layernorm_wide(x, *blk.ln_2, eps, out=yw))
            staged("gemm_fc1", lambda: ops.gemm(y, blk.c_fc[0], hw, bias=blk.c_fc[1], act=self.act_code))
            staged("gemm_fc2", lambda: ops.gemm(hid, blk.c_proj[0], x, bias=blk.c_proj[1], residual=x))
            if tap is not None and i == 0:
                tap["block0"].copy_(x.view(n, L, W))
        if tap is not None:
            tap["last_block"].copy_(x.view(n, L, W))
        cls_rows = x.view(n, L, W)[:, 0]                  # the class rows: a [n, W] view with leading dimension L * W
        if self.feature == "cls_prenorm":
            out.copy_(cls_rows)
        elif self.feature == "cls":
            staged("layernorm", lambda: ops.layernorm_wide(cls_rows, *self.ln_post, eps, out=out))
        else:
            staged("layernorm", lambda: ops.layernorm_wide(cls_rows, *self.ln_post, eps, out=pooled[:, :W]))
            staged("gemm_head", lambda: ops.gemm(pooled, self.proj_t, out))
        if tap is not None:
            tap["cls_row"].copy_(out if self.feature != "embedding" else pooled[:, :W])


# ------------------------------------------------------------------------------------------- the metric
def normalize_embedding(e: torch.Tensor) -> torch.Tensor:
    """the dreamsim package's normalize_embedding in float64: e / |e| along the feature dimension, then minus its mean along it"""
    e = e.double()
    e = e / e.norm(dim=-1, keepdim=True)
    return e - e.mean(dim=-1, keepdim=True)


class DreamSim:
    """metric = DreamSim(towers); metric(a, b) -> fp64 [T] on the device: 1 - cos of the two clips' concatenated tower features
    per frame pair.  Both clips are resized ONCE, as one batch, to size x size (two m324_resample_f32 passes); every tower
    normalises that one image itself.  size=None takes towers of different image sizes (small test towers): one resize per size.  Per tower the feature goes through normalize_embedding in float64 (normalize_embeds), the
    towers' vectors are concatenated, and the cosine is taken in float64."""

    def __init__(self, towers, normalize_embeds: bool = True, size: int = 224, antialias: bool = True):
        towers = tuple(towers)
        if not towers or not all(isinstance(t, VitTower) for t in towers):
            raise M324Error("DreamSim: towers must be a non-empty sequence of VitTower")
        for t in towers:
            if (size is not None and t.image != int(size)) or t.device != towers[0].device:
                raise M324Error(f"DreamSim: every tower must take {size} x {size} images on one device, got {t.image} on {t.device}")
        self.towers, self.normalize_embeds, self.antialias = towers, bool(normalize_embeds), bool(antialias)
        self.size = None if size is None else int(size)

    def embed(self, frames, **kw) -> torch.Tensor:
        """fp64 [T, sum of the towers' feature widths] of uint8 [T,H,W,3] or fp32 [T,3,H,W] frames in [0, 1]"""
        frames_form(frames, "DreamSim")
        if not frames.is_cuda or frames.device != self.towers[0].device:
            raise M324Error(f"DreamSim: the frames must be on {self.towers[0].device} (there is no CPU path)")
        resized = {}                                    # one resize per image size: one in all when the towers agree
        parts = []
        for t in self.towers:
            if t.image not in resized:
                resized[t.image] = resize(frames, t.image, self.antialias)
            e = t.features(resized[t.image], **kw).double()
            parts.append(normalize_embedding(e) if self.normalize_embeds else e)
        return torch.cat(parts, dim=-1)

    def __call__(self, a, b, **kw) -> torch.Tensor:
        Ta = frames_form(a, "DreamSim")[0]
        frames_form(b, "DreamSim")
        if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
            raise M324Error(f"DreamSim: the two clips must have one shape and dtype, got {a.dtype} {tuple(a.shape)} and "
                            f"{b.dtype} {tuple(b.shape)}")
        e = self.embed(torch.cat([a, b], 0), **kw)
        return distance(e[:Ta], e[Ta:])


def distance(ea: torch.Tensor, eb: torch.Tensor) -> torch.Tensor:
    """row-wise 1 - cos in float64"""
    ea, eb = ea.double(), eb.double()
    return 1.0 - (ea * eb).sum(-1) / (ea.norm(dim=-1) * eb.norm(dim=-1))


def evaluate_clips_dreamsim(gt, result, metric, **kw) -> ClipScore:
    """Scores `result` against `gt` as the reference's process_single_video does with only_final=True: the DreamSim distance of
    every frame pair, the clip extended to whole 32-frame sub-videos by its reversed tail (the padding repeats values, not work),
    mean and standard deviation over the kept frames.  metric: a DreamSim or any callable (a, b, **kw) -> [T]."""
    for x in (gt, result):
        frames_form(x, "evaluate_clips_dreamsim")
    if tuple(gt.shape) != tuple(result.shape) or gt.dtype != result.dtype:
        raise M324Error(f"evaluate_clips_dreamsim: the clips must have equal shapes, got {tuple(gt.shape)} and {tuple(result.shape)}")
    subvideo_frames(gt.shape[0])                        # refuses T < 16 before any work
    return clip_statistics(metric(gt, result, **kw).double().cpu().numpy())


def build_ensemble(dino, clip, open_clip, device="cuda", lora=None, lora_alpha: Optional[float] = None, dino_feature: str = "cls",
                   antialias: bool = True) -> DreamSim:
    """The published ensemble from the user's three files (state dicts or paths): dino_vitb16 (DINO layout, ImageNet mean / std,
    eps 1e-6, feature `dino_feature`), clip_vitb16 (open_clip layout, QuickGELU) and open_clip_vitb16 (open_clip layout, GELU),
    the latter two with OpenAI's mean / std and feature "embedding".  lora: an adapter state dict or path holding the adapters of
    every tower it names; it is merged into the tower whose keys it matches (lora_alpha has no default)."""
    states = []
    for s in (dino, clip, open_clip):
        states.append(_load_file(os.fspath(s)) if isinstance(s, (str, os.PathLike)) else s)
    if lora is not None:
        if lora_alpha is None:
            raise M324Error("build_ensemble: lora needs lora_alpha (the adapter's adapter_config.json has it)")
        adapter = _load_file(os.fspath(lora)) if isinstance(lora, (str, os.PathLike)) else lora
        states[0] = merge_lora(states[0], adapter, lora_alpha)
    towers = (VitTower(load_vit_weights(states[0], "dino"), device, "gelu", DINO_LN_EPS, IMAGENET_MEAN, IMAGENET_STD, dino_feature),
              VitTower(load_vit_weights(states[1], "open_clip"), device, "quick_gelu", CLIP_LN_EPS, OPENAI_MEAN, OPENAI_STD, "embedding"),
              VitTower(load_vit_weights(states[2], "open_clip"), device, "gelu", CLIP_LN_EPS, OPENAI_MEAN, OPENAI_STD, "embedding"))
    return DreamSim(towers, normalize_embeds=True, size=towers[0].image, antialias=antialias)


def main(argv=None):
    parser = argparse.ArgumentParser(description="DreamSim (three ViT-B/16 towers) between ground-truth and result clips on the GPU")
    parser.add_argument("--gt_paths", type=str, required=True, nargs="+", help="frame directories or .npy clips")
    parser.add_argument("--result_paths", type=str, required=True, nargs="+")
    parser.add_argument("--dino", type=str, required=True, help="the DINO ViT-B/16 state dict (timm layout)")
    parser.add_argument("--clip", type=str, required=True, help="the OpenAI CLIP ViT-B/16 image tower (open_clip layout, QuickGELU)")
    parser.add_argument("--open_clip", type=str, required=True, help="open_clip's ViT-B/16 image tower (open_clip layout, GELU)")
    parser.add_argument("--lora", type=str, default=None, help="LoRA adapters on the DINO tower's attn.qkv (peft keys)")
    parser.add_argument("--lora_alpha", type=float, default=None, help="the adapter's alpha (adapter_config.json); no default")
    parser.add_argument("--dino_feature", type=str, default="cls", choices=("cls", "cls_prenorm"))
    parser.add_argument("--no_antialias", action="store_true", help="torchvision before 0.17 resized tensors without antialiasing")
    parser.add_argument("--output_dir", type=str, default=None)
    args = parser.parse_args(argv)
    if len(args.gt_paths) != len(args.result_paths):
        raise M324Error(f"{len(args.gt_paths)} gt paths but {len(args.result_paths)} result paths: pairs are matched by position")
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.dreamsim needs a HIP device (there is no CPU path)")
    metric = build_ensemble(args.dino, args.clip, args.open_clip, "cuda", args.lora, args.lora_alpha, args.dino_feature, not args.no_antialias)
    results = []
    for gt_path, result_path in zip(args.gt_paths, args.result_paths):
        missing = [p for p in (gt_path, result_path) if not os.path.exists(p)]
        if missing:
            print(f"Warning: {missing[0]} not found, skipping")
            continue
        gt, result = (torch.from_numpy(load_frames(p)).to("cuda") for p in (gt_path, result_path))
        score = evaluate_clips_dreamsim(gt, result, metric)
        results.append(score.value)
        line = f"{result_path}: DreamSim {score.value:.6f} (std {score.value_std:.6f}, {len(score.per_video)} sub-video(s))"
        if args.output_dir:
            base = os.path.basename(result_path.rstrip("/"))
            if os.path.isfile(result_path):
                base = os.path.splitext(base)[0]
            os.makedirs(args.output_dir, exist_ok=True)
            out_file = os.path.join(args.output_dir, base + ".dreamsim.txt")
            with open(out_file, "w") as f:
                f.write(f"GT Source: {gt_path}\nResult Source: {result_path}\nDreamSim: {score.value}\n" + "-" * 50 + "\n")
            line += f" -> {out_file}"
        print(line)
    print(f"Summary: processed {len(results)}/{len(args.gt_paths)} pairs" + (f"; Average DreamSim: {np.mean(results):.6f}" if results else ""))
    return results


if __name__ == "__main__":
    main()
