"""CLIP image similarity on the GPU: the cosine of open_clip ViT image features between two clips, frame by frame.

The "CLIP Loss" line of the reference's evaluation (evaluation/calculate_lpips.py:90-136: open_clip's ViT-bigG-14, `encode_image`,
F.normalize and cosine_similarity per frame pair).  The tower is open_clip's VisionTransformer without its options: a patch
convolution without bias, the class token and a learned positional embedding, ln_pre, pre-norm residual blocks of
nn.MultiheadAttention and a GELU MLP, ln_post on the class token and the projection.  Everything is fp32: the Linears are
m324_gemm on the fp32 MFMA, attention, LayerNorm, patch rows and the token assembly are csrc/vit.hip, the resize is the 8-bit
bicubic of m324_frame_resample under the tables of framing.resample_tables.  The weights are the user's (an open_clip state dict
or checkpoint file); nothing is downloaded.

    python -m motion324_amd.clipsim --gt_paths A ... --result_paths B ... --weights open_clip_pytorch_model.bin [--heads N] [--output_dir DIR]
"""
from __future__ import annotations

import argparse
import math
import os
import re
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import framing, ops
from .lib import ACT_GELU, M324Error
from .perceptual import ClipScore, clip_statistics, load_frames, subvideo_frames

OPENAI_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_STD = (0.26862954, 0.26130258, 0.27577711)
LN_EPS = 1e-5
HEADS_BY_WIDTH = {768: 12, 1024: 16, 1280: 16, 1408: 16, 1664: 16}       # open_clip's named towers: B, L, H, g, bigG
MAX_WIDTH = ops.LAYERNORM_WIDE_MAX_C
MAX_HEAD = ops.ATTN_TOK_MAX_D
FRAME_MAX_SIDE = 16384                  # M324_FRAME_MAX_SIDE
GEMM_K = 32                             # the fp32 GEMM contracts K in steps of 32: every K is padded with zero columns to it
DEFAULT_MAX_SCRATCH_BYTES = 2 << 30
TAPS = ("ln_pre", "block0", "last_block", "ln_post")
_PREFIXES = ("module.", "visual.")


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


class ClipBlock(NamedTuple):
    ln_1: tuple            # (weight [W], bias [W])
    in_proj: tuple         # (weight [3W, Wp], bias [3W])
    out_proj: tuple        # (weight [W, Wp], bias [W])
    ln_2: tuple
    c_fc: tuple            # (weight [M, Wp], bias [M])
    c_proj: tuple          # (weight [W, Mp], bias [W])


class ClipVisionWeights(NamedTuple):
    """fp32 CPU tensors in the layouts the kernels take; every GEMM weight is [N, K padded to a multiple of 32 with zeros]"""
    width: int
    heads: int
    layers: int
    mlp: int
    patch: int
    image: int
    tokens: int
    embed: int
    patch_w: torch.Tensor  # [W, Kp], Kp = round_up(3 patch^2, 32)
    cls: torch.Tensor      # [W]
    pos: torch.Tensor      # [L, W]
    ln_pre: tuple
    blocks: tuple          # of ClipBlock
    ln_post: tuple
    proj_t: torch.Tensor   # [E, Wp]: proj transposed once


def _load_file(path: str) -> dict:
    if not os.path.isfile(path):
        raise M324Error(f"load_clip_vision_weights: no such file {path!r}")
    if path.lower().endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError:
            raise M324Error(f"load_clip_vision_weights: {path!r} is a .safetensors file and the safetensors package is not installed; "
                            "convert it to a torch.save'd state dict") from None
        return load_file(path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    if not isinstance(state, dict):
        raise M324Error(f"load_clip_vision_weights: {path!r} holds a {type(state).__name__}, not a state dict")
    return state


def _strip(key: str) -> str:
    stripped = True
    while stripped:
        stripped = False
        for p in _PREFIXES:
            if key.startswith(p):
                key, stripped = key[len(p):], True
    return key


def _pad_k(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> contiguous [N, round_up(K, 32)], zeros behind K"""
    n, k = w.shape
    out = torch.zeros((n, _round_up(k, GEMM_K)), dtype=torch.float32)
    out[:, :k] = w
    return out


def load_clip_vision_weights(state_or_path, heads: Optional[int] = None) -> ClipVisionWeights:
    """The image tower of an open_clip checkpoint, checked and repacked once (fp32 CPU tensors; ClipVision moves them to its
    device).  state_or_path: a state dict, or a file torch.load(weights_only=True) reads (.safetensors where that package is
    installed); keys may carry `visual.` and / or `module.` in front, the text tower's keys are ignored.  Sizes come from the
    shapes; the head count is not in a state dict: `heads`, or open_clip's named towers by width (HEADS_BY_WIDTH).  What this
    tower does not do is refused by the key or shape that shows it."""
    who = "load_clip_vision_weights"
    state = _load_file(os.fspath(state_or_path)) if isinstance(state_or_path, (str, os.PathLike)) else state_or_path
    if not isinstance(state, dict):
        raise M324Error(f"{who}: expected a state dict or a path to one")
    vis = {}
    has_visual = any(_strip_module(k).startswith("visual.") for k in state)
    for k, v in state.items():
        if has_visual and not _strip_module(k).startswith("visual."):
            continue                                    # the text tower, logit_scale
        vis[_strip(k)] = v
    for k in vis:
        if re.search(r"(^|\.)ls_[12](\.|$)", k):
            raise M324Error(f"{who}: key {k!r}: layer scale (ls_1 / ls_2) is not part of this tower")
        if "attn_pool" in k:
            raise M324Error(f"{who}: key {k!r}: attentional pooling (attn_pool) is not part of this tower")

    def get(key, shape=None, dims=None):
        if key not in vis:
            raise M324Error(f"{who}: the state dict has no key {key!r}")
        t = vis[key]
        t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
        if (shape is not None and tuple(t.shape) != tuple(shape)) or (dims is not None and t.dim() != dims):
            want = tuple(shape) if shape is not None else f"{dims} dimensions"
            raise M324Error(f"{who}: {key!r} has shape {tuple(t.shape)}, expected {want}")
        t = t.detach().to(torch.float32).cpu()
        if not torch.isfinite(t).all():
            raise M324Error(f"{who}: {key!r} holds values that are not finite")
        return t.contiguous()

    conv = get("conv1.weight", dims=4)
    W, cin, p, p2 = conv.shape
    if cin != 3 or p != p2:
        raise M324Error(f"{who}: 'conv1.weight' has shape {tuple(conv.shape)}, expected [W, 3, patch, patch]")
    if "conv1.bias" in vis:
        raise M324Error(f"{who}: key 'conv1.bias': the patch convolution of this tower has no bias")
    if W > MAX_WIDTH:
        raise M324Error(f"{who}: 'conv1.weight' {tuple(conv.shape)}: width {W}: W > {MAX_WIDTH} is not supported")
    if W % 4:
        raise M324Error(f"{who}: 'conv1.weight' {tuple(conv.shape)}: width {W} is no multiple of 4")
    pos = get("positional_embedding", dims=2)
    L = pos.shape[0]
    g = math.isqrt(max(L - 1, 0))
    if pos.shape[1] != W or L < 2 or g * g != L - 1:
        raise M324Error(f"{who}: 'positional_embedding' has shape {tuple(pos.shape)}: expected [1 + g * g, {W}], a class token and a "
                        f"square grid (a non-square grid is not supported)")
    if heads is None:
        if W not in HEADS_BY_WIDTH:
            raise M324Error(f"{who}: the head count is not part of a state dict and width {W} is none of open_clip's named towers "
                            f"{sorted(HEADS_BY_WIDTH)}; pass heads=")
        heads = HEADS_BY_WIDTH[W]
    heads = int(heads)
    if heads < 1 or W % heads:
        raise M324Error(f"{who}: width {W} is not divisible by heads={heads} (W % heads != 0)")
    D = W // heads
    if D % 8:
        raise M324Error(f"{who}: head width {D} = {W} / {heads}: D % 8 != 0 is not supported")
    if D > MAX_HEAD:
        raise M324Error(f"{who}: head width {D} = {W} / {heads}: D > {MAX_HEAD} is not supported")
    layers = 0
    while f"transformer.resblocks.{layers}.ln_1.weight" in vis:
        layers += 1
    if layers == 0:
        raise M324Error(f"{who}: the state dict has no key 'transformer.resblocks.0.ln_1.weight'")
    mlp = get("transformer.resblocks.0.mlp.c_fc.weight", dims=2).shape[0]
    if mlp % 4:
        raise M324Error(f"{who}: 'transformer.resblocks.0.mlp.c_fc.weight': an MLP width of {mlp} is no multiple of 4")

    def ln(name):
        return get(name + ".weight", (W,)), get(name + ".bias", (W,))

    blocks = []
    for i in range(layers):
        b = f"transformer.resblocks.{i}."
        blocks.append(ClipBlock(
            ln(b + "ln_1"),
            (_pad_k(get(b + "attn.in_proj_weight", (3 * W, W))), get(b + "attn.in_proj_bias", (3 * W,))),
            (_pad_k(get(b + "attn.out_proj.weight", (W, W))), get(b + "attn.out_proj.bias", (W,))),
            ln(b + "ln_2"),
            (_pad_k(get(b + "mlp.c_fc.weight", (mlp, W))), get(b + "mlp.c_fc.bias", (mlp,))),
            (_pad_k(get(b + "mlp.c_proj.weight", (W, mlp))), get(b + "mlp.c_proj.bias", (W,)))))
    proj = get("proj", dims=2)
    if proj.shape[0] != W or proj.shape[1] % 4:
        raise M324Error(f"{who}: 'proj' has shape {tuple(proj.shape)}, expected [{W}, E] with E a multiple of 4")
    return ClipVisionWeights(W, heads, layers, mlp, p, g * p, L, proj.shape[1], _pad_k(conv.reshape(W, 3 * p * p)),
                             get("class_embedding", (W,)), pos, ln("ln_pre"), tuple(blocks), ln("ln_post"), _pad_k(proj.t()))


def _strip_module(key: str) -> str:
    while key.startswith("module."):
        key = key[len("module."):]
    return key


def synth_clip_state_dict(seed: int, width: int, layers: int, heads: int, mlp: int, patch: int, image: int, embed: int) -> dict:
    """Seeded weights in the form of an open_clip VisionTransformer state dict (no prefix), of trained-like scale, for tests and
    timing: Linear weights randn / sqrt(fan-in) (the in-projection's q and k rows twice that, so that the softmax is not flat),
    LayerNorm weights around 1, small biases, a patch projection, class token and positions of size 0.1 (ln_pre brings the stream to size one).  `heads` only checks
    the width: a state dict does not hold it."""
    if width % heads or image % patch:
        raise M324Error(f"synth_clip_state_dict: width {width} / heads {heads} or image {image} / patch {patch} does not divide")
    g = torch.Generator().manual_seed(int(seed))

    def randn(*shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale

    L = (image // patch) ** 2 + 1
    sd = {"conv1.weight": randn(width, 3, patch, patch, scale=0.1 / math.sqrt(3 * patch * patch)),
          "class_embedding": randn(width, scale=0.1), "positional_embedding": randn(L, width, scale=0.1),
          "ln_pre.weight": 1.0 + randn(width, scale=0.1), "ln_pre.bias": randn(width, scale=0.05)}
    for i in range(layers):
        b = f"transformer.resblocks.{i}."
        for n in ("ln_1", "ln_2"):
            sd[b + n + ".weight"] = 1.0 + randn(width, scale=0.1)
            sd[b + n + ".bias"] = randn(width, scale=0.05)
        w = randn(3 * width, width, scale=1.0 / math.sqrt(width))
        w[:2 * width] *= 2.0
        sd[b + "attn.in_proj_weight"] = w
        sd[b + "attn.in_proj_bias"] = randn(3 * width, scale=0.05)
        sd[b + "attn.out_proj.weight"] = randn(width, width, scale=1.0 / math.sqrt(width))
        sd[b + "attn.out_proj.bias"] = randn(width, scale=0.05)
        sd[b + "mlp.c_fc.weight"] = randn(mlp, width, scale=1.0 / math.sqrt(width))
        sd[b + "mlp.c_fc.bias"] = randn(mlp, scale=0.05)
        sd[b + "mlp.c_proj.weight"] = randn(width, mlp, scale=1.0 / math.sqrt(mlp))
        sd[b + "mlp.c_proj.bias"] = randn(width, scale=0.05)
    sd["ln_post.weight"] = 1.0 + randn(width, scale=0.1)
    sd["ln_post.bias"] = randn(width, scale=0.05)
    sd["proj"] = randn(width, embed, scale=1.0 / math.sqrt(width))
    return sd


def frames_form(frames, name: str = "preprocess"):
    """(T, H, W, is_bytes) of a clip in one of the two accepted forms, uint8 [T,H,W,3] or fp32 [T,3,H,W]; host-only"""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise M324Error(f"{name}: expected a uint8 [T,H,W,3] or fp32 [T,3,H,W] tensor")
    if frames.dtype == torch.uint8 and frames.shape[3] == 3:
        T, H, W, is_bytes = frames.shape[0], frames.shape[1], frames.shape[2], True
    elif frames.dtype == torch.float32 and frames.shape[1] == 3:
        T, H, W, is_bytes = frames.shape[0], frames.shape[2], frames.shape[3], False
    else:
        raise M324Error(f"{name}: expected uint8 [T,H,W,3] or fp32 [T,3,H,W], got {frames.dtype} {tuple(frames.shape)}")
    if T < 1 or not 1 <= H <= FRAME_MAX_SIDE or not 1 <= W <= FRAME_MAX_SIDE:
        raise M324Error(f"{name}: at least one frame and sides of 1 to {FRAME_MAX_SIDE} pixels, got {tuple(frames.shape)}")
    return T, H, W, is_bytes


def resize_geometry(H: int, W: int, size: int):
    """(new_h, new_w, top, left) of torchvision's Resize(size) and CenterCrop(size): the shorter side becomes `size`, the longer
    int(size * longer / shorter); the crop starts at int(round((side - size) / 2.0)) (Python's round: half to even)"""
    H, W, size = int(H), int(W), int(size)
    if W <= H:
        new_w, new_h = size, int(size * H / W)
    else:
        new_h, new_w = size, int(size * W / H)
    return new_h, new_w, int(round((new_h - size) / 2.0)), int(round((new_w - size) / 2.0))


_TABLES = {}


def _tables(n_in: int, n_out: int, first: int, count: int, device):
    """the bicubic tables of a pass from n_in to n_out samples, cut to the outputs [first, first + count), on the device"""
    key = (n_in, n_out, first, count, str(device))
    if key not in _TABLES:
        if len(_TABLES) > 64:
            _TABLES.clear()
        coef, bounds = framing.resample_tables(n_in, n_out, filter="bicubic")
        _TABLES[key] = tuple(torch.from_numpy(np.ascontiguousarray(t[first:first + count])).to(device) for t in (coef, bounds))
    return _TABLES[key]


def to_bytes(frames: torch.Tensor) -> torch.Tensor:
    """fp32 [T,3,H,W] in [0, 1] -> uint8 [T,H,W,3] as ToPILImage does: trunc(clamp(x * 255, 0, 255)), the product in fp32"""
    return (frames.detach() * 255.0).clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def preprocess(frames: torch.Tensor, size: int, mean=OPENAI_MEAN, std=OPENAI_STD) -> torch.Tensor:
    """The byte half of the reference's chain -- ToPILImage, then open_clip's eval transform up to the crop -- on the device:
    uint8 [T,size,size,3].  frames uint8 [T,H,W,3] as they are, or fp32 [T,3,H,W] in [0, 1] (to_bytes).  The shorter side is
    resized to `size` with the reference library's 8-bit bicubic (two m324_frame_resample passes in framing.pass_order's
    order) and the centre size x size crop is cut from the tables: only the kept outputs are computed.  ToTensor and
    Normalize(mean, std) are fp32 and belong to the patch rows (ops.vit_patches); mean and std are only checked here."""
    T, H, W, is_bytes = frames_form(frames)
    size = int(size)
    if not frames.is_cuda:
        raise M324Error("preprocess: the frames must be on a HIP device (there is no CPU path)")
    if not 1 <= size <= FRAME_MAX_SIDE or len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
        raise M324Error(f"preprocess: size must be 1 to {FRAME_MAX_SIDE} and mean, std three numbers (std not zero)")
    src = frames.detach().contiguous() if is_bytes else to_bytes(frames)
    new_h, new_w, top, left = resize_geometry(H, W, size)
    if max(new_h, new_w) > FRAME_MAX_SIDE:
        raise M324Error(f"preprocess: {H} x {W} resized to {new_h} x {new_w} passes {FRAME_MAX_SIDE} pixels")
    tabs = {"x": _tables(W, new_w, left, size, src.device), "y": _tables(H, new_h, top, size, src.device)}
    order = framing.pass_order(W, H, new_h)
    mid = ops.frame_resample(src, *tabs[order[0]], order[0])
    return ops.frame_resample(mid, *tabs[order[1]], order[1])


class ClipVision:
    """tower = ClipVision(weights, device); tower.features(frames) -> fp32 [T, E], open_clip's encode_image before any
    normalisation.  weights: a ClipVisionWeights, or whatever load_clip_vision_weights accepts."""

    def __init__(self, weights, device="cuda", act: str = "gelu", mean=OPENAI_MEAN, std=OPENAI_STD):
        if act == "quick_gelu":
            raise M324Error("ClipVision: act='quick_gelu' (the OpenAI-pretrained towers) is not supported: the GEMM has no epilogue "
                            "for x * sigmoid(1.702 x)")
        if act != "gelu":
            raise M324Error(f"ClipVision: act must be 'gelu', got {act!r}")
        if not isinstance(weights, ClipVisionWeights):
            weights = load_clip_vision_weights(weights)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise M324Error("ClipVision: needs a HIP device (there is no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        w = weights
        self.width, self.heads, self.layers, self.mlp, self.patch, self.image, self.tokens, self.embed = w[:8]
        self.head_dim = self.width // self.heads
        dev = self.device

        def to(t):
            return tuple(x.to(dev) for x in t) if isinstance(t, tuple) else t.to(dev)

        self.patch_w, self.cls, self.pos, self.proj_t = to(w.patch_w), to(w.cls), to(w.pos), to(w.proj_t)
        self.ln_pre, self.ln_post = to(w.ln_pre), to(w.ln_post)
        self.blocks = tuple(ClipBlock(*(to(part) for part in blk)) for blk in w.blocks)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.mean_std = torch.tensor(self.mean + self.std, dtype=torch.float32, device=dev)
        self.Kp, self.Wp, self.Mp = self.patch_w.shape[1], _round_up(self.width, GEMM_K), _round_up(self.mlp, GEMM_K)

    def bytes_per_image(self) -> int:
        """scratch of one image in a chunk: the preprocessed bytes, the patch rows and their projection, the stream, the
        normalised / attended rows, q|k|v and the MLP's hidden rows (the resize intermediate of the source size is not counted)"""
        L, W = self.tokens, self.width
        return 3 * self.image ** 2 + 4 * ((L - 1) * (self.Kp + W) + L * (W + self.Wp + 3 * W + self.Mp))

    def images_per_chunk(self, n_images: int, max_scratch_bytes: int) -> int:
        per = self.bytes_per_image()
        if per > int(max_scratch_bytes):
            raise M324Error(f"ClipVision: one image needs {per} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
        return max(1, min(int(n_images), int(max_scratch_bytes) // per))

    def features(self, frames, *, taps: bool = False, max_scratch_bytes: int = DEFAULT_MAX_SCRATCH_BYTES, stage_events=None):
        """frames: uint8 [T,H,W,3] or fp32 [T,3,H,W] in [0, 1] on the tower's device.  Returns fp32 [T, E]; with taps also a dict
        of the stream [T, L, W] after ln_pre ("ln_pre"), after block 0 ("block0") and after the last block ("last_block") and
        the ln_post class rows [T, W] ("ln_post").  The images pass the tower `images_per_chunk` at a time; the result does not
        depend on the chunking and nothing synchronises.  stage_events: a list that receives (label, start, end) device events."""
        T = frames_form(frames, "ClipVision")[0]
        if not frames.is_cuda or frames.device != self.device:
            raise M324Error(f"ClipVision: the frames must be on {self.device} (there is no CPU path)")
        n = self.images_per_chunk(T, max_scratch_bytes)
        L, W, dev = self.tokens, self.width, self.device
        f32 = torch.float32
        # y and hid keep zeros in their K-padding columns: the kernels write the first W (mlp) columns only
        bufs = {"rows": torch.empty((n * (L - 1), self.Kp), dtype=f32, device=dev), "pe": torch.empty((n * (L - 1), W), dtype=f32, device=dev),
                "x": torch.empty((n * L, W), dtype=f32, device=dev), "y": torch.zeros((n * L, self.Wp), dtype=f32, device=dev),
                "qkv": torch.empty((n * L, 3 * W), dtype=f32, device=dev), "hid": torch.zeros((n * L, self.Mp), dtype=f32, device=dev),
                "pooled": torch.zeros((n, self.Wp), dtype=f32, device=dev)}
        out = torch.empty((T, self.embed), dtype=f32, device=dev)
        tap = {k: torch.empty((T, L, W) if k != "ln_post" else (T, W), dtype=f32, device=dev) for k in TAPS} if taps else None
        for t0 in range(0, T, n):
            t1 = min(T, t0 + n)
            self._chunk(frames[t0:t1], bufs, out[t0:t1], {k: v[t0:t1] for k, v in tap.items()} if taps else None, stage_events)
        return (out, tap) if taps else out

    def _chunk(self, frames, bufs, out, tap, stage_events):
        n, L, W, H, D = frames.shape[0], self.tokens, self.width, self.heads, self.head_dim
        M = n * L

        def begin():
            if stage_events is None:
                return None
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        def mark(label, start):
            if stage_events is not None:
                end = torch.cuda.Event(enable_timing=True)
                end.record()
                stage_events.append((label, start, end))

        def staged(label, fn):
            start = begin()
            r = fn()
            mark(label, start)
            return r

        x, y, qkv, hid = bufs["x"][:M], bufs["y"][:M], bufs["qkv"][:M], bufs["hid"][:M]
        rows, pe, pooled = bufs["rows"][:n * (L - 1)], bufs["pe"][:n * (L - 1)], bufs["pooled"][:n]
        yw, hw = y[:, :W], hid[:, :self.mlp]
        img = staged("preprocess", lambda: preprocess(frames, self.image, self.mean, self.std))
        start = begin()
        ops.vit_patches(img, self.patch, self.mean_std, self.Kp, out=rows)
        ops.gemm(rows, self.patch_w, pe)
        tokens = qkv.view(-1)[:M * W].view(M, W)          # q|k|v is free until block 0: the stream starts at ln_pre's output
        ops.vit_tokens(pe, self.cls, self.pos, out=tokens)
        mark("patch_embed", start)
        staged("layernorm", lambda: ops.layernorm_wide(tokens, *self.ln_pre, LN_EPS, out=x))
        if tap is not None:
            tap["ln_pre"].copy_(x.view(n, L, W))
        for i, blk in enumerate(self.blocks):
            staged("layernorm", lambda: ops.layernorm_wide(x, *blk.ln_1, LN_EPS, out=yw))
            staged("gemm_in_proj", lambda: ops.gemm(y, blk.in_proj[0], qkv, bias=blk.in_proj[1]))
            staged("attention", lambda: ops.attention_tok(qkv, n, L, H, D, D ** -0.5, out=yw))
            staged("gemm_out_proj", lambda: ops.gemm(y, blk.out_proj[0], x, bias=blk.out_proj[1], residual=x))
            staged("layernorm", lambda: ops.layernorm_wide(x, *blk.ln_2, LN_EPS, out=yw))
            staged("gemm_c_fc", lambda: ops.gemm(y, blk.c_fc[0], hw, bias=blk.c_fc[1], act=ACT_GELU))
            staged("gemm_c_proj", lambda: ops.gemm(hid, blk.c_proj[0], x, bias=blk.c_proj[1], residual=x))
            if tap is not None and i == 0:
                tap["block0"].copy_(x.view(n, L, W))
        if tap is not None:
            tap["last_block"].copy_(x.view(n, L, W))
        start = begin()
        ops.layernorm_wide(x.view(n, L, W)[:, 0], *self.ln_post, LN_EPS, out=pooled[:, :W])       # the class rows: ldx = L * W
        ops.gemm(pooled, self.proj_t, out)
        mark("head", start)
        if tap is not None:
            tap["ln_post"].copy_(pooled[:, :W])


class ClipSimilarity:
    """metric = ClipSimilarity(model); metric(a, b) -> fp64 [T] on the device: the cosine of the two clips' image features per
    frame pair.  Both clips pass the tower as one batch; the features are normalised and multiplied in float64 (the reference's
    F.normalize followed by cosine_similarity is a cosine)."""

    def __init__(self, model: ClipVision):
        self.model = model

    def __call__(self, a, b, **kw):
        Ta, Ha, Wa, _ = frames_form(a, "ClipSimilarity")
        if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
            raise M324Error(f"ClipSimilarity: the two clips must have one shape and dtype, got {a.dtype} {tuple(a.shape)} and "
                            f"{b.dtype} {tuple(b.shape)}")
        f = self.model.features(torch.cat([a, b], 0), **kw).double()
        return cosine(f[:Ta], f[Ta:])


def cosine(fa: torch.Tensor, fb: torch.Tensor) -> torch.Tensor:
    """row-wise cosine in float64"""
    fa, fb = fa.double(), fb.double()
    return (fa * fb).sum(-1) / (fa.norm(dim=-1) * fb.norm(dim=-1))


def evaluate_clips_clip(gt, result, model, **kw) -> ClipScore:
    """Scores `result` against `gt` as the reference's process_single_video does with only_final=True: the cosine of every frame
    pair, the clip extended to whole 32-frame sub-videos by its reversed tail, mean and standard deviation over the kept
    frames.  model: a ClipVision, a ClipSimilarity or any callable (a, b, **kw) -> [T].  The clips have equal shapes and sides of
    1 to 16384 pixels; any size goes (the tower resizes)."""
    for x in (gt, result):
        frames_form(x, "evaluate_clips_clip")
    if tuple(gt.shape) != tuple(result.shape) or gt.dtype != result.dtype:
        raise M324Error(f"evaluate_clips_clip: the clips must have equal shapes, got {tuple(gt.shape)} and {tuple(result.shape)}")
    subvideo_frames(gt.shape[0])                        # refuses T < 16 before any work
    metric = ClipSimilarity(model) if isinstance(model, ClipVision) else model
    return clip_statistics(metric(gt, result, **kw).double().cpu().numpy())


def main(argv=None):
    parser = argparse.ArgumentParser(description="CLIP image similarity (open_clip ViT image tower) between ground-truth and result clips on the GPU")
    parser.add_argument("--gt_paths", type=str, required=True, nargs="+", help="frame directories or .npy clips")
    parser.add_argument("--result_paths", type=str, required=True, nargs="+")
    parser.add_argument("--weights", type=str, required=True, help="an open_clip checkpoint (state dict) with the image tower")
    parser.add_argument("--heads", type=int, default=None, help="attention heads of the tower; default: open_clip's named towers by width")
    parser.add_argument("--output_dir", type=str, default=None)
    args = parser.parse_args(argv)
    if len(args.gt_paths) != len(args.result_paths):
        raise M324Error(f"{len(args.gt_paths)} gt paths but {len(args.result_paths)} result paths: pairs are matched by position")
    weights = load_clip_vision_weights(args.weights, heads=args.heads)
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.clipsim needs a HIP device (there is no CPU path)")
    metric = ClipSimilarity(ClipVision(weights, "cuda"))
    results = []
    for gt_path, result_path in zip(args.gt_paths, args.result_paths):
        missing = [p for p in (gt_path, result_path) if not os.path.exists(p)]
        if missing:
            print(f"Warning: {missing[0]} not found, skipping")
            continue
        gt, result = (torch.from_numpy(load_frames(p)).to("cuda") for p in (gt_path, result_path))
        score = evaluate_clips_clip(gt, result, metric)
        results.append(score.value)
        line = f"{result_path}: CLIP similarity {score.value:.6f} (std {score.value_std:.6f}, {len(score.per_video)} sub-video(s))"
        if args.output_dir:
            base = os.path.basename(result_path.rstrip("/"))
            if os.path.isfile(result_path):
                base = os.path.splitext(base)[0]
            os.makedirs(args.output_dir, exist_ok=True)
            out_file = os.path.join(args.output_dir, base + ".clip.txt")
            with open(out_file, "w") as f:
                f.write(f"GT Source: {gt_path}\nResult Source: {result_path}\nCLIP Loss: {score.value}\n" + "-" * 50 + "\n")
            line += f" -> {out_file}"
        print(line)
    print(f"Summary: processed {len(results)}/{len(args.gt_paths)} pairs" + (f"; Average CLIP similarity: {np.mean(results):.6f}" if results else ""))
    return results


if __name__ == "__main__":
    main()
