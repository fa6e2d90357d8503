"""The ViT image tower behind CLIP similarity (clipsim) and DreamSim (dreamsim): its weights, the loader of both state-dict
layouts, the seeded weight generators and the runner.

One tower serves open_clip's VisionTransformer and timm's (DINO): a patch convolution with or without bias, the class token and
learned positions, an optional LayerNorm in front of the blocks, pre-norm residual blocks of a fused q|k|v projection, attention
and a GELU or QuickGELU MLP, a final LayerNorm and an optional projection.  Everything on the device is fp32: the Linears are
m324_gemm on the fp32 MFMA, attention, LayerNorm, patch rows and the token assembly are csrc/vit.hip.  The weights are the user's;
nothing is downloaded.
"""
from __future__ import annotations

import math
import os
import re
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .lib import ACT_GELU, ACT_QUICK_GELU, M324Error

OPENAI_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_STD = (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
CLIP_LN_EPS = 1e-5
DINO_LN_EPS = 1e-6                      # timm's VisionTransformer: partial(nn.LayerNorm, eps=1e-6)
HEADS_BY_WIDTH = {768: 12, 1024: 16, 1280: 16, 1408: 16, 1664: 16}       # open_clip's named towers: B, L, H, g, bigG
DINO_HEADS_BY_WIDTH = {192: 3, 384: 6, 768: 12, 1024: 16}                # timm's ViT-Ti / S / B / L
MAX_WIDTH = ops.LAYERNORM_WIDE_MAX_C
MAX_HEAD = ops.ATTN_TOK_MAX_D
FRAME_MAX_SIDE = 16384                  # M324_FRAME_MAX_SIDE
GEMM_K = 32                             # the fp32 GEMM contracts K in steps of 32: every K is padded with zero columns to it
DEFAULT_MAX_SCRATCH_BYTES = 2 << 30
TAPS = ("embed", "block0", "last_block", "cls_row")
FEATURES = ("embedding", "cls", "cls_prenorm")
ACTS = {"gelu": ACT_GELU, "quick_gelu": ACT_QUICK_GELU}


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _pad_k(w: torch.Tensor) -> torch.Tensor:
    """[N, K] -> contiguous [N, round_up(K, 32)], zeros behind K"""
    n, k = w.shape
    out = torch.zeros((n, _round_up(k, GEMM_K)), dtype=torch.float32)
    out[:, :k] = w
    return out


def tensor_of(v) -> torch.Tensor:
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))


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


# ------------------------------------------------------------------------------------------- weights
class VitBlock(NamedTuple):
    ln_1: tuple            # (weight [W], bias [W])
    in_proj: tuple         # (weight [3W, Wp], bias [3W]); the rows are q | k | v, each head-major
    out_proj: tuple        # (weight [W, Wp], bias [W])
    ln_2: tuple
    c_fc: tuple            # (weight [M, Wp], bias [M])
    c_proj: tuple          # (weight [W, Mp], bias [W])


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
    patch_w: torch.Tensor  # [W, Kp], Kp = round_up(3 patch^2, 32)
    patch_b: Optional[torch.Tensor]     # [W] or None
    cls: torch.Tensor      # [W]
    pos: torch.Tensor      # [L, W]
    ln_pre: Optional[tuple]
    blocks: tuple          # of VitBlock
    ln_post: tuple         # the final norm
    proj_t: Optional[torch.Tensor]      # [E, Wp]: proj transposed once, or None


def _load_file(path: str, who: str) -> dict:
    if not os.path.isfile(path):
        raise M324Error(f"{who}: no such file {path!r}")
    if path.lower().endswith(".safetensors"):
        try:
            from safetensors.torch import load_file
        except ImportError:
            raise M324Error(f"{who}: {path!r} is a .safetensors file and the safetensors package is not installed; "
                            "convert it to a torch.save'd state dict") from None
        return load_file(path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    if not isinstance(state, dict):
        raise M324Error(f"{who}: {path!r} holds a {type(state).__name__}, not a state dict")
    return state


def state_of(state_or_path, who: str) -> dict:
    """a state dict as it is, or the one in the file torch.load(weights_only=True) reads (.safetensors where that package is
    installed)"""
    state = _load_file(os.fspath(state_or_path), who) if isinstance(state_or_path, (str, os.PathLike)) else state_or_path
    if not isinstance(state, dict):
        raise M324Error(f"{who}: expected a state dict or a path to one")
    return state


def _open_clip_keys(state: dict, who: str) -> dict:
    """the image tower of an open_clip state dict: `visual.` and / or `module.` in front are stripped, and where some key has
    `visual.` the rest (the text tower, logit_scale) is skipped"""
    visual = re.compile(r"^(module\.)*visual\.")
    has_visual = any(visual.match(k) for k in state)
    return {re.sub(r"^(module\.|visual\.)+", "", k): v for k, v in state.items() if not has_visual or visual.match(k)}


_DINO_ANCHOR = "patch_embed.proj.weight"


def _dino_keys(state: dict, who: str) -> dict:
    """whatever prefix stands in front of patch_embed.proj.weight is stripped from every key that has it"""
    anchors = [k for k in state if k.endswith(_DINO_ANCHOR)]
    if len(anchors) != 1:
        raise M324Error(f"{who}: expected one key ending in {_DINO_ANCHOR!r}, found {sorted(anchors)}")
    prefix = anchors[0][:-len(_DINO_ANCHOR)]
    return {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}


class Layout(NamedTuple):
    """what tells one state-dict layout from the other; "required", "optional" or "refused" for the three parts a tower may lack"""
    keys: object           # (state, who) -> the tower's keys, prefixes stripped
    names: dict
    cls_lead: tuple        # the dimensions of size one in front of the class token's [W] and of the positions' [L, W]
    pos_lead: tuple
    patch_b: str
    ln_pre: str
    proj: str
    refused: tuple         # of (pattern, what it is)
    heads_by_width: dict
    towers: str


LAYOUTS = {
    "open_clip": Layout(
        _open_clip_keys,
        {"patch_w": "conv1.weight", "patch_b": "conv1.bias", "cls": "class_embedding", "pos": "positional_embedding", "ln_pre": "ln_pre",
         "block": "transformer.resblocks.{}.", "ln_1": "ln_1", "qkv_w": "attn.in_proj_weight", "qkv_b": "attn.in_proj_bias",
         "proj": "attn.out_proj", "ln_2": "ln_2", "fc1": "mlp.c_fc", "fc2": "mlp.c_proj", "norm": "ln_post"},
        (), (), "refused", "required", "required",
        ((r"(^|\.)ls_[12](\.|$)", "layer scale (ls_1 / ls_2)"), (r"attn_pool", "attentional pooling (attn_pool)")),
        HEADS_BY_WIDTH, "open_clip's named towers"),
    "dino": Layout(
        _dino_keys,
        {"patch_w": _DINO_ANCHOR, "patch_b": "patch_embed.proj.bias", "cls": "cls_token", "pos": "pos_embed", "ln_pre": "norm_pre",
         "block": "blocks.{}.", "ln_1": "norm1", "qkv_w": "attn.qkv.weight", "qkv_b": "attn.qkv.bias",
         "proj": "attn.proj", "ln_2": "norm2", "fc1": "mlp.fc1", "fc2": "mlp.fc2", "norm": "norm"},
        (1, 1), (1,), "required", "optional", "optional",
        ((r"(^|\.)(ls1|ls2|gamma_1|gamma_2)(\.|$)", "layer scale"), (r"^(reg_token|register_tokens|dist_token)", "register / distillation tokens")),
        DINO_HEADS_BY_WIDTH, "the named towers"),
}


def _layout_of(state: dict, who: str) -> str:
    if any(k.endswith(_DINO_ANCHOR) for k in state):
        return "dino"
    if any(k.endswith("conv1.weight") for k in state):
        return "open_clip"
    raise M324Error(f"{who}: the state dict has neither 'conv1.weight' (open_clip layout) nor 'patch_embed.proj.weight' "
                    "(DINO / timm layout)")


def load_vit_weights(state_or_path, layout: Optional[str] = None, heads: Optional[int] = None) -> VitWeights:
    """A ViT tower's weights, checked and repacked once (fp32 CPU tensors; VitTower moves them to its device).  state_or_path: a
    state dict or a file (state_of).  Two layouts, told apart by their keys (or `layout`): "open_clip" (conv1.weight without a
    bias, class_embedding [W], positional_embedding [L,W], ln_pre, transformer.resblocks.{i}.ln_1 / attn.in_proj_{weight,bias} /
    attn.out_proj / ln_2 / mlp.c_fc / mlp.c_proj, ln_post, proj [W,E]; `visual.` and / or `module.` may stand in front and the
    text tower's keys are ignored) and "dino" (timm's VisionTransformer: cls_token [1,1,W], pos_embed [1,L,W],
    patch_embed.proj.{weight,bias}, blocks.{i}.norm1 / attn.qkv / attn.proj / norm2 / mlp.fc1 / mlp.fc2, norm, and optionally
    norm_pre.* and proj [W,E]; whatever stands in front of patch_embed.proj.weight is stripped from every key).  The fused
    projection's rows are q | k | v, each head-major: nn.MultiheadAttention's order.  Sizes come from the shapes; the head count
    is not in a state dict: `heads`, or the layout's named towers by width.  What the tower does not do is refused by the key or
    shape that shows it."""
    return _load_weights(state_or_path, layout, heads, "load_vit_weights")


def load_clip_vision_weights(state_or_path, heads: Optional[int] = None) -> VitWeights:
    """The image tower of an open_clip checkpoint: load_vit_weights(state_or_path, "open_clip", heads) under its own name"""
    return _load_weights(state_or_path, "open_clip", heads, "load_clip_vision_weights")


def _load_weights(state_or_path, layout, heads, who: str) -> VitWeights:
    state = state_of(state_or_path, who)
    layout = _layout_of(state, who) if layout is None else layout
    if layout not in LAYOUTS:
        raise M324Error(f"{who}: layout must be 'open_clip' or 'dino', got {layout!r}")
    lay = LAYOUTS[layout]
    names = lay.names
    vis = lay.keys(state, who)
    for k in vis:
        for pattern, what in lay.refused:
            if re.search(pattern, k):
                raise M324Error(f"{who}: key {k!r}: {what} is not part of this tower")

    def get(key, shape=None, dims=None):
        if key not in vis:
            raise M324Error(f"{who}: the state dict has no key {key!r}")
        t = tensor_of(vis[key])
        if (shape is not None and tuple(t.shape) != tuple(shape)) or (dims is not None and t.dim() != dims):
            want = tuple(shape) if shape is not None else f"{dims} dimensions"
            raise M324Error(f"{who}: {key!r} has shape {tuple(t.shape)}, expected {want}")
        t = t.detach().to(torch.float32).cpu()
        if not torch.isfinite(t).all():
            raise M324Error(f"{who}: {key!r} holds values that are not finite")
        return t.contiguous()

    def has(rule, key):
        if rule == "refused" and key in vis:
            raise M324Error(f"{who}: key {key!r} is not part of this tower (the {layout} layout has none)")
        return rule == "required" or (rule == "optional" and key in vis)

    conv = get(names["patch_w"], dims=4)
    W, cin, p, p2 = conv.shape
    if cin != 3 or p != p2:
        raise M324Error(f"{who}: {names['patch_w']!r} has shape {tuple(conv.shape)}, expected [W, 3, patch, patch]")
    if W > MAX_WIDTH:
        raise M324Error(f"{who}: {names['patch_w']!r} {tuple(conv.shape)}: width {W}: W > {MAX_WIDTH} is not supported")
    if W % 4:
        raise M324Error(f"{who}: {names['patch_w']!r} {tuple(conv.shape)}: width {W} is no multiple of 4")
    pos = get(names["pos"], dims=len(lay.pos_lead) + 2)
    L = pos.shape[-2]
    g = math.isqrt(max(L - 1, 0))
    if tuple(pos.shape[:-2]) != lay.pos_lead or pos.shape[-1] != W or L < 2 or g * g != L - 1:
        want = ", ".join(str(d) for d in lay.pos_lead + ("1 + g * g", W))
        raise M324Error(f"{who}: {names['pos']!r} has shape {tuple(pos.shape)}: expected [{want}], a class token and a square grid "
                        f"(a non-square grid is not supported)")
    block0 = names["block"].format(0)
    if heads is None:
        if W not in lay.heads_by_width:
            raise M324Error(f"{who}: the head count is not part of a state dict and width {W} is none of {lay.towers} "
                            f"{sorted(lay.heads_by_width)}; pass heads=")
        heads = lay.heads_by_width[W]
    heads = int(heads)
    if heads < 1 or W % heads:
        raise M324Error(f"{who}: width {W} is not divisible by heads={heads} (W % heads != 0)")
    D = W // heads
    if D % 8:
        raise M324Error(f"{who}: {block0 + names['qkv_w']!r}: head width {D} = {W} / {heads}: D % 8 != 0 is not supported")
    if D > MAX_HEAD:
        raise M324Error(f"{who}: {block0 + names['qkv_w']!r}: head width {D} = {W} / {heads}: D > {MAX_HEAD} is not supported")
    layers = 0
    while names["block"].format(layers) + names["ln_1"] + ".weight" in vis:
        layers += 1
    if layers == 0:
        raise M324Error(f"{who}: the state dict has no key {block0 + names['ln_1'] + '.weight'!r}")
    mlp = get(block0 + names["fc1"] + ".weight", dims=2).shape[0]
    if mlp % 4:
        raise M324Error(f"{who}: {block0 + names['fc1'] + '.weight'!r}: an MLP width of {mlp} is no multiple of 4")

    def ln(name):
        return get(name + ".weight", (W,)), get(name + ".bias", (W,))

    def linear(name, n, k):
        return _pad_k(get(name + ".weight", (n, k))), get(name + ".bias", (n,))

    blocks = []
    for i in range(layers):
        b = names["block"].format(i)
        blocks.append(VitBlock(ln(b + names["ln_1"]), (_pad_k(get(b + names["qkv_w"], (3 * W, W))), get(b + names["qkv_b"], (3 * W,))),
                               linear(b + names["proj"], W, W), ln(b + names["ln_2"]), linear(b + names["fc1"], mlp, W),
                               linear(b + names["fc2"], W, mlp)))
    patch_b = get(names["patch_b"], (W,)) if has(lay.patch_b, names["patch_b"]) else None
    ln_pre = ln(names["ln_pre"]) if has(lay.ln_pre, names["ln_pre"] + ".weight") else None
    proj_t, embed = None, 0
    if has(lay.proj, "proj"):
        proj = get("proj", dims=2)
        if proj.shape[0] != W or proj.shape[1] % 4:
            raise M324Error(f"{who}: 'proj' has shape {tuple(proj.shape)}, expected [{W}, E] with E a multiple of 4")
        proj_t, embed = _pad_k(proj.t()), proj.shape[1]
    return VitWeights(W, heads, layers, mlp, p, g * p, L, embed, _pad_k(conv.reshape(W, 3 * p * p)), patch_b,
                      get(names["cls"], lay.cls_lead + (W,)).reshape(W).contiguous(), pos.reshape(L, W).contiguous(), ln_pre,
                      tuple(blocks), ln(names["norm"]), proj_t)


# ------------------------------------------------------------------------------------------- seeded weights
def _synth(who: str, seed: int, width: int, heads: int, patch: int, image: int):
    if width % heads or image % patch:
        raise M324Error(f"{who}: width {width} / heads {heads} or image {image} / patch {patch} does not divide")
    g = torch.Generator().manual_seed(int(seed))

    def randn(*shape, scale=1.0):
        return torch.randn(shape, generator=g) * scale

    def ln(sd, name):
        sd[name + ".weight"] = 1.0 + randn(width, scale=0.1)
        sd[name + ".bias"] = randn(width, scale=0.05)

    return randn, ln


def _synth_blocks(sd: dict, randn, ln, names: dict, layers: int, width: int, mlp: int):
    """the blocks of either layout, in one order of draws: the two norms, the fused projection (its q and k rows twice the
    size, so that the softmax is not flat), the output projection, the MLP"""
    for i in range(layers):
        b = names["block"].format(i)
        ln(sd, b + names["ln_1"])
        ln(sd, b + names["ln_2"])
        w = randn(3 * width, width, scale=1.0 / math.sqrt(width))
        w[:2 * width] *= 2.0
        sd[b + names["qkv_w"]] = w
        sd[b + names["qkv_b"]] = randn(3 * width, scale=0.05)
        for name, n, k in ((names["proj"], width, width), (names["fc1"], mlp, width), (names["fc2"], width, mlp)):
            sd[b + name + ".weight"] = randn(n, k, scale=1.0 / math.sqrt(k))
            sd[b + name + ".bias"] = randn(n, scale=0.05)


def synth_clip_state_dict(seed: int, width: int, layers: int, heads: int, mlp: int, patch: int, image: int, embed: int) -> dict:
    """Seeded weights in the form of an open_clip VisionTransformer state dict (no prefix), of trained-like scale, for tests and
    timing: Linear weights randn / sqrt(fan-in), LayerNorm weights around 1, small biases, a patch projection, class token and
    positions of size 0.1 (ln_pre brings the stream to size one).  `heads` only checks the width: a state dict does not hold it."""
    randn, ln = _synth("synth_clip_state_dict", seed, width, heads, patch, image)
    L = (image // patch) ** 2 + 1
    sd = {"conv1.weight": randn(width, 3, patch, patch, scale=0.1 / math.sqrt(3 * patch * patch)),
          "class_embedding": randn(width, scale=0.1), "positional_embedding": randn(L, width, scale=0.1)}
    ln(sd, "ln_pre")
    _synth_blocks(sd, randn, ln, LAYOUTS["open_clip"].names, layers, width, mlp)
    ln(sd, "ln_post")
    sd["proj"] = randn(width, embed, scale=1.0 / math.sqrt(width))
    return sd


def synth_dino_state_dict(seed: int, width: int, layers: int, heads: int, mlp: int, patch: int, image: int, embed: int = 0,
                          norm_pre: bool = False) -> dict:
    """Seeded weights in the form of a timm VisionTransformer state dict (no prefix), in the manner of synth_clip_state_dict.  The
    patch projection, its bias, the class token and the positions have size 0.1 and nothing normalises them before block 0: norm1
    of block 0 sees a variance near 0.03, where an eps of 1e-5 in place of 1e-6 moves the result by 1e-4 relative -- far outside
    an fp32 band."""
    randn, ln = _synth("synth_dino_state_dict", seed, width, heads, patch, image)
    L = (image // patch) ** 2 + 1
    sd = {"cls_token": randn(1, 1, width, scale=0.1), "pos_embed": randn(1, L, width, scale=0.1),
          "patch_embed.proj.weight": randn(width, 3, patch, patch, scale=0.1 / math.sqrt(3 * patch * patch)),
          "patch_embed.proj.bias": randn(width, scale=0.1)}
    if norm_pre:
        ln(sd, "norm_pre")
    _synth_blocks(sd, randn, ln, LAYOUTS["dino"].names, layers, width, mlp)
    ln(sd, "norm")
    if embed:
        sd["proj"] = randn(width, embed, scale=1.0 / math.sqrt(width))
    return sd


# ------------------------------------------------------------------------------------------- the tower
def staged(stage_events, label: str, fn):
    """fn(), between two device events that go to the list stage_events as (label, start, end) when there is one"""
    if stage_events is None:
        return fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    r = fn()
    end.record()
    stage_events.append((label, start, end))
    return r


class VitTower:
    """tower = VitTower(weights, device, act=, ln_eps=, mean=, std=, feature=); tower.features(img) -> fp32 [F, E] of fp32 planar
    images [F,3,S,S] that are already S = tower.image pixels a side and in [0, 1]: the tower normalises them itself, in its patch
    rows.  feature: "embedding" = the class row after the last LayerNorm times proj (open_clip's encode_image), "cls" = the
    class row after the final norm, "cls_prenorm" = the class row of the last block's output.  weights: a VitWeights, or whatever
    load_vit_weights accepts."""

    def __init__(self, weights, device="cuda", act: str = "gelu", ln_eps: float = CLIP_LN_EPS, mean=OPENAI_MEAN, std=OPENAI_STD,
                 feature: str = "embedding"):
        self.who = who = type(self).__name__
        if act not in ACTS:
            raise M324Error(f"{who}: act must be 'gelu' or 'quick_gelu', got {act!r}")
        if feature not in FEATURES:
            raise M324Error(f"{who}: feature must be one of {FEATURES}, got {feature!r}")
        if not isinstance(weights, VitWeights):
            weights = load_vit_weights(weights)
        if feature == "embedding" and weights.proj_t is None:
            raise M324Error(f"{who}: feature='embedding' needs a 'proj' in the weights")
        if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std) or not float(ln_eps) > 0.0:
            raise M324Error(f"{who}: mean and std are three numbers each (std not zero) and ln_eps is positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise M324Error(f"{who}: needs a HIP device (there is no CPU path)")
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
        self.blocks = tuple(VitBlock(*(to(part) for part in blk)) for blk in w.blocks)
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
            raise M324Error(f"{self.who}: one image needs {per} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
        return max(1, min(int(n_images), int(max_scratch_bytes) // per))

    def _buffers(self, n: int) -> dict:
        """the scratch of a chunk of n images"""
        L, W, dev, f32 = self.tokens, self.width, self.device, torch.float32
        # y and hid keep zeros in their K-padding columns: the kernels write the first W (mlp) columns only
        return {"rows": torch.empty((n * (L - 1), self.Kp), dtype=f32, device=dev), "pe": torch.empty((n * (L - 1), W), dtype=f32, device=dev),
                "x": torch.empty((n * L, W), dtype=f32, device=dev), "y": torch.zeros((n * L, self.Wp), dtype=f32, device=dev),
                "qkv": torch.empty((n * L, 3 * W), dtype=f32, device=dev), "hid": torch.zeros((n * L, self.Mp), dtype=f32, device=dev),
                "pooled": torch.zeros((n, self.Wp), dtype=f32, device=dev)}

    def _outputs(self, T: int, taps: bool):
        """(features [T, out_dim], the taps' tensors by TAPS or None)"""
        L, W, dev, f32 = self.tokens, self.width, self.device, torch.float32
        out = torch.empty((T, self.out_dim), dtype=f32, device=dev)
        return out, {k: torch.empty((T, L, W) if k != "cls_row" else (T, W), dtype=f32, device=dev) for k in TAPS} if taps else None

    def features(self, img, taps: bool = False, max_scratch_bytes: int = DEFAULT_MAX_SCRATCH_BYTES, stage_events=None):
        """img: fp32 planar [F,3,S,S], S = self.image, on the tower's device.  Returns fp32 [F, out_dim]; with taps also a dict of
        the stream [F, L, W] after the embedding or the LayerNorm in front of the blocks ("embed"), after block 0 ("block0") and
        after the last block ("last_block"), and the class rows [F, W] the feature is made of ("cls_row").  The images pass the
        tower `images_per_chunk` at a time; the result does not depend on the chunking and nothing synchronises.  stage_events:
        a list that receives (label, start, end) device events."""
        if not isinstance(img, torch.Tensor) or not img.is_cuda or img.device != self.device:
            raise M324Error(f"{self.who}: the images must be on {self.device} (there is no CPU path)")
        if img.dtype != torch.float32 or img.dim() != 4 or tuple(img.shape[1:]) != (3, self.image, self.image) or img.shape[0] < 1:
            raise M324Error(f"{self.who}: expected fp32 [F,3,{self.image},{self.image}], got {img.dtype} {tuple(img.shape)}")
        T = img.shape[0]
        img = img.detach().contiguous()
        n = self.images_per_chunk(T, max_scratch_bytes)
        bufs = self._buffers(n)
        out, tap = self._outputs(T, taps)
        for t0 in range(0, T, n):
            t1 = min(T, t0 + n)
            self._chunk(img[t0:t1], bufs, out[t0:t1], {k: v[t0:t1] for k, v in tap.items()} if taps else None, stage_events)
        return (out, tap) if taps else out

    def _chunk(self, images, bufs, out, tap, stage_events):
        """one chunk through the tower.  images: fp32 planar [n,3,S,S] in [0, 1] or bytes [n,S,S,3], S = self.image; each form has
        its own patch-row kernel and everything behind the patch rows is shared"""
        n, L, W, H, D = images.shape[0], self.tokens, self.width, self.heads, self.head_dim
        M, eps = n * L, self.ln_eps

        def run(label, fn):
            return staged(stage_events, label, fn)

        x, y, qkv, hid = bufs["x"][:M], bufs["y"][:M], bufs["qkv"][:M], bufs["hid"][:M]
        rows, pe, pooled = bufs["rows"][:n * (L - 1)], bufs["pe"][:n * (L - 1)], bufs["pooled"][:n]
        yw, hw = y[:, :W], hid[:, :self.mlp]
        patches = ops.vit_patches if images.dtype == torch.uint8 else ops.vit_patches_f32
        run("patch_rows", lambda: patches(images, self.patch, self.mean_std, self.Kp, out=rows))
        run("gemm_patch", lambda: ops.gemm(rows, self.patch_w, pe, bias=self.patch_b))
        if self.ln_pre is not None:
            tokens = qkv.view(-1)[:M * W].view(M, W)      # q|k|v is free until block 0: the stream starts at ln_pre's output
            run("tokens", lambda: ops.vit_tokens(pe, self.cls, self.pos, out=tokens))
            run("layernorm", lambda: ops.layernorm_wide(tokens, *self.ln_pre, eps, out=x))
        else:
            run("tokens", lambda: ops.vit_tokens(pe, self.cls, self.pos, out=x))
        if tap is not None:
            tap["embed"].copy_(x.view(n, L, W))
        for i, blk in enumerate(self.blocks):
            run("layernorm", lambda: ops.layernorm_wide(x, *blk.ln_1, eps, out=yw))
            run("gemm_qkv", lambda: ops.gemm(y, blk.in_proj[0], qkv, bias=blk.in_proj[1]))
            run("attention", lambda: ops.attention_tok(qkv, n, L, H, D, D ** -0.5, out=yw))
            run("gemm_proj", lambda: ops.gemm(y, blk.out_proj[0], x, bias=blk.out_proj[1], residual=x))
            run("layernorm", lambda: ops.layernorm_wide(x, *blk.ln_2, eps, out=yw))
            run("gemm_fc1", lambda: ops.gemm(y, blk.c_fc[0], hw, bias=blk.c_fc[1], act=self.act_code))
            run("gemm_fc2", lambda: ops.gemm(hid, blk.c_proj[0], x, bias=blk.c_proj[1], residual=x))
            if tap is not None and i == 0:
                tap["block0"].copy_(x.view(n, L, W))
        if tap is not None:
            tap["last_block"].copy_(x.view(n, L, W))
        cls_rows = x.view(n, L, W)[:, 0]                  # the class rows: a [n, W] view with leading dimension L * W
        if self.feature == "cls_prenorm":
            out.copy_(cls_rows)
        elif self.feature == "cls":
            run("layernorm", lambda: ops.layernorm_wide(cls_rows, *self.ln_post, eps, out=out))
        else:
            run("layernorm", lambda: ops.layernorm_wide(cls_rows, *self.ln_post, eps, out=pooled[:, :W]))
            run("gemm_head", lambda: ops.gemm(pooled, self.proj_t, out))
        if tap is not None:
            tap["cls_row"].copy_(out if self.feature != "embedding" else pooled[:, :W])
