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
import os
import re
from typing import Optional

import numpy as np
import torch

from . import ops
from .lib import M324Error
from .perceptual import ClipScore, clip_statistics, load_frames, subvideo_frames
from .vit import (CLIP_LN_EPS, DEFAULT_MAX_SCRATCH_BYTES, DINO_HEADS_BY_WIDTH, DINO_LN_EPS, FEATURES, IMAGENET_MEAN, IMAGENET_STD, OPENAI_MEAN,
                  OPENAI_STD, TAPS, VitTower, VitWeights, frames_form, load_vit_weights, state_of, synth_dino_state_dict, tensor_of)

RESIZE_SCRATCH_BYTES = 256 << 20        # the intermediate of the first resize pass, per chunk of frames


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


# ------------------------------------------------------------------------------------------- LoRA
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
        pairs.setdefault(m["module"], {})[m["which"]] = (k, tensor_of(v).detach().to(torch.float64).cpu())
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
        base = tensor_of(state[hits[0]])
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1] or A.shape[0] < 1 or tuple(base.shape) != (B.shape[0], A.shape[1]):
            raise M324Error(f"{who}: adapter key {ka!r}: lora_A {tuple(A.shape)} and lora_B {tuple(B.shape)} do not fit the base weight "
                            f"{hits[0]!r} {tuple(base.shape)}")
        r = A.shape[0]
        merged = base.detach().to(torch.float64).cpu() + (float(alpha) / r) * (B @ A)
        if not torch.isfinite(merged).all():
            raise M324Error(f"{who}: adapter key {ka!r}: the merged weight is not finite")
        out[hits[0]] = merged.to(base.dtype if base.dtype.is_floating_point else torch.float32)
    return out

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
    states = [state_of(s, "build_ensemble") for s in (dino, clip, open_clip)]
    if lora is not None:
        if lora_alpha is None:
            raise M324Error("build_ensemble: lora needs lora_alpha (the adapter's adapter_config.json has it)")
        states[0] = merge_lora(states[0], state_of(lora, "build_ensemble"), lora_alpha)
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