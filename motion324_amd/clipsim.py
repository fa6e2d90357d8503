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
import os

import numpy as np
import torch

from . import framing, ops, vit
from .lib import M324Error
from .perceptual import ClipScore, clip_statistics, load_frames, subvideo_frames
from .vit import (CLIP_LN_EPS, DEFAULT_MAX_SCRATCH_BYTES, FRAME_MAX_SIDE, HEADS_BY_WIDTH, OPENAI_MEAN, OPENAI_STD, VitBlock as ClipBlock,
                  VitTower, VitWeights as ClipVisionWeights, frames_form, load_clip_vision_weights, staged, synth_clip_state_dict)

TAPS = ("ln_pre", "block0", "last_block", "ln_post")       # the tower's vit.TAPS under this metric's names


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


class ClipVision(VitTower):
    """tower = ClipVision(weights, device); tower.features(frames) -> fp32 [T, E], open_clip's encode_image before any
    normalisation: the GELU tower of the "CLIP Loss" line (feature "embedding", eps 1e-5) behind its byte preprocessing.
    weights: a ClipVisionWeights, or whatever load_clip_vision_weights accepts."""

    def __init__(self, weights, device="cuda", act: str = "gelu", mean=OPENAI_MEAN, std=OPENAI_STD):
        if act == "quick_gelu":
            raise M324Error("ClipVision: act='quick_gelu' (the OpenAI-pretrained towers) is not supported: ClipVision is the GELU tower "
                            "of the \"CLIP Loss\" line; vit.VitTower(act='quick_gelu') runs such weights")
        if act != "gelu":
            raise M324Error(f"ClipVision: act must be 'gelu', got {act!r}")
        if not isinstance(weights, ClipVisionWeights):
            weights = load_clip_vision_weights(weights)
        super().__init__(weights, device, act, CLIP_LN_EPS, mean, std, "embedding")

    def bytes_per_image(self) -> int:
        """the tower's scratch of one image and its preprocessed bytes (the resize intermediate of the source size is not counted)"""
        return super().bytes_per_image() + 3 * self.image ** 2

    def features(self, frames, *, taps: bool = False, max_scratch_bytes: int = DEFAULT_MAX_SCRATCH_BYTES, stage_events=None):
        """frames: uint8 [T,H,W,3] or fp32 [T,3,H,W] in [0, 1] on the tower's device.  Returns fp32 [T, E]; with taps also a dict
        of the stream [T, L, W] after ln_pre ("ln_pre"), after block 0 ("block0") and after the last block ("last_block") and
        the ln_post class rows [T, W] ("ln_post").  The images are preprocessed and pass the tower `images_per_chunk` at a time;
        the result does not depend on the chunking and nothing synchronises.  stage_events: a list that receives (label, start,
        end) device events."""
        T = frames_form(frames, "ClipVision")[0]
        if not frames.is_cuda or frames.device != self.device:
            raise M324Error(f"ClipVision: the frames must be on {self.device} (there is no CPU path)")
        n = self.images_per_chunk(T, max_scratch_bytes)
        bufs = self._buffers(n)
        out, tap = self._outputs(T, taps)
        for t0 in range(0, T, n):
            t1 = min(T, t0 + n)
            # the preprocessed bytes are this call's argument only: one chunk's are alive at a time
            self._chunk(staged(stage_events, "preprocess", lambda: preprocess(frames[t0:t1], self.image, self.mean, self.std)), bufs,
                        out[t0:t1], {k: v[t0:t1] for k, v in tap.items()} if taps else None, stage_events)
        return (out, dict(zip(TAPS, (tap[k] for k in vit.TAPS)))) if taps else out


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
