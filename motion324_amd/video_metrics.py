"""The reference's result file from one command line: FVD, LPIPS, DreamSim and CLIP Loss of every clip pair, for whichever of the
four metrics weights were given.

The reference's evaluation/evaluation.py writes, per pair, `<result name>.txt` with the lines `GT Source`, `Result Source`, `FVD`,
`LPIPS`, `DreamSim`, `CLIP Loss` and a rule of 50 dashes.  This module writes the same file with the lines of the metrics it was
given weights for, in that order.  It adds no arithmetic: the values are those of fvd.evaluate_clips_fvd,
perceptual.evaluate_clips, dreamsim.evaluate_clips_dreamsim and clipsim.evaluate_clips_clip.

    python -m motion324_amd.video_metrics --gt_paths A ... --result_paths B ... [--fvd i3d_torchscript.pt] [--lpips FILE [FILE]]
        [--dino FILE --clip FILE --open_clip FILE [--lora FILE --lora_alpha X]] [--clip_loss open_clip_pytorch_model.bin [--clip_heads N]]
        [--output_dir DIR]
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .lib import M324Error

ORDER = ("FVD", "LPIPS", "DreamSim", "CLIP Loss")           # the reference's line order
RULE = "-" * 50


def result_file(result_path: str, output_dir=None) -> str:
    """<output_dir or the result's own directory>/<the result's base name>.txt, as the reference names it"""
    base = os.path.basename(result_path.rstrip("/"))
    if os.path.isfile(result_path):
        base = os.path.splitext(base)[0]
    out_dir = output_dir if output_dir else os.path.dirname(result_path.rstrip("/"))
    return os.path.join(out_dir, base + ".txt")


def format_result(gt_path: str, result_path: str, values: dict) -> str:
    """the text of one result file: the two sources, the given metrics' lines in the reference's order, the rule"""
    unknown = [k for k in values if k not in ORDER]
    if unknown:
        raise M324Error(f"video_metrics: unknown metric {unknown[0]!r}; the reference's lines are {ORDER}")
    lines = [f"GT Source: {gt_path}", f"Result Source: {result_path}"] + [f"{k}: {values[k]}" for k in ORDER if k in values]
    return "\n".join(lines + [RULE]) + "\n"


def evaluate_pairs(gt_paths, result_paths, scorers: dict, output_dir=None, load=None, log=print):
    """Runs the given scorers over every pair and writes one result file per pair.  scorers: {line name: callable (gt, result) ->
    float} for any subset of ORDER; load: path -> clip (default: perceptual.load_frames onto the device).  Returns the list of
    (output file, {line name: value}) of the pairs that were found."""
    unknown = [k for k in scorers if k not in ORDER]
    if unknown or not scorers:
        raise M324Error(f"video_metrics: scorers must be a non-empty subset of {ORDER}, got {sorted(scorers)}")
    if len(gt_paths) != len(result_paths):
        raise M324Error(f"{len(gt_paths)} gt paths but {len(result_paths)} result paths: pairs are matched by position")
    if load is None:
        from .perceptual import load_frames

        def load(path):
            return torch.from_numpy(load_frames(path)).to("cuda")
    done = []
    for gt_path, result_path in zip(gt_paths, result_paths):
        missing = [p for p in (gt_path, result_path) if not os.path.exists(p)]
        if missing:
            log(f"Warning: {missing[0]} not found, skipping")
            continue
        gt, result = load(gt_path), load(result_path)
        values = {k: float(scorers[k](gt, result)) for k in ORDER if k in scorers}
        out_file = result_file(result_path, output_dir)
        if os.path.dirname(out_file):
            os.makedirs(os.path.dirname(out_file), exist_ok=True)
        with open(out_file, "w") as f:
            f.write(format_result(gt_path, result_path, values))
        log(f"{result_path}: " + ", ".join(f"{k} {v:.6f}" for k, v in values.items()) + f" -> {out_file}")
        done.append((out_file, values))
    summary = f"Summary: processed {len(done)}/{len(gt_paths)} pairs"
    for k in ORDER:
        if k in scorers and done:
            summary += f"; Average {k}: {np.mean([v[k] for _, v in done]):.6f}"
    log(summary)
    return done


def main(argv=None):
    parser = argparse.ArgumentParser(description="FVD, LPIPS, DreamSim and CLIP Loss between ground-truth and result clips on the GPU: the "
                                                 "reference's result file, with the lines of the metrics whose weights are given")
    parser.add_argument("--gt_paths", type=str, required=True, nargs="+", help="frame directories or .npy clips")
    parser.add_argument("--result_paths", type=str, required=True, nargs="+")
    parser.add_argument("--fvd", type=str, default=None, help="i3d_torchscript.pt, or a state dict of the PyTorch port of I3D")
    parser.add_argument("--lpips", type=str, default=None, nargs="+", help="the LPIPS module's state dict, or torchvision's VGG16 and vgg.pth")
    parser.add_argument("--dino", type=str, default=None, help="DreamSim: the DINO ViT-B/16 state dict (timm layout)")
    parser.add_argument("--clip", type=str, default=None, help="DreamSim: OpenAI CLIP ViT-B/16 (open_clip layout, QuickGELU)")
    parser.add_argument("--open_clip", type=str, default=None, help="DreamSim: open_clip's ViT-B/16 (open_clip layout, GELU)")
    parser.add_argument("--lora", type=str, default=None)
    parser.add_argument("--lora_alpha", type=float, default=None)
    parser.add_argument("--clip_loss", type=str, default=None, help="CLIP Loss: an open_clip checkpoint with the image tower")
    parser.add_argument("--clip_heads", type=int, default=None)
    parser.add_argument("--output_dir", type=str, default=None)
    args = parser.parse_args(argv)
    if len(args.gt_paths) != len(args.result_paths):
        raise M324Error(f"{len(args.gt_paths)} gt paths but {len(args.result_paths)} result paths: pairs are matched by position")
    dream = [args.dino, args.clip, args.open_clip]
    if any(dream) and not all(dream):
        raise M324Error("DreamSim needs all three of --dino, --clip and --open_clip")
    if not (args.fvd or args.lpips or all(dream) or args.clip_loss):
        raise M324Error("give the weights of at least one metric: --fvd, --lpips, --dino/--clip/--open_clip, --clip_loss")
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.video_metrics needs a HIP device (there is no CPU path)")
    scorers = {}
    if args.fvd:
        from . import fvd
        i3d = fvd.I3D(fvd.load_i3d_weights(args.fvd), "cuda")
        scorers["FVD"] = lambda gt, result: fvd.evaluate_clips_fvd(gt, result, i3d).value
    if args.lpips:
        from . import perceptual
        if len(args.lpips) > 2:
            raise M324Error("--lpips takes one file or two")
        lp = perceptual.LPIPS(perceptual.load_lpips_weights(*args.lpips), "cuda")
        scorers["LPIPS"] = lambda gt, result: perceptual.evaluate_clips(gt, result, lp).value
    if all(dream):
        from . import dreamsim
        ds = dreamsim.build_ensemble(args.dino, args.clip, args.open_clip, "cuda", args.lora, args.lora_alpha)
        scorers["DreamSim"] = lambda gt, result: dreamsim.evaluate_clips_dreamsim(gt, result, ds).value
    if args.clip_loss:
        from . import clipsim
        cs = clipsim.ClipSimilarity(clipsim.ClipVision(clipsim.load_clip_vision_weights(args.clip_loss, heads=args.clip_heads), "cuda"))
        scorers["CLIP Loss"] = lambda gt, result: clipsim.evaluate_clips_clip(gt, result, cs).value
    return evaluate_pairs(args.gt_paths, args.result_paths, scorers, args.output_dir)


if __name__ == "__main__":
    main()
