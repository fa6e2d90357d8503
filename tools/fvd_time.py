"""Times FVD's detector (I3D) on a device-resident pair of 32-frame sub-videos with seeded weights:
python tools/fvd_time.py [--frames 32 --size 512 --pairs 1]

Device events around the call, one warm-up, the median of 5 with min and max: the time per sub-video PAIR (the two sides of one
comparison pass the trunk as one batch of two).  Per-stage time of the prepare kernel, the stem, the four stages behind the pools
and the head from events inside the call.  The executed multiply-adds (the stem's padded fourth channel included) are set against
the fp32 matrix peak (157.3 TFLOP/s).  Prints a markdown table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from motion324_amd import fvd as V  # noqa: E402

PEAK_TFLOPS = 157.3
REPEATS = 5
PARTS = ("prepare", "stem", "stage2", "stage3", "stage4", "stage5", "head")


def timed(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times), min(times), max(times)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=32)
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--pairs", type=int, nargs="+", default=[1, 4])
    args = parser.parse_args(argv)
    T, S = args.frames, args.size
    model = V.I3D(V.load_i3d_weights(V.synth_i3d_state_dict(0)), "cuda")
    macs = V.trunk_macs(T, model.resolution, model.resolution)
    flop_video = 2 * sum(macs.values())
    result = {"frames": T, "size": S, "gflop_per_subvideo": flop_video / 1e9, "runs": []}
    print(f"I3D, sub-videos of {T} frames of {S} x {S} -> {model.resolution} x {model.resolution}: {flop_video / 1e9:.1f} GFLOP each\n")
    print("| pairs per call | median ms | min | max | ms per pair | TFLOP/s | of peak |")
    print("|---|---|---|---|---|---|---|")
    g = torch.Generator().manual_seed(1)
    for pairs in args.pairs:
        videos = torch.randint(0, 256, (2 * pairs, T, S, S, 3), generator=g, dtype=torch.uint8).to("cuda")
        med, lo, hi = timed(lambda: model.features(videos))
        tf = 2 * pairs * flop_video / med / 1e9
        result["runs"].append({"pairs": pairs, "ms": med, "min": lo, "max": hi, "ms_per_pair": med / pairs, "tflops": tf})
        print(f"| {pairs} | {med:.2f} | {lo:.2f} | {hi:.2f} | {med / pairs:.2f} | {tf:.1f} | {100 * tf / PEAK_TFLOPS:.0f} % |")

    pairs = args.pairs[0]
    videos = torch.randint(0, 256, (2 * pairs, T, S, S, 3), generator=g, dtype=torch.uint8).to("cuda")
    model.features(videos)
    events = []
    model.features(videos, stage_events=events)
    torch.cuda.synchronize()
    spent = {}
    for label, start, end in events:
        spent[label] = spent.get(label, 0.0) + start.elapsed_time(end)
    print(f"\nper part at {pairs} pair(s) per call (events inside one call; a stage includes the pool that opens it):\n")
    print("| part | ms | GFLOP | TFLOP/s | of peak |")
    print("|---|---|---|---|---|")
    result["parts"] = {}
    for part in PARTS:
        ms, fl = spent[part], 2 * 2 * pairs * macs.get(part, 0)
        result["parts"][part] = {"ms": ms, "tflops": fl / ms / 1e9}
        rate = f"{fl / ms / 1e9:.1f} | {100 * fl / ms / 1e9 / PEAK_TFLOPS:.0f} %" if fl else "- | -"
        print(f"| {part} | {ms:.3f} | {fl / 1e9:.1f} | {rate} |")
    print("\n" + json.dumps(result))


if __name__ == "__main__":
    main()
