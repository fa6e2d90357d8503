"""Times LPIPS (VGG16) on device-resident clips with seeded weights: python tools/lpips_time.py [--frames 32 --size 512]

Device events around the call, one warm-up, the median of 5 with min and max; per-stage time of the five trunk stages and the
head from events inside the call; a sweep of max_scratch_bytes.  The trunk costs 305 856 multiply-adds per input pixel, which is
set against the fp32 matrix peak (157.3 TFLOP/s) and against the 122 TFLOP/s of an untuned fp32 MFMA GEMM.  --yardstick adds
torch.nn.functional.conv2d on the same layers (skipped if it raises).  Prints a markdown table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from motion324_amd import perceptual as P  # noqa: E402

PEAK_TFLOPS = 157.3
UNTUNED_GEMM_TFLOPS = 122.0
REPEATS = 5


def stage_macs_per_pixel():
    """multiply-adds per INPUT pixel of each stage (stage s works at 1 / 4^s of the pixels)"""
    return [9 * sum(cin * cout for cin, cout in stage) / 4 ** s for s, stage in enumerate(P.STAGES)]


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
    parser.add_argument("--pairs_per_chunk", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    parser.add_argument("--yardstick", action="store_true")
    args = parser.parse_args(argv)
    T, S = args.frames, args.size
    dev = "cuda"
    metric = P.LPIPS(P.load_lpips_weights(P.synth_lpips_state_dict(0)), dev)
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    b = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    per_pair = P.BYTES_PER_PAIR_PIXEL * S * S
    macs = stage_macs_per_pixel()
    flop_clip = 2 * 2 * T * S * S * sum(macs)                   # two clips, two flops per multiply-add
    result = {"frames": T, "size": S, "tflop_per_clip_pair": flop_clip / 1e12, "floor_ms_at_peak": flop_clip / PEAK_TFLOPS / 1e9, "sweep": []}

    print(f"LPIPS, {T} frame pairs of {S} x {S}: {flop_clip / 1e12:.2f} TFLOP, floor {result['floor_ms_at_peak']:.1f} ms at {PEAK_TFLOPS} TFLOP/s\n")
    print("| pairs per chunk | max_scratch_bytes | median ms | min | max | TFLOP/s | of peak | of the untuned GEMM |")
    print("|---|---|---|---|---|---|---|---|")
    for n in args.pairs_per_chunk:
        if n > T:
            continue
        budget = n * per_pair
        med, lo, hi = timed(lambda: metric(a, b, max_scratch_bytes=budget))
        tf = flop_clip / med / 1e9
        result["sweep"].append({"pairs": n, "bytes": budget, "ms": med, "min": lo, "max": hi, "tflops": tf})
        print(f"| {n} | {budget} | {med:.1f} | {lo:.1f} | {hi:.1f} | {tf:.1f} | {100 * tf / PEAK_TFLOPS:.0f} % | {100 * tf / UNTUNED_GEMM_TFLOPS:.0f} % |")

    best = min(result["sweep"], key=lambda r: r["ms"])
    events = []
    metric(a, b, max_scratch_bytes=best["bytes"], stage_events=events)
    torch.cuda.synchronize()
    spent = {}
    for label, start, end in events:
        spent[label] = spent.get(label, 0.0) + start.elapsed_time(end)
    print(f"\nper stage at {best['pairs']} pairs per chunk (events inside one call; stage 1 includes the input scaling, stages 2-5 their pool):\n")
    print("| part | ms | TFLOP | TFLOP/s | of peak |")
    print("|---|---|---|---|---|")
    result["stages"] = {}
    for s in range(5):
        ms, fl = spent[f"stage{s + 1}"], 2 * 2 * T * S * S * macs[s]
        result["stages"][f"stage{s + 1}"] = {"ms": ms, "tflops": fl / ms / 1e9}
        print(f"| stage {s + 1} | {ms:.2f} | {fl / 1e12:.2f} | {fl / ms / 1e9:.1f} | {100 * fl / ms / 1e9 / PEAK_TFLOPS:.0f} % |")
    result["stages"]["head"] = {"ms": spent["head"]}
    print(f"| head (5 layers) | {spent['head']:.2f} | - | - | - |")

    if args.yardstick:
        try:
            import torch.nn.functional as F
            n = min(T, 4)
            print(f"\ntorch.nn.functional.conv2d, fp32 NCHW, {2 * n} images, the same layers:\n\n| stage | ms | TFLOP/s |\n|---|---|---|")
            h = S
            for s, stage in enumerate(P.STAGES):
                ws = [torch.randn((cout, cin, 3, 3), device=dev) * 0.05 for cin, cout in stage]

                def run():
                    x = torch.randn((2 * n, stage[0][0], h, h), device=dev)
                    for w in ws:
                        x = F.relu(F.conv2d(x, w, padding=1))
                med, _, _ = timed(run)
                fl = 2 * 2 * n * S * S * macs[s]
                print(f"| stage {s + 1} | {med:.2f} | {fl / med / 1e9:.1f} |")
                h //= 2
        except Exception as exc:  # the yardstick is optional
            print(f"conv2d yardstick skipped: {type(exc).__name__}: {exc}")
    print("\n" + json.dumps(result))


if __name__ == "__main__":
    main()
