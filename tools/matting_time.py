"""Times U2-Net matting on device-resident clips with seeded weights: python tools/matting_time.py [--variants u2net u2netp]

Device events around the call, one warm-up, the median of 5 (3 for the 256-frame clips) with min and max.  Per clip shape the whole
matte_video (resize, normalise, network, quantise, resize back) and the share of the network; per stage the time from events inside
the call, its multiply-adds from the layer table, and the tiles its layers took; a sweep of the frames per chunk.  Set against the
fp32 matrix peak (157.3 TFLOP/s).  Prints markdown tables and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from motion324_amd import matting as M  # noqa: E402
from motion324_amd import ops  # noqa: E402

PEAK_TFLOPS = 157.3
CLIPS = ((32, 1080, 1920), (256, 1080, 1920), (32, 512, 512), (256, 512, 512))


def half(n):
    return (n + 1) // 2


def stage_layout(variant, size, frames):
    """{stage: (multiply-adds per frame, {tile width: layers})} of a U2-Net variant at input size `size`"""
    return table_layout(M.VARIANTS[variant], size, frames)


def table_layout(stages, size, frames):
    """{stage: (multiply-adds per frame, {tile width: layers})} from a stage table whose stage1 works at `size`: stage k works at
    size / 2^(k-1) (rounded up), a block's layers at its own pyramid of resolutions"""
    out, side = {}, size
    sizes = {}
    for k in range(1, 7):
        sizes[f"stage{k}"] = side
        if k < 6:
            sizes[f"stage{k}d"] = side
        side = half(side)
    for stage, spec in stages.items():
        kind, r = spec[0], sizes[stage]
        macs, tiles = 0, {}
        for name, cin, cout, _ in M.stage_layers(*spec):
            res = r
            if kind != "4F":
                L = int(kind)
                digits = "".join(c for c in name if c.isdigit())
                k = int(digits) if digits else 1
                k = min(k, L - 1)                               # rebnconv<L> runs at the resolution of rebnconv<L-1>
                for _ in range(k - 1):
                    res = half(res)
            macs += 9 * cin * cout * res * res
            t = ops.conv3x3_ex_tile(frames, res, res, cout)
            tiles[t] = tiles.get(t, 0) + 1
        out[stage] = (macs, tiles)
    return out


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times), min(times), max(times)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--variants", nargs="+", default=["u2net", "u2netp"])
    parser.add_argument("--size", type=int, default=M.SIZE)
    parser.add_argument("--frames_per_chunk", type=int, nargs="+", default=[1, 2, 4, 8, 16, 20, 32])
    args = parser.parse_args(argv)
    dev, S = "cuda", args.size
    per_frame = 4 * M.FLOATS_PER_FRAME_PIXEL * S * S
    result = {"size": S, "variants": {}}
    g = torch.Generator().manual_seed(1)
    for variant in args.variants:
        net = M.U2Net(M.load_u2net_weights(M.synth_u2net_state_dict(variant, 0)), dev)
        n_default = M.frames_per_chunk(256, S, M.DEFAULT_MAX_SCRATCH_BYTES)
        macs_frame = sum(m for m, _ in stage_layout(variant, S, 1).values())
        res = result["variants"][variant] = {"gmac_per_frame": macs_frame / 1e9, "floor_ms_per_frame": 2 * macs_frame / PEAK_TFLOPS / 1e9, "clips": [],
                                             "sweep": [], "stages": {}}
        print(f"\n## {variant}: {macs_frame / 1e9:.2f} G multiply-adds per {S} x {S} frame, floor {res['floor_ms_per_frame']:.3f} ms per frame at "
              f"{PEAK_TFLOPS} TFLOP/s\n")
        print("| frames | H x W | matte_video ms (median) | min | max | ms per frame | network alone ms | network TFLOP/s | of peak |")
        print("|---|---|---|---|---|---|---|---|---|")
        for T, H, W in CLIPS:
            video = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            repeats = 5 if T <= 32 else 3
            med, lo, hi = timed(lambda: M.matte_video(video, net, size=S), repeats)
            x = ops.matte_prepare(M._resize(video[:min(T, n_default)], 3, W, H, S, S))
            net_med, _, _ = timed(lambda: net(x), repeats)
            net_ms = net_med * T / x.shape[0]
            tf = 2 * macs_frame * T / net_ms / 1e9
            res["clips"].append({"frames": T, "H": H, "W": W, "ms": med, "min": lo, "max": hi, "network_ms": net_ms, "network_tflops": tf})
            print(f"| {T} | {H} x {W} | {med:.1f} | {lo:.1f} | {hi:.1f} | {med / T:.2f} | {net_ms:.1f} | {tf:.1f} | {100 * tf / PEAK_TFLOPS:.0f} % |")
            del video, x

        T = 32
        video = torch.randint(0, 256, (T, 512, 512, 3), generator=g, dtype=torch.uint8).to(dev)
        print(f"\nframes per chunk, {T} frames of 512 x 512 (peak: what the call allocated at its highest, activations and results):\n\n"
              "| frames per chunk | max_scratch_bytes | median ms | min | max | peak bytes |\n|---|---|---|---|---|---|")
        for n in args.frames_per_chunk:
            if n > T:
                continue
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            med, lo, hi = timed(lambda: M.matte_video(video, net, size=S, max_scratch_bytes=n * per_frame), 5)
            peak = torch.cuda.max_memory_allocated() - before
            res["sweep"].append({"frames": n, "bytes": n * per_frame, "ms": med, "min": lo, "max": hi, "peak_bytes": peak})
            print(f"| {n} | {n * per_frame} | {med:.1f} | {lo:.1f} | {hi:.1f} | {peak} |")

        n = min(T, n_default)
        layout = stage_layout(variant, S, n)                    # the tiles of the chunk that is timed
        events = []
        M.matte_video(video[:n], net, size=S, stage_events=events)
        torch.cuda.synchronize()
        spent = {}
        for label, start, end in events:
            spent[label] = spent.get(label, 0.0) + start.elapsed_time(end)
        print(f"\nper stage, {n} frames in one chunk (events inside one call; a stage's pools and upsamples are inside, the pool or upsample "
              f"in front of it is not):\n\n| stage | block (in, mid, out) | ms | G multiply-adds per frame | TFLOP/s | of peak | tiles (width: layers) |")
        print("|---|---|---|---|---|---|---|")
        for stage, (macs, tiles) in layout.items():
            ms = spent[stage]
            tf = 2 * macs * n / ms / 1e9
            kind, cin, mid, cout = M.VARIANTS[variant][stage]
            res["stages"][stage] = {"ms": ms, "gmac_per_frame": macs / 1e9, "tflops": tf, "tiles": tiles}
            print(f"| {stage} | RSU-{kind} ({cin}, {mid}, {cout}) | {ms:.2f} | {macs / 1e9:.2f} | {tf:.1f} | {100 * tf / PEAK_TFLOPS:.0f} % | "
                  + ", ".join(f"{t}: {c}" for t, c in sorted(tiles.items())) + " |")
        del video
    print("\n" + json.dumps(result))


if __name__ == "__main__":
    main()
