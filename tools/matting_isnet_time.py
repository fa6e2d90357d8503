"""Times ISNet matting next to U2-Net on one device-resident window with seeded weights: python tools/matting_isnet_time.py

A window of --frames frames of --height x --width, through matte_video with ISNet at 1024 and with u2net at 320, in one run on one
box.  Per network: the whole call (device events, one warm-up, the median of 5 with min and max), the time per stage from events
inside one call summed over the chunks, the multiply-adds from the layer table, the share of the fp32 matrix peak (157.3 TFLOP/s),
the tiles the stage's layers took, and what the call allocated at its highest against the estimate frames_per_chunk works with.
Prints markdown tables and one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import matting_time as MT  # noqa: E402
from motion324_amd import matting as M  # noqa: E402
from motion324_amd import ops  # noqa: E402


def network(model):
    """(net, stage table, side of stage1's maps as a function of the input size)"""
    if model == "isnet":
        net = M.ISNet(M.load_isnet_weights(M.synth_isnet_state_dict(0)), "cuda")
        return net, M.ISNET_STAGES, lambda s: (s - 1) // 2 + 1
    net = M.U2Net(M.load_u2net_weights(M.synth_u2net_state_dict(model, 0)), "cuda")
    return net, M.VARIANTS[model], lambda s: s


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--models", nargs="+", default=["isnet", "u2net"])
    parser.add_argument("--frames", type=int, default=32)
    parser.add_argument("--height", type=int, default=1080)
    parser.add_argument("--width", type=int, default=1920)
    args = parser.parse_args(argv)
    T, H, W = args.frames, args.height, args.width
    g = torch.Generator().manual_seed(1)
    video = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8).to("cuda")
    result = {"device": torch.cuda.get_device_name(0), "frames": T, "H": H, "W": W, "models": {}}
    print(f"device: {result['device']}; window: {T} frames of {W} x {H}\n")
    for model in args.models:
        net, stages, stage1_side = network(model)
        S = net.input_size
        n = M.frames_per_chunk(T, S, M.DEFAULT_MAX_SCRATCH_BYTES, net.floats_per_frame_pixel)
        side = stage1_side(S)
        layout = MT.table_layout(stages, side, n)
        stem_macs = 9 * M.ISNET_STEM[0] * M.ISNET_STEM[1] * side * side if model == "isnet" else 0
        macs_frame = stem_macs + sum(m for m, _ in layout.values())
        estimate = n * 4 * net.floats_per_frame_pixel * S * S

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        med, lo, hi = MT.timed(lambda: M.matte_video(video, net), 5)
        peak = torch.cuda.max_memory_allocated() - before
        results_bytes = T * (H * W + S * S)                     # alpha and the size x size mask, which the peak includes

        events = []
        M.matte_video(video, net, stage_events=events)
        torch.cuda.synchronize()
        spent = {}
        for label, start, end in events:
            spent[label] = spent.get(label, 0.0) + start.elapsed_time(end)
        net_ms = sum(spent.values())
        tf = 2 * macs_frame * T / net_ms / 1e9
        res = result["models"][model] = {"size": S, "frames_per_chunk": n, "gmac_per_frame": macs_frame / 1e9, "ms": med, "min": lo, "max": hi,
                                         "stages_ms": net_ms, "stages_tflops": tf, "peak_bytes": peak, "estimate_bytes": estimate,
                                         "results_bytes": results_bytes, "stages": {}}
        print(f"## {model} at {S}: {macs_frame / 1e9:.2f} G multiply-adds per frame, {n} frames per chunk\n")
        print(f"matte_video: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f}), {med / T:.2f} ms per frame; the stages alone {net_ms:.1f} ms, "
              f"{tf:.1f} TFLOP/s, {100 * tf / MT.PEAK_TFLOPS:.0f} % of {MT.PEAK_TFLOPS}\n")
        print(f"peak allocation of the call {peak} bytes ({peak / 2 ** 30:.2f} GiB), of which {results_bytes} are its results; the estimate for a chunk of "
              f"{n} frames is {estimate} bytes ({estimate / 2 ** 30:.2f} GiB): peak / estimate {peak / estimate:.2f}, "
              f"{(peak - results_bytes) / (n * S * S * 4):.0f} floats per frame pixel against {net.floats_per_frame_pixel}\n")
        print("| stage | block (in, mid, out) | ms | G multiply-adds per frame | TFLOP/s | of peak | tiles (width: layers) |\n|---|---|---|---|---|---|---|")
        rows = [("conv_in", f"stride 2 {M.ISNET_STEM}", stem_macs, {ops.conv3x3_ex_tile(n, side, side, M.ISNET_STEM[1]): 1})] if model == "isnet" else []
        rows += [(stage, f"RSU-{stages[stage][0]} {stages[stage][1:]}", macs, tiles) for stage, (macs, tiles) in layout.items()]
        for stage, block, macs, tiles in rows:
            ms = spent[stage]
            stf = 2 * macs * T / ms / 1e9
            res["stages"][stage] = {"ms": ms, "gmac_per_frame": macs / 1e9, "tflops": stf, "tiles": tiles}
            print(f"| {stage} | {block} | {ms:.2f} | {macs / 1e9:.2f} | {stf:.1f} | {100 * stf / MT.PEAK_TFLOPS:.0f} % | "
                  + ", ".join(f"{t}: {c}" for t, c in sorted(tiles.items())) + " |")
        print()
        del net
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
