"""Times DreamSim of two device-resident clips under three seeded ViT-B/16 towers (DINO layout; open_clip layout with QuickGELU;
open_clip layout with GELU):  python tools/dreamsim_time.py [--frames 32 --size 512]

Device events around the call, one warm-up, the median of 5 with min and max; the shares of the resize, the patch rows, the
GEMM roles, attention and the LayerNorms from events inside one call; the towers' achieved TFLOP/s against the fp32 matrix peak
(157.3 TFLOP/s); and, as a yardstick in the same run, the block's four GEMMs alone at the towers' shapes -- towers / GEMMs-alone
is what the other kernels and launches cost on top.  Prints markdown tables and one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from motion324_amd import clipsim as C  # noqa: E402
from motion324_amd import dreamsim as D  # noqa: E402
from motion324_amd import lib, ops  # noqa: E402

PEAK_TFLOPS = 157.3
REPEATS = 5
WIDTH, HEADS, LAYERS, MLP, PATCH, IMAGE, EMBED = 768, 12, 12, 3072, 16, 224, 512


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


def towers(dev):
    dino = D.load_vit_weights(D.synth_dino_state_dict(1, WIDTH, LAYERS, HEADS, MLP, PATCH, IMAGE))
    clip = D.load_vit_weights(C.synth_clip_state_dict(2, WIDTH, LAYERS, HEADS, MLP, PATCH, IMAGE, EMBED))
    oclip = D.load_vit_weights(C.synth_clip_state_dict(3, WIDTH, LAYERS, HEADS, MLP, PATCH, IMAGE, EMBED))
    return (D.VitTower(dino, dev, "gelu", D.DINO_LN_EPS, D.IMAGENET_MEAN, D.IMAGENET_STD, "cls"),
            D.VitTower(clip, dev, "quick_gelu", D.CLIP_LN_EPS, C.OPENAI_MEAN, C.OPENAI_STD, "embedding"),
            D.VitTower(oclip, dev, "gelu", D.CLIP_LN_EPS, C.OPENAI_MEAN, C.OPENAI_STD, "embedding"))


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=32)
    parser.add_argument("--size", type=int, default=512)
    args = parser.parse_args(argv)
    T, S = args.frames, args.size
    dev = "cuda"
    name, cus = lib.device_info()
    tw = towers(dev)
    metric = D.DreamSim(tw)
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    b = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    n, L, W = 2 * T, tw[0].tokens, WIDTH
    M = n * L
    gemm_flop = {"gemm_qkv": 2.0 * M * W * 3 * W, "gemm_proj": 2.0 * M * W * W, "gemm_fc1": 2.0 * M * W * MLP, "gemm_fc2": 2.0 * M * MLP * W}
    attn_flop = 4.0 * n * HEADS * L * L * (W // HEADS)
    patch_flop = 2.0 * n * (L - 1) * tw[0].Kp * W
    tower_flop = LAYERS * (sum(gemm_flop.values()) + attn_flop) + patch_flop
    total_flop = 3 * tower_flop
    result = {"device": name, "cus": cus, "frames": T, "size": S, "images": n, "towers": 3, "total_tflop": total_flop / 1e12,
              "chunk_images": tw[0].images_per_chunk(n, D.DEFAULT_MAX_SCRATCH_BYTES)}

    med, lo, hi = timed(lambda: metric(a, b))
    result["pair_ms"] = {"median": med, "min": lo, "max": hi}
    print(f"{name} ({cus} CUs): DreamSim of {T} frame pairs of {S} x {S}, three ViT-B/16 towers, {n} images in chunks of "
          f"{result['chunk_images']}: {total_flop / 1e12:.2f} TFLOP\n")
    print("| ms per clip pair (median of 5) | min | max | TFLOP/s | of the fp32 matrix peak |\n|---|---|---|---|---|")
    print(f"| {med:.1f} | {lo:.1f} | {hi:.1f} | {total_flop / med / 1e9:.1f} | {100 * total_flop / med / 1e9 / PEAK_TFLOPS:.0f} % |")

    rm, rlo, rhi = timed(lambda: D.resize(torch.cat([a, b]), IMAGE))
    result["resize_ms"] = {"median": rm, "min": rlo, "max": rhi}
    img = D.resize(torch.cat([a, b]), IMAGE)
    tm, tlo, thi = timed(lambda: [t.features(img) for t in tw])
    result["towers_ms"] = {"median": tm, "min": tlo, "max": thi}
    print(f"\nresize of {n} frames {S} -> {IMAGE}: {rm:.3f} ms (min {rlo:.3f}, max {rhi:.3f}); the three towers alone: {tm:.1f} ms "
          f"(min {tlo:.1f}, max {thi:.1f})")

    events = []
    for t in tw:
        t.features(img, stage_events=events)
    torch.cuda.synchronize()
    spent = {}
    for label, start, end in events:
        spent[label] = spent.get(label, 0.0) + start.elapsed_time(end)
    total = sum(spent.values())
    result["stages_ms"] = spent
    print("\nshares (events inside one pass of the three towers, around every launch):\n\n| part | ms | share | TFLOP/s |\n|---|---|---|---|")
    for label in ("patch_rows", "gemm_patch", "tokens", "layernorm", "gemm_qkv", "attention", "gemm_proj", "gemm_fc1", "gemm_fc2", "gemm_head"):
        fl = 3 * LAYERS * gemm_flop[label] if label in gemm_flop else (3 * LAYERS * attn_flop if label == "attention" else
                                                                      3 * patch_flop if label == "gemm_patch" else 0.0)
        rate = f"{fl / spent[label] / 1e9:.1f}" if fl else "-"
        print(f"| {label} | {spent[label]:.2f} | {100 * spent[label] / total:.1f} % | {rate} |")

    # the block's four GEMMs alone at the chunk's row count: twice with GELU (two towers), once with QuickGELU
    rows = result["chunk_images"] * L
    blk = tw[0].blocks[0]
    Wp, Mp = tw[0].Wp, tw[0].Mp
    y, hid, x = torch.randn((rows, Wp), device=dev), torch.randn((rows, Mp), device=dev), torch.randn((rows, W), device=dev)
    qkv, hw = torch.empty((rows, 3 * W), device=dev), torch.empty((rows, MLP), device=dev)

    def four_gemms(act):
        ops.gemm(y, blk.in_proj[0], qkv, bias=blk.in_proj[1])
        ops.gemm(y, blk.out_proj[0], x, bias=blk.out_proj[1], residual=x)
        ops.gemm(y, blk.c_fc[0], hw, bias=blk.c_fc[1], act=act)
        ops.gemm(hid, blk.c_proj[0], x, bias=blk.c_proj[1], residual=x)

    gm, glo, ghi = timed(lambda: four_gemms(lib.ACT_GELU))
    qm, qlo, qhi = timed(lambda: four_gemms(lib.ACT_QUICK_GELU))
    chunks = math.ceil(n / result["chunk_images"])
    alone = (2 * gm + qm) * LAYERS * chunks
    block_flop = sum(gemm_flop.values()) * rows / M
    result["gemms_alone_ms"] = {"per_block_gelu": gm, "per_block_quick_gelu": qm, "min": min(glo, qlo), "max": max(ghi, qhi),
                                "towers_equivalent": alone, "tflops": block_flop / gm / 1e9}
    result["towers_over_gemms"] = tm / alone
    print(f"\nthe block's four GEMMs alone at {rows} rows: {gm:.3f} ms per block with GELU (min {glo:.3f}, max {ghi:.3f}), {qm:.3f} ms with "
          f"QuickGELU (min {qlo:.3f}, max {qhi:.3f}), {block_flop / gm / 1e9:.1f} TFLOP/s; x {LAYERS} layers x 3 towers x {chunks} chunk(s) = "
          f"{alone:.1f} ms; towers / GEMMs alone = {tm / alone:.3f}")
    print("\n" + json.dumps(result))


if __name__ == "__main__":
    main()
