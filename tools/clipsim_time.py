"""Times the CLIP similarity of two device-resident clips under seeded ViT-bigG-14-sized weights:
python tools/clipsim_time.py [--frames 32 --size 512 --layers 48]

Device events around the call, one warm-up, the median of 5 with min and max; the shares of preprocessing, the patch rows and
their GEMM, the token assembly, LayerNorms, the four GEMM roles, attention and the head GEMM from events inside one call; the tower's achieved TFLOP/s against the
fp32 matrix peak (157.3 TFLOP/s); m324_attention_tok alone at B H = 1024, L = 257, D = 104; and, as a yardstick in the same
run, the block's four GEMMs alone at the tower's shapes -- tower / GEMMs-alone is what the new kernels and launches cost on top.
The weights are generated on the device (7.4 GB at 48 layers).  Prints markdown tables and one JSON line.
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
from motion324_amd import lib, ops  # noqa: E402
from motion324_amd.vit import VitBlock, VitWeights  # noqa: E402

PEAK_TFLOPS = 157.3
REPEATS = 5
WIDTH, HEADS, MLP, PATCH, IMAGE, EMBED = 1664, 16, 8192, 14, 224, 1280


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


def device_weights(layers, dev, seed=0):
    """a VitWeights of bigG's sizes made on the device, of synth_clip_state_dict's scales"""
    g = torch.Generator(device=dev).manual_seed(seed)

    def randn(*shape, scale=1.0):
        return torch.randn(shape, generator=g, device=dev) * scale

    def ln():
        return 1.0 + randn(WIDTH, scale=0.1), randn(WIDTH, scale=0.05)

    L = (IMAGE // PATCH) ** 2 + 1
    Kp = (3 * PATCH * PATCH + 31) // 32 * 32
    patch_w = torch.zeros((WIDTH, Kp), device=dev)
    patch_w[:, :3 * PATCH * PATCH] = randn(WIDTH, 3 * PATCH * PATCH, scale=0.1 / math.sqrt(3 * PATCH * PATCH))
    blocks = []
    for _ in range(layers):
        w_in = randn(3 * WIDTH, WIDTH, scale=1.0 / math.sqrt(WIDTH))
        w_in[:2 * WIDTH] *= 2.0
        blocks.append(VitBlock(ln(), (w_in, randn(3 * WIDTH, scale=0.05)),
                               (randn(WIDTH, WIDTH, scale=1.0 / math.sqrt(WIDTH)), randn(WIDTH, scale=0.05)), ln(),
                               (randn(MLP, WIDTH, scale=1.0 / math.sqrt(WIDTH)), randn(MLP, scale=0.05)),
                               (randn(WIDTH, MLP, scale=1.0 / math.sqrt(MLP)), randn(WIDTH, scale=0.05))))
    # keyword arguments are evaluated in the order written: the order of draws is the one this tool has always had
    return VitWeights(width=WIDTH, heads=HEADS, layers=layers, mlp=MLP, patch=PATCH, image=IMAGE, tokens=L, embed=EMBED, patch_w=patch_w,
                      patch_b=None, cls=randn(WIDTH, scale=0.1), pos=randn(L, WIDTH, scale=0.1), ln_pre=ln(), blocks=tuple(blocks),
                      ln_post=ln(), proj_t=randn(EMBED, WIDTH, scale=1.0 / math.sqrt(WIDTH)))


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=32)
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--layers", type=int, default=48)
    args = parser.parse_args(argv)
    T, S, layers = args.frames, args.size, args.layers
    dev = "cuda"
    name, cus = lib.device_info()
    model = C.ClipVision(device_weights(layers, dev), dev)
    metric = C.ClipSimilarity(model)
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    b = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    n, L, W, D = 2 * T, model.tokens, WIDTH, WIDTH // HEADS
    M = n * L
    gemm_flop = {"gemm_qkv": 2.0 * M * W * 3 * W, "gemm_proj": 2.0 * M * W * W, "gemm_fc1": 2.0 * M * W * MLP, "gemm_fc2": 2.0 * M * MLP * W}
    attn_flop = 4.0 * n * HEADS * L * L * D
    tower_flop = layers * (sum(gemm_flop.values()) + attn_flop) + 2.0 * n * (L - 1) * model.Kp * W + 2.0 * n * W * EMBED
    result = {"device": name, "cus": cus, "frames": T, "size": S, "layers": layers, "images": n, "tower_tflop": tower_flop / 1e12,
              "chunk_images": model.images_per_chunk(n, C.DEFAULT_MAX_SCRATCH_BYTES)}

    med, lo, hi = timed(lambda: metric(a, b))
    result["pair_ms"] = {"median": med, "min": lo, "max": hi}
    print(f"{name} ({cus} CUs): CLIP similarity of {T} frame pairs of {S} x {S}, ViT-bigG-14 sizes with {layers} layers, {n} images in chunks of "
          f"{result['chunk_images']}: {tower_flop / 1e12:.1f} TFLOP\n")
    print("| ms per clip pair (median of 5) | min | max | tower TFLOP/s | of the fp32 matrix peak |\n|---|---|---|---|---|")
    print(f"| {med:.1f} | {lo:.1f} | {hi:.1f} | {tower_flop / med / 1e9:.1f} | {100 * tower_flop / med / 1e9 / PEAK_TFLOPS:.0f} % |")

    events = []
    metric(a, b, stage_events=events)
    torch.cuda.synchronize()
    spent = {}
    for label, start, end in events:
        spent[label] = spent.get(label, 0.0) + start.elapsed_time(end)
    total = sum(spent.values())
    result["stages_ms"] = spent
    print("\nshares (events inside one call, around every launch):\n\n| part | ms | share | TFLOP/s |\n|---|---|---|---|")
    for label in ("preprocess", "patch_rows", "gemm_patch", "tokens", "layernorm", "gemm_qkv", "attention", "gemm_proj", "gemm_fc1", "gemm_fc2", "gemm_head"):
        fl = layers * gemm_flop[label] if label in gemm_flop else (layers * attn_flop if label == "attention" else 0.0)
        rate = f"{fl / spent[label] / 1e9:.1f}" if fl else "-"
        print(f"| {label} | {spent[label]:.2f} | {100 * spent[label] / total:.1f} % | {rate} |")

    # the block's four GEMMs alone, at the chunk's row count, layers times each
    rows = result["chunk_images"] * L
    blk = model.blocks[0]
    y = torch.randn((rows, W), device=dev)
    hid = torch.randn((rows, MLP), device=dev)
    x = torch.randn((rows, W), device=dev)
    qkv = torch.empty((rows, 3 * W), device=dev)
    hw = torch.empty((rows, MLP), device=dev)

    def four_gemms():
        ops.gemm(y, blk.in_proj[0], qkv, bias=blk.in_proj[1])
        ops.gemm(y, blk.out_proj[0], x, bias=blk.out_proj[1], residual=x)
        ops.gemm(y, blk.c_fc[0], hw, bias=blk.c_fc[1], act=lib.ACT_GELU)
        ops.gemm(hid, blk.c_proj[0], x, bias=blk.c_proj[1], residual=x)

    gm, glo, ghi = timed(four_gemms)
    chunks = math.ceil(n / result["chunk_images"])
    alone = gm * layers * chunks
    block_flop = sum(gemm_flop.values()) * rows / M
    result["gemms_alone_ms"] = {"per_block": gm, "min": glo, "max": ghi, "tower_equivalent": alone, "tflops": block_flop / gm / 1e9}
    result["tower_over_gemms"] = med / alone
    print(f"\nthe block's four GEMMs alone at {rows} rows: {gm:.2f} ms per block (min {glo:.2f}, max {ghi:.2f}), {block_flop / gm / 1e9:.1f} TFLOP/s; "
          f"x {layers} layers x {chunks} chunk(s) = {alone:.1f} ms; clip pair / GEMMs alone = {med / alone:.3f}")

    B = 1024 // HEADS
    q = torch.randn((B * L, 3 * W), device=dev)
    o = torch.empty((B * L, W), device=dev)
    am, alo, ahi = timed(lambda: ops.attention_tok(q, B, L, HEADS, D, out=o))
    fl = 4.0 * B * HEADS * L * L * D
    result["attention_tok"] = {"ms": am, "min": alo, "max": ahi, "tflops": fl / am / 1e9}
    print(f"\nm324_attention_tok alone, B H = {B * HEADS}, L = {L}, D = {D}: {am:.3f} ms (min {alo:.3f}, max {ahi:.3f}), {fl / am / 1e9:.1f} TFLOP/s, "
          f"{100 * fl / am / 1e9 / PEAK_TFLOPS:.0f} % of the peak; attention is {100 * spent['attention'] / total:.1f} % of the tower")
    print("\n" + json.dumps(result))


if __name__ == "__main__":
    main()
