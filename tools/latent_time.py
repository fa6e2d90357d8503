#!/usr/bin/env python3
"""The c2 clip cut at the motion latent, as hipGraph replays, five rounds of 20 replays: one line per process (run the modes alternately in
separate processes on one box, next to tools/clip_time.py of this commit and of the parent; profiles/motion_latent.md).
usage: tools/latent_time.py full | encode | decode [N points, default 2048]"""
import os, sys, torch
sys.path.insert(0, os.getcwd())
import bench
import motion324_amd as m
from motion324_amd import synth
mode = sys.argv[1] if len(sys.argv) > 1 else "full"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
dev = torch.device("cuda")
model, _ = bench.build_model(dev, 32)
m.set_precision("bf16")
s = synth.synth_inputs(1, 32, 2048, 4096, 512, seed=1)
sample = {k: torch.from_numpy(v).to(dev) for k, v in s.items()}
points = ("ref_pcd", "ref_normal", "ref_rgb")
with torch.no_grad():
    if mode == "encode":
        sample = {k: v for k, v in sample.items() if k not in points}
        sample["m324_encode_only"] = True
    elif mode == "decode":
        model.auto_graph = False
        latent = model.encode_motion(sample)
        p = synth.synth_inputs(1, 1, N, 8, 14, seed=2)
        sample = {k: torch.from_numpy(p[k]).to(dev) for k in points}
        sample["m324_latent"] = latent.tokens
    fast = m.GraphedForward(model)
    clip = fast.static_inputs(sample)
    for _ in range(5): fast(clip)
    torch.cuda.synchronize()
    ts = []
    for r in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20): fast(clip)
        e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1) / 20)
print(mode + (f" N={N}" if mode == "decode" else ""), "ms:", " ".join(f"{t:.3f}" for t in ts), flush=True)
