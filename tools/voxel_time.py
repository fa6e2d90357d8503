#!/usr/bin/env python3
"""Timing of the volumetric IoU (motion324_amd.evaluation.compute_iou_voxel, csrc/voxel.hip); the numbers live in
profiles/voxel_iou.md.

Two synthetic clips from a seed: an icosphere subdivided six times (40962 vertices, 81920 faces) of radius about 0.8, deformed per
frame by a travelling wave and a seeded per-vertex wobble; the second clip is the first one slightly scaled, shifted and wobbled
differently (a "prediction").  32 frames each, resolution 128, half 2: a grid of 512^3 voxels, 16 MiB per frame.

Reported, per stage and for both clips together: device events around back-to-back calls -- as many as fill about 0.2 s, after a
warm-up call -- divided by the number of calls, median of `--rounds` such windows with (min .. max):
  * zero + mark (ops.voxelize), for big_voxels in {16, 64, 256, 1024}, after the grids of all four (and of 0 and 2^31 - 1 on the
    first four frames) were compared bit for bit;
  * fill (ops.voxel_fill into a second grid);
  * counts (ops.voxel_counts), with the bytes it must read -- two grids of G^3 / 8 bytes per frame -- over its time, beside a
    device-to-device copy that moves the same number of bytes (half read, half written), timed in the same process;
and the host clock around compute_iou_voxel on the device-resident clips, ending in a synchronise.

    python tools/voxel_time.py [--frames 32] [--resolution 128] [--level 6] [--rounds 5] [--out FILE.md]

A run without a HIP device fails: there is no CPU timing of the GPU path."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

BIG = (16, 64, 256, 1024)
WINDOW_S = 0.2


def icosphere(level):
    """(vertices fp64 [V,3] on the unit sphere, faces int32 [F,3]), F = 20 * 4^level"""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [np.array(q, dtype=np.float64) / math.sqrt(1.0 + p * p) for q in ((-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p),
                                                                          (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1))]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            key = (a, b) if a < b else (b, a)
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, dtype=np.int32)


def clip_of(base, frames, seed, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """fp32 [T,V,3]: radius 0.8, a wave that travels with the frame, a seeded wobble of 0.002, then scale and shift"""
    rng = np.random.default_rng(seed)
    out = np.empty((frames,) + base.shape, dtype=np.float32)
    for t in range(frames):
        r = 0.8 * (1.0 + 0.10 * np.sin(3.0 * base[:, :1] + 0.3 * t) * np.cos(2.0 * base[:, 1:2] - 0.2 * t))
        out[t] = scale * (base * r * np.array([1.0, 0.85, 0.7])) + np.asarray(shift) + 0.002 * rng.standard_normal(base.shape)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--half", type=int, default=2)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from motion324_amd import evaluation as ev, ops
    if not torch.cuda.is_available():
        sys.exit("voxel_time: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    T, R, H = args.frames, args.resolution, args.half
    G = ops.voxel_side(R, H)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def events(fn):
        """(median, min, max) ms per call: device events around `calls` back-to-back calls filling about WINDOW_S, after a warm-up"""
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        calls = max(1, min(1000, int(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))
        ms = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / calls)
        return statistics.median(ms), min(ms), max(ms), calls

    base, faces_np = icosphere(args.level)
    faces = torch.from_numpy(faces_np).to(dev)
    clips = [torch.from_numpy(clip_of(base, T, 1)).to(dev), torch.from_numpy(clip_of(base, T, 2, scale=1.03, shift=(0.02, -0.01, 0.015))).to(dev)]
    nv, nf = base.shape[0], faces_np.shape[0]
    frame_bytes = G ** 3 // 8
    emit(dict(what="setup", frames=T, vertices=nv, faces=nf, resolution=R, half=H, side=G, grid_bytes_per_clip=T * frame_bytes))

    # results before speed: the grid must not depend on big_voxels
    first = [ops.voxelize(c, faces, R, H, big_voxels=BIG[0])[0] for c in clips]
    same = all(torch.equal(first[s], ops.voxelize(clips[s], faces, R, H, big_voxels=bv)[0]) for s in range(2) for bv in BIG[1:])
    few = min(T, 4)
    same = same and all(torch.equal(first[0][:few], ops.voxelize(clips[0][:few], faces, R, H, big_voxels=bv)[0]) for bv in (0, 2 ** 31 - 1))
    outside = [int(ops.voxelize(c, faces, R, H)[1].sum()) for c in clips]
    counts = ops.voxel_counts(first[0], first[1]).cpu().numpy()
    emit(dict(what="check", identical_for_every_big_voxels=bool(same), outside=outside, surface_voxels_per_frame=[float(counts[:, 0].mean()), float(counts[:, 1].mean())]))
    if not same:
        sys.exit("voxel_time: the grid depends on big_voxels; no time is reported")

    scratch = torch.empty((ops.voxel_plan(nv, nf, T, R, H),), dtype=torch.uint8, device=dev)
    for bv in BIG:
        ms = events(lambda: [ops.voxelize(clips[s], faces, R, H, big_voxels=bv, scratch=scratch, out=first[s], faces_checked=True) for s in range(2)])
        emit(dict(what="mark", big_voxels=bv, events_ms=ms[:3], calls_per_window=ms[3], us_per_frame_and_side=ms[0] * 1e3 / (2 * T)))
    zero = events(lambda: [first[s].zero_() for s in range(2)])
    emit(dict(what="zero_only", events_ms=zero[:3], calls_per_window=zero[3]))

    filled = [torch.empty_like(g) for g in first]
    ms = events(lambda: [ops.voxel_fill(first[s], out=filled[s]) for s in range(2)])
    emit(dict(what="fill", events_ms=ms[:3], calls_per_window=ms[3], us_per_frame_and_side=ms[0] * 1e3 / (2 * T)))

    read_bytes = 2 * T * frame_bytes
    ms = events(lambda: ops.voxel_counts(first[0], first[1]))
    cp = events(lambda: filled[0].copy_(first[0]))                      # moves the same bytes: one clip's grids read, as many written
    emit(dict(what="counts", events_ms=ms[:3], calls_per_window=ms[3], bytes_read=read_bytes, bytes_per_s=read_bytes / (ms[0] * 1e-3),
              copy_events_ms=cp[:3], copy_calls_per_window=cp[3], copy_bytes_moved=read_bytes, copy_bytes_per_s=read_bytes / (cp[0] * 1e-3),
              share_of_copy_rate=cp[0] / ms[0]))

    shell = ev.compute_iou_voxel(clips[0], faces, clips[1], faces, resolution=R, half=H, max_scratch_bytes=4 << 30)
    solid = ev.compute_iou_voxel(clips[0], faces, clips[1], faces, resolution=R, half=H, fill="orthographic", max_scratch_bytes=4 << 30)
    for fill in ("none", "orthographic"):
        wall = []
        for _ in range(args.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.compute_iou_voxel(clips[0], faces, clips[1], faces, resolution=R, half=H, fill=fill, max_scratch_bytes=4 << 30)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        wall = wall[1:]
        emit(dict(what="compute_iou_voxel", fill=fill, wall_ms=(statistics.median(wall), min(wall), max(wall)), ms_per_frame=statistics.median(wall) / T,
                  iou_mean=float((shell if fill == "none" else solid).mean())))

    if args.out:
        prop = torch.cuda.get_device_properties(0)
        arch = getattr(prop, "gcnArchName", "").split(":")[0]
        fmt = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"       # noqa: E731
        get = lambda what: [r for r in records if r["what"] == what]    # noqa: E731
        chk, cnt, fl, zr = get("check")[0], get("counts")[0], get("fill")[0], get("zero_only")[0]
        lines = ["# Volumetric IoU: what was measured", "",
                 f"`tools/voxel_time.py` on one GPU ({prop.name}, {arch}, {prop.multi_processor_count} CUs), one process, one run.  Two device-resident clips of "
                 f"{T} frames, {nv} vertices and {nf} faces (an icosphere of radius about 0.8, deformed per frame), resolution {R}, half {H}: a grid of {G}^3 "
                 f"voxels, {frame_bytes / 2 ** 20:.0f} MiB per frame, {T * frame_bytes / 2 ** 20:.0f} MiB per clip.  About {chk['surface_voxels_per_frame'][0]:.0f} surface "
                 f"voxels per frame; {sum(chk['outside'])} vertices outside the grid.  Device events around back-to-back calls filling about {WINDOW_S} s, "
                 f"after a warm-up, divided by the calls; median of {args.rounds} windows with (min .. max).  All stage times are for BOTH clips ({2 * T} "
                 "frames).  Before timing, the grids for big_voxels in {16, 64, 256, 1024} (and 0 and 2^31 - 1 on four frames) were compared: bit-identical.", "",
                 "| stage | ms for both clips | us per frame and side | calls per window |", "|---|---|---|---|"]
        for r in get("mark"):
            lines.append(f"| zero + mark, big_voxels = {r['big_voxels']} | {fmt(r['events_ms'])} | {r['us_per_frame_and_side']:.1f} | {r['calls_per_window']} |")
        lines += [f"| zeroing alone (torch) | {fmt(zr['events_ms'])} | {zr['events_ms'][0] * 1e3 / (2 * T):.1f} | {zr['calls_per_window']} |",
                  f"| fill | {fmt(fl['events_ms'])} | {fl['us_per_frame_and_side']:.1f} | {fl['calls_per_window']} |",
                  f"| counts | {fmt(cnt['events_ms'])} | {cnt['events_ms'][0] * 1e3 / (2 * T):.1f} | {cnt['calls_per_window']} |", "",
                  f"Counts: it must read {cnt['bytes_read'] / 2 ** 20:.0f} MiB (two grids per frame) and does so at {cnt['bytes_per_s'] / 1e12:.2f} TB/s.  A "
                  f"device-to-device copy that moves the same number of bytes ({cnt['copy_bytes_moved'] / 2 ** 21:.0f} MiB read, as many written) takes "
                  f"{fmt(cnt['copy_events_ms'])} ms in the same process: {cnt['copy_bytes_per_s'] / 1e12:.2f} TB/s.  The counts kernel runs at "
                  f"{100 * cnt['share_of_copy_rate']:.0f} % of the copy's rate.", "",
                  "| compute_iou_voxel on the device-resident clips | host clock, ms | ms per frame | mean IoU |", "|---|---|---|---|"]
        for r in get("compute_iou_voxel"):
            lines.append(f"| fill = {r['fill']} | {fmt(r['wall_ms'])} | {r['ms_per_frame']:.3f} | {r['iou_mean']:.4f} |")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
