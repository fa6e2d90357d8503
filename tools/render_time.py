#!/usr/bin/env python3
"""Timing of the mesh clip renderer (motion324_amd.render.render_clip, csrc/render.hip); the numbers live in
profiles/mesh_render.md.

Three synthetic clips, generated on the device from a seed (a latitude / longitude sphere that turns and wobbles, or a box):
  * c2:    64 x 64 quads (4225 vertices, 8192 faces), 32 frames;
  * dense: 316 x 316 quads (100489 vertices, 199712 faces), 256 frames;
  * box:   12 faces that fill most of the image, 32 frames: every triangle goes down the queued path.
Per clip and per big_pixels in {16, 64, 256, 1024}: the host clock around render_clip on the device-resident clip (ending in a
synchronise) and device events around the whole call and around each stage (project, raster, shade) over the same chunks
render_clip uses.  The resolve stage is set against its byte floor, T * S^2 * (8 read + 11 written) bytes at the HBM peak of
8.0 TB/s, and against a device-to-device copy of 1 GiB timed the same way.  Before any time is reported the results for the
four big_pixels are compared with each other, bit for bit.

    python tools/render_time.py [--size 512] [--rounds 5] [--cases c2,dense,box] [--out FILE.md]

A run without a HIP device fails: there is no CPU timing of the GPU path."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

HBM_PEAK = 8.0e12
BIG = (16, 64, 256, 1024)
CASES = {"c2": (64, 32), "dense": (316, 256), "box": (0, 32)}


def sphere(n, dev):
    """(vertices fp32 [(n+1)^2, 3] of radius 0.42, faces int32 [2 n^2, 3]) of a latitude / longitude grid"""
    import torch
    i = torch.arange(n + 1, device=dev, dtype=torch.float64)
    lat = (i / n - 0.5) * math.pi * 0.998
    lon = i / n * 2.0 * math.pi
    la, lo = torch.meshgrid(lat, lon, indexing="ij")
    v = 0.42 * torch.stack([la.cos() * lo.cos(), la.sin(), la.cos() * lo.sin()], dim=-1).reshape(-1, 3)
    r, c = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
    a = (r * (n + 1) + c).reshape(-1)
    faces = torch.cat([torch.stack([a, a + 1, a + n + 2], dim=1), torch.stack([a, a + n + 2, a + n + 1], dim=1)])
    return v.float(), faces.to(torch.int32).contiguous()


def box(dev):
    import torch
    s = 0.33
    v = torch.tensor([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], dtype=torch.float32, device=dev)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    faces = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, torch.tensor(faces, dtype=torch.int32, device=dev)


def clip_of(base, T, wobble=0.003, seed=0):
    """[T,V,3]: frame t turns the mesh by 3 t degrees around y and 1 t around x and adds a seeded per-vertex wobble"""
    import torch
    g = torch.Generator(device=base.device).manual_seed(seed)
    out = torch.empty((T,) + tuple(base.shape), dtype=torch.float32, device=base.device)
    for t in range(T):
        a, b = math.radians(3.0 * t), math.radians(1.0 * t)
        ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float32, device=base.device)
        rx = torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]], dtype=torch.float32, device=base.device)
        out[t] = base @ (rx @ ry).T + wobble * torch.randn(base.shape, generator=g, device=base.device)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="c2,dense,box")
    ap.add_argument("--frames", type=int, default=0, help="override every case's frame count (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from motion324_amd import ops, render
    if not torch.cuda.is_available():
        sys.exit("render_time: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    S = args.size
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def events(fn, rounds=args.rounds):
        """median, min, max in ms of fn() between device events, after one warm-up call"""
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    def wall(fn, rounds=args.rounds):
        fn()
        torch.cuda.synchronize()
        s = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            s.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(s), min(s), max(s)

    gib = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    gib2 = torch.empty_like(gib)
    copy_ms = events(lambda: gib2.copy_(gib))
    copy_rate = 2 * (1 << 30) / (copy_ms[0] * 1e-3)
    del gib, gib2
    emit(dict(case="copy_1GiB", events_ms=copy_ms, bytes_per_s=copy_rate))

    for name in args.cases.split(","):
        n, T = CASES[name]
        T = args.frames or T
        base, faces = box(dev) if n == 0 else sphere(n, dev)
        clip = clip_of(base, T)
        nv, nf = base.shape[0], faces.shape[0]
        m = render.view_matrix(20.0, 10.0)
        kw = dict(size=S, azimuth=20.0, elevation=10.0)

        # results before speed: the four big_pixels (and both ends of its range) must agree bit for bit
        first = render.render_clip(clip, faces, big_pixels=BIG[0], **kw)
        same = all(all(torch.equal(a, b) for a, b in zip(first, render.render_clip(clip, faces, big_pixels=bp, **kw))) for bp in BIG[1:] + (0, 2 ** 31 - 1))
        covered = float((first.face >= 0).float().mean())
        emit(dict(case=name, what="check", frames=T, vertices=nv, faces=nf, size=S, identical_for_every_big_pixels=same, covered_share=covered))
        if not same:
            sys.exit("render_time: the result depends on big_pixels; no time is reported")
        del first

        per_frame = ops.render_plan(nv, nf, 1, S)
        chunk = max(1, min(T, (1 << 30) // per_frame))
        while chunk > 1 and ops.render_plan(nv, nf, chunk, S) > (1 << 30):
            chunk -= 1
        scratch = torch.empty((ops.render_plan(nv, nf, chunk, S),), dtype=torch.uint8, device=dev)
        out = (torch.empty((chunk, S, S, 3), dtype=torch.uint8, device=dev), torch.empty((chunk, S, S), dtype=torch.int32, device=dev),
               torch.empty((chunk, S, S), dtype=torch.int32, device=dev))
        spans = [(t0, min(T, t0 + chunk)) for t0 in range(0, T, chunk)]
        emit(dict(case=name, what="chunks", frames_per_chunk=chunk, chunks=len(spans), scratch_bytes=scratch.numel()))

        def prepare(t0, t1, bp):
            ops.render_project(clip[t0:t1], m, S, nf, scratch)
            ops.render_raster(faces, nv, t1 - t0, S, scratch, bp, faces_checked=True)

        def stage_ms(stage, bp):
            """device events around one stage over every chunk, the stages in front of it redone (untimed) per chunk"""
            total = []
            for _ in range(args.rounds + 1):
                ms = 0.0
                for t0, t1 in spans:
                    k = t1 - t0
                    if stage == "project":
                        fn = lambda: ops.render_project(clip[t0:t1], m, S, nf, scratch)                              # noqa: E731
                    elif stage == "raster":
                        ops.render_project(clip[t0:t1], m, S, nf, scratch)
                        fn = lambda: ops.render_raster(faces, nv, k, S, scratch, bp, faces_checked=True)             # noqa: E731
                    else:
                        prepare(t0, t1, bp)
                        fn = lambda: ops.render_shade(faces, nv, k, S, scratch, m, out=tuple(o[:k] for o in out), faces_checked=True)   # noqa: E731
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    ms += a.elapsed_time(b)
                total.append(ms)
            total = total[1:]                                    # the first round is the warm-up
            return statistics.median(total), min(total), max(total)

        pj = stage_ms("project", 64)
        emit(dict(case=name, what="stage", stage="project", events_ms=pj, us_per_frame=pj[0] * 1e3 / T))
        sh = stage_ms("shade", 64)
        floor_bytes = T * S * S * 19
        emit(dict(case=name, what="stage", stage="shade", events_ms=sh, us_per_frame=sh[0] * 1e3 / T, floor_bytes=floor_bytes,
                  floor_ms_at_hbm_peak=floor_bytes / HBM_PEAK * 1e3, share_of_floor=floor_bytes / HBM_PEAK * 1e3 / sh[0],
                  share_of_copy_rate=floor_bytes / (sh[0] * 1e-3) / copy_rate))
        for bp in BIG:
            rs = stage_ms("raster", bp)
            ev = events(lambda: render.render_clip(clip, faces, big_pixels=bp, **kw))
            wl = wall(lambda: render.render_clip(clip, faces, big_pixels=bp, **kw))
            emit(dict(case=name, what="big_pixels", big_pixels=bp, raster_events_ms=rs, raster_us_per_frame=rs[0] * 1e3 / T, clip_events_ms=ev,
                      clip_wall_ms=wl, wall_ms_per_frame=wl[0] / T))
        del clip, scratch, out
        torch.cuda.empty_cache()

    if args.out:
        prop = torch.cuda.get_device_properties(0)
        arch = getattr(prop, "gcnArchName", "").split(":")[0]
        fmt = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"       # noqa: E731
        lines = ["# Mesh clip rendering: what was measured", "",
                 f"`tools/render_time.py` on one GPU ({prop.name}, {arch}, {prop.multi_processor_count} CUs), one process, one run, S = {S}.  The clips "
                 f"are device-resident.  Device events around the calls, one warm-up, median of {args.rounds} rounds with (min .. max); the host clock "
                 "ends in a device synchronise.  Before timing, the results for big_pixels in {0, 16, 64, 256, 1024, 2^31 - 1} were compared: "
                 "bit-identical in every case.", "",
                 f"Copy rate of this box: {copy_rate / 1e12:.2f} TB/s (device-to-device copy of 1 GiB, reads + writes, {fmt(copy_ms)} ms).", ""]
        for name in args.cases.split(","):
            rec = [r for r in records if r.get("case") == name]
            chk = next(r for r in rec if r["what"] == "check")
            chunks = next(r for r in rec if r["what"] == "chunks")
            lines += [f"## {name}: {chk['vertices']} vertices, {chk['faces']} faces, {chk['frames']} frames", "",
                      f"{100 * chk['covered_share']:.1f} % of the pixels are covered; {chunks['chunks']} chunk(s) of {chunks['frames_per_chunk']} frames, "
                      f"{chunks['scratch_bytes'] / 2 ** 20:.0f} MiB of scratch.", "",
                      "| big_pixels | raster, ms per clip | raster, us per frame | render_clip, events, ms | render_clip, host clock, ms | ms per frame (host clock) |",
                      "|---|---|---|---|---|---|"]
            for r in rec:
                if r["what"] == "big_pixels":
                    lines.append(f"| {r['big_pixels']} | {fmt(r['raster_events_ms'])} | {r['raster_us_per_frame']:.1f} | {fmt(r['clip_events_ms'])} | "
                                 f"{fmt(r['clip_wall_ms'])} | {r['wall_ms_per_frame']:.4f} |")
            lines += ["", "| stage (big_pixels = 64) | ms per clip | us per frame |", "|---|---|---|"]
            for r in rec:
                if r["what"] == "stage":
                    lines.append(f"| {r['stage']} | {fmt(r['events_ms'])} | {r['us_per_frame']:.1f} |")
            shade = next(r for r in rec if r["what"] == "stage" and r["stage"] == "shade")
            lines += ["", f"Resolve: its byte floor is {shade['floor_bytes'] / 1e6:.1f} MB = {shade['floor_ms_at_hbm_peak']:.3f} ms at the HBM peak of 8.0 TB/s; "
                      f"the stage runs at {100 * shade['share_of_floor']:.1f} % of that floor ({100 * shade['share_of_copy_rate']:.1f} % of the measured copy rate).", ""]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
