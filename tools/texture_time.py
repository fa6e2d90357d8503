#!/usr/bin/env python3
"""Timing of textured and supersampled mesh clips (render_clip with uv / texture / supersample, csrc/render.hip); the numbers
live in profiles/mesh_render_textured.md.

The two sphere meshes of tools/render_time.py (c2: 8192 faces; dense: 199712 faces), 32 frames each, S = 512, a 2048 x 2048 seeded
noise texture mapped once around the sphere (longitude, latitude), which minifies it.  Four configurations of render_clip on the
device-resident clip, interleaved round by round in one process:
  * colors:        per-vertex colours, the path through m324_render_shade that textures did not touch;
  * tex_mips:      the texture, mipmaps=True (the mip chain is built inside every call);
  * tex_level0:    the texture, mipmaps=False;
  * tex_mips_ss2:  the texture, mipmaps=True, supersample=2 (rasterized at 1024).
Device events around each call, one warm-up round, median of the rounds with (min .. max).  Next to them the mip build alone
(ops.texture_mips) and the shade stage alone per configuration, project and raster redone untimed in front of it.  Before any
time is reported the textured result is compared across big_pixels in {0, 64, 2^31 - 1}, bit for bit.

    python tools/texture_time.py [--size 512] [--rounds 5] [--frames 32] [--texture 2048] [--cases c2,dense] [--out FILE.md]

A run without a HIP device fails: there is no CPU timing of the GPU path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

CASES = {"c2": 64, "dense": 316}
CONFIGS = ("colors", "tex_mips", "tex_level0", "tex_mips_ss2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--texture", type=int, default=2048, help="side of the square noise texture")
    ap.add_argument("--cases", default="c2,dense")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from motion324_amd import ops, render
    from render_time import clip_of, sphere
    if not torch.cuda.is_available():
        sys.exit("texture_time: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    S, T, R = args.size, args.frames, args.rounds
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def summary(ms):
        return statistics.median(ms), min(ms), max(ms)

    g = torch.Generator(device=dev).manual_seed(324)
    texture = torch.randint(0, 256, (args.texture, args.texture, 3), generator=g, device=dev, dtype=torch.uint8)
    ops.texture_mips(texture)
    torch.cuda.synchronize()
    build = summary([timed(lambda: ops.texture_mips(texture)) for _ in range(R)])
    levels, chain = ops.texture_plan(args.texture, args.texture)
    emit(dict(what="mip_build", texture=args.texture, levels=levels, chain_bytes=chain, events_ms=build))

    for name in args.cases.split(","):
        n = CASES[name]
        base, faces = sphere(n, dev)
        clip = clip_of(base, T)
        nv, nf = base.shape[0], faces.shape[0]
        i = torch.arange(n + 1, device=dev, dtype=torch.float32) / n
        la, lo = torch.meshgrid(i, i, indexing="ij")
        uv = torch.stack([lo, la], dim=-1).reshape(-1, 2).contiguous()           # the grid of sphere(): longitude, latitude
        colors = torch.rand((nv, 3), generator=g, device=dev)
        kw = dict(size=S, azimuth=20.0, elevation=10.0)
        calls = {"colors": lambda: render.render_clip(clip, faces, colors=colors, **kw),
                 "tex_mips": lambda: render.render_clip(clip, faces, uv=uv, texture=texture, **kw),
                 "tex_level0": lambda: render.render_clip(clip, faces, uv=uv, texture=texture, mipmaps=False, **kw),
                 "tex_mips_ss2": lambda: render.render_clip(clip, faces, uv=uv, texture=texture, supersample=2, **kw)}

        first = render.render_clip(clip, faces, uv=uv, texture=texture, big_pixels=0, **kw)
        same = all(all(torch.equal(a, b) for a, b in zip(first, render.render_clip(clip, faces, uv=uv, texture=texture, big_pixels=bp, **kw)))
                   for bp in (64, 2 ** 31 - 1))
        emit(dict(case=name, what="check", frames=T, vertices=nv, faces=nf, size=S, identical_for_every_big_pixels=same,
                  covered_share=float((first.face >= 0).float().mean())))
        if not same:
            sys.exit("texture_time: the textured result depends on big_pixels; no time is reported")
        del first

        m = render.view_matrix(20.0, 10.0)
        per = {c: [] for c in CONFIGS}
        for r in range(R + 1):                                                   # round 0 is the warm-up; configurations interleaved
            for c in CONFIGS:
                ms = timed(calls[c])
                if r:
                    per[c].append(ms)
        for c in CONFIGS:
            s = summary(per[c])
            emit(dict(case=name, what="clip", config=c, events_ms=s, ms_per_frame=s[0] / T))

        # the shade stage alone: project and raster redone (untimed) in front of every timed call
        fuv = uv[faces.long()].contiguous()
        mips, _ = ops.texture_mips(texture)
        tex = dict(face_uvs=fuv, mips=mips, tex_size=(args.texture, args.texture))
        stage = {c: [] for c in CONFIGS}
        for side, ss, configs in ((S, 1, CONFIGS[:3]), (2 * S, 2, CONFIGS[3:])):
            scratch = torch.empty((ops.render_plan(nv, nf, T, side),), dtype=torch.uint8, device=dev)
            out = (torch.empty((T, side // ss, side // ss, 3), dtype=torch.uint8, device=dev), torch.empty((T, side, side), dtype=torch.int32, device=dev),
                   torch.empty((T, side, side), dtype=torch.int32, device=dev))
            shade = {"colors": lambda: ops.render_shade(faces, nv, T, side, scratch, m, colors=colors, out=out, faces_checked=True),
                     "tex_mips": lambda: ops.render_shade_tex(faces, nv, T, side, scratch, m, out=out, faces_checked=True, **tex),
                     "tex_level0": lambda: ops.render_shade_tex(faces, nv, T, side, scratch, m, out=out, use_mips=False, faces_checked=True, **tex),
                     "tex_mips_ss2": lambda: ops.render_shade_tex(faces, nv, T, side, scratch, m, out=out, supersample=2, faces_checked=True, **tex)}
            for r in range(R + 1):
                for c in configs:
                    ops.render_project(clip, m, side, nf, scratch)
                    ops.render_raster(faces, nv, T, side, scratch, None, faces_checked=True)
                    ms = timed(shade[c])
                    if r:
                        stage[c].append(ms)
            del scratch, out
        for c in CONFIGS:
            s = summary(stage[c])
            emit(dict(case=name, what="shade", config=c, events_ms=s, us_per_frame=s[0] * 1e3 / T))
        del clip, mips, fuv
        torch.cuda.empty_cache()

    if args.out:
        prop = torch.cuda.get_device_properties(0)
        arch = getattr(prop, "gcnArchName", "").split(":")[0]
        fmt = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"       # noqa: E731
        mb = next(r for r in records if r["what"] == "mip_build")
        lines = ["# Textured and supersampled mesh clips: what was measured", "",
                 f"`tools/texture_time.py` on one GPU ({prop.name}, {arch}, {prop.multi_processor_count} CUs), one process, one run, S = {S}, {T} frames, a "
                 f"{args.texture} x {args.texture} noise texture mapped once around the sphere.  The clips are device-resident.  Device events around "
                 f"the calls, one warm-up round, median of {R} rounds with (min .. max), the configurations interleaved round by round.  Before "
                 "timing, the textured result was compared across big_pixels in {0, 64, 2^31 - 1}: bit-identical in every case.", "",
                 f"Mip build alone (`ops.texture_mips`, {mb['levels']} levels, {mb['chain_bytes'] / 2 ** 20:.1f} MiB): {fmt(mb['events_ms'])} ms.  "
                 "`render_clip` builds the chain once per call, so the textured rows below include it.", ""]
        for name in args.cases.split(","):
            rec = [r for r in records if r.get("case") == name]
            chk = next(r for r in rec if r["what"] == "check")
            ref = next(r for r in rec if r["what"] == "clip" and r["config"] == "colors")
            sref = next(r for r in rec if r["what"] == "shade" and r["config"] == "colors")
            lines += [f"## {name}: {chk['vertices']} vertices, {chk['faces']} faces, {chk['frames']} frames", "",
                      f"{100 * chk['covered_share']:.1f} % of the pixels are covered.", "",
                      "| configuration | render_clip, ms per clip | ms per frame | ratio to colors | shade stage alone, ms per clip | us per frame | ratio to colors |",
                      "|---|---|---|---|---|---|---|"]
            for c in CONFIGS:
                a = next(r for r in rec if r["what"] == "clip" and r["config"] == c)
                b = next(r for r in rec if r["what"] == "shade" and r["config"] == c)
                lines.append(f"| {c} | {fmt(a['events_ms'])} | {a['ms_per_frame']:.4f} | {a['events_ms'][0] / ref['events_ms'][0]:.2f} | {fmt(b['events_ms'])} | "
                             f"{b['us_per_frame']:.1f} | {b['events_ms'][0] / sref['events_ms'][0]:.2f} |")
            lines.append("")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
