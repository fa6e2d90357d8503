#!/usr/bin/env python3
"""Timing of the tracked surface samples (m324_vertex_normals, m324_surface_track in csrc/surface.hip; motion324_amd/dataset.py)
against the numpy host path that defines them; the numbers live in profiles/tracked_samples.md.

Two cases, both on an icosphere of 16 386 vertices / 32 768 faces that deforms over the clip:
  * the dataset's own sizes (configs/dyscene.yaml of the reference): 12 frames, 4096 shape + 4096 tracked samples, B = 16;
  * the long-clip case c3: B = 8 clips of 32 frames, the same sample counts.

The sizes are written out below: the repository carries no copy of that config file.

One process.  The kernels alone are timed between device events: every variant warmed up twice, the variants of a case
ALTERNATED inside each round, the median over the rounds reported (min and max beside it).  One side of the comparison is host
numpy, so the "wall" figures are host clock around a call that starts and ends with the device idle; the host path and the
device path are timed one after the other, not alternated (the host path takes seconds and is not warmed up, the device path
is warmed up twice, which also builds and caches the vertex-corner table; the first, uncached call is timed separately on a
fresh copy of the faces).  The event figures come with the
bytes each of them must move at least (its inputs read once, its outputs written once) over that time beside the rate of a
plain device-to-device copy of 256 MB measured the same way in the same run.  Before any speed is compared the run checks
that the device batch equals the host path (points and colours bit for bit, normals within 2^-23).

    python tools/track_time.py [--out FILE] [--rounds N]     # on the GPU; prints one JSON line per case

A run without a HIP device fails: there is no CPU timing."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def icosphere(levels):
    import numpy as np
    pv = [np.array(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    pf = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = pv[i] + pv[j]
                pv.append(m / np.linalg.norm(m))
                cache[k] = len(pv) - 1
            return cache[k]
        for i, j, k in pf:
            ij, jk, ki = mid(i, j), mid(j, k), mid(k, i)
            nf += [(i, ij, ki), (j, jk, ij), (k, ki, jk), (ij, jk, ki)]
        pf = nf
    return 0.45 * np.array(pv), np.array(pf, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2, help="rounds of the host path (seconds per call)")
    args = ap.parse_args()

    import numpy as np
    import torch
    from motion324_amd import dataset, ops, preprocess, synth
    if not torch.cuda.is_available():
        sys.exit("track_time: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    results = []

    def emit(rec):
        results.append(rec)
        print(json.dumps(rec), flush=True)

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def wall(fn, rounds, warm=2):
        for _ in range(warm):
            fn()
        per = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
        return stats(per)

    def events(variants, iters=10, rounds=args.rounds):
        for fn in variants.values():
            fn(); fn()
        torch.cuda.synchronize()
        per = {k: [] for k in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    fn()
                b.record()
                b.synchronize()
                per[name].append(a.elapsed_time(b) / iters)
        return {k: stats(v) for k, v in per.items()}

    # the copy yardstick: 256 MB read + 256 MB written
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = events({"copy": lambda: dst.copy_(src)})["copy"]["median"]
    copy_rate = 2 * src.numel() / (copy_ms * 1e-3) / 1e12
    emit({"case": "device-to-device copy of 256 MB", "ms": copy_ms, "TB_per_s": round(copy_rate, 3)})

    verts, faces = icosphere(6)
    nv, nf = len(verts), len(faces)
    face_uvs = synth.uniform(1, "track_time.uv", (nf, 3, 2)).astype(np.float64)
    tex = (synth.uniform(1, "track_time.tex", (512, 512, 3)) * 256).astype(np.uint8)
    n_shape = n_pcd = 4096
    cfg = {"training": {"num_shape_samples": n_shape, "num_pcd_samples": n_pcd}}

    for label, B, T in (("dataset sizes: B = 16 x 12 frames", 16, 12), ("c3: B = 8 x 32 frames", 8, 32)):
        clips = []
        for k in range(B):
            frames = np.stack([verts * (1.0 + 0.02 * np.sin(3.0 * verts[:, :1] + 0.2 * t + k)) * np.array([1.0, 0.9, 0.8]) for t in range(T)])
            clips.append(dict(vertex_frames=frames, faces=faces, face_uvs=face_uvs, texture_array=tex, rgb_video=np.zeros((T, 8, 8, 3), dtype=np.float32)))
        seeds = list(range(100, 100 + B))

        def host():                                   # the reference's two calls per sample, on the definition's numpy path
            out = []
            for c, s in zip(clips, seeds):
                a, b = dataset._draw_seeds(s)
                out.append((dataset.track_with_normal_rgb(c["vertex_frames"][:1], faces, n_shape, face_uvs, tex, seed=a),
                            dataset.track_with_normal_rgb(c["vertex_frames"], faces, n_pcd, face_uvs, tex, seed=b)))
            return out

        def device():                                 # from the same numpy arrays: checks, uploads, launches; the face list is known
            return dataset.make_training_batch(clips, cfg, seeds, device=dev)

        def first_call():                             # a face list seen for the first time: check, sort and uploads of the table included
            fresh = faces.copy()
            return dataset.make_training_batch([dict(c, faces=fresh) for c in clips], cfg, seeds, device=dev)

        batch, finite = device()
        ref = host()
        same_points = all(np.array_equal(batch["point_clouds"][k].cpu().numpy(), ref[k][1][0].numpy()) and
                          np.array_equal(batch["ref_shape_pcd"][k].cpu().numpy(), ref[k][0][0][0].numpy()) and
                          np.array_equal(batch["ref_rgb"][k].cpu().numpy(), ref[k][1][2][0].numpy()) for k in range(B))
        normal_err = max(float((batch["ref_normal"][k].cpu() - ref[k][1][1][0]).abs().max()) for k in range(B))

        v = torch.stack([torch.from_numpy(c["vertex_frames"]) for c in clips]).to(dev)
        f = torch.from_numpy(faces.astype(np.int32)).to(dev)
        table = ops.vertex_corners(f, nv)
        vn = ops.vertex_normals(v, f, table, faces_checked=True)
        cdf = ops.surface_cdf(v[:, 0], f, faces_checked=True)
        sd = torch.from_numpy(preprocess.surface_seeds(seeds)).to(dev)
        uv_d, tex_d = torch.from_numpy(face_uvs).to(dev), torch.from_numpy(tex).to(dev)
        kernels = events({
            "m324_vertex_normals (angle)": lambda: ops.vertex_normals(v, f, table, faces_checked=True),
            "m324_vertex_normals (area)": lambda: ops.vertex_normals(v, f, table, "area", faces_checked=True),
            "m324_surface_cdf (frame 0)": lambda: ops.surface_cdf(v[:, 0], f, faces_checked=True),
            "m324_surface_track (points, normals, colours)": lambda: ops.surface_track(v, f, cdf, sd, n_pcd, vertex_normals=vn, face_uvs=uv_d,
                                                                                       texture=tex_d, want_face=False, faces_checked=True),
            "m324_surface_track (points only)": lambda: ops.surface_track(v, f, cdf, sd, n_pcd, want_face=False, faces_checked=True)})
        least = {                                     # bytes: inputs once + outputs once
            "m324_vertex_normals (angle)": 2 * B * T * nv * 24 + nf * 12 * 2 + nv * 4,
            "m324_vertex_normals (area)": 2 * B * T * nv * 24 + nf * 12 * 2 + nv * 4,
            "m324_surface_cdf (frame 0)": B * nv * 24 + nf * 12 + B * nf * 8,
            "m324_surface_track (points, normals, colours)": 2 * B * T * n_pcd * 12 + B * n_pcd * 12 + 2 * B * T * min(nv, 3 * n_pcd) * 24,
            "m324_surface_track (points only)": B * T * n_pcd * 12 + B * T * min(nv, 3 * n_pcd) * 24}
        for name, rec in kernels.items():
            rec["least_MB"] = round(least[name] / 1e6, 2)
            rec["TB_per_s"] = round(least[name] / (rec["median"] * 1e-3) / 1e12, 3)
            rec["of_copy_rate"] = round(rec["TB_per_s"] / copy_rate, 3)
        emit({"case": f"{label}, {n_shape} + {n_pcd} samples, {nv} vertices / {nf} faces",
              "device_points_and_colours_equal_host_bit_for_bit": bool(same_points), "worst_normal_component_error": normal_err,
              "all_finite": bool(finite.all()),
              "wall_ms": {"host: 2 x track_with_normal_rgb per clip": wall(host, args.host_rounds, warm=0),
                          "device: make_training_batch from numpy": wall(device, args.rounds),
                          "device: the same, first call on a face list": wall(first_call, args.rounds, warm=0)},
              "device_events_ms": kernels})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
