#!/usr/bin/env python3
"""Timing of the device surface sampler (csrc/surface.hip) against the host sampler it reproduces; the numbers live in
profiles/surface_sampler.md.

One process.  Every variant is warmed up twice; the variants of one case are ALTERNATED inside each of 7 rounds and the time
reported is the median over the rounds (min and max beside it).  All times are host clock around a call that ends with the
device idle (torch.cuda.synchronize), because one side of every comparison is host numpy: the yardstick is
preprocess.sample_surface / the host path of the caller, in the same process.  The device kernels alone are timed between
device events as well.

    python tools/sampler_time.py [--out FILE]     # on the GPU; prints one JSON line per case

A run without a HIP device fails: there is no CPU timing."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-sequence", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import surface_cases as sc
    from motion324_amd import evaluation as ev, ops, preprocess
    if not torch.cuda.is_available():
        sys.exit("sampler_time: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    results = []

    def emit(rec):
        results.append(rec)
        print(json.dumps(rec), flush=True)

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def wall(variants, rounds=args.rounds):
        """variants: {name: fn}; host clock around one call each, device idle before and after; milliseconds"""
        for fn in variants.values():
            fn(); fn()
        torch.cuda.synchronize()
        per = {k: [] for k in variants}
        for _ in range(rounds):
            for name, fn in variants.items():                          # alternated inside the round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                per[name].append((time.perf_counter() - t0) * 1e3)
        return {k: stats(v) for k, v in per.items()}

    def events(variants, iters, rounds=args.rounds):
        """the same for work that stays on the device: between device events, milliseconds per call"""
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

    # ---- 1. the sampler: 1 x 50 000 and 64 x 50 000 samples of the 8192-face soup
    v, f, colors = sc.soup()
    num = 50000
    for B in (1, 64):
        meshes = np.stack([v * (1.0 + 0.01 * k) for k in range(B)])
        seeds = list(range(10, 10 + B))
        vd = torch.from_numpy(meshes if B > 1 else meshes[0]).to(dev)
        fd = torch.from_numpy(f.astype(np.int32)).to(dev)
        sd = torch.from_numpy(preprocess.surface_seeds(seeds if B > 1 else seeds[0])).to(dev)
        sd = sd if B > 1 else sd[0]

        def host():
            for k in range(B):
                preprocess.sample_surface(meshes[k], f, num, seeds[k])

        def device_from_numpy():                                       # upload, CDF, draw: what a caller with host meshes pays
            preprocess.sample_surface_device(meshes if B > 1 else meshes[0], f, num, seeds if B > 1 else seeds[0], dev)

        cdf = ops.surface_cdf(vd, fd)
        cd = torch.from_numpy(colors).to(dev)
        kernels = events({"m324_surface_cdf": lambda: ops.surface_cdf(vd, fd, faces_checked=True),
                          "m324_surface_sample (points + face index)": lambda: ops.surface_sample(vd, fd, cdf, sd, num, faces_checked=True),
                          "m324_surface_sample (+ fp64 points, normals, vertex colours)": lambda: ops.surface_sample(
                              vd, fd, cdf, sd, num, faces_checked=True, want_points64=True, want_normals=True, want_colors=True,
                              vertex_colors=cd)}, iters=10)
        # same samples before any speed is compared
        got = ops.surface_sample(vd, fd, cdf, sd, num, faces_checked=True, want_points64=True)
        p64 = got.points64.cpu().numpy().reshape(B, num, 3)
        fi = got.face_index.cpu().numpy().reshape(B, num)
        same = all(np.array_equal(p64[k], pts) and np.array_equal(fi[k], idx)
                   for k in range(B) for pts, idx in [preprocess.sample_surface(meshes[k], f, num, seeds[k])])
        emit({"case": f"sampler, {B} x {num} samples, {len(f)} faces", "device_equals_host_bit_for_bit": bool(same),
              "wall_ms": wall({"host sample_surface": host, "device sample_surface_device (from numpy)": device_from_numpy}),
              "device_events_ms": kernels})

    # ---- 2. prepare_mesh_data, host against device sampler (16 384 shape samples of the soup)
    vn = np.zeros_like(v, dtype=np.float32)
    vn[:, 2] = 1.0
    mesh = {"vertices": v.astype(np.float32), "faces": f, "vertex_normals": vn, "vertex_colors": colors}
    cfg = {"training": {"num_shape_samples": 16384}}
    a = preprocess.prepare_mesh_data(cfg, mesh, dev, seed=1)[0]
    b = preprocess.prepare_mesh_data(cfg, mesh, dev, seed=1, sampler="device")[0]
    emit({"case": "prepare_mesh_data, 16384 shape samples, 4098 vertices / 8192 faces",
          "device_equals_host_bit_for_bit": bool(all(torch.equal(a[k], b[k]) for k in a)),
          "wall_ms": wall({"sampler=host": lambda: preprocess.prepare_mesh_data(cfg, mesh, dev, seed=1),
                           "sampler=device": lambda: preprocess.prepare_mesh_data(cfg, mesh, dev, seed=1, sampler="device")})})

    # ---- 3. the evaluate_sequence of profiles/geometry_eval.md: 32 frames x 50 000 samples of a 4098-vertex deforming sphere
    if not args.skip_sequence:
        pv = [np.array(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
        pf = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
        for _ in range(5):
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
        sv, faces = np.array(pv), np.array(pf, dtype=np.int64)
        frames = np.stack([sv * (1.0 + 0.01 * k * np.sin(3.0 * sv[:, :1] + 0.1 * k)) * np.array([1.0, 0.8, 0.7]) for k in range(32)]).astype(np.float32)
        rng = np.random.default_rng(0)
        pred = (1.3 * frames + np.array([0.2, -0.1, 0.05]) + 0.003 * rng.standard_normal(frames.shape)).astype(np.float32)
        res = ev.evaluate_sequence(frames, faces, pred, faces, num_samples=50000)
        alignment = (res["R"], res["t"], res["s"])
        res_d = ev.evaluate_sequence(frames, faces, pred, faces, num_samples=50000, sampler="device")
        same = res_d["chamfer_distances"] == res["chamfer_distances"] and res_d["fscores"] == res["fscores"]
        run = lambda **kw: (lambda: ev.evaluate_sequence(frames, faces, pred, faces, num_samples=50000, **kw))      # noqa: E731
        t = wall({"sampler=host": run(), "sampler=device": run(sampler="device"),
                  "sampler=host, alignment given": run(alignment=alignment),
                  "sampler=device, alignment given": run(alignment=alignment, sampler="device")})
        # what the device call is made of, with the alignment given: host transforms, the two draws (upload included), the metrics
        _, gc, gs = ev.normalize_points(frames[0])
        _, pc, ps = ev.normalize_points(pred[0])
        hold = {}

        def transforms():
            hold["gt"] = np.stack([ev.apply_icp_alignment(ev.apply_normalization(frames[k], gc, gs), *alignment) for k in range(32)])
            hold["pred"] = np.stack([ev.apply_normalization(pred[k], pc, ps) for k in range(32)])

        def draws():
            hold["a"] = preprocess.sample_surface_device(hold["gt"], faces, 50000, [ev.sample_seed(0, 0, k) for k in range(32)], dev)[0]
            hold["b"] = preprocess.sample_surface_device(hold["pred"], faces, 50000, [ev.sample_seed(0, 1, k) for k in range(32)], dev)[0]

        transforms(); draws()
        parts = wall({"fp64 host transforms of 2 x 32 frames": transforms, "2 x (upload, CDF, draw)": draws,
                      "chamfer_and_fscore on device points": lambda: ev.chamfer_and_fscore(hold["a"], hold["b"])})
        emit({"case": "evaluate_sequence, 32 frames x 50000 samples, 4098 vertices", "device_equals_host": bool(same), "wall_ms": t,
              "parts_of_the_device_call_ms": parts, "chamfer_mean": float(np.mean(res["chamfer_distances"])),
              "fscore_mean": float(np.mean(res["fscores"]))})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
