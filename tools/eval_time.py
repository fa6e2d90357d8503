#!/usr/bin/env python3
"""Lab timing of the geometry-evaluation kernels (csrc/geometry.hip); the numbers live in profiles/geometry_eval.md.

Graph-free stream launches between device events, after a warm-up of every shape; the variants of one case are ALTERNATED
inside every round and the per-call time reported is the median over the rounds (min and max beside it).  The yardstick is
m324_nearest_point (one query per lane, indices only, one point set per launch) on the same point sets in the same process.

    python tools/eval_time.py --build-lab      # no GPU needed: tools/lablibs/libm324_q8.so, the library with 8 queries per lane
    python tools/eval_time.py [--out FILE]     # on the GPU; prints one JSON line per case

A run without a HIP device fails: there is no CPU timing."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAB_LIB = os.path.join(ROOT, "tools", "lablibs", "libm324_q8.so")


def build_lab():
    """the product's objects with geometry.hip recompiled at 8 queries per lane"""
    from motion324_amd import build as B
    B.build()
    os.makedirs(os.path.dirname(LAB_LIB), exist_ok=True)
    hipcc = B._hipcc()
    obj = os.path.join(os.path.dirname(LAB_LIB), "geometry_q8.o")
    subprocess.run([hipcc] + B.FLAGS + ["-DM324_NN_QPL=8", "-c", os.path.join(B.CSRC, "geometry.hip"), "-o", obj], check=True)
    objs = [os.path.join(B.OBJ, s.replace(".hip", ".o")) for s in B.SOURCES if s != "geometry.hip"] + [obj]
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LAB_LIB] + objs + ["-ldl"], check=True)
    print(LAB_LIB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-lab", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-sequence", action="store_true")
    args = ap.parse_args()
    if args.build_lab:
        return build_lab()

    import numpy as np
    import torch
    from motion324_amd import evaluation as ev, lib as L, ops, preprocess
    if not torch.cuda.is_available():
        sys.exit("eval_time: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream          # noqa: E731
    h4 = L.load()
    h8 = None
    if os.path.exists(LAB_LIB):
        h8 = C.CDLL(LAB_LIB)
        for name in ("m324_nn_search", "m324_nn_plan"):
            getattr(h8, name).argtypes, getattr(h8, name).restype = L.SIGNATURES[name], C.c_int
    results = []

    def emit(rec):
        results.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(variants, iters, rounds=args.rounds):
        """variants: {name: fn}; every fn enqueues ONE call.  Returns {name: (median, min, max)} in milliseconds per call."""
        for fn in variants.values():                                   # warm-up: code objects, allocator
            fn(); fn()
        torch.cuda.synchronize()
        per = {k: [] for k in variants}
        for _ in range(rounds):
            for name, fn in variants.items():                          # alternated inside the round
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(iters):
                    fn()
                b.record()
                b.synchronize()
                per[name].append(a.elapsed_time(b) / iters)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in per.items()}

    def search_fn(h, q, r, B, nq, nr, want_index, want_dist=True, ref_slices=0):
        need = C.c_long(0)
        slices = h.m324_nn_plan(nq, nr, B, ref_slices, C.addressof(need))
        assert slices >= 1
        scratch = torch.empty((max(need.value, 1),), dtype=torch.uint8, device=dev)
        dist = torch.empty((B, nq), dtype=torch.float32, device=dev) if want_dist else None
        index = torch.empty((B, nq), dtype=torch.int32, device=dev) if want_index else None
        sq, sr = (nq * 3, nr * 3) if B > 1 else (0, 0)

        def fn():
            rc = h.m324_nn_search(q.data_ptr(), sq, nq, r.data_ptr(), sr, nr, B, dist.data_ptr() if want_dist else None,
                                  index.data_ptr() if want_index else None, ref_slices, scratch.data_ptr(), need.value, stream())
            assert rc == 0, L.last_error()
        return fn, slices, dist, index

    def yardstick_fn(q, r, B, nq, nr):
        index = torch.empty((B, nq), dtype=torch.int32, device=dev)

        def fn():                                                      # one point set per launch: B launches
            for b in range(B):
                rc = h4.m324_nearest_point(q[b].data_ptr(), nq, r[b].data_ptr(), nr, index[b].data_ptr(), stream())
                assert rc == 0
        return fn, index

    def search_case(label, B, nq, nr, iters):
        g = torch.Generator().manual_seed(1)
        q = torch.rand(B, nq, 3, generator=g).to(dev)
        r = torch.rand(B, nr, 3, generator=g).to(dev)
        variants, outs, info = {}, {}, {}
        fn, index_y = yardstick_fn(q, r, B, nq, nr)
        variants["nearest_point (yardstick, index)"] = fn
        for tag, h in (("q4", h4), ("q8", h8)):
            if h is None:
                continue
            for kind, wi, wd in (("dist", False, True), ("dist+index", True, True), ("index", True, False)):
                fn, slices, dist, index = search_fn(h, q, r, B, nq, nr, wi, wd)
                variants[f"nn_search {tag} {kind}"] = fn
                outs[(tag, kind)] = (dist, index)
                info[tag] = slices
        t = timed(variants, iters)
        # same results before any speed is compared: indices against the yardstick (same arithmetic, same tie rule), distances across variants
        same_index = all(torch.equal(i, index_y) for (_, i) in outs.values() if i is not None)
        dists = [d for (d, _) in outs.values() if d is not None]
        same_dist = all(torch.equal(d, dists[0]) for d in dists)
        pairs = float(B) * nq * nr
        emit({"case": label, "batch": B, "n_query": nq, "n_ref": nr, "slices": info, "indices_equal_yardstick": same_index,
              "distances_equal_across_variants": same_dist,
              "ms": {k: {"median": round(v[0], 4), "min": round(v[1], 4), "max": round(v[2], 4), "Gpairs_per_s": round(pairs / v[0] / 1e6, 1)}
                     for k, v in t.items()}})

    search_case("metrics, 1 frame", 1, 50000, 50000, iters=5)
    search_case("metrics, 32 frames", 32, 50000, 50000, iters=1)
    search_case("ICP shape", 1, 20000, 10000, iters=20)

    if not args.skip_sequence:
        # the whole evaluate_sequence: 32 frames x 50 000 samples of a 4098-vertex deforming sphere (host clock around work that
        # ends in a device-to-host copy), split into its parts by timing them again one by one
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        v = [np.array(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
        f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
        for _ in range(5):
            cache, nf = {}, []

            def mid(a, b):
                k = (min(a, b), max(a, b))
                if k not in cache:
                    m = v[a] + v[b]
                    v.append(m / np.linalg.norm(m))
                    cache[k] = len(v) - 1
                return cache[k]
            for a, b, c in f:
                ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
                nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
            f = nf
        v, faces = np.array(v), np.array(f, dtype=np.int64)
        frames = np.stack([v * (1.0 + 0.01 * k * np.sin(3.0 * v[:, :1] + 0.1 * k)) * np.array([1.0, 0.8, 0.7]) for k in range(32)]).astype(np.float32)
        rng = np.random.default_rng(0)
        pred = (1.3 * frames + np.array([0.2, -0.1, 0.05]) + 0.003 * rng.standard_normal(frames.shape)).astype(np.float32)
        ev.evaluate_sequence(frames[:2], faces, pred[:2], faces, num_samples=2048)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.evaluate_sequence(frames, faces, pred, faces, num_samples=50000)
        t_all = time.perf_counter() - t0
        t0 = time.perf_counter()
        ev.evaluate_sequence(frames, faces, pred, faces, num_samples=50000, alignment=(res["R"], res["t"], res["s"]))
        t_no_icp = time.perf_counter() - t0
        t0 = time.perf_counter()
        for k in range(32):
            preprocess.sample_surface(frames[k], faces, 50000, k)
            preprocess.sample_surface(pred[k], faces, 50000, 100 + k)
        t_sampling = time.perf_counter() - t0
        emit({"case": "evaluate_sequence, 32 frames x 50000 samples, 4098 vertices", "wall_s": round(t_all, 3),
              "wall_s_with_alignment_given": round(t_no_icp, 3), "host_surface_sampling_s": round(t_sampling, 3),
              "chamfer_mean": float(np.mean(res["chamfer_distances"])), "fscore_mean": float(np.mean(res["fscores"]))})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
