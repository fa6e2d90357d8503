#!/usr/bin/env python3
"""Golden of the geometry evaluation (tests/golden/eval_pcd.npz), produced by running the reference's OWN functions:
evaluation/evaluation_pcd.py is imported whole, with trimesh, matplotlib and mpl_toolkits shimmed as absent packages (none of
the functions called here touches them; scipy's cKDTree is the real one).  It runs normalize_mesh, apply_normalization,
apply_icp_alignment, compute_chamfer_distance, compute_fscore and icp_alignment (optimize_scale False and True) on the
inputs of tests/eval_inputs.py and stores outputs, seeds and sizes only.

The maker asserts on its own inputs, and SEED is chosen so that all of it holds:
  (a) no nearest distance of the metric case lies within 1e-6 of the threshold 0.02;
  (b) an fp64 numpy replay of the ICP loop (brute force instead of the k-d tree) reproduces the reference's (R, t, s), and in
      every iteration of it each query's nearest and second-nearest d2 differ by more than 1e-6 relative;
  (c) the same replay with the search done in fp32 on the fp32-rounded transformed points (what m324_nn_search does) picks
      the same correspondences in every iteration.
These are not measurements of the code under test: they keep an fp32 search from legitimately picking another neighbour.
Build container only: needs the reference checkout and scipy."""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import eval_inputs  # noqa: E402

REFERENCE = os.environ.get("M324_REFERENCE") or os.path.join(os.path.dirname(REPO), "reference")      # a checkout beside this one
SEED = int(os.environ.get("M324_EVAL_SEED", "0"))
THRESHOLD = 0.02


def load_reference():
    for name in ("trimesh", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["mpl_toolkits.mplot3d"].Axes3D = None
    spec = importlib.util.spec_from_file_location("evaluation_pcd", os.path.join(REFERENCE, "evaluation", "evaluation_pcd.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def nearest_two(query, ref, dtype):
    q, r = query.astype(dtype), ref.astype(dtype)
    diff = q[:, None, :] - r[None, :, :]
    d2 = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
    idx = np.argmin(d2, axis=1)
    part = np.partition(d2, 1, axis=1)
    return idx, part[:, 0], part[:, 1], d2


def replay_icp(source, target, optimize_scale, max_iterations=1000, tolerance=1e-7):
    """the reference's loop in fp64 numpy with a brute-force search; returns (R, t, s, iterations, smallest relative margin
    between nearest and second-nearest d2, whether an fp32 search agreed everywhere)"""
    rng_s = np.max((source.max(0) - source.min(0))[:2])
    rng_t = np.max((target.max(0) - target.min(0))[:2])
    scale = np.clip(rng_t / rng_s, 0.95, 1.05)
    R, t, prev = np.eye(3), np.zeros(3), float("inf")
    margin, fp32_agrees, its = np.inf, True, 0
    for its in range(1, max_iterations + 1):
        moved = scale * (source @ R.T) + t
        idx, d0, d1, d2 = nearest_two(moved, target, np.float64)
        margin = min(margin, float(np.min((d1 - d0) / d1)))
        idx32 = nearest_two(moved.astype(np.float32), target, np.float32)[0]
        fp32_agrees = fp32_agrees and bool(np.array_equal(idx, idx32))
        matched = target[idx]
        error = np.mean(np.sqrt(d2[np.arange(len(idx)), idx]))
        if abs(prev - error) < tolerance:
            break
        prev = error
        cs, cm = moved.mean(0), matched.mean(0)
        H = (moved - cs).T @ (matched - cm)
        U, _, Vt = np.linalg.svd(H)
        Rd = Vt.T @ U.T
        if np.linalg.det(Rd) < 0:
            Vt[-1, :] *= -1
            Rd = Vt.T @ U.T
        td = cm - cs @ Rd.T
        R = R @ Rd
        t = t @ Rd.T + td
        U, _, Vt = np.linalg.svd(R)
        R = U @ Vt
        if optimize_scale:
            srt = source @ R.T + t
            den = np.sum(srt * srt)
            if den > 1e-10:
                scale = np.clip(0.8 * scale + 0.2 * np.clip(np.sum(matched * srt) / den, 0.95, 1.05), 0.95, 1.05)
    return R, t, float(scale), its, margin, fp32_agrees


def main():
    ref = load_reference()
    save = {"seed": np.int64(SEED), "threshold": np.float64(THRESHOLD), "icp_source": np.int64(eval_inputs.ICP_SOURCE),
            "icp_target": np.int64(eval_inputs.ICP_TARGET), "metric_points": np.int64(eval_inputs.METRIC_POINTS),
            "norm_vertices": np.int64(eval_inputs.NORM_VERTICES)}

    # ---- metrics
    p1, p2 = (a.astype(np.float64) for a in eval_inputs.metric_case(SEED))
    save["chamfer"] = np.float64(ref.compute_chamfer_distance(p1, p2))
    save["fscore"] = np.float64(ref.compute_fscore(p1, p2, threshold=THRESHOLD))
    _, d12, _, _ = nearest_two(p1, p2, np.float64)
    _, d21, _, _ = nearest_two(p2, p1, np.float64)
    dists = np.sqrt(np.concatenate([d12, d21]))
    assert np.min(np.abs(dists - THRESHOLD)) > 1e-6, ("condition (a) fails for this seed", np.min(np.abs(dists - THRESHOLD)))
    assert dists.max() < 0.2, dists.max()
    below = float(np.mean(dists < THRESHOLD))
    assert 0.3 < below < 0.7, below

    # ---- ICP, both scale modes
    source, target = (a.astype(np.float64) for a in eval_inputs.icp_case(SEED))
    for tag, opt in (("fixed", False), ("scaled", True)):
        R, t, s = quiet(ref.icp_alignment, source, target, optimize_scale=opt)
        Rr, tr, sr, its, margin, fp32_agrees = replay_icp(source, target, opt)
        assert np.allclose(Rr, R, atol=1e-12, rtol=0) and np.allclose(tr, t, atol=1e-12, rtol=0) and abs(sr - s) < 1e-12, \
            ("condition (b): the replay does not reproduce the reference", tag, np.abs(Rr - R).max(), np.abs(tr - t).max(), sr - s)
        assert margin > 1e-6, ("condition (b): a near tie between nearest and second-nearest", tag, margin)
        assert fp32_agrees, ("condition (c): an fp32 search picks another neighbour", tag)
        assert 10 <= its < 1000, (tag, its)
        print(f"icp[{tag}]: {its} iterations, smallest nearest/second margin {margin:.3e}, s = {s!r}")
        save.update({f"icp_{tag}_R": np.asarray(R), f"icp_{tag}_t": np.asarray(t), f"icp_{tag}_s": np.float64(s),
                     f"icp_{tag}_iterations": np.int64(its)})

    # ---- normalisation and alignment
    v = eval_inputs.norm_case(SEED).astype(np.float64)
    vn, center, scale = ref.normalize_mesh(types.SimpleNamespace(vertices=v))
    save.update(norm_vertices_out=vn, norm_center=center, norm_scale=np.float64(scale),
                norm_applied=ref.apply_normalization(v, center, scale),
                norm_aligned=ref.apply_icp_alignment(vn, save["icp_scaled_R"], save["icp_scaled_t"], save["icp_scaled_s"]))

    out = os.path.join(HERE, "eval_pcd.npz")
    np.savez_compressed(out, **save)
    size = os.path.getsize(out)
    assert size < 64 * 1024, size
    print(f"metric: chamfer {save['chamfer']!r} fscore {save['fscore']!r} ({below:.3f} of the distances under the threshold)")
    print(f"{out}: {size} bytes")


if __name__ == "__main__":
    main()
