"""Deterministic inputs of the geometry-evaluation tests (tests/test_eval_cpu.py, tests/test_eval_gpu.py) and of the golden
maker tests/golden/make_eval_golden.py: functions of a seed through motion324_amd.synth, rounded to fp32 so that the
reference's fp64 code and the fp32 kernels see the same numbers.  tests/golden/eval_pcd.npz stores seeds, sizes and the
reference's outputs only; the inputs are regenerated from here."""
import numpy as np

from motion324_amd import synth

ICP_SOURCE, ICP_TARGET = 700, 1500
METRIC_POINTS = 2048
NORM_VERTICES = 300


def _directions(seed, key, n):
    g = synth.normal(seed, key, (n, 3)).astype(np.float64)
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def _blob(d, wobble):
    """a bumpy ellipsoid of about unit size, sampled along the directions d"""
    r = 1.0 + 0.10 * np.sin(4.0 * d[:, 0]) * np.cos(3.0 * d[:, 1]) + wobble * np.cos(5.0 * d[:, 2] + 1.0)
    return d * np.array([0.9, 0.6, 0.5]) * r[:, None]


def _rotation(deg_z, deg_x):
    a, b = np.deg2rad(deg_z), np.deg2rad(deg_x)
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    return rz @ rx


def icp_case(seed):
    """(source [700,3], target [1500,3]) fp32: two samplings of related shapes (3 % of shape difference), the source rotated
    by a few degrees and shifted, so that ICP needs tens of iterations."""
    target = _blob(_directions(seed, "eval.icp.target", ICP_TARGET), 0.0)
    source = _blob(_directions(seed, "eval.icp.source", ICP_SOURCE), 0.03) @ _rotation(4.0, 3.0).T + np.array([0.03, -0.02, 0.01])
    return source.astype(np.float32), target.astype(np.float32)


def metric_case(seed):
    """(points1, points2) fp32 [2048,3]: two samplings of nearly the same surface of about 0.7 x 0.5 x 0.4 -- the typical spacing makes
    roughly half of the nearest distances fall under 0.02, and every one stays below 0.2."""
    p1 = 0.8 * _blob(_directions(seed, "eval.metric.1", METRIC_POINTS), 0.0)
    p2 = 0.8 * _blob(_directions(seed, "eval.metric.2", METRIC_POINTS), 0.004)
    return p1.astype(np.float32), p2.astype(np.float32)


def norm_case(seed):
    """vertices [300,3] fp32 of an off-centre, anisotropic blob (what normalize_points sees)"""
    v = 3.0 * _blob(_directions(seed, "eval.norm", NORM_VERTICES), 0.02) + np.array([2.0, -1.0, 0.25])
    return v.astype(np.float32)
