"""Geometry evaluation of a predicted 4D mesh on the GPU: Chamfer distance, F-score, voxel IoU and ICP alignment
(reference evaluation/evaluation_pcd.py).

Everything expensive in the reference is a cKDTree nearest-neighbour query on the CPU: one per ICP iteration (up to 1000
iterations), two per frame for the metrics.  Here every query is m324_nn_search (brute force in fp32, csrc/geometry.hip), the
reductions behind it are m324_dist_stats / m324_icp_moments (fp64, deterministic), and all frames of a sequence go through
batched launches.  Same function names, argument defaults and return conventions as the reference; arrays or tensors where
the reference takes trimesh objects.  What stays on the host: the 3x3 SVDs of ICP (numpy), file I/O and, by default, surface
sampling (preprocess.sample_surface; sampler="device" / --sampler device draws the same samples with m324_surface_sample).

The voxel IoU (compute_iou_voxel, which the reference defines and leaves commented out) voxelises both meshes exactly with
m324_voxelize and counts with m324_voxel_counts (csrc/voxel.hip): integers throughout, the quotient formed here.

    python -m motion324_amd.evaluation --gt_path GT_DIR --pred_path PRED_DIR [--num_samples 50000] [--seed 0] [--sampler device]
                                       [--iou [--iou_resolution 128] [--iou_half 2] [--iou_fill none|orthographic]]

reads two directories in the reference's layout (faces.npy, frame_0000.npy, frame_0001.npy, ...).
"""
from __future__ import annotations

import argparse
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops, preprocess
from .lib import M324Error

ICP_TARGET_SAMPLES = 10000          # evaluation_pcd.py:538
_LAYOUT = "a directory holding faces.npy and frame_0000.npy, frame_0001.npy, ..."


def _is_tensor(x) -> bool:
    return isinstance(x, torch.Tensor)


def _host64(x) -> np.ndarray:
    if _is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def _device32(x, device=None) -> torch.Tensor:
    """fp32 points on a HIP device (numpy input is uploaded to `device`, default the current one)"""
    if _is_tensor(x):
        if not x.is_cuda:
            raise M324Error("evaluation: tensors must live on a HIP device (pass numpy arrays for host data)")
        return x.detach().to(torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(device or "cuda")


def _params(s: float, R: np.ndarray, t: np.ndarray, device) -> torch.Tensor:
    """the 13 doubles m324_transform_points / m324_icp_moments read: one upload"""
    host = np.concatenate([[float(s)], np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)])
    return torch.from_numpy(host).to(device)


# ------------------------------------------------------------------------------------------------ normalisation
def normalize_points(vertices):
    """CUBE normalisation (evaluation_pcd.py:171-194, normalize_mesh): centre of the bounding box to the origin, largest
    extent to 2.  Returns (normalised vertices, center, scale) with normalised = (vertices - center) / scale.  The parameters
    are fp64 numpy; numpy vertices give fp64 numpy (the reference's arithmetic), device tensors give an fp32 device tensor."""
    v = _host64(vertices)
    bbox_min = v.min(axis=0)
    bbox_max = v.max(axis=0)
    offset = -(bbox_min + bbox_max) / 2
    center = -offset
    scale = 2.0 / np.max(bbox_max - bbox_min)
    if _is_tensor(vertices):
        return apply_normalization(vertices, center, 1.0 / scale), center, 1.0 / scale
    return (v + offset) * scale, center, 1.0 / scale


def apply_normalization(vertices, center, scale):
    """(vertices - center) / scale (evaluation_pcd.py:196-198)."""
    if _is_tensor(vertices):
        inv = 1.0 / float(scale)
        x = _device32(vertices)
        return ops.transform_points(x, _params(inv, np.eye(3), -np.asarray(center, dtype=np.float64) * inv, x.device))
    return (_host64(vertices) - center) / scale


def apply_icp_alignment(vertices, R, t, s):
    """s * (vertices @ R.T) + t (evaluation_pcd.py:200-202)."""
    if _is_tensor(vertices):
        x = _device32(vertices)
        return ops.transform_points(x, _params(float(s), R, t, x.device))
    return s * (_host64(vertices) @ R.T) + t


# ------------------------------------------------------------------------------------------------ metrics
def _metric_sums(points1, points2, threshold: float):
    """per frame: (sum and count<threshold of the distances of points2 to points1, the same of points1 to points2, n1, n2)"""
    p1 = _device32(points1)
    p2 = _device32(points2, p1.device)
    if p1.dim() != p2.dim() or p1.dim() not in (2, 3):
        raise M324Error(f"evaluation: expected two [n,3] or two [T,n,3] point sets, got {tuple(p1.shape)} / {tuple(p2.shape)}")
    dist1 = ops.nn_search(p2, p1)                       # tree1.query(points2)
    dist2 = ops.nn_search(p1, p2)                       # tree2.query(points1)
    sum1, cnt1 = ops.dist_stats(dist1, threshold)
    sum2, cnt2 = ops.dist_stats(dist2, threshold)
    host = torch.stack([sum1.reshape(-1), cnt1.reshape(-1).double(), sum2.reshape(-1), cnt2.reshape(-1).double()]).cpu().numpy()
    return host, p1.shape[-2], p2.shape[-2], p1.dim() == 3, p1.device


def _chamfer(host, n1, n2):
    return host[0] / n2 + host[2] / n1                  # np.mean(dist1) + np.mean(dist2), unsquared distances


def _fscore(host, n1, n2):
    precision, recall = host[1] / n2, host[3] / n1
    total = precision + recall
    return np.where(total == 0, 0.0, 2 * precision * recall / np.where(total == 0, 1.0, total))


def _shaped(values: np.ndarray, batched: bool, device):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(device) if batched else float(values[0])


def compute_chamfer_distance(points1, points2):
    """Bidirectional Chamfer distance, mean(d(points2 -> points1)) + mean(d(points1 -> points2)) of unsquared distances
    (evaluation_pcd.py:575-588).  [n,3] inputs give a float, [T,n,3] inputs a [T] fp64 tensor."""
    host, n1, n2, batched, device = _metric_sums(points1, points2, 0.0)
    return _shaped(_chamfer(host, n1, n2), batched, device)


def compute_fscore(points1, points2, threshold=0.02):
    """F-score at `threshold` (evaluation_pcd.py:591-609): precision from the distances of points2 to points1, recall the
    other way round, both with `<`; 0.0 when both are 0."""
    host, n1, n2, batched, device = _metric_sums(points1, points2, threshold)
    return _shaped(_fscore(host, n1, n2), batched, device)


def chamfer_and_fscore(points1, points2, threshold=0.02):
    """(compute_chamfer_distance, compute_fscore) from one pair of searches."""
    host, n1, n2, batched, device = _metric_sums(points1, points2, threshold)
    return _shaped(_chamfer(host, n1, n2), batched, device), _shaped(_fscore(host, n1, n2), batched, device)


# ------------------------------------------------------------------------------------------------ voxel IoU
VOXEL_FILLS = ("none", "orthographic")


def _voxel_shapes(vertices, faces, name: str):
    """(frames, vertices, faces, whether the caller gave one frame) of a mesh or clip: every refusal that needs shapes, dtypes
    and host data alone, before any copy or launch"""
    vs = tuple(vertices.shape) if hasattr(vertices, "shape") else np.shape(vertices)
    fs = tuple(faces.shape) if hasattr(faces, "shape") else np.shape(faces)
    if len(vs) not in (2, 3) or vs[-1] != 3 or 0 in vs:
        raise M324Error(f"{name}: expected vertices [V,3] or [T,V,3], got {tuple(vs)}")
    if len(fs) != 2 or fs[1] != 3:
        raise M324Error(f"{name}: expected faces [F,3], got {tuple(fs)}")
    kind = faces.dtype if hasattr(faces, "dtype") else np.asarray(faces).dtype
    if "int" not in str(kind):
        raise M324Error(f"{name}: faces are integers, got {kind}")
    if not _is_tensor(faces) and fs[0] and (np.min(faces) < 0 or np.max(faces) >= vs[-2]):
        raise M324Error(f"{name}: faces index vertices {int(np.min(faces))}..{int(np.max(faces))}, the mesh has {vs[-2]}")
    return (1 if len(vs) == 2 else vs[0]), vs[-2], fs[0], len(vs) == 2


def _voxel_upload(vertices, faces, device, name: str):
    """(fp32 device clip [T,V,3], int32 device faces [F,3]) after _voxel_shapes; a host array goes only to a device the caller
    named, and the range of faces that were on a device already is checked here (one reduction and a sync)"""
    def up(x, dtype):
        if _is_tensor(x) and x.is_cuda:
            return x.detach() if x.dtype == dtype else x.detach().to(dtype)
        if device is None:
            raise M324Error(f"{name}: a host array needs device= (the voxeliser runs on the GPU; there is no host path)")
        t = x if _is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=device, dtype=dtype)
    v = up(vertices, torch.float32)
    f = up(faces, torch.int32).contiguous()
    v = v if v.dim() == 3 else v[None]
    if f.shape[0] and _is_tensor(faces):
        ops._faces_in_range(f, v.shape[1], name)
    return v, f


def _voxel_chunk(frames: int, n_vertices: int, n_faces: int, resolution: int, half: int, grids: int, max_scratch_bytes: int, name: str) -> int:
    """frames per call so that `grids` grids of a chunk plus the voxeliser's scratch stay under max_scratch_bytes"""
    side = ops.voxel_side(resolution, half)
    frame = side * side * side // 8

    def need(n):
        return grids * n * frame + ops.voxel_plan(n_vertices, n_faces, n, resolution, half)
    if need(1) > max_scratch_bytes:
        raise M324Error(f"{name}: one frame needs {need(1)} bytes ({grids} grids of side {side} and the scratch), max_scratch_bytes is {max_scratch_bytes}")
    chunk = max(1, min(frames, 65535, int(max_scratch_bytes) // need(1)))
    while chunk > 1 and (chunk * max(n_faces, 1) >= 2 ** 31 - 1 or chunk * n_vertices >= 2 ** 31 - 1 or need(chunk) > max_scratch_bytes):
        chunk -= 1
    return chunk


def _check_fill(fill, name: str) -> None:
    if fill not in VOXEL_FILLS:
        raise M324Error(f"{name}: fill must be one of {VOXEL_FILLS}, got {fill!r}")


def voxelize_clip(vertices, faces, resolution=128, half=2, fill="none", max_scratch_bytes=1 << 30, device=None):
    """Occupancy grids of a mesh clip: vertices [V,3] or [T,V,3] (a device tensor, or numpy with `device`), faces int [F,3] ->
    (grid int32 [T,G,G,G/32], outside int32 [T]) over [-half, half)^3 at `resolution` voxels per unit, G = 2 * half * resolution
    (bit layout: include/m324.h; unpack_voxels gives booleans).  Exact closed-cube overlap of every triangle; fill="orthographic"
    also sets the voxels with surface on both sides along x, y and z (ops.voxel_fill).  outside[t] counts vertices of frame t
    beyond the grid: their triangles are clipped, not refused.  The result is allocated once; the frames go through in chunks so
    that two grids of a chunk (the fill's temporary is the second) plus the scratch stay under max_scratch_bytes."""
    _check_fill(fill, "voxelize_clip")
    side = ops.voxel_side(resolution, half)
    T, nv, nf, _ = _voxel_shapes(vertices, faces, "voxelize_clip")
    chunk = _voxel_chunk(T, nv, nf, resolution, half, 2, max_scratch_bytes, "voxelize_clip")
    v, f = _voxel_upload(vertices, faces, device, "voxelize_clip")
    grid = torch.empty((T, side, side, side // 32), dtype=torch.int32, device=v.device)
    outside = torch.empty((T,), dtype=torch.int32, device=v.device)
    scratch = torch.empty((ops.voxel_plan(nv, nf, chunk, resolution, half),), dtype=torch.uint8, device=v.device)
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        part = grid[t0:t1]
        _, out = ops.voxelize(v[t0:t1], f, resolution, half, scratch=scratch, out=part, faces_checked=True)
        outside[t0:t1] = out
        if fill == "orthographic":
            ops.voxel_fill(part, out=part)
    return grid, outside


def unpack_voxels(grid) -> torch.Tensor:
    """bool [T,G,G,G] indexed [t, k, j, i] (z, y, x: the grid's own order) of an int32 grid [T,G,G,G/32]"""
    if not _is_tensor(grid) or grid.dtype != torch.int32 or grid.dim() != 4 or grid.shape[1] != grid.shape[2] or grid.shape[1] != 32 * grid.shape[3]:
        raise M324Error(f"unpack_voxels: expected an int32 grid [T,G,G,G/32], got {tuple(grid.shape) if _is_tensor(grid) else type(grid).__name__}")
    bits = torch.arange(32, dtype=torch.int32, device=grid.device)
    return ((grid[..., None] >> bits) & 1).bool().reshape(grid.shape[0], grid.shape[1], grid.shape[2], grid.shape[1])


def _iou_of_counts(counts: np.ndarray) -> np.ndarray:
    """[T,3] integer (|A|, |B|, |A & B|) -> fp64 intersection / union, 0.0 where the union is empty (evaluation_pcd.py:631-637)"""
    inter = counts[:, 2].astype(np.float64)
    union = (counts[:, 0] + counts[:, 1] - counts[:, 2]).astype(np.float64)
    return np.where(union == 0, 0.0, inter / np.where(union == 0, 1.0, union))


def _iou_chunk(frames, mesh1, mesh2, resolution, half, fill, max_scratch_bytes, name) -> int:
    """frames per round of _iou_clips for two meshes (n_vertices, n_faces): the two grids of a chunk, a third while one is
    filled, and the scratch stay under max_scratch_bytes"""
    grids = 3 if fill == "orthographic" else 2
    return min(_voxel_chunk(frames, nv, nf, resolution, half, grids, max_scratch_bytes, name) for nv, nf in (mesh1, mesh2))


def _iou_clips(v1, f1, v2, f2, resolution, half, fill, chunk):
    """(iou fp64 [T], outside int64 [T,2]) of two device clips with the same number of frames, `chunk` frames at a time; the
    faces are range-checked already"""
    T = v1.shape[0]
    counts, outside = [], []
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        sides = []
        for v, f in ((v1, f1), (v2, f2)):
            grid, out = ops.voxelize(v[t0:t1], f, resolution, half, faces_checked=True)
            sides.append((ops.voxel_fill(grid) if fill == "orthographic" else grid, out))
        counts.append(ops.voxel_counts(sides[0][0], sides[1][0]))
        outside.append(torch.stack([sides[0][1], sides[1][1]], dim=1))
    return _iou_of_counts(torch.cat(counts).cpu().numpy()), torch.cat(outside).cpu().numpy().astype(np.int64)


def compute_iou_voxel(vertices1, faces1, vertices2, faces2, resolution=128, half=2, fill="none", device=None, max_scratch_bytes=1 << 30):
    """Voxel IoU of two meshes (evaluation_pcd.py:612-637, which the reference leaves commented out: trimesh's voxeliser is too
    slow for a clip): both meshes are voxelised over [-half, half)^3 at pitch 1 / resolution (voxelize_clip's grids), IoU =
    |A & B| / |A | B| from integer counts, 0.0 when both grids are empty.  [V,3] inputs give a float, [T,V,3] inputs a [T] fp64
    tensor; device tensors, or numpy with `device`.  Unlike the reference both grids share world coordinates (it aligns each
    grid at its own lower corner), occupancy is the exact overlap of triangle and closed voxel cube (not subdivide-and-round),
    and the default is the surface shell as there; fill="orthographic" compares solids.  Geometry beyond the grid is clipped
    silently here: voxelize_clip reports it."""
    name = "compute_iou_voxel"
    _check_fill(fill, name)
    ops.voxel_side(resolution, half)
    T1, nv1, nf1, single1 = _voxel_shapes(vertices1, faces1, name)
    T2, nv2, nf2, single2 = _voxel_shapes(vertices2, faces2, name)
    if single1 != single2 or T1 != T2:
        raise M324Error(f"{name}: expected two [V,3] meshes or two clips of one length, got {T1} and {T2} frame(s)")
    chunk = _iou_chunk(T1, (nv1, nf1), (nv2, nf2), resolution, half, fill, max_scratch_bytes, name)
    v1, f1 = _voxel_upload(vertices1, faces1, device, name)
    v2, f2 = _voxel_upload(vertices2, faces2, device if device is not None else v1.device, name)
    if v1.device != v2.device:
        raise M324Error(f"{name}: the two meshes live on different devices")
    iou, _ = _iou_clips(v1, f1, v2, f2, resolution, half, fill, chunk)
    return _shaped(iou, not single1, v1.device)


# ------------------------------------------------------------------------------------------------ ICP
def icp_alignment(source_points, target_points, max_iterations=1000, tolerance=1e-7, optimize_scale=False):
    """Point-to-point ICP of source onto target (evaluation_pcd.py:205-408, step by step).  Returns fp64 numpy (R, t) and the
    scale s with aligned = s * (source @ R.T) + t.  Per iteration the device runs transform -> nearest-neighbour search ->
    moment sums; the host gets one 32-double record, does the two 3x3 SVDs with numpy and uploads 13 doubles."""
    source, target = _host64(source_points), _host64(target_points)
    src = _device32(source_points)
    tgt = _device32(target_points, src.device)
    if src.dim() != 2 or tgt.dim() != 2:
        raise M324Error(f"icp_alignment: expected [n,3] point sets, got {tuple(src.shape)} / {tuple(tgt.shape)}")

    source_max_range = np.max((np.max(source, axis=0) - np.min(source, axis=0))[:2])          # x and y extents only
    target_max_range = np.max((np.max(target, axis=0) - np.min(target, axis=0))[:2])
    scale = float(np.clip(target_max_range / source_max_range, 0.95, 1.05)) if source_max_range > 1e-10 else 1.0

    R = np.eye(3)
    t = np.zeros(3)
    prev_error = float("inf")
    for _ in range(int(max_iterations)):
        params = _params(scale, R, t, src.device)
        moved = ops.transform_points(src, params)
        index = ops.nn_search(moved, tgt, want_dist=False, want_index=True)
        rec = ops.icp_moments(src, params, tgt, index).cpu().numpy()
        if not np.all(np.isfinite(rec)):
            raise M324Error("icp_alignment: non-finite moment sums (non-finite input points?)")
        n = rec[0]
        error = rec[1] / n                                          # mean distance BEFORE the update
        if abs(prev_error - error) < tolerance:
            break
        prev_error = error

        source_centroid, target_centroid = rec[2:5] / n, rec[5:8] / n
        H = rec[8:17].reshape(3, 3) - n * np.outer(source_centroid, target_centroid)           # centred covariance
        U, _, Vt = np.linalg.svd(H)
        R_delta = Vt.T @ U.T
        if np.linalg.det(R_delta) < 0:                              # reflection fix
            Vt[-1, :] *= -1
            R_delta = Vt.T @ U.T
        t_delta = target_centroid - source_centroid @ R_delta.T
        R = R @ R_delta
        t = t @ R_delta.T + t_delta
        U, _, Vt = np.linalg.svd(R)                                 # re-orthogonalise
        R = U @ Vt

        if optimize_scale:
            # sum(m . (R x + t)) and sum(|R x + t|^2) over the matched pairs, from the moments of the untransformed source
            sum_m, sum_x, x_m, x_x = rec[5:8], rec[17:20], rec[20:29].reshape(3, 3), rec[29]
            numerator = np.sum(R * x_m.T) + t @ sum_m
            denominator = x_x + 2.0 * (t @ (R @ sum_x)) + n * (t @ t)
            if denominator > 1e-10:
                scale_new = np.clip(numerator / denominator, 0.95, 1.05)
                scale = float(np.clip(0.8 * scale + 0.2 * scale_new, 0.95, 1.05))
    return R, t, scale


# ------------------------------------------------------------------------------------------------ sequences
def sample_seed(seed: int, side: int, frame: int) -> int:
    """The seed of preprocess.sample_surface for one (side, frame): side 0 = ground truth, 1 = prediction; frame -1 = the
    ICP target samples of ground-truth frame 0.  Distinct for every (side, frame) below 65535 frames."""
    return (int(seed) * 2 + int(side)) * 65536 + int(frame) + 1


def evaluate_sequence(gt_vertices, gt_faces, pred_vertices, pred_faces, num_samples=2048, seed=0, threshold=0.02, alignment=None,
                      sampler="host", iou_resolution=None, iou_half=2, iou_fill="none"):
    """Per-frame Chamfer distance and F-score of a predicted mesh sequence against ground truth (evaluation_pcd.py:746-916):
    normalisation parameters from frame 0 of each side; ICP of the normalised predicted frame-0 vertices onto 10 000 surface
    samples of the normalised ground-truth frame 0 (skipped when alignment=(R, t, s) is given); per frame the ground truth is
    normalised and aligned, the prediction normalised, `num_samples` surface points drawn from each, and both metrics computed
    -- all frames in batched launches.  A shorter ground-truth sequence repeats its last frame.
    sampler="device" draws the per-frame samples on the GPU (preprocess.sample_surface_device: the same samples; one CDF and one
    sample launch per side for all frames) and hands them to the metrics without a round trip through the host; the per-frame
    transforms stay the fp64 host arithmetic, and the ICP target samples stay on the host sampler.
    iou_resolution (None: off) adds the voxel IoU of every frame (compute_iou_voxel's arithmetic) between the aligned ground truth
    and the normalised prediction -- the vertices the samplers get, uploaded once as fp32 -- on a grid over [-iou_half, iou_half)^3
    with iou_fill.  Frame 0 spans [-1, 1] after normalisation; later frames and the ICP move geometry past that, hence
    iou_half=2.  A frame with vertices beyond the grid raises instead of scoring clipped geometry.
    Returns {'chamfer_distances': [...], 'fscores': [...], 'R', 't', 's'}, and 'ious': [...] with iou_resolution."""
    if sampler not in ("host", "device"):
        raise M324Error(f"evaluate_sequence: sampler must be 'host' or 'device', got {sampler!r}")
    if iou_resolution is not None:
        _check_fill(iou_fill, "evaluate_sequence: iou_fill")
        ops.voxel_side(iou_resolution, iou_half)
    gt, pred = _host64(gt_vertices), _host64(pred_vertices)
    gt_faces, pred_faces = np.asarray(gt_faces), np.asarray(pred_faces)
    if gt.ndim != 3 or pred.ndim != 3 or gt.shape[2] != 3 or pred.shape[2] != 3 or len(gt) == 0 or len(pred) == 0:
        raise M324Error(f"evaluate_sequence: expected [T,V,3] vertices, got {gt.shape} / {pred.shape}")
    num_frames = len(pred)
    if len(gt) < num_frames:
        gt = np.concatenate([gt, np.repeat(gt[-1:], num_frames - len(gt), axis=0)])

    _, pred_center, pred_scale = normalize_points(pred[0])
    _, gt_center, gt_scale = normalize_points(gt[0])
    if alignment is None:
        gt_sampled, _ = preprocess.sample_surface(gt[0], gt_faces, ICP_TARGET_SAMPLES, sample_seed(seed, 0, -1))
        R, t, s = icp_alignment(apply_normalization(pred[0], pred_center, pred_scale), (gt_sampled - gt_center) / gt_scale)
    else:
        R, t, s = alignment
        R, t, s = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64), float(s)

    if sampler == "device":
        gt_aligned = np.stack([apply_icp_alignment(apply_normalization(gt[f], gt_center, gt_scale), R, t, s) for f in range(num_frames)])
        pred_norm = np.stack([apply_normalization(pred[f], pred_center, pred_scale) for f in range(num_frames)])
        gt_points, _ = preprocess.sample_surface_device(gt_aligned, gt_faces, num_samples, [sample_seed(seed, 0, f) for f in range(num_frames)])
        pred_points, _ = preprocess.sample_surface_device(pred_norm, pred_faces, num_samples, [sample_seed(seed, 1, f) for f in range(num_frames)],
                                                          gt_points.device)
    else:
        gt_points = np.empty((num_frames, num_samples, 3), dtype=np.float32)
        pred_points = np.empty((num_frames, num_samples, 3), dtype=np.float32)
        keep = iou_resolution is not None
        gt_kept, pred_kept = [], []
        for f in range(num_frames):
            gt_aligned = apply_icp_alignment(apply_normalization(gt[f], gt_center, gt_scale), R, t, s)
            gt_points[f] = preprocess.sample_surface(gt_aligned, gt_faces, num_samples, sample_seed(seed, 0, f))[0]
            pred_norm = apply_normalization(pred[f], pred_center, pred_scale)
            pred_points[f] = preprocess.sample_surface(pred_norm, pred_faces, num_samples, sample_seed(seed, 1, f))[0]
            if keep:
                gt_kept.append(gt_aligned.astype(np.float32))
                pred_kept.append(pred_norm.astype(np.float32))
        if keep:
            gt_aligned, pred_norm = np.stack(gt_kept), np.stack(pred_kept)
    chamfer, fscore = chamfer_and_fscore(gt_points, pred_points, threshold)
    results = {"chamfer_distances": [float(c) for c in chamfer.cpu()], "fscores": [float(v) for v in fscore.cpu()], "R": R, "t": t, "s": s}
    if iou_resolution is not None:
        name, device = "evaluate_sequence", chamfer.device
        chunk = _iou_chunk(num_frames, _voxel_shapes(gt_aligned, gt_faces, name)[1:3], _voxel_shapes(pred_norm, pred_faces, name)[1:3], iou_resolution,
                           iou_half, iou_fill, 1 << 30, name)
        v1, f1 = _voxel_upload(gt_aligned, gt_faces, device, name)
        v2, f2 = _voxel_upload(pred_norm, pred_faces, device, name)
        iou, outside = _iou_clips(v1, f1, v2, f2, iou_resolution, iou_half, iou_fill, chunk)
        if outside.any():
            frame = int(np.argmax(outside.sum(axis=1) > 0))
            raise M324Error(f"evaluate_sequence: frame {frame} has {int(outside[frame, 0])} ground-truth and {int(outside[frame, 1])} predicted vertices "
                            f"beyond the voxel grid [-{int(iou_half)}, {int(iou_half)})^3: raise iou_half (the grid side is 2 * iou_half * iou_resolution)")
        results["ious"] = [float(v) for v in iou]
    return results


# ------------------------------------------------------------------------------------------------ directory layer and CLI (host only)
def load_sequence_dir(path) -> Tuple[np.ndarray, np.ndarray]:
    """(vertices [T,V,3], faces [F,3]) of a directory in the reference's layout (evaluation_pcd.py:70-75, :762-769)."""
    path = os.fspath(path)
    if not os.path.isdir(path):
        raise M324Error(f"{path}: expected {_LAYOUT} (GLB / FBX files are not read here: export the frames first)")
    names = sorted(n for n in os.listdir(path) if n.startswith("frame_") and n.endswith(".npy"))
    if not names or not os.path.exists(os.path.join(path, "faces.npy")):
        raise M324Error(f"{path}: expected {_LAYOUT}")
    return np.stack([np.load(os.path.join(path, n)) for n in names]), np.load(os.path.join(path, "faces.npy"))


def write_results(gt_path, results) -> Tuple[str, Optional[str]]:
    """evaluation_results.txt in the reference's three-line format (evaluation_pcd.py:902-909) and, when the results carry
    an alignment, icp_alignment_params.npz (R, t, s; :562-563), both in the ground-truth directory.  Returns the two paths."""
    gt_path = os.fspath(gt_path)
    os.makedirs(gt_path, exist_ok=True)
    txt = os.path.join(gt_path, "evaluation_results.txt")
    with open(txt, "w") as f:
        f.write(f"{os.path.basename(os.path.normpath(gt_path))}\n")
        f.write(f"cd_mean_{np.mean(results['chamfer_distances']):.6f}\n")
        f.write(f"fs_mean_{np.mean(results['fscores']):.6f}\n")
        if "ious" in results:
            f.write(f"iou_mean_{np.mean(results['ious']):.6f}\n")
    npz = None
    if "R" in results:
        npz = os.path.join(gt_path, "icp_alignment_params.npz")
        np.savez(npz, R=results["R"], t=results["t"], s=results["s"])
    return txt, npz


def main(argv=None) -> dict:
    parser = argparse.ArgumentParser(description="Evaluate mesh reconstruction quality (Chamfer distance, F-score) on the GPU")
    parser.add_argument("--gt_path", type=str, required=True, help="ground-truth directory (faces.npy and frame_*.npy)")
    parser.add_argument("--pred_path", type=str, required=True, help="predicted directory (faces.npy and frame_*.npy)")
    parser.add_argument("--num_samples", type=int, default=50000, help="points sampled from each mesh")
    parser.add_argument("--seed", type=int, default=0, help="seed of the surface samples")
    parser.add_argument("--sampler", choices=("host", "device"), default="host", help="where the surface samples are drawn (same samples)")
    parser.add_argument("--iou", action="store_true", help="also score the voxel IoU of every frame")
    parser.add_argument("--iou_resolution", type=int, default=128, help="voxels per unit length of the IoU grid (a multiple of 16)")
    parser.add_argument("--iou_half", type=int, default=2, help="the IoU grid covers [-iou_half, iou_half)^3 of the normalised space")
    parser.add_argument("--iou_fill", choices=VOXEL_FILLS, default="none", help="compare surface shells (none) or orthographically filled solids")
    args = parser.parse_args(argv)
    gt_vertices, gt_faces = load_sequence_dir(args.gt_path)
    pred_vertices, pred_faces = load_sequence_dir(args.pred_path)
    results = evaluate_sequence(gt_vertices, gt_faces, pred_vertices, pred_faces, num_samples=args.num_samples, seed=args.seed,
                                sampler=args.sampler, iou_resolution=args.iou_resolution if args.iou else None, iou_half=args.iou_half,
                                iou_fill=args.iou_fill)
    for f, (cd, fs) in enumerate(zip(results["chamfer_distances"], results["fscores"])):
        print(f"Frame {f} - Chamfer: {cd:.6f}, F-score: {fs:.4f}" + (f", IoU: {results['ious'][f]:.4f}" if "ious" in results else ""))
    print(f"Chamfer Distance - Mean: {np.mean(results['chamfer_distances']):.6f}, Std: {np.std(results['chamfer_distances']):.6f}")
    print(f"F-score - Mean: {np.mean(results['fscores']):.4f}, Std: {np.std(results['fscores']):.4f}")
    if "ious" in results:
        print(f"IoU - Mean: {np.mean(results['ious']):.4f}, Std: {np.std(results['ious']):.4f}")
    txt, _ = write_results(args.gt_path, results)
    print(f"Results saved to {txt}")
    return results


if __name__ == "__main__":
    main()
