"""Pre-step of the path: mesh -> the tensors Motion_Latent_Model.forward consumes.

Counterpart of the reference caller's `prepare_mesh_data` (scripts/inference_with_video_mesh.py:60-129) with
`normalize_mesh` / `sample_pointcloud_with_albedo` (utils/mesh_processing.py:130-191,194-...): unit-cube
normalisation of the vertices, area-weighted surface sampling with per-sample normal and colour, nearest-sample colour
for every vertex, and the packing into `ref_shape_pcd / ref_shape_normals / ref_shape_rgbs / ref_pcd / ref_normal /
ref_rgb / faces` ([1, n, 3] fp32, faces int64) on the device.

The reference reads the mesh with trimesh (not installable offline) and draws the samples from trimesh's sampler with
numpy's global RNG; here the mesh arrives as plain arrays and the sampler is a repo-owned counter-based one
(motion324_amd.synth's SplitMix64 stream), so a mesh + seed gives the same samples on every machine.  The arithmetic
that IS numpy in the reference -- normalisation, vertex-colour averaging, nearest-sample colours, packing -- is pinned
against the reference's own code run on a stand-in mesh (tests/golden/make_prestep_golden.py).  The nearest-sample
search is the HIP kernel m324_nearest_point (a cKDTree query on the CPU in the reference).

The sampler exists twice with one definition: sample_surface (numpy) and sample_surface_device (m324_surface_cdf +
m324_surface_sample, csrc/surface.hip), which draws the same samples for the same (mesh, num, seed), a batch of meshes per
launch, and serves the reference's third colour source, the UV texture (a Python loop per sample there;
tests/golden/make_sampler_golden.py pins it against the reference's own code).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops, synth
from .lib import M324Error


def normalize_vertices(vertices: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.float32]:
    """float32 vertices -> (vertices in [-0.5, 0.5]^3, center, scale = 2 (max |v - center| + 1e-8))
    (utils/mesh_processing.py normalize_mesh; scripts/inference_with_video_mesh.py:93-97)."""
    v = np.asarray(vertices).astype(np.float32)
    center = (v.max(axis=0) + v.min(axis=0)) / 2
    v = v - center
    v_max = np.abs(v).max()
    scale = 2 * (v_max + 1e-8)
    return v / scale, center, scale


def face_normals(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """Unit normals of the triangles (zero for degenerate ones), float64 like trimesh's."""
    tri = np.asarray(vertices, dtype=np.float64)[faces]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.maximum(ln, 1e-300), 0.0)


def sample_surface(vertices: np.ndarray, faces: np.ndarray, num: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """`num` points distributed uniformly over the surface: faces drawn with probability proportional to their area,
    uniform barycentric coordinates by reflection (the published construction trimesh.sample implements).  Returns
    (points float64 [num, 3], face index int64 [num]); deterministic in (mesh, num, seed)."""
    tri = np.asarray(vertices, dtype=np.float64)[faces]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    cum = np.cumsum(area)
    u = synth.uniform(seed, "surface.face", (num,)).astype(np.float64)
    fi = np.minimum(np.searchsorted(cum, u * cum[-1], side="right"), len(faces) - 1).astype(np.int64)
    r = synth.uniform(seed, "surface.bary", (num, 2)).astype(np.float64)
    flip = r.sum(axis=1) > 1.0
    r[flip] = 1.0 - r[flip]
    pts = tri[fi, 0] + r[:, :1] * e1[fi] + r[:, 1:] * e2[fi]
    return pts, fi


def surface_seeds(seed) -> np.ndarray:
    """int64 [B, 2]: the bit patterns of the two uint64 stream seeds (face draw, barycentric draw) of sample_surface for every
    seed of `seed` (an int or a sequence of ints) -- the table m324_surface_sample reads."""
    seeds = [int(seed)] if np.ndim(seed) == 0 else [int(s) for s in seed]
    table = np.array([[synth._stream_seed(s, "surface.face"), synth._stream_seed(s, "surface.bary")] for s in seeds], dtype=np.uint64)
    return table.reshape(len(seeds), 2).view(np.int64)


def _device_mesh(vertices, faces, device):
    """(vertices fp64 on the device, faces int32 on the device, faces_checked).  Host faces are range-checked here, before
    anything is uploaded or launched: the kernels do not check vertex indices."""
    if isinstance(vertices, torch.Tensor):
        n_vertices = vertices.shape[-2] if vertices.dim() >= 2 else 0
    else:
        vertices = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64))
        n_vertices = vertices.shape[-2] if vertices.ndim >= 2 else 0
    checked = False
    if not isinstance(faces, torch.Tensor):
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or len(faces) == 0 or not np.issubdtype(faces.dtype, np.integer):
            raise M324Error(f"surface sampling: expected non-empty integer faces [F,3], got {faces.dtype}{faces.shape}")
        if faces.min() < 0 or faces.max() >= n_vertices:
            raise M324Error(f"surface sampling: faces index vertices {faces.min()}..{faces.max()}, the mesh has {n_vertices}")
        faces = torch.from_numpy(np.ascontiguousarray(faces.astype(np.int32)))
        checked = True
    if isinstance(vertices, torch.Tensor):
        dev = torch.device(device) if device is not None else (vertices.device if vertices.is_cuda else torch.device("cuda"))
        v = vertices.detach().to(dev, torch.float64)
    else:
        dev = torch.device(device if device is not None else "cuda")
        v = torch.from_numpy(vertices).to(dev)
    return v, faces.to(dev, torch.int32), checked


def _draw_on_device(mesh, num, seed, **want) -> "ops.SurfaceSamples":
    v, f, checked = mesh
    batch = v.shape[0] if v.dim() == 3 else 1
    table = surface_seeds(seed)
    if len(table) != batch or (v.dim() == 2 and np.ndim(seed) != 0):
        raise M324Error(f"surface sampling: {len(table)} seed(s) for {batch} mesh(es)")
    seeds = torch.from_numpy(table if v.dim() == 3 else table[0]).to(v.device)
    cdf = ops.surface_cdf(v, f, faces_checked=checked)
    return ops.surface_sample(v, f, cdf, seeds, num, faces_checked=True, **want)


def sample_surface_device(vertices, faces, num: int, seed=0, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """sample_surface on the GPU (m324_surface_cdf + m324_surface_sample): the same samples for the same (mesh, num, seed).
    vertices [V,3] with an int seed, or [B,V,3] with a sequence of B seeds (one face list, one launch pair for the batch); numpy
    arrays are uploaded to `device`.  Returns device tensors (points float32 [.., num, 3], face index int64 [.., num]) -- the
    host sampler's float64 points rounded once."""
    s = _draw_on_device(_device_mesh(vertices, faces, device), num, seed)
    return s.points, s.face_index.long()


def _usable_vertex_colors(vertex_colors, n_vertices: int) -> bool:
    return vertex_colors is not None and len(vertex_colors) == n_vertices and vertex_colors.ndim == 2 and vertex_colors.shape[1] >= 3


def sample_pointcloud_with_albedo(vertices, faces, num: int, vertex_colors: Optional[np.ndarray] = None, seed: int = 0, *,
                                  uv: Optional[np.ndarray] = None, texture: Optional[np.ndarray] = None, device=None):
    """(points, normals, colours) float32 [num, 3] (utils/mesh_processing.py:130-191): face normals at the samples; the
    colour of a sample is the mean of its triangle's vertex colours (uint8 RGB(A) / 255) when the mesh has them, else 0.5
    grey.  With `device=` the draw and all three of the reference's colour sources run on the GPU (m324_surface_sample) and
    device tensors come back: vertex colours first, then the texel under the sample's interpolated UV (`uv` [V,2], `texture`
    uint8 [H,W,3|4] as the image decodes), then grey.  The host path has no texture lookup."""
    if device is None:
        if texture is not None:
            raise M324Error("sample_pointcloud_with_albedo: the texture lookup runs on the GPU only, pass device=")
        pts, fi = sample_surface(vertices, faces, num, seed)
        normals = face_normals(vertices, faces)[fi]
        if _usable_vertex_colors(vertex_colors, len(vertices)):
            vc = vertex_colors[:, :3] / 255.0
            colors = vc[faces[fi]].mean(axis=1)
        else:
            colors = np.full((num, 3), 0.5, dtype=np.float32)
        return pts.astype(np.float32), normals.astype(np.float32), colors.astype(np.float32)
    dev = torch.device(device)
    mesh = _device_mesh(vertices, faces, dev)                                # checks the faces before anything else is uploaded
    source = {}
    if _usable_vertex_colors(vertex_colors, len(vertices)):
        vc = np.asarray(vertex_colors)
        if vc.dtype != np.uint8:
            raise M324Error(f"sample_pointcloud_with_albedo: vertex colours on the device path are uint8, got {vc.dtype}")
        source["vertex_colors"] = torch.from_numpy(np.ascontiguousarray(vc[:, :4])).to(dev)
    elif texture is not None and uv is not None:
        tex = np.asarray(texture)
        if tex.dtype != np.uint8 or tex.ndim not in (2, 3):
            raise M324Error(f"sample_pointcloud_with_albedo: texture must be a uint8 image, got {tex.dtype}{tex.shape}")
        tex = np.stack([tex] * 3, axis=-1) if tex.ndim == 2 else tex[:, :, :3]
        source["texture"] = torch.from_numpy(np.ascontiguousarray(tex)).to(dev)
        source["uv"] = torch.from_numpy(np.ascontiguousarray(np.asarray(uv, dtype=np.float64))).to(dev)
    s = _draw_on_device(mesh, num, seed, want_face=False, want_normals=True, want_colors=True, **source)
    return s.points, s.normals, s.colors


def prepare_mesh_data(config, mesh: Dict[str, np.ndarray], device, seed: int = 0, sampler: str = "host"):
    """mesh: {'vertices' [V,3], 'faces' [F,3] int, 'vertex_normals' [V,3], optional 'vertex_colors' [V,3|4] uint8, optional
    'uv' [V,2] + 'texture' uint8 [H,W,3] (sampler="device" only)}.
    Returns (input_data, normalised float64 vertices, faces) -- the reference returns (input_data, mesh, faces).
    sampler="device": the shape samples are drawn on the GPU (the same samples) and stay there through the nearest-sample
    search to the packed dict."""
    if sampler not in ("host", "device"):
        raise M324Error(f"prepare_mesh_data: sampler must be 'host' or 'device', got {sampler!r}")
    tr = config.get("training", {}) if isinstance(config, dict) else getattr(config, "training", {})
    num = (tr.get("num_shape_samples", 16384) if isinstance(tr, dict) else getattr(tr, "num_shape_samples", 16384))
    raw = np.asarray(mesh["vertices"])
    faces = np.asarray(mesh["faces"]).astype(np.int64)
    vertex_normals = np.asarray(mesh["vertex_normals"]).astype(np.float32)
    vertices, center, scale = normalize_vertices(raw)                       # float32 chain (ref_pcd)
    mesh_vertices = (raw.astype(np.float64) - center) / scale               # the mesh itself, float64 chain (samples)
    dev = torch.device(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None].float().to(dev)
    if sampler == "device":
        samples_dev, nrm_dev, rgb_dev = sample_pointcloud_with_albedo(mesh_vertices, faces, num, mesh.get("vertex_colors"), seed,
                                                                      uv=mesh.get("uv"), texture=mesh.get("texture"), device=dev)
        shape_pcd, shape_normals, shape_rgbs = samples_dev[None], nrm_dev[None], rgb_dev[None]
    else:
        xyz, nrm, rgb = sample_pointcloud_with_albedo(mesh_vertices, faces, num, mesh.get("vertex_colors"), seed)
        samples_dev = torch.from_numpy(xyz).to(dev)
        rgb_dev = torch.from_numpy(rgb).to(dev)
        shape_pcd, shape_normals, shape_rgbs = t(xyz), t(nrm), t(rgb)
    verts_dev = torch.from_numpy(vertices).to(dev)
    nearest = ops.nearest_point(verts_dev, samples_dev)                     # scripts/inference_with_video_mesh.py:112-115
    input_data = {
        "ref_shape_pcd": shape_pcd, "ref_shape_normals": shape_normals, "ref_shape_rgbs": shape_rgbs,
        "ref_pcd": verts_dev[None].float(), "ref_normal": t(vertex_normals), "ref_rgb": rgb_dev[nearest][None].float(),
        "faces": torch.from_numpy(faces)[None].long().to(dev),
    }
    return input_data, mesh_vertices, faces
