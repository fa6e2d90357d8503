"""Mesh clip -> training sample: the GPU-shaped part of the reference's dataset (dataset/dataset_utils.py:44-136
`track_with_normal_rgb`, called twice per sample by dataset/dyscene.py:266-300).

A clip is a deforming mesh: vertex positions [T, V, 3] over one face list.  Samples are drawn area-weighted on frame 0, keep their
face and barycentric weights, and are carried through every frame with interpolated, renormalised vertex normals and one colour
looked up through per-corner UVs.  The reference does this on dataloader workers with trimesh, rebuilding the vertex normals
with sparse products once per frame and call; here the path exists twice with one definition (include/m324.h, "Tracked surface
samples"):

  * device=None: numpy, fp64, the expression order of the header.  It is the definition, as preprocess.sample_surface is for
    the sampler whose draw it uses.
  * device=...: m324_surface_cdf + m324_vertex_normals + m324_surface_track (csrc/surface.hip).  Points, face indices and colours
    equal the host path bit for bit; normals differ only by the rounding of fp64 acos.

trimesh is not a dependency, so `init_mesh` is gone from the signature (frame 0 of `vertex_frames` is the initial mesh) and the
draw is the repository's seeded sampler, not trimesh's global-RNG one.  Host-side by design: the vertex-corner table (topology
only, built once per face list), the range check of the faces, the seeds.  Image loading, camera choice and the frame-index
policy of the dataset are the caller's.
"""
from __future__ import annotations

import weakref
from collections import OrderedDict
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import ops, preprocess, synth
from .lib import M324Error

SAMPLE_KEYS = ("rgb_video", "point_clouds", "point_rgbs", "ref_shape_pcd", "ref_shape_normals", "ref_shape_rgbs", "ref_pcd", "ref_normal",
               "ref_rgb")
_WEIGHTINGS = ("angle", "area")


# ------------------------------------------------------------------------------------------------ host path (the definition)
def vertex_corners(faces: np.ndarray, n_vertices: int) -> Tuple[np.ndarray, np.ndarray]:
    """(corner_offsets int64 [V+1], corner_list int64 [3F]): for vertex v the corners 3 f + k with faces[f][k] == v, ascending
    (a stable counting sort of the corners by vertex)."""
    flat = np.asarray(faces).reshape(-1)
    offsets = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=n_vertices), out=offsets[1:])
    return offsets, np.argsort(flat, kind="stable").astype(np.int64)


def _norm3(a: np.ndarray) -> np.ndarray:
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def _dot3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def vertex_normals(vertices: np.ndarray, faces: np.ndarray, corners=None, weighting: str = "angle") -> np.ndarray:
    """Unit vertex normals, fp64 [..., V, 3], of every pose in `vertices` [..., V, 3]: per corner the face's unit normal times
    its angle at the corner (or half its |e1 x e2|), added per vertex one after the other in ascending corner order, then
    normalised; exactly 0 where the sum has no length.  Faces without area contribute nothing."""
    if weighting not in _WEIGHTINGS:
        raise M324Error(f"vertex_normals: weighting must be one of {_WEIGHTINGS}, got {weighting!r}")
    v = np.asarray(vertices, dtype=np.float64)
    shape = v.shape
    v = v.reshape(-1, shape[-2], 3)
    faces = np.asarray(faces)
    nv, nf = shape[-2], len(faces)
    offsets, corner_list = vertex_corners(faces, nv) if corners is None else (np.asarray(corners[0]), np.asarray(corners[1]))
    with np.errstate(all="ignore"):
        v0, v1, v2 = v[:, faces[:, 0]], v[:, faces[:, 1]], v[:, faces[:, 2]]
        e1, e2 = v1 - v0, v2 - v0
        c = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                      e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                      e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], axis=-1)
        ln = _norm3(c)
        if weighting == "area":
            w = np.repeat((0.5 * ln)[..., None], 3, axis=-1)
        else:
            e3 = v2 - v1
            u, q, p = e1 / _norm3(e1)[..., None], e2 / _norm3(e2)[..., None], e3 / _norm3(e3)[..., None]
            a0 = np.arccos(np.clip(_dot3(u, q), -1.0, 1.0))
            a1 = np.arccos(np.clip(-_dot3(u, p), -1.0, 1.0))
            w = np.stack([a0, a1, (np.pi - a0) - a1], axis=-1)                                   # [P, F, corner]
        unit = c / ln[..., None]
        contrib = np.where((ln == 0.0)[..., None, None], 0.0, w[..., None] * unit[:, :, None, :])    # [P, F, corner, 3]
        contrib = contrib.reshape(len(v), 3 * nf, 3)
        # the sequential sum of every vertex, all vertices at once: round r adds the r-th corner of each vertex that has one
        # (adding the +0.0 of a face without area leaves a sum that started at +0.0 unchanged, bit for bit)
        valence = np.diff(offsets)
        n = np.zeros((len(v), nv, 3), dtype=np.float64)
        for r in range(int(valence.max()) if nv else 0):
            at = np.nonzero(valence > r)[0]
            n[:, at] = n[:, at] + contrib[:, corner_list[offsets[at] + r]]
        length = _norm3(n)[..., None]
        out = np.where(length != 0.0, n / length, 0.0)
    return out.reshape(shape)


def _texel(x: np.ndarray, n: int) -> np.ndarray:
    """(int)clip(trunc(x), 0, n - 1); a NaN lands on 0"""
    x = np.where(np.isnan(x), 0.0, x)
    return np.clip(np.trunc(x), 0, n - 1).astype(np.int64)


def _faces_array(faces, n_vertices: int, name: str) -> np.ndarray:
    """the face list as int64 numpy, shape, dtype and index range checked (the kernels trust the indices)"""
    faces = np.asarray(faces.cpu() if isinstance(faces, torch.Tensor) else faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or len(faces) == 0 or not np.issubdtype(faces.dtype, np.integer):
        raise M324Error(f"{name}: expected non-empty integer faces [F,3], got {faces.dtype}{faces.shape}")
    if faces.min() < 0 or faces.max() >= n_vertices:
        raise M324Error(f"{name}: faces index vertices {faces.min()}..{faces.max()}, the mesh has {n_vertices}")
    return faces.astype(np.int64)


def _check_clip(vertex_frames, num_samples, weighting, name) -> None:
    shape = tuple(vertex_frames.shape)
    if len(shape) != 3 or shape[-1] != 3 or 0 in shape:
        raise M324Error(f"{name}: expected non-empty vertex_frames [T,V,3], got {shape}")
    if int(num_samples) <= 0:
        raise M324Error(f"{name}: num_samples must be positive, got {num_samples}")
    if weighting not in _WEIGHTINGS:
        raise M324Error(f"{name}: weighting must be one of {_WEIGHTINGS}, got {weighting!r}")


def _check_colour_source(n_faces: int, face_uvs, texture_array, name) -> None:
    uv_shape, tex_shape = tuple(face_uvs.shape), tuple(texture_array.shape)
    if uv_shape != (n_faces, 3, 2) or len(tex_shape) != 3 or tex_shape[2] != 3 or 0 in tex_shape or texture_array.dtype not in (np.uint8, torch.uint8):
        raise M324Error(f"{name}: expected face_uvs [{n_faces},3,2] and a uint8 texture [H,W,3], got {uv_shape} / "
                        f"{texture_array.dtype}{tex_shape}")


def _track_host(vertex_frames, faces, num, face_uvs, texture, seed, normals):
    """(points64 [T,num,3], unit normals fp64 [T,num,3], colours fp32 [num,3], face index int64 [num]) in the header's order"""
    v = np.asarray(vertex_frames, dtype=np.float64)
    _, fi = preprocess.sample_surface(v[0], faces, num, seed)
    r = synth.uniform(seed, "surface.bary", (num, 2)).astype(np.float64)              # sample_surface's pair, reflected as there
    flip = r.sum(axis=1) > 1.0
    r[flip] = 1.0 - r[flip]
    r0, r1 = r[:, 0], r[:, 1]
    w0 = (1.0 - r0) - r1
    idx = faces[fi]                                                                   # [num, 3]
    t0, t1, t2 = v[:, idx[:, 0]], v[:, idx[:, 1]], v[:, idx[:, 2]]                    # [T, num, 3]
    points = (t0 + r0[:, None] * (t1 - t0)) + r1[:, None] * (t2 - t0)
    with np.errstate(all="ignore"):
        m = (w0[:, None] * normals[:, idx[:, 0]] + r0[:, None] * normals[:, idx[:, 1]]) + r1[:, None] * normals[:, idx[:, 2]]
        length = _norm3(m)[..., None]
        m = m / np.where(length == 0.0, 1.0, length)
        uv = np.asarray(face_uvs, dtype=np.float64)[fi]                               # [num, 3, 2]
        s = (w0[:, None] * uv[:, 0] + r0[:, None] * uv[:, 1]) + r1[:, None] * uv[:, 2]
        tex = np.asarray(texture)
        col = _texel(s[:, 0] * (tex.shape[1] - 1), tex.shape[1])
        row = _texel((1.0 - s[:, 1]) * (tex.shape[0] - 1), tex.shape[0])
    colors = (tex[row, col].astype(np.float64) / 255.0).astype(np.float32)
    return points, m, colors, fi


# ------------------------------------------------------------------------------------------------ device path
def _upload(a, dtype, dev):
    if isinstance(a, torch.Tensor):
        return a.detach().to(dev, dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


class _Topology(NamedTuple):
    """what depends on the face list alone, on one device: built once per mesh, reused by every later call"""
    faces_np: np.ndarray                        # int64 [F,3], checked against n_vertices; a private copy (astype)
    faces: torch.Tensor                         # int32 [F,3] on the device
    corners: "ops.VertexCorners"                # the vertex-corner table on the device


_TOPOLOGIES: "OrderedDict[tuple, tuple]" = OrderedDict()        # (id(faces), n_vertices, device) -> (weakref, version, _Topology)
_TOPOLOGY_SLOTS = 16


def _topology(faces, n_vertices: int, dev: torch.device, name: str) -> _Topology:
    """The checked face list, its device copy and its vertex-corner table, cached on the identity of the caller's `faces` object
    (a numpy array or a tensor; anything else is rebuilt every call).  A hit is verified: a tensor by its version counter, an
    array by comparing it with the copy the table was built from (about 0.1 ms for 10^5 corners, against milliseconds for the
    check, the sort and the uploads), so an array changed in place is noticed.  The table is built in numpy from the host
    faces (vertex_corners above) and handed to the kernels explicitly."""
    key = (id(faces), int(n_vertices), str(dev))
    hit = _TOPOLOGIES.get(key)
    if hit is not None and hit[0]() is faces:
        if hit[1] == faces._version if isinstance(faces, torch.Tensor) else np.array_equal(faces, hit[2].faces_np):
            _TOPOLOGIES.move_to_end(key)
            return hit[2]
    faces_np = _faces_array(faces, n_vertices, name)
    if faces_np.shape[0] > (2 ** 31 - 1) // 3:
        raise M324Error(f"{name}: {faces_np.shape[0]} faces are more than int32 corner indices hold")
    offsets, corner_list = vertex_corners(faces_np, n_vertices)
    topo = _Topology(faces_np, _upload(faces_np, torch.int32, dev),
                     ops.VertexCorners(_upload(offsets, torch.int32, dev), _upload(corner_list, torch.int32, dev)))
    if isinstance(faces, (np.ndarray, torch.Tensor)):
        _TOPOLOGIES[key] = (weakref.ref(faces, lambda _, key=key: _TOPOLOGIES.pop(key, None)),
                            faces._version if isinstance(faces, torch.Tensor) else None, topo)
        while len(_TOPOLOGIES) > _TOPOLOGY_SLOTS:
            _TOPOLOGIES.popitem(last=False)
    return topo


def _stream_seeds(seeds: Sequence[int], dev) -> torch.Tensor:
    return torch.from_numpy(preprocess.surface_seeds(list(seeds))).to(dev)


def _draw_seeds(seed: int) -> Tuple[int, int]:
    """the seeds of the two draws of one training sample (shape samples, tracked points): distinct streams derived from `seed`"""
    return int(synth._stream_seed(int(seed), "dataset.shape")), int(synth._stream_seed(int(seed), "dataset.pcd"))


def track_with_normal_rgb(vertex_frames, faces, num_samples: int, face_uvs, texture_array, seed: int = 0, *, device=None,
                          weighting: str = "angle"):
    """The reference's track_with_normal_rgb without trimesh: `num_samples` area-weighted samples of frame 0 followed through
    vertex_frames [T,V,3].  Returns (points fp32 [T,num,3], unit normals fp32 [T,num,3], rgbs fp32 [T,num,3] -- one colour per
    sample, the frame axis an expanded view --, face indices int64 [num]).
    device=None: the numpy fp64 definition; torch CPU tensors and a numpy index array come back, as from the reference.
    device=...: the draw, the vertex normals and the tracking run on the GPU and device tensors come back."""
    name = "track_with_normal_rgb"
    _check_clip(vertex_frames, num_samples, weighting, name)
    num, nv = int(num_samples), vertex_frames.shape[1]
    if device is None:
        faces_np = _faces_array(faces, nv, name)
        _check_colour_source(len(faces_np), face_uvs, texture_array, name)
        v = np.asarray(vertex_frames, dtype=np.float64)
        points, normals, colors, fi = _track_host(v, faces_np, num, face_uvs, texture_array, seed, vertex_normals(v, faces_np, None, weighting))
        rgbs = torch.from_numpy(colors)[None].expand(len(v), num, 3)
        return torch.from_numpy(points).float(), torch.from_numpy(normals).float(), rgbs, fi
    dev = torch.device(device)
    topo = _topology(faces, nv, dev, name)
    _check_colour_source(len(topo.faces_np), face_uvs, texture_array, name)
    v = _upload(vertex_frames, torch.float64, dev)
    f = topo.faces
    normals = ops.vertex_normals(v, f, topo.corners, weighting, faces_checked=True)
    s = ops.surface_track(v, f, ops.surface_cdf(v[0], f, faces_checked=True), _stream_seeds([seed], dev)[0], num, vertex_normals=normals,
                          face_uvs=_upload(face_uvs, torch.float64, dev), texture=_upload(texture_array, torch.uint8, dev), faces_checked=True)
    return s.points, s.normals, s.colors[None].expand(v.shape[0], num, 3), s.face_index.long()


def _sizes(config) -> Tuple[int, int]:
    tr = config.get("training", {}) if isinstance(config, dict) else getattr(config, "training", {})
    get = (lambda k, d: tr.get(k, d)) if isinstance(tr, dict) else (lambda k, d: getattr(tr, k, d))
    return int(get("num_shape_samples", 4096)), int(get("num_pcd_samples", 4096))


def _same(x, y) -> bool:
    """one object, or two numpy arrays / two tensors of one device with equal contents; anything mixed counts as different"""
    if x is y:
        return True
    if isinstance(x, np.ndarray) and isinstance(y, np.ndarray):
        return np.array_equal(x, y)
    if isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.device == y.device and x.shape == y.shape:
        return torch.equal(x, y)
    return False


def _one_launch_set(clips: List[dict]) -> bool:
    """True when the clips can be tracked together: one face list, one vertex_frames shape, one colour source.  Clips that share
    the objects (one mesh in several motions, the usual case) are recognised by identity; equal copies are compared."""
    first = clips[0]
    return all(tuple(c["vertex_frames"].shape) == tuple(first["vertex_frames"].shape) and _same(c["faces"], first["faces"])
               and _same(c["face_uvs"], first["face_uvs"]) and _same(c["texture_array"], first["texture_array"]) for c in clips[1:])


def _build_batch(clips: List[dict], config, seeds: Sequence[int], dev: torch.device, weighting: str):
    """clips for which _one_launch_set holds: faces, UVs and texture are checked on the first clip and are the others' too"""
    first, name = clips[0], "make_training_batch"
    _check_clip(first["vertex_frames"], 1, weighting, name)
    topo = _topology(first["faces"], first["vertex_frames"].shape[1], dev, name)
    _check_colour_source(len(topo.faces_np), first["face_uvs"], first["texture_array"], name)
    for k, c in enumerate(clips):
        if tuple(c["rgb_video"].shape[:1]) != tuple(c["vertex_frames"].shape[:1]) or len(c["rgb_video"].shape) != 4:
            raise M324Error(f"make_training_batch: clip {k} has rgb_video {tuple(c['rgb_video'].shape)} for vertex_frames "
                            f"{tuple(c['vertex_frames'].shape)}; expected [T,H,W,3] with the same T")
    n_shape, n_pcd = _sizes(config)
    B = len(clips)
    v = torch.stack([_upload(c["vertex_frames"], torch.float64, dev) for c in clips])                    # [B,T,V,3]
    f = topo.faces
    normals = ops.vertex_normals(v, f, topo.corners, weighting, faces_checked=True)                     # once, shared by both draws
    cdf = ops.surface_cdf(v[:, 0], f, faces_checked=True)
    derived = [_draw_seeds(s) for s in seeds]
    colour = dict(face_uvs=_upload(first["face_uvs"], torch.float64, dev), texture=_upload(first["texture_array"], torch.uint8, dev))
    shape = ops.surface_track(v, f, cdf, _stream_seeds([d[0] for d in derived], dev), n_shape, vertex_normals=normals, frames=1,
                              want_face=False, faces_checked=True, **colour)                            # frame 0 in place: no copy
    pcd = ops.surface_track(v, f, cdf, _stream_seeds([d[1] for d in derived], dev), n_pcd, vertex_normals=normals, want_face=False,
                            faces_checked=True, **colour)
    batch = {
        "rgb_video": torch.stack([_upload(c["rgb_video"], torch.float32, dev) for c in clips]),
        "point_clouds": pcd.points, "point_rgbs": pcd.colors[:, None].expand(B, v.shape[1], n_pcd, 3),
        "ref_shape_pcd": shape.points[:, 0], "ref_shape_normals": shape.normals[:, 0], "ref_shape_rgbs": shape.colors,
        "ref_pcd": pcd.points[:, 0], "ref_normal": pcd.normals[:, 0], "ref_rgb": pcd.colors,
    }
    finite = torch.stack([torch.isfinite(t).reshape(B, -1).all(dim=1) for t in (shape.points, shape.normals, pcd.points, pcd.normals)]).all(dim=0)
    return batch, finite


def make_training_batch(clips: List[dict], config, seeds: Sequence[int], *, device, weighting: str = "angle"):
    """Training samples of several clips.  clips: dicts with 'vertex_frames' [T,V,3], 'faces' [F,3], 'face_uvs' [F,3,2],
    'texture_array' uint8 [H,W,3], 'rgb_video' [T,H,W,3]; seeds: one per clip.  Clips that share the face list, the UVs and the
    texture (one object in several motions) are built by one set of launches; anything else is built clip by clip and collated.
    Returns (batch, finite): the [B, ...] dict training.forward_backward accepts and a device bool [B], false where a sample's
    points or normals hold a NaN or an infinity."""
    if len(clips) == 0 or len(seeds) != len(clips):
        raise M324Error(f"make_training_batch: {len(seeds)} seed(s) for {len(clips)} clip(s)")
    dev = torch.device(device)
    if _one_launch_set(clips):
        return _build_batch(clips, config, seeds, dev, weighting)
    built = [_build_batch([c], config, [s], dev, weighting) for c, s in zip(clips, seeds)]
    return collate([{k: t[0] for k, t in b.items()} for b, _ in built]), torch.cat([fin for _, fin in built])


def make_training_sample(vertex_frames, faces, face_uvs, texture_array, rgb_video, config, seed: int = 0, *, device,
                         weighting: str = "angle") -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """One sample of the reference's dataset (dyscene.py:266-329) from a mesh clip, built on the GPU: `num_shape_samples` samples
    of frame 0 (ref_shape_*) and `num_pcd_samples` samples tracked through the clip (point_clouds, point_rgbs; ref_pcd /
    ref_normal / ref_rgb are their frame 0), from two distinct streams derived from `seed`; the clip's vertex normals are
    computed once for both.  Returns (sample, finite): the dataset's keys, shapes and dtypes without the batch axis, and one
    device bool that is false when points or normals hold a NaN or an infinity -- the reference draws another object then;
    that policy stays with the caller."""
    clip = dict(vertex_frames=vertex_frames, faces=faces, face_uvs=face_uvs, texture_array=texture_array, rgb_video=rgb_video)
    batch, finite = make_training_batch([clip], config, [seed], device=device, weighting=weighting)
    return {k: t[0] for k, t in batch.items()}, finite[0]


def collate(samples: Sequence[Dict[str, torch.Tensor]]) -> Dict[str, torch.Tensor]:
    """Samples of make_training_sample -> the [B, ...] batch training.forward_backward accepts (torch's default collate of the
    reference's dataloader, for the tensor keys)."""
    if len(samples) == 0:
        raise M324Error("collate: no samples")
    missing = [k for k in SAMPLE_KEYS if any(k not in s for s in samples)]
    if missing:
        raise M324Error(f"collate: samples lack {missing}")
    return {k: torch.stack([s[k] for s in samples]).contiguous() for k in SAMPLE_KEYS}
