"""Renders a predicted mesh clip on the GPU: `pcd_moved` in, shaded frames with face-id and depth buffers out.

The last stage after the forward pass: an orthographic, z-buffered rasterizer over every frame of a clip with one topology
(csrc/render.hip; the arithmetic is spelled out in include/m324.h).  Ownership of a pixel is decided in integers, so the
buffers are exact: the same inputs give the same bytes on any grid, chunking or `big_pixels`.

    python -m motion324_amd.render --pred_path DIR --out DIR [--size 512 --azimuth 0 --elevation 0 --shading flat|smooth]
"""
from __future__ import annotations

import argparse
import math
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .lib import M324Error

SHADINGS = ("flat", "smooth")
MAX_SIDE = 1024                 # M324_RENDER_MAX_SIDE


class RenderedClip(NamedTuple):
    frames: torch.Tensor        # uint8 [T,S,S,3]
    face: torch.Tensor          # int32 [T,S,S]: the face that owns the pixel, -1 on the background
    depth: torch.Tensor         # int32 [T,S,S]: z_pix (smaller is nearer, 2^22 at view z = 0), -1 on the background

    def mask(self) -> torch.Tensor:
        """coverage as uint8 0 / 255 [T,S,S], the form of framing.FramedVideo.mask"""
        return (self.face >= 0).to(torch.uint8) * 255


def view_matrix(azimuth: float = 0.0, elevation: float = 0.0) -> np.ndarray:
    """The row-major 3 x 4 view matrix (fp32, built in fp64) of a camera that orbits the origin: `azimuth` degrees around +y,
    then `elevation` degrees up.  Model space is glTF's (+y up, the unit cube centred on the origin); the camera looks down -z,
    so (0, 0) is the identity rotation.  No translation: the orthographic window is the cube's face."""
    a, e = math.radians(float(azimuth)), math.radians(float(elevation))
    ry = np.array([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]], dtype=np.float64)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(e), -math.sin(e)], [0.0, math.sin(e), math.cos(e)]], dtype=np.float64)
    m = np.zeros((3, 4), dtype=np.float64)
    m[:, :3] = rx @ ry
    return m.astype(np.float32)


def _to_device(x, dtype: torch.dtype, device, name: str) -> torch.Tensor:
    """a device tensor as it is; numpy / CPU data only when the caller named a device (there is no CPU path)"""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x if x.dtype == dtype else x.to(dtype)
    if device is None:
        raise M324Error(f"render_clip: {name} is not on a HIP device and no device was given (there is no CPU renderer)")
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype)


def render_clip(vertices, faces, *, colors=None, shading: str = "flat", size: int = 512, azimuth: float = 0.0, elevation: float = 0.0,
                ambient: float = 0.3, background=(0, 0, 0), device=None, max_scratch_bytes: int = 1 << 30,
                big_pixels: Optional[int] = None) -> RenderedClip:
    """Renders every frame of a mesh clip.  vertices fp32 [T,V,3] or [1,T,V,3] (the shape of `pcd_moved` and of what
    smooth_trajectories returns), a device tensor -- a view with contiguous last two axes is used in place -- or numpy with
    `device`; faces int [F,3]; colors fp32 [V,3] or [1,V,3] in [0, 1] (the shape of `ref_rgb`), 0.8 grey without.
    shading "flat" (face normals) or "smooth" (ops.vertex_normals, angle-weighted).  The frames are processed in chunks whose
    scratch stays under max_scratch_bytes; the outputs are allocated once.  big_pixels: see ops.render_raster; never visible."""
    if shading not in SHADINGS:
        raise M324Error(f"render_clip: shading must be one of {SHADINGS}, got {shading!r}")
    size = int(size)
    if not 1 <= size <= MAX_SIDE:
        raise M324Error(f"render_clip: size must be in 1..{MAX_SIDE}, got {size}")
    if big_pixels is not None and not 0 <= int(big_pixels) <= 2 ** 31 - 1:
        raise M324Error(f"render_clip: big_pixels must be in 0..2^31-1, got {big_pixels}")
    if not 0.0 <= float(ambient) <= 1.0 or len(tuple(background)) != 3 or any(not 0 <= int(c) <= 255 for c in background):
        raise M324Error(f"render_clip: ambient lies in [0, 1] and background is three bytes, got {ambient!r}, {background!r}")
    v = _to_device(vertices, torch.float32, device, "vertices")
    if v.dim() == 4 and v.shape[0] == 1:
        v = v[0]
    if v.dim() != 3 or v.shape[2] != 3 or 0 in v.shape:
        raise M324Error(f"render_clip: expected vertices [T,V,3] or [1,T,V,3], got {tuple(v.shape)}")
    dev = v.device
    f = _to_device(faces, torch.int32, dev, "faces").contiguous()
    T, nv = v.shape[0], v.shape[1]
    f = ops._render_faces(f, nv, dev, "render_clip", faces_checked=False)       # the one range check of the whole clip
    nf = f.shape[0]
    col = None
    if colors is not None:
        col = _to_device(colors, torch.float32, dev, "colors")
        if col.dim() == 3 and col.shape[0] == 1:
            col = col[0]
        if tuple(col.shape) != (nv, 3):
            raise M324Error(f"render_clip: expected colors [{nv},3] or [1,{nv},3], got {tuple(col.shape)}")
        col = col.contiguous()
    m = view_matrix(azimuth, elevation)

    per_frame = ops.render_plan(nv, nf, 1, size)
    chunk = max(1, min(T, int(max_scratch_bytes) // per_frame))
    while chunk > 1 and (chunk * nf >= 2 ** 31 - 1 or chunk * nv >= 2 ** 31 - 1 or ops.render_plan(nv, nf, chunk, size) > max_scratch_bytes):
        chunk -= 1
    need = ops.render_plan(nv, nf, chunk, size)
    if need > max_scratch_bytes:
        raise M324Error(f"render_clip: one frame needs {need} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
    scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
    out = RenderedClip(torch.empty((T, size, size, 3), dtype=torch.uint8, device=dev), torch.empty((T, size, size), dtype=torch.int32, device=dev),
                       torch.empty((T, size, size), dtype=torch.int32, device=dev))
    corners = ops.vertex_corners(f, nv) if shading == "smooth" else None
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        part = v[t0:t1]
        normals = None
        if shading == "smooth":
            normals = ops.vertex_normals(part.to(torch.float64), f, corners, faces_checked=True).to(torch.float32)
        ops.render_project(part, m, size, nf, scratch)
        ops.render_raster(f, nv, t1 - t0, size, scratch, big_pixels, faces_checked=True)
        ops.render_shade(f, nv, t1 - t0, size, scratch, m, colors=col, normals=normals, ambient=ambient, background=background,
                         out=(out.frames[t0:t1], out.face[t0:t1], out.depth[t0:t1]), faces_checked=True)
    return out


def main(argv=None) -> RenderedClip:
    from .evaluation import load_sequence_dir
    parser = argparse.ArgumentParser(description="Render a predicted mesh sequence on the GPU (orthographic, exact rasterizer)")
    parser.add_argument("--pred_path", type=str, required=True, help="directory with faces.npy and frame_%%04d.npy")
    parser.add_argument("--out", type=str, required=True, help="directory for frame_%%04d.png (frames.npy without PIL)")
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--azimuth", type=float, default=0.0, help="degrees around +y")
    parser.add_argument("--elevation", type=float, default=0.0, help="degrees up")
    parser.add_argument("--shading", choices=SHADINGS, default="flat")
    args = parser.parse_args(argv)
    vertices, faces = load_sequence_dir(args.pred_path)          # refuses a GLB / FBX path, naming the layout
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.render needs a HIP device (there is no CPU renderer)")
    clip = render_clip(vertices.astype(np.float32), faces.astype(np.int32), shading=args.shading, size=args.size, azimuth=args.azimuth,
                       elevation=args.elevation, device="cuda")
    os.makedirs(args.out, exist_ok=True)
    frames = clip.frames.cpu().numpy()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is None:
        np.save(os.path.join(args.out, "frames.npy"), frames)
    else:
        for t, frame in enumerate(frames):
            Image.fromarray(frame).save(os.path.join(args.out, f"frame_{t:04d}.png"))
    print(f"{len(frames)} frame(s) of {args.size} x {args.size} -> {args.out}")
    return clip


if __name__ == "__main__":
    main()
