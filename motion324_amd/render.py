"""Renders a predicted mesh clip on the GPU: `pcd_moved` in, shaded frames with face-id and depth buffers out.

The last stage after the forward pass: an orthographic, z-buffered rasterizer over every frame of a clip with one topology
(csrc/render.hip; the arithmetic is spelled out in include/m324.h).  Ownership of a pixel is decided in integers, so the
buffers are exact: the same inputs give the same bytes on any grid, chunking or `big_pixels`.

A base-colour texture addressed through UVs (mip-mapped, bilinear, repeat) and ss x ss supersampling are part of the same
contract: the level of a (frame, face) is exact under the orthographic camera, and the resolve is an integer mean.

    python -m motion324_amd.render --pred_path DIR --out DIR [--size 512 --azimuth 0 --elevation 0 --shading flat|smooth]
                                   [--texture FILE] [--supersample N] [--no-mipmaps]
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
    # with supersample = ss > 1, face and depth are [T,S ss,S ss], one value per sample; frames stay [T,S,S,3]

    def mask(self) -> torch.Tensor:
        """coverage as uint8 [T,S,S], the form of framing.FramedVideo.mask: 0 / 255, and with supersample = ss > 1 the share of
        a pixel's ss^2 samples that are covered, (255 * covered + ss^2 / 2) // ss^2"""
        ss = self.face.shape[1] // self.frames.shape[1]
        if ss == 1:
            return (self.face >= 0).to(torch.uint8) * 255
        T, S = self.frames.shape[0], self.frames.shape[1]
        covered = (self.face >= 0).view(T, S, ss, S, ss).sum(dim=(2, 4), dtype=torch.int32)
        return ((255 * covered + ss * ss // 2) // (ss * ss)).to(torch.uint8)


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


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else tuple(np.shape(x))


def _dtype_name(x) -> str:
    return str(x.dtype).replace("torch.", "") if hasattr(x, "dtype") else str(np.asarray(x).dtype)


def _check_texturing(vertices, faces, colors, uv, face_uvs, texture, supersample, size):
    """every refusal of the texture and supersampling keywords, on shapes and dtypes alone: before any copy or launch"""
    if supersample not in ops.SUPERSAMPLES or isinstance(supersample, bool):
        raise M324Error(f"render_clip: supersample must be one of {ops.SUPERSAMPLES}, got {supersample!r}")
    if size * supersample > MAX_SIDE:
        raise M324Error(f"render_clip: size * supersample must stay within {MAX_SIDE} samples a side, got {size} * {supersample}")
    if uv is not None and face_uvs is not None:
        raise M324Error("render_clip: give uv ([V,2], per vertex) or face_uvs ([F,3,2], per corner), not both")
    has_uv = uv is not None or face_uvs is not None
    if has_uv and texture is None:
        raise M324Error("render_clip: uv / face_uvs without a texture")
    if texture is not None and not has_uv:
        raise M324Error("render_clip: a texture needs uv ([V,2]) or face_uvs ([F,3,2])")
    if texture is None:
        return
    if colors is not None:
        raise M324Error("render_clip: a texture and colors are two albedos: give one")
    shape = _shape_of(texture)
    if _dtype_name(texture) != "uint8" or len(shape) != 3 or shape[2] not in (3, 4) or 0 in shape:
        raise M324Error(f"render_clip: expected a uint8 texture [H,W,3] or [H,W,4], got {_dtype_name(texture)} {shape}")
    if max(shape[0], shape[1]) > ops.TEXTURE_MAX_SIDE:
        raise M324Error(f"render_clip: texture sides must be in 1..{ops.TEXTURE_MAX_SIDE}, got {shape[0]} x {shape[1]}")
    vs, fs = _shape_of(vertices), _shape_of(faces)
    for given, want, name in ((uv, (vs[-2], 2) if len(vs) >= 2 else None, "uv"), (face_uvs, (fs[0], 3, 2) if len(fs) == 2 else None, "face_uvs")):
        if given is None:
            continue
        if want is None or _shape_of(given) != want or not _dtype_name(given).startswith("float"):
            raise M324Error(f"render_clip: expected floating-point {name} {list(want) if want else ''}, got {_dtype_name(given)} {_shape_of(given)}")


def render_clip(vertices, faces, *, colors=None, shading: str = "flat", size: int = 512, azimuth: float = 0.0, elevation: float = 0.0,
                ambient: float = 0.3, background=(0, 0, 0), device=None, max_scratch_bytes: int = 1 << 30,
                big_pixels: Optional[int] = None, uv=None, face_uvs=None, texture=None, mipmaps: bool = True,
                supersample: int = 1) -> RenderedClip:
    """Renders every frame of a mesh clip.  vertices fp32 [T,V,3] or [1,T,V,3] (the shape of `pcd_moved` and of what
    smooth_trajectories returns), a device tensor -- a view with contiguous last two axes is used in place -- or numpy with
    `device`; faces int [F,3]; colors fp32 [V,3] or [1,V,3] in [0, 1] (the shape of `ref_rgb`), 0.8 grey without.
    shading "flat" (face normals) or "smooth" (ops.vertex_normals, angle-weighted).  The frames are processed in chunks whose
    scratch stays under max_scratch_bytes; the outputs are allocated once.  big_pixels: see ops.render_raster; never visible.
    texture uint8 [H,W,3|4] (a fourth channel is ignored) with uv fp32 [V,2] or face_uvs fp32 [F,3,2] (per corner: UV seams)
    replaces colors as the albedo: repeat wrap, v up, bilinear taps on the mip level of the (frame, face) -- level 0 always with
    mipmaps=False.  The chain is built once per call.  supersample = ss in (1, 2, 4) rasterizes at size * ss (at most 1024) and
    averages ss x ss samples per pixel: frames stay [T,size,size,3]; face and depth are [T,size ss,size ss]."""
    if shading not in SHADINGS:
        raise M324Error(f"render_clip: shading must be one of {SHADINGS}, got {shading!r}")
    size = int(size)
    if not 1 <= size <= MAX_SIDE:
        raise M324Error(f"render_clip: size must be in 1..{MAX_SIDE}, got {size}")
    if big_pixels is not None and not 0 <= int(big_pixels) <= 2 ** 31 - 1:
        raise M324Error(f"render_clip: big_pixels must be in 0..2^31-1, got {big_pixels}")
    if not 0.0 <= float(ambient) <= 1.0 or len(tuple(background)) != 3 or any(not 0 <= int(c) <= 255 for c in background):
        raise M324Error(f"render_clip: ambient lies in [0, 1] and background is three bytes, got {ambient!r}, {background!r}")
    _check_texturing(vertices, faces, colors, uv, face_uvs, texture, supersample, size)
    ss = int(supersample)
    textured = texture is not None
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
    corner_uvs = mips = tex_size = None
    if textured:
        if uv is not None:
            per_vertex = _to_device(uv, torch.float32, dev, "uv")
            if tuple(per_vertex.shape) != (nv, 2):
                raise M324Error(f"render_clip: expected uv [{nv},2], got {tuple(per_vertex.shape)}")
            corner_uvs = per_vertex[f.long()].contiguous()                        # [F,3,2], once per call
        else:
            corner_uvs = _to_device(face_uvs, torch.float32, dev, "face_uvs").contiguous()
        tex = _to_device(texture, torch.uint8, dev, "texture")
        tex_size = (tex.shape[0], tex.shape[1])
        mips, _levels = ops.texture_mips(tex)                                     # once per call, not per chunk
    m = view_matrix(azimuth, elevation)

    side = size * ss                                                              # the sample resolution: project and raster run at it
    per_frame = ops.render_plan(nv, nf, 1, side)
    chunk = max(1, min(T, int(max_scratch_bytes) // per_frame))
    while chunk > 1 and (chunk * nf >= 2 ** 31 - 1 or chunk * nv >= 2 ** 31 - 1 or ops.render_plan(nv, nf, chunk, side) > max_scratch_bytes):
        chunk -= 1
    need = ops.render_plan(nv, nf, chunk, side)
    if need > max_scratch_bytes:
        raise M324Error(f"render_clip: one frame needs {need} scratch bytes, max_scratch_bytes is {max_scratch_bytes}")
    scratch = torch.empty((need,), dtype=torch.uint8, device=dev)
    out = RenderedClip(torch.empty((T, size, size, 3), dtype=torch.uint8, device=dev), torch.empty((T, side, side), dtype=torch.int32, device=dev),
                       torch.empty((T, side, side), dtype=torch.int32, device=dev))
    corners = ops.vertex_corners(f, nv) if shading == "smooth" else None
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        part = v[t0:t1]
        normals = None
        if shading == "smooth":
            normals = ops.vertex_normals(part.to(torch.float64), f, corners, faces_checked=True).to(torch.float32)
        ops.render_project(part, m, side, nf, scratch)
        ops.render_raster(f, nv, t1 - t0, side, scratch, big_pixels, faces_checked=True)
        views = (out.frames[t0:t1], out.face[t0:t1], out.depth[t0:t1])
        if textured or ss > 1:
            ops.render_shade_tex(f, nv, t1 - t0, side, scratch, m, colors=col, normals=normals, ambient=ambient, background=background,
                                 face_uvs=corner_uvs, mips=mips, tex_size=tex_size, use_mips=mipmaps, supersample=ss, out=views,
                                 faces_checked=True)
        else:                                                                     # none of the texture keywords: the path as it was
            ops.render_shade(f, nv, t1 - t0, side, scratch, m, colors=col, normals=normals, ambient=ambient, background=background,
                             out=views, faces_checked=True)
    return out


def _load_texture(path: str) -> np.ndarray:
    """uint8 [H,W,3|4] of a .npy array or of an image file (through PIL)"""
    if path.lower().endswith(".npy"):
        return np.load(path)
    try:
        from PIL import Image
    except ImportError:
        raise M324Error(f"{path}: reading an image file needs PIL; a .npy array uint8 [H,W,3] or [H,W,4] is read without it") from None
    with Image.open(path) as im:
        return np.asarray(im.convert("RGBA" if "A" in im.getbands() else "RGB"))


def main(argv=None) -> RenderedClip:
    from .evaluation import load_sequence_dir
    parser = argparse.ArgumentParser(description="Render a predicted mesh sequence on the GPU (orthographic, exact rasterizer)")
    parser.add_argument("--pred_path", type=str, required=True, help="directory with faces.npy and frame_%%04d.npy")
    parser.add_argument("--out", type=str, required=True, help="directory for frame_%%04d.png (frames.npy without PIL)")
    parser.add_argument("--size", type=int, default=512)
    parser.add_argument("--azimuth", type=float, default=0.0, help="degrees around +y")
    parser.add_argument("--elevation", type=float, default=0.0, help="degrees up")
    parser.add_argument("--shading", choices=SHADINGS, default="flat")
    parser.add_argument("--texture", type=str, default=None, help="base-colour texture: PNG / JPG (through PIL) or .npy uint8 [H,W,3|4]; needs uv.npy in --pred_path")
    parser.add_argument("--supersample", type=int, default=1, help="samples per pixel side: 1, 2 or 4")
    parser.add_argument("--no-mipmaps", dest="mipmaps", action="store_false", help="sample level 0 of the texture only")
    args = parser.parse_args(argv)
    vertices, faces = load_sequence_dir(args.pred_path)          # refuses a GLB / FBX path, naming the layout
    tex_kw = {}
    if args.texture is not None:
        uv_path = os.path.join(args.pred_path, "uv.npy")
        V, F = vertices.shape[1], faces.shape[0]
        if not os.path.exists(uv_path):
            raise M324Error(f"{uv_path} not found: --texture needs it, fp32 [V,2] = [{V},2] (per vertex) or [F,3,2] = [{F},3,2] (per corner)")
        uvs = np.load(uv_path).astype(np.float32)
        if uvs.shape == (F, 3, 2):
            tex_kw["face_uvs"] = uvs
        elif uvs.shape == (V, 2):
            tex_kw["uv"] = uvs
        else:
            raise M324Error(f"{uv_path}: expected [V,2] = [{V},2] or [F,3,2] = [{F},3,2], got {list(uvs.shape)}")
        tex_kw["texture"] = _load_texture(args.texture)
    if args.supersample not in ops.SUPERSAMPLES or args.size * args.supersample > MAX_SIDE:
        raise M324Error(f"--supersample must be one of {ops.SUPERSAMPLES} with size * supersample <= {MAX_SIDE}, got {args.supersample} at size {args.size}")
    if not torch.cuda.is_available():
        raise M324Error("motion324_amd.render needs a HIP device (there is no CPU renderer)")
    clip = render_clip(vertices.astype(np.float32), faces.astype(np.int32), shading=args.shading, size=args.size, azimuth=args.azimuth,
                       elevation=args.elevation, device="cuda", mipmaps=args.mipmaps, supersample=args.supersample, **tex_kw)
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
