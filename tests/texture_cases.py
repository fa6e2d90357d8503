"""Cases and the numpy model of textured, supersampled mesh clips (tests/test_texture_cpu.py, tests/test_texture_gpu.py).

Written from the arithmetic documented in include/m324.h ("Textured and anti-aliased mesh clips"), in numpy integers and
float32; it shares no code with motion324_amd/render.py or the kernels.  Projection, rasterization and the untextured shading
are render_cases' (imported, not changed); the textured albedo, the mip chain and the resolve are modelled here."""
import math

import numpy as np

import render_cases as rc

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the chain
def model_plan(tex_h, tex_w):
    """([(byte offset, H_l, W_l)], bytes of the chain) by the header's offset rule"""
    out, at, h, w = [], 0, int(tex_h), int(tex_w)
    while True:
        out.append((at, h, w))
        at += (4 * w * h + 255) // 256 * 256
        if h == 1 and w == 1:
            return out, at
        h, w = max(1, h >> 1), max(1, w >> 1)


def model_mips(texture):
    """the levels as uint8 [H_l, W_l, 4] arrays (R, G, B, 0), integer arithmetic throughout"""
    texture = np.asarray(texture)
    assert texture.dtype == np.uint8 and texture.ndim == 3 and texture.shape[2] in (3, 4)
    level = np.zeros(texture.shape[:2] + (4,), dtype=np.int64)
    level[..., :3] = texture[..., :3]
    levels = [level]
    while level.shape[:2] != (1, 1):
        H, W = level.shape[:2]
        h, w = max(1, H >> 1), max(1, W >> 1)
        x0, x1 = np.minimum(2 * np.arange(w), W - 1), np.minimum(2 * np.arange(w) + 1, W - 1)
        y0, y1 = np.minimum(2 * np.arange(h), H - 1), np.minimum(2 * np.arange(h) + 1, H - 1)
        level = (level[y0][:, x0] + level[y0][:, x1] + level[y1][:, x0] + level[y1][:, x1] + 2) >> 2
        levels.append(level)
    return [lv.astype(np.uint8) for lv in levels]


def chain_bytes(texture):
    """the whole chain as the uint8 buffer m324_texture_mips fills, zeros between the levels"""
    levels = model_mips(texture)
    plan, total = model_plan(*np.asarray(texture).shape[:2])
    assert len(plan) == len(levels)
    buf = np.zeros(total, dtype=np.uint8)
    for (off, h, w), lv in zip(plan, levels):
        assert lv.shape == (h, w, 4)
        buf[off:off + 4 * h * w] = lv.reshape(-1)
    return buf


# ------------------------------------------------------------------------------------------------ sampling
def model_level(rho, last):
    """l = 0; while (l < last && rho > 2 * 4^l) ++l, on a float32 array"""
    rho = np.asarray(rho, dtype=np.float32)
    l = np.zeros(rho.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for k in range(last):
            l = np.where((l == k) & (rho > F32(2.0 * 4.0 ** k)), k + 1, l)
    return l


def model_taps(levels, l, u, v):
    """float32 albedo [n, 3] of bilinear taps at (u, v) on level l[n] of `levels` (steps 4 and 5 of the header)"""
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    out = np.zeros(u.shape + (3,), dtype=np.float32)
    with np.errstate(all="ignore"):
        u = np.where(np.isfinite(u), u, F32(0))
        v = np.where(np.isfinite(v), v, F32(0))
        for k in np.unique(l):
            sel = np.nonzero(l == k)[0]
            lv = levels[int(k)].astype(np.float32)
            H, W = lv.shape[:2]
            uw, vw = u[sel] - np.floor(u[sel]), v[sel] - np.floor(v[sel])
            x = uw * F32(W) - F32(0.5)
            y = (F32(1.0) - vw) * F32(H) - F32(0.5)
            xf, yf = np.floor(x), np.floor(y)
            fx, fy = x - xf, y - yf
            assert fx.dtype == np.float32 and fy.dtype == np.float32
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            c0, c1, r0, r1 = np.mod(x0, W), np.mod(x0 + 1, W), np.mod(y0, H), np.mod(y0 + 1, H)
            for c in range(3):
                t00, t01, t10, t11 = lv[r0, c0, c], lv[r0, c1, c], lv[r1, c0, c], lv[r1, c1, c]
                top = t00 + fx * (t01 - t00)
                bot = t10 + fx * (t11 - t10)
                val = top + fy * (bot - top)
                assert val.dtype == np.float32
                out[sel, c] = val / F32(255.0)
    return out


def model_shade_tex(keys, xs, ys, pos, faces, view, S, face_uvs, texture, use_mips=True, normals=None, ambient=0.3, background=(0, 0, 0)):
    """(rgb uint8 [T,S,S,3] per SAMPLE, face, depth, levels used int64 [T,S,S] with -1 on the background): m324_render_shade's
    arithmetic restated with the textured albedo"""
    T = keys.shape[0]
    faces = np.asarray(faces, dtype=np.int64)
    M = np.asarray(view, dtype=np.float32)
    amb = F32(ambient)
    levels = model_mips(texture)
    H0, W0 = levels[0].shape[:2]
    last = len(levels) - 1 if use_mips else 0
    uvs = np.asarray(face_uvs, dtype=np.float32)
    uvs = np.where(np.isfinite(uvs), uvs, F32(0)).astype(np.float32)
    rgb = np.empty((T, S, S, 3), dtype=np.uint8)
    rgb[...] = np.asarray(background, dtype=np.uint8)
    face = np.full((T, S, S), -1, dtype=np.int32)
    depth = np.full((T, S, S), -1, dtype=np.int32)
    used = np.full((T, S, S), -1, dtype=np.int64)
    for t in range(T):
        py, px = np.nonzero(keys[t] != rc.EMPTY)
        if len(py) == 0:
            continue
        k = keys[t, py, px]
        f = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
        face[t, py, px] = f
        depth[t, py, px] = (k >> np.uint64(32)).astype(np.int64)
        idx = faces[f]
        x = [xs[t, idx[:, i]] for i in range(3)]
        y = [ys[t, idx[:, i]] for i in range(3)]
        A, B, Cc, area2 = rc._edges(x, y)
        X, Y = 16 * px.astype(np.int64) + 8, 16 * py.astype(np.int64) + 8
        area = area2.astype(np.float32)
        b = [(A[i] * X + B[i] * Y + Cc[i]).astype(np.float32) / area for i in range(3)]
        with np.errstate(all="ignore"):
            if normals is None:
                p = [pos[t, idx[:, i]] for i in range(3)]
                e1, e2 = p[1] - p[0], p[2] - p[0]
                n = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
            else:
                vn = np.asarray(normals, dtype=np.float32)[t]
                m = [(b[0] * vn[idx[:, 0], c] + b[1] * vn[idx[:, 1], c]) + b[2] * vn[idx[:, 2], c] for c in range(3)]
                n = [(M[r, 0] * m[0] + M[r, 1] * m[1]) + M[r, 2] * m[2] for r in range(3)]
            length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            ok = (length > 0) & np.isfinite(length)
            lit = np.where(ok, np.abs(n[2]) / np.where(ok, length, F32(1)), F32(0)).astype(np.float32)
            shade = amb + (F32(1.0) - amb) * lit
            cu, cv = [uvs[f, i, 0] for i in range(3)], [uvs[f, i, 1] for i in range(3)]
            u = (b[0] * cu[0] + b[1] * cu[1]) + b[2] * cu[2]
            v = (b[0] * cv[0] + b[1] * cv[1]) + b[2] * cv[2]
            ua2 = np.abs((cu[1] - cu[0]) * (cv[2] - cv[0]) - (cu[2] - cu[0]) * (cv[1] - cv[0]))
            rho = ((ua2 * F32(W0)) * F32(H0)) / (area / F32(256.0))
            assert rho.dtype == np.float32 and u.dtype == np.float32 and shade.dtype == np.float32
            l = model_level(rho, last)
            used[t, py, px] = l
            albedo = model_taps(levels, l, u, v)
            for c in range(3):
                val = albedo[:, c] * shade
                val = np.where(val > 0, val, F32(0))
                val = np.where(val < 1, val, F32(1))
                out = np.floor(val * F32(255.0) + F32(0.5))
                assert out.dtype == np.float32
                rgb[t, py, px, c] = out.astype(np.uint8)
    return rgb, face, depth, used


def model_resolve(samples, ss):
    """uint8 [T,S,S,3] samples -> uint8 [T,S/ss,S/ss,3]: (sum + ss^2 / 2) >> log2(ss^2)"""
    T, S = samples.shape[:2]
    assert ss in (1, 2, 4) and S % ss == 0
    total = samples.astype(np.int64).reshape(T, S // ss, ss, S // ss, ss, 3).sum(axis=(2, 4))
    return ((total + ss * ss // 2) >> {1: 0, 2: 2, 4: 4}[ss]).astype(np.uint8)


def model_coverage(face, ss):
    """uint8 [T,S/ss,S/ss]: (255 * covered + ss^2 / 2) // ss^2"""
    T, S = face.shape[:2]
    covered = (face >= 0).astype(np.int64).reshape(T, S // ss, ss, S // ss, ss).sum(axis=(2, 4))
    return ((255 * covered + ss * ss // 2) // (ss * ss)).astype(np.uint8)


def model_render_tex(vertices, faces, view, size, supersample=1, face_uvs=None, texture=None, use_mips=True, colors=None, normals=None,
                     ambient=0.3, background=(0, 0, 0), cache_key=None):
    """dict(frames [T,size,size,3], face, depth [T,size ss,size ss], levels): render_cases' projection and rasterization at the
    sample resolution size * ss (cached under cache_key like rc.model_render), the shading above, the resolve"""
    vertices = np.asarray(vertices, dtype=np.float32)
    if vertices.ndim == 2:
        vertices = vertices[None]
    S = size * supersample
    hit = rc._MODEL_CACHE.get(cache_key) if cache_key is not None else None
    if hit is None:
        xs, ys, zq, valid, pos = rc.model_project(vertices, view, S)
        keys, hits, peak = rc.model_raster(xs, ys, zq, valid, faces, S)
        hit = (xs, ys, pos, keys, hits, peak)
        if cache_key is not None:
            rc._MODEL_CACHE[cache_key] = hit
    xs, ys, pos, keys, _hits, _peak = hit
    assert keys.shape[1] == S
    used = None
    if texture is None:
        rgb, face, depth = rc.model_shade(keys, xs, ys, pos, faces, view, S, colors, normals, ambient, background)
    else:
        rgb, face, depth, used = model_shade_tex(keys, xs, ys, pos, faces, view, S, face_uvs, texture, use_mips, normals, ambient, background)
    return dict(frames=model_resolve(rgb, supersample), face=face, depth=depth, levels=used)


# ------------------------------------------------------------------------------------------------ cases
def noise_texture(h, w, channels=3, seed=324):
    return np.random.default_rng([seed, h, w, channels]).integers(0, 256, (h, w, channels), dtype=np.uint8)


def anchor_quad(x0, y0, x1, y1, S=16):
    """(vertices [4,3], faces [2,3], uv [4,2]): the camera-facing quad over the pixels [x0, x1) x [y0, y1) of an S x S image; its
    UVs run over the whole texture, u to the right and v up, so a texture of (x1 - x0) x (y1 - y0) texels has texel (i, j) on
    pixel (x0 + i, y0 + j)"""
    vertices = rc.pixels_to_model([x0, x1, x1, x0], [y0, y0, y1, y1], S)
    uv = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0], [0.0, 0.0]], dtype=np.float32)
    return vertices, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32), uv


def random_corner_uvs(n_faces, seed, lo=-1.25, hi=2.5):
    """fp32 [F,3,2] drawn per corner: every shared vertex is a UV seam, the range exercises wrap and negative x0"""
    return np.random.default_rng([seed, n_faces]).uniform(lo, hi, (n_faces, 3, 2)).astype(np.float32)


def grid_textured(S, k=3):
    """render_cases.grid_snapped with per-corner UVs over [-1.25, 2.5] (seams everywhere), a face whose three UVs coincide
    (level 0), NaN and +-inf components, and two faces with a large UV footprint (high levels)"""
    vertices, faces = rc.grid_snapped(S, k)
    uvs = random_corner_uvs(len(faces), S)
    uvs[5] = uvs[5, 0]
    uvs[7, 0, 0] = np.nan
    uvs[9, 1, 1] = np.inf
    uvs[11, 2, 0] = -np.inf
    uvs[20] *= F32(16.0)
    uvs[30] *= F32(64.0)
    return vertices, faces, uvs


def sphere_uvs(vertices0, repeat=(1.0, 1.0)):
    """spherical UVs fp32 [V,2] of a sphere's first pose: longitude and latitude of the direction from its centre"""
    d = np.asarray(vertices0, dtype=np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    u = np.arctan2(d[:, 2], d[:, 0]) / (2.0 * math.pi) + 0.5
    v = np.arcsin(np.clip(d[:, 1], -1.0, 1.0)) / math.pi + 0.5
    return np.stack([u * repeat[0], v * repeat[1]], axis=1).astype(np.float32)
