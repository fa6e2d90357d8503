"""Cases and the numpy model of the mesh clip renderer (tests/test_render_cpu.py, tests/test_render_gpu.py).

The model is written from the arithmetic documented in include/m324.h ("Mesh clip rendering"), in numpy int64 / float32, and
shares no code with motion324_amd/render.py or the kernels.  Besides the three buffers it returns what the kernel does not keep:
the number of triangles that cover each pixel (`hits`) and the largest |sum w_i z_i| it met (`peak`, for the int64 bound)."""
import math

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
F32 = np.float32


def identity_view():
    m = np.zeros((3, 4), dtype=np.float32)
    m[0, 0] = m[1, 1] = m[2, 2] = 1.0
    return m


def orbit_view(azimuth, elevation):
    """the documented camera, restated: azimuth degrees around +y, then elevation degrees up; fp64, rounded to fp32"""
    a, e = math.radians(azimuth), math.radians(elevation)
    ca, sa, ce, se = math.cos(a), math.sin(a), math.cos(e), math.sin(e)
    ry = np.array([[ca, 0, -sa], [0, 1, 0], [sa, 0, ca]], dtype=np.float64)
    rx = np.array([[1, 0, 0], [0, ce, -se], [0, se, ce]], dtype=np.float64)
    m = np.zeros((3, 4), dtype=np.float64)
    m[:, :3] = rx @ ry
    return m.astype(np.float32)


def _clamp(v, lo, hi):
    return np.where(v < F32(lo), F32(lo), np.where(v > F32(hi), F32(hi), v)).astype(np.float32)


def model_project(vertices, view, S):
    """(x_sub, y_sub, z_q int64 [T,V], valid bool [T,V], view-space positions fp32 [T,V,3])"""
    v = np.asarray(vertices, dtype=np.float32)
    M = np.asarray(view, dtype=np.float32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        p = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]
        valid = np.isfinite(p[0]) & np.isfinite(p[1]) & np.isfinite(p[2])
        scale = F32(16 * S)
        xs = np.rint(_clamp((p[0] + F32(0.5)) * scale, -131072, 131072))
        ys = np.rint(_clamp((F32(0.5) - p[1]) * scale, -131072, 131072))
        zq = np.rint(_clamp((F32(1.0) - p[2]) * F32(4194304.0), 0, 8388607))
    for a in (xs, ys, zq):
        assert a.dtype == np.float32
    to_int = lambda a: np.where(valid, a, 0).astype(np.int64)
    return to_int(xs), to_int(ys), to_int(zq), valid, np.stack(p, axis=-1).astype(np.float32)


def _edges(x, y):
    """x, y: three int64 values or arrays each -> (A[3], B[3], C[3], |area2|), positive inside"""
    area2 = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    s = np.sign(area2)
    A, B, Cc = [], [], []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        a, b = y[j] - y[k], x[k] - x[j]
        A.append(s * a)
        B.append(s * b)
        Cc.append(-s * (a * x[j] + b * y[j]))
    return A, B, Cc, area2 * s


def _owns(w, A, B):
    return (w > 0) | ((w == 0) & ((A > 0) | ((A == 0) & (B > 0))))


def model_raster(xs, ys, zq, valid, faces, S):
    """keys uint64 [T,S,S], hits int32 [T,S,S], peak: one loop per frame and triangle, its (generously taken) box as arrays"""
    T = xs.shape[0]
    faces = np.asarray(faces, dtype=np.int64)
    keys = np.full((T, S, S), EMPTY, dtype=np.uint64)
    hits = np.zeros((T, S, S), dtype=np.int32)
    peak = 0
    for t in range(T):
        for f, tri in enumerate(faces):
            if not valid[t, tri].all():
                continue
            x = [int(xs[t, i]) for i in tri]
            y = [int(ys[t, i]) for i in tri]
            z = [int(zq[t, i]) for i in tri]
            A, B, Cc, area2 = _edges(x, y)
            if area2 == 0:
                continue
            # one pixel more than the documented box on every side: the box is work distribution, never the result
            x0, x1 = max(((min(x) + 7) >> 4) - 1, 0), min(((max(x) - 8) >> 4) + 1, S - 1)
            y0, y1 = max(((min(y) + 7) >> 4) - 1, 0), min(((max(y) - 8) >> 4) + 1, S - 1)
            if x0 > x1 or y0 > y1:
                continue
            X = (16 * np.arange(x0, x1 + 1, dtype=np.int64) + 8)[None, :]
            Y = (16 * np.arange(y0, y1 + 1, dtype=np.int64) + 8)[:, None]
            w = [np.int64(A[i]) * X + np.int64(B[i]) * Y + np.int64(Cc[i]) for i in range(3)]
            cover = _owns(w[0], A[0], B[0]) & _owns(w[1], A[1], B[1]) & _owns(w[2], A[2], B[2])
            if not cover.any():
                continue
            num = w[0] * z[0] + w[1] * z[1] + w[2] * z[2]
            peak = max(peak, int(np.abs(num[cover]).max()), max(abs(int(c)) for c in Cc))
            zp = num // np.int64(area2)
            key = (zp.astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            box = keys[t, y0:y1 + 1, x0:x1 + 1]
            box[cover] = np.minimum(box[cover], key[cover])
            hits[t, y0:y1 + 1, x0:x1 + 1] += cover
    return keys, hits, peak


def model_shade(keys, xs, ys, pos, faces, view, S, colors=None, normals=None, ambient=0.3, background=(0, 0, 0)):
    """(rgb uint8 [T,S,S,3], face int32 [T,S,S], depth int32 [T,S,S]); every owned pixel of a frame at once, float32 throughout"""
    T = keys.shape[0]
    faces = np.asarray(faces, dtype=np.int64)
    M = np.asarray(view, dtype=np.float32)
    amb = F32(ambient)
    rgb = np.empty((T, S, S, 3), dtype=np.uint8)
    rgb[...] = np.asarray(background, dtype=np.uint8)
    face = np.full((T, S, S), -1, dtype=np.int32)
    depth = np.full((T, S, S), -1, dtype=np.int32)
    for t in range(T):
        py, px = np.nonzero(keys[t] != EMPTY)
        if len(py) == 0:
            continue
        k = keys[t, py, px]
        f = (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
        face[t, py, px] = f
        depth[t, py, px] = (k >> np.uint64(32)).astype(np.int64)
        idx = faces[f]                                            # [n, 3]
        x = [xs[t, idx[:, i]] for i in range(3)]
        y = [ys[t, idx[:, i]] for i in range(3)]
        A, B, Cc, area2 = _edges(x, y)
        X, Y = 16 * px.astype(np.int64) + 8, 16 * py.astype(np.int64) + 8
        area = area2.astype(np.float32)
        b = [(A[i] * X + B[i] * Y + Cc[i]).astype(np.float32) / area for i in range(3)]
        with np.errstate(all="ignore"):
            if normals is None:
                p = [pos[t, idx[:, i]] for i in range(3)]        # [n, 3] each
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
            for c in range(3):
                if colors is None:
                    albedo = np.full(len(py), 0.8, dtype=np.float32)
                else:
                    col = np.asarray(colors, dtype=np.float32)
                    albedo = (b[0] * col[idx[:, 0], c] + b[1] * col[idx[:, 1], c]) + b[2] * col[idx[:, 2], c]
                v = albedo * shade
                v = np.where(v > 0, v, F32(0))
                v = np.where(v < 1, v, F32(1))
                out = np.floor(v * F32(255.0) + F32(0.5))
                assert out.dtype == np.float32 and shade.dtype == np.float32 and b[0].dtype == np.float32
                rgb[t, py, px, c] = out.astype(np.uint8)
    return rgb, face, depth


_MODEL_CACHE = {}


def model_render(vertices, faces, view, S, colors=None, normals=None, ambient=0.3, background=(0, 0, 0), cache_key=None):
    """dict(frames, face, depth, hits, peak).  cache_key: the rasterization (the slow part) of a named case is computed once and
    shared by the tests that shade it differently."""
    vertices = np.asarray(vertices, dtype=np.float32)
    if vertices.ndim == 2:
        vertices = vertices[None]
    hit = _MODEL_CACHE.get(cache_key) if cache_key is not None else None
    if hit is None:
        xs, ys, zq, valid, pos = model_project(vertices, view, S)
        keys, hits, peak = model_raster(xs, ys, zq, valid, faces, S)
        hit = (xs, ys, pos, keys, hits, peak)
        if cache_key is not None:
            _MODEL_CACHE[cache_key] = hit
    xs, ys, pos, keys, hits, peak = hit
    rgb, face, depth = model_shade(keys, xs, ys, pos, faces, view, S, colors, normals, ambient, background)
    return dict(frames=rgb, face=face, depth=depth, hits=hits, peak=peak)


# ------------------------------------------------------------------------------------------------ cases
def pixels_to_model(u, v, S, z=0.0):
    """pixel coordinates (u right, v down; a pixel centre is at +0.5) -> model space under the identity view"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return np.stack([u / S - 0.5, 0.5 - v / S, np.broadcast_to(np.asarray(z, dtype=np.float64), u.shape)], axis=-1).astype(np.float32)


def quad_variants():
    """(name, vertices [4,3], faces [2,3]) of the quad with corners at the pixel centres (2.5, 2.5)..(12.5, 12.5) at S = 16:
    both diagonals, both windings of each triangle, every rotation of its indices"""
    corners = pixels_to_model([2.5, 12.5, 12.5, 2.5], [2.5, 2.5, 12.5, 12.5], 16)
    out = []
    for diag, (ta, tb) in (("02", ((0, 1, 2), (0, 2, 3))), ("13", ((0, 1, 3), (1, 2, 3)))):
        for flip_a in (False, True):
            for flip_b in (False, True):
                for rot in range(3):
                    a = ta[::-1] if flip_a else ta
                    b = tb[::-1] if flip_b else tb
                    a, b = a[rot:] + a[:rot], b[(rot + 1) % 3:] + b[:(rot + 1) % 3]
                    out.append((f"diag{diag}-a{int(flip_a)}b{int(flip_b)}r{rot}", corners, np.array([a, b], dtype=np.int32)))
    return out


def grid_snapped(S, k, seed=324):
    """7 x 7 jittered grid, 72 triangles, rotated in the plane by the k-th seeded angle, then snapped to the half-pixel lattice.
    spacing s = S / 8 >= 2 pixels, jitter 0.12 s, snap 0.25: every vertex moves less than s / 4, so no triangle flips."""
    rng = np.random.default_rng([seed, S, k])
    angle = rng.uniform(0.0, 2.0 * math.pi)
    s = S / 8.0
    g = (np.arange(7) - 3.0) * s
    u, v = np.meshgrid(g, g, indexing="xy")
    u = u + rng.uniform(-0.12, 0.12, u.shape) * s
    v = v + rng.uniform(-0.12, 0.12, v.shape) * s
    ca, sa = math.cos(angle), math.sin(angle)
    ur, vr = ca * u - sa * v + S / 2.0, sa * u + ca * v + S / 2.0
    ur, vr = np.round(ur * 2.0) / 2.0, np.round(vr * 2.0) / 2.0
    faces = []
    for r in range(6):
        for c in range(6):
            i = r * 7 + c
            if (r + c) % 2:
                faces += [(i, i + 1, i + 8), (i, i + 8, i + 7)]
            else:
                faces += [(i, i + 1, i + 7), (i + 1, i + 8, i + 7)]
    return pixels_to_model(ur.reshape(-1), vr.reshape(-1), S), np.array(faces, dtype=np.int32)


def coincident(S, low=3, high=7):
    """ten triangles, the ones at `low` and `high` identical and in front, the rest small ones at the back"""
    rng = np.random.default_rng(7)
    verts, faces = [], []
    for f in range(10):
        if f in (low, high):
            tri = pixels_to_model([1.2, S - 1.7, S / 2.0], [1.3, 2.1, S - 1.4], S, z=0.25)
        else:
            c = rng.uniform(3, S - 3, 2)
            tri = pixels_to_model(c[0] + np.array([-2.0, 2.0, 0.3]), c[1] + np.array([-1.5, -1.0, 2.2]), S, z=-0.5)
        faces.append([3 * f, 3 * f + 1, 3 * f + 2])
        verts.append(tri)
    return np.concatenate(verts), np.array(faces, dtype=np.int32)


def interpenetrating(S):
    """two triangles over the same pixels whose depths cross along a vertical line in the middle"""
    a = pixels_to_model([1.0, S - 1.0, 1.0], [1.0, S / 2.0, S - 1.0], S)
    b = pixels_to_model([S - 1.0, 1.0, S - 1.0], [1.0, S / 2.0, S - 1.0], S)
    a[:, 2] = [0.4, -0.4, 0.4]
    b[:, 2] = [0.4, -0.4, 0.4]
    return np.concatenate([a, b]), np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)


def degenerate(S):
    """one good triangle (face 3) behind three that must draw nothing: zero area, collinear, a repeated index"""
    good = pixels_to_model([2.0, S - 2.0, S / 2.0], [2.0, 3.0, S - 2.0], S, z=-0.2)
    point = pixels_to_model([5.5, 5.5, 5.5], [5.5, 5.5, 5.5], S, z=0.5)
    line = pixels_to_model([1.5, 6.5, 11.5], [1.5, 6.5, 11.5], S, z=0.5)
    verts = np.concatenate([point, line, good])
    return verts, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 7], [6, 7, 8]], dtype=np.int32)


def with_bad_vertex(S, bad=np.nan):
    """a fan of four triangles around vertex 0; vertex 1 is non-finite and belongs to faces 0 and 3 only"""
    verts = pixels_to_model([S / 2.0, 1.0, S - 1.0, S - 1.0, 1.0], [S / 2.0, 1.0, 1.0, S - 1.0, S - 1.0], S)
    verts[1, 1] = bad
    return verts, np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], dtype=np.int32)


def fullscreen():
    """one triangle with vertices 4 units out: the whole screen and far more, so the box is clipped on every side"""
    verts = np.array([[-4.0, -4.0, 0.3], [4.0, -4.0, -0.2], [0.0, 4.0, 0.1]], dtype=np.float32)
    return verts, np.array([[0, 1, 2]], dtype=np.int32)


def icosphere(subdivisions=3):
    """(vertices fp64 [V,3] on the unit sphere, faces int32 [20 * 4^n, 3]); 3 subdivisions: 642 vertices, 1280 faces"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(v, dtype=np.float64) / math.sqrt(1 + t * t) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts), np.array(faces, dtype=np.int32)


def many_small(seed=324):
    """(vertices fp32 [3,642,3], faces [1280,3], colors fp32 [642,3]): an icosphere of radius 0.4 in three poses, each another
    rotation plus a per-vertex wobble"""
    rng = np.random.default_rng(seed)
    base, faces = icosphere(3)
    poses = []
    for _ in range(3):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        poses.append(0.4 * base @ q.T + rng.normal(scale=0.004, size=base.shape))
    return np.stack(poses).astype(np.float32), faces, rng.uniform(0.0, 1.0, (len(base), 3)).astype(np.float32)


def pile(S=32, n=200, seed=5):
    """n near-coincident triangles over the same 8 x 8 pixels: every pixel is fought over by all of them"""
    rng = np.random.default_rng(seed)
    base_u, base_v = np.array([11.3, 20.9, 12.1]), np.array([11.2, 12.4, 20.8])
    verts = []
    for _ in range(n):
        tri = pixels_to_model(base_u + rng.uniform(-0.4, 0.4, 3), base_v + rng.uniform(-0.4, 0.4, 3), S)
        tri[:, 2] = rng.uniform(-1e-5, 1e-5, 3) + rng.choice([0.0, 0.0, 1e-6])
        verts.append(tri)
    return np.concatenate(verts).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)
