"""Cases and the numpy model of the voxeliser tests (tests/test_voxel_cpu.py, tests/test_voxel_gpu.py).  The model is written from
the text of include/m324.h ("Volumetric IoU") in int64 numpy and shares no code with motion324_amd/evaluation.py or the kernels:
snap, the 13 separating axes, the bit layout, the orthographic fill and the counts.  clip_exact is the independent check of the
13-axis rule itself: Sutherland-Hodgman clipping of the triangle to the closed cube in rational arithmetic.

Every case is (vertices fp32 [T,V,3], faces int32 [F,3], resolution, half); R = 16 throughout, so a voxel is 1/16 and a sub-voxel
unit 1/256 of a unit length, and every coordinate below that is a multiple of 1/256 snaps without rounding."""
from fractions import Fraction

import numpy as np

R = 16


def side(resolution, half):
    return 2 * half * resolution


# ------------------------------------------------------------------------------------------------ the model
def snap(vertices, resolution, half):
    """fp32 [T,V,3] -> (q int64 [T,V,3], valid bool [T,V], outside int64 [T])"""
    v = np.asarray(vertices, dtype=np.float32)
    lo, hi = np.float32(-131072), np.float32(131072)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (v + np.float32(half)) * np.float32(16 * resolution)          # two fp32 operations, nothing fused
        c = np.where(s < lo, lo, np.where(s > hi, hi, s))
        q = np.rint(c)                                                    # ties to even
    valid = np.isfinite(v).all(axis=-1)
    q = np.where(valid[..., None], q, 0).astype(np.int64)
    limit = 16 * side(resolution, half)
    outside = (valid & ((q < 0) | (q > limit)).any(axis=-1)).sum(axis=-1).astype(np.int64)
    return q, valid, outside


def overlap(tri, centres):
    """tri int64 [3,3] (vertex, coordinate), centres int64 [N,3] -> bool [N]: no axis of the 13 separates"""
    tri = np.asarray(tri, dtype=np.int64)
    v = tri[None, :, :] - np.asarray(centres, dtype=np.int64)[:, None, :]          # v'_m, [N, 3, 3]
    e = np.stack([tri[1] - tri[0], tri[2] - tri[1], tri[0] - tri[2]])
    separated = np.zeros(len(v), dtype=bool)
    for a in range(3):
        separated |= (v[:, :, a].min(axis=1) > 8) | (v[:, :, a].max(axis=1) < -8)
    n = np.cross(e[0], e[1])
    separated |= np.abs((v[:, 0, :] * n).sum(axis=1)) > 8 * np.abs(n).sum()
    for m in range(3):
        for u in np.eye(3, dtype=np.int64):
            a = np.cross(e[m], u)
            p = (v * a).sum(axis=2)
            r = 8 * np.abs(a).sum()
            separated |= (p.min(axis=1) > r) | (p.max(axis=1) < -r)
    return ~separated


def voxelize(vertices, faces, resolution, half):
    """(occupancy bool [T,G,G,G] indexed [t,k,j,i], outside int64 [T]).  Only voxels within two of the triangle's bounding box are
    tested: every other one is separated by a cube axis."""
    q, valid, outside = snap(vertices, resolution, half)
    G = side(resolution, half)
    occ = np.zeros((len(q), G, G, G), dtype=bool)
    for t in range(len(q)):
        for f in np.asarray(faces, dtype=np.int64).reshape(-1, 3):
            if not valid[t, f].all():
                continue
            tri = q[t, f]
            lo = np.clip((tri.min(axis=0) >> 4) - 2, 0, G)
            hi = np.clip((tri.max(axis=0) >> 4) + 3, 0, G)
            if (lo >= hi).any():
                continue
            i, j, k = np.meshgrid(np.arange(lo[0], hi[0]), np.arange(lo[1], hi[1]), np.arange(lo[2], hi[2]), indexing="ij")
            ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
            hit = ijk[overlap(tri, 16 * ijk + 8)]
            occ[t, hit[:, 2], hit[:, 1], hit[:, 0]] = True
    return occ, outside


def pack(occ):
    """bool [T,G,G,G] -> int32 [T,G,G,G/32]: voxel i is bit i % 32 of word i / 32 of its row"""
    T, G = occ.shape[0], occ.shape[1]
    bits = occ.reshape(T, G, G, G // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return bits.sum(axis=-1).astype(np.uint32).view(np.int32)


def fill(occ):
    """orthographic fill: E_x & E_y & E_z, each "occupied somewhere at or before AND somewhere at or after" along its axis"""
    out = np.ones_like(occ)
    for axis in (3, 2, 1):
        before = np.maximum.accumulate(occ, axis=axis)
        after = np.flip(np.maximum.accumulate(np.flip(occ, axis=axis), axis=axis), axis=axis)
        out &= before & after
    return out


def counts(a, b):
    """int64 [T,3] = (|A|, |B|, |A & B|) of two bool grids"""
    T = len(a)
    return np.stack([a.reshape(T, -1).sum(axis=1), b.reshape(T, -1).sum(axis=1), (a & b).reshape(T, -1).sum(axis=1)], axis=1).astype(np.int64)


def iou(c):
    """fp64 [T] of integer counts [T,3]; 0.0 where the union is empty"""
    out = []
    for na, nb, nab in np.asarray(c).tolist():
        union = na + nb - nab
        out.append(0.0 if union == 0 else float(np.float64(nab) / np.float64(union)))
    return np.array(out, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ exact clipping
def _clip(poly, axis, sign, bound):
    out = []
    for a in range(len(poly)):
        p, q = poly[a], poly[(a + 1) % len(poly)]
        dp, dq = sign * (p[axis] - bound), sign * (q[axis] - bound)
        if dp >= 0:
            out.append(p)
        if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
            s = dp / (dp - dq)
            out.append(tuple(p[c] + s * (q[c] - p[c]) for c in range(3)))
    return out


def clip_exact(tri, voxel):
    """does the triangle (integer vertices, degenerate or not) meet the closed cube of voxel (i, j, k)?  The polygon is clipped
    against the six closed half spaces in Fractions; it meets the cube iff something is left."""
    poly = [tuple(Fraction(int(x)) for x in p) for p in tri]
    for axis in range(3):
        for sign, bound in ((1, 16 * int(voxel[axis])), (-1, 16 * int(voxel[axis]) + 16)):
            poly = _clip(poly, axis, sign, bound)
            if not poly:
                return False
    return True


def pair_cases(seed=11, count=400):
    """(triangle int64 [3,3], voxel (i, j, k)) pairs around voxel (2, 2, 2) of a small grid: general position, coordinates on
    the cube's face planes (multiples of 16) and centre planes (multiples of 8), collinear and coincident vertices"""
    rng = np.random.default_rng(seed)
    out = []
    for n in range(count):
        kind = n % 8
        if kind == 0:                                           # general position, close by
            tri = rng.integers(0, 81, size=(3, 3))
        elif kind == 1:                                         # every coordinate on a face or centre plane
            tri = 8 * rng.integers(0, 11, size=(3, 3))
        elif kind == 2:                                         # in a face plane of the cube
            tri = rng.integers(0, 81, size=(3, 3))
            tri[:, rng.integers(0, 3)] = 16 * rng.integers(2, 4)
        elif kind == 3:                                         # in a centre plane
            tri = rng.integers(0, 81, size=(3, 3))
            tri[:, rng.integers(0, 3)] = 40
        elif kind == 4:                                         # a segment: two vertices coincide
            tri = 4 * rng.integers(0, 21, size=(3, 3))
            tri[2] = tri[rng.integers(0, 2)]
        elif kind == 5:                                         # collinear, three distinct points
            a, d = rng.integers(0, 41, size=3), rng.integers(-8, 9, size=3)
            tri = np.stack([a, a + 2 * d, a + 5 * d])
        elif kind == 6:                                         # a point, often on the cube's boundary
            tri = np.repeat(8 * rng.integers(2, 9, size=(1, 3)), 3, axis=0)
        else:                                                   # large, far-reaching: edge axes decide
            tri = rng.integers(-400, 481, size=(3, 3))
        out.append((tri.astype(np.int64), (2, 2, 2)))
    return out


# ------------------------------------------------------------------------------------------------ meshes
def _quad(a, b, c, d):
    return [(a, b, c), (a, c, d)]


def box(lo, hi, top=True):
    """the 8 corners and the 12 triangles of an axis-aligned box; top=False leaves the +z face out (an open cup)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(lo, hi)[(n >> c) & 1][c] for c in range(3)] for n in range(8)], dtype=np.float32)      # bit c of n: hi along c
    f = _quad(0, 2, 3, 1) + _quad(0, 1, 5, 4) + _quad(0, 4, 6, 2) + _quad(1, 3, 7, 5) + _quad(2, 6, 7, 3)
    if top:
        f += _quad(4, 5, 7, 6)
    return v, np.array(f, dtype=np.int32)


def sphere(level=2):
    """a subdivided octahedron on the unit sphere: (vertices fp64 [V,3], faces int32 [F,3]), F = 8 * 4^level"""
    v = [np.array(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, dtype=np.int32)


def soup(seed=5, triangles=200, frames=3, half=2):
    """a seeded triangle soup: mostly small triangles, every tenth a large one, a few reaching past the grid"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-half, half, size=(frames, triangles, 1, 3))
    extent = np.where(np.arange(triangles) % 10 == 0, 1.2, 0.15)[None, :, None, None]
    v = (centre + extent * rng.uniform(-1, 1, size=(frames, triangles, 3, 3))).reshape(frames, triangles * 3, 3)
    return v.astype(np.float32), np.arange(triangles * 3, dtype=np.int32).reshape(triangles, 3)


def _clip_of(*frames):
    return np.stack([np.asarray(f, dtype=np.float32) for f in frames])


def mesh_cases():
    """name -> (vertices fp32 [T,V,3], faces int32 [F,3], resolution, half)"""
    one = np.array([[0, 1, 2]], dtype=np.int32)
    nan, inf = np.float32("nan"), np.float32("inf")
    cases = {}
    cases["no_faces"] = (_clip_of([[0.1, 0.2, 0.3], [0.5, 0.1, -0.2], [-0.3, 0.4, 0.1]]), np.zeros((0, 3), dtype=np.int32), R, 1)
    cases["one_face"] = (_clip_of([[-0.41, -0.33, 0.12], [0.52, -0.2, 0.31], [0.07, 0.61, -0.45]]), one, R, 1)
    # z = 0 is the plane between layers k = 31 and k = 32 of the 64 grid: both are marked
    cases["between_layers"] = (_clip_of([[-0.7, -0.5, 0.0], [0.9, -0.3, 0.0], [0.1, 0.8, 0.0]]), one, R, 2)
    # vertex 0 sits on the corner shared by eight voxels; frame 1 moves it half a sub-voxel unit, a tie that rounds to even
    cases["corner_vertex"] = (_clip_of([[0.25, -0.125, 0.5], [0.61, 0.2, 0.73], [0.3, 0.4, 0.9]],
                                       [[0.25 + 1 / 512, -0.125 - 1 / 512, 0.5 + 3 / 512], [0.61, 0.2, 0.73], [0.3, 0.4, 0.9]]), one, R, 1)
    cases["segment"] = (_clip_of([[-0.8, -0.6, -0.7], [0.7, 0.5, 0.9], [0.7, 0.5, 0.9]]), one, R, 1)
    cases["point"] = (_clip_of([[0.3, -0.2, 0.1]] * 3, [[0.25, 0.25, 0.25]] * 3, [[-1.0, -1.0, -1.0]] * 3), one, R, 1)
    two = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    quad = [[-0.5, -0.5, 0.1], [0.5, -0.5, 0.2], [-0.5, 0.5, 0.3], [0.5, 0.5, 0.4]]
    bad0, bad3 = [list(p) for p in quad], [list(p) for p in quad]
    bad0[0][1] = nan                                    # kills face 0 only
    bad3[3][2] = inf                                    # kills face 1 only
    cases["non_finite"] = (_clip_of(quad, bad0, bad3), two, R, 1)
    # frame 0 reaches past +x and -y, frame 1 lies wholly beyond +z, frame 2 touches the grid's far faces from outside
    cases["outside"] = (_clip_of([[0.2, -1.4, 0.1], [1.7, 0.3, 0.2], [-0.4, 0.6, -0.3]], [[0.1, 0.2, 1.5], [0.6, -0.3, 1.8], [-0.2, 0.5, 2.5]],
                                 [[1.0, 0.0, 0.0], [1.0, 0.5, 0.5], [1.5, 0.2, 0.1]]), one, R, 1)
    # vertices hundreds of units away: x and y are clamped to +-131072 sub-voxel units, and the projections pass 2^32
    cases["far"] = (_clip_of([[-400.0, -300.0, -0.9], [500.0, -200.0, 0.3], [10.0, 450.0, 0.8]], [[3e38, -3e38, 0.0], [-3e38, -3e38, 0.5], [0.3, 3e38, -0.5]]),
                    one, R, 1)
    cases["whole_grid"] = (_clip_of([[-2.5, -2.2, -1.9], [2.4, -1.7, 0.3], [-0.6, 2.3, 2.1]]), one, R, 2)
    v, f = soup()
    cases["soup"] = (v, f, R, 2)
    return cases


def fill_cases():
    """name -> (vertices [1,V,3], faces, R, 2) in a grid of 64: a closed box shell; the same box without its top (an open cup); and
    the cup with a lid over the half x < -0.05 of its top"""
    lo, hi = (-0.55, -0.4, -0.3), (0.45, 0.35, 0.5)
    v, f = box(lo, hi)
    cv, cf = box(lo, hi, top=False)
    lid = np.array([[lo[0], lo[1], hi[2]], [-0.05, lo[1], hi[2]], [-0.05, hi[1], hi[2]], [lo[0], hi[1], hi[2]]], dtype=np.float32)
    lv, lf = np.concatenate([cv, lid]), np.concatenate([cf, np.array(_quad(8, 9, 10, 11), dtype=np.int32)])
    return {"shell": (v[None], f, R, 2), "cup": (cv[None], cf, R, 2), "half_lid": (lv[None], lf, R, 2)}


def sequence_clip():
    """(gt [4,V,3] fp32, gt_faces, pred [4,V,3] fp32, pred_faces): a deforming ellipsoid of 66 vertices and a prediction of it,
    slightly rotated, shifted and scaled -- small enough for ICP and the model to take a moment"""
    import eval_inputs
    v, faces = sphere(2)
    frames = np.stack([v * (1.0 + 0.08 * f * np.sin(3.0 * v[:, :1] + 0.5 * f)) * np.array([1.0, 0.8, 0.7]) for f in range(4)])
    pred = 1.7 * (frames @ eval_inputs._rotation(3.0, -2.0).T) + np.array([0.4, -0.1, 0.2])
    return frames.astype(np.float32), faces.astype(np.int64), pred.astype(np.float32), faces[::-1].astype(np.int64).copy()
