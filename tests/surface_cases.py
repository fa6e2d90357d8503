"""Inputs of the surface-sampler tests and a numpy model of what csrc/surface.hip computes (include/m324.h, "Surface
sampling"): the area formula, the nested scan of the CDF, and the bookkeeping of the two exemptions the GPU tests allow
(a draw within rounding of a CDF entry; a texture coordinate within rounding of a texel border).  No GPU, no product code
beyond motion324_amd.synth's streams and the host sampler the device is compared with."""
import os

import numpy as np

from conftest import GOLDEN
from motion324_amd import synth

CHUNK, BLOCK = 16, 1024          # M324_SURFACE_CHUNK, M324_SURFACE_BLOCK (test_surface_cpu.py compares them with the header)


# ------------------------------------------------------------------------------------------------ numpy model
def model_cross(vertices, faces):
    """(c, |c|) of every face, written out: c = e1 x e2 component by component, |c| = sqrt((cx*cx + cy*cy) + cz*cz)"""
    v = np.asarray(vertices, dtype=np.float64)
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.stack([cx, cy, cz], axis=1), np.sqrt((cx * cx + cy * cy) + cz * cz)


def model_areas(vertices, faces):
    return 0.5 * model_cross(vertices, faces)[1]


def _exclusive(totals):
    """sequential exclusive prefix: 0, t0, t0 + t1, (t0 + t1) + t2, ..."""
    out = np.zeros(len(totals), dtype=np.float64)
    run = 0.0
    for k in range(1, len(totals)):
        run = totals[k - 1] if k == 1 else run + totals[k - 1]
        out[k] = run
    return out


def model_cdf(area):
    """cdf = fl(B + fl(W + p)): p the sequential inclusive prefix inside chunks of 16 faces, W the sequential exclusive prefix of
    the chunk totals inside blocks of 1024 faces, B the sequential exclusive prefix of the block totals"""
    area = np.asarray(area, dtype=np.float64)
    n = len(area)
    local = np.empty(n, dtype=np.float64)                  # L = W + p
    block_totals = []
    for b0 in range(0, n, BLOCK):
        blk = area[b0:b0 + BLOCK]
        starts = range(0, len(blk), CHUNK)
        prefixes = [np.cumsum(blk[c0:c0 + CHUNK]) for c0 in starts]          # np.cumsum is one sequential chain
        W = _exclusive(np.array([p[-1] for p in prefixes]))
        for c0, p, w in zip(starts, prefixes, W):
            local[b0 + c0:b0 + c0 + len(p)] = w + p
        block_totals.append(local[min(b0 + BLOCK, n) - 1])
    B = _exclusive(np.array(block_totals))
    return np.concatenate([B[k] + local[k * BLOCK:(k + 1) * BLOCK] for k in range(len(B))])


# ------------------------------------------------------------------------------------------------ meshes
def grid_mesh(nx=23, ny=23, seed=0):
    """nx x ny uneven cells, two axis-aligned right triangles each, on coordinates that are multiples of 1/64: every area and
    every partial sum of areas is an exact dyadic number, so every summation order gives the same CDF.  The face list depends
    on (nx, ny) only; the seed moves the vertices."""
    wx = 1 + (synth.uniform(seed, "surface.grid.x", (nx,)) * 8).astype(np.int64)
    wy = 1 + (synth.uniform(seed, "surface.grid.y", (ny,)) * 8).astype(np.int64)
    xs = np.concatenate([[0], np.cumsum(wx)]) / 64.0 - 0.5
    ys = np.concatenate([[0], np.cumsum(wy)]) / 64.0 - 0.25
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    vertices = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, (seed % 7) / 64.0)], axis=1)
    at = lambda i, j: i * (ny + 1) + j
    faces = []
    for i in range(nx):
        for j in range(ny):
            faces += [[at(i, j), at(i + 1, j), at(i, j + 1)], [at(i + 1, j + 1), at(i, j + 1), at(i + 1, j)]]
    return vertices, np.array(faces, dtype=np.int64)


def blob():
    """the perturbed icosphere of the prestep golden (162 vertices, 320 faces) with its vertex colours"""
    g = np.load(os.path.join(GOLDEN, "prestep.npz"))
    return g["in_vertices"].astype(np.float64), g["in_faces"].astype(np.int64), g["in_vertex_colors"]


def random_mesh(n_faces, n_vertices, seed, degenerate=0.1):
    """random triangles over random vertices; about `degenerate` of the faces have no area (a repeated vertex)"""
    vertices = synth.uniform(seed, "surface.soup.v", (n_vertices, 3), -0.5, 0.5).astype(np.float64)
    vertices += 1e-3 * synth.normal(seed, "surface.soup.jitter", (n_vertices, 3)).astype(np.float64)          # off the fp32 grid
    faces = np.minimum((synth.uniform(seed, "surface.soup.f", (n_faces, 3)).astype(np.float64) * n_vertices).astype(np.int64), n_vertices - 1)
    flat = synth.uniform(seed, "surface.soup.flat", (n_faces,)) < degenerate
    faces[flat, 2] = faces[flat, 1]
    return vertices, faces


def soup():
    """8192 random faces over 4098 vertices, about 10 % of them degenerate, with vertex colours"""
    vertices, faces = random_mesh(8192, 4098, 21)
    colors = (synth.uniform(21, "surface.soup.vc", (len(vertices), 4)) * 255).astype(np.uint8)
    return vertices, faces, colors


# ------------------------------------------------------------------------------------------------ exemptions
def near_cdf_entry(vertices, faces, num, seed):
    """bool [num]: draws of the HOST sampler whose u * total lies within 4 F 2^-53 total of a host CDF entry -- the only draws
    for which another summation order of the areas (each order is within F 2^-53 total of the exact sums) may pick another face"""
    tri = np.asarray(vertices, dtype=np.float64)[faces]
    cum = np.cumsum(0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1))
    target = synth.uniform(seed, "surface.face", (num,)).astype(np.float64) * cum[-1]
    at = np.searchsorted(cum, target)
    gap = np.minimum(np.abs(cum[np.minimum(at, len(cum) - 1)] - target), np.abs(cum[np.maximum(at - 1, 0)] - target))
    return gap <= 4.0 * len(faces) * 2.0 ** -53 * cum[-1]


def texel_coordinates(vertices, faces, uv, fi, num, seed, tex_h, tex_w):
    """fp64 restatement of the texture lookup of include/m324.h for the samples the host sampler drew on faces `fi`: the drawn
    weights (1 - r0 - r1, r0, r1), 1/3 each on a face without area, uv = sum w_k (uv_k mod 1).
    Returns (x = uv.x * W, y = (1 - uv.y) * H, column, row)."""
    r = synth.uniform(seed, "surface.bary", (num, 2)).astype(np.float64)
    flip = r.sum(axis=1) > 1.0
    r[flip] = 1.0 - r[flip]
    w = np.stack([(1.0 - r[:, 0]) - r[:, 1], r[:, 0], r[:, 1]], axis=1)
    w[model_cross(vertices, faces)[1][fi] == 0.0] = 1.0 / 3.0
    tri_uv = (np.asarray(uv, dtype=np.float64) % 1.0)[faces[fi]]                                       # [num, 3, 2]
    s = (w[:, 0:1] * tri_uv[:, 0] + w[:, 1:2] * tri_uv[:, 1]) + w[:, 2:3] * tri_uv[:, 2]
    x, y = s[:, 0] * tex_w, (1.0 - s[:, 1]) * tex_h
    return x, y, np.clip(x, 0, tex_w - 1).astype(np.int64), np.clip(y, 0, tex_h - 1).astype(np.int64)


def near_texel_border(x, y, eps=1e-9):
    """bool [num]: samples whose texel coordinate lies within eps of an integer, where another rounding of the weights may
    land in the neighbouring texel"""
    return (np.abs(x - np.rint(x)) <= eps) | (np.abs(y - np.rint(y)) <= eps)
