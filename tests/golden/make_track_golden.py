#!/usr/bin/env python3
"""Golden of the tracked surface samples, produced by executing the reference's OWN `track_with_normal_rgb` and
`sample_texture_color_vectorized` (dataset/dataset_utils.py:19-136), cut out of their file with `ast`, against a stand-in
`trimesh` namespace.

trimesh is not installed here, so the stand-in supplies what the reference asks of it:
  * `sample.sample_surface`: the repository's seeded sampler (preprocess.sample_surface);
  * `triangles.points_to_barycentric` / `barycentric_to_points`: their textbook forms (Cramer's rule on the two edge vectors;
    the weighted sum of the corners);
  * `Trimesh(...).vertex_normals`: the numpy model of tests/track_cases.py.
The golden therefore pins the reference's own PLUMBING, not trimesh's normals: the barycentric weights recomputed from the
point, the einsum interpolation of UVs and normals, the W - 1 / H - 1 texel rule with its clip, the division by 255, the
renormalisation with `norms == 0 -> 1`, the tiling of the colours over the frames, and the dtypes of what comes back.

Inputs: the perturbed icosphere of prestep.npz deformed over T = 4 frames by a seeded smooth displacement, per-corner UVs in
[-0.25, 1.25), a 64 x 48 texture, 3000 samples, seed 17.
Build container only.  Output: tests/golden/track.npz (inputs + the reference's four results)."""
import ast
import os
import sys
import types
from typing import Dict, Tuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import track_cases as tc  # noqa: E402
from motion324_amd import preprocess  # noqa: E402

NUM, SEED, T, TEX_W, TEX_H = 3000, 17, 4, 64, 48


def extract(path, names, ns):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)


def points_to_barycentric(triangles, points):
    e0, e1 = triangles[:, 1] - triangles[:, 0], triangles[:, 2] - triangles[:, 0]
    w = points - triangles[:, 0]
    dot = lambda a, b: (a * b).sum(axis=1)
    d00, d01, d11, d0w, d1w = dot(e0, e0), dot(e0, e1), dot(e1, e1), dot(e0, w), dot(e1, w)
    inv = 1.0 / (d00 * d11 - d01 * d01)
    b1, b2 = (d11 * d0w - d01 * d1w) * inv, (d00 * d1w - d01 * d0w) * inv
    return np.stack([1.0 - b1 - b2, b1, b2], axis=1)


def barycentric_to_points(triangles, barycentric):
    return (triangles * barycentric[:, :, None]).sum(axis=1)


class StubTrimesh:
    def __init__(self, vertices=None, faces=None, process=False):
        self.vertices = None if vertices is None else np.asarray(vertices, dtype=np.float64)
        self.faces = np.asarray(faces)

    @property
    def vertex_normals(self):
        return tc.model_vertex_normals(self.vertices, self.faces, "angle")


trimesh = types.SimpleNamespace(
    Trimesh=StubTrimesh,
    sample=types.SimpleNamespace(sample_surface=lambda mesh, num: preprocess.sample_surface(mesh.vertices, mesh.faces, num, SEED)),
    triangles=types.SimpleNamespace(points_to_barycentric=points_to_barycentric, barycentric_to_points=barycentric_to_points))

blob = np.load(os.path.join(HERE, "prestep.npz"))                  # the perturbed icosphere make_prestep_golden.py built
vertices, faces = blob["in_vertices"].astype(np.float64), blob["in_faces"].astype(np.int64)
frames = tc.clip_of(vertices, T, SEED)
face_uvs = tc.corner_uvs(len(faces), SEED)
texture = tc.texture(SEED, TEX_H, TEX_W)

ns = {"np": np, "torch": torch, "trimesh": trimesh, "Tuple": Tuple, "Dict": Dict}
extract("/root/reference/dataset/dataset_utils.py", {"track_with_normal_rgb", "sample_texture_color_vectorized"}, ns)
points, normals, rgbs, face_indices = ns["track_with_normal_rgb"](StubTrimesh(frames[0], faces), frames, faces, NUM, face_uvs, texture)
assert points.shape == normals.shape == rgbs.shape == (T, NUM, 3) and face_indices.shape == (NUM,)
assert bool((rgbs == rgbs[:1]).all())                               # tiled: one colour per sample, so frame 0 is all there is to keep

# what the draw exercises: samples whose texel coordinate is within 1e-9 of an integer, samples whose UV leaves [0, 1]
r0, r1 = tc.model_weights(NUM, SEED)
x, y, _, _ = tc.model_texels(face_uvs, face_indices, r0, r1, TEX_H, TEX_W)
near = int(((np.abs(x - np.rint(x)) <= 1e-9) | (np.abs(y - np.rint(y)) <= 1e-9)).sum())
outside = int(((x < 0) | (x > TEX_W - 1) | (y < 0) | (y > TEX_H - 1)).sum())
print(f"{near} of {NUM} samples within 1e-9 of a texel border; {outside} with a UV outside [0, 1]")
assert near <= NUM // 1000 and outside > 0

save = {"in_frames": frames, "in_faces": faces, "in_face_uvs": face_uvs, "in_texture": texture, "num": np.int64(NUM), "seed": np.int64(SEED),
        "out_points": points.numpy(), "out_normals": normals.numpy(), "out_rgbs": rgbs.numpy()[0], "out_rgbs_shape": np.array(rgbs.shape),
        "out_face_indices": np.asarray(face_indices)}
np.savez_compressed(os.path.join(HERE, "track.npz"), **save)
print({k: (a.shape, a.dtype) for k, a in save.items()})
