#!/usr/bin/env python3
"""Golden of the texture colour source of the surface sampler, produced by executing the reference's OWN
`sample_pointcloud_with_albedo` and `barycentric_coords` (utils/mesh_processing.py:102-191), cut out of their file with `ast`,
on a stand-in mesh object.

The stand-in is the perturbed icosphere of make_prestep_golden.py.  Its `.sample()` is the repo's deterministic sampler, it
has no usable vertex colours (so the reference falls through to its second source), `.visual.uv` holds per-vertex UVs that
reach outside [0, 1) (the reference wraps them), and `.visual.material.baseColorTexture` is a 64 x 48 RGB PIL image of seeded
bytes.  Everything downstream of the sampler -- the barycentric weights recomputed from the point, the UV interpolation, the
texel lookup, dtypes -- is the reference's code, its Python loop per sample included.
Build container only.  Output: tests/golden/sampler_tex.npz (inputs + the reference's colours)."""
import ast
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from motion324_amd import preprocess, synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NUM, SEED, TEX_W, TEX_H = 3000, 17, 64, 48


def extract(path, names, ns):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)


class StubMesh:
    def __init__(self, vertices, faces, uv, image, seed):
        self.vertices = vertices
        self.faces = faces
        self.visual = types.SimpleNamespace(vertex_colors=np.zeros((0, 4), dtype=np.uint8), uv=uv,
                                            material=types.SimpleNamespace(baseColorTexture=image))
        self._seed = seed

    @property
    def face_normals(self):
        return preprocess.face_normals(self.vertices, self.faces)

    @property
    def triangles(self):
        return np.asarray(self.vertices)[self.faces]

    def sample(self, num, return_index=False):
        pts, fi = preprocess.sample_surface(self.vertices, self.faces, num, self._seed)
        return (pts, fi) if return_index else pts


blob = np.load(os.path.join(HERE, "prestep.npz"))                  # the perturbed icosphere make_prestep_golden.py built
vertices, faces = blob["in_vertices"].astype(np.float64), blob["in_faces"].astype(np.int64)
uv = synth.uniform(SEED, "sampler.uv", (len(vertices), 2), -0.75, 1.75).astype(np.float64)
uv += 1e-4 * synth.normal(SEED, "sampler.uv.jitter", uv.shape).astype(np.float64)                     # off the fp32 grid
texture = (synth.uniform(SEED, "sampler.texture", (TEX_H, TEX_W, 3)) * 256).astype(np.uint8)
mesh = StubMesh(vertices, faces, uv, Image.fromarray(texture, "RGB"), SEED)

ns = {"np": np, "torch": torch, "Image": Image, "print": lambda *a, **k: None}
extract("/root/reference/utils/mesh_processing.py", {"sample_pointcloud_with_albedo", "barycentric_coords"}, ns)
points, normals, colors = ns["sample_pointcloud_with_albedo"](mesh, NUM)
assert colors.shape == (NUM, 3) and not np.all(colors.numpy() == 0.5)      # the texture branch ran, not the grey one

save = {"in_vertices": vertices, "in_faces": faces, "in_uv": uv, "in_texture": texture, "num": np.int64(NUM), "seed": np.int64(SEED),
        "out_points": points.numpy(), "out_normals": normals.numpy(), "out_colors": colors.numpy()}
np.savez_compressed(os.path.join(HERE, "sampler_tex.npz"), **save)
print({k: (a.shape, a.dtype) for k, a in save.items()})
