"""Surface sampler, the part that needs no GPU: the C ABI's argument validation and plan query (csrc/surface.hip), the
wrappers' refusals, the numpy model of the CDF (tests/surface_cases.py) against numpy's own cross / norm / cumsum, and the
host paths that must not move."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import surface_cases as sc
from conftest import REPO

SURFACE = ("m324_surface_plan", "m324_surface_cdf", "m324_surface_sample")
P = 4096                                                         # a stand-in address: nothing is dereferenced


def test_surface_entry_points_are_declared_and_bound_at_abi_23():
    from motion324_amd import lib
    text = open(os.path.join(REPO, "include", "m324.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SURFACE:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert lib.ABI_VERSION == 23 and lib.load().m324_abi_version() == 23
    # the two constants of the scan order are published, and the numpy model uses them
    assert int(re.search(r"#define\s+M324_SURFACE_CHUNK\s+(\d+)", header).group(1)) == sc.CHUNK == 16
    assert int(re.search(r"#define\s+M324_SURFACE_BLOCK\s+(\d+)", header).group(1)) == sc.BLOCK == 1024
    from motion324_amd import build
    assert "surface.hip" in build.SOURCES                        # build() and build_sanitized() both walk SOURCES


@pytest.mark.parametrize("n_faces,batch", [(1, 1), (1024, 1), (1025, 1), (8192, 64), (16389, 3), (100003, 32)])
def test_surface_plan_blocks_and_scratch(n_faces, batch):
    from motion324_amd import lib, ops
    need = C.c_long(-1)
    blocks = lib.load().m324_surface_plan(n_faces, batch, C.addressof(need))
    assert blocks == -(-n_faces // sc.BLOCK)
    assert need.value == (batch * blocks * 8 if blocks > 1 else 0)
    assert lib.load().m324_surface_plan(n_faces, batch, None) == blocks                      # the size is optional
    assert ops.surface_plan(n_faces, batch) == (blocks, need.value)


def test_surface_plan_refuses_non_positive_sizes():
    from motion324_amd import lib, ops
    for args in ((0, 1), (-5, 1), (8, 0), (8, -1)):
        assert lib.load().m324_surface_plan(*args, None) == -1, args
        assert "m324_surface_plan" in lib.last_error()
    with pytest.raises(lib.M324Error, match="m324_surface_plan"):
        ops.surface_plan(0, 1)


def test_surface_cdf_validates_before_any_hip_call():
    """every refusal returns -1 with a message on a machine without a GPU: the checks run before the first HIP call"""
    from motion324_amd import lib
    h = lib.load()
    ok = dict(vertices=P, stride=0, nv=8, faces=P, nf=8, batch=1, cdf=P, scratch=None, nbytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return h.m324_surface_cdf(a["vertices"], a["stride"], a["nv"], a["faces"], a["nf"], a["batch"], a["cdf"], a["scratch"], a["nbytes"], None)
    for kw, word in ((dict(vertices=None), "null"), (dict(faces=None), "null"), (dict(cdf=None), "null"),
                     (dict(nv=0), "positive"), (dict(nf=0), "positive"), (dict(nf=-2), "positive"), (dict(batch=0), "positive"),
                     (dict(stride=-3), "positive"),
                     (dict(nf=1025, scratch=None, nbytes=0), "scratch"),
                     (dict(nf=1025, batch=3, scratch=P, nbytes=3 * 2 * 8 - 1), "scratch"),
                     (dict(nf=1025, scratch=None, nbytes=1 << 20), "scratch")):
        assert call(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())


def test_surface_sample_validates_before_any_hip_call():
    from motion324_amd import lib
    h = lib.load()
    ok = dict(vertices=P, stride=0, nv=8, faces=P, nf=8, cdf=P, seeds=P, num=16, batch=1, points=P, points64=None, face=None, normals=None,
              colors=None, vc=None, channels=0, uv=None, texels=None, th=0, tw=0)

    def call(**kw):
        a = dict(ok, **kw)
        return h.m324_surface_sample(a["vertices"], a["stride"], a["nv"], a["faces"], a["nf"], a["cdf"], a["seeds"], a["num"], a["batch"],
                                     a["points"], a["points64"], a["face"], a["normals"], a["colors"], a["vc"], a["channels"], a["uv"],
                                     a["texels"], a["th"], a["tw"], None)
    for kw, word in ((dict(vertices=None), "null"), (dict(faces=None), "null"), (dict(cdf=None), "null"), (dict(seeds=None), "null"),
                     (dict(points=None), "null"),
                     (dict(nv=0), "positive"), (dict(nf=0), "positive"), (dict(num=0), "positive"), (dict(num=-1), "positive"),
                     (dict(batch=0), "positive"), (dict(stride=-1), "positive"),
                     (dict(colors=P, vc=P, channels=2), "channels"), (dict(colors=P, vc=P, channels=5), "channels"),
                     (dict(colors=P, uv=P), "texture"), (dict(colors=P, texels=P, th=4, tw=4), "texture"),
                     (dict(colors=P, uv=P, texels=P, th=0, tw=4), "texture"), (dict(colors=P, uv=P, texels=P, th=4, tw=-1), "texture")):
        assert call(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())


def test_ops_refuse_cpu_tensors():
    from motion324_amd import ops
    from motion324_amd.lib import M324Error
    v, f = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(M324Error, match="HIP device"):
        ops.surface_cdf(v, f)
    with pytest.raises(M324Error, match="HIP device"):
        ops.surface_sample(v, f, torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int64), 8)


def test_the_wrapper_refuses_out_of_range_faces_before_anything_reaches_a_device():
    """the kernels do not check vertex indices; the range check is host arithmetic and comes first, so it is observable here"""
    from motion324_amd import preprocess
    from motion324_amd.lib import M324Error
    v, f = sc.grid_mesh(3, 3)
    for bad in (len(v), -1, 2 ** 31 - 1):
        faces = f.copy()
        faces[5, 1] = bad
        with pytest.raises(M324Error, match="faces index vertices"):
            preprocess.sample_surface_device(v, faces, 16, 0, "cuda")
        with pytest.raises(M324Error, match="faces index vertices"):
            preprocess.sample_pointcloud_with_albedo(v, faces, 16, None, 0, device="cuda")
        with pytest.raises(M324Error, match="faces index vertices"):
            preprocess.sample_surface_device(np.stack([v, v]), faces, 16, [0, 1], "cuda")
    with pytest.raises(M324Error, match=r"integer faces \[F,3\]"):
        preprocess.sample_surface_device(v, f[:, :2], 16, 0, "cuda")


def test_seed_table_holds_the_two_stream_seeds_of_the_host_sampler():
    from motion324_amd import preprocess, synth
    table = preprocess.surface_seeds([0, 7, 2 ** 40 + 3])
    assert table.shape == (3, 2) and table.dtype == np.int64
    for row, seed in zip(table.view(np.uint64), (0, 7, 2 ** 40 + 3)):
        assert row[0] == synth._stream_seed(seed, "surface.face") and row[1] == synth._stream_seed(seed, "surface.bary")
    assert np.array_equal(preprocess.surface_seeds(7), table[1:2])


@pytest.mark.parametrize("mesh", ["grid", "blob", "soup"])
def test_model_areas_equal_numpy_cross_and_norm_bit_for_bit(mesh):
    v, f = {"grid": sc.grid_mesh, "blob": sc.blob, "soup": sc.soup}[mesh]()[:2]
    tri = v[f]
    cross = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    c, ln = sc.model_cross(v, f)
    assert np.array_equal(c, cross) and np.array_equal(ln, np.linalg.norm(cross, axis=1))
    assert np.array_equal(sc.model_areas(v, f), 0.5 * np.linalg.norm(cross, axis=1))
    if mesh == "soup":
        assert len(f) == 8192 and len(v) == 4098 and 600 < np.count_nonzero(ln == 0) < 1000          # about 10 % degenerate
    if mesh == "grid":
        assert len(f) == 1058 and np.all(ln > 0)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 1024, 1025, 2049, 16389, 100003])
def test_model_cdf_is_monotone_and_repeats_across_zero_areas(n):
    rng = np.random.default_rng(n)
    area = np.abs(rng.normal(size=n)) * 10.0 ** rng.integers(-6, 3, size=n)
    area[rng.random(n) < 0.1] = 0.0
    cdf = sc.model_cdf(area)
    assert cdf.shape == (n,) and cdf[0] == area[0] and np.all(np.diff(cdf) >= 0)
    zero = np.nonzero(area[1:] == 0)[0] + 1
    assert np.array_equal(cdf[zero], cdf[zero - 1])
    assert abs(cdf[-1] - np.sum(area)) <= n * 2.0 ** -53 * np.sum(area)


@pytest.mark.parametrize("nx,ny,seed", [(23, 23, 0), (23, 23, 5), (1, 1, 1), (8, 1, 2), (40, 13, 3), (91, 91, 4)])
def test_model_cdf_equals_cumsum_exactly_on_grid_meshes(nx, ny, seed):
    v, f = sc.grid_mesh(nx, ny, seed)
    area = sc.model_areas(v, f)
    assert len(f) == 2 * nx * ny and np.all(area * 8192 == np.rint(area * 8192))          # multiples of 2^-13: exact dyadics
    assert np.array_equal(sc.model_cdf(area), np.cumsum(area))


def test_general_meshes_have_no_draw_near_a_cdf_entry():
    """the GPU tests allow a face mismatch only for draws within rounding of a CDF entry, and at most 0.1 % of them; on the
    committed inputs there is none, and the model's nested scan picks the host's face for every draw"""
    from motion324_amd import preprocess, synth
    for (v, f, _), num in ((sc.blob(), 4096), (sc.soup(), 50000)):
        assert not sc.near_cdf_entry(v, f, num, 5).any()
        cdf = sc.model_cdf(sc.model_areas(v, f))
        u = synth.uniform(5, "surface.face", (num,)).astype(np.float64)
        model = np.minimum(np.searchsorted(cdf, u * cdf[-1], side="right"), len(f) - 1)
        assert np.array_equal(model, preprocess.sample_surface(v, f, num, 5)[1])


def test_host_albedo_path_is_unchanged_and_refuses_a_texture():
    from motion324_amd import preprocess
    from motion324_amd.lib import M324Error
    v, f, colors = sc.blob()
    pts, nrm, rgb = preprocess.sample_pointcloud_with_albedo(v, f, 200, colors, 11)
    p64, fi = preprocess.sample_surface(v, f, 200, 11)
    assert np.array_equal(pts, p64.astype(np.float32)) and np.array_equal(nrm, preprocess.face_normals(v, f)[fi].astype(np.float32))
    assert np.array_equal(rgb, (colors[:, :3] / 255.0)[f[fi]].mean(axis=1).astype(np.float32))
    again = preprocess.sample_pointcloud_with_albedo(v, f, 200, colors, 11, uv=None, texture=None, device=None)
    assert all(np.array_equal(a, b) for a, b in zip(again, (pts, nrm, rgb)))
    assert np.all(preprocess.sample_pointcloud_with_albedo(v, f, 50, None, 11)[2] == 0.5)
    with pytest.raises(M324Error, match="device="):
        preprocess.sample_pointcloud_with_albedo(v, f, 50, None, 11, uv=np.zeros((len(v), 2)), texture=np.zeros((4, 4, 3), dtype=np.uint8))


def test_evaluate_sequence_host_sampler_is_the_default(monkeypatch):
    """sampler="host" hands the metrics exactly the points the call without the argument hands them (the metrics themselves
    need a GPU: they are replaced by a recorder here); an unknown sampler is refused"""
    from motion324_amd import evaluation as ev
    from motion324_amd.lib import M324Error
    v, f, _ = sc.blob()
    gt = np.stack([v * (1.0 + 0.05 * k) for k in range(3)]).astype(np.float32)
    pred = (1.3 * gt + 0.2).astype(np.float32)
    seen = []

    def record(points1, points2, threshold=0.02):
        seen.append((np.array(points1), np.array(points2), threshold))
        n = len(points1)
        return torch.arange(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    monkeypatch.setattr(ev, "chamfer_and_fscore", record)
    alignment = (np.eye(3), np.array([0.01, 0.0, -0.02]), 1.01)
    a = ev.evaluate_sequence(gt, f, pred, f[::-1].copy(), num_samples=300, seed=4, alignment=alignment)
    b = ev.evaluate_sequence(gt, f, pred, f[::-1].copy(), num_samples=300, seed=4, alignment=alignment, sampler="host")
    assert len(seen) == 2 and seen[0][0].shape == (3, 300, 3) and seen[0][0].dtype == np.float32
    assert np.array_equal(seen[0][0], seen[1][0]) and np.array_equal(seen[0][1], seen[1][1]) and seen[0][2] == seen[1][2]
    assert a["chamfer_distances"] == b["chamfer_distances"] and a["fscores"] == b["fscores"]
    with pytest.raises(M324Error, match="sampler"):
        ev.evaluate_sequence(gt, f, pred, f, num_samples=300, seed=4, alignment=alignment, sampler="gpu")
    with pytest.raises(SystemExit):
        ev.main(["--gt_path", "a", "--pred_path", "b", "--sampler", "gpu"])
