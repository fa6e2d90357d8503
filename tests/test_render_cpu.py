"""Mesh clip renderer without a GPU: the integer rules of include/m324.h on the numpy model (known answers), the host side
of the C ABI (every refusal comes before the first HIP call), the view matrix and the refusals of the Python layers."""
import ctypes

import numpy as np
import pytest
import torch

import render_cases as rc
from motion324_amd import lib, ops, render
from motion324_amd.lib import M324Error


def owned(result):
    return result["face"][0] >= 0


# ------------------------------------------------------------------------------------------------ the rules, on the model
@pytest.mark.parametrize("name,vertices,faces", rc.quad_variants(), ids=[v[0] for v in rc.quad_variants()])
def test_quad_centres(name, vertices, faces):
    r = rc.model_render(vertices, faces, rc.identity_view(), 16)
    want = np.zeros((16, 16), dtype=np.int32)
    want[2:12, 2:12] = 1
    assert np.array_equal(r["hits"][0], want) and want.sum() == 100
    assert np.array_equal(r["depth"][0], np.where(want == 1, 4194304, -1))
    assert np.array_equal(owned(r), want == 1)


@pytest.mark.parametrize("S", [16, 33])
def test_grid_snapped_never_draws_a_pixel_twice(S):
    on_edge = 0
    for k in range(20):
        vertices, faces = rc.grid_snapped(S, k)
        assert faces.shape == (72, 3)
        r = rc.model_render(vertices, faces, rc.identity_view(), S)
        assert r["hits"].max() == 1, (S, k)
        # the interior of the grid has no holes either: every pixel well inside its hull is drawn exactly once
        c = S // 2
        assert (r["hits"][0, c - 2:c + 2, c - 2:c + 2] == 1).all(), (S, k)
        xs, ys, _, _, _ = rc.model_project(vertices[None], rc.identity_view(), S)
        on_edge += int(((xs % 16 == 8) & (ys % 16 == 8)).sum())
    assert on_edge > 100         # the lattice does put vertices on pixel centres: the tie rules are what is being tested


@pytest.mark.parametrize("S", [16, 33])
def test_coincident_triangles_go_to_the_lower_index(S):
    for low, high in ((3, 7), (2, 8)):
        vertices, faces = rc.coincident(S, low, high)
        r = rc.model_render(vertices, faces, rc.identity_view(), S)
        front = r["depth"][0] == r["depth"][0][r["face"][0] == low].min()
        assert (r["hits"][0][r["face"][0] == low] >= 2).all() and (r["face"][0] == low).sum() > S
        assert not (r["face"][0] == high).any()
        swapped = faces.copy()
        swapped[[low, high]] = swapped[[high, low]]
        r2 = rc.model_render(vertices, swapped, rc.identity_view(), S)
        assert np.array_equal(r2["face"], r["face"]) and np.array_equal(r2["depth"], r["depth"]) and front.any()


@pytest.mark.parametrize("S", [16, 33])
def test_interpenetrating_triangles_split_along_their_intersection(S):
    vertices, faces = rc.interpenetrating(S)
    r = rc.model_render(vertices, faces, rc.identity_view(), S)
    both = r["hits"][0] == 2
    assert both.sum() > S
    cols = np.nonzero(both)[1]
    face = r["face"][0]
    # face 0 is nearer (smaller depth) where its z is larger: on the left of the crossing line x = S / 2, face 1 on the right
    assert (face[both][cols < S // 2 - 1] == 0).all() and (face[both][cols > S // 2 + 1] == 1).all()
    assert (face[both] == 0).any() and (face[both] == 1).any()


@pytest.mark.parametrize("S", [16, 33])
def test_degenerate_triangles_draw_nothing(S):
    vertices, faces = rc.degenerate(S)
    r = rc.model_render(vertices, faces, rc.identity_view(), S)
    assert set(np.unique(r["face"])) == {-1, 3} and r["hits"].max() == 1


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_vertex_removes_exactly_its_own_triangles(bad):
    S = 16
    vertices, faces = rc.with_bad_vertex(S, bad)
    r = rc.model_render(vertices, faces, rc.identity_view(), S)
    clean, _ = rc.with_bad_vertex(S, 0.4)
    clean[1] = rc.pixels_to_model([1.0], [1.0], S)[0]
    full = rc.model_render(clean, faces, rc.identity_view(), S)
    assert set(np.unique(r["face"])) == {-1, 1, 2} and set(np.unique(full["face"])) == {-1, 0, 1, 2, 3}
    keep = np.isin(full["face"], (1, 2))
    assert np.array_equal(r["face"][keep], full["face"][keep]) and (r["face"][~keep] == -1).all()


def test_far_vertices_clamp_and_stay_inside_int64():
    S = 1024
    vertices = np.array([[-1e6, -1e6, 1e6], [1e6, -1e6, -1e6], [0.0, 1e6, 0.0]], dtype=np.float32)
    xs, ys, zq, valid, _ = rc.model_project(vertices[None], rc.identity_view(), S)
    assert valid.all() and set(np.abs(xs).ravel()) <= {0, 2 ** 17, 8192} and np.abs(ys).max() == 2 ** 17
    assert xs.min() == -2 ** 17 and xs.max() == 2 ** 17 and zq.min() == 0 and zq.max() == 2 ** 23 - 1
    r = rc.model_render(vertices, np.array([[0, 1, 2]], dtype=np.int32), rc.identity_view(), S)
    assert 0 < r["peak"] <= 2 ** 60 and (r["face"] == 0).all()
    assert r["depth"].min() >= 0 and r["depth"].max() <= 2 ** 23 - 1


# ------------------------------------------------------------------------------------------------ view matrix
def test_view_matrix_is_orthonormal_and_the_identity_at_zero():
    assert np.array_equal(render.view_matrix(0.0, 0.0), rc.identity_view())
    for az, el in ((30.0, 0.0), (0.0, 45.0), (123.0, -37.0), (-270.0, 89.0)):
        m = render.view_matrix(az, el)
        assert m.dtype == np.float32 and m.shape == (3, 4) and not m[:, 3].any()
        r = m[:, :3].astype(np.float64)
        assert np.allclose(r @ r.T, np.eye(3), atol=3e-7) and abs(np.linalg.det(r) - 1.0) < 1e-6
        assert np.array_equal(m, rc.orbit_view(az, el))
    # azimuth 90 puts the camera on +x: the model's +x axis points at the viewer
    assert np.allclose(render.view_matrix(90.0, 0.0)[:, :3] @ np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 1.0], atol=1e-7)
    assert np.allclose(render.view_matrix(0.0, 90.0)[:, :3] @ np.array([0.0, 1.0, 0.0]), [0.0, 0.0, 1.0], atol=1e-7)


# ------------------------------------------------------------------------------------------------ C ABI, host side
def _plan(nv, nf, frames, size):
    need = ctypes.c_long(-7)
    return lib.load().m324_render_plan(nv, nf, frames, size, ctypes.addressof(need)), need.value


def test_plan_reports_scratch_and_refuses_bad_sizes():
    rcode, need = _plan(642, 1280, 3, 64)
    assert rcode == 0 and need >= 3 * (64 * 64 * 8 + 642 * 28 + 1280 * 4)
    assert _plan(642, 1280, 6, 64)[1] > need
    assert lib.load().m324_render_plan(3, 1, 1, 1, None) == 0
    for args, word in (((3, 1, 1, 0), "size"), ((3, 1, 1, 1025), "size"), ((3, 1, 0, 16), "frames"), ((3, 1, -2, 16), "frames"),
                       ((3, -1, 1, 16), "n_faces"), ((0, 1, 1, 16), "n_vertices"), ((3, 2 ** 30, 4, 16), "2^31")):
        rcode, need = _plan(*args)
        assert rcode == -1 and need == -7 and word in lib.last_error(), (args, lib.last_error())
    assert _plan(3, 1, 1, 1024)[0] == 0


def _launchers(nv=3, nf=1, frames=1, size=16, ptr=4096, scratch=4096, nbytes=1 << 40):
    """the three launch entry points with plausible (never dereferenced) pointers; every call must be refused"""
    h = lib.load()
    view = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    vp = ctypes.addressof(view)
    return (("m324_render_project", lambda: h.m324_render_project(ptr, nv * 3, nv, nf, frames, vp, size, scratch, nbytes, None)),
            ("m324_render_raster", lambda: h.m324_render_raster(ptr, nf, nv, frames, size, 64, scratch, nbytes, None)),
            ("m324_render_shade", lambda: h.m324_render_shade(ptr, nf, nv, frames, size, None, None, 0, vp, 0.3, 0, ptr, ptr, ptr, scratch, nbytes, None)))


@pytest.mark.parametrize("kwargs,word", [(dict(size=0), "size"), (dict(size=1025), "size"), (dict(frames=0), "frames"), (dict(frames=-1), "frames"),
                                         (dict(nf=-1), "n_faces"), (dict(ptr=None), "null"), (dict(scratch=None), "null"),
                                         (dict(nbytes=64), "scratch bytes"), (dict(scratch=4104), "aligned")])
def test_launch_entry_points_refuse_before_any_hip_call(kwargs, word):
    for name, call in _launchers(**kwargs):
        assert call() == -1, name
        assert name in lib.last_error() and word in lib.last_error(), lib.last_error()


def test_launch_entry_points_refuse_their_own_arguments():
    h = lib.load()
    view = (ctypes.c_float * 12)()
    vp = ctypes.addressof(view)
    big = 1 << 40
    assert h.m324_render_project(4096, -3, 3, 1, 1, vp, 16, 4096, big, None) == -1 and "stride_t" in lib.last_error()
    assert h.m324_render_project(4096, 9, 3, 1, 1, None, 16, 4096, big, None) == -1 and "null" in lib.last_error()
    assert h.m324_render_raster(4096, 1, 3, 1, 16, -1, 4096, big, None) == -1 and "big_pixels" in lib.last_error()
    assert h.m324_render_shade(4096, 1, 3, 1, 16, None, None, 0, vp, 0.3, 0, None, None, None, 4096, big, None) == -1 and "nothing to write" in lib.last_error()
    assert h.m324_render_shade(4096, 1, 3, 1, 16, None, None, 0, vp, 1.5, 0, 4096, None, None, 4096, big, None) == -1 and "ambient" in lib.last_error()
    assert h.m324_render_shade(4096, 1, 3, 1, 16, None, None, 0, vp, 0.3, 1 << 24, 4096, None, None, 4096, big, None) == -1 and "background" in lib.last_error()
    assert h.m324_render_shade(4096, 1, 3, 1, 16, None, None, 0, None, 0.3, 0, 4096, None, None, 4096, big, None) == -1 and "null" in lib.last_error()


# ------------------------------------------------------------------------------------------------ Python layers
def test_ops_refuse_cpu_tensors_and_bad_sizes():
    v = torch.zeros(2, 3, 3)
    f = torch.zeros(1, 3, dtype=torch.int32)
    s = torch.zeros(1 << 16, dtype=torch.uint8)
    m = rc.identity_view()
    with pytest.raises(M324Error, match="HIP device"):
        ops.render_project(v, m, 16, 1)
    with pytest.raises(M324Error, match="HIP device"):
        ops.render_raster(f, 3, 2, 16, s)
    with pytest.raises(M324Error, match="HIP device"):
        ops.render_shade(f, 3, 2, 16, s, m)
    with pytest.raises(M324Error, match="size must be in 1..1024"):
        ops.render_plan(3, 1, 1, 1025)
    assert ops.render_plan(3, 1, 1, 16) > 16 * 16 * 8


def test_render_clip_refuses_cpu_input_without_a_device_and_bad_arguments():
    vertices, faces = rc.fullscreen()
    with pytest.raises(M324Error, match="no device was given"):
        render.render_clip(vertices[None], faces, size=16)
    with pytest.raises(M324Error, match="no device was given"):
        render.render_clip(torch.from_numpy(vertices)[None], torch.from_numpy(faces), size=16)
    with pytest.raises(M324Error, match="shading"):
        render.render_clip(vertices[None], faces, shading="phong")
    for size in (0, 1025):
        with pytest.raises(M324Error, match="size must be in 1..1024"):
            render.render_clip(vertices[None], faces, size=size, device="cuda")


def test_command_line_refuses_a_glb_path(tmp_path):
    glb = tmp_path / "prediction.glb"
    glb.write_bytes(b"glTF")
    with pytest.raises(M324Error, match=r"faces\.npy.*GLB"):
        render.main(["--pred_path", str(glb), "--out", str(tmp_path / "out")])
    assert not (tmp_path / "out").exists()
