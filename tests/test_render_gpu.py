"""Mesh clip renderer on the GPU against the numpy model of tests/render_cases.py: no tolerances, every comparison is
torch.equal of frames, face and depth."""
import numpy as np
import pytest
import torch

import render_cases as rc
from motion324_amd import ops, render

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = (0, None, 2 ** 31 - 1)           # everything queued, the default, everything in the loading lane


def assert_equal(clip, model, what=""):
    for got, name in ((clip.frames, "frames"), (clip.face, "face"), (clip.depth, "depth")):
        want = torch.from_numpy(model[name])
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, got.shape)
        assert torch.equal(got.cpu(), want), (what, name, int((got.cpu() != want).sum()))


def assert_same(a, b, what=""):
    assert torch.equal(a.frames, b.frames) and torch.equal(a.face, b.face) and torch.equal(a.depth, b.depth), what


def run(vertices, faces, S, **kw):
    vertices = np.asarray(vertices, dtype=np.float32)
    if vertices.ndim == 2:
        vertices = vertices[None]
    return render.render_clip(vertices, faces, size=S, device=DEV, **kw)


def test_quad_centres():
    for name, vertices, faces in rc.quad_variants():
        clip = run(vertices, faces, 16)
        assert_equal(clip, rc.model_render(vertices, faces, rc.identity_view(), 16), name)
        assert int((clip.face >= 0).sum()) == 100 and int(clip.depth.max()) == 4194304


@pytest.mark.parametrize("S", [16, 33])
def test_grid_snapped(S):
    for k in range(20):
        vertices, faces = rc.grid_snapped(S, k)
        assert_equal(run(vertices, faces, S), rc.model_render(vertices, faces, rc.identity_view(), S), (S, k))


@pytest.mark.parametrize("S", [16, 33])
def test_ownership_rules(S):
    cases = {"coincident": rc.coincident(S, 3, 7), "interpenetrating": rc.interpenetrating(S), "degenerate": rc.degenerate(S),
             "nan": rc.with_bad_vertex(S, np.nan), "inf": rc.with_bad_vertex(S, np.inf)}
    vertices, faces = cases["coincident"]
    swapped = faces.copy()
    swapped[[3, 7]] = swapped[[7, 3]]
    cases["coincident_swapped"] = (vertices, swapped)
    for name, (vertices, faces) in cases.items():
        clip = run(vertices, faces, S, background=(7, 130, 255), ambient=0.45)
        assert_equal(clip, rc.model_render(vertices, faces, rc.identity_view(), S, background=(7, 130, 255), ambient=0.45), (name, S))
    assert not bool((clip.face == 7).any()) and bool((clip.face == 3).any())


def test_fullscreen_is_clipped_and_independent_of_big_pixels():
    vertices, faces = rc.fullscreen()
    model = rc.model_render(vertices, faces, rc.orbit_view(10.0, -5.0), 33)
    assert (model["face"] == 0).all()
    for big in BIG:
        assert_equal(run(vertices, faces, 33, azimuth=10.0, elevation=-5.0, big_pixels=big), model, big)


@pytest.fixture(scope="module")
def sphere():
    vertices, faces, colors = rc.many_small()
    v = torch.from_numpy(vertices).to(DEV)
    normals = ops.vertex_normals(v.double(), torch.from_numpy(faces).to(DEV)).float().cpu().numpy()
    return vertices, faces, colors, normals


@pytest.mark.parametrize("shading", ["flat", "smooth"])
@pytest.mark.parametrize("colored", [False, True])
def test_many_small(sphere, shading, colored):
    vertices, faces, colors, normals = sphere
    assert faces.shape == (1280, 3) and vertices.shape == (3, 642, 3)
    kw = dict(colors=colors if colored else None)
    model = rc.model_render(vertices, faces, rc.orbit_view(35.0, 20.0), 64, normals=normals if shading == "smooth" else None,
                            cache_key="many_small", **kw)
    assert (model["face"] >= 0).sum() > 3 * 1500 and len(np.unique(model["face"])) > 400
    first = None
    for big in BIG:
        clip = run(vertices, faces, 64, azimuth=35.0, elevation=20.0, shading=shading, big_pixels=big, **kw)
        assert_equal(clip, model, (shading, colored, big))
        first = first or clip
        assert_same(clip, first, big)


def test_pile_is_deterministic_under_contention():
    vertices, faces = rc.pile()
    model = rc.model_render(vertices, faces, rc.identity_view(), 32)
    assert model["hits"].max() >= 150
    a, b = run(vertices, faces, 32), run(vertices, faces, 32, big_pixels=0)
    assert_equal(a, model, "pile")
    assert_same(a, b, "pile twice")
    assert_same(a, run(vertices, faces, 32), "pile again")


def test_input_layouts_and_chunking(sphere):
    vertices, faces, colors, _ = sphere
    f = torch.from_numpy(faces).to(DEV)
    v = torch.from_numpy(vertices).to(DEV)
    kw = dict(size=48, azimuth=-20.0, elevation=15.0, colors=torch.from_numpy(colors).to(DEV))
    plain = render.render_clip(v, f, **kw)
    assert_equal(plain, rc.model_render(vertices, faces, rc.orbit_view(-20.0, 15.0), 48, colors=colors), "device input")
    assert_same(plain, render.render_clip(v[None], f, **{**kw, "colors": kw["colors"][None]}), "pcd_moved shape")
    larger = torch.full((5, 642, 3), float("nan"), device=DEV)
    larger[1:4] = v
    view = larger[1:4]
    assert view.data_ptr() != larger.data_ptr() and view.data_ptr() == larger[1].data_ptr()
    assert_same(plain, render.render_clip(view, f, **kw), "view of a larger tensor")
    strided = torch.zeros((3, 2, 642, 3), device=DEV)
    strided[:, 1] = v
    assert strided[:, 1].stride(0) == 2 * 642 * 3
    assert_same(plain, render.render_clip(strided[:, 1], f, **kw), "frame stride")
    one = ops.render_plan(642, 1280, 1, 48)
    assert ops.render_plan(642, 1280, 2, 48) > one + 1000
    assert_same(plain, render.render_clip(v, f, max_scratch_bytes=one + 1000, **kw), "one frame per pass")
    for shading in ("flat", "smooth"):
        whole = render.render_clip(v, f, shading=shading, **kw)
        assert_same(whole, render.render_clip(v, f, shading=shading, max_scratch_bytes=one + 1000, **kw), shading)
    assert torch.equal(plain.mask(), (plain.face >= 0).to(torch.uint8) * 255) and plain.mask().dtype == torch.uint8
    assert set(plain.mask().unique().tolist()) == {0, 255}


def test_refusals_come_before_any_launch():
    from motion324_amd.lib import M324Error
    vertices, faces = rc.fullscreen()
    v = torch.from_numpy(vertices)[None].to(DEV)
    for bad in ([[0, 1, 3]], [[0, -1, 2]]):
        with pytest.raises(M324Error, match="faces index vertices"):
            render.render_clip(v, torch.tensor(bad, dtype=torch.int32, device=DEV), size=16)
    with pytest.raises(M324Error, match="big_pixels"):
        render.render_clip(v, faces, size=16, device=DEV, big_pixels=-1)
    with pytest.raises(M324Error, match="max_scratch_bytes"):
        render.render_clip(v, faces, size=16, device=DEV, max_scratch_bytes=100)
    with pytest.raises(M324Error, match=r"colors \[3,3\]"):
        render.render_clip(v, faces, size=16, device=DEV, colors=np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(M324Error, match="ambient"):
        render.render_clip(v, faces, size=16, device=DEV, ambient=1.5)


@pytest.mark.parametrize("z,x", [(0.0, 0.0), (0.3, 0.0), (0.0, 3.0)])
def test_single_pixel(z, x):
    vertices = np.array([[x - 1.0, -1.0, z], [x + 1.0, -1.0, z], [x, 1.5, z]], dtype=np.float32)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    model = rc.model_render(vertices, faces, rc.identity_view(), 1)
    assert int(model["face"][0, 0, 0]) == (0 if x == 0.0 else -1)
    clip = run(vertices, faces, 1)
    assert_equal(clip, model, (z, x))
    assert clip.mask().shape == (1, 1, 1) and int(clip.mask()[0, 0, 0]) == (255 if x == 0.0 else 0)
