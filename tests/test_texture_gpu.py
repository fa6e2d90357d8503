"""Textured and supersampled mesh clips on the GPU against the numpy model of tests/texture_cases.py and against two analytic
anchors that do not use the model: no tolerances, every comparison is torch.equal."""
import numpy as np
import pytest
import torch

import render_cases as rc
import texture_cases as tc
from motion324_amd import ops, render
from motion324_amd.lib import M324Error

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = (0, None, 2 ** 31 - 1)


def assert_equal(clip, model, what=""):
    for got, name in ((clip.frames, "frames"), (clip.face, "face"), (clip.depth, "depth")):
        want = torch.from_numpy(model[name])
        assert got.dtype == want.dtype and got.shape == want.shape, (what, name, got.dtype, got.shape, want.shape)
        assert torch.equal(got.cpu(), want), (what, name, int((got.cpu() != want).sum()))


def assert_same(a, b, what=""):
    assert torch.equal(a.frames, b.frames) and torch.equal(a.face, b.face) and torch.equal(a.depth, b.depth), what


def run(vertices, faces, S, **kw):
    vertices = np.asarray(vertices, dtype=np.float32)
    if vertices.ndim == 2:
        vertices = vertices[None]
    return render.render_clip(vertices, faces, size=S, device=DEV, **kw)


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("h,w,channels", [(1, 1, 3), (5, 3, 3), (7, 16, 3), (64, 64, 3), (7, 16, 4), (5, 3, 4)])
def test_mip_chain_is_the_integer_model(h, w, channels):
    texture = tc.noise_texture(h, w, channels)
    mips, levels = ops.texture_mips(torch.from_numpy(texture).to(DEV))
    plan, total = tc.model_plan(h, w)
    assert ops.texture_plan(h, w) == (len(plan), total) and levels == plan and mips.numel() == total and mips.dtype == torch.uint8
    want = tc.model_mips(texture)
    assert want[-1].shape == (1, 1, 4) and len(want) == len(plan)
    host = mips.cpu()
    for (off, lh, lw), level in zip(plan, want):
        assert off % 256 == 0
        assert torch.equal(host[off:off + 4 * lh * lw].view(lh, lw, 4), torch.from_numpy(level)), (h, w, channels, lh, lw)
    assert torch.equal(host, torch.from_numpy(tc.chain_bytes(texture)))       # nothing is written between the levels
    if channels == 4:
        assert texture[..., 3].any()                                          # the fourth byte was random, and is ignored
        assert torch.equal(ops.texture_mips(torch.from_numpy(np.ascontiguousarray(texture[..., :3])).to(DEV))[0], mips)


# ------------------------------------------------------------------------------------------------ analytic anchors
def test_texel_per_pixel_quad_shows_the_texture_itself():
    texture = tc.noise_texture(16, 16)
    vertices, faces, uv = tc.anchor_quad(0, 0, 16, 16)
    for mipmaps in (True, False):
        clip = run(vertices, faces, 16, uv=uv, texture=texture, ambient=1.0, mipmaps=mipmaps)
        assert bool((clip.face >= 0).all())
        assert torch.equal(clip.frames[0].cpu(), torch.from_numpy(texture)), mipmaps


def test_minified_quad_shows_level_four():
    texture = tc.noise_texture(64, 64)
    vertices, faces, uv = tc.anchor_quad(6, 6, 10, 10)                        # 4 x 4 pixels for 64 x 64 texels: rho = 256
    mips, levels = ops.texture_mips(torch.from_numpy(texture).to(DEV))
    off, lh, lw = levels[4]
    assert (lh, lw) == (4, 4)
    level4 = mips[off:off + 64].view(4, 4, 4)[..., :3]
    clip = run(vertices, faces, 16, uv=uv, texture=texture, ambient=1.0, background=(9, 9, 9))
    assert int((clip.face >= 0).sum()) == 16
    assert torch.equal(clip.frames[0, 6:10, 6:10], level4)
    twin = run(vertices, faces, 16, uv=uv, texture=texture, ambient=1.0, background=(9, 9, 9), mipmaps=False)
    assert torch.equal(twin.face, clip.face) and not torch.equal(twin.frames, clip.frames)
    outside = torch.ones(16, 16, dtype=torch.bool)
    outside[6:10, 6:10] = False
    assert bool((clip.frames[0][outside] == 9).all())


# ------------------------------------------------------------------------------------------------ model parity
@pytest.mark.parametrize("S", [16, 33])
@pytest.mark.parametrize("shading", ["flat", "smooth"])
def test_grid_textured(S, shading):
    vertices, faces, uvs = tc.grid_textured(S)
    finite = uvs[:20][np.isfinite(uvs[:20])]
    assert np.isnan(uvs).any() and np.isinf(uvs).any() and (uvs[5] == uvs[5, 0]).all() and finite.min() < -1.0 and finite.max() > 2.0
    normals = None
    if shading == "smooth":
        v = torch.from_numpy(vertices)[None].to(DEV)
        normals = ops.vertex_normals(v.double(), torch.from_numpy(faces).to(DEV)).float().cpu().numpy()
    for th, tw in ((5, 3), (12, 20)):
        texture = tc.noise_texture(th, tw)
        for mipmaps in (True, False):
            model = tc.model_render_tex(vertices, faces, rc.identity_view(), S, face_uvs=uvs, texture=texture, use_mips=mipmaps, normals=normals,
                                        ambient=0.45, background=(7, 130, 255))
            levels = set(np.unique(model["levels"])) - {-1}
            assert len(levels) >= 3 if mipmaps else levels == {0}
            assert (model["levels"][model["face"] == 5] == 0).all()
            clip = run(vertices, faces, S, face_uvs=uvs, texture=texture, mipmaps=mipmaps, shading=shading, ambient=0.45, background=(7, 130, 255))
            assert_equal(clip, model, (S, shading, th, tw, mipmaps))


@pytest.mark.parametrize("S", [16, 33])
def test_ownership_cases_textured(S):
    texture = tc.noise_texture(12, 20)
    cases = {"coincident": rc.coincident(S, 3, 7), "interpenetrating": rc.interpenetrating(S)}
    for name, (vertices, faces) in cases.items():
        uvs = tc.random_corner_uvs(len(faces), 17)
        model = tc.model_render_tex(vertices, faces, rc.identity_view(), S, face_uvs=uvs, texture=texture)
        assert_equal(run(vertices, faces, S, face_uvs=uvs, texture=texture), model, (name, S))
    assert not (model["face"] == -1).all()


@pytest.fixture(scope="module")
def sphere():
    vertices, faces, colors = rc.many_small()
    v = torch.from_numpy(vertices).to(DEV)
    normals = ops.vertex_normals(v.double(), torch.from_numpy(faces).to(DEV)).float().cpu().numpy()
    return vertices, faces, colors, normals, tc.sphere_uvs(vertices[0])


@pytest.mark.parametrize("shading", ["flat", "smooth"])
def test_many_small_textured(sphere, shading):
    vertices, faces, _colors, normals, uv = sphere
    texture = tc.noise_texture(64, 64)
    model = tc.model_render_tex(vertices, faces, rc.orbit_view(35.0, 20.0), 64, face_uvs=uv[faces], texture=texture,
                                normals=normals if shading == "smooth" else None, cache_key="many_small")
    assert {0, 1, 2, 3} <= set(np.unique(model["levels"]))
    first = None
    for big in BIG:
        clip = run(vertices, faces, 64, azimuth=35.0, elevation=20.0, shading=shading, big_pixels=big, uv=uv, texture=texture)
        assert_equal(clip, model, (shading, big))
        first = first or clip
        assert_same(clip, first, big)


# ------------------------------------------------------------------------------------------------ equivalences
def test_equivalent_inputs_and_chunking(sphere):
    vertices, faces, colors, _normals, uv = sphere
    texture = tc.noise_texture(12, 20, 4)
    v, f = torch.from_numpy(vertices).to(DEV), torch.from_numpy(faces).to(DEV)
    kw = dict(size=48, azimuth=-20.0, elevation=15.0)
    plain = render.render_clip(v, f, uv=torch.from_numpy(uv).to(DEV), texture=torch.from_numpy(texture).to(DEV), **kw)
    assert_same(plain, render.render_clip(v, f, face_uvs=uv[faces], texture=texture, **kw), "uv= against face_uvs=uv[faces]")
    assert_same(plain, render.render_clip(v, f, uv=uv, texture=np.ascontiguousarray(texture[..., :3]), **kw), "RGBA against RGB")
    for big in BIG:
        assert_same(plain, render.render_clip(v, f, uv=uv, texture=texture, big_pixels=big, **kw), big)
    one = ops.render_plan(642, 1280, 1, 48)
    assert_same(plain, render.render_clip(v, f, uv=uv, texture=texture, max_scratch_bytes=one + 1000, **kw), "one frame per pass")
    two = ops.render_plan(642, 1280, 1, 96)
    whole = render.render_clip(v, f, uv=uv, texture=texture, supersample=2, shading="smooth", **kw)
    assert_same(whole, render.render_clip(v, f, uv=uv, texture=texture, supersample=2, shading="smooth", max_scratch_bytes=two + 1000, **kw), "ss = 2, chunked")
    # without the new keywords nothing changed, and spelling out the defaults is the same call
    col = torch.from_numpy(colors).to(DEV)
    old = render.render_clip(v, f, colors=col, **kw)
    assert_equal(old, rc.model_render(vertices, faces, rc.orbit_view(-20.0, 15.0), 48, colors=colors), "no new keywords")
    assert_same(old, render.render_clip(v, f, colors=col, supersample=1, mipmaps=True, uv=None, face_uvs=None, texture=None, **kw), "explicit defaults")


@pytest.mark.parametrize("shading", ["flat", "smooth"])
@pytest.mark.parametrize("colored", [False, True])
def test_shade_tex_without_uvs_is_render_shade(sphere, shading, colored):
    vertices, faces, colors, normals, _uv = sphere
    v, f = torch.from_numpy(vertices).to(DEV), torch.from_numpy(faces).to(DEV)
    m = rc.orbit_view(35.0, 20.0)
    scratch = ops.render_project(v, m, 40, 1280)
    ops.render_raster(f, 642, 3, 40, scratch)
    kw = dict(colors=torch.from_numpy(colors).to(DEV) if colored else None, normals=torch.from_numpy(normals).to(DEV) if shading == "smooth" else None,
              ambient=0.25, background=(1, 2, 250))
    old = ops.render_shade(f, 642, 3, 40, scratch, m, **kw)
    new = ops.render_shade_tex(f, 642, 3, 40, scratch, m, supersample=1, **kw)
    assert all(torch.equal(a, b) for a, b in zip(old, new)) and bool((old[1] >= 0).any()) and bool((old[1] < 0).any())


# ------------------------------------------------------------------------------------------------ supersampling
@pytest.mark.parametrize("ss", [2, 4])
@pytest.mark.parametrize("albedo", ["texture", "colors", "grey"])
def test_supersampling_is_the_box_average_of_the_larger_render(sphere, ss, albedo):
    vertices, faces, colors, _normals, uv = sphere
    kw = dict(azimuth=35.0, elevation=20.0, background=(40, 200, 90), shading="smooth" if albedo == "colors" else "flat")
    if albedo == "texture":
        kw.update(uv=uv, texture=tc.noise_texture(12, 20))
    elif albedo == "colors":
        kw.update(colors=colors)
    fine = run(vertices, faces, 16 * ss, **kw)
    clip = run(vertices, faces, 16, supersample=ss, **kw)
    assert clip.frames.shape == (3, 16, 16, 3) and clip.face.shape == (3, 16 * ss, 16 * ss) and clip.depth.shape == clip.face.shape
    box = fine.frames.to(torch.int32).view(3, 16, ss, 16, ss, 3).sum(dim=(2, 4))
    assert torch.equal(clip.frames, ((box + ss * ss // 2) >> (2 if ss == 2 else 4)).to(torch.uint8))
    assert torch.equal(clip.face, fine.face) and torch.equal(clip.depth, fine.depth)
    covered = (fine.face >= 0).view(3, 16, ss, 16, ss).sum(dim=(2, 4))
    mask = clip.mask()
    assert mask.dtype == torch.uint8 and torch.equal(mask, ((255 * covered + ss * ss // 2) // (ss * ss)).to(torch.uint8))
    assert len(mask.unique()) > 2 and torch.equal(mask.cpu(), torch.from_numpy(tc.model_coverage(fine.face.cpu().numpy(), ss)))
    if albedo == "texture":                                                   # and the whole thing against the model
        model = tc.model_render_tex(vertices, faces, rc.orbit_view(35.0, 20.0), 16, ss, face_uvs=uv[faces], texture=kw["texture"], background=(40, 200, 90))
        assert_equal(clip, model, ss)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch():
    vertices, faces, uv = tc.anchor_quad(0, 0, 16, 16)
    v = torch.from_numpy(vertices)[None].to(DEV)
    tex = tc.noise_texture(4, 4)
    fuv = uv[faces]
    for kw, word in ((dict(uv=uv, face_uvs=fuv, texture=tex), "not both"), (dict(uv=uv), "without a texture"), (dict(face_uvs=fuv), "without a texture"),
                     (dict(texture=tex), "needs uv"), (dict(uv=uv, texture=tex, colors=np.zeros((4, 3), dtype=np.float32)), "two albedos"),
                     (dict(uv=uv[:3], texture=tex), r"uv \[4, 2\]"), (dict(face_uvs=fuv[:1], texture=tex), r"face_uvs \[2, 3, 2\]"),
                     (dict(uv=uv.astype(np.int32), texture=tex), "floating-point uv"), (dict(uv=uv, texture=tex.astype(np.float32)), "uint8 texture"),
                     (dict(uv=uv, texture=tex[..., :2]), "uint8 texture"), (dict(uv=uv, texture=tex[0]), "uint8 texture"),
                     (dict(uv=uv, texture=np.zeros((1, 16385, 3), dtype=np.uint8)), "texture sides"), (dict(supersample=3), "supersample"),
                     (dict(supersample=0), "supersample"), (dict(supersample=8), "supersample")):
        with pytest.raises(M324Error, match=word):
            render.render_clip(v, faces, size=16, device=DEV, **kw)
    with pytest.raises(M324Error, match=r"size \* supersample"):
        render.render_clip(v, faces, size=512, supersample=4, device=DEV)
    with pytest.raises(M324Error, match=r"size \* supersample"):
        render.render_clip(v, faces, size=1024, supersample=2, device=DEV)
    scratch = ops.render_project(v, rc.identity_view(), 16, 2)
    f = torch.from_numpy(faces).to(DEV)
    ops.render_raster(f, 4, 1, 16, scratch)
    mips, _ = ops.texture_mips(torch.from_numpy(tex).to(DEV))
    with pytest.raises(M324Error, match="go together"):
        ops.render_shade_tex(f, 4, 1, 16, scratch, rc.identity_view(), face_uvs=torch.from_numpy(fuv).to(DEV))
    with pytest.raises(M324Error, match="chain of a 64 x 64"):
        ops.render_shade_tex(f, 4, 1, 16, scratch, rc.identity_view(), face_uvs=torch.from_numpy(fuv).to(DEV), mips=mips, tex_size=(64, 64))
    with pytest.raises(M324Error, match="supersample"):
        ops.render_shade_tex(f, 4, 1, 15, scratch, rc.identity_view(), supersample=2)
