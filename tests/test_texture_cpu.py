"""Textured, supersampled mesh clips without a GPU: m324_texture_plan and the refusals of the new entry points (all before the
first HIP call), the refusals of render_clip and of the command line, and properties of the numpy model itself."""
import ctypes

import numpy as np
import pytest
import torch

import render_cases as rc
import texture_cases as tc
from motion324_amd import lib, ops, render
from motion324_amd.lib import M324Error


# ------------------------------------------------------------------------------------------------ C ABI, host side
def _plan(h, w):
    levels, need = ctypes.c_int(-7), ctypes.c_long(-7)
    return lib.load().m324_texture_plan(h, w, ctypes.addressof(levels), ctypes.addressof(need)), levels.value, need.value


@pytest.mark.parametrize("h,w,levels", [(1, 1, 1), (5, 3, 3), (3, 5, 3), (7, 16, 5), (64, 64, 7), (2048, 2048, 12), (1, 16384, 15), (16384, 16384, 15)])
def test_plan_counts_levels_and_bytes(h, w, levels):
    plan, total = tc.model_plan(h, w)
    assert len(plan) == levels and plan[-1][1:] == (1, 1) and all(off % 256 == 0 for off, _, _ in plan)
    assert _plan(h, w) == (0, levels, total)
    assert ops.texture_plan(h, w) == (levels, total) and ops.texture_levels(h, w) == plan
    assert total >= sum(4 * lh * lw for _, lh, lw in plan) and total < 2 ** 31


def test_plan_known_answers_and_bad_sizes():
    assert _plan(1, 1) == (0, 1, 256)
    assert _plan(5, 3) == (0, 3, 768)                       # 60 bytes, 8 bytes, 4 bytes: one 256-byte slot each
    assert _plan(64, 64) == (0, 7, 16384 + 4096 + 1024 + 256 * 4)
    assert lib.load().m324_texture_plan(4, 4, None, None) == 0
    for h, w in ((0, 4), (4, 0), (-1, 4), (16385, 4), (4, 16385)):
        assert _plan(h, w) == (-1, -7, -7) and "texture sides" in lib.last_error() and "m324_texture_plan" in lib.last_error()
        with pytest.raises(M324Error, match="texture sides"):
            ops.texture_plan(h, w)


def _shade_tex(h, **kw):
    """m324_render_shade_tex with plausible (never dereferenced) pointers; every call here must be refused"""
    view = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    a = dict(faces=4096, nf=1, nv=3, frames=1, size=16, colors=None, normals=None, stride=0, view=ctypes.addressof(view), ambient=0.3, background=0,
             face_uvs=None, mips=None, th=0, tw=0, use_mips=1, ss=1, rgb=4096, face=4096, depth=4096, scratch=4096, nbytes=1 << 40)
    a.update(kw)
    return h.m324_render_shade_tex(a["faces"], a["nf"], a["nv"], a["frames"], a["size"], a["colors"], a["normals"], a["stride"], a["view"], a["ambient"],
                                   a["background"], a["face_uvs"], a["mips"], a["th"], a["tw"], a["use_mips"], a["ss"], a["rgb"], a["face"], a["depth"],
                                   a["scratch"], a["nbytes"], None)


@pytest.mark.parametrize("kwargs,word", [
    (dict(size=0), "size"), (dict(size=1025), "size"), (dict(frames=0), "frames"), (dict(nf=-1), "n_faces"), (dict(faces=None), "null"),
    (dict(scratch=None), "null"), (dict(view=None), "null"), (dict(rgb=None, face=None, depth=None), "nothing to write"), (dict(ambient=1.5), "ambient"),
    (dict(background=1 << 24), "background"), (dict(stride=-1), "normal_stride_t"), (dict(ss=3), "supersample"), (dict(ss=0), "supersample"),
    (dict(ss=8), "supersample"), (dict(size=15, ss=2), "multiple of supersample"), (dict(size=18, ss=4), "multiple of supersample"),
    (dict(face_uvs=4096), "go together"), (dict(mips=4096), "go together"), (dict(th=4, tw=4), "without face_uvs"),
    (dict(face_uvs=4096, mips=4096, th=4, tw=4, colors=4096), "two albedos"), (dict(face_uvs=4096, mips=4096, th=0, tw=4), "texture sides"),
    (dict(face_uvs=4096, mips=4096, th=4, tw=16385), "texture sides"), (dict(face_uvs=4096, mips=4098, th=4, tw=4), "4-byte aligned"),
    (dict(nbytes=64), "scratch bytes"), (dict(scratch=4104), "aligned")])
def test_shade_tex_refuses_before_any_hip_call(kwargs, word):
    assert _shade_tex(lib.load(), **kwargs) == -1
    assert "m324_render_shade_tex" in lib.last_error() and word in lib.last_error(), lib.last_error()


def test_texture_mips_refuses_before_any_hip_call():
    h = lib.load()
    big = 1 << 40
    for args, word in (((None, 4, 4, 3, 4096, big), "null"), ((4096, 4, 4, 3, None, big), "null"), ((4096, 0, 4, 3, 4096, big), "texture sides"),
                       ((4096, 4, 16385, 3, 4096, big), "texture sides"), ((4096, 4, 4, 2, 4096, big), "channels"), ((4096, 4, 4, 5, 4096, big), "channels"),
                       ((4096, 4, 4, 3, 4096, 767), "mips bytes"), ((4096, 4, 4, 3, 4097, big), "4-byte aligned")):
        assert h.m324_texture_mips(*args, None) == -1, args
        assert "m324_texture_mips" in lib.last_error() and word in lib.last_error(), lib.last_error()


# ------------------------------------------------------------------------------------------------ Python layers
def test_ops_refuse_cpu_tensors():
    with pytest.raises(M324Error, match="HIP device"):
        ops.texture_mips(torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(M324Error, match="HIP device"):
        ops.render_shade_tex(torch.zeros(1, 3, dtype=torch.int32), 3, 1, 16, torch.zeros(1 << 16, dtype=torch.uint8), rc.identity_view())


def test_render_clip_refuses_as_specified():
    vertices, faces, uv = tc.anchor_quad(0, 0, 16, 16)
    tex = tc.noise_texture(4, 4)
    fuv = uv[faces]
    for kw, word in ((dict(uv=uv, face_uvs=fuv, texture=tex), "not both"), (dict(uv=uv), "without a texture"), (dict(face_uvs=fuv), "without a texture"),
                     (dict(texture=tex), "needs uv"), (dict(uv=uv, texture=tex, colors=np.zeros((4, 3), dtype=np.float32)), "two albedos"),
                     (dict(uv=uv[:3], texture=tex), r"uv \[4, 2\]"), (dict(uv=uv.T, texture=tex), r"uv \[4, 2\]"),
                     (dict(face_uvs=fuv[:1], texture=tex), r"face_uvs \[2, 3, 2\]"), (dict(face_uvs=uv, texture=tex), r"face_uvs \[2, 3, 2\]"),
                     (dict(uv=uv.astype(np.int32), texture=tex), "floating-point uv"), (dict(uv=uv, texture=tex.astype(np.float32)), "uint8 texture"),
                     (dict(uv=uv, texture=torch.zeros(4, 4, 3)), "uint8 texture"), (dict(uv=uv, texture=tex[..., :2]), "uint8 texture"),
                     (dict(uv=uv, texture=tex[0]), "uint8 texture"), (dict(uv=uv, texture=np.zeros((16385, 1, 3), dtype=np.uint8)), "texture sides"),
                     (dict(supersample=3), "supersample"), (dict(supersample=0), "supersample"), (dict(supersample=2.5), "supersample"),
                     (dict(supersample=True), "supersample")):
        with pytest.raises(M324Error, match=word):
            render.render_clip(vertices[None], faces, size=16, device="cuda", **kw)
    for size, ss in ((512, 4), (1024, 2), (513, 2), (257, 4)):
        with pytest.raises(M324Error, match=r"size \* supersample"):
            render.render_clip(vertices[None], faces, size=size, supersample=ss, device="cuda")


def test_mask_is_the_coverage_share_of_the_samples():
    face = torch.full((1, 4, 4), -1, dtype=torch.int32)
    face[0, :2, :2] = 3                                     # pixel (0, 0) fully covered
    face[0, 0, 2] = 1                                       # pixel (0, 1): one sample of four
    face[0, 2, 0] = face[0, 3, 1] = face[0, 3, 0] = 0       # pixel (1, 0): three of four
    clip = render.RenderedClip(torch.zeros((1, 2, 2, 3), dtype=torch.uint8), face, face.clone())
    assert clip.mask().dtype == torch.uint8 and clip.mask().tolist() == [[[255, 64], [191, 0]]]
    assert np.array_equal(clip.mask().numpy(), tc.model_coverage(face.numpy(), 2))
    quarter = render.RenderedClip(torch.zeros((1, 1, 1, 3), dtype=torch.uint8), face, face.clone())
    assert quarter.mask().tolist() == [[[(255 * 8 + 8) // 16]]]
    plain = render.RenderedClip(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), face, face.clone())
    assert torch.equal(plain.mask(), (face >= 0).to(torch.uint8) * 255)


def _sequence(tmp_path, uv=None):
    vertices, faces, _ = tc.anchor_quad(0, 0, 16, 16)
    np.save(tmp_path / "faces.npy", faces)
    np.save(tmp_path / "frame_0000.npy", vertices)
    np.save(tmp_path / "texture.npy", tc.noise_texture(4, 4))
    if uv is not None:
        np.save(tmp_path / "uv.npy", uv)
    return ["--pred_path", str(tmp_path), "--out", str(tmp_path / "out")]


def test_command_line_names_the_missing_uv_file_and_both_shapes(tmp_path):
    argv = _sequence(tmp_path)
    with pytest.raises(M324Error, match=r"uv\.npy not found.*\[4,2\].*\[2,3,2\]"):
        render.main(argv + ["--texture", str(tmp_path / "texture.npy")])
    assert not (tmp_path / "out").exists()


def test_command_line_refuses_a_wrong_uv_shape_and_supersample(tmp_path):
    argv = _sequence(tmp_path, uv=np.zeros((3, 2), dtype=np.float32))
    with pytest.raises(M324Error, match=r"uv\.npy: expected \[V,2\] = \[4,2\] or \[F,3,2\] = \[2,3,2\], got \[3, 2\]"):
        render.main(argv + ["--texture", str(tmp_path / "texture.npy")])
    for extra in (["--supersample", "3"], ["--supersample", "4", "--size", "512"]):
        with pytest.raises(M324Error, match="--supersample"):
            render.main(argv + extra)
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------ the model itself
@pytest.mark.parametrize("h,w", [(1, 1), (5, 3), (7, 16), (12, 20)])
def test_a_constant_texture_is_constant_at_every_level_and_uv(h, w):
    texture = np.empty((h, w, 3), dtype=np.uint8)
    texture[...] = (3, 141, 255)
    levels = tc.model_mips(texture)
    for lv in levels:
        assert (lv[..., :3] == (3, 141, 255)).all() and (lv[..., 3] == 0).all()
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.uniform(-3.0, 3.0, 200), [0.0, 1.0, -1.0, 0.5, np.nan, np.inf, -np.inf, 1e30]]).astype(np.float32)
    v = np.concatenate([rng.uniform(-3.0, 3.0, 200), [1.0, 0.0, -0.0, 0.5, 2.0, np.nan, 0.25, -1e30]]).astype(np.float32)
    want = (np.array([3, 141, 255], dtype=np.float32) / np.float32(255.0))[None]
    for l in range(len(levels)):
        assert np.array_equal(tc.model_taps(levels, np.full(len(u), l), u, v), np.broadcast_to(want, (len(u), 3)))


def test_mip_levels_average_with_rounding_and_drop_an_odd_edge():
    texture = np.zeros((2, 3, 3), dtype=np.uint8)
    texture[..., 0] = [[1, 2, 200], [2, 2, 200]]            # (1 + 2 + 2 + 2 + 2) >> 2 = 2; the third column is dropped
    texture[..., 1] = [[255, 255, 0], [255, 254, 0]]        # (1019 + 2) >> 2 = 255
    levels = tc.model_mips(texture)
    assert [lv.shape for lv in levels] == [(2, 3, 4), (1, 1, 4)] and levels[1][0, 0].tolist() == [2, 255, 0, 0]
    tall = tc.model_mips(np.arange(4, dtype=np.uint8).reshape(4, 1, 1).repeat(3, axis=2))
    assert [lv.shape for lv in tall] == [(4, 1, 4), (2, 1, 4), (1, 1, 4)]
    assert tall[1][:, 0, 0].tolist() == [(0 + 0 + 1 + 1 + 2) >> 2, (2 + 2 + 3 + 3 + 2) >> 2]      # the clamped column counts twice


def test_level_rule_at_its_thresholds():
    for l in range(13):
        t = np.float32(2.0 * 4.0 ** l)
        below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(np.inf))
        got = tc.model_level(np.array([below, t, above], dtype=np.float32), 14)
        assert got.tolist() == [l, l, l + 1], (l, got)
        assert tc.model_level(np.array([above], dtype=np.float32), l).tolist() == [l]         # never past the last level
    special = tc.model_level(np.array([np.nan, np.inf, 0.0, -1.0, 1.0], dtype=np.float32), 6)
    assert special.tolist() == [0, 6, 0, 0, 0]
    assert tc.model_level(np.array([1e9], dtype=np.float32), 0).tolist() == [0]                # use_mips = 0


def test_wrap_is_periodic_in_exact_integer_shifts():
    levels = tc.model_mips(tc.noise_texture(12, 20))
    rng = np.random.default_rng(11)
    # multiples of 2^-10 below 4 in magnitude: adding an integer up to 64 is exact in fp32
    u = (rng.integers(-4096, 4096, 300) / 1024.0).astype(np.float32)
    v = (rng.integers(-4096, 4096, 300) / 1024.0).astype(np.float32)
    for l in (0, 1, 2, 4):
        base = tc.model_taps(levels, np.full(300, l), u, v)
        for du, dv in ((1, 0), (0, 1), (-3, 7), (64, -64)):
            assert np.array_equal((u + np.float32(du)) - np.float32(du), u)
            assert np.array_equal(tc.model_taps(levels, np.full(300, l), u + np.float32(du), v + np.float32(dv)), base), (l, du, dv)
    assert len(levels) == 5 and len(np.unique(tc.model_taps(levels, np.zeros(300, dtype=np.int64), u, v))) > 50


def test_sphere_case_reaches_four_levels_on_the_model():
    vertices, faces, _ = rc.many_small()
    uv = tc.sphere_uvs(vertices[0])
    model = tc.model_render_tex(vertices, faces, rc.orbit_view(35.0, 20.0), 64, face_uvs=uv[faces], texture=tc.noise_texture(64, 64), cache_key="many_small")
    assert {0, 1, 2, 3} <= set(np.unique(model["levels"]))
    flat = tc.model_render_tex(vertices, faces, rc.orbit_view(35.0, 20.0), 64, face_uvs=uv[faces], texture=tc.noise_texture(64, 64), use_mips=False,
                               cache_key="many_small")
    assert set(np.unique(flat["levels"])) == {-1, 0} and np.array_equal(flat["face"], model["face"]) and not np.array_equal(flat["frames"], model["frames"])
    same = rc.model_render(vertices, faces, rc.orbit_view(35.0, 20.0), 64, cache_key="many_small")
    assert np.array_equal(same["face"], model["face"]) and np.array_equal(same["depth"], model["depth"])
