"""Tracked surface samples without a GPU: the numpy host path of motion324_amd.dataset (the definition the device is held to)
against the reference's own track_with_normal_rgb (tests/golden/track.npz, see make_track_golden.py for what it pins), against
the loop model of tests/track_cases.py, and against the sampler it builds on."""
import numpy as np
import pytest
import torch

import surface_cases as sc
import track_cases as tc
from conftest import load_golden

MESHES = {"blob": lambda: sc.blob()[:2], "soup": lambda: sc.soup()[:2], "fan": tc.fan}


@pytest.fixture(scope="module")
def golden():
    return load_golden("track")


@pytest.fixture(scope="module")
def host_of_golden(golden):
    from motion324_amd import dataset
    return dataset.track_with_normal_rgb(golden["in_frames"], golden["in_faces"], int(golden["num"]), golden["in_face_uvs"], golden["in_texture"],
                                         seed=int(golden["seed"]))


# ------------------------------------------------------------------------------------------------ 1. the reference's own code
def test_host_path_draws_the_golden_faces_and_colours(golden, host_of_golden):
    """Face indices are equal.  Colours are equal except where the texel coordinate lies within 1e-9 of an integer (the
    reference recomputes the weights from the point, which may land in the neighbouring texel there): at most 0.1 % of the draw."""
    _, _, rgbs, fi = host_of_golden
    num = int(golden["num"])
    assert fi.dtype == np.int64 and np.array_equal(fi, golden["out_face_indices"])
    r0, r1 = tc.model_weights(num, int(golden["seed"]))
    x, y, _, _ = tc.model_texels(golden["in_face_uvs"], fi, r0, r1, *golden["in_texture"].shape[:2])
    exempt = sc.near_texel_border(x, y)
    print(f"texel-border exemptions: {int(exempt.sum())} of {num}")
    assert exempt.sum() <= 0.001 * num
    assert tuple(rgbs.shape) == tuple(golden["out_rgbs_shape"]) and rgbs.dtype == torch.float32
    assert np.array_equal(rgbs[0].numpy()[~exempt], golden["out_rgbs"][~exempt])
    assert bool((rgbs == rgbs[:1]).all())


def test_host_path_points_are_within_one_fp32_ulp_of_the_golden(golden, host_of_golden):
    """The reference turns the drawn point into weights (Cramer) and back into a point: fp64 noise of ~1e-16 that may flip the
    one rounding to fp32, never more."""
    points = host_of_golden[0]
    want = golden["out_points"]
    assert points.dtype == torch.float32 and tuple(points.shape) == want.shape
    diff = np.abs(points.numpy().astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    print(f"points: {int((diff > 0).sum())} of {diff.size} coordinates differ, worst {float((diff / ulp).max()):.2f} ulp")
    assert np.all(diff <= ulp)


def test_host_path_normals_are_within_2_to_the_minus_23_of_the_golden(golden, host_of_golden):
    normals = host_of_golden[1]
    want = golden["out_normals"]
    assert normals.dtype == torch.float32 and tuple(normals.shape) == want.shape
    err = np.abs(normals.numpy().astype(np.float64) - want.astype(np.float64)).max()
    print(f"normals: worst component error {err:.3e} (limit {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23
    assert np.abs(np.linalg.norm(want.astype(np.float64), axis=-1) - 1.0).max() < 1e-6


# ------------------------------------------------------------------------------------------------ 2. the pieces
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_corner_table_equals_a_brute_force_loop(mesh):
    from motion324_amd import dataset
    v, f = MESHES[mesh]()
    offsets, corners = dataset.vertex_corners(f, len(v))
    want_offsets, want_corners = tc.model_corners(f, len(v))
    assert np.array_equal(offsets, want_offsets) and np.array_equal(corners, want_corners)
    assert offsets[0] == 0 and offsets[-1] == 3 * len(f) and np.array_equal(np.sort(corners), np.arange(3 * len(f)))


def test_the_fan_has_what_the_tests_need_of_it():
    v, f = tc.fan()
    offsets, _ = tc.model_corners(f, len(v))
    valence = np.diff(offsets)
    assert valence[0] >= 300 and valence[-1] == 0 and (sc.model_areas(v, f) == 0).sum() >= 10
    assert len({tuple(np.nonzero(face == 0)[0]) for face in f}) == 3            # the hub sits at every corner position


@pytest.mark.parametrize("weighting", ["angle", "area"])
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_host_vertex_normals_equal_the_loop_model_bit_for_bit(mesh, weighting):
    """The vectorised host path adds a vertex's corners in rounds, the model one vertex at a time: the same chain of additions."""
    from motion324_amd import dataset
    v, f = MESHES[mesh]()
    clip = tc.clip_of(v, 2, 11)
    got = dataset.vertex_normals(clip, f, weighting=weighting)
    for t in range(2):
        want, cond = tc.model_vertex_normals(clip[t], f, weighting, return_condition=True)
        assert np.array_equal(got[t], want), t
        length = np.linalg.norm(want, axis=1)
        faceless = np.diff(tc.model_corners(f, len(v))[0]) == 0
        assert np.all(want[faceless] == 0.0) and np.all(np.abs(length[length > 0] - 1.0) < 1e-15)
        if weighting == "angle" and t == 0:                                     # what tests/ERROR_BOUNDS_TRACK.md builds on
            print(f"{mesh}: conditioning of the angle-weighted sum <= {np.nanmax(cond):.1f}; {int(faceless.sum())} faceless vertices")
            assert np.nanmax(cond) <= 34.0
    # the soup: 9 vertices that no face names and 4 more whose faces all lack area; no vertex with area around it sums to zero
    assert mesh != "soup" or (int(faceless.sum()), int((length == 0).sum())) == (9, 13)


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_frame_zero_of_the_host_track_is_the_host_sampler(mesh):
    from motion324_amd import dataset, preprocess
    v, f = MESHES[mesh]()
    clip = tc.clip_of(v, 3, 4)
    uv, tex = tc.corner_uvs(len(f), 4), tc.texture(4)
    points, normals, rgbs, fi = dataset.track_with_normal_rgb(clip, f, 500, uv, tex, seed=9)
    pts, want_fi = preprocess.sample_surface(clip[0], f, 500, 9)
    assert np.array_equal(fi, want_fi) and np.array_equal(points[0].numpy(), pts.astype(np.float32))
    r0, r1 = tc.model_weights(500, 9)
    _, _, col, row = tc.model_texels(uv, fi, r0, r1, *tex.shape[:2])
    assert np.array_equal(rgbs[0].numpy(), (tex[row, col] / 255.0).astype(np.float32))
    want_n = tc.model_track_normals(dataset.vertex_normals(clip, f), f, fi, r0, r1)
    assert np.array_equal(normals.numpy(), want_n.astype(np.float32))


def test_rgbs_are_an_expanded_view_over_the_frames():
    from motion324_amd import dataset
    v, f = tc.fan()
    points, normals, rgbs, fi = dataset.track_with_normal_rgb(tc.clip_of(v, 6, 1), f, 40, tc.corner_uvs(len(f), 1), tc.texture(1), seed=2)
    assert tuple(points.shape) == tuple(normals.shape) == tuple(rgbs.shape) == (6, 40, 3) and fi.shape == (40,)
    assert rgbs.stride(0) == 0 and rgbs.dtype == torch.float32 and float(rgbs.min()) >= 0.0 and float(rgbs.max()) <= 1.0


def test_a_nan_uv_lands_on_texel_zero_and_a_far_uv_on_the_border():
    from motion324_amd import dataset
    v, f = tc.fan()
    uv = np.full((len(f), 3, 2), np.nan)
    tex = tc.texture(3)
    rgbs = dataset.track_with_normal_rgb(v[None], f, 16, uv, tex, seed=0)[2]
    assert np.array_equal(rgbs[0].numpy(), np.tile((tex[0, 0] / 255.0).astype(np.float32), (16, 1)))
    rgbs = dataset.track_with_normal_rgb(v[None], f, 16, np.full((len(f), 3, 2), 1e300), tex, seed=0)[2]     # u large, 1 - v very negative
    assert np.array_equal(rgbs[0].numpy(), np.tile((tex[0, -1] / 255.0).astype(np.float32), (16, 1)))


# ------------------------------------------------------------------------------------------------ 3. validation
def test_bad_arguments_are_refused_with_their_shapes():
    from motion324_amd import dataset, ops
    from motion324_amd.lib import M324Error
    v, f = tc.fan()
    clip, uv, tex = tc.clip_of(v, 2, 0), tc.corner_uvs(len(f), 0), tc.texture(0)
    track = dataset.track_with_normal_rgb
    with pytest.raises(M324Error, match=r"vertex_frames \[T,V,3\], got \(322, 3\)"):
        track(v, f, 10, uv, tex)
    with pytest.raises(M324Error, match="faces index vertices"):
        track(clip, f + 5, 10, uv, tex)
    with pytest.raises(M324Error, match="integer faces"):
        track(clip, f.astype(np.float64), 10, uv, tex)
    with pytest.raises(M324Error, match="num_samples must be positive"):
        track(clip, f, 0, uv, tex)
    with pytest.raises(M324Error, match=r"face_uvs \[320,3,2\]"):
        track(clip, f, 10, uv[:-1], tex)
    with pytest.raises(M324Error, match="uint8 texture"):
        track(clip, f, 10, uv, tex.astype(np.float32))
    with pytest.raises(M324Error, match="weighting"):
        track(clip, f, 10, uv, tex, weighting="uniform")
    with pytest.raises(M324Error, match="weighting"):
        dataset.vertex_normals(clip, f, weighting="uniform")
    with pytest.raises(M324Error, match="HIP device"):
        ops.vertex_normals(torch.from_numpy(clip), torch.from_numpy(f.astype(np.int32)))
    with pytest.raises(M324Error, match="HIP device"):
        ops.surface_track(torch.from_numpy(clip), torch.from_numpy(f.astype(np.int32)), torch.zeros(len(f), dtype=torch.float64),
                          torch.zeros(2, dtype=torch.int64), 10)
    with pytest.raises(M324Error, match="HIP device"):
        ops.vertex_corners(torch.from_numpy(f.astype(np.int32)), len(v))
    with pytest.raises(M324Error, match="no samples"):
        dataset.collate([])


def test_entry_points_refuse_bad_calls_before_any_launch():
    """Argument validation happens before any HIP call, so it is observable without a GPU."""
    from motion324_amd import lib
    h = lib.load()
    assert h.m324_vertex_normals(None, 0, 4, 16, 2, 16, 16, 1, 0, 16, None) == -1 and "null" in lib.last_error()
    assert h.m324_vertex_normals(16, 12, 4, 16, 2, 16, 16, 1, 2, 16, None) == -1 and "weighting" in lib.last_error()
    assert h.m324_vertex_normals(16, 12, 4, 16, 0, 16, 16, 1, 0, 16, None) == -1 and "n_faces=0" in lib.last_error()
    ok = dict(vertices=16, stride_b=0, stride_t=12, n_vertices=4, faces=16, n_faces=2, cdf=16, seeds=16, num=8, batch=1, frames=1, points=16,
              points64=None, face_index=None, vertex_normals=None, nsb=0, nst=0, normals=None, face_uvs=None, texels=None, tex_h=0, tex_w=0,
              colors=None, stream=None)
    call = lambda **kw: h.m324_surface_track(*{**ok, **kw}.values())
    assert call(points=None) == -1 and "null" in lib.last_error()
    assert call(frames=0) == -1 and "frames=0" in lib.last_error()
    assert call(stride_b=-1) == -1 and "stride_b=-1" in lib.last_error()
    assert call(normals=16) == -1 and "go together" in lib.last_error()
    assert call(colors=16, face_uvs=16) == -1 and "go together" in lib.last_error()
    assert call(colors=16, face_uvs=16, texels=16, tex_h=4) == -1 and "go together" in lib.last_error()
    assert call(face_uvs=16) == -1 and "go together" in lib.last_error()
