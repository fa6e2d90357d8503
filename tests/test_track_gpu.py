"""Tracked surface samples on the GPU (m324_vertex_normals, m324_surface_track in csrc/surface.hip) against the numpy host path
of motion324_amd.dataset and the loop model of tests/track_cases.py.

Points, face indices and colours have no transcendental on their path: they equal the host path bit for bit, without an
exemption.  (The device's CDF adds the areas in another order than np.cumsum; the tests first check, on the host, that no draw
of theirs lies within rounding of a CDF entry -- a statement about the inputs.)  Normals go through fp64 acos; their limit,
2^-23 per component, is derived in tests/ERROR_BOUNDS_TRACK.md."""
import numpy as np
import pytest
import torch

import surface_cases as sc
import track_cases as tc
from conftest import CASES, synth_sd

pytestmark = pytest.mark.gpu
LIMIT = 2.0 ** -23
MESHES = {"blob": lambda: sc.blob()[:2], "soup": lambda: sc.soup()[:2], "fan": tc.fan,
          "one_face": lambda: (np.array([[0.1, 0.2, 0.3], [0.7, 0.1, 0.25], [0.3, 0.9, 0.4]]), np.array([[0, 1, 2]]))}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _host(t):
    return t.cpu().numpy()


def _seeds(seeds):
    from motion324_amd import preprocess
    table = preprocess.surface_seeds(seeds)
    return _dev(table if np.ndim(seeds) else table[0])


def _clips(mesh, B, T):
    """B different clips of one mesh [B,T,V,3], its faces, per-corner UVs and a texture"""
    v, f = MESHES[mesh]()
    clips = np.stack([tc.clip_of((1.0 + 0.3 * k) * v + 0.05 * k, T, 20 + k) for k in range(B)])
    return clips, f, tc.corner_uvs(len(f), 8), tc.texture(8)


def _host_track(clip, f, num, seed, uv, tex):
    """the host path's fp64 points, colours and face indices for one clip"""
    from motion324_amd import dataset
    assert not sc.near_cdf_entry(clip[0], f, num, seed).any(), "pick another seed: a draw lies within rounding of a CDF entry"
    points, _, colors, fi = dataset._track_host(clip, f, num, uv, tex, seed, np.zeros_like(clip))
    return points, colors, fi


def _device_track(clips, f, seeds, num, uv=None, tex=None, normals=None, shared=False):
    from motion324_amd import ops
    v, fd = _dev(clips, torch.float64), _dev(f, torch.int32)
    cdf = ops.surface_cdf(v[0] if shared else v[:, 0], fd)
    extra = {} if uv is None else dict(face_uvs=_dev(uv), texture=_dev(tex))
    return ops.surface_track(v, fd, cdf, _seeds(seeds), num, vertex_normals=normals, want_points64=True, **extra)


# ------------------------------------------------------------------------------------------------ 1. points, faces, colours
@pytest.mark.parametrize("mesh,B,T,num", [("blob", 3, 5, 1000), ("soup", 3, 5, 1000), ("fan", 3, 5, 1000), ("blob", 1, 1, 1), ("fan", 2, 1, 1000),
                                          ("soup", 1, 33, 257), ("blob", 2, 33, 1), ("one_face", 2, 2, 300), ("blob", 3, 33, 6000)])
def test_points_faces_and_colours_equal_the_host_path_bit_for_bit(mesh, B, T, num):
    """The last case has 3 x 33 x 24 (item, frame, sample tile) work items, more than four per compute unit of a 256-CU chip: the
    entry point then gives a lane two frames to walk (17 frame groups, the last one with a single frame); the others walk one."""
    from motion324_amd import ops
    clips, f, uv, tex = _clips(mesh, B, T)
    seeds = [3 + 5 * k for k in range(B)]
    s = _device_track(clips, f, seeds, num, uv, tex)
    assert tuple(s.points.shape) == (B, T, num, 3) and tuple(s.colors.shape) == (B, num, 3) and tuple(s.face_index.shape) == (B, num)
    assert s.points.dtype == torch.float32 and s.colors.dtype == torch.float32 and s.face_index.dtype == torch.int32 and s.normals is None
    for k in range(B):
        points, colors, fi = _host_track(clips[k], f, num, seeds[k], uv, tex)
        assert np.array_equal(_host(s.face_index[k]), fi), k
        assert np.array_equal(_host(s.points64[k]), points), k
        assert np.array_equal(_host(s.points[k]), points.astype(np.float32)), k
        assert np.array_equal(_host(s.colors[k]), colors), k
    # frame 0 is the sampler's draw on frame 0
    v0, fd = _dev(clips[:, 0], torch.float64), _dev(f, torch.int32)
    draw = ops.surface_sample(v0, fd, ops.surface_cdf(v0, fd), _seeds(seeds), num, want_points64=True)
    assert torch.equal(s.points64[:, 0], draw.points64) and torch.equal(s.points[:, 0], draw.points) and torch.equal(s.face_index, draw.face_index)


@pytest.mark.parametrize("mesh,T,num", [("blob", 5, 1000), ("soup", 1, 300)])
def test_one_clip_for_every_item_is_a_batch_stride_of_zero(mesh, T, num):
    clips, f, uv, tex = _clips(mesh, 1, T)
    seeds = [2, 40, 7]
    s = _device_track(clips[0], f, seeds, num, uv, tex, shared=True)           # vertices [T,V,3], three seed pairs
    assert tuple(s.points.shape) == (3, T, num, 3)
    for k in range(3):
        points, colors, fi = _host_track(clips[0], f, num, seeds[k], uv, tex)
        assert np.array_equal(_host(s.points64[k]), points) and np.array_equal(_host(s.face_index[k]), fi) and np.array_equal(_host(s.colors[k]), colors)
    single = _device_track(clips[0], f, seeds[1], num, uv, tex, shared=True)    # one seed pair: no batch axis
    assert tuple(single.points.shape) == (T, num, 3) and torch.equal(single.points, s.points[1]) and torch.equal(single.colors, s.colors[1])


def test_the_device_path_of_the_public_function_equals_its_host_path():
    from motion324_amd import dataset
    clips, f, uv, tex = _clips("fan", 1, 4)
    assert not sc.near_cdf_entry(clips[0, 0], f, 600, 12).any()
    hp, hn, hc, hf = dataset.track_with_normal_rgb(clips[0], f, 600, uv, tex, seed=12)
    dp, dn, dc, df = dataset.track_with_normal_rgb(clips[0], f, 600, uv, tex, seed=12, device="cuda")
    assert all(t.is_cuda for t in (dp, dn, dc, df)) and df.dtype == torch.int64 and tuple(dc.shape) == (4, 600, 3) and dc.stride(0) == 0
    assert np.array_equal(_host(dp), hp.numpy()) and np.array_equal(_host(dc), hc.numpy()) and np.array_equal(_host(df), hf)
    err = np.abs(_host(dn).astype(np.float64) - hn.numpy().astype(np.float64)).max()
    print(f"device normals against the host path: worst component error {err:.3e}")
    assert err <= LIMIT


# ------------------------------------------------------------------------------------------------ 2. vertex normals
@pytest.mark.parametrize("weighting", ["angle", "area"])
@pytest.mark.parametrize("mesh", ["blob", "soup", "fan", "one_face"])
def test_vertex_normals_are_within_2_to_the_minus_23_of_the_model(mesh, weighting):
    from motion324_amd import ops
    clips, f, _, _ = _clips(mesh, 2, 2)
    fd = _dev(f, torch.int32)
    got = _host(ops.vertex_normals(_dev(clips, torch.float64), fd, weighting=weighting))
    assert got.shape == clips.shape and got.dtype == np.float64
    worst = 0.0
    for b in range(2):
        for t in range(2):
            want = tc.model_vertex_normals(clips[b, t], f, weighting)
            worst = max(worst, np.abs(got[b, t] - want).max())
            zero = ~want.any(axis=1)                            # vertices without faces, or with faces without area only
            assert np.all(got[b, t][zero] == 0.0) and not np.any(np.signbit(got[b, t][zero]))
    print(f"{mesh} {weighting}: worst component error {worst:.3e} (limit {LIMIT:.3e}); hub/first vertex {got[0, 0, 0]}")
    assert worst <= LIMIT
    if mesh == "fan":
        assert zero[-1] and not zero[0] and abs(np.linalg.norm(got[0, 0, 0]) - 1.0) < 1e-15       # the unused vertex; the hub
    # one pose [V,3], an explicit table, and the cached table give the same values
    table = ops.vertex_corners(fd, clips.shape[-2])
    assert ops.vertex_corners(fd, clips.shape[-2]) is table
    offsets, corners = tc.model_corners(f, clips.shape[-2])
    assert np.array_equal(_host(table.offsets), offsets) and np.array_equal(_host(table.corners), corners)
    single = ops.vertex_normals(_dev(clips[1, 1], torch.float64), fd, (table.offsets.clone(), table.corners.clone()), weighting)
    assert np.array_equal(_host(single), got[1, 1])


def test_a_vertex_whose_contributions_cancel_is_exactly_zero():
    """Two faces over the same three vertices with opposite orientation: vertex 0 is corner 0 of both, its two contributions
    are w n and w (-n) with the same w, and the sum is exactly 0 -> the normal is 0, not 0 / 0.  Area weights cancel at all three."""
    from motion324_amd import ops
    v = np.array([[0.1, 0.2, 0.3], [0.7, 0.1, 0.25], [0.3, 0.9, 0.4], [0.5, 0.5, 0.9]])
    f = np.array([[0, 1, 2], [0, 2, 1], [1, 2, 3]])
    angle = _host(ops.vertex_normals(_dev(v), _dev(f, torch.int32)))
    area = _host(ops.vertex_normals(_dev(v), _dev(f[:2], torch.int32), weighting="area"))
    assert np.all(tc.model_vertex_normals(v, f)[0] == 0.0) and np.all(angle[0] == 0.0) and np.isfinite(angle).all()
    assert abs(np.linalg.norm(angle[3]) - 1.0) < 1e-15
    assert np.all(area == 0.0)


# ------------------------------------------------------------------------------------------------ 3. tracked normals
@pytest.mark.parametrize("mesh,B,T,num", [("blob", 2, 5, 1000), ("soup", 1, 3, 1000), ("fan", 3, 2, 300)])
def test_tracked_normals_are_within_the_limit_of_the_model_on_the_devices_vertex_normals(mesh, B, T, num):
    from motion324_amd import ops
    clips, f, _, _ = _clips(mesh, B, T)
    seeds = [11 + k for k in range(B)]
    vn = ops.vertex_normals(_dev(clips, torch.float64), _dev(f, torch.int32))
    s = _device_track(clips, f, seeds, num, normals=vn)
    assert tuple(s.normals.shape) == (B, T, num, 3) and s.normals.dtype == torch.float32 and s.colors is None
    worst = 0.0
    for k in range(B):
        r0, r1 = tc.model_weights(num, seeds[k])
        want = tc.model_track_normals(_host(vn[k]), f, _host(s.face_index[k]).astype(np.int64), r0, r1)
        worst = max(worst, np.abs(_host(s.normals[k]).astype(np.float64) - want).max())
    print(f"{mesh}: tracked normals, worst component error {worst:.3e} (limit {LIMIT:.3e})")
    assert worst <= LIMIT


def test_an_interpolated_normal_that_cancels_stays_zero():
    """One sample on the single-face mesh, whose weights (w0, r0, r1) the host knows: with n0 = (r0, 0, 0), n1 = (-w0, 0, 0) and
    n2 = 0 the interpolation is w0 r0 + r0 (-w0) -- two equal products of opposite sign -- and cancels to exactly 0.  The output
    is that 0 (the reference's `norms == 0 -> 1`), not 0 / 0.  A second item with the same normal at all three corners comes back
    as that normal."""
    clips, f, _, _ = _clips("one_face", 2, 2)
    seeds = [1, 2]
    r0, r1 = tc.model_weights(1, seeds[0])
    w0 = (1.0 - r0) - r1
    assert r0[0] > 0.0 and w0[0] > 0.0
    vn = torch.zeros((2, 2, 3, 3), dtype=torch.float64, device="cuda")
    vn[0, :, 0, 0], vn[0, :, 1, 0] = float(r0[0]), -float(w0[0])
    vn[1, :, :, 2] = 1.0
    s = _device_track(clips, f, seeds, 1, normals=vn)
    assert bool((s.normals[0] == 0.0).all()) and bool(torch.isfinite(s.normals).all())
    assert bool((s.normals[1, :, :, :2] == 0.0).all()) and bool((s.normals[1, :, :, 2] == 1.0).all())


def test_vertex_normals_that_are_all_zero_give_zero_not_nan():
    """samples on faces whose vertices have no area around them (zero vertex normals): m = 0 without any cancellation"""
    clips, f, _, _ = _clips("one_face", 1, 2)
    s = _device_track(clips, f, [3], 200, normals=torch.zeros((1, 2, 3, 3), dtype=torch.float64, device="cuda"))
    assert bool((s.normals == 0.0).all())


def test_the_first_frames_of_a_clip_are_tracked_in_place():
    """frames=k addresses the clip by its strides: the same values as tracking a copy of the first k frames"""
    from motion324_amd import ops
    clips, f, uv, tex = _clips("blob", 2, 5)
    v, fd = _dev(clips, torch.float64), _dev(f, torch.int32)
    vn, cdf, seeds = ops.vertex_normals(v, fd), ops.surface_cdf(v[:, 0], fd), _seeds([5, 6])
    for k in (1, 3, 5):
        part = ops.surface_track(v, fd, cdf, seeds, 300, vertex_normals=vn, face_uvs=_dev(uv), texture=_dev(tex), frames=k, want_points64=True)
        copy = ops.surface_track(v[:, :k].contiguous(), fd, cdf, seeds, 300, vertex_normals=vn[:, :k].contiguous(), face_uvs=_dev(uv),
                                 texture=_dev(tex), want_points64=True)
        assert tuple(part.points.shape) == (2, k, 300, 3)
        assert all(torch.equal(a, b) for a, b in zip(part, copy))
    with pytest.raises(Exception, match=r"frames must be in 1\.\.5"):
        ops.surface_track(v, fd, cdf, seeds, 300, frames=6)


# ------------------------------------------------------------------------------------------------ 4. determinism, streams
def test_two_runs_and_a_side_stream_give_the_same_bits():
    from motion324_amd import ops
    clips, f, uv, tex = _clips("soup", 2, 5)

    def run():
        vn = ops.vertex_normals(_dev(clips, torch.float64), _dev(f, torch.int32))
        s = _device_track(clips, f, [4, 6], 1000, uv, tex, normals=vn)
        return [vn, s.points, s.points64, s.normals, s.colors, s.face_index]

    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for a, b, c in zip(first, second, third):
        same = lambda x, y: torch.equal(x.view(torch.int64 if x.dtype == torch.float64 else torch.int32), y.view(torch.int64 if y.dtype == torch.float64 else torch.int32))
        assert same(a, b) and same(a, c)


def test_bad_arguments_are_refused_with_their_shapes():
    from motion324_amd import ops
    from motion324_amd.lib import M324Error
    clips, f, uv, tex = _clips("fan", 2, 3)
    v, fd = _dev(clips, torch.float64), _dev(f, torch.int32)
    cdf, seeds = ops.surface_cdf(v[:, 0], fd), _seeds([1, 2])
    with pytest.raises(M324Error, match="faces index vertices"):
        ops.vertex_normals(v, fd + clips.shape[-2])
    with pytest.raises(M324Error, match="corner table"):
        ops.vertex_normals(v, fd, (torch.zeros(5, dtype=torch.int32, device="cuda"), torch.zeros(3 * len(f), dtype=torch.int32, device="cuda")))
    with pytest.raises(M324Error, match="weighting"):
        ops.vertex_normals(v, fd, weighting="uniform")
    with pytest.raises(M324Error, match=r"seed pair\(s\) for vertices \(2, 3, 322, 3\)"):
        ops.surface_track(v, fd, cdf, _seeds([1, 2, 3]), 10)
    with pytest.raises(M324Error, match="cdf"):
        ops.surface_track(v, fd, cdf[0], seeds, 10)
    with pytest.raises(M324Error, match="shaped like vertices"):
        ops.surface_track(v, fd, cdf, seeds, 10, vertex_normals=v[:, :1])
    with pytest.raises(M324Error, match="both face_uvs and texture"):
        ops.surface_track(v, fd, cdf, seeds, 10, face_uvs=_dev(uv))
    with pytest.raises(M324Error, match=r"face_uvs fp64 \[320,3,2\]"):
        ops.surface_track(v, fd, cdf, seeds, 10, face_uvs=_dev(uv[:-1]), texture=_dev(tex))
    with pytest.raises(M324Error, match="num must be positive"):
        ops.surface_track(v, fd, cdf, seeds, 0)


# ------------------------------------------------------------------------------------------------ 5. training samples
def _clip_dict(k, T=3, HW=64):
    from motion324_amd import synth
    v, f = tc.fan()
    return dict(vertex_frames=tc.clip_of(v, T, 30 + k), faces=f, face_uvs=tc.corner_uvs(len(f), 8), texture_array=tc.texture(8),
                rgb_video=synth.uniform(30 + k, "track.video", (T, HW, HW, 3)))


TINY_SAMPLES = {"training": {"num_shape_samples": 100, "num_pcd_samples": 40}}


def test_training_sample_has_the_datasets_keys_shapes_and_dtypes():
    from motion324_amd import dataset
    c = _clip_dict(0)
    sample, finite = dataset.make_training_sample(c["vertex_frames"], c["faces"], c["face_uvs"], c["texture_array"], c["rgb_video"], TINY_SAMPLES,
                                                  seed=5, device="cuda")
    want = {"rgb_video": (3, 64, 64, 3), "point_clouds": (3, 40, 3), "point_rgbs": (3, 40, 3), "ref_shape_pcd": (100, 3),
            "ref_shape_normals": (100, 3), "ref_shape_rgbs": (100, 3), "ref_pcd": (40, 3), "ref_normal": (40, 3), "ref_rgb": (40, 3)}
    assert {k: tuple(t.shape) for k, t in sample.items()} == want
    assert all(t.dtype == torch.float32 and t.is_cuda for t in sample.values())
    assert finite.dtype == torch.bool and finite.is_cuda and finite.dim() == 0 and bool(finite)
    assert torch.equal(sample["ref_pcd"], sample["point_clouds"][0]) and torch.equal(sample["ref_rgb"], sample["point_rgbs"][0])
    assert torch.equal(sample["point_rgbs"][2], sample["point_rgbs"][0])
    # the two draws come from distinct streams, and each is the public function's draw for its derived seed
    assert not torch.equal(sample["ref_shape_pcd"][:40], sample["ref_pcd"])
    shape_seed, pcd_seed = dataset._draw_seeds(5)
    pts, nrm, rgb, _ = dataset.track_with_normal_rgb(c["vertex_frames"], c["faces"], 40, c["face_uvs"], c["texture_array"], seed=pcd_seed, device="cuda")
    assert torch.equal(pts, sample["point_clouds"]) and torch.equal(nrm[0], sample["ref_normal"]) and torch.equal(rgb, sample["point_rgbs"])
    pts, nrm, rgb, _ = dataset.track_with_normal_rgb(c["vertex_frames"][:1], c["faces"], 100, c["face_uvs"], c["texture_array"], seed=shape_seed,
                                                     device="cuda")
    assert torch.equal(pts[0], sample["ref_shape_pcd"]) and torch.equal(nrm[0], sample["ref_shape_normals"]) and torch.equal(rgb[0], sample["ref_shape_rgbs"])


def test_a_nan_vertex_makes_the_sample_not_finite():
    from motion324_amd import dataset
    c = _clip_dict(1)
    c["vertex_frames"] = c["vertex_frames"].copy()
    c["vertex_frames"][1, 0, 2] = np.nan                          # the hub, in frame 1: every tracked sample of that frame
    good = _clip_dict(2)
    batch, finite = dataset.make_training_batch([good, c], TINY_SAMPLES, [1, 2], device="cuda")
    assert finite.tolist() == [True, False]
    assert bool(torch.isfinite(batch["point_clouds"][0]).all()) and not bool(torch.isfinite(batch["point_clouds"][1]).all())


def test_the_corner_table_of_a_face_list_is_built_once(monkeypatch):
    """Every public device entry builds the vertex-corner table from the host faces on its first call with a face list and
    finds it again afterwards -- also when every call uploads fresh tensors -- and hands it to the kernels explicitly; an array
    changed in place is noticed and rebuilt."""
    from motion324_amd import dataset, ops
    built = []
    real = dataset.vertex_corners
    monkeypatch.setattr(dataset, "vertex_corners", lambda faces, nv: built.append(len(faces)) or real(faces, nv))
    monkeypatch.setattr(ops, "vertex_corners", lambda *a, **k: pytest.fail("the dataset path passes its table explicitly"))
    clips = [_clip_dict(0), _clip_dict(1)]
    faces = clips[0]["faces"].copy()                             # an object of this test's own: nothing cached for it yet
    for c in clips:
        c["faces"] = faces
    first, _ = dataset.make_training_batch(clips, TINY_SAMPLES, [1, 2], device="cuda")
    assert built == [len(faces)]
    again, _ = dataset.make_training_batch(clips, TINY_SAMPLES, [1, 2], device="cuda")
    c = clips[0]
    dataset.make_training_sample(c["vertex_frames"], faces, c["face_uvs"], c["texture_array"], c["rgb_video"], TINY_SAMPLES, seed=3, device="cuda")
    dataset.track_with_normal_rgb(c["vertex_frames"], faces, 50, c["face_uvs"], c["texture_array"], seed=3, device="cuda")
    assert built == [len(faces)] and all(torch.equal(first[k], again[k]) for k in first)
    faces[[0, 1]] = faces[[1, 0]]                                # the same object, another face list
    swapped, _ = dataset.make_training_batch(clips, TINY_SAMPLES, [1, 2], device="cuda")
    assert built == [len(faces)] * 2
    fresh = [dict(c, faces=faces.copy()) for c in clips]        # equal contents in new objects: built again, the same batch
    rebuilt, _ = dataset.make_training_batch(fresh, TINY_SAMPLES, [1, 2], device="cuda")
    assert built == [len(faces)] * 3 and all(torch.equal(swapped[k], rebuilt[k]) for k in swapped)
    tensor_faces = torch.from_numpy(faces).cuda()                # a device tensor: cached on identity and version
    for _ in range(2):
        dataset.track_with_normal_rgb(c["vertex_frames"], tensor_faces, 50, c["face_uvs"], c["texture_array"], seed=3, device="cuda")
    assert built == [len(faces)] * 4


def test_clips_of_different_meshes_are_built_one_by_one_and_collated():
    from motion324_amd import dataset, synth
    v, f = sc.blob()[:2]
    other = dict(vertex_frames=tc.clip_of(v, 3, 2), faces=f, face_uvs=tc.corner_uvs(len(f), 3), texture_array=tc.texture(3, 20, 30),
                 rgb_video=synth.uniform(2, "track.video", (3, 64, 64, 3)))
    clips = [_clip_dict(0), other]
    batch, finite = dataset.make_training_batch(clips, TINY_SAMPLES, [4, 5], device="cuda")
    assert finite.tolist() == [True, True]
    for k, (c, s) in enumerate(zip(clips, (4, 5))):
        single, _ = dataset.make_training_sample(c["vertex_frames"], c["faces"], c["face_uvs"], c["texture_array"], c["rgb_video"], TINY_SAMPLES,
                                                 seed=s, device="cuda")
        assert all(torch.equal(batch[name][k], single[name]) for name in dataset.SAMPLE_KEYS), k


def test_a_collated_batch_goes_through_a_training_step():
    import motion324_amd as m
    from motion324_amd import dataset, synth, training
    dims = CASES["tiny"]["dims"]
    dm = synth.Dims(**dims)
    cfg = synth.make_config(frames=dm.frames, d=dm.d, d_head=dm.d_head, tokens=dm.tokens, pcd_layers=dm.pcd_layers, n_layer=dm.n_layer)
    cfg["model"]["dino"] = {"depth": dm.dino_depth}
    cfg["training"].update(TINY_SAMPLES["training"])
    model = m.Motion_Latent_Model(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_sd(dims).items()}, strict=False)
    model = model.cuda().train()
    model.drop_rate = 0.0
    clips = [_clip_dict(0), _clip_dict(1)]
    singles = [dataset.make_training_sample(c["vertex_frames"], c["faces"], c["face_uvs"], c["texture_array"], c["rgb_video"], cfg, seed=s,
                                            device="cuda")[0] for c, s in zip(clips, (7, 8))]
    batch = dataset.collate(singles)
    together, finite = dataset.make_training_batch(clips, cfg, [7, 8], device="cuda")
    assert finite.tolist() == [True, True] and set(batch) == set(together) == set(dataset.SAMPLE_KEYS)
    for k in batch:                                              # one launch set for the batch = the samples one by one
        assert tuple(batch[k].shape)[0] == 2 and torch.equal(batch[k], together[k]), k
    loss, out, _ = training.forward_backward(model, batch)
    torch.cuda.synchronize()
    print(f"training step on a collated batch of tracked samples: loss {float(loss):.6f}")
    assert tuple(out.shape) == (2, 3, 40, 3) and np.isfinite(float(loss)) and bool(torch.isfinite(out).all())
