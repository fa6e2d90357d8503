"""Volumetric IoU without a device: the numpy model of tests/voxel_cases.py against exact rational clipping, the fill rule on a
shell, a cup and a half-lidded cup, every refusal of the four m324_voxel* entry points (they validate before their first HIP
call) and of the Python layers above them, and the defaults that leave evaluate_sequence as it was."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import voxel_cases as vc


# ------------------------------------------------------------------------------------------------ the model itself
def test_the_13_axes_agree_with_exact_clipping():
    pairs = vc.pair_cases()
    assert len(pairs) == 400
    hits = 0
    for n, (tri, voxel) in enumerate(pairs):
        centre = 16 * np.array([voxel], dtype=np.int64) + 8
        model = bool(vc.overlap(tri, centre)[0])
        assert model == vc.clip_exact(tri, voxel), (n, tri.tolist(), voxel)
        hits += model
    assert 80 <= hits <= 320, hits                       # both answers are exercised


def test_touching_counts_and_degenerates_need_no_special_case():
    centre = np.array([[40, 40, 40]], dtype=np.int64)                       # voxel (2, 2, 2): the cube [32, 48]^3
    point = lambda p: np.array([p, p, p], dtype=np.int64)
    assert vc.overlap(point((48, 48, 48)), centre)[0] and vc.clip_exact(point((48, 48, 48)), (2, 2, 2))       # on a corner
    assert not vc.overlap(point((49, 40, 40)), centre)[0]
    plane = np.array([[0, 0, 48], [90, 0, 48], [0, 90, 48]], dtype=np.int64)                                   # the face z = 48
    assert vc.overlap(plane, centre)[0] and vc.overlap(plane, centre + np.array([0, 0, 16]))[0]                # both layers
    segment = np.array([[20, 20, 20], [60, 60, 60], [60, 60, 60]], dtype=np.int64)
    assert vc.overlap(segment, centre)[0] and vc.overlap(segment, centre + np.array([16, 0, 0]))[0]       # it passes through the shared corner
    assert not vc.overlap(segment, centre + np.array([32, 0, 0]))[0]


def test_snap_rounds_ties_to_even_and_counts_what_the_grid_does_not_hold():
    v = np.array([[[0.25 + 1 / 512, -0.125 - 1 / 512, 0.5 + 3 / 512], [1.0, -1.0, 0.0], [1.5, 0.0, np.nan], [0.0, -1.01, 0.0]]], dtype=np.float32)
    q, valid, outside = vc.snap(v, 16, 1)
    assert q[0, 0].tolist() == [320, 224, 386] and q[0, 1].tolist() == [512, 0, 256]
    assert valid[0].tolist() == [True, True, False, True] and outside.tolist() == [1]       # the NaN vertex is invalid, not outside


def test_pack_puts_voxel_i_in_bit_i_mod_32_and_unpack_voxels_reads_it_back():
    from motion324_amd import evaluation as ev
    occ = np.zeros((2, 64, 64, 64), dtype=bool)
    occ[0, 3, 2, 0] = occ[0, 3, 2, 31] = occ[0, 3, 2, 33] = occ[1, 63, 63, 63] = True
    words = vc.pack(occ)
    assert words.shape == (2, 64, 64, 2) and words.dtype == np.int32
    assert words[0, 3, 2].tolist() == [1 - 2 ** 31, 2] and words[1, 63, 63].tolist() == [0, -2 ** 31] and np.count_nonzero(words) == 3
    assert np.array_equal(ev.unpack_voxels(torch.from_numpy(words)).numpy(), occ)
    with pytest.raises(ev.M324Error, match="unpack_voxels: expected an int32 grid"):
        ev.unpack_voxels(torch.zeros((1, 64, 64, 3), dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the fill rule
@pytest.fixture(scope="module")
def filled():
    out = {}
    for name, (v, f, R, H) in vc.fill_cases().items():
        occ, outside = vc.voxelize(v, f, R, H)
        assert outside.tolist() == [0]
        out[name] = (occ[0], vc.fill(occ)[0])
    return out


def test_fill_makes_a_closed_shell_solid(filled):
    shell, solid = filled["shell"]
    assert (solid & shell).sum() == shell.sum()                             # the fill contains the surface
    k, j, i = np.nonzero(shell)
    box = np.zeros_like(shell)
    box[k.min():k.max() + 1, j.min():j.max() + 1, i.min():i.max() + 1] = True
    assert np.array_equal(solid, box) and solid.sum() > shell.sum() and not shell[28:39, 26:37, 24:39].any()


def test_fill_is_not_a_flood_fill(filled):
    """An open cup stays empty inside: nothing lies above its interior, so E_z fails there -- here the rule agrees with a flood
    fill from outside.  With a lid over the half x < -0.05 the interior under the lid is filled although it is connected to the
    outside through the open half, where a flood fill would drain all of it; the column under the opening stays empty."""
    cup, cup_filled = filled["cup"]
    assert np.array_equal(cup_filled, cup)                                  # only the surface itself
    lid, lid_filled = filled["half_lid"]
    k, j, i = np.nonzero(lid)
    # x = -0.05 snaps to 499.2 -> 499: the lid ends in voxel i = 31; interior columns run over y 26..36 (j), z 28..39 (k)
    under = lid_filled[28:40, 26:37, 24:32]
    beside = lid_filled[28:40, 26:37, 32:39]
    assert under.all() and not beside.any()
    assert not lid[28:39, 26:37, 24:39].any() and i.min() == 23 and i.max() == 39 and k.max() == 40


# ------------------------------------------------------------------------------------------------ the C entry points
P = 4096        # an aligned stand-in for a device pointer: every call below returns before it would be used


def _refused(rc, text):
    from motion324_amd import lib
    assert rc == -1 and text in lib.last_error(), (rc, lib.last_error())


def test_voxel_plan_counts_the_snapped_vertices_and_the_queue():
    from motion324_amd import lib, ops
    h = lib.load()
    need = ctypes.c_long(-1)
    assert h.m324_voxel_plan(100, 50, 3, 128, 2, ctypes.addressof(need)) == 0
    assert need.value == 256 + 4864 + 768                                   # counter, 300 * 16 and 150 * 4 bytes, each rounded up to 256
    assert ops.voxel_plan(100, 50, 3, 128, 2) == need.value and h.m324_voxel_plan(100, 0, 1, 16, 1, None) == 0
    assert ops.voxel_plan(1, 0, 1, 16, 1) == 512
    for args, text in (((100, 50, 3, 120, 2), "multiple of 16"), ((100, 50, 3, 0, 2), "multiple of 16"), ((100, 50, 3, 16, 0), "must be in 32..1024"),
                       ((100, 50, 3, 128, 5), "must be in 32..1024"), ((100, 50, 3, 512, 2), "must be in 32..1024"), ((0, 50, 3, 128, 2), "n_vertices >= 1"),
                       ((100, -1, 3, 128, 2), "n_faces >= 0"), ((100, 50, 0, 128, 2), "frames >= 1"), ((2 ** 30, 1, 2, 128, 2), "below 2^31"),
                       ((1, 2 ** 30, 2, 128, 2), "below 2^31")):
        _refused(h.m324_voxel_plan(*args, None), text)
    assert ops.voxel_side(128, 4) == 1024 and ops.voxel_side(16, 1) == 32


def test_voxelize_refuses_before_any_launch():
    from motion324_amd import lib
    h = lib.load()
    good = dict(vertices=P, stride_t=300, n_vertices=100, faces=P, n_faces=50, frames=3, resolution=16, half=2, big_voxels=64, grid=P, outside=P,
                scratch=P, scratch_bytes=1 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return h.m324_voxelize(*[a[k] for k in good], None)
    for kw, text in ((dict(vertices=None), "null"), (dict(grid=None), "null"), (dict(outside=None), "null"), (dict(scratch=None), "null"),
                     (dict(faces=None), "null"), (dict(resolution=24), "multiple of 16"), (dict(half=40), "must be in 32..1024"),
                     (dict(frames=0), "frames >= 1"), (dict(stride_t=-1), "stride_t"), (dict(big_voxels=-1), "big_voxels"),
                     (dict(scratch_bytes=5887), "needs 5888 scratch bytes"), (dict(scratch=P + 8), "16-byte aligned"), (dict(grid=P + 2), "4-byte aligned")):
        _refused(call(**kw), text)


def test_fill_and_counts_refuse_before_any_launch():
    from motion324_amd import lib
    h = lib.load()
    grid_bytes = 2 * 64 * 64 * 2 * 4
    for args, text in (((None, P, 2, 64, None, 0), "null"), ((P, None, 2, 64, None, 0), "null"), ((P, 2 * P, 2, 48, None, 0), "multiple of 32"),
                       ((P, 2 * P, 2, 2048, None, 0), "multiple of 32"), ((P, 2 * P, 0, 64, None, 0), "frames must be positive"),
                       ((P, P + 2, 2, 64, None, 0), "4-byte aligned"), ((P, P, 2, 64, None, 0), f"needs {grid_bytes} scratch bytes"),
                       ((P, P, 2, 64, 2 * P, grid_bytes - 1), f"needs {grid_bytes} scratch bytes"), ((P, P + 4096, 2, 64, None, 0), "overlaps")):
        _refused(h.m324_voxel_fill(*args, None), text)
    for args, text in (((None, P, 2, 64, P), "null"), ((P, None, 2, 64, P), "null"), ((P, P, 2, 64, None), "null"), ((P, P, 2, 40, P), "multiple of 32"),
                       ((P, P, 0, 64, P), "frames must be in 1..65535"), ((P, P, 65536, 64, P), "frames must be in 1..65535"),
                       ((P + 4, P, 2, 64, P), "16-byte aligned"), ((P, P, 2, 64, P + 4), "8-byte aligned")):
        _refused(h.m324_voxel_counts(*args, None), text)


# ------------------------------------------------------------------------------------------------ the Python layers
def test_ops_refuse_host_tensors_and_bad_grids():
    from motion324_amd import ops
    from motion324_amd.lib import M324Error
    v, f = torch.zeros((1, 3, 3)), torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(M324Error, match="voxelize: vertices: libm324 ops need HIP device tensors"):
        ops.voxelize(v, f, 16, 1)
    for resolution, half, text in ((24, 2, "multiple of 16"), (0, 2, "multiple of 16"), (16.5, 2, "integers"), (16, 0, "must be in 32..1024"),
                                   (128, 5, "must be in 32..1024"), (1024, 1, "must be in 32..1024")):
        with pytest.raises(M324Error, match=text):
            ops.voxelize(v, f, resolution, half)                            # the grid is refused before the tensors are looked at
    grid = torch.zeros((1, 32, 32, 1), dtype=torch.int32)
    with pytest.raises(M324Error, match="voxel_fill: libm324 ops need HIP device tensors"):
        ops.voxel_fill(grid)
    with pytest.raises(M324Error, match="voxel_counts: a: libm324 ops need HIP device tensors"):
        ops.voxel_counts(grid, grid)


def test_evaluation_wrappers_refuse_on_shapes_alone():
    from motion324_amd import evaluation as ev
    v = np.zeros((4, 3), dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int64)
    for call in (lambda **kw: ev.compute_iou_voxel(kw.pop("v", v), kw.pop("f", f), v, f, **kw), lambda **kw: ev.voxelize_clip(kw.pop("v", v), kw.pop("f", f), **kw)):
        with pytest.raises(ev.M324Error, match="a host array needs device="):
            call()
        with pytest.raises(ev.M324Error, match="a host array needs device="):
            call(v=torch.zeros((4, 3)))                                     # a CPU tensor is a host array too
        with pytest.raises(ev.M324Error, match="multiple of 16"):
            call(resolution=100)
        with pytest.raises(ev.M324Error, match=r"must be in 32\.\.1024"):
            call(resolution=128, half=5)
        with pytest.raises(ev.M324Error, match=r"must be in 32\.\.1024"):
            call(resolution=16, half=0)
        with pytest.raises(ev.M324Error, match="fill must be one of"):
            call(fill="flood")
        with pytest.raises(ev.M324Error, match=r"expected faces \[F,3\]"):
            call(f=np.zeros((2, 4), dtype=np.int64))
        with pytest.raises(ev.M324Error, match="faces are integers"):
            call(f=np.zeros((2, 3), dtype=np.float32))
        with pytest.raises(ev.M324Error, match=r"faces index vertices 0\.\.4, the mesh has 4"):
            call(f=np.array([[0, 1, 4]]))
        with pytest.raises(ev.M324Error, match=r"faces index vertices -1\.\.2, the mesh has 4"):
            call(f=np.array([[0, -1, 2]]))
        with pytest.raises(ev.M324Error, match=r"expected vertices \[V,3\] or \[T,V,3\]"):
            call(v=np.zeros((4, 2), dtype=np.float32))
        with pytest.raises(ev.M324Error, match="max_scratch_bytes is 1000"):
            call(max_scratch_bytes=1000, device="cuda")                     # sized on the host: refused before the upload
    with pytest.raises(ev.M324Error, match="two clips of one length"):
        ev.compute_iou_voxel(np.zeros((2, 4, 3), dtype=np.float32), f, np.zeros((3, 4, 3), dtype=np.float32), f, device="cuda", max_scratch_bytes=1000)


def test_evaluate_sequence_leaves_iou_off_by_default():
    from motion324_amd import evaluation as ev
    p = inspect.signature(ev.evaluate_sequence).parameters
    assert p["iou_resolution"].default is None and p["iou_half"].default == 2 and p["iou_fill"].default == "none"
    assert list(p)[:9] == ["gt_vertices", "gt_faces", "pred_vertices", "pred_faces", "num_samples", "seed", "threshold", "alignment", "sampler"]
    q = inspect.signature(ev.compute_iou_voxel).parameters
    assert q["resolution"].default == 128 and q["half"].default == 2 and q["fill"].default == "none"      # the reference's name and resolution
    v = np.zeros((1, 4, 3), dtype=np.float32)
    f = np.array([[0, 1, 2]])
    with pytest.raises(ev.M324Error, match="multiple of 16"):
        ev.evaluate_sequence(v, f, v, f, iou_resolution=100)               # refused before anything is sampled or uploaded
    with pytest.raises(ev.M324Error, match="iou_fill: fill must be one of"):
        ev.evaluate_sequence(v, f, v, f, iou_resolution=16, iou_fill="solid")


def test_write_results_adds_the_iou_line_only_when_scored(tmp_path):
    from motion324_amd import evaluation as ev
    base = {"chamfer_distances": [0.5, 0.25], "fscores": [0.75, 0.5]}
    txt, npz = ev.write_results(tmp_path / "case_a", base)
    assert open(txt).read().split("\n") == ["case_a", "cd_mean_0.375000", "fs_mean_0.625000", ""] and npz is None
    txt, _ = ev.write_results(tmp_path / "case_b", dict(base, ious=[0.5, 0.125]))
    assert open(txt).read().split("\n") == ["case_b", "cd_mean_0.375000", "fs_mean_0.625000", "iou_mean_0.312500", ""]
