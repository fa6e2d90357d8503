"""Volumetric IoU on the device against the numpy model of tests/voxel_cases.py (written from include/m324.h): grids, outside
counts, fills and popcounts are compared with torch.equal, IoUs with ==.  There is no tolerance anywhere: every result is an
integer or a quotient of two integers formed on the host.  R = 16 with half 1 (G = 32, one word per row) and half 2 (G = 64, two
words per row: word index and bit order), 1..3 frames."""
import numpy as np
import pytest
import torch

import voxel_cases as vc

pytestmark = pytest.mark.gpu

CASES = vc.mesh_cases()
MODEL = {}


def model(name):
    """the model's (packed int32 grid, occupancy, outside) of a case, computed once"""
    if name not in MODEL:
        v, f, R, H = {**CASES, **vc.fill_cases()}[name]
        occ, outside = vc.voxelize(v, f, R, H)
        MODEL[name] = (vc.pack(occ), occ, outside)
    return MODEL[name]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run(name, **kw):
    from motion324_amd import ops
    v, f, R, H = {**CASES, **vc.fill_cases()}[name]
    grid, outside = ops.voxelize(dev(v), dev(f), R, H, **kw)
    torch.cuda.synchronize()
    return grid, outside


@pytest.mark.parametrize("name", list(CASES))
def test_voxelize_equals_the_model(name):
    v, f, R, H = CASES[name]
    want, occ, want_outside = model(name)
    grid, outside = run(name)
    G = vc.side(R, H)
    assert grid.shape == (len(v), G, G, G // 32) and grid.dtype == torch.int32 and outside.dtype == torch.int32
    print(name, "voxels per frame", occ.reshape(len(v), -1).sum(axis=1).tolist(), "outside", want_outside.tolist())
    assert torch.equal(outside.cpu(), torch.from_numpy(want_outside).to(torch.int32))
    assert torch.equal(grid.cpu(), torch.from_numpy(want))


def test_the_cases_are_what_their_names_say():
    """the model's view of the edge cases, so that an empty-equals-empty comparison cannot pass for one of them"""
    per_frame = lambda name: model(name)[1].reshape(len(CASES[name][0]), -1).sum(axis=1).tolist()
    assert per_frame("no_faces") == [0] and per_frame("one_face")[0] > 100
    occ = model("between_layers")[1][0]
    assert occ[31].any() and np.array_equal(occ[31], occ[32]) and not occ[30].any() and not occ[33].any()
    assert per_frame("point") == [1, 8, 1] and per_frame("corner_vertex")[0] != per_frame("corner_vertex")[1]
    assert per_frame("non_finite")[0] > per_frame("non_finite")[1] > 0 and per_frame("non_finite")[2] > 0
    assert model("outside")[2].tolist() == [2, 3, 1] and per_frame("outside")[1] == 0 and per_frame("outside")[0] > 0 and per_frame("outside")[2] > 0
    assert model("far")[2].tolist() == [3, 3] and min(per_frame("far")) > 32 and min(per_frame("whole_grid")) > 64 * 64
    assert model("soup")[2].min() > 0 and min(per_frame("soup")) > 5000


def test_the_grid_does_not_depend_on_the_work_distribution():
    """one triangle across the whole grid, and the soup: everything queued, nothing queued, and the default split"""
    for name in ("whole_grid", "soup", "far"):
        want = torch.from_numpy(model(name)[0])
        for big in (0, 2 ** 31 - 1, 8):
            grid, _ = run(name, big_voxels=big)
            assert torch.equal(grid.cpu(), want), (name, big)


def test_a_face_permutation_and_a_strided_clip_give_the_same_grid():
    from motion324_amd import ops
    v, f, R, H = CASES["soup"]
    want = torch.from_numpy(model("soup")[0])
    perm = np.random.default_rng(9).permutation(len(f))
    grid, _ = ops.voxelize(dev(v), dev(f[perm][:, [1, 2, 0]]), R, H)
    assert torch.equal(grid.cpu(), want)
    wide = torch.full((len(v), 2, v.shape[1], 3), float("nan"), device="cuda")
    wide[:, 0] = dev(v)
    view = wide[:, 0]
    assert not view.is_contiguous() and view.stride(0) == 2 * v.shape[1] * 3
    grid, outside = ops.voxelize(view, dev(f), R, H)
    assert torch.equal(grid.cpu(), want) and torch.equal(outside.cpu(), torch.from_numpy(model("soup")[2]).to(torch.int32))
    # a grid of one's own is zeroed by the call, and a caller's scratch is used
    out = torch.full((len(v), 64, 64, 2), -1, dtype=torch.int32, device="cuda")
    scratch = torch.empty((ops.voxel_plan(v.shape[1], len(f), len(v), R, H) + 64,), dtype=torch.uint8, device="cuda")
    got, _ = ops.voxelize(dev(v), dev(f), R, H, scratch=scratch, out=out)
    assert got is out and torch.equal(out.cpu(), want)


def test_faces_past_the_vertices_are_refused_before_any_launch():
    from motion324_amd import ops
    from motion324_amd.lib import M324Error
    v, f, R, H = CASES["one_face"]
    with pytest.raises(M324Error, match=r"voxelize: faces index vertices 0\.\.3, the mesh has 3"):
        ops.voxelize(dev(v), dev(np.array([[0, 1, 3]], dtype=np.int32)), R, H)
    with pytest.raises(M324Error, match=r"voxelize: faces index vertices -1\.\.2, the mesh has 3"):
        ops.voxelize(dev(v), dev(np.array([[0, -1, 2]], dtype=np.int32)), R, H)
    with pytest.raises(M324Error, match=r"expected \[F,3\] int32 faces"):
        ops.voxelize(dev(v), dev(np.zeros((2, 4), dtype=np.int32)), R, H)


@pytest.mark.parametrize("name", list(vc.fill_cases()))
def test_voxel_fill_equals_the_model(name):
    from motion324_amd import ops
    want_surface, occ, _ = model(name)
    want = torch.from_numpy(vc.pack(vc.fill(occ)))
    grid, _ = run(name)
    assert torch.equal(grid.cpu(), torch.from_numpy(want_surface))
    filled = ops.voxel_fill(grid)
    assert filled is not grid and torch.equal(filled.cpu(), want) and torch.equal(grid.cpu(), torch.from_numpy(want_surface))      # the source is untouched
    second = torch.full_like(grid, -1)
    assert ops.voxel_fill(grid, out=second) is second and torch.equal(second.cpu(), want)
    assert ops.voxel_fill(grid, out=grid) is grid and torch.equal(grid.cpu(), want)                                                # in place


def test_voxel_fill_per_frame_and_on_an_empty_grid():
    from motion324_amd import ops
    shell, cup = model("shell")[1], model("cup")[1]
    occ = np.concatenate([shell, np.zeros_like(shell), cup])
    filled = ops.voxel_fill(dev(vc.pack(occ)))
    assert torch.equal(filled.cpu(), torch.from_numpy(vc.pack(vc.fill(occ)))) and not filled[1].any()
    # G = 32: one word per row
    small = np.zeros((1, 32, 32, 32), dtype=bool)
    small[0, 3, 4, 5] = small[0, 3, 4, 30] = small[0, 3, 20, 7] = small[0, 28, 4, 7] = small[0, 28, 20, 7] = True
    assert torch.equal(ops.voxel_fill(dev(vc.pack(small))).cpu(), torch.from_numpy(vc.pack(vc.fill(small))))


def test_voxel_counts_equal_numpy_popcounts():
    from motion324_amd import ops
    a = np.concatenate([model("soup")[1], np.zeros((1, 64, 64, 64), dtype=bool)])
    b = np.concatenate([model("soup")[1][::-1], np.zeros((1, 64, 64, 64), dtype=bool)])
    b[1, 10:50, 7, 3:61] = True
    want = vc.counts(a, b)
    assert want[3].tolist() == [0, 0, 0] and want[1, 2] == want[1, 0] < want[1, 1] and 0 < want[0, 2] < want[0, 0]
    got = ops.voxel_counts(dev(vc.pack(a)), dev(vc.pack(b)))
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(want))
    full = np.ones((2, 32, 32, 32), dtype=bool)                              # every bit set, the sign bits included; G = 32
    full[1, ::2] = False
    got = ops.voxel_counts(dev(vc.pack(full)), dev(vc.pack(full[::-1].copy())))
    assert got.cpu().tolist() == [[32768, 16384, 16384], [16384, 32768, 16384]]


def test_compute_iou_voxel():
    from motion324_amd import evaluation as ev
    v, f = vc.box((-0.55, -0.4, -0.3), (0.45, 0.35, 0.5))
    far, _ = vc.box((1.2, 1.1, 1.0), (1.6, 1.7, 1.5))
    none = np.zeros((0, 3), dtype=np.int32)
    kw = dict(resolution=16, half=2, device="cuda")
    assert ev.compute_iou_voxel(v, f, v, f, **kw) == 1.0
    assert ev.compute_iou_voxel(v, f, far, f, **kw) == 0.0
    assert ev.compute_iou_voxel(v, none, v, none, **kw) == 0.0                # both empty: the reference's 0.0, not a division
    shifted = v + np.array([1 / 16, 0, 0], dtype=np.float32)                  # one pitch along x
    for fill in ("none", "orthographic"):
        a, _ = vc.voxelize(v[None], f, 16, 2)
        b, _ = vc.voxelize(shifted[None], f, 16, 2)
        if fill == "orthographic":
            a, b = vc.fill(a), vc.fill(b)
        want = vc.iou(vc.counts(a, b))[0]
        got = ev.compute_iou_voxel(v, f, shifted, f, fill=fill, **kw)
        print(fill, "counts", vc.counts(a, b).tolist(), "iou", got, "model", want)
        assert isinstance(got, float) and got == want and 0.0 < want < 1.0
    # clips: a [T] fp64 tensor, device tensors in, chunked to one frame per round by a small cap
    clip1, clip2 = np.stack([v, shifted, far]), np.stack([v, v, v])
    a, _ = vc.voxelize(clip1, f, 16, 2)
    b, _ = vc.voxelize(clip2, f, 16, 2)
    want = vc.iou(vc.counts(a, b))
    assert want[0] == 1.0 and want[2] == 0.0
    for cap in (1 << 30, 2 * 64 ** 3 // 8 + 4096):
        got = ev.compute_iou_voxel(dev(clip1), dev(f), dev(clip2), dev(f.astype(np.int64)), resolution=16, half=2, max_scratch_bytes=cap)
        assert got.dtype == torch.float64 and got.is_cuda and got.cpu().tolist() == want.tolist()


def test_voxelize_clip_chunks_fills_and_unpacks():
    from motion324_amd import evaluation as ev
    v, f, R, H = CASES["soup"]
    want_surface, occ, want_outside = model("soup")
    for cap in (1 << 30, 2 * 64 ** 3 // 8 + 65536):                          # everything at once; one frame per round
        grid, outside = ev.voxelize_clip(v, f, resolution=R, half=H, max_scratch_bytes=cap, device="cuda")
        assert torch.equal(grid.cpu(), torch.from_numpy(want_surface)) and outside.cpu().tolist() == want_outside.tolist()
        solid, _ = ev.voxelize_clip(dev(v), dev(f), resolution=R, half=H, fill="orthographic", max_scratch_bytes=cap)
        assert torch.equal(solid.cpu(), torch.from_numpy(vc.pack(vc.fill(occ))))
    assert torch.equal(ev.unpack_voxels(grid).cpu(), torch.from_numpy(occ))
    single, _ = ev.voxelize_clip(dev(v[0]), dev(f), resolution=R, half=H)
    assert torch.equal(single.cpu(), torch.from_numpy(want_surface[:1]))


def test_evaluate_sequence_adds_ious_and_leaves_the_rest_alone(tmp_path, capsys):
    from motion324_amd import evaluation as ev
    gt, gt_faces, pred, pred_faces = vc.sequence_clip()
    res = ev.evaluate_sequence(gt, gt_faces, pred, pred_faces, num_samples=256, seed=3, iou_resolution=16, iou_half=2)
    assert set(res) == {"chamfer_distances", "fscores", "R", "t", "s", "ious"} and len(res["ious"]) == 4
    plain = ev.evaluate_sequence(gt, gt_faces, pred, pred_faces, num_samples=256, seed=3, alignment=(res["R"], res["t"], res["s"]))
    assert set(plain) == {"chamfer_distances", "fscores", "R", "t", "s"}
    assert plain["chamfer_distances"] == res["chamfer_distances"] and plain["fscores"] == res["fscores"]
    # the model on the vertices the samplers get: the fp64 host transforms, rounded to fp32 once
    _, gc, gs = ev.normalize_points(gt[0])
    _, pc, ps = ev.normalize_points(pred[0])
    ga = np.stack([ev.apply_icp_alignment(ev.apply_normalization(gt[t], gc, gs), res["R"], res["t"], res["s"]) for t in range(4)]).astype(np.float32)
    pn = np.stack([ev.apply_normalization(pred[t], pc, ps) for t in range(4)]).astype(np.float32)
    for fill in ("none", "orthographic"):
        a, out_a = vc.voxelize(ga, gt_faces, 16, 2)
        b, out_b = vc.voxelize(pn, pred_faces, 16, 2)
        assert not out_a.any() and not out_b.any()
        if fill == "orthographic":
            a, b = vc.fill(a), vc.fill(b)
        want = vc.iou(vc.counts(a, b)).tolist()
        got = ev.evaluate_sequence(gt, gt_faces, pred, pred_faces, num_samples=256, seed=3, alignment=(res["R"], res["t"], res["s"]), iou_resolution=16,
                                   iou_fill=fill, sampler="device" if fill == "orthographic" else "host")
        print(fill, "ious", got["ious"], "model", want)
        assert got["ious"] == want and all(0.0 < x < 1.0 for x in want)
        if fill == "none":
            assert got["ious"] == res["ious"]
    # half = 1 does not hold the aligned clip (it spans [-1, 1] and moves): refused, naming the keyword
    with pytest.raises(ev.M324Error, match=r"beyond the voxel grid \[-1, 1\)\^3: raise iou_half"):
        ev.evaluate_sequence(gt * 1.3, gt_faces, pred, pred_faces, num_samples=256, seed=3, alignment=(np.eye(3), np.array([0.3, 0.0, 0.0]), 1.0),
                             iou_resolution=16, iou_half=1)
    # the command line: per-frame IoU, the summary line and the extra line of the results file
    for name, verts, faces in (("gt_case", gt, gt_faces), ("pred_case", pred, pred_faces)):
        (tmp_path / name).mkdir()
        np.save(tmp_path / name / "faces.npy", faces)
        for t in range(len(verts)):
            np.save(tmp_path / name / f"frame_{t:04d}.npy", verts[t])
    cli = ev.main(["--gt_path", str(tmp_path / "gt_case"), "--pred_path", str(tmp_path / "pred_case"), "--num_samples", "256", "--seed", "3", "--iou",
                   "--iou_resolution", "16"])
    out = capsys.readouterr().out
    assert cli["ious"] == res["ious"] and f"F-score: {res['fscores'][3]:.4f}, IoU: {res['ious'][3]:.4f}" in out and "IoU - Mean:" in out
    lines = open(tmp_path / "gt_case" / "evaluation_results.txt").read().split("\n")
    assert lines[3] == f"iou_mean_{np.mean(res['ious']):.6f}" and len(lines) == 5
