"""Geometry evaluation on the GPU (csrc/geometry.hip, motion324_amd/evaluation.py): the nearest-neighbour search against fp64
torch.cdist, its tie / slicing / batching / non-finite contracts, and Chamfer, F-score and ICP against the reference's own
outputs (tests/golden/eval_pcd.npz).  Bounds: tests/ERROR_BOUNDS_GEOMETRY.md."""
import numpy as np
import pytest
import torch

import eval_inputs
from conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL_F, SENTINEL_I = -7.5, -12345


def _unit_points(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, 3, generator=g)


def _raw_search(q, r, ref_slices=0):
    """m324_nn_search through the C ABI into guard-padded outputs; returns (dist, index) and checks the guards"""
    from motion324_amd import lib, ops
    B = q.shape[0] if q.dim() == 3 else (r.shape[0] if r.dim() == 3 else 1)
    nq, nr = q.shape[-2], r.shape[-2]
    slices, need = ops.nn_plan(nq, nr, B, ref_slices)
    dist = torch.full((B * nq + GUARD,), SENTINEL_F, dtype=torch.float32, device="cuda")
    index = torch.full((B * nq + GUARD,), SENTINEL_I, dtype=torch.int32, device="cuda")
    scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
    rc = lib.load().m324_nn_search(q.data_ptr(), nq * 3 if q.dim() == 3 else 0, nq, r.data_ptr(), nr * 3 if r.dim() == 3 else 0, nr, B,
                                   dist.data_ptr(), index.data_ptr(), ref_slices, scratch.data_ptr(), need,
                                   torch.cuda.current_stream().cuda_stream)
    lib.check(rc, "m324_nn_search")
    torch.cuda.synchronize()
    assert bool((dist[B * nq:] == SENTINEL_F).all()) and bool((index[B * nq:] == SENTINEL_I).all()), "guard rows were written"
    return dist[:B * nq].reshape(B, nq), index[:B * nq].reshape(B, nq)


# ------------------------------------------------------------------------------------------------ 1. search against fp64 cdist
@pytest.mark.parametrize("n_ref", [1, 1023, 1025, 5000])
@pytest.mark.parametrize("n_query", [1, 255, 257, 1000])
def test_nn_search_matches_fp64_cdist(n_query, n_ref):
    from motion324_amd import ops
    for batch in (1, 3):
        q = _unit_points(11 * n_query + batch, batch, n_query)
        r = _unit_points(13 * n_ref + batch, batch, n_ref)
        for shared in (False, True):
            rr = r[0] if shared else r                                       # a 2-D reference beside 3-D queries: stride 0
            full = torch.cdist(q.double(), (rr[None].expand(batch, -1, -1) if shared else rr).double())      # [B, nq, nr]
            want_d, want_i = full.min(dim=2)
            qd, rd = q.cuda(), rr.cuda()
            dist, index = _raw_search(qd, rd)
            got_d, got_i = dist.cpu().double(), index.cpu().long()
            assert int(got_i.min()) >= 0 and int(got_i.max()) < n_ref
            # the same index, or a point no more than 1e-6 farther (the rule of test_nearest_point_kernel_large)
            chosen = full.gather(2, got_i[..., None])[..., 0]
            assert float((chosen - want_d).max()) <= 1e-6, (batch, shared)
            assert float((got_d - want_d).abs().max()) <= 1e-6, (batch, shared, float((got_d - want_d).abs().max()))
            # the tensor-level wrapper returns the same bits, in every output combination
            o_d, o_i = ops.nn_search(qd, rd, want_dist=True, want_index=True)
            assert torch.equal(o_d, dist) and torch.equal(o_i, index)
            assert torch.equal(ops.nn_search(qd, rd), dist)                  # the distance-only instantiation
            assert torch.equal(ops.nn_search(qd, rd, want_dist=False, want_index=True), index)
    one = ops.nn_search(qd[0], rd)                                            # 2-D operands give 1-D results
    assert one.shape == (n_query,) and torch.equal(one, dist[0])


# ------------------------------------------------------------------------------------------------ 2. ties and slicing
def test_ties_go_to_the_lowest_index_for_every_slice_count():
    from motion324_amd import ops
    n_query, n_ref = 64, 20000
    base = _unit_points(5, n_ref // 4)
    r = torch.cat([base, base, base, base])                                   # every point four times: 5000 apart in index
    q = _unit_points(6, n_query)
    q[:8] = base[100:108]                                                     # exact hits: d2 = 0 four times over
    assert ops.nn_plan(n_query, n_ref, 1, 0)[0] > 1, "the automatic choice must take the sliced path at this size"
    for forced, want in ((1, 1), (2, 2), (7, 7)):
        assert ops.nn_plan(n_query, n_ref, 1, forced)[0] == want
    outs = [_raw_search(q.cuda(), r.cuda(), s) for s in (1, 2, 7, 0)]
    want_i = torch.cdist(q.double(), base.double()).argmin(dim=1)            # the first copy holds the lowest index
    for dist, index in outs:
        assert torch.equal(dist, outs[0][0]) and torch.equal(index, outs[0][1])          # bit-identical for every slice count
    index = outs[0][1][0].cpu().long()
    assert int(index.max()) < n_ref // 4, "a duplicate with a higher index won a tie"
    assert float((index == want_i).double().mean()) > 0.95
    assert torch.equal(index[:8], torch.arange(100, 108)) and bool((outs[0][0][0, :8] == 0).all())
    # distance-only through the sliced path: the same bits
    assert torch.equal(ops.nn_search(q.cuda(), r.cuda(), ref_slices=7), outs[0][0][0])


# ------------------------------------------------------------------------------------------------ 3. batching, non-finite input
def test_a_batch_equals_single_calls_and_a_nan_query_stays_alone():
    from motion324_amd import ops
    q, r = _unit_points(21, 5, 300), _unit_points(22, 5, 1500)
    q[2, 17] = float("nan")
    q[3, 40, 1] = float("inf")
    qd, rd = q.cuda(), r.cuda()
    dist, index = ops.nn_search(qd, rd, want_dist=True, want_index=True)
    for f in range(5):
        d1, i1 = ops.nn_search(qd[f], rd[f], want_dist=True, want_index=True)
        assert torch.equal(d1, dist[f]) and torch.equal(i1, index[f]), f
    only = ops.nn_search(qd, rd)
    assert torch.equal(only, dist)
    for f, i in ((2, 17), (3, 40)):
        assert float(dist[f, i]) == float("inf") and int(index[f, i]) == -1
    finite = torch.ones(5, 300, dtype=torch.bool)
    finite[2, 17] = finite[3, 40] = False
    want = torch.cdist(q.double(), r.double()).min(dim=2).values
    assert bool(torch.isfinite(dist.cpu()[finite]).all()) and int(index.cpu()[finite].min()) >= 0
    assert float((dist.cpu().double() - want)[finite].abs().max()) <= 1e-6
    # a non-finite distance propagates into the statistics
    total, count = ops.dist_stats(dist, 0.02)
    assert float(total[2]) == float("inf") and bool(torch.isfinite(total[[0, 1, 4]]).all())
    assert int(count[2]) == int((dist[2] < 0.02).sum())


def test_dist_stats_and_transform_points_against_fp64():
    from motion324_amd import ops
    g = torch.Generator().manual_seed(3)
    d = torch.rand(3, 5001, generator=g) * 0.05
    total, count = ops.dist_stats(d.cuda(), 0.02)
    assert total.dtype == torch.float64 and count.dtype == torch.int64
    assert float((total.cpu() - d.double().sum(dim=1)).abs().max()) < 1e-10
    assert torch.equal(count.cpu(), (d.double() < 0.02).sum(dim=1))
    t1, c1 = ops.dist_stats(d[1].cuda(), 0.02)
    assert float(t1) == float(total[1]) and int(c1) == int(count[1])          # deterministic, and independent of the batch
    x = _unit_points(4, 2, 777)
    R = torch.linalg.qr(torch.rand(3, 3, generator=g, dtype=torch.float64))[0]
    t = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    params = torch.cat([torch.tensor([0.97], dtype=torch.float64), R.reshape(9), t])
    got = ops.transform_points(x.cuda(), params.cuda())
    want = (0.97 * (x.double() @ R.T) + t).float()
    assert got.shape == x.shape and float((got.cpu() - want).abs().max()) <= 2 ** -23          # one rounding of a value below 2


# ------------------------------------------------------------------------------------------------ 4. metrics against the golden
@pytest.fixture(scope="module")
def golden():
    return load_golden("eval_pcd")


def test_chamfer_and_fscore_match_the_reference(golden):
    from motion324_amd import evaluation as ev
    p1, p2 = eval_inputs.metric_case(int(golden["seed"]))
    a, b = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
    chamfer = ev.compute_chamfer_distance(a, b)
    fscore = ev.compute_fscore(a, b, threshold=float(golden["threshold"]))
    print(f"chamfer {chamfer!r} (golden {float(golden['chamfer'])!r}), fscore {fscore!r} (golden {float(golden['fscore'])!r})")
    assert isinstance(chamfer, float) and isinstance(fscore, float)
    assert fscore == float(golden["fscore"])
    assert abs(chamfer - float(golden["chamfer"])) <= 1e-6
    both = ev.chamfer_and_fscore(a, b, float(golden["threshold"]))
    assert both == (chamfer, fscore)
    assert ev.compute_fscore(a, b) == fscore                                  # the default threshold is the reference's 0.02
    # numpy inputs are uploaded
    assert ev.compute_chamfer_distance(p1, p2) == chamfer
    # the [T,n,3] form equals the per-frame calls (frame 1: the sets swapped, frame 2: a set against itself)
    A, B = torch.stack([a, b, a]), torch.stack([b, a, a])
    cd, fs = ev.chamfer_and_fscore(A, B, float(golden["threshold"]))
    assert cd.dtype == torch.float64 and cd.shape == (3,) and fs.shape == (3,)
    for f in range(3):
        assert (float(cd[f]), float(fs[f])) == ev.chamfer_and_fscore(A[f], B[f], float(golden["threshold"])), f
    assert float(cd[2]) == 0.0 and float(fs[2]) == 1.0
    assert torch.equal(ev.compute_chamfer_distance(A, B), cd) and torch.equal(ev.compute_fscore(A, B), fs)
    far = a + 10.0                                                            # nothing within the threshold: the score is 0.0
    assert ev.compute_fscore(a, far) == 0.0


# ------------------------------------------------------------------------------------------------ 5. ICP
@pytest.mark.parametrize("tag,optimize_scale", [("fixed", False), ("scaled", True)])
def test_icp_matches_the_reference(golden, tag, optimize_scale, monkeypatch):
    from motion324_amd import evaluation as ev, ops
    calls = []
    real = ops.icp_moments
    monkeypatch.setattr(ops, "icp_moments", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    source, target = eval_inputs.icp_case(int(golden["seed"]))
    R, t, s = ev.icp_alignment(source, target, optimize_scale=optimize_scale)
    dR, dt, ds = np.abs(R - golden[f"icp_{tag}_R"]).max(), np.abs(t - golden[f"icp_{tag}_t"]).max(), abs(s - float(golden[f"icp_{tag}_s"]))
    print(f"icp[{tag}]: {len(calls)} iterations (golden {int(golden[f'icp_{tag}_iterations'])}), |dR| {dR:.3e} |dt| {dt:.3e} |ds| {ds:.3e}")
    assert R.dtype == np.float64 and R.shape == (3, 3) and t.shape == (3,) and isinstance(s, float)
    assert ds <= 1e-12
    assert dR <= 1e-6 and dt <= 1e-6
    assert len(calls) == int(golden[f"icp_{tag}_iterations"])
    # device tensors are accepted as well, with the same result
    R2, t2, s2 = ev.icp_alignment(torch.from_numpy(source).cuda(), torch.from_numpy(target).cuda(), optimize_scale=optimize_scale)
    assert np.array_equal(R2, R) and np.array_equal(t2, t) and s2 == s


def _recovery_case():
    """target: 2000 points of a blob that is longest in x; source: 500 of them (the two x-extremes among them, so that the
    initial x/y scale estimate is 1) moved by the inverse of a known 5 degree rotation about x and a 0.02 offset"""
    target = eval_inputs._blob(eval_inputs._directions(7, "eval.recovery", 2000), 0.0)
    order = np.argsort(target[:, 0])
    target = np.concatenate([target[order[[0, -1]]], target[order[1:-1]][np.argsort(eval_inputs.synth.uniform(7, "eval.shuffle", (1998,)))]])
    target = target.astype(np.float32).astype(np.float64)
    a = np.deg2rad(5.0)
    R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
    t = 0.02 * np.array([0.48, 0.6, -0.64])                                   # a unit direction: |t| = 0.02
    source = (target[:500] - t) @ R                                           # so that source @ R.T + t gives the originals
    return source.astype(np.float32), target.astype(np.float32), R, t


def test_icp_recovers_a_known_motion_and_stops_at_max_iterations(monkeypatch):
    from motion324_amd import evaluation as ev, ops
    source, target, R_true, t_true = _recovery_case()
    R, t, s = ev.icp_alignment(source, target)
    aligned = ev.apply_icp_alignment(source.astype(np.float64), R, t, s)
    err = np.abs(aligned - target[:500].astype(np.float64)).max()
    print(f"recovery: max |aligned - original| {err:.3e}, s {s!r}, |dR| {np.abs(R - R_true).max():.3e}")
    assert err <= 1e-5
    calls = []
    real = ops.icp_moments
    monkeypatch.setattr(ops, "icp_moments", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ev.icp_alignment(source, target, max_iterations=3)
    assert len(calls) == 3


# ------------------------------------------------------------------------------------------------ 6. evaluate_sequence
def _octahedron(level=3):
    v = [np.array(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, dtype=np.int64)


@pytest.fixture(scope="module")
def sequence():
    """a deforming sphere (258 vertices, 4 frames) and a prediction of it: slightly rotated, shifted, scaled and noisy"""
    v, faces = _octahedron(3)
    assert len(v) == 258
    frames = np.stack([v * (1.0 + 0.08 * f * np.sin(3.0 * v[:, :1] + 0.5 * f)) * np.array([1.0, 0.8, 0.7]) for f in range(4)])
    R = eval_inputs._rotation(3.0, -2.0)
    noise = 0.004 * eval_inputs.synth.normal(5, "eval.seq.noise", frames.shape).astype(np.float64)
    pred = 1.7 * (frames @ R.T) + np.array([0.4, -0.1, 0.2]) + noise
    return frames.astype(np.float32), faces, pred.astype(np.float32), faces[::-1].copy()


def _check_sequence(ev, preprocess, gt, gt_faces, pred, pred_faces, res, num_samples, seed, threshold=0.02):
    """fp64 numpy brute force on the same samples (same derived seeds, rounded to fp32 as the call uploads them) with the
    alignment the call returned"""
    T = len(pred)
    gt = np.concatenate([gt, np.repeat(gt[-1:], T - len(gt), axis=0)]) if len(gt) < T else gt
    _, gc, gs = ev.normalize_points(gt[0])
    _, pc, ps = ev.normalize_points(pred[0])
    assert len(res["chamfer_distances"]) == len(res["fscores"]) == T
    for f in range(T):
        ga = ev.apply_icp_alignment(ev.apply_normalization(gt[f], gc, gs), res["R"], res["t"], res["s"])
        a = preprocess.sample_surface(ga, gt_faces, num_samples, ev.sample_seed(seed, 0, f))[0].astype(np.float32).astype(np.float64)
        pn = ev.apply_normalization(pred[f], pc, ps)
        b = preprocess.sample_surface(pn, pred_faces, num_samples, ev.sample_seed(seed, 1, f))[0].astype(np.float32).astype(np.float64)
        d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))
        d_ab, d_ba = d.min(axis=1), d.min(axis=0)
        chamfer = d_ba.mean() + d_ab.mean()
        precision, recall = np.mean(d_ba < threshold), np.mean(d_ab < threshold)
        fscore = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
        print(f"frame {f}: chamfer {res['chamfer_distances'][f]!r} (checker {chamfer!r}), fscore {res['fscores'][f]!r} (checker {fscore!r})")
        assert abs(res["chamfer_distances"][f] - chamfer) <= 1e-6, f
        near = np.min(np.abs(np.concatenate([d_ab, d_ba]) - threshold)) <= 1e-6
        assert (abs(res["fscores"][f] - fscore) <= 1.0 / num_samples) if near else (res["fscores"][f] == fscore), f


def test_evaluate_sequence_against_a_brute_force_checker(sequence, monkeypatch):
    from motion324_amd import evaluation as ev, preprocess
    gt, gt_faces, pred, pred_faces = sequence
    res = ev.evaluate_sequence(gt, gt_faces, pred, pred_faces, num_samples=512, seed=3)
    assert set(res) == {"chamfer_distances", "fscores", "R", "t", "s"} and all(isinstance(c, float) for c in res["chamfer_distances"])
    _check_sequence(ev, preprocess, gt, gt_faces, pred, pred_faces, res, 512, 3)
    # device tensors in: the same result
    res_t = ev.evaluate_sequence(torch.from_numpy(gt).cuda(), gt_faces, torch.from_numpy(pred).cuda(), pred_faces, num_samples=512, seed=3)
    assert res_t["chamfer_distances"] == res["chamfer_distances"] and res_t["fscores"] == res["fscores"]
    # a shorter ground truth repeats its last frame; alignment= skips ICP
    monkeypatch.setattr(ev, "icp_alignment", lambda *a, **k: pytest.fail("alignment= was given: ICP must not run"))
    short = ev.evaluate_sequence(gt[:2], gt_faces, pred, pred_faces, num_samples=512, seed=3, alignment=(res["R"], res["t"], res["s"]))
    _check_sequence(ev, preprocess, gt[:2], gt_faces, pred, pred_faces, short, 512, 3)
    assert short["chamfer_distances"][:2] == res["chamfer_distances"][:2] and np.array_equal(short["R"], res["R"])


def test_cli_writes_the_reference_s_result_files(sequence, tmp_path, capsys):
    from motion324_amd import evaluation as ev
    gt, gt_faces, pred, pred_faces = sequence
    for name, verts, faces in (("gt_case", gt, gt_faces), ("pred_case", pred, pred_faces)):
        (tmp_path / name).mkdir()
        np.save(tmp_path / name / "faces.npy", faces)
        for f in range(len(verts)):
            np.save(tmp_path / name / f"frame_{f:04d}.npy", verts[f])
    res = ev.main(["--gt_path", str(tmp_path / "gt_case"), "--pred_path", str(tmp_path / "pred_case"), "--num_samples", "512", "--seed", "3"])
    out = capsys.readouterr().out
    assert "Frame 3 - Chamfer:" in out and "Chamfer Distance - Mean:" in out and "F-score - Mean:" in out
    lines = open(tmp_path / "gt_case" / "evaluation_results.txt").read().split("\n")
    assert lines == ["gt_case", f"cd_mean_{np.mean(res['chamfer_distances']):.6f}", f"fs_mean_{np.mean(res['fscores']):.6f}", ""]
    saved = np.load(tmp_path / "gt_case" / "icp_alignment_params.npz")
    assert np.array_equal(saved["R"], res["R"]) and np.array_equal(saved["t"], res["t"]) and float(saved["s"]) == res["s"]
    direct = ev.evaluate_sequence(gt, gt_faces, pred, pred_faces, num_samples=512, seed=3)
    assert direct["chamfer_distances"] == res["chamfer_distances"]
