"""Geometry evaluation, the part that needs no GPU: the C ABI's argument validation and plan query (csrc/geometry.hip), the
host (numpy) paths of motion324_amd/evaluation.py against the reference's own outputs (tests/golden/eval_pcd.npz, made by
tests/golden/make_eval_golden.py), and the directory layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eval_inputs
from conftest import REPO, load_golden

GEOMETRY = ("m324_nn_plan", "m324_nn_search", "m324_dist_stats", "m324_transform_points", "m324_icp_moments")


def test_geometry_entry_points_are_declared_and_bound_at_abi_23():
    from motion324_amd import lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "m324.h")).read(), flags=re.S)
    for name in GEOMETRY:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SIGNATURES, name
    assert lib.ABI_VERSION == 23 and lib.load().m324_abi_version() == 23


@pytest.mark.parametrize("n_query,n_ref,batch", [(1, 1, 1), (64, 20000, 1), (10000, 10000, 1), (2048, 2048, 32), (50000, 50000, 32)])
def test_nn_plan_slices_and_scratch(n_query, n_ref, batch):
    from motion324_amd import lib
    h = lib.load()
    for forced in (0, 1, 2, 7):
        need = C.c_long(-1)
        slices = h.m324_nn_plan(n_query, n_ref, batch, forced, C.addressof(need))
        assert slices >= 1 and need.value >= slices * batch * n_query * 8, (forced, slices, need.value)
        if forced:
            assert slices == min(forced, n_ref)
        assert h.m324_nn_plan(n_query, n_ref, batch, forced, None) == slices          # the size is optional
    # few work items and a long reference set: the automatic choice slices
    assert h.m324_nn_plan(64, 20000, 1, 0, None) > 1


def test_nn_plan_refuses_non_positive_sizes():
    from motion324_amd import lib
    h = lib.load()
    for args in ((0, 5, 1, 0), (5, 0, 1, 0), (5, 5, 0, 0), (-1, 5, 1, 0), (5, 5, 1, -1)):
        assert h.m324_nn_plan(*args, None) == -1, args
        assert "m324_nn_plan" in lib.last_error()


def test_nn_search_validates_before_any_hip_call():
    """every refusal below returns -1 with a message on a machine without a GPU: the checks run before the first HIP call"""
    from motion324_amd import lib
    h = lib.load()
    P = 4096                                                     # a stand-in address: nothing is dereferenced
    ok = dict(query=P, sq=0, nq=8, ref=P, sr=0, nr=8, batch=1, dist=P, index=P, slices=0, scratch=None, nbytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return h.m324_nn_search(a["query"], a["sq"], a["nq"], a["ref"], a["sr"], a["nr"], a["batch"], a["dist"], a["index"], a["slices"],
                                a["scratch"], a["nbytes"], None)
    for kw, word in ((dict(query=None), "null"), (dict(ref=None), "null"), (dict(dist=None, index=None), "both outputs"),
                     (dict(nq=0), "positive"), (dict(nr=0), "positive"), (dict(batch=0), "positive"), (dict(nr=-3), "positive"),
                     (dict(slices=-1), "positive"),
                     (dict(nr=4096, slices=2, scratch=None, nbytes=0), "scratch"),
                     (dict(nr=4096, slices=2, scratch=P, nbytes=2 * 8 * 8 - 1), "scratch")):
        assert call(**kw) == -1, kw
        assert word in lib.last_error(), (kw, lib.last_error())
    assert h.m324_dist_stats(None, 4, 1, 0.02, None, None, None, None) == -1
    assert h.m324_transform_points(None, 4, None, None, None) == -1
    assert h.m324_icp_moments(None, 4, None, None, 4, None, None, None, None) == -1


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from motion324_amd import ops
    from motion324_amd.lib import M324Error
    pts = torch.zeros(8, 3)
    with pytest.raises(M324Error, match="HIP device"):
        ops.nn_search(pts, pts)
    with pytest.raises(M324Error, match="HIP device"):
        ops.dist_stats(torch.zeros(8), 0.02)
    with pytest.raises(M324Error, match="HIP device"):
        ops.transform_points(pts, torch.zeros(13, dtype=torch.float64))
    with pytest.raises(M324Error, match="HIP device"):
        ops.icp_moments(pts, torch.zeros(13, dtype=torch.float64), pts, torch.zeros(8, dtype=torch.int32))


def test_numpy_normalisation_paths_equal_the_reference_bit_for_bit():
    from motion324_amd import evaluation as ev
    g = load_golden("eval_pcd")
    v = eval_inputs.norm_case(int(g["seed"]))
    assert v.shape == (int(g["norm_vertices"]), 3) and v.dtype == np.float32
    vn, center, scale = ev.normalize_points(v)
    assert vn.dtype == np.float64
    assert np.array_equal(vn, g["norm_vertices_out"]) and np.array_equal(center, g["norm_center"]) and scale == float(g["norm_scale"])
    assert np.array_equal(ev.apply_normalization(v, center, scale), g["norm_applied"])
    aligned = ev.apply_icp_alignment(vn, g["icp_scaled_R"], g["icp_scaled_t"], float(g["icp_scaled_s"]))
    assert np.array_equal(aligned, g["norm_aligned"])
    # CUBE normalisation: the largest extent becomes 2, centred
    assert abs((vn.max(0) - vn.min(0)).max() - 2.0) < 1e-12 and np.abs(vn.max(0) + vn.min(0)).max() < 1e-12


def test_golden_inputs_regenerate_with_the_recorded_sizes():
    g = load_golden("eval_pcd")
    seed = int(g["seed"])
    src, tgt = eval_inputs.icp_case(seed)
    p1, p2 = eval_inputs.metric_case(seed)
    assert src.shape == (int(g["icp_source"]), 3) and tgt.shape == (int(g["icp_target"]), 3)
    assert p1.shape == p2.shape == (int(g["metric_points"]), 3) and p1.dtype == np.float32
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "eval_pcd.npz")) < 64 * 1024
    assert 10 <= int(g["icp_fixed_iterations"]) < 1000 and 10 <= int(g["icp_scaled_iterations"]) < 1000


def test_sequence_directory_round_trip_and_result_files(tmp_path):
    from motion324_amd import evaluation as ev
    gt = tmp_path / "case_0007"
    gt.mkdir()
    verts = np.arange(3 * 5 * 3, dtype=np.float32).reshape(3, 5, 3)
    faces = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int64)
    np.save(gt / "faces.npy", faces)
    for f in (2, 0, 1):                                          # written out of order: read back sorted
        np.save(gt / f"frame_{f:04d}.npy", verts[f])
    got_v, got_f = ev.load_sequence_dir(gt)
    assert np.array_equal(got_v, verts) and np.array_equal(got_f, faces)

    results = {"chamfer_distances": [0.0123456789, 0.02], "fscores": [0.5, 0.75], "R": np.eye(3), "t": np.array([0.1, 0.2, 0.3]), "s": 0.97}
    txt, npz = ev.write_results(gt, results)
    assert open(txt).read() == "case_0007\ncd_mean_0.016173\nfs_mean_0.625000\n"
    assert os.path.basename(txt) == "evaluation_results.txt" and os.path.basename(npz) == "icp_alignment_params.npz"
    saved = np.load(npz)
    assert np.array_equal(saved["R"], np.eye(3)) and np.array_equal(saved["t"], results["t"]) and float(saved["s"]) == 0.97


def test_a_file_path_is_refused_naming_the_directory_layout(tmp_path):
    from motion324_amd import evaluation as ev
    from motion324_amd.lib import M324Error
    f = tmp_path / "pred.glb"
    f.write_bytes(b"glTF")
    with pytest.raises(M324Error, match=r"faces\.npy and frame_0000\.npy"):
        ev.load_sequence_dir(f)
    with pytest.raises(M324Error, match=r"faces\.npy"):
        ev.load_sequence_dir(tmp_path)                           # a directory without the files


def test_evaluation_needs_none_of_the_reference_s_packages():
    """the product does not import scipy, trimesh, matplotlib or the checker"""
    text = open(os.path.join(REPO, "motion324_amd", "evaluation.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(scipy|trimesh|matplotlib|oracle)\b", text, flags=re.M)
    assert "torch.linalg" not in text


# ------------------------------------------------------------------------------------------------ the tables of geometry_cases.py
def _geometry_constants():
    """the work-decomposition constants, read from the text of csrc/geometry.hip"""
    text = open(os.path.join(REPO, "motion324_amd", "csrc", "geometry.hip")).read()

    def const(name):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert m, f"geometry.hip no longer defines {name} as a literal: tests/geometry_cases.py and this reader need another look"
        return int(m.group(1))
    qpl = re.search(r"#ifndef M324_NN_QPL\s*\n#define M324_NN_QPL (\d+)", text)
    assert qpl and "constexpr int NN_QPL = M324_NN_QPL;" in text and "constexpr int NN_TILE = NN_THREADS * NN_QPL;" in text
    stat = re.search(r"i < n; i \+= STAT_BLOCKS \* (\d+)\)", text)
    mom = re.search(r"i < n; i \+= MOM_BLOCKS \* (\d+)\)", text)
    assert stat and mom, "the grid strides of dist_stats / icp_moments are no longer STAT_BLOCKS * k / MOM_BLOCKS * k"
    c = {n: const(n) for n in ("NN_THREADS", "NN_CHUNK", "NN_MIN_SLICE", "NN_MAX_SLICES", "STAT_BLOCKS", "MOM_BLOCKS")}
    return dict(c, NN_QPL=int(qpl.group(1)), STAT_PASS=c["STAT_BLOCKS"] * int(stat.group(1)), MOM_PASS=c["MOM_BLOCKS"] * int(mom.group(1)))


def _straddles(values, boundary):
    return any(v < boundary for v in values) and boundary in values and any(v > boundary for v in values)


def test_geometry_tables_straddle_the_kernel_constants():
    """a retune of a constant in geometry.hip fails here; it does not silently move a table of geometry_cases.py off its boundary"""
    import geometry_cases as gc
    k = _geometry_constants()
    tile = k["NN_THREADS"] * k["NN_QPL"]
    assert (gc.TILE, gc.CHUNK, gc.MIN_SLICE, gc.MAX_SLICES, gc.STAT_PASS, gc.MOM_PASS) == \
        (tile, k["NN_CHUNK"], k["NN_MIN_SLICE"], k["NN_MAX_SLICES"], k["STAT_PASS"], k["MOM_PASS"]), k
    # one query tile: one below, exactly at, one above; a third tile; a ragged last tile behind full ones
    assert {tile - 1, tile, tile + 1} <= set(gc.TILE_QUERIES) and _straddles(gc.TILE_QUERIES, tile)
    assert any(2 * tile < n for n in gc.TILE_QUERIES) and any(n > tile and n % tile for n in gc.TILE_QUERIES)
    # one LDS chunk of reference records
    assert _straddles(gc.TILE_REFS, k["NN_CHUNK"]) and k["NN_CHUNK"] + 1 in gc.TILE_REFS
    # one pass of the grid-stride loops
    for sizes, one_pass in ((gc.STAT_SIZES, k["STAT_PASS"]), (gc.MOM_SIZES, k["MOM_PASS"])):
        assert {one_pass - 1, one_pass, one_pass + 1} <= set(sizes) and _straddles(sizes, one_pass), (sizes, one_pass)
        assert any(n > 2 * one_pass for n in sizes), "no size reaches a third pass"
        assert 1 in sizes
    # the slice limits: a forced count below, at and above NN_MAX_SLICES; a reference set the automatic rule may slice and one it never does
    asked = [f for case in gc.FORCED_CASES for f, _ in case.forced]
    assert _straddles(asked, k["NN_MAX_SLICES"])
    assert gc.GRID.n_ref // k["NN_MIN_SLICE"] >= 2 and gc.EMPTY.n_ref < k["NN_MIN_SLICE"]
    assert gc.GRID.batch > 1 and gc.GRID.n_query > 2 * tile and gc.GRID.n_ref > k["NN_CHUNK"]
    qtiles = -(-gc.GRID.n_query // tile)
    assert any(np.gcd(want, qtiles) > 1 for _, want in gc.GRID.forced), "with slices and query tiles coprime a swapped tile / slice digit only renumbers the work items"
    # what the tests plant sits where their names say
    assert gc.NAN_QUERY[0] > 0 and gc.NAN_QUERY[1] >= tile and gc.NAN_REF[1] < gc.GRID.n_ref
    assert gc.TIE_QUERY_TILE0 < tile and 2 * tile <= gc.TIE_QUERY_TILE2 < gc.TIE_QUERIES
    assert gc.TIE_LOW < k["NN_CHUNK"] <= gc.TIE_HIGH < gc.GRID.n_ref, "the planted pair shares a chunk of the one-slice call"
    for slices in [want for _, want in gc.GRID.forced if want > 1] + list(range(2, gc.GRID.n_ref // k["NN_MIN_SLICE"] + 1)):
        ps = gc.per_slice(gc.GRID.n_ref, slices)
        assert gc.TIE_LOW // ps != gc.TIE_HIGH // ps, f"the planted pair shares a slice at {slices} slices"
    assert any(p < k["STAT_PASS"] for p in gc.STAT_PLANTS) and any(p >= k["STAT_PASS"] for p in gc.STAT_PLANTS)
    assert max(gc.STAT_PLANTS) < gc.STAT_SIZES[-1] and k["STAT_PASS"] <= gc.STAT_INF_AT[1] < gc.STAT_SIZES[-1] and gc.STAT_INF_AT[0] > 0
    assert k["MOM_PASS"] <= gc.MOM_POISON_AT < gc.MOM_POISON_N and gc.MOM_POISON_N in gc.MOM_SIZES
    assert sorted(gc.MOM_MATCHED + gc.MOM_UNMATCHED) == list(range(30))
    assert all(n > tile for _, n in gc.CHAMFER_SHAPES) and gc.CHAMFER_SHAPES[0][1] != gc.CHAMFER_SHAPES[1][1]
    assert gc.ICP_BIG_SOURCE > k["MOM_PASS"]


def test_forced_slice_counts_of_the_geometry_table():
    import geometry_cases as gc
    from motion324_amd import lib
    h = lib.load()
    for case in gc.FORCED_CASES:
        for forced, want in case.forced:
            need = C.c_long(-1)
            assert want == min(forced, 64, case.n_ref), (case, forced, want)
            assert h.m324_nn_plan(case.n_query, case.n_ref, case.batch, forced, C.addressof(need)) == want, (case, forced)
            assert need.value == want * case.batch * case.n_query * 8
    # the empty-slice case really has empty trailing slices, and 7 slices of the grid case end in a ragged group of 4 records
    e = gc.EMPTY
    ps = gc.per_slice(e.n_ref, e.forced[0][1])
    assert ps * (e.forced[0][1] - 1) >= e.n_ref and ps == 2
    assert -(-e.n_ref // ps) == 35, "slices 35 .. 63 own nothing"
    assert gc.per_slice(gc.GRID.n_ref, 7) == 215 and 215 % 4 != 0


def test_geometry_references_agree_with_simpler_statements_of_themselves():
    import geometry_cases as gc
    # the brute-force search against torch.cdist, per-item and shared references, ties to the lowest index
    q, r = gc.unit_points(1, 3, 300), gc.unit_points(2, 3, 200)
    r[1, 150] = r[1, 20]                                         # an exact duplicate: index 20 must win
    q[1, 7] = r[1, 20]
    for rr in (r, r[0]):
        full = torch.cdist(q.double(), (rr if rr.dim() == 3 else rr[None].expand(3, -1, -1)).double(), compute_mode="donot_use_mm_for_euclid_dist")
        d1, idx, d2 = gc.brute_force_nn(q, rr, block=128)
        two = full.sort(dim=2).values[..., :2]
        assert float((d1 - full.min(dim=2).values).abs().max()) <= 1e-15 and float((d2 - two[..., 1]).abs().max()) <= 1e-15
        assert torch.equal(torch.gather(full, 2, idx[..., None])[..., 0], full.min(dim=2).values)
        assert float((gc.chosen_distance(q, rr, idx) - d1).abs().max()) == 0.0
    assert int(gc.brute_force_nn(q, r)[1][1, 7]) == 20 and float(gc.brute_force_nn(q, r)[2][1, 7]) == 0.0
    d1, idx, d2 = gc.brute_force_nn(q, r[:, :1])                 # one reference point: no second-nearest
    assert bool((idx == 0).all()) and bool(torch.isinf(d2).all())
    qn = q.clone()
    qn[2, 5, 1] = float("nan")                                   # a non-finite query has no neighbour below +inf
    assert float(gc.brute_force_nn(qn, r)[0][2, 5]) == float("inf")
    # the planted case names its own answer
    for shared in (False, True):
        pq, pr, assign = gc.planted_search_case(3, 2, 260, 100, shared)
        d1, idx, d2 = gc.brute_force_nn(pq, pr)
        assert torch.equal(idx, assign) and float(d1.max()) < 1.8e-3 and float((d2 - d1).min()) > 1e-5
        assert not torch.equal(assign[0], assign[1])
    # the moment record against a literal loop, and the absolute record above it
    src, tgt, index = gc.moment_case(257)
    assert int(index.min()) == 0 and int(index.max()) == gc.MOM_TARGET - 1
    params = gc.rigid_params(5)
    R = params[1:10].reshape(3, 3)
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-14 and float(torch.linalg.det(R)) > 0.99
    assert float((R - torch.eye(3, dtype=torch.float64)).abs().max()) > 0.1 and float(params[0]) == 1.03
    rec, rec_abs = gc.moment_record(src, params, tgt, index)
    loop = gc.moment_record_loop(src, params, tgt, index)
    assert rec[0] == 257.0 and rec[30] == rec[31] == 0.0
    assert np.all(np.abs(rec - loop) <= gc.moment_bound(257, rec_abs)), np.abs(rec - loop) / np.maximum(gc.moment_bound(257, rec_abs), 1e-300)
    assert np.all(rec_abs[1:30] >= np.abs(rec[1:30])) and np.all(np.abs(rec[1:30]) > 0)
    # the sums and counts
    d = gc.stat_input(255, 3)
    total, count, total_abs = gc.stats_reference(d, 0.02)
    assert np.abs(total - d.double().sum(dim=1).numpy()).max() <= 1e-13 and np.array_equal(total, total_abs)
    assert np.array_equal(count, [sum(1 for v in row.tolist() if v < 0.02) for row in d])
    assert not torch.equal(d[0], d[1])
    planted, below = gc.strict_input()
    assert gc.stats_reference(planted[None], gc.STAT_THRESHOLD)[1][0] == below == 2
    assert float(np.float32(0.02)) < 0.02                        # why float32(0.02) counts at threshold 0.02


def test_the_poison_check_catches_a_dropped_upper_bound_on_a_model_of_the_kernel():
    """`ok = j >= 0 && j < n_target` with the second half dropped would read one point past the target.  That defect is never run
    on a device: a CPU statement of the kernel's addressing on the sentinel-padded target shows that the check the GPU test applies
    (NaN in every entry that involves the matched point) turns it into a failure -- the sentinel arrives as a finite value."""
    import geometry_cases as gc
    n = 600
    src, tgt, index = gc.moment_case(n)
    params = gc.rigid_params(5)
    whole, _ = gc.padded(tgt, gc.TARGET_GUARD, gc.TARGET_SENTINEL)
    clean = gc.moments_model(src, params, whole, gc.MOM_TARGET, index)
    want, want_abs = gc.moment_record(src, params, tgt, index)
    assert np.all(np.abs(clean - want) <= gc.moment_bound(n, want_abs))          # the model is the record
    for bad in (-1, gc.MOM_TARGET):
        poisoned = index.clone()
        poisoned[n // 3] = bad
        gc.check_poisoned(gc.moments_model(src, params, whole, gc.MOM_TARGET, poisoned), clean)
    poisoned[n // 3] = gc.MOM_TARGET
    defect = gc.moments_model(src, params, whole, gc.MOM_TARGET, poisoned, drop_upper_bound=True)
    assert np.all(np.isfinite(defect)) and abs(defect[5] - clean[5]) > 1e4       # the sentinel went into sum m
    with pytest.raises(AssertionError, match="must be NaN"):
        gc.check_poisoned(defect, clean)


def test_the_chamfer_case_keeps_clear_of_the_threshold():
    """the seed of the multi-tile Chamfer / F-score case: no fp64 nearest distance within 1e-6 of the threshold (the golden maker's
    condition (a)), every distance below 0.2 (the Chamfer bound's premise), and a score that is neither 0 nor 1"""
    import geometry_cases as gc
    p1, p2 = gc.chamfer_case()
    assert tuple(p1.shape) == gc.CHAMFER_SHAPES[0] + (3,) and tuple(p2.shape) == gc.CHAMFER_SHAPES[1] + (3,) and p1.dtype == torch.float32
    chamfer, fscore, margin = gc.chamfer_reference(p1, p2)
    assert margin > 1e-6, margin
    assert float(gc.brute_force_nn(p1, p2)[0].max()) < 0.2 and float(gc.brute_force_nn(p2, p1)[0].max()) < 0.2
    assert np.all((fscore > 0.2) & (fscore < 0.9)) and fscore[0] != fscore[1] and chamfer[0] != chamfer[1]
