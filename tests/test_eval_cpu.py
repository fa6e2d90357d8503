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
