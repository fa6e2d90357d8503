"""Surface sampler on the GPU (csrc/surface.hip) against its two references: the numpy model of the CDF's nested scan
(tests/surface_cases.py) and the host sampler preprocess.sample_surface, whose samples the device must draw bit for bit; the
texture colours against the reference's own code (tests/golden/sampler_tex.npz); and the callers that switch samplers.

Where the device may differ from the host at all, the difference is an exemption with a cap, not a tolerance:
  * a draw whose u * total lies within 4 F 2^-53 total of a host CDF entry may land on a neighbouring face (np.cumsum and the
    nested scan round the partial sums differently, each within F 2^-53 total); at most 0.1 % of a draw, none on these inputs;
  * a texture coordinate within 1e-9 of an integer may land in the neighbouring texel (the reference recomputes the weights
    from the point, the device uses the drawn ones); at most 0.1 %, none on the golden's inputs."""
import numpy as np
import pytest
import torch

import surface_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu
GUARD = 64


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _seeds(seed):
    from motion324_amd import preprocess
    table = preprocess.surface_seeds(seed)
    return _dev(table if np.ndim(seed) else table[0])


def _draw(v, f, num, seed, **want):
    """device draw through motion324_amd.ops; v [V,3] with an int seed or [B,V,3] with B seeds"""
    from motion324_amd import ops
    vd, fd = _dev(v, torch.float64), _dev(f, torch.int32)
    return ops.surface_sample(vd, fd, ops.surface_cdf(vd, fd), _seeds(seed), num, want_points64=True, **want)


def _host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. CDF
def _raw_cdf(v, f, batch, shared):
    """m324_surface_cdf through the C ABI into a guard-padded table; checks the guards"""
    from motion324_amd import lib, ops
    vd, fd = _dev(v, torch.float64), _dev(f, torch.int32)
    nf = len(f)
    blocks, need = ops.surface_plan(nf, batch)
    out = torch.full((batch * nf + GUARD,), -7.0, dtype=torch.float64, device="cuda")
    scratch = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = lib.load().m324_surface_cdf(vd.data_ptr(), 0 if shared else v.shape[-2] * 3, v.shape[-2], fd.data_ptr(), nf, batch, out.data_ptr(),
                                     scratch.data_ptr() if need else None, need, torch.cuda.current_stream().cuda_stream)
    lib.check(rc, "m324_surface_cdf")
    torch.cuda.synchronize()
    assert bool((out[batch * nf:] == -7.0).all()) and bool((scratch[need:] == 0x5A).all()), "guard overwritten"
    return _host(out[:batch * nf]).reshape(batch, nf)


@pytest.mark.parametrize("n_faces", [1, 15, 16, 17, 1023, 1024, 1025, 2049, 16389])
def test_cdf_equals_the_numpy_model_bit_for_bit(n_faces):
    from motion324_amd import ops
    v, f = sc.random_mesh(n_faces, max(3, n_faces // 2 + 2), 100 + n_faces)
    items = np.stack([v, 1.7 * v + 0.3, 0.01 * v[::-1]])
    want = [sc.model_cdf(sc.model_areas(x, f)) for x in items]
    assert np.array_equal(_raw_cdf(v, f, 1, True)[0], want[0])
    assert np.array_equal(_raw_cdf(items[:1], f, 1, False)[0], want[0])
    shared = _raw_cdf(v, f, 3, True)                             # one mesh for every item: three equal rows
    assert all(np.array_equal(row, want[0]) for row in shared)
    per_item = _raw_cdf(items, f, 3, False)
    for k in range(3):
        assert np.array_equal(per_item[k], want[k]), k
    # the wrapper: the same tables, shaped like the vertices
    assert np.array_equal(_host(ops.surface_cdf(_dev(items), _dev(f, torch.int32))), per_item)
    assert np.array_equal(_host(ops.surface_cdf(_dev(v), _dev(f, torch.int32))), want[0])
    with pytest.raises(Exception, match="faces index vertices"):
        ops.surface_cdf(_dev(v), _dev(f, torch.int32) + len(v))


# ------------------------------------------------------------------------------------------------ 2. samples, exact case
@pytest.mark.parametrize("num", [1, 255, 256, 257, 4099])
def test_samples_on_a_grid_mesh_equal_the_host_sampler_bit_for_bit(num):
    from motion324_amd import preprocess
    v, f = sc.grid_mesh()
    for seed in (0, 3, 2 ** 40 + 1):
        pts, fi = preprocess.sample_surface(v, f, num, seed)
        s = _draw(v, f, num, seed)
        assert s.face_index.dtype == torch.int32 and np.array_equal(_host(s.face_index), fi), seed
        assert np.array_equal(_host(s.points64), pts) and np.array_equal(_host(s.points), pts.astype(np.float32)), seed
        p32, fi64 = preprocess.sample_surface_device(v, f, num, seed, "cuda")
        assert p32.is_cuda and p32.dtype == torch.float32 and fi64.dtype == torch.int64
        assert np.array_equal(_host(p32), pts.astype(np.float32)) and np.array_equal(_host(fi64), fi)


def test_a_batch_of_three_meshes_and_seeds_equals_three_single_calls():
    from motion324_amd import preprocess
    meshes = [sc.grid_mesh(seed=k) for k in range(3)]
    f = meshes[0][1]
    assert all(np.array_equal(m[1], f) for m in meshes) and not np.array_equal(meshes[0][0], meshes[1][0])
    seeds, num = [5, 9, 2 ** 33], 777
    batch = _draw(np.stack([m[0] for m in meshes]), f, num, seeds, want_normals=True, want_colors=True)
    assert tuple(batch.points.shape) == (3, num, 3) and tuple(batch.face_index.shape) == (3, num)
    for k in range(3):
        single = _draw(meshes[k][0], f, num, seeds[k], want_normals=True, want_colors=True)
        pts, fi = preprocess.sample_surface(meshes[k][0], f, num, seeds[k])
        for name in ("points", "points64", "face_index", "normals", "colors"):
            assert torch.equal(getattr(batch, name)[k], getattr(single, name)), (k, name)
        assert np.array_equal(_host(batch.points64[k]), pts) and np.array_equal(_host(batch.face_index[k]), fi), k
    assert bool((batch.colors == 0.5).all())                     # no colour source: grey
    p32, fi64 = preprocess.sample_surface_device(np.stack([m[0] for m in meshes]), f, num, seeds, "cuda")
    assert torch.equal(p32, batch.points) and torch.equal(fi64, batch.face_index.long())


def test_a_mesh_without_area_puts_every_sample_on_the_last_face():
    from motion324_amd import preprocess
    v, f = sc.grid_mesh(4, 4)
    f = f.copy()
    f[:, 2] = f[:, 1]
    pts, fi = preprocess.sample_surface(v, f, 300, 2)
    assert np.all(fi == len(f) - 1)
    s = _draw(v, f, 300, 2, want_normals=True)
    assert np.array_equal(_host(s.face_index), fi) and np.array_equal(_host(s.points64), pts)
    assert bool((s.normals == 0).all())


def test_nothing_is_written_past_num_entries_and_null_outputs_are_skipped():
    """m324_surface_sample through the C ABI: every output guard-padded, then only the required one"""
    from motion324_amd import lib, ops
    v, f, colors = sc.blob()
    vd, fd, cd = _dev(v), _dev(f, torch.int32), _dev(colors)
    cdf = ops.surface_cdf(vd, fd)
    num, seeds = 257, _seeds(4)
    stream = torch.cuda.current_stream().cuda_stream

    def padded(n, dtype, fill):
        return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    p32, p64, fi = padded(num * 3, torch.float32, -7.0), padded(num * 3, torch.float64, -7.0), padded(num, torch.int32, -7)
    nrm, rgb = padded(num * 3, torch.float32, -7.0), padded(num * 3, torch.float32, -7.0)
    lib.check(lib.load().m324_surface_sample(vd.data_ptr(), 0, len(v), fd.data_ptr(), len(f), cdf.data_ptr(), seeds.data_ptr(), num, 1, p32.data_ptr(),
                                             p64.data_ptr(), fi.data_ptr(), nrm.data_ptr(), rgb.data_ptr(), cd.data_ptr(), 4, None, None, 0, 0, stream),
              "m324_surface_sample")
    torch.cuda.synchronize()
    for t, n in ((p32, num * 3), (p64, num * 3), (fi, num), (nrm, num * 3), (rgb, num * 3)):
        assert bool((t[n:] == -7).all()) and bool((t[:n] != -7).all())
    only = padded(num * 3, torch.float32, -7.0)
    lib.check(lib.load().m324_surface_sample(vd.data_ptr(), 0, len(v), fd.data_ptr(), len(f), cdf.data_ptr(), seeds.data_ptr(), num, 1, only.data_ptr(),
                                             None, None, None, None, None, 0, None, None, 0, 0, stream), "m324_surface_sample")
    torch.cuda.synchronize()
    assert torch.equal(only, p32)


def test_the_face_index_stays_in_range_for_non_finite_vertices():
    v, f, _ = sc.blob()
    v = v.copy()
    v[::5] = np.nan
    v[3] = np.inf
    s = _draw(v, f, 2000, 1)
    fi = _host(s.face_index)
    assert fi.min() >= 0 and fi.max() <= len(f) - 1


# ------------------------------------------------------------------------------------------------ 3. samples, general case
@pytest.fixture(scope="module")
def general():
    """per mesh: inputs, the host sampler's draw with normals and colours, the device's, the exemption mask"""
    from motion324_amd import preprocess
    out = {}
    for name, (v, f, colors), num in (("blob", sc.blob(), 4096), ("soup", sc.soup(), 50000)):
        pts, fi = preprocess.sample_surface(v, f, num, 5)
        host = preprocess.sample_pointcloud_with_albedo(v, f, num, colors, 5)
        dev = _draw(v, f, num, 5, want_normals=True, want_colors=True, vertex_colors=_dev(colors))
        out[name] = dict(v=v, f=f, colors=colors, num=num, pts=pts, fi=fi, host=host, dev=dev, exempt=sc.near_cdf_entry(v, f, num, 5))
    return out


@pytest.mark.parametrize("mesh", ["blob", "soup"])
def test_general_meshes_draw_the_host_s_faces_and_points(general, mesh):
    g = general[mesh]
    exempt = g["exempt"]
    print(f"{mesh}: {exempt.sum()} of {g['num']} draws within rounding of a CDF entry")
    assert exempt.sum() <= 0.001 * g["num"]
    fi = _host(g["dev"].face_index)
    differ = fi != g["fi"]
    print(f"{mesh}: {differ.sum()} face indices differ from the host's")
    assert not np.any(differ & ~exempt)
    same = ~differ
    assert np.array_equal(_host(g["dev"].points64)[same], g["pts"][same])
    assert np.array_equal(_host(g["dev"].points)[same], g["pts"].astype(np.float32)[same])


@pytest.mark.parametrize("mesh", ["blob", "soup"])
def test_normals_and_vertex_colours_equal_the_host_s_bit_for_bit(general, mesh):
    from motion324_amd import preprocess
    g = general[mesh]
    same = _host(g["dev"].face_index) == g["fi"]
    _, normals, colors = g["host"]
    assert np.array_equal(_host(g["dev"].normals)[same], normals[same])
    assert np.array_equal(_host(g["dev"].colors)[same], colors[same])
    # a face without area repeats its predecessor's CDF entry, so no draw lands on one unless it is the clamped last face: the
    # zero normal of such a face is checked on the mesh without area above; here every sampled face has a unit normal
    flat = sc.model_cross(g["v"], g["f"])[1][g["fi"]] == 0
    assert np.all(_host(g["dev"].normals)[flat & same] == 0)
    assert np.allclose(np.linalg.norm(_host(g["dev"].normals).astype(np.float64), axis=1)[~flat & same], 1.0, atol=1e-6)
    # the public wrapper returns the same three tensors
    pts, nrm, rgb = preprocess.sample_pointcloud_with_albedo(g["v"], g["f"], g["num"], g["colors"], 5, device="cuda")
    assert torch.equal(pts, g["dev"].points) and torch.equal(nrm, g["dev"].normals) and torch.equal(rgb, g["dev"].colors)


# ------------------------------------------------------------------------------------------------ 4. texture
def test_texture_colours_equal_the_reference_s():
    from motion324_amd import preprocess
    g = load_golden("sampler_tex")
    v, f, uv, tex, num, seed = g["in_vertices"], g["in_faces"], g["in_uv"], g["in_texture"], int(g["num"]), int(g["seed"])
    assert tex.shape == (48, 64, 3) and num == 3000 and (uv.min() < 0 and uv.max() > 1)
    pts, nrm, rgb = preprocess.sample_pointcloud_with_albedo(v, f, num, None, seed, uv=uv, texture=tex, device="cuda")
    assert np.array_equal(_host(pts), g["out_points"]) and np.array_equal(_host(nrm), g["out_normals"])
    _, fi = preprocess.sample_surface(v, f, num, seed)
    x, y, col, row = sc.texel_coordinates(v, f, uv, fi, num, seed, tex.shape[0], tex.shape[1])
    exempt = sc.near_texel_border(x, y)
    print(f"texture: {exempt.sum()} of {num} samples within 1e-9 of a texel border")
    assert exempt.sum() <= 0.001 * num
    got = _host(rgb)
    assert got.dtype == np.float32 and np.array_equal(got[~exempt], g["out_colors"][~exempt])
    # the order of preference: vertex colours beat the texture, no source at all is grey
    colors = sc.blob()[2]
    with_vc = preprocess.sample_pointcloud_with_albedo(v, f, num, colors, seed, uv=uv, texture=tex, device="cuda")[2]
    assert np.array_equal(_host(with_vc), preprocess.sample_pointcloud_with_albedo(v, f, num, colors, seed)[2])
    grey = preprocess.sample_pointcloud_with_albedo(v, f, num, None, seed, device="cuda")[2]
    assert bool((grey == 0.5).all())
    # a texture with an alpha channel decodes to [H,W,4]: the first three channels are read
    rgba = np.concatenate([tex, np.full(tex.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)
    assert torch.equal(preprocess.sample_pointcloud_with_albedo(v, f, num, None, seed, uv=uv, texture=rgba, device="cuda")[2], rgb)


def test_texture_on_a_face_without_area_uses_equal_weights():
    from motion324_amd import ops
    v, f = sc.grid_mesh(4, 4)
    f = f.copy()
    f[:, 2] = f[:, 1]                                            # every face flat: all samples on the last one
    uv = np.zeros((len(v), 2))
    uv[f[-1]] = [[0.2, 0.3], [0.8, 0.6], [0.8, 0.6]]
    tex = (np.arange(8 * 10 * 3) % 251).astype(np.uint8).reshape(8, 10, 3)
    s = _draw(v, f, 64, 3, want_colors=True, uv=_dev(uv), texture=_dev(tex))
    su = (1 / 3 * 0.2 + 1 / 3 * 0.8) + 1 / 3 * 0.8
    sv = (1 / 3 * 0.3 + 1 / 3 * 0.6) + 1 / 3 * 0.6
    want = tex[int((1 - sv) * 8), int(su * 10)].astype(np.float32) / np.float32(255)
    assert np.all(_host(s.face_index) == len(f) - 1) and np.all(_host(s.colors) == want)


# ------------------------------------------------------------------------------------------------ 5. callers
def test_prepare_mesh_data_with_the_device_sampler_equals_the_host_path():
    from motion324_amd.preprocess import prepare_mesh_data
    g = load_golden("prestep")
    mesh = {"vertices": g["in_vertices"], "faces": g["in_faces"], "vertex_normals": g["in_vertex_normals"], "vertex_colors": g["in_vertex_colors"]}
    cfg = {"training": {"num_shape_samples": int(g["num_shape_samples"])}}
    host, host_v, host_f = prepare_mesh_data(cfg, mesh, "cuda", seed=int(g["seed"]))
    again, _, _ = prepare_mesh_data(cfg, mesh, "cuda", seed=int(g["seed"]), sampler="host")
    dev, dev_v, dev_f = prepare_mesh_data(cfg, mesh, "cuda", seed=int(g["seed"]), sampler="device")
    assert set(dev) == set(host) == set(again)
    for k in host:
        assert dev[k].is_cuda and dev[k].dtype == host[k].dtype and dev[k].shape == host[k].shape, k
        assert torch.equal(dev[k], host[k]) and torch.equal(again[k], host[k]), k
    assert np.array_equal(dev_v, host_v) and np.array_equal(dev_f, host_f)
    # a textured mesh: the dict carries uv and texture, the colours are the reference's
    t = load_golden("sampler_tex")
    tmesh = {"vertices": t["in_vertices"], "faces": t["in_faces"], "vertex_normals": g["in_vertex_normals"], "uv": t["in_uv"], "texture": t["in_texture"]}
    with pytest.raises(Exception, match="sampler"):
        prepare_mesh_data(cfg, tmesh, "cuda", sampler="gpu")
    textured, _, _ = prepare_mesh_data({"training": {"num_shape_samples": 500}}, tmesh, "cuda", seed=3, sampler="device")
    assert tuple(textured["ref_shape_rgbs"].shape) == (1, 500, 3) and not bool((textured["ref_shape_rgbs"] == 0.5).all())


@pytest.fixture(scope="module")
def sequence():
    """three frames of the blob, deforming, and a prediction of it: rotated a little, shifted, scaled, on the reversed face list"""
    v, f, _ = sc.blob()
    gt = np.stack([v * (1.0 + 0.06 * k * np.sin(2.0 * v[:, :1] + 0.4 * k)) for k in range(3)])
    c, s = np.cos(0.04), np.sin(0.04)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    pred = 1.4 * (gt @ R.T) + np.array([0.3, -0.2, 0.1])
    return gt.astype(np.float32), f, pred.astype(np.float32), f[::-1].copy()


def test_evaluate_sequence_with_the_device_sampler_returns_the_host_s_results(sequence):
    from motion324_amd import evaluation as ev
    gt, gt_faces, pred, pred_faces = sequence
    num = 2048
    host = ev.evaluate_sequence(gt, gt_faces, pred, pred_faces, num_samples=num, seed=3, sampler="host")
    # on the host first: no draw of either side lies within rounding of a CDF entry, so the two samplers must agree entirely
    _, gc, gs = ev.normalize_points(gt[0])
    _, pc, ps = ev.normalize_points(pred[0])
    for k in range(3):
        ga = ev.apply_icp_alignment(ev.apply_normalization(gt[k], gc, gs), host["R"], host["t"], host["s"])
        assert not sc.near_cdf_entry(ga, gt_faces, num, ev.sample_seed(3, 0, k)).any(), k
        assert not sc.near_cdf_entry(ev.apply_normalization(pred[k], pc, ps), pred_faces, num, ev.sample_seed(3, 1, k)).any(), k
    dev = ev.evaluate_sequence(gt, gt_faces, pred, pred_faces, num_samples=num, seed=3, sampler="device")
    print("host", host["chamfer_distances"], host["fscores"], "device", dev["chamfer_distances"], dev["fscores"])
    assert dev["chamfer_distances"] == host["chamfer_distances"] and dev["fscores"] == host["fscores"]
    assert np.array_equal(dev["R"], host["R"]) and np.array_equal(dev["t"], host["t"]) and dev["s"] == host["s"]
    assert len(dev["chamfer_distances"]) == 3 and all(np.isfinite(dev["chamfer_distances"]))


def test_cli_accepts_the_device_sampler_and_writes_the_same_files(sequence, tmp_path, capsys):
    from motion324_amd import evaluation as ev
    gt, gt_faces, pred, pred_faces = sequence
    results = {}
    for sampler in ("host", "device"):
        for name, verts, faces in (("gt_case", gt, gt_faces), ("pred_case", pred, pred_faces)):
            (tmp_path / sampler / name).mkdir(parents=True)
            np.save(tmp_path / sampler / name / "faces.npy", faces)
            for k in range(len(verts)):
                np.save(tmp_path / sampler / name / f"frame_{k:04d}.npy", verts[k])
        results[sampler] = ev.main(["--gt_path", str(tmp_path / sampler / "gt_case"), "--pred_path", str(tmp_path / sampler / "pred_case"),
                                    "--num_samples", "1024", "--seed", "3", "--sampler", sampler])
    assert "Frame 2 - Chamfer:" in capsys.readouterr().out
    assert results["device"]["chamfer_distances"] == results["host"]["chamfer_distances"]
    text = {s: open(tmp_path / s / "gt_case" / "evaluation_results.txt").read() for s in results}
    assert text["device"] == text["host"] and text["host"].startswith("gt_case\ncd_mean_")
    a, b = (np.load(tmp_path / s / "gt_case" / "icp_alignment_params.npz") for s in ("host", "device"))
    assert all(np.array_equal(a[k], b[k]) for k in ("R", "t", "s"))
