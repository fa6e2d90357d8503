"""The small kernels around the transformer at ragged and edge shapes (motion324_amd/csrc/elementwise.hip: patchify / patchify_u8,
point_encode, point_concat, dino_cls_rows, assemble_tokens, linear_n3, the four trajectory filters, nearest_point), run through
motion324_amd.ops and motion324_amd.postprocess and held to the gates tests/test_frontend_cpu.py proves sound and sharp.
Cases, references and emulations: tests/frontend_cases.py; bounds: tests/error_bounds.py, derivations in tests/ERROR_BOUNDS.md
("The kernels around the transformer").  `pytest -s` prints the worst err / bound of every case (a record, the gate is 1.0)."""
import numpy as np
import pytest
import torch

import error_bounds as eb
import frontend_cases as fc

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
DT = [F32, BF]


def _ops():
    from motion324_amd import ops
    return ops


def _smooth(x, **kw):
    from motion324_amd.postprocess import smooth_trajectories
    out = smooth_trajectories(torch.from_numpy(x).to(DEV), **kw)
    assert out.shape == x.shape and out.dtype == torch.float32
    return out.cpu().numpy()


def _record(what, worst):
    print(f"\nRECORD {what}: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------- patchify
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", fc.PATCHIFY_CASES, ids=fc.patchify_id)
def test_patchify_ragged_frames(case, dtype):
    ops = _ops()
    (Fr, Hin, Win), (size, patch), Kp = case
    n = 3 * patch * patch
    video, video8 = fc.patchify_frames(Fr, Hin, Win)
    out = ops.patchify(video.to(DEV), size, patch, Kp, dtype)
    assert out.shape == (Fr * (size // patch) ** 2, Kp) and out.dtype == dtype
    out = out.float().cpu()
    ref = fc.patchify_reference(video, size, patch)
    worst = eb.assert_within(out[:, :n], ref, eb.patchify(ref, max(Hin, Win), dtype), "patch rows")
    assert out[:, n:].numel() == (Kp - n) * out.shape[0] and not bool(out[:, n:].any())          # padding columns: exact zeros
    # byte frames: bit for bit the fp32 path on video.float() / 255, and inside the same bound against fp64
    as_float = video8.float() / 255
    out8 = ops.patchify(video8.to(DEV), size, patch, Kp, dtype)
    assert torch.equal(out8, ops.patchify(as_float.to(DEV), size, patch, Kp, dtype))
    ref8 = fc.patchify_reference(as_float, size, patch)
    out8 = out8.float().cpu()
    worst8 = eb.assert_within(out8[:, :n], ref8, eb.patchify(ref8, max(Hin, Win), dtype), "patch rows of byte frames")
    assert not bool(out8[:, n:].any())
    _record(f"patchify {fc.patchify_id(case)} {dtype}", max(worst, worst8))


# ------------------------------------------------------------------------------------------- point features
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("P", fc.POINT_COUNTS)
def test_point_encode_edge_coordinates(P, dtype):
    xyz = fc.point_coordinates(P)
    enc = _ops().point_encode(xyz.to(DEV), dtype)
    assert enc.shape == (P, 64) and enc.dtype == dtype
    enc = enc.float().cpu()
    proj, ref = fc.point_encode_reference(xyz)
    worst = eb.assert_within(enc[:, :51], ref, eb.point_encode(proj, ref, dtype), "point features")
    assert not bool(enc[:, 51:].any())
    assert enc[0].tolist() == fc.ZERO_POINT_ROW                                       # xyz = 0: 0 | 1 | 0, exactly
    _record(f"point_encode P={P} {dtype}", worst)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C,Kp,P", fc.POINT_CONCAT_CASES)
def test_point_concat_widths(C, Kp, P, dtype):
    nrm, rgb = fc.point_concat_inputs(C, Kp, P)
    feat = torch.full((P, Kp), 7.0, dtype=dtype, device=DEV)
    _ops().point_concat(nrm.to(DEV), rgb.to(DEV), feat, C)
    f = feat.float().cpu()
    assert bool((f[:, :C] == 7.0).all())                                              # the columns in front are not this kernel's
    six = torch.cat([nrm, rgb], dim=1)
    if dtype == F32:
        assert torch.equal(f[:, C:C + 6], six)
    else:
        assert bool(((f[:, C:C + 6].double() - six.double()).abs() <= 1.01 * eb.U16 * six.double().abs()).all())
    assert f[:, C + 6:].shape[1] == Kp - C - 6 and not bool(f[:, C + 6:].any())


@pytest.mark.parametrize("Fr,rpf,C", fc.DINO_CLS_CASES)
def test_dino_cls_rows_touch_nothing_else(Fr, rpf, C):
    cls, pos0 = fc.cls_inputs(C)
    x = torch.full((Fr * rpf, C), fc.SENTINEL, device=DEV)
    _ops().dino_cls_rows(cls.to(DEV), pos0.to(DEV), x, Fr, rpf)
    want = torch.full((Fr, rpf, C), fc.SENTINEL)
    want[:, 0] = cls + pos0                                                           # one fp32 addition: exact
    assert torch.equal(x.cpu().view(torch.int32), want.reshape(-1, C).view(torch.int32))


# ------------------------------------------------------------------------------------------- token assembly
@pytest.mark.parametrize("mode", fc.ASSEMBLE_MODES)
@pytest.mark.parametrize("shape", fc.ASSEMBLE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_assemble_tokens_row_by_row(shape, mode):
    ops = _ops()
    B, T, K, P, C = shape
    Lt = 4 + K + P
    inp = fc.assemble_inputs(*shape)
    d = {k: v.to(DEV) for k, v in inp.items()}
    drop = (fc.DROP_P, fc.DROP_SEED) if mode == "dropout" else ()

    def run(lw):
        out = ops.assemble_tokens(d["dino_x"], d["dw"], d["db"], fc.EPS_DINO, d["pos"], d["sp0"], d["spr"], d["mesh"],
                                  d["lw"] if lw else None, fc.EPS_IN, B, T, K, P, *drop)
        assert out.shape == (B * T * Lt, C)
        err = fc.row_rel_err(out, fc.assemble_reference(inp, *shape, drop=bool(drop), lw=lw))
        assert float(err.max()) < fc.ASSEMBLE_GATE, (lw, [(int(i), float(err[i])) for i in (err >= fc.ASSEMBLE_GATE).nonzero()[:8, 0]])
        print(f"\nRECORD assemble_tokens {shape} {mode} ln_w={lw}: worst row error {float(err.max()):.3g}")
        return out.cpu().reshape(B, T, Lt, C)

    if mode in ("normalised", "dropout"):
        run(True)
    if mode in ("raw", "dropout"):
        pre = run(False)
        # the rows that are copies: frame 0 takes sp0, every later frame spr, every frame of batch item b that item's mesh rows
        assert torch.equal(pre[:, 0, :4], inp["sp0"].expand(B, -1, -1))
        assert torch.equal(pre[:, 1:, :4], inp["spr"].expand(B, T - 1, -1, -1))
        assert torch.equal(pre[:, :, 4:4 + K], inp["mesh"].reshape(B, 1, K, C).expand(-1, T, -1, -1))
        if mode == "dropout":
            assert torch.equal(pre[:, :, 4 + K:] == 0, ~fc.dropout_keep(B, T, P, C))   # the mask itself is bit-exact
        else:
            assert not bool((pre == 0).any())


# ------------------------------------------------------------------------------------------- 3-wide head
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M,K", fc.LINEAR_N3_CASES)
def test_linear_n3_idle_lanes_and_long_rows(M, K, dtype):
    a, w, bias = fc.linear_n3_inputs(M, K, dtype)
    out = torch.full((M, 3), float("nan"), dtype=F32, device=DEV)
    _ops().linear_n3(a.to(dtype).to(DEV), w.to(DEV), bias.to(DEV), out)
    worst = eb.assert_within(out, fc.linear_n3_reference(a, w, bias), eb.linear_n3(a, w, bias), "linear_n3")
    _record(f"linear_n3 M={M} K={K} {dtype}", worst)


# ------------------------------------------------------------------------------------------- trajectory filters
def _ref_smooth():
    from oracle import ref_smooth
    return ref_smooth


@pytest.mark.parametrize("shape", fc.TRAJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_threshold_pass_is_exact_and_strict(shape):
    x, planted = fc.trajectories(*shape)
    got = _smooth(x, method="threshold", motion_threshold=fc.THR)
    assert np.array_equal(got, _ref_smooth().smooth_trajectories(x, fc.THR, 0.0))
    if planted:
        want = fc.planted_outcome(x)
        assert np.array_equal(got[0, :, 0], x[0, :, 0])          # a step of exactly the threshold moves the point: `<` is strict
        assert np.array_equal(got[0, :, 1], np.broadcast_to(x[0, 0, 1], want[:, 1].shape))        # half a threshold: held for good
        assert np.array_equal(got[0, :6, 2], np.broadcast_to(x[0, 0, 2], (6, 3)))                 # five half steps: still at frame 0
        assert np.array_equal(got[0, 6:, 2], x[0, 6:, 2])                                         # then the true position
        assert np.array_equal(got[0, :, :fc.PLANTED_N], want)


@pytest.mark.parametrize("sigma", fc.SIGMAS)
@pytest.mark.parametrize("shape", fc.TRAJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gaussian_and_combined_filters(shape, sigma):
    x, _ = fc.trajectories(*shape)
    for method, thr in (("gaussian", -1.0), ("combined", fc.THR)):
        got = _smooth(x, method=method, motion_threshold=fc.THR, sigma=sigma)
        err = float(np.abs(got - _ref_smooth().smooth_trajectories(x, thr, sigma)).max())
        print(f"\nRECORD {method} {shape} sigma={sigma}: max error {err:.3g}")
        assert err < fc.SMOOTH_GATE
        if sigma == 0.1:                                         # radius 0: one tap of weight 1, the threshold pass comes through as it is
            assert np.array_equal(got, x if thr < 0 else _smooth(x, method="threshold", motion_threshold=fc.THR))


@pytest.mark.parametrize("window,polyorder,T", fc.SAVGOL_CASES)
def test_savgol_window_against_clip_length(window, polyorder, T):
    shape = next(s for s in fc.TRAJ_SHAPES if s[1] >= T and (T > 2 or s[1] == 2))
    x = np.ascontiguousarray(fc.trajectories(*shape)[0][:, :T])
    got = _smooth(x, method="savgol", window_size=window, savgol_polyorder=polyorder)
    err = float(np.abs(got - _ref_smooth().savgol(x, window, polyorder)).max())
    print(f"\nRECORD savgol ({window}, {polyorder}) on {x.shape[:3]}: max error {err:.3g}")
    assert err < fc.SMOOTH_GATE
    if T == 2:
        assert np.array_equal(got, x)                            # shorter than the window: a copy


@pytest.mark.parametrize("mincutoff,beta", fc.ONEEURO_PARAMS)
@pytest.mark.parametrize("shape", fc.TRAJ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oneeuro_short_clips_and_many_points(shape, mincutoff, beta):
    x, _ = fc.trajectories(*shape)
    got = _smooth(x, method="oneeuro", oneeuro_mincutoff=mincutoff, oneeuro_beta=beta)
    err = float(np.abs(got - _ref_smooth().oneeuro(x, mincutoff, beta)).max())
    print(f"\nRECORD oneeuro {shape} ({mincutoff}, {beta}): max error {err:.3g}")
    assert err < fc.SMOOTH_GATE
    assert np.array_equal(got[:, 0], x[:, 0])                    # T = 1: the whole output


# ------------------------------------------------------------------------------------------- nearest point
@pytest.mark.parametrize("nq,nr", fc.NEAREST_CASES)
def test_nearest_point_partial_tiles_and_workgroups(nq, nr):
    q, r = fc.nearest_inputs(nq, nr)
    got = _ops().nearest_point(q.to(DEV), r.to(DEV))
    assert got.dtype == torch.int64
    worst = fc.nearest_gate(got, fc.squared_distances(q, r), f"nearest_point {nq} x {nr}")
    print(f"\nRECORD nearest_point {nq} x {nr}: largest chosen d2 / min d2 - 1 = {worst:.3g}")
    if nr > 1:
        assert int(got[-1]) == nr - 1                            # the last lane of the last workgroup, the last point of the last tile


def test_nearest_point_lowest_index_wins_ties():
    q, r = fc.nearest_tie_inputs()
    got = _ops().nearest_point(q.to(DEV), r.to(DEV)).cpu()
    fc.nearest_gate(got, fc.squared_distances(q, r), "nearest_point ties")
    assert int(got.max()) < fc.TIE_BASE                          # every point's copy stands behind it, in another LDS tile
    assert got[:len(fc.TIE_EXACT)].tolist() == fc.TIE_EXACT
