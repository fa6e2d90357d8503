"""The tests of the tests of tests/test_frontend_gpu.py (no GPU needed).  For every gate the GPU tests apply to the small kernels
around the transformer:
  soundness -- the fp32 emulation of the kernel's arithmetic (tests/frontend_cases.py) passes the gate on the GPU tests' inputs;
  power     -- an index mistake of the kind the kernel can make, planted in the emulation, fails the same gate."""
import numpy as np
import pytest
import torch

import error_bounds as eb
import frontend_cases as fc

F32, BF = torch.float32, torch.bfloat16
DT = [F32, BF]


def _fails(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


# ------------------------------------------------------------------------------------------- patchify
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", fc.PATCHIFY_CASES, ids=fc.patchify_id)
def test_patchify_emulation_is_inside_the_bound(case, dtype):
    (Fr, Hin, Win), (size, patch), Kp = case
    video, video8 = fc.patchify_frames(Fr, Hin, Win)
    n = 3 * patch * patch
    for frames in (video, video8):
        as_float = frames if frames.dtype == F32 else frames.float() / 255
        ref = fc.patchify_reference(as_float, size, patch)
        out = fc.patchify_emulation(frames, size, patch, Kp, dtype).float()
        assert out.shape == ((size // patch) ** 2 * Fr, Kp)
        eb.assert_within(out[:, :n], ref, eb.patchify(ref, max(Hin, Win), dtype), "patch rows")
        assert torch.equal(out, fc.patchify_emulation(as_float, size, patch, Kp, dtype).float())


def test_patchify_case_table_covers_what_it_claims():
    pairs, frames = {}, {}
    for shape, sp, Kp in fc.PATCHIFY_CASES:
        pairs.setdefault(sp, set()).add(Kp)
        frames.setdefault(shape, set()).add(sp)
    assert set(frames) == {(2, 48, 80), (1, 300, 200), (3, 1, 7), (1, 224, 224), (2, 40, 333)}
    assert all(len(v) >= 2 for v in frames.values())
    assert set(pairs) == {(224, 14), (42, 14), (28, 14)}
    assert all(v == {3 * p * p, 640} for (_, p), v in pairs.items())


@pytest.mark.parametrize("dtype", DT)
def test_patchify_gate_catches_swapped_axes(dtype):
    for case in fc.PATCHIFY_CASES:
        (Fr, Hin, Win), (size, patch), Kp = case
        if Hin == Win:
            continue
        video, _ = fc.patchify_frames(Fr, Hin, Win)
        ref = fc.patchify_reference(video, size, patch)
        out = fc.patchify_emulation(video, size, patch, Kp, dtype, fault="swap_hw").float()
        _fails(eb.assert_within, out[:, :3 * patch * patch], ref, eb.patchify(ref, max(Hin, Win), dtype), fc.patchify_id(case))


# ------------------------------------------------------------------------------------------- point features
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("P", fc.POINT_COUNTS)
def test_point_encode_emulation_is_inside_the_bound(P, dtype):
    xyz = fc.point_coordinates(P)
    proj, ref = fc.point_encode_reference(xyz)
    out = fc.point_encode_emulation(xyz, dtype).float()
    eb.assert_within(out[:, :51], ref, eb.point_encode(proj, ref, dtype), "point features")
    assert out[0].tolist() == fc.ZERO_POINT_ROW
    moved = out.clone()
    moved[P - 1, 48:51] = out[0, 48:51] if P > 1 else 0.25                            # the last point holds another point's xyz
    _fails(eb.assert_within, moved[:, :51], ref, eb.point_encode(proj, ref, dtype), "point features")


def test_point_coordinates_hold_the_edge_values():
    xyz = fc.point_coordinates(333)
    for v in (0.0, 0.5, -0.5, fc.TINY, -fc.TINY):
        assert bool((xyz == v).any()), v
    assert float(xyz.abs().max()) <= 0.5 and bool((xyz[0] == 0).all())


# ------------------------------------------------------------------------------------------- token assembly
@pytest.mark.parametrize("mode", fc.ASSEMBLE_MODES)
@pytest.mark.parametrize("shape", fc.ASSEMBLE_CASES)
def test_assemble_emulation_is_inside_a_quarter_of_the_row_gate(shape, mode):
    inp = fc.assemble_inputs(*shape)
    for lw in ((True,) if mode == "normalised" else (False,) if mode == "raw" else (False, True)):
        kw = dict(drop=mode == "dropout", lw=lw)
        err = fc.row_rel_err(fc.assemble_emulation(inp, *shape, **kw), fc.assemble_reference(inp, *shape, **kw))
        assert float(err.max()) <= 2.5e-7, (shape, mode, lw, float(err.max()))


@pytest.mark.parametrize("shape", fc.ASSEMBLE_CASES)
def test_assemble_row_gate_catches_an_unwritten_row_and_the_wrong_special_rows(shape):
    B, T, K, P, C = shape
    inp = fc.assemble_inputs(*shape)
    rows = B * T * (4 + K + P)
    for lw in (True, False):
        ref = fc.assemble_reference(inp, *shape, lw=lw)
        err = fc.row_rel_err(fc.assemble_emulation(inp, *shape, lw=lw, fault="last_row_unwritten"), ref)
        assert float(err[-1]) > fc.ASSEMBLE_GATE and float(err[:-1].max()) < fc.ASSEMBLE_GATE
        err = fc.row_rel_err(fc.assemble_emulation(inp, *shape, lw=lw, fault="spr_in_frame0"), ref)
        hit = (err > fc.ASSEMBLE_GATE).nonzero()[:, 0].tolist()
        assert hit == [b * T * (4 + K + P) + j for b in range(B) for j in range(4)], hit
    # a workgroup owns 4 rows: 21 and 18 rows end in a partial one; C = 1024 is the limit, T = 1 has no spr rows
    assert rows % 4 == {768: 1, 1024: 0, 196: 2, 192: 0}[C]


def test_one_wrong_row_hides_in_the_norm_over_the_whole_output():
    """why the gate is per row: at (2, 3, 8, 16, 192) a last row that is off by 1e-5 of its norm passes rel_err < 1e-6"""
    from conftest import rel_err
    shape = (2, 3, 8, 16, 192)
    inp = fc.assemble_inputs(*shape)
    ref = fc.assemble_reference(inp, *shape)
    out = fc.assemble_emulation(inp, *shape).double()
    out[-1] += 1e-5 * ref[-1].flip(0)
    assert rel_err(out, ref) < fc.ASSEMBLE_GATE < float(fc.row_rel_err(out, ref).max())


# ------------------------------------------------------------------------------------------- 3-wide head
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("M,K", fc.LINEAR_N3_CASES)
def test_linear_n3_emulation_is_inside_the_bound(M, K, dtype):
    a, w, bias = fc.linear_n3_inputs(M, K, dtype)
    ref, bound = fc.linear_n3_reference(a, w, bias), eb.linear_n3(a, w, bias)
    worst = eb.assert_within(fc.linear_n3_emulation(a, w, bias), ref, bound, "linear_n3")
    assert worst <= 0.3, worst
    unwritten = fc.linear_n3_emulation(a, w, bias)
    unwritten[M - 1, 2] = float("nan")                                                 # the NaN fill left in the last value
    _fails(eb.assert_within, unwritten, ref, bound, "linear_n3")


@pytest.mark.parametrize("M,K", [c for c in fc.LINEAR_N3_CASES if c[1] >= 64])
def test_linear_n3_bound_catches_a_dropped_step(M, K):
    a, w, bias = fc.linear_n3_inputs(M, K, F32)
    ref, bound = fc.linear_n3_reference(a, w, bias), eb.linear_n3(a, w, bias)
    _fails(eb.assert_within, fc.linear_n3_emulation(a, w, bias, fault="drop_step"), ref, bound, "linear_n3")


# ------------------------------------------------------------------------------------------- trajectory filters
def _oracle():
    from oracle import ref_smooth
    return ref_smooth


@pytest.mark.parametrize("shape", fc.TRAJ_SHAPES)
def test_no_random_displacement_lies_near_the_threshold(shape):
    x, planted = fc.trajectories(*shape)
    d = fc.random_displacement_norms(x, planted)
    assert not bool(((d > fc.THR / 2) & (d < 2 * fc.THR)).any())
    if d.size > 100:
        assert 0.1 < float((d < fc.THR).mean()) < 0.9                                  # both outcomes are common
    if shape[0] > 1:
        assert not np.array_equal(x[0], x[1])
    assert planted == (shape[1] >= 8)


@pytest.mark.parametrize("shape", fc.TRAJ_SHAPES)
def test_threshold_emulation_equals_the_oracle_and_the_planted_outcomes(shape):
    x, planted = fc.trajectories(*shape)
    want = _oracle().smooth_trajectories(x, fc.THR, 0.0)
    got = fc.threshold_emulation(x, fc.THR)
    assert np.array_equal(got, want)
    if planted:
        assert np.array_equal(got[0, :, :fc.PLANTED_N], fc.planted_outcome(x))
        le = fc.threshold_emulation(x, fc.THR, fault="le")
        assert not np.array_equal(le, want)
        assert not np.array_equal(le[0, :, 0], fc.planted_outcome(x)[:, 0])           # `<=` holds the point that sits on the threshold
        assert np.array_equal(le[0, :, 1:fc.PLANTED_N], fc.planted_outcome(x)[:, 1:])
    if shape[0] > 1:
        assert not np.array_equal(fc.threshold_emulation(x, fc.THR, fault="batch_stride0"), want)


@pytest.mark.parametrize("sigma", fc.SIGMAS)
@pytest.mark.parametrize("shape", fc.TRAJ_SHAPES)
def test_gaussian_emulation_is_inside_the_gate(shape, sigma):
    x, _ = fc.trajectories(*shape)
    T = shape[1]
    for thr in (-1.0, fc.THR):
        want = _oracle().smooth_trajectories(x, thr, sigma)
        got = fc.smooth_emulation(x, thr, sigma)
        assert np.abs(got - want).max() < fc.SMOOTH_GATE
        if sigma == 0.1:
            assert np.array_equal(got, fc.threshold_emulation(x, thr))
        elif T > 1:
            assert not np.abs(fc.smooth_emulation(x, thr, sigma, fault="wrap") - want).max() < fc.SMOOTH_GATE
        if shape[0] > 1:
            assert not np.abs(fc.smooth_emulation(x, thr, sigma, fault="batch_stride0") - want).max() < fc.SMOOTH_GATE


def _savgol_input(T):
    x, _ = fc.trajectories(*next(s for s in fc.TRAJ_SHAPES if s[1] >= T and (T > 2 or s[1] == 2)))
    return np.ascontiguousarray(x[:, :T])


@pytest.mark.parametrize("window,polyorder,T", fc.SAVGOL_CASES)
def test_savgol_emulation_is_inside_the_gate(window, polyorder, T):
    x = _savgol_input(T)
    assert x.shape[1] == T
    want = _oracle().savgol(x, window, polyorder)
    got = fc.savgol_emulation(x, window, polyorder)
    assert np.abs(got - want).max() < fc.SMOOTH_GATE
    if T == 2:
        assert np.array_equal(got, x)
    elif x.shape[0] > 1:
        assert not np.abs(fc.savgol_emulation(x, window, polyorder, fault="batch_stride0") - want).max() < fc.SMOOTH_GATE


@pytest.mark.parametrize("mincutoff,beta", fc.ONEEURO_PARAMS)
@pytest.mark.parametrize("shape", fc.TRAJ_SHAPES)
def test_oneeuro_emulation_is_inside_the_gate(shape, mincutoff, beta):
    x, _ = fc.trajectories(*shape)
    want = _oracle().oneeuro(x, mincutoff, beta)
    got = fc.oneeuro_emulation(x, mincutoff, beta)
    assert np.abs(got - want).max() < fc.SMOOTH_GATE
    if shape[1] == 1:
        assert np.array_equal(got, x)
    if shape[0] > 1:
        assert not np.abs(fc.oneeuro_emulation(x, mincutoff, beta, fault="batch_stride0") - want).max() < fc.SMOOTH_GATE


# ------------------------------------------------------------------------------------------- nearest point
@pytest.mark.parametrize("nq,nr", fc.NEAREST_CASES)
def test_nearest_emulation_passes_the_gate_and_picks_the_fp64_nearest(nq, nr):
    q, r = fc.nearest_inputs(nq, nr)
    d2 = fc.squared_distances(q, r)
    got = fc.nearest_emulation(q, r)
    fc.nearest_gate(got, d2, "emulation")
    assert torch.equal(got, d2.argmin(dim=1))
    if nr > 1:
        assert int(got[-1]) == nr - 1                                                  # the planted pair: last lane, last point
    if nr > 1:                                                                         # every such nr has a partial last tile
        assert nr % 1024
        _fails(fc.nearest_gate, fc.nearest_emulation(q, r, fault="skip_partial_tile"), d2, "skipped tile")
    _fails(fc.nearest_gate, torch.full((nq,), nr), d2, "index out of range")


def test_nearest_ties_go_to_the_lowest_index_in_the_emulation():
    q, r = fc.nearest_tie_inputs()
    assert r.shape[0] == 2 * fc.TIE_BASE and torch.equal(r[:fc.TIE_BASE].sort(0).values, r[fc.TIE_BASE:].sort(0).values)
    got = fc.nearest_emulation(q, r)
    fc.nearest_gate(got, fc.squared_distances(q, r), "ties")
    assert int(got.max()) < fc.TIE_BASE
    assert got[:len(fc.TIE_EXACT)].tolist() == fc.TIE_EXACT
    # every copy lies in another LDS tile than its original; the exact queries' points stand on both sides of 1024
    copies = [int((r[fc.TIE_BASE:] == r[i]).all(1).nonzero()[0, 0]) + fc.TIE_BASE for i in range(fc.TIE_BASE)]
    assert all(c // 1024 != i // 1024 for i, c in enumerate(copies))
    assert min(fc.TIE_EXACT) < 1024 <= max(fc.TIE_EXACT) < fc.TIE_BASE
