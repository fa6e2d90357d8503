"""The geometry evaluation kernels (csrc/geometry.hip) past their first work item: query tiles, reference slices and batch items
together, later passes of the grid-stride loops of m324_dist_stats and m324_icp_moments, and the host path on top at sizes that
span several tiles -- each against an fp64 reference of the same operation on the same fp32 numbers.  Shapes, inputs and references:
tests/geometry_cases.py (held against the kernel's constants by tests/test_eval_cpu.py); bounds: tests/ERROR_BOUNDS_GEOMETRY.md."""
import time

import numpy as np
import pytest
import torch

import geometry_cases as gc
from test_eval_gpu import GUARD, SENTINEL_F, _raw_search, _recovery_case

pytestmark = pytest.mark.gpu

SENTINEL_D, SENTINEL_L = -7.5, -12345


def _bits_equal(a, b):
    """bit equality of two float tensors (NaN equals NaN, +0 differs from -0)"""
    kind = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(kind), b.contiguous().view(kind))


def _check_against_fp64(q, r, dist, index, d1, what):
    """the rule of ERROR_BOUNDS_GEOMETRY.md on unit-cube data: the fp64 index or a point at most 1e-6 farther; distance within 1e-6"""
    got_d, got_i = dist.cpu().double(), index.cpu().long()
    n_ref = r.shape[-2]
    assert int(got_i.min()) >= 0 and int(got_i.max()) < n_ref, what
    farther = float((gc.chosen_distance(q, r, got_i) - d1).max())
    off = float((got_d - d1).abs().max())
    assert farther <= 1e-6, (what, farther)
    assert off <= 1e-6, (what, off)
    return off


# ------------------------------------------------------------------------------------------------ m324_nn_search: query tiles
@pytest.mark.parametrize("n_ref", gc.TILE_REFS)
@pytest.mark.parametrize("n_query", gc.TILE_QUERIES)
def test_nn_search_query_tiles_against_fp64(n_query, n_ref):
    """every query has a KNOWN nearest reference (a per-item permutation), so a query taken from another tile, register slot or
    batch item answers with another index; shared (stride 0) and per-item references"""
    from motion324_amd import ops
    worst = 0.0
    for batch in gc.TILE_BATCHES:
        for shared in (False, True):
            q, r, assign = gc.planted_search_case(17 * n_query + 3 * n_ref + batch, batch, n_query, n_ref, shared)
            d1, i1, d2 = gc.brute_force_nn(q, r)
            # from the reference alone: the planted neighbour is the nearest, and no second candidate within 1e-5 of it
            assert torch.equal(i1, assign), (batch, shared)
            assert n_ref == 1 or float((d2 - d1).min()) > 1e-5, (batch, shared, float((d2 - d1).min()))
            qd, rd = q.cuda(), r.cuda()
            dist, index = _raw_search(qd, rd)
            worst = max(worst, _check_against_fp64(q, r, dist, index, d1, (batch, shared)))
            bad = (index.cpu().long() != assign).nonzero()
            assert bad.numel() == 0, f"batch {batch} shared {shared}: {bad.shape[0]} queries miss their planted neighbour, first (item, query): {bad[:6].tolist()}"
            o_d, o_i = ops.nn_search(qd, rd, want_dist=True, want_index=True)
            assert _bits_equal(o_d, dist) and torch.equal(o_i, index)
            assert _bits_equal(ops.nn_search(qd, rd), dist)                      # the distance-only instantiation
            assert torch.equal(ops.nn_search(qd, rd, want_dist=False, want_index=True), index)
            one_d, one_i = _raw_search(qd, rd, 1)                                # the one-slice kernel writes the results itself
            assert _bits_equal(one_d, dist) and torch.equal(one_i, index), (batch, shared)
    print(f"nn_search tiles nq={n_query} nr={n_ref}: worst |d - d64| {worst:.3e} (bound 1e-6)")


# ------------------------------------------------------------------------------------------------ batch x tiles x slices
@pytest.fixture(scope="module")
def grid_case():
    """GRID's operands (uniform, so that winners are contested across chunks and slices), their fp64 answer and the one-slice run"""
    c = gc.GRID
    q, r = gc.unit_points(31, c.batch, c.n_query), gc.unit_points(32, c.batch, c.n_ref)
    d1 = gc.brute_force_nn(q, r)[0]
    dist, index = _raw_search(q.cuda(), r.cuda(), 1)
    return q, r, d1, dist, index


def test_nn_search_batch_tiles_and_slices_together(grid_case):
    from motion324_amd import ops
    c = gc.GRID
    q, r, d1, dist, index = grid_case
    qd, rd = q.cuda(), r.cuda()
    off = _check_against_fp64(q, r, dist, index, d1, "one slice")
    print(f"nn_search grid {tuple(c[:3])}: worst |d - d64| {off:.3e} (bound 1e-6)")
    automatic = ops.nn_plan(c.n_query, c.n_ref, c.batch, 0)[0]
    assert 1 < automatic <= c.n_ref // gc.MIN_SLICE, f"the automatic choice must slice this shape, got {automatic}"
    for forced, want in c.forced + ((0, automatic),):
        assert ops.nn_plan(c.n_query, c.n_ref, c.batch, forced)[0] == want
        d_s, i_s = _raw_search(qd, rd, forced)
        assert _bits_equal(d_s, dist), f"{want} slices: {int((d_s != dist).sum())} distances differ from the one-slice run"
        assert torch.equal(i_s, index), f"{want} slices: {int((i_s != index).sum())} indices differ from the one-slice run"
        # the distance-only and index-only instantiations through the same path
        assert _bits_equal(ops.nn_search(qd, rd, ref_slices=forced), dist), want
        assert torch.equal(ops.nn_search(qd, rd, want_dist=False, want_index=True, ref_slices=forced), index), want
        # every batch item equals its own call
        for b in range(c.batch):
            d_b, i_b = _raw_search(qd[b], rd[b], forced)
            assert _bits_equal(d_b[0], dist[b]) and torch.equal(i_b[0], index[b]), (want, b)


def test_nn_search_empty_trailing_slices():
    c = gc.EMPTY
    q, r = gc.unit_points(41, c.n_query), gc.unit_points(42, c.n_ref)
    d1 = gc.brute_force_nn(q[None], r)[0]
    one_d, one_i = _raw_search(q.cuda(), r.cuda(), 1)
    _check_against_fp64(q[None], r, one_d, one_i, d1, "one slice")
    for forced, want in c.forced + gc.CAPPED.forced:
        d_s, i_s = _raw_search(q.cuda(), r.cuda(), forced)
        assert _bits_equal(d_s, one_d) and torch.equal(i_s, one_i), forced
        assert int(i_s.min()) >= 0 and int(i_s.max()) < c.n_ref


def test_nn_search_ties_across_a_slice_and_a_chunk_boundary():
    from motion324_amd import ops
    q, r = gc.tie_case(51)
    d1 = gc.brute_force_nn(q[None], r)[0]
    qd, rd = q.cuda(), r.cuda()
    automatic = ops.nn_plan(gc.TIE_QUERIES, gc.GRID.n_ref, 1, 0)[0]
    assert automatic > 1
    first = None
    for forced in [f for f, _ in gc.GRID.forced] + [0]:
        slices = ops.nn_plan(gc.TIE_QUERIES, gc.GRID.n_ref, 1, forced)[0]
        ps = gc.per_slice(gc.GRID.n_ref, slices)
        assert slices == 1 or gc.TIE_LOW // ps != gc.TIE_HIGH // ps, "the planted pair shares a slice"
        dist, index = _raw_search(qd, rd, forced)
        for where, want_d in ((gc.TIE_QUERY_TILE0, 0.0), (gc.TIE_QUERY_TILE2, 0.25)):
            assert int(index[0, where]) == gc.TIE_LOW, f"{slices} slices, query {where}: index {int(index[0, where])}, the lower duplicate is {gc.TIE_LOW}"
            assert float(dist[0, where]) == want_d
        assert torch.equal(ops.nn_search(qd, rd, want_dist=False, want_index=True, ref_slices=forced), index[0])
        if first is None:
            first = (dist, index)
            _check_against_fp64(q[None], r, dist, index, d1, "one slice")
        assert _bits_equal(dist, first[0]) and torch.equal(index, first[1]), slices


@pytest.mark.parametrize("mode", ["offset_100", "scale_1000"])
def test_nn_search_away_from_the_origin(mode):
    """the relative form of the bound: distance within 8 * 2^-24 of the fp64 distance, the chosen point no farther than the fp64
    minimum by that factor (ERROR_BOUNDS_GEOMETRY.md)"""
    c = gc.GRID
    q, r = gc.unit_points(61, c.batch, c.n_query), gc.unit_points(62, c.batch, c.n_ref)
    q, r = (q + 100.0, r + 100.0) if mode == "offset_100" else (q * 1000.0, r * 1000.0)      # rounded to fp32: the inputs of both sides
    d1 = gc.brute_force_nn(q, r)[0]
    assert float(d1.min()) > 0.0
    outs = [_raw_search(q.cuda(), r.cuda(), forced) for forced in (1, 0)]
    assert _bits_equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])
    got_d, got_i = outs[0][0].cpu().double(), outs[0][1].cpu().long()
    assert int(got_i.min()) >= 0 and int(got_i.max()) < c.n_ref
    dist_ratio = float(((got_d - d1).abs() / d1).max()) / gc.U24
    choice_ratio = float((gc.chosen_distance(q, r, got_i) / d1 - 1.0).max()) / gc.U24
    print(f"nn_search {mode}: worst |d - d64| / d64 = {dist_ratio:.3f} x 2^-24, chosen / nearest - 1 = {choice_ratio:.3f} x 2^-24 (bound 8)")
    assert dist_ratio <= 8.0 and choice_ratio <= 8.0


def test_nn_search_non_finite_in_a_later_tile_and_item(grid_case):
    c = gc.GRID
    q, r, _, clean_d, clean_i = grid_case
    (qb, qi), (rb, ri) = gc.NAN_QUERY, gc.NAN_REF
    q, r = q.clone(), r.clone()
    q[qb, qi, 1] = float("nan")
    r[rb, ri, 2] = float("nan")
    lost = clean_i[rb].cpu() == ri                                              # queries whose clean answer was the point now NaN
    assert int(lost.sum()) > 0, "the NaN reference point was nobody's neighbour: the case checks nothing"
    r_without = r.clone()
    r_without[rb, ri] = 1e3                                                     # for fp64: the same set with that point out of reach
    d1 = gc.brute_force_nn(q, r_without)[0]
    for forced in (1, 0):
        dist, index = _raw_search(q.cuda(), r.cuda(), forced)
        assert float(dist[qb, qi]) == float("inf") and int(index[qb, qi]) == -1
        assert int((index[rb] == ri).sum()) == 0, "a NaN reference point was chosen"
        same = torch.ones(c.batch, c.n_query, dtype=torch.bool)
        same[qb, qi] = False
        same[rb] &= ~lost
        same = same.cuda()
        assert _bits_equal(dist[same], clean_d[same]) and torch.equal(index[same], clean_i[same]), forced
        # those that lost their neighbour found the next one
        rest = lost.nonzero()[:, 0]
        got_d, got_i = dist[rb].cpu().double()[rest], index[rb].cpu().long()[rest]
        assert float((got_d - d1[rb][rest]).abs().max()) <= 1e-6
        assert float((gc.chosen_distance(q[rb:rb + 1, rest], r_without[rb], got_i[None]) - d1[rb][rest]).max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ m324_dist_stats
def _raw_stats(d, threshold):
    """m324_dist_stats through the C ABI: the input sits between NaN guards (a read outside it poisons the sum), the outputs are
    guard-padded.  d [B,n] fp32 (CPU) -> (sum fp64 [B], count int64 [B]) on the device"""
    from motion324_amd import lib
    B, n = d.shape
    whole, _ = gc.padded(d.reshape(-1), GUARD, float("nan"))
    whole = whole.cuda()
    partial = torch.full((B * 64 + GUARD,), SENTINEL_D, dtype=torch.float64, device="cuda")
    total = torch.full((B + GUARD,), SENTINEL_D, dtype=torch.float64, device="cuda")
    count = torch.full((B + GUARD,), SENTINEL_L, dtype=torch.int64, device="cuda")
    rc = lib.load().m324_dist_stats(whole[GUARD:].data_ptr(), n, B, float(threshold), partial.data_ptr(), total.data_ptr(), count.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    lib.check(rc, "m324_dist_stats")
    torch.cuda.synchronize()
    assert bool((partial[B * 64:] == SENTINEL_D).all()) and bool((total[B:] == SENTINEL_D).all()) and bool((count[B:] == SENTINEL_L).all()), \
        "guard entries were written"
    return total[:B], count[:B]


@pytest.mark.parametrize("batch", gc.STAT_BATCHES)
@pytest.mark.parametrize("n", gc.STAT_SIZES)
def test_dist_stats_sizes_against_fp64(n, batch):
    from motion324_amd import ops
    d = gc.stat_input(n, batch)
    want_sum, want_count, sum_abs = gc.stats_reference(d, 0.02)
    total, count = _raw_stats(d, 0.02)
    assert np.array_equal(count.cpu().numpy(), want_count), (count.tolist(), want_count.tolist())
    err, bound = np.abs(total.cpu().numpy() - want_sum), n * 2.0 ** -53 * sum_abs
    print(f"dist_stats n={n} batch={batch}: worst |sum - fp64| / (n 2^-53 sum|d|) = {float((err / bound).max()):.3e}")
    assert np.all(err <= bound), (err.tolist(), bound.tolist())
    # the wrapper gives the raw call's bits, and every row of the batch equals its own call
    o_sum, o_count = ops.dist_stats(d.cuda(), 0.02)
    assert _bits_equal(o_sum, total) and torch.equal(o_count, count)
    for b in range(batch):
        s1, c1 = _raw_stats(d[b:b + 1], 0.02)
        assert _bits_equal(s1, total[b:b + 1]) and int(c1) == int(count[b]), b
        s0, c0 = ops.dist_stats(d[b].cuda(), 0.02)                            # the 1-D form
        assert _bits_equal(s0.reshape(1), total[b:b + 1]) and int(c0) == int(count[b])


def test_dist_stats_compares_strictly_and_in_fp64():
    d, below = gc.strict_input()
    for rows in (d[None], torch.stack([torch.ones_like(d), d, torch.ones_like(d)])):
        total, count = _raw_stats(rows, gc.STAT_THRESHOLD)
        want = [0] * (rows.shape[0] // 2) + [below] + [0] * (rows.shape[0] // 2)
        assert count.tolist() == want, f"entries at, one fp32 step below and one above {gc.STAT_THRESHOLD}: only the {below} below count, got {count.tolist()}"
        assert np.array_equal(total.cpu().numpy(), gc.stats_reference(rows, gc.STAT_THRESHOLD)[0])     # these sums are exact in fp64
    # float32(0.02) lies below the fp64 threshold 0.02: it counts, in the first pass and in a later one
    d = torch.ones(gc.STAT_SIZES[-1])
    d[[7, gc.STAT_PASS + 7]] = 0.02
    assert float(d[7].double()) < 0.02
    assert _raw_stats(d[None], 0.02)[1].tolist() == [2]
    assert _raw_stats(d[None], float(d[7].double()))[1].tolist() == [0]        # ... and not below itself


def test_dist_stats_non_finite_entry_in_a_later_pass():
    d = gc.stat_input(gc.STAT_SIZES[-1], 3)
    clean_sum, clean_count = _raw_stats(d, 0.02)
    row, at = gc.STAT_INF_AT
    was_below = bool(d[row, at] < 0.02)
    d[row, at] = float("inf")
    total, count = _raw_stats(d, 0.02)
    assert float(total[row]) == float("inf")
    others = [b for b in range(3) if b != row]
    assert bool(torch.isfinite(total[others]).all()) and _bits_equal(total[others], clean_sum[others])
    assert torch.equal(count[others], clean_count[others]) and int(count[row]) == int(clean_count[row]) - int(was_below)


# ------------------------------------------------------------------------------------------------ m324_transform_points
@pytest.mark.parametrize("n", gc.TRANSFORM_SIZES)
def test_transform_points_sizes_against_fp64(n):
    from motion324_amd import lib, ops
    x = gc.unit_points(70 + n, n) * 2 - 1
    params = gc.rigid_params(71, s=0.97)
    want, want_abs = gc.transform_reference(x, params)
    # from the reference alone: no component so close to zero that the fp64 roundings (2^-50 of the terms) show beside half an fp32 ulp
    assert float(np.abs(want).min()) > 2.0 ** -20 * float(want_abs.max()), float(np.abs(want).min())
    out = torch.full((n * 3 + GUARD,), SENTINEL_F, dtype=torch.float32, device="cuda")
    xd, pd = x.cuda(), params.cuda()
    lib.check(lib.load().m324_transform_points(xd.data_ptr(), n, pd.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "m324_transform_points")
    torch.cuda.synchronize()
    assert bool((out[n * 3:] == SENTINEL_F).all()), "guard entries were written"
    got = out[:n * 3].reshape(n, 3)
    ratio = float((np.abs(got.cpu().double().numpy() - want) / np.abs(want)).max()) / gc.U24
    print(f"transform_points n={n}: worst |out - fp64| / |fp64| = {ratio:.4f} x 2^-24 (bound 1: half an ulp)")
    assert ratio <= 1.0
    assert _bits_equal(ops.transform_points(xd, pd), got)
    shaped = ops.transform_points(xd.reshape(1, n, 3), pd)
    assert shaped.shape == (1, n, 3) and _bits_equal(shaped[0], got)


def test_transform_points_with_two_leading_dimensions():
    from motion324_amd import ops
    x = gc.unit_points(75, 7, 1001)                                            # 7007 points as [7, 1001, 3]
    pd = gc.rigid_params(71, s=0.97).cuda()
    shaped = ops.transform_points(x.cuda(), pd)
    assert shaped.shape == (7, 1001, 3) and _bits_equal(shaped.reshape(-1, 3), ops.transform_points(x.reshape(-1, 3).cuda(), pd))
    want = gc.transform_reference(x, gc.rigid_params(71, s=0.97))[0]
    assert float(np.abs(shaped.cpu().double().numpy() - want).max()) <= 2.0 ** -23          # one rounding of a value below 2


# ------------------------------------------------------------------------------------------------ m324_icp_moments
def _raw_moments(src, params, tgt, index, partial_fill=SENTINEL_D):
    """m324_icp_moments through the C ABI: target and index sit between sentinel guards that must come back untouched, record and
    partial scratch are guard-padded; `partial_fill` is what the scratch holds before the call.  Returns the record (numpy [32])"""
    from motion324_amd import lib
    n, nt = src.shape[0], tgt.shape[0]
    t_whole, _ = gc.padded(tgt, gc.TARGET_GUARD, gc.TARGET_SENTINEL)
    i_whole, _ = gc.padded(index, gc.TARGET_GUARD, gc.INDEX_SENTINEL)
    t_dev, i_dev, s_dev, p_dev = t_whole.cuda(), i_whole.cuda(), src.cuda().contiguous(), params.cuda()
    partial = torch.full((64 * 32 + GUARD,), partial_fill, dtype=torch.float64, device="cuda")
    partial[64 * 32:] = SENTINEL_D
    record = torch.full((32 + GUARD,), SENTINEL_D, dtype=torch.float64, device="cuda")
    rc = lib.load().m324_icp_moments(s_dev.data_ptr(), n, p_dev.data_ptr(), t_dev[gc.TARGET_GUARD:].data_ptr(), nt,
                                     i_dev[gc.TARGET_GUARD:].data_ptr(), partial.data_ptr(), record.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    lib.check(rc, "m324_icp_moments")
    torch.cuda.synchronize()
    assert bool((partial[64 * 32:] == SENTINEL_D).all()) and bool((record[32:] == SENTINEL_D).all()), "guard entries were written"
    assert torch.equal(t_dev.cpu(), t_whole) and torch.equal(i_dev.cpu(), i_whole), "the target or the index changed"
    return record[:32].cpu().numpy()


@pytest.mark.parametrize("n", gc.MOM_SIZES)
def test_icp_moments_all_entries_against_fp64(n):
    from motion324_amd import ops
    src, tgt, index = gc.moment_case(n)
    params = gc.rigid_params(5)
    want, want_abs = gc.moment_record(src, params, tgt, index)
    rec = _raw_moments(src, params, tgt, index)
    assert rec[0] == float(n) and rec[30] == 0.0 and rec[31] == 0.0
    bound = gc.moment_bound(n, want_abs[1:30])
    ratio = np.abs(rec[1:30] - want[1:30]) / bound
    print(f"icp_moments n={n}: worst |entry - fp64| / ((n + 16) 2^-52 S) = {float(ratio.max()):.3e} at entry {1 + int(ratio.argmax())}")
    assert np.all(ratio <= 1.0), {1 + int(k): float(ratio[k]) for k in np.nonzero(~(ratio <= 1.0))[0]}
    # deterministic, whatever the scratch held; the wrapper gives the same bits
    again = _raw_moments(src, params, tgt, index, partial_fill=float("nan"))
    assert np.array_equal(rec.view(np.int64), again.view(np.int64))
    wrapped = ops.icp_moments(src.cuda(), params.cuda(), tgt.cuda(), index.cuda()).cpu().numpy()
    assert np.array_equal(rec.view(np.int64), wrapped.view(np.int64))


@pytest.mark.parametrize("bad", [-1, gc.MOM_TARGET], ids=["minus_one", "n_target"])
def test_icp_moments_unmatched_index_in_the_second_pass_poisons(bad):
    n = gc.MOM_POISON_N
    src, tgt, index = gc.moment_case(n)
    params = gc.rigid_params(5)
    clean = _raw_moments(src, params, tgt, index)
    assert np.all(np.isfinite(clean))
    index[gc.MOM_POISON_AT] = bad
    gc.check_poisoned(_raw_moments(src, params, tgt, index), clean)


# ------------------------------------------------------------------------------------------------ the host path on top
def test_chamfer_and_fscore_over_several_tiles_against_fp64():
    from motion324_amd import evaluation as ev
    p1, p2 = gc.chamfer_case()
    chamfer, fscore, margin = gc.chamfer_reference(p1, p2)
    assert margin > 1e-6, "a nearest distance lies within 1e-6 of the threshold: the seed of gc.chamfer_case does not qualify"
    cd, fs = ev.chamfer_and_fscore(p1.cuda(), p2.cuda(), gc.CHAMFER_THRESHOLD)
    assert cd.dtype == torch.float64 and cd.shape == fs.shape == (p1.shape[0],)
    for f in range(p1.shape[0]):
        print(f"frame {f}: chamfer {float(cd[f])!r} (fp64 {float(chamfer[f])!r}), fscore {float(fs[f])!r} (fp64 {float(fscore[f])!r})")
        assert abs(float(cd[f]) - chamfer[f]) <= 1e-6, f
        assert float(fs[f]) == fscore[f], f
        assert (float(cd[f]), float(fs[f])) == ev.chamfer_and_fscore(p1[f].cuda(), p2[f].cuda(), gc.CHAMFER_THRESHOLD), f


def _big_recovery_case():
    """_recovery_case's 2000-point target; the source: 17000 exact copies of its points (every point eight or nine times) under the
    inverse of the same rigid motion -- more points than one pass of m324_icp_moments covers"""
    _, target, R, t = _recovery_case()
    pick = np.arange(gc.ICP_BIG_SOURCE) % len(target)
    source = (target.astype(np.float64)[pick] - t) @ R
    return source.astype(np.float32), target, pick


def test_icp_alignment_past_one_pass_of_the_moment_kernel(monkeypatch):
    """the only test that sends more than 16384 points through the loop end to end; 9 iterations and a few milliseconds when it
    was written, so max_iterations stays at its default"""
    from motion324_amd import evaluation as ev, ops
    source, target, pick = _big_recovery_case()
    calls = []
    real = ops.icp_moments
    monkeypatch.setattr(ops, "icp_moments", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    t0 = time.perf_counter()
    R, t, s = ev.icp_alignment(source, target)
    seconds = time.perf_counter() - t0
    aligned = ev.apply_icp_alignment(source.astype(np.float64), R, t, s)
    err = np.abs(aligned - target.astype(np.float64)[pick]).max()
    print(f"recovery of {len(source)} points: {len(calls)} iterations in {seconds:.3f} s, max |aligned - original| {err:.3e}, s {s!r}")
    assert err <= 1e-5


def test_icp_alignment_with_a_nan_source_point_raises():
    """the NaN point is met in the second pass of the moment kernel; the search leaves it unmatched (index -1), the record is
    poisoned, and the host reports it"""
    from motion324_amd import evaluation as ev
    from motion324_amd.lib import M324Error
    source, target, _ = _big_recovery_case()
    source[gc.MOM_PASS + 116, 1] = np.nan
    with pytest.raises(M324Error, match="non-finite moment sums"):
        ev.icp_alignment(source, target)
