"""Case tables, seeded inputs and fp64 references of the geometry evaluation kernels of motion324_amd/csrc/geometry.hip
(m324_nn_search, m324_dist_stats, m324_transform_points, m324_icp_moments), shared by tests/test_eval_cpu.py and
tests/test_geometry_gpu.py.  Nothing here touches a device.  Inputs are fp32; every reference is fp64 on those same fp32 numbers.

The work decomposition the tables straddle, restated here (never imported from the code under test; tests/test_eval_cpu.py reads the
constants from the text of geometry.hip and holds the tables against them, so a retune fails there instead of moving a table
off its boundary):
  search   a work item is (batch item, query tile, reference slice) of a flat grid: slice = item % slices, qt = (item / slices) %
           qtiles, b = item / (slices * qtiles).  A query tile holds NN_THREADS * NN_QPL = 1024 queries; a slice holds per_slice =
           ceil(n_ref / slices) reference points and stages them NN_CHUNK = 1024 at a time, padded to a multiple of 4 records.
           Forced slice counts are capped at NN_MAX_SLICES = 64 and at n_ref; an automatic slice is never shorter than
           NN_MIN_SLICE = 256.  Slice s of a sliced call writes its partial at s * (batch * n_query) + b * n_query + query.
  stats    STAT_BLOCKS = 32 workgroups of 256 threads per batch row, grid stride 32 * 256 = 8192 entries per pass.
  moments  MOM_BLOCKS = 64 workgroups of 256 threads, grid stride 64 * 256 = 16384 points per pass."""
import math
from collections import namedtuple

import numpy as np
import torch

# what the tables assume of geometry.hip (test_eval_cpu.py: test_geometry_tables_straddle_the_kernel_constants)
TILE = 1024                  # NN_THREADS * NN_QPL queries per work item
CHUNK = 1024                 # NN_CHUNK reference records per LDS fill
MAX_SLICES = 64              # NN_MAX_SLICES
MIN_SLICE = 256              # NN_MIN_SLICE
STAT_PASS = 32 * 256         # STAT_BLOCKS workgroups of 256 entries
MOM_PASS = 64 * 256          # MOM_BLOCKS workgroups of 256 points

# ------------------------------------------------------------------------------------------------ the tables
TILE_QUERIES = (1023, 1024, 1025, 2049, 3 * 1024 + 7)      # below, at and above one tile; three tiles; a ragged fourth
TILE_REFS = (1, 1024, 1025)                                # one record; exactly one LDS chunk; a second chunk of one record
TILE_BATCHES = (1, 3)

GridCase = namedtuple("GridCase", "batch n_query n_ref forced")
# (forced slice count -> slices m324_nn_plan must answer); 0 = automatic.  7 slices: per_slice = 215, no multiple of 4.  3 slices:
# the one count here that shares a factor with the 3 query tiles -- `qt = item % qtiles` in place of `(item / slices) % qtiles` merely
# renumbers the work items while slices and qtiles are coprime (2, 7 and 64 against 3), and computes some cells twice and others never
# once they are not
GRID = GridCase(3, 2049, 1500, ((1, 1), (2, 2), (3, 3), (7, 7), (64, 64)))
EMPTY = GridCase(1, 1025, 70, ((64, 64),))                 # per_slice = 2: slices 35 .. 63 own nothing
CAPPED = GridCase(1, 1025, 70, ((100, 64), (65, 64)))      # asked for more than NN_MAX_SLICES
CAPPED_BY_REF = GridCase(1, 8, 5, ((64, 5), (7, 5)))       # asked for more slices than reference points (host-only: plan query)
FORCED_CASES = (GRID, EMPTY, CAPPED, CAPPED_BY_REF)

# the planted pair of the tie test (GRID's reference size and slice counts, one batch item): a reference point and its exact duplicate,
# in different 1024-record chunks of the one-slice call and in different slices of every sliced call (per_slice 750, 500, 215, 24,
# and 750 .. 300 for the 2 .. 5 slices the automatic rule may choose)
TIE_QUERIES = 3 * 1024 + 7
TIE_LOW, TIE_HIGH = 100, 1300
TIE_QUERY_TILE0, TIE_QUERY_TILE2 = 5, 2 * 1024 + 452       # an exact hit (d2 = 0) and a query 0.25 away (equal non-zero d2)

NAN_QUERY = (2, 1500)                                      # (batch item, query) of GRID: a later item, the second tile
NAN_REF = (1, 700)                                         # (batch item, reference point) of GRID

STAT_SIZES = (1, 255, STAT_PASS - 1, STAT_PASS, STAT_PASS + 1, 3 * STAT_PASS + 5)
STAT_BATCHES = (1, 3)
STAT_THRESHOLD = 0.03125                                   # exact in fp32
STAT_PLANTS = (5, 300, STAT_PASS - 1, STAT_PASS + 3, 2 * STAT_PASS + 100, 3 * STAT_PASS + 4)      # first pass / later passes
STAT_INF_AT = (1, STAT_PASS + 17)                          # (row, entry): met in the second pass

TRANSFORM_SIZES = (1, 255, 257, 70001)

MOM_SIZES = (1, 257, MOM_PASS - 1, MOM_PASS, MOM_PASS + 1, 40000)
MOM_TARGET = 1500
MOM_POISON_N, MOM_POISON_AT = 40000, MOM_PASS + 3616       # position 20000: met in the second pass
MOM_MATCHED = (1,) + tuple(range(5, 17)) + tuple(range(20, 29))          # record entries that involve the matched point
MOM_UNMATCHED = (0, 2, 3, 4, 17, 18, 19, 29)                             # ... and those that do not

CHAMFER_SHAPES = ((2, 2500), (2, 3000))                    # unequal, each more than one tile
CHAMFER_SEED, CHAMFER_THRESHOLD = 0, 0.02
ICP_BIG_SOURCE = 17000                                     # more than one m324_icp_moments pass

U24 = 2.0 ** -24


def per_slice(n_ref, slices):
    return -(-n_ref // slices)


# ------------------------------------------------------------------------------------------------ search inputs
def unit_points(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, 3, generator=g)


def planted_search_case(seed, batch, n_query, n_ref, shared):
    """Queries with a KNOWN nearest reference: the references are uniform in the unit cube, query i of item b is reference
    assign[b, i] plus a jitter of at most 1e-3 per coordinate, assign[b] = (a permutation of the queries) % n_ref -- a different
    permutation per item, so a query read from another tile, slot or item gets another index.  Returns (q [B,nq,3],
    r [B,nr,3] or, shared, [nr,3], assign int64 [B,nq])."""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(1 if shared else batch, n_ref, 3, generator=g)
    assign = torch.stack([torch.randperm(n_query, generator=g) % n_ref for _ in range(batch)])
    jitter = (torch.rand(batch, n_query, 3, generator=g) * 2 - 1) * 1e-3
    q = torch.stack([r[0 if shared else b][assign[b]] for b in range(batch)]) + jitter
    return q, (r[0] if shared else r), assign


def tie_case(seed):
    """(q [TIE_QUERIES,3], r [GRID.n_ref,3]): unit-cube points; reference points TIE_LOW and TIE_HIGH are both (2, 2, 2), away from
    everything else; query TIE_QUERY_TILE0 sits on that point and query TIE_QUERY_TILE2 0.25 beside it (all exact in fp32)"""
    q, r = unit_points(seed, TIE_QUERIES), unit_points(seed + 1, GRID.n_ref)
    r[TIE_LOW] = r[TIE_HIGH] = torch.tensor([2.0, 2.0, 2.0])
    q[TIE_QUERY_TILE0] = torch.tensor([2.0, 2.0, 2.0])
    q[TIE_QUERY_TILE2] = torch.tensor([2.25, 2.0, 2.0])
    return q, r


# ------------------------------------------------------------------------------------------------ search reference
def brute_force_nn(q, r, block=512):
    """fp64 brute force on fp32 inputs: q [B,nq,3], r [B,nr,3] or [nr,3] -> (nearest distance [B,nq], its index (the lowest among
    equals), second-nearest distance (+inf with one reference point)), every distance sqrt(dx^2 + dy^2 + dz^2) of fp64 differences"""
    q, r = q.double(), r.double()
    B, nq = q.shape[0], q.shape[1]
    d1 = torch.empty(B, nq, dtype=torch.float64)
    d2 = torch.full((B, nq), float("inf"), dtype=torch.float64)
    idx = torch.empty(B, nq, dtype=torch.int64)
    for b in range(B):
        rb = r if r.dim() == 2 else r[b]
        for i0 in range(0, nq, block):
            diff = q[b, i0:i0 + block, None, :] - rb[None, :, :]
            d = (diff[..., 0] ** 2 + diff[..., 1] ** 2 + diff[..., 2] ** 2).sqrt()
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)       # a non-finite pair never wins
            low, arg = d.min(dim=1)                                                    # the first of equal minima
            idx[b, i0:i0 + block] = arg
            d1[b, i0:i0 + block] = low
            if rb.shape[0] > 1:
                d2[b, i0:i0 + block] = d.scatter(1, arg[:, None], float("inf")).min(dim=1).values
    return d1, idx, d2


def chosen_distance(q, r, index):
    """fp64 distance of every query to the reference point `index` names ([B,nq] int)"""
    q, r = q.double(), r.double()
    rb = r[None].expand(q.shape[0], -1, -1) if r.dim() == 2 else r
    picked = torch.gather(rb, 1, index.long()[..., None].expand(-1, -1, 3))
    diff = q - picked
    return (diff[..., 0] ** 2 + diff[..., 1] ** 2 + diff[..., 2] ** 2).sqrt()


# ------------------------------------------------------------------------------------------------ statistics
def stat_input(n, batch, seed=0):
    """[batch, n] fp32 in [0, 0.05): every row its own data"""
    g = torch.Generator().manual_seed(9000 + 31 * n + batch + seed)
    return torch.rand(batch, n, generator=g) * 0.05


def strict_input(threshold=STAT_THRESHOLD):
    """[3 * STAT_PASS + 5] of 1.0 with, at STAT_PLANTS, the threshold itself, one fp32 step below and one above (twice each: in the
    first pass and in a later one).  Returns (the entries, how many lie below the threshold: the two `below` plants)"""
    t = np.float32(threshold)
    assert float(t) == threshold, "the threshold must be exact in fp32"
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))
    d = np.ones(STAT_SIZES[-1], dtype=np.float32)
    d[list(STAT_PLANTS)] = [t, below, above, above, t, below]
    return torch.from_numpy(d), 2


def stats_reference(d, threshold):
    """per row of d [B,n] fp32: (the correctly rounded fp64 sum, the count of entries below the threshold compared in fp64, the
    sum of absolute values)"""
    rows = d.double().numpy()
    total = np.array([math.fsum(row) for row in rows])
    return total, (rows < float(threshold)).sum(axis=1).astype(np.int64), np.array([math.fsum(np.abs(row)) for row in rows])


# ------------------------------------------------------------------------------------------------ transform and moments
def rigid_params(seed, s=1.03):
    """13 fp64 values (s, R row-major, t) with a proper rotation far from the identity, a scale other than 1 and a translation"""
    g = torch.Generator().manual_seed(seed)
    Q = torch.linalg.qr(torch.rand(3, 3, generator=g, dtype=torch.float64))[0]
    if float(torch.linalg.det(Q)) < 0:
        Q[:, 0] = -Q[:, 0]
    t = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    return torch.cat([torch.tensor([s], dtype=torch.float64), Q.reshape(9), t])


def transform_reference(x, params):
    """s * (R x) + t in fp64 (numpy [..., 3]); also the same expression on absolute values"""
    p = params.numpy()
    s, R, t = p[0], p[1:10].reshape(3, 3), p[10:13]
    x = x.double().numpy()
    return s * (x @ R.T) + t, abs(s) * (np.abs(x) @ np.abs(R).T) + np.abs(t)


def moment_case(n, seed=0):
    """(source [n,3], target [MOM_TARGET,3], index int32 [n]): unit-cube points; random in-range indices that include 0 and
    MOM_TARGET - 1 (as far as n allows: n = 1 gets MOM_TARGET - 1)"""
    g = torch.Generator().manual_seed(7000 + n + seed)
    src, tgt = torch.rand(n, 3, generator=g) - 0.5, torch.rand(MOM_TARGET, 3, generator=g) - 0.5
    index = torch.randint(0, MOM_TARGET, (n,), generator=g, dtype=torch.int32)
    index[n // 2] = MOM_TARGET - 1
    if n > 1:
        index[n - 1] = 0
    return src, tgt, index


def _record(x, st, m, dist_of):
    """the 32 sums of include/m324.h from per-point arrays [n,3], each sum correctly rounded (math.fsum of the fp64 terms)"""
    rec = np.zeros(32)
    rec[0] = float(len(x))
    rec[1] = math.fsum(dist_of(st, m))
    for c in range(3):
        rec[2 + c] = math.fsum(st[:, c])
        rec[5 + c] = math.fsum(m[:, c])
        rec[17 + c] = math.fsum(x[:, c])
        for e in range(3):
            rec[8 + 3 * c + e] = math.fsum(st[:, c] * m[:, e])
            rec[20 + 3 * c + e] = math.fsum(x[:, c] * m[:, e])
    rec[29] = math.fsum(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    return rec


def moment_record(src, params, target, index):
    """(the fp64 record of include/m324.h, the same record on absolute values).  record: [0] n, [1] sum |st - m|, [2..4] sum st,
    [5..7] sum m, [8..16] sum st (x) m (row = st component), [17..19] sum x, [20..28] sum x (x) m, [29] sum |x|^2, [30..31] zero,
    with st = s (R x) + t and m = target[index].  The absolute record takes |x|, |R|, |t|, |m| (so its st bounds every term of st)
    and |st| + |m| for the difference: S of tests/ERROR_BOUNDS_GEOMETRY.md."""
    st, st_abs = transform_reference(src, params)
    x = src.double().numpy()
    m = target.double().numpy()[index.long().numpy()]
    euclid = lambda a, b: np.sqrt(((a - b) ** 2).sum(axis=1))
    return _record(x, st, m, euclid), _record(np.abs(x), st_abs, np.abs(m), lambda a, b: np.sqrt(((a + b) ** 2).sum(axis=1)))


def moment_record_loop(src, params, target, index):
    """the record once more as a literal loop over the points in Python floats: what moment_record is held against"""
    p = [float(v) for v in params]
    rec = [0.0] * 32
    for i in range(src.shape[0]):
        x = [float(v) for v in src[i]]
        st = [p[0] * (x[0] * p[1 + 3 * c] + x[1] * p[2 + 3 * c] + x[2] * p[3 + 3 * c]) + p[10 + c] for c in range(3)]
        m = [float(v) for v in target[int(index[i])]]
        rec[0] += 1.0
        rec[1] += math.sqrt(sum((st[c] - m[c]) ** 2 for c in range(3)))
        for c in range(3):
            rec[2 + c] += st[c]
            rec[5 + c] += m[c]
            rec[17 + c] += x[c]
            for e in range(3):
                rec[8 + 3 * c + e] += st[c] * m[e]
                rec[20 + 3 * c + e] += x[c] * m[e]
        rec[29] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
    return np.array(rec)


def moment_bound(n, S):
    """|entry - fp64 entry| <= (n + 16) 2^-52 S: n additions at 2^-53 each on either side, 16 for the roundings inside a term"""
    return (n + 16) * 2.0 ** -52 * S


# a finite value no sum of unit-cube data comes near: a read outside `target` shows as a wrong FINITE entry where NaN is due
TARGET_SENTINEL = 12345.0
INDEX_SENTINEL = 7                      # a valid-looking index: a read outside `index` goes unnoticed by the kernel, not by the record
TARGET_GUARD = 64                       # points in front of and behind the target; entries in front of and behind the index


def moments_model(src, params, padded_target, n_target, index, drop_upper_bound=False):
    """A CPU statement of icp_moments_partial_kernel's addressing: `padded_target` is the flat allocation (TARGET_GUARD sentinel
    points, the target, TARGET_GUARD sentinel points) and the kernel's `target` pointer sits TARGET_GUARD points in.  ok = 0 <= j <
    n_target, else NaN -- or, with drop_upper_bound, the planted defect `ok = j >= 0`, which reads the guard.  Returns the record."""
    flat = padded_target.double().numpy().reshape(-1, 3)
    j = index.long().numpy()
    ok = (j >= 0) if drop_upper_bound else ((j >= 0) & (j < n_target))
    m = np.where(ok[:, None], flat[np.clip(TARGET_GUARD + j, 0, len(flat) - 1)], np.nan)
    st, _ = transform_reference(src, params)
    x = src.double().numpy()
    with np.errstate(invalid="ignore"):
        rec = np.zeros(32)
        rec[0] = len(x)
        rec[1] = np.sqrt(((st - m) ** 2).sum(axis=1)).sum()
        rec[2:5], rec[5:8], rec[17:20] = st.sum(axis=0), m.sum(axis=0), x.sum(axis=0)
        rec[8:17], rec[20:29] = (st.T @ m).reshape(9), (x.T @ m).reshape(9)
        rec[29] = (x * x).sum()
    return rec


def padded(t, guard, sentinel):
    """(the allocation: `guard` leading rows of `sentinel`, t, `guard` trailing rows; the view of t inside it)"""
    whole = torch.full((t.shape[0] + 2 * guard,) + tuple(t.shape[1:]), sentinel, dtype=t.dtype)
    whole[guard:guard + t.shape[0]] = t
    return whole, whole[guard:guard + t.shape[0]]


def check_poisoned(record, clean):
    """what a record with one unmatched point must look like beside the clean run's (numpy [32] each)"""
    for k in MOM_MATCHED:
        assert np.isnan(record[k]), f"entry {k} involves the matched point and must be NaN, got {record[k]!r}"
    for k in MOM_UNMATCHED:
        assert record[k] == clean[k], f"entry {k} does not involve the matched point: {record[k]!r} != clean {clean[k]!r}"
    assert record[30] == 0.0 and record[31] == 0.0


# ------------------------------------------------------------------------------------------------ the host path
def chamfer_case(seed=CHAMFER_SEED):
    """two [2, n, 3] fp32 samplings of nearly the same bumpy ellipsoid (eval_inputs.metric_case's surface) with 2500 and 3000
    points: about half of the nearest distances fall under 0.02 and every one stays below 0.2"""
    import eval_inputs
    g = torch.Generator().manual_seed(4000 + seed)
    sets = []
    for (frames, n), wobble in zip(CHAMFER_SHAPES, (0.0, 0.004)):
        d = torch.randn(frames, n, 3, generator=g, dtype=torch.float64).numpy()
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        sets.append(torch.from_numpy(np.stack([0.8 * eval_inputs._blob(d[f], wobble + 0.002 * f) for f in range(frames)]).astype(np.float32)))
    return sets[0], sets[1]


def chamfer_reference(p1, p2, threshold=CHAMFER_THRESHOLD):
    """fp64 brute force of evaluation.chamfer_and_fscore per frame: (chamfer [T], fscore [T], the smallest |d - threshold| over every
    nearest distance of both directions)"""
    d21 = brute_force_nn(p2, p1)[0].numpy()             # points2 to points1: precision
    d12 = brute_force_nn(p1, p2)[0].numpy()             # points1 to points2: recall
    chamfer = d21.mean(axis=1) + d12.mean(axis=1)
    precision, recall = (d21 < threshold).mean(axis=1), (d12 < threshold).mean(axis=1)
    total = precision + recall
    fscore = np.where(total == 0, 0.0, 2 * precision * recall / np.where(total == 0, 1.0, total))
    return chamfer, fscore, min(np.abs(d21 - threshold).min(), np.abs(d12 - threshold).min())
