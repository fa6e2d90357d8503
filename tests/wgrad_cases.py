"""Cases, operands, an fp64 model and the checker of the weight-gradient GEMM m324_gemm_tn (dW[n, j] = sum_m X[m, n] Y[m, j]),
shared by tests/test_wgrad_cpu.py and tests/test_wgrad_gpu.py.  Nothing here touches a device.

The instrument: a bf16 x bf16 product is exact in fp32, and with INTEGER operands in -8 .. 8 every partial sum of a column of up
to 262144 tokens is an integer below 2^24 -- exact in fp32 whatever the order of the additions.  The kernel's result must then equal
the fp64 result bit for bit: one token contracted twice or not at all, one value in another (n, j), changes an integer.

The rules restated here (never imported from the code under test):
  slices   include/m324.h, m324_gemm_tn: "the M tokens are cut into `slices` ranges of whole 64-row tiles"; motion324_amd/csrc/gemm.hip
           above the launch: ks = ceil(ceil(M / slices) / 64) * 64 tokens per slice, slice s = tokens s ks .. min((s + 1) ks, M) - 1,
           and no slice may be empty: ks (slices - 1) < M.  ops.gemm_tn clamps what it is asked for to ceil(M / 64) and then
           lowers it until no slice is empty.
  kernel   gemm.hip: the 256 x 256 pipelined kernel ("big") runs when M % 32 == 0, N % 256 == 0, Kc % 256 == 0 and M / slices >= 256
           (integer division), unless the switch M324_GEMM_TN is 128; the 128 x 128 kernel ("small") otherwise.
The library has NO plan query for this entry point: which kernel a TN_CASES row reaches rests on that documented rule alone.  That
is why every "big" row is run a second time with M324_GEMM_TN = 128 and BOTH runs must be exact -- a wrong guess in the table
changes which kernel a run exercises, it cannot hide a failure."""
from collections import namedtuple

import torch

from test_strides_gpu import SENTINEL, _bits, _signed, assert_sentinel, embedded, window

BF, F32 = torch.bfloat16, torch.float32
SENT = SENTINEL[F32]

Case = namedtuple("Case", "M N Kc slices lengths big why")


def _c(M, N, Kc, slices, lengths, big, why=""):
    return Case(M, N, Kc, slices, tuple(lengths), big, why)


# (M, N, Kc, slices asked) -> the length of every slice, written out (test_wgrad_cpu.py holds slice_plan against them)
TN_CASES = [
    _c(1, 8, 8, 1, [1], False, "smallest legal call"),
    _c(8, 8, 136, 1, [8], False, "N = 8 column clamp, ragged Kc"),
    _c(63, 136, 72, 1, [63], False, "one short stage"),
    _c(64, 128, 128, 1, [64], False, "exactly one stage, one tile"),
    _c(65, 264, 8, 2, [64, 1], False, "one-token last slice, Kc = 8"),
    _c(129, 8, 264, 3, [64, 64, 1], False),
    _c(200, 192, 328, 4, [64, 64, 64, 8], False),
    _c(1000, 136, 72, 5, [256, 256, 256, 232], False, "the wrapper's clamp: 4 slices used"),
    _c(1296, 256, 256, 5, [320] * 4 + [16], False, "M % 32 != 0: one condition short of big"),
    _c(1312, 264, 256, 5, [320] * 4 + [32], False, "N % 256 != 0: one condition short of big"),
    _c(1312, 256, 256, 6, [256] * 5 + [32], False, "M / slices < 256: one condition short of big"),
    _c(256, 256, 256, 1, [256], True, "smallest big call, NH = 8"),
    _c(288, 256, 256, 1, [288], True, "odd NH = 9"),
    _c(1280, 256, 256, 5, [256] * 5, True),
    _c(1312, 256, 256, 5, [320] * 4 + [32], True, "last slice NH = 1"),
    _c(1344, 256, 512, 5, [320] * 4 + [64], True, "last slice NH = 2"),
    _c(1376, 512, 256, 5, [320] * 4 + [96], True, "last slice NH = 3"),
    _c(1408, 256, 256, 5, [320] * 4 + [128], True, "last slice NH = 4, one ring turn"),
]


def case_id(c):
    return f"{c.M}x{c.N}x{c.Kc}s{c.slices}"


# ------------------------------------------------------------------------------------------- the slicing rule
def tokens_per_slice(M, slices):
    """ks of gemm.hip: ceil(ceil(M / slices) / 64) * 64"""
    return (-(-M // slices) + 63) // 64 * 64


def accepted(M, slices):
    """the library's refusal rules for the slicing (gemm.hip, in front of the launch): 1 <= slices <= 65535, no empty slice"""
    return M > 0 and 1 <= slices <= 65535 and tokens_per_slice(M, slices) * (slices - 1) < M


def slice_plan(M, slices):
    """(slices used, ks, [length of every slice]) of ops.gemm_tn(x [M, N], y, slices): the wrapper's clamp, then the library's cut"""
    used = max(1, min(slices, -(-M // 64)))
    while used > 1 and tokens_per_slice(M, used) * (used - 1) >= M:
        used -= 1
    ks = tokens_per_slice(M, used)
    return used, ks, [min(ks, M - s * ks) for s in range(used)]


def big_applies(M, N, Kc, slices):
    """the 256 x 256 pipelined kernel's condition in gemm.hip (`slices` as the library receives it)"""
    return M % 32 == 0 and N % 256 == 0 and Kc % 256 == 0 and M // slices >= 256


def staging_ok(M, slices, ld):
    """the 2 GiB staging guard of gemm.hip: (ks + 64) * max(ldx, ldy) * 2 < 0x7FFFFFFF"""
    return (tokens_per_slice(M, slices) + 64) * ld * 2 < 0x7FFFFFFF


# ------------------------------------------------------------------------------------------- operands
def int_operands(M, N, Kc, seed):
    """bf16 integers in -8 .. 8: x [M, N], y [M, Kc]"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-8, 9, (M, N), generator=g).to(BF), torch.randint(-8, 9, (M, Kc), generator=g).to(BF))


def probe_operands(M, N, Kc):
    """X one-hot per token, X[m, (7 m) % N] = 1, and Y[m, j] = ((3 m + j) % 15) - 7: dW[n] is the sum of the Y rows of the tokens
    that point at n, so a transposing-read lane mix-up, a swapped stage or a wrong swizzle MOVES a value to another (n, j)"""
    m = torch.arange(M)
    x = torch.zeros((M, N))
    x[m, (7 * m) % N] = 1.0
    y = ((3 * m[:, None] + torch.arange(Kc)[None, :]) % 15 - 7).float()
    return x.to(BF), y.to(BF)


def away_from_zero(M, C, seed):
    """bf16 [M, C], magnitude in [0.5, 1], random sign: every product of two such values is at least 0.25 in magnitude"""
    g = torch.Generator().manual_seed(seed)
    mag = (0.5 + 0.5 * torch.rand((M, C), generator=g)).to(BF)            # rounding keeps [0.5, 1]: both ends are bf16 values
    sign = torch.randint(0, 2, (M, C), generator=g) * 2 - 1
    return (mag.float() * sign).to(BF)


def gaussian_operands(M, N, Kc, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((M, N), generator=g).to(BF), (0.3 * torch.randn((M, Kc), generator=g)).to(BF)


# ------------------------------------------------------------------------------------------- the fp64 model and its planted faults
ARITHMETIC_FAULTS = ("drop_last_token_of_ragged_slice", "last_slice_takes_ks_rows", "slice_begins_one_stage_late",
                     "column_clamp_lands_in_a_real_column", "short_ring_reads_slot_of_previous_slice")
LAYOUT_FAULTS = ("tile_written_at_ldc_equals_Kc", "slice_written_at_stride_N_times_Kc", "epilogue_fills_the_ragged_tile")
FAULTS = ARITHMETIC_FAULTS + LAYOUT_FAULTS


def fault_can_occur(fault, c, ldc=None, col0=0):
    """whether `fault` changes anything at case `c` (written into a C of leading dimension ldc > Kc for the layout faults)"""
    used, ks, lengths = slice_plan(c.M, c.slices)
    if fault == "drop_last_token_of_ragged_slice":
        return any(n % 64 for n in lengths)
    if fault == "last_slice_takes_ks_rows":
        return lengths[-1] % 64 != 0                   # the rows of the last 64-row stage past the slice end
    if fault == "slice_begins_one_stage_late":
        return used > 1
    if fault == "column_clamp_lands_in_a_real_column":
        return c.N % 128 != 0 and c.N >= 16
    if fault == "short_ring_reads_slot_of_previous_slice":
        return big_applies(c.M, c.N, c.Kc, used) and used > 1 and lengths[-1] // 32 < 3
    if fault == "tile_written_at_ldc_equals_Kc":
        return ldc is not None and ldc > c.Kc and c.N > 1
    if fault == "slice_written_at_stride_N_times_Kc":
        return ldc is not None and ldc > c.Kc and used > 1
    if fault == "epilogue_fills_the_ragged_tile":
        return ldc is not None and ldc - col0 > c.Kc
    raise KeyError(fault)


def emulate(x, y, slices, fault=None):
    """fp64 model of ops.gemm_tn's launch: the slice partials [slices used, N, Kc], one of the ARITHMETIC_FAULTS planted"""
    assert fault is None or fault in FAULTS, fault
    M, N = x.shape
    used, ks, lengths = slice_plan(M, slices)
    xd, yd = x.double(), y.double()
    parts = []
    for s, n in enumerate(lengths):
        mbeg, mend = s * ks, s * ks + n
        rows = torch.arange(mbeg, mend)
        if fault == "drop_last_token_of_ragged_slice" and n % 64:
            rows = rows[:-1]
        if fault == "last_slice_takes_ks_rows" and s == used - 1 and n % 64:
            # the staging clamps the rows past the slice end to its last row: contracted again unless the X rows are zeroed
            rows = torch.cat([rows, torch.full((64 - n % 64,), mend - 1)])
        if fault == "slice_begins_one_stage_late":
            # every slice but the first skips its first stage, and the slice in front of it covers the gap: the SUM stays right
            if s > 0:
                rows = rows[min(64, n):]
            if s + 1 < used:
                rows = torch.cat([rows, torch.arange(mend, mend + min(64, lengths[s + 1]))])
        if fault == "short_ring_reads_slot_of_previous_slice" and s == used - 1 and s > 0 and n % 32 == 0 and n // 32 < 3:
            rows = torch.cat([rows[:-32], torch.arange(32, 64)])          # half-tile 1 of the first slice for the clamped one
        p = xd[rows].T @ yd[rows]
        if fault == "column_clamp_lands_in_a_real_column" and N % 128 and N >= 16:
            p[N - 16:N - 8] = p[N - 8:N]
        parts.append(p)
    return torch.stack(parts)


def exact_partials(x, y, lengths):
    """what every slice must hold: x[mbeg:mend]^T y[mbeg:mend] in fp64, cast to fp32 (CPU)"""
    xd, yd = x.double().cpu(), y.double().cpu()
    out, m = [], 0
    for n in lengths:
        out.append((xd[m:m + n].T @ yd[m:m + n]).float())
        m += n
    return torch.stack(out)


# ------------------------------------------------------------------------------------------- a strided C and the checker
Layout = namedtuple("Layout", "N Kc slices ldc col0 gap")          # strideC = (N + gap) * ldc


def c_buffer(lay, device="cpu"):
    """One fp32 allocation [1 + slices (N + gap) + 1, ldc] in which EVERY element holds the SENTINEL bits; slice s's window is rows
    1 + s (N + gap) .. + N - 1, columns col0 .. col0 + Kc - 1: a full sentinel row in front and behind, ldc - Kc pad columns, `gap`
    rows between two slices (and behind the last).  Returns (the windows [slices] of [N, Kc] views, the allocation)."""
    N, Kc, ns, ldc, col0, gap = lay
    first, whole = embedded(torch.zeros((N, Kc), dtype=F32, device=device), ldc, col0, SENT, rows_before=1,
                            rows_after=(ns - 1) * (N + gap) + gap + 1)
    _bits(first).fill_(_signed(SENT, F32))
    assert whole.shape == (1 + ns * (N + gap) + 1, ldc)
    return [whole[1 + s * (N + gap):1 + s * (N + gap) + N, col0:col0 + Kc] for s in range(ns)], whole


def stride_c(lay):
    return (lay.N + lay.gap) * lay.ldc


def emulate_into(whole, lay, x, y, fault=None):
    """the model as the kernel's epilogue would leave it in c_buffer(lay): element (n, j) of slice s at C + s strideC + n ldc + j
    with C = the first window's first element; the LAYOUT_FAULTS change that address arithmetic (lay.slices = the slices used)"""
    N, Kc, ns, ldc, col0, gap = lay
    parts = emulate(x, y, ns, fault).float()
    assert parts.shape == (ns, N, Kc), (parts.shape, lay)
    flat = whole.view(-1)
    ld = Kc if fault == "tile_written_at_ldc_equals_Kc" else ldc
    stride = N * Kc if fault == "slice_written_at_stride_N_times_Kc" else stride_c(lay)
    wide = ldc - col0 if fault == "epilogue_fills_the_ragged_tile" else Kc
    n = torch.arange(N)[:, None]
    for s in range(ns):
        rowsrc = parts[s] if wide == Kc else torch.cat([parts[s], torch.zeros((N, wide - Kc))], 1)
        idx = ldc + col0 + s * stride + n * ld + torch.arange(wide)[None, :]
        flat[idx.reshape(-1)] = rowsrc.reshape(-1)
    return whole


def check_total(total, x, y, what):
    """the summed result, bit for bit against fp64"""
    want = (x.double().cpu().T @ y.double().cpu()).float()
    got = total.detach().cpu()
    assert got.shape == want.shape and got.dtype == F32, (what, tuple(got.shape), got.dtype)
    bad = ~(got == want)                                                  # a NaN differs
    assert torch.equal(got, want), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 result; first (n, j): "
                                    f"{bad.nonzero()[:6].tolist()}, got {got[bad][:6].tolist()} want {want[bad][:6].tolist()}")


def check_c(windows, whole, x, y, lengths, what):
    """The checker of a strided C, the same for the model (CPU) and the kernel (GPU): every slice's window holds that slice's exact
    partial, bit for bit; so does their sum; everything outside the windows still holds the sentinel bits."""
    assert len(windows) == len(lengths), (what, len(windows), lengths)
    want = exact_partials(x, y, lengths)
    got = torch.stack([w.detach().cpu() for w in windows])
    for s in range(len(lengths)):
        bad = ~(got[s] == want[s])
        assert torch.equal(got[s], want[s]), (f"{what}: slice {s} of lengths {list(lengths)}: {int(bad.sum())} of {bad.numel()} elements differ from "
                    f"x[mbeg:mend]^T y[mbeg:mend]; first (n, j): {bad.nonzero()[:6].tolist()}, got {got[s][bad][:6].tolist()} "
                    f"want {want[s][bad][:6].tolist()}")
    check_total(got.sum(0), x, y, what + ": sum of the partials")
    # the sentinel check of test_strides_gpu.py knows one window: hand it a copy in which the other windows are sentinels again
    probe = whole.detach().cpu().clone()
    for w in windows[1:]:
        r0, c0, R, C = window(w, whole)
        _bits(probe)[r0:r0 + R, c0:c0 + C] = _signed(SENT, F32)
    r0, c0, R, C = window(windows[0], whole)
    assert_sentinel(probe[r0:r0 + R, c0:c0 + C], probe, SENT, what)
