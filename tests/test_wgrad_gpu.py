"""The weight-gradient GEMMs on the GPU: m324_gemm_tn (both tile kernels) + m324_colsum through ops.gemm_tn, the C ABI itself
with a strided C, backward.weight_grad, and ops.gemm_splitk -- exact on integer operands, slice by slice.

bf16 x bf16 products are exact in fp32 and the sums of integer operands in -8 .. 8 stay below 2^24, so the result must equal the fp64
result BIT FOR BIT in any summation order (tests/wgrad_cases.py; tests/test_wgrad_cpu.py shows which mistakes that catches).  On
Gaussian operands the summed result is held element by element to error_bounds.gemm_tn.  Every launch here is inside the documented
contract and every refusal is returned in front of a launch."""
import pytest
import torch

import error_bounds as eb
import wgrad_cases as wc
from test_strides_gpu import _bits, _signed, assert_sentinel, embedded

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SENT = wc.SENT
IDS = [wc.case_id(c) for c in wc.TN_CASES]
BIG = [c for c in wc.TN_CASES if c.big]
# every row once, the big rows a second time on the 128 x 128 kernel
RUNS = [(c, False) for c in wc.TN_CASES] + [(c, True) for c in BIG]
RUN_IDS = [wc.case_id(c) + ("-forced128" if f else "") for c, f in RUNS]


def _ops():
    from motion324_amd import ops
    return ops


def _err():
    from motion324_amd.lib import M324Error
    return M324Error


_OPERANDS = {}


def _operands(c, kind):
    """CPU operands of a case, built once"""
    key = (wc.case_id(c), kind)
    if key not in _OPERANDS:
        _OPERANDS[key] = {"int": lambda: wc.int_operands(c.M, c.N, c.Kc, 7), "probe": lambda: wc.probe_operands(c.M, c.N, c.Kc),
                          "gauss": lambda: wc.gaussian_operands(c.M, c.N, c.Kc, 141)}[kind]()
    return _OPERANDS[key]


def _wide(t, pad, col0):
    """t [M, C] as a column slice of a NaN-filled [M, C + pad] device buffer starting at column col0"""
    whole = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=DEV)
    view = whole[:, col0:col0 + t.shape[1]]
    view.copy_(t)
    return view


def _sentinel_like(shape):
    return torch.full(shape, _signed(SENT, F32), dtype=torch.int32, device=DEV).view(F32)


def _untouched(t):
    return bool((_bits(t) == _signed(SENT, F32)).all())


def _tn(x, y, c_first, ldc, slices, stride_c, M=None, N=None, Kc=None):
    """m324_gemm_tn itself: C = c_first's first element"""
    ops = _ops()
    px, ldx = ops._rows(x, "x")
    py, ldy = ops._rows(y, "y")
    ops._launch("m324_gemm_tn", px, ldx, py, ldy, c_first.data_ptr(), ldc, x.shape[0] if M is None else M,
                x.shape[1] if N is None else N, y.shape[1] if Kc is None else Kc, slices, stride_c)


# ------------------------------------------------------------------------------------------- 1. exact, through the wrapper
@pytest.mark.parametrize("kind", ["int", "probe"])
@pytest.mark.parametrize("c,forced", RUNS, ids=RUN_IDS)
def test_gemm_tn_is_exact(tune, c, forced, kind):
    ops = _ops()
    if forced:
        tune("M324_GEMM_TN", "128")
    x, y = _operands(c, kind)
    xd, yd = x.to(DEV), y.to(DEV)
    what = f"{wc.case_id(c)} {kind}{' forced 128' if forced else ''}"
    wc.check_total(ops.gemm_tn(xd, yd, c.slices), x, y, what)
    # column slices of wider buffers (as dqkv / qkv are), the pad holds NaN
    wc.check_total(ops.gemm_tn(_wide(x, 8, 0), _wide(y, 8, 0), c.slices), x, y, what + " ld = C + 8")
    wc.check_total(ops.gemm_tn(_wide(x, 64, 64), _wide(y, 64, 64), c.slices), x, y, what + " ld = C + 64, col0 = 64")


# ------------------------------------------------------------------------------------------- 2. the slice partials, a strided C
ABI_CASES = [c for c in wc.TN_CASES if len(c.lengths) > 1] + [c for c in wc.TN_CASES if (c.M, c.N, c.Kc) in
                                                               ((8, 8, 136), (63, 136, 72), (256, 256, 256), (288, 256, 256))]
ABI_RUNS = [(c, False) for c in ABI_CASES] + [(c, True) for c in ABI_CASES if c.big]
# (ldc - Kc, col0, gap rows between the slices): strideC = (N + gap) * ldc; once strideC = N * ldc exactly
C_LAYOUTS = [(4, 0, 3), (4, 4, 3), (64, 0, 3), (64, 4, 3), (64, 4, 0)]


@pytest.mark.parametrize("c,forced", ABI_RUNS, ids=[wc.case_id(c) + ("-forced128" if f else "") for c, f in ABI_RUNS])
def test_gemm_tn_partials_in_a_strided_c(tune, c, forced):
    """the C ABI with ldc > Kc, strideC > N ldc and C off the start of a row: every slice's window holds that slice's exact partial,
    the pad columns, the gap rows and the rows in front and behind keep their sentinel bits"""
    if forced:
        tune("M324_GEMM_TN", "128")
    used, _, lengths = wc.slice_plan(c.M, c.slices)
    x, y = _operands(c, "int")
    xd, yd = x.to(DEV), y.to(DEV)
    for pad, col0, gap in C_LAYOUTS:
        lay = wc.Layout(c.N, c.Kc, used, c.Kc + pad, col0, gap)
        windows, whole = wc.c_buffer(lay, DEV)
        assert windows[0].data_ptr() % 16 == 0 and lay.ldc % 4 == 0
        _tn(xd, yd, windows[0], lay.ldc, used, wc.stride_c(lay))
        wc.check_c(windows, whole, x, y, lengths, f"{wc.case_id(c)} ldc={lay.ldc} col0={col0} gap={gap}{' forced 128' if forced else ''}")
    # the probe operands once, at the tightest layout
    x, y = _operands(c, "probe")
    lay = wc.Layout(c.N, c.Kc, used, c.Kc + 4, 0, 3)
    windows, whole = wc.c_buffer(lay, DEV)
    _tn(x.to(DEV), y.to(DEV), windows[0], lay.ldc, used, wc.stride_c(lay))
    wc.check_c(windows, whole, x, y, lengths, f"{wc.case_id(c)} probe")


# ------------------------------------------------------------------------------------------- 3. out=, accumulate, deferred sums
def _flat_out(N, Kc):
    """a view of N * Kc floats inside a larger flat fp32 buffer of sentinels (the optimizer's layout): (out [1, N Kc], allocation)"""
    return embedded(torch.zeros((1, N * Kc), dtype=F32, device=DEV), N * Kc + 8, 4, SENT)


def _int_out(N, Kc, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-100, 101, (N, Kc), generator=g).float()


WRAPPER_CASES = [c for c in wc.TN_CASES if (c.M, c.N, c.Kc, c.slices) in ((63, 136, 72, 1), (200, 192, 328, 4), (256, 256, 256, 1), (1312, 256, 256, 5))]


@pytest.mark.parametrize("c", WRAPPER_CASES, ids=[wc.case_id(c) for c in WRAPPER_CASES])
def test_gemm_tn_out_and_accumulate(c):
    ops = _ops()
    x, y = _operands(c, "int")
    xd, yd = x.to(DEV), y.to(DEV)
    saved = ops.DEFER_COLSUM
    ops.DEFER_COLSUM = False
    try:
        out, whole = _flat_out(c.N, c.Kc)
        _bits(out).fill_(_signed(SENT, F32))
        got = ops.gemm_tn(xd, yd, c.slices, out=out)
        assert got is out
        wc.check_total(out.view(c.N, c.Kc), x, y, f"{wc.case_id(c)} out=")
        assert_sentinel(out, whole, SENT, f"{wc.case_id(c)} out=")
        # out += dW on integers: exact
        out0 = _int_out(c.N, c.Kc, 11)
        out, whole = _flat_out(c.N, c.Kc)
        out.copy_(out0.reshape(1, -1))
        assert ops.gemm_tn(xd, yd, c.slices, out=out, accumulate=True) is out
        want = (out0.double() + x.double().T @ y.double()).float()
        assert torch.equal(out.view(c.N, c.Kc).cpu(), want), f"{wc.case_id(c)} accumulate"
        assert_sentinel(out, whole, SENT, f"{wc.case_id(c)} accumulate")
    finally:
        ops.DEFER_COLSUM = saved


def test_gemm_tn_deferred_sums():
    """ops.DEFER_COLSUM: three gradients wait in ops.COLSUMS, two of them accumulating into the same out; exact after the flush"""
    ops = _ops()
    c = next(c for c in wc.TN_CASES if (c.M, c.N, c.Kc) == (200, 192, 328))
    c2 = next(c for c in wc.TN_CASES if (c.M, c.N, c.Kc, c.slices) == (1312, 256, 256, 5))
    (x1, y1), (x2, y2), (x3, y3) = wc.int_operands(c.M, c.N, c.Kc, 21), wc.int_operands(c.M, c.N, c.Kc, 22), _operands(c2, "int")
    out0 = _int_out(c.N, c.Kc, 23)
    saved = ops.DEFER_COLSUM
    ops.COLSUMS.flush()
    ops.DEFER_COLSUM = True
    try:
        a, a_whole = _flat_out(c.N, c.Kc)
        a.copy_(out0.reshape(1, -1))
        b, b_whole = _flat_out(c2.N, c2.Kc)
        ops.gemm_tn(x1.to(DEV), y1.to(DEV), c.slices, out=a, accumulate=True)
        ops.gemm_tn(x3.to(DEV), y3.to(DEV), c2.slices, out=b)
        ops.gemm_tn(x2.to(DEV), y2.to(DEV), c.slices, out=a, accumulate=True)
        assert ops.COLSUMS.count == 3 and ops.COLSUMS.busy(a.view(-1)) and ops.COLSUMS.busy(b.view(-1))
        ops.COLSUMS.flush()
        assert ops.COLSUMS.count == 0
        want = (out0.double() + x1.double().T @ y1.double() + x2.double().T @ y2.double()).float()
        assert torch.equal(a.view(c.N, c.Kc).cpu(), want)
        wc.check_total(b.view(c2.N, c2.Kc), x3, y3, "deferred, not accumulating")
        assert_sentinel(a, a_whole, SENT, "deferred a")
        assert_sentinel(b, b_whole, SENT, "deferred b")
    finally:
        ops.DEFER_COLSUM = saved
        ops.COLSUMS.clear()


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,Ka", [(200, 192, 328), (1312, 256, 256), (1100, 768, 64)])
def test_weight_grad_is_exact(M, N, Ka, dtype):
    """backward.weight_grad: bf16 = m324_gemm_tn with the slices of its own rule; fp32 (the parity mode) = ops.transpose +
    ops.gemm_splitk.  Returned, written into out, accumulated onto out: exact."""
    from motion324_amd import backward
    ops = _ops()
    dy, a = wc.int_operands(M, N, Ka, 31)
    dyd, ad = dy.to(dtype).to(DEV), a.to(dtype).to(DEV)
    saved = ops.DEFER_COLSUM
    ops.DEFER_COLSUM = False
    try:
        wc.check_total(backward.weight_grad(dyd, ad), dy, a, f"weight_grad {dtype}")
        out0 = _int_out(N, Ka, 32)
        out = out0.to(DEV)
        got = backward.weight_grad(dyd, ad, out=out, accumulate=True)
        assert got is out and torch.equal(out.cpu(), (out0.double() + dy.double().T @ a.double()).float())
        if dtype == BF:                                           # out= without accumulate is the bf16 path's
            out = _sentinel_like((N, Ka))
            assert backward.weight_grad(dyd, ad, out=out) is out
            wc.check_total(out, dy, a, "weight_grad out=")
    finally:
        ops.DEFER_COLSUM = saved


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K,slices", [(192, 768, 4096, 8), (768, 64, 1024, 3), (100, 52, 640, 4), (8, 8, 64, 4)])
def test_gemm_splitk_is_exact(M, N, K, slices, dtype):
    """ops.gemm_splitk (a [M, K] w [N, K]^T, the contraction in slices + a remainder + m324_colsum) on integer operands; the last
    case has ks == 0: fewer K-tiles than slices, one plain GEMM"""
    ops = _ops()
    g = torch.Generator().manual_seed(41)
    a, w = torch.randint(-8, 9, (M, K), generator=g).to(dtype), torch.randint(-8, 9, (N, K), generator=g).to(dtype)
    out = ops.gemm_splitk(a.to(DEV), w.to(DEV), slices)
    want = (a.double() @ w.double().T).float()
    assert out.dtype == F32 and torch.equal(out.cpu(), want), (M, N, K, slices, dtype, int((out.cpu() != want).sum()))


def test_gemm_splitk_refuses_a_contraction_that_is_no_whole_tile():
    """K = 40 (the case (8, 8, 40, 4)) is outside m324_gemm's contract -- K % 64 == 0 for bf16, K % 32 == 0 for fp32, "pad K with
    zeros" (include/m324.h) -- and is refused in front of the launch; weight_grad's parity path pads the tokens to 64 (ops.transpose)"""
    ops = _ops()
    for dtype in (BF, F32):
        a, w = torch.ones((8, 40), dtype=dtype, device=DEV), torch.ones((8, 40), dtype=dtype, device=DEV)
        with pytest.raises(_err(), match="multiple of"):
            ops.gemm_splitk(a, w, 4)


# ------------------------------------------------------------------------------------------- 4. element-wise, realistic operands
GAUSS = list(wc.TN_CASES) + [wc.Case(4096, 768, 3072, 7, None, True, ""), wc.Case(8192, 2304, 768, 9, None, True, "")]


@pytest.mark.parametrize("c", GAUSS, ids=[wc.case_id(c) for c in GAUSS])
def test_gemm_tn_within_its_bound(tune, c):
    """Gaussian bf16 operands: every element within 2 (M + slices) U32 |x|^T |y| of fp64, nothing masked; two calls give the same
    bits; where a tile runs (M324_XCD) changes no bit at the ragged small shapes"""
    ops = _ops()
    x, y = _operands(c, "gauss")
    xd, yd = x.to(DEV), y.to(DEV)
    used = wc.slice_plan(c.M, c.slices)[0]
    out = ops.gemm_tn(xd, yd, c.slices)
    ref = (xd.double().T @ yd.double()).cpu() if c.M > 2000 else x.double().T @ y.double()        # fp64 of the same bf16 values
    ratio = eb.assert_within(out, ref, eb.gemm_tn(x, y, used), f"gemm_tn {wc.case_id(c)}")
    print(f"WGRAD_RATIO {wc.case_id(c)} {ratio:.4f}")
    assert torch.equal(out, ops.gemm_tn(xd, yd, c.slices))
    if not c.big and c.M <= 2000:
        tune("M324_XCD", "0")
        plain = ops.gemm_tn(xd, yd, c.slices)
        tune("M324_XCD", "1")
        assert torch.equal(plain, ops.gemm_tn(xd, yd, c.slices)) and torch.equal(plain, out)


# ------------------------------------------------------------------------------------------- 5. non-finite values
def test_gemm_tn_nan_stays_in_its_row():
    """a NaN at X[m0, n0] makes exactly row n0 of dW NaN: m0 in the last stage of a middle slice, and in the ragged last stage of
    the last slice"""
    ops = _ops()
    c = next(c for c in wc.TN_CASES if (c.M, c.N, c.Kc) == (1000, 136, 72))
    for m0, n0 in ((256 + 192 + 5, 131), (768 + 192 + 39, 7)):
        x, y = (t.clone() for t in _operands(c, "gauss"))
        x[m0, n0] = float("nan")
        out = ops.gemm_tn(x.to(DEV), y.to(DEV), c.slices).cpu()
        nan = torch.isnan(out)
        assert bool(nan[n0].all()) and int(nan.sum()) == c.Kc and bool(torch.isfinite(out[torch.arange(c.N) != n0]).all()), (m0, n0)


def test_gemm_tn_inf_in_the_last_token():
    """an Inf at Y[M - 1, j0] with M ragged: the kernel contracts the zeroed X rows past the slice end against a repeat of that Y row
    (0 * Inf), so the finite-masks are compared, not the values: column j0 non-finite, everything else finite, as in fp64"""
    ops = _ops()
    c = next(c for c in wc.TN_CASES if (c.M, c.N, c.Kc) == (200, 192, 328))
    j0 = 301
    x, y = (t.clone() for t in _operands(c, "gauss"))
    y[c.M - 1, j0] = float("inf")
    out = ops.gemm_tn(x.to(DEV), y.to(DEV), c.slices).cpu()
    ref = x.double().T @ y.double()
    fin = torch.isfinite(out)
    assert torch.equal(fin, torch.isfinite(ref)) and not bool(fin[:, j0].any()) and int((~fin).sum()) == c.N


# ------------------------------------------------------------------------------------------- 6. the 2 GiB staging limit, both sides
def test_gemm_tn_staging_limit(tune):
    """(ks + 64) * max(ldx, ldy) * 2 < 0x7FFFFFFF: 349440 tokens of a 3072-wide buffer in ONE slice are accepted -- the staging offsets
    of both kernels stay below ks * ld * 2 bytes (gemm.hip: row < mend - mbeg <= ks in the small kernel, (h 32 + r) < ks in the big
    one), inside the 0x7FFFFFFF bytes of dma_rsrc -- and the gradient of the LAST tokens is there; 349504 tokens are refused"""
    ops = _ops()
    R, M, LD = 349504, 349440, 3072
    x = y = out = None
    try:
        x, y = torch.zeros((R, LD), dtype=BF, device=DEV), torch.zeros((R, LD), dtype=BF, device=DEV)
        xs, ys = wc.int_operands(128, 256, 256, 51)
        for t, s, col in ((x, xs, 0), (y, ys, 256)):
            t[:64, col:col + 256] = s[:64].to(DEV)
            t[M - 64:M, col:col + 256] = s[64:].to(DEV)
        assert (M + 64) * LD * 2 < 0x7FFFFFFF <= (R + 64) * LD * 2
        for forced in (False, True):
            if forced:
                tune("M324_GEMM_TN", "128")
            wc.check_total(ops.gemm_tn(x[:M, :256], y[:M, 256:512], 1), xs, ys, f"349440 tokens, forced 128: {forced}")
        wc.check_total(ops.gemm_tn(x[:M, :8], y[:M, 256:264], 1), xs[:, :8], ys[:, :8], "349440 tokens, 8 x 8")
        out = _sentinel_like((256, 256))
        with pytest.raises(_err(), match="2 GiB"):
            ops.gemm_tn(x[:, :256], y[:, 256:512], 1, out=out)
        torch.cuda.synchronize()
        assert _untouched(out)
    finally:
        del x, y, out
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- 7. refusals in front of the launch
def test_gemm_tn_refusals():
    Err = _err()
    M, N, Kc = 64, 8, 8
    x12, y12 = torch.ones((M, 12), dtype=BF, device=DEV), torch.ones((M, 12), dtype=BF, device=DEV)
    x16, y16 = torch.ones((M, 16), dtype=BF, device=DEV), torch.ones((M, 16), dtype=BF, device=DEV)
    x8, y8 = x16[:, :8].contiguous(), y16[:, :8].contiguous()
    c = _sentinel_like((4, N, 16))
    first = c.view(-1)
    calls = {
        "N = 12": lambda: _tn(x12, y8, first, 8, 1, 0),
        "Kc = 12": lambda: _tn(x8, y12, first, 12, 1, 0),
        "ldx % 8 != 0": lambda: _tn(x12[:, :8], y8, first, 8, 1, 0),
        "ldy % 8 != 0": lambda: _tn(x8, y12[:, :8], first, 8, 1, 0),
        "X 8 bytes off": lambda: _tn(x16[:, 4:12], y8, first, 8, 1, 0),
        "Y 8 bytes off": lambda: _tn(x8, y16[:, 4:12], first, 8, 1, 0),
        "ldc < Kc": lambda: _tn(x16, y16, first, 12, 1, 0),
        "ldc % 4 != 0": lambda: _tn(x8, y8, first, 10, 1, 0),
        "C 8 bytes off": lambda: _tn(x8, y8, first[2:], 8, 1, 0),
        "strideC < N ldc": lambda: _tn(x8.repeat(2, 1), y8.repeat(2, 1), first, 16, 2, N * 16 - 4),
        "slices = 0": lambda: _tn(x8, y8, first, 8, 0, N * 8),
        "slices = 65536": lambda: _tn(x8, y8, first, 8, 65536, N * 8),
        "an empty slice": lambda: _tn(x8.repeat(2, 1)[:65], y8.repeat(2, 1)[:65], first, 8, 3, N * 8),
        "M = 0": lambda: _tn(x8, y8, first, 8, 1, 0, M=0),
    }
    for what, call in calls.items():
        with pytest.raises(Err):
            call()
        torch.cuda.synchronize()
        assert _untouched(c), what
    # the same calls inside the contract are taken
    _tn(x8.repeat(2, 1)[:65], y8.repeat(2, 1)[:65], first, 8, 2, N * 8)
    torch.cuda.synchronize()
    assert torch.equal(c.view(-1)[:2 * N * 8].cpu(), torch.cat([torch.full((64,), 64.0), torch.full((64,), 1.0)]))
