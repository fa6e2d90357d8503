"""The leading-dimension contract of include/m324.h ("matrices are row-major; `ld*` are leading dimensions in ELEMENTS") for the
GEMM, attention and row kernels: every operand is a view strictly inside a larger allocation, with `ld` and the column offset at
the minimum the entry point's own validation allows.

  inputs   sit in POISON (NaN; byte 0x7F with scale 0xFF for MX operands): a pad value that reaches an accumulator makes the
           result NaN;
  outputs  sit in a SENTINEL bit pattern no kernel produces: after the call everything outside the window must still hold it,
           bit for bit (compared through an integer view of the storage).

Every strided call is compared with the same call on contiguous operands -- same plan string (m324_gemm_plan /
m324_attention_plan), same bits -- and with the fp64 reference of the operation under the bound the kernel's own test in
test_kernels_gpu.py / test_backward_gpu.py / test_mx_kernels_gpu.py uses.  The two helper self-tests at the top run on the CPU."""
import math

import numpy as np
import pytest
import torch

import error_bounds as eb
from conftest import rel_err, vt_layout
from test_kernels_gpu import TOL, _attn_ref, _block_table, _folded, _ln_ref
from test_mx_kernels_gpu import _int_operands, _quant_input, deq, mx_quant_ref

gpu = pytest.mark.gpu
DEV = "cuda"
DT = [torch.float32, torch.bfloat16]
F32, BF = torch.float32, torch.bfloat16
NAN = float("nan")

# fill bit patterns, per element of the storage's integer view
POISON = {F32: 0x7FC00000, BF: 0x7FC0, torch.uint8: 0x7F}           # quiet NaN; e4m3 NaN
POISON_SCALE = 0xFF                                                 # E8M0 NaN
SENTINEL = {F32: 0xCB5A5A5A, BF: 0xCB5A, torch.uint8: 0xA5}         # -1.4e7: nothing here computes it; 0xA5 for MX bytes
_INT = {F32: torch.int32, BF: torch.int16, torch.uint8: torch.uint8}


# ------------------------------------------------------------------------------------------- the helper
def _bits(t):
    return t.view(_INT[t.dtype])


def _signed(fill, dtype):
    """the bit pattern `fill` as a value of the integer dtype behind `dtype`"""
    if dtype == torch.uint8:
        return fill
    n = 8 * torch.empty((), dtype=dtype).element_size()
    return fill - (1 << n) if fill >= 1 << (n - 1) else fill


def embedded(t, ld, col0, fill, rows_before=1, rows_after=1):
    """A [rows_before + R + rows_after, ld] allocation on t's device, every element the bit pattern `fill`, with t [R, C] copied
    into the window [rows_before : rows_before + R, col0 : col0 + C].  Returns (view of the window, the whole allocation): the view
    has the stride `ld`, starts col0 elements into a row and lies strictly inside the allocation -- at least one full filled
    row in front and behind, ld - C pad columns between consecutive rows."""
    R, C = t.shape
    assert rows_before >= 1 and rows_after >= 1 and col0 >= 0 and col0 + C <= ld and ld > C, (t.shape, ld, col0)
    whole = torch.full((rows_before + R + rows_after, ld), _signed(fill, t.dtype), dtype=_INT[t.dtype], device=t.device).view(t.dtype)
    view = whole[rows_before:rows_before + R, col0:col0 + C]
    view.copy_(t)
    return view, whole


def window(view, whole):
    """(first row, first column, rows, columns) of `view` inside `whole`"""
    off = view.storage_offset() - whole.storage_offset()
    return off // whole.stride(0), off % whole.stride(0), view.shape[0], view.shape[1]


def sentinel_violations(view, whole, fill):
    """[n, 2] (row, column) in `whole` of the elements OUTSIDE the window that no longer hold `fill` (bit comparison)"""
    r0, c0, R, C = window(view, whole)
    bad = _bits(whole) != _signed(fill, whole.dtype)
    bad[r0:r0 + R, c0:c0 + C] = False
    return bad.nonzero()


def assert_sentinel(view, whole, fill, what):
    bad = sentinel_violations(view, whole, fill)
    r0, c0, R, C = window(view, whole)
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} elements outside the window rows {r0}..{r0 + R - 1}, columns {c0}..{c0 + C - 1} "
                               f"of a [{whole.shape[0]}, {whole.shape[1]}] allocation were written; first (row, column): {bad[:8].tolist()}")


def test_embedded_gives_the_stride_offset_and_alignment_asked_for():
    for dtype, C, ld, col0, before, after in ((BF, 192, 200, 8, 1, 1), (F32, 260, 264, 4, 1, 1), (BF, 52, 56, 1, 2, 3), (torch.uint8, 8, 12, 4, 1, 1)):
        R = 5
        t = (torch.arange(R * C) % 97).reshape(R, C).to(dtype)
        view, whole = embedded(t, ld, col0, SENTINEL[dtype], before, after)
        esz = t.element_size()
        assert view.shape == t.shape and view.stride() == (ld, 1) and whole.shape == (before + R + after, ld) and whole.is_contiguous()
        assert window(view, whole) == (before, col0, R, C)
        assert view.data_ptr() - whole.data_ptr() == (before * ld + col0) * esz
        # strictly inside: a full row in front, a full row behind
        assert view.data_ptr() >= whole.data_ptr() + ld * esz
        assert view.data_ptr() + ((R - 1) * ld + C) * esz <= whole.data_ptr() + (before + R) * ld * esz
        assert whole.data_ptr() % 16 == 0                      # the allocator's alignment: the view's is (before * ld + col0) * esz on top of it
        assert torch.equal(view, t)
        outside = torch.ones(whole.shape, dtype=torch.bool)
        outside[before:before + R, col0:col0 + C] = False
        assert bool((_bits(whole)[outside] == _signed(SENTINEL[dtype], dtype)).all()) and int(outside.sum()) == whole.numel() - R * C
        assert sentinel_violations(view, whole, SENTINEL[dtype]).shape[0] == 0
    # the bf16 GEMM operand layout: rows 16-byte but not 128-byte aligned
    view, whole = embedded(torch.zeros((4, 192), dtype=BF), 200, 8, POISON[BF])
    rows = [view.data_ptr() + r * 200 * 2 for r in range(4)]
    assert all(p % 16 == 0 for p in rows) and any(p % 128 for p in rows)
    assert bool(torch.isnan(whole[0].float()).all()) and bool(torch.isnan(whole[1, :8].float()).all())     # the poison is a NaN
    view, whole = embedded(torch.zeros((4, 52), dtype=BF), 56, 1, SENTINEL[BF])                           # one element into a row
    assert view.data_ptr() % 4 == 2
    assert float(whole[0, 0]) < -1e7 and float(embedded(torch.zeros((1, 4)), 8, 4, SENTINEL[F32])[1][0, 0]) < -1e7


def test_sentinel_check_notices_one_changed_element_in_the_pad_and_in_the_rows_around():
    for dtype in (F32, BF, torch.uint8):
        t = torch.ones((6, 8), dtype=dtype)
        fill = SENTINEL[dtype]
        for r, c in ((1, 3), (1, 12), (3, 0), (6, 15), (0, 5), (0, 0), (7, 9), (7, 15)):    # pads left / right, the row in front, the row behind
            view, whole = embedded(t, 16, 4, fill)
            assert_sentinel(view, whole, fill, "untouched")
            view.fill_(3)                                          # writes inside the window are the kernel's business
            view[5, 7] = 0
            assert_sentinel(view, whole, fill, "window written")
            _bits(whole)[r, c] ^= 1                                # one bit of one element outside
            bad = sentinel_violations(view, whole, fill)
            assert bad.tolist() == [[r, c]]
            with pytest.raises(AssertionError, match="outside the window"):
                assert_sentinel(view, whole, fill, "changed")
    # a NaN sentinel would compare unequal to itself as a float: the check is on the bits
    view, whole = embedded(torch.zeros((2, 4)), 8, 4, POISON[F32])
    assert sentinel_violations(view, whole, POISON[F32]).shape[0] == 0


# ------------------------------------------------------------------------------------------- harness of the GPU tests
def _ops():
    from motion324_amd import ops
    return ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def _q(t, dtype):
    return t.to(dtype).to(torch.float32)


def _dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _gelu(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))


def _plan(ops, a, w, out, **kw):
    """the plan string(s) of the launch ops.gemm makes for this call (m324_gemm_plan, through the timing label)"""
    from motion324_amd import timing
    with timing.Recorder() as rec:
        ops.gemm(a, w, out, **kw)
    return " ".join(item[5] for item in rec.items)


_IN_PAD = {F32: (4, 4), BF: (8, 8), torch.uint8: (16, 16)}          # (ld - C, col0): 16-byte rows, nothing more
_OUT_PAD = {F32: (4, 4), BF: (4, 4), torch.uint8: (8, 8)}           # what the vectorised epilogues ask for: 4 elements


class Lay:
    """Operand factory of one run of a case: contiguous copies (strided=False) or views embedded in poison / sentinel."""

    def __init__(self, strided):
        self.strided, self.outs = strided, []

    def inp(self, t, pad=None, col0=None, fill=None):
        if not self.strided:
            return t.clone()
        p, c = _IN_PAD[t.dtype]
        return embedded(t, t.shape[1] + (p if pad is None else pad), c if col0 is None else col0, POISON[t.dtype] if fill is None else fill)[0]

    def out(self, t, pad=None, col0=None, name="out"):
        if not self.strided:
            return t.clone()
        p, c = _OUT_PAD[t.dtype]
        view, whole = embedded(t, t.shape[1] + (p if pad is None else pad), c if col0 is None else col0, SENTINEL[t.dtype])
        self.outs.append((view, whole, name))
        return view

    def check(self):
        for view, whole, name in self.outs:
            assert_sentinel(view, whole, SENTINEL[whole.dtype], name)


def _no_nan(t, what):
    if t.dtype != torch.uint8:
        assert not bool(torch.isnan(t.float()).any()), f"{what}: NaN in the result (poison read, or an element never written)"


def _both(case, what, nan_ok=()):
    """case(lay) -> (plan, {name: result}) once on contiguous operands and once on embedded views: same plan, same bits, no
    NaN, sentinel intact around every output.  Returns (plan, results of the strided run)."""
    lc, ls = Lay(False), Lay(True)
    pc, rc = case(lc)
    ps, rs = case(ls)
    torch.cuda.synchronize()
    assert ps == pc, f"{what}: strided plan {ps!r} != contiguous plan {pc!r}"
    for k in rc:
        if k not in nan_ok:
            _no_nan(rs[k], f"{what}: {k}")
        assert rs[k].shape == rc[k].shape and torch.equal(_bits(rs[k].contiguous()), _bits(rc[k].contiguous())), \
            f"{what}: {k} differs from the contiguous call ({int((_bits(rs[k].contiguous()) != _bits(rc[k].contiguous())).sum())} elements)"
    ls.check()
    return ps, rs


_LOGGED = set()


def _log(key, plan):
    if key not in _LOGGED:
        _LOGGED.add(key)
        print(f"[strides] {key}: {plan}")


# ------------------------------------------------------------------------------------------- m324_gemm, forced schedules
SCHEDULES = ["v1", "v2", "v5", "v10", "v11", "v12", "v13"]
MNK = (513, 260, 192)        # three row tiles of 256 (the last a single row), one column tile + 4; the same raggedness at 128


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("variant", SCHEDULES)
def test_gemm_strided_operands_every_schedule(tune, variant, dtype):
    """A [M, lda], W [N, ldw != lda], C [*, ldc], residual [res_rows, ldr != ldc]: bias + GELU into the operand dtype; gamma + broadcast
    residual + row map into fp32; the in-place residual update of an fp32 x and of the bf16 stream."""
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    tune("M324_GEMM", variant)
    M, N, K = MNK
    a, w = _q(_rand((M, K), 11), dtype), _q(_rand((N, K), 12, 0.1), dtype)
    bias, gamma, res = _rand((N,), 13), 1 + 0.1 * _rand((N,), 14), _rand((M // 3, N), 15)
    ad, wd, bd, gd = _dev(a, dtype), _dev(w, dtype), _dev(bias), _dev(gamma)
    wpad = (16, 8) if dtype == BF else (8, 4)                      # ldw != lda
    v = a.double() @ w.double().T + bias.double()
    g = _gelu(v)

    # bf16 outputs twice: ldc = N + 4 with C 8-byte aligned (the 4-column epilogue), and the same ldc (a multiple of 8) with C at the
    # start of its rows, 16-byte aligned, where interior tiles take the 8-column epilogue
    for opad in ((4, 4), (4, 0)) if dtype == BF else ((4, 4),):
        def gelu_case(lay):
            out = lay.out(torch.full((M, N), NAN, dtype=dtype, device=DEV), *opad)
            return _plan(ops, lay.inp(ad), lay.inp(wd, *wpad), out, bias=bd, act=ACT_GELU), {"out": out}
        plan, r = _both(gelu_case, f"{variant} bias + gelu, out layout {opad}")
        _log(f"{variant} {dtype}", plan)
        assert rel_err(r["out"].float(), g) < TOL[dtype]
        if dtype == BF:
            eb.assert_within(r["out"], g, eb.gemm(a, w, z=v, bias=bias, act=True), f"{variant} bias + gelu, strided {opad}")

    gin, gout, off = M // 3, M // 3 + 3, 2
    rows = torch.arange(M)
    dst = (rows // gin) * gout + rows % gin + off

    def remap_case(lay):
        out = lay.out(torch.zeros((3 * gout, N), dtype=F32, device=DEV))
        resd = lay.inp(_dev(res), 8, 4)                             # ldr = N + 8 != ldc = N + 4
        return _plan(ops, lay.inp(ad), lay.inp(wd, *wpad), out, bias=bd, gamma=gd, residual=resd, res_rows=gin, row_map=(gin, gout, off)), {"out": out}
    _, r = _both(remap_case, f"{variant} gamma + residual + row map")
    ref = torch.zeros(3 * gout, N, dtype=torch.float64)
    ref[dst] = v * gamma.double() + res.double().repeat(3, 1)
    assert rel_err(r["out"], ref) < 2e-5
    mask = torch.ones(3 * gout, dtype=torch.bool)
    mask[dst] = False
    assert float(r["out"].cpu()[mask].abs().max()) == 0.0           # rows no input row maps to stay as they were

    x0 = _rand((M, N), 16)

    def inplace_case(lay):
        x = lay.out(_dev(x0))
        return _plan(ops, lay.inp(ad), lay.inp(wd, *wpad), x, residual=x), {"x": x}
    _, r = _both(inplace_case, f"{variant} in place, fp32 x")
    assert rel_err(r["x"], x0.double() + a.double() @ w.double().T) < 1e-5

    if dtype == BF:                                                 # x += A W^T + b with x the bf16 output itself
        xb0 = _q(_rand((M, N), 17), BF)

        # the residual operand of the vectorised epilogue is 16-byte aligned: N + 8 + 4 elements in (ldc % 8 == 4: the 4-column
        # epilogue) and N + 12 + 8 elements in (ldc % 8 == 0: the 8-column one on interior tiles)
        for opad in ((8, 4), (12, 8)):
            def stream_case(lay):
                x = lay.out(_dev(xb0, BF), *opad)
                return _plan(ops, lay.inp(ad), lay.inp(wd, *wpad), x, bias=bd, residual=x), {"x": x}
            _, r = _both(stream_case, f"{variant} in place, bf16 stream, layout {opad}")
            assert rel_err(r["x"].float(), v + xb0.double()) < 4e-3
            eb.assert_within(r["x"], v + xb0.double(), eb.gemm(a, w, z=v, bias=bias, residual=xb0), f"{variant} bf16 stream in place, strided {opad}")


@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("variant", ["v0", "v2", "v5", "v10", "v11", "v12", "v13"])
def test_gemm_strided_training_aux_operand(tune, variant, dtype):
    """preact_out, gelu_grad_of, gelu_grad_out, mul_by: aux [M, ldaux] with ldaux != ldc (and != lda, ldw)."""
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    if variant != "v0":
        tune("M324_GEMM", variant)
    M, N, K = MNK
    a, w = _q(_rand((M, K), 31), dtype), _q(_rand((N, K), 32, 0.1), dtype)
    bias = _rand((N,), 33)
    dy = _q(_rand((M, K), 34), dtype)
    ad, wd, bd, dyd = _dev(a, dtype), _dev(w, dtype), _dev(bias), _dev(dy, dtype)
    zref = a.double() @ w.double().T + bias.double()
    gref = _gelu(zref)

    def empty():
        return torch.full((M, N), NAN, dtype=dtype, device=DEV)

    def preact(lay):
        g, z = lay.out(empty()), lay.out(empty(), 12, 8, name="preact_out")     # ldaux = N + 12, ldc = N + 4
        return _plan(ops, lay.inp(ad), lay.inp(wd), g, bias=bd, act=ACT_GELU, preact_out=z), {"g": g, "z": z}
    plan, r = _both(preact, f"{variant} preact_out")
    _log(f"{variant} {dtype} aux", plan)
    z, g = r["z"].contiguous(), r["g"].contiguous()
    assert rel_err(z.float(), zref) < TOL[dtype] and rel_err(g.float(), gref) < TOL[dtype]
    if dtype == BF:
        eb.assert_within(z, zref, eb.gemm(a, w, z=zref, bias=bias), "stored pre-activation, strided")
        eb.assert_within(g, gref, eb.gemm(a, w, z=zref, bias=bias, act=True), "gelu next to the stored pre-activation, strided")

    zs = z.float().cpu().double()
    dref = (dy.double() @ w.double().T) * eb.gelu_grad(zs)

    def grad_of(lay):
        dz = lay.out(empty())
        return _plan(ops, lay.inp(dyd), lay.inp(wd), dz, gelu_grad_of=lay.inp(z, 8, 4)), {"dz": dz}
    _, r = _both(grad_of, f"{variant} gelu_grad_of")
    assert rel_err(r["dz"].float(), dref) < TOL[dtype]
    if dtype == BF:
        eb.assert_within(r["dz"], dref, eb.gemm_mul_gelu_grad(dy, w, zs), "product with gelu' of the stored pre-activation, strided")

    def grad_out(lay):
        g2, d = lay.out(empty()), lay.out(empty(), 8, 8, name="gelu_grad_out")
        return _plan(ops, lay.inp(ad), lay.inp(wd), g2, bias=bd, act=ACT_GELU, gelu_grad_out=d), {"g": g2, "d": d}
    _, r = _both(grad_out, f"{variant} gelu_grad_out")
    d = r["d"].contiguous()
    assert torch.equal(r["g"].contiguous(), g)
    assert rel_err(d.float(), eb.gelu_grad(zref)) < TOL[dtype]
    if dtype == BF:
        eb.assert_within(d, eb.gelu_grad(zref), eb.gemm_gelu_grad_store(a, w, z=zref, bias=bias), "stored gelu'(z), strided")

    def mul(lay):
        dz = lay.out(empty())
        return _plan(ops, lay.inp(dyd), lay.inp(wd), dz, mul_by=lay.inp(d, 12, 4)), {"dz": dz}
    _, r = _both(mul, f"{variant} mul_by")
    mref = (dy.double() @ w.double().T) * d.float().cpu().double()
    assert rel_err(r["dz"].float(), mref) < TOL[dtype]
    if dtype == BF:
        eb.assert_within(r["dz"], mref, eb.gemm(dy, w, gamma=d.float().cpu().double()), "product with the stored gelu'(z), strided")


@gpu
@pytest.mark.parametrize("variant", ["v2", "v10", "v11", "v12", "v13"])
def test_gemm_strided_ln_fold_producer(tune, variant):
    """fp32 x = residual + A W^T + b with its per-block row statistics and the bf16 twin [M, ln_ldcopy]: ldc, ldr and ln_ldcopy all
    different."""
    ops = _ops()
    tune("M324_GEMM", variant)
    M, N, K = 513, 320, 192
    a, w = _q(_rand((M, K), 201), BF), _q(_rand((N, K), 202, 0.1), BF)
    bias, res = _rand((N,), 203), _rand((M, N), 204)
    res[::7] += 30.0
    ad, wd = _dev(a, BF), _dev(w, BF)
    exact = a.double() @ w.double().T + bias.double() + res.double()

    def case(lay):
        out = lay.out(torch.full((M, N), NAN, device=DEV))                                       # ldc = N + 4
        copy = lay.out(torch.full((M, N), NAN, dtype=BF, device=DEV), 12, 4, name="copy_out")      # ln_ldcopy = N + 12
        part = torch.full((N // 64, M, 2), NAN, device=DEV)
        plan = _plan(ops, lay.inp(ad), lay.inp(wd, 16, 8), out, bias=_dev(bias), residual=lay.inp(_dev(res), 8, 4), stats_out=part, copy_out=copy)
        return plan, {"out": out, "copy": copy, "part": part.reshape(-1, 2)}
    plan, r = _both(case, f"{variant} fold producer")
    _log(f"{variant} fold producer", plan)
    assert rel_err(r["out"], exact) < 1e-5
    assert torch.equal(r["copy"].cpu(), r["out"].cpu().to(BF))
    p = r["part"].reshape(N // 64, M, 2).double().cpu()
    blocks = exact.reshape(M, N // 64, 64)
    assert torch.allclose(p[..., 0].T, blocks.sum(-1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(p[..., 1].T, ((blocks - blocks.mean(-1, keepdim=True)) ** 2).sum(-1), rtol=1e-4, atol=1e-4)


@gpu
@pytest.mark.parametrize("variant", ["v2", "v10", "v11", "v12", "v13"])
def test_gemm_strided_ln_fold_consumer(tune, variant):
    """A = the raw bf16 stream as a strided view, with the merged statistics table and with the producer's block table."""
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    tune("M324_GEMM", variant)
    M, N, K = 513, 320, 256
    x = _rand((M, K), 321)
    x[::7] += 5.0
    xb = x.to(BF)
    lnw, lnb = 1 + 0.2 * _rand((K,), 322), 0.1 * _rand((K,), 323)
    w, b = _rand((N, K), 324, 0.05), _rand((N,), 325)
    wf, colsum, bias = _folded(lnw, lnb, w, b)
    part = _block_table(xb).to(DEV)
    stat = torch.empty((M, 2), device=DEV)
    ops.rowstats_finish(part, 1e-5, stat)
    ref = _gelu(_ln_ref(xb.float(), lnw, lnb, 1e-5) @ w.double().T + b.double())
    outs = []
    for name, ln in (("merged table", (stat, colsum.to(DEV))), ("block table", (part, colsum.to(DEV), 1e-5))):
        def case(lay):
            out = lay.out(torch.full((M, N), NAN, dtype=BF, device=DEV))
            return _plan(ops, lay.inp(_dev(xb)), lay.inp(_dev(wf), 16, 8), out, bias=_dev(bias), act=ACT_GELU, ln=ln), {"out": out}
        plan, r = _both(case, f"{variant} fold consumer, {name}")
        _log(f"{variant} fold consumer, {name}", plan)
        outs.append(r["out"].float().cpu())
        assert rel_err(outs[-1], ref) < 5e-3
    assert rel_err(outs[1], outs[0]) < 2e-4
    st = stat.double().cpu()
    zf = st[:, :1] * (xb.double() @ wf.double().T) + st[:, 1:2] * colsum.double() + bias.double()
    eb.assert_within(outs[0], eb.gelu(zf), eb.gemm(xb, wf, z=zf, bias=bias, fold=(st[:, 0], st[:, 1], colsum), act=True),
                     "consumer epilogue on the merged table, strided A")


def _heads_ref(y, i, C, B, L, H, nw, sc):
    r = y[:, i * C:(i + 1) * C].reshape(B, L, H, 64).permute(0, 2, 1, 3)
    if nw is not None:
        r = r * torch.rsqrt((r * r).mean(-1, keepdim=True) + 1e-5) * nw.double() * sc
    return r


@gpu
@pytest.mark.parametrize("variant,L,vt", [(None, 171, False), ("v2", 171, False), ("v13", 171, False), (None, 192, True), ("v2", 192, True),
                                          ("v10", 192, True), ("v11", 192, True), ("v13", 192, True)])
def test_gemm_strided_qkv_heads(tune, variant, L, vt):
    """The head-major q|k|v epilogue (plain and transposed V) reading strided A and W."""
    ops = _ops()
    if variant:
        tune("M324_GEMM", variant)
    B, H, K = 3, 2, 192
    C, M = H * 64, B * L
    x, w = _q(_rand((M, K), 91), BF), _q(_rand((3 * C, K), 92, 0.1), BF)
    b, qw, kw = _rand((3 * C,), 93), 1 + 0.1 * _rand((64,), 94), 1 + 0.1 * _rand((64,), 95)

    def case(lay):
        Q, Kk = (torch.full((B, H, L, 64), NAN, dtype=BF, device=DEV) for _ in range(2))
        V = torch.full((B, H, 64, L) if vt else (B, H, L, 64), NAN, dtype=BF, device=DEV)
        plan = _plan(ops, lay.inp(_dev(x, BF)), lay.inp(_dev(w, BF), 16, 8), None, bias=_dev(b),
                     qkv_heads=(Q, Kk, V, _dev(qw), _dev(kw), 1e-5, ops.Q_PRESCALE, L, H))
        return plan, {"Q": Q.reshape(-1, 64), "K": Kk.reshape(-1, 64), "V": V.reshape(-1, V.shape[-1])}
    plan, r = _both(case, f"{variant} qkv heads vt={vt}")
    _log(f"{variant} qkv heads vt={vt}", plan)
    y = x.double() @ w.double().T + b.double()
    for i, (name, nw, sc) in enumerate((("Q", qw, ops.Q_PRESCALE), ("K", kw, 1.0), ("V", None, 1.0))):
        ref = _heads_ref(y, i, C, B, L, H, nw, sc)
        bound = eb.qkv_heads(x, w[i * C:(i + 1) * C], bias=b[i * C:(i + 1) * C], norm_w=nw, eps=1e-5, scale=sc).reshape(B, L, H, 64).permute(0, 2, 1, 3)
        if name == "V" and vt:
            ref, bound = vt_layout(ref), vt_layout(bound)
        got = r[name].reshape(ref.shape)
        assert rel_err(got.float(), ref) < 4e-3
        eb.assert_within(got, ref, bound, f"{name}, strided A and W")


@gpu
def test_gemm_strided_n3_head():
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    M, N, K = 513, 256, 192
    a, w = _q(_rand((M, K), 95), BF), _q(_rand((N, K), 96, 0.1), BF)
    bias, w3, b3 = _rand((N,), 97), _rand((3, N), 98, 0.2), _rand((3,), 99)

    def case(lay):
        part = torch.full((N // 64, M, 3), NAN, device=DEV)
        plan = _plan(ops, lay.inp(_dev(a, BF)), lay.inp(_dev(w, BF), 16, 8), None, bias=_dev(bias), act=ACT_GELU, n3=(_dev(w3), part))
        out = torch.empty((M, 3), device=DEV)
        ops.n3_finish(part, _dev(b3), out)
        return plan, {"part": part.reshape(-1, 3), "out": out}
    plan, r = _both(case, "n3 head")
    _log("n3 head", plan)
    v = a.double() @ w.double().T + bias.double()
    ref = _gelu(v) @ w3.double().T + b3.double()
    assert rel_err(r["out"], ref) < 2e-3
    eb.assert_within(r["out"], ref, eb.n3_head(a, w, bias, w3, b3, z=v), "fused n3 head, strided A and W")


@gpu
def test_gemm_pair_strided_a_in_both_halves():
    """m324_gemm_pair (the decoder's q and k|v projections in one launch) with both A operands strided: the pair must still be the
    one launch on the 128 x 128 chunk ring, with the bits of the contiguous pair."""
    ops = _ops()
    H, Lq, T, Lk, K = 2, 513, 3, 64, 192
    C = H * 64
    xq, xkv = _q(_rand((Lq, K), 401), BF), _q(_rand((T * Lk, K), 402), BF)
    wq, wkv = _q(_rand((C, K), 403, 0.1), BF), _q(_rand((2 * C, K), 404, 0.1), BF)
    bq, bkv = _rand((C,), 405, 0.1), _rand((2 * C,), 406, 0.1)
    qw, kw = 1 + 0.1 * _rand((64,), 407), 1 + 0.1 * _rand((64,), 408)

    def case(lay):
        from motion324_amd import timing
        Q = torch.full((1, H, Lq, 64), NAN, dtype=BF, device=DEV)
        Kk = torch.full((T, H, Lk, 64), NAN, dtype=BF, device=DEV)
        Vt = torch.full((T, H, 64, Lk), NAN, dtype=BF, device=DEV)
        pair = []
        ops.gemm(lay.inp(_dev(xq, BF)), lay.inp(_dev(wq, BF)), None, bias=_dev(bq), qkv_heads=(Q, None, None, _dev(qw), None, 1e-5, ops.Q_PRESCALE, Lq, H), defer=pair)
        ops.gemm(lay.inp(_dev(xkv, BF), 16, 8), lay.inp(_dev(wkv, BF), 24, 8), None, bias=_dev(bkv), qkv_heads=(None, Kk, Vt, None, _dev(kw), 1e-5, 1.0, Lk, H, True), defer=pair)
        plans = " + ".join(ops._gemm_plan(p[0]) for p in pair)
        with timing.Recorder() as rec:
            ops.gemm_pair(pair)
        return plans + " | " + " ".join(i[5] for i in rec.items), {"Q": Q.reshape(-1, 64), "K": Kk.reshape(-1, 64), "Vt": Vt.reshape(-1, Lk)}
    plan, r = _both(case, "gemm_pair")
    _log("gemm_pair", plan)
    assert plan.count("gemm_ring2_kernel") == 2 and plan.count("gemm_ring2_pair_kernel") == 1, plan          # ONE launch, no fallback pair
    yq = xq.double() @ wq.double().T + bq.double()
    ykv = xkv.double() @ wkv.double().T + bkv.double()
    for name, y, i, B, L, wm, bv, nw, sc in (("Q", yq, 0, 1, Lq, wq, bq, qw, ops.Q_PRESCALE), ("K", ykv, 0, T, Lk, wkv[:C], bkv[:C], kw, 1.0),
                                             ("Vt", ykv, 1, T, Lk, wkv[C:], bkv[C:], None, 1.0)):
        ref = _heads_ref(y, i, C, B, L, H, nw, sc)
        bound = eb.qkv_heads(xq if name == "Q" else xkv, wm, bias=bv, norm_w=nw, eps=1e-5, scale=sc).reshape(B, L, H, 64).permute(0, 2, 1, 3)
        if name == "Vt":
            ref, bound = vt_layout(ref), vt_layout(bound)
        got = r[name].reshape(ref.shape)
        assert rel_err(got.float(), ref) < 4e-3
        eb.assert_within(got, ref, bound, f"pair {name}, strided A")


@gpu
@pytest.mark.parametrize("M,N,K", [(37, 200, 64), (64, 264, 448)])
def test_gemm_strided_skinny_rows(M, N, K):
    """The split-K-over-waves kernel (M <= 64, bf16): strided A / W / out / residual, bf16 and fp32 out."""
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    a, w = _q(_rand((M, K), 21), BF), _q(_rand((N, K), 22, 0.05), BF)
    bias, gamma, res = _rand((N,), 23), 1 + 0.1 * _rand((N,), 24), _rand((M, N), 25)
    ad, wd = _dev(a, BF), _dev(w, BF)
    v = a.double() @ w.double().T + bias.double()

    def gelu_case(lay):
        out = lay.out(torch.full((M, N), NAN, dtype=BF, device=DEV))
        return _plan(ops, lay.inp(ad), lay.inp(wd, 16, 8), out, bias=_dev(bias), act=ACT_GELU), {"out": out}
    plan, r = _both(gelu_case, "skinny bias + gelu")
    _log(f"skinny {M}x{N}x{K}", plan)
    assert "gemm_skinny_kernel" in plan
    assert rel_err(r["out"].float(), _gelu(v)) < TOL[BF]
    eb.assert_within(r["out"], _gelu(v), eb.gemm(a, w, z=v, bias=bias, act=True), "skinny bias + gelu, strided")

    def f32_case(lay):
        out = lay.out(torch.zeros((M + 3, N), device=DEV))
        plan = _plan(ops, lay.inp(ad), lay.inp(wd, 16, 8), out, bias=_dev(bias), gamma=_dev(gamma), residual=lay.inp(_dev(res), 8, 4), row_map=(M, M, 3))
        return plan, {"out": out}
    plan, r = _both(f32_case, "skinny fp32 out")
    assert "gemm_skinny_kernel" in plan
    assert rel_err(r["out"][3:], v * gamma.double() + res.double()) < 2e-5
    assert float(r["out"][:3].abs().max()) == 0.0

    def inplace_case(lay):
        x = lay.out(_dev(res))
        return _plan(ops, lay.inp(ad), lay.inp(wd, 16, 8), x, residual=x), {"x": x}
    plan, r = _both(inplace_case, "skinny in place")
    assert "gemm_skinny_kernel" in plan
    assert rel_err(r["x"], res.double() + a.double() @ w.double().T) < 1e-5


@gpu
@pytest.mark.parametrize("M,N", [(200, 128), (1000, 256)])
@pytest.mark.parametrize("mode", ["bias", "gelu", "fold", "fold_gelu"])
def test_gemm_v15_strided(tune, M, N, mode):
    """The hand-placed K = 768 stream with lda = 776, ldw = 784, ldc = N + 8 and the out view 8 columns into its rows: the bits of
    v2 on the same strided operands and of v15 on contiguous ones."""
    ops = _ops()
    from motion324_amd.lib import ACT_GELU, ACT_NONE
    K = 768
    a, w = _q(_rand((M, K), 71), BF), _q(_rand((N, K), 72, 0.03), BF)
    bias = _rand((N,), 73)
    rowstat = torch.stack([torch.rand(M, generator=torch.Generator().manual_seed(75)) + 0.5, 0.1 * _rand((M,), 76)], dim=1).contiguous()
    colsum = _rand((N,), 74)
    kw = dict(bias=_dev(bias), act=ACT_GELU if "gelu" in mode else ACT_NONE, ln=(_dev(rowstat), _dev(colsum)) if "fold" in mode else None)

    def case(lay):
        out = lay.out(torch.full((M, N), NAN, dtype=BF, device=DEV), 8, 8)
        return _plan(ops, lay.inp(_dev(a, BF), 8, 8), lay.inp(_dev(w, BF), 16, 8), out, **kw), {"out": out}
    tune("M324_GEMM", "v2")
    plan2, r2 = _both(case, f"v2 {mode}")
    tune("M324_GEMM", "v15")
    plan, r = _both(case, f"v15 {mode}")
    _log(f"v15 {mode} {M}x{N}", plan)
    assert "gemm_hp_kernel" in plan and "gemm_glds_kernel" in plan2
    assert torch.equal(r["out"], r2["out"])
    v = a.double() @ w.double().T
    if "fold" in mode:
        v = rowstat[:, :1].double() * v + rowstat[:, 1:2].double() * colsum.double()
    v = v + bias.double()
    bound = eb.gemm(a, w, z=v, bias=bias, fold=(rowstat[:, 0], rowstat[:, 1], colsum) if "fold" in mode else None, act="gelu" in mode)
    if "gelu" in mode:
        v = _gelu(v)
    assert rel_err(r["out"].float(), v) < TOL[BF]
    eb.assert_within(r["out"], v, bound, f"v15 {mode}, strided")


# ------------------------------------------------------------------------------------------- automatic fallback to v1
@gpu
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("why,M,N,K,pad,col0", [("N = 50", 130, 50, 128, 3, 1), ("ldc = N + 1", 130, 52, 128, 1, 0),
                                                ("C one element into a row", 130, 52, 128, 4, 1), ("M <= 64, N = 50", 37, 50, 64, 3, 1)])
def test_gemm_falls_back_to_the_scalar_store_kernel_by_itself(tune, dtype, why, M, N, K, pad, col0):
    """What the vectorised epilogue cannot address (N % 4, ldc % 4, a C pointer off its vector alignment) goes to the scalar-store
    kernel without anybody forcing it -- also for M <= 64, where the skinny kernel is not eligible then.  The strided call is NOT
    forced; the contiguous call it is compared with is forced to v1 where it would be vectorisable.  The sentinel sits right
    behind every unaligned row end."""
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    a, w = _q(_rand((M, K), 111), dtype), _q(_rand((N, K), 112, 0.1), dtype)
    bias, gamma, res = _rand((N,), 113), 1 + 0.1 * _rand((N,), 114), _rand((M, N), 115)
    ad, wd = _dev(a, dtype), _dev(w, dtype)
    v = a.double() @ w.double().T + bias.double()

    def force(lay):
        # Sets the switch directly, without the fixture: it is the tune("M324_GEMM", 0) call below, made before the first case runs,
        # that registers the restore to the default after the test.  Keep that call in front of every _both().
        from motion324_amd import lib
        lib.set_tunable("M324_GEMM", 0 if lay.strided else 1)

    def gelu_case(lay):
        force(lay)
        out = lay.out(torch.full((M, N), NAN, dtype=dtype, device=DEV), pad, col0)
        return _plan(ops, lay.inp(ad), lay.inp(wd), out, bias=_dev(bias), act=ACT_GELU), {"out": out}

    def res_case(lay):
        force(lay)
        out = lay.out(torch.full((M, N), NAN, device=DEV), pad, col0)
        return _plan(ops, lay.inp(ad), lay.inp(wd), out, bias=_dev(bias), gamma=_dev(gamma), residual=lay.inp(_dev(res), 5, 2)), {"out": out}

    def inplace_case(lay):
        force(lay)
        x = lay.out(_dev(res), pad, col0)
        return _plan(ops, lay.inp(ad), lay.inp(wd), x, residual=x), {"x": x}
    tune("M324_GEMM", 0)                                            # the fixture restores the switch after the test
    plan, r = _both(gelu_case, f"fallback ({why}) bias + gelu")
    _log(f"fallback {why} {dtype}", plan)
    assert plan.startswith("gemm_kernel<"), plan
    assert rel_err(r["out"].float(), _gelu(v)) < TOL[dtype]
    if dtype == BF:
        eb.assert_within(r["out"], _gelu(v), eb.gemm(a, w, z=v, bias=bias, act=True), f"fallback ({why}) bias + gelu")
    plan, r = _both(res_case, f"fallback ({why}) gamma + residual")
    assert plan.startswith("gemm_kernel<"), plan
    assert rel_err(r["out"], v * gamma.double() + res.double()) < 2e-5
    plan, r = _both(inplace_case, f"fallback ({why}) in place")
    assert plan.startswith("gemm_kernel<"), plan
    assert rel_err(r["x"], res.double() + a.double() @ w.double().T) < 1e-5


# ------------------------------------------------------------------------------------------- MX
def _mx_in(lay, q, s, qpad, spad):
    """MX operand (numpy q, s) -> ops.MX of strided views: q rows 16-byte aligned, scale rows 4-byte aligned, lds > K / 32"""
    ops = _ops()
    qt, st = torch.from_numpy(np.ascontiguousarray(q)).to(DEV), torch.from_numpy(np.ascontiguousarray(s)).to(DEV)
    return ops.MX(lay.inp(qt, qpad, 16), lay.inp(st, spad, 4, fill=POISON_SCALE))


@gpu
def test_gemm_mx_strided_operands_exact_on_integer_operands():
    """m324_gemm_mx with lda / ldw multiples of 16 beyond K and scale rows of lds > K / 32 bytes: the bf16 output, the fp32 residual
    update of a strided x (ldr == ldc) and the MX output into a strided (q, s) pair -- every product exact, so the results are
    exact (test_gemm_mx_exact_on_integer_operands)."""
    ops = _ops()
    M, N, K = 130, 192, 256
    qa, sa = _int_operands(M, K, 1)
    qw, sw = _int_operands(N, K, 2, asym=True)
    ref = deq(qa, sa) @ deq(qw, sw).T

    def operands(lay):
        return _mx_in(lay, qa, sa, 16, 4), _mx_in(lay, qw, sw, 32, 8)

    def bf16_case(lay):
        A, W = operands(lay)
        out = lay.out(torch.full((M, N), NAN, dtype=BF, device=DEV), 8, 8)
        ops.gemm_mx(A, W, out)
        return None, {"out": out}
    _, r = _both(bf16_case, "gemm_mx bf16 out")
    refb = torch.from_numpy(ref).float().to(BF).float().numpy()
    got = r["out"].float().cpu().numpy()
    assert np.array_equal(got, refb), np.argwhere(got != refb)[:8]

    x0 = torch.from_numpy(np.random.default_rng(3).integers(-64, 65, (M, N)).astype(np.float32))

    def f32_case(lay):
        A, W = operands(lay)
        x = lay.out(_dev(x0))
        ops.gemm_mx(A, W, x, residual=x)
        return None, {"x": x}
    _, r = _both(f32_case, "gemm_mx fp32 residual update")
    assert np.array_equal(r["x"].cpu().numpy(), (ref + x0.double().numpy()).astype(np.float32))

    def mx_case(lay):
        A, W = operands(lay)
        q = lay.out(torch.full((M, N), 0x7F, dtype=torch.uint8, device=DEV), 8, 8, name="C")
        s = lay.out(torch.full((M, N // 32), 0xFF, dtype=torch.uint8, device=DEV), 3, 1, name="C_scale")
        ops.gemm_mx(A, W, ops.MX(q, s))
        return None, {"q": q, "s": s}
    _, r = _both(mx_case, "gemm_mx MX out")
    qr, sr = mx_quant_ref(ref)
    q, s = r["q"].cpu().numpy(), r["s"].cpu().numpy()
    assert np.array_equal(s, sr), np.argwhere(s != sr)[:8]
    assert np.array_equal(q, qr), np.argwhere(q != qr)[:8]


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_mx_quant_strided(dtype):
    """m324_mx_quant: strided x and a strided (q, s) pair against the numpy rule; the input holds NaN / Inf blocks on purpose."""
    ops = _ops()
    x = torch.from_numpy(_quant_input()).to(dtype)
    rows, K = x.shape

    def case(lay):
        q = lay.out(torch.zeros((rows, K), dtype=torch.uint8, device=DEV), 8, 8, name="q")
        s = lay.out(torch.zeros((rows, K // 32), dtype=torch.uint8, device=DEV), 3, 1, name="s")
        ops.mx_quant(lay.inp(_dev(x)), ops.MX(q, s))
        return None, {"q": q, "s": s}
    _, r = _both(case, "mx_quant")
    qr, sr = mx_quant_ref(x.float().numpy())
    q, s = r["q"].cpu().numpy(), r["s"].cpu().numpy()
    assert np.array_equal(s, sr), np.argwhere(s != sr)[:8]
    assert np.array_equal(q, qr), np.argwhere(q != qr)[:8]


@gpu
@pytest.mark.parametrize("rows,C", [(77, 192), (77, 768)])
def test_layernorm_mx_strided(rows, C):
    """m324_layernorm_mx on a strided x into a strided (q, s) pair: the bits of the contiguous call, and the numpy rule applied to
    m324_layernorm's fp32 output up to the rare e4m3 boundary crossing test_layernorm_mx_equals_quantised_layernorm allows."""
    ops = _ops()
    x = _rand((rows, C), 3) * 3 + 1.5
    w, b = 1 + 0.5 * _rand((C,), 4), 0.1 * _rand((C,), 5)

    def case(lay):
        q = lay.out(torch.zeros((rows, C), dtype=torch.uint8, device=DEV), 4, 4, name="q")
        s = lay.out(torch.zeros((rows, C // 32), dtype=torch.uint8, device=DEV), 3, 1, name="s")
        ops.layernorm_mx(lay.inp(_dev(x)), _dev(w), _dev(b), 1e-6, ops.MX(q, s))
        return None, {"q": q, "s": s}
    _, r = _both(case, "layernorm_mx")
    y = torch.empty((rows, C), device=DEV)
    ops.layernorm(_dev(x), _dev(w), _dev(b), 1e-6, y)
    qa, sa = mx_quant_ref(y.cpu().numpy())
    qm, sm = r["q"].cpu().numpy(), r["s"].cpu().numpy()
    assert np.array_equal(sa, sm)
    diff = qa != qm
    assert diff.mean() < 1e-3, diff.sum()
    if diff.any():
        d = np.abs(deq(qa, sa) - deq(qm, sm))[diff]
        step = np.abs(deq(qa, sa))[diff] * 2.0 ** -3 + 2.0 ** -9 * 2.0 ** (sa.repeat(32, 1)[diff].astype(float) - 127)
        assert np.all(d <= step * 1.01)


# ------------------------------------------------------------------------------------------- attention
# One smallest shape per distinct kernel name m324_attention_plan reports over the attention calls of test_kernels_gpu.py (fourteen
# names: eleven attn_bf16_kernel instantiations, the two one-wave-per-SIMD streams, the frame loop, fp32).  The last column is the
# whole name, every template argument <PS, NQ, NW, VROW, NST> included, so that a row pins ONE compiled instantiation: each of
# them stores through O + row * ldo in its own code.  M324_ATTN_NW forces the wave count at a small shape, as
# test_attention_long_sequence_schedules does; NST follows the key count (one tile: 1, 2 .. 16 tiles with a prescaled q: 2, else 3).
#            name                        dtype B  H  Lq    Lk    kwargs                                       tunable               kernel name
ATTN = [("64 keys",                      BF,  1, 2, 64,   64,   {},                                          None,                 "attn_bf16_kernel<false, 1, 4, false, 3>"),
        ("100 keys",                     BF,  2, 3, 100,  100,  {},                                          None,                 "attn_bf16_kernel<false, 1, 4, false, 3>"),
        ("row-major V",                  BF,  2, 3, 100,  100,  dict(v_rowmajor=True),                       None,                 "attn_bf16_kernel<false, 1, 4, true, 3>"),
        ("row-major V, prescaled",       BF,  2, 3, 100,  100,  dict(prescaled=True, v_rowmajor=True),       None,                 "attn_bf16_kernel<true, 1, 4, true, 2>"),
        ("row-major V, nw8",             BF,  1, 1, 1100, 192,  dict(v_rowmajor=True),                       ("M324_ATTN_NW", 8),  "attn_bf16_kernel<false, 1, 8, true, 3>"),
        ("row-major V, prescaled, nw8",  BF,  1, 1, 1100, 192,  dict(prescaled=True, v_rowmajor=True),       ("M324_ATTN_NW", 8),  "attn_bf16_kernel<true, 1, 8, true, 3>"),
        ("nw4, two stages",              BF,  1, 1, 1100, 192,  dict(prescaled=True),                        ("M324_ATTN_NW", 4),  "attn_bf16_kernel<true, 1, 4, false, 2>"),
        ("nw4, three stages",            BF,  1, 1, 200,  1100, dict(prescaled=True),                        ("M324_ATTN_NW", 4),  "attn_bf16_kernel<true, 1, 4, false, 3>"),
        ("nw8",                          BF,  1, 1, 1100, 192,  dict(prescaled=True),                        ("M324_ATTN_NW", 8),  "attn_bf16_kernel<true, 1, 8, false, 3>"),
        ("nw8, plain q",                 BF,  1, 1, 1100, 192,  {},                                          ("M324_ATTN_NW", 8),  "attn_bf16_kernel<false, 1, 8, false, 3>"),
        ("one wave / SIMD",              BF,  1, 2, 2049, 513,  dict(prescaled=True),                        None,                 "attn_pwg_kernel"),
        ("bounded",                      BF,  1, 2, 2049, 513,  dict(prescaled=True, bounded=True),          None,                 "attn_pwg_bounded_kernel"),
        ("frame loop",                   BF,  2, 2, 513,  37,   dict(prescaled=True, shared_q=True),         None,                 "attn_frames_kernel<2, true>"),
        ("shared q, one key tile",       BF,  5, 3, 200,  64,   dict(prescaled=True, shared_q=True),         None,                 "attn_bf16_kernel<true, 1, 4, false, 1>"),
        ("fp32",                         F32, 2, 3, 100,  100,  {},                                          None,                 "attn_f32_kernel")]


def test_attention_table_names_every_kernel_once_or_more():
    """the table above is what it says: whole names, and no kernel family of m324_attention_plan without a row"""
    names = {c[8] for c in ATTN}
    assert len(names) == 14 and all(n.endswith(">") or "<" not in n for n in names)
    assert {n.split("<")[0] for n in names} == {"attn_bf16_kernel", "attn_pwg_kernel", "attn_pwg_bounded_kernel", "attn_frames_kernel", "attn_f32_kernel"}


@gpu
@pytest.mark.parametrize("name,dtype,B,H,Lq,Lk,kw,tunable,kernel", ATTN, ids=[c[0].replace(", ", "-").replace(" ", "_") for c in ATTN])
def test_attention_strided_out(tune, name, dtype, B, H, Lq, Lk, kw, tunable, kernel):
    """O [B * Lq, ldo = H * 64 + 8], the view 8 columns into its rows, with lse: one smallest shape per kernel name (the whole name:
    see ATTN) that m324_attention_plan gives over the attention calls of test_kernels_gpu.py."""
    ops = _ops()
    if tunable:
        tune(*tunable)
    shared, pre = kw.get("shared_q", False), kw.get("prescaled", False)
    q, k, v = (_rand((b_, H, L, 64), s_, 1.5 if i < 2 else 1.0) for i, (b_, L, s_) in enumerate(((1 if shared else B, Lq, 19), (B, Lk, 20), (B, Lk, 21))))
    k, v = _q(k, dtype), _q(v, dtype)
    qs = _q(q * ops.Q_PRESCALE, dtype) if pre else _q(q, dtype)
    scale = math.log(2.0) if pre else 64 ** -0.5
    flags = int(pre) | (2 if kw.get("v_rowmajor") else 0) | (4 if kw.get("bounded") else 0) | (256 if shared else 0)
    plan = ops._attn_plan(B, H, Lq, Lk, flags, ops.code_of(dtype))
    _log(f"attention {name}", plan)
    assert plan.split(" grid=")[0] == kernel, plan
    dq, dk = _dev(qs, dtype), _dev(k, dtype)
    dv = _dev(v if kw.get("v_rowmajor") else vt_layout(v), dtype)

    def case(lay):
        out = lay.out(torch.full((B * Lq, H * 64), NAN, dtype=dtype, device=DEV), 8, 8)
        lse = torch.full((B, H, Lq), NAN, device=DEV)
        ops.attention(dq, dk, dv, out, lse=lse, **kw)
        return ops._attn_plan(B, H, Lq, Lk, flags, ops.code_of(dtype)), {"out": out, "lse": lse.reshape(-1, Lq)}
    _, r = _both(case, f"attention {name}")
    sc = torch.einsum("bhqd,bhkd->bhqk", qs.expand(B, -1, -1, -1).double(), k.double()) * scale
    if kw.get("bounded"):
        assert float(sc.abs().max()) / math.log(2.0) < 60.0
    ref = _attn_ref(qs.expand(B, -1, -1, -1), k, v, scale).reshape(B * Lq, H * 64)
    lse_ref = torch.logsumexp(sc, dim=-1) / math.log(2.0)
    assert rel_err(r["out"].float(), ref) < (1e-5 if dtype == F32 else 8e-3)
    got_lse = r["lse"].reshape(B, H, Lq)
    if dtype == BF:
        bound, lse_bound = eb.attention_and_lse(qs, k, v, scale)
        eb.assert_within(r["out"], ref, bound, f"attention {name}, strided out")
        eb.assert_within(got_lse, lse_ref, lse_bound, f"lse {name}")
    else:                                   # no existing test bounds the fp32 kernel's LSE: the absolute bound test_attention_shared_q_frame_loop sets
        assert float((got_lse.double().cpu() - lse_ref).abs().max()) < 2e-3


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_attention_merge_strided_parts_and_out(dtype):
    ops = _ops()
    B, H, Lq, cuts = 2, 2, 300, (0, 64, 200, 333)
    Lk = cuts[-1]
    q, k, v = (_rand((B, H, L, 64), s_, 1.2) for L, s_ in ((Lq, 261), (Lk, 262), (Lk, 263)))
    k[0, 0, cuts[1] + 3] = q[0, 0, 7] * 3.0
    k, v = _q(k, dtype), _q(v, dtype)
    qs = _q(q * ops.Q_PRESCALE, dtype)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o = torch.full((B * Lq, H * 64), NAN, dtype=dtype, device=DEV)
        lse = torch.full((B, H, Lq), NAN, device=DEV)
        ops.attention(_dev(qs, dtype), _dev(k[:, :, a:b].contiguous(), dtype), _dev(vt_layout(v[:, :, a:b]), dtype), o, prescaled=True, lse=lse)
        parts.append((o, lse))

    def case(lay):
        out = lay.out(torch.full((B * Lq, H * 64), NAN, dtype=dtype, device=DEV), 16, 8)             # ldo != ldp
        ops.attention_merge([(lay.inp(o), lse) for o, lse in parts], out, B, H, Lq)                # ldp = H * 64 + 8 (bf16) / + 4 (fp32)
        return None, {"out": out}
    _, r = _both(case, "attention_merge")
    sc = torch.einsum("bhqd,bhkd->bhqk", qs.double(), k.double())
    ref = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(sc * math.log(2.0), dim=-1), v.double()).reshape(B * Lq, H * 64)
    tol = 8e-3 if dtype == BF else 2e-5
    got = r["out"].float().cpu()
    assert rel_err(got, ref) < tol and rel_err(got[7], ref[7]) < 1.5 * tol
    if dtype == BF:
        eb.assert_within(got, ref, eb.attention_merge(qs, k, v, math.log(2.0), cuts), "merged key parts, strided")


@gpu
@pytest.mark.parametrize("dtype", DT)
def test_attention_delta_strided(dtype):
    """D = rowsum(dO * O) per head from token-major O, dO with ld = H * 64 + 8: fp32 sums of 64 exact products each."""
    ops = _ops()
    B, H, L = 2, 3, 77
    o, do = _q(_rand((B * L, H * 64), 14), dtype), _q(_rand((B * L, H * 64), 15), dtype)

    def case(lay):
        return None, {"D": ops.attention_delta(lay.inp(_dev(o, dtype), 8, 8), lay.inp(_dev(do, dtype), 8, 8), B, H, L).reshape(-1, L)}
    _, r = _both(case, "attention_delta")
    ref = (o.double() * do.double()).reshape(B, L, H, 64).sum(-1).permute(0, 2, 1)
    assert rel_err(r["D"].reshape(B, H, L), ref) < TOL[F32]


# ------------------------------------------------------------------------------------------- row kernels
ROWS = 77
WIDTHS = [192, 768]


@gpu
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("xdt,odt", [(F32, F32), (F32, BF), (BF, BF)])
def test_layernorm_strided_with_row_map(C, xdt, odt):
    ops = _ops()
    gin, gout, off = 7, 10, 2
    x = _q(_rand((ROWS // gin * gout, C), 91) * 2 + 0.3, xdt)
    w, b = 1 + 0.1 * _rand((C,), 92), _rand((C,), 93)

    def case(lay):
        out = lay.out(torch.full((ROWS, C), NAN, dtype=odt, device=DEV), 8, 4)                      # ldy = C + 8, ldx = C + 4
        ops.layernorm(lay.inp(_dev(x, xdt), 4, 4), _dev(w), _dev(b), 1e-5, out, row_map=(gin, gout, off))
        return None, {"out": out}
    _, r = _both(case, "layernorm")
    sel = x.reshape(-1, gout, C)[:, off:off + gin].reshape(-1, C)
    ref = torch.nn.functional.layer_norm(sel.double(), (C,), w.double(), b.double(), 1e-5)
    assert rel_err(r["out"].float(), ref) < (1e-6 if odt == F32 else 4e-3)
    if odt == BF:
        eb.assert_within(r["out"], ref, eb.layernorm(sel, w, b, 1e-5), "layernorm, strided")


@gpu
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("odt", DT)
def test_layernorm_pair_strided(C, odt):
    ops = _ops()
    gin, gout, off = 7, 10, 2
    x0, x1 = _rand((ROWS, C), 401) * 2 + 0.3, _rand((ROWS // gin * gout, C), 402)
    w = [1 + 0.1 * _rand((C,), 403 + i) for i in range(2)]
    b = [0.1 * _rand((C,), 405 + i) for i in range(2)]

    def case(lay):
        y0 = lay.out(torch.full((ROWS, C), NAN, dtype=odt, device=DEV), 4, 4, name="y0")
        y1 = lay.out(torch.full((ROWS, C), NAN, dtype=odt, device=DEV), 12, 8, name="y1")
        ops.layernorm_pair(lay.inp(_dev(x0), 4, 4), _dev(w[0]), _dev(b[0]), 1e-5, y0, lay.inp(_dev(x1), 8, 4), _dev(w[1]), _dev(b[1]), 1e-6, y1,
                           row_map1=(gin, gout, off))
        return None, {"y0": y0, "y1": y1}
    _, r = _both(case, "layernorm_pair")
    sel = x1.reshape(-1, gout, C)[:, off:off + gin].reshape(-1, C)
    for got, xin, i, eps in ((r["y0"], x0, 0, 1e-5), (r["y1"], sel, 1, 1e-6)):
        ref = torch.nn.functional.layer_norm(xin.double(), (C,), w[i].double(), b[i].double(), eps)
        assert rel_err(got.float(), ref) < (1e-6 if odt == F32 else 4e-3)
        if odt == BF:
            eb.assert_within(got, ref, eb.layernorm(xin, w[i], b[i], eps), f"layernorm_pair problem {i}, strided")
        # the separate launch on contiguous operands gives the same bits
        one = torch.empty((ROWS, C), dtype=odt, device=DEV)
        ops.layernorm(_dev(xin), _dev(w[i]), _dev(b[i]), eps, one)
        assert torch.equal(got.contiguous(), one)


@gpu
@pytest.mark.parametrize("C", WIDTHS)
def test_rowstats_strided_with_copy(C):
    ops = _ops()
    x = _rand((ROWS, C), 211)
    x[::5] += 12.0

    def case(lay):
        stat = torch.full((ROWS, 2), NAN, device=DEV)
        copy = lay.out(torch.full((ROWS, C), NAN, dtype=BF, device=DEV), 8, 4, name="copy")
        ops.rowstats(lay.inp(_dev(x), 4, 4), 1e-6, stat, copy)
        return None, {"stat": stat, "copy": copy}
    _, r = _both(case, "rowstats")
    rstd = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-6)
    s = r["stat"].double().cpu()
    assert torch.allclose(s[:, 0], rstd, rtol=1e-5) and torch.allclose(s[:, 1], -rstd * x.double().mean(1), rtol=1e-5, atol=1e-6)
    assert torch.equal(r["copy"].cpu(), x.to(BF))


@gpu
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", DT)
def test_layernorm_backward_strided(C, dtype):
    """m324_layernorm_bwd and m324_layernorm_bwd_cast: x [*, ldx], dy [*, ldy], dx [*, lddx] (accumulated into) and the bf16 copy
    [*, ldc], four different leading dimensions."""
    ops = _ops()
    x, w = _rand((ROWS, C), 5) * 2 + 0.3, 1 + 0.1 * _rand((C,), 6)
    dy, dx0 = _q(_rand((ROWS, C), 7), dtype), _rand((ROWS, C), 8)
    xt, wt = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bt = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xt, (C,), wt, bt, 1e-5).backward(dy.double())

    def plain(lay):
        dx = lay.out(_dev(dx0), 12, 4, name="dx")
        dw, db = ops.layernorm_bwd(lay.inp(_dev(x), 4, 4), _dev(w), 1e-5, lay.inp(_dev(dy, dtype), 8, 4), dx, accumulate=True)
        return None, {"dx": dx, "dw": dw[None], "db": db[None]}
    _, r = _both(plain, "layernorm_bwd")
    assert rel_err(r["dx"], dx0.double() + xt.grad) < 2e-6
    assert rel_err(r["dw"][0], wt.grad) < 2e-5 and rel_err(r["db"][0], bt.grad) < 2e-5

    def with_cast(lay):
        dx = lay.out(_dev(dx0), 12, 4, name="dx")
        copy = lay.out(torch.full((ROWS, C), NAN, dtype=BF, device=DEV), 16, 4, name="cast_out")
        dw, db, cs = ops.layernorm_bwd(lay.inp(_dev(x), 4, 4), _dev(w), 1e-5, lay.inp(_dev(dy, dtype), 8, 4), dx, accumulate=True, cast_out=copy)
        return None, {"dx": dx, "dw": dw[None], "db": db[None], "copy": copy, "cs": cs[None]}
    _, r2 = _both(with_cast, "layernorm_bwd_cast")
    assert torch.equal(r2["dx"], r["dx"]) and torch.equal(r2["dw"], r["dw"]) and torch.equal(r2["db"], r["db"])
    assert torch.equal(r2["copy"].contiguous(), r2["dx"].contiguous().to(BF))
    ref = r2["copy"].double().sum(0)
    assert float((r2["cs"][0].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max() + 1)


@gpu
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("src,dst", [(F32, BF), (BF, F32)])
@pytest.mark.parametrize("kernel", ["8-wide", "scalar"])
def test_cast_strided(C, src, dst, kernel):
    """m324_cast: ld % 8 == 0 and 16-byte pointers take the 8-wide kernel; a bf16 operand 4 elements (8 bytes) into its row sends
    the call to the scalar one.  Bit equality holds whichever kernel runs, so the arithmetic that selects it, from m324_cast's
    `vec` condition: both ld = C + 8 (% 8 == 0); a view starts (ld + col0) elements into a 16-byte aligned allocation, so with
    col0 = 8 both pointers are at a multiple of 16 bytes (bf16: 2 (ld + 8), fp32: 4 (ld + 8)): 8-wide.  With col0 = 4 the bf16
    side is at 2 (ld + 4) = 8 mod 16: scalar.  The fp32 side keeps col0 = 8; one misaligned operand is enough."""
    ops = _ops()
    x = _q(_rand((ROWS, C), 26), src)
    off = 8 if kernel == "8-wide" else 4

    def case(lay):
        out = lay.out(torch.full((ROWS, C), NAN, dtype=dst, device=DEV), 8, off if dst == BF else 8)
        ops.cast(lay.inp(_dev(x, src), 8, off if src == BF else 8), dst, out=out)
        return None, {"out": out}
    _, r = _both(case, f"cast {kernel}")
    assert torch.equal(r["out"].cpu(), x.to(dst))


@gpu
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dtype", DT)
def test_transpose_strided_input(C, dtype):
    ops = _ops()
    x = _q(_rand((ROWS, C), 1), dtype)

    def case(lay):
        return None, {"out": ops.transpose(lay.inp(_dev(x, dtype), 3, 1))}        # any ld_in >= cols is legal
    _, r = _both(case, "transpose")
    out = r["out"].float().cpu()
    assert out.shape == (C, 128) and torch.equal(out[:, :ROWS], x.T) and float(out[:, ROWS:].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("K", [192, 52])
@pytest.mark.parametrize("dtype", DT)
def test_linear_n3_strided_forward_and_backward(K, dtype):
    """m324_linear_n3 with a strided A; m324_linear_n3_bwd with strided A and mul_by (different leading dimensions): the 16-byte
    kernel at K = 192 and the scalar one at K = 52.  Bit equality holds whichever kernel runs, so the arithmetic that selects it, from
    m324_linear_n3_bwd's condition (K % 8 == 0, 64 <= K <= 2048, every ld and pointer at a multiple of 16 bytes), with _IN_PAD:
    fp32 a: lda = K + 4 -> 4 * 196 = 16 * 49 bytes, the view 4 * (196 + 4) = 16 * 50 bytes in; mul_by: ld = K + 8 -> 16 * 50, view
    4 * (200 + 4) = 16 * 51 in.  bf16 a: lda = K + 8 -> 2 * 200 = 16 * 25, view 2 * (200 + 8) = 16 * 26 in; mul_by: ld = K + 16 ->
    16 * 26, view 2 * (208 + 8) = 16 * 27 in.  dA is the wrapper's own contiguous [M, K].  So K = 192 takes the 16-byte kernel and
    K = 52 (52 % 8 == 4) the scalar one; a change of _IN_PAD that breaks a product above silently moves K = 192 to the scalar kernel."""
    ops = _ops()
    M = ROWS
    a, w, b = _q(_rand((M, K), 21), dtype), _rand((3, K), 22, 0.1), _rand((3,), 46)
    dout, f = _rand((M, 3), 23), _q(_rand((M, K), 24), dtype)
    pad = _IN_PAD[dtype]
    pad2 = (2 * pad[0], pad[1])

    def fwd(lay):
        out = torch.full((M, 3), NAN, device=DEV)
        ops.linear_n3(lay.inp(_dev(a, dtype), *pad), _dev(w), _dev(b), out)
        return None, {"out": out}
    _, r = _both(fwd, "linear_n3")
    assert rel_err(r["out"], a.double() @ w.double().T + b.double()) < 1e-5

    at, wt = a.double().requires_grad_(True), w.double().requires_grad_(True)
    bt = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (at @ wt.T + bt).backward(dout.double())

    def bwd(lay):
        dA, dW, db = ops.linear_n3_bwd(lay.inp(_dev(a, dtype), *pad), _dev(w), _dev(dout))
        return None, {"dA": dA, "dW": dW, "db": db[None]}
    _, r = _both(bwd, "linear_n3_bwd")
    assert rel_err(r["dA"].float(), at.grad) < (1e-6 if dtype == F32 else 5e-3)
    assert rel_err(r["dW"], wt.grad) < 1e-5 and rel_err(r["db"][0], bt.grad) < 1e-5

    def bwd_mul(lay):
        dA, dW, db = ops.linear_n3_bwd(lay.inp(_dev(a, dtype), *pad), _dev(w), _dev(dout), mul_by=lay.inp(_dev(f, dtype), *pad2))
        return None, {"dA": dA, "dW": dW, "db": db[None]}
    _, r2 = _both(bwd_mul, "linear_n3_bwd, mul_by")
    assert rel_err(r2["dA"].float(), at.grad * f.double()) < (1e-6 if dtype == F32 else 5e-3)
    assert torch.equal(r2["dW"], r["dW"]) and torch.equal(r2["db"], r["db"])
