"""Block-scaled FP8 (MX) kernels: m324_mx_quant against a numpy statement of the quantisation rule (include/m324.h, "MX
operands"), m324_gemm_mx against fp64 products of the dequantised operands, m324_layernorm_mx against m324_layernorm + the rule
and against fp64 LayerNorm within its error bound.  The reference, the operand builders and the checker (admissible sets) live
in tests/mx_cases.py; their names stay importable from here (tests/test_strides_gpu.py)."""
import math

import numpy as np
import pytest
import torch

import error_bounds
import mx_cases
from mx_cases import E4M3, _e4m3_table, _int_operands, _mx_to_np, _quant_input, _rand_mx, _rne_e4m3, _to_mx, deq, mx_quant_ref  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from motion324_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mx_quant_is_bit_identical_to_the_rule(dtype):
    ops = _ops()
    x = torch.from_numpy(_quant_input()).to(dtype)
    m = ops.mx_quant(x.to(DEV))
    q, s = _mx_to_np(m, *x.shape)
    qr, sr = mx_quant_ref(x.float().numpy())
    assert np.array_equal(s, sr), np.argwhere(s != sr)[:8]
    assert np.array_equal(q, qr), np.argwhere(q != qr)[:8]
    assert s[21, 0] == 0xFF and s[22, 1] == 0xFF and s[23, 3] == 0xFF and s[3, 1] == 0


def test_layernorm_mx_equals_quantised_layernorm():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    rows, C = 300, 768
    x = (torch.randn(rows, C, generator=g) * 3 + 1.5).to(DEV)
    w, b = (torch.randn(C, generator=g) * 0.5 + 1).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    y = torch.empty(rows, C, device=DEV)
    ops.layernorm(x, w, b, 1e-6, y)
    a = ops.mx_quant(y)
    m = ops.layernorm_mx(x, w, b, 1e-6)
    qa, sa = _mx_to_np(a, rows, C)
    qm, sm = _mx_to_np(m, rows, C)
    assert np.array_equal(sa, sm)
    # equal except where an fp32-ulp difference of the normalised value crosses an e4m3 rounding boundary
    diff = qa != qm
    assert diff.mean() < 1e-3, diff.sum()
    if diff.any():
        d = np.abs(deq(qa, sa) - deq(qm, sm))[diff]
        step = np.abs(deq(qa, sa))[diff] * 2.0 ** -3 + 2.0 ** -9 * 2.0 ** (sa.repeat(32, 1)[diff].astype(float) - 127)
        assert np.all(d <= step * 1.01)


# ---------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (200, 2304, 768), (333, 3072, 768), (130, 768, 3072), (64, 192, 128)])
def test_gemm_mx_exact_on_integer_operands(M, N, K):
    ops = _ops()
    qa, sa = _int_operands(M, K, 1)
    qw, sw = _int_operands(N, K, 2, asym=True)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), out)
    ref = deq(qa, sa) @ deq(qw, sw).T
    got = out.float().cpu().numpy()
    refb = torch.from_numpy(ref).float().to(torch.bfloat16).float().numpy()   # exact fp32 sum, rounded once to bf16
    assert np.array_equal(got, refb), np.argwhere(got != refb)[:8]


def test_gemm_mx_lane_map_single_k():
    """One non-zero k per output element pair: a wrong A/B lane map or scale byte selection moves a value to another k."""
    ops = _ops()
    M, N, K = 128, 128, 256
    qa = np.zeros((M, K), np.uint8)
    qw = np.zeros((N, K), np.uint8)
    ks = (np.arange(M) * 7) % K
    qa[np.arange(M), ks] = _rne_e4m3(np.ones(M))
    wv = (np.arange(N)[:, None] * 3 + np.arange(K)[None, :]) % 15 - 7.0
    qw[:] = _rne_e4m3(wv)
    sa = (127 + (np.arange(K // 32)[None, :] % 3) - 1 + np.zeros((M, 1), int)).astype(np.uint8)
    sw = (127 + ((np.arange(K // 32)[None, :] + np.arange(N)[:, None]) % 4) - 2).astype(np.uint8)
    out = torch.empty((M, N), dtype=torch.float32, device=DEV).zero_()
    ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), out, residual=out)
    ref = deq(qa, sa) @ deq(qw, sw).T
    assert np.array_equal(out.cpu().numpy(), ref.astype(np.float32))


def test_gemm_mx_residual_epilogue_matches_fp64():
    ops = _ops()
    M, N, K = 333, 768, 3072
    qa, sa = _rand_mx(M, K, 4)
    qw, sw = _rand_mx(N, K, 5, 0.02)
    g = torch.Generator().manual_seed(6)
    bias, gamma, res = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(M, N, generator=g)
    x = res.clone().to(DEV)
    ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), x, bias=bias.to(DEV), gamma=gamma.to(DEV), residual=x)
    prod = deq(qa, sa) @ deq(qw, sw).T
    ref = (prod + bias.double().numpy()) * gamma.double().numpy() + res.double().numpy()
    absd = np.abs(deq(qa, sa)) @ np.abs(deq(qw, sw)).T
    err = np.abs(x.cpu().double().numpy() - ref)
    # fp32 accumulation: K roundings of a running sum (<= K 2^-24 sum|a w|), then the epilogue's few roundings
    assert np.all(err <= K * 2.0 ** -24 * absd * gamma.double().numpy() + 2.0 ** -21 * (np.abs(ref) + np.abs(res.double().numpy())))


def _gelu64(z):
    return 0.5 * z * (1 + torch.special.erf(torch.from_numpy(z / math.sqrt(2))).numpy())


def test_gemm_mx_gelu_mx_output_matches_quantised_fp64():
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    M, N, K = 300, 3072, 768
    qa, sa = _rand_mx(M, K, 8)
    qw, sw = _rand_mx(N, K, 9, 0.05)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(10)) * 0.1
    out = ops.mx_empty(M, N, DEV)
    ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), out, bias=bias.to(DEV), act=ACT_GELU)
    ref = _gelu64(deq(qa, sa) @ deq(qw, sw).T + bias.double().numpy())
    qr, sr = mx_quant_ref(ref)
    q, s = _mx_to_np(out, M, N)
    # the fp32 sum and the epilogue's erf (|error| <= 1.5e-7) move a value across an e4m3 rounding boundary rarely
    assert (s != sr).mean() < 2e-3
    same = np.repeat(s == sr, 32, axis=1)
    bad = (q != qr) & same
    assert bad.mean() < 2e-3, bad.sum()
    # ... and then only where the fp64 value lies within the fp32 accumulation error (K 2^-24 sum|a w|, times GELU's slope
    # <= 1.13) of the interval the kernel's code stands for (half an e4m3 step around it); near-zero results can change sign
    absd = np.abs(deq(qa, sa)) @ np.abs(deq(qw, sw)).T
    eb = (1.13 * K * 2.0 ** -24 * absd + 1e-6)[bad]
    got = deq(q, s)[bad]
    half = np.abs(got) * 2.0 ** -4 + 2.0 ** (s.repeat(32, 1)[bad].astype(float) - 127 - 10)
    assert np.all(np.abs(got - ref[bad]) <= half + eb)


@pytest.mark.parametrize("L,vt", [(257, False), (256, True), (256, False)])
def test_gemm_mx_qkv_heads_epilogue(L, vt):
    ops = _ops()
    B, H = 3, 12
    C = H * 64
    M, N, K = B * L, 3 * C, C
    qa, sa = _rand_mx(M, K, 11)
    qw, sw = _rand_mx(N, K, 12, 0.03)
    g = torch.Generator().manual_seed(13)
    bias, qn, kn = torch.randn(N, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5, torch.rand(64, generator=g) + 0.5
    Q, Kh = (torch.empty(B, H, L, 64, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    V = torch.empty((B, H, 64, L) if vt else (B, H, L, 64), dtype=torch.bfloat16, device=DEV)
    scale = 0.18
    ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), None, bias=bias.to(DEV),
                qkv_heads=(Q, Kh, V, qn.to(DEV), kn.to(DEV), 1e-5, scale, L, H))
    p = torch.from_numpy(deq(qa, sa) @ deq(qw, sw).T + bias.double().numpy())
    heads = p.reshape(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)            # [3, B, H, L, 64]

    def rms(t, w):
        return t * torch.rsqrt((t * t).mean(-1, keepdim=True) + 1e-5) * w.double()
    qref, kref, vref = rms(heads[0], qn) * scale, rms(heads[1], kn), heads[2]
    for got, ref in ((Q, qref), (Kh, kref)):
        assert torch.allclose(got.double().cpu(), ref, rtol=2 ** -7, atol=1e-3 * float(ref.abs().max()))
    # element-wise error bounds: the operands are the DEQUANTISED values, so the bf16 GEMM's builder applies unchanged
    da, dw = torch.from_numpy(deq(qa, sa)), torch.from_numpy(deq(qw, sw))
    for i, (got, ref, nw, sc_) in enumerate(((Q, qref, qn, scale), (Kh, kref, kn, 1.0), (V, vref, None, 1.0))):
        bound = error_bounds.qkv_heads(da, dw[i * C:(i + 1) * C], bias=bias[i * C:(i + 1) * C], norm_w=nw, eps=1e-5, scale=sc_)
        bound = bound.reshape(B, L, H, 64).permute(0, 2, 1, 3)
        if i == 2 and vt:
            from conftest import vt_layout
            ref, bound = vt_layout(ref), vt_layout(bound)
        error_bounds.assert_within(got, ref, bound, "QKV"[i] + " of MXFP8 operands")
    if vt:
        # the transposed V with the documented key order (quarters 0, 2, 1, 3 of every 16 keys: conftest.vt_layout), element by element
        from conftest import vt_layout
        ref = vt_layout(vref.to(torch.bfloat16)).double()
        assert torch.allclose(V.double().cpu(), ref, rtol=2 ** -7, atol=1e-3 * float(vref.abs().max()))
    else:
        assert torch.allclose(V.double().cpu(), vref, rtol=2 ** -7, atol=1e-3 * float(vref.abs().max()))


def test_gemm_mx_nan_block_reaches_exactly_its_row():
    ops = _ops()
    M, N, K = 256, 256, 768
    g = torch.Generator().manual_seed(14)
    a = torch.randn(M, K, generator=g)
    a[77, 300] = float("nan")
    w = torch.randn(N, K, generator=g) * 0.05
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ops.gemm_mx(ops.mx_quant(a.to(DEV)), ops.mx_quant(w.to(DEV)), out)
    bad = torch.isnan(out.float()).cpu()
    assert bad[77].all() and bad.sum() == N


def test_gemm_mx_refuses_unbuilt_problems_before_launching():
    ops = _ops()
    from motion324_amd.lib import M324Error
    a, w = ops.mx_empty(128, 192, DEV), ops.mx_empty(128, 192, DEV)
    with pytest.raises(M324Error, match="multiple of 128"):
        ops.gemm_mx(a, w, torch.empty(128, 128, dtype=torch.bfloat16, device=DEV))


# ==================================================================================================== tails, scale range, epilogues
# Everything below compares with tests/mx_cases.py: bit equality where the arithmetic is exact (the quantiser; the GEMM on
# integer operands with power-of-two scales), assert_mx_within against fp64 where it is not (LayerNorm -> MX).
SENT = 0xA5                                                       # fill byte of MX outputs: what is not written keeps it


def _mx_out(rows, K):
    """MX output storage one row and one block larger than [rows, K], filled with SENT"""
    from motion324_amd.ops import MX
    return MX(torch.full((rows + 1, K + 32), SENT, dtype=torch.uint8, device=DEV),
              torch.full((rows + 1, K // 32 + 1), SENT, dtype=torch.uint8, device=DEV))


def _mx_result(m, rows, K, what):
    """(q, s) of the [rows, K] corner after checking that nothing outside it was written"""
    q, s = m.q.cpu().numpy(), m.s.cpu().numpy()
    assert np.all(q[rows:] == SENT) and np.all(q[:, K:] == SENT), (what, "element bytes written outside [rows, K]")
    assert np.all(s[rows:] == SENT) and np.all(s[:, K // 32:] == SENT), (what, "scale bytes written outside [rows, K / 32]")
    return q[:rows, :K], s[:rows, :K // 32]


# ---------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,K", mx_cases.QUANT_SHAPES)
def test_mx_quant_tails_and_special_blocks_bit_exact(rows, K, dtype):
    """Block counts that are no multiple of the 64 blocks of a workgroup (the `g >= rows * nb` exit), nb = 1, 3, 5, 7 (a wave's
    16 blocks straddle rows), a block of -0.0, a negative amax element and, in fp32, amax mantissas on and next to 1.75."""
    ops = _ops()
    x = torch.from_numpy(mx_cases.quant_input(rows, K).copy()).to(dtype)
    out = _mx_out(rows, K)
    ops.mx_quant(x.to(DEV), out)
    q, s = _mx_result(out, rows, K, f"mx_quant {rows} x {K}")
    qr, sr = mx_quant_ref(x.float().numpy())
    assert np.array_equal(s, sr), np.argwhere(s != sr)[:8]
    assert np.array_equal(q, qr), np.argwhere(q != qr)[:8]
    zero = np.all(x.float().numpy().reshape(rows, K // 32, 32) == 0, axis=2)
    assert np.all(s[zero] == 0) and np.all(q.reshape(rows, K // 32, 32)[zero] == 0)       # -0.0 blocks included: +0 elements


# ---------------------------------------------------------------------------------------------------- LayerNorm -> MX
@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("rows,C", mx_cases.LN_SHAPES)
def test_layernorm_mx_within_fp64_bound(rows, C, with_b):
    """Against fp64 LayerNorm and error_bounds.layernorm: every scale byte admissible, every element code in its range (bit
    equality wherever the range is one code; tests/test_mx_cases_cpu.py caps the share of the others at 3 %)."""
    ops = _ops()
    x, w, b, ref, err = mx_cases.ln_case(rows, C, with_b)
    out = _mx_out(rows, C)
    ops.layernorm_mx(x.to(DEV), w.to(DEV), b.to(DEV) if with_b else None, mx_cases.LN_EPS, out)
    what = f"layernorm_mx {rows} x {C} b={with_b}"
    q, s = _mx_result(out, rows, C, what)
    blocks, elements = mx_cases.assert_mx_within(q, s, ref, err, what)
    print(f"{what}: {100 * elements:.2f} % of elements admit two codes, {100 * blocks:.2f} % of blocks two bytes")
    assert elements <= mx_cases.CAP_ELEMENTS and blocks <= mx_cases.CAP_BLOCKS


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("rows,C", [(5, 192), (6, 800)])
def test_layernorm_mx_constant_row_is_the_quantised_bias(rows, C, with_b):
    """x - mean = 0 exactly on a constant row (its sums are exact: small integers), so y = b bit for bit; without b the row is
    all-zero blocks: byte 0 and +0 elements, whatever the sign of w."""
    ops = _ops()
    x, w, b = mx_cases.ln_input(rows, C)
    x[1], x[rows - 1] = 3.0, -5.0
    m = ops.layernorm_mx(x.to(DEV), w.to(DEV), b.to(DEV) if with_b else None, mx_cases.LN_EPS)
    q, s = _mx_to_np(m, rows, C)
    want = b.numpy()[None, :] if with_b else np.zeros((1, C), np.float32)
    qr, sr = mx_quant_ref(want)
    for r in (1, rows - 1):
        assert np.array_equal(s[r], sr[0]) and np.array_equal(q[r], qr[0]), r
    if not with_b:
        assert not s[1].any() and not q[1].any()


def test_layernorm_mx_nan_row_reaches_exactly_its_row():
    ops = _ops()
    rows, C = 9, 288
    x, w, b = mx_cases.ln_input(rows, C)
    clean = ops.layernorm_mx(x.to(DEV), w.to(DEV), b.to(DEV), mx_cases.LN_EPS)
    qc, sc = _mx_to_np(clean, rows, C)
    x[5, 77] = float("nan")                                       # rows 4 .. 7 share a workgroup
    m = ops.layernorm_mx(x.to(DEV), w.to(DEV), b.to(DEV), mx_cases.LN_EPS)
    q, s = _mx_to_np(m, rows, C)
    assert np.all(s[5] == 0xFF) and np.all(q[5] == 0x7F)
    others = np.arange(rows) != 5
    assert np.array_equal(s[others], sc[others]) and np.array_equal(q[others], qc[others])


# ---------------------------------------------------------------------------------------------------- GEMM: outputs with a frame
def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()


def _framed(M, N, dtype, inner=None):
    """[M + 1, N + 8] of NaN (a spare row and spare columns that must stay) with the [M, N] corner set to `inner` (or left NaN);
    returns (whole tensor, the view a kernel gets)"""
    big = torch.full((M + 1, N + 8), float("nan"), dtype=dtype, device=DEV)
    if inner is not None:
        big[:M, :N] = torch.from_numpy(np.asarray(inner)).to(dtype).to(DEV)
    return big, big[:M, :N]


def _framed_result(big, M, N, what):
    fill = _bits(torch.full((1,), float("nan"), dtype=big.dtype))[0]
    bits = _bits(big)
    assert np.all(bits[M:] == fill) and np.all(bits[:, N:] == fill), (what, "written outside [M, N]")
    return big[:M, :N].float().cpu().numpy() if big.dtype == torch.bfloat16 else big[:M, :N].cpu().numpy()


def _bf16_of(ref):
    return torch.from_numpy(np.asarray(ref)).float().to(torch.bfloat16).float().numpy()      # exact fp32 value, rounded once


def _run_exact(kind, qa, sa, qw, sw, what, bias=None, gamma=None, res=None):
    """One m324_gemm_mx launch on integer operands into a framed output of `kind` ("bf16", "f32", "mx"), compared bit for bit
    with the fp64 result rounded once to the output type: ((a w^T + bias) gamma + res; "f32" updates res, zero by default, in
    place).  Returns (got, want) as the test may want to say more about a difference; asserts equality itself."""
    ops = _ops()
    M, N = qa.shape[0], qw.shape[0]
    ref = deq(qa, sa) @ deq(qw, sw).T
    dev = {k: None if v is None else torch.from_numpy(np.asarray(v, np.float32)).to(DEV) for k, v in (("bias", bias), ("gamma", gamma))}
    if bias is not None:
        ref = ref + np.asarray(bias, np.float64)
    if kind == "mx":
        out = _mx_out(M, N)
        ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), out, bias=dev["bias"])
        q, s = _mx_result(out, M, N, what)
        qr, sr = mx_quant_ref(ref)
        assert np.array_equal(s, sr), (what, np.argwhere(s != sr)[:8])
        assert np.array_equal(q, qr), (what, np.argwhere(q != qr)[:8])
        return (q, s), (qr, sr)
    if kind == "bf16":
        big, view = _framed(M, N, torch.bfloat16)
        ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), view, bias=dev["bias"])
        want = _bf16_of(ref)
    else:
        res = np.zeros((M, N)) if res is None else res
        if gamma is not None:
            ref = ref * np.asarray(gamma, np.float64)
        ref = ref + res
        big, view = _framed(M, N, torch.float32, res)
        ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), view, bias=dev["bias"], gamma=dev["gamma"], residual=view)
        want = ref.astype(np.float32)
        assert np.array_equal(want.astype(np.float64)[np.isfinite(ref)], ref[np.isfinite(ref)])      # the case is exact in fp32
    got = _framed_result(big, M, N, what)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in np.argwhere(~same)[:8]])
    return got, want


# ---------------------------------------------------------------------------------------------------- GEMM: scale range
G_WIDE = (-126, -100, -64, 0, 1, 64, 100, 126)                    # per block of K = 256: A gets 2^g, W gets 2^-g
G_ENDS = (-127, -100, -64, 0, 1, 64, 100, 127)                    # bytes 0 and 254 on both sides


def _scale_range_operands(g, per_block=False):
    """M = N = 128, K = 256.  A byte 127 + g(blk) + r(row), W byte 127 - g(blk) + c(col), r and c in -1 .. 1 (0 in the blocks
    where |g| = 127, so that the bytes there are exactly 0 and 254): every product is an integer times 2^(r + c), a multiple of
    1/4 below 2^17, so the fp32 sum is exact in any order -- IF the scaled MFMA applies 2^(s - 127) to every byte as
    include/m324.h states, combining 2^-126 with 2^+126 without leaving fp32's range in between.
    With r and c per row / column alone, a kernel that takes the scales of the WRONG block for A and W alike still gets every
    product right (g cancels); per_block draws r(row, blk) and c(col, blk), so that the pairing of scale and block matters."""
    rng = np.random.default_rng(21)
    M = N = 128
    qa, qw = _rne_e4m3(rng.integers(-8, 9, (M, 256)).astype(np.float64)), _rne_e4m3(rng.integers(-8, 9, (N, 256)).astype(np.float64))
    g = np.asarray(g)
    free = (np.abs(g) < 127)[None, :]
    if per_block:
        r, c = rng.integers(-1, 2, (M, 8)) * free, rng.integers(-1, 2, (N, 8)) * free
    else:
        r, c = (np.arange(M) % 3 - 1)[:, None] * free, ((np.arange(N) // 2) % 3 - 1)[:, None] * free
    sa, sw = 127 + g[None, :] + r, 127 - g[None, :] + c
    assert sa.min() >= 0 and sw.min() >= 0 and sa.max() <= 254 and sw.max() <= 254
    return qa, sa.astype(np.uint8), qw, sw.astype(np.uint8)


@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("g,per_block", [(G_WIDE, False), (G_ENDS, False), (G_WIDE, True)], ids=["wide", "bytes_0_and_254", "wide_per_block"])
def test_gemm_mx_scale_range_exact(g, per_block, kind):
    qa, sa, qw, sw = _scale_range_operands(g, per_block)
    if g is G_ENDS:
        assert (sa[:, 0] == 0).all() and (sw[:, 0] == 254).all() and (sa[:, 7] == 254).all() and (sw[:, 7] == 0).all()
    _run_exact(kind, qa, sa, qw, sw, f"scale range {g} -> {kind}")


# ---------------------------------------------------------------------------------------------------- GEMM: shapes, tile order
@pytest.mark.parametrize("kind", ["bf16", "f32", "mx"])
@pytest.mark.parametrize("M,N,K,xcd", [(1, 64, 128, None), (129, 64, 256, None), (127, 192, 128, None), (300, 640, 128, 0),
                                       (300, 640, 128, None)])
def test_gemm_mx_small_and_ragged_shapes_exact(M, N, K, xcd, kind, tune):
    """One row; a second row tile holding one row; N = 64 (half the waves idle); N = 192 (the last column tile half empty) with a
    ragged M through store_tile_mx's shuffles; 15 tiles (no multiple of the 8 XCDs) in round-robin and in XCD-contiguous order."""
    if xcd is not None:
        tune("M324_XCD", xcd)
    qa, sa = _int_operands(M, K, 31)
    qw, sw = _int_operands(N, K, 32, asym=True)
    _run_exact(kind, qa, sa, qw, sw, f"{M} x {N} x {K} -> {kind}, M324_XCD={xcd}")


# ---------------------------------------------------------------------------------------------------- GEMM: epilogue forms
def _epilogue_operands():
    M, N, K = 127, 192, 128
    rng = np.random.default_rng(41)
    qa, sa = _int_operands(M, K, 42)
    qw, sw = _int_operands(N, K, 43, asym=True)
    bias = rng.integers(-16, 17, N).astype(np.float64)
    gamma = 2.0 ** rng.integers(-2, 3, N)
    res = rng.integers(-64, 65, (M, N)).astype(np.float64)
    return qa, sa, qw, sw, bias, gamma, res


@pytest.mark.parametrize("kind", ["bf16", "mx"])
def test_gemm_mx_integer_bias_exact(kind):
    """bf16 output with bias, and MX output with bias and no activation (bit-exact against mx_quant_ref of the fp64 result)"""
    qa, sa, qw, sw, bias, _, _ = _epilogue_operands()
    _run_exact(kind, qa, sa, qw, sw, f"{kind} + bias", bias=bias)


@pytest.mark.parametrize("with_bias,with_gamma", [(True, False), (False, True), (True, True), (False, False)])
def test_gemm_mx_residual_update_forms_exact(with_bias, with_gamma):
    """x <- (a w^T + bias) gamma + x element by element: integer bias and residual, power-of-two gamma, every value a multiple of
    2^-4 below 2^20"""
    qa, sa, qw, sw, bias, gamma, res = _epilogue_operands()
    _run_exact("f32", qa, sa, qw, sw, f"residual update bias={with_bias} gamma={with_gamma}", bias=bias if with_bias else None,
               gamma=gamma if with_gamma else None, res=res)


# ---------------------------------------------------------------------------------------------------- GEMM: q|k|v heads
@pytest.mark.parametrize("parts,norm,vt", [("kv", True, False), ("q", True, False), ("qkv", False, False), ("kv", True, True)],
                         ids=["kv_knorm", "q_alone", "qkv_no_norm", "kv_vt"])
def test_gemm_mx_qkv_heads_parts(parts, norm, vt):
    ops = _ops()
    B, L, H, K = 2, 128, 2, 128
    C = H * 64
    M, N = B * L, len(parts) * C
    qa, sa = _rand_mx(M, K, 51)
    qw, sw = _rand_mx(N, K, 52, 0.1)
    g = torch.Generator().manual_seed(53)
    bias, qn, kn = torch.randn(N, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5, torch.rand(64, generator=g) + 0.5
    scale = 0.18
    outs = {p: torch.full((B, H, 64, L) if (p == "v" and vt) else (B, H, L, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
            for p in parts}
    nw = {"q": qn if norm else None, "k": kn if norm else None, "v": None}
    ops.gemm_mx(_to_mx(qa, sa), _to_mx(qw, sw), None, bias=bias.to(DEV),
                qkv_heads=(outs.get("q"), outs.get("k"), outs.get("v"), nw["q"].to(DEV) if "q" in parts and norm else None,
                           nw["k"].to(DEV) if "k" in parts and norm else None, 1e-5, scale, L, H))
    da, dw = torch.from_numpy(deq(qa, sa)), torch.from_numpy(deq(qw, sw))
    p64 = da @ dw.T + bias.double()
    heads = p64.reshape(B, L, len(parts), H, 64).permute(2, 0, 3, 1, 4)              # [parts, B, H, L, 64]
    for i, p in enumerate(parts):
        sc_ = scale if p == "q" else 1.0
        ref = heads[i]
        if nw[p] is not None:
            ref = ref * torch.rsqrt((ref * ref).mean(-1, keepdim=True) + 1e-5) * nw[p].double()
        ref = ref * sc_
        bound = error_bounds.qkv_heads(da, dw[i * C:(i + 1) * C], bias=bias[i * C:(i + 1) * C], norm_w=nw[p], eps=1e-5, scale=sc_)
        bound = bound.reshape(B, L, H, 64).permute(0, 2, 1, 3)
        if p == "v" and vt:
            from conftest import vt_layout
            ref, bound = vt_layout(ref), vt_layout(bound)
        error_bounds.assert_within(outs[p], ref, bound, f"{p} of parts {parts} (norm={norm}, vt={vt})")


# ---------------------------------------------------------------------------------------------------- GEMM: non-finite operands
def _poison(q, s, row, blk):
    q, s = q.copy(), s.copy()
    q[row, blk * 32:blk * 32 + 32], s[row, blk] = 0x7F, 0xFF
    return q, s


@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_gemm_mx_nan_weight_block_reaches_exactly_its_column(kind):
    qa, sa, qw, sw, bias, gamma, res = _epilogue_operands()
    qw, sw = _poison(qw, sw, 70, 2)
    got, _ = _run_exact(kind, qa, sa, qw, sw, f"NaN block in W row 70 -> {kind}", bias=bias, gamma=gamma if kind == "f32" else None,
                        res=res if kind == "f32" else None)
    bad = np.isnan(got)
    assert bad[:, 70].all() and bad.sum() == got.shape[0]


def test_gemm_mx_nan_operand_block_reaches_exactly_its_mx_row():
    qa, sa, qw, sw, bias, _, _ = _epilogue_operands()
    qa, sa = _poison(qa, sa, 100, 1)
    (q, s), _ = _run_exact("mx", qa, sa, qw, sw, "NaN block in A row 100 -> MX", bias=bias)
    assert np.all(s[100] == 0xFF) and np.all(q[100] == 0x7F)
    others = np.arange(q.shape[0]) != 100
    assert not np.any(s[others] == 0xFF) and not np.any((q[others] & 0x7F) == 0x7F)


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(match, call, *outputs):
    """`call` must raise M324Error matching `match` and, after a device synchronise, have left every output as it was"""
    from motion324_amd.lib import M324Error
    before = [t.clone() for t in outputs]
    with pytest.raises(M324Error, match=match):
        call()
    torch.cuda.synchronize()
    for t, b in zip(outputs, before):
        assert torch.equal(t, b), "a refused call wrote to its output"


def _filled(shape, dtype):
    return torch.full(shape, SENT if dtype == torch.uint8 else 7.0, dtype=dtype, device=DEV)


def _mx_filled(rows, K):
    from motion324_amd.ops import MX
    return MX(_filled((rows, K), torch.uint8), _filled((rows, (K // 32 + 3) // 4 * 4), torch.uint8)[:, :K // 32])


def test_gemm_mx_refusals_leave_the_outputs_alone():
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    from motion324_amd.ops import MX
    a, w = _mx_filled(128, 128), _mx_filled(128, 128)
    bf, f32 = _filled((128, 128), torch.bfloat16), _filled((128, 128), torch.float32)
    vec = _filled((128,), torch.float32)
    _refused("multiple of 64", lambda: ops.gemm_mx(a, _mx_filled(96, 128), bf), bf)
    _refused("not built", lambda: ops.gemm_mx(a, w, bf, act=ACT_GELU), bf)
    _refused("not built", lambda: ops.gemm_mx(a, w, bf, gamma=vec), bf)
    _refused("not built", lambda: ops.gemm_mx(a, w, f32), f32)
    other = _filled((128, 128), torch.float32)
    _refused("not built", lambda: ops.gemm_mx(a, w, f32, residual=other), f32, other)
    # operand and output views
    wide = _filled((128, 136), torch.uint8)
    _refused("operand rows must be 16-byte", lambda: ops.gemm_mx(MX(wide[:, :128], a.s), w, bf), bf)        # lda = 136
    s6 = _filled((128, 6), torch.uint8)
    _refused("scale rows 4-byte", lambda: ops.gemm_mx(a, MX(w.q, s6[:, :4]), bf), bf)                       # scale row stride 6
    bf132 = _filled((128, 132), torch.bfloat16)
    _refused("bf16 C misaligned", lambda: ops.gemm_mx(a, w, bf132[:, :128]), bf132)                          # ldc = 132
    narrow = MX(_filled((128, 128), torch.uint8), _filled((128, 3), torch.uint8))
    _refused(r"MX operand of at least \[128, 128\]", lambda: ops.gemm_mx(a, w, narrow), narrow.q, narrow.s)  # 3 scale bytes for 4 blocks


def test_gemm_mx_qkv_heads_refusals_leave_the_outputs_alone():
    ops = _ops()
    from motion324_amd.lib import ACT_GELU
    H = 2
    w3 = _mx_filled(3 * H * 64, 128)
    vec = _filled((3 * H * 64,), torch.float32)

    def heads(B, L, vt=False):
        q, k = _filled((B, H, L, 64), torch.bfloat16), _filled((B, H, L, 64), torch.bfloat16)
        v = _filled((B, H, 64, L) if vt else (B, H, L, 64), torch.bfloat16)
        return (q, k, v, None, None, 1e-5, 1.0, L, H), (q, k, v)
    hv, outs = heads(1, 192, vt=True)                             # L % 64 == 0, so the wrapper lets it through: L % 128 != 0
    _refused("qkv_L % 128", lambda: ops.gemm_mx(_mx_filled(192, 128), w3, None, qkv_heads=hv), *outs)
    hn, outs = heads(1, 128)
    _refused("N=256 vs 3 parts of 2 heads", lambda: ops.gemm_mx(_mx_filled(128, 128), _mx_filled(256, 128), None, qkv_heads=hn), *outs)
    a = _mx_filled(128, 128)
    # arguments the q|k|v heads epilogue does not take: refused, never dropped
    res = _filled((128, 3 * H * 64), torch.float32)
    _refused("residual= goes with the fp32 residual stream only", lambda: ops.gemm_mx(a, w3, None, qkv_heads=hn, residual=res), res, *outs)
    _refused("no activation / residual / gamma", lambda: ops.gemm_mx(a, w3, None, qkv_heads=hn, act=ACT_GELU), *outs)
    _refused("no activation / residual / gamma", lambda: ops.gemm_mx(a, w3, None, qkv_heads=hn, gamma=vec), *outs)


def test_gemm_mx_refuses_a_residual_with_an_mx_output():
    ops = _ops()
    a, w, out = _mx_filled(128, 128), _mx_filled(128, 128), _mx_filled(128, 128)
    res = _filled((128, 128), torch.float32)
    _refused("residual= goes with the fp32 residual stream only", lambda: ops.gemm_mx(a, w, out, residual=res), out.q, out.s, res)
    _refused("not built", lambda: ops.gemm_mx(a, w, out, gamma=_filled((128,), torch.float32)), out.q, out.s)


def test_layernorm_mx_and_mx_quant_refusals_leave_the_outputs_alone():
    ops = _ops()
    for C in (48, 1056):
        out = _mx_filled(4, C)
        x, w = _filled((4, C), torch.float32), _filled((C,), torch.float32)
        _refused(f"C={C} ", lambda: ops.layernorm_mx(x, w, None, 1e-6, out), out.q, out.s)
    out = _mx_filled(4, 64)
    _refused("x must be fp32", lambda: ops.layernorm_mx(_filled((4, 64), torch.bfloat16), _filled((64,), torch.float32), None, 1e-6, out),
             out.q, out.s)
    out = _mx_filled(4, 48)
    _refused("K=48 ", lambda: ops.mx_quant(_filled((4, 48), torch.float32), out), out.q, out.s)
    out = _mx_filled(4, 64)
    _refused("unsupported dtype", lambda: ops.mx_quant(_filled((4, 64), torch.float16), out), out.q, out.s)
    x34 = _filled((4, 34), torch.float32)
    out = _mx_filled(4, 32)
    _refused("x rows must be 16-byte", lambda: ops.mx_quant(x34[:, :32], out), out.q, out.s)                 # row stride 136 bytes
