"""Block-scaled FP8 (MX) kernels: m324_mx_quant against a numpy statement of the quantisation rule (include/m324.h, "MX
operands"), m324_gemm_mx against fp64 products of the dequantised operands, m324_layernorm_mx against m324_layernorm + the rule."""
import math

import numpy as np
import pytest
import torch

import error_bounds

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from motion324_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------- numpy reference
def _e4m3_table():
    """value of every finite e4m3fn code 0x00 .. 0x7E (positive half)"""
    v = np.zeros(127)
    for c in range(127):
        e, m = c >> 3, c & 7
        v[c] = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
    return v


E4M3 = _e4m3_table()


def _rne_e4m3(y):
    """|y| <= 448 -> e4m3fn code, round to nearest, ties to the even code (independent of the kernels: table search)"""
    a = np.abs(y)
    hi = np.searchsorted(E4M3, a, side="left").clip(0, 126)
    lo = (hi - 1).clip(0, 126)
    dl, dh = a - E4M3[lo], E4M3[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(a == E4M3[hi], hi, code)
    return (code | np.where(np.signbit(y), 0x80, 0)).astype(np.uint8)


def mx_quant_ref(x):
    """x float64-representable [rows, K] -> (q uint8, s uint8) by the rule: X = ceil(log2(amax / 448)) in [-127, 127]"""
    rows, K = x.shape
    b = x.reshape(rows, K // 32, 32).astype(np.float64)
    q = np.zeros(b.shape, np.uint8)
    s = np.zeros(b.shape[:2], np.uint8)
    for r in range(rows):
        for j in range(K // 32):
            v = b[r, j]
            if not np.all(np.isfinite(v)):
                s[r, j], q[r, j] = 0xFF, 0x7F
                continue
            amax = np.abs(v).max()
            if amax == 0:
                continue
            X = math.ceil(math.log2(amax / 448.0))
            while amax > 448.0 * 2.0 ** X:          # guard against log2 rounding: the smallest X with amax <= 448 2^X
                X += 1
            while amax <= 448.0 * 2.0 ** (X - 1):
                X -= 1
            X = max(-127, min(127, X))
            s[r, j] = X + 127
            q[r, j] = _rne_e4m3(v * 2.0 ** -X)
    return q.reshape(rows, K), s


def deq(q, s):
    """(q, s) -> float64 values"""
    q = np.asarray(q, np.uint8)
    mag = np.where((q & 0x7F) == 0x7F, np.nan, E4M3[np.minimum(q & 0x7F, 126)])
    v = np.where(q & 0x80, -mag, mag)
    sc = np.where(s == 0xFF, np.nan, 2.0 ** (s.astype(np.float64) - 127))
    return v * np.repeat(sc, 32, axis=1)


def _mx_to_np(m, rows, K):
    return m.q[:rows, :K].cpu().numpy(), m.s[:rows, :K // 32].cpu().numpy()


def _to_mx(q, s):
    from motion324_amd.ops import mx_empty
    rows, K = q.shape
    m = mx_empty(rows, K, DEV)
    m.q.copy_(torch.from_numpy(np.ascontiguousarray(q)))
    m.s.copy_(torch.from_numpy(np.ascontiguousarray(s)))
    return m


# ---------------------------------------------------------------------------------------------------- quantiser
def _quant_input():
    rng = np.random.default_rng(7)
    rows, K = 96, 256
    x = (rng.standard_normal((rows, K)) * 2.0 ** rng.integers(-20, 21, (rows, 1))).astype(np.float32)
    x[3, 32:64] = 0.0                                            # zero block
    x[4, :32] = 2.0 ** rng.integers(-30, 30, 32)                 # exact powers of two
    for i, a in enumerate((448.0, 449.0, 447.99997, 512.0, 896.0, 896.0001, 224.0, 3.0e38, 1e-38, 1e-42)):
        x[5 + i, 64:96] = rng.uniform(-1, 1, 32).astype(np.float32) * np.float32(a) / 2
        x[5 + i, 64] = np.float32(a)                             # amax next to / on a scale boundary
    x[20, 0:32] = np.linspace(-448, 448, 32, dtype=np.float32) / 64    # element rounding ties
    x[21, 5], x[22, 40], x[23, 100] = np.nan, np.inf, -np.inf     # non-finite blocks
    return x


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
def _int_operands(rows, K, seed, asym=False):
    """integer-valued MX operands: elements -8 .. 8 (exact in e4m3), scales 2^-1 .. 2^1 -> every product exact in fp32"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, (rows, K)).astype(np.float64)
    if asym:
        v += (np.arange(rows)[:, None] % 5) - 2
        v = np.clip(v, -8, 8)
    s = (127 + rng.integers(-1, 2, (rows, K // 32))).astype(np.uint8)
    q = _rne_e4m3(v)
    return q, s


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


def _rand_mx(rows, K, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g) * scale
    q, s = mx_quant_ref(x.numpy())
    return q, s


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
