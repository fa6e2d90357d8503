"""The tests of the test: tests/error_bounds.py on the CPU (no GPU needed).

For every bound builder a CPU EMULATION of the operation with the kernels' rounding points (bf16-rounded operands, fp32 torch
arithmetic, bf16 rounding of P / dS / of the output) on the shapes the GPU tests use, and three kinds of assertion:
  soundness -- the emulation lies inside the bound everywhere (a builder that is unsound on its own emulation is wrong);
  power     -- planted faults of the kind the kernels can produce (a 16-byte store chunk holding its neighbour's values, a (row,
               head) vector holding the previous row's, a NaN fill left behind, a row never written, an LSE entry off by 0.05) are
               caught, every one of them, by the same assert_within / violations the GPU tests call;
  the hole  -- for three of those faults the Frobenius-norm ratio `rel_err` stays BELOW the gate the GPU tests had before
               (6e-3 / 8e-3 / 2e-2): why a norm gate alone was not enough."""
import math

import numpy as np
import pytest
import torch

import error_bounds as eb
import optimizer_cases as oc
import rowkernel_cases as rc
import wgrad_cases as wc
from conftest import rel_err

BF = torch.bfloat16
PS = 64 ** -0.5 * math.log2(math.e)           # ops.Q_PRESCALE: softmax scale * log2(e)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def _q(t, dtype=BF):
    return t.to(dtype).to(torch.float32)


def _gelu32(z):
    return 0.5 * z * (1 + torch.erf(z * 0.70710678118654752440))


# ------------------------------------------------------------------------------------------- emulations
def _gemm_operands(M, N, K, wscale=0.1):
    return _q(_rand((M, K), 11)), _q(_rand((N, K), 12, wscale)), _rand((N,), 13)


def _gemm_emulation(a, w, bias, act, out_dtype=BF):
    """bf16 operands (already rounded), fp32 a w^T + b, fp32 erf GELU, one rounding to out_dtype"""
    z = a @ w.T + bias
    return (_gelu32(z) if act else z).to(out_dtype).float()


def _gemm_reference(a, w, bias, act):
    z = a.double() @ w.double().T + bias.double()
    return z, (eb.gelu(z) if act else z)


def _attn_operands(B, H, Lq, Lk, amp=1.5, seed=19):
    q, k, v = (_rand((B, H, L, 64), seed + i, sc) for i, (L, sc) in enumerate(((Lq, amp), (Lk, amp), (Lk, 1.0))))
    return _q(q * PS), _q(k), _q(v)                 # q carries scale * log2(e), as m324_qkv_split stores it


def _attn_emulation(qs, k, v):
    """log2-domain fp32 scores, fp32 exp2 and row sums of the UNROUNDED probabilities, P rounded to bf16 for P V, bf16 output;
    returns O [B * Lq, H * 64], the log2-domain LSE [B, H, Lq] and the fp32 O before rounding"""
    B, H, Lq, _ = qs.shape
    s = torch.einsum("bhqd,bhkd->bhqk", qs, k)
    m = s.max(-1, keepdim=True).values
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("bhqk,bhkd->bhqd", p.to(BF).float(), v) / l
    lse = (m + torch.log2(l))[..., 0]
    return o.to(BF).float().permute(0, 2, 1, 3).reshape(B * Lq, H * 64), lse, o


def _attn_reference(qs, k, v):
    B, H, Lq, _ = qs.shape
    s = torch.einsum("bhqd,bhkd->bhqk", qs.double(), k.double())
    o = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(s * math.log(2.0), -1), v.double()).reshape(B * Lq, H * 64)
    return o, torch.logsumexp(s * math.log(2.0), -1) / math.log(2.0)


def _bwd_case(B, H, Lq, Lk):
    """operands of the GPU backward tests (inputs scaled 1.2), the emulation of the MFMA backward (fp32 softmax from the saved LSE,
    P and dS rounded to bf16 before their products, D from the bf16-rounded O, bf16 dQ / dK / dV) and fp64 autograd"""
    qs = _q(_rand((B, H, Lq, 64), 41, 1.2) * PS)
    k, v, dO = _q(_rand((B, H, Lk, 64), 42, 1.2)), _q(_rand((B, H, Lk, 64), 43)), _q(_rand((B, H, Lq, 64), 44))
    _, lse, o32 = _attn_emulation(qs, k, v)
    D = (o32.to(BF).float() * dO).sum(-1, keepdim=True)
    p = torch.exp2(torch.einsum("bhqd,bhkd->bhqk", qs, k) - lse[..., None])
    dS = p * (torch.einsum("bhqd,bhkd->bhqk", dO, v) - D)
    pb, dSb = p.to(BF).float(), dS.to(BF).float()
    scale = 64 ** -0.5
    got = ((torch.einsum("bhqk,bhkd->bhqd", dSb, k) * scale).to(BF).float(),
           (torch.einsum("bhqk,bhqd->bhkd", dSb, qs) * math.log(2.0)).to(BF).float(),
           torch.einsum("bhqk,bhqd->bhkd", pb, dO).to(BF).float())
    qh = (qs.double() / PS).requires_grad_(True)
    kd, vd = k.double().requires_grad_(True), v.double().requires_grad_(True)
    sc = torch.einsum("bhqd,bhkd->bhqk", qh, kd) * scale
    torch.einsum("bhqk,bhkd->bhqd", torch.softmax(sc, -1), vd).backward(dO.double())
    ref = (qh.grad, kd.grad, vd.grad)
    bounds = eb.attention_backward(qh.detach(), k, v, dO, scale)
    return got, ref, bounds


def _run_holds_previous(out, r, c0, n):
    """the fault: the n-element run at (r, c0) holds the previous run's values (a clamped column offset, a wrong epilogue choice)"""
    bad = out.clone()
    bad[r, c0:c0 + n] = out[r, c0 - n:c0]
    return bad


# ------------------------------------------------------------------------------------------- the assertion itself
def test_assert_within_counts_nan_and_unwritten_fill_as_violations():
    ref = torch.linspace(-2, 2, 40).reshape(5, 8).double()
    bound = eb.cast(ref)
    out = ref.to(BF).float()
    assert eb.assert_within(out, ref, bound, "rounded") <= 1.0
    nan = out.clone()
    nan[3, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 40 .*\(3, 5\)"):
        eb.assert_within(nan, ref, bound, "nan left behind")
    fill = out.clone()
    fill[4] = 7.0
    with pytest.raises(AssertionError, match="8 of 40"):
        eb.assert_within(fill, ref, bound, "row never written")
    with pytest.raises(AssertionError):                       # a NaN bound passes nothing either
        eb.assert_within(out, ref, bound * float("nan"), "nan bound")
    zero = torch.zeros(3, 4, dtype=torch.float64)             # an exact zero against a zero bound (rows a row map skips) passes
    assert eb.assert_within(zero, zero, zero, "zeros") == 0.0
    with pytest.raises(AssertionError):
        eb.assert_within(zero + 1e-30, zero, zero, "not quite zero")


# ------------------------------------------------------------------------------------------- GEMM
GEMM_SHAPES = [(690, 328, 64), (690, 328, 192), (690, 328, 832), (2048, 768, 3072), (1028, 3072, 768)]


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_bound_is_sound_and_catches_every_planted_chunk(M, N, K, act):
    a, w, bias = _gemm_operands(M, N, K, 0.05 if K >= 768 else 0.1)
    out = _gemm_emulation(a, w, bias, act)
    z, ref = _gemm_reference(a, w, bias, act)
    bound = eb.gemm(a, w, z=z, bias=bias, act=act)
    assert torch.equal(bound, eb.gemm(a, w, bias=bias, act=act))              # the caller's z is only a shortcut
    worst = eb.assert_within(out, ref, bound, f"gemm emulation {M}x{N}x{K} act={act}")
    assert 0.3 < worst <= 1.0                                                 # sound, and not slack: one bf16 rounding fills it
    # (a) a 16-byte run (8 bf16) holding the previous run's values, at 500 seeded positions and the last run of the last row
    g = torch.Generator().manual_seed(1000 + K)
    rows = torch.randint(0, M, (500,), generator=g).tolist() + [M - 1]
    cols = (torch.randint(1, N // 8, (500,), generator=g) * 8).tolist() + [N - 8]
    for r, c0 in zip(rows, cols):
        hit = eb.violations(out[r, c0 - 8:c0], ref[r, c0:c0 + 8], bound[r, c0:c0 + 8])
        assert int(hit.sum()) >= 1, (r, c0)
    for r, c0 in list(zip(rows, cols))[:3] + [(M - 1, N - 8)]:                # and through the assertion the GPU tests call
        with pytest.raises(AssertionError, match="outside their error bound"):
            eb.assert_within(_run_holds_previous(out, r, c0, 8), ref, bound, "planted chunk")
    # (c) one element left at a NaN fill, (d) one row never written (fill 7.0, as the guard rows of the v15 test)
    bad = out.clone()
    bad[M // 2, N - 1] = float("nan")
    with pytest.raises(AssertionError, match="1 of"):
        eb.assert_within(bad, ref, bound, "nan")
    bad = out.clone()
    bad[M - 1] = 7.0
    with pytest.raises(AssertionError):
        eb.assert_within(bad, ref, bound, "unwritten row")
    assert int(eb.violations(bad, ref, bound).sum()) >= N - 2


@pytest.mark.parametrize("act", [False, True])
def test_gemm_planted_chunk_passes_the_norm_gate_but_not_the_bound(act):
    """The hole: at the shape and with the operands of test_gemm_every_schedule_forced, a 16-byte chunk holding its neighbour's
    values adds sqrt(16 / (690 * 328)) = 8.4e-3 of the norm when the two chunks are unrelated and less when they happen to be
    alike: of the 501 seeded positions 54 (plain) and 160 (behind GELU, where half of the values are near zero) keep rel_err
    under the 6e-3 gate of TOL[bf16], down to 3.2e-3 / 2.2e-3.  (The last chunk of the last row itself gives 7.3e-3 with these
    operands.)  The bound catches all 501."""
    M, N, K = 690, 328, 192
    a, w, bias = _gemm_operands(M, N, K)
    out = _gemm_emulation(a, w, bias, act)
    z, ref = _gemm_reference(a, w, bias, act)
    bound = eb.gemm(a, w, z=z, bias=bias, act=act)
    assert rel_err(out, ref) < 2e-3
    g = torch.Generator().manual_seed(1000 + K)
    rows = torch.randint(0, M, (500,), generator=g).tolist() + [M - 1]
    cols = (torch.randint(1, N // 8, (500,), generator=g) * 8).tolist() + [N - 8]
    passed_the_gate = []
    for r, c0 in zip(rows, cols):
        bad = _run_holds_previous(out, r, c0, 8)
        assert int(eb.violations(bad[r], ref[r], bound[r]).sum()) >= 1, (r, c0)
        if rel_err(bad, ref) < 6e-3:                           # the old gate lets it through
            passed_the_gate.append((r, c0))
    assert len(passed_the_gate) >= (120 if act else 40), len(passed_the_gate)
    r, c0 = passed_the_gate[0]
    with pytest.raises(AssertionError, match=rf"first rows hit \[{r}\]"):
        eb.assert_within(_run_holds_previous(out, r, c0, 8), ref, bound, "planted chunk")


def test_gemm_bound_fp32_output_epilogue_chain_and_fold():
    """fp32 output (4-element runs), gamma + residual + row map, the in-place bf16 residual stream, the LayerNorm-fold consumer"""
    M, N, K = 690, 328, 192
    a, w, bias = _gemm_operands(M, N, K)
    gamma, res = 1 + 0.1 * _rand((N,), 14), _rand((M, N), 15)
    out = (a @ w.T + bias) * gamma + res
    ref = (a.double() @ w.double().T + bias.double()) * gamma.double() + res.double()
    bound = eb.gemm(a, w, bias=bias, gamma=gamma, residual=res, out_dtype=torch.float32)
    assert eb.assert_within(out, ref, bound, "fp32 chain") <= 1.0
    g = torch.Generator().manual_seed(5)
    for r, c0 in zip(torch.randint(0, M, (500,), generator=g).tolist() + [M - 1],
                     (torch.randint(1, N // 4, (500,), generator=g) * 4).tolist() + [N - 4]):
        assert int(eb.violations(out[r, c0 - 4:c0], ref[r, c0:c0 + 4], bound[r, c0:c0 + 4]).sum()) >= 1, (r, c0)
    # row map: rows nothing maps to stay exactly zero
    placed = eb.remap_rows(out[:460].double(), 230, 233, 1, 2 * 233)
    assert eb.assert_within(placed, eb.remap_rows(ref[:460], 230, 233, 1, 2 * 233), eb.remap_rows(bound[:460], 230, 233, 1, 2 * 233),
                            "row map") <= 1.0
    placed[0, 3] = 1e-6
    with pytest.raises(AssertionError, match=r"\(0, 3\)"):
        eb.assert_within(placed, eb.remap_rows(ref[:460], 230, 233, 1, 2 * 233), eb.remap_rows(bound[:460], 230, 233, 1, 2 * 233), "x")
    # x += a w^T + b on the bf16 stream itself
    x0 = _q(_rand((M, N), 16))
    got = (x0 + (a @ w.T + bias)).to(BF).float()
    assert eb.assert_within(got, x0.double() + a.double() @ w.double().T + bias.double(),
                            eb.gemm(a, w, bias=bias, residual=x0), "bf16 stream in place") <= 1.0
    # fold consumer: rstd acc - rstd mean colsum + bias, then GELU
    r0, r1, colsum = _rand((M,), 18).abs() * 0.5 + 0.5, 0.1 * _rand((M,), 19), _rand((N,), 17)
    zf = r0[:, None] * (a @ w.T) + (r1[:, None] * colsum[None, :] + bias)
    zd = r0.double()[:, None] * (a.double() @ w.double().T) + r1.double()[:, None] * colsum.double()[None, :] + bias.double()
    bound = eb.gemm(a, w, bias=bias, fold=(r0, r1, colsum), act=True)
    out = _gelu32(zf).to(BF).float()
    assert eb.assert_within(out, eb.gelu(zd), bound, "fold + gelu") <= 1.0
    with pytest.raises(AssertionError):
        eb.assert_within(_run_holds_previous(out, M - 1, N - 8, 8), eb.gelu(zd), bound, "fold chunk")


def test_gemm_gelu_polynomial_term_is_what_the_kernel_documents():
    """the bf16 epilogue's erf polynomial (|erf error| <= 1.7e-5, argument clamped at 3): an emulation that is off by exactly that
    stays inside, one off by four times that does not (at outputs small enough for the term to matter)"""
    z = torch.linspace(-8, 8, 4001).double().reshape(1, -1)
    a, w = torch.ones(1, 64, dtype=torch.float64) / 8, z.T.repeat(1, 64) / 8                 # a w^T = z exactly
    ref = eb.gelu(z)
    bound = eb.gemm(a, w, act=True)
    erf_ = torch.erf(z / math.sqrt(2.0)).clamp(-math.erf(3.0), math.erf(3.0))
    for sign in (1.0, -1.0):
        approx = z * (0.5 + 0.5 * (erf_ + sign * 1.7e-5))
        assert eb.assert_within(approx.to(BF), ref, bound, "documented polynomial error") <= 1.0
    with pytest.raises(AssertionError):
        eb.assert_within((z * (0.5 + 0.5 * (erf_ + 6.8e-5))).to(BF), ref, bound, "four times the documented error")
    exact = eb.gemm(a, w, act=True, out_dtype=torch.float32)                                  # erff: no such term
    assert bool((exact < bound).all()) and float((bound - exact)[0, 0]) > 7e-5       # z = -8: |z| / 2 * (1 - erf(3) + 1.7e-5)


def test_n3_head_and_gelu_grad_bounds_are_sound():
    M, N, K = 300, 256, 192
    a, w, bias = _gemm_operands(M, N, K)
    w3, b3 = _rand((3, N), 98, 0.2), _rand((3,), 99)
    z, g = _gemm_reference(a, w, bias, True)
    out = _gelu32(a @ w.T + bias) @ w3.T + b3
    bound = eb.n3_head(a, w, bias, w3, b3, z=z)
    assert eb.assert_within(out, g @ w3.double().T + b3.double(), bound, "n3 head") <= 1.0
    bad = out.clone()
    bad[M - 1] = out[M - 2]
    with pytest.raises(AssertionError):
        eb.assert_within(bad, g @ w3.double().T + b3.double(), bound, "n3 row")
    z32 = a @ w.T + bias
    d32 = 0.5 * (1 + torch.erf(z32 * 0.70710678118654752440)) + z32 * torch.exp(-0.5 * z32 * z32) * 0.39894228040143267794
    bound = eb.gemm_gelu_grad_store(a, w, z=z, bias=bias)
    assert eb.assert_within(d32.to(BF).float(), eb.gelu_grad(z), bound, "gelu'") <= 1.0
    with pytest.raises(AssertionError):
        eb.assert_within(_run_holds_previous(d32.to(BF).float(), M - 1, N - 8, 8), eb.gelu_grad(z), bound, "gelu' chunk")


# ------------------------------------------------------------------------------------------- LayerNorm / cast
@pytest.mark.parametrize("rows,C,bf16_in,with_bias,eps", [(77, 768, False, False, 1e-5), (77, 768, False, True, 1e-6), (77, 192, True, True, 1e-5)])
def test_layernorm_and_cast_bounds(rows, C, bf16_in, with_bias, eps):
    x = _rand((rows, C), 11) * 3 + 0.5
    if bf16_in:
        x = _q(x)
    w, b = 1 + 0.1 * _rand((C,), 12), (_rand((C,), 13) if with_bias else None)
    out = torch.nn.functional.layer_norm(x, (C,), w, b, eps).to(BF).float()
    ref = torch.nn.functional.layer_norm(x.double(), (C,), w.double(), None if b is None else b.double(), eps)
    bound = eb.layernorm(x, w, b, eps)
    assert 0.3 < eb.assert_within(out, ref, bound, "layernorm") <= 1.0
    with pytest.raises(AssertionError):
        eb.assert_within(_run_holds_previous(out, rows - 1, C - 8, 8), ref, bound, "layernorm chunk")
    bad = out.clone()
    bad[rows - 1] = out[rows - 2]                             # a row normalised with its neighbour's statistics' row
    with pytest.raises(AssertionError):
        eb.assert_within(bad, ref, bound, "layernorm row")
    assert eb.assert_within(x.to(BF).float(), x.double(), eb.cast(x), "cast") <= 1.0
    f32 = torch.nn.functional.layer_norm(x, (C,), w, b, eps)
    assert eb.assert_within(f32, ref, eb.layernorm(x, w, b, eps, out_dtype=torch.float32), "layernorm fp32") <= 1.0


# ------------------------------------------------------------------------------------------- attention forward, LSE, merge
@pytest.mark.parametrize("B,H,Lq,Lk,amp", [(1, 2, 300, 2100, 1.5), (2, 3, 100, 100, 1.5), (1, 2, 300, 2100, 2.2), (1, 2, 129, 65, 1.5)])
def test_attention_bounds_are_sound_and_catch_planted_faults(B, H, Lq, Lk, amp):
    qs, k, v = _attn_operands(B, H, Lq, Lk, amp)
    out, lse, _ = _attn_emulation(qs, k, v)
    ref, lse_ref = _attn_reference(qs, k, v)
    bound, lse_bound = eb.attention_and_lse(qs, k, v, math.log(2.0))
    assert 0.2 < eb.assert_within(out, ref, bound, f"attention emulation {B}x{H}x{Lq}x{Lk}") <= 1.0
    assert eb.assert_within(lse, lse_ref, lse_bound, "lse emulation") <= 1.0
    assert float(lse_bound.max()) < 2e-3                       # far inside the gates the GPU tests had (2e-3 / 2e-2)
    assert torch.equal(lse_bound, eb.attention_lse(qs, k, math.log(2.0))) and torch.equal(bound, eb.attention(qs, k, v, math.log(2.0)))
    # (a) 16-byte runs
    g = torch.Generator().manual_seed(7)
    n = B * Lq
    for r, c0 in zip(torch.randint(0, n, (500,), generator=g).tolist() + [n - 1],
                     (torch.randint(1, H * 8, (500,), generator=g) * 8).tolist() + [H * 64 - 8]):
        assert int(eb.violations(out[r, c0 - 8:c0], ref[r, c0:c0 + 8], bound[r, c0:c0 + 8]).sum()) >= 1, (r, c0)
    # (b) one (row, head) 64-vector holding the previous row's values: the ragged last query row, and a seeded one
    for r, h in ((n - 1, H - 1), (n // 2, 0)):
        bad = out.clone()
        bad[r, h * 64:(h + 1) * 64] = out[r - 1, h * 64:(h + 1) * 64]
        assert int(eb.violations(bad, ref, bound).sum()) >= 32
        with pytest.raises(AssertionError, match=rf"first rows hit \[{r}\]"):
            eb.assert_within(bad, ref, bound, "row of a head")
    # (c), (d)
    bad = out.clone()
    bad[n - 1, 5] = float("nan")
    with pytest.raises(AssertionError, match="1 of"):
        eb.assert_within(bad, ref, bound, "nan")
    bad = out.clone()
    bad[n - 1] = 7.0
    with pytest.raises(AssertionError):
        eb.assert_within(bad, ref, bound, "unwritten row")
    # (e) one LSE entry off by 0.05 (passes the 2e-2 gate of the long-sequence tests only just not; the 2e-3 one never sees 1e-3)
    for off in (0.05, 1e-3):
        bad = lse.clone()
        bad[B - 1, H - 1, Lq - 1] += off
        with pytest.raises(AssertionError, match="1 of"):
            eb.assert_within(bad, lse_ref, lse_bound, "lse entry")


def test_attention_wrong_row_of_one_head_passes_the_norm_gate_but_not_the_bound():
    """The hole: a 10368 x 768 output (32 frames x 324 tokens, 12 heads) with the last row of the last head holding the previous
    row's values has rel_err under the 8e-3 gate of the forward attention tests."""
    B, H, L = 32, 12, 324
    qs, k, v = _attn_operands(B, H, L, L)
    out, _, _ = _attn_emulation(qs, k, v)
    ref, _ = _attn_reference(qs, k, v)
    bound = torch.cat([eb.attention(qs[b:b + 1], k[b:b + 1], v[b:b + 1], math.log(2.0)) for b in range(B)])
    assert eb.assert_within(out, ref, bound, "attention emulation 10368 x 768") <= 1.0
    bad = out.clone()
    bad[-1, -64:] = out[-2, -64:]
    assert rel_err(out, ref) < 2.5e-3
    assert rel_err(bad, ref) < 8e-3                            # the old gate lets it through
    assert int(eb.violations(bad, ref, bound).sum()) >= 48
    with pytest.raises(AssertionError, match=r"first rows hit \[10367\]"):
        eb.assert_within(bad, ref, bound, "row of a head")


@pytest.mark.parametrize("B,H,Lq,cuts", [(1, 2, 300, (0, 700, 1500, 2100)), (2, 2, 100, (0, 64, 200, 333))])
def test_attention_merge_bound(B, H, Lq, cuts):
    Lk = cuts[-1]
    qs, k, v = _attn_operands(B, H, Lq, Lk, 1.2, seed=261)
    parts = [_attn_emulation(qs, k[:, :, a:b], v[:, :, a:b])[:2] for a, b in zip(cuts[:-1], cuts[1:])]
    lses = torch.stack([p[1] for p in parts])                                           # [parts, B, H, Lq]
    wgt = torch.exp2(lses - lses.max(0).values)
    tok = lambda t: t.permute(0, 2, 1).reshape(B * Lq, H, 1).expand(-1, -1, 64).reshape(B * Lq, H * 64)
    num = sum(tok(wgt[i]) * parts[i][0] for i in range(len(parts)))
    out = (num / tok(wgt.sum(0))).to(BF).float()
    ref, _ = _attn_reference(qs, k, v)
    bound = eb.attention_merge(qs, k, v, math.log(2.0), cuts)
    assert 0.1 < eb.assert_within(out, ref, bound, "merge emulation") <= 1.0
    bad = out.clone()
    bad[-1, -64:] = out[-2, -64:]
    with pytest.raises(AssertionError):
        eb.assert_within(bad, ref, bound, "merge row of a head")
    with pytest.raises(AssertionError):
        eb.assert_within(_run_holds_previous(out, B * Lq - 1, H * 64 - 8, 8), ref, bound, "merge chunk")


# ------------------------------------------------------------------------------------------- attention backward
@pytest.mark.parametrize("B,H,Lq,Lk", [(1, 2, 300, 2100), (2, 3, 100, 100), (1, 2, 700, 129)])
def test_attention_backward_bounds_are_sound_and_catch_planted_faults(B, H, Lq, Lk):
    got, ref, bounds = _bwd_case(B, H, Lq, Lk)
    for name, g_, r_, b_ in zip(("dQ", "dK", "dV"), got, ref, bounds):
        worst = eb.assert_within(g_, r_, b_, f"backward emulation {name} {B}x{H}x{Lq}x{Lk}")
        assert 0.02 < worst <= 1.0
        assert float((r_.abs() / b_).median()) > 2.5           # the bound is a fraction of a typical gradient element: it can see faults
        L = g_.shape[2]
        for row, h in ((L - 1, H - 1), (L // 2, 0)):           # (b) a (row, head) vector holding the previous row's values
            bad = g_.clone()
            bad[B - 1, h, row] = g_[B - 1, h, row - 1]
            assert int(eb.violations(bad, r_, b_).sum()) >= 32, (name, row, h)
            with pytest.raises(AssertionError):
                eb.assert_within(bad, r_, b_, "row of a head")
        bad = g_.clone()                                       # (a) a 16-byte run of the last row
        bad[B - 1, H - 1, L - 1, 56:] = g_[B - 1, H - 1, L - 1, 48:56]
        with pytest.raises(AssertionError):
            eb.assert_within(bad, r_, b_, "chunk")
        bad = g_.clone()                                       # a whole zeroed row of one head
        bad[B - 1, H - 1, L - 1] = 0.0
        assert int(eb.violations(bad, r_, b_).sum()) >= 32
        bad = g_.clone()                                       # (c)
        bad[0, 0, 0, 0] = float("nan")
        with pytest.raises(AssertionError, match="1 of"):
            eb.assert_within(bad, r_, b_, "nan")


def test_attention_backward_wrong_dv_row_passes_the_norm_gate_but_not_the_bound():
    """The hole: at 324 tokens x 12 heads one (row, head) vector is 1 / 3888 of the gradient's energy.  A dQ / dK / dV row of one
    head left at ZERO has rel_err ~ sqrt(1 / 3888) = 1.6e-2, under the 2e-2 gate of
    test_attention_backward_mfma_against_autograd; one holding its neighbour's values ~ sqrt(2 / 3888) = 2.3e-2, under the gate
    whenever the two rows are a little alike (here: for most of the 36 rows tried in dV, about half in dQ and dK).  The bound
    catches every one of them."""
    got, ref, bounds = _bwd_case(1, 12, 324, 324)
    for name, g_, r_, b_ in zip(("dQ", "dK", "dV"), got, ref, bounds):
        assert rel_err(g_, r_) < 3e-3
        assert eb.assert_within(g_, r_, b_, f"backward emulation 324 x 12 heads {name}") <= 1.0
        bad = g_.clone()
        bad[0, -1, -1] = 0.0
        assert rel_err(bad, r_) < 2e-2                         # the old gate lets it through
        assert int(eb.violations(bad, r_, b_).sum()) >= 48
        with pytest.raises(AssertionError, match="outside their error bound"):
            eb.assert_within(bad, r_, b_, f"{name} row of a head left at zero")
        under_the_gate = 0
        for h in range(12):
            for row in (323, 100, 1):
                bad = g_.clone()
                bad[0, h, row] = g_[0, h, row - 1]
                under_the_gate += rel_err(bad, r_) < 2e-2
                assert int(eb.violations(bad, r_, b_).sum()) >= 32, (name, h, row)
        assert under_the_gate >= 12, (name, under_the_gate)    # measured on this emulation: 17 / 18 / 22 of 36


def test_attention_backward_shared_query_set_and_fp32_arithmetic_forms():
    """shared: dQ is the sum over the batches of per-batch results (each rounded); p_bf16=False: the fp32-arithmetic kernels round
    nothing but D's O and the outputs -- a tighter bound everywhere"""
    got, ref, bounds = _bwd_case(2, 3, 100, 100)
    qs = _q(_rand((2, 3, 100, 64), 41, 1.2) * PS)
    k, v, dO = _q(_rand((2, 3, 100, 64), 42, 1.2)), _q(_rand((2, 3, 100, 64), 43)), _q(_rand((2, 3, 100, 64), 44))
    tight = eb.attention_backward(qs.double() / PS, k, v, dO, 64 ** -0.5, p_bf16=False)
    for b_, t_ in zip(bounds, tight):
        assert bool((t_ <= b_).all())
    shared = eb.attention_backward(qs[:1].double() / PS, k, v, dO, 64 ** -0.5, shared=True)
    assert shared[0].shape == (1, 3, 100, 64) and shared[1].shape == (2, 3, 100, 64)


# ------------------------------------------------------------------------------------------- q|k|v heads, elementwise GELU
@pytest.mark.parametrize("norm,two_pass", [(True, False), (True, True), (False, False), (False, True)])
def test_qkv_heads_bound_fused_and_two_pass(norm, two_pass):
    """emulation: fp32 a w^T + b, (two-pass: rounded to bf16,) fp32 per-head RMSNorm and q pre-scale, one bf16 rounding"""
    M, H, K = 300, 3, 192
    C = H * 64
    a, w, bias = _q(_rand((M, K), 91)), _q(_rand((C, K), 92, 0.1)), _rand((C,), 93)
    nw = 1 + 0.1 * _rand((64,), 94) if norm else None
    y = a @ w.T + bias
    if two_pass:
        y = y.to(BF).float()
    y = y.reshape(M, H, 64)
    if norm:
        y = y * torch.rsqrt((y * y).mean(-1, keepdim=True) + 1e-5) * nw
    out = (y * PS).to(BF).float().reshape(M, C)
    r = (a.double() @ w.double().T + bias.double()).reshape(M, H, 64)
    if norm:
        r = r * torch.rsqrt((r * r).mean(-1, keepdim=True) + 1e-5) * nw.double()
    ref = (r * PS).reshape(M, C)
    bound = eb.qkv_heads(a, w, bias=bias, norm_w=nw, eps=1e-5, scale=PS, two_pass=two_pass)
    assert 0.3 < eb.assert_within(out, ref, bound, f"qkv heads norm={norm} two_pass={two_pass}") <= 1.0
    with pytest.raises(AssertionError):
        eb.assert_within(_run_holds_previous(out, M - 1, C - 8, 8), ref, bound, "chunk")
    bad = out.clone()
    bad[M - 1, -64:] = out[M - 2, -64:]
    assert int(eb.violations(bad, ref, bound).sum()) >= 32
    if not two_pass:                                           # the fused form must not pass as the two-pass one's bound is looser
        assert bool((bound <= eb.qkv_heads(a, w, bias=bias, norm_w=nw, eps=1e-5, scale=PS, two_pass=True)).all())


def test_rmsnorm_heads_and_elementwise_gelu_bounds():
    x = _q(_rand((2, 100, 3, 64), 16))
    w = 1 + 0.1 * _rand((64,), 17)
    out = (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-5) * w * 0.25).to(BF).float()
    xd = x.double()
    ref = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-5) * w.double() * 0.25
    bound = eb.rmsnorm_heads(x, w, 1e-5, 0.25)
    assert 0.3 < eb.assert_within(out, ref, bound, "rmsnorm heads") <= 1.0
    bad = out.clone()
    bad[1, 99, 2] = out[1, 98, 2]
    assert int(eb.violations(bad, ref, bound).sum()) >= 32
    z, dh = _q(_rand((1000, 64), 3, 2.0)), _q(_rand((1000, 64), 4))
    zt = z.double().requires_grad_(True)
    h = torch.nn.functional.gelu(zt)
    h.backward(dh.double())
    z32 = z.clone().requires_grad_(True)
    h32 = torch.nn.functional.gelu(z32)
    h32.backward(dh)
    assert 0.3 < eb.assert_within(h32.detach().to(BF).float(), h.detach(), eb.gelu_elementwise(z), "gelu") <= 1.0
    assert 0.3 < eb.assert_within(z32.grad.to(BF).float(), zt.grad, eb.gelu_backward(z, dh), "gelu backward") <= 1.0
    with pytest.raises(AssertionError):
        eb.assert_within(_run_holds_previous(z32.grad.to(BF).float(), 999, 56, 8), zt.grad, eb.gelu_backward(z, dh), "chunk")


# ------------------------------------------------------------------------------------------- second GELU product, RMSNorm backward
def test_gemm_mul_gelu_grad_bound():
    """emulation: fp32 dy w^T times fp32 gelu'(z) of the stored bf16 z, one rounding; and the documented polynomial error"""
    M, N, K = 300, 328, 192
    dy, w = _q(_rand((M, K), 34)), _q(_rand((N, K), 32, 0.1))
    z = _q(_rand((M, N), 35, 1.7))
    z32 = z.clone()
    d32 = 0.5 * (1 + torch.erf(z32 * 0.70710678118654752440)) + z32 * torch.exp(-0.5 * z32 * z32) * 0.39894228040143267794
    out = ((dy @ w.T) * d32).to(BF).float()
    ref = (dy.double() @ w.double().T) * eb.gelu_grad(z.double())
    bound = eb.gemm_mul_gelu_grad(dy, w, z)
    assert 0.3 < eb.assert_within(out, ref, bound, "product with gelu'(z)") <= 1.0
    off = ((dy.double() @ w.double().T) * (eb.gelu_grad(z.double()) + 0.5 * 1.7e-5)).to(BF)       # Phi off by the documented figure
    assert eb.assert_within(off, ref, bound, "documented polynomial error") <= 1.0
    with pytest.raises(AssertionError):
        eb.assert_within(_run_holds_previous(out, M - 1, N - 8, 8), ref, bound, "chunk")
    bad = out.clone()
    bad[M - 1] = 7.0
    assert int(eb.violations(bad, ref, bound).sum()) >= N - 2


def test_rmsnorm_heads_backward_bound():
    """emulation of qkv_split_bwd_kernel: fp32 r, xh, g, m = mean(g xh), dx = r (g - xh m), bf16 out; against fp64 autograd"""
    B, L, H = 2, 100, 3
    x, dy, w = _q(_rand((B, L, H, 64), 15)), _q(_rand((B, L, H, 64), 18)), 1 + 0.1 * _rand((64,), 16)
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-5)
    xh, g = x * r, dy * w
    out = (r * (g - xh * (g * xh).mean(-1, keepdim=True))).to(BF).float()
    xd = x.double().requires_grad_(True)
    (xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-5) * w.double() * dy.double()).sum().backward()
    bound = eb.rmsnorm_heads_backward(x, dy, w, 1e-5)
    assert 0.3 < eb.assert_within(out, xd.grad, bound, "rmsnorm backward") <= 1.0
    bad = out.clone()
    bad[1, 99, 2] = out[1, 98, 2]                              # (b) a (row, head) vector holding the previous row's
    assert int(eb.violations(bad, xd.grad, bound).sum()) >= 32
    bad = out.clone()
    bad[1, 99, 2, 56:] = out[1, 99, 2, 48:56]                  # (a)
    with pytest.raises(AssertionError):
        eb.assert_within(bad, xd.grad, bound, "chunk")
    bad = out.clone()
    bad[0, 0, 0, 0] = float("nan")                             # (c)
    with pytest.raises(AssertionError, match="1 of"):
        eb.assert_within(bad, xd.grad, bound, "nan")
    assert eb.assert_within(dy.to(BF).float(), dy.double(), eb.rmsnorm_heads_backward(x, dy, None, 1e-5), "no norm: dx = dy") == 0.0


# ------------------------------------------------------------------------------------------- patch rows, point features
@pytest.mark.parametrize("Hin", [64, 224, 512])
def test_patchify_bound(Hin):
    """emulation: fp32 bilinear resize + normalisation + im2col, one bf16 rounding; reference the same in fp64"""
    Fr, size, patch = 2, 224, 14
    video = torch.rand((Fr, Hin, Hin, 3), generator=torch.Generator().manual_seed(31))
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)

    def rows(v, m, s_):
        img = torch.nn.functional.interpolate(v.permute(0, 3, 1, 2), (size, size), mode="bilinear", align_corners=False)
        return torch.nn.functional.unfold((img - m) / s_, kernel_size=patch, stride=patch).transpose(1, 2).reshape(Fr * 256, 588)
    out, ref = rows(video, mean, std).to(BF).float(), rows(video.double(), mean.double(), std.double())
    bound = eb.patchify(ref, Hin)
    assert 0.3 < eb.assert_within(out, ref, bound, f"patch rows from {Hin} x {Hin}") <= 1.0
    # the coordinate term is the same absolute figure for every element (1.1e-3 at Hin = 512): faults must still be caught
    g = torch.Generator().manual_seed(9)
    caught = 0
    for r, c0 in zip(torch.randint(0, Fr * 256, (500,), generator=g).tolist() + [Fr * 256 - 1],
                     (torch.randint(1, 588 // 8, (500,), generator=g) * 8).tolist() + [580]):     # (a): 588 = 73 chunks and a half
        caught += int(eb.violations(out[r, c0 - 8:c0], ref[r, c0:c0 + 8], bound[r, c0:c0 + 8]).sum()) >= 1
    assert caught == 501
    bad = out.clone()
    bad[-1, 5] = float("nan")                                  # (c)
    with pytest.raises(AssertionError, match="1 of"):
        eb.assert_within(bad, ref, bound, "nan")
    bad = out.clone()
    bad[-1] = 7.0                                              # (d)
    assert int(eb.violations(bad, ref, bound).sum()) == 588
    bad = out.clone()
    bad[-1] = out[-2]                                          # a patch row holding its neighbour's pixels
    assert int(eb.violations(bad, ref, bound).sum()) >= 500


def test_point_encode_bound():
    """emulation: fp32 products xyz * 2^j pi, fp32 sin / cos, bf16 store"""
    P = 333
    xyz = torch.rand((P, 3), generator=torch.Generator().manual_seed(32)) - 0.5
    e = (2.0 ** torch.arange(8, dtype=torch.float32)) * math.pi
    proj = torch.cat([xyz[:, i:i + 1] * e for i in range(3)], dim=1)
    out = torch.cat([proj.sin(), proj.cos(), xyz], dim=1).to(BF).float()
    ref = torch.cat([proj.double().sin(), proj.double().cos(), xyz.double()], dim=1)
    bound = eb.point_encode(proj, ref)
    assert 0.3 < eb.assert_within(out, ref, bound, "point features") <= 1.0
    for r in range(0, P, 7):                                   # (a) 16-byte runs: 51 columns = 6 chunks and three values
        for c0 in range(8, 48, 8):
            assert int(eb.violations(out[r, c0 - 8:c0], ref[r, c0:c0 + 8], bound[r, c0:c0 + 8]).sum()) >= 1, (r, c0)
    bad = out.clone()
    bad[P - 1, 50] = float("nan")                              # (c)
    with pytest.raises(AssertionError, match="1 of"):
        eb.assert_within(bad, ref, bound, "nan")
    bad = out.clone()
    bad[P - 1] = 7.0                                           # (d)
    assert int(eb.violations(bad, ref, bound).sum()) == 51
    bad = out.clone()
    bad[P - 1] = out[P - 2]
    assert int(eb.violations(bad, ref, bound).sum()) >= 40


# ------------------------------------------------------------------------------------------- the optimizer step
def _adamw_check(n, step, gs, form, fma, seed, wd=oc.HYPER["weight_decay"], emu_wd=None, fault=None):
    """The emulation (decay `emu_wd`, default `wd`; with `fault`, if any) next to the reference and the bound of the CORRECT update
    with decay `wd` (a scalar or one value per element).  Returns (outs, refs, bounds), each (p', m', v')."""
    p, g, m, v = oc.adamw_inputs(n, step, seed)
    hp = dict(oc.HYPER, step=step, weight_decay=wd, grad_scale=None if gs is None else eb.f32(gs))
    refs, bounds = eb.adamw_reference(p, g, m, v, **hp), eb.adamw_step(p, g, m, v, **hp)
    emu_wd = wd if emu_wd is None else emu_wd
    outs = oc.emulate(p.numpy(), g.numpy(), m.numpy(), v.numpy(), form=form, fma=fma, fault=fault,
                      **dict(hp, grad_scale=gs, weight_decay=emu_wd.numpy() if torch.is_tensor(emu_wd) else emu_wd))
    return outs, refs, bounds


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("form", ["divide", "reciprocal"])
def test_adamw_bound_holds_for_both_kernel_forms(form, fma):
    """soundness: the fp32 emulation of adamw_kernel (divide) and adamw_flat_kernel (reciprocal), contracted or not, inside the
    bound for p', m' and v' at every step count and gradient scale the GPU tests use"""
    worst = [0.0, 0.0, 0.0]
    for step in oc.STEPS:
        for gs in oc.GRAD_SCALES:
            outs, refs, bounds = _adamw_check(20000, step, gs, form, fma, seed=100 + step)
            for i, what in enumerate(("p'", "m'", "v'")):
                worst[i] = max(worst[i], eb.assert_within(outs[i], refs[i], bounds[i], f"{what} step {step} gs {gs} {form} fma={fma}"))
    print('worst err / bound (p, m, v):', worst)
    assert all(0.2 < w <= 1.0 for w in worst), worst            # sound, and not so loose that it could hide a lost rounding


def test_adamw_bound_does_not_depend_on_subnormal_flushing():
    """gradients so small that (1 - b2) g^2 is subnormal or zero: the emulation with gradual underflow and the same results with
    every subnormal flushed to zero are both inside the bound (its floor of a few smallest normals)"""
    n = 4096
    p, _, m, v = oc.adamw_inputs(n, 2, 7)
    g = (10.0 ** (-22 + 4 * torch.rand(n, generator=torch.Generator().manual_seed(8), dtype=torch.float64))).to(torch.float32)
    m, v = torch.zeros(n), torch.zeros(n)
    hp = dict(oc.HYPER, step=1)
    refs, bounds = eb.adamw_reference(p, g, m, v, **hp), eb.adamw_step(p, g, m, v, **hp)
    outs = oc.emulate(p.numpy(), g.numpy(), m.numpy(), v.numpy(), **hp)
    tiny = float(np.finfo(np.float32).tiny)
    assert int((outs[2] < tiny).sum()) > n // 4                  # the case is there
    for i, what in enumerate(("p'", "m'", "v'")):
        eb.assert_within(outs[i], refs[i], bounds[i], what)
        flushed = torch.where(outs[i].abs() < tiny, torch.zeros_like(outs[i]), outs[i])
        eb.assert_within(flushed, refs[i], bounds[i], what + " flushed")


def test_adamw_decay_boundary_fault_hits_four_elements_and_passes_the_norm_gate():
    """the hole this bound closes: weight decay applied to the four elements BEHIND n_decay (a 16-byte unit too many) moves four
    parameters by lr wd = 2e-5 of their value -- exactly those four leave the bound, and `rel_err` over the tensor stays far
    below the 1e-4 the model-level tests ask of a step"""
    n, n_decay = 4096 + 4, 2048
    good_wd, bad_wd = oc.decay_vector(n, n_decay, oc.HYPER["weight_decay"]), oc.decay_vector(n, n_decay + 4, oc.HYPER["weight_decay"])
    for step in (1, 3):
        outs, refs, bounds = _adamw_check(n, step, 0.37, "reciprocal", True, seed=5, wd=good_wd, emu_wd=bad_wd)
        bad = eb.violations(outs[0], refs[0], bounds[0])
        assert bad.nonzero().flatten().tolist() == [n_decay, n_decay + 1, n_decay + 2, n_decay + 3]
        assert rel_err(outs[0], refs[0]) < 1e-4
        assert not eb.violations(outs[1], refs[1], bounds[1]).any() and not eb.violations(outs[2], refs[2], bounds[2]).any()
        # and the other way round: decay missing on the last four of the decay group
        outs, refs, bounds = _adamw_check(n, step, 0.37, "reciprocal", True, seed=5, wd=good_wd,
                                          emu_wd=oc.decay_vector(n, n_decay - 4, oc.HYPER["weight_decay"]))
        assert eb.violations(outs[0], refs[0], bounds[0]).nonzero().flatten().tolist() == list(range(n_decay - 4, n_decay))
        assert rel_err(outs[0], refs[0]) < 1e-4


@pytest.mark.parametrize("fault,steps,gs,which", [("step", (1, 2, 3), 1.0, 0), ("eps_inside", (1, 3, 100), None, 0),
                                                  ("m_factor", (1, 3, 20000), 0.37, 1), ("no_scale", (1, 3, 20000), 0.37, 2)])
def test_adamw_planted_faults_leave_the_bound(fault, steps, gs, which):
    """power: a step count off by one (bias corrections of the next step), eps added under the bias-corrected square root, m'
    without its (1 - b1) factor, grad_scale ignored -- each puts elements of p' (and of the moment it touches) outside"""
    for step in steps:
        for form in ("divide", "reciprocal"):
            outs, refs, bounds = _adamw_check(20000, step, gs, form, False, seed=200 + step, fault=fault)
            n_p = int(eb.violations(outs[0], refs[0], bounds[0]).sum())
            n_w = int(eb.violations(outs[which], refs[which], bounds[which]).sum())
            assert n_p > 200 and n_w > 200, (fault, step, form, n_p, n_w)


def test_sum_of_squares_bound_and_plans():
    """the launch arithmetic of m324_grad_sumsq / m324_mse as the builders reproduce it, and an fp32 emulation of the documented
    summation order (lane sums, butterfly, four waves, final kernel) inside the bound -- a plain 1e-5 * sum is more than four times looser"""
    assert eb.grad_sumsq_plan(1, True) == (False, 1, 1 + 6 + 3 + 1 + 6)
    assert eb.grad_sumsq_plan(4095, True)[:2] == (False, 16) and eb.grad_sumsq_plan(4096, True)[:2] == (True, 1)
    assert eb.grad_sumsq_plan(4096, False)[:2] == (False, 16)
    assert eb.grad_sumsq_plan(4096 + 3, True) == (True, 1, 4 * 4 + 1 + 6 + 3 + 1 + 6)
    vec, grid, depth = eb.grad_sumsq_plan(16_777_216 + 5, True)
    assert (vec, grid) == (True, 1024) and depth == 4 * 17 + 1 + 6 + 3 + 16 + 6       # 4 194 305 units over 262 144 lanes: 17 for lane 0
    assert eb.mse_plan(255) == (1, 1 + 16) and eb.mse_plan(262_144 + 1) == (1024, 2 + 6 + 3 + 16 + 6)
    n = 1_000_003
    x = _rand((n,), 77).numpy()
    _, grid, depth = eb.grad_sumsq_plan(n, False)
    lanes = grid * 256
    sq = np.zeros((-(-n // lanes)) * lanes, dtype=np.float32)
    sq[:n] = x * x
    lane = np.zeros(lanes, dtype=np.float32)
    for row in sq.reshape(-1, lanes):
        lane = lane + row
    w = lane.reshape(grid * 4, 64)
    for s in (1, 2, 4, 8, 16, 32):
        w = w + w[:, np.arange(64) ^ s]
    red = w[:, 0].reshape(grid, 4)
    partial = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    fin = np.zeros(64, dtype=np.float32)
    pp = np.zeros(-(-grid // 64) * 64, dtype=np.float32)
    pp[:grid] = partial
    for row in pp.reshape(-1, 64):
        fin = fin + row
    for s in (1, 2, 4, 8, 16, 32):
        fin = fin + fin[np.arange(64) ^ s]
    want = float((x.astype(np.float64) ** 2).sum())
    bound = eb.sum_of_squares(want, n, depth)
    assert abs(float(fin[0]) - want) <= bound < 1e-5 * want / 4
    assert abs(float(np.float32(want * (1 + 3e-6))) - want) > bound          # a sum that is off by 3e-6 passed the old gate


# ------------------------------------------------------------------------------------------- row, reduction and layout kernels
def _within(out, ref, bound, what):
    return eb.assert_within(out, ref, bound, what)


@pytest.mark.parametrize("C", rc.LN_WIDTHS)
def test_layernorm_and_rowstats_bounds_are_sound_over_the_case_table(C):
    """fp32 emulation (torch's summation order) of every width, with the special rows, fp32 and bf16 inputs"""
    for rows in rc.LN_ROWS:
        w, b = rc.ln_params(C)
        for xdt in (torch.float32, BF):
            x = rc.ln_input(rows, C, dtype=xdt).float()
            for odt, bias, eps in rc.LN_VARIANTS:
                bb = b if bias else None
                _within(rc.emu_layernorm(x, w, bb, eps, odt), rc.ln_reference(x, w, bb, eps), eb.layernorm(x, w, bb, eps, out_dtype=odt),
                        f"layernorm emulation C={C} rows={rows} {odt} bias={bias} eps={eps}")
            for eps in (1e-5, 1e-6):
                got, ref, bnd = rc.emu_rowstats(x, eps), rc.rowstats_reference(x, eps), eb.rowstats(x, eps)
                for k, name in enumerate(("rstd", "-rstd mean")):
                    _within(got[k], ref[k], bnd[k], f"rowstats emulation {name} C={C} rows={rows} eps={eps}")


@pytest.mark.parametrize("ncb", rc.FINISH_NCB)
def test_rowstats_finish_bound_is_sound(ncb):
    for M in rc.FINISH_M:
        for eps in (1e-5, 1e-6):
            part = rc.finish_table(ncb, M)
            got, ref, bnd = rc.emu_rowstats_finish(part, eps), eb.rowstats_finish_reference(part, eps), eb.rowstats_finish(part, eps)
            for k, name in enumerate(("rstd", "-rstd mean")):
                _within(got[k], ref[k], bnd[k], f"rowstats_finish emulation {name} ncb={ncb} M={M}")
            # the bounds still test something: 1e-4 of rstd, and of -rstd mean measured against sqrt((rstd mean)^2 + 1)
            assert float((bnd[0] / ref[0]).max()) < 1e-4 and float((bnd[1] / (ref[1] ** 2 + 1).sqrt()).max()) < 1e-4


@pytest.mark.parametrize("i", [1, 3, 7])
def test_chan_block_merged_with_the_wrong_weight_leaves_the_bound(i):
    """block i of the first half merged with weight 64 in place of 64 i / (i + 1): M2 grows by 64 d^2 / (i + 1)"""
    part = rc.finish_table(16, 257)
    bad = rc.emu_rowstats_finish(part, 1e-5, wrong_weight_block=i)
    ref, bnd = eb.rowstats_finish_reference(part, 1e-5), eb.rowstats_finish(part, 1e-5)
    hit = eb.violations(bad[0], ref[0], bnd[0])
    m = torch.arange(257)
    assert float(hit[m % 4 == 1].double().mean()) > 0.9 and int(hit.sum()) > 128    # nearly every row whose block means differ, and most others


@pytest.mark.parametrize("C", rc.BWD_WIDTHS)
def test_layernorm_backward_bound_is_sound(C):
    for rows in rc.BWD_ROWS:
        w, _ = rc.ln_params(C)
        x = rc.ln_input(rows, C)
        for dt in (torch.float32, BF):
            dy = _q(_rand((rows, C), 77 + C), dt)
            for addend in (None, _rand((rows, C), 78 + C)):
                got = rc.emu_layernorm_bwd(x, w, 1e-5, dy, addend)
                ref = eb.layernorm_backward_reference(x, w, 1e-5, dy, addend)
                bnd = eb.layernorm_backward(x, w, 1e-5, dy, addend)
                for k, name in enumerate(("dx", "dw", "db")):
                    _within(got[k], ref[k], bnd[k], f"layernorm backward emulation {name} C={C} rows={rows} {dt}")


def test_one_rows_dw_contribution_dropped_leaves_the_bound():
    C, rows = 260, 70
    w, _ = rc.ln_params(C)
    x, dy = rc.ln_input(rows, C), _rand((rows, C), 79)
    ref, bnd = eb.layernorm_backward_reference(x, w, 1e-5, dy), eb.layernorm_backward(x, w, 1e-5, dy)
    for row in (0, 33, 69):
        bad = rc.emu_layernorm_bwd(x, w, 1e-5, dy, drop_dw_row=row)
        assert int(eb.violations(bad[1], ref[1], bnd[1]).sum()) >= 0.9 * C, row      # every column but those where the row's term is small by chance
        assert not bool(eb.violations(bad[0], ref[0], bnd[0]).any()) and not bool(eb.violations(bad[2], ref[2], bnd[2]).any())


def test_skipped_slot_in_the_statistics_passes_the_norm_gate_but_not_the_bound():
    """columns 256 i + 4 lane .. + 3 of ONE row missing from the row's two sums (an `if (c < C)` that skips a partly filled slot): at
    the existing test's shape, 77 x 768 with a bf16 output, the Frobenius-norm ratio stays below that test's 4e-3 gate"""
    rows, C, eps = 77, 768, 1e-5
    x = _rand((rows, C), 11) * 3 + 0.5
    w, _ = rc.ln_params(C)
    ref = rc.ln_reference(x, w, None, eps)
    for slot, lane in ((0, 0), (1, 63), (2, 17)):
        skip = (40, 256 * slot + 4 * lane)
        bad = rc.emu_layernorm(x, w, None, eps, BF, skip=skip)
        assert rel_err(bad.float(), ref) < 4e-3
        hit = eb.violations(bad, ref, eb.layernorm(x, w, None, eps))
        assert bool(hit[40].any()) and not bool(hit[:40].any()) and not bool(hit[41:].any())
        st, sref, sb = rc.emu_rowstats(x, eps, skip=skip), rc.rowstats_reference(x, eps), eb.rowstats(x, eps)
        assert bool(eb.violations(st[1], sref[1], sb[1])[40]) and int(eb.violations(st[1], sref[1], sb[1]).sum()) == 1
    # the widths of the new cases: the last, partly filled slot
    for C in (260, 1000):
        x, (w, _) = rc.ln_input(17, C), rc.ln_params(C)
        skip = (5, C - 4)
        bad = rc.emu_layernorm(x, w, None, eps, torch.float32, skip=skip)
        hit = eb.violations(bad, rc.ln_reference(x, w, None, eps), eb.layernorm(x, w, None, eps, out_dtype=torch.float32))
        assert bool(hit[5].any()) and int(hit.any(-1).sum()) == 1


def test_lone_last_row_left_unwritten_leaves_the_bound():
    C, rows = 260, 9
    x, (w, b) = rc.ln_input(rows, C), rc.ln_params(C)
    out = torch.full((rows, C), float("nan"))
    out[:8] = rc.emu_layernorm(x, w, b, 1e-5, torch.float32)[:8]
    hit = eb.violations(out, rc.ln_reference(x, w, b, 1e-5), eb.layernorm(x, w, b, 1e-5, out_dtype=torch.float32))
    assert bool(hit[8].all()) and not bool(hit[:8].any())
    stale = out.clone()
    stale[8] = out[7]                                                      # or holding its neighbour's values
    hit = eb.violations(stale, rc.ln_reference(x, w, b, 1e-5), eb.layernorm(x, w, b, 1e-5, out_dtype=torch.float32))
    assert int(hit[8].sum()) > C - 8


@pytest.mark.parametrize("case,kernel", rc.COLSUM_CASES)
def test_colsum_bound_is_sound_and_rejects_a_group_taken_from_its_neighbour(case, kernel):
    rows, cols, ld, voff = case
    name, depth = eb.colsum_plan(rows, cols, ld, aligned16=(voff == 0), scratch_rows=rc.colsum_scratch_rows(rows))
    assert name == kernel
    for dt in (torch.float32, BF):
        _, x = rc.colsum_input(rows, cols, ld, voff, dt)
        addend = _rand((cols,), 80)
        for add in (None, addend):
            got = rc.emu_colsum(x, 4 if kernel == "colsum" else 1)
            ref = x.double().sum(0)
            if add is not None:
                got, ref = add + got, ref + add.double()
            bnd = eb.colsum(x, depth, add)
            _within(got, ref, bnd, f"colsum emulation {case} {dt}")
            bad = got.clone()
            c0 = (cols // 4 // 2) * 4 + 4 if cols >= 12 else 4
            bad[c0:c0 + 4] = got[c0 - 4:c0]
            assert int(eb.violations(bad, ref, bnd).sum()) >= min(4, cols - c0) - 1, case


def test_colsum_multi_depth_attention_delta_and_rmsnorm_weight_grad_bounds():
    assert eb.colsum_multi_depth([5, 5, 5]) == 7 and eb.colsum_multi_depth([65]) == 20 and eb.colsum_multi_depth([700, 3]) == 44 + 15 + 1
    for B, H, L in rc.DELTA_SHAPES:
        for dt in (torch.float32, BF):
            o, do = _q(_rand((B * L, H, 64), 81), dt), _q(_rand((B * L, H, 64), 82), dt)
            _within((o * do).sum(-1), (o.double() * do.double()).sum(-1), eb.attention_delta(o, do), f"delta emulation {(B, H, L)} {dt}")
    x, dy = _q(_rand((520, 64), 83)), _q(_rand((520, 64), 84))
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-5)
    _, dw = rc.rmsnorm_backward_reference(x, dy, torch.ones(64), 1e-5)
    _within((dy * (x * r)).sum(0), dw, eb.rmsnorm_weight_grad(x, dy, 1e-5), "rmsnorm weight gradient emulation")
    drop = (dy * (x * r))[1:].sum(0)
    assert int(eb.violations(drop, dw, eb.rmsnorm_weight_grad(x, dy, 1e-5)).sum()) >= 56


@pytest.mark.parametrize("gap", [0.0, 30.0])
@pytest.mark.parametrize("n_parts", [2, 3])
def test_merge_parts_bound_is_sound_and_rejects_a_part_weighted_as_its_neighbour(gap, n_parts):
    """fp32 emulation of attention_merge_kernel on synthetic parts; the fault: the last part enters with the first part's weight"""
    B, H, Lq = rc.MERGE_SHAPES[1]
    tok = lambda t: t.permute(0, 2, 1).reshape(B * Lq, H, 1).expand(-1, -1, 64).reshape(B * Lq, H * 64)
    for dt in (torch.float32, BF):
        parts = [_q(_rand((B * Lq, H * 64), 130 + i), dt) for i in range(n_parts)]
        base = _rand((B, H, Lq), 135, 3.0)
        lses = [base + 0.0, base - gap] + ([base - gap] if n_parts == 3 else [])
        ref, bound = eb.merge_parts(parts, lses, out_dtype=dt)
        m = torch.stack(lses).max(0).values
        w = [torch.exp2(l - m) for l in lses]
        inv = 1.0 / sum(w)
        out = sum(tok(wi * inv) * p for wi, p in zip(w, parts)).to(dt).float()
        eb.assert_within(out, ref, bound, f"merge emulation gap={gap} parts={n_parts} {dt}")
        if gap:
            w[-1] = w[0]
            inv = 1.0 / sum(w)
            bad = sum(tok(wi * inv) * p for wi, p in zip(w, parts)).to(dt).float()
            assert float(eb.violations(bad, ref, bound).double().mean()) > 0.95


# ------------------------------------------------------------------------------------------- the weight-gradient GEMM (m324_gemm_tn)
def _tn_emulation(x, y, lengths, order):
    """fp32 per-slice sums of the exact products, then the slices added one after the other in fp32.  order 0: one fp32 matrix
    product per slice; order 1: 32-token pieces from the back of the slice to its front, added one by one"""
    xf, yf = x.float(), y.float()
    total, m = None, 0
    for n in lengths:
        xs, ys = xf[m:m + n], yf[m:m + n]
        if order == 0:
            part = xs.T @ ys
        else:
            part = torch.zeros((x.shape[1], y.shape[1]))
            for b in range((n - 1) // 32 * 32, -1, -32):
                part = part + xs[b:b + 32].T @ ys[b:b + 32]
        total = part if total is None else total + part
        m += n
    return total


@pytest.mark.parametrize("c", wc.TN_CASES, ids=[wc.case_id(c) for c in wc.TN_CASES])
def test_gemm_tn_bound_is_sound(c):
    x, y = wc.gaussian_operands(c.M, c.N, c.Kc, 141)
    used, _, lengths = wc.slice_plan(c.M, c.slices)
    ref, bound = x.double().T @ y.double(), eb.gemm_tn(x, y, used)
    for order in (0, 1):
        eb.assert_within(_tn_emulation(x, y, lengths, order), ref, bound, f"gemm_tn emulation {wc.case_id(c)} order {order}")


@pytest.mark.parametrize("M,N,Kc,slices", [(63, 136, 72, 1), (200, 192, 328, 4), (1000, 136, 72, 5), (1024, 256, 256, 4)])
def test_gemm_tn_bound_rejects_a_dropped_token(M, N, Kc, slices):
    """Operands of magnitude 0.5 .. 1: a token left out of the contraction takes x[m, n] y[m, j], at least 0.25, out of EVERY element,
    and the bound is at most 2 (1024 + 5) 2^-24 1024 < 0.126 for M <= 1024 -- so every element is flagged, by the numbers alone."""
    x, y = wc.away_from_zero(M, N, 142), wc.away_from_zero(M, Kc, 143)
    used, ks, lengths = wc.slice_plan(M, slices)
    ref, bound = x.double().T @ y.double(), eb.gemm_tn(x, y, used)
    assert float(bound.max()) < 0.126 and float(x.float().abs().min() * y.float().abs().min()) >= 0.25
    eb.assert_within(_tn_emulation(x, y, lengths, 0), ref, bound, "unfaulted")
    for m in (0, ks - 1 if used > 1 else M // 2, M - 1):          # the first token, the last of the first slice, the last of all
        keep = torch.ones(M, dtype=torch.bool)
        keep[m] = False
        out = _tn_emulation(x[keep], y[keep], [n - (1 if sum(lengths[:i]) <= m < sum(lengths[:i + 1]) else 0) for i, n in enumerate(lengths)], 0)
        assert bool(eb.violations(out, ref, bound).all()), (M, N, Kc, m)
