"""Per-element forward error bounds for the bf16 kernel parity checks (derivations: tests/ERROR_BOUNDS.md).

Every builder returns a tensor shaped like the kernel's output that bounds |kernel - fp64 reference| element by element.  The
bounds are derived from the operation's arithmetic and the rounding points the kernels document (include/m324.h, the kernel
comments cited below), never fitted to kernel output.  The only free multipliers are: 2 on fp32 accumulation terms (the MFMA's
internal summation order and rounding are not documented), 1.01 on the output rounding, 4 on transcendental evaluations.
Everything here is fp64 torch on the CPU; the operands are the values the kernel reads (already rounded to its operand dtype).
"""
import math

import torch

U16 = 2.0 ** -8            # unit roundoff of bf16 (8-bit significand, round to nearest even)
U32 = 2.0 ** -24           # unit roundoff of fp32
EXP2 = 4 * U32             # one device exp2 / exp / log2 evaluation
GELU_LIPSCHITZ = 1.13      # max |gelu'(z)| (attained near z = 1.41: 1.1289)
GELU2_LIPSCHITZ = 0.8      # max |gelu''(z)| = 2 phi(0) = 0.798
# bf16-output GEMM epilogues evaluate erf by an odd minimax polynomial, |erf error| <= 1.7e-5, whose argument is clamped to
# +-3 (x clamped to +-3 sqrt 2): beyond the clamp erf(3) stands in for erf(x / sqrt 2)  (gelu_poly2n and the comment above it, motion324_amd/csrc/gemm_tile.h)
GELU_POLY_ERF = 1.7e-5
GELU_POLY_CLAMP = 3.0
# coefficients of the second polynomial, erf(t) ~ t p(t^2) in gelu_grad<TOUT> (motion324_amd/csrc/gemm_tile.h), highest power first: they
# alternate in sign and their terms reach 30 at |t| = 3 where p = 0.33, so the fp32 Horner evaluation itself loses digits there
GELU_GRAD_POLY = (4.074096087e-08, -1.944782217e-06, 4.105993727e-05, -5.110323815e-04, 4.235408041e-03, -2.510281415e-02,
                  1.110792751e-01, -3.753148415e-01, 1.128268421e+00)
LN2 = math.log(2.0)


# ------------------------------------------------------------------------------------------- the assertion
def _f64(t):
    return t.detach().double().cpu()


def _violations(err, bound):
    return ~(err <= bound)


def _worst_ratio(err, bound):
    if err.numel() == 0:
        return 0.0
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).max())


def violations(out, ref, bound):
    """Boolean mask of the elements that are NOT within the bound.  Written as ~(err <= bound): a NaN in the output (or in the
    bound) and a fill value that was never overwritten count as violations, never as a pass."""
    return _violations((_f64(out) - _f64(ref)).abs(), _f64(bound))


def worst_ratio(out, ref, bound):
    """max over the elements of err / bound (inf where the bound is 0 and the error is not, or where the output is NaN)."""
    return _worst_ratio((_f64(out) - _f64(ref)).abs(), _f64(bound))


def assert_within(out, ref, bound, what):
    """Fails unless EVERY element satisfies |out - ref| <= bound.  Nothing is excluded, masked or sampled.  On failure the message
    holds the count, the worst err / bound and the index of the first violations -- where they lie (a tile edge? the last row?
    one head?) is the diagnostic.  Returns the worst err / bound (a record, not a gate: the gate is 1.0)."""
    out, ref, bound = _f64(out), _f64(ref), _f64(bound)
    assert out.shape == ref.shape == bound.shape, (what, tuple(out.shape), tuple(ref.shape), tuple(bound.shape))
    err = (out - ref).abs()
    bad = _violations(err, bound)
    worst = _worst_ratio(err, bound)
    n_bad = int(bad.sum())
    if n_bad:
        idx = bad.nonzero()[:8]
        first = ", ".join(f"{tuple(int(i) for i in ix)}: got {float(out[tuple(ix)]):.6g} want {float(ref[tuple(ix)]):.6g} "
                          f"(err {float(err[tuple(ix)]):.3g}, bound {float(bound[tuple(ix)]):.3g})" for ix in idx)
        rows = sorted({int(ix[0]) for ix in bad.nonzero()[:4096]})
        raise AssertionError(f"{what}: {n_bad} of {bad.numel()} elements outside their error bound, worst err / bound {worst:.3g}; "
                             f"shape {tuple(out.shape)}; first rows hit {rows[:12]}; first violations {first}")
    return worst


# ------------------------------------------------------------------------------------------- small pieces
def gelu(z):
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def _round_out(val, e, out_dtype):
    """|stored - exact| when the computed value (exact value `val` with error <= e) is stored as out_dtype"""
    if out_dtype == torch.bfloat16:
        return e + 1.01 * U16 * val.abs() + U16 * e            # the rounding acts on the computed value, within e of val
    return e + 2 * U32 * val.abs()


def cast(x, out_dtype=torch.bfloat16):
    """m324_cast and every plain store of an exact fp32 value"""
    return _round_out(x.double(), torch.zeros_like(x, dtype=torch.float64), out_dtype)


def remap_rows(t, gin, gout, off, rows_out):
    """row r of t at row (r // gin) * gout + r % gin + off of a zero tensor with rows_out rows (m324_gemm's row_map: rows that no
    input row maps to are not written, their bound is 0)"""
    out = torch.zeros((rows_out,) + tuple(t.shape[1:]), dtype=t.dtype)
    rows = torch.arange(t.shape[0])
    out[(rows // gin) * gout + rows % gin + off] = t
    return out


def _gelu_eval_error(z, g, out_dtype):
    """error of the device's GELU evaluation at an exact argument: erff for fp32 outputs (gelu_erf, motion324_amd/csrc/common.h); for bf16 outputs the
    polynomial erf, clamped (gelu_poly2n, motion324_amd/csrc/gemm_tile.h) -- GELU(x) = x (1/2 + erf~(x / sqrt 2) / 2)"""
    e = 4 * U32 * (g.abs() + z.abs())
    if out_dtype == torch.bfloat16:
        beyond = (torch.erf(z.abs() / math.sqrt(2.0)) - math.erf(GELU_POLY_CLAMP)).clamp_min(0.0)
        e = e + 0.5 * z.abs() * (GELU_POLY_ERF + beyond)
    return e


# ------------------------------------------------------------------------------------------- GEMM
def gemm(a, w, *, z=None, bias=None, fold=None, act=False, gamma=None, residual=None, out_dtype=torch.bfloat16, extra_ops=0,
         parts=False):
    """m324_gemm (include/m324.h, the comment above m324_gemm_args): v = acc (+ bias) ; gelu ; * gamma ; + residual ; stored as out_dtype.
    a [M, K], w [N, K]: the operand values the kernel reads.  z: the fp64 pre-activation, if the caller has it already
    (a w^T, folded, + bias).  fold = (r0 [M], r1 [M], colsum [N]): the LayerNorm-fold consumer, acc <- r0 acc + r1 colsum
    (ln_fold4, motion324_amd/csrc/gemm_tile.h).  residual: full [M, N] (a broadcast one repeated by the caller); the in-place bf16 stream is the
    bf16 values as they are.  parts=True: returns (value, error before the output rounding) instead of the bound.

    pre-activation: dz = 2 (K + c) U32 (|a| |w|^T + |bias| + ...), the gamma_K bound of an fp32 dot product in any order, c = the
    number of fp32 epilogue operations in front of the activation."""
    a, w = a.detach().double().cpu(), w.detach().double().cpu()
    K = a.shape[1]
    mag = a.abs() @ w.abs().T
    val = a @ w.T if z is None else None
    c = extra_ops
    if fold is not None:
        r0, r1, colsum = (t.detach().double().cpu() for t in fold)
        mag = r0.abs()[:, None] * mag + r1.abs()[:, None] * colsum.abs()[None, :]
        if val is not None:
            val = r0[:, None] * val + r1[:, None] * colsum[None, :]
        c += 3
    if bias is not None:
        bias = bias.detach().double().cpu()
        mag = mag + bias.abs()
        if val is not None:
            val = val + bias
        c += 1
    if z is not None:
        val = z.detach().double().cpu()
    if act:
        e = GELU_LIPSCHITZ * (2 * (K + c) * U32 * mag)
        g = gelu(val)
        e = e + _gelu_eval_error(val, g, out_dtype)
        val = g
        if gamma is not None:
            gamma = gamma.detach().double().cpu()
            val = val * gamma
            e = e * gamma.abs() + 2 * U32 * val.abs()
        if residual is not None:
            residual = residual.detach().double().cpu()
            e = e + 2 * U32 * (val.abs() + residual.abs())
            val = val + residual
    else:                                                   # linear all the way: one gamma_(K + c) term over the magnitudes
        if gamma is not None:
            gamma = gamma.detach().double().cpu()
            mag, val, c = mag * gamma.abs(), val * gamma, c + 1
        if residual is not None:
            residual = residual.detach().double().cpu()
            mag, val, c = mag + residual.abs(), val + residual, c + 1
        e = 2 * (K + c) * U32 * mag
    if parts:
        return val, e
    return _round_out(val, e, out_dtype)


def gemm_gelu_grad_store(a, w, *, z, bias=None):
    """M324_AUX_STORE_GELU_GRAD: aux = gelu'(z) of the fp32 pre-activation, bf16 (gelu_poly2n<N, GRAD>, motion324_amd/csrc/gemm_tile.h: the polynomial erf of
    the GELU next to it, and one exp2)."""
    zv, dz = gemm(a, w, z=z, bias=bias, parts=True)
    d = gelu_grad(zv)
    pdf = torch.exp(-0.5 * zv * zv) / math.sqrt(2 * math.pi)
    beyond = (torch.erf(zv.abs() / math.sqrt(2.0)) - math.erf(GELU_POLY_CLAMP)).clamp_min(0.0)
    # Phi by the polynomial; z phi(z): exp2 of an argument with relative error 2 U32 (absolute z^2 U32 ln-domain), two products
    e = GELU2_LIPSCHITZ * dz + 0.5 * (GELU_POLY_ERF + beyond) + (EXP2 + (zv * zv + 4) * U32) * (zv * pdf).abs() + 4 * U32 * d.abs()
    return _round_out(d, e, torch.bfloat16)


def gemm_mul_gelu_grad(dy, w, z):
    """M324_AUX_MUL_GELU_GRAD: (dy w^T) gelu'(z) with z the STORED bf16 pre-activation (exact operand).  bf16 outputs evaluate
    gelu' in gelu_grad<TOUT> (motion324_amd/csrc/gemm_tile.h): Phi by a second polynomial erf with the argument clamped at +-3,
    |erf error| <= 1.7e-5 (stated next to its coefficients), and phi by one exp2 whose argument carries a relative (z^2 + 4) U32.
    The polynomial is evaluated by nine fp32 FMAs: 2 * 9 U32 sum_k |c_k| t^2k (Horner's bound with the factor 2), times |t| / 2 on
    Phi -- 2.4e-4 at the clamp, nothing in the middle.  Found on the MI355X: without it 698 of 393216 elements of
    test_gemm_training_aux_operand[512-768-256] with |gelu'(z)| ~ 1e-4 (z near -4.2) lay up to 1.57x outside the bound; a CPU
    emulation of the same FMAs puts |Phi error| at 1.65e-5 there, twice the polynomial's own 0.83e-5."""
    acc, e_acc = gemm(dy, w, extra_ops=1, parts=True)
    z = _f64(z)
    d = gelu_grad(z)
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    beyond = (torch.erf(z.abs() / math.sqrt(2.0)) - math.erf(GELU_POLY_CLAMP)).clamp_min(0.0)
    t2 = (z * z / 2).clamp_max(GELU_POLY_CLAMP ** 2)
    horner = 2 * len(GELU_GRAD_POLY) * U32 * sum(abs(c) * t2 ** (len(GELU_GRAD_POLY) - 1 - i) for i, c in enumerate(GELU_GRAD_POLY))
    e_d = 0.5 * (GELU_POLY_ERF + beyond + t2.sqrt() * horner) + (EXP2 + (z * z + 4) * U32) * (z * pdf).abs() + 4 * U32 * d.abs()
    return _round_out(acc * d, e_acc * d.abs() + acc.abs() * e_d + 2 * U32 * (acc * d).abs(), torch.bfloat16)


def n3_head(a, w, bias, w3, b3, *, z=None, fold=None):
    """M324_AUX_N3 + m324_n3_finish: out[M, 3] fp32 = gelu(a w^T + bias) w3^T + b3, h never rounded to bf16 (the epilogue is the
    bf16-output one: polynomial erf), fp32 sums over N in some order."""
    g, e = gemm(a, w, z=z, bias=bias, fold=fold, act=True, out_dtype=torch.bfloat16, parts=True)
    w3, b3 = w3.detach().double().cpu(), b3.detach().double().cpu()
    N = w3.shape[1]
    val = g @ w3.T + b3
    e = e @ w3.abs().T + 2 * (N + 2) * U32 * (g.abs() @ w3.abs().T + b3.abs())
    return _round_out(val, e, torch.float32)


# ------------------------------------------------------------------------------------------- LayerNorm
def layernorm(x, w, b, eps, out_dtype=torch.bfloat16):
    """m324_layernorm / m324_layernorm_in: y = (x - mean) rsqrt(var + eps) w (+ b), fp32 statistics of the values as read (two
    sums over C in any order: gamma_C with the factor 2), then one output rounding."""
    x, w = x.detach().double().cpu(), w.detach().double().cpu()
    C = x.shape[-1]
    g = 2 * (C + 2) * U32
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    var = (xc * xc).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    dm = g * x.abs().mean(-1, keepdim=True)
    dxc = dm + U32 * xc.abs()
    dvar = 2 * (xc.abs() * dxc).mean(-1, keepdim=True) + (g + 2 * U32) * var
    drstd = rstd * (0.5 * dvar / (var + eps) + EXP2)
    val = xc * rstd * w
    e = w.abs() * (dxc * rstd + xc.abs() * drstd) + 4 * U32 * val.abs()
    if b is not None:
        b = b.detach().double().cpu()
        e = e + 2 * U32 * (val.abs() + b.abs())
        val = val + b
    return _round_out(val, e, out_dtype)


# ------------------------------------------------------------------------------------------- q|k|v heads
def rmsnorm_heads(x, w, eps, scale=1.0, *, dx=None, out_dtype=torch.bfloat16, parts=False):
    """per-head RMSNorm of m324_qkv_split and of the M324_AUX_QKV_HEADS epilogue: y = x rsqrt(mean x^2 + eps) w scale over the
    last dimension (64), fp32 arithmetic on x known to within dx (None: exact operands), one output rounding.
    |d (x_i rsqrt(mean x^2 + eps))| <= (max|dx| / rms) (1 + |x_i| / rms): dx_i / rms directly, and the rms itself moves by at most
    max|dx|  (2 max|dx| / rms for the elements below the rms, more for the few above it)  + the fp32 evaluation: the sum of 64
    squares under a square root (half of its factor-2 gamma), rsqrt, three products.  w = None: no norm, y = x scale."""
    x = x.detach().double().cpu()
    dx = torch.zeros_like(x) if dx is None else dx.detach().double().cpu()
    if w is None:
        val, e = x * scale, dx * abs(scale) + 2 * U32 * (x * scale).abs()
    else:
        w = w.detach().double().cpu()
        n = x.shape[-1]
        rms = torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
        val = x / rms * w * scale
        e = (dx.max(-1, keepdim=True).values / rms) * (1 + x.abs() / rms) * (w * scale).abs() + ((n + 2) * U32 + EXP2 + 6 * U32) * val.abs()
    if parts:
        return val, e
    return _round_out(val, e, out_dtype)


def rmsnorm_heads_backward(x, dy, w, eps, out_dtype=torch.bfloat16):
    """m324_qkv_split_bwd (qkv_split_bwd_kernel, motion324_amd/csrc/backward.hip: "dx = r * (g - xh * mean(g * xh)), g = dy * w,
    xh = x * r"), fp32 on exact operands x, dy [..., 64], one output rounding.  r = rsqrt(mean x^2 + eps) carries the relative
    dr = (n + 2) U32 + EXP2 (half the factor-2 gamma of the sum of squares, the rsqrt); m = mean(g xh) the factor-2 gamma of its
    sum plus dr and the two products of every term.  w = None: dx = dy, stored as it is."""
    x, dy = _f64(x), _f64(dy)
    if w is None:
        return _round_out(dy, torch.zeros_like(dy), out_dtype)
    w = _f64(w)
    n = x.shape[-1]
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    xh, g = x * r, dy * w
    m = (g * xh).mean(-1, keepdim=True)
    dr = (n + 2) * U32 + EXP2
    e_m = (2 * (n + 2) * U32 + dr + 3 * U32) * (g * xh).abs().mean(-1, keepdim=True)
    val = r * (g - xh * m)
    e = r * ((dr + 4 * U32) * (g.abs() + (xh * m).abs()) + xh.abs() * e_m) + (dr + 2 * U32) * val.abs()
    return _round_out(val, e, out_dtype)


def qkv_heads(a, w, *, bias=None, fold=None, norm_w=None, eps=1e-5, scale=1.0, two_pass=False):
    """One of q / k / v of the fused projection, token-major [M, H * 64] in and out (the caller permutes): the GEMM's dz pushed
    through the per-head RMSNorm (norm_w [64] or None) and the q pre-scale, then one bf16 rounding (M324_AUX_QKV_HEADS: both on
    the fp32 accumulators, include/m324.h, m324_gemm_args.qkv_q); two_pass: m324_gemm + m324_qkv_split, one more bf16 rounding before the norm."""
    z, dz = gemm(a, w, bias=bias, fold=fold, parts=True)
    if two_pass:
        dz = _round_out(z, dz, torch.bfloat16)
    M, C = z.shape
    bound = rmsnorm_heads(z.reshape(M, C // 64, 64), norm_w, eps, scale, dx=dz.reshape(M, C // 64, 64))
    return bound.reshape(M, C)


# ------------------------------------------------------------------------------------------- attention
def _attention_terms(q, k, v, scale, p_bf16):
    """q [B or 1, H, Lq, 64], k, v [B, H, Lk, 64] (operand values), scale: what multiplies q . k to give the natural-log-domain
    score (ln 2 for a q that carries scale * log2 e).  Returns p, o, mag = p |v|, the relative error bound of p (dp) and the
    row-wise score error maximum, everything [B, H, Lq, *]."""
    q, k, v = (t.detach().double().cpu() for t in (q, k, v))
    B, Lk = k.shape[0], k.shape[2]
    q = q.expand(B, -1, -1, -1)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    ds = 2 * 66 * U32 * torch.einsum("bhqd,bhkd->bhqk", q.abs(), k.abs()) * scale     # 64 products + the scale and the shift
    dsmax = ds.max(-1, keepdim=True).values
    p = torch.softmax(s, dim=-1)
    lse = torch.logsumexp(s, dim=-1)
    rel = (2 * U16 if p_bf16 else 0.0) + 4 * dsmax + 2 * Lk * U32 + EXP2
    return q, k, v, s, p, lse, dsmax, rel


def attention_and_lse(q, k, v, scale, *, p_bf16=True, out_dtype=torch.bfloat16, extra_roundings=0):
    """m324_attention: O = softmax(q k^T scale) v, token-major [B * Lq, H * 64], and its log2-domain LSE [B, H, Lq].
    Output: 1.01 U16 |O| + (2 U16 + 4 max_k ds + 2 Lk U32 + EXP2) (p |v|).  2 U16: P rounded to bf16 in the numerator
    (pack_bf16x2 of p in attn_bf16_kernel, motion324_amd/csrc/attention.hip; v_cvt_pk_bf16_f32 in gen_attn_pwg.py) and, at worst, in the denominator; ds: the fp32 score error; 2 Lk U32: the fp32
    sums over the keys.  LSE: max_k ds / ln 2 + (Lk U32 + EXP2) / ln 2 + 2 U32 |lse|  (the row sums add the UNROUNDED fp32
    probabilities: rs2 += p in attn_bf16_kernel, v_pk_add_f32 in gen_attn_pwg.py).  extra_roundings: further bf16 roundings of the output."""
    q, k, v, s, p, lse, dsmax, rel = _attention_terms(q, k, v, scale, p_bf16)
    B, H, Lq, Lk = s.shape
    o = torch.einsum("bhqk,bhkd->bhqd", p, v)
    mag = torch.einsum("bhqk,bhkd->bhqd", p, v.abs())
    e = rel * mag
    bound = _round_out(o, e, out_dtype) + extra_roundings * 1.01 * U16 * (o.abs() + e)
    lse2 = lse / LN2
    lse_bound = dsmax[..., 0] / LN2 + (Lk * U32 + EXP2) / LN2 + 2 * U32 * lse2.abs()
    return bound.permute(0, 2, 1, 3).reshape(B * Lq, H * 64), lse_bound


def attention(q, k, v, scale, **kw):
    return attention_and_lse(q, k, v, scale, **kw)[0]


def attention_lse(q, k, scale):
    return attention_and_lse(q, k, k, scale)[1]


def attention_merge(q, k, v, scale, cuts, *, p_bf16=True, out_dtype=torch.bfloat16):
    """m324_attention_merge over the key ranges cuts[i]:cuts[i + 1]: O = sum_i w_i O_i, w_i = 2^(lse_i - lse).  Each part arrives
    with its own attention bound (its output rounding included: one rounding per part) and an LSE within its LSE bound, which
    moves w_i by the relative 2 ln 2 max_i dlse_i (numerator and normalisation); then fp32 sums over the parts and one rounding."""
    q, k, v = (t.detach().double().cpu() for t in (q, k, v))
    B, H, Lq = k.shape[0], k.shape[1], q.shape[2]
    whole = torch.logsumexp(torch.einsum("bhqd,bhkd->bhqk", q.expand(B, -1, -1, -1), k) * scale, dim=-1) / LN2
    e = torch.zeros((B * Lq, H * 64), dtype=torch.float64)
    val = torch.zeros_like(e)
    dl = torch.zeros((B, H, Lq), dtype=torch.float64)
    items = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        kp, vp = k[:, :, lo:hi], v[:, :, lo:hi]
        bnd, lse_b = attention_and_lse(q, kp, vp, scale, p_bf16=p_bf16, out_dtype=out_dtype)
        sp = torch.einsum("bhqd,bhkd->bhqk", q.expand(B, -1, -1, -1), kp) * scale
        op = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(sp, dim=-1), vp).reshape(B * Lq, H * 64)
        wgt = torch.exp2(torch.logsumexp(sp, dim=-1) / LN2 - whole)
        items.append((op, bnd, wgt))
        dl = torch.maximum(dl, lse_b)
    tok = lambda t: t.permute(0, 2, 1).reshape(B * Lq, H, 1).expand(-1, -1, 64).reshape(B * Lq, H * 64)
    drel = tok(2 * LN2 * dl + 2 * EXP2 + 2 * (len(items) + 2) * U32)
    for op, bnd, wgt in items:
        wt = tok(wgt)
        val = val + wt * op
        e = e + wt * (bnd + drel * (op.abs() + bnd))
    return _round_out(val, e, out_dtype)


def attention_backward(q, k, v, dO, scale, *, p_bf16=True, fwd_p_bf16=True, o_bf16=True, out_dtype=torch.bfloat16, shared=False):
    """Bounds for dQ, dK, dV of O = softmax(q k^T scale) v against fp64 autograd.  q is the UNSCALED normalised q [B or 1, H, Lq,
    64] (the kernels read qs = q scale log2 e and hand back d/dq), k, v [B, H, Lk, 64], dO [B, H, Lq, 64].
      dp (relative error of the recomputed P) = 4 max ds + EXP2 + 2 Lk U32;  with P and dS rounded to bf16 once before their
      products (pack_frags of s / dp in attn_bwd_dkv_mfma_kernel and attn_bwd_dq_mfma_kernel, motion324_amd/csrc/attention.hip): r = 2 U16 + dp
      |d dV| <= r (p^T |dO|) + rounding
      D = sum_d O dO is taken from the forward kernel's STORED output (m324_attention_delta: attn_delta_kernel, motion324_amd/csrc/backward.hip), which the
      fp64 reference does not do.  With A_q = sum_d |O_qd| |dO_qd|:  |d D_q| <= (U16 + gamma_64) A_q  (O's output rounding, D's
      own sum)  +  (2 U16 + 4 max ds + EXP2) sum_k p_qk |dP_qk|  +  2 Lk U32 sum_d |dO| (p |v|).  The middle term is the FORWARD's
      rounding of P to bf16 (pack_bf16x2 of p in attn_bf16_kernel) seen through D: a relative error e_k of p_qk moves D by
      sum_d dO_qd sum_k e_k p_qk v_kd = sum_k e_k p_qk dP_qk.
      |d dS_qk| <= p_qk [ r |dP_qk - D_q| + |d D_q| + gamma_64 sum_d |dO_qd| |v_kd| ]
      |d dK| <= scale |d dS|^T |q| + rounding, |d dQ| <= scale |d dS| |k| + rounding
    rounding = one output rounding + the factor-2 gamma term of the final product.  p_bf16=False: the BACKWARD kernel rounds neither
    P nor dS (the fp32-arithmetic attn_bwd_dq_kernel / attn_bwd_dkv_kernel, motion324_amd/csrc/backward.hip); fwd_p_bf16: whether the
    FORWARD kernel that left the stored O rounded its P to bf16 -- independent of the backward kernel's form.  shared: one query set for every batch; dQ is the sum over the batches of the per-batch results."""
    q, k, v, s, p, lse, dsmax, _ = _attention_terms(q, k, v, scale, p_bf16)
    dO = dO.detach().double().cpu()
    B, H, Lq, Lk = s.shape
    dp_rel = 4 * dsmax + EXP2 + 2 * Lk * U32
    r = (2 * U16 if p_bf16 else 0.0) + dp_rel
    g64 = 2 * 66 * U32
    o = torch.einsum("bhqk,bhkd->bhqd", p, v)
    # dV
    dv = torch.einsum("bhqk,bhqd->bhkd", p, dO)
    mag_v = torch.einsum("bhqk,bhqd->bhkd", p, dO.abs())
    e_dv = torch.einsum("bhqk,bhqd->bhkd", r * p, dO.abs()) + 2 * (Lq + 2) * U32 * mag_v
    # dS
    dP = torch.einsum("bhqd,bhkd->bhqk", dO, v)
    e_dP = g64 * torch.einsum("bhqd,bhkd->bhqk", dO.abs(), v.abs())
    D = (o * dO).sum(-1, keepdim=True)
    A = (o.abs() * dO.abs()).sum(-1, keepdim=True)
    fwd_rel = (2 * U16 if fwd_p_bf16 else 0.0) + 4 * dsmax + EXP2                # of every forward p_qk (numerator and normalisation)
    e_D = ((1.01 * U16 if o_bf16 else 2 * U32) + g64) * A + fwd_rel * (p * dP.abs()).sum(-1, keepdim=True) \
        + 2 * Lk * U32 * (dO.abs() * torch.einsum("bhqk,bhkd->bhqd", p, v.abs())).sum(-1, keepdim=True)
    dS = p * (dP - D)
    e_dS = p * (r * (dP - D).abs() + e_D + e_dP)
    # dK, dQ
    dk = scale * torch.einsum("bhqk,bhqd->bhkd", dS, q)
    e_dk = scale * (torch.einsum("bhqk,bhqd->bhkd", e_dS, q.abs()) + 2 * (Lq + 2) * U32 * torch.einsum("bhqk,bhqd->bhkd", dS.abs(), q.abs()))
    dq = scale * torch.einsum("bhqk,bhkd->bhqd", dS, k)
    e_dq = scale * (torch.einsum("bhqk,bhkd->bhqd", e_dS, k.abs()) + 2 * (Lk + 2) * U32 * torch.einsum("bhqk,bhkd->bhqd", dS.abs(), k.abs()))
    b_dq = _round_out(dq, e_dq, out_dtype)
    if shared:
        b_dq = b_dq.sum(0, keepdim=True)
    return b_dq, _round_out(dk, e_dk, out_dtype), _round_out(dv, e_dv, out_dtype)


# ------------------------------------------------------------------------------------------- elementwise GELU
def gelu_elementwise(z, out_dtype=torch.bfloat16):
    """m324_gelu: erff on the stored pre-activation (gelu_fwd_kernel / gelu_fwd8_kernel, motion324_amd/csrc/elementwise.hip), one output rounding"""
    z = z.detach().double().cpu()
    g = gelu(z)
    return _round_out(g, 4 * U32 * (g.abs() + z.abs()), out_dtype)


def gelu_backward(z, dh, out_dtype=torch.bfloat16):
    """m324_gelu_bwd: dz = dh (Phi(z) + z phi(z)), erff and expf (gelu_bwd_kernel / gelu_bwd8_kernel, motion324_amd/csrc/elementwise.hip); the argument of expf carries the
    rounding of z^2 / 2: a relative (z^2 + 4) U32 on phi; Phi = (1 + erf) / 2 is known to an ABSOLUTE 4 U32 (1 + |erf|) / 2 (for
    negative z the sum cancels)"""
    z, dh = z.detach().double().cpu(), dh.detach().double().cpu()
    d = gelu_grad(z)
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2.0)))
    e_d = 4 * U32 * 0.5 * (1 + torch.erf(z / math.sqrt(2.0)).abs()) + (EXP2 + (z * z + 4) * U32) * (d - cdf).abs() + 2 * U32 * d.abs()
    return _round_out(dh * d, dh.abs() * e_d + 2 * U32 * (dh * d).abs(), out_dtype)


# ------------------------------------------------------------------------------------------- patch rows, point features
def patchify(ref, Hin, out_dtype=torch.bfloat16):
    """m324_patchify against an fp64 bilinear resize + normalisation of frames in [0, 1] (patchify_kernel, motion324_amd/csrc/elementwise.hip): the source
    coordinate sh (o + 0.5) - 0.5 <= Hin is formed in fp32 (two roundings, factor 2: 4 U32 Hin on each of the two interpolation
    weights, which multiply tap differences <= 1), ten fp32 operations on values <= 1 + mean, all divided by std >= 0.224."""
    ref = ref.detach().double().cpu()
    e = (2 * 4 * U32 * Hin + 2 * 10 * U32 * 1.485) / 0.224
    return _round_out(ref, torch.full_like(ref, e), out_dtype)


def point_encode(proj, ref, out_dtype=torch.bfloat16):
    """m324_point_encode: sinf / cosf (4 U32 absolute) of an fp32 product known to one rounding (factor 2: 2 U32 |proj|, the
    functions' slope is <= 1); proj = the arguments, ref = [sin | cos | xyz] in fp64; the xyz columns are stored as they are."""
    proj, ref = proj.detach().double().cpu(), ref.detach().double().cpu()
    e = torch.zeros_like(ref)
    n = proj.shape[1]
    e[:, :n] = e[:, n:2 * n] = 4 * U32 + 2 * U32 * proj.abs()
    return _round_out(ref, e, out_dtype)


def linear_n3(a, w, bias):
    """m324_linear_n3 (linear_n3_kernel, motion324_amd/csrc/elementwise.hip): out[M, 3] fp32 = a w^T + bias, a [M, K] the values
    the kernel reads, w [3, K], bias [3].  The longest chain of roundings a product passes through: the four-term dot of one step
    (4: its product and three additions), the lane's running sum over ceil(K / 256) steps, the six butterfly levels of wave_sum
    (motion324_amd/csrc/common.h), the bias addition: (4 + ceil(K / 256) + 6 + 1) U32 (|a| |w|^T + |bias|).  The order is
    known, so the factor 2 of the MFMA sums is not applied; contraction into FMAs only removes roundings.  The output is fp32 and
    the last rounding is the bias addition's: no further term."""
    a, w, bias = _f64(a), _f64(w), _f64(bias)
    K = a.shape[1]
    return (4 + -(-K // 256) + 6 + 1) * U32 * (a.abs() @ w.abs().T + bias.abs())


# ------------------------------------------------------------------------------------------- optimizer step (fp32 throughout)
TINY32 = 2.0 ** -126       # smallest normal fp32: what one operation loses at most when its result (or an operand) is flushed to zero


def _gamma(k):
    """k roundings in a row, (1 + U32)^k - 1 <= k U32 / (1 - k U32)"""
    return k * U32 / (1 - k * U32)


def f32(x):
    """the fp32 value a kernel receives for the Python scalar x (ctypes c_float rounds to nearest), as a Python float"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    gs = 1.0 if grad_scale is None else float(grad_scale)
    wd = _f64(weight_decay) if torch.is_tensor(weight_decay) else f32(weight_decay)
    return f32(lr), f32(beta1), f32(beta2), f32(eps), wd, float(int(step)), gs


def adamw_reference(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=None):
    """One AdamW update in fp64 from the operands the kernels read: fp32 tensors, the fp32 values of the scalars, grad_scale the
    fp32 device scalar's value (None: 1).  weight_decay: a scalar, or a tensor with one value per element (m324_adamw_flat:
    weight_decay in front of n_decay, 0 behind it).  Returns (p', m', v')."""
    p, g, m, v = (_f64(t) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, t, gs = _adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale)
    gc = g * gs
    m2 = b1 * m + (1 - b1) * gc
    v2 = b2 * v + (1 - b2) * gc * gc
    den = v2.sqrt() / math.sqrt(1 - b2 ** t) + eps
    return p * (1 - lr * wd) - lr / (1 - b1 ** t) * m2 / den, m2, v2


def adamw_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=None):
    """m324_adamw and m324_adamw_flat (adamw_kernel, adamw_flat_kernel, motion324_amd/csrc/backward.hip): per-element bounds
    (bp, bm, bv) of one update against adamw_reference, same arguments.  One bound for both kernels -- the first divides by
    bc2_sqrt, the second multiplies by its rounded reciprocal -- with or without contraction of a product and a sum into an FMA
    (that only removes roundings).  Derivation, rounding point by rounding point: tests/ERROR_BOUNDS.md, "The optimizer step"."""
    p, g, m, v = (_f64(t) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, t, gs = _adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale)
    u = U32
    p2, m2, v2 = adamw_reference(p, g, m, v, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, step=step, grad_scale=grad_scale)
    gc = (g * gs).abs()
    # m' = b1 m + (1 - b1) gc: the two products may cancel, so the error is absolute.  b1 m: its product, the sum (2).
    # (1 - b1) gc: g gs, 1 - b1, the product, the sum (4).  Four operations whose result may be flushed.
    e_m = _gamma(2) * b1 * m.abs() + _gamma(4) * (1 - b1) * gc + 4 * TINY32
    # v' = b2 v + ((1 - b2) gc) gc: both terms are >= 0.  b2 v: 2 roundings; the other: g gs counted twice, 1 - b2, two products,
    # the sum (6).
    e_v = _gamma(6) * v2 + 4 * TINY32
    # host: bc1 = 1 - powf(b1, t), bc2_sqrt = sqrtf(1 - powf(b2, t)): 4 U32 on the transcendental, one rounding of the
    # difference, the square root halves what is under it and rounds once
    r_bc1 = 4 * u * b1 ** t / (1 - b1 ** t) + u
    r_bc2s = 0.5 * (4 * u * b2 ** t / (1 - b2 ** t) + u) + u
    bc1, bc2s = 1 - b1 ** t, math.sqrt(1 - b2 ** t)
    # sqrtf(v'): |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|); 2 U32 for the device's sqrtf (1 ulp)
    root = v2.sqrt()
    e_root = torch.minimum(e_v / root.clamp_min(1e-300), e_v.sqrt()) + 2 * u * root
    # D = sqrt(v') / bc2_sqrt + eps: the quotient (1 ulp: 2 U32), or the reciprocal (2 U32) and a product (U32) -> 3 U32; the sum
    e_den = (e_root + (r_bc2s + 3 * u) * root) / bc2s
    den = root / bc2s + eps
    e_den = e_den + u * (den + e_den) + TINY32
    # delta = ((lr / bc1) m') / D: lr / bc1 (2 U32 + r_bc1), the product (U32), the quotient (2 U32)
    theta = (1 + r_bc1 + 2 * u) * (1 + u) * (1 + 2 * u) / (1 - e_den / den) - 1
    delta = lr / bc1 * m2 / den
    e_delta = delta.abs() * theta + (lr / bc1) * e_m / den * (1 + theta) + 2 * TINY32
    # p (1 - lr wd): lr wd, the difference, the product; then the final difference rounds the value it computed
    keep = abs(1 - lr * wd)
    e_keep = u * lr * wd + u * keep * (1 + u)
    e_pk = p.abs() * (e_keep + u * (keep + e_keep)) + TINY32
    e_p = e_pk + e_delta
    e_p = e_p + u * (p2.abs() + e_p) + TINY32
    return e_p, e_m, e_v


def sum_depth(n_per_lane, grid):
    """longest chain of fp32 additions of the two-kernel sums (grad_sanitize_sumsq_kernel + sum_partial_kernel,
    motion324_amd/csrc/backward.hip; mse_partial_kernel + mse_final_kernel, motion324_amd/csrc/elementwise.hip): the lane's own
    running sum, wave_sum's six butterfly steps (motion324_amd/csrc/common.h), red[0] + red[1] + red[2] + red[3], then the final
    kernel's lane sum over ceil(grid / 64) partials and its wave_sum"""
    return n_per_lane + 6 + 3 + -(-grid // 64) + 6


def grad_sumsq_plan(n, aligned16):
    """(vec, grid, depth) of m324_grad_sumsq(n) -- the host arithmetic of motion324_amd/csrc/backward.hip, m324_grad_sumsq:
    `vec = g % 16 == 0 && n >= 4096`, `nb = min(grid_for(vec ? n / 16 : n), 1024)`, grid_for(k) = min(ceil(k / 256), 4096).
    The 16-byte form adds four squares per unit and lane, and lane k < n % 4 of workgroup 0 one more (the tail)."""
    vec = bool(aligned16) and n >= 4096
    k = n // 16 if vec else n
    grid = min(-(-k // 256), 1024)
    if vec:
        per_lane = 4 * -(-(n // 4) // (grid * 256)) + (1 if n % 4 else 0)
    else:
        per_lane = -(-n // (grid * 256))
    return vec, grid, sum_depth(per_lane, grid)


def mse_plan(n):
    """(grid, depth) of m324_mse(n): `nb = min(ceil(n / 256), 1024)` (motion324_amd/csrc/elementwise.hip, m324_mse)"""
    grid = min(-(-n // 256), 1024)
    return grid, sum_depth(-(-n // (grid * 256)), grid)


def sum_of_squares(total, n, depth, *, term_roundings=1, post_roundings=0):
    """|fp32 sum - fp64 sum| for a sum of n non-negative terms whose exact total is `total`: every term carries term_roundings
    roundings of its own (x x: 1; (a - b)^2: 2 for the difference squared, 1 for the product), passes through at most `depth`
    additions (sum_depth), and post_roundings further operations scale the result.  Non-negative terms: the relative errors add,
    gamma_k total; n TINY32 for squares that underflow."""
    return _gamma(depth + term_roundings + post_roundings) * float(total) + n * TINY32


# ------------------------------------------------------------------------------------------- row, reduction and layout kernels
def _two_pass_stats(x, eps):
    """row_stats (motion324_amd/csrc/elementwise.hip): fp32 two-pass mean / rstd of a row held in registers.  Returns the fp64
    values and what the fp32 evaluation may be off by: mean, xc = x - mean, var, rstd and their errors dm, dxc, drstd.
    The sums over C run in an undocumented order across lanes and butterfly levels: gamma_C with the factor 2.  Unlike `layernorm`
    the variance keeps its second-order term mean(dxc^2) (on a constant row it is all there is: the exact variance is 0 and the
    computed one is the square of the mean's error), and the rsqrt is bounded by its exact form 1 / sqrt(1 - t) - 1 for a
    relative error t of its argument, not by the tangent t / 2."""
    C = x.shape[-1]
    g = 2 * (C + 2) * U32
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    var = (xc * xc).mean(-1, keepdim=True)
    dm = g * x.abs().mean(-1, keepdim=True)
    dxc = dm + U32 * xc.abs()
    sq = ((xc.abs() + dxc) ** 2).mean(-1, keepdim=True)               # what the squares may sum to
    dvar = (2 * xc.abs() * dxc + dxc * dxc).mean(-1, keepdim=True) + (g + 2 * U32) * sq + U32 * (sq + eps)
    t = dvar / (var + eps)
    assert float(t.max()) < 0.5, "row statistics: the variance is not known to within half of var + eps"
    rstd = 1.0 / torch.sqrt(var + eps)
    drstd = rstd * ((1.0 / torch.sqrt(1 - t) - 1) * (1 + EXP2) + EXP2)
    return mean, xc, var, rstd, dm, dxc, drstd


def rowstats(x, eps):
    """m324_rowstats (rowstats_kernel): rowstat[m] = (rstd, -rstd mean) by the two-pass statistics.  Returns the two bounds
    [rows] separately: an error of rstd scales every output of the folded consumer, one of -rstd mean shifts it."""
    x = _f64(x)
    mean, _, _, rstd, dm, _, drstd = _two_pass_stats(x, eps)
    b1 = drstd * mean.abs() + (rstd + drstd) * dm + 2 * U32 * (rstd * mean).abs()
    return drstd[:, 0], b1[:, 0]


def rowstats_finish_reference(part, eps):
    """fp64 statement of m324_rowstats_finish: part [ncb, M, 2] = (sum, M2) of blocks of 64 values -> (rstd, -rstd mean) [M]"""
    part = _f64(part)
    ncb = part.shape[0]
    n = 64.0 * ncb
    mean = part[..., 0].sum(0) / n
    m2 = part[..., 1].sum(0) + 64.0 * ((part[..., 0] / 64.0 - mean) ** 2).sum(0)
    rstd = 1.0 / torch.sqrt(m2 / n + eps)
    return rstd, -rstd * mean


def rowstats_finish(part, eps):
    """m324_rowstats_finish (rowstats_finish_kernel): one thread per row, every operation in the order written, so the bound is a
    running error analysis of that code and the factor 2 of the undocumented orders is not applied (as in linear_n3); contraction
    of a product and a sum into an FMA only removes roundings.  Even ncb: each half of the blocks by Chan's update (d = mean_b -
    mean; mean += d / (i + 1); M2 += d^2 64 i / (i + 1) + M2_b), then ln_combine_halves' pairwise form.  Odd ncb: the sum of the
    block sums, then M2 = sum (64 d^2 + M2_b).  e_x below is the absolute error of the computed x.  Returns (b_rstd, b_-rstd mean)."""
    part = _f64(part)
    ncb, M, _ = part.shape
    u = U32
    sx, sy = part[..., 0], part[..., 1]
    n = 64.0 * ncb
    if ncb % 2 == 0:
        h = ncb // 2
        mean, m2, e_mean, e_m2 = [], [], [], []
        for half in range(2):
            mu, q = sx[half * h] / 64.0, sy[half * h].clone()
            e_mu, e_q = torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.float64)
            for i in range(1, h):
                d = sx[half * h + i] / 64.0 - mu
                e_d = e_mu + u * d.abs()
                mu = mu + d / (i + 1)
                e_mu = e_mu + (e_d + u * (d.abs() + e_d)) / (i + 1) + u * (mu.abs() + e_mu + e_d)     # 1 / (i + 1) rounded; the fma
                coef = 64.0 * i / (i + 1)
                T = coef * d * d
                e_T = coef * (2 * d.abs() * e_d + e_d * e_d) + 2 * u * (T + coef * (2 * d.abs() * e_d + e_d * e_d))   # d d, the coefficient
                inner = T + sy[half * h + i]
                e_in = e_T + u * (inner.abs() + e_T)
                q = q + inner
                e_q = e_q + e_in + u * (q.abs() + e_q + e_in)
            mean.append(mu), m2.append(q), e_mean.append(e_mu), e_m2.append(e_q)
        d = mean[1] - mean[0]
        e_d = e_mean[0] + e_mean[1] + u * d.abs()
        ssum = m2[0] + m2[1]
        e_s = e_m2[0] + e_m2[1] + u * (ssum.abs() + e_m2[0] + e_m2[1])
        T = 32.0 * h * d * d
        e_T = 32.0 * h * (2 * d.abs() * e_d + e_d * e_d)
        e_T = e_T + 2 * u * (T + e_T)
        mm2 = ssum + T
        e_mm2 = e_s + e_T + u * (mm2.abs() + e_s + e_T)
        mu = mean[0] + 0.5 * d
        e_mu = e_mean[0] + 0.5 * e_d + u * (mu.abs() + e_mean[0] + e_d)
    else:
        s = sx.sum(0)
        e_s = _gamma(ncb) * sx.abs().sum(0)
        mu = s / n
        e_mu = e_s / n + u * (mu.abs() + e_s / n)
        d = sx / 64.0 - mu
        e_d = e_mu + u * d.abs()
        term = 64.0 * d * d + sy
        e_t = 64.0 * (2 * d.abs() * e_d + e_d * e_d)
        e_t = e_t + u * (term.abs() + e_t)
        mm2 = term.sum(0)
        e_mm2 = e_t.sum(0) + _gamma(ncb) * (term.abs() + e_t).sum(0)
    var = mm2 / n
    dvar = e_mm2 / n + u * (var.abs() + e_mm2 / n)                       # the division
    dvar = dvar + u * (var.abs() + eps + dvar)                          # + eps
    t = dvar / (var + eps)
    assert float(t.max()) < 0.5, "rowstats_finish: the variance is not known to within half of var + eps"
    rstd = 1.0 / torch.sqrt(var + eps)
    drstd = rstd * ((1.0 / torch.sqrt(1 - t) - 1) * (1 + EXP2) + EXP2)
    b1 = drstd * mu.abs() + (rstd + drstd) * e_mu + 2 * u * (rstd * mu).abs()
    return drstd, b1


def layernorm_backward_reference(x, w, eps, dy, addend=None):
    """fp64 statement of m324_layernorm_bwd on compact rows: (dx (+ addend), dw, db)"""
    x, w, dy = _f64(x), _f64(w), _f64(dy)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    xh = xc * rstd
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if addend is not None:
        dx = dx + _f64(addend)
    return dx, (dy * xh).sum(0), dy.sum(0)


def layernorm_backward(x, w, eps, dy, addend=None):
    """m324_layernorm_bwd / _bwd_cast (layernorm_bwd_kernel, motion324_amd/csrc/elementwise.hip: "xh = (x - mean) * rstd ; g = dy * w ;
    dx += rstd * (g - mean(g) - xh * mean(g * xh))"), fp32 on exact operands x [rows, C], dy [rows, C] (compact rows: the caller
    maps them), in the style of rmsnorm_heads_backward.  Statistics as in `rowstats`; xh carries them and two products; the two
    row means are sums over C in an undocumented order (gamma_C with the factor 2); three operations inside the bracket, the
    product with rstd, then the accumulate addend and the fp32 store (2 U32 of the stored value).  dw = sum_rows dy xh and db =
    sum_rows dy pass the wave's running sum, the eight waves' sum through LDS and m324_colsum's levels: the rows in any order,
    gamma_rows with the factor 2.  Returns (b_dx [rows, C], b_dw [C], b_db [C])."""
    x, w, dy = _f64(x), _f64(w), _f64(dy)
    rows, C = x.shape
    gC = 2 * (C + 2) * U32
    _, xc, _, rstd, _, dxc, drstd = _two_pass_stats(x, eps)
    xh = xc * rstd
    e_xh = dxc * rstd + (xc.abs() + dxc) * drstd + 2 * U32 * xh.abs()
    g = dy * w
    e_g = U32 * g.abs()
    s1 = g.mean(-1, keepdim=True)
    e_s1 = (gC + U32) * g.abs().mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    e_s2 = ((g.abs() + e_g) * e_xh).mean(-1, keepdim=True) + (gC + 2 * U32) * (g * xh).abs().mean(-1, keepdim=True)
    inner = g - s1 - xh * s2
    e_in = e_g + e_s1 + xh.abs() * e_s2 + (s2.abs() + e_s2) * e_xh + 3 * U32 * (g.abs() + s1.abs() + (xh * s2).abs())
    val = rstd * inner
    e = rstd * e_in + drstd * (inner.abs() + e_in) + U32 * val.abs()
    if addend is not None:
        val = val + _f64(addend)
    gR = 2 * (rows + 2) * U32
    b_dw = (dy.abs() * e_xh).sum(0) + gR * (dy * xh).abs().sum(0)
    b_db = gR * dy.abs().sum(0)
    return _round_out(val, e, torch.float32), b_dw, b_db


def colsum_plan(rows, cols, ld, aligned16=True, scratch_rows=0):
    """(kernel, depth) of m324_colsum -- the host conditions of the entry point (motion324_amd/csrc/elementwise.hip, m324_colsum)
    and the longest chain of fp32 additions a term passes through in the kernel it selects:
      wide / wide4   (rows <= 64): one thread walks the rows: rows
      plain          (65 .. 255 rows, or no scratch): wave w takes rows w, w + 4, ...: ceil(rows / 4), then red[0] + .. + red[3]: 3
      two-stage      (rows >= 256 with scratch): chunk k of R = min(scratch_rows, 256) takes rows 4 k + w, step 4 R:
                     ceil(rows / (4 R)) + 3, then the wide kernel over the R partial rows: R"""
    v4 = cols % 4 == 0 and ld % 4 == 0 and aligned16
    if scratch_rows > 1 and rows >= 256:
        R = min(scratch_rows, 256)
        return ("colsum_chunk4 + colsum_wide4" if v4 else "colsum_chunk + colsum_wide"), -(-rows // (4 * R)) + 3 + R
    if rows <= 64:
        return ("colsum_wide4" if v4 else "colsum_wide"), rows
    return "colsum", -(-rows // 4) + 3


def colsum_multi_depth(rows_of_chain):
    """longest chain of additions of one destination of m324_colsum_multi (colsum_multi_kernel): a chain with a source of more than
    64 rows takes the tall path for every item -- wave w of 16 walks rows w, w + 16, ..., the sixteen sums are added in order:
    ceil(rows / 16) + 15 -- any other chain the row walk of colsum_wide: rows; every item after the first adds once more."""
    tall = any(r > 64 for r in rows_of_chain)
    return max((-(-r // 16) + 15) if tall else r for r in rows_of_chain) + len(rows_of_chain) - 1


def colsum(x, depth, addend=None):
    """m324_colsum / m324_colsum_multi: out[c] (+)= sum_r x[r][c] -- a sum of exact terms in the kernel's own order, so no factor 2:
    gamma_depth sum |x| with depth from colsum_plan / colsum_multi_depth, plus the rounding of the accumulate addition.
    x [rows, cols]: the values the kernel reads (a list of tensors: the items of a chain)."""
    xs = [_f64(t) for t in (x if isinstance(x, (list, tuple)) else [x])]
    total = sum(t.sum(0) for t in xs)
    e = _gamma(depth) * sum(t.abs().sum(0) for t in xs)
    if addend is not None:
        e = e + U32 * ((total + _f64(addend)).abs() + e)
    return e


def attention_delta(o, do):
    """m324_attention_delta (attn_delta_kernel, motion324_amd/csrc/backward.hip): D = sum over a head's 64 columns of O dO, exact
    operands [..., 64].  A 64-term dot product in a known order: the product (1), the lane's eight additions, the three xor-shuffle
    levels of group8_sum: gamma_12 sum |O dO|."""
    o, do = _f64(o), _f64(do)
    return _gamma(12) * (o * do).abs().sum(-1)


def rmsnorm_weight_grad(x, dy, eps):
    """weight gradient of the per-head RMSNorm (qkv_split_bwd_kernel + m324_colsum): dw[c] = sum over the (token, head) rows of
    dy xh, xh = x r.  xh carries r's relative (n + 2) U32 + EXP2 and one product; the rows are added per lane, across the eight
    rows of a wave, the four waves, the workgroups' partials (m324_colsum): any order, gamma_rows with the factor 2.
    x, dy [rows, 64]."""
    x, dy = _f64(x), _f64(dy)
    rows, n = x.shape
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    t = (dy * x * r).abs().sum(0)
    return ((n + 2) * U32 + EXP2 + 2 * U32 + 2 * (rows + 2) * U32) * t


def merge_parts(parts, lses, out_dtype=torch.bfloat16):
    """m324_attention_merge on GIVEN parts (attention_merge_kernel, motion324_amd/csrc/elementwise.hip): O = sum_i w_i O_i,
    w_i = 2^(l_i - m) / sum_j 2^(l_j - m), exact operands O_i [rows, H 64] and l_i [B, H, Lq] (fp32, log2 domain).  Each weight
    carries the rounding of l_i - m (U32 |l_i - m| ln 2 on the weight), one exp2, the sum of the weights, the reciprocal and a
    product -- twice, for the numerator and the normalisation, as in attention_merge: 2 ln 2 U32 max|l_i - m| + 2 EXP2 +
    2 (n + 2) U32 -- then the fp32 sum over the parts and one output rounding.  Returns (fp64 reference, bound)."""
    parts, lses = [_f64(p) for p in parts], [_f64(l) for l in lses]
    B, H, Lq = lses[0].shape
    tok = lambda t: t.permute(0, 2, 1).reshape(B * Lq, H, 1).expand(-1, -1, 64).reshape(B * Lq, H * 64)
    m = torch.stack(lses).max(0).values
    w = [torch.exp2(l - m) for l in lses]
    tot = sum(w)
    gap = torch.stack([(l - m).abs() for l in lses]).max(0).values
    drel = tok(2 * LN2 * U32 * gap + 2 * EXP2 + 2 * (len(parts) + 2) * U32)
    val = sum(tok(wi / tot) * p for wi, p in zip(w, parts))
    mag = sum(tok(wi / tot) * p.abs() for wi, p in zip(w, parts))
    return val, _round_out(val, drel * mag, out_dtype)


def gemm_tn(x, y, slices):
    """m324_gemm_tn + m324_colsum (the weight gradient dW[n, j] = sum_m x[m, n] y[m, j], bf16 operands [M, N] and [M, Kc], `slices`
    token ranges): the products of two bf16 values are exact in fp32, so what is left is the sum of M exact terms -- inside a slice in
    the MFMA's own order (the factor 2 of this file), the slices - 1 additions of m324_colsum behind it: 2 (M + slices) U32 |x|^T |y|."""
    x, y = _f64(x), _f64(y)
    return 2 * (x.shape[0] + slices) * U32 * (x.abs().T @ y.abs())
