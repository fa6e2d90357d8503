"""Case tables, input builders, fp64 references and fp32 emulations for the row, reduction and layout kernels of
motion324_amd/csrc/elementwise.hip and backward.hip (tests/test_rowkernels_gpu.py on the device, tests/test_rowkernels_cpu.py and
tests/test_error_bounds_cpu.py without one).  Everything here is torch on the CPU.  Each table says which kernel or branch a case
reaches; the shapes are the smallest that reach it.

The LayerNorm family keeps a row as up to four float4 slots per lane (LN_FOR: slot i of lane l holds columns 256 i + 4 l .. + 3):
  C = 4     one lane, one slot                 C = 252   slot 0, lane 63 empty         C = 256   slot 0 full
  C = 260   slot 1 holds lane 0 only           C = 384   slot 1 half filled            C = 1000  slot 3 partly filled (lanes 0 .. 57)
  C = 1024  all four slots full (the backward's 64 KiB of dynamic LDS)
Rows: the forward kernel takes two rows per wave and eight per workgroup (M324_LN_ROWS=1: one and four): 1 = a lone row, 7 = a
workgroup less one (8 k + 7), 9 and 17 = 8 k + 1, a lone last row in a second / third workgroup."""

import torch

import error_bounds as eb

BF = torch.bfloat16
F32 = torch.float32

LN_WIDTHS = (4, 252, 256, 260, 384, 1000, 1024)
LN_ROWS = (1, 7, 9, 17)
ROW_MAP = (3, 7, 2)                      # (gin, gout, off): compact row r <-> stream row (r // 3) * 7 + r % 3 + 2
ROW_MAP_ROWS = 9                         # the lone last row (8) is a mapped row (stream row 18)
# (out dtype, bias, eps): every pair of values of two factors occurs (a covering array of strength 2)
LN_VARIANTS = ((F32, False, 1e-5), (F32, True, 1e-6), (BF, False, 1e-6), (BF, True, 1e-5))
LN_IN_VARIANTS = ((False, 1e-5), (True, 1e-6), (False, 1e-6), (True, 1e-5))       # bf16 input: (bias, eps), output bf16
# the offset of the "mean much larger than std" row: eb.layernorm grows with C |mean|; per width the largest of the existing
# statistics tests' +12 that keeps every element's fp32-output bound below 2^-6 of the row's output RMS (offset_row_condition)
LN_OFFSET = {4: 12.0, 252: 12.0, 256: 12.0, 260: 12.0, 384: 12.0, 1000: 8.0, 1024: 8.0}
GUARD = 8                                # guard rows behind every output

BWD_WIDTHS = (4, 260, 384, 1000, 1024)
BWD_ROWS = (1, 9, 70)                    # 70 rows: direct calls with n_partial 1 and 3 make a wave walk several rows, ragged at the end

FINISH_NCB = (1, 2, 3, 4, 5, 12, 16, 17)
FINISH_M = (1, 255, 257)                 # one thread; a workgroup less one; a second workgroup with one thread


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def mapped_rows(rows, row_map):
    gin, gout, off = row_map
    r = torch.arange(rows)
    return r if gin <= 0 else (r // gin) * gout + r % gin + off


def stream_rows(rows, row_map):
    """rows of the stream a mapped call touches at most, rounded up to whole groups"""
    gin, gout, _ = row_map
    return rows if gin <= 0 else -(-rows // gin) * gout


# ------------------------------------------------------------------------------------------- LayerNorm inputs
SPECIAL_ROWS = ("constant", "zero", "var << eps", "offset")


def special_row_index(rows):
    """where the special rows sit in an input of `rows` rows: constant 1, zero 2, var << eps 3, offset LAST (the lone last row of an
    odd row count); none in a single-row input"""
    if rows < 5:
        return {}
    return {"constant": 1, "zero": 2, "var << eps": 3, "offset": rows - 1}


def ln_input(rows, C, seed=0, dtype=F32):
    x = rand((rows, C), 1000 + 7 * C + rows + seed, 1.3) + 0.2
    sp = special_row_index(rows)
    if sp:
        x[sp["constant"]] = 1.7
        x[sp["zero"]] = 0.0
        x[sp["var << eps"]] = 0.5 + 1e-5 * rand((C,), 5000 + C + seed)      # var ~ 1e-10 << eps
        x[sp["offset"]] = LN_OFFSET[C] + rand((C,), 6000 + C + seed)
    return x.to(dtype)


def ln_params(C, seed=0):
    return 1 + 0.2 * rand((C,), 2000 + C + seed), 0.1 * rand((C,), 3000 + C + seed)


def ln_reference(x, w, b, eps):
    x, w = x.double(), w.double()
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    y = xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps) * w
    return y if b is None else y + b.double()


def offset_row_condition(C, eps=1e-5):
    """max over the offset row's elements of bound / (2^-6 row RMS of the output), fp32 output, from the reference alone"""
    x = (LN_OFFSET[C] + rand((C,), 6000 + C))[None]
    w, b = ln_params(C)
    worst = 0.0
    for bias in (None, b):
        ref = ln_reference(x, w, bias, eps)
        bound = eb.layernorm(x, w, bias, eps, out_dtype=F32)
        worst = max(worst, float(bound.max() / (2.0 ** -6 * ref.pow(2).mean().sqrt())))
    return worst


def rowstats_reference(x, eps):
    x = x.double()
    mean = x.mean(-1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(-1) + eps)
    return rstd, -rstd * mean


# fp32 emulations: torch's fp32 sums are one summation order the kernels could use
def emu_row_stats(x, eps, skip=None):
    """skip = (row, first column): the planted fault -- one float4 slot of one row missing from both sums"""
    x = x.float()
    C = x.shape[-1]
    keep = torch.ones_like(x)
    if skip is not None:
        keep[skip[0], skip[1]:skip[1] + 4] = 0
    mean = (x * keep).sum(-1, keepdim=True) / C
    q = (((x - mean) * keep) ** 2).sum(-1, keepdim=True) / C + torch.tensor(eps, dtype=F32)
    return mean, torch.rsqrt(q)


def emu_layernorm(x, w, b, eps, out_dtype, skip=None):
    mean, rstd = emu_row_stats(x, eps, skip)
    y = (x.float() - mean) * rstd * w
    if b is not None:
        y = y + b
    return y.to(out_dtype)


def emu_rowstats(x, eps, skip=None):
    mean, rstd = emu_row_stats(x, eps, skip)
    return rstd[:, 0], (-rstd * mean)[:, 0]


def emu_layernorm_bwd(x, w, eps, dy, addend=None, drop_dw_row=None):
    """drop_dw_row: the planted fault -- that row's contribution missing from dw"""
    mean, rstd = emu_row_stats(x, eps)
    xh = (x.float() - mean) * rstd
    dy = dy.float()
    g = dy * w
    C = x.shape[-1]
    dx = rstd * (g - g.sum(-1, keepdim=True) / C - xh * ((g * xh).sum(-1, keepdim=True) / C))
    if addend is not None:
        dx = dx + addend
    t = dy * xh
    if drop_dw_row is not None:
        t = t.clone()
        t[drop_dw_row] = 0
    return dx, t.sum(0), dy.sum(0)


# ------------------------------------------------------------------------------------------- m324_rowstats_finish
def finish_table(ncb, M, seed=0):
    """part [ncb, M, 2] fp32 = (sum, M2) of the 64-column blocks of a known fp64 stream, rounded once.  Rows m % 4 == 1 have block
    means that differ strongly (the Chan merge term 64 (mean_b - mean)^2 dominates M2), rows m % 4 == 2 sit on a large common
    mean, row m % 4 == 3 is nearly constant (var << eps)."""
    g = torch.Generator().manual_seed(9000 + 31 * ncb + M + seed)
    x = torch.randn((M, ncb, 64), generator=g, dtype=torch.float64)
    m = torch.arange(M)
    shift = 6.0 * torch.randn((M, ncb, 1), generator=g, dtype=torch.float64)
    x = torch.where((m % 4 == 1)[:, None, None], x + shift, x)
    x = torch.where((m % 4 == 2)[:, None, None], x + 12.0, x)
    x = torch.where((m % 4 == 3)[:, None, None], 0.5 + 1e-5 * x, x)
    s = x.sum(-1)
    m2 = ((x - x.mean(-1, keepdim=True)) ** 2).sum(-1)
    return torch.stack([s, m2], -1).permute(1, 0, 2).contiguous().to(F32)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emu_rowstats_finish(part, eps, wrong_weight_block=None):
    """rowstats_finish_kernel operation by operation in fp32.  wrong_weight_block = i: the planted fault -- block i of the first half
    merged with weight 64 in place of 64 i / (i + 1)"""
    part = part.float()
    ncb, M, _ = part.shape
    sx, sy = part[..., 0], part[..., 1]
    f = lambda v: torch.tensor(v, dtype=F32)
    epsf = f(eps)
    if ncb % 2 == 0:
        h = ncb // 2
        mean, m2 = [], []
        for half in range(2):
            mu, q = sx[half * h] * f(1 / 64), sy[half * h].clone()
            for i in range(1, h):
                d = sx[half * h + i] * f(1 / 64) - mu
                mu = _fma(d, (f(1.0) / f(i + 1)).expand(M), mu)
                coef = f(64.0) * f(i) / f(i + 1)
                if half == 0 and wrong_weight_block == i:
                    coef = f(64.0)
                q = q + _fma(d * d, coef.expand(M), sy[half * h + i])
            mean.append(mu), m2.append(q)
        d = mean[1] - mean[0]
        mm2 = (m2[0] + m2[1]) + (d * d) * (f(32.0) * f(h))
        mu = _fma(f(0.5).expand(M), d, mean[0])
        rstd = torch.rsqrt(mm2 / (f(64.0) * f(ncb)) + epsf)
        return rstd, -rstd * mu
    s = torch.zeros(M, dtype=F32)
    for b in range(ncb):
        s = s + sx[b]
    n = f(64.0) * f(ncb)
    mu = s / n
    q = torch.zeros(M, dtype=F32)
    for b in range(ncb):
        d = sx[b] * f(1 / 64) - mu
        q = q + _fma(f(64.0) * d, d, sy[b])
    rstd = torch.rsqrt(q / n + epsf)
    return rstd, -rstd * mu


# ------------------------------------------------------------------------------------------- column sums
# (rows, cols, ld, view offset in columns) -> the kernel of m324_colsum the case reaches (ops.colsum's scratch: 16 rows from 256 rows on)
COLSUM_CASES = (
    ((64, 8, 8, 0), "colsum_wide4"),                                  # rows <= 64, 4 columns per lane
    ((64, 10, 10, 0), "colsum_wide"),                                 # cols % 4 != 0
    ((5, 260, 264, 1), "colsum_wide"),                                # a view offset by one column: rows not 16-byte aligned
    ((65, 70, 70, 0), "colsum"),                                      # plain: the first row count above the wide kernels
    ((255, 64, 64, 0), "colsum"),                                     # plain: the last row count below the two-stage form
    ((256, 260, 260, 0), "colsum_chunk4 + colsum_wide4"),             # two-stage, a second 256-column workgroup with one lane
    ((300, 1024, 1028, 0), "colsum_chunk4 + colsum_wide4"),           # ld > cols
    ((257, 70, 70, 0), "colsum_chunk + colsum_wide"),                 # two-stage scalar
    ((300, 260, 264, 1), "colsum_chunk + colsum_wide"),               # two-stage on the misaligned view
)


def colsum_scratch_rows(rows):
    """ops.colsum's choice"""
    return 0 if rows < 256 else (256 if rows >= 16384 else (64 if rows >= 2048 else 16))


def colsum_input(rows, cols, ld, voff, dtype, seed=0):
    """(backing [rows, ld], view [rows, cols]) -- the view starts `voff` columns into the backing rows"""
    assert voff + cols <= ld
    base = (rand((rows, ld), 7000 + rows + cols + seed) + 0.3).to(dtype)
    return base, base[:, voff:voff + cols]


def emu_colsum(x, wave_rows=4):
    """fp32: rows r = w, w + wave_rows, ... per partial sum, the partial sums added in order (colsum_kernel's order)"""
    x = x.float()
    parts = [x[w::wave_rows].sum(0) for w in range(wave_rows)]
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


# ------------------------------------------------------------------------------------------- q|k|v split, delta, merge
QKV_SHAPES = ((1, 1, 1), (2, 63, 1), (1, 65, 3), (2, 130, 2))            # (B, L, H): B L H = 1, 126, 195, 520 (token, head) rows:
#   1 and 126 and 195 are no multiples of 8 (clamped lanes in the backward), 520 = 8 * 65 is no multiple of 32 (a ragged last pass);
#   L = 1, 63, 65, 130: one token, a tile less one, a tile plus one, two tiles and two tokens
DELTA_SHAPES = ((1, 1, 1), (2, 3, 5), (1, 2, 33))                        # (B, H, L): 1, 30, 66 rows of 64: one lane group; 3.75 waves-of-8; 8.25
MERGE_SHAPES = ((1, 1, 1), (2, 3, 33))                                   # (B, H, Lq): one thread-octet; 1584 chunks = 6.2 workgroups
Q_SCALES = (1.0, 64 ** -0.5 * 1.4426950408889634)


def rmsnorm_heads_reference(x, w, eps, scale):
    x = x.double()
    if w is None:
        return x * scale
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * w.double() * scale


def head_major(t, B, L, H):
    """token-major [B L, H 64] -> [B, H, L, 64]"""
    return t.reshape(B, L, H, 64).permute(0, 2, 1, 3).contiguous()


def token_major(t):
    B, H, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * 64).contiguous()


def rmsnorm_backward_reference(x, dy, w, eps):
    """fp64: (dx, dw[64]) of y = x r w; x, dy [..., 64]"""
    x, dy = x.double(), dy.double()
    if w is None:
        return dy, None
    w = w.double()
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    xh, g = x * r, dy * w
    return r * (g - xh * (g * xh).mean(-1, keepdim=True)), (dy * xh).reshape(-1, 64).sum(0)


# ------------------------------------------------------------------------------------------- GELU, cast
GELU_Z = (-10.0, -3.0, 0.0, 3.0, 10.0)
# n -> the kernel: n % 8 != 0 scalar (gelu_fwd_kernel / gelu_bwd_kernel), else eight per thread; the last two pass the grid caps
# (4096 workgroups of 256 scalar threads; 8192 x 256 threads x 8 values) so that the grid-stride loops take a second turn
GELU_SMALL = ((1, "scalar"), (7, "scalar"), (1001, "scalar"), (8, "8-wide"), (2048, "8-wide"))
GELU_LARGE = ((4096 * 256 + 3, "scalar, grid-stride"), (8192 * 256 * 8 + 8, "8-wide, grid-stride"))
CAST_COLS = ((1, "cast_kernel"), (8, "cast8_kernel"), (100, "cast_kernel"), (104, "cast8_kernel"))


def gelu_input(n, dtype, seed=0):
    z = rand((n,), 8000 + seed + n % 1000, 2.0)
    k = min(n, len(GELU_Z))
    z[:k] = torch.tensor(GELU_Z[:k])
    if n > 8:
        z[-len(GELU_Z):] = torch.tensor(GELU_Z)             # the special values in the last (grid-stride) elements too
    return z.to(dtype)
