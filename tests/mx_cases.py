"""Shared reference, operand builders and checker of the block-scaled FP8 (MX) kernel tests (include/m324.h, "MX operands";
the method is written up in tests/ERROR_BOUNDS.md, "MX operands").

Everything here is numpy / fp64 on the CPU and independent of the kernels: the e4m3 table and its table-search rounding, the
quantisation rule, and `admissible` / `assert_mx_within`, which turn an fp64 result with a per-element error bound into the
set of MX encodings a correct kernel may produce -- and accept nothing else."""
import functools
import math

import numpy as np
import torch

DEV = "cuda"


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


# ---------------------------------------------------------------------------------------------------- operand builders
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


def _rand_mx(rows, K, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g) * scale
    q, s = mx_quant_ref(x.numpy())
    return q, s


QUANT_SHAPES = [(1, 32), (7, 32), (3, 96), (5, 160), (130, 224), (96, 256)]    # block tails of 1, 7, 9, 25, 14 and 0 (of 64)
# amax with mantissa exactly 1.75 (the last value of a scale: 448 2^X = 1.75 2^(X + 8)), one fp32 ulp below and one above
_MANT = (np.float32(1.75), np.nextafter(np.float32(1.75), np.float32(0)), np.nextafter(np.float32(1.75), np.float32(2)))
_MANT_AMAX = [m * np.float32(2.0 ** e) for e in (-60, 3, 41) for m in _MANT]


def _block_fillers(rng):
    """The special blocks of quant_input, each a function block -> None.  The ones this file adds to _quant_input's ideas come
    last: where a shape has fewer blocks than fillers the later ones overwrite the earlier."""
    def amax_block(a, sign=1.0):
        def fill(b):
            b[:] = rng.uniform(-1, 1, 32).astype(np.float32) * np.float32(a) / 2
            b[int(rng.integers(0, 32))] = np.float32(sign) * np.float32(a)
        return fill

    def put(values):
        def fill(b):
            b[:] = values
        return fill

    def one(value):
        def fill(b):
            b[int(rng.integers(0, 32))] = value
        return fill
    fills = [put(np.float32(0.0)), put((2.0 ** rng.integers(-30, 30, 32)).astype(np.float32)),
             put(np.linspace(-448, 448, 32, dtype=np.float32) / 64), one(np.nan), one(np.inf), one(-np.inf)]
    fills += [amax_block(a) for a in (448.0, 449.0, 447.99997, 512.0, 896.0, 896.0001, 224.0, 3.0e38, 1e-38, 1e-42)]
    fills += [amax_block(a, s) for a, s in zip(_MANT_AMAX, (1, -1, 1, -1, 1, -1, 1, -1, 1))]
    fills += [amax_block(37.5, -1.0), put(np.float32(-0.0))]     # the amax element negative; a block of all -0.0
    return fills


@functools.lru_cache(maxsize=None)
def quant_input(rows, K):
    """fp32 [rows, K] for m324_mx_quant: rows of very different magnitude, and the special blocks spread over the matrix"""
    rng = np.random.default_rng(1000 * rows + K)
    x = (rng.standard_normal((rows, K)) * 2.0 ** rng.integers(-20, 21, (rows, 1))).astype(np.float32)
    nb = K // 32
    total = rows * nb
    fills = _block_fillers(rng)
    step = max(1, total // len(fills))
    for i, fill in enumerate(fills):
        g = (i * step) % total if total >= len(fills) else i % total
        fill(x[g // nb, (g % nb) * 32:(g % nb) * 32 + 32])
    x.setflags(write=False)
    return x


# LayerNorm -> MX: the inputs of tests/test_mx_kernels_gpu.py (randn * 3 + 1.5, seed 3, w = randn * 0.5 + 1, b = randn * 0.1)
LN_SHAPES = [(5, 32), (77, 192), (33, 288), (6, 800), (300, 768), (9, 1024), (1, 768)]
LN_EPS = 1e-6
CAP_ELEMENTS, CAP_BLOCKS = 0.03, 0.01     # at most this share may admit two codes / two scale bytes (conditions on the INPUT)


def ln_input(rows, C):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, C, generator=g) * 3 + 1.5
    w, b = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.1
    return x, w, b


def layernorm64(x, w, b, eps):
    x = x.double()
    xc = x - x.mean(-1, keepdim=True)
    y = xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps) * w.double()
    return y if b is None else y + b.double()


@functools.lru_cache(maxsize=None)
def ln_case(rows, C, with_b):
    """(x, w, b or None, fp64 LayerNorm [rows, C], its fp32 error bound [rows, C]): computed once, shared, never modified"""
    import error_bounds
    x, w, b = ln_input(rows, C)
    b = b if with_b else None
    ref = layernorm64(x, w, b, LN_EPS).numpy()
    err = error_bounds.layernorm(x, w, b, LN_EPS, out_dtype=torch.float32).numpy()
    ref.setflags(write=False)
    err.setflags(write=False)
    return x, w, b, ref, err


# ---------------------------------------------------------------------------------------------------- the checker
def rule_byte(amax):
    """scale byte of the rule for an fp64 amax >= 0 (array): 0 for amax == 0, else X + 127 with X the smallest exponent such
    that amax <= 448 2^X = 1.75 2^(X + 8), clamped to [-127, 127].  frexp: amax = f 2^E exactly, f in [1, 2)."""
    amax = np.asarray(amax, np.float64)
    m, e = np.frexp(amax)                                        # amax = m 2^e, m in [0.5, 1)
    X = np.where(2 * m <= 1.75, e - 1 - 8, e - 1 - 7)
    return np.where(amax == 0, 0, np.clip(X, -127, 127) + 127).astype(np.int64)


def _key(code):
    """e4m3 code -> an integer that orders the codes by value: -0 (0x80) directly below +0 (0x00); NaN codes far outside"""
    code = np.asarray(code).astype(np.int64)
    mag = code & 0x7F
    k = np.where(code & 0x80, -(2 * mag + 1), 2 * mag + 1)
    return np.where(mag == 0x7F, 1 << 20, k)


def admissible(ref64, err):
    """The MX encodings a kernel may produce whose fp32 value y' of every element lies within err of the fp64 result ref64.

    Returns (s_lo, s_hi, code_range):
      s_lo, s_hi [rows, K / 32]: the admissible scale bytes of a block are s_lo .. s_hi, every byte the rule gives for an amax
        in [max_i (|y_i| - e_i)+, max_i (|y_i| + e_i)], the interval the block's computed amax lies in (the rule is monotone in
        amax, so the set is a range).  A block whose reference or bound is not finite admits byte 0xFF only.
      code_range(s) -> (k_lo, k_hi) [rows, K] for ANY choice s [rows, K / 32] of scale bytes (call it with each admissible X):
        the closed range of codes between rne((y - e) 2^-X) and rne((y + e) 2^-X), X = s - 127, as ordered keys (_key).
        Rounding is monotone, so rne(y' 2^-X) lies in it.  A block that can only be all-zero has +0 alone (the rule stores no
        -0 there); a non-finite block has the key of NaN."""
    ref64, err = np.asarray(ref64, np.float64), np.asarray(err, np.float64)
    rows, K = ref64.shape
    nb = K // 32
    a, e = np.abs(ref64).reshape(rows, nb, 32), err.reshape(rows, nb, 32)
    finite = np.all(np.isfinite(a) & np.isfinite(e), axis=2)
    a0, e0 = np.where(finite[..., None], a, 0.0), np.where(finite[..., None], e, 0.0)
    amax_lo, amax_hi = np.maximum(a0 - e0, 0.0).max(axis=2), (a0 + e0).max(axis=2)
    s_lo = np.where(finite, rule_byte(amax_lo), 0xFF)
    s_hi = np.where(finite, rule_byte(amax_hi), 0xFF)
    zero = np.repeat(finite & (amax_hi == 0), 32, axis=1)
    fin_el = np.repeat(finite, 32, axis=1)
    y, ee = np.where(fin_el, ref64, 0.0), np.where(fin_el, err, 0.0)

    def code_range(s):
        s = np.asarray(s).astype(np.int64)
        inv = 2.0 ** -(np.repeat(np.minimum(s, 254), 32, axis=1) - 127.0)
        k_lo = _key(_rne_e4m3(np.clip((y - ee) * inv, -448.0, 448.0)))
        k_hi = _key(_rne_e4m3(np.clip((y + ee) * inv, -448.0, 448.0)))
        k_lo, k_hi = np.where(zero, 1, k_lo), np.where(zero, 1, k_hi)
        return np.where(fin_el, k_lo, 1 << 20), np.where(fin_el, k_hi, 1 << 20)
    return s_lo, s_hi, code_range


def ambiguity(ref64, err):
    """(share of blocks with more than one admissible scale byte, share of elements with more than one admissible code under
    ANY admissible byte) of a reference alone: what the caps CAP_BLOCKS / CAP_ELEMENTS limit"""
    s_lo, s_hi, code_range = admissible(ref64, err)
    multi = np.zeros(np.shape(ref64), bool)
    for d in range(int((s_hi - s_lo).max()) + 1):
        k_lo, k_hi = code_range(np.minimum(s_lo + d, s_hi))
        multi |= k_lo != k_hi
    return float((s_lo != s_hi).mean()), float(multi.mean())


def assert_mx_within(q, s, ref64, err, what):
    """Fails unless the kernel's scale byte of EVERY block is admissible and the code of EVERY element lies in its range for the
    kernel's own scale (admissible()); where a range is one code that is bit equality.  Nothing is excluded or sampled.
    Returns (share of blocks with more than one admissible byte, share of elements with more than one admissible code)."""
    q, s = np.asarray(q, np.uint8), np.asarray(s, np.uint8)
    assert q.shape == np.shape(ref64) == np.shape(err) and s.shape == (q.shape[0], q.shape[1] // 32), (what, q.shape, s.shape)
    s_lo, s_hi, code_range = admissible(ref64, err)
    bad_s = (s < s_lo) | (s > s_hi)
    if bad_s.any():
        at = np.argwhere(bad_s)
        first = ", ".join(f"({r}, {j}): byte {s[r, j]} admissible {s_lo[r, j]}..{s_hi[r, j]}" for r, j in at[:8])
        raise AssertionError(f"{what}: {len(at)} of {s.size} scale bytes not admissible; first {first}")
    k_lo, k_hi = code_range(s)
    k = _key(q)
    bad_q = (k < k_lo) | (k > k_hi) | ((np.repeat(s_lo, 32, axis=1) == 0xFF) & (q != 0x7F))     # NaN is stored as 0x7F, not 0xFF
    if bad_q.any():
        at = np.argwhere(bad_q)
        first = ", ".join(f"({r}, {c}): code 0x{q[r, c]:02X} (key {k[r, c]}) admissible keys {k_lo[r, c]}..{k_hi[r, c]}, "
                          f"reference {np.asarray(ref64)[r, c]:.9g} +- {np.asarray(err)[r, c]:.3g}, scale byte {s[r, c // 32]}"
                          for r, c in at[:8])
        raise AssertionError(f"{what}: {len(at)} of {q.size} element codes outside their admissible range; first {first}")
    return float((s_lo != s_hi).mean()), float((k_lo != k_hi).mean())
