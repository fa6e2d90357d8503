"""Tensor-level wrappers over the libm324 C ABI (motion324_amd/lib.py).

PyTorch is only the owner of device memory and of the HIP stream here; every op below is one
C-ABI call that enqueues hand-written gfx950 kernels on torch's current stream.  All tensors must
live on a HIP device -- there is deliberately no CPU / eager fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import lib as L
from . import switches
from .timing import active as _timing, span

F32, BF16, MXFP8 = L.F32, L.BF16, L.MXFP8
_TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}


def code_of(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise L.M324Error(f"unsupported dtype {dtype}")


def torch_dtype(code: int) -> torch.dtype:
    return _TORCH_DT[code]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _is_device(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda


def _on_device(t, name: str = "") -> None:
    """Refuses whatever is not a HIP device tensor; `name` (the wrapper, or "wrapper: operand") leads the message."""
    if not _is_device(t):
        raise L.M324Error((name + ": " if name else "") + "libm324 ops need HIP device tensors (no CPU fallback on this path)")


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    _on_device(t)
    return t.data_ptr()


def _launch(name: str, *args) -> None:
    """One stream-ordered libm324 call, enqueued on torch's current stream; a failure is reported under the same `name`."""
    L.check(getattr(L.load(), name)(*args, _stream()), name)


def _plan_query(name: str, *args):
    """(count, bytes needed) of a host-only m324_*_plan query: the call returns its count (m324_render_plan has none: 0), or a
    negative status"""
    need = C.c_long(0)
    n = int(getattr(L.load(), name)(*args, C.addressof(need)))
    L.check(0 if n > 0 else n, name)
    return n, int(need.value)


def _row_extent(n: int, gin: int, gout: int, off: int) -> int:
    """rows a row-mapped operand must have for n mapped rows: row m lives at (m // gin) * gout + m % gin + off (gin > 0)"""
    return (n - 1) // gin * gout + (n - 1) % gin + off + 1


def _wrote(*tensors) -> None:
    """libm324 writes through raw pointers: torch's in-place version counters do not see it.  A mark is REQUIRED wherever a
    `_version`-keyed cache can see the written tensor.  The caches, and what covers each:
      backward.Carry (the bf16 twin of a gradient dx): a dx it holds is written only through gemm()'s plain mode and
        layernorm_bwd, and both mark it;
      Prepared's stamps and mirrors (parameters): only the optimizer wrappers (adamw_step, adamw_flat, weight_mirror) write
        them, and those do NOT mark -- optim calls prepared.bump_generation() after its raw writes, which the stamps include;
      _CORNER_CACHE (vertex_corners) and dataset's topology cache (a faces tensor): no kernel writes faces; the geometry,
        surface, framing and render wrappers mark the outputs they return, so a tensor made by one of them is covered.
    Everywhere else a mark is a courtesy, and the set is incomplete: layernorm, attention, rowstats*, cast, colsum(out=),
    gemm(n3=) and the direct gemm_tn(out=) path, among others, write without one.  tests/test_ops_calls_cpu.py pins the set."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def _vec(t: Optional[torch.Tensor], n: int, name: str) -> Optional[int]:
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
        raise L.M324Error(f"{name}: expected contiguous fp32[{n}], got {t.dtype}{tuple(t.shape)}")
    return _p(t)


def _rows(t: torch.Tensor, name: str):
    """2-D view contract: unit inner stride; returns (ptr, leading dimension in elements)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise L.M324Error(f"{name}: expected a 2-D tensor with unit inner stride, got {tuple(t.shape)} {t.stride()}")
    return _p(t), t.stride(0)


def _gemm_query(args):
    """(schedule number, kernel name and grid) of the launch m324_gemm would make for `args`: m324_gemm_plan, host-only"""
    buf = C.create_string_buffer(192)
    schedule = int(L.load().m324_gemm_plan(C.byref(args), buf, 192))
    return schedule, buf.value.decode()


def _gemm_plan(args) -> str:
    return _gemm_query(args)[1]


def gemm_schedule(M: int, N: int, K: int, *, act: int = L.ACT_NONE, out_dtype: torch.dtype = torch.bfloat16, bias: bool = True,
                  fold_merged: bool = False) -> int:
    """The schedule m324_gemm WOULD pick for a bf16 GEMM of this shape and epilogue with the library's live tunables (host-only
    query, m324_gemm_plan: no launch, no device memory touched).  fold_merged: a LayerNorm-fold consumer handed the MERGED
    statistics table.  The host never mirrors the chooser's rules: it asks."""
    args = L.GemmArgs()
    args.A = args.W = args.C = 4096                       # aligned stand-ins: the plan query reads sizes and flags only
    args.M, args.N, args.K, args.lda, args.ldw, args.ldc = M, N, K, K, K, N
    args.in_dtype, args.out_dtype, args.act, args.batch = BF16, code_of(out_dtype), act, 1
    if bias:
        args.bias = 4096
    if fold_merged:
        args.ln_rowstat, args.ln_colsum, args.ln_ncb, args.ln_eps = 4096, 4096, 0, 1e-5
    return _gemm_query(args)[0]


def _attn_plan(B, H, Lq, Lk, flags, dtype_code) -> str:
    buf = C.create_string_buffer(192)
    L.load().m324_attention_plan(B, H, Lq, Lk, flags, dtype_code, buf, 192)
    return buf.value.decode()


def gemm_splitk(a: torch.Tensor, w: torch.Tensor, slices: int) -> torch.Tensor:
    """out[M,N] fp32 = a[M,K] @ w[N,K]^T with the contraction cut into `slices` independent GEMMs launched together
    (grid.y) and summed by m324_colsum: for weight gradients, where M x N is small and K (tokens) is huge."""
    M, K = a.shape
    N = w.shape[0]
    esz = a.element_size()
    tile = 64 if esz == 2 else 32
    ks = (K // tile // slices) * tile
    if slices <= 1 or ks == 0:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
        return gemm(a, w, out)
    main = ks * slices
    part = torch.empty((slices + (1 if main < K else 0), M, N), dtype=torch.float32, device=a.device)
    args = L.GemmArgs()
    args.A, args.lda = _rows(a, "a")
    args.W, args.ldw = _rows(w, "w")
    args.C, args.ldc = _p(part), N
    args.M, args.N, args.K = M, N, ks
    args.in_dtype, args.out_dtype = code_of(a.dtype), F32
    args.batch, args.strideA, args.strideW, args.strideC = slices, ks, ks, M * N
    with span(f"gemm_{'bf16' if esz == 2 else 'f32'}", 2.0 * M * N * main, esz * (M + N) * main + 4.0 * slices * M * N,
              f"split-K M={M} N={N} K={main} slices={slices}" if _timing() else ""):
        _launch("m324_gemm", C.byref(args))
    if main < K:                                        # remainder of the contraction
        gemm(a[:, main:], w[:, main:], part[slices])
    return colsum(part.reshape(part.shape[0], M * N)).reshape(M, N)


def gemm_tn(x: torch.Tensor, y: torch.Tensor, slices: int = 1, out: Optional[torch.Tensor] = None,
            accumulate: bool = False) -> torch.Tensor:
    """out[N, Kc] fp32 = x[M, N]^T @ y[M, Kc] (bf16, token-major operands): the weight gradient dW = dY^T A without
    transposed copies (m324_gemm_tn).  The M tokens are cut into `slices` ranges whose partials m324_colsum adds.
    out: contiguous fp32 [N, Kc] (or any view of N * Kc contiguous floats) that receives the result -- the optimizer's flat
    gradient buffer, so that no copy follows."""
    M, N = x.shape
    Kc = y.shape[1]
    if y.shape[0] != M or x.dtype != torch.bfloat16 or y.dtype != torch.bfloat16:
        raise L.M324Error(f"gemm_tn: x{tuple(x.shape)} {x.dtype} vs y{tuple(y.shape)} {y.dtype} (bf16 operands with equal rows)")
    slices = max(1, min(slices, (M + 63) // 64))
    while slices > 1 and ((M + slices - 1) // slices + 63) // 64 * 64 * (slices - 1) >= M:
        slices -= 1                                   # no empty slice
    if out is not None and (out.dtype != torch.float32 or out.numel() != N * Kc or not out.is_contiguous()):
        raise L.M324Error("gemm_tn: out must be N * Kc contiguous fp32 values")
    # accumulate (out += x^T y: a shared weight's gradient over the decoder's per-sample passes): the slice partials are summed
    # INTO out by the same m324_colsum launch that would have produced a temporary (a single slice goes through it too)
    if accumulate and out is None:
        raise L.M324Error("gemm_tn: accumulate needs out")
    direct = out is not None and slices == 1 and not accumulate
    if direct and COLSUMS.busy(out.view(-1)):
        COLSUMS.flush()
    part = out.view(1, N, Kc) if direct else torch.empty((slices, N, Kc), dtype=torch.float32, device=x.device)
    px, ldx = _rows(x, "x")
    py, ldy = _rows(y, "y")
    with span("gemm_bf16", 2.0 * M * N * Kc, 2.0 * M * (N + Kc) + 4.0 * slices * N * Kc,
              f"TN M={N} N={Kc} K={M} slices={slices}" if _timing() else ""):
        _launch("m324_gemm_tn", px, ldx, py, ldy, _p(part), Kc, M, N, Kc, slices, N * Kc)
    if slices == 1 and not accumulate:
        return out if direct else part[0]
    if out is not None:
        if DEFER_COLSUM:
            # nobody reads a weight gradient before its bucket is declared done (backward.GradStore.done flushes): the sum of the
            # slice partials joins the queue and leaves with the other sums of the block in one m324_colsum_multi launch
            COLSUMS.defer(part.reshape(slices, N * Kc), out.view(-1), accumulate)
            return out
        colsum(part.reshape(slices, N * Kc), out=out.view(-1), accumulate=accumulate)
        _wrote(out)
        return out
    return colsum(part.reshape(slices, N * Kc)).reshape(N, Kc)


class QKVHeads(NamedTuple):
    """gemm(qkv_heads=...), gemm_mx(qkv_heads=...): the fused q|k|v projection is written head-major into Q / K / V
    [B, H, L, 64] with per-head RMSNorm (q_w, k_w: fp32 [64] or None; eps) and the q pre-scale q_scale (M324_AUX_QKV_HEADS);
    the GEMM's `out` is ignored (may be None).  Q None = the k|v projection of a cross-attention, K and V None = its q
    projection.  A V of shape [B, H, 64, L] selects M324_AUX_QKV_HEADS_VT: V leaves transposed and key-permuted, the operand
    attention() reads by default (L % 128 == 0).  vt asks for that form outright; None = V has the transposed shape and L != 64.
    A plain tuple of the first nine or of all ten entries is taken wherever a QKVHeads is."""
    Q: Optional[torch.Tensor]
    K: Optional[torch.Tensor]
    V: Optional[torch.Tensor]
    q_w: Optional[torch.Tensor]
    k_w: Optional[torch.Tensor]
    eps: float
    q_scale: float
    L: int
    H: int
    vt: Optional[bool] = None


def _qkv_heads_args(args, heads, M: int, N: int, who: str) -> torch.Tensor:
    """Validates `heads` (QKVHeads) for a projection of M rows and N columns and fills its part of `args`: C / ldc, the output
    dtype, aux_mode and the qkv_* fields.  Marks the outputs as written and returns the first one given."""
    h = QKVHeads(*heads)
    Bh = M // h.L
    vt = h.vt if h.vt is not None else (h.V is not None and tuple(h.V.shape) == (Bh, h.H, 64, h.L) and h.L != 64)
    outs = [t for t in (h.Q, h.K, h.V) if t is not None]
    for t in outs:
        want = (Bh, h.H, 64, h.L) if (vt and t is h.V) else (Bh, h.H, h.L, 64)
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or tuple(t.shape) != want:
            raise L.M324Error(f"{who}: qkv_heads output {t.dtype}{tuple(t.shape)} (want bf16 {want})")
    if vt and h.L % 64:
        raise L.M324Error(f"{who}: a transposed V output needs L % 64 == 0 (L={h.L})")
    args.C, args.ldc, args.out_dtype = None, N, BF16
    args.aux_mode = 4 if vt else 3
    args.qkv_q, args.qkv_k, args.qkv_v = _p(h.Q), _p(h.K), _p(h.V)
    args.qkv_qw, args.qkv_kw = _vec(h.q_w, 64, "q_w"), _vec(h.k_w, 64, "k_w")
    args.qkv_eps, args.qkv_qscale, args.qkv_L, args.qkv_H = h.eps, h.q_scale, h.L, h.H
    _wrote(*outs)
    return outs[0]


def _gemm_ln_fold(args, a, M: int, N: int, K: int, ln, stats_out, copy_out) -> None:
    """the LayerNorm-fold arguments of gemm(): the consumer's ln (merged 2-tuple or unmerged 3-tuple), the producer's stats_out
    and copy_out"""
    if ln is not None and len(ln) == 3:
        part, colsum, eps = ln                       # the producer's unmerged table: the consumer merges its rows' blocks itself
        if (part.dtype != torch.float32 or not part.is_contiguous() or K % 64 or tuple(part.shape) != (K // 64, M, 2) or a.dtype != torch.bfloat16):
            raise L.M324Error(f"gemm: ln block table {part.dtype}{tuple(part.shape)} (want contiguous fp32 [{K // 64}, {M}, 2], bf16 operands)")
        args.ln_rowstat, args.ln_colsum = _p(part), _vec(colsum, N, "ln colsum")
        args.ln_ncb, args.ln_eps = K // 64, float(eps)
    elif ln is not None:
        rowstat, colsum = ln
        if (rowstat.dtype != torch.float32 or not rowstat.is_contiguous() or rowstat.numel() != 2 * M or a.dtype != torch.bfloat16):
            raise L.M324Error(f"gemm: ln rowstat {rowstat.dtype}{tuple(rowstat.shape)} (want contiguous fp32 [{M}, 2], bf16 operands)")
        args.ln_rowstat, args.ln_colsum = _p(rowstat), _vec(colsum, N, "ln colsum")
    if stats_out is not None:
        if (stats_out.dtype != torch.float32 or not stats_out.is_contiguous() or N % 64 or tuple(stats_out.shape) != (N // 64, M, 2)):
            raise L.M324Error(f"gemm: stats_out {stats_out.dtype}{tuple(stats_out.shape)} (want contiguous fp32 [{N // 64}, {M}, 2])")
        args.ln_stats_out = _p(stats_out)
    if copy_out is not None:
        if copy_out.dtype != torch.bfloat16 or copy_out.shape[0] < M or copy_out.shape[1] < N:
            raise L.M324Error(f"gemm: copy_out {copy_out.dtype}{tuple(copy_out.shape)} (want bf16 [{M}, {N}])")
        args.ln_copy_out, args.ln_ldcopy = _rows(copy_out, "copy_out")


# The three modes of gemm(): each fills the rest of `args` for a[M, K] @ w[N, K]^T and returns (what gemm() returns, span class,
# FLOPs, bytes, the words of the span's tag after the plan -- built only where `tagged`).
def _gemm_heads(args, a, bias, heads, tagged: bool):
    M, N, K = args.M, args.N, args.K
    first = _qkv_heads_args(args, heads, M, N, "gemm")
    args.in_dtype = code_of(a.dtype)
    args.bias = _vec(bias, N, "bias")
    return first, "gemm_bf16", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N), f"M={M} N={N} K={K} qkv-heads" if tagged else ""


def _gemm_n3(args, a, bias, act, gamma, residual, n3, tagged: bool):
    """n3 = (w3 fp32 [3, N], part fp32 [N / 64, M, 3]): gelu(a w^T + bias) is contracted with w3 in the epilogue (M324_AUX_N3);
    `out` is ignored (may be None); finish with n3_finish(part, bias3, out3)"""
    M, N, K = args.M, args.N, args.K
    w3, part = n3
    if (a.dtype != torch.bfloat16 or w3.dtype != torch.float32 or tuple(w3.shape) != (3, N) or not w3.is_contiguous()
            or part.dtype != torch.float32 or tuple(part.shape) != (N // 64, M, 3) or not part.is_contiguous()
            or residual is not None or gamma is not None or act != L.ACT_GELU or N % 256):
        raise L.M324Error(f"gemm: n3 mode needs bf16 operands, act=GELU, N % 256 == 0, w3 [3,{N}] and part [{N // 64},{M},3] fp32")
    args.C, args.ldc = None, N
    args.in_dtype, args.out_dtype = BF16, BF16
    args.bias = _vec(bias, N, "bias")
    args.act = act
    args.aux, args.ldaux, args.aux_mode = _p(part), 3, 5
    args.qkv_qw = _p(w3)
    return (part, "gemm_bf16", 2.0 * M * N * K + 2.0 * M * N * 3, 2.0 * (M * K + N * K) + 4.0 * part.numel(),
            f"M={M} N={N} K={K} gelu n3" if tagged else "")


def _gemm_plain(args, a, out, bias, act, gamma, residual, res_rows, row_map, auxes, tagged: bool):
    """auxes: (preact_out, gelu_grad_of, gelu_grad_out, mul_by), at most one of them given"""
    M, N, K = args.M, args.N, args.K
    args.C, args.ldc = _rows(out, "out")
    _wrote(out)
    args.in_dtype, args.out_dtype = code_of(a.dtype), code_of(out.dtype)
    args.bias = _vec(bias, N, "bias")
    args.act = act
    args.gamma = _vec(gamma, N, "gamma")
    if residual is not None:
        in_place_bf16 = residual.dtype == torch.bfloat16 and out.dtype == torch.bfloat16 and residual.data_ptr() == out.data_ptr()
        if residual.dtype != torch.float32 and not in_place_bf16:
            raise L.M324Error("gemm: residual must be fp32 (or the bf16 output itself, updated in place)")
        args.residual, args.ldr = _rows(residual, "residual")
        args.res_rows = res_rows
    gin, gout, off = row_map
    need = _row_extent(M, gin, gout, off) if gin > 0 else M
    if out.shape[0] < need or out.shape[1] < N:
        raise L.M324Error(f"gemm: out{tuple(out.shape)} too small for {need} x {N}")
    args.row_gin, args.row_gout, args.row_off = gin, gout, off
    auxes = [(t, mode) for t, mode in zip(auxes, (1, 2, 6, 7)) if t is not None]        # M324_AUX_* of the four
    if auxes:
        if len(auxes) > 1:
            raise L.M324Error("gemm: preact_out, gelu_grad_of, gelu_grad_out and mul_by are mutually exclusive")
        aux, mode = auxes[0]
        if aux.dtype != out.dtype or aux.shape[0] < M or aux.shape[1] < N:
            raise L.M324Error(f"gemm: aux operand {aux.dtype}{tuple(aux.shape)} does not match out {out.dtype} [{M}, {N}]")
        args.aux, args.ldaux = _rows(aux, "aux")
        args.aux_mode = mode
    esz = a.element_size()
    # algorithmic bytes: both operands once, the output once, the fp32 residual rows once
    nbytes = esz * (M * K + N * K) + out.element_size() * M * N
    if residual is not None:
        nbytes += residual.element_size() * N * (res_rows if 0 < res_rows < M else M)
    what = "" if not tagged else (
        f"M={M} N={N} K={K}{' bias' if bias is not None else ''}{' gelu' if act else ''}"
        f"{' gamma' if gamma is not None else ''}{' res' if residual is not None else ''} out={'bf16' if out.element_size() == 2 else 'f32'}")
    return out, f"gemm_{'bf16' if esz == 2 else 'f32'}", 2.0 * M * N * K, nbytes, what


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, *, bias=None, act: int = L.ACT_NONE, gamma=None,
         residual: Optional[torch.Tensor] = None, res_rows: int = 0, row_map=(0, 0, 0),
         preact_out: Optional[torch.Tensor] = None, gelu_grad_of: Optional[torch.Tensor] = None,
         gelu_grad_out: Optional[torch.Tensor] = None, mul_by: Optional[torch.Tensor] = None,
         qkv_heads: Optional[tuple] = None, n3: Optional[tuple] = None, ln: Optional[tuple] = None,
         stats_out: Optional[torch.Tensor] = None, copy_out: Optional[torch.Tensor] = None, defer: Optional[list] = None,
         in_rows: Optional[tuple] = None) -> torch.Tensor:
    """out[row_map(m), :N] = epilogue(a[M,K] @ w[N,K]^T); see include/m324.h m324_gemm.
    in_rows = (gin, gout, off) (m324_gemm_rows): M = out.shape[0], and row m reads row (m // gin) * gout + m % gin + off of `a` and
    of `residual`; out, stats_out and copy_out are compact.  Built for the fp32 LayerNorm-statistics producer only.
    preact_out [M, N] (out's dtype) also receives the value the activation is applied to (M324_AUX_STORE_PREACT);
    gelu_grad_of [M, N] = z: the result is multiplied by gelu'(z) (M324_AUX_MUL_GELU_GRAD).  Training only.
    gelu_grad_out [M, N] receives gelu'(pre-activation) (M324_AUX_STORE_GELU_GRAD) and mul_by [M, N] multiplies the result
    (M324_AUX_MUL): the same pair with erf evaluated once, in the forward.
    qkv_heads: a QKVHeads -- the head-major q|k|v outputs replace `out`; n3: see _gemm_n3.
    defer (qkv_heads only): a list that receives the prepared call instead of a launch; gemm_pair(list) then runs two of them
    as ONE launch (m324_gemm_pair).
    LayerNorm fold (include/m324.h): ln = (rowstat fp32 [M, 2], colsum fp32 [N]) -- `a` is the raw stream, `w` carries the
    LayerNorm scale; ln = (part fp32 [K / 64, M, 2], colsum, eps): the producer's stats_out itself, merged by this GEMM; stats_out fp32 [N / 64, M, 2] receives the per-block row statistics of the stored values and copy_out
    bf16 [M, N] their bf16 twin (fp32 `out` only)."""
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or a.dtype != w.dtype:
        raise L.M324Error(f"gemm: a{tuple(a.shape)} {a.dtype} vs w{tuple(w.shape)} {w.dtype}")
    if in_rows is not None:
        gin, gout, off = rows = tuple(int(v) for v in in_rows)
        M = out.shape[0] if out is not None else 0
        src_need = _row_extent(M, gin, gout, off) if gin > 0 and M > 0 else 0
        if (gin <= 0 or M <= 0 or qkv_heads is not None or n3 is not None or residual is None or a.shape[0] < src_need
                or residual.shape[0] < src_need or residual.data_ptr() == out.data_ptr()):
            raise L.M324Error(f"gemm: in_rows {tuple(in_rows)} needs an output of M rows, a and a residual (not the output) of "
                              f"{src_need} rows: a{tuple(a.shape)}")
    args = L.GemmArgs()
    args.A, args.lda = _rows(a, "a")
    args.W, args.ldw = _rows(w, "w")
    args.M, args.N, args.K = M, N, K
    _gemm_ln_fold(args, a, M, N, K, ln, stats_out, copy_out)
    tagged = _timing() or defer is not None
    if qkv_heads is not None:
        ret, cls, flops, nbytes, what = _gemm_heads(args, a, bias, qkv_heads, tagged)
        if defer is not None:                       # gemm_pair() launches it together with another one
            defer.append((args, flops, nbytes, what, (a, w, bias) + tuple(qkv_heads[:5])))        # ... and Q, K, V, q_w, k_w stay alive
            return ret
    elif n3 is not None:
        ret, cls, flops, nbytes, what = _gemm_n3(args, a, bias, act, gamma, residual, n3, tagged)
    else:
        ret, cls, flops, nbytes, what = _gemm_plain(args, a, out, bias, act, gamma, residual, res_rows, row_map,
                                                    (preact_out, gelu_grad_of, gelu_grad_out, mul_by), tagged)
        if copy_out is not None:
            nbytes += 2 * M * N
        if what:
            what += (f"{' ln-fold' if ln is not None else ''}{' ln-stats' if stats_out is not None else ''}"
                     f"{f' in_rows={tuple(in_rows)}' if in_rows else ''}")
    with span(cls, flops, nbytes, f"{_gemm_plan(args)} | {what}" if _timing() else ""):
        if in_rows is not None:
            _launch("m324_gemm_rows", C.byref(args), *rows)
        else:
            _launch("m324_gemm", C.byref(args))
    return ret


class MX(NamedTuple):
    """A block-scaled FP8 operand (include/m324.h, "MX operands"): q uint8 [rows, >= K] OCP e4m3fn element bytes and s uint8
    [rows, >= K / 32] E8M0 scale bytes, one per 32 consecutive K of a row."""
    q: torch.Tensor
    s: torch.Tensor

    @property
    def shape(self):
        return self.q.shape


def mx_empty(rows: int, K: int, device) -> MX:
    """Storage for an MX matrix [rows, K]; scale rows padded to 4 bytes (m324_gemm_mx reads one dword per row and K-tile)."""
    return MX(torch.empty((rows, K), dtype=torch.uint8, device=device),
              torch.empty((rows, (K // 32 + 3) // 4 * 4), dtype=torch.uint8, device=device)[:, :K // 32])


def _mx_rows(t: MX, rows: int, K: int, name: str):
    if (not isinstance(t, MX) or t.q.dtype != torch.uint8 or t.s.dtype != torch.uint8 or t.q.shape[0] < rows or t.q.shape[1] < K
            or t.s.shape[0] < rows or t.s.shape[1] < K // 32):
        raise L.M324Error(f"{name}: expected an MX operand of at least [{rows}, {K}]")
    (pq, lq), (ps, ls) = _rows(t.q, name + ".q"), _rows(t.s, name + ".s")
    return pq, lq, ps, ls


def mx_quant(x: torch.Tensor, out: Optional[MX] = None) -> MX:
    """x fp32 / bf16 [rows, K] (K % 32 == 0) -> MX operand by the rule of include/m324.h (m324_mx_quant)."""
    rows, K = x.shape
    out = mx_empty(rows, K, x.device) if out is None else out
    px, ldx = _rows(x, "x")
    pq, lq, ps, ls = _mx_rows(out, rows, K, "out")
    with span("hbm_pass", 0.0, float(rows) * K * (x.element_size() + 1), f"mx_quant_kernel | rows={rows} K={K}" if _timing() else ""):
        _launch("m324_mx_quant", px, code_of(x.dtype), ldx, rows, K, pq, lq, ps, ls)
    _wrote(out.q, out.s)
    return out


def layernorm_mx(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float, out: Optional[MX] = None) -> MX:
    """LayerNorm of the fp32 stream x [rows, C] straight into an MX operand (m324_layernorm_mx)."""
    if x.dtype != torch.float32:
        raise L.M324Error("layernorm_mx: x must be fp32")
    rows, Cdim = x.shape
    out = mx_empty(rows, Cdim, x.device) if out is None else out
    px, ldx = _rows(x, "x")
    pq, lq, ps, ls = _mx_rows(out, rows, Cdim, "out")
    with span("hbm_pass", 0.0, float(rows) * Cdim * 5, f"layernorm_mx_kernel | rows={rows} C={Cdim}" if _timing() else ""):
        _launch("m324_layernorm_mx", px, ldx, _vec(w, Cdim, "w"), _vec(b, Cdim, "b"), eps, rows, Cdim, pq, lq, ps, ls)
    _wrote(out.q, out.s)
    return out


def gemm_mx(a: MX, w: MX, out, *, bias=None, act: int = L.ACT_NONE, gamma=None, residual: Optional[torch.Tensor] = None,
            qkv_heads: Optional[tuple] = None):
    """out = epilogue(a @ w^T) on MX operands (m324_gemm_mx).  Epilogues: `out` bf16 [M, N] (+ bias); qkv_heads, a QKVHeads
    (`out` None); `out` the fp32 residual stream with residual=out (+ bias, * gamma); `out` an MX operand [M, N] (+ bias, GELU
    with act=ACT_GELU).  Any other combination raises M324Error: none of bias / act / gamma / residual is ever dropped.
    Returns `out` (the first head-major output for qkv_heads)."""
    M, K = a.q.shape[0], a.q.shape[1]
    N = w.q.shape[0]
    pa, la, psa, lsa = _mx_rows(a, M, K, "a")
    pw, lw, psw, lsw = _mx_rows(w, N, K, "w")
    args = L.GemmArgs()
    args.A, args.lda, args.W, args.ldw = pa, la, pw, lw
    args.M, args.N, args.K = M, N, K
    args.in_dtype, args.batch = MXFP8, 1
    args.bias = _vec(bias, N, "bias")
    args.act = act
    args.gamma = _vec(gamma, N, "gamma")
    pcs, lcs = None, 0
    first = out
    # the branches below read residual only for a plain tensor `out`: refuse it elsewhere instead of dropping it (act / gamma
    # with the q|k|v heads, and every other combination that is not built, are refused by m324_gemm_mx itself)
    if residual is not None and (qkv_heads is not None or isinstance(out, MX)):
        raise L.M324Error("gemm_mx: residual= goes with the fp32 residual stream only (residual=out), not with "
                          + ("qkv_heads=" if qkv_heads is not None else "an MX output"))
    if qkv_heads is not None:
        first = _qkv_heads_args(args, qkv_heads, M, N, "gemm_mx")
    elif isinstance(out, MX):
        args.C, args.ldc, pcs, lcs = _mx_rows(out, M, N, "out")
        args.out_dtype = MXFP8
        _wrote(out.q, out.s)
    else:
        args.C, args.ldc = _rows(out, "out")
        args.out_dtype = code_of(out.dtype)
        if out.shape[0] < M or out.shape[1] < N:
            raise L.M324Error(f"gemm_mx: out{tuple(out.shape)} too small for {M} x {N}")
        if residual is not None:
            args.residual, args.ldr = _rows(residual, "residual")
        _wrote(out)
    with span("gemm_mx", 2.0 * M * N * K, float(M * K + N * K + M * N * 2),
              f"gemm_mx_kernel | M={M} N={N} K={K}" if _timing() else ""):
        _launch("m324_gemm_mx", C.byref(args), psa, lsa, psw, lsw, pcs, lcs)
    return first


def gemm_pair(deferred: list) -> None:
    """Launch the two projections prepared with gemm(..., qkv_heads=..., defer=deferred) as one kernel (m324_gemm_pair: horizontal
    fusion of two small latency-bound GEMMs); pairs the library does not build run as two m324_gemm launches."""
    if len(deferred) != 2:
        raise L.M324Error("gemm_pair: exactly two deferred projections")
    (a0, f0, b0, t0, _), (a1, f1, b1, t1, _) = deferred
    with span("gemm_bf16", f0 + f1, b0 + b1, f"gemm_ring2_pair_kernel<unsigned short, 4, 0> | {t0} + {t1}" if _timing() else "") as sp:
        rc = L.load().m324_gemm_pair(C.byref(a0), C.byref(a1), _stream())      # not _launch: "unsupported" is an answer here
        if rc == L.ERR_UNSUPPORTED:
            sp.cancel()                          # nothing ran: the two fallback launches below carry the work
    if rc == L.ERR_UNSUPPORTED:
        for args, fl, by, tag, _ in deferred:
            with span("gemm_bf16", fl, by, f"{_gemm_plan(args)} | {tag}" if _timing() else ""):
                _launch("m324_gemm", C.byref(args))
    else:
        L.check(rc, "m324_gemm_pair")
    deferred.clear()


def layernorm_pair(x0, w0, b0, eps0, out0, x1, w1, b1, eps1, out1, row_map1=(0, 0, 0)) -> None:
    """Two fp32 -> out-dtype LayerNorms of the same width in one launch (m324_layernorm_pair); the second may gather its rows
    (row_map1 as in layernorm)."""
    Cdim = x0.shape[1]
    if (x0.dtype != torch.float32 or x1.dtype != torch.float32 or x1.shape[1] != Cdim or out0.shape[1] != Cdim or out1.shape[1] != Cdim
            or out0.dtype != out1.dtype or out0.shape[0] > x0.shape[0]):
        raise L.M324Error("layernorm_pair: two fp32 inputs of one width, outputs of one dtype")
    gin, gout, off = row_map1
    rows1 = out1.shape[0]
    need = _row_extent(rows1, gin, gout, off) if gin > 0 else rows1
    if x1.shape[0] < need:
        raise L.M324Error("layernorm_pair: shape mismatch")
    (p0, l0), (q0, m0), (p1, l1), (q1, m1) = _rows(x0, "x0"), _rows(out0, "out0"), _rows(x1, "x1"), _rows(out1, "out1")
    tag = f"layernorm_pair_kernel | rows={out0.shape[0]}+{rows1} C={Cdim}" if _timing() else ""
    with span("hbm_pass", 0.0, float(out0.shape[0] + rows1) * Cdim * (4 + out0.element_size()), tag):
        _launch("m324_layernorm_pair", p0, l0, _vec(w0, Cdim, "w0"), _vec(b0, Cdim, "b0"), eps0, q0, m0, out0.shape[0], 0, 0, 0,
                p1, l1, _vec(w1, Cdim, "w1"), _vec(b1, Cdim, "b1"), eps1, q1, m1, rows1, gin, gout, off, Cdim, code_of(out0.dtype))
    _wrote(out0, out1)


def rowstats_finish(part: torch.Tensor, eps: float, rowstat: torch.Tensor) -> torch.Tensor:
    """rowstat[m] = (rstd, -rstd mean) from the per-block (sum, M2) pairs part[ncb, M, 2] a producer GEMM left."""
    ncb, M, two = part.shape
    if (two != 2 or part.dtype != torch.float32 or not part.is_contiguous() or rowstat.dtype != torch.float32
            or not rowstat.is_contiguous() or rowstat.numel() != 2 * M):
        raise L.M324Error("rowstats_finish: part [ncb, M, 2] and rowstat [M, 2] must be contiguous fp32")
    with span("hbm_pass", 0.0, 8.0 * (ncb + 1) * M, f"rowstats_finish_kernel | rows={M} blocks={ncb}" if _timing() else ""):
        _launch("m324_rowstats_finish", _p(part), ncb, M, eps, _p(rowstat))
    return rowstat


def rowstats(x: torch.Tensor, eps: float, rowstat: torch.Tensor, copy: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same table straight from an fp32 stream x [rows, C], plus its bf16 twin `copy` (head of a folded chain)."""
    px, ldx = _rows(x, "x")
    rows, Cdim = x.shape
    if x.dtype != torch.float32 or rowstat.dtype != torch.float32 or not rowstat.is_contiguous() or rowstat.numel() != 2 * rows:
        raise L.M324Error("rowstats: x fp32 [rows, C], rowstat contiguous fp32 [rows, 2]")
    pc, ldc = (None, 0)
    if copy is not None:
        if copy.dtype != torch.bfloat16 or copy.shape[0] < rows or copy.shape[1] != Cdim:
            raise L.M324Error("rowstats: copy must be bf16 [rows, C]")
        pc, ldc = _rows(copy, "copy")
    with span("hbm_pass", 0.0, rows * Cdim * (4.0 + (2.0 if copy is not None else 0.0)), f"rowstats_kernel | rows={rows} C={Cdim}" if _timing() else ""):
        _launch("m324_rowstats", px, ldx, rows, Cdim, eps, _p(rowstat), pc, ldc)
    return rowstat


def layernorm(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float, out: torch.Tensor,
              rows: Optional[int] = None, row_map=(0, 0, 0)) -> torch.Tensor:
    if x.dtype != torch.float32 and not (x.dtype == torch.bfloat16 and out.dtype == torch.bfloat16):
        raise L.M324Error("layernorm: x must be fp32 (or bf16 with a bf16 output)")
    px, ldx = _rows(x, "x")
    py, ldy = _rows(out, "out")
    Cdim = x.shape[1]
    rows = out.shape[0] if rows is None else rows
    gin, gout, off = row_map
    need = _row_extent(rows, gin, gout, off) if gin > 0 else rows
    if x.shape[0] < need or out.shape[0] < rows or out.shape[1] != Cdim:
        raise L.M324Error("layernorm: shape mismatch")
    tag = (f"layernorm_kernel<{'unsigned short' if out.element_size() == 2 else 'float'}, {'unsigned short' if x.element_size() == 2 else 'float'}>"
           f" | rows={rows} C={Cdim}") if _timing() else ""
    # a bf16 input goes through m324_layernorm_in, which takes the input dtype after the input pointer
    name, in_dtype = ("m324_layernorm_in", (BF16,)) if x.dtype == torch.bfloat16 else ("m324_layernorm", ())
    with span("hbm_pass", 0.0, float(rows) * Cdim * (x.element_size() + out.element_size()), tag):
        _launch(name, px, *in_dtype, ldx, _vec(w, Cdim, "w"), _vec(b, Cdim, "b"), eps, py, ldy, code_of(out.dtype), rows, Cdim, gin, gout, off)
    return out


LOG2E = 1.4426950408889634
Q_PRESCALE = (64 ** -0.5) * LOG2E      # softmax scale of head_dim 64, log2 domain


def qkv_split(q_src, k_src, v_src, q_w, k_w, eps: float, B: int, Lq: int, H: int, dtype: torch.dtype, *,
              q_scale: float = 1.0, train: bool = False):
    """Head-major attention operands from token-major sources (any source may be None).

    Inference (train=False): returns (Q[B,H,L,64], K[B,H,L,64], Vt[B,H,64,Lp]).
    Training  (train=True):  returns a dict with Q, K, V (row-major) and Qt, Kt, Vt (transposed, permuted) for every
    given source -- what m324_attention_bwd needs.  All given sources share B and L."""
    dev = next(t for t in (q_src, k_src, v_src) if t is not None).device
    Lp = (Lq + 63) // 64 * 64

    def row():
        return torch.empty((B, H, Lq, 64), dtype=dtype, device=dev)

    def tr():
        return torch.empty((B, H, 64, Lp), dtype=dtype, device=dev)
    Q = row() if q_src is not None else None
    K = row() if k_src is not None else None
    V = row() if (v_src is not None and train) else None
    Qt = tr() if (q_src is not None and train) else None
    Kt = tr() if (k_src is not None and train) else None
    Vt = tr() if v_src is not None else None

    def src(t, name):
        if t is None:
            return None, 0
        if t.dtype != dtype or t.shape[0] < B * Lq:
            raise L.M324Error(f"qkv_split: {name} {t.dtype}{tuple(t.shape)}")
        return _rows(t, name)
    pq, ldq = src(q_src, "q_src")
    pk, ldk = src(k_src, "k_src")
    pv, ldv = src(v_src, "v_src")
    _launch("m324_qkv_split", pq, ldq, pk, ldk, pv, ldv, _vec(q_w, 64, "q_w"), _vec(k_w, 64, "k_w"), eps, q_scale,
            _p(Q), _p(K), _p(V), _p(Qt), _p(Kt), _p(Vt), B, Lq, H, code_of(dtype))
    if train:
        return {"Q": Q, "K": K, "V": V, "Qt": Qt, "Kt": Kt, "Vt": Vt}
    return Q, K, Vt


def attention(Q: torch.Tensor, K: torch.Tensor, Vt: torch.Tensor, out: torch.Tensor, *, shared_q: bool = False,
              scale: Optional[float] = None, prescaled: bool = False, lse: Optional[torch.Tensor] = None,
              v_rowmajor: bool = False, bounded: bool = False, q_rows: Optional[int] = None) -> torch.Tensor:
    """out[B*Lq, H*64] = softmax(Q K^T scale) V.  Q[Bq,H,Lq,64] (Bq == 1 with shared_q), K[B,H,Lk,64],
    Vt[B,H,64,Lkp] -- or, with v_rowmajor (bf16 only), V[B,H,Lk,64].  prescaled: Q carries Q_PRESCALE.
    bounded: the caller vouches for |log2-domain score| <= 64 (M324_ATTN_SCORES_BOUNDED; see qk_score_bound).
    q_rows (m324_attention_rows): only the first q_rows queries of every (batch, head) are computed; the other rows of `out` are
    not written.  A multiple of 32, and the written rows are the full call's bit for bit."""
    B, H, Lk, D = K.shape
    Lq = Q.shape[2]
    vshape = (B, H, Lk, 64) if v_rowmajor else (B, H, 64, (Lk + 63) // 64 * 64)
    if D != 64 or Q.shape[3] != 64 or Q.shape[1] != H or tuple(Vt.shape) != vshape:
        raise L.M324Error(f"attention: Q{tuple(Q.shape)} K{tuple(K.shape)} V{tuple(Vt.shape)} (want {vshape})")
    if not (Q.is_contiguous() and K.is_contiguous() and Vt.is_contiguous()):
        raise L.M324Error("attention: operands must be contiguous")
    if Q.dtype != K.dtype or K.dtype != Vt.dtype or out.dtype != Q.dtype:
        raise L.M324Error("attention: dtype mismatch")
    if not shared_q and Q.shape[0] != B:
        raise L.M324Error("attention: batch mismatch")
    po, ldo = _rows(out, "out")
    if out.shape[0] < B * Lq or out.shape[1] < H * 64:
        raise L.M324Error("attention: out too small")
    qbs = 0 if shared_q else H * Lq * 64
    scale = 64 ** -0.5 if scale is None else scale
    esz = Q.element_size()
    flags = int(prescaled) | (2 if v_rowmajor else 0) | (4 if bounded else 0)       # M324_ATTN_*; the plan query takes shared_q as bit 8
    # q_rows: the other entry point, one more argument, fewer computed queries in the span, a word more in its tag
    name, nq, rows_arg, rows_tag = ("m324_attention", Lq, (), "") if q_rows is None else \
        ("m324_attention_rows", min(int(q_rows), Lq), (int(q_rows),), f" q_rows={q_rows}")
    with span(f"attention_{'bf16' if esz == 2 else 'f32'}", 4.0 * B * H * nq * Lk * 64,
              esz * 64.0 * H * ((1 if shared_q else B) * nq + 2 * B * Lk + B * nq),
              f"{_attn_plan(B, H, Lq, Lk, flags | (256 if shared_q else 0), code_of(Q.dtype))} | B={B} H={H} Lq={Lq} Lk={Lk}{rows_tag}"
              if _timing() else ""):
        _launch(name, _p(Q), qbs, _p(K), _p(Vt), po, ldo, B, H, Lq, Lk, scale, flags, _p(lse), code_of(Q.dtype), *rows_arg)
    return out


def attention_merge(parts, out: torch.Tensor, B: int, H: int, Lq: int) -> torch.Tensor:
    """out[B*Lq, H*64] = the attention over the union of two or three disjoint key sets from the (O_i, lse_i) pairs attention(...,
    lse=...) left for each of them (m324_attention_merge: log2-domain weights 2^(lse_i - max))."""
    if not 2 <= len(parts) <= 3:
        raise L.M324Error("attention_merge: two or three (output, lse) parts")
    O0 = parts[0][0]
    p0, ldp = _rows(O0, "O0")
    ptrs = []
    for O, lse in parts:
        po, ld = _rows(O, "part")
        if (O.dtype != out.dtype or ld != ldp or O.shape[0] < B * Lq or O.shape[1] < H * 64 or lse.dtype != torch.float32
                or not lse.is_contiguous() or lse.numel() != B * H * Lq):
            raise L.M324Error(f"attention_merge: part {O.dtype}{tuple(O.shape)} / lse {lse.dtype}{tuple(lse.shape)}")
        ptrs += [po, _p(lse)]
    if len(parts) == 2:
        ptrs += [None, None]
    po, ldo = _rows(out, "out")
    if out.shape[0] < B * Lq or out.shape[1] < H * 64:
        raise L.M324Error("attention_merge: out too small")
    esz = out.element_size()
    with span("hbm_pass", 0.0, float(B * Lq) * H * 64 * esz * (len(parts) + 1),
              f"attention_merge_kernel | rows={B * Lq} parts={len(parts)}" if _timing() else ""):
        _launch("m324_attention_merge", *ptrs, ldp, po, ldo, B, H, Lq, code_of(out.dtype))
    _wrote(out)
    return out


def patchify(video: torch.Tensor, size: int, patch: int, Kp: int, dtype: torch.dtype) -> torch.Tensor:
    """video [F,Hin,Win,3] fp32 in [0,1] -- or uint8 in 0..255, converted per tap as v / 255 (m324_patchify_u8: the rows equal the
    fp32 path's on `video.float() / 255` bit for bit) -> [F*(size/patch)^2, Kp] normalised, bilinearly resized patch rows."""
    if video.dtype not in (torch.float32, torch.uint8) or not video.is_contiguous() or video.dim() != 4 or video.shape[3] != 3:
        raise L.M324Error(f"patchify: video {video.dtype}{tuple(video.shape)}")
    Fr, Hin, Win, _ = video.shape
    g = size // patch
    out = torch.empty((Fr * g * g, Kp), dtype=dtype, device=video.device)
    _launch("m324_patchify_u8" if video.dtype == torch.uint8 else "m324_patchify", _p(video), Fr, Hin, Win, size, patch, _p(out), Kp, code_of(dtype))
    _wrote(out)
    return out


def point_encode(xyz: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    xyz = xyz.reshape(-1, 3)
    if xyz.dtype != torch.float32 or not xyz.is_contiguous():
        raise L.M324Error("point_encode: xyz must be contiguous fp32")
    out = torch.empty((xyz.shape[0], 64), dtype=dtype, device=xyz.device)
    _launch("m324_point_encode", _p(xyz), xyz.shape[0], _p(out), 64, code_of(dtype))
    return out


def point_concat(normal: torch.Tensor, rgb: torch.Tensor, feat: torch.Tensor, Cdim: int) -> torch.Tensor:
    normal, rgb = normal.reshape(-1, 3), rgb.reshape(-1, 3)
    for t in (normal, rgb):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise L.M324Error("point_concat: normal/rgb must be contiguous fp32")
    P, Kp = feat.shape
    if not feat.is_contiguous() or normal.shape[0] != P or rgb.shape[0] != P:
        raise L.M324Error("point_concat: shape mismatch")
    _launch("m324_point_concat", _p(normal), _p(rgb), P, _p(feat), Cdim, Kp, code_of(feat.dtype))
    return feat


def dino_cls_rows(cls: torch.Tensor, pos0: torch.Tensor, x: torch.Tensor, Fr: int, rows_per_frame: int) -> None:
    Cdim = x.shape[1]
    _launch("m324_dino_cls_rows", _vec(cls, Cdim, "cls"), _vec(pos0, Cdim, "pos0"), _p(x), Fr, rows_per_frame, Cdim)


def assemble_tokens(dino_x, dino_w, dino_b, eps_dino, pos, sp0, spr, mesh, ln_w, eps_in, B, T, K, P,
                    drop_p: float = 0.0, drop_seed: int = 0) -> torch.Tensor:
    Cdim = dino_x.shape[1]
    for name, t, n in (("dino_x", dino_x, B * T * (P + 1) * Cdim), ("pos", pos, T * P * Cdim), ("sp0", sp0, 4 * Cdim),
                       ("spr", spr, 4 * Cdim), ("mesh", mesh, B * K * Cdim)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise L.M324Error(f"assemble_tokens: {name} {t.dtype}{tuple(t.shape)} (want {n} fp32)")
    out = torch.empty((B * T * (4 + K + P), Cdim), dtype=torch.float32, device=dino_x.device)
    _launch("m324_assemble_tokens", _p(dino_x), _vec(dino_w, Cdim, "dino_w"), _vec(dino_b, Cdim, "dino_b"), eps_dino, _p(pos), _p(sp0),
            _p(spr), _p(mesh), _vec(ln_w, Cdim, "ln_w"), eps_in, _p(out), B, T, K, P, Cdim, float(drop_p), int(drop_seed) & 0xFFFFFFFFFFFFFFFF)
    return out


def linear_n3(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    M, K = a.shape
    pa, lda = _rows(a, "a")
    if w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape) != (3, K):
        raise L.M324Error("linear_n3: w must be contiguous fp32 [3,K]")
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != M * 3:
        raise L.M324Error("linear_n3: out must be contiguous fp32 [M,3]")
    _launch("m324_linear_n3", pa, lda, _p(w), _vec(bias, 3, "bias"), _p(out), M, K, code_of(a.dtype))
    return out


def n3_finish(part: torch.Tensor, bias: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[M, 3] (fp32, contiguous) = bias + sum over the column blocks of part[ncb, M, 3] (second half of gemm(..., n3=...))."""
    ncb, M, three = part.shape
    if three != 3 or part.dtype != torch.float32 or not part.is_contiguous() or out.dtype != torch.float32 \
            or not out.is_contiguous() or out.numel() != M * 3:
        raise L.M324Error("n3_finish: part [ncb, M, 3] and out [M, 3] must be contiguous fp32")
    _launch("m324_n3_finish", _p(part), ncb, M, _vec(bias, 3, "bias"), _p(out))
    return out


def mse(pred: torch.Tensor, target: torch.Tensor, weight: float) -> torch.Tensor:
    if pred.shape != target.shape:
        raise L.M324Error(f"mse: shape mismatch {tuple(pred.shape)} vs {tuple(target.shape)}")
    pred = pred.contiguous().float()
    target = target.contiguous().float()
    partial = torch.empty(1024, dtype=torch.float32, device=pred.device)
    out = torch.empty((), dtype=torch.float32, device=pred.device)
    _launch("m324_mse", _p(pred), _p(target), pred.numel(), weight, _p(partial), _p(out))
    return out


def smooth_trajectories(trajs: torch.Tensor, threshold: float, sigma: float) -> torch.Tensor:
    """[B,T,N,3] fp32 -> thresholded (threshold >= 0) and/or gaussian-filtered (sigma > 0) trajectories."""
    if trajs.dim() != 4 or trajs.shape[3] != 3:
        raise L.M324Error(f"smooth_trajectories: expected [B,T,N,3], got {tuple(trajs.shape)}")
    x = trajs.detach().to(torch.float32).contiguous()
    B, T, N, _ = x.shape
    tmp, out = torch.empty_like(x), torch.empty_like(x)
    _launch("m324_smooth_trajectories", _p(x), _p(tmp), _p(out), B, T, N, threshold, sigma)
    return out


def smooth_savgol(trajs: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """[B,T,N,3] fp32 filtered along T with the odd-length fp64 coefficient vector `coef` (clamped borders)."""
    x = trajs.detach().to(torch.float32).contiguous()
    B, T, N, _ = x.shape
    if coef.dtype != torch.float64 or not coef.is_cuda or not coef.is_contiguous():
        raise L.M324Error("smooth_savgol: coef must be a contiguous fp64 HIP tensor")
    out = torch.empty_like(x)
    _launch("m324_smooth_savgol", _p(x), _p(out), B, T, N, _p(coef), coef.numel())
    return out


def smooth_oneeuro(trajs: torch.Tensor, mincutoff: float, beta: float, dcutoff: float = 1.0) -> torch.Tensor:
    x = trajs.detach().to(torch.float32).contiguous()
    B, T, N, _ = x.shape
    out = torch.empty_like(x)
    _launch("m324_smooth_oneeuro", _p(x), _p(out), B, T, N, mincutoff, beta, dcutoff)
    return out


def nearest_point(query: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """query [Nq,3], ref [Nr,3] fp32 -> int64 [Nq] index of the nearest reference point."""
    q = query.detach().to(torch.float32).contiguous()
    r = ref.detach().to(torch.float32).contiguous()
    if q.dim() != 2 or q.shape[1] != 3 or r.dim() != 2 or r.shape[1] != 3:
        raise L.M324Error(f"nearest_point: expected [n,3] point sets, got {tuple(q.shape)} / {tuple(r.shape)}")
    idx = torch.empty((q.shape[0],), dtype=torch.int32, device=q.device)
    _launch("m324_nearest_point", _p(q), q.shape[0], _p(r), r.shape[0], _p(idx))
    return idx.long()


# ------------------------------------------------------------------------------------------------ geometry evaluation
def _points(t: torch.Tensor, name: str) -> torch.Tensor:
    """[n,3] or [B,n,3] point set -> contiguous fp32 device tensor (CPU tensors are refused: there is no host path here)"""
    _on_device(t, name)
    if t.dim() not in (2, 3) or t.shape[-1] != 3 or t.shape[-2] == 0 or t.shape[0] == 0:
        raise L.M324Error(f"{name}: expected a non-empty [n,3] or [B,n,3] point set, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def nn_plan(n_query: int, n_ref: int, batch: int = 1, ref_slices: int = 0):
    """(reference slices, scratch bytes) of the launch m324_nn_search makes for these sizes: m324_nn_plan, host-only"""
    return _plan_query("m324_nn_plan", n_query, n_ref, batch, ref_slices)


def nn_search(query: torch.Tensor, ref: torch.Tensor, want_dist: bool = True, want_index: bool = False, ref_slices: int = 0):
    """Nearest reference point of every query point, brute force in fp32 (m324_nn_search).  query / ref: [n,3] or [B,n,3];
    a 2-D operand beside a 3-D one is shared by every batch item.  Returns the Euclidean distance (fp32), the index (int32,
    -1 where nothing compares below +inf), or the pair (dist, index) -- shaped [n_query] or [B, n_query]."""
    q, r = _points(query, "nn_search: query"), _points(ref, "nn_search: ref")
    if not (want_dist or want_index):
        raise L.M324Error("nn_search: neither distances nor indices requested")
    batched = q.dim() == 3 or r.dim() == 3
    B = q.shape[0] if q.dim() == 3 else (r.shape[0] if r.dim() == 3 else 1)
    if q.dim() == 3 and r.dim() == 3 and q.shape[0] != r.shape[0]:
        raise L.M324Error(f"nn_search: batch sizes differ, {tuple(q.shape)} / {tuple(r.shape)}")
    if q.device != r.device:
        raise L.M324Error("nn_search: query and ref live on different devices")
    nq, nr = q.shape[-2], r.shape[-2]
    stride_q = nq * 3 if q.dim() == 3 else 0
    stride_r = nr * 3 if r.dim() == 3 else 0
    slices, need = nn_plan(nq, nr, B, ref_slices)
    scratch = torch.empty((need,), dtype=torch.uint8, device=q.device) if slices > 1 else None
    shape = (B, nq) if batched else (nq,)
    dist = torch.empty(shape, dtype=torch.float32, device=q.device) if want_dist else None
    index = torch.empty(shape, dtype=torch.int32, device=q.device) if want_index else None
    _launch("m324_nn_search", _p(q), stride_q, nq, _p(r), stride_r, nr, B, _p(dist), _p(index), ref_slices, _p(scratch), need if slices > 1 else 0)
    _wrote(dist, index)
    if want_dist and want_index:
        return dist, index
    return dist if want_dist else index


def dist_stats(dist: torch.Tensor, threshold: float):
    """dist [n] or [B,n] fp32 -> (fp64 sum, int64 count of entries < threshold) per row, deterministic (m324_dist_stats)."""
    _on_device(dist, "dist_stats")
    if dist.dim() not in (1, 2) or dist.numel() == 0 or dist.dtype != torch.float32:
        raise L.M324Error(f"dist_stats: expected a non-empty fp32 [n] or [B,n] tensor, got {dist.dtype}{tuple(dist.shape)}")
    d = dist.detach().contiguous()
    B, n = (d.shape[0], d.shape[1]) if d.dim() == 2 else (1, d.shape[0])
    partial = torch.empty((B * 64,), dtype=torch.float64, device=d.device)
    total = torch.empty((B,), dtype=torch.float64, device=d.device)
    count = torch.empty((B,), dtype=torch.int64, device=d.device)
    _launch("m324_dist_stats", _p(d), n, B, float(threshold), _p(partial), _p(total), _p(count))
    _wrote(partial, total, count)
    return (total, count) if dist.dim() == 2 else (total[0], count[0])


def _transform_params(params: torch.Tensor, name: str) -> torch.Tensor:
    if not _is_device(params) or params.dtype != torch.float64 or params.numel() != 13 or not params.is_contiguous():
        raise L.M324Error(f"{name}: params must be a contiguous fp64 HIP tensor of 13 values (s, R row-major, t)")
    return params


def transform_points(x: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """s * (x @ R.T) + t for fp32 points [..., 3], evaluated in fp64 and rounded once (m324_transform_points); params =
    fp64 device tensor (s, R row-major, t)."""
    _on_device(x, "transform_points")
    if x.dim() < 2 or x.shape[-1] != 3 or x.numel() == 0:
        raise L.M324Error(f"transform_points: expected non-empty [..., 3] points, got {tuple(x.shape)}")
    xs = x.detach().to(torch.float32).contiguous()
    out = torch.empty_like(xs)
    _launch("m324_transform_points", _p(xs), xs.numel() // 3, _p(_transform_params(params, "transform_points")), _p(out))
    _wrote(out)
    return out


def icp_moments(source: torch.Tensor, params: torch.Tensor, target: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """The fp64 moment record (32 doubles, layout in include/m324.h) of one ICP iteration: source [n,3] fp32 transformed by
    params, matched to target[index] (m324_icp_moments)."""
    s, t = _points(source, "icp_moments: source"), _points(target, "icp_moments: target")
    if s.dim() != 2 or t.dim() != 2:
        raise L.M324Error(f"icp_moments: expected [n,3] point sets, got {tuple(s.shape)} / {tuple(t.shape)}")
    if not _is_device(index) or index.dtype != torch.int32 or not index.is_contiguous() or index.numel() != s.shape[0]:
        raise L.M324Error(f"icp_moments: index must be a contiguous int32 HIP tensor of {s.shape[0]} entries")
    partial = torch.empty((64 * 32,), dtype=torch.float64, device=s.device)
    record = torch.empty((32,), dtype=torch.float64, device=s.device)
    _launch("m324_icp_moments", _p(s), s.shape[0], _p(_transform_params(params, "icp_moments")), _p(t), t.shape[0], _p(index), _p(partial), _p(record))
    _wrote(partial, record)
    return record


# ------------------------------------------------------------------------------------------------ surface sampling
class SurfaceSamples(NamedTuple):
    points: torch.Tensor                        # fp32 [num,3] or [B,num,3]
    points64: Optional[torch.Tensor]            # the same points before rounding
    face_index: Optional[torch.Tensor]          # int32 [num] or [B,num]
    normals: Optional[torch.Tensor]             # fp32, like points
    colors: Optional[torch.Tensor]              # fp32, like points


def _device_array(t, dtype: torch.dtype, name: str) -> torch.Tensor:
    _on_device(t, name)
    if t.dtype != dtype:
        raise L.M324Error(f"{name}: expected {dtype}, got {t.dtype}")
    return t.detach().contiguous()


def _faces_in_range(f: torch.Tensor, n_vertices: int, name: str) -> None:
    """the host-side range check of a face list in front of kernels that do not check it: one device reduction and a sync"""
    lo, hi = (int(x) for x in torch.aminmax(f))
    if lo < 0 or hi >= n_vertices:
        raise L.M324Error(f"{name}: faces index vertices {lo}..{hi}, the mesh has {n_vertices}")


def _surface_mesh(vertices, faces, name: str, faces_checked: bool):
    """(vertices fp64 contiguous, faces int32 contiguous, batch, stride_v in elements, batched); the kernels do not check
    vertex indices, so the range of `faces` is checked here (one device reduction and a sync) unless the caller did it on the
    host already."""
    v = _device_array(vertices, torch.float64, f"{name}: vertices")
    f = _device_array(faces, torch.int32, f"{name}: faces")
    if v.dim() not in (2, 3) or v.shape[-1] != 3 or v.shape[-2] == 0 or v.shape[0] == 0:
        raise L.M324Error(f"{name}: expected non-empty [V,3] or [B,V,3] fp64 vertices, got {tuple(v.shape)}")
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise L.M324Error(f"{name}: expected non-empty [F,3] int32 faces, got {tuple(f.shape)}")
    if f.device != v.device:
        raise L.M324Error(f"{name}: vertices and faces live on different devices")
    if not faces_checked:
        _faces_in_range(f, v.shape[-2], name)
    batched = v.dim() == 3
    return v, f, (v.shape[0] if batched else 1), (v.shape[-2] * 3 if batched else 0), batched


def surface_plan(n_faces: int, batch: int = 1):
    """(face blocks of the scan, scratch bytes) of m324_surface_cdf for these sizes: m324_surface_plan, host-only"""
    return _plan_query("m324_surface_plan", n_faces, batch)


def surface_cdf(vertices: torch.Tensor, faces: torch.Tensor, faces_checked: bool = False) -> torch.Tensor:
    """Area-weighted CDF of the faces (m324_surface_cdf): vertices fp64 [V,3] or [B,V,3], faces int32 [F,3] shared by the batch
    -> fp64 [F] or [B,F].  The additions run in the fixed nested order of include/m324.h; on a mesh whose partial sums are
    exact the table equals np.cumsum of the areas."""
    v, f, B, stride_v, batched = _surface_mesh(vertices, faces, "surface_cdf", faces_checked)
    nf = f.shape[0]
    _, need = surface_plan(nf, B)
    scratch = torch.empty((need,), dtype=torch.uint8, device=v.device) if need else None
    cdf = torch.empty((B, nf) if batched else (nf,), dtype=torch.float64, device=v.device)
    _launch("m324_surface_cdf", _p(v), stride_v, v.shape[-2], _p(f), nf, B, _p(cdf), _p(scratch), need)
    _wrote(cdf, scratch)
    return cdf


def surface_sample(vertices: torch.Tensor, faces: torch.Tensor, cdf: torch.Tensor, seeds: torch.Tensor, num: int, *,
                   want_points64: bool = False, want_face: bool = True, want_normals: bool = False, want_colors: bool = False,
                   vertex_colors: Optional[torch.Tensor] = None, uv: Optional[torch.Tensor] = None,
                   texture: Optional[torch.Tensor] = None, faces_checked: bool = False) -> SurfaceSamples:
    """`num` surface samples per mesh (m324_surface_sample), the draws of preprocess.sample_surface for the same seeds.
    vertices / faces / cdf as in surface_cdf; seeds int64 [B,2] (or [2]): the bit patterns of the two uint64 stream seeds.
    Colours (want_colors) come from vertex_colors (uint8 [V,3|4]) when given, else from uv (fp64 [V,2]) + texture (uint8
    [H,W,3]), else they are 0.5."""
    v, f, B, stride_v, batched = _surface_mesh(vertices, faces, "surface_sample", faces_checked)
    nv, nf, num = v.shape[-2], f.shape[0], int(num)
    table = _device_array(cdf, torch.float64, "surface_sample: cdf")
    if tuple(table.shape) != ((B, nf) if batched else (nf,)):
        raise L.M324Error(f"surface_sample: cdf {tuple(table.shape)} does not match {B} mesh(es) of {nf} faces")
    sd = _device_array(seeds, torch.int64, "surface_sample: seeds")
    if sd.numel() != 2 * B or sd.shape[-1] != 2:
        raise L.M324Error(f"surface_sample: seeds must be int64 [{B},2], got {tuple(sd.shape)}")
    if num <= 0:
        raise L.M324Error(f"surface_sample: num must be positive, got {num}")
    vc = tex = tuv = None
    channels = tex_h = tex_w = 0
    if vertex_colors is not None:
        vc = _device_array(vertex_colors, torch.uint8, "surface_sample: vertex_colors")
        if vc.dim() != 2 or vc.shape[0] != nv or vc.shape[1] not in (3, 4):
            raise L.M324Error(f"surface_sample: vertex_colors must be uint8 [{nv},3|4], got {tuple(vc.shape)}")
        channels = vc.shape[1]
    elif uv is not None or texture is not None:
        if uv is None or texture is None:
            raise L.M324Error("surface_sample: a texture lookup needs both uv and texture")
        tuv = _device_array(uv, torch.float64, "surface_sample: uv")
        tex = _device_array(texture, torch.uint8, "surface_sample: texture")
        if tuple(tuv.shape) != (nv, 2) or tex.dim() != 3 or tex.shape[2] != 3 or tex.shape[0] == 0 or tex.shape[1] == 0:
            raise L.M324Error(f"surface_sample: expected uv fp64 [{nv},2] and texture uint8 [H,W,3], got {tuple(tuv.shape)} / {tuple(tex.shape)}")
        tex_h, tex_w = tex.shape[0], tex.shape[1]
    shape = (B, num) if batched else (num,)
    dev = v.device
    points = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
    points64 = torch.empty(shape + (3,), dtype=torch.float64, device=dev) if want_points64 else None
    face_index = torch.empty(shape, dtype=torch.int32, device=dev) if want_face else None
    normals = torch.empty(shape + (3,), dtype=torch.float32, device=dev) if want_normals else None
    colors = torch.empty(shape + (3,), dtype=torch.float32, device=dev) if want_colors else None
    _launch("m324_surface_sample", _p(v), stride_v, nv, _p(f), nf, _p(table), _p(sd), num, B, _p(points), _p(points64), _p(face_index),
            _p(normals), _p(colors), _p(vc), channels, _p(tuv), _p(tex), tex_h, tex_w)
    _wrote(points, points64, face_index, normals, colors)
    return SurfaceSamples(points, points64, face_index, normals, colors)


# ------------------------------------------------------------------------------------------------ tracked surface samples
class VertexCorners(NamedTuple):
    offsets: torch.Tensor                       # int32 [V+1]: start of every vertex's group in `corners`
    corners: torch.Tensor                       # int32 [3F]: corners 3 f + k grouped by vertex, ascending inside a vertex


class TrackedSamples(NamedTuple):
    points: torch.Tensor                        # fp32 [T,num,3] or [B,T,num,3]
    normals: Optional[torch.Tensor]             # fp32, like points
    colors: Optional[torch.Tensor]              # fp32 [num,3] or [B,num,3]: a sample keeps its colour through the clip
    face_index: Optional[torch.Tensor]          # int32 [num] or [B,num]
    points64: Optional[torch.Tensor] = None     # the same points before rounding


NORMAL_WEIGHTINGS = {"angle": 0, "area": 1}    # M324_NORMALS_ANGLE, M324_NORMALS_AREA
_CORNER_CACHE = {}                              # id(faces) -> (weakref to faces, its version, n_vertices, VertexCorners)


def vertex_corners(faces: torch.Tensor, n_vertices: int) -> VertexCorners:
    """The vertex-corner table of include/m324.h for faces int32 [F,3] on the device: a stable counting sort of the corners by
    vertex, done in numpy on the host (one download of the faces; their range is checked on the way) and cached on the identity
    and version of the faces tensor -- the table depends on the topology alone, so a mesh pays for it once."""
    import weakref
    import numpy as np
    f = _device_array(faces, torch.int32, "vertex_corners: faces")
    n_vertices = int(n_vertices)
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0 or n_vertices <= 0 or f.shape[0] > (2 ** 31 - 1) // 3:
        raise L.M324Error(f"vertex_corners: expected non-empty [F,3] int32 faces and a positive vertex count, got {tuple(f.shape)} / {n_vertices}")
    hit = _CORNER_CACHE.get(id(faces))
    if hit is not None and hit[0]() is faces and hit[1] == faces._version and hit[2] == n_vertices:
        return hit[3]
    flat = f.cpu().numpy().reshape(-1)
    if flat.min() < 0 or flat.max() >= n_vertices:
        raise L.M324Error(f"vertex_corners: faces index vertices {flat.min()}..{flat.max()}, the mesh has {n_vertices}")
    offsets = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=n_vertices), out=offsets[1:])
    corners = np.argsort(flat, kind="stable")                                   # ascending corner index inside a vertex
    table = VertexCorners(torch.from_numpy(offsets.astype(np.int32)).to(f.device), torch.from_numpy(corners.astype(np.int32)).to(f.device))
    key = id(faces)
    _CORNER_CACHE[key] = (weakref.ref(faces, lambda _, key=key: _CORNER_CACHE.pop(key, None)), faces._version, n_vertices, table)
    return table


def _corner_table(corners, faces: torch.Tensor, f: torch.Tensor, n_vertices: int, name: str) -> VertexCorners:
    """the caller's table, shape-checked against the mesh, or the cached one of the caller's faces tensor (f: its contiguous form)"""
    if corners is None:
        return vertex_corners(faces, n_vertices)
    if not isinstance(corners, tuple) or len(corners) != 2:
        raise L.M324Error(f"{name}: corners is what vertex_corners returns: (offsets int32 [V+1], corners int32 [3F])")
    off = _device_array(corners[0], torch.int32, f"{name}: corner offsets")
    lst = _device_array(corners[1], torch.int32, f"{name}: corner list")
    if tuple(off.shape) != (n_vertices + 1,) or tuple(lst.shape) != (3 * f.shape[0],) or off.device != f.device or lst.device != f.device:
        raise L.M324Error(f"{name}: the corner table {tuple(off.shape)} / {tuple(lst.shape)} does not fit {n_vertices} vertices and "
                          f"{f.shape[0]} faces")
    return VertexCorners(off, lst)


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor, corners: Optional[VertexCorners] = None, weighting: str = "angle",
                   faces_checked: bool = False) -> torch.Tensor:
    """Unit vertex normals of every pose of one topology (m324_vertex_normals): vertices fp64 [V,3] or [..., V, 3] (any leading
    axes: frames, batch x frames), faces int32 [F,3] -> fp64 like vertices.  weighting "angle" (trimesh's default) or "area";
    corners: vertex_corners(faces, V), built (and cached) here when omitted.  A vertex without faces, or whose sum is zero, gets 0."""
    if weighting not in NORMAL_WEIGHTINGS:
        raise L.M324Error(f"vertex_normals: weighting must be one of {sorted(NORMAL_WEIGHTINGS)}, got {weighting!r}")
    v = _device_array(vertices, torch.float64, "vertex_normals: vertices")
    if v.dim() < 2 or v.shape[-1] != 3 or v.numel() == 0:
        raise L.M324Error(f"vertex_normals: expected non-empty fp64 vertices [..., V, 3], got {tuple(v.shape)}")
    nv = v.shape[-2]
    _, f, _, _, _ = _surface_mesh(v.reshape(-1, nv, 3)[0], faces, "vertex_normals", faces_checked)
    table = _corner_table(corners, faces, f, nv, "vertex_normals")
    frames = v.numel() // (nv * 3)
    out = torch.empty_like(v)
    _launch("m324_vertex_normals", _p(v), nv * 3, nv, _p(f), f.shape[0], _p(table.offsets), _p(table.corners), frames,
            NORMAL_WEIGHTINGS[weighting], _p(out))
    _wrote(out)
    return out


def surface_track(vertices: torch.Tensor, faces: torch.Tensor, cdf: torch.Tensor, seeds: torch.Tensor, num: int, *,
                  vertex_normals: Optional[torch.Tensor] = None, face_uvs: Optional[torch.Tensor] = None,
                  texture: Optional[torch.Tensor] = None, frames: Optional[int] = None, want_points64: bool = False,
                  want_face: bool = True, faces_checked: bool = False) -> TrackedSamples:
    """`num` surface samples drawn on frame 0 and carried through every frame (m324_surface_track): frame 0 repeats
    surface_sample for the same seeds.  vertices fp64 [T,V,3] (one clip) or [B,T,V,3]; faces int32 [F,3]; cdf = surface_cdf of
    frame 0, [F] or [B,F]; seeds int64 [2] or [B,2].  One clip with B > 1 seeds draws B sample sets on it (batch stride 0).
    vertex_normals (fp64, shaped like vertices) adds interpolated unit normals; face_uvs (fp64 [F,3,2]) with texture (uint8
    [H,W,3]) adds one colour per sample.  frames: track only the first `frames` frames of the clip (the outputs have that many);
    the clip is addressed in place by its strides, so frames=1 draws on frame 0 without a copy of it."""
    v = _device_array(vertices, torch.float64, "surface_track: vertices")
    if v.dim() not in (3, 4) or v.shape[-1] != 3 or v.numel() == 0:
        raise L.M324Error(f"surface_track: expected non-empty fp64 vertices [T,V,3] or [B,T,V,3], got {tuple(v.shape)}")
    T, nv = v.shape[-3], v.shape[-2]
    stride_t = nv * 3
    if frames is not None:
        if not 1 <= int(frames) <= T:
            raise L.M324Error(f"surface_track: frames must be in 1..{T} for vertices {tuple(v.shape)}, got {frames}")
        T = int(frames)
    _, f, _, _, _ = _surface_mesh(v.reshape(-1, nv, 3)[0], faces, "surface_track", faces_checked)
    nf, num = f.shape[0], int(num)
    sd = _device_array(seeds, torch.int64, "surface_track: seeds")
    if sd.dim() not in (1, 2) or sd.shape[-1] != 2 or sd.numel() == 0:
        raise L.M324Error(f"surface_track: seeds must be int64 [2] or [B,2], got {tuple(sd.shape)}")
    batched = v.dim() == 4 or sd.dim() == 2
    B = sd.numel() // 2
    if v.dim() == 4 and v.shape[0] != B:
        raise L.M324Error(f"surface_track: {B} seed pair(s) for vertices {tuple(v.shape)}")
    stride_b = v.shape[-3] * stride_t if v.dim() == 4 else 0
    table = _device_array(cdf, torch.float64, "surface_track: cdf")
    if tuple(table.shape) not in (((B, nf), (nf,)) if stride_b == 0 else ((B, nf),)):
        raise L.M324Error(f"surface_track: cdf {tuple(table.shape)} does not match {B} item(s) of {nf} faces on vertices {tuple(v.shape)}")
    if table.dim() == 1 and B > 1:
        table = table.expand(B, nf).contiguous()
    if num <= 0:
        raise L.M324Error(f"surface_track: num must be positive, got {num}")
    vn = None
    if vertex_normals is not None:
        vn = _device_array(vertex_normals, torch.float64, "surface_track: vertex_normals")
        if vn.shape != v.shape:
            raise L.M324Error(f"surface_track: vertex_normals {tuple(vn.shape)} must be shaped like vertices {tuple(v.shape)}")
    tuv = tex = None
    tex_h = tex_w = 0
    if face_uvs is not None or texture is not None:
        if face_uvs is None or texture is None:
            raise L.M324Error("surface_track: a colour lookup needs both face_uvs and texture")
        tuv = _device_array(face_uvs, torch.float64, "surface_track: face_uvs")
        tex = _device_array(texture, torch.uint8, "surface_track: texture")
        if tuple(tuv.shape) != (nf, 3, 2) or tex.dim() != 3 or tex.shape[2] != 3 or tex.shape[0] == 0 or tex.shape[1] == 0:
            raise L.M324Error(f"surface_track: expected face_uvs fp64 [{nf},3,2] and texture uint8 [H,W,3], got {tuple(tuv.shape)} / {tuple(tex.shape)}")
        tex_h, tex_w = tex.shape[0], tex.shape[1]
    if any(t is not None and t.device != v.device for t in (f, sd, table, vn, tuv, tex)):
        raise L.M324Error("surface_track: the inputs live on different devices")
    lead = (B,) if batched else ()
    dev = v.device
    points = torch.empty(lead + (T, num, 3), dtype=torch.float32, device=dev)
    points64 = torch.empty(lead + (T, num, 3), dtype=torch.float64, device=dev) if want_points64 else None
    face_index = torch.empty(lead + (num,), dtype=torch.int32, device=dev) if want_face else None
    normals = torch.empty(lead + (T, num, 3), dtype=torch.float32, device=dev) if vn is not None else None
    colors = torch.empty(lead + (num, 3), dtype=torch.float32, device=dev) if tex is not None else None
    _launch("m324_surface_track", _p(v), stride_b, stride_t, nv, _p(f), nf, _p(table), _p(sd), num, B, T, _p(points), _p(points64),
            _p(face_index), _p(vn), stride_b, stride_t, _p(normals), _p(tuv), _p(tex), tex_h, tex_w, _p(colors))
    _wrote(points, points64, face_index, normals, colors)
    return TrackedSamples(points, normals, colors, face_index, points64)


# ------------------------------------------------------------------------------------------------ video framing
FRAME_MODES = {"none": 0, "threshold": 1, "soft": 2, "binary": 3}          # M324_FRAME_* of include/m324.h
FRAME_AXES = {"x": 0, "y": 1}


def frame_plan(in_size: int, out_size: int, lines: int = 1, channels: int = 3, frames: int = 1):
    """(ksize, bytes of the pass's result) of one resampling pass: m324_frame_plan, host-only"""
    return _plan_query("m324_frame_plan", in_size, out_size, lines, channels, frames)


def _frame_image(t, channels, name: str):
    """uint8 device image stack [T,H,W,>=channels] (or [T,H,W] for one channel) with a unit channel stride -> (pointer, byte
    strides of frame / row / pixel, T, H, W); views with a padded pitch or a wider pixel are taken as they are"""
    _on_device(t, name)
    if t.dtype != torch.uint8:
        raise L.M324Error(f"{name}: expected uint8, got {t.dtype}")
    if t.dim() == 3 and channels == 1:
        t = t.unsqueeze(-1)
    if t.dim() != 4 or t.shape[3] < channels or 0 in t.shape or (t.shape[3] > 1 and t.stride(3) != 1) or min(t.stride()[:3]) < 0:
        raise L.M324Error(f"{name}: expected a non-empty [T,H,W,{channels}] uint8 image stack with a unit channel stride, got {tuple(t.shape)} {t.stride()}")
    return t.data_ptr(), t.stride(0), t.stride(1), t.stride(2), t.shape[0], t.shape[1], t.shape[2]


def _frame_table(table, mode: str, device, name: str):
    if mode != "soft":
        return None
    table = _device_array(table, torch.uint8, f"{name}: table") if table is not None else None
    if table is None or table.numel() != 65536 or table.device != device:
        raise L.M324Error(f"{name}: the soft mode needs a uint8 [256,256] table on the video's device")
    return table


def frame_mask(video: torch.Tensor, alpha: Optional[torch.Tensor] = None, *, mode: str = "threshold", threshold: int = 204,
               table: Optional[torch.Tensor] = None, want_masked: bool = True, want_mask: bool = True):
    """Masking and per-frame boxes (m324_frame_mask): video uint8 [T,H,W,4] (RGBA) or [T,H,W,3] with alpha [T,H,W] ->
    (masked [T,H,W,3] or None, mask [T,H,W] or None, boxes int32 [T,4] = (left, top, right, bottom), left >= right on a frame
    without foreground)."""
    if mode not in ("threshold", "soft"):
        raise L.M324Error(f"frame_mask: mode must be 'threshold' or 'soft', got {mode!r}")
    sp, sf, spitch, spix, T, H, W = _frame_image(video, 3, "frame_mask: video")
    ap = af = apitch = apix = 0
    if alpha is None:
        if video.shape[3] != 4:
            raise L.M324Error(f"frame_mask: without alpha the video is RGBA [T,H,W,4], got {tuple(video.shape)}")
        ap = None
    else:
        ap, af, apitch, apix, Ta, Ha, Wa = _frame_image(alpha, 1, "frame_mask: alpha")
        if (Ta, Ha, Wa) != (T, H, W) or alpha.device != video.device:
            raise L.M324Error(f"frame_mask: alpha {tuple(alpha.shape)} does not match video {tuple(video.shape)}")
    table = _frame_table(table, mode, video.device, "frame_mask")
    dev = video.device
    masked = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev) if want_masked else None
    mask = torch.empty((T, H, W), dtype=torch.uint8, device=dev) if want_mask else None
    boxes = torch.empty((T, 4), dtype=torch.int32, device=dev)
    _launch("m324_frame_mask", sp, sf, spitch, spix, ap, af, apitch, apix, T, H, W, FRAME_MODES[mode], int(threshold), _p(table),
            _p(masked), _p(mask), _p(boxes))
    _wrote(masked, mask, boxes)
    return masked, mask, boxes


def frame_resample(src: torch.Tensor, coef: torch.Tensor, bounds: torch.Tensor, axis: str, *, channels: int = 3, crop=None,
                   alpha: Optional[torch.Tensor] = None, mode: str = "none", threshold: int = 204, table: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, paste=(0, 0), fill: int = -1) -> torch.Tensor:
    """One separable resampling pass (m324_frame_resample) along `axis` ("x" or "y") over the crop (x, y, w, h) of src uint8
    [T,H,W,channels]; coef int32 [out_size, ksize], bounds int32 [out_size, 2] as framing.resample_tables builds them.  The
    result goes to a new dense tensor, or is pasted at `paste` = (x, y) into `out`; fill >= 0 writes all of `out`."""
    if axis not in FRAME_AXES or mode not in FRAME_MODES:
        raise L.M324Error(f"frame_resample: axis must be 'x' or 'y' and mode one of {sorted(FRAME_MODES)}, got {axis!r}, {mode!r}")
    sp, sf, spitch, spix, T, H, W = _frame_image(src, channels, "frame_resample: src")
    cx, cy, cw, ch = (0, 0, W, H) if crop is None else (int(v) for v in crop)
    coef = _device_array(coef, torch.int32, "frame_resample: coef")
    bounds = _device_array(bounds, torch.int32, "frame_resample: bounds")
    if coef.dim() != 2 or 0 in coef.shape or tuple(bounds.shape) != (coef.shape[0], 2):
        raise L.M324Error(f"frame_resample: expected coef [out,ksize] and bounds [out,2], got {tuple(coef.shape)} / {tuple(bounds.shape)}")
    out_size, ksize = coef.shape
    ap = af = apitch = apix = 0
    if mode == "none":
        ap = None
    else:
        if alpha is None:
            raise L.M324Error(f"frame_resample: mode {mode!r} needs alpha")
        ap, af, apitch, apix, Ta, Ha, Wa = _frame_image(alpha, 1, "frame_resample: alpha")
        if (Ta, Ha, Wa) != (T, H, W):
            raise L.M324Error(f"frame_resample: alpha {tuple(alpha.shape)} does not match src {tuple(src.shape)}")
    table = _frame_table(table, mode, src.device, "frame_resample")
    if out is None:
        shape = (T, ch, out_size) if axis == "x" else (T, out_size, cw)
        out = torch.empty(shape + (channels,), dtype=torch.uint8, device=src.device)
    dp, df, dpitch, dpix, Td, Hd, Wd = _frame_image(out, channels, "frame_resample: out")
    if Td != T or any(t.device != src.device for t in (coef, bounds, out) + (() if alpha is None else (alpha,))):
        raise L.M324Error("frame_resample: out has another frame count, or the tensors live on different devices")
    _launch("m324_frame_resample", sp, sf, spitch, spix, W, H, cx, cy, cw, ch, channels, T, FRAME_AXES[axis], _p(coef), _p(bounds), out_size,
            ksize, ap, af, apitch, apix, FRAME_MODES[mode], int(threshold), _p(table), dp, df, dpitch, dpix, Wd, Hd,
            int(paste[0]), int(paste[1]), int(fill))
    _wrote(out)
    return out


# ------------------------------------------------------------------------------------------------ mesh clip rendering
RENDER_BIG_PIXELS = 64          # default of big_pixels, measured against 16 / 256 / 1024 (profiles/mesh_render.md); never in the result


def render_plan(n_vertices: int, n_faces: int, frames: int, size: int) -> int:
    """scratch bytes of the three render entry points for these sizes: m324_render_plan, host-only"""
    return _plan_query("m324_render_plan", int(n_vertices), int(n_faces), int(frames), int(size))[1]


def _render_view(view, name: str):
    """the row-major 3 x 4 view matrix as 12 host floats"""
    import numpy as np
    m = np.ascontiguousarray(np.asarray(view, dtype=np.float32))
    if m.shape != (3, 4):
        raise L.M324Error(f"{name}: the view matrix is 3 x 4, got {m.shape}")
    return m


def _render_clip(vertices, name: str):
    """fp32 device clip [T,V,3] -> (tensor, stride_t in elements); a view whose last two axes are contiguous is used in place"""
    _on_device(vertices, name)
    if vertices.dtype != torch.float32:
        raise L.M324Error(f"{name}: expected torch.float32, got {vertices.dtype}")
    v = vertices.detach()
    if v.dim() != 3 or v.shape[2] != 3 or 0 in v.shape:
        raise L.M324Error(f"{name}: expected non-empty fp32 vertices [T,V,3], got {tuple(v.shape)}")
    if v.stride(2) != 1 or v.stride(1) != 3 or (v.shape[0] > 1 and v.stride(0) < 0):
        v = v.contiguous()
    return v, (v.stride(0) if v.shape[0] > 1 else v.shape[1] * 3)


def _render_faces(faces, n_vertices: int, device, name: str, faces_checked: bool) -> torch.Tensor:
    """int32 faces [F,3] on the clip's device; their range is checked here (one reduction and a sync), as _surface_mesh does,
    unless the caller did it already"""
    f = _device_array(faces, torch.int32, f"{name}: faces")
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise L.M324Error(f"{name}: expected non-empty [F,3] int32 faces, got {tuple(f.shape)}")
    if f.device != device:
        raise L.M324Error(f"{name}: vertices and faces live on different devices")
    if not faces_checked:
        _faces_in_range(f, n_vertices, name)
    return f


def _render_scratch(scratch, need: int, device, name: str) -> torch.Tensor:
    if scratch is None:
        return torch.empty((need,), dtype=torch.uint8, device=device)
    if not _is_device(scratch) or scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need or scratch.device != device:
        raise L.M324Error(f"{name}: scratch must be a contiguous uint8 device tensor of at least {need} bytes (render_plan)")
    return scratch


def render_project(vertices: torch.Tensor, view, size: int, n_faces: int, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Projects every vertex of a clip (m324_render_project): vertices fp32 [T,V,3] (a view with contiguous last two axes is used
    in place), view = the 3 x 4 matrix.  Returns the scratch buffer the raster and shade steps continue on."""
    v, stride_t = _render_clip(vertices, "render_project: vertices")
    m = _render_view(view, "render_project")
    T, nv = v.shape[0], v.shape[1]
    need = render_plan(nv, n_faces, T, size)
    scratch = _render_scratch(scratch, need, v.device, "render_project")
    _launch("m324_render_project", _p(v), stride_t, nv, int(n_faces), T, m.ctypes.data, int(size), _p(scratch), scratch.numel())
    _wrote(scratch)
    return scratch


def render_raster(faces: torch.Tensor, n_vertices: int, frames: int, size: int, scratch: torch.Tensor, big_pixels: Optional[int] = None,
                  faces_checked: bool = False) -> torch.Tensor:
    """Fills the (depth, face) keys of every frame (m324_render_raster) on the scratch render_project returned.  big_pixels:
    boxes larger than this go through the queued pass; None = RENDER_BIG_PIXELS.  The keys do not depend on it."""
    _on_device(scratch, "render_raster")
    f = _render_faces(faces, int(n_vertices), scratch.device, "render_raster", faces_checked)
    need = render_plan(n_vertices, f.shape[0], frames, size)
    scratch = _render_scratch(scratch, need, scratch.device, "render_raster")
    big = RENDER_BIG_PIXELS if big_pixels is None else int(big_pixels)
    if not 0 <= big <= 2 ** 31 - 1:
        raise L.M324Error(f"render_raster: big_pixels must be in 0..2^31-1, got {big_pixels}")
    _launch("m324_render_raster", _p(f), f.shape[0], int(n_vertices), int(frames), int(size), big, _p(scratch), scratch.numel())
    _wrote(scratch)
    return scratch


def render_shade(faces: torch.Tensor, n_vertices: int, frames: int, size: int, scratch: torch.Tensor, view, *,
                 colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, ambient: float = 0.3,
                 background=(0, 0, 0), out=None, faces_checked: bool = False):
    """Resolves the keys into (rgb uint8 [T,S,S,3], face int32 [T,S,S], depth int32 [T,S,S]) (m324_render_shade).  colors fp32
    [V,3]; normals fp32 [T,V,3] (model space) selects smooth shading, None flat; out: the three tensors to write, dense."""
    _on_device(scratch, "render_shade")
    dev = scratch.device
    T, S, nv = int(frames), int(size), int(n_vertices)
    f = _render_faces(faces, nv, dev, "render_shade", faces_checked)
    m = _render_view(view, "render_shade")
    need = render_plan(nv, f.shape[0], T, S)
    scratch = _render_scratch(scratch, need, dev, "render_shade")
    col = None
    if colors is not None:
        col = _device_array(colors, torch.float32, "render_shade: colors")
        if tuple(col.shape) != (nv, 3) or col.device != dev:
            raise L.M324Error(f"render_shade: colors must be fp32 [{nv},3] on the clip's device, got {tuple(col.shape)}")
    vn, normal_stride = None, 0
    if normals is not None:
        vn, normal_stride = _render_clip(normals, "render_shade: normals")
        if tuple(vn.shape) != (T, nv, 3) or vn.device != dev:
            raise L.M324Error(f"render_shade: normals must be fp32 [{T},{nv},3] on the clip's device, got {tuple(vn.shape)}")
    bg = [int(c) for c in background]
    if len(bg) != 3 or any(not 0 <= c <= 255 for c in bg) or not 0.0 <= float(ambient) <= 1.0:
        raise L.M324Error(f"render_shade: background is three bytes and ambient lies in [0, 1], got {background!r}, {ambient!r}")
    if out is None:
        out = (torch.empty((T, S, S, 3), dtype=torch.uint8, device=dev), torch.empty((T, S, S), dtype=torch.int32, device=dev),
               torch.empty((T, S, S), dtype=torch.int32, device=dev))
    rgb, face, depth = out
    for t, shape, dt, what in ((rgb, (T, S, S, 3), torch.uint8, "rgb"), (face, (T, S, S), torch.int32, "face"), (depth, (T, S, S), torch.int32, "depth")):
        if not _is_device(t) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise L.M324Error(f"render_shade: out {what} must be a contiguous {dt} device tensor {shape}")
    _launch("m324_render_shade", _p(f), f.shape[0], nv, T, S, _p(col), _p(vn), normal_stride, m.ctypes.data, float(ambient),
            bg[0] | bg[1] << 8 | bg[2] << 16, _p(rgb), _p(face), _p(depth), _p(scratch), scratch.numel())
    _wrote(rgb, face, depth)
    return rgb, face, depth


TEXTURE_MAX_SIDE = 16384        # M324_TEXTURE_MAX_SIDE
SUPERSAMPLES = (1, 2, 4)


def texture_plan(tex_h: int, tex_w: int):
    """(levels, bytes) of the mip chain of a tex_h x tex_w texture: m324_texture_plan, host-only"""
    levels, need = C.c_int(0), C.c_long(0)
    L.check(L.load().m324_texture_plan(int(tex_h), int(tex_w), C.addressof(levels), C.addressof(need)), "m324_texture_plan")
    return int(levels.value), int(need.value)


def texture_levels(tex_h: int, tex_w: int):
    """[(byte offset, H_l, W_l)] of every level, by the offset rule of include/m324.h; its length and end are the plan's"""
    count, need = texture_plan(tex_h, tex_w)
    out, at, h, w = [], 0, int(tex_h), int(tex_w)
    while True:
        out.append((at, h, w))
        at += (4 * w * h + 255) // 256 * 256
        if h == 1 and w == 1:
            break
        h, w = max(1, h >> 1), max(1, w >> 1)
    if len(out) != count or at != need:
        raise L.M324Error(f"texture_levels: {len(out)} levels / {at} bytes by the offset rule, m324_texture_plan says {count} / {need}")
    return out


def _texture(texture, name: str) -> torch.Tensor:
    _on_device(texture, name)
    if texture.dtype != torch.uint8 or texture.dim() != 3 or texture.shape[2] not in (3, 4) or 0 in texture.shape:
        raise L.M324Error(f"{name}: expected a uint8 texture [H,W,3] or [H,W,4], got {texture.dtype} {tuple(texture.shape)}")
    if max(texture.shape[0], texture.shape[1]) > TEXTURE_MAX_SIDE:
        raise L.M324Error(f"{name}: texture sides must be in 1..{TEXTURE_MAX_SIDE}, got {texture.shape[0]} x {texture.shape[1]}")
    return texture.detach().contiguous()


def texture_mips(texture: torch.Tensor):
    """The mip chain of a uint8 device texture [H,W,3|4] (m324_texture_mips; a fourth channel is ignored): (mips uint8 [bytes],
    levels = texture_levels(H, W)).  Level l is mips[off : off + 4 H_l W_l] viewed as [H_l, W_l, 4], texels (R, G, B, 0)."""
    tex = _texture(texture, "texture_mips")
    H, W, ch = tex.shape
    levels = texture_levels(H, W)
    need = texture_plan(H, W)[1]
    mips = torch.zeros((need,), dtype=torch.uint8, device=tex.device)
    _launch("m324_texture_mips", _p(tex), H, W, ch, _p(mips), need)
    _wrote(mips)
    return mips, levels


def render_shade_tex(faces: torch.Tensor, n_vertices: int, frames: int, size: int, scratch: torch.Tensor, view, *,
                     colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, ambient: float = 0.3,
                     background=(0, 0, 0), face_uvs: Optional[torch.Tensor] = None, mips: Optional[torch.Tensor] = None,
                     tex_size=None, use_mips: bool = True, supersample: int = 1, out=None, faces_checked: bool = False):
    """render_shade with an optional texture and supersampling (m324_render_shade_tex).  `size` is the sample resolution S' that
    render_project and render_raster ran at; rgb is uint8 [T,S'/ss,S'/ss,3], face and depth stay int32 [T,S',S'].  face_uvs
    fp32 [F,3,2] with mips and tex_size = (H, W) of texture_mips select the textured albedo; use_mips False samples level 0."""
    _on_device(scratch, "render_shade_tex")
    dev = scratch.device
    T, S, nv, ss = int(frames), int(size), int(n_vertices), int(supersample)
    if ss not in SUPERSAMPLES or S % ss:
        raise L.M324Error(f"render_shade_tex: supersample must be one of {SUPERSAMPLES} and divide size, got {supersample!r} at size {S}")
    f = _render_faces(faces, nv, dev, "render_shade_tex", faces_checked)
    m = _render_view(view, "render_shade_tex")
    need = render_plan(nv, f.shape[0], T, S)
    scratch = _render_scratch(scratch, need, dev, "render_shade_tex")
    col = None
    if colors is not None:
        col = _device_array(colors, torch.float32, "render_shade_tex: colors")
        if tuple(col.shape) != (nv, 3) or col.device != dev:
            raise L.M324Error(f"render_shade_tex: colors must be fp32 [{nv},3] on the clip's device, got {tuple(col.shape)}")
    vn, normal_stride = None, 0
    if normals is not None:
        vn, normal_stride = _render_clip(normals, "render_shade_tex: normals")
        if tuple(vn.shape) != (T, nv, 3) or vn.device != dev:
            raise L.M324Error(f"render_shade_tex: normals must be fp32 [{T},{nv},3] on the clip's device, got {tuple(vn.shape)}")
    bg = [int(c) for c in background]
    if len(bg) != 3 or any(not 0 <= c <= 255 for c in bg) or not 0.0 <= float(ambient) <= 1.0:
        raise L.M324Error(f"render_shade_tex: background is three bytes and ambient lies in [0, 1], got {background!r}, {ambient!r}")
    uvs, th, tw = None, 0, 0
    if (face_uvs is None) != (mips is None) or (mips is None) != (tex_size is None):
        raise L.M324Error("render_shade_tex: face_uvs, mips and tex_size go together (a texture needs UVs, UVs need a texture)")
    if face_uvs is not None:
        if col is not None:
            raise L.M324Error("render_shade_tex: a texture and colors are two albedos: give one")
        uvs = _device_array(face_uvs, torch.float32, "render_shade_tex: face_uvs")
        if tuple(uvs.shape) != (f.shape[0], 3, 2) or uvs.device != dev:
            raise L.M324Error(f"render_shade_tex: face_uvs must be fp32 [{f.shape[0]},3,2] on the clip's device, got {tuple(uvs.shape)}")
        th, tw = (int(s) for s in tex_size)
        if not _is_device(mips) or mips.dtype != torch.uint8 or not mips.is_contiguous() or mips.device != dev or mips.numel() < texture_plan(th, tw)[1]:
            raise L.M324Error(f"render_shade_tex: mips must be the contiguous uint8 chain of a {th} x {tw} texture on the clip's device (texture_mips)")
    So = S // ss
    if out is None:
        out = (torch.empty((T, So, So, 3), dtype=torch.uint8, device=dev), torch.empty((T, S, S), dtype=torch.int32, device=dev),
               torch.empty((T, S, S), dtype=torch.int32, device=dev))
    rgb, face, depth = out
    for t, shape, dt, what in ((rgb, (T, So, So, 3), torch.uint8, "rgb"), (face, (T, S, S), torch.int32, "face"), (depth, (T, S, S), torch.int32, "depth")):
        if not _is_device(t) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise L.M324Error(f"render_shade_tex: out {what} must be a contiguous {dt} device tensor {shape}")
    _launch("m324_render_shade_tex", _p(f), f.shape[0], nv, T, S, _p(col), _p(vn), normal_stride, m.ctypes.data, float(ambient),
            bg[0] | bg[1] << 8 | bg[2] << 16, _p(uvs), _p(mips), th, tw, int(bool(use_mips)), ss, _p(rgb), _p(face), _p(depth), _p(scratch),
            scratch.numel())
    _wrote(rgb, face, depth)
    return rgb, face, depth


# ------------------------------------------------------------------------------------------------ volumetric IoU
VOXEL_MIN_SIDE, VOXEL_MAX_SIDE = 32, 1024   # M324_VOXEL_MIN_SIDE, M324_VOXEL_MAX_SIDE
VOXEL_BIG_VOXELS = 64           # default of big_voxels, measured against 16 / 256 / 1024 (profiles/voxel_iou.md); never in the result


def voxel_side(resolution: int, half: int = 2) -> int:
    """G = 2 * half * resolution, the voxels per axis of the grid over [-half, half)^3, after the refusals of include/m324.h"""
    if isinstance(resolution, bool) or isinstance(half, bool) or int(resolution) != resolution or int(half) != half:
        raise L.M324Error(f"voxel grid: resolution and half are integers, got {resolution!r}, {half!r}")
    resolution, half = int(resolution), int(half)
    if resolution < 16 or resolution % 16:
        raise L.M324Error(f"voxel grid: resolution must be a positive multiple of 16, got {resolution}")
    side = 2 * half * resolution
    if half < 1 or not VOXEL_MIN_SIDE <= side <= VOXEL_MAX_SIDE:
        raise L.M324Error(f"voxel grid: the side 2 * half * resolution must be in {VOXEL_MIN_SIDE}..{VOXEL_MAX_SIDE} (half={half} resolution={resolution})")
    return side


def voxel_plan(n_vertices: int, n_faces: int, frames: int, resolution: int, half: int = 2) -> int:
    """scratch bytes of m324_voxelize for these sizes: m324_voxel_plan, host-only"""
    return _plan_query("m324_voxel_plan", int(n_vertices), int(n_faces), int(frames), int(resolution), int(half))[1]


def _voxel_grid(grid, name: str) -> int:
    """the side G of a contiguous int32 device grid [T,G,G,G/32]"""
    _on_device(grid, name)
    s = tuple(grid.shape)
    if grid.dtype != torch.int32 or len(s) != 4 or s[0] < 1 or s[1] != s[2] or s[1] != 32 * s[3] or not VOXEL_MIN_SIDE <= s[1] <= VOXEL_MAX_SIDE \
            or not grid.is_contiguous():
        raise L.M324Error(f"{name}: expected a contiguous int32 grid [T,G,G,G/32] with G a multiple of 32 in {VOXEL_MIN_SIDE}..{VOXEL_MAX_SIDE}, "
                          f"got {grid.dtype} {s}")
    return s[1]


def voxelize(vertices: torch.Tensor, faces: torch.Tensor, resolution: int, half: int = 2, big_voxels: Optional[int] = None,
             scratch: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, faces_checked: bool = False):
    """Surface occupancy of every frame of a clip (m324_voxelize): vertices fp32 [T,V,3] (a view with contiguous last two axes is
    used in place), faces int32 [F,3] (F = 0 gives empty grids) -> (grid int32 [T,G,G,G/32], outside int32 [T]) over [-half, half)^3
    at `resolution` voxels per unit; bit layout and overlap rule in include/m324.h.  outside[t] counts the vertices of frame t the
    grid does not hold.  big_voxels: boxes larger than this go through the queued pass; None = VOXEL_BIG_VOXELS.  The grid does
    not depend on it.  out: the grid to write (it is zeroed by the call)."""
    side = voxel_side(resolution, half)
    v, stride_t = _render_clip(vertices, "voxelize: vertices")
    T, nv = v.shape[0], v.shape[1]
    f = _device_array(faces, torch.int32, "voxelize: faces")
    if f.dim() != 2 or f.shape[1] != 3:
        raise L.M324Error(f"voxelize: expected [F,3] int32 faces, got {tuple(f.shape)}")
    if f.device != v.device:
        raise L.M324Error("voxelize: vertices and faces live on different devices")
    nf = f.shape[0]
    if nf and not faces_checked:
        _faces_in_range(f, nv, "voxelize")
    big = VOXEL_BIG_VOXELS if big_voxels is None else int(big_voxels)
    if not 0 <= big <= 2 ** 31 - 1:
        raise L.M324Error(f"voxelize: big_voxels must be in 0..2^31-1, got {big_voxels}")
    need = voxel_plan(nv, nf, T, resolution, half)
    scratch = _render_scratch(scratch, need, v.device, "voxelize")
    if out is None:
        out = torch.empty((T, side, side, side // 32), dtype=torch.int32, device=v.device)
    elif _voxel_grid(out, "voxelize: out") != side or out.shape[0] != T or out.device != v.device:
        raise L.M324Error(f"voxelize: out must be an int32 grid [{T},{side},{side},{side // 32}] on the clip's device, got {tuple(out.shape)}")
    outside = torch.empty((T,), dtype=torch.int32, device=v.device)
    _launch("m324_voxelize", _p(v), stride_t, nv, _p(f) if nf else None, nf, T, int(resolution), int(half), big, _p(out), _p(outside), _p(scratch),
            scratch.numel())
    _wrote(out, outside, scratch)
    return out, outside


def voxel_fill(grid: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Orthographic fill of a grid (m324_voxel_fill): a voxel is set iff occupied voxels lie on both sides of it (or on it) along
    x, along y and along z.  Returns a new grid; out=grid fills in place (through a temporary of the grid's size), any other
    out is a second grid of the same shape."""
    side = _voxel_grid(grid, "voxel_fill")
    T = grid.shape[0]
    scratch = None
    if out is None:
        out = torch.empty_like(grid)
    elif out is grid or (_is_device(out) and out.data_ptr() == grid.data_ptr() and out.shape == grid.shape):
        scratch = torch.empty_like(grid)
    elif _voxel_grid(out, "voxel_fill: out") != side or out.shape != grid.shape or out.device != grid.device:
        raise L.M324Error(f"voxel_fill: out must be shaped like grid {tuple(grid.shape)} on its device, got {tuple(out.shape)}")
    _launch("m324_voxel_fill", _p(grid), _p(out), T, side, _p(scratch), scratch.numel() * 4 if scratch is not None else 0)
    _wrote(out)
    return out


def voxel_counts(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """int64 [T,3] = (|A|, |B|, |A & B|) per frame of two grids of the same shape (m324_voxel_counts); deterministic"""
    side = _voxel_grid(a, "voxel_counts: a")
    if _voxel_grid(b, "voxel_counts: b") != side or a.shape != b.shape or a.device != b.device:
        raise L.M324Error(f"voxel_counts: two grids of one shape on one device, got {tuple(a.shape)} / {tuple(b.shape)}")
    counts = torch.empty((a.shape[0], 3), dtype=torch.int64, device=a.device)
    _launch("m324_voxel_counts", _p(a), _p(b), a.shape[0], side, _p(counts))
    _wrote(counts)
    return counts


# ------------------------------------------------------------------------------------------------ convolution
# the 3 x 3 convolution and the 2 x 2 pool that the perceptual evaluation and the foreground matting share (csrc/conv.hip)
CONV_KPAD = 16                  # M324_CONV_KPAD: the packed weights have 9 Cin rows rounded up to this, zeros behind 9 Cin
CONV_MAX_CHANNELS = 4096        # M324_CONV_MAX_CHANNELS
CONV_MAX_DILATION = 64          # M324_CONV_MAX_DILATION


def conv_kpad(cin: int) -> int:
    """rows of the K-major weight matrix m324_conv3x3 reads for `cin` input channels"""
    return (9 * int(cin) + CONV_KPAD - 1) // CONV_KPAD * CONV_KPAD


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] (torch's layout) -> fp32 [Kpad, Cout] with row (3 ky + kx) * Cin4 + c, Cin4 = Cin rounded up to a multiple
    of 4 (the pad channels are zero rows: the first layer's three channels become four) and zero rows up to Kpad."""
    cout, cin = int(w.shape[0]), int(w.shape[1])
    cin4 = (cin + 3) // 4 * 4
    packed = torch.zeros((conv_kpad(cin4), cout), dtype=torch.float32)
    taps = torch.zeros((9, cin4, cout), dtype=torch.float32)
    taps[:, :cin] = w.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(9, cin, cout)
    packed[:9 * cin4] = taps.reshape(9 * cin4, cout)
    return packed


def _nhwc(x, name: str) -> torch.Tensor:
    x = _device_array(x, torch.float32, name)
    if x.dim() != 4 or 0 in x.shape or x.shape[3] % 4 or x.shape[3] > CONV_MAX_CHANNELS:
        raise L.M324Error(f"{name}: expected fp32 NHWC [images,H,W,C] with C a multiple of 4 up to {CONV_MAX_CHANNELS}, got {tuple(x.shape)}")
    if x.shape[0] * x.shape[1] * x.shape[2] >= 2 ** 31:
        raise L.M324Error(f"{name}: images * H * W must stay below 2^31, got {tuple(x.shape)}")
    return x


def _out_like(out, shape, device, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not _is_device(out) or out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise L.M324Error(f"{name}: out must be a contiguous fp32 device tensor {tuple(shape)}")
    return out


def _conv_weights(wp, bias, cin: int, cin_text: str, multiple: int, name: str):
    """wp [conv_kpad(cin), Cout] and bias [Cout] of the convolution `name`, Cout a multiple of `multiple`: (wp, bias, Cout)"""
    wp = _device_array(wp, torch.float32, f"{name}: wp")
    bias = _device_array(bias, torch.float32, f"{name}: bias")
    if cin > CONV_MAX_CHANNELS or wp.dim() != 2 or wp.shape[0] != conv_kpad(cin):
        raise L.M324Error(f"{name}: wp must be [{conv_kpad(cin)},Cout] for {cin_text}, got {tuple(wp.shape)}")
    cout = wp.shape[1]
    if cout % multiple or not multiple <= cout <= CONV_MAX_CHANNELS or tuple(bias.shape) != (cout,):
        raise L.M324Error(f"{name}: Cout must be a multiple of {multiple} up to {CONV_MAX_CHANNELS} with bias [Cout], got wp {tuple(wp.shape)}, "
                          f"bias {tuple(bias.shape)}")
    return wp, bias, cout


def conv3x3(x: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, *, relu: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3 x 3 convolution, stride 1, zero padding 1, bias and (relu) max(., 0) (m324_conv3x3, fp32 MFMA): x fp32 NHWC
    [images,H,W,Cin], Cin % 4 = 0; wp fp32 [conv_kpad(Cin), Cout], row (3 (dy + 1) + dx + 1) * Cin + c, zeros behind 9 Cin
    (pack_conv_weight makes it); bias fp32 [Cout], Cout % 32 = 0.  Returns fp32 [images,H,W,Cout]."""
    x = _nhwc(x, "conv3x3: x")
    n, H, W, cin = x.shape
    wp, bias, cout = _conv_weights(wp, bias, cin, f"Cin {cin}", 32, "conv3x3")
    out = _out_like(out, (n, H, W, cout), x.device, "conv3x3")
    _launch("m324_conv3x3", _p(x), _p(wp), _p(bias), _p(out), n, H, W, cin, cout, 1 if relu else 0)
    _wrote(out)
    return out


def conv3x3_ex_tile(images: int, H: int, W: int, cout: int) -> int:
    """output channels per workgroup tile (128, 64 or 32) m324_conv3x3_ex takes for this shape: host-only, never in the bits"""
    n = int(L.load().m324_conv3x3_ex_tile(int(images), int(H), int(W), int(cout)))
    L.check(0 if n > 0 else n, "m324_conv3x3_ex_tile")
    return n


def conv3x3_ex(a: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, *, b: Optional[torch.Tensor] = None, dilation: int = 1, relu: bool = True,
               res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dilated 3 x 3 convolution over the channel concatenation of a and (optionally) b, which is never built, with bias,
    (relu) max(., 0) and an optional residual added last (m324_conv3x3_ex, fp32 MFMA): a [images,H,W,Ca], b [images,H,W,Cb],
    Ca % 4 = Cb % 4 = 0; wp fp32 [conv_kpad(Ca + Cb), Cout] laid out as for conv3x3 with Cin = Ca + Cb; bias [Cout], Cout % 4 = 0;
    res [images,H,W,Cout].  Returns fp32 [images,H,W,Cout] = act(conv + bias) + res."""
    a = _nhwc(a, "conv3x3_ex: a")
    n, H, W, ca = a.shape
    cb = 0
    if b is not None:
        b = _nhwc(b, "conv3x3_ex: b")
        if tuple(b.shape[:3]) != (n, H, W) or b.device != a.device:
            raise L.M324Error(f"conv3x3_ex: b {tuple(b.shape)} does not match a {tuple(a.shape)}, or lives on another device")
        cb = b.shape[3]
    wp, bias, cout = _conv_weights(wp, bias, ca + cb, f"Ca + Cb = {ca} + {cb} <= {CONV_MAX_CHANNELS}", 4, "conv3x3_ex")
    if not 1 <= int(dilation) <= CONV_MAX_DILATION:
        raise L.M324Error(f"conv3x3_ex: dilation must be in 1..{CONV_MAX_DILATION}, got {dilation}")
    if res is not None:
        res = _device_array(res, torch.float32, "conv3x3_ex: res")
        if tuple(res.shape) != (n, H, W, cout) or res.device != a.device:
            raise L.M324Error(f"conv3x3_ex: res must be {(n, H, W, cout)} on a's device, got {tuple(res.shape)}")
    out = _out_like(out, (n, H, W, cout), a.device, "conv3x3_ex")
    _launch("m324_conv3x3_ex", _p(a), ca, _p(b), cb, _p(wp), _p(bias), _p(res), _p(out), n, H, W, cout, int(dilation), 1 if relu else 0)
    _wrote(out)
    return out


def conv3x3_s2(x: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, *, relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3 x 3 convolution with stride 2 and zero padding 1, bias and (relu) max(., 0) (m324_conv3x3_s2, the kernel of conv3x3_ex with
    a strided gather): x fp32 NHWC [images,H,W,Cin], Cin % 4 = 0; wp, bias as for conv3x3_ex with one source, Cout % 4 = 0.  Returns
    fp32 [images,(H - 1) // 2 + 1,(W - 1) // 2 + 1,Cout], the bits of conv3x3_ex(x, wp, bias, relu=relu)[:, ::2, ::2]."""
    x = _nhwc(x, "conv3x3_s2: x")
    n, H, W, cin = x.shape
    wp, bias, cout = _conv_weights(wp, bias, cin, f"Cin {cin}", 4, "conv3x3_s2")
    out = _out_like(out, (n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout), x.device, "conv3x3_s2")
    _launch("m324_conv3x3_s2", _p(x), _p(wp), _p(bias), _p(out), n, H, W, cin, cout, 1 if relu else 0)
    _wrote(out)
    return out


def maxpool2x2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """2 x 2, stride 2 max-pool of fp32 NHWC [images,H,W,C] with even H, W (m324_maxpool2x2) -> [images,H/2,W/2,C]"""
    x = _nhwc(x, "maxpool2x2: x")
    n, H, W, c = x.shape
    if H % 2 or W % 2:
        raise L.M324Error(f"maxpool2x2: H and W must be even, got {H} x {W}")
    out = _out_like(out, (n, H // 2, W // 2, c), x.device, "maxpool2x2")
    _launch("m324_maxpool2x2", _p(x), _p(out), n, H, W, c)
    _wrote(out)
    return out


def maxpool2x2_ceil(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """2 x 2, stride 2 max-pool with the window cut at the edge (MaxPool2d(2, 2, ceil_mode=True); m324_maxpool2x2_ceil): fp32
    NHWC [images,H,W,C] -> [images,ceil(H/2),ceil(W/2),C]"""
    x = _nhwc(x, "maxpool2x2_ceil: x")
    n, H, W, c = x.shape
    out = _out_like(out, (n, (H + 1) // 2, (W + 1) // 2, c), x.device, "maxpool2x2_ceil")
    _launch("m324_maxpool2x2_ceil", _p(x), _p(out), n, H, W, c)
    _wrote(out)
    return out


# ------------------------------------------------------------------------------------------------ 3D convolution (video metric)
# the pieces of the I3D trunk behind FVD (csrc/conv3d.hip): fp32 NDHWC, channel slices in and out
CONV3D_BOXES = (1, 3, 7)        # side of the tap boxes m324_conv3d has instances of
CONV3D_MAX_STRIDE = 16384       # M324_CONV3D_MAX_STRIDE: the widest tensor a channel slice may be cut from
POOL3D_WINDOWS = ((1, 3, 3), (3, 3, 3), (2, 2, 2))
I3D_HEAD_MAX_SAMPLES = 65536    # M324_I3D_HEAD_MAX_SAMPLES
I3D_HEAD_MAX_SIDE = 64          # M324_I3D_HEAD_MAX_SIDE
FVD_MODES = {torch.uint8: 0, torch.float32: 1}         # M324_FVD_U8, M324_FVD_F32


def same_padding(n: int, k: int, s: int):
    """TensorFlow's "SAME" rule along one axis of n samples, window k, stride s: (front padding, output size).  The one place
    the rule lives: the kernels take the front padding as an argument and derive the output size ceil(n / s) themselves."""
    n, k, s = int(n), int(k), int(s)
    if n < 1 or k < 1 or s < 1:
        raise L.M324Error(f"same_padding: n, k and s must be at least 1, got {n}, {k}, {s}")
    total = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
    return total // 2, -(-n // s)


def conv3d_kpad(cin: int, box: int) -> int:
    """rows of the K-major weight matrix m324_conv3d reads for `cin` input channels and a tap box of side `box`"""
    return (int(box) ** 3 * int(cin) + CONV_KPAD - 1) // CONV_KPAD * CONV_KPAD


def pack_conv3d_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, k, k, k] (torch's layout) -> fp32 [Kpad, Cout] with row ((dt k + dh) k + dw) * Cin4 + c, Cin4 = Cin rounded up
    to a multiple of 4 (zero rows for the pad channels: the stem's three channels become four) and zero rows up to Kpad."""
    if w.dim() != 5 or w.shape[2] not in CONV3D_BOXES or not (w.shape[2] == w.shape[3] == w.shape[4]):
        raise L.M324Error(f"pack_conv3d_weight: expected [Cout,Cin,k,k,k] with k in {CONV3D_BOXES}, got {tuple(w.shape)}")
    cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    cin4 = (cin + 3) // 4 * 4
    packed = torch.zeros((conv3d_kpad(cin4, k), cout), dtype=torch.float32)
    taps = torch.zeros((k ** 3, cin4, cout), dtype=torch.float32)
    taps[:, :cin] = w.detach().to(torch.float32).permute(2, 3, 4, 1, 0).reshape(k ** 3, cin, cout)
    packed[:k ** 3 * cin4] = taps.reshape(k ** 3 * cin4, cout)
    return packed


def _ndhwc(x, name: str, sliced: bool) -> int:
    """Checks fp32 NDHWC [samples,T,H,W,C] on the device, C % 4 = 0, 16-byte aligned; dense, or (sliced) a channel slice of a
    dense tensor: returns the channel stride"""
    _on_device(x, name)
    if x.dtype != torch.float32 or x.dim() != 5 or 0 in x.shape or x.shape[4] % 4 or x.shape[4] > CONV_MAX_CHANNELS:
        raise L.M324Error(f"{name}: expected fp32 NDHWC [samples,T,H,W,C] with C a multiple of 4 up to {CONV_MAX_CHANNELS}, got {x.dtype} {tuple(x.shape)}")
    n, T, H, W, c = x.shape
    if n * T * H * W >= 2 ** 31:
        raise L.M324Error(f"{name}: samples * T * H * W must stay below 2^31, got {tuple(x.shape)}")
    ld = _channel_stride(x)
    dense = (T * H * W * ld, H * W * ld, W * ld, ld, 1)
    if any(x.shape[i] > 1 and x.stride(i) != dense[i] for i in range(5)) or ld < c or ld % 4 or ld > CONV3D_MAX_STRIDE or (not sliced and ld != c):
        raise L.M324Error(f"{name}: expected a dense NDHWC tensor" + (" or a channel slice of one (channel stride a multiple of 4 up to "
                          f"{CONV3D_MAX_STRIDE})" if sliced else "") + f", got shape {tuple(x.shape)} strides {x.stride()}")
    if x.data_ptr() % 16:
        raise L.M324Error(f"{name}: must be 16-byte aligned (a slice starts at a channel that is a multiple of 4)")
    return ld


def _channel_stride(x) -> int:
    """channel stride of an NDHWC tensor: from the stride of the innermost axis longer than 1 (-1 when that is no whole number of
    voxels), the width when there is one voxel"""
    for i in (3, 2, 1, 0):
        if x.shape[i] > 1:
            q, r = divmod(x.stride(i), math.prod(x.shape[i + 1:4]))
            return q if r == 0 else -1
    return x.shape[4]


def _triple(v, name: str):
    v = tuple(int(a) for a in ((v,) * 3 if isinstance(v, int) else v))
    if len(v) != 3:
        raise L.M324Error(f"{name}: expected three values (t, h, w), got {v}")
    return v


def _geometry3d(shape, window, stride, padding, name: str):
    """(strides, front padding, output sizes) of a window over [T,H,W]; padding None is the SAME rule"""
    stride = _triple(stride, f"{name}: stride")
    if any(s not in (1, 2) for s in stride):
        raise L.M324Error(f"{name}: every stride is 1 or 2, got {stride}")
    same = tuple(same_padding(n, k, s) for n, k, s in zip(shape, window, stride))
    padding = tuple(f for f, _ in same) if padding is None else _triple(padding, f"{name}: padding")
    if any(not 0 <= p < k for p, k in zip(padding, window)):
        raise L.M324Error(f"{name}: the front padding must be in 0..k - 1 per axis, got {padding} for the window {tuple(window)}")
    return stride, padding, tuple(o for _, o in same)


def _out_slice(out, shape, device, name: str):
    """(out, channel stride): a new dense tensor, or the caller's dense tensor or channel slice of that shape"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device), shape[4]
    if not _is_device(out) or out.device != device or tuple(out.shape) != tuple(shape):
        raise L.M324Error(f"{name}: out must be an fp32 device tensor {tuple(shape)} (dense, or a channel slice of a dense tensor)")
    _ndhwc(out, f"{name}: out", True)
    return out, _channel_stride(out)


def conv3d_tile(voxels: int, cout: int) -> int:
    """output channels per workgroup tile (128, 64 or 32) m324_conv3d takes for this many output voxels: host-only, never in the bits"""
    n = int(L.load().m324_conv3d_tile(int(voxels), int(cout)))
    L.check(0 if n > 0 else n, "m324_conv3d_tile")
    return n


def conv3d(x: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, *, box: int, stride=(1, 1, 1), padding=None, relu: bool = True,
           out: Optional[torch.Tensor] = None, tile: int = 0) -> torch.Tensor:
    """3D convolution with a (box, box, box) tap box, box in 1, 3, 7, per-axis strides 1 or 2, bias and (relu) max(., 0)
    (m324_conv3d, fp32 MFMA).  x fp32 NDHWC [samples,T,H,W,Cin], dense or a channel slice of a dense tensor, Cin % 4 = 0; wp fp32
    [conv3d_kpad(Cin, box), Cout] (pack_conv3d_weight makes it); bias [Cout], Cout % 8 = 0.  padding: the front padding (pt, ph, pw),
    None for the SAME rule (same_padding); voxels outside the volume read as zero.  out: None, or a tensor [samples,To,Ho,Wo,Cout]
    that may be a channel slice of a wider dense tensor, whose other channels are left alone.  tile: 0 lets the library choose,
    32 / 64 / 128 force a tile width; the bits are the same.  Returns out, [samples,ceil(T/st),ceil(H/sh),ceil(W/sw),Cout]."""
    if int(box) not in CONV3D_BOXES:
        raise L.M324Error(f"conv3d: the tap box is (1,1,1), (3,3,3) or (7,7,7), got side {box}")
    box = int(box)
    lda = _ndhwc(x, "conv3d: x", True)
    n, T, H, W, cin = x.shape
    wp = _device_array(wp, torch.float32, "conv3d: wp")
    bias = _device_array(bias, torch.float32, "conv3d: bias")
    if wp.dim() != 2 or wp.shape[0] != conv3d_kpad(cin, box):
        raise L.M324Error(f"conv3d: wp must be [{conv3d_kpad(cin, box)},Cout] for Cin {cin} and box {box}, got {tuple(wp.shape)}")
    cout = wp.shape[1]
    if cout % 8 or not 8 <= cout <= CONV_MAX_CHANNELS or tuple(bias.shape) != (cout,):
        raise L.M324Error(f"conv3d: Cout must be a multiple of 8 up to {CONV_MAX_CHANNELS} with bias [Cout], got wp {tuple(wp.shape)}, bias {tuple(bias.shape)}")
    if int(tile) not in (0, 32, 64, 128):
        raise L.M324Error(f"conv3d: tile is 0, 32, 64 or 128, got {tile}")
    stride, padding, (To, Ho, Wo) = _geometry3d((T, H, W), (box,) * 3, stride, padding, "conv3d")
    out, ldo = _out_slice(out, (n, To, Ho, Wo, cout), x.device, "conv3d")
    _launch("m324_conv3d", _p(x), lda, _p(wp), _p(bias), _p(out), ldo, n, T, H, W, cin, cout, box, *stride, *padding, 1 if relu else 0, int(tile))
    _wrote(out)
    return out


def maxpool3d(x: torch.Tensor, window, stride, padding=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3D max-pool with the window (1,3,3), (3,3,3) or (2,2,2) and per-axis strides 1 or 2 (m324_maxpool3d).  Padding (None: the
    SAME rule) is excluded from the maximum.  x dense fp32 NDHWC, C % 4 = 0; out as for conv3d.  Exact."""
    window = _triple(window, "maxpool3d: window")
    if window not in POOL3D_WINDOWS:
        raise L.M324Error(f"maxpool3d: the window is (1,3,3), (3,3,3) or (2,2,2), got {window}")
    _ndhwc(x, "maxpool3d: x", False)
    n, T, H, W, c = x.shape
    stride, padding, (To, Ho, Wo) = _geometry3d((T, H, W), window, stride, padding, "maxpool3d")
    out, ldo = _out_slice(out, (n, To, Ho, Wo, c), x.device, "maxpool3d")
    _launch("m324_maxpool3d", _p(x), _p(out), ldo, n, T, H, W, c, *window, *stride, *padding)
    _wrote(out)
    return out


def i3d_head(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The head of I3D (m324_i3d_head): x dense fp32 [samples,T,hw,hw,C], T >= 2; the average over a (2, hw, hw) window with stride
    1 in time, the 1 x 1 x 1 logits layer w fp32 [C,classes] with bias b [classes], and the mean over the T - 1 time steps.
    Returns fp32 [samples,classes].  A fixed order of sums (include/m324.h): deterministic, independent of the batch."""
    _ndhwc(x, "i3d_head: x", False)
    n, T, hh, hw, c = x.shape
    if hh != hw or not 2 <= T <= I3D_HEAD_MAX_SIDE or hw > I3D_HEAD_MAX_SIDE or n > I3D_HEAD_MAX_SAMPLES:
        raise L.M324Error(f"i3d_head: expected [samples,T,hw,hw,C] with T in 2..{I3D_HEAD_MAX_SIDE}, hw up to {I3D_HEAD_MAX_SIDE} and at most "
                          f"{I3D_HEAD_MAX_SAMPLES} samples, got {tuple(x.shape)}")
    w = _device_array(w, torch.float32, "i3d_head: w")
    b = _device_array(b, torch.float32, "i3d_head: b")
    if w.dim() != 2 or w.shape[0] != c or not 1 <= w.shape[1] <= CONV_MAX_CHANNELS or tuple(b.shape) != (w.shape[1],):
        raise L.M324Error(f"i3d_head: w must be [{c},classes] with classes up to {CONV_MAX_CHANNELS} and b [classes], got {tuple(w.shape)}, {tuple(b.shape)}")
    classes = w.shape[1]
    if out is None:
        out = torch.empty((n, classes), dtype=torch.float32, device=x.device)
    elif not _is_device(out) or out.dtype != torch.float32 or tuple(out.shape) != (n, classes) or not out.is_contiguous() or out.device != x.device:
        raise L.M324Error(f"i3d_head: out must be a contiguous fp32 device tensor {(n, classes)}")
    pooled = torch.empty((n * (T - 1) * c,), dtype=torch.float32, device=x.device)
    _launch("m324_i3d_head", _p(x), _p(w), _p(b), _p(pooled), _p(out), n, T, hw, c, classes)
    _wrote(out)
    return out


def fvd_geometry(H: int, W: int, resolution: Optional[int] = 224):
    """(Hr, Wr, y0, x0, Ho, Wo) of the reference's preprocess_single: the shorter side scaled to `resolution`, the longer to
    ceil(side * resolution / shorter), and the centre resolution x resolution crop.  resolution None: the frame as it is."""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or (resolution is not None and int(resolution) < 1):
        raise L.M324Error(f"fvd_geometry: sizes must be at least 1, got {H} x {W} -> {resolution}")
    if resolution is None:
        return H, W, 0, 0, H, W
    r = int(resolution)
    scale = r / min(H, W)
    Hr, Wr = (r, math.ceil(W * scale)) if H < W else (math.ceil(H * scale), r)
    return Hr, Wr, (Hr - r) // 2, (Wr - r) // 2, r, r


def fvd_prepare(src: torch.Tensor, resolution: Optional[int] = 224, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The trunk's input fp32 NDHWC [samples,T,res,res,4] (channel 3 is zero) from clips uint8 [samples,T,H,W,3] or fp32 in [0, 1]
    of that shape (m324_fvd_prepare): bilinear resize (align_corners=False, no antialiasing) of the shorter side to `resolution`,
    centre crop, (v - 0.5) * 2.  resolution None keeps the frames' own size."""
    _on_device(src, "fvd_prepare")
    if src.dtype not in FVD_MODES or src.dim() != 5 or src.shape[4] != 3 or 0 in src.shape:
        raise L.M324Error(f"fvd_prepare: expected uint8 or fp32 [samples,T,H,W,3], got {src.dtype} {tuple(src.shape)}")
    n, T, H, W = src.shape[:4]
    Hr, Wr, y0, x0, Ho, Wo = fvd_geometry(H, W, resolution)
    if max(H, W, Hr, Wr) > MATTE_MAX_SIDE or n * T * H * W >= 2 ** 31 or n * T * Ho * Wo >= 2 ** 31:
        raise L.M324Error(f"fvd_prepare: sizes up to {MATTE_MAX_SIDE} and samples * T * H * W below 2^31, got {tuple(src.shape)} -> {Hr} x {Wr}")
    src = src.detach().contiguous()
    if out is None:
        out = torch.empty((n, T, Ho, Wo, 4), dtype=torch.float32, device=src.device)
    elif not _is_device(out) or out.dtype != torch.float32 or tuple(out.shape) != (n, T, Ho, Wo, 4) or not out.is_contiguous() or out.device != src.device:
        raise L.M324Error(f"fvd_prepare: out must be a contiguous fp32 device tensor {(n, T, Ho, Wo, 4)}")
    _launch("m324_fvd_prepare", _p(src), FVD_MODES[src.dtype], n * T, H, W, Hr, Wr, y0, x0, Ho, Wo, _p(out))
    _wrote(out)
    return out


# ------------------------------------------------------------------------------------------------ perceptual evaluation
LPIPS_MAX_CHANNELS = 1024      # M324_LPIPS_MAX_CHANNELS
LPIPS_CHUNKS = 64               # M324_LPIPS_CHUNKS
LPIPS_MODES = {"u8_nhwc": 0, "f32_nchw": 1}


def lpips_prepare(src: torch.Tensor, *, normalize: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The trunk's scaled input fp32 [images,H,W,4] (channel 3 is zero) from uint8 [images,H,W,3] or fp32 [images,3,H,W] in
    [-1, 1] -- in [0, 1] with normalize (m324_lpips_prepare; the formula is in include/m324.h)."""
    _on_device(src, "lpips_prepare")
    if src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3 and 0 not in src.shape:
        mode, (n, H, W) = LPIPS_MODES["u8_nhwc"], src.shape[:3]
        if normalize:
            raise L.M324Error("lpips_prepare: normalize applies to fp32 input only; bytes are always 0..255")
    elif src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == 3 and 0 not in src.shape:
        mode, (n, H, W) = LPIPS_MODES["f32_nchw"], (src.shape[0], src.shape[2], src.shape[3])
    else:
        raise L.M324Error(f"lpips_prepare: expected uint8 [images,H,W,3] or fp32 [images,3,H,W], got {src.dtype} {tuple(src.shape)}")
    if n * H * W >= 2 ** 31:
        raise L.M324Error(f"lpips_prepare: images * H * W must stay below 2^31, got {tuple(src.shape)}")
    src = src.detach().contiguous()
    out = _out_like(out, (n, H, W, 4), src.device, "lpips_prepare")
    _launch("m324_lpips_prepare", _p(src), mode, 1 if normalize else 0, n, H, W, _p(out))
    _wrote(out)
    return out


def lpips_layer(fa: torch.Tensor, fb: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One LPIPS layer (m324_lpips_layer): fa, fb fp32 NHWC [pairs,H,W,C] taps of the two clips, w fp32 [C] the 1 x 1 layer;
    returns fp32 [pairs], the mean over the pixels of sum_c w_c (n(fa)_c - n(fb)_c)^2.  Deterministic, symmetric in fa and fb."""
    fa, fb = _nhwc(fa, "lpips_layer: fa"), _nhwc(fb, "lpips_layer: fb")
    w = _device_array(w, torch.float32, "lpips_layer: w")
    n, H, W, c = fa.shape
    if fb.shape != fa.shape or tuple(w.shape) != (c,) or c > LPIPS_MAX_CHANNELS or H * W > 2 ** 24:
        raise L.M324Error(f"lpips_layer: expected fa and fb of one shape [pairs,H,W,C], C <= {LPIPS_MAX_CHANNELS}, H * W <= 2^24, and w [C]; "
                          f"got {tuple(fa.shape)}, {tuple(fb.shape)}, {tuple(w.shape)}")
    out = _out_like(out, (n,), fa.device, "lpips_layer")
    partial = torch.empty((n * LPIPS_CHUNKS,), dtype=torch.float32, device=fa.device)
    _launch("m324_lpips_layer", _p(fa), _p(fb), _p(w), n, H * W, c, _p(partial), _p(out))
    _wrote(out)
    return out


# ------------------------------------------------------------------------------------------------ ViT image tower (fp32)
ATTN_TOK_MAX_D = 128            # m324_attention_tok: D % 8 == 0, 8 <= D <= 128
LAYERNORM_WIDE_MAX_C = 4096     # m324_layernorm_wide: C % 4 == 0, 4 <= C <= 4096


def _f32_rows(t, name: str):
    _on_device(t, name)
    if t.dtype != torch.float32:
        raise L.M324Error(f"{name}: expected fp32, got {t.dtype}")
    return _rows(t, name)


def attention_tok(qkv: torch.Tensor, B: int, L_: int, H: int, D: int, scale: Optional[float] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 self-attention from the token-major q|k|v rows of a fused in-projection (m324_attention_tok): qkv [B * L, >= 3 H D]
    with q, k, v at columns 0, H D, 2 H D (+ h D); returns out [B * L, >= H D], of which only the first H D columns are
    written.  scale None: D ** -0.5.  The library refuses the head widths and leading dimensions it does not do."""
    pq, ld = _f32_rows(qkv, "attention_tok: qkv")
    B, L_, H, D = int(B), int(L_), int(H), int(D)
    if out is None:
        out = torch.empty((B * L_, H * D), dtype=torch.float32, device=qkv.device)
    po, ldo = _f32_rows(out, "attention_tok: out")
    if min(B, L_, H, D) < 1 or qkv.shape[0] < B * L_ or out.shape[0] < B * L_ or qkv.shape[1] < 3 * H * D or out.shape[1] < H * D \
            or out.device != qkv.device:
        raise L.M324Error(f"attention_tok: qkv{tuple(qkv.shape)} / out{tuple(out.shape)} do not hold B={B} L={L_} H={H} D={D}")
    scale = D ** -0.5 if scale is None else float(scale)
    tag = f"attn_tok_kernel | B={B} L={L_} H={H} D={D}" if _timing() else ""
    with span("attention", 4.0 * B * H * L_ * L_ * D, 4.0 * B * L_ * H * D * 4, tag):
        _launch("m324_attention_tok", pq, ld, po, ldo, B, L_, H, D, scale)
    _wrote(out)
    return out


def layernorm_wide(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float, out: Optional[torch.Tensor] = None,
                   rows: Optional[int] = None) -> torch.Tensor:
    """fp32 LayerNorm over the last dimension for C up to 4096 (m324_layernorm_wide): x [>= rows, C] with any leading dimension
    that is a multiple of 4 (a strided row selection is a view), out [>= rows, C]; rows None: x.shape[0]."""
    px, ldx = _f32_rows(x, "layernorm_wide: x")
    Cdim = x.shape[1]
    rows = x.shape[0] if rows is None else int(rows)
    if out is None:
        out = torch.empty((rows, Cdim), dtype=torch.float32, device=x.device)
    py, ldy = _f32_rows(out, "layernorm_wide: out")
    if rows < 1 or x.shape[0] < rows or out.shape[0] < rows or out.shape[1] != Cdim or out.device != x.device:
        raise L.M324Error(f"layernorm_wide: x{tuple(x.shape)} / out{tuple(out.shape)} do not hold {rows} rows of one width")
    tag = f"layernorm_wide_kernel | rows={rows} C={Cdim}" if _timing() else ""
    with span("hbm_pass", 0.0, float(rows) * Cdim * 8, tag):
        _launch("m324_layernorm_wide", px, ldx, _vec(w, Cdim, "layernorm_wide: w"), _vec(b, Cdim, "layernorm_wide: b"), float(eps), py, ldy,
                rows, Cdim)
    _wrote(out)
    return out


def vit_patches(img: torch.Tensor, patch: int, mean_std: torch.Tensor, Kp: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Patch rows fp32 [F * g * g, Kp] of square byte images uint8 [F,S,S,3] (m324_vit_patches): ToTensor, then Normalize with
    mean_std = fp32 [6] on the device (three means, three standard deviations); columns past 3 patch^2 are zero."""
    _on_device(img, "vit_patches")
    if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3 or img.shape[1] != img.shape[2] or 0 in img.shape:
        raise L.M324Error(f"vit_patches: expected uint8 [F,S,S,3], got {img.dtype} {tuple(img.shape)}")
    F_, S = img.shape[0], img.shape[1]
    patch, Kp = int(patch), int(Kp)
    if patch < 1 or S % patch:
        raise L.M324Error(f"vit_patches: the image side {S} is no multiple of the patch {patch}")
    g = S // patch
    img = img.detach().contiguous()
    mean_std = _device_array(mean_std, torch.float32, "vit_patches: mean_std")
    if mean_std.numel() != 6 or mean_std.device != img.device:
        raise L.M324Error("vit_patches: mean_std must be fp32 [6] on the images' device")
    out = _out_like(out, (F_ * g * g, Kp), img.device, "vit_patches")
    _launch("m324_vit_patches", _p(img), F_, S, patch, _p(mean_std), _p(out), Kp)
    _wrote(out)
    return out


def vit_tokens(patch_rows: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The tower's input stream fp32 [F * L, C] (m324_vit_tokens): per image the class token, then its L - 1 patch rows, each
    plus its row of pos [L, C]."""
    for t, name in ((patch_rows, "patch_rows"), (cls, "cls"), (pos, "pos")):
        _on_device(t, "vit_tokens: " + name)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise L.M324Error(f"vit_tokens: {name} must be contiguous fp32, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    if pos.dim() != 2 or patch_rows.dim() != 2 or pos.shape[0] < 2 or patch_rows.shape[1] != pos.shape[1] or cls.numel() != pos.shape[1] \
            or patch_rows.shape[0] == 0 or patch_rows.shape[0] % (pos.shape[0] - 1):
        raise L.M324Error(f"vit_tokens: patch_rows{tuple(patch_rows.shape)}, cls{tuple(cls.shape)} and pos{tuple(pos.shape)} do not fit "
                          f"[F * (L - 1), C], [C] and [L, C]")
    L_, Cdim = pos.shape
    F_ = patch_rows.shape[0] // (L_ - 1)
    out = _out_like(out, (F_ * L_, Cdim), patch_rows.device, "vit_tokens")
    _launch("m324_vit_tokens", _p(patch_rows), _p(cls), _p(pos), _p(out), F_, L_, Cdim)
    _wrote(out)
    return out


RESAMPLE_MAX_SIDE = 16384       # m324_resample_f32: sides of 1 to 16384
RESAMPLE_MAX_KSIZE = 64         # m324_resample_f32: 1 <= ksize <= 64
RESAMPLE_AXES = {"x": 0, "y": 1}


def resample_f32(src: torch.Tensor, weights: torch.Tensor, first: torch.Tensor, axis: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One separable pass of a float resize (m324_resample_f32): src uint8 [F,H,W,3] (a sample is v / 255 in fp32) or fp32 planar
    [F,3,H,W]; weights fp32 [n_out, ksize] and first int32 [n_out] on the device (dreamsim.resize_tables); returns fp32 planar
    [F,3,H,n_out] (axis "x") or [F,3,n_out,W] (axis "y"): per output an fp32 fma chain in tap order."""
    _on_device(src, "resample_f32")
    if axis not in RESAMPLE_AXES:
        raise L.M324Error(f"resample_f32: axis must be 'x' or 'y', got {axis!r}")
    if src.dim() == 4 and src.dtype == torch.uint8 and src.shape[3] == 3:
        F_, H, W, u8 = src.shape[0], src.shape[1], src.shape[2], 1
    elif src.dim() == 4 and src.dtype == torch.float32 and src.shape[1] == 3:
        F_, H, W, u8 = src.shape[0], src.shape[2], src.shape[3], 0
    else:
        raise L.M324Error(f"resample_f32: expected uint8 [F,H,W,3] or fp32 [F,3,H,W], got {getattr(src, 'dtype', None)} {tuple(src.shape)}")
    if F_ < 1 or not 1 <= H <= RESAMPLE_MAX_SIDE or not 1 <= W <= RESAMPLE_MAX_SIDE:
        raise L.M324Error(f"resample_f32: at least one frame and sides of 1 to {RESAMPLE_MAX_SIDE}, got {tuple(src.shape)}")
    src = src.detach().contiguous()
    weights = _device_array(weights, torch.float32, "resample_f32: weights")
    first = _device_array(first, torch.int32, "resample_f32: first")
    if weights.dim() != 2 or first.dim() != 1 or first.shape[0] != weights.shape[0] or weights.device != src.device or first.device != src.device \
            or not 1 <= weights.shape[0] <= RESAMPLE_MAX_SIDE or not 1 <= weights.shape[1] <= RESAMPLE_MAX_KSIZE:
        raise L.M324Error(f"resample_f32: weights{tuple(weights.shape)} / first{tuple(first.shape)} must be fp32 [n_out, ksize] and int32 [n_out] "
                          f"on the source's device (n_out up to {RESAMPLE_MAX_SIDE}, ksize up to {RESAMPLE_MAX_KSIZE})")
    n_out, ksize = weights.shape
    ax = RESAMPLE_AXES[axis]
    out = _out_like(out, (F_, 3, H, n_out) if ax == 0 else (F_, 3, n_out, W), src.device, "resample_f32")
    if out.data_ptr() == src.data_ptr():
        raise L.M324Error("resample_f32: out must not be the source")
    _launch("m324_resample_f32", _p(src), u8, F_, H, W, ax, _p(weights), _p(first), ksize, n_out, _p(out))
    _wrote(out)
    return out


def vit_patches_f32(img: torch.Tensor, patch: int, mean_std: torch.Tensor, Kp: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Patch rows fp32 [F * g * g, Kp] of square fp32 planar images [F,3,S,S] (m324_vit_patches_f32): (x - mean) / std with
    mean_std = fp32 [6] on the device, vit_patches' column order; columns past 3 patch^2 are zero."""
    _on_device(img, "vit_patches_f32")
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 3 or img.shape[2] != img.shape[3] or 0 in img.shape:
        raise L.M324Error(f"vit_patches_f32: expected fp32 [F,3,S,S], got {img.dtype} {tuple(img.shape)}")
    F_, S = img.shape[0], img.shape[2]
    patch, Kp = int(patch), int(Kp)
    if patch < 1 or S % patch:
        raise L.M324Error(f"vit_patches_f32: the image side {S} is no multiple of the patch {patch}")
    g = S // patch
    img = img.detach().contiguous()
    mean_std = _device_array(mean_std, torch.float32, "vit_patches_f32: mean_std")
    if mean_std.numel() != 6 or mean_std.device != img.device:
        raise L.M324Error("vit_patches_f32: mean_std must be fp32 [6] on the images' device")
    out = _out_like(out, (F_ * g * g, Kp), img.device, "vit_patches_f32")
    _launch("m324_vit_patches_f32", _p(img), F_, S, patch, _p(mean_std), _p(out), Kp)
    _wrote(out)
    return out


# ------------------------------------------------------------------------------------------------ foreground matting
MATTE_SIDES = 6                # M324_MATTE_SIDES
MATTE_MAX_SIDE = 16384          # M324_MATTE_MAX_SIDE
MATTE_CHUNKS = 64               # M324_MATTE_CHUNKS: runs per frame of the two-level per-frame reductions


def upsample_bilinear(x: torch.Tensor, size, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bilinear resize, align_corners=False, of fp32 NHWC [images,H,W,C] to size = (Ho, Wo) (m324_upsample_bilinear; the
    evaluation order is in include/m324.h) -> [images,Ho,Wo,C]"""
    x = _nhwc(x, "upsample_bilinear: x")
    n, H, W, c = x.shape
    Ho, Wo = (int(v) for v in size)
    if not (1 <= Ho <= MATTE_MAX_SIDE and 1 <= Wo <= MATTE_MAX_SIDE and H <= MATTE_MAX_SIDE and W <= MATTE_MAX_SIDE) or n * Ho * Wo >= 2 ** 31:
        raise L.M324Error(f"upsample_bilinear: sizes must be in 1..{MATTE_MAX_SIDE} and images * Ho * Wo below 2^31, got {tuple(x.shape)} -> {(Ho, Wo)}")
    out = _out_like(out, (n, Ho, Wo, c), x.device, "upsample_bilinear")
    _launch("m324_upsample_bilinear", _p(x), _p(out), n, H, W, Ho, Wo, c)
    _wrote(out)
    return out


def matte_prepare(src: torch.Tensor, out: Optional[torch.Tensor] = None, mean=None, std=None) -> torch.Tensor:
    """The matting network's input fp32 [images,H,W,4] (channel 3 is zero) from uint8 [images,H,W,3]: every frame divided by its
    own largest byte, then (. - mean) / std, in float64 rounded once.  mean = std = None: the ImageNet constants
    (m324_matte_prepare); both given, three numbers each, std > 0: m324_matte_prepare_ex."""
    _on_device(src, "matte_prepare")
    if (mean is None) != (std is None):
        raise L.M324Error("matte_prepare: give mean and std together, or neither")
    if mean is not None:
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != 3 or len(std) != 3 or not all(math.isfinite(v) for v in mean) or not all(math.isfinite(v) and v > 0 for v in std):
            raise L.M324Error(f"matte_prepare: mean and std must be three finite numbers each, every std above 0, got {mean} and {std}")
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or 0 in src.shape:
        raise L.M324Error(f"matte_prepare: expected uint8 [images,H,W,3], got {src.dtype} {tuple(src.shape)}")
    n, H, W = src.shape[:3]
    if n * H * W >= 2 ** 31:
        raise L.M324Error(f"matte_prepare: images * H * W must stay below 2^31, got {tuple(src.shape)}")
    src = src.detach().contiguous()
    out = _out_like(out, (n, H, W, 4), src.device, "matte_prepare")
    frame_max = torch.empty((n,), dtype=torch.int32, device=src.device)
    partial = torch.empty((n * MATTE_CHUNKS,), dtype=torch.int32, device=src.device)
    if mean is None:
        _launch("m324_matte_prepare", _p(src), n, H, W, _p(partial), _p(frame_max), _p(out))
    else:
        ms = (C.c_double * 6)(*mean, *std)
        _launch("m324_matte_prepare_ex", _p(src), n, H, W, C.addressof(ms), _p(partial), _p(frame_max), _p(out))
    _wrote(out)
    return out


def matte_side(side: torch.Tensor, size, *, want_logits: bool = False):
    """The one-map head (m324_matte_side): side fp32 NHWC [images,h,w,C] whose channel 0 is the side output.  Returns (prob fp32
    [images,Ho,Wo] = sigmoid(d1), d1 or None) with d1 the bits of upsample_bilinear(side, size)[..., 0], which is not built."""
    side = _nhwc(side, "matte_side: side")
    n, h, w, stride = side.shape
    Ho, Wo = (int(v) for v in size)
    if not (h <= Ho <= MATTE_MAX_SIDE and w <= Wo <= MATTE_MAX_SIDE) or n * Ho * Wo >= 2 ** 31:
        raise L.M324Error(f"matte_side: the output must be no smaller than the side map {(h, w)}, within {MATTE_MAX_SIDE} a side, and images * Ho * Wo "
                          f"below 2^31, got {(n, Ho, Wo)}")
    prob = torch.empty((n, Ho, Wo), dtype=torch.float32, device=side.device)
    logit = torch.empty((n, Ho, Wo), dtype=torch.float32, device=side.device) if want_logits else None
    _launch("m324_matte_side", _p(side), h, w, stride, n, Ho, Wo, _p(prob), _p(logit))
    _wrote(prob, logit)
    return prob, logit


def matte_fuse(sides, weights, bias: float, size, *, want_logits: bool = False):
    """The fused side-output head (m324_matte_fuse): sides six fp32 NHWC maps [images,h_k,w_k,C] whose channel 0 is the side
    output, each at its own resolution; weights six floats and bias, the 1 x 1 `outconv` (host numbers).  Returns (prob fp32
    [images,Ho,Wo] = sigmoid(d0), d0 or None)."""
    if len(sides) != MATTE_SIDES or len(weights) != MATTE_SIDES:
        raise L.M324Error(f"matte_fuse: expected {MATTE_SIDES} side maps and weights, got {len(sides)} and {len(weights)}")
    sides = [_nhwc(s, f"matte_fuse: side {k}") for k, s in enumerate(sides)]
    n, stride, dev = sides[0].shape[0], sides[0].shape[3], sides[0].device
    Ho, Wo = (int(v) for v in size)
    for k, s in enumerate(sides):
        if s.shape[0] != n or s.shape[3] != stride or s.device != dev or s.shape[1] > Ho or s.shape[2] > Wo:
            raise L.M324Error(f"matte_fuse: side {k} {tuple(s.shape)} must have {n} images and {stride} channels on one device and be no "
                              f"larger than the output {(Ho, Wo)}")
    if not (1 <= Ho <= MATTE_MAX_SIDE and 1 <= Wo <= MATTE_MAX_SIDE) or n * Ho * Wo >= 2 ** 31:
        raise L.M324Error(f"matte_fuse: the output must be within {MATTE_MAX_SIDE} a side and images * Ho * Wo below 2^31, got {(n, Ho, Wo)}")
    ptrs = (C.c_void_p * MATTE_SIDES)(*[s.data_ptr() for s in sides])
    hs = (C.c_int * MATTE_SIDES)(*[s.shape[1] for s in sides])
    ws = (C.c_int * MATTE_SIDES)(*[s.shape[2] for s in sides])
    oc = (C.c_float * (MATTE_SIDES + 1))(*[float(w) for w in weights], float(bias))
    prob = torch.empty((n, Ho, Wo), dtype=torch.float32, device=dev)
    logit = torch.empty((n, Ho, Wo), dtype=torch.float32, device=dev) if want_logits else None
    _launch("m324_matte_fuse", C.addressof(ptrs), C.addressof(hs), C.addressof(ws), stride, C.addressof(oc), n, Ho, Wo, _p(prob), _p(logit))
    _wrote(prob, logit)
    return prob, logit


def matte_quantise(prob: torch.Tensor, out: Optional[torch.Tensor] = None):
    """The 8-bit matte of fp32 [images,H,W] probabilities (m324_matte_quantise): per frame (p - min) / (max - min) * 255,
    truncated; a constant frame gives 0.  Returns (uint8 [images,H,W], fp32 [images,2] = the frame's min and max)."""
    prob = _device_array(prob, torch.float32, "matte_quantise: prob")
    if prob.dim() != 3 or 0 in prob.shape or prob.numel() >= 2 ** 31:
        raise L.M324Error(f"matte_quantise: expected fp32 [images,H,W] with fewer than 2^31 values, got {tuple(prob.shape)}")
    n, H, W = prob.shape
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.uint8, device=prob.device)
    elif not _is_device(out) or out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W) or not out.is_contiguous() or out.device != prob.device:
        raise L.M324Error(f"matte_quantise: out must be a contiguous uint8 device tensor {(n, H, W)}")
    minmax = torch.empty((n, 2), dtype=torch.float32, device=prob.device)
    partial = torch.empty((n * MATTE_CHUNKS * 2,), dtype=torch.float32, device=prob.device)
    _launch("m324_matte_quantise", _p(prob), n, H * W, _p(partial), _p(minmax), _p(out))
    _wrote(out, minmax)
    return out, minmax


# ------------------------------------------------------------------------------------------------ training side
def transpose(x: torch.Tensor, rows_pad: Optional[int] = None) -> torch.Tensor:
    """[R, C] -> [C, rows_pad] (rows_pad = round_up(R, 64) by default; the pad columns are zeros)."""
    R, Cc = x.shape
    px, ld = _rows(x, "x")
    rp = (R + 63) // 64 * 64 if rows_pad is None else rows_pad
    out = torch.empty((Cc, rp), dtype=x.dtype, device=x.device)
    _launch("m324_transpose", px, ld, _p(out), rp, R, Cc, rp, code_of(x.dtype))
    return out


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    R, Cc = x.shape
    px, ld = _rows(x, "x")
    if out is None:
        out = torch.empty((Cc,), dtype=torch.float32, device=x.device)
        accumulate = False
    elif COLSUMS.busy(out):                        # queued sums into this destination come first
        COLSUMS.flush()
    scratch, srows = None, 0
    if R >= 256:                                   # two-stage: row chunks in parallel, then a short fixed-order sum
        srows = 256 if R >= 16384 else (64 if R >= 2048 else 16)
        scratch = torch.empty((srows, Cc), dtype=torch.float32, device=x.device)
    _launch("m324_colsum", px, ld, _vec(out, Cc, "out"), R, Cc, code_of(x.dtype), int(accumulate), _p(scratch), srows)
    return out


class _ColsumQueue:
    """Column sums that nobody reads yet, collected and launched together (m324_colsum_multi): the split-K partials of the weight
    gradients, the per-workgroup partials of LayerNorm / RMSNorm weight gradients.  ``defer(src, dst, accumulate)`` = what
    ``colsum(src, out=dst, accumulate=...)`` would do, later.  At the flush the entries are grouped by destination (order kept
    within a destination; destinations are independent of each other): one destination = one chain, summed in order by the same
    threads -- the arithmetic of consecutive m324_colsum calls.  ``flush()`` MUST run before anyone reads or torch-writes a
    destination (backward.GradStore does: done(), add() on a gradient it already holds, get(); colsum(out=...) checks too)."""

    LIMIT = 256

    def __init__(self):
        self.by_dst = {}         # data_ptr of a destination -> [(dst 1-D fp32 view, src 2-D fp32, accumulate)]
        self.count = 0

    def defer(self, src: torch.Tensor, dst: torch.Tensor, accumulate: bool) -> None:
        if src.dtype != torch.float32 or dst.dtype != torch.float32 or src.dim() != 2 or src.stride(1) != 1 or not dst.is_contiguous() \
                or dst.numel() != src.shape[1]:
            raise L.M324Error(f"colsum queue: fp32 [rows, cols] -> contiguous fp32 [cols], got {src.dtype}{tuple(src.shape)} -> {dst.dtype}{tuple(dst.shape)}")
        chain = self.by_dst.setdefault(dst.data_ptr(), [])
        if chain and not accumulate:
            raise L.M324Error("colsum queue: a second sum into a pending destination must accumulate")
        chain.append((dst.view(-1), src, bool(accumulate)))
        self.count += 1
        if self.count >= self.LIMIT:
            self.flush()

    def busy(self, t: torch.Tensor) -> bool:
        return self.count > 0 and t.data_ptr() in self.by_dst

    def clear(self) -> None:
        """Drops the queue (a step that failed half way: its partial buffers are gone)."""
        self.by_dst, self.count = {}, 0

    def flush(self) -> None:
        if not self.count:
            return
        arr = (L.ColsumItem * self.count)()
        k, dsts = 0, []
        # tall sources first: their workgroups (16 waves over up to 1024 rows) are the longest-running of the launch
        for chain in sorted(self.by_dst.values(), key=lambda ch: -max(src.shape[0] for _, src, _a in ch)):
            for j, (dst, src, acc) in enumerate(chain):
                it = arr[k]
                it.dst, it.src, it.ld, it.rows, it.cols = dst.data_ptr(), src.data_ptr(), src.stride(0), src.shape[0], src.shape[1]
                it.accumulate, it.chain = int(acc and j == 0), int(j > 0)
                k += 1
            dsts.append(chain[0][0])
        keep = self.by_dst                                # the sources stay referenced until the launch is enqueued
        self.by_dst, self.count = {}, 0
        _launch("m324_colsum_multi", arr, k)
        _wrote(*dsts)
        del keep


class Rows:
    """Marks an fp32 [rows, cols] tensor whose COLUMN SUMS are a gradient (the per-workgroup partials of a norm-weight gradient):
    backward.GradStore.add queues the sum into the gradient's own memory instead of taking a reduced temporary and copying it."""

    def __init__(self, t: torch.Tensor):
        self.t = t

    def reduce(self) -> torch.Tensor:
        return colsum(self.t)


COLSUMS = _ColsumQueue()
DEFER_COLSUM = switches.flag("M324_DEFER_COLSUM")


def gelu(z: torch.Tensor) -> torch.Tensor:
    assert z.is_contiguous()
    h = torch.empty_like(z)
    _launch("m324_gelu", _p(z), _p(h), z.numel(), code_of(z.dtype))
    return h


def gelu_bwd(z: torch.Tensor, dh: torch.Tensor) -> torch.Tensor:
    assert z.is_contiguous() and dh.is_contiguous() and z.shape == dh.shape and z.dtype == dh.dtype
    dz = torch.empty_like(z)
    _launch("m324_gelu_bwd", _p(z), _p(dh), _p(dz), z.numel(), code_of(z.dtype))
    return dz


def layernorm_bwd(x: torch.Tensor, w: torch.Tensor, eps: float, dy: torch.Tensor, dx: torch.Tensor, accumulate: bool,
                  row_map=(0, 0, 0), cast_out: Optional[torch.Tensor] = None, reduce: bool = True):
    """dx[in_row(r)] (+)= LN backward of row r; returns (dw [C], db [C]) fp32.  x, dx fp32; dy in the compute dtype.
    cast_out (bf16, shaped like dx): also receives the resulting dx rounded to bf16, and a third vector is returned: the
    column sums of that rounded copy (m324_layernorm_bwd_cast: one pass instead of LayerNorm backward + cast + column sum).
    reduce=False: the vectors come back as ops.Rows -- the per-workgroup partial rows, whose column sums the caller queues
    (backward.GradStore.add) instead of reducing them here with a launch each."""
    if x.dtype != torch.float32 or dx.dtype != torch.float32:
        raise L.M324Error("layernorm_bwd: x and dx must be fp32")
    rows, Cdim = dy.shape
    px, ldx = _rows(x, "x")
    pdy, ldy = _rows(dy, "dy")
    pdx, lddx = _rows(dx, "dx")
    _wrote(dx)
    # workgroups of 8 waves, one row per wave at a time; their partial rows are summed by m324_colsum (two stages from 256 rows
    # on) -- or (reduce=False) queued for the block's m324_colsum_multi launch
    n_partial = min(512, (rows + 7) // 8)
    nb = 2 if cast_out is None else 3
    partial = torch.empty((n_partial, nb * Cdim), dtype=torch.float32, device=x.device)
    name, cast_args = "m324_layernorm_bwd", ()
    if cast_out is not None:
        if cast_out.dtype != torch.bfloat16 or cast_out.shape != dx.shape:
            raise L.M324Error("layernorm_bwd: cast_out must be a bf16 tensor shaped like dx")
        name, cast_args = "m324_layernorm_bwd_cast", _rows(cast_out, "cast_out")
        _wrote(cast_out)
    _launch(name, px, ldx, _vec(w, Cdim, "w"), eps, pdy, ldy, code_of(dy.dtype), pdx, lddx, int(accumulate), _p(partial), n_partial,
            rows, Cdim, *row_map, *cast_args)
    if not reduce:
        return tuple(Rows(partial[:, i * Cdim:(i + 1) * Cdim]) for i in range(nb))
    sums = colsum(partial)
    return tuple(sums[i * Cdim:(i + 1) * Cdim] for i in range(nb))


def cast(x: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    R, Cc = x.shape
    px, ld = _rows(x, "x")
    if out is None:
        out = torch.empty((R, Cc), dtype=dtype, device=x.device)
    po, ldo = _rows(out, "out")
    _launch("m324_cast", px, ld, code_of(x.dtype), po, ldo, code_of(out.dtype), R, Cc)
    return out


def attention_delta(O: torch.Tensor, dO: torch.Tensor, B: int, H: int, Lq: int) -> torch.Tensor:
    po, ld = _rows(O, "O")
    pd, ld2 = _rows(dO, "dO")
    if ld != ld2 or O.dtype != dO.dtype:
        raise L.M324Error("attention_delta: O and dO must share layout and dtype")
    D = torch.empty((B, H, Lq), dtype=torch.float32, device=O.device)
    _launch("m324_attention_delta", po, pd, ld, _p(D), B, H, Lq, code_of(O.dtype))
    return D


def attention_bwd(Qs, K, V, dO, lse, D, *, shared_q: bool = False, scale: float = 64 ** -0.5):
    """Head-major operands (see include/m324.h) -> (dQ [B,H,Lq,64] w.r.t. the unscaled normalised q, dK, dV)."""
    B, H, Lk, _ = K.shape
    Lq = Qs.shape[2]
    for t in (Qs, K, V, dO):
        if not t.is_contiguous() or t.dtype != K.dtype:
            raise L.M324Error("attention_bwd: operands must be contiguous and share a dtype")
    dQ = torch.empty((B, H, Lq, 64), dtype=K.dtype, device=K.device)
    dK, dV = torch.empty_like(K), torch.empty_like(V)
    _launch("m324_attention_bwd", _p(Qs), 0 if shared_q else H * Lq * 64, _p(K), _p(V), _p(dO), _p(lse), _p(D), _p(dQ),
            _p(dK), _p(dV), B, H, Lq, Lk, scale, code_of(K.dtype))
    return dQ, dK, dV


def attention_bwd_mfma(spq: dict, spk: dict, spdo: dict, lse, D, *, shared_q: bool = False, scale: float = 64 ** -0.5):
    """bf16 MFMA backward.  spq / spk / spdo: the dicts qkv_split(train=True) returns for q, for k|v and for dO
    (passed as its q source).  Returns (dQ, dK, dV) like attention_bwd."""
    Qs, Qst, K, Kt, V = spq["Q"], spq["Qt"], spk["K"], spk["Kt"], spk["V"]
    dO, dOt = spdo["Q"], spdo["Qt"]
    B, H, Lk, _ = K.shape
    Lq = Qs.shape[2]
    Lqp = (Lq + 63) // 64 * 64
    if K.dtype != torch.bfloat16:
        raise L.M324Error("attention_bwd_mfma is the bf16 kernel; use attention_bwd for fp32")
    dQ = torch.empty((B, H, Lq, 64), dtype=K.dtype, device=K.device)
    dK, dV = torch.empty_like(K), torch.empty_like(V)
    _launch("m324_attention_bwd_mfma", _p(Qs), _p(Qst), 0 if shared_q else H * Lq * 64, 0 if shared_q else H * 64 * Lqp,
            _p(K), _p(Kt), _p(V), _p(dO), _p(dOt), _p(lse), _p(D), _p(dQ), _p(dK), _p(dV), B, H, Lq, Lk, scale)
    return dQ, dK, dV


def qkv_split_bwd(dQ, dK, dV, q_raw, k_raw, q_w, k_w, eps: float, B: int, Lq: int, H: int, dq_out, dk_out, dv_out, reduce: bool = True):
    """Writes token-major gradients into dq_out / dk_out / dv_out (2-D views, any may be None with its dX);
    returns (dq_norm_w [64] or None, dk_norm_w [64] or None)."""
    dtype = next(t for t in (dQ, dK, dV) if t is not None).dtype
    n_partial = min(1024, max(1, (B * Lq * H + 31) // 32))      # a workgroup takes 32 (token, head) rows per pass
    dev = next(t for t in (dQ, dK, dV) if t is not None).device
    partial = torch.empty((n_partial, 128), dtype=torch.float32, device=dev)

    def rw(t):
        return _rows(t, "view") if t is not None else (None, 0)
    pq, ldq = rw(q_raw)
    pk, ldk = rw(k_raw)
    poq, ldoq = rw(dq_out)
    pok, ldok = rw(dk_out)
    pov, ldov = rw(dv_out)
    _launch("m324_qkv_split_bwd", _p(dQ), _p(dK), _p(dV), pq, ldq, pk, ldk, _vec(q_w, 64, "q_w"), _vec(k_w, 64, "k_w"),
            eps, poq, ldoq, pok, ldok, pov, ldov, _p(partial), n_partial, B, Lq, H, code_of(dtype))
    if not reduce:                                          # ops.Rows: see layernorm_bwd
        return (Rows(partial[:, :64]) if (dQ is not None and q_w is not None) else None,
                Rows(partial[:, 64:]) if (dK is not None and k_w is not None) else None)
    both = colsum(partial)
    return (both[:64] if (dQ is not None and q_w is not None) else None,
            both[64:] if (dK is not None and k_w is not None) else None)


def linear_n3_bwd(a: torch.Tensor, w: torch.Tensor, dout: torch.Tensor, mul_by: Optional[torch.Tensor] = None):
    """Backward of linear_n3: returns (dA [M,K] in a.dtype, dW [3,K] fp32, db [3] fp32).  mul_by [M, K] (a's dtype): dA is multiplied by it
    (the gelu'(z) the Linear in front left with gemm(gelu_grad_out=...): dA is then the gradient of ITS pre-activation)."""
    M, K = a.shape
    pa, lda = _rows(a, "a")
    dout = dout.reshape(M, 3)
    if dout.dtype != torch.float32 or not dout.is_contiguous():
        raise L.M324Error("linear_n3_bwd: dout must be contiguous fp32 [M,3]")
    pm, ldm = (None, 0)
    if mul_by is not None:
        if mul_by.dtype != a.dtype or mul_by.shape[0] < M or mul_by.shape[1] < K:
            raise L.M324Error(f"linear_n3_bwd: mul_by {mul_by.dtype}{tuple(mul_by.shape)} does not match a {a.dtype}[{M}, {K}]")
        pm, ldm = _rows(mul_by, "mul_by")
    dA = torch.empty((M, K), dtype=a.dtype, device=a.device)
    n_partial = min(1024, M)
    partial = torch.empty((n_partial, 3 * K), dtype=torch.float32, device=a.device)
    _launch("m324_linear_n3_bwd", pa, lda, _p(w), _p(dout), _p(dA), K, _p(partial), n_partial, M, K, code_of(a.dtype), pm, ldm)
    return dA, colsum(partial).reshape(3, K), colsum(dout)


def mse_bwd(pred: torch.Tensor, target: torch.Tensor, weight: float, grad_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    pred, target = pred.contiguous().float(), target.contiguous().float()
    d = torch.empty_like(pred)
    _launch("m324_mse_bwd", _p(pred), _p(target), _p(grad_scale), 2.0 * weight / pred.numel(), _p(d), pred.numel())
    return d


def adamw_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, beta1: float, beta2: float,
               eps: float, weight_decay: float, step: int, grad_scale: Optional[torch.Tensor] = None) -> None:
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise L.M324Error("adamw_step: tensors must be contiguous fp32 of equal size")
    _launch("m324_adamw", _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step, _p(grad_scale))


def adamw_flat(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, n_decay: int, lr: float, beta1: float,
               beta2: float, eps: float, weight_decay: float, step: int, grad_scale: Optional[torch.Tensor] = None) -> None:
    """One launch over the optimizer's flat buffers: elements [0, n_decay) decay, the rest do not (m324_adamw_flat)."""
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise L.M324Error("adamw_flat: tensors must be contiguous fp32 of equal size")
    _launch("m324_adamw_flat", _p(p), _p(g), _p(m), _p(v), p.numel(), int(n_decay), lr, beta1, beta2, eps, weight_decay, step, _p(grad_scale))


def weight_mirror(src: torch.Tensor, dst: torch.Tensor, dstT: Optional[torch.Tensor], table: torch.Tensor, n_items: int, n_tiles: int) -> None:
    """bf16 row-major and transposed copies of the Linear weights inside a flat fp32 parameter buffer, one launch
    (m324_weight_mirror; table: the items as a device byte tensor, see lib.MirrorItem)."""
    if src.dtype != torch.float32 or dst.dtype != torch.bfloat16 or (dstT is not None and dstT.dtype != torch.bfloat16) or table.dtype != torch.uint8 \
            or table.numel() != n_items * C.sizeof(L.MirrorItem) or not table.is_cuda:
        raise L.M324Error("weight_mirror: fp32 source, bf16 copies and a device table of lib.MirrorItem records")
    _launch("m324_weight_mirror", _p(src), _p(dst), _p(dstT), _p(table), n_items, n_tiles)


def grad_sumsq(g: torch.Tensor, out: torch.Tensor, partial: torch.Tensor, sanitize: bool, accumulate: bool) -> None:
    _launch("m324_grad_sumsq", _p(g), g.numel(), int(sanitize), _p(partial), _p(out), int(accumulate))
