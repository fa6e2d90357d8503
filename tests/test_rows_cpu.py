"""m324_attention_rows / m324_gemm_rows without a device: argument validation happens before any HIP call, the ABI number is the
one the suite pins (the two entry points are additions), and the plan queries of the existing entry points answer as before
(tests/test_plans_cpu.py holds the whole table; the ten shapes here are the launches the last per-frame block is made of)."""
import ctypes

from motion324_amd import lib

INVALID, UNSUPPORTED = -1, -3


def test_abi_version_is_still_23():
    assert lib.load().m324_abi_version() == 23 == lib.ABI_VERSION


def test_query_window_is_validated_before_any_launch():
    h = lib.load()

    def call(q_rows, Lq=324, dtype=lib.BF16, Q=16, flags=3):
        return h.m324_attention_rows(Q, 2 * Lq * 64, 16, 16, 16, 128, 2, 2, Lq, Lq, 0.125, flags, None, dtype, q_rows, None)
    assert call(0) == INVALID and "q_rows=0" in lib.last_error()
    assert call(-32) == INVALID
    assert call(48) == UNSUPPORTED and "multiple of 32" in lib.last_error()
    assert call(100) == UNSUPPORTED
    assert call(96, Q=None) == INVALID and "null" in lib.last_error()
    assert call(96, dtype=lib.F32, flags=1) == UNSUPPORTED and "no query window" in lib.last_error()        # the fp32 kernel
    # the hand-placed long-sequence stream
    assert h.m324_attention_rows(16, 2048 * 64, 16, 16, 16, 64, 1, 1, 2048, 512, 0.125, 1, None, lib.BF16, 96, None) == UNSUPPORTED
    assert call(96, dtype=7, flags=1) == UNSUPPORTED                                                                 # as m324_attention


def _producer(M=192, N=768, K=768):
    a = lib.GemmArgs()
    a.A = a.W = a.C = 4096
    a.residual, a.ldr = 8192, N
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    a.in_dtype, a.out_dtype, a.batch = lib.BF16, lib.F32, 1
    a.ln_stats_out, a.ln_copy_out, a.ln_ldcopy = 4096, 4096, N
    return a


def test_input_row_map_is_validated_before_any_launch():
    h = lib.load()
    assert h.m324_gemm_rows(None, 64, 100, 4, None) == INVALID and "null" in lib.last_error()
    a = _producer()
    for gin, gout, off in ((0, 100, 4), (64, 32, 0), (64, 100, -1), (64, 100, 40), (50, 100, 4)):      # 50: 192 rows are no whole groups
        assert h.m324_gemm_rows(ctypes.byref(a), gin, gout, off, None) == INVALID, (gin, gout, off)
        assert "m324_gemm_rows" in lib.last_error()
    # combinations that are not built: in place, no statistics, a bf16 stream, a GELU
    b = _producer()
    b.residual = b.C
    assert h.m324_gemm_rows(ctypes.byref(b), 64, 100, 4, None) == UNSUPPORTED
    b = _producer()
    b.ln_stats_out = b.ln_copy_out = None
    assert h.m324_gemm_rows(ctypes.byref(b), 64, 100, 4, None) == UNSUPPORTED
    b = _producer()
    b.out_dtype, b.ln_copy_out = lib.BF16, None
    assert h.m324_gemm_rows(ctypes.byref(b), 64, 100, 4, None) == UNSUPPORTED
    b = _producer()
    b.ln_stats_out = b.ln_copy_out = None
    b.act = lib.ACT_GELU
    assert h.m324_gemm_rows(ctypes.byref(b), 64, 100, 4, None) == UNSUPPORTED
    # m324_gemm's own validation comes first
    b = _producer(K=40)
    b.lda = b.ldw = 40
    assert h.m324_gemm_rows(ctypes.byref(b), 64, 100, 4, None) == INVALID and "K=40" in lib.last_error()


# (M, N, K, out dtype, act, residual, statistics producer, k|v heads, folded consumer) -> (schedule, kernel and grid)
GEMM_PLANS = [
    ((10368, 768, 768, 0, 0, True, True, False, False), (13, 'gemm_ring2_kernel<float, 48, 1> grid=124416x1x1')),
    ((10368, 768, 3072, 0, 0, True, False, False, False), (12, 'gemm_ring3_kernel<float, 0, 1> grid=62976x1x1')),
    ((2048, 768, 768, 0, 0, True, True, False, False), (13, 'gemm_ring2_kernel<float, 48, 1> grid=24576x1x1')),
    ((2048, 3072, 768, 1, 1, False, False, False, True), (13, 'gemm_ring2_kernel<unsigned short, 9, 0> grid=98304x1x1')),
    ((2048, 768, 3072, 0, 0, True, False, False, False), (13, 'gemm_ring2_kernel<float, 0, 1> grid=24576x1x1')),
    ((2048, 1536, 768, 1, 0, False, False, True, False), (13, 'gemm_ring2_kernel<unsigned short, 4, 0> grid=49152x1x1')),
]
# (B, H, Lq, Lk, flags) -> (waves, kernel and grid)
ATTN_PLANS = [
    ((32, 12, 324, 324, 3), (4, 'attn_bf16_kernel<true, 1, 4, true, 2> grid=294912x1x1')),
    ((32, 12, 257, 257, 3), (4, 'attn_bf16_kernel<true, 1, 4, true, 2> grid=294912x1x1')),
    ((1, 12, 10368, 10368, 5), (4, 'attn_pwg_bounded_kernel grid=125952x1x1')),
    ((2, 2, 160, 160, 3), (4, 'attn_bf16_kernel<true, 1, 4, true, 2> grid=512x2x2')),
]


def _gemm_plan(M, N, K, out_dt, act, residual, stats, heads, ln):
    a = lib.GemmArgs()
    a.A = a.W = a.C = 4096
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    a.in_dtype, a.out_dtype, a.act, a.batch, a.bias = lib.BF16, out_dt, act, 1, 4096
    if residual:
        a.residual, a.ldr = 4096, N
    if stats:
        a.ln_stats_out = 4096
        if out_dt == lib.F32:
            a.ln_copy_out, a.ln_ldcopy = 4096, N
    if ln:
        a.ln_rowstat, a.ln_colsum, a.ln_ncb, a.ln_eps = 4096, 4096, K // 64, 1e-5
    if heads:
        a.C, a.aux_mode, a.qkv_L, a.qkv_H = None, 4, 64, N // 128
        a.qkv_k = a.qkv_v = 4096
    buf = ctypes.create_string_buffer(192)
    v = lib.load().m324_gemm_plan(ctypes.byref(a), buf, 192)
    return (v, buf.value.decode())


def test_existing_plan_queries_answer_as_before():
    """The window and the row map are arguments of new entry points: what m324_gemm and m324_attention launch for a shape did not
    move (recorded from the library before the entry points were added; none of the ten depends on the compute-unit count)."""
    h = lib.load()
    for case, want in GEMM_PLANS:
        assert _gemm_plan(*case) == want, case
    for case, want in ATTN_PLANS:
        buf = ctypes.create_string_buffer(192)
        v = h.m324_attention_plan(*case, lib.BF16, buf, 192)
        assert (v, buf.value.decode()) == want, case
