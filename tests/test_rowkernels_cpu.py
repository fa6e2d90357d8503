"""The row, reduction and layout kernels without a device: every entry point refuses what include/m324.h forbids before any HIP
call (fake pointers, as tests/test_rows_cpu.py does: a call that reached a launch would come back as M324_ERR_HIP here, not as the
status asserted), and the case module's own conditions hold (tests/rowkernel_cases.py)."""
import pytest

import error_bounds as eb
import rowkernel_cases as rc
from motion324_amd import lib

INVALID, UNSUPPORTED = -1, -3
P = 4096                                  # a 16-byte aligned address that is never dereferenced


def _refused(rc_, name, status=INVALID):
    assert rc_ == status, (name, rc_, lib.last_error())
    assert name in lib.last_error(), (name, lib.last_error())


def _ln(h, C=256, ldx=None, ldy=None, rows=9):
    return h.m324_layernorm(P, C if ldx is None else ldx, P, None, 1e-5, P, C if ldy is None else ldy, lib.F32, rows, C, 0, 0, 0, None)


def _ln_in(h, C=256, ldx=None, ldy=None, out=lib.BF16):
    return h.m324_layernorm_in(P, lib.BF16, C if ldx is None else ldx, P, None, 1e-5, P, C if ldy is None else ldy, out, 9, C, 0, 0, 0, None)


def _ln_pair(h, C=256, ld=None):
    ld = C if ld is None else ld
    return h.m324_layernorm_pair(P, C, P, None, 1e-5, P, C, 9, 0, 0, 0, P, ld, P, None, 1e-5, P, C, 7, 3, 7, 2, C, lib.F32, None)


def _rowstats(h, C=256, ldx=None, ldcopy=None):
    return h.m324_rowstats(P, C if ldx is None else ldx, 9, C, 1e-5, P, P, C if ldcopy is None else ldcopy, None)


def _ln_bwd(h, C=256, n_partial=2, ld=None):
    return h.m324_layernorm_bwd(P, C if ld is None else ld, P, 1e-5, P, C, lib.F32, P, C, 0, P, n_partial, 9, C, 0, 0, 0, None)


def _ln_bwd_cast(h, C=256, n_partial=2, ldc=None):
    return h.m324_layernorm_bwd_cast(P, C, P, 1e-5, P, C, lib.F32, P, C, 0, P, n_partial, 9, C, 0, 0, 0, P, C if ldc is None else ldc, None)


LN_FAMILY = (("m324_layernorm", _ln), ("m324_layernorm_in", _ln_in), ("m324_layernorm_pair", _ln_pair), ("m324_rowstats", _rowstats),
             ("m324_layernorm_bwd", _ln_bwd), ("m324_layernorm_bwd_cast", _ln_bwd_cast))


@pytest.mark.parametrize("name,call", LN_FAMILY)
@pytest.mark.parametrize("C", [0, 6, 1028])
def test_layernorm_family_refuses_widths_outside_the_documented_range(name, call, C):
    """C % 4 == 0, 0 < C <= 1024; the leading dimensions stay multiples of 4 so that the width is what is refused"""
    h = lib.load()
    ld = 1028 if C != 6 else 8
    if call in (_ln, _ln_in):
        _refused(call(h, C=C, ldx=ld, ldy=ld), name)
    elif call is _rowstats:
        _refused(call(h, C=C, ldx=ld, ldcopy=ld), name)
    else:
        _refused(call(h, C=C), name)


def test_layernorm_family_refuses_leading_dimensions_that_are_no_multiples_of_4():
    h = lib.load()
    _refused(_ln(h, ldx=258), "m324_layernorm")
    _refused(_ln(h, ldy=262), "m324_layernorm")
    _refused(_ln_in(h, ldx=258), "m324_layernorm_in")
    _refused(_ln_in(h, ldy=262), "m324_layernorm_in")
    _refused(_ln_pair(h, ld=258), "m324_layernorm_pair")
    _refused(_rowstats(h, ldx=258), "m324_rowstats")
    _refused(_rowstats(h, ldx=252), "m324_rowstats")                 # a multiple of 4 below C
    _refused(_rowstats(h, ldcopy=258), "m324_rowstats")
    _refused(_ln_bwd(h, ld=258), "m324_layernorm_bwd")
    _refused(_ln_bwd_cast(h, ldc=258), "m324_layernorm_bwd_cast")
    _refused(_ln(h, rows=0), "m324_layernorm")


def test_bf16_input_needs_a_bf16_output():
    _refused(_ln_in(lib.load(), out=lib.F32), "m324_layernorm_in")


@pytest.mark.parametrize("n_partial", [0, 4097])
def test_layernorm_backward_refuses_workgroup_counts_outside_1_to_4096(n_partial):
    h = lib.load()
    _refused(_ln_bwd(h, n_partial=n_partial), "m324_layernorm_bwd")
    _refused(_ln_bwd_cast(h, n_partial=n_partial), "m324_layernorm_bwd_cast")


def _split(h, q=P, k=None, v=None, ldq=64, Q=P, Qt=None, K=None, Kt=None, V=None, Vt=None, dtype=lib.BF16):
    return h.m324_qkv_split(q, ldq, k, 64, v, 64, None, None, 1e-5, 1.0, Q, K, V, Qt, Kt, Vt, 1, 1, 1, dtype, None)


def _split_bwd(h, n_partial=1, ldq=64, ldoq=64, ldov=64):
    return h.m324_qkv_split_bwd(P, None, P, P, ldq, None, 64, P, None, 1e-5, P, ldoq, None, 64, P, ldov, P, n_partial, 1, 1, 1, lib.BF16, None)


def test_qkv_split_refuses_a_source_without_output_and_ragged_leading_dimensions():
    h = lib.load()
    _refused(_split(h, Q=None), "m324_qkv_split")                    # q source, neither Q nor Qt
    _refused(_split(h, k=P), "m324_qkv_split")                       # k source, neither K nor Kt
    _refused(_split(h, v=P), "m324_qkv_split")
    _refused(_split(h, ldq=68), "m324_qkv_split")                    # bf16: multiples of 8
    _refused(_split(h, ldq=66, dtype=lib.F32), "m324_qkv_split")     # fp32: multiples of 4
    for n_partial in (0, 2049):
        _refused(_split_bwd(h, n_partial=n_partial), "m324_qkv_split_bwd")
    _refused(_split_bwd(h, ldq=68), "m324_qkv_split_bwd")            # the header says 8 for either dtype
    _refused(_split_bwd(h, ldoq=68), "m324_qkv_split_bwd")
    _refused(_split_bwd(h, ldov=68), "m324_qkv_split_bwd")


def test_layout_kernels_refuse_a_leading_dimension_below_the_width():
    h = lib.load()
    _refused(h.m324_colsum(P, 63, P, 5, 64, lib.F32, 0, None, 0, None), "m324_colsum")
    _refused(h.m324_cast(P, 63, lib.F32, P, 64, lib.BF16, 1, 64, None), "m324_cast")
    _refused(h.m324_cast(P, 64, lib.F32, P, 63, lib.BF16, 1, 64, None), "m324_cast")
    _refused(h.m324_transpose(P, 63, P, 64, 5, 64, 64, lib.F32, None), "m324_transpose")
    _refused(h.m324_transpose(P, 64, P, 63, 5, 64, 64, lib.F32, None), "m324_transpose")       # ld_out < rows_pad


def test_attention_delta_refuses_short_and_ragged_leading_dimensions():
    h = lib.load()
    _refused(h.m324_attention_delta(P, P, 120, P, 1, 2, 5, lib.BF16, None), "m324_attention_delta")      # ld < H * 64
    _refused(h.m324_attention_delta(P, P, 132, P, 1, 2, 5, lib.BF16, None), "m324_attention_delta")      # ld % 8 != 0


# ------------------------------------------------------------------------------------------- the case module's own conditions
@pytest.mark.parametrize("C", rc.LN_WIDTHS)
def test_offset_row_bound_stays_below_a_64th_of_the_row_rms(C):
    """eb.layernorm is sound on a row whose mean dwarfs its deviation but grows with C |mean|: the offset per width is chosen so
    that the check of that row still tests something (at +1000 and C = 1000 the bound would allow 0.24 on outputs of order 1)"""
    assert rc.offset_row_condition(C) < 1.0


def test_case_tables_name_the_kernel_the_entry_point_selects():
    for (rows, cols, ld, voff), kernel in rc.COLSUM_CASES:
        got, depth = eb.colsum_plan(rows, cols, ld, aligned16=(voff == 0), scratch_rows=rc.colsum_scratch_rows(rows))
        assert got == kernel, ((rows, cols, ld, voff), got)
        assert 0 < depth <= rows
    kernels = {k for _c, k in rc.COLSUM_CASES}
    assert kernels == {"colsum_wide4", "colsum_wide", "colsum", "colsum_chunk4 + colsum_wide4", "colsum_chunk + colsum_wide"}
    for rows in rc.LN_ROWS[1:]:
        sp = rc.special_row_index(rows)
        assert sorted(sp) == sorted(rc.SPECIAL_ROWS) and sp["offset"] == rows - 1 and rows % 2 == 1     # the lone last row
    assert int(rc.mapped_rows(rc.ROW_MAP_ROWS, rc.ROW_MAP)[-1]) == 18 and rc.stream_rows(rc.ROW_MAP_ROWS, rc.ROW_MAP) == 21
    for B, L, H in rc.QKV_SHAPES[:3]:
        assert (B * L * H) % 8 != 0                                    # the backward's clamped lanes run
    assert all((B * L * H) % 32 != 0 for B, L, H in rc.QKV_SHAPES)
