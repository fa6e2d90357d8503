"""The small HBM-bound kernels between the GEMMs (motion324_amd/csrc/elementwise.hip, backward.hip) over their documented range:
the LayerNorm family, the row statistics of the LayerNorm fold, the q|k|v split and its backward, m324_attention_delta,
m324_attention_merge, the column sums, GELU and cast -- at the widths, row counts and dispatch forms of tests/rowkernel_cases.py.

Ground rules of every test: the reference is an fp64 torch statement of the operation on the CPU from the values the kernel reads;
every element goes through error_bounds.assert_within (torch.equal where the code or the header promises identical bits); every
output buffer is NaN-filled with at least 8 guard rows behind the last row the kernel may write (for row-mapped outputs the
unmapped rows in between are guards too), the guards must still be NaN afterwards and no written element may be.  No launching
call receives a shape or pointer the header forbids.  `pytest -s` prints the worst err / bound per family (a record, not a gate)."""
import json
import math
import os

import pytest
import torch

import error_bounds as eb
import rowkernel_cases as rc
from conftest import vt_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _print_record():
    yield
    for k in sorted(RECORD):
        print(f"\nworst err / bound  {k:40s} {RECORD[k]:.3f}", end="")
    path = os.environ.get("M324_ROWKERNEL_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)


def _rec(family, ratio):
    RECORD[family] = max(RECORD.get(family, 0.0), float(ratio))


def _lib():
    from motion324_amd import lib
    return lib


def _ops():
    from motion324_amd import ops
    return ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(dtype):
    return _lib().BF16 if dtype == BF else _lib().F32


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(rows, cols, dtype=F32, guard=rc.GUARD):
    return torch.full((rows + guard, cols), NAN, dtype=dtype, device=DEV)


def _all_nan(t):
    return bool(torch.isnan(t.float()).all())


def _guards_untouched(buf, rows, what, cols=None):
    assert _all_nan(buf[rows:]), f"{what}: rows behind the last output row were written"
    if cols is not None and cols < buf.shape[1]:
        assert _all_nan(buf[:, cols:]), f"{what}: columns behind the row's width were written"


def _check(rc_, what):
    _lib().check(rc_, what)


# ------------------------------------------------------------------------------------------- 1. LayerNorm forward
def _layernorm(x, w, b, eps, rows, C, odt, row_map=(0, 0, 0), via_in=False):
    h, y = _lib().load(), _nan(rows, C, odt)
    if x.dtype == BF or via_in:
        _check(h.m324_layernorm_in(_p(x), _code(x.dtype), x.stride(0), _p(w), _p(b), eps, _p(y), y.stride(0), _code(odt), rows, C,
                                   *row_map, _stream()), "m324_layernorm_in")
    else:
        _check(h.m324_layernorm(_p(x), x.stride(0), _p(w), _p(b), eps, _p(y), y.stride(0), _code(odt), rows, C, *row_map, _stream()),
               "m324_layernorm")
    return y


def _ln_stream(rows, C, xdt, row_map):
    """(compact rows the call normalises, the stream it reads them from)"""
    xin = rc.ln_input(rows, C, dtype=xdt)
    if row_map[0] <= 0:
        return xin, xin
    stream = rc.rand((rc.stream_rows(rows, row_map), C), 4000 + C).to(xdt)
    stream[rc.mapped_rows(rows, row_map)] = xin
    return xin, stream


@pytest.mark.parametrize("C", rc.LN_WIDTHS)
def test_layernorm_every_width_row_count_and_form(tune, C):
    """m324_layernorm and m324_layernorm_in (bf16 input): the full cross of width and row count, output dtype / bias / eps pairwise,
    both M324_LN_ROWS forms bit-identical (the comment above layernorm1_kernel promises it), the row map (3, 7, 2) with 9 rows (the
    lone last row is a mapped row), the special rows inside every input."""
    w, b = rc.ln_params(C)
    wd, bd = w.to(DEV), b.to(DEV)
    cases = [(rows, (0, 0, 0)) for rows in rc.LN_ROWS] + [(rc.ROW_MAP_ROWS, rc.ROW_MAP)]
    for rows, row_map in cases:
        for xdt in (F32, BF):
            xin, stream = _ln_stream(rows, C, xdt, row_map)
            sd = stream.to(DEV)
            variants = rc.LN_VARIANTS if xdt == F32 else [(BF, bias, eps) for bias, eps in rc.LN_IN_VARIANTS]
            for odt, bias, eps in variants:
                what = f"layernorm C={C} rows={rows} map={row_map} x={xdt} out={odt} bias={bias} eps={eps}"
                outs = []
                for form in (2, 1):
                    tune("M324_LN_ROWS", form)
                    outs.append(_layernorm(sd, wd, bd if bias else None, eps, rows, C, odt, row_map))
                torch.cuda.synchronize()
                assert torch.equal(outs[0][:rows], outs[1][:rows]), what + ": the two M324_LN_ROWS forms differ"
                ref = rc.ln_reference(xin.float(), w, b if bias else None, eps)
                bound = eb.layernorm(xin.float(), w, b if bias else None, eps, out_dtype=odt)
                for y in outs:
                    _guards_untouched(y, rows, what)
                _rec(f"layernorm {'bf16' if xdt == BF else 'fp32'} in, {'bf16' if odt == BF else 'fp32'} out",
                     eb.assert_within(outs[0][:rows], ref, bound, what))
            if xdt == F32:                                  # m324_layernorm_in with an fp32 input is m324_layernorm
                tune("M324_LN_ROWS", 2)
                y = _layernorm(sd, wd, bd, 1e-5, rows, C, F32, row_map, via_in=True)
                assert torch.equal(y[:rows], _layernorm(sd, wd, bd, 1e-5, rows, C, F32, row_map)[:rows])


@pytest.mark.parametrize("C", [260, 1024])
def test_layernorm_pair_equals_the_two_separate_launches(C):
    """m324_layernorm_pair: problem 1 row-mapped; bit-identical to m324_layernorm twice (whose fp64 comparison is the test above)"""
    h = _lib().load()
    (w0, b0), (w1, b1) = rc.ln_params(C), rc.ln_params(C, seed=1)
    w0, b0, w1, b1 = (t.to(DEV) for t in (w0, b0, w1, b1))
    for rows0 in (1, 9):
        for rows1 in (7, 16):
            for odt in (F32, BF):
                x0 = rc.ln_input(rows0, C).to(DEV)
                _, s1 = _ln_stream(rows1, C, F32, rc.ROW_MAP)
                x1 = s1.to(DEV)
                y0, y1 = _nan(rows0, C, odt), _nan(rows1, C, odt)
                _check(h.m324_layernorm_pair(_p(x0), C, _p(w0), _p(b0), 1e-5, _p(y0), C, rows0, 0, 0, 0, _p(x1), C, _p(w1), None, 1e-6,
                                             _p(y1), C, rows1, *rc.ROW_MAP, C, _code(odt), _stream()), "m324_layernorm_pair")
                z0 = _layernorm(x0, w0, b0, 1e-5, rows0, C, odt)
                z1 = _layernorm(x1, w1, None, 1e-6, rows1, C, odt, rc.ROW_MAP)
                torch.cuda.synchronize()
                what = f"layernorm_pair C={C} rows={rows0}+{rows1} {odt}"
                _guards_untouched(y0, rows0, what), _guards_untouched(y1, rows1, what)
                assert not bool(torch.isnan(y0[:rows0].float()).any()) and not bool(torch.isnan(y1[:rows1].float()).any()), what
                assert torch.equal(y0[:rows0], z0[:rows0]) and torch.equal(y1[:rows1], z1[:rows1]), what


# ------------------------------------------------------------------------------------------- 2. row statistics
@pytest.mark.parametrize("C", rc.LN_WIDTHS)
def test_rowstats_every_width_and_row_count(C):
    h = _lib().load()
    for rows in rc.LN_ROWS:
        x = rc.ln_input(rows, C)
        xd = x.to(DEV)
        for eps in (1e-5, 1e-6):
            for with_copy in (False, True):
                st = _nan(rows, 2)
                copy = _nan(rows, C + 4, BF) if with_copy else None
                _check(h.m324_rowstats(_p(xd), C, rows, C, eps, _p(st), _p(copy), C + 4 if with_copy else 0, _stream()), "m324_rowstats")
                torch.cuda.synchronize()
                what = f"rowstats C={C} rows={rows} eps={eps} copy={with_copy}"
                _guards_untouched(st, rows, what)
                ref, bnd = rc.rowstats_reference(x, eps), eb.rowstats(x, eps)
                _rec("rowstats rstd", eb.assert_within(st[:rows, 0], ref[0], bnd[0], what + " rstd"))
                _rec("rowstats -rstd mean", eb.assert_within(st[:rows, 1], ref[1], bnd[1], what + " -rstd mean"))
                if with_copy:
                    _guards_untouched(copy, rows, what, cols=C)
                    assert torch.equal(copy[:rows, :C].cpu(), x.to(BF)), what + ": the bf16 copy"


@pytest.mark.parametrize("ncb", rc.FINISH_NCB)
def test_rowstats_finish_every_block_count(ncb):
    h = _lib().load()
    for M in rc.FINISH_M:
        part = rc.finish_table(ncb, M)
        pd = part.to(DEV)
        for eps in (1e-5, 1e-6):
            st = _nan(M, 2)
            _check(h.m324_rowstats_finish(_p(pd), ncb, M, eps, _p(st), _stream()), "m324_rowstats_finish")
            torch.cuda.synchronize()
            what = f"rowstats_finish ncb={ncb} M={M} eps={eps}"
            _guards_untouched(st, M, what)
            ref, bnd = eb.rowstats_finish_reference(part, eps), eb.rowstats_finish(part, eps)
            _rec("rowstats_finish rstd", eb.assert_within(st[:M, 0], ref[0], bnd[0], what + " rstd"))
            _rec("rowstats_finish -rstd mean", eb.assert_within(st[:M, 1], ref[1], bnd[1], what + " -rstd mean"))


# ------------------------------------------------------------------------------------------- 3. LayerNorm backward
def _bwd_case(rows, C, dt, accumulate, row_map):
    xin, stream = _ln_stream(rows, C, F32, row_map)
    S = stream.shape[0]
    dy = rc.rand((rows, C), 70 + C + rows).to(dt)
    idx = rc.mapped_rows(rows, row_map)
    addend = rc.rand((rows, C), 71 + C + rows) if accumulate else None
    dx0 = torch.full((S + rc.GUARD, C), NAN)
    if accumulate:
        dx0[idx] = addend
    return xin, stream, dy, idx, addend, dx0


def _check_bwd(what, xin, w, dy, idx, addend, dx, dw, db, S):
    ref = eb.layernorm_backward_reference(xin, w, 1e-5, dy.float(), addend)
    bnd = eb.layernorm_backward(xin, w, 1e-5, dy.float(), addend)
    dxc = dx.cpu()
    untouched = torch.ones(dxc.shape[0], dtype=torch.bool)
    untouched[idx] = False
    assert _all_nan(dxc[untouched]), what + ": dx rows that no input row maps to (or guard rows) were written"
    _rec("layernorm_bwd dx", eb.assert_within(dxc[idx], ref[0], bnd[0], what + " dx"))
    _rec("layernorm_bwd dw", eb.assert_within(dw, ref[1], bnd[1], what + " dw"))
    _rec("layernorm_bwd db", eb.assert_within(db, ref[2], bnd[2], what + " db"))


def _check_cast(what, plain, cast, idx, rows, n_partial, C):
    dx, dw, db = plain
    dx2, dw2, db2, copy, third = cast
    assert torch.equal(dx.cpu()[idx], dx2.cpu()[idx]), what + ": dx of the cast form"
    assert torch.equal(dw, dw2) and torch.equal(db, db2), what + ": dw / db of the cast form"
    cc, dxc = copy.cpu(), dx2.cpu()
    untouched = torch.ones(cc.shape[0], dtype=torch.bool)
    untouched[idx] = False
    assert _all_nan(cc[untouched]), what + ": untouched rows of the bf16 copy"
    assert torch.equal(cc[idx], dxc[idx].to(BF)), what + ": the bf16 copy"
    # third vector: column sums of the rounded copy -- a wave's rows, the eight waves through LDS, then m324_colsum over the partial rows
    depth = -(-rows // (8 * n_partial)) + 7 + eb.colsum_plan(n_partial, 3 * C, 3 * C, True, rc.colsum_scratch_rows(n_partial))[1]
    _rec("layernorm_bwd_cast column sums", eb.assert_within(third, cc[idx].double().sum(0), eb.colsum(cc[idx], depth), what + " third vector"))


@pytest.mark.parametrize("C", rc.BWD_WIDTHS)
def test_layernorm_backward_every_width(C):
    """m324_layernorm_bwd and _bwd_cast through ops.layernorm_bwd (the product's n_partial): C = 1024 asks for 64 KiB of dynamic
    LDS; rows 1 / 9 / 70, dy fp32 / bf16, accumulate, the row map (3, 7, 2)"""
    ops = _ops()
    w, _ = rc.ln_params(C)
    wd = w.to(DEV)
    for rows in rc.BWD_ROWS:
        for dt in (F32, BF):
            for accumulate in (False, True):
                for row_map in ((0, 0, 0), rc.ROW_MAP):
                    xin, stream, dy, idx, addend, dx0 = _bwd_case(rows, C, dt, accumulate, row_map)
                    S = stream.shape[0]
                    what = f"layernorm_bwd C={C} rows={rows} dy={dt} accumulate={accumulate} map={row_map}"
                    xd, dyd = torch.cat([stream, torch.zeros(rc.GUARD, C)]).to(DEV), dy.to(DEV)
                    dx = dx0.clone().to(DEV)
                    dw, db = ops.layernorm_bwd(xd, wd, 1e-5, dyd, dx, accumulate, row_map=row_map)
                    dx2, copy = dx0.clone().to(DEV), torch.full((S + rc.GUARD, C), NAN, dtype=BF, device=DEV)
                    dw2, db2, third = ops.layernorm_bwd(xd, wd, 1e-5, dyd, dx2, accumulate, row_map=row_map, cast_out=copy)
                    torch.cuda.synchronize()
                    _check_bwd(what, xin, w, dy, idx, addend, dx, dw, db, S)
                    _check_cast(what, (dx, dw, db), (dx2, dw2, db2, copy, third), idx, rows, min(512, (rows + 7) // 8), C)


@pytest.mark.parametrize("n_partial", [1, 3])
@pytest.mark.parametrize("C", rc.BWD_WIDTHS)
def test_layernorm_backward_grid_stride_rows(C, n_partial):
    """the library binding directly with fewer workgroups than rows / 8: at 70 rows a wave walks 9 rows with one workgroup, 3 with
    three, and in the last pass some waves have none"""
    h = _lib().load()
    rows = 70
    w, _ = rc.ln_params(C)
    wd = w.to(DEV)
    xin, stream, dy, idx, addend, dx0 = _bwd_case(rows, C, BF, True, (0, 0, 0))
    xd, dyd = stream.to(DEV), dy.to(DEV)
    outs = []
    for cast in (False, True):
        nb = 3 if cast else 2
        dx, partial = dx0.clone().to(DEV), _nan(n_partial, nb * C)
        copy = torch.full((rows + rc.GUARD, C), NAN, dtype=BF, device=DEV)
        if cast:
            _check(h.m324_layernorm_bwd_cast(_p(xd), C, _p(wd), 1e-5, _p(dyd), C, _code(BF), _p(dx), C, 1, _p(partial), n_partial, rows, C,
                                             0, 0, 0, _p(copy), C, _stream()), "m324_layernorm_bwd_cast")
        else:
            _check(h.m324_layernorm_bwd(_p(xd), C, _p(wd), 1e-5, _p(dyd), C, _code(BF), _p(dx), C, 1, _p(partial), n_partial, rows, C,
                                        0, 0, 0, _stream()), "m324_layernorm_bwd")
        torch.cuda.synchronize()
        what = f"layernorm_bwd direct C={C} n_partial={n_partial} cast={cast}"
        _guards_untouched(partial, n_partial, what)
        assert not bool(torch.isnan(partial[:n_partial]).any()), what + ": a partial row was left unwritten"
        sums = partial[:n_partial].double().sum(0).cpu()
        outs.append((dx, sums[:C], sums[C:2 * C], copy, sums[2 * C:]))
    dx, dw, db, _, _ = outs[0]
    _check_bwd(f"layernorm_bwd direct C={C} n_partial={n_partial}", xin, w, dy, idx, addend, dx, dw, db, rows)
    dx2, dw2, db2, copy, third = outs[1]
    assert torch.equal(dx[:rows], dx2[:rows])
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    cc = copy.cpu()
    assert _all_nan(cc[rows:]) and torch.equal(cc[:rows], dx2[:rows].cpu().to(BF))
    depth = -(-rows // (8 * n_partial)) + 7 + n_partial
    _rec("layernorm_bwd_cast column sums", eb.assert_within(third, cc[:rows].double().sum(0), eb.colsum(cc[:rows], depth), "third vector"))


# ------------------------------------------------------------------------------------------- 4. q|k|v split, its backward, delta
def _flat_nan(rows, cols, dtype):
    return torch.full((rows + rc.GUARD, cols), NAN, dtype=dtype, device=DEV)


def _split(srcs, wq, wk, scale, B, L, H, dtype, want):
    """want: the set of outputs to emit, of "Q K V Qt Kt Vt"; returns {name: (buffer with guard rows, view)}"""
    h = _lib().load()
    Lp = (L + 63) // 64 * 64
    out = {}
    for name in ("Q", "K", "V"):
        out[name] = _flat_nan(B * H * L, 64, dtype) if name in want else None
    for name in ("Qt", "Kt", "Vt"):
        out[name] = _flat_nan(B * H * 64, Lp, dtype) if name in want else None
    q, k, v = (srcs[n] if any(o in want for o in outs) else None for n, outs in (("q", ("Q", "Qt")), ("k", ("K", "Kt")), ("v", ("V", "Vt"))))
    ld = H * 64
    _check(h.m324_qkv_split(_p(q), ld if q is not None else 0, _p(k), ld if k is not None else 0, _p(v), ld if v is not None else 0,
                            _p(wq), _p(wk), 1e-5, scale, _p(out["Q"]), _p(out["K"]), _p(out["V"]), _p(out["Qt"]), _p(out["Kt"]),
                            _p(out["Vt"]), B, L, H, _code(dtype), _stream()), "m324_qkv_split")
    torch.cuda.synchronize()
    res = {}
    for name, buf in out.items():
        if buf is None:
            continue
        n = B * H * (L if len(name) == 1 else 64)
        _guards_untouched(buf, n, f"qkv_split {name}")
        res[name] = buf[:n].cpu().reshape((B, H, L, 64) if len(name) == 1 else (B, H, 64, Lp))
    return res


def _unpermute(t):
    """[B, H, 64, Lp] in the stored key order -> natural key order (the quarter swap 0, 2, 1, 3 is its own inverse)"""
    B, H, D, Lp = t.shape
    return t.reshape(B, H, D, Lp // 16, 4, 4)[..., [0, 2, 1, 3], :].reshape(B, H, D, Lp)


SPLIT_FORMS = (("all six", ("Q", "K", "V", "Qt", "Kt", "Vt")), ("q only", ("Q", "Qt")), ("k|v only", ("K", "Kt", "V", "Vt")),
               ("transposed only", ("Qt", "Kt", "Vt")), ("inference", ("Q", "K", "Vt")))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,L,H", rc.QKV_SHAPES)
def test_qkv_split_small_and_ragged(B, L, H, dtype):
    srcs_cpu = {n: rc.rand((B * L, H * 64), 90 + i + L, 1.5).to(dtype) for i, n in enumerate("qkv")}
    srcs = {n: t.to(DEV) for n, t in srcs_cpu.items()}
    wq_c, wk_c = 1 + 0.2 * rc.rand((64,), 93), 1 + 0.2 * rc.rand((64,), 94)
    for norm in (True, False):
        wq, wk = (wq_c.to(DEV), wk_c.to(DEV)) if norm else (None, None)
        for scale in rc.Q_SCALES:
            what = f"qkv_split {(B, L, H)} {dtype} norm={norm} scale={scale:.3f}"
            full = _split(srcs, wq, wk, scale, B, L, H, dtype, SPLIT_FORMS[0][1])
            hm = {n: rc.head_major(srcs_cpu[n].float(), B, L, H) for n in "qkv"}
            for name, src, w, sc in (("Q", "q", wq_c if norm else None, scale), ("K", "k", wk_c if norm else None, 1.0)):
                ref = rc.rmsnorm_heads_reference(hm[src], w, 1e-5, sc)
                bound = eb.rmsnorm_heads(hm[src], w, 1e-5, sc, out_dtype=dtype)
                _rec(f"qkv_split {'bf16' if dtype == BF else 'fp32'}", eb.assert_within(full[name], ref, bound, f"{what} {name}"))
            assert torch.equal(full["V"], rc.head_major(srcs_cpu["v"], B, L, H)), what + ": V is a copy"
            for name in ("Q", "K", "V"):
                assert torch.equal(full[name + "t"], vt_layout(full[name])), f"{what}: {name}t against vt_layout({name})"
                assert float(_unpermute(full[name + "t"])[..., L:].float().abs().sum()) == 0.0, f"{what}: {name}t padding columns"
            for form, want in SPLIT_FORMS[1:]:
                got = _split(srcs, wq, wk, scale, B, L, H, dtype, want)
                assert sorted(got) == sorted(want)
                for name in want:
                    assert torch.equal(got[name], full[name]), f"{what}: {name} of the form '{form}'"


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,L,H", rc.QKV_SHAPES)
def test_qkv_split_backward_small_and_ragged(B, L, H, dtype):
    """through ops.qkv_split_bwd and directly with n_partial 1 and 2 (several passes per workgroup, the last one ragged; with
    B L H no multiple of 8 the clamped lanes run)"""
    ops, h = _ops(), _lib().load()
    n = B * L * H
    g_cpu = {k: rc.rand((B, H, L, 64), 100 + i + L).to(dtype) for i, k in enumerate("qkv")}
    raw_cpu = {k: rc.rand((B * L, H * 64), 104 + i + L, 1.5).to(dtype) for i, k in enumerate("qk")}
    w_cpu = {"q": 1 + 0.2 * rc.rand((64,), 107), "k": 1 + 0.2 * rc.rand((64,), 108)}
    g, raw = {k: t.to(DEV) for k, t in g_cpu.items()}, {k: t.to(DEV) for k, t in raw_cpu.items()}
    refs = {}
    for norm in (True, False):
        for k in "qk":
            x = rc.head_major(raw_cpu[k].float(), B, L, H)
            w = w_cpu[k] if norm else None
            dx, dw = rc.rmsnorm_backward_reference(x, g_cpu[k].float(), w, 1e-5)
            refs[k, norm] = (rc.token_major(dx), rc.token_major(eb.rmsnorm_heads_backward(x, g_cpu[k].float(), w, 1e-5, out_dtype=dtype)), dw,
                             eb.rmsnorm_weight_grad(x.reshape(-1, 64), g_cpu[k].float().reshape(-1, 64), 1e-5) if norm else None)
    fam = f"qkv_split_bwd {'bf16' if dtype == BF else 'fp32'}"
    for which in ("q", "k", "v", "qkv"):
        for norm in (True, False):
            for n_partial in (None, 1, 2):
                what = f"qkv_split_bwd {(B, L, H)} {dtype} which={which} norm={norm} n_partial={n_partial}"
                out = {k: _flat_nan(B * L, H * 64, dtype) if k in which else None for k in "qkv"}
                wq = w_cpu["q"].to(DEV) if norm else None
                wk = w_cpu["k"].to(DEV) if norm else None
                args = [g[k] if k in which else None for k in "qkv"]
                if n_partial is None:
                    dwq, dwk = ops.qkv_split_bwd(*args, raw["q"], raw["k"], wq, wk, 1e-5, B, L, H, out["q"], out["k"], out["v"])
                    torch.cuda.synchronize()
                else:
                    partial = _nan(n_partial, 128)
                    ld = H * 64
                    _check(h.m324_qkv_split_bwd(_p(args[0]), _p(args[1]), _p(args[2]), _p(raw["q"]), ld, _p(raw["k"]), ld, _p(wq), _p(wk), 1e-5,
                                                _p(out["q"]), ld, _p(out["k"]), ld, _p(out["v"]), ld, _p(partial), n_partial, B, L, H,
                                                _code(dtype), _stream()), "m324_qkv_split_bwd")
                    torch.cuda.synchronize()
                    _guards_untouched(partial, n_partial, what)
                    assert not bool(torch.isnan(partial[:n_partial]).any()), what + ": partial rows"
                    both = partial[:n_partial].double().sum(0).cpu()
                    dwq, dwk = both[:64], both[64:]
                for k, dwk_ in (("q", dwq), ("k", dwk)):
                    if k not in which:
                        continue
                    _guards_untouched(out[k], B * L, what)
                    ref, bound, dw_ref, dw_bound = refs[k, norm]
                    _rec(fam, eb.assert_within(out[k][:B * L], ref, bound, f"{what} d{k}"))
                    if norm:
                        _rec(fam + " weight gradient", eb.assert_within(dwk_, dw_ref, dw_bound, f"{what} d{k}_norm weight"))
                if "v" in which:
                    _guards_untouched(out["v"], B * L, what)
                    assert torch.equal(out["v"][:B * L].cpu(), rc.token_major(g_cpu["v"])), what + ": dV is a copy"


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,H,L", rc.DELTA_SHAPES)
def test_attention_delta_small(B, H, L, dtype):
    h = _lib().load()
    for ld in (H * 64, H * 64 + 8):
        o, do = rc.rand((B * L, ld), 110 + L).to(dtype), rc.rand((B * L, ld), 111 + L).to(dtype)
        od, dod = o.to(DEV), do.to(DEV)
        D = torch.full((B * H * L + 64,), NAN, device=DEV)
        _check(h.m324_attention_delta(_p(od), _p(dod), ld, _p(D), B, H, L, _code(dtype), _stream()), "m324_attention_delta")
        torch.cuda.synchronize()
        assert _all_nan(D[B * H * L:]), "attention_delta wrote behind D"
        oh, doh = (t[:, :H * 64].float().reshape(B, L, H, 64).permute(0, 2, 1, 3) for t in (o, do))
        ref = (oh.double() * doh.double()).sum(-1)
        _rec("attention_delta", eb.assert_within(D[:B * H * L].reshape(B, H, L), ref, eb.attention_delta(oh, doh),
                                                 f"attention_delta {(B, H, L)} ld={ld} {dtype}"))


# ------------------------------------------------------------------------------------------- 5. attention merge
def _merge(parts, lses, B, H, Lq, dtype, ldp, ldo):
    h = _lib().load()
    bufs = []
    for o in parts:
        t = torch.zeros((B * Lq, ldp), dtype=dtype)
        t[:, :H * 64] = o
        bufs.append(t.to(DEV))
    ls = [l.to(F32).contiguous().to(DEV) for l in lses]
    out = _nan(B * Lq, ldo, dtype)
    three = len(parts) == 3
    _check(h.m324_attention_merge(_p(bufs[0]), _p(ls[0]), _p(bufs[1]), _p(ls[1]), _p(bufs[2]) if three else None, _p(ls[2]) if three else None,
                                  ldp, _p(out), ldo, B, H, Lq, _code(dtype), _stream()), "m324_attention_merge")
    torch.cuda.synchronize()
    _guards_untouched(out, B * Lq, "attention_merge", cols=H * 64)
    return out[:B * Lq, :H * 64].cpu()


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,H,Lq", rc.MERGE_SHAPES)
@pytest.mark.parametrize("cuts", [(0, 40, 96), (0, 30, 60, 96)])
def test_attention_merge_of_a_real_key_set_small(cuts, B, H, Lq, dtype):
    """parts made on the CPU (fp64 softmax over each key range, rounded once to the operand dtype; the log2-domain LSE rounded to
    fp32): the reference is the attention over all 96 keys and eb.attention_merge applies -- each part is within the bound of a
    part m324_attention would have left"""
    scale = 64 ** -0.5
    q, k, v = (rc.rand((B, H, n, 64), 120 + i, 1.2).to(dtype).double() for i, n in enumerate((Lq, 96, 96)))
    parts, lses = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        s = torch.einsum("bhqd,bhkd->bhqk", q, k[:, :, lo:hi]) * scale
        parts.append(torch.einsum("bhqk,bhkd->bqhd", torch.softmax(s, -1), v[:, :, lo:hi]).reshape(B * Lq, H * 64).to(dtype))
        lses.append(torch.logsumexp(s, -1) / math.log(2.0))
    out = _merge(parts, lses, B, H, Lq, dtype, H * 64 + 8, H * 64 + 16)
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    ref = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(s, -1), v).reshape(B * Lq, H * 64)
    bound = eb.attention_merge(q, k, v, scale, cuts, p_bf16=False, out_dtype=dtype)
    _rec("attention_merge, real key set", eb.assert_within(out, ref, bound, f"attention_merge {cuts} {(B, H, Lq)} {dtype}"))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,H,Lq", rc.MERGE_SHAPES)
@pytest.mark.parametrize("gap", [0.0, 30.0, 160.0])
def test_attention_merge_of_synthetic_parts(gap, B, H, Lq, dtype):
    """equal LSE, a gap of 30, and a gap above 150 where the smaller part's weight underflows to zero: the result is the other
    part's row bit for bit (weight 1, and the output dtype is the parts')"""
    for n_parts in (2, 3):
        parts = [rc.rand((B * Lq, H * 64), 130 + i).to(dtype) for i in range(n_parts)]
        base = rc.rand((B, H, Lq), 135, 3.0)
        lses = [base + 0.0, base - gap] + ([base - gap] if n_parts == 3 else [])
        out = _merge(parts, lses, B, H, Lq, dtype, H * 64 + 8, H * 64 + 16)
        what = f"attention_merge synthetic gap={gap} parts={n_parts} {(B, H, Lq)} {dtype}"
        if gap > 150:
            assert torch.equal(out, parts[0]), what + ": the underflowed parts must not move the row"
            continue
        ref, bound = eb.merge_parts(parts, [l.to(F32) for l in lses], out_dtype=dtype)
        _rec("attention_merge, synthetic parts", eb.assert_within(out, ref, bound, what))


# ------------------------------------------------------------------------------------------- 6. column sums
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("case,kernel", rc.COLSUM_CASES)
def test_colsum_every_kernel(case, kernel, dtype):
    h = _lib().load()
    rows, cols, ld, voff = case
    srows = rc.colsum_scratch_rows(rows)
    name, depth = eb.colsum_plan(rows, cols, ld, aligned16=(voff == 0), scratch_rows=srows)
    assert name == kernel
    base, view = rc.colsum_input(rows, cols, ld, voff, dtype)
    bd = base.to(DEV)
    vd = bd[:, voff:voff + cols]
    assert (vd.data_ptr() % 16 == 0) == (voff == 0) and vd.stride(0) == ld
    for accumulate in (0, 1):
        addend = rc.rand((cols,), 140 + cols)
        out = torch.full((cols + 64,), NAN, device=DEV)
        if accumulate:
            out[:cols] = addend.to(DEV)
        scratch = torch.full((srows + rc.GUARD, cols), NAN, device=DEV) if srows else None
        _check(h.m324_colsum(_p(vd), vd.stride(0), _p(out), rows, cols, _code(dtype), accumulate, _p(scratch), srows, _stream()), "m324_colsum")
        torch.cuda.synchronize()
        what = f"colsum {case} -> {kernel} {dtype} accumulate={accumulate}"
        assert _all_nan(out[cols:]), what + ": wrote behind the output"
        if scratch is not None:
            _guards_untouched(scratch, srows, what + " scratch")
        ref = view.double().sum(0) + (addend.double() if accumulate else 0)
        _rec(f"colsum: {kernel}", eb.assert_within(out[:cols], ref, eb.colsum(view, depth, addend if accumulate else None), what))


def _multi_specs():
    """(sources [(rows, cols, ld, view offset)], accumulate on the head) per destination, in table order; the direct call's first
    launch is filled exactly by the 64-item chain"""
    small = (3, 40, 40, 0)
    return [
        ([small] * 64, False),                                               # fills the 64-entry table exactly
        ([small] * 65, True),                                                # cut: 64 + 1, the continuation accumulates
        ([small] * 130, False),                                              # cut twice: 64 + 64 + 2
        ([small], True), ([small] * 2, False),                               # chain lengths 1 and 2
        ([(5, 70, 70, 0), (65, 70, 70, 0), (7, 70, 70, 0)], True),           # tall: one source with 65 rows makes the whole chain tall
        ([(700, 192, 576, 0)], False),                                       # tall, ld > cols (a column group of a partial buffer)
        ([(7, 4100, 4100, 0), (9, 4100, 4100, 0)], False),                   # vector path, a second workgroup with one lane
        ([(5, 333, 333, 0)], True),                                          # scalar: cols % 4 != 0
        ([(6, 260, 264, 1), (4, 260, 260, 0)], False),                       # scalar: a misaligned source in the chain
    ]


def test_colsum_multi_paths_chains_and_cuts():
    """m324_colsum_multi directly with an item table and through ops._ColsumQueue: bit-identical to consecutive m324_colsum calls
    wherever every source has at most 64 rows (include/m324.h), everything within the bound of the fp64 sums"""
    ops, lib = _ops(), _lib()
    specs = _multi_specs()
    srcs, wants, refs, bounds, addends = [], [], [], [], []
    for i, (chain, acc) in enumerate(specs):
        cols = chain[0][1]
        views = []
        for j, (rows, c, ld, voff) in enumerate(chain):
            base, _ = rc.colsum_input(rows, c, ld, voff, F32, seed=1000 * i + j)
            views.append(base.to(DEV)[:, voff:voff + c])
        addend = rc.rand((cols,), 150 + i)
        want = torch.full((cols + 64,), NAN, device=DEV)
        if acc:
            want[:cols] = addend.to(DEV)
        for j, v in enumerate(views):
            ops.colsum(v, out=want[:cols], accumulate=acc or j > 0)
        cpu = [v.cpu() for v in views]
        srcs.append(views), wants.append(want), addends.append(addend)
        refs.append(sum(v.double().sum(0) for v in cpu) + (addend.double() if acc else 0))
        bounds.append(eb.colsum(cpu, eb.colsum_multi_depth([v.shape[0] for v in cpu]), addend if acc else None))

    def fresh():
        ds = []
        for (chain, acc), addend in zip(specs, addends):
            d = torch.full((chain[0][1] + 64,), NAN, device=DEV)
            if acc:
                d[:chain[0][1]] = addend.to(DEV)
            ds.append(d)
        return ds

    direct = fresh()
    n = sum(len(c) for c, _ in specs)
    arr = (lib.ColsumItem * n)()
    k = 0
    for (chain, acc), views, d in zip(specs, srcs, direct):
        for j, v in enumerate(views):
            it = arr[k]
            it.dst, it.src, it.ld, it.rows, it.cols = d.data_ptr(), v.data_ptr(), v.stride(0), v.shape[0], v.shape[1]
            it.accumulate, it.chain = int(acc and j == 0), int(j > 0)
            k += 1
    _check(lib.load().m324_colsum_multi(arr, n, _stream()), "m324_colsum_multi")
    queued = fresh()
    q = ops._ColsumQueue()
    q.LIMIT = 10 ** 6                                       # one flush: the cuts are the library's
    for (chain, acc), views, d in zip(specs, srcs, queued):
        for j, v in enumerate(views):
            q.defer(v, d[:chain[0][1]], acc or j > 0)
    q.flush()
    torch.cuda.synchronize()
    for how, dsts in (("direct", direct), ("queue", queued)):
        for i, ((chain, acc), d) in enumerate(zip(specs, dsts)):
            cols = chain[0][1]
            what = f"colsum_multi {how} destination {i}: {len(chain)} x {chain[0]} accumulate={acc}"
            assert _all_nan(d[cols:]), what + ": wrote behind the destination"
            if all(r <= 64 for r, *_ in chain):
                assert torch.equal(d[:cols], wants[i][:cols]), what + ": differs from consecutive m324_colsum calls"
            _rec("colsum_multi", eb.assert_within(d[:cols], refs[i], bounds[i], what))
    for i, want in enumerate(wants):                        # the consecutive single calls themselves, against fp64
        depth = max(eb.colsum_plan(r, c, ld, vo == 0, rc.colsum_scratch_rows(r))[1] for r, c, ld, vo in specs[i][0]) + len(specs[i][0])
        cpu = [v.cpu() for v in srcs[i]]
        eb.assert_within(want[:specs[i][0][0][1]], refs[i], eb.colsum(cpu, depth, addends[i] if specs[i][1] else None), f"consecutive colsum {i}")


# ------------------------------------------------------------------------------------------- 7. GELU, cast
def _gelu_both(z, dh):
    h = _lib().load()
    n, dtype = z.numel(), z.dtype
    zd, dhd = z.to(DEV), dh.to(DEV)
    out, dz = torch.full((n + 64,), NAN, dtype=dtype, device=DEV), torch.full((n + 64,), NAN, dtype=dtype, device=DEV)
    _check(h.m324_gelu(_p(zd), _p(out), n, _code(dtype), _stream()), "m324_gelu")
    _check(h.m324_gelu_bwd(_p(zd), _p(dhd), _p(dz), n, _code(dtype), _stream()), "m324_gelu_bwd")
    torch.cuda.synchronize()
    assert _all_nan(out[n:]) and _all_nan(dz[n:]), "gelu wrote behind its output"
    return out[:n].cpu(), dz[:n].cpu()


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("n,kernel", rc.GELU_SMALL)
def test_gelu_forward_backward_small(n, kernel, dtype):
    assert (n % 8 == 0) == (kernel == "8-wide")
    z, dh = rc.gelu_input(n, dtype), rc.rand((n,), 160 + n).to(dtype)
    out, dz = _gelu_both(z, dh)
    _rec("gelu", eb.assert_within(out, eb.gelu(z.double()), eb.gelu_elementwise(z, out_dtype=dtype), f"gelu n={n} {kernel} {dtype}"))
    _rec("gelu_bwd", eb.assert_within(dz, dh.double() * eb.gelu_grad(z.double()), eb.gelu_backward(z, dh, out_dtype=dtype),
                                      f"gelu_bwd n={n} {kernel} {dtype}"))


@pytest.mark.parametrize("n,kernel", rc.GELU_LARGE)
def test_gelu_past_the_grid_caps(n, kernel):
    """bf16; the grid-stride loops take a second turn.  The input repeats a block of 2^20 values: the first block and the tail are
    held to the bound element by element, every further block must equal the first bit for bit (same inputs, an element-wise
    kernel), which holds every element of the output to the bound."""
    blk = 1 << 20
    zb, dhb = rc.gelu_input(blk, BF), rc.rand((blk,), 170).to(BF)
    reps, tail = divmod(n, blk)
    z = torch.cat([zb.repeat(reps), zb[:tail]])
    dh = torch.cat([dhb.repeat(reps), dhb[:tail]])
    out, dz = _gelu_both(z, dh)
    for got, ref, bound, what in ((out, eb.gelu(zb.double()), eb.gelu_elementwise(zb), "gelu"),
                                  (dz, dhb.double() * eb.gelu_grad(zb.double()), eb.gelu_backward(zb, dhb), "gelu_bwd")):
        _rec(what, eb.assert_within(got[:blk], ref, bound, f"{what} n={n} {kernel}"))
        if reps > 1:
            assert torch.equal(got[:reps * blk].view(torch.int16).reshape(reps, blk), got[:blk].view(torch.int16).expand(reps, blk)), what
        if tail:
            eb.assert_within(got[reps * blk:], ref[:tail], bound[:tail], f"{what} n={n} tail")


@pytest.mark.parametrize("src,dst", [(F32, BF), (BF, F32)])
@pytest.mark.parametrize("cols,kernel", rc.CAST_COLS)
def test_cast_one_row_strided(cols, kernel, src, dst):
    """rows = 1, leading dimensions cols + 8 / cols + 16: cast8_kernel needs cols and both leading dimensions to be multiples of 8"""
    h = _lib().load()
    ld_in, ld_out = cols + 8, cols + 16
    assert (cols % 8 == 0 and ld_in % 8 == 0 and ld_out % 8 == 0) == (kernel == "cast8_kernel")
    x = rc.rand((1, ld_in), 180 + cols, 3.0).to(src)
    xd = x.to(DEV)
    out = _nan(1, ld_out, dst)
    _check(h.m324_cast(_p(xd), ld_in, _code(src), _p(out), ld_out, _code(dst), 1, cols, _stream()), "m324_cast")
    torch.cuda.synchronize()
    _guards_untouched(out, 1, f"cast cols={cols}", cols=cols)
    assert torch.equal(out[:1, :cols].cpu(), x[:, :cols].to(dst))
