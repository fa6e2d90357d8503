"""Attention over many (batch, head) items, on both grid forms of m324_attention.

attn_bf16_kernel runs on a 3-D grid (query tile, head, batch) or, when attn_plan (motion324_amd/csrc/attention.hip) sets nqt > 0,
on a flat grid whose 1-D index the kernel decodes itself: each of the 8 XCDs takes a contiguous range of q + 1 or q items
(q = nb >> 3, r = nb & 7), then qt = lid % nqt, h = (lid / nqt) % H, b = lid / (nqt * H).  The hand-placed long-sequence kernels
(attn_pwg_kernel.inl) repeat that decode.  Production attention is flat (32 frames x 12 heads x 3 tiles = 1152 workgroups); the other
attention tests use the smallest shape per kernel and so run the four-wave kernels on the 3-D grid only.

ROWS has one row per compiled kernel that can run flat, at the smallest item that still has two query tiles and a ragged last key
tile, with enough (batch, head) items to cross the 512-workgroup line at a chosen nb % 8.  The host-only test pins the table against
m324_attention_plan, so a chooser change that moves a row off the form it is meant to test fails there, by name.  On the GPU:

  items    every (b, h) has operands of its own; all of O and of lse within the error_bounds.py bound of fp64 (ratio 1.0);
  slices   batches [0:2] and [B-2:B] as calls of their own -- on the 3-D grid for the four-wave kernels, on a flat grid of another
           size for the others -- are the flat launch's rows bit for bit: the grid form is invisible;
  window   m324_attention_rows on the flat grid (the production kernel at 19 x 9 items of 324 tokens = 513 workgroups);
  strides  a padded batch stride of Q, and shared queries (q_bstride == 0) with more than one key tile, on the flat grid.
"""
import functools
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import error_bounds as eb
from conftest import GOLDEN, vt_layout
from test_rows_gpu import _votes

gpu = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
BF16_CODE = 1                        # motion324_amd.lib.BF16 (the host-only test runs without the package)
SENTINEL = 0x5A5A                    # bf16 bit pattern of rows nobody may write (tests/test_rows_gpu.py)
SENTINEL32 = 0x5A5A5A5A              # the same for the fp32 lse

PS, VROW, BOUNDED, SHARED = dict(prescaled=True), dict(v_rowmajor=True), dict(bounded=True), dict(shared_q=True)
NW8 = ("M324_ATTN_NW", 8)
#        id               tunable kwargs                      B   H  Lq    Lk    kernel                                      nb   nb % 8
ROWS = [("ps-vrow",       None,   {**PS, **VROW},             43, 6, 130,  130,  "attn_bf16_kernel<true, 1, 4, true, 2>",    516, 4),
        ("plain",         None,   {},                         32, 8, 130,  130,  "attn_bf16_kernel<false, 1, 4, false, 3>",  512, 0),
        ("ps-257",        None,   PS,                         19, 9, 257,  257,  "attn_bf16_kernel<true, 1, 4, false, 2>",   513, 1),
        ("vrow",          None,   VROW,                       43, 6, 130,  130,  "attn_bf16_kernel<false, 1, 4, true, 3>",   516, 4),
        ("ps-1100",       None,   PS,                         43, 6, 130,  1100, "attn_bf16_kernel<true, 1, 4, false, 3>",   516, 4),
        ("ps-vrow-1100",  None,   {**PS, **VROW},             43, 6, 130,  1100, "attn_bf16_kernel<true, 1, 4, true, 3>",    516, 4),
        ("ps-shared",     None,   {**PS, **SHARED},           43, 6, 130,  130,  "attn_bf16_kernel<true, 1, 4, false, 2>",   516, 4),
        ("nw8-ps",        NW8,    PS,                         3,  3, 300,  130,  "attn_bf16_kernel<true, 1, 8, false, 3>",   18,  2),
        ("nw8-plain",     NW8,    {},                         3,  3, 300,  130,  "attn_bf16_kernel<false, 1, 8, false, 3>",  18,  2),
        ("nw8-ps-vrow",   NW8,    {**PS, **VROW},             3,  3, 300,  130,  "attn_bf16_kernel<true, 1, 8, true, 3>",    18,  2),
        ("nw8-vrow",      NW8,    VROW,                       3,  3, 300,  130,  "attn_bf16_kernel<false, 1, 8, true, 3>",   18,  2),
        ("pwg",           None,   PS,                         3,  3, 2049, 513,  "attn_pwg_kernel",                          81,  1),
        ("pwg-bounded",   None,   {**PS, **BOUNDED},          3,  3, 2049, 513,  "attn_pwg_bounded_kernel",                  81,  1)]
IDS = [r[0] for r in ROWS]
BY_ID = {r[0]: r for r in ROWS}
# the forms without a flat grid, at as many items: (tunable, kwargs, B, H, Lq, Lk, kernel).  The frame loop takes batches in pairs,
# so its row has 44 of them.
NEVER_FLAT = [(None, {**PS, **SHARED}, 43, 6, 130,  64, "attn_bf16_kernel<true, 1, 4, false, 1>"),
              (None, {**PS, **SHARED}, 43, 6, 1030, 64, "attn_bf16_kernel<true, 1, 4, false, 1>"),
              (None, PS,               43, 6, 130,  64, "attn_bf16_kernel<true, 1, 4, false, 1>"),
              (None, {**PS, **SHARED}, 44, 6, 513,  64, "attn_frames_kernel<2, true>")]
# the window of section "window": the production per-frame kernel, flat at 513 workgroups
WIN = dict(B=19, H=9, L=324, kernel="attn_bf16_kernel<true, 1, 4, true, 2>", nb=513, seed=324)
WIN_ROWS = [32, 96, 160, 288]


def _flags(kw):
    """M324_ATTN_* of a call, and bit 8 (the queries are shared) as m324_attention_plan takes it"""
    return (int(bool(kw.get("prescaled"))) | (2 if kw.get("v_rowmajor") else 0) | (4 if kw.get("bounded") else 0)
            | (256 if kw.get("shared_q") else 0))


def _four_waves(kernel):
    return kernel.startswith("attn_bf16_kernel<") and kernel.split(", ")[2] == "4"


def _grid(plan):
    """'name grid=<grid.x * threads>x<y>x<z>' -> (name, workgroups along x, y, z)"""
    name, grid = plan.split(" grid=")
    x, y, z = (int(v) for v in grid.split("x"))
    threads = 64 * int(name.split(", ")[2]) if name.startswith("attn_bf16_kernel<") else 256
    assert x % threads == 0, plan
    return name, x // threads, y, z


# ------------------------------------------------------------------------------------------- 1. the table, on the host
_ASK = """
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import make_plan_table as t
L = t.load_lib()
h = L.load()
buf = ctypes.create_string_buffer(256)
out = []
for tunable, B, H, Lq, Lk, flags in json.loads(sys.argv[2]):
    if tunable:
        L.set_tunable(*tunable)
    buf.value = b""
    rc = h.m324_attention_plan(B, H, Lq, Lk, flags, %d, buf, 256)
    out.append([rc, buf.value.decode()])
    if tunable:
        L.set_tunable(tunable[0])
print(json.dumps(out))
""" % BF16_CODE


def test_case_table_names_the_kernels_and_grids_it_is_meant_to_test():
    """Every row of ROWS: the whole kernel name, a flat grid of nb workgroups, nb % 8 as listed; the four-wave rows at B = 2 (the
    slice form): the same kernel on a 3-D grid; the other rows at B = 2: flat again, another size; the one-tile form and the frame
    loop: 3-D at as many items.  A child process with the devices hidden answers, as in tests/test_plans_cpu.py."""
    asks = [(tun, B, H, Lq, Lk, _flags(kw)) for _, tun, kw, B, H, Lq, Lk, _, _, _ in ROWS]
    asks += [(tun, 2, H, Lq, Lk, _flags(kw)) for _, tun, kw, B, H, Lq, Lk, _, _, _ in ROWS]
    asks += [(tun, B, H, Lq, Lk, _flags(kw)) for tun, kw, B, H, Lq, Lk, _ in NEVER_FLAT]
    asks += [(None, WIN["B"], WIN["H"], WIN["L"], WIN["L"], 3), (None, 2, WIN["H"], WIN["L"], WIN["L"], 3)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("M324_") or k == "M324_LIB"}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _ASK, GOLDEN, json.dumps(asks)], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == len(asks)
    n = len(ROWS)
    assert len({row[7] for row in ROWS}) == 12                       # ps / no vrow / two stages twice: own q and shared q
    for (rid, _, kw, B, H, Lq, Lk, kernel, nb, rem), (rc, plan), (rc2, plan2) in zip(ROWS, got[:n], got[n:2 * n]):
        name, x, y, z = _grid(plan)
        assert name == kernel, (rid, plan)
        assert rc == (8 if ", 8, " in kernel else 4), (rid, rc)
        assert (y, z) == (1, 1) and x == nb and nb % 8 == rem, (rid, plan)
        tiles = -(-Lq // (256 if not _four_waves(kernel) else 128))
        assert nb == tiles * H * B and tiles >= 2 and Lk % 64 != 0 and Lk > 64, rid
        name2, x2, y2, z2 = _grid(plan2)
        assert name2 == kernel, (rid, plan2)
        if _four_waves(kernel):
            assert (x2, y2, z2) == (tiles, H, 2), (rid, plan2)       # the slice form: the same kernel, blockIdx is the item
        else:
            assert (x2, y2, z2) == (tiles * H * 2, 1, 1), (rid, plan2)
    for (tun, kw, B, H, Lq, Lk, kernel), (rc, plan) in zip(NEVER_FLAT, got[2 * n:]):
        name, x, y, z = _grid(plan)
        assert name == kernel, plan
        assert (x, y, z) == (-(-Lq // 128), H, B // 2 if "frames" in kernel else B), plan
    (_, full), (_, two) = got[-2:]
    assert _grid(full) == (WIN["kernel"], WIN["nb"], 1, 1) and _grid(two) == (WIN["kernel"], 3, WIN["H"], 2)


# ------------------------------------------------------------------------------------------- operands and launches
def _ops():
    from motion324_amd import ops
    return ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


@functools.lru_cache(maxsize=2)
def _operands(rid):
    """The row's operands at the scales of test_attention_strided_out (q, k: 1.5, v: 1), every (b, h) its own: bf16 values on the
    host (q [1 or B, H, Lq, 64], k, v [B, H, Lk, 64]) and on the device (v row-major or in the Vt layout), and the scale that turns
    q . k into the natural-log score."""
    _, _, kw, B, H, Lq, Lk, _, _, _ = BY_ID[rid]
    ops = _ops()
    pre = bool(kw.get("prescaled"))
    seed = 1000 + 10 * IDS.index(rid)
    q = _rand((1 if kw.get("shared_q") else B, H, Lq, 64), seed, 1.5)
    k, v = _rand((B, H, Lk, 64), seed + 1, 1.5), _rand((B, H, Lk, 64), seed + 2)
    q, k, v = (q * ops.Q_PRESCALE if pre else q).to(BF), k.to(BF), v.to(BF)
    dv = (v if kw.get("v_rowmajor") else vt_layout(v)).to(DEV)
    return dict(q=q, k=k, v=v, dq=q.to(DEV), dk=k.to(DEV), dv=dv, scale=math.log(2.0) if pre else 64 ** -0.5)


def _launch(kw, dq, dk, dv):
    """one m324_attention call into NaN-filled O [B * Lq, H * 64] and lse [B, H, Lq]"""
    B, H, Lq = dk.shape[0], dk.shape[1], dq.shape[2]
    out = torch.full((B * Lq, H * 64), NAN, dtype=BF, device=DEV)
    lse = torch.full((B, H, Lq), NAN, device=DEV)
    _ops().attention(dq, dk, dv, out, lse=lse, **kw)
    return out, lse


def _plan(kw, B, H, Lq, Lk):
    ops = _ops()
    return ops._attn_plan(B, H, Lq, Lk, _flags(kw), ops.code_of(BF))


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int16 if a.dtype == BF else torch.int32
    return a.shape == b.shape and torch.equal(a.view(it), b.view(it))


@pytest.fixture(scope="module", params=IDS)
def flat(request):
    """The row's flat launch, made once for the tests of that row; its tunable stays set while they run."""
    from motion324_amd import lib
    rid = request.param
    _, tunable, kw, B, H, Lq, Lk, kernel, nb, _ = BY_ID[rid]
    if tunable:
        lib.set_tunable(*tunable)
    try:
        assert _grid(_plan(kw, B, H, Lq, Lk)) == (kernel, nb, 1, 1)
        op = _operands(rid)
        out, lse = _launch(kw, op["dq"], op["dk"], op["dv"])
        torch.cuda.synchronize()
        yield dict(op, rid=rid, out=out, lse=lse)
    finally:
        if tunable:
            lib.set_tunable(tunable[0])


def _reference(q, k, v, scale):
    """fp64 O [B * Lq, H * 64] and log2-domain lse [B, H, Lq] of bf16 operand values"""
    B = k.shape[0]
    s = torch.einsum("bhqd,bhkd->bhqk", q.expand(B, -1, -1, -1).double(), k.double()) * scale
    o = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(s, dim=-1), v.double())
    return o.reshape(B * q.shape[2], -1), torch.logsumexp(s, dim=-1) / math.log(2.0), s


# ------------------------------------------------------------------------------------------- 2. every item right
@gpu
def test_every_item_of_the_flat_grid_is_within_the_bound(flat):
    """All of O and all of lse of the flat launch against fp64, element by element under eb.attention_and_lse: a (batch, head,
    tile) that the decode sends to another item's operands, or that no workgroup computes (NaN prefill), is an O(1) error in a
    whole head.  Worst err / bound on the MI355X: tests/ERROR_BOUNDS.md."""
    rid = flat["rid"]
    kw = BY_ID[rid][2]
    ref, lse_ref, s = _reference(flat["q"], flat["k"], flat["v"], flat["scale"])
    if kw.get("bounded"):
        assert float(s.abs().max()) / math.log(2.0) < 60.0
    del s
    bound, lse_bound = eb.attention_and_lse(flat["q"], flat["k"], flat["v"], flat["scale"])
    wo = eb.assert_within(flat["out"], ref, bound, f"attention items {rid}")
    wl = eb.assert_within(flat["lse"], lse_ref, lse_bound, f"lse items {rid}")
    print(f"[items] {rid}: worst err / bound attention {wo:.3f} lse {wl:.3f}")


# ------------------------------------------------------------------------------------------- 3. the grid form is invisible
@gpu
def test_batch_slices_on_the_other_grid_equal_the_flat_launch(flat):
    """Batches [0:2] and [B-2:B] as calls of their own: 3-D grid, same kernel for the four-wave rows (asserted), a flat grid of
    another size for the eight-wave and one-wave-per-SIMD rows; O and lse are the flat launch's rows of those batches, bit for bit."""
    rid = flat["rid"]
    _, _, kw, B, H, Lq, Lk, kernel, nb, _ = BY_ID[rid]
    name, x, y, z = _grid(_plan(kw, 2, H, Lq, Lk))
    assert name == kernel
    if _four_waves(kernel):
        assert (x, y, z) == (nb // (B * H), H, 2)
    else:
        assert (y, z) == (1, 1) and x == nb // B * 2 and x != nb
    for b0 in (0, B - 2):
        dq = flat["dq"] if kw.get("shared_q") else flat["dq"][b0:b0 + 2]
        out, lse = _launch(kw, dq, flat["dk"][b0:b0 + 2], flat["dv"][b0:b0 + 2])
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
        assert _same_bits(out, flat["out"][b0 * Lq:(b0 + 2) * Lq]), f"{rid}: O of batches {b0}, {b0 + 1}"
        assert _same_bits(lse, flat["lse"][b0:b0 + 2]), f"{rid}: lse of batches {b0}, {b0 + 1}"


# ------------------------------------------------------------------------------------------- 4. the window on the flat grid
@pytest.fixture(scope="module")
def window_case():
    """Operands as _attn_operands of tests/test_rows_gpu.py chooses them (scores ~ N(0, 6^2) in the log2 domain: a few lie 8 above
    the first tile's maximum, so the lazy reference maximum moves on a vote), the full flat launch, its fp64 reference and bound."""
    B, H, L = WIN["B"], WIN["H"], WIN["L"]
    g = torch.Generator().manual_seed(WIN["seed"])
    Q = (torch.randn((B, H, L, 64), generator=g) * 0.75).to(BF)
    K = torch.randn((B, H, L, 64), generator=g).to(BF)
    V = torch.randn((B, H, L, 64), generator=g).to(BF)
    kw = {**PS, **VROW}
    assert _grid(_plan(kw, B, H, L, L)) == (WIN["kernel"], WIN["nb"], 1, 1)
    dq, dk, dv = Q.to(DEV), K.to(DEV), V.to(DEV)
    out, lse = _launch(kw, dq, dk, dv)
    torch.cuda.synchronize()
    ref, lse_ref, _ = _reference(Q, K, V, math.log(2.0))
    bound, lse_bound = eb.attention_and_lse(Q, K, V, math.log(2.0))
    return dict(Q=Q, K=K, dq=dq, dk=dk, dv=dv, kw=kw, out=out, lse=lse, ref=ref, lse_ref=lse_ref, bound=bound, lse_bound=lse_bound)


@gpu
@pytest.mark.parametrize("q_rows", WIN_ROWS)
def test_window_on_the_flat_grid_equals_the_full_flat_launch(window_case, q_rows):
    """m324_attention_rows where production runs it: the full plan is flat (513 workgroups), so the window launches flat on
    ceil(q_rows / 128) tiles per item.  Rows below q_rows: the full launch's bits and within the bound of fp64; rows from q_rows
    on: the sentinel, in O and in lse.  The inputs make the vote move in blocks that also hold calm rows (asserted)."""
    c = window_case
    B, H, L = WIN["B"], WIN["H"], WIN["L"]
    moved, mixed = _votes(c["Q"], c["K"], q_rows)
    print(f"[window] q_rows={q_rows}: reference moved in {moved} (block, tile) pairs, {mixed} of them with calm rows")
    assert moved > 0 and mixed > 0, "the inputs do not exercise the vote path"
    win = torch.full((B * L, H * 64), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
    wlse = torch.full((B, H, L), SENTINEL32, dtype=torch.int32, device=DEV).view(torch.float32)
    _ops().attention(c["dq"], c["dk"], c["dv"], win, lse=wlse, q_rows=q_rows, **c["kw"])
    torch.cuda.synchronize()
    w, f = win.view(torch.int16).view(B, L, H * 64), c["out"].view(torch.int16).view(B, L, H * 64)
    assert torch.equal(w[:, :q_rows], f[:, :q_rows])
    assert bool((w[:, q_rows:] == SENTINEL).all())
    wl, fl = wlse.view(torch.int32), c["lse"].view(torch.int32)
    assert torch.equal(wl[..., :q_rows], fl[..., :q_rows])
    assert bool((wl[..., q_rows:] == SENTINEL32).all())
    rows = lambda t: t.view(B, L, H * 64)[:, :q_rows]
    wo = eb.assert_within(rows(win), rows(c["ref"]), rows(c["bound"]), f"attention window q_rows={q_rows}")
    wl = eb.assert_within(wlse[..., :q_rows], c["lse_ref"][..., :q_rows], c["lse_bound"][..., :q_rows], f"lse window q_rows={q_rows}")
    print(f"[window] q_rows={q_rows}: worst err / bound attention {wo:.3f} lse {wl:.3f}")


# ------------------------------------------------------------------------------------------- 5. batch strides of Q
@gpu
def test_padded_q_batch_stride_on_the_flat_grid():
    """Q in a buffer with q_bstride = H * Lq * 64 + 192, NaN between the batches (ops.attention cannot express the stride: the
    library is called directly): the contiguous call's O and lse, bit for bit."""
    from motion324_amd import lib
    rid, _, kw, B, H, Lq, Lk, kernel, nb, _ = ROWS[0]
    op = _operands(rid)
    assert _grid(_plan(kw, B, H, Lq, Lk)) == (kernel, nb, 1, 1)
    out0, lse0 = _launch(kw, op["dq"], op["dk"], op["dv"])
    item, pad = H * Lq * 64, 192
    buf = torch.full((B, item + pad), NAN, dtype=BF, device=DEV)
    buf[:, :item] = op["dq"].reshape(B, item)
    assert bool(torch.isnan(buf[:, item:].float()).all())
    out = torch.full((B * Lq, H * 64), NAN, dtype=BF, device=DEV)
    lse = torch.full((B, H, Lq), NAN, device=DEV)
    rc = lib.load().m324_attention(buf.data_ptr(), item + pad, op["dk"].data_ptr(), op["dv"].data_ptr(), out.data_ptr(), H * 64, B, H, Lq, Lk,
                                   64 ** -0.5, _flags(kw), lse.data_ptr(), lib.BF16, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    assert torch.isfinite(out0.float()).all() and torch.isfinite(lse0).all()
    assert _same_bits(out, out0) and _same_bits(lse, lse0)


@gpu
def test_shared_q_on_the_flat_grid_equals_q_copied_per_batch():
    """q_bstride == 0 with three key tiles on the flat grid: the call with Q copied B times (q_bstride = H * Lq * 64, the same
    kernel and grid), bit for bit, and within the bound of fp64."""
    rid = "ps-shared"
    _, _, kw, B, H, Lq, Lk, kernel, nb, _ = BY_ID[rid]
    op = _operands(rid)
    own = {k: v for k, v in kw.items() if k != "shared_q"}
    assert _grid(_plan(kw, B, H, Lq, Lk)) == _grid(_plan(own, B, H, Lq, Lk)) == (kernel, nb, 1, 1)
    out, lse = _launch(kw, op["dq"], op["dk"], op["dv"])
    out0, lse0 = _launch(own, op["dq"].expand(B, -1, -1, -1).contiguous(), op["dk"], op["dv"])
    torch.cuda.synchronize()
    assert _same_bits(out, out0) and _same_bits(lse, lse0)
    ref, lse_ref, _ = _reference(op["q"], op["k"], op["v"], op["scale"])
    bound, lse_bound = eb.attention_and_lse(op["q"], op["k"], op["v"], op["scale"])
    wo = eb.assert_within(out, ref, bound, "attention, shared q on the flat grid")
    wl = eb.assert_within(lse, lse_ref, lse_bound, "lse, shared q on the flat grid")
    print(f"[shared q] worst err / bound attention {wo:.3f} lse {wl:.3f}")
