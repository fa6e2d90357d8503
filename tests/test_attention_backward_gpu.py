"""The bf16 attention backward behind every forward kernel that training puts in front of it, at long and ragged shapes.

The chain is backward.self_attn_block_bwd's: ops.qkv_split(train=True) for q, k|v and dO -> ops.attention(prescaled, lse) ->
ops.attention_delta -> ops.attention_bwd_mfma.  The reference is fp64 autograd on the stored operands, and THE ONLY GATE is
error_bounds.assert_within: every element of out, lse, dQ (summed over the batches when the queries are shared), dK and dV, nothing
masked, against the analytic bounds of error_bounds.attention_and_lse / attention_backward.  Where the fp32-arithmetic
ops.attention_bwd runs too, it is held to its own bound (p_bf16=False), not to a distance from the MFMA result.

Inputs and cases: tests/attn_bwd_cases.py (two dominant keys for every query at a tile / wave / workgroup edge, every edge key in such
a pair).  tests/test_attention_backward_cpu.py shows on the CPU model that these inputs put a kernel that loses an edge key, an edge
query, the ln 2, the right LSE / D row or the key order of Kt at 4.9x .. 1e5x the bound.  References and bounds are computed once per
case and shared by every test here.  Worst err / bound on the MI355X: tests/ERROR_BOUNDS.md.
"""
import pytest
import torch

import attn_bwd_cases as ac
import error_bounds as eb

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
OUTS = ("out", "lse", "dQ", "dK", "dV")
GRADS = ("dQ", "dK", "dV")


def _ops():
    from motion324_amd import ops
    return ops


def _plan(name, kw):
    ops = _ops()
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    flags = 1 | (4 if kw.get("bounded") else 0) | (256 if shared else 0)        # prescaled q, transposed Vt
    return ops._attn_plan(B, H, Lq, Lk, flags, ops.code_of(BF)).split(" grid=")[0]


def _forward(name, *, kw=None, k=None, v=None):
    """m324_qkv_split of q and k|v (no norm weights: the stored operands are the case's values, asserted bit for bit) and
    m324_attention into NaN-filled O and lse.  k / v: other values than the case's (the non-finite runs)."""
    ops = _ops()
    inp = ac.inputs(name)
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    Bq = 1 if shared else B
    k, v = inp["k"] if k is None else k, inp["v"] if v is None else v
    tok = lambda t: ac.token_major(t).to(DEV)
    spq = ops.qkv_split(tok(inp["q_src"]), None, None, None, None, 0.0, Bq, Lq, H, BF, q_scale=ops.Q_PRESCALE, train=True)
    spk = ops.qkv_split(None, tok(k), tok(v), None, None, 0.0, B, Lk, H, BF, train=True)
    assert ops.Q_PRESCALE == ac.Q_PRESCALE
    assert torch.equal(spq["Q"].cpu(), inp["qs"]), "m324_qkv_split stores another q than the reference assumes"
    out = torch.full((B * Lq, H * 64), NAN, dtype=BF, device=DEV)
    lse = torch.full((B, H, Lq), NAN, device=DEV)
    ops.attention(spq["Q"], spk["K"], spk["Vt"], out, shared_q=shared, prescaled=True, lse=lse, **(kw or {}))
    return dict(spq=spq, spk=spk, out=out, lse=lse)


def _backward(name, fwd, *, dO=None, fp32_arithmetic=False):
    """m324_attention_delta on the stored O, m324_qkv_split of dO, m324_attention_bwd_mfma (or the fp32-arithmetic m324_attention_bwd)"""
    ops = _ops()
    inp = ac.inputs(name)
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    dO_tok = ac.token_major(inp["dO"] if dO is None else dO).to(DEV)
    D = ops.attention_delta(fwd["out"], dO_tok, B, H, Lq)
    spdo = ops.qkv_split(dO_tok, None, None, None, None, 0.0, B, Lq, H, BF, train=True)
    if fp32_arithmetic:
        dQ, dK, dV = ops.attention_bwd(fwd["spq"]["Q"], fwd["spk"]["K"], fwd["spk"]["V"], spdo["Q"], fwd["lse"], D, shared_q=shared)
    else:
        dQ, dK, dV = ops.attention_bwd_mfma(fwd["spq"], fwd["spk"], spdo, fwd["lse"], D, shared_q=shared)
    torch.cuda.synchronize()
    return dict(out=fwd["out"], lse=fwd["lse"], dQ=dQ, dK=dK, dV=dV)


def _host(name, got):
    """the outputs on the host; dQ summed over the batches in fp64 when the queries are shared (autograd's dQ is that sum)"""
    res = {k: v.float().cpu().double() for k, v in got.items()}
    if ac.CASES[name][4]:
        res["dQ"] = res["dQ"].sum(0, keepdim=True)
    return res


def _assert_chain(name, got, what, *, kind="mfma", f32=False, keys=OUTS):
    ref, bnd = ac.reference(name, f32), ac.bounds(name, kind)
    res = _host(name, got)
    worst = {k: eb.assert_within(res[k], ref[k], bnd[k], f"{k}, {name}, {what}") for k in keys}
    print(f"[attention backward] {name}, {what}: worst err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


RUNS = [(name, "default") for name in ac.CASES] + [(name, var) for name, vs in ac.VARIANTS.items() for var in vs]


def _variant(name, var):
    if var == "default":
        return None, {}, ac.CASES[name][5]
    return ac.VARIANTS[name][var]


# ------------------------------------------------------------------------------------------- 1. the table
def test_case_table_selects_the_forward_kernels_it_names(tune):
    """Every case and forward variant through ops._attn_plan, by the whole kernel name: if the chooser moves, the table fails here
    instead of silently testing another kernel.  The table must hold the forwards no other backward test runs."""
    for name, var in RUNS:
        tunable, kw, kernel = _variant(name, var)
        if tunable:
            tune(*tunable)
        assert _plan(name, kw) == kernel, (name, var, _plan(name, kw))
        if tunable:
            from motion324_amd import lib
            lib.set_tunable(tunable[0])
    kernels = {_variant(n, v)[2] for n, v in RUNS}
    assert {"attn_pwg_kernel", "attn_pwg_bounded_kernel", "attn_frames_kernel<2, true>", "attn_bf16_kernel<true, 1, 8, false, 3>",
            ac.PLAIN3, ac.PLAIN2, ac.PLAIN1} == kernels
    B, H, Lq, Lk, _, _ = ac.CASES["pwg"]
    assert Lk >= 1024 and Lk % 64 and Lq % 256 and Lq >= 2048                   # M324_ATTN_BWD_NW=2 reaches attn_bwd_dq2_mfma_kernel; ragged both ways
    assert ac.CASES["tiles-exact"][2] % 64 == 0 and ac.CASES["tiles-exact"][3] % 64 == 0


# ------------------------------------------------------------------------------------------- 2. every forward, default backward
@pytest.mark.parametrize("name,var", RUNS, ids=[f"{n}-{v}" for n, v in RUNS])
def test_backward_behind_every_forward_kernel(tune, name, var):
    """Default backward tunables behind the case's forward (asserted by name): out, lse, dQ, dK, dV within their bounds.  The small
    cases also run the fp32-arithmetic m324_attention_bwd on the same stored O, LSE and D, against its own bound."""
    tunable, kw, kernel = _variant(name, var)
    if tunable:
        tune(*tunable)
    assert _plan(name, kw) == kernel
    fwd = _forward(name, kw=kw)
    got = _backward(name, fwd)
    _assert_chain(name, got, f"{var} ({kernel})")
    if name != "pwg":
        _assert_chain(name, _backward(name, fwd, fp32_arithmetic=True), f"{var}, fp32-arithmetic backward", kind="fp32-arithmetic", keys=GRADS)


# ------------------------------------------------------------------------------------------- 3. wave layouts
def test_every_wave_layout_at_the_long_ragged_case(tune):
    """M324_ATTN_BWD_NW in {0, 4, 8, 84, 48, 2} at 2100 x 1090 behind attn_pwg_kernel, every result within the bound.  There is no
    plan query for the backward; which kernels a mode launches rests on reading m324_attention_bwd_mfma (attention.hip):
      0, 4  attn_bwd_dq_mfma_kernel<4> + attn_bwd_dkv_mfma_kernel<4>       8   <8> + <8>
      84    dQ <8>, dK / dV <4>                                            48  dQ <4>, dK / dV <8>
      2     attn_bwd_dq2_mfma_kernel (Lk >= 1024), dK / dV <8>
    so the halves that share a kernel are equal bit for bit: 0 == 4; 84 == (8's dQ, 4's dK / dV); 48 == (4's dQ, 8's dK / dV);
    2's dK / dV == 8's.  dQ of mode 2 (64 queries per wave) is held by its bound alone."""
    name = "pwg"
    assert _plan(name, {}) == "attn_pwg_kernel" and ac.CASES[name][3] >= 1024
    fwd = _forward(name)
    got = {}
    for nw in (0, 4, 8, 84, 48, 2):
        tune("M324_ATTN_BWD_NW", nw)
        got[nw] = _backward(name, fwd)
        _assert_chain(name, got[nw], f"M324_ATTN_BWD_NW={nw}", keys=GRADS)
    same = lambda a, b, keys: all(_same_bits(got[a][k], got[b][k]) for k in keys)
    assert same(0, 4, GRADS)
    assert same(84, 8, ("dQ",)) and same(84, 4, ("dK", "dV"))
    assert same(48, 4, ("dQ",)) and same(48, 8, ("dK", "dV"))
    assert same(2, 8, ("dK", "dV"))


@pytest.mark.parametrize("nw", [4, 8])
@pytest.mark.parametrize("name", ["one-tile", "frames"])
def test_wave_layouts_with_one_partly_filled_workgroup(tune, name, nw):
    """Lk = 37: the dK / dV kernel's only workgroup is partly filled at both sizes (one wave of four / eight has five live lanes in
    its second key block), and the dQ kernel's only key tile is the ragged one."""
    tune("M324_ATTN_BWD_NW", nw)
    assert _plan(name, {}) == ac.CASES[name][5]
    _assert_chain(name, _backward(name, _forward(name)), f"M324_ATTN_BWD_NW={nw}")


# ------------------------------------------------------------------------------------------- 4. fp32 parity mode
@pytest.mark.parametrize("name", ["many-keys", "one-tile"])
def test_fp32_parity_mode(name):
    """attn_f32_kernel + m324_attention_delta + m324_attention_bwd on fp32 operands (the case's values, q pre-scaled in fp32): bounds
    without any bf16 rounding (p_bf16 = fwd_p_bf16 = o_bf16 = False, fp32 outputs)."""
    from conftest import vt_layout
    ops = _ops()
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    op = ac.f32_operands(name)
    assert ops._attn_plan(B, H, Lq, Lk, 1, ops.code_of(torch.float32)).startswith("attn_f32_kernel ")
    qs, k, v = op["qs"].to(DEV), op["k"].to(DEV), op["v"].to(DEV)
    out = torch.full((B * Lq, H * 64), NAN, device=DEV)
    lse = torch.full((B, H, Lq), NAN, device=DEV)
    ops.attention(qs, k, vt_layout(op["v"]).to(DEV), out, shared_q=shared, prescaled=True, lse=lse)
    D = ops.attention_delta(out, ac.token_major(op["dO"]).to(DEV), B, H, Lq)
    dQ, dK, dV = ops.attention_bwd(qs, k, v, op["dO"].to(DEV), lse, D, shared_q=shared)
    torch.cuda.synchronize()
    _assert_chain(name, dict(out=out, lse=lse, dQ=dQ, dK=dK, dV=dV), "fp32 parity mode", kind="f32", f32=True)


# ------------------------------------------------------------------------------------------- 5. exact structure
def _items(B, H):
    return [(b, h) for b in range(B) for h in range(H)]


@pytest.mark.parametrize("name", ["pwg", "one-tile"])
def test_zero_gradients_stay_exactly_zero(name):
    """dO = 0: D = 0 and dP = 0, so dQ, dK, dV are exactly 0.  dO non-zero in one query row of one (batch, head) only -- an edge
    query of the first item, then row Lq - 1 of the last item: dQ is exactly 0 in every other row and item, dK and dV in every other
    item (a kernel that reads a neighbour's dO, D or LSE row, or another item's, leaves something there)."""
    inp = ac.inputs(name)
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    fwd = _forward(name)
    got = _backward(name, fwd, dO=torch.zeros_like(inp["dO"]))
    for k in GRADS:
        assert not bool(got[k].float().any()), f"{k} of dO = 0"
    for (b, h), q in (((0, 0), inp["eq"][3]), ((B - 1, H - 1), Lq - 1)):
        assert q in inp["eq"]
        dO = torch.zeros_like(inp["dO"])
        dO[b, h, q] = inp["dO"][b, h, q]
        got = {k: v.float().cpu() for k, v in _backward(name, fwd, dO=dO).items()}
        assert bool(got["dQ"][b, h, q].any()) and bool(got["dK"][b, h].any()) and bool(got["dV"][b, h].any())
        rows = torch.ones(Lq, dtype=torch.bool)
        rows[q] = False
        assert not bool(got["dQ"][b, h, rows].any()), f"dQ of the rows beside ({b}, {h}, {q})"
        for item in _items(B, H):
            if item != (b, h):
                for k in GRADS:
                    assert not bool(got[k][item].any()), f"{k} of item {item}, dO in ({b}, {h}, {q}) only"


# ------------------------------------------------------------------------------------------- 6. non-finite values
def _finite_and_within(name, got, where, what):
    """the elements selected by the boolean masks where[k] (shaped like the output): finite and within the unpoisoned reference's
    bound (the items are independent, so their reference does not change)"""
    ref, bnd = ac.reference(name), ac.bounds(name)
    res = _host(name, got)
    for k, mask in where.items():
        assert bool(torch.isfinite(res[k][mask]).all()), f"{k}: non-finite values outside what depends on the poison ({what})"
        eb.assert_within(res[k][mask], ref[k][mask], bnd[k][mask], f"{k} beside the poison, {name}, {what}")


@pytest.mark.parametrize("poison", ["nan-in-dO", "nan-row-of-K", "inf-in-V"])
@pytest.mark.parametrize("name", ["pwg", "one-tile"])
def test_non_finite_values_stay_where_they_belong(name, poison):
    """One non-finite input in the LAST (batch, head): a NaN in one element of dO (an edge query), a NaN row of K (key Lk - 1, in the
    ragged tile, which the kernels mask by assignment), a +inf in one element of V.  Every gradient of every other item is finite and
    within its bound.  Inside the item, what depends on the value is non-finite in every element:
      dO[q, d]   dQ row q, all of dK (through D_q and dP_q), column d of dV;  the other rows of dQ and columns of dV do not depend
                 on it and stay within their bounds
      K[k, :]    out, lse (every query sees the key), hence all of dQ, dK, dV
      V[k, d]    out column d, hence D of every query, hence all of dQ and dK;  dV = P^T dO does not depend on V: finite, in bound
    These are ordinary operands through ordinary launches."""
    inp = ac.inputs(name)
    B, H, Lq, Lk, shared, _ = ac.CASES[name]
    b, h = B - 1, H - 1
    q, d = inp["eq"][4], 37
    k, v, dO = inp["k"].clone(), inp["v"].clone(), inp["dO"].clone()
    if poison == "nan-in-dO":
        dO[b, h, q, d] = NAN
    elif poison == "nan-row-of-K":
        k[b, h, Lk - 1] = NAN
    else:
        v[b, h, Lk - 1, d] = float("inf")
    got = _backward(name, _forward(name, k=k, v=v), dO=dO)
    res = {key: t.float().cpu() for key, t in got.items()}
    res["out"] = res["out"].reshape(B, Lq, H, 64).permute(0, 2, 1, 3)                # head-major view
    dep = {key: torch.zeros_like(res[key], dtype=torch.bool) for key in OUTS}        # what depends on the poisoned value
    if poison == "nan-in-dO":
        dep["dQ"][b, h, q] = True
        dep["dK"][b, h] = True
        dep["dV"][b, h, :, d] = True
    elif poison == "nan-row-of-K":
        for key in OUTS:
            dep[key][b, h] = True
    else:
        dep["out"][b, h, :, d] = True
        dep["dQ"][b, h] = True
        dep["dK"][b, h] = True
    for key in OUTS:
        assert not bool(torch.isfinite(res[key][dep[key]]).any()), f"{key}: finite values where {poison} must show"
    dep["out"] = ac.token_major(dep["out"])
    _finite_and_within(name, got, {key: ~dep[key] for key in OUTS}, poison)
