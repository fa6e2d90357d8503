"""Inputs, case table and CPU model of the attention-backward tests (tests/test_attention_backward_cpu.py, tests/test_attention_backward_gpu.py).

The chain under test is backward.self_attn_block_bwd's: m324_qkv_split (train outputs) -> m324_attention with a saved LSE ->
m324_attention_delta -> m324_attention_bwd_mfma.  Uniform random operands give every key about 1 / sqrt(Lk) of a dQ row, so a kernel
that loses the last key of the ragged tile, or the last query row, stays inside error_bounds.attention_backward.  edge_inputs() puts
the weight where these kernels break: on the rows and keys at tile, wave and workgroup edges.

  edge queries   rows {0, 31, 32, 63, 64, 127, 128, 255, 256, first row of the last 64-row tile, Lq - 1} that exist
  edge keys      {0, 31, 32, 63, 64, 127, 128, first key of the last 64-key tile, Lk - 1} that exist

Every edge query is given two edge keys (pair_table).  The edge keys of a (batch, head) are then rewritten as THE combination of the
edge-query directions whose natural-log scores with the edge queries are exactly S0 +- DELTA for a query's own pair and 0 for the
other edge queries: K_e^T = pinv(Q_e) T / scale, the minimum-norm solution, which lies in the span of the edge queries.  The
directions are random in 64 dimensions, i.e. nearly orthogonal, so this is nearly (8 S0 / |q|) times the sum of the unit directions a
key serves; solving instead of summing removes the q_i . q_j cross terms (+- 3 nats at this scale), which would otherwise leave most
queries with ONE dominant key.  The rest of a row's keys score N(0, 1.44^2), all of them together about e^8 against the pair's
2 e^12: each key of a pair has a probability between 0.2 and 0.8, and dS = p (dP - D) of the pair is as large as it can be.

model_kernel() is the kernels' arithmetic in fp32 torch on the CPU with the roundings where attention.hip puts them, and switches for
deliberate mistakes.  The switches change the model only, never a device kernel: they show, on a machine without a GPU, that the
inputs would expose such a mistake through error_bounds.attention_backward.
"""
import functools
import math

import torch

import error_bounds as eb

BF = torch.bfloat16
SCALE = 64 ** -0.5
LOG2E = 1.4426950408889634
Q_PRESCALE = SCALE * LOG2E           # motion324_amd.ops.Q_PRESCALE (this module is imported without the package)
LN2 = math.log(2.0)
S0 = 12.0                            # natural-log score of an edge query with each key of its pair ...
DELTA = 0.3                          # ... +- this: probabilities 0.65 / 0.35, alternating which key of the pair leads
SCORE_RANGE = 60.0                   # max |log2-domain score| the inputs may reach (the bounded-scores forward vouches for 64)

PLAIN3 = "attn_bf16_kernel<true, 1, 4, false, 3>"
PLAIN2 = "attn_bf16_kernel<true, 1, 4, false, 2>"
PLAIN1 = "attn_bf16_kernel<true, 1, 4, false, 1>"
#        case           B  H  Lq    Lk    shared  forward kernel of the default call
CASES = {"pwg":         (1, 2, 2100, 1090, False, "attn_pwg_kernel"),
         "many-keys":   (2, 2, 70,   1090, False, PLAIN3),                      # Lk > 1024: three LDS stages
         "frames":      (4, 2, 513,  37,   True,  "attn_frames_kernel<2, true>"),
         "one-tile":    (2, 2, 100,  37,   False, PLAIN1),
         "tiles-exact": (1, 2, 128,  1024, False, PLAIN2),                      # per-frame form, no ragged tile at all
         "one-query":   (2, 1, 1,    130,  False, PLAIN2),
         "one-key":     (2, 1, 130,  1,    False, PLAIN1),
         "one-one":     (1, 1, 1,    1,    False, PLAIN1)}
# other forwards of a case: variant -> (tunable or None, kwargs of ops.attention, kernel)
VARIANTS = {"pwg": {"bounded": (None, dict(bounded=True), "attn_pwg_bounded_kernel"),
                    "pwg-off": (("M324_ATTN_PWG", 0), {}, "attn_bf16_kernel<true, 1, 8, false, 3>")}}


def edge_queries(Lq):
    return sorted({r for r in (0, 31, 32, 63, 64, 127, 128, 255, 256, (Lq - 1) // 64 * 64, Lq - 1) if r < Lq})


def edge_keys(Lk):
    return sorted({r for r in (0, 31, 32, 63, 64, 127, 128, (Lk - 1) // 64 * 64, Lk - 1) if r < Lk})


def degenerate(Lq, Lk):
    return Lq == 1 or Lk == 1


def pair_table(Lq, Lk):
    """{edge query: (key, key)}: two different edge keys for every edge query, every edge key in some pair (the degenerate shapes
    excepted).  With at least as many queries as keys the pairs walk the keys with a stride that changes every lap, so that the
    queries that share a key do not share its partner."""
    eq, ek = edge_queries(Lq), edge_keys(Lk)
    nq, nk = len(eq), len(ek)
    if nk < 2:
        return {}
    out = {}
    for i, q in enumerate(eq):
        if nq >= nk:
            a, b = i % nk, (i + 1 + (i // nk) % (nk - 1)) % nk
        else:
            a, b = (2 * i) % nk, (2 * i + 1) % nk
        out[q] = (ek[a], ek[b])
    if not degenerate(Lq, Lk):
        assert {k for p in out.values() for k in p} == set(ek), (Lq, Lk)
    assert all(a != b for a, b in out.values())
    return out


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def edge_inputs(B, H, Lq, Lk, shared, seed=0):
    """The operands of one case, head-major, as the values the kernels read: q_src [Bq, H, Lq, 64] bf16 (the q that goes into
    m324_qkv_split), qs = bf16(q_src * Q_PRESCALE) (what it stores), q_hat = qs / Q_PRESCALE in fp64 (the unscaled q the gradient is
    taken against), k, v, dO bf16.  Asserts the dominance rule and the score range."""
    Bq = 1 if shared else B
    q_src = (_randn((Bq, H, Lq, 64), seed + 1) * 1.2).to(BF)
    qs = (q_src.float() * torch.tensor(Q_PRESCALE, dtype=torch.float32)).to(BF)
    q_hat = qs.double() / Q_PRESCALE
    k = (_randn((B, H, Lk, 64), seed + 2) * 1.2).to(BF)
    v = _randn((B, H, Lk, 64), seed + 3).to(BF)
    dO = _randn((B, H, Lq, 64), seed + 4).to(BF)
    eq, ek, pairs = edge_queries(Lq), edge_keys(Lk), pair_table(Lq, Lk)
    if pairs:
        T = torch.zeros((len(eq), len(ek)), dtype=torch.float64)
        for i, q in enumerate(eq):
            a, b = pairs[q]
            d = DELTA if i % 2 == 0 else -DELTA
            T[i, ek.index(a)], T[i, ek.index(b)] = S0 + d, S0 - d
        for b in range(B):
            for h in range(H):
                Qe = q_hat[b if not shared else 0, h, eq]                        # [nq, 64]
                k[b, h, ek] = (torch.linalg.pinv(Qe) @ (T / SCALE)).T.to(BF)      # [nk, 64]: Qe Ke^T scale = T
    inp = dict(B=B, H=H, Lq=Lq, Lk=Lk, shared=shared, q_src=q_src, qs=qs, q_hat=q_hat, k=k, v=v, dO=dO, eq=eq, ek=ek, pairs=pairs)
    check_edge_structure(inp)
    return inp


def check_edge_structure(inp):
    """The conditions the inputs are built for, from the operand values alone (fp64): score range; for every (batch, head) and every
    edge query its two largest probabilities belong to its pair and lie in [0.2, 0.8]."""
    B, shared = inp["B"], inp["shared"]
    s = torch.einsum("bhqd,bhkd->bhqk", inp["q_hat"].expand(B, -1, -1, -1), inp["k"].double()) * SCALE
    top = float(s.abs().max()) * LOG2E
    assert top < SCORE_RANGE, f"max |log2-domain score| {top:.1f}"
    lo, hi = 1.0, 0.0
    if inp["pairs"]:
        p = torch.softmax(s[:, :, inp["eq"]], dim=-1)                            # [B, H, nq, Lk]
        for i, q in enumerate(inp["eq"]):
            best = p[:, :, i].topk(2, dim=-1)
            want = torch.tensor(sorted(inp["pairs"][q]))
            assert bool((best.indices.sort(-1).values == want).all()), f"query {q}: dominant keys are not its pair {inp['pairs'][q]}"
            lo, hi = min(lo, float(best.values.min())), max(hi, float(best.values.max()))
        assert 0.2 <= lo and hi <= 0.8, (lo, hi)
    return top, lo, hi


@functools.lru_cache(maxsize=None)
def inputs(name):
    B, H, Lq, Lk, shared, _ = CASES[name]
    return edge_inputs(B, H, Lq, Lk, shared, seed=100 * (1 + list(CASES).index(name)))


def token_major(t):
    """head-major [B, H, L, 64] -> token-major [B * L, H * 64] (the layout of m324_qkv_split's sources and of O)"""
    B, H, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, H * 64).contiguous()


# ------------------------------------------------------------------------------------------- fp64 reference and bounds (once per case)
def _autograd(q_hat, k, v, dO):
    B, H, Lq = k.shape[0], k.shape[1], q_hat.shape[2]
    qh = q_hat.double().clone().requires_grad_(True)
    kd, vd = k.double().requires_grad_(True), v.double().requires_grad_(True)
    s = torch.einsum("bhqd,bhkd->bhqk", qh.expand(B, -1, -1, -1), kd) * SCALE
    o = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(s, -1), vd)
    o.backward(dO.double())
    return dict(out=token_major(o.detach()), lse=torch.logsumexp(s.detach(), -1) / LN2, dQ=qh.grad, dK=kd.grad, dV=vd.grad)


@functools.lru_cache(maxsize=None)
def reference(name, f32=False):
    """fp64 autograd of O = softmax(q_hat k^T / 8) v on the stored operands: out (token-major), lse (log2 domain), dQ (summed over
    the batches when the queries are shared), dK, dV.  f32=True: the fp32 parity mode's operands (f32_operands)."""
    inp = inputs(name)
    if f32:
        op = f32_operands(name)
        return _autograd(op["q_hat"], op["k"], op["v"], op["dO"])
    return _autograd(inp["q_hat"], inp["k"], inp["v"], inp["dO"])


@functools.lru_cache(maxsize=None)
def bounds(name, kind="mfma"):
    """error_bounds of the chain, keyed like reference(): kind "mfma" (bf16 forward, m324_attention_bwd_mfma), "fp32-arithmetic"
    (bf16 forward, m324_attention_bwd on bf16 operands: neither P nor dS rounded) or "f32" (attn_f32_kernel + m324_attention_bwd in fp32)."""
    inp = inputs(name)
    if kind == "f32":
        op = f32_operands(name)
        out, lse = eb.attention_and_lse(op["qs"], op["k"], op["v"], LN2, p_bf16=False, out_dtype=torch.float32)
        dq, dk, dv = eb.attention_backward(op["q_hat"], op["k"], op["v"], op["dO"], SCALE, p_bf16=False, fwd_p_bf16=False, o_bf16=False,
                                           out_dtype=torch.float32, shared=inp["shared"])
    else:
        out, lse = eb.attention_and_lse(inp["qs"], inp["k"], inp["v"], LN2)
        dq, dk, dv = eb.attention_backward(inp["q_hat"], inp["k"], inp["v"], inp["dO"], SCALE, p_bf16=kind == "mfma", shared=inp["shared"])
    return dict(out=out, lse=lse, dQ=dq, dK=dk, dV=dv)


@functools.lru_cache(maxsize=None)
def f32_operands(name):
    """The case's operands for the fp32 kernels: the same q_src, k, v, dO values in fp32, qs = q_src * Q_PRESCALE rounded to fp32 only"""
    inp = inputs(name)
    qs = inp["q_src"].float() * torch.tensor(Q_PRESCALE, dtype=torch.float32)
    return dict(qs=qs, q_hat=qs.double() / Q_PRESCALE, k=inp["k"].float(), v=inp["v"].float(), dO=inp["dO"].float())


def ratios(got, name, kind="mfma", f32=False, keys=("out", "lse", "dQ", "dK", "dV")):
    """worst err / bound per output, without asserting"""
    ref, bnd = reference(name, f32), bounds(name, kind)
    return {k: eb.worst_ratio(got[k], ref[k], bnd[k]) for k in keys}


# ------------------------------------------------------------------------------------------- the model kernel
def _r16(t):
    return t.to(BF).float()


_FWD = {}


def _model_forward(inp):
    """attn_bf16_kernel / attn_pwg_kernel / attn_frames_kernel: log2-domain scores of the stored qs, fp32 row sums of the UNROUNDED
    probabilities, P rounded to bf16 in front of P V, O stored as bf16, lse = m + log2(l)."""
    key = id(inp)
    if key not in _FWD:
        qs, k, v = inp["qs"].float(), inp["k"].float(), inp["v"].float()
        s2 = torch.einsum("bhqd,bhkd->bhqk", qs.expand(inp["B"], -1, -1, -1), k)
        m = s2.max(-1, keepdim=True).values
        p = torch.exp2(s2 - m)
        l = p.sum(-1, keepdim=True)
        o = _r16(torch.einsum("bhqk,bhkd->bhqd", _r16(p), v) / l)
        _FWD[key] = (s2, o, (m + torch.log2(l))[..., 0], torch.einsum("bhqd,bhkd->bhqk", inp["dO"].float(), v))
    return _FWD[key]


def swap_allowed(Lk):
    """the 16-key group that holds key Lk - 1 has a valid key in its quarter 1 or 2"""
    return Lk >= 2 and (Lk - 1) % 16 >= 4


def model_kernel(inp, *, drop_key=None, drop_query=None, no_ln2=False, neighbour_lse=False, d_from_other_head=False,
                 swap_quarters=False):
    """The chain in fp32 torch with the kernels' roundings (attention.hip, backward.hip): D = rowsum(stored bf16 O * dO) in fp32;
    P = exp2(qs . k - lse), dS = P (dO . v - D) in fp32; the dQ kernel rounds dS to bf16 in front of dS K and stores
    bf16(scale * acc); the dK / dV kernel rounds P and dS to bf16 in front of P^T dO and dS^T qs and stores bf16(acc) and
    bf16(ln 2 * acc).  Returns out (token-major), lse, dQ (summed over the batches when shared), dK, dV.

    Deliberate mistakes (the model's, never the device kernels'):
      drop_key=k          the dQ kernel masks key k (as it masks the keys past Lk)
      drop_query=q        the dK / dV kernel masks query q (as it masks the queries past Lq)
      no_ln2              dK without its ln 2
      neighbour_lse       row q is recomputed with the LSE of row q + 1
      d_from_other_head   D taken from the next head of the same batch
      swap_quarters       Kt of the dQ kernel with key quarters 1 and 2 exchanged inside the 16-key group that holds key Lk - 1"""
    B, H, Lq, Lk = inp["B"], inp["H"], inp["Lq"], inp["Lk"]
    s2, o, lse, dP = _model_forward(inp)
    qs, k, dO = inp["qs"].float().expand(B, -1, -1, -1), inp["k"].float(), inp["dO"].float()
    D = (o * dO).sum(-1)
    lse_b = lse
    if d_from_other_head:
        D = D.roll(1, dims=1)
    if neighbour_lse:
        lse_b = lse.roll(-1, dims=2)
    P = torch.exp2(s2 - lse_b[..., None])
    dS = P * (dP - D[..., None])
    # dQ kernel (lane = query, walks the keys)
    dSq = _r16(dS)
    if drop_key is not None:
        dSq[..., drop_key] = 0.0
    kq = k
    if swap_quarters:
        Lkp = (Lk + 15) // 16 * 16
        g0 = (Lk - 1) // 16 * 16
        perm = torch.arange(Lkp)
        perm[g0 + 4:g0 + 8], perm[g0 + 8:g0 + 12] = torch.arange(g0 + 8, g0 + 12), torch.arange(g0 + 4, g0 + 8)
        kq = torch.nn.functional.pad(k, (0, 0, 0, Lkp - Lk))[:, :, perm]
        dSq = torch.nn.functional.pad(dSq, (0, Lkp - Lk))
    dQ = _r16(torch.einsum("bhqk,bhkd->bhqd", dSq, kq) * torch.tensor(SCALE, dtype=torch.float32))
    # dK / dV kernel (lane = key, walks the queries)
    Pk, dSk = _r16(P), _r16(dS)
    if drop_query is not None:
        Pk[:, :, drop_query] = 0.0
        dSk[:, :, drop_query] = 0.0
    dV = _r16(torch.einsum("bhqk,bhqd->bhkd", Pk, dO))
    dK = _r16(torch.einsum("bhqk,bhqd->bhkd", dSk, qs) * (1.0 if no_ln2 else torch.tensor(LN2, dtype=torch.float32)))
    dQ = dQ.double().sum(0, keepdim=True) if inp["shared"] else dQ
    return dict(out=token_major(o), lse=lse, dQ=dQ, dK=dK, dV=dV)


def mistakes(inp):
    """(label, kwargs of model_kernel) of every planted mistake the case's shape allows.  Lq = 1 or Lk = 1 (exempt from the
    dominance rule): only the mistakes that need no dominant pair -- with one key P = 1 and dS = 0 whatever the kernel does."""
    H, Lq, Lk = inp["H"], inp["Lq"], inp["Lk"]
    out = []
    paired = sorted({k for p in inp["pairs"].values() for k in p})
    out += [(f"drop key {k} from dQ", dict(drop_key=k)) for k in (inp["ek"] if not degenerate(Lq, Lk) else paired)]
    if Lk >= 2:
        out += [(f"drop query {q} from dK, dV", dict(drop_query=q)) for q in inp["eq"]]
        out.append(("dK without ln 2", dict(no_ln2=True)))
    if Lq >= 2:
        out.append(("LSE of the next query", dict(neighbour_lse=True)))
    if H >= 2:
        out.append(("D of another head", dict(d_from_other_head=True)))
    if swap_allowed(Lk):
        out.append(("key quarters 1 and 2 of Kt exchanged", dict(swap_quarters=True)))
    return out
