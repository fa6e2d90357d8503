"""What motion324_amd.ops hands to libm324, call by call: tests/golden/ops_calls.json.

ops.py is the one place where tensors become raw pointers, leading dimensions and flag words for the C ABI; an argument-order slip
in a call of twenty arguments shows only on a GPU machine.  This script runs the wrappers on small CPU tensors with the library,
the stream and the device test replaced by recorders -- no libm324, no device -- and writes down, per case:
  calls   every C-ABI call in order: [entry point, arguments].  A GemmArgs or a ColsumItem array is expanded into its non-zero
          fields; a pointer becomes [storage label, byte offset], the labels s0, s1, ... numbered in the order the storages first
          appear in these argument lists (so the order in which a wrapper happens to evaluate its pointers does not count);
  spans   the (class, FLOPs, bytes, tag) rows bench.py's roofline and the committed profiles are keyed by, tags switched on;
  wrote   which of the case's named tensors had their version counter raised (ops._wrote);
  ret     dtype, shape, strides and storage of what the wrapper returned;
  error   the M324Error text of a call that must be refused.
tests/test_ops_calls_cpu.py runs the same cases on the tree of the day and compares exactly.

The fixture is written from the PARENT of a change to ops.py, never from the code under test:

    git worktree add ../parent HEAD~1
    python tests/golden/make_ops_calls.py --repo ../parent            writes tests/golden/ops_calls.json
    python tests/golden/make_ops_calls.py --stdout                    prints what this tree does instead

so the cases use only names both sides have (qkv_heads travels as a plain tuple).  EXPECTED holds the differences a change
intends, patched into the parent's record in main() where everybody can see them."""
import ctypes as C
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ops_calls.json")

# Intended differences from the parent's record.  "One parser for qkv_heads": gemm(qkv_heads=...) now marks the head-major outputs
# as written, as gemm_mx always did.  case -> names added to its "wrote".
EXPECTED = {
    "gemm heads q k v, ln fold": ["K", "Q", "V"],
    "gemm heads transposed V by shape": ["K", "Q", "V"],
    "gemm heads explicit vt": ["K", "V"],
    "gemm heads explicit row-major V": ["K", "V"],
    "gemm heads q only": ["Q"],
    "gemm heads k v only": ["K", "V"],
    "gemm heads deferred pair": ["K", "Q", "V"],
    "gemm heads deferred pair, unsupported": ["K", "Q", "V"],
}

F32, BF16, U8, F64 = torch.float32, torch.bfloat16, torch.uint8, torch.float64
ops = L = None                      # the modules under the recorders: bound by record()
CASES = []


class _Dev(torch.Tensor):
    """a CPU tensor that answers is_cuda: for the two wrappers that ask the tensor itself"""
    is_cuda = property(lambda self: True)


class Tensors:
    """the named tensors of one case: t("a", 8, 16) makes (once) a zero tensor the record can speak of by name"""

    def __init__(self):
        self.named = {}

    def __call__(self, name, *shape, dtype=F32, dev=False):
        if name not in self.named:
            x = torch.zeros(shape, dtype=dtype)
            self.named[name] = x.as_subclass(_Dev) if dev else x
        return self.named[name]

    def mx(self, name, rows, K):
        m = ops.mx_empty(rows, K, "cpu")
        self.named[name + ".q"], self.named[name + ".s"] = m.q, m.s
        return m


def case(name):
    def add(fn):
        CASES.append((name, fn))
        return fn
    return add


class Recorder:
    def __init__(self):
        self.calls, self.spans, self.seen, self.pair_rc = [], [], [], 0

    def lib(self):
        rec = self

        class Lib:
            pass
        lib = Lib()
        for name in L.SIGNATURES:
            setattr(lib, name, lambda *args, _n=name: rec.call(_n, args))
        return lib

    def call(self, name, args):
        # structures are copied as they are at the call; pointers get their labels when the case is over
        args = tuple(type(a._obj).from_buffer_copy(a._obj) if hasattr(a, "_obj") else
                     type(a).from_buffer_copy(a) if isinstance(a, C.Array) and isinstance(a[0], C.Structure) else a for a in args)
        self.calls.append((name, args))
        if name.endswith("_plan"):                                  # the two text queries: a kernel name for the tag, schedule 0
            args[-2].value = b"plan"
            return 0
        return self.pair_rc if name == "m324_gemm_pair" else 0

    def p(self, t):
        if t is None:
            return None
        self.seen.append(t)                                         # alive until the case ends: no address is used twice
        return t.data_ptr()

    def span(self, cls, flops, nbytes=0.0, tag=""):
        rec = self

        class Span:
            def __enter__(self):
                self.row = [cls, flops, nbytes, tag]
                rec.spans.append(self.row)
                return self

            def cancel(self):
                self.row.append("cancelled")

            def __exit__(self, *exc):
                return False
        return Span()


def _storages(tensors):
    out = []
    for t in tensors:
        s = t.untyped_storage()
        out.append((s.data_ptr(), s.nbytes(), t))
    return out


def _normalise(rec, named, ret, error):
    stores = _storages(list(named.values()) + rec.seen)
    labels = {}

    def ptr(addr):
        if addr is None or addr == 0:
            return None
        for base, n, _t in stores:
            if base <= addr < base + max(n, 1):
                return [labels.setdefault(base, f"s{len(labels)}"), addr - base]
        raise AssertionError(f"pointer {addr:#x} belongs to no tensor the case or the wrapper showed")

    def struct(s):
        out = {}
        for field, ctype in s._fields_:
            v = getattr(s, field)
            if ctype is C.c_void_p:
                v = ptr(v)
            if v:
                out[field] = v
        return out

    def arg(a, ctype):
        if isinstance(a, C.Array) and isinstance(a[0], C.Structure):
            return [struct(item) for item in a]
        if isinstance(a, C.Structure):                              # what byref(...) pointed to
            return struct(a)
        if isinstance(a, C.Array):
            return "buffer"
        return ptr(a) if ctype is C.c_void_p else a

    for name, args in rec.calls:
        assert len(args) == len(L.SIGNATURES[name]), f"{name}: {len(args)} arguments for {len(L.SIGNATURES[name])} parameters"
    calls = [[name, [arg(a, ct) for a, ct in zip(args, L.SIGNATURES[name])]] for name, args in rec.calls]

    def describe(v):
        if isinstance(v, torch.Tensor):
            s = v.untyped_storage()
            known = labels.get(s.data_ptr())
            return [str(v.dtype).replace("torch.", ""), list(v.shape), list(v.stride()), known or "new", v.data_ptr() - s.data_ptr()]
        if isinstance(v, dict):
            return {k: describe(v[k]) for k in sorted(v)}
        if isinstance(v, (tuple, list)):
            return [describe(x) for x in v]
        if hasattr(v, "t") and isinstance(v.t, torch.Tensor):       # ops.Rows
            return {"Rows": describe(v.t)}
        return v
    entry = {"calls": calls, "spans": rec.spans}
    if error is not None:
        entry["error"] = error
    else:
        entry["ret"] = describe(ret)
    return entry


def record(ops_module, lib_module):
    """{case name: entry} of ops_module (motion324_amd.ops) over lib_module (motion324_amd.lib); both are left as they were"""
    global ops, L
    ops, L = ops_module, lib_module
    saved = (L.load, ops._p, ops._stream, ops.span, ops._timing, ops.DEFER_COLSUM)
    out = {}
    try:
        for name, fn in CASES:
            rec, t = Recorder(), Tensors()
            lib = rec.lib()
            L.load, ops._p, ops._stream, ops.span, ops._timing = (lambda: lib), rec.p, (lambda: 0), rec.span, (lambda: True)
            ops.COLSUMS.clear()
            ret = error = None
            try:
                ret = fn(t, rec)
            except L.M324Error as e:
                error = str(e)
            finally:
                ops.DEFER_COLSUM = saved[5]
            assert name not in out, name
            out[name] = _normalise(rec, t.named, ret, error)
            out[name]["wrote"] = sorted(nm for nm, x in t.named.items() if x._version > 0)      # a new tensor starts at version 0
    finally:
        L.load, ops._p, ops._stream, ops.span, ops._timing, ops.DEFER_COLSUM = saved
        ops.COLSUMS.clear()
    return json.loads(json.dumps(out))


# ------------------------------------------------------------------------------------------------------------------ gemm
def _abw(t, M=8, N=12, K=16, dtype=BF16):
    return t("a", M, K, dtype=dtype), t("w", N, K, dtype=dtype)


@case("gemm f32 bias gelu gamma")
def _(t, rec):
    return ops.gemm(*_abw(t, dtype=F32), t("out", 8, 12), bias=t("bias", 12), act=L.ACT_GELU, gamma=t("gamma", 12))


@case("gemm bf16 plain")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12, dtype=BF16))


@case("gemm bf16 strided operands")
def _(t, rec):
    return ops.gemm(t("a", 8, 24, dtype=BF16)[:, 8:], t("w", 12, 20, dtype=BF16)[:, :16], t("out", 9, 16, dtype=BF16)[1:, 2:14])


@case("gemm fp32 residual res_rows")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), bias=t("bias", 12), residual=t("res", 4, 12), res_rows=4)


@case("gemm fp32 stream in place")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), gamma=t("gamma", 12), residual=t("out", 8, 12))


@case("gemm bf16 residual in place")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12, dtype=BF16), residual=t("out", 8, 12, dtype=BF16))


@case("gemm row_map")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 16, 12), row_map=(2, 4, 1), residual=t("out", 16, 12))


for _kw in ("preact_out", "gelu_grad_of", "gelu_grad_out", "mul_by"):
    @case("gemm aux " + _kw)
    def _(t, rec, _kw=_kw):
        return ops.gemm(*_abw(t), t("out", 8, 12, dtype=BF16), act=L.ACT_GELU if "out" in _kw else L.ACT_NONE,
                        **{_kw: t("aux", 8, 14, dtype=BF16)})


@case("gemm ln merged")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12, dtype=BF16), bias=t("bias", 12), ln=(t("rowstat", 8, 2), t("colsum", 12)))


@case("gemm ln unmerged")
def _(t, rec):
    return ops.gemm(*_abw(t, K=128), t("out", 8, 12, dtype=BF16), act=L.ACT_GELU, ln=(t("part", 2, 8, 2), t("colsum", 12), 1e-5))


@case("gemm stats_out copy_out")
def _(t, rec):
    return ops.gemm(*_abw(t, N=128), t("out", 8, 128), residual=t("out", 8, 128), stats_out=t("stats", 2, 8, 2),
                    copy_out=t("copy", 8, 128, dtype=BF16))


@case("gemm in_rows")
def _(t, rec):
    return ops.gemm(*_abw(t, M=16, N=64), t("out", 8, 64), residual=t("res", 16, 64), stats_out=t("stats", 1, 8, 2),
                    copy_out=t("copy", 8, 64, dtype=BF16), in_rows=(2, 4, 1))


@case("gemm n3")
def _(t, rec):
    return ops.gemm(*_abw(t, N=256), None, bias=t("bias", 256), act=L.ACT_GELU, n3=(t("w3", 3, 256), t("part", 4, 8, 3)))


def _heads(t, B, Lh, H=2, vshape=None, q=True, k=True, v=True):
    Q = t("Q", B, H, Lh, 64, dtype=BF16) if q else None
    K = t("K", B, H, Lh, 64, dtype=BF16) if k else None
    V = t("V", *(vshape or (B, H, Lh, 64)), dtype=BF16) if v else None
    return Q, K, V, (t("qw", 64) if q else None), (t("kw", 64) if k else None)


@case("gemm heads q k v, ln fold")
def _(t, rec):
    a, w = _abw(t, M=8, N=384)
    return ops.gemm(a, w, None, bias=t("bias", 384), qkv_heads=_heads(t, 2, 4) + (1e-5, ops.Q_PRESCALE, 4, 2),
                    ln=(t("rowstat", 8, 2), t("colsum", 384)))


@case("gemm heads transposed V by shape")
def _(t, rec):
    a, w = _abw(t, M=128, N=384)
    return ops.gemm(a, w, None, qkv_heads=_heads(t, 1, 128, vshape=(1, 2, 64, 128)) + (1e-5, ops.Q_PRESCALE, 128, 2))


@case("gemm heads explicit vt")
def _(t, rec):
    a, w = _abw(t, M=64, N=256)
    return ops.gemm(a, w, None, bias=t("bias", 256), qkv_heads=_heads(t, 1, 64, q=False) + (1e-5, 1.0, 64, 2, True))


@case("gemm heads explicit row-major V")
def _(t, rec):
    a, w = _abw(t, M=64, N=256)
    return ops.gemm(a, w, None, qkv_heads=_heads(t, 1, 64, q=False) + (1e-5, 1.0, 64, 2, False))


@case("gemm heads q only")
def _(t, rec):
    a, w = _abw(t, M=8, N=128)
    return ops.gemm(a, w, None, bias=t("bias", 128), qkv_heads=_heads(t, 2, 4, k=False, v=False) + (1e-5, ops.Q_PRESCALE, 4, 2))


@case("gemm heads k v only")
def _(t, rec):
    a, w = _abw(t, M=8, N=256)
    return ops.gemm(a, w, None, qkv_heads=_heads(t, 2, 4, q=False) + (1e-5, 1.0, 4, 2))


def _pair(t, rec, rc):
    rec.pair_rc = rc
    pair = []
    Q, _, _, qw, _ = _heads(t, 1, 8, k=False, v=False)
    K, V, kw = t("K", 1, 2, 64, 64, dtype=BF16), t("V", 1, 2, 64, 64, dtype=BF16), t("kw", 64)
    r0 = ops.gemm(t("a", 8, 16, dtype=BF16), t("w", 128, 16, dtype=BF16), None, bias=t("bq", 128),
                  qkv_heads=(Q, None, None, qw, None, 1e-5, ops.Q_PRESCALE, 8, 2), defer=pair)
    r1 = ops.gemm(t("kv", 64, 16, dtype=BF16), t("wkv", 256, 16, dtype=BF16), None, bias=t("bkv", 256),
                  qkv_heads=(None, K, V, None, kw, 1e-5, 1.0, 64, 2, True), defer=pair)
    shape = [(type(p).__name__, len(p), type(p[0]).__name__, p[1], p[2], p[3], len(p[4])) for p in pair]
    ops.gemm_pair(pair)
    return r0, r1, shape, len(pair)


@case("gemm heads deferred pair")
def _(t, rec):
    return _pair(t, rec, 0)


@case("gemm heads deferred pair, unsupported")
def _(t, rec):
    return _pair(t, rec, L.ERR_UNSUPPORTED)


@case("gemm_splitk remainder")
def _(t, rec):
    return ops.gemm_splitk(t("a", 8, 200, dtype=BF16), t("w", 12, 200, dtype=BF16), 2)


@case("gemm_splitk one slice")
def _(t, rec):
    return ops.gemm_splitk(t("a", 8, 40), t("w", 12, 40), 4)


# --------------------------------------------------------------------------------------------------------------- gemm_mx
@case("gemm_mx bf16 out bias")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 8, 64), t.mx("w", 32, 64), t("out", 8, 40, dtype=BF16)[:, :32], bias=t("bias", 32))


@case("gemm_mx heads")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 8, 64), t.mx("w", 384, 64), None, bias=t("bias", 384),
                       qkv_heads=_heads(t, 2, 4) + (1e-5, ops.Q_PRESCALE, 4, 2))


@case("gemm_mx heads transposed V by shape")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 128, 64), t.mx("w", 384, 64), None,
                       qkv_heads=_heads(t, 1, 128, vshape=(1, 2, 64, 128)) + (1e-5, ops.Q_PRESCALE, 128, 2))


@case("gemm_mx fp32 stream")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 8, 64), t.mx("w", 32, 64), t("out", 8, 32), bias=t("bias", 32), gamma=t("gamma", 32),
                       residual=t("out", 8, 32))


@case("gemm_mx mx out gelu")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 8, 64), t.mx("w", 32, 64), t.mx("out", 8, 32), bias=t("bias", 32), act=L.ACT_GELU)


# --------------------------------------------------------------------------------------------------------------- gemm_tn
@case("gemm_tn direct")
def _(t, rec):
    return ops.gemm_tn(t("x", 40, 8, dtype=BF16), t("y", 40, 12, dtype=BF16), out=t("out", 8, 12))


@case("gemm_tn one slice, no out")
def _(t, rec):
    return ops.gemm_tn(t("x", 40, 8, dtype=BF16), t("y", 40, 12, dtype=BF16))


@case("gemm_tn sliced")
def _(t, rec):
    return ops.gemm_tn(t("x", 200, 8, dtype=BF16), t("y", 200, 12, dtype=BF16), slices=2)


@case("gemm_tn sliced into out")
def _(t, rec):
    return ops.gemm_tn(t("x", 200, 8, dtype=BF16), t("y", 200, 12, dtype=BF16), slices=3, out=t("out", 8, 12))


@case("gemm_tn accumulate, one slice")
def _(t, rec):
    return ops.gemm_tn(t("x", 40, 8, dtype=BF16), t("y", 40, 12, dtype=BF16), out=t("out", 8, 12), accumulate=True)


@case("gemm_tn deferred column sums, flush")
def _(t, rec):
    ops.DEFER_COLSUM = True
    x, y = t("x", 200, 8, dtype=BF16), t("y", 200, 12, dtype=BF16)
    r0 = ops.gemm_tn(x, y, slices=2, out=t("out", 8, 12))
    r1 = ops.gemm_tn(x, y, slices=2, out=t("out", 8, 12), accumulate=True)
    r2 = ops.gemm_tn(t("x2", 40, 4, dtype=BF16), t("y2", 40, 4, dtype=BF16), out=t("out2", 4, 4), accumulate=True)
    n = len(rec.calls)
    ops.COLSUMS.flush()
    return r0, r1, r2, n


@case("gemm_tn direct flushes a pending sum")
def _(t, rec):
    ops.DEFER_COLSUM = True
    x, y = t("x", 200, 8, dtype=BF16), t("y", 200, 12, dtype=BF16)
    ops.gemm_tn(x, y, slices=2, out=t("out", 8, 12))
    return ops.gemm_tn(x[:40], y[:40], out=t("out", 8, 12))


# ------------------------------------------------------------------------------------------------ row kernels, MX, q|k|v
@case("layernorm f32 to bf16, row_map")
def _(t, rec):
    return ops.layernorm(t("x", 16, 16), t("w", 16), t("b", 16), 1e-5, t("out", 8, 16, dtype=BF16), row_map=(2, 4, 1))


@case("layernorm bf16 in, rows")
def _(t, rec):
    return ops.layernorm(t("x", 8, 24, dtype=BF16)[:, :16], t("w", 16), None, 1e-6, t("out", 8, 16, dtype=BF16), rows=5)


@case("layernorm f32 to f32")
def _(t, rec):
    return ops.layernorm(t("x", 8, 16), t("w", 16), t("b", 16), 1e-5, t("out", 8, 16))


@case("layernorm_pair")
def _(t, rec):
    return ops.layernorm_pair(t("x0", 4, 16), t("w0", 16), t("b0", 16), 1e-5, t("out0", 4, 16, dtype=BF16),
                              t("x1", 16, 16), t("w1", 16), None, 1e-6, t("out1", 8, 16, dtype=BF16), row_map1=(2, 4, 1))


@case("layernorm_mx")
def _(t, rec):
    return ops.layernorm_mx(t("x", 4, 64), t("w", 64), t("b", 64), 1e-5)


@case("mx_quant f32")
def _(t, rec):
    return ops.mx_quant(t("x", 4, 64))


@case("mx_quant bf16 into out")
def _(t, rec):
    return ops.mx_quant(t("x", 4, 64, dtype=BF16), t.mx("out", 6, 64))


@case("rowstats")
def _(t, rec):
    return ops.rowstats(t("x", 4, 16), 1e-5, t("rowstat", 4, 2))


@case("rowstats copy")
def _(t, rec):
    return ops.rowstats(t("x", 4, 16), 1e-5, t("rowstat", 4, 2), copy=t("copy", 6, 16, dtype=BF16))


@case("rowstats_finish")
def _(t, rec):
    return ops.rowstats_finish(t("part", 3, 4, 2), 1e-5, t("rowstat", 4, 2))


def _srcs(t):
    qkv = t("qkv", 8, 384, dtype=BF16)
    return qkv[:, :128], qkv[:, 128:256], qkv[:, 256:]


@case("qkv_split inference")
def _(t, rec):
    return ops.qkv_split(*_srcs(t), t("qw", 64), t("kw", 64), 1e-5, 2, 4, 2, BF16, q_scale=ops.Q_PRESCALE)


@case("qkv_split train")
def _(t, rec):
    return ops.qkv_split(*_srcs(t), t("qw", 64), None, 1e-5, 2, 4, 2, BF16, train=True)


@case("qkv_split k v only")
def _(t, rec):
    return ops.qkv_split(None, *_srcs(t)[1:], None, t("kw", 64), 1e-5, 2, 4, 2, BF16)


# ------------------------------------------------------------------------------------------------------------- attention
def _qkv(t, B=2, H=2, Lq=4, Lk=5, dtype=BF16, shared=False, rowmajor=False):
    return (t("Q", 1 if shared else B, H, Lq, 64, dtype=dtype), t("K", B, H, Lk, 64, dtype=dtype),
            t("V", *((B, H, Lk, 64) if rowmajor else (B, H, 64, (Lk + 63) // 64 * 64)), dtype=dtype), t("out", B * Lq, H * 64, dtype=dtype))


@case("attention plain")
def _(t, rec):
    return ops.attention(*_qkv(t))


@case("attention f32 scale")
def _(t, rec):
    return ops.attention(*_qkv(t, dtype=F32), scale=0.25)


@case("attention shared_q")
def _(t, rec):
    return ops.attention(*_qkv(t, shared=True), shared_q=True)


@case("attention lse")
def _(t, rec):
    return ops.attention(*_qkv(t), lse=t("lse", 2, 2, 4))


@case("attention v_rowmajor prescaled")
def _(t, rec):
    return ops.attention(*_qkv(t, rowmajor=True), v_rowmajor=True, prescaled=True)


@case("attention bounded")
def _(t, rec):
    return ops.attention(*_qkv(t), bounded=True, prescaled=True)


@case("attention q_rows")
def _(t, rec):
    return ops.attention(*_qkv(t, Lq=64, Lk=64, rowmajor=True), v_rowmajor=True, prescaled=True, q_rows=32)


@case("attention q_rows past Lq, shared_q")
def _(t, rec):
    return ops.attention(*_qkv(t, Lq=40, shared=True), shared_q=True, q_rows=64)


def _parts(t, n, B=2, H=2, Lq=4):
    return [(t(f"O{i}", B * Lq, H * 64, dtype=BF16), t(f"lse{i}", B, H, Lq)) for i in range(n)]


@case("attention_merge two")
def _(t, rec):
    return ops.attention_merge(_parts(t, 2), t("out", 8, 128, dtype=BF16), 2, 2, 4)


@case("attention_merge three")
def _(t, rec):
    return ops.attention_merge(_parts(t, 3), t("out", 8, 128, dtype=BF16), 2, 2, 4)


# ------------------------------------------------------------------------------------------------------- training side
for _R in (8, 256, 2048):
    @case(f"colsum R={_R}")
    def _(t, rec, _R=_R):
        return ops.colsum(t("x", _R, 4))


@case("colsum into out, accumulate")
def _(t, rec):
    return ops.colsum(t("x", 8, 4, dtype=BF16), out=t("out", 4), accumulate=True)


for _cast, _reduce in ((False, True), (False, False), (True, True), (True, False)):
    @case(f"layernorm_bwd cast={_cast} reduce={_reduce}")
    def _(t, rec, _cast=_cast, _reduce=_reduce):
        return ops.layernorm_bwd(t("x", 16, 16), t("w", 16), 1e-5, t("dy", 8, 16, dtype=BF16), t("dx", 16, 16), True, row_map=(2, 4, 1),
                                 cast_out=t("cast", 16, 16, dtype=BF16) if _cast else None, reduce=_reduce)


for _reduce in (True, False):
    @case(f"qkv_split_bwd reduce={_reduce}")
    def _(t, rec, _reduce=_reduce):
        dQ, dK, dV = (t(n, 2, 2, 4, 64, dtype=BF16) for n in ("dQ", "dK", "dV"))
        raw, dout = t("raw", 8, 384, dtype=BF16), t("dout", 8, 384, dtype=BF16)
        return ops.qkv_split_bwd(dQ, dK, dV, raw[:, :128], raw[:, 128:256], t("qw", 64), t("kw", 64), 1e-5, 2, 4, 2,
                                 dout[:, :128], dout[:, 128:256], dout[:, 256:], reduce=_reduce)


@case("qkv_split_bwd q only")
def _(t, rec):
    return ops.qkv_split_bwd(t("dQ", 2, 2, 4, 64), None, None, t("raw", 8, 128), None, t("qw", 64), None, 1e-5, 2, 4, 2,
                             t("dout", 8, 128), None, None)


@case("attention_delta")
def _(t, rec):
    return ops.attention_delta(t("O", 8, 128, dtype=BF16), t("dO", 8, 128, dtype=BF16), 2, 2, 4)


@case("attention_bwd")
def _(t, rec):
    return ops.attention_bwd(t("Q", 2, 2, 4, 64), t("K", 2, 2, 5, 64), t("V", 2, 2, 5, 64), t("dO", 2, 2, 4, 64), t("lse", 2, 2, 4),
                             t("D", 2, 2, 4), scale=0.2)


@case("attention_bwd_mfma")
def _(t, rec):
    def split(prefix, Lh, names):
        return {n: t(prefix + n, 2, 2, *((64, 64) if n.endswith("t") else (Lh, 64)), dtype=BF16) for n in names}
    return ops.attention_bwd_mfma(split("q.", 4, ("Q", "Qt")), split("k.", 5, ("K", "Kt", "V")), split("do.", 4, ("Q", "Qt")),
                                  t("lse", 2, 2, 4), t("D", 2, 2, 4), shared_q=False)


@case("attention_bwd_mfma shared_q")
def _(t, rec):
    def split(prefix, B, Lh, names):
        return {n: t(prefix + n, B, 2, *((64, 64) if n.endswith("t") else (Lh, 64)), dtype=BF16) for n in names}
    return ops.attention_bwd_mfma(split("q.", 1, 4, ("Q", "Qt")), split("k.", 2, 5, ("K", "Kt", "V")), split("do.", 2, 4, ("Q", "Qt")),
                                  t("lse", 2, 2, 4), t("D", 2, 2, 4), shared_q=True)


@case("linear_n3")
def _(t, rec):
    return ops.linear_n3(t("a", 8, 16, dtype=BF16), t("w", 3, 16), t("bias", 3), t("out", 8, 3))


@case("linear_n3_bwd")
def _(t, rec):
    return ops.linear_n3_bwd(t("a", 8, 16, dtype=BF16), t("w", 3, 16), t("dout", 8, 3))


@case("linear_n3_bwd mul_by")
def _(t, rec):
    return ops.linear_n3_bwd(t("a", 8, 16, dtype=BF16), t("w", 3, 16), t("dout", 8, 3), mul_by=t("dg", 8, 24, dtype=BF16))


@case("n3_finish")
def _(t, rec):
    return ops.n3_finish(t("part", 4, 8, 3), t("bias", 3), t("out", 8, 3))


@case("cast")
def _(t, rec):
    return ops.cast(t("x", 8, 24)[:, :16], BF16)


@case("cast into out")
def _(t, rec):
    return ops.cast(t("x", 8, 16, dtype=BF16), F32, out=t("out", 8, 20)[:, 4:])


@case("transpose")
def _(t, rec):
    return ops.transpose(t("x", 70, 16, dtype=BF16))


@case("transpose rows_pad")
def _(t, rec):
    return ops.transpose(t("x", 8, 16), rows_pad=8)


@case("gelu")
def _(t, rec):
    return ops.gelu(t("z", 8, 16, dtype=BF16))


@case("gelu_bwd")
def _(t, rec):
    return ops.gelu_bwd(t("z", 8, 16), t("dh", 8, 16))


@case("mse")
def _(t, rec):
    return ops.mse(t("pred", 2, 5, 3), t("target", 2, 5, 3), 0.5)


@case("mse_bwd")
def _(t, rec):
    return ops.mse_bwd(t("pred", 2, 5, 3), t("target", 2, 5, 3), 0.5)


@case("mse_bwd grad_scale")
def _(t, rec):
    return ops.mse_bwd(t("pred", 2, 5, 3), t("target", 2, 5, 3), 0.5, grad_scale=t("scale", 1))


@case("adamw_step")
def _(t, rec):
    return ops.adamw_step(t("p", 10), t("g", 10), t("m", 10), t("v", 10), 1e-3, 0.9, 0.999, 1e-8, 0.01, 3)


@case("adamw_flat")
def _(t, rec):
    return ops.adamw_flat(t("p", 10), t("g", 10), t("m", 10), t("v", 10), 6, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, grad_scale=t("scale", 1))


@case("weight_mirror")
def _(t, rec):
    table = t("table", 2 * C.sizeof(L.MirrorItem), dtype=U8, dev=True)
    return ops.weight_mirror(t("src", 64), t("dst", 64, dtype=BF16), t("dstT", 128, dtype=BF16), table, 2, 5)


@case("weight_mirror no transposed copies")
def _(t, rec):
    return ops.weight_mirror(t("src", 64), t("dst", 64, dtype=BF16), None, t("table", C.sizeof(L.MirrorItem), dtype=U8, dev=True), 1, 1)


@case("grad_sumsq")
def _(t, rec):
    return ops.grad_sumsq(t("g", 10), t("out", 1), t("partial", 256), True, False)


# ------------------------------------------------------------------------------------------- pre- and post-processing
@case("patchify f32")
def _(t, rec):
    return ops.patchify(t("video", 2, 6, 8, 3), 4, 2, 16, BF16)


@case("patchify uint8")
def _(t, rec):
    return ops.patchify(t("video", 2, 6, 8, 3, dtype=U8), 4, 2, 16, F32)


@case("point_encode")
def _(t, rec):
    return ops.point_encode(t("xyz", 2, 5, 3), BF16)


@case("point_concat")
def _(t, rec):
    return ops.point_concat(t("normal", 5, 3), t("rgb", 5, 3), t("feat", 5, 16, dtype=BF16), 8)


@case("dino_cls_rows")
def _(t, rec):
    return ops.dino_cls_rows(t("cls", 8), t("pos0", 8), t("x", 10, 8), 2, 5)


def _tokens(t, ln_w):
    B, T, K, P, Cd = 1, 2, 2, 3, 8
    return ops.assemble_tokens(t("dino_x", B * T * (P + 1), Cd), t("dino_w", Cd), t("dino_b", Cd), 1e-6, t("pos", T * P, Cd), t("sp0", 4, Cd),
                               t("spr", 4, Cd), t("mesh", B * K, Cd), ln_w, 1e-5, B, T, K, P, drop_p=0.25, drop_seed=-3)


@case("assemble_tokens")
def _(t, rec):
    return _tokens(t, t("ln_w", 8))


@case("assemble_tokens no ln_w")
def _(t, rec):
    return _tokens(t, None)


@case("smooth_trajectories")
def _(t, rec):
    return ops.smooth_trajectories(t("trajs", 1, 3, 2, 3), 0.1, 1.5)


@case("smooth_savgol")
def _(t, rec):
    return ops.smooth_savgol(t("trajs", 1, 3, 2, 3), t("coef", 5, dtype=F64, dev=True))


@case("smooth_oneeuro")
def _(t, rec):
    return ops.smooth_oneeuro(t("trajs", 1, 3, 2, 3), 1.0, 0.5)


# --------------------------------------------------------------------------- calls that must be refused: one per raise
@case("refused gemm: operand shapes")
def _(t, rec):
    return ops.gemm(t("a", 8, 16, dtype=BF16), t("w", 12, 24, dtype=BF16), t("out", 8, 12))


@case("refused gemm: in_rows without residual")
def _(t, rec):
    return ops.gemm(*_abw(t, M=16), t("out", 8, 12), in_rows=(2, 4, 1))


@case("refused gemm: ln block table")
def _(t, rec):
    return ops.gemm(*_abw(t, K=128), t("out", 8, 12), ln=(t("part", 1, 8, 2), t("colsum", 12), 1e-5))


@case("refused gemm: ln rowstat")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), ln=(t("rowstat", 4, 2), t("colsum", 12)))


@case("refused gemm: stats_out")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), stats_out=t("stats", 1, 8, 2))


@case("refused gemm: copy_out")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), copy_out=t("copy", 8, 12))


@case("refused gemm: heads output shape")
def _(t, rec):
    return ops.gemm(*_abw(t), None, qkv_heads=_heads(t, 2, 4, H=3) + (1e-5, 1.0, 4, 2))


@case("refused gemm: transposed V at a ragged length")
def _(t, rec):
    return ops.gemm(*_abw(t), None, qkv_heads=_heads(t, 2, 4, vshape=(2, 2, 64, 4)) + (1e-5, 1.0, 4, 2))


@case("refused gemm: n3")
def _(t, rec):
    return ops.gemm(*_abw(t, N=256), None, n3=(t("w3", 3, 256), t("part", 4, 8, 3)))


@case("refused gemm: residual dtype")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), residual=t("res", 8, 12, dtype=BF16))


@case("refused gemm: out too small")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 12, 12), row_map=(2, 4, 1))


@case("refused gemm: two aux operands")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), preact_out=t("aux", 8, 12), mul_by=t("aux2", 8, 12))


@case("refused gemm: aux dtype")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), mul_by=t("aux", 8, 12, dtype=BF16))


@case("refused gemm: bias length")
def _(t, rec):
    return ops.gemm(*_abw(t), t("out", 8, 12), bias=t("bias", 8))


@case("refused gemm: inner stride")
def _(t, rec):
    return ops.gemm(t("a", 16, 8, dtype=BF16).t(), t("w", 12, 16, dtype=BF16), t("out", 8, 12))


@case("refused gemm_pair: one projection")
def _(t, rec):
    return ops.gemm_pair([None])


@case("refused gemm_mx: heads output shape")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 8, 64), t.mx("w", 384, 64), None, qkv_heads=_heads(t, 2, 4, H=3) + (1e-5, 1.0, 4, 2))


@case("refused gemm_mx: out too small")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 8, 64), t.mx("w", 32, 64), t("out", 8, 16, dtype=BF16))


@case("refused gemm_mx: operand")
def _(t, rec):
    return ops.gemm_mx(t.mx("a", 8, 64), t.mx("w", 32, 32), t("out", 8, 32, dtype=BF16))


@case("refused gemm_tn: operands")
def _(t, rec):
    return ops.gemm_tn(t("x", 40, 8, dtype=BF16), t("y", 32, 12, dtype=BF16))


@case("refused gemm_tn: out")
def _(t, rec):
    return ops.gemm_tn(t("x", 40, 8, dtype=BF16), t("y", 40, 12, dtype=BF16), out=t("out", 8, 12, dtype=BF16))


@case("refused gemm_tn: accumulate without out")
def _(t, rec):
    return ops.gemm_tn(t("x", 40, 8, dtype=BF16), t("y", 40, 12, dtype=BF16), accumulate=True)


@case("refused attention: shapes")
def _(t, rec):
    return ops.attention(*_qkv(t, rowmajor=True))


@case("refused attention: not contiguous")
def _(t, rec):
    Q, K, V, out = _qkv(t)
    return ops.attention(t("Q2", 2, 2, 64, 4, dtype=BF16).transpose(2, 3), K, V, out)


@case("refused attention: dtypes")
def _(t, rec):
    Q, K, V, _ = _qkv(t)
    return ops.attention(Q, K, V, t("out32", 8, 128))


@case("refused attention: batch")
def _(t, rec):
    return ops.attention(*_qkv(t, shared=True))


@case("refused attention: out too small")
def _(t, rec):
    Q, K, V, _ = _qkv(t)
    return ops.attention(Q, K, V, t("small", 8, 64, dtype=BF16))


@case("refused layernorm: dtypes")
def _(t, rec):
    return ops.layernorm(t("x", 8, 16, dtype=BF16), t("w", 16), None, 1e-5, t("out", 8, 16))


@case("refused layernorm: rows")
def _(t, rec):
    return ops.layernorm(t("x", 12, 16), t("w", 16), None, 1e-5, t("out", 8, 16), row_map=(2, 4, 1))


@case("refused layernorm_pair: widths")
def _(t, rec):
    return ops.layernorm_pair(t("x0", 4, 16), t("w0", 16), None, 1e-5, t("out0", 4, 16), t("x1", 8, 12), t("w1", 12), None, 1e-5, t("out1", 8, 12))


@case("refused layernorm_pair: rows")
def _(t, rec):
    return ops.layernorm_pair(t("x0", 4, 16), t("w0", 16), None, 1e-5, t("out0", 4, 16), t("x1", 12, 16), t("w1", 16), None, 1e-5,
                              t("out1", 8, 16), row_map1=(2, 4, 1))


# ----------------------------------------------------------------------------------------------------------------- file
def dumps(table):
    """one line per call"""
    enc = lambda v: json.dumps(v, separators=(",", ":"))
    out = []
    for name, e in table.items():
        rest = ",".join(f"{enc(k)}:{enc(v)}" for k, v in e.items() if k != "calls")
        out.append("%s:{\"calls\":[\n%s],\n%s}" % (enc(name), ",\n".join(enc(c) for c in e["calls"]), rest))
    return "{\n" + ",\n".join(out) + "\n}\n"


def main(argv):
    repo = argv[argv.index("--repo") + 1] if "--repo" in argv else REPO
    sys.path.insert(0, repo)
    import motion324_amd.lib as lib_module
    import motion324_amd.ops as ops_module
    assert os.path.dirname(os.path.dirname(os.path.abspath(ops_module.__file__))) == os.path.abspath(repo), ops_module.__file__
    table = record(ops_module, lib_module)
    # the intended differences (EXPECTED, above) go into the parent's record here, by hand: nothing else of the fixture is ever
    # taken from the code under test
    for name, names in EXPECTED.items():
        table[name]["wrote"] = sorted(set(table[name]["wrote"]) | set(names))
    text = dumps(table)
    if "--stdout" in argv:
        sys.stdout.write(text)
    else:
        with open(OUT, "w") as f:
            f.write(text)
        print(OUT, len(table), "cases,", len(text), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
