"""Table of what libm324's host-only plan queries answer: tests/golden/plans.json.

m324_gemm_plan and m324_attention_plan name the kernel, its template arguments and its grid for a call; the launchers work from
the same plan (csrc/gemm.hip make_plan, csrc/attention.hip attn_plan).  bench.py and profiles/ label their rows with these
strings, transformer.hp_consumer and m324_gemm_pair act on the schedule number -- so a refactor of the launch path must leave
every answer as it is.  This script enumerates the model's GEMM shapes and a few ragged ones under every epilogue kind and every
chooser switch, and the attention shapes under every attention switch, and records the answers; tests/test_plans_cpu.py
enumerates the same cases against the library of the day and compares case by case.  (A few crossings are calls m324_gemm itself
would reject -- a folded LayerNorm at M = 64, say; the query does not validate, its answer is recorded all the same.)

The queries touch no device: run with the devices hidden (HIP_VISIBLE_DEVICES=-1), so that the compute-unit count the
persistent grids are clamped to is the library's fallback of 256 on every machine.

    python tests/golden/make_plan_table.py            writes tests/golden/plans.json (M324_LIB selects the library)
    python tests/golden/make_plan_table.py --stdout   prints the table instead

Format: "plans" holds every distinct [return value, text] once; "gemm" / "attn" hold one index into it per case, in the order
gemm_cases() / attn_cases() yield them ("attn" packed: pack()); "key" is a digest of the case descriptions (a changed enumeration
is told apart from a changed answer).  A plan that is in the file already keeps its index, so recording again changes the file
only where cases or answers changed; loads() reads what dumps() wrote."""
import ctypes as C
import hashlib
import importlib.util
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "plans.json")

GEMM_SHAPES = [(10368, 3072, 768), (10368, 2304, 768), (10368, 768, 3072), (10368, 768, 768), (65536, 3072, 768), (45056, 3072, 768),
               (8224, 768, 3072), (2048, 1536, 768), (64, 768, 768), (293, 256, 192), (200, 128, 768), (300, 328, 64)]
GEMM_SETTINGS = ([()] + [(("M324_GEMM", v),) for v in (1, 2, 5, 7, 9, 10, 11, 12, 13, 14, 15)] + [(("M324_HP", v),) for v in (0, 3)]
                 + [(("M324_QKV_RING", v),) for v in (0, 3)] + [(("M324_GEMM_PERSIST", 0),)])
ATTN_SETTINGS = [()] + [((name, v),) for name, vals in (("M324_ATTN_NW", (4, 8)), ("M324_ATTN_EXP", (8,)), ("M324_ATTN_PWG", (0,))) for v in vals]
F32, BF16 = 0, 1
AUX_STORE_PREACT, AUX_MUL_GELU_GRAD, AUX_HEADS, AUX_HEADS_VT, AUX_N3, AUX_STORE_GELU_GRAD, AUX_MUL = 1, 2, 3, 4, 5, 6, 7
PTR = 4096                      # aligned stand-in: the queries read sizes, flags and alignments only


def gemm_kinds():
    """(name, fields): every epilogue kind the library accepts.  fields are GemmArgs members; `res` / `fold` are expanded by
    gemm_args()."""
    kinds = []
    for out, gelu, res in itertools.product((BF16, F32), (0, 1), ("none", "rows", "res_rows", "row_map")):
        kinds.append((f"plain out={out} gelu={gelu} res={res}", dict(out_dtype=out, act=gelu, res=res)))
    for mode, gelu in ((AUX_STORE_PREACT, 1), (AUX_STORE_GELU_GRAD, 1), (AUX_MUL_GELU_GRAD, 0), (AUX_MUL, 0)):
        for out in (BF16, F32):
            kinds.append((f"aux={mode} out={out}", dict(out_dtype=out, act=gelu, aux_mode=mode, aux=PTR)))
    for mode, fold in itertools.product((AUX_HEADS, AUX_HEADS_VT), ("", "merged")):
        kinds.append((f"heads={mode} fold={fold}", dict(out_dtype=BF16, aux_mode=mode, qkv=True, fold=fold)))
    for fold in ("", "merged"):
        kinds.append((f"n3 fold={fold}", dict(out_dtype=BF16, act=1, aux_mode=AUX_N3, aux=PTR, qkv_qw=PTR, fold=fold)))
    for fold, (out, gelu) in itertools.product(("merged", "unmerged"), ((BF16, 0), (BF16, 1), (F32, 0))):
        kinds.append((f"consumer {fold} out={out} gelu={gelu}", dict(out_dtype=out, act=gelu, fold=fold)))
    for out, res in itertools.product((BF16, F32), ("rows", "res_rows")):
        kinds.append((f"producer out={out} res={res}", dict(out_dtype=out, res=res, fold="producer")))
    for gelu, res in itertools.product((0, 1), ("none", "rows")):
        kinds.append((f"f32 operands gelu={gelu} res={res}", dict(in_dtype=F32, out_dtype=F32, act=gelu, res=res)))
    kinds.append(("batched bf16", dict(out_dtype=F32, batch=4)))
    kinds.append(("batched f32", dict(in_dtype=F32, out_dtype=F32, batch=4)))
    kinds.append(("misaligned C bf16", dict(out_dtype=BF16, C=PTR + 2)))
    kinds.append(("misaligned C f32", dict(out_dtype=F32, C=PTR + 4)))
    return kinds


def gemm_args(L, M, N, K, fields):
    a = L.GemmArgs()
    a.A = a.W = a.C = a.bias = PTR
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc = M, N, K, K, K, N
    a.in_dtype, a.batch = BF16, 1
    f = dict(fields)
    res, fold, qkv = f.pop("res", "none"), f.pop("fold", ""), f.pop("qkv", False)
    for k, v in f.items():
        setattr(a, k, v)
    if a.aux:
        a.ldaux = N
    if a.batch > 1:
        a.strideA = a.strideW = M * K
        a.strideC = M * N
    if res != "none":
        a.residual, a.ldr = PTR, N
    if res == "res_rows":
        a.res_rows = 100
    if res == "row_map":
        a.row_gin, a.row_gout, a.row_off = 4, 8, 2
    if qkv:
        a.qkv_q = a.qkv_k = a.qkv_v = PTR
        a.qkv_L, a.qkv_H = 64, max(N // 192, 1)
    if fold in ("merged", "unmerged"):
        a.ln_rowstat, a.ln_colsum, a.ln_eps = PTR, PTR, 1e-5
        a.ln_ncb = K // 64 if fold == "unmerged" else 0
    if fold == "producer":
        a.ln_stats_out = PTR
        if a.out_dtype == F32:
            a.ln_copy_out, a.ln_ldcopy = PTR, N
    return a


def gemm_cases():
    for setting, (M, N, K), (name, fields) in itertools.product(GEMM_SETTINGS, GEMM_SHAPES, gemm_kinds()):
        yield setting, (M, N, K), name, fields


def attn_cases():
    # (the key length innermost, the dtype outside the lengths: long runs of equal answers, which pack() stores as runs)
    for setting, B, H, dtype, Lq, flags, Lk in itertools.product(ATTN_SETTINGS, (1, 2, 32), (1, 12), (BF16, F32),
                                                                 (1, 64, 128, 257, 324, 512, 700, 1024, 2048, 4096, 10368),
                                                                 (0, 1, 2, 3, 5, 257), (1, 37, 64, 257, 512, 1100, 4096, 10368)):
        yield setting, B, H, Lq, Lk, flags, dtype


def load_lib():
    """motion324_amd/lib.py by path: the binding alone, without the package (and torch) around it"""
    spec = importlib.util.spec_from_file_location("m324lib", os.path.join(REPO, "motion324_amd", "lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L


def table(keep=None):
    """keep: the table recorded before (loads()); its plans keep their places"""
    L = load_lib()
    h = L.load()
    buf = C.create_string_buffer(256)
    plans = [tuple(p) for p in keep["plans"]] if keep else []
    index = {p: i for i, p in enumerate(plans)}

    def record(rc):
        key = (int(rc), buf.value.decode())
        if key not in index:
            index[key] = len(plans)
            plans.append(key)
        return index[key]

    def answers(cases, ask):
        out, digest, current = [], hashlib.sha256(), ()
        for case in cases:
            setting = case[0]
            if setting != current:
                for name, _ in current:
                    L.set_tunable(name)
                for name, v in setting:
                    L.set_tunable(name, v)
                current = setting
            digest.update(repr(case).encode())
            buf.value = b""
            out.append(record(ask(*case[1:])))
        for name, _ in current:
            L.set_tunable(name)
        return out, digest.hexdigest()

    gemm, kg = answers(gemm_cases(), lambda shape, name, fields: h.m324_gemm_plan(C.byref(gemm_args(L, *shape, fields)), buf, 256))
    attn, ka = answers(attn_cases(), lambda *c: h.m324_attention_plan(*c, buf, 256))
    # plans no case answers any more leave the list; the used ones past its new end move into their places, every other index stays
    used = set(gemm) | set(attn)
    n = len(used)
    move = dict(zip((i for i in range(n, len(plans)) if i in used), (i for i in range(n) if i not in used)))
    for i, hole in move.items():
        plans[hole] = plans[i]
    del plans[n:]
    return {"key": hashlib.sha256((kg + ka).encode()).hexdigest()[:16], "plans": [list(p) for p in plans],
            "gemm": [move.get(i, i) for i in gemm], "attn": [move.get(i, i) for i in attn]}


def pack(idx, settings):
    """Runs of equal answers.  The first (default) setting: [answer, count, ...]; every further setting: [position, count, answer, ...]
    of the cases it answers differently from the default.  (The cases run setting by setting.)"""
    n = len(idx) // settings
    base, out = idx[:n], [[]]
    for v in base:
        if out[0] and out[0][-2] == v:
            out[0][-1] += 1
        else:
            out[0] += [v, 1]
    for s in range(1, settings):
        runs = []
        for i, (v, b) in enumerate(zip(idx[s * n:(s + 1) * n], base)):
            if v != b and runs and runs[-3] + runs[-2] == i and runs[-1] == v:
                runs[-2] += 1
            elif v != b:
                runs += [i, 1, v]
        out.append(runs)
    return out


def unpack(packed):
    base = [v for v, c in zip(packed[0][::2], packed[0][1::2]) for _ in range(c)]
    out = list(base)
    for runs in packed[1:]:
        block = list(base)
        for i, c, v in zip(runs[::3], runs[1::3], runs[2::3]):
            block[i:i + c] = [v] * c
        out += block
    return out


def loads(text):
    t = json.loads(text)
    t["attn"] = unpack(t["attn"])
    return t


def dumps(t):
    enc = lambda v: json.dumps(v, separators=(",", ":"))
    return ('{"key":%s,\n"plans":[\n%s\n],\n"gemm":%s,\n"attn":%s}\n'
            % (enc(t["key"]), ",\n".join(enc(p) for p in t["plans"]), enc(t["gemm"]), enc(pack(t["attn"], len(ATTN_SETTINGS)))))


if __name__ == "__main__":
    keep = None
    if os.path.exists(OUT):
        with open(OUT) as f:
            keep = loads(f.read())
    text = dumps(table(keep))
    if "--stdout" in sys.argv:
        sys.stdout.write(text)
    else:
        with open(OUT, "w") as f:
            f.write(text)
        print(OUT, len(text), "bytes")
