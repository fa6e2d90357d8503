#!/usr/bin/env python3
"""The MXFP8 inference mode: what it buys per GEMM role and what it costs in accuracy.
  gemm : per shape, MX against the bf16 GEMM the clip runs today, interleaved in one process (median of rounds).  bf16: the
         LayerNorm-folded consumer merging the producer's statistics table itself (q|k|v, fc1; what the clip runs) and the fp32
         residual update (fc2).  MX: the GEMM, and on its own the LayerNorm -> MX pass it needs in front (q|k|v, fc1).
  roles: pcd_moved / per-stage error vs the fp32 forward at c1 (synthetic and trained-like weights) with every built role alone,
         the default set and all four (transformer.MX_ROLES is the table the mode reads, MX_ROLES_BUILT what exists).
usage: tools/mx_ab.py gemm|roles"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from motion324_amd import ops                     # noqa: E402
from motion324_amd.lib import ACT_GELU            # noqa: E402

DEV = "cuda"


def _time(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3              # us


def gemm():
    g = torch.Generator().manual_seed(0)
    rows_of = {"trunk": 10368, "dino": 8224}
    print("| role | M x N x K | bf16 GEMM as the clip runs it (us) | MX GEMM (us) | LayerNorm -> MX pass (us) | MX total / bf16 |")
    print("|---|---|---|---|---|---|")
    for part, M in rows_of.items():
        C = 768
        x = torch.randn(M, C, generator=g).to(DEV)
        lw, lb = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
        # the producer's per-block statistics table the clip's folded consumers merge themselves (M324_FOLD_MERGE): from the stream
        part_tab = torch.empty(C // 64, M, 2, device=DEV)
        xv = x.reshape(M, C // 64, 64)
        part_tab[..., 0] = xv.sum(-1).T
        part_tab[..., 1] = ((xv - xv.mean(-1, keepdim=True)) ** 2).sum(-1).T
        xb = x.to(torch.bfloat16)
        for role, N, K in (("qkv", 3 * C, C), ("fc1", 4 * C, C), ("fc2", C, 4 * C)):
            w = (torch.randn(N, K, generator=g) * 0.02).to(DEV)
            bias = (torch.randn(N, generator=g) * 0.02).to(DEV)
            wb, wmx = w.to(torch.bfloat16), ops.mx_quant(w)
            amx = ops.mx_empty(M, C, DEV)
            f_ln = None
            if role == "fc2":
                a = (torch.randn(M, K, generator=g) * 0.3).to(DEV)
                ab, amx = a.to(torch.bfloat16), ops.mx_quant(a)
                res = x.clone()
                gamma = torch.ones(N, device=DEV)
                f_bf = lambda: ops.gemm(ab, wb, res, bias=bias, gamma=gamma, residual=res)
                f_mx = lambda: ops.gemm_mx(amx, wmx, res, bias=bias, gamma=gamma, residual=res)
            else:
                # today: the LayerNorm folded into the projection, statistics merged by the consumer from the producer's table
                colsum = wb.float().sum(1).contiguous()
                outb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
                act = ACT_GELU if role == "fc1" else 0
                omx = ops.mx_empty(M, N, DEV) if role == "fc1" else outb
                f_bf = lambda: ops.gemm(xb, wb, outb, bias=bias, act=act, ln=(part_tab, colsum, 1e-5))
                f_mx = lambda: ops.gemm_mx(amx, wmx, omx, bias=bias, act=act)
                f_ln = lambda: ops.layernorm_mx(x, lw, lb, 1e-5, out=amx)
            fs = [f_bf, f_mx] + ([f_ln] if f_ln else [])
            for f in fs:
                f()
            torch.cuda.synchronize()
            t = [[] for _ in fs]
            for _ in range(7):                                  # interleaved rounds
                for i, f in enumerate(fs):
                    t[i].append(_time(f))
            med = [float(np.median(v)) for v in t]
            ln = med[2] if f_ln else 0.0
            print(f"| {part}.{role} | {M} x {N} x {K} | {med[0]:.1f} | {med[1]:.1f} | {ln:.1f} | {(med[1] + ln) / med[0]:.2f} |", flush=True)


def roles():
    from conftest import CASES, rel_err, synth_sd
    from test_model_gpu import build, inputs, run
    from test_trained_like_gpu import _model as tl_model, trained_like
    from motion324_amd import transformer
    full, default = transformer.MX_ROLES_BUILT, transformer.MX_ROLES
    sets = [(r,) for r in sorted(full)] + [tuple(sorted(default)), tuple(sorted(full))]
    stages = ("dino_tokens", "trunk_block0", "trunk_out", "pcd_moved")
    print("| weights | roles in MX | " + " | ".join(stages) + " |")
    print("|---|---|" + "---|" * len(stages))
    dims = CASES["c1"]["dims"]
    for kind in ("synthetic", "trained-like"):
        if kind == "synthetic":
            model, _ = build("c1")
        else:
            model, _ = tl_model(dims, trained_like(synth_sd(dims)))
        sample = inputs("c1", with_target=False)
        ref, cref = run(model, sample, "fp32")
        model.inference_precision = "bf16"
        b16, c16 = run(model, sample, "bf16")
        rows = [("(none: bf16 mode)", b16, c16)]
        model.inference_precision = "mxfp8"
        for s in sets:
            transformer.MX_ROLES = frozenset(s)
            o, c = run(model, sample, "bf16")
            rows.append(("all four" if len(s) == len(full) else " + ".join(s) + (" (default)" if frozenset(s) == default else ""), o, c))
        transformer.MX_ROLES = default
        for name, o, c in rows:
            errs = [rel_err(c[k], cref[k]) for k in stages[:-1]] + [rel_err(o.pcd_moved, ref.pcd_moved)]
            print(f"| {kind} | {name} | " + " | ".join(f"{e:.2e}" for e in errs) + " |", flush=True)


if __name__ == "__main__":
    {"gemm": gemm, "roles": roles}[sys.argv[1] if len(sys.argv) > 1 else "gemm"]()
