"""Records the gate of the U2-Net tests: python tests/golden/make_matting_band.py

For every case of tests/matting_cases.py the oracle runs twice on the CPU, in fp64 and in torch fp32.
tests/golden/matting_band.npz keeps, per case, the largest deviation of the fp32 run from the fp64 one for the logits d0 and the
eleven taps, each relative to the fp64 tensor's largest magnitude (<case> [12]); the table of tests/ERROR_BOUNDS_MATTING.md between
its two markers is rewritten from the same numbers, with what the quantised-mask check needs next to them.  Nothing here runs the
code under test.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import matting_cases as MC  # noqa: E402

DOC = os.path.join(os.path.dirname(HERE), "ERROR_BOUNDS_MATTING.md")
BEGIN, END = "<!-- band:begin -->", "<!-- band:end -->"


def main():
    torch.manual_seed(0)
    out, rows = {}, []
    for name, (variant, size, T) in MC.CASES.items():
        x, ref = MC.reference(name)
        got = MC.oracle(variant, x, torch.float32)
        out[name] = MC.deviation(got, ref)
    np.savez(MC.GOLDEN, **out)
    for name, (variant, size, T) in MC.CASES.items():        # the quantised-mask columns read the gate: after the file is written
        x, ref = MC.reference(name)
        _, delta, R = MC.quantised_reference(name)
        q32 = MC.model_quantise(MC.sigmoid64(MC.oracle(variant, x, torch.float32)["d0"]).astype(np.float32))
        ambiguous, wrong, far = MC.check_quantised(name, q32)
        band = out[name]
        rows.append(f"| {name} | {size} | {T} | {band[0]:.2e} | {band[1:7].max():.2e} | {band[7:].max():.2e} | {np.abs(ref['d0']).max():.2f} | "
                    f"{R.min():.3f} | {delta.max():.4f} | {100 * ambiguous:.2f} | {wrong} / {far} |")
    table = ["| case | size | T | d0 | hx1..hx6 (largest) | hx5d..hx1d (largest) | max abs d0 | min range | delta, levels | ambiguous, % | "
             "fp32 CPU: wrong outside the zone / off by more than one |", "|---|---|---|---|---|---|---|---|---|---|---|"] + rows
    text = open(DOC).read()
    head, rest = text.split(BEGIN)
    tail = rest.split(END)[1]
    open(DOC, "w").write(head + BEGIN + "\n" + "\n".join(table) + "\n" + END + tail)
    print("\n".join(table))
    for name in MC.CASES:
        print(name, " ".join(f"{v:.2e}" for v in out[name]))


if __name__ == "__main__":
    main()
