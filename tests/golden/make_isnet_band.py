"""Records the gate of the ISNet tests: python tests/golden/make_isnet_band.py

For every case of tests/isnet_cases.py the oracle runs twice on the CPU, in fp64 and in torch fp32.  tests/golden/isnet_band.npz
keeps, per case, the largest deviation of the fp32 run from the fp64 one for the logits d1, the stem's output hxin and the eleven
taps, each relative to the fp64 tensor's largest magnitude (<case> [13]); the table of tests/ERROR_BOUNDS_ISNET.md between its two
markers is rewritten from the same numbers, with what the quantised-mask check needs next to them.  Nothing here runs the code
under test.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import isnet_cases as IC  # noqa: E402
import matting_cases as MC  # noqa: E402

DOC = os.path.join(os.path.dirname(HERE), "ERROR_BOUNDS_ISNET.md")
BEGIN, END = "<!-- band:begin -->", "<!-- band:end -->"
CASE_LIST = list(IC.CASES)


def row(name, band):
    """the document's row of a case; the quantised-mask columns read the gate, so the band file must be written first"""
    size, T = IC.CASES[name]
    ref = IC.reference(name)[1]
    _, delta, R = IC.quantised_reference(name)
    q32 = MC.model_quantise(MC.sigmoid64(IC.fp32_run(name)["d1"]).astype(np.float32))
    ambiguous, wrong, far = IC.check_quantised(name, q32)
    return (f"| {name} | {size} | {T} | {band[0]:.2e} | {band[1]:.2e} | {band[2:8].max():.2e} | {band[8:].max():.2e} | {np.abs(ref['d1']).max():.2f} | "
            f"{R.min():.3f} | {delta.max():.4f} | {100 * ambiguous:.2f} | {wrong} / {far} |")


def main():
    torch.manual_seed(0)
    out = {name: IC.deviation(IC.fp32_run(name), IC.reference(name)[1]) for name in CASE_LIST}
    np.savez(IC.GOLDEN, **out)
    table = ["| case | size | T | d1 | hxin | hx1..hx6 (largest) | hx5d..hx1d (largest) | max abs d1 | min range | delta, levels | ambiguous, % | "
             "fp32 CPU: wrong outside the zone / off by more than one |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    table += [row(name, out[name]) for name in CASE_LIST]
    text = open(DOC).read()
    head, rest = text.split(BEGIN)
    tail = rest.split(END)[1]
    open(DOC, "w").write(head + BEGIN + "\n" + "\n".join(table) + "\n" + END + tail)
    print("\n".join(table))
    for name in CASE_LIST:
        print(name, " ".join(f"{v:.2e}" for v in out[name]))


if __name__ == "__main__":
    main()
