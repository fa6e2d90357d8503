"""Records the gate of the end-to-end LPIPS tests: python tests/golden/make_lpips_band.py

For every case of tests/lpips_cases.py the oracle runs twice on the CPU, in fp64 and in torch fp32.  tests/golden/lpips_band.npz
keeps the fp64 values per frame and layer (<case>.ref [T,5]) and, per layer and for the total, the largest relative deviation
of the fp32 run over the frames (<case>.band [6]); the table of tests/ERROR_BOUNDS_LPIPS.md between its two markers is
rewritten from the same numbers.  Nothing here runs the code under test.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import lpips_cases as LC  # noqa: E402

DOC = os.path.join(os.path.dirname(HERE), "ERROR_BOUNDS_LPIPS.md")
BEGIN, END = "<!-- band:begin -->", "<!-- band:end -->"


def main():
    torch.manual_seed(0)
    out, rows = {}, []
    for name in LC.CASES:
        a, b = LC.clips(name)
        ref, up = LC.oracle(a, b, torch.float64)
        low32, _ = LC.oracle(a, b, torch.float32)
        band = LC.relative_deviation(low32, ref)
        identity = float(np.abs(LC.with_total(up) - LC.with_total(ref)).max() / np.abs(LC.with_total(ref)).max())
        out[name + ".ref"], out[name + ".band"] = ref, band
        H, W, T, _ = LC.CASES[name]
        share = ref.sum(0) / ref.sum()
        rows.append(f"| {name} | {H} x {W} | {T} | " + " | ".join(f"{v:.2e}" for v in band) + f" | {ref.sum(1).mean():.6f} | "
                    + " ".join(f"{100 * s:.1f}" for s in share) + f" | {identity:.1e} |")
    np.savez(LC.GOLDEN, **out)
    table = ["| case | size | T | layer 1 | layer 2 | layer 3 | layer 4 | layer 5 | total | mean score (fp64) | share of the layers, % | "
             "upsampled vs own mean |", "|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows
    text = open(DOC).read()
    head, rest = text.split(BEGIN)
    tail = rest.split(END)[1]
    open(DOC, "w").write(head + BEGIN + "\n" + "\n".join(table) + "\n" + END + tail)
    print("\n".join(table))


if __name__ == "__main__":
    main()
