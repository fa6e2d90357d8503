"""Writes tests/golden/fvd_band.npz and the band table of tests/ERROR_BOUNDS_FVD.md: per case and tap (and for the 400 features)
the fp64 oracle's values at a seeded sample of elements, the RMS and the fraction of positive elements of the whole map, and the
band -- the largest deviation of the SAME oracle run in torch fp32 on the CPU from the fp64 values over the whole map, relative
to that RMS.  Runs on the CPU only:

    python tests/golden/make_fvd_band.py
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import fvd_cases as FC  # noqa: E402


def main():
    out, rows = {}, []
    for name, (N, T, H, W, window, _) in FC.CASES.items():
        frames = FC.videos(name)
        ref = FC.oracle(frames, torch.float64)
        low = FC.oracle(frames, torch.float32)
        cells, alive = [], []
        for key in FC.KEYS:
            r = ref[key]
            p = f"{name}.{key}."
            out[p + "ref"] = r.reshape(-1)[FC.sample_index(name, key, r.size)]
            out[p + "size"] = np.int64(r.size)
            out[p + "rms"] = np.float64(FC.rms(r))
            out[p + "band"] = np.float64(FC.deviation(low[key], r))
            out[p + "positive"] = np.float64((r > 0).mean())
            cells.append(f"{float(out[p + 'band']):.2e}")
            alive.append(f"{100 * float(out[p + 'positive']):.0f} % / {float(out[p + 'rms']):.2f}")
        rows.append(f"| {name} | {N} x {T} x {H} x {W} | {window} | " + " | ".join(cells) + " | " + " | ".join(alive[:4]) + " |")
        print(rows[-1], flush=True)
    np.savez(FC.GOLDEN, **out)
    head = ("| case | N x T x H x W | head window | " + " | ".join(FC.KEYS) + " | "
            + " | ".join(f"{k}: positive / RMS" for k in FC.TAPS) + " |\n|" + "---|" * (3 + len(FC.KEYS) + len(FC.TAPS)) + "\n")
    doc = os.path.join(os.path.dirname(HERE), "ERROR_BOUNDS_FVD.md")
    if os.path.exists(doc):
        text = open(doc).read()
        text = re.sub(r"(<!-- band:begin -->\n).*?(<!-- band:end -->)", lambda m: m.group(1) + head + "\n".join(rows) + "\n" + m.group(2), text, flags=re.S)
        open(doc, "w").write(text)
    print(f"wrote {FC.GOLDEN} ({os.path.getsize(FC.GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
