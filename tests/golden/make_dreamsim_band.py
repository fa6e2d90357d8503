"""Writes tests/golden/dreamsim_band.npz: per case of tests/dreamsim_cases.py and per tap (and the features) the fp64 values of
the oracle at a seeded sample of elements, the RMS of the whole tap, and the band -- the largest deviation of the same oracle in
torch fp32 on the CPU from the fp64 values over the WHOLE tap, relative to that RMS (the rule of tests/ERROR_BOUNDS_FVD.md).

    python tests/golden/make_dreamsim_band.py [--table]

CPU only, a few seconds.  --table prints the band table of tests/ERROR_BOUNDS_DREAMSIM.md.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import dreamsim_cases as cases      # noqa: E402


def records(name):
    """{"<case>.<key>.<field>": array} of one case"""
    ref = cases.case_oracle(name, torch.float64)
    f32 = cases.case_oracle(name, torch.float32)
    out = {}
    for key in cases.KEYS:
        r = ref[key].reshape(-1)
        p = f"{name}.{key}."
        out[p + "ref"] = r[cases.sample_index(name, key, r.size)]
        out[p + "size"] = np.int64(r.size)
        out[p + "rms"] = np.float64(cases.rms(r))
        out[p + "band"] = np.float64(cases.deviation(f32[key].reshape(-1), r))
    return out


def table(z):
    lines = ["| case | layout, activation, feature | width / heads / layers / MLP | patch, tokens | images | " + " | ".join(cases.KEYS) + " | RMS of "
             + ", ".join(cases.KEYS) + " |", "|---|---|---|---|---|" + "---|" * (len(cases.KEYS) + 1)]
    for name, c in cases.CASES.items():
        bands = " | ".join(f"{float(z[f'{name}.{k}.band']):.2e}" for k in cases.KEYS)
        sizes = ", ".join(f"{float(z[f'{name}.{k}.rms']):.2f}" for k in cases.KEYS)
        lines.append(f"| {name} | {c['layout']}, {c['act']}, {c['feature']} | {c['width']} / {c['heads']} / {c['layers']} / {c['mlp']} | "
                     f"{c['patch']}, {(c['image'] // c['patch']) ** 2 + 1} | {c['images']} ({c['image']} x {c['image']}) | {bands} | {sizes} |")
    return "\n".join(lines)


def main():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    z = {}
    for name in cases.CASES:
        z.update(records(name))
    if "--table" in sys.argv:
        print(table(z))
        return
    np.savez(cases.GOLDEN, **z)
    print(f"wrote {cases.GOLDEN} ({os.path.getsize(cases.GOLDEN)} bytes)")
    print(table(z))


if __name__ == "__main__":
    main()
