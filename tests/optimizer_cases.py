"""Inputs of the optimizer-step tests (tests/test_optimizer_gpu.py, tests/test_error_bounds_cpu.py) and an fp32 numpy emulation of
the two AdamW kernels with their rounding points (adamw_kernel, adamw_flat_kernel: motion324_amd/csrc/backward.hip), with the faults
the CPU tests plant."""
import numpy as np
import torch

# lr 4e-4 is the schedule's peak: one step of decay is lr * wd = 2e-5 of |p|, some 300 fp32 roundings, so a wrong decay is visible
# element by element.  At a late-cosine lr such as 4e-6 it is 2e-7 |p| -- three roundings, inside any honest bound of the update --
# and a test run there would prove nothing about the decay.
HYPER = dict(lr=4e-4, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)
STEPS = (1, 2, 3, 100, 20000)
GRAD_SCALES = (None, 1.0, 0.37, 1e-3)


def adamw_inputs(n, step, seed):
    """p: magnitudes 1e-4 .. 10, random sign.  g: log-uniform 1e-12 .. 10, random sign, every 17th an exact zero: from `eps` ruling
    the denominator to `eps` invisible in it.  m, v: zero at step 1; afterwards m has |g|'s magnitude (times 0.1 .. 10) with a sign
    of its own, so b1 m and (1 - b1) g cancel in half of the elements, and v = g^2 times 0.25 .. 4 (1e-6 / 1e-12 scale where g = 0)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    sign = lambda: torch.where(r() < 0.5, -1.0, 1.0)
    p = sign() * 10.0 ** (-4 + 5 * r())
    g = sign() * 10.0 ** (-12 + 13 * r())
    g[::17] = 0.0
    if step == 1:
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    else:
        mag = torch.where(g == 0, torch.full_like(g, 1e-6), g.abs())
        m = sign() * mag * 10.0 ** (-1 + 2 * r())
        v = mag * mag * (0.25 + 3.75 * r())
    return tuple(t.to(torch.float32) for t in (p, g, m, v))


def decay_vector(n, n_decay, weight_decay):
    wd = torch.zeros(n, dtype=torch.float64)
    wd[:n_decay] = float(np.float32(weight_decay))
    return wd


def emulate(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=None, form="divide", fma=False, fault=None):
    """One update in fp32 numpy, every operation rounded where the kernel rounds it.  form "divide": adamw_kernel
    (sqrtf(v) / bc2_sqrt), "reciprocal": adamw_flat_kernel (sqrtf(v) * (1 / bc2_sqrt), weight decay as a factor per element).
    fma: the product-and-sum pairs contracted (one rounding: computed in fp64, rounded once).  weight_decay: scalar or per-element
    array.  fault: None | "step" | "eps_inside" | "m_factor" | "no_scale".  Returns fp32 (p', m', v')."""
    f = np.float32
    p, g, m, v = (np.asarray(t, dtype=f) for t in (p, g, m, v))
    lr, b1, b2, eps = f(lr), f(beta1), f(beta2), f(eps)
    wd = np.asarray(weight_decay, dtype=f)
    t = f(step + 1 if fault == "step" else step)
    gs = f(1.0 if grad_scale is None or fault == "no_scale" else grad_scale)
    bc1 = f(1) - np.power(b1, t, dtype=f)
    bc2s = np.sqrt(f(1) - np.power(b2, t, dtype=f), dtype=f)
    mul_add = (lambda a, b, c: (a.astype(np.float64) * b + c).astype(f)) if fma else (lambda a, b, c: a * b + c)
    gc = g * gs
    one_b1 = f(1) if fault == "m_factor" else f(1) - b1
    mi = mul_add(np.broadcast_to(b1, m.shape), m, one_b1 * gc)
    vi = mul_add(np.broadcast_to(b2, v.shape), v, (f(1) - b2) * gc * gc)
    keep = f(1) - lr * wd
    root = np.sqrt(vi, dtype=f)
    if fault == "eps_inside":
        den = np.sqrt(vi / (bc2s * bc2s) + eps, dtype=f)
    elif form == "divide":
        den = root / bc2s + eps
    else:
        den = mul_add(root, np.broadcast_to(f(1) / bc2s, root.shape), eps)
    q = (lr / bc1) * mi / den
    if form == "divide":
        pi = p * keep - q
    else:
        pi = mul_add(p, np.broadcast_to(keep, p.shape), -q)
    return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in (pi, mi, vi))
