"""The small kernels around the transformer (motion324_amd/csrc/elementwise.hip: patchify, point features, the DINO class rows,
token assembly, the 3-wide head, the trajectory filters, the nearest-point search): seeded case tables at ragged and edge shapes,
fp64 references, and fp32 CPU emulations that follow the kernels' arithmetic order.  tests/test_frontend_cpu.py (no GPU) holds the
emulations to the gates and plants faults in them; tests/test_frontend_gpu.py holds the kernels to the same gates.

Every emulation takes a `fault` argument: None gives the kernel's arithmetic, a name gives one of the index mistakes the kernel could
make (the tests of the tests show that the gates catch each of them)."""
import math

import numpy as np
import torch

F32 = np.float32
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _gen(*key):
    return torch.Generator().manual_seed(int.from_bytes(repr(key).encode(), "little") % (2 ** 31 - 1))


# =========================================================================================== patchify
# (F, Hin, Win), (size, patch), Kp.  Every frame shape with at least two (size, patch) pairs, both Kp values with every pair.
# (3, 1, 7): one source row (both vertical taps clamp onto it) and up-sampling on both axes; (2, 40, 333): up-sampling in y beside
# down-sampling in x at size 224; (42, 14): an odd patch grid g = 3; Kp = 3 patch^2 = 588: the zero-fill loop is empty.
PATCHIFY_CASES = [
    ((2, 48, 80), (224, 14), 640), ((2, 48, 80), (42, 14), 588),
    ((1, 300, 200), (224, 14), 588), ((1, 300, 200), (28, 14), 640),
    ((3, 1, 7), (42, 14), 640), ((3, 1, 7), (28, 14), 588), ((3, 1, 7), (224, 14), 640),
    ((1, 224, 224), (224, 14), 588), ((1, 224, 224), (42, 14), 640),
    ((2, 40, 333), (28, 14), 640), ((2, 40, 333), (42, 14), 588), ((2, 40, 333), (224, 14), 588),
]


def patchify_id(case):
    (Fr, Hin, Win), (size, patch), Kp = case
    return f"{Fr}x{Hin}x{Win}-{size}/{patch}-Kp{Kp}"


def patchify_frames(Fr, Hin, Win):
    """(fp32 frames [F, Hin, Win, 3] in [0, 1], the same frames as bytes).  Noise plus a horizontal ramp of 0.30, a vertical one of
    0.15 and a step per frame and channel: a kernel that swaps the axes, the frames or the channels reads other values."""
    g = _gen("patchify", Fr, Hin, Win)
    noise = torch.rand((Fr, Hin, Win, 3), generator=g, dtype=torch.float64)
    x = torch.arange(Win, dtype=torch.float64).view(1, 1, Win, 1) / max(Win - 1, 1)
    y = torch.arange(Hin, dtype=torch.float64).view(1, Hin, 1, 1) / max(Hin - 1, 1)
    f = torch.arange(Fr, dtype=torch.float64).view(Fr, 1, 1, 1) / Fr
    c = torch.arange(3, dtype=torch.float64).view(1, 1, 1, 3) / 3
    v = 0.45 * noise + 0.30 * x + 0.15 * y + 0.05 * f + 0.05 * c
    return v.float().contiguous(), (v * 255).round().to(torch.uint8).contiguous()


def patchify_reference(video, size, patch):
    """fp64: F.interpolate(bilinear, align_corners=False) of the fp32 frame values, normalisation (the fp32 constants the kernel
    holds), unfold -> [F g^2, 3 patch^2]"""
    Fr = video.shape[0]
    g = size // patch
    img = torch.nn.functional.interpolate(video.double().permute(0, 3, 1, 2), (size, size), mode="bilinear", align_corners=False)
    mean = torch.tensor(MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).double().view(1, 3, 1, 1)
    rows = torch.nn.functional.unfold((img - mean) / std, kernel_size=patch, stride=patch).transpose(1, 2)
    return rows.reshape(Fr * g * g, 3 * patch * patch)


def patchify_emulation(video, size, patch, Kp, out_dtype, fault=None):
    """patchify_kernel in fp32 numpy, operation by operation (no contraction).  video: fp32 [F, Hin, Win, 3], or uint8 (each tap
    converted as (float)v / 255.0f).  fault="swap_hw": the scales take the other axis' extent."""
    v = video.numpy()
    Fr, Hin, Win, _ = v.shape
    if v.dtype == np.uint8:
        v = v.astype(F32) / F32(255.0)
    sh, sw = F32(Hin) / F32(size), F32(Win) / F32(size)
    if fault == "swap_hw":
        sh, sw = sw, sh
    o = np.arange(size, dtype=F32)
    fy = np.maximum(sh * (o + F32(0.5)) - F32(0.5), F32(0))
    fx = np.maximum(sw * (o + F32(0.5)) - F32(0.5), F32(0))
    y0, x0 = np.minimum(fy.astype(np.int64), Hin - 1), np.minimum(fx.astype(np.int64), Win - 1)
    y1, x1 = np.minimum(y0 + 1, Hin - 1), np.minimum(x0 + 1, Win - 1)
    ly, lx = (fy - y0.astype(F32))[None, :, None, None], (fx - x0.astype(F32))[None, None, :, None]
    hy, hx = F32(1) - ly, F32(1) - lx
    p00, p01 = v[:, y0][:, :, x0], v[:, y0][:, :, x1]
    p10, p11 = v[:, y1][:, :, x0], v[:, y1][:, :, x1]
    val = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11)                       # [F, size, size, 3]
    val = (val - np.array(MEAN, dtype=F32)) / np.array(STD, dtype=F32)
    g = size // patch
    rows = val.reshape(Fr, g, patch, g, patch, 3).transpose(0, 1, 3, 5, 2, 4).reshape(Fr * g * g, 3 * patch * patch)
    out = np.zeros((Fr * g * g, Kp), dtype=F32)
    out[:, :3 * patch * patch] = rows
    return torch.from_numpy(out).to(out_dtype)


# =========================================================================================== point features
POINT_COUNTS = [1, 3, 4, 5, 333]
TINY = 2.0 ** -12
_PLANTED_XYZ = [(0.0, 0.0, 0.0), (0.5, -0.5, TINY), (-TINY, 0.0, 0.5), (-0.5, TINY, -TINY)]


def point_coordinates(P):
    """[P, 3] fp32: row 0 is the origin, rows 1..3 hold +-0.5 and +-2^-12, the rest is uniform in [-0.5, 0.5]"""
    xyz = torch.rand((P, 3), generator=_gen("points", P)) - 0.5
    n = min(P, len(_PLANTED_XYZ))
    xyz[:n] = torch.tensor(_PLANTED_XYZ[:n])
    return xyz.contiguous()


def point_encode_reference(xyz):
    """(proj, ref): the fp32 products xyz * fl32(2^j pi) the kernel hands to sinf / cosf, and [sin | cos | xyz] of them in fp64"""
    e = (2.0 ** torch.arange(8, dtype=torch.float32)) * math.pi
    proj = torch.cat([xyz[:, i:i + 1] * e for i in range(3)], dim=1)
    return proj, torch.cat([proj.double().sin(), proj.double().cos(), xyz.double()], dim=1)


def point_encode_emulation(xyz, out_dtype):
    proj, _ = point_encode_reference(xyz)
    out = torch.zeros((xyz.shape[0], 64), dtype=torch.float32)
    out[:, :24], out[:, 24:48], out[:, 48:51] = torch.sin(proj), torch.cos(proj), xyz
    return out.to(out_dtype)


ZERO_POINT_ROW = [0.0] * 24 + [1.0] * 24 + [0.0] * 16                  # xyz = 0: sin 0 | cos 0 | 0 0 0 | padding
POINT_CONCAT_CASES = [(C, Kp, P) for C, Kp in ((192, 198), (192, 256), (768, 832), (4, 12)) for P in (1, 257)]
DINO_CLS_CASES = [(1, 1, 4), (3, 5, 192), (2, 257, 768), (5, 2, 1024)]
SENTINEL = -3.25


def point_concat_inputs(C, Kp, P):
    g = _gen("concat", C, Kp, P)
    return torch.randn((P, 3), generator=g), torch.rand((P, 3), generator=g)


def cls_inputs(C):
    g = _gen("cls", C)
    return torch.randn((C,), generator=g), torch.randn((C,), generator=g)


# =========================================================================================== token assembly
# (B, T, K, P, C).  (1, 3, 1, 2, 768): 21 rows, the last workgroup owns one; (2, 1, 3, 5, 1024): T = 1 (no spr rows), the widest
# row, all four float4 slots of a lane; (1, 2, 2, 3, 196): 49 of 64 lanes hold a float4, 18 rows; the last is the first tests' shape.
ASSEMBLE_CASES = [(1, 3, 1, 2, 768), (2, 1, 3, 5, 1024), (1, 2, 2, 3, 196), (2, 3, 8, 16, 192)]
ASSEMBLE_MODES = ["normalised", "raw", "dropout"]
ASSEMBLE_GATE = 1e-6
DROP_P, DROP_SEED = 0.3, 0xDEADBEEFCAFE1234
EPS_DINO, EPS_IN = 1e-6, 1e-5


def assemble_inputs(B, T, K, P, C):
    g = _gen("assemble", B, T, K, P, C)
    r = lambda *s: torch.randn(s, generator=g)
    return dict(dino_x=r(B * T * (P + 1), C) * 2, dw=1 + 0.1 * r(C), db=0.1 * r(C), pos=r(T * P, C), sp0=r(4, C), spr=r(4, C),
                mesh=r(B * K, C), lw=1 + 0.1 * r(C))


def dropout_keep(B, T, P, C):
    from motion324_amd import synth
    return torch.from_numpy(synth.dropout_keep(DROP_SEED, B * T * P * C, DROP_P)).reshape(B, T, P, C)


def _assemble(inp, B, T, K, P, C, dt, ln, drop, lw, fault):
    c = lambda t: t.to(dt)
    dn = ln(c(inp["dino_x"]).reshape(B, T, P + 1, C)[:, :, 1:], c(inp["dw"]), c(inp["db"]), EPS_DINO)
    vid = dn + c(inp["pos"]).reshape(1, T, P, C)
    if drop:
        keep = dropout_keep(B, T, P, C)
        scale = 1.0 / (1.0 - DROP_P) if dt == torch.float64 else float(F32(1) / (F32(1) - F32(DROP_P)))
        vid = torch.where(keep, vid * scale, torch.zeros_like(vid))
    first = inp["spr"] if fault == "spr_in_frame0" else inp["sp0"]
    special = torch.stack([c(first)] + [c(inp["spr"])] * (T - 1), dim=0).unsqueeze(0).expand(B, -1, -1, -1)
    tok = torch.cat([special, c(inp["mesh"]).reshape(B, 1, K, C).expand(-1, T, -1, -1), vid], dim=2)
    out = (ln(tok, c(inp["lw"]), None, EPS_IN) if lw else tok).reshape(-1, C).clone()
    if fault == "last_row_unwritten":
        out[-1] = 0.0
    return out


def assemble_reference(inp, B, T, K, P, C, *, drop=False, lw=True):
    """fp64 construction of the first test (tests/test_kernels_gpu.py::test_assemble_tokens) -> [B T (4 + K + P), C]"""
    ln = lambda x, w, b, eps: torch.nn.functional.layer_norm(x, (C,), w, b, eps)
    return _assemble(inp, B, T, K, P, C, torch.float64, ln, drop, lw, None)


def assemble_emulation(inp, B, T, K, P, C, *, drop=False, lw=True, fault=None):
    """assemble_kernel in fp32: two-pass row statistics (the mean, then the centred squares), rsqrt, (x - mean) rstd w + b + pos,
    the keep-mask scaled by fl32(1 / (1 - p)), the input LayerNorm without bias"""
    def ln(x, w, b, eps):
        mean = x.sum(-1, keepdim=True) / C
        xc = x - mean
        rstd = torch.rsqrt((xc * xc).sum(-1, keepdim=True) / C + eps)
        y = xc * rstd * w
        return y if b is None else y + b
    return _assemble(inp, B, T, K, P, C, torch.float32, ln, drop, lw, fault)


def row_rel_err(out, ref):
    """per token row: |out - ref|_2 / |ref|_2 over C -- one wrong row is not averaged away by the others"""
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    assert out.shape == ref.shape, (tuple(out.shape), tuple(ref.shape))
    err = (out - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-30)
    return torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)


# =========================================================================================== 3-wide head
# (M, K): one row, one float4 (63 idle lanes); 16 lanes; 63 lanes; 260: lane 0 alone takes a second step; 768; 2048: eight steps
LINEAR_N3_CASES = [(1, 4), (3, 64), (5, 252), (6, 260), (9, 768), (7, 2048)]


def linear_n3_inputs(M, K, dtype):
    g = _gen("n3", M, K)
    a = torch.randn((M, K), generator=g).to(dtype).float()               # the values the kernel reads
    return a, torch.randn((3, K), generator=g) * 0.05, torch.randn((3,), generator=g)


def linear_n3_reference(a, w, bias):
    return a.double() @ w.double().T + bias.double()


def linear_n3_emulation(a, w, bias, fault=None):
    """linear_n3_kernel in fp32: lane l owns columns 4 l + 256 s .. + 3 of step s; per step a four-term dot added to the lane's sum;
    the 64 lane sums meet in six butterfly levels; + bias.  fault="drop_step": lane 5 skips its last step."""
    a, w = a.numpy().astype(F32), w.numpy().astype(F32)
    M, K = a.shape
    steps = -(-K // 256)
    ap, wp = np.zeros((M, steps * 256), dtype=F32), np.zeros((3, steps * 256), dtype=F32)
    ap[:, :K], wp[:, :K] = a, w
    ap, wp = ap.reshape(M, 1, steps, 64, 4), wp.reshape(1, 3, steps, 64, 4)
    lane = np.zeros((M, 3, 64), dtype=F32)
    for s in range(steps):
        pr = ap[:, :, s] * wp[:, :, s]                                                  # [M, 3, 64, 4]
        dot = ((pr[..., 0] + pr[..., 1]) + pr[..., 2]) + pr[..., 3]
        if fault == "drop_step" and s == (K - 24) // 256:                                # lane 5's last step (columns 20 + 256 s ..)
            dot[:, :, 5] = 0
        lane = lane + dot
    while lane.shape[-1] > 1:
        lane = lane[..., 0::2] + lane[..., 1::2]
    return torch.from_numpy(lane[..., 0] + bias.numpy().astype(F32))


# =========================================================================================== trajectory filters
# (B, T, N).  B N = 513 and B T N = 4617: both past a 256 boundary, unevenly; T = 1; T = 2 with 600 points; 257 points, T = 40
TRAJ_SHAPES = [(3, 9, 171), (1, 1, 5), (2, 2, 300), (1, 40, 257)]
THR = 2.0 ** -8
SIGMAS = [0.1, 1.0, 3.0]                     # radius 0 (the filter is the identity), 4, 12 (> T = 9)
SAVGOL_CASES = [(5, 2, 5), (9, 3, 9), (8, 3, 9), (5, 2, 40), (5, 2, 2)]          # (window, polyorder, T)
ONEEURO_PARAMS = [(1.0, 0.007), (0.3, 0.5)]
SMOOTH_GATE = 2e-6
PLANTED_N = 3                                # points 0, 1, 2 of batch item 0 (T >= 8 only)


def trajectories(B, T, N):
    """(trajs fp32 [B, T, N, 3] numpy, planted: bool).  The recipe of tests/golden/make_smooth_golden.py -- a base in [-0.5, 0.5]
    plus the running sum of small steps, every fifth frame four times larger -- with every step whose length lies between 0.45
    and 2.2 thresholds moved out of that band (the shorter ones to 0.4, the others to 2.5 thresholds): the fp32 displacement
    the kernel forms is then below THR / 2 or above 2 THR, and `norm < THR` falls the same way however the squares are summed.
    Batch items get different data.  T >= 8: three planted points in batch item 0, coordinates and steps on the 2^-12 grid --
      point 0: one step (THR, 0, 0) at t = 1: the norm IS the threshold, `<` is false, the point moves;
      point 1: one step (THR / 2, 0, 0): held at its first position for good;
      point 2: five steps of THR / 2, held, then one of 2 THR: jumps to the true position."""
    g = _gen("traj", B, T, N)
    base = torch.rand((B, 1, N, 3), generator=g, dtype=torch.float64) - 0.5
    steps = torch.randn((B, T, N, 3), generator=g, dtype=torch.float64) * 0.004
    steps[:, ::5] *= 4
    norm = steps.norm(dim=-1, keepdim=True)
    band = (norm > 0.45 * THR) & (norm < 2.2 * THR)
    target = torch.where(norm < THR, torch.full_like(norm, 0.4 * THR), torch.full_like(norm, 2.5 * THR))
    steps = torch.where(band, steps * target / norm, steps)
    x = (base + torch.cumsum(steps, dim=1)).float().numpy()
    planted = T >= 8
    if planted:
        for n in range(PLANTED_N):
            p0 = np.array([(100 + 37 * n) * TINY, -(900 + n) * TINY, (n - 1) * 511 * TINY], dtype=F32)
            dx = np.zeros(T, dtype=F32)
            if n == 0:
                dx[1:] = THR
            elif n == 1:
                dx[1:] = THR / 2
            else:
                dx[1:6] = np.arange(1, 6) * (THR / 2)
                dx[6:] = 5 * (THR / 2) + 2 * THR
            x[0, :, n] = p0
            x[0, :, n, 0] += dx
    return np.ascontiguousarray(x), planted


def random_displacement_norms(x, planted):
    """fp64 norms of the frame-to-frame displacements of the fp32 positions, the planted points left out"""
    d = np.linalg.norm(np.diff(x.astype(np.float64), axis=1), axis=-1)                # [B, T - 1, N]
    keep = np.ones(d.shape, dtype=bool)
    if planted:
        keep[0, :, :PLANTED_N] = False
    return d[keep]


def planted_outcome(x):
    """what the threshold pass leaves of the three planted points: [T, 3, 3]"""
    T = x.shape[1]
    want = x[0, :, :PLANTED_N].copy()
    want[:, 1] = x[0, 0, 1]
    want[:6, 2] = x[0, 0, 2]
    assert T >= 8
    return want


def threshold_emulation(x, thr, fault=None):
    """smooth_threshold_kernel in fp32.  faults: "le" (`<=` for `<`), "batch_stride0" (every batch item reads item 0)"""
    x = np.asarray(x, dtype=F32)
    if fault == "batch_stride0":
        x = np.broadcast_to(x[:1], x.shape)
    out = x.copy()
    for t in range(1, x.shape[1]):
        d = x[:, t] - x[:, t - 1]
        n = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        still = (thr >= 0) & ((n <= F32(thr)) if fault == "le" else (n < F32(thr)))
        out[:, t] = np.where(still[..., None], out[:, t - 1], x[:, t])
    return out


def gauss_emulation(x, sigma, fault=None):
    """smooth_gauss_kernel in fp32: expf weights divided by their fp32 sum, taps added in order, clamped indices.
    fault="wrap": indices taken modulo T"""
    x = np.asarray(x, dtype=F32)
    T = x.shape[1]
    radius = int(F32(4.0) * F32(sigma) + F32(0.5))
    s = F32(sigma)
    wts = [np.exp(F32(-0.5) * F32(r * r) / (s * s), dtype=F32) for r in range(-radius, radius + 1)]
    wsum = F32(0)
    for w in wts:
        wsum = F32(wsum + w)
    acc = np.zeros_like(x)
    t = np.arange(T)
    for r, w in zip(range(-radius, radius + 1), wts):
        tt = (t + r) % T if fault == "wrap" else np.clip(t + r, 0, T - 1)
        acc = acc + F32(w / wsum) * x[:, tt]
    return acc


def smooth_emulation(x, thr, sigma, fault=None):
    out = threshold_emulation(x, thr, fault if fault in ("le", "batch_stride0") else None)
    return gauss_emulation(out, sigma, fault if fault == "wrap" else None) if sigma > 0 else out


def savgol_emulation(x, window, polyorder, fault=None):
    """postprocess.smooth_trajectories(method="savgol") + smooth_fir_kernel: fp64 taps, one rounding"""
    from motion324_amd.postprocess import savgol_coeffs
    x = np.asarray(x, dtype=F32)
    T = x.shape[1]
    if window % 2 == 0:
        window += 1
    if T < window:
        return x.copy()
    coef = savgol_coeffs(window, min(polyorder, window - 1))
    src = np.broadcast_to(x[:1], x.shape) if fault == "batch_stride0" else x
    h, t = window // 2, np.arange(T)
    acc = np.zeros(x.shape, dtype=np.float64)
    for j in range(window):
        acc += coef[j] * src[:, np.clip(t + h - j, 0, T - 1)].astype(np.float64)
    return acc.astype(F32)


def oneeuro_emulation(x, mincutoff, beta, fault=None):
    """smooth_oneeuro_kernel: fp64 state, the first difference in fp32, the parameters as the fp32 values the entry point takes"""
    x = np.asarray(x, dtype=F32)
    src = np.broadcast_to(x[:1], x.shape) if fault == "batch_stride0" else x
    mc, bt = float(F32(mincutoff)), float(F32(beta))
    rd = 2 * math.pi * 1.0
    alpha_d = rd / (rd + 1.0)
    out = src.copy()
    x_prev, dx_prev = src[:, 0].astype(np.float64), np.zeros(src[:, 0].shape)
    for t in range(1, x.shape[1]):
        xt = src[:, t].astype(np.float64)
        dx = (src[:, t] - src[:, 0]).astype(np.float64) if t == 1 else xt - x_prev
        dx_hat = alpha_d * dx + (1.0 - alpha_d) * dx_prev
        r = 2 * math.pi * (mc + bt * np.abs(dx_hat))
        alpha = r / (r + 1.0)
        x_prev = alpha * xt + (1.0 - alpha) * x_prev
        dx_prev = dx_hat
        out[:, t] = x_prev.astype(F32)
    return out


# =========================================================================================== nearest point
# (n_query, n_ref): one of each; a full workgroup less one lane against a tile less one point; one lane and one point more than
# full; 300 queries against two tiles and 452 points.  LDS tiles hold 1024 reference points, a workgroup 256 queries.
NEAREST_CASES = [(1, 1), (255, 1023), (257, 1025), (300, 2500)]
NEAREST_SLACK = 16 * 2.0 ** -24
TIE_BASE = 1100
TIE_EXACT = [0, 1, 500, 1023, 1024, 1025, 1099]


def nearest_inputs(nq, nr):
    """(query [nq, 3], ref [nr, 3]) fp32 in the centred unit cube.  The last reference point lies 2^-10 from the last query --
    for nr > 1 the answer of the last lane of the last workgroup is the last point of the last (partial) tile."""
    g = _gen("nearest", nq, nr)
    q, r = torch.rand((nq, 3), generator=g) - 0.5, torch.rand((nr, 3), generator=g) - 0.5
    if nr > 1:
        r[-1] = q[-1] + torch.tensor([2.0 ** -10, 0.0, -(2.0 ** -11)])
    return q.contiguous(), r.contiguous()


def nearest_tie_inputs():
    """ref = [base; base[perm]], 1100 base points, perm the rotation by 76 = 1100 - 1024: the copy of base[i] stands at
    1100 + (i - 76) mod 1100, in ANOTHER LDS tile of 1024 than base[i] for every i (i < 76: tile 2; i < 1024: tile 1 or 2 against
    0; i >= 1024: tile 2 against 1), and the lowest index of every pair is < 1100.  Queries: base[i] itself for i in TIE_EXACT
    (distance 0 to base[i] and to its copy), then random points."""
    g = _gen("nearest-ties")
    base = torch.rand((TIE_BASE, 3), generator=g) - 0.5
    perm = (torch.arange(TIE_BASE) + 76) % TIE_BASE
    q = torch.cat([base[TIE_EXACT], torch.rand((293, 3), generator=g) - 0.5])
    return q.contiguous(), torch.cat([base, base[perm]]).contiguous()


def squared_distances(q, r):
    """fp64 [nq, nr] from the fp32 coordinates"""
    d = q.double()[:, None, :] - r.double()[None, :, :]
    return (d * d).sum(-1)


def nearest_emulation(q, r, fault=None):
    """nearest_point_kernel in fp32: d = dx dx + dy dy + dz dz of fp32 differences, tile after tile, `d < best` keeps the lowest
    index.  fault="skip_partial_tile": the reference points behind the last full tile of 1024 are never looked at."""
    q, r = q.numpy().astype(F32), r.numpy().astype(F32)
    nr = r.shape[0]
    if fault == "skip_partial_tile":
        nr = nr // 1024 * 1024
    best = np.full(q.shape[0], np.inf, dtype=F32)
    besti = np.zeros(q.shape[0], dtype=np.int64)
    for r0 in range(0, nr, 1024):
        d = r[None, r0:min(r0 + 1024, nr)] - q[:, None]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        j = d2.argmin(axis=1)                                                          # numpy: the first minimum
        m = d2[np.arange(q.shape[0]), j]
        better = m < best
        best, besti = np.where(better, m, best), np.where(better, r0 + j, besti)
    return torch.from_numpy(besti)


def nearest_gate(index, d2, what):
    """EVERY query: the index is in range and the chosen point's fp64 squared distance is <= (1 + 16 U32) the fp64 minimum.
    Returns the largest chosen / minimum - 1 (a record)."""
    index = index.detach().cpu().long()
    nq, nr = d2.shape
    assert index.shape == (nq,), (what, tuple(index.shape))
    assert int(index.min()) >= 0 and int(index.max()) < nr, (what, int(index.min()), int(index.max()))
    chosen, best = d2.gather(1, index[:, None])[:, 0], d2.min(dim=1).values
    bad = ~(chosen <= (1 + NEAREST_SLACK) * best)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {nq} queries took a point farther than the nearest; first "
                                 f"{[(int(i), int(index[i]), int(d2[i].argmin())) for i in bad.nonzero()[:8, 0]]} (query, got, want)")
    return float(((chosen - best) / best.clamp_min(1e-300)).max())
