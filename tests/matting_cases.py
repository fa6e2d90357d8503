"""Cases, oracle and gates of the matting tests (tests/test_matting_cpu.py, tests/test_matting_gpu.py,
tests/golden/make_matting_band.py).

The oracle is a torch CPU model of U2-Net written from its definition (REBNCONV = conv2d with dilation, eval-mode batch-norm
NOT folded, ReLU; max_pool2d with ceil_mode; interpolate bilinear align_corners=False) at a chosen precision.  Six faults can be
planted into it; the CPU tests require the gate to see each of them.  Around it the host model of what `rembg` does: numpy for
the normalisation and the quantisation, the resampling model of tests/framing_cases.py for the resizes, and the cut-out table.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import framing_cases as FC
from motion324_amd import matting as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matting_band.npz")
WEIGHT_SEED = {"u2net": 2320, "u2netp": 2321}
# With unit side weights the seeded logits reach some tens and the matte saturates.  These scale the side weights and centre the logits
# so that every frame keeps a wide range without plateaus: the conditions of the quantised-mask check (tests/ERROR_BOUNDS_MATTING.md)
SIDE_GAIN = {"u2net": 0.05, "u2netp": 0.045}
OUTCONV_BIAS = {"u2net": 0.4, "u2netp": -1.2}
# The oracle's own reading of the published module, independent of the tables of motion324_amd/matting.py: the block of every stage,
# and the dilation of every REBNCONV of a block
STAGE_KIND = {"stage1": 7, "stage2": 6, "stage3": 5, "stage4": 4, "stage5": "4F", "stage6": "4F",
              "stage5d": "4F", "stage4d": 4, "stage3d": 5, "stage2d": 6, "stage1d": 7}
RSU4F_DILATION = {"rebnconvin": 1, "rebnconv1": 1, "rebnconv2": 2, "rebnconv3": 4, "rebnconv4": 8, "rebnconv3d": 4, "rebnconv2d": 2, "rebnconv1d": 1}


def oracle_dilation(kind, name):
    """RSU-4F: 1, 1, 2, 4, 8, 4, 2, 1; RSU-L: 2 for rebnconv<L>, the layer without a pool in front of it, and 1 everywhere else"""
    if kind == "4F":
        return RSU4F_DILATION[name]
    return 2 if name == f"rebnconv{kind}" else 1


GATE_FACTOR = 8.0           # times the recorded deviation of the fp32 CPU run; the reason is in tests/ERROR_BOUNDS_MATTING.md
U32 = 2.0 ** -24
FAULTS = ("rebnconv7_dilation1", "swapped_cat", "floor_pool", "align_corners", "no_residual", "side6_from_hx5d")
TENSORS = ("d0",) + M.TAPS
SIGMOID_ERROR = 8 * U32     # fp32 1 / (1 + expf(-x)): expf within 4 U32 of exp, the sum and the quotient one rounding each, p <= 1
MAX_AMBIGUOUS = 0.05        # of a case's pixels may lie within delta of an integer
MIN_RANGE = 0.3             # of max p - min p per frame

# name: (variant, size, T).  37 -> 19, 10, 5, 3, 2 exercises the ceil-mode pool and non-integer upsampling
CASES = {f"{variant}_{size}x{T}": (variant, size, T) for variant in ("u2net", "u2netp") for size in (40, 37) for T in (1, 3)}

_CACHE = {}


def state_dict(variant):
    if ("sd", variant) not in _CACHE:
        _CACHE["sd", variant] = M.synth_u2net_state_dict(variant, WEIGHT_SEED[variant], SIDE_GAIN[variant], OUTCONV_BIAS[variant])
    return _CACHE["sd", variant]


def frames(name):
    """uint8 [T,size,size,3] numpy of a case: smooth content plus texture, seeded by the case's position"""
    _, size, T = CASES[name]
    rng = np.random.default_rng(3000 + list(CASES).index(name))
    yy, xx = np.meshgrid(np.linspace(0, 1, size), np.linspace(0, 1, size), indexing="ij")
    base = np.stack([np.sin(5.0 * xx + c + t) * np.cos(4.0 * yy - t) for t in range(T) for c in range(3)]).reshape(T, 3, size, size)
    blob = np.exp(-((xx - 0.5) ** 2 + (yy - 0.45) ** 2) / 0.05)
    a = 110 + 60 * base.transpose(0, 2, 3, 1) + 70 * blob[None, :, :, None] + rng.normal(0, 20, (T, size, size, 3))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ what rembg does, on the host
def model_prepare(small):
    """fp32 [T,S,S',4] from uint8 [T,S,S',3]: rembg's normalisation, float64 rounded once, and a zero fourth channel"""
    out = np.zeros(small.shape[:3] + (4,), dtype=np.float32)
    for t in range(small.shape[0]):
        im = small[t] / max(np.max(small[t]), 1e-6)
        for c in range(3):
            out[t, :, :, c] = ((im[:, :, c] - M.MEAN[c]) / M.STD[c]).astype(np.float32)
    return out


def model_quantise(p):
    """uint8 [T,S,S] from probabilities [T,S,S] of either precision, the arithmetic in the array's own; a constant frame gives 0"""
    q = np.zeros(p.shape, dtype=np.uint8)
    for t in range(p.shape[0]):
        ma, mi = p[t].max(), p[t].min()
        if ma > mi:
            q[t] = (((p[t] - mi) / (ma - mi)) * p.dtype.type(255)).astype(np.uint8)
    return q


def model_cutout_table():
    """uint8 [256,256] of (mask byte, colour byte): Pillow's composite, t = v a + 128, (t + (t >> 8)) >> 8, then the soft masking of
    tests/framing_cases.py with the composite's own alpha"""
    table = np.zeros((256, 256), dtype=np.uint8)
    soft = FC.model_soft_table()
    for a in range(256):
        ta = 255 * a + 128
        alpha = (ta + (ta >> 8)) >> 8
        for v in range(256):
            t = v * a + 128
            table[a, v] = soft[alpha, (t + (t >> 8)) >> 8]
    return table


def model_from_mask(mask320, video):
    """(alpha [T,H,W], masked_frames [T,H,W,3], masks fp32 [T,H,W,1]) of a quantised mask [T,S,S] and the frames [T,H,W,3]: steps 5
    and 6, and the reference's mask"""
    H, W = video.shape[1:3]
    alpha = FC.model_resize(mask320[..., None], W, H)[..., 0]
    if "table" not in _CACHE:
        _CACHE["table"] = model_cutout_table()
    masked = _CACHE["table"][alpha[..., None], video]
    return alpha, masked, (alpha[..., None] / 255.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the oracle
def _oracle_net(state, variant, x, dtype, fault):
    P = lambda key: state[key].to(dtype)

    def rebn(prefix, x, dilation):
        if fault == "rebnconv7_dilation1" and prefix.endswith(".rebnconv7"):
            dilation = 1
        x = F.conv2d(x, P(prefix + ".conv_s1.weight"), P(prefix + ".conv_s1.bias"), padding=dilation, dilation=dilation)
        x = F.batch_norm(x, P(prefix + ".bn_s1.running_mean"), P(prefix + ".bn_s1.running_var"), P(prefix + ".bn_s1.weight"),
                         P(prefix + ".bn_s1.bias"), training=False, eps=1e-5)
        return F.relu(x)

    def cat(a, b):
        return torch.cat((b, a) if fault == "swapped_cat" else (a, b), dim=1)

    def pool(x):
        if fault == "floor_pool" and min(x.shape[2:]) >= 2:
            return F.max_pool2d(x, 2, 2, ceil_mode=False)
        return F.max_pool2d(x, 2, 2, ceil_mode=True)

    def up(a, b):
        if fault == "align_corners":
            return F.interpolate(a, size=b.shape[2:], mode="bilinear", align_corners=True)
        return F.interpolate(a, size=b.shape[2:], mode="bilinear", align_corners=False)

    def rsu(stage, x):
        kind = STAGE_KIND[stage]
        conv = lambda name, x: rebn(f"{stage}.{name}", x, oracle_dilation(kind, name))
        hxin = conv("rebnconvin", x)
        if kind == "4F":
            hx1 = conv("rebnconv1", hxin)
            hx2 = conv("rebnconv2", hx1)
            hx3 = conv("rebnconv3", hx2)
            hx4 = conv("rebnconv4", hx3)
            d = conv("rebnconv3d", cat(hx4, hx3))
            d = conv("rebnconv2d", cat(d, hx2))
            d = conv("rebnconv1d", cat(d, hx1))
        else:
            L = int(kind)
            hx = [None, conv("rebnconv1", hxin)]
            for k in range(2, L):
                hx.append(conv(f"rebnconv{k}", pool(hx[k - 1])))
            d = conv(f"rebnconv{L - 1}d", cat(conv(f"rebnconv{L}", hx[L - 1]), hx[L - 1]))
            for k in range(L - 2, 0, -1):
                d = conv(f"rebnconv{k}d", cat(up(d, hx[k]), hx[k]))
        return d if fault == "no_residual" else d + hxin

    t = {"hx1": rsu("stage1", x)}
    for k in range(2, 7):
        t[f"hx{k}"] = rsu(f"stage{k}", pool(t[f"hx{k - 1}"]))
    d = t["hx6"]
    for k in range(5, 0, -1):
        d = t[f"hx{k}d"] = rsu(f"stage{k}d", cat(up(d, t[f"hx{k}"]), t[f"hx{k}"]))
    sources = [t["hx1d"], t["hx2d"], t["hx3d"], t["hx4d"], t["hx5d"], t["hx5d"] if fault == "side6_from_hx5d" else t["hx6"]]
    sides = [F.conv2d(s, P(f"side{k + 1}.weight"), P(f"side{k + 1}.bias"), padding=1) for k, s in enumerate(sources)]
    sides = [sides[0]] + [up(s, sides[0]) for s in sides[1:]]
    t["d0"] = F.conv2d(torch.cat(sides, dim=1), P("outconv.weight"), P("outconv.bias"))[:, 0]
    return t


def oracle(variant, x_nhwc, dtype=torch.float64, fault=None, state=None):
    """{name: numpy float64} of d0 [T,S,S] and the eleven taps (NHWC), for x fp32 numpy [T,S,S,4] as model_prepare makes it"""
    state = state_dict(variant) if state is None else state
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc[..., :3])).permute(0, 3, 1, 2).to(dtype)
    with torch.no_grad():
        t = _oracle_net(state, variant, x, dtype, fault)
    return {name: (v if name == "d0" else v.permute(0, 2, 3, 1)).double().contiguous().numpy() for name, v in t.items()}


def reference(name):
    """(x fp32 [T,S,S,4], the fp64 oracle's tensors) of a case, computed once"""
    if ("ref", name) not in _CACHE:
        x = model_prepare(frames(name))
        _CACHE["ref", name] = (x, oracle(CASES[name][0], x))
    return _CACHE["ref", name]


def deviation(got, ref):
    """[12]: per tensor of TENSORS the largest |got - ref| relative to the reference tensor's largest magnitude; inf for a tensor of
    another shape"""
    return np.array([np.abs(np.asarray(got[n], dtype=np.float64) - ref[n]).max() / np.abs(ref[n]).max() if got[n].shape == ref[n].shape
                     else np.inf for n in TENSORS])


def golden():
    """{case: band [12]} from tests/golden/matting_band.npz"""
    z = np.load(GOLDEN)
    return {name: z[name] for name in CASES}


def gate(name):
    """[12]: the largest deviation allowed per tensor in a case: GATE_FACTOR times the recorded band, floored at one unit roundoff"""
    return GATE_FACTOR * np.maximum(golden()[name], U32)


# ------------------------------------------------------------------------------------------------ the quantised mask
def sigmoid64(d0):
    return 1.0 / (1.0 + np.exp(-np.asarray(d0, dtype=np.float64)))


def quantised_reference(name):
    """(q float64 [T,S,S] before truncation, delta [T], range [T]) from the fp64 oracle: the derivation of delta is in
    tests/ERROR_BOUNDS_MATTING.md -- e_p = gate(d0) max|d0| / 4 + SIGMOID_ERROR bounds the error of every probability, of mi and of
    ma; delta = 255 * 4 e_p / (R - 2 e_p) + 255 * 4 U32 with R = ma - mi"""
    ref = reference(name)[1]["d0"]
    p = sigmoid64(ref)
    e_p = gate(name)[0] * np.abs(ref).max() / 4.0 + SIGMOID_ERROR
    mi, ma = p.min(axis=(1, 2)), p.max(axis=(1, 2))
    R = ma - mi
    q = (p - mi[:, None, None]) / R[:, None, None] * 255.0
    return q, 255.0 * 4.0 * e_p / (R - 2.0 * e_p) + 255.0 * 4.0 * U32, R


def check_quantised(name, got):
    """(ambiguous fraction, mismatches outside the zone, pixels off by more than one level) of a uint8 mask against the fp64 one"""
    q, delta, _ = quantised_reference(name)
    ambiguous = np.abs(q - np.rint(q)) <= delta[:, None, None]
    want = np.floor(q).astype(np.int64)
    diff = np.abs(got.astype(np.int64) - want)
    return float(ambiguous.mean()), int((diff[~ambiguous] != 0).sum()), int((diff > 1).sum())
