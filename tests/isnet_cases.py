"""Cases, oracle and gates of the ISNet tests (tests/test_isnet_cpu.py, tests/test_isnet_gpu.py, tests/golden/make_isnet_band.py).

The oracle is a torch CPU model of ISNetDIS written from its definition: conv_in = conv2d(stride=2, padding=1) with nothing behind
it, the eleven RSU blocks (REBNCONV = conv2d with dilation, eval-mode batch-norm NOT folded, ReLU; max_pool2d with ceil_mode;
interpolate bilinear align_corners=False), side1 on hx1d, and d1 = that map resized to the network input.  Its block structure is
its own (STAGE_KIND and oracle_dilation of tests/matting_cases.py, which are that file's reading of the RSU blocks), not the tables
of motion324_amd/matting.py.  Eight faults can be planted into it; the CPU tests require the gate to see each of them.  Around it
the host model of what `rembg`'s DIS session does, with that session's constants as this file reads them.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import matting_cases as MC
from motion324_amd import matting as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "isnet_band.npz")
WEIGHT_SEED = 2330
SIDE_GAIN, SIDE_BIAS = 1.0, 0.0         # unit side weights: d1 reads one map of a 64-channel tensor and stays within a few units
MEAN, STD = (0.485, 0.456, 0.406), (1.0, 1.0, 1.0)
GATE_FACTOR, U32, SIGMOID_ERROR, MAX_AMBIGUOUS, MIN_RANGE = MC.GATE_FACTOR, MC.U32, MC.SIGMOID_ERROR, MC.MAX_AMBIGUOUS, MC.MIN_RANGE
FAULTS = ("conv_in_stride1", "conv_in_relu", "pool_in", "floor_pool", "align_corners", "swapped_cat", "no_residual", "d1_from_side2")
TENSORS = ("d1", "hxin") + M.TAPS
# name: (size, T).  40 -> 20 behind the stem, then 10, 5, 3, 2, 1; 37 -> 19 (an odd stem output), 10, 5, 3, 2, 1, and the last
# upsample is 19 -> 37, no factor of two.  stage6 runs on 1 x 1 maps in both.
CASES = {f"isnet_{size}x{T}": (size, T) for size in (40, 37) for T in (1, 3)}

_CACHE = {}


def state_dict():
    if "sd" not in _CACHE:
        _CACHE["sd"] = M.synth_isnet_state_dict(WEIGHT_SEED, SIDE_GAIN, SIDE_BIAS)
    return _CACHE["sd"]


def frames(name):
    """uint8 [T,size,size,3]: the frames of tests/matting_cases.py for the same size and length"""
    size, T = CASES[name]
    return MC.frames(f"u2net_{size}x{T}")


def model_prepare(small, mean=MEAN, std=STD):
    """fp32 [T,S,S',4] from uint8 [T,S,S',3]: the normalisation with given constants, float64 rounded once, a zero fourth channel"""
    out = np.zeros(small.shape[:3] + (4,), dtype=np.float32)
    for t in range(small.shape[0]):
        im = small[t] / max(np.max(small[t]), 1e-6)
        for c in range(3):
            out[t, :, :, c] = ((im[:, :, c] - mean[c]) / std[c]).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the oracle
def _oracle_net(state, x, dtype, fault):
    P = lambda key: state[key].to(dtype)

    def rebn(prefix, x, dilation):
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

    def up(a, size):
        return F.interpolate(a, size=size, mode="bilinear", align_corners=fault == "align_corners")

    def rsu(stage, x):
        kind = MC.STAGE_KIND[stage]
        conv = lambda name, x: rebn(f"{stage}.{name}", x, MC.oracle_dilation(kind, name))
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
                d = conv(f"rebnconv{k}d", cat(up(d, hx[k].shape[2:]), hx[k]))
        return d if fault == "no_residual" else d + hxin

    hxin = F.conv2d(x, P("conv_in.weight"), P("conv_in.bias"), stride=1 if fault == "conv_in_stride1" else 2, padding=1)
    if fault == "conv_in_relu":
        hxin = F.relu(hxin)
    if fault == "pool_in":
        hxin = F.max_pool2d(hxin, 2, 2, ceil_mode=True)
    t = {"hxin": hxin, "hx1": rsu("stage1", hxin)}
    for k in range(2, 7):
        t[f"hx{k}"] = rsu(f"stage{k}", pool(t[f"hx{k - 1}"]))
    d = t["hx6"]
    for k in range(5, 0, -1):
        d = t[f"hx{k}d"] = rsu(f"stage{k}d", cat(up(d, t[f"hx{k}"].shape[2:]), t[f"hx{k}"]))
    n = 2 if fault == "d1_from_side2" else 1
    side = F.conv2d(t[f"hx{n}d"], P(f"side{n}.weight"), P(f"side{n}.bias"), padding=1)
    t["d1"] = up(side, x.shape[2:])[:, 0]
    return t


def oracle(x_nhwc, dtype=torch.float64, fault=None, state=None):
    """{name: numpy float64} of d1 [T,S,S] and the twelve taps (NHWC), for x fp32 numpy [T,S,S,4] as model_prepare makes it"""
    state = state_dict() if state is None else state
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc[..., :3])).permute(0, 3, 1, 2).to(dtype)
    with torch.no_grad():
        t = _oracle_net(state, x, dtype, fault)
    return {name: (v if name == "d1" else v.permute(0, 2, 3, 1)).double().contiguous().numpy() for name, v in t.items()}


def reference(name):
    """(x fp32 [T,S,S,4], the fp64 oracle's tensors) of a case, computed once"""
    if ("ref", name) not in _CACHE:
        x = model_prepare(frames(name))
        _CACHE["ref", name] = (x, oracle(x))
    return _CACHE["ref", name]


def fp32_run(name):
    """the oracle's own fp32 CPU run of a case, computed once"""
    if ("f32", name) not in _CACHE:
        _CACHE["f32", name] = oracle(reference(name)[0], torch.float32)
    return _CACHE["f32", name]


def deviation(got, ref):
    """[13]: per tensor of TENSORS the largest |got - ref| relative to the reference tensor's largest magnitude; inf for a tensor of
    another shape"""
    return np.array([np.abs(np.asarray(got[n], dtype=np.float64) - ref[n]).max() / np.abs(ref[n]).max() if got[n].shape == ref[n].shape
                     else np.inf for n in TENSORS])


def golden():
    """{case: band [13]} from tests/golden/isnet_band.npz"""
    z = np.load(GOLDEN)
    return {name: z[name] for name in z.files}


def gate(name):
    """[13]: the largest deviation allowed per tensor in a case: GATE_FACTOR times the recorded band, floored at one unit roundoff"""
    return GATE_FACTOR * np.maximum(golden()[name], U32)


# ------------------------------------------------------------------------------------------------ the quantised mask
def quantised_reference(name):
    """(q float64 [T,S,S] before truncation, delta [T], range [T]) from the fp64 oracle: tests/matting_cases.quantised_reference with
    d1 in place of d0 -- e_p = gate(d1) max|d1| / 4 + SIGMOID_ERROR; delta = 255 * 4 e_p / (R - 2 e_p) + 255 * 4 U32, R = ma - mi"""
    ref = reference(name)[1]["d1"]
    p = MC.sigmoid64(ref)
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
