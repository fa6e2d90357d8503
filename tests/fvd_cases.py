"""Cases, oracle and gate of the FVD tests (tests/test_fvd_cpu.py, tests/test_fvd_gpu.py, tests/golden/make_fvd_band.py).

The oracle is a torch CPU model of I3D written from its definition: F.conv3d and F.max_pool3d at a chosen precision with explicit
F.pad by the TensorFlow "SAME" rule (the max-pool pads with -inf), unfolded batch norm with eps 1e-3, the head as an average
pool, a 1 x 1 x 1 convolution and a mean.  Five faults can be planted into it; the CPU tests require the gate to see each.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from motion324_amd import fvd as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fvd_band.npz")
WEIGHT_SEED = 324
GATE_FACTOR = 8.0           # times the recorded deviation of the fp32 CPU run; the reason is in tests/ERROR_BOUNDS_FVD.md
FAULTS = ("symmetric_stem_padding", "zero_padded_pool_before_relu", "b1_b2_swapped", "bn_eps_1e-5", "temporal_tap_exchanged")
EXCHANGED_UNIT = "Mixed_4c.b1b"         # a 3 x 3 x 3 in the middle of the trunk
TAPS = V.TAPS
KEYS = TAPS + ("features",)

# name: (N, T, H, W, head window, resolution); resolution None feeds the frames at their own size
CASES = {
    "t10_64": (2, 10, 64, 64, (2, 2, 2), None),         # every time size odd or minimal: 10, 5, 5, 5, 3, 2
    "t16_64": (1, 16, 64, 64, (2, 2, 2), None),
    "t10_224": (1, 10, 224, 224, (2, 7, 7), 224),       # the published window; its oracle runs in the generator only
}
REFUSED = (1, 10, 96, 64, (2, 2, 2), None)              # a final map of 3 x 2 against a 2 x 2 window

_STATE = {}


def state_dict():
    if "sd" not in _STATE:
        _STATE["sd"] = V.synth_i3d_state_dict(WEIGHT_SEED)
    return _STATE["sd"]


def videos(name):
    """uint8 [N,T,H,W,3] numpy of a case, seeded by the case's position: moving smooth content plus texture"""
    N, T, H, W = CASES[name][:4]
    return make_videos(N, T, H, W, 2000 + list(CASES).index(name))


def make_videos(N, T, H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = np.empty((N, T, H, W, 3), np.uint8)
    for n in range(N):
        for t in range(T):
            base = np.stack([np.sin(6.0 * xx + c + 0.3 * t + n) * np.cos(4.0 * yy - 0.2 * t) for c in range(3)], axis=-1)
            out[n, t] = np.clip(np.rint(128 + 70 * base + rng.normal(0, 25, (H, W, 3))), 0, 255).astype(np.uint8)
    return out


def prepared(frames, dtype):
    """[N,3,T,H,W] in [-1, 1] from bytes at their own size, by the formula of the prepare kernel: (v / 255 - 0.5) * 2, each
    operation in fp32 (so that every precision of the oracle starts from the input the kernel sees)"""
    x = torch.from_numpy(np.ascontiguousarray(frames)).permute(0, 4, 1, 2, 3).to(torch.float32)
    return ((x / 255.0 - 0.5) * 2.0).to(dtype).contiguous()


def same_pad(x, window, stride, value=0.0, symmetric=False):
    """x [N,C,T,H,W] padded by the SAME rule for `window` and `stride` (symmetric: the fault, front = ceil(total / 2))"""
    pads = []
    for n, k, s in zip(x.shape[2:], window, stride):
        total = max(k - s, 0) if n % s == 0 else max(k - n % s, 0)
        front = (total + 1) // 2 if symmetric else total // 2
        pads.append((front, total - front))
    return F.pad(x, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]), value=value)


def _unit(state, unit, x, dtype, stride=(1, 1, 1), fault=None, pre_relu=False):
    w = state[f"{unit}.conv3d.weight"].to(dtype)
    if fault == "temporal_tap_exchanged" and unit == EXCHANGED_UNIT:
        w = w.clone()
        w[:, :, 0], w[:, :, 1] = w[:, :, 1].clone(), w[:, :, 0].clone()
    k = w.shape[2]
    x = F.conv3d(same_pad(x, (k, k, k), stride, symmetric=fault == "symmetric_stem_padding" and unit == "Conv3d_1a_7x7"), w, stride=stride)
    gamma = state.get(f"{unit}.bn.weight", torch.ones(w.shape[0])).to(dtype)
    beta, mean, var = (state[f"{unit}.bn.{n}"].to(dtype) for n in ("bias", "running_mean", "running_var"))
    eps = 1e-5 if fault == "bn_eps_1e-5" else V.BN_EPS
    shape = (1, -1, 1, 1, 1)
    x = (x - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + eps) * gamma.reshape(shape) + beta.reshape(shape)
    return x if pre_relu else F.relu(x)


def _pool(x, window, stride, zero_padded=False):
    return F.max_pool3d(same_pad(x, window, stride, value=0.0 if zero_padded else float("-inf")), window, stride)


def oracle(frames, dtype=torch.float64, fault=None, state=None):
    """{tap: [N,T,H,W,C] numpy float64, "features": [N,400]} of uint8 frames [N,T,H,W,3] taken at their own size"""
    state = state_dict() if state is None else state
    return oracle_from(prepared(frames, dtype), dtype, fault, state)


def oracle_from(x, dtype=torch.float64, fault=None, state=None):
    """the same from a prepared input [N,3,T,H,W] in [-1, 1]"""
    state = state_dict() if state is None else state
    out = {}
    with torch.no_grad():
        x = x.to(dtype)
        pool_fault = fault == "zero_padded_pool_before_relu"
        for step in V.TRUNK:
            if step[0] == "conv":
                # the pool fault: Conv3d_2c_3x3 hands its pre-ReLU map to a zero-padded pool.  No ReLU follows: max and ReLU
                # commute, so a ReLU behind the pool would undo the fault exactly, whatever the padding
                late_relu = pool_fault and step[1] == "Conv3d_2c_3x3"
                x = _unit(state, step[1], x, dtype, step[2], fault, pre_relu=late_relu)
                if late_relu:
                    out[step[1]] = F.relu(x).permute(0, 2, 3, 4, 1).double().numpy()
                    continue
            elif step[0] == "pool":
                if pool_fault and x.min() < 0:
                    x = _pool(x, step[1], step[2], zero_padded=True)
                else:
                    x = _pool(x, step[1], step[2])
            else:
                block = step[1]
                b0 = _unit(state, f"{block}.b0", x, dtype, fault=fault)
                b1 = _unit(state, f"{block}.b1b", _unit(state, f"{block}.b1a", x, dtype, fault=fault), dtype, fault=fault)
                b2 = _unit(state, f"{block}.b2b", _unit(state, f"{block}.b2a", x, dtype, fault=fault), dtype, fault=fault)
                b3 = _unit(state, f"{block}.b3b", _pool(x, (3, 3, 3), (1, 1, 1)), dtype, fault=fault)
                x = torch.cat([b0, b2, b1, b3] if fault == "b1_b2_swapped" and block == "Mixed_3b" else [b0, b1, b2, b3], 1)
            if step[1] in V.TAPS:
                out[step[1]] = x.permute(0, 2, 3, 4, 1).double().numpy()
        hw = x.shape[3]
        x = F.avg_pool3d(x, (2, hw, x.shape[4]), stride=(1, 1, 1))
        x = F.conv3d(x, state[V.LOGITS + ".weight"].to(dtype), state[V.LOGITS + ".bias"].to(dtype))
        out["features"] = x.mean(dim=(2, 3, 4)).double().numpy()
    return out


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def deviation(values, ref):
    """the largest |values - ref| relative to the RMS of ref: feature maps have zeros, so no element-wise quotient"""
    return float(np.abs(np.asarray(values, dtype=np.float64) - ref).max() / rms(ref))


SAMPLE = 4096               # elements of a map the golden file keeps (a committed file stays small); the features are kept whole


def sample_index(name, key, size):
    """the seeded element sample of a case's map: indices into the flattened [N,T,H,W,C] array"""
    if size <= SAMPLE:
        return np.arange(size)
    rng = np.random.default_rng(7000 + 10 * list(CASES).index(name) + KEYS.index(key))
    return np.sort(rng.choice(size, SAMPLE, replace=False))


class Entry:
    """one golden record: the fp64 values at the sampled elements, the RMS and the positive fraction of the whole map, and the
    band, the fp32 CPU run's largest deviation over the WHOLE map relative to that RMS"""

    def __init__(self, z, name, key):
        p = f"{name}.{key}."
        self.ref, self.size, self.rms, self.band, self.positive = z[p + "ref"], int(z[p + "size"]), float(z[p + "rms"]), float(z[p + "band"]), float(z[p + "positive"])
        self.index = sample_index(name, key, self.size)

    def deviation(self, values):
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        assert v.size == self.size, (v.size, self.size)
        return float(np.abs(v[self.index] - self.ref).max() / self.rms)


def golden():
    """{case: {key: Entry}} from tests/golden/fvd_band.npz"""
    if "golden" not in _STATE:
        z = np.load(GOLDEN)
        _STATE["golden"] = {name: {k: Entry(z, name, k) for k in KEYS} for name in CASES}
    return _STATE["golden"]


def gate(name, key):
    """the largest deviation allowed for a tap (or the features) of a case: GATE_FACTOR times the recorded band"""
    return GATE_FACTOR * golden()[name][key].band
