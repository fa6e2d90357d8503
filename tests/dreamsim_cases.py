"""Cases, oracle, bounds and gate of the DreamSim tests (tests/test_dreamsim_cpu.py, tests/test_dreamsim_gpu.py,
tests/golden/make_dreamsim_band.py).  Derivations: tests/ERROR_BOUNDS_DREAMSIM.md.

The oracle is the tower model of tests/vit_cases.py.  The resize model is the float64 matrix product under
dreamsim.resize_matrix, itself checked against F.interpolate.  Faults can be planted; the CPU tests require the gate to see each.
"""
import math
import os

import numpy as np
import torch

from motion324_amd import dreamsim as D
from motion324_amd.vit import OPENAI_MEAN, OPENAI_STD, synth_clip_state_dict

import clipsim_cases as CC
import vit_cases as V
from error_bounds import EXP2, TINY32, U32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dreamsim_band.npz")
WEIGHT_SEED = 3240
TAPS = D.TAPS
KEYS = TAPS + ("features",)
RESIZE_SHAPES = ((512, 512, 224, 224), (37, 53, 224, 224), (96, 130, 32, 48), (225, 300, 224, 224), (64, 64, 64, 64), (5, 7, 3, 2))
TOWER_FAULTS = {"dino_cls": ("ln_eps_1e-5", "patch_bias_dropped", "ln_pre_applied", "openai_mean_std"), "clip_quick": ("erf_gelu",)}

# name: layout, width, heads, layers, mlp, patch, image, embed, images, act, ln_eps, mean, std, feature
CASES = {
    "dino_cls": dict(layout="dino", width=192, heads=3, layers=2, mlp=384, patch=16, image=64, embed=0, images=3, act="gelu",
                     ln_eps=1e-6, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD, feature="cls"),
    "dino_prenorm_l197": dict(layout="dino", width=128, heads=2, layers=1, mlp=256, patch=16, image=224, embed=0, images=2, act="gelu",
                              ln_eps=1e-6, mean=D.IMAGENET_MEAN, std=D.IMAGENET_STD, feature="cls_prenorm"),
    "clip_quick": dict(layout="open_clip", width=160, heads=2, layers=2, mlp=320, patch=32, image=96, embed=64, images=3,
                       act="quick_gelu", ln_eps=1e-5, mean=OPENAI_MEAN, std=OPENAI_STD, feature="embedding"),
}

_STATE = {}


def state_dict(name):
    if ("sd", name) not in _STATE:
        c = CASES[name]
        seed = WEIGHT_SEED + list(CASES).index(name)
        if c["layout"] == "dino":
            sd = D.synth_dino_state_dict(seed, c["width"], c["layers"], c["heads"], c["mlp"], c["patch"], c["image"], c["embed"])
        else:
            sd = synth_clip_state_dict(seed, c["width"], c["layers"], c["heads"], c["mlp"], c["patch"], c["image"], c["embed"])
        _STATE["sd", name] = sd
    return _STATE["sd", name]


def weights(name):
    if ("w", name) not in _STATE:
        _STATE["w", name] = D.load_vit_weights(state_dict(name), heads=CASES[name]["heads"])
    return _STATE["w", name]


def tower_kwargs(name):
    c = CASES[name]
    return dict(act=c["act"], ln_eps=c["ln_eps"], mean=c["mean"], std=c["std"], feature=c["feature"])


def images(name):
    """the input images of a case: fp32 planar [n,3,S,S] torch in [0, 1], bytes / 255, seeded by the case's position"""
    c = CASES[name]
    b = CC.make_frames(c["images"], c["image"], c["image"], 4000 + list(CASES).index(name))
    return torch.from_numpy(CC.bytes_to_float(b))


# ------------------------------------------------------------------------------------------- the resize model
def resize_model(frames, out_h, out_w, antialias=True, rounded=False):
    """float64 [T,3,out_h,out_w] numpy of uint8 [T,H,W,3] or fp32 [T,3,H,W] frames: Ry x Rx^T under dreamsim.resize_matrix;
    a byte sample is the fp32 quotient v / 255, as the kernel forms it"""
    x = np.asarray(frames)
    if x.dtype == np.uint8:
        x = CC.bytes_to_float(x)
    x = x.astype(np.float64)
    ry, rx = D.resize_matrix(x.shape[2], out_h, antialias, rounded), D.resize_matrix(x.shape[3], out_w, antialias, rounded)
    return ry @ x @ rx.T


def resample_pass(x, weights, first, axis):
    """(reference, bound, sum |w| per output) float64 of one m324_resample_f32 pass over fp32 planar samples x [F,3,H,W] (numpy)
    under the fp32 tables the kernel reads: the value in float64 and (ksize + 1) U32 sum |w| |x| for the fma chain
    (ERROR_BOUNDS_DREAMSIM.md); the row sums carry a first pass's error through a second one"""
    x = np.moveaxis(np.asarray(x, np.float64), 2 if axis == "y" else 3, -1)
    n_in = x.shape[-1]
    m = np.zeros((weights.shape[0], n_in))
    for i in range(weights.shape[0]):
        n = min(weights.shape[1], n_in - int(first[i]))
        m[i, first[i]:first[i] + n] = weights[i, :n].astype(np.float64)
    ref, mag = x @ m.T, np.abs(x) @ np.abs(m).T
    back = 2 if axis == "y" else 3
    return np.moveaxis(ref, -1, back), np.moveaxis((weights.shape[1] + 1) * U32 * mag + TINY32, -1, back), np.abs(m).sum(1)


# ------------------------------------------------------------------------------------------- the oracle
oracle, patch_rows_model = V.oracle, V.patch_rows_model


def case_oracle(name, dtype=torch.float64, fault=None, img=None):
    c = CASES[name]
    return oracle(images(name) if img is None else img, state_dict(name), c["heads"], act=c["act"], ln_eps=c["ln_eps"], mean=c["mean"],
                  std=c["std"], feature=c["feature"], dtype=dtype, fault=fault)


def synth_lora(state, rank, seed):
    """peft-style adapters on every attn.qkv of a DINO-layout state dict, both factors of visible size"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    i = 0
    while f"blocks.{i}.attn.qkv.weight" in state:
        n, k = state[f"blocks.{i}.attn.qkv.weight"].shape
        out[f"base_model.model.blocks.{i}.attn.qkv.lora_A.default.weight"] = torch.randn((rank, k), generator=g) / math.sqrt(k)
        out[f"base_model.model.blocks.{i}.attn.qkv.lora_B.default.weight"] = torch.randn((n, rank), generator=g) * 0.3
        i += 1
    return out


# ------------------------------------------------------------------------------------------- the distance
def normalize_embedding_model(e):
    e = np.asarray(e, np.float64)
    e = e / np.linalg.norm(e, axis=-1, keepdims=True)
    return e - e.mean(axis=-1, keepdims=True)


def distance_model(feats_a, feats_b, normalize=True):
    """fp64 [T]: 1 - cos of the concatenated (normalised) tower features; feats_*: one [T, E_i] array per tower"""
    u, v = (np.concatenate([normalize_embedding_model(f) if normalize else np.asarray(f, np.float64) for f in fs], -1) for fs in (feats_a, feats_b))
    return 1.0 - (u * v).sum(-1) / (np.linalg.norm(u, axis=-1) * np.linalg.norm(v, axis=-1))


def concat_delta(feats, devs):
    """[T]: how far the concatenated normalised vector can move when tower i's feature moves by at most devs[i] per element: e ->
    e / |e| has gain at most 1 / |e_i|, centring is a projection, so delta = sqrt(sum_i E_i dev_i^2 / |e_i|^2)"""
    total = 0.0
    for f, dev in zip(feats, devs):
        f = np.asarray(f, np.float64)
        total = total + f.shape[-1] * dev ** 2 / (np.linalg.norm(f, axis=-1) ** 2)
    return np.sqrt(total)


def distance_bound(feats_a, feats_b, devs):
    """|d (1 - cos)| [T] (ERROR_BOUNDS_DREAMSIM.md): 1.01 (delta_u / |u| + delta_v / |v|) for the concatenated u, v"""
    u, v = (np.concatenate([normalize_embedding_model(f) for f in fs], -1) for fs in (feats_a, feats_b))
    return 1.01 * (concat_delta(feats_a, devs) / np.linalg.norm(u, axis=-1) + concat_delta(feats_b, devs) / np.linalg.norm(v, axis=-1))


DISTANCE_SOURCES = ((100, 60), (225, 300))          # H x W of the distance test's clips, 3 frame pairs each


def distance_frames(H, W):
    return CC.make_frames(3, H, W, 5000 + H), CC.make_frames(3, H, W, 6000 + W)


def distance_features(frames, dtype=torch.float64, antialias=True):
    """the three small towers' fp64-oracle features of a clip: each tower sees the clip resized to its own image size"""
    feats = []
    for name, c in CASES.items():
        img = torch.from_numpy(resize_model(frames, c["image"], c["image"], antialias).astype(np.float32))
        feats.append(case_oracle(name, dtype, img=img)["features"])
    return feats


# ------------------------------------------------------------------------------------------- the band and the gate
rms, deviation, SAMPLE = V.rms, V.deviation, V.SAMPLE


def sample_index(name, key, size):
    return V.sample_index(19000, list(CASES).index(name), KEYS.index(key), size)


def golden():
    """{case: {key: Entry}} from tests/golden/dreamsim_band.npz"""
    return V.golden(GOLDEN, CASES, KEYS, 19000)


def gate(name, key):
    return V.gate(golden(), name, key)


# ------------------------------------------------------------------------------------------- kernel bounds
QUICK_GELU_LIPSCHITZ = 1.1      # max |d/dz z sigmoid(1.702 z)| = 1.0998, near 1.702 z = 2.4


def quick_gelu(z):
    return z * torch.sigmoid(1.702 * z)


def quick_gelu_bound(z, dz):
    """|error| of the QuickGELU epilogue at the fp64 pre-activation z known to dz (ERROR_BOUNDS_DREAMSIM.md): the pre-activation's
    error through the slope, plus the evaluation -- t = -1.702f z carries 2 U32 (the constant and the product), e = exp(t) that
    times |t| and EXP2 of its own, d = 1 + e the share e / d = 1 - sigma of both and one rounding, the quotient one more."""
    t = 1.702 * z.abs()
    one_minus_sigma = torch.sigmoid(-1.702 * z)
    rel = 1.01 * (one_minus_sigma * (2 * t * U32 + EXP2) + 2 * U32)
    return QUICK_GELU_LIPSCHITZ * dz + rel * quick_gelu(z).abs() + TINY32
