"""Cases, oracle, bounds and gate of the DreamSim tests (tests/test_dreamsim_cpu.py, tests/test_dreamsim_gpu.py,
tests/golden/make_dreamsim_band.py).  Derivations: tests/ERROR_BOUNDS_DREAMSIM.md.

The oracle is a torch CPU model of a ViT image tower at a chosen precision, written from the definitions of timm's and
open_clip's VisionTransformer: F.conv2d with stride = patch (with the bias the DINO layout has), the class token and positions,
an optional LayerNorm in front of the blocks, explicit q / k / v slices of the fused projection, softmax(q k^T D^-0.5) v per head,
F.gelu or x sigmoid(1.702 x), and one of three class features.  The resize model is the float64 matrix product under
dreamsim.resize_matrix, itself checked against F.interpolate.  Faults can be planted; the CPU tests require the gate to see each.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from motion324_amd import dreamsim as D
from motion324_amd.clipsim import OPENAI_MEAN, OPENAI_STD, synth_clip_state_dict

import clipsim_cases as CC
from error_bounds import EXP2, TINY32, U32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dreamsim_band.npz")
WEIGHT_SEED = 3240
GATE_FACTOR = 8.0           # times the recorded deviation of the fp32 CPU run; the reason is in tests/ERROR_BOUNDS_FVD.md
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
def normalised(img, dtype, mean, std):
    """[n,3,S,S] by the formula of the patch kernel: (x - mean) / std, both operations in fp32 (every precision of the oracle
    starts from the input the kernel sees)"""
    m = torch.tensor(mean, dtype=torch.float32).reshape(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).reshape(1, 3, 1, 1)
    return ((img.to(torch.float32) - m) / s).to(dtype).contiguous()


def patch_rows_model(img, patch, Kp, mean, std):
    """fp32 [n * g * g, Kp]: the host formula of m324_vit_patches_f32"""
    x = normalised(img, torch.float32, mean, std)
    n, _, S, _ = x.shape
    g = S // patch
    rows = x.reshape(n, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * patch * patch)
    out = torch.zeros((n * g * g, Kp), dtype=torch.float32)
    out[:, :3 * patch * patch] = rows
    return out


_OPEN_CLIP_NAMES = {"patch_w": "conv1.weight", "patch_b": None, "cls": "class_embedding", "pos": "positional_embedding", "ln_pre": "ln_pre",
                    "block": "transformer.resblocks.{}.", "ln_1": "ln_1", "qkv_w": "attn.in_proj_weight", "qkv_b": "attn.in_proj_bias",
                    "proj": "attn.out_proj", "ln_2": "ln_2", "fc1": "mlp.c_fc", "fc2": "mlp.c_proj", "norm": "ln_post"}
_DINO_NAMES = {"patch_w": "patch_embed.proj.weight", "patch_b": "patch_embed.proj.bias", "cls": "cls_token", "pos": "pos_embed",
               "ln_pre": "norm_pre", "block": "blocks.{}.", "ln_1": "norm1", "qkv_w": "attn.qkv.weight", "qkv_b": "attn.qkv.bias",
               "proj": "attn.proj", "ln_2": "norm2", "fc1": "mlp.fc1", "fc2": "mlp.fc2", "norm": "norm"}


def oracle(img, state, heads, *, act="gelu", ln_eps=1e-5, mean=OPENAI_MEAN, std=OPENAI_STD, feature="embedding", dtype=torch.float64,
           fault=None, lora=None):
    """{tap: numpy float64, "features": [n, E]} of fp32 planar images [n,3,S,S]; taps as VitTower.features(taps=True).
    lora = (adapter state dict, alpha): the adapters of attn.qkv applied UNMERGED, x W^T + (alpha / r) (x A^T) B^T."""
    assert fault in (None, "erf_gelu", "ln_eps_1e-5", "patch_bias_dropped", "ln_pre_applied", "openai_mean_std"), fault
    names = _DINO_NAMES if "patch_embed.proj.weight" in state else _OPEN_CLIP_NAMES
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in state.items()}
    eps = 1e-5 if fault == "ln_eps_1e-5" else ln_eps
    if fault == "openai_mean_std":
        mean, std = OPENAI_MEAN, OPENAI_STD
    if fault == "erf_gelu":
        act = "gelu"

    def ln(x, name):
        return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)

    out = {}
    with torch.no_grad():
        x = normalised(img, dtype, mean, std)
        conv = sd[names["patch_w"]]
        W, patch = conv.shape[0], conv.shape[2]
        bias = sd[names["patch_b"]] if names["patch_b"] and fault != "patch_bias_dropped" else None
        x = F.conv2d(x, conv, bias, stride=patch)
        n = x.shape[0]
        x = x.reshape(n, W, -1).permute(0, 2, 1)
        x = torch.cat([sd[names["cls"]].reshape(1, 1, W).expand(n, 1, W), x], 1) + sd[names["pos"]].reshape(1, -1, W)
        L = x.shape[1]
        if names["ln_pre"] + ".weight" in sd:
            x = ln(x, names["ln_pre"])
        elif fault == "ln_pre_applied":
            x = F.layer_norm(x, (W,), None, None, eps)
        out["embed"] = x.double().numpy()
        Dh = W // heads
        i = 0
        while names["block"].format(i) + names["ln_1"] + ".weight" in sd:
            b = names["block"].format(i)
            y = ln(x, b + names["ln_1"])
            qkv = y @ sd[b + names["qkv_w"]].t() + sd[b + names["qkv_b"]]
            if lora is not None:
                adapter, alpha = lora
                A, B = (torch.as_tensor(adapter[f"base_model.model.{b}attn.qkv.lora_{s}.default.weight"]).to(dtype) for s in "AB")
                qkv = qkv + (alpha / A.shape[0]) * ((y @ A.t()) @ B.t())
            q, k, v = (qkv[..., j * W:(j + 1) * W].reshape(n, L, heads, Dh).permute(0, 2, 1, 3) for j in range(3))
            a = torch.softmax(q @ k.transpose(2, 3) * Dh ** -0.5, dim=-1) @ v
            a = a.permute(0, 2, 1, 3).reshape(n, L, W)
            x = x + a @ sd[b + names["proj"] + ".weight"].t() + sd[b + names["proj"] + ".bias"]
            y = ln(x, b + names["ln_2"])
            h = y @ sd[b + names["fc1"] + ".weight"].t() + sd[b + names["fc1"] + ".bias"]
            h = h * torch.sigmoid(1.702 * h) if act == "quick_gelu" else F.gelu(h)
            x = x + h @ sd[b + names["fc2"] + ".weight"].t() + sd[b + names["fc2"] + ".bias"]
            if i == 0:
                out["block0"] = x.double().numpy()
            i += 1
        out["last_block"] = x.double().numpy()
        row = x[:, 0]
        if feature != "cls_prenorm":
            row = ln(row, names["norm"])
        out["cls_row"] = row.double().numpy()
        out["features"] = (row @ sd["proj"]).double().numpy() if feature == "embedding" else out["cls_row"]
    return out


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
rms, deviation, SAMPLE = CC.rms, CC.deviation, CC.SAMPLE


def sample_index(name, key, size):
    if size <= SAMPLE:
        return np.arange(size)
    rng = np.random.default_rng(19000 + 10 * list(CASES).index(name) + KEYS.index(key))
    return np.sort(rng.choice(size, SAMPLE, replace=False))


class Entry(CC.Entry):
    def __init__(self, z, name, key):
        p = f"{name}.{key}."
        self.ref, self.size, self.rms, self.band = z[p + "ref"], int(z[p + "size"]), float(z[p + "rms"]), float(z[p + "band"])
        self.index = sample_index(name, key, self.size)


def golden():
    """{case: {key: Entry}} from tests/golden/dreamsim_band.npz"""
    if "golden" not in _STATE:
        z = np.load(GOLDEN)
        _STATE["golden"] = {name: {k: Entry(z, name, k) for k in KEYS} for name in CASES}
    return _STATE["golden"]


def gate(name, key):
    """the largest deviation allowed for a tap (or the features) of a case: GATE_FACTOR times the recorded band"""
    return GATE_FACTOR * golden()[name][key].band


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
