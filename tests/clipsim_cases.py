"""Cases, oracle, bounds and gate of the CLIP similarity tests (tests/test_clipsim_cpu.py, tests/test_clipsim_gpu.py,
tests/golden/make_clip_band.py).  Derivations: tests/ERROR_BOUNDS_CLIP.md.

The oracle is the tower model of tests/vit_cases.py on the preprocessed bytes / 255, as open_clip's VisionTransformer (GELU, eps
1e-5, the embedding), with the taps under ClipVision's names.  Six faults can be planted into it; the CPU tests require the gate
to see each.  The preprocessing model is PIL's own resize on the host.
"""
import math
import os

import numpy as np
import torch

from motion324_amd import clipsim as C

import vit_cases as V
from error_bounds import EXP2, U32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_band.npz")
WEIGHT_SEED = 324
FAULTS = ("quick_gelu", "scale_64", "kv_swapped", "pos_shifted_one_row", "ln_post_skipped", "ln_eps_1e-6")
TAPS = C.TAPS
KEYS = TAPS + ("features",)
SOURCE_SIZES = ((512, 512), (96, 130), (225, 300), (224, 224), (100, 60), (37, 53))      # H x W: shrinking and enlarging

# name: (width, heads, layers, mlp, patch, image, embed, images, source H, source W)
CASES = {
    "d104_l257": (208, 2, 2, 512, 14, 224, 64, 3, 96, 130),     # bigG's head and token count: five key tiles, the last ragged
    "d80_l50": (160, 2, 2, 320, 32, 224, 32, 2, 100, 60),       # ViT-H's head; under one key tile; C % 64 != 0
    "d88_l197": (176, 2, 1, 352, 16, 224, 48, 2, 225, 300),     # ViT-g's head
}

_STATE = {}


def state_dict(name):
    if ("sd", name) not in _STATE:
        width, heads, layers, mlp, patch, image, embed = CASES[name][:7]
        _STATE["sd", name] = C.synth_clip_state_dict(WEIGHT_SEED + list(CASES).index(name), width, layers, heads, mlp, patch, image, embed)
    return _STATE["sd", name]


def weights(name):
    if ("w", name) not in _STATE:
        _STATE["w", name] = C.load_clip_vision_weights(state_dict(name), heads=CASES[name][1])
    return _STATE["w", name]


def make_frames(T, H, W, seed):
    """uint8 [T,H,W,3] numpy: moving smooth content plus texture"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        base = np.stack([np.sin(6.0 * xx + c + 0.3 * t) * np.cos(4.0 * yy - 0.2 * t) for c in range(3)], axis=-1)
        out[t] = np.clip(np.rint(128 + 70 * base + rng.normal(0, 25, (H, W, 3))), 0, 255).astype(np.uint8)
    return out


def frames(name):
    """the source images uint8 [n,H,W,3] of a case, seeded by the case's position"""
    n, H, W = CASES[name][7:10]
    return make_frames(n, H, W, 3000 + list(CASES).index(name))


# ------------------------------------------------------------------------------------------- preprocessing on the host
def float_to_bytes(x):
    """fp32 [T,3,H,W] numpy in [0, 1] -> uint8 [T,H,W,3]: pic.mul(255).byte() of ToPILImage, the product in fp32"""
    v = np.clip(np.asarray(x, np.float32) * np.float32(255.0), np.float32(0.0), np.float32(255.0))
    return np.ascontiguousarray(np.trunc(v).astype(np.uint8).transpose(0, 2, 3, 1))


def bytes_to_float(b):
    """uint8 [T,H,W,3] -> fp32 [T,3,H,W] in [0, 1], ToTensor's division"""
    return np.ascontiguousarray((np.asarray(b).astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def preprocess_model(frames_u8_or_f32, size):
    """uint8 [T,size,size,3]: ToPILImage, torchvision's Resize(size, BICUBIC) and CenterCrop(size) with PIL itself"""
    from PIL import Image
    x = np.asarray(frames_u8_or_f32)
    if x.dtype != np.uint8:
        x = float_to_bytes(x)
    out = []
    for frame in x:
        h, w = frame.shape[:2]
        if w <= h:
            nw, nh = size, int(size * h / w)
        else:
            nh, nw = size, int(size * w / h)
        im = Image.fromarray(frame).resize((nw, nh), Image.BICUBIC)
        top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
        out.append(np.asarray(im.crop((left, top, left + size, top + size))))
    return np.stack(out)


def resample_pass(img, coef, bounds, axis):
    """numpy model of one m324_frame_resample pass over uint8 [H,W,C]: acc = 2^21 + sum value * coef, >> 22, clamp"""
    img = np.moveaxis(np.asarray(img).astype(np.int64), axis, 0)
    out = np.empty((coef.shape[0],) + img.shape[1:], np.int64)
    for i in range(coef.shape[0]):
        x0, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = np.tensordot(coef[i, :n].astype(np.int64), img[x0:x0 + n], axes=(0, 0)) + (1 << 21)
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def patch_rows_model(img_u8, patch, Kp, mean=C.OPENAI_MEAN, std=C.OPENAI_STD):
    """fp32 [n * g * g, Kp]: the host formula of m324_vit_patches, (v / 255 - mean) / std with each operation in fp32"""
    return V.patch_rows_model(torch.from_numpy(bytes_to_float(img_u8)), patch, Kp, mean, std)


# ------------------------------------------------------------------------------------------- the oracle
def oracle(img_u8, state, heads, dtype=torch.float64, fault=None):
    """{tap: numpy float64, "features": [n, E]} of preprocessed bytes uint8 [n,S,S,3]; taps as ClipVision.features(taps=True)"""
    assert fault is None or fault in FAULTS, fault
    out = V.oracle(torch.from_numpy(bytes_to_float(img_u8)), state, heads, dtype=dtype, fault=fault)
    return {**{mine: out[shared] for mine, shared in zip(TAPS, V.TAPS)}, "features": out["features"]}


def case_oracle(name, dtype=torch.float64, fault=None):
    return oracle(preprocess_model(frames(name), CASES[name][5]), state_dict(name), CASES[name][1], dtype, fault)


def cosine_model(fa, fb):
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    return (fa * fb).sum(-1) / (np.linalg.norm(fa, axis=-1) * np.linalg.norm(fb, axis=-1))


# ------------------------------------------------------------------------------------------- the band and the gate
rms, deviation, SAMPLE = V.rms, V.deviation, V.SAMPLE


def sample_index(name, key, size):
    return V.sample_index(9000, list(CASES).index(name), KEYS.index(key), size)


def golden():
    """{case: {key: Entry}} from tests/golden/clip_band.npz"""
    return V.golden(GOLDEN, CASES, KEYS, 9000)


def gate(name, key):
    return V.gate(golden(), name, key)


def cosine_bound(fa, fb, dev_abs):
    """|d cos| for feature vectors each moved by at most dev_abs per element (ERROR_BOUNDS_CLIP.md): the gradient of the cosine
    with respect to a has norm sqrt(1 - cos^2) / |a| <= 1 / |a|, and an E-vector of element errors dev_abs has norm at most
    sqrt(E) dev_abs; second-order terms are covered by the factor 1.01.  Returns [T]."""
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    d = math.sqrt(fa.shape[-1]) * dev_abs
    return 1.01 * d * (1.0 / np.linalg.norm(fa, axis=-1) + 1.0 / np.linalg.norm(fb, axis=-1))


# ------------------------------------------------------------------------------------------- kernel bounds
def attention_tok(qkv, B, L, H, D, scale):
    """(reference, bound) fp64 [B * L, H * D] of m324_attention_tok on the fp32 rows qkv [B * L, >= 3 H D]: error_bounds.
    _attention_terms with D + 2 in place of 66 (D products, the scale and the shift), p kept in fp32, one fp32 output rounding:
    (4 max_k ds + 2 L U32 + EXP2) (p |v|) + 2 U32 |o|,  ds = 2 (D + 2) U32 (|q| . |k|) scale."""
    x = qkv.detach().double().cpu()[:B * L, :3 * H * D]
    q, k, v = (x[:, j * H * D:(j + 1) * H * D].reshape(B, L, H, D).permute(0, 2, 1, 3) for j in range(3))
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    ds = 2 * (D + 2) * U32 * torch.einsum("bhqd,bhkd->bhqk", q.abs(), k.abs()) * scale
    dsmax = ds.max(-1, keepdim=True).values
    p = torch.softmax(s, dim=-1)
    rel = 4 * dsmax + 2 * L * U32 + EXP2
    o = torch.einsum("bhqk,bhkd->bhqd", p, v)
    mag = torch.einsum("bhqk,bhkd->bhqd", p, v.abs())
    bound = rel * mag + 2 * U32 * o.abs()
    return o.permute(0, 2, 1, 3).reshape(B * L, H * D), bound.permute(0, 2, 1, 3).reshape(B * L, H * D)
