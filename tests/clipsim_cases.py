"""Cases, oracle, bounds and gate of the CLIP similarity tests (tests/test_clipsim_cpu.py, tests/test_clipsim_gpu.py,
tests/golden/make_clip_band.py).  Derivations: tests/ERROR_BOUNDS_CLIP.md.

The oracle is a torch CPU model of open_clip's VisionTransformer at a chosen precision, written from its definition: F.conv2d
with stride = patch, F.layer_norm with eps 1e-5, explicit q / k / v slices of the in-projection, softmax(q k^T D^-0.5) v per
head, F.gelu, the class token through ln_post and `pooled @ proj`.  Six faults can be planted into it; the CPU tests require the
gate to see each.  The preprocessing model is PIL's own resize on the host.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from motion324_amd import clipsim as C

from error_bounds import EXP2, U32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_band.npz")
WEIGHT_SEED = 324
GATE_FACTOR = 8.0           # times the recorded deviation of the fp32 CPU run; the reason is in tests/ERROR_BOUNDS_FVD.md
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


def normalised(img_u8, dtype, mean=C.OPENAI_MEAN, std=C.OPENAI_STD):
    """[n,3,S,S] of preprocessed bytes by the formula of the patch kernel: (v / 255 - mean) / std, each operation in fp32 (so
    that every precision of the oracle starts from the input the kernel sees)"""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).permute(0, 3, 1, 2).to(torch.float32)
    m = torch.tensor(mean, dtype=torch.float32).reshape(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).reshape(1, 3, 1, 1)
    return ((x / 255.0 - m) / s).to(dtype).contiguous()


def patch_rows_model(img_u8, patch, Kp, mean=C.OPENAI_MEAN, std=C.OPENAI_STD):
    """fp32 [n * g * g, Kp]: the host formula of m324_vit_patches"""
    x = normalised(img_u8, torch.float32, mean, std)
    n, _, S, _ = x.shape
    g = S // patch
    rows = x.reshape(n, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * patch * patch)
    out = torch.zeros((n * g * g, Kp), dtype=torch.float32)
    out[:, :3 * patch * patch] = rows
    return out


# ------------------------------------------------------------------------------------------- the oracle
def oracle(img_u8, state, heads, dtype=torch.float64, fault=None):
    """{tap: numpy float64, "features": [n, E]} of preprocessed bytes uint8 [n,S,S,3]; taps as ClipVision.features(taps=True)"""
    assert fault is None or fault in FAULTS, fault
    sd = {k: v.to(dtype) for k, v in state.items()}
    eps = 1e-6 if fault == "ln_eps_1e-6" else 1e-5
    out = {}
    with torch.no_grad():
        x = normalised(img_u8, dtype)
        W, patch = sd["conv1.weight"].shape[0], sd["conv1.weight"].shape[2]
        x = F.conv2d(x, sd["conv1.weight"], stride=patch)                       # [n, W, g, g]
        n = x.shape[0]
        x = x.reshape(n, W, -1).permute(0, 2, 1)
        x = torch.cat([sd["class_embedding"].reshape(1, 1, W).expand(n, 1, W), x], 1)
        pos = sd["positional_embedding"]
        x = x + (torch.roll(pos, 1, 0) if fault == "pos_shifted_one_row" else pos)
        L = x.shape[1]
        x = F.layer_norm(x, (W,), sd["ln_pre.weight"], sd["ln_pre.bias"], eps)
        out["ln_pre"] = x.double().numpy()
        D = W // heads
        scale = 64 ** -0.5 if fault == "scale_64" else D ** -0.5
        i = 0
        while f"transformer.resblocks.{i}.ln_1.weight" in sd:
            b = f"transformer.resblocks.{i}."
            y = F.layer_norm(x, (W,), sd[b + "ln_1.weight"], sd[b + "ln_1.bias"], eps)
            qkv = y @ sd[b + "attn.in_proj_weight"].t() + sd[b + "attn.in_proj_bias"]
            q, k, v = (qkv[..., j * W:(j + 1) * W].reshape(n, L, heads, D).permute(0, 2, 1, 3) for j in range(3))
            if fault == "kv_swapped":
                k, v = v, k
            a = torch.softmax(q @ k.transpose(2, 3) * scale, dim=-1) @ v
            a = a.permute(0, 2, 1, 3).reshape(n, L, W)
            x = x + a @ sd[b + "attn.out_proj.weight"].t() + sd[b + "attn.out_proj.bias"]
            y = F.layer_norm(x, (W,), sd[b + "ln_2.weight"], sd[b + "ln_2.bias"], eps)
            h = y @ sd[b + "mlp.c_fc.weight"].t() + sd[b + "mlp.c_fc.bias"]
            h = h * torch.sigmoid(1.702 * h) if fault == "quick_gelu" else F.gelu(h)
            x = x + h @ sd[b + "mlp.c_proj.weight"].t() + sd[b + "mlp.c_proj.bias"]
            if i == 0:
                out["block0"] = x.double().numpy()
            i += 1
        out["last_block"] = x.double().numpy()
        pooled = x[:, 0]
        if fault != "ln_post_skipped":
            pooled = F.layer_norm(pooled, (W,), sd["ln_post.weight"], sd["ln_post.bias"], eps)
        out["ln_post"] = pooled.double().numpy()
        out["features"] = (pooled @ sd["proj"]).double().numpy()
    return out


def case_oracle(name, dtype=torch.float64, fault=None):
    return oracle(preprocess_model(frames(name), CASES[name][5]), state_dict(name), CASES[name][1], dtype, fault)


def cosine_model(fa, fb):
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    return (fa * fb).sum(-1) / (np.linalg.norm(fa, axis=-1) * np.linalg.norm(fb, axis=-1))


# ------------------------------------------------------------------------------------------- the band and the gate
def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def deviation(values, ref):
    """the largest |values - ref| relative to the RMS of ref"""
    return float(np.abs(np.asarray(values, dtype=np.float64) - ref).max() / rms(ref))


SAMPLE = 4096               # elements of a tap the golden file keeps (a committed file stays small); the features are kept whole


def sample_index(name, key, size):
    if size <= SAMPLE:
        return np.arange(size)
    rng = np.random.default_rng(9000 + 10 * list(CASES).index(name) + KEYS.index(key))
    return np.sort(rng.choice(size, SAMPLE, replace=False))


class Entry:
    """one golden record: the fp64 values at the sampled elements, the RMS of the whole tap, and the band, the fp32 CPU run's
    largest deviation over the WHOLE tap relative to that RMS"""

    def __init__(self, z, name, key):
        p = f"{name}.{key}."
        self.ref, self.size, self.rms, self.band = z[p + "ref"], int(z[p + "size"]), float(z[p + "rms"]), float(z[p + "band"])
        self.index = sample_index(name, key, self.size)

    def deviation(self, values):
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        assert v.size == self.size, (v.size, self.size)
        return float(np.abs(v[self.index] - self.ref).max() / self.rms)


def golden():
    """{case: {key: Entry}} from tests/golden/clip_band.npz"""
    if "golden" not in _STATE:
        z = np.load(GOLDEN)
        _STATE["golden"] = {name: {k: Entry(z, name, k) for k in KEYS} for name in CASES}
    return _STATE["golden"]


def gate(name, key):
    """the largest deviation allowed for a tap (or the features) of a case: GATE_FACTOR times the recorded band"""
    return GATE_FACTOR * golden()[name][key].band


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
