"""The oracle, the band records and the gate shared by the CLIP similarity and DreamSim tests (tests/clipsim_cases.py,
tests/dreamsim_cases.py): both metrics run motion324_amd.vit's tower.

The oracle is a torch CPU model of a ViT image tower at a chosen precision, written from the definitions of timm's and
open_clip's VisionTransformer: F.conv2d with stride = patch (with the bias the DINO layout has), the class token and positions,
an optional LayerNorm in front of the blocks, explicit q / k / v slices of the fused projection, softmax(q k^T D^-0.5) v per head,
F.gelu or x sigmoid(1.702 x), and one of three class features.  Eleven faults can be planted into it; the CPU tests require the
gates to see each.
"""
import numpy as np
import torch
import torch.nn.functional as F

from motion324_amd.vit import OPENAI_MEAN, OPENAI_STD

GATE_FACTOR = 8.0           # times the recorded deviation of the fp32 CPU run; the reason is in tests/ERROR_BOUNDS_FVD.md
SAMPLE = 4096               # elements of a tap the golden file keeps (a committed file stays small); the features are kept whole
TAPS = ("embed", "block0", "last_block", "cls_row")
FAULTS = ("quick_gelu", "scale_64", "kv_swapped", "pos_shifted_one_row", "ln_post_skipped", "ln_eps_1e-6",
          "erf_gelu", "ln_eps_1e-5", "patch_bias_dropped", "ln_pre_applied", "openai_mean_std")


def normalised(img, dtype, mean, std):
    """[n,3,S,S] of fp32 planar images in [0, 1] by the formula of the patch kernels: (x - mean) / std, both operations in fp32
    (every precision of the oracle starts from the input the kernel sees; a byte is x = v / 255 in fp32)"""
    m = torch.tensor(mean, dtype=torch.float32).reshape(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).reshape(1, 3, 1, 1)
    return ((img.to(torch.float32) - m) / s).to(dtype).contiguous()


def patch_rows_model(img, patch, Kp, mean, std):
    """fp32 [n * g * g, Kp]: the host formula of m324_vit_patches_f32 (and, on v / 255, of m324_vit_patches)"""
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
    assert fault is None or fault in FAULTS, fault
    names = _DINO_NAMES if "patch_embed.proj.weight" in state else _OPEN_CLIP_NAMES
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in state.items()}
    eps = {"ln_eps_1e-5": 1e-5, "ln_eps_1e-6": 1e-6}.get(fault, ln_eps)
    if fault == "openai_mean_std":
        mean, std = OPENAI_MEAN, OPENAI_STD
    act = {"erf_gelu": "gelu", "quick_gelu": "quick_gelu"}.get(fault, act)

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
        pos = sd[names["pos"]].reshape(-1, W)
        x = torch.cat([sd[names["cls"]].reshape(1, 1, W).expand(n, 1, W), x], 1) + (torch.roll(pos, 1, 0) if fault == "pos_shifted_one_row" else pos)
        L = x.shape[1]
        if names["ln_pre"] + ".weight" in sd:
            x = ln(x, names["ln_pre"])
        elif fault == "ln_pre_applied":
            x = F.layer_norm(x, (W,), None, None, eps)
        out["embed"] = x.double().numpy()
        Dh = W // heads
        scale = 64 ** -0.5 if fault == "scale_64" else Dh ** -0.5
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
            if fault == "kv_swapped":
                k, v = v, k
            a = torch.softmax(q @ k.transpose(2, 3) * scale, dim=-1) @ v
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
        if feature != "cls_prenorm" and fault != "ln_post_skipped":
            row = ln(row, names["norm"])
        out["cls_row"] = row.double().numpy()
        out["features"] = (row @ sd["proj"]).double().numpy() if feature == "embedding" else out["cls_row"]
    return out


# ------------------------------------------------------------------------------------------- the band and the gate
def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def deviation(values, ref):
    """the largest |values - ref| relative to the RMS of ref"""
    return float(np.abs(np.asarray(values, dtype=np.float64) - ref).max() / rms(ref))


def sample_index(seed_base, case, key, size):
    """the elements of tap number `key` of case number `case` that a golden file keeps"""
    if size <= SAMPLE:
        return np.arange(size)
    rng = np.random.default_rng(seed_base + 10 * case + key)
    return np.sort(rng.choice(size, SAMPLE, replace=False))


class Entry:
    """one golden record: the fp64 values at the sampled elements, the RMS of the whole tap, and the band, the fp32 CPU run's
    largest deviation over the WHOLE tap relative to that RMS"""

    def __init__(self, z, name, key, index_of):
        p = f"{name}.{key}."
        self.ref, self.size, self.rms, self.band = z[p + "ref"], int(z[p + "size"]), float(z[p + "rms"]), float(z[p + "band"])
        self.index = index_of(self.size)

    def deviation(self, values):
        v = np.asarray(values, dtype=np.float64).reshape(-1)
        assert v.size == self.size, (v.size, self.size)
        return float(np.abs(v[self.index] - self.ref).max() / self.rms)


_GOLDEN = {}


def golden(path, cases, keys, seed_base):
    """{case: {key: Entry}} from a golden file, read once"""
    if path not in _GOLDEN:
        z = np.load(path)
        _GOLDEN[path] = {name: {k: Entry(z, name, k, lambda size, i=i, j=j: sample_index(seed_base, i, j, size)) for j, k in enumerate(keys)}
                         for i, name in enumerate(cases)}
    return _GOLDEN[path]


def gate(table, name, key):
    """the largest deviation allowed for a tap (or the features) of a case: GATE_FACTOR times the recorded band"""
    return GATE_FACTOR * table[name][key].band
