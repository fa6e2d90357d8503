"""CLIP similarity without a device: the bicubic tables and the preprocessing rules against PIL, the loader and its refusals,
the committed band, the power of the gate against six planted faults, the sub-video statistics and the wrappers' refusals."""
import os
import re

import numpy as np
import pytest
import torch

import clipsim_cases as CC

from conftest import REPO
from motion324_amd import clipsim as C
from motion324_amd import framing, lib, ops
from motion324_amd.lib import M324Error

NAMES = ("m324_attention_tok", "m324_layernorm_wide", "m324_vit_patches", "m324_vit_tokens")


def test_entry_points_are_declared_bound_and_built():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "m324.h")).read(), flags=re.S)
    for name in NAMES:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert proto, name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
        assert len(proto.group(1).split(",")) == len(lib.SIGNATURES[name]), name
    from motion324_amd import build
    assert "vit.hip" in build.SOURCES


def test_c_abi_refuses_before_any_device_call():
    """argument validation comes before the first HIP call, so it is observable without a GPU"""
    import ctypes
    h = lib.load()
    f = ctypes.c_float
    assert h.m324_attention_tok(16, 36, 16, 12, 1, 4, 1, 12, f(0.3), None) == -3 and "D=12" in lib.last_error()
    assert h.m324_attention_tok(16, 408, 16, 136, 1, 4, 1, 136, f(0.1), None) == -3 and "D=136" in lib.last_error()
    assert h.m324_attention_tok(16, 184, 16, 64, 1, 4, 1, 64, f(0.1), None) == -1 and "ld=184" in lib.last_error()
    assert h.m324_attention_tok(16, 194, 16, 64, 1, 4, 1, 64, f(0.1), None) == -1 and "ld=194" in lib.last_error()
    assert h.m324_attention_tok(16, 192, 16, 64, 1, 0, 1, 64, f(0.1), None) == -1 and "L=0" in lib.last_error()
    assert h.m324_attention_tok(20, 192, 16, 64, 1, 4, 1, 64, f(0.1), None) == -1 and "aligned" in lib.last_error()
    assert h.m324_attention_tok(None, 192, 16, 64, 1, 4, 1, 64, f(0.1), None) == -1 and "null" in lib.last_error()
    assert h.m324_layernorm_wide(16, 4100, 16, 16, f(1e-5), 16, 4100, 1, 4100, None) == -3 and "C=4100" in lib.last_error()
    assert h.m324_layernorm_wide(16, 8, 16, 16, f(1e-5), 16, 16, 1, 16, None) == -1 and "ldx=8" in lib.last_error()
    assert h.m324_layernorm_wide(16, 16, None, 16, f(1e-5), 16, 16, 1, 16, None) == -1 and "null" in lib.last_error()
    assert h.m324_vit_patches(16, 1, 224, 14, 16, 16, 600, None) == -3 and "Kp=600" in lib.last_error()
    assert h.m324_vit_patches(16, 1, 224, 15, 16, 16, 704, None) == -1 and "patch=15" in lib.last_error()
    assert h.m324_vit_patches(None, 1, 224, 14, 16, 16, 608, None) == -1 and "null" in lib.last_error()
    assert h.m324_vit_tokens(16, 16, 16, 16, 1, 5, 6, None) == -3 and "C=6" in lib.last_error()
    assert h.m324_vit_tokens(16, 16, None, 16, 1, 5, 8, None) == -1 and "null" in lib.last_error()


def test_ops_wrappers_refuse_cpu_tensors():
    z = torch.zeros
    with pytest.raises(M324Error, match="attention_tok: qkv: libm324 ops need HIP device"):
        ops.attention_tok(z(4, 192), 1, 4, 1, 64)
    with pytest.raises(M324Error, match="layernorm_wide: x: libm324 ops need HIP device"):
        ops.layernorm_wide(z(4, 16), z(16), z(16), 1e-5)
    with pytest.raises(M324Error, match="vit_patches: libm324 ops need HIP device"):
        ops.vit_patches(z((1, 28, 28, 3), dtype=torch.uint8), 14, z(6), 608)
    with pytest.raises(M324Error, match="vit_tokens: patch_rows: libm324 ops need HIP device"):
        ops.vit_tokens(z(4, 16), z(16), z(5, 16))
    with pytest.raises(M324Error, match="HIP device"):
        C.preprocess(z((1, 8, 8, 3), dtype=torch.uint8), 224)
    with pytest.raises(M324Error, match="HIP device"):
        C.ClipVision(CC.weights("d80_l50"), "cpu")


# ------------------------------------------------------------------------------------------------ tables and preprocessing
def test_default_tables_are_the_lanczos_tables():
    for n_in, n_out in ((512, 224), (37, 224), (300, 298)):
        a, b = framing.resample_tables(n_in, n_out), framing.resample_tables(n_in, n_out, filter="lanczos")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[0].shape[1] == 2 * int(np.ceil(3.0 * max(n_in / n_out, 1.0))) + 1
    with pytest.raises(M324Error, match="filter must be one of"):
        framing.resample_tables(8, 8, filter="box")


def two_passes(img, new_w, new_h, x_keep=None, y_keep=None):
    """the numpy model of the two device passes with the bicubic tables, optionally cut to the kept outputs"""
    h, w = img.shape[:2]
    tx, ty = framing.resample_tables(w, new_w, filter="bicubic"), framing.resample_tables(h, new_h, filter="bicubic")
    if x_keep is not None:
        tx, ty = tuple(t[x_keep] for t in tx), tuple(t[y_keep] for t in ty)
    assert framing.pass_order(w, h, new_h) == "xy"
    return CC.resample_pass(CC.resample_pass(img, *tx, axis=1), *ty, axis=0)


@pytest.mark.parametrize("H, W", CC.SOURCE_SIZES)
def test_bicubic_tables_reproduce_pil_bit_for_bit(H, W):
    from PIL import Image
    img = CC.make_frames(1, H, W, 10 * H + W)[0]
    for new_w, new_h in ((224, 224), (int(224 * W / H), 224) if W > H else (224, int(224 * H / W)), (W, H), (61, 47)):
        want = np.asarray(Image.fromarray(img).resize((new_w, new_h), Image.BICUBIC))
        assert np.array_equal(two_passes(img, new_w, new_h), want), (H, W, new_w, new_h)


@pytest.mark.parametrize("H, W", CC.SOURCE_SIZES)
def test_preprocess_rules_against_pil_in_both_forms(H, W):
    """the float -> byte rule, the resize geometry and the crop from the tables, as clipsim.preprocess applies them"""
    frames = CC.make_frames(2, H, W, 7 * H + W)
    want = CC.preprocess_model(frames, 224)
    new_h, new_w, top, left = C.resize_geometry(H, W, 224)
    assert min(new_h, new_w) == 224 and max(new_h, new_w) == int(224 * max(H, W) / min(H, W))
    assert top == int(round((new_h - 224) / 2.0)) and left == int(round((new_w - 224) / 2.0))
    keep_x, keep_y = slice(left, left + 224), slice(top, top + 224)
    got = np.stack([two_passes(f, new_w, new_h, keep_x, keep_y) for f in frames])
    assert np.array_equal(got, want)
    as_float = CC.bytes_to_float(frames)
    assert np.array_equal(CC.float_to_bytes(as_float), frames)                      # every byte survives b / 255 * 255, truncated
    assert np.array_equal(C.to_bytes(torch.from_numpy(as_float)).numpy(), frames)
    free = np.random.default_rng(H).uniform(-0.2, 1.2, (2, 3, 9, 11)).astype(np.float32)
    assert np.array_equal(C.to_bytes(torch.from_numpy(free)).numpy(), CC.float_to_bytes(free))


def test_all_bytes_survive_the_float_round_trip():
    b = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    assert np.array_equal(CC.float_to_bytes(CC.bytes_to_float(b)), b)


def test_resize_geometry_rounds_the_crop_half_to_even():
    assert C.resize_geometry(96, 130, 224) == (224, 303, 0, 40)                    # (303 - 224) / 2 = 39.5 -> 40
    assert C.resize_geometry(100, 60, 224) == (373, 224, 74, 0)                     # 74.5 -> 74
    assert C.resize_geometry(224, 224, 224) == (224, 224, 0, 0)


# ------------------------------------------------------------------------------------------------ the loader
def small_state():
    return C.synth_clip_state_dict(1, 64, 1, 2, 128, 14, 28, 16)


def test_loader_reads_sizes_prefixes_and_layouts(tmp_path):
    sd = small_state()
    w = C.load_clip_vision_weights(sd, heads=2)
    assert w[:8] == (64, 2, 1, 128, 14, 28, 5, 16)
    Kp = (3 * 14 * 14 + 31) // 32 * 32
    assert w.patch_w.shape == (64, Kp) and bool((w.patch_w[:, 588:] == 0).all())
    assert torch.equal(w.patch_w[:, :588], sd["conv1.weight"].reshape(64, 588))
    assert torch.equal(w.proj_t, sd["proj"].t()) and w.proj_t.is_contiguous() and w.proj_t.shape == (16, 64)
    assert torch.equal(w.blocks[0].in_proj[0], sd["transformer.resblocks.0.attn.in_proj_weight"]) and w.pos.dtype == torch.float32
    for prefix in ("visual.", "module.", "module.visual."):
        full = {prefix + k: v for k, v in sd.items()}
        if "visual." in prefix:             # a whole CLIP checkpoint: the text tower shares key names with the image tower
            full.update({prefix.replace("visual.", "") + k: torch.zeros(3) for k in ("positional_embedding", "transformer.resblocks.0.ln_1.weight", "logit_scale")})
        w2 = C.load_clip_vision_weights(full, heads=2)
        assert all(torch.equal(a, b) for a, b in zip((w.patch_w, w.cls, w.pos, w.proj_t), (w2.patch_w, w2.cls, w2.pos, w2.proj_t)))
    path = tmp_path / "tower.pt"
    torch.save({"state_dict": sd}, path)
    assert torch.equal(C.load_clip_vision_weights(str(path), heads=2).pos, w.pos)
    # a K that is no multiple of 32 is padded with zero columns
    w208 = CC.weights("d104_l257")
    assert w208.blocks[0].in_proj[0].shape == (624, 224) and bool((w208.blocks[0].in_proj[0][:, 208:] == 0).all()) and w208.proj_t.shape == (64, 224)


def test_loader_head_table_and_heads_argument():
    assert C.HEADS_BY_WIDTH == {768: 12, 1024: 16, 1280: 16, 1408: 16, 1664: 16}
    sd = C.synth_clip_state_dict(2, 768, 1, 12, 64, 32, 64, 8)
    assert C.load_clip_vision_weights(sd).heads == 12 and C.load_clip_vision_weights(sd, heads=8).heads == 8
    with pytest.raises(M324Error, match="head count is not part of a state dict and width 64"):
        C.load_clip_vision_weights(small_state())


def test_loader_refuses_by_key_or_shape(tmp_path):
    sd = small_state()

    def refused(match, change=None, heads=2, **extra):
        s = dict(sd)
        s.update(extra)
        if change:
            change(s)
        with pytest.raises(M324Error, match=match):
            C.load_clip_vision_weights(s, heads=heads)

    refused("ls_1", **{"transformer.resblocks.0.ls_1.gamma": torch.ones(64)})
    refused("attn_pool", **{"attn_pool.query": torch.ones(4, 64)})
    refused("non-square grid", **{"positional_embedding": torch.zeros(7, 64)})
    refused(r"W % heads != 0", heads=3)
    refused(r"D % 8 != 0", heads=16)                                                # D = 4
    refused("no key 'proj'", change=lambda s: s.pop("proj"))
    refused(r"in_proj_weight' has shape \(192, 32\)", **{"transformer.resblocks.0.attn.in_proj_weight": torch.zeros(192, 32)})
    refused("not finite", **{"ln_pre.weight": torch.full((64,), float("nan"))})
    refused("'conv1.bias'", **{"conv1.bias": torch.zeros(64)})
    wide = C.synth_clip_state_dict(3, 4104, 1, 36, 8, 32, 32, 8)
    with pytest.raises(M324Error, match=r"W > 4096"):
        C.load_clip_vision_weights(wide, heads=36)
    big_head = C.synth_clip_state_dict(3, 272, 1, 2, 8, 32, 32, 8)
    with pytest.raises(M324Error, match=r"D > 128"):
        C.load_clip_vision_weights(big_head, heads=2)
    with pytest.raises(M324Error, match="no such file"):
        C.load_clip_vision_weights(str(tmp_path / "absent.pt"))
    st = tmp_path / "tower.safetensors"
    st.write_bytes(b"\0" * 16)
    try:
        import safetensors  # noqa: F401
    except ImportError:
        with pytest.raises(M324Error, match="safetensors package is not installed"):
            C.load_clip_vision_weights(str(st))


def test_quick_gelu_is_refused():
    with pytest.raises(M324Error, match="quick_gelu"):
        C.ClipVision(CC.weights("d80_l50"), "cuda", act="quick_gelu")


# ------------------------------------------------------------------------------------------------ band and power
def test_band_file_matches_the_cases_and_the_document():
    table = CC.golden()
    text = open(os.path.join(REPO, "tests", "ERROR_BOUNDS_CLIP.md")).read()
    rows = re.search(r"<!-- band:begin -->\n(.*?)<!-- band:end -->", text, flags=re.S).group(1)
    for name, (width, heads, layers, mlp, patch, image, embed, n, H, W) in CC.CASES.items():
        row = next(r for r in rows.splitlines() if r.startswith(f"| {name} |"))
        L = (image // patch) ** 2 + 1
        for key in CC.KEYS:
            e = table[name][key]
            assert f"{e.band:.2e}" in row, (name, key)
            assert 1e-8 < e.band < 1e-4 and 0.3 < e.rms < 5, (name, key, e.band, e.rms)
            assert e.ref.shape == (min(e.size, CC.SAMPLE),) and e.ref.dtype == np.float64
        assert table[name]["ln_pre"].size == table[name]["last_block"].size == n * L * width
        assert table[name]["ln_post"].size == n * width and table[name]["features"].size == n * embed
    assert CC.CASES["d104_l257"][0] // CC.CASES["d104_l257"][1] == 104 and (224 // 14) ** 2 + 1 == 257


def test_fp64_oracle_reproduces_the_golden_values():
    out = CC.case_oracle("d80_l50")
    for key in CC.KEYS:
        assert CC.golden()["d80_l50"][key].deviation(out[key]) <= 1e-12, key


@pytest.fixture(scope="module")
def d104_images():
    return CC.preprocess_model(CC.frames("d104_l257"), 224)


def test_fp32_oracle_stays_inside_the_gate(d104_images):
    name = "d104_l257"
    out = CC.oracle(d104_images, CC.state_dict(name), 2, torch.float32)
    for key in CC.KEYS:
        assert CC.golden()[name][key].deviation(out[key]) <= CC.gate(name, key), key


@pytest.mark.parametrize("fault", CC.FAULTS)
def test_gate_sees_the_planted_fault_in_the_features(fault, d104_images):
    name = "d104_l257"
    out = CC.oracle(d104_images, CC.state_dict(name), 2, torch.float64, fault)
    d = CC.golden()[name]["features"].deviation(out["features"])
    assert d > CC.gate(name, "features"), f"the gate does not see {fault}: {d:.3g}"


def test_cosine_bound_covers_perturbed_features():
    """cosine_bound against features moved by dev_abs per element in random and in the worst directions"""
    rng = np.random.default_rng(3)
    fa, fb = rng.normal(size=(64, 32)), rng.normal(size=(64, 32))
    dev = 1e-5
    base = CC.cosine_model(fa, fb)
    bound = CC.cosine_bound(fa, fb, dev)
    for _ in range(20):
        da, db = (dev * np.sign(rng.normal(size=fa.shape)) for _ in range(2))
        assert (np.abs(CC.cosine_model(fa + da, fb + db) - base) <= bound).all()
    na, nb = fa / np.linalg.norm(fa, axis=-1, keepdims=True), fb / np.linalg.norm(fb, axis=-1, keepdims=True)
    ga = np.sign(nb - base[:, None] * na)                                           # steepest ascent under the max norm
    gb = np.sign(na - base[:, None] * nb)
    worst = np.abs(CC.cosine_model(fa + dev * ga, fb + dev * gb) - base)
    assert (worst <= bound).all() and (worst > 0.05 * bound).any()


# ------------------------------------------------------------------------------------------------ evaluation
def test_evaluate_clips_clip_statistics_with_a_stub_metric():
    T = 40
    values = torch.linspace(0.5, 0.9, T, dtype=torch.float64)
    calls = []

    def metric(a, b, **kw):
        calls.append(kw)
        return values

    gt = torch.zeros((T, 37, 53, 3), dtype=torch.uint8)                              # no multiple-of-16 rule here
    score = C.evaluate_clips_clip(gt, gt.clone(), metric, max_scratch_bytes=123)
    assert calls == [{"max_scratch_bytes": 123}]
    kept = values.numpy()[:32]                                                       # 40 frames: one 32-frame sub-video, the rest dropped
    assert score.value == float(kept.mean()) and score.value_std == float(kept.std()) and score.per_video.shape == (1,)
    assert np.array_equal(score.per_frame, values.numpy())
    short = C.evaluate_clips_clip(gt[:20], gt[:20], lambda a, b: values[:20])
    idx = list(range(20)) + list(range(20))[-12:][::-1]
    assert short.value == float(values.numpy()[idx].mean())
    with pytest.raises(M324Error, match="equal shapes"):
        C.evaluate_clips_clip(gt, gt[:, :36], metric)
    with pytest.raises(M324Error, match="at least 16 frames"):
        C.evaluate_clips_clip(gt[:8], gt[:8], metric)
    with pytest.raises(M324Error, match="sides of 1 to 16384"):
        C.evaluate_clips_clip(torch.zeros((16, 0, 4, 3), dtype=torch.uint8), torch.zeros((16, 0, 4, 3), dtype=torch.uint8), metric)
    with pytest.raises(M324Error, match=r"uint8 \[T,H,W,3\] or fp32 \[T,3,H,W\]"):
        C.evaluate_clips_clip(gt.to(torch.int32), gt.to(torch.int32), metric)


def test_main_refuses_unequal_path_lists():
    with pytest.raises(M324Error, match="pairs are matched by position"):
        C.main(["--gt_paths", "a", "b", "--result_paths", "c", "--weights", "w.pt"])
