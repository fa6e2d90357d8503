"""DreamSim without a device: the resize tables against torch, the loader and the LoRA merge, the oracle against its planted
faults, the distance bound, what the new wrappers hand to the library, and the refusals (tests/dreamsim_cases.py,
tests/ERROR_BOUNDS_DREAMSIM.md)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dreamsim_cases as DC

from motion324_amd import dreamsim as D
from motion324_amd import lib, ops
from motion324_amd.lib import M324Error

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ops_calls as MOC      # noqa: E402


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("H, W, oh, ow", DC.RESIZE_SHAPES)
def test_tables_equal_torch_interpolate_in_float64(H, W, oh, ow, antialias):
    x = torch.rand((2, 3, H, W), dtype=torch.float64, generator=torch.Generator().manual_seed(H * W))
    want = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=antialias).numpy()
    got = DC.resize_model(x.numpy(), oh, ow, antialias)
    err = float(np.abs(got - want).max())
    print(H, W, oh, ow, antialias, err)
    assert err <= 1e-12


@pytest.mark.parametrize("n_in, n_out, antialias", [(512, 224, True), (96, 32, True), (37, 224, True), (300, 224, False), (7, 2, True), (5, 3, False)])
def test_table_rows_sum_to_one_and_stay_inside_the_axis(n_in, n_out, antialias):
    w, first = D.resize_tables(n_in, n_out, antialias)
    assert w.dtype == np.float32 and first.dtype == np.int32 and w.shape[0] == first.shape[0] == n_out
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= (w.shape[1] + 1) * 2.0 ** -24
    assert (w >= 0).all() and (first >= 0).all() and (first < n_in).all()
    last = np.array([np.flatnonzero(r).max() for r in w])
    assert (first + last < n_in).all()                              # every non-zero weight reads inside the axis
    w64, _ = D.resize_tables64(n_in, n_out, antialias)
    assert np.array_equal(w, w64.astype(np.float32))


def test_table_sizes_and_the_identity():
    assert D.resize_tables(512, 224)[0].shape[1] == 5 and D.resize_tables(96, 32)[0].shape[1] == 6
    for aa in (True, False):
        w, first = D.resize_tables(64, 64, aa)
        assert np.array_equal(first, np.arange(64)) and (w[:, 0] == 1.0).all() and (w[:, 1:] == 0.0).all()
    with pytest.raises(M324Error, match="positive"):
        D.resize_tables(0, 4)


def test_pass_order_counts_the_work():
    assert D.pass_order(512, 512, 224, 224, 5, 5) == ("y", "x")            # a tie goes to y first
    assert D.pass_order(100, 1000, 50, 50, 5, 41) == ("x", "y")
    assert D.pass_order(1000, 100, 50, 50, 41, 5) == ("y", "x")


# ------------------------------------------------------------------------------------------------ loader
def test_loader_accepts_both_layouts():
    for name, c in DC.CASES.items():
        w = DC.weights(name)
        assert isinstance(w, D.VitWeights)
        assert (w.width, w.heads, w.layers, w.mlp, w.patch, w.image, w.embed) == (c["width"], c["heads"], c["layers"], c["mlp"], c["patch"],
                                                                                 c["image"], c["embed"])
        assert w.tokens == (c["image"] // c["patch"]) ** 2 + 1 and w.patch_w.shape == (c["width"], 3 * c["patch"] ** 2)
        assert (w.patch_b is not None) == (c["layout"] == "dino") and (w.ln_pre is None) == (c["layout"] == "dino")
        assert (w.proj_t is None) == (c["embed"] == 0)
    sd = DC.state_dict("dino_cls")
    prefixed = {"module.extractor.model." + k: v for k, v in sd.items()}
    a, b = D.load_vit_weights(sd, heads=3), D.load_vit_weights(prefixed, heads=3)
    assert torch.equal(a.blocks[1].in_proj[0], b.blocks[1].in_proj[0]) and torch.equal(a.pos, b.pos)
    assert torch.equal(a.blocks[0].in_proj[0], sd["blocks.0.attn.qkv.weight"]) and a.cls.shape == (192,) and a.pos.shape == (17, 192)
    with_pre = D.synth_dino_state_dict(1, 64, 1, 2, 128, 16, 32, embed=16, norm_pre=True)
    w = D.load_vit_weights(with_pre, heads=2)
    assert w.ln_pre is not None and w.embed == 16 and w.proj_t.shape == (16, 64)
    assert D.load_vit_weights(D.synth_dino_state_dict(1, 192, 1, 3, 64, 16, 32)).heads == 3        # the named tower by width


def test_loader_refuses_by_key():
    sd = DC.state_dict("dino_cls")

    def without(key):
        return {k: v for k, v in sd.items() if k != key}

    with pytest.raises(M324Error, match="no key 'norm.weight'"):
        D.load_vit_weights(without("norm.weight"), heads=3)
    with pytest.raises(M324Error, match="no key 'blocks.1.attn.qkv.bias'"):
        D.load_vit_weights(without("blocks.1.attn.qkv.bias"), heads=3)
    with pytest.raises(M324Error, match="'pos_embed'.*non-square"):
        D.load_vit_weights(dict(sd, pos_embed=torch.zeros(1, 16, 192)), heads=3)
    with pytest.raises(M324Error, match="'blocks.0.attn.qkv.weight'.*D % 8"):
        D.load_vit_weights(sd, heads=16)                                                           # D = 12
    with pytest.raises(M324Error, match="'blocks.0.mlp.fc2.weight' has shape"):
        D.load_vit_weights(dict(sd, **{"blocks.0.mlp.fc2.weight": torch.zeros(192, 380)}), heads=3)
    bad = dict(sd)
    bad["blocks.1.norm2.bias"] = sd["blocks.1.norm2.bias"].clone()
    bad["blocks.1.norm2.bias"][5] = float("nan")
    with pytest.raises(M324Error, match="'blocks.1.norm2.bias' holds values that are not finite"):
        D.load_vit_weights(bad, heads=3)
    with pytest.raises(M324Error, match="no multiple of 4"):
        D.load_vit_weights(D.synth_dino_state_dict(1, 66, 1, 1, 128, 16, 32), heads=1)
    with pytest.raises(M324Error, match="pass heads="):
        D.load_vit_weights(D.synth_dino_state_dict(1, 64, 1, 2, 128, 16, 32))
    with pytest.raises(M324Error, match="neither"):
        D.load_vit_weights({"weight": torch.zeros(3)})
    with pytest.raises(M324Error, match="layer scale"):
        D.load_vit_weights(dict(sd, **{"blocks.0.ls1.gamma": torch.ones(192)}), heads=3)


# ------------------------------------------------------------------------------------------------ LoRA
def test_merged_lora_equals_the_unmerged_adapters():
    name, alpha = "dino_cls", 0.5
    sd = DC.state_dict(name)
    adapter = DC.synth_lora(sd, 4, 77)
    merged = D.merge_lora({k: v.double() for k, v in sd.items()}, adapter, alpha)
    assert merged["blocks.0.norm1.weight"] is not None and not torch.equal(merged["blocks.0.attn.qkv.weight"], sd["blocks.0.attn.qkv.weight"].double())
    c = DC.CASES[name]
    kw = dict(act=c["act"], ln_eps=c["ln_eps"], mean=c["mean"], std=c["std"], feature=c["feature"])
    a = DC.oracle(DC.images(name), merged, c["heads"], **kw)
    b = DC.oracle(DC.images(name), sd, c["heads"], lora=(adapter, alpha), **kw)
    plain = DC.case_oracle(name)
    for k in DC.KEYS:
        assert np.abs(a[k] - b[k]).max() <= 1e-12, k
    assert DC.deviation(a["features"], plain["features"]) > 1e-2           # the adapters are not a no-op
    w = D.load_vit_weights(D.merge_lora(sd, adapter, alpha), heads=3)
    assert w.blocks[0].in_proj[0].dtype == torch.float32


def test_merge_lora_refuses_by_key():
    sd = DC.state_dict("dino_cls")
    adapter = DC.synth_lora(sd, 4, 78)
    stray = dict(adapter)
    stray["base_model.model.blocks.7.attn.qkv.lora_A.default.weight"] = torch.zeros(4, 192)
    stray["base_model.model.blocks.7.attn.qkv.lora_B.default.weight"] = torch.zeros(576, 4)
    with pytest.raises(M324Error, match=r"blocks\.7\.attn\.qkv\.lora_A\.default\.weight.*no base weight"):
        D.merge_lora(sd, stray, 1.0)
    lonely = {k: v for k, v in adapter.items() if "blocks.1.attn.qkv.lora_B" not in k}
    with pytest.raises(M324Error, match="no lora_B partner"):
        D.merge_lora(sd, lonely, 1.0)
    wrong = dict(adapter)
    wrong["base_model.model.blocks.0.attn.qkv.lora_B.default.weight"] = torch.zeros(192, 4)
    with pytest.raises(M324Error, match="do not fit the base weight"):
        D.merge_lora(sd, wrong, 1.0)


# ------------------------------------------------------------------------------------------------ the oracle and its faults
@pytest.fixture(scope="module")
def refs():
    return {name: DC.case_oracle(name) for name in DC.CASES}


@pytest.mark.parametrize("name", list(DC.CASES))
def test_fp64_oracle_reproduces_the_file_and_fp32_stays_inside_the_gate(name, refs):
    table = DC.golden()[name]
    f32 = DC.case_oracle(name, torch.float32)
    for k in DC.KEYS:
        assert table[k].deviation(refs[name][k]) <= 1e-12, k
        assert abs(table[k].rms - DC.rms(refs[name][k])) <= 1e-12 * table[k].rms
        assert 1e-8 < table[k].band < 5e-5, (k, table[k].band)           # an fp32 band: neither empty nor loose
        assert table[k].deviation(f32[k]) <= DC.gate(name, k), k


@pytest.mark.parametrize("name, fault", [(n, f) for n, fs in DC.TOWER_FAULTS.items() for f in fs])
def test_planted_faults_leave_the_gate(name, fault, refs):
    out = DC.case_oracle(name, fault=fault)
    devs = {k: DC.golden()[name][k].deviation(out[k]) for k in DC.KEYS}
    print(name, fault, {k: f"{v:.2e} / {DC.gate(name, k):.2e}" for k, v in devs.items()})
    for k in ("block0", "last_block", "cls_row", "features"):
        assert devs[k] > DC.gate(name, k), (fault, k)


@pytest.fixture(scope="module")
def clips():
    out = {}
    for H, W in DC.DISTANCE_SOURCES:
        a, b = DC.distance_frames(H, W)
        out[H, W] = (a, b, DC.distance_features(a), DC.distance_features(b))
    return out


def feature_devs():
    return [DC.gate(n, "features") * DC.golden()[n]["features"].rms for n in DC.CASES]


def test_antialias_off_leaves_the_gate_when_shrinking(clips):
    a, _, fa, _ = clips[225, 300]
    off = DC.distance_features(a, antialias=False)
    for name, x, y in zip(DC.CASES, off, fa):
        assert DC.deviation(x, y) > DC.gate(name, "features"), name


def test_skipped_normalisation_leaves_the_distance_bound(clips):
    for a, b, fa, fb in clips.values():
        d, raw = DC.distance_model(fa, fb), DC.distance_model(fa, fb, normalize=False)
        assert (np.abs(d - raw) > DC.distance_bound(fa, fb, feature_devs())).all()


def test_distance_bound_holds_for_random_and_steepest_perturbations(clips):
    devs = feature_devs()
    rng = np.random.default_rng(5)
    for a, b, fa, fb in clips.values():
        d = DC.distance_model(fa, fb)
        bound = DC.distance_bound(fa, fb, devs)
        assert (bound > 0).all() and (bound < 1e-3).all()
        worst = 0.0
        for trial in range(20):
            pa = [f + dev * rng.choice([-1.0, 1.0], f.shape) for f, dev in zip(fa, devs)]
            pb = [f + dev * rng.choice([-1.0, 1.0], f.shape) for f, dev in zip(fb, devs)]
            worst = max(worst, float((np.abs(DC.distance_model(pa, pb) - d) / bound).max()))
        # steepest: every element of every tower's feature moves by dev against the distance's gradient
        ta, tb = ([torch.tensor(f, dtype=torch.float64, requires_grad=True) for f in fs] for fs in (fa, fb))
        u, v = (torch.cat([D.normalize_embedding(t) for t in ts], -1) for ts in (ta, tb))
        D.distance(u, v).sum().backward()
        pa = [f + dev * np.sign(t.grad.numpy()) for f, dev, t in zip(fa, devs, ta)]
        pb = [f + dev * np.sign(t.grad.numpy()) for f, dev, t in zip(fb, devs, tb)]
        steep = float((np.abs(DC.distance_model(pa, pb) - d) / bound).max())
        print("random", worst, "steepest", steep)
        assert worst <= 1.0 and steep <= 1.0 and steep > worst


def test_normalize_embedding_and_distance_equal_their_models():
    rng = np.random.default_rng(1)
    e, f = rng.normal(size=(4, 48)), rng.normal(size=(4, 48))
    assert np.abs(D.normalize_embedding(torch.from_numpy(e)).numpy() - DC.normalize_embedding_model(e)).max() <= 1e-15
    assert np.abs(D.distance(torch.from_numpy(e), torch.from_numpy(f)).numpy() - DC.distance_model([e], [f], normalize=False)).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ what the wrappers hand over
def record(cases):
    saved = MOC.CASES
    MOC.CASES = cases
    try:
        return MOC.record(ops, lib)
    finally:
        MOC.CASES = saved


def test_wrappers_marshal_their_calls():
    U8, I32 = torch.uint8, torch.int32

    def resample_u8_x(t, rec):
        return ops.resample_f32(t("src", 2, 5, 7, 3, dtype=U8, dev=True), t("w", 4, 3, dev=True), t("first", 4, dtype=I32, dev=True), "x")

    def resample_f32_y_out(t, rec):
        return ops.resample_f32(t("src", 2, 3, 5, 8, dev=True), t("w", 6, 2, dev=True), t("first", 6, dtype=I32, dev=True), "y",
                                out=t("out", 2, 3, 6, 8, dev=True))

    def patches(t, rec):
        return ops.vit_patches_f32(t("img", 2, 3, 32, 32, dev=True), 16, t("ms", 6, dev=True), 800)

    def quick(t, rec):
        return ops.gemm(t("a", 8, 32), t("w", 12, 32), t("out", 8, 12), bias=t("bias", 12), act=lib.ACT_QUICK_GELU)

    def bad_axis(t, rec):
        return ops.resample_f32(t("src", 2, 3, 5, 8, dev=True), t("w", 6, 2, dev=True), t("first", 6, dtype=I32, dev=True), "z")

    def bad_tables(t, rec):
        return ops.resample_f32(t("src", 2, 3, 5, 8, dev=True), t("w", 6, 2, dev=True), t("first", 5, dtype=I32, dev=True), "y")

    got = record([("u8 x", resample_u8_x), ("f32 y out", resample_f32_y_out), ("patches", patches), ("quick", quick), ("bad axis", bad_axis),
                  ("bad tables", bad_tables)])
    c = got["u8 x"]
    assert c["calls"] == [["m324_resample_f32", [["s0", 0], 1, 2, 5, 7, 0, ["s1", 0], ["s2", 0], 3, 4, ["s3", 0], None]]]
    assert c["ret"] == ["float32", [2, 3, 5, 4], [60, 20, 4, 1], "s3", 0]
    c = got["f32 y out"]
    assert c["calls"] == [["m324_resample_f32", [["s0", 0], 0, 2, 5, 8, 1, ["s1", 0], ["s2", 0], 2, 6, ["s3", 0], None]]]
    assert c["wrote"] == ["out"] and c["ret"][1] == [2, 3, 6, 8] and c["ret"][3] == "s3"
    c = got["patches"]
    assert c["calls"] == [["m324_vit_patches_f32", [["s0", 0], 2, 32, 16, ["s1", 0], ["s2", 0], 800, None]]]
    assert c["ret"] == ["float32", [8, 800], [800, 1], "s2", 0]
    c = got["quick"]
    assert [name for name, _ in c["calls"]] == ["m324_gemm_plan", "m324_gemm"]
    args = c["calls"][1][1][0]
    assert args == {"A": ["s0", 0], "lda": 32, "W": ["s1", 0], "ldw": 32, "C": ["s2", 0], "ldc": 12, "M": 8, "N": 12, "K": 32,
                    "bias": ["s3", 0], "act": 2} and c["wrote"] == ["out"]
    assert "axis must be" in got["bad axis"]["error"] and got["bad axis"]["calls"] == []
    assert "int32 [n_out]" in got["bad tables"]["error"] and got["bad tables"]["calls"] == []


# ------------------------------------------------------------------------------------------------ refusals
def test_cpu_tensors_and_bad_arguments_are_refused():
    img = torch.zeros((1, 3, 64, 64))
    with pytest.raises(M324Error, match="HIP device"):
        ops.resample_f32(img, torch.zeros(4, 2), torch.zeros(4, dtype=torch.int32), "x")
    with pytest.raises(M324Error, match="HIP device"):
        ops.vit_patches_f32(img, 16, torch.zeros(6), 768)
    with pytest.raises(M324Error, match="HIP device"):
        D.resize(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4)
    with pytest.raises(M324Error, match="HIP device"):
        D.VitTower(DC.weights("dino_cls"), "cpu", feature="cls")
    with pytest.raises(M324Error, match="act must be"):
        D.VitTower(DC.weights("dino_cls"), "cuda", act="relu")
    with pytest.raises(M324Error, match="feature must be"):
        D.VitTower(DC.weights("dino_cls"), "cuda", feature="mean")
    with pytest.raises(M324Error, match="needs a 'proj'"):
        D.VitTower(DC.weights("dino_cls"), "cuda", feature="embedding")
    with pytest.raises(M324Error, match="non-empty"):
        D.DreamSim([])
    with pytest.raises(M324Error, match="equal shapes"):
        D.evaluate_clips_dreamsim(torch.zeros((16, 8, 8, 3), dtype=torch.uint8), torch.zeros((16, 8, 9, 3), dtype=torch.uint8), None)
    with pytest.raises(M324Error, match="at least 16"):
        D.evaluate_clips_dreamsim(torch.zeros((8, 8, 8, 3), dtype=torch.uint8), torch.zeros((8, 8, 8, 3), dtype=torch.uint8), None)


def test_evaluate_clips_dreamsim_applies_the_subvideo_rule_to_any_callable():
    values = torch.linspace(0.1, 0.9, 20, dtype=torch.float64)
    gt = torch.zeros((20, 8, 8, 3), dtype=torch.uint8)
    score = D.evaluate_clips_dreamsim(gt, gt.clone(), lambda a, b: values)
    want = D.clip_statistics(values.numpy())
    assert score.value == want.value and score.value_std == want.value_std and score.per_video.shape == (1,)
    kept = np.concatenate([values.numpy(), values.numpy()[-12:][::-1]])
    assert abs(score.value - kept.mean()) <= 1e-15


def test_command_line_refuses_unequal_path_counts():
    with pytest.raises(M324Error, match="pairs are matched by position"):
        D.main(["--gt_paths", "a", "b", "--result_paths", "c", "--dino", "x", "--clip", "y", "--open_clip", "z"])
