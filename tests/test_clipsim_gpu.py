"""CLIP similarity on the device: the four kernels of csrc/vit.hip element by element, the preprocessing bit for bit, and the
tower end to end inside the recorded band (tests/clipsim_cases.py, tests/ERROR_BOUNDS_CLIP.md)."""
import ctypes

import numpy as np
import pytest
import torch

import clipsim_cases as CC
import error_bounds as EB

from motion324_amd import clipsim as C
from motion324_amd import lib, ops
from motion324_amd.lib import M324Error

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7777.0


def guarded(rows, cols, guard_rows=3, guard_cols=4):
    """(whole buffer, the [rows, cols] view inside it): guard rows in front and behind, guard columns to the right"""
    whole = torch.full((rows + 2 * guard_rows, cols + guard_cols), SENTINEL, dtype=torch.float32, device=DEV)
    return whole, whole[guard_rows:guard_rows + rows, :cols]


def guards_untouched(whole, rows, cols, guard_rows=3):
    w = whole.cpu()
    return bool((w[:guard_rows] == SENTINEL).all() and (w[guard_rows + rows:] == SENTINEL).all() and (w[:, cols:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ attention_tok
def qkv_rows(B, L, H, D, seed, ld=None, spread=1.0):
    g = torch.Generator().manual_seed(seed)
    ld = 3 * H * D if ld is None else ld
    x = torch.randn((B * L, ld), generator=g) * spread
    return x


def run_attention(x, B, L, H, D, ldo=None, scale=None):
    ldo = H * D if ldo is None else ldo
    whole, view = guarded(B * L, ldo, guard_cols=0)
    out = view[:, :H * D] if ldo == H * D else view
    got = ops.attention_tok(x.to(DEV), B, L, H, D, scale, out=out)
    assert got.data_ptr() == out.data_ptr()
    return whole, view


@pytest.mark.parametrize("D", [8, 64, 80, 88, 104, 128])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 257, 577])
def test_attention_tok_against_fp64(D, L):
    B, H = 2, 3
    x = qkv_rows(B, L, H, D, 100 * D + L)
    whole, view = run_attention(x, B, L, H, D)
    ref, bound = CC.attention_tok(x, B, L, H, D, D ** -0.5)
    EB.assert_within(view, ref, bound, f"attention_tok D={D} L={L}")
    assert guards_untouched(whole, B * L, H * D)


def test_attention_tok_padded_leading_dimensions_and_guards():
    B, L, H, D = 2, 65, 3, 104
    ld, ldo = 3 * H * D + 8, H * D + 4
    x = qkv_rows(B, L, H, D, 7, ld=ld)
    whole, view = run_attention(x, B, L, H, D, ldo=ldo)
    ref, bound = CC.attention_tok(x, B, L, H, D, D ** -0.5)
    EB.assert_within(view[:, :H * D], ref, bound, "attention_tok padded ld")
    w = whole.cpu()
    assert (w[:3] == SENTINEL).all() and (w[3 + B * L:] == SENTINEL).all() and (w[3:3 + B * L, H * D:] == SENTINEL).all()


def test_attention_tok_row_maximum_rises_in_the_last_key_tile():
    """scores of magnitude ~60 whose maximum sits among the last keys: every earlier tile's sums are rescaled"""
    B, L, H, D = 1, 257, 2, 104
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn((L, H, D), generator=g) for _ in range(3))
    q /= q.norm(dim=-1, keepdim=True)
    k /= k.norm(dim=-1, keepdim=True)
    direction = torch.randn((H, D), generator=g)
    direction /= direction.norm(dim=-1, keepdim=True)
    amp = torch.linspace(5.0, 60.0, L).reshape(L, 1, 1)             # the score q . k * scale grows with the key index
    q = direction.expand(L, H, D) * (D ** 0.25) * 8.0 + 0.05 * q
    k = direction.expand(L, H, D) * amp * (D ** 0.25) / 8.0 + 0.05 * k
    x = torch.cat([t.reshape(L, H * D) for t in (q, k, v)], 1).contiguous()
    ref, bound = CC.attention_tok(x, B, L, H, D, D ** -0.5)
    s = (q.double().permute(1, 0, 2) @ k.double().permute(1, 2, 0)) * D ** -0.5
    assert 50 < float(s.abs().max()) < 70 and bool((s.argmax(-1) >= 256).all())        # the last tile holds key 256 alone
    whole, view = run_attention(x, B, L, H, D)
    EB.assert_within(view, ref, bound, "attention_tok rising maximum")


def test_attention_tok_96_items():
    B, L, H, D = 6, 257, 16, 104                # B H = 96 items of three query tiles: 288 workgroups on 256 CUs
    x = qkv_rows(B, L, H, D, 17)
    whole, view = run_attention(x, B, L, H, D)
    ref, bound = CC.attention_tok(x, B, L, H, D, D ** -0.5)
    EB.assert_within(view, ref, bound, "attention_tok 96 items")
    assert guards_untouched(whole, B * L, H * D)


def test_attention_tok_agrees_with_m324_attention_at_64():
    from conftest import vt_layout
    B, L, H, D = 2, 197, 3, 64
    x = qkv_rows(B, L, H, D, 19)
    q, k, v = (x[:, j * H * D:(j + 1) * H * D].reshape(B, L, H, D).permute(0, 2, 1, 3).contiguous() for j in range(3))
    whole, view = run_attention(x, B, L, H, D)
    other = torch.empty((B * L, H * D), dtype=torch.float32, device=DEV)
    ops.attention(q.to(DEV), k.to(DEV), vt_layout(v).to(DEV), other, scale=D ** -0.5)
    ref, bound = CC.attention_tok(x, B, L, H, D, D ** -0.5)
    bound64 = EB.attention(q, k, v, D ** -0.5, p_bf16=False, out_dtype=torch.float32)
    EB.assert_within(view, ref, bound, "attention_tok D=64")
    EB.assert_within(view, other, bound + bound64, "attention_tok against m324_attention")


# ------------------------------------------------------------------------------------------------ layernorm_wide
@pytest.mark.parametrize("C_", [4, 1024, 1028, 1664, 4096])
@pytest.mark.parametrize("rows", [1, 5, 771])
def test_layernorm_wide_against_fp64(C_, rows):
    g = torch.Generator().manual_seed(C_ + rows)
    x = torch.randn((rows, C_), generator=g) * 1.5 + 0.3
    w, b = 1.0 + 0.2 * torch.randn((C_,), generator=g), 0.1 * torch.randn((C_,), generator=g)
    whole, view = guarded(rows, C_)
    ops.layernorm_wide(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, out=view)
    xd = x.double()
    ref = torch.nn.functional.layer_norm(xd, (C_,), w.double(), b.double(), 1e-5)
    EB.assert_within(view, ref, EB.layernorm(x, w, b, 1e-5, out_dtype=torch.float32), f"layernorm_wide C={C_} rows={rows}")
    assert guards_untouched(whole, rows, C_)


def test_layernorm_wide_strided_rows_and_no_bias():
    rows, C_ = 5, 1664
    g = torch.Generator().manual_seed(5)
    x3 = torch.randn((rows, 3 * C_), generator=g)
    w = 1.0 + 0.2 * torch.randn((C_,), generator=g)
    whole, view = guarded(rows, C_)
    ops.layernorm_wide(x3.to(DEV)[:, :C_], w.to(DEV), None, 1e-5, out=view)           # ldx = 3 C
    x = x3[:, :C_]
    ref = torch.nn.functional.layer_norm(x.double(), (C_,), w.double(), None, 1e-5)
    EB.assert_within(view, ref, EB.layernorm(x, w, None, 1e-5, out_dtype=torch.float32), "layernorm_wide strided")
    assert guards_untouched(whole, rows, C_)


# ------------------------------------------------------------------------------------------------ patches and tokens
@pytest.mark.parametrize("patch", [14, 16, 32])
@pytest.mark.parametrize("F_", [1, 3])
def test_vit_patches_equal_the_host_formula(patch, F_):
    S = 224
    img = CC.make_frames(F_, S, S, 50 + patch)
    Kp = (3 * patch * patch + 31) // 32 * 32 + (32 if patch == 16 else 0)            # patch 16: 768 + a whole pad block
    mean_std = torch.tensor(C.OPENAI_MEAN + C.OPENAI_STD, dtype=torch.float32, device=DEV)
    got = ops.vit_patches(torch.from_numpy(img).to(DEV), patch, mean_std, Kp).cpu()
    want = CC.patch_rows_model(img, patch, Kp)
    assert torch.equal(got, want)
    assert Kp == 3 * patch * patch or bool((got[:, 3 * patch * patch:] == 0).all())


@pytest.mark.parametrize("F_, L, C_", [(1, 50, 160), (3, 257, 208), (2, 197, 1664)])
def test_vit_tokens_equal_the_host_formula(F_, L, C_):
    g = torch.Generator().manual_seed(L)
    rows, cls, pos = torch.randn((F_ * (L - 1), C_), generator=g), torch.randn((C_,), generator=g), torch.randn((L, C_), generator=g)
    got = ops.vit_tokens(rows.to(DEV), cls.to(DEV), pos.to(DEV)).cpu()
    want = torch.cat([cls.reshape(1, 1, C_).expand(F_, 1, C_), rows.reshape(F_, L - 1, C_)], 1) + pos
    assert torch.equal(got, want.reshape(F_ * L, C_))


# ------------------------------------------------------------------------------------------------ preprocess
@pytest.mark.parametrize("H, W", CC.SOURCE_SIZES)
def test_preprocess_equals_the_host_model_in_both_forms(H, W):
    frames = CC.make_frames(2, H, W, H * 1000 + W)
    want = CC.preprocess_model(frames, 224)
    got = C.preprocess(torch.from_numpy(frames).to(DEV), 224).cpu().numpy()
    assert got.shape == want.shape == (2, 224, 224, 3) and np.array_equal(got, want)
    as_float = torch.from_numpy(CC.bytes_to_float(frames))
    assert np.array_equal(C.preprocess(as_float.to(DEV), 224).cpu().numpy(), want)
    rng = np.random.default_rng(H + W)
    free = rng.uniform(-0.1, 1.1, (1, 3, H, W)).astype(np.float32)                   # values that are no byte / 255, some outside [0, 1]
    assert np.array_equal(C.preprocess(torch.from_numpy(free).to(DEV), 224).cpu().numpy(), CC.preprocess_model(free, 224))


# ------------------------------------------------------------------------------------------------ the band cases end to end
@pytest.fixture(scope="module")
def towers():
    return {}


def tower(towers, name):
    if name not in towers:
        towers[name] = C.ClipVision(CC.weights(name), DEV)
    return towers[name]


@pytest.mark.parametrize("name", list(CC.CASES))
def test_tower_inside_the_band(name, towers):
    model = tower(towers, name)
    frames = torch.from_numpy(CC.frames(name)).to(DEV)
    feats, taps = model.features(frames, taps=True)
    table = CC.golden()[name]
    got = dict(taps, features=feats)
    report = {k: (table[k].deviation(got[k].cpu().numpy()), CC.gate(name, k)) for k in CC.KEYS}
    print(name, {k: f"{d:.2e} / {g:.2e}" for k, (d, g) in report.items()})
    for k, (d, g) in report.items():
        assert d <= g, (name, k, d, g)


def test_tower_does_not_depend_on_the_chunking(towers):
    name = "d104_l257"
    model = tower(towers, name)
    frames = torch.from_numpy(CC.frames(name)).to(DEV)
    per = model.bytes_per_image()
    assert model.images_per_chunk(3, per) == 1 and model.images_per_chunk(3, 3 * per) == 3
    one = model.features(frames, max_scratch_bytes=per)
    three = model.features(frames, max_scratch_bytes=3 * per)
    assert torch.equal(one, three)
    assert CC.golden()[name]["features"].deviation(one.cpu().numpy()) <= CC.gate(name, "features")
    with pytest.raises(M324Error, match="scratch bytes"):
        model.features(frames, max_scratch_bytes=per - 1)


def test_cosine_of_two_clips_against_the_fp64_oracle(towers):
    name = "d80_l50"
    model = tower(towers, name)
    a, b = CC.make_frames(2, 100, 60, 71), CC.make_frames(2, 100, 60, 72)
    got = C.ClipSimilarity(model)(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert got.dtype == torch.float64 and got.shape == (2,) and got.is_cuda
    heads, size = CC.CASES[name][1], CC.CASES[name][5]
    fa, fb = (CC.oracle(CC.preprocess_model(x, size), CC.state_dict(name), heads)["features"] for x in (a, b))
    entry = CC.golden()[name]["features"]
    bound = CC.cosine_bound(fa, fb, CC.gate(name, "features") * entry.rms)
    err = np.abs(got.cpu().numpy() - CC.cosine_model(fa, fb))
    print("cosine", got.cpu().numpy(), "err", err, "bound", bound)
    assert (err <= bound).all(), (err, bound)


def test_evaluate_clips_clip_statistics_and_identity(towers):
    model = tower(towers, "d80_l50")
    gt = torch.from_numpy(CC.make_frames(16, 64, 64, 81)).to(DEV)
    result = torch.from_numpy(CC.make_frames(16, 64, 64, 82)).to(DEV)
    metric = C.ClipSimilarity(model)
    score = C.evaluate_clips_clip(gt, result, model)
    want = C.clip_statistics(metric(gt, result).cpu().numpy())
    assert score.value == want.value and score.value_std == want.value_std and np.array_equal(score.per_frame, want.per_frame)
    assert score.per_frame.shape == (16,) and score.per_video.shape == (1,) and bool((np.abs(score.per_frame) < 1).all())
    same = metric(gt, gt.clone()).cpu().numpy()
    assert np.abs(same - 1.0).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ refusals without a launch
def test_entry_points_refuse_without_a_launch():
    h = lib.load()
    buf = torch.full((4096,), SENTINEL, dtype=torch.float32, device=DEV)
    src = torch.zeros((65536,), dtype=torch.float32, device=DEV)
    img = torch.zeros((224 * 224 * 3,), dtype=torch.uint8, device=DEV)
    o, s, u = buf.data_ptr(), src.data_ptr(), img.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    f = ctypes.c_float
    cases = [
        ("D % 8", h.m324_attention_tok(s, 36, o, 12, 1, 4, 1, 12, f(0.3), stream), -3),
        ("D > 128", h.m324_attention_tok(s, 408, o, 136, 1, 4, 1, 136, f(0.1), stream), -3),
        ("short ld", h.m324_attention_tok(s, 184, o, 64, 1, 4, 1, 64, f(0.1), stream), -1),
        ("short ldo", h.m324_attention_tok(s, 192, o, 60, 1, 4, 1, 64, f(0.1), stream), -1),
        ("null qkv", h.m324_attention_tok(None, 192, o, 64, 1, 4, 1, 64, f(0.1), stream), -1),
        ("null O", h.m324_attention_tok(s, 192, None, 64, 1, 4, 1, 64, f(0.1), stream), -1),
        ("misaligned", h.m324_attention_tok(s + 4, 192, o, 64, 1, 4, 1, 64, f(0.1), stream), -1),
        ("C > 4096", h.m324_layernorm_wide(s, 4100, s, s, f(1e-5), o, 4100, 1, 4100, stream), -3),
        ("C % 4", h.m324_layernorm_wide(s, 8, s, s, f(1e-5), o, 8, 1, 6, stream), -3),
        ("ldx < C", h.m324_layernorm_wide(s, 8, s, s, f(1e-5), o, 16, 1, 16, stream), -1),
        ("null w", h.m324_layernorm_wide(s, 16, None, s, f(1e-5), o, 16, 1, 16, stream), -1),
        ("Kp % 32", h.m324_vit_patches(u, 1, 224, 14, s, o, 600, stream), -3),
        ("Kp short", h.m324_vit_patches(u, 1, 224, 14, s, o, 576, stream), -3),
        ("S % patch", h.m324_vit_patches(u, 1, 224, 15, s, o, 704, stream), -1),
        ("null mean_std", h.m324_vit_patches(u, 1, 224, 14, None, o, 608, stream), -1),
        ("tokens C % 4", h.m324_vit_tokens(s, s, s, o, 1, 5, 6, stream), -3),
        ("null cls", h.m324_vit_tokens(s, None, s, o, 1, 5, 8, stream), -1),
    ]
    for what, rc, want in cases:
        assert rc == want, (what, rc, lib.last_error())
    assert h.m324_attention_tok(s, 36, o, 12, 1, 4, 1, 12, f(0.3), stream) == -3 and "D=12" in lib.last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    with pytest.raises(M324Error, match="D=12"):
        ops.attention_tok(src[:4 * 36].view(4, 36), 1, 4, 1, 12)
