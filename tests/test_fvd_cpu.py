"""FVD without a GPU: the binding, every host-side refusal, the SAME rule, the weight loader and the batch-norm fold, the Frechet
distance, the sub-video rule, the committed band, and the power of the gate against five planted faults
(tests/ERROR_BOUNDS_FVD.md)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO

import fvd_cases as FC
from motion324_amd import fvd as V
from motion324_amd.lib import M324Error

ENTRY_POINTS = ("m324_conv3d", "m324_conv3d_tile", "m324_maxpool3d", "m324_i3d_head", "m324_fvd_prepare")


# ------------------------------------------------------------------------------------------------ binding
def test_entry_points_are_declared_bound_and_built():
    from motion324_amd import build, lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "m324.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, flags=re.S)
        assert proto, name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
        assert len(proto.group(1).split(",")) == len(lib.SIGNATURES[name]), name
    assert lib.ABI_VERSION == 23 and lib.load().m324_abi_version() == 23          # added entry points: no bump
    assert "conv3d.hip" in build.SOURCES and "conv.hip" in build.SOURCES
    for macro, value in (("M324_CONV3D_MAX_STRIDE", ops.CONV3D_MAX_STRIDE), ("M324_I3D_HEAD_MAX_SAMPLES", ops.I3D_HEAD_MAX_SAMPLES),
                         ("M324_I3D_HEAD_MAX_SIDE", ops.I3D_HEAD_MAX_SIDE), ("M324_FVD_U8", ops.FVD_MODES[torch.uint8]),
                         ("M324_FVD_F32", ops.FVD_MODES[torch.float32])):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", header).group(1)) == value, macro


def test_c_abi_refuses_what_is_outside_the_shape_contract():
    """validation comes before the first HIP call, so it shows without a GPU"""
    from motion324_amd import lib
    h = lib.load()
    p = 4096                                             # an aligned stand-in: no call below gets as far as using it
    ok = dict(a=p, lda=16, wp=p, bias=p, out=p, ldo=48, samples=1, T=4, H=4, W=4, Cin=16, Cout=48, box=3, s=(1, 1, 1), pad=(1, 1, 1), relu=1, tile=0)

    def conv(**kw):
        a = dict(ok, **kw)
        return h.m324_conv3d(a["a"], a["lda"], a["wp"], a["bias"], a["out"], a["ldo"], a["samples"], a["T"], a["H"], a["W"], a["Cin"], a["Cout"],
                             a["box"], *a["s"], *a["pad"], a["relu"], a["tile"], None)

    for bad, word in ((dict(box=5), "tap box"), (dict(box=2), "tap box"), (dict(s=(1, 3, 1)), "stride"), (dict(s=(0, 1, 1)), "stride"),
                      (dict(pad=(3, 1, 1)), "front padding"), (dict(pad=(1, -1, 1)), "front padding"), (dict(box=1), "front padding"),
                      (dict(Cin=6), "multiple of 4"), (dict(Cin=0), "multiple of 4"), (dict(Cout=12), "multiple of 8"), (dict(Cout=8192), "multiple of 8"),
                      (dict(lda=8), "lda"), (dict(lda=18), "lda"), (dict(ldo=40), "ldo"), (dict(ldo=2 ** 20), "ldo"), (dict(T=0), "at least 1"),
                      (dict(samples=0), "at least 1"), (dict(samples=2 ** 11, T=2 ** 4, H=2 ** 8, W=2 ** 8), "2^31"), (dict(relu=2), "relu"),
                      (dict(tile=16), "tile"), (dict(a=None), "null"), (dict(bias=None), "null"), (dict(a=p + 4), "aligned"),
                      (dict(out=p + 8), "aligned"), (dict(bias=p + 2), "aligned")):
        assert conv(**bad) == -1 and word in lib.last_error(), (bad, lib.last_error())
    assert h.m324_conv3d_tile(0, 64) < 0 and h.m324_conv3d_tile(100, 12) < 0
    assert h.m324_conv3d_tile(10 ** 6, 384) == 128 and h.m324_conv3d_tile(1000, 384) == 64 and h.m324_conv3d_tile(10 ** 6, 208) == 128
    assert h.m324_conv3d_tile(10 ** 6, 48) == 64 and h.m324_conv3d_tile(10 ** 6, 24) == 32 and h.m324_conv3d_tile(10 ** 6, 32) == 32

    def pool(inp=p, out=p, ldo=16, samples=1, T=4, H=4, W=4, C=16, k=(3, 3, 3), s=(1, 1, 1), pad=(1, 1, 1)):
        return h.m324_maxpool3d(inp, out, ldo, samples, T, H, W, C, *k, *s, *pad, None)

    for bad, word in ((dict(k=(3, 3, 1)), "window"), (dict(k=(2, 3, 3)), "window"), (dict(s=(2, 2, 4)), "stride"), (dict(pad=(1, 1, 3)), "front padding"),
                      (dict(k=(2, 2, 2), pad=(0, 2, 0)), "front padding"), (dict(C=6), "multiple of 4"), (dict(ldo=12), "ldo"), (dict(H=0), "at least 1"),
                      (dict(inp=None), "null"), (dict(out=p + 4), "aligned"), (dict(samples=2 ** 15, H=2 ** 8, W=2 ** 8), "2^31")):
        assert pool(**bad) == -1 and word in lib.last_error(), (bad, lib.last_error())

    def head(x=p, w=p, b=p, pooled=p, out=p, samples=1, T=2, hw=7, C=1024, classes=400):
        return h.m324_i3d_head(x, w, b, pooled, out, samples, T, hw, C, classes, None)

    for bad, word in ((dict(T=1), "T must"), (dict(hw=0), "hw"), (dict(hw=65), "hw"), (dict(C=1022), "multiple of 4"), (dict(classes=0), "classes"),
                      (dict(samples=0), "samples"), (dict(pooled=None), "null"), (dict(w=p + 2), "aligned")):
        assert head(**bad) == -1 and word in lib.last_error(), (bad, lib.last_error())

    def prepare(src=p, mode=0, frames=1, H=8, W=8, Hr=8, Wr=8, y0=0, x0=0, Ho=8, Wo=8, dst=p):
        return h.m324_fvd_prepare(src, mode, frames, H, W, Hr, Wr, y0, x0, Ho, Wo, dst, None)

    for bad, word in ((dict(mode=2), "mode"), (dict(frames=0), "at least 1"), (dict(W=0), "at least 1"), (dict(H=2 ** 15), "sizes up to"),
                      (dict(y0=1), "crop"), (dict(Wo=9), "crop"), (dict(x0=-1), "crop"), (dict(frames=2 ** 26), "2^31"), (dict(src=None), "null"),
                      (dict(dst=p + 4), "aligned"), (dict(mode=1, src=p + 2), "aligned")):
        assert prepare(**bad) == -1 and word in lib.last_error(), (bad, lib.last_error())


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from motion324_amd import ops
    x = torch.zeros(1, 2, 4, 4, 16)
    wp, b = torch.zeros(ops.conv3d_kpad(16, 3), 48), torch.zeros(48)
    with pytest.raises(M324Error, match="HIP device"):
        ops.conv3d(x, wp, b, box=3)
    with pytest.raises(M324Error, match="tap box"):
        ops.conv3d(x, wp, b, box=5)
    with pytest.raises(M324Error, match="HIP device"):
        ops.maxpool3d(x, (3, 3, 3), (1, 1, 1))
    with pytest.raises(M324Error, match="window"):
        ops.maxpool3d(x, (3, 1, 3), (1, 1, 1))
    with pytest.raises(M324Error, match="HIP device"):
        ops.i3d_head(x, torch.zeros(16, 400), torch.zeros(400))
    with pytest.raises(M324Error, match="HIP device"):
        ops.fvd_prepare(torch.zeros(1, 10, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(M324Error, match="HIP device"):
        V.I3D(V.load_i3d_weights(FC.state_dict()), "cpu")
    with pytest.raises(M324Error, match="head_window"):
        V.I3D(V.load_i3d_weights(FC.state_dict()), "cpu", head_window=(3, 7, 7))
    assert ops.conv3d_kpad(4, 7) == 1376 and ops.conv3d_kpad(192, 3) == 5184 and ops.conv3d_kpad(832, 1) == 832 and ops.conv3d_kpad(24, 1) == 32
    with pytest.raises(M324Error, match=r"\[Cout,Cin,k,k,k\]"):
        ops.pack_conv3d_weight(torch.zeros(8, 4, 3, 3))
    with pytest.raises(M324Error, match=r"\[Cout,Cin,k,k,k\]"):
        ops.pack_conv3d_weight(torch.zeros(8, 4, 3, 3, 5))
    # the packed layout: row ((dt k + dh) k + dw) Cin4 + c, pad channels and pad rows zero
    w = torch.arange(8 * 3 * 27, dtype=torch.float32).reshape(8, 3, 3, 3, 3) + 1
    packed = ops.pack_conv3d_weight(w)
    assert tuple(packed.shape) == (112, 8)
    assert packed[(1 * 9 + 2 * 3 + 0) * 4 + 2, 5] == w[5, 2, 1, 2, 0] and not packed[3::4].any() and not packed[108:].any()
    # the geometry of the reference's preprocess_single
    assert ops.fvd_geometry(512, 512) == (224, 224, 0, 0, 224, 224) and ops.fvd_geometry(224, 224) == (224, 224, 0, 0, 224, 224)
    assert ops.fvd_geometry(48, 80) == (224, 374, 0, 75, 224, 224) and ops.fvd_geometry(80, 48) == (374, 224, 75, 0, 224, 224)
    assert ops.fvd_geometry(30, 50, None) == (30, 50, 0, 0, 30, 50)


def test_model_refuses_sizes_by_name():
    """host-only checks of I3D.check_videos: they need no device"""
    model = V.I3D.__new__(V.I3D)
    N, T, H, W, window, resolution = FC.REFUSED
    model.head_window, model.resolution = window, resolution
    with pytest.raises(M324Error, match=r"96 x 64.*3 x 2.*\(2, 2, 2\)"):
        model.check_videos(torch.zeros((N, T, H, W, 3), dtype=torch.uint8))
    with pytest.raises(M324Error, match="at least 10 frames, got 9"):
        model.check_videos(torch.zeros((1, 9, 64, 64, 3), dtype=torch.uint8))
    with pytest.raises(M324Error, match=r"uint8 \[N,T,H,W,3\]"):
        model.check_videos(torch.zeros((1, 10, 3, 64, 64), dtype=torch.uint8))
    assert model.check_videos(torch.zeros((2, 10, 64, 64, 3), dtype=torch.uint8)) == (2, 10, 64, 64)
    model.head_window, model.resolution = (2, 7, 7), 224
    assert model.check_videos(torch.zeros((1, 32, 48, 80, 3), dtype=torch.uint8)) == (1, 32, 224, 224)
    assert [s for _, s, _ in V.trunk_shapes(10, 64, 64)][::5] == [(10, 64, 64), (5, 8, 8), (3, 4, 4), (2, 2, 2)]
    assert V.trunk_shapes(32, 224, 224)[-1] == ("Mixed_5c", (4, 7, 7), 1024)
    assert V.scratch_bytes_per_video(32, 224, 224) < 128 << 20


# ------------------------------------------------------------------------------------------------ the SAME rule
@pytest.mark.parametrize("s", (1, 2))
@pytest.mark.parametrize("k", (1, 2, 3, 7))
def test_same_padding_against_window_enumeration(k, s):
    """brute force: the output size is ceil(n / s); the smallest total padding with which that many windows fit is split with
    the smaller half in front"""
    from motion324_amd import ops
    for n in range(1, 18):
        out = -(-n // s)
        total = next(t for t in range(0, k + s) if (n + t - k) // s + 1 >= out and n + t >= k)
        front, size = ops.same_padding(n, k, s)
        assert (front, size) == (total // 2, out), (n, k, s)
        # every output window starts inside [-front, n) and the last one ends no further than the back padding allows
        starts = [o * s - front for o in range(size)]
        assert starts[0] == -front and starts[-1] + k <= n + (total - front) and starts[-1] < n
    with pytest.raises(M324Error, match="at least 1"):
        ops.same_padding(0, 3, 1)


# ------------------------------------------------------------------------------------------------ weights
def _same(w1, w2):
    return all(torch.equal(w1.units[k][0], w2.units[k][0]) and torch.equal(w1.units[k][1], w2.units[k][1]) for k in V.UNITS) and \
        torch.equal(w1.logits[0], w2.logits[0]) and torch.equal(w1.logits[1], w2.logits[1])


class _Holder(torch.nn.Module):
    """a module tree that holds a state dict's tensors under its names, to be scripted into a TorchScript file"""

    def __init__(self, state):
        super().__init__()
        for key, value in state.items():
            node, parts = self, key.split(".")
            for part in parts[:-1]:
                if not hasattr(node, part):
                    node.add_module(part, torch.nn.Module())
                node = getattr(node, part)
            node.register_buffer(parts[-1], value.clone())

    def forward(self, x):
        return x


def test_loader_accepts_the_three_forms(tmp_path):
    state = FC.state_dict()
    w = V.load_i3d_weights(state)
    assert len(w.units) == 57 and tuple(w.logits[0].shape) == (1024, 400) and tuple(w.logits[1].shape) == (400,)
    assert tuple(w.units["Conv3d_1a_7x7"][0].shape) == (1376, 64) and tuple(w.units["Mixed_5c.b1b"][0].shape) == (5184, 384)
    torch.save(state, tmp_path / "i3d.pth")
    assert _same(w, V.load_i3d_weights(str(tmp_path / "i3d.pth")))
    torch.save({"state_dict": {"module." + k: v for k, v in state.items()}}, tmp_path / "wrapped.pth")
    assert _same(w, V.load_i3d_weights(str(tmp_path / "wrapped.pth")))
    tracked = dict(state, **{"Mixed_3b.b0.bn.num_batches_tracked": torch.tensor(7)})
    assert _same(w, V.load_i3d_weights(tracked))
    torch.jit.script(_Holder({"model." + k: v for k, v in state.items()})).save(str(tmp_path / "i3d_torchscript.pt"))
    assert _same(w, V.load_i3d_weights(str(tmp_path / "i3d_torchscript.pt")))
    # a missing bn.weight counts as ones
    ones = dict(state, **{"Mixed_4b.b2a.bn.weight": torch.ones(16)})
    without = {k: v for k, v in ones.items() if k != "Mixed_4b.b2a.bn.weight"}
    assert _same(V.load_i3d_weights(ones), V.load_i3d_weights(without))


def test_loader_refuses_wrong_shapes_and_foreign_keys(tmp_path):
    state = FC.state_dict()
    with pytest.raises(M324Error, match=r"'Mixed_3c.b1b.conv3d.weight' has shape \(192, 128, 3, 3\), expected \(192, 128, 3, 3, 3\)"):
        V.load_i3d_weights(dict(state, **{"Mixed_3c.b1b.conv3d.weight": torch.zeros(192, 128, 3, 3)}))
    with pytest.raises(M324Error, match=r"expected \(400, 1024, 1, 1, 1\)"):
        V.load_i3d_weights(dict(state, **{"logits.conv3d.weight": torch.zeros(400, 1024)}))
    with pytest.raises(M324Error, match="no key 'Mixed_5b.b3b.bn.running_var'"):
        V.load_i3d_weights({k: v for k, v in state.items() if k != "Mixed_5b.b3b.bn.running_var"})
    with pytest.raises(M324Error, match="2 keys match no part of I3D: Mixed_6a.b0.conv3d.weight, features.0.weight"):
        V.load_i3d_weights(dict(state, **{"features.0.weight": torch.zeros(1), "Mixed_6a.b0.conv3d.weight": torch.zeros(1)}))
    with pytest.raises(M324Error, match="not finite"):
        V.load_i3d_weights(dict(state, **{"Conv3d_2b_1x1.bn.bias": torch.full((64,), float("nan"))}))
    with pytest.raises(M324Error, match="no such file"):
        V.load_i3d_weights(str(tmp_path / "absent.pt"))
    with pytest.raises(M324Error, match="state dict"):
        V.load_i3d_weights(3)


def test_batch_norm_fold_against_unfolded_fp64():
    """the folded unit, conv(x, w') + b' in fp64, equals conv + batch norm evaluated unfolded in fp64 to rounding; and what the
    loader packs is that w', b' rounded once to fp32, in the K-major layout"""
    from motion324_amd import ops
    state = FC.state_dict()
    g = torch.Generator().manual_seed(5)
    for unit in ("Conv3d_1a_7x7", "Mixed_3b.b2b", "Mixed_4e.b1a"):
        cin, cout, box = V.UNITS[unit]
        w = state[f"{unit}.conv3d.weight"]
        gamma, beta, mean, var = (state[f"{unit}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
        wf, bf = V.fold_batch_norm(w, gamma, beta, mean, var)
        assert wf.dtype == torch.float64 and bf.dtype == torch.float64
        x = torch.randn((1, cin, box + 1, box + 2, box), generator=g, dtype=torch.float64)
        unfolded = F.batch_norm(F.conv3d(x, w.double()), mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, V.BN_EPS)
        folded = F.conv3d(x, wf, bf)
        assert (folded - unfolded).abs().max() <= 1e-12 * unfolded.abs().max()
        wp, b = V.load_i3d_weights(state).units[unit]
        assert torch.equal(wp, ops.pack_conv3d_weight(wf.to(torch.float32))) and torch.equal(b, bf.to(torch.float32))
    # eps is the model's 1e-3: the fold with 1e-5 differs by more than rounding
    wf5, _ = V.fold_batch_norm(w, gamma, beta, mean, var, eps=1e-5)
    assert ((wf5 - wf).abs().max() / wf.abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------------ the distance
def test_frechet_distance_rules():
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(1, 400)), rng.normal(size=(1, 400))
    assert V.frechet_distance(a, b) == float(np.square(a - b).sum())                      # N == 1: the squared distance of the rows
    f1, f2 = rng.normal(size=(5, 400)), rng.normal(size=(5, 400)) + 0.3
    d12, d21 = V.frechet_distance(f1, f2), V.frechet_distance(f2, f1)
    assert d12 > 0 and abs(d12 - d21) <= 1e-12 * d12                                      # symmetric
    assert V.frechet_distance(f1, f1.copy()) == 0.0 and V.frechet_distance(a, a.copy()) == 0.0
    with pytest.raises(M324Error, match="single row"):
        V.frechet_distance(a, f1)
    with pytest.raises(M324Error, match="one d"):
        V.frechet_distance(f1, f2[:, :10])
    with pytest.raises(M324Error, match="not finite"):
        V.frechet_distance(f1, np.full_like(f2, np.inf))


def test_frechet_distance_against_sqrtm_at_full_rank():
    from scipy.linalg import sqrtm
    rng = np.random.default_rng(4)
    f1 = rng.normal(size=(40, 6)) @ rng.normal(size=(6, 6))
    f2 = rng.normal(size=(40, 6)) @ rng.normal(size=(6, 6)) + rng.normal(size=6)
    s1, s2 = np.cov(f1, rowvar=False), np.cov(f2, rowvar=False)
    root = sqrtm(s1 @ s2)
    ref = float(np.real(np.square(f1.mean(0) - f2.mean(0)).sum() + np.trace(s1 + s2 - 2 * root)))
    assert abs(V.frechet_distance(f1, f2) - ref) <= 1e-9 * abs(ref)


def test_frechet_distance_rank_deficient_against_small_eigenvalues():
    """d = 400, N = 3: S1 S2 has rank 2.  Its non-zero eigenvalues are those of the N x N matrix (A1 A2^T)(A2 A1^T)."""
    rng = np.random.default_rng(5)
    f1, f2 = rng.normal(size=(3, 400)), 1.5 * rng.normal(size=(3, 400)) + 0.1
    a1, a2 = ((f - f.mean(0)) / np.sqrt(2.0) for f in (f1, f2))
    small = (a1 @ a2.T) @ (a2 @ a1.T)
    eig = np.clip(np.linalg.eigvals(small).real, 0, None)
    ref = float(np.square(f1.mean(0) - f2.mean(0)).sum() + np.trace(np.cov(f1, rowvar=False)) + np.trace(np.cov(f2, rowvar=False)) - 2 * np.sqrt(eig).sum())
    got = V.frechet_distance(f1, f2)
    assert abs(got - ref) <= 1e-9 * abs(ref) and got > 0


def test_subvideo_rule_is_the_one_of_lpips():
    assert V.subvideo_frames is __import__("motion324_amd.perceptual", fromlist=["x"]).subvideo_frames
    assert V.subvideo_frames(40) == [list(range(32))]
    assert V.subvideo_frames(16) == [list(range(16)) + list(range(15, -1, -1))]
    assert len(V.subvideo_frames(64)) == 2
    with pytest.raises(M324Error, match="at least 16"):
        V.subvideo_frames(15)
    with pytest.raises(M324Error, match="equal shapes"):
        V.check_clip_pair(torch.zeros((32, 8, 8, 3), dtype=torch.uint8), torch.zeros((32, 8, 9, 3), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ band and power
def test_band_file_matches_the_cases_and_the_document():
    table = FC.golden()
    text = open(os.path.join(REPO, "tests", "ERROR_BOUNDS_FVD.md")).read()
    rows = re.search(r"<!-- band:begin -->\n(.*?)<!-- band:end -->", text, flags=re.S).group(1)
    for name, (N, T, H, W, window, _) in FC.CASES.items():
        row = next(r for r in rows.splitlines() if r.startswith(f"| {name} |"))
        for key in FC.KEYS:
            e = table[name][key]
            assert f"{e.band:.2e}" in row, (name, key)
            assert 1e-8 < e.band < 1e-4 and 0.3 < e.positive < 0.7 and 0.05 < e.rms < 20, (name, key, e.band, e.positive, e.rms)
            assert e.ref.shape == (min(e.size, FC.SAMPLE),) and e.ref.dtype == np.float64
        shape = V.trunk_shapes(T, H, W)[-1]
        assert table[name]["Mixed_5c"].size == N * shape[1][0] * shape[1][1] * shape[1][2] * 1024 and table[name]["features"].size == N * 400


@pytest.fixture(scope="module")
def small_cases():
    return {name: FC.videos(name) for name in ("t16_64", "t10_64")}


def test_fp64_oracle_reproduces_the_golden_values(small_cases):
    table = FC.golden()
    for name, frames in small_cases.items():
        out = FC.oracle(frames)
        for key in FC.KEYS:
            assert table[name][key].deviation(out[key]) <= 1e-12, (name, key)


@pytest.mark.parametrize("fault", FC.FAULTS)
def test_gate_sees_the_planted_fault(fault, small_cases):
    table = FC.golden()
    seen = []
    for name, frames in small_cases.items():
        out = FC.oracle(frames, fault=fault)
        seen += [(name, key) for key in FC.KEYS if not table[name][key].deviation(out[key]) <= FC.gate(name, key)]
        if seen:
            break
    assert seen, f"the gate does not see {fault}"
