"""The opt-in MXFP8 inference mode on the model: accuracy against the committed fp32 goldens (and trained-like weights), bit
identity where the mode must not change anything or must be deterministic."""
import numpy as np
import pytest
import torch

from conftest import CASES, load_golden, rel_err, synth_sd
from test_model_gpu import build, inputs, run, stage_errs
from test_trained_like_gpu import _model as tl_model, _run as tl_run, trained_like

pytestmark = pytest.mark.gpu

# Gates: the error measured on MI355X (default roles, transformer.MX_ROLES: the trunk and DINOv2 q|k|v projections) + 25 %.
# Each lies below the reference's own autocast(bf16)-vs-fp32 band (tests/golden/trained_like_band.json) for the nearest case and
# the same kind of weights: c1 against its c1 entry (synthetic 5.6e-2, trained-like 0.119), c2 against the c2-trunk entry
# (synthetic 8.5e-2).
MX_TOL = {                        # measured: c1 pcd 1.86e-2, dino 4.08e-2, block0 3.01e-2, trunk 3.80e-2; c2 2.18e-2 / 4.05e-2 / 3.01e-2 / 3.81e-2
    "c1": {"pcd_moved": 2.3e-2, "dino_tokens": 5.1e-2, "trunk_block0": 3.8e-2, "trunk_out": 4.8e-2},
    "c2": {"pcd_moved": 2.7e-2, "dino_tokens": 5.1e-2, "trunk_block0": 3.8e-2, "trunk_out": 4.8e-2},
}
MX_TOL_TRAINED_LIKE_C1 = 8.7e-2   # measured 6.96e-2 (vs the HIP fp32 forward, itself 1e-6 from the reference)
BAND_KEY = {"c1": "synthetic", "c2": "synthetic_c2_trunk"}


def _band():
    import json, os
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_like_band.json")))


def _mx(model):
    model.inference_precision = "mxfp8"
    return model


@pytest.mark.parametrize("case", ["c1", "c2"])
def test_mxfp8_forward_against_the_fp32_golden(case):
    model, dm = build(case)
    gold = load_golden(case)
    sample = inputs(case, with_target=False)
    out, cap = run(_mx(model), sample, "bf16")
    errs = stage_errs(cap, gold)
    errs["pcd_moved"] = rel_err(out.pcd_moved, torch.from_numpy(gold["pcd_moved"]))
    print(f"[{case} mxfp8] " + "  ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    band = _band()[BAND_KEY[case]]
    for k, tol in MX_TOL[case].items():
        assert tol < band
        assert errs[k] < tol, (k, errs)
    # the mode really ran: bf16 gives another result
    model.inference_precision = "bf16"
    out16, _ = run(model, sample, "bf16")
    assert not torch.equal(out16.pcd_moved, out.pcd_moved)


def test_mxfp8_trained_like_weights_at_c1():
    from motion324_amd import synth
    dims = CASES["c1"]["dims"]
    model, dm = tl_model(dims, trained_like(synth_sd(dims)))
    B, T, N, S, HW = CASES["c1"]["shape"]
    sample = {k: torch.from_numpy(v).cuda() for k, v in synth.synth_inputs(B, T, N, S, HW, seed=1).items()}
    out32, _ = tl_run(model, sample, "fp32")
    outmx, _ = tl_run(_mx(model), sample, "bf16")
    e = rel_err(outmx.pcd_moved, out32.pcd_moved.cpu())
    print(f"[trained-like c1 mxfp8] {e:.2e}")
    assert MX_TOL_TRAINED_LIKE_C1 < _band()["trained_like"]
    assert e < MX_TOL_TRAINED_LIKE_C1


def test_mxfp8_eager_graph_replay_repeat_and_mode_switches_are_bit_identical():
    import motion324_amd as m
    model, dm = build("c1")
    sample = inputs("c1", with_target=False)
    m.set_precision("bf16")
    try:
        with torch.no_grad():
            model.auto_graph = False
            bf_before = model(sample).pcd_moved.clone()
            _mx(model)
            e1 = model(sample).pcd_moved.clone()
            e2 = model(sample).pcd_moved.clone()
            fast = m.GraphedForward(model)
            g1 = fast(sample).pcd_moved.clone()
            g2 = fast(sample).pcd_moved.clone()
            model.inference_precision = "bf16"
            bf_after = model(sample).pcd_moved.clone()
            gb = fast(sample).pcd_moved.clone()            # a new key: the bf16 graph, not the MX one
    finally:
        m.set_precision(None)
    assert torch.equal(e1, e2) and torch.equal(g1, e1) and torch.equal(g2, e1)
    assert torch.equal(bf_after, bf_before) and torch.equal(gb, bf_before)
    assert not torch.equal(e1, bf_before)


def test_mxfp8_setting_changes_nothing_in_fp32_mode():
    model, dm = build("c1")
    sample = inputs("c1", with_target=False)
    ref, _ = run(model, sample, "fp32")
    got, _ = run(_mx(model), sample, "fp32")
    assert torch.equal(got.pcd_moved, ref.pcd_moved)


def test_mxfp8_setting_changes_nothing_in_a_training_step():
    """A training step (training.forward_backward: fusion_disabled, its frozen DINO under fusion_allowed with grad off) gives the
    same loss and gradients with the setting on -- the model in EVAL mode (so mx_effective's training check does not decide it)
    and even with an MXFP8 scope of every built role left open around the step: only the training step's own predicate
    (fusion_disabled closes the scope, fusion_allowed does not reopen it) keeps the frozen DINO and the trunk bf16."""
    import motion324_amd as m
    from motion324_amd import synth, training, transformer

    def step(mode):
        dims = CASES["tiny"]["dims"] | {"d": 384}
        dm = synth.Dims(**dims)
        cfg = synth.make_config(frames=dm.frames, d=384, tokens=dm.tokens, pcd_layers=dm.pcd_layers, n_layer=dm.n_layer)
        cfg["model"]["dino"] = {"depth": dm.dino_depth}
        cfg["model"]["inference_precision"] = mode
        torch.manual_seed(0)
        model = m.Motion_Latent_Model(cfg).cuda().eval()
        sample = inputs("tiny")
        m.set_precision("bf16")
        try:
            with transformer.mx_scope(transformer.MX_ROLES_BUILT if mode == "mxfp8" else ()):
                loss, _, store = training.forward_backward(model, sample, drop_seed=1)
            grads = [store.get(p).clone() for p in model.parameters() if p.requires_grad and store.get(p) is not None]
        finally:
            m.set_precision(None)
        torch.cuda.synchronize()
        return float(loss), grads

    l0, g0 = step("bf16")
    l1, g1 = step("mxfp8")
    assert l0 == l1 and len(g0) == len(g1) and len(g0) > 0
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_mxfp8_setting_changes_nothing_in_a_model_training_step():
    """The reference's loop form: model.train(); model(batch).loss_metrics.loss.backward() -- loss and every .grad unchanged."""
    import motion324_amd as m
    from motion324_amd import synth

    def step(mode):
        dims = CASES["tiny"]["dims"] | {"d": 384}
        dm = synth.Dims(**dims)
        cfg = synth.make_config(frames=dm.frames, d=384, tokens=dm.tokens, pcd_layers=dm.pcd_layers, n_layer=dm.n_layer)
        cfg["model"]["dino"] = {"depth": dm.dino_depth}
        cfg["model"]["inference_precision"] = mode
        torch.manual_seed(0)
        model = m.Motion_Latent_Model(cfg).cuda().train()
        sample = inputs("tiny")
        m.set_precision("bf16")
        try:
            out = model(sample)
            out.loss_metrics.loss.backward()
        finally:
            m.set_precision(None)
        torch.cuda.synchronize()
        return float(out.loss_metrics.loss), [p.grad.clone() for p in model.parameters() if p.grad is not None]

    l0, g0 = step("bf16")
    l1, g1 = step("mxfp8")
    assert l0 == l1 and len(g0) == len(g1) and len(g0) > 0
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_mxfp8_pipelined_driver_equals_the_plain_loop():
    import motion324_amd as m
    from motion324_amd import synth
    from motion324_amd.inference import run_model_inference
    dims = dict(d=384, d_head=64, tokens=8, pcd_layers=1, n_layer=2, frames=4, dino_depth=2)
    cfg = synth.make_config(frames=4, d=384, tokens=8, pcd_layers=1, n_layer=2)
    cfg["model"]["dino"] = {"depth": 2}
    cfg["model"]["inference_precision"] = "mxfp8"
    model = m.Motion_Latent_Model(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_sd(dims).items()}, strict=False)
    model = model.eval().cuda()
    s = synth.synth_inputs(1, 30, 24, 60, 64, seed=9)
    video = torch.from_numpy(s.pop("rgb_video"))[0]
    inp = {k: torch.from_numpy(v).cuda() for k, v in s.items()}
    m.set_precision("bf16")
    try:
        model.auto_graph = False
        plain = run_model_inference(model, inp, video, cfg, "cuda", pipelined=False)
        model.auto_graph = True
        got = run_model_inference(model, inp, video, cfg, "cuda")
        model.inference_precision = "bf16"
        model.auto_graph = False
        bf = run_model_inference(model, inp, video, cfg, "cuda", pipelined=False)
    finally:
        m.set_precision(None)
    assert torch.isfinite(plain).all()
    assert torch.equal(got, plain)
    assert not torch.equal(bf, plain)


def test_mxfp8_with_the_mlp_roles_too(monkeypatch):
    """The MLP roles (fc1 + GELU -> MX -> fc2) are built but not in the default table (they do not win, profiles/mxfp8.md); with
    every built role switched on the c1 clip stays inside its gate (measured 3.63e-2, + 25 %; the c1 band is 5.6e-2)."""
    from motion324_amd import transformer
    monkeypatch.setattr(transformer, "MX_ROLES", transformer.MX_ROLES_BUILT)
    model, dm = build("c1")
    gold = load_golden("c1")
    out, cap = run(_mx(model), inputs("c1", with_target=False), "bf16")
    e = rel_err(out.pcd_moved, torch.from_numpy(gold["pcd_moved"]))
    print(f"[c1 mxfp8, all roles] pcd_moved={e:.2e}")
    assert 4.5e-2 < _band()["synthetic"]
    assert e < 4.5e-2
