"""The motion latent API on the GPU: encode_motion / decode_motion against the closed forward (bit for bit), against the CPU
oracle (fp32, FP32_TOL), under decoder chunking and frame subsets, under hipGraph replay, through the long-video driver, and
across precisions.

Configurations: `tiny` (tests/conftest.py: d 192, 8 tokens, B 2, T 3, N 40 -- the unfused projections and the general attention
kernel) and `small64` (d 384, 64 tokens, B 1, T 4, N 200, 64 x 64 frames -- the smallest shape on the product's decoder path:
paired LayerNorm / projection launches, head-major epilogues, attn_frames_kernel on frame pairs, the LayerNorm fold; N is no
multiple of 64; the width is 384 because the model's constructor refuses 256: transformer.d must be a multiple of 12, and the MXFP8
mode needs a multiple of 128).

Bit-for-bit equalities are the project's standing expectation (row-wise kernels, schedule-independent GEMM results,
test_decoder_chunking_is_invisible), not a new tolerance.  The bf16 kernels change path at 64 rows (transformer.fuse_proj,
LNFold.usable, the skinny GEMM).  The decode-only chunk plan and the frame subsets keep every pass on the whole decode's side of
that line (Motion_Latent_Model._decode / decode_motion), which is what makes them invisible in bf16 as well; the DECODE_ROWS
values below are at least 65, so the passes hold as many rows as the value asks for."""
import pytest
import torch

from conftest import CASES, rel_err, synth_sd

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3            # tests/test_model_gpu.py
BF16_TOL = 6e-3

CONFIGS = {
    "tiny": dict(dims=CASES["tiny"]["dims"], shape=CASES["tiny"]["shape"], n2=23,
                 # DECODE_ROWS -> (points per pass, frames per pass) at N 40, T 3: 100 -> (40, 2); 70 -> (35, 2)
                 decode_rows=(100, 70)),
    "small64": dict(dims=dict(d=384, d_head=64, tokens=64, pcd_layers=1, n_layer=2, frames=4, dino_depth=2),
                    shape=(1, 4, 200, 128, 64), n2=77,
                    # at N 200, T 4: 400 -> (200, 2); 268 -> (67, 4): three passes of 67 points; 200 -> (100, 2)
                    decode_rows=(400, 268, 200)),
}
POINTS = ("ref_pcd", "ref_normal", "ref_rgb")


def build(name, frames=None):
    import motion324_amd as m
    from motion324_amd import synth
    dims = dict(CONFIGS[name]["dims"])
    if frames is not None:
        dims["frames"] = frames
    dm = synth.Dims(**dims)
    cfg = synth.make_config(frames=dm.frames, d=dm.d, d_head=dm.d_head, tokens=dm.tokens, pcd_layers=dm.pcd_layers,
                            n_layer=dm.n_layer)
    cfg["model"]["dino"] = {"depth": dm.dino_depth}
    model = m.Motion_Latent_Model(cfg)
    sd = {k: torch.from_numpy(v) for k, v in synth_sd(dims).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert set(missing) <= {"pos_embed", "point_embed.basis"} and not unexpected
    model.auto_graph = False                     # eager unless a test turns the replay on
    return model.eval().cuda(), sd, cfg, dm


def inputs(name, seed=1):
    from motion324_amd import synth
    B, T, N, S, HW = CONFIGS[name]["shape"]
    s = synth.synth_inputs(B, T, N, S, HW, seed=seed)
    return {k: torch.from_numpy(v).cuda() for k, v in s.items()}


def other_points(name, seed=11):
    from motion324_amd import synth
    B, T, N, S, HW = CONFIGS[name]["shape"]
    s = synth.synth_inputs(B, 1, CONFIGS[name]["n2"], 8, 14, seed=seed)
    return [torch.from_numpy(s[k]).cuda() for k in POINTS]


def clip_only(sample):
    return {k: v for k, v in sample.items() if k not in POINTS}


class precision:
    def __init__(self, p):
        self.p = p

    def __enter__(self):
        import motion324_amd as m
        m.set_precision(self.p)
        self.ng = torch.no_grad()
        self.ng.__enter__()

    def __exit__(self, *exc):
        import motion324_amd as m
        self.ng.__exit__(*exc)
        m.set_precision(None)


def same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(a, b), float((a - b).abs().max())


# ---------------------------------------------------------------------------------------------- 1, 2: the closed forward
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small64"])
def test_encode_then_decode_is_the_forward_bit_for_bit(name, prec):
    """decode_motion(encode_motion(s), s's points) == model(s).pcd_moved; the latent is rows 4..4+K of the captured trunk_out;
    a second point set with another N decodes from the SAME latent to what the forward gives for it."""
    from motion324_amd import MotionLatent
    model, sd, cfg, dm = build(name)
    sample = inputs(name)
    B, T, N, S, HW = CONFIGS[name]["shape"]
    K, C = dm.tokens, dm.d
    with precision(prec):
        full = model(sample).pcd_moved
        cap = {}
        model._capture = cap
        try:
            lat_cap = model.encode_motion(sample)
        finally:
            model._capture = None
        lat = model.encode_motion(clip_only(sample))                 # no ref_pcd / ref_normal / ref_rgb needed
        got = model.decode_motion(lat, *(sample[k] for k in POINTS))
        pts2 = other_points(name)
        full2 = model(dict(sample, **dict(zip(POINTS, pts2)))).pcd_moved
        got2 = model.decode_motion(lat, *pts2)
        torch.cuda.synchronize()
    assert isinstance(lat, MotionLatent) and lat.tokens.dtype == torch.float32 and lat.tokens.shape == (B, T, K, C)
    assert (lat.d, lat.K, lat.frames, lat.from_ref) == (C, K, dm.frames, [])
    assert "decoder_out_t0" not in cap                               # encode-only: no decoder ran
    same(lat.tokens, cap["trunk_out"].reshape(B, T, -1, C)[:, :, 4:4 + K])
    same(lat_cap.tokens, lat.tokens)
    same(got, full)
    assert got2.shape == (B, T, CONFIGS[name]["n2"], 3)
    same(got2, full2)
    with precision(prec):                                            # m324_keep_latent on the whole forward: both results
        both = model(dict(sample, m324_keep_latent=True))
    same(both.pcd_moved, full)
    same(both.latent, lat.tokens)


# ---------------------------------------------------------------------------------------------- 3: chunks and subsets
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small64"])
def test_decoder_chunks_and_frame_subsets_are_invisible(name, prec, monkeypatch):
    """Point chunks, frame chunks and frame subsets ([2, 0]; [1] and [0, 2, 1]: odd counts; slice(0, 4, 2)) against the full
    decode, bit for bit.  On tiny one frame is 40 rows and the whole decode 120 per sample, on small64 one frame's k|v side is 64
    rows: [1] alone would run the bf16 kernels' small-problem paths, and T = 3 ends any frame chunking in a single frame."""
    import motion324_amd.Pcd_motion as pm
    model, sd, cfg, dm = build(name)
    sample = inputs(name)
    B, T, N, S, HW = CONFIGS[name]["shape"]
    pts = [sample[k] for k in POINTS]
    subsets = ([2, 0], [1], slice(0, 4, 2), [0, 2, 1])
    launches = []
    real = model.decoder_block
    monkeypatch.setattr(model, "decoder_block", lambda P, Kd, Vd, pf, Q=None: (launches.append((Kd.shape[0], pf.shape[0])), real(P, Kd, Vd, pf, Q))[1])
    seen, differ = {}, []

    def check(what, got, want):
        if not torch.equal(got, want):
            differ.append((what, float((got - want).abs().max()), rel_err(got, want)))
    with precision(prec):
        lat = model.encode_motion(sample)
        full = model.decode_motion(lat, *pts)
        assert launches == [(T, N)] * B
        for rows in (None,) + CONFIGS[name]["decode_rows"]:
            if rows is not None:
                monkeypatch.setattr(pm, "DECODE_ROWS", rows)
                del launches[:]
                check(f"DECODE_ROWS={rows}", model.decode_motion(lat, *pts), full)
                assert all(t * n <= rows for t, n in launches) and len(launches) > B, launches
                seen[rows] = (max(n for _, n in launches), max(t for t, _ in launches))
            for fr in subsets:
                idx = list(range(T))[fr] if isinstance(fr, slice) else fr
                got = model.decode_motion(lat, *pts, frames=fr)
                assert got.shape == (B, len(idx), N, 3)
                check(f"DECODE_ROWS={rows} frames={fr}", got, full[:, idx])
        torch.cuda.synchronize()
    print(f"[{name} {prec}] cases that differ from the full decode (max abs, relative): {differ}")
    assert not differ, differ
    # (points, frames) per pass as CONFIGS names them: frame chunks alone, (small64) point chunks alone, both
    assert seen == {"tiny": {100: (40, 2), 70: (35, 2)}, "small64": {400: (200, 2), 268: (67, 4), 200: (100, 2)}}[name]


# ---------------------------------------------------------------------------------------------- 4: the oracle
@pytest.mark.parametrize("name", ["tiny", "small64"])
def test_latent_and_decode_match_the_oracle_fp32(name):
    from oracle import ref_forward as oracle
    model, sd, cfg, dm = build(name)
    sample = inputs(name)
    K = dm.tokens
    stages = {}
    with torch.no_grad():
        oracle.forward(sd, {k: v.cpu() for k, v in sample.items()}, frames=dm.frames, stages=stages)
    with precision("fp32"):
        lat = model.encode_motion(sample)
        pts2 = other_points(name)
        got = model.decode_motion(lat, *pts2)
        torch.cuda.synchronize()
    e_lat = rel_err(lat.tokens, stages["trunk_out"][:, :, 4:4 + K])
    # the oracle's decoder lines (ref_forward.forward, stage F) on the GPU's latent and the new points
    tok = lat.tokens.cpu()
    with torch.no_grad():
        pf = oracle.point_features(sd, *(p.cpu() for p in pts2))
        outs = []
        for t in range(tok.shape[1]):
            dec = oracle.cross_attn_block(sd, "decoder_cross_attn", pf, tok[:, t], dm.d_head)
            h = oracle.layer_norm(dec, sd["shared_mlp_output.0.weight"], sd["shared_mlp_output.0.bias"])
            h = oracle.gelu(h @ sd["shared_mlp_output.1.weight"].T + sd["shared_mlp_output.1.bias"])
            outs.append(h @ sd["shared_mlp_output.3.weight"].T + sd["shared_mlp_output.3.bias"])
        want = torch.stack(outs, dim=1)
    e_dec = rel_err(got, want)
    print(f"[{name} fp32] latent vs oracle {e_lat:.2e}  decode of new points vs oracle {e_dec:.2e}")
    assert e_lat < FP32_TOL and e_dec < FP32_TOL


# ---------------------------------------------------------------------------------------------- 5: graph replay
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small64"])
def test_graph_replay_serves_encode_only_and_decode_only(name, prec):
    import motion324_amd as m
    model, sd, cfg, dm = build(name)
    sample = inputs(name)
    pts = [sample[k] for k in POINTS]
    enc_s = dict(clip_only(sample), m324_encode_only=True)
    enc_s2 = dict(enc_s, rgb_video=sample["rgb_video"] * 0.5)
    with precision(prec):
        lat, lat2 = model.encode_motion(sample), model.encode_motion(enc_s2)
        assert not torch.equal(lat.tokens, lat2.tokens)
        eager, eager2 = model.decode_motion(lat, *pts), model.decode_motion(lat2, *pts)
        fast = m.GraphedForward(model)
        # encode-only: no pcd_moved, the latent in a static buffer; new frames with the same shapes are picked up
        r = fast(enc_s)
        assert "pcd_moved" not in r
        same(r.latent, lat.tokens)
        same(fast(enc_s2).latent, lat2.tokens)
        same(fast(enc_s).latent, lat.tokens)
        # decode-only: new latent values with the same shapes are picked up through the static buffers
        dec_s = dict(zip(POINTS, pts), m324_latent=lat.tokens)
        a = fast(dec_s).pcd_moved.clone()
        b = fast(dict(dec_s, m324_latent=lat2.tokens)).pcd_moved.clone()
        c = fast(dec_s).pcd_moved.clone()
        same(a, eager), same(b, eager2), same(c, eager)
        assert len(fast._graphs) == 2
        # the automatic replay: the third plain call with one set of shapes replays, and what a call returned is the caller's own
        model.auto_graph = True
        outs = [model.decode_motion(lat, *pts) for _ in range(3)]
        ag = model.__dict__["_ag"]
        assert len(ag._graphs) == 1
        lats = [model.encode_motion(sample) for _ in range(3)]
        assert len(ag._graphs) == 2
        kept = lats[2].tokens
        model.encode_motion(enc_s2)                                  # a replay of the same graph with other frames
        same(model.decode_motion(lat2, *pts), eager2)
        torch.cuda.synchronize()
    for o in outs:
        same(o, eager)
    for l in lats:
        same(l.tokens, lat.tokens)
    same(kept, lat.tokens)                                           # the returned latent survived the later call
    assert kept.data_ptr() != ag._graphs[next(k for k in ag._graphs if ("m324_encode_only", True) in k)][2]["latent"].data_ptr()


# ---------------------------------------------------------------------------------------------- 6: the long-video driver
def _driver_inputs(T, seed=9, mesh_seed=None, byte_frames=False):
    from motion324_amd import synth
    s = synth.synth_inputs(1, T, 24, 60, 64, seed=seed)
    video = torch.from_numpy(s.pop("rgb_video"))[0]                    # [T, H, W, 3]
    if byte_frames:
        video = (video * 255).round().clamp(0, 255).to(torch.uint8)
    inp = {k: torch.from_numpy(v).cuda() for k, v in s.items()}
    if mesh_seed is not None:                                          # the same shape samples, other vertices
        other = synth.synth_inputs(1, 1, 24, 60, 14, seed=mesh_seed)
        for k in POINTS:
            inp[k] = torch.from_numpy(other[k]).cuda()
    return inp, video


@pytest.mark.parametrize("byte_frames", [False, True])
@pytest.mark.parametrize("pipelined,reuse", [(False, False), (True, False), (True, True)])
def test_driver_returns_the_video_latent_and_decodes_other_meshes(pipelined, reuse, byte_frames):
    """3-frame windows over 8 frames: four windows, the second-to-last rule, the anchor frame (plan_windows).  Trajectories with
    return_latent equal those without; decode_video_latent on the same mesh equals them; on a second mesh it equals a fresh
    driver run on that mesh."""
    from motion324_amd.inference import decode_video_latent, plan_windows, run_model_inference
    T = 8
    windows, out_map = plan_windows(T, 3)
    assert len(windows) == 4 and out_map[0] is None and [w for w, _ in out_map[1:]] == [0, 0, 1, 1, 2, 3, 3]
    model, sd, cfg, dm = build("tiny")
    cfg["training"]["use_amp"] = False
    model.auto_graph = True                                            # the driver's later windows replay
    inp, video = _driver_inputs(T, byte_frames=byte_frames)
    inp2, _ = _driver_inputs(T, mesh_seed=21)
    assert torch.equal(inp["ref_shape_pcd"], inp2["ref_shape_pcd"]) and not torch.equal(inp["ref_pcd"], inp2["ref_pcd"])
    kw = dict(pipelined=pipelined, reuse=reuse)
    plain = run_model_inference(model, inp, video, cfg, "cuda", **kw)
    assert isinstance(plain, torch.Tensor)
    traj, lat = run_model_inference(model, inp, video, cfg, "cuda", return_latent=True, **kw)
    same(traj, plain)
    assert lat.tokens.shape == (1, T, dm.tokens, dm.d) and lat.from_ref == [0] and lat.frames == 3
    same(decode_video_latent(model, lat, inp, cfg, "cuda"), plain)
    fresh = run_model_inference(model, inp2, video, cfg, "cuda", **kw)
    assert not torch.equal(fresh, plain)
    same(decode_video_latent(model, lat, inp2, cfg, "cuda"), fresh)


# ---------------------------------------------------------------------------------------------- 7: precision mix, refusals
def test_latents_cross_precisions():
    model, sd, cfg, dm = build("small64")
    sample = inputs("small64")
    pts = [sample[k] for k in POINTS]
    with precision("bf16"):
        model.inference_precision = "mxfp8"
        assert model.mx_effective()
        lat_mx = model.encode_motion(sample)
        model.inference_precision = "bf16"
        lat_bf = model.encode_motion(sample)
        got_mx = model.decode_motion(lat_mx, *pts)
        got_bf = model.decode_motion(lat_bf, *pts)
        full_bf = model(sample).pcd_moved
        model.inference_precision = "mxfp8"
        full_mx = model(sample).pcd_moved
        model.inference_precision = "bf16"
    assert not torch.equal(lat_mx.tokens, lat_bf.tokens)              # the MXFP8 mode ran on the encode side
    assert torch.isfinite(got_mx).all()
    same(got_mx, full_mx)                                             # the decoder has no MX role: the MXFP8 forward's own result
    same(got_bf, full_bf)
    # a bf16 latent decoded by the fp32 kernels: inside the bf16 band of the fp32 forward (tiny)
    model, sd, cfg, dm = build("tiny")
    sample = inputs("tiny")
    pts = [sample[k] for k in POINTS]
    with precision("bf16"):
        lat = model.encode_motion(sample)
    with precision("fp32"):
        mixed = model.decode_motion(lat, *pts)
        full = model(sample).pcd_moved
    err = rel_err(mixed, full)
    print(f"[tiny] bf16 latent decoded in fp32 vs the fp32 forward {err:.2e}")
    assert err < BF16_TOL


def test_refusals():
    import motion324_amd as m
    from motion324_amd.lib import M324Error
    model, sd, cfg, dm = build("tiny")
    sample = inputs("tiny")
    pts = [sample[k] for k in POINTS]
    with precision("fp32"):
        lat = model.encode_motion(sample)
    with pytest.raises(M324Error):                                    # grad enabled
        model.encode_motion(sample)
    with pytest.raises(M324Error):
        model.decode_motion(lat, *pts)
    with torch.no_grad():
        model.train()
        try:
            with pytest.raises(M324Error):                            # training mode
                model.encode_motion(sample)
            with pytest.raises(M324Error):
                model.decode_motion(lat, *pts)
        finally:
            model.eval()
        for key in (dict(m324_keep_latent=True), dict(m324_encode_only=True), dict(m324_latent=lat.tokens)):
            with pytest.raises(M324Error):                            # frame-parallel forward
                model.forward_frame_parallel(dict(sample, **key))
        with pytest.raises(M324Error):                                # CPU tensors
            model.encode_motion({k: v.cpu() for k, v in sample.items()})
        with pytest.raises(M324Error):
            model.decode_motion(lat.to("cpu"), *pts)
        with pytest.raises(M324Error):
            model.decode_motion(lat, *(p.cpu() for p in pts))
        wrong = m.MotionLatent(torch.zeros((2, 3, dm.tokens, 2 * dm.d), device="cuda"), d=2 * dm.d, K=dm.tokens, frames=3)
        with pytest.raises(M324Error):                                # sizes of another model
            model.decode_motion(wrong, *pts)
        with pytest.raises(M324Error):
            model(dict(zip(POINTS, pts), m324_latent=wrong.tokens))
        with pytest.raises(M324Error):                                # batch of 2 in the latent, one mesh
            model.decode_motion(lat, *(p[:1] for p in pts))
        with pytest.raises(M324Error):
            model.decode_motion(lat, *pts, frames=[3])
        # and the model still serves a correct call afterwards
        same(model.decode_motion(lat, *pts), model(sample).pcd_moved)
