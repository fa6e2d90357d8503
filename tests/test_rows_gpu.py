"""The trunk's last per-frame block on the rows its readers read (M324_LAST_BLOCK_ROWS): m324_attention_rows (query window),
m324_gemm_rows (row-gathered A and residual) and the model path built from them.

Everything here is an equality, not a tolerance: the window keeps the full launch's 32-row blocks (the lazy softmax maximum moves
on a vote of such a block), a GEMM row does not depend on its neighbours, and the LayerNorm statistics are merged the same way by
every schedule.  The attention inputs are scaled so that the vote does move; the test asserts that from an fp32 reference."""
import ctypes

import pytest
import torch

from test_latent_gpu import POINTS, build, clip_only, inputs, precision, same

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
SENTINEL = 0x5A5A          # bf16 bit pattern of rows nobody may write


def _votes(Q, K, q_rows):
    """Emulates the kernel's lazy reference maximum on fp32 scores: (tile, 32-row block) pairs below q_rows in which some row's score
    exceeds its reference by more than the threshold 8 (with a margin for the fp32 / MFMA summation order), and how many of those
    blocks also hold a row that stays calm -- the rows whose rounding the vote changes."""
    S = Q.float() @ K.float().transpose(-1, -2)                       # [B, H, Lq, Lk], log2 domain (pre-scaled q)
    B, H, Lq, Lk = S.shape
    moved = mixed = 0
    for q0 in range(0, min(q_rows, Lq), 32):
        blk = S[:, :, q0:q0 + 32]
        m = blk[..., :64].max(-1).values
        for k0 in range(64, Lk, 64):
            mx = blk[..., k0:k0 + 64].max(-1).values
            hot = (mx - m) > 8.05
            vote = hot.any(-1)                                        # per (b, h): the wave-uniform decision
            moved += int(vote.sum())
            mixed += int((vote & ~((mx - m) > 7.95).all(-1)).sum())
            m = torch.where(vote[..., None], m + (mx - m).clamp_min(0), m)
    return moved, mixed


def _attn_operands(Lq, seed):
    g = torch.Generator().manual_seed(seed)
    B, H = 2, 2
    Q = (torch.randn((B, H, Lq, 64), generator=g) * 0.75).to(torch.bfloat16).cuda()        # scores ~ N(0, 6^2): a few 8 above the first tile's maximum
    K = torch.randn((B, H, Lq, 64), generator=g).to(torch.bfloat16).cuda()
    V = torch.randn((B, H, Lq, 64), generator=g).to(torch.bfloat16).cuda()
    return Q, K, V


@pytest.mark.parametrize("Lq,q_rows", [(324, 96), (257, 32), (160, 128), (324, 324)])
def test_attention_window_equals_the_full_launch_bit_for_bit(Lq, q_rows):
    from motion324_amd import ops
    B, H = 2, 2
    Q, K, V = _attn_operands(Lq, seed=Lq + q_rows)
    moved, mixed = _votes(Q, K, q_rows)
    print(f"Lq={Lq} q_rows={q_rows}: reference moved in {moved} (block, tile) pairs, {mixed} of them with calm rows")
    assert moved > 0 and mixed > 0, "the inputs do not exercise the vote path"
    full = torch.empty((B * Lq, H * 64), dtype=torch.bfloat16, device="cuda")
    ops.attention(Q, K, V, full, prescaled=True, v_rowmajor=True)
    win = torch.full((B * Lq, H * 64), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    ops.attention(Q, K, V, win, prescaled=True, v_rowmajor=True, q_rows=q_rows)
    torch.cuda.synchronize()
    f, w = full.view(torch.int16).view(B, Lq, H * 64), win.view(torch.int16).view(B, Lq, H * 64)
    assert torch.isfinite(full.float()).all()
    assert torch.equal(w[:, :q_rows], f[:, :q_rows])
    assert bool((w[:, q_rows:] == SENTINEL).all())


def test_attention_window_refuses_what_is_not_built():
    from motion324_amd import lib
    h = lib.load()
    s = torch.cuda.current_stream().cuda_stream

    def call(Q, K, V, out, Lq, Lk, flags, dtype, q_rows):
        B, H = K.shape[0], K.shape[1]
        return h.m324_attention_rows(Q.data_ptr(), H * Lq * 64, K.data_ptr(), V.data_ptr(), out.data_ptr(), H * 64, B, H, Lq, Lk, 0.125,
                                     flags, None, dtype, q_rows, s)
    Q, K, V = _attn_operands(160, seed=3)
    out = torch.full((2 * 160, 128), SENTINEL, dtype=torch.int16, device="cuda")
    assert call(Q, K, V, out, 160, 160, 3, lib.BF16, 48) == UNSUPPORTED and "32" in lib.last_error()       # not whole 32-row blocks
    # long sequences run the hand-placed stream, which takes no window
    Ql = torch.zeros((1, 1, 2048, 64), dtype=torch.bfloat16, device="cuda")
    Kl = torch.zeros((1, 1, 512, 64), dtype=torch.bfloat16, device="cuda")
    Vl = torch.zeros((1, 1, 64, 512), dtype=torch.bfloat16, device="cuda")
    outl = torch.full((2048, 64), SENTINEL, dtype=torch.int16, device="cuda")
    assert call(Ql, Kl, Vl, outl, 2048, 512, 1, lib.BF16, 96) == UNSUPPORTED
    # the fp32 kernel
    Qf, Kf = (torch.zeros((1, 1, 160, 64), dtype=torch.float32, device="cuda") for _ in range(2))
    Vf = torch.zeros((1, 1, 64, 192), dtype=torch.float32, device="cuda")
    outf = torch.full((160, 64), 7.0, dtype=torch.float32, device="cuda")
    assert call(Qf, Kf, Vf, outf, 160, 160, 1, lib.F32, 96) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((outl == SENTINEL).all()) and bool((outf == 7.0).all())      # nothing was launched


@pytest.mark.parametrize("N", [768, 256])
def test_gathered_gemm_equals_the_gemm_on_gathered_copies(N):
    """3 frames of 100 rows, map (64, 100, 4): 192 rows (two row tiles, the second half full).  Every source row outside the map is
    NaN, in A and in the residual: a read of an unmapped row poisons the result."""
    from motion324_amd import ops
    g = torch.Generator().manual_seed(N)
    F, L, n_per, first, K = 3, 100, 64, 4, 768
    M = F * n_per
    idx = (torch.arange(F)[:, None] * L + first + torch.arange(n_per)[None]).reshape(-1)
    A = torch.full((F * L, K), float("nan"))
    R = torch.full((F * L, N), float("nan"))
    A[idx] = torch.randn((M, K), generator=g)
    R[idx] = torch.randn((M, N), generator=g) * 3.0
    A, R = A.to(torch.bfloat16).cuda(), R.cuda()
    W = (torch.randn((N, K), generator=g) * 0.05).to(torch.bfloat16).cuda()
    bias = torch.randn((N,), generator=g).cuda()

    def outs():
        return (torch.zeros((M, N), dtype=torch.float32, device="cuda"), torch.zeros((N // 64, M, 2), dtype=torch.float32, device="cuda"),
                torch.zeros((M, N), dtype=torch.bfloat16, device="cuda"))
    x0, st0, tw0 = outs()
    ops.gemm(A[idx.cuda()].contiguous(), W, x0, bias=bias, residual=R[idx.cuda()].contiguous(), stats_out=st0, copy_out=tw0)
    x1, st1, tw1 = outs()
    ops.gemm(A, W, x1, bias=bias, residual=R, stats_out=st1, copy_out=tw1, in_rows=(n_per, L, first))
    torch.cuda.synchronize()
    assert torch.isfinite(x0).all() and torch.isfinite(st0).all()
    assert torch.equal(x1, x0)
    assert torch.equal(st1, st0)
    assert torch.equal(tw1.view(torch.int16), tw0.view(torch.int16))


def test_gathered_gemm_refuses_what_is_not_built():
    from motion324_amd import ops
    from motion324_amd.lib import M324Error
    A = torch.zeros((300, 768), dtype=torch.bfloat16, device="cuda")
    W = torch.zeros((768, 768), dtype=torch.bfloat16, device="cuda")
    R = torch.zeros((300, 768), dtype=torch.float32, device="cuda")
    x = torch.full((192, 768), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(M324Error, match=r"m324_gemm_rows failed \(-3\)"):
        ops.gemm(A, W, x, residual=R, in_rows=(64, 100, 4))                       # no statistics / twin: a plain residual update
    xb = torch.zeros((192, 768), dtype=torch.bfloat16, device="cuda")
    st = torch.zeros((12, 192, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(M324Error, match=r"m324_gemm_rows failed \(-3\)"):
        ops.gemm(A, W, xb, residual=R, stats_out=st, in_rows=(64, 100, 4))        # bf16 stream
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ the model
def _load(model, sd_np):
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert set(missing) <= {"pos_embed", "point_embed.basis"} and not unexpected


class _Record:
    """Wraps ops.gemm / ops.attention: the launches a forward issues, as (kind, shape, the new keyword or None)."""

    def __init__(self, monkeypatch):
        from motion324_amd import ops
        self.calls, self.window = [], None
        g, a = ops.gemm, ops.attention

        def gemm(x, w, out, **kw):
            self.calls.append(("gemm", tuple(x.shape), tuple(w.shape), None if out is None else tuple(out.shape), kw.get("in_rows")))
            return g(x, w, out, **kw)

        def attention(Q, K, V, out, **kw):
            self.calls.append(("attention", tuple(Q.shape), tuple(K.shape), tuple(out.shape), kw.get("q_rows")))
            if kw.get("q_rows") is not None:
                self.window = (Q.clone(), K.clone(), kw["q_rows"])
            return a(Q, K, V, out, **kw)
        monkeypatch.setattr(ops, "gemm", gemm)
        monkeypatch.setattr(ops, "attention", attention)

    def take(self):
        c, self.calls = self.calls, []
        return c


@pytest.mark.parametrize("weights", ["synthetic", "trained_like"])
def test_model_results_do_not_depend_on_the_switch(weights, monkeypatch):
    """small64 (d 384, two trunk blocks per kind, 4 frames of 324 tokens, 64 latent tokens): pcd_moved, the motion latent and graph
    replays with M324_LAST_BLOCK_ROWS on and off, bit for bit.  trained_like: grown q / k norms, the per-frame blocks' once more
    (x 2), so that the windowed attention's vote moves -- asserted on the operands the model hands to it."""
    import motion324_amd as m
    import motion324_amd.Pcd_motion as pm
    model, sd, cfg, dm = build("small64")
    if weights == "trained_like":
        from test_trained_like_gpu import trained_like
        from conftest import synth_sd
        from test_latent_gpu import CONFIGS
        sd_np = trained_like(synth_sd(dict(CONFIGS["small64"]["dims"])))
        for k in sd_np:
            if k.startswith("local_transformer_blocks.") and (k.endswith("q_norm.weight") or k.endswith("k_norm.weight")):
                sd_np[k] = sd_np[k] * 2.0
        _load(model, sd_np)
    sample = inputs("small64")
    res = {}
    for on in (False, True):
        monkeypatch.setattr(pm, "LAST_BLOCK_ROWS", on)
        with precision("bf16"):
            out = model(dict(sample, m324_keep_latent=True))
            lat = model.encode_motion(clip_only(sample)).tokens
            fast = m.GraphedForward(model)
            rep = [fast(sample).pcd_moved.clone() for _ in range(2)]
            torch.cuda.synchronize()
        res[on] = (out.pcd_moved, out.latent, lat, rep[0], rep[1])
    assert torch.isfinite(res[True][0]).all()
    for a, b in zip(res[True], res[False]):
        same(a, b)
    same(res[True][3], res[True][0])
    # the new path did run, once per forward, on the window the issue names
    monkeypatch.setattr(pm, "LAST_BLOCK_ROWS", True)
    rec = _Record(monkeypatch)
    with precision("bf16"):
        model(sample)
        torch.cuda.synchronize()
    calls = rec.take()
    assert [c[4] for c in calls if c[0] == "attention" and c[4] is not None] == [96]
    assert [c[4] for c in calls if c[0] == "gemm" and c[4] is not None] == [(64, 324, 4)]
    if weights == "trained_like":
        Q, K, q_rows = rec.window
        moved, mixed = _votes(Q, K, q_rows)
        print(f"trained-like weights: the last per-frame block's reference moved in {moved} (block, tile) pairs, {mixed} with calm rows")
        assert moved > 0 and mixed > 0


def test_captures_and_fp32_keep_the_whole_stream(monkeypatch):
    """A forward with _capture set and a forward in fp32 mode issue the launches they issue with the switch off."""
    import motion324_amd.Pcd_motion as pm
    model, sd, cfg, dm = build("small64")
    sample = inputs("small64")
    rec = _Record(monkeypatch)

    def launches(prec, capture):
        model._capture = {} if capture else None
        try:
            with precision(prec):
                out = model(sample).pcd_moved
                torch.cuda.synchronize()
        finally:
            model._capture = None
        return rec.take(), out
    for prec, capture in (("bf16", True), ("fp32", False)):
        monkeypatch.setattr(pm, "LAST_BLOCK_ROWS", False)
        off, out_off = launches(prec, capture)
        monkeypatch.setattr(pm, "LAST_BLOCK_ROWS", True)
        on, out_on = launches(prec, capture)
        assert on == off and all(c[4] is None for c in on)
        same(out_on, out_off)
