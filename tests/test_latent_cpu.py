"""Host side of the motion latent API: the MotionLatent file format, the latent merge of the long-video driver against the window
plan, the graph key of the new sample keys, and the world-2 gather of the windows' latents (gloo)."""
import json
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN


def test_motion_latent_save_load_round_trip(tmp_path):
    from motion324_amd import MotionLatent
    g = torch.Generator().manual_seed(3)
    lat = MotionLatent(torch.randn((2, 5, 8, 12), generator=g), d=12, K=8, frames=3, from_ref=[0, 4])
    path = str(tmp_path / "clip.latent.pt")
    lat.save(path)
    blob = torch.load(path, weights_only=True)                     # a plain dict of tensors and ints, like a checkpoint
    assert isinstance(blob, dict) and all(isinstance(v, (torch.Tensor, int)) for v in blob.values())
    back = MotionLatent.load(path)
    assert torch.equal(back.tokens, lat.tokens) and back.tokens.dtype == torch.float32
    assert (back.d, back.K, back.frames, back.from_ref) == (12, 8, 3, [0, 4])
    assert back.tokens.data_ptr() != lat.tokens.data_ptr()
    with pytest.raises(ValueError):
        MotionLatent(torch.zeros((1, 2, 8, 11)), d=12, K=8, frames=3)
    torch.save({"model": {}}, path)
    with pytest.raises(ValueError):
        MotionLatent.load(path)


def test_latent_merge_follows_the_window_plan():
    """merge_latents against plan_windows read slot by slot, for every golden (T, C) pair: frame t's tokens are the tokens of the
    video frame the reference driver's golden map names, and from_ref is exactly the map's ref_pcd slots."""
    from motion324_amd.inference import merge_latents, plan_windows
    gold = json.load(open(os.path.join(GOLDEN, "chunks.json")))
    assert len(gold) >= 50
    for key, expect in gold.items():
        T, C = map(int, key.split(","))
        windows, out_map = plan_windows(T, C)
        # window w, slot s carries the index of its video frame in every token element
        lats = torch.tensor([[float(f) for f in w] for w in windows]).reshape(len(windows), -1, 1, 1) + torch.zeros((1, 1, 2, 3))
        tokens, from_ref = merge_latents(lats.contiguous(), out_map)
        assert tokens.shape == (1, len(out_map), 2, 3)
        assert from_ref == [t for t, s in enumerate(out_map) if s is None] == [t for t, e in enumerate(expect) if e == -1]
        for t, e in enumerate(expect):
            if e != -1:
                assert torch.equal(tokens[0, t], torch.full((2, 3), float(e))), (key, t)


def test_shape_key_tells_the_latent_keys_apart_and_needs_no_video():
    from motion324_amd.graph import _FLAGS, _KEYS, shape_key
    assert "m324_latent" in _KEYS and "m324_keep_latent" in _FLAGS and "m324_encode_only" in _FLAGS
    pts = {"ref_pcd": torch.zeros((1, 16, 3)), "ref_normal": torch.zeros((1, 16, 3)), "ref_rgb": torch.zeros((1, 16, 3))}
    dec = dict(pts, m324_latent=torch.zeros((1, 4, 8, 12)))
    k = shape_key(dec)                                              # no rgb_video in a decode-only sample
    assert k == shape_key({a: b.clone() for a, b in dec.items()})
    assert shape_key(dict(pts, m324_latent=torch.zeros((1, 3, 8, 12)))) != k
    assert shape_key(dict(dec, ref_pcd=torch.zeros((1, 17, 3)))) != k
    base = {"rgb_video": torch.zeros((1, 4, 8, 8, 3)), "ref_shape_pcd": torch.zeros((1, 16, 3))}
    keys = [shape_key(base), shape_key(dict(base, m324_keep_latent=True)), shape_key(dict(base, m324_encode_only=True)),
            shape_key(dict(base, m324_keep_reuse=True)), shape_key(dict(base, rgb_video=torch.zeros((1, 4, 8, 8, 3), dtype=torch.uint8)))]
    assert len(set(keys)) == len(keys)
    assert shape_key(dict(base, m324_keep_latent=False)) == keys[0]


class _StubModel:
    """Output frame t = ref_pcd + mean of input frame t; its latent [1, T, 2, 3] holds that mean."""

    def __call__(self, sample):
        mean = sample["rgb_video"].mean(dim=(2, 3, 4))
        out = {"pcd_moved": sample["ref_pcd"][:, None] + mean[:, :, None, None]}
        if sample.get("m324_keep_latent", False):
            out["latent"] = mean[:, :, None, None].expand(1, mean.shape[1], 2, 3).contiguous()
        return out


def _video(T):
    return torch.arange(T, dtype=torch.float32).view(T, 1, 1, 1).expand(T, 4, 4, 3).contiguous() / 10


def _run(T, C, **kw):
    from motion324_amd.inference import run_model_inference
    inp = {"ref_pcd": torch.linspace(-1, 1, 15).view(1, 5, 3)}
    cfg = {"training": {"frames": C, "use_amp": False}}
    return run_model_inference(_StubModel(), inp, _video(T), cfg, "cpu", **kw)


def _worker(rank, world, port, T, C, ret):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        traj, lat = _run(T, C, return_latent=True)
        ret[rank] = (traj, lat.tokens, lat.from_ref, (lat.d, lat.K, lat.frames))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("T,C", [(30, 12), (8, 3)])
def test_latents_world2_gloo_are_gathered_in_frame_order(T, C):
    plain = _run(T, C)
    traj, lat = _run(T, C, return_latent=True)
    assert torch.equal(traj, plain)                                 # the default call returns what it returned
    assert lat.tokens.shape == (1, T, 2, 3) and (lat.d, lat.K, lat.frames) == (3, 2, C)
    assert lat.from_ref == [0]
    want = (torch.arange(T, dtype=torch.float32) / 10).view(1, T, 1, 1).expand(1, T, 2, 3)
    assert torch.allclose(lat.tokens[:, 1:], want[:, 1:], atol=1e-6)          # frame t's tokens came from video frame t
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 33500 + (os.getpid() + T) % 2000
    mp.spawn(_worker, args=(2, port, T, C, ret), nprocs=2, join=True)
    for r in range(2):
        assert torch.equal(ret[r][0], plain) and torch.equal(ret[r][1], lat.tokens)
        assert ret[r][2] == lat.from_ref and ret[r][3] == (3, 2, C)


def test_decode_plan_keeps_every_pass_on_the_whole_decodes_side_of_the_64_row_line():
    """The bf16 kernels change path at 64 rows.  Whatever the budget, a decode-only plan's passes hold more than 64 rows if the
    whole decode does, its point chunks more than 64 points if the mesh does, its frame chunks are even, and a budget of at
    least 130 rows is kept."""
    from motion324_amd.Pcd_motion import decode_plan
    assert decode_plan(40, 3, 100) == (40, 2) and decode_plan(40, 3, 70) == (35, 2)
    assert decode_plan(200, 4, 400) == (200, 2) and decode_plan(200, 4, 268) == (67, 4) and decode_plan(200, 4, 200) == (100, 2)
    assert decode_plan(2048, 32, 1 << 17) == (2048, 32) and decode_plan(1 << 18, 32, 1 << 17) == (4096, 32)
    for N in (1, 7, 23, 32, 33, 40, 64, 65, 77, 200, 1000):
        for T in (1, 2, 3, 4, 9, 32):
            for rows in (1, 16, 48, 64, 65, 70, 100, 129, 130, 200, 268, 400, 4096):
                n, t = decode_plan(N, T, rows)
                assert 1 <= n <= N and 1 <= t <= T, (N, T, rows)
                assert t == T or t % 2 == 0, (N, T, rows)
                assert (n > 64) == (N > 64) or n == N, (N, T, rows)
                assert (n * t > 64) == (N * T > 64), (N, T, rows)
                if rows >= 130 or N * T <= rows:
                    assert n * t <= max(rows, 1) or (n, t) == (N, T) and N * T <= rows, (N, T, rows)
