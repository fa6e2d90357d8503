#!/usr/bin/env python3
"""Timing of the video framing (motion324_amd.framing.frame_video, csrc/framing.hip); the numbers live in
profiles/video_framing.md.

A synthetic matted clip (default 256 frames of 1920 x 1080 RGBA: noise colours, an elliptic foreground that drifts, alpha 255
inside and 0..204 outside) is framed to 512 x 512
  * device-resident: the clip is on the GPU already; device events and a host clock around a call that ends in a synchronise;
  * host-resident: the same call on the host array, upload included; host clock;
  * by the host loop of the same work, frame by frame: PIL (threshold, bounding box, crop, LANCZOS resize, paste) where PIL is
    importable, else the numpy model of tests/framing_cases.py; on `--host-frames` frames, reported per frame.
Each kernel stage is timed on its own between device events as well, and set against the bytes it has to move and the copy
bandwidth of the same box (a device-to-device copy of 1 GiB, timed the same way).  Before any time is reported the GPU result
of the host loop's frames is compared with the host loop's, bit for bit.

    python tools/framing_time.py [--frames 256] [--height 1080] [--width 1920] [--out FILE.md]

A run without a HIP device fails: there is no CPU timing of the GPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def synthetic_clip(T, H, W, seed=0):
    """uint8 [T,H,W,4]: two noise frames rolled along x per frame (cheap to make, nothing a resampler could exploit), an ellipse
    of opaque foreground whose centre drifts; alpha 0..204 elsewhere"""
    import numpy as np
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(2, H, W, 4), dtype=np.uint8)
    base[..., 3] = rng.integers(0, 205, size=(2, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    clip = np.empty((T, H, W, 4), dtype=np.uint8)
    for t in range(T):
        clip[t] = np.roll(base[t % 2], 7 * t, axis=1)
        cx, cy = W * (0.45 + 0.1 * t / max(T - 1, 1)), H * (0.52 - 0.04 * t / max(T - 1, 1))
        inside = ((xx - cx) / (0.16 * W)) ** 2 + ((yy - cy) / (0.42 * H)) ** 2 <= 1.0
        clip[t, ..., 3][inside] = 255
    return clip


def host_loop(clip, size=512):
    """the reference's loop on the host: per frame threshold + box, then per frame crop, LANCZOS resize and paste.  Returns
    (frames, masks, seconds, what ran)"""
    import numpy as np
    t0 = time.perf_counter()
    try:
        import PIL
        from PIL import Image
    except ImportError:
        import framing_cases as fc
        out = fc.model_frame(np.ascontiguousarray(clip[..., :3]), np.ascontiguousarray(clip[..., 3]), size)
        return out["frames"], out["mask"], time.perf_counter() - t0, "numpy model"
    box, items = None, []
    for frame in clip:
        keep = frame[..., 3] > 204
        mask = keep.astype(np.uint8) * 255
        rgb = frame[..., :3] * keep[..., None]
        ys, xs = np.nonzero(keep)
        if len(xs):
            b = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
            box = b if box is None else (min(box[0], b[0]), min(box[1], b[1]), max(box[2], b[2]), max(box[3], b[3]))
        items.append((Image.fromarray(rgb), Image.fromarray(mask)))
    w, h = box[2] - box[0], box[3] - box[1]
    s = size / max(w, h)
    new_w, new_h = max(1, int(round(w * s))), max(1, int(round(h * s)))
    frames, masks = [], []
    for rgb, mask in items:
        for img, fill, dst in ((rgb, (0, 0, 0), frames), (mask, 0, masks)):
            canvas = Image.new(img.mode, (size, size), fill)
            canvas.paste(img.crop(box).resize((new_w, new_h), Image.Resampling.LANCZOS), ((size - new_w) // 2, (size - new_h) // 2))
            dst.append(np.asarray(canvas))
    return np.stack(frames), np.stack(masks), time.perf_counter() - t0, "PIL " + PIL.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--host-frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from motion324_amd import framing, ops
    if not torch.cuda.is_available():
        sys.exit("framing_time: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda:0")
    T, H, W = args.frames, args.height, args.width
    clip = synthetic_clip(T, H, W)
    resident = torch.from_numpy(clip).to(dev)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def events(fn, rounds=args.rounds):
        """median, min, max in ms of fn() between device events, after one warm-up call"""
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    def wall(fn, rounds):
        fn()
        torch.cuda.synchronize()
        s = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            s.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(s), min(s), max(s)

    # results before speed: the frames the host loop does, against the GPU's, bit for bit
    n_host = min(args.host_frames, T)
    h_frames, h_masks, h_seconds, h_what = host_loop(clip[:n_host])
    out = framing.frame_video(resident[:n_host])
    equal = bool(torch.equal(out.frames.cpu(), torch.from_numpy(h_frames)) and torch.equal(out.mask.cpu(), torch.from_numpy(h_masks)))
    emit(dict(case="check", frames=n_host, host=h_what, equal=equal, box=out.box, placement=out.placement))
    if not equal:
        sys.exit("framing_time: the GPU result differs from the host loop's; no time is reported")
    emit(dict(case="host_loop", what=h_what, frames=n_host, ms_per_frame=h_seconds * 1e3 / n_host))
    del out

    whole = framing.frame_video(resident)
    box, (new_w, new_h, off_x, off_y) = whole.box, whole.placement
    del whole
    emit(dict(case="clip", frames=T, height=H, width=W, box=box, placement=(new_w, new_h, off_x, off_y)))
    ev = events(lambda: framing.frame_video(resident))
    wl = wall(lambda: framing.frame_video(resident), args.rounds)
    emit(dict(case="device_resident", events_ms=ev, wall_ms=wl, ms_per_frame=ev[0] / T, wall_ms_per_frame=wl[0] / T))
    wl_host = wall(lambda: framing.frame_video(clip, device=dev), max(2, args.rounds // 2))
    emit(dict(case="host_resident", wall_ms=wl_host, wall_ms_per_frame=wl_host[0] / T, upload_bytes=int(clip.nbytes)))

    # the stages on their own, with the bytes each has to move (reads + writes; tables and boxes are negligible)
    left, top, right, bottom = box
    w, h = right - left, bottom - top
    rgb, alpha = resident[..., :3], resident[..., 3]
    tabs = {axis: tuple(torch.from_numpy(t).to(dev) for t in framing.resample_tables(n_in, n_out)) for axis, n_in, n_out in (("x", w, new_w), ("y", h, new_h))}
    order = framing.pass_order(w, h, new_h)
    frames = torch.empty((T, 512, 512, 3), dtype=torch.uint8, device=dev)
    mask = torch.empty((T, 512, 512), dtype=torch.uint8, device=dev)
    first = dict(axis=order[0], crop=(left, top, w, h), alpha=alpha, threshold=204)
    mid_rgb = ops.frame_resample(rgb, *tabs[order[0]], channels=3, mode="threshold", **first)
    mid_mask = ops.frame_resample(alpha, *tabs[order[0]], channels=1, mode="binary", **first)
    mid_px = mid_rgb.shape[1] * mid_rgb.shape[2]
    stages = [
        ("frame_mask (boxes only)", lambda: ops.frame_mask(rgb, alpha, want_masked=False, want_mask=False), H * W * 4),
        ("first pass, colour", lambda: ops.frame_resample(rgb, *tabs[order[0]], channels=3, mode="threshold", **first), w * h * 4 + mid_px * 3),
        ("second pass, colour", lambda: ops.frame_resample(mid_rgb, *tabs[order[1]], order[1], channels=3, out=frames, paste=(off_x, off_y), fill=0),
         mid_px * 3 + 512 * 512 * 3),
        ("first pass, mask", lambda: ops.frame_resample(alpha, *tabs[order[0]], channels=1, mode="binary", **first), w * h + mid_px),
        ("second pass, mask", lambda: ops.frame_resample(mid_mask, *tabs[order[1]], order[1], channels=1, out=mask, paste=(off_x, off_y), fill=0),
         mid_px + 512 * 512),
    ]
    gib = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    gib2 = torch.empty_like(gib)
    copy_ms = events(lambda: gib2.copy_(gib))
    copy_rate = 2 * (1 << 30) / (copy_ms[0] * 1e-3)                     # bytes read + bytes written per second
    del gib, gib2
    emit(dict(case="copy_1GiB", events_ms=copy_ms, bytes_per_s=copy_rate))
    for name, fn, bytes_per_frame in stages:
        ms = events(fn)
        emit(dict(case="stage", stage=name, events_ms=ms, us_per_frame=ms[0] * 1e3 / T, bytes_per_frame=bytes_per_frame,
                  bytes_per_s=bytes_per_frame * T / (ms[0] * 1e-3), share_of_copy_rate=bytes_per_frame * T / (ms[0] * 1e-3) / copy_rate))

    if args.out:
        prop = torch.cuda.get_device_properties(0)
        arch = getattr(prop, "gcnArchName", "").split(":")[0]
        box_class = f"{'MI355X-class ' if arch == 'gfx950' else ''}GPU ({prop.name}, {arch}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB)"
        by = {r["case"]: r for r in records if r["case"] != "stage"}
        lines = ["# Video framing: what was measured", "",
                 f"`tools/framing_time.py` on one {box_class}, one process, one run.  Synthetic clip of {T} frames of {W} x {H} RGBA; "
                 f"union box {box} (crop {w} x {h}), resized to {new_w} x {new_h}, pass order `{order}`.  Device events around the calls, one "
                 f"warm-up, median of {args.rounds} rounds with (min .. max); the host clock ends in a device synchronise.  Before timing, the "
                 f"GPU result of the first {n_host} frames was compared with the host loop's ({h_what}): bit-identical.", "",
                 "| | ms per clip | ms per frame |", "|---|---|---|"]
        d, hr, hl = by["device_resident"], by["host_resident"], by["host_loop"]
        fmt = lambda m: f"{m[0]:.2f} ({m[1]:.2f} .. {m[2]:.2f})"       # noqa: E731
        lines += [f"| `frame_video`, device-resident clip, device events | {fmt(d['events_ms'])} | {d['ms_per_frame']:.4f} |",
                  f"| `frame_video`, device-resident clip, host clock | {fmt(d['wall_ms'])} | {d['wall_ms_per_frame']:.4f} |",
                  f"| `frame_video`, host-resident clip (upload of {clip.nbytes / 2 ** 20:.0f} MiB included), host clock | {fmt(hr['wall_ms'])} | "
                  f"{hr['wall_ms_per_frame']:.4f} |",
                  f"| host loop ({hl['what']}), {hl['frames']} frames, host clock | | {hl['ms_per_frame']:.2f} |", "",
                  f"Per frame the host loop takes {hl['ms_per_frame'] / d['wall_ms_per_frame']:.0f}x the device-resident call and "
                  f"{hl['ms_per_frame'] / hr['wall_ms_per_frame']:.1f}x the host-resident one (host clock on both sides).", "",
                  "## Stages", "",
                  f"Bytes are what a stage must read and write per frame; the copy rate of this box is {copy_rate / 1e12:.2f} TB/s (a device-to-device "
                  f"copy of 1 GiB, reads + writes, {fmt(by['copy_1GiB']['events_ms'])} ms).", "",
                  "| stage | ms per clip | us per frame | MB per frame | GB/s | share of the copy rate |", "|---|---|---|---|---|---|"]
        for r in records:
            if r["case"] == "stage":
                lines.append(f"| {r['stage']} | {fmt(r['events_ms'])} | {r['us_per_frame']:.1f} | {r['bytes_per_frame'] / 1e6:.2f} | "
                             f"{r['bytes_per_s'] / 1e9:.0f} | {100 * r['share_of_copy_rate']:.1f} % |")
        lines += ["", "No fused single-kernel variant was built; there is no A/B of one here.", ""]
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
