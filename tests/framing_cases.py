"""Video framing: the case list (seeded synthetic RGBA clips) and a numpy model of the whole pipeline -- masking, per-frame
boxes, union box, placement, the two 8-bit Lanczos passes, paste on the canvas -- with its loops written out.  The model
shares no code with motion324_amd/framing.py: it builds its own coefficient tables, so a wrong product table cannot hide
behind a model that copies it.  tests/golden/framing.npz pins the model to the reference's own output files."""
import hashlib
import math

import numpy as np

SIZE = 512

# name -> T, H, W, fg: per frame the foreground rectangle (left, top, right, bottom; right / bottom open) or None for a frame
# without foreground; layout: how the GPU tests hand the clip over.  `box` and `place` are what the case is built to give.
CASES = {
    # H = 37, W = 53, RGB + alpha: row pitch 159 bytes (no row but the first starts on a 16-byte boundary); support 3, ksize 7
    "upscale": dict(T=2, H=37, W=53, fg=[(5, 4, 41, 30), (6, 4, 41, 29)], layout="rgb+alpha", box=(5, 4, 41, 30)),
    "down_wide": dict(T=2, H=40, W=700, fg=[(10, 3, 690, 37), (12, 5, 650, 30)], layout="rgba", box=(10, 3, 690, 37)),
    "down_tall": dict(T=2, H=600, W=45, fg=[(4, 20, 40, 580), (6, 25, 41, 590)], layout="rgba", box=(4, 20, 41, 590)),
    "long_kernel": dict(T=1, H=8, W=2100, fg=[(0, 0, 2100, 8)], layout="rgba", box=(0, 0, 2100, 8), ksize_x=27),
    "edges": dict(T=2, H=64, W=80, fg=[(0, 0, 80, 64), (0, 0, 80, 64)], layout="rgb+alpha", box=(0, 0, 80, 64)),
    "interior": dict(T=2, H=90, W=120, fg=[(17, 11, 95, 70), (20, 15, 90, 66)], layout="rgba", box=(17, 11, 95, 70)),
    "side512": dict(T=1, H=64, W=520, fg=[(4, 10, 516, 50)], layout="rgba", box=(4, 10, 516, 50), place=(512, 40, 0, 236)),
    "one_pixel": dict(T=1, H=20, W=20, fg=[(7, 9, 8, 10)], layout="rgba", box=(7, 9, 8, 10), place=(512, 512, 0, 0)),
    "thin": dict(T=1, H=110, W=20, fg=[(9, 5, 10, 105)], layout="rgb+alpha", box=(9, 5, 10, 105), place=(5, 512, 253, 0)),
    "half5": dict(T=1, H=1024, W=8, fg=[(2, 0, 7, 1024)], layout="rgba", box=(2, 0, 7, 1024), place=(2, 512, 255, 0)),
    "half7": dict(T=1, H=1024, W=8, fg=[(1, 0, 8, 1024)], layout="rgba", box=(1, 0, 8, 1024), place=(4, 512, 254, 0)),
    "odd_space": dict(T=1, H=120, W=60, fg=[(10, 8, 43, 108)], layout="rgba", box=(10, 8, 43, 108), place=(169, 512, 171, 0)),
    # T = 4: each of the four extremes comes from a frame of its own
    "union": dict(T=4, H=70, W=96, fg=[(30, 5, 50, 40), (8, 25, 40, 35), (35, 20, 90, 45), (40, 30, 60, 61)], layout="rgba", box=(8, 5, 90, 61)),
    "empty_middle": dict(T=3, H=48, W=66, fg=[(10, 8, 50, 40), None, (12, 6, 55, 38)], layout="rgb+alpha", box=(10, 6, 55, 40)),
    "all_empty": dict(T=2, H=33, W=47, fg=[None, None], layout="rgba", box=None),
    "thr_edge": dict(T=1, H=24, W=40, fg="checker", layout="rgba", box=(3, 2, 36, 21)),
    "padded": dict(T=2, H=90, W=120, fg=[(17, 11, 95, 70), (20, 15, 90, 66)], layout="padded", box=(17, 11, 95, 70), same_as="interior"),
}
GOLDEN_CASES = [n for n, c in CASES.items() if c["box"] is not None and "same_as" not in c]          # what the reference can run
WINDOW = 48                                                 # the golden keeps this corner of the pasted region of two frames


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def make_video(name):
    """(rgb uint8 [T,H,W,3], alpha uint8 [T,H,W]): noise everywhere (the background's colours are NOT black: zeroing them is the
    masking's work), background alpha in 0..204, foreground alpha in 205..255 with a tenth of it punched back to background;
    the two corner pixels that pin the rectangle are foreground"""
    c = CASES[c_name] if (c_name := CASES[name].get("same_as")) else CASES[name]
    rng = np.random.default_rng(_seed(c_name or name))
    T, H, W = c["T"], c["H"], c["W"]
    rgb = rng.integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)
    alpha = rng.integers(0, 205, size=(T, H, W)).astype(np.uint8)
    if c["fg"] == "checker":                                # 204 and 205 side by side: the threshold is `>`, not `>=`
        yy, xx = np.mgrid[0:H, 0:W]
        inside = (xx >= 3) & (xx < 36) & (yy >= 2) & (yy < 21)
        alpha[0] = np.where(inside, np.where((xx + yy) % 2 == 0, 205, 204), alpha[0]).astype(np.uint8)
        alpha[0, 2, 3] = alpha[0, 20, 35] = 205             # the two corners that pin the box
        return rgb, alpha
    for t, box in enumerate(c["fg"]):
        if box is None:
            continue
        left, top, right, bottom = box
        region = rng.integers(205, 256, size=(bottom - top, right - left))
        holes = rng.random(region.shape) < 0.1
        region[holes] = rng.integers(0, 205, size=int(holes.sum()))
        alpha[t, top:bottom, left:right] = region.astype(np.uint8)
        alpha[t, top, left] = 205
        alpha[t, bottom - 1, right - 1] = 254
    return rgb, alpha


def soft_video():
    """one 256 x 256 frame with rgb = row and alpha = column: every entry of the soft table is used"""
    row, col = np.mgrid[0:256, 0:256]
    rgb = np.repeat(row[None, :, :, None], 3, axis=3).astype(np.uint8)
    rgb[..., 1] = 255 - rgb[..., 1]
    return rgb, col[None].astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the model
def model_lanczos(t):
    if t < -3.0 or t >= 3.0:
        return 0.0
    s = 1.0
    for u in (t, t / 3.0):
        if u != 0.0:
            u = u * math.pi
            s = s * (math.sin(u) / u)
    return s


def model_tables(in_size, out_size):
    """coefficients (22 fractional bits) and (first sample, taps) of every output of one pass"""
    scale = in_size / out_size
    stretch = scale if scale > 1.0 else 1.0
    support = 3.0 * stretch
    ksize = 2 * int(math.ceil(support)) + 1
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        first = int(center - support + 0.5)
        first = 0 if first < 0 else first
        last = int(center + support + 0.5)
        last = in_size if last > in_size else last
        w = []
        total = 0.0
        for x in range(first, last):
            w.append(model_lanczos((x - center + 0.5) * (1.0 / stretch)))
            total += w[-1]
        for k in range(len(w)):
            v = w[k] / total if total != 0.0 else w[k]
            coef[i, k] = int(v * 4194304.0 - 0.5) if v < 0 else int(v * 4194304.0 + 0.5)
        bounds[i, 0], bounds[i, 1] = first, last - first
    return coef, bounds


def model_pass(img, coef, bounds, axis):
    """img uint8 [T, R, Cc, C]; axis 1 resamples along Cc (x), axis 0 along R (y).  One output line at a time, one tap at a time,
    in a 32-bit sum that wraps as two's complement."""
    src = np.moveaxis(img, 2 if axis == 1 else 1, 0).astype(np.int64)            # [in, ...]
    out = np.empty((coef.shape[0],) + src.shape[1:], dtype=np.uint8)
    for o in range(coef.shape[0]):
        acc = np.full(src.shape[1:], 1 << 21, dtype=np.int64)
        for k in range(int(bounds[o, 1])):
            acc += src[int(bounds[o, 0]) + k] * int(coef[o, k])
        acc = ((acc + 2 ** 31) % 2 ** 32) - 2 ** 31
        out[o] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, 2 if axis == 1 else 1)


def model_soft_table():
    table = np.zeros((256, 256), dtype=np.uint8)
    for a in range(256):
        for v in range(256):
            table[a, v] = int(v * (a / 255.0))
    return table


def model_mask(rgb, alpha, mode="threshold", threshold=204):
    """(masked rgb, mask): threshold -> keep or zero, mask 0 / 255; soft -> the table, mask = alpha"""
    if mode == "soft":
        return model_soft_table()[alpha[..., None], rgb], alpha.copy()
    keep = alpha > threshold
    return np.where(keep[..., None], rgb, 0).astype(np.uint8), (keep * 255).astype(np.uint8)


def model_boxes(mask):
    """int32 [T, 4]; a frame without foreground keeps (W, H, 0, 0)"""
    T, H, W = mask.shape
    boxes = np.empty((T, 4), dtype=np.int32)
    for t in range(T):
        ys, xs = np.nonzero(mask[t] > 0)
        boxes[t] = (W, H, 0, 0) if len(xs) == 0 else (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return boxes


def model_placement(box, size=SIZE):
    w, h = box[2] - box[0], box[3] - box[1]
    s = size / max(w, h)
    new_w, new_h = max(1, int(round(w * s))), max(1, int(round(h * s)))
    return new_w, new_h, (size - new_w) // 2, (size - new_h) // 2


def model_resize(img, new_w, new_h):
    """img uint8 [T, h, w, C] -> [T, new_h, new_w, C]: the horizontal pass into a uint8 intermediate, then the vertical one.
    Pillow's Image.resize turns the order round for an image over a hundred times as tall as wide whose height shrinks."""
    h, w = img.shape[1:3]
    if h > 100 * w and new_h < h:
        mid = model_pass(img, *model_tables(h, new_h), axis=0)
        return model_pass(mid, *model_tables(w, new_w), axis=1)
    mid = model_pass(img, *model_tables(w, new_w), axis=1)
    return model_pass(mid, *model_tables(h, new_h), axis=0)


def model_frame(rgb, alpha, size=SIZE, mode="threshold", threshold=204):
    """dict(frames [T,size,size,3], mask [T,size,size], box, placement), or None when no frame has foreground"""
    masked, mask = model_mask(rgb, alpha, mode, threshold)
    boxes = model_boxes(mask)
    live = boxes[boxes[:, 0] < boxes[:, 2]]
    if len(live) == 0:
        return None
    box = (int(live[:, 0].min()), int(live[:, 1].min()), int(live[:, 2].max()), int(live[:, 3].max()))
    new_w, new_h, off_x, off_y = place = model_placement(box, size)
    T = len(rgb)
    frames = np.zeros((T, size, size, 3), dtype=np.uint8)
    canvas = np.zeros((T, size, size), dtype=np.uint8)
    crop = (slice(None), slice(box[1], box[3]), slice(box[0], box[2]))
    frames[:, off_y:off_y + new_h, off_x:off_x + new_w] = model_resize(masked[crop], new_w, new_h)
    canvas[:, off_y:off_y + new_h, off_x:off_x + new_w] = model_resize(mask[crop][..., None], new_w, new_h)[..., 0]
    return dict(frames=frames, mask=canvas, box=box, placement=place, boxes=boxes)


_MODEL = {}


def model_of(name):
    """the model's result for a case, computed once and shared (read-only) by the tests"""
    if name not in _MODEL:
        out = model_frame(*make_video(name))
        if out is not None:
            for a in (out["frames"], out["mask"], out["boxes"]):
                a.setflags(write=False)
        _MODEL[name] = out
    return _MODEL[name]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
