#!/usr/bin/env python3
"""Golden of the video framing, produced by the reference's OWN `process_images_in_folder` (utils/rmbg_for_black_bg.py), run
unmodified on the clips of tests/framing_cases.py written out as RGBA PNGs.

Every frame has at least one non-opaque pixel and frame 0 has foreground, so the reference takes the matte from the file's
alpha and never calls the matting network.  The shims, all of them for modules the reference imports at its top but does not
need on this path:
  * `rembg`: `new_session` returns None; `remove` raises (it must not be reached);
  * `cv2`: an empty module (video decoding only);
  * `tqdm`, `easydict`: stand-ins when the real ones are not installed (a progress bar; the argument namespace of its main()).
Pillow is the real one: its resampling is what the golden pins.

Per case the golden keeps the union box (the reference does not write it out, so its own compute_mask_bbox / merge_bbox run
again over the `mask/` files it wrote), the placement (crop_and_center_to_512's arithmetic on that box), a SHA-256 of every
512 x 512 canvas of `masked_rgb/` and `mask_512/`, and the top-left WINDOW x WINDOW corner of the pasted region of the first and
the last frame.  Not run by pytest.  Build container only (needs /root/reference and PIL).  Output: tests/golden/framing.npz."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import framing_cases as fc  # noqa: E402


def _refuse(*a, **k):
    raise AssertionError("the reference asked for the matting network: a frame is fully opaque or not RGBA")


sys.modules["rembg"] = types.SimpleNamespace(new_session=lambda name: None, remove=_refuse)
sys.modules["cv2"] = types.ModuleType("cv2")
for name, attr in (("tqdm", "tqdm"), ("easydict", "EasyDict")):
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.SimpleNamespace(**{attr: dict})

spec = importlib.util.spec_from_file_location("rmbg_for_black_bg", "/root/reference/utils/rmbg_for_black_bg.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

save = {}
for name in fc.GOLDEN_CASES:
    rgb, alpha = fc.make_video(name)
    T = len(rgb)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(src)
        for t in range(T):
            assert (alpha[t] < 255).any() and (t > 0 or (alpha[0] > 204).any())
            Image.fromarray(np.concatenate([rgb[t], alpha[t][..., None]], axis=2), mode="RGBA").save(os.path.join(src, f"{t:04d}.png"))
        ref.process_images_in_folder(src, out)
        frames = np.stack([np.asarray(Image.open(os.path.join(out, "masked_rgb", f"{t:04d}_masked_rgb.png"))) for t in range(T)])
        masks = np.stack([np.asarray(Image.open(os.path.join(out, "mask_512", f"{t:04d}_mask_512.png"))) for t in range(T)])
        box = None
        for t in range(T):
            box = ref.merge_bbox(box, ref.compute_mask_bbox(Image.open(os.path.join(out, "mask", f"{t:04d}_mask.png"))))
    assert frames.shape == (T, 512, 512, 3) and masks.shape == (T, 512, 512) and frames.dtype == masks.dtype == np.uint8
    box = tuple(int(v) for v in box)
    # the reference's own placement arithmetic (crop_and_center_to_512), on the box it merged
    w, h = box[2] - box[0], box[3] - box[1]
    scale = 512 / max(w, h)
    new_w, new_h = max(1, int(round(w * scale))), max(1, int(round(h * scale)))
    off_x, off_y = (512 - new_w) // 2, (512 - new_h) // 2
    outside = np.ones((512, 512), dtype=bool)
    outside[off_y:off_y + new_h, off_x:off_x + new_w] = False
    assert not frames[:, outside].any() and not masks[:, outside].any()          # black outside the pasted region
    win = (slice(off_y, off_y + min(new_h, fc.WINDOW)), slice(off_x, off_x + min(new_w, fc.WINDOW)))
    save[f"{name}.box"] = np.array(box, dtype=np.int32)
    save[f"{name}.placement"] = np.array((new_w, new_h, off_x, off_y), dtype=np.int32)
    save[f"{name}.frames_sha256"] = np.array([fc.digest(f) for f in frames])
    save[f"{name}.mask_sha256"] = np.array([fc.digest(m) for m in masks])
    for tag, t in (("first", 0), ("last", T - 1)):
        save[f"{name}.{tag}_frame"] = frames[t][win].copy()
        save[f"{name}.{tag}_mask"] = masks[t][win].copy()
    model = fc.model_of(name)
    print(name, box, (new_w, new_h, off_x, off_y), "model equal:", bool(np.array_equal(model["frames"], frames) and np.array_equal(model["mask"], masks)))

path = os.path.join(HERE, "framing.npz")
np.savez_compressed(path, **save)
print(path, os.path.getsize(path), "bytes")
