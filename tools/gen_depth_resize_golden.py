"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/resize_pil_f32.npz from PILLOW ITSELF (not from the code under test): what the
reference's depth_transform (ToPILImage -> Resize(256) -> CenterCrop(224) -> ToTensor on a float32 (H, W, 1) array) makes of three
seeded raw depth frames.  ToPILImage turns such an array into a mode-F image and Resize(256) calls Image.resize with BILINEAR on it;
both are spelled out here with Pillow alone, so torchvision is not needed.  Run from the repository root:

    python -B tools/gen_depth_resize_golden.py

Stored: in0..in2 (84x84, 130x100, 200x180, values in [0.5, 10)), out0..out2 (the 224x224 centre crop of the resized frame) and
pillow_version.
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((84, 84), (130, 100), (200, 180))
SEED, SIZE, CROP = 20240607, 256, 224


def pillow_depth_transform(frame):
    h, w = frame.shape
    # torchvision Resize(int): the shorter side becomes SIZE, the longer int(SIZE * long / short)
    if (w <= h and w == SIZE) or (h <= w and h == SIZE):
        hr, wr = h, w
    elif w < h:
        hr, wr = int(SIZE * h / w), SIZE
    else:
        hr, wr = SIZE, int(SIZE * w / h)
    im = Image.fromarray(frame)   # float32 (H, W) -> mode F, as ToPILImage does for a float32 (H, W, 1) array
    assert im.mode == "F"
    if (hr, wr) != (h, w):
        im = im.resize((wr, hr), Image.BILINEAR)
    out = np.asarray(im, dtype=np.float32)
    top, left = int(round((hr - CROP) / 2.0)), int(round((wr - CROP) / 2.0))   # CenterCrop
    return np.ascontiguousarray(out[top:top + CROP, left:left + CROP])


def main():
    rng = np.random.default_rng(SEED)
    rec = {"pillow_version": np.array(PIL.__version__)}
    for i, (h, w) in enumerate(SIZES):
        frame = (0.5 + 9.5 * rng.random((h, w))).astype(np.float32)
        rec["in%d" % i] = frame
        rec["out%d" % i] = pillow_depth_transform(frame)
    path = os.path.join(ROOT, "tests", "golden", "resize_pil_f32.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print("%s: %d bytes (Pillow %s)" % (path, size, PIL.__version__))
    assert size <= 1000 * 1000, size


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
