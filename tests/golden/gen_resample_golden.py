"""Writes tests/golden/resample_pillow.npz: random uint8 images and what Pillow's own bilinear ``Image.resize`` makes of them.

Needs Pillow (the fixture was written with 12.2.0); the tests that read the fixture do not.
    python tests/golden/gen_resample_golden.py
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

IMAGES = [(37, 53), (64, 48), (33, 64), (5, 5)]            # (h, w), three channels each
PAIRS = [                                                   # (image, new_h, new_w)
    (0, 50, 70), (0, 17, 29), (0, 1, 53), (0, 37, 1),
    (1, 64, 20), (1, 20, 48), (1, 61, 45),
    (2, 5, 8), (2, 33, 64), (2, 40, 40),
    (3, 1, 1), (3, 9, 13),
]
# image, flip, first resize (h, w), crop (y0, x0, ch, cw), final resize (h, w)
CHAIN = (1, 1, 48, 36, 5, 3, 30, 25, 56, 47)


def pil_resize(img, new_h, new_w):
    return np.asarray(Image.fromarray(img).resize((new_w, new_h), Image.BILINEAR))


def main():
    rng = np.random.default_rng(20240607)
    data = {}
    images = []
    for i, (h, w) in enumerate(IMAGES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i == 1:
            img[:, : w // 2] = np.where(img[:, : w // 2] > 127, 255, 0)   # saturated edges: the clamp and the rounding term
        images.append(img)
        data["img%d" % i] = img
    data["pairs"] = np.array(PAIRS, np.int32)
    for j, (i, nh, nw) in enumerate(PAIRS):
        data["out%d" % j] = pil_resize(images[i], nh, nw)
    i, flip, fh, fw, y0, x0, ch, cw, nh, nw = CHAIN
    img = images[i][:, ::-1] if flip else images[i]
    img = pil_resize(np.ascontiguousarray(img), fh, fw)
    img = np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
    data["chain"] = np.array(CHAIN, np.int32)
    data["chain_out"] = pil_resize(img, nh, nw)
    path = os.path.join(HERE, "resample_pillow.npz")
    np.savez(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
