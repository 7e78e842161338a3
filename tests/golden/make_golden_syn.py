#!/usr/bin/env python
"""Fixture of the `--syn` input path: PILLOW'S OWN outputs for the two steps of the reference's
`alignCollate_syn.__call__` (dataset/dataset.py:952-992) on a few small random images --

    :984-986  images_lr = [image.resize((image.size[0] // s, image.size[1] // s), Image.BICUBIC) ...]        -> st{s}_{j}
    :989      transform2 = resizeNormalize((imgW // s, imgH // s), mask) on those (dataset/dataset.py:615-632) -> lr{s}_{j}, lr{s}_{j}_mask
    :981      transform  = resizeNormalize((imgW, imgH), mask) on the source                                   -> hr{j}, hr{j}_mask

for (imgW, imgH) = (128, 32) and s = 2, 4; the images are stored as uint8 (ToTensor is / 255), the masks as Pillow's 0 / 255.
An image with `w // s == 0` or `h // s == 0` is left out of that scale (`idx{s}` lists the ones kept): Pillow raises there.

    python tests/golden/make_golden_syn.py          # rewrites tests/golden/syn_resize.npz"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (H, W): neither divisible by 2 or 4; 32 x 128 (s = 2 lands on 16 x 64, s = 4 on 8 x 32: the second resize is an identity); 5 x 9
# (s = 2: the second stage UPsamples from 2 x 4; s = 4: h // s == 1); a tall image (H = 70) next to one of H = 6 (the horizontal
# pass's padded scratch; s = 4: h // s == 1); h // 2 == 1; w // 4 == 1; w // 2 == 1
SIZES = [(37, 211), (32, 128), (5, 9), (70, 260), (6, 33), (3, 40), (40, 5), (21, 3)]
IMG_WH = (128, 32)
SCALES = (2, 4)


def resize_normalize_u8(pil, size, Image):
    """dataset/dataset.py:622-629 before ToTensor: (resized uint8 image, 0 / 255 mask)"""
    img = pil.resize(size, Image.BICUBIC)
    mask = img.convert("L")
    thres = np.array(mask).mean()
    return np.array(img), np.array(mask.point(lambda x: 0 if x > thres else 255))


def main():
    import PIL
    from PIL import Image
    rng = np.random.default_rng(11)
    out = {}
    for j, (h, w) in enumerate(SIZES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if j == 0:      # a smooth image (natural-like): gradients + noise in the low bits
            yy, xx = np.mgrid[0:h, 0:w]
            img = np.stack([(xx * 255 / w), (yy * 255 / h), ((xx + yy) * 255 / (w + h))], -1).astype(np.uint8) ^ (img & 7)
        out[f"img{j}"] = img
        pil = Image.fromarray(img)
        out[f"hr{j}"], out[f"hr{j}_mask"] = resize_normalize_u8(pil, IMG_WH, Image)
    for s in SCALES:
        keep = [j for j, (h, w) in enumerate(SIZES) if h // s and w // s]
        out[f"idx{s}"] = np.array(keep)
        for j in keep:
            pil = Image.fromarray(out[f"img{j}"])
            st = pil.resize((pil.size[0] // s, pil.size[1] // s), Image.BICUBIC)
            out[f"st{s}_{j}"] = np.array(st)
            out[f"lr{s}_{j}"], out[f"lr{s}_{j}_mask"] = resize_normalize_u8(st, (IMG_WH[0] // s, IMG_WH[1] // s), Image)
    path = os.path.join(HERE, "syn_resize.npz")
    np.savez_compressed(path, pillow=np.array(PIL.__version__), n=np.array(len(SIZES)), **out)
    print("syn fixture from Pillow", PIL.__version__, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
