"""Numpy restatement of Pillow's antialiased bilinear resize of an 8-bit RGB image (``img.resize((tw, th), Image.BILINEAR)``:
``ImagingResample`` with the triangle filter), the reference the HIP resize kernels and ``yat_amd.image.resample_tables`` are
held to.  Pillow's 8-bit path is integer arithmetic over coefficient tables computed in IEEE doubles, so the restatement is
exact: every byte equals Pillow's.

Per axis (input size ``inS``, output size ``outS``): ``scale = inS / outS``, ``fs = max(scale, 1)``, ``support = fs`` (the
triangle filter's own support is 1), ``ksize = ceil(support) * 2 + 1``.  For output index ``xx``: ``c = (xx + 0.5) * scale``,
``xmin = max(int(c - support + 0.5), 0)``, ``n = min(int(c + support + 0.5), inS) - xmin``, weights ``w[x] = max(0, 1 -
|(x + xmin - c + 0.5) / fs|)`` for ``x < n`` summed in order and divided by the sum, then ``k[x] = int(w[x] * 2^22 + 0.5)``.
A pass along an axis is ``clamp((2^21 + sum_x in[xmin + x] * k[x]) >> 22, 0, 255)``.  The horizontal pass runs first and its
result is rounded to uint8 before the vertical pass reads it; an axis whose size does not change is skipped.

Scope: Pillow 12 resizes an image with ``h > 100 w`` in another pass order; the device path (and this restatement's claim of
exactness) covers ``max(h / w, w / h) <= 16``.
"""
import math

import numpy as np

PRECISION_BITS = 22
MAX_ASPECT = 16


def tables(in_size: int, out_size: int):
    """-> (ksize, bounds [out_size, 2] int32 = (xmin, n), kk [out_size, ksize] int32, zero beyond n), written as the scalar
    loops of the description above."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(n):
            v = max(0.0, 1.0 - abs((x + xmin - c + 0.5) / fs))
            w.append(v)
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    return ksize, bounds, kk


def _pass(img: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """One pass along axis 0 of ``img`` [S, ...] uint8 -> [out_size, ...] uint8."""
    out = np.empty((bounds.shape[0],) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    tail = (1,) * (img.ndim - 1)
    for i, (xmin, n) in enumerate(bounds):
        acc = (src[xmin:xmin + n] * kk[i, :n].astype(np.int64).reshape((n,) + tail)).sum(axis=0) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img: np.ndarray, th: int, tw: int) -> np.ndarray:
    """[H, W, 3] uint8 -> [th, tw, 3] uint8, Pillow's bytes."""
    H, W, _ = img.shape
    out = img
    if tw != W:
        _, b, k = tables(W, tw)
        out = _pass(out.transpose(1, 0, 2), b, k).transpose(1, 0, 2)
    if th != H:
        _, b, k = tables(H, th)
        out = _pass(out, b, k)
    return np.ascontiguousarray(out)


def pillow_resize(img: np.ndarray, th: int, tw: int) -> np.ndarray:
    from PIL import Image
    return np.array(Image.fromarray(img, "RGB").resize((tw, th), Image.BILINEAR), dtype=np.uint8)


# (h, w) -> (th, tw): the shapes every resize test walks (down, up, one axis skipped, copy, degenerate, large ksize, the
# two-launch plan, ragged tile edges, a very wide source)
SHAPES = [
    ((37, 53), (16, 24)), ((16, 24), (37, 53)),
    ((33, 33), (33, 16)), ((33, 33), (16, 33)),
    ((48, 64), (48, 64)),
    ((1, 1), (4, 4)), ((2, 3), (1, 1)),
    ((7, 300), (8, 32)),
    ((640, 480), (40, 24)),
    ((257, 129), (32, 32)), ((301, 203), (256, 256)),
    ((96, 160), (192, 320)), ((129, 257), (128, 256)),
    ((3, 1000), (2, 7)),
]


def test_images(h: int, w: int, seed: int = 0):
    """A random image and two saturating ones (0/255 checkerboards of 1 and 3 pixels)."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    out = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8)]
    for cell in (1, 3):
        board = (((yy // cell + xx // cell) & 1) * 255).astype(np.uint8)
        out.append(np.ascontiguousarray(np.stack([board, 255 - board, board], axis=-1)))
    return out
