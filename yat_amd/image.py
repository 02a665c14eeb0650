"""Image ingest on the device: Pillow's antialiased bilinear resize of an [H, W, 3] uint8 image, bit for bit.

``resize_uint8(img, th, tw)`` returns the bytes of ``Image.fromarray(img).resize((tw, th), Image.BILINEAR)`` -- what
torchvision's ``Resize((th, tw))`` does to a PIL image (bucket_sampler.py:324-398) -- as a device tensor, or writes them
into ``out``, e.g. one slot of the ``[B, th, tw, 3]`` batch that ``encode_uint8`` reads.  Pillow's 8-bit resample is integer
arithmetic over per-axis coefficient tables; the tables are built here, on the host, in IEEE doubles exactly as Pillow
builds them (``resample_tables``; tests/image_resize_ref.py is the scalar restatement they are held to) and uploaded as one
packed int32 block; the kernels of csrc/image.hip do the integer work.

Scope of the device path: ``max(h / w, w / h) <= 16`` (the aspect tables end at ratio 4) and ``H * W * 3 < 2^31``.  Pillow 12
resizes an image with ``h > 100 w`` in another pass order (1000 x 9 -> 7 x 6 differs from the horizontal-first result, 1000
x 10 does not), so anything more extreme than 16, any image of 2^31 bytes or more, and any size the library refuses is
resized by Pillow itself on the host; the result is Pillow's either way.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import lib as _l

PRECISION_BITS = 22
MAX_ASPECT = 16


def resample_tables(in_size: int, out_size: int):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the triangle filter -> (ksize, bounds [out_size, 2]
    int32 = (xmin, n), kk [out_size, ksize] int32, zero beyond n).  Vectorised over the output index; the taps are walked in
    order so that the weight sum is accumulated as Pillow accumulates it."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError("resample_tables: sizes must be positive")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    c = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(c - support + 0.5), 0.0).astype(np.int64)
    n = np.minimum(np.trunc(c + support + 0.5), float(in_size)).astype(np.int64) - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):
        v = np.maximum(0.0, 1.0 - np.abs((x + xmin - c + 0.5) / fs))
        v[x >= n] = 0.0
        w[:, x] = v
        ww = ww + v                                            # (adding 0.0 beyond n leaves the sum's bits alone)
    nz = ww != 0.0
    w[nz] = w[nz] / ww[nz, None]
    kk = np.trunc(w * float(1 << PRECISION_BITS) + 0.5).astype(np.int32)
    kk[np.arange(ksize)[None, :] >= n[:, None]] = 0
    return ksize, np.stack([xmin, n], axis=1).astype(np.int32), kk


def axis_ksize(in_size: int, out_size: int) -> int:
    """``ksize`` as the library expects it: 0 for an axis whose size does not change (the pass is skipped)."""
    return 0 if in_size == out_size else int(math.ceil(max(in_size / out_size, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=256)
def packed_tables(H: int, W: int, th: int, tw: int) -> np.ndarray:
    """The int32 block of yat_image_resize_u8: [hbounds | hk | vbounds | vk], a skipped axis leaving nothing."""
    parts = []
    for in_size, out_size in ((W, tw), (H, th)):
        if in_size != out_size:
            _, bounds, kk = resample_tables(in_size, out_size)
            parts += [bounds.reshape(-1), kk.reshape(-1)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)


_DEVICE_TABLES = {}


def _device_tables(H, W, th, tw, device):
    key = (H, W, th, tw, str(device))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        if len(_DEVICE_TABLES) >= 256:                         # photographs come in few sizes per dataset; bound it anyway
            _DEVICE_TABLES.clear()
        t = torch.from_numpy(packed_tables(H, W, th, tw)).to(device)
        _DEVICE_TABLES[key] = t
    return t


def resize_plan(H: int, W: int, th: int, tw: int) -> int:
    """Which form the device resize takes (pure host code, yat_image_resize_plan): 1 = one launch, both passes of an output
    tile through LDS; 2 = two launches through a workspace (large vertical reductions); -1 = sizes the library refuses."""
    return int(_l.load().yat_image_resize_plan(int(H), int(W), int(th), int(tw)))


def on_device_path(H: int, W: int, th: int, tw: int) -> bool:
    """Whether ``resize_uint8`` runs an image of these sizes on the device (else: Pillow on the host)."""
    if min(H, W, th, tw) <= 0 or max(H / W, W / H) > MAX_ASPECT or H * W * 3 >= 1 << 31:
        return False
    return resize_plan(H, W, th, tw) > 0


def pillow_resize(img_u8: torch.Tensor, th: int, tw: int) -> torch.Tensor:
    """The host resize: ``Image.fromarray(img).resize((tw, th), Image.BILINEAR)`` as a [th, tw, 3] uint8 host tensor."""
    from PIL import Image
    arr = np.ascontiguousarray(img_u8.cpu().numpy())
    return torch.from_numpy(np.array(Image.fromarray(arr, "RGB").resize((int(tw), int(th)), Image.BILINEAR), dtype=np.uint8))


def resize_uint8_device(img_u8: torch.Tensor, th: int, tw: int, out: torch.Tensor = None) -> torch.Tensor:
    """The device resize without the scope checks of ``resize_uint8``: ``img_u8`` a contiguous [H, W, 3] uint8 DEVICE tensor ->
    [th, tw, 3] uint8 on its device (``out`` when given: contiguous, on the same device).  Raises where the library refuses."""
    from . import ops
    H, W, _ = img_u8.shape
    th, tw = int(th), int(tw)
    if out is None:
        out = torch.empty(th, tw, 3, dtype=torch.uint8, device=img_u8.device)
    elif tuple(out.shape) != (th, tw, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != img_u8.device:
        raise ValueError(f"out must be a contiguous [{th}, {tw}, 3] uint8 tensor on {img_u8.device}")
    tables = _device_tables(H, W, th, tw, img_u8.device)
    ops.image_resize_u8(img_u8, tables if tables.numel() else None, axis_ksize(W, tw), axis_ksize(H, th), out)
    return out


def resize_uint8(img_u8: torch.Tensor, th: int, tw: int, out: torch.Tensor = None, device="cuda") -> torch.Tensor:
    """``img_u8``: a host or device [H, W, 3] uint8 tensor -> Pillow's ``resize((tw, th), Image.BILINEAR)`` of it as a
    [th, tw, 3] uint8 tensor on ``device`` (the image's own device when it is already on one), or in ``out``.  A host image
    is uploaded once, whole; images outside the device path's scope (module docstring) go through Pillow on the host."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[-1] != 3:
        raise ValueError(f"img_u8 must be [H, W, 3] uint8, got {tuple(img_u8.shape)} {img_u8.dtype}")
    H, W, _ = img_u8.shape
    dev = img_u8.device if img_u8.is_cuda else torch.device(device)
    if not on_device_path(H, W, int(th), int(tw)):
        res = pillow_resize(img_u8, th, tw)
        if out is None:
            return res.to(dev)
        out.copy_(res)
        return out
    return resize_uint8_device(img_u8.to(dev).contiguous(), th, tw, out)
