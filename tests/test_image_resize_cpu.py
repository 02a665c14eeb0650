"""Host side of the Pillow-exact resize (yat_amd/image.py, csrc/image.hip): the numpy restatement against Pillow, the table
builder against the restatement, the entry point's argument checks and the plan query.  No GPU."""
import random

import numpy as np
import pytest
import torch

from tests import image_resize_ref as R
from yat_amd import image as yimg
from yat_amd import lib as ylib


def _sweep(count=220, seed=0):
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        h, w, th, tw = rng.randint(1, 400), rng.randint(1, 400), rng.randint(1, 130), rng.randint(1, 130)
        if max(h / w, w / h) <= R.MAX_ASPECT:
            out.append(((h, w), (th, tw)))
    return out


def test_tables_equal_the_restatement():
    """``resample_tables`` (vectorised) == the scalar loops of tests/image_resize_ref.py, entry for entry."""
    sizes = {(a, b) for (h, w), (th, tw) in R.SHAPES + _sweep(60, 1) for a, b in ((h, th), (w, tw))}
    sizes |= {(4000, 1152), (3000, 896), (1, 1), (1, 7), (7, 1), (1000, 3)}
    for in_size, out_size in sorted(sizes):
        k0, b0, c0 = R.tables(in_size, out_size)
        k1, b1, c1 = yimg.resample_tables(in_size, out_size)
        assert k0 == k1 and b1.dtype == np.int32 and c1.dtype == np.int32, (in_size, out_size)
        assert np.array_equal(b0, b1) and np.array_equal(c0, c1), (in_size, out_size)


def test_restatement_matches_pillow_bit_for_bit():
    mismatches = []
    for (h, w), (th, tw) in R.SHAPES:
        for img in R.test_images(h, w):
            if not np.array_equal(R.resize(img, th, tw), R.pillow_resize(img, th, tw)):
                mismatches.append(((h, w), (th, tw)))
    for n, ((h, w), (th, tw)) in enumerate(_sweep()):
        img = np.random.default_rng(n).integers(0, 256, (h, w, 3), dtype=np.uint8)
        if not np.array_equal(R.resize(img, th, tw), R.pillow_resize(img, th, tw)):
            mismatches.append(((h, w), (th, tw)))
    assert not mismatches, mismatches


@pytest.mark.parametrize("in_size,out_size", [(53, 24), (24, 53), (300, 32), (7, 8), (480, 24), (1, 4), (3, 1), (1000, 7)])
def test_ksize_and_bounds_at_the_clamped_edges(in_size, out_size):
    ksize, bounds, kk = yimg.resample_tables(in_size, out_size)
    scale = in_size / out_size
    assert ksize == int(np.ceil(max(scale, 1.0))) * 2 + 1 == yimg.axis_ksize(in_size, out_size)
    assert yimg.axis_ksize(in_size, in_size) == 0
    xmin, n = bounds[:, 0], bounds[:, 1]
    assert xmin[0] == 0 and xmin[-1] + n[-1] == in_size                   # the first and last window are clamped to the source
    assert (xmin >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (xmin + n <= in_size).all()
    assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()
    # the clamped windows lose taps, not weight: every row still sums to 2^22 within one unit per tap
    assert (np.abs(kk.sum(axis=1) - (1 << 22)) <= n).all()
    assert all((kk[i, n[i]:] == 0).all() for i in (0, out_size - 1))
    assert (kk >= 0).all()


def test_argument_checks_return_einval(built_lib):
    """Validation precedes any launch: the fake non-null pointers are never dereferenced."""
    lib = ylib.load()
    P, EINVAL = 0x7f0000001000, -1
    good = dict(H=37, W=53, th=16, tw=24, kh=7, kv=7, src=P, tables=P, dst=P + (1 << 20), ws=None)

    def call(**kw):
        a = {**good, **kw}
        return lib.yat_image_resize_u8(a["H"], a["W"], a["th"], a["tw"], a["kh"], a["kv"], a["src"], a["tables"], a["dst"],
                                       a["ws"], None)

    for name in ("H", "W", "th", "tw"):
        for bad in (0, -3):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    for name in ("src", "tables", "dst"):
        assert call(**{name: None}) == EINVAL, name
    assert call(dst=P) == EINVAL                                               # in place
    for kw in (dict(kh=5), dict(kh=9), dict(kv=0), dict(kh=0, kv=0), dict(kv=8)):
        assert call(**kw) == EINVAL, kw                                        # ksize is not what the sizes give
    assert call(H=16, kv=7) == EINVAL and call(W=24, kh=7) == EINVAL           # a skipped axis has ksize 0
    # byte counts: 2^31 - 3 is the last accepted source size
    assert call(H=1 << 15, W=21846, kh=0, kv=0) == EINVAL                      # 2^31 + 6 bytes
    assert call(H=1 << 20, W=1 << 20) == EINVAL and call(H=1 << 30, W=1 << 30) == EINVAL
    assert call(th=1 << 15, tw=21846) == EINVAL
    assert lib.yat_image_resize_plan(1 << 15, 21846, 16, 24) == EINVAL
    assert lib.yat_image_resize_plan(1 << 15, 21845, 16, 24) > 0               # 2^31 - 3 * 2^15 ... below the limit
    # the two-launch plan needs its workspace
    assert lib.yat_image_resize_plan(640, 480, 40, 24) == 2
    assert call(H=640, W=480, th=40, tw=24, kh=41, kv=33, ws=None) == EINVAL
    if not torch.cuda.is_available():                                          # accepted arguments get as far as the launch
        assert call() > 0


def test_plan_query_is_pure_host_code_and_splits_the_shapes(built_lib):
    plans = {shape: yimg.resize_plan(*shape[0], *shape[1]) for shape in R.SHAPES}
    assert set(plans.values()) == {1, 2}, plans
    assert plans[((640, 480), (40, 24))] == 2
    assert plans[((37, 53), (16, 24))] == 1 and plans[((48, 64), (48, 64))] == 1
    lib = ylib.load()
    assert lib.yat_image_resize_workspace_bytes(640, 480, 40, 24) == 640 * 24 * 3
    assert lib.yat_image_resize_workspace_bytes(37, 53, 16, 24) == 0
    # a 12-megapixel photograph to its 1024 bucket runs in one launch; the boundary sits where 16 output rows read more
    # source rows than the 170 of the LDS image: ceil(16 H / th) + ksize_v
    assert yimg.resize_plan(4000, 3000, 1152, 896) == 1
    assert yimg.resize_plan(9 * 64, 64, 64, 64) == 1 and yimg.resize_plan(10 * 64, 64, 64, 64) == 2
    assert yimg.resize_plan(0, 3, 1, 1) == -1


def test_extreme_aspects_take_the_pillow_fallback(built_lib):
    """``resize_uint8`` keeps images with aspect > 16 off the device path (``device='cpu'``: a device call would raise here) and
    still returns Pillow's bytes -- including the tall case where Pillow's result is NOT the horizontal-first one."""
    assert not yimg.on_device_path(1000, 9, 7, 6) and not yimg.on_device_path(3, 1000, 2, 7)
    assert not yimg.on_device_path(17, 1, 4, 4) and yimg.on_device_path(16, 1, 4, 4) and yimg.on_device_path(37, 53, 16, 24)
    for (h, w), (th, tw) in [((1000, 9), (7, 6)), ((3, 1000), (2, 7)), ((7, 300), (8, 32)), ((340, 20), (33, 9))]:
        img = R.test_images(h, w)[0]
        got = yimg.resize_uint8(torch.from_numpy(img), th, tw, device="cpu")
        assert got.dtype == torch.uint8 and tuple(got.shape) == (th, tw, 3)
        assert np.array_equal(got.numpy(), R.pillow_resize(img, th, tw)), ((h, w), (th, tw))
        out = torch.zeros(th, tw, 3, dtype=torch.uint8)
        assert yimg.resize_uint8(torch.from_numpy(img), th, tw, out=out, device="cpu") is out
        assert np.array_equal(out.numpy(), R.pillow_resize(img, th, tw))
