"""The HIP resize (csrc/image.hip through yat_amd.image) against Pillow, byte for byte: random and saturating images at every
shape of tests/image_resize_ref.py SHAPES, written into the middle slot of a sentinel-filled batch, on both plans."""
import numpy as np
import pytest
import torch

from tests import image_resize_ref as R
from yat_amd import image as yimg

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def plans_run():
    return set()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_device_resize_equals_pillow(shape, plans_run, built_lib):
    """``resize_uint8_device`` -- the kernels themselves, also for the two very wide sources that ``resize_uint8`` would hand
    to Pillow -- writes Pillow's bytes into slot 1 of a [3, th, tw, 3] batch and leaves slots 0 and 2 alone."""
    (h, w), (th, tw) = shape
    plans_run.add(yimg.resize_plan(h, w, th, tw))
    for img in R.test_images(h, w):
        want = R.pillow_resize(img, th, tw)
        batch = torch.full((3, th, tw, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        out = yimg.resize_uint8_device(torch.from_numpy(img).to(DEV), th, tw, out=batch[1])
        assert out.data_ptr() == batch[1].data_ptr()
        got = batch.cpu().numpy()
        assert np.array_equal(got[1], want), f"{int((got[1] != want).sum())} of {want.size} bytes differ"
        assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all()


def test_both_plans_have_run(plans_run):
    assert plans_run == {1, 2}, plans_run


def test_resize_uint8_takes_host_and_device_images(built_lib):
    """The public entry: a host image is uploaded, a device image used in place; an aspect beyond 16 goes through Pillow and
    comes back on the device; a photograph-sized source lands on its 1024 bucket exactly."""
    for (h, w), (th, tw) in [((301, 203), (256, 256)), ((7, 300), (8, 32)), ((1500, 1125), (1152, 896))]:
        img = R.test_images(h, w)[0]
        want = R.pillow_resize(img, th, tw)
        host = yimg.resize_uint8(torch.from_numpy(img), th, tw, device=DEV)
        dev = yimg.resize_uint8(torch.from_numpy(img).to(DEV), th, tw)
        assert host.is_cuda and dev.is_cuda
        assert np.array_equal(host.cpu().numpy(), want) and np.array_equal(dev.cpu().numpy(), want)
