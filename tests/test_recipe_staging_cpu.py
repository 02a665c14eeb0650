"""The staging arithmetic of the three recipes' device path (yat_amd/recipe.py ``_Layout``) over plain ``uint8`` tensors: no
GPU, no pinned memory.  Recorded launch plans hold the device addresses of the staged segments, so for one bucket shape the
fixed-size segments must not move when the captions' row count changes, and the buffer is sized once for the longest captions."""
import pytest
import torch

from yat_amd import ops
from yat_amd.recipe import PixArtRecipe, SanaRecipe, SD3Recipe, kv_work_pairs

B, T, C = 3, 128, 24
SHAPE = (B, 4, 6, 10)                 # one latent bucket
ROWS = (1, 77)                        # two row counts of that bucket (odd: the ragged segment's size is no multiple of 16)


def _text_recipe(cls):
    r = cls.__new__(cls)              # host arithmetic only: no model, no device
    r.pad_to = T
    return r


def _layouts(name, rows):
    if name == "sana":
        return _text_recipe(SanaRecipe)._layout(SHAPE, B, C, rows)
    if name == "pixart-host-noise":
        return _text_recipe(PixArtRecipe)._layout(SHAPE, B, C, rows, host_noise=True)
    if name == "pixart-device-noise":
        return _text_recipe(PixArtRecipe)._layout(SHAPE, B, C, rows, host_noise=False)
    return SD3Recipe._layout(SHAPE, (B, 10, 16), (B, 8), host_noise=name == "sd3-host-noise")


RECIPES = ["sana", "pixart-host-noise", "pixart-device-noise", "sd3-host-noise", "sd3-device-noise"]
NAMES = {"sana": ["lat", "noise", "off", "t", "sig", "work", "emb"], "pixart": ["lat", "noise", "off", "t", "a", "c", "work", "emb"],
         "sd3": ["lat", "noise", "prompt", "pooled", "t", "sig"]}


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("rows", ROWS)
def test_segments_are_aligned_disjoint_and_read_back_by_name(recipe, rows):
    lay = _layouts(recipe, rows)
    assert list(lay.spec) == NAMES[recipe.split("-")[0]]                         # the declaration order is the buffer order
    end = 0
    for name, (o, n, dtype, shape) in lay.spec.items():
        assert o % 16 == 0 and o >= end, name                                     # 16-byte aligned, no overlap
        end = o + n
    assert end <= lay.total <= lay.capacity and lay.total % 16 == 0
    buf = torch.zeros(lay.total, dtype=torch.uint8)
    host = lay.views(buf)
    for k, (name, v) in enumerate(host.items()):                                 # a distinct value per segment
        assert v.shape == lay.spec[name][3] and v.dtype == lay.spec[name][2]
        v.fill_(k + 1)
    landed = lay.views(buf.clone())                                              # what the one copy delivers
    for k, (name, v) in enumerate(landed.items()):
        assert (v == k + 1).all(), name
    assert landed["lat"].shape == SHAPE and landed["noise"].numel() == (0 if "device-noise" in recipe else landed["lat"].numel())


@pytest.mark.parametrize("recipe", RECIPES[:3])
def test_fixed_segments_stay_put_and_capacity_covers_the_longest_captions(recipe):
    short, long_, full = (_layouts(recipe, rows) for rows in (*ROWS, B * T))
    assert list(short.spec)[-1] == "emb"                                         # the ragged segment is last
    for name in list(short.spec)[:-1]:
        assert short.spec[name] == long_.spec[name] == full.spec[name], name     # offset, size, dtype, shape
    assert short.spec["emb"][0] == long_.spec["emb"][0] == full.spec["emb"][0]
    one = _layouts(recipe, 1)
    assert one.capacity >= full.total and one.capacity == one.total + 2 * (B * T - 1) * C
    assert full.capacity == full.total


def test_work_list_rule_for_empty_captions():
    """SANA's device path lists no key tile for an empty caption; PixArt-Sigma's lists all T padding rows (the padded layout
    attends to them), which is also ``ops.kv_work_list``'s rule.  The two rules differ for empty captions only."""
    lens, T_ = [0, 1, 64, 65], 128
    sana, pixart = kv_work_pairs(lens, T_, empty_attends_all=False), kv_work_pairs(lens, T_, empty_attends_all=True)
    per_image = lambda pairs: [sum(1 for b, _ in pairs if b == i) for i in range(len(lens))]
    assert per_image(sana) == [0, 1, 1, 2] and per_image(pixart) == [2, 1, 1, 2]
    want = [tuple(p) for p in ops.kv_work_list(lens, T_, "cpu").tolist()]
    assert pixart == want
    assert sana == [p for p in want if lens[p[0]] > 0]


@pytest.mark.parametrize("cls,empty_attends_all,lens", [(SanaRecipe, False, [5, 64, 17]), (PixArtRecipe, True, [0, 65, 9]),
                                                        (PixArtRecipe, True, [0, 0, 0])])
def test_ragged_text_lands_in_its_segments(cls, empty_attends_all, lens):
    """``_stage_text`` over a plain buffer: offsets, the work list in the front of its fixed-size segment, the rows one after
    the other (nothing to pack when every caption is empty)."""
    r = _text_recipe(cls)
    g = torch.Generator().manual_seed(0)
    embs = [torch.randn(L, C, generator=g).to(torch.bfloat16) for L in lens]
    lay = r._layout(SHAPE, B, C, sum(lens))
    buf = torch.full((lay.capacity,), 0xAB, dtype=torch.uint8)
    npairs = r._stage_text(lay.views(buf), embs, lens, empty_attends_all)
    got = lay.views(buf.clone())
    assert got["off"].tolist() == [0, lens[0], lens[0] + lens[1], sum(lens)]
    want = kv_work_pairs(lens, T, empty_attends_all)
    assert npairs == len(want) <= got["work"].shape[0] and [tuple(p) for p in got["work"][:npairs].tolist()] == want
    assert torch.equal(got["emb"], torch.cat(embs))
