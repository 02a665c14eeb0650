"""The properties test_prefill_attn_exact_gpu.py rests on, proven on the CPU from tests/prefill_attn_ref.py: raw scores are
exact fp32 integers, the winners tie and everybody else lies more than the bound below them after each kernel's logit
transform (fp64, with margin), l is a power of two, the expected outputs are exact in bf16 or rounded once from an exact fp32
value, and the case lists reach every instantiation, length class and step of the lazy rescale."""
import math

import numpy as np
import pytest
import torch

from tests import prefill_attn_ref as R

BF = torch.bfloat16
MARGIN = 200.0                    # log2 units between the winners and everybody else: the bound is R.GAP_BOUND = 134


def _pow2(x):
    return x > 0 and math.frexp(x)[0] == 0.5


@pytest.mark.parametrize("spec", R.CASES, ids=R.case_id)
def test_case_is_exact(spec):
    c, ref, written = R.case(spec)
    dh = spec.dh
    # products and every partial sum of a score are integers below 2^24: exact in fp32 in any order
    assert torch.equal(c["q"], c["q"].round()) and torch.equal(c["k"], c["k"].round())
    assert float(c["q"].view(-1, spec.H, dh).abs().sum(-1).max() * c["k"].abs().max()) < 2 ** 24
    live = 0
    for (b, h, raw, bias, v), (_, _, t, _) in zip(R.raw_scores(c), R.masked_logits(c)):
        assert torch.equal(raw, raw.round()) and float(raw.abs().max()) < 2 ** 24
        live += 1
        top = t.max(-1, keepdim=True).values
        rel = t - top
        if spec.mode in ("sel", "bias"):
            win = rel == 0
            n = win.sum(-1)
            assert bool(((n == 1) | (n == 2) | (n == 4)).all()), (b, h)
            if spec.mode == "bias":
                assert bool((n <= 2).all())
            assert float(rel[~win].max() if (~win).any() else -math.inf) < -MARGIN, (b, h)
            # equal raw scores (and equal bias): the tie is exact under any transform
            key = raw if bias is None else raw * 4096 + bias
            assert all(len(set(key[i][win[i]].tolist())) == 1 for i in range(t.shape[0]))
            if spec.kind == "vae":
                # exp2(fma(s, ce, -(m ce))) of a winner: the residue of the rounded product is far inside bf16's half-ulp of 1
                ce = np.float32(R.scale_of(spec)) * R.LOG2E_F
                m = np.float32(raw.max())
                resid = float(m) * float(ce) - float(np.float32(m * ce))
                assert abs(resid) < 2.0 ** -12
        else:
            near = rel > -40
            assert float(rel[~near].max() if (~near).any() else -math.inf) < -MARGIN - 16, (b, h)
            assert torch.equal(rel[near], rel[near].round()) and float(rel[near].min()) >= -14
            l = torch.where(near, torch.exp2(rel), torch.zeros_like(rel)).sum(-1)
            assert all(_pow2(x) for x in l.tolist()), (b, h)
    assert live == sum(1 for x in c["eff"] if x) * spec.H
    out = ref[written]
    assert bool(torch.isfinite(out).all()) and bool(torch.isnan(ref[~written]).all())
    if spec.mode in ("sel", "bias"):
        e = out.to(BF).double()                              # exact in bf16 (up to what fp64 keeps of the losers: < 2^-200)
        assert torch.equal(e * 4, (e * 4).round()) and float(e.abs().max()) <= 8 and float((e - out).abs().max()) < 1e-60
    else:
        e = out.float().double()                             # exact in fp32 (at most 20 bits): rounded once
        assert torch.equal(e * 2 ** 16, (e * 2 ** 16).round()) and float((e - out).abs().max()) < 1e-60
    assert (out != 0).double().mean() > 0.5                                 # dense v: most columns of every row speak


def test_soft_cap_keeps_the_gap():
    """The capped logit, from the formula in fp64: winners to everybody else is beyond the bound with margin, and with
    negative winners a phantom zero key would beat them by more than the lazy threshold."""
    for spec in R.CASES:
        if spec.kind == "gemma" and spec.cap > 0:
            Aq, kc1, q2, kc2 = R.amplitudes(spec)
            w = Aq * (8 + kc1) + q2 * kc2
            nxt = w - 2 * Aq
            s = R.scale_of(spec)
            tw, tn = (spec.cap * math.tanh(x * s / spec.cap) * R.LOG2E for x in (w, nxt))
            assert tw - tn > MARGIN, (spec, tw, tn)
            if spec.sign < 0:
                assert tw < -R.LAZY_LOG2 - 8


def test_case_lists_reach_every_class():
    by_kind = {}
    for spec in R.CASES:
        by_kind.setdefault(spec.kind, []).append(spec)
    # VAE: both head dims, every N, both signs, B = 1 and 3
    vae = by_kind["vae"]
    assert {(s.dh, s.lens[0]) for s in vae} == {(dh, N) for dh in (64, 512) for N in R.VAE_N}
    assert {(s.dh, s.sign) for s in vae} == {(64, 1), (64, -1), (512, 1), (512, -1)}
    assert {len(s.lens) for s in vae} == {1, 3}
    feats = set().union(*(R.walk(s) for s in vae))
    assert {"last_tile_masked", "last_tile_full", "dead_strip", "ragged_strip", "stages_1", "stages_2", "stages_3"} <= feats
    # Gemma: every instantiation, each with both caps, both signs, every length, every tile class
    gemma = by_kind["gemma"]
    assert {R.gemma_instance(s.H, s.Hkv) for s in gemma} == set(R.GEMMA_INSTANCES)
    assert R.gemma_instance(4, 4) == R.gemma_instance(3, 3) == (4, 1)
    for inst in R.GEMMA_INSTANCES:
        mine = [s for s in gemma if R.gemma_instance(s.H, s.Hkv) == inst]
        assert {(s.cap > 0, s.sign) for s in mine if s.mode == "sel"} == {(False, 1), (False, -1), (True, 1), (True, -1)}
        assert any(s.mode == "ladder" for s in mine)
        assert set(R.GEMMA_LENS) <= {x for s in mine for x in s.lens}
        feats = set().union(*(R.walk(s) for s in mine))
        assert {"half_skipped", "diag_in_half_0", "diag_in_half_1", "stages_1", "stages_2", "stages_3", "tile_exits",
                "empty_prompt", "cut_by_max_len", "ragged_strip"} <= feats, (inst, feats)
        if inst[0] // inst[1] > 1:
            assert "dead_strip" in feats
    assert {R.query_tile(s) for s in gemma} == {16, 32, 64}
    # T5 and CLIP: every length, H = 1 and 3, the prompt's end in either half and on a tile edge, dead strips, empty tiles
    for kind in ("t5", "clip"):
        mine = by_kind[kind]
        assert {s.H for s in mine} == {1, 3}
        assert set(R.TEXT_LENS) <= {x for s in mine for x in s.lens}
        feats = set().union(*(R.walk(s) for s in mine))
        want = {"dead_strip", "ragged_strip", "tile_exits", "empty_prompt", "cut_by_max_len", "stages_1", "stages_2", "stages_3"}
        want |= {"end_on_edge", "end_in_half_0", "end_in_half_1"} if kind == "t5" else {"half_skipped", "diag_in_half_1"}
        assert want <= feats, (kind, feats)
        # an empty prompt first, in the middle and last
        zero_at = {("first" if i == 0 else "last" if i == len(s.lens) - 1 else "middle") for s in mine
                   for i, x in enumerate(s.lens) if x == 0}
        assert zero_at == {"first", "middle", "last"}
        assert any(s.max_len > max(s.lens) for s in mine) and any(s.max_len < max(s.lens) for s in mine)
    # T5's bias-only cases: both directions, |d| >= 64 and d = +-(len - 1), a table per head, max_len above the longest prompt
    bias = [s for s in by_kind["t5"] if s.mode == "bias"]
    ds = {d for s in bias for d in s.dist}
    assert any(d >= 64 for d in ds) and any(d <= -64 for d in ds) and {1, -1} <= ds
    assert any(max(s.dist) == max(min(x, s.max_len) for x in s.lens) - 1 for s in bias)
    assert any(min(s.dist) == -(max(min(x, s.max_len) for x in s.lens) - 1) for s in bias)
    assert any(s.max_len > max(s.lens) for s in bias) and any(len(set(s.dist)) == 3 for s in bias)


def test_ladder_cases_meet_every_step_of_the_lazy_rescale():
    kinds = {"gemma": set(), "clip": set()}
    for spec in R.CASES:
        if spec.mode == "ladder":
            c, _, _ = R.case(spec)
            for _, _, t, _ in R.masked_logits(c):
                kinds[spec.kind] |= R.lazy_walk(t)
    for kind, got in kinds.items():
        assert {("P", e) for e in range(1, 9)} <= got, kind                  # P = 2^1 .. 2^8 without a rescale
        assert ("eight",) in got and ("lone",) in got, kind                  # exactly 8: no rescale; one query forces its strip
        assert ("alpha", 0) in got and any(("alpha", j) in got for j in range(1, 9)), kind
        assert any(k[0] == "stay" for k in got), kind


def test_reference_is_plain_attention():
    """the reference against torch's own softmax on a case's logits (natural units), and its isolation: rows of no live
    query stay NaN"""
    spec = next(s for s in R.CASES if s.kind == "t5" and s.mode == "sel" and s.H == 3)
    c, ref, written = R.case(spec)
    for b, h, t, v in R.masked_logits(c):
        want = torch.softmax(t * math.log(2.0), -1) @ v
        r0 = c["off"][b]
        got = ref[r0:r0 + t.shape[0], h * spec.dh:(h + 1) * spec.dh]
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
