"""Torch-CPU restatement of the SANA-1.5 transformer (test-only): ``oracle.sana_ref`` with
``qk_norm="rms_norm_across_heads"``.

[RECALL] diffusers, not importable here: ``SanaTransformer2DModel(..., qk_norm="rms_norm_across_heads")`` hands the setting to
every ``Attention`` of every block, whose constructor then builds ``norm_q = RMSNorm(heads * dim_head, eps=1e-5)`` and
``norm_k = RMSNorm(kv_heads * dim_head, eps=1e-5)`` (affine, weight only).  Both processors -- ``SanaLinearAttnProcessor2_0`` on
attn1, ``AttnProcessor2_0`` (SDPA) on attn2 and on the attn1 of a block in ``modified_blocks`` -- do
``query = attn.norm_q(attn.to_q(x))`` and ``key = attn.norm_k(attn.to_k(.))`` on the [B, rows, D] projections (attn2's biases
included), before the head split, before the ReLU of linear attention and before the softmax scale; ``value`` is untouched and
attn2's ``norm_k`` runs on the text rows.  The RMSNorm arithmetic is the class ``caption_norm`` uses
(``oracle.sana_ref.RMSNorm``): mean of squares and rsqrt in fp32, ``x * rstd`` rounded to the weight's dtype, times the weight.

Only the three attention methods are re-stated (with the two norms in place); everything else is the oracle's.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.sana_ref import RMSNorm, SanaBlock, SanaConfig, SanaTransformerRef, _CrossAttn, _SelfAttn

QK_EPS = 1e-5


class SelfAttn15(_SelfAttn):
    def __init__(self, dim, heads, head_dim, bias=False):
        super().__init__(dim, heads, head_dim, bias=bias)
        self.norm_q = RMSNorm(heads * head_dim, eps=QK_EPS)
        self.norm_k = RMSNorm(heads * head_dim, eps=QK_EPS)

    def linear_attention(self, x):
        """[RECALL] SanaLinearAttnProcessor2_0 with attn.norm_q / attn.norm_k set."""
        dt = x.dtype
        q, k, v = self.norm_q(self.to_q(x)), self.norm_k(self.to_k(x)), self.to_v(x)
        q = q.transpose(1, 2).unflatten(1, (self.heads, -1))                  # [B,H,C,N]
        k = k.transpose(1, 2).unflatten(1, (self.heads, -1)).transpose(2, 3)  # [B,H,N,C]
        v = v.transpose(1, 2).unflatten(1, (self.heads, -1))                  # [B,H,C,N]
        q, k = F.relu(q), F.relu(k)
        q, k, v = q.float(), k.float(), v.float()
        v = F.pad(v, (0, 0, 0, 1), mode="constant", value=1.0)                # [B,H,C+1,N]
        scores = torch.matmul(v, k)                                           # [B,H,C+1,C]
        o = torch.matmul(scores, q)                                           # [B,H,C+1,N]
        o = o[:, :, :-1] / (o[:, :, -1:] + 1e-15)
        o = o.flatten(1, 2).transpose(1, 2).to(dt)                            # [B,N,D]
        return self.to_out[0](o)

    def softmax_attention(self, x):
        """[RECALL] AttnProcessor2_0 with attn.norm_q / attn.norm_k set (blocks in ``modified_blocks``)."""
        B, N, _ = x.shape
        q = self.norm_q(self.to_q(x)).view(B, N, self.heads, self.head_dim).transpose(1, 2)
        k = self.norm_k(self.to_k(x)).view(B, N, self.heads, self.head_dim).transpose(1, 2)
        v = self.to_v(x).view(B, N, self.heads, self.head_dim).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v)
        return self.to_out[0](o.transpose(1, 2).reshape(B, N, -1))


class CrossAttn15(_CrossAttn):
    def __init__(self, dim, cross_dim, heads, head_dim):
        super().__init__(dim, cross_dim, heads, head_dim)
        self.norm_q = RMSNorm(heads * head_dim, eps=QK_EPS)
        self.norm_k = RMSNorm(heads * head_dim, eps=QK_EPS)

    def forward(self, x, enc, bias):
        B, N, _ = x.shape
        T = enc.shape[1]
        q = self.norm_q(self.to_q(x)).view(B, N, self.heads, self.head_dim).transpose(1, 2)
        k = self.norm_k(self.to_k(enc)).view(B, T, self.heads, self.head_dim).transpose(1, 2)
        v = self.to_v(enc).view(B, T, self.heads, self.head_dim).transpose(1, 2)
        mask = None if bias is None else bias[:, None, :, :].expand(B, self.heads, 1, T)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        return self.to_out[0](o.transpose(1, 2).reshape(B, N, -1))


class SanaBlock15(SanaBlock):
    def __init__(self, cfg: SanaConfig, softmax_self_attn: bool):
        super().__init__(cfg, softmax_self_attn)
        D = cfg.inner_dim
        self.attn1 = SelfAttn15(D, cfg.num_attention_heads, cfg.attention_head_dim)
        self.attn2 = CrossAttn15(D, cfg.cross_attention_dim, cfg.num_cross_attention_heads, cfg.cross_attention_head_dim)


class SanaTransformer15Ref(SanaTransformerRef):
    qk_norm = "rms_norm_across_heads"

    def __init__(self, cfg: SanaConfig):
        super().__init__(cfg)
        self.transformer_blocks = nn.ModuleList(
            [SanaBlock15(cfg, i in cfg.modified_blocks) for i in range(cfg.num_layers)])


def init_like_pretrained15(model: SanaTransformerRef, seed: int = 0) -> None:
    """``oracle.sana_ref.init_like_pretrained`` with every norm weight -- caption_norm, norm_q, norm_k -- drawn as
    1 + 0.1 * randn: all-ones norm weights would hide a missing or swapped weight."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(("caption_norm.weight", "norm_q.weight", "norm_k.weight")):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif "scale_shift_table" in name:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5 + (0.5 if p.shape[0] == 6 else 0.0))
            elif p.ndim == 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel()))


def hip_config(rcfg: SanaConfig, qk_norm="rms_norm_across_heads"):
    """The device model's config for the oracle config ``rcfg`` (which has no ``qk_norm`` attribute of its own)."""
    from yat_amd.sana import SanaConfig as HipCfg
    return HipCfg(**{k: getattr(rcfg, k) for k in HipCfg.__dataclass_fields__}, qk_norm=qk_norm)
