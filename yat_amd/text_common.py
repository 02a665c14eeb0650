"""What the HIP text encoders share (yat_amd/gemma2.py, yat_amd/t5.py): finding the pipeline's directories, reading the
safetensors files, and the packed-prompt runner -- ``encode`` lays the prompts' token ids end to end as the rows of one matrix,
computes no pad row and hands each prompt its rows back.  A model module keeps what is its own: the config checks, the
expected keys, the weight packing, its table (rotary or relative bias) and the op sequence of a forward.
"""
from __future__ import annotations

import json
import os
from collections import namedtuple

import torch

from .vae_common import BF16

# One chunk of prompts laid end to end: ``ids`` int32 [rows] and ``off_d`` int32 [B + 1] on the device, ``off`` int64 [B + 1]
# on the host (prompt b is rows off[b]:off[b + 1]), ``lens`` the B lengths, ``rows`` their sum.
PromptPack = namedtuple("PromptPack", "ids off off_d lens rows")


def find_text_dirs(pretrained_pipe_path, tokenizer_files):
    """(``<pipe>/text_encoder``, ``<pipe>/tokenizer``) when the first holds a config.json and the second one of
    ``tokenizer_files``, else None."""
    if not pretrained_pipe_path:
        return None
    te, tk = os.path.join(pretrained_pipe_path, "text_encoder"), os.path.join(pretrained_pipe_path, "tokenizer")
    if os.path.isfile(os.path.join(te, "config.json")) and any(os.path.isfile(os.path.join(tk, n)) for n in tokenizer_files):
        return te, tk
    return None


def read_text_encoder_tensors(te_dir: str, rename=None) -> dict:
    """{key: tensor} of ``<te_dir>/model.safetensors`` or of the shards ``model.safetensors.index.json`` names.  ``rename`` maps
    a stored key to the key kept, or to None to drop the tensor unread."""
    from safetensors import safe_open
    index = os.path.join(te_dir, "model.safetensors.index.json")
    if os.path.isfile(index):
        with open(index) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
    else:
        files = ["model.safetensors"]
    sd = {}
    for name in files:
        with safe_open(os.path.join(te_dir, name), framework="pt") as f:
            for k in f.keys():
                kk = rename(k) if rename else k
                if kk is not None:
                    sd[kk] = f.get_tensor(k)
    return sd


class TextEncoderHIP:
    """Host side of one text encoder in bf16 on the HIP kernels: the packed weights on the device and the activation buffers
    of the largest call.  A subclass sets ``load_text_encoder_dir`` (directory -> (cfg, tensors)) as a static method and the
    two class attributes below; its ``__init__`` sets ``H`` (the width of an embedding row), ``max_prompt``, ``embed``
    ``[vocab, H]`` and ``layers``, and it supplies ``_buffer_widths()``, ``_forward(pack, bufs, y)`` and ``describe()``."""
    EMPTY_HINT = ""               # why the tokenizer never yields an empty id sequence
    MAX_PROMPT_RULE = ""          # where ``max_prompt`` comes from

    def __init__(self, cfg: dict, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        self._bufs = None

    def dev(self, t):
        return t.to(self.device, BF16).contiguous()

    @classmethod
    def from_pretrained(cls, te_dir: str, device="cuda", **kwargs):
        cfg, sd = cls.load_text_encoder_dir(te_dir)
        return cls(cfg, sd, device, **kwargs)

    def free(self) -> None:
        """Drop the weights and buffers (the trainer's validate() after its prompts are encoded)."""
        for k, v in list(vars(self).items()):
            if torch.is_tensor(v):
                setattr(self, k, None)
        self.layers = self._bufs = None

    def _buffers(self, rows: int):
        if self._bufs is not None and self._bufs[0] >= rows:
            return self._bufs[1]
        self._bufs = None
        cap = (rows + 63) // 64 * 64
        bufs = {k: torch.empty(cap, n, dtype=BF16, device=self.device) for k, n in self._buffer_widths().items()}
        self._bufs = (cap, bufs)
        return bufs

    @torch.no_grad()
    def encode(self, prompts, max_batch=None):
        """``prompts``: a list of 1-D integer id tensors -> a list of ``[L_i, H]`` bf16 tensors on the device."""
        if self.layers is None:
            raise RuntimeError("the encoder's weights were freed")
        prompts = [torch.as_tensor(p).reshape(-1).to("cpu", torch.int64) for p in prompts]
        vocab = self.embed.shape[0]
        for p in prompts:
            if p.numel() == 0:
                raise ValueError(f"an empty id sequence cannot be encoded ({self.EMPTY_HINT})")
            if p.numel() > self.max_prompt:
                raise NotImplementedError(f"a prompt of {p.numel()} tokens is beyond the {self.max_prompt} this encoder is built "
                                          f"for ({self.MAX_PROMPT_RULE})")
            if int(p.min()) < 0 or int(p.max()) >= vocab:
                raise ValueError(f"token id outside the vocabulary [0, {vocab})")
        step = int(max_batch) if max_batch else len(prompts)
        out = []
        for i in range(0, len(prompts), max(step, 1)):
            out += self._encode_chunk(prompts[i:i + step])
        return out

    def _encode_chunk(self, prompts):
        lens = [p.numel() for p in prompts]
        rows, B = sum(lens), len(prompts)
        off = torch.zeros(B + 1, dtype=torch.int64)
        off[1:] = torch.tensor(lens).cumsum(0)
        ids = torch.cat(prompts).to(torch.int32).to(self.device)
        pack = PromptPack(ids, off, off.to(torch.int32).to(self.device), lens, rows)
        bufs = {k: v[:rows] for k, v in self._buffers(rows).items()}
        y = torch.empty(rows, self.H, dtype=BF16, device=self.device)
        self._forward(pack, bufs, y)
        return [y[int(off[b]):int(off[b + 1])] for b in range(B)]
