"""Prompts -> prompt embeddings on the HIP text encoders: SANA's Gemma-2 (yat_amd/gemma2.py; train_sana.py:84-94, :113-129,
common/trainer.py:307-308), PixArt-Sigma's T5 v1.1 (yat_amd/t5.py; train_pixart_sigma.py:68-74, :97-108) and SD3.5's CLIP-L +
OpenCLIP bigG + T5 (yat_amd/clip.py, yat_amd/t5.py; train_sd35.py:79-92, :113-118), the text half of the reference's feature
extraction and validation.  ``PIPE/text_encoder/config.json``'s ``model_type`` (``gemma2``, ``t5`` or ``clip_text_model``) picks
the encoder and its prompt rules.

    python -m yat_amd.encode_prompts --pipe PIPE [--empty OUT.pt] [--validation prompts.txt OUT.pt] [CAPTION.txt ...]

* ``CAPTION.txt ...``: writes ``STEM.emb.pt`` next to each ``STEM.txt``: the unpadded ``[L, C]`` bf16 rows the reference
  stores (train_sana.py:92-94) -- the sidecar ``python -m yat_amd.extract_latents`` reads;
* ``--empty OUT.pt``: ``extract_embeddings([""])``, a list with one ``[L, C]`` tensor (the trainer's ``empty_embeds.pt``);
* ``--validation prompts.txt OUT.pt``: one prompt per line -> the list of ``(prompt_embeds [1, 300, C], mask [1, 300],
  negative_embeds, negative_mask)`` tuples the trainer's ``validate()`` reads (``validation_embeds.pt``): the prompt with
  the complex human instruction, the negative prompt ``""`` without it (train_sana.py:113-129); a T5 pipe has no instruction.

The tokenizer is ``PIPE/tokenizer/tokenizer.json``, read with the ``tokenizers`` package; a T5 pipe that ships only
``PIPE/tokenizer/spiece.model`` (PixArt-Sigma does) is read with ``sentencepiece``.

An SD3.5 pipe (``text_encoder`` + ``text_encoder_2`` CLIP, ``text_encoder_3`` T5, ``tokenizer`` / ``_2`` / ``_3``) writes two files
per caption: ``STEM.emb.pt`` ``[333, 4096]`` and ``STEM.pooled.pt`` ``[2048]``, the two sidecars ``extract_latents`` reads.  A
``STEM.clip.txt`` beside ``STEM.txt``, when present, is the text the two CLIP encoders get (the reference feeds them
``compress_caption(caption)``, a spaCy model this build does not have: without the file CLIP gets the caption itself).
``--empty`` writes a list with the empty prompt's ``(prompt_embeds, pooled)`` pair and ``--validation`` the list of
``(prompt_embeds [1, 333, 4096], negative_prompt_embeds, pooled [1, 2048], negative_pooled)`` tuples.
"""
from __future__ import annotations

import argparse
import json
import os
from collections import namedtuple

import torch

from . import text_common
from .clip import CLIPTextEncoderHIP
from .gemma2 import Gemma2EncoderHIP
from .t5 import T5EncoderHIP

MAX_SEQUENCE_LENGTH = 300             # SanaPipeline.encode_prompt's max_sequence_length default

# The instruction the reference's validate() puts in front of every validation prompt (train_sana.py:113-122; the text SANA
# publishes for its pipeline).
COMPLEX_HUMAN_INSTRUCTION = [
    "Given a user prompt, generate an 'Enhanced prompt' that provides detailed visual descriptions suitable for image generation. Evaluate the level of detail in the user prompt:",
    "- If the prompt is simple, focus on adding specifics about colors, shapes, sizes, textures, and spatial relationships to create vivid and concrete scenes.",
    "- If the prompt is already detailed, refine and enhance the existing details slightly without overcomplicating.",
    "Here are examples of how to transform or refine prompts:",
    "- User Prompt: A cat sleeping -> Enhanced: A small, fluffy white cat curled up in a round shape, sleeping peacefully on a warm sunny windowsill, surrounded by pots of blooming red flowers.",
    "- User Prompt: A busy city street -> Enhanced: A bustling city street scene at dusk, featuring glowing street lamps, a diverse crowd of people in colorful clothing, and a double-decker bus passing by towering glass skyscrapers.",
    "Please generate only the enhanced description for the prompt below and avoid including any additional commentary or evaluations:",
    "User Prompt: ",
]


def load_tokenizer(tokenizer_dir: str):
    """``<tokenizer_dir>/tokenizer.json`` through the ``tokenizers`` package; its own padding / truncation are switched off
    (``tokenize_prompts`` applies the pipeline's)."""
    try:
        from tokenizers import Tokenizer
    except ImportError as e:
        raise ImportError("encoding prompts needs the `tokenizers` package (it reads <pipe>/tokenizer/tokenizer.json); without "
                          "it, train from cached embeddings") from e
    tok = Tokenizer.from_file(os.path.join(tokenizer_dir, "tokenizer.json"))
    tok.no_padding()
    tok.no_truncation()
    return tok


def tokenize_prompts(tokenizer, prompts, complex_human_instruction=None, max_sequence_length=MAX_SEQUENCE_LENGTH):
    """The prompt rules of diffusers ``SanaPipeline.encode_prompt`` / ``SanaPipeline._get_gemma_prompt_embeds`` [RECALL:
    restated from knowledge of upstream diffusers, which is not importable here]:

    * ``_text_preprocessing`` without ``clean_caption``: ``text.lower().strip()``;
    * with a complex human instruction: ``chi = "\\n".join(instruction)``, every prompt becomes ``chi + prompt`` and
      ``max_length_all = len(tokenizer.encode(chi)) + max_sequence_length - 2``; without: ``max_length_all =
      max_sequence_length``;
    * ``tokenizer(prompt, padding="max_length", max_length=max_length_all, truncation=True, add_special_tokens=True)``: the
      tokenizer's template supplies BOS, the ids are cut at ``max_length_all`` and padded on the right;
    * after the encoder: ``select_index = [0] + list(range(-max_sequence_length + 1, 0))`` on embeddings and mask
      (``select_rows``).

    -> (list of id lists without the padding, max_length_all)."""
    if isinstance(prompts, str):
        prompts = [prompts]
    texts = [p.lower().strip() for p in prompts]
    max_length_all = max_sequence_length
    if complex_human_instruction:
        chi = "\n".join(complex_human_instruction)
        texts = [chi + t for t in texts]
        max_length_all = len(tokenizer.encode(chi).ids) + max_sequence_length - 2
    return [list(tokenizer.encode(t).ids)[:max_length_all] for t in texts], max_length_all


def select_rows(emb: torch.Tensor, max_length_all: int, max_sequence_length=MAX_SEQUENCE_LENGTH):
    """``emb``: the ``[L, C]`` rows of one prompt's real tokens -> (``[max_sequence_length, C]``, mask ``[max_sequence_length]``
    int64): row 0, then the last ``max_sequence_length - 1`` rows of the sequence padded on the right to ``max_length_all``.
    A pad row comes back as zeros with mask 0 (the reference computes something there that the mask then hides)."""
    L = emb.shape[0]
    index = torch.tensor([0] + list(range(max_length_all - max_sequence_length + 1, max_length_all)))
    real = index < L
    out = torch.zeros(len(index), emb.shape[1], dtype=emb.dtype, device=emb.device)
    out[real.to(emb.device)] = emb[index[real].to(emb.device)]
    return out, real.to(torch.int64)


# ---------------------------------------------------------------------------------------- T5 (PixArt-Sigma) tokenizer rules
class T5Tokenizer:
    """T5's tokenizer rule over a sentencepiece model: ``tokenize(text, max_length)`` = the pieces cut to ``max_length - 1``,
    then EOS (the id of ``</s>``) -- what ``transformers.T5Tokenizer(text, max_length=..., truncation=True,
    add_special_tokens=True)`` returns before its padding.  The empty text is ``[eos]``."""

    def __init__(self, pieces, eos_id: int):
        self._pieces, self.eos_id = pieces, int(eos_id)

    def tokenize(self, text: str, max_length: int = MAX_SEQUENCE_LENGTH):
        return [int(i) for i in self._pieces(text)][:max_length - 1] + [self.eos_id]


def load_t5_tokenizer(tokenizer_dir: str) -> T5Tokenizer:
    """``<tokenizer_dir>/tokenizer.json`` through ``tokenizers`` when present (encoded without special tokens; EOS is appended
    here), else ``<tokenizer_dir>/spiece.model`` through ``sentencepiece``."""
    fast = os.path.join(tokenizer_dir, "tokenizer.json")
    if os.path.isfile(fast):
        try:
            from tokenizers import Tokenizer
        except ImportError as e:
            raise ImportError("encoding prompts needs the `tokenizers` package (it reads <pipe>/tokenizer/tokenizer.json); "
                              "without it, train from cached embeddings") from e
        tok = Tokenizer.from_file(fast)
        tok.no_padding()
        tok.no_truncation()
        eos = tok.token_to_id("</s>")
        if eos is None:
            raise ValueError(f"{fast}: no </s> token")
        return T5Tokenizer(lambda text: tok.encode(text, add_special_tokens=False).ids, eos)
    try:
        import sentencepiece
    except ImportError as e:
        raise ImportError("encoding prompts needs the `sentencepiece` package (it reads <pipe>/tokenizer/spiece.model); "
                          "without it, train from cached embeddings") from e
    sp = sentencepiece.SentencePieceProcessor(model_file=os.path.join(tokenizer_dir, "spiece.model"))
    eos = sp.piece_to_id("</s>")
    if eos == sp.unk_id():
        raise ValueError(f"{tokenizer_dir}/spiece.model: no </s> piece")
    return T5Tokenizer(lambda text: sp.encode(text), eos)


def tokenize_t5_prompts(tokenizer: T5Tokenizer, prompts, complex_human_instruction=None, max_sequence_length=MAX_SEQUENCE_LENGTH):
    """The prompt rules of diffusers ``PixArtSigmaPipeline.encode_prompt`` [RECALL: restated from knowledge of upstream
    diffusers, which is not importable here]:

    * ``_text_preprocessing`` without ``clean_caption``: ``text.lower().strip()``;
    * ``max_sequence_length = 300``;
    * ``tokenizer(text, padding="max_length", max_length=300, truncation=True, add_special_tokens=True)``: the pieces are cut
      to 299 and ``</s>`` closes them, then the ids are padded on the right with 0 (``pad_right``);
    * the encoder runs under the attention mask; with classifier-free guidance the negative prompt ``""`` is padded to the
      same 300.

    PixArt has no complex human instruction.  -> (list of id lists without the padding (the empty prompt is ``[eos]``),
    max_sequence_length)."""
    if complex_human_instruction:
        raise ValueError("PixArt-Sigma's prompt rules take no complex human instruction")
    if isinstance(prompts, str):
        prompts = [prompts]
    return [tokenizer.tokenize(p.lower().strip(), max_sequence_length) for p in prompts], max_sequence_length


def pad_right(emb: torch.Tensor, max_length_all: int):
    """``emb``: the ``[L, C]`` rows of one prompt's real tokens -> (``[max_length_all, C]``, mask ``[max_length_all]`` int64),
    padded on the right.  A pad row comes back as zeros with mask 0 (the reference computes something there that the mask
    then hides)."""
    L = emb.shape[0]
    out = torch.zeros(max_length_all, emb.shape[1], dtype=emb.dtype, device=emb.device)
    out[:L] = emb
    return out, (torch.arange(max_length_all) < L).to(torch.int64)


# ------------------------------------------------------------------------------------ SD3.5: CLIP-L + OpenCLIP bigG + T5
CLIP_LENGTH = 77                      # tokenizer_max_length of StableDiffusion3Pipeline
SD3_T5_LENGTH = 256                   # its max_sequence_length default
_CLIP_SPLIT = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""


class CLIPTokenizer:
    """CLIP's tokenizer rule over a byte-level BPE: ``tokenize(text)`` = ``[bos] + pieces[:max_length - 2] + [eos]`` padded on
    the right to ``max_length`` with ``pad_id`` -- what ``transformers.CLIPTokenizer(text, padding="max_length",
    max_length=77, truncation=True)`` returns.  The empty text is ``[bos, eos, pad, ...]``."""

    def __init__(self, pieces, bos_id: int, eos_id: int, pad_id: int):
        self._pieces, self.bos_id, self.eos_id, self.pad_id = pieces, int(bos_id), int(eos_id), int(pad_id)

    def tokenize(self, text: str, max_length: int = CLIP_LENGTH):
        ids = [self.bos_id] + [int(i) for i in self._pieces(text)][:max_length - 2] + [self.eos_id]
        return ids + [self.pad_id] * (max_length - len(ids))


def _token_text(value):
    """A special token as ``special_tokens_map.json`` / ``tokenizer_config.json`` store it: a string or {"content": ...}."""
    return value.get("content") if isinstance(value, dict) else value


def load_clip_tokenizer(tokenizer_dir: str) -> CLIPTokenizer:
    """``<tokenizer_dir>/tokenizer.json`` when present, else ``vocab.json`` + ``merges.txt`` (all SD3.5 ships for its two CLIP
    tokenizers), through the ``tokenizers`` package: a byte-level BPE with the end-of-word suffix ``</w>``, NFC normalisation,
    whitespace collapse, lowercasing, CLIP's split pattern and no prefix space (the construction of transformers'
    ``CLIPTokenizer``).  The pad token is the directory's own, from ``special_tokens_map.json`` or ``tokenizer_config.json``
    (CLIP-L's tokenizer pads with ``<|endoftext|>``, tokenizer_2 with ``!``); without either file: ``<|endoftext|>``."""
    try:
        from tokenizers import Regex, Tokenizer, normalizers, pre_tokenizers
        from tokenizers.models import BPE
    except ImportError as e:
        raise ImportError("encoding prompts needs the `tokenizers` package (it reads <pipe>/tokenizer/vocab.json + merges.txt); "
                          "without it, train from cached embeddings") from e
    fast = os.path.join(tokenizer_dir, "tokenizer.json")
    if os.path.isfile(fast):
        tok = Tokenizer.from_file(fast)
    else:
        tok = Tokenizer(BPE.from_file(os.path.join(tokenizer_dir, "vocab.json"), os.path.join(tokenizer_dir, "merges.txt"),
                                      continuing_subword_prefix="", end_of_word_suffix="</w>", fuse_unk=False,
                                      unk_token="<|endoftext|>"))
        tok.normalizer = normalizers.Sequence([normalizers.NFC(), normalizers.Replace(Regex(r"\s+"), " "), normalizers.Lowercase()])
        tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Split(Regex(_CLIP_SPLIT), behavior="removed", invert=True),
                                                     pre_tokenizers.ByteLevel(add_prefix_space=False)])
    tok.no_padding()
    tok.no_truncation()
    special = {"bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>", "pad_token": "<|endoftext|>"}
    for name in ("tokenizer_config.json", "special_tokens_map.json"):          # (the map, read last, wins)
        path = os.path.join(tokenizer_dir, name)
        if os.path.isfile(path):
            with open(path) as f:
                stored = json.load(f)
            special.update({k: _token_text(stored[k]) for k in special if _token_text(stored.get(k))})
    if not os.path.isfile(fast):
        # as transformers registers them: a special token written in the text is matched whole, before the BPE -- so under
        # tokenizer_2 an "!" in a caption becomes the pad token's id, not the piece "!</w>"
        tok.add_special_tokens(sorted(set(special.values())))
    ids = {k: tok.token_to_id(v) for k, v in special.items()}
    for k, v in ids.items():
        if v is None:
            raise ValueError(f"{tokenizer_dir}: the {k} {special[k]!r} is not in the vocabulary")
    return CLIPTokenizer(lambda text: tok.encode(text, add_special_tokens=False).ids, ids["bos_token"], ids["eos_token"],
                         ids["pad_token"])


def tokenize_sd3_prompts(tokenizers, prompts, complex_human_instruction=None, clip_prompts=None):
    """The prompt rules of diffusers ``StableDiffusion3Pipeline.encode_prompt`` [RECALL: restated from knowledge of upstream
    diffusers, which is not importable here]:

    * no ``lower().strip()``: the text goes to the tokenizers as it is (CLIP's own normaliser lowercases);
    * ``_get_clip_prompt_embeds``, for ``tokenizer`` and ``tokenizer_2`` alike: ``tokenizer(prompt, padding="max_length",
      max_length=77, truncation=True)`` = ``[bos] + pieces[:75] + [eos]`` padded on the right with the tokenizer's own pad
      token; all 77 ids are encoded (the model is causal and takes no mask) and ``hidden_states[-2]`` + ``text_embeds`` kept;
    * ``_get_t5_prompt_embeds``: ``tokenizer_3(prompt, padding="max_length", max_length=256, truncation=True,
      add_special_tokens=True)``: the pieces cut to 255, ``</s>``, padded on the right with id 0; the encoder gets NO
      attention mask, so the 256 ids with their pads are one prompt.

    ``clip_prompts``: the text for the two CLIP tokenizers when it differs from the T5 text (default: the prompt itself).
    SD3 has no complex human instruction.  -> ((CLIP-L ids, bigG ids, T5 ids), 77 + 256)."""
    if complex_human_instruction:
        raise ValueError("SD3's prompt rules take no complex human instruction")
    if isinstance(prompts, str):
        prompts = [prompts]
    clip_prompts = list(prompts) if clip_prompts is None else ([clip_prompts] if isinstance(clip_prompts, str) else list(clip_prompts))
    if len(clip_prompts) != len(prompts):
        raise ValueError(f"{len(clip_prompts)} CLIP prompt(s) for {len(prompts)} prompt(s)")
    tok_l, tok_g, tok_t5 = tokenizers
    t5 = [tok_t5.tokenize(p, SD3_T5_LENGTH) for p in prompts]
    t5 = [i + [0] * (SD3_T5_LENGTH - len(i)) for i in t5]
    return ([tok_l.tokenize(p, CLIP_LENGTH) for p in clip_prompts], [tok_g.tokenize(p, CLIP_LENGTH) for p in clip_prompts], t5), \
        CLIP_LENGTH + SD3_T5_LENGTH


def assemble_sd3(clip_l, clip_g, t5_rows):
    """``encode_prompt``'s assembly for one prompt [RECALL: as above], plain torch: ``clip_l`` / ``clip_g`` = (hidden_states[-2]
    [77, C], text_embeds [P]) of the two CLIP encoders, ``t5_rows`` [256, J] -> (``cat([pad(cat([l, g], -1), to J with zeros),
    t5], rows)`` [333, J], ``cat([pooled_l, pooled_g])`` [P_l + P_g])."""
    clip = torch.cat([clip_l[0], clip_g[0]], dim=-1)
    if clip.shape[-1] > t5_rows.shape[-1]:
        raise ValueError(f"the CLIP widths add to {clip.shape[-1]}, more than the T5 width {t5_rows.shape[-1]}")
    clip = torch.nn.functional.pad(clip, (0, t5_rows.shape[-1] - clip.shape[-1]))
    return torch.cat([clip, t5_rows.to(clip.dtype)], dim=0), torch.cat([clip_l[1], clip_g[1]], dim=-1)


class SD3TextEncodersHIP:
    """The three text encoders of an SD3.5 pipe (``CLIPTextEncoderHIP`` x 2, ``T5EncoderHIP``) and their three tokenizers.
    ``H`` is the width of a prompt row (T5's), ``pooled_dim`` that of the pooled vector.

    Stated deviation: the reference feeds the two CLIP encoders ``compress_caption(caption)`` (spaCy with a downloaded model,
    train_sd35.py:79-92), which is not restated here; ``encode_prompts(..., clip_prompts=...)`` takes the CLIP text separately
    and defaults to the caption itself."""
    model_type = "clip_text_model"

    def __init__(self, clip_l, clip_g, t5, tokenizers):
        self.clip_l, self.clip_g, self.t5, self.tokenizers = clip_l, clip_g, t5, tuple(tokenizers)
        self.H = t5.H
        self.pooled_dim = clip_l.projection_dim + clip_g.projection_dim
        if clip_l.H + clip_g.H > t5.H:
            raise ValueError(f"the CLIP widths {clip_l.H} + {clip_g.H} exceed the T5 width {t5.H}")

    @classmethod
    def from_pretrained(cls, pipe_dir: str, device="cuda"):
        dirs = find_text_dirs(pipe_dir, cls.model_type)
        if dirs is None:                     # (a lone CLIP text encoder is another pipeline's, SD1.5's for one)
            raise NotImplementedError(f"{pipe_dir!r}: text encoder model_type {cls.model_type!r} is built for an SD3.5 pipe only: "
                                      "text_encoder, text_encoder_2, text_encoder_3 (config.json) and tokenizer, tokenizer_2, "
                                      "tokenizer_3 must all be there")
        tokenizers = load_sd3_tokenizers(dirs[3])
        return cls(CLIPTextEncoderHIP.from_pretrained(dirs[0], device=device), CLIPTextEncoderHIP.from_pretrained(dirs[1], device=device),
                   T5EncoderHIP.from_pretrained(dirs[2], device=device), tokenizers)

    @property
    def layers(self):
        """None once freed, as an encoder's own ``layers``."""
        parts = [self.clip_l.layers, self.clip_g.layers, self.t5.layers]
        return None if any(p is None for p in parts) else [w for p in parts for w in p]

    def describe(self) -> str:
        return ("SD3.5 text encoders on HIP, prompt rows [77 CLIP + 256 T5, " f"{self.H}], pooled [{self.pooled_dim}]; the CLIP "
                "text defaults to the caption itself (the reference's compress_caption is not restated)\n  "
                + "\n  ".join(e.describe() for e in (self.clip_l, self.clip_g, self.t5)))

    def free(self) -> None:
        for e in (self.clip_l, self.clip_g, self.t5):
            e.free()

    def encode_prompts(self, prompts, clip_prompts=None, max_batch=None):
        """-> per prompt (prompt_embeds [333, H], pooled [pooled_dim]) on the encoders' device."""
        (ids_l, ids_g, ids_t5), _ = tokenize_sd3_prompts(self.tokenizers, prompts, None, clip_prompts)
        as_ids = lambda rows: [torch.tensor(i, dtype=torch.int64) for i in rows]          # noqa: E731
        out_l = self.clip_l.encode(as_ids(ids_l), max_batch=max_batch)
        out_g = self.clip_g.encode(as_ids(ids_g), max_batch=max_batch)
        out_t5 = self.t5.encode(as_ids(ids_t5), max_batch=max_batch)
        return [assemble_sd3(a, b, c) for a, b, c in zip(out_l, out_g, out_t5)]


def load_sd3_tokenizers(pipe_tokenizer_dir):
    """tokenizer, tokenizer_2, tokenizer_3 beside ``<pipe>/tokenizer``."""
    return (load_clip_tokenizer(pipe_tokenizer_dir), load_clip_tokenizer(pipe_tokenizer_dir + "_2"),
            load_t5_tokenizer(pipe_tokenizer_dir + "_3"))


# ------------------------------------------------------------------------------------------- one rule record per model_type
# encoder: the class; options: the ``load_encoder`` options it takes; tokenizer_files: what ``<pipe>/tokenizer`` may hold;
# load_tokenizer(dir); tokenize(tokenizer, prompts, instruction) -> (ids, max_length_all); pad(rows of one prompt,
# max_length_all) -> ([300, C], mask [300]); instruction: what validate() puts in front of a validation prompt, or None.
# ``clip_text_model`` is an SD3.5 pipe: its encoder is the three encoders together, its tokenizer the three tokenizers, and it
# pads nothing afterwards (every prompt is 77 + 256 rows); ``extract_embeddings`` / ``validation_embeddings`` return its pairs.
TextRules = namedtuple("TextRules", "encoder options tokenizer_files load_tokenizer tokenize pad instruction")
RULES = {
    "gemma2": TextRules(Gemma2EncoderHIP, ("softcap",), ("tokenizer.json",), load_tokenizer, tokenize_prompts, select_rows,
                        COMPLEX_HUMAN_INSTRUCTION),
    "t5": TextRules(T5EncoderHIP, (), ("tokenizer.json", "spiece.model"), load_t5_tokenizer, tokenize_t5_prompts, pad_right, None),
    "clip_text_model": TextRules(SD3TextEncodersHIP, (), ("tokenizer.json", "vocab.json"), load_sd3_tokenizers, tokenize_sd3_prompts,
                                 None, None),
}
SD3 = "clip_text_model"


def rules_for(encoder) -> TextRules:
    """The prompt rules of an encoder, by its ``model_type`` (absent: Gemma-2's)."""
    return RULES[getattr(encoder, "model_type", "gemma2")]


def extract_embeddings(encoder, tokenizer, captions, max_batch=None, clip_captions=None):
    """train_sana.py:84-94, train_pixart_sigma.py:68-74: ``encode_prompt`` without an instruction, then the mask-true rows of
    each prompt -- without an instruction those are the rows of its (truncated) tokens, so nothing is padded and selected
    first.

    An SD3.5 pipe (train_sd35.py:79-92) returns a list of ``(prompt_embeds [333, 4096], pooled [2048])`` pairs, the layout
    ``SD3Recipe.stack_embeddings`` and ``SD35Trainer.check_empty_embeddings`` take.  Stated deviation: the reference feeds the
    two CLIP encoders ``compress_caption(caption)`` (spaCy plus a downloaded model), which is not restated here;
    ``clip_captions`` takes the CLIP text separately and defaults to the caption itself."""
    if getattr(encoder, "model_type", None) == SD3:
        return encoder.encode_prompts(list(captions), clip_captions, max_batch=max_batch)
    if clip_captions is not None:
        raise ValueError("clip_captions applies to an SD3.5 pipe only")
    ids, _ = rules_for(encoder).tokenize(tokenizer, list(captions), None)
    return encoder.encode([torch.tensor(i, dtype=torch.int64) for i in ids], max_batch=max_batch)


def encode_prompt(encoder, tokenizer, prompts, complex_human_instruction=None, max_batch=None):
    """``pipe.encode_prompt(prompts, complex_human_instruction=..., do_classifier_free_guidance=False)`` -> (embeds ``[B, 300,
    C]`` bf16, mask ``[B, 300]`` int64), both on the encoder's device.  ``encoder.encode`` maps id tensors to ``[L, C]`` rows."""
    rules = rules_for(encoder)
    ids, max_length_all = rules.tokenize(tokenizer, prompts, complex_human_instruction)
    rows = encoder.encode([torch.tensor(i, dtype=torch.int64) for i in ids], max_batch=max_batch)
    picked = [rules.pad(r, max_length_all) for r in rows]
    return torch.stack([p[0] for p in picked]), torch.stack([p[1] for p in picked]).to(picked[0][0].device)


def validation_embeddings(encoder, tokenizer, prompts):
    """train_sana.py:124-129, train_pixart_sigma.py:97-108: per prompt ``pipe.encode_prompt(prompt)`` (SANA: with the complex
    human instruction) with classifier-free guidance on and the default negative prompt ``""`` -> a list of (prompt_embeds,
    mask, negative_embeds, negative_mask) on the CPU.  An SD3.5 pipe (train_sd35.py:113-118): (prompt_embeds [1, 333, 4096],
    negative_prompt_embeds, pooled [1, 2048], negative_pooled), the negative prompt ``""`` on all three encoders."""
    if getattr(encoder, "model_type", None) == SD3:
        (ne, npool), = encoder.encode_prompts([""])
        out = []
        for p in prompts:
            (pe, pool), = encoder.encode_prompts([p])
            out.append((pe[None].cpu(), ne[None].cpu().clone(), pool[None].cpu(), npool[None].cpu().clone()))
        return out
    out = []
    neg, neg_mask = encode_prompt(encoder, tokenizer, [""])
    for p in prompts:
        pe, pm = encode_prompt(encoder, tokenizer, [p], rules_for(encoder).instruction)
        out.append((pe.cpu(), pm.cpu(), neg.cpu().clone(), neg_mask.cpu().clone()))
    return out


def find_text_dirs(pipe_dir, kind):
    """(``<pipe>/text_encoder``, ``<pipe>/tokenizer``) for a ``gemma2`` or ``t5`` pipe, None when either is absent.  An SD3.5
    pipe (``clip_text_model``) needs all six: (text_encoder, text_encoder_2, text_encoder_3, tokenizer, tokenizer_2,
    tokenizer_3), the first two tokenizers with ``tokenizer.json`` or ``vocab.json`` + ``merges.txt``."""
    if kind != SD3:
        return text_common.find_text_dirs(pipe_dir, RULES.get(kind, RULES["gemma2"]).tokenizer_files)
    if not pipe_dir:
        return None
    at = lambda *names: os.path.join(pipe_dir, *names)                                    # noqa: E731
    te = [at("text_encoder" + sfx) for sfx in ("", "_2", "_3")]
    tk = [at("tokenizer" + sfx) for sfx in ("", "_2", "_3")]
    has_clip = all(os.path.isfile(os.path.join(d, "tokenizer.json"))
                   or all(os.path.isfile(os.path.join(d, n)) for n in ("vocab.json", "merges.txt")) for d in tk[:2])
    has_t5 = any(os.path.isfile(os.path.join(tk[2], n)) for n in RULES["t5"].tokenizer_files)
    if all(os.path.isfile(os.path.join(d, "config.json")) for d in te) and has_clip and has_t5:
        return tuple(te + tk)
    return None


def text_encoder_model_type(pipe_dir):
    """``model_type`` of ``<pipe>/text_encoder/config.json``; None without that file."""
    path = os.path.join(pipe_dir or "", "text_encoder", "config.json")
    if not os.path.isfile(path):
        return None
    with open(path) as f:
        return json.load(f).get("model_type")


def load_encoder(pipe_dir: str, device="cuda", softcap=True):
    """(encoder, tokenizer) of a pipeline directory: ``T5EncoderHIP`` with T5's tokenizer when ``text_encoder/config.json``
    says ``model_type`` ``t5`` (PixArt-Sigma; ``softcap`` does not apply), ``SD3TextEncodersHIP`` with its three tokenizers
    when it says ``clip_text_model`` (SD3.5), else ``Gemma2EncoderHIP`` (SANA)."""
    kind = text_encoder_model_type(pipe_dir) or "gemma2"
    if kind not in RULES:
        raise NotImplementedError(f"{pipe_dir!r}: text encoder model_type {kind!r} is not built (gemma2, t5 and clip_text_model "
                                  "are)")
    rules = RULES[kind]
    if kind == SD3:
        encoder = rules.encoder.from_pretrained(pipe_dir, device=device)
        return encoder, encoder.tokenizers
    dirs = find_text_dirs(pipe_dir, kind)
    if dirs is None:
        raise FileNotFoundError(f"{pipe_dir!r} holds no text_encoder/config.json + tokenizer/{' or '.join(rules.tokenizer_files)}")
    tokenizer = rules.load_tokenizer(dirs[1])
    options = {k: v for k, v in {"softcap": softcap}.items() if k in rules.options}
    return rules.encoder.from_pretrained(dirs[0], device=device, **options), tokenizer


def main(argv=None, loader=load_encoder) -> None:
    ap = argparse.ArgumentParser(prog="python -m yat_amd.encode_prompts",
                                 description="encode captions / prompts into prompt embeddings on the HIP text encoder of a SANA "
                                             "(Gemma-2), PixArt-Sigma (T5) or SD3.5 (CLIP-L + OpenCLIP bigG + T5) pipeline directory")
    ap.add_argument("--pipe", required=True, help="pipeline directory (text_encoder/ and tokenizer/)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--no-softcap", action="store_true", help="drop the attention soft cap (what transformers' SDPA path computes)")
    ap.add_argument("--empty", metavar="OUT.pt", help="write the empty prompt's embedding (empty_embeds.pt)")
    ap.add_argument("--validation", nargs=2, metavar=("PROMPTS.txt", "OUT.pt"), help="one prompt per line -> validation_embeds.pt")
    ap.add_argument("--batch", type=int, default=8, help="captions per encoder call")
    ap.add_argument("captions", nargs="*", help="STEM.txt caption files; STEM.emb.pt is written next to each (SD3.5: and "
                                               "STEM.pooled.pt; a STEM.clip.txt beside STEM.txt is the CLIP text)")
    a = ap.parse_args(argv)
    encoder, tokenizer = loader(a.pipe, device=a.device, softcap=not a.no_softcap)
    if hasattr(encoder, "describe"):
        print(encoder.describe())
    sd3 = getattr(encoder, "model_type", None) == SD3
    keep = lambda t: t.to(torch.bfloat16).cpu().clone()                                   # noqa: E731
    if a.captions:
        texts, clip_texts = [], []
        for path in a.captions:
            with open(path, encoding="utf-8") as f:
                texts.append(f.read())
            clip_path = os.path.splitext(path)[0] + ".clip.txt"
            clip_texts.append(texts[-1])
            if sd3 and os.path.isfile(clip_path):
                with open(clip_path, encoding="utf-8") as f:
                    clip_texts[-1] = f.read()
        embs = extract_embeddings(encoder, tokenizer, texts, max_batch=a.batch, clip_captions=clip_texts if sd3 else None)
        for path, emb in zip(a.captions, embs):
            stem = os.path.splitext(path)[0]
            for out, t in ((stem + ".emb.pt", emb[0]), (stem + ".pooled.pt", emb[1])) if sd3 else ((stem + ".emb.pt", emb),):
                torch.save(keep(t), out)
                print(f"{out}: {tuple(t.shape)}")
    if a.empty:
        emb = extract_embeddings(encoder, tokenizer, [""])
        torch.save([tuple(keep(t) for t in e) if sd3 else keep(e) for e in emb], a.empty)
        print(f"{a.empty}: {tuple(emb[0][0].shape) if sd3 else tuple(emb[0].shape)}")
    if a.validation:
        with open(a.validation[0], encoding="utf-8") as f:
            prompts = [line.rstrip("\n") for line in f if line.strip()]
        torch.save(validation_embeddings(encoder, tokenizer, prompts), a.validation[1])
        print(f"{a.validation[1]}: {len(prompts)} prompt(s)")


if __name__ == "__main__":
    main()
