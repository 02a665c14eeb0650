"""Prompts -> prompt embeddings on the HIP text encoders: SANA's Gemma-2 (yat_amd/gemma2.py; train_sana.py:84-94, :113-129,
common/trainer.py:307-308) and PixArt-Sigma's T5 v1.1 (yat_amd/t5.py; train_pixart_sigma.py:68-74, :97-108), the text half of the
reference's feature extraction and validation.  ``PIPE/text_encoder/config.json``'s ``model_type`` (``gemma2`` or ``t5``) picks
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
"""
from __future__ import annotations

import argparse
import json
import os
from collections import namedtuple

import torch

from . import text_common
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


# ------------------------------------------------------------------------------------------- one rule record per model_type
# encoder: the class; options: the ``load_encoder`` options it takes; tokenizer_files: what ``<pipe>/tokenizer`` may hold;
# load_tokenizer(dir); tokenize(tokenizer, prompts, instruction) -> (ids, max_length_all); pad(rows of one prompt,
# max_length_all) -> ([300, C], mask [300]); instruction: what validate() puts in front of a validation prompt, or None.
TextRules = namedtuple("TextRules", "encoder options tokenizer_files load_tokenizer tokenize pad instruction")
RULES = {
    "gemma2": TextRules(Gemma2EncoderHIP, ("softcap",), ("tokenizer.json",), load_tokenizer, tokenize_prompts, select_rows,
                        COMPLEX_HUMAN_INSTRUCTION),
    "t5": TextRules(T5EncoderHIP, (), ("tokenizer.json", "spiece.model"), load_t5_tokenizer, tokenize_t5_prompts, pad_right, None),
}


def rules_for(encoder) -> TextRules:
    """The prompt rules of an encoder, by its ``model_type`` (absent: Gemma-2's)."""
    return RULES[getattr(encoder, "model_type", "gemma2")]


def extract_embeddings(encoder, tokenizer, captions, max_batch=None):
    """train_sana.py:84-94, train_pixart_sigma.py:68-74: ``encode_prompt`` without an instruction, then the mask-true rows of
    each prompt -- without an instruction those are the rows of its (truncated) tokens, so nothing is padded and selected
    first."""
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
    mask, negative_embeds, negative_mask) on the CPU."""
    out = []
    neg, neg_mask = encode_prompt(encoder, tokenizer, [""])
    for p in prompts:
        pe, pm = encode_prompt(encoder, tokenizer, [p], rules_for(encoder).instruction)
        out.append((pe.cpu(), pm.cpu(), neg.cpu().clone(), neg_mask.cpu().clone()))
    return out


def find_text_dirs(pipe_dir, kind):
    """(``<pipe>/text_encoder``, ``<pipe>/tokenizer``) for a ``gemma2`` or ``t5`` pipe, None when either is absent."""
    return text_common.find_text_dirs(pipe_dir, RULES.get(kind, RULES["gemma2"]).tokenizer_files)


def text_encoder_model_type(pipe_dir):
    """``model_type`` of ``<pipe>/text_encoder/config.json``; None without that file."""
    path = os.path.join(pipe_dir or "", "text_encoder", "config.json")
    if not os.path.isfile(path):
        return None
    with open(path) as f:
        return json.load(f).get("model_type")


def load_encoder(pipe_dir: str, device="cuda", softcap=True):
    """(encoder, tokenizer) of a pipeline directory: ``T5EncoderHIP`` with T5's tokenizer when ``text_encoder/config.json``
    says ``model_type`` ``t5`` (PixArt-Sigma; ``softcap`` does not apply), else ``Gemma2EncoderHIP`` (SANA)."""
    kind = text_encoder_model_type(pipe_dir) or "gemma2"
    if kind not in RULES:
        raise NotImplementedError(f"{pipe_dir!r}: text encoder model_type {kind!r} is not built (gemma2 and t5 are)")
    rules = RULES[kind]
    dirs = find_text_dirs(pipe_dir, kind)
    if dirs is None:
        raise FileNotFoundError(f"{pipe_dir!r} holds no text_encoder/config.json + tokenizer/{' or '.join(rules.tokenizer_files)}")
    tokenizer = rules.load_tokenizer(dirs[1])
    options = {k: v for k, v in {"softcap": softcap}.items() if k in rules.options}
    return rules.encoder.from_pretrained(dirs[0], device=device, **options), tokenizer


def main(argv=None, loader=load_encoder) -> None:
    ap = argparse.ArgumentParser(prog="python -m yat_amd.encode_prompts",
                                 description="encode captions / prompts into prompt embeddings on the HIP text encoder of a SANA "
                                             "(Gemma-2) or PixArt-Sigma (T5) pipeline directory")
    ap.add_argument("--pipe", required=True, help="pipeline directory (text_encoder/ and tokenizer/)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--no-softcap", action="store_true", help="drop the attention soft cap (what transformers' SDPA path computes)")
    ap.add_argument("--empty", metavar="OUT.pt", help="write the empty prompt's embedding (empty_embeds.pt)")
    ap.add_argument("--validation", nargs=2, metavar=("PROMPTS.txt", "OUT.pt"), help="one prompt per line -> validation_embeds.pt")
    ap.add_argument("--batch", type=int, default=8, help="captions per encoder call")
    ap.add_argument("captions", nargs="*", help="STEM.txt caption files; STEM.emb.pt is written next to each")
    a = ap.parse_args(argv)
    encoder, tokenizer = loader(a.pipe, device=a.device, softcap=not a.no_softcap)
    if hasattr(encoder, "describe"):
        print(encoder.describe())
    if a.captions:
        texts = []
        for path in a.captions:
            with open(path, encoding="utf-8") as f:
                texts.append(f.read())
        embs = extract_embeddings(encoder, tokenizer, texts, max_batch=a.batch)
        for path, emb in zip(a.captions, embs):
            out = os.path.splitext(path)[0] + ".emb.pt"
            torch.save(emb.to(torch.bfloat16).cpu().clone(), out)
            print(f"{out}: {tuple(emb.shape)}")
    if a.empty:
        emb = extract_embeddings(encoder, tokenizer, [""])
        torch.save([e.to(torch.bfloat16).cpu().clone() for e in emb], a.empty)
        print(f"{a.empty}: {tuple(emb[0].shape)}")
    if a.validation:
        with open(a.validation[0], encoding="utf-8") as f:
            prompts = [line.rstrip("\n") for line in f if line.strip()]
        torch.save(validation_embeddings(encoder, tokenizer, prompts), a.validation[1])
        print(f"{a.validation[1]}: {len(prompts)} prompt(s)")


if __name__ == "__main__":
    main()
