"""Host side of the CLIP text encoders and the SD3 prompt rules without a GPU: the torch restatement (tests/clip_ref.py) pinned
against transformers' own CLIPTextModelWithProjection, the causal-prefix property, CLIP's tokenizer rule against
transformers.CLIPTokenizer, the checkpoint loader, the SD3 assembly on stub encoders and the command line."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests import clip_ref as R
from yat_amd import clip as CL
from yat_amd import encode_prompts as EP

BF = torch.bfloat16
EOS, HIGH_PAD = 400, 450                       # the end-of-text id of the test prompts, and a pad id above it


def _prompt_batch(vocab_below=EOS, seed=5):
    """Three prompts of 77 ids.  0: a second EOS later on, padded with EOS (CLIP-L's pad).  1: EOS at 10, then a pad id ABOVE
    EOS: ``argmax`` lands on the first pad, the first-EOS rule on 10.  2: EOS in the last position."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab_below, (3, 77), generator=g)
    ids[:, 0] = 0
    ids[0, 21], ids[0, 40:] = EOS, EOS
    ids[1, 10], ids[1, 11:] = EOS, HIGH_PAD
    ids[2, 76] = EOS
    return ids


# ------------------------------------------------------------------------------------------------- pin against transformers
@pytest.fixture(scope="module", params=[("quick_gelu", 2), ("gelu", EOS)], ids=["quick_gelu-argmax", "gelu-first_eos"])
def hf(request, tmp_path_factory):
    """A random transformers CLIPTextModelWithProjection saved with save_pretrained."""
    transformers = pytest.importorskip("transformers")
    act, eos = request.param
    cfg = R.tiny_config(act, eos)
    keys = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "projection_dim",
            "max_position_embeddings", "vocab_size", "hidden_act", "layer_norm_eps", "bos_token_id", "eos_token_id", "pad_token_id")
    hcfg = transformers.CLIPTextConfig(**{k: cfg[k] for k in keys}, attn_implementation="eager")
    model = transformers.CLIPTextModelWithProjection(hcfg).eval()
    sd = R.random_state_dict(cfg, seed=3, logit_gain=2.0)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    d = str(tmp_path_factory.mktemp("clip") / "text_encoder")
    model.save_pretrained(d)
    return SimpleNamespace(model=model, dir=d, ids=_prompt_batch(), sd=sd, cfg=cfg)


@pytest.mark.parametrize("dtype,bound", [(torch.float32, 1e-6), (BF, 1e-3)])
def test_restatement_matches_transformers(hf, dtype, bound):
    cfg, sd = CL.load_text_encoder_dir(hf.dir)                      # (bf16 copies of the stored fp32 weights)
    sd = {k: v.to(dtype) for k, v in (hf.sd if dtype == torch.float32 else sd).items()}
    model = type(hf.model).from_pretrained(hf.dir, dtype=dtype, attn_implementation="eager").eval().to(dtype)
    with torch.no_grad():
        out = model(input_ids=hf.ids, output_hidden_states=True)
    assert len(out.hidden_states) == cfg["num_hidden_layers"] + 1
    hs, te, _ = R.CLIPRef(cfg, sd, dtype).forward(hf.ids)
    for name, a, b in (("hidden_states[-2]", hs, out.hidden_states[-2]), ("text_embeds", te, out.text_embeds)):
        e = R.rel_l2(a, b)
        print(f"[clip] restatement vs transformers, {cfg['hidden_act']} eos={cfg['eos_token_id']}, {dtype}, {name}: rel_l2={e:.3e}")
        assert a.shape == b.shape and e <= bound, (name, e)
    # the prompts are built so that the two EOS rules disagree, and the restatement follows the config's
    assert R.eos_position(hf.ids, 2).tolist() == [21, 11, 76] and R.eos_position(hf.ids, EOS).tolist() == [21, 10, 76]
    other = R.CLIPRef({**cfg, "eos_token_id": EOS if cfg["eos_token_id"] == 2 else 2}, sd, dtype).forward(hf.ids)[1]
    assert R.rel_l2(other[1], te[1]) > 1e-2 and torch.equal(other[0], te[0])
    assert [CL.eos_position(r, cfg["eos_token_id"]) for r in hf.ids] == R.eos_position(hf.ids, cfg["eos_token_id"]).tolist()


def test_a_prefix_encodes_to_the_prefix_rows():
    cfg = R.tiny_config()
    ref = R.CLIPRef(cfg, R.random_state_dict(cfg, seed=3, logit_gain=2.0))
    ids = _prompt_batch()
    full = ref.forward(ids)[0]
    for n in (1, 30, 76):
        e = R.rel_l2(ref.forward(ids[:, :n])[0], full[:, :n])
        assert e <= 1e-6, (n, e)


# ---------------------------------------------------------------------------------------------------------- tokenizer rule
@pytest.fixture(scope="module")
def clip_tok_dirs(tmp_path_factory):
    pytest.importorskip("tokenizers")
    d = tmp_path_factory.mktemp("clip_tok")
    return R.clip_tokenizer_dir(d / "tokenizer", "<|endoftext|>"), R.clip_tokenizer_dir(d / "tokenizer_2", "!")


TEXTS = ["A Cat", "the   DOG \n\t and the cat's  dog", "", "cat " * 100, "café 42 dogs!!", "  The cat. "]


@pytest.mark.parametrize("which", [0, 1], ids=["pad=eos", "pad=!"])
def test_clip_tokenizer_rule_matches_transformers(clip_tok_dirs, which):
    transformers = pytest.importorskip("transformers")
    d = clip_tok_dirs[which]
    theirs = transformers.CLIPTokenizer.from_pretrained(d)
    ours = EP.load_clip_tokenizer(d)
    assert ours.pad_id == theirs.pad_token_id and ours.eos_id == theirs.eos_token_id and ours.bos_id == theirs.bos_token_id
    assert (ours.pad_id == ours.eos_id) == (which == 0)
    for text in TEXTS:
        want = theirs(text, padding="max_length", max_length=77, truncation=True).input_ids
        got = ours.tokenize(text)
        assert got == want and len(got) == 77, text
    assert ours.tokenize("") == [ours.bos_id, ours.eos_id] + [ours.pad_id] * 75
    long = ours.tokenize("cat " * 100)
    assert long[0] == ours.bos_id and long[76] == ours.eos_id and ours.eos_id not in long[1:76]      # 75 pieces kept
    assert ours.tokenize("A Cat") == ours.tokenize("a   cat")                                          # lowercased, collapsed


# ------------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture()
def tiny(tmp_path):
    cfg = R.tiny_config()
    sd = {k: v.to(BF) for k, v in R.random_state_dict(cfg, seed=1).items()}
    return cfg, sd, str(tmp_path / "text_encoder")


def test_loader_single_file_and_shards(tiny):
    cfg, sd, d = tiny
    R.save_pretrained_layout(d, cfg, sd)
    c1, one = CL.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, sd, shards=3)
    c2, many = CL.load_text_encoder_dir(d)
    assert c1 == c2 == cfg and sorted(one) == sorted(many) == sorted(CL.expected_keys(cfg))
    assert all(torch.equal(one[k], many[k]) and one[k].dtype == BF for k in one)
    R.save_pretrained_layout(d, cfg, {k: v.float() for k, v in sd.items()})             # stored fp32: cast to bf16
    assert all(v.dtype == BF and torch.equal(v, sd[k]) for k, v in CL.load_text_encoder_dir(d)[1].items())


def test_loader_is_strict(tiny):
    cfg, sd, d = tiny
    lost = "text_model.encoder.layers.1.self_attn.k_proj.bias"
    R.save_pretrained_layout(d, cfg, {k: v for k, v in sd.items() if k != lost})
    with pytest.raises(KeyError, match="layers.1.self_attn.k_proj.bias"):
        CL.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, sd, extra={"vision_model.post_layernorm.weight": torch.zeros(8)})
    with pytest.raises(KeyError, match="vision_model.post_layernorm"):
        CL.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, {**sd, "text_projection.weight": torch.zeros(8, 8)})
    with pytest.raises(ValueError, match="text_projection"):
        CL.load_text_encoder_dir(d)
    # a stored position_ids buffer (older transformers) is dropped unread
    R.save_pretrained_layout(d, cfg, sd, extra={"text_model.embeddings.position_ids": torch.arange(77)[None]})
    assert sorted(CL.load_text_encoder_dir(d)[1]) == sorted(sd)


@pytest.mark.parametrize("over", [{"num_attention_heads": 4}, {"hidden_act": "relu"}, {"hidden_act": "gelu_new"},
                                  {"max_position_embeddings": 513}, {"intermediate_size": 260}, {"projection_dim": 60}])
def test_refused_configs(tiny, over):
    cfg, sd, d = tiny
    R.save_pretrained_layout(d, {**cfg, **over}, sd)
    with pytest.raises(NotImplementedError):
        CL.load_text_encoder_dir(d)
    with pytest.raises(NotImplementedError):
        CL.validate_config({**cfg, **over})


def test_the_shipped_shapes_are_accepted():
    CL.validate_config(R.real_width_config())
    CL.validate_config(R.tiny_config(hidden_size=768, num_attention_heads=12, intermediate_size=3072, projection_dim=768))


# ---------------------------------------------------------------------------------------------------------------- assembly
class StubClip:
    """hidden_states[-2] row r is ``base + r`` in every channel, text_embeds is ``base`` everywhere."""
    model_type = "clip_text_model"
    layers = []

    def __init__(self, width, base):
        self.H = self.projection_dim = width
        self.base, self.calls = float(base), []

    def encode(self, prompts, max_batch=None):
        self.calls.append(([p.tolist() for p in prompts], max_batch))
        return [(((torch.arange(len(p), dtype=torch.float32) + self.base)[:, None] * torch.ones(1, self.H)).to(BF),
                 torch.full((self.projection_dim,), self.base).to(BF)) for p in prompts]

    def describe(self):
        return f"stub CLIP {self.H}"

    def free(self):
        self.layers = None


class StubT5:
    H, layers = 4096, []

    def __init__(self):
        self.calls = []

    def encode(self, prompts, max_batch=None):
        self.calls.append(([p.tolist() for p in prompts], max_batch))
        return [torch.full((len(p), self.H), 7.0).to(BF) for p in prompts]

    def describe(self):
        return "stub T5"

    def free(self):
        self.layers = None


def _stub_encoders(clip_tok_dirs):
    toks = (EP.load_clip_tokenizer(clip_tok_dirs[0]), EP.load_clip_tokenizer(clip_tok_dirs[1]),
            EP.T5Tokenizer(lambda text: [5 + (i % 3) for i in range(len(text.split()))], 1))
    return EP.SD3TextEncodersHIP(StubClip(768, 100.0), StubClip(1280, 300.0), StubT5(), toks)


def test_sd3_assembly_on_stub_encoders(clip_tok_dirs):
    enc = _stub_encoders(clip_tok_dirs)
    assert enc.H == 4096 and enc.pooled_dim == 2048 and enc.layers == [] and EP.rules_for(enc) is EP.RULES["clip_text_model"]
    assert "compress_caption" in enc.describe()
    out = EP.extract_embeddings(enc, enc.tokenizers, ["A Cat and the dog", ""], max_batch=3)
    assert len(out) == 2
    for prompt, pooled in out:
        assert prompt.shape == (333, 4096) and pooled.shape == (2048,) and prompt.dtype == pooled.dtype == BF
        assert not prompt[:77, 2048:].any()                                               # the zero block beside the CLIP rows
        want_rows = torch.arange(77, dtype=torch.float32)[:, None]
        assert torch.equal(prompt[:77, :768].float(), (want_rows + 100.0).expand(77, 768).to(BF).float())       # L first
        assert torch.equal(prompt[:77, 768:2048].float(), (want_rows + 300.0).expand(77, 1280).to(BF).float())  # then G
        assert (prompt[77:] == 7.0).all()
        assert (pooled[:768] == 100.0).all() and (pooled[768:] == 300.0).all()
    tl, tg, _ = enc.tokenizers
    assert enc.clip_l.calls == [([tl.tokenize("A Cat and the dog"), tl.tokenize("")], 3)]
    assert enc.clip_g.calls == [([tg.tokenize("A Cat and the dog"), tg.tokenize("")], 3)]
    assert enc.clip_l.calls[0][0][0] != enc.clip_g.calls[0][0][0]                         # the two pad tokens
    (ids, _), = enc.t5.calls                                                              # 256 ids each, pads included
    assert ids == [[5, 6, 7, 5, 6, 1] + [0] * 250, [1] + [0] * 255]
    # the CLIP text may differ from the T5 text
    enc = _stub_encoders(clip_tok_dirs)
    EP.extract_embeddings(enc, enc.tokenizers, ["a long caption about the cat"], clip_captions=["cat"])
    assert enc.clip_l.calls[0][0] == [tl.tokenize("cat")] and enc.t5.calls[0][0][0][:7] == [5, 6, 7, 5, 6, 7, 1]
    with pytest.raises(ValueError, match="CLIP prompt"):
        EP.extract_embeddings(enc, enc.tokenizers, ["a", "b"], clip_captions=["a"])
    with pytest.raises(ValueError, match="instruction"):
        EP.tokenize_sd3_prompts(enc.tokenizers, ["a"], ["an instruction"])
    val = EP.validation_embeddings(enc, enc.tokenizers, ["the cat", "the dog"])
    assert len(val) == 2
    for pe, ne, pp, npp in val:
        assert pe.shape == ne.shape == (1, 333, 4096) and pp.shape == npp.shape == (1, 2048) and pe.device.type == "cpu"
    assert enc.t5.calls[1][0] == [[1] + [0] * 255]                                        # the negative prompt is ""
    enc.free()
    assert enc.layers is None


def test_sd3_encoders_refuse_widths_that_do_not_fit(clip_tok_dirs):
    with pytest.raises(ValueError, match="768.*4096.*4096"):
        EP.SD3TextEncodersHIP(StubClip(768, 0.0), StubClip(4096, 0.0), StubT5(), (None, None, None))


def test_find_text_dirs_needs_all_six(clip_tok_dirs, tmp_path):
    import shutil
    pipe = tmp_path / "pipe"
    for sfx in ("", "_2", "_3"):
        os.makedirs(pipe / ("text_encoder" + sfx))
        (pipe / ("text_encoder" + sfx) / "config.json").write_text(json.dumps({"model_type": "clip_text_model"}))
    shutil.copytree(clip_tok_dirs[0], pipe / "tokenizer")
    shutil.copytree(clip_tok_dirs[1], pipe / "tokenizer_2")
    assert EP.text_encoder_model_type(str(pipe)) == "clip_text_model"
    assert EP.find_text_dirs(str(pipe), "clip_text_model") is None                        # no tokenizer_3 yet
    os.makedirs(pipe / "tokenizer_3")
    (pipe / "tokenizer_3" / "spiece.model").write_bytes(b"")
    dirs = EP.find_text_dirs(str(pipe), "clip_text_model")
    assert [os.path.basename(d) for d in dirs] == ["text_encoder", "text_encoder_2", "text_encoder_3", "tokenizer", "tokenizer_2",
                                                   "tokenizer_3"]
    os.remove(pipe / "tokenizer_2" / "merges.txt")
    assert EP.find_text_dirs(str(pipe), "clip_text_model") is None
    shutil.rmtree(pipe / "text_encoder_2")
    with pytest.raises(NotImplementedError, match="SD3.5"):
        EP.load_encoder(str(pipe), device="cpu")


# ------------------------------------------------------------------------------------------------------------ command line
def test_command_line_writes_the_two_sidecars(clip_tok_dirs, tmp_path, capsys):
    from yat_amd import extract_latents
    from train_sd35 import SD35Trainer
    enc = _stub_encoders(clip_tok_dirs)
    seen = []

    def loader(pipe, device="cuda", softcap=True):
        seen.append((pipe, device))
        return enc, enc.tokenizers
    (tmp_path / "img0.txt").write_text("A long caption about the Cat\n")
    (tmp_path / "img0.clip.txt").write_text("cat")
    (tmp_path / "img1.txt").write_text("the dog")
    (tmp_path / "prompts.txt").write_text("the cat\nthe dog\n")
    EP.main(["--pipe", "PIPE", "--device", "cpu", "--empty", str(tmp_path / "empty_embeds.pt"), "--validation",
             str(tmp_path / "prompts.txt"), str(tmp_path / "validation_embeds.pt"), str(tmp_path / "img0.txt"),
             str(tmp_path / "img1.txt")], loader=loader)
    assert seen == [("PIPE", "cpu")] and "stub CLIP 768" in capsys.readouterr().out
    tl = enc.tokenizers[0]
    assert enc.clip_l.calls[0][0] == [tl.tokenize("cat"), tl.tokenize("the dog")]          # img0.clip.txt, and img1's caption
    assert enc.t5.calls[0][0][0][:7] == [5, 6, 7, 5, 6, 7, 1]                               # T5 gets img0.txt itself
    e0 = extract_latents.load_embedding(str(tmp_path / "img0.png"))                        # the sidecars extract_latents reads
    p0 = extract_latents.load_pooled(str(tmp_path / "img0.png"))
    assert e0.shape == (333, 4096) and p0.shape == (2048,) and e0.dtype == p0.dtype == BF
    assert os.path.isfile(tmp_path / "img1.emb.pt") and os.path.isfile(tmp_path / "img1.pooled.pt")
    empty = torch.load(tmp_path / "empty_embeds.pt", map_location="cpu")
    checked = SD35Trainer.check_empty_embeddings(None, empty, "empty_embeds.pt")            # the trainer's reader
    assert len(checked) == 1 and checked[0][0].shape == (333, 4096) and checked[0][1].shape == (2048,)
    val = torch.load(tmp_path / "validation_embeds.pt", map_location="cpu")
    assert len(val) == 2 and all(len(v) == 4 and v[0].shape == v[1].shape == (1, 333, 4096) and v[2].shape == v[3].shape == (1, 2048)
                                 for v in val)
