"""Host side of the T5 text encoder without a GPU: the torch restatement (tests/t5_ref.py) pinned against transformers' own
T5EncoderModel, the per-distance bias table, T5's tokenizer rule, the checkpoint loader, the prompt rules of
yat_amd/encode_prompts.py, the trainer's refusal and the command line with its ``model_type`` dispatch."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests import t5_ref as R
from yat_amd import encode_prompts as EP
from yat_amd import t5 as T

BF = torch.bfloat16
LENGTHS = (1, 23, 70)
PAD_TO = 300


# ------------------------------------------------------------------------------------------------- pin against transformers
@pytest.fixture(scope="module")
def hf(tmp_path_factory):
    """A random transformers T5EncoderModel saved with save_pretrained, and a batch right-padded to 300."""
    transformers = pytest.importorskip("transformers")
    cfg = R.tiny_config()
    keys = ("d_model", "num_layers", "num_heads", "d_kv", "d_ff", "vocab_size", "layer_norm_epsilon",
            "relative_attention_num_buckets", "relative_attention_max_distance", "feed_forward_proj")
    hcfg = transformers.T5Config(**{k: cfg[k] for k in keys}, pad_token_id=0, attn_implementation="eager")
    model = transformers.T5EncoderModel(hcfg).eval()
    sd = R.random_state_dict(cfg, seed=3, logit_gain=2.0)          # logits reach tens (asserted below)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("embed_tokens" in k for k in missing), (missing, unexpected)
    d = str(tmp_path_factory.mktemp("t5") / "text_encoder")
    model.save_pretrained(d)
    g = torch.Generator().manual_seed(5)
    ids = [torch.randint(1, cfg["vocab_size"], (n,), generator=g) for n in LENGTHS]
    batch = torch.zeros(len(ids), PAD_TO, dtype=torch.long)
    mask = torch.zeros_like(batch)
    for b, t in enumerate(ids):
        batch[b, :len(t)], mask[b, :len(t)] = t, 1
    return SimpleNamespace(model=model, dir=d, ids=ids, batch=batch, mask=mask, sd=sd, cfg=cfg)


def _hf_rows(hf, dtype):
    model = type(hf.model).from_pretrained(hf.dir, dtype=dtype, attn_implementation="eager").eval()
    model = model.to(dtype)                                        # (``pipe.to(bfloat16)``: wo too, which a load may keep in fp32)
    with torch.no_grad():
        out = model(input_ids=hf.batch, attention_mask=hf.mask).last_hidden_state
    return [out[b, :n] for b, n in enumerate(LENGTHS)]


@pytest.mark.parametrize("dtype,bound", [(torch.float32, 1e-6), (BF, 1e-3)])
def test_restatement_matches_transformers(hf, dtype, bound):
    cfg, sd = T.load_text_encoder_dir(hf.dir)                      # (bf16 copies of the stored fp32 weights)
    sd = {k: v.to(dtype) for k, v in (hf.sd if dtype == torch.float32 else sd).items()}
    want = _hf_rows(hf, dtype)
    ref = R.T5Ref(cfg, sd, dtype)
    padded = ref.forward(hf.batch, hf.mask)         # the same right-padded batch: the same op shapes as transformers runs
    got = [padded[b, :n] for b, n in enumerate(LENGTHS)]
    if dtype == torch.float32:                      # packing is exact: a prompt alone sees what its real rows see in the batch
        for n, a, b in zip(LENGTHS, ref.encode(hf.ids), got):
            assert R.rel_l2(a, b) <= 1e-6, (n, R.rel_l2(a, b))
    for n, a, b in zip(LENGTHS, got, want):
        e = R.rel_l2(a, b)
        print(f"[t5] restatement vs transformers, {dtype}, L={n}: rel_l2={e:.3e}")
        assert a.shape == b.shape and e <= bound, (n, e)


def test_logits_reach_tens_and_the_bias_matters(hf):
    cfg, sd = hf.cfg, hf.sd
    ids = hf.ids[2]
    h = R.layer_norm(torch.nn.functional.embedding(ids, sd["shared.weight"]), sd["encoder.block.0.layer.0.layer_norm.weight"], 1e-6)
    q = (h @ sd["encoder.block.0.layer.0.SelfAttention.q.weight"].T)[:, :64]
    k = (h @ sd["encoder.block.0.layer.0.SelfAttention.k.weight"].T)[:, :64]
    assert (q @ k.T).abs().max() > 30
    on = R.T5Ref(cfg, sd).encode([ids])[0]
    off = R.T5Ref(cfg, {**sd, R.REL: torch.zeros_like(sd[R.REL])}).encode([ids])[0]
    assert R.rel_l2(on, off) > 1e-2


# -------------------------------------------------------------------------------------------------------------- bias table
@pytest.mark.parametrize("L", [1, 2, 9, 17, 129, 300, 512])
def test_relative_bias_table_is_compute_bias(hf, L):
    attn = hf.model.encoder.block[0].layer[0].SelfAttention
    with torch.no_grad():
        want = attn.compute_bias(L, L)[0]                           # [H, L, L], fp32
    w = attn.relative_attention_bias.weight.detach()
    for max_len in sorted({L, 512}):
        table = T.relative_bias_table(w, 32, 128, max_len)
        assert table.shape == (4, 2 * max_len - 1) and table.dtype == BF
        i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
        got = table[:, (j - i) + max_len - 1]                       # the kernel's lookup: key index - query index
        assert torch.equal(got, want.to(BF)), (L, max_len)
    if L > 1:                                                       # the sign of the distance is not symmetric
        assert not torch.equal(want[:, 0, L - 1], want[:, L - 1, 0])
    assert torch.equal(R.compute_bias(w, L), attn.compute_bias(L, L).detach())


# ---------------------------------------------------------------------------------------------------------- tokenizer rule
WORDS = [f"w{i}" for i in range(40)] + ["a", "cat"]


@pytest.fixture(scope="module")
def spiece(tmp_path_factory):
    """A sentencepiece model trained here (T5's layout: <pad> 0, </s> 1, <unk> 2) in a tokenizer directory."""
    spm = pytest.importorskip("sentencepiece")
    d = tmp_path_factory.mktemp("tok")
    corpus = d / "corpus.txt"
    corpus.write_text("\n".join(" ".join(WORDS[i:] + WORDS[:i]) for i in range(len(WORDS))) + "\n")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(d / "spiece"), vocab_size=60, model_type="unigram",
                                   hard_vocab_limit=False, pad_id=0, eos_id=1, unk_id=2, bos_id=-1, minloglevel=2)
    os.remove(corpus)
    os.remove(d / "spiece.vocab")
    (d / "tokenizer_config.json").write_text(json.dumps({"tokenizer_class": "T5Tokenizer", "eos_token": "</s>",
                                                         "unk_token": "<unk>", "pad_token": "<pad>", "extra_ids": 0}))
    return str(d)


def _text_of_pieces(tok, n):
    """A text of exactly ``n`` sentencepiece pieces, mixed words first and one-piece words to land on ``n``."""
    text, i = "", 0
    while len(tok._pieces(text)) < n:
        for w in [WORDS[i % len(WORDS)], "cat", "a"]:
            cand = (text + " " + w).strip()
            if len(tok._pieces(cand)) <= n:
                text, i = cand, i + 1
                break
        else:
            raise AssertionError(f"no text of {n} pieces")
    return text


def test_tokenizer_rule_matches_transformers(spiece):
    transformers = pytest.importorskip("transformers")
    want_tok = transformers.T5Tokenizer.from_pretrained(spiece)
    tok = EP.load_t5_tokenizer(spiece)
    assert tok.eos_id == 1
    texts = ["", "a cat", _text_of_pieces(tok, 299), _text_of_pieces(tok, 300), _text_of_pieces(tok, 301),
             "  A  Cat ", "W1  w2   A", " cat"]
    for text in texts:
        clean = text.lower().strip()
        want = want_tok(clean, padding="max_length", max_length=300, truncation=True, add_special_tokens=True)
        ids = EP.tokenize_t5_prompts(tok, [text])[0][0]
        n = sum(want["attention_mask"])
        assert ids == list(want["input_ids"][:n]), text[:40]
        assert all(i == 0 for i in want["input_ids"][n:]) and len(want["input_ids"]) == 300
        assert ids[-1] == 1 and len(ids) <= 300
    assert EP.tokenize_t5_prompts(tok, "")[0][0] == [1]
    assert [len(EP.tokenize_t5_prompts(tok, [t])[0][0]) for t in texts[2:5]] == [300, 300, 300]


def test_tokenizer_json_is_preferred_and_gets_eos(tmp_path):
    tk = pytest.importorskip("tokenizers")
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.processors import TemplateProcessing
    vocab = {"<pad>": 0, "</s>": 1, "<unk>": 2, "a": 3, "cat": 4}
    tok = tk.Tokenizer(WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = Whitespace()
    tok.post_processor = TemplateProcessing(single="$A </s>", special_tokens=[("</s>", 1)])
    tok.save(str(tmp_path / "tokenizer.json"))
    t = EP.load_t5_tokenizer(str(tmp_path))
    assert EP.tokenize_t5_prompts(t, [" A Cat", ""])[0] == [[3, 4, 1], [1]]
    assert EP.tokenize_t5_prompts(t, ["a " * 400])[0][0] == [3] * 299 + [1]


# ------------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture()
def tiny(tmp_path):
    cfg = R.tiny_config(num_layers=1)
    return cfg, R.random_state_dict(cfg, seed=1), str(tmp_path / "text_encoder")


def test_single_file_and_sharded_layouts_load_the_same(tiny, tmp_path):
    cfg, sd, d = tiny
    R.save_pretrained_layout(d, cfg, sd)
    d2 = str(tmp_path / "sharded")
    tied = {k: v for k, v in sd.items() if k != "shared.weight"}
    tied["encoder.embed_tokens.weight"] = sd["shared.weight"]      # the other name of the tied embedding
    R.save_pretrained_layout(d2, cfg, tied, shards=2)
    assert os.path.isfile(os.path.join(d2, "model.safetensors.index.json"))
    _, a = T.load_text_encoder_dir(d)
    _, b = T.load_text_encoder_dir(d2)
    assert sorted(a) == sorted(b) == sorted(sd)
    assert all(a[k].dtype == BF and torch.equal(a[k], b[k]) and torch.equal(a[k], sd[k].to(BF)) for k in sd)
    wo = "encoder.block.0.layer.1.DenseReluDense.wo.weight"
    assert sd[wo].dtype == torch.float32 and a[wo].dtype == BF     # a wo kept in fp32 is cast
    R.save_pretrained_layout(d, cfg, {**{k: v.to(BF) for k, v in sd.items()}, wo: sd[wo]})
    _, c = T.load_text_encoder_dir(d)
    assert c[wo].dtype == BF and torch.equal(c[wo], a[wo])


def test_a_dropped_an_extra_and_an_untied_key_are_named(tiny):
    cfg, sd, d = tiny
    R.save_pretrained_layout(d, cfg, {k: v for k, v in sd.items() if "wi_1" not in k})
    with pytest.raises(KeyError, match="wi_1"):
        T.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, {k: v for k, v in sd.items() if k != R.REL})
    with pytest.raises(KeyError, match="relative_attention_bias"):
        T.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, {k: v for k, v in sd.items() if k != "shared.weight"})
    with pytest.raises(KeyError, match="shared.weight"):
        T.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, sd, extra={"decoder.final_layer_norm.weight": torch.zeros(8)})
    with pytest.raises(KeyError, match="decoder.final_layer_norm"):
        T.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, {**sd, "encoder.final_layer_norm.weight": torch.zeros(8)})
    with pytest.raises(ValueError, match="final_layer_norm"):
        T.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, sd, extra={"encoder.embed_tokens.weight": sd["shared.weight"].clone()})
    T.load_text_encoder_dir(d)                                     # both names, equal: accepted
    R.save_pretrained_layout(d, cfg, sd, extra={"encoder.embed_tokens.weight": sd["shared.weight"] + 1.0})
    with pytest.raises(ValueError, match="tied"):
        T.load_text_encoder_dir(d)


@pytest.mark.parametrize("over", [{"feed_forward_proj": "relu"}, {"feed_forward_proj": "gated-silu"}, {"d_kv": 128},
                                  {"is_decoder": True}, {"is_encoder_decoder": True, "architectures": ["T5ForConditionalGeneration"]},
                                  {"d_model": 132}, {"d_ff": 260}])
def test_refused_configs(tiny, over):
    cfg, sd, d = tiny
    R.save_pretrained_layout(d, {**cfg, **over}, sd)
    with pytest.raises(NotImplementedError):
        T.load_text_encoder_dir(d)
    with pytest.raises(NotImplementedError):
        T.validate_config({**cfg, **over})


def test_a_t5_encoder_model_config_as_shipped_is_accepted(tiny):
    cfg = tiny[0]
    T.validate_config({**cfg, "is_encoder_decoder": True})          # what save_pretrained of a T5EncoderModel may leave
    T.validate_config(R.real_width_config())


# ------------------------------------------------------------------------------------------------------------ prompt rules
class StubEncoder:
    """Row r of a prompt's embedding is (r + 1) in every channel: shows which rows the rules keep."""
    H = 16
    model_type = "t5"

    def __init__(self):
        self.calls = []

    def encode(self, prompts, max_batch=None):
        self.calls.append(([p.tolist() for p in prompts], max_batch))
        return [(torch.arange(1, len(p) + 1, dtype=torch.float32)[:, None] * torch.ones(1, self.H)).to(BF) for p in prompts]


def test_prompt_rules(spiece):
    tok = EP.load_t5_tokenizer(spiece)
    enc = StubEncoder()
    embs = EP.extract_embeddings(enc, tok, ["  A Cat ", ""], max_batch=3)
    n = len(tok._pieces("a cat"))
    assert [tuple(e.shape) for e in embs] == [(n + 1, 16), (1, 16)]
    assert enc.calls[0] == ([tok._pieces("a cat") + [1], [1]], 3)
    emb, mask = EP.encode_prompt(enc, tok, ["a cat", ""])
    assert emb.shape == (2, 300, 16) and mask.shape == (2, 300) and mask.dtype == torch.int64 and emb.dtype == BF
    assert mask.sum(1).tolist() == [n + 1, 1] and not emb[0, n + 1:].any() and not emb[1, 1:].any()
    assert torch.equal(emb[0, :n + 1], embs[0])
    out = EP.validation_embeddings(enc, tok, ["a cat", "w1 w2"])
    assert len(out) == 2
    for pe, pm, ne, nm in out:
        assert pe.shape == ne.shape == (1, 300, 16) and pm.shape == nm.shape == (1, 300) and pe.dtype == BF
        assert pe.device.type == "cpu" and int(nm.sum()) == 1 and nm[0, 0] == 1 and not ne[0, 1:].any()      # "" is </s> alone
    assert int(out[0][1].sum()) == n + 1                            # no instruction in front of the prompt


# ----------------------------------------------------------------------------------------------------------------- trainer
def test_extract_embeddings_without_a_text_encoder_names_the_directory(tmp_path):
    import train_pixart_sigma
    import train_sd35
    m = train_pixart_sigma.PixartSigmaTrainer.__new__(train_pixart_sigma.PixartSigmaTrainer)      # host check only
    m.params = SimpleNamespace(pretrained_pipe_path=str(tmp_path / "pipe"))
    with pytest.raises(NotImplementedError) as e:
        m.extract_embeddings(["a"])
    assert os.path.join(str(tmp_path / "pipe"), "text_encoder") in str(e.value) and "T5" in str(e.value)
    assert m.encode_validation_prompts() is None
    s = train_sd35.SD35Trainer.__new__(train_sd35.SD35Trainer)
    s.params = SimpleNamespace(pretrained_pipe_path=str(tmp_path / "pipe"))
    with pytest.raises(NotImplementedError, match="outside the hot-path scope"):
        s.extract_embeddings(["a"])
    assert s.encode_validation_prompts() is None


# ------------------------------------------------------------------------------------------------------------ command line
def test_command_line_dispatches_on_model_type(spiece, tiny, tmp_path, capsys, monkeypatch):
    """``load_encoder`` reads ``text_encoder/config.json``: ``t5`` builds T5EncoderHIP with T5's tokenizer, and ``main`` then
    applies T5's rules (no BOS, EOS appended, no instruction)."""
    import shutil
    from yat_amd import extract_latents
    from yat_amd.common.trainer import Model
    cfg, sd, _ = tiny
    pipe = tmp_path / "pipe"
    R.save_pretrained_layout(str(pipe / "text_encoder"), cfg, sd)
    shutil.copytree(spiece, pipe / "tokenizer")
    assert EP.text_encoder_model_type(str(pipe)) == "t5" and EP.text_encoder_model_type(str(tmp_path / "none")) is None
    built = []

    def fake_from_pretrained(cls, te_dir, device="cuda"):
        built.append((te_dir, device))
        return StubEncoder()
    monkeypatch.setattr(T.T5EncoderHIP, "from_pretrained", classmethod(fake_from_pretrained))
    (tmp_path / "img0.txt").write_text(" A Cat \n")
    (tmp_path / "img1.txt").write_text("")
    (tmp_path / "prompts.txt").write_text("a cat\nw1 w2 w3\n")
    EP.main(["--pipe", str(pipe), "--device", "cpu", "--empty", str(tmp_path / "empty_embeds.pt"), "--validation",
             str(tmp_path / "prompts.txt"), str(tmp_path / "validation_embeds.pt"), str(tmp_path / "img0.txt"),
             str(tmp_path / "img1.txt")])
    assert built == [(str(pipe / "text_encoder"), "cpu")]
    n = len(EP.load_t5_tokenizer(spiece)._pieces("a cat"))
    e0 = extract_latents.load_embedding(str(tmp_path / "img0.png"))                 # the sidecar extract_latents reads
    e1 = extract_latents.load_embedding(str(tmp_path / "img1.png"))
    assert e0.shape == (n + 1, 16) and e1.shape == (1, 16) and e0.dtype == BF
    empty = torch.load(tmp_path / "empty_embeds.pt", map_location="cpu")
    checked = Model.check_empty_embeddings(None, empty, "empty_embeds.pt")           # the trainer's reader
    assert len(checked) == 1 and checked[0].shape == (1, 16) and checked[0].dtype == BF
    val = torch.load(tmp_path / "validation_embeds.pt", map_location="cpu")
    assert len(val) == 2 and all(len(v) == 4 and v[0].shape == (1, 300, 16) and v[1].shape == (1, 300) for v in val)
    assert int(val[0][1].sum()) == n + 1 and int(val[0][3].sum()) == 1
    # an unknown model_type is refused by name
    (pipe / "text_encoder" / "config.json").write_text(json.dumps({**cfg, "model_type": "clip_text_model"}))
    with pytest.raises(NotImplementedError, match="clip_text_model"):
        EP.load_encoder(str(pipe), device="cpu")
