"""Host side of the Gemma-2 text encoder without a GPU: the torch restatement (tests/gemma2_ref.py) pinned against
transformers' own Gemma2Model, the checkpoint loader, the prompt rules of yat_amd/encode_prompts.py, the trainer's refusal and
the command line's three file layouts."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from tests import gemma2_ref as R
from yat_amd import encode_prompts as EP
from yat_amd import gemma2 as G

BF = torch.bfloat16
LENGTHS = (1, 23, 70)


# ------------------------------------------------------------------------------------------------- pin against transformers
@pytest.fixture(scope="module")
def hf(tmp_path_factory):
    """A random transformers Gemma2Model (eager attention) saved with save_pretrained, the same weights through this
    project's loader, and a right-padded batch."""
    transformers = pytest.importorskip("transformers")
    cfg = R.tiny_config()
    keys = ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim", "intermediate_size",
            "vocab_size", "rms_norm_eps", "query_pre_attn_scalar", "attn_logit_softcapping", "sliding_window",
            "max_position_embeddings", "hidden_activation", "attention_bias")
    hcfg = transformers.Gemma2Config(**{k: cfg[k] for k in keys}, pad_token_id=0, attn_implementation="eager")
    model = transformers.Gemma2Model(hcfg).eval()
    sd = R.random_state_dict(cfg, seed=3, logit_gain=6.0)          # q / k gain: the pre-cap logits pass +-50 (asserted below)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    d = str(tmp_path_factory.mktemp("gemma2") / "text_encoder")
    model.save_pretrained(d)
    g = torch.Generator().manual_seed(5)
    ids = [torch.randint(1, cfg["vocab_size"], (n,), generator=g) for n in LENGTHS]
    batch = torch.zeros(len(ids), max(LENGTHS), dtype=torch.long)
    mask = torch.zeros_like(batch)
    for b, t in enumerate(ids):
        batch[b, :len(t)], mask[b, :len(t)] = t, 1
    return SimpleNamespace(model=model, dir=d, ids=ids, batch=batch, mask=mask)


def _hf_rows(hf, dtype, softcap):
    # loaded in its dtype as a pipeline loads it (a later ``model.to(bf16)`` would also round the rotary inv_freq buffer)
    model = type(hf.model).from_pretrained(hf.dir, dtype=dtype, attn_implementation="eager").eval()
    assert model.rotary_emb.inv_freq.dtype == torch.float32 and model.embed_tokens.weight.dtype == dtype
    for layer in model.layers:
        layer.self_attn.attn_logit_softcapping = softcap
    with torch.no_grad():
        out = model(input_ids=hf.batch, attention_mask=hf.mask).last_hidden_state
    return [out[b, :n] for b, n in enumerate(LENGTHS)]


@pytest.mark.parametrize("softcap", [True, False])
@pytest.mark.parametrize("dtype,bound", [(torch.float32, 1e-6), (BF, 1e-3)])
def test_restatement_matches_transformers(hf, dtype, bound, softcap):
    cfg, sd = G.load_text_encoder_dir(hf.dir)
    want = _hf_rows(hf, dtype, cfg["attn_logit_softcapping"] if softcap else None)
    ref = R.Gemma2Ref(cfg, sd, dtype, softcap=softcap)
    padded = ref.forward(hf.batch, hf.mask)         # the same right-padded batch: the same op shapes as transformers runs
    got = [padded[b, :n] for b, n in enumerate(LENGTHS)]
    if dtype == torch.float32:                      # packing is exact: a prompt alone sees what its real rows see in the batch
        for n, a, b in zip(LENGTHS, ref.encode(hf.ids), got):
            assert R.rel_l2(a, b) <= 1e-6, (n, R.rel_l2(a, b))
    for n, a, b in zip(LENGTHS, got, want):
        e = R.rel_l2(a, b)
        print(f"[gemma2] restatement vs transformers, {dtype}, softcap={softcap}, L={n}: rel_l2={e:.3e}")
        assert a.shape == b.shape and e <= bound, (n, e)


def test_the_cap_bites(hf):
    cfg, sd = G.load_text_encoder_dir(hf.dir)
    ids = hf.ids[2]
    h = R.rmsnorm(torch.nn.functional.embedding(ids, sd["embed_tokens.weight"]) * cfg["hidden_size"] ** 0.5,
                  sd["layers.0.input_layernorm.weight"], cfg["rms_norm_eps"])
    q = (h @ sd["layers.0.self_attn.q_proj.weight"].T)[:, :256]
    k = h @ sd["layers.0.self_attn.k_proj.weight"].T
    logits = (q @ k.T) * cfg["query_pre_attn_scalar"] ** -0.5
    assert logits.abs().max() > 50, logits.abs().max()
    on = R.Gemma2Ref(cfg, sd, torch.float32, softcap=True).encode([ids])[0]
    off = R.Gemma2Ref(cfg, sd, torch.float32, softcap=False).encode([ids])[0]
    assert R.rel_l2(on, off) > 1e-3
    hf_on, hf_off = _hf_rows(hf, torch.float32, 50.0)[2], _hf_rows(hf, torch.float32, None)[2]
    assert R.rel_l2(hf_on, hf_off) > 1e-3


# ------------------------------------------------------------------------------------------------------------------ loader
@pytest.fixture()
def tiny(tmp_path):
    cfg = R.tiny_config(num_hidden_layers=1)
    return cfg, R.random_state_dict(cfg, seed=1), str(tmp_path / "text_encoder")


def test_single_file_and_sharded_layouts_load_the_same(tiny, tmp_path):
    cfg, sd, d = tiny
    R.save_pretrained_layout(d, cfg, sd)
    d2 = str(tmp_path / "sharded")
    R.save_pretrained_layout(d2, cfg, sd, prefix="model.", shards=3, extra={"lm_head.weight": torch.zeros(4, 4)})
    _, a = G.load_text_encoder_dir(d)
    _, b = G.load_text_encoder_dir(d2)
    assert sorted(a) == sorted(b) == sorted(sd) and "lm_head.weight" not in b
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], sd[k]) for k in sd)


def test_a_dropped_and_an_extra_key_are_named(tiny):
    cfg, sd, d = tiny
    drop = "layers.0.mlp.up_proj.weight"
    R.save_pretrained_layout(d, cfg, {k: v for k, v in sd.items() if k != drop})
    with pytest.raises(KeyError, match="up_proj"):
        G.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, sd, extra={"layers.0.self_attn.q_norm.weight": torch.zeros(8)})
    with pytest.raises(KeyError, match="q_norm"):
        G.load_text_encoder_dir(d)
    R.save_pretrained_layout(d, cfg, {**sd, "norm.weight": torch.zeros(8)})
    with pytest.raises(ValueError, match="norm.weight"):
        G.load_text_encoder_dir(d)


@pytest.mark.parametrize("over", [{"hidden_activation": "gelu"}, {"attention_bias": True}, {"head_dim": 128}])
def test_refused_configs(tiny, over):
    cfg, sd, d = tiny
    R.save_pretrained_layout(d, {**cfg, **over}, sd)
    with pytest.raises(NotImplementedError):
        G.load_text_encoder_dir(d)


def test_rope_tables_are_the_restatement_s():
    for a, b in zip(G.rope_tables(256, 10000.0, 40), R.rope_tables(256, 10000.0, 40, BF)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ prompt rules
WORDS = [f"w{i}" for i in range(40)] + ["a", "cat"]


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    tk = pytest.importorskip("tokenizers")
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.processors import TemplateProcessing
    vocab = {"<pad>": 0, "<unk>": 1, "<bos>": 2, **{w: 3 + i for i, w in enumerate(WORDS)}}
    tok = tk.Tokenizer(WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = Whitespace()
    tok.post_processor = TemplateProcessing(single="<bos> $A", special_tokens=[("<bos>", 2)])
    d = tmp_path_factory.mktemp("tok")
    tok.save(str(d / "tokenizer.json"))
    return EP.load_tokenizer(str(d))


class StubEncoder:
    """Row r of a prompt's embedding is (r + 1) in every channel: shows which rows the rules pick."""
    H = 16

    def encode(self, prompts, max_batch=None):
        return [(torch.arange(1, len(p) + 1, dtype=torch.float32)[:, None] * torch.ones(1, self.H)).to(BF) for p in prompts]


def test_lower_strip_bos_truncation_and_the_empty_prompt(tokenizer):
    ids, n = EP.tokenize_prompts(tokenizer, ["  A Cat ", "", " ".join(WORDS * 10)])
    assert n == 300
    assert ids[0] == [2, 3 + WORDS.index("a"), 3 + WORDS.index("cat")]                 # lowered: no <unk>
    assert ids[1] == [2]
    assert len(ids[2]) == 300 and ids[2][0] == 2 and ids[2][1] == 3
    embs = EP.extract_embeddings(StubEncoder(), tokenizer, ["  A Cat ", ""])
    assert [tuple(e.shape) for e in embs] == [(3, 16), (1, 16)]


@pytest.mark.parametrize("words", [2, 400])
def test_instruction_form_keeps_row_0_and_the_last_299(tokenizer, words):
    chi = EP.COMPLEX_HUMAN_INSTRUCTION
    n_chi = len(tokenizer.encode("\n".join(chi)).ids)
    prompt = " ".join((WORDS * 10)[:words])
    ids, max_all = EP.tokenize_prompts(tokenizer, [prompt], chi)
    assert max_all == n_chi + 300 - 2
    L = len(ids[0])
    assert L == min(n_chi + words, max_all) and ids[0][0] == 2
    emb, mask = EP.encode_prompt(StubEncoder(), tokenizer, [prompt], chi)
    assert emb.shape == (1, 300, 16) and mask.shape == (1, 300) and mask.dtype == torch.int64
    # the pipeline's own order of work: pad on the right to max_length_all, then index embeddings and mask
    padded = torch.zeros(max_all, 16)
    padded[:L] = torch.arange(1, L + 1, dtype=torch.float32)[:, None]
    pmask = torch.zeros(max_all, dtype=torch.int64)
    pmask[:L] = 1
    index = [0] + list(range(-300 + 1, 0))
    assert torch.equal(emb[0].float(), padded[index].to(BF).float()) and torch.equal(mask[0], pmask[index])
    assert mask[0, 0] == 1 and int(mask.sum()) == (300 if words == 400 else 1 + max(0, L - (max_all - 299)))


def test_validation_entries(tokenizer):
    out = EP.validation_embeddings(StubEncoder(), tokenizer, ["a cat", "w1 w2"])
    assert len(out) == 2
    for pe, pm, ne, nm in out:
        assert pe.shape == ne.shape == (1, 300, 16) and pm.shape == nm.shape == (1, 300) and pe.dtype == BF
        assert int(nm.sum()) == 1 and nm[0, 0] == 1 and not ne[0, 1:].any()              # "" is BOS alone


# ----------------------------------------------------------------------------------------------------------------- trainer
def test_extract_embeddings_without_a_text_encoder_names_the_directory(tmp_path):
    import train_sana
    m = train_sana.SanaModel.__new__(train_sana.SanaModel)      # host check only: no model, no device
    m.params = SimpleNamespace(pretrained_pipe_path=str(tmp_path / "pipe"))
    with pytest.raises(NotImplementedError) as e:
        m.extract_embeddings(["a"])
    assert os.path.join(str(tmp_path / "pipe"), "text_encoder") in str(e.value)
    assert m.encode_validation_prompts() is None


# ------------------------------------------------------------------------------------------------------------ command line
def test_command_line_file_layouts(tokenizer, tmp_path, capsys):
    from yat_amd import extract_latents
    from yat_amd.common.trainer import Model
    (tmp_path / "img0.txt").write_text(" A Cat \n")
    (tmp_path / "img1.txt").write_text("")
    (tmp_path / "prompts.txt").write_text("a cat\nw1 w2 w3\n")
    EP.main(["--pipe", "unused", "--empty", str(tmp_path / "empty_embeds.pt"), "--validation", str(tmp_path / "prompts.txt"),
             str(tmp_path / "validation_embeds.pt"), str(tmp_path / "img0.txt"), str(tmp_path / "img1.txt")],
            loader=lambda pipe, device, softcap: (StubEncoder(), tokenizer))
    e0 = extract_latents.load_embedding(str(tmp_path / "img0.png"))                 # the sidecar extract_latents reads
    e1 = extract_latents.load_embedding(str(tmp_path / "img1.png"))
    assert e0.shape == (3, 16) and e1.shape == (1, 16) and e0.dtype == BF
    empty = torch.load(tmp_path / "empty_embeds.pt", map_location="cpu")
    checked = Model.check_empty_embeddings(None, empty, "empty_embeds.pt")           # the trainer's reader
    assert len(checked) == 1 and checked[0].shape == (1, 16) and checked[0].dtype == BF
    val = torch.load(tmp_path / "validation_embeds.pt", map_location="cpu")
    assert len(val) == 2 and all(len(v) == 4 and v[0].shape == (1, 300, 16) and v[1].shape == (1, 300) for v in val)
