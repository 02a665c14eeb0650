"""The Gemma-2 text-encoder kernels (csrc/gemma.hip), the whole encoder (yat_amd/gemma2.py) and the SANA trainer's text side on
the GPU, against torch and the restatement of tests/gemma2_ref.py (pinned to transformers in tests/test_gemma2_cpu.py).
Tolerances: ``close()`` / ``as_good_as()`` of tests/gpu_common.py at their defaults; the whole-encoder bar is stated there."""
import ctypes
import os
import sys

import pytest
import torch

from tests import gemma2_ref as R
from tests.gpu_common import BF, DEV, _collect_failures, as_good_as, close, rel  # noqa: F401

pytestmark = pytest.mark.gpu
DH = 256


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ embed
@pytest.mark.parametrize("hidden", [256, 2304])
@pytest.mark.parametrize("rows", [1, 65, 300])
def test_embed_rows(hidden, rows):
    from yat_amd import ops
    vocab = 97
    table = _randn(vocab, hidden, seed=hidden)
    g = torch.Generator().manual_seed(rows)
    ids = torch.randint(0, vocab, (rows,), generator=g)
    ids[0] = vocab - 1
    if rows > 3:
        ids[1], ids[2], ids[3] = 0, vocab - 1, 0              # both ends, with repeats
    scale = torch.tensor(hidden ** 0.5).to(BF)
    want = torch.nn.functional.embedding(ids.to(DEV), table) * scale.to(DEV)
    out = torch.full((rows, hidden), 7.0, dtype=BF, device=DEV)
    ops.embed_rows(ids.to(torch.int32).to(DEV), table, float(scale), out)
    assert torch.equal(out, want)
    for bad in (-1, vocab):
        ids2 = ids.clone()
        ids2[-1] = bad
        with pytest.raises(ValueError, match="vocabulary"):
            ops.embed_rows(ids2.to(torch.int32).to(DEV), table, float(scale), out)


# ---------------------------------------------------------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("D", [256, 2304])
@pytest.mark.parametrize("M", [1, 3, 64, 301])
def test_gemma_rmsnorm(D, M):
    from yat_amd import ops
    x = _randn(M, D, seed=M + D, scale=3.0)
    res = _randn(M, D, seed=M + D + 1)
    for wname, w in (("w~0", _randn(D, seed=2, scale=0.3)), ("w~-1", (_randn(D, seed=3, scale=0.05).float() - 1.0).to(BF))):
        want = R.rmsnorm(x.float(), w.float(), 1e-6)               # fp32 truth; the module rounds it once
        y = torch.empty_like(x)
        ops.gemma_rmsnorm(x, w, y, 1e-6)
        close(y, want.to(BF), f"rmsnorm {M}x{D} {wname}")
        # With the residual the kernel adds its own rounded norm output, bit for bit.  Against the fp32 truth the sum cannot
        # be held to ulps of ITSELF: where a norm output lies within fp32 rounding of a bf16 tie (a few dozen of 7e5
        # elements, whatever the summation order) and the residual nearly cancels it, that one-ulp difference of the larger
        # operand is many ulps of the small sum.  So close() gets one bf16 ulp of the largest norm output (2^-7 of it) as
        # its absolute term; the norm output itself is held to close() at its defaults above.
        y2 = torch.empty_like(x)
        ops.gemma_rmsnorm(x, w, y2, 1e-6, residual=res)
        assert torch.equal(y2, res + y)
        close(y2, res + want.to(BF), f"rmsnorm+res {M}x{D} {wname}", atol=2.0 ** -7 * float(want.abs().max()))
        y3 = res.clone()
        ops.gemma_rmsnorm(x, w, y3, 1e-6, residual=y3)              # in place on the residual
        assert torch.equal(y3, y2)


# ------------------------------------------------------------------------------------------------------------------- rope
def _packed(lens):
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.tensor(lens).cumsum(0)
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens])
    return off, pos


def test_rope_qk():
    from yat_amd import ops
    from yat_amd.gemma2 import rope_tables
    lens, Hq, Hkv = [1, 65, 300], 8, 4
    off, pos = _packed(lens)
    rows, ld = int(off[-1]), (Hq + 2 * Hkv) * DH
    qkv = _randn(rows, ld, seed=11)
    cos, sin = (t.to(DEV) for t in rope_tables(DH, 10000.0, 320))
    want = qkv.clone()
    for b, n in enumerate(lens):                                   # positions restart per prompt
        blk = qkv[int(off[b]):int(off[b + 1]), :(Hq + Hkv) * DH].view(n, Hq + Hkv, DH).transpose(0, 1)
        rot = R.apply_rope(blk, cos[:n], sin[:n])                  # the bf16 restatement
        want[int(off[b]):int(off[b + 1]), :(Hq + Hkv) * DH] = rot.transpose(0, 1).reshape(n, -1)
    got = qkv.clone()
    ops.rope_qk(got, Hq + Hkv, DH, pos.to(DEV), cos, sin)
    assert torch.equal(got[:, :(Hq + Hkv) * DH], want[:, :(Hq + Hkv) * DH])
    assert torch.equal(got[:, (Hq + Hkv) * DH:], qkv[:, (Hq + Hkv) * DH:])          # v: bit-identical
    assert not torch.equal(got[1:, :DH], qkv[1:, :DH])


# -------------------------------------------------------------------------------------------------------------- attention
SCALE = DH ** -0.5


def _attn_hip(qkv, lens, Hq, Hkv, cap, max_len=None):
    from yat_amd import ops
    off, _ = _packed(lens)
    out = torch.full((qkv.shape[0], Hq * DH), 3.0, dtype=BF, device=DEV)
    ops.gemma_attn_fwd(qkv, off.to(torch.int32).to(DEV), len(lens), Hq, Hkv, DH, max_len or max(lens), SCALE, cap, out)
    return out


def _attn_ref(qkv, lens, Hq, Hkv, cap, dtype):
    off, _ = _packed(lens)
    outs = []
    for b, n in enumerate(lens):
        blk = qkv[int(off[b]):int(off[b + 1])].to(dtype)
        q = blk[:, :Hq * DH].view(n, Hq, DH).transpose(0, 1)
        k = blk[:, Hq * DH:(Hq + Hkv) * DH].view(n, Hkv, DH).transpose(0, 1)
        v = blk[:, (Hq + Hkv) * DH:].view(n, Hkv, DH).transpose(0, 1)
        outs.append(R.eager_attention(q, k, v, SCALE, cap or None))
    return torch.cat(outs)


def _attn_data(lens, Hq, Hkv, seed=0):
    """q and k ~ N(0, 6^2): a logit q k^T scale has std 6^2 * sqrt(256) / 16 = 36, so |s scale| passes 100; v ~ N(0, 1)."""
    rows = sum(lens)
    qkv = _randn(rows, (Hq + 2 * Hkv) * DH, seed=seed)
    qkv[:, :(Hq + Hkv) * DH] = (qkv[:, :(Hq + Hkv) * DH].float() * 6.0).to(BF)
    return qkv


@pytest.mark.parametrize("heads", [(8, 4), (2, 1), (4, 4), (8, 1)])
@pytest.mark.parametrize("lens", [[1], [2], [63], [64], [65], [129], [300], [513], [1, 65, 300, 17]], ids=str)
def test_attention(lens, heads):
    Hq, Hkv = heads
    qkv = _attn_data(lens, Hq, Hkv, seed=sum(lens) + Hq)
    if sum(lens) >= 63:
        q, k = qkv[-60:, :DH].float(), qkv[-60:, Hq * DH:Hq * DH + DH].float()
        assert (q @ k.T).abs().max() * SCALE >= 100
    for cap in (50.0, 0.0):
        truth = _attn_ref(qkv, lens, Hq, Hkv, cap, torch.float32)
        flow = _attn_ref(qkv, lens, Hq, Hkv, cap, BF)
        as_good_as(_attn_hip(qkv, lens, Hq, Hkv, cap), flow, truth, f"attn {lens} {Hq}/{Hkv} cap={cap}")


def test_attention_moderate_logits_match_the_bf16_flow():
    """At ordinary logits the bf16 eager formula is itself close to the truth, so as_good_as() also holds the kernel to it."""
    lens, Hq, Hkv = [65, 300], 8, 4
    qkv = _randn(sum(lens), (Hq + 2 * Hkv) * DH, seed=4)
    for cap in (50.0, 0.0):
        truth = _attn_ref(qkv, lens, Hq, Hkv, cap, torch.float32)
        flow = _attn_ref(qkv, lens, Hq, Hkv, cap, BF)
        assert rel(flow, truth) <= 6e-3
        as_good_as(_attn_hip(qkv, lens, Hq, Hkv, cap), flow, truth, f"attn moderate cap={cap}")


def test_attention_is_causal_and_prompts_are_isolated():
    lens, Hq, Hkv = [65, 300, 17], 8, 4
    qkv = _attn_data(lens, Hq, Hkv, seed=9)
    base = _attn_hip(qkv, lens, Hq, Hkv, 50.0)
    for i in (0, 15, 16, 63, 64, 200):                              # k and v at positions > i of prompt 1
        changed = qkv.clone()
        changed[65 + i + 1:65 + 300, Hq * DH:] = _randn(300 - i - 1, 2 * Hkv * DH, seed=i + 1)
        out = _attn_hip(changed, lens, Hq, Hkv, 50.0)
        assert torch.equal(out[65:65 + i + 1], base[65:65 + i + 1]), i
        assert not torch.equal(out[65 + i + 1:365], base[65 + i + 1:365])
        assert torch.equal(out[:65], base[:65]) and torch.equal(out[365:], base[365:])
    changed = qkv.clone()
    changed[65:365] = _randn(300, qkv.shape[1], seed=77)            # all of prompt 1: q, k and v
    out = _attn_hip(changed, lens, Hq, Hkv, 50.0)
    assert torch.equal(out[:65], base[:65]) and torch.equal(out[365:], base[365:])
    assert not torch.equal(out[65:365], base[65:365])
    # a larger max_len (more, empty query tiles) changes nothing
    assert torch.equal(_attn_hip(qkv, lens, Hq, Hkv, 50.0, max_len=1024), base)


@pytest.mark.parametrize("heads", [(8, 4), (2, 1), (4, 4), (8, 1), (6, 2)])
def test_query_head_reads_its_kv_head(heads):
    Hq, Hkv = heads
    lens = [70, 33]
    qkv = _attn_data(lens, Hq, Hkv, seed=2)
    v = qkv[:, (Hq + Hkv) * DH:].view(-1, Hkv, DH)
    for h in range(Hkv):
        v[:, h] = float(h + 1)                                     # a distinct constant per kv head
    out = _attn_hip(qkv, lens, Hq, Hkv, 50.0).view(-1, Hq, DH)
    for h in range(Hq):
        assert torch.equal(out[:, h], torch.full_like(out[:, h], float(h // (Hq // Hkv) + 1))), h


def test_attention_bad_arguments_return_einval():
    from yat_amd import lib
    L = lib.load()
    qkv = _randn(16, 16 * DH, seed=1)
    out = torch.full((16, 8 * DH), 3.0, dtype=BF, device=DEV)
    off = torch.tensor([0, 16], dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(Hq=8, Hkv=4, dh=DH, max_len=16):
        return L.yat_gemma_attn_fwd(1, 16, Hq, Hkv, dh, max_len, SCALE, 50.0, ctypes.c_void_p(qkv.data_ptr()), qkv.stride(0), 0,
                                    Hq * dh, (Hq + Hkv) * dh, ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                    out.stride(0), st)
    assert call(dh=128) == -1 and call(Hq=6, Hkv=4) == -1 and call(max_len=1025) == -1
    torch.cuda.synchronize()
    assert (out == 3.0).all()                                       # nothing was launched
    assert call() == 0


# ------------------------------------------------------------------------------------------------------------------ geglu
@pytest.mark.parametrize("M,N", [(1, 512), (65, 9216), (301, 512)])
def test_geglu(M, N):
    from yat_amd import ops
    gu = _randn(M, 2 * N, seed=M + N, scale=2.0)
    out = torch.empty(M, N, dtype=BF, device=DEV)
    ops.geglu(gu, N, out)
    want = torch.nn.functional.gelu(gu[:, :N].float(), approximate="tanh").to(BF) * gu[:, N:]
    close(out, want, f"geglu {M}x{N}")


# ---------------------------------------------------------------------------------------------------------- whole encoder
def _prompts(vocab, lens=(1, 23, 300), seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, vocab, (n,), generator=g) for n in lens]


# Measured on an MI355X over the three prompts (1, 23, 300 tokens) -- e_h: HIP vs the fp32 restatement, e_b: the bf16
# restatement vs the fp32 one:   tiny  e_h = 4.870e-3, e_b = 6.576e-3      real width  e_h = 4.115e-3, e_b = 4.118e-3
# The absolute caps are 1.5 x the measured e_h.
ENCODER_CAP = {"tiny": 1.5 * 4.870e-3, "real": 1.5 * 4.115e-3}


@pytest.mark.parametrize("name", ["tiny", "real"])
def test_whole_encoder_against_restatement(name, tmp_path):
    from yat_amd.gemma2 import Gemma2EncoderHIP
    cfg = R.tiny_config() if name == "tiny" else R.real_width_config()
    sd = R.random_state_dict(cfg, seed=3, logit_gain=6.0 if name == "tiny" else 1.0)
    d = str(tmp_path / "text_encoder")
    R.save_pretrained_layout(d, cfg, {k: v.to(BF) for k, v in sd.items()}, prefix="model.", shards=2 if name == "real" else 1)
    enc = Gemma2EncoderHIP.from_pretrained(d, device=DEV)
    print(enc.describe())
    prompts = _prompts(cfg["vocab_size"])
    hip = enc.encode(prompts)
    sdb = {k: v.to(BF) for k, v in sd.items()}                      # both restatements start from the stored bf16 weights
    truth = R.Gemma2Ref(cfg, sdb, torch.float32, DEV).encode(prompts)
    flow = R.Gemma2Ref(cfg, sdb, BF, DEV).encode(prompts)
    hip2 = enc.encode(list(reversed(prompts)), max_batch=2)          # another packing, chunked: the same rows
    for p, a in zip(prompts, hip):
        assert a.shape == (p.numel(), cfg["hidden_size"]) and a.dtype == BF
        assert torch.isfinite(a.float()).all()
    e_h = rel(torch.cat(hip), torch.cat(truth))
    e_b = rel(torch.cat(flow), torch.cat(truth))
    e_2 = rel(torch.cat(list(reversed(hip2))), torch.cat(truth))
    print(f"[gemma2] whole encoder {name}: e_h={e_h:.3e} e_b={e_b:.3e} e_h(other packing)={e_2:.3e}")
    assert e_h <= 1.1 * e_b and e_2 <= 1.1 * e_b, (e_h, e_2, e_b)
    assert e_h <= ENCODER_CAP[name], (e_h, ENCODER_CAP[name])
    with pytest.raises(NotImplementedError, match="beyond"):
        enc.encode([torch.ones(1025, dtype=torch.long)])
    with pytest.raises(ValueError, match="vocabulary"):
        enc.encode([torch.tensor([1, cfg["vocab_size"]])])


def test_softcap_flag_changes_the_result(tmp_path):
    from yat_amd.gemma2 import Gemma2EncoderHIP
    cfg = R.tiny_config()
    sd = {k: v.to(BF) for k, v in R.random_state_dict(cfg, seed=3, logit_gain=6.0).items()}
    on, off = Gemma2EncoderHIP(cfg, sd, DEV), Gemma2EncoderHIP(cfg, sd, DEV, softcap=False)
    assert "soft-capped at 50" in on.describe() and "NOT soft-capped" in off.describe()
    p = _prompts(cfg["vocab_size"], lens=(70,))
    a, b = on.encode(p)[0], off.encode(p)[0]
    truth_off = R.Gemma2Ref(cfg, sd, torch.float32, DEV, softcap=False).encode(p)[0]
    flow_off = R.Gemma2Ref(cfg, sd, BF, DEV, softcap=False).encode(p)[0]
    assert rel(a, b) > 1e-3
    assert rel(b, truth_off) <= 1.1 * rel(flow_off, truth_off)


# ---------------------------------------------------------------------------------------------------------------- trainer
def _pipe_dir(tmp_path, cfg, sd):
    import tokenizers
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.processors import TemplateProcessing
    pipe = tmp_path / "pipe"
    R.save_pretrained_layout(str(pipe / "text_encoder"), cfg, sd)
    words = ["a", "cat", "x", "user", "prompt"]
    vocab = {"<pad>": 0, "<unk>": 1, "<bos>": 2, **{w: 3 + i for i, w in enumerate(words)}}
    tok = tokenizers.Tokenizer(WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = Whitespace()
    tok.post_processor = TemplateProcessing(single="<bos> $A", special_tokens=[("<bos>", 2)])
    os.makedirs(pipe / "tokenizer")
    tok.save(str(pipe / "tokenizer" / "tokenizer.json"))
    return str(pipe)


def test_sana_trainer_encodes_its_own_prompts(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests.test_trainer_gpu import _write_shards
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    from yat_amd.sana import SanaConfig
    tcfg = R.tiny_config()
    sd = {k: v.to(BF) for k, v in R.random_state_dict(tcfg, seed=3).items()}
    pipe = _pipe_dir(tmp_path, tcfg, sd)
    cfg = SanaConfig(num_layers=1, num_attention_heads=2, attention_head_dim=32, num_cross_attention_heads=2,
                     cross_attention_head_dim=32, cross_attention_dim=64, caption_channels=tcfg["hidden_size"], in_channels=8,
                     out_channels=8, sample_size=32)
    paths = _write_shards(tmp_path, cfg)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", *[f"  - {p}" for p in paths], "num_shards: 2", "dataset_seed: 7",
        "batch_size: 4", "learning_rate: 1e-3", "steps: 2", "num_steps_per_validation: 100", "validation_prompts:",
        "  - A Cat", "bfloat16: true", "aspect_ratio: 1024", f"pretrained_pipe_path: {pipe}", "train_unconditional_prob: 1.0", ""]))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("YAT_TENSORBOARD", "0")
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    trainer = SanaModel(params, config=cfg)
    embs = trainer.extract_embeddings(["A Cat ", ""])
    ref = R.Gemma2Ref(tcfg, sd, torch.float32, DEV)
    flow = R.Gemma2Ref(tcfg, sd, BF, DEV)
    ids = [torch.tensor([2, 3, 4]), torch.tensor([2])]              # <bos> a cat | <bos>
    truth, fl = ref.encode(ids), flow.encode(ids)
    for e, t in zip(embs, truth):
        assert e.shape == t.shape and e.dtype == BF
    e_h, e_b = rel(torch.cat(embs), torch.cat(truth)), rel(torch.cat(fl), torch.cat(truth))
    print(f"[gemma2] trainer extract_embeddings: e_h={e_h:.3e} e_b={e_b:.3e}")
    assert e_h <= 1.1 * e_b
    # CFG dropout on every step, and no empty_embeds.pt anywhere: the empty prompt is encoded
    seen, inner = [], trainer.optimize

    def spy(ratio, latents, embeddings, repa, generator):
        seen.append([e.clone() for e in embeddings])
        return inner(ratio, latents, embeddings, repa, generator)
    trainer.optimize = spy
    trainer.run()
    torch.cuda.synchronize()
    assert len(seen) == 2 and all(torch.equal(e.cpu(), embs[1].cpu()) for es in seen for e in es)
    assert all(float(l) == float(l) for l in trainer.loss_history)
    # validate() without a validation_embeds.pt: the prompts are encoded once, kept, and the encoder's weights freed
    assert not os.path.exists("validation_embeds.pt")
    out = trainer.validate()
    assert len(out) == 1 and out[0].shape == (1, 8, 32, 32) and torch.isfinite(out[0].float()).all()
    assert os.path.isfile(f"models/{trainer.global_step}/validation_latents.pt")
    kept = trainer.validation_embeds
    assert trainer.text_encoder is None and kept[0][0].shape == (1, 300, tcfg["hidden_size"]) and kept[0][1].shape == (1, 300)
    trainer.validate()
    assert trainer.validation_embeds is kept and trainer.text_encoder is None


def test_sana_trainer_refuses_a_mismatched_text_encoder(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train_sana import SanaModel
    from types import SimpleNamespace
    tcfg = R.tiny_config(num_hidden_layers=1)
    pipe = _pipe_dir(tmp_path, tcfg, {k: v.to(BF) for k, v in R.random_state_dict(tcfg, seed=3).items()})
    m = SanaModel.__new__(SanaModel)
    m.params = SimpleNamespace(pretrained_pipe_path=pipe)
    m.accelerator = SimpleNamespace(device=DEV)
    m.model = SimpleNamespace(config=SimpleNamespace(caption_channels=96))
    with pytest.raises(ValueError, match="256.*96"):
        m.extract_embeddings(["a"])
