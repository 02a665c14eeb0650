"""The T5 text-encoder kernels (csrc/t5.hip), the whole encoder (yat_amd/t5.py) and the PixArt-Sigma trainer's text side on the
GPU, against torch and the restatement of tests/t5_ref.py (pinned to transformers in tests/test_t5_cpu.py).  Tolerances:
``close()`` / ``as_good_as()`` of tests/gpu_common.py at their defaults; the whole-encoder bar is stated there."""
import ctypes
import os
import sys

import pytest
import torch

from tests import t5_ref as R
from tests.gpu_common import BF, DEV, _collect_failures, as_good_as, close, rel  # noqa: F401

pytestmark = pytest.mark.gpu
DH = 64


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("D", [128, 4096])
@pytest.mark.parametrize("M", [1, 3, 64, 301])
def test_t5_rmsnorm(D, M):
    from yat_amd import ops
    x = _randn(M, D, seed=M + D, scale=3.0)
    res = _randn(M, D, seed=M + D + 1)
    for wname, w in (("w~0", _randn(D, seed=2, scale=0.3)), ("w~1", (_randn(D, seed=3, scale=0.05).float() + 1.0).to(BF))):
        # the fp32 truth rounded as the module rounds: after the normalisation, and after the weight
        xf = x.float()
        normed = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)).to(BF)
        want = w * normed
        assert torch.equal(want, R.layer_norm(x, w, 1e-6))
        y = torch.full_like(x, 7.0)
        ops.t5_rmsnorm(x, w, y, 1e-6)
        close(y, want, f"t5_rmsnorm {M}x{D} {wname}")
        # with a residual: the stored sum is torch's bf16 add to the bit, and y is the kernel's own norm of that sum
        s = torch.full_like(x, 7.0)
        y2 = torch.full_like(x, 7.0)
        ops.t5_rmsnorm(x, w, y2, 1e-6, residual=res, sum_out=s)
        assert torch.equal(s, res + x)
        y_of_s = torch.empty_like(x)
        ops.t5_rmsnorm(s, w, y_of_s, 1e-6)
        assert torch.equal(y2, y_of_s)
        close(y2, R.layer_norm(res + x, w, 1e-6), f"t5_rmsnorm+res {M}x{D} {wname}")
        r3, y3 = res.clone(), torch.empty_like(x)
        ops.t5_rmsnorm(x, w, y3, 1e-6, residual=r3)                 # in place on the residual
        assert torch.equal(r3, s) and torch.equal(y3, y2)


# -------------------------------------------------------------------------------------------------------------- attention
def _offsets(lens):
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.tensor(lens).cumsum(0)
    return off


def _table(H, max_len, seed=1, std=3.0):
    from yat_amd.t5 import relative_bias_table
    w = torch.randn(32, H, generator=torch.Generator().manual_seed(seed)) * std
    return relative_bias_table(w.to(BF).to(DEV), 32, 128, max_len)


def _attn_hip(qkv, lens, H, table, max_len=None, fill=3.0):
    from yat_amd import ops
    out = torch.full((qkv.shape[0], H * DH), fill, dtype=BF, device=DEV)
    ops.t5_attn_fwd(qkv, _offsets(lens).to(torch.int32).to(DEV), len(lens), H, DH, max_len or max(lens), table, out)
    return out


def _attn_ref(qkv, lens, H, table, max_len, dtype):
    """R.eager_attention per prompt; the [H, L, L] bias is gathered from the per-distance table (the table itself is pinned to
    compute_bias in tests/test_t5_cpu.py)."""
    off = _offsets(lens)
    outs = []
    for b, n in enumerate(lens):
        blk = qkv[int(off[b]):int(off[b + 1])].to(dtype)
        q, k, v = (blk[:, i * H * DH:(i + 1) * H * DH].view(n, H, DH).transpose(0, 1) for i in range(3))
        i, j = torch.arange(n, device=qkv.device)[:, None], torch.arange(n, device=qkv.device)[None, :]
        bias = table[:, (j - i) + max_len - 1].to(dtype)
        outs.append(R.eager_attention(q, k, v, bias))
    return torch.cat(outs)


def _attn_data(lens, H, seed=0, gain=2.5):
    """q and k ~ N(0, gain^2): a logit q . k (no 1 / sqrt(dh)) has std gain^2 * 8 = 50 at 2.5, so |q . k| passes 100;
    v ~ N(0, 1)."""
    qkv = _randn(sum(lens), 3 * H * DH, seed=seed)
    qkv[:, :2 * H * DH] = (qkv[:, :2 * H * DH].float() * gain).to(BF)
    return qkv


@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("lens", [[1], [2], [63], [64], [65], [129], [300], [512], [1, 65, 300, 17]], ids=str)
def test_attention(lens, H):
    qkv = _attn_data(lens, H, seed=sum(lens) + H)
    if sum(lens) >= 63:
        q, k = qkv[-60:, :DH].float(), qkv[-60:, H * DH:H * DH + DH].float()
        assert (q @ k.T).abs().max() >= 100
    max_len = max(lens)
    table = _table(H, max_len, seed=H)
    truth = _attn_ref(qkv, lens, H, table, max_len, torch.float32)
    flow = _attn_ref(qkv, lens, H, table, max_len, BF)
    as_good_as(_attn_hip(qkv, lens, H, table), flow, truth, f"t5 attn {lens} H={H}")


def test_attention_moderate_logits_match_the_bf16_flow():
    """At ordinary logits the bf16 eager formula is itself close to the truth, so as_good_as() also holds the kernel to it."""
    lens, H = [65, 300], 8
    qkv = _randn(sum(lens), 3 * H * DH, seed=4)
    qkv[:, :2 * H * DH] = (qkv[:, :2 * H * DH].float() * 0.25).to(BF)           # q . k of std 0.5: T5 has no 1 / sqrt(dh)
    table = _table(H, 300, std=0.5)
    truth = _attn_ref(qkv, lens, H, table, 300, torch.float32)
    flow = _attn_ref(qkv, lens, H, table, 300, BF)
    assert rel(flow, truth) <= 6e-3
    as_good_as(_attn_hip(qkv, lens, H, table), flow, truth, "t5 attn moderate")


def test_attention_uses_the_bias():
    lens, H = [65, 300, 17], 3
    qkv = _attn_data(lens, H, seed=6, gain=1.0)
    table = _table(H, 300)
    with_bias = _attn_hip(qkv, lens, H, table)
    without = _attn_hip(qkv, lens, H, torch.zeros_like(table))
    assert rel(with_bias, without) > 1e-2
    truth0 = _attn_ref(qkv, lens, H, torch.zeros_like(table), 300, torch.float32)
    as_good_as(without, _attn_ref(qkv, lens, H, torch.zeros_like(table), 300, BF), truth0, "t5 attn zero table")


def _masked_attention(qkv, lens, H, allowed_fn, dtype):
    """Plain softmax attention in torch where ``allowed_fn(i, j)`` says which keys a query sees."""
    off = _offsets(lens)
    outs = []
    for b, n in enumerate(lens):
        blk = qkv[int(off[b]):int(off[b + 1])].to(dtype)
        q, k, v = (blk[:, i * H * DH:(i + 1) * H * DH].view(n, H, DH).transpose(0, 1) for i in range(3))
        i, j = torch.arange(n, device=qkv.device)[:, None], torch.arange(n, device=qkv.device)[None, :]
        w = torch.matmul(q, k.transpose(-1, -2))
        w = w + torch.zeros(n, n, dtype=dtype, device=qkv.device).masked_fill(~allowed_fn(i, j), torch.finfo(dtype).min)
        w = torch.softmax(w, dim=-1)
        outs.append(torch.matmul(w, v).transpose(0, 1).reshape(n, -1))
    return torch.cat(outs)


@pytest.mark.parametrize("direction", ["causal", "anticausal"])
def test_attention_direction_of_the_distance(direction):
    """A table of -30000 on one side of distance 0 turns the kernel into causal (keys j > i dropped) or anti-causal attention:
    the index is key minus query, not the reverse."""
    lens, H, max_len = [65, 300, 17], 3, 300
    qkv = _attn_data(lens, H, seed=8, gain=1.0)
    d = torch.arange(-(max_len - 1), max_len, device=DEV)
    drop = (d > 0) if direction == "causal" else (d < 0)
    table = torch.zeros(H, 2 * max_len - 1, dtype=BF, device=DEV).masked_fill(drop[None, :], -30000.0)

    def allowed(i, j):
        return (j <= i) if direction == "causal" else (j >= i)
    truth = _masked_attention(qkv, lens, H, allowed, torch.float32)
    flow = _masked_attention(qkv, lens, H, allowed, BF)
    as_good_as(_attn_hip(qkv, lens, H, table, max_len), flow, truth, f"t5 attn {direction}")
    other = _masked_attention(qkv, lens, H, lambda i, j: ~allowed(i, j) | (i == j), torch.float32)
    assert rel(truth, other) > 0.1                                  # the two directions are far apart on this data


def test_attention_prompts_are_isolated():
    lens, H = [65, 300, 17], 3
    qkv = _attn_data(lens, H, seed=9)
    table = _table(H, 300)
    base = _attn_hip(qkv, lens, H, table)
    changed = qkv.clone()
    changed[65:365] = _randn(300, qkv.shape[1], seed=77)            # all of prompt 1: q, k and v
    out = _attn_hip(changed, lens, H, table)
    assert torch.equal(out[:65], base[:65]) and torch.equal(out[365:], base[365:])
    assert not torch.equal(out[65:365], base[65:365])
    # a larger max_len (more, empty query tiles; a longer table with the same distances) changes nothing
    for bigger in (301, 320, 512):
        w = torch.randn(32, H, generator=torch.Generator().manual_seed(1)) * 3.0
        from yat_amd.t5 import relative_bias_table
        t2 = relative_bias_table(w.to(BF).to(DEV), 32, 128, bigger)
        assert torch.equal(_attn_hip(qkv, lens, H, t2, max_len=bigger), base), bigger
    # every row of out is written, whatever it held
    for fill in (float("nan"), -7.0):
        assert torch.equal(_attn_hip(qkv, lens, H, table, fill=fill), base)


def test_attention_bad_arguments_return_einval():
    from yat_amd import lib
    L = lib.load()
    H = 2
    qkv = _randn(16, 3 * H * 128, seed=1)
    out = torch.full((16, H * 128), 3.0, dtype=BF, device=DEV)
    off = torch.tensor([0, 16], dtype=torch.int32, device=DEV)
    table = torch.zeros(H, 2 * 513 - 1, dtype=BF, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(H=H, dh=DH, max_len=16, ld=None, k_off=None):
        return L.yat_t5_attn_fwd(1, 16, H, dh, max_len, ctypes.c_void_p(qkv.data_ptr()), ld or qkv.stride(0), 0,
                                 H * dh if k_off is None else k_off, 2 * H * dh, ctypes.c_void_p(table.data_ptr()),
                                 ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(out.data_ptr()), out.stride(0), st)
    assert call(dh=128) == -1 and call(max_len=513) == -1 and call(H=0) == -1
    assert call(ld=qkv.stride(0) - 4) == -1 and call(k_off=H * DH + 4) == -1
    torch.cuda.synchronize()
    assert (out == 3.0).all()                                       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out[:, :H * DH] == 3.0).all()


# ---------------------------------------------------------------------------------------------------------- whole encoder
def _prompts(vocab, lens=(1, 23, 300), seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, vocab, (n,), generator=g) for n in lens]


# Measured on an MI355X over the three prompts (1, 23, 300 tokens) -- e_h: HIP vs the fp32 restatement, e_b: the bf16
# restatement vs the fp32 one:   tiny  e_h = 6.584e-2, e_b = 1.081e-1      real width  e_h = 8.885e-3, e_b = 1.374e-2
# (tiny runs at logit gain 2: its logits reach +-100 with no 1 / sqrt(dh), where the bf16 rounding of q and k alone moves the
# softmax by percents -- in the bf16 module more than here).  The absolute caps are 1.5 x the measured e_h.
ENCODER_CAP = {"tiny": 1.5 * 6.584e-2, "real": 1.5 * 8.885e-3}
GAIN = {"tiny": 2.0, "real": 1.0}


def _encoder(name, tmp_path, zero_bias=False):
    from yat_amd.t5 import T5EncoderHIP
    cfg = R.tiny_config() if name == "tiny" else R.real_width_config()
    sd = R.random_state_dict(cfg, seed=3, logit_gain=GAIN[name])
    if zero_bias:
        sd[R.REL] = torch.zeros_like(sd[R.REL])
    d = str(tmp_path / ("text_encoder" + ("_zero" if zero_bias else "")))
    R.save_pretrained_layout(d, cfg, {k: v.to(BF) for k, v in sd.items()}, shards=2 if name == "real" else 1)
    return cfg, {k: v.to(BF) for k, v in sd.items()}, T5EncoderHIP.from_pretrained(d, device=DEV)


@pytest.mark.parametrize("name", ["tiny", "real"])
def test_whole_encoder_against_restatement(name, tmp_path):
    cfg, sdb, enc = _encoder(name, tmp_path)
    print(enc.describe())
    prompts = _prompts(cfg["vocab_size"])
    hip = enc.encode(prompts)
    truth = R.T5Ref(cfg, sdb, torch.float32, DEV).encode(prompts)   # both restatements start from the stored bf16 weights
    flow = R.T5Ref(cfg, sdb, BF, DEV).encode(prompts)
    hip2 = enc.encode(list(reversed(prompts)), max_batch=2)          # another packing, chunked: the same rows
    for p, a in zip(prompts, hip):
        assert a.shape == (p.numel(), cfg["d_model"]) and a.dtype == BF
        assert torch.isfinite(a.float()).all()
    e_h = rel(torch.cat(hip), torch.cat(truth))
    e_b = rel(torch.cat(flow), torch.cat(truth))
    e_2 = rel(torch.cat(list(reversed(hip2))), torch.cat(truth))
    print(f"[t5] whole encoder {name}: e_h={e_h:.3e} e_b={e_b:.3e} e_h(other packing)={e_2:.3e}")
    assert e_h <= 1.1 * e_b and e_2 <= 1.1 * e_b, (e_h, e_2, e_b)
    assert e_h <= ENCODER_CAP[name], (e_h, ENCODER_CAP[name])
    with pytest.raises(NotImplementedError, match="beyond"):
        enc.encode([torch.ones(513, dtype=torch.long)])
    with pytest.raises(ValueError, match="vocabulary"):
        enc.encode([torch.tensor([1, cfg["vocab_size"]])])


def test_whole_encoder_uses_the_relative_bias(tmp_path):
    cfg, _, enc = _encoder("tiny", tmp_path)
    _, _, enc0 = _encoder("tiny", tmp_path, zero_bias=True)
    p = _prompts(cfg["vocab_size"], lens=(70,))
    assert rel(enc.encode(p)[0], enc0.encode(p)[0]) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- trainer
WORDS = [f"w{i}" for i in range(40)] + ["a", "cat"]


def _pipe_dir(tmp_path, cfg, sd):
    """A PixArt-Sigma pipe directory: text_encoder/ in the transformers layout and tokenizer/spiece.model trained here."""
    import sentencepiece as spm
    pipe = tmp_path / "pipe"
    R.save_pretrained_layout(str(pipe / "text_encoder"), cfg, sd)
    os.makedirs(pipe / "tokenizer")
    corpus = tmp_path / "corpus.txt"
    corpus.write_text("\n".join(" ".join(WORDS[i:] + WORDS[:i]) for i in range(len(WORDS))) + "\n")
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(pipe / "tokenizer" / "spiece"), vocab_size=60,
                                   model_type="unigram", hard_vocab_limit=False, pad_id=0, eos_id=1, unk_id=2, bos_id=-1,
                                   minloglevel=2)
    return str(pipe), spm.SentencePieceProcessor(model_file=str(pipe / "tokenizer" / "spiece.model"))


def _write_pixart_shards(tmp_path, cfg):
    from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN
    from yat_amd.common.shards import write_shard
    g = torch.Generator().manual_seed(0)
    paths = []
    for s in range(2):
        samples = []
        for i in range(16):
            r = ["1.0", "0.5", "2.0"][(i + s) % 3]
            H, W = ASPECT_RATIO_1024_BIN[r]
            L = int(torch.randint(3, 40, (1,), generator=g))
            samples.append(dict(__key__=f"{s:03d}{i:05d}", ratio=r,          # 1024 px bucket / 32: small latents, same ratios
                                latent=(torch.randn(4, int(H) // 32, int(W) // 32, generator=g) * 0.5).to(BF),
                                emb=torch.randn(L, cfg.caption_channels, generator=g).to(BF)))
        p = str(tmp_path / f"shard-{s:06d}.tar")
        write_shard(p, samples)
        paths.append(p)
    return paths


def test_pixart_trainer_encodes_its_own_prompts(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train_pixart_sigma import PixartSigmaTrainer
    from yat_amd.common.training_parameters_reader import TrainingParameters
    from yat_amd.pixart import PixArtConfig
    tcfg = R.tiny_config()
    sd = {k: v.to(BF) for k, v in R.random_state_dict(tcfg, seed=3).items()}
    pipe, sp = _pipe_dir(tmp_path, tcfg, sd)
    cfg = PixArtConfig(num_layers=2, num_attention_heads=2, attention_head_dim=24, cross_attention_dim=48,
                       caption_channels=tcfg["d_model"], sample_size=128)
    paths = _write_pixart_shards(tmp_path, cfg)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", *[f"  - {p}" for p in paths], "num_shards: 2", "dataset_seed: 7",
        "batch_size: 4", "learning_rate: 1e-3", "steps: 2", "num_steps_per_validation: 100", "validation_prompts:",
        "  - A Cat", "bfloat16: true", "aspect_ratio: 1024", f"pretrained_pipe_path: {pipe}", "train_unconditional_prob: 1.0",
        "text_encoder_max_batch_size: 1", ""]))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("YAT_TENSORBOARD", "0")
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    trainer = PixartSigmaTrainer(params, config=cfg)
    embs = trainer.extract_embeddings(["A Cat ", ""])
    ids = [torch.tensor(sp.encode("a cat") + [1]), torch.tensor([1])]                # pieces of the lowered text, </s> | </s>
    truth = R.T5Ref(tcfg, sd, torch.float32, DEV).encode(ids)
    fl = R.T5Ref(tcfg, sd, BF, DEV).encode(ids)
    for e, t in zip(embs, truth):
        assert e.shape == t.shape and e.dtype == BF
    assert embs[1].shape == (1, tcfg["d_model"])
    e_h, e_b = rel(torch.cat(embs), torch.cat(truth)), rel(torch.cat(fl), torch.cat(truth))
    print(f"[t5] trainer extract_embeddings: e_h={e_h:.3e} e_b={e_b:.3e}")
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
    assert len(out) == 1 and out[0].shape[0] == 1 and out[0].shape[-2:] == (128, 128) and torch.isfinite(out[0].float()).all()
    assert os.path.isfile(f"models/{trainer.global_step}/validation_latents.pt")
    kept = trainer.validation_embeds
    assert trainer.text_encoder is None and kept[0][0].shape == (1, 300, tcfg["d_model"]) and kept[0][1].shape == (1, 300)
    assert int(kept[0][1].sum()) == len(ids[0]) and int(kept[0][3].sum()) == 1
    trainer.validate()
    assert trainer.validation_embeds is kept and trainer.text_encoder is None


def test_pixart_trainer_refuses_a_mismatched_text_encoder(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train_pixart_sigma import PixartSigmaTrainer
    from types import SimpleNamespace
    tcfg = R.tiny_config(num_layers=1)
    pipe, _ = _pipe_dir(tmp_path, tcfg, {k: v.to(BF) for k, v in R.random_state_dict(tcfg, seed=3).items()})
    m = PixartSigmaTrainer.__new__(PixartSigmaTrainer)
    m.params = SimpleNamespace(pretrained_pipe_path=pipe)
    m.accelerator = SimpleNamespace(device=DEV)
    m.model = SimpleNamespace(config=SimpleNamespace(caption_channels=96))
    with pytest.raises(ValueError, match="128.*96"):
        m.extract_embeddings(["a"])
