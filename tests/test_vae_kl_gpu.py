"""AutoencoderKL decoder on the GPU: GroupNorm and the single-head attention against fp32 torch, the whole decoder at the
SDXL / PixArt-Sigma and SD3.5 widths against the restatement (tests/autoencoder_kl_ref.py) in the project's bar style, and
the PixArt-Sigma / SD3.5 trainers' validation images (yat_amd/autoencoder_kl.py, csrc/vae_kl.hip)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import autoencoder_kl_ref as klref
from tests.gpu_common import BF, DEV, ROOT, _rbf, _rel

pytestmark = pytest.mark.gpu


def _ulp(t):
    """one bf16 step at the magnitude of each element"""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


# ----------------------------------------------------------------------------------------------------------- groupnorm
GN_SHAPES = [
    # B, C, H, W, G, offset
    (1, 128, 32, 32, 32, 0.0),
    (1, 256, 24, 40, 32, 0.0),
    (1, 512, 16, 16, 32, 0.0),
    (1, 512, 37, 23, 32, 0.0),            # odd grid: the last slab is partial
    (2, 256, 19, 45, 32, 0.0),            # two images
    (1, 64, 30, 30, 32, 0.0),             # 2 channels per group: one 8-channel chunk spans four groups
    # large common offsets (mean >> std): a naive E[x^2] - E[x]^2 in fp32 loses the variance
    (1, 256, 40, 48, 32, 300.0),          # std ~ 30: bf16 steps of 2 still resolve the spread
    (1, 128, 17, 29, 8, -1000.0),         # std ~ 60, steps of 4
    (1, 256, 40, 48, 32, -300.0),         # std ~ 1.5 (COARSE below): the inputs take ~8 values per channel
]
COARSE = 1.0                              # the offset / std ratio is 200 instead of 10 - 15
GN_CASES = [s + (silu,) for s in GN_SHAPES for silu in (False, True)] + [
    (1, 256, 1024, 1024, 32, 0.0, True),  # the largest real case: 1024 px, 8 channels x 1 M pixels per group
]


@pytest.mark.parametrize("B,C,H,W,G,off,silu", GN_CASES)
def test_groupnorm_against_fp32(B, C, H, W, G, off, silu):
    from yat_amd import ops
    g = torch.Generator().manual_seed(C * 13 + H + G)
    coarse = off < 0 and -off < 500
    spread = COARSE if coarse or off == 0 else abs(off) / 20
    x = (off + spread * (1 + torch.rand(B, 1, 1, C, generator=g)) * torch.randn(B, H, W, C, generator=g)).to(BF)
    w = (1 + 0.3 * torch.randn(C, generator=g)).to(BF)
    b = (0.2 * torch.randn(C, generator=g)).to(BF)
    # truth: the group norm of the same bf16 values (fp64 statistics and arithmetic), rounded at the module boundaries
    xn = x.permute(0, 3, 1, 2).double()
    ref = F.group_norm(xn, G, w.double(), b.double(), eps=1e-6)
    ref = ref.float().to(BF).float()
    if silu:
        ref = _rbf(F.silu(ref))
    ref = ref.permute(0, 2, 3, 1)
    xd = x.to(DEV)
    ws = torch.empty(ops.vae_groupnorm_workspace_bytes(B, H * W, C, G), dtype=torch.uint8, device=DEV)
    y = torch.empty_like(xd)
    ops.vae_groupnorm(xd, w.to(DEV), b.to(DEV), y, B, H * W, C, G, ws, 1e-6, silu=silu)
    y2 = xd.clone()
    ops.vae_groupnorm(y2, w.to(DEV), b.to(DEV), y2, B, H * W, C, G, ws, 1e-6, silu=silu)          # in place
    torch.cuda.synchronize()
    got = y.cpu().float()
    assert torch.equal(y, y2), "two calls (one in place) differ"
    diff = (got - ref).abs()
    same = (diff == 0).float().mean().item()
    # ulps at the magnitude of the terms of the one rounding, |xhat w| + |b|: where they cancel, a last-bit difference of the
    # fp32 statistics is many steps of the tiny result (SiLU's slope is at most 1.1)
    xhat = F.group_norm(xn, G, eps=1e-6).float().permute(0, 2, 3, 1)
    mag = torch.maximum(ref.abs(), xhat.abs() * w.float().abs() + b.float().abs())
    worst = (diff / _ulp(mag)).max().item()
    print(f"[groupnorm B={B} C={C} {H}x{W} G={G} off={off} silu={silu}] identical={same:.6f} max_ulps={worst:.2f}")
    # on COARSE inputs every output is one of ~8 values per channel, so a flipped rounding flips ~1 / 8 of a channel at once:
    # the share of identical elements is lumpy there and is held to 99 % (a naive variance loses a third of a bf16 step of
    # rstd at this offset and flips far more); the step bound holds everywhere
    assert same >= (0.99 if coarse else 0.999), same
    assert worst <= 2.0, worst


# ----------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("dh,N", [(512, 64), (512, 1008), (512, 16384), (64, 1008), (64, 4096)])
def test_attention_against_fp32(dh, N):
    from yat_amd import ops
    g = torch.Generator().manual_seed(dh + N)
    qkv = torch.randn(N, 3 * dh, generator=g)
    qkv[:, :dh] *= 2.0                                                       # peaked scores: a non-uniform softmax
    qkv[:, 2 * dh:] += 0.5
    qkv = qkv.to(BF)
    q, k, v = qkv[:, :dh], qkv[:, dh:2 * dh], qkv[:, 2 * dh:]
    qd = qkv.to(DEV)
    ref = F.scaled_dot_product_attention(q.float().to(DEV)[None, None], k.float().to(DEV)[None, None],
                                         v.float().to(DEV)[None, None])[0, 0]
    tb = F.scaled_dot_product_attention(q.to(DEV)[None, None], k.to(DEV)[None, None], v.to(DEV)[None, None])[0, 0]
    out = torch.empty(N, dh, dtype=BF, device=DEV)
    ops.vae_attn_fwd(qd[:, :dh], qd[:, dh:2 * dh], qd[:, 2 * dh:], out, 1, N, dh, 3 * dh, dh)
    out2 = torch.full_like(out, float("nan"))
    ops.vae_attn_fwd(qd[:, :dh], qd[:, dh:2 * dh], qd[:, 2 * dh:], out2, 1, N, dh, 3 * dh, dh)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, out2), "two calls differ"
    e_h, e_b = _rel(out, ref), _rel(tb, ref)
    print(f"[attention dh={dh} N={N}] rel_l2 hip={e_h:.3e} torch_bf16={e_b:.3e}")
    assert e_h <= 1.1 * e_b, (e_h, e_b)
    assert e_h <= 6e-3
    assert (out.float() - ref).abs().max().item() <= 0.02 * ref.abs().max().item()


def test_attention_batch_and_strides():
    """B = 2 images of N rows each, q / k / v column blocks of a wider row, output into a wider row."""
    from yat_amd import ops
    g = torch.Generator().manual_seed(5)
    B, N, dh, ld, ldo = 2, 333, 64, 3 * 64 + 8, 64 + 16
    m = torch.randn(B * N, ld, generator=g).to(BF).to(DEV)
    out = torch.zeros(B * N, ldo, dtype=BF, device=DEV)
    ops.vae_attn_fwd(m[:, :dh], m[:, dh:2 * dh], m[:, 2 * dh:3 * dh], out, B, N, dh, ld, ldo)
    torch.cuda.synchronize()
    for b in range(B):
        r = slice(b * N, (b + 1) * N)
        ref = F.scaled_dot_product_attention(m[r, :dh].float()[None], m[r, dh:2 * dh].float()[None],
                                             m[r, 2 * dh:3 * dh].float()[None])[0]
        assert _rel(out[r, :dh], ref) <= 6e-3
    assert (out[:, dh:] == 0).all(), "wrote past dh"


# ------------------------------------------------------------------------------------------------------- whole decoder
def _write_vae(d, cfg, seed):
    from safetensors.torch import save_file
    d.mkdir(parents=True, exist_ok=True)
    sd = klref.random_state(cfg, seed=seed)
    sd["encoder.conv_in.weight"] = torch.zeros(8, 3, 3, 3)                   # encoder keys are ignored by the decoder
    save_file({k: v.to(BF).contiguous() for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text(json.dumps(klref.diffusers_config(cfg)))
    return {k: v.to(BF) for k, v in sd.items()}


@pytest.fixture(scope="module", params=["sdxl", "sd35"])
def kl_vae(request, tmp_path_factory):
    from yat_amd.autoencoder_kl import AutoencoderKLDecoderHIP
    cfg = {"sdxl": klref.SDXL_KL, "sd35": klref.SD35_KL}[request.param]
    d = tmp_path_factory.mktemp("kl") / "vae"
    sd = _write_vae(d, cfg, seed=3)
    return request.param, cfg, AutoencoderKLDecoderHIP.from_pretrained(str(d), device=DEV), sd


@pytest.mark.parametrize("h,w", [(16, 16), (24, 40), (128, 128)])
def test_decoder_against_restatement(kl_vae, h, w):
    name, cfg, dec, sd = kl_vae
    g = torch.Generator().manual_seed(h * 100 + w)
    lat = (torch.randn(1, cfg["latent_channels"], h, w, generator=g) * cfg["scaling_factor"]).to(BF)
    img = dec.decode(lat)
    img2 = dec.decode(lat)
    torch.cuda.synchronize()
    assert img.shape == (1, 3, 8 * h, 8 * w) and img.dtype == BF
    assert torch.equal(img, img2), "two decodes differ"
    with torch.backends.cudnn.flags(enabled=False):                          # torch's own conv kernels
        r16 = klref.decode(cfg, sd, lat.to(DEV), BF)
        r32 = klref.decode(cfg, sd, lat.to(DEV), torch.float32)
    e_h, e_b, e_hb = _rel(img, r32), _rel(r16, r32), _rel(img, r16)
    print(f"[kl {name} {h}x{w}] rel_l2 hip_vs_fp32={e_h:.3e} bf16_ref_vs_fp32={e_b:.3e} hip_vs_bf16_ref={e_hb:.3e}")
    assert torch.isfinite(img.float()).all()
    assert e_h <= 1.1 * e_b, (e_h, e_b)
    assert e_h <= 3e-2 and e_hb <= 5e-2
    u_h = dec.to_uint8(img).cpu().numpy().astype(np.int32)
    u_b = klref.postprocess(r16).astype(np.int32)
    u_t = klref.postprocess(r32).astype(np.int32)
    f_hb, f_ht, f_bt = [(np.abs(a - b) <= 2).mean() for a, b in ((u_h, u_b), (u_h, u_t), (u_b, u_t))]
    print(f"[kl {name} {h}x{w}] uint8 within +-2: hip_vs_bf16_ref={f_hb:.4f} hip_vs_fp32={f_ht:.4f} bf16_ref_vs_fp32={f_bt:.4f}")
    # as in the DC-AE test: two bf16 evaluations of this random full-depth decoder sit ~1.5e-2 apart (each about as far from
    # the fp32 truth), and only 93 - 96 % of the restatement's own bf16 pixels are within +-2 of its fp32 ones; the HIP image is
    # held to the bf16 restatement's closeness to the truth, and to the bf16 restatement about as closely as that
    assert f_ht >= f_bt - 0.01, (f_ht, f_bt)
    assert f_hb >= f_bt - 0.03 and f_hb >= 0.90, (f_hb, f_bt)


def test_deprecated_attention_names_decode_the_same(tmp_path):
    """A checkpoint with ``query`` / ``key`` / ``value`` / ``proj_attn`` as [C, C, 1, 1] decodes bit-identically."""
    from safetensors.torch import save_file
    from yat_amd.autoencoder_kl import AutoencoderKLDecoderHIP
    cfg = dict(klref.SDXL_KL, block_out_channels=[64, 64], layers_per_block=1)
    sd = _write_vae(tmp_path / "new", cfg, seed=9)
    old = {}
    for k, v in sd.items():
        for new, dep in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
            tag = f"attentions.0.{new}."
            if tag in k:
                k = k.replace(tag, f"attentions.0.{dep}.")
                if k.endswith("weight"):
                    v = v.reshape(*v.shape, 1, 1)
        old[k] = v.contiguous()
    (tmp_path / "old").mkdir()
    save_file(old, str(tmp_path / "old" / "diffusion_pytorch_model.safetensors"))
    (tmp_path / "old" / "config.json").write_text((tmp_path / "new" / "config.json").read_text())
    lat = torch.randn(1, 4, 12, 20, generator=torch.Generator().manual_seed(2)).to(BF)
    a = AutoencoderKLDecoderHIP.from_pretrained(str(tmp_path / "new"), device=DEV).decode(lat)
    b = AutoencoderKLDecoderHIP.from_pretrained(str(tmp_path / "old"), device=DEV).decode(lat)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ trainers
TINY_KL = {"latent_channels": 4, "block_out_channels": [32, 32, 64, 64], "layers_per_block": 1, "norm_num_groups": 8,
           "scaling_factor": 0.5, "shift_factor": None, "use_post_quant_conv": True, "mid_block_add_attention": True}


def _check_validation_images(tmp_path, trainer, vae, latent_hw):
    from yat_amd.common.tb_writer import read_events
    steps = sorted(os.listdir(tmp_path / "models"), key=int)
    ck = tmp_path / "models" / steps[0]
    assert (ck / "validation_latents.pt").exists()
    png = (ck / "validation_0.png").read_bytes()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    ev = read_events(trainer.logger.path)
    imgs = [e for e in ev if e.get("tag") == "validation/0/a red fox" and "image" in e]
    h, w = latent_hw
    assert imgs and (imgs[0]["image"]["colorspace"], imgs[0]["image"]["height"], imgs[0]["image"]["width"]) == (3, 8 * h, 8 * w)
    assert any(e.get("tag") == "validation_latents/0" and "image" in e for e in ev)
    out = tmp_path / "png"
    r = subprocess.run([sys.executable, "-m", "yat_amd.autoencoder_kl", "--vae", str(vae), str(ck / "validation_latents.pt"),
                        str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (out / "validation_0.png").read_bytes() == png


def test_pixart_trainer_logs_decoded_validation_images(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    from train_pixart_sigma import PixartSigmaTrainer
    from yat_amd.common.shards import write_shard
    from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN
    from yat_amd.common.training_parameters_reader import TrainingParameters
    from yat_amd.pixart import PixArtConfig
    cfg = PixArtConfig(num_layers=2, num_attention_heads=2, attention_head_dim=24, cross_attention_dim=48,
                       caption_channels=64, sample_size=128)
    vae = tmp_path / "pipe" / "vae"
    _write_vae(vae, TINY_KL, seed=4)
    g = torch.Generator().manual_seed(0)
    samples = []
    for i in range(16):
        r = ["1.0", "0.5", "2.0"][i % 3]
        H, W = ASPECT_RATIO_1024_BIN[r]
        samples.append(dict(__key__=f"{i:07d}", ratio=r, latent=(torch.randn(4, int(H) // 32, int(W) // 32, generator=g) * 0.5).to(BF),
                            emb=torch.randn(int(torch.randint(3, 20, (1,), generator=g)), cfg.caption_channels, generator=g).to(BF)))
    path = str(tmp_path / "shard-000000.tar")
    write_shard(path, samples)
    (tmp_path / "config.yaml").write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", f"  - {path}", "num_shards: 1", "dataset_seed: 7", "batch_size: 4",
        "learning_rate: 1e-3", "steps: 2", "num_steps_per_validation: 2", "validation_prompts:", "  - a red fox",
        "bfloat16: true", "aspect_ratio: 1024", "train_unconditional_prob: 0.0", f"pretrained_pipe_path: {tmp_path / 'pipe'}",
        ""]))
    torch.save([(torch.randn(1, 9, cfg.caption_channels, generator=g).to(BF), torch.ones(1, 9, dtype=torch.long),
                 torch.randn(1, 9, cfg.caption_channels, generator=g).to(BF), torch.ones(1, 9, dtype=torch.long))],
               tmp_path / "validation_embeds.pt")
    monkeypatch.chdir(tmp_path)
    params = TrainingParameters()
    params.read_yaml(str(tmp_path / "config.yaml"))
    trainer = PixartSigmaTrainer(params, config=cfg)
    assert trainer.vae_dir == str(vae) and trainer.vae is None
    trainer.run()
    torch.cuda.synchronize()
    _check_validation_images(tmp_path, trainer, vae, (cfg.sample_size, cfg.sample_size))


def test_sd35_trainer_logs_decoded_validation_images(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    from train_sd35 import SD35Trainer
    from yat_amd.common.shards import write_shard
    from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN
    from yat_amd.common.training_parameters_reader import TrainingParameters
    from yat_amd.sd3 import SD3Config
    cfg = SD3Config(sample_size=16, in_channels=16, out_channels=16, num_layers=2, attention_head_dim=64, num_attention_heads=2,
                    joint_attention_dim=96, caption_projection_dim=128, pooled_projection_dim=64, pos_embed_max_size=24,
                    dual_attention_layers=(0,))
    vae = tmp_path / "pipe" / "vae"
    _write_vae(vae, dict(TINY_KL, latent_channels=16, use_post_quant_conv=False, block_out_channels=[32, 32, 64, 512],
                         shift_factor=0.0609), seed=6)
    g = torch.Generator().manual_seed(0)
    samples = []
    for i in range(24):
        r = ["1.0", "0.5", "2.0"][i % 3]
        Hpx, Wpx = ASPECT_RATIO_1024_BIN[r]
        samples.append(dict(__key__=f"{i:07d}", ratio=r,
                            latent=(torch.randn(cfg.in_channels, int(Hpx) // 128 * 2, int(Wpx) // 128 * 2, generator=g) * 0.5).to(BF),
                            emb=torch.randn(11, cfg.joint_attention_dim, generator=g).to(BF),
                            pooled=torch.randn(cfg.pooled_projection_dim, generator=g).to(BF)))
    path = str(tmp_path / "shard-000000.tar")
    write_shard(path, samples)
    (tmp_path / "config.yaml").write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", f"  - {path}", "num_shards: 1", "dataset_seed: 3", "batch_size: 4",
        "learning_rate: 1e-3", "steps: 2", "num_steps_per_validation: 2", "validation_prompts:", "  - a red fox",
        "bfloat16: true", "aspect_ratio: 1024", f"pretrained_pipe_path: {tmp_path / 'pipe'}", ""]))
    torch.save([(torch.randn(1, 11, cfg.joint_attention_dim, generator=g).to(BF),
                 torch.randn(1, 11, cfg.joint_attention_dim, generator=g).to(BF),
                 torch.randn(1, cfg.pooled_projection_dim, generator=g).to(BF),
                 torch.randn(1, cfg.pooled_projection_dim, generator=g).to(BF))], tmp_path / "validation_embeds.pt")
    monkeypatch.chdir(tmp_path)
    params = TrainingParameters()
    params.read_yaml(str(tmp_path / "config.yaml"))
    trainer = SD35Trainer(params, config=cfg)
    assert trainer.vae_dir == str(vae) and trainer.vae is None
    trainer.run()
    torch.cuda.synchronize()
    _check_validation_images(tmp_path, trainer, vae, (cfg.sample_size, cfg.sample_size))
