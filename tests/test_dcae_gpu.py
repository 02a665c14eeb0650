"""DC-AE decoder on the GPU: each new kernel against fp32 torch, the whole decoder at SANA's widths against the restatement
(tests/dcae_ref.py) in the project's bar style, and the trainer's validation images (yat_amd/dcae.py, csrc/dcae.hip)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dcae_ref
from tests.gpu_common import BF, DEV, ROOT, _rbf, _rel

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- conv3x3
CONV_CASES = [
    # B, Cin, Cout, H, W, upsample, shortcut mode, silu, residual
    (1, 32, 1024, 8, 8, False, 1, False, False),        # conv_in: latent 32 -> 1024, repeat shortcut
    (1, 64, 128, 13, 11, False, 0, True, False),        # odd grid, ResBlock conv1 (bias + SiLU)
    (2, 128, 128, 33, 17, False, 0, False, True),       # residual, batch 2
    (1, 256, 128, 18, 22, True, 2, False, False),       # DCUpBlock2d 256 -> 128 (r = 2)
    (1, 1024, 1024, 8, 10, True, 2, False, False),      # DCUpBlock2d 1024 -> 1024 (r = 4)
    (1, 512, 256, 16, 16, False, 0, True, True),
    (1, 96, 64, 7, 9, False, 0, False, False),          # Cin not a multiple of 64: taps change inside a K-tile
    (1, 32, 32, 256, 256, False, 0, False, False),      # large grid, narrow channels
    (1, 128, 3, 37, 29, False, 0, False, False),        # conv_out, Cout = 3 (direct kernel, NCHW output)
    (1, 128, 3, 20, 20, True, 0, True, True),           # direct kernel with upsample / SiLU / residual (NHWC)
]


@pytest.mark.parametrize("B,Cin,Cout,H,W,up,sc,silu,res", CONV_CASES)
def test_conv3x3_against_fp32(B, Cin, Cout, H, W, up, sc, silu, res):
    from yat_amd import ops
    g = torch.Generator().manual_seed(Cin * 7 + Cout + H)
    hi, wi = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(B, Cin, hi, wi, generator=g).to(BF)
    x[:, :, 0, :] += 1.0                                                    # asymmetric data: a transpose does not pass
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(BF)
    b = (0.1 * torch.randn(Cout, generator=g)).to(BF)
    sc_ch = {0: 0, 1: Cin, 2: Cin}[sc]
    r = torch.randn(B, Cout, H, W, generator=g).to(BF) if res else None
    # torch, fp32 arithmetic over the same bf16 values, rounded at the module boundaries
    xi = F.interpolate(x.float(), scale_factor=2, mode="nearest") if up else x.float()
    ref = _rbf(F.conv2d(xi, w.float(), b.float(), padding=1))
    if silu:
        ref = _rbf(F.silu(ref))
    if sc == 1:
        ref = _rbf(ref + x.float().repeat_interleave(Cout // Cin, dim=1))
    elif sc == 2:
        ref = _rbf(ref + F.pixel_shuffle(x.float().repeat_interleave(4 * Cout // Cin, dim=1), 2))
    if res:
        ref = _rbf(ref + r.float())
    nchw = Cout <= 4 and not (up or silu or res)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    y = torch.empty(B, Cout, H, W, dtype=BF, device=DEV) if nchw else torch.empty(B, H, W, Cout, dtype=BF, device=DEV)
    ops.dcae_conv3x3(xd, w.permute(0, 2, 3, 1).contiguous().to(DEV), y, B, H, W, Cin, Cout, bias=b.to(DEV), upsample=up,
                     silu=silu, shortcut_mode=sc, shortcut=xd if sc else None, shortcut_channels=sc_ch,
                     residual=r.permute(0, 2, 3, 1).contiguous().to(DEV) if res else None, out_nchw=nchw)
    torch.cuda.synchronize()
    got = y.cpu().float() if nchw else y.cpu().float().permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    # summation order only: one bf16 rounding step of the result at most
    assert err.max().item() <= 2.0 ** -6 * ref.abs().max().item() + 1e-6, err.max().item()
    assert _rel(got, ref) <= 4e-3


def test_msla_aggregate_against_fp32():
    from yat_amd import ops
    g = torch.Generator().manual_seed(11)
    B, C3, H, W = 2, 192, 19, 70                                             # W > 64: two pixel segments per row
    x = torch.randn(B, C3, H, W, generator=g).to(BF)
    wdw = (torch.randn(C3, 1, 5, 5, generator=g) / 5).to(BF)
    wpw = (torch.randn(C3, 32, 1, 1, generator=g) / 32 ** 0.5).to(BF)
    t = _rbf(F.conv2d(x.float(), wdw.float(), padding=2, groups=C3))
    ref = _rbf(F.conv2d(t, wpw.float(), groups=C3 // 32))
    out = torch.empty(B, H, W, C3, dtype=BF, device=DEV)
    ops.dcae_msla_aggregate(x.permute(0, 2, 3, 1).contiguous().to(DEV), wdw.reshape(C3, 25).contiguous().to(DEV),
                            wpw.reshape(C3, 32).contiguous().to(DEV), out, B, H, W, C3)
    got = out.cpu().float().permute(0, 3, 1, 2)
    assert _rel(got, ref) <= 4e-3
    assert (got - ref).abs().max().item() <= 2.0 ** -6 * ref.abs().max().item()


@pytest.mark.parametrize("D,res,relu", [(128, True, False), (1024, True, False), (96, False, True), (24, False, False)])
def test_rmsnorm_bias_against_torch(D, res, relu):
    from yat_amd import ops
    g = torch.Generator().manual_seed(D)
    M = 777
    x = (3 * torch.randn(M, D, generator=g) + 0.5).to(BF)
    w = (1 + 0.3 * torch.randn(D, generator=g)).to(BF)
    b = (0.2 * torch.randn(D, generator=g)).to(BF)
    r = torch.randn(M, D, generator=g).to(BF) if res else None
    ref = dcae_ref.rms_norm(x.reshape(M, D, 1, 1), w, b).reshape(M, D)           # bf16, diffusers' rounding
    if res:
        ref = ref + r
    if relu:
        ref = F.relu(ref)
    yd = r.to(DEV) if res else torch.empty(M, D, dtype=BF, device=DEV)
    ops.dcae_rmsnorm_bias(x.to(DEV), w.to(DEV), b.to(DEV), yd, 1e-5, residual=yd if res else None, relu=relu)
    got = yd.cpu()
    diff = (got.float() - ref.float()).abs()
    # the fp32 sum order may move rsqrt by an ulp and flip the rounding of x * rsqrt: one bf16 step of that product (times
    # w), carried through the later roundings -- bounded by two steps of the magnitudes that enter the sums
    rs = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    scale = (x.float() * rs).abs() * w.float().abs() + b.float().abs() + (r.float().abs() if res else 0)
    assert (diff <= scale.clamp_min(1e-3) * 2.0 ** -6).all(), diff.max().item()
    assert (diff == 0).float().mean().item() >= 0.99


def test_image_to_uint8_is_exact():
    from yat_amd import ops
    g = torch.Generator().manual_seed(2)
    crafted = torch.tensor([2 * (k + 0.5) / 255 - 1 for k in range(255)] + [-1.0, 1.0, -5.0, 5.0, 0.0, -0.0])
    x = torch.cat([crafted, 1.2 * torch.randn(3 * 61 * 47 - crafted.numel(), generator=g)]).to(BF).reshape(1, 3, 61, 47)
    got = ops.dcae_image_to_uint8(x.to(DEV)).cpu().numpy()
    assert np.array_equal(got, dcae_ref.postprocess(x))


# ------------------------------------------------------------------------------------------------------- whole decoder
@pytest.fixture(scope="module")
def sana_vae(tmp_path_factory):
    from safetensors.torch import save_file
    d = tmp_path_factory.mktemp("dcae") / "vae"
    d.mkdir()
    sd = dcae_ref.random_state(dcae_ref.SANA_F32C32, seed=3)
    sd["encoder.conv_in.weight"] = torch.zeros(8, 3, 3, 3)                   # encoder keys are ignored by the decoder
    save_file({k: v.to(BF).contiguous() for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    (d / "config.json").write_text(json.dumps(dcae_ref.diffusers_config(dcae_ref.SANA_F32C32)))
    from yat_amd.dcae import AutoencoderDCDecoderHIP
    return AutoencoderDCDecoderHIP.from_pretrained(str(d), device=DEV), {k: v.to(BF) for k, v in sd.items()}


@pytest.mark.parametrize("h,w", [(8, 8), (24, 42), (32, 32)])
def test_decoder_sana_widths_against_restatement(sana_vae, h, w):
    dec, sd = sana_vae
    g = torch.Generator().manual_seed(h * 100 + w)
    lat = torch.randn(1, 32, h, w, generator=g).to(BF)
    img = dec.decode(lat)
    torch.cuda.synchronize()
    assert img.shape == (1, 3, 32 * h, 32 * w) and img.dtype == BF
    with torch.backends.cudnn.flags(enabled=False):                          # torch's own conv kernels
        r16 = dcae_ref.decode(dcae_ref.SANA_F32C32, sd, lat.to(DEV), BF)
        r32 = dcae_ref.decode(dcae_ref.SANA_F32C32, sd, lat.to(DEV), torch.float32)
    e_h, e_b, e_hb = _rel(img, r32), _rel(r16, r32), _rel(img, r16)
    print(f"[dcae {h}x{w}] rel_l2 hip_vs_fp32={e_h:.3e} bf16_ref_vs_fp32={e_b:.3e} hip_vs_bf16_ref={e_hb:.3e}")
    assert torch.isfinite(img.float()).all()
    assert e_h <= 1.1 * e_b, (e_h, e_b)
    assert e_h <= 3e-2 and e_hb <= 5e-2
    u_h = dec.to_uint8(img).cpu().numpy().astype(np.int32)
    u_b = dcae_ref.postprocess(r16).astype(np.int32)
    u_t = dcae_ref.postprocess(r32).astype(np.int32)
    f_hb, f_ht, f_bt = [(np.abs(a - b) <= 2).mean() for a, b in ((u_h, u_b), (u_h, u_t), (u_b, u_t))]
    print(f"[dcae {h}x{w}] uint8 within +-2: hip_vs_bf16_ref={f_hb:.4f} hip_vs_fp32={f_ht:.4f} bf16_ref_vs_fp32={f_bt:.4f}")
    # two bf16 evaluations of this random full-depth decoder sit ~1.3e-2 apart (as far as each is from the fp32 truth), so
    # a fixed 99 % of pixels within +-2 does not hold even between the restatement's bf16 and fp32 runs: the HIP image is
    # held to the bf16 restatement's own closeness to the truth, and to an absolute floor against the bf16 restatement
    assert f_ht >= f_bt - 0.01, (f_ht, f_bt)
    assert f_hb >= 0.95, f_hb


def test_decoder_refuses_quadratic_grids(sana_vae):
    dec, _ = sana_vae
    with pytest.raises(ValueError):
        dec.decode(torch.zeros(1, 32, 4, 8, dtype=BF))


# ------------------------------------------------------------------------------------------------------------ trainer
TINY6 = {"latent_channels": 8, "block_out_channels": [32, 32, 32, 64, 64, 64],
         "block_types": ["ResBlock"] * 3 + ["EfficientViTBlock"] * 3, "layers_per_block": [1] * 6, "scaling_factor": 0.5}


def test_trainer_logs_decoded_validation_images(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    from safetensors.torch import save_file
    from train_sana import SanaModel
    from tests.test_trainer_gpu import _write_shards
    from yat_amd.common.tb_writer import read_events
    from yat_amd.common.training_parameters_reader import TrainingParameters
    from yat_amd.sana import SanaConfig
    cfg = SanaConfig(num_layers=2, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2,
                     cross_attention_head_dim=64, cross_attention_dim=128, caption_channels=96, in_channels=8, out_channels=8,
                     sample_size=32)
    vae = tmp_path / "pipe" / "vae"
    vae.mkdir(parents=True)
    save_file({k: v.to(BF).contiguous() for k, v in dcae_ref.random_state(TINY6, seed=4).items()},
              str(vae / "diffusion_pytorch_model.safetensors"))
    (vae / "config.json").write_text(json.dumps(dcae_ref.diffusers_config(TINY6)))
    paths = _write_shards(tmp_path, cfg)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", *[f"  - {p}" for p in paths], "num_shards: 2", "dataset_seed: 7",
        "batch_size: 4", "learning_rate: 1e-3", "steps: 2", "num_steps_per_validation: 2", "validation_prompts:",
        "  - a red fox", "bfloat16: true", "aspect_ratio: 1024", f"pretrained_pipe_path: {tmp_path / 'pipe'}", ""]))
    g = torch.Generator().manual_seed(1)
    pe = torch.randn(1, 12, cfg.caption_channels, generator=g).to(BF)
    torch.save([(pe, torch.ones(1, 12, dtype=torch.long), torch.zeros(1, 12, cfg.caption_channels, dtype=BF),
                 torch.cat([torch.ones(1, 1, dtype=torch.long), torch.zeros(1, 11, dtype=torch.long)], 1))],
               tmp_path / "validation_embeds.pt")
    monkeypatch.chdir(tmp_path)
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    trainer = SanaModel(params, config=cfg)
    assert trainer.vae_dir == str(vae) and trainer.vae is None
    trainer.run()
    torch.cuda.synchronize()
    steps = sorted(os.listdir(tmp_path / "models"), key=int)
    ck = tmp_path / "models" / steps[0]
    assert (ck / "validation_latents.pt").exists()
    png = (ck / "validation_0.png").read_bytes()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    ev = read_events(trainer.logger.path)
    imgs = [e for e in ev if e.get("tag") == "validation/0/a red fox" and "image" in e]
    assert imgs and (imgs[0]["image"]["colorspace"], imgs[0]["image"]["height"], imgs[0]["image"]["width"]) == (3, 1024, 1024)
    assert any(e.get("tag") == "validation_latents/0" and "image" in e for e in ev)
    # the CLI turns the saved latents into PNGs
    out = tmp_path / "png"
    r = subprocess.run([sys.executable, "-m", "yat_amd.dcae", "--vae", str(vae), str(ck / "validation_latents.pt"), str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (out / "validation_0.png").read_bytes()[:8] == png[:8]
