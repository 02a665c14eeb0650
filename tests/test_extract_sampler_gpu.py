"""``compute_features: true`` on the GPU: the SANA trainer over a raw PNG + caption shard with a tiny DC-AE and a tiny Gemma-2
in its pipe directory (batches bitwise equal to the extractors called directly on Pillow-resized images, a short ``run()``,
a clean exit), the PixArt-Sigma and SD3.5 trainers on a tiny AutoencoderKL (seeded latent noise; their T5 / CLIP pipes are
too heavy to build in seconds, so ``extract_embeddings`` is stubbed there), and ``extract_latents --device-resize``."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_common import BF, DEV, ROOT

pytestmark = pytest.mark.gpu

WORDS = ["a", "cat", "x", "user", "prompt"]


def _raw_shard(tmp, count=12):
    """A raw shard over two ratios of the 256 table (1.0 and 0.6) -> (path, {caption: [H, W, 3] uint8 array})."""
    import io
    import tarfile
    from PIL import Image
    rng = np.random.default_rng(3)
    path, by_caption = str(tmp / "00000.tar"), {}
    with tarfile.open(path, "w") as tar:
        for i in range(count):
            h, w = ((300, 300), (200, 330), (150, 250))[i % 3]
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            caption = " ".join(WORDS[(i + j) % len(WORDS)] for j in range(1 + i))       # distinct, 1 .. count tokens
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, format="PNG")
            for ext, payload in ((".png", buf.getvalue()), (".txt", caption.encode()), (".json", b"{}")):
                info = tarfile.TarInfo(f"{i:05d}{ext}")
                info.size = len(payload)
                tar.addfile(info, io.BytesIO(payload))
            by_caption[caption] = img
    return path, by_caption


def _pillow(img, table, ratio):
    from yat_amd.image import pillow_resize
    th, tw = (int(v) for v in table[str(ratio)])
    return pillow_resize(torch.from_numpy(img), th, tw)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())


def sana_scenario(tmp):
    """Runs in a process of its own (``test_sana_trains_from_a_raw_shard``)."""
    from safetensors.torch import save_file
    from tests import dcae_encoder_ref as enc_ref
    from tests import dcae_ref
    from tests import gemma2_ref as G
    from tests.test_dcae_encoder_gpu import TINY6
    from tests.test_gemma2_gpu import _pipe_dir
    from train_sana import SanaModel
    from yat_amd.common.aspect_ratios import ASPECT_RATIO_256_BIN
    from yat_amd.common.bucket_sampler import BucketSamplerExtractFeatures
    from yat_amd.common.training_parameters_reader import TrainingParameters
    from yat_amd.sana import SanaConfig
    tmp = pathlib.Path(tmp)
    tcfg = G.tiny_config()
    pipe = pathlib.Path(_pipe_dir(tmp, tcfg, {k: v.to(BF) for k, v in G.random_state_dict(tcfg, seed=3).items()}))
    (pipe / "vae").mkdir()
    sd = dict(dcae_ref.random_state(TINY6, seed=4), **enc_ref.random_encoder_state(TINY6, seed=5))
    save_file({k: v.to(BF).contiguous() for k, v in sd.items()}, str(pipe / "vae" / "diffusion_pytorch_model.safetensors"))
    (pipe / "vae" / "config.json").write_text(json.dumps(enc_ref.diffusers_config(TINY6)))
    shard, by_caption = _raw_shard(tmp)
    cfg = SanaConfig(num_layers=1, num_attention_heads=2, attention_head_dim=32, num_cross_attention_heads=2,
                     cross_attention_head_dim=32, cross_attention_dim=64, caption_channels=tcfg["hidden_size"], in_channels=8,
                     out_channels=8, sample_size=8)                         # sample_size * 32 = 256: the 256 table
    (tmp / "config.yaml").write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", f"  - {shard}", "num_shards: 1", "dataset_seed: 7", "batch_size: 4",
        "learning_rate: 1e-3", "steps: 2", "num_steps_per_validation: 100", "validation_prompts:", "  - a cat", "bfloat16: true",
        f"pretrained_pipe_path: {pipe}", "train_unconditional_prob: 0.0", "compute_features: true", "vae_max_batch_size: 2",
        "text_encoder_max_batch_size: 3", ""]))
    os.chdir(tmp)
    params = TrainingParameters()
    params.read_yaml(str(tmp / "config.yaml"))
    trainer = SanaModel(params, config=cfg)
    assert trainer.aspect_ratios is ASPECT_RATIO_256_BIN
    sampler = trainer.make_sampler()
    assert type(sampler) is BucketSamplerExtractFeatures and sampler.device_resize
    assert sampler.vae_max_batch_size == 2 and sampler.text_encoder_max_batch_size == 3
    handed, asked = [], []
    lat_fn, emb_fn = trainer.extract_latents_uint8, trainer.extract_embeddings
    trainer.extract_latents_uint8 = lambda u8, generator=None: (handed.append(u8.cpu()), lat_fn(u8, generator=generator))[1]
    trainer.extract_embeddings = lambda caps: (asked.append(list(caps)), emb_fn(caps))[1]
    it = iter(sampler)
    seen = set()
    for _ in range(6):                                              # (two or three batches reach both ratios)
        if seen == {1.0, 0.6}:
            break
        handed.clear()
        asked.clear()
        batch = next(it)
        seen.add(batch.ratio)
        assert [len(c) for c in asked] == [3, 1] and [h.shape[0] for h in handed] == [2, 2]
        captions = [c for chunk in asked for c in chunk]
        want_u8 = torch.stack([_pillow(by_caption[c], ASPECT_RATIO_256_BIN, batch.ratio) for c in captions])
        assert torch.equal(torch.cat(handed), want_u8), "the device resize is not Pillow's"
        want_lat = torch.cat([lat_fn(want_u8[i:i + 2]).to(BF).cpu() for i in (0, 2)])
        want_emb = [e.cpu() for chunk in (captions[:3], captions[3:]) for e in emb_fn(chunk)]
        assert batch.vae_features.dtype == BF and not batch.vae_features.is_cuda
        assert batch.vae_features.shape == (4, 8, want_u8.shape[1] // 32, want_u8.shape[2] // 32)
        assert torch.equal(batch.vae_features, want_lat)
        assert len(batch.embeddings) == 4 and all(_same(a, b) for a, b in zip(batch.embeddings, want_emb))
        assert all(not e.is_cuda and e.shape[1] == tcfg["hidden_size"] for e in batch.embeddings)
    assert seen == {1.0, 0.6}, seen
    sampler.close()
    trainer.extract_latents_uint8, trainer.extract_embeddings = lat_fn, emb_fn
    trainer.run()
    torch.cuda.synchronize()
    losses = [float(l) for l in trainer.loss_history]
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert type(trainer.sampler) is BucketSamplerExtractFeatures
    print("sana scenario ok", losses)


def test_sana_trains_from_a_raw_shard(tmp_path):
    env = dict(os.environ, YAT_TENSORBOARD="0", PYTHONPATH=ROOT)
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_extract_sampler_gpu import sana_scenario; sana_scenario({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "sana scenario ok" in r.stdout, (r.returncode, r.stderr[-3000:])


def _kl_trainer(cls, config, tmp_path, pipe, monkeypatch):
    from yat_amd.common.training_parameters_reader import TrainingParameters
    yaml_path = tmp_path / f"{cls.__name__}.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "num_shards: 1", "dataset_seed: 7", "batch_size: 2", "learning_rate: 1e-3", "steps: 1",
        "num_steps_per_validation: 1", "validation_prompts:", "  - a red fox", "bfloat16: true", f"pretrained_pipe_path: {pipe}", ""]))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("YAT_TENSORBOARD", "0")
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    return cls(params, config=config)


@pytest.mark.parametrize("recipe", ["pixart", "sd35"])
def test_kl_trainers_sample_reproducible_latents(recipe, tmp_path, monkeypatch):
    """The AutoencoderKL recipes: the sampler's own generator (seed + process_index, on the device) draws the latent noise, so
    the same shard and seed give the same batch and another seed another; SD3.5's ``(emb, pooled)`` pairs arrive as pairs of
    host tensors.  The text side is a stub (module docstring), so the sampler is built directly, not by ``make_sampler``."""
    sys.path.insert(0, ROOT)
    from tests.test_vae_kl_encoder_gpu import TINY_KL, _write_vae
    from yat_amd.common.aspect_ratios import ASPECT_RATIO_256_BIN
    from yat_amd.common.bucket_sampler import BucketSamplerExtractFeatures
    pipe = tmp_path / "pipe"
    _write_vae(pipe / "vae", TINY_KL, seed=5, decoder_too=True)
    if recipe == "pixart":
        from train_pixart_sigma import PixartSigmaTrainer
        from yat_amd.pixart import PixArtConfig
        trainer = _kl_trainer(PixartSigmaTrainer, PixArtConfig(num_layers=2, num_attention_heads=2, attention_head_dim=24,
                                                               cross_attention_dim=48, caption_channels=64, sample_size=32),
                              tmp_path, pipe, monkeypatch)
        assert trainer.aspect_ratios is ASPECT_RATIO_256_BIN                 # sample_size * 8
    else:
        from train_sd35 import SD35Trainer
        from yat_amd.sd3 import SD3Config
        trainer = _kl_trainer(SD35Trainer, SD3Config(sample_size=16, in_channels=16, out_channels=16, num_layers=2,
                                                     attention_head_dim=64, num_attention_heads=2, joint_attention_dim=96,
                                                     caption_projection_dim=128, pooled_projection_dim=64, pos_embed_max_size=24,
                                                     dual_attention_layers=(0,)), tmp_path, pipe, monkeypatch)
        trainer.aspect_ratios = ASPECT_RATIO_256_BIN                         # (the recipe's 1024 table: megapixel images)
    with pytest.raises(NotImplementedError, match="text_encoder"):
        trainer.check_feature_extractors()                                   # the VAE is there, the text encoder is not

    def stub(captions):
        embs = [torch.full((len(c.split()), 8), float(len(c)), dtype=BF, device=DEV) for c in captions]
        return [(e, e[0].clone()) for e in embs] if recipe == "sd35" else embs
    trainer.extract_embeddings = stub
    shard, by_caption = _raw_shard(tmp_path)

    def first_batch(seed):
        s = BucketSamplerExtractFeatures([], trainer.accelerator, 2, model=trainer, seed=seed, local_paths=[shard],
                                         vae_max_batch_size=1, text_encoder_max_batch_size=2, decode_ahead=0)
        return next(iter(s))
    a, b, c = first_batch(7), first_batch(7), first_batch(8)
    assert a.ratio == b.ratio and torch.equal(a.vae_features, b.vae_features)
    assert not (a.ratio == c.ratio and torch.equal(a.vae_features, c.vae_features))
    th, tw = (int(v) for v in ASPECT_RATIO_256_BIN[str(a.ratio)])
    assert a.vae_features.shape == (2, 4, th // 8, tw // 8) and a.vae_features.dtype == BF and not a.vae_features.is_cuda
    assert torch.isfinite(a.vae_features.float()).all()
    # ... and it is the encoder's seeded sample of the Pillow-resized images, with the recipe's shift switch
    gen = torch.Generator(device=DEV).manual_seed(7)
    pairs = a.embeddings
    if recipe == "sd35":
        assert all(isinstance(p, tuple) and len(p) == 2 and p[0].dim() == 2 and p[1].dim() == 1 and not p[0].is_cuda
                   and not p[1].is_cuda for p in pairs)
        lengths = [int(p[0][0, 0]) for p in pairs]
    else:
        assert all(torch.is_tensor(p) and p.dim() == 2 and not p.is_cuda for p in pairs)
        lengths = [int(p[0, 0]) for p in pairs]
    by_length = {len(c): c for c in by_caption}
    assert len(by_length) == len(by_caption)
    imgs = torch.stack([_pillow(by_caption[by_length[n]], ASPECT_RATIO_256_BIN, a.ratio) for n in lengths])
    want = torch.cat([trainer.vae_encoder.encode_uint8(imgs[i:i + 1], apply_shift=trainer.apply_shift, generator=gen)
                      for i in range(2)]).to(BF).cpu()
    assert torch.equal(a.vae_features, want)


def test_extract_latents_device_resize_writes_the_same_bytes(tmp_path):
    from PIL import Image
    from tests.test_vae_kl_encoder_gpu import TINY_KL, _write_vae
    vae = tmp_path / "pipe" / "vae"
    _write_vae(vae, TINY_KL, seed=5)
    rng = np.random.default_rng(0)
    paths = []
    for name, (h, w) in {"a": (150, 250), "b": (201, 203), "c": (350, 200)}.items():
        p = tmp_path / f"{name}.png"
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        torch.save(torch.randn(7, 96).to(BF), tmp_path / f"{name}.emb.pt")
        paths.append(str(p))
    outs = {flag: tmp_path / f"shard-{i:06d}.tar" for i, flag in enumerate(("", "--device-resize"))}
    for flag, out in outs.items():
        cmd = [sys.executable, "-m", "yat_amd.extract_latents", "--vae", str(vae), "--resolution", "256", "--seed", "7",
               *([flag] if flag else []), "--out", str(out), *paths]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    assert outs[""].read_bytes() == outs["--device-resize"].read_bytes()
