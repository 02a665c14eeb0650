"""``compute_features`` without a GPU: the raw shard reader, ``BucketSamplerExtractFeatures`` over a stub model with the host
resize, and the trainer's choice of sampler."""
import io
import os
import sys
import tarfile
import types

import numpy as np
import pytest
import torch
from PIL import Image

from yat_amd.common.aspect_ratios import ASPECT_RATIO_256_BIN
from yat_amd.common.bucket_sampler import BucketSampler, BucketSamplerExtractFeatures
from yat_amd.common.shards import read_raw_shard
from yat_amd.common.trainer import HipAccelerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(300, 300), (200, 330), (310, 290), (150, 250)]          # h, w -> buckets 1.0, 0.6, 1.07, 0.6 of the 256 table


def _png(arr, mode=None):
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, format="PNG")
    return buf.getvalue()


def _add(tar, name, payload):
    info = tarfile.TarInfo(name)
    info.size = len(payload)
    tar.addfile(info, io.BytesIO(payload))


def write_raw_shard(path, count, seed=0, image_dir=None):
    """``count`` PNG + caption samples over SIZES -> [(key, png bytes, caption)]; the PNGs also as files in ``image_dir``."""
    rng = np.random.default_rng(seed)
    out = []
    with tarfile.open(path, "w") as tar:
        for i in range(count):
            h, w = SIZES[i % len(SIZES)]
            key, caption = f"{seed:03d}{i:06d}", f"caption {seed} {i} " + "x " * (i % 5)
            png = _png(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            _add(tar, key + ".png", png)
            _add(tar, key + ".txt", caption.encode())
            _add(tar, key + ".json", b'{"url": "unused"}')
            if image_dir is not None:
                with open(os.path.join(image_dir, key + ".png"), "wb") as f:
                    f.write(png)
            out.append((key, png, caption))
    return out


def test_read_raw_shard(tmp_path):
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, (5, 6, 4), dtype=np.uint8)
    grey = rng.integers(0, 256, (4, 8), dtype=np.uint8)
    jpg = io.BytesIO()
    Image.fromarray(rgb).save(jpg, format="JPEG")
    path = str(tmp_path / "00000.tar")
    with tarfile.open(path, "w") as tar:
        _add(tar, "a/000.JPG", jpg.getvalue())                    # upper-case extension, a directory in the name
        _add(tar, "a/000.txt", "a café".encode("utf-8"))
        _add(tar, "a/000.json", b"{}")
        _add(tar, "001.json", b"{}")                              # the json first: still one sample
        _add(tar, "001.txt", b"rgba")
        _add(tar, "001.png", _png(rgba, "RGBA"))
        _add(tar, "002.png", _png(grey, "L"))
        _add(tar, "002.txt", b"grey")
        _add(tar, "003.png", _png(rgb)[:60])                      # truncated: dropped and counted
        _add(tar, "003.txt", b"broken")
        _add(tar, "004.png", _png(rgb))                           # no caption: incomplete
        _add(tar, "005.txt", b"\xff\xfe bad utf-8")
        _add(tar, "005.png", _png(rgb))
        _add(tar, "006.jpeg", jpg.getvalue())
        _add(tar, "006.txt", b"last")
    lines = []
    got = list(read_raw_shard(path, report=lines.append))
    assert [s["__key__"] for s in got] == ["a/000", "001", "002", "006"]
    assert [s["caption"] for s in got] == ["a café", "rgba", "grey", "last"]
    for s in got:
        assert s["image"].dtype == np.uint8 and s["image"].ndim == 3 and s["image"].shape[2] == 3
        assert s["image"].flags["C_CONTIGUOUS"]
    assert got[0]["image"].shape == (9, 7, 3) and np.array_equal(got[0]["image"], got[3]["image"])
    assert np.array_equal(got[1]["image"], np.asarray(Image.fromarray(rgba, "RGBA").convert("RGB")))
    assert np.array_equal(got[2]["image"], np.stack([grey] * 3, axis=-1))
    assert len(lines) == 1 and path in lines[0] and "4 sample(s), 3 dropped" in lines[0]


class StubModel:
    """``aspect_ratios`` + recording extractors: a latent is the image's 8 x 8 block means, an embedding the caption's bytes."""

    def __init__(self, pooled=False):
        self.aspect_ratios = ASPECT_RATIO_256_BIN
        self.latent_calls, self.text_calls, self.images, self.pooled = [], [], [], pooled

    def extract_latents_uint8(self, images_u8, generator=None):
        assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3
        assert isinstance(generator, torch.Generator)
        self.latent_calls.append(images_u8.shape[0])
        self.images += [im.clone() for im in images_u8]
        x = images_u8.permute(0, 3, 1, 2).float()
        noise = torch.rand(1, generator=generator)
        return torch.nn.functional.avg_pool2d(x, 8) / 255.0 + noise

    def extract_embeddings(self, captions):
        self.text_calls.append(len(captions))
        embs = [torch.tensor(list(c.encode()), dtype=torch.float32)[:, None].repeat(1, 4).to(torch.bfloat16) for c in captions]
        return [(e, e[0]) for e in embs] if self.pooled else embs


def _sampler(paths, model, **kw):
    kw = {"batch_size": 3, "seed": 5, "vae_max_batch_size": 2, "text_encoder_max_batch_size": 1, "device_resize": False, **kw}
    return BucketSamplerExtractFeatures([], HipAccelerator(1, device="cpu"), model=model, local_paths=paths, **kw)


def test_sampler_buckets_chunks_and_hands_over_pillow_images(tmp_path):
    from yat_amd.extract_latents import resized_uint8
    samples = []
    for s in range(2):
        samples += write_raw_shard(str(tmp_path / f"{s:05d}.tar"), 12, seed=s, image_dir=str(tmp_path))
    paths = [str(tmp_path / f"{s:05d}.tar") for s in range(2)]
    by_caption = {c: key for key, _, c in samples}
    model = StubModel()
    sampler = _sampler(paths, model)
    assert sampler.decode_ahead == 2 * 3                            # a few batches of decoded photographs, not 16 * batch_size
    assert all(b.maxlen == 4 * 3 for b in sampler.buckets.values())
    it = iter(sampler)
    seen = set()
    for _ in range(6):
        n_img = len(model.images)
        model.latent_calls.clear()
        model.text_calls.clear()
        batch = next(it)
        th, tw = (int(v) for v in ASPECT_RATIO_256_BIN[str(batch.ratio)])
        seen.add(batch.ratio)
        assert model.latent_calls == [2, 1] and model.text_calls == [1, 1, 1]          # the two max-batch settings
        assert batch.vae_features.shape == (3, 3, th // 8, tw // 8) and batch.vae_features.dtype == torch.bfloat16
        assert not batch.vae_features.is_cuda and len(batch.embeddings) == 3
        handed = model.images[n_img:]
        assert all(tuple(im.shape) == (th, tw, 3) for im in handed)                    # every batch is one ratio
        for im, emb in zip(handed, batch.embeddings):
            caption = bytes(emb[:, 0].to(torch.int64).tolist()).decode()
            key, want = resized_uint8(str(tmp_path / (by_caption[caption] + ".png")), ASPECT_RATIO_256_BIN)
            assert float(key) == batch.ratio and torch.equal(im, want)
    assert seen == {1.0, 0.6, 1.07}
    t = sampler._producer[0]
    assert t.is_alive()
    sampler.close()
    assert not t.is_alive() and sampler._producer is None
    # the same shards and seed: the same batches, noise included; SD3.5's (emb, pooled) pairs pass through
    a, b = iter(_sampler(paths, StubModel())), iter(_sampler(paths, StubModel(pooled=True), decode_ahead=0))
    for _ in range(3):
        x, y = next(a), next(b)
        assert x.ratio == y.ratio and torch.equal(x.vae_features, y.vae_features)
        assert all(isinstance(e, tuple) and torch.equal(e[0], f) for e, f in zip(y.embeddings, x.embeddings))
    a.close()
    other = next(iter(_sampler(paths, StubModel(), seed=6, decode_ahead=0)))
    first = next(iter(_sampler(paths, StubModel(), decode_ahead=0)))
    assert not (other.ratio == first.ratio and torch.equal(other.vae_features, first.vae_features))


def test_a_full_bucket_drops_its_oldest(tmp_path):
    write_raw_shard(str(tmp_path / "00000.tar"), 4)
    sampler = _sampler([str(tmp_path / "00000.tar")], StubModel(), batch_size=2, decode_ahead=0)
    bucket = sampler.buckets[1.0]
    assert bucket.maxlen == 8
    for i in range(11):
        sampler.process_element({"image": np.full((40, 40, 3), i, dtype=np.uint8), "caption": str(i)})
    assert len(bucket) == 8 and [c for _, c in bucket] == [str(i) for i in range(3, 11)]
    assert all(tuple(im.shape) == (256, 256, 3) and int(im[0, 0, 0]) == int(c) for im, c in bucket)


def _trainer(tmp_path, monkeypatch, extra):
    sys.path.insert(0, ROOT)
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    write_raw_shard(str(tmp_path / "00000.tar"), 4)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", f"  - {tmp_path / '00000.tar'}", "num_shards: 1", "dataset_seed: 7",
        "batch_size: 2", "learning_rate: 1e-3", "steps: 1", "num_steps_per_validation: 100", "validation_prompts:", "  - x",
        "bfloat16: true", f"pretrained_pipe_path: {tmp_path / 'pipe'}", *extra, ""]))
    monkeypatch.chdir(tmp_path)
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    m = SanaModel.__new__(SanaModel)                                # the sampler choice needs no transformer
    m.params, m.accelerator = params, HipAccelerator(1, device="cpu")
    m.aspect_ratios, m.shard_index_begin, m.shard_index_end = ASPECT_RATIO_256_BIN, 0, 1
    m.vae_dir = None
    return m


def test_make_sampler_without_compute_features_is_the_cached_sampler(tmp_path, monkeypatch):
    m = _trainer(tmp_path, monkeypatch, [])
    s = m.make_sampler()
    assert type(s) is BucketSampler and s.decode_ahead == 16 * 2


def test_make_sampler_names_the_missing_directories(tmp_path, monkeypatch):
    extra = ["compute_features: true", "vae_max_batch_size: 2", "text_encoder_max_batch_size: 1"]
    m = _trainer(tmp_path, monkeypatch, extra)
    with pytest.raises(NotImplementedError, match=r"needs the DC-AE in .*pipe/vae"):
        m.make_sampler()
    m.vae_dir = str(tmp_path / "pipe" / "vae")                      # a VAE, but no text encoder: the other error, still here
    with pytest.raises(NotImplementedError, match=r"needs the Gemma-2 encoder in .*pipe/text_encoder"):
        m.make_sampler()
    from yat_amd.common.trainer import Model
    base = Model.__new__(Model)
    base.params = m.params
    base.shard_index_begin, base.shard_index_end = 0, 1
    with pytest.raises(NotImplementedError):
        base.make_sampler()
    with pytest.raises(NotImplementedError):
        base.extract_latents_uint8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
