"""Aspect-ratio bucket sampler over cached-feature shards (common/bucket_sampler.py:32-274, the cached path).

Kept from the reference: the ``Batch`` container (:32-39), bucketing by the float ``ratio`` of each sample
(:151-156), batches of exactly ``batch_size`` samples of ONE ratio, and the cross-rank lock-step rule -- a bucket
is yielded only when EVERY rank holds a full batch of it, so all ranks train the same (h, w) in the same step
(:229-234).

Changed: the reference runs a barrier plus one all-gather + ``.item()`` per bucket key (33-40
of them) for every ingested sample.  Here each rank reads ahead until it owns at least one full bucket, then ALL
ranks exchange one int32 vector of bucket fill counts (a single MIN all-reduce per yielded batch attempt); the first
key (in table order) that is full everywhere is yielded.  Single-process runs exchange nothing.
Reference defects not reproduced (SURVEY.md App. B-2,5,6): the TypeError in the cached-path constructor call, the
silent discard of surplus samples (`.clear()` :267 -- surplus stays queued here) and the one-shard dead-lock of
``local_file_getter`` (:81-90 -- shards are cycled in a seeded random order here).
Asynchronous feed (the reference runs a producer ``mp.Process`` that fills a queue with shard paths, :203-220, and decodes on
the consumer): here a producer THREAD reads the tars and unpickles the samples (``decode_ahead`` of them, bounded
queue) while the training thread is inside C-ABI launches (ctypes drops the GIL), so shard decode never sits on the step's
critical path.  A thread, not a process: nothing is re-executed or forked once the GPU is initialised, and the decoded CPU
tensors are handed over by reference.  The collectives of the consensus stay on the training thread -- one thread per rank
talks to the process group.  ``decode_ahead=0`` (or ``YAT_SAMPLER_THREAD=0``) decodes synchronously.
On-the-fly VAE / text encoding from raw image + caption shards: ``BucketSamplerExtractFeatures`` below.
Out of scope: R2/HTTP download, Dreambooth, dual-GPU and REPA branches.
"""
from __future__ import annotations

import atexit
import os
import queue
import random
import threading
from collections import deque

import torch
import torch.distributed as dist

from .shards import iter_legacy_cache, read_raw_shard, read_shard


def _rng_to_json(st):
    """``random.Random.getstate()`` as JSON values (version, the 625 words, the cached gauss value)."""
    return [st[0], list(st[1]), st[2]]


def _rng_from_json(st):
    return (int(st[0]), tuple(int(x) for x in st[1]), st[2])


class Batch:
    def __init__(self):
        self.embeddings = None
        self.vae_features = None
        self.repa_features = None
        self.ratio = None
        self.repa_spatial_dims = None
        self.proj_spatial_dims = None


class BucketSampler:
    def __init__(self, shards, accelerator, batch_size, model=None, seed=0, local_paths=None, features_path=None,
                 max_read_ahead=4096, legacy_cache_dir=None, decode_ahead=None):
        self.accelerator = accelerator
        if decode_ahead is None:
            decode_ahead = 0 if os.environ.get("YAT_SAMPLER_THREAD", "1") == "0" else 16 * batch_size
        self.decode_ahead = int(decode_ahead)
        self._producer = None
        self.process_index = accelerator.process_index
        self.num_processes = accelerator.num_processes
        self.batch_size = batch_size
        self.seed = seed
        self.max_read_ahead = max_read_ahead
        keys = list(model.aspect_ratios.keys()) if model is not None else []
        self.keys = [float(k) for k in keys]                      # table order = consensus priority order
        self.buckets = {k: deque() for k in self.keys}
        # resumable position (state_dict / load_state_dict): per bucket item its (shard path, __key__), the stream position of
        # the last element the CONSUMER took, and what a restore left for the stream to start from
        self._refs, self._pos, self._resume, self._restore_cache = {}, None, None, {}
        self.legacy_cache_dir = legacy_cache_dir                  # cache/{idx}.npy tuples (common/cache.py) instead of shards
        if legacy_cache_dir:
            self.paths = []
            return
        if local_paths:
            paths = [p for p in local_paths if os.path.exists(p)]
            if self.num_processes > 1 and len(paths) >= self.num_processes:
                paths = paths[self.process_index::self.num_processes]       # static partition, C10
        else:
            paths = [os.path.join(features_path or ".", s) for s in shards]
        if not paths:
            raise FileNotFoundError("BucketSampler: no local shard found")
        self.paths = paths

    def _read(self, path):
        """The samples of one shard in tar order, each tagged with the shard it came from (a restore hands over the shards it
        has read already)."""
        cached = self._restore_cache.pop(path, None)
        for sample in (cached if cached is not None else self._read_shard(path)):
            sample["__shard__"] = path
            yield sample

    def _read_shard(self, path):
        return read_shard(path)

    def _shard_stream(self, resume=None):
        rng = random.Random(self.seed + self.process_index)
        while self.legacy_cache_dir:
            samples = list(iter_legacy_cache(self.legacy_cache_dir, self.process_index, self.num_processes))
            if not samples:
                raise FileNotFoundError(f"no cache/<idx>.npy sample for rank {self.process_index} in {self.legacy_cache_dir}")
            rng.shuffle(samples)
            yield from samples
        order, start, skip = None, 0, 0
        if resume is not None:
            # the shard the consumer stood in is shuffled again from the generator state taken before its shuffle: the order
            # inside it, the shards after it and every later epoch's order follow without replaying anything
            order, start, skip = list(resume["order"]), int(resume["order_index"]), int(resume["consumed"])
            rng.setstate(_rng_from_json(resume["rng"]))
        while True:
            if order is None:
                order, start = list(self.paths), 0
                rng.shuffle(order)
            for oi in range(start, len(order)):
                cursor = dict(order=order, order_index=oi, rng=rng.getstate())     # shared by the shard's elements
                samples = list(self._read(order[oi]))
                rng.shuffle(samples)                               # webdataset .shuffle(1000) stand-in, seeded
                for j in range(skip, len(samples)):
                    samples[j]["__pos__"] = (cursor, j + 1)
                    yield samples[j]
                skip = 0
            order = None

    @staticmethod
    def _stream_state(pos):
        cursor, consumed = pos
        return dict(order=list(cursor["order"]), order_index=cursor["order_index"], rng=_rng_to_json(cursor["rng"]),
                    consumed=consumed)

    def _prefetched(self, stream):
        """``stream`` drained by a daemon producer thread through a bounded queue; exceptions travel to the consumer.  The
        thread is stopped AND joined when the consumer is closed, by ``close()`` and, at the latest, by an exit hook: a daemon
        thread that is still inside a torch call when the interpreter finalises is ended by the interpreter from within C++
        frames, which aborts the process ("terminate called without an active exception") after the work is done."""
        q = queue.Queue(maxsize=self.decode_ahead)
        stop = threading.Event()
        done = object()

        def put(item):
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.2)
                    return True
                except queue.Full:
                    continue
            return False

        def produce():
            try:
                for item in stream:
                    if not put(item):
                        return
                put(done)
            except BaseException as e:      # noqa: BLE001 -- re-raised on the training thread
                put(e)
        t = threading.Thread(target=produce, name="yat-shard-decode", daemon=True)
        self._producer = (t, stop)
        atexit.register(self.close)
        t.start()
        try:
            while True:
                item = q.get()
                if item is done:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            self._join(t, stop)

    @staticmethod
    def _join(t, stop):
        stop.set()
        if t is not threading.current_thread():
            t.join(timeout=10.0)            # (the producer looks at ``stop`` every 0.2 s and after every decoded shard)

    def close(self):
        prod, self._producer = self._producer, None
        if prod is not None:
            self._join(*prod)
            atexit.unregister(self.close)

    def process_element(self, elem):
        ratio = float(elem["ratio"])
        if ratio not in self.buckets:
            if self.keys and self.num_processes > 1:
                # an unknown ratio must not change the key list on one rank only (the consensus vector is positional):
                # snap to the closest table key
                ratio = min(self.keys, key=lambda k: abs(k - ratio))
            else:
                self.buckets[ratio] = deque()
                self.keys.append(ratio)
        emb = elem["emb.pt"]
        if "pooled.pt" in elem:                   # SD3.5 samples: (prompt_embeds, pooled_projections) travel together
            emb = (emb, elem["pooled.pt"])
        self.buckets[ratio].append((elem["latent.pt"], emb))
        return ratio

    def _make_item(self, elem):
        """The bucket entry of a sample that a restore read again."""
        emb = (elem["emb.pt"], elem["pooled.pt"]) if "pooled.pt" in elem else elem["emb.pt"]
        return (elem["latent.pt"], emb)

    def _ingest(self, elem):
        """One element from the stream into its bucket; the consumer's position moves behind it."""
        key = self.process_element(elem)
        if key is not None and "__key__" in elem:
            refs = self._refs.get(key)
            if refs is None:
                refs = self._refs[key] = deque(maxlen=self.buckets[key].maxlen)     # (a bounded bucket drops its oldest: so does this)
            refs.append((elem.get("__shard__"), elem["__key__"]))
        if "__pos__" in elem:
            self._pos = elem.pop("__pos__")

    def _full_everywhere(self):
        counts = torch.tensor([len(self.buckets[k]) for k in self.keys], dtype=torch.int32)
        if self.num_processes > 1:
            dev = self.accelerator.device if dist.get_backend() == "nccl" else torch.device("cpu")
            counts = counts.to(dev)
            dist.all_reduce(counts, op=dist.ReduceOp.MIN)
            counts = counts.cpu()
        full = (counts >= self.batch_size).nonzero().flatten()
        return self.keys[int(full[0])] if full.numel() else None

    def __iter__(self):
        stream = self._shard_stream(self._resume) if self._resume is not None else self._shard_stream()
        if self.decode_ahead > 0:
            stream = self._prefetched(stream)
        while True:
            # read ahead until this rank owns a full bucket (bounded), then ask everyone
            read = 0
            while not any(len(self.buckets[k]) >= self.batch_size for k in self.keys) and read < self.max_read_ahead:
                self._ingest(next(stream))
                read += 1
            key = self._full_everywhere()
            if key is None:
                # some rank lacks this bucket: everybody ingests a few more samples and retries
                for _ in range(self.batch_size):
                    self._ingest(next(stream))
                continue
            items = [self.buckets[key].popleft() for _ in range(self.batch_size)]
            if key in self._refs:
                for _ in range(min(self.batch_size, len(self._refs[key]))):
                    self._refs[key].popleft()
            yield self.make_batch(key, items)

    def make_batch(self, key, items):
        batch = Batch()
        batch.ratio = key
        batch.vae_features = torch.stack([it[0] for it in items])       # :161-162
        batch.embeddings = [it[1] for it in items]
        return batch

    # ------------------------------------------------------------------ resumable position
    def state_dict(self):
        """The CONSUMER's position after the last batch it was handed, as JSON-able values: a sampler restored from it yields
        exactly the batches the uninterrupted one goes on to yield, at any ``decode_ahead`` (what the producer thread has read
        ahead but not handed over is not consumed).  Bucket entries are kept as (shard path, ``__key__``) references."""
        if self.legacy_cache_dir:
            raise NotImplementedError("the legacy cache/<idx>.npy path keeps no resumable position: use cached-feature shards")
        for k in self.keys:
            if len(self._refs.get(k, ())) != len(self.buckets[k]):
                raise RuntimeError(f"bucket {k}: entries that did not come from the shard stream cannot be saved by reference")
        stream = self._stream_state(self._pos) if self._pos is not None else self._resume
        return dict(version=1, kind=type(self).__name__, seed=self.seed, process_index=self.process_index,
                    num_processes=self.num_processes, batch_size=self.batch_size, keys=list(self.keys), stream=stream,
                    buckets=[[k, [list(r) for r in self._refs.get(k, ())]] for k in self.keys])

    def load_state_dict(self, state):
        """Before the first batch is asked for.  Reads the shards that hold pending bucket entries and nothing else (the
        stream reads the shard it stood in when it starts); never replays the run."""
        if self.legacy_cache_dir:
            raise NotImplementedError("the legacy cache/<idx>.npy path keeps no resumable position: use cached-feature shards")
        if self._producer is not None or self._pos is not None:
            raise RuntimeError("load_state_dict on a sampler that is already being read")
        for name, mine in (("kind", type(self).__name__), ("seed", self.seed), ("process_index", self.process_index),
                           ("num_processes", self.num_processes), ("batch_size", self.batch_size)):
            if state.get(name) != mine:
                raise ValueError(f"sampler state: {name} is {state.get(name)!r}, this sampler's is {mine!r}")
        stream = state.get("stream")
        wanted = {}
        for refs in [refs for _, refs in state["buckets"]] + [self._extra_refs(state)]:
            for path, key in refs:
                wanted.setdefault(path, set()).add(key)
        unknown = (set(wanted) | set(stream["order"] if stream else ())) - set(self.paths)
        if unknown:
            raise ValueError(f"sampler state: shard(s) not in this sampler's list: {sorted(unknown)[:3]}")
        found, current = {}, (stream["order"][stream["order_index"]] if stream else None)
        for path, keys in wanted.items():
            samples = list(self._read_shard(path))
            if path == current:
                self._restore_cache[path] = samples            # (the stream starts in this shard: it is not read twice)
            found.update({(path, s["__key__"]): s for s in samples if s["__key__"] in keys})
        self.keys = [float(k) for k in state["keys"]]
        self.buckets, self._refs = {}, {}
        for k, refs in state["buckets"]:
            k = float(k)
            self.buckets[k], self._refs[k] = self._new_bucket(), self._new_bucket()
            for path, key in refs:
                if (path, key) not in found:
                    raise ValueError(f"sampler state: sample {key!r} is not in {path}")
                self.buckets[k].append(self._make_item(found[(path, key)]))
                self._refs[k].append((path, key))
        self._resume = stream
        self._load_extra(state, found)

    def _new_bucket(self):
        return deque()

    def _extra_refs(self, state):
        """References to samples, beside the bucket entries, that a restore has to read again."""
        return []

    def _load_extra(self, state, found):
        pass


class BucketSamplerExtractFeatures(BucketSampler):
    """``compute_features: true`` (trainer.py:182-199, bucket_sampler.py:324-398): train straight from raw WebDataset shards
    of ``<key>.jpg`` + ``<key>.txt`` as img2dataset writes them.  Everything of the base class is kept -- the producer thread
    with its ``close()`` / join, the seeded shard order, one MIN all-reduce consensus per batch -- and three things change:

    * the producer thread reads tars and decodes images (``read_raw_shard``) and does nothing else: no GPU call leaves the
      training thread.  A decoded photograph is megabytes (12 megapixels: 36 MB), not the ~100 KB of a cached sample, so the
      bounded queue holds ``2 * batch_size`` samples instead of the base's ``16 * batch_size``, and the samples of a shard
      are mixed through a seeded shuffle buffer of ``2 * batch_size`` instead of a shuffle of the whole decoded shard;
    * ``process_element`` buckets by ``find_closest_ratio(h / w)`` over ``model.aspect_ratios`` (first minimum wins, the
      function of ``yat_amd.extract_latents``) and resizes the image AT INGEST to the bucket's ``(th, tw)`` -- on the device
      with ``device_resize=True`` (``yat_amd.image.resize_uint8``: one upload of the decoded image, the HIP kernel, the
      result stays on the device), by Pillow otherwise; both give Pillow's bytes.  The bucket stores ``(resized [th, tw, 3]
      uint8 tensor, caption)``.  Buckets are ``deque(maxlen=4 * batch_size)``: a bucket that the other ranks never fill
      drops its oldest entry (the reference's is ``maxlen=batch_size``, bucket_sampler.py:149), so at most ``len(table) * 4 *
      batch_size`` resized images are resident, ``th * tw * 3`` bytes each (1024 table: ~3 MB each);
    * a yielded batch is stacked to ``[B, th, tw, 3]``, encoded in chunks of ``vae_max_batch_size`` through
      ``model.extract_latents_uint8`` and its captions in chunks of ``text_encoder_max_batch_size`` through
      ``model.extract_embeddings``, and handed over as the cached path hands it over: ``vae_features`` ``[B, C, h, w]`` bf16 and
      ``embeddings`` a list of ``[L, C]`` tensors (SD3.5: ``(emb, pooled)`` pairs), all on the host, so the step's one-copy
      staging and the recipes are untouched (keeping the features on the device is a later change).

    The noise of an AutoencoderKL latent comes from a generator the sampler owns, on the accelerator's device, seeded
    ``seed + process_index``: the same shards and seed give the same batches.
    Out of scope: R2 / HTTP download, Dreambooth, dual-GPU and REPA."""

    def __init__(self, shards, accelerator, batch_size, model, seed=0, local_paths=None, features_path=None,
                 max_read_ahead=4096, decode_ahead=None, vae_max_batch_size=None, text_encoder_max_batch_size=None,
                 device_resize=True):
        super().__init__(shards, accelerator, batch_size, model=model, seed=seed, local_paths=local_paths,
                         features_path=features_path, max_read_ahead=max_read_ahead, decode_ahead=decode_ahead)
        if decode_ahead is None and self.decode_ahead > 0:
            self.decode_ahead = 2 * batch_size
        self.model = model
        self.sizes = {float(k): (int(v[0]), int(v[1])) for k, v in model.aspect_ratios.items()}
        self.buckets = {k: deque(maxlen=4 * batch_size) for k in self.keys}
        self.vae_max_batch_size = int(vae_max_batch_size or batch_size)
        self.text_encoder_max_batch_size = int(text_encoder_max_batch_size or batch_size)
        self.device_resize = bool(device_resize)
        self.generator = None
        self._held_restored = []            # the shuffle buffer a restore decoded again, until the stream takes it over

    def _read_shard(self, path):
        return read_raw_shard(path)

    def _shard_stream(self, resume=None):
        rng = random.Random(self.seed + self.process_index)
        held, order, start, skip, seen = [], None, 0, 0, 0
        if resume is not None:
            # the generator state behind the last draw, the samples read from the current shard so far and the shuffle buffer
            # (decoded again by load_state_dict): everything the walk below depends on
            order, start, skip, seen = list(resume["order"]), int(resume["order_index"]), int(resume["consumed"]), int(resume["seen"])
            rng.setstate(_rng_from_json(resume["rng"]))
            held, self._held_restored = self._held_restored, []
        while True:
            if order is None:
                order, start, seen = list(self.paths), 0, 0
                rng.shuffle(order)
            for oi in range(start, len(order)):
                for n, sample in enumerate(self._read(order[oi])):
                    if n < skip:
                        continue
                    seen += 1
                    held.append(sample)
                    if len(held) > 2 * self.batch_size:
                        out = held.pop(rng.randrange(len(held)))
                        out["__pos__"] = dict(order=order, order_index=oi, consumed=n + 1, seen=seen, rng=rng.getstate(),
                                              held=[(h["__shard__"], h["__key__"]) for h in held])
                        yield out
                skip = 0
            if not seen:
                raise FileNotFoundError(f"BucketSamplerExtractFeatures: no decodable image + caption sample in {self.paths}")
            order = None

    @staticmethod
    def _stream_state(pos):
        return dict(order=list(pos["order"]), order_index=pos["order_index"], consumed=pos["consumed"], seen=pos["seen"],
                    rng=_rng_to_json(pos["rng"]), held=[list(r) for r in pos["held"]])

    def state_dict(self):
        """The base class's position plus the shuffle buffer (by reference, in ``stream``) and the state of the generator that
        draws an AutoencoderKL latent's noise (hex bytes; None before the first batch)."""
        state = super().state_dict()
        gen = self.generator
        state["generator"] = None if gen is None else bytes(gen.get_state().cpu().tolist()).hex()
        return state

    def _new_bucket(self):
        return deque(maxlen=4 * self.batch_size)

    def _extra_refs(self, state):
        return [tuple(r) for r in (state.get("stream") or {}).get("held", [])]

    def _load_extra(self, state, found):
        self._held_restored = []
        for path, key in self._extra_refs(state):
            if (path, key) not in found:
                raise ValueError(f"sampler state: sample {key!r} is not in {path}")
            sample = found[(path, key)]
            sample["__shard__"] = path
            self._held_restored.append(sample)
        if state.get("generator") is not None:
            self.generator = torch.Generator(device=self.accelerator.device)
            self.generator.set_state(torch.tensor(list(bytes.fromhex(state["generator"])), dtype=torch.uint8))

    def _make_item(self, elem):
        key, img = self._resized(elem)
        return (img, elem["caption"])

    def process_element(self, elem):
        key, img = self._resized(elem)
        self.buckets[key].append((img, elem["caption"]))
        return key

    def _resized(self, elem):
        from ..extract_latents import find_closest_ratio
        from ..image import pillow_resize, resize_uint8
        img = torch.from_numpy(elem["image"])
        h, w = img.shape[:2]
        key = float(find_closest_ratio(self.model.aspect_ratios, h / w))
        th, tw = self.sizes[key]
        if self.device_resize:
            img = resize_uint8(img, th, tw, device=self.accelerator.device)
        else:
            img = pillow_resize(img, th, tw)
        return key, img

    def make_batch(self, key, items):
        if self.generator is None:
            self.generator = torch.Generator(device=self.accelerator.device).manual_seed(self.seed + self.process_index)
        images = torch.stack([it[0] for it in items])
        captions = [it[1] for it in items]
        host = lambda e: tuple(t.cpu() for t in e) if isinstance(e, (tuple, list)) else e.cpu()      # noqa: E731
        latents, embeddings = [], []
        with torch.no_grad():
            for i in range(0, len(items), self.vae_max_batch_size):
                chunk = images[i:i + self.vae_max_batch_size]
                latents.append(self.model.extract_latents_uint8(chunk, generator=self.generator).to(torch.bfloat16).cpu())
            for i in range(0, len(items), self.text_encoder_max_batch_size):
                embeddings += [host(e) for e in self.model.extract_embeddings(captions[i:i + self.text_encoder_max_batch_size])]
        batch = Batch()
        batch.ratio = key
        batch.vae_features = torch.cat(latents)
        batch.embeddings = embeddings
        return batch
