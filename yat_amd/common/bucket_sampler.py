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
Out of scope: R2/HTTP download, on-the-fly VAE/text encoding, Dreambooth, dual-GPU and REPA branches.
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

from .shards import iter_legacy_cache, read_shard


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

    def _shard_stream(self):
        rng = random.Random(self.seed + self.process_index)
        while self.legacy_cache_dir:
            samples = list(iter_legacy_cache(self.legacy_cache_dir, self.process_index, self.num_processes))
            if not samples:
                raise FileNotFoundError(f"no cache/<idx>.npy sample for rank {self.process_index} in {self.legacy_cache_dir}")
            rng.shuffle(samples)
            yield from samples
        while True:
            order = list(self.paths)
            rng.shuffle(order)
            for p in order:
                samples = list(read_shard(p))
                rng.shuffle(samples)                               # webdataset .shuffle(1000) stand-in, seeded
                yield from samples

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
        stream = self._shard_stream()
        if self.decode_ahead > 0:
            stream = self._prefetched(stream)
        while True:
            # read ahead until this rank owns a full bucket (bounded), then ask everyone
            read = 0
            while not any(len(self.buckets[k]) >= self.batch_size for k in self.keys) and read < self.max_read_ahead:
                self.process_element(next(stream))
                read += 1
            key = self._full_everywhere()
            if key is None:
                # some rank lacks this bucket: everybody ingests a few more samples and retries
                for _ in range(self.batch_size):
                    self.process_element(next(stream))
                continue
            items = [self.buckets[key].popleft() for _ in range(self.batch_size)]
            batch = Batch()
            batch.ratio = key
            batch.vae_features = torch.stack([it[0] for it in items])       # :161-162
            batch.embeddings = [it[1] for it in items]
            yield batch
