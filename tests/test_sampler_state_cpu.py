"""``BucketSampler.state_dict()`` / ``load_state_dict()`` (yat_amd/common/bucket_sampler.py) without a GPU.

Contract: a sampler restored from the state taken after it yielded batch k yields exactly the batches k + 1, k + 2, ... of the
sampler that was never stopped -- ratio key, tensors and embedding lists equal --, at any ``decode_ahead``; a restore reads the
shards that hold pending bucket entries and the one the stream stood in, and nothing else."""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from yat_amd.common import bucket_sampler as bs
from yat_amd.common.bucket_sampler import BucketSampler, BucketSamplerExtractFeatures
from yat_amd.common.shards import write_shard
from yat_amd.common.trainer import HipAccelerator

BATCH, FOLLOW, SHARDS, PER = 4, 12, 3, 10
RATIOS = {"1.0": [8, 8], "0.5": [4, 8], "2.0": [8, 4]}


class Table:
    aspect_ratios = RATIOS


def make_shards(tmp, seed=0, shards=SHARDS, per=PER):
    """``shards`` x ``per`` samples over three ratios; "2.0" comes three times per pass over all shards -- fewer than one batch
    -- so its leftovers wait in their bucket across an epoch boundary."""
    g = torch.Generator().manual_seed(seed)
    paths, rare = [], {(0, 3), (1, 7), (2, 1)}
    for s in range(shards):
        samples = []
        for i in range(per):
            r = "2.0" if (s, i) in rare else ("1.0" if (i + s) % 2 else "0.5")
            h, w = RATIOS[r]
            samples.append(dict(__key__=f"{seed}{s:02d}{i:04d}", ratio=r, latent=torch.randn(2, h, w, generator=g).to(torch.bfloat16),
                                emb=torch.randn(1 + (i % 5), 6, generator=g).to(torch.bfloat16)))
        p = str(tmp / f"shard-{s:06d}.tar")
        write_shard(p, samples)
        paths.append(p)
    return paths


def sampler(paths, decode_ahead, seed=3, acc=None):
    return BucketSampler([], acc or HipAccelerator(1, device="cpu"), batch_size=BATCH, model=Table(), seed=seed, local_paths=paths,
                         decode_ahead=decode_ahead)


def same(a, b):
    return (a.ratio == b.ratio and torch.equal(a.vae_features, b.vae_features) and len(a.embeddings) == len(b.embeddings)
            and all(torch.equal(x, y) for x, y in zip(a.embeddings, b.embeddings)))


def recorded_run(paths, n, decode_ahead):
    """n batches of an uninterrupted sampler and the (JSON round-tripped) state after each"""
    s = sampler(paths, decode_ahead)
    it = iter(s)
    batches, states = [], [json.loads(json.dumps(s.state_dict()))]          # states[k]: after k batches (0: before any)
    for _ in range(n):
        batches.append(next(it))
        states.append(json.loads(json.dumps(s.state_dict())))
    s.close()
    return batches, states


def where(state):
    st = state["stream"]
    if st is None:
        return "start"
    if st["consumed"] < PER:
        return "mid-shard"
    return "epoch boundary" if st["order_index"] == SHARDS - 1 else "shard boundary"


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    paths = make_shards(tmp_path_factory.mktemp("shards"))
    batches, states = recorded_run(paths, 60 + FOLLOW, decode_ahead=0)
    return paths, batches, states


def test_state_is_the_consumers_position_at_any_decode_ahead(reference):
    paths, batches, states = reference
    ahead, states_ahead = recorded_run(paths, 20, decode_ahead=7)          # the producer thread reads ahead of the consumer
    assert all(same(a, b) for a, b in zip(ahead, batches))
    assert states_ahead == states[:21]


@pytest.mark.parametrize("decode_ahead", [0, 5])
def test_restored_sampler_continues_the_uninterrupted_sequence(reference, decode_ahead):
    paths, batches, states = reference
    seen = set()
    picks = {}
    for k in range(0, 61):
        picks.setdefault(where(states[k]), []).append(k)
    assert set(picks) == {"start", "mid-shard", "shard boundary", "epoch boundary"}, {w: len(v) for w, v in picks.items()}
    # the rare ratio's leftovers really wait across an epoch boundary in at least one of the states that are restored
    chosen = [ks[i] for w, ks in picks.items() for i in sorted({0, len(ks) // 2, len(ks) - 1})]
    crossing = [k for k in picks["epoch boundary"] if dict((float(r), v) for r, v in states[k]["buckets"])[2.0]]
    assert crossing, "no state with pending rare-ratio samples on an epoch boundary"
    for k in sorted(set(chosen + crossing[:1])):
        s = sampler(paths, decode_ahead)
        s.load_state_dict(states[k])
        assert json.loads(json.dumps(s.state_dict())) == states[k]           # before anything is consumed: the state itself
        it = iter(s)
        for j in range(FOLLOW):
            assert same(next(it), batches[k + j]), (k, where(states[k]), j)
        assert json.loads(json.dumps(s.state_dict())) == states[k + FOLLOW]
        s.close()
        seen.add(where(states[k]))
    assert seen == {"start", "mid-shard", "shard boundary", "epoch boundary"}


def test_restore_reads_only_the_current_and_the_pending_shards(reference, monkeypatch):
    paths, batches, states = reference
    reads = []
    real = bs.read_shard
    monkeypatch.setattr(bs, "read_shard", lambda p: (reads.append(p), real(p))[1])
    for k in (5, 17, 33, 58):
        st = states[k]
        current = st["stream"]["order"][st["stream"]["order_index"]]
        pending = {p for _, refs in st["buckets"] for p, _ in refs}
        s = sampler(paths, 0)
        reads.clear()
        s.load_state_dict(st)
        assert sorted(reads) == sorted(pending)                               # every pending shard once, nothing else
        stream = s._shard_stream(s._resume)
        first = next(stream)
        after = st["stream"]["order"][st["stream"]["order_index"] + 1] if st["stream"]["order_index"] + 1 < SHARDS else None
        allowed = pending | {current} | ({after} if st["stream"]["consumed"] == PER and after else set())
        if st["stream"]["consumed"] == PER and after is None:
            allowed = allowed | set(paths)                                    # (an epoch boundary: the next epoch's first shard)
        assert set(reads) <= allowed and len(reads) <= len(pending | {current}) + 1, (k, reads)
        if st["stream"]["consumed"] < PER:
            assert len([p for p in reads if p == current]) == 1               # the current shard is not read twice
        assert "__shard__" in first


def test_refusals(reference, tmp_path):
    paths, _, states = reference
    st = states[9]
    for field, value in (("seed", 4), ("batch_size", 3), ("kind", "BucketSamplerExtractFeatures"), ("num_processes", 2)):
        with pytest.raises(ValueError, match=field):
            sampler(paths, 0).load_state_dict({**st, field: value})
    with pytest.raises(ValueError, match="not in this sampler's list"):
        sampler(paths[:2], 0).load_state_dict(st)
    s = sampler(paths, 0)
    next(iter(s))
    with pytest.raises(RuntimeError, match="already being read"):
        s.load_state_dict(st)
    os.makedirs(tmp_path / "cache")
    legacy = BucketSampler([], HipAccelerator(1, device="cpu"), batch_size=BATCH, model=Table(), legacy_cache_dir=str(tmp_path / "cache"))
    with pytest.raises(NotImplementedError, match="legacy"):
        legacy.state_dict()
    with pytest.raises(NotImplementedError, match="legacy"):
        legacy.load_state_dict(st)


# ---------------------------------------------------------------------------------------------- the raw-shard sampler
def test_raw_shard_sampler_with_the_host_resize(tmp_path, monkeypatch):
    """``BucketSamplerExtractFeatures`` driven as tests/test_extract_sampler_cpu.py drives it: the stream position, the shuffle
    buffer of 2 x batch_size samples (by reference, decoded and resized again), the bounded buckets and the generator's state."""
    from tests.test_extract_sampler_cpu import StubModel, write_raw_shard
    paths = []
    for s in range(3):
        write_raw_shard(str(tmp_path / f"{s:05d}.tar"), 9, seed=s)
        paths.append(str(tmp_path / f"{s:05d}.tar"))

    def make(decode_ahead):
        return BucketSamplerExtractFeatures([], HipAccelerator(1, device="cpu"), model=StubModel(), local_paths=paths, batch_size=3,
                                            seed=5, vae_max_batch_size=2, text_encoder_max_batch_size=1, device_resize=False,
                                            decode_ahead=decode_ahead)
    ref = make(0)
    it = iter(ref)
    batches, states = [], [json.loads(json.dumps(ref.state_dict()))]
    for _ in range(14 + 6):
        batches.append(next(it))
        states.append(json.loads(json.dumps(ref.state_dict())))
    assert states[0]["generator"] is None and states[1]["generator"] is not None
    assert all(len(s["stream"]["held"]) == 6 for s in states[1:])
    assert {s["stream"]["order_index"] for s in states[1:]} == {0, 1, 2}          # positions in every shard of the epoch
    reads = []
    real = bs.read_raw_shard
    monkeypatch.setattr(bs, "read_raw_shard", lambda p: (reads.append(p), real(p))[1])
    for k, ahead in ((0, 0), (1, 0), (4, 4), (9, 0), (14, 3)):
        s = make(ahead)
        reads.clear()
        s.load_state_dict(states[k])
        st = states[k]["stream"]
        if st is not None:
            pending = {p for _, refs in states[k]["buckets"] for p, _ in refs} | {p for p, _ in st["held"]}
            assert sorted(reads) == sorted(pending)
        it2 = iter(s)
        for j in range(6):
            b = next(it2)
            assert b.ratio == batches[k + j].ratio and torch.equal(b.vae_features, batches[k + j].vae_features), (k, j)
            assert all(torch.equal(x, y) for x, y in zip(b.embeddings, batches[k + j].embeddings))
        assert json.loads(json.dumps(s.state_dict())) == states[k + 6]
        s.close()


def test_a_bounded_bucket_reproduces_its_drops(tmp_path):
    """A bucket of ``maxlen`` 4 x batch_size that nobody empties drops its oldest: the saved references are the survivors."""
    from tests.test_extract_sampler_cpu import StubModel, write_raw_shard
    write_raw_shard(str(tmp_path / "00000.tar"), 24)
    path = str(tmp_path / "00000.tar")

    def make():
        return BucketSamplerExtractFeatures([], HipAccelerator(1, device="cpu"), model=StubModel(), local_paths=[path], batch_size=1,
                                            seed=1, device_resize=False, decode_ahead=0)
    a = make()
    stream = a._shard_stream()
    for _ in range(20):
        a._ingest(next(stream))                                   # 20 samples over 3 ratios, buckets of 4: the oldest are gone
    assert all(len(b) <= 4 for b in a.buckets.values()) and sum(len(b) for b in a.buckets.values()) < 20
    state = json.loads(json.dumps(a.state_dict()))
    b = make()
    b.load_state_dict(state)
    for k in a.keys:
        assert len(a.buckets[k]) == len(b.buckets[k]) and b.buckets[k].maxlen == 4
        for (im_a, c_a), (im_b, c_b) in zip(a.buckets[k], b.buckets[k]):
            assert c_a == c_b and torch.equal(im_a, im_b)
    rest_a, rest_b = [next(stream)["__key__"] for _ in range(6)], []
    sb = b._shard_stream(b._resume)
    rest_b = [next(sb)["__key__"] for _ in range(6)]
    assert rest_a == rest_b


# ---------------------------------------------------------------------------------------------- world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _world2_worker(rank, world, port, tmp):
    import pathlib
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    paths = make_shards(pathlib.Path(tmp) / f"r{rank}", seed=rank)          # every rank its own shards: the consensus decides
    acc = HipAccelerator(1, device="cpu")
    assert acc.num_processes == 2 and acc.process_index == rank
    ref = sampler(paths, 0, acc=acc)
    it = iter(ref)
    batches, states = [], []
    for _ in range(9 + FOLLOW):
        batches.append(next(it))
        states.append(json.loads(json.dumps(ref.state_dict())))
    for k in (2, 9):                                                          # both ranks restore the state after batch k
        s = sampler(paths, 0 if k == 2 else 4, acc=acc)
        s.load_state_dict(states[k - 1])
        it2 = iter(s)
        for j in range(FOLLOW):
            b = next(it2)
            assert same(b, batches[k + j]), (rank, k, j)
            both = [torch.zeros(1), torch.zeros(1)]
            dist.all_gather(both, torch.tensor([b.ratio]))
            assert both[0].item() == both[1].item()
        s.close()
    with pytest.raises(ValueError, match="process_index"):
        sampler(paths, 0, acc=acc).load_state_dict({**states[3], "process_index": 1 - rank})
    dist.barrier()
    dist.destroy_process_group()


def test_world2_gloo_both_ranks_restored(tmp_path):
    for r in range(2):
        (tmp_path / f"r{r}").mkdir()
    mp.spawn(_world2_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
