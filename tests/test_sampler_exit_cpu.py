"""The bucket sampler's decode thread at interpreter exit.  A daemon thread that is inside a torch call when the interpreter
finalises is ended from within C++ frames, and the process aborts ("terminate called without an active exception", exit
status -6) after all its work is done -- so the sampler stops and joins its producer when the consumer is closed, in
``close()`` and, at the latest, in an exit hook."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the queue never fills (decode_ahead far above what is consumed), so the producer is decoding shards when the script ends
SCRIPT = """
import pathlib, sys, types
sys.path.insert(0, {root!r})
from tests.test_host_logic import _make_shards
from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN
from yat_amd.common.bucket_sampler import BucketSampler
from yat_amd.common.trainer import HipAccelerator
paths = _make_shards(pathlib.Path({tmp!r}), 2, 24)
model = types.SimpleNamespace(aspect_ratios=ASPECT_RATIO_1024_BIN)
sampler = BucketSampler([], HipAccelerator(1, device="cpu"), batch_size=3, model=model, seed=5, local_paths=paths,
                        decode_ahead=1 << 20)
it = iter(sampler)
batch = next(it)
{end}
print("done", batch.ratio)
"""


def _run(tmp_path, end):
    env = dict(os.environ, YAT_TENSORBOARD="0", PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-c", SCRIPT.format(root=ROOT, tmp=str(tmp_path), end=end)], env=env,
                          capture_output=True, text=True, timeout=120)


def test_exit_with_the_producer_still_decoding(tmp_path):
    r = _run(tmp_path, "")                              # the iterator is never closed: the exit hook joins the thread
    assert r.returncode == 0 and "done" in r.stdout, (r.returncode, r.stderr[-1000:])


def test_close_joins_the_producer(tmp_path):
    end = ("t = sampler._producer[0]\nsampler.close()\nassert not t.is_alive() and sampler._producer is None\n"
           "sampler.close()")
    r = _run(tmp_path, end)
    assert r.returncode == 0 and "done" in r.stdout, (r.returncode, r.stderr[-1000:])
