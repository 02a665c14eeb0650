"""What the VAE side benchmarks share (bench_dcae.py, bench_dcae_encoder.py, bench_vae_kl.py): random weights of a given
key -> shape map, a median-of-HIP-event-pairs timer and the per-launch instrumentation of ``yat_amd.ops`` functions."""
import torch

from yat_amd import ops

PEAK = 2.5e15


def random_weights(expected, seed=0):
    """``expected``: a module's ``expected_keys(cfg)``.  Norm weights one, other vectors small, matrices 1 / sqrt(fan-in)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in expected.items():
        if len(shape) == 1:
            sd[k] = torch.ones(shape) if "norm" in k else 0.05 * torch.randn(shape, generator=g)
        else:
            fan = 1
            for s in shape[1:]:
                fan *= s
            sd[k] = torch.randn(shape, generator=g) / fan ** 0.5
    return sd


def timed(fn, repeats):
    """(median ms, every ms, the last result) of ``fn()`` between two HIP events, synchronised after each repeat."""
    times, out = [], None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2], times, out


def instrumented(meters, run):
    """``run()`` with an event pair around every launch of the ``ops`` functions named in ``meters`` ({name: f(*args, **kw)
    -> (key, flops or bytes)}).  -> {name: [(key, amount, ms)]} in launch order."""
    rec = {name: [] for name in meters}
    saved = {name: getattr(ops, name) for name in meters}

    def wrap(name):
        def call(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = saved[name](*a, **kw)
            e1.record()
            rec[name].append(meters[name](*a, **kw) + (e0, e1))
            return out
        return call
    for name in meters:
        setattr(ops, name, wrap(name))
    try:
        run()
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    return {name: [(key, amount, e0.elapsed_time(e1)) for key, amount, e0, e1 in r] for name, r in rec.items()}


def conv_rows(records, fields):
    """Conv launches [(key, flops, ms)] aggregated per key, slowest first: (total ms, rows naming the key by ``fields``)."""
    shapes = {}
    for key, f, ms in records:
        s = shapes.setdefault(key, [0, 0.0, 0.0])
        s[0] += 1
        s[1] += ms
        s[2] += f
    rows = [{**dict(zip(fields, k)), "calls": v[0], "ms": round(v[1], 3), "tflops": round(v[2] / v[1] / 1e9, 1),
             "frac_peak": round(v[2] / v[1] / 1e-3 / PEAK, 3)} for k, v in sorted(shapes.items(), key=lambda kv: -kv[1][1])]
    return sum(v[1] for v in shapes.values()), rows
