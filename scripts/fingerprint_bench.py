#!/usr/bin/env python3
"""The device fingerprint (yat_fingerprint_u64) beside the bf16 AdamW kernel in ONE process over a SANA-1.6B-sized bf16 buffer,
each alone on the chip, the way scripts/adamw_master_bench.py compares the AdamW forms.

    python scripts/fingerprint_bench.py [--n ELEMENTS] [--rounds R] [--launches K] [--out FILE.txt]

Bytes: the fingerprint reads every byte once (2 B / element, nothing written but 8 bytes); yat_adamw_step moves 14 B / parameter.
Measured and recorded, no bar: the fingerprint does two 64-bit multiplies per 32-bit word, so it is not expected to reach the
streaming rate of a kernel that only adds.  The two alternate over the rounds; device events bracket K launches; the value is
checked against the numpy restatement on a 1 Mi-word slice and for additivity over the whole buffer."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from yat_amd import ops  # noqa: E402
from yat_amd.common.trainer_state import fingerprint_host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1604462752, help="bf16 elements (default: SANA-1.6B's flat buffer)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
n, dev = a.n // 8 * 8, "cuda"
gen = torch.Generator(device=dev).manual_seed(0)
p = (torch.randn(n, device=dev, generator=gen) * 0.02).to(torch.bfloat16)
g = (torch.randn(n, device=dev, generator=gen) * 0.01).to(torch.bfloat16)
m, v = torch.zeros_like(p), torch.zeros_like(p)
coef = torch.ones(1, device=dev)
out = torch.zeros(1, dtype=torch.int64, device=dev)
step = [0]


def fp():
    ops.fingerprint(p, out=out)


def adamw():
    step[0] += 1
    ops.adamw_step(p, g, m, v, coef, 1e-5, 0.9, 0.999, 1e-8, 0.0, step[0], zero_grad=False)


forms = {"fingerprint": (fp, 2), "adamw_step": (adamw, 14)}
for f, _ in forms.values():
    f(), f()
torch.cuda.synchronize()
times = {k: [] for k in forms}
for _ in range(a.rounds):
    for name, (f, _) in forms.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            f()
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / a.launches)
lines = [f"device: {torch.cuda.get_device_name(0)}; {n} bf16 elements ({2 * n / 1e9:.3f} GB); {a.rounds} rounds x {a.launches} launches, "
         "the two kernels alternating, device events"]
rate = {}
for name, (_, bpe) in forms.items():
    ms = sorted(times[name])
    med = ms[len(ms) // 2]
    rate[name] = bpe * n / med / 1e9
    lines.append(f"{name:12s} {bpe:2d} B/element: {med:8.3f} ms median (min {ms[0]:.3f}, max {ms[-1]:.3f})  {rate[name]:.3f} TB/s")
lines.append(f"fingerprint / adamw_step bytes per second: {rate['fingerprint'] / rate['adamw_step']:.3f} (recorded, no bar)")
# same value? a slice against the restatement, and the whole against the sum of three uneven slices
k = 1 << 21
sl = p[8:8 + k]
assert ops.fingerprint(sl, word_offset=5) == fingerprint_host(sl.cpu(), word_offset=5)
whole = ops.fingerprint(p)
cuts = [0, 8 * 12345, n // 2 + 8, n]
parts = sum(ops.fingerprint(p[lo:hi], word_offset=lo // 2) for lo, hi in zip(cuts[:-1], cuts[1:])) & ((1 << 64) - 1)
assert parts == whole, (parts, whole)
lines.append(f"value {whole:016x}: a 1 Mi-word slice equals the numpy restatement; the whole equals the sum of 3 uneven slices")
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
