#!/usr/bin/env python3
"""Side measurement for the ingest resize: one random 12-megapixel 3:4 photograph (4000 x 3000) to its bucket of the 1024
aspect table, by Pillow on one core, by the device path of ``yat_amd.image.resize_uint8`` including the upload of the decoded
image from pageable host memory, and by the kernel alone (device events, source already resident) with its effective
bandwidth against the bytes it must move (the source once + the result once).

    python scripts/bench_image_resize.py [--out profiles/image_resize_a_bench.json] [--reps 10]

The sampler's ``device_resize`` default follows from the first two numbers.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import image as yimg                                   # noqa: E402
from yat_amd.common.aspect_ratios import table_for_resolution       # noqa: E402
from yat_amd.extract_latents import bucket_for                      # noqa: E402

HBM_PEAK_GBS = 8000.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/image_resize_a_bench.json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=4000)
    ap.add_argument("--width", type=int, default=3000)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_resize needs a GPU")
    dev = torch.device("cuda")
    H, W = a.height, a.width
    key, th, tw = bucket_for(table_for_resolution(1024), H, W)
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8))

    def timed(fn, reps):
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    want = yimg.pillow_resize(img, th, tw)                            # (also the warm-up of Pillow)
    pillow = timed(lambda: yimg.pillow_resize(img, th, tw), a.reps)

    def device_path():
        yimg.resize_uint8(img, th, tw, device=dev)
        torch.cuda.synchronize()
    for _ in range(3):
        device_path()                                                 # code object, tables, allocator
    path = timed(device_path, a.reps)

    src, out = img.to(dev), torch.empty(th, tw, 3, dtype=torch.uint8, device=dev)
    for _ in range(3):
        yimg.resize_uint8_device(src, th, tw, out=out)
    inner = 20
    kernel = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            yimg.resize_uint8_device(src, th, tw, out=out)
        e1.record()
        torch.cuda.synchronize()
        kernel.append(e0.elapsed_time(e1) / inner)
    exact = bool(torch.equal(out.cpu(), want))
    moved = H * W * 3 + th * tw * 3
    k_ms = statistics.median(kernel)
    res = {
        "metric": "image_resize_ms", "source_hw": [H, W], "bucket": key, "target_hw": [th, tw], "plan": yimg.resize_plan(H, W, th, tw),
        "equals_pillow": exact,
        "pillow_one_core_ms": round(statistics.median(pillow), 3), "pillow_all_ms": [round(v, 3) for v in pillow],
        "device_path_with_upload_ms": round(statistics.median(path), 3), "device_path_all_ms": [round(v, 3) for v in path],
        "kernel_ms": round(k_ms, 4), "kernel_all_ms": [round(v, 4) for v in kernel],
        "bytes_moved": moved, "kernel_effective_gbs": round(moved / (k_ms * 1e-3) / 1e9, 1),
        "kernel_frac_hbm_peak": round(moved / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "upload": "pageable host memory, torch .to(device)", "pillow_version": __import__("PIL").__version__,
        "device": torch.cuda.get_device_name(0),
    }
    res["device_resize_faster_than_pillow"] = res["device_path_with_upload_ms"] < res["pillow_one_core_ms"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not exact:
        raise SystemExit("the device result is not Pillow's")


if __name__ == "__main__":
    main()
