"""Hash-grid field timings (hashgrid.py, csrc/hash_grid.hip); prints one JSON line:

    python ab/bench_hashgrid.py [--out FILE] [--ab LIB]      # everything (+ the A/B of the default library against LIB at 4K)
    python ab/bench_hashgrid.py --encode-only                 # the 4K encode kernels alone (what --ab runs in child processes)

- ``encode``: nic_hash_encode / nic_hash_encode_backward at 3840 x 2160, L 16, F 2, T 2^19 - HIP events around each launch, 5 warm-up
  launches, median of 30;
- ``step_4k`` / ``step_256cube``: the whole ``HashGridField.train_step`` (one crop = the whole field) - median of 10 after 3 warm-up steps;
- ``multilevel_4k``: the same 4K step through ``MultiLevelField``'s layer-wise route (3 pairs of 4 channels) - the decoder kernels are shared;
- ``ab``: the encode kernels of the default library against ``--ab LIB`` (``ab/mkv.sh norun hash_grid -DNIC_HASH_NO_RUNSUM``: no run sums,
  every lane issues its own atomics), fresh child processes interleaved A B A B A B, median of the three per side.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def encode_times(dev):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, hash_encode, hash_encode_backward, level_resolutions
    size = (3840, 2160)
    geo = HashGeometry(size, tuple(level_resolutions(16, 16, max(size))), 2, 19)
    table = (torch.rand(geo.table_shape(), device=dev) - 0.5) * 2e-4
    org = geo.upload_origins([[0, 0]], size, dev)
    dx = torch.randn(size[0] * size[1], geo.width, device=dev)
    grad = torch.zeros_like(table)
    fwd = event_ms(lambda: hash_encode(geo, table, org, size), 5, 30)
    bwd = event_ms(lambda: hash_encode_backward(geo, org, size, dx, grad), 5, 30)
    return {"shape": [*size], "levels": 16, "features": 2, "log2_table": 19, "resolutions": list(geo.resolutions),
            "fwd_ms": round(fwd, 4), "bwd_ms": round(bwd, 4), "fwd_plus_bwd_ms": round(fwd + bwd, 4)}


def step_ms(step, warm=3, reps=10):
    return event_ms(step, warm, reps)


def field_step(dev, size):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    field = HashGridField(size, device=dev, seed=0)
    n = 1
    for s in size:
        n *= s
    target = torch.rand(n, 3, device=dev)
    origin = [[0] * len(size)]
    ms = step_ms(lambda: field.train_step(origin, size, target))
    return {"shape": [*size], "levels": 16, "features": 2, "log2_table": 19, "step_ms": round(ms, 3), "mpix_per_s": round(n / ms / 1e3, 1)}


def multilevel_step(dev, size):
    from neural_image_compression_v2_amd.multilevel import MultiLevelField
    field = MultiLevelField(size, levels=3, channels=4, device=dev, seed=0, fused_step=False)
    n = size[0] * size[1]
    target = torch.rand(n, 3, device=dev)
    ms = step_ms(lambda: field.train_step([[0, 0]], size, target))
    return {"shape": [*size], "levels": 3, "channels": 4, "route": "layer-wise", "step_ms": round(ms, 3), "mpix_per_s": round(n / ms / 1e3, 1)}


def ab(lib_b):
    runs = {"default": [], "variant": []}
    for _ in range(3):
        for side, lib in (("default", None), ("variant", lib_b)):
            env = dict(os.environ)
            if lib:
                env["NIC_LIB_PATH"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--encode-only"], env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"A/B child ({side}) failed: {r.returncode}\n{r.stderr[-2000:]}")
            runs[side].append(json.loads(r.stdout.strip().splitlines()[-1])["encode"])
    med = lambda side, k: round(statistics.median(e[k] for e in runs[side]), 4)   # noqa: E731
    return {"variant": os.path.basename(lib_b), "what": "no run sums (-DNIC_HASH_NO_RUNSUM): every live lane issues its own atomics",
            "default_fwd_ms": med("default", "fwd_ms"), "default_bwd_ms": med("default", "bwd_ms"),
            "variant_fwd_ms": med("variant", "fwd_ms"), "variant_bwd_ms": med("variant", "bwd_ms"),
            "runs": {k: [[e["fwd_ms"], e["bwd_ms"]] for e in v] for k, v in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode-only", action="store_true")
    ap.add_argument("--ab", default=None, help="variant library for the A/B of the encode kernels")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid", "device": torch.cuda.get_device_name(0), "encode": encode_times(dev)}
    if not a.encode_only:
        res["step_4k"] = field_step(dev, (3840, 2160))
        torch.cuda.empty_cache()
        res["step_256cube"] = field_step(dev, (256, 256, 256))
        torch.cuda.empty_cache()
        res["multilevel_4k"] = multilevel_step(dev, (3840, 2160))
        if a.ab:
            torch.cuda.synchronize()
            res["ab"] = ab(a.ab)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
