"""Whole training steps of the hash-grid field at arbitrary points: the default layer-wise ``train_points`` against the cell-ordered and the
fused ones (hashgrid.py train_points(order=, fused=), csrc/hash_points_train.hip); prints one JSON line:

    python ab/bench_hashgrid_points_train.py [--out FILE] [--reps N]
    python ab/bench_hashgrid_points_train.py --default-only --root PARENT_CHECKOUT      # column (a) alone, from another checkout's package

The method of ab/bench_hashgrid_points.py: one process, HIP events around each call, the routes interleaved call by call (a, b, c, d, e, a, ..),
2 + 10 rounds, medians with min - max.  At 3840 x 2160, L 16, F 2, T 2^19, for three point sets: ``raster`` (the 8.29 M sample centres in
nic_encode order), ``random`` (8.29 M uniformly random points) and ``random_small`` (2^18 uniformly random points).  Columns, each a whole
training step with the optimiser:
  a  the default ``train_points`` (layer-wise, unordered: the parent's code, the baseline)
  b  layer-wise with ``order="cell"`` (keys + sort + ordered scatter, every step)
  c  ``fused=True``, unordered
  d  ``fused=True, order="cell"`` (keys + sort every step)
  e  ``fused=True`` with a precomputed order
plus ``sort`` (``hash_point_order`` alone) and, once, the fused crop ``train_step`` over the whole field (the yardstick).  ``expected`` holds what
DESIGN 4.7.5 wrote down before the first run.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = {
    "sort": "8.29 M int64 keys: 2 - 6 ms (a radix sort moves ~ 100 MB per pass over a few passes; the key kernel itself is 0.1 - 0.2 ms); "
            "2^18 keys: 0.1 - 0.4 ms, launch-bound",
    "a": "raster 35 - 50 ms (the 32 ms layer-wise crop step + the 5.5 ms raster penalty of the backward + a slower forward); random 150 - 175 ms "
         "(124 ms of it the backward)",
    "b": "random: the 124 ms backward falls to 12 - 25 ms (cell order gives runs at every level a raster wave has them, and 2D neighbours besides), "
         "so 45 - 70 ms with the sort; raster: a few ms SLOWER than (a) (the sort buys nothing the raster did not have, dx rows are read through "
         "an index)",
    "c": "random 100 - 135 ms: fusing removes the 1 GB row traffic, not the 8.3 M atomics per coarse level - still bound by them; raster 14 - 22 ms "
         "(the 12.2 ms crop step x the 1.65x raster scatter penalty on the scatter's share)",
    "d": "random 16 - 30 ms (the fused crop step's 12.2 ms, gathers from a Z-curve instead of 8 x 8 patches, + the sort): 5 - 10x faster than (a), "
         "the hard condition; raster 16 - 25 ms",
    "e": "(d) minus the sort: 13 - 24 ms",
    "random_small": "2^18 points: (a) 4 - 8 ms, dominated by the optimiser over the 16.8 M-entry table and the launches; the sort may not pay: (b), "
                    "(d) within +- 30 % of (a), (c)",
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, warm, reps):
    """{name: [median, min, max] ms}: every round runs each variant once, in order"""
    for _ in range(warm):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(timed(f))
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is timed")
    ap.add_argument("--default-only", action="store_true", help="column (a) alone: runs on a checkout without the new arguments")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    dev = torch.device("cuda:0")
    size = (3840, 2160)
    field = HashGridField(size, device=dev, seed=0, fused=True)
    assert field.route == "fused"
    geo = field.geo
    n = size[0] * size[1]
    g = torch.Generator(device=dev).manual_seed(1)
    S = torch.tensor([float(s) for s in size], device=dev)
    sets = {
        "raster": field._resample_points(size, (0, 0), size),
        "random": (torch.rand(n, 2, generator=g, device=dev) * S - 0.5).contiguous(),
        "random_small": (torch.rand(1 << 18, 2, generator=g, device=dev) * S - 0.5).contiguous(),
    }
    target = torch.rand(n, 3, generator=g, device=dev)
    res = {"bench": "hashgrid_points_train", "device": torch.cuda.get_device_name(0), "shape": list(size), "levels": 16, "features": 2, "log2_table": 19,
           "reps": a.reps, "package": os.path.abspath(a.root) == ROOT and "this checkout" or "another checkout", "expected": EXPECTED, "sets": {}}
    if not a.default_only:
        res["crop_train_step_ms"] = interleaved({"crop": lambda: field.train_step([[0, 0]], size, target)}, 2, a.reps)["crop"]
    for name, pts in sets.items():
        tgt = target[:pts.shape[0]]
        fns = {"a_default": lambda: field.train_points(pts, tgt)}
        if not a.default_only:
            pre = hashgrid.hash_point_order(geo, pts)
            fns.update({
                "b_layerwise_cell": lambda: field.train_points(pts, tgt, order="cell"),
                "c_fused": lambda: field.train_points(pts, tgt, fused=True),
                "d_fused_cell": lambda: field.train_points(pts, tgt, order="cell", fused=True),
                "e_fused_preordered": lambda: field.train_points(pts, tgt, order=pre, fused=True),
                "sort": lambda: hashgrid.hash_point_order(geo, pts),
            })
        t = interleaved(fns, 2, a.reps)
        entry = {"points": pts.shape[0], "step_ms": t}
        if not a.default_only:
            entry["over_a"] = {k: round(v[0] / t["a_default"][0], 3) for k, v in t.items() if k != "sort"}
            entry["d_range_below_a_range"] = t["d_fused_cell"][2] < t["a_default"][1]
        res["sets"][name] = entry
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
