"""Training the field and the point positions in one step: the joint call against the two calls it replaces and against the step alone
(hashgrid.py, csrc/hashgrid_points_joint.hip); prints one JSON line:

    python ab/bench_hashgrid_pointtrain.py [--out profiles/hashgrid_pointtrain_bench.json]

4K (3840 x 2160; L 16, F 2, T 2^19; 8.29 M points) on a ``fused=True`` field, two point sets - the sample centres in raster order, and as many
uniformly random points walked in cell order, the sort inside every timed call (``order="cell"``, as DESIGN 4.7.5 reports it) - each plain and
at ``lod=3.0``.  ONE process, the routes of a row interleaved call by call, HIP events around each call, 2 warm-up and 10 timed rounds: median,
minimum, maximum.  Routes of a row:
- ``two_calls``: ``point_gradient(points, target=)`` followed by ``train_points(points, target, fused=True)`` - the loop as it had to be written;
- ``joint``: ``train_points(points, target, fused=True, dpoints=)`` - nic_hash_fused_forward_backward_points_grad;
- ``train``: ``train_points(points, target, fused=True)`` alone - this build's untouched kernel, the yardstick.
``ships``: the joint call's median lies below the two calls' median by more than the two calls' own min - max spread, on every row.  The file is
written with its ``expected`` block before the first timed call and rewritten with the results."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run.  The joint kernel is the training kernel plus the second walk over the levels that point_gradient adds to a
# query (README: query 2.84 ms, point_gradient 5.14 ms at 4K raster, of which the decoder's backward to the input is part - the training
# kernel has that backward already, so the walk alone is the upper part of that difference); the two calls gather every level twice, run the
# decoder forward twice and the backward to the row twice.
EXPECTED = {
    "raster_ms": {"train": "15.7 (README)", "two_calls": "15.7 + 5.14 = 20.8", "joint": "train + (point_gradient - query) = 15.7 + 2.3 = 18.0 at most"},
    "random_cell_ms": "the sort is in all three routes; joint - train as in raster order or a little more (the second gather of a level hits L2)",
    "lod3": "every route faster than plain (the finest levels are gathered by no wave), the same ordering",
    "joint_over_train": "about 1.15",
}
ROUTES = ("two_calls", "joint", "train")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "n": len(ts)}


def row(fns, warm=2, reps=10):
    """fns: {route: callable}, interleaved call by call"""
    for _ in range(warm):
        for r in ROUTES:
            fns[r]()
    torch.cuda.synchronize()
    ts = {r: [] for r in ROUTES}
    for _ in range(reps):
        for r in ROUTES:
            ts[r].append(timed(fns[r]))
    out = {r: stats(ts[r]) for r in ROUTES}
    spread = out["two_calls"]["max_ms"] - out["two_calls"]["min_ms"]
    out["joint"]["saves_ms"] = round(out["two_calls"]["median_ms"] - out["joint"]["median_ms"], 3)
    out["joint"]["two_calls_spread_ms"] = round(spread, 3)
    out["joint"]["ships"] = out["two_calls"]["median_ms"] - out["joint"]["median_ms"] > spread
    out["joint"]["over_train_median"] = round(out["joint"]["median_ms"] / out["train"]["median_ms"], 3)
    return out


def step_row(f, pts, target, order, lod):
    dp = torch.empty_like(pts)

    def two_calls():
        f.point_gradient(pts, target=target, lod=lod)
        f.train_points(pts, target, fused=True, order=order, lod=lod)

    return row({"two_calls": two_calls, "joint": lambda: f.train_points(pts, target, fused=True, order=order, lod=lod, dpoints=dp),
                "train": lambda: f.train_points(pts, target, fused=True, order=order, lod=lod)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    dev = torch.device("cuda:0")
    size = (3840, 2160)
    res = {"bench": "hashgrid_pointtrain", "device": torch.cuda.get_device_name(0), "expected": EXPECTED, "shape": [*size], "levels": 16, "features": 2,
           "log2_table": 19}

    def write():
        line = json.dumps(res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return line

    write()                                                                      # the expectation is on disk before anything is timed
    f = HashGridField(size, device=dev, seed=0, fused=True)
    assert f.route == "fused"
    lattice = f._resample_points(size, (0, 0), size)
    n = lattice.shape[0]
    res["points"] = n
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand(n, 3, generator=g, device=dev)
    rnd = (torch.rand(n, 2, generator=g, device=dev) * torch.tensor([float(s) for s in size], device=dev) - 0.5).contiguous()
    for name, pts, order in (("raster", lattice, None), ("random_cell", rnd, "cell")):
        for lod_name, lod in (("plain", None), ("lod3", 3.0)):
            res[f"{name}_{lod_name}"] = step_row(f, pts, target, order, lod)
    res["ships"] = all(v["joint"]["ships"] for k, v in res.items() if isinstance(v, dict) and "joint" in v)
    print(write())


if __name__ == "__main__":
    main()
