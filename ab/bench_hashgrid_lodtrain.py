"""The gradient with respect to the level of detail from the training step: the new call against the two calls it replaces and against the
step that returns the position gradient alone (hashgrid.py, csrc/hashgrid_lodtrain.hip); prints one JSON line:

    python ab/bench_hashgrid_lodtrain.py [--out profiles/hashgrid_lodtrain_bench.json]

4K (3840 x 2160; L 16, F 2, T 2^19; 8.29 M points) on ``fused=True`` fields - one plain, one with ``num_bits=4`` whose steps add the codec noise -
two point sets: the sample centres in raster order, and as many uniformly random points walked in cell order, the sort inside every timed call
(``order="cell"``).  Each at lambda = 0, lambda = 3 and one lambda per point in [0, 3].  ONE process, the routes of a row interleaved call by
call, HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum (the method of ab/bench_hashgrid_pointtrain.py).
Routes of a row:
- ``two_calls``: ``point_gradient_lod(points, lod, target=)`` followed by ``train_points(points, target, fused=True, lod=)`` - with noise on a
  timing comparison only: it cannot produce the right dlod;
- ``joint``: ``train_points_grad_lod(points, target, lod, dpoints, dlod, fused=True)`` - nic_hash_fused_forward_backward_points_grad_lod;
- ``sibling``: ``train_points(points, target, fused=True, lod=, dpoints=)`` - nic_hash_fused_forward_backward_points_grad, untouched.
``ships``: the joint call's median lies below the two calls' median by more than the two calls' own min - max spread.  The file is written with
its ``expected`` block before the first timed call and rewritten with the results."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run (DESIGN 4.7.23 has the reasoning)
EXPECTED = {
    "joint_over_sibling_noise_off": "1.00 - 1.02: one accumulator on a walk that is a smaller share of the step than of point_gradient (0.99 - 1.01 there)",
    "joint_over_sibling_noise_on_uniform_lambda": "1.01 - 1.03: one or two regenerated generator blocks per lane (about 170 vector instructions each) on top",
    "joint_over_sibling_noise_on_per_point": "1.03 - 1.08: the lanes of a wave sit on different ramps, so the wave makes a block for each of up to ~7 levels",
    "joint_under_two_calls": "by the cost of point_gradient_lod less the walk, 25 - 35 % of the two calls, on every row: all rows ship",
    "lambda3": "every route faster than lambda = 0 (the finest levels are gathered by no wave), the same ordering and ratios",
}
ROUTES = ("two_calls", "joint", "sibling")


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
    out["joint"]["over_sibling_median"] = round(out["joint"]["median_ms"] / out["sibling"]["median_ms"], 3)
    return out


def step_row(f, pts, target, order, lod):
    dp, dl = torch.empty_like(pts), torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)

    def two_calls():
        f.point_gradient_lod(pts, lod, target=target)
        f.train_points(pts, target, fused=True, order=order, lod=lod)

    return row({"two_calls": two_calls, "joint": lambda: f.train_points_grad_lod(pts, target, lod, dp, dl, fused=True, order=order),
                "sibling": lambda: f.train_points(pts, target, fused=True, order=order, lod=lod, dpoints=dp)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    dev = torch.device("cuda:0")
    size = (3840, 2160)
    res = {"bench": "hashgrid_lodtrain", "device": torch.cuda.get_device_name(0), "expected": EXPECTED, "shape": [*size], "levels": 16, "features": 2,
           "log2_table": 19}

    def write():
        line = json.dumps(res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return line

    write()                                                                      # the expectation is on disk before anything is timed
    fields = {"noise_off": HashGridField(size, device=dev, seed=0, fused=True), "noise_b4": HashGridField(size, device=dev, seed=0, fused=True, num_bits=4)}
    assert all(f.route == "fused" for f in fields.values())
    lattice = fields["noise_off"]._resample_points(size, (0, 0), size)
    n = lattice.shape[0]
    res["points"] = n
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand(n, 3, generator=g, device=dev)
    rnd = (torch.rand(n, 2, generator=g, device=dev) * torch.tensor([float(s) for s in size], device=dev) - 0.5).contiguous()
    per_point = (torch.rand(n, generator=g, device=dev) * 3.0).contiguous()
    for noise, f in fields.items():
        for name, pts, order in (("raster", lattice, None), ("random_cell", rnd, "cell")):
            for lod_name, lod in (("lod0", 0.0), ("lod3", 3.0), ("per_point", per_point)):
                res[f"{noise}_{name}_{lod_name}"] = step_row(f, pts, target, order, lod)
                write()
    res["ships"] = all(v["joint"]["ships"] for v in res.values() if isinstance(v, dict) and "joint" in v)
    print(write())


if __name__ == "__main__":
    main()
