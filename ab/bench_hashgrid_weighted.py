"""Per-point loss weights in the training step at points: the weighted call against the sibling step of the same arguments, and a 50 % mask in
one weighted call against compaction on the host (hashgrid.py, csrc/hashgrid_weighted.hip); prints one JSON line:

    python ab/bench_hashgrid_weighted.py [--out profiles/hashgrid_weighted_bench.json]

4K (3840 x 2160; L 16, F 2, T 2^19; 8.29 M points) on ``fused=True`` fields - one plain, one with ``num_bits=4`` whose steps add the codec noise -
two point sets: the sample centres in raster order, and as many uniformly random points walked in cell order, the sort inside every timed call
(``order="cell"``).  Each without a level of detail, at lambda = 3 and with one lambda per point in [0, 3].  ONE process, the routes of a row
interleaved call by call, HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum (the method of
ab/bench_hashgrid_lodtrain.py).  Routes of a row:
- ``sibling``: ``train_points(points, target, fused=True, lod=)`` - nic_hash_fused_forward_backward_points / _points_lod, untouched;
- ``weighted``: ``train_points_weighted(points, target, weight, lod=, fused=True)`` with uniform(0, 2) weights -
  nic_hash_fused_forward_backward_points_weighted;
- ``masked``: the weighted call with a random 0 / 1 mask that keeps half of the points;
- ``compacted``: ``keep = mask > 0; train_points(points[keep], target[keep], ...)`` - the boolean index inside the timed call, the sibling on the
  kept half (informational: it says when a caller should still compact).
``inside_spread``: the weighted median lies no further above the sibling's than the sibling's own min - max spread.  The file is written with
its ``expected`` block before the first timed call and rewritten with the results."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run (DESIGN 4.7.26 has the reasoning)
EXPECTED = {
    "weighted_over_sibling": "1.00 within the sibling's own min - max spread on every row: one 4-byte load per point (33 MB against a 17 - 19 ms step), "
                             "two multiplies per sample; the rows without a level of detail run the level-of-detail body at lambda = 0, one weight per level more",
    "masked_over_weighted": "1.00: a point of weight 0 costs its gathers, its decoder passes and its scatter of zeros; no wave is skipped",
    "compacted_over_masked": "0.5 - 0.7 in raster order (half the points, plus two boolean-index copies of 100 + 66 MB and the mask reduction); "
                             "closer to 1 at random points in cell order, where the sort of the kept half is a larger share",
}
ROUTES = ("sibling", "weighted", "masked", "compacted")


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
    spread = out["sibling"]["max_ms"] - out["sibling"]["min_ms"]
    out["weighted"]["over_sibling_median"] = round(out["weighted"]["median_ms"] / out["sibling"]["median_ms"], 3)
    out["weighted"]["sibling_spread_ms"] = round(spread, 3)
    out["weighted"]["inside_spread"] = out["weighted"]["median_ms"] - out["sibling"]["median_ms"] <= spread
    out["masked"]["over_weighted_median"] = round(out["masked"]["median_ms"] / out["weighted"]["median_ms"], 3)
    out["compacted"]["over_masked_median"] = round(out["compacted"]["median_ms"] / out["masked"]["median_ms"], 3)
    return out


def step_row(f, pts, target, order, lod, weight, mask):
    per_point = isinstance(lod, torch.Tensor)

    def compacted():
        keep = mask > 0
        f.train_points(pts[keep], target[keep], fused=True, order=order, lod=lod[keep] if per_point else lod)

    return row({"sibling": lambda: f.train_points(pts, target, fused=True, order=order, lod=lod),
                "weighted": lambda: f.train_points_weighted(pts, target, weight, lod=lod, fused=True, order=order),
                "masked": lambda: f.train_points_weighted(pts, target, mask, lod=lod, fused=True, order=order),
                "compacted": compacted})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    dev = torch.device("cuda:0")
    size = (3840, 2160)
    res = {"bench": "hashgrid_weighted", "device": torch.cuda.get_device_name(0), "expected": EXPECTED, "shape": [*size], "levels": 16, "features": 2,
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
    weight = (torch.rand(n, generator=g, device=dev) * 2.0).contiguous()
    mask = (torch.rand(n, generator=g, device=dev) < 0.5).float().contiguous()
    res["mask_kept"] = int(mask.sum())
    for noise, f in fields.items():
        for name, pts, order in (("raster", lattice, None), ("random_cell", rnd, "cell")):
            for lod_name, lod in (("no_lod", None), ("lod3", 3.0), ("per_point", per_point)):
                res[f"{noise}_{name}_{lod_name}"] = step_row(f, pts, target, order, lod, weight, mask)
                write()
    res["inside_spread"] = all(v["weighted"]["inside_spread"] for v in res.values() if isinstance(v, dict) and "weighted" in v)
    print(write())


if __name__ == "__main__":
    main()
