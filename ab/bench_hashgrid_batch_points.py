"""B hash-grid fields trained at their own points per launch against a loop of B single fused fields (hashgrid.py,
HashGridFieldBatch.train_points; csrc/hashgrid_batch.hip, hash_batch_points_kernel); prints one JSON line:

    python ab/bench_hashgrid_batch_points.py [--out profiles/hashgrid_batch_points_bench.json] [--rows small|tiles|all]

Rows: 64 and 8 fields of 256 x 256 (L 8, F 2, T 2^12) with 2^14 uniformly random points each; the 64-field row again with ragged counts
from n / 4 to n; 64 tiles of 512 x 512 (T 2^15) with 2^16 points each; and 64 fields of 256 x 256 at ALL their sample centres in raster
order, where ``train_step`` on the same pixels runs too - the per-point cost over the crop route.  Per row, in ONE process and interleaved
call by call: the whole training step, optimiser included, of ``HashGridFieldBatch.train_points(order=precomputed)`` (the contender) and of a
loop of ``HashGridField.train_points(fused=True, order=precomputed)`` over the same fields and points (the route that exists without the
batch; that code is untouched).  The orders are computed before the timed region, as a fixed point set has them.  HIP events around each
call, 2 warm-up and 10 timed rounds: median, minimum, maximum.  ``ships``: the batch's median lies below the loop's minimum of the same run.
``expected`` was written before the first run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run, from the code and from profiles/hashgrid_batch_bench.json alone.  Nobody has measured this route; the crop
# batch's ratios (2.0 x at 8 fields, 2.3 x at 64, 1.2 x on the tiles) are the only guide and are not a target.  2^14 points are 256 wave
# items = 64 groups of four: a single field launches 64 workgroups, each staging the decoder and writing a record for ONE group - a quarter
# of the crop step's work (1024 patches) behind the same prologue, epilogue, launches and host path, so the loop should be bound by those
# even more than the crop loop is.
EXPECTED = {
    "B64_256_n16384": "the loop 64 x (0.1 - 0.16 ms) = 6 - 10 ms; the batch 512 workgroups of 8 groups each, two rounds on 256 CUs, plus reduce and optimiser: "
                      "1.5 - 3 ms; 2.5 - 5 x",
    "B8_256_n16384": "the batch 8 x 32 workgroups of 2 groups each, one round: 0.25 - 0.4 ms against 0.8 - 1.3 ms; 2 - 4 x",
    "B64_256_ragged": "counts from n / 4 to n average 5/8 n: the batch's kernel walks 5/8 of the items but its prologue, records, reduce and optimiser stay, "
                      "and so do the loop's launches: the ratio of the full row, or slightly below it",
    "B64_tiles_512_T15_n65536": "1024 wave items per field = 256 groups: a single field fills the chip; the batch wins the launches and host paths only: 1.1 - 1.5 x",
    "B64_256_raster": "65536 raster-ordered centres per field: the gather is as coherent as the crop's; train_points pays a load of the position and its "
                      "fixed-point conversion per point where train_step computes it from the patch index: the batch at points within 1.0 - 1.2 x of "
                      "the batch's train_step, and 2 - 2.5 x ahead of the loop, as the crop batch",
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "n": len(ts)}


def row(n_fields, size, log2_table, points, counts, dev, crop_route=False, warm=2, reps=10):
    """``points`` [B, n, 2] on the device; ``counts`` None or B ints.  ``crop_route``: the points are all sample centres in raster order, and
    ``HashGridFieldBatch.train_step`` on the whole field is timed too"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch, hash_batch_point_order
    kw = dict(levels=8, features=2, log2_table=log2_table, device=dev)
    batch = HashGridFieldBatch(n_fields, size, seed=0, **kw)
    singles = [HashGridField(size, seed=b, fused=True, **kw) for b in range(n_fields)]
    assert all(f.route == "fused" for f in singles)
    n = points.shape[1]
    target = torch.rand(n_fields, n, 3, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    order = None if crop_route else hash_batch_point_order(batch.geo, points, counts)          # raster order is coherent as it is
    cnt = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)
    nb = [n if counts is None else counts[b] for b in range(n_fields)]
    own = [(points[b, :nb[b]].contiguous(), target[b, :nb[b]].contiguous(), None if order is None else order[b, :nb[b]].contiguous()) for b in range(n_fields)]
    fns = {"loop_points": lambda: [f.train_points(p, t, fused=True, order=o) for f, (p, t, o) in zip(singles, own)],
           "batch_points": lambda: batch.train_points(points, target, counts=cnt, order=order)}
    if crop_route:
        crop = HashGridFieldBatch(n_fields, size, seed=0, **kw)
        origin = [[0] * len(size)]
        fns["batch_train_step"] = lambda: crop.train_step(origin, size, target)
    routes = list(fns)
    for _ in range(warm):
        for r in routes:
            fns[r]()
    torch.cuda.synchronize()
    ts = {r: [] for r in routes}
    for _ in range(reps):
        for r in routes:
            ts[r].append(timed(fns[r]))
    out = {r: stats(ts[r]) for r in routes}
    out["batch_points"]["ships"] = out["batch_points"]["median_ms"] < out["loop_points"]["min_ms"]
    out["batch_points"]["loop_over_batch_median"] = round(out["loop_points"]["median_ms"] / out["batch_points"]["median_ms"], 3)
    if crop_route:
        out["batch_points"]["points_over_train_step_median"] = round(out["batch_points"]["median_ms"] / out["batch_train_step"]["median_ms"], 3)
    out.update({"fields": n_fields, "shape": [*size], "levels": 8, "features": 2, "log2_table": log2_table, "points_per_field": n,
                "counts": "all" if counts is None else [min(counts), max(counts)], "order": "raster" if crop_route else "cell, precomputed",
                "groups_per_field": "automatic"})
    return out


def random_points(n_fields, size, n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(n_fields, n, 2, generator=g, device=dev) * torch.tensor(size, device=dev, dtype=torch.float32) - 0.5).contiguous()


def raster_centres(n_fields, size, dev):
    c = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device=dev) for s in size], indexing="ij"), dim=-1).reshape(1, -1, 2)
    return c.expand(n_fields, -1, -1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="all", choices=["small", "tiles", "all"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_batch_points", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
    if a.rows in ("small", "all"):
        n = 1 << 14
        for n_fields in (64, 8):
            res[f"B{n_fields}_256_n16384"] = row(n_fields, (256, 256), 12, random_points(n_fields, (256, 256), n, dev, 2), None, dev)
            torch.cuda.empty_cache()
        ragged = [n // 4 + (3 * n // 4) * b // 63 for b in range(64)]                  # n / 4 .. n
        res["B64_256_ragged"] = row(64, (256, 256), 12, random_points(64, (256, 256), n, dev, 2), ragged, dev)
        torch.cuda.empty_cache()
        res["B64_256_raster"] = row(64, (256, 256), 12, raster_centres(64, (256, 256), dev), None, dev, crop_route=True)
        torch.cuda.empty_cache()
    if a.rows in ("tiles", "all"):
        res["B64_tiles_512_T15_n65536"] = row(64, (512, 512), 15, random_points(64, (512, 512), 1 << 16, dev, 3), None, dev)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
