"""B hash-grid fields per launch with gradients to the point positions against a loop of B single fused fields (hashgrid.py,
HashGridFieldBatch.train_points_grad / point_gradient; csrc/hashgrid_batch.hip, hash_batch_points_joint_kernel; csrc/hashgrid_batch_grad.hip,
hash_batch_points_grad_kernel); prints one JSON line:

    python ab/bench_hashgrid_batch_pointgrad.py [--out profiles/hashgrid_batch_pointgrad_bench.json] [--rows small|tiles|all]

Rows, those of DESIGN 4.7.18 and 4.7.20: 64 and 8 fields of 256 x 256 (L 8, F 2, T 2^12) with 2^14 uniformly random points each, and 64 tiles
of 512 x 512 (T 2^15) with 2^16 points each; every row plain and with a level of detail per point, the points laid out in cell order once,
before the timed region, as a fixed point set has them.  Per row, in ONE process and interleaved call by call:

  (a) ``loop_joint``: a loop of single fields doing ``train_points(fused=True, dpoints=)`` - the route that exists without this code -, and
      ``loop_grad``: their ``point_gradient(target=)``;
  (b) ``batch_joint``: ``HashGridFieldBatch.train_points_grad``, and ``batch_grad``: ``HashGridFieldBatch.point_gradient(target=)``;
  (c) ``batch_train``: the batch's ``train_points`` / ``train_points_lod`` alone, and ``batch_query``: its ``query`` / ``query_lod``.

Training calls are whole steps, optimiser included.  HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum.
``ships``: (b)'s median lies below (a)'s median by more than (a)'s own min - max spread.  ``b_over_c``: what the position gradient costs on top
of the batch's own call (the single field pays 1.04 - 1.10).  ``expected`` was written before the first run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run, from the code and from profiles/hashgrid_batch_points_bench.json, hashgrid_batch_lod_bench.json and the single
# field's joint figures alone; nobody has measured these routes.  Both sides gain the same second walk over the levels, so the
# loop / batch ratios of the training rows should be those of train_points without it; the gradient entry is a forward-sized launch, where a
# loop of single fields is bound by its launches and host path (0.1 - 0.15 ms a field), as on query.
EXPECTED = {
    "joint, 64 x 256 x 256": "train_points' 3 - 5 x over the loop (DESIGN 4.7.18: 3.0 - 5.2 x), with a level of detail the 2.4 x of DESIGN 4.7.20's step or above; "
                             "b / c 1.05 - 1.15: the walk re-gathers every corner, as on the single field (1.04 - 1.10), and the batch's step has less fixed "
                             "cost per field to hide it behind",
    "joint, 8 x 256 x 256": "3 - 5 x the loop; b / c 1.03 - 1.12",
    "joint, 64 tiles of 512 x 512": "1.5 - 2 x the loop (DESIGN 4.7.18: 1.8 x); b / c 1.05 - 1.15, the random second gather missing more at T 2^15",
    "grad, 64 x 256 x 256": "the loop 64 x (0.1 - 0.15 ms) = 6 - 10 ms; the batch one launch of about twice a query (decoder backward to the row and a second "
                            "gather): 0.5 - 1.2 ms; 6 - 15 x; b / c (over query) 1.6 - 2.5",
    "grad, 8 x 256 x 256": "0.8 - 1.3 ms against 0.15 - 0.3 ms: 3 - 7 x",
    "grad, 64 tiles of 512 x 512": "a single field's 1024 wave items fill the chip: the batch wins the launches and host paths only, 1.1 - 2 x",
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


def row(n_fields, size, log2_table, points, with_lod, dev, warm=2, reps=10):
    """``points`` [B, n, 2] on the device, in any order: they are laid out in cell order here, once"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch, hash_batch_point_order
    kw = dict(levels=8, features=2, log2_table=log2_table, device=dev)
    joint, alone = HashGridFieldBatch(n_fields, size, seed=0, **kw), HashGridFieldBatch(n_fields, size, seed=0, **kw)
    singles = [joint.extract(b) for b in range(n_fields)]
    assert all(f.route == "fused" for f in singles)
    n = points.shape[1]
    order = hash_batch_point_order(joint.geo, points).long()
    points = torch.gather(points, 1, order.unsqueeze(-1).expand(-1, -1, 2)).contiguous()
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand(n_fields, n, 3, generator=g, device=dev)
    lod = (torch.rand(n_fields, n, generator=g, device=dev) * 3.0).contiguous() if with_lod else None
    dp = torch.empty(n_fields, n, 2, device=dev)
    dps = [torch.empty(n, 2, device=dev) for _ in range(n_fields)]
    lods = [None if lod is None else lod[b].contiguous() for b in range(n_fields)]
    own = [(points[b].contiguous(), target[b].contiguous()) for b in range(n_fields)]
    fns = {"loop_joint": lambda: [f.train_points(p, t, fused=True, dpoints=d, lod=l) for f, (p, t), d, l in zip(singles, own, dps, lods)],
           "batch_joint": lambda: joint.train_points_grad(points, target, dpoints=dp, lod=lod),
           "batch_train": (lambda: alone.train_points(points, target)) if lod is None else (lambda: alone.train_points_lod(points, target, lod)),
           "loop_grad": lambda: [f.point_gradient(p, target=t, lod=l) for f, (p, t), l in zip(singles, own, lods)],
           "batch_grad": lambda: joint.point_gradient(points, target=target, lod=lod),
           "batch_query": (lambda: joint.query(points)) if lod is None else (lambda: joint.query_lod(points, lod))}
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
    for a, b, c in (("loop_joint", "batch_joint", "batch_train"), ("loop_grad", "batch_grad", "batch_query")):
        out[b]["ships"] = out[b]["median_ms"] < out[a]["median_ms"] - (out[a]["max_ms"] - out[a]["min_ms"])
        out[b]["a_over_b"] = round(out[a]["median_ms"] / out[b]["median_ms"], 3)
        out[b]["b_over_c"] = round(out[b]["median_ms"] / out[c]["median_ms"], 3)
    out.update({"fields": n_fields, "shape": [*size], "levels": 8, "features": 2, "log2_table": log2_table, "points_per_field": n,
                "lod": "per point, uniform in [0, 3)" if with_lod else "none", "order": "laid out in cell order", "groups_per_field": "automatic"})
    return out


def random_points(n_fields, size, n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(n_fields, n, 2, generator=g, device=dev) * torch.tensor(size, device=dev, dtype=torch.float32) - 0.5).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="all", choices=["small", "tiles", "all"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_batch_pointgrad", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
    for with_lod in (False, True):
        tag = "_lod" if with_lod else ""
        if a.rows in ("small", "all"):
            for n_fields in (64, 8):
                res[f"B{n_fields}_256_n16384{tag}"] = row(n_fields, (256, 256), 12, random_points(n_fields, (256, 256), 1 << 14, dev, 2), with_lod, dev)
                torch.cuda.empty_cache()
        if a.rows in ("tiles", "all"):
            res[f"B64_tiles_512_T15_n65536{tag}"] = row(64, (512, 512), 15, random_points(64, (512, 512), 1 << 16, dev, 3), with_lod, dev)
            torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
