"""B hash-grid fields per launch with gradients to the level of detail against a loop of B single fused fields (hashgrid.py,
HashGridFieldBatch.train_points_grad_lod / point_gradient_lod; csrc/hashgrid_batch.hip, hash_batch_points_joint_lod_kernel;
csrc/hashgrid_batch_grad.hip, hash_batch_points_grad_kernel<.., DLOD>); prints one JSON line:

    python ab/bench_hashgrid_batch_lodgrad.py [--out profiles/hashgrid_batch_lodgrad_bench.json] [--rows small|tiles|all]

Rows, those of ab/bench_hashgrid_batch_pointgrad.py: 8 and 64 fields of 256 x 256 (L 8, F 2, T 2^12) with 2^14 uniformly random points each,
and 64 tiles of 512 x 512 (T 2^15) with 2^16 points each; a level of detail per point, the points laid out in cell order once, before the
timed region, as a fixed point set has them.  Per row, in ONE process and interleaved call by call:

  (a) ``loop_joint``: the loop of ``extract(b).train_points_grad_lod(fused=True)`` over the fields - the route that exists without this code -,
      and ``loop_grad``: their ``point_gradient_lod(target=)``;
  (b) ``batch_joint``: ``HashGridFieldBatch.train_points_grad_lod``, and ``batch_grad``: ``HashGridFieldBatch.point_gradient_lod(target=)``;
  (c) ``batch_sibling_joint``: the batch's ``train_points_grad(lod=)``, and ``batch_sibling_grad``: its ``point_gradient(lod=)`` - the same
      calls without ``dlod``.

Training calls are whole steps, optimiser included.  HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum.
``ships``: the project's rule - (b)'s median lies below (a)'s minimum.  ``b_over_c``: what ``dlod`` costs on top of the batch's own call,
recorded and not bounded in advance (the single field measured 0.99 - 1.03).  ``expected`` was written before the
first run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run, from the code and from profiles/hashgrid_batch_pointgrad_bench.json and the single field's figures (DESIGN
# 4.7.22, 4.7.23) alone; nobody has measured these routes.  Both sides run the same walk with one more accumulator and one more store per
# point, so the loop / batch ratios should be those of the position gradients with a level of detail (4.4 - 4.8 x on the small
# fields), and dlod itself should cost what it costs the single field: within a few per cent of nothing.
EXPECTED = {
    "joint, 64 x 256 x 256": "train_points_grad(lod=)'s 4 - 5 x over the loop (DESIGN 4.7.21: 4.4 - 4.8 x); b / c 0.98 - 1.05",
    "joint, 8 x 256 x 256": "3 - 5 x the loop; b / c 0.98 - 1.05",
    "joint, 64 tiles of 512 x 512": "1.3 - 2 x the loop: a single tile's 1024 wave items fill the chip, the batch wins launches and host paths; b / c 0.98 - 1.05",
    "grad, 64 x 256 x 256": "the loop 64 x (0.1 - 0.15 ms) = 6 - 10 ms against one launch of 0.5 - 1.2 ms: 6 - 15 x; b / c 0.98 - 1.05",
    "grad, 8 x 256 x 256": "0.8 - 1.3 ms against 0.15 - 0.3 ms: 3 - 7 x; b / c 0.98 - 1.05",
    "grad, 64 tiles of 512 x 512": "1.1 - 2 x; b / c 0.98 - 1.05",
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


def row(n_fields, size, log2_table, points, dev, warm=2, reps=10):
    """``points`` [B, n, 2] on the device, in any order: they are laid out in cell order here, once"""
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch, hash_batch_point_order
    kw = dict(levels=8, features=2, log2_table=log2_table, device=dev)
    joint, sibling = HashGridFieldBatch(n_fields, size, seed=0, **kw), HashGridFieldBatch(n_fields, size, seed=0, **kw)
    singles = [joint.extract(b) for b in range(n_fields)]
    assert all(f.route == "fused" for f in singles)
    n = points.shape[1]
    order = hash_batch_point_order(joint.geo, points).long()
    points = torch.gather(points, 1, order.unsqueeze(-1).expand(-1, -1, 2)).contiguous()
    g = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand(n_fields, n, 3, generator=g, device=dev)
    lod = (torch.rand(n_fields, n, generator=g, device=dev) * 3.0).contiguous()
    dp, dl = torch.empty(n_fields, n, 2, device=dev), torch.empty(n_fields, n, device=dev)
    dps, dls = [torch.empty(n, 2, device=dev) for _ in range(n_fields)], [torch.empty(n, device=dev) for _ in range(n_fields)]
    own = [(points[b].contiguous(), target[b].contiguous(), lod[b].contiguous()) for b in range(n_fields)]
    fns = {"loop_joint": lambda: [f.train_points_grad_lod(p, t, l, d, e, fused=True) for f, (p, t, l), d, e in zip(singles, own, dps, dls)],
           "batch_joint": lambda: joint.train_points_grad_lod(points, target, lod, dp, dl),
           "batch_sibling_joint": lambda: sibling.train_points_grad(points, target, dpoints=dp, lod=lod),
           "loop_grad": lambda: [f.point_gradient_lod(p, l, target=t) for f, (p, t, l) in zip(singles, own)],
           "batch_grad": lambda: joint.point_gradient_lod(points, lod, target=target),
           "batch_sibling_grad": lambda: joint.point_gradient(points, target=target, lod=lod)}
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
    for a, b, c in (("loop_joint", "batch_joint", "batch_sibling_joint"), ("loop_grad", "batch_grad", "batch_sibling_grad")):
        out[b]["ships"] = out[b]["median_ms"] < out[a]["min_ms"]
        out[b]["a_over_b"] = round(out[a]["median_ms"] / out[b]["median_ms"], 3)
        out[b]["b_over_c"] = round(out[b]["median_ms"] / out[c]["median_ms"], 3)
    out.update({"fields": n_fields, "shape": [*size], "levels": 8, "features": 2, "log2_table": log2_table, "points_per_field": n,
                "lod": "per point, uniform in [0, 3)", "order": "laid out in cell order", "groups_per_field": "automatic"})
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
    res = {"bench": "hashgrid_batch_lodgrad", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
    if a.rows in ("small", "all"):
        for n_fields in (8, 64):
            res[f"B{n_fields}_256_n16384_lod"] = row(n_fields, (256, 256), 12, random_points(n_fields, (256, 256), 1 << 14, dev, 2), dev)
            torch.cuda.empty_cache()
    if a.rows in ("tiles", "all"):
        res["B64_tiles_512_T15_n65536_lod"] = row(64, (512, 512), 15, random_points(64, (512, 512), 1 << 16, dev, 3), dev)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
