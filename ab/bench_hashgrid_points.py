"""The hash-grid field at arbitrary points against the crop route (hashgrid.py hash_encode_points / query / resample, csrc/hash_points.hip,
DESIGN 4.7.4); prints one JSON line:

    python ab/bench_hashgrid_points.py [--out FILE] [--reps N]

The method of ab/bench_hashgrid_packed.py: one process, HIP events around each call, warm-up first, the point kernels interleaved call by call
with the crop route's unchanged kernels (crop, points, crop, points ..), medians with min - max.  At 3840 x 2160, L 16, F 2, T 2^19 (11 dense
and 5 hashed levels), for three point sets:
- ``raster``: the 8.29 M sample centres in nic_encode order (the rows equal the crop route's bit for bit; a wave holds 64 consecutive y samples
  of one x, not an 8 x 8 patch);
- ``resample2x``: the 33.2 M points of ``resample((7680, 4320))``, tile by tile in raster order (times are reported per launch set and per point);
- ``random``: 8.29 M uniformly random points (no gather locality, no runs for the backward's run sums).
Per set: ``forward`` (hash_encode_points against hash_encode of the whole field), ``backward`` (hash_encode_points_backward against
hash_encode_backward) and ``fused_query`` (hash_fused_forward_points against hash_fused_forward).  ``expected`` holds what DESIGN 4.7.4 wrote
down before the first run.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ab.bench_hashgrid_codec import timed      # noqa: E402

EXPECTED = {
    "raster": "forward within 1.5x of the crop route (both bound by the row writes; the hashed levels gather from ~128 lines per wave instead of "
              "~18); backward 1 - 2x (the same long runs at the coarse levels, scattered atomics at the hashed ones); fused query 1 - 2x",
    "resample2x": "per point like raster or better: neighbouring points share cells, so runs are longer and gathers hit the same lines",
    "random": "forward 3 - 6x per point (every corner its own line, from L2 / MALL: the 67 MB table fits); backward near the 189 ms of the "
              "no-run-sum A/B (DESIGN 4.7): neighbouring lanes share no cell, so the coarse levels add 8.3 M times into a few hundred addresses",
}


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
    a = ap.parse_args()
    from neural_image_compression_v2_amd.hashgrid import (HashGridField, hash_encode, hash_encode_backward, hash_encode_points,
                                                          hash_encode_points_backward, hash_fused_forward, hash_fused_forward_points)
    dev = torch.device("cuda:0")
    size = (3840, 2160)
    field = HashGridField(size, device=dev, seed=0, fused=True)
    assert field.route == "fused"
    geo = field.geo
    with torch.no_grad():
        field.table.copy_(torch.rand(geo.table_shape(), device=dev) * 0.8 - 0.4)
    table = field.table.detach()
    params = [p.detach() for p in field.decoder.linear_params()]
    org = geo.upload_origins([[0, 0]], size, dev)
    n = size[0] * size[1]
    g = torch.Generator(device=dev).manual_seed(1)
    big = (2 * size[0], 2 * size[1])
    tiles = [(o, [min(1920, s - v) for s, v in zip(big, o)]) for o in ((x, y) for x in range(0, big[0], 1920) for y in range(0, big[1], 1920))]
    sets = {
        "raster": [field._resample_points(size, (0, 0), size)],
        "resample2x": [field._resample_points(big, o, e) for o, e in tiles],
        "random": [(torch.rand(n, 2, generator=g, device=dev) * torch.tensor([float(s) for s in size], device=dev) - 0.5).contiguous()],
    }
    rows_equal = bool(torch.equal(hash_encode_points(geo, table, sets["raster"][0]), hash_encode(geo, table, org, size)))
    grad = torch.zeros_like(table)
    dx_crop = torch.rand(n, geo.width, generator=g, device=dev) * 2 - 1
    res = {"bench": "hashgrid_points", "device": torch.cuda.get_device_name(0), "shape": list(size), "levels": 16, "features": 2, "log2_table": 19,
           "reps": a.reps, "raster_rows_equal_crop_rows": rows_equal, "expected": EXPECTED, "sets": {}}
    for name, chunks in sets.items():
        npts = sum(c.shape[0] for c in chunks)
        dxs = [dx_crop if c.shape[0] == n else torch.rand(c.shape[0], geo.width, generator=g, device=dev) * 2 - 1 for c in chunks]

        def fwd_points():
            for c in chunks:
                hash_encode_points(geo, table, c)

        def bwd_points():
            for c, d in zip(chunks, dxs):
                hash_encode_points_backward(geo, c, d, grad)

        def query_points():
            for c in chunks:
                hash_fused_forward_points(geo, table, c, params)

        fw = interleaved({"crop": lambda: hash_encode(geo, table, org, size), "points": fwd_points}, 2, a.reps)
        bw = interleaved({"crop": lambda: hash_encode_backward(geo, org, size, dx_crop, grad), "points": bwd_points}, 2, a.reps)
        qu = interleaved({"crop": lambda: hash_fused_forward(geo, table, org, size, params), "points": query_points}, 2, a.reps)
        per = lambda t, cnt: round(t[0] * 1e6 / cnt, 4)      # noqa: E731   ns per point, from the median
        res["sets"][name] = {
            "points": npts, "launches": len(chunks),
            "forward_ms": fw, "backward_ms": bw, "fused_query_ms": qu,
            "ns_per_point": {k: {"crop": per(v["crop"], n), "points": per(v["points"], npts)} for k, v in (("forward", fw), ("backward", bw), ("fused_query", qu))},
            "points_over_crop_per_point": {k: round((v["points"][0] / npts) / (v["crop"][0] / n), 3) for k, v in (("forward", fw), ("backward", bw), ("fused_query", qu))},
        }
        del dxs
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
