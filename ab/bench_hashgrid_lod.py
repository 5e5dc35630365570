"""The hash-grid field's per-point level of detail (hashgrid.py query / train_points(lod=), decode_mip; csrc/hash_points.hip, csrc/hash_points_train.hip): what
the lambda = 0 lod routes cost over the plain point routes, and what a mip costs against the full decode and against point-sampling the
full-detail field at the mip's size; prints one JSON line:

    python ab/bench_hashgrid_lod.py [--out FILE] [--reps N]

The method of ab/bench_hashgrid_points.py: one process, HIP events around each call, the variants interleaved call by call, 2 + 10 rounds,
medians with min - max.  At 3840 x 2160, L 16, F 2, T 2^19, on ``raster`` (the 8.29 M sample centres) and ``random`` (8.29 M uniformly random
points, walked in a precomputed cell order where an order applies).  Per kernel pair: ``plain`` (the entry without _lod), ``lod_null``
(lod = NULL, lod_uniform = 0), ``lod_zeros`` (a zero tensor), ``lod_3`` (lod_uniform = 3: the four finest levels are skipped).  Nothing is
asserted on times.  ``expected`` holds what was written down before the first run.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = {
    "lambda_0": "lod_null and lod_zeros within 0 - 5 % of plain on every pair: per point one lod load (zeros only), per level one subtract, one "
                "add, two clamps, a ballot and F multiplies beside 4 gathers and 8 F multiply-adds; the kernels are bound by the gathers of the "
                "hashed levels (encode, query) and by the atomics (backward, step)",
    "lod_3": "the default fade at 4K falls 0.53 octaves per level: lambda = 3 switches levels 12 .. 15 off and fades level 11 - a quarter of the "
             "levels, all hashed and cache-hostile, so 25 - 40 % off the encode and the query, less off the backward (its coarse levels carry "
             "the contended atomics) and off the step (the decoder's share does not move)",
    "mips": "decode_mip(m) gathers 4^-m of the points and 16, 15, 14, 12 of the 16 levels at m = 0 .. 3, the skipped ones the most expensive: "
            "0.25, 0.06, 0.016 of decode() or a little less, above the launch floor of ~ 0.1 ms; against resample at the same size (same "
            "points, all levels) 0 - 10 % less at m = 1, 10 - 20 % at m = 2, 25 - 40 % at m = 3",
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


def over_plain(t):
    return {k: round(v[0] / t["plain"][0], 3) for k, v in t.items() if k != "plain"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    dev = torch.device("cuda:0")
    size = (3840, 2160)
    field = HashGridField(size, device=dev, seed=0, fused=True)
    assert field.route == "fused"
    geo, table = field.geo, field.table.detach()
    params = [p.detach() for p in field.decoder.linear_params()]
    n = size[0] * size[1]
    g = torch.Generator(device=dev).manual_seed(1)
    S = torch.tensor([float(s) for s in size], device=dev)
    sets = {"raster": field._resample_points(size, (0, 0), size), "random": (torch.rand(n, 2, generator=g, device=dev) * S - 0.5).contiguous()}
    target = torch.rand(n, 3, generator=g, device=dev)
    zeros = torch.zeros(n, device=dev)
    res = {"bench": "hashgrid_lod", "device": torch.cuda.get_device_name(0), "shape": list(size), "levels": 16, "features": 2, "log2_table": 19,
           "reps": a.reps, "fade": [round(v, 4) for v in hg.hash_lod_fade(geo)], "expected": EXPECTED, "sets": {}}
    for name, pts in sets.items():
        order = hg.hash_point_order(geo, pts) if name == "random" else None
        dx = torch.rand(n, geo.width, generator=g, device=dev) * 2 - 1
        grad = torch.zeros_like(table)
        entry = {"points": n, "order": "precomputed cell order" if order is not None else None}
        t = interleaved({"plain": lambda: hg.hash_encode_points(geo, table, pts),
                         "lod_null": lambda: hg.hash_encode_points_lod(geo, table, pts),
                         "lod_zeros": lambda: hg.hash_encode_points_lod(geo, table, pts, zeros),
                         "lod_3": lambda: hg.hash_encode_points_lod(geo, table, pts, None, 3.0)}, 2, a.reps)
        entry["encode_ms"], entry["encode_over_plain"] = t, over_plain(t)
        t = interleaved({"plain": lambda: hg.hash_encode_points_backward(geo, pts, dx, grad, order=order),
                         "lod_null": lambda: hg.hash_encode_points_backward_lod(geo, pts, dx, grad, order=order),
                         "lod_zeros": lambda: hg.hash_encode_points_backward_lod(geo, pts, dx, grad, zeros, order=order),
                         "lod_3": lambda: hg.hash_encode_points_backward_lod(geo, pts, dx, grad, None, 3.0, order=order)}, 2, a.reps)
        entry["backward_ms"], entry["backward_over_plain"] = t, over_plain(t)
        del dx, grad
        t = interleaved({"plain": lambda: hg.hash_fused_forward_points(geo, table, pts, params),
                         "lod_null": lambda: hg.hash_fused_forward_points_lod(geo, table, pts, params),
                         "lod_zeros": lambda: hg.hash_fused_forward_points_lod(geo, table, pts, params, zeros),
                         "lod_3": lambda: hg.hash_fused_forward_points_lod(geo, table, pts, params, None, 3.0)}, 2, a.reps)
        entry["fused_query_ms"], entry["fused_query_over_plain"] = t, over_plain(t)
        pre = order if order is not None else hg.hash_point_order(geo, pts)
        t = interleaved({"plain": lambda: field.train_points(pts, target, order=pre, fused=True),
                         "lod_null": lambda: field.train_points(pts, target, order=pre, fused=True, lod=0.0),
                         "lod_zeros": lambda: field.train_points(pts, target, order=pre, fused=True, lod=zeros),
                         "lod_3": lambda: field.train_points(pts, target, order=pre, fused=True, lod=3.0)}, 2, a.reps)
        entry["fused_cell_step_ms"], entry["fused_cell_step_over_plain"] = t, over_plain(t)
        res["sets"][name] = entry
        torch.cuda.empty_cache()
    fns = {"decode": lambda: field.decode()}
    for m in (1, 2, 3):
        fns[f"decode_mip_{m}"] = lambda m=m: field.decode_mip(m)
        fns[f"resample_{m}"] = lambda m=m: field.resample(tuple(s >> m for s in size))
    t = interleaved(fns, 2, a.reps)
    res["mips_ms"] = t
    res["mip_over_decode"] = {f"m{m}": round(t[f"decode_mip_{m}"][0] / t["decode"][0], 4) for m in (1, 2, 3)}
    res["mip_over_resample"] = {f"m{m}": round(t[f"decode_mip_{m}"][0] / t[f"resample_{m}"][0], 4) for m in (1, 2, 3)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
