"""The gradient with respect to the level of detail: what ``dlod`` costs on top of the position gradient (hashgrid.py,
csrc/hashgrid_lodgrad.hip); prints one JSON line:

    python ab/bench_hashgrid_lodgrad.py [--out profiles/hashgrid_lodgrad_bench.json]

4K (3840 x 2160; L 16, F 2, T 2^19; 8.29 M points: the sample centres in raster order, and as many uniformly random points), in ONE process, the
routes of a row interleaved call by call, HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum.  A row is an
order (raster, random), a table (fp32, uint8 b = 8, packed b = 4) and a level of detail (0, 3, one per point uniform in [0, 3]).  Routes of a row:
- ``sibling``: ``point_gradient(lod=)`` of a ``fused=True`` field - nic_hash_fused_points_grad with a level of detail, this build's untouched kernel;
- ``fused``: ``point_gradient_lod`` of the same field - nic_hash_fused_points_grad_lod, one launch;
- ``layerwise``: ``point_gradient_lod`` of a layer-wise field - encode_lod, general decoder forward and backward, nic_hash_encode_points_grad_lod.
``vs_sibling_median``: the fused median over the sibling's.  ``ships``: the fused median lies below the layer-wise composition's minimum of the
same run (the rule of DESIGN 4.7.11).  ``expected`` was written before the first run."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run; nobody has measured this.  The new walk is the sibling's with one accumulator per level (one more fmaf per corner
# and D - 1 multiplies for the full corner weight), one subtract per live level and one 4-byte store per point next to the 8 or 12 bytes of
# dpoints: no extra gather, no extra LDS, the same decoder.
EXPECTED = {
    "fused_vs_sibling": "the sibling plus a few percent (1.00 - 1.05 x) on every row: one accumulator and one extra store per point, no extra gather",
    "lod3": "as at lod 0: the four finest of 16 levels are gathered by no wave in either kernel, the ratio does not move",
    "per_point": "between the lod 0 and the lod 3 row in time (most waves keep most levels), the same ratio",
    "stored_tables": "the uint8 and packed rows within 10 % of the f32 row, as for the sibling (DESIGN 4.7.11)",
    "ships": "true on every row: the layer-wise composition moves the [N, 32] row through HBM four times and launches five kernels",
}
ROUTES = ("sibling", "fused", "layerwise")


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
    out["fused"]["vs_sibling_median"] = round(out["fused"]["median_ms"] / out["sibling"]["median_ms"], 3)
    out["fused"]["ships"] = out["fused"]["median_ms"] < out["layerwise"]["min_ms"]
    return out


def loaded(size, dev, num_bits, packed):
    """(fused, layer-wise) fields from one stored file"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    with tempfile.TemporaryDirectory() as tmp:
        q = HashGridField(size, device=dev, seed=0, num_bits=num_bits)
        q.freeze()
        path = os.path.join(tmp, "f.pt")
        q.save_compressed(path, packed=packed)
        del q
        return HashGridField.load_compressed(path, dev, fused=True), HashGridField.load_compressed(path, dev, fused=False)


def fields(size, dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f, lw = HashGridField(size, device=dev, seed=0, fused=True), HashGridField(size, device=dev, seed=0)
    assert f.route == "fused" and lw.route == "layerwise"
    return {"f32": (f, lw), "u8_b8": loaded(size, dev, 8, False), "packed_b4": loaded(size, dev, 4, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    size = (3840, 2160)
    fs = fields(size, dev)
    res = {"bench": "hashgrid_lodgrad", "device": torch.cuda.get_device_name(0), "expected": EXPECTED, "shape": [*size], "levels": 16, "features": 2,
           "log2_table": 19}
    g = torch.Generator(device=dev).manual_seed(1)
    lattice = fs["f32"][0]._resample_points(size, (0, 0), size)
    n = lattice.shape[0]
    res["points"] = n
    orders = {"raster": lattice,
              "random": (torch.rand(n, 2, generator=g, device=dev) * torch.tensor([float(s) for s in size], device=dev) - 0.5).contiguous()}
    dy = torch.rand(n, 3, generator=g, device=dev) * 2 - 1
    lods = {"lod0": 0.0, "lod3": 3.0, "per_point_0_3": (torch.rand(n, generator=g, device=dev) * 3.0).contiguous()}
    for order, pts in orders.items():
        res[order] = {}
        for table, (f, lw) in fs.items():
            for name, lod in lods.items():
                res[order][f"{table}_{name}"] = row({"sibling": lambda: f.point_gradient(pts, dy=dy, lod=lod), "fused": lambda: f.point_gradient_lod(pts, lod, dy=dy),
                                                     "layerwise": lambda: lw.point_gradient_lod(pts, lod, dy=dy)})
    rows = [v for order in orders for v in res[order].values()]
    ratios = [v["fused"]["vs_sibling_median"] for v in rows]
    res["vs_sibling_median"] = {"min": min(ratios), "median": round(statistics.median(ratios), 3), "max": max(ratios)}
    res["ships"] = all(v["fused"]["ships"] for v in rows)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
