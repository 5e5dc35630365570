"""The gradient with respect to the point coordinates: the fused entry against the layer-wise composition and the fused query (hashgrid.py,
csrc/hashgrid_pointgrad.hip); prints one JSON line:

    python ab/bench_hashgrid_pointgrad.py [--out profiles/hashgrid_pointgrad_bench.json] [--shape 4k|256cube|both]

4K (3840 x 2160; L 16, F 2, T 2^19; 8.29 M points: the sample centres in raster order, and as many uniformly random points) and the 256^3 field
on its lattice points, in ONE process, the routes of a row interleaved call by call, HIP events around each call, 2 warm-up and 10 timed rounds:
median, minimum, maximum.  Routes of a row:
- ``query``: the fused ``query`` (this build's untouched kernel, the yardstick);
- ``layerwise``: ``point_gradient`` of a layer-wise field - encode, general decoder forward and backward, nic_hash_encode_points_grad;
- ``fused_f32`` / ``fused_u8_b8`` / ``fused_packed_b4``: ``point_gradient`` of a ``fused=True`` field, one launch, from the three tables;
- ``fused_lod3``: the same from the fp32 table with ``lod=3.0``.
``ships``: the fused route's median lies below the layer-wise composition's minimum of the same run.  ``expected`` was written before the first run."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run.  By MFMA count per half tile at L F = 32 the backward to the input is 6 + 64 + 32 KT = 102 against the forward's
# 224, so forward + backward is ~1.46 x the query's matrix work, and the second walk over the levels re-gathers corners whose lines were fetched
# microseconds earlier (L2 hits for raster order; for random points the second gather misses like the first).  The layer-wise composition moves
# the [N, 32] row through HBM four times (encode writes it, the decoder forward and backward read it, the backward writes dx, the gradient
# kernel reads dx): 4 x 1.06 GB at 4K, ~1 ms at the achievable bandwidth, on top of five launches and two gathers.
EXPECTED = {
    "4k_raster_ms": {"query": "2.78 (README)", "fused_f32": "4 - 5.5 (1.5 x the query plus one more gather)", "layerwise": "well above the fused entry: 7 - 10"},
    "4k_random_ms": {"fused_f32": "the query's random-order time x 1.5 plus a second gather that misses like the first: up to 2 x the query"},
    "stored_tables": "the uint8 and packed rows within 10 % of the f32 row, as on the query (DESIGN 4.7.1 / 4.7.3)",
    "lod3": "faster than lod none: the four finest of 16 levels are gathered by no wave, twice",
    "256cube": "8 corners per level, twice: the gather weighs more, the ratio to the query is nearer 2 than 1.5",
}
ROUTES = ("query", "layerwise", "fused_f32", "fused_u8_b8", "fused_packed_b4", "fused_lod3")


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
    for r in ROUTES:
        if r.startswith("fused"):
            out[r]["ships"] = out[r]["median_ms"] < out["layerwise"]["min_ms"]
            out[r]["vs_query_median"] = round(out[r]["median_ms"] / out["query"]["median_ms"], 3)
    out["layerwise"]["vs_query_median"] = round(out["layerwise"]["median_ms"] / out["query"]["median_ms"], 3)
    return out


def loaded(size, dev, num_bits, packed):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    with tempfile.TemporaryDirectory() as tmp:
        q = HashGridField(size, device=dev, seed=0, num_bits=num_bits)
        q.freeze()
        path = os.path.join(tmp, "f.pt")
        q.save_compressed(path, packed=packed)
        del q
        return HashGridField.load_compressed(path, dev, fused=True)


def fields(size, dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = HashGridField(size, device=dev, seed=0, fused=True)
    lw = HashGridField(size, device=dev, seed=0)
    assert f.route == "fused" and lw.route == "layerwise"
    return f, lw, loaded(size, dev, 8, False), loaded(size, dev, 4, True)


def gradient_row(fs, pts, dev):
    f, lw, u8, packed = fs
    dy = torch.rand(pts.shape[0], 3, generator=torch.Generator(device=dev).manual_seed(2), device=dev) * 2 - 1
    return row({"query": lambda: f.query(pts), "layerwise": lambda: lw.point_gradient(pts, dy=dy), "fused_f32": lambda: f.point_gradient(pts, dy=dy),
                "fused_u8_b8": lambda: u8.point_gradient(pts, dy=dy), "fused_packed_b4": lambda: packed.point_gradient(pts, dy=dy),
                "fused_lod3": lambda: f.point_gradient(pts, dy=dy, lod=3.0)})


def leg(size, dev, random_too):
    fs = fields(size, dev)
    res = {"shape": [*size], "levels": 16, "features": 2, "log2_table": 19}
    lattice = fs[0]._resample_points(size, (0,) * len(size), size)
    res["points"] = lattice.shape[0]
    res["raster"] = gradient_row(fs, lattice, dev)
    if random_too:
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = (torch.rand(lattice.shape[0], len(size), generator=g, device=dev) * torch.tensor([float(s) for s in size], device=dev) - 0.5).contiguous()
        del lattice
        res["random"] = gradient_row(fs, rnd, dev)
    res["ships"] = all(v["ships"] for k in ("raster", "random") if k in res for r, v in res[k].items() if r.startswith("fused"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="both", choices=["4k", "256cube", "both"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_pointgrad", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
    if a.shape in ("4k", "both"):
        res["4k"] = leg((3840, 2160), dev, True)
        torch.cuda.empty_cache()
    if a.shape in ("256cube", "both"):
        res["256cube"] = leg((256, 256, 256), dev, False)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
