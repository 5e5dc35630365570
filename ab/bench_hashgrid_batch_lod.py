"""B hash-grid fields with a level of detail per point, decoded and trained per launch, against a loop of B single fields (hashgrid.py,
HashGridFieldBatch.decode_mip / train_points_lod; csrc/hashgrid_batch.hip, hash_batch_decode_lod_kernel and hash_batch_points_lod_kernel;
DESIGN 4.7.20); prints one JSON line:

    python ab/bench_hashgrid_batch_lod.py [--out profiles/hashgrid_batch_lod_bench.json] [--rows small|tiles|all]

Rows: 64 and 8 fields of 256 x 256 (L 8, F 2, T 2^12, num_bits 4) and 64 tiles of 512 x 512 (T 2^15).  Per row, in ONE process and
interleaved call by call:
  decode_mip(1 | 2 | 3) from the fp32 tables, from the uint8 files and from the bit-packed b = 4 files - the batch's one launch per mip against
  the loop of ``extract(b)`` / ``HashGridField.load_compressed(path, fused=True)`` fields' own ``decode_mip`` (the route without the batch);
  a whole training step, optimiser included, at the mip chain's points (mips 0 to 2: 86 016 points per 256 x 256 field, cell order precomputed)
  - ``HashGridFieldBatch.train_points_lod`` against the loop of ``HashGridField.train_points(fused=True, lod=, order=)``;
  the price of the lod code: the same step and the same query with lambda = 0 everywhere against the plain batch calls on the same points
  (the single field measured 1.00 to 1.06, profiles/hashgrid_lod_bench.json); reported, not gated.
HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum.  ``ships``: the batch's median lies below the loop's
minimum of the same run.  ``expected`` was written before the first run."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run, from the code, profiles/hashgrid_batch_points_bench.json (the plain step at 2^14 points: loop 7.2 ms, batch
# 1.6 ms at 64 fields; 0.95 / 0.32 ms at 8; tiles at 2^16 points 10.7 / 6.0 ms) and profiles/hashgrid_batch_stored_bench.json alone.  Nobody has
# measured any of this and no number is a target.
EXPECTED = {
    "decode_mip": "a mip of a 256 x 256 field is 16384 / 4096 / 1024 points = 256 / 64 / 16 wave items: a single field cannot fill the chip and its call "
                  "is bound by the host path and the launch (0.04 - 0.08 ms whatever the mip), so the loop of 64 costs 2.5 - 5 ms at every mip; the batch "
                  "is one launch of 64 x those items plus the tile's points: 0.1 - 0.3 ms at mip 1 and less above: 10 - 30 x at 64 fields, 3 - 8 x at 8; "
                  "uint8 and packed sources within 20 % of fp32 on either side (tables of 2^12 entries sit in the cache)",
    "train_mips": "86016 points = 1344 wave items per field, five times the 2^14-point row: the loop 64 x (0.2 - 0.3 ms) = 13 - 19 ms, the batch's kernel "
                  "work grows with the points while its three launches stay: 5 - 8 ms; 2 - 3 x at 64 fields, about 2 x at 8",
    "lod_price": "lambda = 0 keeps every level live: the lod kernels pay the weight, a ballot per level and a multiply per column, as the single field "
                 "does (1.00 - 1.06): 1.00 - 1.08 for the step and for the query",
    "tiles": "512 x 512 tiles: a mip 1 is 65536 points = 1024 wave items and fills the chip from ONE field, the step's 344064 points more so: the batch "
             "wins launches and host paths only: decode_mip(1) 1.5 - 4 x, mips 2 and 3 nearer the small row's ratios, the training step 1.0 - 1.3 x",
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


def race(fns, warm=2, reps=10):
    """name -> stats of every route of ``fns``, interleaved call by call"""
    routes = list(fns)
    for _ in range(warm):
        for r in routes:
            fns[r]()
    torch.cuda.synchronize()
    ts = {r: [] for r in routes}
    for _ in range(reps):
        for r in routes:
            ts[r].append(timed(fns[r]))
    return {r: stats(ts[r]) for r in routes}


def versus(out, batch, loop):
    out[batch]["ships"] = out[batch]["median_ms"] < out[loop]["min_ms"]
    out[batch]["loop_over_batch_median"] = round(out[loop]["median_ms"] / out[batch]["median_ms"], 3)


def mip_set(field, size, mips, dev):
    """the single field's fit_mips construction without the colours: (points [n, 2], lod [n]) of mips 0 .. ``mips``"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    pts, lods = [], []
    for m in range(mips + 1):
        sz = tuple(s >> m for s in size)
        pts.append(HashGridField._resample_points(field, sz, [0, 0], sz))
        lods.append(torch.full((pts[-1].shape[0],), float(m), dtype=torch.float32, device=dev))
    return torch.cat(pts).contiguous(), torch.cat(lods).contiguous()


def row(n_fields, size, log2_table, dev, tmp, mips=(1, 2, 3)):
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch, hash_point_order
    kw = dict(levels=8, features=2, log2_table=log2_table, device=dev, num_bits=4)
    batch = HashGridFieldBatch(n_fields, size, seed=0, **kw)
    out = {}
    # ---- decode_mip from the three sources
    sources = {"f32": (batch, [batch.extract(b) for b in range(n_fields)])}
    for name, packed in (("u8", False), ("bits4", True)):
        paths = [os.path.join(tmp, f"{name}_{n_fields}_{size[0]}_{b}.pt") for b in range(n_fields)]
        batch.save_compressed(paths, packed=packed)
        sources[name] = (HashGridFieldBatch.load_compressed(paths, device=dev), [HashGridField.load_compressed(p, device=dev, fused=True) for p in paths])
    for name, (bt, singles) in sources.items():
        assert all(f.route == "fused" for f in singles)
        for m in mips:
            r = race({"loop": lambda: [f.decode_mip(m) for f in singles], "batch": lambda: bt.decode_mip(m)})
            versus(r, "batch", "loop")
            out[f"decode_mip{m}_{name}"] = r
    # ---- a training step at the mip chain's points, and the price of the lod code
    singles = [batch.extract(b) for b in range(n_fields)]
    plain = HashGridFieldBatch(n_fields, size, seed=0, **kw)
    zero = HashGridFieldBatch(n_fields, size, seed=0, **kw)
    pts, lod = mip_set(batch, size, 2, dev)
    n = pts.shape[0]
    target = torch.rand(n_fields, n, 3, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    order1 = hash_point_order(batch.geo, pts)
    order = order1.unsqueeze(0).expand(n_fields, -1).contiguous()
    own = [target[b].contiguous() for b in range(n_fields)]
    r = race({"loop": lambda: [f.train_points(pts, t, fused=True, order=order1, lod=lod) for f, t in zip(singles, own)],
              "batch": lambda: batch.train_points_lod(pts, target, lod, order=order),
              "batch_lambda0": lambda: zero.train_points_lod(pts, target, 0.0, order=order),
              "batch_plain": lambda: plain.train_points(pts, target, order=order)})
    versus(r, "batch", "loop")
    r["batch_lambda0"]["lod_over_plain_median"] = round(r["batch_lambda0"]["median_ms"] / r["batch_plain"]["median_ms"], 3)
    out["train_mips"] = r
    q = race({"query_lambda0": lambda: batch.query_lod(pts, 0.0), "query_plain": lambda: batch.query(pts)})
    q["query_lambda0"]["lod_over_plain_median"] = round(q["query_lambda0"]["median_ms"] / q["query_plain"]["median_ms"], 3)
    out["query_price"] = q
    out.update({"fields": n_fields, "shape": [*size], "levels": 8, "features": 2, "log2_table": log2_table, "num_bits": 4, "points_per_field": n,
                "order": "cell, precomputed", "groups_per_field": "automatic", "single_field_lod_over_plain": [1.00, 1.06]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="all", choices=["small", "tiles", "all"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_batch_lod", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
    with tempfile.TemporaryDirectory() as tmp:
        if a.rows in ("small", "all"):
            for n_fields in (64, 8):
                res[f"B{n_fields}_256"] = row(n_fields, (256, 256), 12, dev, tmp)
                torch.cuda.empty_cache()
        if a.rows in ("tiles", "all"):
            res["B64_tiles_512_T15"] = row(64, (512, 512), 15, dev, tmp)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
