"""B STORED hash-grid fields per launch against a loop of B single decode-only fields (hashgrid.py, HashGridFieldBatch.load_compressed;
csrc/hashgrid_batch.hip, hash_batch_decode_kernel); prints one JSON line:

    python ab/bench_hashgrid_batch_stored.py [--out profiles/hashgrid_batch_stored_bench.json] [--rows small|tiles|all]

Rows: 8 and 64 fields of 256 x 256 (L 8, F 2, T 2^12) - ``decode()`` and ``resample((128, 128))`` - and 64 tiles of 512 x 512 (T 2^15) -
``decode()`` -, each from the uint8 files and from the bit-packed files at b = 4 that ``save_compressed`` wrote.  Per row, in ONE process and
interleaved call by call: ``HashGridFieldBatch.load_compressed(paths)`` against a loop over ``HashGridField.load_compressed(path, fused=True)``
of the same files - that code is untouched, so it is the parent's.  HIP events around each call, 2 warm-up and 10 timed rounds: median,
minimum, maximum.  ``ships``: the batch's median lies below the loop's minimum of the same run.  ``parity``: the largest absolute difference
between the two results.  The tables are random values of the quantiser's range (the time of a gather does not depend on what it reads, a
fit would only make the run longer); ``expected`` was written before the first run."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run.  Nobody has measured these kernels; the priors come from others: DESIGN 4.7.13's fp32 decode rows (2.4 x at
# B = 8, 3.0 x at B = 64, 1.3 x on the tiles) and 4.7.3's +2.7 % for the packed gather against the uint8 one.
EXPECTED = {
    "decode_256": "about 4.7.13's fp32 rows: 2 - 3 x at B = 8 and B = 64 from either stored form (a 256 x 256 decode is launch- and prologue-bound, "
                  "the bytes of the gather do not show); packed within a few percent of uint8",
    "resample_128": "a larger ratio than decode: the loop generates the points of every field (a meshgrid and a stack per field) where the batch "
                    "generates them once and expands; 256 wave items a field",
    "tiles_512_T15": "about 4.7.13's 1.3 x: 4096 patches a field fill the chip alone, the batch saves launches and host paths only",
}
ROUTES = ("loop", "batch")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "n": len(ts)}


def write_files(n_fields, size, log2_table, num_bits, folder, dev):
    """B fields with random tables of the quantiser's range and their own decoders, frozen and saved in both forms -> {packed: paths}"""
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    batch = HashGridFieldBatch(n_fields, size, levels=8, features=2, log2_table=log2_table, device=dev, seed=0, num_bits=num_bits)
    lo, hi = models._q_range(num_bits)
    with torch.no_grad():
        batch.tables.uniform_(lo, hi, generator=torch.Generator(device=dev).manual_seed(1))
    batch.freeze()
    files = {}
    for packed in (False, True):
        files[packed] = [os.path.join(folder, f"{n_fields}_{size[0]}_{int(packed)}_{b}.pt") for b in range(n_fields)]
        batch.save_compressed(files[packed], packed=packed)
    return files


def compare(loop_fn, batch_fn, warm=2, reps=10):
    fns = {"loop": loop_fn, "batch": batch_fn}
    for _ in range(warm):
        for r in ROUTES:
            fns[r]()
    torch.cuda.synchronize()
    ts = {r: [] for r in ROUTES}
    for _ in range(reps):
        for r in ROUTES:
            ts[r].append(timed(fns[r]))
    out = {r: stats(ts[r]) for r in ROUTES}
    out["ships"] = out["batch"]["median_ms"] < out["loop"]["min_ms"]
    out["loop_over_batch_median"] = round(out["loop"]["median_ms"] / out["batch"]["median_ms"], 3)
    got, ref = batch_fn(), torch.stack(loop_fn())
    out["parity"] = float((got.double() - ref.double()).abs().max())
    return out


def rows(n_fields, size, log2_table, dev, resample):
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch
    out = {"fields": n_fields, "shape": [*size], "levels": 8, "features": 2, "log2_table": log2_table, "num_bits": 4, "groups_per_field": "automatic"}
    with tempfile.TemporaryDirectory() as folder:
        files = write_files(n_fields, size, log2_table, 4, folder, dev)
        for packed, form in ((False, "u8"), (True, "bits4")):
            batch = HashGridFieldBatch.load_compressed(files[packed], device=dev)
            singles = [HashGridField.load_compressed(p, device=dev, fused=True) for p in files[packed]]
            assert batch.decode_only and all(f.route == "fused" and f.table is None for f in singles)
            out[f"decode_{form}"] = compare(lambda: [f.decode() for f in singles], lambda: batch.decode())
            if resample:
                out[f"resample_{resample[0]}_{form}"] = compare(lambda: [f.resample(resample) for f in singles], lambda: batch.resample(resample))
            del batch, singles
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="all", choices=["small", "tiles", "all"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_batch_stored", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
    if a.rows in ("small", "all"):
        for n_fields in (8, 64):
            res[f"B{n_fields}_256"] = rows(n_fields, (256, 256), 12, dev, (128, 128))
    if a.rows in ("tiles", "all"):
        res["B64_tiles_512_T15"] = rows(64, (512, 512), 15, dev, None)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
