"""B stored hash-grid fields per launch on the 16-bit matrix pipe (hashgrid.py, HashGridFieldBatch.decode / resample(precision=);
csrc/hashgrid_fused16.hip, hash_batch16_kernel) against the two routes a user had before; prints one JSON line:

    python ab/bench_hashgrid_batch_p16.py [--out profiles/hashgrid_batch_p16_bench.json] [--rows small|tiles|all]

Rows: ab/bench_hashgrid_batch_stored.py's - 8 and 64 fields of 256 x 256 (L 8, F 2, T 2^12), ``decode()`` and ``resample((128, 128))``, and 64
tiles of 512 x 512 (T 2^15), ``decode()``, each from the uint8 files and from the bit-packed files at b = 4.  Per row, in ONE process and
interleaved call by call:
  (a)  ``batch``: the batch at ``precision=None`` - today's fp32 launch, untouched;
  (b)  ``loop_<p>``: a loop over ``HashGridField.load_compressed(path, fused=True)`` of the same files with ``precision=p`` - untouched too;
  (c)  ``batch_<p>``: the batch with ``precision=p``, p = split and bf16, ``groups_per_field`` automatic (the doubled cap at L F <= 32);
  (c') ``batch_<p>_cap1``: (c) with the G the undoubled cap would give (``hash_batch_groups`` on one workgroup per CU), where that differs.
HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum.  ``ships``: (c)'s median lies below the minimum of both
(a) and (b) of the same run.  ``doubled_cap_wins``: (c)'s median lies below (c')'s minimum.  ``parity``: the largest absolute difference between
(c) and (b).  The tables are random values of the quantiser's range (the time of a gather does not depend on what it reads); ``expected`` was
written before the first run."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run.  Nobody has measured this kernel.  The priors: DESIGN 4.7.14's rows for (a) (0.24 / 1.40 ms decode at B = 8 / 64,
# 0.19 / 0.52 ms resample, 5.3 ms on the tiles), 4.7.10's 1.9 x (split) / 2.2 x (bf16) where the decoder binds, and a prologue that now converts
# the decoder to bf16 images once per workgroup.
EXPECTED = {
    "decode_256": "(c) against (a): 1.2 - 1.6 x at B = 8 (about 0.16 - 0.20 ms; 512 workgroups of 4 groups each, the prologue is a larger share) and "
                  "1.5 - 1.8 x at B = 64 (about 0.8 - 0.9 ms: the decoder halves, the gather and the prologue do not); bf16 5 - 10 % under split. "
                  "(b) is launch-bound - 8 / 64 launches of a 256 x 256 field, about 0.5 / 3.8 ms as the fp32 loop of 4.7.14 - and loses to both.",
    "resample_128": "64 wave items a field and a host path that makes the points: (a) is 0.19 / 0.52 ms of which little is decoder. (c) about equal "
                    "to (a) at B = 8 (may not ship), 1.1 - 1.3 x at B = 64; (b) pays points and a launch per field, 1 / 9 ms.",
    "tiles_512_T15": "4096 patches a field fill the chip, so this is 4.7.10's case: (c) 1.6 - 1.9 x against (a)'s 5.3 ms (split about 3.0 ms, bf16 "
                     "about 2.7 ms). (b), 64 launches of 1024 groups on the doubled grid, is close behind (c): about 1.1 - 1.3 x, as 4.7.13's tiles.",
    "cap": "G differs only at B = 8 (64 against 32 workgroups a field; at B = 64 both caps give 8): the doubled cap hides the prologue and the "
           "gathers behind a second workgroup per CU, expected 5 - 15 % faster on decode, inside the spread on resample.",
}
MODES = ("split", "bf16")


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


def compare(fns, warm=2, reps=10):
    """``fns``: route -> callable, timed interleaved call by call"""
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
    for p in MODES:
        c, rivals = out[f"batch_{p}"], (out["batch"], out[f"loop_{p}"])
        floor = min(r["min_ms"] for r in rivals)
        out[f"ships_{p}"] = c["median_ms"] < floor
        out[f"batch_over_batch_{p}"] = round(out["batch"]["median_ms"] / c["median_ms"], 3)
        out[f"loop_over_batch_{p}"] = round(out[f"loop_{p}"]["median_ms"] / c["median_ms"], 3)
        if f"batch_{p}_cap1" in out:
            out[f"doubled_cap_wins_{p}"] = c["median_ms"] < out[f"batch_{p}_cap1"]["min_ms"]
        got, ref = fns[f"batch_{p}"](), torch.stack(fns[f"loop_{p}"]())
        out[f"parity_{p}"] = float((got.double() - ref.double()).abs().max())
    return out


def routes_of(batch, cap1, singles, call):
    """the routes of one row; ``call(field_or_batch, precision)`` makes the call under test"""
    fns = {"batch": lambda: call(batch, None)}
    for p in MODES:
        fns[f"loop_{p}"] = lambda p=p: [call(f, p) for f in singles]
        fns[f"batch_{p}"] = lambda p=p: call(batch, p)
        if cap1 is not None:
            fns[f"batch_{p}_cap1"] = lambda p=p: call(cap1, p)
    return fns


def rows(n_fields, size, log2_table, dev, resample):
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch, _patches, hash_batch_groups, hash_batch_groups_p16
    cap = max(torch.cuda.get_device_properties(dev).multi_processor_count // 8 * 8, 8)
    out = {"fields": n_fields, "shape": [*size], "levels": 8, "features": 2, "log2_table": log2_table, "num_bits": 4, "workgroup_cap": cap}
    with tempfile.TemporaryDirectory() as folder:
        files = write_files(n_fields, size, log2_table, 4, folder, dev)
        for packed, form in ((False, "u8"), (True, "bits4")):
            batch = HashGridFieldBatch.load_compressed(files[packed], device=dev)
            singles = [HashGridField.load_compressed(p, device=dev, fused=True) for p in files[packed]]
            assert batch.decode_only and all(f.route == "fused" and f.table is None for f in singles)
            calls = [("decode", _patches(batch.geo, 1, size), lambda f, p: f.decode(precision=p))]
            if resample:
                n = resample[0] * resample[1]
                calls.append((f"resample_{resample[0]}", (n + 63) // 64, lambda f, p: f.resample(resample, precision=p)))
            for name, items, call in calls:
                g2, g1 = hash_batch_groups_p16(n_fields, items, cap, False), hash_batch_groups(n_fields, items, cap)
                cap1 = HashGridFieldBatch.load_compressed(files[packed], device=dev, groups_per_field=g1) if g1 != g2 else None
                row = compare(routes_of(batch, cap1, singles, call))
                row["groups_per_field"] = {"automatic": g2, "undoubled_cap": g1}
                out[f"{name}_{form}"] = row
                del cap1
            del batch, singles
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="all", choices=["small", "tiles", "all"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_batch_p16", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
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
