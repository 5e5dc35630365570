"""B hash-grid fields per launch against a loop of B single fused fields (hashgrid.py, HashGridFieldBatch; csrc/hashgrid_batch.hip);
prints one JSON line:

    python ab/bench_hashgrid_batch.py [--out profiles/hashgrid_batch_bench.json] [--rows small|tiles|all]

Rows: B = 1, 8 and 64 fields of 256 x 256 (L 8, F 2, T 2^12: the structured image of DESIGN 4.7.1), and 64 tiles of 512 x 512 cut from one
4096 x 4096 image (L 8, F 2, T 2^15).  Per row, in ONE process and interleaved call by call: the whole training step (``train_step`` on the
whole field, optimiser included) and ``decode()``, of the batch and of a loop over B ``HashGridField(fused=True)`` of the same build - that
code is untouched, so it is the parent's.  HIP events around each call, 2 warm-up and 10 timed rounds: median, minimum, maximum.  ``ships``:
the batch's median lies below the loop's minimum of the same run.  ``parity``: the largest difference between the two decodes over the
largest magnitude, at the sizes timed, from the same parameters.  ``expected`` was written before the first run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# written before the first run, from the code alone.  A single 256 x 256 step is two launches whose kernel stages a 33 KB decoder, zeroes its
# row tiles and writes a 5.5 K-float record per workgroup to train ONE group of four patches: prologue, epilogue and launch latency, with the
# host path of train_step (origins upload, tail table, two ctypes calls) on top - 0.1 - 0.3 ms per field as events see it, so a loop of 64 is
# 6 - 20 ms.  The batch at B = 64 runs 512 workgroups of 32 groups each, one workgroup per CU (134 KB of LDS): two rounds of ~32 x (5 - 10 us),
# 0.4 - 0.8 ms, plus one reduce and one optimiser launch and ONE host path.
EXPECTED = {
    "B1": "the batch loses or ties: three launches against two (the optimiser does not ride on the reduction), the same kernel work; 1.0 - 1.3 x the single step",
    "B8_step": "3 - 6 x faster than the loop: 256 workgroups of 8 groups each against 8 x (two launches + host path)",
    "B64_step": "8 - 20 x faster than the loop; the batch itself 0.5 - 1 ms, bound by 512 workgroups sharing 256 CUs at one workgroup per CU",
    "decode": "the forward kernel fits one workgroup per CU too (101 KB of LDS); one launch against B: 3 - 5 x at B = 8, 5 - 15 x at B = 64; B = 1 ties",
    "tiles_512_T15": "4096 patches per field fill the chip alone (1024 groups on 256 workgroups): the loop is no longer latency-bound, the batch wins by "
                     "the launches and host paths only: 1.2 - 2 x on the step, about the same on decode",
}
ROUTES = ("loop_step", "batch_step", "loop_decode", "batch_decode")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "n": len(ts)}


def images(n_fields, size, dev):
    """B different smooth images with a little noise, [B, S_x, S_y, 3]"""
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for b in range(n_fields):
        base = torch.stack([0.5 + 0.3 * torch.sin((5 + b % 7) * x + 3 * y + b), 0.5 + 0.3 * torch.cos((3 + b % 5) * x * y * 4 - b),
                            0.5 + 0.2 * torch.sin((9 - b % 4) * y - 2 * x + 2 * b)], dim=-1)
        out.append((base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1))
    return torch.stack(out)


def tiles_of_one_image(dev, side=4096, tile=512):
    """the 64 tiles of 512 x 512 of one 4096 x 4096 image, [64, 512, 512, 3]"""
    img = images(1, (side, side), dev)[0]
    k = side // tile
    return img.reshape(k, tile, k, tile, 3).permute(0, 2, 1, 3, 4).reshape(k * k, tile, tile, 3).contiguous()


def row(n_fields, size, log2_table, target, dev, warm=2, reps=10):
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch
    kw = dict(levels=8, features=2, log2_table=log2_table, device=dev)
    batch = HashGridFieldBatch(n_fields, size, seed=0, **kw)
    singles = [HashGridField(size, seed=b, fused=True, **kw) for b in range(n_fields)]
    assert all(f.route == "fused" for f in singles)
    flat = target.reshape(n_fields, -1, 3).contiguous()
    origin = [[0] * len(size)]
    fns = {"loop_step": lambda: [f.train_step(origin, size, flat[b]) for b, f in enumerate(singles)],
           "batch_step": lambda: batch.train_step(origin, size, flat),
           "loop_decode": lambda: [f.decode() for f in singles],
           "batch_decode": lambda: batch.decode()}
    for _ in range(warm):
        for r in ROUTES:
            fns[r]()
    torch.cuda.synchronize()
    ts = {r: [] for r in ROUTES}
    for _ in range(reps):
        for r in ROUTES:
            ts[r].append(timed(fns[r]))
    out = {r: stats(ts[r]) for r in ROUTES}
    for what in ("step", "decode"):
        out[f"batch_{what}"]["ships"] = out[f"batch_{what}"]["median_ms"] < out[f"loop_{what}"]["min_ms"]
        out[f"batch_{what}"]["loop_over_batch_median"] = round(out[f"loop_{what}"]["median_ms"] / out[f"batch_{what}"]["median_ms"], 3)
    # the same parameters through both decodes, at the size timed
    for b, f in enumerate(singles):
        batch.insert(b, f)
    got, ref = batch.decode(), torch.stack([f.decode() for f in singles])
    out["parity"] = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
    out.update({"fields": n_fields, "shape": [*size], "levels": 8, "features": 2, "log2_table": log2_table, "groups_per_field": "automatic"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="all", choices=["small", "tiles", "all"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_batch", "device": torch.cuda.get_device_name(0), "expected": EXPECTED}
    if a.rows in ("small", "all"):
        for n_fields in (1, 8, 64):
            res[f"B{n_fields}_256"] = row(n_fields, (256, 256), 12, images(n_fields, (256, 256), dev), dev)
            torch.cuda.empty_cache()
    if a.rows in ("tiles", "all"):
        res["B64_tiles_512_T15"] = row(64, (512, 512), 15, tiles_of_one_image(dev), dev)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
