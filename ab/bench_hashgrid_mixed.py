"""A bit depth per level: timings against the uniform packed routes of the same build and rate-distortion rows for a few allocations
(hashgrid.py HashGridField(num_bits=[..]), csrc/hash_mixed.hip); prints one JSON line:

    python ab/bench_hashgrid_mixed.py [--out FILE] [--no-rd]

The method of ab/bench_hashgrid_packed.py: one process, HIP events around each call, warm-up first, the variants interleaved call by call
(A B A B ..), medians with min - max.  At 3840 x 2160, L 16, F 2, T 2^19:
- ``encode``: nic_hash_encode_bits at b = 4 against nic_hash_encode_levels from a format /2 table with all depths 4, one launch, 20 rounds;
- ``fused_decode``: ``load_compressed(file, fused=True).decode()`` of the /1 file against the /2 file, 10 rounds;
- ``train_step``: the whole step on a 2048 x 1024 crop, both routes: uniform b = 4, the list [4] * 16 (no clamp launch) and 8 bits on the dense
  levels with 4 on the hashed ones (with the clamp launch), 10 rounds.
``rate_distortion``: the 256 x 256 fits of bench_hashgrid_codec.py for a few allocations next to uniform 8 and 4; the PSNR is that of the
decode of the saved file.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ab.bench_hashgrid_codec import _image, psnr      # noqa: E402
from ab.bench_hashgrid_packed import interleaved      # noqa: E402


def timings(dev):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridField, hash_encode_bits, hash_encode_levels, hash_pack_bits, hash_pack_bits_levels
    size, b = (3840, 2160), 4
    field = HashGridField(size, device=dev, seed=0, num_bits=b)
    geo = field.geo
    same = [b] * geo.levels
    lo, hi = models._q_range(b)
    with torch.no_grad():
        field.table.copy_(torch.rand(geo.table_shape(), device=dev) * (hi - lo) + lo)
    table = field.table.detach()
    p1, p2 = hash_pack_bits(geo, table, b), hash_pack_bits_levels(geo, table, same)
    org = geo.upload_origins([[0, 0]], size, dev)
    rows_equal = bool(torch.equal(hash_encode_bits(geo, p1, org, size, b), hash_encode_levels(geo, p2, same, coord=org, extent=size, kind="bits")))
    enc = interleaved({"bits1": lambda: hash_encode_bits(geo, p1, org, size, b),
                       "bits2": lambda: hash_encode_levels(geo, p2, same, coord=org, extent=size, kind="bits")}, 3, 20)
    field.freeze()
    mixed = HashGridField(size, device=dev, seed=0, num_bits=same)
    with torch.no_grad():
        mixed.table.copy_(field.table)
    mixed.freeze()
    with tempfile.TemporaryDirectory() as d:
        pa, pb = os.path.join(d, "v1.pt"), os.path.join(d, "v2.pt")
        field.save_compressed(pa, packed=True)
        mixed.save_compressed(pb, packed=True)
        fa, fb = HashGridField.load_compressed(pa, dev, fused=True), HashGridField.load_compressed(pb, dev, fused=True)
    assert fa.route == fb.route == "fused"
    images_equal = bool(torch.equal(fa.decode(), fb.decode()))
    dec = interleaved({"bits1": lambda: fa.decode(), "bits2": lambda: fb.decode()}, 2, 10)
    del field, mixed, fa, fb, p1, p2
    torch.cuda.empty_cache()
    crop = (2048, 1024)
    target = torch.rand(crop[0] * crop[1], 3, device=dev)
    dense = [8 if (r + 1) ** 2 <= geo.table_size else 4 for r in geo.resolutions]
    steps = {}
    for fused in (False, True):
        fields = {"uniform4": HashGridField(size, device=dev, seed=0, num_bits=b, fused=fused),
                  "list4": HashGridField(size, device=dev, seed=0, num_bits=same, fused=fused),
                  "dense8_hashed4": HashGridField(size, device=dev, seed=0, num_bits=dense, fused=fused)}
        fns = {k: (lambda f=f: f.train_step([[512, 256]], crop, target)) for k, f in fields.items()}
        steps["fused" if fused else "layerwise"] = interleaved(fns, 2, 10)
        del fields, fns
        torch.cuda.empty_cache()
    return {"num_bits": b, "rows_equal": rows_equal, "images_equal": images_equal, "encode_ms": enc,
            "encode_bits2_over_bits1": round(enc["bits2"][0] / enc["bits1"][0], 3), "fused_decode_ms": dec,
            "fused_decode_bits2_over_bits1": round(dec["bits2"][0] / dec["bits1"][0], 3), "train_step_crop": list(crop), "train_step_ms": steps,
            "train_step_dense8_hashed4_bits": dense}


def rate_distortion(dev, epochs=300):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (256, 256)
    image = _image(size, dev)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for lg in (12, 16):
            probe = HashGridField(size, num_bits=4, levels=8, features=2, log2_table=lg, device=dev, seed=1)
            entries = [min((r + 1) ** 2, 1 << lg) for r in probe.resolutions]
            med = statistics.median(entries)
            allocs = {"uniform8": 8, "uniform4": 4, "8_below_median_4_rest": [8 if e < med else 4 for e in entries],
                      "8_dense_4_hashed": [8 if (r + 1) ** 2 <= (1 << lg) else 4 for r in probe.resolutions],
                      "graded_8_to_3": [8, 8, 7, 6, 5, 4, 3, 3], "8_below_median_2_rest": [8 if e < med else 2 for e in entries]}
            for name, bits in allocs.items():
                q = HashGridField(size, num_bits=bits, levels=8, features=2, log2_table=lg, device=dev, seed=1)
                q.set_schedule(epochs)
                q.fit(image, epochs)
                p = os.path.join(d, f"{lg}_{name}.pt")
                q.save_compressed(p, packed=True)
                y = HashGridField.load_compressed(p, dev).decode()
                rows.append({"log2_table": lg, "allocation": name, "bits": bits, "entries": entries, "packed_table_bytes": q.stored_bytes(packed=True)["table"],
                             "decoder_bytes": q.stored_bytes(packed=True)["decoder"], "packed_file_bytes": os.path.getsize(p), "psnr_db": psnr(y, image)})
    return {"image": [*size, 3], "levels": 8, "features": 2, "epochs": epochs, "freeze_at": 0.95, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-rd", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_mixed", "device": torch.cuda.get_device_name(0), "shape": [3840, 2160], "levels": 16, "features": 2, "log2_table": 19,
           "timings": timings(dev)}
    if not a.no_rd:
        res["rate_distortion"] = rate_distortion(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
