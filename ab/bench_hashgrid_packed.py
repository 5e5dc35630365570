"""Bit-packed hash-grid table: timings against the uint8 route and the rate-distortion rows (hashgrid.py save_compressed(packed=True),
csrc/hash_grid.hip / hash_fused.hip); prints one JSON line:

    python ab/bench_hashgrid_packed.py [--out FILE] [--no-rd]

The method of ab/bench_hashgrid_codec.py: one process, HIP events around each call, warm-up first, the variants interleaved call by call
(A B A B ..), medians with min - max.  At 3840 x 2160, L 16, F 2, T 2^19 (11 dense and 5 hashed levels), for b in {8, 4, 3} (F b = 16, 8: one
dword per entry; 6: an entry may straddle two):
- ``encode``: nic_hash_encode_u8 against nic_hash_encode_bits, the whole field in one launch, 20 rounds;
- ``fused_decode``: ``load_compressed(file, fused=True).decode()`` of the uint8 file against the packed file, 10 rounds;
- ``pack``: nic_hash_pack_u8, nic_hash_pack_bits and nic_hash_unpack_bits, 10 rounds.
``rate_distortion``: the 256 x 256 fits of bench_hashgrid_codec.py with a packed-bytes column and a b = 2 row; the PSNR is that of the decode of
the packed file.
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

from ab.bench_hashgrid_codec import _image, psnr, timed      # noqa: E402


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


def timings(dev, num_bits):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import (HashGridField, hash_encode_bits, hash_encode_u8, hash_pack_bits, hash_pack_u8,
                                                          hash_unpack_bits)
    size = (3840, 2160)
    field = HashGridField(size, device=dev, seed=0, num_bits=num_bits)
    geo = field.geo
    lo, hi = models._q_range(num_bits)
    with torch.no_grad():
        field.table.copy_(torch.rand(geo.table_shape(), device=dev) * (hi - lo) + lo)
    table = field.table.detach()
    u8, bits = hash_pack_u8(geo, table, num_bits), hash_pack_bits(geo, table, num_bits)
    org = geo.upload_origins([[0, 0]], size, dev)
    same_rows = bool(torch.equal(hash_encode_u8(geo, u8, org, size, num_bits), hash_encode_bits(geo, bits, org, size, num_bits)))
    enc = interleaved({"u8": lambda: hash_encode_u8(geo, u8, org, size, num_bits), "bits": lambda: hash_encode_bits(geo, bits, org, size, num_bits)}, 3, 20)
    pk = interleaved({"pack_u8": lambda: hash_pack_u8(geo, table, num_bits), "pack_bits": lambda: hash_pack_bits(geo, table, num_bits),
                      "unpack_bits": lambda: hash_unpack_bits(geo, bits, num_bits)}, 3, 10)
    field.freeze()
    with tempfile.TemporaryDirectory() as d:
        pa, pb = os.path.join(d, "u8.pt"), os.path.join(d, "bits.pt")
        field.save_compressed(pa)
        field.save_compressed(pb, packed=True)
        fa, fb = HashGridField.load_compressed(pa, dev, fused=True), HashGridField.load_compressed(pb, dev, fused=True)
        files = {"u8": os.path.getsize(pa), "bits": os.path.getsize(pb)}
    assert fa.route == fb.route == "fused"
    same_image = bool(torch.equal(fa.decode(), fb.decode()))
    dec = interleaved({"u8": lambda: fa.decode(), "bits": lambda: fb.decode()}, 2, 10)
    return {"num_bits": num_bits, "table_bytes": {"u8": int(u8.numel()), "bits": int(bits.numel())}, "file_bytes": files,
            "encode_ms": enc, "encode_bits_over_u8": round(enc["bits"][0] / enc["u8"][0], 3), "rows_equal": same_rows,
            "fused_decode_ms": dec, "fused_decode_bits_over_u8": round(dec["bits"][0] / dec["u8"][0], 3), "images_equal": same_image,
            "pack_ms": pk}


def rate_distortion(dev, epochs=300):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (256, 256)
    image = _image(size, dev)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for lg in (12, 16):
            for b in (8, 4, 2):
                q = HashGridField(size, num_bits=b, levels=8, features=2, log2_table=lg, device=dev, seed=1)
                q.set_schedule(epochs)
                q.fit(image, epochs)
                pa, pb = os.path.join(d, f"u{lg}_{b}.pt"), os.path.join(d, f"p{lg}_{b}.pt")
                q.save_compressed(pa)
                q.save_compressed(pb, packed=True)
                ya, yb = HashGridField.load_compressed(pa, dev).decode(), HashGridField.load_compressed(pb, dev).decode()
                rows.append({"log2_table": lg, "num_bits": b, "table_bytes": q.stored_bytes()["table"], "packed_table_bytes": q.stored_bytes(packed=True)["table"],
                             "decoder_bytes": q.stored_bytes()["decoder"], "packed_file_bytes": os.path.getsize(pb), "psnr_db": psnr(yb, image),
                             "packed_decode_equals_u8_decode": bool(torch.equal(ya, yb))})
    return {"image": [*size, 3], "levels": 8, "features": 2, "epochs": epochs, "freeze_at": 0.95, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-rd", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_packed", "device": torch.cuda.get_device_name(0), "shape": [3840, 2160], "levels": 16, "features": 2, "log2_table": 19,
           "timings": []}
    for b in (8, 4, 3):
        res["timings"].append(timings(dev, b))
        torch.cuda.empty_cache()
    if not a.no_rd:
        res["rate_distortion"] = rate_distortion(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
