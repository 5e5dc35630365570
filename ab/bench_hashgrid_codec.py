"""Hash-grid codec timings and rate-distortion (hashgrid.py num_bits, csrc/hash_grid.hip); prints one JSON line:

    python ab/bench_hashgrid_codec.py [--out FILE]

At 3840 x 2160, L 16, F 2, T 2^19 (11 dense and 5 hashed levels), b = 8; HIP events around each call, warm-up first, then the variants
interleaved call by call with the plain fp32 encode (A B C A B C ..) on one device, medians:
- ``encode``: nic_hash_encode / nic_hash_encode_noisy / nic_hash_encode_u8 (the compact table), 30 rounds;
- ``decode``: ``decode()`` of the fp32 field against ``load_compressed(file).decode()`` (uint8 table), 10 rounds;
- ``step``: ``train_step`` of a num_bits=None field against a num_bits=8 one (noise on), one crop = the whole field, 10 rounds.
``rate_distortion``: a 256 x 256 synthetic image (no random term), 8 levels x 2 features, 300 whole-image passes (noise, then freeze at 0.95 N); stored bytes
(table + fp32 decoder) and the PSNR of the stored decode for b in {8, 4} and log2_table in {12, 16}, beside the unquantised fit.
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, warm, reps):
    """{name: median ms}: every round runs each variant once, in order"""
    for _ in range(warm):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(timed(f))
    return {k: round(statistics.median(v), 4) for k, v in ts.items()}


def encode_times(dev, num_bits=8):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, hash_encode, hash_encode_noisy, hash_encode_u8, hash_pack_u8, level_resolutions
    size = (3840, 2160)
    geo = HashGeometry(size, tuple(level_resolutions(16, 16, max(size))), 2, 19)
    lo, hi = models._q_range(num_bits)
    table = torch.rand(geo.table_shape(), device=dev) * (hi - lo) + lo
    packed = hash_pack_u8(geo, table, num_bits)
    org = geo.upload_origins([[0, 0]], size, dev)
    step = [0]

    def noisy():
        step[0] += 1
        hash_encode_noisy(geo, table, org, size, num_bits, 7, step[0], 0)

    ms = interleaved({"plain": lambda: hash_encode(geo, table, org, size), "noisy": noisy,
                      "u8": lambda: hash_encode_u8(geo, packed, org, size, num_bits)}, 5, 30)
    pack = interleaved({"pack": lambda: hash_pack_u8(geo, table, num_bits)}, 3, 10)["pack"]
    return {"shape": [*size], "levels": 16, "features": 2, "log2_table": 19, "num_bits": num_bits, "plain_ms": ms["plain"], "noisy_ms": ms["noisy"],
            "u8_ms": ms["u8"], "noisy_over_plain": round(ms["noisy"] / ms["plain"], 3), "u8_over_plain": round(ms["u8"] / ms["plain"], 3),
            "pack_ms": pack, "stored_table_bytes": int(packed.numel()), "fp32_table_bytes": table.numel() * 4}


def decode_and_step_times(dev, num_bits=8):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (3840, 2160)
    n = size[0] * size[1]
    target = torch.rand(n, 3, device=dev)
    plain = HashGridField(size, device=dev, seed=0)
    qat = HashGridField(size, device=dev, seed=0, num_bits=num_bits)
    step = interleaved({"plain": lambda: plain.train_step([[0, 0]], size, target), "qat": lambda: qat.train_step([[0, 0]], size, target)}, 3, 10)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "field.pt")
        qat.freeze()
        qat.save_compressed(path)
        loaded = HashGridField.load_compressed(path, dev)
        dec = interleaved({"fp32": lambda: qat.decode(), "stored": lambda: loaded.decode()}, 2, 10)
        file_bytes = os.path.getsize(path)
        same = bool(torch.equal(qat.decode(), loaded.decode()))
    return ({"shape": [*size], "plain_step_ms": step["plain"], "qat_step_ms": step["qat"], "qat_over_plain": round(step["qat"] / step["plain"], 3)},
            {"shape": [*size], "fp32_decode_ms": dec["fp32"], "stored_decode_ms": dec["stored"], "file_bytes": file_bytes,
             "stored_bytes": loaded.stored_bytes(), "stored_decode_equals_frozen": same})


def _image(size, dev):
    """the structured image of tests/test_gpu_hashgrid_codec.py: smooth ramps, finer texture, soft edges, no random term"""
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.25 * torch.sin(7 * x + 3 * y) + 0.15 * torch.sin(41 * x) * torch.cos(37 * y),
                        0.5 + 0.25 * torch.cos(20 * x * y) + 0.15 * torch.sin(60 * (x - y) ** 2),
                        0.5 + 0.2 * torch.sin(13 * y - 2 * x) + 0.1 * torch.sign(torch.sin(9 * x + 11 * y))], dim=-1)
    return base.clamp(0, 1)


def psnr(a, b):
    return round(float(10 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean())), 3)


def rate_distortion(dev, epochs=300):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (256, 256)
    image = _image(size, dev)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for lg in (12, 16):
            kw = dict(levels=8, features=2, log2_table=lg, device=dev, seed=1)
            fp = HashGridField(size, **kw)
            fp.set_schedule(epochs)
            fp.fit(image, epochs)
            rows.append({"log2_table": lg, "num_bits": None, "table_bytes": fp.table.numel() * 4, "decoder_bytes": fp.stored_bytes()["decoder"],
                         "psnr_db": psnr(fp.decode(), image)})
            for b in (8, 4):
                q = HashGridField(size, num_bits=b, **kw)
                q.set_schedule(epochs)
                q.fit(image, epochs)
                path = os.path.join(d, f"q{lg}_{b}.pt")
                q.save_compressed(path)
                sb = q.stored_bytes()
                rows.append({"log2_table": lg, "num_bits": b, "table_bytes": sb["table"], "decoder_bytes": sb["decoder"], "file_bytes": os.path.getsize(path),
                             "psnr_db": psnr(HashGridField.load_compressed(path, dev).decode(), image)})
    return {"image": [*size, 3], "levels": 8, "features": 2, "epochs": epochs, "freeze_at": 0.95, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_codec", "device": torch.cuda.get_device_name(0), "encode": encode_times(dev)}
    torch.cuda.empty_cache()
    res["step"], res["decode"] = decode_and_step_times(dev)
    torch.cuda.empty_cache()
    res["rate_distortion"] = rate_distortion(dev)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
