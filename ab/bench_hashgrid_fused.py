"""The fused hash-grid step against the layer-wise one (hashgrid.py, csrc/hash_fused.hip); prints one JSON line:

    python ab/bench_hashgrid_fused.py [--out profiles/hashgrid_fused_bench.json] [--shape 4k|256cube|both]

Per shape (4K: 3840 x 2160; 256^3; L 16, F 2, T 2^19; one crop = the whole field), in ONE process:
- ``step``: the whole ``HashGridField.train_step`` with ``fused=False`` and ``fused=True``, interleaved call by call (A B A B ..), HIP events
  around each call, 3 warm-up and 12 timed steps per side: median, minimum, maximum;
- ``fused_kernel_ms``: the fused kernel alone inside those steps (``nic_mark_kernel_end``: start of the call to the event recorded between
  the kernel and the reduction launch), median;
- ``decode``: ``decode()`` both ways from the fp32 table, and from the stored uint8 table (a field that was frozen, saved and loaded).
"""
import argparse
import ctypes
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


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "n": len(ts)}


def interleaved(fa, fb, warm=3, reps=12):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa))
        tb.append(timed(fb))
    return ta, tb


def kernel_alone(step, reps=10):
    """start of the call -> the event the training entry point records after its fused kernel"""
    from neural_image_compression_v2_amd import _lib
    lib, hip = _lib.load(), ctypes.CDLL("libamdhip64.so")
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    ts = []
    try:
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(reps):
            torch.cuda.synchronize()
            assert hip.hipEventRecord(ev[0], stream) == 0
            lib.nic_mark_kernel_end(ev[1])
            step()
            torch.cuda.synchronize()
            ms = ctypes.c_float()
            if hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0:
                ts.append(ms.value)
    finally:
        lib.nic_mark_kernel_end(None)
        for e in ev:
            hip.hipEventDestroy(e)
    return ts


def shape_leg(dev, size, stored_decode):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    n = 1
    for s in size:
        n *= s
    target = torch.rand(n, 3, device=dev)
    origin = [[0] * len(size)]
    fields = {r: HashGridField(size, device=dev, seed=0, fused=(r == "fused")) for r in ("layerwise", "fused")}
    assert fields["fused"].route == "fused" and fields["layerwise"].route == "layerwise"
    steps = {r: (lambda f=f: f.train_step(origin, size, target)) for r, f in fields.items()}
    ta, tb = interleaved(steps["layerwise"], steps["fused"])
    res = {"shape": [*size], "levels": 16, "features": 2, "log2_table": 19,
           "step": {"layerwise": stats(ta), "fused": stats(tb)},
           "speedup": round(statistics.median(ta) / statistics.median(tb), 3),
           "fused_mpix_per_s": round(n / statistics.median(tb) / 1e3, 1), "layerwise_mpix_per_s": round(n / statistics.median(ta) / 1e3, 1)}
    ks = kernel_alone(steps["fused"])
    res["fused_kernel_ms"] = stats(ks) if ks else None
    da, db = interleaved(fields["layerwise"].decode, fields["fused"].decode, warm=2, reps=10)
    res["decode_fp32_table"] = {"layerwise": stats(da), "fused": stats(db)}
    if stored_decode:
        with tempfile.TemporaryDirectory() as tmp:
            q = HashGridField(size, device=dev, seed=0, num_bits=8)
            q.freeze()
            path = os.path.join(tmp, "f.pt")
            q.save_compressed(path)
            del q
            la, lb = HashGridField.load_compressed(path, dev), HashGridField.load_compressed(path, dev, fused=True)
        da, db = interleaved(la.decode, lb.decode, warm=2, reps=10)
        res["decode_stored_u8"] = {"layerwise": stats(da), "fused": stats(db)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="both", choices=["4k", "256cube", "both"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "hashgrid_fused", "device": torch.cuda.get_device_name(0)}
    if a.shape in ("4k", "both"):
        res["4k"] = shape_leg(dev, (3840, 2160), True)
        torch.cuda.empty_cache()
    if a.shape in ("256cube", "both"):
        res["256cube"] = shape_leg(dev, (256, 256, 256), False)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
