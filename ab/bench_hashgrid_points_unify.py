"""The fused training kernels at points whose generated code changed when the level-of-detail unit was folded into the point units (DESIGN 4.7.9:
2D with L F > 32, and 3D): the parent commit's library (ab/libparent.so, its libnicv2_hip.so copied there) against this checkout's, interleaved in
one process, 2 + 10 rounds, 4.2 M points, plain / noisy / lod / lod noisy.  Writes the JSON to the path given as the first argument (default: stdout only); the record is
profiles/hashgrid_points_unify_bench.json.  Rule: the new median inside the parent's min - max of the same run, or below it."""
import ctypes, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_image_compression_v2_amd import _lib, hashgrid as hg

EXPECTED = ("written before the first run: the 44 kernels differ from the parent's in the place of one kernarg load, one sign/zero extension and the "
            "schedule around them, with equal registers, scratch, LDS and occupancy; expected: every median of `new` inside the min-max of `parent` "
            "of the same run, or below it (the rule of DESIGN 4.7.7)")

def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    assert lib.nic_abi_version() == _lib.NIC_ABI_VERSION
    return lib

def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)

def main():
    dev = torch.device("cuda:0")
    libs = {"parent": load(os.path.join(ROOT, "ab", "libparent.so")), "new": load(os.path.join(ROOT, "neural_image_compression_v2_amd", "libnicv2_hip.so"))}
    g = torch.Generator(device=dev).manual_seed(1)
    res = {"bench": "hashgrid_points_unify", "device": torch.cuda.get_device_name(0), "rounds": "2 + 10, interleaved parent / new", "expected": EXPECTED,
           "rule": "new median <= parent max", "cases": {}}
    # every reachable (dim, F, KT) whose generated code changed: 2D with L F > 32, and 3D (F = 1 cannot reach L F > 32 with <= 32 levels)
    cases = {}
    for feats, levels in ((2, 32), (4, 16), (8, 8)):
        cases[f"2d_4k_{levels}x{feats}_kt2"] = ((3840, 2160), levels, feats)
    for feats, levels in ((1, 16), (2, 16), (4, 8), (8, 4)):
        cases[f"3d_256_{levels}x{feats}_kt1"] = ((256, 256, 256), levels, feats)
    for feats, levels in ((2, 32), (4, 16), (8, 8)):
        cases[f"3d_256_{levels}x{feats}_kt2"] = ((256, 256, 256), levels, feats)
    n = 1 << 22
    ok = True
    for cname, (size, levels, feats) in cases.items():
        geo = hg.HashGeometry(tuple(size), tuple(hg.level_resolutions(levels, 16, max(size))), feats, 19)
        table = (torch.rand(geo.table_shape(), generator=g, device=dev) - 0.5) * 0.1
        S = torch.tensor([float(s) for s in size], device=dev)
        target = torch.rand(n, 3, generator=g, device=dev)
        lf = geo.width
        params = [torch.randn(64, lf, generator=g, device=dev) * 0.1, torch.zeros(64, device=dev), torch.randn(64, 64, generator=g, device=dev) * 0.1,
                  torch.zeros(64, device=dev), torch.randn(3, 64, generator=g, device=dev) * 0.1, torch.zeros(3, device=dev)]
        grads = [torch.zeros_like(p) for p in params]
        tg = torch.zeros_like(table)
        lod = torch.rand(n, generator=g, device=dev) * 3
        for pname in (("random", "ordered") if feats == 4 else ("random",)):
            pts = (torch.rand(n, len(size), generator=g, device=dev) * S - 0.5).contiguous()
            order = hg.hash_point_order(geo, pts) if pname == "ordered" else None
            variants = {
                "plain": lambda: hg.hash_fused_forward_backward_points(geo, table, pts, params, target, grads, table_grad=tg, order=order),
                "plain_noisy": lambda: hg.hash_fused_forward_backward_points(geo, table, pts, params, target, grads, table_grad=tg, order=order, quant=(4, 7, 3, 0)),
                "lod": lambda: hg.hash_fused_forward_backward_points_lod(geo, table, pts, params, target, grads, lod=lod, table_grad=tg, order=order),
                "lod_noisy": lambda: hg.hash_fused_forward_backward_points_lod(geo, table, pts, params, target, grads, lod=lod, table_grad=tg, order=order,
                                                                              quant=(4, 7, 3, 0)),
            }
            for vname, fn in variants.items():
                ts = {k: [] for k in libs}
                for rnd in range(12):
                    for k, lib in libs.items():
                        _lib._lib = lib
                        t = timed(fn)
                        if rnd >= 2:
                            ts[k].append(t)
                ent = {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}
                ent["inside"] = ent["new"][0] <= ent["parent"][2]
                ok = ok and ent["inside"]
                res["cases"][f"{cname}/{pname}/{vname}"] = ent
                print(cname, pname, vname, ent, flush=True)
        del table, tg, target, lod
        torch.cuda.empty_cache()
    res["all_inside"] = ok
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(json.dumps(res) + "\n")
    print("all_inside", ok)

if __name__ == "__main__":
    main()
