"""Return-code sweep of the point-gradient and point-step entry points against the parent commit's library, and with --batch of
the batched entries at points: both libraries in one process through ctypes, the same seeded random arguments to each, every
return value compared.  Nothing launches: n_points is <= 0, or >= 2^31 where the entry refuses that (the single field's step: together with an
order), and every device pointer is a made-up address that no host path reads.  No GPU is needed.

    python ab/points_rc_sweep.py PARENT_LIB [NEW_LIB] [--seed 20261021] [--calls 20000] [--out profiles/hashgrid_walk_unify_retcodes.json]
    python ab/points_rc_sweep.py PARENT_LIB [NEW_LIB] --batch [--out profiles/hashgrid_batch_unify_retcodes.json]

Exit status 1 on a return value that differs, or on a code an entry can return that the sweep did not reach."""
import argparse, ctypes, json, os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_image_compression_v2_amd import _lib as L

OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5
NAMES = {OK: "NIC_OK", NULL: "NIC_E_NULL", UNSUP: "NIC_E_UNSUPPORTED", SHAPE: "NIC_E_SHAPE", WORKSPACE: "NIC_E_WORKSPACE", ARG: "NIC_E_ARG"}
STEP = ["nic_hash_fused_forward_backward_points", "nic_hash_fused_forward_backward_points_lod", "nic_hash_fused_forward_backward_points_grad",
        "nic_hash_fused_forward_backward_points_grad_lod"]
GRAD = ["nic_hash_encode_points_grad", "nic_hash_fused_points_grad", "nic_hash_encode_points_grad_lod", "nic_hash_fused_points_grad_lod"]
NOISY, BYTES = "nic_hash_encode_points_grad_lod_noisy", "nic_hash_fused_points_workspace_bytes"
# the codes each entry can return: the layer-wise entries take no workspace; the workspace size answers 0 or a size
CAN = {**{e: {OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG} for e in STEP}, **{e: {OK, NULL, UNSUP, SHAPE, ARG} for e in GRAD + [NOISY]}}
# the batched entries at points (hashgrid_batch.hip, hashgrid_batch_grad.hip): the four steps, the two gradient-only entries, the two decodes
B_STEP = ["nic_hash_batch_forward_backward_points", "nic_hash_batch_forward_backward_points_lod", "nic_hash_batch_forward_backward_points_grad",
          "nic_hash_batch_forward_backward_points_grad_lod"]
B_GRAD = ["nic_hash_batch_points_grad", "nic_hash_batch_points_grad_lod"]
B_FWD = ["nic_hash_batch_forward_source", "nic_hash_batch_forward_points_lod"]
B_BYTES = "nic_hash_batch_points_workspace_bytes"
CAN.update({**{e: {OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG} for e in B_STEP}, **{e: {OK, NULL, UNSUP, SHAPE, ARG} for e in B_GRAD + B_FWD}})


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in {**L.SIGNATURES, **L.EXT_SIGNATURES}.items():
        fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    assert lib.nic_abi_version() == L.NIC_ABI_VERSION
    return lib


class Gen:
    """one call's arguments; `keep` holds the ctypes objects alive until both libraries have answered"""
    def __init__(self, rng):
        self.r, self.keep = rng, []

    def good(self, p=0.88):
        return self.r.random() < p

    def ptr(self, p=0.9):                                  # a device pointer nothing reads, or null
        return 16 * self.r.randint(1, 1 << 20) if self.good(p) else None

    def ref(self, obj):
        self.keep.append(obj)
        return ctypes.byref(obj)

    def desc(self):
        if not self.good(0.95):
            return None
        r, d = self.r, L.NicHashDesc()
        p = 0.997 if r.random() < 0.7 else 0.85              # most descriptors pass, so that the later checks are reached
        d.dim = r.choice((2, 3)) if self.good(p) else r.choice((1, 4))
        d.levels = r.randint(1, 16) if self.good(p) else r.choice((0, 33, 24))
        d.features = r.choice((1, 2, 4, 8)) if self.good(p) else r.choice((3, 16))
        d.log2_table = r.randint(10, 22) if self.good(p) else r.choice((9, 3, 30))
        d.S_max = r.choice((16, 64, 256, 4096)) if self.good(p) else r.choice((0, 1 << 22, 1 << 23))
        d.num_crops = 1 if self.good(p) else r.choice((0, 2))
        for a in range(3):
            d.extent[a] = 1 if a >= d.dim else (r.randint(1, max(1, d.S_max)) if self.good(p) else r.choice((0, d.S_max + 1)))
        for l in range(32):
            d.resolution[l] = r.randint(1, max(1, d.S_max)) if self.good(0.9 + p / 10) else r.choice((0, d.S_max + 1))
        d.flags = 0 if self.good(p) else 1
        d.reserved = 0 if self.good(p) else 1
        return self.ref(d)

    def lod(self, p=0.9):
        if not self.good(p):
            return None
        r, s = self.r, L.NicHashLod()
        for l in range(32):
            s.fade[l] = r.uniform(0, 8) if self.good(0.985) else r.choice((-1.0, float("nan"), float("inf")))
        s.lod_uniform = r.uniform(-2, 4) if self.good(0.95) else float("nan")
        s.reserved = 0 if self.good(0.95) else 1
        return self.ref(s)

    def quant(self):
        if not self.good(0.6):
            return None
        r, q = self.r, L.NicHashQuant()
        q.num_bits = r.randint(1, 8) if self.good() else r.choice((0, 9))
        q.noise_mode = r.choice((0, 2)) if self.good() else r.choice((1, 3))
        q.noise_seed, q.noise_offset = r.getrandbits(64), r.getrandbits(64)
        q.sample_base = r.randint(0, 1 << 40) if self.good(0.93) else -1
        return self.ref(q)

    def source(self):
        if not self.good(0.95):
            return None
        r, s = self.r, L.NicHashSource()
        s.kind = r.choice((0, 1, 2)) if self.good(0.93) else r.choice((3, -1))
        s.num_bits = (0 if s.kind == 0 else r.randint(1, 8)) if self.good() else r.choice((0, 9, 4))
        s.data = (16 * r.randint(1, 1 << 20) + (0 if self.good() else 2)) if self.good(0.95) else None
        return self.ref(s)

    def mlp(self):
        if not self.good(0.95):
            return None
        m = L.NicMlp()
        for i in range(3):
            m.w[i], m.b[i] = self.ptr(0.97), self.ptr(0.97)
        m.n_linear = 3 if self.good(0.93) else self.r.choice((2, 5))
        return self.ref(m)

    def grads(self):
        if not self.good(0.95):
            return None, None
        g = L.NicMlpGrads()
        for i in range(3):
            g.w[i], g.b[i] = 4096 * (2 * i + 1), 4096 * (2 * i + 2)
        return self.ref(g), g

    def tail(self, g):
        if not self.good(0.5):
            return None
        r, t = self.r, L.NicStepTail()
        t.count = r.randint(1, 6) if self.good() else r.choice((0, 33))
        t.n_stream = r.randint(0, max(0, min(t.count, 6))) if self.good() else r.choice((-1, t.count + 1))
        arr = (L.NicAdamTensor * 40)()
        pool = [4096 * k for k in range(1, 7)]
        for i in range(40):
            a = arr[i]
            a.param, a.exp_avg, a.exp_avg_sq = 16 * (i + 1), 16 * (i + 50), 16 * (i + 100)
            a.grad = (r.choice(pool) if (g is not None and self.good(0.93)) else r.choice((None, 8192 * 100))) if i >= t.n_stream else 16 * (i + 200)
            a.n, a.step, a.lr = r.randint(1, 4096) if self.good(0.95) else 0, r.randint(1, 100), 1e-3
            a.clamp_lo, a.clamp_hi = -1.0, 1.0
            a.reps = r.choice((0, 1))
        self.keep.append(arr)
        t.tensors = ctypes.cast(arr, ctypes.c_void_p).value if self.good(0.95) else None
        t.beta1, t.beta2, t.eps = 0.9, 0.999, 1e-8
        t.sched = None if self.good(0.95) else 64
        return self.ref(t)

    def n_order(self):                                      # (n_points, order) of a step entry: nothing may launch
        r = self.r
        k = r.random()
        if k < 0.55:
            return 0, self.ptr(0.5)
        if k < 0.75:
            return r.choice((-1, -(1 << 40))), self.ptr(0.5)
        return r.choice((1 << 31, (1 << 31) + 7, 1 << 40)), 16 * r.randint(1, 99)

    def n_grad(self):                                       # n_points of an entry without an order
        return 0 if self.good(0.7) else self.r.choice((-1, -(1 << 33)))

    def fields(self):                                       # (n_fields, groups_per_field) of a batched entry
        r = self.r
        b = r.choice((1, 2, 3, 8, 64, 65535)) if self.good(0.95) else r.choice((0, -1, 65536))
        # at no points G is taken on one wave item: 0 and 8 pass there, 16 and 64 only beside an n_points that is refused later
        return b, (r.choice((0, 0, 8, 16, 64)) if self.good(0.9) else r.choice((-8, 4, 12, 1 << 20)))

    def n_batch(self, high):                                # n_points of a batched entry; `high`: the entry refuses 2^31 and more before it launches
        k = self.r.random()
        if k < 0.6:
            return 0
        if k < 0.8 or not high:
            return self.r.choice((-1, -(1 << 40)))
        return self.r.choice((1 << 31, (1 << 31) + 7, 1 << 40))


def make_call(name, rng):
    """(the generator that keeps the ctypes objects alive, the arguments) of one random call of entry `name`"""
    g = Gen(rng)
    if name == BYTES:
        return g, (g.desc(), g.mlp())
    if name == B_BYTES:
        d, (b, grp) = g.desc(), g.fields()
        return g, (d, b, grp, rng.choice((0, 1, 64, 1000, 1 << 20, (1 << 31) - 1)) if g.good() else rng.choice((-1, 1 << 31, 1 << 40)), g.mlp())
    if name in B_STEP:
        d, (b, grp), q, m = g.desc(), g.fields(), g.quant(), g.mlp()
        n, (gp, gs) = g.n_batch(True), g.grads()
        flags = rng.choice((0, 1, 2, 3)) if g.good(0.93) else rng.choice((4, 8, -1))
        wbytes = rng.choice((1 << 40, 1 << 34)) if g.good(0.85) else rng.choice((0, 64, 4096))
        table, points, lod, counts, order, target = g.ptr(0.97), g.ptr(0.97), g.ptr(0.5), g.ptr(0.5), g.ptr(0.5), g.ptr(0.97)
        tg, loss, y, dp, dl, wsp = g.ptr(0.6), g.ptr(0.97), g.ptr(0.5), g.ptr(0.96), g.ptr(0.96), g.ptr(0.97)
        if name == B_STEP[0]:
            return g, (d, b, grp, q, table, points, n, counts, order, m, target, 1.0, tg, gp, loss, y, flags, wsp, wbytes, None)
        lp = g.lod(0.6 if name == B_STEP[2] else 0.95)
        head = (d, b, grp, lp, q, table, points, lod, n, counts, order, m, target, 1.0, tg, gp, loss, y)
        return g, head + {B_STEP[1]: (), B_STEP[2]: (dp,), B_STEP[3]: (dp, dl)}[name] + (flags, wsp, wbytes, None)
    if name in B_GRAD:
        d, (b, grp) = g.desc(), g.fields()
        lp, src = g.lod(0.6 if name == B_GRAD[0] else 0.95), g.source()
        points, lod, n, counts, order, m = g.ptr(0.96), g.ptr(0.5), g.n_batch(True), g.ptr(0.5), g.ptr(0.5), g.mlp()
        k = rng.random()
        dy, target = (g.ptr(1), None) if k < 0.45 else ((None, g.ptr(1)) if k < 0.9 else rng.choice(((None, None), (16, 32))))
        tail = (g.ptr(0.96),) if name == B_GRAD[0] else (g.ptr(0.96), g.ptr(0.96))
        return g, (d, b, grp, lp, src, points, lod, n, counts, order, m, dy, target, 1.0, g.ptr(0.5)) + tail + (None,)
    if name in B_FWD:                                       # at points alone: a lattice launches, and so does a count of 2^31 points
        d, (b, grp), src, n, m = g.desc(), g.fields(), g.source(), g.n_batch(False), g.mlp()
        if name == B_FWD[0]:
            origins, points = (None, g.ptr(1)) if g.good(0.92) else rng.choice(((None, None), (16, 32)))
            return g, (d, b, grp, src, origins, points, n, m, g.ptr(0.96), None)
        return g, (d, b, grp, g.lod(0.95), src, g.ptr(0.96), g.ptr(0.5), n, m, g.ptr(0.96), None)
    if name in STEP:
        d, q, m = g.desc(), g.quant(), g.mlp()
        n, order = g.n_order()
        gp, gs = g.grads()
        tail = g.tail(gs)
        flags = rng.choice((0, 1, 2, 3)) if g.good(0.93) else rng.choice((4, 8, -1))
        wbytes = rng.choice((1 << 30, 1 << 26)) if g.good(0.85) else rng.choice((0, 64, 4096))
        table, points, lod, target, tg, loss, y, dp, dl, wsp = g.ptr(0.97), g.ptr(0.97), g.ptr(0.5), g.ptr(0.97), g.ptr(0.6), g.ptr(0.97), g.ptr(0.5), g.ptr(0.96), g.ptr(0.96), g.ptr(0.97)
        if name == STEP[0]:
            return g, (d, q, table, points, n, order, m, target, 1.0, tg, gp, loss, y, flags, wsp, wbytes, tail, None)
        if name == STEP[1]:
            return g, (d, g.lod(0.95), q, table, points, lod, n, order, m, target, 1.0, tg, gp, loss, y, flags, wsp, wbytes, tail, None)
        if name == STEP[2]:
            return g, (d, g.lod(0.6), q, table, points, lod, n, order, m, target, 1.0, tg, gp, loss, y, dp, flags, wsp, wbytes, tail, None)
        return g, (d, g.lod(0.95), q, table, points, lod, n, order, m, target, 1.0, tg, gp, loss, y, dp, dl, flags, wsp, wbytes, tail, None)
    d = g.desc()
    points, lod, dx, dp, dl, n = g.ptr(0.96), g.ptr(0.5), g.ptr(0.96), g.ptr(0.96), g.ptr(0.96), g.n_grad()
    if name == NOISY:
        return g, (d, g.lod(0.95), g.quant(), g.ptr(0.96), points, lod, n, dx, dp, dl, None)
    lp = g.lod(0.6 if name in GRAD[:2] else 0.95)
    src = g.source()
    if name == GRAD[0]:
        return g, (d, lp, src, points, lod, n, dx, dp, None)
    if name == GRAD[2]:
        return g, (d, lp, src, points, lod, n, dx, dp, dl, None)
    k = rng.random()
    dy, target = (g.ptr(1), None) if k < 0.45 else ((None, g.ptr(1)) if k < 0.9 else rng.choice(((None, None), (16, 32))))
    if name == GRAD[1]:
        return g, (d, lp, src, points, lod, n, g.mlp(), dy, target, 1.0, g.ptr(0.5), dp, None)
    return g, (d, lp, src, points, lod, n, g.mlp(), dy, target, 1.0, g.ptr(0.5), dp, dl, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new", nargs="?", default=L.LIB_PATH)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--calls", type=int, default=20000, help="per entry point")
    ap.add_argument("--out")
    ap.add_argument("--batch", action="store_true", help="the batched entries at points instead of the single field's")
    a = ap.parse_args()
    parent, new = load(a.parent), load(a.new)
    entries, sizes = (B_STEP + B_GRAD + B_FWD + [B_BYTES], B_BYTES) if a.batch else (STEP + GRAD + [NOISY, BYTES], BYTES)
    res = {"sweep": "hashgrid_batch_unify_retcodes" if a.batch else "hashgrid_walk_unify_retcodes", "seed": a.seed, "calls_per_entry": a.calls, "entries": {}, "differences": 0, "unreached": []}
    for name in entries:
        rng = random.Random(f"{a.seed}/{name}")
        hist = {}
        for _ in range(a.calls):
            g, args = make_call(name, rng)
            rp, rn = getattr(parent, name)(*args), getattr(new, name)(*args)
            if rp != rn:
                res["differences"] += 1
                print("DIFFERENT", name, rp, rn, flush=True)
            key = NAMES[rp] if name != sizes else ("size > 0" if rp else "0")
            hist[key] = hist.get(key, 0) + 1
        res["entries"][name] = hist
        want = {NAMES[c] for c in CAN[name]} if name != sizes else {"0", "size > 0"}
        res["unreached"] += [f"{name}: {c}" for c in sorted(want - set(hist))]
        print(name, hist, flush=True)
    res["total_calls"] = a.calls * len(entries)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(1 if res["differences"] or res["unreached"] else 0)


if __name__ == "__main__":
    main()
