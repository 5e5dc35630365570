"""CPU-only (run with -m "not gpu"): the return code of every fused C-ABI entry point over a sweep of the dispatch space, against codes recorded
from the library before the dispatch layer became one table (tests/golden/dispatch_codes.npz; its ``parent`` entry names the commit).

Pointers are fake (never dereferenced: every check decides first).  The training entry points get a 16-byte workspace, so no call launches; the
forward entry points are swept only in the cells they refuse (a negative NIC_E_* in the fixture; -128 marks a cell that would launch, not called
here - tests/test_gpu_dispatch_matrix.py runs those).  nic_workspace_bytes is recorded for every descriptor of the main sweep.

    python -m tests.test_dispatch_codes_cpu      # rewrites the fixture from the library in the tree"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dispatch_codes.npz")
FAKE, NULL = 16, None
LAUNCH = -128                                   # a forward cell that would launch

SPLIT, TILE32, MLPN, GBF16, GFP16, BF16, FP16, ORG_HOST = 2, 4, 8, 16, 32, 64, 128, 256
# (dim, method, pe_mode): the four layouts, then combinations pick_layout refuses
DIMS = [(2, 1, 0), (2, 1, 1), (3, 3, 0), (3, 4, 1), (3, 3, 1), (3, 4, 0), (2, 3, 0), (2, 1, 2), (3, 1, 0), (1, 1, 0)]
FLAGS = [a | b | c for a in (0, SPLIT, SPLIT | TILE32, BF16, FP16, BF16 | FP16, SPLIT | BF16) for b in (0, MLPN) for c in (0, GBF16, GFP16, GBF16 | GFP16)]
CP = [(c, p) for c in (4, 8, 12, 16, 20) for p in (4, 6, 8)]
NL = (0, 2, 3, 4, 5)
# argument variants on top of a valid call: which error wins when a dispatch refusal and an argument error apply together
VARIANTS = ("ok", "null_g0", "extent0", "noise_null", "org_host", "img_u8_3", "rgbx_huge", "tail", "passes2", "bits0")


def _main_cells():
    for (dim, method, pe), flags, (c, p), nl in itertools.product(DIMS, FLAGS, CP, NL):
        yield dim, method, pe, flags, c, p, 64, nl, "ok"
    for (dim, method, pe), flags, (c, p), nl in itertools.product(DIMS, (0, SPLIT, BF16), CP, NL):
        yield dim, method, pe, flags, c, p, 32, nl, "ok"


def _variant_cells():
    for (dim, method, pe), flags, (c, p), nl, v in itertools.product(DIMS, FLAGS, ((12, 6), (4, 6)), (3, 5, 2), VARIANTS[1:]):
        yield dim, method, pe, flags, c, p, 64, nl, v


def _ml_cells():
    for levels, (dim, method, pe), flags, (c, p), hidden, nl, v in itertools.product(range(1, 7), DIMS[:6], (0, GBF16, GFP16, BF16, SPLIT), CP, (64, 32), NL,
                                                                                    ("ok", "null_g0", "extent0")):
        if v == "ok" or (hidden == 64 and p == 6 and flags == 0):
            yield levels, dim, method, pe, flags, c, p, hidden, nl, v


def _desc(dim, method, pe, flags, c, p, hidden, v):
    from neural_image_compression_v2_amd import _lib
    d = _lib.NicPathDesc()
    d.dim, d.method, d.pe_mode, d.flags, d.channels, d.pe_channels, d.hidden = dim, method, pe, flags, c, p, hidden
    d.log2_step, d.num_crops, d.num_bits, d.loss_scale, d.noise_mode = -2, 3, 8, 1.0, _lib.NIC_NOISE_KERNEL
    for a in range(3):
        d.extent[a], d.g0_nodes[a], d.g1_nodes[a] = 37 - 8 * a, 65, 33
    d.g1_weight_mode = 1
    if v == "extent0":
        d.extent[0] = 0
    elif v == "noise_null":
        d.noise_mode = _lib.NIC_NOISE_TENSOR
    elif v == "org_host":
        d.flags |= ORG_HOST
        d.num_crops = 40
    elif v == "tail":
        d.tail = FAKE
    elif v == "passes2":
        d.passes = 2
    elif v == "bits0":
        d.num_bits = 0
    return d


def _mlp(nl):
    from neural_image_compression_v2_amd import _lib
    m = _lib.NicMlp()
    m.n_linear = nl
    for i in range(max(nl, 3)):
        m.w[i] = m.b[i] = FAKE
    return m


def _img(v):
    from neural_image_compression_v2_amd import _lib
    t = _lib.NicTargetImage()
    t.data, t.is_u8, t.den = FAKE, 1, 255.0
    for a in range(3):
        t.size[a] = 256
    if v == "img_u8_3":
        t.is_u8 = 3
    elif v == "rgbx_huge":
        t.is_u8, t.size[0], t.size[1] = 2, 65536, 65536
    return t


def _train_codes(lib, cell):
    """nic_fused_forward_backward, _img, nic_fused_backward_dy, _img_dev"""
    from neural_image_compression_v2_amd import _lib
    d = _desc(*cell[:7], cell[8])
    m, gs, img = _mlp(cell[7]), _lib.NicMlpGrads(), _img(cell[8])
    g0 = NULL if cell[8] == "null_g0" else FAKE
    step = ctypes.c_int64(0)
    a = (ctypes.byref(d), g0, FAKE, FAKE, ctypes.byref(m), NULL)
    return (lib.nic_fused_forward_backward(*a, FAKE, NULL, FAKE, FAKE, FAKE, ctypes.byref(gs), FAKE, 16, NULL),
            lib.nic_fused_forward_backward_img(*a, ctypes.byref(img), NULL, FAKE, FAKE, FAKE, ctypes.byref(gs), FAKE, 16, NULL),
            lib.nic_fused_backward_dy(*a, FAKE, FAKE, FAKE, ctypes.byref(gs), FAKE, 16, NULL),
            lib.nic_fused_forward_backward_img_dev(ctypes.byref(d), g0, FAKE, FAKE, ctypes.byref(m), ctypes.byref(img), FAKE, FAKE, FAKE, ctypes.byref(gs),
                                                   ctypes.byref(step), FAKE, 16, NULL))


def _forward_codes(lib, cell, expect=None):
    """nic_fused_forward, nic_fused_forward_u8: called only where ``expect`` (the fixture) says they refuse; recording calls every cell on a
    machine without a GPU, where a launch fails with a positive hip error"""
    d = _desc(*cell[:7], cell[8])
    m = _mlp(cell[7])
    g0 = NULL if cell[8] == "null_g0" else FAKE
    du = _desc(*cell[:7], cell[8])
    if cell[8] != "noise_null":
        du.noise_mode = 0                       # a decode draws no noise
    calls = (lambda: lib.nic_fused_forward(ctypes.byref(d), g0, FAKE, FAKE, ctypes.byref(m), NULL, FAKE, NULL),
             lambda: lib.nic_fused_forward_u8(ctypes.byref(du), g0, FAKE, FAKE, ctypes.byref(m), FAKE, NULL, NULL))
    out = []
    for i, call in enumerate(calls):
        if expect is not None and expect[i] == LAUNCH:
            out.append(LAUNCH)
            continue
        rc = call()
        out.append(rc if rc < 0 else LAUNCH)
    return out


def _ml_codes(lib, cell, expect=None):
    """nic_fused_ml_forward_backward (16-byte workspace), nic_fused_ml_forward (refused cells only, as above)"""
    from neural_image_compression_v2_amd import _lib
    from neural_image_compression_v2_amd.multilevel import level_nodes
    levels, v = cell[0], cell[9]
    d = _desc(*cell[1:8], v)
    d.noise_mode = _lib.NIC_NOISE_NONE
    pr = _lib.NicMlPairs()
    pr.levels = levels
    for l in range(min(levels, _lib.NIC_ML_MAX_LEVELS)):
        nodes = level_nodes((1024, 1024), l)
        pr.g0[l] = pr.g1[l] = pr.g0_grad[l] = pr.g1_grad[l] = FAKE
        for ax in range(2):
            pr.g0_nodes[l][ax], pr.g1_nodes[l][ax] = nodes[0][ax], nodes[1][ax]
    for ax in range(2):
        d.g0_nodes[ax], d.g1_nodes[ax] = pr.g0_nodes[0][ax], pr.g1_nodes[0][ax]
    if v == "null_g0":
        pr.g0[levels - 1 if levels <= _lib.NIC_ML_MAX_LEVELS else 0] = None
    m, gs = _mlp(cell[8]), _lib.NicMlpGrads()
    train = lib.nic_fused_ml_forward_backward(ctypes.byref(d), ctypes.byref(pr), FAKE, ctypes.byref(m), NULL, FAKE, NULL, FAKE, ctypes.byref(gs), FAKE,
                                              16, NULL)
    if expect is not None and expect == LAUNCH:
        return train, LAUNCH
    rc = lib.nic_fused_ml_forward(ctypes.byref(d), ctypes.byref(pr), FAKE, ctypes.byref(m), FAKE, NULL)
    return train, (rc if rc < 0 else LAUNCH)


def _decoder_codes(lib):
    """nic_decoder_backward (16-byte workspace) over Cin / hidden / depth / n, and the pointer checks"""
    from neural_image_compression_v2_amd import _lib
    out = []
    for cin, hidden, nl, n, null_x in itertools.product((73, 127, 79, 72, 74), (64, 32), NL, (-1, 0, 1, 1 << 20), (False, True)):
        m, gs = _mlp(nl), _lib.NicMlpGrads()
        out.append(lib.nic_decoder_backward(ctypes.byref(m), NULL if null_x else FAKE, FAKE, n, cin, hidden, FAKE, ctypes.byref(gs), FAKE, 16, NULL))
    return out


def sweep(lib, fixture=None):
    """the codes of every cell, as int arrays; with ``fixture`` the forward entry points skip the cells the fixture marks as launching"""
    main = list(_main_cells()) + list(_variant_cells())
    train = np.array([_train_codes(lib, c) for c in main], dtype=np.int32)
    fexp = fixture["forward"] if fixture is not None else itertools.repeat(None)
    forward = np.array([_forward_codes(lib, c, e) for c, e in zip(main, fexp)], dtype=np.int32)
    ws = np.array([lib.nic_workspace_bytes(ctypes.byref(_desc(*c[:7], c[8]))) for c in _main_cells()] + [lib.nic_workspace_bytes(None)], dtype=np.int64)
    mcells = list(_ml_cells())
    mexp = fixture["ml"][:, 1] if fixture is not None else itertools.repeat(None)
    ml = np.array([_ml_codes(lib, c, e) for c, e in zip(mcells, mexp)], dtype=np.int32)
    return {"train": train, "forward": forward, "workspace": ws, "ml": ml, "decoder": np.array(_decoder_codes(lib), dtype=np.int32)}


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def test_return_codes_match_the_recorded_dispatch(lib):
    want = dict(np.load(FIXTURE))
    got = sweep(lib, want)
    for k, g in got.items():
        w = want[k]
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{k}: {len(bad)} cells differ, first {bad[:5].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"
    assert (want["forward"] != 0).all() and (want["ml"][:, 1] != 0).all()       # a forward cell either refuses or is not called


if __name__ == "__main__":
    from neural_image_compression_v2_amd import _lib
    codes = sweep(_lib.load())
    parent = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip()
    np.savez_compressed(FIXTURE, parent=np.array(parent), **codes)
    print({k: v.shape for k, v in codes.items()}, parent, os.path.getsize(FIXTURE))
