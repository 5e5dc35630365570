#!/usr/bin/env python3
"""Writes the stored hash-grid fixtures under ``tests/golden/hashgrid/`` (test infrastructure; CPU only, no GPU, no test runs it).

For every case of ``CASES``: ``NAME.pt``, a stored file built by ``oracle.hashgrid_ref.make_file`` (codes from an integer formula, the
decoder from ``torch.manual_seed`` + nn.Linear's default initialisation times the case's scale), and ``NAME.npz`` with what the float64
reference decoder makes of that file's bytes: ``decode`` (the whole field), ``points`` (fp32, ``query_points``) and ``query`` at them,
``resample`` to the odd size ``resample_size``.  The cases are the smallest with dense and hashed levels and partial patches, the shapes of
``tests/test_gpu_hashgrid_p16.py``.  ``tests/test_hashgrid_stored_ref_cpu.py`` regenerates everything into a temporary directory and holds the
committed files to it bit for bit, so a format change that moves the meaning of the bytes, or a change of the reference, shows up as a diff of
fixtures that were written by an earlier commit.

Run:  python oracle/make_hashgrid_golden.py            (from the repository root)"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import hashgrid_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hashgrid")
N_POINTS = 209          # three waves and a ragged fourth

_2D = dict(field_size=(44, 37), log2_table=10, base=16, hidden=64, n_linear=3)
_3D = dict(field_size=(12, 10, 9), log2_table=10, base=4, hidden=64, n_linear=3)
SIZE_2D, SIZE_3D = (17, 50), (5, 13, 4)     # down on one axis and up on another

# The decoder scale is 1.5 (activations leave GELU's linear part, tests/test_gpu_hashgrid_fused.py); hg2d_u8_b5 keeps the default
# initialisation, for which the project's bf16 bound is stated.  Every file must let one step of ONE code of its finest level move the
# reference's decode by more than 1e-4 (tests/test_hashgrid_stored_ref_cpu.py).  The finest level equals the field size here, so all its
# corner weights are 1/4 (2D) or 1/8 (3D), and a step of 1/255 or 1/127 needs a steeper decoder than a step of 1/15: where seeds 1, 2, 3 do
# not get there the seed is the best of 1 .. 60, and where no seed does the scale is the lowest step of 0.5 at which one does (hg3d_u8_b8
# 2.5, hg2d_u8_b8 and hg2d_u8_b8_h32n4 2.0) - as small as possible, since the project states its split-bf16 bound up to a doubled decoder
# only.  hg2d_u8_b8 was meant to keep scale 1.0 for the bf16 bound as well, but there a step of 1/255 moves decode by at most 1.5e-5
# (seeds 1 .. 150; 5.8e-5 at scale 1.5): the teeth condition decides, and the bf16 bound stays asserted on hg2d_u8_b5 and its batches.
CASES = [
    dict(name="hg2d_u8_b8", seed=49, resample=SIZE_2D, spec=dict(_2D, levels=6, features=2, fmt="u8", bits=8, scale=2.0)),
    dict(name="hg2d_u8_b5", seed=12, resample=SIZE_2D, spec=dict(_2D, levels=6, features=2, fmt="u8", bits=5, scale=1.0)),
    dict(name="hg2d_bits1_b4", seed=3, resample=SIZE_2D, spec=dict(_2D, levels=6, features=2, fmt="bits1", bits=4, scale=1.5)),      # tight: F b divides 32
    dict(name="hg2d_bits1_b5", seed=1, resample=SIZE_2D, spec=dict(_2D, levels=6, features=2, fmt="bits1", bits=5, scale=1.5)),      # straddling
    dict(name="hg2d_bits2", seed=2, resample=SIZE_2D, spec=dict(_2D, levels=6, features=2, fmt="bits2", bits=(8, 5, 3, 4, 1, 6), scale=1.5)),
    dict(name="hg2d_bits1_b3_w64", seed=3, resample=SIZE_2D, spec=dict(_2D, levels=8, features=8, fmt="bits1", bits=3, scale=1.5)),  # L F = 64
    dict(name="hg3d_u8_b8", seed=24, resample=SIZE_3D, spec=dict(_3D, levels=4, features=4, fmt="u8", bits=8, scale=2.5)),
    dict(name="hg3d_bits1_b7", seed=37, resample=SIZE_3D, spec=dict(_3D, levels=4, features=1, fmt="bits1", bits=7, scale=1.5)),
    dict(name="hg3d_bits2", seed=3, resample=SIZE_3D, spec=dict(_3D, levels=4, features=4, fmt="bits2", bits=(7, 2, 6, 1), scale=1.5)),
    # the general decoder: layer-wise route only
    dict(name="hg2d_u8_b8_h32n4", seed=20, resample=SIZE_2D, spec=dict(_2D, levels=6, features=2, fmt="u8", bits=8, scale=2.0, hidden=32, n_linear=4)),
]


def _unit(seed: int, n: int, dim: int) -> np.ndarray:
    """[n, dim] float64 in [0, 1): 24 bits of an integer mix of (seed, point, axis), no RNG"""
    m = np.uint64(0xFFFFFFFF)
    i = np.arange(n, dtype=np.uint64)[:, None]
    a = np.arange(dim, dtype=np.uint64)[None, :]
    h = (np.uint64(seed) * np.uint64(0x9E3779B1) + i * np.uint64(0x85EBCA77) + a * np.uint64(0xC2B2AE3D) + np.uint64(0x27D4EB2F)) & m
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & m
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & m
    h = h ^ (h >> np.uint64(16))
    return (h >> np.uint64(8)).astype(np.float64) / float(1 << 24)


def query_points(field_size, resolutions, seed: int = 0, n: int = N_POINTS) -> np.ndarray:
    """fp32 [n, dim]: the edges of the accepted domain first, then pseudo-random points in [-0.2 S, 1.2 S] (``seed`` moves only those)"""
    S = [int(s) for s in field_size]
    dim, s_max, r0 = len(S), max(S), int(resolutions[0])
    mid = [np.float32(s // 2) + np.float32(0.25) for s in S]
    rows = []

    def put(**axes):                       # a point at the field's middle with the named axes replaced
        p = list(mid)
        for a, v in axes.items():
            p[int(a[1:])] = np.float32(v)
        rows.append(p)

    for corner in np.ndindex(*([2] * dim)):                                      # the corner sample centres
        rows.append([np.float32(c * (s - 1)) for c, s in zip(corner, S)])
    rows.append([np.float32(-0.5)] * dim)                                        # the edges of the field themselves
    rows.append([np.float32(s - 0.5) for s in S])
    rows.append([np.nextafter(np.float32(s - 0.5), np.float32(0)) for s in S])   # the largest fp32 below S_a - 1/2
    for a in range(dim):                                                         # outside on either side, one axis at a time and all at once
        put(**{f"a{a}": -3.75})
        put(**{f"a{a}": S[a] + 2.5})
    rows.append([np.float32(-1e6)] * dim)
    rows.append([np.float32(s + 1e6) for s in S])
    for v in (np.nan, np.inf, -np.inf):                                          # NaN, +inf and -inf in one coordinate each, on every axis
        for a in range(dim):
            put(**{f"a{a}": v})
    put(a0=np.inf, a1=np.nan)
    # a vertex of the coarsest level: t R_0 = 256 S_max k, w = 0 on that axis
    assert (256 * s_max) % r0 == 0
    for k in (1, 2):
        t = 256 * s_max * k // r0
        rows.append([np.float32((t - 128) / 256.0)] * dim)
    put(a0=(256 * s_max // r0 - 128) / 256.0)
    # the two tie cases of rint: 256 p = k + 1/2 with k even and k odd
    for k in (1000, 1001, -64, -63):
        put(a0=k / 256.0 + 1.0 / 512.0)
        put(**{f"a{dim - 1}": k / 256.0 + 1.0 / 512.0})
    fixed = np.array(rows, dtype=np.float32)
    assert fixed.shape[0] < n
    rest = ((-0.2 + 1.4 * _unit(seed, n - fixed.shape[0], dim)) * np.array(S, dtype=np.float64)).astype(np.float32)
    return np.concatenate([fixed, rest]).astype(np.float32)


def reference_arrays(case: dict, d: dict) -> dict:
    """what ``NAME.npz`` holds for the file dict ``d`` of ``case``"""
    f = R.parse(d)
    pts = query_points(f.field_size, f.resolutions)
    return {"decode": R.decode(f), "points": pts, "query": R.query(f, pts), "resample": R.resample(f, case["resample"]),
            "resample_size": np.array(case["resample"], dtype=np.int64)}


def write(out_dir: str, cases=CASES) -> None:
    os.makedirs(out_dir, exist_ok=True)
    for case in cases:
        d = R.make_file(case["spec"], case["seed"])
        R.save(d, os.path.join(out_dir, case["name"] + ".pt"))
        np.savez(os.path.join(out_dir, case["name"] + ".npz"), **reference_arrays(case, d))


if __name__ == "__main__":
    write(OUT)
    for case in CASES:
        sizes = [os.path.getsize(os.path.join(OUT, case["name"] + ext)) for ext in (".pt", ".npz")]
        print(f"{case['name']}: .pt {sizes[0]} bytes, .npz {sizes[1]} bytes")
