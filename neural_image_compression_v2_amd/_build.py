"""Builds libnicv2_hip.so (the C-ABI library, include/nicv2_hip.h) in-tree with hipcc for gfx950.

    python -m neural_image_compression_v2_amd._build [--force]

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels to the GPU box with the snapshot.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(HERE, "libnicv2_hip.so")
SOURCES = ["simple_kernels.hip", "decoder_general.hip", "fused_capi.hip", "fused_m1.hip", "fused_m2.hip", "fused_m3.hip", "fused_m4.hip", "fused_t16.hip", "fused_mlpn.hip", "fused_q1.hip", "fused_q2.hip", "fused_q3.hip", "fused_q4.hip",
           "hash_grid.hip", "hash_fused.hip", "hash_points.hip", "hash_points_train.hip", "hash_mixed.hip", "hashgrid_fused16.hip", "hashgrid_pointgrad.hip", "hashgrid_points_joint.hip", "hashgrid_batch.hip",
           "hashgrid_batch_grad.hip", "hashgrid_lodgrad.hip", "hashgrid_lodtrain.hip", "hashgrid_weighted.hip"]
# the lists of csrc/fused_capi.hip (NIC_CP_LIST, NIC_ML_LIST): one object per entry, compiled from one source with the entry as NIC_ENTRY
LISTED = {"NIC_CP_LIST": ("fused_qc.hip", "fused_qc_{}_{}_{}.o"),        # (layout, C, P): non-default channel counts on the plain-bf16 kernels
          "NIC_ML_LIST": ("fused_ml.hip", "fused_ml_{}_{}_{}.o")}        # (levels, C, n_linear): multi-level layouts (fused_q16.hpp::QML)
HEADERS = ["nic_device.hpp", "nic_adam.hpp", "fused_kernel.hpp", "fused_dispatch.hpp", "fused_launch.hpp", "fused_train16.hpp", "fused_mlpn.hpp", "fused_q16.hpp", "fused_q16_launch.hpp", "hash_common.hpp", "hashgrid_pointgrad.hpp", "hashgrid_batch.hpp", os.path.join("..", "..", "include", "nicv2_hip.h"),
           os.path.join("..", "..", "include", "nicv2_hip_ext.h")]
# -amdgpu-mfma-vgpr-form: MFMA results that vector instructions consume may live in the architectural VGPRs instead of bouncing
# through v_accvgpr_read / write (split training kernel: 656 -> 423 of them, -0.7 %; fp32 2D 18 -> 0 spills; 3D 170 -> 115 / 135 -> 85)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def instance_list(name: str):
    """the (a, b, c) entries of ``#define NAME(X) X(a, b, c) ...`` in csrc/fused_capi.hip, in order"""
    with open(os.path.join(CSRC, "fused_capi.hip")) as f:
        lines = f.read().splitlines()
    start = [i for i, ln in enumerate(lines) if re.match(rf"\s*#define\s+{name}\(X\)", ln)]
    assert len(start) == 1, f"{name} is defined {len(start)} times in fused_capi.hip"
    body, i = [], start[0]
    while True:
        body.append(lines[i])
        if not lines[i].rstrip().endswith("\\"):
            break
        i += 1
    return [tuple(int(v) for v in m) for m in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", "\n".join(body))]


def units():
    """(source, object, extra defines) of every translation unit of the library"""
    out = [(s, s.replace(".hip", ".o"), []) for s in SOURCES]
    for name, (src, obj) in LISTED.items():
        out += [(src, obj.format(*e), ["-DNIC_ENTRY=" + ",".join(str(v) for v in e)]) for e in instance_list(name)]
    return out


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    jobs = []
    for src, obj, defs in units():
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, obj)
        if force or _stale(o, [s] + hdrs):
            jobs.append((s, o, defs))

    def cc(job):
        s, o, defs = job
        extra = ["-ffp-contract=off"] if os.path.basename(s) == "simple_kernels.hip" else []   # op-by-op rounding like eager torch
        # the plain-bf16 kernels without SLP vectorisation (the guide's anti-lever: adjacent scalar f32 operations packed into v_pk_* beside MFMAs):
        # 4K launch 1.420 -> 1.401 ms, 128^3 method 3 0.483 -> 0.461, method 4 0.426 -> 0.417 (interleaved A/B, identical results); the split and fp32
        # kernels do not move (or lose 1 %): they keep the default
        # (fused_t16: 2.122 -> 2.104 ms on the final kernel; it did not move before the 16x16x16 products went in)
        if os.path.basename(s).startswith("fused_q") or os.path.basename(s) in ("fused_ml.hip", "fused_t16.hip"):
            extra.append("-fno-slp-vectorize")
        cmd = [hipcc, *FLAGS, *extra, *defs, "-c", s, "-o", o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {s}:\n{r.stdout}\n{r.stderr}")
        if verbose:
            print(f"[build] {os.path.basename(o)}", flush=True)
        return o

    if jobs:
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            list(ex.map(cc, jobs))
    objs = [os.path.join(OBJ, obj) for _, obj, _ in units()]
    if force or jobs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        if verbose:
            print(f"[build] linked {LIB}", flush=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
