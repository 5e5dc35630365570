"""CPU-only checks (run with -m "not gpu") that tie the fused dispatch tables together: NIC_CP_LIST / NIC_ML_LIST in csrc/fused_capi.hip, the
objects _build.py compiles for them, the dispatch table of csrc/fused_capi.hip, fused.ML_FUSED, and the cell matrix of
tests/test_gpu_dispatch_matrix.py.  Through the C ABI with
fake pointers (never dereferenced: the checks decide first, as in test_host_cpu.py) every listed entry gets past dispatch and its unlisted
neighbours are refused with NIC_E_UNSUPPORTED."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_gpu_dispatch_matrix import (FAMILIES, LAYOUTS, MODES, REFUSED, Cell, cp_list, enumerate_cells, geometry,
                                            ml_list)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural_image_compression_v2_amd", "csrc")
E_UNSUPPORTED, E_WORKSPACE = -2, -4
MODE_NAMES = {"TRAIN_MSE": "mse", "TRAIN_IMG": "img", "TRAIN_DY": "dy", "INFER": "infer"}


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _launched_modes(path: str, start: str):
    """the MODE_* of the hipLaunchKernelGGL lines of the function template of ``path`` that begins at the line matching ``start``"""
    with open(path) as f:
        lines = f.read().splitlines()
    i = next(k for k, ln in enumerate(lines) if re.search(start, ln))
    modes = set()
    for ln in lines[i + 1:]:
        if re.match(r"\s*(#define|template <|}\s*//\s*namespace)", ln):
            break
        if "hipLaunchKernelGGL" in ln:
            modes |= {MODE_NAMES[m] for m in re.findall(r"MODE_(\w+)", ln.split("hipLaunchKernelGGL", 1)[1])}
    return modes


def test_lists_match_the_build_and_the_translation_units():
    """the lists live in fused_capi.hip alone; every entry has an object in the build and a record in the dispatch table"""
    from neural_image_compression_v2_amd import _build, fused
    cp = cp_list()
    ml = ml_list()
    assert len(cp) == len(set(cp)) >= 15 and len(ml) == len(set(ml)) >= 7
    objs = [o for _, o, _ in _build.units()]
    assert len(objs) == len(set(objs))
    for e in cp:
        assert "fused_qc_{}_{}_{}.o".format(*e) in objs, e
    for e in ml:
        assert "fused_ml_{}_{}_{}.o".format(*e) in objs, e
    assert set(fused.ML_FUSED) == set(ml), "fused.ML_FUSED (MultiLevelField's choice of route) and NIC_ML_LIST differ"
    with open(os.path.join(CSRC, "fused_capi.hip")) as f:
        capi = f.read()
    # the table holds one record per list entry (q16_cp_kernels / ml_kernels, expanded from the lists)
    assert re.search(r"#define X\(L, C, P\) q16_cp_kernels<L, C, P>\(\),\s*NIC_CP_LIST\(X\)", capi)
    assert re.search(r"#define X\(LV, C, NL\) ml_kernels<LV, C, NL>\(\),\s*NIC_ML_LIST\(X\)", capi)
    for name in os.listdir(CSRC):                            # no other copy of the lists
        if name != "fused_capi.hip" and name.endswith((".h", ".hpp", ".hip")):
            with open(os.path.join(CSRC, name)) as f:
                assert not re.search(r"#define\s+NIC_(CP|ML)_LIST", f.read()), name


def test_the_enumerator_covers_every_entry_in_every_instantiated_mode():
    cells = enumerate_cells()
    assert len(cells) == len(set(cells))
    q16_modes = _launched_modes(os.path.join(CSRC, "fused_q16_launch.hpp"), r"static int launch_q16_nl\(")
    ml_modes = _launched_modes(os.path.join(CSRC, "fused_q16_launch.hpp"), r"static int launch_ml\(")
    assert q16_modes == set(MODES) and ml_modes == {"mse", "infer"}
    for layout, C, P in cp_list():
        for grid in ("fp32", "bf16", "fp16"):
            got = {c.mode for c in cells if c.family == "cp" and (c.layout, c.C, c.P, c.grid) == (layout, C, P, grid)}
            assert got == q16_modes, (layout, C, P, grid, got)
    for levels, C, nl in ml_list():
        for layout in (1, 2):                                # both positional encodings
            got = {c.mode for c in cells if c.family == "ml" and (c.levels, c.C, c.nl, c.layout) == (levels, C, nl, layout)}
            assert got == ml_modes, (levels, C, nl, layout, got)
    for fam, (layouts, nls, grids) in FAMILIES.items():
        for layout in layouts:
            for nl in nls:
                for grid in grids:
                    assert {c.mode for c in cells if c[:6] == (fam, layout, 12, 6, nl, grid)} == set(MODES), (fam, layout, nl, grid)
    assert not set(REFUSED) & set(cells)


def test_the_enumerator_does_not_touch_a_device():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import torch; import tests.test_gpu_dispatch_matrix as M; M.enumerate_cells(); "
            "assert not torch.cuda.is_initialized()" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ the C ABI with fake pointers (16-byte workspace: NIC_E_WORKSPACE = got past dispatch)

FAKE, NULL = ctypes.c_void_p(16), ctypes.c_void_p(0)


def _desc(c: Cell):
    """nic_path_desc of a cell at the GPU test's shapes (grid shapes and dtype from CPU stand-ins: to_desc reads shapes and dtype only)"""
    from tests.test_gpu_dispatch_matrix import DTYPE, EXTENT, ORIGINS
    dim = LAYOUTS[c.layout][0]
    n0, n1 = (65, 33) if dim == 2 else (17, 9)
    g0 = torch.empty((c.C,) + (n0,) * dim, dtype=DTYPE[c.grid])
    g1 = torch.empty((c.C,) + (n1,) * dim, dtype=DTYPE[c.grid])
    return geometry(c, EXTENT[dim], len(ORIGINS[dim])).to_desc(g0, g1)


def _mlp(nl):
    from neural_image_compression_v2_amd import _lib
    m = _lib.NicMlp()
    m.n_linear = nl
    for i in range(nl):
        m.w[i] = m.b[i] = 16
    return m


def _train_rc(lib, c: Cell) -> int:
    from neural_image_compression_v2_amd import _lib
    d, m, gs = _desc(c), _mlp(c.nl), _lib.NicMlpGrads()
    if c.mode == "img":
        t = _lib.NicTargetImage()
        t.data, t.is_u8, t.den = 16, 1, 255.0
        for a in range(3):
            t.size[a] = 256
        return lib.nic_fused_forward_backward_img(ctypes.byref(d), FAKE, FAKE, FAKE, ctypes.byref(m), NULL, ctypes.byref(t), NULL, FAKE, FAKE, FAKE,
                                                  ctypes.byref(gs), FAKE, 16, NULL)
    if c.mode == "dy":
        return lib.nic_fused_backward_dy(ctypes.byref(d), FAKE, FAKE, FAKE, ctypes.byref(m), NULL, FAKE, FAKE, FAKE, ctypes.byref(gs), FAKE, 16, NULL)
    return lib.nic_fused_forward_backward(ctypes.byref(d), FAKE, FAKE, FAKE, ctypes.byref(m), NULL, FAKE, NULL, FAKE, FAKE, FAKE, ctypes.byref(gs),
                                          FAKE, 16, NULL)


def _ml_rc(lib, levels, C, nl, layout=1, grid="fp32") -> int:
    from neural_image_compression_v2_amd import _lib
    from neural_image_compression_v2_amd.multilevel import level_nodes
    size = (1024, 1024)
    pr = _lib.NicMlPairs()
    pr.levels = levels
    for l in range(levels):
        nodes = level_nodes(size, l)
        pr.g0[l] = pr.g1[l] = pr.g0_grad[l] = pr.g1_grad[l] = 16
        for ax in range(2):
            pr.g0_nodes[l][ax], pr.g1_nodes[l][ax] = nodes[0][ax], nodes[1][ax]
    c = Cell("ml", layout, C, 6, nl, grid, levels, "mse")
    d = _desc(c)
    for ax in range(2):
        d.g0_nodes[ax], d.g1_nodes[ax] = pr.g0_nodes[0][ax], pr.g1_nodes[0][ax]
    gs = _lib.NicMlpGrads()
    return lib.nic_fused_ml_forward_backward(ctypes.byref(d), ctypes.byref(pr), FAKE, ctypes.byref(_mlp(nl)), NULL, FAKE, NULL, FAKE, ctypes.byref(gs),
                                             FAKE, 16, NULL)


def test_every_training_cell_gets_past_dispatch(lib):
    bad = {}
    for c in enumerate_cells():
        if c.mode == "infer":                                # (no workspace: the forward entry points would launch)
            continue
        rc = _ml_rc(lib, c.levels, c.C, c.nl, c.layout) if c.family == "ml" else _train_rc(lib, c)
        if rc != E_WORKSPACE:
            bad[str(c)] = rc
    assert not bad, bad


def test_refused_combinations_are_unsupported(lib):
    for c in REFUSED:
        rc = _ml_rc(lib, c.levels, c.C, c.nl, c.layout, c.grid) if c.family == "ml" else _train_rc(lib, c)
        assert rc == E_UNSUPPORTED, (c, rc)


def test_channel_count_list_through_the_c_abi(lib):
    """every NIC_CP_LIST entry with NIC_FLAG_BF16 dispatches; unlisted neighbours, the same widths without the bf16 flag, with the fp16 flag or with
    a 5-layer decoder are refused"""
    listed = set(cp_list())
    for layout, C, P in listed:
        c = Cell("cp", layout, C, P, 3, "fp32", 1, "mse")
        assert _train_rc(lib, c) == E_WORKSPACE, c
        for fam in ("fp32", "t16" if layout <= 2 else "split3d", "fp16"):
            assert _train_rc(lib, c._replace(family=fam)) == E_UNSUPPORTED, (fam, c)
        assert _train_rc(lib, c._replace(nl=5)) == E_UNSUPPORTED, c
    neighbours = [(1, 4, 4), (3, 16, 6), (4, 12, 4), (2, 20, 6), (3, 12, 4), (4, 12, 8), (1, 16, 4), (2, 8, 8)]
    for layout, C, P in neighbours:
        assert (layout, C, P) not in listed
        assert _train_rc(lib, Cell("cp", layout, C, P, 3, "fp32", 1, "mse")) == E_UNSUPPORTED, (layout, C, P)


def test_multilevel_list_through_the_c_abi(lib):
    """every NIC_ML_LIST entry, both encodings, dispatches; a neighbour in levels, channels or depth is refused"""
    from neural_image_compression_v2_amd import _lib
    listed = set(ml_list())
    for levels, C, nl in listed:
        for layout in (1, 2):
            assert _ml_rc(lib, levels, C, nl, layout) == E_WORKSPACE, (levels, C, nl, layout)
        for nb in ((levels + 1, C, nl), (levels, C + 4, nl), (levels, C, 8 - nl), (4, C, nl)):
            if nb not in listed and nb[0] <= _lib.NIC_ML_MAX_LEVELS:
                assert _ml_rc(lib, *nb) == E_UNSUPPORTED, (nb, "neighbour of", (levels, C, nl))
