"""CPU-only tests of the fused hash-grid encode + decoder entry points (run with -m "not gpu"): the symbols exist in the library, the header
and the ctypes mirror; every argument error is decided on the host; the supported set and the Python route choice that follows it; no product
path without a HIP device."""
import ctypes
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nicv2_hip.h")
NEW = ["nic_hash_fused_supported", "nic_hash_fused_workspace_bytes", "nic_hash_fused_forward", "nic_hash_fused_forward_u8", "nic_hash_fused_forward_backward"]
OK, NULL, UNSUP, SHAPE, WORKSPACE, ARG = 0, -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def lib():
    from neural_image_compression_v2_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _desc(dim=2, resolutions=(16,) * 16, features=2, log2_table=19, s_max=3840, num_crops=1, extent=(8, 8, 1)):
    from neural_image_compression_v2_amd._lib import NicHashDesc
    d = NicHashDesc()
    d.dim, d.levels, d.features, d.log2_table, d.S_max, d.num_crops = dim, len(resolutions), features, log2_table, s_max, num_crops
    for a in range(3):
        d.extent[a] = extent[a]
    for l, r in enumerate(resolutions):
        d.resolution[l] = r
    return d


def _mlp(n_linear=3, null_at=None):
    from neural_image_compression_v2_amd._lib import NicMlp
    m = NicMlp()
    for i in range(3):
        m.w[i] = 16
        m.b[i] = 16
    if null_at is not None:
        m.w[null_at] = 0
    m.n_linear = n_linear
    return m


def _grads():
    from neural_image_compression_v2_amd._lib import NicMlpGrads
    g = NicMlpGrads()
    for i in range(3):
        g.w[i] = 32 + 64 * i
        g.b[i] = 48 + 64 * i
    return g


DUMMY = ctypes.c_void_p(16)                 # never dereferenced: every case fails on the host first


def _calls(lib, d, m=None, bits=8, ws_bytes=1 << 30, quant=None, flags=0, tail=None):
    """the return codes of the three launching entry points for one descriptor"""
    m = _mlp() if m is None else m
    dp = None if d is None else ctypes.byref(d)
    f = lib.nic_hash_fused_forward(dp, DUMMY, DUMMY, ctypes.byref(m), DUMMY, None)
    u = lib.nic_hash_fused_forward_u8(dp, bits, DUMMY, DUMMY, ctypes.byref(m), DUMMY, None)
    g = _grads()
    t = lib.nic_hash_fused_forward_backward(dp, quant, DUMMY, DUMMY, ctypes.byref(m), DUMMY, 1.0, DUMMY, ctypes.byref(g), DUMMY, None, flags, DUMMY, ws_bytes,
                                            tail, None)
    return f, u, t


def test_symbols_exported_declared_and_mirrored(lib):
    from neural_image_compression_v2_amd import _lib
    header = open(HEADER).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\b{name}\s*\(", header), name
    assert lib.nic_abi_version() == 9 == _lib.NIC_ABI_VERSION
    assert (_lib.NIC_HASH_FUSED_ADD_GRADS, _lib.NIC_HASH_FUSED_ADD_LOSS) == (1, 2)
    assert re.search(r"#define\s+NIC_HASH_FUSED_ADD_GRADS\s+1\b", header) and re.search(r"#define\s+NIC_HASH_FUSED_ADD_LOSS\s+2\b", header)


def test_descriptor_errors_before_any_gpu_work(lib):
    def all_rc(d):
        f, u, t = _calls(lib, d)
        s = lib.nic_hash_fused_supported(None if d is None else ctypes.byref(d), 64, 3)
        assert f == u == t == s, (f, u, t, s)
        return f

    assert all_rc(None) == NULL
    for dim in (1, 4):
        assert all_rc(_desc(dim=dim)) == UNSUP
    for f in (0, 3, 5, 16):
        assert all_rc(_desc(features=f, resolutions=(16,))) == UNSUP
    assert all_rc(_desc(resolutions=())) == ARG                                         # levels 0
    too_many = _desc(resolutions=(16,) * 32, features=1)
    too_many.levels = 33
    assert all_rc(too_many) == ARG
    for lg in (9, 25):
        assert all_rc(_desc(log2_table=lg)) == ARG
    assert all_rc(_desc(resolutions=(16, 0, 32))) == ARG
    assert all_rc(_desc(resolutions=(1 << 20,), s_max=1 << 10)) == ARG
    assert all_rc(_desc(num_crops=0)) == SHAPE
    assert all_rc(_desc(extent=(0, 8, 1))) == SHAPE
    assert all_rc(_desc(extent=(8, 4000, 1))) == SHAPE
    bad = _desc()
    bad.flags = 1
    assert all_rc(bad) == ARG


def test_pointer_bits_workspace_and_flag_errors(lib):
    from neural_image_compression_v2_amd._lib import NicHashQuant, NicStepTail, NicAdamTensor, NIC_NOISE_KERNEL, NIC_NOISE_TENSOR
    d, m, g = _desc(), _mlp(), _grads()
    dp, mp, gp = ctypes.byref(d), ctypes.byref(m), ctypes.byref(g)
    # forward
    assert lib.nic_hash_fused_forward(dp, None, DUMMY, mp, DUMMY, None) == NULL
    assert lib.nic_hash_fused_forward(dp, DUMMY, None, mp, DUMMY, None) == NULL
    assert lib.nic_hash_fused_forward(dp, DUMMY, DUMMY, None, DUMMY, None) == NULL
    assert lib.nic_hash_fused_forward(dp, DUMMY, DUMMY, mp, None, None) == NULL
    assert lib.nic_hash_fused_forward(dp, DUMMY, DUMMY, ctypes.byref(_mlp(null_at=1)), DUMMY, None) == NULL
    # forward from the stored table
    assert lib.nic_hash_fused_forward_u8(dp, 8, None, DUMMY, mp, DUMMY, None) == NULL
    assert lib.nic_hash_fused_forward_u8(dp, 8, DUMMY, None, mp, DUMMY, None) == NULL
    assert lib.nic_hash_fused_forward_u8(dp, 8, DUMMY, DUMMY, None, DUMMY, None) == NULL
    assert lib.nic_hash_fused_forward_u8(dp, 8, DUMMY, DUMMY, mp, None, None) == NULL
    for bits in (0, 9, -1):
        assert lib.nic_hash_fused_forward_u8(dp, bits, DUMMY, DUMMY, mp, DUMMY, None) == ARG
    # training
    big = 1 << 30

    def train(quant=None, table=DUMMY, org=DUMMY, mlp=mp, target=DUMMY, grad=DUMMY, grads=gp, loss=DUMMY, flags=0, ws=DUMMY, ws_bytes=big, tail=None):
        return lib.nic_hash_fused_forward_backward(dp, quant, table, org, mlp, target, 1.0, grad, grads, loss, None, flags, ws, ws_bytes, tail, None)

    for kw in (dict(table=None), dict(org=None), dict(mlp=None), dict(target=None), dict(grads=None), dict(loss=None), dict(ws=None)):
        assert train(**kw) == NULL, kw
    assert train(mlp=ctypes.byref(_mlp(null_at=2))) == NULL
    assert train(ws_bytes=64) == WORKSPACE
    rec = 64 * 32 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 1                                 # one record: the decoder's gradients + the loss
    need = lib.nic_hash_fused_workspace_bytes(dp, mp)
    assert need >= 8 * rec * 4 and need % (rec * 4) == 0
    assert train(ws_bytes=8 * rec * 4 - 1) == WORKSPACE                                 # the smallest launch is 8 workgroups
    assert train(flags=4) == ARG
    for bits in (0, 9):
        assert train(quant=ctypes.byref(NicHashQuant(bits, NIC_NOISE_KERNEL, 1, 2, 0))) == ARG
    assert train(quant=ctypes.byref(NicHashQuant(8, NIC_NOISE_KERNEL, 1, 2, -1))) == ARG
    assert train(quant=ctypes.byref(NicHashQuant(8, NIC_NOISE_TENSOR, 1, 2, 0))) == UNSUP
    assert train(quant=ctypes.byref(NicHashQuant(8, 7, 1, 2, 0))) == ARG
    # a tail whose decoder gradient is not one of this call's buffers
    ent = (NicAdamTensor * 1)(NicAdamTensor(16, 4096, 16, 16, 64, 1, 0.005, 1.0, -1.0, 0, 0, 0))
    tl = NicStepTail()
    tl.tensors, tl.count, tl.n_stream, tl.beta1, tl.beta2, tl.eps = ctypes.cast(ent, ctypes.c_void_p).value, 1, 0, 0.9, 0.999, 1e-8
    assert train(tail=ctypes.byref(tl)) == ARG
    tl.count = 0
    assert train(tail=ctypes.byref(tl)) == ARG
    # the workspace query refuses what the entry points refuse
    assert lib.nic_hash_fused_workspace_bytes(ctypes.byref(_desc(features=3, resolutions=(16,))), mp) == 0
    assert lib.nic_hash_fused_workspace_bytes(dp, ctypes.byref(_mlp(n_linear=5))) == 0
    assert lib.nic_hash_fused_workspace_bytes(None, mp) == 0


def test_supported_set(lib):
    def sup(d, hidden=64, n_linear=3):
        return lib.nic_hash_fused_supported(ctypes.byref(d), hidden, n_linear)

    assert sup(_desc(resolutions=(16,) * 32, features=2)) == OK                        # L F = 64
    assert sup(_desc(resolutions=(16,) * 8, features=8)) == OK
    assert sup(_desc(resolutions=(16,) * 9, features=8)) == UNSUP                      # L F = 72
    assert sup(_desc(resolutions=(16,) * 18, features=4)) == UNSUP
    assert sup(_desc(features=3, resolutions=(16,))) == UNSUP
    for nl in (2, 4, 5):
        assert sup(_desc(), n_linear=nl) == UNSUP
    for h in (32, 63, 128):
        assert sup(_desc(), hidden=h) == UNSUP
    assert sup(_desc(dim=3, extent=(4, 4, 4))) == OK
    # the launching entry points agree (n_linear travels in nic_mlp)
    for nl in (2, 4, 5):
        assert set(_calls(lib, _desc(), _mlp(n_linear=nl))) == {UNSUP}
    assert set(_calls(lib, _desc(resolutions=(16,) * 9, features=8))) == {UNSUP}


def test_python_route_choice_agrees_with_the_c_query(lib):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, hash_fused_supported
    for dim, L, F, hidden, nl in itertools.product((2, 3), (1, 4, 8, 9, 16, 17, 32), (1, 2, 4, 8), (32, 64), (2, 3, 5)):
        geo = HashGeometry((64,) * dim, (16,) * L, F, 12)
        want = lib.nic_hash_fused_supported(ctypes.byref(geo.to_desc(1, [1] * dim)), hidden, nl) == OK
        assert hash_fused_supported(geo, hidden, nl) == want
        assert want == (L * F <= 64 and hidden == 64 and nl == 3), (dim, L, F, hidden, nl)


def test_fused_field_refuses_cpu():
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    with pytest.raises(RuntimeError):
        HashGridField((64, 48), device="cpu", fused=True)
    with pytest.raises(RuntimeError):
        HashGridField((32, 32, 32), levels=4, device=torch.device("cpu"), fused=True)
