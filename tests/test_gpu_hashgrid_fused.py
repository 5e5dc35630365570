"""GPU tests of the fused hash-grid encode + decoder kernels (nic_hash_fused_*, csrc/hash_fused.hip; HashGridField(fused=True)).

The yardstick is the LAYER-WISE route on the same device - hash_encode / hash_encode_noisy / hash_encode_u8 -> fused.DecoderFunction -> MSE ->
hash_encode_backward - which tests/test_gpu_hashgrid.py pins to a float64 torch restatement; it is not the code under test.  Tolerances are the
package's for fp32 against fp32 with another summation order (error over the largest magnitude of the reference tensor): y and loss 5e-6, the
table gradient and every decoder gradient 1e-4."""
import ctypes
import subprocess
import sys
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_Y, TOL_G = 5e-6, 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def check(a, b, tol, what):
    e = relmax(a, b)
    print(f"{what}: {e:.3e}")
    assert e <= tol, f"{what}: max error over the reference's largest magnitude {e:.3e} > {tol:.1e}"


def _geo(field_size, levels, F, log2_table, n_min=16):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(tuple(field_size), tuple(level_resolutions(levels, n_min, max(field_size))), F, log2_table)


def _decoder(geo, dev, seed):
    from neural_image_compression_v2_amd.image_compression import ColorDecoder
    torch.manual_seed(seed)
    dec = ColorDecoder(geo.width, 64, 3).to(dev)
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(1.5)                       # past torch's init: activations that are not all in GELU's linear part
    return [p.detach().clone() for p in dec.linear_params()]


def _table(geo, dev, seed, mag=0.3):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand(geo.table_shape(), generator=g, device=dev) * 2 - 1) * mag


def _layerwise(geo, table, origins, extent, params, target, scale=1.0, quant=None, stored=None, frozen=False):
    """y, loss, table gradient, decoder gradients of the layer-wise route"""
    from neural_image_compression_v2_amd import fused
    from neural_image_compression_v2_amd.hashgrid import hash_encode, hash_encode_backward, hash_encode_noisy, hash_encode_u8
    org = geo.upload_origins(origins, extent, table.device)
    if stored is not None:
        x = hash_encode_u8(geo, stored, org, extent, quant)
    elif quant is not None:
        x = hash_encode_noisy(geo, table, org, extent, *quant)
    else:
        x = hash_encode(geo, table, org, extent)
    if target is None:
        return fused.DecoderFunction.apply(x, *params), None, None, None
    x.requires_grad_(not frozen)
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    y = fused.DecoderFunction.apply(x, *ps)
    loss = ((y - target) ** 2).mean() * scale
    loss.backward()
    tg = None
    if not frozen:
        tg = torch.zeros_like(table)
        hash_encode_backward(geo, org, extent, x.grad, tg)
    return y.detach(), loss.detach(), tg, [p.grad for p in ps]


def _fused(geo, table, origins, extent, params, target, scale=1.0, quant=None, frozen=False, **kw):
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_backward
    gm = [torch.full_like(p, 7.0) for p in params]
    tg = None if frozen else torch.zeros_like(table)
    loss, y = hash_fused_forward_backward(geo, table, origins, extent, params, target, gm, table_grad=tg, loss_scale=scale, want_y=True, quant=quant, **kw)
    return y, loss[0], tg, gm


NAMES = ["dW1", "db1", "dW2", "db2", "dW3", "db3"]


def _compare(got, ref, what):
    check(got[0], ref[0], TOL_Y, f"{what} y")
    check(got[1].reshape(1), ref[1].reshape(1), TOL_Y, f"{what} loss")
    if ref[2] is not None:
        check(got[2], ref[2], TOL_G, f"{what} table gradient")
    for n, a, b in zip(NAMES, got[3], ref[3]):
        check(a, b, TOL_G, f"{what} {n}")


CASES_2D = [(1, 8, 10), (1, 32, 12), (2, 4, 11), (2, 16, 12), (2, 32, 12), (4, 2, 10), (4, 8, 12), (4, 16, 11), (8, 1, 10), (8, 4, 12), (8, 8, 11), (2, 16, 19)]
CASES_3D = [(1, 16, 12), (2, 8, 10), (2, 32, 12), (4, 4, 11), (8, 2, 12), (8, 8, 10), (2, 16, 19)]


# ---- 1. forward and forward-backward parity
@pytest.mark.parametrize("F,levels,log2_table", CASES_2D)
def test_parity_2d(dev, F, levels, log2_table):
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward
    size, extent = (200, 150), (37, 29)
    geo = _geo(size, levels, F, log2_table)
    origins = [[0, 0], [size[0] - extent[0], size[1] - extent[1]], [size[0] - extent[0], 3], [11, size[1] - extent[1]]]
    table, params = _table(geo, dev, 1), _decoder(geo, dev, 2)
    n = len(origins) * extent[0] * extent[1]
    target = torch.rand(n, 3, device=dev)
    ref = _layerwise(geo, table, origins, extent, params, target)
    _compare(_fused(geo, table, origins, extent, params, target), ref, f"2D F{F} L{levels} T{log2_table}")
    check(hash_fused_forward(geo, table, origins, extent, params), ref[0], TOL_Y, "forward y")
    # a single-sample crop
    one = [[size[0] - 1, size[1] - 1]]
    t1 = torch.rand(1, 3, device=dev)
    _compare(_fused(geo, table, one, (1, 1), params, t1), _layerwise(geo, table, one, (1, 1), params, t1), "single sample")


@pytest.mark.parametrize("F,levels,log2_table", CASES_3D)
def test_parity_3d(dev, F, levels, log2_table):
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward
    size, extent = (40, 33, 29), (9, 6, 5)
    geo = _geo(size, levels, F, log2_table, n_min=4)
    origins = [[0, 0, 0], [size[0] - extent[0], size[1] - extent[1], size[2] - extent[2]], [5, size[1] - extent[1], 2], [size[0] - extent[0], 1, size[2] - extent[2]]]
    table, params = _table(geo, dev, 3), _decoder(geo, dev, 4)
    n = len(origins) * extent[0] * extent[1] * extent[2]
    target = torch.rand(n, 3, device=dev)
    ref = _layerwise(geo, table, origins, extent, params, target)
    _compare(_fused(geo, table, origins, extent, params, target), ref, f"3D F{F} L{levels} T{log2_table}")
    check(hash_fused_forward(geo, table, origins, extent, params), ref[0], TOL_Y, "forward y")
    one = [[size[0] - 1, size[1] - 1, size[2] - 1]]
    t1 = torch.rand(1, 3, device=dev)
    _compare(_fused(geo, table, one, (1, 1, 1), params, t1), _layerwise(geo, table, one, (1, 1, 1), params, t1), "single sample")


# ---- 2. noise
@pytest.mark.parametrize("num_bits", [4, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_noise_is_hash_encode_noisys(dev, num_bits, dim):
    if dim == 2:
        size, extent, origins, geo = (200, 150), (37, 29), [[3, 5], [163, 121]], _geo((200, 150), 16, 2, 12)
    else:
        size, extent, origins, geo = (40, 33, 29), (9, 6, 5), [[1, 2, 3], [31, 27, 24]], _geo((40, 33, 29), 8, 4, 11, n_min=4)
    table, params = _table(geo, dev, 5), _decoder(geo, dev, 6)
    n = len(origins)
    for e in extent:
        n *= e
    target = torch.rand(n, 3, device=dev)
    quant = (num_bits, 0x1234_5678_9ABC, 77, 123_457)
    ref = _layerwise(geo, table, origins, extent, params, target, quant=quant)
    _compare(_fused(geo, table, origins, extent, params, target, quant=quant), ref, f"noisy b{num_bits} {dim}D")
    # the noise matters at this tolerance, and two chunks of one pass (another sample_base) do not share it
    clean = _layerwise(geo, table, origins, extent, params, target)
    assert relmax(ref[0], clean[0]) > 20 * TOL_Y                      # (b = 8: 2^-8 on every column moves y by ~4e-4)
    other = _fused(geo, table, origins, extent, params, target, quant=(num_bits, quant[1], quant[2], quant[3] + n))
    assert relmax(other[0], ref[0]) > 20 * TOL_Y
    check(other[0], _layerwise(geo, table, origins, extent, params, None, quant=(num_bits, quant[1], quant[2], quant[3] + n))[0], TOL_Y, "next chunk y")


def test_field_chunks_draw_their_own_noise(dev, monkeypatch):
    """the fused field hands (offset = optimiser step, sample_base = samples of the pass so far) to the kernel, like the layer-wise one"""
    from neural_image_compression_v2_amd import hashgrid
    size, chunk = (64, 40), 32
    field = hashgrid.HashGridField(size, levels=6, features=2, log2_table=12, device=dev, seed=2, num_bits=8, fused=True)
    assert field.route == "fused"
    seen, real = [], hashgrid.hash_fused_forward_backward

    def spy(*a, **kw):
        seen.append(kw["quant"])
        return real(*a, **kw)

    monkeypatch.setattr(hashgrid, "hash_fused_forward_backward", spy)
    image = torch.rand(*size, 3, device=dev)
    for _ in range(2):
        for k, x0 in enumerate((0, chunk)):
            field.train_step([[x0, 0]], (chunk, size[1]), image[x0:x0 + chunk].reshape(-1, 3).contiguous(), accumulate=k > 0, scale=0.5, step=k == 1)
    n = chunk * size[1]
    assert seen == [(8, 7, 0, 0), (8, 7, 0, n), (8, 7, 1, 0), (8, 7, 1, n)]


# ---- 3. uint8 decode
@pytest.mark.parametrize("num_bits", [2, 4, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_u8_decode(dev, num_bits, dim):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward, hash_fused_forward_u8, hash_pack_u8
    if dim == 2:
        extent, origins, geo = (37, 29), [[3, 5], [163, 121]], _geo((200, 150), 16, 2, 12)
    else:
        extent, origins, geo = (9, 6, 5), [[1, 2, 3], [31, 27, 24]], _geo((40, 33, 29), 8, 4, 11, n_min=4)
    table, params = models.quantize_clamp(_table(geo, dev, 7, mag=0.5), num_bits), _decoder(geo, dev, 8)
    stored = hash_pack_u8(geo, table, num_bits)
    y = hash_fused_forward_u8(geo, stored, origins, extent, num_bits, params)
    check(y, _layerwise(geo, table, origins, extent, params, None, quant=num_bits, stored=stored)[0], TOL_Y, f"u8 b{num_bits} y")
    # load4fp(save4fp(table)) through the fp32 kernel: the same rows into the same decoder code
    deq = models.load4fp(models.save4fp(table, num_bits), num_bits)
    assert torch.equal(y, hash_fused_forward(geo, deq, origins, extent, params))


# ---- 4. frozen table
def test_frozen_table_issues_no_scatter(dev):
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_backward
    geo = _geo((200, 150), 16, 2, 12)
    origins, extent = [[3, 5], [163, 121]], (37, 29)
    table, params = _table(geo, dev, 9), _decoder(geo, dev, 10)
    target = torch.rand(2 * 37 * 29, 3, device=dev)
    ref = _layerwise(geo, table, origins, extent, params, target, frozen=True)
    got = _fused(geo, table, origins, extent, params, target, frozen=True)
    _compare(got, ref, "frozen")
    assert got[2] is None
    # the field: after freeze() the fused step gives the kernel no table gradient - a poisoned buffer of the table's shape, kept beside
    # the field, and the table itself stay as they are while the decoder trains
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    f = HashGridField((128, 96), levels=8, features=2, log2_table=12, device=dev, seed=5, num_bits=8, fused=True)
    f.train_step([[0, 0]], (64, 48), torch.rand(64 * 48, 3, device=dev))
    poison = f.table.grad
    f.freeze()
    poison.fill_(3.25)
    t0, w0 = f.table.detach().clone(), f.decoder.linear_params()[0].detach().clone()
    f.train_step([[0, 0]], (64, 48), torch.rand(64 * 48, 3, device=dev))
    torch.cuda.synchronize()
    assert f.table.grad is None and bool((poison == 3.25).all()) and torch.equal(f.table.detach(), t0)
    assert not torch.equal(f.decoder.linear_params()[0].detach(), w0)

# ---- 5. chunked pass
def test_chunked_pass_adds_up(dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, chunk = (128, 96), 32
    image = torch.rand(*size, 3, device=dev)
    field = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=4, fused=True)
    with torch.no_grad():
        field.table.copy_(_table(field.geo, dev, 11))
    params = [p.detach().clone() for p in field.decoder.linear_params()]
    table = field.table.detach().clone()
    ref = _layerwise(field.geo, table, [[0, 0]], size, params, image.reshape(-1, 3))
    starts = list(range(0, size[0], chunk))
    steps0 = [int(field.optimizer.state[p]["step"].item()) if field.optimizer.state[p] else 0 for p in [field.table]]
    tot = 0.0
    for k, x0 in enumerate(starts[:-1]):
        tot = tot + field.train_step([[x0, 0]], (chunk, size[1]), image[x0:x0 + chunk].reshape(-1, 3).contiguous(), accumulate=k > 0, scale=1 / len(starts), step=False)
    # the last chunk without the optimiser, to read the sums; then the step itself
    tot = tot + field.train_step([[starts[-1], 0]], (chunk, size[1]), image[starts[-1]:].reshape(-1, 3).contiguous(), accumulate=True, scale=1 / len(starts), step=False)
    check(tot.reshape(1), ref[1].reshape(1), TOL_Y, "chunked loss")
    check(field.table.grad, ref[2], TOL_G, "chunked table gradient")
    for n, p, b in zip(NAMES, field.decoder.linear_params(), ref[3]):
        check(p.grad, b, TOL_G, f"chunked {n}")
    assert torch.equal(field.table.detach(), table)
    # a whole pass with the step on the last chunk: one optimiser step
    field2 = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=4, fused=True)
    for k, x0 in enumerate(starts):
        field2.train_step([[x0, 0]], (chunk, size[1]), image[x0:x0 + chunk].reshape(-1, 3).contiguous(), accumulate=k > 0, scale=1 / len(starts), step=k == len(starts) - 1)
    assert field2.steps == 1 and steps0 == [0]
    for p in [field2.table, *field2.decoder.linear_params()]:
        assert int(field2.optimizer.state[p]["step"].item()) == 1
    assert bool((field2.table.grad == 0).all())


# ---- 6. the optimiser tail
def _adam_entries(_lib, tensors, grads, states, lrs, zero_first):
    ent = []
    for i, (p, g, (m, v), lr) in enumerate(zip(tensors, grads, states, lrs)):
        ent.append(_lib.NicAdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 1, lr, 1.0, -1.0, 0, 0,
                                      _lib.NIC_ADAM_ZERO_GRAD if (zero_first and i == 0) else 0))
    return (_lib.NicAdamTensor * len(ent))(*ent)


@pytest.mark.parametrize("zero", [False, True])
def test_tail_equals_adam_multi_on_the_same_gradients(dev, zero):
    from neural_image_compression_v2_amd import _lib, fused
    lib = _lib.load()
    geo = _geo((200, 150), 16, 2, 12)
    origins, extent = [[3, 5], [163, 121]], (37, 29)
    table, params = _table(geo, dev, 12), _decoder(geo, dev, 13)
    target = torch.rand(2 * 37 * 29, 3, device=dev)
    tensors = [table, *params]
    g2 = torch.Generator(device=dev).manual_seed(14)
    states = [(torch.rand(t.shape, generator=g2, device=dev) * 1e-3, torch.rand(t.shape, generator=g2, device=dev) * 1e-6) for t in tensors]
    copies = [t.clone() for t in tensors]
    cstates = [(m.clone(), v.clone()) for m, v in states]
    tg, gm = torch.zeros_like(table), [torch.empty_like(p) for p in params]
    lrs = [0.01] + [0.005] * 6
    arr = _adam_entries(_lib, tensors, [tg, *gm], states, lrs, zero)
    tail = _lib.NicStepTail()
    tail.tensors, tail.count, tail.n_stream, tail.beta1, tail.beta2, tail.eps = ctypes.cast(arr, ctypes.c_void_p).value, 7, 1, 0.9, 0.999, 1e-8
    d = geo.to_desc(2, extent)
    org = geo.upload_origins(origins, extent, dev)
    m, gs = fused._mlp_struct(params), fused._grads_struct(gm)
    loss = torch.empty(1, device=dev)
    ws = _lib.workspace(dev, int(lib.nic_hash_fused_workspace_bytes(ctypes.byref(d), ctypes.byref(m))))
    _lib.check(lib.nic_hash_fused_forward_backward(ctypes.byref(d), None, _lib.ptr(table), _lib.ptr(org), ctypes.byref(m), _lib.ptr(target), 1.0, _lib.ptr(tg),
                                                   ctypes.byref(gs), _lib.ptr(loss), None, 0, _lib.ptr(ws), ws.numel(), ctypes.byref(tail), _lib.stream_ptr(dev)), "fused")
    torch.cuda.synchronize()
    if zero:
        assert bool((tg == 0).all())
        assert not torch.equal(table, copies[0])                       # the update happened
        return
    assert float(tg.abs().max()) > 0
    arr2 = _adam_entries(_lib, copies, [tg, *gm], cstates, lrs, False)
    _lib.check(lib.nic_adam_multi(arr2, 7, 0.9, 0.999, 1e-8, _lib.stream_ptr(dev)), "adam")
    torch.cuda.synchronize()
    for a, b in zip(tensors, copies):
        assert torch.equal(a, b)
    for (m1, v1), (m2, v2) in zip(states, cstates):
        assert torch.equal(m1, m2) and torch.equal(v1, v2)


def test_step_with_tail_updates_once(dev):
    """train_step's own optimizer.step() after a committed tail launches nothing: every step count is 1, and no entry moved further than one
    first Adam step can move it (|update| = lr |g| / (|g| + eps) <= lr; a second update on the same gradients would move the output bias,
    whose gradients are far above eps, by nearly 2 lr)"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, extent = (128, 96), (64, 48)
    target = torch.rand(64 * 48, 3, device=dev)
    f = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=5, fused=True)
    before = [p.detach().clone() for p in [f.table, *f.decoder.linear_params()]]
    f.train_step([[0, 0]], extent, target)
    torch.cuda.synchronize()
    for k, (p, b) in enumerate(zip([f.table, *f.decoder.linear_params()], before)):
        lr = 0.01 if k == 0 else 0.005
        assert int(f.optimizer.state[p]["step"].item()) == 1
        move = float((p.detach() - b).abs().max())
        assert 0 < move <= lr * (1 + 1e-5), (k, move)
        if k == 6:                                                       # the output bias: gradients far above eps, its entries move by lr
            assert move > 0.9 * lr, move
    assert bool((f.table.grad == 0).all()) and f.steps == 1


# ---- 7. nic_mark_kernel_end
def test_kernel_end_event_recorded_and_dropped(dev):
    from neural_image_compression_v2_amd import _lib, fused
    lib, hip = _lib.load(), ctypes.CDLL("libamdhip64.so")
    geo = _geo((200, 150), 16, 2, 12)
    origins, extent = [[3, 5]], (37, 29)
    table, params = _table(geo, dev, 15), _decoder(geo, dev, 16)
    target = torch.rand(37 * 29, 3, device=dev)
    ev = [ctypes.c_void_p() for _ in range(3)]
    for e in ev:
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
    try:
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        assert hip.hipEventRecord(ev[0], stream) == 0
        assert lib.nic_mark_kernel_end(ev[1]) == 0
        _fused(geo, table, origins, extent, params, target)
        torch.cuda.synchronize()
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[1]) == 0 and ms.value >= 0     # recorded by the successful call
        # a refused call drops it
        assert lib.nic_mark_kernel_end(ev[2]) == 0
        d = geo.to_desc(1, extent)
        m, gs = fused._mlp_struct(params), fused._grads_struct([torch.empty_like(p) for p in params])
        fake = ctypes.c_void_p(16)
        rc = lib.nic_hash_fused_forward_backward(ctypes.byref(d), None, fake, fake, ctypes.byref(m), fake, 1.0, None, ctypes.byref(gs), fake, None, 0, fake, 16,
                                                 None, _lib.stream_ptr(dev))
        assert rc == -4
        _fused(geo, table, origins, extent, params, target)
        torch.cuda.synchronize()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), ev[0], ev[2]) != 0, "the parked end event was recorded by a later call"
        hip.hipGetLastError()
    finally:
        lib.nic_mark_kernel_end(None)
        for e in ev:
            hip.hipEventDestroy(e)


# ---- 8. host loop
def _image(size, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.3 * torch.sin(7 * x + 3 * y), 0.5 + 0.3 * torch.cos(5 * x * y * 4), 0.5 + 0.2 * torch.sin(13 * y - 2 * x)], dim=-1)
    return (base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1)


def test_host_loop_matches_layerwise_field(dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, extent = (256, 192), (64, 48)
    image = _image(size, dev)
    g = torch.Generator().manual_seed(9)
    crops = [torch.stack([torch.randint(0, size[0] - extent[0] + 1, (4,), generator=g), torch.randint(0, size[1] - extent[1] + 1, (4,), generator=g)], 1)
             for _ in range(20)]
    grids = torch.meshgrid(torch.arange(extent[0], device=dev), torch.arange(extent[1], device=dev), indexing="ij")
    local = torch.stack([t.reshape(-1) for t in grids], 1)
    out = {}
    for fused_route in (False, True):
        field = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=3, fused=fused_route)
        assert field.route == ("fused" if fused_route else "layerwise")
        losses = []
        for k in range(20):
            i = (crops[k].to(dev)[:, None, :] + local[None]).reshape(-1, 2)
            losses.append(float(field.train_step(crops[k], extent, image[i[:, 0], i[:, 1]])))
        out[fused_route] = (losses, field.decode())
    for k, (a, b) in enumerate(zip(out[True][0], out[False][0])):
        assert abs(a - b) <= 1e-3 * abs(b), (k, a, b)
    assert float((out[True][1] - out[False][1]).abs().max()) < 2e-3


# ---- 9. fit quality
def test_fit_quality_2d_chunked_passes_fused(dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (256, 256)
    image = _image(size, dev, seed=1)
    field = HashGridField(size, device=dev, seed=1, fused=True)
    field.set_schedule(300)
    hist = field.fit(image, 300, chunk=64)
    assert hist[-1] < 0.05 * hist[0], (hist[0], hist[-1])
    assert float(((field.decode(tile=100) - image) ** 2).mean()) < 0.05 * hist[0]


def test_fit_quality_3d_volume_fused(dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    n = 64
    ax = torch.linspace(0, 1, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.stack([0.5 + 0.3 * torch.sin(6 * x + 2 * z), 0.5 + 0.3 * torch.cos(4 * y - 3 * z), 0.5 + 0.25 * torch.sin(5 * (x + y + z))], dim=-1)
    target = vol.reshape(-1, 3).contiguous()
    field = HashGridField((n, n, n), levels=8, features=2, log2_table=16, base_resolution=4, device=dev, seed=2, fused=True)
    hist = [float(field.train_step([[0, 0, 0]], (n, n, n), target)) for _ in range(150)]
    assert hist[-1] < 0.1 * hist[0], (hist[0], hist[-1])
    assert float(((field.decode(tile=40) - vol) ** 2).mean()) < 0.1 * hist[0]


def _structured_image(size, dev):
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.25 * torch.sin(7 * x + 3 * y) + 0.15 * torch.sin(41 * x) * torch.cos(37 * y),
                        0.5 + 0.25 * torch.cos(20 * x * y) + 0.15 * torch.sin(60 * (x - y) ** 2),
                        0.5 + 0.2 * torch.sin(13 * y - 2 * x) + 0.1 * torch.sign(torch.sin(9 * x + 11 * y))], dim=-1)
    return base.clamp(0, 1)


def _psnr(a, b):
    return float(-10 * torch.log10(((a - b) ** 2).mean()))


def test_fit_quality_2d_qat_fused(dev, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, epochs = (256, 256), 300
    image = _structured_image(size, dev)
    kw = dict(levels=8, features=2, log2_table=12, device=dev, seed=1, fused=True)
    fp = HashGridField(size, **kw)
    fp.set_schedule(epochs)
    fp.fit(image, epochs)
    p_fp = _psnr(fp.decode(), image)
    q = HashGridField(size, num_bits=8, **kw)
    q.set_schedule(epochs)
    q.fit(image, epochs)
    assert q.frozen
    q.save_compressed(tmp_path / "q8.pt")
    p_q = _psnr(HashGridField.load_compressed(tmp_path / "q8.pt", dev, fused=True).decode(), image)
    print(f"2D PSNR fused: fp32 {p_fp:.2f} dB, QAT b=8 stored {p_q:.2f}")
    assert p_q >= p_fp - 1.0, (p_fp, p_q)


# ---- 10. stored file
def test_stored_file_decodes_the_same_in_a_fresh_process(dev, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (96, 80)
    image = _image(size, dev, seed=2)
    field = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=6, num_bits=6, fused=True)
    field.fit(image, 20, chunk=48, freeze_at=0.5)
    assert field.frozen and field.route == "fused"
    want = field.decode()
    path, out = tmp_path / "f.pt", tmp_path / "decoded.pt"
    field.save_compressed(path)
    torch.save(want.cpu(), tmp_path / "want.pt")
    code = ("import sys, torch\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from neural_image_compression_v2_amd.hashgrid import HashGridField\n"
            f"f = HashGridField.load_compressed({str(path)!r}, 'cuda:0', fused=True)\n"
            "assert f.route == 'fused'\n"
            f"torch.save(f.decode().cpu(), {str(out)!r})\n")
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)
    assert torch.equal(torch.load(out), want.cpu())


# ---- 11. the 4K bench shape
def test_4k_launch(dev):
    size = (3840, 2160)
    geo = _geo(size, 16, 2, 19)
    table, params = _table(geo, dev, 17), _decoder(geo, dev, 18)
    target = torch.rand(size[0] * size[1], 3, device=dev)
    ref = _layerwise(geo, table, [[0, 0]], size, params, target)
    _compare(_fused(geo, table, [[0, 0]], size, params, target), ref, "4K")


# ---- 12. the default is untouched
def test_default_field_calls_none_of_the_new_entry_points(dev, monkeypatch):
    from neural_image_compression_v2_amd import _lib
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    lib = _lib.load()

    def boom(*a, **kw):
        raise AssertionError("a fused hash-grid entry point was called by a field built without fused=True")

    for name in ("nic_hash_fused_supported", "nic_hash_fused_workspace_bytes", "nic_hash_fused_forward", "nic_hash_fused_forward_u8",
                 "nic_hash_fused_forward_backward"):
        monkeypatch.setattr(lib, name, boom, raising=True)
    field = HashGridField((64, 48), levels=4, features=2, log2_table=10, device=dev, seed=1)
    assert field.route == "layerwise"
    field.train_step([[0, 0]], (64, 48), torch.rand(64 * 48, 3, device=dev))
    assert field.decode().shape == (64, 48, 3)


def test_unsupported_shape_takes_the_layerwise_route(dev):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    field = HashGridField((64, 48), levels=9, features=8, log2_table=10, device=dev, seed=1, fused=True)      # L F = 72
    assert field.route == "layerwise"
    field.train_step([[0, 0]], (64, 48), torch.rand(64 * 48, 3, device=dev))
    assert HashGridField((64, 48), levels=4, device=dev, n_linear=5, fused=True).route == "layerwise"
