"""GPU tests of cell-ordered and fused training at points (nic_hash_point_keys, nic_hash_encode_points_backward_ordered,
nic_hash_fused_forward_backward_points, csrc/hash_points_train.hip; HashGridField.train_points(order=, fused=) / fit_points).

Tolerances are the project's own: TOL_Y = 5e-6 and TOL_G = 1e-4 of the reference's largest magnitude for fused against layer-wise
(tests/test_gpu_hashgrid_fused.py), 1e-5 for the same arithmetic in another order (tests/test_gpu_hashgrid_points.py).

1. keys equal the torch restatement of the header's definition, bit for bit; the order is a permutation that sorts them;
2. the ordered scatter against the unordered one on the same points and gradients, any permutation, short launches, one run;
3. the fused step on a crop's centres ordered patch by patch against the fused crop step;
4. the fused step on random off-lattice points against the layer-wise train_points, with noise and with y;
5. any order computes the same step, with noise, on both routes; y lands at the caller's rows;
6. three accumulate chunks against one call;
7. a frozen table stays bit for bit, and the optimiser tail equals optimizer.step() bit for bit;
8. a refused fused or ordered call leaves a pass in progress alone;
9. fit_points and the scattered-samples fit with order="cell", fused=True reach the yardstick's thresholds;
10. the defaults are today's call."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_Y, TOL_G, TOL_ORDER = 5e-6, 1e-4, 1e-5
NAMES = ["dW1", "db1", "dW2", "db2", "dW3", "db3"]


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


def _geo_for(dim, F=2, log2_table=12):
    """coarse levels dense, fine ones hashed; non-square, not a power of two; a small table"""
    return _geo((200, 131), 8, F, log2_table) if dim == 2 else _geo((40, 27, 33), 8, F, log2_table, n_min=4)


def centres(extent, dev, origin=None):
    origin = [0] * len(extent) if origin is None else origin
    grids = torch.meshgrid(*[torch.arange(int(o), int(o) + int(e), device=dev) for o, e in zip(origin, extent)], indexing="ij")
    return torch.stack([g.reshape(-1) for g in grids], dim=1).to(torch.float32).contiguous()


def _rand_points(geo, dev, seed, n):
    g = torch.Generator(device=dev).manual_seed(seed)
    S = torch.tensor([float(s) for s in geo.field_size], device=dev)
    return (torch.rand(n, geo.dim, generator=g, device=dev) * S - 0.5).contiguous()


def _odd_points(geo, dev, seed, n=3000):
    """random fractional points, then edges, points outside, huge, NaN and infinite coordinates"""
    inside = _rand_points(geo, dev, seed, n)
    rows = []
    for a in range(geo.dim):
        for val in [-0.5, float("nan"), float("inf"), float("-inf"), -3.7, -1e30, 1e30, 0.0, 0.001953125, geo.field_size[a] - 0.5,
                    geo.field_size[a] + 10.25, geo.field_size[a] - 0.5 - 2.0 ** -9, geo.field_size[a] - 1.0]:
            r = inside[len(rows) % n].clone()
            r[a] = val
            rows.append(r)
    rows.append(torch.full((geo.dim,), float("nan"), device=dev))
    rows.append(torch.full((geo.dim,), float("inf"), device=dev))
    rows.append(torch.full((geo.dim,), float("-inf"), device=dev))
    return torch.cat([inside, torch.stack(rows)], dim=0).contiguous()


def _randperm(n, dev, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(dev)


# ---- 1. keys -----------------------------------------------------------------------------------------------------------------------------
def ref_keys(points, field_size):
    """the header's definition in int64: clamp in floating point, t = rint(256 p) + 128 clamped, u = t >> s, bit j of axis a -> bit j dim + a"""
    dim = len(field_size)
    lo = torch.full((dim,), -0.5, dtype=torch.float32, device=points.device)
    hi = torch.tensor([float(s) - 0.5 for s in field_size], dtype=torch.float32, device=points.device)
    p = torch.where(points >= lo, points, lo)
    p = torch.where(p <= hi, p, hi)
    t = torch.round(p * 256.0).to(torch.int64) + 128
    top = torch.tensor([256 * int(s) - 1 for s in field_size], dtype=torch.int64, device=points.device)
    t = torch.minimum(torch.clamp(t, min=0), top)
    b = (256 * max(field_size) - 1).bit_length()
    k = 31 if dim == 2 else 21
    s = max(0, b - k)
    u = t >> s
    key = torch.zeros(points.shape[0], dtype=torch.int64, device=points.device)
    for j in range(k):
        for a in range(dim):
            key |= ((u[:, a] >> j) & 1) << (j * dim + a)
    return key, s


@pytest.mark.parametrize("case", ["2d", "3d", "3d_shifted", "2d_large"])
def test_keys_equal_the_restatement(dev, case):
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd.hashgrid import HashGeometry
    geo = {"2d": lambda: _geo_for(2), "3d": lambda: _geo_for(3), "3d_shifted": lambda: _geo((20000, 300, 17), 4, 2, 12, n_min=4),
           "2d_large": lambda: HashGeometry(((1 << 22) - 1, 77), (4, 16, 64, 200), 2, 12)}[case]()     # the largest S_max the point entries take: b = 30
    pts = _odd_points(geo, dev, seed=len(case))
    keys = hg.hash_point_keys(geo, pts)
    want, s = ref_keys(pts, geo.field_size)
    assert (s > 0) == (case == "3d_shifted"), s                                  # 256 * 20000 - 1 has 23 bits: two are shifted out in 3D
    assert keys.dtype == torch.int64 and keys.shape == (pts.shape[0],)
    assert torch.equal(keys, want), case
    assert int(keys.min()) >= 0
    order = hg.hash_point_order(geo, pts)
    assert order.dtype == torch.int32 and torch.equal(torch.sort(order.long()).values, torch.arange(pts.shape[0], device=dev))
    sk = keys[order.long()]
    assert bool((sk[1:] >= sk[:-1]).all())
    assert torch.equal(hg.hash_point_order(geo, pts), order)                     # deterministic (a stable sort)
    assert hg.hash_point_keys(geo, torch.empty(0, geo.dim, device=dev)).shape == (0,)


# ---- 2. the ordered scatter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_ordered_scatter_is_the_unordered_one(dev, dim, F):
    from neural_image_compression_v2_amd import hashgrid as hg
    for n in (1, 63, 64, 65, 2048 * 256 + 77 if F == 2 else 5003):               # the last: not a multiple of the grid (2048 blocks of 256)
        geo = _geo_for(dim, F)
        if n > 2048 * 256 and dim == 3:
            # the bound is for the ORDER of the sums, not for the depth of an fp32 accumulation: at R = 4 the coarsest 3D level would take
            # 524 k x 8 adds on 125 entries (33 k each, on both sides of the comparison); R = 16 in a 2^14 table keeps it dense at ~ 850 each
            geo = _geo((40, 27, 33), 8, F, 14, n_min=16)
            assert {(r + 1) ** 3 <= (1 << 14) for r in geo.resolutions} == {True, False}
        pts = _odd_points(geo, dev, seed=n % 97, n=n) if n > 100 else _rand_points(geo, dev, n, n)
        n = pts.shape[0]
        g = torch.Generator(device=dev).manual_seed(n % 1000)
        dx = torch.rand(n, geo.width, generator=g, device=dev) * 2 - 1
        base = torch.rand(geo.table_shape(), generator=g, device=dev)            # the call ADDS
        ref = base.clone()
        hg.hash_encode_points_backward(geo, pts, dx, ref)
        for name, order in (("random", _randperm(n, dev, 3)), ("cell", hg.hash_point_order(geo, pts))):
            got = base.clone()
            hg.hash_encode_points_backward(geo, pts, dx, got, order=order)
            e = relmax(got - base, ref - base)
            print(f"ordered scatter {dim}D F={F} N={n} {name}: {e:.3e}")
            assert e <= TOL_ORDER, (dim, F, n, name, e)


@pytest.mark.parametrize("dim", [2, 3])
def test_ordered_scatter_of_coinciding_points_and_of_no_permutation(dev, dim):
    from neural_image_compression_v2_amd import hashgrid as hg
    geo = _geo_for(dim)
    n = 1000
    pts = torch.tensor([17.3, 101.77, 5.5][:dim], device=dev).repeat(n, 1).contiguous()      # every wave is one run
    dx = torch.rand(n, geo.width, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    ref, got = torch.zeros(geo.table_shape(), device=dev), torch.zeros(geo.table_shape(), device=dev)
    hg.hash_encode_points_backward(geo, pts, dx, ref)
    hg.hash_encode_points_backward(geo, pts, dx, got, order=_randperm(n, dev, 9))
    check(got, ref, TOL_ORDER, f"one run {dim}D")
    # a buffer that is no permutation: the sum over the rows it names, indices clamped into the set
    pts = _rand_points(geo, dev, 11, n)
    bad = torch.tensor([0, 0, 5, -7, n + 3, 2 ** 31 - 1, -2 ** 31, 999], dtype=torch.int32, device=dev).repeat(n // 8)
    rows = bad.long().clamp(0, n - 1)
    ref, got = torch.zeros(geo.table_shape(), device=dev), torch.zeros(geo.table_shape(), device=dev)
    hg.hash_encode_points_backward(geo, pts[rows].contiguous(), dx[rows].contiguous(), ref)
    hg.hash_encode_points_backward(geo, pts, dx, got, order=bad)
    check(got, ref, TOL_ORDER, f"no permutation {dim}D")


# ---- fields --------------------------------------------------------------------------------------------------------------------------------
def _field(size, dev, seed, fused=False, num_bits=None, **kw):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    kw = dict(dict(levels=8, features=2, log2_table=12), **kw)
    f = HashGridField(size, device=dev, seed=seed, num_bits=num_bits, fused=fused, **kw)
    with torch.no_grad():
        f.table.uniform_(-0.4, 0.4, generator=torch.Generator(device=dev).manual_seed(seed))
        for p in f.decoder.parameters():
            p.mul_(1.5)                       # past torch's init: activations that are not all in GELU's linear part
    return f


def _twin(f, fused=False):
    """a deep copy of a trainable field: its own table, decoder and optimiser state with the same values and step counts, on the asked route"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    g = HashGridField(f.field_size, levels=f.geo.levels, features=f.geo.features, log2_table=f.geo.log2_table, hidden=f.hidden, n_linear=f.n_linear,
                      device=f.device, num_bits=f.num_bits, noise_seed=f.noise_seed)
    assert not f.frozen and g.geo.table_shape() == f.geo.table_shape()
    g.geo = f.geo
    g._set_route(fused)
    with torch.no_grad():
        g.table.copy_(f.table)
    g.decoder.load_state_dict(copy.deepcopy(f.decoder.state_dict()))
    g.optimizer.load_state_dict(copy.deepcopy(f.optimizer.state_dict()))
    g.steps = f.steps
    return g


def _grads_of(f):
    return [f.table.grad.clone()] + [p.grad.clone() for p in f.decoder.linear_params()]


def _compare_grads(got, ref, tol, what):
    """(loss, [table gradient, decoder gradients]) of two fields after a step=False call"""
    check(got[0].reshape(1), ref[0].reshape(1), TOL_Y if tol == TOL_G else tol, f"{what} loss")
    for n, a, b in zip(["table gradient"] + NAMES, got[1], ref[1]):
        check(a, b, tol, f"{what} {n}")


def _image(size, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.3 * torch.sin(7 * x + 3 * y), 0.5 + 0.3 * torch.cos(5 * x * y * 4), 0.5 + 0.2 * torch.sin(13 * y - 2 * x)], dim=-1)
    return (base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1)


SIZES = {2: ((200, 131), {}), 3: ((40, 27, 33), dict(base_resolution=4))}


# ---- 3. a crop's centres, patch by patch, against the fused crop step -------------------------------------------------------------------------
def _patch_order(ext, dev):
    """row indices of a crop's samples in the fused crop kernel's order: patches of 8 x 8 (4 x 4 x 4), the first axis the fastest lane axis"""
    ps = 8 if len(ext) == 2 else 4
    assert all(e % ps == 0 for e in ext)
    rows = torch.arange(int(torch.tensor(ext).prod()), device=dev).reshape(*ext)
    if len(ext) == 2:
        r = rows.reshape(ext[0] // ps, ps, ext[1] // ps, ps).permute(0, 2, 3, 1)                 # patch x, patch y, lane >> 3 = y, lane & 7 = x
    else:
        r = rows.reshape(ext[0] // ps, ps, ext[1] // ps, ps, ext[2] // ps, ps).permute(0, 2, 4, 5, 3, 1)
    return r.reshape(-1).to(torch.int32).contiguous()


@pytest.mark.parametrize("num_bits", [None, 6])
@pytest.mark.parametrize("dim", [2, 3])
def test_fused_points_on_a_crop_is_the_fused_crop_step(dev, dim, num_bits):
    size, kw = SIZES[dim]
    org, ext = ([40, 24], (64, 48)) if dim == 2 else ([8, 4, 12], (16, 12, 8))
    base = _field(size, dev, 3, fused=True, num_bits=num_bits, **kw)
    assert base.route == "fused"
    n = int(torch.tensor(ext).prod())
    target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    a, b = _twin(base, fused=True), _twin(base, fused=True)
    la = a.train_step([org], ext, target, step=False)
    lb = b.train_points(centres(ext, dev, org), target, step=False, order=_patch_order(ext, dev), fused=True)
    _compare_grads((lb, _grads_of(b)), (la, _grads_of(a)), TOL_G, f"crop centres {dim}D bits {num_bits}")
    assert a._pass_samples == b._pass_samples == n and a.steps == b.steps == 0


# ---- 4. random points against the layer-wise route -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_bits", [None, 6])
@pytest.mark.parametrize("dim", [2, 3])
def test_fused_points_against_layerwise_train_points(dev, dim, num_bits):
    from neural_image_compression_v2_amd import fused
    from neural_image_compression_v2_amd import hashgrid as hg
    size, kw = SIZES[dim]
    base = _field(size, dev, 4, num_bits=num_bits, **kw)
    for n in (1, 65, 4099):                                                      # one lane; two waves; a ragged last wave
        pts = _odd_points(base.geo, dev, seed=dim, n=n)[-n:].contiguous() if n > 100 else _rand_points(base.geo, dev, 7, n)
        target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(2), device=dev)
        a, b = _twin(base), _twin(base, fused=True)
        assert a.route == "layerwise" and b.route == "fused"
        la = a.train_points(pts, target, step=False)
        lb = b.train_points(pts, target, step=False, fused=True)
        _compare_grads((lb, _grads_of(b)), (la, _grads_of(a)), TOL_G, f"random points {dim}D bits {num_bits} N={n}")
    # y returned: the functional entry against the layer-wise encode + decoder, with the same noise keys
    quant = None if num_bits is None else (num_bits, 77, 5, 12345)
    params = [p.detach() for p in base.decoder.linear_params()]
    gm = [torch.empty_like(p) for p in params]
    tg = torch.zeros_like(base.table)
    loss, y = hg.hash_fused_forward_backward_points(base.geo, base.table, pts, params, target, gm, table_grad=tg, want_y=True, quant=quant)
    with torch.no_grad():
        want = fused.DecoderFunction.apply(hg.hash_encode_points(base.geo, base.table, pts, quant=quant), *params)
    check(y, want, TOL_Y, f"y {dim}D bits {num_bits}")
    check(loss, ((want - target) ** 2).mean().reshape(1), TOL_Y, f"loss {dim}D bits {num_bits}")


# ---- 5. order invariance, with noise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_route", [False, True])
@pytest.mark.parametrize("dim", [2, 3])
def test_any_order_is_the_same_step(dev, dim, fused_route):
    from neural_image_compression_v2_amd import hashgrid as hg
    size, kw = SIZES[dim]
    base = _field(size, dev, 5, fused=fused_route, num_bits=6, **kw)
    n = 5003
    pts = _odd_points(base.geo, dev, seed=dim + 10, n=n)[-n:].contiguous()
    target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    tol = TOL_G if fused_route else TOL_ORDER
    ref = None
    for name, order in (("none", None), ("cell", "cell"), ("random", _randperm(n, dev, 4))):
        f = _twin(base, fused=fused_route)
        loss = f.train_points(pts, target, step=False, order=order, fused=fused_route)
        got = (loss, _grads_of(f))
        if ref is None:
            ref = got
            clean = _twin(base, fused=fused_route)
            clean.train_points(pts, target, step=False, noise=False, fused=fused_route)
            moved = relmax(clean.table.grad, ref[1][0])
            print(f"noise moves the table gradient by {moved:.3e}")
            assert moved > 20 * TOL_ORDER                                        # the noise is there: without it the step differs visibly
        else:
            _compare_grads(got, ref, tol, f"order {name} {dim}D {'fused' if fused_route else 'layer-wise'}")
    if fused_route:                                                              # y rows land at the caller's rows
        params = [p.detach() for p in base.decoder.linear_params()]
        ys = []
        for order in (None, hg.hash_point_order(base.geo, pts), _randperm(n, dev, 4)):
            gm = [torch.empty_like(p) for p in params]
            _, y = hg.hash_fused_forward_backward_points(base.geo, base.table, pts, params, target, gm, order=order, want_y=True, quant=(6, 7, 0, 100))
            ys.append(y)
        check(ys[1], ys[0], TOL_Y, f"y rows, cell order {dim}D")
        check(ys[2], ys[0], TOL_Y, f"y rows, random order {dim}D")


# ---- 6. accumulate chunks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_three_chunks_against_one_call(dev, dim):
    size, kw = SIZES[dim]
    base = _field(size, dev, 6, fused=True, num_bits=6, **kw)
    n, cut = 4000, [0, 1000, 2048, 4000]
    pts = _rand_points(base.geo, dev, 12, n)
    target = torch.rand(n, 3, generator=torch.Generator(device=dev).manual_seed(4), device=dev)
    one, three = _twin(base, fused=True), _twin(base, fused=True)
    l1 = one.train_points(pts, target, step=False, order="cell", fused=True)
    tot = 0.0
    for k in range(3):
        s = slice(cut[k], cut[k + 1])
        tot = tot + three.train_points(pts[s], target[s], accumulate=k > 0, scale=(cut[k + 1] - cut[k]) / n, step=False, order="cell", fused=True)
    assert three._pass_samples == one._pass_samples == n
    _compare_grads((tot, _grads_of(three)), (l1, _grads_of(one)), TOL_G, f"three chunks {dim}D")


# ---- 7. stepped and frozen -------------------------------------------------------------------------------------------------------------------
def _twin_frozen(f):
    """a deep copy of a frozen field on the fused route"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    g = HashGridField(f.field_size, levels=f.geo.levels, features=f.geo.features, log2_table=f.geo.log2_table, device=f.device, num_bits=f.num_bits,
                      noise_seed=f.noise_seed, fused=True)
    g.geo = f.geo
    g.freeze()
    with torch.no_grad():
        g.table.copy_(f.table)
    g.decoder.load_state_dict(copy.deepcopy(f.decoder.state_dict()))
    g.optimizer.load_state_dict(copy.deepcopy(f.optimizer.state_dict()))
    g.steps = f.steps
    return g


def test_tail_is_optimizer_step_bit_for_bit(dev):
    """one train_points(fused=True) with the optimiser tail against the same call without it followed by optimizer.step().  The decoder's
    gradients are fixed-order sums, so the decoder is compared bit for bit, while the table trains and after freeze(); the table gradient is a
    sum of atomics whose order differs from launch to launch, so the trained table is compared within 1e-5 of the largest update."""
    size, kw = SIZES[2]
    base = _field(size, dev, 7, fused=True, num_bits=6, **kw)
    pts = _rand_points(base.geo, dev, 13, 3000)
    target = torch.rand(3000, 3, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    base.train_points(pts, target, fused=True)                                   # off the first Adam step
    order = torch.sort(torch.rand(3000, generator=torch.Generator(device=dev).manual_seed(1), device=dev)).indices.to(torch.int32)
    for frozen in (False, True):
        if frozen:
            base.freeze()
        a, b = (_twin_frozen(base), _twin_frozen(base)) if frozen else (_twin(base, fused=True), _twin(base, fused=True))
        table = base.table.detach().clone()
        la = a.train_points(pts, target, order="cell" if frozen else order, fused=True)
        lb = b.train_points(pts, target, order="cell" if frozen else order, fused=True, step=False)
        b.optimizer.step()
        torch.cuda.synchronize()
        assert torch.equal(la, lb)
        for pa, pb, p0 in zip(a.decoder.linear_params(), b.decoder.linear_params(), base.decoder.linear_params()):
            assert torch.equal(pa, pb), frozen
            assert not torch.equal(pa, p0)
        if frozen:
            for f in (a, b):
                assert torch.equal(f.table.detach(), table) and f.table.grad is None     # bit for bit; no table gradient is formed
        else:
            upd = float((a.table.detach() - table).abs().max())
            e = float((a.table.detach() - b.table.detach()).abs().max()) / upd
            print(f"tail against optimizer.step(): table {e:.3e} of the largest update {upd:.3e}")
            assert upd > 0 and e <= TOL_ORDER
        assert a.steps == base.steps + 1


def test_frozen_fused_points_trains_the_decoder_alone(dev):
    size, kw = SIZES[3]
    f = _field(size, dev, 8, fused=True, num_bits=6, **kw)
    pts = _rand_points(f.geo, dev, 14, 2500)
    target = torch.rand(2500, 3, generator=torch.Generator(device=dev).manual_seed(6), device=dev)
    f.train_points(pts, target, order="cell", fused=True)
    poison = f.table.grad
    f.freeze()
    poison.fill_(3.25)
    t0, w0 = f.table.detach().clone(), [p.detach().clone() for p in f.decoder.linear_params()]
    f.train_points(pts, target, order="cell", fused=True)
    torch.cuda.synchronize()
    assert f.table.grad is None and bool((poison == 3.25).all()) and torch.equal(f.table.detach(), t0)
    for p, w in zip(f.decoder.linear_params(), w0):
        assert not torch.equal(p.detach(), w)


def test_stepped_fused_points_updates_once(dev):
    size, kw = SIZES[2]
    f = _field(size, dev, 9, fused=True, **kw)
    pts = _rand_points(f.geo, dev, 15, 3000)
    target = torch.rand(3000, 3, generator=torch.Generator(device=dev).manual_seed(7), device=dev)
    before = [p.detach().clone() for p in [f.table, *f.decoder.linear_params()]]
    f.train_points(pts, target, order="cell", fused=True)
    torch.cuda.synchronize()
    for k, (p, b) in enumerate(zip([f.table, *f.decoder.linear_params()], before)):
        lr = 0.01 if k == 0 else 0.005
        assert int(f.optimizer.state[p]["step"].item()) == 1
        move = float((p.detach() - b).abs().max())
        assert 0 < move <= lr * (1 + 1e-5), (k, move)                            # one first Adam step moves an entry by at most lr
    assert bool((f.table.grad == 0).all()) and f.steps == 1
    f.train_step([[0, 0]], (64, 48), torch.rand(64 * 48, 3, device=dev))         # the field goes on training on its crop route
    assert f.steps == 2


# ---- 8. refused calls -------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_pass_alone(dev):
    size = (96, 80)
    image = _image(size, dev, seed=2)
    pts, target = centres(size, dev), image.reshape(-1, 3).contiguous()
    for fused_route in (False, True):
        f = _field(size, dev, 4, fused=fused_route)
        f.train_points(pts[:4000].contiguous(), target[:4000].contiguous(), scale=0.5, step=False, order="cell", fused=fused_route)
        grad = f.table.grad.clone()
        dec = [p.grad.clone() for p in f.decoder.linear_params()]
        assert bool((grad != 0).any()) and f._pass_samples == 4000
        rest, trest = pts[4000:].contiguous(), target[4000:].contiguous()
        n = rest.shape[0]
        with pytest.raises(ValueError):
            f.train_points(rest, target[4001:].contiguous(), order="cell", fused=fused_route)          # one target short
        with pytest.raises(ValueError):
            f.train_points(rest, trest, order=torch.zeros(n, dtype=torch.int64, device=dev), fused=fused_route)
        with pytest.raises(ValueError):
            f.train_points(rest, trest, order=torch.zeros(n - 1, dtype=torch.int32, device=dev), fused=fused_route)
        with pytest.raises(ValueError):
            f.train_points(rest, trest, order=torch.zeros(n, dtype=torch.int32), fused=fused_route)    # on the host
        with pytest.raises(ValueError):
            f.train_points(rest, trest, order="raster", fused=fused_route)
        with pytest.raises(ValueError):
            f.train_points(torch.empty(0, 2, device=dev), torch.empty(0, 3, device=dev), fused=fused_route)
        if not fused_route:
            with pytest.raises(ValueError, match="fused=True"):
                f.train_points(rest, trest, fused=True)
        assert torch.equal(f.table.grad, grad) and f._pass_samples == 4000 and f.steps == 0
        for p, g in zip(f.decoder.linear_params(), dec):
            assert p.grad is not None and torch.equal(p.grad, g)


# ---- 9. fits -----------------------------------------------------------------------------------------------------------------------------------
def test_fused_cell_ordered_train_points_fits_scattered_samples(dev):
    """test_train_points_fits_scattered_samples (tests/test_gpu_hashgrid_points.py) with order="cell", fused=True: its configuration, its thresholds"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (128, 128)
    image = _image(size, dev, seed=5)
    f = HashGridField(size, levels=8, features=2, log2_table=14, device=dev, seed=5, fused=True)
    assert f.route == "fused"
    g = torch.Generator(device=dev).manual_seed(6)
    first = None
    for it in range(200):
        idx = torch.randint(0, size[0] * size[1], (8192,), generator=g, device=dev)
        pts = torch.stack([idx // size[1], idx % size[1]], dim=1).float().contiguous()
        loss = float(f.train_points(pts, image.reshape(-1, 3)[idx].contiguous(), order="cell", fused=True))
        first = loss if first is None else first
    print(f"scattered samples, fused + cell order: first {first:.3e} last {loss:.3e}")
    assert loss < 0.1 * first, (first, loss)
    assert float(((f.decode() - image) ** 2).mean()) < 0.1 * first


@pytest.mark.parametrize("fused_route", [False, True])
def test_fit_points_on_a_masked_image(dev, fused_route):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (128, 128)
    image = _image(size, dev, seed=5)
    f = HashGridField(size, levels=8, features=2, log2_table=14, device=dev, seed=5, fused=fused_route)
    g = torch.Generator(device=dev).manual_seed(8)
    keep = torch.nonzero(torch.rand(size[0] * size[1], generator=g, device=dev) < 0.5).reshape(-1)      # a 50 % random mask
    pts = torch.stack([keep // size[1], keep % size[1]], dim=1).float().contiguous()
    hist = f.fit_points(pts, image.reshape(-1, 3)[keep].contiguous(), epochs=200, batch=3000)
    print(f"fit_points {'fused' if fused_route else 'layer-wise'}: first {hist[0]:.3e} last {hist[-1]:.3e}")
    assert len(hist) == 200 and f.steps == 200
    assert hist[-1] < 0.1 * hist[0], (hist[0], hist[-1])
    assert float(((f.decode() - image) ** 2).mean()) < 0.1 * hist[0]


# ---- 10. the defaults are today's call ---------------------------------------------------------------------------------------------------------
def test_defaults_are_untouched(dev):
    size, kw = SIZES[2]
    base = _field(size, dev, 10, fused=True, num_bits=6, **kw)
    pts = _rand_points(base.geo, dev, 16, 3000)
    target = torch.rand(3000, 3, generator=torch.Generator(device=dev).manual_seed(9), device=dev)
    base.train_points(pts, target)
    a, b = _twin(base, fused=True), _twin(base, fused=True)
    a.freeze()
    b.freeze()
    la = a.train_points(pts, target)
    lb = b.train_points(pts, target, order=None, fused=False)
    assert torch.equal(la, lb) and torch.equal(a.table.detach(), b.table.detach()) and a.table.grad is None and b.table.grad is None
    for pa, pb in zip(a.decoder.linear_params(), b.decoder.linear_params()):
        assert torch.equal(pa, pb)                                               # no atomics on this path: the same launches
