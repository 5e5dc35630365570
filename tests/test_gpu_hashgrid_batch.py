"""GPU tests of the batched hash-grid kernels (nic_hash_batch_*, csrc/hashgrid_batch.hip; HashGridFieldBatch).

The yardstick is always the existing SINGLE-field entries - hash_fused_forward / hash_fused_forward_backward, which tests/test_gpu_hashgrid_fused.py
pins to the layer-wise route - called once per field on slices of the same stacked tensors; it is never the code under test.  Tolerances are that
file's for fp32 against fp32 with another summation order (error over the largest magnitude of the reference tensor): y and loss 5e-6, the table
gradient and every decoder gradient 1e-4.  Initial values are large (tables +-0.6, the decoder twice nn.Linear's init) and differ per field, so a
swapped or shared field cannot pass; shapes are the smallest at which each thing can go wrong (patch rims, two crops, more workgroups than groups
of patches, more workgroups than CUs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_Y, TOL_G = 5e-6, 1e-4
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


def _stacked(geo, dev, B, seed):
    """tables [B, L, T, F] in +-0.6 and the six stacked decoder tensors at twice nn.Linear's init, every field its own values"""
    from neural_image_compression_v2_amd.image_compression import ColorDecoder
    g = torch.Generator(device=dev).manual_seed(seed)
    tables = (torch.rand(B, *geo.table_shape(), generator=g, device=dev) * 2 - 1) * 0.6
    torch.manual_seed(seed + 1)
    decs = [ColorDecoder(geo.width, 64, 3).linear_params() for _ in range(B)]
    params = [(2.0 * torch.stack([d[k].detach() for d in decs])).to(dev).contiguous() for k in range(6)]
    return tables, params


def _origins(geo, extent, B, num_crops, dev, seed):
    """[B, num_crops, dim] int32 on the device, every field its own crops, all inside the field"""
    g = torch.Generator().manual_seed(seed)
    o = torch.stack([torch.randint(0, s - e + 1, (B, num_crops), generator=g) for s, e in zip(geo.field_size, extent)], dim=-1)
    return o.to(torch.int32).to(dev)


def _n(num_crops, extent):
    n = num_crops
    for e in extent:
        n *= e
    return n


def _singles(geo, tables, org, extent, params, target, scale=1.0, quant=None, frozen=False, **kw):
    """the reference: one hash_fused_forward_backward per field on slices of the stacked tensors -> per field (y, loss, table gradient, gm)"""
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_backward
    out = []
    for b in range(tables.shape[0]):
        ps = [p[b] for p in params]
        gm = [torch.full_like(p, 7.0) for p in ps]
        tg = None if frozen else torch.zeros_like(tables[b])
        loss, y = hash_fused_forward_backward(geo, tables[b], org[b], extent, ps, target[b], gm, table_grad=tg, loss_scale=scale, want_y=True, quant=quant, **kw)
        out.append((y, loss[0], tg, gm))
    return out


def _batch(geo, tables, org, extent, params, target, scale=1.0, quant=None, frozen=False, want_y=True, **kw):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_backward
    gm = [torch.full_like(p, 7.0) for p in params]
    tg = None if frozen else torch.zeros_like(tables)
    loss, y = hash_batch_forward_backward(geo, tables, org, extent, params, target, gm, table_grads=tg, loss_scale=scale, want_y=want_y, quant=quant, **kw)
    return y, loss, tg, gm


def _compare(got, refs, what):
    y, loss, tg, gm = got
    for b, ref in enumerate(refs):
        if y is not None:
            check(y[b], ref[0], TOL_Y, f"{what} field {b} y")
        check(loss[b].reshape(1), ref[1].reshape(1), TOL_Y, f"{what} field {b} loss")
        if ref[2] is not None:
            check(tg[b], ref[2], TOL_G, f"{what} field {b} table gradient")
        for n, a, r in zip(NAMES, gm, ref[3]):
            check(a[b], r, TOL_G, f"{what} field {b} {n}")


# field size, levels, F, log2_table, n_min, crop extent, crops, B
CASES = {
    "2d_kt1": ((40, 36), 4, 2, 10, 16, (20, 12), 2, 3),          # patch rims on both axes, two crops, L F = 8
    "2d_kt2": ((40, 36), 12, 4, 10, 16, (20, 12), 2, 3),         # L F = 48: the two-tile dW1 / dX path
    "3d_f1": ((12, 10, 9), 4, 1, 10, 4, (7, 10, 5), 2, 3),       # 4 x 4 x 4 patches with rims, F = 1
    "single": ((40, 36), 4, 2, 10, 16, (20, 12), 2, 1),          # B = 1
    "split": ((40, 36), 4, 2, 10, 16, (40, 36), 3, 3),           # 75 patches = 19 groups of four: persistent grid 24
}
_cache = {}


def _case(name, dev):
    """the inputs of a case and the single-field reference, computed once per module and left unchanged"""
    if name not in _cache:
        size, levels, F, log2_table, n_min, extent, crops, B = CASES[name]
        geo = _geo(size, levels, F, log2_table, n_min)
        k = list(CASES).index(name)
        tables, params = _stacked(geo, dev, B, 100 + k)
        org = _origins(geo, extent, B, crops, dev, 200 + k)
        target = torch.rand(B, _n(crops, extent), 3, generator=torch.Generator(device=dev).manual_seed(300 + k), device=dev)
        _cache[name] = (geo, tables, org, extent, params, target, _singles(geo, tables, org, extent, params, target))
    return _cache[name]


# ---- 1. the batch against the loop of singles
@pytest.mark.parametrize("name", ["2d_kt1", "2d_kt2", "3d_f1", "single"])
def test_batch_matches_the_loop_of_singles(dev, name):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward, hash_fused_forward
    geo, tables, org, extent, params, target, refs = _case(name, dev)
    assert not torch.equal(org[0], org[-1]) or tables.shape[0] == 1
    _compare(_batch(geo, tables, org, extent, params, target), refs, name)
    # forward only: against hash_fused_forward per field, and the same crops for every field through a [num_crops, dim] coord
    y = hash_batch_forward(geo, tables, org, extent, params)
    shared = hash_batch_forward(geo, tables, org[0].cpu(), extent, params)
    for b in range(tables.shape[0]):
        ps = [p[b] for p in params]
        check(y[b], hash_fused_forward(geo, tables[b], org[b], extent, ps), TOL_Y, f"{name} forward field {b}")
        check(shared[b], hash_fused_forward(geo, tables[b], org[0], extent, ps), TOL_Y, f"{name} shared crops field {b}")


# ---- 2. the work split
def test_more_workgroups_than_groups_of_patches(dev):
    """12 patches = 3 groups of four per field on 8 workgroups: five of them have no patch and write an all-zero record"""
    geo, tables, org, extent, params, target, refs = _case("2d_kt1", dev)
    _compare(_batch(geo, tables, org, extent, params, target, groups_per_field=8), refs, "G = 8, 3 groups")


@pytest.mark.parametrize("groups", [16, 8, 0])
def test_group_counts_the_walk_does_not_divide(dev, groups):
    """19 groups of four patches per field on 16 (two per XCD slice of three), 8 and the automatic count of workgroups"""
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward, hash_fused_forward
    geo, tables, org, extent, params, target, refs = _case("split", dev)
    _compare(_batch(geo, tables, org, extent, params, target, groups_per_field=groups), refs, f"G = {groups}, 19 groups")
    y = hash_batch_forward(geo, tables, org, extent, params, groups_per_field=groups)
    for b in range(tables.shape[0]):
        check(y[b], hash_fused_forward(geo, tables[b], org[b], extent, [p[b] for p in params]), TOL_Y, f"G = {groups} forward field {b}")


def test_more_workgroups_than_compute_units(dev):
    """B = 40 fields of 16 x 16 (one group of patches each; T = 2^10, the smallest table a descriptor takes) on 8 workgroups per field: 320
    workgroups, more than the chip has CUs - the grid is not persistent across fields and nothing depends on that"""
    B, size = 40, (16, 16)
    geo = _geo(size, 3, 2, 10, n_min=4)
    tables, params = _stacked(geo, dev, B, 11)
    org = torch.zeros(B, 1, 2, dtype=torch.int32, device=dev)
    target = torch.rand(B, 256, 3, device=dev)
    _compare(_batch(geo, tables, org, size, params, target, groups_per_field=8), _singles(geo, tables, org, size, params, target), "40 fields")


# ---- 3. independence
def test_a_field_does_not_see_its_neighbours(dev):
    geo, tables, org, extent, params, target, _ = _case("2d_kt1", dev)
    first = _batch(geo, tables, org, extent, params, target)
    again = _batch(geo, tables, org, extent, params, target)
    for a, c in zip((first[0], first[1], *first[3]), (again[0], again[1], *again[3])):
        assert torch.equal(a, c)                                  # the same launch twice: everything but the atomics is the same bits
    check(again[2], first[2], TOL_G, "table gradient, second run")
    b = 1
    t2, p2 = _stacked(geo, dev, tables.shape[0], 999)
    o2 = _origins(geo, extent, tables.shape[0], org.shape[1], dev, 998)
    g2 = torch.rand_like(target)
    for src, dst in zip((tables, org, target, *params), (t2, o2, g2, *p2)):
        dst[b] = src[b]                                           # every field but b replaced
    other = _batch(geo, t2, o2, extent, p2, g2)
    assert not torch.equal(other[0][0], first[0][0])
    assert torch.equal(other[0][b], first[0][b]) and torch.equal(other[1][b], first[1][b])
    for a, c in zip(other[3], first[3]):
        assert torch.equal(a[b], c[b])
    check(other[2][b], first[2][b], TOL_G, "table gradient of field b among other fields")


# ---- 4. flags and options
def test_frozen_tables_and_no_y(dev):
    geo, tables, org, extent, params, target, refs = _case("2d_kt1", dev)
    full = _batch(geo, tables, org, extent, params, target)
    frozen = _batch(geo, tables, org, extent, params, target, frozen=True)
    assert frozen[2] is None
    for a, c in zip((frozen[0], frozen[1], *frozen[3]), (full[0], full[1], *full[3])):
        assert torch.equal(a, c)                                  # no table gradient is formed; the decoder gradients are unchanged
    _compare(frozen, [(r[0], r[1], None, r[3]) for r in refs], "frozen")
    quiet = _batch(geo, tables, org, extent, params, target, want_y=False)
    assert quiet[0] is None
    _compare(quiet, refs, "y = None")


def test_two_chunks_add_up(dev):
    """two chunks with ADD_GRADS | ADD_LOSS against one call over both: each chunk's MSE weighted by its share"""
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_backward
    geo, tables, org, extent, params, target, refs = _case("2d_kt1", dev)
    n1 = _n(1, extent)
    gm = [torch.full_like(p, 7.0) for p in params]
    tg, loss = torch.zeros_like(tables), torch.full((tables.shape[0],), 7.0, device=dev)
    for k in range(2):
        hash_batch_forward_backward(geo, tables, org[:, k:k + 1].contiguous(), extent, params, target[:, k * n1:(k + 1) * n1].contiguous(), gm,
                                    table_grads=tg, loss=loss, loss_scale=0.5, add_grads=k > 0, add_loss=k > 0)
    _compare((None, loss, tg, gm), refs, "two chunks")


# ---- 5. the codec's noise
def test_noise_is_the_single_fields(dev):
    geo, tables, org, extent, params, target, refs = _case("2d_kt1", dev)
    quant = (4, 0x1234_5678_9ABC, 77, 123_457)
    noisy = _singles(geo, tables, org, extent, params, target, quant=quant)
    got = _batch(geo, tables, org, extent, params, target, quant=quant)
    _compare(got, noisy, "noisy b4")
    for b, (n, c) in enumerate(zip(noisy, refs)):
        assert relmax(n[0], c[0]) > 20 * TOL_Y, b                  # the noise is on (the existing file's sanity check)
        assert relmax(got[0][b], c[0]) > 20 * TOL_Y, b


# ---- 6. the optimiser
def test_step_is_fused_adam_on_the_stacked_tensors(dev):
    """the gradients of train_step(step=False), cloned; the parameters after the step on those gradients (apply_step, the optimiser half of
    train_step(step=True)) equal, bit for bit, FusedAdam on clones of the seven stacked tensors with the clones of the gradients.  A second
    train_step(step=True) forms its own table gradient, whose atomics do not fix the order: its decoder tensors - whose gradients are fixed -
    are held to the same bits, its tables to the same step on a gradient within TOL_G."""
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    from neural_image_compression_v2_amd.optim import FusedAdam
    B, size = 3, (40, 36)

    def build():
        f = HashGridFieldBatch(B, size, levels=4, features=2, log2_table=10, device=dev, seed=5, num_bits=6)
        with torch.no_grad():
            t, p = _stacked(f.geo, dev, B, 21)
            f.tables.copy_(t * 0.5)
            for a, c in zip(f.params, p):
                a.copy_(c)
        return f
    target = torch.rand(B, size[0] * size[1], 3, device=dev)
    f = build()
    losses = f.train_step([[0, 0]], size, target, step=False, noise=False)
    assert losses.shape == (B,) and f.steps == 0
    tensors = [f.tables, *f.params]
    grads = [f.tables.grad.clone(), *[g.clone() for g in f._gm]]
    assert all(float(g.abs().max()) > 0 for g in grads)
    clones = [t.detach().clone().requires_grad_(True) for t in tensors]
    ref = FusedAdam([{"params": clones[:1], "lr": 0.01}, {"params": clones[1:], "lr": 0.005}])
    ref.set_clamp(clones[:1], *models._q_range(6))
    for c, g in zip(clones, grads):
        c.grad = g.clone()
    ref.step()
    f.apply_step()
    assert f.steps == 1 and bool((f.tables.grad == 0).all())
    for n, a, c in zip(["tables"] + NAMES, tensors, clones):
        assert torch.equal(a.detach(), c.detach()), n
    lo, hi = models._q_range(6)
    assert float(f.tables.detach().min()) >= lo and float(f.tables.detach().max()) <= hi
    # the whole step in one call, on a fresh batch
    f2 = build()
    f2.train_step([[0, 0]], size, target, noise=False)
    assert f2.steps == 1
    for n, a, c in zip(NAMES, f2.params, clones[1:]):
        assert torch.equal(a.detach(), c.detach()), n
    check(f2.tables.detach(), clones[0].detach(), TOL_G, "tables after train_step(step=True)")


# ---- 7. end to end
def _image(size, dev, b):
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    g = torch.Generator(device=dev).manual_seed(b)
    base = torch.stack([0.5 + 0.3 * torch.sin((5 + 2 * b) * x + 3 * y + b), 0.5 + 0.3 * torch.cos((3 + b) * x * y * 4 - b),
                        0.5 + 0.2 * torch.sin((9 - b) * y - 2 * x + 2 * b)], dim=-1)
    return (base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1)


def test_fit_extract_insert_and_files(dev, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch
    B, size, epochs = 4, (64, 64), 300
    images = torch.stack([_image(size, dev, b) for b in range(B)])
    batch = HashGridFieldBatch(B, size, levels=8, features=2, log2_table=12, device=dev, seed=1, num_bits=8)
    batch.set_schedule(epochs)
    hist = batch.fit(images, epochs, chunk=24)                        # slabs of 24, 24 and 16 rows
    assert len(hist) == epochs and len(hist[0]) == B and batch.steps == epochs and batch.frozen
    out = batch.decode(tile=40)
    assert out.shape == (B, *size, 3)
    for b in range(B):
        assert hist[-1][b] < 0.05 * hist[0][b], (b, hist[0][b], hist[-1][b])
        err = [float(((out[b] - images[k]) ** 2).mean()) for k in range(B)]
        assert all(err[b] < e for k, e in enumerate(err) if k != b), (b, err)
    fields = [batch.extract(b) for b in range(B)]
    for b, f in enumerate(fields):
        assert isinstance(f, HashGridField) and f.route == "fused" and f.frozen and f.steps == epochs and f.num_bits == 8
        check(f.decode(), out[b], TOL_Y, f"extract({b}).decode()")
        assert f.query(torch.rand(50, 2, device=dev) * 63).shape == (50, 3)
    # the copy is independent: training it leaves the batch alone, and the other way round
    before = fields[0].decode()
    fields[1].train_step([[0, 0]], size, images[1].reshape(-1, 3).contiguous())
    assert torch.equal(batch.decode(tile=40), out)
    batch.train_step([[0, 0]], size, images.reshape(B, -1, 3).contiguous())
    assert torch.equal(fields[0].decode(), before)
    # insert(b, extract(b)) changes nothing; a field of another geometry or codec is refused
    now = batch.decode()
    for b in range(B):
        batch.insert(b, batch.extract(b))
    assert torch.equal(batch.decode(), now)
    with pytest.raises(ValueError):
        batch.insert(0, HashGridField(size, levels=8, features=2, log2_table=11, device=dev, num_bits=8, fused=True))
    with pytest.raises(ValueError):
        batch.insert(0, HashGridField(size, levels=8, features=2, log2_table=12, device=dev, num_bits=4, fused=True))
    # one ordinary single-field file per field
    for packed in (False, True):
        paths = [tmp_path / f"f{b}_{int(packed)}.pt" for b in range(B)]
        batch.save_compressed(paths, packed=packed)
        for b in range(B):
            own = tmp_path / f"own{b}_{int(packed)}.pt"
            batch.extract(b).save_compressed(own, packed=packed)
            got = HashGridField.load_compressed(paths[b], device=dev, fused=True).decode()
            assert torch.equal(got, HashGridField.load_compressed(own, device=dev, fused=True).decode())
