"""GPU tests of the hash-grid field (nic_hash_encode / nic_hash_encode_backward, csrc/hash_grid.hip; hashgrid.py).  No reference counterpart,
so the pin is an independent torch restatement of the semantics of include/nicv2_hip.h kept here, in the test: int64 index arithmetic, float64
interpolation, the backward by autograd through the gathers (index_add of the corner entries).  Forward within 1e-6 of the largest magnitude,
backward within 1e-5 of the largest gradient entry; 2D and 3D, every F, small (colliding) and large tables, non-square fields, several crops that
touch the far edge of every axis, ragged extents; the full 4K launch; the host loop against a torch-only restatement of the whole step; fit
quality in 2D and 3D."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def sample_coords(origins, extent, device):
    """[N, d] int64 sample coordinates in nic_encode order: crops back to back, the last axis fastest"""
    grids = torch.meshgrid(*[torch.arange(int(e), device=device) for e in extent], indexing="ij")
    local = torch.stack([g.reshape(-1) for g in grids], dim=1)
    org = torch.as_tensor(origins, dtype=torch.int64, device=device).reshape(-1, len(extent))
    return (org[:, None, :] + local[None]).reshape(-1, len(extent))


def ref_encode(table, field_size, resolutions, log2_table, origins, extent):
    """the semantics, restated: int64 index math, float64 weights and sums; differentiable w.r.t. ``table`` [L, T, F] (float64)"""
    dim, T = len(field_size), 1 << log2_table
    S2 = 2 * max(field_size)
    i = sample_coords(origins, extent, table.device)
    cols = []
    for l, R in enumerate(resolutions):
        q = (2 * i + 1) * R
        v, w = q // S2, (q % S2).double() / S2
        dense = (R + 1) ** dim <= T
        acc = 0
        for c in range(1 << dim):
            vc = [v[:, a] + ((c >> a) & 1) for a in range(dim)] + [torch.zeros_like(v[:, 0])] * (3 - dim)
            if dense:
                h = vc[0] + (R + 1) * (vc[1] + (R + 1) * vc[2])
            else:
                h = (vc[0] & M32) ^ ((vc[1] * 2654435761) & M32) ^ ((vc[2] * 805459861) & M32)
            h = h & (T - 1)
            cw = torch.ones_like(w[:, 0])
            for a in range(dim):
                cw = cw * (w[:, a] if (c >> a) & 1 else 1 - w[:, a])
            acc = acc + cw[:, None] * table[l][h]
        cols.append(acc)
    return torch.cat(cols, dim=1)


def relmax(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _geo(field_size, levels, F, log2_table, n_min=16):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(tuple(field_size), tuple(level_resolutions(levels, n_min, max(field_size))), F, log2_table)


def _check_fwd_bwd(dev, geo, origins, extent, seed, dx_positive=False):
    from neural_image_compression_v2_amd.hashgrid import hash_encode, hash_encode_backward
    g = torch.Generator(device=dev).manual_seed(seed)
    table = torch.rand(geo.table_shape(), generator=g, device=dev) * 2 - 1
    out = hash_encode(geo, table, origins, extent)
    t64 = table.double().requires_grad_(True)
    ref = ref_encode(t64, geo.field_size, geo.resolutions, geo.log2_table, origins, extent)
    assert out.shape == ref.shape
    e = relmax(out, ref)
    assert e < 1e-6, (geo, extent, e)
    dx = torch.rand(out.shape, generator=g, device=dev)
    if not dx_positive:
        dx = dx * 2 - 1
    ref.backward(dx.double())
    base = torch.rand(geo.table_shape(), generator=g, device=dev)                  # the call ADDS to what is there
    grad = base.clone()
    org = geo.upload_origins(origins, extent, dev)
    hash_encode_backward(geo, org, extent, dx, grad)
    torch.cuda.synchronize()
    gref = t64.grad
    eb = float(((grad.double() - base.double()) - gref).abs().max() / gref.abs().max())
    assert eb < 1e-5, (geo, extent, eb)
    # entries no sample touches stay exactly as they were
    touched = torch.zeros(geo.table_shape(), dtype=torch.float64, device=dev)
    r2 = ref_encode(touched.requires_grad_(True), geo.field_size, geo.resolutions, geo.log2_table, origins, extent)
    r2.backward(torch.ones_like(r2))
    untouched = touched.grad == 0
    assert bool(untouched.any()) or geo.log2_table == 10
    assert torch.equal(grad[untouched], base[untouched])
    z = torch.zeros_like(grad)
    hash_encode_backward(geo, org, extent, dx, z)
    assert bool((z[untouched] == 0).all())
    return e, eb


@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("levels", [1, 5, 16])
@pytest.mark.parametrize("log2_table", [10, 19])
def test_forward_backward_2d(dev, F, levels, log2_table):
    geo = _geo((200, 131), levels, F, log2_table)                                   # non-square, not a power of two
    origins = [[0, 0], [200 - 37, 131 - 21], [64, 3]]                                # the second crop touches the far edge of both axes
    _check_fwd_bwd(dev, geo, origins, (37, 21), seed=F * 100 + levels + log2_table)  # ragged: 37 x 21 is not a multiple of the 8 x 8 patch


@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("levels", [1, 5, 16])
@pytest.mark.parametrize("log2_table", [10, 19])
def test_forward_backward_3d(dev, F, levels, log2_table):
    geo = _geo((40, 27, 33), levels, F, log2_table, n_min=4)
    origins = [[0, 0, 0], [40 - 13, 27 - 10, 33 - 9], [5, 11, 2]]
    _check_fwd_bwd(dev, geo, origins, (13, 10, 9), seed=F * 100 + levels + log2_table + 7)


def test_coarse_vertices_run_sums(dev):
    """a whole 512^2 crop on a handful of coarse vertices (N_min 2): every wave of the backward reduces long runs before its atomics"""
    geo = _geo((512, 512), 4, 2, 19, n_min=2)
    assert geo.resolutions[0] == 2
    _check_fwd_bwd(dev, geo, [[0, 0]], (512, 512), seed=5, dx_positive=True)


def test_4k_launch(dev):
    """the bench shape: 3840 x 2160, L 16, F 2, T 2^19 (11 dense and 5 hashed levels), forward and backward against the restatement on the GPU"""
    geo = _geo((3840, 2160), 16, 2, 19)
    _check_fwd_bwd(dev, geo, [[0, 0]], (3840, 2160), seed=11)


def _torch_step_restatement(field, image, crops, extent, steps):
    """the host loop in torch alone: the same init, the encoding of ``ref_encode``, nn.Linear + erf GELU + sigmoid, torch.optim.Adam"""
    table = field.table.detach().clone().requires_grad_(True)
    dec = copy.deepcopy(field.decoder.decoder)
    opt = torch.optim.Adam([{"params": [table], "lr": 0.01}, {"params": dec.parameters(), "lr": 0.005}])
    geo = field.geo
    losses = []
    for k in range(steps):
        org = crops[k]
        i = sample_coords(org, extent, image.device)
        target = image[i[:, 0], i[:, 1]]
        opt.zero_grad()
        x = ref_encode(table.double(), geo.field_size, geo.resolutions, geo.log2_table, org, extent).float()
        loss = ((dec(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    with torch.no_grad():
        y = dec(ref_encode(table.double(), geo.field_size, geo.resolutions, geo.log2_table, [[0, 0]], geo.field_size).float())
    return losses, y.reshape(*geo.field_size, 3)


def _image(size, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.3 * torch.sin(7 * x + 3 * y), 0.5 + 0.3 * torch.cos(5 * x * y * 4), 0.5 + 0.2 * torch.sin(13 * y - 2 * x)], dim=-1)
    return (base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1)


def test_host_loop_matches_torch_restatement(dev):
    """20 steps of HashGridField against the torch-only restatement: per-step losses within 1e-3 relative, the decoded image within 2e-3"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, extent = (256, 192), (64, 48)
    image = _image(size, dev)
    field = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=3)   # coarse levels dense, fine ones hashed into 2^12
    assert any((r + 1) ** 2 > 2 ** 12 for r in field.resolutions)
    g = torch.Generator().manual_seed(9)
    crops = [torch.stack([torch.randint(0, size[0] - extent[0] + 1, (4,), generator=g), torch.randint(0, size[1] - extent[1] + 1, (4,), generator=g)], 1)
             for _ in range(20)]
    ref_losses, ref_img = _torch_step_restatement(field, image, crops, extent, 20)
    losses = []
    for k in range(20):
        i = sample_coords(crops[k], extent, dev)
        losses.append(float(field.train_step(crops[k], extent, image[i[:, 0], i[:, 1]])))
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(losses, ref_losses)):
        assert abs(a - b) <= 1e-3 * abs(b), (k, a, b)
    assert losses[-1] < losses[0]
    img = field.decode()
    assert img.shape == (*size, 3)
    assert float((img - ref_img).abs().max()) < 2e-3


def test_fit_quality_2d_chunked_passes(dev):
    """300 whole-image passes walked in four chunks (accumulate / scale / step): the loss falls below 0.05 x its start; decode(tile=100) equals
    the untiled forward"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size = (256, 256)
    image = _image(size, dev, seed=1)
    field = HashGridField(size, device=dev, seed=1)
    field.set_schedule(300)
    chunk = 64
    targets = [image[x0:x0 + chunk].reshape(-1, 3).contiguous() for x0 in range(0, size[0], chunk)]
    hist = []
    for it in range(300):
        tot = 0.0
        for k, x0 in enumerate(range(0, size[0], chunk)):
            last = k == len(targets) - 1
            tot = tot + field.train_step([[x0, 0]], (chunk, size[1]), targets[k], accumulate=k > 0, scale=1 / len(targets), step=last)
        hist.append(float(tot))
    assert hist[-1] < 0.05 * hist[0], (hist[0], hist[-1])
    with torch.no_grad():
        full = field.forward([[0, 0]], size).reshape(*size, 3)
    tiled = field.decode(tile=100)
    assert float((tiled - full).abs().max()) <= 1e-6
    assert float(((full - image) ** 2).mean()) < 0.05 * hist[0]


def test_fit_quality_3d_volume(dev):
    """a 64^3 volume: the loss falls below 0.1 x its start; the tiled decode of a volume equals its untiled forward"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    n = 64
    ax = torch.linspace(0, 1, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.stack([0.5 + 0.3 * torch.sin(6 * x + 2 * z), 0.5 + 0.3 * torch.cos(4 * y - 3 * z), 0.5 + 0.25 * torch.sin(5 * (x + y + z))], dim=-1)
    target = vol.reshape(-1, 3).contiguous()
    field = HashGridField((n, n, n), levels=8, features=2, log2_table=16, base_resolution=4, device=dev, seed=2)
    hist = [float(field.train_step([[0, 0, 0]], (n, n, n), target)) for _ in range(150)]
    assert hist[-1] < 0.1 * hist[0], (hist[0], hist[-1])
    with torch.no_grad():
        full = field.forward([[0, 0, 0]], (n, n, n)).reshape(n, n, n, 3)
    assert float((field.decode(tile=40) - full).abs().max()) <= 1e-6
