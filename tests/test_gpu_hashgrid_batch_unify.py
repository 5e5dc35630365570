"""GPU tests of the batched entries at points at the smallest shapes that can still go wrong: field b's outputs are the
single-field entry's on field b's tensors and first n_b rows, bit for bit, for each of the four training entries (plain, level of detail,
d loss / d points, d loss / d lambda on top) with and without the codec's noise, and for the two gradient-only entries - in 2D and 3D, at
L F <= 32 (levels 4, features 2) and L F > 32 (levels 9, features 4: both KT), with and without an order.  B = 2, log2_table 10:

- n = 64, counts (64, 37): one wave item per field, the second ragged.  Every output is bit-equal: y, loss, decoder gradients, dpoints, dlod,
  table gradients (one wave adds to a field's table: the single-field launch adds the same values in the same order).
- n = 70, counts (70, 5): two wave items, the second with 6 live lanes, beside a field with fewer points than one wave.  y, dpoints, dlod, loss
  and the decoder gradients bit for bit; the table gradients within 1e-5 of the largest update (tests/test_gpu_hashgrid_batch_lodgrad.py's
  rule: the order of the atomics is free once two waves add to one field).
- n = 64, counts (64, 0): a field without points - its record is all zero (decoder gradients 0), its loss is 0, nothing of its rows is written.

The inputs of a shape are made once and left unchanged."""
import pytest
import torch

from tests.test_hashgrid_lodtrain_cpu import NOISE_KEYS

pytestmark = pytest.mark.gpu

B, LOSS_SCALE, SENTINEL, TOL_ORDER = 2, 3.0, -12345.5, 1e-5
SHAPES = {"one_wave": (64, (64, 37)), "two_waves": (70, (70, 5)), "empty_field": (64, (64, 0))}
GEOS = {(2, False): ((40, 36), 4, 2), (2, True): ((40, 36), 9, 4), (3, False): ((12, 10, 8), 4, 2), (3, True): ((12, 10, 8), 9, 4)}
TRAIN = ("plain", "lod", "joint", "joint_with_lod", "joint_lod")       # joint: nic_hash_batch_forward_backward_points_grad without and with a lodp
GRAD = ("grad", "grad_with_lod", "grad_lod")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_INPUTS = {}


def inputs(dim, wide, shape, dev):
    """the two fields of a case on the device, stacked; made once and left unchanged"""
    key = (dim, wide, shape)
    if key not in _INPUTS:
        from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
        size, levels, features = GEOS[(dim, wide)]
        geo = HashGeometry(size, tuple(level_resolutions(levels, 4, max(size))), features, 10)
        assert (geo.width > 32) == wide
        n, counts = SHAPES[shape]
        g = torch.Generator().manual_seed(1000 * dim + 100 * wide + n)
        lf = geo.width
        params = [torch.randn(B, 64, lf, generator=g) * 0.3, torch.randn(B, 64, generator=g) * 0.1, torch.randn(B, 64, 64, generator=g) * 0.15,
                  torch.randn(B, 64, generator=g) * 0.1, torch.randn(B, 3, 64, generator=g) * 0.2, torch.randn(B, 3, generator=g) * 0.1]
        points = torch.rand(B, n, dim, generator=g) * torch.tensor([float(s) for s in size])
        order = torch.stack([torch.cat([torch.randperm(c, generator=g), torch.arange(c, n)]) for c in counts]).to(torch.int32)
        d = dict(geo=geo, n=n, counts=counts, fade=tuple(float(levels - l) for l in range(levels)),
                 tables=(torch.rand(B, *geo.table_shape(), generator=g) - 0.5) * 0.5, params=params, points=points,
                 target=torch.rand(B, n, 3, generator=g), lod=torch.rand(B, n, generator=g) * (levels + 1.5), order=order)
        _INPUTS[key] = {k: ([t.to(dev) for t in v] if k == "params" else v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    return _INPUTS[key]


def _lod_args(i, with_lod, b=None, n_b=None):
    if not with_lod:
        return {}
    lod = i["lod"] if b is None else i["lod"][b, :n_b].contiguous()
    return dict(lod=lod, lod_uniform=0.25, fade=i["fade"])


@pytest.mark.parametrize("ordered", [False, True], ids=["rows", "order"])
@pytest.mark.parametrize("noise", [None, 4], ids=["exact", "noisy"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
@pytest.mark.parametrize("wide", [False, True], ids=["kt1", "kt2"])
@pytest.mark.parametrize("dim", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("family", TRAIN)
def test_a_training_entry_is_the_single_fields_per_field(dev, family, dim, wide, shape, noise, ordered):
    from neural_image_compression_v2_amd import hashgrid as hg
    i = inputs(dim, wide, shape, dev)
    geo, n, counts = i["geo"], i["n"], i["counts"]
    with_lod = family in ("lod", "joint_with_lod", "joint_lod")
    batch_fn, single_fn = {"plain": (hg.hash_batch_forward_backward_points, hg.hash_fused_forward_backward_points),
                           "lod": (hg.hash_batch_forward_backward_points_lod, hg.hash_fused_forward_backward_points_lod),
                           "joint": (hg.hash_batch_forward_backward_points_grad, hg.hash_fused_forward_backward_points_grad),
                           "joint_with_lod": (hg.hash_batch_forward_backward_points_grad, hg.hash_fused_forward_backward_points_grad),
                           "joint_lod": (hg.hash_batch_forward_backward_points_grad_lod, hg.hash_fused_forward_backward_points_grad_lod)}[family]
    quant = None if noise is None else NOISE_KEYS[noise]
    more = {}
    y = torch.full((B, n, 3), SENTINEL, device=dev)
    if family.startswith("joint"):
        more["dpoints"] = torch.full((B, n, dim), SENTINEL, device=dev)
    if family == "joint_lod":
        more["dlod"] = torch.full((B, n), SENTINEL, device=dev)
    gm, tg = [torch.zeros_like(p) for p in i["params"]], torch.zeros_like(i["tables"])
    out = batch_fn(geo, i["tables"], i["points"], i["params"], i["target"], gm, **_lod_args(i, with_lod), table_grads=tg,
                   order=i["order"] if ordered else None, counts=counts, loss_scale=LOSS_SCALE, want_y=y, quant=quant, **more)
    loss = out[0]
    extra = [more[k] for k in ("dpoints", "dlod") if k in more]
    for b in range(B):
        n_b = counts[b]
        for t in [y] + extra:
            assert bool((t[b, n_b:] == SENTINEL).all()) and bool((t[b, :n_b] != SENTINEL).all()), (b, n_b)    # rows at or past n_b are not written
        if n_b == 0:
            assert float(loss[b]) == 0.0 and all(bool((g[b] == 0).all()) for g in gm) and bool((tg[b] == 0).all())
            continue
        pb = [p[b].contiguous() for p in i["params"]]
        gm1, tg1 = [torch.zeros_like(p) for p in pb], torch.zeros_like(i["tables"][b])
        out1 = single_fn(geo, i["tables"][b], i["points"][b, :n_b].contiguous(), pb, i["target"][b, :n_b].contiguous(), gm1,
                         **_lod_args(i, with_lod, b, n_b), table_grad=tg1, order=i["order"][b, :n_b].contiguous() if ordered else None,
                         loss_scale=LOSS_SCALE, want_y=True, quant=quant)
        what = (family, dim, wide, shape, noise, ordered, b)
        assert torch.equal(loss[b], out1[0].reshape(())) and torch.equal(y[b, :n_b], out1[1]), what
        assert all(torch.equal(g[b], g1) for g, g1 in zip(gm, gm1)), what
        for k, t in enumerate(extra):
            assert torch.equal(t[b, :n_b], out1[2 + k]), (what, k)
        assert bool((tg1 != 0).any())
        if n_b <= 64:
            assert torch.equal(tg[b], tg1), what
        else:
            e = float((tg[b] - tg1).abs().max() / tg1.abs().max())
            print(f"{what}: table gradient {e:.3e} of the single field's largest")
            assert e <= TOL_ORDER, (what, e)


@pytest.mark.parametrize("kind,bits", [("f32", None), ("bits", 4)], ids=["f32", "bits"])
@pytest.mark.parametrize("ordered", [False, True], ids=["rows", "order"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
@pytest.mark.parametrize("wide", [False, True], ids=["kt1", "kt2"])
@pytest.mark.parametrize("dim", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("family", GRAD)
def test_a_gradient_entry_is_the_single_fields_per_field(dev, family, dim, wide, shape, ordered, kind, bits):
    from neural_image_compression_v2_amd import hashgrid as hg
    from neural_image_compression_v2_amd import models
    i = inputs(dim, wide, shape, dev)
    geo, n, counts = i["geo"], i["n"], i["counts"]
    with_lod = family != "grad"
    batch_fn, single_fn = (hg.hash_batch_points_grad_lod, hg.hash_fused_points_grad_lod) if family == "grad_lod" else (hg.hash_batch_points_grad,
                                                                                                                       hg.hash_fused_points_grad)
    data = i["tables"] if kind == "f32" else torch.stack([hg.hash_pack_bits(geo, models.quantize_clamp(i["tables"][b], bits), bits) for b in range(B)])
    # y and, where the wrapper takes them, dpoints and dlod go into tensors full of a sentinel; a tensor the call allocates is zero where not written
    outs = [torch.full((B, n, 3), SENTINEL, device=dev)]
    more = {}
    if family == "grad_lod":
        outs += [torch.full((B, n, dim), SENTINEL, device=dev), torch.full((B, n), SENTINEL, device=dev)]
        more = dict(dpoints=outs[1], dlod=outs[2])
    got = batch_fn(geo, data, i["points"], i["params"], target=i["target"], loss_scale=LOSS_SCALE, counts=counts, order=i["order"] if ordered else None,
                   want_y=outs[0], kind=kind, num_bits=bits, **_lod_args(i, with_lod), **more)
    assert got[0] is outs[0]
    blank = [SENTINEL] * len(outs) + [0.0] * (len(got) - len(outs))
    outs += list(got[len(outs):])
    for b in range(B):
        n_b = counts[b]
        for t, v in zip(outs, blank):
            assert bool((t[b, n_b:] == v).all()) and (v == 0.0 or bool((t[b, :n_b] != v).all())), (b, n_b)    # rows at or past n_b are not written
        if n_b == 0:
            continue
        out1 = single_fn(geo, data[b], i["points"][b, :n_b].contiguous(), [p[b].contiguous() for p in i["params"]],
                         target=i["target"][b, :n_b].contiguous(), loss_scale=LOSS_SCALE, kind=kind, num_bits=bits, **_lod_args(i, with_lod, b, n_b))
        for k, t in enumerate(outs):
            assert torch.equal(t[b, :n_b], out1[k]), (family, dim, wide, shape, ordered, kind, b, k)
