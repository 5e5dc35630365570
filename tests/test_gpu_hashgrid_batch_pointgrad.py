"""GPU tests of the batch's gradients with respect to the point positions (nic_hash_batch_points_grad, csrc/hashgrid_batch_grad.hip;
nic_hash_batch_forward_backward_points_grad, csrc/hashgrid_batch.hip, hash_batch_points_joint_kernel; ``HashGridFieldBatch.point_gradient`` /
``jacobian`` / ``query_differentiable`` / ``train_points_grad`` / ``train_points_differentiable``).

The yardstick is the float64 reference step (oracle/hashgrid_train_ref.py) of EVERY field at ITS OWN points, ``dpoints`` included, with the
metric and the bounds of tests/test_hashgrid_train_ref_cpu.py untouched (``C.measure``: y and loss 5e-6, every gradient and dpoints 1e-4) and
the ``Batch`` discipline of tests/test_gpu_hashgrid_batch_points.py: B = 3 fields of 209 points with the edges of the domain, points outside,
NaN and infinities, a non-zero table-gradient base, sevens that must be overwritten - and sevens that must STAY in the rows of y and dpoints
at or past a field's count.  tests/test_hashgrid_batch_pointgrad_cpu.py shows on the CPU that these inputs notice the neighbour's table, the
padded width in the scale, ``dpoints`` stored at the position in the order and ``lod`` read there.

Then the siblings (the training entries without dpoints bit for bit; the gradient entry bit for bit), the gradient entry from the three kinds
of stacked tables against the single-field entry and the reference, the class against the extracted fields, and what it is for: three fields
fitted while each registers its own second view."""
import types

import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests import test_gpu_hashgrid_batch_lod as BL
from tests import test_gpu_hashgrid_batch_points as BP
from tests import test_gpu_hashgrid_pointtrain as PT
from tests import test_gpu_hashgrid_train_ref as R
from tests import test_hashgrid_batch_lod_cpu as L
from tests import test_hashgrid_batch_pointgrad_cpu as Q
from tests import test_hashgrid_batch_points_cpu as P
from tests import test_hashgrid_train_ref_cpu as C
from tests.test_hashgrid_train_ref_cpu import LOSS_SCALE, NAMES, SHAPES, TOL_G, TOL_Y, shape_id

pytestmark = pytest.mark.gpu
B, N = C.N_FIELDS, P.N
COUNT_IDS = ["full", "209-65-1", "64-0-63"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _refs(shape, counts, noisy, mode):
    return [Q.joint_reference(shape, b, P.count_of(counts, b), noisy, mode) if P.count_of(counts, b) else None for b in range(B)]


def _batch(dev, shape, noisy, counts, mode):
    refs = _refs(shape, counts, noisy, mode)
    return BP.Batch(dev, shape, noisy, refs) if mode is None else BL.LodBatch(dev, shape, noisy, refs, mode)


def _lod_kw(h):
    """the level of detail of a harness as the wrappers' keywords (none for the plain ``Batch``)"""
    return dict(lod=h.lod, lod_uniform=h.uniform, fade=h.fade) if isinstance(h, BL.LodBatch) else {}


def _joint(h, counts=None, order=None, y=None, dp=None, **kw):
    from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_backward_points_grad
    y = torch.full((B, N, 3), 7.0, device=h.dev) if y is None else y
    dp = torch.full((B, N, h.geo.dim), 7.0, device=h.dev) if dp is None else dp
    args = dict(table_grads=h.tg, order=h.order(order, counts), counts=counts, loss=h.loss, loss_scale=LOSS_SCALE, want_y=y, quant=h.quant, dpoints=dp)
    args.update(_lod_kw(h))
    args.update(kw)
    _, _, out = hash_batch_forward_backward_points_grad(h.geo, h.tables, h.points, h.params, h.target, h.gm, **args)
    assert out is dp
    return y, dp


def _exactly_zero(x):
    return bool((x.contiguous().view(torch.int32) == 0).all())


def _hold(h, what, y, dp, counts):
    """every field against its reference, dpoints included (``R._check``), on top of ``Batch.finish``'s discipline"""
    for b, ref in enumerate(h.refs):
        name, n_b = f"{what} field {b}", P.count_of(counts, b)
        assert bool((y[b, n_b:] == 7.0).all()), f"{name}: a row of y at or past the field's count was written"
        assert bool((dp[b, n_b:] == 7.0).all()), f"{name}: a row of dpoints at or past the field's count was written"
        if ref is None:                         # no point: loss 0, decoder gradients 0, the table gradient and dpoints untouched
            assert float(h.loss[b]) == 0.0 and all(bool((g[b] == 0).all()) for g in h.gm), name
            assert torch.equal(h.tg[b].view(torch.int32), h.base[b].view(torch.int32)), name
            continue
        tgd = [(h.tg[b][l].double() - h.base[b][l].double()).cpu() for l in range(h.geo.levels)]
        got = types.SimpleNamespace(y=y[b, :n_b].cpu(), loss=h.loss[b].reshape(()).cpu(), table_grad=tgd, decoder_grads=[g[b].cpu() for g in h.gm],
                                    dpoints=dp[b, :n_b].cpu())
        assert "dpoints" in C.measure(got, ref)
        R._check(name, got, ref)
        f = P.field_inputs(h.shape, b)
        moved = torch.from_numpy(T.clamp_points(f.geo, f.points[:n_b])[1])
        assert _exactly_zero(got.dpoints[moved]), f"{name}: an axis whose clamp moved the point is not exactly 0.0"
        for l, gl in enumerate(ref.table_grad):                           # what the reference leaves at zero keeps the buffer's bits
            z = (gl == 0).to(h.dev)
            assert torch.equal(h.tg[b][l][z].view(torch.int32), h.base[b][l][z].view(torch.int32)), f"{name}: level {l}, an untouched entry moved"


# ---- 1. the joint entry: every field against ITS float64 reference, dpoints included
@pytest.mark.parametrize("order", [None, "perm", "cell"], ids=["unordered", "perm", "cell"])
@pytest.mark.parametrize("counts", P.COUNTS, ids=COUNT_IDS)
@pytest.mark.parametrize("noisy", [False, True], ids=["table", "table_q"])
@pytest.mark.parametrize("mode", [None, "point"], ids=["plain", "lod"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_field_against_its_reference(dev, shape, mode, noisy, counts, order):
    h = _batch(dev, shape, noisy, counts, mode)
    y, dp = _joint(h, counts, order)
    _hold(h, f"joint {shape_id(shape)} {mode or 'plain'} {'noisy' if noisy else 'plain'} counts={counts} order={order}", y, dp, counts)


@pytest.mark.parametrize("shape,noisy,mode", [((2, 2, 16), False, "uniform"), ((3, 4, 8), True, "uniform"), ((2, 4, 10), True, "skip"), ((3, 2, 4), True, "skip"),
                                              ((2, 4, 10), True, "boundary"), ((3, 8, 8), True, "boundary"), ((2, 2, 16), True, "off"), ((3, 8, 8), True, "off")],
                         ids=lambda v: v if isinstance(v, str) else (shape_id(v) if isinstance(v, tuple) else ("table_q" if v else "table")))
def test_launch_wide_levels_of_detail(dev, shape, noisy, mode):
    """the lod file's launch-wide cases: lod_uniform alone, whole waves skipping every level but the coarsest, a skipped level that opens a
    block of noise columns, and every level off - where nothing is read, the table gradient keeps its bits and dpoints is exactly zero"""
    h = _batch(dev, shape, noisy, None, mode)
    assert h.lod is None
    y, dp = _joint(h)
    _hold(h, f"joint {shape_id(shape)} {mode}", y, dp, None)
    if mode == "off":
        assert torch.equal(h.tg.view(torch.int32), h.base.view(torch.int32)) and _exactly_zero(dp)


# ---- 2. against the siblings
@pytest.mark.parametrize("order", [None, "cell"], ids=["unordered", "cell"])
@pytest.mark.parametrize("noisy", [False, True], ids=["table", "table_q"])
@pytest.mark.parametrize("mode", [None, "point"], ids=["plain", "lod"])
@pytest.mark.parametrize("shape", [(2, 2, 16), (3, 8, 8)], ids=shape_id)
def test_against_the_training_and_the_gradient_entries(dev, shape, mode, noisy, order):
    """loss, y and the six decoder gradients are the training entry's without dpoints bit for bit (the same records, the same reduction); the
    table gradient within 1e-5 of its largest magnitude (atomics, DESIGN 4.7.12's bound); without noise dpoints is the gradient entry's with
    ``target`` bit for bit, from trained and from frozen tables"""
    from neural_image_compression_v2_amd.hashgrid import (hash_batch_forward_backward_points, hash_batch_forward_backward_points_lod,
                                                          hash_batch_points_grad)
    from tests.test_gpu_hashgrid_batch import check
    counts = (209, 65, 1)
    h = _batch(dev, shape, noisy, counts, mode)
    h.tg.zero_()
    od = h.order(order, counts)
    y, dp = _joint(h, counts, order)
    gm = [torch.full_like(p, 7.0) for p in h.params]
    tg, loss, y1 = torch.zeros_like(h.tg), torch.full((B,), 7.0, device=dev), torch.full((B, N, 3), 7.0, device=dev)
    kw = dict(table_grads=tg, order=od, counts=counts, loss=loss, loss_scale=LOSS_SCALE, want_y=y1, quant=h.quant)
    if mode is None:
        hash_batch_forward_backward_points(h.geo, h.tables, h.points, h.params, h.target, gm, **kw)
    else:
        hash_batch_forward_backward_points_lod(h.geo, h.tables, h.points, h.params, h.target, gm, h.lod, h.uniform, h.fade, **kw)
    assert torch.equal(h.loss, loss) and torch.equal(y, y1)
    for n, a, r in zip(NAMES, h.gm, gm):
        assert torch.equal(a, r), n
    check(h.tg, tg, 1e-5, f"{shape_id(shape)} table gradient against the entry without dpoints")
    if not noisy:
        for frozen in (False, True):
            if frozen:
                y2, dp2 = _joint(h, counts, order, table_grads=None)
                assert torch.equal(y2, y)
            else:
                dp2 = dp
            yg, dg = hash_batch_points_grad(h.geo, h.tables, h.points, h.params, target=h.target, loss_scale=LOSS_SCALE, counts=counts, order=od, **_lod_kw(h))
            for b, n_b in enumerate(counts):
                assert torch.equal(dp2[b, :n_b], dg[b, :n_b]) and torch.equal(y[b, :n_b], yg[b, :n_b]), (b, frozen)
                assert _exactly_zero(dg[b, n_b:]) and _exactly_zero(yg[b, n_b:])       # fresh tensors: zero where nothing is written


def test_dpoints_is_overwritten_under_the_add_flags(dev):
    """NIC_HASH_FUSED_ADD_GRADS adds the decoder gradients; dpoints is written, never added to"""
    shape, counts = (2, 4, 10), (209, 65, 1)
    h = _batch(dev, shape, False, counts, None)
    y, dp = _joint(h, counts, "cell")
    first = dp.clone()
    gm1 = [g.clone() for g in h.gm]
    _joint(h, counts, "cell", y=y, dp=dp, add_grads=True, add_loss=True)
    assert torch.equal(dp, first)
    for n, a, r in zip(NAMES, h.gm, gm1):
        assert torch.equal(a, r + r), n


# ---- 3. the gradient entry
NUM_BITS = C.NOISE_BITS


def _stacks(h, kind):
    """(data, kind, num_bits, per-field fp32 tables the stored values stand for) of the harness's table_q fields"""
    from neural_image_compression_v2_amd import hashgrid
    if kind == "f32":
        return h.tables, None, [h.tables[b] for b in range(B)]
    if kind == "u8":
        data = torch.stack([hashgrid.hash_pack_u8(h.geo, h.tables[b], NUM_BITS) for b in range(B)]).contiguous()
        return data, NUM_BITS, [hashgrid._table_of_u8(h.geo, data[b], NUM_BITS) for b in range(B)]
    data = torch.stack([hashgrid.hash_pack_bits(h.geo, h.tables[b], NUM_BITS) for b in range(B)]).contiguous()
    return data, NUM_BITS, [hashgrid._table_of_u8(h.geo, hashgrid.hash_unpack_bits(h.geo, data[b], NUM_BITS), NUM_BITS) for b in range(B)]


@pytest.mark.parametrize("mode", [None, "point"], ids=["plain", "lod"])
@pytest.mark.parametrize("kind", ["f32", "u8", "bits"])
@pytest.mark.parametrize("shape", [(2, 2, 16), (2, 4, 10), (3, 1, 6), (3, 8, 8)], ids=shape_id)
def test_the_gradient_entry_from_every_kind_of_table(dev, shape, kind, mode):
    """with ``dy``: field b's rows are ``hash_fused_points_grad`` on field b's tensors bit for bit, with ragged counts and an order, and rows at
    or past the count keep their sevens; with ``target``: within TOL_G of the float64 reference taken on the values the stored table stands
    for; twice the same bits"""
    from neural_image_compression_v2_amd import hashgrid
    counts = (209, 65, 1)
    h = _batch(dev, shape, True, counts, mode)
    data, bits, tables = _stacks(h, kind)
    lod_kw = _lod_kw(h)
    g = torch.Generator().manual_seed(3)
    dy = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    for order in (None, "cell", "perm"):
        od = h.order(order, counts)
        y, dp = torch.full((B, N, 3), 7.0, device=dev), torch.full((B, N, h.geo.dim), 7.0, device=dev)
        args = (h.geo, data, h.points, h.params, dy, None, 1.0, counts, od, y, kind, bits, lod_kw.get("lod"), lod_kw.get("lod_uniform", 0.0), lod_kw.get("fade"), 0)
        hashgrid._batch_points_grad(*args, dpoints=dp)
        again = hashgrid._batch_points_grad(*args[:9], True, *args[10:])
        for b, n_b in enumerate(counts):
            single_lod = {} if mode is None else dict(lod=h.lod[b, :n_b].contiguous(), lod_uniform=h.uniform, fade=h.fade)
            y1, dp1 = hashgrid.hash_fused_points_grad(h.geo, data[b], h.points[b, :n_b].contiguous(), [p[b] for p in h.params], dy=dy[b, :n_b].contiguous(),
                                                      kind=kind, num_bits=bits, **single_lod)
            what = f"{shape_id(shape)} {kind} {mode or 'plain'} order={order} field {b}"
            assert torch.equal(dp[b, :n_b], dp1) and torch.equal(y[b, :n_b], y1), f"{what}: not the single-field entry's bits"
            assert bool((dp[b, n_b:] == 7.0).all()) and bool((y[b, n_b:] == 7.0).all()), f"{what}: a row at or past the count was written"
            assert torch.equal(again[1][b, :n_b], dp1) and torch.equal(again[0][b, :n_b], y1), f"{what}: the second launch gave other bits"
    # with a target: the float64 reference on the dequantised values (frozen: the table is a constant here)
    y, dp = hashgrid.hash_batch_points_grad(h.geo, data, h.points, h.params, target=h.target, loss_scale=LOSS_SCALE, counts=counts, order=h.order("cell", counts),
                                            kind=kind, num_bits=bits, **lod_kw)
    for b, n_b in enumerate(counts):
        f = P.field_inputs(shape, b)
        lod = None if mode is None else (L.lod_of(shape, b, mode)[0], L.lod_of(shape, b, mode)[1][:n_b], L.lod_of(shape, b, mode)[2])
        ref = T.step(f.geo, tables[b].cpu(), f.params, f.target[:n_b], points=f.points[:n_b], loss_scale=LOSS_SCALE, frozen=True, lod=lod)
        ey, ed = float((y[b, :n_b].double().cpu() - ref.y).abs().max()), C.relmax(dp[b, :n_b].cpu(), ref.dpoints)
        print(f"MEASURED gradient entry {shape_id(shape)} {kind} {mode or 'plain'} field {b} | y {ey:.3e} | dpoints {ed:.3e}")
        assert ey <= TOL_Y and ed <= TOL_G, (b, ey, ed)
        moved = torch.from_numpy(T.clamp_points(f.geo, f.points[:n_b])[1])
        assert _exactly_zero(dp[b, :n_b].cpu()[moved])


# ---- 4. the class
def test_train_points_grad_is_the_extracted_fields(dev):
    """one step with ragged counts against ``extract(b).train_points(fused=True, dpoints=)`` on twins, plain and with a level of detail:
    the comparison and the bounds tests/test_gpu_hashgrid_batch_points.py applies to ``train_points``; the bookkeeping is ``train_points``'"""
    from tests.test_gpu_hashgrid_batch import check
    shape, counts = (2, 2, 16), BP.COUNTS_D
    lod_all = torch.stack([torch.from_numpy(C.inputs(*shape, b).lod) for b in range(B)]).to(dev)
    for lod in (None, lod_all):
        f, points, target = BP._build(dev, shape)
        twin, _, _ = BP._build(dev, shape)
        singles = [f.extract(b) for b in range(B)]
        dp = torch.full((B, N, 2), 7.0, device=dev)
        losses, out = f.train_points_grad(points, target, dpoints=dp, lod=lod, counts=counts, step=False, order="cell")
        assert out is dp and losses.shape == (B,) and f.steps == 0 and f._pass_samples == N and not f._grad_clean
        l0 = twin.train_points(points, target, counts=counts, step=False, order="cell") if lod is None else \
            twin.train_points_lod(points, target, lod, counts=counts, step=False, order="cell")
        assert torch.equal(losses, l0) and all(torch.equal(a, c) for a, c in zip(f._gm, twin._gm))       # the same step as without dpoints
        for b, n_b in enumerate(counts):
            s = singles[b]
            dp1 = torch.full((n_b, 2), 7.0, device=dev)
            kw = {} if lod is None else dict(lod=lod[b, :n_b].contiguous())
            l1 = s.train_points(points[b, :n_b].contiguous(), target[b, :n_b].contiguous(), fused=True, step=False, order="cell", dpoints=dp1, **kw)
            what = f"train_points_grad {'plain' if lod is None else 'lod'} field {b} ({n_b} points)"
            check(losses[b].reshape(1), l1.reshape(1), TOL_Y, f"{what} loss")
            check(f.tables.grad[b], s.table.grad, TOL_G, f"{what} table gradient")
            for n, a, r in zip(NAMES, f._gm, s._fused_gm):
                check(a[b], r, TOL_G, f"{what} {n}")
            check(dp[b, :n_b], dp1, TOL_G, f"{what} dpoints")
            assert bool((dp[b, n_b:] == 7.0).all())
        f.apply_step()
        assert f.steps == 1
    # a fresh dpoints: zero at the rows a field does not own; after freeze() it still comes, and no table moves
    f, points, target = BP._build(dev, shape)
    f.freeze()
    before = f.tables.detach().clone()
    losses, dp = f.train_points_grad(points, target, counts=counts)
    assert dp.shape == (B, N, 2) and all(_exactly_zero(dp[b, n_b:]) and bool((dp[b, :n_b] != 0).any()) for b, n_b in enumerate(counts))
    assert torch.equal(f.tables.detach().view(torch.int32), before.view(torch.int32)) and f.steps == 1


def test_accumulate_fills_each_chunks_own_dpoints(dev):
    """a pass in two chunks: each call overwrites ITS dpoints with the gradient of ITS chunk's loss (noise keyed by the samples before it),
    the decoder gradients add up, one optimiser step"""
    shape = (2, 2, 16)
    f, points, target = BP._build(dev, shape)
    twin, _, _ = BP._build(dev, shape)
    chunks = [(209, 65, 1), (64, 0, 63)]
    dps = [torch.full((B, N, 2), 7.0, device=dev) for _ in chunks]
    for k, counts in enumerate(chunks):
        f.train_points_grad(points, target, dpoints=dps[k], counts=counts, accumulate=k > 0, scale=0.5, step=k == len(chunks) - 1, order="cell")
        assert f._pass_samples == (k + 1) * N
    assert f.steps == 1
    for k, counts in enumerate(chunks):          # chunk k alone, from the same state, with the noise keys of its place in the pass
        t = twin if k == 0 else BP._build(dev, shape)[0]
        t._pass_samples = k * N
        _, alone = t.train_points_grad(points, target, counts=counts, accumulate=True, scale=0.5, step=False, order="cell")
        for b, n_b in enumerate(counts):
            assert torch.equal(dps[k][b, :n_b], alone[b, :n_b]) and bool((dps[k][b, n_b:] == 7.0).all()), (k, b)
    assert not torch.equal(dps[0][0, :64], dps[1][0, :64])


def test_the_differentiable_calls(dev):
    """``train_points_differentiable``: backward = upstream[b] * dpoints[b], summed over the fields for shared points;
    ``query_differentiable``: backward = the ``jacobian`` contraction"""
    shape, counts = (2, 2, 16), BP.COUNTS_D
    f, points, target = BP._build(dev, shape)
    twin, _, _ = BP._build(dev, shape)
    up = torch.tensor([0.5, -2.0, 3.0], device=dev)
    p = points.clone().requires_grad_(True)
    loss = f.train_points_differentiable(p, target, counts=counts, order="cell")
    (loss * up).sum().backward()
    l1, dp = twin.train_points_grad(points, target, counts=counts, order="cell")
    assert torch.equal(loss.detach(), l1) and f.steps == twin.steps == 1
    assert torch.equal(p.grad, up.reshape(B, 1, 1) * dp)
    assert all(torch.equal(a.detach(), c.detach()) for a, c in zip(f.params, twin.params))
    shared = points[0, :64].clone().requires_grad_(True)           # inside every field: one set of points for all three
    loss = f.train_points_differentiable(shared, target[:, :64].contiguous(), step=False)
    (loss * up).sum().backward()
    _, dp = f.train_points_grad(points[0, :64].contiguous(), target[:, :64].contiguous(), step=False)      # step=False: the same state, the same bits
    assert shared.grad.shape == (64, 2) and torch.equal(shared.grad, (up.reshape(B, 1, 1) * dp).sum(0))
    plain = f.train_points_differentiable(points, target, counts=counts, step=False)                 # no requires_grad: the plain call
    assert plain.grad_fn is None and plain.shape == (B,)
    # query_differentiable against the jacobian, per-field and shared points, plain and with a level of detail
    lod = torch.stack([torch.from_numpy(C.inputs(*shape, b).lod) for b in range(B)]).to(dev)
    w = torch.rand(B, N, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    for lod_arg in (None, lod, 1.25):
        p = points.clone().requires_grad_(True)
        y = f.query_differentiable(p, lod=lod_arg)
        assert torch.equal(y.detach(), f.query(points) if lod_arg is None else f.query_lod(points, lod_arg))
        (y * w).sum().backward()
        jac = f.jacobian(points, lod=lod_arg)
        assert jac.shape == (B, N, 3, 2)
        want = torch.einsum("bno,bnoa->bna", w, jac)
        err = float((p.grad - want).abs().max()) / float(want.abs().max())
        print(f"MEASURED query_differentiable against the jacobian contraction, lod={'none' if lod_arg is None else 'given'}: {err:.3e}")
        assert err <= TOL_G                      # three launches with a one-hot dy against one with w: another order of the three products
        assert torch.equal(p.grad, f.point_gradient(points, dy=w, lod=lod_arg)[1])
    s = points[1].clone().requires_grad_(True)
    (f.query_differentiable(s) * w).sum().backward()
    assert torch.equal(s.grad, f.point_gradient(points[1].contiguous(), dy=w)[1].sum(0))
    assert f.query_differentiable(points).grad_fn is None


@pytest.mark.parametrize("packed", [False, True], ids=["u8", "bits"])
def test_point_gradient_of_a_loaded_batch_is_the_loaded_fields(dev, tmp_path, packed):
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch
    f, points, target = BP._build(dev)
    paths = [tmp_path / f"f{b}.pt" for b in range(B)]
    f.save_compressed(paths, packed=packed)
    g = HashGridFieldBatch.load_compressed(paths, device=dev)
    singles = [HashGridField.load_compressed(p, device=dev, fused=True) for p in paths]
    assert g.decode_only and (g.packed is not None) == packed
    dy = (torch.rand(B, N, 3, generator=torch.Generator().manual_seed(2)) - 0.5).to(dev)
    for lod in (None, 1.25):
        y, dp = g.point_gradient(points, dy=dy, lod=lod)
        yt, dt = g.point_gradient(points, target=target, scale=LOSS_SCALE, lod=lod, order="cell")
        for b in range(B):
            y1, d1 = singles[b].point_gradient(points[b], dy=dy[b], lod=lod)
            assert torch.equal(y[b], y1) and torch.equal(dp[b], d1), (b, lod)
            y1, d1 = singles[b].point_gradient(points[b], target=target[b], scale=LOSS_SCALE, lod=lod)
            assert torch.equal(yt[b], y1) and torch.equal(dt[b], d1), (b, lod)
    assert torch.equal(g.point_gradient(points, dy=dy)[0], g.query(points))


# ---- 5. what it is for: three fields fitted while each registers its own second view
DELTAS = ((1.25, -0.75), (-0.9, 1.1), (0.6, 1.4))


def _views(dev):
    """per field DESIGN 4.7.12's two views of 2000 points in [8, 56]^2 - its own positions, its own image (the test image with swapped
    channels and axes), its own shift of the second view: (positions with theta = 0 [B, 4000, 2], colours [B, 4000, 3], mask [4000, 1])"""
    n = PT.JOINT["n"]
    p0, col = [], []
    for b, delta in enumerate(DELTAS):
        g = torch.Generator().manual_seed(PT.JOINT["seed"] + b)
        p1 = torch.rand(n, 2, generator=g, dtype=torch.float64) * 48.0 + 8.0
        p2 = torch.rand(n, 2, generator=g, dtype=torch.float64) * 48.0 + 8.0
        image = lambda p: PT.joint_image(p if b != 1 else p.flip(1)).roll(b, dims=1)
        col.append(torch.cat([image(p1), image(p2)]))
        p0.append(torch.cat([p1, p2 - torch.tensor(delta, dtype=torch.float64)]))
    mask = torch.cat([torch.zeros(n, 1), torch.ones(n, 1)])
    return torch.stack(p0).float().to(dev), torch.stack(col).float().to(dev), mask.to(dev)


def _register(step, theta, p0, mask, steps):
    opt = torch.optim.Adam([theta], lr=PT.JOINT["lr_shift"])
    first = last = None
    for _ in range(steps):
        opt.zero_grad()
        loss = step(p0 + mask * theta.reshape(-1, 1, 2) if p0.dim() == 3 else p0 + mask * theta)
        first = loss.detach().clone() if first is None else first
        last = loss.detach()
        loss.sum().backward()
        opt.step()
    return first, last


def test_three_fields_register_while_they_are_fitted(dev):
    """tests/test_gpu_hashgrid_pointtrain.py::test_two_views_register_while_the_field_is_fitted for B = 3 fields at once: field (64, 64),
    R = 4, 8, 16, 32, F = 2, table 2^12, each field its OWN two views of 2000 points and its OWN shift; 200 steps of
    ``train_points_differentiable`` (one call steps all three fields), the three shifts from 0 by ONE torch Adam at 0.05.  The conditions are
    the single-field test's, per field: final loss <= 0.01 of the first, |theta_b - delta_b|_inf <= 0.1 samples.  The same run on the three
    extracted single fields must land on the same shifts: both runs meet the condition, so they lie within 0.2 samples of each other; the
    measured difference is printed (DESIGN 4.7.21 records it)."""
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    steps = PT.JOINT["steps"]
    f = HashGridFieldBatch(B, PT.JOINT["size"], levels=4, features=2, log2_table=12, base_resolution=4, finest_resolution=32, device=dev, seed=PT.JOINT["seed"])
    assert f.resolutions == (4, 8, 16, 32)
    singles = [f.extract(b) for b in range(B)]
    p0, colours, mask = _views(dev)
    theta = torch.zeros(B, 2, device=dev, requires_grad=True)
    first, last = _register(lambda p: f.train_points_differentiable(p, colours, order="cell"), theta, p0, mask, steps)
    assert f.steps == steps
    deltas = torch.tensor(DELTAS, device=dev)
    for b in range(B):
        t1 = torch.zeros(2, device=dev, requires_grad=True)
        f1, l1 = _register(lambda p: singles[b].train_points_differentiable(p, colours[b], fused=True, order="cell"), t1, p0[b], mask, steps)
        err, err1 = float((theta[b].detach() - deltas[b]).abs().max()), float((t1.detach() - deltas[b]).abs().max())
        apart = float((theta[b] - t1).detach().abs().max())
        print(f"MEASURED registration field {b} | batch loss {float(first[b]):.4e} -> {float(last[b]):.4e} (ratio {float(last[b] / first[b]):.3e}) | theta "
              f"{theta[b].tolist()} error {err:.4f} | single loss {float(f1):.4e} -> {float(l1):.4e} theta {t1.tolist()} error {err1:.4f} | apart {apart:.2e} samples")
        assert float(last[b]) < 0.01 * float(first[b]) and err <= 0.1, (b, float(first[b]), float(last[b]), err)
        assert float(l1) < 0.01 * float(f1) and err1 <= 0.1 and apart <= 0.2, (b, err1, apart)
