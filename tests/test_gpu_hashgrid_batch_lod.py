"""GPU tests of the batch's level of detail per point (nic_hash_batch_forward_points_lod, nic_hash_batch_forward_backward_points_lod,
csrc/hashgrid_batch.hip: hash_batch_decode_lod_kernel, hash_batch_points_lod_kernel; ``HashGridFieldBatch.query_lod`` / ``resample_lod`` /
``decode_mip`` / ``train_points_lod`` / ``fit_points_lod`` / ``fit_mips``).

Training: EVERY field is held to ITS float64 reference step with ITS level of detail (oracle/hashgrid_train_ref.py, ``lod=(fade, lod_b[:n_b],
u)``), with the metric and the bounds of tests/test_hashgrid_train_ref_cpu.py untouched (``C.measure``: y and loss 5e-6, every gradient 1e-4,
the table gradient per level) and the ``Batch`` / ``finish`` discipline of tests/test_gpu_hashgrid_batch_points.py: a non-zero gradient base,
untouched entries keep their bits, sevens overwritten, rows of y past a count untouched.  The inputs are that file's B = 3 fields of 209
points with the edges of the domain, points outside, NaN and infinities, and the per-point ``lod`` of tests/test_hashgrid_train_ref_cpu.py
(NaN, a negative, a value past the clamp); tests/test_hashgrid_batch_lod_cpu.py shows on the CPU that they notice an ignored ``lod``, the
neighbour's ``lod`` and ``lod`` read at the position instead of the row, and reach every weight case.

Then bit-for-bit anchors (the single-field fused lod entries, lambda = 0 against the plain batch calls, the same call twice), stored sources
against a float64 decode of the files' bytes times the float64 level weights, and the class against the extracted fields."""
import math

import numpy as np
import pytest
import torch

from oracle import hashgrid_ref as HR
from oracle import hashgrid_train_ref as T
from oracle import make_hashgrid_golden as G
from tests import test_gpu_hashgrid_batch_points as BP
from tests import test_hashgrid_batch_lod_cpu as L
from tests import test_hashgrid_batch_points_cpu as P
from tests import test_hashgrid_train_ref_cpu as C
from tests.test_hashgrid_train_ref_cpu import LOSS_SCALE, NAMES, SHAPES, TOL_G, TOL_Y, shape_id

pytestmark = pytest.mark.gpu
B, N = C.N_FIELDS, P.N
TOL_FP32 = 5e-6                       # the bound tests/test_gpu_hashgrid_stored_ref.py applies to ``query``


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class LodBatch(BP.Batch):
    """``Batch`` with each field's own level of detail of a mode (tests/test_hashgrid_batch_lod_cpu.py, ``MODES``)"""

    def __init__(self, dev, shape, noisy, refs, mode):
        super().__init__(dev, shape, noisy, refs)
        per_field = [L.lod_of(shape, b, mode) for b in range(B)]
        self.fade, self.uniform = per_field[0][0], per_field[0][2]
        assert all(p[0] == self.fade and p[2] == self.uniform for p in per_field)         # one nic_hash_lod serves the launch
        self.lod = None if per_field[0][1] is None else torch.stack([torch.from_numpy(p[1]) for p in per_field]).to(dev)
        if self.lod is not None:
            assert len({p[1].tobytes() for p in per_field}) == B                          # every field its own: a shared or swapped slice fails

    def order(self, kind, counts):
        if kind != "perm":
            return super().order(kind, counts)
        rows = []
        for b in range(B):                      # the permutation the CPU file's teeth use; what follows a field's rows is never read
            n_b = P.count_of(counts, b)
            rows.append(torch.cat([L.permutation(b, n_b).to(torch.int32), torch.full((N - n_b,), 0x7FFFFFFF, dtype=torch.int32)]))
        return torch.stack(rows).to(self.dev)

    def run(self, counts=None, order=None, y=None):
        from neural_image_compression_v2_amd.hashgrid import hash_batch_forward_backward_points_lod
        y = torch.full((B, N, 3), 7.0, device=self.dev) if y is None else y
        hash_batch_forward_backward_points_lod(self.geo, self.tables, self.points, self.params, self.target, self.gm, self.lod, self.uniform, self.fade,
                                               table_grads=self.tg, order=self.order(order, counts), counts=counts, loss=self.loss, loss_scale=LOSS_SCALE,
                                               want_y=y, quant=self.quant)
        return y


def _refs(shape, counts, noisy, mode):
    return [L.lod_reference(shape, b, P.count_of(counts, b), noisy, mode) if P.count_of(counts, b) else None for b in range(B)]


# ---- a. every field against ITS float64 reference
@pytest.mark.parametrize("noisy", [False, True], ids=["table", "table_q"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_field_against_its_reference(dev, shape, noisy):
    h = LodBatch(dev, shape, noisy, _refs(shape, None, noisy, "point"), "point")
    h.finish(f"batch lod {shape_id(shape)} {'noisy' if noisy else 'plain'}", [h.run()], [None])


RAGGED_SHAPES = [(2, 1, 8), (3, 2, 4), (2, 4, 10)]          # a 3D one and an L F > 32 one among them


@pytest.mark.parametrize("order", [None, "perm", "cell"], ids=["unordered", "perm", "cell"])
@pytest.mark.parametrize("counts", P.COUNTS[1:], ids=["209-65-1", "64-0-63"])
@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=shape_id)
def test_ragged_counts_and_orders(dev, shape, counts, order):
    """lod is read at the field-local ROW: with an order at order[b, pos], clamped to the field's own count"""
    h = LodBatch(dev, shape, True, _refs(shape, counts, True, "point"), "point")
    h.finish(f"batch lod {shape_id(shape)} noisy counts={counts} order={order}", [h.run(counts, order)], [counts])


@pytest.mark.parametrize("order", ["perm", "cell"])
@pytest.mark.parametrize("shape", RAGGED_SHAPES, ids=shape_id)
def test_full_counts_with_an_order(dev, shape, order):
    h = LodBatch(dev, shape, False, _refs(shape, None, False, "point"), "point")
    h.finish(f"batch lod {shape_id(shape)} plain order={order}", [h.run(None, order)], [None])


@pytest.mark.parametrize("shape,noisy,mode", [((2, 2, 16), False, "uniform"), ((3, 4, 8), True, "uniform"), ((2, 4, 10), True, "skip"), ((3, 2, 4), True, "skip"),
                                              ((2, 4, 10), True, "boundary"), ((3, 8, 8), True, "boundary")],
                         ids=lambda v: v if isinstance(v, str) else (shape_id(v) if isinstance(v, tuple) else ("table_q" if v else "table")))
def test_launch_wide_levels_of_detail(dev, shape, noisy, mode):
    """lod_uniform alone (1.25); one lambda just past the second fade + 1, where whole waves skip every level but the coarsest; and a fade
    that is not monotone, where the whole wave skips the level that opens a generator block of noise columns and the block's later levels
    keep their noise (F = 4: level 4 is column 16; F = 8: column 32)"""
    h = LodBatch(dev, shape, noisy, _refs(shape, None, noisy, mode), mode)
    assert h.lod is None
    h.finish(f"batch lod {shape_id(shape)} {mode}", [h.run()], [None])


@pytest.mark.parametrize("shape", [(2, 2, 16), (3, 8, 8)], ids=shape_id)
def test_every_level_off(dev, shape):
    """lambda = 40 (clamped to 32): no level is read; the table gradient keeps its bits and the loss is the decoder's at a zero row"""
    refs = _refs(shape, None, True, "off")
    h = LodBatch(dev, shape, True, refs, "off")
    y = h.run()
    h.finish(f"batch lod {shape_id(shape)} off", [y], [None])
    assert torch.equal(h.tg.view(torch.int32), h.base.view(torch.int32))
    for b in range(B):
        f = P.field_inputs(shape, b)
        zero = T.decoder(torch.zeros(1, f.geo.width, dtype=torch.float64), [p.double() for p in f.params])
        # the reference agrees on what "off" means, up to float64 rounding: a product of 209 rows sums its 64 terms in another order than one row
        assert float((refs[b].y - zero).abs().max()) <= 64 * 2.0 ** -53
        assert float((y[b].double().cpu() - zero).abs().max()) <= TOL_Y and len({tuple(r.tolist()) for r in y[b].cpu()}) == 1


# ---- b. bit-for-bit anchors
@pytest.mark.parametrize("order", [None, "cell"], ids=["unordered", "cell"])
@pytest.mark.parametrize("shape", [(2, 2, 16), (3, 8, 8)], ids=shape_id)
def test_against_the_single_field_entries(dev, shape, order):
    """training: y[b, :n_b] is ``hash_fused_forward_backward_points_lod`` on field b's tensors bit for bit, loss and gradients within the
    bounds the sibling file applies (another summation order); forward: ``hash_fused_forward_points_lod`` bit for bit"""
    from neural_image_compression_v2_amd.hashgrid import (hash_batch_forward_points_lod, hash_fused_forward_backward_points_lod,
                                                          hash_fused_forward_points_lod)
    from tests.test_gpu_hashgrid_batch import check
    counts = (209, 65, 1)
    h = LodBatch(dev, shape, True, _refs(shape, counts, True, "point"), "point")
    h.tg.zero_()
    od = h.order(order, counts)
    y = h.run(counts, order)
    yq = hash_batch_forward_points_lod(h.geo, h.tables, h.points, h.params, h.lod, h.uniform, h.fade)
    for b, n_b in enumerate(counts):
        ps = [p[b] for p in h.params]
        gm = [torch.full_like(p, 7.0) for p in ps]
        tg = torch.zeros_like(h.tables[b])
        loss1, y1 = hash_fused_forward_backward_points_lod(h.geo, h.tables[b], h.points[b, :n_b].contiguous(), ps, h.target[b, :n_b].contiguous(), gm,
                                                           h.lod[b, :n_b].contiguous(), h.uniform, h.fade, table_grad=tg,
                                                           order=None if od is None else od[b, :n_b].contiguous(), loss_scale=LOSS_SCALE, want_y=True,
                                                           quant=h.quant)
        what = f"{shape_id(shape)} field {b} ({n_b} points)"
        assert torch.equal(y[b, :n_b], y1), f"{what}: y is not the single-field lod entry's bit for bit"
        check(h.loss[b].reshape(1), loss1.reshape(1), TOL_Y, f"{what} loss")
        check(h.tg[b], tg, TOL_G, f"{what} table gradient")
        for n, a, r in zip(NAMES, h.gm, gm):
            check(a[b], r, TOL_G, f"{what} {n}")
        q1 = hash_fused_forward_points_lod(h.geo, h.tables[b], h.points[b], ps, h.lod[b], h.uniform, h.fade)
        assert torch.equal(yq[b], q1), f"{what}: the query is not the single-field lod entry's bit for bit"


@pytest.mark.parametrize("shape", [(2, 2, 16), (2, 4, 10), (3, 4, 8)], ids=shape_id)
def test_lambda_zero_is_the_plain_call_and_the_same_call_gives_the_same_bits(dev, shape):
    """with the default fade every weight is exactly 1 at lambda = 0: y of the lod training call and the colours of the lod query are the plain
    batch calls' bit for bit; the forward entry has no atomics: twice the same bits"""
    from neural_image_compression_v2_amd.hashgrid import (hash_batch_forward_backward_points, hash_batch_forward_backward_points_lod,
                                                          hash_batch_forward_points_lod, hash_batch_forward_source)
    h = LodBatch(dev, shape, True, _refs(shape, None, True, "point"), "point")
    _, y0 = hash_batch_forward_backward_points(h.geo, h.tables, h.points, h.params, h.target, h.gm, table_grads=h.tg, loss_scale=LOSS_SCALE, want_y=True, quant=h.quant)
    for lod in (None, torch.zeros(B, N, device=dev), torch.full((N,), float("nan"), device=dev)):                  # NaN -> 0
        _, y1 = hash_batch_forward_backward_points_lod(h.geo, h.tables, h.points, h.params, h.target, h.gm, lod, 0.0, None, table_grads=h.tg,
                                                       loss_scale=LOSS_SCALE, want_y=True, quant=h.quant)
        assert torch.equal(y0, y1)
    q0 = hash_batch_forward_source(h.geo, h.tables, h.params, points=h.points)
    assert torch.equal(q0, hash_batch_forward_points_lod(h.geo, h.tables, h.points, h.params, None, 0.0, None))
    a = hash_batch_forward_points_lod(h.geo, h.tables, h.points, h.params, h.lod, 0.25, h.fade)
    assert torch.equal(a, hash_batch_forward_points_lod(h.geo, h.tables, h.points, h.params, h.lod, 0.25, h.fade)) and not torch.equal(a, q0)


# ---- c. stored sources: B files of one geometry, against a float64 decode of their bytes times the float64 level weights
STORED = {"2d_u8": dict(field_size=(44, 36), log2_table=10, base=16, levels=8, features=2, fmt="u8", bits=8),
          "2d_bits": dict(field_size=(44, 36), log2_table=10, base=16, levels=10, features=4, fmt="bits1", bits=5),
          "3d_bits": dict(field_size=(12, 10, 8), log2_table=10, base=4, levels=4, features=2, fmt="bits1", bits=4),
          "3d_u8": dict(field_size=(12, 10, 8), log2_table=10, base=4, levels=8, features=8, fmt="u8", bits=6)}
_stored = {}


def _stored_case(name, tmp_path_factory):
    if name not in _stored:
        root = tmp_path_factory.mktemp(name)
        paths, files = [], []
        for seed in (1, 2, 3):
            d = HR.make_file(dict(STORED[name], hidden=64, n_linear=3, scale=1.5), seed)
            paths.append(str(root / f"seed{seed}.pt"))
            HR.save(d, paths[-1])
            files.append(HR.parse(d))
        _stored[name] = (paths, files)
    return _stored[name]


def _reference_colours(f, points, fade, lod, uniform):
    """float64: the rows of the file's bytes at the points, each level times its float64-held fp32 weight, through the file's decoder"""
    rows = HR.rows_points(f, points)
    a = T.level_weights(f, points.shape[0], fade, lod, uniform)
    return HR.decoder(rows * np.repeat(a, f.features, axis=1), f)


@pytest.mark.parametrize("name", list(STORED))
def test_stored_batches_against_the_reference_and_the_single_fields(dev, tmp_path_factory, name):
    from neural_image_compression_v2_amd.hashgrid import HashGridField, HashGridFieldBatch
    from tests.test_gpu_hashgrid_stored_ref import hold, same_points
    paths, files = _stored_case(name, tmp_path_factory)
    f0 = files[0]
    batch = HashGridFieldBatch.load_compressed(paths, device=dev)
    singles = [HashGridField.load_compressed(p, device=dev, fused=True) for p in paths]
    assert batch.decode_only and batch.n_fields == 3 and all(s.route == "fused" for s in singles)
    fade = T.default_fade(f0)
    assert batch.lod_fade == singles[0].lod_fade == fade
    points = np.stack([G.query_points(f.field_size, f.resolutions, seed=s) for s, f in zip((1, 2, 3), files)])
    g = torch.Generator().manual_seed(5)
    lod = (torch.rand(3, N, generator=g) * (max(fade) + 1.5)).numpy().astype(np.float32)
    lod[:, :3] = (np.nan, -3.0, 40.0)
    pts, lod_t = torch.from_numpy(points).to(dev), torch.from_numpy(lod).to(dev)
    # query: a lod per field, a shared one, a float
    for what, arg, per_field in (("[B, N]", lod_t, lambda b: (lod[b], 0.0)), ("[N]", lod_t[1].contiguous(), lambda b: (lod[1], 0.0)), ("1.25", 1.25, lambda b: (None, 1.25))):
        y = batch.query_lod(pts, arg)
        for b, f in enumerate(files):
            hold(y[b], _reference_colours(f, points[b], fade, *per_field(b)), TOL_FP32, f"{name} query_lod {what} field {b}")
            one = singles[b].query(pts[b], lod=arg[b].contiguous() if what == "[B, N]" else arg)
            assert torch.equal(y[b], one), f"{name} query_lod {what} field {b}: not the single field's bits"
    # resample(lod="auto") and decode_mip(1)
    size = tuple(max(1, s // 3) for s in f0.field_size)
    same_points(batch, f0, size)
    auto = max(0.0, math.log2(max(s / v for s, v in zip(f0.field_size, size))))
    mip = tuple(s // 2 for s in f0.field_size)
    for what, y, sz, lam, tile in (("resample_lod auto", batch.resample_lod(size), size, auto, None), ("resample_lod auto tile=5", batch.resample_lod(size, tile=5), size, auto, 5),
                                   ("decode_mip(1)", batch.decode_mip(1), mip, 1.0, None)):
        assert tuple(y.shape) == (3, *sz, 3), what
        p = HR.resample_points(f0, sz)
        for b, f in enumerate(files):
            hold(y[b].reshape(-1, 3), _reference_colours(f, p, fade, None, lam), TOL_FP32, f"{name} {what} field {b}")
            if tile is None:
                one = singles[b].decode_mip(1) if what.startswith("decode_mip") else singles[b].resample(sz, lod="auto")
                assert torch.equal(y[b], one), f"{name} {what} field {b}: not the single field's bits"
    # an assigned fade reaches the kernel and the extracted field
    custom = tuple(float(v) for v in np.linspace(2.5, 0.25, f0.levels).astype(np.float32))
    batch.lod_fade = custom
    y = batch.query_lod(pts, lod_t)
    for b, f in enumerate(files):
        hold(y[b], _reference_colours(f, points[b], custom, lod[b], 0.0), TOL_FP32, f"{name} query_lod custom fade field {b}")
    assert batch.extract(1).lod_fade == custom and torch.equal(batch.extract(1).query(pts[1], lod=lod_t[1].contiguous()), y[1])


# ---- d. the class
def test_train_points_lod_is_the_extracted_fields(dev):
    """one step with ragged counts and a lod per field against ``extract(b).train_points(fused=True, lod=)`` from the same state: the comparison
    the sibling file makes for the plain call"""
    from tests.test_gpu_hashgrid_batch import check
    shape = (2, 2, 16)
    f, points, target = BP._build(dev, shape)
    lod = torch.stack([torch.from_numpy(C.inputs(*shape, b).lod) for b in range(B)]).to(dev)
    singles, stepped = [f.extract(b) for b in range(B)], [f.extract(b) for b in range(B)]
    counts = BP.COUNTS_D
    losses = f.train_points_lod(points, target, lod, counts=counts, step=False, order="cell")
    assert losses.shape == (B,) and f.steps == 0 and f._pass_samples == N and not f._grad_clean
    for b, n_b in enumerate(counts):
        s = singles[b]
        l1 = s.train_points(points[b, :n_b].contiguous(), target[b, :n_b].contiguous(), fused=True, step=False, order="cell", lod=lod[b, :n_b].contiguous())
        what = f"train_points_lod field {b} ({n_b} points)"
        check(losses[b].reshape(1), l1.reshape(1), TOL_Y, f"{what} loss")
        check(f.tables.grad[b], s.table.grad, TOL_G, f"{what} table gradient")
        for n, a, r in zip(NAMES, f._gm, s._fused_gm):
            check(a[b], r, TOL_G, f"{what} {n}")
    f.apply_step()
    assert f.steps == 1 and bool((f.tables.grad == 0).all())
    for b, n_b in enumerate(counts):
        s = stepped[b]
        s.train_points(points[b, :n_b].contiguous(), target[b, :n_b].contiguous(), fused=True, order="cell", lod=lod[b, :n_b].contiguous())
        check(f.tables.detach()[b], s.table.detach(), TOL_G, f"field {b} table after the step")
        for n, a, r in zip(NAMES, f.params, s.decoder.linear_params()):
            check(a.detach()[b], r.detach(), TOL_G, f"field {b} {n[1:]} after the step")
    # a float and a shared tensor take the same launch; lod = 0 is the plain step's loss bit for bit in y's sense: the same forward
    a, _, _ = BP._build(dev, shape)
    c, _, _ = BP._build(dev, shape)
    la = a.train_points_lod(points, target, 0.0, noise=False, step=False)
    lc = c.train_points(points, target, noise=False, step=False)
    check(la, lc, TOL_Y, "lod 0.0 against the plain step")
    assert f.lod_fade == singles[0].lod_fade


MIP_SIZE, MIP_EPOCHS, MIP_BITS = (32, 32), 20, 6


def test_fit_mips_is_the_extracted_fields_fit_mips(dev):
    """three 32 x 32 images, L 4, T 2^10, mips 0 .. 2, 20 epochs with ``num_bits`` so that the freeze schedule runs: each field's final loss
    against ``HashGridField.fit_mips(fused=True)`` of the extracted field, with the bound and construction of
    tests/test_gpu_hashgrid_batch_points.py::test_fit_points_is_the_extracted_fields_fit: two repeats of the single-field fit from one state
    give a spread s = |ln(l1 / l2)| (the order of its atomics); the batch must lie within s + ln(1 + 10 %) of the repeats' geometric mean."""
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    from tests.test_gpu_hashgrid_batch import _image
    targets = torch.stack([_image(MIP_SIZE, dev, b) for b in range(B)]).contiguous()
    f = HashGridFieldBatch(B, MIP_SIZE, levels=4, features=2, log2_table=10, device=dev, seed=3, num_bits=MIP_BITS)
    repeats = [[f.extract(b) for b in range(B)] for _ in range(2)]
    hist = f.fit_mips(targets, MIP_EPOCHS, mips=2)
    n_points = 32 * 32 + 16 * 16 + 8 * 8
    assert len(hist) == MIP_EPOCHS and len(hist[0]) == B and f.steps == MIP_EPOCHS and f.frozen and f._pass_samples == n_points
    for b in range(B):
        finals = [s[b].fit_mips(targets[b], MIP_EPOCHS, mips=2, fused=True)[-1] for s in repeats]
        spread = abs(math.log(finals[0] / finals[1]))
        off = abs(math.log(hist[-1][b] / math.sqrt(finals[0] * finals[1])))
        print(f"MEASURED fit_mips field {b} | first loss {hist[0][b]:.4e} | batch {hist[-1][b]:.6e} | single {finals[0]:.6e} {finals[1]:.6e} | "
              f"spread {spread:.3e} | batch off the mean by {off:.3e} | admitted {spread + math.log(1 + BP.FIT_MARGIN):.3e}")
        assert hist[-1][b] < hist[0][b] and repeats[0][b].frozen and repeats[0][b].steps == MIP_EPOCHS
        assert off <= spread + math.log(1 + BP.FIT_MARGIN), (b, hist[-1][b], finals)
    # the mips the fit trained: shapes, and resample_lod("auto") picks lambda as the single field does
    one = f.extract(0)
    for m, side in ((0, 32), (1, 16), (2, 8)):
        y = f.decode_mip(m)
        assert tuple(y.shape) == (B, side, side, 3) and torch.equal(y[0], one.decode_mip(m))
    for size in ((16, 16), (20, 12), (40, 40)):
        lam = max(0.0, math.log2(max(32 / v for v in size)))
        y = f.resample_lod(size)
        assert tuple(y.shape) == (B, *size, 3) and torch.equal(y, f.resample_lod(size, lam)) and torch.equal(y[0], one.resample(size, lod="auto"))
    assert torch.equal(f.resample_lod((40, 40)), f.resample((40, 40)))                   # lambda = 0 with the default fade: the plain launch's colours
