"""GPU tests of the batch's gradients with respect to the level of detail (nic_hash_batch_points_grad_lod, csrc/hashgrid_batch_grad.hip;
nic_hash_batch_forward_backward_points_grad_lod, csrc/hashgrid_batch.hip; HashGridFieldBatch.point_gradient_lod / jacobian_lod /
query_differentiable_lod / train_points_grad_lod / train_points_differentiable_lod).  Inputs are
tests/test_hashgrid_batch_lodgrad_cpu.py's: B = 3 fields of 130 rows on the geometries of tests/test_hashgrid_lodgrad_cpu.py (13 x 9 and 7 x 6 x 5,
log2_table 10, dense and hashed levels, L F up to 40: both KT), every field with rows exactly on every kink, a whole wave with every level off,
points outside and a NaN; counts full, (130, 65, 1) and (64, 0, 63); no order, a fixed permutation and "cell"; lambda per point, launch-wide
and both.  The reference of field b is ``reference_step`` (tests/test_hashgrid_lodtrain_cpu.py) on field b's own tensors and first n_b rows.
TOL_G = 1e-4 of the largest magnitude of the compared tensor, the project's bound since 4.7.21.

1. the gradient entry from fp32, uint8 (b = 8) and bit-packed (b = 4) stacks: dlod and dpoints against each field's reference (on the
   dequantised table), y / dpoints / owned dlod rows bit for bit nic_hash_fused_points_grad_lod's, y / dpoints nic_hash_batch_points_grad's;
2. the training entry without noise: loss, y, decoder gradients and dpoints bit for bit nic_hash_batch_forward_backward_points_grad's, the
   table gradient within 1e-5, dlod bit for bit entry 1's with target= and nic_hash_fused_forward_backward_points_grad_lod's per field;
3. the training entry with noise (b = 4 and 8) against each field's reference with its noise key; the noise is in dlod; every order the same bits;
4. write behaviour: sentinels, exact zeros, NIC_HASH_FUSED_ADD_GRADS, the same bits twice, a frozen batch;
5. the class against ``extract(b)``'s methods; 6. what it is for: (a) a lambda per field recovered with the fields held, (b) 20 joint steps."""
import pytest
import torch

from tests import test_hashgrid_lodgrad_cpu as L
from tests.test_hashgrid_batch_lodgrad_cpu import B, COUNTS, LOSS_SCALE, batch_inputs, close, count_of, field_lod, field_reference, permutation, stacked
from tests.test_hashgrid_lodgrad_cpu import CASES, MODES, N, TOL_G
from tests.test_hashgrid_lodtrain_cpu import NOISE_KEYS, reference_step

pytestmark = pytest.mark.gpu

TOL_Y, TOL_ORDER = 5e-6, 1e-5               # y against the reference (absolute); the table gradient against the sibling's (the atomics' order, 4.7.12)
SOURCES = [("f32", None), ("u8", 8), ("bits", 4)]
ORDERS = (None, "perm", "cell")
SENTINEL = -12345.5
# test 6b: 10 x the largest deviation of the batch's trajectories from the three extracted fields' over the 20 steps as recorded in DESIGN
# 4.7.25 (room for the order of the table atomics across runs) - lambda: none seen, so the resolution of the comparison, one fp32 ulp of the
# values in [2, 4) = 2.4e-7, stands for it; the shift 3.0e-8 samples; the loss 1.0e-6 of its value.  No bound may be looser than 1e-3
JOINT_BOUND = {"lambda": 2.4e-6, "shift": 3.0e-7, "loss": 1.0e-5}
JOINT_CEILING = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Harness:
    """the three fields of a case on the device, stacked"""

    def __init__(self, case, dev):
        from neural_image_compression_v2_amd import hashgrid as hg
        self.bi = bi = batch_inputs(case)
        self.case, self.dev, self.geo, self.fade = case, dev, bi.geo, bi.fade
        self.tables, self.params = stacked(bi, "table").to(dev), [p.to(dev) for p in stacked(bi, "params")]
        self.points, self.target, self.dy = stacked(bi, "points").to(dev), stacked(bi, "target").to(dev), stacked(bi, "dy").to(dev)
        self.lod = stacked(bi, "lod").to(dev)
        self.cell = {c: hg.hash_batch_point_order(bi.geo, self.points, c) for c in COUNTS}

    def order(self, name, counts):
        if name is None:
            return None
        if name == "cell":
            return self.cell[counts]
        rows = torch.arange(N, dtype=torch.int32).repeat(B, 1)
        for b in range(B):
            n_b = count_of(counts, b)
            if n_b:
                rows[b, :n_b] = permutation(b, n_b).to(torch.int32)
        return rows.to(self.dev)

    def lod_kw(self, mode):
        per_point, u = MODES[mode]
        return dict(lod=self.lod if per_point else None, lod_uniform=u, fade=self.fade)

    def single_lod_kw(self, mode, b, n_b):
        per_point, u = MODES[mode]
        return dict(lod=self.lod[b, :n_b].contiguous() if per_point else None, lod_uniform=u, fade=self.fade)

    def source(self, kind, bits):
        """(stacked data, per-field fp32 [L, T, F] values the forward blends, on the CPU)"""
        from neural_image_compression_v2_amd import hashgrid as hg
        from neural_image_compression_v2_amd import models
        if kind == "f32":
            return self.tables, [f.table for f in self.bi.fields]
        clamped = [models.quantize_clamp(self.tables[b], bits) for b in range(B)]
        stored = [hg.hash_pack_u8(self.geo, c, bits) for c in clamped]
        data = stored if kind == "u8" else [hg.hash_pack_bits(self.geo, c, bits) for c in clamped]
        return torch.stack(data).contiguous(), [hg._table_of_u8(self.geo, s, bits).cpu() for s in stored]

    def train(self, fn, counts, order, mode, frozen=False, **more):
        """one call of a training entry from zeroed gradient buffers: (loss, y, decoder gradients, table gradients or None, the rest)"""
        gm = [torch.zeros_like(p) for p in self.params]
        tg = None if frozen else torch.zeros_like(self.tables)
        kw = self.lod_kw(mode)
        out = fn(self.geo, self.tables, self.points, self.params, self.target, gm, kw["lod"], kw["lod_uniform"], kw["fade"], table_grads=tg,
                 order=self.order(order, counts), counts=counts, loss_scale=LOSS_SCALE, want_y=True, **more)
        return out[0], out[1], gm, tg, out[2:]


_HARNESS = {}


def harness(case, dev):
    if case not in _HARNESS:
        _HARNESS[case] = Harness(case, dev)
    return _HARNESS[case]


def _check_zeros(dlod, ref):
    """rows with no level on the ramp, or whose lambda_raw is < 0, >= 32 or NaN, are exactly 0 (compared as bits: -0.0 is not 0.0f)"""
    flat = torch.from_numpy(~ref.passes | ~ref.ramp.any(axis=1))
    assert bool((dlod.cpu().view(torch.int32)[flat] == 0).all()) and bool(torch.isfinite(dlod).all())


def _stored_reference(h, values, b, n_b, mode):
    f = h.bi.fields[b]
    lod, u = field_lod(h.bi, b, mode, n_b)
    return reference_step(h.bi.tgeo, values[b], f.params, f.points[:n_b], h.fade, lod, u, target=f.target[:n_b], loss_scale=LOSS_SCALE)


# ---- 1. the gradient entry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bits", SOURCES, ids=[s[0] for s in SOURCES])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_gradient_entry_per_field_against_its_reference_and_the_siblings(dev, case, kind, bits):
    from neural_image_compression_v2_amd import hashgrid as hg
    h = harness(case, dev)
    data, values = h.source(kind, bits)
    worst = {"dlod": 0.0, "dpoints": 0.0, "y": 0.0}
    for counts in COUNTS:
        for mode in MODES:
            kw = h.lod_kw(mode)
            refs = [None if count_of(counts, b) == 0 else field_reference(case, b, count_of(counts, b), mode) if kind == "f32" else
                    _stored_reference(h, values, b, count_of(counts, b), mode) for b in range(B)]
            first = None
            for order in ORDERS:
                what = (kind, counts, mode, order)
                od = h.order(order, counts)
                y, dp, dl = hg.hash_batch_points_grad_lod(h.geo, data, h.points, h.params, target=h.target, loss_scale=LOSS_SCALE, counts=counts, order=od,
                                                          kind=kind, num_bits=bits, **kw)
                assert dl.shape == (B, N) and dl.dtype == torch.float32 and dp.shape == (B, N, case[0])
                ys, dps = hg.hash_batch_points_grad(h.geo, data, h.points, h.params, target=h.target, loss_scale=LOSS_SCALE, counts=counts, order=od,
                                                    kind=kind, num_bits=bits, **kw)
                assert torch.equal(y, ys) and torch.equal(dp, dps), what                 # the sibling's bits
                first = (y, dp, dl) if first is None else first
                assert all(torch.equal(a, c) for a, c in zip((y, dp, dl), first)), what   # the lane a row lands on changes nothing
                for b in range(B):
                    n_b = count_of(counts, b)
                    assert bool((dl[b, n_b:].view(torch.int32) == 0).all()) and bool((dp[b, n_b:] == 0).all()), what   # fresh tensors: zero where nothing is written
                    if n_b == 0:
                        continue
                    ref = refs[b]
                    e = {"dlod": close(dl[b, :n_b], ref.dlod), "dpoints": close(dp[b, :n_b], ref.dpoints),
                         "y": float((y[b, :n_b].double().cpu() - ref.y).abs().max())}
                    worst = {k: max(worst[k], v) for k, v in e.items()}
                    assert e["dlod"] < TOL_G and e["dpoints"] < TOL_G and e["y"] <= TOL_Y, (what, b, e)
                    _check_zeros(dl[b, :n_b], ref)
                    if order is None:                                                    # field b's tensors through the single-field entry
                        y1, dp1, dl1 = hg.hash_fused_points_grad_lod(h.geo, data[b], h.points[b, :n_b].contiguous(), [p[b] for p in h.params],
                                                                     target=h.target[b, :n_b].contiguous(), loss_scale=LOSS_SCALE, kind=kind, num_bits=bits,
                                                                     **h.single_lod_kw(mode, b, n_b))
                        assert torch.equal(y[b, :n_b], y1) and torch.equal(dp[b, :n_b], dp1) and torch.equal(dl[b, :n_b], dl1), (what, b)
    # with dy: the single-field entry's bits again
    kw = h.lod_kw("both")
    y, dp, dl = hg.hash_batch_points_grad_lod(h.geo, data, h.points, h.params, dy=h.dy, kind=kind, num_bits=bits, **kw)
    for b in range(B):
        y1, dp1, dl1 = hg.hash_fused_points_grad_lod(h.geo, data[b], h.points[b], [p[b] for p in h.params], dy=h.dy[b], kind=kind, num_bits=bits,
                                                     **h.single_lod_kw("both", b, N))
        assert torch.equal(y[b], y1) and torch.equal(dp[b], dp1) and torch.equal(dl[b], dl1), b
    print(f"gradient entry {case} {kind}: dlod {worst['dlod']:.3e}, dpoints {worst['dpoints']:.3e} of the reference's largest magnitude; y {worst['y']:.3e}")


# ---- 2. the training entry, noise off -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=str)
def test_training_entry_without_noise_against_the_siblings(dev, case):
    from neural_image_compression_v2_amd import hashgrid as hg
    h = harness(case, dev)
    worst = {"dlod": 0.0, "dpoints": 0.0, "table": 0.0}
    for counts in COUNTS:
        for mode in MODES:
            kw = h.lod_kw(mode)
            for order in ORDERS:
                what = (counts, mode, order)
                loss_s, y_s, gm_s, tg_s, (dp_s,) = h.train(hg.hash_batch_forward_backward_points_grad, counts, order, mode)
                loss, y, gm, tg, (dp, dl) = h.train(hg.hash_batch_forward_backward_points_grad_lod, counts, order, mode)
                assert torch.equal(loss, loss_s) and torch.equal(y, y_s) and all(torch.equal(a, c) for a, c in zip(gm, gm_s)), what
                assert torch.equal(dp, dp_s), what
                e_t = float((tg - tg_s).abs().max() / tg_s.abs().max())
                worst["table"] = max(worst["table"], e_t)
                assert e_t <= TOL_ORDER, (what, e_t)
                _, _, dl_alone = hg.hash_batch_points_grad_lod(h.geo, h.tables, h.points, h.params, target=h.target, loss_scale=LOSS_SCALE, counts=counts,
                                                               order=h.order(order, counts), **kw)
                assert torch.equal(dl, dl_alone), what                                   # entry 1's bits: the two kernels' row gradients are bit-equal
                for b in range(B):
                    n_b = count_of(counts, b)
                    if n_b == 0:
                        continue
                    ref = field_reference(case, b, n_b, mode)
                    e_l, e_p = close(dl[b, :n_b], ref.dlod), close(dp[b, :n_b], ref.dpoints)
                    worst.update(dlod=max(worst["dlod"], e_l), dpoints=max(worst["dpoints"], e_p))
                    assert e_l < TOL_G and e_p < TOL_G, (what, b, e_l, e_p)
                    _check_zeros(dl[b, :n_b], ref)
                    if order is None:
                        pb = [p[b].contiguous() for p in h.params]
                        out = hg.hash_fused_forward_backward_points_grad_lod(
                            h.geo, h.tables[b], h.points[b, :n_b].contiguous(), pb, h.target[b, :n_b].contiguous(), [torch.zeros_like(p) for p in pb],
                            table_grad=torch.zeros_like(h.tables[b]), loss_scale=LOSS_SCALE, **h.single_lod_kw(mode, b, n_b))
                        assert torch.equal(dl[b, :n_b], out[3]) and torch.equal(dp[b, :n_b], out[2]), (what, b)
    print(f"training entry, no noise {case}: dlod {worst['dlod']:.3e}, dpoints {worst['dpoints']:.3e} of the reference; table gradient "
          f"{worst['table']:.3e} of the sibling's")


# ---- 3. the training entry, noise on --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_training_entry_with_noise_against_each_fields_reference(dev, case, bits):
    from neural_image_compression_v2_amd import hashgrid as hg
    h = harness(case, dev)
    key = NOISE_KEYS[bits]
    worst = {"y": 0.0, "dlod": 0.0, "dpoints": 0.0, "table": 0.0}
    for counts in COUNTS:
        for mode in MODES:
            _, _, _, _, (_, dl_off) = h.train(hg.hash_batch_forward_backward_points_grad_lod, counts, None, mode)
            first = None
            for order in ORDERS:
                what = (counts, mode, order)
                _, y, _, tg, (dp, dl) = h.train(hg.hash_batch_forward_backward_points_grad_lod, counts, order, mode, quant=key)
                first = dl if first is None else first
                assert torch.equal(dl, first), what                                      # noise is keyed by the field-local row, whatever the order
                for b in range(B):
                    n_b = count_of(counts, b)
                    if n_b == 0:
                        assert bool((tg[b] == 0).all()), what
                        continue
                    ref = field_reference(case, b, n_b, mode, bits)
                    e = {"y": float((y[b, :n_b].double().cpu() - ref.y).abs().max()), "dlod": close(dl[b, :n_b], ref.dlod),
                         "dpoints": close(dp[b, :n_b], ref.dpoints), "table": 0.0}
                    for l, want in enumerate(ref.table_grad):
                        e["table"] = max(e["table"], close(tg[b, l], want))
                    worst = {k: max(worst[k], v) for k, v in e.items()}
                    assert e["y"] <= TOL_Y and e["dlod"] < TOL_G and e["dpoints"] < TOL_G and e["table"] < TOL_G, (what, b, e)
                    _check_zeros(dl[b, :n_b], ref)
                    if bool((ref.ramp.any(axis=1) & ref.passes).any()):
                        assert not torch.equal(dl[b, :n_b], dl_off[b, :n_b]), (what, b)    # the noise is in it
                    if order is None:
                        pb = [p[b].contiguous() for p in h.params]
                        out = hg.hash_fused_forward_backward_points_grad_lod(
                            h.geo, h.tables[b], h.points[b, :n_b].contiguous(), pb, h.target[b, :n_b].contiguous(), [torch.zeros_like(p) for p in pb],
                            table_grad=torch.zeros_like(h.tables[b]), loss_scale=LOSS_SCALE, quant=key, **h.single_lod_kw(mode, b, n_b))
                        assert torch.equal(dl[b, :n_b], out[3]), (what, b)
    print(f"training entry, b = {bits} {case}: y {worst['y']:.3e}; dlod {worst['dlod']:.3e}, dpoints {worst['dpoints']:.3e}, table gradient "
          f"{worst['table']:.3e} of the reference")


# ---- 4. write behaviour ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", COUNTS, ids=str)
@pytest.mark.parametrize("case", [(2, 2, 4), (3, 8, 5)], ids=str)
def test_write_behaviour(dev, case, counts):
    from neural_image_compression_v2_amd import hashgrid as hg
    h = harness(case, dev)
    dim = case[0]
    key = NOISE_KEYS[4]
    y, dp, dl = (torch.full((B, N, 3), SENTINEL, device=dev), torch.full((B, N, dim), SENTINEL, device=dev), torch.full((B, N), SENTINEL, device=dev))
    more = dict(quant=key, dpoints=dp, dlod=dl)
    gm = [torch.zeros_like(p) for p in h.params]
    tg = torch.zeros_like(h.tables)
    kw = h.lod_kw("point")
    args = (h.geo, h.tables, h.points, h.params, h.target, gm, kw["lod"], kw["lod_uniform"], kw["fade"])
    common = dict(order=h.order("perm", counts), counts=counts, loss_scale=LOSS_SCALE, want_y=y)
    out = hg.hash_batch_forward_backward_points_grad_lod(*args, table_grads=tg, **common, **more)
    assert out[1] is y and out[2] is dp and out[3] is dl
    for b in range(B):
        n_b = count_of(counts, b)
        for t in (y, dp, dl):
            assert bool((t[b, :n_b] != SENTINEL).all()) and bool((t[b, n_b:] == SENTINEL).all()), (b, n_b)      # owned rows overwritten, nothing at or past n_b touched
        if n_b:
            ref = field_reference(case, b, n_b, "point", 4)
            _check_zeros(dl[b, :n_b], ref)
            assert close(dl[b, :n_b], ref.dlod) < TOL_G
    first = [t.clone() for t in (y, dp, dl)]
    loss1, gm1 = out[0].clone(), [g.clone() for g in gm]
    # a second identical call under NIC_HASH_FUSED_ADD_GRADS: the decoder gradients add up, y / dpoints / dlod are overwritten with the same bits
    hg.hash_batch_forward_backward_points_grad_lod(*args, table_grads=None, add_grads=True, **common, **more)
    assert all(torch.equal(t, f0) for t, f0 in zip((y, dp, dl), first))
    assert all(torch.equal(g, g1 + g1) for g, g1 in zip(gm, gm1)) and bool((gm1[0] != 0).any())
    # a frozen batch (table_grads = None) from zeroed buffers: the unfrozen call's loss, records, dpoints and dlod; the gradient entry twice
    gm_f = [torch.zeros_like(p) for p in h.params]
    out_f = hg.hash_batch_forward_backward_points_grad_lod(h.geo, h.tables, h.points, h.params, h.target, gm_f, kw["lod"], kw["lod_uniform"], kw["fade"],
                                                           table_grads=None, quant=key, **{**common, "want_y": True})
    assert torch.equal(out_f[0], loss1) and all(torch.equal(a, c) for a, c in zip(gm_f, gm1))
    for b in range(B):
        n_b = count_of(counts, b)
        assert torch.equal(out_f[2][b, :n_b], dp[b, :n_b]) and torch.equal(out_f[3][b, :n_b], dl[b, :n_b])
        assert bool((out_f[3][b, n_b:].view(torch.int32) == 0).all())
    y2, dp2, dl2 = (torch.full_like(y, SENTINEL), torch.full_like(dp, SENTINEL), torch.full_like(dl, SENTINEL))
    for _ in range(2):
        hg.hash_batch_points_grad_lod(h.geo, h.tables, h.points, h.params, target=h.target, loss_scale=LOSS_SCALE, counts=counts,
                                      order=common["order"], want_y=y2, dpoints=dp2, dlod=dl2, **kw)
        again = [t.clone() for t in (y2, dp2, dl2)] if _ == 0 else again
    assert all(torch.equal(t, a) for t, a in zip((y2, dp2, dl2), again))
    for b in range(B):
        n_b = count_of(counts, b)
        for t in (y2, dp2, dl2):
            assert bool((t[b, :n_b] != SENTINEL).all()) and bool((t[b, n_b:] == SENTINEL).all()), (b, n_b)


# ---- 5. the class ---------------------------------------------------------------------------------------------------------------------------
def _batch(dev, num_bits=4, seed=11):
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    f = HashGridFieldBatch(B, (40, 27), levels=4, features=2, log2_table=10, base_resolution=4, device=dev, seed=seed, num_bits=num_bits)
    with torch.no_grad():
        f.tables.uniform_(-0.4, 0.4, generator=torch.Generator(device=dev).manual_seed(seed))
        for p in f.params:
            p.mul_(3.0)                                                    # decoders that do something with their input
    return f


def _class_inputs(dev, n=200):
    g = torch.Generator().manual_seed(2)
    pts = (torch.rand(B, n, 2, generator=g) * torch.tensor([42.0, 29.0]) - 1.5).contiguous()       # some outside the field
    lod = (torch.rand(B, n, generator=g) * 4.5).contiguous()
    lod[:, :4] = torch.tensor([0.0, -1.0, 40.0, float("nan")])
    return pts.to(dev), lod.to(dev), torch.rand(B, n, 3, generator=g).to(dev), (torch.rand(B, n, 3, generator=g) * 2 - 1).to(dev)


def _lod_of_field(lod, b):
    return lod[b].contiguous() if isinstance(lod, torch.Tensor) and lod.dim() == 2 else lod


def test_the_gradient_methods_are_the_extracted_fields(dev, tmp_path):
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    f = _batch(dev)
    pts, lod, target, dy = _class_inputs(dev)
    n = pts.shape[1]
    f.freeze()
    paths = [tmp_path / f"f{b}.pt" for b in range(B)]
    f.save_compressed(paths, packed=True)
    loaded = HashGridFieldBatch.load_compressed(paths, device=dev)
    for batch in (f, loaded):                                             # trained and load_compressed batches
        singles = [batch.extract(b) for b in range(B)]
        for lod_arg in (1.25, lod[0].contiguous(), lod):                  # a float, a shared [N], a [B, N]
            y, dp, dl = batch.point_gradient_lod(pts, lod_arg, dy=dy)
            yt, dpt, dlt = batch.point_gradient_lod(pts, lod_arg, target=target, scale=3.0, order="cell")
            ys, dps = batch.point_gradient(pts, dy=dy, lod=lod_arg)
            assert torch.equal(y, ys) and torch.equal(dp, dps) and dl.shape == (B, n)
            jac = batch.jacobian_lod(pts, lod_arg)
            assert jac.shape == (B, n, 3)
            for b in range(B):
                l1 = _lod_of_field(lod_arg, b)
                y1, dp1, dl1 = singles[b].point_gradient_lod(pts[b], l1, dy=dy[b])
                assert torch.equal(y[b], y1) and torch.equal(dp[b], dp1) and torch.equal(dl[b], dl1), b
                y1, dp1, dl1 = singles[b].point_gradient_lod(pts[b], l1, target=target[b], scale=3.0)
                assert torch.equal(yt[b], y1) and torch.equal(dpt[b], dp1) and torch.equal(dlt[b], dl1), b
                assert torch.equal(jac[b], singles[b].jacobian_lod(pts[b], l1)), b
        # query_differentiable_lod: dlod for a [B, N] lod, its sum over the fields for a shared [N], over everything for a 0-dim tensor
        for lod_arg in (lod, lod[0].contiguous(), torch.tensor(1.25, device=dev)):
            _, dp, dl = batch.point_gradient_lod(pts, lod_arg, dy=dy)
            p_leaf, l_leaf = pts.clone().requires_grad_(True), lod_arg.clone().requires_grad_(True)
            out = batch.query_differentiable_lod(p_leaf, l_leaf)
            assert torch.equal(out.detach(), batch.query_lod(pts, lod_arg))
            (out * dy).sum().backward()
            want = dl if lod_arg.dim() == 2 else dl.sum(0) if lod_arg.dim() == 1 else dl.sum()
            assert l_leaf.grad.shape == lod_arg.shape and torch.equal(l_leaf.grad, want) and torch.equal(p_leaf.grad, dp)
            assert bool((l_leaf.grad != 0).any())
            if lod_arg.dim() == 0:                                        # the single fields' own backward, summed
                total = 0.0
                for b in range(B):
                    l1 = lod_arg.clone().requires_grad_(True)
                    (singles[b].query_differentiable_lod(pts[b], l1) * dy[b]).sum().backward()
                    total += float(l1.grad)
                assert abs(float(l_leaf.grad) - total) <= 1e-4 * float(dl.abs().sum())
        shared = pts[0].clone().requires_grad_(True)                      # shared points: dpoints summed over the fields
        l_leaf = lod.clone().requires_grad_(True)
        (batch.query_differentiable_lod(shared, l_leaf) * dy).sum().backward()
        _, dp, dl = batch.point_gradient_lod(pts[0].contiguous(), lod, dy=dy)
        assert torch.equal(shared.grad, dp.sum(0)) and torch.equal(l_leaf.grad, dl)
        plain = batch.query_differentiable_lod(pts, lod)
        assert plain.grad_fn is None and torch.equal(plain, batch.query_lod(pts, lod))
    with pytest.raises(RuntimeError, match="decode-only"):
        loaded.train_points_grad_lod(pts, target, lod)


@pytest.mark.parametrize("num_bits", [None, 4])
def test_train_points_grad_lod_is_the_extracted_fields_and_the_siblings_step(dev, num_bits):
    """One step against ``train_points_grad(lod=)`` on a copy of the batch and against the extracted fields.  Tables, optimiser moments and
    step counts are the sibling's bit for bit where that is a property the sibling has with itself: the table gradient is summed by atomics,
    so two identical calls agree in every bit only while ONE wave does all of a field's adds (at most 64 points a field: the first pass
    below).  With more waves per field (the second pass: 200 / 65 / 1 points) the hardware orders the adds: the decoders and their moments,
    which come from the fixed-order reduction, are still the sibling's bits, and the tables are held to 4.7.12's 1e-5 of the largest update
    (the count of differing values and the deviation are printed)."""
    pts_all, lod_all, target_all, _ = _class_inputs(dev)
    for n, counts in ((64, (64, 33, 1)), (200, (200, 65, 1))):
        pts, lod, target = pts_all[:, :n].contiguous(), lod_all[:, :n].contiguous(), target_all[:, :n].contiguous()
        for lod_arg in (1.25, lod[0].contiguous(), lod):
            a, c = _batch(dev, num_bits), _batch(dev, num_bits)
            before = a.tables.detach().clone()
            singles = [a.extract(b) for b in range(B)]
            dp, dl = torch.full((B, n, 2), 9.0, device=dev), torch.full((B, n), 9.0, device=dev)
            la, out_p, out_l = a.train_points_grad_lod(pts, target, lod_arg, dp, dl, counts=counts, order="cell")
            lc, dpc = c.train_points_grad(pts, target, lod=lod_arg, counts=counts, order="cell")
            assert out_p is dp and out_l is dl and torch.equal(la, lc) and a.steps == c.steps == 1 and a._pass_samples == c._pass_samples == n
            for b, n_b in enumerate(counts):
                assert torch.equal(dp[b, :n_b], dpc[b, :n_b]) and bool((dp[b, n_b:] == 9.0).all()) and bool((dl[b, n_b:] == 9.0).all())
            # tables, optimiser moments and step counts: train_points_grad(lod=)'s on a copy of the batch
            for k, (ta, tc) in enumerate(zip([a.tables] + a.params, [c.tables] + c.params)):
                sa, sc = a._adam_state(ta), c._adam_state(tc)
                assert torch.equal(sa["step"], sc["step"])
                if k > 0 or n <= 64:
                    assert torch.equal(ta.detach(), tc.detach()), (n, k)
                    assert torch.equal(sa["exp_avg"], sc["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sc["exp_avg_sq"]), (n, k)
                else:
                    upd = float((tc.detach() - before).abs().max())
                    differ = int((ta.detach() != tc.detach()).sum())
                    e_t = float((ta.detach() - tc.detach()).abs().max()) / upd
                    print(f"train_points_grad_lod num_bits={num_bits}, {n} points a field: {differ} of {ta.numel()} table values differ from the sibling's, "
                          f"by at most {e_t:.3e} of the largest update")
                    assert upd > 0 and e_t <= TOL_ORDER, (n, e_t)
            for b, n_b in enumerate(counts):                                  # field b's own step
                l1, dp1, dl1 = singles[b].train_points_grad_lod(pts[b, :n_b].contiguous(), target[b, :n_b].contiguous(),
                                                                lod_arg[..., :n_b].contiguous() if isinstance(lod_arg, torch.Tensor) and lod_arg.dim() == 1 else
                                                                lod_arg[b, :n_b].contiguous() if isinstance(lod_arg, torch.Tensor) else lod_arg,
                                                                fused=True, order="cell")
                assert torch.equal(dl[b, :n_b], dl1) and torch.equal(dp[b, :n_b], dp1), (b, n_b)
                assert abs(float(la[b]) - float(l1)) <= TOL_Y * abs(float(l1))
    # fresh tensors: zero at the rows a field does not own
    f = _batch(dev, num_bits)
    _, dp, dl = f.train_points_grad_lod(pts, target, lod, counts=counts)
    assert dl.shape == (B, n) and all(bool((dl[b, n_b:].view(torch.int32) == 0).all()) for b, n_b in enumerate(counts))
    assert bool((dl[0] != 0).any()) and bool((dl[1, :65] != 0).any())     # field 2's one row has lambda = 0: every level at full weight, no slope
    # a pass in two chunks: the sibling's noise bookkeeping - each call fills ITS dlod with the keys of its place in the pass
    f, twin = _batch(dev, num_bits), _batch(dev, num_bits)
    chunks = [(200, 65, 1), (64, 0, 63)]
    outs = [(torch.full((B, n, 2), 9.0, device=dev), torch.full((B, n), 9.0, device=dev)) for _ in chunks]
    for k, cnt in enumerate(chunks):
        f.train_points_grad_lod(pts, target, lod, outs[k][0], outs[k][1], counts=cnt, accumulate=k > 0, scale=0.5, step=k == 1, order="cell")
        twin.train_points_grad(pts, target, lod=lod, counts=cnt, accumulate=k > 0, scale=0.5, step=k == 1, order="cell")
        assert f._pass_samples == twin._pass_samples == (k + 1) * n
    assert f.steps == twin.steps == 1
    for ta, tc in zip(f.params, twin.params):
        assert torch.equal(ta.detach(), tc.detach())
    for k, cnt in enumerate(chunks):                                      # chunk k alone, from the starting state, at its place in the pass
        t = _batch(dev, num_bits)
        t._pass_samples = k * n
        _, dp1, dl1 = t.train_points_grad_lod(pts, target, lod, counts=cnt, accumulate=True, scale=0.5, step=False, order="cell")
        for b, n_b in enumerate(cnt):
            assert torch.equal(outs[k][1][b, :n_b], dl1[b, :n_b]) and torch.equal(outs[k][0][b, :n_b], dp1[b, :n_b]), (k, b)
            assert bool((outs[k][1][b, n_b:] == 9.0).all())
    if num_bits is not None:                                              # the key of the place in the pass matters
        t = _batch(dev, num_bits)
        _, _, dl0 = t.train_points_grad_lod(pts, target, lod, counts=chunks[1], accumulate=True, scale=0.5, step=False, order="cell")
        assert not torch.equal(dl0[0, :64], outs[1][1][0, :64])


def test_train_points_differentiable_lod(dev):
    pts, lod, target, _ = _class_inputs(dev)
    counts = (200, 65, 1)
    up = torch.tensor([0.5, -2.0, 3.0], device=dev)
    kw = dict(counts=counts, order="cell")
    for lod_arg in (lod, lod[0].contiguous(), torch.tensor(1.25, device=dev)):
        want = _batch(dev)
        lw, dp, dl = want.train_points_grad_lod(pts, target, lod_arg, **kw)
        g = up.reshape(B, 1) * dl
        glod = g if lod_arg.dim() == 2 else g.sum(0) if lod_arg.dim() == 1 else g.sum()
        a = _batch(dev)
        p_leaf, l_leaf = pts.clone().requires_grad_(True), lod_arg.clone().requires_grad_(True)
        loss = a.train_points_differentiable_lod(p_leaf, l_leaf, target, **kw)
        assert loss.requires_grad and loss.shape == (B,) and a.steps == 1
        (loss * up).sum().backward()
        assert torch.equal(loss.detach(), lw) and torch.equal(p_leaf.grad, up.reshape(B, 1, 1) * dp)
        assert l_leaf.grad.shape == lod_arg.shape and torch.equal(l_leaf.grad, glod) and bool((l_leaf.grad != 0).any())
        assert all(torch.equal(x.detach(), w.detach()) for x, w in zip(a.params, want.params))
        c = _batch(dev)                                                   # the level of detail alone
        l_leaf = lod_arg.clone().requires_grad_(True)
        (c.train_points_differentiable_lod(pts, l_leaf, target, **kw) * up).sum().backward()
        assert torch.equal(l_leaf.grad, glod)
        e, twin = _batch(dev), _batch(dev)                                # nothing asks for a gradient: the plain call
        plain = e.train_points_differentiable_lod(pts, lod_arg, target, **kw)
        assert not plain.requires_grad and torch.equal(plain, twin.train_points_lod(pts, target, lod_arg, **kw))
    shared = pts[0].clone().requires_grad_(True)                          # shared points: summed over the fields
    a, want = _batch(dev), _batch(dev)
    (a.train_points_differentiable_lod(shared, lod, target) * up).sum().backward()
    _, dp, _ = want.train_points_grad_lod(pts[0].contiguous(), target, lod)
    assert torch.equal(shared.grad, (up.reshape(B, 1, 1) * dp).sum(0))
    with pytest.raises(TypeError):
        a.train_points_differentiable_lod(pts.clone().requires_grad_(True), lod, target, dlod=torch.zeros(B, pts.shape[1], device=dev))


# ---- 6. what it is for ----------------------------------------------------------------------------------------------------------------------
LAM_TRUE = (1.25, 1.75, 2.5)                 # each field its own; the default fades are 4, 3, 2, 1
SHIFT_TRUE = ((0.75, -0.5), (-0.6, 0.9), (0.4, 0.7))


def _descent_batch(dev):
    """three 64 x 64 fields of table 2^12 (tests/test_hashgrid_lodgrad_cpu.py's DESCENT geometry): field 0 is its table and decoder, fields 1
    and 2 draw theirs from other seeds; 256 points inside the field per field"""
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    d = L.DESCENT
    geo, _, table, params, points = L.descent_inputs()
    f = HashGridFieldBatch(B, d["size"], levels=4, features=d["features"], log2_table=d["log2_table"], base_resolution=4, finest_resolution=32, device=dev,
                           seed=d["seed"])
    assert f.resolutions == d["resolutions"] and f.lod_fade == (4.0, 3.0, 2.0, 1.0)
    tables, decoders, pts = [table], [params], [points]
    for b in (1, 2):
        g = torch.Generator().manual_seed(d["seed"] + 100 * b)
        tables.append((torch.rand(*geo.table_shape(), generator=g) - 0.5).contiguous())
        pts.append((torch.rand(d["n"], 2, generator=g) * 62.0 + 0.5).contiguous())
        decoders.append(L.decoder_params(geo.width, d["seed"] + b))
    with torch.no_grad():
        f.tables.copy_(torch.stack(tables).to(dev))
        for k, p in enumerate(f.params):
            p.copy_(torch.stack([dec[k] for dec in decoders]).to(dev))
    return f, torch.stack(pts).to(dev)


def test_a_level_of_detail_per_field_is_recovered_with_the_fields_held(dev):
    """4.7.22's descent for three fields at once through the training entry with step=False: colours from query_lod at each field's own
    lambda_b, ONE torch Adam (lr 0.02, 200 steps) on a [B] parameter broadcast to [B, N] from 2.0; ``run_descent``'s tolerance, |lambda_hat_b -
    lambda_b| <= 0.075, per field.  The fields' parameters never move"""
    d = L.DESCENT
    f, pts = _descent_batch(dev)
    n = pts.shape[1]
    true = torch.tensor(LAM_TRUE, device=dev)
    tables0 = f.tables.detach().clone()
    colours = f.query_lod(pts, true.reshape(B, 1).expand(B, n).contiguous())
    lam = torch.full((B,), d["start"], dtype=torch.float32, device=dev, requires_grad=True)
    opt = torch.optim.Adam([lam], lr=d["lr"])
    first = last = None
    for _ in range(d["steps"]):
        opt.zero_grad()
        loss = f.train_points_differentiable_lod(pts, lam.reshape(B, 1).expand(B, n), colours, step=False)
        first = loss.detach().clone() if first is None else first
        last = loss.detach()
        loss.sum().backward()
        opt.step()
    err = (lam.detach() - true).abs()
    print(f"descent on a lambda per field: loss {first.tolist()} -> {last.tolist()}, lambda_hat {lam.tolist()}, errors {err.tolist()}")
    assert bool((err <= 0.075).all()) and f.steps == 0 and torch.equal(f.tables.detach(), tables0)


def test_twenty_joint_steps_follow_the_extracted_fields(dev):
    """20 joint steps through ``train_points_differentiable_lod``, the fields stepping inside the call, with a lambda_b and a 2-vector shift per
    field stepped by one torch Adam - against the same loop over the three extracted fields, each with its own Adam.  The largest deviation
    per quantity over the 20 steps is printed; the bound is 10 x the value recorded in DESIGN 4.7.25 and at most 1e-3.  (Whether lambda is
    recovered while the fields are fitted is not claimed: DESIGN 4.7.23.)"""
    from tests.test_hashgrid_lodtrain_cpu import JOINT
    f, pts = _descent_batch(dev)
    n = pts.shape[1]
    singles = [f.extract(b) for b in range(B)]
    shift_true = torch.tensor(SHIFT_TRUE, device=dev)
    colours = f.query_lod((pts + shift_true.reshape(B, 1, 2)).contiguous(), torch.tensor(LAM_TRUE, device=dev).reshape(B, 1).expand(B, n).contiguous())

    def run(step, shape):
        lam = torch.full(shape, JOINT["lam_start"], dtype=torch.float32, device=dev, requires_grad=True)
        shift = torch.zeros(*shape, 2, dtype=torch.float32, device=dev, requires_grad=True)
        opt = torch.optim.Adam([lam, shift], lr=JOINT["lr"])
        lams, shifts, losses = [], [], []
        for _ in range(JOINT["steps"]):
            opt.zero_grad()
            loss = step(lam, shift)
            loss.sum().backward()
            opt.step()
            lams.append(lam.detach().double().cpu().clone())
            shifts.append(shift.detach().double().cpu().clone())
            losses.append(loss.detach().double().cpu().clone())
        return torch.stack(lams), torch.stack(shifts), torch.stack(losses)

    got = run(lambda lam, shift: f.train_points_differentiable_lod(pts + shift.reshape(B, 1, 2), lam.reshape(B, 1).expand(B, n), colours, order="cell"), (B,))
    assert f.steps == JOINT["steps"]
    dev_lam = dev_shift = dev_loss = 0.0
    for b in range(B):
        want = run(lambda lam, shift: singles[b].train_points_differentiable_lod(pts[b] + shift, lam, colours[b], fused=True, order="cell"), ())
        dev_lam = max(dev_lam, float((got[0][:, b] - want[0]).abs().max()))
        dev_shift = max(dev_shift, float((got[1][:, b] - want[1]).abs().max()))
        dev_loss = max(dev_loss, float(((got[2][:, b] - want[2].reshape(-1)).abs() / want[2].reshape(-1).abs()).max()))
    print(f"20 joint steps, three fields: lambda {got[0][0].tolist()} -> {got[0][-1].tolist()}, loss {got[2][0].tolist()} -> {got[2][-1].tolist()}; largest "
          f"deviation from the extracted fields: lambda {dev_lam:.3e}, shift {dev_shift:.3e} samples, loss {dev_loss:.3e} (relative)")
    assert max(JOINT_BOUND.values()) <= JOINT_CEILING
    assert dev_lam <= JOINT_BOUND["lambda"] and dev_shift <= JOINT_BOUND["shift"] and dev_loss <= JOINT_BOUND["loss"]
