"""GPU tests that hold every optimiser step of the hash-grid FIT loops to the float64 reference (oracle/hashgrid_fit_ref.py):
``HashGridField.fit`` / ``fit_points`` / ``fit_mips`` and ``HashGridFieldBatch.fit`` / ``fit_points``.

A fit is recorded, not compared as a whole.  ``Recorder`` shadows ``train_step``, ``train_points`` and ``freeze`` on the instance (the fit
methods call them through ``self``) and keeps, per pass, clones of the state the pass started from (tables, the six decoder tensors, every
``exp_avg`` / ``exp_avg_sq`` / ``step`` of the optimiser), every call's arguments as the method received them and the loss it returned,
the public table-gradient buffer after a call with ``step=False``, the same state clones after the step, and the table right before and right after ``freeze()``.
``verify`` then judges every pass alone from the device's own fp32 pre-state, within the per-step bounds of DESIGN 4.7.17 - errors do not
compound - and compares the written-back moments and step counts too, since they are the next pass's given.

The cases, their inputs, the installed Adam state and the model that shows on the CPU that the judgement has teeth live in
tests/test_hashgrid_fit_ref_cpu.py."""
import numpy as np
import pytest
import torch

from oracle import hashgrid_fit_ref as V
from oracle import hashgrid_ref as R
from tests import test_hashgrid_fit_ref_cpu as M
from tests.test_hashgrid_train_ref_cpu import NOISE_SEED

pytestmark = pytest.mark.gpu

FLOOR = 0.08                     # sqrt(min v) >= 0.08 gmax per pass and tensor: without it the step bound goes slack silently


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Recorder:
    """shadows ``train_step`` / ``train_points`` / ``freeze`` of one field or batch and builds the ``Recording`` (module docstring)"""

    def __init__(self, f, batch):
        self.f, self.batch = f, batch
        self.rec = V.Recording()
        self.cur, self.frozen_table, self.unfrozen_table = None, None, None
        self._step, self._points, self._freeze = f.train_step, f.train_points, f.freeze
        f.train_step, f.train_points, f.freeze = self.train_step, self.train_points, self.freeze

    def lift(self, t):
        """a CPU clone with the field axis in front"""
        t = t.detach().cpu().clone()
        return t if self.batch else t.unsqueeze(0)

    def table(self):
        return self.f.tables if self.batch else self.f.table

    def state(self):
        opt = self.f.optimizer
        dec = self.f.params if self.batch else self.f.decoder.linear_params()

        def moments(p):
            st = opt.state.get(p, {})
            if len(st) == 0:                                     # the optimiser's own fresh state: zeros it has not made yet
                z = self.lift(torch.zeros_like(p))
                return z, z.clone(), 0
            return self.lift(st["exp_avg"]), self.lift(st["exp_avg_sq"]), int(st["step"].item())

        return V.State(self.lift(self.table()), [self.lift(p) for p in dec], moments(self.table()), [moments(p) for p in dec])

    def before(self, accumulate):
        if not accumulate:
            self.cur = V.Pass(pre=self.state(), steps=int(self.f.steps), frozen_table=self.frozen_table, unfrozen_table=self.unfrozen_table)
            self.frozen_table = self.unfrozen_table = None

    def after(self, call):
        if not call.step:
            g = self.table().grad
            call.grad = None if g is None else self.lift(g)
        self.cur.calls.append(call)
        if call.step:
            self.cur.post = self.state()
            self.rec.passes.append(self.cur)
            self.cur = None

    def train_step(self, coord, extent, target, accumulate=False, scale=1.0, step=True, noise=None):
        self.before(accumulate)
        loss = self._step(coord, extent, target, accumulate=accumulate, scale=scale, step=step, noise=noise)
        org = np.asarray(coord.cpu() if isinstance(coord, torch.Tensor) else coord, dtype=np.int64)
        if org.ndim < 3:                                         # [num_crops, dim]: the crops of every field
            org = np.broadcast_to(org.reshape(1, -1, len(extent)), (self.f.n_fields if self.batch else 1, org.size // len(extent), len(extent)))
        self.after(V.Call(target=self.lift(target), accumulate=bool(accumulate), scale=float(scale), step=bool(step),
                          loss=loss.detach().cpu().reshape(-1).double(), origins=np.ascontiguousarray(org), extent=tuple(int(v) for v in extent)))
        return loss

    def train_points(self, points, target, *args, **kw):
        names = ("counts", "accumulate", "scale", "step", "noise", "order") if self.batch else ("accumulate", "scale", "step", "noise", "order", "fused", "lod", "dpoints")
        kw.update(zip(names, args))
        accumulate, scale, step = kw.get("accumulate", False), kw.get("scale", 1.0), kw.get("step", True)
        self.before(accumulate)
        loss = self._points(points, target, **kw)
        pts = points.detach().cpu().numpy()
        if pts.ndim == 2:
            pts = np.broadcast_to(pts[None], (self.f.n_fields if self.batch else 1, *pts.shape))
        lod, counts = kw.get("lod"), kw.get("counts")
        if isinstance(lod, torch.Tensor):
            lod = lod.detach().cpu().numpy().copy() if lod.dim() > 0 else float(lod)
        if counts is not None:
            counts = [int(v) for v in (counts.cpu().tolist() if isinstance(counts, torch.Tensor) else counts)]
        self.after(V.Call(target=self.lift(target), accumulate=bool(accumulate), scale=float(scale), step=bool(step),
                          loss=loss.detach().cpu().reshape(-1).double(), points=np.ascontiguousarray(pts), lod=lod, counts=counts))
        return loss

    def freeze(self):
        self.unfrozen_table = self.lift(self.table())             # the quantiser is judged from this, not from the pass's pre-state
        self._freeze()
        self.frozen_table = self.lift(self.table())


def build(dev, p, fused):
    """the field or batch of plan ``p`` with the plan's parameters, the installed Adam state (read back), ``steps`` and the schedule"""
    from neural_image_compression_v2_amd import hashgrid
    _, F, L = p.shape
    args = dict(levels=L, features=F, log2_table=p.geo.log2_table, base_resolution=p.base, device=dev, seed=1, num_bits=p.bits, noise_seed=NOISE_SEED)
    batch = p.B > 1
    if batch:
        f = hashgrid.HashGridFieldBatch(p.B, p.field_size, **args)
        tab_p, dec_p = f.tables, f.params
    else:
        f = hashgrid.HashGridField(p.field_size, fused=fused, **args)
        assert f.route == ("fused" if fused else "layerwise")
        tab_p, dec_p = f.table, f.decoder.linear_params()
    assert tuple(f.geo.resolutions) == tuple(p.geo.resolutions)

    def stacked(per_field):
        return torch.stack(per_field) if batch else per_field[0]

    with torch.no_grad():
        tab_p.copy_(stacked(p.tables).to(dev))
        for k, q in enumerate(dec_p):
            q.copy_(stacked([p.params[b][k] for b in range(p.B)]).to(dev))
    st = M.installed_state(p)
    if st is not None:
        opt = f.optimizer
        sd = opt.state_dict()
        index = {id(q): idx for grp, ids in zip(opt.param_groups, sd["param_groups"]) for q, idx in zip(grp["params"], ids["params"])}

        def entry(m, v):
            return {"step": torch.tensor(float(p.k0)), "exp_avg": (m if batch else m[0]).clone(), "exp_avg_sq": (v if batch else v[0]).clone()}

        state = {index[id(tab_p)]: entry(*st["table"])}
        for k, q in enumerate(dec_p):
            state[index[id(q)]] = entry(*st["decoder"][k])
        opt.load_state_dict({"state": state, "param_groups": sd["param_groups"]})
        f.steps = p.k0
        for q, (m, v) in [(tab_p, st["table"])] + list(zip(dec_p, st["decoder"])):                # read back: fp32 in, the same fp32 out
            s = opt.state[q]
            assert torch.equal(s["exp_avg"].cpu(), m if batch else m[0]) and torch.equal(s["exp_avg_sq"].cpu(), v if batch else v[0])
            assert int(s["step"].item()) == p.k0
    if p.schedule:
        f.set_schedule(p.epochs)
    return f


def run_fit(dev, p, f, fused):
    t = p.target.to(dev)
    if p.entry == "fit":
        return [[h] for h in f.fit(t[0], p.epochs, chunk=p.chunk, freeze_at=p.freeze_at)]
    if p.entry == "batch_fit":
        return f.fit(t, p.epochs, chunk=p.chunk, freeze_at=p.freeze_at)
    if p.entry == "fit_mips":
        return [[h] for h in f.fit_mips(t[0], p.epochs, mips=p.mips, batch=p.batch, order=p.order, fused=fused, freeze_at=p.freeze_at)]
    pts = torch.from_numpy(p.points).to(dev)
    if p.entry == "fit_points":
        lod = None if p.lod is None else torch.from_numpy(p.lod).to(dev)
        return [[h] for h in f.fit_points(pts[0], t[0], p.epochs, batch=p.batch, order=p.order, fused=fused, freeze_at=p.freeze_at, lod=lod)]
    return f.fit_points(pts, t, p.epochs, counts=p.counts, order=p.order, freeze_at=p.freeze_at)


def record_and_verify(dev, name, fused=True):
    p = M.plan(name)
    f = build(dev, p, fused)
    r = Recorder(f, p.B > 1)
    r.rec.returned = run_fit(dev, p, f, fused)
    what = f"{name} {'batch' if p.B > 1 else 'fused' if fused else 'layer-wise'}"
    assert len(r.rec.passes) == p.epochs and r.cur is None
    rep = V.verify(r.rec, M.case_of(p), what=what)
    assert not rep.failures(), f"{what}: " + "; ".join(rep.failures()[:8])
    if p.fresh:
        print(f"MEASURED {what} | shares | " + ", ".join(f"{k} {v:.2f}" for k, v in rep.share.items()))
    else:
        low = min((v, q, e) for e, m in enumerate(rep.floor) for q, v in m.items())
        assert low[0] >= FLOOR, f"{what}: sqrt(min v) = {low[0]:.4f} gmax at pass {low[2]} {low[1]}: the step bound would go slack"
    return p, f, r.rec


ROUTES = pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])


@ROUTES
@pytest.mark.parametrize("name", ["A-2D", "A-3D"])
def test_fit(dev, name, fused, tmp_path):
    """case A; then the stored files of the fitted field, read from their BYTES by oracle/hashgrid_ref.py, hold the frozen table"""
    p, f, rec = record_and_verify(dev, name, fused)
    frozen = rec.passes[-1].post.tables[0]
    for packed in (False, True):
        path = tmp_path / f"{name}-{packed}.pt"
        f.save_compressed(path, packed=packed)
        stored = R.read_file(path)
        for l, vals in enumerate(R.table_values(stored)):
            got = torch.from_numpy(vals.astype(np.float32))
            assert torch.equal(got.view(torch.int32), frozen[l][:got.shape[0]].contiguous().view(torch.int32)), f"{name} packed={packed}: level {l}"


@ROUTES
def test_fit_with_a_depth_per_level(dev, fused):
    """case B: clamp, noise scale and freeze per level"""
    record_and_verify(dev, "B-2D", fused)


@ROUTES
@pytest.mark.parametrize("name", ["C-2D", "C-3D"])
def test_fit_points(dev, name, fused):
    """case C: cell order, a level of detail per point (NaN, negative and 40 among them), chunks of 500, 500, 209"""
    record_and_verify(dev, name, fused)


def test_fit_points_plain(dev):
    """case C once more: order=None, lod=None, batch=None"""
    record_and_verify(dev, "C-2D-plain", True)


@pytest.mark.parametrize("name,fused", [("D-2D", True), ("D-2D", False), ("D-3D", True)], ids=["2D-fused", "2D-layerwise", "3D-fused"])
def test_fit_mips(dev, name, fused):
    record_and_verify(dev, name, fused)


@pytest.mark.parametrize("name", ["E-fit-2D", "E-fit-3D"])
def test_batch_fit(dev, name):
    record_and_verify(dev, name)


@pytest.mark.parametrize("name", ["E-points-2D-cell", "E-points-2D-none", "E-points-3D-cell", "E-points-3D-none"])
def test_batch_fit_points(dev, name):
    record_and_verify(dev, name)


def test_fit_from_the_optimisers_own_fresh_state(dev):
    """case F: m = v = 0, no schedule, three passes"""
    record_and_verify(dev, "F-2D", True)
