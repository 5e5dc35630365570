"""CPU-only tests of the step-by-step judgement of a recorded hash-grid fit (run with -m "not gpu"; oracle/hashgrid_fit_ref.py; DESIGN
4.7.19), and the cases, inputs and constants tests/test_gpu_hashgrid_fit_ref.py records the GPU's fits with.

- a MODEL fit in float64 (``model_fit``) walks the loops as the docstrings of ``fit`` / ``fit_points`` / ``fit_mips`` and of the batch methods
  state them and emits a ``Recording``; clean, it passes ``verify`` with every error at most 1e-3 of its bound on every case;
- teeth: each of eleven deliberate mistakes in the model (a switch each) moves some compared quantity by more than 20 bounds, on every case
  it applies to; three more (a quantiser that truncates, one with a depth off by one, a freeze of an older table) trip the exact check
  that is theirs, and the allowance for entries on a rounding boundary excuses those and nothing else;
- the floor: the free-running float64 model keeps sqrt(min v) >= 0.09 gmax on every pass and tensor (the GPU asserts 0.08);
- ``step_bound`` equals the function it replaces; the reference's learning rates equal ``CosineAnnealing``'s; the quantiser is idempotent,
  puts every x of ``q_range`` on a code of 0 .. 2^b - 1 and equals the dequantised ``save4fp`` code of ``oracle/hashgrid_ref.py``.

The inputs are those of tests/test_hashgrid_train_ref_cpu.py (``C.inputs``: ``table_c`` clamped into the range, decoder, ``points``, ``lod``)
plus seeded uniform targets and points.  Everything a plan holds is shared and READ-ONLY."""
import functools
import hashlib
import math
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_fit_ref as V
from oracle import hashgrid_ref as R
from oracle import hashgrid_train_ref as T
from tests import test_hashgrid_train_ref_cpu as C

TEETH = C.TEETH
NUM_BITS, EPOCHS, FREEZE_AT, K0 = 6, 6, 0.5, 3
FIT_CHUNK = {2: 16, 3: 5}                               # slabs of 16, 16, 12 rows of 44; of 5, 5, 2 of 12
SHAPE = {2: (2, 2, 16), 3: (3, 4, 8)}
POINTS_EXTRA, POINTS_BATCH = 1000, 500                  # 209 + 1000 points in chunks of 500, 500, 209
MIP_FIELDS = {2: dict(field_size=(48, 40), mips=2, batch=1000), 3: dict(field_size=(12, 8, 8), mips=1, batch=None)}
N_FIELDS = C.N_FIELDS
F64 = torch.float64

PLANS = ["A-2D", "A-3D", "B-2D", "C-2D", "C-3D", "C-2D-plain", "D-2D", "D-3D", "E-fit-2D", "E-fit-3D", "E-points-2D-cell", "E-points-2D-none",
         "E-points-3D-cell", "E-points-3D-none", "F-2D"]
# the factor of the installed exp_avg_sq = (factor gmax)^2 (1.001 + U(0, 1)): 0.1 unless the free-running model cannot hold the floor of
# 0.09 with it (test_floor_of_the_free_running_model)
FACTOR = {"B-2D": 0.2}             # B with 0.1: 0.0887 at pass 1 on level 11 (3 bits: the noise moves that level's gradient most)


def plan(name):
    """one case: constructor arguments, parameters, the arguments of the fit call (CPU tensors), what ``verify`` is told"""
    return _plan(str(name))


@functools.lru_cache(maxsize=None)
def _plan(name):
    kind, rest = name.split("-", 1)
    dim = 3 if "3D" in rest else 2
    shape = SHAPE[dim]
    _, F, L = shape
    spec = C.SPECS[dim]
    entry = {"A": "fit", "B": "fit", "C": "fit_points", "D": "fit_mips", "F": "fit"}.get(kind) or ("batch_fit" if "fit" in rest else "batch_fit_points")
    B = N_FIELDS if kind == "E" else 1
    size = MIP_FIELDS[dim]["field_size"] if kind == "D" else spec["field_size"]
    geo = T.geometry(size, L, F, 10, spec["base"])
    bits = C.level_bits(dim, L) if kind == "B" else NUM_BITS
    lb = bits if kind == "B" else (NUM_BITS,) * L
    inps = [C.inputs(*shape, b) for b in range(B)]
    tables = [torch.stack([i.table_c[l].clamp(*T.q_range(lb[l])) for l in range(L)]) for i in inps]
    g = torch.Generator().manual_seed(4719 + 10 * dim + sum(map(ord, name)))
    p = types.SimpleNamespace(name=name, kind=kind, dim=dim, shape=shape, entry=entry, B=B, geo=geo, field_size=tuple(size), base=spec["base"],
                              bits=bits, epochs=3 if kind == "F" else EPOCHS, freeze_at=FREEZE_AT, schedule=kind != "F", fresh=kind == "F",
                              k0=0 if kind == "F" else K0, tables=tables, params=[i.params for i in inps], fade=None, factor=FACTOR.get(name, 0.1))
    S = p.field_size
    if entry in ("fit", "batch_fit"):
        p.target = torch.rand(B, *S, 3, generator=g)
        p.chunk = FIT_CHUNK[dim]
        p.chunks = [min(p.chunk, S[0] - x0) * int(np.prod(S[1:])) for x0 in range(0, S[0], p.chunk)]
    elif entry == "fit_mips":
        p.target = torch.rand(1, *S, 3, generator=g)
        p.mips, p.batch, p.order = MIP_FIELDS[dim]["mips"], MIP_FIELDS[dim]["batch"], "cell"
        p.fade = T.default_fade(geo)
        n = sum(int(np.prod([s >> m for s in S])) for m in range(p.mips + 1))
        p.chunks = _cuts(n, p.batch)
    else:
        pts = []
        for b in range(B):
            extra = (torch.rand(POINTS_EXTRA, dim, generator=g) * torch.tensor(S, dtype=torch.float32) - 0.5).numpy().astype(np.float32)
            pts.append(np.concatenate([inps[b].points, extra]))
        p.points = np.stack(pts)                                                      # [B, N, dim]
        n = p.points.shape[1]
        p.target = torch.rand(B, n, 3, generator=g)
        p.lod, p.counts = None, None
        if entry == "fit_points":
            plain = rest.endswith("plain")
            p.order, p.batch = (None, None) if plain else ("cell", POINTS_BATCH)
            if not plain:
                p.fade = T.default_fade(geo)
                more = (torch.rand(POINTS_EXTRA, generator=g) * (max(p.fade) + 1.5)).numpy().astype(np.float32)
                p.lod = np.concatenate([inps[0].lod, more])
            p.chunks = _cuts(n, p.batch)
        else:
            p.order = "cell" if rest.endswith("cell") else None
            p.counts = (n, n - 37, 70)
            p.chunks = [n]
    return p


def _cuts(n, batch):
    batch = n if batch is None else batch
    return [min(batch, n - c0) for c0 in range(0, n, batch)]


def case_of(p):
    """what ``verify`` is told about plan ``p``"""
    c = V.Case(geo=p.geo, bits=p.bits, seed=C.NOISE_SEED, k0=p.k0, epochs=p.epochs, freeze_at=p.freeze_at, schedule=p.epochs if p.schedule else None,
               fade=p.fade, fresh=p.fresh, chunks=p.chunks)
    if p.entry == "fit_mips":
        c.mips = (p.target[0], p.mips)
    elif p.entry in ("fit_points", "batch_fit_points"):
        c.rows = []
        for b in range(p.B):
            n = p.points.shape[1] if p.counts is None else p.counts[b]
            c.rows.append((p.points[b, :n], p.target[b, :n], None if p.lod is None else p.lod[:n]))
    return c


# ------------------------------------------------------------------------------------------------------------------ a memoised T.step

_MEMO = {}


def cached_step(geo, table, params, target, **kw):
    """``T.step``, remembered by the bytes of everything it reads: the model and the verifier evaluate the same call at the same state"""
    h = hashlib.sha1()
    for x in [table, target, *params]:
        h.update(np.ascontiguousarray(T.as_f64(x).numpy()).tobytes())
    for k in sorted(kw):
        v = kw[k]
        if k == "lod" and v is not None:
            v = (tuple(v[0]), None if v[1] is None else np.asarray(v[1]).tobytes(), v[2])
        elif isinstance(v, np.ndarray):
            v = (v.shape, v.tobytes())
        h.update(repr((k, v)).encode())
    key = (geo, h.digest())
    if key not in _MEMO:
        if len(_MEMO) > 200:                         # a result holds the table gradient: about 0.7 MB
            _MEMO.clear()
        _MEMO[key] = T.step(geo, table, params, target, **kw)
    return _MEMO[key]


# ------------------------------------------------------------------------------------------------------------------ the model fit

MISTAKES = ["stale_gradient", "lr_of_the_epoch_before", "bias_correction_stuck", "noise_offset_stuck", "sample_base_restarts", "ragged_chunk_full_weight",
            "exp_avg_sq_not_written_back", "freeze_one_epoch_late", "noise_after_the_freeze", "decoder_lr_on_the_table", "moments_of_the_field_before",
            "quantiser_truncates", "quantiser_depth_off_by_one", "freeze_of_an_older_table"]
# mistakes whose whole effect is on a check that is exact (bits against bits): the line they must trip, instead of 20 bounds of a tolerance
EXACT = {"quantiser_truncates": "freeze | table bits", "quantiser_depth_off_by_one": "freeze | table bits",
         "freeze_of_an_older_table": "freeze | quantises the table the last step left"}


def first_pass_to_show(p, mistake):
    """the 0-based pass at which ``mistake`` first moves a compared quantity of plan ``p``, or None where it cannot show"""
    fe = math.ceil(p.freeze_at * p.epochs)
    chunked, ragged = len(p.chunks) > 1, len(set(p.chunks)) > 1
    return {"stale_gradient": 1,                                           # the buffer of pass 0 is still there in pass 1
            "lr_of_the_epoch_before": 1 if p.schedule else None,
            "bias_correction_stuck": None if p.fresh else 1,              # a fresh state's later parameters are not compared (case F)
            "noise_offset_stuck": 1,
            "sample_base_restarts": 0 if chunked else None,
            "ragged_chunk_full_weight": 0 if ragged else None,
            "exp_avg_sq_not_written_back": 0,
            "freeze_one_epoch_late": fe,
            "noise_after_the_freeze": fe,
            "decoder_lr_on_the_table": 0,
            "quantiser_truncates": fe, "quantiser_depth_off_by_one": fe, "freeze_of_an_older_table": fe,
            "moments_of_the_field_before": 0 if p.B > 1 and not p.fresh else None}[mistake]


def model_calls(p):
    """the calls of one pass as the docstrings state them (without losses): ``fit`` walks slabs of ``chunk`` x-rows, each weighted by its
    share; ``fit_points`` lays the set out in the order once and walks ``batch``-sized ranges of it; ``fit_mips`` hands the (point, lod,
    colour) sets of all mips to ``fit_points``; the batch's ``fit_points`` makes one call per pass, every field's real rows first.  The cell
    order is the device's business: the model uses a seeded permutation (``verify`` holds the rows as a multiset)."""
    S, dim, B = p.field_size, p.dim, p.B
    calls = []
    if p.entry in ("fit", "batch_fit"):
        total = int(np.prod(S))
        for x0 in range(0, S[0], p.chunk):
            ext = (min(p.chunk, S[0] - x0), *S[1:])
            slab = p.target[:, x0:x0 + p.chunk].reshape(B, -1, 3)
            org = np.array([[[x0] + [0] * (dim - 1)]] * B, dtype=np.int64)
            calls.append(dict(origins=org, extent=ext, target=slab, scale=slab.shape[1] / total))
        return _flag(calls)
    if p.entry == "fit_mips":
        pts, lods, cols = [], [], []
        tgt = p.target[0].double()
        for m in range(p.mips + 1):
            sz = tuple(s >> m for s in S)
            blocks = tgt.reshape(*[v for s in sz for v in (s, 1 << m)], 3)
            cols.append(blocks.mean(dim=tuple(range(1, 2 * dim, 2))).reshape(-1, 3).float())
            j = np.stack([g.reshape(-1) for g in np.meshgrid(*[np.arange(s) for s in sz], indexing="ij")], axis=1)
            pts.append(((j + 0.5) * float(1 << m) - 0.5).astype(np.float32))
            lods.append(np.full(j.shape[0], float(m), dtype=np.float32))
        points, target, lod, counts = np.concatenate(pts)[None], torch.cat(cols)[None], np.concatenate(lods), None
    else:
        points, target, lod, counts = p.points, p.target, p.lod, p.counts
    n = points.shape[1]
    if p.order is not None:
        gen = torch.Generator().manual_seed(23)
        pp, tt = [], []
        for b in range(B):
            nb = n if counts is None else counts[b]
            idx = torch.cat([torch.randperm(nb, generator=gen), torch.arange(nb, n)]).numpy()
            pp.append(points[b][idx])
            tt.append(target[b][idx])
            if lod is not None:
                lod = lod[idx]                                                  # B = 1 wherever there is a level of detail
        points, target = np.stack(pp), torch.stack(tt)
    batch = n if getattr(p, "batch", None) is None else p.batch
    for c0 in range(0, n, batch):
        c1 = min(c0 + batch, n)
        calls.append(dict(points=points[:, c0:c1], target=target[:, c0:c1], lod=None if lod is None else lod[c0:c1], counts=counts, scale=(c1 - c0) / n))
    return _flag(calls)


def _flag(calls):
    for k, c in enumerate(calls):
        c.update(accumulate=k > 0, step=k == len(calls) - 1)
    return calls


def _evaluate(p, call, b, table, params, key, frozen, scale):
    n = call["target"].shape[1] if call.get("counts") is None else call["counts"][b]
    kw = dict(loss_scale=scale, noise_key=key, frozen=frozen)
    if "points" in call:
        kw["points"] = np.ascontiguousarray(call["points"][b, :n])
        if call["lod"] is not None:
            kw["lod"] = (p.fade, call["lod"][:n], 0.0)
    else:
        kw.update(origins=call["origins"][b], extent=call["extent"])
    return cached_step(p.geo, table, params, call["target"].double()[b, :n], **kw)


def _cosine(base, e, t_max):
    return base if t_max is None else base * (1 + math.cos(math.pi * e / t_max)) / 2


def model_fit(p, state=None, mistake=None, stop_after=None):
    """the fit of plan ``p`` in float64 from ``state`` (``installed_state``; None: the optimiser's own zeros) as a ``Recording``"""
    B, L, geo = p.B, p.geo.levels, p.geo
    lb = p.bits if isinstance(p.bits, tuple) else (p.bits,) * L
    tables = torch.stack([t.double() for t in p.tables])
    params = [torch.stack([p.params[b][i].double() for b in range(B)]) for i in range(6)]
    if state is None:
        mt, vt = torch.zeros_like(tables), torch.zeros_like(tables)
        md, vd = [torch.zeros_like(q) for q in params], [torch.zeros_like(q) for q in params]
    else:
        mt, vt = state["table"][0].double().clone(), state["table"][1].double().clone()
        md, vd = [m.double().clone() for m, _ in state["decoder"]], [v.double().clone() for _, v in state["decoder"]]
    steps, st_t, st_d = p.k0, p.k0, p.k0
    calls = model_calls(p)
    fe = math.ceil(p.freeze_at * p.epochs) + (1 if mistake == "freeze_one_epoch_late" else 0)
    t_max = p.epochs if p.schedule else None
    frozen, stale = False, None
    rec = V.Recording(returned=[])

    def snapshot():
        return V.State(tables.clone(), [q.clone() for q in params], (mt.clone(), vt.clone(), st_t), [(m.clone(), v.clone(), st_d) for m, v in zip(md, vd)])

    for e in range(p.epochs if stop_after is None else min(p.epochs, stop_after + 1)):
        frozen_table = unfrozen_table = None
        if e >= fe and not frozen:
            unfrozen_table = (older if mistake == "freeze_of_an_older_table" else tables).clone()
            if mistake == "quantiser_truncates":
                q = torch.stack([torch.floor(unfrozen_table[:, l] * ((1 << b) - 1)) / ((1 << b) - 1) for l, b in enumerate(lb)], dim=1)
            elif mistake == "quantiser_depth_off_by_one":
                q = V.quantise_levels(unfrozen_table, [b - 1 if b > 1 else b + 1 for b in lb])
            else:
                q = V.quantise_levels(unfrozen_table, lb)
            tables = q.float().double()                                              # the device stores fp32
            frozen, frozen_table = True, tables.clone()
        older = tables.clone()                                                       # the table one step back, for the mistake above
        ps = V.Pass(pre=snapshot(), steps=steps, frozen_table=frozen_table, unfrozen_table=unfrozen_table)
        g_t = torch.zeros_like(tables) if stale is None or mistake != "stale_gradient" or frozen else stale.clone()
        g_d = [torch.zeros_like(q) for q in params]
        before, tot = 0, torch.zeros(B, dtype=F64)
        for k, call in enumerate(calls):
            offset = p.k0 if mistake == "noise_offset_stuck" else steps
            base = 0 if mistake == "sample_base_restarts" else before
            key = (p.bits, C.NOISE_SEED, offset, base) if not frozen or mistake == "noise_after_the_freeze" else None
            scale = calls[0]["scale"] if mistake == "ragged_chunk_full_weight" else call["scale"]
            loss = torch.zeros(B, dtype=F64)
            for b in range(B):
                r = _evaluate(p, call, b, tables[b], [q[b] for q in params], key, frozen, scale)
                loss[b] = r.loss
                for i in range(6):
                    g_d[i][b] += r.decoder_grads[i]
                if not frozen:
                    g_t[b] += torch.stack(r.table_grad)
            before += call["target"].shape[1]
            tot += loss
            ps.calls.append(V.Call(target=call["target"], accumulate=call["accumulate"], scale=scale, step=call["step"], loss=loss, origins=call.get("origins"),
                                   extent=call.get("extent"), points=call.get("points"), lod=call.get("lod"), counts=call.get("counts"),
                                   grad=None if call["step"] or frozen else g_t.clone()))
        # the optimiser step
        le = max(e - 1, 0) if mistake == "lr_of_the_epoch_before" else e
        lr_t, lr_d = _cosine(0.01, le, t_max), _cosine(0.005, le, t_max)
        if mistake == "decoder_lr_on_the_table":
            lr_t = lr_d
        count = p.k0 + 1 if mistake == "bias_correction_stuck" else steps + 1
        shift = 1 if mistake == "moments_of_the_field_before" else 0
        if not frozen:
            stale = g_t.clone()                                                    # what a missing fill leaves behind: everything so far
            for b in range(B):
                for l in range(L):
                    s = (b - shift) % B
                    tables[b, l], m1, v1 = T.adam_step(tables[b, l], g_t[b, l], mt[s, l], vt[s, l], count, lr_t, clamp=T.q_range(lb[l]))
                    mt[b, l] = m1
                    if mistake != "exp_avg_sq_not_written_back":
                        vt[b, l] = v1
            st_t += 1
        new_m, new_v = [m.clone() for m in md], [v.clone() for v in vd]
        for i in range(6):
            for b in range(B):
                s = (b - shift) % B
                params[i][b], m1, v1 = T.adam_step(params[i][b], g_d[i][b], md[i][s], vd[i][s], count, lr_d)
                new_m[i][b] = m1
                if mistake != "exp_avg_sq_not_written_back":
                    new_v[i][b] = v1
        md, vd = new_m, new_v
        st_d += 1
        steps += 1
        ps.post = snapshot()
        rec.passes.append(ps)
        rec.returned.append([float(v) for v in tot])
    return rec


def installed_state(p):
    """Adam's state as ``StepCase`` installs it, fp32: exp_avg = 0.01 gmax U(-1, 1), exp_avg_sq = (factor gmax)^2 (1.001 + U(0, 1)), gmax per
    tensor / level / field the largest gradient of the reference's first pass.  None for a fresh case."""
    return None if p.fresh else _installed_state(p.name)


@functools.lru_cache(maxsize=None)
def _installed_state(name):
    p = plan(name)
    B, L = p.B, p.geo.levels
    g_t = torch.zeros(B, L, p.geo.table_size, p.geo.features, dtype=F64)
    g_d = [torch.zeros(B, *q.shape, dtype=F64) for q in p.params[0]]
    before = 0
    for call in model_calls(p):
        for b in range(B):
            r = _evaluate(p, call, b, p.tables[b].double(), [q.double() for q in p.params[b]], (p.bits, C.NOISE_SEED, p.k0, before), False, call["scale"])
            g_t[b] += torch.stack(r.table_grad)
            for i in range(6):
                g_d[i][b] += r.decoder_grads[i]
        before += call["target"].shape[1]
    gen = torch.Generator().manual_seed(17)

    def moments(g, per):
        """``per``: the leading axes that have a gmax of their own"""
        gmax = g.abs().reshape(*g.shape[:per], -1).max(dim=-1).values.reshape(*g.shape[:per], *([1] * (g.dim() - per)))
        assert float(gmax.min()) > 0
        m = (0.01 * gmax * (torch.rand(g.shape, generator=gen, dtype=F64) * 2 - 1)).float()
        v = ((p.factor * gmax) ** 2 * (1.001 + torch.rand(g.shape, generator=gen, dtype=F64))).float()
        assert bool((v.double() >= (p.factor * gmax) ** 2).all())
        return m, v

    return {"table": moments(g_t, 2), "decoder": [moments(g, 1) for g in g_d]}


@functools.lru_cache(maxsize=None)
def clean_report(name):
    p = plan(name)
    return V.verify(model_fit(p, installed_state(p)), case_of(p), what=f"model {name}", step_fn=cached_step)


# ------------------------------------------------------------------------------------------------------------------ the tests

@pytest.mark.parametrize("name", PLANS)
def test_clean_model_is_inside_a_thousandth_of_every_bound(name):
    rep = clean_report(name)
    assert len(rep.passes) == plan(name).epochs
    # the mip colours are fp32 DATA the model rounds once (half an ulp, 1/8 of that bound or less); everything else is float64 arithmetic
    worst = max((V.ratio(err, bound), q, e) for e, m in enumerate(rep.passes) for q, (err, bound) in m.items() if q != "layout | mip colours")
    assert worst[0] <= 1e-3, worst
    assert not rep.failures(), rep.failures()
    if plan(name).fresh:
        # case F: at least a quarter of the touched entries of every tensor qualify for the comparison of step 1
        print(f"MEASURED model {name} | shares | " + ", ".join(f"{k} {v:.2f}" for k, v in rep.share.items()))
        assert len(rep.share) == plan(name).geo.levels + 6 and min(rep.share.values()) >= 0.25, rep.share


@pytest.mark.parametrize("name", [n for n in PLANS if not plan(n).fresh])
def test_floor_of_the_free_running_model(name):
    """sqrt(min v) >= 0.09 gmax on every pass and tensor of the float64 model; the GPU asserts 0.08, the difference is room for the fp32
    trajectory.  A case that cannot hold it gets a larger installed factor (``FACTOR``), never a lower assertion."""
    rep = clean_report(name)
    assert sum(len(m) for m in rep.floor) > 0
    low = min((r, q, e) for e, m in enumerate(rep.floor) for q, r in m.items())
    print(f"MEASURED model {name} | floor | {low[0]:.4f} at pass {low[2]} {low[1]}")
    assert low[0] >= 0.09, low


EVERYWHERE = ("stale_gradient", "noise_offset_stuck", "exp_avg_sq_not_written_back", "freeze_one_epoch_late", "noise_after_the_freeze", "decoder_lr_on_the_table",
              "quantiser_truncates", "quantiser_depth_off_by_one", "freeze_of_an_older_table")


def test_where_the_mistakes_apply():
    """nine lines apply to every case; the others need a schedule, an installed state (case F compares no later parameters), more than one
    chunk, a ragged chunk or more than one field - and every line has cases"""
    for m in MISTAKES:
        there = [n for n in PLANS if first_pass_to_show(plan(n), m) is not None]
        assert len(there) == len(PLANS) if m in EVERYWHERE else len(there) >= 2, (m, there)
    assert [n for n in PLANS if first_pass_to_show(plan(n), "moments_of_the_field_before") is not None] == [n for n in PLANS if n.startswith("E-")]


@pytest.mark.parametrize("name,mistake", [(n, m) for n in PLANS for m in MISTAKES if first_pass_to_show(plan(n), m) is not None])
def test_teeth(name, mistake):
    """a deliberate mistake in the model moves a compared quantity by more than 20 x its bound, on every case it applies to
    (``first_pass_to_show``).  The model is stopped after the first pass at which the mistake can show: the passes before it are the clean
    model's and must pass."""
    p = plan(name)
    at = first_pass_to_show(p, mistake)
    rec = model_fit(p, installed_state(p), mistake=mistake, stop_after=at)
    rep = V.verify(rec, case_of(p), quiet=True, step_fn=cached_step)
    finite = [(V.ratio(err, bound), q) for q, (err, bound) in rep.passes[at].items() if bound > 0]
    exact = [q for q, (err, bound) in rep.passes[at].items() if bound == 0 and err > 0]
    if mistake in EXACT:
        print(f"MEASURED teeth {name} | {mistake} | pass {at} | exact checks failed: {exact}, entries: {rep.passes[at][EXACT[mistake]][0]:.0f}, excused as ties: {rep.ties}")
        assert EXACT[mistake] in exact and rep.passes[at][EXACT[mistake]][0] > 100, exact
        return
    best = max(finite)
    print(f"MEASURED teeth {name} | {mistake} | pass {at} | {best[1]} moves by {best[0]:.1f} x its bound | exact checks failed: {exact}")
    assert best[0] > TEETH, f"{mistake}: the largest movement is {best[0]:.2f} x the bound ({best[1]})"
    for e in range(at):
        assert not [q for q, (err, bound) in rep.passes[e].items() if not err <= bound], f"pass {e} is before the mistake"


def _old_step_bound(gmax, m_max, lr, betas, eps, step):
    """``_step_bound`` of tests/test_gpu_hashgrid_train_ref.py as it was before ``step_bound`` took the floor as an argument"""
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    gp = gmax * (1 + C.TOL_G)
    s0 = math.sqrt(b2) * 0.1 * gmax
    d0 = s0 / math.sqrt(bc2) + eps
    m1 = b1 * m_max + (1 - b1) * gp
    lip = lr / bc1 * ((1 - b1) / d0 + m1 * (1 - b2) * gp / (s0 * math.sqrt(bc2) * d0 * d0))
    return lip * C.TOL_G * gmax


@pytest.mark.parametrize("shape,mode", [((2, 2, 16), "crops"), ((3, 4, 8), "crops"), ((2, 2, 16), "points"), ((3, 4, 8), "points")],
                         ids=lambda v: v if isinstance(v, str) else C.shape_id(v))
def test_step_bound_is_the_function_it_replaces(shape, mode):
    """on the inputs of the existing optimiser-step cases (``StepCase`` of tests/test_gpu_hashgrid_train_ref.py): its two chunks' reference
    gradients summed (scale 1/2 each, keys (6, seed, 3, samples before the chunk)) on ``table_c`` clamped to 6 bits, per level and per decoder
    tensor, for the three fields of the batch case (crops) and for the field at points cut at 100; ``Moments`` of that file with its seed;
    both learning rates, step 4.  Without the eight entries ``put_edges`` moves onto the range's edges - they need no device, but change a
    level's gmax only if one of them carries it."""
    from tests.test_gpu_hashgrid_train_ref import ADAM_STEP, NUM_BITS as STEP_BITS, Moments
    gen = torch.Generator().manual_seed(17)
    n = 0
    for b in range(N_FIELDS if mode == "crops" else 1):
        i = C.inputs(*shape, b)
        table = i.table_c.clamp(*T.q_range(STEP_BITS))
        sizes = [100, i.points.shape[0] - 100] if mode == "points" else [i.n_chunk] * 2
        refs = []
        for k in range(2):
            if mode == "points":
                sl = slice(0, 100) if k == 0 else slice(100, None)
                kw = dict(points=i.points[sl], target=i.target_points[sl])
            else:
                kw = dict(origins=i.crops[k:k + 1], extent=i.extent, target=i.target[k * i.n_chunk:(k + 1) * i.n_chunk])
            refs.append(cached_step(i.geo, table, i.params, loss_scale=0.5, noise_key=(STEP_BITS, C.NOISE_SEED, ADAM_STEP, sum(sizes[:k])), **kw))
        grads = [refs[0].table_grad[l] + refs[1].table_grad[l] for l in range(shape[2])] + [refs[0].decoder_grads[j] + refs[1].decoder_grads[j] for j in range(6)]
        for g in grads:
            st = Moments(g, gen)
            for lr in (0.01, 0.005):
                old = _old_step_bound(st.gmax, float(st.m.abs().max()), lr, (0.9, 0.999), 1e-8, ADAM_STEP + 1)
                new = V.step_bound(st.gmax, float(st.m.abs().max()), lr, (0.9, 0.999), 1e-8, ADAM_STEP + 1, s0=math.sqrt(0.999) * 0.1 * st.gmax)
                assert new == old and old > 0
                n += 1
    assert n == 2 * (shape[2] + 6) * (N_FIELDS if mode == "crops" else 1)


def test_the_tie_allowance_excuses_a_rounding_boundary_and_nothing_else():
    """``_check_freeze`` on a table the test builds: an entry whose float64 x (2^b - 1) + 1/2 lies within 2^-20 of an integer may come out on
    either side; an entry that is not that close may not, and neither may an entry two codes off"""
    geo = T.geometry((8, 8), 2, 1, 10, 4)
    case = V.Case(geo=geo, bits=(6, 3), seed=0, k0=0, epochs=2, freeze_at=0.5, schedule=None)
    before = torch.zeros(1, 2, geo.table_size, 1, dtype=F64)
    s = [63.0, 7.0]
    before[0, 0, 0, 0] = (10.5 + 2.0 ** -22) / s[0]               # frac = 11 + 2^-22: a tie, the quantiser says 11
    before[0, 1, 0, 0] = (-2.5 - 2.0 ** -22) / s[1]               # frac = -2 - 2^-22: a tie, the quantiser says -3
    before[0, 0, 1, 0] = (10.5 + 2.0 ** -10) / s[0]               # no tie
    before[0, 0, 2, 0] = 0.3
    want = V.quantise_levels(before, (6, 3))
    assert float(want[0, 0, 0, 0]) == 11 / 63 and float(want[0, 1, 0, 0]) == -3 / 7

    def judged(got):
        out, rep = {}, V.Report()
        V._check_freeze(case, before, got.float(), out, rep)
        return out["freeze | table bits"][0], rep.ties

    assert judged(want) == (0.0, 0)
    got = want.clone()
    got[0, 0, 0, 0], got[0, 1, 0, 0] = 10 / 63, -2 / 7            # the other side of each boundary
    assert judged(got) == (0.0, 2)
    got[0, 0, 0, 0] = 12 / 63                                      # the wrong side: two codes from the other candidate
    assert judged(got) == (1.0, 1)
    got = want.clone()
    got[0, 0, 1, 0] = 10 / 63                                      # one code off where there is no tie
    assert judged(got) == (1.0, 0)
    got = want.clone()
    got[0, 0, 2, 0] += 2.0 ** -20                                  # not a code at all
    assert judged(got) == (1.0, 0)


@pytest.mark.parametrize("t_max", [1, 6, 7, 20])
def test_learning_rates_are_cosine_annealings(t_max):
    from neural_image_compression_v2_amd.optim import CosineAnnealing
    ps = [torch.zeros(1, requires_grad=True) for _ in range(2)]
    opt = torch.optim.SGD([{"params": [ps[0]], "lr": 0.01}, {"params": [ps[1]], "lr": 0.005}])
    sched = CosineAnnealing(opt, T_max=t_max, eta_min=0)
    want = V.learning_rates(t_max + 3, (0.01, 0.005), t_max)
    for e in range(t_max + 3):
        assert tuple(g["lr"] for g in opt.param_groups) == want[e], e
        sched.step()
    assert V.learning_rates(4, (0.01, 0.005), None) == [(0.01, 0.005)] * 4
    for e in range(t_max):                                                            # and the closed form the model uses
        assert abs(_cosine(0.01, e, t_max) - want[e][0]) <= 1e-15


@pytest.mark.parametrize("bits", range(1, 9))
def test_quantiser(bits):
    """idempotent; every x of ``q_range`` lands on a code of 0 .. 2^b - 1 at most half a step away (the top code's value 2^(b-1) / (2^b - 1)
    lies ABOVE the range's 1/2: the range is where the clamp holds the trained table, not the set of values); equals the dequantised save4fp
    code as ``oracle/hashgrid_ref.py`` reads it from a file's bytes"""
    lo, hi = T.q_range(bits)
    x = torch.cat([torch.linspace(lo, hi, 4097, dtype=F64), torch.tensor([lo, hi, 0.0], dtype=F64),
                   (torch.rand(4092, generator=torch.Generator().manual_seed(bits), dtype=F64) * (hi - lo) + lo).float().double()])
    q = V.quantise(x, bits)
    assert torch.equal(V.quantise(q, bits), q)
    s = (1 << bits) - 1
    code = torch.round(q * s).to(torch.int64) + (1 << (bits - 1)) - 1
    assert int(code.min()) == 0 and int(code.max()) == s and float((q - x).abs().max()) <= 0.5 / s + 1e-15
    spec = dict(field_size=(16, 16), levels=2, base=4, features=2, log2_table=12, fmt="u8", bits=bits, hidden=64, n_linear=3, scale=1.0)
    d = R.make_file(spec, 1)
    f = R.parse(d)
    sizes = [R.level_entries(f, l) * 2 for l in range(2)]
    assert sum(sizes) <= x.numel()
    codes, k = [], 0
    for n in sizes:
        u = torch.floor(x[k:k + n] * ((1 << bits) - 1) + 0.5).to(torch.int64) + (1 << (bits - 1)) - 1
        codes.append(u.numpy().reshape(-1, 2))
        k += n
    for fmt in ("u8", "bits1"):
        d2 = R.with_codes(R.make_file(dict(spec, fmt=fmt), 1), codes)
        vals = np.concatenate([v.reshape(-1) for v in R.table_values(R.parse(d2))])
        assert np.array_equal(vals, q[:k].numpy())
    assert torch.equal(V.quantise_levels(x.reshape(1, 2, -1, 2), (bits, bits))[0, 1], V.quantise(x.reshape(2, -1, 2)[1], bits))
