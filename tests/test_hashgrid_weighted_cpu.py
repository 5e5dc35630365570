"""CPU-only tests of the per-point loss weights of the training step at points (run with -m "not gpu"; DESIGN 4.7.26;
nic_hash_fused_forward_backward_points_weighted, csrc/hashgrid_weighted.hip; HashGridField.train_points_weighted /
train_points_weighted_differentiable / fit_points_weighted / fit_mips_weighted, hash_mip_weights).

The float64 reference is tests/hashgrid_weighted_ref.py's ``step``: the oracle's own pieces, the weighted loss
loss_scale sum_n w_n sum_o (y - t)^2 / (3 N), one ``torch.autograd.grad``.

- at w = 1 (None and ones) it is ``T.step`` with ``torch.equal`` in y, loss, row, the table and decoder gradients and dpoints, on every
  ``points*`` run of ``C.runs`` for all nine ``C.SHAPES``;
- it is held to differences of its own float64 loss: a table entry of every level and every decoder tensor (Richardson, the bound of
  tests/test_hashgrid_train_ref_cpu.py with the weights' largest value as one more factor of the loss's size), points inside a cell by the
  exactly linear row, lambda away from the kinks (central, h = 2^-10, 1e-9 of the largest dlod: 4.7.22's recipe);
- weights in {0, 1} on a run without noise equal ``T.step`` on the kept subset with loss_scale n_kept / N, to 1e-12;
- teeth: on the GPU tests' very inputs and weights each of six deliberate mistakes moves a compared quantity by more than ``C.TEETH`` x its
  bound.  "negative weights kept" can show only where a weight is negative: the mixed vector; the five others show on both vectors;
- host logic with the built library alone: signatures, refusals that leave the field's ``__dict__`` as it was, ``hash_mip_weights``, the symbol,
  its declaration and ctypes mirror, the host-check order of the C entry code by code (n_points <= 0 and refusals only: nothing launches)."""
import ctypes
import inspect
import re
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_train_ref as T
from tests import hashgrid_weighted_ref as W
from tests import test_hashgrid_train_ref_cpu as C
from tests.test_hashgrid_batch_points_cpu import ARG, NULL, OK, SHAPE, UNSUP, WORKSPACE, HEADER, EXT_HEADER, _desc, _mlp, _ref, lib  # noqa: F401
from tests.test_hashgrid_batch_lod_cpu import _bad_lods, _lod
from tests.test_hashgrid_lodtrain_cpu import _c_args, _quant
from tests.test_hashgrid_pointtrain_cpu import _grads
from tests.test_hashgrid_train_ref_cpu import SHAPES, TEETH, TOL_G, shape_id

ENTRY = "nic_hash_fused_forward_backward_points_weighted"
ARGS = ["desc", "lodp", "quant", "table", "points", "lod", "weight", "n_points", "order", "mlp", "target", "loss_scale", "table_grad", "mlp_grads", "loss",
        "y", "dpoints", "dlod", "flags", "workspace", "workspace_bytes", "tail", "stream"]
PTR = ctypes.c_void_p
UNIT = "hashgrid_weighted.hip"
POINT_RUNS = ["points", "points_noise", "points_lod", "points_lod_noise", "points_lod_uniform"] + [f"points_{n}" for n in C.PREFIXES]
KINDS = ("mixed", "last")

# ------------------------------------------------------------------------------------------------------------------ shared with the GPU file


def permutation(n):
    """the given order of the GPU file, int64 on the CPU"""
    return torch.randperm(n, generator=torch.Generator().manual_seed(11))


def step_kw(kw):
    """the keywords of ``W.step`` from a run of ``C.runs``"""
    return dict(table=kw["table"], target=kw["target"], points=kw["points"], loss_scale=kw["loss_scale"], noise_key=kw.get("noise_key"), lod=kw.get("lod"))


def measure(got, ref):
    """``C.measure`` and, where both have it, dlod over the reference's largest magnitude (TOL_G, as the lodtrain tests hold it)"""
    m = C.measure(got, ref)
    if getattr(ref, "dlod", None) is not None and getattr(got, "dlod", None) is not None:
        m["dlod"] = (C.relmax(got.dlod, ref.dlod), TOL_G)
    return m


# ------------------------------------------------------------------------------------------------------------------ the reference at w = 1
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_the_reference_at_ones_is_the_oracles_step(shape):
    inp = C.inputs(*shape)
    for run in POINT_RUNS:
        kw = C.runs(inp)[run]
        st = C.reference(*shape, run)
        n = kw["points"].shape[0]
        for weight in (None, np.ones(n, dtype=np.float32)):
            ref = W.step(inp.geo, params=inp.params, weight=weight, **step_kw(kw))
            pairs = [(ref.y, st.y), (ref.loss, st.loss), (ref.row, st.row), (ref.dpoints, st.dpoints)]
            pairs += list(zip(ref.table_grad, st.table_grad)) + list(zip(ref.decoder_grads, st.decoder_grads))
            assert all(torch.equal(a, b) for a, b in pairs), run
            assert (ref.dlod is None) == ("lod" not in kw)
    fr = W.step(inp.geo, params=inp.params, frozen=True, **step_kw(C.runs(inp)["points_lod_noise"]))
    st = C.reference(*shape, "points_lod_noise")
    assert fr.table_grad is None and torch.equal(fr.dpoints, st.dpoints) and all(torch.equal(a, b) for a, b in zip(fr.decoder_grads, st.decoder_grads))


# ------------------------------------------------------------------------------------------------------------------ differences of its own loss
@pytest.mark.parametrize("shape,run", [((2, 2, 16), "points_noise"), ((3, 4, 8), "points_lod_noise")], ids=lambda v: v if isinstance(v, str) else shape_id(v))
def test_the_reference_against_differences_of_its_own_loss(shape, run):
    inp = C.inputs(*shape)
    kw = step_kw(C.runs(inp)[run])
    geo = inp.geo
    n = kw["points"].shape[0]
    weight = W.weights(n, "mixed")
    ref = W.step(geo, params=inp.params, weight=weight, **kw)
    # the loss is a sum of 3 N squares, each times a weight <= 4: test_hashgrid_train_ref_cpu's bound on a loss of that size
    bound = C._fd_bound(ref.loss, n, geo.width) * 4.0

    def loss_with(table=None, params=None):
        k2 = dict(kw)
        if table is not None:
            k2["table"] = table
        return float(W.step(geo, params=inp.params if params is None else params, weight=weight, **k2).loss)

    def richardson(f):
        h = C.FD_H
        return (4 * (f(h) - f(-h)) / (2 * h) - (f(2 * h) - f(-2 * h)) / (4 * h)) / 3

    table64 = kw["table"].double()
    for l in range(geo.levels):                                            # a table entry of every level: the largest gradient of the level
        g = ref.table_grad[l]
        if float(g.abs().max()) == 0:
            continue
        ti, fi = divmod(int(g.abs().reshape(-1).argmax()), geo.features)

        def f(h, l=l, ti=ti, fi=fi):
            t = table64.clone()
            t[l, ti, fi] += h
            return loss_with(table=t)
        assert abs(richardson(f) - float(g[ti, fi])) <= bound, (l, ti, fi)
        assert abs(float(g[ti, fi])) > 100 * bound
    for k, g in enumerate(ref.decoder_grads):                              # every decoder tensor: its largest entry
        e = int(g.abs().reshape(-1).argmax())

        def f(h, k=k, e=e):
            ps = [p.double().clone() for p in inp.params]
            ps[k].reshape(-1)[e] += h
            return loss_with(params=ps)
        assert abs(richardson(f) - float(g.reshape(-1)[e])) <= bound, C.NAMES[k]
        assert abs(float(g.reshape(-1)[e])) > 100 * bound
    # points inside a cell at every level: test_position_gradient_matches_differences_of_the_row with the row gradient of the WEIGHTED loss
    tables = [table64[l] for l in range(geo.levels)]
    nz = None if kw["noise_key"] is None else torch.from_numpy(T.noise(n, geo.width, *kw["noise_key"]))
    wt = None if kw["lod"] is None else torch.from_numpy(T.level_weights(geo, n, *kw["lod"]))
    row = ref.row.clone().requires_grad_(True)
    loss = W.weighted_loss(T.decoder(row, [p.double() for p in inp.params]), kw["target"].double(), torch.from_numpy(ref.w), kw["loss_scale"])
    dx, = torch.autograd.grad(loss, row)
    _, moved = T.clamp_points(geo, kw["points"])
    t = T.rows(geo, points=kw["points"]).t.detach().to(torch.int64).numpy()
    den = 256 * geo.s_max
    inside = ~moved & (t >= 1) & (t + 1 <= 256 * np.array(geo.field_size)[None, :] - 1)
    for r in geo.resolutions:
        inside &= ((t - 1) * r // den == t * r // den) & ((t + 1) * r // den == t * r // den) & ((t * r) % den != 0)
    u, checked = 2.0 ** -53, 0
    for a in range(inp.dim):
        pm = []
        for s in (+1, -1):
            p = kw["points"].astype(np.float64).copy()
            p[:, a] += s / 256.0
            p32 = p.astype(np.float32)
            pm.append((T.encode(geo, tables, T.rows(geo, points=p32), nz, wt).detach(), (p32.astype(np.float64) == p)[:, a]))
        J = (pm[0][0] - pm[1][0]) * 128.0
        use = inside[:, a] & pm[0][1] & pm[1][1] & ~np.isnan(kw["points"]).any(axis=1)
        err = np.abs((dx * J).sum(dim=1).numpy() - ref.dpoints[:, a].numpy())
        lim = (dx.abs().sum(dim=1) * 256 * (2 ** inp.dim + inp.dim + 2) * u).numpy()
        assert use.sum() >= 50 and (err[use] <= lim[use]).all(), a
        checked += int(use.sum())
    assert checked >= 100 and (ref.dpoints.numpy()[moved] == 0.0).all()
    zero = torch.from_numpy(ref.w == 0)
    assert bool(zero.any()) and bool((ref.dpoints[zero] == 0).all())
    # lambda away from the kinks: central differences of the float64 loss in a float64 lambda, the noise held fixed
    if kw["lod"] is None:
        return
    fade, lod, uni = kw["lod"]
    from tests.test_hashgrid_lodgrad_cpu import ramp_f32
    a_raw, ramp, passes = ramp_f32(fade, lod, uni, n)
    with np.errstate(invalid="ignore"):
        raw = (np.asarray(lod, dtype=np.float32) + np.float32(uni)).astype(np.float32)
    away = (np.minimum(np.abs(a_raw), np.abs(a_raw - 1)) >= 2.0 ** -6).all(axis=1) & (raw >= 2.0 ** -6) & (raw <= 32 - 2.0 ** -6)
    h = 2.0 ** -10
    fd = np.asarray(fade, dtype=np.float64)
    pos = T.rows(geo, points=kw["points"])
    y_of = [p.double() for p in inp.params]

    def rows_loss(lam):
        wl = torch.from_numpy(np.clip((fd[None, :] - np.clip(lam, 0.0, 32.0)[:, None]) + 1.0, 0.0, 1.0))
        y = T.decoder(T.encode(geo, tables, pos, nz, wl), y_of)
        return ((torch.from_numpy(ref.w)[:, None] * (y - kw["target"].double()) ** 2).sum(dim=1) / (3 * n) * kw["loss_scale"]).detach().numpy()
    safe = np.where(away, raw.astype(np.float64), 1.0)
    # behind the decoder the loss is curved in lambda, so Richardson as above: 2 h = 2^-9 stays inside the linear piece of every level weight
    cd = (4 * (rows_loss(safe + h) - rows_loss(safe - h)) / (2 * h) - (rows_loss(safe + 2 * h) - rows_loss(safe - 2 * h)) / (4 * h)) / 3
    err = np.abs(cd - ref.dlod.numpy())[away].max() / float(ref.dlod.abs().max())
    assert (away & ramp.any(axis=1) & (ref.w > 0)).sum() >= 20 and err <= 1e-9, err
    assert bool((ref.dlod[zero] == 0).all()) and bool((ref.dlod[torch.from_numpy(~passes)] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ weights in {0, 1}
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_a_mask_is_the_step_on_the_kept_subset(shape):
    inp = C.inputs(*shape)
    for run in ("points", "points_lod"):
        kw = step_kw(C.runs(inp)[run])
        n = kw["points"].shape[0]
        keep = torch.rand(n, generator=torch.Generator().manual_seed(5)) < 0.5
        keep[:4] = torch.tensor([True, False, True, False])
        ref = W.step(inp.geo, params=inp.params, weight=keep.float().numpy(), **kw)
        k = keep.numpy()
        lod = kw["lod"]
        sub = T.step(inp.geo, kw["table"], inp.params, kw["target"][keep], points=kw["points"][k], loss_scale=kw["loss_scale"] * int(k.sum()) / n,
                     lod=None if lod is None else (lod[0], None if lod[1] is None else lod[1][k], lod[2]))
        pairs = [(ref.y[keep], sub.y), (ref.loss, sub.loss), (ref.dpoints[keep], sub.dpoints)] + list(zip(ref.table_grad, sub.table_grad))
        pairs += list(zip(ref.decoder_grads, sub.decoder_grads))
        for a, b in pairs:
            assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), run
        assert bool((ref.dpoints[~keep] == 0).all()) and (ref.dlod is None or bool((ref.dlod[~keep] == 0).all()))


# ------------------------------------------------------------------------------------------------------------------ teeth
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_teeth_the_mistakes_are_each_seen_on_the_gpu_tests_inputs(shape):
    inp = C.inputs(*shape)
    kw = step_kw(C.runs(inp)["points_lod_noise"])
    n = kw["points"].shape[0]
    order = permutation(n).numpy()
    assert not np.array_equal(order, np.arange(n))
    for kind in KINDS:
        weight = W.weights(n, kind, None if kind == "mixed" else order[n - 1])
        ref = W.step(inp.geo, params=inp.params, weight=weight, **kw)
        for mistake in W.MISTAKES:
            if mistake == "negative weights kept" and not (weight < 0).any():
                continue
            bad = W.step(inp.geo, params=inp.params, weight=weight, mistake=mistake, order=order, **kw)
            q, ratio = C.worst(measure(bad, ref))
            print(f"{shape_id(shape)} {kind} | {mistake}: {q} moves by {ratio:.1f} x its bound")
            assert ratio > TEETH, (kind, mistake, q, ratio)


def test_the_weight_vectors():
    n = C.G.N_POINTS
    w = W.weights(n, "mixed")
    assert w.dtype == np.float32 and np.isnan(w[1]) and w[2] < 0 and (w[4::5] == 0).all() and np.nanmax(w) < 4 and (w > 1).any() and (w[w > 0] < 1).any()
    c = W.clamp_weight(w, n)
    assert c[1] == 0 and c[2] == 0 and (c >= 0).all() and (c[w > 0] == w[w > 0]).all()
    last = W.weights(n, "last")
    assert (last != 0).sum() == 1 and last[n - 1] == W.LAST_WEIGHT and n - 1 >= 64 * (n // 64) and n % 64 != 0      # in the last, partial wave
    assert W.weights(1, "mixed").shape == (1,) and W.weights(1, "mixed")[0] > 0
    assert (W.clamp_weight(None, 5) == 1).all()


# ------------------------------------------------------------------------------------------------------------------ the C entry
def _fus(lib, d, lodp="default", q=None, table=16, pts=16, lod=0, weight=0, n=0, order=0, m="default", target=16, tg=16, gs="default", loss=16, y=0,
         dpoints=16, dlod=16, flags=0, ws=16, ws_bytes=1 << 30, tail=None):
    """the return code of the entry.  Every pointer is a dummy that is never dereferenced: n_points <= 0 only, so nothing launches"""
    lodp = _lod() if lodp == "default" else lodp
    m = _mlp() if m == "default" else m
    gs = _grads() if gs == "default" else gs
    assert n <= 0 or order
    return getattr(lib, ENTRY)(_ref(d), _ref(lodp), _ref(q), PTR(table), PTR(pts), PTR(lod), PTR(weight), n, PTR(order), _ref(m), PTR(target), 1.0, PTR(tg),
                               _ref(gs), PTR(loss), PTR(y), PTR(dpoints), PTR(dlod), flags, PTR(ws), ws_bytes, _ref(tail), None)


def test_the_entry_is_exported_declared_in_the_companion_header_and_mirrored(lib):
    from neural_image_compression_v2_amd import _build, _lib, hashgrid
    import neural_image_compression_v2_amd as pkg
    header, ext = open(HEADER).read(), open(EXT_HEADER).read()
    assert hasattr(lib, ENTRY) and ENTRY not in header and ENTRY not in _lib.SIGNATURES and ENTRY in _lib.EXT_SIGNATURES
    res, args = _lib.EXT_SIGNATURES[ENTRY]
    cargs = _c_args(ext, ENTRY)
    assert res is ctypes.c_int and [c.split()[-1].lstrip("*") for c in cargs] == ARGS and len(args) == len(ARGS)
    # the _grad_lod sibling argument for argument, with weight after lod
    sargs = _c_args(ext, "nic_hash_fused_forward_backward_points_grad_lod")
    k = [c.split()[-1].lstrip("*") for c in sargs].index("lod")
    assert cargs == sargs[:k + 1] + ["const float *weight"] + sargs[k + 1:]
    sig = _lib.EXT_SIGNATURES["nic_hash_fused_forward_backward_points_grad_lod"][1]
    assert args == sig[:k + 1] + [ctypes.c_void_p] + sig[k + 1:]
    fn = getattr(lib, ENTRY)
    assert fn.restype is res and list(fn.argtypes) == args
    declared = set(re.findall(r"\b(nic_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", ext, flags=re.S)))
    assert declared == set(_lib.EXT_SIGNATURES) and len(_lib.SIGNATURES) == 86 and _lib.NIC_ABI_VERSION == 9 == lib.nic_abi_version()
    for name in ("hash_fused_forward_backward_points_weighted", "hash_mip_weights"):
        assert getattr(pkg, name) is getattr(hashgrid, name)
    comment = " ".join(ext[ext.index("WEIGHT PER POINT"):ext.index(f"int {ENTRY}(")].replace("*", " ").split())
    for words in ("w_n = weight[n] > 0 ? weight[n] : 0", "+inf is the caller's error", "weight == NULL is w = 1", "/ (3 n_points)", "n_points, not sum w",
                  "adds exactly +0 to the loss", "keeps its value", "lod without lodp, dlod without lodp, dlod without dpoints", "bit for bit",
                  "table_grad == NULL is a frozen table"):
        assert words in comment, words
    # the unit is in the build, made of the shared pieces, with no atomics of its own
    assert UNIT in _build.SOURCES and len(set(_build.SOURCES)) == len(_build.SOURCES)
    unit = open(f"{_build.CSRC}/{UNIT}").read()
    for piece in ("hash_points_weighted_train_kernel<D, F, 2, NOISE, WALK>", "hash_points_weighted_train_kernel<D, F, 1, NOISE, WALK>",
                  "encode_point<D, F, NIC_HASH_SRC_F32, NOISE, false, true>(s, t, row, lam, xrow)", "decoder_train_half<KT, true>(", "scatter_point<D, F, true>(",
                  "point_walk<D, F, NIC_HASH_SRC_F32, true, DLOD, NOISE && DLOD>(", "write_record<KT>(", "open_fused_points(", "fill_fused_points(",
                  "points_fused_step(", "w = w > 0.f ? w : 0.f;", "__fmul_rn(s.dscale, w)"):
        assert piece in unit, piece
    assert "atomicAdd" not in unit and "check_fused_tail(" not in unit and "finish_fused_step(" not in unit


def test_entry_argument_errors_in_the_documented_order(lib):
    from neural_image_compression_v2_amd import _lib
    d = _desc(resolutions=(16, 64))
    for kw in (dict(), dict(lod=16), dict(weight=16), dict(tg=0), dict(y=16), dict(order=16), dict(flags=3), dict(q=_quant()), dict(dlod=0), dict(dpoints=0, dlod=0),
               dict(lodp=None, dlod=0), dict(lodp=None, dpoints=0, dlod=0, weight=16)):
        assert _fus(lib, d, **kw) == OK, kw                                    # n_points == 0: NIC_OK, nothing written
    # 1. null desc / mlp; the fused set; the descriptor of a point source: open_fused_points' codes, before every pointer
    assert _fus(lib, None) == NULL and _fus(lib, d, m=None) == NULL and _fus(lib, None, lodp=None, pts=0, n=-1, ws_bytes=16) == NULL
    bad = _desc()
    bad.flags = 1
    wide = _desc(resolutions=(16,) * 9, features=8)
    big = _desc(resolutions=(1, 1), s_max=1 << 22, extent=(8, 8, 1))
    for desc, want in [(bad, ARG), (_desc(features=3), UNSUP), (_desc(dim=4), UNSUP), (_desc(log2_table=9), ARG), (wide, UNSUP), (_desc(num_crops=2), SHAPE),
                       (big, ARG)]:
        assert _fus(lib, desc) == want and _fus(lib, desc, lodp=None, table=0, dpoints=0, flags=4, n=-1, ws_bytes=16) == want
    assert _fus(lib, d, m=_mlp(5, 5)) == UNSUP
    # 2. null pointers: before flags, the combinations, the nic_hash_lod, quant, n_points, the workspace and the tail
    for kw in (dict(table=0), dict(pts=0), dict(target=0), dict(loss=0), dict(ws=0), dict(gs=None), dict(m=_mlp(3, 2))):
        assert _fus(lib, d, **kw) == NULL, kw
        assert _fus(lib, d, flags=4, lodp=_lod(reserved=1), q=_quant(bits=0), n=-1, ws_bytes=16, **kw) == NULL, kw
        assert _fus(lib, d, lodp=None, lod=16, **kw) == NULL, kw
    # 3. flags: before the combinations and the nic_hash_lod (all NIC_E_ARG; quant's NIC_E_UNSUPPORTED tells them from what follows)
    tensor_noise = _quant(mode=1)
    assert _fus(lib, d, flags=4) == ARG and _fus(lib, d, flags=-1) == ARG and _fus(lib, d, flags=4, q=tensor_noise, n=-1, ws_bytes=16) == ARG
    # 4. lod without lodp, dlod without lodp, dlod without dpoints: before quant
    assert _fus(lib, d, q=tensor_noise) == UNSUP
    for kw in (dict(lodp=None, lod=16, dlod=0), dict(lodp=None), dict(lodp=None, dpoints=0), dict(dpoints=0)):
        assert _fus(lib, d, **kw) == ARG and _fus(lib, d, q=tensor_noise, n=-1, ws_bytes=16, **kw) == ARG, kw
    # 5. the nic_hash_lod where given: before quant
    for lp in _bad_lods():
        assert _fus(lib, _desc(), lodp=lp) == ARG and _fus(lib, _desc(), lodp=lp, q=tensor_noise, n=-1, ws_bytes=16) == ARG
    assert _fus(lib, d, lodp=_lod((1.0, 1.0, -1.0, float("nan")))) == OK       # fade entries past desc->levels are ignored
    # 6. points_fused_step's own checks in its order: quant, n_points, the workspace, the tail, n_points == 0
    for q in (_quant(bits=0), _quant(bits=9), _quant(base=-1), _quant(mode=7)):
        assert _fus(lib, d, q=q) == ARG
    assert _fus(lib, d, q=tensor_noise, n=-1, ws_bytes=16) == UNSUP and _fus(lib, d, q=_quant(mode=0, bits=8)) == OK
    assert _fus(lib, d, n=-1) == ARG and _fus(lib, d, n=-(1 << 40)) == ARG and _fus(lib, d, n=1 << 31, order=16) == ARG and _fus(lib, d, n=-1, ws_bytes=16) == ARG
    need = lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(d), ctypes.byref(_mlp()))
    assert need > 16 and _fus(lib, d, ws_bytes=need) == OK and _fus(lib, d, ws_bytes=need - 1) == WORKSPACE and _fus(lib, d, ws_bytes=16) == WORKSPACE
    gs = _grads()

    def tail_of(grad, count=1, n_stream=0):
        arr = (_lib.NicAdamTensor * 1)(_lib.NicAdamTensor(0x2000, grad, 0x3000, 0x4000, 64, 1, 0.005, 1.0, -1.0, 0, 0, 0))
        t = _lib.NicStepTail()
        t.tensors = ctypes.cast(arr, ctypes.c_void_p).value
        t.count, t.n_stream, t.beta1, t.beta2, t.eps = count, n_stream, 0.9, 0.999, 1e-8
        t._keep = arr
        return t

    assert _fus(lib, d, gs=gs, tail=tail_of(gs.w[0])) == OK and _fus(lib, d, gs=gs, tail=tail_of(0x7000)) == ARG
    assert _fus(lib, d, gs=gs, tail=tail_of(gs.w[0], count=0)) == ARG and _fus(lib, d, gs=gs, tail=tail_of(0x7000), ws_bytes=16) == WORKSPACE
    for desc in (_desc(dim=3, resolutions=(4, 6, 9, 12), features=1, s_max=12, extent=(12, 10, 9)), _desc(features=8, resolutions=(16,) * 4),
                 _desc(resolutions=(16,) * 5, features=8)):
        assert _fus(lib, desc) == OK and _fus(lib, desc, q=_quant(bits=4, base=9), lod=16, weight=16, order=16) == OK
        assert _fus(lib, desc, lodp=None, dpoints=0, dlod=0) == OK and _fus(lib, desc, lodp=None, dlod=0) == OK


# ------------------------------------------------------------------------------------------------------------------ Python: signatures, refusals
def test_the_python_signatures():
    from neural_image_compression_v2_amd import hashgrid
    sib = list(inspect.signature(hashgrid.hash_fused_forward_backward_points_grad_lod).parameters)
    k = sib.index("target")
    sig = inspect.signature(hashgrid.hash_fused_forward_backward_points_weighted).parameters
    assert list(sig) == sib[:k + 1] + ["weight"] + sib[k + 1:]
    assert sig["lod"].default is None and sig["dpoints"].default is None and sig["dlod"].default is None
    cls = hashgrid.HashGridField
    sig = inspect.signature(cls.train_points_weighted).parameters
    assert list(sig) == ["self", "points", "target", "weight", "lod", "dpoints", "dlod", "accumulate", "scale", "step", "noise", "order", "fused"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, None, None, False, 1.0, True, None, None, False]
    assert sig["weight"].default is inspect.Parameter.empty
    sig = inspect.signature(cls.train_points_weighted_differentiable).parameters
    assert list(sig) == ["self", "points", "target", "weight", "lod", "kwargs"] and sig["lod"].default is None
    assert sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    sig = inspect.signature(cls.fit_points_weighted).parameters
    assert list(sig) == ["self", "points", "target", "weight", "epochs", "batch", "order", "fused", "freeze_at", "lod"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, "cell", None, 0.95, None]
    sig = inspect.signature(cls.fit_mips_weighted).parameters
    assert list(sig) == ["self", "target", "epochs", "mips", "mip_weights", "batch", "order", "fused", "freeze_at"]
    assert [sig[k].default for k in list(sig)[3:]] == [2, None, None, "cell", None, 0.95]
    assert list(inspect.signature(hashgrid.hash_mip_weights).parameters) == ["n_points_per_mip", "mode"]
    # the existing ones are as they were
    tp = inspect.signature(cls.train_points).parameters
    assert list(tp) == ["self", "points", "target", "accumulate", "scale", "step", "noise", "order", "fused", "lod", "dpoints"]
    assert list(inspect.signature(cls.fit_points).parameters) == ["self", "points", "target", "epochs", "batch", "order", "fused", "freeze_at", "lod"]
    assert list(inspect.signature(cls.fit_mips).parameters) == ["self", "target", "epochs", "mips", "batch", "order", "fused", "freeze_at"]


def test_hash_mip_weights():
    from neural_image_compression_v2_amd.hashgrid import hash_mip_weights
    counts = (4096, 1024, 256)
    w = hash_mip_weights(counts, "balanced")
    n = sum(counts)
    assert w == tuple(n / (3 * c) for c in counts) and hash_mip_weights(counts) == w
    # the weighted loss over the joint set is the mean of the per-mip means: sum_m w_m N_m e_m / N = sum_m e_m / (M + 1)
    assert all(abs(wm * c / n - 1 / 3) < 1e-15 for wm, c in zip(w, counts))
    assert hash_mip_weights(counts, [1, 0, 2.5]) == (1.0, 0.0, 2.5) and hash_mip_weights([7], "balanced") == (1.0,)
    for bad in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], [1.0, -1.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0], "even", 3.0, [1.0, "x", 2.0]):
        with pytest.raises(ValueError):
            hash_mip_weights(counts, bad)
    for bad in ([], [0, 4], [-1]):
        with pytest.raises(ValueError):
            hash_mip_weights(bad, "balanced")


def test_the_field_refuses_on_the_host():
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, HashGridField, level_resolutions

    def bare(size=(96, 80), level_bits=None, table="present"):
        f = HashGridField.__new__(HashGridField)
        f.field_size, f.device, f.level_bits = size, torch.device("cpu"), level_bits
        f.geo = HashGeometry(size, tuple(level_resolutions(8, 16, max(size))), 2, 12)
        f.table = None if table is None else torch.zeros(1)
        f.hidden, f.n_linear, f.route, f.frozen, f.num_bits, f._lod_fade = 64, 3, "fused", False, None, None
        return f
    pts, target, w = torch.zeros(5, 2), torch.zeros(5, 3), torch.ones(5)
    dp, dl = torch.full((5, 2), 7.0), torch.full((5,), 7.0)
    image = torch.zeros(96, 80, 3)
    g = bare(table=None)
    before = dict(g.__dict__)
    for call in (lambda: g.train_points_weighted(pts, target, w), lambda: g.train_points_weighted(pts, target, w, 1.0, dp, dl, fused=True),
                 lambda: g.train_points_weighted_differentiable(pts.clone().requires_grad_(), target, w),
                 lambda: g.train_points_weighted_differentiable(pts, target, w, torch.tensor(1.0, requires_grad=True)),
                 lambda: g.fit_points_weighted(pts, target, w, 1), lambda: g.fit_mips_weighted(image, 1)):
        with pytest.raises(RuntimeError, match="decodes only"):
            call()
    assert g.__dict__ == before
    g = bare(level_bits=(8,) * 8)
    before = dict(g.__dict__)
    for call in (lambda: g.train_points_weighted(pts, target, w), lambda: g.train_points_weighted(pts, target, w, torch.zeros(5), fused=True),
                 lambda: g.train_points_weighted_differentiable(pts.clone().requires_grad_(), target, w),
                 lambda: g.fit_points_weighted(pts, target, w, 1), lambda: g.fit_mips_weighted(image, 1, mip_weights="balanced")):
        with pytest.raises(NotImplementedError, match="bit depth per level"):
            call()
    assert g.__dict__ == before
    f = bare()
    before = dict(f.__dict__)
    with pytest.raises(TypeError):
        f.train_points_weighted(pts, target)                                   # weight is required
    for bad in (torch.zeros(5, 3), torch.zeros(5), [[0.0, 0.0]] * 5):
        with pytest.raises(ValueError, match="points must be"):
            f.train_points_weighted(bad, target, w)
    for call in (f.train_points_weighted, lambda p, t, ww: f.fit_points_weighted(p, t, ww, 1)):
        for bad in (None, [1.0] * 5, 1.0):
            with pytest.raises(ValueError, match="weight must be an fp32"):
                call(pts, target, bad)
        for bad in (torch.ones(4), torch.ones(5, 1), torch.ones(()), torch.ones(5, 3)):
            with pytest.raises(ValueError, match=r"weight must be \[5\]"):
                call(pts, target, bad)
        with pytest.raises(ValueError, match="dtype"):
            call(pts, target, torch.ones(5, dtype=torch.float64))
        with pytest.raises(ValueError, match="contiguous"):
            call(pts, target, torch.ones(10)[::2])
        with pytest.raises(RuntimeError, match="HIP device"):                  # a host tensor of the right shape: no CPU path
            call(pts, target, w)
    with pytest.raises(ValueError, match="dlod needs lod"):
        f.train_points_weighted(pts, target, w, None, dp, dl)
    with pytest.raises(ValueError, match="dlod needs dpoints"):
        f.train_points_weighted(pts, target, w, 1.0, None, dl)
    with pytest.raises(ValueError, match=r"dlod must be \[5\]"):
        f.train_points_weighted(pts, target, w, 1.0, dp, torch.zeros(4))
    for kw in (dict(dpoints=dp), dict(dlod=dl)):
        with pytest.raises(TypeError, match="dpoints and dlod"):
            f.train_points_weighted_differentiable(pts.clone().requires_grad_(), target, w, 1.0, **kw)
    for bad in ("even", [1.0, 2.0], [1.0, -1.0, 1.0]):
        with pytest.raises(ValueError):
            f.fit_mips_weighted(image, 1, mip_weights=bad)
    with pytest.raises(ValueError, match="target must be"):
        f.fit_mips_weighted(torch.zeros(96, 81, 3), 1)
    assert f.__dict__ == before and bool((dp == 7.0).all()) and bool((dl == 7.0).all())


def test_the_functional_wrapper_refuses_on_the_host():
    from neural_image_compression_v2_amd import hashgrid
    geo = hashgrid.HashGeometry((96, 80), tuple(hashgrid.level_resolutions(8, 16, 96)), 2, 12)
    pts, dp, dl = torch.zeros(5, 2), torch.zeros(5, 2), torch.zeros(5)
    args = (geo, torch.zeros(1), pts, [], torch.zeros(5, 3))
    with pytest.raises(ValueError, match="dlod needs dpoints"):
        hashgrid.hash_fused_forward_backward_points_weighted(*args, torch.ones(5), [], dlod=dl)
    with pytest.raises(ValueError, match=r"dpoints must be \[5, 2\]"):
        hashgrid.hash_fused_forward_backward_points_weighted(*args, torch.ones(5), [], dpoints=torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        hashgrid.hash_fused_forward_backward_points_weighted(*args, torch.ones(5), [], dpoints=dp, dlod=dl)
