"""Judgement of a RECORDED hash-grid fit, optimiser step by optimiser step, in float64 (test infrastructure) - what
``oracle/hashgrid_train_ref.py`` is for one step, for the loops that take many: ``HashGridField.fit`` / ``fit_points`` / ``fit_mips`` and
``HashGridFieldBatch.fit`` / ``fit_points``.

A free-running fp32 trajectory drifts from a float64 one and no tolerance for that drift can be derived, so a fit is never compared as a
whole.  A ``Recording`` holds, per pass, the state the pass STARTED from (tables, decoder tensors, every ``exp_avg`` / ``exp_avg_sq`` /
``step``), every call of the pass with the arguments it received and the loss it returned, the table-gradient buffer after a call that did
not step, and the state after the step.  ``verify`` judges each pass alone from its recorded pre-state - fp32 values, exact in float64:
``T.step`` per call at the pre-state, the gradients summed, ``T.adam_step`` with the verifier's OWN learning rate and step count - against
the recorded post-state, within the per-step bound of DESIGN 4.7.17.  Errors do not compound.  Because every written-back value is the next
pass's given, the moments and step counts after every step are compared too.

The rules are written once, from the docstrings of the fit methods and from ``include/nicv2_hip.h``: the noise key of call k of pass e is
(bits, seed, K0 + e, samples of the pass before the call), none once frozen; a chunk advances the pass by the rows of the call (a batch: the
padded width N); a call's loss weight is the ``scale`` it was given and the scales of a pass sum to 1; the freeze falls before pass
ceil(freeze_at * epochs); the learning rate of step e is ``torch.optim.lr_scheduler.CosineAnnealingLR``'s on a dummy ``torch.optim.Adam``.

Plain CPU code; imports ``hashgrid_train_ref`` and nothing of ``neural_image_compression_v2_amd``.  The GPU recorder
(tests/test_gpu_hashgrid_fit_ref.py) and the float64 model fit (tests/test_hashgrid_fit_ref_cpu.py) both produce a ``Recording``."""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from oracle import hashgrid_train_ref as T

TOL_Y, TOL_G = 5e-6, 1e-4          # the project's bounds for fp32 against a reference: y and loss; every gradient
NAMES = ["W1", "b1", "W2", "b2", "W3", "b3"]
TIE = 2.0 ** -20                   # a float64 x (2^b - 1) + 1/2 this close to an integer may round either way in fp32
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------ the recording

@dataclass
class State:
    """everything a step reads and writes, for B fields (a single field is B = 1): ``tables`` [B, L, T, F], ``params`` six tensors [B, ..],
    the table's Adam state (exp_avg, exp_avg_sq [B, L, T, F], step) or None where the optimiser holds none, the same per decoder tensor"""
    tables: torch.Tensor
    params: List[torch.Tensor]
    table_moments: Optional[Tuple[torch.Tensor, torch.Tensor, int]]
    decoder_moments: List[Tuple[torch.Tensor, torch.Tensor, int]]


@dataclass
class Call:
    """one ``train_step`` (``origins`` [B, num_crops, dim] + ``extent``) or ``train_points`` (``points`` [B, N, dim] fp32, ``lod`` None / a
    float / fp32 [N], ``counts`` None or B ints) as the method received it, the [B] losses it returned, and after ``step=False`` the public
    table-gradient buffer [B, L, T, F]"""
    target: torch.Tensor
    accumulate: bool
    scale: float
    step: bool
    loss: torch.Tensor
    origins: Optional[np.ndarray] = None
    extent: Optional[Tuple[int, ...]] = None
    points: Optional[np.ndarray] = None
    lod: Union[None, float, np.ndarray] = None
    counts: Optional[Sequence[int]] = None
    grad: Optional[torch.Tensor] = None

    @property
    def rows(self) -> int:
        return int(self.target.shape[1])


@dataclass
class Pass:
    """``unfrozen_table`` / ``frozen_table``: the tables right before and right after a ``freeze()`` that ran before this pass's first call
    (else None) - ``pre`` is taken at the first call, so at the freeze pass it already holds the quantised table; ``steps``: the field's own
    ``steps`` counter before the pass"""
    pre: State
    steps: int
    calls: List[Call] = field(default_factory=list)
    post: Optional[State] = None
    frozen_table: Optional[torch.Tensor] = None
    unfrozen_table: Optional[torch.Tensor] = None


@dataclass
class Recording:
    passes: List[Pass] = field(default_factory=list)
    returned: Optional[List[List[float]]] = None          # what fit* returned: [epochs][B]


@dataclass
class Case:
    """what ``verify`` is told about a fit - never read from the objects under test.  ``bits``: one depth or one per level; ``k0``: the
    optimiser steps taken before the fit; ``schedule``: T_max of the cosine schedule or None; ``fresh``: the optimiser's own zero state (case
    F: step 1 has no Lipschitz bound, see ``verify``); ``chunks``: the rows of the calls of a pass; ``rows``: per field the (points [N, dim],
    target [N, 3], lod [N] or None) set a ``fit_points`` pass must hold, real rows only; ``mips``: (target [S.., 3] fp32, mips) of ``fit_mips``"""
    geo: T.Geometry
    bits: Union[int, Tuple[int, ...]]
    seed: int
    k0: int
    epochs: int
    freeze_at: float
    schedule: Optional[int]
    base_lrs: Tuple[float, float] = (0.01, 0.005)
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    fade: Optional[Tuple[float, ...]] = None
    fresh: bool = False
    chunks: Optional[Sequence[int]] = None
    rows: Optional[list] = None
    mips: Optional[tuple] = None

    @property
    def freeze_epoch(self) -> int:
        return math.ceil(self.freeze_at * self.epochs)

    def level_bits(self) -> Tuple[int, ...]:
        return tuple(self.bits) if isinstance(self.bits, (tuple, list)) else (int(self.bits),) * self.geo.levels


@dataclass
class Report:
    """``passes[e]``: quantity -> (error, bound) - a quantity whose bound differs from entry to entry is reported as (the largest error /
    bound, 1), an exact check as (violations, 0); ``floor[e]``: tensor -> sqrt(min v) / gmax of the pre-state (tensors with a gradient);
    ``ties``: table entries within ``TIE`` of a rounding boundary that the freeze put one code off; ``share``: tensor -> the share of touched
    entries whose step-1 update is compared (``fresh``)"""
    passes: List[Dict[str, Tuple[float, float]]] = field(default_factory=list)
    floor: List[Dict[str, float]] = field(default_factory=list)
    ties: int = 0
    share: Dict[str, float] = field(default_factory=dict)

    def failures(self) -> List[str]:
        return [f"pass {e} {q}: {err:.3e} > {bound:.3e}" for e, m in enumerate(self.passes) for q, (err, bound) in m.items() if not err <= bound]

    def min_floor(self) -> float:
        return min((r for m in self.floor for r in m.values()), default=math.inf)


def ratio(err: float, bound: float) -> float:
    if bound > 0:
        return err / bound
    return 0.0 if err == 0 else math.inf


# ------------------------------------------------------------------------------------------------------------------ the rules

def learning_rates(steps: int, base_lrs: Sequence[float], t_max: Optional[int]) -> List[Tuple[float, ...]]:
    """the learning rates of optimiser steps 0 .. steps - 1 per group: ``CosineAnnealingLR(T_max, eta_min=0)`` stepped after every step of a
    dummy ``torch.optim.Adam`` with the groups' base rates; constant without a schedule"""
    if t_max is None:
        return [tuple(float(b) for b in base_lrs)] * steps
    ps = [torch.zeros(1, requires_grad=True) for _ in base_lrs]
    opt = torch.optim.Adam([{"params": [p], "lr": float(b)} for p, b in zip(ps, base_lrs)])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=int(t_max), eta_min=0)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(steps):
            out.append(tuple(float(g["lr"]) for g in opt.param_groups))
            for p in ps:
                p.grad = torch.zeros(1)
            opt.step()
            sched.step()
    return out


def quantise(x, bits: int) -> torch.Tensor:
    """the header's ``floor(x (2^b - 1) + 1/2) / (2^b - 1)`` in float64"""
    s = float((1 << int(bits)) - 1)
    return torch.floor(T.as_f64(x) * s + 0.5) / s


def quantise_levels(table, level_bits: Sequence[int]) -> torch.Tensor:
    """``quantise`` of a [.., L, T, F] table, level l with b_l"""
    t = T.as_f64(table)
    return torch.stack([quantise(t[..., l, :, :], b) for l, b in enumerate(level_bits)], dim=-3)


def ulp32(x) -> torch.Tensor:
    a = T.as_f64(x).abs().numpy().astype(np.float32)
    return torch.from_numpy(np.spacing(a).astype(np.float64))


def step_bound(gmax: float, m_max: float, lr: float, betas, eps: float, step: int, s0: float) -> float:
    """the Lipschitz constant of Adam's update in the gradient, times TOL_G gmax (``StepCase`` of tests/test_gpu_hashgrid_train_ref.py
    derives it): ``s0`` is a floor of sqrt(exp_avg_sq') that holds for EVERY gradient - sqrt(beta2 min v)"""
    b1, b2 = betas
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    gp = gmax * (1 + TOL_G)
    d0 = s0 / math.sqrt(bc2) + eps
    m1 = b1 * m_max + (1 - b1) * gp                      # |m'| <= this
    lip = lr / bc1 * ((1 - b1) / d0 + m1 * (1 - b2) * gp / (s0 * math.sqrt(bc2) * d0 * d0))
    return lip * TOL_G * gmax


def relmax(a, b) -> float:
    """max |a - b| over max |b|; a reference that is all zero admits no error"""
    a, b = T.as_f64(a), T.as_f64(b)
    num, den = float((a - b).abs().max()), float(b.abs().max())
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)


def _bits32(x) -> np.ndarray:
    return np.ascontiguousarray(T.as_f64(x).numpy().astype(np.float32)).view(np.uint32)


def _bits32_t(x) -> torch.Tensor:
    return torch.from_numpy(_bits32(x).astype(np.int64))


def _same_bits(a, b) -> int:
    """how many entries differ once both are fp32"""
    return int((_bits32(a) != _bits32(b)).sum())


def _sorted_rows(cols: Sequence[np.ndarray]) -> np.ndarray:
    m = np.concatenate([np.ascontiguousarray(np.asarray(c, dtype=np.float32).reshape(len(c), -1)).view(np.uint32) for c in cols], axis=1)
    return m[np.lexsort(m.T[::-1])]


# ------------------------------------------------------------------------------------------------------------------ the judgement

def _call_reference(case: Case, call: Call, b: int, table, params, key, frozen: bool, step_fn=T.step) -> T.StepResult:
    n = call.rows if call.counts is None else int(call.counts[b])
    kw = dict(loss_scale=float(call.scale), noise_key=key, frozen=frozen)
    if call.points is not None:
        kw["points"] = np.ascontiguousarray(call.points[b, :n])
        if call.lod is not None:
            if case.fade is None:
                raise ValueError("a call with a level of detail needs Case.fade")
            per_point = isinstance(call.lod, np.ndarray)
            kw["lod"] = (case.fade, call.lod[:n] if per_point else None, 0.0 if per_point else float(call.lod))
    else:
        kw.update(origins=call.origins[b], extent=call.extent)
    return step_fn(case.geo, table, params, T.as_f64(call.target)[b, :n], **kw)


def _check_freeze(case: Case, before, got, out: dict, report: Report) -> torch.Tensor:
    """``got``, the table after ``freeze()``, equals fp32(quantiser(``before``)), ``before`` the table the last noisy step left, bit for
    bit - but for entries on a rounding boundary, which may be one code off.  ``got`` None: no freeze was recorded before this pass, and
    ``before`` (the pass's own table) is counted against its quantiser.  Returns the table the frozen passes are evaluated at: the recorded
    one where there is one."""
    lb = case.level_bits()
    want = quantise_levels(before, lb)
    if got is None:
        out["freeze | table bits"] = (float(_same_bits(before, want)), 0.0)
        return torch.from_numpy(want.numpy().astype(np.float32)).to(F64)
    diff = torch.from_numpy(_bits32(got) != _bits32(want))
    x = T.as_f64(before)
    ties = 0
    for l, b in enumerate(lb):
        s = float((1 << b) - 1)
        frac = x[..., l, :, :] * s + 0.5
        near = (frac - torch.round(frac)).abs() <= TIE
        d = diff[..., l, :, :]
        other = torch.floor(frac) + 1.0 - 2.0 * (torch.round(frac) == torch.floor(frac))      # the code on the other side of the boundary
        one_off = _bits32_t(got)[..., l, :, :] == _bits32_t(other / s)
        excused = d & near & one_off
        ties += int(excused.sum())
        diff[..., l, :, :] = d & ~excused
    report.ties += ties
    out["freeze | table bits"] = (float(diff.sum()), 0.0)
    return T.as_f64(got)


def _continuity(prev: State, pre: State, tables: bool) -> int:
    """entries of a pass's pre-state that are not the bits of the state the pass before left (``tables``: the tables too - not across a
    freeze, which rewrites them)"""
    bad = _same_bits(prev.tables, pre.tables) if tables else 0
    for a, b in zip(prev.params, pre.params):
        bad += _same_bits(a, b)
    pairs = list(zip(prev.decoder_moments, pre.decoder_moments))
    if prev.table_moments is not None and pre.table_moments is not None:
        pairs.append((prev.table_moments, pre.table_moments))
    elif (prev.table_moments is None) != (pre.table_moments is None):
        bad += 1
    for (m0, v0, s0), (m1, v1, s1) in pairs:
        bad += _same_bits(m0, m1) + _same_bits(v0, v1) + abs(int(s0) - int(s1))
    return bad


def _check_rows(case: Case, calls: List[Call], out: dict) -> None:
    """host layout: chunk sizes, and the rows of the pass as a multiset against the input set (or against the mip chain)"""
    if case.chunks is not None:
        out["layout | chunk sizes"] = (0.0 if [c.rows for c in calls] == list(case.chunks) else 1.0, 0.0)
    if case.rows is None and case.mips is None:
        return
    B = calls[0].points.shape[0]
    for b in range(B):
        def real(c):
            return c.rows if c.counts is None else int(c.counts[b])
        pts = np.concatenate([c.points[b, :real(c)] for c in calls])
        col = np.concatenate([T.as_f64(c.target)[b, :real(c)].numpy().astype(np.float32) for c in calls])
        per_point = isinstance(calls[0].lod, np.ndarray)
        lod = np.concatenate([c.lod[:real(c)] for c in calls]) if per_point else None
        if case.rows is not None:
            p0, t0, l0 = case.rows[b]
            got = _sorted_rows([pts, col] + ([lod] if lod is not None else []))
            want = _sorted_rows([p0, T.as_f64(t0).numpy(), ] + ([l0] if l0 is not None else []))
            bad = 1.0 if (lod is None) != (l0 is None) or got.shape != want.shape else float((got != want).any(axis=1).sum())
            out[f"layout | rows field {b}"] = (bad, 0.0)
        else:
            _check_mips(case, pts, col, lod, out)


def _check_mips(case: Case, pts, col, lod, out: dict) -> None:
    """every sample of every mip exactly once: p = (j + 1/2) 2^m - 1/2 exactly, lod = m exactly, the colour within 2^m dim 2^-24 of the
    float64 mean of its block of the target (values in [0, 1])"""
    target, mips = case.mips
    tgt = T.as_f64(target)
    size, dim = tuple(tgt.shape[:-1]), case.geo.dim
    bad, seen, worst = 0, 0, 0.0
    for m in range(int(mips) + 1):
        sz = tuple(s >> m for s in size)
        blocks = tgt.reshape(*[v for s in sz for v in (s, 1 << m)], 3)
        mean = blocks.mean(dim=tuple(range(1, 2 * dim, 2))).reshape(-1, 3).numpy()
        sel = np.nonzero(lod == np.float32(m))[0]
        j = (pts[sel].astype(np.float64) + 0.5) / float(1 << m) - 0.5
        ji = np.rint(j).astype(np.int64)
        exact = (((ji + 0.5) * float(1 << m) - 0.5).astype(np.float32) == pts[sel]).all(axis=1) & ((ji >= 0) & (ji < np.array(sz))).all(axis=1)
        flat = np.ravel_multi_index(tuple(np.clip(ji, 0, np.array(sz) - 1).T), sz)
        once = np.bincount(flat[exact], minlength=int(np.prod(sz)))
        bad += int((~exact).sum()) + int((once != 1).sum())
        seen += sel.shape[0]
        if exact.any():
            worst = max(worst, float(np.abs(col[sel][exact].astype(np.float64) - mean[flat[exact]]).max()) / ((1 << m) * dim * 2.0 ** -24))
    bad += pts.shape[0] - seen                                    # a level of detail that is no mip's
    out["layout | mip points and lod"] = (float(bad), 0.0)
    out["layout | mip colours"] = (worst, 1.0)


def verify(rec: Recording, case: Case, what: str = "fit", quiet: bool = False, step_fn=T.step) -> Report:
    """judge every pass of ``rec`` from its own recorded pre-state (module docstring).  Compared, per pass: every call's loss and the
    returned per-pass loss (relative, TOL_Y); the table-gradient buffer after a ``step=False`` call against the partial sum, per level over the
    level's largest magnitude (TOL_G); per tensor (a table level of a field, a decoder tensor of a field), with g the summed reference
    gradient, gmax its largest magnitude, c the 1-based count of the step and (p, m, v) the pre-state:

    - the parameter: ``step_bound(gmax, max |m|, lr, betas, eps, c, s0 = sqrt(b2 min v)) + ulp32(want)``, the clamp to the level's
      ``q_range`` on the reference side, no Lipschitz term where g is all zero;
    - ``exp_avg``: (1 - b1) TOL_G gmax + 3 ulp32(max(|m|, |g|, |m'|)) - three roundings in m + (g - m)(1 - b1);
    - ``exp_avg_sq``: (1 - b2)(2 gmax (1 + TOL_G) + TOL_G gmax) TOL_G gmax + 4 ulp32(max(v, (1 - b2) g^2, v'));
    - ``step`` = c, and the field's own ``steps`` = c - 1 before the pass, exactly.

    ``fresh`` (m = v = 0 before the first step): the update lr g / (|g| + eps) has no Lipschitz bound near g = 0, so the FIRST step's
    parameters are compared on entries with |g| >= 0.1 gmax only, bound lr eps / (0.1 gmax - TOL_G gmax + eps)^2 TOL_G gmax + 8 2^-24 lr +
    ulp32(p); entries the reference leaves at exactly zero keep their parameter and have m' = v' = 0 exactly; later passes compare
    everything but the parameters.

    The freeze: before pass ``freeze_epoch`` and not before, ``_check_freeze`` against the table BEFORE the freeze (recorded by the
    freeze wrapper, and asserted to be the table the last noisy step left); every pass's pre-state is the bits of the post-state before it
    (tables, decoder, moments, step counts; across the freeze all but the tables); afterwards the table and its Adam state keep their bits, no
    call carries noise, the decoder still meets its bound.  Exact checks are reported as (violations, 0).  ``step_fn``: ``T.step``, or a
    memoised form of it (the CPU tests evaluate the same pass many times)."""
    report = Report()
    lrs = learning_rates(len(rec.passes), case.base_lrs, case.schedule)
    b1, b2 = case.betas
    lb = case.level_bits()
    L = case.geo.levels
    frozen_tab = None
    for e, ps in enumerate(rec.passes):
        out: Dict[str, Tuple[float, float]] = {}
        floors: Dict[str, float] = {}
        B = ps.pre.tables.shape[0]
        frozen = e >= case.freeze_epoch
        c = case.k0 + e + 1
        out["count | field.steps"] = (abs(float(ps.steps - (c - 1))), 0.0)
        tab = T.as_f64(ps.pre.tables)
        if e > 0 and rec.passes[e - 1].post is not None:                     # what a step wrote back is what the next pass starts from
            out["continuity | pre-state is the last post-state"] = (float(_continuity(rec.passes[e - 1].post, ps.pre, ps.frozen_table is None)), 0.0)
        if e == case.freeze_epoch:
            if ps.frozen_table is None:
                tab = frozen_tab = _check_freeze(case, ps.pre.tables, None, out, report)
            else:
                # the table BEFORE the freeze: recorded by the freeze wrapper, and the bits the last noisy step left
                before = ps.unfrozen_table
                if before is None:
                    out["freeze | the table before the freeze is missing"] = (1.0, 0.0)
                    before = rec.passes[e - 1].post.tables if e > 0 else ps.pre.tables
                elif e > 0 and rec.passes[e - 1].post is not None:
                    out["freeze | quantises the table the last step left"] = (float(_same_bits(before, rec.passes[e - 1].post.tables)), 0.0)
                tab = frozen_tab = _check_freeze(case, before, ps.frozen_table, out, report)
                out["freeze | the pass starts from the frozen table"] = (float(_same_bits(ps.pre.tables, ps.frozen_table)), 0.0)
        else:
            if ps.frozen_table is not None:
                out["freeze | at another pass"] = (1.0, 0.0)
            if frozen:
                out["freeze | table keeps its bits (pre)"] = (float(_same_bits(ps.pre.tables, frozen_tab)), 0.0)
        # ---- the calls
        total = sum(cl.rows for cl in ps.calls)
        out["weights | scales sum to 1"] = (abs(sum(float(cl.scale) for cl in ps.calls) - 1.0), 1e-12)
        out["weights | share of the pass"] = (max(abs(float(cl.scale) - cl.rows / total) for cl in ps.calls), 1e-12)
        flags = [(cl.accumulate, cl.step) for cl in ps.calls]
        want_flags = [(k > 0, k == len(ps.calls) - 1) for k in range(len(ps.calls))]
        out["layout | accumulate and step flags"] = (0.0 if flags == want_flags else 1.0, 0.0)
        if ps.calls[0].points is not None:
            _check_rows(case, ps.calls, out)
        elif case.chunks is not None:
            out["layout | chunk sizes"] = (0.0 if [cl.rows for cl in ps.calls] == list(case.chunks) else 1.0, 0.0)
        g_t = [[torch.zeros(case.geo.table_size, case.geo.features, dtype=F64) for _ in range(L)] for _ in range(B)]
        g_d = [[torch.zeros_like(T.as_f64(p[b])) for p in ps.pre.params] for b in range(B)]
        loss_sum = [0.0] * B
        before = 0
        for k, cl in enumerate(ps.calls):
            key = None if frozen else (case.bits if isinstance(case.bits, int) else tuple(case.bits), case.seed, case.k0 + e, before)
            for b in range(B):
                r = _call_reference(case, cl, b, tab[b], [p[b] for p in ps.pre.params], key, frozen, step_fn)
                want = float(r.loss)
                out[f"loss | call {k} field {b}"] = (abs(float(cl.loss.reshape(-1)[b]) - want) / abs(want), TOL_Y)
                loss_sum[b] += want
                for i in range(6):
                    g_d[b][i] += r.decoder_grads[i]
                if not frozen:
                    for l in range(L):
                        g_t[b][l] += r.table_grad[l]
                    if not cl.step:
                        if cl.grad is None:
                            out[f"table gradient buffer | call {k} field {b} missing"] = (1.0, 0.0)
                        else:
                            for l in range(L):
                                out[f"table gradient buffer | call {k} field {b} level {l}"] = (relmax(cl.grad[b][l], g_t[b][l]), TOL_G)
            before += cl.rows
        if rec.returned is not None:
            for b in range(B):
                out[f"loss | returned field {b}"] = (abs(float(rec.returned[e][b]) - loss_sum[b]) / abs(loss_sum[b]), TOL_Y)
        # ---- the step
        lr_t, lr_d = lrs[e]
        post = ps.post
        if post is None:
            out["count | the pass took no step"] = (1.0, 0.0)
            report.passes.append(out)
            report.floor.append(floors)
            continue
        first_fresh = case.fresh and e == 0
        compare_p = not case.fresh or e == 0

        def tensor(name, p, g, mom, got_p, got_mom, lr, clamp):
            m, v, st = mom
            gmax, m_max = float(g.abs().max()), float(T.as_f64(m).abs().max())
            want, m1, v1 = T.adam_step(p, g, m, v, c, lr, case.betas, case.eps, clamp=clamp)
            out[f"count | step {name}"] = (abs(float(st - (c - 1))) + abs(float(got_mom[2] - c)), 0.0)
            gm, gv = T.as_f64(got_mom[0]), T.as_f64(got_mom[1])
            bm = (1 - b1) * TOL_G * gmax + 3 * ulp32(torch.maximum(torch.maximum(T.as_f64(m).abs(), g.abs()), m1.abs()))
            out[f"exp_avg | {name}"] = (float(((gm - m1).abs() / bm).max()), 1.0)
            bv = (1 - b2) * (2 * gmax * (1 + TOL_G) + TOL_G * gmax) * TOL_G * gmax + 4 * ulp32(torch.maximum(torch.maximum(T.as_f64(v), (1 - b2) * g * g), v1))
            out[f"exp_avg_sq | {name}"] = (float(((gv - v1).abs() / bv).max()), 1.0)
            gp = T.as_f64(got_p)
            if first_fresh:
                zero = g == 0
                moved = int((gp[zero] != T.as_f64(p)[zero]).sum()) + int((gm[zero] != 0).sum()) + int((gv[zero] != 0).sum())
                out[f"parameter | {name} untouched entries"] = (float(moved), 0.0)
                sel = g.abs() >= 0.1 * gmax
                report.share[name] = float(sel.sum()) / max(1, int((~zero).sum()))
                bound = lr * case.eps / (0.1 * gmax - TOL_G * gmax + case.eps) ** 2 * TOL_G * gmax + 8 * 2.0 ** -24 * lr + ulp32(p)
                out[f"parameter | {name}"] = (float(((gp - want).abs() / bound)[sel].max()), 1.0)
            elif compare_p:
                bound = ulp32(want)
                if gmax > 0:
                    v_min = float(T.as_f64(v).min())
                    floors[name] = math.sqrt(v_min) / gmax
                    bound = bound + step_bound(gmax, m_max, lr, case.betas, case.eps, c, math.sqrt(b2 * v_min))
                out[f"parameter | {name}"] = (float(((gp - want).abs() / bound).max()), 1.0)

        for b in range(B):
            tag = f"field {b} " if B > 1 else ""
            if not frozen:
                if ps.pre.table_moments is None or post.table_moments is None:
                    out[f"count | {tag}table state missing"] = (1.0, 0.0)
                else:
                    pm, pv, pst = ps.pre.table_moments
                    qm, qv, qst = post.table_moments
                    for l in range(L):
                        tensor(f"{tag}table[{l}]", tab[b][l], g_t[b][l], (pm[b][l], pv[b][l], pst), post.tables[b][l], (qm[b][l], qv[b][l], qst), lr_t, T.q_range(lb[l]))
            for i in range(6):
                pm, pv, pst = ps.pre.decoder_moments[i]
                qm, qv, qst = post.decoder_moments[i]
                tensor(f"{tag}{NAMES[i]}", ps.pre.params[i][b], g_d[b][i], (pm[b], pv[b], pst), post.params[i][b], (qm[b], qv[b], qst), lr_d, None)
        if frozen:
            out["freeze | table keeps its bits (post)"] = (float(_same_bits(post.tables, frozen_tab)), 0.0)
            if ps.pre.table_moments is not None and post.table_moments is not None:
                moved = _same_bits(ps.pre.table_moments[0], post.table_moments[0]) + _same_bits(ps.pre.table_moments[1], post.table_moments[1])
                out["freeze | table state untouched"] = (float(moved + abs(ps.pre.table_moments[2] - post.table_moments[2])), 0.0)
        report.passes.append(out)
        report.floor.append(floors)
        if not quiet:
            kinds: Dict[str, Tuple[float, float, float]] = {}
            for q, (err, bound) in out.items():
                kind = q.split(" | ")[0]
                if kind not in kinds or ratio(err, bound) > kinds[kind][0]:
                    kinds[kind] = (ratio(err, bound), err, bound)
            for kind, (r, err, bound) in kinds.items():
                print(f"MEASURED {what} | pass {e} | {kind} | {err:.3e} | {bound:.0e} | {r:.3f}")
            if floors:
                print(f"MEASURED {what} | pass {e} | floor sqrt(min v) / gmax | {min(floors.values()):.4f}")
    if not quiet:
        print(f"MEASURED {what} | entries one code off on a rounding boundary at the freeze | {report.ties}")
        if report.share:
            print(f"MEASURED {what} | smallest share of touched entries compared at step 1 | {min(report.share.values()):.3f}")
    return report
