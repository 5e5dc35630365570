"""Reference of one hash-grid TRAINING step in float64 (test infrastructure) - the sibling of ``oracle/hashgrid_ref.py`` for the
half of the field that writes parameters.

Plain CPU code in float64 (torch) and int64, written from the contract comments of ``include/nicv2_hip.h`` (``nic_hash_desc``,
``nic_hash_quant``, the "arbitrary points" section, ``nic_hash_level_bits``, ``nic_hash_lod``, and the training entries from
``nic_hash_fused_forward_backward`` down) and from nothing else: it imports nothing of ``neural_image_compression_v2_amd``.  From
``oracle/hashgrid_ref.py`` it takes ``entry_index``, ``fixed_point`` and ``level_resolutions``, from ``oracle/nic_oracle.py`` ``threefry4x32``.

The forward is written once; every gradient is ``torch.autograd``'s over that forward.  The table is read by index (``table[l][idx]``), so the
scatter is autograd's ``index_add``; no derivative formula is restated.  The two places where the header defines a derivative that the
forward's arithmetic does not have are written as straight-through values in the forward itself: the 1/256 rounding and the integer clamp of a
point's position (``position``: the value is the rounded one, the slope that of ``256 p + 128``), and the codec noise (added to the row, the
gradient passes through the sum).  The floating-point clamp of a point is ``torch.clamp``: an axis it moved carries no gradient.

The stages a wrong rule could live in are small module-level functions (``gather``, ``weigh``, ``add_noise``, ``gelu``, ``mse``, ``position``) so
that tests/test_hashgrid_train_ref_cpu.py can damage a COPY of this module one stage at a time and show that the comparison notices."""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from oracle import hashgrid_ref as R
from oracle.nic_oracle import threefry4x32

NOISE_TWEAK = 0x4E494332          # "NIC2", the third key word
F64 = torch.float64


@dataclass(frozen=True)
class Geometry:
    """what ``hashgrid_ref.entry_index`` reads of a file, without the file"""
    field_size: Tuple[int, ...]
    resolutions: Tuple[int, ...]
    features: int
    log2_table: int

    @property
    def dim(self) -> int:
        return len(self.field_size)

    @property
    def levels(self) -> int:
        return len(self.resolutions)

    @property
    def s_max(self) -> int:
        return max(self.field_size)

    @property
    def table_size(self) -> int:
        return 1 << self.log2_table

    @property
    def width(self) -> int:
        return self.levels * self.features


def geometry(field_size: Sequence[int], levels: int, features: int, log2_table: int, base_resolution: float) -> Geometry:
    """the finest level is max(field_size), like ``HashGridField``'s default"""
    fs = tuple(int(s) for s in field_size)
    return Geometry(fs, tuple(R.level_resolutions(levels, base_resolution, max(fs))), int(features), int(log2_table))


def level_dense(geo: Geometry, l: int) -> bool:
    return (geo.resolutions[l] + 1) ** geo.dim <= geo.table_size


# ------------------------------------------------------------------------------------------------------------------ positions

@dataclass
class Rows:
    """positions of N samples: ``t`` [N, dim] float64, the fixed-point coordinate (an integer value; with ``points`` it carries the slope of
    256 p + 128 back to them), ``points`` the float64 leaf the position gradient is taken at (None on the lattice)"""
    t: torch.Tensor
    points: Optional[torch.Tensor]


def position(tc: torch.Tensor, t_int: torch.Tensor) -> torch.Tensor:
    """the value of the rounded, clamped integer position ``t_int`` with the slope of the unrounded ``tc = 256 p + 128``: "the 1/256 rounding
    and the integer clamp of t are passed straight through".  tc, t_int and their difference are exact in float64."""
    return tc + (t_int - tc).detach()


def rows(geo: Geometry, origins=None, extent=None, points=None) -> Rows:
    """lattice crops (``origins`` [num_crops, dim] and ``extent``: crops back to back, the last axis fastest; sample i is the point
    t = 256 i + 128) or fp32 ``points`` [N, dim] (numpy float32 or a float32 tensor: clamped in floating point to [-1/2, S_a - 1/2] with NaN to
    the low edge, t = rint(256 p) + 128 clamped to [0, 256 S_a - 1])"""
    if (origins is None) == (points is None):
        raise ValueError("exactly one of origins / points")
    if origins is not None:
        org = np.asarray(origins, dtype=np.int64).reshape(-1, geo.dim)
        if len(extent) != geo.dim:
            raise ValueError(f"extent {tuple(extent)} for a {geo.dim}D field")
        local = np.stack([g.reshape(-1) for g in np.meshgrid(*[np.arange(int(e), dtype=np.int64) for e in extent], indexing="ij")], axis=1)
        i = (org[:, None, :] + local[None]).reshape(-1, geo.dim)
        if (i < 0).any() or (i >= np.array(geo.field_size)).any():
            raise ValueError("a crop leaves the field")
        return Rows(torch.from_numpy(256 * i + 128).to(F64), None)
    p32 = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
    t_int = torch.from_numpy(R.fixed_point(geo, p32)).to(F64)                  # checks fp32 [N, dim]
    clamped, moved = clamp_points(geo, p32)
    p = torch.from_numpy(p32.astype(np.float64)).requires_grad_(True)
    pc = torch.where(torch.from_numpy(moved), torch.from_numpy(clamped), p)     # a clamped axis is a constant: it carries no position gradient
    return Rows(position(256.0 * pc + 128.0, t_int), p)


def clamp_points(geo: Geometry, points_fp32: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(the points clamped in floating point to [-1/2, S_a - 1/2] as float64, NaN at the low edge; a bool [N, dim] of the axes the clamp
    moved: NaN, +-inf, p < -1/2, p > S_a - 1/2 - p = S_a - 1/2 itself is not clamped)"""
    p64 = np.asarray(points_fp32).astype(np.float64)
    clamped = np.where(np.isnan(p64), -0.5, p64)
    clamped = np.minimum(np.maximum(clamped, -0.5), np.array([s - 0.5 for s in geo.field_size])[None, :])
    return clamped, p64 != clamped


def level_weights(geo: Geometry, n: int, fade: Sequence[float], lod=None, lod_uniform: float = 0.0) -> np.ndarray:
    """a [N, L] float64 holding fp32 values: lambda = (lod[n] or 0) + lod_uniform in fp32, NaN -> 0, clamped to [0, 32];
    a_l = min(max((fade[l] - lambda) + 1, 0), 1) in fp32, in that order"""
    f32 = np.float32
    lam = (np.zeros(n, dtype=f32) if lod is None else np.asarray(lod, dtype=f32).reshape(n)) + f32(lod_uniform)
    lam = np.where(np.isnan(lam), f32(0), lam).astype(f32)
    lam = np.minimum(np.maximum(lam, f32(0)), f32(32))
    fd = np.asarray(fade, dtype=f32).reshape(1, geo.levels)
    a = ((fd - lam[:, None]).astype(f32) + f32(1)).astype(f32)
    return np.minimum(np.maximum(a, f32(0)), f32(1)).astype(np.float64)


def default_fade(geo: Geometry) -> Tuple[float, ...]:
    """max(0, log2(S_max / R_l)) in float64, rounded once to fp32"""
    return tuple(float(np.float32(max(0.0, math.log2(geo.s_max / r)))) for r in geo.resolutions)


# ------------------------------------------------------------------------------------------------------------------ noise

def noise(n: int, width: int, bits: Union[int, Sequence[int]], seed: int, offset: int, sample_base: int) -> np.ndarray:
    """[n, width] float64 (every value is exact in fp32 too).  Sample s = sample_base + row; column c is value c & 15 of block c >> 4:
    Threefry-4x32-12 of counter (s_lo, (c >> 4) + (s_hi << 8), offset_lo, offset_hi), key (seed_lo, seed_hi, "NIC2", 0); value i = byte i & 3
    of word i >> 2; u8 -> ((u8 + 1/2) / 256 - 1/2) 2^-b.  ``bits``: one depth, or one per level (then column l F + f takes b_l, F = width / L)."""
    m32 = np.uint64(0xFFFFFFFF)
    nblk = (width + 15) // 16
    s = np.arange(n, dtype=np.uint64) + np.uint64(sample_base)
    ctr = np.zeros((n, nblk, 4), dtype=np.uint32)
    ctr[..., 0] = (s & m32).astype(np.uint32)[:, None]
    ctr[..., 1] = np.arange(nblk, dtype=np.uint32)[None, :] + ((s >> np.uint64(32)).astype(np.uint32)[:, None] << np.uint32(8))
    ctr[..., 2] = np.uint32(int(offset) & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32((int(offset) >> 32) & 0xFFFFFFFF)
    r = threefry4x32(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, NOISE_TWEAK, 0), rounds=12)
    c = np.arange(width)
    i = c & 15
    words = r[:, c >> 4, i >> 2].astype(np.int64)
    u8 = (words >> (8 * (i & 3))[None, :]) & 255
    if isinstance(bits, (int, np.integer)):
        b = np.full(width, int(bits), dtype=np.int64)
    else:
        if width % len(bits):
            raise ValueError(f"{len(bits)} depths for {width} columns")
        b = np.repeat(np.asarray(bits, dtype=np.int64), width // len(bits))
    return ((u8.astype(np.float64) + 0.5) / 256.0 - 0.5) * np.ldexp(1.0, -b)[None, :]


# ------------------------------------------------------------------------------------------------------------------ the forward, by stage

def gather(table_l: torch.Tensor, idx: torch.Tensor, level: int, corner: Tuple[int, ...]) -> torch.Tensor:
    """[N, F]: the entries ``idx`` of one level's [T, F] table - autograd's backward of this read is the scatter"""
    return table_l[idx]


def weigh(a_l: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """a level's [N, F] columns times its per-point weight [N]"""
    return a_l[:, None] * r


def add_noise(r: torch.Tensor, nz: torch.Tensor) -> torch.Tensor:
    return r + nz


def gelu(z: torch.Tensor) -> torch.Tensor:
    """exact-erf GELU"""
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def mse(y: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """mean((y - target)^2) over the [N, 3] outputs"""
    return ((y - target) ** 2).sum() / (3 * y.shape[0])


def encode(geo: Geometry, tables: Sequence[torch.Tensor], pos: Rows, nz: Optional[torch.Tensor] = None,
           weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, L F]: per level q = t R_l, v = q div (256 S_max), w = (q mod 256 S_max) / (256 S_max); column l F + f = a_l (sum over the 2^dim
    corners c of prod_a (c_a ? w_a : 1 - w_a) table[l][idx(v + c), f] + noise)"""
    den = 256 * geo.s_max
    t_int = pos.t.detach().to(torch.int64)
    cols = []
    for l, r in enumerate(geo.resolutions):
        v = (t_int * r) // den                                                  # exact integers (< 2^38)
        w = (pos.t * float(r) - (v * den).to(F64)) / float(den)                 # = (q mod den) / den, with the slope R_l / (256 S_max) in t
        acc = torch.zeros(t_int.shape[0], geo.features, dtype=F64)
        for c in itertools.product((0, 1), repeat=geo.dim):
            idx = torch.from_numpy(R.entry_index(geo, l, v.numpy() + np.array(c, dtype=np.int64)))
            cw = torch.ones(t_int.shape[0], dtype=F64)
            for a in range(geo.dim):
                cw = cw * (w[:, a] if c[a] else 1.0 - w[:, a])
            acc = acc + cw[:, None] * gather(tables[l], idx, l, c)
        if nz is not None:
            acc = add_noise(acc, nz[:, l * geo.features:(l + 1) * geo.features])
        if weights is not None:
            acc = weigh(weights[:, l], acc)
        cols.append(acc)
    return torch.cat(cols, dim=1)


def decoder(x: torch.Tensor, params: Sequence[torch.Tensor]) -> torch.Tensor:
    """[N, 3]: Linear, GELU, .., Linear, sigmoid for ``params`` = W1, b1, W2, b2, .. (any hidden width, any number of layers)"""
    a = x
    n_linear = len(params) // 2
    for i in range(n_linear):
        z = a @ params[2 * i].T + params[2 * i + 1]
        a = gelu(z) if i < n_linear - 1 else torch.sigmoid(z)
    return a


# ------------------------------------------------------------------------------------------------------------------ the step

@dataclass
class StepResult:
    y: torch.Tensor                              # [N, 3]
    loss: torch.Tensor                           # scalar
    table_grad: Optional[List[torch.Tensor]]     # per level [T, F]; None with a frozen table
    decoder_grads: List[torch.Tensor]            # dW1, db1, ..
    dpoints: Optional[torch.Tensor]              # [N, dim] with points, else None
    row: torch.Tensor                            # [N, L F], the decoder's input


def as_f64(x) -> torch.Tensor:
    return (x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(F64)


def step(geo: Geometry, table, params, target, origins=None, extent=None, points=None, loss_scale: float = 1.0, noise_key=None, lod=None,
         frozen: bool = False) -> StepResult:
    """one forward + backward: y, loss = mean((y - target)^2) * loss_scale, d loss / d table per level, the decoder gradients, d loss / d points.
    ``table``: [L, T, F] (any float dtype; the values are taken as they are).  ``noise_key``: None or (bits, seed, offset, sample_base), ``bits``
    one depth or one per level.  ``lod``: None or (fade [L], lod per point [N] or None, lod_uniform).  ``frozen``: no table gradient."""
    tab = as_f64(table)
    tables = [tab[l].clone().requires_grad_(not frozen) for l in range(geo.levels)]
    ps = [as_f64(p).clone().requires_grad_(True) for p in params]
    tgt = as_f64(target)
    pos = rows(geo, origins, extent, points)
    n = pos.t.shape[0]
    if tuple(tgt.shape) != (n, 3):
        raise ValueError(f"target must be [{n}, 3], got {tuple(tgt.shape)}")
    nz = None if noise_key is None else torch.from_numpy(noise(n, geo.width, *noise_key))
    wt = None if lod is None else torch.from_numpy(level_weights(geo, n, lod[0], lod[1], lod[2]))
    row = encode(geo, tables, pos, nz, wt)
    y = decoder(row, ps)
    loss = mse(y, tgt) * float(loss_scale)
    leaves = ps + ([] if frozen else tables) + ([] if pos.points is None else [pos.points])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    k = len(ps)
    tg = None if frozen else list(grads[k:k + geo.levels])
    dp = None if pos.points is None else grads[-1]
    return StepResult(y.detach(), loss.detach(), tg, list(grads[:k]), dp, row.detach())


def q_range(bits: int) -> Tuple[float, float]:
    """the dense quantiser's range [-(2^b - 1) / 2^(b + 1), 1/2]"""
    return -((1 << bits) - 1) / float(1 << (bits + 1)), 0.5


def adam_step(param, grad, exp_avg, exp_avg_sq, step_count: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, clamp=None):
    """``torch.optim.Adam``'s update (no weight decay, no amsgrad) on float64 copies, ``step_count`` the 1-based count of THIS step; then the
    clamp to ``clamp`` = (lo, hi) where the field has a quantiser.  Returns (param, exp_avg, exp_avg_sq)."""
    p, g, m, v = as_f64(param).clone(), as_f64(grad), as_f64(exp_avg).clone(), as_f64(exp_avg_sq).clone()
    opt = torch.optim.Adam([p], lr=float(lr), betas=betas, eps=float(eps))
    p.grad = g.clone()
    opt.state[p] = {"step": torch.tensor(float(step_count - 1)), "exp_avg": m, "exp_avg_sq": v}
    opt.step()
    if clamp is not None:
        p.clamp_(float(clamp[0]), float(clamp[1]))
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]
