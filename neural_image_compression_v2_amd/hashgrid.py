"""Multi-resolution hash-grid field (Instant-NGP-style encoding; BASELINE config 2's "16-level (hash) grid").  No reference counterpart: the
reference reads dense G0 / G1 pairs only (fp_def.py), and so does ``MultiLevelField`` (multilevel.py).  The semantics are this project's own
(include/nicv2_hip.h, nic_hash_desc):

- a field covers integer sample coordinates i_a in [0, S_a) on d = 2 or 3 axes, S_max = max_a S_a;
- L levels of resolution R_l = floor(N_min b^l), b = exp((ln N_max - ln N_min) / (L - 1)) in float64 (``level_resolutions``), N_max = S_max by default;
- one fp32 table [L, T, F], T = 2^log2_table entries of F features per level;
- on axis a, q = (2 i_a + 1) R_l: base vertex v_a = floor(q / 2 S_max) (exact integer), weight w_a = (q mod 2 S_max) / 2 S_max (fp32);
- entry of vertex v: dense levels ((R_l + 1)^d <= T) v_x + (R_l + 1) (v_y + (R_l + 1) v_z), hashed ones (v_x * 1) ^ (v_y * 2654435761) ^
  (v_z * 805459861) in wrapping uint32, both & (T - 1);
- row n of the [N, L F] encoding holds at column l F + f the d-linear interpolation of the 2^d corner entries; samples in ``nic_encode`` order
  (crops back to back, the last axis fastest), so the targets of ``MultiLevelField`` serve unchanged.

The gather / interpolate (``nic_hash_encode``) and its gradient scatter (``nic_hash_encode_backward``) are the HIP kernels of csrc/hash_grid.hip;
the decoder is ``ColorDecoder`` on the general layer-wise kernels, the optimiser ``FusedAdam``.  No noise and no clamp: there is no quantiser
behind a hash table."""
from __future__ import annotations

import ctypes
import itertools
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib, fused
from .image_compression import ColorDecoder
from .optim import CosineAnnealing, FusedAdam


def level_resolutions(levels: int, n_min: float, n_max: float) -> List[int]:
    """R_l = floor(n_min * b^l), b = exp((ln n_max - ln n_min) / (levels - 1)), in float64 (one level: [floor(n_min)])"""
    if not 1 <= levels <= _lib.NIC_HASH_MAX_LEVELS:
        raise ValueError(f"1 .. {_lib.NIC_HASH_MAX_LEVELS} levels")
    if levels == 1:
        return [int(math.floor(n_min))]
    b = math.exp((math.log(n_max) - math.log(n_min)) / (levels - 1))
    return [int(math.floor(n_min * b ** l)) for l in range(levels)]


def level_is_dense(resolution: int, dim: int, log2_table: int) -> bool:
    """a level indexes its vertices densely when (R + 1)^dim of them fit the table, else through the hash"""
    return (int(resolution) + 1) ** dim <= (1 << log2_table)


@dataclass(frozen=True)
class HashGeometry:
    """what a hash-grid launch needs besides the crops: field size (S_x, S_y(, S_z)), per-level resolutions, features, table size"""
    field_size: Tuple[int, ...]
    resolutions: Tuple[int, ...]
    features: int = 2
    log2_table: int = 19

    def __post_init__(self):
        if len(self.field_size) not in (2, 3):
            raise ValueError("a hash-grid field is 2D or 3D")
        if any(int(s) < 1 for s in self.field_size):
            raise ValueError(f"field size {self.field_size}")
        if not 1 <= len(self.resolutions) <= _lib.NIC_HASH_MAX_LEVELS:
            raise ValueError(f"1 .. {_lib.NIC_HASH_MAX_LEVELS} levels")
        if self.features not in (1, 2, 4, 8):
            raise ValueError("1, 2, 4 or 8 features per entry")
        if not 10 <= self.log2_table <= 24:
            raise ValueError("log2_table in 10 .. 24")
        if any(int(r) < 1 or 2 * self.s_max * int(r) >= 2 ** 31 for r in self.resolutions):
            raise ValueError(f"resolutions {self.resolutions}: each >= 1 and 2 * S_max * R < 2^31")

    @property
    def dim(self) -> int:
        return len(self.field_size)

    @property
    def levels(self) -> int:
        return len(self.resolutions)

    @property
    def s_max(self) -> int:
        return max(int(s) for s in self.field_size)

    @property
    def table_size(self) -> int:
        return 1 << self.log2_table

    @property
    def width(self) -> int:
        """columns of the encoding: L F"""
        return self.levels * self.features

    def table_shape(self) -> Tuple[int, int, int]:
        return (self.levels, self.table_size, self.features)

    def to_desc(self, num_crops: int, extent: Sequence[int]) -> "_lib.NicHashDesc":
        d = _lib.NicHashDesc()
        d.dim, d.levels, d.features, d.log2_table, d.S_max, d.num_crops = self.dim, self.levels, self.features, self.log2_table, self.s_max, int(num_crops)
        for a in range(3):
            d.extent[a] = int(extent[a]) if a < self.dim else 1
        for l, r in enumerate(self.resolutions):
            d.resolution[l] = int(r)
        return d

    def check_crops(self, coord, extent: Sequence[int]) -> torch.Tensor:
        """host origins [num_crops, dim] as int64, every crop inside the field (the kernel clamps for memory safety only)"""
        if len(extent) != self.dim or any(int(e) < 1 for e in extent):
            raise ValueError(f"extent {tuple(extent)} for a {self.dim}D field")
        o = torch.as_tensor(coord).reshape(-1, self.dim).to(torch.int64)
        if o.shape[0] < 1:
            raise ValueError("no crops")
        for a in range(self.dim):
            if bool((o[:, a] < 0).any()) or int(o[:, a].max()) + int(extent[a]) > int(self.field_size[a]):
                raise IndexError(f"axis {a}: crops of extent {int(extent[a])} at origins {o[:, a].tolist()} leave the field of {self.field_size[a]} samples")
        return o

    def upload_origins(self, coord, extent: Sequence[int], device) -> torch.Tensor:
        """int32 [num_crops, dim] on the device; host origins are validated first, a device tensor is taken as is (validating it would sync)"""
        if isinstance(coord, torch.Tensor) and coord.is_cuda:
            return coord.reshape(-1, self.dim).to(torch.int32).contiguous()
        return self.check_crops(coord, extent).to(torch.int32).to(device, non_blocking=True)


def _check_table(geo: HashGeometry, table: torch.Tensor, name: str = "table") -> torch.Tensor:
    t = _lib.require_cuda_f32(table, name)
    if tuple(t.shape) != geo.table_shape():
        raise ValueError(f"{name} must be {geo.table_shape()} = [levels, 2^log2_table, features], got {tuple(t.shape)}")
    return t


def _n_samples(num_crops: int, extent: Sequence[int]) -> int:
    n = int(num_crops)
    for e in extent:
        n *= int(e)
    return n


@fused._on_tensor_device
def hash_encode(geo: HashGeometry, table: torch.Tensor, coord, extent: Sequence[int]) -> torch.Tensor:
    """[N, L F] encoding of the crops at ``coord`` ([num_crops, dim] origins) of ``extent`` samples per axis (nic_hash_encode)"""
    t = _check_table(geo, table.detach())
    org = geo.upload_origins(coord, extent, t.device)
    num_crops = org.shape[0]
    out = torch.empty(_n_samples(num_crops, extent), geo.width, dtype=torch.float32, device=t.device)
    d = geo.to_desc(num_crops, extent)
    _lib.check(_lib.load().nic_hash_encode(ctypes.byref(d), _lib.ptr(t), _lib.ptr(org), _lib.ptr(out), _lib.stream_ptr(t.device)), "nic_hash_encode")
    return out


@fused._on_tensor_device
def hash_encode_backward(geo: HashGeometry, org: torch.Tensor, extent: Sequence[int], dx: torch.Tensor, table_grad: torch.Tensor) -> None:
    """ADDS d loss / d table for the [N, L F] gradient ``dx`` of the encoding into ``table_grad`` (nic_hash_encode_backward; fp32 atomics)"""
    g = _check_table(geo, table_grad, "table_grad")
    if g is not table_grad:
        raise ValueError("table_grad must be contiguous: the kernel adds into it in place")
    dx = _lib.require_cuda_f32(dx, "dx")
    num_crops = org.shape[0]
    if tuple(dx.shape) != (_n_samples(num_crops, extent), geo.width):
        raise ValueError(f"dx must be [{_n_samples(num_crops, extent)}, {geo.width}], got {tuple(dx.shape)}")
    d = geo.to_desc(num_crops, extent)
    _lib.check(_lib.load().nic_hash_encode_backward(ctypes.byref(d), _lib.ptr(org), _lib.ptr(dx), _lib.ptr(g), _lib.stream_ptr(g.device)),
               "nic_hash_encode_backward")


class HashEncodeFunction(torch.autograd.Function):
    """``hash_encode`` as a differentiable op of the table: backward = ``nic_hash_encode_backward`` into a fresh zero [L, T, F] (what autograd
    through ``index_add`` of the corner entries would give, collisions summed)"""

    @staticmethod
    def forward(ctx, table, geo: HashGeometry, org: torch.Tensor, extent):
        ctx.geo, ctx.org, ctx.extent = geo, org, tuple(int(e) for e in extent)
        return hash_encode(geo, table, org, extent)

    @staticmethod
    def backward(ctx, dx):
        g = torch.zeros(ctx.geo.table_shape(), dtype=torch.float32, device=dx.device)
        hash_encode_backward(ctx.geo, ctx.org, ctx.extent, dx, g)
        return g, None, None, None


def hash_encode_differentiable(geo: HashGeometry, table: torch.Tensor, coord, extent: Sequence[int]) -> torch.Tensor:
    org = geo.upload_origins(coord, extent, table.device)
    if not table.requires_grad:
        return hash_encode(geo, table, org, extent)
    return HashEncodeFunction.apply(table, geo, org, tuple(int(e) for e in extent))


class HashGridField:
    """a hash-grid table + one decoder over its [N, L F] encoding, trained like ``MultiLevelField`` (module docstring).  ``field_size``:
    (S_x, S_y) or (S_x, S_y, S_z), x = the image tensor's first spatial axis like everywhere in this package."""

    def __init__(self, field_size: Union[int, Sequence[int]], levels: int = 16, features: int = 2, log2_table: int = 19, base_resolution: float = 16,
                 finest_resolution: Optional[float] = None, hidden: int = 64, n_linear: int = 3, device=None, seed: Optional[int] = None):
        self.field_size = (int(field_size),) * 2 if isinstance(field_size, int) else tuple(int(v) for v in field_size)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("HashGridField needs a HIP device: there is no CPU implementation of this path")
        n_max = max(self.field_size) if finest_resolution is None else finest_resolution
        self.geo = HashGeometry(self.field_size, tuple(level_resolutions(levels, base_resolution, n_max)), features, log2_table)
        if seed is not None:
            torch.manual_seed(seed)
        self.table = torch.empty(self.geo.table_shape(), dtype=torch.float32, device=self.device).uniform_(-1e-4, 1e-4).requires_grad_(True)
        self.decoder = ColorDecoder(self.geo.width, hidden, n_linear).to(self.device)
        self.optimizer = FusedAdam([{"params": [self.table], "lr": 0.01}, {"params": self.decoder.parameters(), "lr": 0.005}])
        # the table gradient persists: the optimiser launch zeroes it after reading it, so a step needs no fill launch
        self.table.grad = torch.zeros_like(self.table)
        self.optimizer.zero_grad_in_step([self.table])
        self._grad_clean = True
        self.scheduler = None

    @property
    def resolutions(self) -> Tuple[int, ...]:
        return self.geo.resolutions

    def set_schedule(self, num_epochs: int) -> None:
        self.scheduler = CosineAnnealing(self.optimizer, T_max=num_epochs, eta_min=0)

    def encode(self, coord, extent: Sequence[int]) -> torch.Tensor:
        """[N, L F], differentiable w.r.t. the table"""
        return hash_encode_differentiable(self.geo, self.table, coord, extent)

    def forward(self, coord, extent: Sequence[int]) -> torch.Tensor:
        return self.decoder(self.encode(coord, extent))

    def train_step(self, coord, extent: Sequence[int], target: torch.Tensor, accumulate: bool = False, scale: float = 1.0, step: bool = True) -> torch.Tensor:
        """one step on the crops at ``coord`` with targets [N, 3].  ``accumulate`` / ``scale`` / ``step``: a whole-field pass walked in chunks -
        gradients add up over the chunks (each chunk's MSE scaled by its share), one optimiser step at the end"""
        params = self.decoder.linear_params()
        grad = self.table.grad
        if not accumulate:
            for p in params:
                p.grad = None
            if not self._grad_clean:
                grad.zero_()
        org = self.geo.upload_origins(coord, extent, self.device)
        if tuple(target.shape) != (_n_samples(org.shape[0], extent), 3):
            raise ValueError(f"target must be [{_n_samples(org.shape[0], extent)}, 3], got {tuple(target.shape)}")
        x = hash_encode(self.geo, self.table, org, extent).requires_grad_(True)
        y = fused.DecoderFunction.apply(x, *params)
        loss = ((y - target) ** 2).mean() * scale
        loss.backward()
        hash_encode_backward(self.geo, org, extent, x.grad, grad)
        self._grad_clean = False
        if step:
            self.optimizer.step()
            self._grad_clean = self.optimizer.zeroed_in_last_step(grad)
            if self.scheduler is not None:
                self.scheduler.step()
        return loss.detach()

    @torch.no_grad()
    def decode(self, tile: int = 1024) -> torch.Tensor:
        """the whole field [S_x, S_y(, S_z), 3], in tiles of side <= ``tile``"""
        size = self.field_size
        out = torch.empty(*size, 3, dtype=torch.float32, device=self.device)
        params = [p.detach() for p in self.decoder.linear_params()]
        table = self.table.detach()
        for o in itertools.product(*[range(0, s, tile) for s in size]):
            ext = [min(tile, s - a) for s, a in zip(size, o)]
            x = hash_encode(self.geo, table, [o], ext)
            sl = tuple(slice(a, a + e) for a, e in zip(o, ext))
            out[sl] = fused.DecoderFunction.apply(x, *params).reshape(*ext, 3)
        return out
