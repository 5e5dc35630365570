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
the decoder is ``ColorDecoder`` on the general layer-wise kernels, the optimiser ``FusedAdam``.  Without ``num_bits`` there is no noise and no
clamp.

The codec (``HashGridField(..., num_bits=b)``; include/nicv2_hip.h, nic_hash_quant) is the dense G0 / G1 codec's, carried over:
the optimiser clamps the table to the quantiser's range [-(2^b - 1) / 2^(b+1), 1/2]; training adds uniform noise of one quantisation step 2^-b to
every column of the encoding (``nic_hash_encode_noisy``: in-kernel Threefry keyed by (seed, optimiser step, sample id), straight-through backward);
``freeze()`` quantises the table in place and only the decoder trains on; ``save_compressed`` stores the compact uint8 table (``nic_hash_pack_u8``:
a dense level keeps only the (R + 1)^d vertices it can address) with the decoder, and ``load_compressed(...).decode()`` decodes straight from
those bytes (``nic_hash_encode_u8``).  The schedule is the dense one (image_compression.py:237,385): noise while the epoch is below 0.95 N, then
freeze - ``fit`` runs it.

``save_compressed(path, packed=True)`` stores the table bit-packed instead, b bits per value (``nic_hash_pack_bits``; format tag
``nicv2-hashgrid-bits/1``, layout in include/nicv2_hip.h); ``load_compressed`` reads either form and ``decode()`` of a packed field gathers from
the packed bits (``nic_hash_encode_bits`` / ``nic_hash_fused_forward_bits``) without ever unpacking the table.

``HashGridField(..., fused=True)`` runs the same step as TWO launches: one kernel gathers, decodes, forms the loss, back-propagates
and scatters (``nic_hash_fused_forward_backward``; the [N, L F] row never reaches memory), the reduction of its decoder-gradient records carries
the optimiser.  ``decode`` is one launch per tile.  Shapes outside the kernel's set (``nic_hash_fused_supported``) take the layer-wise route by
themselves; ``field.route`` says which one runs.

A bit depth per level (include/nicv2_hip.h, nic_hash_level_bits; csrc/hash_mixed.hip): ``HashGridField(..., num_bits=[b_0, ..,
b_{L-1}])`` applies the codec per level with b = b_l - level l is clamped to its own range (the optimiser clamps to the widest one,
``nic_hash_clamp_levels`` tightens the rest after each step), its columns take noise of scale 2^-b_l, ``freeze()`` quantises it with b_l, and
``save_compressed(path, packed=True)`` stores format ``nicv2-hashgrid-bits/2``: format /1 with b_l bits per value inside level l.  ``decode`` /
``query`` / ``resample`` of a loaded mixed field read those bits through ``nic_hash_encode_levels`` / ``nic_hash_fused_forward_levels``.  A
sequence always takes this path (equal depths give the uniform rows bit for bit); an int ``num_bits`` makes the calls it always made.

Off the lattice (include/nicv2_hip.h, nic_hash_encode_points): a point is ``dim`` fp32 coordinates in sample units, p_a = i the
centre of sample i, the field spanning [-1/2, S_a - 1/2]; t_a = rint(256 p_a) + 128 clamped to [0, 256 S_a - 1], q = t_a R_l, v_a = q div
256 S_max, w_a = fp32(q mod 256 S_max) / fp32(256 S_max) - at a sample centre the lattice row, bit for bit.  ``hash_encode_points`` /
``hash_encode_points_backward`` / ``hash_fused_forward_points`` (csrc/hash_points.hip) take a [N, dim] device tensor in any order;
``HashGridField.query`` decodes at points from whichever table the field holds, ``resample`` on a regular grid of any size, ``train_points``
is ``train_step`` on (point, colour) samples.

Training at points, cell-ordered and fused (csrc/hash_points_train.hip): ``hash_point_keys`` gives one Morton key per point from its
clamped fixed-point position, ``hash_point_order`` the int32 permutation that sorts them (a stable device sort); a launch that walks the points in
that order sums the neighbouring lanes of one cell before the gradient atomics, which random batches otherwise lose.
``train_points(..., order="cell" | tensor, fused=True)`` opt into the ordered scatter (``nic_hash_encode_points_backward_ordered``) and the fused
step at points (``nic_hash_fused_forward_backward_points``: two launches, the optimiser on the reduction); the defaults are the layer-wise,
unordered call unchanged.  ``fit_points`` fits a fixed (point, colour) set: the order is computed once, every epoch walks it in compact chunks.

A level of detail per point (include/nicv2_hip.h, nic_hash_lod; csrc/hash_points.hip, hash_points_train.hip): lambda = (lod[n] or 0) + lod_uniform, NaN ->
0, clamped to [0, 32]; level l is weighed by a_l = min(max((fade[l] - lambda) + 1, 0), 1) before the decoder, ``hash_lod_fade`` gives the
default fade start max(0, log2(S_max / R_l)), ``HashGridField(..., lod_fade=)`` another.  A level of weight 0 is not gathered, takes no noise
and no gradient; at weight 1 the columns are the plain route's bit for bit.  ``query`` / ``train_points`` / ``fit_points`` take ``lod=`` (a
float, or one value per point; None makes the launches made before), ``resample(size, lod="auto")`` derives it from the size,
``decode_mip(m)`` decodes mip m and ``fit_mips`` fits the box-filtered mip chain with one table and one decoder.

The decoder on the 16-bit matrix pipe (include/nicv2_hip.h, nic_hash_fused_forward_p16; csrc/hashgrid_fused16.hip): ``decode`` /
``query`` / ``resample`` take ``precision="split" | "bf16"`` - the same gather, the three Linear layers' products in split-bf16 (hi hi + hi lo +
lo hi) or plain bf16 operands with fp32 accumulation, bias, GELU and sigmoid in fp32.  ``None`` makes the launches made before.  Forward only, no
level of detail, no bit depth per level.

Gradients with respect to the point coordinates (include/nicv2_hip.h, nic_hash_encode_points_grad; csrc/hashgrid_pointgrad.hip):
d w_a / d p_a = R_l / S_max, so the derivative of a level is the signed-weight sum over its corners - the derivative of the multilinear
interpolant at the rounded position, 0 on an axis where the point lies outside the field.  ``hash_encode_points_grad`` turns a row gradient
into a position gradient, ``hash_fused_points_grad`` does gather, decoder, its backward to the row and the position gradient in one launch;
``HashGridField.point_gradient`` / ``jacobian`` / ``query_differentiable`` are the surface.  The field's parameters are constants there.

Gradients with respect to the level of detail (include/nicv2_hip_ext.h, nic_hash_encode_points_grad_lod; csrc/hashgrid_lodgrad.hip):
column l F + f is a_l r[l, f] with a_l = clamp((fade[l] - lambda) + 1, 0, 1), so dlod[n] = - sum over the levels on the ramp 0 < a_raw <= 1 of
sum_f g[n, l F + f] r[n, l, f] - the right-hand derivative, one more accumulator on the position gradient's walk, exactly 0 where lambda itself
is clamped.  ``hash_encode_points_grad_lod`` / ``hash_fused_points_grad_lod`` return it next to dpoints; ``HashGridField.point_gradient_lod`` /
``jacobian_lod`` / ``query_differentiable_lod`` are the surface.  From the training step (csrc/hashgrid_lodtrain.hip) the row
carries the codec noise inside the weighed column, a_l (r + nz), and the slope counts it: ``hash_fused_forward_backward_points_grad_lod`` /
``hash_encode_points_grad_lod_noisy``, ``HashGridField.train_points_grad_lod`` / ``train_points_differentiable_lod``.

B fields per launch (include/nicv2_hip.h, nic_hash_batch_forward_backward; csrc/hashgrid_batch.hip): ``HashGridFieldBatch`` holds
the stacked tables [B, L, T, F] and decoder tensors of B fields of one geometry; a workgroup of the batched kernel belongs to one field, a step is
three launches whatever B is (the kernel, the reduction per field, one ``FusedAdam`` over the stacked tensors), ``decode`` one per tile.
``hash_batch_forward`` / ``hash_batch_forward_backward`` are the functional forms; ``extract(b)`` / ``insert(b, field)`` move single fields out and in.
The decoder side (nic_hash_batch_forward_source): ``HashGridFieldBatch.load_compressed(paths)`` stacks the uint8 or bit-packed tables of
B stored files, ``decode`` / ``query`` / ``resample`` read whatever table a batch holds in one launch per tile for all fields;
``hash_batch_forward_source`` is the functional form (fp32, uint8 or packed tables; crops or points).
Training at points (include/nicv2_hip_ext.h, nic_hash_batch_forward_backward_points): ``HashGridFieldBatch.train_points`` /
``fit_points`` train every field at its own (point, colour) samples with a count per field, ``hash_batch_forward_backward_points`` and
``hash_batch_point_order`` are the functional forms."""
from __future__ import annotations

import ctypes
import functools
import itertools
import math
import numbers
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _lib, fused, models
from .fused import DecoderFunction
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


def _quant_struct(quant) -> Optional["_lib.NicHashQuant"]:
    """``nic_hash_quant`` of a (num_bits, seed, offset, sample_base) tuple - the kernel's own noise keyed by sample_base + row - or None"""
    if quant is None:
        return None
    bits, seed, offset, base = quant
    return _lib.NicHashQuant(int(bits), _lib.NIC_NOISE_KERNEL, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(base))


def _check_grads(geo: HashGeometry, table_grad: Optional[torch.Tensor], mlp_grads=None, params=None) -> None:
    """the buffers a training kernel writes: ``table_grad`` an fp32 [L, T, F] device table it can add into in place; with ``params``, ``mlp_grads``
    six buffers shaped like them, and ``table_grad`` may be None (a frozen table)"""
    if (table_grad is not None or params is None) and _check_table(geo, table_grad, "table_grad") is not table_grad:
        raise ValueError("table_grad must be contiguous: the kernel adds into it in place")
    if params is not None and (len(mlp_grads) != 6 or any(not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.shape == q.shape)
                                                            for g, q in zip(mlp_grads, params))):
        raise ValueError("mlp_grads: six contiguous fp32 device buffers shaped like the decoder's parameters")


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
    _check_grads(geo, table_grad)
    dx = _lib.require_cuda_f32(dx, "dx")
    num_crops = org.shape[0]
    if tuple(dx.shape) != (_n_samples(num_crops, extent), geo.width):
        raise ValueError(f"dx must be [{_n_samples(num_crops, extent)}, {geo.width}], got {tuple(dx.shape)}")
    d = geo.to_desc(num_crops, extent)
    _lib.check(_lib.load().nic_hash_encode_backward(ctypes.byref(d), _lib.ptr(org), _lib.ptr(dx), _lib.ptr(table_grad),
                                                    _lib.stream_ptr(table_grad.device)), "nic_hash_encode_backward")


@fused._on_tensor_device
def hash_encode_noisy(geo: HashGeometry, table: torch.Tensor, coord, extent: Sequence[int], num_bits: int, seed: int, offset: int,
                      sample_base: int = 0) -> torch.Tensor:
    """``hash_encode`` + uniform noise of one quantisation step 2^-num_bits on every column (nic_hash_encode_noisy): sample id = sample_base +
    row, keyed by (seed, offset).  The gradient w.r.t. the table is ``hash_encode_backward``'s (straight-through)."""
    t = _check_table(geo, table.detach())
    org = geo.upload_origins(coord, extent, t.device)
    num_crops = org.shape[0]
    out = torch.empty(_n_samples(num_crops, extent), geo.width, dtype=torch.float32, device=t.device)
    d = geo.to_desc(num_crops, extent)
    q = _quant_struct((num_bits, seed, offset, sample_base))
    _lib.check(_lib.load().nic_hash_encode_noisy(ctypes.byref(d), ctypes.byref(q), _lib.ptr(t), _lib.ptr(org), _lib.ptr(out), _lib.stream_ptr(t.device)),
               "nic_hash_encode_noisy")
    return out


def hash_stored_bytes(geo: HashGeometry) -> int:
    """bytes of the compact uint8 table: F * sum_l min((R_l + 1)^d, T) (nic_hash_stored_bytes)"""
    n = _lib.load().nic_hash_stored_bytes(ctypes.byref(geo.to_desc(1, [1] * geo.dim)))
    _lib.check(n if n < 0 else 0, "nic_hash_stored_bytes")
    return int(n)


@fused._on_tensor_device
def hash_pack_u8(geo: HashGeometry, table: torch.Tensor, num_bits: int) -> torch.Tensor:
    """the compact uint8 table of an fp32 [L, T, F] one, save4fp's arithmetic per value (nic_hash_pack_u8).  Clamp first: a value outside the
    quantiser's range wraps in the uint8 cast."""
    t = _check_table(geo, table.detach())
    out = torch.empty(hash_stored_bytes(geo), dtype=torch.uint8, device=t.device)
    _lib.check(_lib.load().nic_hash_pack_u8(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), int(num_bits), _lib.ptr(t), _lib.ptr(out), _lib.stream_ptr(t.device)),
               "nic_hash_pack_u8")
    return out


@fused._on_tensor_device
def hash_encode_u8(geo: HashGeometry, stored: torch.Tensor, coord, extent: Sequence[int], num_bits: int) -> torch.Tensor:
    """``hash_encode`` of the table a compact uint8 one stores (nic_hash_encode_u8): bit for bit ``hash_encode(load4fp(save4fp(table)))``"""
    if stored.dtype != torch.uint8 or not stored.is_cuda or stored.dim() != 1 or not stored.is_contiguous():
        raise ValueError("stored must be a contiguous 1-D uint8 tensor on a HIP device")
    if stored.numel() != hash_stored_bytes(geo):
        raise ValueError(f"stored holds {stored.numel()} bytes, the geometry needs {hash_stored_bytes(geo)}")
    org = geo.upload_origins(coord, extent, stored.device)
    num_crops = org.shape[0]
    out = torch.empty(_n_samples(num_crops, extent), geo.width, dtype=torch.float32, device=stored.device)
    d = geo.to_desc(num_crops, extent)
    _lib.check(_lib.load().nic_hash_encode_u8(ctypes.byref(d), int(num_bits), _lib.ptr(stored), _lib.ptr(org), _lib.ptr(out), _lib.stream_ptr(stored.device)),
               "nic_hash_encode_u8")
    return out


def _check_level_bits(levels: int, bits) -> Tuple[int, ...]:
    """a bit depth per level: a sequence of ``levels`` ints in 1 .. 8, as a tuple (anything else: ValueError)"""
    if isinstance(bits, (str, bytes)) or not hasattr(bits, "__len__") or not hasattr(bits, "__iter__"):
        raise ValueError(f"a bit depth per level is a sequence of {levels} ints in 1 .. 8, got {bits!r}")
    out = []
    for b in bits:
        if isinstance(b, bool) or not isinstance(b, int) and not (hasattr(b, "__index__")):
            raise ValueError(f"a bit depth per level is a sequence of ints in 1 .. 8, got {b!r}")
        out.append(int(b))
    if len(out) != int(levels):
        raise ValueError(f"{len(out)} bit depths for {levels} levels")
    if any(not 1 <= b <= 8 for b in out):
        raise ValueError(f"bit depths {out}: each in 1 .. 8")
    return tuple(out)


def _level_bits_struct(geo: HashGeometry, bits) -> "_lib.NicHashLevelBits":
    lb = _lib.NicHashLevelBits()
    for l, b in enumerate(_check_level_bits(geo.levels, bits)):
        lb.bits[l] = b
    return lb


def _is_level_bits(bits) -> bool:
    return bits is not None and not isinstance(bits, (str, bytes)) and hasattr(bits, "__len__")


def hash_packed_bytes(geo: HashGeometry, num_bits) -> int:
    """bytes of the bit-packed table: 4 * sum_l ceil(E_l F b / 32) + 8 (nic_hash_packed_bytes); ``num_bits`` a sequence: a depth per level,
    format /2 (nic_hash_packed_bytes_levels)"""
    if _is_level_bits(num_bits):
        n = _lib.load().nic_hash_packed_bytes_levels(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), ctypes.byref(_level_bits_struct(geo, num_bits)))
        _lib.check(n if n < 0 else 0, "nic_hash_packed_bytes_levels")
        return int(n)
    n = _lib.load().nic_hash_packed_bytes(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), int(num_bits))
    _lib.check(n if n < 0 else 0, "nic_hash_packed_bytes")
    return int(n)


def _check_packed(geo: HashGeometry, packed: torch.Tensor, num_bits: int) -> None:
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or not packed.is_cuda or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("packed must be a contiguous 1-D uint8 tensor on a HIP device")
    if packed.numel() != hash_packed_bytes(geo, num_bits):
        raise ValueError(f"packed holds {packed.numel()} bytes, the geometry needs {hash_packed_bytes(geo, num_bits)} at {num_bits} bits")
    if packed.data_ptr() % 4:
        raise ValueError("packed must start on a 4-byte boundary: the gather reads aligned dwords")


@fused._on_tensor_device
def hash_pack_bits(geo: HashGeometry, table: torch.Tensor, num_bits: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the bit-packed table of an fp32 [L, T, F] one (nic_hash_pack_bits): ``hash_pack_u8``'s value & (2^b - 1) in b bits, each level's stream
    padded to whole dwords, 8 zero bytes at the end.  ``out``: a buffer of ``hash_packed_bytes`` to fill (every byte is written)."""
    t = _check_table(geo, table.detach())
    if out is None:
        out = torch.empty(hash_packed_bytes(geo, num_bits), dtype=torch.uint8, device=t.device)
    _check_packed(geo, out, num_bits)
    _lib.check(_lib.load().nic_hash_pack_bits(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), int(num_bits), _lib.ptr(t), _lib.ptr(out), _lib.stream_ptr(t.device)),
               "nic_hash_pack_bits")
    return out


@fused._on_tensor_device
def hash_unpack_bits(geo: HashGeometry, packed: torch.Tensor, num_bits: int) -> torch.Tensor:
    """the compact uint8 table (``hash_pack_u8``'s layout) a bit-packed one stores (nic_hash_unpack_bits)"""
    _check_packed(geo, packed, num_bits)
    out = torch.empty(hash_stored_bytes(geo), dtype=torch.uint8, device=packed.device)
    _lib.check(_lib.load().nic_hash_unpack_bits(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), int(num_bits), _lib.ptr(packed), _lib.ptr(out),
                                                _lib.stream_ptr(packed.device)), "nic_hash_unpack_bits")
    return out


@fused._on_tensor_device
def hash_encode_bits(geo: HashGeometry, packed: torch.Tensor, coord, extent: Sequence[int], num_bits: int) -> torch.Tensor:
    """``hash_encode_u8`` from the bit-packed table (nic_hash_encode_bits): the same rows, bit for bit"""
    _check_packed(geo, packed, num_bits)
    org = geo.upload_origins(coord, extent, packed.device)
    num_crops = org.shape[0]
    out = torch.empty(_n_samples(num_crops, extent), geo.width, dtype=torch.float32, device=packed.device)
    d = geo.to_desc(num_crops, extent)
    _lib.check(_lib.load().nic_hash_encode_bits(ctypes.byref(d), int(num_bits), _lib.ptr(packed), _lib.ptr(org), _lib.ptr(out), _lib.stream_ptr(packed.device)),
               "nic_hash_encode_bits")
    return out


def hash_fused_supported(geo: HashGeometry, hidden: int = 64, n_linear: int = 3) -> bool:
    """whether the fused encode + decoder kernels exist for this geometry and decoder (nic_hash_fused_supported: the only copy of the set)"""
    return _lib.load().nic_hash_fused_supported(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), int(hidden), int(n_linear)) == 0


def _check_fused_decoder(geo: HashGeometry, params: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    if len(params) != 6:
        raise _lib.Unsupported("the fused hash-grid kernels decode with 3 Linear layers")
    params = fused.check_mlp(params, geo.width, params[0].shape[0])
    if params[0].shape[0] != 64:
        raise _lib.Unsupported("the fused hash-grid kernels decode with 64 hidden units")
    return params


@fused._on_tensor_device
def hash_fused_forward(geo: HashGeometry, table: torch.Tensor, coord, extent: Sequence[int], params: Sequence[torch.Tensor],
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, 3] = ColorDecoder(hash_encode(table)) in one launch (nic_hash_fused_forward); ``params`` = W1, b1, W2, b2, W3, b3"""
    t = _check_table(geo, table.detach())
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    org = geo.upload_origins(coord, extent, t.device)
    y = torch.empty(_n_samples(org.shape[0], extent), 3, dtype=torch.float32, device=t.device) if out is None else out
    d, m = geo.to_desc(org.shape[0], extent), fused._mlp_struct(params)
    _lib.check(_lib.load().nic_hash_fused_forward(ctypes.byref(d), _lib.ptr(t), _lib.ptr(org), ctypes.byref(m), _lib.ptr(y), _lib.stream_ptr(t.device)),
               "nic_hash_fused_forward")
    return y


@fused._on_tensor_device
def hash_fused_forward_u8(geo: HashGeometry, stored: torch.Tensor, coord, extent: Sequence[int], num_bits: int,
                          params: Sequence[torch.Tensor]) -> torch.Tensor:
    """``hash_fused_forward`` from the compact uint8 table (nic_hash_fused_forward_u8): the rows of ``hash_encode_u8`` into the same decoder code"""
    if stored.dtype != torch.uint8 or not stored.is_cuda or stored.dim() != 1 or not stored.is_contiguous():
        raise ValueError("stored must be a contiguous 1-D uint8 tensor on a HIP device")
    if stored.numel() != hash_stored_bytes(geo):
        raise ValueError(f"stored holds {stored.numel()} bytes, the geometry needs {hash_stored_bytes(geo)}")
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    org = geo.upload_origins(coord, extent, stored.device)
    y = torch.empty(_n_samples(org.shape[0], extent), 3, dtype=torch.float32, device=stored.device)
    d, m = geo.to_desc(org.shape[0], extent), fused._mlp_struct(params)
    _lib.check(_lib.load().nic_hash_fused_forward_u8(ctypes.byref(d), int(num_bits), _lib.ptr(stored), _lib.ptr(org), ctypes.byref(m), _lib.ptr(y),
                                                     _lib.stream_ptr(stored.device)), "nic_hash_fused_forward_u8")
    return y


@fused._on_tensor_device
def hash_fused_forward_bits(geo: HashGeometry, packed: torch.Tensor, coord, extent: Sequence[int], num_bits: int,
                            params: Sequence[torch.Tensor]) -> torch.Tensor:
    """``hash_fused_forward_u8`` from the bit-packed table (nic_hash_fused_forward_bits)"""
    _check_packed(geo, packed, num_bits)
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    org = geo.upload_origins(coord, extent, packed.device)
    y = torch.empty(_n_samples(org.shape[0], extent), 3, dtype=torch.float32, device=packed.device)
    d, m = geo.to_desc(org.shape[0], extent), fused._mlp_struct(params)
    _lib.check(_lib.load().nic_hash_fused_forward_bits(ctypes.byref(d), int(num_bits), _lib.ptr(packed), _lib.ptr(org), ctypes.byref(m), _lib.ptr(y),
                                                       _lib.stream_ptr(packed.device)), "nic_hash_fused_forward_bits")
    return y


@fused._on_tensor_device
def hash_fused_forward_backward(geo: HashGeometry, table: torch.Tensor, coord, extent: Sequence[int], params: Sequence[torch.Tensor],
                                target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], table_grad: Optional[torch.Tensor] = None,
                                loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0, want_y: bool = False, quant=None,
                                add_grads: bool = False, add_loss: bool = False, tail=None):
    """the whole training step of a hash-grid field in two launches (nic_hash_fused_forward_backward): loss = mean((y - target)^2) * loss_scale.
    ``table_grad``: d loss / d table is ADDED into it (None: frozen table, no scatter).  ``mlp_grads``: six buffers like ``params``, overwritten
    (``add_grads``: added to).  ``quant``: None or (num_bits, seed, offset, sample_base) for ``hash_encode_noisy``'s noise.  ``tail``: an
    ``optim.StepTail`` on ``table_grad`` / ``mlp_grads`` - committed once the launch is queued.  Returns (loss [1], y or None)."""
    t = _check_table(geo, table.detach())
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    org = geo.upload_origins(coord, extent, t.device)
    n = _n_samples(org.shape[0], extent)
    target = _lib.require_cuda_f32(target, "target")
    if tuple(target.shape) != (n, 3):
        raise ValueError(f"target must be [{n}, 3], got {tuple(target.shape)}")
    _check_grads(geo, table_grad, mlp_grads, params)
    loss = torch.empty(1, dtype=torch.float32, device=t.device) if loss is None else loss
    y = torch.empty(n, 3, dtype=torch.float32, device=t.device) if want_y else None
    lib = _lib.load()
    d, m, gs = geo.to_desc(org.shape[0], extent), fused._mlp_struct(params), fused._grads_struct(list(mlp_grads))
    q = _quant_struct(quant)
    ws = _lib.workspace(t.device, int(lib.nic_hash_fused_workspace_bytes(ctypes.byref(d), ctypes.byref(m))))
    flags = (_lib.NIC_HASH_FUSED_ADD_GRADS if add_grads else 0) | (_lib.NIC_HASH_FUSED_ADD_LOSS if add_loss else 0)
    _lib.check(lib.nic_hash_fused_forward_backward(ctypes.byref(d), None if q is None else ctypes.byref(q), _lib.ptr(t), _lib.ptr(org), ctypes.byref(m),
                                                   _lib.ptr(target), float(loss_scale), _lib.ptr(table_grad), ctypes.byref(gs), _lib.ptr(loss), _lib.ptr(y),
                                                   flags, _lib.ptr(ws), ws.numel(), None if tail is None else ctypes.byref(tail.struct),
                                                   _lib.stream_ptr(t.device)), "nic_hash_fused_forward_backward")
    if tail is not None:
        tail.commit()
    return loss, y


# ---- B fields of one geometry per launch (include/nicv2_hip.h, nic_hash_batch_*; csrc/hashgrid_batch.hip) ---------------------------
def _persistent_grid(n_waves: int, cap: int) -> int:
    """workgroups of a persistent launch over ``n_waves`` patches, four to a workgroup: a multiple of 8, at most ``cap`` (hash_common.hpp)"""
    return min((((int(n_waves) + 3) // 4) + 7) // 8 * 8, int(cap))


def _patches(geo: HashGeometry, num_crops: int, extent: Sequence[int]) -> int:
    ps = 8 if geo.dim == 2 else 4
    n = int(num_crops)
    for e in extent:
        n *= (int(e) + ps - 1) // ps
    return n


def hash_batch_groups(n_fields: int, patches: int, cap: int, groups_per_field: int = 0) -> int:
    """G, the workgroups one field of a batched launch gets (nic_hash_batch_*; the rule in Python ints).  ``patches``: the 8 x 8 / 4 x 4 x 4
    patches of ONE field's crops; ``cap``: the workgroups of a persistent launch (one per CU, a multiple of 8).  0 = automatic: ``cap // n_fields``
    rounded up to a multiple of 8, at least 8, at most the grid one field alone would launch; a positive value must be a multiple of 8 within
    that grid."""
    n_fields, g = int(n_fields), int(groups_per_field)
    if n_fields < 1:
        raise ValueError("a batch holds at least one field")
    top = _persistent_grid(patches, cap)
    if g < 0 or g % 8 or g > top:
        raise ValueError(f"groups_per_field {g}: 0 (automatic) or a multiple of 8 up to {top}, the grid of one field alone")
    if g > 0:
        return g
    return min(max((int(cap) // n_fields + 7) // 8 * 8, 8), top)


def hash_batch_groups_p16(n_fields: int, items: int, cap: int, wide: bool, groups_per_field: int = 0) -> int:
    """G of a batched launch on the 16-bit matrix pipe (nic_hash_batch_forward_p16): ``hash_batch_groups`` on that kernel's workgroup cap.
    ``items``: the wave items of ONE field (its patches, or ceil(points / 64)); ``cap``: one workgroup per CU, a multiple of 8; ``wide``:
    levels * features > 32.  Where it is not, the kernel's 61 KB of LDS let two workgroups share a CU and the cap doubles - for the automatic G
    and for the single-field grid that bounds an explicit one."""
    return hash_batch_groups(n_fields, items, int(cap) * (1 if wide else 2), groups_per_field)


BATCH_DECODER_SHAPES =((64, None), (64,), (64, 64), (64,), (3, 64), (3,))     # None: L F


def _check_batch_tables(geo: HashGeometry, tables: torch.Tensor, name: str = "tables") -> None:
    """the shape of stacked tables: [B, L, T, F] (the field strides follow from the geometry)"""
    if not isinstance(tables, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if tables.dim() != 4 or tuple(tables.shape[1:]) != geo.table_shape() or tables.shape[0] < 1:
        raise ValueError(f"{name} must be [B, {', '.join(str(v) for v in geo.table_shape())}] = [fields, levels, 2^log2_table, features], got {tuple(tables.shape)}")


def _check_batch_decoder(geo: HashGeometry, params: Sequence[torch.Tensor], n_fields: int, name: str = "params") -> List[torch.Tensor]:
    """the shapes of six stacked tensors W1 [B, 64, L F], b1 [B, 64], W2 [B, 64, 64], b2 [B, 64], W3 [B, 3, 64], b3 [B, 3]"""
    params = list(params)
    if len(params) != 6:
        raise ValueError(f"{name}: six stacked tensors W1, b1, W2, b2, W3, b3 (the batched kernels decode with 3 Linear layers of 64 hidden units)")
    for t, s, n in zip(params, BATCH_DECODER_SHAPES, ("W1", "b1", "W2", "b2", "W3", "b3")):
        want = (n_fields, *(geo.width if v is None else v for v in s))
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
            raise ValueError(f"{name}: {n} must be {want}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return params


def _require_stacked(tensors: Sequence[torch.Tensor], name: str) -> None:
    """after every shape check: contiguous fp32 on the device - the kernel reads the fields at the strides of the geometry, in place"""
    for t in tensors:
        if _lib.require_cuda_f32(t, name) is not t:
            raise ValueError(f"{name} must be contiguous: the kernel reads the fields at the strides of the geometry")


def _batch_origins(geo: HashGeometry, coord, extent: Sequence[int], n_fields: int, device) -> torch.Tensor:
    """int32 [B, num_crops, dim] on the device.  ``coord`` [num_crops, dim]: the crops of every field; [B, num_crops, dim]: each field's own.
    Host origins are validated per field like ``check_crops``; a device tensor is taken as is (validating it would sync)."""
    if isinstance(coord, torch.Tensor) and coord.is_cuda:
        o = coord.to(torch.int32)
        if o.dim() == 3 and (o.shape[0] != n_fields or o.shape[2] != geo.dim):
            raise ValueError(f"per-field origins must be [{n_fields}, num_crops, {geo.dim}], got {tuple(o.shape)}")
        o = o if o.dim() == 3 else o.reshape(1, -1, geo.dim).expand(n_fields, -1, -1)
        return o.contiguous()
    c = torch.as_tensor(coord)
    if c.dim() == 3:
        if c.shape[0] != n_fields or c.shape[2] != geo.dim:
            raise ValueError(f"per-field origins must be [{n_fields}, num_crops, {geo.dim}], got {tuple(c.shape)}")
        o = torch.stack([geo.check_crops(c[b], extent) for b in range(n_fields)])
    else:
        o = geo.check_crops(c, extent).unsqueeze(0).expand(n_fields, -1, -1)
    return o.to(torch.int32).contiguous().to(device, non_blocking=True)


@fused._on_tensor_device
def hash_batch_forward(geo: HashGeometry, tables: torch.Tensor, coord, extent: Sequence[int], params: Sequence[torch.Tensor],
                       groups_per_field: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, N, 3]: ``hash_fused_forward`` of B stacked fields of one geometry in ONE launch (nic_hash_batch_forward).  ``tables`` [B, L, T, F],
    ``params`` the six stacked decoder tensors, ``coord`` [num_crops, dim] (shared) or [B, num_crops, dim] (per field)."""
    t = tables.detach() if isinstance(tables, torch.Tensor) else tables
    _check_batch_tables(geo, t)
    n_fields = t.shape[0]
    params = _check_batch_decoder(geo, [q.detach() if isinstance(q, torch.Tensor) else q for q in params], n_fields)
    _require_stacked([t], "tables")
    _require_stacked(params, "params")
    org = _batch_origins(geo, coord, extent, n_fields, t.device)
    n = _n_samples(org.shape[1], extent)
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n_fields, n, 3)):
        raise ValueError(f"out must be a contiguous fp32 device tensor [{n_fields}, {n}, 3]")
    y = torch.empty(n_fields, n, 3, dtype=torch.float32, device=t.device) if out is None else out
    d, m = geo.to_desc(org.shape[1], extent), fused._mlp_struct(params)
    _lib.check(_lib.load().nic_hash_batch_forward(ctypes.byref(d), n_fields, int(groups_per_field), _lib.ptr(t), _lib.ptr(org), ctypes.byref(m), _lib.ptr(y),
                                                  _lib.stream_ptr(t.device)), "nic_hash_batch_forward")
    return y


@fused._on_tensor_device
def hash_batch_forward_backward(geo: HashGeometry, tables: torch.Tensor, coord, extent: Sequence[int], params: Sequence[torch.Tensor],
                                target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], table_grads: Optional[torch.Tensor] = None,
                                loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0, want_y: bool = False, quant=None,
                                add_grads: bool = False, add_loss: bool = False, groups_per_field: int = 0):
    """``hash_fused_forward_backward`` of B stacked fields in TWO launches whatever B is (nic_hash_batch_forward_backward): loss[b] =
    mean((y_b - target_b)^2) * loss_scale over field b's samples.  ``target`` [B, N, 3]; ``table_grads`` [B, L, T, F] is ADDED to (None: frozen
    tables, no scatter); ``mlp_grads``: six buffers like ``params``, overwritten (``add_grads``: added to); ``quant``: None or (num_bits, seed,
    offset, sample_base) - every field sees the noise of a single-field call with the same tuple.  There is no optimiser tail: one ``FusedAdam``
    over the stacked tensors steps every field.  Returns (loss [B], y [B, N, 3] or None)."""
    t = tables.detach() if isinstance(tables, torch.Tensor) else tables
    _check_batch_tables(geo, t)
    n_fields = t.shape[0]
    params = _check_batch_decoder(geo, [q.detach() if isinstance(q, torch.Tensor) else q for q in params], n_fields)
    mlp_grads = _check_batch_decoder(geo, mlp_grads, n_fields, "mlp_grads")
    if table_grads is not None:
        _check_batch_tables(geo, table_grads, "table_grads")
        if table_grads.shape[0] != n_fields:
            raise ValueError(f"table_grads holds {table_grads.shape[0]} fields, tables {n_fields}")
    if len(extent) != geo.dim or any(int(e) < 1 for e in extent):
        raise ValueError(f"extent {tuple(extent)} for a {geo.dim}D field")
    if not isinstance(target, torch.Tensor) or target.dim() != 3 or target.shape[0] != n_fields or target.shape[2] != 3:
        raise ValueError(f"target must be [{n_fields}, N, 3], got {tuple(target.shape) if isinstance(target, torch.Tensor) else type(target).__name__}")
    _require_stacked([t], "tables")
    _require_stacked(params, "params")
    _require_stacked(mlp_grads, "mlp_grads")
    if table_grads is not None:
        _require_stacked([table_grads], "table_grads")
    org = _batch_origins(geo, coord, extent, n_fields, t.device)
    n = _n_samples(org.shape[1], extent)
    if tuple(target.shape) != (n_fields, n, 3):
        raise ValueError(f"target must be [{n_fields}, {n}, 3], got {tuple(target.shape)}")
    target = _lib.require_cuda_f32(target, "target")
    if loss is not None and not (loss.is_cuda and loss.dtype == torch.float32 and loss.is_contiguous() and tuple(loss.shape) == (n_fields,)):
        raise ValueError(f"loss must be a contiguous fp32 device tensor [{n_fields}]")
    loss = torch.empty(n_fields, dtype=torch.float32, device=t.device) if loss is None else loss
    y = torch.empty(n_fields, n, 3, dtype=torch.float32, device=t.device) if want_y else None
    lib = _lib.load()
    d, m, gs = geo.to_desc(org.shape[1], extent), fused._mlp_struct(params), fused._grads_struct(list(mlp_grads))
    q = _quant_struct(quant)
    nbytes = int(lib.nic_hash_batch_workspace_bytes(ctypes.byref(d), n_fields, int(groups_per_field), ctypes.byref(m)))
    if nbytes == 0:          # refused: the entry point below names the reason with its code, and launches nothing on a 16-byte workspace
        nbytes = 16
    ws = _lib.workspace(t.device, nbytes)
    flags = (_lib.NIC_HASH_FUSED_ADD_GRADS if add_grads else 0) | (_lib.NIC_HASH_FUSED_ADD_LOSS if add_loss else 0)
    _lib.check(lib.nic_hash_batch_forward_backward(ctypes.byref(d), n_fields, int(groups_per_field), None if q is None else ctypes.byref(q), _lib.ptr(t),
                                                   _lib.ptr(org), ctypes.byref(m), _lib.ptr(target), float(loss_scale), _lib.ptr(table_grads),
                                                   ctypes.byref(gs), _lib.ptr(loss), _lib.ptr(y), flags, _lib.ptr(ws), nbytes, _lib.stream_ptr(t.device)),
               "nic_hash_batch_forward_backward")
    return loss, y


POINT_SOURCES = {"f32": _lib.NIC_HASH_SRC_F32, "u8": _lib.NIC_HASH_SRC_U8, "bits": _lib.NIC_HASH_SRC_BITS}


def _check_points(geo: HashGeometry, points: torch.Tensor) -> torch.Tensor:
    """[N, dim] fp32 on the device, contiguous; the values are the kernel's business (it clamps: the host never reads them)"""
    pts = _lib.require_cuda_f32(points.detach() if isinstance(points, torch.Tensor) else points, "points")
    if pts.dim() != 2 or pts.shape[1] != geo.dim:
        raise ValueError(f"points must be [N, {geo.dim}] for a {geo.dim}D field, got {tuple(pts.shape)}")
    return pts


def _point_desc(geo: HashGeometry) -> "_lib.NicHashDesc":
    if 256 * geo.s_max >= 2 ** 30:
        raise ValueError(f"a field of {geo.s_max} samples per axis is too large for the point entry points: 256 * S_max < 2^30")
    return geo.to_desc(1, geo.field_size)


def _point_source(geo: HashGeometry, data: torch.Tensor, kind: str, num_bits: Optional[int]) -> Tuple["_lib.NicHashSource", torch.Tensor]:
    """``nic_hash_source`` of a table: kind "f32" = the fp32 [L, T, F] table, "u8" = the compact uint8 one, "bits" = the bit-packed one"""
    if kind not in POINT_SOURCES:
        raise ValueError(f"table source {kind!r}: one of {sorted(POINT_SOURCES)}")
    if kind == "f32":
        if num_bits is not None:
            raise ValueError("an fp32 table has no num_bits")
        data = _check_table(geo, data.detach())
        return _lib.NicHashSource(POINT_SOURCES[kind], 0, data.data_ptr()), data
    if num_bits is None or not 1 <= int(num_bits) <= 8:
        raise ValueError("a stored table needs its num_bits in 1 .. 8")
    if kind == "bits":
        _check_packed(geo, data, num_bits)
    else:
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or not data.is_cuda or data.dim() != 1 or not data.is_contiguous():
            raise ValueError("stored must be a contiguous 1-D uint8 tensor on a HIP device")
        if data.numel() != hash_stored_bytes(geo):
            raise ValueError(f"stored holds {data.numel()} bytes, the geometry needs {hash_stored_bytes(geo)}")
    return _lib.NicHashSource(POINT_SOURCES[kind], int(num_bits), data.data_ptr()), data


def _batch_source_bytes(geo: HashGeometry, kind: str, num_bits: Optional[int]) -> int:
    """bytes of ONE field's stored table of ``kind`` "u8" / "bits": the stride of a stack of them"""
    if num_bits is None or isinstance(num_bits, bool) or _is_level_bits(num_bits) or not 1 <= int(num_bits) <= 8:
        raise ValueError("a stored table needs its num_bits in 1 .. 8")
    return hash_packed_bytes(geo, int(num_bits)) if kind == "bits" else hash_stored_bytes(geo)


def _check_batch_source(geo: HashGeometry, data, kind: str, num_bits: Optional[int]) -> int:
    """shape and dtype of the stacked tables of ``kind``: fp32 [B, L, T, F], or uint8 [B, bytes of one field]; returns B.  Host only."""
    if kind not in POINT_SOURCES:
        raise ValueError(f"table source {kind!r}: one of {sorted(POINT_SOURCES)}")
    if not isinstance(data, torch.Tensor):
        raise TypeError("data must be a torch.Tensor")
    if kind == "f32":
        if num_bits is not None:
            raise ValueError("an fp32 table has no num_bits")
        _check_batch_tables(geo, data, "data")
        if data.dtype != torch.float32:
            raise ValueError(f"data: fp32 tables for kind 'f32', got {data.dtype}")
        return data.shape[0]
    need = _batch_source_bytes(geo, kind, num_bits)
    if data.dtype != torch.uint8 or data.dim() != 2 or data.shape[0] < 1 or data.shape[1] != need:
        raise ValueError(f"data must be uint8 [B, {need}] = [fields, bytes of one {'bit-packed' if kind == 'bits' else 'compact uint8'} table] for kind "
                         f"{kind!r}, got {data.dtype} {tuple(data.shape)}")
    return data.shape[0]


def _require_on_device(t: torch.Tensor, name: str) -> None:
    """after every shape and dtype check: on a HIP device and contiguous - the kernel reads the fields in place, at the strides of the geometry"""
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}: this package only runs on a HIP device (no CPU path)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous: the kernel reads the fields at the strides of the geometry")


def _check_batch_lod(lod, n_fields: int, n: int):
    """None, or the level of detail per point of a batch: an fp32 tensor [N] shared by all fields or [B, N], each field its own; the values
    are the kernel's business (it clamps).  Host only: the device is asked after every shape."""
    if lod is None:
        return None
    if not isinstance(lod, torch.Tensor) or lod.dtype != torch.float32 or tuple(lod.shape) not in ((n,), (n_fields, n)):
        raise ValueError(f"lod must be fp32 [{n}] (shared) or [{n_fields}, {n}] (per field), one value per point, got "
                         f"{(lod.dtype, tuple(lod.shape)) if isinstance(lod, torch.Tensor) else type(lod).__name__}")
    return lod.detach()


def _stack_lod(lod: Optional[torch.Tensor], n_fields: int, device) -> Optional[torch.Tensor]:
    """the checked ``lod`` as the contiguous [B, N] the entry reads, on the device of the points"""
    if lod is None:
        return None
    if not lod.is_cuda:
        raise RuntimeError(f"lod lives on {lod.device}: this package only runs on a HIP device (no CPU path)")
    if lod.device != device:
        raise ValueError(f"lod lives on {lod.device}, the points on {device}")
    return (lod if lod.dim() == 2 else lod.unsqueeze(0).expand(n_fields, -1)).contiguous()


def _batch_forward_source(geo, data, params, kind, num_bits, coord, extent, points, groups_per_field, out, precision, lod=None):
    """``hash_batch_forward_source`` (``precision`` None) and ``hash_batch_forward_p16`` ("split" / "bf16"): one set of refusals, one launch;
    with ``lod`` = (lod, lod_uniform, fade) ``hash_batch_forward_points_lod`` (points, and no ``precision``)"""
    prec = None if precision is None else _check_precision(precision)
    n_fields = _check_batch_source(geo, data, kind, num_bits)
    data = data.detach()
    params = _check_batch_decoder(geo, [q.detach() if isinstance(q, torch.Tensor) else q for q in params], n_fields)
    if any(q.dtype != torch.float32 for q in params):
        raise ValueError("params: fp32 tensors")
    if (coord is None) == (points is None):
        raise ValueError("exactly one of coord (with extent) and points")
    if 256 * geo.s_max >= 2 ** 30:
        raise ValueError(f"a field of {geo.s_max} samples per axis is too large for the batched entry points: 256 * S_max < 2^30")
    if points is not None:
        if extent is not None:
            raise ValueError("extent belongs to coord: points carry their own positions")
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() not in (2, 3) or points.shape[-1] != geo.dim or (
                points.dim() == 3 and points.shape[0] != n_fields):
            raise ValueError(f"points must be fp32 [N, {geo.dim}] (shared) or [{n_fields}, N, {geo.dim}] (per field), got "
                             f"{(points.dtype, tuple(points.shape)) if isinstance(points, torch.Tensor) else type(points).__name__}")
        n = points.shape[-2]
        org = None
        lp = None if lod is None else _lod_struct(geo, lod[2], lod[1])
        lod_t = None if lod is None else _check_batch_lod(lod[0], n_fields, n)
    else:
        if extent is None:
            raise ValueError("coord needs the extent of its crops")
        org = _batch_origins(geo, coord, extent, n_fields, "cpu" if not (isinstance(coord, torch.Tensor) and coord.is_cuda) else coord.device)
        n = _n_samples(org.shape[1], extent)
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n_fields, n, 3)):
        raise ValueError(f"out must be a contiguous fp32 tensor [{n_fields}, {n}, 3]")
    # ---- the device, after every refusal the host can make
    _require_on_device(data, "data")
    for q in params:
        _require_on_device(q, "params")
    if kind == "bits" and data.data_ptr() % 4:
        raise ValueError("data must start on a 4-byte boundary: the packed gather reads aligned dwords")
    if out is not None:
        _require_on_device(out, "out")
    y = torch.empty(n_fields, n, 3, dtype=torch.float32, device=data.device) if out is None else out
    if points is not None:
        if not points.is_cuda:
            raise RuntimeError(f"points live on {points.device}: this package only runs on a HIP device (no CPU path)")
        if n == 0:
            return y
        pts = points.detach()
        pts = (pts if pts.dim() == 3 else pts.unsqueeze(0).expand(n_fields, -1, -1)).contiguous()
        d = _point_desc(geo)
        if lod is not None:
            lod_t, m = _stack_lod(lod_t, n_fields, pts.device), fused._mlp_struct(params)
            src = _lib.NicHashSource(POINT_SOURCES[kind], 0 if kind == "f32" else int(num_bits), data.data_ptr())
            _lib.check(_lib.load().nic_hash_batch_forward_points_lod(ctypes.byref(d), n_fields, int(groups_per_field), ctypes.byref(lp), ctypes.byref(src),
                                                                     _lib.ptr(pts), _lib.ptr(lod_t), n, ctypes.byref(m), _lib.ptr(y),
                                                                     _lib.stream_ptr(data.device)), "nic_hash_batch_forward_points_lod")
            return y
    else:
        pts = None
        org = org.to(data.device, non_blocking=True)
        d = geo.to_desc(org.shape[1], extent)
    src, m = _lib.NicHashSource(POINT_SOURCES[kind], 0 if kind == "f32" else int(num_bits), data.data_ptr()), fused._mlp_struct(params)
    head = (ctypes.byref(d), n_fields, int(groups_per_field), ctypes.byref(src), _lib.ptr(org), _lib.ptr(pts), n if pts is not None else 0, ctypes.byref(m))
    if prec is None:
        _lib.check(_lib.load().nic_hash_batch_forward_source(*head, _lib.ptr(y), _lib.stream_ptr(data.device)), "nic_hash_batch_forward_source")
    else:
        _lib.check(_lib.load().nic_hash_batch_forward_p16(*head, prec, _lib.ptr(y), _lib.stream_ptr(data.device)), "nic_hash_batch_forward_p16")
    return y


@fused._on_tensor_device
def hash_batch_forward_source(geo: HashGeometry, data: torch.Tensor, params: Sequence[torch.Tensor], kind: str = "f32", num_bits: Optional[int] = None,
                              coord=None, extent: Optional[Sequence[int]] = None, points: Optional[torch.Tensor] = None, groups_per_field: int = 0,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, N, 3]: B stacked fields of one geometry decoded in ONE launch from the table they hold (nic_hash_batch_forward_source).
    ``data``: kind "f32" = fp32 [B, L, T, F]; "u8" / "bits" = contiguous uint8 [B, bytes] on the device, bytes = ``hash_stored_bytes`` /
    ``hash_packed_bytes`` of ``num_bits``.  ``params``: the six stacked decoder tensors.  Exactly one position source: the crops ``coord``
    ([num_crops, dim] shared or [B, num_crops, dim] per field) of ``extent``, or ``points`` ([N, dim] shared by all fields or [B, N, dim] per
    field; fp32, sample units, clamped by the kernel like ``hash_fused_forward_points``).  Every shape and dtype is checked on the host first."""
    return _batch_forward_source(geo, data, params, kind, num_bits, coord, extent, points, groups_per_field, out, None)


@fused._on_tensor_device
def hash_batch_forward_p16(geo: HashGeometry, data: torch.Tensor, params: Sequence[torch.Tensor], precision: str, kind: str = "f32",
                           num_bits: Optional[int] = None, coord=None, extent: Optional[Sequence[int]] = None, points: Optional[torch.Tensor] = None,
                           groups_per_field: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, N, 3]: ``hash_batch_forward_source`` with the decoder's products on the 16-bit matrix pipe (nic_hash_batch_forward_p16; DESIGN
    4.7.15) - ``hash_fused_forward_p16`` of every field in ONE launch, bit for bit.  ``precision`` "split" (within 5e-6 of the fp32 route) or
    "bf16" (1e-3 at default initialisation); every other argument and every refusal is ``hash_batch_forward_source``'s.  ``groups_per_field``
    follows ``hash_batch_groups_p16``: two workgroups share a CU at levels * features <= 32."""
    _check_precision(precision)
    return _batch_forward_source(geo, data, params, kind, num_bits, coord, extent, points, groups_per_field, out, precision)


@fused._on_tensor_device
def hash_batch_forward_points_lod(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                  lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None, kind: str = "f32",
                                  num_bits: Optional[int] = None, groups_per_field: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, N, 3]: ``hash_batch_forward_source(points=)`` with a level of detail per point (nic_hash_batch_forward_points_lod) -
    ``hash_fused_forward_points_lod`` of every field in ONE launch, bit for bit.  ``lod``: None, or fp32 [N] shared by all fields or [B, N],
    each field its own; ``lod_uniform`` and ``fade`` (None: ``hash_lod_fade(geo)``) serve every field.  Every other argument and refusal is
    ``hash_batch_forward_source``'s."""
    if points is None:
        raise ValueError("points must be given: a level of detail is served at points only")
    return _batch_forward_source(geo, data, params, kind, num_bits, None, None, points, groups_per_field, out, None, (lod, lod_uniform, fade))


def _lod_args(geo: HashGeometry, lod, n: int, device):
    """() without a level of detail (``lod`` None: the plain entry point is called), else (``nic_hash_lod``, the checked per-point tensor or None)
    of ``lod`` = (lod, lod_uniform, fade)"""
    if lod is None:
        return ()
    per_point = _check_lod(lod[0], n, device)          # the tensor first, then fade and lod_uniform: the order the errors always had
    return _lod_struct(geo, lod[2], lod[1]), per_point


def _encode_points(geo, data, points, kind, num_bits, quant, lod):
    """``hash_encode_points`` (``lod`` None) and ``hash_encode_points_lod`` (``lod`` = (lod, lod_uniform, fade))"""
    src, data = _point_source(geo, data, kind, num_bits)
    pts = _check_points(geo, points)
    la = _lod_args(geo, lod, pts.shape[0], pts.device)
    d = _point_desc(geo)
    out = torch.empty(pts.shape[0], geo.width, dtype=torch.float32, device=data.device)
    if quant is not None and kind != "f32":
        raise ValueError("noise belongs to training, which reads the fp32 table")
    q = _quant_struct(quant)
    if pts.shape[0] == 0:
        return out
    qp, stream = None if q is None else ctypes.byref(q), _lib.stream_ptr(data.device)
    if la:
        _lib.check(_lib.load().nic_hash_encode_points_lod(ctypes.byref(d), ctypes.byref(la[0]), ctypes.byref(src), qp, _lib.ptr(pts), _lib.ptr(la[1]),
                                                          pts.shape[0], _lib.ptr(out), stream), "nic_hash_encode_points_lod")
    else:
        _lib.check(_lib.load().nic_hash_encode_points(ctypes.byref(d), ctypes.byref(src), qp, _lib.ptr(pts), pts.shape[0], _lib.ptr(out), stream),
                   "nic_hash_encode_points")
    return out


@fused._on_tensor_device
def hash_encode_points(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, kind: str = "f32", num_bits: Optional[int] = None,
                       quant=None) -> torch.Tensor:
    """[N, L F] encoding at ``points`` [N, dim] (fp32, sample units: p = i is the centre of sample i; anything outside [-1/2, S - 1/2] or not
    finite is clamped by the kernel) from the table ``data`` of ``kind`` "f32" / "u8" / "bits" (nic_hash_encode_points).  ``quant``: None or
    (num_bits, seed, offset, sample_base) for ``hash_encode_noisy``'s noise keyed by sample_base + row (fp32 table only)."""
    return _encode_points(geo, data, points, kind, num_bits, quant, None)


def _check_order(order, n: int, device) -> torch.Tensor:
    """an int32 [N] device tensor of row indices (``hash_point_order``); its values are the kernel's business (it clamps them)"""
    if not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or not order.is_cuda or order.dim() != 1 or not order.is_contiguous():
        raise ValueError("order must be a contiguous 1-D int32 tensor on a HIP device (hash_point_order)")
    if order.shape[0] != n:
        raise ValueError(f"order names {order.shape[0]} rows, there are {n} points")
    if order.device != device:
        raise ValueError(f"order lives on {order.device}, the points on {device}")
    if n >= 2 ** 31:
        raise ValueError("an order indexes fewer than 2^31 points")
    return order


@fused._on_tensor_device
def hash_point_keys(geo: HashGeometry, points: torch.Tensor) -> torch.Tensor:
    """int64 [N]: the Morton key of every point's clamped fixed-point position (nic_hash_point_keys; include/nicv2_hip.h states the bits)"""
    pts = _check_points(geo, points)
    d = _point_desc(geo)
    keys = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    if pts.shape[0] == 0:
        return keys
    _lib.check(_lib.load().nic_hash_point_keys(ctypes.byref(d), _lib.ptr(pts), pts.shape[0], _lib.ptr(keys), _lib.stream_ptr(pts.device)),
               "nic_hash_point_keys")
    return keys


def hash_point_order(geo: HashGeometry, points: torch.Tensor) -> torch.Tensor:
    """int32 [N]: the permutation that walks ``points`` in cell (Z-) order - ``hash_point_keys`` through a stable device sort, so it is
    deterministic.  For a fixed point set compute it once and pass it to every step."""
    keys = hash_point_keys(geo, points)
    if keys.shape[0] >= 2 ** 31:
        raise ValueError("an order indexes fewer than 2^31 points")
    return torch.sort(keys, stable=True).indices.to(torch.int32)


# ---- B fields trained at their own points per launch (include/nicv2_hip_ext.h, nic_hash_batch_forward_backward_points) -------------
def _check_batch_points(geo: HashGeometry, points, n_fields: int) -> int:
    """the shape and dtype of a batch's points - fp32 [N, dim] shared by all fields or [B, N, dim], each field its own; returns N.  Host only."""
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() not in (2, 3) or points.shape[-1] != geo.dim or (
            points.dim() == 3 and points.shape[0] != n_fields):
        raise ValueError(f"points must be fp32 [N, {geo.dim}] (shared) or [{n_fields}, N, {geo.dim}] (per field), got "
                         f"{(points.dtype, tuple(points.shape)) if isinstance(points, torch.Tensor) else type(points).__name__}")
    return int(points.shape[-2])


def _check_batch_counts(counts, n_fields: int, n: int):
    """``counts``: None, a sequence of B ints or an integer tensor [B] - a host one is validated to 0 <= n_b <= n and becomes an int32 CPU
    tensor, a device one must be int32 and contiguous and is taken as is (the kernels clamp it; validating it would sync)"""
    if counts is None:
        return None
    if isinstance(counts, torch.Tensor) and counts.is_cuda:
        if counts.dtype != torch.int32 or tuple(counts.shape) != (n_fields,) or not counts.is_contiguous():
            raise ValueError(f"counts on the device must be a contiguous int32 tensor [{n_fields}], got {counts.dtype} {tuple(counts.shape)}")
        return counts
    if isinstance(counts, torch.Tensor):
        if counts.dtype not in (torch.int32, torch.int64) or tuple(counts.shape) != (n_fields,):
            raise ValueError(f"counts must be an integer tensor [{n_fields}], got {counts.dtype} {tuple(counts.shape)}")
        values = [int(v) for v in counts.tolist()]
    else:
        values = list(counts)
        if len(values) != n_fields or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in values):
            raise ValueError(f"counts must be {n_fields} ints, one per field, got {counts!r}")
        values = [int(v) for v in values]
    if any(not 0 <= v <= n for v in values):
        raise ValueError(f"counts must lie in 0 .. {n} (the points a field's row holds), got {values}")
    return torch.tensor(values, dtype=torch.int32)


def _check_batch_order(order, n_fields: int, n: int):
    """an int32 [B, N] tensor of field-local row indices (``hash_batch_point_order``); its values are the kernel's business (it clamps them)"""
    if order is None:
        return None
    if not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or tuple(order.shape) != (n_fields, n):
        raise ValueError(f"order must be an int32 tensor [{n_fields}, {n}] of field-local rows (hash_batch_point_order), got "
                         f"{(order.dtype, tuple(order.shape)) if isinstance(order, torch.Tensor) else type(order).__name__}")
    return order


def _stack_points(points: torch.Tensor, n_fields: int) -> torch.Tensor:
    pts = points.detach()
    return (pts if pts.dim() == 3 else pts.unsqueeze(0).expand(n_fields, -1, -1)).contiguous()


@fused._on_tensor_device
def hash_batch_point_order(geo: HashGeometry, points: torch.Tensor, counts=None) -> torch.Tensor:
    """int32 [B, N]: row b is ``hash_point_order`` of field b's first ``counts[b]`` points (all N without ``counts``), field-local; what a row
    holds past its count is the remaining indices in row order (the kernels never read them).  ONE ``hash_point_keys`` launch over the
    flattened points - the keys depend on the geometry only -, the keys at or past a field's count set to the largest int64, one stable
    ``torch.sort`` along dim 1."""
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 3 or points.shape[2] != geo.dim or points.shape[0] < 1:
        raise ValueError(f"points must be fp32 [B, N, {geo.dim}], got {(points.dtype, tuple(points.shape)) if isinstance(points, torch.Tensor) else type(points).__name__}")
    b, n = int(points.shape[0]), int(points.shape[1])
    counts = _check_batch_counts(counts, b, n)
    if n >= 2 ** 31:
        raise ValueError("an order indexes fewer than 2^31 points")
    keys = hash_point_keys(geo, points.detach().reshape(b * n, geo.dim)).reshape(b, n)
    if counts is not None:
        past = torch.arange(n, device=keys.device).unsqueeze(0) >= counts.to(keys.device).unsqueeze(1)
        keys = keys.masked_fill(past, torch.iinfo(torch.int64).max)
    return torch.sort(keys, dim=1, stable=True).indices.to(torch.int32)


def _batch_forward_backward_points(geo, tables, points, params, target, mlp_grads, table_grads, order, counts, loss, loss_scale, want_y, quant, add_grads,
                                   add_loss, groups_per_field, lod, dpoints=False, dlod=False):
    """``hash_batch_forward_backward_points`` (``lod`` None) and ``hash_batch_forward_backward_points_lod`` (``lod`` = (lod, lod_uniform, fade));
    with ``dpoints`` - None for a fresh tensor, or the tensor to fill - ``hash_batch_forward_backward_points_grad``, which returns it too; with
    ``dlod`` on top (``lod`` and ``dpoints`` are then given) - None for a fresh tensor (zeros), or the fp32 [B, N] tensor to fill -
    ``hash_batch_forward_backward_points_grad_lod``, which returns both"""
    t = tables.detach() if isinstance(tables, torch.Tensor) else tables
    _check_batch_tables(geo, t)
    n_fields = t.shape[0]
    params = _check_batch_decoder(geo, [q.detach() if isinstance(q, torch.Tensor) else q for q in params], n_fields)
    mlp_grads = _check_batch_decoder(geo, mlp_grads, n_fields, "mlp_grads")
    if table_grads is not None:
        _check_batch_tables(geo, table_grads, "table_grads")
        if table_grads.shape[0] != n_fields:
            raise ValueError(f"table_grads holds {table_grads.shape[0]} fields, tables {n_fields}")
    n = _check_batch_points(geo, points, n_fields)
    if n < 1:
        raise ValueError("no points")
    if n >= 2 ** 31:
        raise ValueError("a field's row holds fewer than 2^31 points")
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (n_fields, n, 3):
        raise ValueError(f"target must be [{n_fields}, {n}, 3], got {tuple(target.shape) if isinstance(target, torch.Tensor) else type(target).__name__}")
    counts = _check_batch_counts(counts, n_fields, n)
    order = _check_batch_order(order, n_fields, n)
    lod_t = None if lod is None else _check_batch_lod(lod[0], n_fields, n)
    lp = None if lod is None else _lod_struct(geo, lod[2], lod[1])
    y_out = want_y if isinstance(want_y, torch.Tensor) else None
    if y_out is not None and not (y_out.dtype == torch.float32 and y_out.is_contiguous() and tuple(y_out.shape) == (n_fields, n, 3)):
        raise ValueError(f"want_y as a tensor must be contiguous fp32 [{n_fields}, {n}, 3]")
    if loss is not None and not (isinstance(loss, torch.Tensor) and loss.dtype == torch.float32 and loss.is_contiguous() and tuple(loss.shape) == (n_fields,)):
        raise ValueError(f"loss must be a contiguous fp32 device tensor [{n_fields}]")
    if dpoints is not False and dpoints is not None:
        _check_batch_dpoints_shape(geo, n_fields, n, dpoints)
    if dlod is not False and dlod is not None:
        _check_batch_dlod_shape(n_fields, n, dlod)
    _point_desc(geo)
    # ---- the device, after every refusal the host can make
    _require_stacked([t], "tables")
    _require_stacked(params, "params")
    _require_stacked(mlp_grads, "mlp_grads")
    if table_grads is not None:
        _require_stacked([table_grads], "table_grads")
    _require_on_device(points, "points")
    target = _lib.require_cuda_f32(target, "target")
    for x, name in ((order, "order"), (y_out, "want_y"), (loss, "loss")):
        if x is not None:
            _require_on_device(x, name)
    pts = _stack_points(points, n_fields)
    lod_t = _stack_lod(lod_t, n_fields, pts.device)
    counts = None if counts is None else counts.to(t.device, non_blocking=True)
    loss = torch.empty(n_fields, dtype=torch.float32, device=t.device) if loss is None else loss
    if y_out is not None:
        y = y_out
    elif want_y:
        y = (torch.empty if counts is None else torch.zeros)(n_fields, n, 3, dtype=torch.float32, device=t.device)
    else:
        y = None
    lib = _lib.load()
    d, m, gs = _point_desc(geo), fused._mlp_struct(params), fused._grads_struct(list(mlp_grads))
    q = _quant_struct(quant)
    nbytes = int(lib.nic_hash_batch_points_workspace_bytes(ctypes.byref(d), n_fields, int(groups_per_field), n, ctypes.byref(m)))
    if nbytes == 0:          # refused: the entry point below names the reason with its code, and launches nothing on a 16-byte workspace
        nbytes = 16
    ws = _lib.workspace(t.device, nbytes)
    flags = (_lib.NIC_HASH_FUSED_ADD_GRADS if add_grads else 0) | (_lib.NIC_HASH_FUSED_ADD_LOSS if add_loss else 0)
    qp = None if q is None else ctypes.byref(q)
    tail = (_lib.ptr(counts), _lib.ptr(order), ctypes.byref(m), _lib.ptr(target), float(loss_scale), _lib.ptr(table_grads), ctypes.byref(gs), _lib.ptr(loss),
            _lib.ptr(y), flags, _lib.ptr(ws), nbytes, _lib.stream_ptr(t.device))
    if dpoints is not False:
        if dpoints is None:      # rows at or past a field's count, and rows an order does not name, are not written: zero in a fresh tensor
            dpoints = (torch.empty if counts is None and order is None else torch.zeros)(n_fields, n, geo.dim, dtype=torch.float32, device=t.device)
        else:
            _check_batch_dpoints_device(dpoints, pts.device)
        if dlod is not False:
            if dlod is None:
                dlod = torch.zeros(n_fields, n, dtype=torch.float32, device=t.device)
            else:
                _check_batch_dlod_device(dlod, pts.device)
            _lib.check(lib.nic_hash_batch_forward_backward_points_grad_lod(
                ctypes.byref(d), n_fields, int(groups_per_field), ctypes.byref(lp), qp, _lib.ptr(t), _lib.ptr(pts), _lib.ptr(lod_t), n, _lib.ptr(counts),
                _lib.ptr(order), ctypes.byref(m), _lib.ptr(target), float(loss_scale), _lib.ptr(table_grads), ctypes.byref(gs), _lib.ptr(loss), _lib.ptr(y),
                _lib.ptr(dpoints), _lib.ptr(dlod), flags, _lib.ptr(ws), nbytes, _lib.stream_ptr(t.device)),
                "nic_hash_batch_forward_backward_points_grad_lod")
            return loss, y, dpoints, dlod
        _lib.check(lib.nic_hash_batch_forward_backward_points_grad(
            ctypes.byref(d), n_fields, int(groups_per_field), None if lp is None else ctypes.byref(lp), qp, _lib.ptr(t), _lib.ptr(pts), _lib.ptr(lod_t), n,
            _lib.ptr(counts), _lib.ptr(order), ctypes.byref(m), _lib.ptr(target), float(loss_scale), _lib.ptr(table_grads), ctypes.byref(gs), _lib.ptr(loss),
            _lib.ptr(y), _lib.ptr(dpoints), flags, _lib.ptr(ws), nbytes, _lib.stream_ptr(t.device)), "nic_hash_batch_forward_backward_points_grad")
        return loss, y, dpoints
    if lp is None:
        _lib.check(lib.nic_hash_batch_forward_backward_points(ctypes.byref(d), n_fields, int(groups_per_field), qp, _lib.ptr(t), _lib.ptr(pts), n, *tail),
                   "nic_hash_batch_forward_backward_points")
    else:
        _lib.check(lib.nic_hash_batch_forward_backward_points_lod(ctypes.byref(d), n_fields, int(groups_per_field), ctypes.byref(lp), qp, _lib.ptr(t),
                                                                  _lib.ptr(pts), _lib.ptr(lod_t), n, *tail), "nic_hash_batch_forward_backward_points_lod")
    return loss, y


@fused._on_tensor_device
def hash_batch_forward_backward_points(geo: HashGeometry, tables: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                       target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], table_grads: Optional[torch.Tensor] = None,
                                       order: Optional[torch.Tensor] = None, counts=None, loss: Optional[torch.Tensor] = None,
                                       loss_scale: float = 1.0, want_y=False, quant=None, add_grads: bool = False, add_loss: bool = False,
                                       groups_per_field: int = 0):
    """``hash_fused_forward_backward_points`` of B stacked fields, each at ITS OWN points, in TWO launches whatever B is
    (nic_hash_batch_forward_backward_points).  ``points`` fp32 [B, N, dim] (or [N, dim], shared), ``target`` [B, N, 3].
    ``counts``: None, B ints or an int32 [B] tensor - field b trains on its first ``counts[b]`` rows only (a host value is validated to
    0 .. N, a device tensor is clamped by the kernel), and loss[b] = mean((y_b - target_b)^2) * loss_scale over THOSE rows; a field with no
    point has loss 0, decoder gradients 0 and an untouched table gradient.  ``order``: None or int32 [B, N] of field-local rows
    (``hash_batch_point_order``) - wave w of field b takes rows order[b, 64 w ..]; targets, outputs and noise keys stay at the caller's rows.
    ``want_y``: True, or a contiguous fp32 [B, N, 3] device tensor to write into; rows at or past a field's count are not written (zero in
    the tensor ``want_y=True`` allocates).  Everything else as ``hash_batch_forward_backward``.  Returns (loss [B], y or None)."""
    return _batch_forward_backward_points(geo, tables, points, params, target, mlp_grads, table_grads, order, counts, loss, loss_scale, want_y, quant,
                                          add_grads, add_loss, groups_per_field, None)


@fused._on_tensor_device
def hash_batch_forward_backward_points_lod(geo: HashGeometry, tables: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                           target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], lod: Optional[torch.Tensor] = None,
                                           lod_uniform: float = 0.0, fade=None, table_grads: Optional[torch.Tensor] = None,
                                           order: Optional[torch.Tensor] = None, counts=None, loss: Optional[torch.Tensor] = None,
                                           loss_scale: float = 1.0, want_y=False, quant=None, add_grads: bool = False, add_loss: bool = False,
                                           groups_per_field: int = 0):
    """``hash_batch_forward_backward_points`` with a level of detail per point (nic_hash_batch_forward_backward_points_lod):
    the same two launches, every field's row weighed as in ``hash_encode_points_lod`` and its gradient weighed again before the scatter -
    ``hash_fused_forward_backward_points_lod`` per field.  ``lod``: None, or fp32 [N] shared by all fields or [B, N], each field its own,
    read at the row the point is read at (with an ``order``: at ``order[b, pos]``); ``lod_uniform`` and ``fade`` (None:
    ``hash_lod_fade(geo)``) serve every field.  Returns (loss [B], y or None)."""
    return _batch_forward_backward_points(geo, tables, points, params, target, mlp_grads, table_grads, order, counts, loss, loss_scale, want_y, quant,
                                          add_grads, add_loss, groups_per_field, (lod, lod_uniform, fade))


def _encode_points_backward(geo, points, dx, table_grad, order, lod):
    """``hash_encode_points_backward`` (``lod`` None) and ``hash_encode_points_backward_lod`` (``lod`` = (lod, lod_uniform, fade))"""
    _check_grads(geo, table_grad)
    pts = _check_points(geo, points)
    n = pts.shape[0]
    dx = _lib.require_cuda_f32(dx, "dx")
    if tuple(dx.shape) != (n, geo.width):
        raise ValueError(f"dx must be [{n}, {geo.width}], got {tuple(dx.shape)}")
    la = _lod_args(geo, lod, n, pts.device)
    d = _point_desc(geo)
    if order is not None:
        order = _check_order(order, n, pts.device)
    if n == 0:
        return
    lib, stream = _lib.load(), _lib.stream_ptr(table_grad.device)
    if la:
        _lib.check(lib.nic_hash_encode_points_backward_lod(ctypes.byref(d), ctypes.byref(la[0]), _lib.ptr(pts), _lib.ptr(la[1]), n, _lib.ptr(dx),
                                                           _lib.ptr(order), _lib.ptr(table_grad), stream), "nic_hash_encode_points_backward_lod")
    elif order is not None:
        _lib.check(lib.nic_hash_encode_points_backward_ordered(ctypes.byref(d), _lib.ptr(pts), n, _lib.ptr(dx), _lib.ptr(order), _lib.ptr(table_grad),
                                                               stream), "nic_hash_encode_points_backward_ordered")
    else:
        _lib.check(lib.nic_hash_encode_points_backward(ctypes.byref(d), _lib.ptr(pts), n, _lib.ptr(dx), _lib.ptr(table_grad), stream),
                   "nic_hash_encode_points_backward")


@fused._on_tensor_device
def hash_encode_points_backward(geo: HashGeometry, points: torch.Tensor, dx: torch.Tensor, table_grad: torch.Tensor,
                                order: Optional[torch.Tensor] = None) -> None:
    """ADDS d loss / d table for the [N, L F] gradient ``dx`` of ``hash_encode_points`` into ``table_grad`` (nic_hash_encode_points_backward;
    fp32 atomics, neighbouring points of one cell summed first).  ``order``: an int32 [N] device tensor (``hash_point_order``) - lane n of the
    launch takes point ``order[n]`` (nic_hash_encode_points_backward_ordered): the same sums, neighbours in cell order merged."""
    _encode_points_backward(geo, points, dx, table_grad, order, None)


def _fused_forward_points(geo, data, points, params, kind, num_bits, lod):
    """``hash_fused_forward_points`` (``lod`` None) and ``hash_fused_forward_points_lod`` (``lod`` = (lod, lod_uniform, fade))"""
    src, data = _point_source(geo, data, kind, num_bits)
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    pts = _check_points(geo, points)
    n = pts.shape[0]
    la = _lod_args(geo, lod, n, pts.device)
    d, m = _point_desc(geo), fused._mlp_struct(params)
    y = torch.empty(n, 3, dtype=torch.float32, device=data.device)
    if n == 0:
        return y
    if la:
        _lib.check(_lib.load().nic_hash_fused_forward_points_lod(ctypes.byref(d), ctypes.byref(la[0]), ctypes.byref(src), _lib.ptr(pts), _lib.ptr(la[1]), n,
                                                                 ctypes.byref(m), _lib.ptr(y), _lib.stream_ptr(data.device)),
                   "nic_hash_fused_forward_points_lod")
    else:
        _lib.check(_lib.load().nic_hash_fused_forward_points(ctypes.byref(d), ctypes.byref(src), _lib.ptr(pts), n, ctypes.byref(m), _lib.ptr(y),
                                                             _lib.stream_ptr(data.device)), "nic_hash_fused_forward_points")
    return y


@fused._on_tensor_device
def hash_fused_forward_points(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor], kind: str = "f32",
                              num_bits: Optional[int] = None) -> torch.Tensor:
    """[N, 3] = ColorDecoder(hash_encode_points(...)) in one launch (nic_hash_fused_forward_points); ``params`` = W1, b1, W2, b2, W3, b3"""
    return _fused_forward_points(geo, data, points, params, kind, num_bits, None)


def _fused_forward_backward_points(geo, table, points, params, target, mlp_grads, table_grad, order, loss, loss_scale, want_y, quant, add_grads,
                                   add_loss, tail, lod, dpoints=None, dlod=None, weighted=None):
    """``hash_fused_forward_backward_points`` (``lod`` None) and ``hash_fused_forward_backward_points_lod`` (``lod`` = (lod, lod_uniform, fade));
    with ``dpoints`` (checked by the caller) ``hash_fused_forward_backward_points_grad``, which takes either; with ``dlod`` on top (checked by
    the caller; ``lod`` is then required) ``hash_fused_forward_backward_points_grad_lod``.  ``weighted``: None, or (weight,) - the checked
    per-point weights or None - for ``hash_fused_forward_backward_points_weighted``, the one entry that takes every combination of the rest"""
    t = _check_table(geo, table.detach())
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    pts = _check_points(geo, points)
    n = pts.shape[0]
    if n < 1:
        raise ValueError("no points")
    target = _lib.require_cuda_f32(target, "target")
    if tuple(target.shape) != (n, 3):
        raise ValueError(f"target must be [{n}, 3], got {tuple(target.shape)}")
    lod_tensor = None if lod is None else _check_lod(lod[0], n, pts.device)
    if order is not None:
        order = _check_order(order, n, pts.device)
    _check_grads(geo, table_grad, mlp_grads, params)
    d = _point_desc(geo)
    lp = None if lod is None else _lod_struct(geo, lod[2], lod[1])
    loss = torch.empty(1, dtype=torch.float32, device=t.device) if loss is None else loss
    y = torch.empty(n, 3, dtype=torch.float32, device=t.device) if want_y else None
    lib = _lib.load()
    m, gs = fused._mlp_struct(params), fused._grads_struct(list(mlp_grads))
    q = _quant_struct(quant)
    ws = _lib.workspace(t.device, int(lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(d), ctypes.byref(m))))
    flags = (_lib.NIC_HASH_FUSED_ADD_GRADS if add_grads else 0) | (_lib.NIC_HASH_FUSED_ADD_LOSS if add_loss else 0)
    qp, head = None if q is None else ctypes.byref(q), (ctypes.byref(d),) if lp is None else (ctypes.byref(d), ctypes.byref(lp))
    where = (_lib.ptr(pts), n) if lp is None else (_lib.ptr(pts), _lib.ptr(lod_tensor), n)
    name = "nic_hash_fused_forward_backward_points" if lp is None else "nic_hash_fused_forward_backward_points_lod"
    out = (_lib.ptr(y),)
    if dpoints is not None:                                # the one entry with a nullable nic_hash_lod, and the gradient after y
        head, where = (ctypes.byref(d), None if lp is None else ctypes.byref(lp)), (_lib.ptr(pts), _lib.ptr(lod_tensor), n)
        name, out = "nic_hash_fused_forward_backward_points_grad", (_lib.ptr(y), _lib.ptr(dpoints))
    if dlod is not None:                                   # the same entry with a level of detail always on, and dlod after dpoints
        name, out = "nic_hash_fused_forward_backward_points_grad_lod", (_lib.ptr(y), _lib.ptr(dpoints), _lib.ptr(dlod))
    if weighted is not None:                               # nullable nic_hash_lod, weight after lod, both gradients nullable
        head, where = (ctypes.byref(d), None if lp is None else ctypes.byref(lp)), (_lib.ptr(pts), _lib.ptr(lod_tensor), _lib.ptr(weighted[0]), n)
        name, out = "nic_hash_fused_forward_backward_points_weighted", (_lib.ptr(y), _lib.ptr(dpoints), _lib.ptr(dlod))
    _lib.check(getattr(lib, name)(*head, qp, _lib.ptr(t), *where, _lib.ptr(order), ctypes.byref(m), _lib.ptr(target), float(loss_scale),
                                  _lib.ptr(table_grad), ctypes.byref(gs), _lib.ptr(loss), *out, flags, _lib.ptr(ws), ws.numel(),
                                  None if tail is None else ctypes.byref(tail.struct), _lib.stream_ptr(t.device)), name)
    if tail is not None:
        tail.commit()
    return loss, y


@fused._on_tensor_device
def hash_fused_forward_backward_points(geo: HashGeometry, table: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                       target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], table_grad: Optional[torch.Tensor] = None,
                                       order: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0,
                                       want_y: bool = False, quant=None, add_grads: bool = False, add_loss: bool = False, tail=None):
    """``hash_fused_forward_backward`` on (point, colour) samples (nic_hash_fused_forward_backward_points): loss = mean((y - target)^2) *
    loss_scale over ``points`` [N, dim] with ``target`` [N, 3], in two launches.  ``order``: None or an int32 [N] device tensor
    (``hash_point_order``) - wave w takes points order[64 w ..]; targets, outputs and noise keys stay at the caller's rows, so the result is the
    unordered call's up to the order of the sums.  Everything else as there.  Returns (loss [1], y or None)."""
    return _fused_forward_backward_points(geo, table, points, params, target, mlp_grads, table_grad, order, loss, loss_scale, want_y, quant,
                                          add_grads, add_loss, tail, None)


@functools.lru_cache(maxsize=64)
def hash_lod_fade(geo: HashGeometry) -> Tuple[float, ...]:
    """the default fade start of every level (nic_hash_lod): max(0, log2(S_max / R_l)) in float64, rounded once to fp32 - the level's cell size
    in octaves of samples, so a level whose cells are no larger than a sample (R_l >= S_max) starts to fade at once"""
    return tuple(ctypes.c_float(max(0.0, math.log2(geo.s_max / int(r)))).value for r in geo.resolutions)


def _check_fade(levels: int, fade) -> Tuple[float, ...]:
    """a fade start per level: a sequence of ``levels`` finite values >= 0, as a tuple of fp32 values (anything else: ValueError)"""
    if isinstance(fade, (str, bytes)) or not hasattr(fade, "__len__") or not hasattr(fade, "__iter__"):
        raise ValueError(f"lod_fade is a sequence of {levels} finite values >= 0, got {fade!r}")
    try:
        out = tuple(ctypes.c_float(float(v)).value for v in fade)
    except (TypeError, ValueError):
        raise ValueError(f"lod_fade is a sequence of {levels} finite values >= 0, got {fade!r}") from None
    if len(out) != int(levels):
        raise ValueError(f"{len(out)} fade starts for {levels} levels")
    if any(not math.isfinite(v) or v < 0 for v in out):
        raise ValueError(f"lod_fade {out}: each finite and >= 0")
    return out


def _lod_struct(geo: HashGeometry, fade, lod_uniform: float) -> "_lib.NicHashLod":
    lp = _lib.NicHashLod()
    lp.fade[:geo.levels] = hash_lod_fade(geo) if fade is None else _check_fade(geo.levels, fade)
    if not math.isfinite(float(lod_uniform)):
        raise ValueError(f"lod_uniform {lod_uniform!r} is not finite")
    lp.lod_uniform = float(lod_uniform)
    return lp


def _check_lod(lod: Optional[torch.Tensor], n: int, device) -> Optional[torch.Tensor]:
    """None, or a level of detail per point: fp32 [N] on the points' device, contiguous; the values are the kernel's business (it clamps)"""
    if lod is None:
        return None
    lod = _lib.require_cuda_f32(lod.detach() if isinstance(lod, torch.Tensor) else lod, "lod")
    if tuple(lod.shape) != (n,):
        raise ValueError(f"lod must be [{n}], one value per point, got {tuple(lod.shape)}")
    if lod.device != device:
        raise ValueError(f"lod lives on {lod.device}, the points on {device}")
    return lod


@fused._on_tensor_device
def hash_encode_points_lod(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0,
                           fade=None, kind: str = "f32", num_bits: Optional[int] = None, quant=None) -> torch.Tensor:
    """``hash_encode_points`` with a level of detail per point (nic_hash_encode_points_lod): lambda = (``lod`` [N] or 0) + ``lod_uniform``, NaN ->
    0, clamped to [0, 32]; level l is weighed by min(max((fade[l] - lambda) + 1, 0), 1), ``fade`` = None for ``hash_lod_fade(geo)``.  At weight 1
    the columns are ``hash_encode_points``' bit for bit, at weight 0 they are 0 and the level's table is not read."""
    return _encode_points(geo, data, points, kind, num_bits, quant, (lod, lod_uniform, fade))


@fused._on_tensor_device
def hash_encode_points_backward_lod(geo: HashGeometry, points: torch.Tensor, dx: torch.Tensor, table_grad: torch.Tensor,
                                    lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None,
                                    order: Optional[torch.Tensor] = None) -> None:
    """``hash_encode_points_backward`` of ``hash_encode_points_lod`` (nic_hash_encode_points_backward_lod): ADDS the gradient of the table for
    ``dx`` weighed per point and level into ``table_grad``; a level of weight 0 takes no atomic.  ``order`` as there (``lod`` is read at
    ``order[n]`` like the point)."""
    _encode_points_backward(geo, points, dx, table_grad, order, (lod, lod_uniform, fade))


@fused._on_tensor_device
def hash_fused_forward_points_lod(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                  lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None, kind: str = "f32",
                                  num_bits: Optional[int] = None) -> torch.Tensor:
    """[N, 3] = ColorDecoder(hash_encode_points_lod(...)) in one launch (nic_hash_fused_forward_points_lod)"""
    return _fused_forward_points(geo, data, points, params, kind, num_bits, (lod, lod_uniform, fade))


@fused._on_tensor_device
def hash_fused_forward_backward_points_lod(geo: HashGeometry, table: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                           target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], lod: Optional[torch.Tensor] = None,
                                           lod_uniform: float = 0.0, fade=None, table_grad: Optional[torch.Tensor] = None,
                                           order: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0,
                                           want_y: bool = False, quant=None, add_grads: bool = False, add_loss: bool = False, tail=None):
    """``hash_fused_forward_backward_points`` with a level of detail per point (nic_hash_fused_forward_backward_points_lod): the same two
    launches, the row weighed as in ``hash_encode_points_lod`` and its gradient weighed again before the scatter.  Returns (loss [1], y or None)."""
    return _fused_forward_backward_points(geo, table, points, params, target, mlp_grads, table_grad, order, loss, loss_scale, want_y, quant,
                                          add_grads, add_loss, tail, (lod, lod_uniform, fade))


def _check_dpoints(geo: HashGeometry, points, dpoints) -> torch.Tensor:
    """the output of a joint step: an fp32 [N, dim] tensor on the points' HIP device, contiguous - the kernel writes it in place, so nothing is
    converted or copied (shapes and dtype are decided before any device is asked)"""
    if not isinstance(dpoints, torch.Tensor):
        raise TypeError("dpoints must be a torch.Tensor")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != geo.dim:
        raise ValueError(f"points must be [N, {geo.dim}] for a {geo.dim}D field, got "
                         f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    if tuple(dpoints.shape) != tuple(points.shape):
        raise ValueError(f"dpoints must be [{points.shape[0]}, {geo.dim}], one row per point, got {tuple(dpoints.shape)}")
    if dpoints.dtype != torch.float32:
        raise ValueError(f"dpoints has dtype {dpoints.dtype}; the kernel writes fp32")
    if not dpoints.is_contiguous():
        raise ValueError("dpoints must be contiguous: the kernel writes it in place")
    if not dpoints.is_cuda:
        raise RuntimeError(f"dpoints lives on {dpoints.device}: this package only runs on a HIP device (no CPU path)")
    if dpoints.device != points.device:
        raise ValueError(f"dpoints lives on {dpoints.device}, the points on {points.device}")
    return dpoints


@fused._on_tensor_device
def hash_fused_forward_backward_points_grad(geo: HashGeometry, table: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                            target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], lod: Optional[torch.Tensor] = None,
                                            lod_uniform: float = 0.0, fade=None, table_grad: Optional[torch.Tensor] = None,
                                            order: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0,
                                            want_y: bool = False, quant=None, add_grads: bool = False, add_loss: bool = False, tail=None,
                                            dpoints: Optional[torch.Tensor] = None):
    """``hash_fused_forward_backward_points`` - with any of ``lod`` / ``lod_uniform`` / ``fade``, ``hash_fused_forward_backward_points_lod`` -
    that also writes d loss / d points of the loss it returns (nic_hash_fused_forward_backward_points_grad): the same two
    launches, loss, y and gradients; the position gradient is ``hash_fused_points_grad``'s with ``target``, taken at the parameters the forward
    used (before the ``tail``'s step), noise and level weights constant.  ``dpoints``: None for a fresh tensor, or an fp32 [N, dim] device tensor
    that is overwritten (never added to).  Returns (loss [1], y or None, dpoints)."""
    if dpoints is None:
        pts = _check_points(geo, points)
        dpoints = torch.empty(pts.shape[0], geo.dim, dtype=torch.float32, device=pts.device)
    else:
        dpoints = _check_dpoints(geo, points, dpoints)
    plain = lod is None and fade is None and float(lod_uniform) == 0.0
    loss, y = _fused_forward_backward_points(geo, table, points, params, target, mlp_grads, table_grad, order, loss, loss_scale, want_y, quant,
                                             add_grads, add_loss, tail, None if plain else (lod, lod_uniform, fade), dpoints=dpoints)
    return loss, y, dpoints


def _grad_lod(geo: HashGeometry, lod, lod_uniform, fade, n: int, device, always: bool = False):
    """(``nic_hash_lod`` or None, the checked per-point tensor or None) of the gradient entries: no level of detail at all - ``lod`` None,
    ``lod_uniform`` 0 and ``fade`` None - is the plain launch, unless the entry is ``always`` a level-of-detail launch"""
    if not always and lod is None and fade is None and float(lod_uniform) == 0.0:
        return None, None
    per_point = _check_lod(lod, n, device)
    return _lod_struct(geo, fade, lod_uniform), per_point


def _check_dy_target(dy, target, n: int):
    """exactly one of ``dy`` / ``target``, [N, 3] (ValueError otherwise; decided on the shapes alone, before any device is asked)"""
    if (dy is None) == (target is None):
        raise ValueError("exactly one of dy and target: the gradient of the output, or the colours of a mean squared error")
    for name, v in (("dy", dy), ("target", target)):
        if v is not None and (not isinstance(v, torch.Tensor) or tuple(v.shape) != (n, 3)):
            raise ValueError(f"{name} must be [{n}, 3], got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")


def _encode_points_grad(geo: HashGeometry, data: torch.Tensor, points, dx, lod, lod_uniform, fade, name: str, src=None, quant=None,
                        dlod: bool = True):
    """the three layer-wise gradient entries after the check of their table, which is the caller's: ``data`` is the checked table, ``src`` its
    ``nic_hash_source`` or None for the entry that takes ``quant`` and the fp32 table; ``dlod`` False is the entry without d / d lambda, where no
    level of detail at all is the plain launch.  Returns (dpoints, dlod or None)"""
    pts = _check_points(geo, points)
    n = pts.shape[0]
    dx = _lib.require_cuda_f32(dx.detach() if isinstance(dx, torch.Tensor) else dx, "dx")
    if tuple(dx.shape) != (n, geo.width):
        raise ValueError(f"dx must be [{n}, {geo.width}], got {tuple(dx.shape)}")
    lp, lod_t = _grad_lod(geo, lod, lod_uniform, fade, n, pts.device, always=dlod)
    d = _point_desc(geo)
    if src is not None:
        source = (ctypes.byref(src),)
    else:
        q = _quant_struct(quant)
        source = (None if q is None else ctypes.byref(q), _lib.ptr(data))
    out = torch.empty(n, geo.dim, dtype=torch.float32, device=data.device)
    dl = torch.empty(n, dtype=torch.float32, device=data.device) if dlod else None
    if n == 0:
        return out, dl
    outs = (_lib.ptr(out), _lib.ptr(dl)) if dlod else (_lib.ptr(out),)
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(d), None if lp is None else ctypes.byref(lp), *source, _lib.ptr(pts), _lib.ptr(lod_t), n,
                                          _lib.ptr(dx), *outs, _lib.stream_ptr(data.device)), name)
    return out, dl


def _fused_points_grad(geo: HashGeometry, data, points, params, dy, target, loss_scale, want_y, kind, num_bits, lod, lod_uniform, fade, name: str,
                       dlod: bool):
    """the two fused gradient entries; ``dlod`` False is the one without d / d lambda, where no level of detail at all is the plain launch.
    Returns (y or None, dpoints, dlod or None)"""
    n = points.shape[0] if isinstance(points, torch.Tensor) and points.dim() == 2 else -1
    if n >= 0:
        _check_dy_target(dy, target, n)
    src, data = _point_source(geo, data, kind, num_bits)
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    pts = _check_points(geo, points)
    n = pts.shape[0]
    _check_dy_target(dy, target, n)
    dy = None if dy is None else _lib.require_cuda_f32(dy.detach(), "dy")
    target = None if target is None else _lib.require_cuda_f32(target.detach(), "target")
    lp, lod_t = _grad_lod(geo, lod, lod_uniform, fade, n, pts.device, always=dlod)
    d, m = _point_desc(geo), fused._mlp_struct(params)
    y = torch.empty(n, 3, dtype=torch.float32, device=data.device) if want_y else None
    out = torch.empty(n, geo.dim, dtype=torch.float32, device=data.device)
    dl = torch.empty(n, dtype=torch.float32, device=data.device) if dlod else None
    if n == 0:
        return y, out, dl
    outs = (_lib.ptr(out), _lib.ptr(dl)) if dlod else (_lib.ptr(out),)
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(d), None if lp is None else ctypes.byref(lp), ctypes.byref(src), _lib.ptr(pts), _lib.ptr(lod_t), n,
                                          ctypes.byref(m), _lib.ptr(dy), _lib.ptr(target), float(loss_scale), _lib.ptr(y), *outs,
                                          _lib.stream_ptr(data.device)), name)
    return y, out, dl


@fused._on_tensor_device
def hash_encode_points_grad(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, dx: torch.Tensor, kind: str = "f32",
                            num_bits: Optional[int] = None, lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None) -> torch.Tensor:
    """[N, dim] = d loss / d points for the [N, L F] gradient ``dx`` of ``hash_encode_points`` (``hash_encode_points_lod`` with any of ``lod`` /
    ``lod_uniform`` / ``fade``) from the table ``data`` of ``kind`` (nic_hash_encode_points_grad): the derivative of the multilinear
    interpolant at the rounded position, written (not added), 0 on an axis whose clamp moved the point.  The table is a constant."""
    src, data = _point_source(geo, data, kind, num_bits)
    return _encode_points_grad(geo, data, points, dx, lod, lod_uniform, fade, "nic_hash_encode_points_grad", src=src, dlod=False)[0]


@fused._on_tensor_device
def hash_fused_points_grad(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                           dy: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, loss_scale: float = 1.0, want_y: bool = True,
                           kind: str = "f32", num_bits: Optional[int] = None, lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0,
                           fade=None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """(y [N, 3] or None, dpoints [N, dim]) in one launch (nic_hash_fused_points_grad): y = ColorDecoder(hash_encode_points(...)),
    then d loss / d points for the output gradient ``dy`` [N, 3], or for loss = mean((y - ``target``)^2) * ``loss_scale`` - exactly one of the
    two.  Row and row gradient stay on the chip; table and decoder are constants."""
    return _fused_points_grad(geo, data, points, params, dy, target, loss_scale, want_y, kind, num_bits, lod, lod_uniform, fade,
                              "nic_hash_fused_points_grad", dlod=False)[:2]


# ---- the gradient with respect to the level of detail, next to the one with respect to the points (include/nicv2_hip_ext.h) ------
@fused._on_tensor_device
def hash_encode_points_grad_lod(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, dx: torch.Tensor, kind: str = "f32",
                                num_bits: Optional[int] = None, lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0,
                                fade=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dpoints [N, dim], dlod [N]) for the [N, L F] gradient ``dx`` of ``hash_encode_points_lod`` (nic_hash_encode_points_grad_lod; DESIGN
    4.7.22): ``dpoints`` is ``hash_encode_points_grad``'s with the same level of detail bit for bit; ``dlod[n]`` = - sum over the levels on
    the ramp 0 < (fade[l] - lambda) + 1 <= 1 of sum_f dx[n, l F + f] r[n, l, f], r the unweighed blend - the right-hand derivative with
    respect to lambda_n, exactly 0 where lambda_raw < 0, >= 32 or NaN.  Always a level-of-detail launch: ``lod`` None, ``lod_uniform`` 0 and
    ``fade`` None is lambda = 0 with the default fades.  Written, not added; the gradient for ``lod_uniform`` is ``dlod.sum()``."""
    src, data = _point_source(geo, data, kind, num_bits)
    return _encode_points_grad(geo, data, points, dx, lod, lod_uniform, fade, "nic_hash_encode_points_grad_lod", src=src)


@fused._on_tensor_device
def hash_fused_points_grad_lod(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                               dy: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, loss_scale: float = 1.0,
                               want_y: bool = True, kind: str = "f32", num_bits: Optional[int] = None, lod: Optional[torch.Tensor] = None,
                               lod_uniform: float = 0.0, fade=None) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(y [N, 3] or None, dpoints [N, dim], dlod [N]) in one launch (nic_hash_fused_points_grad_lod): ``hash_fused_points_grad``
    with the same level of detail - y and dpoints bit for bit - and the gradient with respect to lambda_n of ``hash_encode_points_grad_lod``
    for the row gradient the decoder's backward leaves on the chip.  Always a level-of-detail launch."""
    return _fused_points_grad(geo, data, points, params, dy, target, loss_scale, want_y, kind, num_bits, lod, lod_uniform, fade,
                              "nic_hash_fused_points_grad_lod", dlod=True)


# ---- the gradient with respect to the level of detail from the training step (include/nicv2_hip_ext.h) ----------------------------
def _check_dlod(points, dlod, device: bool = True) -> torch.Tensor:
    """the second output of a joint step: an fp32 [N] tensor on the points' HIP device, contiguous - the kernel writes it in place (``points``
    is a [N, dim] tensor).  ``device`` False: type, shape, dtype and layout only, what the host decides"""
    if not isinstance(dlod, torch.Tensor):
        raise TypeError("dlod must be a torch.Tensor")
    if tuple(dlod.shape) != (points.shape[0],):
        raise ValueError(f"dlod must be [{points.shape[0]}], one value per point, got {tuple(dlod.shape)}")
    if dlod.dtype != torch.float32:
        raise ValueError(f"dlod has dtype {dlod.dtype}; the kernel writes fp32")
    if not dlod.is_contiguous():
        raise ValueError("dlod must be contiguous: the kernel writes it in place")
    if not device:
        return dlod
    if not dlod.is_cuda:
        raise RuntimeError(f"dlod lives on {dlod.device}: this package only runs on a HIP device (no CPU path)")
    if dlod.device != points.device:
        raise ValueError(f"dlod lives on {dlod.device}, the points on {points.device}")
    return dlod


@fused._on_tensor_device
def hash_fused_forward_backward_points_grad_lod(geo: HashGeometry, table: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                                target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], lod: Optional[torch.Tensor] = None,
                                                lod_uniform: float = 0.0, fade=None, table_grad: Optional[torch.Tensor] = None,
                                                order: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0,
                                                want_y: bool = False, quant=None, add_grads: bool = False, add_loss: bool = False, tail=None,
                                                dpoints: Optional[torch.Tensor] = None, dlod: Optional[torch.Tensor] = None):
    """``hash_fused_forward_backward_points_grad`` that also writes d loss / d lambda of the loss it returns
    (nic_hash_fused_forward_backward_points_grad_lod): the same two launches, loss, y, gradients and ``dpoints``; ``dlod[n]`` =
    - sum over the levels on the ramp of sum_f g[n, l F + f] (r[n, l, f] + nz[n, l F + f]) - g the row gradient the step has on the chip, r the
    unweighed blend, nz the noise this step's forward added under ``quant`` (0 without) -, exactly 0 where lambda_raw < 0, >= 32 or NaN.
    Always a level-of-detail launch: ``lod`` None, ``lod_uniform`` 0 and ``fade`` None is lambda = 0 with the default fades.  ``dpoints``
    / ``dlod``: None for fresh tensors, or fp32 [N, dim] / [N] device tensors that are overwritten (never added to).  Returns (loss [1], y or
    None, dpoints, dlod)."""
    if dpoints is None:
        pts = _check_points(geo, points)
        dpoints = torch.empty(pts.shape[0], geo.dim, dtype=torch.float32, device=pts.device)
    else:
        dpoints = _check_dpoints(geo, points, dpoints)
    dlod = torch.empty(dpoints.shape[0], dtype=torch.float32, device=dpoints.device) if dlod is None else _check_dlod(dpoints, dlod)
    loss, y = _fused_forward_backward_points(geo, table, points, params, target, mlp_grads, table_grad, order, loss, loss_scale, want_y, quant,
                                             add_grads, add_loss, tail, (lod, lod_uniform, fade), dpoints=dpoints, dlod=dlod)
    return loss, y, dpoints, dlod


@fused._on_tensor_device
def hash_encode_points_grad_lod_noisy(geo: HashGeometry, table: torch.Tensor, points: torch.Tensor, dx: torch.Tensor,
                                      lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None,
                                      quant=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dpoints [N, dim], dlod [N]) for the [N, L F] gradient ``dx`` of ``hash_encode_points_lod(table, .., quant=quant)`` from the fp32
    ``table`` (nic_hash_encode_points_grad_lod_noisy): ``hash_encode_points_grad_lod`` whose ``dlod`` counts the noise the
    forward added inside the weighed column - the slope of column l F + f on the ramp is -(r + nz).  ``quant``: None, or the forward's
    (num_bits, seed, offset, sample_base); with None both outputs are ``hash_encode_points_grad_lod``'s bit for bit."""
    t = _check_table(geo, table.detach())
    return _encode_points_grad(geo, t, points, dx, lod, lod_uniform, fade, "nic_hash_encode_points_grad_lod_noisy", quant=quant)


# ---- a weight per point in the loss of the training step (include/nicv2_hip_ext.h) ----------------------------------------------
def _check_weight(points, weight) -> torch.Tensor:
    """the loss weights of a step: an fp32 [N] tensor on the points' HIP device, contiguous (``points`` is a [N, dim] tensor) - what the host
    decides first, then where it lives; the values are the kernel's business (NaN and negative values count 0)"""
    if not isinstance(weight, torch.Tensor):
        raise ValueError(f"weight must be an fp32 [N] tensor, one value per point, got {type(weight).__name__}")
    if tuple(weight.shape) != (points.shape[0],):
        raise ValueError(f"weight must be [{points.shape[0]}], one value per point, got {tuple(weight.shape)}")
    if weight.dtype != torch.float32:
        raise ValueError(f"weight has dtype {weight.dtype}; the kernel reads fp32")
    if not weight.is_contiguous():
        raise ValueError("weight must be contiguous: the kernel reads it in place")
    if not weight.is_cuda:
        raise RuntimeError(f"weight lives on {weight.device}: this package only runs on a HIP device (no CPU path)")
    if weight.device != points.device:
        raise RuntimeError(f"weight lives on {weight.device}, the points on {points.device}")
    return weight.detach()


@fused._on_tensor_device
def hash_fused_forward_backward_points_weighted(geo: HashGeometry, table: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                                target: torch.Tensor, weight: Optional[torch.Tensor], mlp_grads: Sequence[torch.Tensor],
                                                lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None,
                                                table_grad: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None,
                                                loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0, want_y: bool = False, quant=None,
                                                add_grads: bool = False, add_loss: bool = False, tail=None,
                                                dpoints: Optional[torch.Tensor] = None, dlod: Optional[torch.Tensor] = None):
    """The fused step at points with a weight per point in its loss (nic_hash_fused_forward_backward_points_weighted):
    loss = ``loss_scale`` sum_n w_n sum_o (y[n, o] - target[n, o])^2 / (3 N), w_n = ``weight[n]`` where that is > 0 and 0 elsewhere (NaN and
    negative values count 0; +inf is the caller's error), N the number of points - not the sum of the weights.  Every gradient is that loss's:
    a point of weight 0 still gets its y and adds nothing anywhere.  ``weight``: fp32 [N] on the device, read at the caller's row like
    ``target``; None is w = 1.  ``lod`` / ``lod_uniform`` / ``fade``: all at their defaults is the step without a level of detail, anything
    else ``hash_fused_forward_backward_points_lod``'s.  ``dpoints`` / ``dlod``: None (not computed), or fp32 [N, dim] / [N] device tensors
    that are overwritten; ``dlod`` needs ``dpoints`` and makes the call a level-of-detail launch (lambda = 0 with the default fades when
    nothing else says so).  With ``weight`` None or ones the results are the sibling's with the same remaining arguments bit for bit (the
    table gradient up to the order of its atomics).  Returns (loss [1], y or None, dpoints, dlod)."""
    if dlod is not None and dpoints is None:
        raise ValueError("dlod needs dpoints: the gradient for the level of detail comes from the walk that makes the one for the points")
    if dpoints is not None:
        dpoints = _check_dpoints(geo, points, dpoints)
    if dlod is not None:
        dlod = _check_dlod(dpoints, dlod)
    if weight is not None:
        weight = _check_weight(_check_points(geo, points), weight)
    plain = dlod is None and lod is None and fade is None and float(lod_uniform) == 0.0
    loss, y = _fused_forward_backward_points(geo, table, points, params, target, mlp_grads, table_grad, order, loss, loss_scale, want_y, quant,
                                             add_grads, add_loss, tail, None if plain else (lod, lod_uniform, fade), dpoints=dpoints, dlod=dlod,
                                             weighted=(weight,))
    return loss, y, dpoints, dlod


def hash_mip_weights(n_points_per_mip: Sequence[int], mode="balanced") -> Tuple[float, ...]:
    """one loss weight per mip of a chain whose mip m holds ``n_points_per_mip[m]`` of the samples (``fit_mips_weighted``).  ``"balanced"``:
    w_m = N / ((M + 1) N_m) with N = sum N_m - the weighted loss over the joint set is then the mean of the M + 1 per-mip mean squared
    errors.  A sequence of M + 1 finite values >= 0 is returned as given (as floats).  Host arithmetic only."""
    counts = [int(c) for c in n_points_per_mip]
    if len(counts) < 1 or any(c < 1 for c in counts):
        raise ValueError(f"n_points_per_mip {counts}: at least one mip, each with at least one point")
    if isinstance(mode, str):
        if mode != "balanced":
            raise ValueError(f"mip weights {mode!r}: 'balanced' or a sequence of {len(counts)} values >= 0")
        total = sum(counts)
        return tuple(total / (len(counts) * c) for c in counts)
    try:
        out = tuple(float(v) for v in mode)
    except (TypeError, ValueError):
        raise ValueError(f"mip weights {mode!r}: 'balanced' or a sequence of {len(counts)} values >= 0") from None
    if len(out) != len(counts):
        raise ValueError(f"{len(out)} mip weights for {len(counts)} mips")
    if any(not math.isfinite(v) or v < 0 for v in out):
        raise ValueError(f"mip weights {out}: each finite and >= 0")
    return out


# ---- B fields per launch with the gradient with respect to the point coordinates (include/nicv2_hip_ext.h) ------------------------
def _check_batch_dpoints_shape(geo: HashGeometry, n_fields: int, n: int, dpoints) -> None:
    """``_check_dpoints`` for a batch, the part the host decides: an fp32 [B, N, dim] tensor, contiguous - the kernel writes it in place"""
    if not isinstance(dpoints, torch.Tensor):
        raise TypeError("dpoints must be a torch.Tensor")
    if tuple(dpoints.shape) != (n_fields, n, geo.dim):
        raise ValueError(f"dpoints must be [{n_fields}, {n}, {geo.dim}], one row per point of every field, got {tuple(dpoints.shape)}")
    if dpoints.dtype != torch.float32:
        raise ValueError(f"dpoints has dtype {dpoints.dtype}; the kernel writes fp32")
    if not dpoints.is_contiguous():
        raise ValueError("dpoints must be contiguous: the kernel writes it in place")


def _check_batch_dpoints_device(dpoints: torch.Tensor, device) -> None:
    """``_check_dpoints``' device part: on the points' HIP device"""
    if not dpoints.is_cuda:
        raise RuntimeError(f"dpoints lives on {dpoints.device}: this package only runs on a HIP device (no CPU path)")
    if dpoints.device != device:
        raise ValueError(f"dpoints lives on {dpoints.device}, the points on {device}")


def _check_batch_dlod_shape(n_fields: int, n: int, dlod) -> None:
    """``_check_dlod`` for a batch, the part the host decides: an fp32 [B, N] tensor, contiguous - the kernel writes it in place"""
    if not isinstance(dlod, torch.Tensor):
        raise TypeError("dlod must be a torch.Tensor")
    if tuple(dlod.shape) != (n_fields, n):
        raise ValueError(f"dlod must be [{n_fields}, {n}], one value per point of every field, got {tuple(dlod.shape)}")
    if dlod.dtype != torch.float32:
        raise ValueError(f"dlod has dtype {dlod.dtype}; the kernel writes fp32")
    if not dlod.is_contiguous():
        raise ValueError("dlod must be contiguous: the kernel writes it in place")


def _check_batch_dlod_device(dlod: torch.Tensor, device) -> None:
    """``_check_dlod``'s device part: on the points' HIP device"""
    if not dlod.is_cuda:
        raise RuntimeError(f"dlod lives on {dlod.device}: this package only runs on a HIP device (no CPU path)")
    if dlod.device != device:
        raise ValueError(f"dlod lives on {dlod.device}, the points on {device}")


def _plain_lod(lod, lod_uniform, fade) -> bool:
    """no level of detail at all - ``lod`` None, ``lod_uniform`` 0 and ``fade`` None: the gradient entries' plain launch (``_grad_lod``)"""
    return lod is None and fade is None and float(lod_uniform) == 0.0


def _batch_points_grad(geo, data, points, params, dy, target, loss_scale, counts, order, want_y, kind, num_bits, lod, lod_uniform, fade, groups_per_field,
                       dpoints=None, dlod=False):
    """``hash_batch_points_grad``; ``dpoints``: None for a fresh tensor, or the fp32 [B, N, dim] device tensor to fill.  With ``dlod`` - None
    for a fresh tensor (zeros), or the fp32 [B, N] device tensor to fill - ``hash_batch_points_grad_lod``: always a level-of-detail launch,
    and (y, dpoints, dlod) back"""
    n_fields = _check_batch_source(geo, data, kind, num_bits)
    data = data.detach()
    params = _check_batch_decoder(geo, [q.detach() if isinstance(q, torch.Tensor) else q for q in params], n_fields)
    if any(q.dtype != torch.float32 for q in params):
        raise ValueError("params: fp32 tensors")
    n = _check_batch_points(geo, points, n_fields)
    if n >= 2 ** 31:
        raise ValueError("a field's row holds fewer than 2^31 points")
    if (dy is None) == (target is None):
        raise ValueError("exactly one of dy and target: the gradient of the output, or the colours of a mean squared error")
    for name, v in (("dy", dy), ("target", target)):
        if v is not None and (not isinstance(v, torch.Tensor) or tuple(v.shape) != (n_fields, n, 3)):
            raise ValueError(f"{name} must be [{n_fields}, {n}, 3], got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
    counts = _check_batch_counts(counts, n_fields, n)
    order = _check_batch_order(order, n_fields, n)
    plain = dlod is False and _plain_lod(lod, lod_uniform, fade)
    lod_t = None if plain else _check_batch_lod(lod, n_fields, n)
    lp = None if plain else _lod_struct(geo, fade, lod_uniform)
    y_out = want_y if isinstance(want_y, torch.Tensor) else None
    if y_out is not None and not (y_out.dtype == torch.float32 and y_out.is_contiguous() and tuple(y_out.shape) == (n_fields, n, 3)):
        raise ValueError(f"want_y as a tensor must be contiguous fp32 [{n_fields}, {n}, 3]")
    if dpoints is not None:
        _check_batch_dpoints_shape(geo, n_fields, n, dpoints)
    if dlod is not False and dlod is not None:
        _check_batch_dlod_shape(n_fields, n, dlod)
    d = _point_desc(geo)
    # ---- the device, after every refusal the host can make
    _require_on_device(data, "data")
    for q in params:
        _require_on_device(q, "params")
    if kind == "bits" and data.data_ptr() % 4:
        raise ValueError("data must start on a 4-byte boundary: the packed gather reads aligned dwords")
    _require_on_device(points, "points")
    dy = None if dy is None else _lib.require_cuda_f32(dy.detach(), "dy")
    target = None if target is None else _lib.require_cuda_f32(target.detach(), "target")
    for x, name in ((order, "order"), (y_out, "want_y")):
        if x is not None:
            _require_on_device(x, name)
    pts = _stack_points(points, n_fields)
    lod_t = _stack_lod(lod_t, n_fields, pts.device)
    counts = None if counts is None else counts.to(data.device, non_blocking=True)
    fresh = torch.empty if counts is None and order is None else torch.zeros      # rows a field does not own, or an order does not name, are not written
    if y_out is not None:
        y = y_out
    else:
        y = fresh(n_fields, n, 3, dtype=torch.float32, device=data.device) if want_y else None
    if dpoints is None:
        dpoints = fresh(n_fields, n, geo.dim, dtype=torch.float32, device=data.device)
    else:
        _check_batch_dpoints_device(dpoints, pts.device)
    if dlod is None:                                  # a fresh one is zeros: rows a field does not own are not written
        dlod = torch.zeros(n_fields, n, dtype=torch.float32, device=data.device)
    elif dlod is not False:
        _check_batch_dlod_device(dlod, pts.device)
    if n == 0:
        return (y, dpoints) if dlod is False else (y, dpoints, dlod)
    src, m = _lib.NicHashSource(POINT_SOURCES[kind], 0 if kind == "f32" else int(num_bits), data.data_ptr()), fused._mlp_struct(params)
    if dlod is not False:
        _lib.check(_lib.load().nic_hash_batch_points_grad_lod(
            ctypes.byref(d), n_fields, int(groups_per_field), ctypes.byref(lp), ctypes.byref(src), _lib.ptr(pts), _lib.ptr(lod_t), n, _lib.ptr(counts),
            _lib.ptr(order), ctypes.byref(m), _lib.ptr(dy), _lib.ptr(target), float(loss_scale), _lib.ptr(y), _lib.ptr(dpoints), _lib.ptr(dlod),
            _lib.stream_ptr(data.device)), "nic_hash_batch_points_grad_lod")
        return y, dpoints, dlod
    _lib.check(_lib.load().nic_hash_batch_points_grad(
        ctypes.byref(d), n_fields, int(groups_per_field), None if lp is None else ctypes.byref(lp), ctypes.byref(src), _lib.ptr(pts), _lib.ptr(lod_t), n,
        _lib.ptr(counts), _lib.ptr(order), ctypes.byref(m), _lib.ptr(dy), _lib.ptr(target), float(loss_scale), _lib.ptr(y), _lib.ptr(dpoints),
        _lib.stream_ptr(data.device)), "nic_hash_batch_points_grad")
    return y, dpoints


@fused._on_tensor_device
def hash_batch_points_grad(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                           dy: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, loss_scale: float = 1.0, counts=None,
                           order: Optional[torch.Tensor] = None, want_y=True, kind: str = "f32", num_bits: Optional[int] = None,
                           lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None,
                           groups_per_field: int = 0) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """(y [B, N, 3] or None, dpoints [B, N, dim]): ``hash_fused_points_grad`` of B stacked fields, each at ITS OWN points, in ONE launch
    (nic_hash_batch_points_grad).  ``data`` / ``kind`` / ``num_bits`` / ``params`` / ``points`` as ``hash_batch_forward_source``
    takes them (fp32, uint8 or bit-packed stacks); exactly one of ``dy`` / ``target`` [B, N, 3]: the output gradient, or the colours of
    loss_b = mean((y_b - target_b)^2) * ``loss_scale`` over field b's OWN ``counts[b]`` rows.  ``counts`` / ``order`` as
    ``hash_batch_forward_backward_points``: rows at or past a field's count, and rows an ``order`` does not name, are not written (zero in
    the tensors this call allocates).  ``want_y``: True, False, or a contiguous fp32 [B, N, 3] device tensor to write into.  Any of ``lod``
    ([N] shared or [B, N]) / ``lod_uniform`` / ``fade`` makes it the call with a level of detail per point.  Tables and decoders are
    constants: nothing is added anywhere, the same call gives the same bits."""
    return _batch_points_grad(geo, data, points, params, dy, target, loss_scale, counts, order, want_y, kind, num_bits, lod, lod_uniform, fade,
                              groups_per_field)


@fused._on_tensor_device
def hash_batch_forward_backward_points_grad(geo: HashGeometry, tables: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                            target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], lod: Optional[torch.Tensor] = None,
                                            lod_uniform: float = 0.0, fade=None, table_grads: Optional[torch.Tensor] = None,
                                            order: Optional[torch.Tensor] = None, counts=None, loss: Optional[torch.Tensor] = None,
                                            loss_scale: float = 1.0, want_y=False, quant=None, add_grads: bool = False, add_loss: bool = False,
                                            groups_per_field: int = 0, dpoints: Optional[torch.Tensor] = None):
    """``hash_batch_forward_backward_points`` - with any of ``lod`` / ``lod_uniform`` / ``fade``, ``hash_batch_forward_backward_points_lod`` -
    that also writes d loss_b / d points of the loss it returns for field b (nic_hash_batch_forward_backward_points_grad):
    the same two launches, losses, y and gradients; the position gradient is ``hash_batch_points_grad``'s with ``target``, taken at the
    parameters the forward used, noise and level weights constant; frozen tables (``table_grads`` None) still give it.  ``dpoints``: None
    for a fresh tensor, or an fp32 [B, N, dim] device tensor that is overwritten (never added to, whatever ``add_grads`` says) at the rows
    each field owns.  Returns (loss [B], y or None, dpoints)."""
    return _batch_forward_backward_points(geo, tables, points, params, target, mlp_grads, table_grads, order, counts, loss, loss_scale, want_y, quant,
                                          add_grads, add_loss, groups_per_field, None if _plain_lod(lod, lod_uniform, fade) else (lod, lod_uniform, fade),
                                          dpoints=dpoints)


# ---- B fields per launch with the gradient with respect to the level of detail (include/nicv2_hip_ext.h) ---------------------------
@fused._on_tensor_device
def hash_batch_points_grad_lod(geo: HashGeometry, data: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                               lod: Optional[torch.Tensor] = None, lod_uniform: float = 0.0, fade=None, dy: Optional[torch.Tensor] = None,
                               target: Optional[torch.Tensor] = None, loss_scale: float = 1.0, counts=None, order: Optional[torch.Tensor] = None,
                               want_y=True, kind: str = "f32", num_bits: Optional[int] = None, groups_per_field: int = 0,
                               dpoints: Optional[torch.Tensor] = None,
                               dlod: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(y [B, N, 3] or None, dpoints [B, N, dim], dlod [B, N]): ``hash_fused_points_grad_lod`` of B stacked fields, each at ITS OWN points and
    its own level of detail, in ONE launch (nic_hash_batch_points_grad_lod) - ``hash_batch_points_grad`` with the same level of
    detail, y and dpoints bit for bit, and ``dlod[b, n]`` = - sum over the levels on the ramp 0 < (fade[l] - lambda) + 1 <= 1 of the row gradient
    times the unweighed blend of field b's table: the right-hand derivative with respect to lambda_{b, n}, exactly 0 where lambda_raw < 0,
    >= 32 or NaN.  ``lod``: None, fp32 [N] shared by all fields or [B, N]; always a level-of-detail launch (``lod`` None, ``lod_uniform`` 0
    and ``fade`` None is lambda = 0 with the default fades).  With ``target`` field b's gradient is scaled by ITS count.  ``dpoints`` /
    ``dlod``: None for fresh tensors (zero at the rows a field does not own), or contiguous fp32 [B, N, dim] / [B, N] device tensors that are
    overwritten at the rows each field owns.  The gradient for a shared ``lod`` is ``dlod.sum(0)``, for ``lod_uniform`` ``dlod.sum()``.
    Everything else is ``hash_batch_points_grad``'s."""
    return _batch_points_grad(geo, data, points, params, dy, target, loss_scale, counts, order, want_y, kind, num_bits, lod, lod_uniform, fade,
                              groups_per_field, dpoints=dpoints, dlod=dlod)


@fused._on_tensor_device
def hash_batch_forward_backward_points_grad_lod(geo: HashGeometry, tables: torch.Tensor, points: torch.Tensor, params: Sequence[torch.Tensor],
                                                target: torch.Tensor, mlp_grads: Sequence[torch.Tensor], lod: Optional[torch.Tensor] = None,
                                                lod_uniform: float = 0.0, fade=None, table_grads: Optional[torch.Tensor] = None,
                                                order: Optional[torch.Tensor] = None, counts=None, loss: Optional[torch.Tensor] = None,
                                                loss_scale: float = 1.0, want_y=False, quant=None, add_grads: bool = False, add_loss: bool = False,
                                                groups_per_field: int = 0, dpoints: Optional[torch.Tensor] = None,
                                                dlod: Optional[torch.Tensor] = None):
    """``hash_batch_forward_backward_points_grad`` that also writes d loss_b / d lambda of the loss it returns for field b
    (nic_hash_batch_forward_backward_points_grad_lod) - ``hash_fused_forward_backward_points_grad_lod`` per field in the same
    two launches: losses, y, gradients and ``dpoints`` are the sibling's with the same level of detail bit for bit; ``dlod[b, n]`` counts the
    noise this step's forward added under ``quant`` inside the weighed column (the slope on the ramp is -(r + nz), keyed by the field-local
    row whatever the ``order``), exactly 0 where lambda_raw < 0, >= 32 or NaN.  Always a level-of-detail launch.  ``dpoints`` / ``dlod``: None
    for fresh tensors, or contiguous fp32 [B, N, dim] / [B, N] device tensors that are overwritten (never added to, whatever ``add_grads``
    says) at the rows each field owns.  Returns (loss [B], y or None, dpoints, dlod)."""
    return _batch_forward_backward_points(geo, tables, points, params, target, mlp_grads, table_grads, order, counts, loss, loss_scale, want_y, quant,
                                          add_grads, add_loss, groups_per_field, (lod, lod_uniform, fade), dpoints=dpoints, dlod=dlod)


@fused._on_tensor_device
def hash_pack_bits_levels(geo: HashGeometry, table: torch.Tensor, level_bits, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """format /2 of an fp32 [L, T, F] table (nic_hash_pack_bits_levels): ``hash_pack_bits`` with ``level_bits[l]`` bits per value inside level
    l.  Clamp each level to its range first.  ``out``: a buffer of ``hash_packed_bytes(geo, level_bits)`` to fill (every byte is written)."""
    t = _check_table(geo, table.detach())
    lb = _level_bits_struct(geo, level_bits)
    if out is None:
        out = torch.empty(hash_packed_bytes(geo, level_bits), dtype=torch.uint8, device=t.device)
    _check_packed(geo, out, tuple(level_bits))
    _lib.check(_lib.load().nic_hash_pack_bits_levels(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), ctypes.byref(lb), _lib.ptr(t), _lib.ptr(out),
                                                     _lib.stream_ptr(t.device)), "nic_hash_pack_bits_levels")
    return out


@fused._on_tensor_device
def hash_clamp_levels(geo: HashGeometry, table: torch.Tensor, level_bits) -> torch.Tensor:
    """clamps level l of the fp32 [L, T, F] ``table`` to ``models._q_range(level_bits[l])`` IN PLACE (nic_hash_clamp_levels; a NaN stays)"""
    t = _check_table(geo, table.detach())
    if t.data_ptr() != table.data_ptr():
        raise ValueError("table must be contiguous: the kernel clamps it in place")
    lb = _level_bits_struct(geo, level_bits)
    _lib.check(_lib.load().nic_hash_clamp_levels(ctypes.byref(geo.to_desc(1, [1] * geo.dim)), ctypes.byref(lb), _lib.ptr(t), _lib.stream_ptr(t.device)),
               "nic_hash_clamp_levels")
    return table


def _levels_source(geo: HashGeometry, data: torch.Tensor, kind: str, level_bits) -> Tuple["_lib.NicHashSource", torch.Tensor]:
    """``nic_hash_source`` of a mixed-depth launch: "f32" = the fp32 [L, T, F] table, "bits" = a format /2 table (no uint8 form)"""
    if kind == "f32":
        data = _check_table(geo, data.detach())
    elif kind == "bits":
        _check_packed(geo, data, tuple(level_bits))
    else:
        raise ValueError(f"table source {kind!r} of a mixed-depth launch: 'f32' or 'bits'")
    return _lib.NicHashSource(POINT_SOURCES[kind], 0, data.data_ptr()), data


def _levels_positions(geo: HashGeometry, coord, extent, points, device):
    """exactly one position source -> (desc, origins or None, points or None, N)"""
    if (coord is None) == (points is None):
        raise ValueError("exactly one of coord (with extent) and points")
    if 256 * geo.s_max >= 2 ** 30:
        raise ValueError(f"a field of {geo.s_max} samples per axis is too large for the mixed-depth entry points: 256 * S_max < 2^30")
    if points is not None:
        pts = _check_points(geo, points)
        return _point_desc(geo), None, pts, pts.shape[0]
    org = geo.upload_origins(coord, extent, device)
    return geo.to_desc(org.shape[0], extent), org, None, _n_samples(org.shape[0], extent)


def _levels_quant(quant) -> Optional["_lib.NicHashQuant"]:
    """None or (seed, offset, sample_base): ``hash_encode_noisy``'s noise, its scale 2^-level_bits[l] on the columns of level l"""
    if quant is None:
        return None
    seed, offset, base = quant
    return _quant_struct((0, seed, offset, base))


@fused._on_tensor_device
def hash_encode_levels(geo: HashGeometry, data: torch.Tensor, level_bits, coord=None, extent: Optional[Sequence[int]] = None,
                       points: Optional[torch.Tensor] = None, kind: str = "f32", quant=None) -> torch.Tensor:
    """[N, L F] encoding with a bit depth per level (nic_hash_encode_levels) on the crops ``coord`` / ``extent`` or at ``points`` (exactly
    one), from the fp32 table (``kind`` "f32"; ``quant`` = None or (seed, offset, sample_base): per-level noise) or from a format /2 table
    (``kind`` "bits").  Columns l F .. of the result are those of the uniform-depth call at depth ``level_bits[l]``, bit for bit."""
    lb = _level_bits_struct(geo, level_bits)
    src, data = _levels_source(geo, data, kind, level_bits)
    if quant is not None and kind != "f32":
        raise ValueError("noise belongs to training, which reads the fp32 table")
    d, org, pts, n = _levels_positions(geo, coord, extent, points, data.device)
    out = torch.empty(n, geo.width, dtype=torch.float32, device=data.device)
    if n == 0:
        return out
    q = _levels_quant(quant)
    _lib.check(_lib.load().nic_hash_encode_levels(ctypes.byref(d), ctypes.byref(lb), ctypes.byref(src), None if q is None else ctypes.byref(q),
                                                  _lib.ptr(org), _lib.ptr(pts), n if pts is not None else 0, _lib.ptr(out),
                                                  _lib.stream_ptr(data.device)), "nic_hash_encode_levels")
    return out


@fused._on_tensor_device
def hash_fused_forward_levels(geo: HashGeometry, data: torch.Tensor, level_bits, params: Sequence[torch.Tensor], coord=None,
                              extent: Optional[Sequence[int]] = None, points: Optional[torch.Tensor] = None, kind: str = "f32") -> torch.Tensor:
    """[N, 3] = ColorDecoder(hash_encode_levels(...)) in one launch (nic_hash_fused_forward_levels)"""
    lb = _level_bits_struct(geo, level_bits)
    src, data = _levels_source(geo, data, kind, level_bits)
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    d, org, pts, n = _levels_positions(geo, coord, extent, points, data.device)
    y = torch.empty(n, 3, dtype=torch.float32, device=data.device)
    if n == 0:
        return y
    m = fused._mlp_struct(params)
    _lib.check(_lib.load().nic_hash_fused_forward_levels(ctypes.byref(d), ctypes.byref(lb), ctypes.byref(src), _lib.ptr(org), _lib.ptr(pts),
                                                         n if pts is not None else 0, ctypes.byref(m), _lib.ptr(y), _lib.stream_ptr(data.device)),
               "nic_hash_fused_forward_levels")
    return y


PRECISIONS = {"split": _lib.NIC_HASH_PREC_SPLIT, "bf16": _lib.NIC_HASH_PREC_BF16}


def _check_precision(precision) -> int:
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"precision {precision!r}: one of {sorted(PRECISIONS)} (or None: the fp32 route)")
    return PRECISIONS[precision]


def _check_p16_set(geo: HashGeometry, hidden: int, n_linear: int) -> None:
    if not hash_fused_supported(geo, hidden, n_linear):
        raise ValueError("precision= needs a geometry and decoder of the fused set (nic_hash_fused_supported): dim 2 / 3, features 1 / 2 / 4 / 8, "
                         "levels * features <= 64, 64 hidden units, 3 Linear layers")


@fused._on_tensor_device
def hash_fused_forward_p16(geo: HashGeometry, data: torch.Tensor, params: Sequence[torch.Tensor], precision: str, coord=None,
                           extent: Optional[Sequence[int]] = None, points: Optional[torch.Tensor] = None, kind: str = "f32",
                           num_bits: Optional[int] = None) -> torch.Tensor:
    """[N, 3] = ColorDecoder(hash_encode(...)) in one launch with the decoder's products on the 16-bit matrix pipe
    (nic_hash_fused_forward_p16; ``precision`` "split" or "bf16"), on the crops ``coord`` / ``extent`` or at ``points`` (exactly one), from
    the fp32 table (``kind`` "f32"), the compact uint8 one ("u8") or the bit-packed one ("bits", both with ``num_bits``)"""
    prec = _check_precision(precision)
    _check_p16_set(geo, params[0].shape[0] if len(params) else 0, len(params) // 2)
    src, data = _point_source(geo, data, kind, num_bits)
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    d, org, pts, n = _levels_positions(geo, coord, extent, points, data.device)
    y = torch.empty(n, 3, dtype=torch.float32, device=data.device)
    if n == 0:
        return y
    m = fused._mlp_struct(params)
    _lib.check(_lib.load().nic_hash_fused_forward_p16(ctypes.byref(d), ctypes.byref(src), _lib.ptr(org), _lib.ptr(pts), n if pts is not None else 0,
                                                      ctypes.byref(m), prec, _lib.ptr(y), _lib.stream_ptr(data.device)),
               "nic_hash_fused_forward_p16")
    return y


@fused._on_tensor_device
def hash_fused_forward_backward_levels(geo: HashGeometry, table: torch.Tensor, level_bits, params: Sequence[torch.Tensor], target: torch.Tensor,
                                       mlp_grads: Sequence[torch.Tensor], coord=None, extent: Optional[Sequence[int]] = None,
                                       points: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None,
                                       table_grad: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None, loss_scale: float = 1.0,
                                       want_y: bool = False, quant=None, add_grads: bool = False, add_loss: bool = False, tail=None):
    """``hash_fused_forward_backward`` (crops) / ``hash_fused_forward_backward_points`` (points, with ``order``) with a bit depth per level
    (nic_hash_fused_forward_backward_levels): the same two launches, ``quant`` = None or (seed, offset, sample_base) for per-level noise.
    Returns (loss [1], y or None)."""
    t = _check_table(geo, table.detach())
    lb = _level_bits_struct(geo, level_bits)
    params = _check_fused_decoder(geo, [q.detach() for q in params])
    d, org, pts, n = _levels_positions(geo, coord, extent, points, t.device)
    if n < 1:
        raise ValueError("no samples")
    target = _lib.require_cuda_f32(target, "target")
    if tuple(target.shape) != (n, 3):
        raise ValueError(f"target must be [{n}, 3], got {tuple(target.shape)}")
    if order is not None:
        if pts is None:
            raise ValueError("an order names points: it goes with points, not with crops")
        order = _check_order(order, n, pts.device)
    _check_grads(geo, table_grad, mlp_grads, params)
    loss = torch.empty(1, dtype=torch.float32, device=t.device) if loss is None else loss
    y = torch.empty(n, 3, dtype=torch.float32, device=t.device) if want_y else None
    lib = _lib.load()
    m, gs = fused._mlp_struct(params), fused._grads_struct(list(mlp_grads))
    q = _levels_quant(quant)
    ws = _lib.workspace(t.device, int(lib.nic_hash_fused_points_workspace_bytes(ctypes.byref(_point_desc(geo)), ctypes.byref(m))))
    flags = (_lib.NIC_HASH_FUSED_ADD_GRADS if add_grads else 0) | (_lib.NIC_HASH_FUSED_ADD_LOSS if add_loss else 0)
    _lib.check(lib.nic_hash_fused_forward_backward_levels(ctypes.byref(d), ctypes.byref(lb), None if q is None else ctypes.byref(q), _lib.ptr(t),
                                                          _lib.ptr(org), _lib.ptr(pts), n if pts is not None else 0, _lib.ptr(order), ctypes.byref(m),
                                                          _lib.ptr(target), float(loss_scale), _lib.ptr(table_grad), ctypes.byref(gs), _lib.ptr(loss),
                                                          _lib.ptr(y), flags, _lib.ptr(ws), ws.numel(),
                                                          None if tail is None else ctypes.byref(tail.struct), _lib.stream_ptr(t.device)),
               "nic_hash_fused_forward_backward_levels")
    if tail is not None:
        tail.commit()
    return loss, y


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


class HashEncodePointsFunction(torch.autograd.Function):
    """``hash_encode_points`` as a differentiable op of the fp32 table (not of the points): backward = ``nic_hash_encode_points_backward``
    into a fresh zero [L, T, F]"""

    @staticmethod
    def forward(ctx, table, geo: HashGeometry, points: torch.Tensor):
        ctx.geo, ctx.points = geo, points
        return hash_encode_points(geo, table, points)

    @staticmethod
    def backward(ctx, dx):
        g = torch.zeros(ctx.geo.table_shape(), dtype=torch.float32, device=dx.device)
        hash_encode_points_backward(ctx.geo, ctx.points, dx, g)
        return g, None, None


def hash_encode_points_differentiable(geo: HashGeometry, table: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """[N, L F] at ``points``, differentiable w.r.t. the fp32 ``table`` when it requires a gradient (``HashEncodePointsFunction``): the point
    counterpart of ``hash_encode_differentiable``, for callers that put their own decoder and loss behind the encoding"""
    pts = _check_points(geo, points)
    if not table.requires_grad:
        return hash_encode_points(geo, table, pts)
    return HashEncodePointsFunction.apply(table, geo, pts)


class _QueryPointsFunction(torch.autograd.Function):
    """``HashGridField.query`` as a differentiable op of the points (``query_differentiable``): backward = ``point_gradient`` with the
    output gradient; nothing for the field's parameters"""

    @staticmethod
    def forward(ctx, points, field, lod):
        ctx.field, ctx.lod = field, lod
        ctx.save_for_backward(points)
        return field.query(points, lod=lod)

    @staticmethod
    def backward(ctx, dy):
        points, = ctx.saved_tensors
        return ctx.field.point_gradient(points, dy=dy.contiguous(), lod=ctx.lod)[1], None, None


class _QueryPointsLodFunction(torch.autograd.Function):
    """``HashGridField.query(points, lod)`` as a differentiable op of the points and of the level of detail (``query_differentiable_lod``):
    backward = ``point_gradient_lod`` with the output gradient - ``dlod`` for a per-point ``lod``, its sum for a 0-dim one; nothing for the
    field's parameters"""

    @staticmethod
    def forward(ctx, points, lod, field):
        ctx.field = field
        ctx.lod = None if isinstance(lod, torch.Tensor) else lod
        ctx.save_for_backward(points, *([lod] if isinstance(lod, torch.Tensor) else []))
        return field.query(points, lod=lod)

    @staticmethod
    def backward(ctx, dy):
        points, *rest = ctx.saved_tensors
        lod = rest[0] if rest else ctx.lod
        _, dpoints, dlod = ctx.field.point_gradient_lod(points, lod, dy=dy.contiguous())
        glod = None
        if rest and ctx.needs_input_grad[1]:
            glod = (dlod if lod.dim() > 0 else dlod.sum()).to(lod.dtype).reshape(lod.shape)
        return (dpoints if ctx.needs_input_grad[0] else None), glod, None


class _TrainPointsFunction(torch.autograd.Function):
    """``HashGridField.train_points`` as a differentiable op of the points (``train_points_differentiable``): the forward trains the field and
    keeps d loss / d points of the loss it returns, the backward hands upstream * dpoints to the points"""

    @staticmethod
    def forward(ctx, points, field, target, kwargs):
        dp = torch.empty(points.shape, dtype=torch.float32, device=points.device)
        with torch.enable_grad():                      # the layer-wise step runs its own backward
            loss = field.train_points(points.detach(), target, dpoints=dp, **kwargs)
        ctx.save_for_backward(dp)
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        dp, = ctx.saved_tensors
        return g.reshape(()) * dp, None, None, None


class _TrainPointsLodFunction(torch.autograd.Function):
    """``HashGridField.train_points_grad_lod`` as a differentiable op of the points and of the level of detail
    (``train_points_differentiable_lod``): the forward trains the field and keeps d loss / d points and d loss / d lambda of the loss it
    returns, the backward hands upstream * dpoints and upstream * dlod (its sum for a 0-dim ``lod``) to whichever requires a gradient"""

    @staticmethod
    def forward(ctx, points, lod, field, target, kwargs):
        with torch.enable_grad():                      # the layer-wise step runs its own backward
            loss, dp, dl = field.train_points_grad_lod(points.detach(), target, lod.detach() if isinstance(lod, torch.Tensor) else lod, **kwargs)
        ctx.lod_shape = (lod.shape, lod.dtype) if isinstance(lod, torch.Tensor) else None
        ctx.save_for_backward(dp, dl)
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        dp, dl = ctx.saved_tensors
        g = g.reshape(())
        glod = None
        if ctx.lod_shape is not None and ctx.needs_input_grad[1]:
            shape, dtype = ctx.lod_shape
            glod = (g * (dl if len(shape) > 0 else dl.sum())).to(dtype).reshape(shape)
        return (g * dp if ctx.needs_input_grad[0] else None), glod, None, None, None


class _TrainPointsWeightedFunction(torch.autograd.Function):
    """``HashGridField.train_points_weighted`` as a differentiable op of the points and of the level of detail
    (``train_points_weighted_differentiable``): ``_TrainPointsLodFunction`` with the loss weights, and with a level of detail that may be
    absent (then only the points get a gradient)"""

    @staticmethod
    def forward(ctx, points, lod, field, target, weight, kwargs):
        dp = torch.empty(points.shape, dtype=torch.float32, device=points.device)
        dl = None if lod is None else torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
        with torch.enable_grad():                      # the layer-wise step runs its own backward
            loss = field.train_points_weighted(points.detach(), target, weight, lod=lod.detach() if isinstance(lod, torch.Tensor) else lod,
                                               dpoints=dp, dlod=dl, **kwargs)
        ctx.lod_shape = (lod.shape, lod.dtype) if isinstance(lod, torch.Tensor) else None
        ctx.save_for_backward(dp, *(() if dl is None else (dl,)))
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        dp, *rest = ctx.saved_tensors
        g = g.reshape(())
        glod = None
        if ctx.lod_shape is not None and ctx.needs_input_grad[1]:
            shape, dtype = ctx.lod_shape
            glod = (g * (rest[0] if len(shape) > 0 else rest[0].sum())).to(dtype).reshape(shape)
        return (g * dp if ctx.needs_input_grad[0] else None), glod, None, None, None, None


class _BatchQueryPointsFunction(torch.autograd.Function):
    """``HashGridFieldBatch.query`` / ``query_lod`` as a differentiable op of the points (``query_differentiable``): backward =
    ``point_gradient`` with the output gradient, summed over the fields for shared [N, dim] points; nothing for the fields' parameters"""

    @staticmethod
    def forward(ctx, points, batch, lod):
        ctx.batch, ctx.lod = batch, lod
        ctx.save_for_backward(points)
        return batch.query(points) if lod is None else batch.query_lod(points, lod)

    @staticmethod
    def backward(ctx, dy):
        points, = ctx.saved_tensors
        dp = ctx.batch.point_gradient(points, dy=dy.contiguous(), lod=ctx.lod)[1]
        return (dp.sum(0) if points.dim() == 2 else dp), None, None


class _BatchTrainPointsFunction(torch.autograd.Function):
    """``HashGridFieldBatch.train_points_grad`` as a differentiable op of the points (``train_points_differentiable``): the forward trains
    the fields and keeps d loss_b / d points, the backward hands upstream[b] * dpoints[b] to the points (summed over the fields for shared
    [N, dim] points)"""

    @staticmethod
    def forward(ctx, points, batch, target, kwargs):
        loss, dp = batch.train_points_grad(points.detach(), target, **kwargs)
        ctx.save_for_backward(dp)
        ctx.shared = points.dim() == 2
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        dp, = ctx.saved_tensors
        out = g.reshape(-1, 1, 1) * dp
        return (out.sum(0) if ctx.shared else out), None, None, None


def _batch_lod_grad(dlod: torch.Tensor, shape, dtype) -> torch.Tensor:
    """the [B, N] gradient for the level of detail as the gradient of the ``lod`` the caller gave: itself for [B, N], summed over the fields
    for a shared [N], summed over everything for a 0-dim tensor"""
    g = dlod if len(shape) == 2 else dlod.sum(0) if len(shape) == 1 else dlod.sum()
    return g.to(dtype).reshape(shape)


class _BatchQueryPointsLodFunction(torch.autograd.Function):
    """``HashGridFieldBatch.query_lod`` as a differentiable op of the points and of the level of detail (``query_differentiable_lod``):
    backward = ``point_gradient_lod`` with the output gradient - ``dpoints`` summed over the fields for shared [N, dim] points, ``dlod`` for
    a [B, N] ``lod``, its sum over the fields for a shared [N] one, over everything for a 0-dim one; nothing for the fields' parameters"""

    @staticmethod
    def forward(ctx, points, lod, batch):
        ctx.batch = batch
        ctx.lod = None if isinstance(lod, torch.Tensor) else lod
        ctx.save_for_backward(points, *([lod] if isinstance(lod, torch.Tensor) else []))
        return batch.query_lod(points, lod)

    @staticmethod
    def backward(ctx, dy):
        points, *rest = ctx.saved_tensors
        lod = rest[0] if rest else ctx.lod
        _, dp, dl = ctx.batch.point_gradient_lod(points, lod, dy=dy.contiguous())
        glod = _batch_lod_grad(dl, lod.shape, lod.dtype) if rest and ctx.needs_input_grad[1] else None
        return ((dp.sum(0) if points.dim() == 2 else dp) if ctx.needs_input_grad[0] else None), glod, None


class _BatchTrainPointsLodFunction(torch.autograd.Function):
    """``HashGridFieldBatch.train_points_grad_lod`` as a differentiable op of the points and of the level of detail
    (``train_points_differentiable_lod``): the forward trains the fields and keeps d loss_b / d points and d loss_b / d lambda, the backward
    hands upstream[b] * dpoints[b] and upstream[b] * dlod[b] to whichever requires a gradient, summed as the shapes say"""

    @staticmethod
    def forward(ctx, points, lod, batch, target, kwargs):
        loss, dp, dl = batch.train_points_grad_lod(points.detach(), target, lod.detach() if isinstance(lod, torch.Tensor) else lod, **kwargs)
        ctx.lod_shape = (lod.shape, lod.dtype) if isinstance(lod, torch.Tensor) else None
        ctx.shared = points.dim() == 2
        ctx.save_for_backward(dp, dl)
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        dp, dl = ctx.saved_tensors
        gp = glod = None
        if ctx.needs_input_grad[0]:
            gp = g.reshape(-1, 1, 1) * dp
            gp = gp.sum(0) if ctx.shared else gp
        if ctx.lod_shape is not None and ctx.needs_input_grad[1]:
            glod = _batch_lod_grad(g.reshape(-1, 1) * dl, *ctx.lod_shape)
        return gp, glod, None, None, None


def _table_of_u8(geo: HashGeometry, stored: torch.Tensor, num_bits: int) -> torch.Tensor:
    """the fp32 [L, T, F] table a compact uint8 one stores (load4fp per level; the entries a dense level cannot address stay zero) - the input
    ``hash_pack_bits`` takes when a uint8 file is re-saved packed; save4fp of these values gives the bytes back"""
    table = torch.zeros(geo.table_shape(), dtype=torch.float32, device=stored.device)
    off = 0
    for l, r in enumerate(geo.resolutions):
        e = min((int(r) + 1) ** geo.dim, geo.table_size)
        table[l, :e] = models.load4fp(stored[off:off + e * geo.features], num_bits).reshape(e, geo.features)
        off += e * geo.features
    return table


COMPRESSED_FORMAT = "nicv2-hashgrid-u8/1"
PACKED_FORMAT = "nicv2-hashgrid-bits/1"          # the same dict with the bit-packed table (include/nicv2_hip.h, nic_hash_pack_bits)
MIXED_FORMAT = "nicv2-hashgrid-bits/2"           # format /1 with "level_bits": a depth per level (nic_hash_pack_bits_levels); "num_bits" is None


class HashGridField:
    """a hash-grid table + one decoder over its [N, L F] encoding, trained like ``MultiLevelField`` (module docstring).  ``field_size``:
    (S_x, S_y) or (S_x, S_y, S_z), x = the image tensor's first spatial axis like everywhere in this package.  ``num_bits``: None = no codec
    (no noise, no clamp); b in 1..8 = quantisation-aware training for a uint8 table of b-bit values (module docstring), noise keyed by
    ``noise_seed``; a sequence of ``levels`` depths = a bit depth per level (``level_bits`` holds the tuple, ``num_bits`` stays None).  ``fused``: ``train_step`` / ``fit`` / ``decode`` on the fused encode + decoder kernels where they exist (``route``)."""

    level_bits: Optional[Tuple[int, ...]] = None     # a bit depth per level (None: an int ``num_bits`` field, or no codec)
    _lod_fade: Optional[Tuple[float, ...]] = None    # the fade start per level given at construction (None: ``hash_lod_fade`` of the geometry)

    def __init__(self, field_size: Union[int, Sequence[int]], levels: int = 16, features: int = 2, log2_table: int = 19, base_resolution: float = 16,
                 finest_resolution: Optional[float] = None, hidden: int = 64, n_linear: int = 3, device=None, seed: Optional[int] = None,
                 num_bits: Union[None, int, Sequence[int]] = None, noise_seed: int = 7, fused: bool = False,
                 lod_fade: Optional[Sequence[float]] = None):
        level_bits = None
        if _is_level_bits(num_bits):
            level_bits, num_bits = _check_level_bits(levels, num_bits), None
        if num_bits is not None and not 1 <= int(num_bits) <= 8:
            raise ValueError("num_bits in 1 .. 8 (the stored table is uint8), or None")
        self.field_size = (int(field_size),) * 2 if isinstance(field_size, int) else tuple(int(v) for v in field_size)
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("HashGridField needs a HIP device: there is no CPU implementation of this path")
        n_max = max(self.field_size) if finest_resolution is None else finest_resolution
        self.geo = HashGeometry(self.field_size, tuple(level_resolutions(levels, base_resolution, n_max)), features, log2_table)
        self._lod_fade = None if lod_fade is None else _check_fade(self.geo.levels, lod_fade)
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
        self.hidden, self.n_linear = int(hidden), int(n_linear)
        self.num_bits = None if num_bits is None else int(num_bits)
        self.level_bits = level_bits
        self.noise_seed, self.steps, self.frozen, self.stored, self.packed = int(noise_seed), 0, False, None, None
        self._pass_samples = 0                       # samples of the current accumulate pass so far: the next chunk's sample_base
        self._set_route(fused)
        if self.num_bits is not None:
            self.optimizer.set_clamp([self.table], *models._q_range(self.num_bits))
        if self.level_bits is not None:              # the optimiser's one clamp is the widest range; _clamp_levels tightens the rest
            self.optimizer.set_clamp([self.table], *models._q_range(max(self.level_bits)))

    @property
    def lod_fade(self) -> Tuple[float, ...]:
        """the fade start of every level for ``lod=`` calls: the constructor's ``lod_fade``, else ``hash_lod_fade(geo)``"""
        return self._lod_fade if self._lod_fade is not None else hash_lod_fade(self.geo)

    def _lod_args(self, lod) -> Tuple[Optional[torch.Tensor], float]:
        """``lod`` of a call (a finite float, or a tensor with one value per point) as (per-point tensor or None, launch-wide value); the
        tensor is checked against the points by ``_check_lod``"""
        if self.level_bits is not None:
            raise NotImplementedError("a level of detail with a bit depth per level is not built (DESIGN 7): use a uniform num_bits")
        if isinstance(lod, torch.Tensor) and lod.dim() > 0:
            return lod, 0.0
        try:
            v = float(lod)
        except (TypeError, ValueError):
            raise ValueError(f"lod is a float or a [N] tensor, got {lod!r}") from None
        if not math.isfinite(v):
            raise ValueError(f"lod {lod!r} is not finite")
        return None, v

    @property
    def _codec(self) -> bool:
        return self.num_bits is not None or self.level_bits is not None

    def _clamp_levels(self) -> None:
        """after an optimiser step of a mixed-depth field: the levels below the widest depth into their own range (one launch; none when all
        depths are equal)"""
        if self.level_bits is not None and not self.frozen and len(set(self.level_bits)) > 1:
            hash_clamp_levels(self.geo, self.table.detach(), self.level_bits)

    def _set_route(self, want_fused: bool) -> None:
        """"fused" when asked for and the kernels exist for this shape, else "layerwise" (a field built without ``fused`` never asks the library)"""
        self.route = "fused" if want_fused and hash_fused_supported(self.geo, self.hidden, self.n_linear) else "layerwise"
        self._fused_gm = None                        # the decoder-gradient buffers of the fused step: persistent, so the optimiser's table stays valid

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

    def train_step(self, coord, extent: Sequence[int], target: torch.Tensor, accumulate: bool = False, scale: float = 1.0, step: bool = True,
                   noise: Optional[bool] = None) -> torch.Tensor:
        """one step on the crops at ``coord`` with targets [N, 3].  ``accumulate`` / ``scale`` / ``step``: a whole-field pass walked in chunks -
        gradients add up over the chunks (each chunk's MSE scaled by its share), one optimiser step at the end.  ``noise``: None = on while a
        ``num_bits`` field's table trains (offset = the optimiser step count, sample_base = the samples of this pass before this chunk, so no two
        chunks of a pass share noise).  After ``freeze()`` only the decoder trains: no table gradient is formed."""
        if self.table is None:
            raise RuntimeError("a field from load_compressed decodes only")
        if self.route == "fused":
            return self._fused_train_step(coord, extent, target, accumulate, scale, step, noise)
        params = self.decoder.linear_params()
        grad = self.table.grad
        frozen = self.frozen
        if not accumulate:
            for p in params:
                p.grad = None
            if not frozen and not self._grad_clean:
                grad.zero_()
            self._pass_samples = 0
        org = self.geo.upload_origins(coord, extent, self.device)
        n = _n_samples(org.shape[0], extent)
        if tuple(target.shape) != (n, 3):
            raise ValueError(f"target must be [{n}, 3], got {tuple(target.shape)}")
        if noise is None:
            noise = self._codec and not frozen
        if noise and not self._codec:
            raise ValueError("noise needs num_bits: its amplitude is one quantisation step")
        if noise and self.level_bits is not None:
            x = hash_encode_levels(self.geo, self.table, self.level_bits, coord=org, extent=extent, quant=(self.noise_seed, self.steps, self._pass_samples))
        elif noise:
            x = hash_encode_noisy(self.geo, self.table, org, extent, self.num_bits, self.noise_seed, self.steps, self._pass_samples)
        else:
            x = hash_encode(self.geo, self.table, org, extent)
        self._pass_samples += n
        if not frozen:
            x.requires_grad_(True)
        y = fused.DecoderFunction.apply(x, *params)
        loss = ((y - target) ** 2).mean() * scale
        loss.backward()
        if not frozen:
            hash_encode_backward(self.geo, org, extent, x.grad, grad)
            self._grad_clean = False
        if step:
            self.optimizer.step()
            self._clamp_levels()
            if not frozen:
                self._grad_clean = self.optimizer.zeroed_in_last_step(grad)
            if self.scheduler is not None:
                self.scheduler.step()
            self.steps += 1
        return loss.detach()

    def train_points(self, points: torch.Tensor, target: torch.Tensor, accumulate: bool = False, scale: float = 1.0, step: bool = True,
                     noise: Optional[bool] = None, order=None, fused: bool = False, lod=None, dpoints: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``train_step`` on samples that are no raster: ``points`` [N, dim] (fp32, sample units, any order) with their colours ``target``
        [N, 3].  ``accumulate`` / ``scale`` / ``step`` / ``noise``, the noise keys (seed, optimiser step, samples of this pass before this
        chunk + row), the freeze behaviour and the optimiser bookkeeping are ``train_step``'s.  By default the call is layer-wise and unordered
        on either route: on a crop's sample centres in raster order it differs from ``train_step`` in the order of the gradient atomics only.
        ``order``: None, "cell" (``hash_point_order`` of these points, computed for this call) or an int32 [N] device tensor (a precomputed
        ``hash_point_order``, reused across steps for a fixed point set) - the launch walks the points in that order so that neighbouring
        lanes share their cells; rows, targets and noise keys stay the caller's.  ``fused``: the fused step at points (two launches,
        ``nic_hash_fused_forward_backward_points``) - needs ``route == "fused"``.  ``lod``: None (the calls above, unchanged), or a level of
        detail for these samples - a float, or one value per point [N] - which fades the finer levels out of the row and of its gradient
        (the ``_lod`` entry points, fade starts ``lod_fade``).  ``dpoints``: None (exactly the calls above), or an fp32
        [N, dim] contiguous device tensor that the call OVERWRITES with d loss / d points of the loss it returns: the
        derivative ``point_gradient(points, target=, scale=)`` gives, taken at the parameters this step's forward used (before the optimiser
        moves them), noise and level weights constant - registration while fitting, in the step's own launches (``fused=True``:
        nic_hash_fused_forward_backward_points_grad; layer-wise: nic_hash_encode_points_grad on the row gradient the step has anyway, also
        after ``freeze()``).  Each chunk of an ``accumulate`` pass fills its own ``dpoints``."""
        return self._train_points(points, target, accumulate, scale, step, noise, order, fused, lod, dpoints, None)

    def train_points_grad_lod(self, points: torch.Tensor, target: torch.Tensor, lod, dpoints: Optional[torch.Tensor] = None,
                              dlod: Optional[torch.Tensor] = None, accumulate: bool = False, scale: float = 1.0, step: bool = True,
                              noise: Optional[bool] = None, order=None, fused: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(loss, dpoints [N, dim], dlod [N]): ``train_points(points, target, lod=lod, dpoints=...)`` that also fills ``dlod`` with d loss / d
        lambda_n of the loss it returns, taken like ``dpoints`` at the parameters this step's forward used, in the step's own
        launches - for a level of detail that comes from parameters optimised while the field is fitted (a zoom ``lambda = log2 s + bias``, a
        mip bias per view).  ``lod`` is required: a float, a 0-dim tensor or one value per point [N]; the gradient for a launch-wide value is
        ``dlod.sum()``.  ``dlod[n]`` = - sum over the levels on the ramp (0 < (fade[l] - lambda_n) + 1 <= 1, the right-hand derivative) of
        sum_f g[n, l F + f] (r[n, l, f] + nz[n, l F + f]): with a codec the step's forward adds its noise INSIDE the weighed column, and the
        slope counts it - ``point_gradient_lod(target=)`` in front of the step cannot.  Exactly 0 where lambda_n < 0, >= 32 or NaN.
        ``dpoints`` / ``dlod``: None for fresh tensors, or fp32 contiguous device tensors [N, dim] / [N] that are OVERWRITTEN.  ``fused=True``:
        nic_hash_fused_forward_backward_points_grad_lod inside ``train_points``' bookkeeping; layer-wise:
        nic_hash_encode_points_grad_lod_noisy on the row gradient the step has anyway, with the step's noise key, before the optimiser moves
        the table, also after ``freeze()``.  Everything else - ``accumulate`` / ``scale`` / ``step`` / ``noise`` / ``order``, the noise keys
        of a chunked pass - is ``train_points``'."""
        if self.table is None:
            raise RuntimeError("a field from load_compressed decodes only")
        if self.level_bits is not None:
            raise NotImplementedError("gradients with respect to the level of detail with a bit depth per level are not built (DESIGN 7): use a "
                                      "uniform num_bits")
        if lod is None:
            raise ValueError("lod is a float or a [N] tensor: the level of detail the gradient is taken at")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != self.geo.dim:
            raise ValueError(f"points must be [N, {self.geo.dim}] for a {self.geo.dim}D field, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
        # the two tensors: type, shape, dtype and layout of both, then where they live
        if dlod is not None:
            _check_dlod(points, dlod, device=False)
        if dpoints is not None:
            dpoints = _check_dpoints(self.geo, points, dpoints)
        if dlod is not None:
            dlod = _check_dlod(points, dlod)
        if not points.is_cuda:
            raise RuntimeError(f"points live on {points.device}: this package only runs on a HIP device (no CPU path)")
        if dpoints is None:
            dpoints = torch.empty(points.shape[0], self.geo.dim, dtype=torch.float32, device=points.device)
        if dlod is None:
            dlod = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
        loss = self._train_points(points, target, accumulate, scale, step, noise, order, fused, lod, dpoints, dlod)
        return loss, dpoints, dlod

    def train_points_weighted(self, points: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, lod=None,
                              dpoints: Optional[torch.Tensor] = None, dlod: Optional[torch.Tensor] = None, accumulate: bool = False,
                              scale: float = 1.0, step: bool = True, noise: Optional[bool] = None, order=None, fused: bool = False) -> torch.Tensor:
        """``train_points`` with a weight per point in the loss: loss = ``scale`` sum_n w_n sum_o (y[n, o] - target[n, o])^2 /
        (3 N), w_n = ``weight[n]`` where that is > 0 and 0 elsewhere (NaN and negative values count 0; +inf is the caller's error), N the
        number of points - NOT the sum of the weights: ones are ``train_points``, importance weights 1 / (N p_n) go in as they are, a mask or a
        confidence is the weight itself, and a caller who wants the weighted mean divides the weights by their mean.  ``weight``: fp32 [N]
        on the points' device, contiguous, at the caller's rows like ``target`` whatever the ``order``.  Every gradient is that loss's: a
        point of weight 0 still costs its gathers, and adds nothing to the table, the decoder or the loss.  ``lod``: ``train_points``'.
        ``dpoints`` / ``dlod``: None, or fp32 [N, dim] / [N] contiguous device tensors that are OVERWRITTEN with d loss / d points and d
        loss / d lambda of the loss returned (``train_points_grad_lod``'s conventions, each row carrying its w_n; exactly 0 at weight 0);
        ``dlod`` needs ``lod`` and ``dpoints``.  ``fused=True``: nic_hash_fused_forward_backward_points_weighted; layer-wise: the existing
        kernels on the row gradient of the weighted loss.  ``accumulate`` / ``scale`` / ``step`` / ``noise`` / ``order``, the noise keys
        of a chunked pass and the optimiser bookkeeping are ``train_points``'.  Returns the loss."""
        if self.table is None:
            raise RuntimeError("a field from load_compressed decodes only")
        if self.level_bits is not None:
            raise NotImplementedError("loss weights with a bit depth per level are not built (DESIGN 7): use a uniform num_bits")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != self.geo.dim:
            raise ValueError(f"points must be [N, {self.geo.dim}] for a {self.geo.dim}D field, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
        if dlod is not None and lod is None:
            raise ValueError("dlod needs lod: the level of detail the gradient is taken at")
        if dlod is not None and dpoints is None:
            raise ValueError("dlod needs dpoints: both gradients come from one walk of the levels")
        if dlod is not None:
            _check_dlod(points, dlod, device=False)
        weight = _check_weight(points, weight)
        if dpoints is not None:
            dpoints = _check_dpoints(self.geo, points, dpoints)
        if dlod is not None:
            dlod = _check_dlod(points, dlod)
        return self._train_points(points, target, accumulate, scale, step, noise, order, fused, lod, dpoints, dlod, weight)

    def train_points_weighted_differentiable(self, points: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, lod=None, **kwargs) -> torch.Tensor:
        """``train_points_weighted(points, target, weight, lod=lod, **kwargs)`` as a differentiable op of ``points`` and / or ``lod`` (a [N]
        tensor, or a 0-dim tensor whose gradient is the sum of the per-point ones), built like ``train_points_differentiable_lod``: the call
        steps the field as it always does, and the loss it returns has a backward that hands upstream * d loss / d points and upstream * d
        loss / d lambda to whichever requires a gradient.  ``weight`` gets no gradient, and none reaches the field's parameters through
        autograd.  With nothing that requires one, or under ``torch.no_grad()``, it is plain ``train_points_weighted``."""
        if "dpoints" in kwargs or "dlod" in kwargs:
            raise TypeError("train_points_weighted_differentiable keeps dpoints and dlod for the backward: call train_points_weighted for the tensors")
        wants = any(isinstance(t, torch.Tensor) and t.requires_grad for t in (points, lod))
        if not (wants and torch.is_grad_enabled()):
            return self.train_points_weighted(points, target, weight, lod=lod, **kwargs)
        return _TrainPointsWeightedFunction.apply(points, lod, self, target, weight, kwargs)

    def _train_points(self, points, target, accumulate, scale, step, noise, order, fused, lod, dpoints, dlod, weight=None) -> torch.Tensor:
        """``train_points`` (``dlod`` None) and ``train_points_grad_lod`` (``dlod`` a checked [N] tensor; ``lod`` and ``dpoints`` are then given);
        ``weight``: None, or the checked [N] loss weights of ``train_points_weighted``"""
        if self.table is None:
            raise RuntimeError("a field from load_compressed decodes only")
        if dpoints is not None:
            if self.level_bits is not None:
                raise NotImplementedError("gradients with respect to the points with a bit depth per level are not built (DESIGN 7): use a uniform num_bits")
            dpoints = _check_dpoints(self.geo, points, dpoints)
        lod_t, lod_u = (None, 0.0) if lod is None else self._lod_args(lod)
        params = self.decoder.linear_params()
        grad = self.table.grad
        frozen = self.frozen
        # every check comes before the first write: a refused call leaves an accumulate pass as it was
        pts = _check_points(self.geo, points)
        n = pts.shape[0]
        lod_t = _check_lod(lod_t, n, pts.device)
        if n < 1:
            raise ValueError("no points")
        if tuple(target.shape) != (n, 3):
            raise ValueError(f"target must be [{n}, 3], got {tuple(target.shape)}")
        if noise is None:
            noise = self._codec and not frozen
        if noise and not self._codec:
            raise ValueError("noise needs num_bits: its amplitude is one quantisation step")
        _point_desc(self.geo)
        if fused and self.route != "fused":
            raise ValueError(f"fused=True on a field whose route is {self.route!r}: build it with fused=True (and a shape nic_hash_fused_supported takes)")
        if order is not None and not (isinstance(order, str) and order == "cell"):
            order = _check_order(order, n, pts.device)
        if fused:
            target = _lib.require_cuda_f32(target, "target")
        if isinstance(order, str):
            order = hash_point_order(self.geo, pts)
        if fused:
            return self._fused_train_points(pts, target, accumulate, scale, step, noise, order, None if lod is None else (lod_t, lod_u), dpoints, dlod,
                                            weight)
        if not accumulate:
            for p in params:
                p.grad = None
            if not frozen and not self._grad_clean:
                grad.zero_()
            self._pass_samples = 0
        quant = (self.num_bits, self.noise_seed, self.steps, self._pass_samples) if noise else None
        if lod is not None:
            x = hash_encode_points_lod(self.geo, self.table, pts, lod_t, lod_u, self.lod_fade, quant=quant)
        elif noise and self.level_bits is not None:
            x = hash_encode_levels(self.geo, self.table, self.level_bits, points=pts, quant=quant[1:])
        else:
            x = hash_encode_points(self.geo, self.table, pts, quant=quant)
        self._pass_samples += n
        if not frozen or dpoints is not None:
            x.requires_grad_(True)
        y = DecoderFunction.apply(x, *params)          # `fused` is this call's argument here
        if weight is None:
            loss = ((y - target) ** 2).mean() * scale
        else:                                          # sum_n w_n sum_o e^2 / (3 N): the mean of the weighed squares, the plain expression at w = 1
            w = torch.where(weight > 0, weight, torch.zeros_like(weight))
            loss = (w[:, None] * (y - target) ** 2).mean() * scale
        loss.backward()
        if dlod is not None:                           # both gradients from one walk, with the noise this forward added
            dp, dl = hash_encode_points_grad_lod_noisy(self.geo, self.table, pts, x.grad, lod_t, lod_u, self.lod_fade, quant=quant)
            dpoints.copy_(dp)
            dlod.copy_(dl)
        elif dpoints is not None:                      # before the optimiser moves the table: the derivative at the forward's parameters
            dpoints.copy_(hash_encode_points_grad(self.geo, self.table, pts, x.grad, lod=lod_t, lod_uniform=lod_u,
                                                  fade=None if lod is None else self.lod_fade))
        if not frozen and lod is not None:
            hash_encode_points_backward_lod(self.geo, pts, x.grad, grad, lod_t, lod_u, self.lod_fade, order=order)
        elif not frozen:
            hash_encode_points_backward(self.geo, pts, x.grad, grad, order=order)
        if not frozen:
            self._grad_clean = False
        if step:
            self.optimizer.step()
            self._clamp_levels()
            if not frozen:
                self._grad_clean = self.optimizer.zeroed_in_last_step(grad)
            if self.scheduler is not None:
                self.scheduler.step()
            self.steps += 1
        return loss.detach()

    @torch.no_grad()
    def _fused_train_points(self, pts, target, accumulate, scale, step, noise, order, lod=None, dpoints=None, dlod=None, weight=None) -> torch.Tensor:
        """``train_points`` as two launches, with ``_fused_train_step``'s bookkeeping: persistent decoder-gradient buffers, the chunks of a
        pass adding into them and into the table gradient, the optimiser riding on the last chunk's reduction.  The arguments are checked.
        ``lod``: None or (per-point tensor or None, launch-wide value).  ``dpoints``: None, or the tensor the joint entry overwrites;
        ``dlod`` (with ``lod`` and ``dpoints``): the tensor the entry with the gradient for the level of detail overwrites.  ``weight``: None,
        or the [N] loss weights - then every combination of the rest is the weighted entry's."""
        params = self.decoder.linear_params()
        frozen = self.frozen
        grad = None if frozen else self.table.grad
        if self._fused_gm is None:
            self._fused_gm = [torch.zeros_like(p) for p in params]
        gm = self._fused_gm
        for p, g in zip(params, gm):
            p.grad = g
        if not accumulate:
            if not frozen and not self._grad_clean:
                grad.zero_()
            self._pass_samples = 0
        quant = (self.num_bits, self.noise_seed, self.steps, self._pass_samples) if noise else None
        tail = None
        if step:
            tail = self.optimizer.step_tail([] if frozen else [(self.table, grad)], list(zip(params, gm)))
        if weight is not None:
            loss, _, _, _ = hash_fused_forward_backward_points_weighted(self.geo, self.table, pts, params, target, weight, gm,
                                                                        *((None, 0.0, None) if lod is None else (lod[0], lod[1], self.lod_fade)),
                                                                        table_grad=grad, order=order, loss_scale=float(scale), quant=quant,
                                                                        add_grads=accumulate, tail=tail, dpoints=dpoints, dlod=dlod)
        elif dlod is not None:
            loss, _, _, _ = hash_fused_forward_backward_points_grad_lod(self.geo, self.table, pts, params, target, gm, lod[0], lod[1], self.lod_fade,
                                                                        table_grad=grad, order=order, loss_scale=float(scale), quant=quant,
                                                                        add_grads=accumulate, tail=tail, dpoints=dpoints, dlod=dlod)
        elif dpoints is not None:
            loss, _, _ = hash_fused_forward_backward_points_grad(self.geo, self.table, pts, params, target, gm, *((None, 0.0, None) if lod is None else
                                                                 (lod[0], lod[1], self.lod_fade)), table_grad=grad, order=order,
                                                                 loss_scale=float(scale), quant=quant, add_grads=accumulate, tail=tail, dpoints=dpoints)
        elif lod is not None:
            loss, _ = hash_fused_forward_backward_points_lod(self.geo, self.table, pts, params, target, gm, lod[0], lod[1], self.lod_fade,
                                                             table_grad=grad, order=order, loss_scale=float(scale), quant=quant,
                                                             add_grads=accumulate, tail=tail)
        elif self.level_bits is not None:
            loss, _ = hash_fused_forward_backward_levels(self.geo, self.table, self.level_bits, params, target, gm, points=pts, order=order,
                                                         table_grad=grad, loss_scale=float(scale), quant=None if quant is None else quant[1:],
                                                         add_grads=accumulate, tail=tail)
        else:
            loss, _ = hash_fused_forward_backward_points(self.geo, self.table, pts, params, target, gm, table_grad=grad, order=order,
                                                         loss_scale=float(scale), quant=quant, add_grads=accumulate, tail=tail)
        self._pass_samples += pts.shape[0]
        if not frozen:
            self._grad_clean = False
        if step:
            self.optimizer.step()                    # nothing to launch after a committed tail
            self._clamp_levels()
            if not frozen:
                self._grad_clean = self.optimizer.zeroed_in_last_step(grad)
            if self.scheduler is not None:
                self.scheduler.step()
            self.steps += 1
        return loss

    def train_points_differentiable(self, points: torch.Tensor, target: torch.Tensor, **kwargs) -> torch.Tensor:
        """``train_points(points, target, **kwargs)`` as a differentiable op of ``points``: the call steps the field as it
        always does, and the loss it returns has a backward that hands upstream * d loss / d points to ``points`` - so with
        ``loss = f.train_points_differentiable(warp(theta, p0), target, fused=True, order="cell"); loss.backward(); pose_opt.step()`` the
        field steps inside the call and the warp outside it, from one forward.  No gradient reaches the field's parameters through autograd:
        their step is the call's own.  Without ``points.requires_grad``, or under ``torch.no_grad()``, it is plain ``train_points``."""
        if "dpoints" in kwargs:
            raise TypeError("train_points_differentiable keeps dpoints for the backward: call train_points(dpoints=) for the tensor itself")
        if not (isinstance(points, torch.Tensor) and points.requires_grad and torch.is_grad_enabled()):
            return self.train_points(points, target, **kwargs)
        return _TrainPointsFunction.apply(points, self, target, kwargs)

    def train_points_differentiable_lod(self, points: torch.Tensor, lod, target: torch.Tensor, **kwargs) -> torch.Tensor:
        """``train_points(points, target, lod=lod, **kwargs)`` as a differentiable op of ``points`` and / or ``lod`` - ``lod`` a
        [N] tensor, or a 0-dim tensor (one level of detail for the launch, whose gradient is the sum of the per-point ones): the call steps
        the field as it always does, and the loss it returns has a backward that hands upstream * d loss / d points and upstream * d loss / d
        lambda (``train_points_grad_lod``'s, the step's noise counted) to whichever requires a gradient.  With nothing that requires one, or
        under ``torch.no_grad()``, it is plain ``train_points``.  No gradient reaches the field's parameters through autograd."""
        if "dpoints" in kwargs or "dlod" in kwargs:
            raise TypeError("train_points_differentiable_lod keeps dpoints and dlod for the backward: call train_points_grad_lod for the tensors")
        wants = any(isinstance(t, torch.Tensor) and t.requires_grad for t in (points, lod))
        if not (wants and torch.is_grad_enabled()):
            return self.train_points(points, target, lod=lod, **kwargs)
        return _TrainPointsLodFunction.apply(points, lod, self, target, kwargs)

    def fit_points(self, points: torch.Tensor, target: torch.Tensor, epochs: int, batch: Optional[int] = None, order="cell",
                   fused: Optional[bool] = None, freeze_at: float = 0.95, lod=None) -> List[float]:
        """``fit`` for a fixed sample set: ``epochs`` passes over ``points`` [N, dim] with colours ``target`` [N, 3], one optimiser step per
        pass.  ``order``: "cell" (default), None or an int32 [N] device tensor; it is computed once and the set is laid out in that order, so
        every pass walks it in ``batch``-sized accumulate chunks that are contiguous ranges of the order - each chunk spatially compact (None:
        the whole set in one call).  ``fused``: None = the field's route.  With ``num_bits``: noise while the epoch is below ``freeze_at`` *
        epochs, then ``freeze()``.  ``lod``: ``train_points``' (a [N] tensor is laid out and cut with the points).  Returns the per-pass losses."""
        return self._fit_points(points, target, epochs, batch, order, fused, freeze_at, lod, None)

    def fit_points_weighted(self, points: torch.Tensor, target: torch.Tensor, weight: torch.Tensor, epochs: int, batch: Optional[int] = None,
                            order="cell", fused: Optional[bool] = None, freeze_at: float = 0.95, lod=None) -> List[float]:
        """``fit_points`` with ``train_points_weighted``'s loss weights: ``weight`` fp32 [N] on the device, laid out and cut
        with the points.  A chunk's ``scale`` stays its share of the points by COUNT, so the pass loss is sum_n w_n sum_o e^2 / (3 N) over
        the whole set and ones reproduce ``fit_points``.  Returns the per-pass losses."""
        if self.table is None:
            raise RuntimeError("a field from load_compressed decodes only")
        if self.level_bits is not None:
            raise NotImplementedError("loss weights with a bit depth per level are not built (DESIGN 7): use a uniform num_bits")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != self.geo.dim:
            raise ValueError(f"points must be [N, {self.geo.dim}] for a {self.geo.dim}D field, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
        return self._fit_points(points, target, epochs, batch, order, fused, freeze_at, lod, _check_weight(points, weight))

    def _fit_points(self, points, target, epochs, batch, order, fused, freeze_at, lod, weight) -> List[float]:
        """``fit_points`` (``weight`` None) and ``fit_points_weighted`` (``weight`` the checked [N] tensor)"""
        lod_t, lod_u = (None, None) if lod is None else self._lod_args(lod)
        pts = _check_points(self.geo, points)
        n = pts.shape[0]
        if n < 1:
            raise ValueError("no points")
        target = _lib.require_cuda_f32(target, "target")
        if tuple(target.shape) != (n, 3):
            raise ValueError(f"target must be [{n}, 3], got {tuple(target.shape)}")
        lod_t = _check_lod(lod_t, n, pts.device)
        fused = self.route == "fused" if fused is None else bool(fused)
        if fused and self.route != "fused":
            raise ValueError(f"fused=True on a field whose route is {self.route!r}")
        batch = n if batch is None else int(batch)
        if batch < 1:
            raise ValueError("batch >= 1")
        if order is not None:
            idx = hash_point_order(self.geo, pts) if isinstance(order, str) and order == "cell" else _check_order(order, n, pts.device)
            idx = idx.to(torch.int64).clamp_(0, n - 1)
            pts, target = pts[idx].contiguous(), target[idx].contiguous()       # laid out in the order once: a chunk is a slice
            lod_t = None if lod_t is None else lod_t[idx].contiguous()
            weight = None if weight is None else weight[idx].contiguous()
        cuts = list(range(0, n, batch))
        freeze_epoch = math.ceil(freeze_at * epochs) if self._codec else None
        hist = []
        for ep in range(epochs):
            if freeze_epoch is not None and ep >= freeze_epoch and not self.frozen:
                self.freeze()
            tot = 0.0
            for k, c0 in enumerate(cuts):
                c1 = min(c0 + batch, n)
                how = dict(accumulate=k > 0, scale=(c1 - c0) / n, step=k == len(cuts) - 1, fused=fused, lod=lod_u if lod_t is None else lod_t[c0:c1])
                if weight is None:
                    tot = tot + self.train_points(pts[c0:c1], target[c0:c1], **how)
                else:
                    tot = tot + self.train_points_weighted(pts[c0:c1], target[c0:c1], weight[c0:c1], **how)
            hist.append(tot)
        return [float(h) for h in hist]

    @torch.no_grad()
    def _fused_train_step(self, coord, extent, target, accumulate, scale, step, noise) -> torch.Tensor:
        """``train_step`` as two launches: the fused kernel, then the reduction of its decoder-gradient records with the optimiser riding on it
        (``FusedAdam.step_tail``).  The decoder gradients live in persistent buffers; the chunks of a pass add into them and into the table
        gradient, and only the last chunk carries the optimiser."""
        params = self.decoder.linear_params()
        frozen = self.frozen
        grad = None if frozen else self.table.grad
        if self._fused_gm is None:
            self._fused_gm = [torch.zeros_like(p) for p in params]
        gm = self._fused_gm
        for p, g in zip(params, gm):
            p.grad = g
        if not accumulate:
            if not frozen and not self._grad_clean:
                grad.zero_()
            self._pass_samples = 0
        org = self.geo.upload_origins(coord, extent, self.device)
        n = _n_samples(org.shape[0], extent)
        if noise is None:
            noise = self._codec and not frozen
        if noise and not self._codec:
            raise ValueError("noise needs num_bits: its amplitude is one quantisation step")
        quant = (self.num_bits, self.noise_seed, self.steps, self._pass_samples) if noise else None
        tail = None
        if step:
            tail = self.optimizer.step_tail([] if frozen else [(self.table, grad)], list(zip(params, gm)))
        if self.level_bits is not None:
            loss, _ = hash_fused_forward_backward_levels(self.geo, self.table, self.level_bits, params, target, gm, coord=org, extent=extent,
                                                         table_grad=grad, loss_scale=float(scale), quant=None if quant is None else quant[1:],
                                                         add_grads=accumulate, tail=tail)
        else:
            loss, _ = hash_fused_forward_backward(self.geo, self.table, org, extent, params, target, gm, table_grad=grad, loss_scale=float(scale),
                                                  quant=quant, add_grads=accumulate, tail=tail)
        self._pass_samples += n
        if not frozen:
            self._grad_clean = False
        if step:
            self.optimizer.step()                    # nothing to launch after a committed tail
            self._clamp_levels()
            if not frozen:
                self._grad_clean = self.optimizer.zeroed_in_last_step(grad)
            if self.scheduler is not None:
                self.scheduler.step()
            self.steps += 1
        return loss

    @torch.no_grad()
    def freeze(self) -> None:
        """quantise the table in place (nic_quantize) and stop updating it: ``train_step`` then trains the decoder alone, without noise
        (fp_freeze + fp_all_quantize of the dense codec)"""
        if not self._codec:
            raise RuntimeError("freeze() needs num_bits: there is no quantiser without it")
        if self.frozen:
            return
        t = self.table.detach()
        if self.level_bits is not None:              # each level's slice with its own depth
            for l, b in enumerate(self.level_bits):
                tl = t[l]
                _lib.check(_lib.load().nic_quantize(_lib.ptr(tl), _lib.ptr(tl), tl.numel(), b, _lib.stream_ptr(t.device)), "nic_quantize")
        else:
            _lib.check(_lib.load().nic_quantize(_lib.ptr(t), _lib.ptr(t), t.numel(), self.num_bits, _lib.stream_ptr(t.device)), "nic_quantize")
        self.table.grad = None                       # FusedAdam skips a parameter without a gradient
        self.table.requires_grad_(False)
        self.frozen = True

    def fit(self, target: torch.Tensor, epochs: int, chunk: Optional[int] = None, freeze_at: float = 0.95) -> List[float]:
        """``epochs`` whole-field passes on ``target`` [S_x, S_y(, S_z), 3], walked in slabs of ``chunk`` x-rows (one optimiser step per pass,
        each slab's MSE weighted by its share).  With ``num_bits``: noise while the epoch is below ``freeze_at`` * epochs, then ``freeze()``.
        Returns the per-pass losses."""
        size = self.field_size
        if tuple(target.shape) != (*size, 3):
            raise ValueError(f"target must be {(*size, 3)}, got {tuple(target.shape)}")
        chunk = size[0] if chunk is None else int(chunk)
        starts = list(range(0, size[0], chunk))
        slabs = [target[x0:x0 + chunk].reshape(-1, 3).contiguous() for x0 in starts]
        total = sum(s.shape[0] for s in slabs)
        freeze_epoch = math.ceil(freeze_at * epochs) if self._codec else None
        hist = []
        for ep in range(epochs):
            if freeze_epoch is not None and ep >= freeze_epoch and not self.frozen:
                self.freeze()
            tot = 0.0
            for k, x0 in enumerate(starts):
                ext = (min(chunk, size[0] - x0), *size[1:])
                tot = tot + self.train_step([[x0] + [0] * (len(size) - 1)], ext, slabs[k], accumulate=k > 0, scale=slabs[k].shape[0] / total,
                                            step=k == len(starts) - 1)
            hist.append(tot)
        return [float(h) for h in hist]

    def stored_bytes(self, packed: bool = False) -> dict:
        """bytes ``save_compressed`` stores: the compact uint8 table (``packed``: the bit-packed one) and the fp32 decoder"""
        if packed and not self._codec:
            raise RuntimeError("the packed size needs num_bits")
        if self.level_bits is not None and not packed:
            raise ValueError("a mixed-depth table has no uint8 form: stored_bytes(packed=True)")
        table = hash_packed_bytes(self.geo, self.level_bits if self.level_bits is not None else self.num_bits) if packed else hash_stored_bytes(self.geo)
        return {"table": table, "decoder": sum(v.numel() * v.element_size() for v in self.decoder.state_dict().values())}

    @torch.no_grad()
    def save_compressed(self, path, packed: bool = False) -> None:
        """one ``torch.save`` dict: format tag, geometry, num_bits, the compact uint8 table of a clamped copy of the table (``packed``: the
        bit-packed table, num_bits bits per value, under the tag ``nicv2-hashgrid-bits/1``), the decoder.  A decode-only field re-saves the table
        it holds, converted on the device when the other form is asked for."""
        if self.level_bits is not None:
            if not packed:
                raise ValueError("a mixed-depth table has no uint8 form: save_compressed(path, packed=True)")
            if self.table is not None:               # a per-level clamped copy; a decode-only field re-saves its buffer as it is
                stored = hash_pack_bits_levels(self.geo, hash_clamp_levels(self.geo, self.table.detach().clone(), self.level_bits), self.level_bits)
            else:
                stored = self.packed
            torch.save({"format": MIXED_FORMAT, "field_size": list(self.field_size), "resolutions": list(self.geo.resolutions),
                        "features": self.geo.features, "log2_table": self.geo.log2_table, "num_bits": None, "level_bits": list(self.level_bits),
                        "hidden": self.hidden, "n_linear": self.n_linear, "table": stored.cpu(),
                        "decoder": {k: v.detach().cpu() for k, v in self.decoder.state_dict().items()}}, path)
            return
        if self.num_bits is None:
            raise RuntimeError("save_compressed needs num_bits")
        if self.table is not None:
            clamped = models.quantize_clamp(self.table, self.num_bits)
            stored = hash_pack_bits(self.geo, clamped, self.num_bits) if packed else hash_pack_u8(self.geo, clamped, self.num_bits)
        elif packed:
            stored = self.packed if self.packed is not None else hash_pack_bits(self.geo, _table_of_u8(self.geo, self.stored, self.num_bits), self.num_bits)
        else:
            stored = self.stored if self.stored is not None else hash_unpack_bits(self.geo, self.packed, self.num_bits)
        torch.save({"format": PACKED_FORMAT if packed else COMPRESSED_FORMAT, "field_size": list(self.field_size), "resolutions": list(self.geo.resolutions),
                    "features": self.geo.features, "log2_table": self.geo.log2_table, "num_bits": self.num_bits, "hidden": self.hidden,
                    "n_linear": self.n_linear, "table": stored.cpu(), "decoder": {k: v.detach().cpu() for k, v in self.decoder.state_dict().items()}}, path)

    @classmethod
    def load_compressed(cls, path, device=None, fused: bool = False, lod_fade: Optional[Sequence[float]] = None) -> "HashGridField":
        """a decode-only field from ``save_compressed``'s file, either format: ``decode()`` gathers from the table as stored - uint8
        (nic_hash_encode_u8; ``fused``: nic_hash_fused_forward_u8) or bit-packed (nic_hash_encode_bits / nic_hash_fused_forward_bits) - with no
        fp32 table and no conversion between the two.  ``lod_fade``: the constructor's (the file does not hold it)."""
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or d.get("format") not in (COMPRESSED_FORMAT, PACKED_FORMAT, MIXED_FORMAT):
            raise ValueError(f"{path}: not a {COMPRESSED_FORMAT}, {PACKED_FORMAT} or {MIXED_FORMAT} file")
        is_mixed = d["format"] == MIXED_FORMAT
        is_packed = is_mixed or d["format"] == PACKED_FORMAT
        self = cls.__new__(cls)
        self.field_size = tuple(int(v) for v in d["field_size"])
        self.geo = HashGeometry(self.field_size, tuple(int(r) for r in d["resolutions"]), int(d["features"]), int(d["log2_table"]))
        self.hidden, self.n_linear = int(d["hidden"]), int(d["n_linear"])
        self._lod_fade = None if lod_fade is None else _check_fade(self.geo.levels, lod_fade)
        if is_mixed:
            try:
                self.num_bits, self.level_bits = None, _check_level_bits(self.geo.levels, d.get("level_bits"))
            except ValueError as e:
                raise ValueError(f"{path}: level_bits: {e}") from None
        else:
            self.num_bits, self.level_bits = int(d["num_bits"]), None
            if not 1 <= self.num_bits <= 8:
                raise ValueError(f"{path}: num_bits {self.num_bits}")
        stored = d["table"]
        need = hash_packed_bytes(self.geo, self.level_bits if is_mixed else self.num_bits) if is_packed else hash_stored_bytes(self.geo)
        if not isinstance(stored, torch.Tensor) or stored.dtype != torch.uint8 or stored.dim() != 1 or stored.numel() != need:
            raise ValueError(f"{path}: the table holds {stored.numel()} {stored.dtype} values, a {d['format']} file of this geometry needs {need} bytes")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("HashGridField needs a HIP device: there is no CPU implementation of this path")
        stored = stored.to(self.device).contiguous()
        self.stored, self.packed = (None, stored) if is_packed else (stored, None)
        self.table = None
        self.decoder = ColorDecoder(self.geo.width, self.hidden, self.n_linear).to(self.device)
        self.decoder.load_state_dict(d["decoder"])
        self.optimizer = self.scheduler = None
        self.noise_seed, self.steps, self.frozen, self._pass_samples, self._grad_clean = 0, 0, True, 0, True
        self._set_route(fused)
        return self

    def _check_p16(self, precision, lod=None) -> None:
        """the refusals of ``precision=``, on the host and before anything is launched or changed"""
        _check_precision(precision)
        if lod is not None:
            raise NotImplementedError("precision= with a level of detail is not built (DESIGN 7): call without lod, or without precision")
        if self.level_bits is not None:
            raise NotImplementedError("precision= with a bit depth per level is not built (DESIGN 7): use a uniform num_bits")
        _check_p16_set(self.geo, self.hidden, self.n_linear)

    @torch.no_grad()
    def decode(self, tile: int = 1024, precision: Optional[str] = None) -> torch.Tensor:
        """the whole field [S_x, S_y(, S_z), 3], in tiles of side <= ``tile`` (a field from ``load_compressed``: from its uint8 or bit-packed table).
        ``precision``: None (those launches, unchanged), or "split" / "bf16" - every tile through ``hash_fused_forward_p16`` whatever ``route``
        is, the decoder's products on the 16-bit matrix pipe"""
        if precision is not None:
            self._check_p16(precision)
        size = self.field_size
        out = torch.empty(*size, 3, dtype=torch.float32, device=self.device)
        params = [p.detach() for p in self.decoder.linear_params()]
        table = None if self.table is None else self.table.detach()
        for o in itertools.product(*[range(0, s, tile) for s in size]):
            ext = [min(tile, s - a) for s, a in zip(size, o)]
            sl = tuple(slice(a, a + e) for a, e in zip(o, ext))
            if precision is not None:
                data, kind, bits = self._point_table()
                out[sl] = hash_fused_forward_p16(self.geo, data, params, precision, coord=[o], extent=ext, kind=kind, num_bits=bits).reshape(*ext, 3)
                continue
            if self.route == "fused":
                if table is not None:
                    y = hash_fused_forward(self.geo, table, [o], ext, params)
                elif self.level_bits is not None:
                    y = hash_fused_forward_levels(self.geo, self.packed, self.level_bits, params, coord=[o], extent=ext, kind="bits")
                elif self.packed is not None:
                    y = hash_fused_forward_bits(self.geo, self.packed, [o], ext, self.num_bits, params)
                else:
                    y = hash_fused_forward_u8(self.geo, self.stored, [o], ext, self.num_bits, params)
                out[sl] = y.reshape(*ext, 3)
                continue
            if table is not None:
                x = hash_encode(self.geo, table, [o], ext)
            elif self.level_bits is not None:
                x = hash_encode_levels(self.geo, self.packed, self.level_bits, coord=[o], extent=ext, kind="bits")
            elif self.packed is not None:
                x = hash_encode_bits(self.geo, self.packed, [o], ext, self.num_bits)
            else:
                x = hash_encode_u8(self.geo, self.stored, [o], ext, self.num_bits)
            out[sl] = fused.DecoderFunction.apply(x, *params).reshape(*ext, 3)
        return out

    def _point_table(self) -> Tuple[torch.Tensor, str, Optional[int]]:
        """the table this field holds as a point-launch source: (data, kind, num_bits) - never converted"""
        if self.table is not None:
            return self.table.detach(), "f32", None
        if self.packed is not None:
            return self.packed, "bits", self.num_bits
        return self.stored, "u8", self.num_bits

    @torch.no_grad()
    def query(self, points: torch.Tensor, lod=None, precision: Optional[str] = None) -> torch.Tensor:
        """[N, 3] colours at ``points`` [N, dim] (fp32, sample units: p = i is the centre of sample i, the field spans [-1/2, S - 1/2] and
        points outside it read its edge), from the fp32 table or - a field from ``load_compressed`` - straight from its uint8 or bit-packed
        table.  One launch on the fused route (nic_hash_fused_forward_points), encode + general decoder on the layer-wise one.  ``lod``: None
        (those launches, unchanged), or the level of detail of the query - a float, or one value per point [N]: the levels finer than the
        footprint fade out before the decoder and are not gathered (the ``_lod`` entry points, fade starts ``lod_fade``).
        ``precision``: None, or "split" / "bf16" - one launch of ``hash_fused_forward_p16`` whatever ``route`` is (not with ``lod``)."""
        if precision is not None:
            self._check_p16(precision, lod)
            data, kind, bits = self._point_table()
            return hash_fused_forward_p16(self.geo, data, [p.detach() for p in self.decoder.linear_params()], precision, points=points, kind=kind,
                                          num_bits=bits)
        if lod is not None:
            lod_t, lod_u = self._lod_args(lod)
            pts = _check_points(self.geo, points)
            data, kind, bits = self._point_table()
            params = [p.detach() for p in self.decoder.linear_params()]
            if self.route == "fused":
                return hash_fused_forward_points_lod(self.geo, data, pts, params, lod_t, lod_u, self.lod_fade, kind, bits)
            if pts.shape[0] == 0:
                return torch.empty(0, 3, dtype=torch.float32, device=self.device)
            return fused.DecoderFunction.apply(hash_encode_points_lod(self.geo, data, pts, lod_t, lod_u, self.lod_fade, kind, bits), *params)
        data, kind, bits = self._point_table()
        params = [p.detach() for p in self.decoder.linear_params()]
        if kind == "bits" and self.level_bits is not None:       # a loaded mixed-depth field: its format /2 table
            if self.route == "fused":
                return hash_fused_forward_levels(self.geo, data, self.level_bits, params, points=points, kind="bits")
            pts = _check_points(self.geo, points)
            if pts.shape[0] == 0:
                return torch.empty(0, 3, dtype=torch.float32, device=self.device)
            return fused.DecoderFunction.apply(hash_encode_levels(self.geo, data, self.level_bits, points=pts, kind="bits"), *params)
        if self.route == "fused":
            return hash_fused_forward_points(self.geo, data, points, params, kind, bits)
        pts = _check_points(self.geo, points)
        if pts.shape[0] == 0:
            return torch.empty(0, 3, dtype=torch.float32, device=self.device)
        return fused.DecoderFunction.apply(hash_encode_points(self.geo, data, pts, kind, bits), *params)

    def point_gradient(self, points: torch.Tensor, dy: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, scale: float = 1.0,
                       lod=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(y [N, 3], dpoints [N, dim]): ``query(points, lod)`` and the gradient with respect to the point COORDINATES of
        sum(y * ``dy``) for an output gradient ``dy`` [N, 3], or of mean((y - ``target``)^2) * ``scale`` for colours ``target`` [N, 3] -
        exactly one of the two.  It is the derivative of the multilinear interpolant at the rounded position ``query`` uses (piecewise
        constant along its own axis inside a cell), exactly 0 on an axis where the point lies outside the field, in sample units.  Reads
        whichever table the field holds (a field from ``load_compressed`` works).  One launch on the fused route
        (nic_hash_fused_points_grad); encode, general decoder forward and backward and nic_hash_encode_points_grad on the layer-wise one.
        The field's parameters are constants here: no ``.grad`` of the table or the decoder is touched and no optimiser state moves."""
        if self.level_bits is not None:
            raise NotImplementedError("gradients with respect to the points with a bit depth per level are not built (DESIGN 7): use a uniform num_bits")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != self.geo.dim:
            raise ValueError(f"points must be [N, {self.geo.dim}] for a {self.geo.dim}D field, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
        n = points.shape[0]
        _check_dy_target(dy, target, n)
        lod_t, lod_u, fade = None, 0.0, None
        if lod is not None:
            lod_t, lod_u = self._lod_args(lod)
            fade = self.lod_fade
        pts = _check_points(self.geo, points)
        data, kind, bits = self._point_table()
        params = [p.detach() for p in self.decoder.linear_params()]
        if self.route == "fused":
            return hash_fused_points_grad(self.geo, data, pts, params, dy=dy, target=target, loss_scale=scale, want_y=True, kind=kind, num_bits=bits,
                                          lod=lod_t, lod_uniform=lod_u, fade=fade)
        if n == 0:
            return torch.empty(0, 3, dtype=torch.float32, device=self.device), torch.empty(0, self.geo.dim, dtype=torch.float32, device=self.device)
        if lod is None:
            x = hash_encode_points(self.geo, data, pts, kind, bits)
        else:
            x = hash_encode_points_lod(self.geo, data, pts, lod_t, lod_u, fade, kind, bits)
        with torch.enable_grad():
            x.requires_grad_(True)
            y = fused.DecoderFunction.apply(x, *params)
            if dy is None:
                g = (y.detach() - _lib.require_cuda_f32(target.detach(), "target")) * (2.0 * float(scale) / (3.0 * n))
            else:
                g = _lib.require_cuda_f32(dy.detach(), "dy")
            dx, = torch.autograd.grad(y, x, g)
        return y.detach(), hash_encode_points_grad(self.geo, data, pts, dx, kind, bits, lod=lod_t, lod_uniform=lod_u, fade=fade)

    def jacobian(self, points: torch.Tensor, lod=None) -> torch.Tensor:
        """[N, 3, dim]: d y[n, o] / d points[n, a], as three ``point_gradient`` calls with a one-hot ``dy``"""
        rows = []
        for o in range(3):
            dy = torch.zeros(points.shape[0], 3, dtype=torch.float32, device=points.device)
            dy[:, o] = 1.0
            rows.append(self.point_gradient(points, dy=dy, lod=lod)[1])
        return torch.stack(rows, dim=1)

    def query_differentiable(self, points: torch.Tensor, lod=None) -> torch.Tensor:
        """``query(points, lod)`` as a differentiable op of ``points``: the backward hands the output gradient to ``point_gradient``, so
        ``points.requires_grad_()`` works with any torch loss and optimiser on the positions, or on whatever produced them (a shift, a warp, a
        pose).  No gradient reaches the field's parameters through it: table and decoder are constants here (``train_points`` trains them)."""
        if self.level_bits is not None:
            raise NotImplementedError("gradients with respect to the points with a bit depth per level are not built (DESIGN 7): use a uniform num_bits")
        if not (isinstance(points, torch.Tensor) and points.requires_grad and torch.is_grad_enabled()):
            return self.query(points, lod=lod)
        return _QueryPointsFunction.apply(points, self, lod)

    def point_gradient_lod(self, points: torch.Tensor, lod, dy: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
                           scale: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(y [N, 3], dpoints [N, dim], dlod [N]): ``point_gradient(points, dy, target, scale, lod=lod)`` - y and dpoints bit for bit - and
        the gradient of the same loss with respect to the LEVEL OF DETAIL of each point, ``lod`` a float or a [N] tensor as in
        ``query``.  ``dlod[n]`` = - sum over the levels on the ramp (0 < (fade[l] - lambda_n) + 1 <= 1, the right-hand derivative: a level
        exactly at its fade start counts, one exactly at its end does not) of the row gradient times the unweighed blend of the level;
        exactly 0 where lambda_n < 0, >= 32 or NaN; a point outside the field has the clamped point's.  The gradient for a launch-wide
        ``lod`` is ``dlod.sum()``.  One launch on the fused route (nic_hash_fused_points_grad_lod); encode, general decoder forward and
        backward and nic_hash_encode_points_grad_lod on the layer-wise one.  Reads whichever table the field holds; the field's parameters
        are constants: no ``.grad`` is touched and no optimiser state moves."""
        if self.level_bits is not None:
            raise NotImplementedError("gradients with respect to the level of detail with a bit depth per level are not built (DESIGN 7): use a "
                                      "uniform num_bits")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != self.geo.dim:
            raise ValueError(f"points must be [N, {self.geo.dim}] for a {self.geo.dim}D field, got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
        n = points.shape[0]
        _check_dy_target(dy, target, n)
        if lod is None:
            raise ValueError("lod is a float or a [N] tensor: the level of detail the gradient is taken at")
        lod_t, lod_u = self._lod_args(lod)
        fade = self.lod_fade
        pts = _check_points(self.geo, points)
        data, kind, bits = self._point_table()
        params = [p.detach() for p in self.decoder.linear_params()]
        if self.route == "fused":
            return hash_fused_points_grad_lod(self.geo, data, pts, params, dy=dy, target=target, loss_scale=scale, want_y=True, kind=kind,
                                              num_bits=bits, lod=lod_t, lod_uniform=lod_u, fade=fade)
        if n == 0:
            return (torch.empty(0, 3, dtype=torch.float32, device=self.device), torch.empty(0, self.geo.dim, dtype=torch.float32, device=self.device),
                    torch.empty(0, dtype=torch.float32, device=self.device))
        x = hash_encode_points_lod(self.geo, data, pts, lod_t, lod_u, fade, kind, bits)
        with torch.enable_grad():
            x.requires_grad_(True)
            y = fused.DecoderFunction.apply(x, *params)
            if dy is None:
                g = (y.detach() - _lib.require_cuda_f32(target.detach(), "target")) * (2.0 * float(scale) / (3.0 * n))
            else:
                g = _lib.require_cuda_f32(dy.detach(), "dy")
            dx, = torch.autograd.grad(y, x, g)
        dpoints, dlod = hash_encode_points_grad_lod(self.geo, data, pts, dx, kind, bits, lod=lod_t, lod_uniform=lod_u, fade=fade)
        return y.detach(), dpoints, dlod

    def jacobian_lod(self, points: torch.Tensor, lod) -> torch.Tensor:
        """[N, 3]: d y[n, o] / d lambda_n, as three ``point_gradient_lod`` calls with a one-hot ``dy``"""
        cols = []
        for o in range(3):
            dy = torch.zeros(points.shape[0], 3, dtype=torch.float32, device=points.device)
            dy[:, o] = 1.0
            cols.append(self.point_gradient_lod(points, lod, dy=dy)[2])
        return torch.stack(cols, dim=1)

    def query_differentiable_lod(self, points: torch.Tensor, lod) -> torch.Tensor:
        """``query(points, lod)`` as a differentiable op of ``points`` and / or ``lod`` - a [N] tensor, or a 0-dim tensor (one level of detail
        for the launch, whose gradient is the sum of the per-point ones): the backward hands the output gradient to ``point_gradient_lod``, so
        a zoom, a blur or a mip bias can be descended on with any torch loss and optimiser.  With nothing that requires a gradient, or under
        ``no_grad``, it is the plain ``query`` call.  No gradient reaches the field's parameters through it."""
        if self.level_bits is not None:
            raise NotImplementedError("gradients with respect to the level of detail with a bit depth per level are not built (DESIGN 7): use a "
                                      "uniform num_bits")
        wants = any(isinstance(t, torch.Tensor) and t.requires_grad for t in (points, lod))
        if not (wants and torch.is_grad_enabled()):
            return self.query(points, lod=lod)
        return _QueryPointsLodFunction.apply(points, lod, self)

    def _resample_points(self, size: Sequence[int], origin: Sequence[int], extent: Sequence[int]) -> torch.Tensor:
        """[prod(extent), dim] fp32 points of the block ``origin`` .. ``origin + extent`` of a regular grid of ``size`` samples over the field,
        the last axis fastest: p_a = (j + 1/2) S_a / size_a - 1/2, evaluated in float64 on the device and rounded once to fp32"""
        axes = [((torch.arange(o, o + e, dtype=torch.float64, device=self.device) + 0.5) * s / n - 0.5).to(torch.float32)
                for o, e, s, n in zip(origin, extent, self.field_size, size)]
        return torch.stack([g.reshape(-1) for g in torch.meshgrid(*axes, indexing="ij")], dim=1).contiguous()

    @torch.no_grad()
    def resample(self, size: Union[int, Sequence[int]], tile: int = 1024, lod=None, precision: Optional[str] = None) -> torch.Tensor:
        """the field decoded on a regular grid of ANY size, [*size, 3]: output sample j of axis a sits at p_a = (j + 1/2) S_a / size_a - 1/2
        (``size`` = the field size gives ``decode()``'s sample centres).  Walked in tiles of side <= ``tile``; the points of a tile are
        generated on the device.  ``lod``: None = point samples of the full-detail field; a float = ``query``'s level of detail for every
        sample; "auto" = max(0, log2(max_a S_a / size_a)), the footprint of an output sample in octaves.  ``precision``: ``query``'s (not with ``lod``)."""
        size = (int(size),) * self.geo.dim if isinstance(size, int) else tuple(int(v) for v in size)
        if len(size) != self.geo.dim or any(v < 1 for v in size):
            raise ValueError(f"size {size} for a {self.geo.dim}D field")
        if precision is not None:
            self._check_p16(precision, lod)
        if isinstance(lod, str):
            if lod != "auto":
                raise ValueError(f"lod {lod!r}: None, 'auto' or a float")
            lod = max(0.0, math.log2(max(s / v for s, v in zip(self.field_size, size))))
        if lod is not None:
            if isinstance(lod, torch.Tensor) and lod.dim() > 0:
                raise ValueError("resample takes one level of detail for the whole grid: None, 'auto' or a float")
            lod = self._lod_args(lod)[1]
        out = torch.empty(*size, 3, dtype=torch.float32, device=self.device)
        for o in itertools.product(*[range(0, s, tile) for s in size]):
            ext = [min(tile, s - a) for s, a in zip(size, o)]
            sl = tuple(slice(a, a + e) for a, e in zip(o, ext))
            out[sl] = self.query(self._resample_points(size, o, ext), lod=lod, precision=precision).reshape(*ext, 3)
        return out

    def _mip_size(self, m: int) -> Tuple[int, ...]:
        """the size of mip ``m``: S_a / 2^m on every axis, each divisible (else ValueError)"""
        m = int(m)
        if m < 0 or any(s % (1 << m) for s in self.field_size):
            raise ValueError(f"mip {m} of a field of {self.field_size} samples: every axis must be divisible by 2^{m}")
        return tuple(s >> m for s in self.field_size)

    @torch.no_grad()
    def decode_mip(self, m: int, tile: int = 1024, precision: Optional[str] = None) -> torch.Tensor:
        """mip ``m`` of the field, [S_x / 2^m, S_y / 2^m(, S_z / 2^m), 3]: sample j sits at p = (j + 1/2) 2^m - 1/2, the centre of its block of
        2^m samples per axis, and is queried with level of detail m - the levels finer than the block are faded out and not gathered
        (``precision`` other than None is refused: a mip is a level of detail)"""
        return self.resample(self._mip_size(m), tile=tile, lod=float(int(m)), precision=precision)

    def fit_mips(self, target: torch.Tensor, epochs: int, mips: int = 2, batch: Optional[int] = None, order="cell", fused: Optional[bool] = None,
                 freeze_at: float = 0.95) -> List[float]:
        """fits the whole mip chain of ``target`` [S_x, S_y(, S_z), 3] with one table and one decoder: mip m = the mean over blocks of 2^m samples
        per axis (m = 0 .. ``mips``), its samples at ``decode_mip(m)``'s points with level of detail m; the (point, lod, colour) sets of all mips go
        to ``fit_points`` as one set, so cell order, chunks and the fused route are that method's.  Returns the per-pass losses."""
        return self._fit_mips(target, epochs, mips, batch, order, fused, freeze_at, False, None)

    def fit_mips_weighted(self, target: torch.Tensor, epochs: int, mips: int = 2, mip_weights=None, batch: Optional[int] = None, order="cell",
                          fused: Optional[bool] = None, freeze_at: float = 0.95) -> List[float]:
        """``fit_mips`` with every point of mip m weighed by ``mip_weights[m]`` in the loss (``fit_points_weighted``).  Mip m
        holds 2^(-dim m) of the points, so in ``fit_mips`` the coarse mips weigh almost nothing.  ``mip_weights``: None (ones: ``fit_mips``'
        loss), ``"balanced"`` (``hash_mip_weights``: the loss is the mean of the per-mip mean squared errors) or a sequence of ``mips`` + 1
        values >= 0.  Returns the per-pass losses."""
        if self.table is None:
            raise RuntimeError("a field from load_compressed decodes only")
        return self._fit_mips(target, epochs, mips, batch, order, fused, freeze_at, True, mip_weights)

    def _fit_mips(self, target, epochs, mips, batch, order, fused, freeze_at, weighted, mip_weights) -> List[float]:
        """``fit_mips`` and (``weighted``) ``fit_mips_weighted``"""
        size, dim = self.field_size, self.geo.dim
        if tuple(target.shape) != (*size, 3):
            raise ValueError(f"target must be {(*size, 3)}, got {tuple(target.shape)}")
        if int(mips) < 0:
            raise ValueError("mips >= 0")
        sizes = [self._mip_size(m) for m in range(int(mips) + 1)]
        if self.level_bits is not None:
            raise NotImplementedError("a level of detail with a bit depth per level is not built (DESIGN 7): use a uniform num_bits")
        if weighted:
            counts = [math.prod(sz) for sz in sizes]
            mip_weights = hash_mip_weights(counts, [1.0] * len(sizes) if mip_weights is None else mip_weights)
        target = _lib.require_cuda_f32(target, "target")
        pts, lods, cols = [], [], []
        for m, sz in enumerate(sizes):
            blocks = target.reshape(*[v for s in sz for v in (s, 1 << m)], 3)
            cols.append(blocks.mean(dim=tuple(range(1, 2 * dim, 2))).reshape(-1, 3))
            pts.append(self._resample_points(sz, [0] * dim, sz))
            lods.append(torch.full((pts[-1].shape[0],), float(m), dtype=torch.float32, device=self.device))
        if weighted:
            w = torch.cat([torch.full((p.shape[0],), float(v), dtype=torch.float32, device=self.device) for p, v in zip(pts, mip_weights)])
            return self.fit_points_weighted(torch.cat(pts).contiguous(), torch.cat(cols).contiguous(), w.contiguous(), epochs, batch=batch,
                                            order=order, fused=fused, freeze_at=freeze_at, lod=torch.cat(lods).contiguous())
        return self.fit_points(torch.cat(pts).contiguous(), torch.cat(cols).contiguous(), epochs, batch=batch, order=order, fused=fused,
                               freeze_at=freeze_at, lod=torch.cat(lods).contiguous())


class HashGridFieldBatch:
    """``n_fields`` hash-grid fields of ONE geometry - the images of a folder, the tiles of a large image, the frames of a clip - trained and
    decoded together (csrc/hashgrid_batch.hip): stacked tables [B, L, T, F] and decoder tensors [B, ...], one ``FusedAdam``
    over the seven stacked tensors with the single field's learning rates.  A training step is three launches whatever B is (the batched
    kernel, the reduction of its records, the optimiser), ``decode`` one launch per tile.  The arithmetic of field b is ``HashGridField(
    fused=True)``'s: ``extract(b)`` hands it out as such a field, ``insert(b, field)`` takes one in.  ``num_bits``: None or one depth b in
    1 .. 8 for every field (the codec of ``HashGridField``); ``groups_per_field``: the workgroups a field gets per launch (0: automatic,
    ``hash_batch_groups``; a positive value is cut to the grid one field's crops admit).

    The decoder side: ``load_compressed(paths)`` builds a decode-only batch from B ``save_compressed`` files - stacked uint8 or
    bit-packed tables [B, bytes] as stored, no fp32 table, no optimiser - and ``decode`` / ``query`` / ``resample`` read whatever table a batch
    holds in one launch per tile for all fields (nic_hash_batch_forward_source); ``extract(b)`` of such a batch is what
    ``HashGridField.load_compressed(fused=True)`` makes, ``save_compressed`` re-saves it in either format.

    The 16-bit matrix pipe: ``decode`` / ``query`` / ``resample(precision="split" | "bf16")`` run every tile or point set through
    ``hash_batch_forward_p16`` from the same table - ``HashGridField``'s ``precision=`` per field, bit for bit, in one launch.  Forward only.

    Training at points: ``train_points`` / ``fit_points`` train every field at ITS OWN samples - masked images, importance
    samples, point clouds - in the same three launches (nic_hash_batch_forward_backward_points), ``counts`` giving each field's own number of
    points: rows past it are padding that is never read and never trains.  Field b's arithmetic is ``HashGridField.train_points(fused=True)``'s.

    A level of detail per point: ``query_lod`` / ``train_points_lod`` / ``fit_points_lod``, ``resample_lod``, ``decode_mip(m)``
    and ``fit_mips`` are ``HashGridField``'s ``lod=`` calls per field - the levels finer than a sample's footprint fade out before the decoder and are not
    gathered - in the batch's launches (nic_hash_batch_forward_points_lod, nic_hash_batch_forward_backward_points_lod), from the fp32 tables
    and from stored ones.  ``lod_fade``: the fade start of every level, shared by all fields (``hash_lod_fade(geo)`` unless assigned).

    Gradients to the point positions: ``point_gradient`` / ``jacobian`` / ``query_differentiable`` give d y / d points of
    every field in ONE launch (nic_hash_batch_points_grad) from whatever tables the batch holds, and ``train_points_grad`` /
    ``train_points_differentiable`` are ``train_points`` / ``train_points_lod`` that also return d loss_b / d points
    (nic_hash_batch_forward_backward_points_grad) - ``HashGridField.train_points(fused=True, dpoints=)`` per field in the batch's three
    launches: the frames of a jittered clip or the tiles of a scan are registered while they are fitted.

    Gradients to the level of detail: ``point_gradient_lod`` / ``jacobian_lod`` / ``query_differentiable_lod`` add d y / d
    lambda of every point of every field to that ONE launch (nic_hash_batch_points_grad_lod), and ``train_points_grad_lod`` /
    ``train_points_differentiable_lod`` are ``train_points_grad(lod=)`` that also return d loss_b / d lambda, the step's noise counted
    (nic_hash_batch_forward_backward_points_grad_lod) - ``HashGridField.train_points_grad_lod(fused=True)`` per field in the batch's three
    launches: the zoom of a frame or the mip bias of a tile is descended on while the fields are fitted.

    Not built: at points, passes in chunks with ragged counts, and the 16-bit modes with ``lod`` or with position or
    level-of-detail gradients; ``fit_points`` with positions or a level of detail to fit; 16-bit training; a bit depth per level (a ``/2`` file is
    read and refused), fields of differing geometry in one batch, a container format that holds several fields in one file."""

    def __init__(self, n_fields: int, field_size: Union[int, Sequence[int]], levels: int = 16, features: int = 2, log2_table: int = 19,
                 base_resolution: float = 16, finest_resolution: Optional[float] = None, device=None, seed: Optional[int] = None,
                 num_bits: Optional[int] = None, noise_seed: int = 7, groups_per_field: int = 0, hidden: int = 64, n_linear: int = 3):
        # every refusal comes before the device is touched
        if int(n_fields) < 1:
            raise ValueError("a batch holds at least one field")
        if _is_level_bits(num_bits):
            raise NotImplementedError("a bit depth per level in a batch is not built (DESIGN 7): use one num_bits for every field")
        if num_bits is not None and not 1 <= int(num_bits) <= 8:
            raise ValueError("num_bits in 1 .. 8 (the stored table is uint8), or None")
        if int(hidden) != 64 or int(n_linear) != 3:
            raise ValueError("the batched kernels decode with 3 Linear layers of 64 hidden units (hidden=64, n_linear=3)")
        if int(groups_per_field) < 0 or int(groups_per_field) % 8:
            raise ValueError(f"groups_per_field {groups_per_field}: 0 (automatic) or a multiple of 8")
        self.field_size = (int(field_size),) * 2 if isinstance(field_size, int) else tuple(int(v) for v in field_size)
        n_max = max(self.field_size) if finest_resolution is None else finest_resolution
        self.geo = HashGeometry(self.field_size, tuple(level_resolutions(levels, base_resolution, n_max)), features, log2_table)
        if not hash_fused_supported(self.geo, 64, 3):
            raise ValueError("a batch needs a geometry of the fused set (nic_hash_fused_supported): dim 2 / 3, features 1 / 2 / 4 / 8, L F <= 64")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("HashGridFieldBatch needs a HIP device: there is no CPU implementation of this path")
        self.n_fields, self.hidden, self.n_linear = int(n_fields), 64, 3
        self.num_bits = None if num_bits is None else int(num_bits)
        self.noise_seed, self.groups_per_field, self._lod_fade = int(noise_seed), int(groups_per_field), None
        self._field_args = dict(levels=int(levels), features=int(features), log2_table=int(log2_table), base_resolution=base_resolution,
                                finest_resolution=finest_resolution)
        if seed is not None:
            torch.manual_seed(seed)
        b = self.n_fields
        self.stored = self.packed = None             # a decode-only batch (load_compressed) holds one of these instead of ``tables``
        self.tables = torch.empty(b, *self.geo.table_shape(), dtype=torch.float32, device=self.device).uniform_(-1e-4, 1e-4).requires_grad_(True)
        decoders = [ColorDecoder(self.geo.width, 64, 3).linear_params() for _ in range(b)]       # nn.Linear's default init, field by field
        self.params = [torch.stack([d[k].detach() for d in decoders]).to(self.device).contiguous().requires_grad_(True) for k in range(6)]
        self.optimizer = FusedAdam([{"params": [self.tables], "lr": 0.01}, {"params": self.params, "lr": 0.005}])
        # the table gradient persists: the optimiser launch zeroes it after reading it, so a step needs no fill launch
        self.tables.grad = torch.zeros_like(self.tables)
        self.optimizer.zero_grad_in_step([self.tables])
        self._gm = [torch.zeros_like(p) for p in self.params]
        for p, g in zip(self.params, self._gm):
            p.grad = g
        self._grad_clean, self.scheduler, self.steps, self.frozen, self._pass_samples = True, None, 0, False, 0
        if self.num_bits is not None:
            self.optimizer.set_clamp([self.tables], *models._q_range(self.num_bits))

    @property
    def resolutions(self) -> Tuple[int, ...]:
        return self.geo.resolutions

    def set_schedule(self, num_epochs: int) -> None:
        self.scheduler = CosineAnnealing(self.optimizer, T_max=num_epochs, eta_min=0)

    @property
    def lod_fade(self) -> Tuple[float, ...]:
        """the fade start of every level for the ``_lod`` calls, shared by all fields: ``hash_lod_fade(geo)`` unless one was
        assigned (``batch.lod_fade = [...]``: ``levels`` finite values >= 0, or None for the default); ``extract(b)`` hands it to the field"""
        fade = getattr(self, "_lod_fade", None)
        return fade if fade is not None else hash_lod_fade(self.geo)

    @lod_fade.setter
    def lod_fade(self, fade) -> None:
        self._lod_fade = None if fade is None else _check_fade(self.geo.levels, fade)

    @staticmethod
    def _lod_args(lod) -> Tuple[Optional[torch.Tensor], float]:
        """``lod`` of a call - a finite float, or a tensor [N] / [B, N] - as (per-point tensor or None, launch-wide value); the tensor is
        checked against the points by ``_check_batch_lod``"""
        if isinstance(lod, torch.Tensor) and lod.dim() > 0:
            return lod, 0.0
        if isinstance(lod, (str, bytes)):
            raise ValueError(f"lod is a float or a [N] / [B, N] tensor, got {lod!r}")
        try:
            v = float(lod)
        except (TypeError, ValueError):
            raise ValueError(f"lod is a float or a [N] / [B, N] tensor, got {lod!r}") from None
        if not math.isfinite(v):
            raise ValueError(f"lod {lod!r} is not finite")
        return None, v

    def _groups(self, num_crops: int, extent: Sequence[int]) -> int:
        """the constructor's ``groups_per_field`` for a launch on these crops: 0 stays automatic, a positive value is cut to the grid one
        field's patches admit (the C entry refuses more)"""
        if self.groups_per_field == 0:
            return 0
        return min(self.groups_per_field, (((_patches(self.geo, num_crops, extent) + 3) // 4) + 7) // 8 * 8)

    def _check_field_index(self, b) -> int:
        if not 0 <= int(b) < self.n_fields:
            raise IndexError(f"field {b} of a batch of {self.n_fields}")
        return int(b)

    @property
    def decode_only(self) -> bool:
        """a batch from ``load_compressed``: stored tables, no fp32 tables, no optimiser"""
        return getattr(self, "tables", False) is None

    def _refuse_decode_only(self, what: str) -> None:
        if self.decode_only:
            raise RuntimeError(f"{what}: a batch from load_compressed is decode-only (it holds the stored tables, no fp32 tables and no optimiser)")

    @staticmethod
    def _read_compressed(path) -> dict:
        """what one ``save_compressed`` file says about itself, checked on the host: format, geometry, num_bits, decoder shape, table, decoder"""
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or d.get("format") not in (COMPRESSED_FORMAT, PACKED_FORMAT, MIXED_FORMAT):
            raise ValueError(f"{path}: not a {COMPRESSED_FORMAT}, {PACKED_FORMAT} or {MIXED_FORMAT} file")
        if d["format"] == MIXED_FORMAT:
            raise NotImplementedError(f"{path}: a bit depth per level ({MIXED_FORMAT}) in a batch is not built (DESIGN 7): load it with "
                                      "HashGridField.load_compressed")
        field_size = tuple(int(v) for v in d["field_size"])
        geo = HashGeometry(field_size, tuple(int(r) for r in d["resolutions"]), int(d["features"]), int(d["log2_table"]))
        num_bits = int(d["num_bits"])
        if not 1 <= num_bits <= 8:
            raise ValueError(f"{path}: num_bits {num_bits}")
        return {"format": d["format"], "geo": geo, "num_bits": num_bits, "decoder_shape": (int(d["hidden"]), int(d["n_linear"])), "table": d["table"],
                "decoder": d["decoder"]}

    @classmethod
    def load_compressed(cls, paths: Sequence, device=None, groups_per_field: int = 0) -> "HashGridFieldBatch":
        """a decode-only batch from B ``save_compressed`` files of ONE format (uint8 or bit-packed, uniform depth), geometry, ``num_bits`` and
        decoder shape - anything else is a ValueError naming the first path that differs; a ``/2`` (bit depth per level) file raises
        NotImplementedError.  The tables stay as stored, stacked [B, bytes] on the device; ``decode`` / ``query`` / ``resample`` gather from
        them in one launch per tile for all fields.  There is no new file format: each file is ``HashGridField.load_compressed``'s."""
        paths = list(paths)
        if not paths:
            raise ValueError("load_compressed: no paths (a batch holds at least one field)")
        if int(groups_per_field) < 0 or int(groups_per_field) % 8:
            raise ValueError(f"groups_per_field {groups_per_field}: 0 (automatic) or a multiple of 8")
        first, tables, decoders = None, [], []
        for path in paths:
            f = cls._read_compressed(path)
            if first is None:
                first = f
                if f["decoder_shape"] != (64, 3):
                    raise ValueError(f"{path}: hidden {f['decoder_shape'][0]}, n_linear {f['decoder_shape'][1]}: the batched kernels decode with 3 Linear "
                                     "layers of 64 hidden units (hidden=64, n_linear=3)")
                if not hash_fused_supported(f["geo"], 64, 3):
                    raise ValueError(f"{path}: a batch needs a geometry of the fused set (nic_hash_fused_supported): dim 2 / 3, features 1 / 2 / 4 / 8, "
                                     "L F <= 64")
                is_packed = f["format"] == PACKED_FORMAT
                need = hash_packed_bytes(f["geo"], f["num_bits"]) if is_packed else hash_stored_bytes(f["geo"])
            for key, name in (("format", "format"), ("geo", "geometry"), ("num_bits", "num_bits"), ("decoder_shape", "decoder shape (hidden, n_linear)")):
                if f[key] != first[key]:
                    raise ValueError(f"{path}: its {name} {f[key]} is not {first[key]}, that of {paths[0]}: the files of a batch agree in all four")
            t = f["table"]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != need:
                raise ValueError(f"{path}: the table holds {t.numel()} {t.dtype} values, a {f['format']} file of this geometry needs {need} bytes")
            dec = ColorDecoder(first["geo"].width, 64, 3)
            dec.load_state_dict(f["decoder"])
            tables.append(t)
            decoders.append([q.detach() for q in dec.linear_params()])
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise RuntimeError("HashGridFieldBatch needs a HIP device: there is no CPU implementation of this path")
        self = cls.__new__(cls)
        self._lod_fade = None                        # the files hold no fade: ``lod_fade`` may be assigned
        self.geo, self.field_size, self.device = first["geo"], first["geo"].field_size, device
        self.n_fields, self.hidden, self.n_linear, self.num_bits = len(paths), 64, 3, first["num_bits"]
        self.noise_seed, self.groups_per_field = 0, int(groups_per_field)
        stack = torch.stack(tables).to(device).contiguous()
        self.stored, self.packed = (None, stack) if is_packed else (stack, None)
        self.tables = None
        self.params = [torch.stack([d[k] for d in decoders]).to(device).contiguous() for k in range(6)]
        self.optimizer = self.scheduler = self._gm = None
        self._grad_clean, self.steps, self.frozen, self._pass_samples = True, 0, True, 0
        return self

    def _table_source(self) -> Tuple[torch.Tensor, str, Optional[int]]:
        """the stacked tables this batch holds as a launch source: (data, kind, num_bits) - never converted"""
        if self.tables is not None:
            return self.tables.detach(), "f32", None
        if self.packed is not None:
            return self.packed, "bits", self.num_bits
        return self.stored, "u8", self.num_bits

    @torch.no_grad()
    def train_step(self, coord, extent: Sequence[int], target: torch.Tensor, accumulate: bool = False, scale: float = 1.0, step: bool = True,
                   noise: Optional[bool] = None) -> torch.Tensor:
        """``HashGridField.train_step`` for every field at once; returns the [B] losses.  ``coord`` [num_crops, dim]: the crops of every field;
        [B, num_crops, dim]: each field's own (validated per field).  ``target`` [B, N, 3].  ``accumulate`` / ``scale`` / ``step`` / ``noise``
        are the single field's: the noise keys (seed, optimiser step, samples of this pass before this chunk + the row inside the field) are
        the same for every field, so field b trains exactly as alone.  After ``freeze()`` only the decoders train."""
        self._refuse_decode_only("train_step")
        frozen = self.frozen
        if isinstance(coord, torch.Tensor) and coord.is_cuda:
            num_crops = coord.shape[-2] if coord.dim() >= 2 else 1
        else:                                            # host origins: validated before anything else is touched
            coord = _batch_origins(self.geo, coord, extent, self.n_fields, "cpu")
            num_crops = coord.shape[1]
        if len(extent) != self.geo.dim or any(int(e) < 1 for e in extent):
            raise ValueError(f"extent {tuple(extent)} for a {self.geo.dim}D field")
        n = _n_samples(num_crops, extent)
        if not isinstance(target, torch.Tensor) or tuple(target.shape) != (self.n_fields, n, 3):
            raise ValueError(f"target must be [{self.n_fields}, {n}, 3], got {tuple(target.shape) if isinstance(target, torch.Tensor) else type(target).__name__}")
        if noise is None:
            noise = self.num_bits is not None and not frozen
        if noise and self.num_bits is None:
            raise ValueError("noise needs num_bits: its amplitude is one quantisation step")
        grad = None if frozen else self.tables.grad
        if not accumulate:
            if not frozen and not self._grad_clean:
                grad.zero_()
            self._pass_samples = 0
        quant = (self.num_bits, self.noise_seed, self.steps, self._pass_samples) if noise else None
        loss, _ = hash_batch_forward_backward(self.geo, self.tables, coord.to(self.device) if not coord.is_cuda else coord, extent, self.params, target,
                                              self._gm, table_grads=grad, loss_scale=float(scale), quant=quant, add_grads=accumulate,
                                              groups_per_field=self._groups(num_crops, extent))
        self._pass_samples += n
        if not frozen:
            self._grad_clean = False
        if step:
            self.apply_step()
        return loss

    def _check_train_points(self, points, target, counts, order):
        """every host refusal of ``train_points`` / ``fit_points``, nothing set: (N, the counts as ``_check_batch_counts`` leaves them, the order
        - None, "cell" or the checked tensor)"""
        n = _check_batch_points(self.geo, points, self.n_fields)
        if n < 1:
            raise ValueError("no points")
        if not isinstance(target, torch.Tensor) or tuple(target.shape) != (self.n_fields, n, 3):
            raise ValueError(f"target must be [{self.n_fields}, {n}, 3], got {tuple(target.shape) if isinstance(target, torch.Tensor) else type(target).__name__}")
        counts = _check_batch_counts(counts, self.n_fields, n)
        if isinstance(order, str):
            if order != "cell":
                raise ValueError(f"order {order!r}: None, 'cell' or an int32 [{self.n_fields}, {n}] tensor")
        else:
            order = _check_batch_order(order, self.n_fields, n)
        _point_desc(self.geo)
        return n, counts, order

    @torch.no_grad()
    def train_points(self, points: torch.Tensor, target: torch.Tensor, counts=None, accumulate: bool = False, scale: float = 1.0, step: bool = True,
                     noise: Optional[bool] = None, order=None) -> torch.Tensor:
        """``HashGridField.train_points(fused=True)`` for every field at once, each at its own samples; returns the [B] losses.
        ``points`` as ``query`` takes them - [N, dim] shared or [B, N, dim] per field, fp32, sample units -, ``target`` [B, N, 3].  ``counts``:
        None, B ints or an int32 [B] tensor - real point sets are ragged: field b trains on its first ``counts[b]`` rows and its loss is the
        mean over those; the rest of its row is padding that is never read.  ``order``: None, "cell" (``hash_batch_point_order`` of these
        points, computed for this call) or a precomputed int32 [B, N] tensor of it.  ``accumulate`` / ``scale`` / ``step`` / ``noise`` and
        the bookkeeping are ``train_step``'s: the noise keys (seed, optimiser step, samples of this pass before this chunk + the row inside
        the field) are the same for every field, and a chunk advances the pass by the padded width N.  After ``freeze()`` only the decoders
        train.  With a level of detail: ``train_points_lod``."""
        return self._train_points(points, target, counts, accumulate, scale, step, noise, order, None)

    @torch.no_grad()
    def train_points_lod(self, points: torch.Tensor, target: torch.Tensor, lod, counts=None, accumulate: bool = False, scale: float = 1.0,
                         step: bool = True, noise: Optional[bool] = None, order=None) -> torch.Tensor:
        """``train_points`` with a level of detail for these samples - ``HashGridField.train_points(fused=True, lod=)`` for
        every field at once, in the same three launches (nic_hash_batch_forward_backward_points_lod).  ``lod``: a finite float, a tensor [N]
        shared by all fields or [B, N], each field its own; it fades the finer levels out of a sample's row and of its gradient (fade starts
        ``lod_fade``) and is read at the row the point is read at.  Every other argument is ``train_points``'."""
        if lod is None:
            raise ValueError("lod is a float or a [N] / [B, N] tensor: without a level of detail call train_points")
        return self._train_points(points, target, counts, accumulate, scale, step, noise, order, lod)

    @torch.no_grad()
    def _train_points(self, points, target, counts, accumulate, scale, step, noise, order, lod, dpoints=False, dlod=False):
        """``train_points`` (``lod`` None: exactly the calls it always made) and ``train_points_lod``; with ``dpoints`` - None or the tensor
        to fill - ``train_points_grad``: the same bookkeeping around the joint entry, and (loss, dpoints) back; with ``dlod`` on top (``lod``
        is then given) ``train_points_grad_lod``, and (loss, dpoints, dlod) back"""
        self._refuse_decode_only("train_points")
        frozen = self.frozen
        lod_t, lod_u = (None, 0.0) if lod is None else self._lod_args(lod)
        n, counts, order = self._check_train_points(points, target, counts, order)
        lod_t = _check_batch_lod(lod_t, self.n_fields, n)
        if noise is None:
            noise = self.num_bits is not None and not frozen
        if noise and self.num_bits is None:
            raise ValueError("noise needs num_bits: its amplitude is one quantisation step")
        _require_on_device(points, "points")
        pts = _stack_points(points, self.n_fields)
        if isinstance(order, str):
            order = hash_batch_point_order(self.geo, pts, counts)
        grad = None if frozen else self.tables.grad
        if not accumulate:
            if not frozen and not self._grad_clean:
                grad.zero_()
            self._pass_samples = 0
        quant = (self.num_bits, self.noise_seed, self.steps, self._pass_samples) if noise else None
        if dlod is not False:
            loss, _, dpoints, dlod = hash_batch_forward_backward_points_grad_lod(
                self.geo, self.tables, pts, self.params, target, self._gm, lod_t, lod_u, self.lod_fade, table_grads=grad, order=order, counts=counts,
                loss_scale=float(scale), quant=quant, add_grads=accumulate, groups_per_field=self._point_groups(n), dpoints=dpoints, dlod=dlod)
        elif dpoints is not False:
            loss, _, dpoints = hash_batch_forward_backward_points_grad(
                self.geo, self.tables, pts, self.params, target, self._gm, lod_t, lod_u, None if lod is None else self.lod_fade, table_grads=grad,
                order=order, counts=counts, loss_scale=float(scale), quant=quant, add_grads=accumulate, groups_per_field=self._point_groups(n),
                dpoints=dpoints)
        elif lod is None:
            loss, _ = hash_batch_forward_backward_points(self.geo, self.tables, pts, self.params, target, self._gm, table_grads=grad, order=order,
                                                         counts=counts, loss_scale=float(scale), quant=quant, add_grads=accumulate,
                                                         groups_per_field=self._point_groups(n))
        else:
            loss, _ = hash_batch_forward_backward_points_lod(self.geo, self.tables, pts, self.params, target, self._gm, lod_t, lod_u, self.lod_fade,
                                                             table_grads=grad, order=order, counts=counts, loss_scale=float(scale), quant=quant,
                                                             add_grads=accumulate, groups_per_field=self._point_groups(n))
        self._pass_samples += n
        if not frozen:
            self._grad_clean = False
        if step:
            self.apply_step()
        if dlod is not False:
            return loss, dpoints, dlod
        return loss if dpoints is False else (loss, dpoints)

    @torch.no_grad()
    def train_points_grad(self, points: torch.Tensor, target: torch.Tensor, dpoints: Optional[torch.Tensor] = None, lod=None, counts=None,
                          accumulate: bool = False, scale: float = 1.0, step: bool = True, noise: Optional[bool] = None, order=None):
        """``train_points`` (with ``lod``: ``train_points_lod``) that also returns d loss_b / d points of every field's loss -
        ``HashGridField.train_points(fused=True, dpoints=)`` for every field at once, in the same three launches
        (nic_hash_batch_forward_backward_points_grad): the fields step as they always do, and the positions - the shift of a frame, the offset
        of a tile, a pose - can be stepped from the same forward.  Returns (loss [B], dpoints [B, N, dim]); ``dpoints``: None for a fresh
        tensor (zero at the rows a field does not own), or a contiguous fp32 [B, N, dim] device tensor that is overwritten at the rows each
        field owns, whatever ``accumulate`` says: each chunk of an accumulated pass fills its own.  The gradient is taken at the parameters
        the forward used (before this call's optimiser step), the noise and the level weights constant; after ``freeze()`` it still comes.
        Every other argument, the bookkeeping and the noise keys are ``train_points``'."""
        self._refuse_decode_only("train_points_grad")
        if dpoints is not None:
            n, _, _ = self._check_train_points(points, target, counts, order)
            _check_batch_dpoints_shape(self.geo, self.n_fields, n, dpoints)
        return self._train_points(points, target, counts, accumulate, scale, step, noise, order, lod, dpoints=dpoints)

    def train_points_differentiable(self, points: torch.Tensor, target: torch.Tensor, **kwargs) -> torch.Tensor:
        """``train_points_grad(points, target, **kwargs)`` as a differentiable op of ``points``: the call steps the fields as
        it always does and returns the [B] losses, whose backward hands upstream[b] * d loss_b / d points[b] to ``points`` - summed over the
        fields when ``points`` is the shared [N, dim] - so a torch optimiser on whatever produced the positions (a shift per frame, an
        offset per tile) steps from the same forward.  No gradient reaches the fields' parameters through autograd: their step is the
        call's own.  Without ``points.requires_grad``, or under ``torch.no_grad()``, it is plain ``train_points`` / ``train_points_lod``."""
        if "dpoints" in kwargs:
            raise TypeError("train_points_differentiable keeps dpoints for the backward: call train_points_grad for the tensor itself")
        if not (isinstance(points, torch.Tensor) and points.requires_grad and torch.is_grad_enabled()):
            kwargs = dict(kwargs)
            lod = kwargs.pop("lod", None)
            return self.train_points(points, target, **kwargs) if lod is None else self.train_points_lod(points, target, lod, **kwargs)
        return _BatchTrainPointsFunction.apply(points, self, target, kwargs)

    @torch.no_grad()
    def train_points_grad_lod(self, points: torch.Tensor, target: torch.Tensor, lod, dpoints: Optional[torch.Tensor] = None,
                              dlod: Optional[torch.Tensor] = None, counts=None, accumulate: bool = False, scale: float = 1.0, step: bool = True,
                              noise: Optional[bool] = None, order=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(loss [B], dpoints [B, N, dim], dlod [B, N]): ``train_points_grad(points, target, lod=lod)`` that also returns d loss_b / d
        lambda_{b, n} of every field's loss - ``HashGridField.train_points_grad_lod(fused=True)`` for every field at once, in
        the same three launches (nic_hash_batch_forward_backward_points_grad_lod): for a level of detail that comes from parameters fitted
        with the fields - the zoom of a frame ``lambda_b = log2 s_b + bias_b``, a mip bias per tile or view.  ``lod`` is required: a finite
        float, a 0-dim tensor, a tensor [N] shared by all fields or [B, N]; the gradient for a shared one is ``dlod.sum(0)``, for a launch-wide
        one ``dlod.sum()``.  ``dlod`` counts the noise this step's forward added inside the weighed column (the slope on the ramp is
        -(r + nz)), is the right-hand derivative, exactly 0 where lambda < 0, >= 32 or NaN, and is taken like ``dpoints`` at the parameters
        the forward used.  ``dpoints`` / ``dlod``: None for fresh tensors (zero at the rows a field does not own), or contiguous fp32
        [B, N, dim] / [B, N] device tensors that are overwritten at the rows each field owns, whatever ``accumulate`` says.  Every other
        argument, the bookkeeping and the noise keys are ``train_points``'."""
        self._refuse_decode_only("train_points_grad_lod")
        if lod is None:
            raise ValueError("lod is a float or a [N] / [B, N] tensor: the level of detail the gradient is taken at")
        if dpoints is not None or dlod is not None:
            n, _, _ = self._check_train_points(points, target, counts, order)
            if dpoints is not None:
                _check_batch_dpoints_shape(self.geo, self.n_fields, n, dpoints)
            if dlod is not None:
                _check_batch_dlod_shape(self.n_fields, n, dlod)
        return self._train_points(points, target, counts, accumulate, scale, step, noise, order, lod, dpoints=dpoints, dlod=dlod)

    def train_points_differentiable_lod(self, points: torch.Tensor, lod, target: torch.Tensor, **kwargs) -> torch.Tensor:
        """``train_points_grad_lod(points, target, lod, **kwargs)`` as a differentiable op of ``points`` and / or ``lod`` -
        ``lod`` a [B, N] tensor, a [N] tensor shared by the fields or a 0-dim tensor: the call steps the fields as it always does and returns
        the [B] losses, whose backward hands upstream[b] * d loss_b / d points[b] and upstream[b] * d loss_b / d lambda[b] to whichever
        requires a gradient - summed over the fields for shared [N, dim] points or a shared [N] ``lod``, over everything for a 0-dim one.
        With nothing that requires one, or under ``torch.no_grad()``, it is plain ``train_points_lod``.  No gradient reaches the fields'
        parameters through autograd: their step is the call's own."""
        if "dpoints" in kwargs or "dlod" in kwargs:
            raise TypeError("train_points_differentiable_lod keeps dpoints and dlod for the backward: call train_points_grad_lod for the tensors")
        wants = any(isinstance(t, torch.Tensor) and t.requires_grad for t in (points, lod))
        if not (wants and torch.is_grad_enabled()):
            return self.train_points_lod(points, target, lod, **kwargs)
        self._refuse_decode_only("train_points_differentiable_lod")
        _check_batch_points(self.geo, points, self.n_fields)
        return _BatchTrainPointsLodFunction.apply(points, lod, self, target, kwargs)

    def fit_points(self, points: torch.Tensor, target: torch.Tensor, epochs: int, counts=None, order="cell", freeze_at: float = 0.95) -> List[List[float]]:
        """``HashGridField.fit_points(fused=True)`` for every field on its own fixed sample set: ``epochs`` passes over ``points`` / ``target`` /
        ``counts`` (``train_points``'), one call and one optimiser step per pass.  ``order``: "cell" (default), None or an int32 [B, N]
        tensor; it is computed once and every field's set is laid out in it once (its real rows first, in order, then its padding), so the
        passes walk contiguous memory without an index.  With ``num_bits``: noise while the epoch is below ``freeze_at`` * epochs, then
        ``freeze()`` - ``fit``'s schedule.  Returns the per-pass losses, [epochs][B].  With a level of detail: ``fit_points_lod``."""
        return self._fit_points(points, target, epochs, counts, order, freeze_at, None)

    def fit_points_lod(self, points: torch.Tensor, target: torch.Tensor, epochs: int, lod, counts=None, order="cell",
                       freeze_at: float = 0.95) -> List[List[float]]:
        """``fit_points`` with ``train_points_lod``'s level of detail: a ``lod`` tensor is laid out in the order with the points
        and targets, once.  Every other argument is ``fit_points``'."""
        if lod is None:
            raise ValueError("lod is a float or a [N] / [B, N] tensor: without a level of detail call fit_points")
        return self._fit_points(points, target, epochs, counts, order, freeze_at, lod)

    def _fit_points(self, points, target, epochs, counts, order, freeze_at, lod) -> List[List[float]]:
        """``fit_points`` (``lod`` None) and ``fit_points_lod``"""
        self._refuse_decode_only("fit_points")
        lod_t, lod_u = (None, None) if lod is None else self._lod_args(lod)
        n, counts, order = self._check_train_points(points, target, counts, order)
        lod_t = _check_batch_lod(lod_t, self.n_fields, n)
        _require_on_device(points, "points")
        target = _lib.require_cuda_f32(target, "target")
        pts = _stack_points(points, self.n_fields)
        lod_t = _stack_lod(lod_t, self.n_fields, pts.device)
        if order is not None:
            idx = (hash_batch_point_order(self.geo, pts, counts) if isinstance(order, str) else order.to(pts.device)).to(torch.int64)
            top = torch.full((self.n_fields, 1), n, dtype=torch.int64, device=pts.device) if counts is None else counts.to(pts.device, torch.int64).clamp(0, n).unsqueeze(1)
            real = torch.arange(n, device=pts.device).unsqueeze(0) < top          # the kernel's rule: the first n_b entries name rows below n_b
            idx = torch.minimum(idx, torch.where(real, top - 1, torch.full_like(top, n - 1))).clamp_(min=0)
            pts = torch.gather(pts, 1, idx.unsqueeze(2).expand(-1, -1, self.geo.dim)).contiguous()
            target = torch.gather(target, 1, idx.unsqueeze(2).expand(-1, -1, 3)).contiguous()
            lod_t = None if lod_t is None else torch.gather(lod_t, 1, idx).contiguous()
        counts = None if counts is None else counts.to(pts.device)          # once: a device tensor is taken as it is by every pass
        freeze_epoch = math.ceil(freeze_at * epochs) if self.num_bits is not None else None
        hist = []
        for ep in range(epochs):
            if freeze_epoch is not None and ep >= freeze_epoch and not self.frozen:
                self.freeze()
            if lod is None:
                hist.append(self.train_points(pts, target, counts=counts))
            else:
                hist.append(self.train_points_lod(pts, target, lod_u if lod_t is None else lod_t, counts=counts))
        return [[float(v) for v in h] for h in torch.stack(hist).tolist()] if hist else []

    def _mip_size(self, m: int) -> Tuple[int, ...]:
        return HashGridField._mip_size(self, m)

    def fit_mips(self, targets: torch.Tensor, epochs: int, mips: int = 2, order="cell", freeze_at: float = 0.95) -> List[List[float]]:
        """``HashGridField.fit_mips`` for every field at once on ``targets`` [B, S_x, S_y(, S_z), 3]: mip m = the mean over blocks of 2^m
        samples per axis (m = 0 .. ``mips``), its samples at ``decode_mip(m)``'s points with level of detail m.  The points and their ``lod``
        are built once and shared by all fields, the colours are each field's; the sets of all mips go to ONE ``fit_points_lod`` call, so cell
        order and the freeze schedule are that method's.  Returns the per-pass losses, [epochs][B]."""
        self._refuse_decode_only("fit_mips")
        size, dim, b = self.field_size, self.geo.dim, self.n_fields
        if not isinstance(targets, torch.Tensor) or tuple(targets.shape) != (b, *size, 3):
            raise ValueError(f"targets must be {(b, *size, 3)}, got {tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets).__name__}")
        if int(mips) < 0:
            raise ValueError("mips >= 0")
        sizes = [self._mip_size(m) for m in range(int(mips) + 1)]
        targets = _lib.require_cuda_f32(targets, "targets")
        pts, lods, cols = [], [], []
        for m, sz in enumerate(sizes):
            blocks = targets.reshape(b, *[v for s in sz for v in (s, 1 << m)], 3)
            cols.append(blocks.mean(dim=tuple(range(2, 2 * dim + 1, 2))).reshape(b, -1, 3))
            pts.append(HashGridField._resample_points(self, sz, [0] * dim, sz))
            lods.append(torch.full((pts[-1].shape[0],), float(m), dtype=torch.float32, device=self.device))
        return self.fit_points_lod(torch.cat(pts).contiguous(), torch.cat(cols, dim=1).contiguous(), epochs, torch.cat(lods).contiguous(), order=order,
                                   freeze_at=freeze_at)

    @torch.no_grad()
    def apply_step(self) -> None:
        """the optimiser half of ``train_step(step=True)``: ONE ``nic_adam_multi`` over the stacked tensors on the gradients the buffers hold
        (the table gradient is zeroed by the same launch, the tables are clamped to the quantiser's range), then the schedule and the step count"""
        self._refuse_decode_only("apply_step")
        grad = None if self.frozen else self.tables.grad
        for p, g in zip(self.params, self._gm):
            p.grad = g
        self.optimizer.step()
        if grad is not None:
            self._grad_clean = self.optimizer.zeroed_in_last_step(grad)
        if self.scheduler is not None:
            self.scheduler.step()
        self.steps += 1

    @torch.no_grad()
    def freeze(self) -> None:
        """quantise every table in place (nic_quantize) and stop updating them: ``train_step`` then trains the decoders alone, without noise"""
        self._refuse_decode_only("freeze")
        if self.num_bits is None:
            raise RuntimeError("freeze() needs num_bits: there is no quantiser without it")
        if self.frozen:
            return
        t = self.tables.detach()
        _lib.check(_lib.load().nic_quantize(_lib.ptr(t), _lib.ptr(t), t.numel(), self.num_bits, _lib.stream_ptr(t.device)), "nic_quantize")
        self.tables.grad = None                      # FusedAdam skips a parameter without a gradient
        self.tables.requires_grad_(False)
        self.frozen = True

    def fit(self, targets: torch.Tensor, epochs: int, chunk: Optional[int] = None, freeze_at: float = 0.95) -> List[List[float]]:
        """``HashGridField.fit`` on ``targets`` [B, S_x, S_y(, S_z), 3]: ``epochs`` whole-field passes walked in slabs of ``chunk`` x-rows (one
        optimiser step per pass, each slab's MSE weighted by its share); with ``num_bits`` noise while the epoch is below ``freeze_at`` *
        epochs, then ``freeze()``.  Returns the per-pass losses, [epochs][B]."""
        self._refuse_decode_only("fit")
        size = self.field_size
        if not isinstance(targets, torch.Tensor) or tuple(targets.shape) != (self.n_fields, *size, 3):
            raise ValueError(f"targets must be {(self.n_fields, *size, 3)}, got {tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets).__name__}")
        chunk = size[0] if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("chunk >= 1")
        starts = list(range(0, size[0], chunk))
        slabs = [targets[:, x0:x0 + chunk].reshape(self.n_fields, -1, 3).contiguous() for x0 in starts]
        total = sum(s.shape[1] for s in slabs)
        freeze_epoch = math.ceil(freeze_at * epochs) if self.num_bits is not None else None
        hist = []
        for ep in range(epochs):
            if freeze_epoch is not None and ep >= freeze_epoch and not self.frozen:
                self.freeze()
            tot = 0.0
            for k, x0 in enumerate(starts):
                ext = (min(chunk, size[0] - x0), *size[1:])
                tot = tot + self.train_step([[x0] + [0] * (len(size) - 1)], ext, slabs[k], accumulate=k > 0, scale=slabs[k].shape[1] / total,
                                            step=k == len(starts) - 1)
            hist.append(tot)
        return [[float(v) for v in h] for h in torch.stack(hist).tolist()] if hist else []

    @torch.no_grad()
    def decode(self, tile: int = 1024, precision: Optional[str] = None) -> torch.Tensor:
        """every field whole, [B, S_x, S_y(, S_z), 3], in tiles of side <= ``tile``: one launch per tile for all fields, from whatever table the
        batch holds - the fp32 tables (nic_hash_batch_forward, the launches a trained batch always made), or a decode-only batch's uint8 or
        bit-packed ones as stored (nic_hash_batch_forward_source).  ``precision``: None (those launches, unchanged), or "split" / "bf16" -
        every tile through ``hash_batch_forward_p16`` from the same table, ``HashGridField.decode(precision=)``'s bits per field"""
        if precision is not None:
            _check_precision(precision)
        size = self.field_size
        out = torch.empty(self.n_fields, *size, 3, dtype=torch.float32, device=self.device)
        params = [p.detach() for p in self.params]
        data, kind, bits = self._table_source()
        for o in itertools.product(*[range(0, s, tile) for s in size]):
            ext = [min(tile, s - a) for s, a in zip(size, o)]
            sl = (slice(None), *(slice(a, a + e) for a, e in zip(o, ext)))
            if precision is not None:
                y = hash_batch_forward_p16(self.geo, data, params, precision, kind, bits, coord=[o], extent=ext, groups_per_field=self._groups(1, ext))
            elif kind == "f32":
                y = hash_batch_forward(self.geo, data, [o], ext, params, self._groups(1, ext))
            else:
                y = hash_batch_forward_source(self.geo, data, params, kind, bits, coord=[o], extent=ext, groups_per_field=self._groups(1, ext))
            out[sl] = y.reshape(self.n_fields, *ext, 3)
        return out

    def _point_groups(self, n: int) -> int:
        """``_groups`` for a launch at ``n`` points per field: a positive ``groups_per_field`` is cut to the grid their wave items admit"""
        if self.groups_per_field == 0:
            return 0
        return min(self.groups_per_field, ((((int(n) + 63) // 64 + 3) // 4) + 7) // 8 * 8)

    @torch.no_grad()
    def query(self, points: torch.Tensor, precision: Optional[str] = None) -> torch.Tensor:
        """[B, N, 3] colours at ``points`` - [N, dim] shared by all fields, or [B, N, dim], each field its own - in ONE launch, from whatever
        table the batch holds (nic_hash_batch_forward_source).  fp32, sample units, clamped like ``HashGridField.query``.  ``precision``: None,
        or "split" / "bf16" - the same launch through ``hash_batch_forward_p16``.  With a level of detail: ``query_lod``."""
        return self._query(points, precision, None)

    @torch.no_grad()
    def query_lod(self, points: torch.Tensor, lod, precision: Optional[str] = None) -> torch.Tensor:
        """``query`` with the level of detail of the query - ``HashGridField.query(lod=)`` of every field in the ONE launch
        (nic_hash_batch_forward_points_lod), from whatever table the batch holds.  ``lod``: a finite float, a tensor [N] shared by all fields or
        [B, N], each field its own: the levels finer than the footprint fade out before the decoder and are not gathered (fade starts
        ``lod_fade``).  ``precision`` other than None is refused, as on the single field."""
        if lod is None:
            raise ValueError("lod is a float or a [N] / [B, N] tensor: without a level of detail call query")
        return self._query(points, precision, lod)

    @torch.no_grad()
    def _query(self, points, precision, lod) -> torch.Tensor:
        """``query`` (``lod`` None: exactly the calls it always made) and ``query_lod``"""
        if precision is not None:
            _check_precision(precision)
            if lod is not None:
                raise NotImplementedError("precision= with a level of detail is not built (DESIGN 7): call without lod, or without precision")
        lod_t, lod_u = (None, 0.0) if lod is None else self._lod_args(lod)
        data, kind, bits = self._table_source()
        n = points.shape[-2] if isinstance(points, torch.Tensor) and points.dim() >= 2 else 0
        params, groups = [p.detach() for p in self.params], self._point_groups(max(n, 1))
        if precision is not None:
            return hash_batch_forward_p16(self.geo, data, params, precision, kind, bits, points=points, groups_per_field=groups)
        if lod is not None:
            return hash_batch_forward_points_lod(self.geo, data, points, params, lod_t, lod_u, self.lod_fade, kind, bits, groups_per_field=groups)
        return hash_batch_forward_source(self.geo, data, params, kind, bits, points=points, groups_per_field=groups)

    @torch.no_grad()
    def point_gradient(self, points: torch.Tensor, dy: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, scale: float = 1.0,
                       counts=None, order=None, lod=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(y [B, N, 3], dpoints [B, N, dim]): ``query(points)`` (``query_lod`` with ``lod``) and the gradient with respect to the point
        COORDINATES - ``HashGridField.point_gradient`` of every field in ONE launch (nic_hash_batch_points_grad), from
        whatever tables the batch holds: a batch from ``load_compressed`` works.  ``points`` [N, dim] shared or [B, N, dim]; exactly one of
        ``dy`` [B, N, 3] (the gradient of sum(y * dy)) and ``target`` [B, N, 3] (of mean((y_b - target_b)^2) * ``scale`` over field b's own
        rows).  ``counts`` / ``order`` (None, "cell" or an int32 [B, N] tensor) as ``train_points``: rows at or past a field's count are zero
        in both outputs.  ``lod``: a finite float, a tensor [N] or [B, N].  The fields' parameters are constants here: no ``.grad`` is
        touched and no optimiser state moves."""
        n = _check_batch_points(self.geo, points, self.n_fields)
        if (dy is None) == (target is None):
            raise ValueError("exactly one of dy and target: the gradient of the output, or the colours of a mean squared error")
        for name, v in (("dy", dy), ("target", target)):
            if v is not None and (not isinstance(v, torch.Tensor) or tuple(v.shape) != (self.n_fields, n, 3)):
                raise ValueError(f"{name} must be [{self.n_fields}, {n}, 3], got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
        counts = _check_batch_counts(counts, self.n_fields, n)
        if isinstance(order, str):
            if order != "cell":
                raise ValueError(f"order {order!r}: None, 'cell' or an int32 [{self.n_fields}, {n}] tensor")
        else:
            order = _check_batch_order(order, self.n_fields, n)
        lod_t, lod_u = (None, 0.0) if lod is None else self._lod_args(lod)
        lod_t = _check_batch_lod(lod_t, self.n_fields, n)
        _point_desc(self.geo)
        _require_on_device(points, "points")
        pts = _stack_points(points, self.n_fields)
        if isinstance(order, str):
            order = hash_batch_point_order(self.geo, pts, counts)
        data, kind, bits = self._table_source()
        return hash_batch_points_grad(self.geo, data, pts, [p.detach() for p in self.params], dy=dy, target=target, loss_scale=float(scale), counts=counts,
                                      order=order, want_y=True, kind=kind, num_bits=bits, lod=lod_t, lod_uniform=lod_u,
                                      fade=None if lod is None else self.lod_fade, groups_per_field=self._point_groups(max(n, 1)))

    def jacobian(self, points: torch.Tensor, lod=None) -> torch.Tensor:
        """[B, N, 3, dim]: d y[b, n, o] / d points[b, n, a], as three ``point_gradient`` calls with a one-hot ``dy``"""
        n = _check_batch_points(self.geo, points, self.n_fields)
        rows = []
        for o in range(3):
            dy = torch.zeros(self.n_fields, n, 3, dtype=torch.float32, device=points.device)
            dy[..., o] = 1.0
            rows.append(self.point_gradient(points, dy=dy, lod=lod)[1])
        return torch.stack(rows, dim=2)

    def query_differentiable(self, points: torch.Tensor, lod=None) -> torch.Tensor:
        """``query(points)`` (``query_lod`` with ``lod``) as a differentiable op of ``points``: the backward hands the output gradient to
        ``point_gradient`` - for shared [N, dim] points summed over the fields - so ``points.requires_grad_()`` works with any torch loss
        and optimiser on the positions or on whatever produced them.  No gradient reaches the fields' parameters through it.  Without
        ``points.requires_grad``, or under ``torch.no_grad()``, it is the plain call."""
        if not (isinstance(points, torch.Tensor) and points.requires_grad and torch.is_grad_enabled()):
            return self.query(points) if lod is None else self.query_lod(points, lod)
        _check_batch_points(self.geo, points, self.n_fields)
        return _BatchQueryPointsFunction.apply(points, self, lod)

    @torch.no_grad()
    def point_gradient_lod(self, points: torch.Tensor, lod, dy: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
                           scale: float = 1.0, counts=None, order=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(y [B, N, 3], dpoints [B, N, dim], dlod [B, N]): ``point_gradient(points, dy, target, scale, counts, order, lod=lod)`` - y and
        dpoints bit for bit - and the gradient of the same loss with respect to the LEVEL OF DETAIL of each point of each field (DESIGN
        4.7.25) - ``HashGridField.point_gradient_lod`` of every field in ONE launch (nic_hash_batch_points_grad_lod), from whatever tables
        the batch holds: a batch from ``load_compressed`` works.  ``lod`` is required: a finite float, a 0-dim tensor, a tensor [N] shared
        by all fields or [B, N].  ``dlod[b, n]`` is the right-hand derivative (a level exactly at its fade start counts, one exactly at its
        end does not), exactly 0 where lambda < 0, >= 32 or NaN and at the rows a field does not own; a point outside the field has the
        clamped point's.  The gradient for a shared ``lod`` is ``dlod.sum(0)``, for a launch-wide one ``dlod.sum()``.  The fields'
        parameters are constants here: no ``.grad`` is touched and no optimiser state moves."""
        n = _check_batch_points(self.geo, points, self.n_fields)
        if (dy is None) == (target is None):
            raise ValueError("exactly one of dy and target: the gradient of the output, or the colours of a mean squared error")
        for name, v in (("dy", dy), ("target", target)):
            if v is not None and (not isinstance(v, torch.Tensor) or tuple(v.shape) != (self.n_fields, n, 3)):
                raise ValueError(f"{name} must be [{self.n_fields}, {n}, 3], got {tuple(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}")
        counts = _check_batch_counts(counts, self.n_fields, n)
        if isinstance(order, str):
            if order != "cell":
                raise ValueError(f"order {order!r}: None, 'cell' or an int32 [{self.n_fields}, {n}] tensor")
        else:
            order = _check_batch_order(order, self.n_fields, n)
        if lod is None:
            raise ValueError("lod is a float or a [N] / [B, N] tensor: the level of detail the gradient is taken at")
        lod_t, lod_u = self._lod_args(lod)
        lod_t = _check_batch_lod(lod_t, self.n_fields, n)
        _point_desc(self.geo)
        _require_on_device(points, "points")
        pts = _stack_points(points, self.n_fields)
        if isinstance(order, str):
            order = hash_batch_point_order(self.geo, pts, counts)
        data, kind, bits = self._table_source()
        return hash_batch_points_grad_lod(self.geo, data, pts, [p.detach() for p in self.params], lod_t, lod_u, self.lod_fade, dy=dy, target=target,
                                          loss_scale=float(scale), counts=counts, order=order, want_y=True, kind=kind, num_bits=bits,
                                          groups_per_field=self._point_groups(max(n, 1)))

    def jacobian_lod(self, points: torch.Tensor, lod) -> torch.Tensor:
        """[B, N, 3]: d y[b, n, o] / d lambda_{b, n}, as three ``point_gradient_lod`` calls with a one-hot ``dy``"""
        n = _check_batch_points(self.geo, points, self.n_fields)
        cols = []
        for o in range(3):
            dy = torch.zeros(self.n_fields, n, 3, dtype=torch.float32, device=points.device)
            dy[..., o] = 1.0
            cols.append(self.point_gradient_lod(points, lod, dy=dy)[2])
        return torch.stack(cols, dim=2)

    def query_differentiable_lod(self, points: torch.Tensor, lod) -> torch.Tensor:
        """``query_lod(points, lod)`` as a differentiable op of ``points`` and / or ``lod`` - a [B, N] tensor, a [N] tensor shared by the
        fields, or a 0-dim tensor (one level of detail for the launch): the backward hands the output gradient to ``point_gradient_lod`` -
        ``dlod`` for a [B, N] ``lod``, its sum over the fields for a shared [N] one, over everything for a 0-dim one; ``dpoints`` summed over
        the fields for shared [N, dim] points - so a zoom, a blur or a mip bias per field can be descended on with any torch loss and
        optimiser.  With nothing that requires a gradient, or under ``torch.no_grad()``, it is the plain ``query_lod`` call.  No gradient
        reaches the fields' parameters through it."""
        wants = any(isinstance(t, torch.Tensor) and t.requires_grad for t in (points, lod))
        if not (wants and torch.is_grad_enabled()):
            return self.query_lod(points, lod)
        _check_batch_points(self.geo, points, self.n_fields)
        return _BatchQueryPointsLodFunction.apply(points, lod, self)

    @torch.no_grad()
    def resample(self, size: Union[int, Sequence[int]], tile: int = 1024, precision: Optional[str] = None) -> torch.Tensor:
        """every field decoded on a regular grid of ANY size, [B, *size, 3]: ``HashGridField.resample``'s sample positions (its
        ``_resample_points``, generated once per tile and shared by all fields), one launch per tile for all fields; ``precision`` as in
        ``query``.  With a level of detail: ``resample_lod``."""
        return self._resample(size, tile, precision, None)

    @torch.no_grad()
    def resample_lod(self, size: Union[int, Sequence[int]], lod="auto", tile: int = 1024, precision: Optional[str] = None) -> torch.Tensor:
        """``resample`` with ``HashGridField.resample(lod=)``'s level of detail for every sample: a float, or "auto" =
        max(0, log2(max_a S_a / size_a)), the footprint of an output sample in octaves.  ``precision`` other than None is refused."""
        if lod is None:
            raise ValueError("lod is 'auto' or a float: without a level of detail call resample")
        return self._resample(size, tile, precision, lod)

    @torch.no_grad()
    def _resample(self, size, tile, precision, lod) -> torch.Tensor:
        """``resample`` (``lod`` None) and ``resample_lod``"""
        if precision is not None:
            _check_precision(precision)
            if lod is not None:
                raise NotImplementedError("precision= with a level of detail is not built (DESIGN 7): call without lod, or without precision")
        size = (int(size),) * self.geo.dim if isinstance(size, int) else tuple(int(v) for v in size)
        if len(size) != self.geo.dim or any(v < 1 for v in size):
            raise ValueError(f"size {size} for a {self.geo.dim}D field")
        if isinstance(lod, str):
            if lod != "auto":
                raise ValueError(f"lod {lod!r}: None, 'auto' or a float")
            lod = max(0.0, math.log2(max(s / v for s, v in zip(self.field_size, size))))
        if lod is not None:
            if isinstance(lod, torch.Tensor) and lod.dim() > 0:
                raise ValueError("resample takes one level of detail for the whole grid: None, 'auto' or a float")
            lod = self._lod_args(lod)[1]
        out = torch.empty(self.n_fields, *size, 3, dtype=torch.float32, device=self.device)
        for o in itertools.product(*[range(0, s, tile) for s in size]):
            ext = [min(tile, s - a) for s, a in zip(size, o)]
            sl = (slice(None), *(slice(a, a + e) for a, e in zip(o, ext)))
            pts = HashGridField._resample_points(self, size, o, ext)
            out[sl] = (self.query(pts, precision) if lod is None else self.query_lod(pts, lod, precision)).reshape(self.n_fields, *ext, 3)
        return out

    @torch.no_grad()
    def decode_mip(self, m: int, tile: int = 1024) -> torch.Tensor:
        """mip ``m`` of every field, [B, S_x / 2^m, S_y / 2^m(, S_z / 2^m), 3]: ``HashGridField.decode_mip``'s points and level of detail m,
        one launch per tile for all fields"""
        return self.resample_lod(self._mip_size(m), float(int(m)), tile=tile)

    def _adam_state(self, p: torch.Tensor):
        st = self.optimizer.state.get(p)
        return st if st else None

    @torch.no_grad()
    def extract(self, b: int) -> "HashGridField":
        """an independent ``HashGridField(fused=True)`` holding copies of field b's table, decoder, codec state (``num_bits``, ``noise_seed``,
        frozen or not), step count, learning rates and Adam moments: ``decode`` / ``query`` / ``resample`` / ``point_gradient`` /
        ``save_compressed`` work on it, and later training of either side does not touch the other.  From a decode-only batch: the
        decode-only field ``HashGridField.load_compressed(path, fused=True)`` makes of field b's file, on copies of its table and decoder"""
        b = self._check_field_index(b)
        if self.decode_only:
            f = HashGridField.__new__(HashGridField)
            f.field_size, f.geo, f.hidden, f.n_linear, f._lod_fade = self.field_size, self.geo, 64, 3, getattr(self, "_lod_fade", None)
            f.num_bits, f.level_bits, f.device = self.num_bits, None, self.device
            f.stored = None if self.stored is None else self.stored[b].clone()
            f.packed = None if self.packed is None else self.packed[b].clone()
            f.table = None
            with torch.random.fork_rng(devices=[]):  # the default init is overwritten: leave the generator alone
                f.decoder = ColorDecoder(self.geo.width, 64, 3).to(self.device)
            for q, p in zip(f.decoder.linear_params(), self.params):
                q.copy_(p[b])
            f.optimizer = f.scheduler = None
            f.noise_seed, f.steps, f.frozen, f._pass_samples, f._grad_clean = 0, 0, True, 0, True
            f._set_route(True)
            return f
        with torch.random.fork_rng(devices=[self.device]):                     # the constructor's random init is overwritten: leave the generators alone
            f = HashGridField(self.field_size, hidden=64, n_linear=3, device=self.device, num_bits=self.num_bits, noise_seed=self.noise_seed, fused=True,
                              lod_fade=getattr(self, "_lod_fade", None), **self._field_args)
        if f.geo != self.geo or f.route != "fused":
            raise RuntimeError("extract(): the single field's geometry differs from the batch's")
        f.table.copy_(self.tables[b])
        for q, p in zip(f.decoder.linear_params(), self.params):
            q.copy_(p[b])
        for gf, gb in zip(f.optimizer.param_groups, self.optimizer.param_groups):
            gf["lr"] = gb["lr"]
        for q, p in zip([f.table] + f.decoder.linear_params(), [self.tables] + self.params):
            st = self._adam_state(p)
            if st is not None:
                f.optimizer.state[q] = {"step": st["step"].clone(), "exp_avg": st["exp_avg"][b].clone(), "exp_avg_sq": st["exp_avg_sq"][b].clone()}
        f.steps = self.steps
        if self.frozen:                              # the table is already quantised: take the state over without quantising again
            f.table.grad = None
            f.table.requires_grad_(False)
            f.frozen = True
        return f

    @torch.no_grad()
    def insert(self, b: int, field: "HashGridField") -> None:
        """copies a compatible ``HashGridField`` into slot b: its table and decoder (and Adam moments, where both sides have them).  The
        geometry, the decoder shape and the codec state (``num_bits``, no bit depth per level, frozen like the batch) must be the batch's, and
        the field must hold an fp32 table (not one from ``load_compressed``): anything else is a ValueError"""
        self._refuse_decode_only("insert")
        b = self._check_field_index(b)
        if not isinstance(field, HashGridField):
            raise TypeError("insert() takes a HashGridField")
        if field.geo != self.geo:
            raise ValueError(f"insert(): the field's geometry {field.geo} is not the batch's {self.geo}")
        if field.hidden != 64 or field.n_linear != 3:
            raise ValueError("insert(): the field's decoder is not 3 Linear layers of 64 hidden units")
        if field.level_bits is not None or field.num_bits != self.num_bits:
            raise ValueError(f"insert(): the field's codec (num_bits {field.num_bits}, level_bits {field.level_bits}) is not the batch's (num_bits {self.num_bits})")
        if field.table is None:
            raise ValueError("insert(): a field from load_compressed holds no fp32 table")
        if bool(field.frozen) != bool(self.frozen):
            raise ValueError(f"insert(): the field is {'frozen' if field.frozen else 'not frozen'}, the batch {'is' if self.frozen else 'is not'}")
        self.tables[b].copy_(field.table.detach().to(self.device))
        for p, q in zip(self.params, field.decoder.linear_params()):
            p[b].copy_(q.detach().to(self.device))
        if field.optimizer is not None:
            for p, q in zip([self.tables] + self.params, [field.table] + field.decoder.linear_params()):
                st, sf = self._adam_state(p), field.optimizer.state.get(q)
                if st is not None and sf:
                    st["exp_avg"][b].copy_(sf["exp_avg"])
                    st["exp_avg_sq"][b].copy_(sf["exp_avg_sq"])

    def save_compressed(self, paths: Sequence, packed: bool = False) -> None:
        """one ordinary single-field file per field (``HashGridField.save_compressed`` of ``extract(b)``; ``HashGridField.load_compressed`` reads
        each): no new format"""
        if self.num_bits is None:
            raise RuntimeError("save_compressed needs num_bits")
        paths = list(paths)
        if len(paths) != self.n_fields:
            raise ValueError(f"{len(paths)} paths for {self.n_fields} fields")
        for b, path in enumerate(paths):
            self.extract(b).save_compressed(path, packed=packed)
