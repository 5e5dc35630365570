"""Reference decoder of the stored hash-grid files, starting from the BYTES (test infrastructure).

Plain CPU code in float64 and Python / int64 integers, written from the contract comments of ``include/nicv2_hip.h`` (``nic_hash_desc``, the
codec sections of the uint8, ``bits/1`` and ``bits/2`` tables, the "arbitrary points" section) and from nothing else: it imports nothing of
``neural_image_compression_v2_amd``, so it cannot inherit a mistake of the package, and it shares no code with ``ref_pack`` / ``ref_unpack`` of
``tests/test_gpu_hashgrid_packed.py``.

A *file* is the dict ``HashGridField.save_compressed`` hands to ``torch.save`` (``make_file`` builds one on the CPU, ``save`` writes it);
``read_file`` / ``parse`` turn it into a ``StoredFile``: geometry and depths as Python ints, the table as a uint8 numpy array exactly as
stored, the decoder as float64 arrays.  From there: ``table_values`` (bytes -> dequantised float64 entries per level, with every length,
padding-bit and tail-byte check of the format), ``entry_index``, ``rows_lattice`` / ``rows_points`` (the [N, L F] encoding), ``decoder``, and
``decode`` / ``query`` / ``resample``.

Everything that reaches a fixture is evaluated in an order that does not depend on a BLAS or on vector widths: products are accumulated
column by column with elementwise float64 operations, erf and exp are the C library's scalar functions.  The fixtures under
``tests/golden/hashgrid/`` therefore also hold this module still (``tests/test_hashgrid_stored_ref_cpu.py`` regenerates them bit for bit)."""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

FORMAT_U8 = "nicv2-hashgrid-u8/1"
FORMAT_BITS = "nicv2-hashgrid-bits/1"
FORMAT_MIXED = "nicv2-hashgrid-bits/2"
FORMATS = (FORMAT_U8, FORMAT_BITS, FORMAT_MIXED)
PRIME_Y, PRIME_Z = 2654435761, 805459861
TAIL_BYTES = 8


# ------------------------------------------------------------------------------------------------------------------ the file

@dataclass(frozen=True)
class StoredFile:
    format: str
    field_size: Tuple[int, ...]          # (S_x, S_y(, S_z))
    resolutions: Tuple[int, ...]         # R_l
    features: int
    log2_table: int
    num_bits: Optional[int]              # u8/1 and bits/1
    level_bits: Optional[Tuple[int, ...]]    # bits/2
    hidden: int
    n_linear: int
    table: np.ndarray                    # uint8 [bytes], as stored
    weights: Tuple[np.ndarray, ...]      # float64 [out, in] per Linear layer
    biases: Tuple[np.ndarray, ...]       # float64 [out]

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

    def bits_of_level(self, l: int) -> int:
        return self.level_bits[l] if self.format == FORMAT_MIXED else self.num_bits


def parse(d: dict) -> StoredFile:
    """the dict of a stored file as a ``StoredFile``; refuses what is not such a dict (ValueError)"""
    if not isinstance(d, dict) or d.get("format") not in FORMATS:
        raise ValueError(f"not a hash-grid file: format {d.get('format') if isinstance(d, dict) else type(d).__name__!r}")
    fmt = d["format"]
    field_size = tuple(int(v) for v in d["field_size"])
    resolutions = tuple(int(r) for r in d["resolutions"])
    features, log2_table, hidden, n_linear = int(d["features"]), int(d["log2_table"]), int(d["hidden"]), int(d["n_linear"])
    if len(field_size) not in (2, 3) or min(field_size) < 1 or not resolutions or min(resolutions) < 1:
        raise ValueError(f"geometry: field {field_size}, resolutions {resolutions}")
    if features not in (1, 2, 4, 8) or not 10 <= log2_table <= 24 or hidden < 1 or not 2 <= n_linear <= 5:
        raise ValueError(f"features {features}, log2_table {log2_table}, hidden {hidden}, n_linear {n_linear}")
    num_bits = level_bits = None
    if fmt == FORMAT_MIXED:
        if d.get("num_bits") is not None:
            raise ValueError("a bits/2 file stores num_bits None")
        level_bits = tuple(int(b) for b in d["level_bits"])
        if len(level_bits) != len(resolutions) or any(not 1 <= b <= 8 for b in level_bits):
            raise ValueError(f"level_bits {level_bits} for {len(resolutions)} levels")
    else:
        num_bits = int(d["num_bits"])
        if not 1 <= num_bits <= 8:
            raise ValueError(f"num_bits {num_bits}")
    t = d["table"]
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
        raise ValueError("the table is a 1-D uint8 tensor")
    dec = d["decoder"]
    if sorted(dec) != sorted(f"decoder.{2 * i}.{p}" for i in range(n_linear) for p in ("weight", "bias")):
        raise ValueError(f"decoder keys {sorted(dec)} for {n_linear} Linear layers")
    weights, biases = [], []
    width = len(resolutions) * features
    for i in range(n_linear):
        w, b = dec[f"decoder.{2 * i}.weight"], dec[f"decoder.{2 * i}.bias"]
        want = (hidden if i < n_linear - 1 else 3, width if i == 0 else hidden)
        if w.dtype != torch.float32 or b.dtype != torch.float32 or tuple(w.shape) != want or tuple(b.shape) != want[:1]:
            raise ValueError(f"decoder layer {i}: weight {tuple(w.shape)} {w.dtype}, bias {tuple(b.shape)} {b.dtype}, expected {want} float32")
        weights.append(w.numpy().astype(np.float64))
        biases.append(b.numpy().astype(np.float64))
    return StoredFile(fmt, field_size, resolutions, features, log2_table, num_bits, level_bits, hidden, n_linear,
                      t.numpy().copy(), tuple(weights), tuple(biases))


def read_file(path) -> StoredFile:
    return parse(torch.load(path, map_location="cpu", weights_only=True))


def save(d: dict, path) -> None:
    torch.save(d, path)


# ------------------------------------------------------------------------------------------------------------------ geometry

def level_resolutions(levels: int, n_min: float, n_max: float) -> List[int]:
    """R_l = floor(n_min b^l), b = exp((ln n_max - ln n_min) / (levels - 1)), in float64"""
    if levels == 1:
        return [int(math.floor(n_min))]
    b = math.exp((math.log(n_max) - math.log(n_min)) / (levels - 1))
    return [int(math.floor(n_min * b ** l)) for l in range(levels)]


def level_entries(f, l: int) -> int:
    """E_l = min((R_l + 1)^dim, T)"""
    return min((f.resolutions[l] + 1) ** f.dim, f.table_size)


def level_dense(f, l: int) -> bool:
    return (f.resolutions[l] + 1) ** f.dim <= f.table_size


def level_dwords(f, l: int) -> int:
    """ceil(E_l F b_l / 32)"""
    return -(-level_entries(f, l) * f.features * f.bits_of_level(l) // 32)


def table_bytes(f) -> int:
    """the length the format's formula gives for this geometry"""
    if f.format == FORMAT_U8:
        return f.features * sum(level_entries(f, l) for l in range(f.levels))
    return 4 * sum(level_dwords(f, l) for l in range(f.levels)) + TAIL_BYTES


def level_offset(f, l: int) -> int:
    """the byte level l starts at"""
    if f.format == FORMAT_U8:
        return f.features * sum(level_entries(f, k) for k in range(l))
    return 4 * sum(level_dwords(f, k) for k in range(l))


def entry_index(f, level: int, v: np.ndarray) -> np.ndarray:
    """the entry of vertices v [..., dim] (int64, >= 0) at ``level``: dense v_x + (R + 1)(v_y + (R + 1) v_z) when (R + 1)^dim <= T, otherwise
    (v_x * 1) ^ (v_y * 2654435761) ^ (v_z * 805459861) in wrapping uint32; both & (T - 1)"""
    v = np.asarray(v, dtype=np.int64)
    r1 = f.resolutions[level] + 1
    vx, vy = v[..., 0], v[..., 1]
    vz = v[..., 2] if f.dim == 3 else np.zeros_like(vx)
    if level_dense(f, level):
        idx = vx + r1 * (vy + r1 * vz)
    else:
        m = 0xFFFFFFFF
        idx = (vx & m) ^ ((vy * PRIME_Y) & m) ^ ((vz * PRIME_Z) & m)      # v < 2^31 and the primes < 2^32: the products fit int64
    return idx & (f.table_size - 1)


# ------------------------------------------------------------------------------------------------------------------ bytes -> values

def _level_codes(f, l: int) -> np.ndarray:
    """the stored integers u [E_l, F] of level l, read from the bytes"""
    e, F, b = level_entries(f, l), f.features, f.bits_of_level(l)
    off = level_offset(f, l)
    if f.format == FORMAT_U8:
        return f.table[off:off + e * F].astype(np.int64).reshape(e, F)
    raw = f.table.astype(np.int64)
    pos = np.arange(e * F, dtype=np.int64) * b                  # first bit of value j in the level's stream
    k = off + (pos >> 3)
    window = raw[k] | (raw[k + 1] << 8)                         # b <= 8 and a shift <= 7: two bytes hold the value (the tail keeps k + 1 inside)
    return ((window >> (pos & 7)) & ((1 << b) - 1)).reshape(e, F)


def check_layout(f) -> None:
    """the length equals the format's formula; u8: every code fits its depth; packed: every padding bit and the 8 trailing bytes are zero"""
    need = table_bytes(f)
    if f.table.shape[0] != need:
        raise ValueError(f"the table holds {f.table.shape[0]} bytes, a {f.format} file of this geometry holds {need}")
    if f.format == FORMAT_U8:
        if int(f.table.max(initial=0)) > (1 << f.num_bits) - 1:
            raise ValueError(f"a stored byte exceeds 2^{f.num_bits} - 1")
        return
    for l in range(f.levels):
        used = level_entries(f, l) * f.features * f.bits_of_level(l)
        stream = np.unpackbits(f.table[level_offset(f, l):level_offset(f, l) + 4 * level_dwords(f, l)], bitorder="little")
        if stream[used:].any():
            raise ValueError(f"level {l}: a padding bit is set")
    if f.table[need - TAIL_BYTES:].any():
        raise ValueError("the 8 trailing bytes are not zero")


def table_codes(f) -> List[np.ndarray]:
    check_layout(f)
    return [_level_codes(f, l) for l in range(f.levels)]


def table_values(f) -> List[np.ndarray]:
    """per level an [E_l, F] float64 array: (u - 2^(b-1) + 1) / (2^b - 1), from the bytes"""
    out = []
    for l, u in enumerate(table_codes(f)):
        b = f.bits_of_level(l)
        out.append((u - (1 << (b - 1)) + 1).astype(np.float64) / float((1 << b) - 1))
    return out


# ------------------------------------------------------------------------------------------------------------------ positions -> rows

def _blend(f, values: List[np.ndarray], cells: List[Tuple[np.ndarray, np.ndarray]]) -> np.ndarray:
    """[N, L F]: column l F + f = sum over the 2^dim corners c of prod_a (c_a ? w_a : 1 - w_a) value[l][idx(v + c), f]; cells[l] = (v, w),
    both [N, dim]"""
    n = cells[0][0].shape[0]
    out = np.zeros((n, f.levels * f.features), dtype=np.float64)
    for l, (v, w) in enumerate(cells):
        acc = np.zeros((n, f.features), dtype=np.float64)
        for c in itertools.product((0, 1), repeat=f.dim):
            idx = entry_index(f, l, v + np.array(c, dtype=np.int64))
            if int(idx.max()) >= values[l].shape[0]:
                raise AssertionError(f"level {l}: entry {int(idx.max())} of {values[l].shape[0]}")
            cw = np.ones(n, dtype=np.float64)
            for a in range(f.dim):
                cw = cw * (w[:, a] if c[a] else 1.0 - w[:, a])
            acc = acc + cw[:, None] * values[l][idx]
        out[:, l * f.features:(l + 1) * f.features] = acc
    return out


def rows_lattice(f, origin: Sequence[int], extent: Sequence[int]) -> np.ndarray:
    """[N, L F] of the crop ``origin`` .. ``origin + extent``, samples x-outer .. last axis inner: q = (2 i + 1) R_l,
    v = q // (2 S_max), w = (q % (2 S_max)) / (2 S_max)"""
    axes = [np.arange(o, o + e, dtype=np.int64) for o, e in zip(origin, extent)]
    i = np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], axis=1)
    if (i < 0).any() or (i >= np.array(f.field_size)).any():
        raise ValueError("the crop leaves the field")
    den = 2 * f.s_max
    cells = []
    for r in f.resolutions:
        q = (2 * i + 1) * r
        cells.append((q // den, (q % den).astype(np.float64) / den))
    return _blend(f, table_values(f), cells)


def fixed_point(f, points_fp32: np.ndarray) -> np.ndarray:
    """t [N, dim] int64: the fp32 points as given, widened; clamped to [-1/2, S_a - 1/2] (NaN -> the low edge, +-inf -> the nearer edge);
    t = rint(256 p) + 128 (half to even), clamped to [0, 256 S_a - 1]"""
    p = np.asarray(points_fp32)
    if p.dtype != np.float32 or p.ndim != 2 or p.shape[1] != f.dim:
        raise ValueError(f"points are fp32 [N, {f.dim}]")
    p = p.astype(np.float64)
    t = np.empty(p.shape, dtype=np.int64)
    for a, s in enumerate(f.field_size):
        pa = np.where(np.isnan(p[:, a]), -0.5, p[:, a])
        pa = np.minimum(np.maximum(pa, -0.5), s - 0.5)
        ta = np.rint(256.0 * pa).astype(np.int64) + 128
        t[:, a] = np.minimum(np.maximum(ta, 0), 256 * s - 1)
    return t


def rows_points(f, points_fp32: np.ndarray) -> np.ndarray:
    """[N, L F] at fp32 points in sample units: q = t R_l, v = q // (256 S_max), w = (q % (256 S_max)) / (256 S_max)"""
    t = fixed_point(f, points_fp32)
    den = 256 * f.s_max
    cells = []
    for r in f.resolutions:
        q = t * r
        cells.append((q // den, (q % den).astype(np.float64) / den))
    return _blend(f, table_values(f), cells)


# ------------------------------------------------------------------------------------------------------------------ the decoder

_erf = np.vectorize(math.erf, otypes=[np.float64])
_exp = np.vectorize(math.exp, otypes=[np.float64])


def _linear(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """x W^T + b, summed over the input columns in their order with elementwise float64 operations"""
    z = np.zeros((x.shape[0], w.shape[0]), dtype=np.float64)
    for k in range(w.shape[1]):
        z = z + x[:, k:k + 1] * w[None, :, k]
    return z + b[None, :]


def decoder(rows: np.ndarray, f) -> np.ndarray:
    """[N, 3]: Linear, exact-erf GELU, .., Linear, sigmoid, in float64, for the ``hidden`` and ``n_linear`` the file names"""
    a = np.asarray(rows, dtype=np.float64)
    for i in range(f.n_linear):
        z = _linear(a, f.weights[i], f.biases[i])
        if i < f.n_linear - 1:
            a = 0.5 * z * (1.0 + _erf(z / math.sqrt(2.0)))
        else:
            a = 1.0 / (1.0 + _exp(-z))
    return a


# ------------------------------------------------------------------------------------------------------------------ the three routes

def decode(f) -> np.ndarray:
    """the whole field [S_x, S_y(, S_z), 3]"""
    return decoder(rows_lattice(f, (0,) * f.dim, f.field_size), f).reshape(*f.field_size, 3)


def query(f, points_fp32: np.ndarray) -> np.ndarray:
    """[N, 3] at fp32 points [N, dim]"""
    return decoder(rows_points(f, points_fp32), f)


def sample_centres(f) -> np.ndarray:
    """fp32 [prod S, dim]: p = i for every sample, in ``decode``'s order"""
    axes = [np.arange(s, dtype=np.float32) for s in f.field_size]
    return np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], axis=1)


def resample_points(f, size: Sequence[int]) -> np.ndarray:
    """fp32 [prod size, dim], the last axis fastest: p_a = ((j + 0.5) * S_a / size_a - 0.5) in float64, in this order of operations, then
    ONE rounding to fp32 - the rounded value is what enters the fixed-point step"""
    if len(size) != f.dim or any(int(n) < 1 for n in size):
        raise ValueError(f"size {tuple(size)} for a {f.dim}D field")
    axes = [((np.arange(int(n), dtype=np.float64) + 0.5) * s / int(n) - 0.5).astype(np.float32) for s, n in zip(f.field_size, size)]
    return np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], axis=1)


def resample(f, size: Sequence[int]) -> np.ndarray:
    """the field on a regular grid of ``size`` samples, [*size, 3]"""
    return query(f, resample_points(f, size)).reshape(*[int(n) for n in size], 3)


# ------------------------------------------------------------------------------------------------------------------ the writer

def code_formula(seed: int, level: int, n_entries: int, features: int, bits: int) -> np.ndarray:
    """codes u [E, F] in [0, 2^b - 1]: an integer mix of (seed, level, entry, feature) in wrapping uint32, no RNG; the top bits are kept"""
    m = np.uint64(0xFFFFFFFF)
    e = np.arange(n_entries, dtype=np.uint64)[:, None]
    ft = np.arange(features, dtype=np.uint64)[None, :]
    h = (np.uint64(seed) * np.uint64(0x9E3779B1) + np.uint64(level) * np.uint64(0x85EBCA77) + e * np.uint64(0xC2B2AE3D)
         + ft * np.uint64(0x27D4EB2F) + np.uint64(0x165667B1)) & m
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x7FEB352D)) & m
    h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x846CA68B)) & m
    h = h ^ (h >> np.uint64(16))
    return (h >> np.uint64(32 - bits)).astype(np.int64)


def pack_codes(fmt: str, codes: List[np.ndarray], bits: Sequence[int]) -> np.ndarray:
    """the stored bytes of per-level codes [E_l, F] (this module's own restatement of the three layouts).  u8/1: the bytes back to back.
    bits/1, bits/2: per level a little-endian bit stream (value j at bits [j b_l, (j + 1) b_l), least significant bit first, bit k of the
    stream = bit k & 7 of byte k >> 3), padded with zero bits to whole dwords; 8 zero bytes after the last level"""
    if fmt == FORMAT_U8:
        return np.concatenate([u.reshape(-1) for u in codes]).astype(np.uint8)
    parts = []
    for u, b in zip(codes, bits):
        flat = u.reshape(-1).astype(np.int64)
        stream = ((flat[:, None] >> np.arange(b, dtype=np.int64)[None, :]) & 1).astype(np.uint8).reshape(-1)
        stream = np.concatenate([stream, np.zeros(-stream.shape[0] % 32, dtype=np.uint8)])
        parts.append(np.packbits(stream, bitorder="little"))
    parts.append(np.zeros(TAIL_BYTES, dtype=np.uint8))
    return np.concatenate(parts)


def make_decoder(width: int, hidden: int, n_linear: int, seed: int, scale: float) -> Dict[str, torch.Tensor]:
    """``torch.manual_seed(seed)``, then nn.Linear's default initialisation layer by layer, every tensor times ``scale``; keys as the
    package's ColorDecoder state dict (``decoder.{0, 2, ..}.{weight, bias}``)"""
    torch.manual_seed(seed)
    dims = [width] + [hidden] * (n_linear - 1) + [3]
    out = {}
    for i in range(n_linear):
        lin = torch.nn.Linear(dims[i], dims[i + 1])
        out[f"decoder.{2 * i}.weight"] = (lin.weight.detach() * scale).contiguous()
        out[f"decoder.{2 * i}.bias"] = (lin.bias.detach() * scale).contiguous()
    return out


def make_file(spec: dict, seed: int) -> dict:
    """the dict of a stored file, built on the CPU.  ``spec``: field_size, levels, base (R_0; the finest level is max(field_size)),
    features, log2_table, fmt ("u8" | "bits1" | "bits2"), bits (an int, or a depth per level for "bits2"), hidden, n_linear, scale"""
    field_size = tuple(int(s) for s in spec["field_size"])
    res = level_resolutions(int(spec["levels"]), spec["base"], max(field_size))
    F, T, dim = int(spec["features"]), 1 << int(spec["log2_table"]), len(field_size)
    fmt = {"u8": FORMAT_U8, "bits1": FORMAT_BITS, "bits2": FORMAT_MIXED}[spec["fmt"]]
    bits = [int(b) for b in spec["bits"]] if fmt == FORMAT_MIXED else [int(spec["bits"])] * len(res)
    codes = [code_formula(seed, l, min((r + 1) ** dim, T), F, bits[l]) for l, r in enumerate(res)]
    d = {"format": fmt, "field_size": list(field_size), "resolutions": list(res), "features": F, "log2_table": int(spec["log2_table"]),
         "num_bits": None if fmt == FORMAT_MIXED else bits[0]}
    if fmt == FORMAT_MIXED:
        d["level_bits"] = list(bits)
    d.update({"hidden": int(spec["hidden"]), "n_linear": int(spec["n_linear"]), "table": torch.from_numpy(pack_codes(fmt, codes, bits)),
              "decoder": make_decoder(len(res) * F, int(spec["hidden"]), int(spec["n_linear"]), seed, float(spec["scale"]))})
    return d


def with_codes(d: dict, codes: List[np.ndarray]) -> dict:
    """a copy of the file dict ``d`` with its table replaced by the packed ``codes`` (same format and depths)"""
    f = parse(d)
    out = dict(d)
    out["table"] = torch.from_numpy(pack_codes(f.format, codes, [f.bits_of_level(l) for l in range(f.levels)]))
    return out
