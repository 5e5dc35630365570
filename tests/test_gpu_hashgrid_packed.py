"""GPU tests of the bit-packed hash-grid table (nic_hash_pack_bits / nic_hash_unpack_bits / nic_hash_encode_bits, csrc/hash_grid.hip;
nic_hash_fused_forward_bits, csrc/hash_fused.hip; save_compressed(packed=True), hashgrid.py).  The format of include/nicv2_hip.h is restated here
with numpy's unpackbits / packbits (bitorder="little") over the compact uint8 table, level by level; the kernels must reproduce it byte for byte,
and everything decoded from the packed bits must equal, bit for bit, what the uint8 route decodes.  No tolerance appears anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _geo(field_size, levels, F, log2_table, n_min=16):
    from neural_image_compression_v2_amd.hashgrid import HashGeometry, level_resolutions
    return HashGeometry(tuple(field_size), tuple(level_resolutions(levels, n_min, max(field_size))), F, log2_table)


def _entries(geo):
    return [min((r + 1) ** geo.dim, geo.table_size) for r in geo.resolutions]


def _q_table(geo, num_bits, dev, seed):
    from neural_image_compression_v2_amd import models
    lo, hi = models._q_range(num_bits)
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(geo.table_shape(), generator=g, device=dev) * (hi - lo) + lo


def ref_pack(u8: np.ndarray, geo, b: int) -> np.ndarray:
    """the packed table of a compact uint8 one: per level, the low b bits of every value as one little-endian bit stream, zero bits up to a
    multiple of 32, and 8 zero bytes after the last level"""
    parts, off = [], 0
    for e in _entries(geo):
        vals = u8[off:off + e * geo.features]
        off += e * geo.features
        bits = np.unpackbits(vals[:, None], axis=1, bitorder="little")[:, :b].reshape(-1)
        bits = np.concatenate([bits, np.zeros((-bits.size) % 32, np.uint8)])
        parts.append(np.packbits(bits, bitorder="little"))
    assert off == u8.size
    return np.concatenate(parts + [np.zeros(8, np.uint8)])


def ref_unpack(packed: np.ndarray, geo, b: int) -> np.ndarray:
    parts, off = [], 0
    for e in _entries(geo):
        n = e * geo.features
        nbytes = 4 * ((n * b + 31) // 32)
        bits = np.unpackbits(packed[off:off + nbytes], bitorder="little")[:n * b].reshape(n, b)
        off += nbytes
        parts.append(np.packbits(np.concatenate([bits, np.zeros((n, 8 - b), np.uint8)], axis=1), axis=1, bitorder="little").reshape(-1))
    assert off + 8 == packed.size
    return np.concatenate(parts)


# (field size, levels, F, log2_table, n_min, crop origins, crop extent): dense levels only (2^19), dense and hashed (2^14 in 2D, 2^12 in 3D),
# nearly all hashed (2^10); odd extents, several crops, the far corner of the field
CASES = [((200, 131), 8, F, lg, 16, [[0, 0], [200 - 37, 131 - 21], [64, 3]], (37, 21)) for F in (1, 2, 4, 8) for lg in (10, 14, 19)]
CASES += [((40, 27, 33), 6, F, lg, 4, [[0, 0, 0], [40 - 13, 27 - 10, 33 - 9], [5, 11, 2]], (13, 10, 9)) for F in (1, 2, 4, 8) for lg in (10, 12, 19)]
# square / cubic fields: the crop at the far corner reads vertex (R, .., R), the LAST entry of every dense level
CASES += [((72, 72), 5, F, 19, 6, [[72 - 19, 72 - 19], [0, 0]], (19, 19)) for F in (1, 2, 4, 8)]
CASES += [((24, 24, 24), 4, F, 19, 3, [[24 - 7, 24 - 7, 24 - 7], [0, 0, 0]], (7, 7, 7)) for F in (1, 2, 4, 8)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_pack_unpack_and_encode_match_the_restated_format(dev, case):
    from neural_image_compression_v2_amd.hashgrid import (hash_encode_bits, hash_encode_u8, hash_pack_bits, hash_pack_u8, hash_packed_bytes,
                                                          hash_unpack_bits, level_is_dense)
    size, levels, F, lg, n_min, origins, extent = CASES[case]
    geo = _geo(size, levels, F, lg, n_min)
    dense = [level_is_dense(r, geo.dim, lg) for r in geo.resolutions]
    assert dense[0] and (all(dense) if lg == 19 else not dense[-1])
    E = _entries(geo)
    ragged = False
    for b in range(1, 9):
        ragged = ragged or any((e * F * b) % 32 for e in E)
        table = _q_table(geo, b, dev, seed=1000 + 8 * case + b)
        u8 = hash_pack_u8(geo, table, b)
        assert int(u8.max()) <= (1 << b) - 1                                           # inside the clamp range the byte fits b bits
        want = ref_pack(u8.cpu().numpy(), geo, b)
        n = hash_packed_bytes(geo, b)
        assert want.size == n == 4 * sum((e * F * b + 31) // 32 for e in E) + 8
        buf = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)                    # padding and tail must be WRITTEN as zeros
        packed = hash_pack_bits(geo, table, b, out=buf)
        assert packed is buf
        assert np.array_equal(packed.cpu().numpy(), want), (case, b)
        assert not packed[-8:].any()
        if b == 8:                                                                     # each level's bytes are the uint8 format's
            off_p = off_u = 0
            for e in E:
                assert torch.equal(packed[off_p:off_p + e * F], u8[off_u:off_u + e * F])
                off_p, off_u = off_p + 4 * ((e * F + 3) // 4), off_u + e * F
        back = hash_unpack_bits(geo, packed, b)
        assert torch.equal(back, u8), (case, b)
        assert np.array_equal(ref_unpack(want, geo, b), u8.cpu().numpy())
        got = hash_encode_bits(geo, packed, origins, extent, b)
        assert torch.equal(got, hash_encode_u8(geo, u8, origins, extent, b)), (case, b)
        assert bool(torch.isfinite(got).all())
        assert b == 1 or float(got.abs().max()) > 0                                    # (b = 1 stores 0 for everything below the range's top)
    assert ragged                                                                      # some level ends inside a dword at some b


@pytest.mark.parametrize("dim", [2, 3])
def test_an_unclamped_table_is_stored_masked(dev, dim):
    """outside the clamp range the uint8 value does not fit b bits: the packed table keeps u & (2^b - 1)"""
    from neural_image_compression_v2_amd.hashgrid import hash_pack_bits, hash_pack_u8, hash_unpack_bits
    geo = _geo((200, 131), 6, 2, 12) if dim == 2 else _geo((40, 27, 33), 5, 4, 12, 4)
    g = torch.Generator(device=dev).manual_seed(5)
    table = torch.rand(geo.table_shape(), generator=g, device=dev) * 6 - 3
    for b in range(1, 9):
        u8 = hash_pack_u8(geo, table, b)
        if b < 8:
            assert int(u8.max()) > (1 << b) - 1
        packed = hash_pack_bits(geo, table, b)
        assert np.array_equal(packed.cpu().numpy(), ref_pack(u8.cpu().numpy(), geo, b)), b
        assert torch.equal(hash_unpack_bits(geo, packed, b), u8 & ((1 << b) - 1)), b


def test_encode_bits_4k_first_and_last_entry_of_the_last_level(dev):
    """the bench geometry (11 dense and 5 hashed levels).  The last level is hashed; sample i has base vertex floor((2 i + 1) R / 2 S_max) on
    each axis.  One crop sits on vertex (0, 0) = entry 0, another on a sample whose base vertex hashes to entry T - 1, whose window ends in the
    8 tail bytes."""
    from neural_image_compression_v2_amd.hashgrid import hash_encode_bits, hash_encode_u8, hash_pack_bits, hash_pack_u8, hash_packed_bytes, hash_unpack_bits
    geo = _geo((3840, 2160), 16, 2, 19)
    T, R = geo.table_size, geo.resolutions[-1]
    assert (R + 1) ** 2 > T
    bx = ((2 * np.arange(3840, dtype=np.uint64) + 1) * np.uint64(R)) // np.uint64(2 * 3840)
    by = ((2 * np.arange(2160, dtype=np.uint64) + 1) * np.uint64(R)) // np.uint64(2 * 3840)
    vx, vy = np.meshgrid(bx, by, indexing="ij")
    h = ((vx ^ (vy * np.uint64(2654435761))) & np.uint64(0xFFFFFFFF)) & np.uint64(T - 1)
    hit = np.argwhere(h == T - 1)
    assert len(hit) > 0
    x, y = (int(v) for v in hit[len(hit) // 2])
    ext = (24, 16)
    org_last = [min(max(x - 5, 0), 3840 - ext[0]), min(max(y - 5, 0), 2160 - ext[1])]
    assert org_last[0] <= x < org_last[0] + ext[0] and org_last[1] <= y < org_last[1] + ext[1]
    assert int(h[0, 0]) == 0
    origins = [[0, 0], org_last, [3840 - ext[0], 2160 - ext[1]]]
    for b, nbytes in [(8, 6_717_776), (4, 3_358_900), (1, 839_748), (3, 2_519_180)]:
        table = _q_table(geo, b, dev, seed=40 + b)
        u8 = hash_pack_u8(geo, table, b)
        packed = hash_pack_bits(geo, table, b)
        assert packed.numel() == nbytes == hash_packed_bytes(geo, b)
        assert torch.equal(hash_unpack_bits(geo, packed, b), u8)
        assert torch.equal(hash_encode_bits(geo, packed, origins, ext, b), hash_encode_u8(geo, u8, origins, ext, b)), b
    # the whole field in one launch, at the straddling depth
    assert torch.equal(hash_encode_bits(geo, packed, [[0, 0]], (3840, 2160), 3), hash_encode_u8(geo, u8, [[0, 0]], (3840, 2160), 3))


def _decoder(geo, dev, seed):
    from neural_image_compression_v2_amd.image_compression import ColorDecoder
    torch.manual_seed(seed)
    dec = ColorDecoder(geo.width, 64, 3).to(dev)
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(1.5)
    return [p.detach().clone() for p in dec.linear_params()]


# every (D, F, L F <= 32 / L F > 32) the fused kernels exist for (F = 1 cannot pass 32 columns: at most 32 levels)
FUSED_CASES = [(dim, F, L) for dim in (2, 3) for F, Ls in ((1, (16,)), (2, (8, 24)), (4, (4, 12)), (8, (2, 6))) for L in Ls]


@pytest.mark.parametrize("dim,F,L", FUSED_CASES)
def test_fused_forward_bits_equals_fused_forward_u8(dev, dim, F, L):
    from neural_image_compression_v2_amd.hashgrid import hash_fused_forward_bits, hash_fused_forward_u8, hash_fused_supported, hash_pack_bits, hash_pack_u8
    if dim == 2:
        extent, origins, geo = (37, 29), [[3, 5], [163, 121], [0, 0]], _geo((200, 150), L, F, 12, 8)
    else:
        extent, origins, geo = (13, 10, 9), [[0, 0, 0], [27, 17, 24], [5, 11, 2]], _geo((40, 27, 33), L, F, 12, 3)
    assert hash_fused_supported(geo) and (L * F > 32) == (L in (24, 12, 6))
    params = _decoder(geo, dev, seed=L + F)
    for b in range(1, 9):
        table = _q_table(geo, b, dev, seed=77 + b)
        y_bits = hash_fused_forward_bits(geo, hash_pack_bits(geo, table, b), origins, extent, b, params)
        y_u8 = hash_fused_forward_u8(geo, hash_pack_u8(geo, table, b), origins, extent, b, params)
        assert torch.equal(y_bits, y_u8), (dim, F, L, b)
        assert b == 1 or float(y_bits.std()) > 0


def _structured_image(size, dev):
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.25 * torch.sin(7 * x + 3 * y) + 0.15 * torch.sin(41 * x) * torch.cos(37 * y),
                        0.5 + 0.25 * torch.cos(20 * x * y) + 0.15 * torch.sin(60 * (x - y) ** 2),
                        0.5 + 0.2 * torch.sin(13 * y - 2 * x) + 0.1 * torch.sign(torch.sin(9 * x + 11 * y))], dim=-1)
    return base.clamp(0, 1)


def _child_decode(path, out, fused, tile):
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); from neural_image_compression_v2_amd.hashgrid import HashGridField; "
            "f = HashGridField.load_compressed(sys.argv[2], 'cuda:0', fused=sys.argv[4] == '1'); assert f.packed is not None and f.stored is None; "
            "torch.save(f.decode(tile=int(sys.argv[5])).cpu(), sys.argv[3])")
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(path), str(out), "1" if fused else "0", str(tile)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out, weights_only=True)


@pytest.mark.parametrize("which", ["2d_b4", "3d_b8"])
def test_field_saves_loads_and_decodes_packed(dev, tmp_path, monkeypatch, which):
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGridField, hash_packed_bytes, hash_stored_bytes, hash_unpack_bits
    if which == "2d_b4":
        size, b, tile = (256, 256), 4, 96
        target = _structured_image(size, dev)
        field = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=1, num_bits=b)
        epochs = 40
    else:
        n, b, tile = 40, 8, 24
        ax = torch.linspace(0, 1, n, device=dev)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        target = torch.stack([0.5 + 0.3 * torch.sin(6 * x + 2 * z), 0.5 + 0.3 * torch.cos(4 * y - 3 * z), 0.5 + 0.25 * torch.sin(5 * (x + y + z))], dim=-1)
        size = (n, n, n)
        field = HashGridField(size, levels=6, features=2, log2_table=14, base_resolution=4, device=dev, seed=2, num_bits=b)
        epochs = 30
    field.set_schedule(epochs)
    hist = field.fit(target, epochs)
    assert field.frozen and hist[-1] < hist[0]
    p_u8, p_bits = tmp_path / "u8.pt", tmp_path / "bits.pt"
    field.save_compressed(p_u8)
    field.save_compressed(p_bits, packed=True)
    d_u8 = torch.load(p_u8, map_location="cpu", weights_only=True)
    d_bits = torch.load(p_bits, map_location="cpu", weights_only=True)
    assert d_u8["format"] == "nicv2-hashgrid-u8/1" and d_bits["format"] == "nicv2-hashgrid-bits/1"
    assert d_bits["table"].dtype == torch.uint8 and d_bits["num_bits"] == b
    assert d_bits["table"].numel() == hash_packed_bytes(field.geo, b) == field.stored_bytes(packed=True)["table"]
    assert d_u8["table"].numel() == hash_stored_bytes(field.geo) == field.stored_bytes()["table"]
    assert field.stored_bytes(packed=True)["decoder"] == field.stored_bytes()["decoder"]
    if b == 4:
        assert field.stored_bytes(packed=True)["table"] == 21_368                          # about half the uint8 table's bytes
        assert field.stored_bytes()["table"] > 42_000
    assert np.array_equal(d_bits["table"].numpy(), ref_pack(d_u8["table"].numpy(), field.geo, b))
    # a uint8 file loads and decodes as before: exactly the frozen field's image, on each route
    mem = field.decode(tile=tile)
    for fused in (False, True):
        from_u8 = HashGridField.load_compressed(p_u8, dev, fused=fused)
        assert from_u8.packed is None and from_u8.stored is not None and from_u8.route == ("fused" if fused else "layerwise")
        ref = from_u8.decode(tile=tile)
        if not fused:
            assert torch.equal(ref, mem)
        # the packed file decodes to the same bits, and never through a uint8 or fp32 table
        loaded = HashGridField.load_compressed(p_bits, dev, fused=fused)
        assert loaded.table is None and loaded.stored is None and loaded.packed.numel() == hash_packed_bytes(field.geo, b)
        assert loaded.route == from_u8.route

        def boom(*a, **k):
            raise AssertionError("a packed field must decode from the packed bits")
        with monkeypatch.context() as mp:
            for name in ("hash_encode_u8", "hash_fused_forward_u8", "hash_encode", "hash_fused_forward", "hash_unpack_bits", "_table_of_u8"):
                mp.setattr(hashgrid, name, boom)
            got = loaded.decode(tile=tile)
        assert torch.equal(got, ref), (which, fused)
        assert torch.equal(_child_decode(p_bits, tmp_path / f"child{int(fused)}.pt", fused, tile), ref.cpu()), (which, fused)
    # packed -> load -> save as uint8 reproduces the uint8 file's table; uint8 -> load -> save packed reproduces the packed one
    loaded.save_compressed(tmp_path / "back_u8.pt")
    back = torch.load(tmp_path / "back_u8.pt", map_location="cpu", weights_only=True)
    assert back["format"] == "nicv2-hashgrid-u8/1" and torch.equal(back["table"], d_u8["table"])
    assert torch.equal(hash_unpack_bits(loaded.geo, loaded.packed, b).cpu(), d_u8["table"])
    loaded.save_compressed(tmp_path / "again_bits.pt", packed=True)
    assert torch.equal(torch.load(tmp_path / "again_bits.pt", map_location="cpu", weights_only=True)["table"], d_bits["table"])
    from_u8.save_compressed(tmp_path / "u8_to_bits.pt", packed=True)
    assert torch.equal(torch.load(tmp_path / "u8_to_bits.pt", map_location="cpu", weights_only=True)["table"], d_bits["table"])
    for k, v in d_u8["decoder"].items():
        assert torch.equal(back["decoder"][k], v)
    with pytest.raises(RuntimeError):
        loaded.train_step([[0] * len(size)], size, target.reshape(-1, 3))
