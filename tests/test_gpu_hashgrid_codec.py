"""GPU tests of the hash-grid codec (nic_hash_encode_noisy / nic_hash_encode_u8 / nic_hash_pack_u8, csrc/hash_grid.hip; HashGridField(num_bits=b),
hashgrid.py).  The noise is restated on the host from the oracle's Threefry (oracle/nic_oracle.py::threefry4x32, 12 rounds) and must match bit
for bit; the uint8 gather must equal the fp32 gather of load4fp(save4fp(table)) bit for bit and the compact pack must equal save4fp cut to each
level's first E_l entries; a stored file decodes, in this process and in a fresh one, to exactly the frozen field's image; the chunks of one pass
never share noise; num_bits=None trains as before; and quantisation-aware fits in 2D and 3D."""
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


def host_noise(n, width, num_bits, seed, offset, sample_base):
    """the noise of include/nicv2_hip.h (nic_hash_quant) restated: column c is value c & 15 of Threefry-4x32-12 block c >> 4 of sample
    sample_base + row; value i = byte i & 3 of word i >> 2, u8 -> ((u8 + 1/2) / 256 - 1/2) 2^-b"""
    from oracle import nic_oracle as O
    nblk = (width + 15) // 16
    ctr = O._noise_counters(n, nblk, offset, sample_base)
    r = O.threefry4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, O.KERNEL_NOISE_TWEAK, 0), rounds=12)      # [n, nblk, 4]
    c = np.arange(width)
    i = c & 15
    words = r[:, c >> 4, i >> 2]                                                                                    # [n, width]
    u8 = ((words >> (np.uint32(8) * (i & 3).astype(np.uint32))[None, :]) & np.uint32(255)).astype(np.float32)
    u = (u8 + np.float32(0.5)) * np.float32(1.0 / 256.0) - np.float32(0.5)
    return torch.from_numpy((u * np.float32(2.0 ** -num_bits)).astype(np.float32))


def sample_coords(origins, extent, device):
    """[N, d] int64 sample coordinates in nic_encode order: crops back to back, the last axis fastest"""
    grids = torch.meshgrid(*[torch.arange(int(e), device=device) for e in extent], indexing="ij")
    local = torch.stack([g.reshape(-1) for g in grids], dim=1)
    org = torch.as_tensor(origins, dtype=torch.int64, device=device).reshape(-1, len(extent))
    return (org[:, None, :] + local[None]).reshape(-1, len(extent))


def _q_table(geo, num_bits, dev, seed):
    from neural_image_compression_v2_amd import models
    lo, hi = models._q_range(num_bits)
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(geo.table_shape(), generator=g, device=dev) * (hi - lo) + lo


def psnr(a, b):
    return float(10 * torch.log10(1.0 / ((a.double() - b.double()) ** 2).mean()))


# ---- 1. noisy encode, bit-exact
NOISY_CASES = [((200, 131), 5, F, 19, 16, [[0, 0], [200 - 37, 131 - 21], [64, 3]], (37, 21)) for F in (1, 2, 4, 8)]
NOISY_CASES += [((40, 27, 33), 5, F, 12, 4, [[0, 0, 0], [40 - 13, 27 - 10, 33 - 9], [5, 11, 2]], (13, 10, 9)) for F in (1, 2, 4, 8)]
NOISY_CASES += [((96, 80), 32, 8, 14, 2, [[3, 1], [96 - 29, 80 - 17]], (29, 17))]                   # 32 x 8 columns: 16 blocks per sample


@pytest.mark.parametrize("num_bits", [2, 8])
@pytest.mark.parametrize("case", range(len(NOISY_CASES)))
def test_noisy_encode_is_clean_plus_host_noise(dev, case, num_bits):
    from neural_image_compression_v2_amd.hashgrid import hash_encode, hash_encode_noisy
    size, levels, F, lg, n_min, origins, extent = NOISY_CASES[case]
    geo = _geo(size, levels, F, lg, n_min)
    table = _q_table(geo, num_bits, dev, seed=case)
    clean = hash_encode(geo, table, origins, extent)
    for seed, offset, base in [(7, 0, 0), (0x1234_5678_9ABC_DEF0, 3 << 33 | 5, (1 << 32) + 12345), (99, 17, (5 << 40) + 3)]:
        noisy = hash_encode_noisy(geo, table, origins, extent, num_bits, seed, offset, base)
        noise = host_noise(clean.shape[0], geo.width, num_bits, seed, offset, base).to(dev)
        assert torch.equal(noisy, clean + noise), (case, num_bits, seed, offset, base)
        assert float(noise.abs().max()) < 2.0 ** (-num_bits - 1)


# ---- 2. uint8 encode and pack, bit-exact
U8_CASES = [((200, 131), 8, F, lg, 16, [[0, 0], [200 - 37, 131 - 21], [64, 3]], (37, 21)) for F in (1, 2, 4, 8) for lg in (10, 19)]
U8_CASES += [((40, 27, 33), 6, F, lg, 4, [[0, 0, 0], [40 - 13, 27 - 10, 33 - 9], [5, 11, 2]], (13, 10, 9)) for F in (1, 2, 4, 8) for lg in (10, 19)]


@pytest.mark.parametrize("case", range(len(U8_CASES)))
def test_u8_encode_and_pack_match_save4fp_load4fp(dev, case):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import hash_encode, hash_encode_u8, hash_pack_u8, hash_stored_bytes, level_is_dense
    size, levels, F, lg, n_min, origins, extent = U8_CASES[case]
    geo = _geo(size, levels, F, lg, n_min)
    dense = [level_is_dense(r, geo.dim, lg) for r in geo.resolutions]
    assert dense[0] and (all(dense) if lg == 19 else not dense[-1])                                 # 2^10: dense and hashed (colliding) levels
    for num_bits in (8, 3):
        table = _q_table(geo, num_bits, dev, seed=100 + case)
        full = models.save4fp(table, num_bits)                                                      # [L, T, F] uint8
        E = [min((r + 1) ** geo.dim, geo.table_size) for r in geo.resolutions]
        want = torch.cat([full[l, :E[l]].reshape(-1) for l in range(geo.levels)])
        packed = hash_pack_u8(geo, table, num_bits)
        assert packed.numel() == hash_stored_bytes(geo) == F * sum(E)
        assert torch.equal(packed, want), (case, num_bits)
        got = hash_encode_u8(geo, packed, origins, extent, num_bits)
        ref = hash_encode(geo, models.load4fp(full, num_bits), origins, extent)
        assert torch.equal(got, ref), (case, num_bits)


def test_u8_encode_4k_dense_and_hashed(dev):
    """the bench geometry: 11 dense and 5 hashed levels, the whole 3840 x 2160 field in one launch"""
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import hash_encode, hash_encode_u8, hash_pack_u8
    geo = _geo((3840, 2160), 16, 2, 19)
    table = _q_table(geo, 8, dev, seed=4)
    packed = hash_pack_u8(geo, table, 8)
    assert packed.numel() == 6_717_760
    got = hash_encode_u8(geo, packed, [[0, 0]], (3840, 2160), 8)
    ref = hash_encode(geo, models.load4fp(models.save4fp(table, 8), 8), [[0, 0]], (3840, 2160))
    assert torch.equal(got, ref)


# ---- 3. save / load round trip
def test_quantize_equals_load4fp_of_save4fp_inside_the_range(dev):
    from neural_image_compression_v2_amd import models
    for b in range(1, 9):
        lo, hi = models._q_range(b)
        x = torch.cat([torch.rand(1 << 16, device=dev) * (hi - lo) + lo, torch.tensor([lo, hi, 0.0], device=dev)])
        assert torch.equal(models.quantize4fp(x, b), models.load4fp(models.save4fp(x, b), b)), b


def _image(size, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.3 * torch.sin(7 * x + 3 * y), 0.5 + 0.3 * torch.cos(5 * x * y * 4), 0.5 + 0.2 * torch.sin(13 * y - 2 * x)], dim=-1)
    return (base + 0.05 * torch.rand(*size, 3, generator=g, device=dev)).clamp(0, 1)


def test_save_load_round_trip(dev, tmp_path):
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridField, hash_encode_u8, hash_stored_bytes
    size = (120, 72)
    image = _image(size, dev, seed=2)
    field = HashGridField(size, levels=8, features=2, log2_table=12, device=dev, seed=5, num_bits=8)
    hist = field.fit(image, 40, chunk=50)
    assert field.frozen and field.table.grad is None and hist[-1] < hist[0]
    lo, hi = models._q_range(8)
    t = field.table.detach()
    assert float(t.min()) >= lo and float(t.max()) <= hi
    assert torch.equal(t, models.quantize4fp(t, 8))                                                 # the frozen table is nic_quantize'd
    mem = field.decode(tile=64)
    path = tmp_path / "field.pt"
    field.save_compressed(path)
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert d["format"] == "nicv2-hashgrid-u8/1" and d["num_bits"] == 8 and d["table"].dtype == torch.uint8
    assert d["table"].numel() == hash_stored_bytes(field.geo) == field.stored_bytes()["table"]
    loaded = HashGridField.load_compressed(path, dev)
    assert loaded.table is None
    assert torch.equal(loaded.decode(tile=64), mem)
    assert torch.equal(hash_encode_u8(loaded.geo, loaded.stored, [[0, 0]], size, 8), field.encode([[0, 0]], size))
    # a fresh process gets the same image back from the file alone
    out = tmp_path / "decoded.pt"
    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); from neural_image_compression_v2_amd.hashgrid import HashGridField; "
            "torch.save(HashGridField.load_compressed(sys.argv[2], 'cuda:0').decode(tile=64).cpu(), sys.argv[3])")
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(path), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert torch.equal(torch.load(out, weights_only=True), mem.cpu())
    with pytest.raises(RuntimeError):
        loaded.train_step([[0, 0]], size, image.reshape(-1, 3))
    with pytest.raises(RuntimeError):
        HashGridField(size, levels=4, log2_table=12, device=dev).save_compressed(tmp_path / "x.pt")


def test_save_clamps_a_copy_before_packing(dev, tmp_path):
    """a table value outside the quantiser's range is stored as the range's end, never wrapped, and the field's own table is untouched"""
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    field = HashGridField((64, 64), levels=4, features=2, log2_table=12, device=dev, seed=1, num_bits=6)
    with torch.no_grad():
        field.table[0, :3] = torch.tensor([[5.0, -5.0], [0.7, -0.6], [0.1, 0.2]], device=dev)
    before = field.table.detach().clone()
    field.save_compressed(tmp_path / "f.pt")
    assert torch.equal(field.table.detach(), before)
    stored = torch.load(tmp_path / "f.pt", weights_only=True)["table"]
    want = models.save4fp(models.quantize_clamp(before[0, :3].reshape(-1), 6), 6).cpu()
    assert torch.equal(stored[:6], want)
    assert stored[:6].tolist()[:4] == [63, 0, 63, 0]


# ---- 4. no noise sharing
def test_chunks_of_a_pass_draw_their_own_noise(dev, monkeypatch):
    from neural_image_compression_v2_amd import hashgrid
    from neural_image_compression_v2_amd.hashgrid import HashGridField, hash_encode, hash_encode_noisy
    size, chunk = (64, 40), 32
    image = _image(size, dev, seed=3)
    field = HashGridField(size, levels=6, features=2, log2_table=12, device=dev, seed=2, num_bits=8)
    calls = []

    def spy(geo, table, coord, extent, num_bits, seed, offset, sample_base=0):
        out = hash_encode_noisy(geo, table, coord, extent, num_bits, seed, offset, sample_base)
        calls.append((offset, sample_base, (out - hash_encode(geo, table, coord, extent)).clone()))
        return out

    monkeypatch.setattr(hashgrid, "hash_encode_noisy", spy)
    for _ in range(2):                                                                             # two passes of two chunks
        for k, x0 in enumerate((0, chunk)):
            field.train_step([[x0, 0]], (chunk, size[1]), image[x0:x0 + chunk].reshape(-1, 3).contiguous(), accumulate=k > 0, scale=0.5, step=k == 1)
    n = chunk * size[1]
    assert [(o, b) for o, b, _ in calls] == [(0, 0), (0, n), (1, 0), (1, n)]
    assert not torch.equal(calls[0][2], calls[1][2])                                               # same in-chunk rows, different noise
    assert float((calls[0][2] - calls[1][2]).abs().max()) > 2.0 ** -9
    assert not torch.equal(calls[0][2], calls[2][2])                                               # next step: next offset
    # the same (seed, offset, sample_base) repeats exactly
    t = field.table.detach()
    a = hash_encode_noisy(field.geo, t, [[0, 0]], (chunk, size[1]), 8, 7, 3, n)
    b = hash_encode_noisy(field.geo, t, [[0, 0]], (chunk, size[1]), 8, 7, 3, n)
    assert torch.equal(a, b)


# ---- 5. num_bits=None is unchanged
def _run20(dev, image, crops, extent, **kw):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    field = HashGridField(image.shape[:2], levels=8, features=2, log2_table=12, device=dev, seed=3, **kw)
    enc0 = field.encode(crops[0], extent).detach().clone()
    losses = []
    for k in range(20):
        i = sample_coords(crops[k], extent, dev)
        losses.append(field.train_step(crops[k], extent, image[i[:, 0], i[:, 1]]))
    torch.cuda.synchronize()
    return enc0, [float(v) for v in losses], field.table.detach().clone()


def test_num_bits_none_trains_as_before(dev):
    size, extent = (256, 192), (64, 48)
    image = _image(size, dev)
    g = torch.Generator().manual_seed(9)
    crops = [torch.stack([torch.randint(0, size[0] - extent[0] + 1, (4,), generator=g), torch.randint(0, size[1] - extent[1] + 1, (4,), generator=g)], 1)
             for _ in range(20)]
    e_a, l_a, t_a = _run20(dev, image, crops, extent)
    e_r, l_r, t_r = _run20(dev, image, crops, extent)                                               # the run-to-run spread of the atomics
    e_b, l_b, t_b = _run20(dev, image, crops, extent, num_bits=None)
    assert torch.equal(e_a, e_b) and l_a[0] == l_b[0]
    spread_t = float((t_a - t_r).abs().max())
    tol_t = max(4 * spread_t, 1e-6 * float(t_a.abs().max()))
    assert float((t_a - t_b).abs().max()) <= tol_t, (spread_t, float((t_a - t_b).abs().max()))
    for k in range(20):
        tol = max(4 * abs(l_a[k] - l_r[k]), 1e-6 * abs(l_a[k]))
        assert abs(l_a[k] - l_b[k]) <= tol, (k, l_a[k], l_b[k], l_r[k])


# ---- 6. / 7. fit quality
def _structured_image(size, dev):
    """smooth colour ramps plus finer texture and soft edges, no random term: a picture whose detail lives in the table (the random term of
    ``_image`` puts every fit at its noise floor, near 37 dB, where quantisers hardly differ)"""
    x = torch.linspace(0, 1, size[0], device=dev)[:, None]
    y = torch.linspace(0, 1, size[1], device=dev)[None, :]
    base = torch.stack([0.5 + 0.25 * torch.sin(7 * x + 3 * y) + 0.15 * torch.sin(41 * x) * torch.cos(37 * y),
                        0.5 + 0.25 * torch.cos(20 * x * y) + 0.15 * torch.sin(60 * (x - y) ** 2),
                        0.5 + 0.2 * torch.sin(13 * y - 2 * x) + 0.1 * torch.sign(torch.sin(9 * x + 11 * y))], dim=-1)
    return base.clamp(0, 1)


def test_fit_quality_2d_qat(dev, tmp_path):
    """256^2 (``_structured_image``), 8 levels x 2 features x 2^12, 300 passes: b = 8 stored within 1 dB of the unquantised fit; b = 4 stored
    beats post-training quantisation of that unquantised fit (clamp + nic_quantize, no noise, no freeze)"""
    from neural_image_compression_v2_amd import models
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    size, epochs = (256, 256), 300
    image = _structured_image(size, dev)
    kw = dict(levels=8, features=2, log2_table=12, device=dev, seed=1)
    fp = HashGridField(size, **kw)
    fp.set_schedule(epochs)
    fp.fit(image, epochs)
    p_fp = psnr(fp.decode(), image)
    res = {}
    for b in (8, 4):
        q = HashGridField(size, num_bits=b, **kw)
        q.set_schedule(epochs)
        q.fit(image, epochs)
        q.save_compressed(tmp_path / f"q{b}.pt")
        res[b] = psnr(HashGridField.load_compressed(tmp_path / f"q{b}.pt", dev).decode(), image)
    with torch.no_grad():
        fp.table.copy_(models.quantize4fp(models.quantize_clamp(fp.table, 4), 4))
    p_ptq4 = psnr(fp.decode(), image)
    print(f"2D PSNR: fp32 {p_fp:.2f} dB, QAT b=8 stored {res[8]:.2f}, QAT b=4 stored {res[4]:.2f}, PTQ b=4 {p_ptq4:.2f}")
    assert res[8] >= p_fp - 1.0, (p_fp, res[8])
    assert res[4] > p_ptq4, (res[4], p_ptq4)


def test_fit_quality_3d_qat(dev, tmp_path):
    """a 64^3 volume, b = 8: the loss falls below 0.1 x its start and the stored decode equals the frozen field's"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    n = 64
    ax = torch.linspace(0, 1, n, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.stack([0.5 + 0.3 * torch.sin(6 * x + 2 * z), 0.5 + 0.3 * torch.cos(4 * y - 3 * z), 0.5 + 0.25 * torch.sin(5 * (x + y + z))], dim=-1)
    field = HashGridField((n, n, n), levels=8, features=2, log2_table=16, base_resolution=4, device=dev, seed=2, num_bits=8)
    hist = field.fit(vol, 150)
    assert field.frozen and hist[-1] < 0.1 * hist[0], (hist[0], hist[-1])
    mem = field.decode(tile=40)
    field.save_compressed(tmp_path / "vol.pt")
    stored = HashGridField.load_compressed(tmp_path / "vol.pt", dev).decode(tile=40)
    assert torch.equal(stored, mem)
    mse = float(((stored - vol) ** 2).mean())
    print(f"3D QAT b=8: stored PSNR {psnr(stored, vol):.2f} dB, table {field.stored_bytes()}")
    assert mse < 0.1 * hist[0]
