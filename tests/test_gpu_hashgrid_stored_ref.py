"""GPU tests of every route that turns a stored hash-grid file into colours, against a float64 decode of the file's BYTES
(oracle/hashgrid_ref.py, written from the contract text of include/nicv2_hip.h and importing nothing of the package).

The other hash-grid files pin these routes to each other (batch -> singles -> layer-wise -> fp32 gather of load4fp(save4fp) -> ...); here each
route is held to the reference directly, so a misunderstanding the routes share - a bias, an offset, a bit order, the point convention -
cannot hide, and the committed fixtures of tests/golden/hashgrid/ (written by oracle/make_hashgrid_golden.py, held still by
tests/test_hashgrid_stored_ref_cpu.py) keep the three formats readable across commits.

Bounds: the project's own, none measured on the code under test.  y is a sigmoid output, so the error is the maximum absolute difference.
  fp32 routes (layer-wise and fused)   5e-6: the bound of tests/test_gpu_parity.py::test_decoder_forward_backward and the TOL_Y of every hash-grid file
  precision="split"                    1e-5: 5e-6 to the fp32 route (TOL_SPLIT of tests/test_gpu_hashgrid_p16.py) + 5e-6 from there to the reference
  precision="bf16"                     1e-3 + 5e-6 (TOL_BF16 + the above) on the files with the default decoder initialisation, for which TOL_BF16
                                       is stated; elsewhere the error is printed and must be finite (that arithmetic is held to its emulating
                                       oracle in tests/test_gpu_hashgrid_p16.py)
Every test prints the worst error per route; DESIGN 4.7.16 records them."""
import os

import numpy as np
import pytest
import torch

from oracle import hashgrid_ref as R
from oracle import make_hashgrid_golden as G

pytestmark = pytest.mark.gpu

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hashgrid")
TOL_FP32 = 5e-6
TOL_SPLIT = TOL_FP32 + 5e-6
TOL_BF16 = 1e-3 + TOL_FP32
CASES = {c["name"]: c for c in G.CASES}
NAMES = list(CASES)
GENERAL = "hg2d_u8_b8_h32n4"                                     # hidden 32, 4 Linear layers: outside the fused set
MIXED = [n for n in NAMES if CASES[n]["spec"]["fmt"] == "bits2"]
UNIFORM = [n for n in NAMES if n not in MIXED and n != GENERAL]  # what the precision= routes and the batches take


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_cache = {}


def fixture(name):
    """(path of NAME.pt, its dict, its StoredFile, the arrays of NAME.npz), read once"""
    if name not in _cache:
        path = os.path.join(FIXTURES, name + ".pt")
        d = torch.load(path, map_location="cpu", weights_only=True)
        with np.load(os.path.join(FIXTURES, name + ".npz")) as z:
            _cache[name] = (path, d, R.parse(d), {k: z[k] for k in z.files})
    return _cache[name]


def hold(got, ref, bound, what):
    """max |got - ref| <= bound (None: finite), printed first"""
    g = got.detach().double().cpu().numpy()
    assert g.shape == ref.shape, f"{what}: shape {g.shape}, the reference's {ref.shape}"
    e = float(np.abs(g - ref).max())
    print(f"{what}: max abs error {e:.3e}" + ("" if bound is None else f" (bound {bound:.1e})"))
    assert np.isfinite(g).all() and np.isfinite(e), f"{what}: not finite"
    if bound is not None:
        assert e <= bound, f"{what}: {e:.3e} > {bound:.1e}"
    return e


def bound_of(precision, default_init):
    return {None: TOL_FP32, "split": TOL_SPLIT, "bf16": TOL_BF16 if default_init else None}[precision]


def same_points(field, f, size):
    """the fp32 points ``resample`` queries are the reference's, bit for bit: a point within an ulp of a rint tie may not land on the
    neighbouring 1/256 step on one side only"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    mine = HashGridField._resample_points(field, size, (0,) * f.dim, size).cpu().numpy()
    ref = R.resample_points(f, size)
    assert mine.dtype == ref.dtype == np.float32 and mine.shape == ref.shape
    assert mine.tobytes() == ref.tobytes(), f"_resample_points{tuple(size)}: {int((mine != ref).sum())} coordinates differ from the reference's"


# ------------------------------------------------------------------------------------------------------------------ committed fixtures

@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("name", NAMES)
def test_fixture_against_the_reference(dev, name, fused):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    path, d, f, ref = fixture(name)
    field = HashGridField.load_compressed(path, device=dev, fused=fused)
    # a decoder outside the fused set falls back to the layer-wise route when fused=True is asked for (``_set_route``): today's behaviour
    assert field.route == ("fused" if fused and name != GENERAL else "layerwise")
    assert field.table is None and (field.level_bits is not None) == (name in MIXED)
    size = tuple(int(v) for v in ref["resample_size"])
    tag = f"{name} {field.route}"
    pts = torch.from_numpy(ref["points"]).to(dev)
    hold(field.decode(), ref["decode"], TOL_FP32, f"{tag} decode()")
    hold(field.decode(tile=16), ref["decode"], TOL_FP32, f"{tag} decode(tile=16)")
    hold(field.query(pts), ref["query"], TOL_FP32, f"{tag} query({pts.shape[0]} points)")
    same_points(field, f, size)
    hold(field.resample(size), ref["resample"], TOL_FP32, f"{tag} resample{size}")
    hold(field.resample(size, tile=7), ref["resample"], TOL_FP32, f"{tag} resample{size} tile=7")


@pytest.mark.parametrize("fused", [False, True], ids=["layerwise", "fused"])
@pytest.mark.parametrize("name", NAMES)
def test_lattice_and_point_kernels_at_sample_centres(dev, name, fused):
    """``decode()`` (the lattice kernels) and ``query`` at the sample centres (the point kernels) against the reference, whose two routes are
    equal exactly there.  Whether the two GPU results are equal bit for bit is printed, not asserted: the fused point kernel carries its own
    decoder body"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    path, d, f, ref = fixture(name)
    field = HashGridField.load_compressed(path, device=dev, fused=fused)
    centres = torch.from_numpy(R.sample_centres(f)).to(dev)
    y_l = field.decode()
    y_p = field.query(centres).reshape(*f.field_size, 3)
    hold(y_l, ref["decode"], TOL_FP32, f"{name} {field.route} decode()")
    hold(y_p, ref["decode"], TOL_FP32, f"{name} {field.route} query(sample centres)")
    diff = float((y_l.double() - y_p.double()).abs().max())
    print(f"{name} {field.route}: query(sample centres) and decode() bits {'equal' if torch.equal(y_l, y_p) else 'differ'} (max |diff| {diff:.3e})")


# ------------------------------------------------------------------------------------------------------------------ precision= routes

@pytest.mark.parametrize("precision", ["split", "bf16"])
@pytest.mark.parametrize("name", UNIFORM)
def test_fixture_on_the_16_bit_matrix_pipe(dev, name, precision):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    path, d, f, ref = fixture(name)
    field = HashGridField.load_compressed(path, device=dev, fused=True)
    bound = bound_of(precision, CASES[name]["spec"]["scale"] == 1.0)
    size = tuple(int(v) for v in ref["resample_size"])
    pts = torch.from_numpy(ref["points"]).to(dev)
    hold(field.decode(precision=precision), ref["decode"], bound, f"{name} {precision} decode()")
    hold(field.decode(tile=16, precision=precision), ref["decode"], bound, f"{name} {precision} decode(tile=16)")
    hold(field.query(pts, precision=precision), ref["query"], bound, f"{name} {precision} query")
    hold(field.resample(size, precision=precision), ref["resample"], bound, f"{name} {precision} resample{size}")
    hold(field.resample(size, tile=7, precision=precision), ref["resample"], bound, f"{name} {precision} resample{size} tile=7")


@pytest.mark.parametrize("precision", ["split", "bf16"])
def test_what_the_16_bit_routes_refuse(dev, precision):
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    for name, error in [(n, NotImplementedError) for n in MIXED] + [(GENERAL, ValueError)]:
        path, d, f, ref = fixture(name)
        field = HashGridField.load_compressed(path, device=dev, fused=True)
        pts = torch.from_numpy(ref["points"]).to(dev)
        for call in (lambda: field.decode(precision=precision), lambda: field.query(pts, precision=precision),
                     lambda: field.resample(tuple(int(v) for v in ref["resample_size"]), precision=precision)):
            with pytest.raises(error, match="bit depth per level" if error is NotImplementedError else "fused set"):
                call()


# ------------------------------------------------------------------------------------------------------------------ batches

_batches = {}


def batch_case(name, tmp_path_factory):
    """B = 3 files of the fixture's spec (seeds 1, 2, 3, the fixture's own among them) and the reference's arrays per field, made once"""
    if name not in _batches:
        case = CASES[name]
        seeds = (1, 2, 3) if case["seed"] in (1, 2, 3) else (1, 2, case["seed"])
        root = tmp_path_factory.mktemp(name)
        paths, files, points = [], [], []
        for s in seeds:
            d = R.make_file(case["spec"], s)
            paths.append(str(root / f"seed{s}.pt"))
            R.save(d, paths[-1])
            files.append(R.parse(d))
            points.append(G.query_points(files[-1].field_size, files[-1].resolutions, seed=s))      # every field its own points
        path, d0, f0, ref0 = fixture(name)
        k = seeds.index(case["seed"])
        assert np.array_equal(files[k].table, f0.table)                      # that file IS the committed fixture
        size = case["resample"]
        ref = {"decode": np.stack([ref0["decode"] if i == k else R.decode(f) for i, f in enumerate(files)]),
               "query": np.stack([R.query(f, p) for f, p in zip(files, points)]),
               "resample": np.stack([ref0["resample"] if i == k else R.resample(f, size) for i, f in enumerate(files)])}
        assert len({r.tobytes() for r in ref["decode"]}) == 3                  # the fields differ: a swapped or shared one fails
        _batches[name] = (paths, files, np.stack(points), ref)
    return _batches[name]


@pytest.mark.parametrize("precision", [None, "split", "bf16"], ids=["fp32", "split", "bf16"])
@pytest.mark.parametrize("name", UNIFORM)
def test_batch_of_three_files_against_the_reference(dev, tmp_path_factory, name, precision):
    from neural_image_compression_v2_amd.hashgrid import HashGridFieldBatch
    paths, files, points, ref = batch_case(name, tmp_path_factory)
    batch = HashGridFieldBatch.load_compressed(paths, device=dev)
    assert batch.n_fields == 3 and batch.decode_only
    bound = bound_of(precision, CASES[name]["spec"]["scale"] == 1.0)
    size = tuple(CASES[name]["resample"])
    tag = f"{name} batch {precision or 'fp32'}"
    same_points(batch, files[0], size)
    for what, y in (("decode", batch.decode(precision=precision)), ("decode(tile=16)", batch.decode(tile=16, precision=precision)),
                    ("query", batch.query(torch.from_numpy(points).to(dev), precision=precision)),
                    ("resample", batch.resample(size, precision=precision)), ("resample tile=7", batch.resample(size, tile=7, precision=precision))):
        key = what.split()[0].split("(")[0]
        worst = max(hold(y[b], ref[key][b], bound, f"{tag} {what} field {b}") for b in range(3))
        print(f"{tag} {what}: worst of the three fields {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------ on-the-fly matrix

def _tight(F, b):
    """no entry of F b bits straddles a dword (hash_bits_tight, csrc/hash_common.hpp)"""
    return 32 % (F * b) == 0 or F * b == 64


def _depth(F, tight):
    """the ``_depth`` rule of tests/test_gpu_hashgrid_batch_stored.py: a packed depth at which the gather takes the one-dword or the straddling window"""
    return next(b for b in (4, 5, 3, 6, 7) if _tight(F, b) == tight)


MATRIX = [(dim, F, width // F, src) for dim in (2, 3) for F in (1, 2, 4, 8) for width in (8, 24, 32, 40, 64) if width // F <= 32
          for src in ("u8", "tight", "straddle", "mixed")]


@pytest.mark.parametrize("dim,F,L,src", MATRIX, ids=[f"{d}d-F{F}-L{L}-{s}" for d, F, L, s in MATRIX])
def test_matrix_against_the_reference_only(dev, tmp_path, dim, F, L, src):
    """every (dim, F, row width, source) the fused decode dispatches on, decode and query on both routes; nothing is committed for these"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    geo = dict(field_size=(44, 37), log2_table=10, base=16) if dim == 2 else dict(field_size=(12, 10, 9), log2_table=10, base=4)
    fmt, bits = {"u8": ("u8", 8), "tight": ("bits1", _depth(F, True)), "straddle": ("bits1", _depth(F, False)),
                 "mixed": ("bits2", tuple(1 + (3 * l + 2) % 8 for l in range(L)))}[src]
    if src in ("tight", "straddle"):
        assert _tight(F, bits) == (src == "tight")
    d = R.make_file(dict(geo, levels=L, features=F, fmt=fmt, bits=bits, hidden=64, n_linear=3, scale=1.5), seed=1 + (7 * L + F + dim) % 5)
    f = R.parse(d)
    path = str(tmp_path / "file.pt")
    R.save(d, path)
    pts = G.query_points(f.field_size, f.resolutions, seed=L)
    ref_decode, ref_query = R.decode(f), R.query(f, pts)
    for fused in (False, True):
        field = HashGridField.load_compressed(path, device=dev, fused=fused)
        assert field.route == ("fused" if fused else "layerwise")
        hold(field.decode(), ref_decode, TOL_FP32, f"matrix {dim}d F{F} L{L} {src} {field.route} decode()")
        hold(field.query(torch.from_numpy(pts).to(dev)), ref_query, TOL_FP32, f"matrix {dim}d F{F} L{L} {src} {field.route} query")


# ------------------------------------------------------------------------------------------------------------------ the writer

def _same_file(saved: dict, want: dict, what: str) -> None:
    assert set(saved) == set(want), f"{what}: keys {sorted(saved)} against {sorted(want)}"
    for k in want:
        if k == "table":
            assert saved[k].dtype == torch.uint8 and saved[k].shape == want[k].shape and torch.equal(saved[k], want[k]), \
                f"{what}: the table differs in {int((saved[k] != want[k]).sum()) if saved[k].shape == want[k].shape else 'length'} bytes"
        elif k == "decoder":
            assert list(saved[k]) == list(want[k])
            for n in want[k]:
                assert saved[k][n].dtype == torch.float32 and saved[k][n].numpy().tobytes() == want[k][n].numpy().tobytes(), f"{what}: {n}"
        else:
            assert saved[k] == want[k], f"{what}: {k} {saved[k]!r} against {want[k]!r}"


@pytest.mark.parametrize("name", NAMES)
def test_the_writer_writes_the_fixture(dev, tmp_path, name):
    """a trainable field holding the fixture's dequantised values and decoder saves the fixture's dict, byte for byte; the entries a dense
    level cannot address hold 0.25, so a writer that stored them would change the length and the bytes"""
    from neural_image_compression_v2_amd.hashgrid import HashGridField
    path, d, f, ref = fixture(name)
    spec = CASES[name]["spec"]
    field = HashGridField(f.field_size, levels=f.levels, features=f.features, log2_table=f.log2_table, base_resolution=spec["base"],
                          hidden=f.hidden, n_linear=f.n_linear, device=dev, seed=0,
                          num_bits=list(f.level_bits) if name in MIXED else f.num_bits)
    assert tuple(field.geo.resolutions) == f.resolutions
    table = torch.full(field.geo.table_shape(), 0.25, dtype=torch.float32)
    for l, x in enumerate(R.table_values(f)):
        table[l, :x.shape[0]] = torch.from_numpy(x).to(torch.float32)
    with torch.no_grad():
        field.table.copy_(table.to(dev))
    field.decoder.load_state_dict(d["decoder"])
    wants = [(spec["fmt"] != "u8", d)]
    if name not in MIXED:                                                      # the same values in the other uniform format: make_file's own packing of it
        other = "u8" if spec["fmt"] == "bits1" else "bits1"
        wants.append((other != "u8", R.make_file(dict(spec, fmt=other), CASES[name]["seed"])))
    for packed, want in wants:
        out = str(tmp_path / f"saved_{int(packed)}.pt")
        field.save_compressed(out, packed=packed)
        _same_file(torch.load(out, map_location="cpu", weights_only=True), want, f"{name} save_compressed(packed={packed})")
