"""GPU tests of the work-unit pipeline of the 8-wave x 16-sample split-bf16 training kernel (csrc/fused_train16.hpp): the header of a wave's
next work unit (tile -> crop, origin, cell offsets, the 24 gathers per lane, the rounds of the piece) is issued after the last round of the
current unit, ahead of its once-per-unit product and its flush.  What can go wrong is a unit that runs with another unit's header - its grid
values, its cell, its crop, its rounds - or a flush that uses the next unit's offsets, so every case runs the same launch on three kernels
and holds the 16-sample kernel to

  * the fp32 kernel (split_bf16=False), and
  * the 4-wave x 32-sample split kernel (split_tile32=True), which has no such pipeline,

at the tolerances of tests/test_gpu_t16_dx_once.py (its `_hold`: y 1e-6 / 2e-6, loss 2e-6, every gradient 2e-5 of the tensor's largest entry
with the per-row rule), and the passes-against-listed-crops relation at the 2e-6 of test_gpu_parity.py.

Unit schedules (fused_capi.hip::balance_units; mip 0 = 16 rounds per macro-tile of 64 x 4 samples; max_workgroups 8 = 64 waves, one
workgroup per XCD, a wave's units 8 apart; 16 = 128 waves, workgroups 8..15 shifted by 4 rounds):
  * 16x3 at mip 2 (one round per macro-tile, whole units only): at most 6 units, all in workgroup 0 - fewer units than waves of ONE
    workgroup: waves without a unit (tile_ok false), nobody has a successor;
  * 256x64 / 256x128 / 256x192 on 64 waves: exactly one (first = last), two and three whole units per wave;
  * 256x128 / 256x256 on 128 waves: one / two units per wave, in workgroups 8..15 cut in two by the stagger shift (12 + 4 rounds: the pieces
    kk == 0 and kk == n_my are the SAME tile, so a header is issued for a tile the wave has already flushed once);
  * 244x80 at (3, 5) on 64 waves: 62 x 21 cells, three columns of regular tiles and a column of edge tiles - 64 whole units, then the rest in groups of rounds
    (both segments in one launch, leader and followers of a group with different next units, shifted pieces in the groups);
  * the reference's default step: 8 crops of 256 x 256 at unaligned origins in a 512 x 512 image, whole chip - 2 120 macro-tiles = 2 048
    whole units and 72 in 8 groups of 2 rounds;
  * edge tiles and far edges: 150x70 ending at the far corner of the grid, 37x21 at the far corner, a single sample at the far corner;
  * 48 overlapping crops of 64x16 at different origins on 64 waves: three units per wave, consecutive units of a wave two crops apart.
Checked once by hand that the file is not vacuous: a build whose header hands every later unit of a segment the previous unit's gathered values
fails 20 of the 27 cases (all with two or more units per wave in a segment); the 7 that pass have one unit per wave and segment.
The training entry points accept fp32, bf16 and fp16 grid storage (grid kinds 0, 1, 2); the uint8 kind (3) is reachable for decoding
kernels only, so no training launch can be made with it.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import _pyramid, assert_rel  # noqa: E402  (shared helpers)
from tests.test_gpu_t16_dx_once import _geo, _hold, _inputs, _mse_case, _three  # noqa: E402

_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


SHAPES = [
    # extent, origins, passes, mip, max_workgroups
    ((16, 3), [(3, 5)], 1, 2, 0),                       # fewer units than waves of one workgroup
    ((256, 64), [(0, 0)], 1, 0, 8),                     # exactly one unit per wave
    ((256, 128), [(0, 0)], 1, 0, 8),                    # two
    ((256, 192), [(0, 0)], 1, 0, 8),                    # three
    ((256, 128), [(0, 0)], 1, 0, 16),                   # one unit per wave, cut in two by the shift in workgroups 8..15
    ((256, 256), [(0, 0)], 1, 0, 16),                   # two units per wave, three pieces where shifted
    ((244, 80), [(3, 5)], 1, 0, 8),                     # whole units, then round groups; edge tiles
    ((150, 70), [(106, 186)], 1, 0, 0),                 # edge tiles, the crop ends at the far corner of the grid
    ((37, 21), [(219, 235)], 1, 0, 0),
    ((1, 1), [(255, 255)], 1, 0, 0),                    # a single sample at the far corner
    ((64, 16), [((7 * i) % 190, (11 * i) % 236) for i in range(48)], 1, 0, 8),      # consecutive units of a wave in different, overlapping crops
]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"{'x'.join(map(str, c[0]))}-{len(c[1])}crops-p{c[2]}-mip{c[3]}-wg{c[4]}")
def test_unit_pipeline_matches_fp32_and_32_sample_kernels(dev, case):
    """The unit schedules of the module docstring."""
    extent, origins, passes, mip, mw = case
    outs, n, _ = _mse_case(dev, extent, origins, passes, mip, max_workgroups=mw)
    _hold(outs, n, "shape")


def test_unit_pipeline_default_step_shape(dev):
    """8 crops of 256 x 256 at unaligned origins in a 512 x 512 image (a 128-cell pyramid), whole chip: 2 120 macro-tiles."""
    from neural_image_compression_v2_amd import fused
    if "p128" not in _CACHE:
        fp, _ = _pyramid(2, 128, 12, seed=33, no_mip=True)
        _CACHE["p128"] = (fp[0], fp[1])
    g0, g1 = (t.to(dev) for t in _CACHE["p128"])
    _, _, mlp = _inputs(0)
    params = [q.to(dev) for q in mlp.tensors()]
    extent, origins = (256, 256), [(3, 5), (17, 201), (101, 3), (255, 255), (130, 77), (41, 190), (222, 9), (65, 129)]
    n = len(origins) * extent[0] * extent[1]
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    geo = _geo(extent, len(origins))
    outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, g0, g1, origins, params, target, want_y=True))
    _hold(outs, n, "default step")


def test_unit_pipeline_passes_equal_listed_crops(dev):
    """`passes = 3` over 16 overlapping crops == the same crops listed three times (test_gpu_parity.py::test_repeated_passes_equal_repeated_crops:
    y bit for bit, everything else 2e-6 - the order of fp32 additions).  The two launches deal the same rounds out to different units: 48-round
    units against 16-round units of three times as many crops, so a wave's successive headers differ between them."""
    from neural_image_compression_v2_amd import fused
    P = 3
    g0, g1, mlp = _inputs(0)
    g0, g1 = g0.to(dev), g1.to(dev)
    params = [q.to(dev) for q in mlp.tensors()]
    extent, origins = (64, 16), [((13 * i) % 190, (29 * i) % 236) for i in range(16)]
    n_crop = extent[0] * extent[1]
    target = torch.rand(len(origins) * P * n_crop, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    a = fused.fused_forward_backward(_geo(extent, len(origins), P, max_workgroups=8)(split_bf16=True), g0, g1, origins, params, target, want_y=True)
    listed = [o for o in origins for _ in range(P)]
    b = fused.fused_forward_backward(_geo(extent, len(listed), 1, max_workgroups=8)(split_bf16=True), g0, g1, listed, params, target, want_y=True)
    assert torch.equal(a.y, b.y)
    assert_rel(a.loss, b.loss, 1e-6, "loss")
    assert_rel(a.grad_g0, b.grad_g0, 2e-6, "G0 grad")
    assert_rel(a.grad_g1, b.grad_g1, 2e-6, "G1 grad")
    for nme, p_, q_ in zip(["W1", "b1", "W2", "b2", "W3", "b3"], a.grad_mlp, b.grad_mlp):
        assert_rel(p_, q_, 2e-6, nme)


ENTRY_EXTENT, ENTRY_ORIGINS = (128, 128), [(3, 5), (100, 60)]      # 138 macro-tiles on 64 waves: two whole units per wave, then 10 macro-tiles in groups


@pytest.mark.parametrize("pe", ["tri", "sin"])
@pytest.mark.parametrize("entry", ["mse", "dy", "image-u8", "image-rgbx"])
def test_unit_pipeline_every_entry_point(dev, entry, pe):
    """MODE_TRAIN_MSE, MODE_TRAIN_DY (through autograd), MODE_TRAIN_IMG (planar uint8 image) and MODE_TRAIN_RGBX (interleaved image), both PE
    layouts: the eight instantiations of the kernel, each on a launch with both segments."""
    from neural_image_compression_v2_amd import fused
    from neural_image_compression_v2_amd.sampler import rgbx_interleave
    extent, origins = ENTRY_EXTENT, ENTRY_ORIGINS
    n = len(origins) * extent[0] * extent[1]
    g0, g1, mlp = _inputs(0)
    g0d, g1d = g0.to(dev), g1.to(dev)
    params = [q.to(dev) for q in mlp.tensors()]
    geo = _geo(extent, len(origins), use_tri_pe=pe == "tri", max_workgroups=8)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(5))
    if entry == "mse":
        outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, g0d, g1d, origins, params, target.to(dev), want_y=True))
        _hold(outs, n, f"{entry}-{pe}")
    elif entry.startswith("image"):
        isz = [max(o[a] for o in origins) + extent[a] for a in range(2)]
        img = torch.randint(0, 256, (3, *isz), generator=torch.Generator().manual_seed(21), dtype=torch.uint8).to(dev)
        timg = fused.TargetImage(img, 255.0) if entry == "image-u8" else fused.TargetImage(rgbx_interleave(img), 255.0, rgbx=True)
        outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, g0d, g1d, origins, params, timg, want_y=True))
        _hold(outs, n, f"{entry}-{pe}")
    else:
        dy = ((target - 0.5) / n).to(dev)

        class Out:
            pass

        def run(ge, tag):
            gg = [g0d.clone().requires_grad_(True), g1d.clone().requires_grad_(True)]
            pd = [q.clone().requires_grad_(True) for q in params]
            fused.fused_grid_mlp(ge, gg[0], gg[1], origins, pd).backward(dy)
            o = Out()
            o.grad_g0, o.grad_g1, o.grad_mlp = gg[0].grad, gg[1].grad, [q.grad for q in pd]
            return o
        _hold(_three(geo, run), n, f"{entry}-{pe}", with_y=False, with_loss=False)


@pytest.mark.parametrize("noise", ["kernel", "tensor"])
@pytest.mark.parametrize("storage", ["f32", "bf16", "fp16"])
def test_unit_pipeline_grid_storage_and_noise(dev, storage, noise):
    """fp32, bf16 and fp16 grid storage (one switch per unit in front of the 24 gathers), kernel noise and an explicit noise tensor, two units
    per wave.  The references have no 16-bit gather and run on the widened grids (the widening is exact)."""
    from neural_image_compression_v2_amd import _lib, fused
    extent, origins = (256, 128), [(0, 0)]
    n = extent[0] * extent[1]
    g0, g1, mlp = _inputs(0)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[storage]
    s0, s1 = g0.to(dev).to(dt), g1.to(dev).to(dt)
    w0, w1 = s0.float(), s1.float()
    params = [q.to(dev) for q in mlp.tensors()]
    gen = torch.Generator().manual_seed(5)
    target = torch.rand(n, 3, generator=gen).to(dev)
    kw, nd = {}, None
    if noise == "tensor":
        nd = ((torch.rand(n, 73, generator=gen) - 0.5) / 256).to(dev)
        kw = dict(noise_mode=_lib.NIC_NOISE_TENSOR)
    geo = _geo(extent, len(origins), max_workgroups=8, **kw)
    outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, *((s0, s1) if tag == "t16" else (w0, w1)), origins, params, target, nd, want_y=True))
    assert outs["t16"].grad_g0.dtype == torch.float32 and outs["t16"].grad_g0.shape == s0.shape
    _hold(outs, n, f"{storage} grids, {noise} noise")
