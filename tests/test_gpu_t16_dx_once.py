"""GPU tests of the G0 input gradients of the 8-wave x 16-sample split-bf16 training kernel (csrc/fused_train16.hpp), which are formed ONCE per
work unit: the round adds dZ1 into a running sum and keeps only the G1 row tile of dX = W1^T dZ1; after the unit's last round the G0 tiles are
W1^T split(sum of dZ1).  Every case runs the same launch on three kernels and holds the 16-sample kernel to

  * the fp32 kernel (split_bf16=False), and
  * the 4-wave x 32-sample split kernel (split_tile32=True), which keeps the per-round product,

at the tolerances of test_gpu_parity.py::test_train16_kernel_matches_the_32_sample_kernels: y 1e-6 (32-sample) / 2e-6 (fp32), loss 2e-6, every
gradient 2e-5 of the tensor's largest entry with that test's per-row rule (row_factor 10 from 1 000 samples, 100 from 64, none below).

What the host's unit schedule (fused_capi.hip::balance_units) makes of the shapes on a 256-CU device (2 048 waves), mip 0 = 16 rounds per
macro-tile and pass:
  * 64x4, passes 3 / 1: one macro-tile, seg_split 0, rg_log2 4 - sixteen units of 3 rounds / 1 round in two workgroups, summed through LDS;
  * 256x128, passes 3, max_workgroups 16: 128 macro-tiles on 128 waves - seg_split 128, whole units of 48 rounds; workgroups 8..15 run them
    as two pieces (shift 12: 36 + 12 rounds), workgroups 0..7 in one piece.  This is the longest running sum of the file;
  * 256x256 x 2 crops: 512 macro-tiles, seg_split 0, rg_log2 2 - 2 048 units of 4 rounds on 256 workgroups, shift 0..3 (units cut in two),
    groups of four summed through LDS; the same with max_workgroups 16: seg_split 512, whole 16-round units, shift 0 / 4;
  * 256x132: 132 macro-tiles - the smallest count (> 128) at which a whole-chip launch keeps more than one round per unit: seg_split 0,
    rg_log2 3, 1 056 units of 2 rounds on 136 workgroups, shift 0 / 1.  64x36 with max_workgroups 16: 9 macro-tiles on 128 waves, rg_log2 3,
    72 units of 2 rounds on 16 workgroups, shift 1 in workgroups 8..15 - the smallest launch with a unit cut in two.  Any launch of at most
    128 macro-tiles on the whole chip has rg_log2 4 (single rounds, no shift): 1x1 is the smallest with rg_log2 > 0;
  * 150x70 at (3, 5): 39 x 18 cells - two columns of regular tiles and a column of edge tiles, seg_split 0, rg_log2 4, single-round units;
  * mip 1 (40x24): 4 rounds per macro-tile; mip 2 and 3 (10x9): one round per macro-tile and unit - the sum is a single term.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nic_oracle as O  # noqa: E402  (checker only)
from tests.test_gpu_parity import _pyramid, assert_rel, rel_rows, relmax  # noqa: E402

NAMES = ["G0", "G1", "W1", "b1", "W2", "b2", "W3", "b3"]
NOISE = dict(noise_seed=11, noise_offset=3, sample_base=12345)
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _inputs(mip):
    """grids of the level pair and the decoder, built once per pyramid kind and shared (never written)"""
    key = mip == 0
    if key not in _CACHE:
        fp, _ = _pyramid(2, 64, 12, seed=31, no_mip=key)
        _CACHE[key] = (fp[0], fp[1], O.init_mlp(73, 64, generator=torch.Generator().manual_seed(5)))
    return _CACHE[key]


def _geo(extent, ncrops, passes=1, mip=0, **kw):
    from neural_image_compression_v2_amd import _lib, fused
    base = dict(dim=2, method=1, step_number=O.step_number_of(mip, 0), mip_level=mip, extent=extent, num_crops=ncrops, passes=passes,
                noise_mode=_lib.NIC_NOISE_KERNEL, **NOISE)
    base.update(kw)
    return lambda **flags: fused.PathGeometry(**base, **flags)


KERNELS = (("f32", dict(split_bf16=False)), ("t32", dict(split_bf16=True, split_tile32=True)), ("t16", dict(split_bf16=True)))


def _three(geo, run):
    """`run(geometry, tag)` on the fp32, the 32-sample split and the 16-sample split kernel"""
    return {tag: run(geo(**flags), tag) for tag, flags in KERNELS}


def _grads(o):
    return [o.grad_g0, o.grad_g1] + list(o.grad_mlp)


def _hold(outs, n, what, with_y=True, with_loss=True):
    a = outs["t16"]
    rf = 10.0 if n >= 1000 else (100.0 if n >= 64 else 1e9)
    for tag, ty in (("t32", 1e-6), ("f32", 2e-6)):
        ref = outs[tag]
        if with_y:
            print(f"{what} vs {tag}: y {relmax(a.y, ref.y):.2e}", end="")
        if with_loss:
            print(f" loss {relmax(a.loss, ref.loss):.2e}", end="")
        print("".join(f" {nme} {relmax(p_, q_):.2e}/{rel_rows(p_, q_):.2e}" for nme, p_, q_ in zip(NAMES, _grads(a), _grads(ref))), flush=True)
    for tag, ty in (("t32", 1e-6), ("f32", 2e-6)):
        ref = outs[tag]
        if with_y:
            assert_rel(a.y, ref.y, ty, f"{what}: y vs {tag}")
        if with_loss:
            assert_rel(a.loss, ref.loss, 2e-6, f"{what}: loss vs {tag}")
        for nme, p_, q_ in zip(NAMES, _grads(a), _grads(ref)):
            assert_rel(p_, q_, 2e-5, f"{what}: {nme} vs {tag}", row_factor=rf)


def _mse_case(dev, extent, origins, passes=1, mip=0, **kw):
    from neural_image_compression_v2_amd import fused
    g0, g1, mlp = _inputs(mip)
    g0, g1 = g0.to(dev), g1.to(dev)
    params = [q.to(dev) for q in mlp.tensors()]
    n = len(origins) * extent[0] * extent[1] * passes
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    geo = _geo(extent, len(origins), passes, mip, **kw)
    outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, g0, g1, origins, params, target, want_y=True))
    return outs, n, (geo, g0, g1, params, target)


SHAPES = [
    # extent, origins, passes, mip, max_workgroups
    ((64, 4), [(8, 8)], 3, 0, 0),                       # one macro-tile, 48 rounds (as 16 units of 3)
    ((64, 4), [(8, 8)], 1, 0, 0),
    ((256, 128), [(0, 0)], 3, 0, 16),                   # whole units of 48 rounds, in one piece and cut in two by the shift
    ((10, 9), [(3, 5), (20, 7)], 1, 2, 0),              # one round per unit
    ((10, 9), [(3, 5), (12, 0)], 1, 3, 0),
    ((40, 24), [(3, 5), (50, 30)], 1, 1, 0),            # four rounds per unit
    ((256, 256), [(0, 0), (0, 0)], 1, 0, 0),            # > 8 workgroups, round groups, units cut in two by the shift
    ((256, 256), [(0, 0), (0, 0)], 1, 0, 16),           # .. and as whole units of segment 0
    ((256, 132), [(0, 0)], 1, 0, 0),                    # the smallest whole-chip launch with a non-zero shift
    ((64, 36), [(8, 8)], 1, 0, 16),                     # the smallest launch with a non-zero shift
    ((150, 70), [(3, 5)], 1, 0, 0),                     # unaligned origin, edge tiles
    ((1, 1), [(3, 5)], 1, 0, 0),                        # a single sample
    ((16, 4), [(3, 5)], 1, 0, 0),                       # cells partly outside the crop
    ((37, 21), [(3, 5)], 1, 0, 0),
]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: f"{'x'.join(map(str, c[0]))}-{len(c[1])}crops-p{c[2]}-mip{c[3]}-wg{c[4]}")
def test_dx_once_matches_fp32_and_32_sample_kernels(dev, case):
    """The unit schedules of the module docstring: long running sums, single-term sums, units cut in two by the stagger shift, round groups
    summed through LDS, edge tiles, cells partly outside the crop, a single sample."""
    from neural_image_compression_v2_amd import fused
    extent, origins, passes, mip, mw = case
    outs, n, (geo, g0, g1, params, target) = _mse_case(dev, extent, origins, passes, mip, max_workgroups=mw)
    _hold(outs, n, "shape")
    if passes == 1 and mip == 0:
        # run to run: the decoder gradients and the loss come from fixed-order reductions
        b = fused.fused_forward_backward(geo(split_bf16=True), g0, g1, origins, params, target)
        for p_, q_ in zip(outs["t16"].grad_mlp, b.grad_mlp):
            assert torch.equal(p_, q_), "decoder gradients are bit-stable run to run"
        assert torch.equal(outs["t16"].loss, b.loss)


ENTRY_EXTENT, ENTRY_ORIGINS = (40, 24), [(3, 5), (20, 0)]


def _entry_image(dev):
    gen = torch.Generator().manual_seed(21)
    isz = [max(o[a] for o in ENTRY_ORIGINS) + ENTRY_EXTENT[a] for a in range(2)]
    return torch.randint(0, 256, (3, *isz), generator=gen, dtype=torch.uint8).to(dev)


@pytest.mark.parametrize("entry", ["target-tri", "target-sin", "image-u8", "image-f32", "image-rgbx", "mse-no-y", "dy"])
def test_dx_once_every_entry_point(dev, entry):
    """MODE_TRAIN_MSE on a target tensor (both PE layouts; with and without the y output), MODE_TRAIN_IMG on the planar uint8 and fp32 resident
    image, MODE_TRAIN_RGBX on the interleaved image, MODE_TRAIN_DY through autograd.  The target-tensor step is also held to the CPU oracle at
    the tolerances of test_split_bf16_training_step (y 5e-6, loss 1e-5, gradients 1e-4)."""
    from neural_image_compression_v2_amd import fused
    from neural_image_compression_v2_amd.sampler import rgbx_interleave
    extent, origins = ENTRY_EXTENT, ENTRY_ORIGINS
    n = len(origins) * extent[0] * extent[1]
    g0, g1, mlp = _inputs(0)
    g0d, g1d = g0.to(dev), g1.to(dev)
    params = [q.to(dev) for q in mlp.tensors()]
    tri = entry != "target-sin"
    geo = _geo(extent, len(origins), use_tri_pe=tri)
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(5))
    if entry in ("target-tri", "target-sin", "mse-no-y"):
        want_y = entry != "mse-no-y"
        outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, g0d, g1d, origins, params, target.to(dev), want_y=want_y))
        _hold(outs, n, entry, with_y=want_y)
        if entry == "target-tri":
            noise = O.kernel_noise(n, 73, 8, seed=NOISE["noise_seed"], offset=NOISE["noise_offset"], sample_base=NOISE["sample_base"])
            ref = O.forward_backward(g0, g1, mlp, origins, extent, 0.25, 0, target, noise, 6)
            a = outs["t16"]
            assert_rel(a.y, ref.y, 5e-6, "y vs the CPU oracle")
            assert_rel(a.loss, ref.loss, 1e-5, "loss vs the CPU oracle")
            for nme, p_, q_ in zip(NAMES, _grads(a), [ref.grad_g0, ref.grad_g1] + list(ref.grad_mlp)):
                assert_rel(p_, q_, 1e-4, f"{nme} vs the CPU oracle")
    elif entry.startswith("image"):
        img = _entry_image(dev)
        timg = {"image-u8": lambda: fused.TargetImage(img, 255.0), "image-f32": lambda: fused.TargetImage(img.to(torch.float32) / 255.0),
                "image-rgbx": lambda: fused.TargetImage(rgbx_interleave(img), 255.0, rgbx=True)}[entry]()
        outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, g0d, g1d, origins, params, timg, want_y=True))
        _hold(outs, n, entry)
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
        _hold(_three(geo, run), n, entry, with_y=False, with_loss=False)


def test_dx_once_16_bit_grid_storage(dev):
    """bf16 grids gathered by the 16-sample kernel, fp32 gradient buckets; the two references have no 16-bit gather and run on the widened
    grids (the widening is exact, so they see the same values)."""
    from neural_image_compression_v2_amd import fused
    extent, origins = (48, 40), [(3, 5), (120, 64), (200, 17)]
    n = len(origins) * extent[0] * extent[1]
    g0, g1, mlp = _inputs(0)
    s0, s1 = g0.to(dev).to(torch.bfloat16), g1.to(dev).to(torch.bfloat16)
    params = [q.to(dev) for q in mlp.tensors()]
    target = torch.rand(n, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    geo = _geo(extent, len(origins))
    outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, *((s0, s1) if tag == "t16" else (s0.float(), s1.float())), origins, params, target,
                                                                    want_y=True))
    assert outs["t16"].grad_g0.dtype == torch.float32 and outs["t16"].grad_g0.shape == s0.shape
    _hold(outs, n, "bf16 grids")


def test_dx_once_cancelling_sum(dev):
    """Targets = the 16-sample kernel's own output of a first call (same noise) -+ 1/8 with a random sign per element: every y - target of the
    compared launch is +- 1/8, the dZ of a cell have equal size and random signs, and the sums over a unit's rounds, a cell's samples and the
    launch cancel to their statistical remainder (the sum over the launch, db3, has mean zero).  The same tolerances hold; G0 is held to
    2e-5 of its largest row.
    (Targets equal to the own output alone, the differences left to a change of the noise, make every dZ near zero - and the test void: with
    rms |y - target| = 2.4e-4 the 2e-7 by which the three kernels' y differ is a 1e-3 relative change of dZ3, and the gradients that never
    pass through dX - b3, W3, b2 - were 9.5e-3, 4.3e-3 and 5.2e-3 off the fp32 kernel.  The differences must stay large against the
    rounding of y for any of the references to say something.)"""
    from neural_image_compression_v2_amd import fused
    extent, origins = (64, 64), [(17, 101), (0, 0)]
    n = len(origins) * extent[0] * extent[1]
    g0, g1, mlp = _inputs(0)
    g0d, g1d = g0.to(dev), g1.to(dev)
    params = [q.to(dev) for q in mlp.tensors()]
    geo = _geo(extent, len(origins))
    first = fused.fused_forward_backward(geo(split_bf16=True), g0d, g1d, origins, params, torch.zeros(n, 3, device=dev), want_y=True)
    sign = (torch.randint(0, 2, (n, 3), generator=torch.Generator().manual_seed(6)) * 2 - 1).to(torch.float32).to(dev)
    target = first.y + 0.125 * sign
    outs = _three(geo, lambda ge, tag: fused.fused_forward_backward(ge, g0d, g1d, origins, params, target, want_y=True))
    d = outs["t16"].y - target
    print(f"cancelling sum: rms |y - target| {float(d.pow(2).mean().sqrt()):.3e}, mean {float(d.mean()):.3e}")
    _hold(outs, n, "cancelling sum")
