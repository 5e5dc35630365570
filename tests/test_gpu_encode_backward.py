"""The layer-wise encode pair - ``nic_encode`` and ``nic_encode_backward`` (csrc/simple_kernels.hip) - on its own, at the extents, steps
and launch sizes where the backward kernel's patch bookkeeping can go wrong: partial 8 x 8 / 4 x 4 x 4 patches (dead lanes, dead waves, runs
a dead lane cuts), every step from 2^-10 to 4, both 3D weight tables, overlapping crops, non-zero gradient buffers and a launch past
the 2048-block cap.

The backward is called through the C entry point with a seeded ``dx``: no decoder and no loss sit between the kernel and the check.  The
reference is ``oracle.nic_oracle.encode_vjp_f64`` (pinned against the dense Jacobian in tests/test_oracle_encode_vjp_cpu.py) and the
assertion is per element, for every node and channel:

    |got - ref| <= (m + 4) * 2^-24 * abs_ref

with m the number of (sample, corner) addends of the node and abs_ref the sum of their magnitudes.  The bound is derived: a sum of m fp32
addends in any order (the atomics are unordered, so no two runs need agree bit for bit) is within (m - 1) u of the magnitude sum, and
a G1 addend carries at most three more rounded products.  A dropped, doubled or misplaced sample moves a node by about abs_ref / m,
four orders of magnitude above the bound; a node no sample touches has abs_ref = 0 and must be exactly 0.0.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nic_oracle as O  # noqa: E402  (checker only)

U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from neural_image_compression_v2_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Case:
    """One geometry.  The grids are the smallest that hold every corner, so the crop with the largest origin ends on the far edge of every
    axis: its last sample's + 1 corner is the grid's last node."""

    def __init__(self, name, dim, method, step, extent, origins, C=4, P=4, tri=True, textbook=False, slack=0):
        self.name, self.dim, self.method, self.step = name, dim, method, step
        self.extent, self.origins, self.C, self.P, self.tri, self.textbook = tuple(extent), [tuple(o) for o in origins], C, P, tri, textbook
        n0, n1 = [], []
        for a in range(dim):
            qmax = max(o[a] for o in self.origins) + self.extent[a] - 1
            n0.append(math.floor(qmax * step) + 2 + slack)                        # exact: the step is a power of two
            n1.append(math.floor(qmax * step / 2) + 2 + slack)
        self.s0 = (C, *reversed(n0))                                              # [C, (Z,) Y, X]: sample axis 0 is the last tensor axis
        self.s1 = (C, *reversed(n1))
        self.n = len(self.origins) * math.prod(self.extent)
        self.cin = O.decoder_input_channels(C, P, dim, method)
        ps = 8 if dim == 2 else 4
        self.patches = len(self.origins) * math.prod((e + ps - 1) // ps for e in self.extent)
        self.whole = all(e % ps == 0 for e in self.extent) and self.patches % 4 == 0

    def geo(self):
        from neural_image_compression_v2_amd import fused
        return fused.PathGeometry(dim=self.dim, method=self.method, step_number=self.step, mip_level=3.0, extent=self.extent,
                                  num_crops=len(self.origins), channels=self.C, pe_channels=self.P, use_tri_pe=self.tri,
                                  textbook_weights=self.textbook)

    def kw(self):
        return dict(method=self.method, use_tri_pe=self.tri, textbook_weights=self.textbook)

    def __repr__(self):
        return self.name


PARTIAL_2D = [
    Case("2d-1x1-1crop", 2, 1, 0.25, (1, 1), [(6, 9)]),                                          # 1 patch: 63 dead lanes, 3 dead waves
    Case("2d-1x1-3crops", 2, 1, 0.25, (1, 1), [(0, 0), (6, 9), (13, 2)]),
    Case("2d-3x5-1crop", 2, 1, 0.25, (3, 5), [(2, 3)], C=5),
    Case("2d-3x5-3crops", 2, 1, 0.25, (3, 5), [(0, 0), (2, 3), (11, 14)], C=5),                  # 3 patches
    Case("2d-37x21-1crop", 2, 1, 0.25, (37, 21), [(3, 5)]),                                      # 5 x 3 = 15 patches
    Case("2d-37x21-3crops", 2, 1, 0.25, (37, 21), [(3, 5), (40, 2), (43, 38)], tri=False),       # 45 patches; the last crop ends on both far edges
    Case("2d-8x9-1crop", 2, 1, 0.25, (8, 9), [(5, 6)]),                                          # 2 patches, the second a single column
    Case("2d-8x9-3crops", 2, 1, 0.25, (8, 9), [(0, 0), (5, 6), (16, 15)], slack=1),              # 6 patches; grids one node larger than needed
]
PARTIAL_3D = [Case(f"3d-m{m}-{'x'.join(map(str, e))}-{len(o)}crops", 3, m, 0.25, e, o)
              for m in (3, 4)
              for e, o in (((5, 3, 7), [(0, 0, 0), (11, 9, 6)]),                                 # the second crop ends on the far edge of all three axes
                           ((9, 6, 7), [(3, 1, 2)]),                                             # 3 x 2 x 2 = 12 patches
                           ((9, 6, 7), [(3, 1, 2), (0, 0, 0), (8, 7, 5)]),
                           ((1, 1, 1), [(2, 5, 3)]),
                           ((1, 1, 1), [(2, 5, 3), (0, 0, 0), (7, 7, 7)]))]
# whole patches, a multiple of four of them: what the dead-lane code never sees.  Step 2 is the reference's unweighted G1 (its guard
# int(1 // (step / 2)) != 1 fails there only); at 4 the weights are back on with k = 0
STEPS = ([Case(f"2d-step{s}", 2, 1, s, (16, 16), [(3, 6), (9, 1)]) for s in (0.25, 0.5, 1, 2, 4)]
         + [Case(f"3d-m3-step{s}", 3, 3, s, (8, 8, 4), [(3, 6, 1), (2, 1, 5)]) for s in (0.25, 0.5, 1, 2, 4)]
         + [Case("2d-step2^-10", 2, 1, 2.0 ** -10, (64, 72), [(5, 3), (1000, 2040)])])          # a wave inside one cell: runs of 64; the second crop crosses a G0 and a G1 cell edge
WEIGHTS_3D = [Case(f"3d-m{m}-{'textbook' if tb else 'reference'}", 3, m, 0.25, (5, 3, 7), [(1, 2, 3), (6, 5, 2)], textbook=tb) for m in (3, 4) for tb in (False, True)]
OVERLAP = [Case("2d-overlap", 2, 1, 0.25, (13, 10), [(4, 4), (4, 4), (9, 7)]),
           Case("3d-m4-overlap", 3, 4, 0.25, (5, 6, 4), [(1, 1, 1), (1, 1, 1), (3, 2, 2)]),
           Case("2d-overlap-whole", 2, 1, 0.25, (16, 16), [(4, 4), (4, 4), (9, 7), (12, 12)])]
PAST_CAP = Case("2d-728x724-past-the-cap", 2, 1, 0.25, (728, 724), [(2, 1)], C=1, P=2)           # 91 x 91 = 8281 patches > 4 x 2048; 527 072 samples > 2048 x 256
ALL = PARTIAL_2D + PARTIAL_3D + STEPS + WEIGHTS_3D + OVERLAP + [PAST_CAP]


def test_the_cases_reach_the_paths_they_are_named_for():
    assert any(c.patches % 4 for c in PARTIAL_2D) and any(c.patches % 4 for c in PARTIAL_3D)
    assert not any(c.whole for c in PARTIAL_2D + PARTIAL_3D + WEIGHTS_3D) and all(c.whole for c in STEPS)
    assert PAST_CAP.patches == 8281 > 4 * 2048 and PAST_CAP.n > 2048 * 256
    assert len({c.name for c in ALL}) == len(ALL)


_DX, _REF = {}, {}


def _dx(case):
    if case.name not in _DX:
        g = torch.Generator().manual_seed(1000 + sum(map(ord, case.name)))
        _DX[case.name] = torch.randn(case.n, case.cin, generator=g)
    return _DX[case.name]


def _ref(case):
    """the float64 reference of a case, computed once and shared"""
    if case.name not in _REF:
        _REF[case.name] = O.encode_vjp_f64(case.s0, case.s1, case.origins, case.extent, case.step, case.P, _dx(case), **case.kw())
    return _REF[case.name]


def _backward(dev, case, dx, pre0=None, pre1=None):
    """nic_encode_backward through the C entry point into buffers that start at zero or at the given values"""
    from neural_image_compression_v2_amd import _lib, fused
    geo = case.geo()
    gg0 = torch.zeros(case.s0, device=dev) if pre0 is None else pre0.to(dev)
    gg1 = torch.zeros(case.s1, device=dev) if pre1 is None else pre1.to(dev)
    host = torch.tensor(case.origins, dtype=torch.int64)
    fused.check_origins(geo, host, gg0, gg1)                          # the oracle does not clamp: every corner is inside its grid
    org = host.to(torch.int32).to(dev)
    dxd = dx.to(dev).contiguous()
    d = geo.to_desc(gg0, gg1)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nic_encode_backward(ctypes.byref(d), _lib.ptr(org), _lib.ptr(dxd), _lib.ptr(gg0), _lib.ptr(gg1),
                                                   _lib.stream_ptr(dev)), "nic_encode_backward")
    torch.cuda.synchronize()
    return gg0.cpu(), gg1.cpu()


def _ulp(x):
    """spacing of fp32 at |x| (a double tensor)"""
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def _check(case, got0, got1, ref, pre0=None, pre1=None):
    for name, got, grad, ab, m, pre in (("G0", got0, ref.grad_g0, ref.abs_g0, ref.m0, pre0), ("G1", got1, ref.grad_g1, ref.abs_g1, ref.m1, pre1)):
        assert got.shape == grad.shape, (name, got.shape, grad.shape)
        mm = m.unsqueeze(0).expand_as(grad)
        bound = (mm.double() + 4.0) * U * ab
        want = grad
        if pre is not None:
            want = pre.double() + grad
            bound = bound + _ulp(pre.double())
        err = (got.double() - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"{case.name} {name}: max m {int(m.max())}, untouched nodes {int((m == 0).sum())}, worst error / bound {ratio:.3f}")
        bad = err > bound
        assert not bool(bad.any()), (f"{case.name} {name}: {int(bad.sum())} of {bad.numel()} entries outside (m + 4) 2^-24 abs_ref, worst at "
                                     f"{tuple(int(v) for v in torch.nonzero(bad)[0])}: error {float(err[bad].max()):.3e}, error / bound {ratio:.3e}")
        idle = mm == 0
        assert torch.equal(got[idle], torch.zeros_like(got[idle]) if pre is None else pre[idle]), f"{case.name} {name}: an untouched node changed"
        assert bool((m > 0).any())


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_encode_backward_matches_the_f64_vjp(dev, case):
    got0, got1 = _backward(dev, case, _dx(case))
    _check(case, got0, got1, _ref(case))


@pytest.mark.parametrize("method", [3, 4])
def test_the_3d_weight_modes_are_held_to_different_references(dev, method):
    ref_case, tb_case = [c for c in WEIGHTS_3D if c.method == method]
    assert (ref_case.textbook, tb_case.textbook) == (False, True) and ref_case.origins == tb_case.origins
    dx = _dx(ref_case)
    a = O.encode_vjp_f64(ref_case.s0, ref_case.s1, ref_case.origins, ref_case.extent, 0.25, ref_case.P, dx, **ref_case.kw())
    b = O.encode_vjp_f64(tb_case.s0, tb_case.s1, tb_case.origins, tb_case.extent, 0.25, tb_case.P, dx, **tb_case.kw())
    gap = (a.grad_g1 - b.grad_g1).abs()
    assert float((gap / a.abs_g1.clamp_min(1e-300)).max()) > 1e-2, "the two weight tables gave the same reference: one mode would be tested twice"
    from neural_image_compression_v2_amd import _lib
    assert ref_case.geo().g1_mode() == _lib.NIC_G1_REFERENCE and tb_case.geo().g1_mode() == _lib.NIC_G1_TEXTBOOK
    for case, ref in ((ref_case, a), (tb_case, b)):                   # the SAME dx under both modes
        got0, got1 = _backward(dev, case, dx)
        _check(case, got0, got1, ref)


@pytest.mark.parametrize("case", [PARTIAL_2D[3], PARTIAL_2D[5], PARTIAL_3D[2], OVERLAP[0], STEPS[3]], ids=repr)
def test_encode_backward_accumulates_into_its_buffers(dev, case):
    """the kernel adds; only EncodeFunction zero-fills.  Result = pre-fill + VJP within the same bound plus one ulp of the pre-fill"""
    g = torch.Generator().manual_seed(77)
    pre0, pre1 = torch.randn(case.s0, generator=g), torch.randn(case.s1, generator=g)
    got0, got1 = _backward(dev, case, _dx(case), pre0.clone(), pre1.clone())
    _check(case, got0, got1, _ref(case), pre0, pre1)


@pytest.mark.parametrize("case", [PARTIAL_2D[5], PARTIAL_3D[1]], ids=repr)
def test_encode_differentiable_with_a_strided_upstream_gradient(dev, case):
    """through autograd: backpropagating a product with the transposed encoding hands EncodeFunction a transposed (non-contiguous) view,
    which it must copy (require_cuda_f32), and its gradient buffers must start at zero"""
    from neural_image_compression_v2_amd import fused
    g = torch.Generator().manual_seed(5)
    g0 = (torch.rand(case.s0, generator=g) - 0.5).to(dev).requires_grad_(True)
    g1 = (torch.rand(case.s1, generator=g) - 0.5).to(dev).requires_grad_(True)
    wt = _dx(case).t().contiguous().to(dev)                           # [Cin, N]
    seen = []
    x = fused.encode_differentiable(case.geo(), g0, g1, case.origins)
    x.register_hook(lambda gr: seen.append(gr.is_contiguous()))
    (x.t() * wt).sum().backward()
    assert seen == [False], "the upstream gradient was expected to arrive as a strided view"
    _check(case, g0.grad.cpu(), g1.grad.cpu(), _ref(case))


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_encode_forward_on_the_same_geometries(dev, case):
    """nic_encode against the fp32 oracle with the asserts of test_encode_matches_oracle: exact, 5e-7 on sinusoidal PE rows"""
    from neural_image_compression_v2_amd import fused
    g = torch.Generator().manual_seed(9)
    g0, g1 = torch.rand(case.s0, generator=g) - 0.498, torch.rand(case.s1, generator=g) - 0.498
    ref = O.create_decoder_input(g0, g1, case.origins, case.extent, case.step, 3.0, case.P, **case.kw())
    out = fused.encode(case.geo(), g0.to(dev), g1.to(dev), case.origins).cpu()
    assert out.shape == ref.shape
    tri = case.tri if case.dim == 2 else case.method == 3
    pe0 = ((4 if (case.dim == 2 or case.method == 4) else 8) + 1) * case.C
    assert torch.equal(out[:, :pe0], ref[:, :pe0]), f"grid channels: max abs diff {float((out[:, :pe0] - ref[:, :pe0]).abs().max()):.3e}"
    assert torch.equal(out[:, -1], ref[:, -1]), "lod"
    if tri:
        assert torch.equal(out[:, pe0:-1], ref[:, pe0:-1]), "triangular PE"
    else:
        assert float((out[:, pe0:-1] - ref[:, pe0:-1]).abs().max()) <= 5e-7, "sinusoidal PE"
