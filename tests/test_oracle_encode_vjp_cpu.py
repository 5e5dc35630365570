"""Pins ``oracle.nic_oracle.encode_vjp_f64`` - the float64 reference the GPU tests hold ``nic_encode_backward`` to - against the
dense Jacobian of ``create_decoder_input``, built column by column from unit grids, and its addend counts against a brute-force
count in integer arithmetic.  No GPU."""
import itertools
import math

import pytest
import torch

from oracle import nic_oracle as O

U64 = 2.0 ** -53

CASES = [
    # dim, method, tri, textbook, step, extent, origins, C, P, G0 shape, G1 shape
    pytest.param(2, 1, True, False, 0.25, (5, 3), [(2, 7), (4, 8), (4, 8)], 2, 4, (2, 4, 4), (2, 3, 3), id="2d-step1/4-overlap"),
    pytest.param(2, 1, False, False, 2, (2, 3), [(1, 0)], 2, 2, (2, 7, 8), (2, 4, 5), id="2d-step2-unweighted"),
    pytest.param(2, 1, True, False, 1, (3, 2), [(1, 2)], 1, 2, (1, 5, 5), (1, 4, 3), id="2d-step1"),
    pytest.param(3, 3, True, False, 0.25, (3, 2, 5), [(5, 3, 2), (6, 3, 1)], 1, 2, (1, 3, 3, 4), (1, 2, 2, 3), id="3d-m3-reference-weights"),
    pytest.param(3, 3, True, True, 0.25, (3, 2, 5), [(5, 3, 2), (6, 3, 1)], 1, 2, (1, 3, 3, 4), (1, 2, 2, 3), id="3d-m3-textbook-weights"),
    pytest.param(3, 4, False, False, 0.5, (2, 3, 2), [(1, 0, 3)], 2, 2, (2, 4, 3, 3), (2, 3, 2, 2), id="3d-m4-step1/2"),
]


def _dense_jacobian(shape0, shape1, which, enc):
    """d x / d grid[which] as [N * Cin, numel]: column e = enc(unit grid e) - enc(zero grids); the PE and LOD columns cancel exactly"""
    shapes = (shape0, shape1)
    zero = [torch.zeros(s, dtype=torch.float64) for s in shapes]
    base = enc(*zero).reshape(-1)
    cols = []
    for e in range(math.prod(shapes[which])):
        g = [z.clone() for z in zero]
        g[which].view(-1)[e] = 1.0
        cols.append(enc(*g).reshape(-1) - base)
    return torch.stack(cols, dim=1)


def _brute_counts(dim, method, shape, origins, extent, step, half):
    """(sample, corner) pairs per node of a [(Z,) Y, X] grid, by python loops over integers"""
    corners = O.CORNERS_2D if dim == 2 else (O.CORNERS_3D_TETRA if (method == 4 and not half) else O.CORNERS_3D)
    m = torch.zeros(shape, dtype=torch.int64)
    for o in origins:
        for s in itertools.product(*[range(e) for e in extent]):
            cell = [math.floor((o[a] + s[a]) * step / (2 if half else 1)) for a in range(dim)]      # exact: step is a power of two
            for off in corners:
                m[tuple(cell[a] + off[a] for a in reversed(range(dim)))] += 1
    return m


@pytest.mark.parametrize("dim,method,tri,textbook,step,extent,origins,C,P,s0,s1", CASES)
def test_encode_vjp_f64_matches_the_dense_jacobian(dim, method, tri, textbook, step, extent, origins, C, P, s0, s1):
    kw = dict(method=method, use_tri_pe=tri, textbook_weights=textbook)
    enc = lambda a, b: O.create_decoder_input(a, b, origins, extent, step, 0, P, dtype=torch.float64, **kw)
    n = len(origins) * math.prod(extent)
    cin = O.decoder_input_channels(C, P, dim, method)
    dx = torch.randn(n, cin, generator=torch.Generator().manual_seed(17), dtype=torch.float64)
    r = O.encode_vjp_f64(s0, s1, origins, extent, step, P, dx, **kw)
    for which, shape, grad, ab, m in ((0, s0, r.grad_g0, r.abs_g0, r.m0), (1, s1, r.grad_g1, r.abs_g1, r.m1)):
        assert grad.dtype == torch.float64 and ab.dtype == torch.float64 and m.dtype == torch.int64
        J = _dense_jacobian(s0, s1, which, enc)
        assert bool((J >= 0).all()), "the encoding's weights are non-negative"
        want = (J.T @ dx.reshape(-1)).reshape(shape)
        want_abs = (J.T @ dx.abs().reshape(-1)).reshape(shape)
        count = _brute_counts(dim, method, shape[1:], origins, extent, step, half=bool(which))
        assert torch.equal(m, count), f"G{which}: addend counts"
        # two float64 sums of at most m addends (a weight of up to three factors each): both within (m + 3) 2^-53 of the magnitude sum
        tol = 2.0 * (count.unsqueeze(0).double() + 4.0) * U64 * want_abs
        assert bool(((grad - want).abs() <= tol).all()), f"G{which}: J^T dx off by {float((grad - want).abs().max()):.3e}"
        assert bool(((ab - want_abs).abs() <= tol).all()), f"G{which}: |J|^T |dx| off by {float((ab - want_abs).abs().max()):.3e}"
        assert bool((grad[:, count == 0] == 0).all()) and bool((ab[:, count == 0] == 0).all()), f"G{which}: an untouched node is not zero"
        assert int(count.sum()) == n * len(O.CORNERS_2D if dim == 2 else (O.CORNERS_3D_TETRA if (method == 4 and which == 0) else O.CORNERS_3D))
        assert bool((ab[:, count > 0] >= grad[:, count > 0].abs() - tol[:, count > 0]).all())


def test_the_two_3d_weight_tables_differ():
    """the reference's permuted G1 factor table (Q1) and the textbook one are different operators: a test that runs both modes on the same
    inputs compares two references, not one twice"""
    s0, s1, org, ext = (1, 3, 3, 3), (1, 2, 2, 3), [(5, 3, 2)], (3, 2, 5)
    dx = torch.randn(30, O.decoder_input_channels(1, 2, 3, 3), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    a = O.encode_vjp_f64(s0, s1, org, ext, 0.25, 2, dx, method=3)
    b = O.encode_vjp_f64(s0, s1, org, ext, 0.25, 2, dx, method=3, textbook_weights=True)
    assert torch.equal(a.grad_g0, b.grad_g0) and torch.equal(a.m1, b.m1)
    assert not torch.allclose(a.grad_g1, b.grad_g1, rtol=1e-3, atol=0.0)
