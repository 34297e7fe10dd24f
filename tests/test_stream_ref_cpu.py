"""tests/stream_ref.py -- the fp64 models the streaming kernels are held against (tests/test_gpu_streaming.py) -- against torch's
own float64 operators: F.interpolate and its autograd, F.max_pool2d and its autograd.  Runs without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import stream_ref as SR

F64 = torch.float64
N, C = 3, 5
UP_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (7, 9)]
POOL_SIZES = [(2, 2), (2, 5), (5, 2), (3, 3), (7, 9), (10, 8)]
TOL = 1e-12


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def torch_up(x):
    return nhwc(F.interpolate(nchw(x), scale_factor=2, mode='bilinear', align_corners=False))


@pytest.mark.parametrize('H,W', UP_SIZES)
def test_upsample2x_fwd_is_interpolate(H, W):
    x = randn(1, N, H, W, C)
    y, S = SR.upsample2x_fwd(x)
    ref = torch_up(x)
    assert y.shape == ref.shape == (N, 2 * H, 2 * W, C)
    assert float((y - ref).abs().max()) <= TOL
    # S is the same map of |x|, and bounds |y|
    assert float((S - torch_up(x.abs())).abs().max()) <= TOL
    assert bool((S >= y.abs() - TOL).all())


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('H,W', UP_SIZES)
def test_upsample2x_bwd_is_autograd_of_interpolate(H, W, accumulate):
    y = randn(2, N, 2 * H, 2 * W, C)
    old = randn(3, N, H, W, C)
    x = torch.zeros(N, H, W, C, dtype=F64, requires_grad=True)
    torch_up(x).backward(y)
    ref = x.grad + (old if accumulate else 0.0)
    got, S = SR.upsample2x_bwd(y, old if accumulate else None, accumulate)
    assert got.shape == (N, H, W, C)
    assert float((got - ref).abs().max()) <= TOL
    xa = torch.zeros(N, H, W, C, dtype=F64, requires_grad=True)
    torch_up(xa).backward(y.abs())
    assert float((S - (xa.grad + (old.abs() if accumulate else 0.0))).abs().max()) <= TOL


@pytest.mark.parametrize('H,W', UP_SIZES)
def test_upsample2x_adjoint_identity(H, W):
    x, y = randn(4, N, H, W, C), randn(5, N, 2 * H, 2 * W, C)
    lhs = float((SR.upsample2x_fwd(x)[0] * y).sum())
    rhs = float((x * SR.upsample2x_bwd(y)[0]).sum())
    scale = float((SR.upsample2x_fwd(x.abs())[0] * y.abs()).sum())
    assert abs(lhs - rhs) <= TOL * max(scale, 1.0)


def test_upsample2x_weights_of_every_source_sum_to_four():
    """Each axis doubles, so the transpose of a constant 1 is 4 everywhere, borders included."""
    for H, W in UP_SIZES:
        got, _ = SR.upsample2x_bwd(torch.ones(1, 2 * H, 2 * W, 1, dtype=F64))
        assert float((got - 4.0).abs().max()) <= TOL


def ties(seed, H, W):
    return torch.randint(0, 4, (N, H, W, C), generator=torch.Generator().manual_seed(seed)).to(F64)


@pytest.mark.parametrize('H,W', POOL_SIZES)
def test_maxpool2x2_fwd_is_max_pool2d(H, W):
    x = ties(6, H, W)
    y, S = SR.maxpool2x2_fwd(x)
    assert torch.equal(y, nhwc(F.max_pool2d(nchw(x), 2)))
    assert torch.equal(S, y.abs())


@pytest.mark.parametrize('H,W', POOL_SIZES)
def test_maxpool2x2_bwd_is_autograd_of_max_pool2d_on_ties(H, W):
    x = ties(7, H, W)
    dy = randn(8, N, H // 2, W // 2, C)
    old = randn(9, N, H, W, C)
    xt = nchw(x).clone().requires_grad_(True)
    F.max_pool2d(xt, 2).backward(nchw(dy).contiguous())
    grad = nhwc(xt.grad)
    dx, S, k = SR.maxpool2x2_bwd(x, dy, old)
    assert torch.equal(dx, old + grad)               # one add per element: the same double
    assert torch.equal(S, old.abs() + grad.abs())
    # an odd last row / column receives nothing
    assert torch.equal(dx[:, 2 * (H // 2):], old[:, 2 * (H // 2):]) and torch.equal(dx[:, :, 2 * (W // 2):], old[:, :, 2 * (W // 2):])
    # the winner is the first maximum in scan order: nothing before it in its window is as large
    v = SR._windows(x)
    m = v.max(dim=3).values
    for j in range(4):
        here = k == j
        assert torch.equal(v[:, :, :, j][here], m[here])
        for i in range(j):
            assert bool((v[:, :, :, i][here] < m[here]).all())
    # with this many ties every position wins somewhere (5 x 2 and larger)
    if H * W >= 10:
        assert sorted(k.unique().tolist()) == [0, 1, 2, 3]


def test_bn_relu_bwd_is_strict_and_colstats_add_up():
    r = torch.tensor([[0.0, -0.0, 2.0 ** -126, -1.0, 3.0]], dtype=F64).t().repeat(1, 2)
    dy = randn(10, 5, 2)
    coef = randn(11, 3, 2)
    d, S = SR.bn_relu_bwd(dy, r, coef)
    assert torch.equal(d[:2], torch.zeros(2, 2, dtype=F64)) and torch.equal(d[3], torch.zeros(2, dtype=F64))
    assert torch.equal(d[2], coef[0] * dy[2] + coef[1] * r[2] + coef[2]) and torch.equal(d[4], coef[0] * dy[4] + coef[1] * r[4] + coef[2])
    assert bool((S >= d.abs()).all()) and torch.equal(S[:2], torch.zeros(2, 2, dtype=F64))
    d0, S0 = SR.bn_relu_bwd(dy, r, None)
    assert torch.equal(d0, torch.where(r > 0, dy, torch.zeros((), dtype=F64))) and torch.equal(S0, d0.abs())
    s, Ss = SR.colstats(dy, r)
    assert torch.equal(s[0], dy.sum(0)) and torch.equal(s[1], (dy * r).sum(0)) and torch.equal(Ss[1], (dy * r).abs().sum(0))
    s2, _ = SR.colstats(dy)
    assert torch.equal(s2[1], (dy * dy).sum(0))


def test_affine_copy_windows():
    x, y = randn(12, 2, 6, 7, 3), randn(13, 2, 5, 9, 3)
    sc, sh = randn(14, 3), randn(15, 3)
    for acc in (False, True):
        out, S = SR.affine_copy(x, y, 2, 3, 4, 1, 1, 5, sc, sh, acc)
        exp = y.clone()
        exp[:, 1:3, 5:8] = x[:, 4:6, 1:4] * sc + sh + (y[:, 1:3, 5:8] if acc else 0.0)
        assert torch.equal(out, exp)
        assert float(S[:, 0].abs().max()) == 0.0 and bool((S[:, 1:3, 5:8] >= out[:, 1:3, 5:8].abs()).all())
    out, S = SR.affine_copy(x, y, 2, 3, 4, 1, 1, 5)
    assert torch.equal(out[:, 1:3, 5:8], x[:, 4:6, 1:4]) and torch.equal(S[:, 1:3, 5:8], x[:, 4:6, 1:4].abs())
