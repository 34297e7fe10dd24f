"""The serial phases of the bf16 weight-gradient kernel (csrc/wgradp_bf16.hip) at the smallest shapes at which each can go
wrong: the scalar, table-prefetching k-step loop (waves with 0, 1, 2 and 3 steps, both loop bodies), the bias-gradient column
sums read four rows at a time (every remainder), the cross-phase sums in one pass (single slot and slices) and the unit
positions placed by a running (image, row, column) counter.  pytest -m gpu.

Bar: the one of test_gpu_bf16.py::test_wgradp -- fp64 torch.nn.grad.conv2d_weight on the same bf16-rounded operands,
rtol 2e-5, atol 3e-5 max|ref| (fp32 accumulation order is all that differs), the same for the bias sums against the fp64
column sums.  Every case is launched twice: the kernel has a fixed summation order, so the two results are the same bits."""
import numpy as np
import pytest
import torch

from dfl_amd import _native as nat
from test_gpu_bf16 import wgrad_bf16, rb, brb_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _mode4():
    lib = nat.lib()
    prev = lib.dfl_get_math_mode()
    nat.check(lib.dfl_set_math_mode(4), 'dfl_set_math_mode')
    yield
    nat.check(lib.dfl_set_math_mode(prev), 'dfl_set_math_mode')


def run_case(N, Cg, Cm, H, W, K=3, stride=1, pad=1, force_splits=None, in_aff=False, bias=None):
    """bias: None, 'brb' (fused BatchNorm + ReLU backward operand) or 'plain' (bias_plain).  Asserts value and repeatability."""
    g = torch.Generator().manual_seed(N + 3 * Cg + 5 * Cm + 7 * H + 11 * W + 13 * K)
    x = rb(torch.randn(N, Cg, H, W, generator=g))
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    d = rb(torch.randn(N, Cm, Ho, Wo, generator=g))
    aff, xa = None, x
    if in_aff:
        sc, sh = torch.rand(Cg, generator=g) + 0.5, torch.randn(Cg, generator=g) * 0.3
        aff = (sc, sh)
        xa = rb((x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).float())   # fmaf: one rounding
    kw = dict(in_aff=aff, force_splits=force_splits)
    dense = d
    if bias == 'brb':
        r = rb(torch.relu(torch.randn(N, Cm, Ho, Wo, generator=g)))
        coef = torch.stack([torch.rand(Cm, generator=g) + 0.5, torch.randn(Cm, generator=g) * 0.3, torch.randn(Cm, generator=g) * 0.1])
        dense = brb_reference(d, r, coef)
        kw['brb'] = (r, coef)
    elif bias == 'plain':
        kw['bias_plain'] = True
    ref = torch.nn.grad.conv2d_weight(xa.double(), (Cm, Cg, K, K), dense.double(), stride=stride, padding=pad)
    out1 = wgrad_bf16(x, d, K, K, stride, pad, Ho, Wo, **kw)
    out2 = wgrad_bf16(x, d, K, K, stride, pad, Ho, Wo, **kw)
    dw1, dw2 = (out1[0], out2[0]) if bias else (out1, out2)
    what = str((N, Cg, Cm, H, W, K, stride, pad, force_splits, in_aff, bias))
    np.testing.assert_allclose(dw1.numpy(), ref.numpy(), rtol=2e-5, atol=3e-5 * float(ref.abs().max()), err_msg=what)
    assert torch.equal(dw1, dw2), 'two launches differ: ' + what
    if bias:
        refb = dense.double().sum(dim=(0, 2, 3))
        np.testing.assert_allclose(out1[1].numpy(), refb.numpy(), rtol=2e-5,
                                   atol=3e-5 * float(dense.double().abs().sum(dim=(0, 2, 3)).max()), err_msg=what)
        assert torch.equal(out1[1], out2[1]), 'two launches differ (bias): ' + what


# k-step loop, N = 1, 3x3, pad 1: Cg, Cm, H, W.  A patch of H x W pixels has ceil(H W / 16) steps, dealt to 4 / 2 / 1 phases
FOUR_PHASES = [(32, 32, 2, 8), (32, 32, 4, 8), (32, 32, 6, 8), (32, 32, 10, 8),      # 1, 2, 3, 5 steps, runs of 8 pixels: three reads per row of taps
               (32, 32, 2, 7), (32, 32, 4, 7), (32, 32, 6, 7), (32, 32, 10, 7)]      # the other loop body, ragged last step
TWO_PHASES = [(64, 32, 4, 8), (64, 32, 6, 8)]
ONE_PHASE = [(64, 64, 4, 8), (64, 64, 6, 8)]


@pytest.mark.parametrize('case', FOUR_PHASES + TWO_PHASES + ONE_PHASE)
def test_kstep_loop_trip_counts(case):
    Cg, Cm, H, W = case
    run_case(1, Cg, Cm, H, W)


@pytest.mark.parametrize('case', [(1, 32, 32, 2, 8, 1, 1, 0), (2, 64, 64, 8, 8, 1, 1, 0), (2, 32, 64, 12, 10, 2, 2, 0)])
def test_kstep_loop_other_windows(case):
    N, Cg, Cm, H, W, K, stride, pad = case
    run_case(N, Cg, Cm, H, W, K, stride, pad)


def test_table_prefetch_across_patches():
    """One slice walks several patches: the table entries of a patch's first step are asked for after its barrier, and the
    last step of every patch asks for nothing beyond the table."""
    run_case(2, 64, 64, 40, 24, force_splits=1)


# bias-gradient column sums: Cm = 32 -> 24 row groups, Cm = 64 -> 12; rows = H * 8
@pytest.mark.parametrize('case', [(32, 2), (32, 6), (32, 14), (64, 2), (64, 6), (64, 8)])
@pytest.mark.parametrize('form', ['brb', 'plain'])
@pytest.mark.parametrize('in_aff', [False, True])
def test_bias_sums_unroll_boundaries(case, form, in_aff):
    Cm, H = case
    run_case(1, 32, Cm, H, 8, in_aff=in_aff, bias=form)


@pytest.mark.parametrize('case', FOUR_PHASES + TWO_PHASES)
@pytest.mark.parametrize('splits', [1, 2, 3])
def test_cross_phase_sums_one_pass(case, splits):
    """splits = 1: the torch-order tile reuses the LDS of the sums right behind them; splits > 1: the waves of phases > 0 leave."""
    Cg, Cm, H, W = case
    run_case(1, Cg, Cm, H, W, force_splits=splits)
