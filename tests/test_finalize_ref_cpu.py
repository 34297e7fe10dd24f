"""tests/finalize_ref.py -- the fp64 models the finalize, reduction and optimizer kernels are held against
(tests/test_gpu_finalize.py) -- against independent definitions: F.batch_norm and its autograd in float64, torch.optim.SGD / Adam /
RMSprop in float64, and a view / transpose.  Runs without a GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import finalize_ref as FR

F64 = torch.float64
TOL = 1e-12
M, C = 37, 5
EPS, MOM = 1e-5, 0.1


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def close(a, b, scale=1.0):
    return float((a - b).abs().max()) <= TOL * max(scale, 1.0)


# ---------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize('n,T', [(12, 1), (12, 2), (12, 4), (36, 9), (9, 9), (5, 1)])
def test_reduce_slices_is_a_sum_and_a_transpose(n, T):
    src = FR.exact_data(torch.Generator().manual_seed(1), 7, n)       # sums of it are exact: no order to agree on
    dst, S = FR.reduce_slices(src, T)
    assert torch.equal(dst, src.sum(0).view(T, n // T).t().reshape(-1))
    assert torch.equal(S, src.abs().sum(0).view(T, n // T).t().reshape(-1))
    # the header's words: dst[r*T + t] = sum_s src[s*n + t*(n/T) + r]
    R = n // T
    for r in range(R):
        for t in range(T):
            assert float(dst[r * T + t]) == float(src[:, t * R + r].sum())


def test_exact_data_sums_exactly_in_any_order():
    g = torch.Generator().manual_seed(2)
    v = FR.exact_data(g, 2 ** 14, 3)
    assert torch.equal(v.float().double(), v) and float(v.abs().max()) < 2 ** 10
    fwd, bwd = v.cumsum(0)[-1], v.flip(0).cumsum(0)[-1]
    ints = (v * 2 ** 10).long().sum(0)                              # the same sum in integers
    assert torch.equal(fwd, bwd) and torch.equal((fwd * 2 ** 10).long(), ints)
    q = FR.quantize(randn(3, 50) * 100)
    assert torch.equal(q.float().double(), q) and torch.equal(q * 2 ** 10, torch.round(q * 2 ** 10))


# ---------------------------------------------------------------------------------------------------- BatchNorm
def bn_case(seed, count=M):
    x = randn(seed, count, C) * torch.linspace(0.5, 3.0, C, dtype=F64) + torch.linspace(-2.0, 2.0, C, dtype=F64)
    gamma, beta = randn(seed + 1, C) + 1.5, randn(seed + 2, C)
    rm, rv = randn(seed + 3, C), randn(seed + 4, C).abs() + 0.5
    return x, gamma, beta, rm, rv


@pytest.mark.parametrize('count', [M, 2, 1])
def test_bn_finalize_is_batch_norm_in_training_mode(count):
    x, gamma, beta, rm, rv = bn_case(10, count)
    eps, mom = FR.f32(EPS), FR.f32(MOM)              # the model reads them as the C floats they are passed as
    out = FR.bn_finalize(x.sum(0), (x * x).sum(0), gamma, beta, count, EPS, MOM, rm, rv)
    scale, shift = out['scale'][0], out['shift'][0]
    if count > 1:
        trm, trv = rm.clone(), rv.clone()
        y = F.batch_norm(x, trm, trv, gamma, beta, training=True, momentum=mom, eps=eps)
        assert close(x * scale + shift, y, float(y.abs().max()))
        assert close(out['running_mean'][0], trm) and close(out['running_var'][0], trv, float(trv.abs().max()))
    else:
        # one element per channel: torch refuses; the definition gives mean = x, var = 0, and "unbiased" stays the biased 0
        assert close(out['save_mean'][0], x[0]) and float(out['var'][0].abs().max()) <= 1e-12 * float((x * x).max())
        assert close(out['running_var'][0], (1.0 - mom) * rv + mom * out['var'][0])
    assert close(out['save_mean'][0], x.mean(0))
    assert close(out['save_invstd'][0], 1.0 / torch.sqrt(x.var(0, unbiased=False) + eps), 1.0 / math.sqrt(eps))
    for name, (ref, S) in out.items():
        assert bool((S >= ref.abs() * (1 - 1e-12)).all()), name


def test_bn_finalize_clamps_a_negative_variance_and_leaves_no_state_without_running_stats():
    s1, s2 = torch.tensor([192.0, 64.0], dtype=F64), torch.tensor([576.0 - 2.0 ** -10, 128.0], dtype=F64)
    out = FR.bn_finalize(s1, s2, torch.ones(2, dtype=F64), torch.zeros(2, dtype=F64), 64, EPS)
    assert out['var'][0].tolist() == [0.0, 1.0]
    assert float(out['save_invstd'][0][0]) == 1.0 / math.sqrt(FR.f32(EPS))
    assert 'running_mean' not in out and 'running_var' not in out


def test_bn_bwd_finalize_is_autograd_of_batch_norm():
    r, gamma, beta, _, _ = bn_case(20)
    dy = randn(25, M, C) * torch.linspace(1.0, 2.0, C, dtype=F64) + 0.25
    rt, gt, bt = r.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    F.batch_norm(rt, None, None, gt, bt, training=True, eps=FR.f32(EPS)).backward(dy)
    fwd = FR.bn_finalize(r.sum(0), (r * r).sum(0), gamma, beta, M, EPS)
    out = FR.bn_bwd_finalize(dy.sum(0), (dy * r).sum(0), gamma, fwd['save_mean'][0], fwd['save_invstd'][0], M)
    big = float(fwd['save_invstd'][0].max()) ** 2 * float(dy.abs().sum())
    assert close(out['dgamma'][0], gt.grad, big) and close(out['dbeta'][0], bt.grad, big)
    A, B, Cc = out['coef'][0]
    assert close(A * dy + B * r + Cc, rt.grad, big)
    for name, (ref, S) in out.items():
        assert bool((S >= ref.abs() * (1 - 1e-12)).all()), name


def test_bn_bwd_finalize_in_eval_mode_is_autograd_of_the_constant_affine():
    r, gamma, beta, rm, rv = bn_case(30)
    dy = randn(35, M, C)
    rt = r.clone().requires_grad_(True)
    F.batch_norm(rt, rm, rv, gamma, beta, training=False, eps=FR.f32(EPS)).backward(dy)
    invstd = 1.0 / torch.sqrt(rv + FR.f32(EPS))
    out = FR.bn_bwd_finalize(dy.sum(0), (dy * r).sum(0), gamma, rm, invstd, 0)
    A, B, Cc = out['coef'][0]
    assert torch.equal(A, gamma * invstd) and not bool(B.any()) and not bool(Cc.any())
    assert close(A * dy, rt.grad)
    assert not bool(out['coef'][1][1:].any())


def test_bn_eval_is_batch_norm_in_eval_mode():
    x, gamma, beta, rm, rv = bn_case(40)
    (scale, Ss), (shift, Sh) = FR.bn_eval(gamma, beta, rm, rv, EPS)
    y = F.batch_norm(x, rm, rv, gamma, beta, training=False, eps=FR.f32(EPS))
    assert close(x * scale + shift, y, float(y.abs().max()))
    assert torch.equal(Ss, scale.abs()) and bool((Sh >= shift.abs()).all())


# ---------------------------------------------------------------------------------------------------- optimizers
N_OPT, STEPS = 101, 3


def opt_case(seed):
    return randn(seed, N_OPT), [randn(seed + 1 + t, N_OPT) * (1.0 + t) for t in range(STEPS)]


def exact32(*vals):
    """Hyper-parameters that are exact fp32 values, so torch (which keeps Python floats) and the model (which reads C floats) agree."""
    assert all(FR.f32(v) == v for v in vals)
    return vals


@pytest.mark.parametrize('momentum,nesterov', [(0.0, False), (0.875, False), (0.875, True)])
@pytest.mark.parametrize('wd', [0.0, 2.0 ** -10])
def test_sgd_model_is_torch_sgd(momentum, nesterov, wd):
    lr, momentum, wd = exact32(0.125, momentum, wd)
    w0, grads = opt_case(50)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    w, buf = w0.clone(), (randn(59, N_OPT) if momentum else None)      # stale data in the buffer: the first step overwrites it
    for t in range(STEPS):
        p.grad = grads[t].clone()
        opt.step()
        (w, S), nb = FR.sgd_step(w, grads[t], buf, lr, momentum, wd, 1.0, int(nesterov), int(t == 0))
        assert close(w, p.detach()) and bool((S >= w.abs() * (1 - 1e-12)).all())
        if momentum:
            buf = nb[0]
            assert close(buf, opt.state[p]['momentum_buffer'])
        else:
            assert nb is None


def test_sgd_grad_scale_multiplies_the_gradient_only():
    w0, grads = opt_case(60)
    (a, _), _ = FR.sgd_step(w0, grads[0], None, 0.125, 0.0, 0.25, 0.5, 0, 0)
    (b, _), _ = FR.sgd_step(w0, grads[0] * 0.5, None, 0.125, 0.0, 0.25, 1.0, 0, 0)
    assert torch.equal(a, b)


@pytest.mark.parametrize('wd', [0.0, 2.0 ** -10])
def test_adam_model_is_torch_adam(wd):
    lr, b1, b2, eps, wd = exact32(2.0 ** -7, 0.875, 0.96875, 2.0 ** -20, wd)
    w0, grads = opt_case(70)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    w, m, v = w0.clone(), torch.zeros(N_OPT, dtype=F64), torch.zeros(N_OPT, dtype=F64)
    for t in range(1, STEPS + 1):
        p.grad = grads[t - 1].clone()
        opt.step()
        step_size, bc2 = lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
        # the model reads both as C floats: their rounding moves the step by 2^-24 of itself, which is what is allowed here
        (w, S), (m, _), (v, _) = FR.adam_step(w, grads[t - 1], m, v, b1, b2, eps, wd, step_size, bc2, 1.0)
        assert float((w - p.detach()).abs().max()) <= 4 * 2.0 ** -24 * step_size * t * float((m.abs() / (v.sqrt() / bc2 + eps)).max())
        assert close(m, opt.state[p]['exp_avg']) and close(v, opt.state[p]['exp_avg_sq'])
        assert bool((S >= w.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('momentum', [0.0, 0.875])
@pytest.mark.parametrize('wd', [0.0, 2.0 ** -10])
def test_rmsprop_model_is_torch_rmsprop(momentum, wd):
    lr, alpha, eps, wd, momentum = exact32(2.0 ** -7, 0.96875, 2.0 ** -20, wd, momentum)
    w0, grads = opt_case(80)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.RMSprop([p], lr=lr, alpha=alpha, eps=eps, weight_decay=wd, momentum=momentum, foreach=False)
    w, sq, buf = w0.clone(), torch.zeros(N_OPT, dtype=F64), (torch.zeros(N_OPT, dtype=F64) if momentum else None)
    for t in range(STEPS):
        p.grad = grads[t].clone()
        opt.step()
        (w, S), (sq, _), nb = FR.rmsprop_step(w, grads[t], sq, buf, lr, alpha, eps, wd, momentum, 1.0)
        assert close(w, p.detach()) and close(sq, opt.state[p]['square_avg'])
        assert bool((S >= w.abs() * (1 - 1e-12)).all())
        if momentum:
            buf = nb[0]
            assert close(buf, opt.state[p]['momentum_buffer'])
        else:
            assert nb is None


def test_the_fp32_restatements_follow_their_models():
    """adam_step_f32 / rmsprop_step_f32 are the same update as the fp64 models, to fp32 accuracy (a guard against a typo in the
    restatement: the measurement they serve is of bits)."""
    g = torch.Generator().manual_seed(90)
    w, gr = torch.randn(N_OPT, generator=g), torch.randn(N_OPT, generator=g)
    m, v = torch.randn(N_OPT, generator=g) * 0.1, torch.rand(N_OPT, generator=g) + 0.1
    args = (0.9, 0.999, 1e-8, 1e-4, 1e-2, 0.0316, 0.5)
    (rw, Sw), (rm_, Sm), (rv_, Sv) = FR.adam_step(w, gr, m, v, *args)
    gw, gm, gv = FR.adam_step_f32(w.numpy(), gr.numpy(), m.numpy(), v.numpy(), *args)
    assert gw.dtype == gm.dtype == gv.dtype == np.float32
    for got, ref, S, k in ((gw, rw, Sw, 15), (gm, rm_, Sm, 5), (gv, rv_, Sv, 7)):
        assert bool(((torch.from_numpy(got).double() - ref).abs() <= (k + 1) * 2.0 ** -24 * S).all())
    for mom in (0.0, 0.9):
        buf = m if mom else None
        args = (1e-2, 0.99, 1e-8, 1e-4, mom, 0.5)
        (rw, Sw), (rv_, Sv), rb = FR.rmsprop_step(w, gr, v, buf, *args)
        gw, gv, gb = FR.rmsprop_step_f32(w.numpy(), gr.numpy(), v.numpy(), None if buf is None else buf.numpy(), *args)
        assert bool(((torch.from_numpy(gw).double() - rw).abs() <= 13 * 2.0 ** -24 * Sw).all())
        assert bool(((torch.from_numpy(gv).double() - rv_).abs() <= 8 * 2.0 ** -24 * Sv).all())
        assert (gb is None) == (rb is None)
        if rb is not None:
            assert bool(((torch.from_numpy(gb).double() - rb[0]).abs() <= 11 * 2.0 ** -24 * rb[1]).all())
