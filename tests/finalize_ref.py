"""fp64 models of the kernels that finish every sum of a training step and apply every update (include/dfl_hip.h):
dfl_reduce_batch / dfl_reduce_partials / dfl_sum_partials, dfl_bn_finalize / dfl_bn_bwd_finalize and their _live forms,
dfl_bn_eval_prepare, and the update rules of dfl_sgd_step / dfl_adam_step / dfl_rmsprop_step.

Written from the contracts of the header, in plain torch on float64 tensors.  As in tests/stream_ref.py every function returns,
next to each result, S: per output element the sum of the absolute values of the terms of its expression.  An evaluation of the
same expression with k roundings on its longest path is within about k * u * S of the model (tests/test_gpu_finalize.py takes
its bounds from that).  Where an expression divides by, or takes the root of, a sum (the optimizers), S carries the factor
S_sum / |sum| >= 1 by which a relative error of that sum can exceed its roundings; the counts of k are written in the test file.
Hyper-parameters are taken as the kernels see them: f32() of what the C ABI passes as float.  tests/test_finalize_ref_cpu.py
holds the models against torch's own float64 operators and optimizers."""
import numpy as np
import torch

F64 = torch.float64


def f32(x):
    """The double that a C float argument holds."""
    return float(np.float32(x))


def exact_data(g, *shape):
    """Integers times 2^-10 with |integer| < 2^20: each an exact fp32, and every partial sum of at most 2^14 of them an exact
    fp64 in any order (|sum| < 2^34 integers, 34 + 10 < 53 bits).  Returns float64."""
    return torch.randint(-(2 ** 20) + 1, 2 ** 20, shape, generator=g).to(F64) * 2.0 ** -10


def quantize(v):
    """The nearest integer multiple of 2^-10 (the values must stay below 2^10)."""
    q = torch.round(v.to(F64) * 2.0 ** 10)
    assert float(q.abs().max()) < 2 ** 20
    return q * 2.0 ** -10


# ---------------------------------------------------------------------------------------------------- sums
def transpose_index(n, T):
    """Where element i of a tap-major slice [T][n/T] lands in [n/T][T]: i' = (i % (n/T)) * T + i / (n/T); the identity for T <= 1."""
    i = torch.arange(n)
    if T <= 1:
        return i
    R = n // T
    return (i % R) * T + i // R


def reduce_slices(src, T=1):
    """src [count][n] -> dst[i'] = sum_k src[k][i] with the T-transposition of the header.  Returns (dst[n], S[n])."""
    src = src.to(F64)
    n = src.shape[1]
    idx = transpose_index(n, T)
    dst, S = torch.empty(n, dtype=F64), torch.empty(n, dtype=F64)
    dst[idx] = src.sum(0)
    S[idx] = src.abs().sum(0)
    return dst, S


# ---------------------------------------------------------------------------------------------------- BatchNorm finalize
def bn_finalize(s1, s2, gamma, beta, count, eps, momentum=0.0, running_mean=None, running_var=None):
    """From the channel totals s1 = sum x, s2 = sum x^2 over `count` elements: mean, the biased variance clamped at 0, invstd,
    scale = gamma * invstd, shift = beta - mean * scale, and nn.BatchNorm2d's running update with the unbiased variance
    (count == 1: the biased one).  Returns {name: (ref, S)}."""
    s1, s2, gamma, beta = s1.to(F64), s2.to(F64), gamma.to(F64), beta.to(F64)
    cnt, eps, mom = float(count), f32(eps), f32(momentum)
    mean = s1 / cnt
    var = (s2 / cnt - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    out = {'scale': (scale, scale.abs()), 'shift': (beta - mean * scale, beta.abs() + (mean * scale).abs()),
           'save_mean': (mean, mean.abs()), 'save_invstd': (invstd, invstd.abs()), 'var': (var, s2 / cnt + mean * mean)}
    if running_mean is not None:
        rm, rv = running_mean.to(F64), running_var.to(F64)
        unbiased = var * cnt / (cnt - 1.0) if cnt > 1.0 else var
        out['running_mean'] = ((1.0 - mom) * rm + mom * mean, ((1.0 - mom) * rm).abs() + (mom * mean).abs())
        out['running_var'] = ((1.0 - mom) * rv + mom * unbiased, ((1.0 - mom) * rv).abs() + (mom * unbiased).abs())
    return out


def bn_bwd_finalize(sdy, sdyr, gamma, save_mean, save_invstd, count):
    """From the totals of (dy, dy * r): dgamma = invstd * (sum dy r - mean sum dy), dbeta = sum dy, and the rows A, B, C of
    d(pre-activation) = [r > 0] (A dy + B r + C), i.e. dr = s (dy - c1 - xhat c2) with s = gamma invstd, xhat = (r - mean) invstd,
    c1 = sum dy / count, c2 = dgamma / count; count == 0 (eval mode): A = s, B = C = 0.  Returns {name: (ref, S)}."""
    sdy, sdyr, g, mean, invstd = (t.to(F64) for t in (sdy, sdyr, gamma, save_mean, save_invstd))
    dgamma = invstd * (sdyr - mean * sdy)
    Sdg = invstd.abs() * (sdyr.abs() + (mean * sdy).abs())
    s = g * invstd
    zero = torch.zeros_like(s)
    if count > 0:
        c1, c2, Sc2 = sdy / count, dgamma / count, Sdg / count
    else:
        c1, c2, Sc2 = zero, zero, zero
    A, B, Cc = s, -s * c2 * invstd, -s * c1 + s * c2 * invstd * mean
    SB = (s * invstd).abs() * Sc2
    return {'dgamma': (dgamma, Sdg), 'dbeta': (sdy, sdy.abs()),
            'coef': (torch.stack([A, B, Cc]), torch.stack([A.abs(), SB, (s * c1).abs() + SB * mean.abs()]))}


def bn_eval(gamma, beta, running_mean, running_var, eps):
    """scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale.  Returns ((scale, S), (shift, S))."""
    gamma, beta, rm, rv = (t.to(F64) for t in (gamma, beta, running_mean, running_var))
    scale = gamma / torch.sqrt(rv + f32(eps))
    return (scale, scale.abs()), (beta - rm * scale, beta.abs() + (rm * scale).abs())


# ---------------------------------------------------------------------------------------------------- optimizers
def _grad(w, grad, wd, gscale):
    a, b = grad * f32(gscale), f32(wd) * w
    return a + b, a.abs() + b.abs()


def sgd_step(w, grad, buf, lr, momentum, wd, gscale, nesterov, first):
    """torch.optim.SGD: g = grad gscale + wd w; buf = first ? g : mom buf + g; g = nesterov ? g + mom buf : buf; w -= lr g.
    buf is None without momentum.  Returns ((w, S), (buf, S) or None)."""
    w, grad = w.to(F64), grad.to(F64)
    lr, mom = f32(lr), f32(momentum)
    g, Sg = _grad(w, grad, wd, gscale)
    nb = None
    if mom != 0.0:
        if first:
            nb, Snb = g, Sg
        else:
            buf = buf.to(F64)
            nb, Snb = mom * buf + g, (mom * buf).abs() + Sg
        if nesterov:
            g, Sg = g + mom * nb, Sg + mom * Snb
        else:
            g, Sg = nb, Snb
        nb = (nb, Snb)
    return (w - lr * g, w.abs() + lr * Sg), nb


def adam_step(w, grad, m, v, beta1, beta2, eps, wd, step_size, bc2_sqrt, gscale):
    """torch.optim.Adam (coupled weight decay, no amsgrad), step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) given:
    m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g g; w -= step_size m / (sqrt(v) / bc2_sqrt + eps).  The factors
    1 - beta are formed in double and rounded to fp32, as the entry points do.  Returns ((w, S), (m, S), (v, S))."""
    w, grad, m, v = (t.to(F64) for t in (w, grad, m, v))
    w1, omb2, b2 = f32(1.0 - beta1), f32(1.0 - beta2), f32(beta2)
    g, Sg = _grad(w, grad, wd, gscale)
    m2, Sm = m + w1 * (g - m), m.abs() + w1 * (Sg + m.abs())
    v2, Sv = b2 * v + omb2 * g * g, b2 * v.abs() + omb2 * Sg * Sg
    den = torch.sqrt(v2) / f32(bc2_sqrt) + f32(eps)
    q, Sq = m2 / den, Sm / den * (Sv / v2)
    return (w - f32(step_size) * q, w.abs() + f32(step_size) * Sq), (m2, Sm), (v2, Sv)


def rmsprop_step(w, grad, sq, buf, lr, alpha, eps, wd, momentum, gscale):
    """torch.optim.RMSprop (not centered): v = alpha v + (1 - alpha) g g; avg = sqrt(v) + eps; momentum > 0: buf = momentum buf
    + g / avg, w -= lr buf; momentum == 0 (buf None): w -= lr g / avg.  Returns ((w, S), (v, S), (buf, S) or None)."""
    w, grad, sq = w.to(F64), grad.to(F64), sq.to(F64)
    lr, mom, al, oma = f32(lr), f32(momentum), f32(alpha), f32(1.0 - alpha)
    g, Sg = _grad(w, grad, wd, gscale)
    v2, Sv = al * sq + oma * g * g, al * sq.abs() + oma * Sg * Sg
    avg = torch.sqrt(v2) + f32(eps)
    r, Sr = g / avg, Sg / avg * (Sv / v2)
    if mom != 0.0:
        buf = buf.to(F64)
        b2, Sb = mom * buf + r, (mom * buf).abs() + Sr
        return (w - lr * b2, w.abs() + lr * Sb), (v2, Sv), (b2, Sb)
    return (w - lr * r, w.abs() + lr * Sr), (v2, Sv), None


# ---------------------------------------------------------------------------------------------------- fp32, one op at a time
def adam_step_f32(w, grad, m, v, beta1, beta2, eps, wd, step_size, bc2_sqrt, gscale):
    """The arithmetic the comment above AdamRule (csrc/bn_elem.hip) claims -- torch's foreach ops one at a time, each result
    rounded to fp32 -- restated in numpy float32 (whose +, *, /, sqrt are correctly rounded).  A measurement, not a model."""
    f = np.float32
    w, grad, m, v = (np.asarray(t, dtype=f) for t in (w, grad, m, v))
    w1, omb2 = f(1.0 - beta1), f(1.0 - beta2)
    g = grad * f(gscale) + f(wd) * w
    d = g - m
    m2 = m + w1 * d if abs(w1) < 0.5 else g - d * (f(1.0) - w1)
    v2 = v * f(beta2) + (omb2 * g) * g
    den = np.sqrt(v2) / f(bc2_sqrt) + f(eps)
    return w - f(step_size) * (m2 / den), m2, v2


def rmsprop_step_f32(w, grad, sq, buf, lr, alpha, eps, wd, momentum, gscale):
    """RmspropRule's claim, as adam_step_f32."""
    f = np.float32
    w, grad, sq = (np.asarray(t, dtype=f) for t in (w, grad, sq))
    g = grad * f(gscale) + f(wd) * w
    v2 = sq * f(alpha) + (f(1.0 - alpha) * g) * g
    avg = np.sqrt(v2) + f(eps)
    if momentum != 0.0:
        b2 = np.asarray(buf, dtype=f) * f(momentum) + g / avg
        return w + -f(lr) * b2, v2, b2
    return w + -f(lr) * (g / avg), v2, None
