"""numpy float64 restatement of the cross-entropy / focal term (include/dfl_hip.h, "Cross-entropy and focal term"):

    s' = min(max(s, EPS), 1),  EPS = 2^-100
    f  = -w t (1 - s')^gamma log s'                       (0^0 = 1)
    L  = (1 / N) sum f over b, c, p,   N = B h w          (pixels, not elements)
    d(lambda L) / ds = -(lambda / N) w t [(1 - s')^gamma / s' - gamma (1 - s')^(gamma-1) log s']

The gradient below EPS is the formula at s' (not zero).  An element with w t == 0 contributes exactly +0 to the value and
has the gradient +0.0; no logarithm is evaluated for it.
"""
import numpy as np

EPS = 2.0 ** -100


def _weights(shape, class_weights):
    C = shape[1]
    w = np.ones(C) if class_weights is None else np.asarray(class_weights, dtype=np.float64)
    assert w.shape == (C,) and (w >= 0).all() and np.isfinite(w).all()
    return w.reshape(1, C, 1, 1)


def _check_gamma(gamma):
    assert gamma == 0 or 1 <= gamma <= 8, gamma


def count(shape):
    """N: the pixels of the batch."""
    return shape[0] * shape[2] * shape[3]


def elements(seg, target, class_weights=None, gamma=0.0):
    """f per element, float64 [B, C, h, w]; +0.0 where w t == 0."""
    _check_gamma(gamma)
    s = np.minimum(np.maximum(np.asarray(seg, dtype=np.float64), EPS), 1.0)
    wt = _weights(seg.shape, class_weights) * np.asarray(target, dtype=np.float64)
    live = wt != 0
    out = np.zeros(s.shape)
    sl = s[live]
    focus = np.ones(sl.shape) if gamma == 0 else (1.0 - sl) ** gamma        # numpy: 0.0 ** 0.0 = 1, and gamma = 0 asks no power
    out[live] = wt[live] * focus * -np.log(sl)
    out[out == 0] = 0.0                                                      # (-0.0 at s' = 1 -> +0.0)
    return out


def value(seg, target, class_weights=None, gamma=0.0):
    """L_CE in float64."""
    return float(elements(seg, target, class_weights, gamma).sum() / count(seg.shape))


def grad(seg, target, class_weights=None, gamma=0.0, lam=1.0, grad_scale=1.0):
    """d(grad_scale lam L_CE) / d seg, float64 [B, C, h, w]; +0.0 where w t == 0."""
    _check_gamma(gamma)
    s = np.minimum(np.maximum(np.asarray(seg, dtype=np.float64), EPS), 1.0)
    wt = _weights(seg.shape, class_weights) * np.asarray(target, dtype=np.float64)
    live = wt != 0
    out = np.zeros(s.shape)
    sl = s[live]
    if gamma == 0:
        bracket = 1.0 / sl
    else:
        bracket = (1.0 - sl) ** gamma / sl - gamma * (1.0 - sl) ** (gamma - 1.0) * np.log(sl)
    out[live] = -(grad_scale * lam / count(seg.shape)) * wt[live] * bracket
    out[out == 0] = 0.0
    return out


def softmax_noise(shape, seed, scale=3.0):
    """The fp32 soft-max over the channels of scale * N(0, 1) noise."""
    rng = np.random.default_rng(seed)
    x = scale * rng.normal(size=shape)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def one_hot_labels(shape, seed):
    """(labels [B, h, w] int64, one-hot fp32 [B, C, h, w]) from seeded labels."""
    B, C, h, w = shape
    g = np.random.default_rng(seed).integers(0, C, size=(B, h, w))
    t = np.zeros(shape, dtype=np.float32)
    np.put_along_axis(t, g[:, None], 1.0, axis=1)
    return g, t
