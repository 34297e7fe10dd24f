"""fp64 models of the seven streaming NHWC operations of include/dfl_hip.h: dfl_upsample2x_fwd / _bwd, dfl_maxpool2x2_fwd / _bwd,
dfl_affine_copy, dfl_bn_relu_bwd_apply and dfl_colstats.

Written from the contracts of the header, in plain torch on float64 NHWC tensors ([N, H, W, C], or rows [M, C]); pixel strides and
channel offsets are the caller's business (it passes views).  Every function returns, next to its result, S: for each output
element the sum of the absolute values of the terms that were added up to give it.  A floating-point evaluation of the same
expression with k operations on its longest path is within about k * u * S of the model, whatever the order of the operations
(tests/test_gpu_streaming.py takes its bounds from that).  tests/test_stream_ref_cpu.py holds the models against torch."""
import torch

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------- bilinear x2
def up_taps(n):
    """The two source indices and weights of each of the 2n outputs along one axis, align_corners=False: the source coordinate
    of output o is (o + 0.5) / 2 - 0.5, clamped at 0; the upper neighbour is clamped at n - 1."""
    o = torch.arange(2 * n, dtype=F64)
    s = ((o + 0.5) / 2 - 0.5).clamp_min(0.0)
    i0 = s.floor().long()
    i1 = (i0 + 1).clamp_max(n - 1)
    w1 = s - i0.to(F64)
    return i0, i1, 1.0 - w1, w1


def upsample2x_fwd(x):
    """y[N, 2H, 2W, C] = up(x[N, H, W, C]): every output gathers its (up to) four sources.  Returns (y, S)."""
    x = x.to(F64)
    y0, y1, wy0, wy1 = up_taps(x.shape[1])
    x0, x1, wx0, wx1 = up_taps(x.shape[2])

    def run(v):
        def along_w(rows):
            return rows[:, :, x0] * wx0[None, None, :, None] + rows[:, :, x1] * wx1[None, None, :, None]
        return along_w(v[:, y0]) * wy0[None, :, None, None] + along_w(v[:, y1]) * wy1[None, :, None, None]
    return run(x), run(x.abs())      # the weights are >= 0: the same map of |x| is the sum of the |terms|


def upsample2x_bwd(y, x_old=None, accumulate=False):
    """x[N, H, W, C] (+)= up^T(y[N, 2H, 2W, C]): every element of y is scattered to its sources with the weights the forward
    definition gives it -- the transpose by construction, not a gather with weights worked out by hand.  Returns (x, S)."""
    y = y.to(F64)
    N, Ho, Wo, C = y.shape
    H, W = Ho // 2, Wo // 2
    y0, y1, wy0, wy1 = up_taps(H)
    x0, x1, wx0, wx1 = up_taps(W)

    def run(v):
        t = torch.zeros(N, Ho, W, C, dtype=F64)
        t.index_add_(2, x0, v * wx0[None, None, :, None])
        t.index_add_(2, x1, v * wx1[None, None, :, None])
        out = torch.zeros(N, H, W, C, dtype=F64)
        out.index_add_(1, y0, t * wy0[None, :, None, None])
        out.index_add_(1, y1, t * wy1[None, :, None, None])
        return out
    g, S = run(y), run(y.abs())
    if accumulate:
        x_old = x_old.to(F64)
        g, S = g + x_old, S + x_old.abs()
    return g, S


# ---------------------------------------------------------------------------------------------------- 2x2 max-pool
def _windows(x):
    """[N, H, W, C] -> [N, H//2, W//2, 4, C]: the four inputs of each output in scan order (0,0) (0,1) (1,0) (1,1); an odd
    last row / column belongs to no window."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Ho, Wo, 4, C)


def _unwindows(v):
    N, Ho, Wo, _, C = v.shape
    return v.reshape(N, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)


def maxpool2x2_fwd(x):
    """y[N, H//2, W//2, C] = the maximum of each 2 x 2 window.  Returns (y, S)."""
    y = _windows(x.to(F64)).max(dim=3).values
    return y, y.abs()


def maxpool2x2_bwd(x, dy, dx_old):
    """dx = dx_old + dy at the FIRST maximum in scan order of each window of x (added, not stored).  Returns (dx, S, k): k is
    the index 0..3 of the winner of every window."""
    v = _windows(x.to(F64))
    eq = v == v.max(dim=3, keepdim=True).values
    first = eq & (eq.cumsum(3) == 1)                       # the first of the maxima in scan order
    k = (first.long() * torch.arange(4)[None, None, None, :, None]).sum(3)
    g = _unwindows(first.to(F64) * dy.to(F64)[:, :, :, None, :])
    dx = dx_old.to(F64).clone()
    S = dx.abs()
    Hg, Wg = g.shape[1], g.shape[2]
    dx[:, :Hg, :Wg] += g
    S[:, :Hg, :Wg] += g.abs()
    return dx, S, k


# ---------------------------------------------------------------------------------------------------- affine copy
def affine_copy(x, y, H, W, xoy, xox, yoy, yox, scale=None, shift=None, accumulate=False):
    """The H x W window of y[N, yH, yW, C] at (yoy, yox) = the window of x[N, xH, xW, C] at (xoy, xox), * scale + shift per channel
    when scale is given, + the window's old contents when accumulate.  Returns (y_new, S), both of y's shape; outside the
    window y_new is y and S is 0."""
    x, out = x.to(F64), y.to(F64).clone()
    v = x[:, xoy:xoy + H, xox:xox + W]
    S = v.abs()
    if scale is not None:
        scale, shift = scale.to(F64), shift.to(F64)
        S = (v * scale).abs() + shift.abs()
        v = v * scale + shift
    if accumulate:
        old = out[:, yoy:yoy + H, yox:yox + W]
        v, S = v + old, S + old.abs()
    out[:, yoy:yoy + H, yox:yox + W] = v
    Sf = torch.zeros_like(out)
    Sf[:, yoy:yoy + H, yox:yox + W] = S
    return out, Sf


# ---------------------------------------------------------------------------------------------------- row kernels
def bn_relu_bwd(dy, r, coef=None):
    """dpre[M, C] = where(r > 0, A * dy + B * r + C, 0) with (A, B, C) = coef[0..2] per channel, a strict >; coef None is the
    plain ReLU backward where(r > 0, dy, 0).  Returns (dpre, S)."""
    dy, r = dy.to(F64), r.to(F64)
    if coef is None:
        v, S = dy, dy.abs()
    else:
        coef = coef.to(F64)
        v = coef[0] * dy + coef[1] * r + coef[2]
        S = (coef[0] * dy).abs() + (coef[1] * r).abs() + coef[2].abs().expand_as(dy)
    on = r > 0
    zero = torch.zeros((), dtype=F64)
    return torch.where(on, v, zero), torch.where(on, S, zero)


def colsum(v):
    """Column sums of rows [M, C].  Returns (sums[C], S[C])."""
    v = v.to(F64)
    return v.sum(0), v.abs().sum(0)


def colstats(a, b=None):
    """sums[0][c] = sum over the rows of a, sums[1][c] = sum of a * b (b None: a * a).  Returns (sums[2, C], S[2, C])."""
    a = a.to(F64)
    p = a * (a if b is None else b.to(F64))
    return torch.stack([a.sum(0), p.sum(0)]), torch.stack([a.abs().sum(0), p.abs().sum(0)])
