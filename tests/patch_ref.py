"""The numpy restatement of the patch-wise gradient-NCC and of the landmark term: what the GPU
tests compare csrc/sim_patch.hip and dfl_amd.register.landmark_penalty against.  Gradients, counted pixels, the ncc of
two vectors and the "variance is 0" rule are tests/reg_ref.py's (section 16); this file adds the patches.

dtype=np.float64 is the reference; dtype=np.float32 takes the Sobel gradients in float32, as the kernel does (all sums
are float64 in the kernel and in both models); tests/patch_floor.py compares the two.
"""
import numpy as np

import reg_ref as R

SIZES = ((45, 61), (17, 70), (9, 9), (9, 300))
PARAMS = ((3, 2), (2, 5), (1, 1), (7, 8))                    # (radius, stride): overlapping, abutting, every pixel, wide
BAND = (2.0 ** -44, 2.0 ** -36)                              # no live patch may have its fixed-variance ratio in here


def side(rho):
    return 2 * int(rho) + 1


def default_min_count(rho):
    return (side(rho) ** 2 + 1) // 2


def grid(H, W, rho, stride):
    """(PR, PC): patches of side 2 rho + 1 every `stride` interior pixels, wholly inside the (H - 2) x (W - 2) interior."""
    S = side(rho)
    if rho < 1 or stride < 1 or H - 2 < S or W - 2 < S:
        raise ValueError('no patch of radius %d and stride %d in %d x %d' % (rho, stride, H, W))
    return (H - 2 - S) // stride + 1, (W - 2 - S) // stride + 1


def fits(H, W, rho):
    return H - 2 >= side(rho) and W - 2 >= side(rho)


def cases():
    """Every (H, W, rho, stride) of the kernel tests: the sizes times the parameters, wherever the patch fits."""
    return [(H, W, rho, s) for H, W in SIZES for rho, s in PARAMS if fits(H, W, rho)]


def _patches(H, W, rho, stride):
    S = side(rho)
    PR, PC = grid(H, W, rho, stride)
    for a in range(PR):
        for b in range(PC):
            yield slice(a * stride, a * stride + S), slice(b * stride, b * stride + S)


def variance_ratio(v):
    """sum (v - mean)^2 / sum v^2 of a float64 vector (two passes); 0 for an empty or an all-zero one."""
    if v.size == 0:
        return 0.0
    d = v - v.mean()
    ss = float(v @ v)
    return float(d @ d) / ss if ss > 0 else 0.0


def fixed_patches(fixed, mask, rho, stride, min_count=None, dtype=np.float64):
    """(totals [P, 5], flags [P] uint8, ratios [P, 2]) in row-major (a, b) order.  totals: n, sum fx, sum fx^2, sum fy,
    sum fy^2 over the patch's counted pixels; flags: bit 0 = the patch counts in x, bit 1 = in y; ratios: the variance
    ratios of fx and fy that decided it."""
    H, W = fixed.shape
    mc = default_min_count(rho) if min_count is None else int(min_count)
    on = R.counted(H, W, mask)
    gx, gy = (g.astype(np.float64) for g in R.sobel(fixed, dtype))
    totals, flags, ratios = [], [], []
    for rs, cs in _patches(H, W, rho, stride):
        sel = on[rs, cs]
        x, y = gx[rs, cs][sel], gy[rs, cs][sel]
        totals.append([x.size, x.sum(), (x * x).sum(), y.sum(), (y * y).sum()])
        rx, ry = variance_ratio(x), variance_ratio(y)
        live = x.size >= mc
        flags.append((1 if live and rx > R.VAR_EPS else 0) | (2 if live and ry > R.VAR_EPS else 0))
        ratios.append([rx, ry])
    return np.array(totals, np.float64).reshape(-1, 5), np.array(flags, np.uint8), np.array(ratios, np.float64).reshape(-1, 2)


def cost(moving, fixed, mask=None, rho=7, stride=4, min_count=None, dtype=np.float64):
    """[V] float64 (or a scalar for one [H, W] image): 1 - (X + Y) / 2, X the mean of the patches' ncc(gx_v, gx_f) over the
    patches that count in x (0 when none does), Y likewise."""
    moving = np.asarray(moving)
    mv = moving[None] if moving.ndim == 2 else moving
    H, W = fixed.shape
    on = R.counted(H, W, mask)
    _, flags, _ = fixed_patches(fixed, mask, rho, stride, min_count, dtype)
    fx, fy = (g.astype(np.float64) for g in R.sobel(fixed, dtype))
    where = list(_patches(H, W, rho, stride))
    nx, ny = int((flags & 1).sum()), int((flags >> 1 & 1).sum())
    out = np.zeros(mv.shape[0])
    for v in range(mv.shape[0]):
        mx, my = (g.astype(np.float64) for g in R.sobel(mv[v], dtype))
        sx = sy = 0.0
        for f, (rs, cs) in zip(flags, where):
            if f == 0:
                continue
            sel = on[rs, cs]
            if f & 1:
                sx += R.ncc(mx[rs, cs][sel], fx[rs, cs][sel])
            if f & 2:
                sy += R.ncc(my[rs, cs][sel], fy[rs, cs][sel])
        out[v] = 1.0 - 0.5 * ((sx / nx if nx else 0.0) + (sy / ny if ny else 0.0))
    return out[0] if moving.ndim == 2 else out


def landmark_penalty(S, poses, X3d, x2d, weight):
    """weight * mean_l |proj_l - x2d_l|^2 over the finite columns of x2d, for each pelvis pose of poses [n, 4, 4], with
    reg_ref.project (the tilted scene on its full detector grid: G = identity)."""
    x = np.asarray(x2d, np.float64)
    use = np.isfinite(x).all(0)
    out = []
    for P in np.asarray(poses, np.float64).reshape(-1, 4, 4):
        d = R.project(S, P, np.asarray(X3d, np.float64)[use]) - x[:, use]
        out.append(weight * float((d * d).sum(0).mean()))
    return np.array(out)


def with_bar(img):
    """Case D: a foreign structure the CT does not hold -- 0.6 max(img) added where |r - 1.3 c + 40| < 4."""
    rr, cc = np.meshgrid(np.arange(img.shape[0]), np.arange(img.shape[1]), indexing='ij')
    out = np.array(img, np.float64)
    out[np.abs(rr - 1.3 * cc + 40) < 4] += 0.6 * float(img.max())
    return out
