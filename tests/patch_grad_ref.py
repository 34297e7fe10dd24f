"""The numpy restatement of the weighted patch gradient-NCC and of the patch adjoint: what the GPU
tests compare dfl_sim_patch_weights and dfl_sim_patch_eval (csrc/sim_patch.hip) against.  Gradients, counted pixels and
the variance rule are tests/reg_ref.py's (section 16), the patch grid, min_count, "lives" and "counts in x / in y" are
tests/patch_ref.py's (section 18); this file adds the weights, the weighted cost and the adjoint of either weighting.

dtype=np.float64 is the reference.  dtype=np.float32 takes the Sobel values in float32, rounds the eight coefficients of
a patch to float32 and adds a pixel's patches in float32, as the kernel does (all sums over pixels and patches that the
kernel takes in float64 are float64 here too); tests/patch_grad_floor.py compares the two.
"""
import numpy as np

import patch_ref as PT
import reg_ref as R

WEIGHTS = ('uniform', 'variance')
PARAMS = PT.PARAMS + ((1, 4),)                               # ... and a stride larger than the side: some pixels lie in no patch


def cases():
    """Every (H, W, rho, stride) of the kernel tests: patch_ref.SIZES times PARAMS, wherever the patch fits."""
    return [(H, W, rho, s) for H, W in PT.SIZES for rho, s in PARAMS if PT.fits(H, W, rho)]


def textured(fixed):
    """The fixed image plus a texture of 1 % of its maximum, which no rendered view holds: every background patch of the
    result counts, as every patch of a preprocessed projection does."""
    f = np.asarray(fixed, np.float64)
    r, c = np.meshgrid(np.arange(f.shape[0], dtype=np.float64), np.arange(f.shape[1], dtype=np.float64), indexing='ij')
    return f + 0.01 * f.max() * np.sin(0.9 * r + np.mod(0.37 * c * c, 7.0)) * np.cos(1.7 * c - 0.3 * r)


def _where(H, W, rho, stride):
    return list(PT._patches(H, W, rho, stride))


def weights(fixed, mask, rho, stride, min_count=None, dtype=np.float64):
    """(w [P, 2], wsum [2]) float64: w_x[p] = sum (fx - mean fx)^2 over the counted pixels of a patch that counts in x, else
    0, w_y likewise, in row-major (a, b) order; wsum = their sums over the patches."""
    H, W = fixed.shape
    on = R.counted(H, W, mask)
    _, flags, _ = PT.fixed_patches(fixed, mask, rho, stride, min_count, dtype)
    g = [v.astype(np.float64) for v in R.sobel(fixed, dtype)]
    w = np.zeros((flags.size, 2))
    for p, (rs, cs) in enumerate(_where(H, W, rho, stride)):
        sel = on[rs, cs]
        for d in range(2):
            if flags[p] >> d & 1:
                x = g[d][rs, cs][sel]
                w[p, d] = float(((x - x.mean()) ** 2).sum())
    return w, w.sum(0)


def shares(fixed, mask, rho, stride, min_count=None, dtype=np.float64, weight='variance'):
    """c [P, 2]: a patch's share of the cost in x and in y -- w / wsum, or 1 / (how many count) on the patches that count,
    0 elsewhere and where nothing counts."""
    if weight not in WEIGHTS:
        raise ValueError(weight)
    if weight == 'variance':
        w, tot = weights(fixed, mask, rho, stride, min_count, dtype)
    else:
        _, flags, _ = PT.fixed_patches(fixed, mask, rho, stride, min_count, dtype)
        w = np.stack([(flags & 1).astype(np.float64), (flags >> 1 & 1).astype(np.float64)], 1)
        tot = w.sum(0)
    return np.where(tot > 0, w / np.where(tot > 0, tot, 1.0), 0.0)


def patch_terms(moving, fixed, mask, rho, stride, min_count=None, dtype=np.float64):
    """(ncc [V, P, 2], coef [V, P, 2, 4] = alpha, beta, mean a, mean b; ratio [V, P, 2]) in float64 for the patches that
    count (0 elsewhere): the per-patch ncc of section 18, section 19's two factors of its derivative (both 0 when the
    forward rule makes the ncc 0) and the variance ratio of the moving Sobel values that decided it."""
    mv = np.asarray(moving)
    H, W = fixed.shape
    on = R.counted(H, W, mask)
    _, flags, _ = PT.fixed_patches(fixed, mask, rho, stride, min_count, dtype)
    fg = [v.astype(np.float64) for v in R.sobel(fixed, dtype)]
    where = _where(H, W, rho, stride)
    V, P = mv.shape[0], flags.size
    ncc, coef, ratio = np.zeros((V, P, 2)), np.zeros((V, P, 2, 4)), np.zeros((V, P, 2))
    sob = [R.sobel(mv[v], dtype) for v in range(V)]
    mg = [np.stack([s[d] for s in sob]).astype(np.float64) for d in range(2)]            # [V, H - 2, W - 2], all views at once
    for p, (rs, cs) in enumerate(where):
        if flags[p] == 0:
            continue
        sel = on[rs, cs]
        for d in range(2):
            if not flags[p] >> d & 1:
                continue
            a, b = mg[d][:, rs, cs][:, sel], fg[d][rs, cs][sel]                          # [V, n], [n]
            ma, mb = a.mean(1), b.mean()
            da, db = a - ma[:, None], b - mb
            va, vb, saa = (da * da).sum(1), float(db @ db), (a * a).sum(1)
            ratio[:, p, d] = np.where(saa > 0, va / np.where(saa > 0, saa, 1.0), 0.0)
            live = (va > R.VAR_EPS * saa) & (vb > R.VAR_EPS * float(b @ b))
            root, cab = np.sqrt(np.where(live, va, 1.0) * vb), da @ db
            ncc[:, p, d] = np.where(live, cab / root, 0.0)
            coef[:, p, d, 0] = np.where(live, -0.5 / root, 0.0)
            coef[:, p, d, 1] = np.where(live, 0.5 * cab / (np.where(live, va, 1.0) * root), 0.0)
            coef[:, p, d, 2] = np.where(live, ma, 0.0)
            coef[:, p, d, 3] = np.where(live, mb, 0.0)
    return ncc, coef, ratio


def cost(moving, fixed, mask=None, rho=7, stride=4, min_count=None, dtype=np.float64, weight='variance'):
    """[V] float64 (or a scalar for one [H, W] image): 1 - (X + Y) / 2 with X = sum_p c_x[p] ncc_x[p], Y likewise."""
    moving = np.asarray(moving)
    mv = moving[None] if moving.ndim == 2 else moving
    ncc, _, _ = patch_terms(mv, fixed, mask, rho, stride, min_count, dtype)
    c = shares(fixed, mask, rho, stride, min_count, dtype, weight)
    out = 1.0 - 0.5 * (ncc * c[None]).sum((1, 2))
    return out[0] if moving.ndim == 2 else out


def adjoint(moving, fixed, mask=None, rho=7, stride=4, min_count=None, dtype=np.float64, weight='variance', terms=None):
    """(cost [V] float64, d_moving [V, H, W] of `dtype`) of moving [V, H, W] (or [H, W]: no view axis) against fixed:
    d_moving[v] = d cost[v] / d moving[v] = Sobel^T (g_x, g_y), g_d(q) = the sum over the patches that hold the counted
    pixel q, in ascending (a, b) order, of c alpha (b_q - mean b) + c beta (a_q - mean a).  terms: patch_terms' result
    for the same arguments, where the caller has it."""
    moving = np.asarray(moving)
    mv = moving[None] if moving.ndim == 2 else moving
    H, W = fixed.shape
    on = R.counted(H, W, mask)
    ncc, coef, _ = patch_terms(mv, fixed, mask, rho, stride, min_count, dtype) if terms is None else terms
    c = shares(fixed, mask, rho, stride, min_count, dtype, weight)
    costs = 1.0 - 0.5 * (ncc * c[None]).sum((1, 2))
    fg = R.sobel(fixed, dtype)
    where = _where(H, W, rho, stride)
    V = mv.shape[0]
    out = np.zeros(mv.shape, dtype)
    sob = [R.sobel(mv[v], dtype) for v in range(V)]
    mg = [np.stack([s[d] for s in sob]) for d in range(2)]                               # [V, H - 2, W - 2] of dtype, all views at once
    g = [np.zeros((V, H - 2, W - 2), dtype), np.zeros((V, H - 2, W - 2), dtype)]
    for p, (rs, cs) in enumerate(where):
        sel = on[rs, cs]
        for d in range(2):
            if c[p, d] == 0.0:
                continue
            k = [(c[p, d] * coef[:, p, d, 0]).astype(dtype), (c[p, d] * coef[:, p, d, 1]).astype(dtype),     # formed in float64, rounded once
                 coef[:, p, d, 2].astype(dtype), coef[:, p, d, 3].astype(dtype)]
            ca, cb, ma, mb = (x[:, None, None] for x in k)
            term = ca * (fg[d][rs, cs][None] - mb) + cb * (mg[d][:, rs, cs] - ma)
            g[d][:, rs, cs] += np.where(sel[None], term, dtype(0)).astype(dtype)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            kx, ky = dc * (2 - abs(dr)), dr * (2 - abs(dc))                      # the Sobel weights at offset (dr, dc)
            out[:, 1 + dr:H - 1 + dr, 1 + dc:W - 1 + dc] += dtype(kx) * g[0] + dtype(ky) * g[1]
    return (costs[0], out[0]) if moving.ndim == 2 else (costs, out)


def coverage(H, W, rho, stride):
    """int [H - 2, W - 2]: how many patches hold every interior pixel."""
    n = np.zeros((H - 2, W - 2), np.int64)
    for rs, cs in _where(H, W, rho, stride):
        n[rs, cs] += 1
    return n
