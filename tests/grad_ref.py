"""The numpy restatement of the gradient semantics: the adjoint of the gradient-NCC cost, the
force and moment that a detector-space adjoint exerts on every object of a trilinear DRR with its sampling frozen, and
the chain from those to the six pose parameters of dfl_amd.register.  Built on tests/drr_ref.py (_setup and the
trilinear branch of render) and tests/reg_ref.py (sobel, counted, the variance rule).

dtype=np.float64 is the reference.  dtype=np.float32 takes the per-pixel and the per-ray arithmetic in float32 and the
sums across pixels and rays in float64, as the kernels do -- the sample position o + t d with one rounding, as the
compiled kernels take it; tests/grad_floor.py compares the two.
"""
import numpy as np

import drr_ref as D
import reg_ref as R


# ---- the adjoint of the similarity -------------------------------------------------------------------------------------
def _direction(a, b, on, dtype):
    """g = d(-ncc / 2) / d a on the interior grid (0 where not counted), a and b the Sobel values [H - 2, W - 2]."""
    g = np.zeros(a.shape, dtype)
    a64, b64 = a[on].astype(np.float64), b[on].astype(np.float64)
    if a64.size == 0:
        return g
    ma, mb = a64.mean(), b64.mean()
    da, db = a64 - ma, b64 - mb
    va, vb = float(da @ da), float(db @ db)
    if va <= R.VAR_EPS * float(a64 @ a64) or vb <= R.VAR_EPS * float(b64 @ b64):
        return g
    root = np.sqrt(va * vb)
    alpha, beta = -0.5 / root, 0.5 * float(da @ db) / (va * root)
    g[on] = dtype(alpha) * (b[on] - dtype(mb)) + dtype(beta) * (a[on] - dtype(ma))
    return g


def sim_adjoint(moving, fixed, mask=None, dtype=np.float64):
    """(cost [V] float64, d_moving [V, H, W] of `dtype`) of moving [V, H, W] (or [H, W]: no view axis) against fixed:
    d_moving[v] = d cost[v] / d moving[v], Sobel^T of (g_x, g_y)."""
    moving = np.asarray(moving)
    mv = moving[None] if moving.ndim == 2 else moving
    H, W = fixed.shape
    on = R.counted(H, W, mask)
    fx, fy = R.sobel(fixed, dtype)
    cost = np.atleast_1d(R.cost(mv, fixed, mask, dtype))
    out = np.zeros(mv.shape, dtype)
    for v in range(mv.shape[0]):
        mx, my = R.sobel(mv[v], dtype)
        gx, gy = _direction(mx, fx, on, dtype), _direction(my, fy, on, dtype)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                kx, ky = dc * (2 - abs(dr)), dr * (2 - abs(dc))                  # the Sobel weights at offset (dr, dc)
                out[v, 1 + dr:H - 1 + dr, 1 + dc:W - 1 + dc] += dtype(kx) * gx + dtype(ky) * gy
    return (cost[0], out[0]) if moving.ndim == 2 else (cost, out)


# ---- force and moment on every object ----------------------------------------------------------------------------------
def box_pivots(recs):
    """[n_obj, 3]: the middle of every record's box in index coordinates (0 for an empty box), rounded to float32."""
    lo, hi = recs['box_lo'].astype(np.float64), recs['box_hi'].astype(np.float64)
    return np.where((hi < lo).any(-1, keepdims=True), 0.0, (lo + hi) / 2).astype(np.float32)


def pose_moments(mu, lab, recs, qscale, H, W, d_att, pivots, step_mm=1.0, dtype=np.float64):
    """float64 [n_obj, 12]: F[3], then Mom[3][3] row-major, of every object of one view (recs [n_obj]) under the adjoint
    d_att [H, W] about pivots [n_obj, 3]: the samples, corners and ray weights of drr_ref.render(interp='trilinear')."""
    dt = dtype
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    c, r = cc.reshape(-1).astype(dt), rr.reshape(-1).astype(dt)
    q = np.asarray(qscale, np.float32).reshape(-1).astype(dt)
    qv = [D._dot(q[3 * a:3 * a + 3], c, r) for a in range(3)]
    s = np.sqrt(qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2])
    mu = mu.astype(dt)
    da = np.asarray(d_att).reshape(-1).astype(dt)
    nz, ny, nx = lab.shape
    half = dt(0.5)
    out = np.zeros((len(recs), 12))
    for n, rec in enumerate(recs):
        if (rec['box_hi'] < rec['box_lo']).any():
            continue
        o, d, t0, t1, ok = D._setup(rec, c, r, dt)
        adm = D._admit(rec['mask'])
        span = np.where(ok, t1 - t0, 0).astype(dt)
        nf = np.maximum(dt(1), np.ceil(s * span / dt(step_mm))).astype(dt)
        N = np.where(ok, nf, 0).astype(np.int64)
        k = np.arange(max(int(N.max()), 1)).astype(dt)
        live = k[None, :] < N[:, None]
        t = (np.where(ok, t0, 0).astype(dt)[:, None] + (k[None, :] + half) * (span / nf)[:, None]).astype(dt)
        t = np.where(live, t, 0).astype(dt)
        p, i0, i1, w = [], [], [], []
        for a, size in enumerate((nx, ny, nz)):
            # one rounding, as the compiler contracts o + t d to a fused multiply-add in the renderer and in the gradient
            # kernel alike (the product of two float32 is exact in float64).  Where a sample lies within float32 rounding of
            # a cell face the two roundings pick different cells, and grad f -- unlike f -- jumps across a face
            p.append((o[a].astype(np.float64) + t.astype(np.float64) * d[a][:, None].astype(np.float64)).astype(dt))
            f = np.floor(p[a])
            w.append((p[a] - f).astype(dt))
            i0.append(np.clip(f.astype(np.int64), 0, size - 1))
            i1.append(np.clip(f.astype(np.int64) + 1, 0, size - 1))

        def v(x, y, z):
            return np.where(adm[lab[z, y, x]], mu[z, y, x], 0).astype(dt)

        v000, v100 = v(i0[0], i0[1], i0[2]), v(i1[0], i0[1], i0[2])
        v010, v110 = v(i0[0], i1[1], i0[2]), v(i1[0], i1[1], i0[2])
        v001, v101 = v(i0[0], i0[1], i1[2]), v(i1[0], i0[1], i1[2])
        v011, v111 = v(i0[0], i1[1], i1[2]), v(i1[0], i1[1], i1[2])
        e00, e10, e01, e11 = v100 - v000, v110 - v010, v101 - v001, v111 - v011
        ex0, ex1 = e00 + w[1] * (e10 - e00), e01 + w[1] * (e11 - e01)
        a00, a10, a01, a11 = v000 + w[0] * e00, v010 + w[0] * e10, v001 + w[0] * e01, v011 + w[0] * e11
        ey0, ey1 = a10 - a00, a11 - a01
        b0, b1 = a00 + w[1] * ey0, a01 + w[1] * ey1
        g = [np.where(live, x, 0).astype(dt) for x in (ex0 + w[2] * (ex1 - ex0), ey0 + w[2] * (ey1 - ey0), b1 - b0)]
        wgt = (s * span / nf).astype(dt)
        piv = np.asarray(pivots[n], np.float32).astype(dt)
        rays = [g[a].sum(1, dtype=dt) for a in range(3)]
        rays += [(g[a] * (p[b] - piv[b])).astype(dt).sum(1, dtype=dt) for a in range(3) for b in range(3)]
        for j, x in enumerate(rays):
            out[n, j] = (da * (wgt * x).astype(dt)).astype(dt).astype(np.float64).sum()
    return out


# ---- the chain to the pose parameters ----------------------------------------------------------------------------------
def xi(theta, centre, I2P, pose_deltas, h=1e-5):
    """[6, 4, 4]: Xi_i = inv(I2P) (dD / d theta_i) inv(D) I2P by central differences of pose_deltas (float64): the motion
    of a point of the moving objects in index coordinates per unit of theta_i."""
    theta = np.asarray(theta, np.float64).reshape(6)
    steps = np.concatenate([theta[None] + h * np.eye(6), theta[None] - h * np.eye(6)])
    Dm = pose_deltas(steps, centre)
    dD = (Dm[:6] - Dm[6:]) / (2 * h)
    Dinv = np.linalg.inv(pose_deltas(theta[None], centre)[0])
    return np.linalg.inv(I2P)[None] @ dD @ Dinv[None] @ np.asarray(I2P, np.float64)[None]


def chain(grad, pivots, Xi, moving):
    """[6]: d cost / d theta_i = sum over the moving objects of <Mom, L_i> + F . (L_i pivot + tau_i), L_i = Xi_i[:3, :3],
    tau_i = Xi_i[:3, 3]; grad [n_obj, 12], pivots [n_obj, 3]."""
    out = np.zeros(6)
    piv = np.asarray(pivots, np.float64)
    for i in range(6):
        L, tau = Xi[i, :3, :3], Xi[i, :3, 3]
        for n in moving:
            F, Mom = grad[n, :3], grad[n, 3:].reshape(3, 3)
            out[i] += float((Mom * L).sum() + F @ (L @ piv[n] + tau))
    return out


def model_cost_and_grad(S, start_poses, moving, fixed, pose_deltas, step_mm=1.0, dtype=np.float64):
    """fun(theta [6]) -> (cost, gradient [6]) for dfl_amd.register.bfgs: reg_ref.model_cost_fn with its frozen-sampling
    gradient, all by the numpy models."""
    ctr = R.volume_centre(S)
    q = S['Q'].astype(np.float32)

    def fun(theta):
        Dm = pose_deltas(np.asarray(theta, np.float64).reshape(1, 6), ctr)[0]
        poses = [Dm @ P if n in moving else P for n, P in enumerate(start_poses)]
        recs = D.pack([D.c2i(S['I2P'], P, S['E']) for P in poses], D.MASKS, S['Q'], S['lab'], True, 'trilinear')
        att = D.render(S['mu'], S['lab'], recs, q, S['rows'], S['cols'], 'trilinear', step_mm=step_mm, dtype=dtype)[0]
        cost, d_att = sim_adjoint(att, fixed, None, dtype)
        piv = box_pivots(recs)
        grad = pose_moments(S['mu'], S['lab'], recs, q, S['rows'], S['cols'], d_att, piv, step_mm, dtype)
        return float(cost), chain(grad, piv, xi(theta, ctr, S['I2P'], pose_deltas), moving)

    return fun
