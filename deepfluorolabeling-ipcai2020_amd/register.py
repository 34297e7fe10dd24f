"""2D/3D registration of the CT to one projection: a start pose from 2D landmarks (pnp), then a CMA-ES over six pose
parameters whose cost is the gradient-NCC between rendered DRRs and the fixed image: one correlation over the whole
image (similarity='global') or the mean over patches (similarity='patch'), and optionally a reprojection term that
keeps the pose near detected landmarks.

The geometry is float64 numpy on the host, as in dfl_amd.drr; the pixels stay on the device.  One generation of the
optimiser is one dfl_drr_render launch (trilinear, tight boxes, lambda views), one dfl_sim_gradncc launch
(csrc/sim.hip) and one copy of lambda doubles to the host; the records and the argument block of the render are
drr.pack and drr.args_for_records.  DESIGN.md section 16 states the semantics of the similarity; tests/reg_ref.py
restates them in numpy float64.  The patch cost (dfl_sim_patch_gradncc, csrc/sim_patch.hip) and the landmark term are
section 18 and tests/patch_ref.py.  register(refine=K) finishes with a dense BFGS (bfgs) on the gradient of the cost with
respect to the six parameters: one render, the adjoint of the similarity (dfl_sim_gradncc_bwd) and the forces and moments
it exerts on every object (dfl_drr_pose_grad, sampling frozen), chained to theta through pose_delta_jacobians; section 19
and tests/grad_ref.py.  register_many registers N projections of one volume at once: the candidates of all problems go through
one render and one launch against a bank of fixed images (SimilarityBank, dfl_sim_bank_gradncc), the optimisers advance in
lockstep (cma_steps, bfgs_steps, lockstep), and every result has the bytes register() finds for it alone; section 20.
patch_weight='variance' weighs every patch by the energy of its fixed gradient (dfl_sim_patch_weights) and has an adjoint
(dfl_sim_patch_eval), so the patch cost can be refined too; section 21 and tests/patch_grad_ref.py.
similarity='outline' matches the bone outlines of a predicted label map instead of intensities: the exact render writes the
label map of every candidate, dfl_label_edt their boundary distance maps, and dfl_sim_outline (csrc/sim_outline.hip,
OutlineSimilarity) the truncated chamfer cost against the segmentation's; section 26 and tests/outline_ref.py.
similarity='mi' is the negative mutual information of the intensities (MISimilarity: dfl_sim_mi, csrc/sim_mi.hip), from a joint
histogram of integers: it needs neither a known intensity mapping of the fixed image nor edges, and has an adjoint
(dfl_sim_mi_bwd), so refine works with it; section 29 and tests/mi_ref.py.

    D(theta) = [[R, centre - R centre + theta[3:]], [0, 1]],  R = exp(rot_unit theta[:3])      (pose_delta)
    P(theta) = D(theta) P0                                   a cam-to-*-vol matrix as in gt-poses
    C2I(theta) = inv(I2P) D(theta) I2P C2I0                  what the renderer gets (drr.Obj.c2i)

With rot_unit 0.02 one unit of any parameter moves a point 50 mm from the centre by about 1 mm, so one sigma serves
all six.  Tensors on the CPU are refused: there is no CPU path.
"""
import numpy as np
import torch

from . import _native as nat
from . import drr, preprocess
from . import labels as _labels

__all__ = ['se3_exp', 'se3_log', 'pose_delta', 'pose_deltas', 'pose_delta_jacobians', 'pnp', 'cma_es', 'cma_steps', 'CmaResult', 'bfgs', 'bfgs_steps', 'BfgsResult', 'lockstep',
           'Similarity', 'PatchSimilarity', 'SimilarityBank', 'PatchSimilarityBank', 'OutlineSimilarity', 'MISimilarity', 'fixed_of_array', 'landmark_penalty', 'register',
           'register_many', 'default_max_views', 'Registration', 'with_pelvis_pose', 'volume_centre']

ROT_UNIT = 0.02


# ---- rigid motions -----------------------------------------------------------------------------------------------------
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _abc(t):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3, by their series below 1e-4."""
    if t < 1e-4:
        t2 = t * t
        return 1.0 - t2 / 6.0, 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
    return np.sin(t) / t, (1.0 - np.cos(t)) / (t * t), (t - np.sin(t)) / (t ** 3)


def se3_exp(xi):
    """(rotation vector [3], v [3]) -> the 4 x 4 rigid motion exp of the twist: R = exp(hat w), t = V v."""
    xi = np.asarray(xi, np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    a, b, c = _abc(float(np.linalg.norm(w)))
    W = _hat(w)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * W + b * (W @ W)
    T[:3, 3] = (np.eye(3) + b * W + c * (W @ W)) @ v
    return T


def se3_log(T):
    """The inverse of se3_exp for rotations below pi: a 4 x 4 rigid motion -> [6]."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    R = T[:3, :3]
    skew = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(skew)), 0.5 * (np.trace(R) - 1.0)
    t = float(np.arctan2(s, c))
    if s < 1e-12 and c < 0:
        raise nat.DflError('register.se3_log: a rotation by pi has no unique logarithm')
    w = skew * (t / s if s > 1e-8 else 1.0 + t * t / 6.0)
    a, b, c3 = _abc(t)
    W = _hat(w)
    V = np.eye(3) + b * W + c3 * (W @ W)
    return np.concatenate([w, np.linalg.solve(V, T[:3, 3])])


def pose_deltas(thetas, centre, rot_unit=ROT_UNIT):
    """[n, 6] -> [n, 4, 4]: pose_delta of every row, with batched numpy products (Rodrigues' formula)."""
    th = np.asarray(thetas, np.float64).reshape(-1, 6)
    ctr = np.asarray(centre, np.float64).reshape(3)
    w = th[:, :3] * float(rot_unit)
    t = np.linalg.norm(w, axis=1)
    small = t < 1e-4
    ts = np.where(small, 1.0, t)
    a = np.where(small, 1.0 - t * t / 6.0, np.sin(ts) / ts)
    b = np.where(small, 0.5 - t * t / 24.0, (1.0 - np.cos(ts)) / (ts * ts))
    W = np.zeros((th.shape[0], 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    R = np.eye(3)[None] + a[:, None, None] * W + b[:, None, None] * (W @ W)
    D = np.zeros((th.shape[0], 4, 4))
    D[:, :3, :3] = R
    D[:, :3, 3] = ctr[None] - R @ ctr + th[:, 3:]
    D[:, 3, 3] = 1.0
    return D


def pose_delta(theta, centre, rot_unit=ROT_UNIT):
    """Six parameters -> the 4 x 4 D: the rotation exp(theta[:3] rot_unit) (rotation vector, radians) about `centre` in
    the volume's physical frame, followed by the translation theta[3:] in mm."""
    return pose_deltas(np.asarray(theta, np.float64).reshape(1, 6), centre, rot_unit)[0]


def pose_delta_jacobians(thetas, centre, rot_unit=ROT_UNIT):
    """[n, 6] -> [n, 6, 4, 4] float64: d pose_delta(theta) / d theta_i, analytic.  With w = rot_unit theta[:3] and
    R = exp(hat w), d R / d w_i = hat(w_i w + w x (I - R) e_i) R / |w|^2 (Gallego and Yezzi 2015), below |w| = 1e-4 the
    series of the exponential to third order; a translation parameter moves the translation column alone."""
    th = np.asarray(thetas, np.float64).reshape(-1, 6)
    ctr = np.asarray(centre, np.float64).reshape(3)
    R = pose_deltas(th, ctr, rot_unit)[:, :3, :3]
    out = np.zeros((th.shape[0], 6, 4, 4))
    for k in range(th.shape[0]):
        w = th[k, :3] * float(rot_unit)
        t2, W = float(w @ w), _hat(w)
        for i in range(3):
            E = _hat(np.eye(3)[i])
            if t2 < 1e-8:
                dR = E + (E @ W + W @ E) / 2.0 + (E @ W @ W + W @ E @ W + W @ W @ E) / 6.0
            else:
                dR = _hat(w[i] * w + np.cross(w, (np.eye(3) - R[k])[:, i])) @ R[k] / t2
            out[k, i, :3, :3] = float(rot_unit) * dR
            out[k, i, :3, 3] = -float(rot_unit) * (dR @ ctr)
            out[k, 3 + i, i, 3] = 1.0
    return out


def volume_centre(volume_shape, I2P):
    """The physical position of the middle of a [nz, ny, nx] volume."""
    nz, ny, nx = volume_shape
    return (np.asarray(I2P, np.float64) @ np.array([(nx - 1) / 2.0, (ny - 1) / 2.0, (nz - 1) / 2.0, 1.0]))[:3]


def with_pelvis_pose(geom, P):
    """A copy of geom whose pelvis pose (the one drr.project_points uses) is P."""
    poses = dict(geom.poses)
    poses[drr.POSES[0]] = np.array(P, np.float64).reshape(4, 4)
    return drr.Geometry(geom.K, geom.E, poses, geom.I2P, geom.G, geom.objects, geom.grid)


# ---- pose from landmarks -----------------------------------------------------------------------------------------------
def _project(Kt, V2C, X):
    cam = V2C[:3, :3] @ X.T + V2C[:3, 3:4]
    p = Kt @ cam
    return p[:2] / p[2:3]


def _dlt(Kt, X, x):
    """V2C (volume physical frame -> camera projective frame) from >= 6 points, or None when they do not determine it."""
    n = X.shape[0]
    Xm, xm = X.mean(0), x.mean(1)
    Xs = np.sqrt(3.0) / max(float(np.sqrt(((X - Xm) ** 2).sum(1)).mean()), 1e-300)
    xs = np.sqrt(2.0) / max(float(np.sqrt(((x - xm[:, None]) ** 2).sum(0)).mean()), 1e-300)
    TX = np.diag([Xs, Xs, Xs, 1.0])
    TX[:3, 3] = -Xs * Xm
    Tx = np.diag([xs, xs, 1.0])
    Tx[:2, 2] = -xs * xm
    Xh = (TX @ np.concatenate([X, np.ones((n, 1))], 1).T).T
    xh = Tx @ np.concatenate([x, np.ones((1, n))], 0)
    A = np.zeros((2 * n, 12))
    A[0::2, 0:4], A[0::2, 8:12] = Xh, -xh[0][:, None] * Xh
    A[1::2, 4:8], A[1::2, 8:12] = Xh, -xh[1][:, None] * Xh
    _, sv, Vt = np.linalg.svd(A)
    if sv[10] <= 1e-9 * sv[0]:                                 # a null space of more than one dimension: coplanar points
        return None
    M = np.linalg.inv(Tx) @ Vt[-1].reshape(3, 4) @ TX
    T = np.linalg.inv(Kt) @ M
    det = float(np.linalg.det(T[:, :3]))
    if abs(det) < 1e-300:
        return None
    T = T / (np.sign(det) * abs(det) ** (1.0 / 3.0))
    U, _, Wt = np.linalg.svd(T[:, :3])
    V2C = np.eye(4)
    V2C[:3, :3] = U @ Wt
    V2C[:3, 3] = T[:, 3]
    return V2C


def pnp(geom, X3d, x2d, P_init=None, iterations=100):
    """The cam-to-pelvis-vol pose under which drr.project_points maps X3d [L, 3] (volume physical frame) onto x2d [2, L]
    ((column, row) on geom's output grid), in the least-squares sense of the reprojection error.  Columns of x2d holding
    NaN are skipped (est_lands_csv.py marks a landmark it did not find that way).  The start is the linear solution
    (DLT) where at least 6 usable, non-coplanar points exist, else P_init; Levenberg-Marquardt follows.  Fewer than 4
    usable points are refused."""
    X = np.asarray(X3d, np.float64).reshape(-1, 3)
    x = np.asarray(x2d, np.float64)
    if x.ndim != 2 or x.shape[0] != 2 or x.shape[1] != X.shape[0]:
        raise nat.DflError('register.pnp: X3d is %s and x2d %s: [L, 3] and [2, L] expected' % (X.shape, x.shape))
    use = np.isfinite(x).all(0) & np.isfinite(X).all(1)
    if int(use.sum()) < 4:
        raise nat.DflError('register.pnp: %d usable landmarks (at least 4 are needed)' % int(use.sum()))
    X, x = X[use], x[:, use]
    Kt = np.linalg.inv(geom.G) @ geom.K
    V2C = _dlt(Kt, X, x) if X.shape[0] >= 6 else None
    if V2C is None:
        if P_init is None:
            raise nat.DflError('register.pnp: %d usable landmarks do not determine a pose linearly (6 non-coplanar ones do) '
                               'and no P_init was given' % X.shape[0])
        V2C = geom.E @ np.linalg.inv(np.asarray(P_init, np.float64).reshape(4, 4))
    ctr = X.mean(0)

    def moved(T, xi):                                          # turn about the landmarks' centroid, then shift, in mm units
        return T @ pose_delta(xi, ctr)

    def resid(T):
        return (_project(Kt, T, X) - x).reshape(-1)

    r = resid(V2C)
    lam, h = 1e-3, 1e-6
    for _ in range(int(iterations)):
        J = np.stack([(resid(moved(V2C, h * e)) - resid(moved(V2C, -h * e))) / (2 * h) for e in np.eye(6)], 1)
        H, g = J.T @ J, J.T @ r
        better = False
        for _ in range(12):
            step = np.linalg.solve(H + lam * np.diag(np.diag(H) + 1e-12), -g)
            cand = moved(V2C, step)
            rc = resid(cand)
            if rc @ rc < r @ r:
                V2C, r, lam, better = cand, rc, max(lam / 10.0, 1e-12), True
                break
            lam *= 10.0
        if not better or float(np.abs(step).max()) < 1e-13:
            break
    U, _, Wt = np.linalg.svd(V2C[:3, :3])                      # products of rotations drift by rounding only
    V2C[:3, :3] = U @ Wt
    return np.linalg.inv(V2C) @ geom.E                         # V2C = E inv(P)


# ---- the optimiser -----------------------------------------------------------------------------------------------------
class CmaResult:
    """mean: the final mean; best_x, best_f: the best candidate evaluated; trace: the best cost of every generation;
    evaluations: how many candidates were evaluated; sigma: the final step size."""

    def __init__(self, mean, best_x, best_f, trace, evaluations, sigma):
        self.mean, self.best_x, self.best_f, self.trace, self.evaluations, self.sigma = mean, best_x, best_f, trace, evaluations, sigma


def _drive(steps, answer):
    """Run a step-wise optimiser (cma_steps, bfgs_steps) to its end with answer(point) as the reply to every request."""
    try:
        x = next(steps)
        while True:
            x = steps.send(answer(x))
    except StopIteration as stop:
        return stop.value


def lockstep(steppers, evaluate):
    """Advance step-wise optimisers together.  Every round collects the request of each stepper that still runs and calls
    evaluate(indices, points) once -- indices into `steppers`, ascending, and the point each of them asked for -- which
    returns one reply per point; a stepper that ends drops out of the later rounds.  Returns every stepper's result."""
    steppers = list(steppers)
    results, pending = [None] * len(steppers), {}

    def advance(i, step):
        try:
            pending[i] = step()
        except StopIteration as stop:
            pending.pop(i, None)
            results[i] = stop.value

    for i, s in enumerate(steppers):
        advance(i, lambda s=s: next(s))
    while pending:
        idx = sorted(pending)
        replies = list(evaluate(idx, [pending[i] for i in idx]))
        if len(replies) != len(idx):
            raise nat.DflError('register.lockstep: evaluate returned %d replies for %d points' % (len(replies), len(idx)))
        for i, r in zip(idx, replies):
            advance(i, lambda i=i, r=r: steppers[i].send(r))
    return results


def cma_es(cost_fn, x0, sigma0, popsize=None, generations=100, seed=0):
    """A plain (mu/mu_w, lambda) CMA-ES with Hansen's default constants (The CMA Evolution Strategy: A Tutorial, 2016).
    cost_fn takes [lambda, n] and returns [lambda].  Random draws come from numpy.random.default_rng(seed) on the host and
    the ranking is a stable sort, so a run repeats bit for bit.  This is cma_steps driven by cost_fn."""
    return _drive(cma_steps(x0, sigma0, popsize, generations, seed), cost_fn)


def cma_steps(x0, sigma0, popsize=None, generations=100, seed=0):
    """cma_es as a generator: it yields the candidates [lambda, n] of a generation, is sent their costs [lambda], and
    returns its CmaResult (StopIteration.value) after `generations` of them.  Several can be advanced together (lockstep)."""
    x0 = np.asarray(x0, np.float64).reshape(-1)
    n = x0.size
    lam = int(popsize) if popsize else 4 + int(3 * np.log(n))
    if lam < 4 or not float(sigma0) > 0 or int(generations) < 0:
        raise nat.DflError('register.cma_es: popsize %d (at least 4), sigma0 %r (positive), generations %r' % (lam, sigma0, generations))
    rng = np.random.default_rng(seed)
    mu = lam // 2
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1))
    w = w / w.sum()
    mueff = 1.0 / float((w ** 2).sum())
    cc = (4 + mueff / n) / (n + 4 + 2 * mueff / n)
    cs = (mueff + 2) / (n + mueff + 5)
    c1 = 2 / ((n + 1.3) ** 2 + mueff)
    cmu = min(1 - c1, 2 * (mueff - 2 + 1 / mueff) / ((n + 2) ** 2 + mueff))
    damps = 1 + 2 * max(0.0, np.sqrt((mueff - 1) / (n + 1)) - 1) + cs
    chin = np.sqrt(n) * (1 - 1 / (4.0 * n) + 1 / (21.0 * n * n))
    mean, sigma = x0.copy(), float(sigma0)
    pc, ps = np.zeros(n), np.zeros(n)
    Cm, B, Dg = np.eye(n), np.eye(n), np.ones(n)
    best_x, best_f, trace = x0.copy(), np.inf, []
    for gen in range(int(generations)):
        z = rng.standard_normal((lam, n))
        y = (z * Dg[None]) @ B.T
        xs = mean[None] + sigma * y
        f = np.asarray((yield xs), np.float64).reshape(-1)
        if f.size != lam:
            raise nat.DflError('register.cma_es: cost_fn returned %d values for %d candidates' % (f.size, lam))
        f = np.where(np.isfinite(f), f, np.inf)
        order = np.argsort(f, kind='stable')
        if f[order[0]] < best_f:
            best_f, best_x = float(f[order[0]]), xs[order[0]].copy()
        trace.append(float(f[order[0]]))
        ysel = y[order[:mu]]
        yw = w @ ysel
        mean = mean + sigma * yw
        ps = (1 - cs) * ps + np.sqrt(cs * (2 - cs) * mueff) * (B @ ((B.T @ yw) / Dg))
        hsig = float(np.linalg.norm(ps) / np.sqrt(1 - (1 - cs) ** (2 * (gen + 1))) / chin < 1.4 + 2 / (n + 1.0))
        pc = (1 - cc) * pc + hsig * np.sqrt(cc * (2 - cc) * mueff) * yw
        Cm = (1 - c1 - cmu) * Cm + c1 * (np.outer(pc, pc) + (1 - hsig) * cc * (2 - cc) * Cm) + cmu * (ysel.T * w[None]) @ ysel
        sigma = sigma * float(np.exp((cs / damps) * (np.linalg.norm(ps) / chin - 1)))
        Cm = 0.5 * (Cm + Cm.T)
        ev, B = np.linalg.eigh(Cm)
        Dg = np.sqrt(np.maximum(ev, 1e-300))
    return CmaResult(mean, best_x, best_f, np.array(trace), lam * int(generations), sigma)


class BfgsResult:
    """x, f: the last accepted point and its cost; trace: the accepted costs, the start's first (never increasing);
    evaluations: calls of the cost-and-gradient function; iterations: steps accepted."""

    def __init__(self, x, f, trace, evaluations, iterations):
        self.x, self.f, self.trace, self.evaluations, self.iterations = x, f, trace, evaluations, iterations


def bfgs(fun, x0, iterations=30, tol=1e-4, c1=1e-4, min_step=1e-6):
    """A dense BFGS with Armijo backtracking (halving): the local finish of register().  fun takes [n] and returns
    (cost, gradient [n]).  The inverse-Hessian estimate starts as the identity and returns to it when its direction is
    not a descent direction; from the identity the first trial step is min(1, 1 / |g|), else 1.  A trial whose cost is
    not finite or fails f <= f0 + c1 t g.p is rejected, so the accepted costs never increase.  It stops after
    `iterations` accepted steps, when an accepted step is shorter than tol, or when the trial step |t p| falls below min_step."""
    return _drive(bfgs_steps(x0, iterations, tol, c1, min_step), fun)


def bfgs_steps(x0, iterations=30, tol=1e-4, c1=1e-4, min_step=1e-6):
    """bfgs as a generator: it yields the point [n] it wants evaluated, is sent (cost, gradient [n]), and returns its
    BfgsResult (StopIteration.value).  Problems need different numbers of trials, so generators advanced together
    (lockstep) end at different rounds."""
    x = np.asarray(x0, np.float64).reshape(-1).copy()
    n = x.size
    f, g = yield x
    f, g = float(f), np.asarray(g, np.float64).reshape(n)
    if not np.isfinite(f) or not np.isfinite(g).all():
        raise nat.DflError('register.bfgs: the cost or its gradient is not finite at the start (%r)' % f)
    Hm, fresh = np.eye(n), True
    trace, evals, done = [f], 1, 0
    while done < int(iterations):
        p = -Hm @ g
        if not g @ p < 0.0:
            Hm, fresh, p = np.eye(n), True, -g
        slope = float(g @ p)
        if not slope < 0.0:                                        # a zero gradient
            break
        t = min(1.0, 1.0 / float(np.linalg.norm(g))) if fresh else 1.0
        accepted = None
        while t * float(np.linalg.norm(p)) >= min_step:
            xn = x + t * p
            fn, gn = yield xn
            fn, gn = float(fn), np.asarray(gn, np.float64).reshape(n)
            evals += 1
            if np.isfinite(fn) and np.isfinite(gn).all() and fn <= f + c1 * t * slope:
                accepted = (xn, fn, gn)
                break
            t *= 0.5
        if accepted is None:
            break
        xn, fn, gn = accepted
        s, y = xn - x, gn - g
        sy = float(s @ y)
        if sy > 1e-12 * float(np.linalg.norm(s) * np.linalg.norm(y)):
            A = np.eye(n) - np.outer(s, y) / sy
            Hm, fresh = A @ Hm @ A.T + np.outer(s, s) / sy, False
        x, f, g = xn, fn, gn
        trace.append(f)
        done += 1
        if float(np.linalg.norm(s)) < tol:
            break
    return BfgsResult(x, f, np.array(trace), evals, done)


# ---- the similarity on the device --------------------------------------------------------------------------------------
def _device_image(t, what, dims, dtypes=(torch.float32,)):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise nat.DflError('register: %s must be a tensor on the GPU (no CPU path)' % what)
    if t.dim() != dims or t.dtype not in dtypes:
        raise nat.DflError('register: %s has shape %s and dtype %s: %d dimensions of %s expected'
                           % (what, tuple(t.shape), t.dtype, dims, ' or '.join(str(d) for d in dtypes)))
    return t.detach().contiguous()


def _patch_params(radius, stride, min_count):
    """(rho, stride, min_count) as integers; min_count=None is half a patch, rounded up."""
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (radius, stride)) and \
        (min_count is None or (isinstance(min_count, (int, np.integer)) and not isinstance(min_count, bool)))
    if not ok or radius < 1 or stride < 1 or (min_count is not None and min_count < 1):
        raise nat.DflError('register: a patch radius of %r, a stride of %r and a min_count of %r (integers, at least 1 each)'
                           % (radius, stride, min_count))
    side = 2 * int(radius) + 1
    return int(radius), int(stride), (side * side + 1) // 2 if min_count is None else int(min_count)


def _patch_weight(weight):
    if weight not in ('uniform', 'variance'):
        raise nat.DflError("register: a patch weight of %r ('uniform' or 'variance')" % (weight,))
    return weight


def fixed_of_array(fixed_of, V, F):
    """A sequence or array that says which of F fixed images each of V views is scored against -> int32 [V], checked on
    the host: integers, one per view, each in [0, F)."""
    a = np.asarray(fixed_of)
    if a.ndim != 1 or a.shape[0] != V or a.dtype.kind not in 'iu':
        raise nat.DflError('register: fixed_of has shape %s and dtype %s: %d integers expected, one per view' % (a.shape, a.dtype, V))
    if V and (int(a.min()) < 0 or int(a.max()) >= F):
        raise nat.DflError('register: fixed_of holds %d .. %d, the bank has the images 0 .. %d' % (int(a.min()), int(a.max()), F - 1))
    return np.ascontiguousarray(a, np.int32)


_BLOCKS = {}                                                        # entry point -> (its struct, the names of the struct's fields)


def _block(entry, values):
    """The argument block of a dfl_sim_* entry point (dfl_sim_patch_eval -> nat.SimPatchEvalArgs) filled from `values`, a dict of
    every field any of these blocks has, addresses and integers: the struct takes the ones its _fields_ name, in their order."""
    if entry not in _BLOCKS:
        cls = getattr(nat, ''.join(word.capitalize() for word in entry.split('_')[1:]) + 'Args')
        _BLOCKS[entry] = cls, tuple(name for name, *_ in cls._fields_)
    cls, names = _BLOCKS[entry]
    return cls(*map(values.__getitem__, names))


def _scratch(need, dev, least=0):
    """A float64 scratch of `need` doubles, which is what a dfl_*_scratch_doubles function just said: negative is its refusal."""
    if need < 0:
        raise nat.DflError('register: %s' % nat.lib().dfl_last_error().decode())
    return torch.empty(max(int(need), least), dtype=torch.float64, device=dev)


class Similarity:
    """The gradient-NCC cost of `views` moving images against one fixed image [H, W] (float32, on the GPU) with an
    optional uint8 [H, W] mask: dfl_sim_prepare runs here, once; cost(moving) is one dfl_sim_gradncc launch and
    returns a float64 tensor [V] on the device.

    This class holds the one body of the four similarities: the work is done on banks [F, ...]; a class says what it
    calls (`entry`), whether it is a bank (else F = 1 and the attributes are the [0] views of the banks, and fixed_of is
    None everywhere) and whether it has patches."""

    entry, _bank, _patches = 'dfl_sim_gradncc', False, False        # entry: what launch() calls with args()

    def __init__(self, fixed, mask=None, views=1):
        self._setup(fixed, mask, views)

    def _setup(self, fixed, mask, views, patch=None):
        """patch = (radius, stride, min_count, weight) as the caller gave them, for the classes with patches."""
        if self._patches:
            self.radius, self.stride, self.min_count = _patch_params(*patch[:3])
            self.weight = _patch_weight(patch[3])
        dims = 3 if self._bank else 2
        image, the_mask, verb = ('the fixed images', 'the masks', 'are') if self._bank else ('the fixed image', 'the mask', 'is')
        fixed = _device_image(fixed, image, dims)
        dev, shape = fixed.device, tuple(int(s) for s in fixed.shape)
        H, W = shape[-2:]
        F = shape[0] if self._bank else 1
        self.H, self.W, self.views = H, W, int(views)
        if mask is not None:
            mask = _device_image(mask, the_mask, dims, (torch.uint8,))
            if tuple(mask.shape) != shape or mask.device != dev:
                raise nat.DflError('register: %s %s %s on %s, %s %s on %s' % (the_mask, verb, tuple(mask.shape), mask.device, image, shape, dev))
        if self._bank:
            if not 1 <= F <= 65535 or F * H * W >= 2 ** 31:
                raise nat.DflError('register: a bank of %d images of %d x %d (1..65535 images, fewer than 2^31 pixels)' % (F, H, W))
            self.F, self._fixed_of = F, {}
        lib = nat.lib()
        self.scratch = _scratch(lib.dfl_sim_scratch_doubles(self.views, H, W), dev, 1)
        self.out = torch.empty(self.views, dtype=torch.float64, device=dev)
        self.bwd_scratch = None                                     # cost_and_adjoint sizes it when it first runs
        self._sizes = dict(H=H, W=W, F=F, reserved=0)

        def bank(dtype, *per_image):
            return torch.empty((F,) + per_image, dtype=dtype, device=dev)

        self._banks = dict(fixed=fixed.reshape(F, H, W), mask=None if mask is None else mask.reshape(F, H, W),
                           fx=bank(torch.float32, H, W), fy=bank(torch.float32, H, W), counted=bank(torch.uint8, H, W),
                           totals=bank(torch.float64, nat.SIM_TOTALS))
        self._each_image(dev, 'dfl_sim_prepare')
        if self._patches:
            P = int(lib.dfl_sim_patch_count(H, W, self.radius, self.stride))
            if P < 0:
                raise nat.DflError('register: %s' % lib.dfl_last_error().decode())
            self.pscratch = _scratch(lib.dfl_sim_patch_scratch_doubles(self.views, H, W, self.radius, self.stride), dev)
            self.patches = P
            self._sizes.update(rho=self.radius, stride=self.stride, min_count=self.min_count, P=P)
            self._banks.update(ptotals=bank(torch.float64, P, nat.SIM_TOTALS), pflags=bank(torch.uint8, P), pcount=bank(torch.int32, 2))
            self._each_image(dev, 'dfl_sim_patch_prepare')
            if self.weight == 'variance':
                self.entry = 'dfl_sim_patch_eval'
                self._banks.update(pweights=bank(torch.float64, P, 2), pwsum=bank(torch.float64, 2))
                self._each_image(dev, 'dfl_sim_patch_weights')
        for name, t in self._banks.items():                         # fixed, mask, fx, fy, counted, totals, ptotals, pflags, ...
            setattr(self, name, t if self._bank or t is None else t[0])
        self._fields = dict({name: nat.ptr(t) for name, t in self._banks.items()}, **self._sizes)      # what every launch passes

    def _each_image(self, dev, entry):
        """One launch of a preparing entry point per image, on that image's slices of the banks."""
        for f in range(self._sizes['F']):
            drr.launch(dev, entry, _block(entry, dict({name: None if t is None else t[f].data_ptr() for name, t in self._banks.items()}, **self._sizes)))

    def _args(self, entry, moving, fixed_of, scratch, out, d_moving=None):
        return _block(entry, dict(self._fields, moving=moving.data_ptr(), fixed_of=nat.ptr(fixed_of), scratch=scratch.data_ptr(), cost=out.data_ptr(),
                                  d_moving=nat.ptr(d_moving), scratch_doubles=scratch.numel(), V=int(moving.shape[0])))

    def _which(self, fixed_of, V):
        """fixed_of as the kernels read it: a bank's checked device tensor, None for one image."""
        return self.fixed_of(fixed_of, V) if self._bank else None

    def _forward(self, moving, fixed_of, out):
        return self._args(self.entry, moving, fixed_of, self.pscratch if self._patches else self.scratch, self.out if out is None else out)

    def _launch(self, moving, fixed_of=None, out=None):
        drr.launch(moving.device, self.entry, self._forward(moving, self._which(fixed_of, int(moving.shape[0])), out))

    def args(self, moving, out=None):
        return self._forward(moving, None, out)

    def _moving(self, moving):
        mv = _device_image(moving, 'the moving images', 3)
        if tuple(mv.shape[1:]) != (self.H, self.W) or mv.device != self.out.device or not 1 <= mv.shape[0] <= self.views:
            raise nat.DflError('register: moving images of shape %s on %s for a fixed image of %d x %d on %s and at most %d views'
                               % (tuple(mv.shape), mv.device, self.H, self.W, self.out.device, self.views))
        return mv

    def launch(self, moving, out=None):
        """One launch of `entry` on checked moving images; the costs go to `out` (default: the first rows of self.out)."""
        self._launch(moving, None, out)

    def cost(self, moving, fixed_of=None):
        mv = self._moving(moving)
        out = torch.empty(mv.shape[0], dtype=torch.float64, device=mv.device)
        self._launch(mv, fixed_of, out)
        return out

    def cost_and_adjoint(self, moving, fixed_of=None):
        """(cost [V] float64, d_moving [V, H, W] float32 = d cost[v] / d moving[v]) on the device: one dfl_sim_gradncc_bwd or
        dfl_sim_bank_gradncc_bwd launch, with patches one dfl_sim_patch_eval launch (section 21), which
        weight='variance' alone has.  The cost has the bits cost(moving) gives."""
        if self._patches and self.weight != 'variance':
            raise nat.DflError("register: the uniform patch similarity has no adjoint here; weight='variance' has (DESIGN.md section 21)")
        mv = self._moving(moving)
        V, dev = int(mv.shape[0]), mv.device
        fixed_of = self._which(fixed_of, V)
        if self.bwd_scratch is None:
            lib = nat.lib()
            self.bwd_scratch = _scratch(lib.dfl_sim_patch_eval_scratch_doubles(self.views, self.H, self.W, self.radius, self.stride, 1)
                                        if self._patches else lib.dfl_sim_gradncc_bwd_scratch_doubles(self.views, self.H, self.W), dev)
        out = torch.empty(V, dtype=torch.float64, device=dev)
        d_moving = torch.empty((V, self.H, self.W), dtype=torch.float32, device=dev)
        entry = 'dfl_sim_patch_eval' if self._patches else self.entry + '_bwd'
        drr.launch(dev, entry, self._args(entry, mv, fixed_of, self.bwd_scratch, out, d_moving))
        return out, d_moving


class PatchSimilarity(Similarity):
    """The patch-wise gradient-NCC cost with the interface of Similarity: patches of side
    2 radius + 1 every `stride` interior pixels; a patch with fewer than min_count counted pixels (default: half of it,
    rounded up), or whose fixed gradient does not vary, does not take part.  dfl_sim_prepare and dfl_sim_patch_prepare
    run here, once; cost(moving) is one dfl_sim_patch_gradncc launch.

    weight='variance'  weighs every patch by the energy of its fixed gradient: dfl_sim_patch_weights
    runs after the prepare, cost(moving) is one dfl_sim_patch_eval launch and cost_and_adjoint(moving) works.  The default
    'uniform' is the cost of section 18 through the entry point it always used, and has no adjoint here."""

    entry, _patches = 'dfl_sim_patch_gradncc', True

    def __init__(self, fixed, mask=None, views=1, radius=7, stride=4, min_count=None, weight='uniform'):
        self._setup(fixed, mask, views, (radius, stride, min_count, weight))


# ---- the similarity against a bank of fixed images ---------------------------------------------------------------------
class SimilarityBank(Similarity):
    """Similarity against F fixed images [F, H, W] (float32, on the GPU) with optional uint8 masks [F, H, W]: dfl_sim_prepare
    runs here, once per image, on that image's slice of the banks.  cost(moving, fixed_of) scores view v against image
    fixed_of[v] in one dfl_sim_bank_gradncc launch; the bits of a view's cost are those Similarity(fixed[f], masks[f])
    gives it.  fixed_of is an int32 tensor [V] on the device (not checked: a view whose entry is outside [0, F) costs NaN
    and gets a zero adjoint) or a sequence, which is checked here (fixed_of_array)."""

    entry, _bank = 'dfl_sim_bank_gradncc', True

    def __init__(self, fixed, masks=None, views=1):
        self._setup(fixed, masks, views)

    def fixed_of(self, fixed_of, V):
        """The int32 device tensor [V] the kernels read; sequences are checked on the host and uploaded once each."""
        dev = self.out.device
        if torch.is_tensor(fixed_of):
            if not fixed_of.is_cuda or fixed_of.dtype != torch.int32 or tuple(fixed_of.shape) != (V,) or fixed_of.device != dev:
                raise nat.DflError('register: fixed_of is a tensor of shape %s and dtype %s on %s: int32 [%d] on %s expected'
                                   % (tuple(fixed_of.shape), fixed_of.dtype, fixed_of.device, V, dev))
            return fixed_of.detach().contiguous()
        a = fixed_of_array(fixed_of, V, self.F)
        key = a.tobytes()
        if key not in self._fixed_of:
            if len(self._fixed_of) >= 64:
                self._fixed_of.clear()
            self._fixed_of[key] = torch.from_numpy(a).to(dev)
        return self._fixed_of[key]

    def args(self, moving, fixed_of, out=None):
        return self._forward(moving, fixed_of, out)

    def launch(self, moving, fixed_of, out=None):
        """One launch of `entry` on checked moving images; the costs go to `out` (default: the first rows of self.out)."""
        self._launch(moving, fixed_of, out)


class PatchSimilarityBank(SimilarityBank):
    """PatchSimilarity against F fixed images, with the interface of SimilarityBank: dfl_sim_patch_prepare runs once per
    image on its slice of the patch banks; cost(moving, fixed_of) is one dfl_sim_patch_bank_gradncc launch.  weight='variance'
    is PatchSimilarity's: dfl_sim_patch_weights per image, dfl_sim_patch_eval for the cost, and cost_and_adjoint works."""

    entry, _patches = 'dfl_sim_patch_bank_gradncc', True

    def __init__(self, fixed, masks=None, views=1, radius=7, stride=4, min_count=None, weight='uniform'):
        self._setup(fixed, masks, views, (radius, stride, min_count, weight))


# ---- the outline cost --------------------------------------------------------------------------------------------------
class OutlineSimilarity:
    """The outline cost of `views` moving label maps against a fixed label map: the truncated chamfer
    distance between the boundaries of every label set, 0 .. 1.  segs is uint8 [H, W], or a bank [F, H, W], on the GPU (a
    cleaned 'nn-segs' row); label_sets is what labels.edt takes (an integer or a flat sequence is ONE set, a sequence of
    sequences several); cap is the truncation in pixels.  The exact boundary distance maps of segs (dfl_label_edt) are made
    here, once.

    cost(label_maps [V, H, W] uint8, fixed_of=None) returns a float64 tensor [V] on the device: dfl_label_edt on the views
    (three launches, into buffers made here) and dfl_sim_outline (two); nothing is read back to the host.  With a bank,
    fixed_of says which map each view is scored against, as SimilarityBank takes it.  counts [views, S, 2] (int32: nM, nF)
    and sums [views, S, 2] (float64: a, b) hold the terms of the last call in their first V rows."""

    entry = 'dfl_sim_outline'
    fixed_of = SimilarityBank.fixed_of

    def __init__(self, segs, label_sets, views=1, cap=32.0):
        self._bank = torch.is_tensor(segs) and segs.dim() == 3
        what = 'the segmentations' if self._bank else 'the segmentation'
        segs = _device_image(segs, what, 3 if self._bank else 2, (torch.uint8,))
        self.words, _ = _labels._label_sets(label_sets, 'edt (register.OutlineSimilarity)')
        self.cap, self.views = float(cap), int(views)
        if not self.cap > 0.0 or not np.isfinite(self.cap):
            raise nat.DflError('register: an outline cap of %r pixels (finite, positive)' % (cap,))
        dev, (H, W) = segs.device, (int(s) for s in segs.shape[-2:])
        self.segs, self.H, self.W, self.S = segs, H, W, len(self.words)
        self.F, self._fixed_of = (int(segs.shape[0]) if self._bank else 1), {}
        if segs.numel() == 0 or self.views < 1:
            raise nat.DflError('register: %s of shape %s for %d views: an empty problem' % (what, tuple(segs.shape), self.views))
        self.scratch = _scratch(nat.lib().dfl_sim_outline_scratch_doubles(self.views, self.S, H, W), dev, 1)
        self.d2_fixed = _labels._edt(segs.reshape(self.F, H, W), self.words, True)
        self.rowdist = torch.empty(self.views * self.S * (H * W + 1), dtype=torch.int32, device=dev)
        self.d2_moving = torch.empty((self.views, self.S, H, W), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((self.views, self.S, 2), dtype=torch.int32, device=dev)
        self.sums = torch.zeros((self.views, self.S, 2), dtype=torch.float64, device=dev)
        self.out = torch.empty(self.views, dtype=torch.float64, device=dev)

    def args(self, V, fixed_of=None, out=None):
        """The argument block of dfl_sim_outline for the first V views of d2_moving."""
        return nat.SimOutlineArgs(d2_moving=self.d2_moving.data_ptr(), d2_fixed=self.d2_fixed.data_ptr(), fixed_of=nat.ptr(fixed_of),
                                  counts=self.counts.data_ptr(), sums=self.sums.data_ptr(), cost=(self.out if out is None else out).data_ptr(),
                                  scratch=self.scratch.data_ptr(), scratch_doubles=self.scratch.numel(), cap=self.cap, V=V, F=self.F,
                                  S=self.S, H=self.H, W=self.W, reserved=0)

    def _moving(self, label_maps):
        mv = _device_image(label_maps, 'the moving label maps', 3, (torch.uint8,))
        if tuple(mv.shape[1:]) != (self.H, self.W) or mv.device != self.out.device or not 1 <= mv.shape[0] <= self.views:
            raise nat.DflError('register: moving label maps of shape %s on %s for a segmentation of %d x %d on %s and at most %d views'
                               % (tuple(mv.shape), mv.device, self.H, self.W, self.out.device, self.views))
        return mv

    def _launch(self, label_maps, fixed_of=None, out=None):
        """The distance maps of checked label maps, then one dfl_sim_outline; the costs go to `out` (default: the first rows
        of self.out)."""
        V = int(label_maps.shape[0])
        if self._bank and fixed_of is not None:                     # None: every view against map 0
            fixed_of = self.fixed_of(fixed_of, V)
        elif fixed_of is not None:
            raise nat.DflError('register: fixed_of belongs to a bank of segmentations [F, H, W]; this one is a single map')
        _labels._edt(label_maps, self.words, True, self.rowdist, self.d2_moving[:V])
        drr.launch(label_maps.device, self.entry, self.args(V, fixed_of, out))

    def cost(self, label_maps, fixed_of=None):
        mv = self._moving(label_maps)
        out = torch.empty(mv.shape[0], dtype=torch.float64, device=mv.device)
        self._launch(mv, fixed_of, out)
        return out


# ---- mutual information -----------------------------------------------------------------------------------------------
def _mi_bins(bins):
    """bins as (Bf, Bm): an integer for both, or a pair; each 2 .. SIM_MI_MAX_BINS."""
    pair = (bins, bins) if isinstance(bins, (int, np.integer)) else tuple(bins) if isinstance(bins, (tuple, list)) else ()
    if len(pair) != 2 or any(isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 2 <= b <= nat.SIM_MI_MAX_BINS for b in pair):
        raise nat.DflError('register: mi_bins = %r (an integer or a pair (Bf, Bm) of integers, each 2..%d)' % (bins, nat.SIM_MI_MAX_BINS))
    return int(pair[0]), int(pair[1])


def _mi_range(lo, hi):
    """(lo, hi) as float32 scalars, checked on the host: finite, hi > lo, also after rounding."""
    try:
        lo32, hi32 = np.float32(lo), np.float32(hi)
    except (TypeError, ValueError):
        lo32 = hi32 = np.float32('nan')
    if not (np.isfinite(lo32) and np.isfinite(hi32) and hi32 > lo32):
        raise nat.DflError('register: an mi_range of (%r, %r): two finite numbers with hi > lo' % (lo, hi))
    return lo32, hi32


class MISimilarity:
    """The mutual-information cost of `views` moving images against a fixed image [H, W] (float32, on the
    GPU), or a bank [F, H, W], with an optional uint8 mask of the same shape: cost = -MI of the joint histogram of the moving
    intensity (Bm bins over the moving range, a first-order Parzen window in units of 1/4096 pixel) and the fixed intensity
    (Bf bins between the smallest and largest counted value).  bins is an integer or (Bf, Bm).  A pixel counts when its fixed
    value is finite and its mask byte non-zero; the fixed image needs no known intensity mapping.  dfl_sim_mi_prepare runs here,
    once per image.

    The moving range is set with set_range (or moving_range=(lo, hi), or an [F, 2] array); until then every cost is NaN.
    cost(moving [V, H, W], fixed_of=None) is one dfl_sim_mi launch and returns float64 [V] on the device; with a bank fixed_of says
    which image a view is scored against, as SimilarityBank takes it (None: image 0).  cost_and_adjoint adds d cost / d moving
    (dfl_sim_mi_bwd).  hist [views, Bm, Bf] (int64) holds the histograms of the last call in its first V rows."""

    entry, _patches = 'dfl_sim_mi', False
    fixed_of = SimilarityBank.fixed_of

    def __init__(self, fixed, mask=None, views=1, bins=32, moving_range=None):
        self.Bf, self.Bm = _mi_bins(bins)
        self._bank = torch.is_tensor(fixed) and fixed.dim() == 3
        dims = 3 if self._bank else 2
        image, the_mask = ('the fixed images', 'the masks') if self._bank else ('the fixed image', 'the mask')
        fixed = _device_image(fixed, image, dims)
        dev, shape = fixed.device, tuple(int(s) for s in fixed.shape)
        H, W = shape[-2:]
        F = shape[0] if self._bank else 1
        self.H, self.W, self.F, self.views, self._fixed_of = H, W, F, int(views), {}
        if mask is not None:
            mask = _device_image(mask, the_mask, dims, (torch.uint8,))
            if tuple(mask.shape) != shape or mask.device != dev:
                raise nat.DflError('register: %s of shape %s on %s, %s of shape %s on %s' % (the_mask, tuple(mask.shape), mask.device, image, shape, dev))
        if H < 1 or W < 1 or not 1 <= F <= 65535 or F * H * W >= 2 ** 31 or not 1 <= self.views <= 65535:
            raise nat.DflError('register: %d fixed images of %d x %d for %d views (1..65535 images and views, fewer than 2^31 pixels, none empty)'
                               % (F, H, W, self.views))
        self._banks = dict(fixed=fixed.reshape(F, H, W), mask=None if mask is None else mask.reshape(F, H, W),
                           fbin=torch.empty((F, H, W), dtype=torch.uint8, device=dev),
                           info=torch.empty((F, nat.SIM_MI_INFO), dtype=torch.float64, device=dev),
                           mrange=torch.full((F, 2), float('nan'), dtype=torch.float32, device=dev))
        sizes = dict(H=H, W=W, F=F, Bf=self.Bf, Bm=self.Bm, reserved=0)
        for f in range(F):
            drr.launch(dev, 'dfl_sim_mi_prepare', _block('dfl_sim_mi_prepare', dict({name: None if t is None else t[f].data_ptr()
                                                                                      for name, t in self._banks.items()}, **sizes)))
        for name, t in self._banks.items():                         # fixed, mask, fbin, info, mrange
            setattr(self, name, t if self._bank or t is None else t[0])
        self._fields = dict({name: nat.ptr(t) for name, t in self._banks.items()}, **sizes)
        self.hist = torch.zeros((self.views, self.Bm, self.Bf), dtype=torch.int64, device=dev)
        self.out = torch.empty(self.views, dtype=torch.float64, device=dev)
        self.ell = None                                             # cost_and_adjoint makes it when it first runs
        if moving_range is not None:
            pair = isinstance(moving_range, (tuple, list)) and len(moving_range) == 2 and np.ndim(moving_range[0]) == 0
            self.set_range(*(moving_range if pair else (moving_range,)))

    def set_range(self, lo, hi=None):
        """The moving range: two numbers (checked here; the same for every image), or one [F, 2] tensor or array of (lo, hi) rows.
        A float32 tensor on the device is copied as it is: values cannot be checked without a copy to the host, and an image
        whose row is not finite or has hi <= lo makes its views void (cost NaN, zero adjoint)."""
        rng = self._banks['mrange']
        if hi is not None:
            lo32, hi32 = _mi_range(lo, hi)
            rng.copy_(torch.tensor([[float(lo32), float(hi32)]] * self.F, dtype=torch.float32))
            return
        if torch.is_tensor(lo) and lo.is_cuda:
            if lo.dtype != torch.float32 or tuple(lo.shape) != (self.F, 2) or lo.device != rng.device:
                raise nat.DflError('register: a moving range of shape %s and dtype %s on %s: float32 [%d, 2] on %s expected'
                                   % (tuple(lo.shape), lo.dtype, lo.device, self.F, rng.device))
            rng.copy_(lo.detach())
            return
        rows = np.asarray(lo.cpu() if torch.is_tensor(lo) else lo, np.float64)
        if rows.shape != (self.F, 2):
            raise nat.DflError('register: a moving range of shape %s: two numbers or [%d, 2] expected' % (rows.shape, self.F))
        rng.copy_(torch.tensor([[float(v) for v in _mi_range(*row)] for row in rows], dtype=torch.float32))

    _moving = Similarity._moving

    def _args(self, entry, moving, fixed_of, out, ell=None, d_moving=None):
        return _block(entry, dict(self._fields, moving=moving.data_ptr(), fixed_of=nat.ptr(fixed_of), hist=self.hist.data_ptr(), cost=out.data_ptr(),
                                  ell=nat.ptr(ell), d_moving=nat.ptr(d_moving), V=int(moving.shape[0])))

    def _which(self, fixed_of, V):
        if fixed_of is None:                                        # every view against image 0
            return None
        if not self._bank:
            raise nat.DflError('register: fixed_of belongs to a bank of fixed images [F, H, W]; this one is a single image')
        return self.fixed_of(fixed_of, V)

    def _launch(self, moving, fixed_of=None, out=None):
        """One dfl_sim_mi on checked moving images; the costs go to `out` (default: the first rows of self.out)."""
        drr.launch(moving.device, self.entry, self._args(self.entry, moving, self._which(fixed_of, int(moving.shape[0])), self.out if out is None else out))

    def cost(self, moving, fixed_of=None):
        mv = self._moving(moving)
        out = torch.empty(mv.shape[0], dtype=torch.float64, device=mv.device)
        self._launch(mv, fixed_of, out)
        return out

    def cost_and_adjoint(self, moving, fixed_of=None):
        """(cost [V] float64, d_moving [V, H, W] float32 = d cost[v] / d moving[v] at the range as it is set) on the device: one
        dfl_sim_mi_bwd launch.  The cost has the bits cost(moving) gives; clamped, NaN and uncounted pixels get exactly 0."""
        mv = self._moving(moving)
        V, dev = int(mv.shape[0]), mv.device
        fixed_of = self._which(fixed_of, V)
        if self.ell is None:
            self.ell = torch.empty((self.views, self.Bm, self.Bf), dtype=torch.float64, device=dev)
        out = torch.empty(V, dtype=torch.float64, device=dev)
        d_moving = torch.empty((V, self.H, self.W), dtype=torch.float32, device=dev)
        drr.launch(dev, 'dfl_sim_mi_bwd', self._args('dfl_sim_mi_bwd', mv, fixed_of, out, self.ell, d_moving))
        return out, d_moving


# ---- the landmark term -------------------------------------------------------------------------------------------------
def _usable_landmarks(X3d, x2d, who):
    X = np.asarray(X3d, np.float64)
    x = np.asarray(x2d, np.float64)
    if X.ndim != 2 or X.shape[1] != 3 or x.ndim != 2 or x.shape[0] != 2 or x.shape[1] != X.shape[0]:
        raise nat.DflError('%s: X3d is %s and x2d %s: [L, 3] and [2, L] expected' % (who, X.shape, x.shape))
    use = np.isfinite(x).all(0) & np.isfinite(X).all(1)
    if int(use.sum()) < 1:
        raise nat.DflError('%s: no usable landmark (a finite 2D column with a finite 3D point)' % who)
    return X[use], x[:, use]


def landmark_penalty(geom, poses, X3d, x2d, weight):
    """weight * the mean over the landmarks of |proj_l - x2d_l|^2, for every pelvis pose of poses [n, 4, 4] (or [4, 4]):
    float64 [n].  proj is drr.project_points under that pose, so distances are pixels on geom.grid and weight is per
    square pixel; columns of x2d that are not finite are skipped.  A weight of 0 gives exact zeros."""
    weight = float(weight)
    if not weight >= 0.0 or not np.isfinite(weight):
        raise nat.DflError('register.landmark_penalty: a weight of %r (finite, not negative)' % weight)
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    X, x = _usable_landmarks(X3d, x2d, 'register.landmark_penalty')
    if weight == 0.0:
        return np.zeros(P.shape[0])
    Xh = np.concatenate([X, np.ones((X.shape[0], 1))], 1).T                  # [4, L]
    cam = (np.asarray(geom.E, np.float64)[None] @ np.linalg.inv(P)) @ Xh[None]   # [n, 4, L]
    p = np.asarray(geom.K, np.float64)[None] @ cam[:, :3]
    q = np.linalg.inv(geom.G)[None] @ (p / p[:, 2:3])
    d = q[:, :2] - x[None]
    return weight * (d * d).sum(1).mean(1)


# ---- registration ------------------------------------------------------------------------------------------------------
class Registration:
    """pose: D(theta) P0 of the first moving object (a cam-to-*-vol matrix); poses: the same for every moving object;
    theta; delta = D(theta); cost: the best cost of every generation (all levels, in order); final_cost: the cost at
    theta = similarity_cost + landmark_cost (0 without the landmark term); renders: views rendered; levels: [(factor,
    generations, H, W)]; theta_cma: the CMA-ES mean the
    refinement started from (theta itself without one); refine_cost: the costs bfgs accepted, the start's first;
    gradient_evaluations: cost-and-gradient evaluations (each renders one view and is counted in renders)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Level:
    """The buffers and argument blocks of one resolution level: lambda views of every object on one grid."""

    def __init__(self, volume, grid, fixed, mask, lam, step_mm, patch=None, bank=None):
        """bank=(fixed [F, H, W], masks or None) in place of fixed and mask: the views are scored against a bank, and costs()
        takes fixed_of."""
        self.volume, self.grid, self.lam = volume, grid, lam
        if bank is not None:
            self.sim = SimilarityBank(bank[0], bank[1], lam) if patch is None else PatchSimilarityBank(bank[0], bank[1], lam, *patch)
        else:
            if tuple(fixed.shape) != (grid.H, grid.W):
                raise nat.DflError('register: the fixed image is %s, the output grid %d x %d' % (tuple(fixed.shape), grid.H, grid.W))
            self.sim = Similarity(fixed, mask, lam) if patch is None else PatchSimilarity(fixed, mask, lam, *patch)
        self.step_mm = float(step_mm)

    def _render(self, c2is, masks):
        """(records, att [views, H, W], tensors to keep alive until the render ran): one trilinear render with tight boxes."""
        recs = drr.pack(self.volume, c2is, masks, self.grid, 'trilinear', True)
        a, (att, _, _), keep = drr.args_for_records(self.volume, recs, self.grid, 'trilinear', self.step_mm)
        drr.launch(att.device, 'dfl_drr_render', a)
        return recs, att, keep

    def costs(self, c2is, masks, fixed_of=None):
        """[views <= lambda, n_obj, 4, 4] (and, with a bank, fixed_of [views]) -> float64 [views] on the host: one render, one
        similarity launch, one copy."""
        recs, att, keep = self._render(c2is, masks)
        self.sim._launch(att, fixed_of)
        return self.sim.out[:recs.shape[0]].cpu().numpy()           # the copy waits for both launches: `keep` lives until then

    def costs_and_grads(self, c2is, masks, xis, moving, fixed_of=None):
        """[views <= lambda, n_obj, 4, 4], xis [views, 6, 4, 4] (the motion of the moving objects in index coordinates per
        unit of every parameter; with a bank, fixed_of [views]) -> (float64 [views], float64 [views, 6]) on the host: one render,
        one adjoint of the similarity (cost_and_adjoint), one dfl_drr_pose_grad, one copy; the chain from forces and moments to
        the parameters is float64 numpy."""
        recs, att, keep = self._render(c2is, masks)
        both, piv = self._cost_and_moments(recs, att, *self.sim.cost_and_adjoint(att, fixed_of))
        del keep
        return _theta_chain(both, piv, xis, moving)

    def _cost_and_moments(self, recs, att, cost, d_att):
        """(float64 [views, 1 + n_obj 12] on the host: a view's cost, then the force and moment on every object; the pivots)
        for rendered records and the similarity's (cost, adjoint): one dfl_drr_pose_grad, one copy."""
        piv = drr.box_pivots(recs)
        grad = drr.pose_gradient(self.volume, recs, self.grid, d_att, piv, self.step_mm)
        return torch.cat([cost[:, None], grad.reshape(recs.shape[0], -1)], 1).cpu().numpy(), piv    # the copy waits for every launch


class _OutlineLevel(_Level):
    """_Level for similarity='outline': the views are the label maps of one exact render with tight boxes, the similarity
    an OutlineSimilarity against the segmentation; costs() is _Level's."""

    def __init__(self, volume, grid, segmentation, sets, cap, lam, step_mm):
        self.volume, self.grid, self.lam, self.step_mm = volume, grid, lam, float(step_mm)
        self.sim = OutlineSimilarity(segmentation, sets, lam, cap)

    def _render(self, c2is, masks):
        """(records, label_map [views, H, W] uint8, tensors to keep alive until the render ran)"""
        recs = drr.pack(self.volume, c2is, masks, self.grid, 'exact', True)
        a, (_, _, lab), keep = drr.args_for_records(self.volume, recs, self.grid, 'exact', self.step_mm, want_labels=True)
        drr.launch(lab.device, 'dfl_drr_render', a)
        return recs, lab, keep


class _MILevel(_Level):
    """_Level for similarity='mi': an MISimilarity against the fixed image, or against a bank; the views are _Level's trilinear
    renders.  start_range sets the moving range before the search."""

    def __init__(self, volume, grid, fixed, mask, lam, step_mm, bins, bank=None):
        self.volume, self.grid, self.lam, self.step_mm = volume, grid, lam, float(step_mm)
        if bank is None and tuple(fixed.shape) != (grid.H, grid.W):
            raise nat.DflError('register: the fixed image is %s, the output grid %d x %d' % (tuple(fixed.shape), grid.H, grid.W))
        self.sim = MISimilarity(fixed, mask, lam, bins) if bank is None else MISimilarity(bank[0], bank[1], lam, bins)

    def start_range(self, probs, starts, mi_range):
        """The moving range of every problem: mi_range as given (0 views rendered), else (0, 1.25 x the largest value of the
        problem's view at its start): one render of one view per problem.  Returns the views rendered per problem."""
        if mi_range is not None:
            self.sim.set_range(*mi_range)
            return 0
        c2is, masks, _ = _views(self, probs, list(range(len(probs))), [np.asarray(s, np.float64)[None] for s in starts])
        recs, att, keep = self._render(c2is, masks)
        top = att.reshape(att.shape[0], -1).amax(1)
        seen = top.cpu().numpy()                                    # the copy waits for the render: `keep` lives until then
        del keep
        for i, t in enumerate(seen):
            if not t > 0:
                raise nat.DflError("register: nothing is in view at the start of problem %d (the largest value of its rendered view is %r): "
                                   "similarity='mi' takes its moving range from that view; move the start or give mi_range" % (i, float(t)))
        self.sim.set_range(torch.stack([torch.zeros_like(top), top * 1.25], 1))
        return 1


def _mi_options(similarity, mi_bins, mi_range, segmentation, outline_sets):
    """The checks of similarity='mi', made before anything touches a device: ((Bf, Bm), the range or None), or (None, None) for
    another similarity."""
    if similarity != 'mi':
        if mi_range is not None:
            raise nat.DflError("register: mi_range belongs to similarity='mi', not to similarity=%r" % (similarity,))
        return None, None
    if segmentation is not None or outline_sets is not None:
        raise nat.DflError("register: segmentation and outline_sets belong to similarity='outline', not to similarity='mi'")
    bins = _mi_bins(mi_bins)
    if mi_range is not None:
        try:
            lo, hi = mi_range
        except (TypeError, ValueError):
            raise nat.DflError('register: mi_range = (lo, hi) expected, got %r' % (mi_range,)) from None
        mi_range = _mi_range(lo, hi)
    return bins, mi_range


def _outline_options(geom, segmentation, levels, mask, outline_cap):
    """The checks of register(similarity='outline'), made before anything touches a device."""
    if levels is not None or mask is not None:
        raise nat.DflError("register: similarity='outline' works on one grid and on label maps: levels and mask are not supported with it")
    H, W = geom.grid.H, geom.grid.W
    if not torch.is_tensor(segmentation) or segmentation.dim() != 2 or segmentation.dtype != torch.uint8 or tuple(segmentation.shape) != (H, W):
        got = 'None' if segmentation is None else '%s of %s' % (tuple(getattr(segmentation, 'shape', ())), getattr(segmentation, 'dtype', type(segmentation)))
        raise nat.DflError("register: similarity='outline' needs segmentation = a uint8 label map [%d, %d] on the output grid, got %s" % (H, W, got))
    cap = float(outline_cap)
    if not cap > 0.0 or not np.isfinite(cap):
        raise nat.DflError('register: an outline_cap of %r pixels (finite, positive)' % (outline_cap,))
    return cap


def _outline_sets(geom, moving, outline_sets):
    """outline_sets as given, or one set per label >= 1 found in the masks of the moving objects."""
    if outline_sets is not None:
        return outline_sets
    found = 0
    for m in moving:
        found |= int(geom.objects[m].mask)
    sets = [[l] for l in range(1, 32) if (found >> l) & 1]
    if not sets:
        raise nat.DflError('register: the masks of the moving objects %r hold no label >= 1 to take outlines of' % (tuple(moving),))
    return sets


def _theta_chain(both, piv, xis, moving):
    """_Level._cost_and_moments' rows and pivots, xis [V, 6, 4, 4] -> (cost [V], d cost / d theta [V, 6]), float64 numpy."""
    V = both.shape[0]
    g = both[:, 1:].reshape(V, -1, 12)
    F, Mom = g[:, moving, :3], g[:, moving, 3:].reshape(V, len(moving), 3, 3)       # [V, m, 3], [V, m, 3, 3]
    L, tau = xis[:, :, None, :3, :3], xis[:, :, None, :3, 3]                        # [V, 6, 1, 3, 3], [V, 6, 1, 3]
    lever = (L @ piv[:, None, moving, :, None].astype(np.float64))[..., 0] + tau    # [V, 6, m, 3]
    return both[:, 0], ((Mom[:, None] * L).sum((-1, -2)) + (F[:, None] * lever).sum(-1)).sum(-1)


def _cost_options(refine, refine_tol, similarity, patch_radius, patch_stride, patch_min_count, landmark_weight, patch_weight='uniform'):
    """The checks register() and register_many() make first, before anything touches a device: (the patch parameters --
    radius, stride, min_count, weight -- or None, the landmark weight)."""
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0 or not float(refine_tol) >= 0.0:
        raise nat.DflError('register: refine = %r (an integer, at least 0) and refine_tol = %r (not negative)' % (refine, refine_tol))
    _patch_weight(patch_weight)
    if refine > 0 and similarity == 'patch' and patch_weight == 'uniform':
        raise nat.DflError("register: refine needs the adjoint of the similarity, which similarity='patch' does not have yet "
                           "with patch_weight='uniform' (patch_weight='variance' has it)")
    if similarity not in ('global', 'patch', 'outline', 'mi'):
        raise nat.DflError("register: similarity = %r ('global', 'patch', 'outline' or 'mi')" % (similarity,))
    if similarity != 'patch' and patch_weight != 'uniform':
        raise nat.DflError("register: patch_weight = %r belongs to similarity='patch'; similarity=%r has no patches" % (patch_weight, similarity))
    if similarity == 'outline' and refine > 0:
        raise nat.DflError("register: refine needs the gradient of the cost, which similarity='outline' does not have: the outline cost "
                           "is piecewise constant (DESIGN.md section 26); refine a later stage with similarity='global'")
    patch = _patch_params(patch_radius, patch_stride, patch_min_count) + (patch_weight,) if similarity == 'patch' else None
    landmark_weight = float(landmark_weight)
    if not landmark_weight >= 0.0 or not np.isfinite(landmark_weight):
        raise nat.DflError('register: a landmark_weight of %r (finite, not negative)' % landmark_weight)
    return patch, landmark_weight


def _landmarks_of(landmarks, moving):
    """The usable (X [L, 3], x [2, L]) of landmarks=(X3d, x2d), or None without landmarks."""
    if landmarks is None:
        return None
    if 0 not in tuple(int(m) for m in moving):
        raise nat.DflError('register: the landmark term follows the pelvis (object 0), which moving = %r holds still' % (tuple(moving),))
    try:
        X3d, x2d = landmarks
    except (TypeError, ValueError):
        raise nat.DflError('register: landmarks = (X3d [L, 3], x2d [2, L]) expected') from None
    return _usable_landmarks(X3d, x2d, 'register: landmarks')


def _on_the_gpu(who, volume, tensors):
    """The refusals of host data by register() and register_many(): `tensors` maps what a tensor is called to the tensor."""
    if not isinstance(volume, drr.Volume):
        raise nat.DflError('%s needs a drr.Volume (device tensors; no CPU path)' % who)
    for what, t in tensors.items():
        if not torch.is_tensor(t) or not t.is_cuda:
            raise nat.DflError('%s needs %s on the GPU (no CPU path)' % (who, what))


def _moving_and_population(geom, moving, popsize):
    n_obj = len(geom.objects)
    moving = tuple(int(m) for m in moving)
    if not moving or len(set(moving)) != len(moving) or any(not 0 <= m < n_obj for m in moving):
        raise nat.DflError('register: moving = %r selects no or unknown objects (%d objects)' % (moving, n_obj))
    lam = int(popsize)
    if lam < 4:
        raise nat.DflError('register: a population of %d (at least 4)' % lam)
    return moving, lam


class _Problem:
    """The float64 host side of one registration, shared by register() and register_many(): where the objects start,
    candidates -> the C2I matrices the renderer gets, the landmark term, the motion of the moving objects per unit of
    every parameter, and the Registration of a found theta."""

    def __init__(self, volume_shape, geom, moving, P0, centre, rot_unit, lands, landmark_weight):
        self.geom, self.moving, self.rot_unit = geom, moving, rot_unit
        n_obj = len(geom.objects)
        self.I2P = I2P = np.asarray(geom.I2P, np.float64)
        self.back, Ei = np.linalg.inv(I2P), np.linalg.inv(geom.E)
        self.ctr = volume_centre(volume_shape, I2P) if centre is None else np.asarray(centre, np.float64).reshape(3)
        self.base = base = np.stack([ob.c2i for ob in geom.objects])            # [n_obj, 4, 4]
        if P0 is not None:
            P0 = np.asarray(P0, np.float64).reshape(4, 4)
            for m in moving:
                base[m] = self.back @ P0 @ Ei
        self.masks = [ob.mask for ob in geom.objects]
        self.mv = np.zeros(n_obj, bool)
        self.mv[list(moving)] = True
        self.lands, self.weight = lands, landmark_weight
        self.P_pelvis = I2P @ base[0] @ geom.E if lands is not None and landmark_weight > 0.0 else None    # P = I2P C2I E

    def c2is_of(self, thetas):
        A = self.back[None] @ pose_deltas(thetas, self.ctr, self.rot_unit) @ self.I2P[None]     # [views, 4, 4]
        return np.where(self.mv[None, :, None, None], A[:, None] @ self.base[None], self.base[None])

    def penalty(self, thetas):
        return landmark_penalty(self.geom, pose_deltas(thetas, self.ctr, self.rot_unit) @ self.P_pelvis[None], self.lands[0], self.lands[1],
                                self.weight)

    def with_penalty(self, c, thetas):
        """What the CMA-ES minimises: the similarity costs c of the candidates plus their landmark term."""
        return c if self.P_pelvis is None else c + self.penalty(thetas)

    def xis_of(self, th):
        """[1, 6] -> [1, 6, 4, 4]: the motion of the moving objects in index coordinates per unit of every parameter."""
        return self.back[None, None] @ pose_delta_jacobians(th, self.ctr, self.rot_unit) @ \
            (np.linalg.inv(pose_deltas(th, self.ctr, self.rot_unit)) @ self.I2P[None])[:, None]

    def cost_and_grad(self, c, g, th):
        """(cost, gradient [6]) at th [1, 6] from _theta_chain's (c [1], g [1, 6]): the landmark term joins here."""
        c, g = float(c[0]), g[0]
        if self.P_pelvis is not None:                               # float64 on the host and cheap: central differences
            h = 1e-5
            c += float(self.penalty(th)[0])
            g = g + (self.penalty(th + h * np.eye(6)) - self.penalty(th - h * np.eye(6))) / (2 * h)
        return c, g

    def result(self, mean, similarity_cost, trace, renders, done, theta_cma, refine_cost, gradient_evaluations):
        landmark_cost = 0.0 if self.P_pelvis is None else float(self.penalty(mean[None])[0])
        final_cost = similarity_cost if self.P_pelvis is None else similarity_cost + landmark_cost
        D = pose_delta(mean, self.ctr, self.rot_unit)
        poses = [D @ self.I2P @ self.base[m] @ self.geom.E for m in self.moving]    # P = I2P C2I E
        return Registration(pose=poses[0], poses=poses, theta=mean, delta=D, cost=np.array(trace), final_cost=final_cost,
                            similarity_cost=similarity_cost, landmark_cost=landmark_cost, renders=renders, levels=done, centre=self.ctr,
                            theta_cma=theta_cma, refine_cost=refine_cost, gradient_evaluations=gradient_evaluations)


# ---- the driver: register() is these on one problem and one fixed image, register_many() on n problems and a bank --------------
def _views(level, probs, idx, thetas):
    """What _Level.costs and costs_and_grads get for the points thetas[k] [views_k, 6] of the problems idx[k] of `probs`: the
    C2I matrices of all of them, the object masks, and which fixed image each view is scored against (None without a bank)."""
    fixed_of = np.repeat(np.asarray(idx, np.int32), [len(th) for th in thetas]) if level.sim._bank else None
    return np.concatenate([probs[i].c2is_of(th) for i, th in zip(idx, thetas)]), probs[0].masks, fixed_of


def _search(level, probs, starts, sigma, lam, generations, seed):
    """The CMA-ES of every problem from its start, in lockstep: [CmaResult].  A generation is one render of lam views per
    problem, one similarity launch and one copy."""
    def generation(idx, thetas):
        c = level.costs(*_views(level, probs, idx, thetas))
        return [probs[i].with_penalty(c[k * lam:(k + 1) * lam], th) for k, (i, th) in enumerate(zip(idx, thetas))]

    return lockstep([cma_steps(start, sigma, lam, generations, seed) for start in starts], generation)


def _finish(level, probs, means, refine, refine_tol):
    """bfgs from every problem's mean, in lockstep: [BfgsResult], or [None] * n with refine = 0.  A round is one render of one
    view per problem still running, one adjoint of the similarity, one dfl_drr_pose_grad and one copy."""
    if refine <= 0:
        return [None] * len(probs)

    def round_of_the_finish(idx, thetas):
        ths = [t[None] for t in thetas]
        xis = np.concatenate([probs[i].xis_of(th) for i, th in zip(idx, ths)])
        c2is, masks, fixed_of = _views(level, probs, idx, ths)
        c, g = level.costs_and_grads(c2is, masks, xis, list(probs[0].moving), fixed_of)
        return [probs[i].cost_and_grad(c[k:k + 1], g[k:k + 1], th) for k, (i, th) in enumerate(zip(idx, ths))]

    return lockstep([bfgs_steps(mean, refine, refine_tol) for mean in means], round_of_the_finish)


def _final_costs(level, probs, ends):
    """The similarity cost of every problem at its end point: one render, one similarity launch, one copy."""
    return level.costs(*_views(level, probs, list(range(len(probs))), [end[None] for end in ends]))


def _close(level, probs, means, refine, refine_tol, traces, renders, done):
    """The finish from the means of the search and the final costs, on `level`: every problem's Registration.  traces and
    renders are each problem's best costs and rendered views of the search, `done` the levels it ran."""
    fins = _finish(level, probs, means, refine, refine_tol)
    ends = [mean if fin is None else fin.x for mean, fin in zip(means, fins)]
    last = _final_costs(level, probs, ends)
    out = []
    for i, (prob, fin) in enumerate(zip(probs, fins)):
        evals = 0 if fin is None else fin.evaluations
        out.append(prob.result(ends[i], float(last[i]), traces[i], renders[i] + evals + 1, done, means[i],
                               np.zeros(0) if fin is None else fin.trace, evals))
    return out


def register(volume, geom, fixed, moving=(0, 1, 2), theta0=None, P0=None, levels=None, popsize=16, generations=80, sigma0=2.0,
             step_mm=1.0, mask=None, seed=0, centre=None, rot_unit=ROT_UNIT, crop=0, rot180=False, sigma_shrink=0.5,
             similarity='global', patch_radius=7, patch_stride=4, patch_min_count=None, landmarks=None, landmark_weight=0.0,
             refine=0, refine_tol=1e-4, patch_weight='uniform', segmentation=None, outline_sets=None, outline_cap=32.0, mi_bins=32,
             mi_range=None):
    """Find theta such that the DRR of `volume` under P = D(theta) P0 matches `fixed`.

    moving selects the objects of geom.objects that share the pose under optimisation; the others are rendered at their
    own poses.  Every moving object starts from its own pose in geom.objects, or all of them from P0 (a cam-to-*-vol
    matrix) when it is given; theta0 is the start of the search (default 0).  centre (default: the middle of the
    volume) is the point the rotation turns about.

    levels=None: `fixed` is a float32 [H, W] image on geom.grid (what preprocess_projs gives: it grows with attenuation,
    as the DRR does) and `mask` a uint8 [H, W] or None.  levels=[(factor, generations), ...], coarse to fine: `fixed` is
    the detector's own intensities [rows, cols] (float32 or uint16); every level gets its grid from drr.training_grid(rows,
    cols, crop, factor, rot180) and its fixed image from preprocess_projs at that factor, starts from the previous
    level's mean and multiplies sigma by sigma_shrink; mask is not supported there.

    similarity='global' is one gradient-NCC over all counted pixels (Similarity); 'patch' is the mean over patches of
    radius patch_radius every patch_stride pixels with at least patch_min_count counted pixels (PatchSimilarity; with
    levels the same numbers apply on every level's own grid).  landmarks=(X3d [L, 3], x2d [2, L]) with landmark_weight w
    adds landmark_penalty of the pelvis pose D(theta) P_pelvis to every cost (object 0 must move; not with levels).

    refine=K > 0 finishes with at most K iterations of bfgs() from the CMA-ES mean, on the last level's grid, with the
    gradient of the frozen-sampling renderer and the adjoint of the global similarity (the landmark
    term joins with central differences of its host function); refine_tol is the step length that ends it.  The result
    never costs more than the CMA-ES mean (Registration.theta_cma).  generations=0 with refine=K refines theta0 alone.
    similarity='patch' with the default patch_weight='uniform' is refused together with refine.

    patch_weight='variance' (with similarity='patch') weighs every patch by the energy of its fixed
    gradient, which quiets the background patches of a preprocessed projection, and has an adjoint: refine=K works with it.

    similarity='outline'  matches bone outlines instead of intensities: `segmentation` is a uint8
    label map [H, W] on geom.grid on the GPU (a row of 'nn-segs', best cleaned: labels.clean), `fixed` may be None and is
    not read.  Every generation is one exact render that writes the winner-takes-all label_map of every candidate, the
    boundary distance maps of those (dfl_label_edt), one dfl_sim_outline and one copy of lambda doubles (OutlineSimilarity).
    The cost is the truncated chamfer distance between the boundaries of every set of outline_sets (what labels.edt takes;
    default: one set per label >= 1 in the masks of the moving objects), truncated at outline_cap pixels, 0 .. 1.  It sees
    a pose from half an image away and needs no landmarks, but it is piecewise constant: no refine, no levels, no mask,
    and no motion below a pixel -- a start and a coarse stage for the intensity costs, not a replacement.  The landmark
    term adds to it as to the others.

    similarity='mi'  is the negative mutual information between the intensities of the DRR and of
    `fixed` (MISimilarity): it needs no known intensity mapping of the fixed image -- any monotone or even non-monotone
    look-up table gives the same cost up to binning -- and no edges.  mi_bins is the number of bins, an integer or (Bf, Bm),
    2..64.  mi_range=(lo, hi) is the range of the moving intensities the Bm bins span; None takes (0, 1.25 x the largest
    value of the view rendered at the start), per level: one more render, counted in Registration.renders, and a start with
    nothing in view is refused.  mask, levels, landmarks and refine=K work with it; patch_weight, segmentation and outline_sets
    do not belong to it.
    """
    patch, landmark_weight = _cost_options(refine, refine_tol, similarity, patch_radius, patch_stride, patch_min_count, landmark_weight,
                                           patch_weight)
    mi_bins, mi_range = _mi_options(similarity, mi_bins, mi_range, segmentation, outline_sets)
    outline = similarity == 'outline'
    if outline:
        outline_cap = _outline_options(geom, segmentation, levels, mask, outline_cap)
    elif segmentation is not None or outline_sets is not None:
        raise nat.DflError("register: segmentation and outline_sets belong to similarity='outline', not to similarity=%r" % (similarity,))
    if landmarks is not None and levels is not None:
        raise nat.DflError('register: landmarks belong to one grid; they are not supported together with levels')
    lands = _landmarks_of(landmarks, moving)
    _on_the_gpu('register', volume, {'the segmentation': segmentation} if outline else {'the fixed image': fixed})
    moving, lam = _moving_and_population(geom, moving, popsize)
    theta0 = np.zeros(6) if theta0 is None else np.asarray(theta0, np.float64).reshape(6)
    prob = _Problem(volume.shape, geom, moving, P0, centre, rot_unit, lands, landmark_weight)

    if outline:
        plan = [(None, int(generations), geom.grid, None)]
    elif levels is None:
        plan = [(None, int(generations), geom.grid, _device_image(fixed, 'the fixed image', 2))]
    else:
        if mask is not None:
            raise nat.DflError('register: a mask belongs to one grid; it is not supported together with levels')
        px = _device_image(fixed, 'the detector image', 2, (torch.float32, torch.uint16))
        rows, cols = (int(s) for s in px.shape)
        Kinv = np.linalg.inv(geom.K)
        plan = []
        for factor, gens in levels:
            G, (H, W) = drr.training_grid(rows, cols, crop, int(factor), bool(rot180))
            if patch is not None and min(H, W) - 2 < 2 * patch[0] + 1:
                raise nat.DflError('register: level %d (factor %d) has a grid of %d x %d, too small for one patch of side %d'
                                   % (len(plan), int(factor), H, W, 2 * patch[0] + 1))
            img = preprocess.preprocess_projs(px[None], [bool(rot180)], int(crop), int(factor))[0]
            plan.append((int(factor), int(gens), drr.Grid(-Kinv @ G, H, W), img))
        if not plan:
            raise nat.DflError('register: an empty list of levels')
    mean, sigma, trace, renders, done = theta0, float(sigma0), [], 0, []
    for k, (factor, gens, grid, img) in enumerate(plan):
        level = _OutlineLevel(volume, grid, segmentation, _outline_sets(geom, moving, outline_sets), outline_cap, lam, step_mm) if outline \
            else _MILevel(volume, grid, img, mask, lam, step_mm, mi_bins) if mi_bins is not None \
            else _Level(volume, grid, img, mask, lam, step_mm, patch)
        if mi_bins is not None:
            renders += level.start_range([prob], [mean], mi_range)
        res = _search(level, [prob], [mean], sigma, lam, gens, seed + k)[0]
        mean, sigma = res.mean, sigma * float(sigma_shrink)
        trace.extend(res.trace.tolist())
        renders += res.evaluations
        done.append((factor, gens, grid.H, grid.W))
    return _close(level, [prob], [mean], int(refine), float(refine_tol), [trace], [renders], done)[0]


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64))


def default_max_views(H, W):
    """The most views register_many renders at once by default: at most 65535, and at most 1 GiB of float32 pixels."""
    return max(1, min(65535, (1 << 30) // (4 * int(H) * int(W))))


def register_many(volume, geoms, fixed, moving=(0, 1, 2), theta0=None, P0=None, popsize=16, generations=80, sigma0=2.0, step_mm=1.0,
                  masks=None, seed=0, centre=None, rot_unit=ROT_UNIT, similarity='global', patch_radius=7, patch_stride=4,
                  patch_min_count=None, landmarks=None, landmark_weight=0.0, refine=0, refine_tol=1e-4, max_views=None,
                  patch_weight='uniform', mi_bins=32, mi_range=None, **unknown):
    """register() for N projections of one volume at once: [Registration] * N.

    geoms is a list of N drr.Geometry that share the output grid, K, I2P and the object masks (each has its own object
    poses and may have its own E); fixed is float32 [N, H, W] on the GPU, masks uint8 [N, H, W] or None; theta0 [N, 6],
    P0 [N, 4, 4] and landmarks (a list of N entries, (X3d, x2d) or None) are per problem or None; everything else is one
    value for all.  Problem i is register(volume, geoms[i], fixed[i], theta0=theta0[i], P0=P0[i], mask=masks[i],
    landmarks=landmarks[i], seed=seed, ...), and its theta, cost, theta_cma, refine_cost, final_cost, similarity_cost,
    landmark_cost, pose, renders and gradient_evaluations have that call's bytes.

    The device works on all running problems at once: a generation is one render of popsize views per problem and one
    similarity launch against the bank of fixed images (SimilarityBank, PatchSimilarityBank); a round of the finish is one
    render of one view per problem still running, one dfl_sim_bank_gradncc_bwd (with patch_weight='variance': one
    dfl_sim_patch_eval) and one dfl_drr_pose_grad.  The float64
    host work is done problem by problem with the functions register() uses.  max_views caps the views of one render
    (default: default_max_views); problems are processed in chunks of max_views // popsize, which changes no result.
    There is no coarse-to-fine here (no levels).  similarity='mi' works as in register(): with mi_range=None the start views of a
    chunk of problems are one render and their ranges one [F, 2] tensor on the device."""
    if unknown:
        raise nat.DflError('register_many: no argument %s (levels: there is no coarse-to-fine here; register() has it)'
                           % ', '.join(sorted(unknown)))
    if similarity == 'outline':
        raise nat.DflError("register_many: similarity='outline' is not supported here: register() has it, one projection at a time "
                           "(dfl_sim_outline takes fixed_of, but the driver for a bank of segmentations is not written)")
    patch, landmark_weight = _cost_options(refine, refine_tol, similarity, patch_radius, patch_stride, patch_min_count, landmark_weight,
                                           patch_weight)
    mi = _mi_options(similarity, mi_bins, mi_range, None, None)
    try:
        geoms = list(geoms)
    except TypeError:
        raise nat.DflError('register_many: geoms is a list of drr.Geometry, one per problem') from None
    N = len(geoms)
    if N < 1:
        raise nat.DflError('register_many: no problem (N = 0)')

    def per_problem(what, value, shape):
        if value is None:
            return [None] * N
        if shape is not None:
            value = np.asarray(value, np.float64)
            if value.shape != (N,) + shape:
                raise nat.DflError('register_many: %s has shape %s for %d problems: %s expected' % (what, value.shape, N, (N,) + shape))
        elif not isinstance(value, (list, tuple)) or len(value) != N:
            raise nat.DflError('register_many: %s is a list of %d entries, one per problem' % (what, N))
        return list(value)

    theta0s, P0s = per_problem('theta0', theta0, (6,)), per_problem('P0', P0, (4, 4))
    lands = [_landmarks_of(l, moving) for l in per_problem('landmarks', landmarks, None)]
    images = {what: t for what, t in (('fixed', fixed), ('masks', masks)) if t is not None}
    for what, t in images.items():
        if not hasattr(t, 'shape') or len(t.shape) != 3 or int(t.shape[0]) != N:
            raise nat.DflError('register_many: %s is [N, H, W] with N = %d problems, got %s' % (what, N, tuple(getattr(t, 'shape', ()))))
    g0 = geoms[0]
    for i, g in enumerate(geoms):
        if not isinstance(g, drr.Geometry):
            raise nat.DflError('register_many: geoms[%d] is no drr.Geometry' % i)
        if not (_same(g.grid.Q, g0.grid.Q) and (g.grid.H, g.grid.W) == (g0.grid.H, g0.grid.W) and _same(g.K, g0.K) and _same(g.I2P, g0.I2P) and
                [ob.mask for ob in g.objects] == [ob.mask for ob in g0.objects]):
            raise nat.DflError('register_many: geoms[%d] differs from geoms[0] in the grid, K, I2P or the object masks, which all '
                               'problems share' % i)
    moving, lam = _moving_and_population(g0, moving, popsize)
    H, W = g0.grid.H, g0.grid.W
    cap = default_max_views(H, W) if max_views is None else max_views
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < lam or cap > 65535:
        raise nat.DflError('register_many: max_views = %r (an integer from popsize = %d to 65535)' % (max_views, lam))
    _on_the_gpu('register_many', volume, images)
    fixed = _device_image(fixed, 'the fixed images', 3)
    if tuple(fixed.shape[1:]) != (H, W):
        raise nat.DflError('register: the fixed image is %s, the output grid %d x %d' % (tuple(fixed.shape[1:]), H, W))
    probs = [_Problem(volume.shape, g, moving, P0s[i], centre, rot_unit, lands[i], landmark_weight) for i, g in enumerate(geoms)]
    starts = [np.zeros(6) if t is None else t for t in theta0s]
    per, out = max(1, int(cap) // lam), []
    for lo in range(0, N, per):
        hi = min(N, lo + per)
        out.extend(_register_chunk(volume, g0.grid, probs[lo:hi], starts[lo:hi], fixed[lo:hi], None if masks is None else masks[lo:hi],
                                   lam, int(generations), float(sigma0), step_mm, seed, patch, int(refine), float(refine_tol), mi))
    return out


def _register_chunk(volume, grid, probs, starts, fixed, masks, lam, generations, sigma0, step_mm, seed, patch, refine, refine_tol,
                    mi=(None, None)):
    """register_many for problems whose lambda candidates fit into one render together."""
    first = 0
    if mi[0] is not None:
        level = _MILevel(volume, grid, None, None, len(probs) * lam, step_mm, mi[0], bank=(fixed, masks))
        first = level.start_range(probs, starts, mi[1])
    else:
        level = _Level(volume, grid, None, None, len(probs) * lam, step_mm, patch, bank=(fixed, masks))
    cma = _search(level, probs, starts, sigma0, lam, generations, seed)
    return _close(level, probs, [r.mean for r in cma], refine, refine_tol, [r.trace.tolist() for r in cma], [first + r.evaluations for r in cma],
                  [(None, generations, grid.H, grid.W)])
